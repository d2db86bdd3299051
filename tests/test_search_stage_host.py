"""-m "not gpu": a search stage is written down once (pipeline.STAGES) — how the test quarter goes through each of them
(ML2PN.search_plan, a pure function), what a negative option is told under every public name, and which stage has the lane form only."""
import pytest

COUNTERS = ("rounds", "pair_moves", "converged")
WALK = ("steps", "best_step", "stalled")

# (stage, its options' values, from every start) -> (pipeline function, its option kwargs, file, per-problem fields of extra, settings of extra)
PLANS = [
    ("descend", (), False, ("descend", {}, "ML+2PN+descent.txt", (), {})),
    ("descend_pairs", (3,), False, ("descend_pairs", {"max_rounds": 3}, "ML+2PN+pairs.txt", COUNTERS, {})),
    ("descend_pairs_windowed", (3, 2), False,
     ("descend_pairs_windowed", {"max_rounds": 3, "max_span": 2}, "ML+2PN+pairs.txt", COUNTERS, {"span": 2})),
    ("descend_pairs_shortlist", (3, 2, 5), False,
     ("descend_pairs_shortlist", {"max_rounds": 3, "max_span": 2, "max_rank": 5}, "ML+2PN+pairs.txt", COUNTERS, {"span": 2, "top": 5})),
    ("descend_tabu", (8, 4), False,
     ("descend_tabu", {"max_steps": 8, "tenure": 4}, "ML+2PN+tabu.txt", WALK, {"tabu_steps": 8, "tenure": 4})),
    ("descend", (), True, ("descend_starts", {}, "ML+2PN+multistart.txt", (), {})),
    ("descend_pairs", (3,), True, ("descend_starts_pairs", {"pair_rounds": 3}, "ML+2PN+multistart+pairs.txt", COUNTERS, {})),
    # from every start a span without a rank runs the full sweep and is still written
    ("descend_pairs_windowed", (3, 2), True, ("descend_starts_pairs", {"pair_rounds": 3}, "ML+2PN+multistart+pairs.txt", COUNTERS, {"span": 2})),
    ("descend_pairs_shortlist", (3, 2, 5), True,
     ("descend_starts_pairs_shortlist", {"pair_rounds": 3, "pair_span": 2, "pair_rank": 5}, "ML+2PN+multistart+pairs.txt", COUNTERS,
      {"span": 2, "top": 5})),
    ("descend_tabu", (8, 4), True,
     ("descend_starts_tabu", {"max_steps": 8, "tenure": 4}, "ML+2PN+multistart+tabu.txt", WALK, {"tabu_steps": 8, "tenure": 4})),
]


@pytest.mark.parametrize("name,values,multi,want", PLANS)
def test_plan_of_the_test_quarter(name, values, multi, want):
    import inspect
    from gnnpn_sc_amd import ML2PN
    from gnnpn_sc_amd import pipeline as pl
    function, options, file, fields, settings = ML2PN.search_plan(pl.STAGES[name].bind(*values), multi)
    assert (function, options, file, tuple(fields), settings) == want
    assert list(settings) == list(want[4])                                    # extra's keys in the artefact's order
    taken = inspect.signature(getattr(pl, function)).parameters              # the function exists and takes these options
    assert set(options) <= set(taken) and {"max_sweeps", "reduct", "min_cost"} <= set(taken)
    assert "starts" in taken if multi else "out" in taken


def test_the_table_has_the_five_stages():
    from gnnpn_sc_amd import ML2PN, ops
    from gnnpn_sc_amd import pipeline as pl
    assert list(pl.STAGES) == ["descend", "descend_pairs", "descend_pairs_windowed", "descend_pairs_shortlist", "descend_tabu"]
    assert (pl.ONE_SWAP, pl.PAIRS, pl.PAIRS_WINDOWED, pl.PAIRS_SHORTLIST, pl.TABU) == tuple(pl.STAGES.values())
    assert set(ML2PN.RUNS) == set(pl.STAGES)
    for name, stage in pl.STAGES.items():
        assert stage.method == name and stage.values == () and callable(getattr(ops.SearchTables, name))
        assert callable(getattr(pl, name)) and callable(getattr(pl, stage.starts[0])) and callable(getattr(ML2PN, ML2PN.RUNS[name][2]))
        assert len(ML2PN.RUNS[name][0]) == len(stage.options) == stage.refusal.count("{}")
    assert pl.ONE_SWAP.options == ()                                          # nothing of one-swap descent can be negative but max_sweeps


# (stage, keyword arguments with a negative option, the parent's sentence behind "<who>: ")
NEGATIVE = [
    ("descend_pairs", {"max_rounds": -1}, "the number of rounds must be >= 0, got -1"),
    ("descend_pairs_windowed", {"max_span": -1}, "the number of rounds and the span must be >= 0, got 4 and -1"),
    ("descend_pairs_windowed", {"max_rounds": -3, "max_span": 2}, "the number of rounds and the span must be >= 0, got -3 and 2"),
    ("descend_pairs_shortlist", {"max_rank": -1}, "the number of rounds, the span and the rank must be >= 0, got 4, 0 and -1"),
    ("descend_pairs_shortlist", {"max_rounds": 2, "max_span": -5, "max_rank": 1},
     "the number of rounds, the span and the rank must be >= 0, got 2, -5 and 1"),
    ("descend_tabu", {"max_steps": -1, "tenure": 2}, "the number of steps and the tenure must be >= 0, got -1 and 2"),
    ("descend_tabu", {"max_steps": 8, "tenure": -2}, "the number of steps and the tenure must be >= 0, got 8 and -2"),
]
# the descend_starts* variants: (function, who says so, keyword arguments, sentence); descend_starts_pairs speaks as descend_pairs
NEGATIVE_STARTS = [
    ("descend_starts_pairs", "descend_pairs", {"pair_rounds": -2}, "the number of rounds must be >= 0, got -2"),
    ("descend_starts_pairs_shortlist", "descend_starts_pairs_shortlist", {"pair_span": -1},
     "the number of rounds, the span and the rank must be >= 0, got 4, -1 and 0"),
    ("descend_starts_pairs_shortlist", "descend_starts_pairs_shortlist", {"pair_rounds": -1, "pair_rank": 3},
     "the number of rounds, the span and the rank must be >= 0, got -1, 0 and 3"),
    ("descend_starts_tabu", "descend_starts_tabu", {"max_steps": -4, "tenure": 1}, "the number of steps and the tenure must be >= 0, got -4 and 1"),
    ("descend_starts_tabu", "descend_starts_tabu", {"max_steps": 4, "tenure": -1}, "the number of steps and the tenure must be >= 0, got 4 and -1"),
]


def _refused(f, kw):
    """The message with which ``f`` refuses ``kw`` — before it looks at the services, the batch or the rows (None each)."""
    from gnnpn_sc_amd import ops
    with pytest.raises(ops.GnnpnError) as e:
        f(None, None, None, **kw)
    return str(e.value)


@pytest.mark.parametrize("name,kw,sentence", NEGATIVE)
def test_a_negative_option_is_told_the_stages_sentence(name, kw, sentence):
    from gnnpn_sc_amd import pipeline as pl
    assert _refused(getattr(pl, name), kw) == f"{name}: {sentence}"
    assert _refused(lambda *a, **k: getattr(pl.ML2PNPipeline, name)(None, *a, **k), kw) == f"{name}: {sentence}"


@pytest.mark.parametrize("name,who,kw,sentence", NEGATIVE_STARTS)
def test_a_negative_option_from_every_start(name, who, kw, sentence):
    from gnnpn_sc_amd import pipeline as pl
    assert _refused(getattr(pl, name), kw) == f"{who}: {sentence}"
    assert _refused(lambda *a, **k: getattr(pl.ML2PNPipeline, name)(None, *a, **k), kw) == f"{who}: {sentence}"


class _Tables(dict):
    """Tables that launch nothing: every SearchTables method records its call."""
    def __getattr__(self, name):
        return lambda *a: self["calls"].append((name, a)) or {}


@pytest.mark.parametrize("name,values", [(p[0], p[1]) for p in PLANS[:5]])
def test_only_descend_pairs_is_refused_at_65_slots(name, values):
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd import pipeline as pl
    tabs = _Tables(max_slots=65, max_cand=100, n_slots="n", calls=[])
    stage = pl.STAGES[name].bind(*values)
    if name == "descend_pairs":
        with pytest.raises(ops.GnnpnError) as e:
            pl._search_tables(tabs, 16, stage)
        assert str(e.value) == ("descend_pairs: a problem of the batch has 65 slots; the pair sweep takes at most 64 per problem "
                                "(descend runs one-swap descent at any slot count)")
        assert tabs["calls"] == []                                            # before any launch
    else:
        assert pl._search_tables(tabs, 16, stage) == {"n_slots": "n"} and tabs["calls"] == [(name, (16, *values))]
    tabs = _Tables(max_slots=64, max_cand=100, n_slots="n", calls=[])
    pl._search_tables(tabs, 7, stage)
    assert tabs["calls"] == [(name, (7, *values))]


def test_infer_preconditions_name_their_caller():
    from gnnpn_sc_amd import ML2PN
    call = lambda f, **kw: f("QWS", None, None, None, 3, **kw)      # noqa: E731
    cases = [
        (ML2PN.infer, {"pair_rounds": 2}, "ML2PN.infer: pair_rounds needs descend and at least one round"),
        (ML2PN.infer, {"descend": 4, "pair_rounds": 0}, "ML2PN.infer: pair_rounds needs descend and at least one round"),
        (ML2PN.infer_services, {"woa": {}, "pair_rounds": 2}, "ML2PN.infer: pair_rounds needs descend and at least one round"),
        (ML2PN.infer, {"all_starts": True, "descend": 4}, "ML2PN.infer: all_starts needs samples > 1 and descend"),
        (ML2PN.infer_pairs_windowed, {"pair_span": -1}, "ML2PN.infer_pairs_windowed: pair_span needs descend, at least one round and a span >= 0"),
        (ML2PN.infer_pairs_windowed, {"descend": None}, "ML2PN.infer_pairs_windowed: pair_span needs descend, at least one round and a span >= 0"),
        (ML2PN.infer_services, {"descend": 4, "pair_span": 2},
         "ML2PN.infer_services: pair_span needs descend, at least one round and a span >= 0"),
        (ML2PN.infer_pairs_shortlist, {"pair_rank": None},
         "ML2PN.infer_pairs_shortlist: pair_rank needs descend, at least one round, a span >= 0 and a rank >= 0"),
        (ML2PN.infer_services, {"descend": 4, "pair_rounds": 2, "pair_rank": 1},
         "ML2PN.infer_services: pair_rank needs descend, at least one round, a span >= 0 and a rank >= 0"),
        (ML2PN.infer_tabu, {"tabu_steps": -1, "tenure": 2}, "ML2PN.infer_tabu: tabu_steps needs descend, a number of steps >= 0 and a tenure >= 0"),
        (ML2PN.infer_tabu, {"tabu_steps": 4, "tenure": -1}, "ML2PN.infer_tabu: tabu_steps needs descend, a number of steps >= 0 and a tenure >= 0"),
        (ML2PN.infer_services, {}, "ML2PN.infer_services: needs descend or woa (the services of a searched composition)"),
    ]
    for f, kw, message in cases:
        with pytest.raises(ValueError) as e:
            call(f, **kw)
        assert str(e.value) == message, kw
    assert ML2PN.stage_given() == "descend" and ML2PN.stage_given(4) == "descend_pairs" and ML2PN.stage_given(4, 0) == "descend_pairs_windowed"
    assert ML2PN.stage_given(4, None, 2) == ML2PN.stage_given(4, 1, 2) == "descend_pairs_shortlist"
    assert ML2PN.stage_given(tabu_steps=0) == "descend_tabu"
