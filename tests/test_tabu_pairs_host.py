"""-m "not gpu": the tabu walk over pair moves (gnnpn_descend_tabu_pairs_ragged_f64, ops.descend_tabu_pairs_ragged,
SearchTables.descend_tabu_pairs, pipeline.descend_tabu_pairs / descend_starts_tabu_pairs, ML2PN.infer_tabu_pairs, `main.py ... --descend
--tabu --pair-moves`) rejects bad arguments and host tensors before any launch, and the plain-Python reference the GPU tests compare
with (tests/tabu_pairs_reference.py) has the properties that make those comparisons meaningful."""
import ctypes
import inspect
import os

import pytest
import torch

import descent_reference as ref
import pair_descent_reference as pref
import pair_shortlist_reference as sref
import pair_window_reference as wref
import tabu_pairs_reference as tpref
import tabu_reference as tref
from conftest import ROOT

P = ctypes.c_void_p(64)          # a non-null stand-in: every call below fails before it is dereferenced
SHARED = ("best_fitness", "start_fitness", "best_pos", "best_rows", "sweeps", "moves")
WALK = SHARED + ("history", "walk", "steps", "best_step", "stalled")


def _all_runs():
    """(case name, table, its keyword arguments, reference run) of every case of the table."""
    for name, (tables, kw, _wide) in tpref.CASES.items():
        for tab, r in zip(tables, tpref.case_want(name)):
            yield name, tab, kw, r


# ---- the reference ----------------------------------------------------------------------------------------------------------------------

def test_the_wall_is_crossed_in_one_step():
    tab = pref.wall_problem()
    r = tpref.descend_tabu_pairs(*tab, max_steps=1, tenure=2, max_rank=2, with_trace=True)
    assert r["pair_steps"] == 1 and r["steps"] == 1 and r["best_pos"] == [1, 1] and len(r["trace"][0][1]) == 2
    assert r["best_fitness"] == pref.descend_pairs(*tab)["best_fitness"] == 0.55
    assert r["best_fitness"] < tref.descend_tabu(*tab, max_steps=1, tenure=2)["best_fitness"] == 1.5
    assert tref.descend_tabu(*tab, max_steps=2, tenure=2)["best_fitness"] == 0.55          # the tabu walk needs its second step


def test_without_a_pair_it_is_the_tabu_walk():
    for tab in (tref.one_slot(), tref.single_rows()):
        for rank in (0, 2):
            r = tpref.descend_tabu_pairs(*tab, max_steps=6, tenure=2, max_rank=rank)
            t = tref.descend_tabu(*tab, max_steps=6, tenure=2)
            assert {k: r[k] for k in WALK} == {k: t[k] for k in WALK} and r["pair_steps"] == 0


def test_no_steps_is_one_swap_descent():
    tables = sref._seeds_tables()
    assert len(tables) == 20
    for tab, r in zip(tables, tpref.seeds_runs(0, 3, 2)):
        one = ref.descend(*tab)
        assert {k: r[k] for k in SHARED} == {k: one[k] for k in SHARED}
        assert r["history"] == [one["best_fitness"]] and r["walk"] == [] and (r["steps"], r["best_step"], r["stalled"], r["pair_steps"]) == (0, 0, 0, 0)


def test_never_above_one_swap_descent_and_the_pairs_matter():
    one = {}
    for name, tab, kw, r in _all_runs():
        key = (id(tab), kw.get("max_sweeps", 16))
        if key not in one:
            one[key] = ref.descend(*tab, max_sweeps=kw.get("max_sweeps", 16))["best_fitness"]
        assert not r["best_fitness"] > one[key], name
        assert r["best_fitness"] <= r["history"][-1] and r["pair_steps"] <= r["steps"], name
        assert (r["best_fitness"] < r["history"][-1]) <= (r["polished"][1] > 0), name              # strict only where the polish moved
        assert r["polished"][0] == (r["steps"] > 0 and r["best_step"] == r["steps"] and not r["stalled"]), name
    tabu = [r["best_fitness"] for r in tref.seeds_runs(32, 3)]
    for rank in (2, 0):
        runs = tpref.seeds_runs(32, 3 if rank else 0, rank)
        assert sum(r["pair_steps"] for r in runs) > 0
        if rank:                                                        # same tenure: never above the walk over single swaps on these tables
            assert not any(r["best_fitness"] > t for r, t in zip(runs, tabu)) and any(r["best_fitness"] < t for r, t in zip(runs, tabu))


def test_no_component_returns_within_the_tenure():
    for name, _tab, kw, r in _all_runs():
        assert tpref.returns_within_tenure(r, kw["tenure"]) == [], name
    assert any(tpref.returns_within_tenure(r, 3) for r in tpref.seeds_runs(32, 0, 0))      # the check bites: without a tenure the walk returns
    assert any(tabu for r in tpref.seeds_runs(32, 3, 2) for _t, parts, _f, _b in r["trace"] for *_x, tabu in parts) or \
        any(tabu for r in tpref.seeds_runs(32, 3, 4, 1) for _t, parts, _f, _b in r["trace"] for *_x, tabu in parts)      # aspiration admits a tabu move


def test_a_single_wins_over_an_equal_pair_and_the_lowest_pair_among_pairs():
    """duplicated_rows(): rows that stand twice give equal merits.  Every step's choice is recomputed here from the contract's order:
    over all admissible moves the smallest merit, singles before pairs, then the lowest key."""
    cats, bounds, start = sref.duplicated_rows()
    r = tpref.descend_tabu_pairs(cats, bounds, start, max_steps=6, tenure=2, max_rank=0, with_trace=True)
    assert r["steps"] == 6
    cur = list(ref.descend(cats, bounds, start)["best_pos"])
    T, expire, best_f, saw_tie = len(cats), {}, ref.descend(cats, bounds, start)["best_fitness"], False
    for t, parts, f, best_before in r["trace"]:
        assert best_before == best_f
        moves = []
        for j in range(T):
            for c in range(len(cats[j])):
                if c != cur[j]:
                    rows = [cats[s][c if s == j else cur[s]] for s in range(T)]
                    moves.append((ref.merit(rows, bounds), 0, (j, c), ((j, c),)))
        for i in range(T):
            for j in range(i + 1, T):
                for a in range(len(cats[i])):
                    for b in range(len(cats[j])):
                        if a != cur[i] and b != cur[j]:
                            rows = [cats[s][a if s == i else b if s == j else cur[s]] for s in range(T)]
                            moves.append((ref.merit(rows, bounds), 1, (i, j, a, b), ((i, a), (j, b))))
        ok = [m for m in moves if m[0] == m[0] and (all(expire.get(p, 0) < t for p in m[3]) or m[0] < best_f)]
        win = min(ok, key=lambda m: m[:3])
        saw_tie |= sum(m[0] == win[0] for m in ok) > 1
        assert f == win[0] and tuple((j, c) for j, c, _was, _tabu in parts) == win[3], t
        for j, c in win[3]:
            expire[j, cur[j]] = t + 2
            cur[j] = c
        best_f = min(best_f, f)
    assert saw_tie
    twice = pref.wall_problem(twice=True)                               # four pairs tie: the lowest (a, b) is taken
    w = tpref.descend_tabu_pairs(*twice, max_steps=1, tenure=2, max_rank=0, with_trace=True)
    assert w["pair_steps"] == 1 and w["best_pos"] == [1, 1]


def test_a_nan_merit_is_never_taken_and_ranks_last():
    cats, bounds, start = sref.nan_row_problem()
    r = tpref.descend_tabu_pairs(cats, bounds, start, max_steps=6, tenure=2, max_rank=2, with_trace=True)
    assert r["steps"] == 6 and all(f == f for f in r["walk"])
    assert not any((j, c) in ((1, 0), (1, 2)) for _t, parts, *_ in r["trace"] for j, c, *_x in parts)
    lists = pref.shortlists(cats, bounds, list(r["best_pos"]), 1)
    assert lists[1] not in ([0], [2])                                   # the NaN rows of slot 1 rank behind its numbers


def test_the_gpu_cases_are_not_vacuous():
    """What each GPU case is there for: pair steps in both forms, a pair 37 slots apart, pairs across two leaves of np.sum and across the
    parting node above the leaves, ranking in chunks beyond the wave and the workgroup, a stall, a polish that moves."""
    (r,) = tpref.case_want("planted65")
    assert r["pair_steps"] >= 1 and any(len(p) == 2 and p[1][0] - p[0][0] == 37 for _t, p, *_ in r["trace"])
    (r,) = tpref.case_want("planted129")
    assert r["pair_steps"] >= 1 and any(len(p) == 2 and wref.leaf_of(129, p[0][0]) != wref.leaf_of(129, p[1][0]) for _t, p, *_ in r["trace"])
    (r,) = tpref.case_want("planted257")
    assert r["pair_steps"] >= 1 and any(len(p) == 2 and wref.leaf_of(257, p[0][0]) != wref.leaf_of(257, p[1][0]) for _t, p, *_ in r["trace"])
    assert r["best_fitness"] < tref.descend_tabu(*tpref.CASES["planted257"][0][0], max_steps=6, tenure=4)["best_fitness"]
    (r,) = tpref.case_want("wall131")
    assert (r["steps"], r["best_step"], r["pair_steps"], r["stalled"]) == (1, 1, 1, 1) and r["best_fitness"] < 1.0
    assert wref.leaf_of(131, 63) != wref.leaf_of(131, 64)
    assert [len(c) for c in tpref.CASES["long"][0][0][0]] == [139, 70, 5] and tpref.CASES["long"][1]["max_rank"] == 8
    assert max(len(c) for c in tpref.CASES["long_wide"][0][0][0]) == 300
    assert all(len(t[0]) == 64 for t in tpref.CASES["t64"][0]) and all(r["pair_steps"] >= 1 for r in tpref.case_want("t64"))
    small = tpref.case_want("small")
    assert [r["stalled"] for r in small] == [0, 0, 0, 1, 1] and small[0]["pair_steps"] >= 1 and small[4]["pair_steps"] == 1
    assert any(r["polished"][1] > 0 for r in tpref.case_want("seeds_s2_t3_r2_w0"))
    assert sum(r["pair_steps"] for r in tpref.case_want("seeds_s32_t3_r4_w1")) > 0 and sum(r["pair_steps"] for r in tpref.case_want("seeds_s32_t0_r0_w0")) > 0


# ---- the C entry ------------------------------------------------------------------------------------------------------------------------

def _entry():
    from gnnpn_sc_amd import _lib
    lib = _lib.load()
    names = ("prob_ptr", "cand_ptr", "cand", "bounds", "start_pos", "best_fitness", "start_fitness", "best_pos", "best_rows", "history",
             "sweeps", "moves", "walk", "steps", "best_step", "stalled", "pair_steps")

    def call(B=3, n_lists=12, max_slots=5, max_cand=20, max_sweeps=4, max_steps=8, tenure=2, max_span=0, max_rank=2, wide=0, **null):
        a = {n: (None if n in null else P) for n in names}
        return lib.gnnpn_descend_tabu_pairs_ragged_f64(
            B, a["prob_ptr"], n_lists, max_slots, max_cand, a["cand_ptr"], a["cand"], a["bounds"], a["start_pos"], max_sweeps, max_steps,
            tenure, max_span, max_rank, wide, a["best_fitness"], a["start_fitness"], a["best_pos"], a["best_rows"], a["history"], a["sweeps"],
            a["moves"], a["walk"], a["steps"], a["best_step"], a["stalled"], a["pair_steps"], None)
    return _lib, lib, names, call


def test_entry_rejects_bad_arguments():
    _lib, lib, names, call = _entry()
    for n in names:
        if n != "best_rows":                                # the one optional output
            assert call(**{n: True}) == -1 and b"null" in lib.gnnpn_last_error(), n
    for kw in ({"B": -1}, {"n_lists": -1}, {"max_slots": 0}, {"max_sweeps": -1}, {"max_steps": -1}, {"tenure": -1}, {"max_span": -1},
               {"max_rank": -1}):
        assert call(**kw) == -1 and b"bad argument" in lib.gnnpn_last_error(), kw
    for kw in ({}, {"wide": 1}, {"max_slots": 100}):        # the tabu table and the merit buffer are sized by max_cand in both forms
        assert call(max_cand=0, **kw) == _lib.E_UNSUP and b"max_cand" in lib.gnnpn_last_error(), kw
    assert call(B=0) == 0 and call(B=0, prob_ptr=True, pair_steps=True, max_slots=5000) == 0      # an empty batch launches nothing
    assert "gnnpn_descend_tabu_pairs_ragged_f64" in _lib.EXPORTS
    assert lib.gnnpn_abi_version() == 9
    with open(os.path.join(ROOT, "include", "gnnpn_hip.h")) as f:
        header = f.read()
    assert "int gnnpn_descend_tabu_pairs_ragged_f64(" in header and "#define GNNPN_ABI_VERSION 9" in header
    at = header.index("int gnnpn_descend_tabu_pairs_ragged_f64(")
    decl = " ".join(header[at:header.index(";", at)].split())
    assert "int32_t tenure, int32_t max_span, int32_t max_rank, int32_t wide," in decl and decl.endswith("int32_t* stalled, int32_t* pair_steps, void* stream)")
    assert "New: no reference counterpart" in header[header.rindex("/*", 0, at):at]


def test_lds_bytes_are_what_the_carve_takes():
    """The refusal names the bytes the host asked the carve for; here they are counted by hand from the layout, per form, at the launch's
    maxima.  Lane form: [4][64] columns + 4 bounds (260 f64), base / len / cur [64] i32, the table [max_cand][4] and mer [max_cand] f64,
    rk [max_cand], list [max_slots][rank], expire [max_cand], best [max_slots] i32.  Workgroup form: four columns [T], red [8], bounds
    [4], three sibling rows [32] and mer [max_cand] f64; cnt [4], base / len [T], rk, list [T][rank], expire, best [T] i32."""
    _lib, lib, _names, call = _entry()
    slots, cand, rank = 5, 6000, 7
    assert call(max_slots=slots, max_cand=cand, max_rank=rank) == _lib.E_UNSUP
    msg = lib.gnnpn_last_error()
    lane = 260 * 8 + 192 * 4 + cand * 4 * 8 + cand * 8 + (cand + slots * rank + cand + slots) * 4
    assert str(lane).encode() + b" B of LDS per problem (5 slots, 6000 candidates, shortlists of 7) exceed a CU" in msg and b"wide=1" in msg
    assert msg.startswith(b"descend_tabu_pairs_ragged:")
    slots, cand = 3000, 20                                 # above 64 slots: the workgroup form, asked for or not
    assert call(max_slots=slots, max_cand=cand, max_rank=rank) == _lib.E_UNSUP
    msg = lib.gnnpn_last_error()
    wide = (4 * slots + 8 + 4 + 3 * 32 + cand) * 8 + (4 + 2 * slots) * 4 + (cand + slots * rank + cand + slots) * 4
    assert str(wide).encode() + b" B of LDS per problem (3000 slots, 20 candidates, shortlists of 7) exceed a CU" in msg and b"wide=1" not in msg
    assert call(max_slots=3000, max_cand=20, max_rank=0) == _lib.E_UNSUP and b"shortlists of 20" in lib.gnnpn_last_error()      # whole lists
    assert call(max_slots=100, max_cand=50000) == _lib.E_UNSUP and b"50000 candidates" in lib.gnnpn_last_error()


# ---- the Python layers --------------------------------------------------------------------------------------------------------------------

def _defaults(f):
    return {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}


def test_signatures_and_defaults():
    from gnnpn_sc_amd import ML2PN, ops
    from gnnpn_sc_amd.pipeline import ML2PNPipeline, descend_starts_tabu_pairs, descend_tabu_pairs
    assert ops.DEFAULT_PAIR_RANK in (1, 2, 4, 8)                                   # a value of the sweep of tools/bench_tabu_pairs.py
    assert list(inspect.signature(ops.descend_tabu_pairs_ragged).parameters) == [
        "prob_ptr", "cand_ptr", "cand", "bounds", "start_pos", "max_sweeps", "max_steps", "tenure", "max_rank", "max_span", "max_slots", "max_cand",
        "wide"]
    assert _defaults(ops.descend_tabu_pairs_ragged) == {"max_sweeps": 16, "max_steps": 32, "tenure": ops.DEFAULT_TENURE,
                                                        "max_rank": ops.DEFAULT_PAIR_RANK, "max_span": 0, "max_slots": None, "max_cand": None,
                                                        "wide": None}
    assert list(inspect.signature(ops.SearchTables.descend_tabu_pairs).parameters) == ["self", "max_sweeps", "max_steps", "tenure", "max_rank",
                                                                                       "max_span", "wide"]
    sig = inspect.signature(descend_tabu_pairs)
    assert list(sig.parameters) == ["services", "batch", "out", "max_sweeps", "max_steps", "tenure", "max_rank", "max_span", "reduct", "min_cost",
                                    "patches"]
    assert _defaults(descend_tabu_pairs) == {"max_sweeps": 16, "max_steps": 32, "tenure": ops.DEFAULT_TENURE, "max_rank": ops.DEFAULT_PAIR_RANK,
                                             "max_span": 0, "reduct": 0, "min_cost": None, "patches": ()}
    assert list(inspect.signature(ML2PNPipeline.descend_tabu_pairs).parameters)[1:] == list(sig.parameters)
    assert _defaults(ML2PNPipeline.descend_tabu_pairs) == _defaults(descend_tabu_pairs)
    sig = inspect.signature(descend_starts_tabu_pairs)
    assert list(sig.parameters) == ["services", "batch", "starts", "max_sweeps", "max_steps", "tenure", "max_rank", "max_span", "reduct", "min_cost",
                                    "patches"]
    assert list(inspect.signature(ML2PNPipeline.descend_starts_tabu_pairs).parameters)[1:] == list(sig.parameters)
    assert _defaults(ML2PNPipeline.descend_starts_tabu_pairs) == _defaults(descend_starts_tabu_pairs)
    assert list(inspect.signature(ML2PN.infer_tabu_pairs).parameters) == [
        "dataset", "net", "low", "high", "n_per", "epoch", "device", "batch_size", "precision", "samples", "sample_seed", "descend",
        "all_starts", "tabu_steps", "tenure", "pair_rank", "pair_span"]
    assert list(inspect.signature(ML2PN.stage_given).parameters) == ["pair_rounds", "pair_span", "pair_rank", "tabu_steps", "pair_moves"]


def test_the_sixth_stage_lives_in_a_second_table():
    from gnnpn_sc_amd import ML2PN, ops
    from gnnpn_sc_amd import pipeline as pl
    assert list(pl.STAGES) == ["descend", "descend_pairs", "descend_pairs_windowed", "descend_pairs_shortlist", "descend_tabu"]
    assert set(ML2PN.RUNS) == set(pl.STAGES) and len(ML2PN.RUNS) == 5
    assert list(pl.MORE_STAGES) == list(ML2PN.MORE_RUNS) == ["descend_tabu_pairs"] and pl.MORE_STAGES["descend_tabu_pairs"] is pl.TABU_PAIRS
    st = pl.TABU_PAIRS
    assert st.method == "descend_tabu_pairs" and st.values == () and not st.lane_only and callable(getattr(ops.SearchTables, st.method))
    assert st.options == ("max_steps", "tenure", "max_rank", "max_span") and st.row_keys == ("steps", "best_step", "pair_steps")
    assert st.winner_rows == ("walk",) and callable(getattr(pl, st.method)) and callable(getattr(pl, st.starts[0]))
    assert callable(getattr(ML2PN, ML2PN.MORE_RUNS[st.method][2]))
    assert len(ML2PN.MORE_RUNS[st.method][0]) == len(st.options) == st.refusal.count("{}")
    assert pl.stage_named("descend_tabu") is pl.TABU and pl.stage_named("descend_tabu_pairs") is st
    assert ML2PN.run_named("descend_tabu") is ML2PN.RUNS["descend_tabu"]
    # every existing call of stage_given keeps its answer; the new keyword comes last and wins
    assert ML2PN.stage_given() == "descend" and ML2PN.stage_given(4) == "descend_pairs" and ML2PN.stage_given(4, 0) == "descend_pairs_windowed"
    assert ML2PN.stage_given(4, 1, 2) == "descend_pairs_shortlist" and ML2PN.stage_given(tabu_steps=0) == "descend_tabu"
    assert ML2PN.stage_given(tabu_steps=8, pair_moves=0) == "descend_tabu_pairs"
    assert ML2PN.stage_ok("descend_tabu_pairs", 4, 8, 2, 0, 0) and not ML2PN.stage_ok("descend_tabu_pairs", None, 8, 2, 0, 0)
    assert not ML2PN.stage_ok("descend_tabu_pairs", 4, 8, 2, -1, 0) and not ML2PN.stage_ok("descend_tabu_pairs", 4, 8, 2, 0, None)


@pytest.mark.parametrize("multi,function,file", [(False, "descend_tabu_pairs", "ML+2PN+tabu+pairs.txt"),
                                                 (True, "descend_starts_tabu_pairs", "ML+2PN+multistart+tabu+pairs.txt")])
def test_plan_of_the_test_quarter(multi, function, file):
    from gnnpn_sc_amd import ML2PN
    from gnnpn_sc_amd import pipeline as pl
    got = ML2PN.search_plan(pl.TABU_PAIRS.bind(8, 4, 2, 1), multi)
    assert got == (function, {"max_steps": 8, "tenure": 4, "max_rank": 2, "max_span": 1}, file, ("steps", "best_step", "pair_steps", "stalled"),
                   {"tabu_steps": 8, "tenure": 4, "top": 2, "span": 1})
    assert list(got[4]) == ["tabu_steps", "tenure", "top", "span"]                 # extra's keys in the artefact's order
    taken = inspect.signature(getattr(pl, function)).parameters
    assert set(got[1]) <= set(taken) and {"max_sweeps", "reduct", "min_cost"} <= set(taken) and ("starts" if multi else "out") in taken


SENTENCE = "the number of steps, the tenure, the rank and the span must be >= 0, got {}, {}, {} and {}"
NEGATIVE = [({"max_steps": -1, "tenure": 2, "max_rank": 2}, (-1, 2, 2, 0)), ({"tenure": -2, "max_rank": 2}, (32, -2, 2, 0)),
            ({"tenure": 2, "max_rank": -1}, (32, 2, -1, 0)), ({"tenure": 2, "max_rank": 3, "max_span": -4}, (32, 2, 3, -4))]


@pytest.mark.parametrize("kw,values", NEGATIVE)
def test_a_negative_option_is_told_the_stages_sentence_under_every_public_name(kw, values):
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd import pipeline as pl
    for who in ("descend_tabu_pairs", "descend_starts_tabu_pairs"):
        for f in (getattr(pl, who), lambda *a, _w=who, **k: getattr(pl.ML2PNPipeline, _w)(None, *a, **k)):
            with pytest.raises(ops.GnnpnError) as e:
                f(None, None, None, **kw)                   # before it looks at the services, the batch or the rows
            assert str(e.value) == f"{who}: " + SENTENCE.format(*values)


def test_wrappers_reject_host_tensors_and_inconsistent_sizes():
    from gnnpn_sc_amd import ML2PN, ops
    from gnnpn_sc_amd.pipeline import descend_starts_tabu_pairs, descend_tabu_pairs
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)   # noqa: E731
    operands = (i32([0, 2, 3]), i32([0, 1, 2, 3]), f64(3, 4), f64(2, 4), i32([0, 0, 0]))
    for kw in ({"max_slots": 2, "max_cand": 2}, {}, {"wide": True}, {"max_steps": 0}, {"max_rank": 0}, {"max_slots": 70, "max_cand": 2}):
        with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
            ops.descend_tabu_pairs_ragged(*operands, **{"tenure": 2, "max_rank": 2, **kw})
    for kw in ({"max_steps": -1}, {"tenure": -1}, {"max_sweeps": -1}, {"max_rank": -1}, {"max_span": -1}):
        with pytest.raises(ops.GnnpnError, match="descend_tabu_pairs_ragged: inconsistent"):
            ops.descend_tabu_pairs_ragged(*operands, **{"tenure": 2, "max_rank": 2, **kw})
    with pytest.raises(ops.GnnpnError, match="inconsistent"):
        ops.descend_tabu_pairs_ragged(*operands[:4], i32([0, 0]), tenure=2, max_rank=2)
    with pytest.raises(ops.GnnpnError, match="inconsistent"):
        ops.descend_tabu_pairs_ragged(*operands[:3], f64(3, 4), operands[4], tenure=2, max_rank=2)
    tabs = ops.SearchTables(prob_ptr=operands[0], cand_ptr=operands[1], cand=operands[2], bounds=operands[3], start_pos=operands[4],
                            max_slots=2, max_cand=2)
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        tabs.descend_tabu_pairs(4, 8, 2, 2, 0)

    class Svc:
        cat_ptr, qos = i32([0, 2, 4, 6]), f64(6, 4)

    class Batch:
        n_problems = 2
        x, seg_ptr = torch.zeros(6, 7), i32([0, 3, 6])
        local_bounds, global_bounds = f64(2, 3, 4), f64(2, 4)
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        descend_tabu_pairs(Svc, Batch, {"actions": torch.zeros(2, 3, 8)}, tenure=2, max_rank=2)
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        descend_starts_tabu_pairs(Svc, Batch, torch.zeros(2, 3, 3, 8), tenure=2, max_rank=2)
    for kw in ({"tabu_steps": -1}, {"tenure": -1}, {"descend": None}, {"tabu_steps": None}, {"pair_rank": -1}, {"pair_span": -1},
               {"pair_span": None}):
        with pytest.raises(ValueError) as e:
            ML2PN.infer_tabu_pairs("QWS", None, None, None, 3, **{"tenure": 2, "pair_rank": 2, **kw})
        assert str(e.value) == ("ML2PN.infer_tabu_pairs: pair_moves needs descend, a number of steps >= 0, a tenure >= 0, a rank >= 0 and a "
                                "span >= 0")


def test_main_cli_refuses_pair_moves_before_any_file_is_read(capsys, tmp_path, monkeypatch):
    import main as cli
    monkeypatch.chdir(tmp_path)                            # no ./data here: reading a file would raise, not return 1
    base = ["main.py", "QWS", "ML+2PN", "-1", "--infer"]
    assert cli.main(base + ["--descend", "--pair-moves"]) == 1                                   # without --tabu
    assert cli.main(base + ["--descend", "--tabu", "--pair-moves=-1"]) == 1
    assert cli.main(base + ["--descend", "--tabu", "--pair-moves=x"]) == 1
    assert capsys.readouterr().out.count("--pair-moves[=RANK]: needs --tabu[=STEPS] and RANK >= 0 (0: whole lists)\n") == 3
    assert cli.main(base + ["--descend", "--tabu", "--pair-span=2"]) == 1                        # without --pair-moves
    assert cli.main(base + ["--descend", "--tabu", "--pair-moves", "--pair-span=-1"]) == 1
    assert cli.main(base + ["--descend", "--tabu", "--pair-moves=2", "--pair-span"]) == 1
    assert capsys.readouterr().out.count("--pair-span=N: needs --pair-moves[=RANK] and N >= 0 (0: every slot pair)\n") == 3
    assert cli.main(base + ["--descend", "--tabu", "--pair-moves", "--woa"]) == 1
    assert cli.main(base + ["--descend", "--tabu", "--pair-moves=2", "--pair-span=1", "--services"]) == 1
    assert capsys.readouterr().out.count("--pair-moves[=RANK], --pair-span=N: not with --woa or --services") == 2
    assert cli.main(base + ["--descend", "--tabu", "--pairs"]) == 1                              # as before
    assert cli.main(base + ["--descend", "--tabu", "--pairs", "--pair-moves"]) == 1
    assert capsys.readouterr().out.count("--tabu[=STEPS]: not with --pairs, --woa or --services (the walk takes single swaps, and the ES-WOA "
                                         "start and the services artefact take the descent's result)\n") == 2
    for more in (["--pair-moves"], ["--tabu=0", "--pair-moves=0", "--pair-span=0"],
                 ["--tabu=8", "--tenure=2", "--pair-moves=4", "--pair-span=3", "--samples=3", "--all-starts"]):
        with pytest.raises(FileNotFoundError):
            cli.main(base + ["--descend", "--tabu"][:1 if any(m.startswith("--tabu") for m in more) else 2] + more)      # accepted: goes on to the data
