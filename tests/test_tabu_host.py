"""-m "not gpu": the tabu walk (gnnpn_descend_tabu_ragged_f64, ops.descend_tabu_ragged, SearchTables.descend_tabu,
pipeline.descend_tabu / descend_starts_tabu, ML2PN.infer_tabu, `main.py ... --descend --tabu`) rejects bad arguments and host tensors
before any launch, and the plain-Python reference the GPU tests compare with (tests/tabu_reference.py) has the properties that make
those comparisons meaningful."""
import ctypes
import inspect

import pytest
import torch

import descent_reference as ref
import pair_descent_reference as pref
import pair_shortlist_reference as sref
import pair_window_reference as wref
import tabu_reference as tref

P = ctypes.c_void_p(64)          # a non-null stand-in: every call below fails before it is dereferenced
SHARED = ("best_fitness", "start_fitness", "best_pos", "best_rows", "sweeps", "moves")


# ---- the reference ----------------------------------------------------------------------------------------------------------------------

def test_no_steps_is_one_swap_descent():
    tables = sref._seeds_tables()
    assert len(tables) == 20
    for tab, r in zip(tables, tref.seeds_runs(0, 3)):
        one = ref.descend(*tab)
        assert {k: r[k] for k in SHARED} == {k: one[k] for k in SHARED}
        assert r["history"] == [one["best_fitness"]] and r["walk"] == [] and (r["steps"], r["best_step"], r["stalled"]) == (0, 0, 0)
        cut = tref.descend_tabu(*tab, max_sweeps=0, max_steps=0, tenure=3)
        assert cut["best_fitness"] == cut["start_fitness"] == one["start_fitness"] and cut["sweeps"] == 0


def test_the_walk_leaves_one_swap_optima_and_tenure_matters():
    tables = sref._seeds_tables()
    one = [ref.descend(*tab)["best_fitness"] for tab in tables]
    below = {}
    for tenure in (0, 3, 5):
        runs = tref.seeds_runs(32, tenure)
        below[tenure] = sum(r["best_fitness"] < o for r, o in zip(runs, one))
        assert not any(r["best_fitness"] > o for r, o in zip(runs, one)), tenure          # never above one-swap descent
        assert all(r["best_fitness"] <= r["history"][-1] for r in runs)
        assert all((r["best_fitness"] < r["history"][-1]) <= (r["polished"][1] > 0) for r in runs)      # strict only where the polish moved
    assert below[3] >= 5 and below[0] < below[3]                                            # measured: 8 and 4
    assert sum(any(s[4] for s in r["trace"]) for r in tref.seeds_runs(32, 3)) >= 1        # a tabu move admitted by aspiration (measured: 2)
    assert sum(r["stalled"] for r in tref.seeds_runs(32, 5)) >= 1                          # measured: 3
    assert not any(r["stalled"] for r in tref.seeds_runs(32, 3))


def test_the_polish_runs_and_moves_where_the_walk_is_cut_at_its_best():
    for steps in (2, 3):
        runs = tref.seeds_runs(steps, 3)
        assert sum(r["polished"][0] for r in runs) >= 1 and sum(r["polished"][1] > 0 for r in runs) >= 1      # measured: 4, and 2 / 3
        for r in runs:
            assert r["polished"][0] == (r["steps"] > 0 and r["best_step"] == r["steps"] and not r["stalled"])


def test_no_step_returns_within_the_tenure():
    for steps, tenure in tref.SEED_RUNS:
        for r in tref.seeds_runs(steps, tenure):
            assert tref.returns_within_tenure(r, tenure) == []
    assert any(tref.returns_within_tenure(r, 3) for r in tref.seeds_runs(32, 0))          # the check bites: without a tenure the walk returns


def test_the_wall_is_left_in_two_steps():
    tab = pref.wall_problem()
    r = tref.descend_tabu(*tab, max_steps=4, tenure=2)
    assert r["walk"] == [1.525, 0.55] and r["best_pos"] == [1, 1] and (r["steps"], r["best_step"], r["stalled"]) == (2, 2, 1)
    assert r["history"] == [1.5, 0.55, 0.55, 0.55]
    free = tref.descend_tabu(*tab, max_steps=4, tenure=0)
    assert free["walk"] == [1.525, 0.55, 1.525, 0.55] and free["stalled"] == 0 and free["best_pos"] == [1, 1]


def test_ties_go_to_the_lower_slot_and_position():
    r = tref.descend_tabu(*sref.duplicated_rows(), max_steps=6, tenure=2)
    assert r["best_pos"] == [1, 2, 1] and r["best_step"] == 3


def test_a_nan_merit_is_never_taken():
    cats, bounds, start = sref.nan_row_problem()
    r = tref.descend_tabu(cats, bounds, start, max_steps=6, tenure=2, with_trace=True)
    assert r["steps"] == 6 and all(f == f for f in r["walk"]) and not any((j, c) in ((1, 0), (1, 2)) for _t, j, c, *_ in r["trace"])


def test_lists_of_one_row_stall_at_once():
    r = tref.descend_tabu(*tref.single_rows(), max_steps=6, tenure=2)
    assert (r["steps"], r["best_step"], r["stalled"]) == (0, 0, 1) and r["walk"] == [] and r["history"] == [r["best_fitness"]] * 6


def test_the_gpu_cases_are_not_vacuous():
    """Above 128 slots np.sum takes its recursion: the planted cases hold the walk on every step there (best_step = 0), and the
    wall across two leaf blocks has best_step > 0; the long lists have the best swaps beyond one chunk."""
    for name in ("planted65", "planted129", "planted257"):
        (r,) = tref.case_want(name)
        assert r["steps"] == 12 and r["best_step"] == 0 and len(set(r["walk"])) > 1, name
    (r,) = tref.case_want("wall131")
    assert len(tref.CASES["wall131"][0][0][0]) == 131 and (r["steps"], r["best_step"], r["stalled"]) == (2, 2, 1) and r["best_fitness"] < 1.0
    assert wref.leaf_of(131, 63) != wref.leaf_of(131, 64)
    assert [len(c) for c in tref.CASES["long"][0][0][0]] == [139, 70, 5] and any(c >= 128 for _t, j, c, *_ in tref.case_want("long")[0]["trace"])
    assert max(len(c) for c in tref.CASES["long_wide"][0][0][0]) == 300
    assert any(c >= 256 for _t, j, c, *_ in tref.case_want("long_wide")[0]["trace"])
    assert all(len(t[0]) == 64 for t in tref.CASES["t64"][0]) and all(r["steps"] == 32 for r in tref.case_want("t64"))
    small = tref.case_want("small")
    assert [r["stalled"] for r in small] == [0, 0, 0, 1, 1] and small[2]["steps"] == 6      # T = 1 walks on: its list is its neighbourhood
    cut = tref.case_want("seeds_s32_t3_sweeps0")
    assert any(r["best_step"] > 0 for r in cut) and all(r["sweeps"] == 0 or r["polished"][0] for r in cut)


# ---- the C entry ------------------------------------------------------------------------------------------------------------------------

def test_tabu_entry_rejects_bad_arguments():
    from gnnpn_sc_amd import _lib
    lib = _lib.load()
    names = ("prob_ptr", "cand_ptr", "cand", "bounds", "start_pos", "best_fitness", "start_fitness", "best_pos", "best_rows", "history",
             "sweeps", "moves", "walk", "steps", "best_step", "stalled")

    def call(B=3, n_lists=12, max_slots=5, max_cand=20, max_sweeps=4, max_steps=8, tenure=2, wide=0, **null):
        a = {n: (None if n in null else P) for n in names}
        return lib.gnnpn_descend_tabu_ragged_f64(
            B, a["prob_ptr"], n_lists, max_slots, max_cand, a["cand_ptr"], a["cand"], a["bounds"], a["start_pos"], max_sweeps, max_steps,
            tenure, wide, a["best_fitness"], a["start_fitness"], a["best_pos"], a["best_rows"], a["history"], a["sweeps"], a["moves"],
            a["walk"], a["steps"], a["best_step"], a["stalled"], None)
    for n in names:
        if n != "best_rows":                                # the one optional output
            assert call(**{n: True}) == -1 and b"null" in lib.gnnpn_last_error(), n
    for kw in ({"B": -1}, {"n_lists": -1}, {"max_slots": 0}, {"max_sweeps": -1}, {"max_steps": -1}, {"tenure": -1}):
        assert call(**kw) == -1 and b"bad argument" in lib.gnnpn_last_error(), kw
    for kw in ({}, {"wide": 1}, {"max_slots": 100}):        # the tabu table is sized by max_cand in both forms
        assert call(max_cand=0, **kw) == _lib.E_UNSUP and b"max_cand" in lib.gnnpn_last_error(), kw
    assert call(max_cand=6000) == _lib.E_UNSUP
    msg = lib.gnnpn_last_error()
    assert b"LDS" in msg and b"5 slots" in msg and b"6000 candidates" in msg and b"wide=1" in msg
    assert call(max_slots=5000, max_cand=20) == _lib.E_UNSUP
    msg = lib.gnnpn_last_error()
    lds = (4 * 5000 + 12 + 32) * 8 + (2 * 5000 + 4) * 4 + (20 + 5000) * 4
    assert b"5000 slots" in msg and b"20 candidates" in msg and str(lds).encode() + b" B of LDS" in msg and b"wide=1" not in msg
    assert call(max_slots=100, max_cand=50000) == _lib.E_UNSUP and b"50000 candidates" in lib.gnnpn_last_error()      # the tabu table alone
    assert call(B=0) == 0 and call(B=0, prob_ptr=True, walk=True, max_slots=5000) == 0          # an empty batch launches nothing
    assert "gnnpn_descend_tabu_ragged_f64" in _lib.EXPORTS
    assert lib.gnnpn_abi_version() == 9


# ---- the Python layers --------------------------------------------------------------------------------------------------------------------

def _defaults(f):
    return {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}


def test_signatures_and_defaults():
    from gnnpn_sc_amd import ML2PN, ops
    from gnnpn_sc_amd.pipeline import ML2PNPipeline, descend_starts_tabu, descend_tabu
    assert ops.DEFAULT_TENURE in (1, 2, 4, 8, 16)                                  # a value of the sweep of tools/bench_tabu.py
    assert list(inspect.signature(ops.descend_tabu_ragged).parameters) == ["prob_ptr", "cand_ptr", "cand", "bounds", "start_pos", "max_sweeps",
                                                                          "max_steps", "tenure", "max_slots", "max_cand", "wide"]
    assert _defaults(ops.descend_tabu_ragged) == {"max_sweeps": 16, "max_steps": 32, "tenure": ops.DEFAULT_TENURE, "max_slots": None,
                                                  "max_cand": None, "wide": None}
    assert list(inspect.signature(ops.SearchTables.descend_tabu).parameters) == ["self", "max_sweeps", "max_steps", "tenure", "wide"]
    sig = inspect.signature(descend_tabu)
    assert list(sig.parameters) == ["services", "batch", "out", "max_sweeps", "max_steps", "tenure", "reduct", "min_cost", "patches"]
    assert _defaults(descend_tabu) == {"max_sweeps": 16, "max_steps": 32, "tenure": ops.DEFAULT_TENURE, "reduct": 0, "min_cost": None, "patches": ()}
    assert list(inspect.signature(ML2PNPipeline.descend_tabu).parameters)[1:] == list(sig.parameters)
    assert _defaults(ML2PNPipeline.descend_tabu) == _defaults(descend_tabu)
    sig = inspect.signature(descend_starts_tabu)
    assert list(sig.parameters) == ["services", "batch", "starts", "max_sweeps", "max_steps", "tenure", "reduct", "min_cost", "patches"]
    assert list(inspect.signature(ML2PNPipeline.descend_starts_tabu).parameters)[1:] == list(sig.parameters)
    assert _defaults(ML2PNPipeline.descend_starts_tabu) == _defaults(descend_starts_tabu)
    assert "tabu_steps" not in inspect.signature(ML2PN.infer).parameters           # infer's parameter list is pinned: a function of its own
    assert list(inspect.signature(ML2PN.infer_tabu).parameters) == [
        "dataset", "net", "low", "high", "n_per", "epoch", "device", "batch_size", "precision", "samples", "sample_seed", "descend",
        "all_starts", "tabu_steps", "tenure"]


def test_wrappers_reject_host_tensors_and_negative_arguments():
    from gnnpn_sc_amd import ML2PN, ops
    from gnnpn_sc_amd.pipeline import ML2PNPipeline, descend_starts_tabu, descend_tabu
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)   # noqa: E731
    operands = (i32([0, 2, 3]), i32([0, 1, 2, 3]), f64(3, 4), f64(2, 4), i32([0, 0, 0]))
    for kw in ({"max_slots": 2, "max_cand": 2}, {}, {"wide": True}, {"max_steps": 0}, {"max_slots": 70, "max_cand": 2}):
        with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
            ops.descend_tabu_ragged(*operands, tenure=2, **kw)
    for kw in ({"max_steps": -1}, {"tenure": -1}, {"max_sweeps": -1}):
        with pytest.raises(ops.GnnpnError, match="inconsistent"):
            ops.descend_tabu_ragged(*operands, **{"tenure": 2, **kw})
    with pytest.raises(ops.GnnpnError, match="inconsistent"):
        ops.descend_tabu_ragged(*operands[:4], i32([0, 0]), tenure=2)
    tabs = ops.SearchTables(prob_ptr=operands[0], cand_ptr=operands[1], cand=operands[2], bounds=operands[3], start_pos=operands[4],
                            max_slots=2, max_cand=2)
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        tabs.descend_tabu(4, 8, 2)

    class Svc:
        cat_ptr, qos = i32([0, 2, 4, 6]), f64(6, 4)

    class Batch:
        n_problems = 2
        x, seg_ptr = torch.zeros(6, 7), i32([0, 3, 6])
        local_bounds, global_bounds = f64(2, 3, 4), f64(2, 4)
    out = {"actions": torch.zeros(2, 3, 8)}
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        descend_tabu(Svc, Batch, out, tenure=2)
    starts = torch.zeros(2, 3, 3, 8)
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        descend_starts_tabu(Svc, Batch, starts, tenure=2)
    for who, fs, arg in (("descend_tabu", (descend_tabu, lambda *a, **k: ML2PNPipeline.descend_tabu(None, *a, **k)), out),
                         ("descend_starts_tabu", (descend_starts_tabu, lambda *a, **k: ML2PNPipeline.descend_starts_tabu(None, *a, **k)), starts)):
        for f in fs:
            for kw in ({"max_steps": -1, "tenure": 2}, {"tenure": -1}):
                with pytest.raises(ops.GnnpnError, match=who + ": the number of steps and the tenure must be >= 0"):
                    f(Svc, Batch, arg, **kw)
    for kw in ({"tabu_steps": -1}, {"tenure": -1}, {"descend": None}, {"tabu_steps": None}):
        with pytest.raises(ValueError, match="tabu_steps"):
            ML2PN.infer_tabu("QWS", None, None, None, 3, **{"tenure": 2, **kw})


def test_main_cli_refuses_tabu_before_any_file_is_read(capsys, tmp_path, monkeypatch):
    import main as cli
    monkeypatch.chdir(tmp_path)                            # no ./data here: reading a file would raise, not return 1
    base = ["main.py", "QWS", "ML+2PN", "-1", "--infer"]
    assert cli.main(base + ["--tabu"]) == 1                                                      # without --descend
    assert cli.main(base + ["--descend", "--tabu=-1"]) == 1
    assert cli.main(base + ["--descend", "--tabu=x"]) == 1
    assert capsys.readouterr().out.count("--tabu[=STEPS]: needs --descend[=SWEEPS] and STEPS >= 0") == 3
    assert cli.main(base + ["--descend", "--tabu", "--pairs"]) == 1
    assert cli.main(base + ["--descend", "--tabu=8", "--woa"]) == 1
    assert cli.main(base + ["--descend", "--tabu=8", "--pairs", "--top=2"]) == 1
    assert capsys.readouterr().out.count("--tabu[=STEPS]: not with --pairs, --woa") == 3
    assert cli.main(base + ["--descend", "--tenure=2"]) == 1                                     # without --tabu
    assert cli.main(base + ["--descend", "--tabu", "--tenure=-2"]) == 1
    assert cli.main(base + ["--descend", "--tabu", "--tenure"]) == 1
    assert capsys.readouterr().out.count("--tenure=N: needs --tabu[=STEPS] and N >= 0") == 3
    assert cli.main(base + ["--descend", "--tabu", "--all-starts"]) == 1                         # --all-starts' own refusal
    assert "--all-starts: needs --samples=N" in capsys.readouterr().out
    assert cli.main(base + ["--tabu", "--pairs"]) == 1                                           # --pairs' own refusal comes first
    assert "--pairs[=ROUNDS]: needs --descend" in capsys.readouterr().out
    for more in (["--tabu"], ["--tabu=0", "--tenure=0"], ["--tabu=8", "--tenure=2", "--samples=3", "--all-starts"]):
        with pytest.raises(FileNotFoundError):
            cli.main(base + ["--descend"] + more)                                                # accepted: goes on to the data

