"""-m "not gpu": the windowed pair-swap descent (gnnpn_descend_pairs_windowed_ragged_f64, ops.descend_pairs_windowed_ragged,
SearchTables.descend_pairs_windowed, pipeline.descend_pairs_windowed, `main.py ... --pairs --span=N`) rejects bad arguments and host
tensors before any launch, and the plain-Python reference the GPU tests compare with (tests/pair_window_reference.py) has the
properties that make those comparisons meaningful."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import descent_reference as ref
import pair_descent_reference as pref
import pair_window_reference as wref

P = ctypes.c_void_p(64)          # a non-null stand-in: every call below fails before it is dereferenced


# ---- the reference ----------------------------------------------------------------------------------------------------------------------

def test_span_zero_is_the_pair_reference():
    """Every field, on the tables of the pair-swap host test (T = 2, 3, 7, 8, 9) and at three cut-offs."""
    from test_gpu_woa import _random_problems
    from test_pair_descend_host import SEEDS
    n = 0
    for seed, sizes, per, mc in SEEDS:
        g = np.random.default_rng(seed)
        for T in sizes:
            for tab in ref.prepare(_random_problems(g, T, per, mc)):
                for kw in ({}, {"max_rounds": 1}, {"max_sweeps": 0}):
                    assert wref.descend_pairs(*tab, max_span=0, **kw) == pref.descend_pairs(*tab, **kw), (T, kw)
                # a span that holds every pair is the full sweep too
                assert wref.descend_pairs(*tab, max_span=T) == pref.descend_pairs(*tab)
                n += 1
    assert n == 20


def test_the_window_has_its_effect():
    """A planted wall farther apart than the span stays: one violation is left and nothing within the span helps (converged = 1).
    The same wall within the span is removed."""
    tab = wref.planted(7, 40, wall2=(5, 20), nfill=2)
    one = ref.descend(*tab)
    assert one["best_fitness"] > 1.0
    for span, removed in ((14, False), (15, True), (0, True), (1, False)):
        r = wref.descend_pairs(*tab, max_span=span)
        assert r["converged"] == 1, span
        assert (r["best_fitness"] < 1.0) == removed and (r["pair_moves"] >= 1) == removed, span
        if not removed:
            assert r["best_fitness"] == one["best_fitness"] and r["rounds"] == 1 and r["best_pos"] == one["best_pos"]
        else:
            assert one["best_fitness"] - r["best_fitness"] > 0.5 and r["best_pos"][5] == 1 and r["best_pos"][20] == 1
    (tab,), (r,) = wref.beyond_tables(), wref.beyond_want()
    assert 1.0 < r["best_fitness"] < 2.0 and r["converged"] == 1 and r["pair_moves"] == 2          # wall3 and mins go, wall2 stays
    assert r["best_pos"][0] == 0 and r["best_pos"][200] == 0 and r["best_pos"][190] == 1 and r["best_pos"][256] == 1


def test_one_and_two_slots():
    one = ([[(0.3, 0.5, 0.9, 0.9), (0.2, 0.6, 0.9, 0.9)]], [0.0, 1.0, 0.0, 1.0], [0])
    for span in (0, 1, 5):
        r = wref.descend_pairs(*one, max_span=span)
        assert r == pref.descend_pairs(*one) and r["rounds"] == 1 and r["pair_moves"] == 0 and r["converged"] == 1
    two = pref.wall_problem()
    for span in (0, 1, 2):
        r = wref.descend_pairs(*two, max_span=span)
        assert r == pref.descend_pairs(*two) and r["pair_moves"] == 1 and r["best_pos"] == [1, 1]


def test_the_gpu_cases_are_not_vacuous():
    """On the reference results of the size cases of tests/test_gpu_pair_window.py: every case moves by pairs, somewhere a violation
    is removed, and pairs whose two slots lie in different leaf blocks of np.sum are taken — across the root and below it."""
    gains, depths, inside = [], set(), set()
    for T, (span, kws) in wref.SIZE_CASES.items():
        for kw, tab, w in zip(kws, wref.size_tables(T), wref.size_want(T)):
            assert len(tab[0]) == T and w["pair_moves"] > 0 and w["converged"] == 1, T
            one = ref.descend(*tab)
            gains.append(one["best_fitness"] - w["best_fitness"])
            pairs = [kw[k] for k in ("wall2", "wall3", "mins") if k in kw]
            assert all(one["best_pos"][s] == 0 for p in pairs for s in p), T            # no single swap takes a planted slot
            taken = [(i, j) for i, j in pairs if w["best_pos"][i] == 1 and w["best_pos"][j] == 1]
            assert len(taken) == w["pair_moves"] == len(pairs), T                       # every planted pair goes, and only by a pair move
            for i, j in taken:
                assert not span or j - i <= span, (T, i, j)
                if wref.leaf_of(T, i) != wref.leaf_of(T, j):
                    depths.add((T, i, j))
                else:
                    inside.add(T)
    assert inside == set(wref.SIZE_CASES)                                               # ... and in every case one pair inside a leaf block
    assert max(gains) > 0.5
    assert {(129, 63, 64), (257, 127, 128), (257, 191, 192), (520, 255, 256), (520, 383, 384), (520, 447, 448)} <= depths
    assert wref.leaf_of(520, 447) == (384, 64) and wref.leaf_of(520, 448) == (448, 72) and wref.leaf_of(257, 200) == (192, 65)
    assert wref.leaf_of(129, 63) == (0, 64) and wref.leaf_of(128, 127) == (0, 128)


# ---- the C entry ------------------------------------------------------------------------------------------------------------------------

def test_windowed_entry_rejects_bad_arguments():
    from gnnpn_sc_amd import _lib
    lib = _lib.load()
    names = ("prob_ptr", "cand_ptr", "cand", "bounds", "start_pos", "best_fitness", "start_fitness", "best_pos", "best_rows",
             "round_history", "sweeps", "moves", "rounds", "pair_moves", "converged")

    def call(B=3, n_lists=12, max_slots=5, max_cand=20, max_sweeps=4, max_rounds=2, max_span=0, wide=0, **null):
        a = {n: (None if n in null else P) for n in names}
        return lib.gnnpn_descend_pairs_windowed_ragged_f64(
            B, a["prob_ptr"], n_lists, max_slots, max_cand, a["cand_ptr"], a["cand"], a["bounds"], a["start_pos"], max_sweeps, max_rounds,
            max_span, wide, a["best_fitness"], a["start_fitness"], a["best_pos"], a["best_rows"], a["round_history"], a["sweeps"],
            a["moves"], a["rounds"], a["pair_moves"], a["converged"], None)
    for n in names:
        if n != "best_rows":                                # optional, as in gnnpn_descend_pairs_ragged_f64
            assert call(**{n: True}) == -1 and b"null" in lib.gnnpn_last_error(), n
    for kw in ({"B": -1}, {"n_lists": -1}, {"max_slots": 0}, {"max_sweeps": -1}, {"max_rounds": -1}, {"max_span": -1}):
        assert call(**kw) == -1 and b"bad argument" in lib.gnnpn_last_error(), kw
    assert call(max_cand=0) == _lib.E_UNSUP and b"max_cand" in lib.gnnpn_last_error()           # the lane form sizes its table by it
    assert call(max_cand=6000) == _lib.E_UNSUP and b"LDS" in lib.gnnpn_last_error()
    for kw in ({"max_slots": 5000}, {"max_slots": 5000, "wide": 1, "max_cand": 0}):              # the workgroup form: its columns
        assert call(**kw) == _lib.E_UNSUP and b"5000 slots" in lib.gnnpn_last_error(), kw
    assert call(B=0) == 0 and call(B=0, prob_ptr=True, cand=True, max_slots=5000) == 0          # an empty batch launches nothing
    assert "gnnpn_descend_pairs_windowed_ragged_f64" in _lib.EXPORTS
    assert lib.gnnpn_abi_version() == 9


# ---- the Python layers --------------------------------------------------------------------------------------------------------------------

def _defaults(f):
    return {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}


def test_signatures_and_defaults():
    from gnnpn_sc_amd import ML2PN, ops
    from gnnpn_sc_amd.pipeline import ML2PNPipeline, descend_pairs_windowed
    sig = inspect.signature(ops.descend_pairs_windowed_ragged)
    assert list(sig.parameters) == ["prob_ptr", "cand_ptr", "cand", "bounds", "start_pos", "max_sweeps", "max_rounds", "max_span", "max_slots",
                                    "max_cand", "wide"]
    assert _defaults(ops.descend_pairs_windowed_ragged) == {"max_sweeps": 16, "max_rounds": 4, "max_span": 0, "max_slots": None,
                                                            "max_cand": None, "wide": None}
    assert list(inspect.signature(ops.SearchTables.descend_pairs_windowed).parameters) == ["self", "max_sweeps", "max_rounds", "max_span", "wide"]
    assert _defaults(ops.SearchTables.descend_pairs_windowed) == {"max_sweeps": 16, "max_rounds": 4, "max_span": 0, "wide": None}
    sig = inspect.signature(descend_pairs_windowed)
    assert list(sig.parameters) == ["services", "batch", "out", "max_sweeps", "max_rounds", "max_span", "reduct", "min_cost", "patches"]
    assert _defaults(descend_pairs_windowed) == {"max_sweeps": 16, "max_rounds": 4, "max_span": 0, "reduct": 0, "min_cost": None, "patches": ()}
    assert list(inspect.signature(ML2PNPipeline.descend_pairs_windowed).parameters)[1:] == list(sig.parameters)
    assert _defaults(ML2PNPipeline.descend_pairs_windowed) == _defaults(descend_pairs_windowed)
    # ML2PN.infer's parameter list is pinned by tests/test_search_tables_host.py, so the span comes under a name of its own
    assert "pair_span" not in inspect.signature(ML2PN.infer).parameters
    assert list(inspect.signature(ML2PN.infer_pairs_windowed).parameters) == [
        "dataset", "net", "low", "high", "n_per", "epoch", "device", "batch_size", "precision", "samples", "sample_seed", "descend",
        "pair_rounds", "pair_span"]
    assert _defaults(ML2PN.infer_pairs_windowed) == {"epoch": -1, "device": "cuda:0", "batch_size": 128, "precision": "f32", "samples": 1,
                                                     "sample_seed": None, "descend": 16, "pair_rounds": 4, "pair_span": 0}


def test_wrappers_reject_host_tensors_and_negative_arguments():
    from gnnpn_sc_amd import ML2PN, ops
    from gnnpn_sc_amd.pipeline import ML2PNPipeline, descend_pairs_windowed
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)   # noqa: E731
    operands = (i32([0, 2, 3]), i32([0, 1, 2, 3]), f64(3, 4), f64(2, 4), i32([0, 0, 0]))
    for kw in ({"max_slots": 2, "max_cand": 2}, {}, {"max_span": 1, "wide": True}, {"max_slots": 70, "max_cand": 2}):
        with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
            ops.descend_pairs_windowed_ragged(*operands, **kw)
    for kw in ({"max_rounds": -1}, {"max_span": -1}, {"max_sweeps": -1}):
        with pytest.raises(ops.GnnpnError, match="inconsistent"):
            ops.descend_pairs_windowed_ragged(*operands, **kw)
    with pytest.raises(ops.GnnpnError, match="inconsistent"):
        ops.descend_pairs_windowed_ragged(*operands[:4], i32([0, 0]))
    tabs = ops.SearchTables(prob_ptr=operands[0], cand_ptr=operands[1], cand=operands[2], bounds=operands[3], start_pos=operands[4],
                            max_slots=2, max_cand=2)
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        tabs.descend_pairs_windowed(4, 2, 1)

    class Svc:
        cat_ptr, qos = i32([0, 2, 4, 6]), f64(6, 4)

    class Batch:
        n_problems = 2
        x, seg_ptr = torch.zeros(6, 7), i32([0, 3, 6])
        local_bounds, global_bounds = f64(2, 3, 4), f64(2, 4)
    out = {"actions": torch.zeros(2, 3, 8)}
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        descend_pairs_windowed(Svc, Batch, out)
    for f in (descend_pairs_windowed, lambda *a, **k: ML2PNPipeline.descend_pairs_windowed(None, *a, **k)):
        with pytest.raises(ops.GnnpnError, match="span"):
            f(Svc, Batch, out, max_span=-1)
        with pytest.raises(ops.GnnpnError, match="rounds"):
            f(Svc, Batch, out, max_rounds=-1)
    for kw in ({"pair_span": -1}, {"pair_span": 2, "pair_rounds": 0}, {"pair_span": 2, "descend": None}, {"pair_span": None}):
        with pytest.raises(ValueError, match="pair_span"):
            ML2PN.infer_pairs_windowed("QWS", None, None, None, 3, **kw)


def test_main_cli_refuses_span_before_any_file_is_read(capsys, tmp_path, monkeypatch):
    import main as cli
    monkeypatch.chdir(tmp_path)                            # no ./data here: reading a file would raise, not return 1
    base = ["main.py", "QWS", "ML+2PN", "-1", "--infer"]
    assert cli.main(base + ["--descend", "--span=2"]) == 1                                       # without --pairs
    assert cli.main(base + ["--descend", "--pairs", "--span=-1"]) == 1                           # a negative span
    assert cli.main(base + ["--descend", "--pairs", "--span"]) == 1                              # no number
    assert capsys.readouterr().out.count("--span=N: needs --pairs[=ROUNDS] and N >= 0") == 3
    assert cli.main(base + ["--descend", "--pairs", "--span=2", "--woa"]) == 1
    assert cli.main(base + ["--descend", "--pairs", "--span=2", "--samples=3", "--all-starts"]) == 1
    assert capsys.readouterr().out.count("--span=N: not with --all-starts or --woa") == 2
    assert cli.main(base + ["--pairs", "--span=2"]) == 1                                         # --pairs' own refusal comes first
    assert "--pairs[=ROUNDS]: needs --descend" in capsys.readouterr().out
    with pytest.raises(FileNotFoundError):
        cli.main(base + ["--descend", "--pairs", "--span=0"])                                    # accepted: goes on to the data
