"""-m "not gpu": the pair-swap descent (gnnpn_descend_pairs_ragged_f64, ops.descend_pairs_ragged, pipeline.descend_pairs) rejects bad
arguments and host tensors before any launch, and the plain-Python reference the GPU tests compare with
(tests/pair_descent_reference.py) has the properties that make those comparisons meaningful."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import descent_reference as ref
import pair_descent_reference as pref

P = ctypes.c_void_p(64)          # a non-null stand-in: every call below fails before it is dereferenced


def _lib():
    from gnnpn_sc_amd import _lib
    return _lib.load()


def test_descend_pairs_ragged_rejects_bad_arguments():
    lib = _lib()
    names = ("prob_ptr", "cand_ptr", "cand", "bounds", "start_pos", "best_fitness", "start_fitness", "best_pos", "best_rows",
             "round_history", "sweeps", "moves", "rounds", "pair_moves", "converged")

    def call(B=3, n_lists=12, max_slots=5, max_cand=20, max_sweeps=4, max_rounds=2, **null):
        a = {n: (None if n in null else P) for n in names}
        return lib.gnnpn_descend_pairs_ragged_f64(B, a["prob_ptr"], n_lists, max_slots, max_cand, a["cand_ptr"], a["cand"], a["bounds"],
                                                  a["start_pos"], max_sweeps, max_rounds, a["best_fitness"], a["start_fitness"],
                                                  a["best_pos"], a["best_rows"], a["round_history"], a["sweeps"], a["moves"], a["rounds"],
                                                  a["pair_moves"], a["converged"], None)
    for n in names:
        if n != "best_rows":                                # optional, as in gnnpn_descend_ragged_f64
            assert call(**{n: True}) == -1 and b"null" in lib.gnnpn_last_error(), n
    for kw in ({"B": -1}, {"n_lists": -1}, {"max_slots": 0}, {"max_sweeps": -1}, {"max_rounds": -1}):
        assert call(**kw) == -1 and b"bad argument" in lib.gnnpn_last_error(), kw
    assert call(max_slots=65) == -2 and b"gnnpn_descend_ragged_f64" in lib.gnnpn_last_error()      # the lane form only
    assert b"64" in lib.gnnpn_last_error()
    assert call(max_cand=0) == -2 and b"max_cand" in lib.gnnpn_last_error()
    assert call(max_cand=6000) == -2 and b"LDS" in lib.gnnpn_last_error()          # the table exceeds a CU's LDS
    assert call(B=0) == 0 and call(B=0, prob_ptr=True, cand=True) == 0             # an empty batch launches nothing


def test_wrappers_reject_host_tensors_and_signatures():
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.pipeline import ML2PNPipeline, descend_pairs, descend_starts, descend_starts_pairs, refine
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)   # noqa: E731
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        ops.descend_pairs_ragged(i32([0, 2, 3]), i32([0, 1, 2, 3]), f64(3, 4), f64(2, 4), i32([0, 0, 0]), max_slots=2, max_cand=2)
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        ops.descend_pairs_ragged(i32([0, 2, 3]), i32([0, 1, 2, 3]), f64(3, 4), f64(2, 4), i32([0, 0, 0]))
    with pytest.raises(ops.GnnpnError, match="inconsistent"):
        ops.descend_pairs_ragged(i32([0, 2, 3]), i32([0, 1, 2, 3]), f64(3, 4), f64(2, 4), i32([0, 0]))
    with pytest.raises(ops.GnnpnError, match="inconsistent"):
        ops.descend_pairs_ragged(i32([0, 2, 3]), i32([0, 1, 2, 3]), f64(3, 4), f64(2, 4), i32([0, 0, 0]), max_rounds=-1)
    sig = inspect.signature(ops.descend_pairs_ragged)
    assert list(sig.parameters) == ["prob_ptr", "cand_ptr", "cand", "bounds", "start_pos", "max_sweeps", "max_rounds", "max_slots", "max_cand"]
    assert sig.parameters["max_sweeps"].default == 16 and sig.parameters["max_rounds"].default == 4

    class Svc:
        cat_ptr, qos = i32([0, 2, 4, 6]), f64(6, 4)

    class Batch:
        n_problems = 2
        x, seg_ptr = torch.zeros(6, 7), i32([0, 3, 6])
        local_bounds, global_bounds = f64(2, 3, 4), f64(2, 4)
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        descend_pairs(Svc, Batch, {"actions": torch.zeros(2, 3, 8)})
    with pytest.raises(ops.GnnpnError, match="starts"):
        descend_starts_pairs(Svc, Batch, torch.zeros(2, 3, 8))
    sig = inspect.signature(descend_pairs)
    assert list(sig.parameters) == ["services", "batch", "out", "max_sweeps", "max_rounds", "reduct", "min_cost", "patches"]
    assert sig.parameters["max_sweeps"].default == 16 and sig.parameters["max_rounds"].default == 4
    assert list(inspect.signature(ML2PNPipeline.descend_pairs).parameters)[1:] == list(sig.parameters)
    sig = inspect.signature(descend_starts_pairs)
    assert list(sig.parameters) == ["services", "batch", "starts", "max_sweeps", "pair_rounds", "reduct", "min_cost", "patches"]
    assert list(inspect.signature(ML2PNPipeline.descend_starts_pairs).parameters)[1:] == list(sig.parameters)
    assert "pair_rounds" not in inspect.signature(descend_starts).parameters          # it keeps the signature its callers know
    assert inspect.signature(refine).parameters["pair_rounds"].default == 0


def test_pipeline_refuses_more_than_64_slots_naming_descend():
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.pipeline import _descend_tables
    tabs = {"max_slots": 65, "max_cand": 100}
    with pytest.raises(ops.GnnpnError, match=r"65 slots.*descend"):
        _descend_tables(tabs, 16, 4)
    with pytest.raises(ops.GnnpnError, match="rounds"):
        _descend_tables({"max_slots": 5, "max_cand": 10}, 16, -1)


def test_main_cli_refuses_pairs_without_descend(capsys):
    import main as cli
    from gnnpn_sc_amd import ML2PN
    assert cli.main(["main.py", "QWS", "ML+2PN", "-1", "--infer", "--pairs"]) == 1               # before any file is read
    assert cli.main(["main.py", "QWS", "ML+2PN", "-1", "--infer", "--descend", "--pairs=0"]) == 1
    assert capsys.readouterr().out.count("--pairs[=ROUNDS]: needs --descend") == 2
    with pytest.raises(ValueError, match="pair_rounds"):
        ML2PN.infer("QWS", None, None, None, 3, pair_rounds=2)
    assert inspect.signature(ML2PN.infer).parameters["pair_rounds"].default is None


SEEDS = [(1200 + T, (T,), 4, 8) for T in (2, 3, 7, 8, 9)]


@pytest.fixture(scope="module")
def runs():
    """(tables, pair-descent run at the defaults, one-swap run) of the problems the GPU tests use at T in (2, 3, 7, 8, 9)."""
    from test_gpu_woa import _random_problems
    out = []
    for seed, sizes, n, mc in SEEDS:
        g = np.random.default_rng(seed)
        for T in sizes:
            for tab in ref.prepare(_random_problems(g, T, n, mc)):
                out.append((tab, pref.descend_pairs(*tab), ref.descend(*tab)))
    return out


def test_reference_without_rounds_is_the_one_swap_descent(runs):
    for tab, _r, one in runs:
        zero = pref.descend_pairs(*tab, max_rounds=0)
        for k in ("best_fitness", "start_fitness", "best_pos", "best_rows", "sweeps", "moves"):
            assert zero[k] == one[k], k
        assert zero["rounds"] == 0 and zero["pair_moves"] == 0 and zero["converged"] == 0
        assert zero["round_history"] == [one["best_fitness"]]


def test_reference_ends_where_no_swap_and_no_pair_helps(runs):
    for (cats, bounds, _start), r, one in runs:
        T = len(cats)
        assert r["converged"] == 1 and 1 <= r["rounds"] <= 4
        assert ref.improving_swaps(cats, bounds, r["best_pos"], r["best_fitness"]) == []
        assert pref.improving_pairs(cats, bounds, r["best_pos"], r["best_fitness"]) == []
        assert r["best_fitness"] <= one["best_fitness"] and r["start_fitness"] == one["start_fitness"]
        assert r["best_fitness"] == ref.merit([cats[j][r["best_pos"][j]] for j in range(T)], bounds)
        assert r["best_rows"] == [tuple(cats[j][r["best_pos"][j]]) for j in range(T)]
        h = r["round_history"]
        assert len(h) == 4 and all(a >= b for a, b in zip(h, h[1:])) and h[-1] == r["best_fitness"]
        assert (r["pair_moves"] == 0) == (r["rounds"] == 1)        # converged: only a first pair sweep without a move ends at once
        if r["pair_moves"] == 0:
            assert r["best_pos"] == one["best_pos"] and r["sweeps"] == one["sweeps"] and r["moves"] == one["moves"]
        else:
            assert r["best_fitness"] < one["best_fitness"] and r["rounds"] >= 2


def test_reference_runs_are_not_vacuous(runs):
    """Pairs move somewhere in the set (the one-swap optimum sits behind a wall), and somewhere they remove a violation."""
    assert any(r["pair_moves"] > 0 for _t, r, _o in runs)
    assert any(one["best_fitness"] - r["best_fitness"] > 0.5 for _t, r, one in runs)
    assert any(r["rounds"] >= 3 for _t, r, _o in runs)
    assert any(start is None for (_c, _b, start), _r, _o in runs) and any(start is not None for (_c, _b, start), _r, _o in runs)


GOOD, POOR = (0.1, 0.9, 0.99, 0.99), (0.8, 0.2, 0.99, 0.99)


def test_reference_wall_ties_and_cut_off():
    # a wall: slot 0 = LOW keeps column 2's product inside [0.5, 0.6] only beside HIGH; the better rows break the bound singly
    tab = pref.wall_problem()
    one, r = ref.descend(*tab), pref.descend_pairs(*tab)
    assert one["moves"] == 0 and one["best_fitness"] > 1.0
    assert r["pair_moves"] == 1 and one["best_fitness"] - r["best_fitness"] > 0.5 and r["converged"] == 1 and r["rounds"] == 2
    assert pref.improving_pairs(tab[0], tab[1], one["best_pos"], one["best_fitness"]) == [(0, 1, 1, 1)]      # exactly one pair repairs
    twice = pref.descend_pairs(*pref.wall_problem(twice=True))
    assert twice["best_pos"] == r["best_pos"] and twice["pair_moves"] == 1                   # the lower (a, b) of two equal best pairs
    equal = pref.descend_pairs([[GOOD, GOOD], [POOR, POOR]], [0.5, 1.0, 0.5, 1.0], [1, 1])
    assert equal["best_pos"] == [1, 1] and equal["pair_moves"] == 0 and equal["rounds"] == 1 and equal["converged"] == 1
    sweeps_off = pref.descend_pairs(*tab, max_sweeps=0)                                      # pair sweeps only
    assert sweeps_off["sweeps"] == 0 and sweeps_off["moves"] == 0 and sweeps_off["pair_moves"] == 1 and sweeps_off["converged"] == 0
    assert sweeps_off["best_fitness"] == r["best_fitness"]
    one_round = pref.descend_pairs(*tab, max_rounds=1)
    assert one_round["rounds"] == 1 and one_round["converged"] == 0 and one_round["round_history"] == [r["best_fitness"]]
