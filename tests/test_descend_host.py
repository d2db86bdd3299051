"""-m "not gpu": the one-swap descent (gnnpn_descend_ragged_f64, ops.descend_ragged, pipeline.descend) rejects bad arguments and
host tensors before any launch, and the plain-Python reference the GPU tests compare with (tests/descent_reference.py) has the
properties that make those comparisons meaningful."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import descent_reference as ref

P = ctypes.c_void_p(64)          # a non-null stand-in: every call below fails before it is dereferenced


def _lib():
    from gnnpn_sc_amd import _lib
    return _lib.load()


def test_descend_ragged_rejects_bad_arguments():
    lib = _lib()
    names = ("prob_ptr", "cand_ptr", "cand", "bounds", "start_pos", "best_fitness", "start_fitness", "best_pos", "best_rows", "history",
             "sweeps", "moves")

    def call(B=3, n_lists=12, max_slots=5, max_cand=20, max_sweeps=4, wide=0, **null):
        a = {n: (None if n in null else P) for n in names}
        return lib.gnnpn_descend_ragged_f64(B, a["prob_ptr"], n_lists, max_slots, max_cand, a["cand_ptr"], a["cand"], a["bounds"],
                                            a["start_pos"], max_sweeps, wide, a["best_fitness"], a["start_fitness"], a["best_pos"],
                                            a["best_rows"], a["history"], a["sweeps"], a["moves"], None)
    for n in names:
        if n != "best_rows":                                # optional, as in gnnpn_eswoa_ragged_f64
            assert call(**{n: True}) == -1 and b"null" in lib.gnnpn_last_error(), n
    for kw in ({"B": -1}, {"n_lists": -1}, {"max_slots": 0}, {"max_sweeps": -1}):
        assert call(**kw) == -1 and b"bad argument" in lib.gnnpn_last_error(), kw
    assert call(max_cand=0) == -1 and b"max_cand" in lib.gnnpn_last_error()          # the lane form sizes its LDS by it
    assert call(B=0) == 0 and call(B=0, prob_ptr=True, cand=True) == 0             # an empty batch launches nothing
    assert call(max_cand=6000) == -2 and b"wide" in lib.gnnpn_last_error()          # the lane form's table exceeds a CU's LDS
    assert call(max_slots=7000) == -2                                              # four float64 columns of 7000 slots do too


def test_wrappers_reject_host_tensors():
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.pipeline import ML2PNPipeline, descend, refine
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        ops.descend_ragged(i32([0, 2, 3]), i32([0, 1, 2, 3]), torch.zeros(3, 4, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.float64),
                           i32([0, 0, 0]), max_slots=2, max_cand=2)
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        ops.descend_ragged(i32([0, 2, 3]), i32([0, 1, 2, 3]), torch.zeros(3, 4, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.float64),
                           i32([0, 0, 0]))
    with pytest.raises(ops.GnnpnError, match="inconsistent"):
        ops.descend_ragged(i32([0, 2, 3]), i32([0, 1, 2, 3]), torch.zeros(3, 4, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.float64),
                           i32([0, 0]))

    class Svc:
        cat_ptr, qos = i32([0, 2, 4, 6]), torch.zeros(6, 4, dtype=torch.float64)

    class Batch:
        n_problems = 2
        x, seg_ptr = torch.zeros(6, 7), i32([0, 3, 6])
        local_bounds, global_bounds = torch.zeros(2, 3, 4, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.float64)
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        descend(Svc, Batch, {"actions": torch.zeros(2, 3, 8)})
    sig = inspect.signature(descend)
    assert list(sig.parameters) == ["services", "batch", "out", "max_sweeps", "reduct", "min_cost", "patches"]
    assert sig.parameters["max_sweeps"].default == 16
    assert list(inspect.signature(ML2PNPipeline.descend).parameters)[1:] == list(sig.parameters)
    assert inspect.signature(refine).parameters["descend"].default == 0


def test_write_ml2pn_woa_takes_a_file_name(tmp_path, monkeypatch, capsys):
    import json
    from gnnpn_sc_amd.WOA import write_ml2pn_woa
    monkeypatch.chdir(tmp_path)
    a = write_ml2pn_woa("QWS", [0.5, 0.25], 0.1, 30)
    b = write_ml2pn_woa("QWS", [0.5, 0.25], 0.1, 30, name="ML+2PN+descent.txt")
    capsys.readouterr()
    with open("./solutions/WOA/QWS/ML+2PN+WOA.txt") as f, open("./solutions/WOA/QWS/ML+2PN+descent.txt") as g:
        assert json.load(f) == a == b == json.load(g)


@pytest.fixture(scope="module")
def runs():
    """(tables, reference run at 16 sweeps) of _random_problems(default_rng(5), T, 4) for T in (7, 8, 9, 33, 64)."""
    from test_gpu_woa import _random_problems
    g = np.random.default_rng(5)
    out = []
    for T in (7, 8, 9, 33, 64):
        for tab in ref.prepare(_random_problems(g, T, 4)):
            out.append((tab, ref.descend(*tab, max_sweeps=16)))
    return out


def test_reference_descends_to_a_one_swap_optimum(runs):
    for (cats, bounds, start), r in runs:
        T = len(cats)
        h = r["history"]
        assert len(h) == 16 and all(a >= b for a, b in zip(h, h[1:]))
        assert r["best_fitness"] <= r["start_fitness"] and r["best_fitness"] == h[-1]
        assert all(v == r["best_fitness"] for v in h[r["sweeps"] - 1:])          # no uninitialised tail
        assert r["start_fitness"] == ref.merit([cats[j][(start or [0] * T)[j]] for j in range(T)], bounds)
        assert r["best_fitness"] == ref.merit([cats[j][r["best_pos"][j]] for j in range(T)], bounds)
        assert r["best_rows"] == [tuple(cats[j][r["best_pos"][j]]) for j in range(T)]
        assert 1 <= r["sweeps"] <= 16 and (r["moves"] == 0) == (r["sweeps"] == 1 and r["best_pos"] == (start or [0] * T))
        if r["sweeps"] < 16:                                                     # converged: no single swap lowers the result
            assert ref.improving_swaps(cats, bounds, r["best_pos"], r["best_fitness"]) == []


def test_reference_runs_are_not_vacuous(runs):
    """What keeps the GPU comparisons from being trivial: most problems move, and some need three sweeps or more."""
    moved = sum(1 for _t, r in runs if r["moves"] > 0)
    assert 2 * moved >= len(runs), moved
    assert any(r["sweeps"] >= 3 for _t, r in runs)
    assert any(start is None for (_c, _b, start), _r in runs) and any(start is not None for (_c, _b, start), _r in runs)


def test_reference_cut_off_and_ties():
    (cats, bounds, start), full = next((t, r) for t, r in _three_sweeps())
    one = ref.descend(cats, bounds, start, max_sweeps=1)
    assert one["sweeps"] == 1 and one["history"] == [full["history"][0]] and one["moves"] > 0
    zero = ref.descend(cats, bounds, start, max_sweeps=0)
    assert zero["sweeps"] == 0 and zero["moves"] == 0 and zero["history"] == [] and zero["best_fitness"] == zero["start_fitness"]
    good, poor = (0.1, 0.9, 0.99, 0.99), (0.8, 0.2, 0.99, 0.99)
    twice = ref.descend([[poor, good, poor, good], [poor]], [0.5, 1.0, 0.5, 1.0], [0, 0])
    assert twice["best_pos"] == [1, 0] and twice["moves"] == 1                   # the lower of two equal best rows
    equal = ref.descend([[good, good], [poor]], [0.5, 1.0, 0.5, 1.0], [1, 0])
    assert equal["best_pos"] == [1, 0] and equal["moves"] == 0 and equal["sweeps"] == 1      # an equal merit is no move


def _three_sweeps():
    from test_gpu_woa import _random_problems
    g = np.random.default_rng(5)
    for tab in ref.prepare(_random_problems(g, 7, 4)):
        r = ref.descend(*tab, max_sweeps=16)
        if r["sweeps"] >= 3:
            yield tab, r
