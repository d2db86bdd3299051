"""-m "not gpu": multi-start descent — the replica forms of the candidate-table entries and gnnpn_descend_select_f64 reject bad
arguments before any launch, the wrappers refuse host tensors, the public signatures are the documented ones, and the reference of the
GPU tests (tests/multistart_reference.py) has the properties that make those comparisons mean something."""
import ctypes
import inspect
import math

import pytest
import torch

import multistart_reference as mref

P = ctypes.c_void_p(64)          # a non-null, 8-aligned stand-in: every call below fails before it is dereferenced
ODD = ctypes.c_void_p(66)        # non-null, aligned to 2 only


def _lib():
    from gnnpn_sc_amd import _lib
    return _lib.load()


COUNT_PTRS = ("x", "seg_ptr", "local_bounds", "global_bounds", "cat_ptr", "qos", "actions", "patches", "workspace", "prob_ptr", "n_slots",
              "bounds", "status", "totals")


def _count(lib, B=3, R=2, n_nodes=12, x_ld=7, n_cat=5, actions_f64=1, actions_T=5, n_patches=0, max_cat=9, ws_bytes=None, **ptr):
    a = {n: P for n in COUNT_PTRS}
    a.update(ptr)
    if ws_bytes is None:
        ws_bytes = max(int(lib.gnnpn_woa_candidates_replicas_workspace_bytes(B, R, n_nodes, max_cat)), 0)
    return lib.gnnpn_woa_candidates_replicas_count(B, R, n_nodes, a["x"], x_ld, a["seg_ptr"], a["local_bounds"], a["global_bounds"], n_cat,
                                                   a["cat_ptr"], a["qos"], a["actions"], actions_f64, actions_T, 0.0, a["patches"], n_patches,
                                                   max_cat, a["workspace"], ws_bytes, a["prob_ptr"], a["n_slots"], a["bounds"], a["status"],
                                                   a["totals"], None)


FILL_PTRS = ("seg_ptr", "cat_ptr", "qos", "workspace", "status", "prob_ptr", "cand_ptr", "len_init", "cand", "start_pos")


def _fill(lib, B=3, R=2, n_nodes=12, max_cat=9, n_lists=4, n_cand=9, ws_bytes=None, **ptr):
    a = {n: P for n in FILL_PTRS}
    a.update(ptr)
    if ws_bytes is None:
        ws_bytes = max(int(lib.gnnpn_woa_candidates_replicas_workspace_bytes(B, R, n_nodes, max_cat)), 0)
    return lib.gnnpn_woa_candidates_replicas_fill(B, R, n_nodes, a["seg_ptr"], a["cat_ptr"], a["qos"], max_cat, a["workspace"], ws_bytes,
                                                  a["status"], a["prob_ptr"], n_lists, n_cand, a["cand_ptr"], a["len_init"], a["cand"],
                                                  a["start_pos"], None)


def test_replica_workspace_size():
    lib = _lib()
    one = lib.gnnpn_woa_candidates_workspace_bytes
    rep = lib.gnnpn_woa_candidates_replicas_workspace_bytes
    for B, N, cap in ((0, 0, 0), (3, 12, 9), (256, 2900, 120)):
        assert rep(B, 1, N, cap) == one(B, N, cap) >= 0                   # the R = 1 call of the same size formula
        assert rep(B, 4, N, cap) == one(4 * B, 4 * N, cap)                # rows and (replica, node) pairs both scale by R
    assert rep(3, 0, 12, 9) == rep(3, -1, 12, 9) == rep(-1, 2, 12, 9) == rep(3, 2, -1, 9) == rep(3, 2, 12, -1) == -1
    assert rep(2 ** 30, 2, 12, 9) == rep(3, 2 ** 20, 2 ** 12, 9) == -1    # B * R, n_nodes * R beyond int32
    assert rep(2 ** 30, 1, 12, 9) > 0


def test_replica_count_rejects_bad_arguments():
    lib = _lib()
    for kw in ({"R": 0}, {"R": -3}, {"B": -1}, {"n_nodes": -1}, {"x_ld": 0}, {"n_cat": 0}, {"actions_T": 0}, {"n_patches": -1},
               {"max_cat": -1}, {"actions_f64": 2}):
        assert _count(lib, **kw) == -1 and b"woa_candidates_replicas_count: bad argument" in lib.gnnpn_last_error(), kw
    for kw in ({"B": 2 ** 30, "R": 2}, {"n_nodes": 2 ** 30, "R": 2}):
        assert _count(lib, ws_bytes=2 ** 40, **kw) == -1 and b"exceed int32" in lib.gnnpn_last_error(), kw
    for n in COUNT_PTRS:
        if n not in ("patches", "workspace"):
            assert _count(lib, **{n: None}) == -1 and b"null operand" in lib.gnnpn_last_error(), n
    assert _count(lib, n_patches=1, patches=None) == -1 and b"null patches" in lib.gnnpn_last_error()
    need = int(lib.gnnpn_woa_candidates_replicas_workspace_bytes(3, 2, 12, 9))
    assert need > int(lib.gnnpn_woa_candidates_workspace_bytes(3, 12, 9))
    assert _count(lib, ws_bytes=need - 1) == -1 and f"{need} B needed".encode() in lib.gnnpn_last_error()
    assert _count(lib, ws_bytes=int(lib.gnnpn_woa_candidates_workspace_bytes(3, 12, 9))) == -1     # sized for one replica
    assert _count(lib, workspace=None) == -1 and b"workspace" in lib.gnnpn_last_error()
    assert _count(lib, workspace=ODD) == -1 and b"misaligned workspace" in lib.gnnpn_last_error()
    assert _count(lib, actions_T=1025) == -2 and b"at most 1024" in lib.gnnpn_last_error()


def test_replica_fill_rejects_bad_arguments():
    lib = _lib()
    for kw in ({"R": 0}, {"B": -1}, {"n_nodes": -1}, {"max_cat": -1}, {"n_lists": -1}, {"n_cand": -1}):
        assert _fill(lib, **kw) == -1 and b"woa_candidates_replicas_fill: bad argument" in lib.gnnpn_last_error(), kw
    assert _fill(lib, B=2 ** 30, R=2, ws_bytes=2 ** 40) == -1 and b"exceed int32" in lib.gnnpn_last_error()
    for n in FILL_PTRS:
        if n != "workspace":
            assert _fill(lib, **{n: None}) == -1 and b"null operand" in lib.gnnpn_last_error(), n
    need = int(lib.gnnpn_woa_candidates_replicas_workspace_bytes(3, 2, 12, 9))
    for kw in ({"ws_bytes": need - 1}, {"workspace": None}, {"workspace": ODD}):
        assert _fill(lib, **kw) == -1 and b"workspace" in lib.gnnpn_last_error(), kw
    assert _fill(lib, B=0, seg_ptr=None, qos=None, workspace=None, ws_bytes=0) == 0          # an empty batch launches nothing


SELECT_IN = ("best_fitness", "start_fitness", "sweeps", "moves", "n_slots", "best_pos", "best_rows", "history", "actions")
SELECT_OUT = tuple(n + "_out" for n in SELECT_IN) + ("start_index",)


def _select(lib, B=3, R=2, max_slots=5, hist_ld=4, actions_T=5, words=8, **ptr):
    a = {n: P for n in SELECT_IN + SELECT_OUT}
    a.update(ptr)
    return lib.gnnpn_descend_select_f64(B, R, max_slots, hist_ld, actions_T, words, *(a[n] for n in SELECT_IN),
                                        *(a[n] for n in ("best_fitness_out", "start_fitness_out", "sweeps_out", "moves_out", "n_slots_out",
                                                         "best_pos_out", "best_rows_out", "history_out", "actions_out", "start_index")), None)


def test_select_rejects_bad_arguments():
    lib = _lib()
    for kw in ({"R": 0}, {"R": -1}, {"B": -1}, {"max_slots": 0}, {"hist_ld": -1}, {"actions_T": -1}, {"words": 0}):
        assert _select(lib, **kw) == -1 and b"descend_select: bad argument" in lib.gnnpn_last_error(), kw
    assert _select(lib, B=2 ** 16, R=2 ** 15) == -1 and b"exceed int32" in lib.gnnpn_last_error()
    for n in SELECT_IN + SELECT_OUT:
        assert _select(lib, **{n: None}) == -1 and b"null operand" in lib.gnnpn_last_error(), n
    assert _select(lib, actions=ctypes.c_void_p(66)) == -1 and b"misaligned" in lib.gnnpn_last_error()
    assert _select(lib, B=0) == 0 and _select(lib, B=0, best_fitness=None, start_index=None) == 0      # an empty batch launches nothing


def test_wrappers_refuse_host_tensors_and_signatures():
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.modelPN import two_level_best_of
    from gnnpn_sc_amd.pipeline import ML2PNPipeline, descend, descend_starts
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)      # noqa: E731
    cat_ptr, qos, x, seg = i32([0, 2, 4, 6]), f64(6, 4), torch.zeros(6, 7), i32([0, 3, 6])
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        ops.woa_candidates_replicas(cat_ptr, qos, x, seg, f64(2, 3, 4), f64(2, 4), torch.zeros(2, 4, 3, 8))
    with pytest.raises(ops.GnnpnError, match=r"\[B=2, R >= 1, T, 8\]"):
        ops.woa_candidates_replicas(cat_ptr, qos, x, seg, f64(2, 3, 4), f64(2, 4), torch.zeros(2, 3, 8))
    res = {"best_fitness": f64(4), "start_fitness": f64(4), "best_pos": torch.zeros(4, 3, dtype=torch.int32), "best_rows": f64(4, 3, 4),
           "history": f64(4, 16), "sweeps": i32([1] * 4), "moves": i32([0] * 4)}
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        ops.descend_select(res, torch.zeros(2, 2, 3, 8), i32([3] * 4))
    with pytest.raises(ops.GnnpnError, match="2 x 3 rows"):
        ops.descend_select(res, torch.zeros(2, 3, 3, 8), i32([3] * 4))

    class Svc:
        pass

    class Batch:
        n_problems = 2
        local_bounds, global_bounds = f64(2, 3, 4), f64(2, 4)
    Svc.cat_ptr, Svc.qos, Batch.x, Batch.seg_ptr = cat_ptr, qos, x, seg
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        descend_starts(Svc, Batch, {"actions_all": torch.zeros(2, 4, 3, 9)})
    with pytest.raises(ops.GnnpnError, match=r"\[B, N, T, 8\|9\]"):
        descend_starts(Svc, Batch, torch.zeros(2, 3, 8))
    sig = inspect.signature(descend_starts)
    assert list(sig.parameters) == ["services", "batch", "starts", "max_sweeps", "reduct", "min_cost", "patches"]
    assert sig.parameters["max_sweeps"].default == 16 and sig.parameters["reduct"].default == 0
    assert sig.parameters["min_cost"].default is None and sig.parameters["patches"].default == ()
    assert list(inspect.signature(ML2PNPipeline.descend_starts).parameters)[1:] == list(sig.parameters)
    assert inspect.signature(ML2PNPipeline.best_of).parameters["return_all"].default is False
    assert inspect.signature(two_level_best_of).parameters["return_all"].default is False
    assert list(inspect.signature(descend).parameters) == ["services", "batch", "out", "max_sweeps", "reduct", "min_cost", "patches"]
    for name in ("gnnpn_woa_candidates_replicas_workspace_bytes", "gnnpn_woa_candidates_replicas_count", "gnnpn_woa_candidates_replicas_fill",
                 "gnnpn_descend_select_f64"):
        from gnnpn_sc_amd import _lib
        assert name in _lib.EXPORTS
    assert _lib.load().gnnpn_abi_version() == 9


def test_main_refuses_all_starts_without_samples_and_descend(capsys):
    import main as cli
    for argv in (["--all-starts"], ["--all-starts", "--samples=4"], ["--all-starts", "--descend"], ["--all-starts", "--samples=1", "--descend"]):
        assert cli.main(["main.py", "QWS", "ML+2PN", "-1", "--infer"] + argv) != 0, argv
        out = capsys.readouterr().out.strip().splitlines()
        assert len(out) == 1 and "--all-starts" in out[0], (argv, out)


def test_select_rule():
    rows = lambda *f: [{"best_fitness": v} for v in f]      # noqa: E731
    nan = math.nan
    assert mref.select(rows(0.5)) == 0
    assert mref.select(rows(0.5, 0.25, 0.25)) == 1                   # the lowest replica among equals
    assert mref.select(rows(nan, 0.5, nan, 0.25)) == 3               # a NaN never wins, below or above the winner
    assert mref.select(rows(nan, nan)) == 0                          # nothing searched: replica 0
    assert mref.select(rows(0.0, -0.0)) == 0 and mref.select(rows(-0.0, 0.0)) == 0
    assert mref.select(rows(math.inf, nan)) == 0 and mref.select(rows(nan, math.inf)) == 1


RAGGED = (606, (1, 9, 64, 65, 3, 129), 4, 5, True)      # the ragged mixture of tests/test_gpu_multistart.py


def test_the_ragged_cases_are_not_vacuous():
    tables, runs = mref.replica_tables(*RAGGED), mref.replica_runs(*RAGGED)
    assert len(tables) == 24 and all(len(reps) == 5 for reps in tables)
    assert any(r["start_index"] >= 1 for r in runs)                                      # a problem won by a replica >= 1
    assert any(sorted(r["fitness_all"])[0] == sorted(r["fitness_all"])[1] for r in runs)  # an exact tie at the minimum
    assert any(reps[0][2] is None for reps in tables)                                     # a problem without a start
    from test_gpu_woa import _random_problems      # a foreign pick: replica 0's list is longer than the problem's service list
    import numpy as np
    g = np.random.default_rng(RAGGED[0])
    problems = []
    for T in RAGGED[1]:
        problems += _random_problems(g, T, RAGGED[2])
    problems = [problems[i] for i in g.permutation(len(problems))]
    assert any(len(c) > len(s) for (services, _c, _s), reps in zip(problems, tables) for c, s in zip(reps[0][0], services))
    for reps, r in zip(tables, runs):
        w = r["start_index"]
        assert r["best_fitness"] == min(r["fitness_all"]) == r["fitness_all"][w] and w == r["fitness_all"].index(r["best_fitness"])
        assert r["best_fitness"] <= r["fitness_all"][0]                                   # never worse than the first start alone
        assert len(reps[w][0]) == len(r["best_pos"])
