"""-m "not gpu": the entry points of the device-side ES-WOA refinement (gnnpn_woa_candidates_count / _fill,
gnnpn_eswoa_ragged_f64, gnnpn_debug_round5_f64) reject bad arguments before any launch, and their Python wrappers refuse
host tensors (no CPU path)."""
import ctypes

import pytest
import torch

P = ctypes.c_void_p(64)          # a non-null stand-in: every call below fails before it is dereferenced


def _lib():
    from gnnpn_sc_amd import _lib
    return _lib.load()


def test_candidates_count_rejects_bad_arguments():
    lib = _lib()
    ws = int(lib.gnnpn_woa_candidates_workspace_bytes(4, 40, 10))
    assert ws > 0 and lib.gnnpn_woa_candidates_workspace_bytes(-1, 40, 10) < 0
    good = dict(B=4, N=40, x=P, x_ld=7, seg=P, lb=P, gb=P, n_cat=5, cat_ptr=P, qos=P, act=P, f64=0, aT=5, reduct=0.0,
                patches=None, n_patches=0, max_cat=10, ws=P, ws_bytes=ws, prob_ptr=P, n_slots=P, bounds=P, status=P, totals=P)

    def call(**kw):
        a = dict(good, **kw)
        return lib.gnnpn_woa_candidates_count(a["B"], a["N"], a["x"], a["x_ld"], a["seg"], a["lb"], a["gb"], a["n_cat"], a["cat_ptr"],
                                              a["qos"], a["act"], a["f64"], a["aT"], a["reduct"], a["patches"], a["n_patches"],
                                              a["max_cat"], a["ws"], a["ws_bytes"], a["prob_ptr"], a["n_slots"], a["bounds"],
                                              a["status"], a["totals"], None)
    for kw in ({"x": None}, {"seg": None}, {"act": None}, {"totals": None}, {"ws": None}, {"n_patches": 1}):
        assert call(**kw) == -1, kw
        assert b"null" in lib.gnnpn_last_error() or b"workspace" in lib.gnnpn_last_error()
    for kw in ({"B": -1}, {"x_ld": 0}, {"n_cat": 0}, {"aT": 0}, {"f64": 2}, {"max_cat": -1}):
        assert call(**kw) == -1, kw
        assert b"bad argument" in lib.gnnpn_last_error()
    assert call(ws_bytes=ws - 1) == -1 and b"workspace" in lib.gnnpn_last_error()
    assert call(aT=5000) == -2                          # more action rows per problem than the builder's LDS holds


def test_candidates_fill_rejects_bad_arguments():
    lib = _lib()
    ws = int(lib.gnnpn_woa_candidates_workspace_bytes(4, 40, 10))

    def call(B=4, seg=P, status=P, cand_ptr=P, cand=P, n_lists=8, n_cand=30, ws_bytes=ws, max_cat=10):
        return lib.gnnpn_woa_candidates_fill(B, 40, seg, P, P, max_cat, P, ws_bytes, status, P, n_lists, n_cand, cand_ptr, P, cand,
                                             P, None)
    assert call(seg=None) == -1 and b"null" in lib.gnnpn_last_error()
    assert call(cand_ptr=None) == -1 and b"null" in lib.gnnpn_last_error()
    assert call(cand=None) == -1 and b"null" in lib.gnnpn_last_error()
    assert call(n_cand=-1) == -1 and b"bad argument" in lib.gnnpn_last_error()
    assert call(ws_bytes=ws - 8) == -1 and b"workspace" in lib.gnnpn_last_error()


def test_eswoa_ragged_rejects_bad_arguments():
    lib = _lib()

    def call(B=3, prob_ptr=P, n_lists=12, max_slots=5, max_cand=20, cand=P, pop=4, max_iter=3, wide=0, ws=None, ws_bytes=0,
             best_pos=P):
        return lib.gnnpn_eswoa_ragged_f64(B, prob_ptr, n_lists, max_slots, max_cand, P, P, cand, P, P, pop, max_iter, P, wide, ws,
                                          ws_bytes, P, best_pos, None, P, P, None)
    assert call(prob_ptr=None) == -1 and b"null" in lib.gnnpn_last_error()
    assert call(cand=None) == -1 and b"null" in lib.gnnpn_last_error()
    assert call(best_pos=None) == -1 and b"null" in lib.gnnpn_last_error()
    for kw in ({"B": -1}, {"n_lists": -1}, {"max_slots": 0}, {"pop": 0}, {"max_iter": -1}):
        assert call(**kw) == -1 and b"bad argument" in lib.gnnpn_last_error(), kw
    assert call(max_cand=0) == -1                       # the lane-per-category form sizes its LDS by it
    need = int(lib.gnnpn_eswoa_ragged_workspace_bytes(12, 5, 4, 1))
    assert need == 12 * 4 * 4 and lib.gnnpn_eswoa_ragged_workspace_bytes(12, 5, 4, 0) == 0
    assert lib.gnnpn_eswoa_ragged_workspace_bytes(12, 65, 4, 0) == 12 * 4 * 4      # above 64 categories: the workgroup form
    assert call(wide=1) == -1 and b"workspace" in lib.gnnpn_last_error()
    assert call(wide=1, ws=P, ws_bytes=need - 4) == -1 and b"workspace" in lib.gnnpn_last_error()
    assert call(max_slots=7000, ws=P, ws_bytes=10 ** 9) == -2                      # three float64 columns of 7000 exceed a CU's LDS
    assert call(max_cand=5000, pop=100) == -2                                        # the lane form's table exceeds a CU's LDS


def test_debug_round5_rejects_bad_arguments():
    lib = _lib()
    assert lib.gnnpn_debug_round5_f64(None, P, 3, None) == -1 and b"null" in lib.gnnpn_last_error()
    assert lib.gnnpn_debug_round5_f64(P, P, -1, None) == -1
    assert lib.gnnpn_debug_round5_f64(None, None, 0, None) == 0      # an empty batch launches nothing


def test_wrappers_reject_host_tensors():
    from gnnpn_sc_amd import ops
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        ops.debug_round5(torch.zeros(4, dtype=torch.float64))
    B, T, N = 2, 3, 6
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        ops.woa_candidates(torch.tensor([0, 2, 4, 6], dtype=torch.int32), torch.zeros(6, 4, dtype=torch.float64),
                           torch.zeros(N, 7), torch.tensor([0, 3, 6], dtype=torch.int32), torch.zeros(B, T, 4, dtype=torch.float64),
                           torch.zeros(B, 4, dtype=torch.float64), torch.zeros(B, T, 8))
    with pytest.raises(ops.GnnpnError, match="actions"):
        ops.woa_candidates(torch.tensor([0, 2, 4, 6], dtype=torch.int32), torch.zeros(6, 4, dtype=torch.float64),
                           torch.zeros(N, 7), torch.tensor([0, 3, 6], dtype=torch.int32), torch.zeros(B, T, 4, dtype=torch.float64),
                           torch.zeros(B, 4, dtype=torch.float64), torch.zeros(B, T, 4))
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        ops.eswoa_ragged(torch.tensor([0, 2, 3], dtype=torch.int32), torch.tensor([0, 1, 2, 3], dtype=torch.int32),
                         torch.ones(3, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.float64),
                         torch.zeros(3, dtype=torch.int32), 4, 2, torch.zeros(2, dtype=torch.int64), max_slots=2, max_cand=2)


def test_refine_is_an_extra_call():
    """refine exists beside run / capture and takes the arguments the issue of the feature names."""
    import inspect
    from gnnpn_sc_amd.pipeline import ML2PNPipeline
    sig = inspect.signature(ML2PNPipeline.refine)
    assert list(sig.parameters)[1:] == ["services", "batch", "out", "popSize", "MAX_Iter", "reduct", "seeds", "min_cost", "patches"]
    assert sig.parameters["reduct"].default == 0 and sig.parameters["patches"].default == ()
