"""-m "not gpu": the training-step wrappers and entry points without a GPU — empty gemm shapes follow torch.mm, and the
argument checks that come before any device access (wrapper checks on CPU tensors, C checks on non-null stand-ins) raise."""
import ctypes

import pytest
import torch

P = ctypes.c_void_p(64)          # a non-null stand-in: every call below fails before it is dereferenced
E_ARG, E_UNSUP = -1, -2


def _lib():
    from gnnpn_sc_amd import _lib
    return _lib, _lib.load()


@pytest.mark.parametrize("a_kmajor", [False, True])
@pytest.mark.parametrize("b_kmajor", [False, True])
@pytest.mark.parametrize("M,N,K", [(0, 5, 4096), (5, 0, 4096), (0, 5, 100), (5, 0, 100), (0, 0, 4096), (3, 4, 0), (200, 65, 0)])
def test_gemm_empty_shapes_follow_torch_mm(M, N, K, a_kmajor, b_kmajor):
    from gnnpn_sc_amd import ops
    a = torch.empty((K, M) if a_kmajor else (M, K))
    b = torch.empty((K, N) if b_kmajor else (N, K))
    c = ops.gemm(a, b, a_kmajor, b_kmajor)               # no launch, no ZeroDivisionError
    assert c.shape == (M, N) and c.dtype == torch.float32
    assert torch.equal(c, torch.zeros(M, N))             # torch.mm: K = 0 gives zeros
    assert torch.equal(c, torch.mm(a.t() if a_kmajor else a, (b.t() if b_kmajor else b).t()))


def test_gemm_checks_before_launch():
    from gnnpn_sc_amd import ops
    with pytest.raises(ops.GnnpnError, match="K mismatch"):
        ops.gemm(torch.empty(0, 4), torch.empty(5, 3))
    with pytest.raises(ops.GnnpnError, match="float32"):
        ops.gemm(torch.empty(0, 4, dtype=torch.float64), torch.empty(5, 4))
    with pytest.raises(ops.GnnpnError, match="CUDA"):
        ops.gemm(torch.ones(3, 4), torch.ones(5, 4))     # a non-empty product has no CPU path
    # the split choice: one slice below K = 2048 or from 256 tiles on, at most 64; (200, 65, 60160) leaves slice 63 empty
    assert ops.gemm_split(200, 65, 2047) == 1 and ops.gemm_split(1024, 1024, 60160) == 1
    assert ops.gemm_split(200, 65, 60160) == 64
    k_chunk = -(-(-(-60160 // 64)) // 32) * 32
    assert k_chunk == 960 and 63 * k_chunk >= 60160
    _, lib = _lib()
    for M, N, K, split, ldc in ((4, 0, 8, 1, 1), (4, 5, 0, 1, 5), (-1, 5, 8, 1, 5), (4, 5, 8, 0, 5), (4, 5, 8, 1025, 5), (4, 5, 8, 1, 4)):
        assert lib.gnnpn_gemm_f32(P, 8, 0, P, 8, 0, P, ldc, M, N, K, split, None) == E_ARG
    assert lib.gnnpn_gemm_f32(P, 7, 0, P, 8, 0, P, 5, 4, 5, 8, 1, None) == E_ARG       # lda < K
    assert lib.gnnpn_gemm_f32(P, 3, 1, P, 8, 0, P, 5, 4, 5, 8, 1, None) == E_ARG       # k-major lda < M
    assert lib.gnnpn_gemm_f32(P, 8, 0, P, 4, 1, P, 5, 4, 5, 8, 1, None) == E_ARG       # k-major ldb < N


def test_colsum_checks_extent_before_launch():
    from gnnpn_sc_amd import ops
    x = torch.zeros(10, 8)
    with pytest.raises(ops.GnnpnError, match="ld"):
        ops.colsum(x, rows=10, cols=8, ld=7)             # ld < cols
    with pytest.raises(ops.GnnpnError, match="need"):
        ops.colsum(x, rows=10, cols=8, ld=9)             # 9 * 9 + 8 = 89 > 80
    with pytest.raises(ops.GnnpnError, match="need"):
        ops.colsum(x, rows=11)
    with pytest.raises(ops.GnnpnError, match="need"):
        ops.colsum(torch.zeros(5000, 4), rows=5001)      # the two-pass form checks too
    with pytest.raises(ops.GnnpnError, match="cols"):
        ops.colsum(x, rows=10, cols=0)
    with pytest.raises(ops.GnnpnError, match="CUDA"):
        ops.colsum(x, rows=10, cols=8, ld=8)             # a fitting extent gets as far as the device check
    with pytest.raises(ops.GnnpnError, match="CUDA"):
        ops.colsum(x, rows=8, cols=1, ld=10)             # (8 - 1) * 10 + 1 = 71 <= 80
    with pytest.raises(ops.GnnpnError, match="CUDA"):
        ops.colsum(torch.zeros(0, 8))                     # no rows: zeros, once x passes the device check
    assert ops.colsum_chunking(4095) is None
    for rows in (4096, 4097, 70000):
        per, chunks = ops.colsum_chunking(rows)
        assert (chunks - 1) * per < rows <= chunks * per and chunks <= 128
    _, lib = _lib()
    assert lib.gnnpn_colsum_f32(P, 7, 10, 8, P, None) == E_ARG
    assert lib.gnnpn_colsum_chunks_f32(P, 7, 10, 8, 4, P, None) == E_ARG
    assert lib.gnnpn_colsum_chunks_f32(P, 8, 10, 8, 0, P, None) == E_ARG
    assert lib.gnnpn_colsum_chunks_f32(P, 8, 0, 8, 4, P, None) == 0     # no rows, no chunk: nothing launched


def test_precision_at_k_and_attention_logits_check_before_launch():
    from gnnpn_sc_amd import ops
    ranking, labels = torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 8)
    for ks in ((0,), (1, 0), (-1,), ()):
        with pytest.raises(ops.GnnpnError, match="k must be >= 1"):
            ops.precision_at_k(ranking, labels, ks)
    with pytest.raises(ops.GnnpnError, match="ranking"):
        ops.precision_at_k(ranking, labels, (1, 6))      # reads min(6, 8) = 6 entries of a 5-wide ranking
    with pytest.raises(ops.GnnpnError, match="CUDA"):
        ops.precision_at_k(ranking, labels[:, :5].contiguous(), (1, 9))   # k > S reads S entries only
    enc, q, idx = torch.zeros(2, 6, 8), torch.zeros(2, 3, 8), torch.zeros(2, 3, dtype=torch.int32)
    for step in (-1, 3, 4):
        with pytest.raises(ops.GnnpnError, match="step"):
            ops.attention_logits(enc, q, step, idx)
    with pytest.raises(ops.GnnpnError, match="queries"):
        ops.attention_logits(enc, torch.zeros(2, 3, 4), 0, idx)
    with pytest.raises(ops.GnnpnError, match="idx"):
        ops.attention_logits(enc, q, 1, idx[:, :2].contiguous())
    with pytest.raises(ops.GnnpnError, match="queries: expected a CUDA"):
        ops.attention_logits(enc, q, 2, idx)             # queries are validated like every operand
    _, lib = _lib()
    assert lib.gnnpn_precision_at_k(P, 5, P, 8, 2, 8, None, 1, P, None) == E_ARG      # null ks


def test_train_entry_points_reject_before_launch():
    lib_mod, lib = _lib()
    # BatchNorm on batch statistics needs two rows (torch raises on one)
    assert lib.gnnpn_bn_train_forward_f32(P, 1, 4, P, P, 1e-5, 0.1, 0, P, P, P, None, None, None) == E_ARG
    assert lib.gnnpn_bn_train_forward_f32(P, 0, 4, P, P, 1e-5, 0.1, 0, P, P, P, None, None, None) == E_ARG
    assert lib.gnnpn_bn_train_forward_f32(P, 2, 4, P, P, 1e-5, 0.1, 0, P, P, P, P, None, None) == E_ARG   # one running buffer
    assert lib.gnnpn_bn_train_backward_f32(P, None, P, P, P, 4, 4, 1, P, P, P, None) == E_ARG            # ReLU mask without y
    assert lib.gnnpn_bce_sigmoid_f32(P, P, 0, P, P, None) == E_ARG
    assert lib.gnnpn_embed_grad_f32(P, 3, P, 1, 5, 4, 7, P, None) == E_ARG                                # ldh < c
    assert lib.gnnpn_embed_grad_f32(P, 4, P, 0, 5, 4, 7, P, None) == E_ARG                                # ldx < 1
    assert lib.gnnpn_scatter_dx_f32(P, P, P, 2, 5, 4, 8, None) == E_ARG                                   # L < T
    assert lib.gnnpn_scatter_dx_f32(P, P, P, 2, 1, 4, 8, None) == 0                                       # T = 1: nothing to add
    assert lib.gnnpn_sumsq_f32(P, -1, P, None) == E_ARG
    assert lib.gnnpn_sumsq_f32(P, 0, P, None) == 0
    assert lib.gnnpn_adam_step_f32(P, P, P, P, 4, P, 2.0, 1e-3, 0.9, 0.999, 1e-8, 0, None) == E_ARG       # step < 1
    # hidden sizes other than 256 / 32 are not built; B = 0 enqueues nothing (empty operands have no pointers)
    assert lib.gnnpn_lstm_train_forward_f32(P, P, P, P, P, P, 2, 3, 64, None) == E_UNSUP
    assert lib.gnnpn_lstm_train_backward_f32(P, P, P, P, P, P, P, 2, 3, 64, None) == E_UNSUP
    assert lib.gnnpn_lstm_train_forward_f32(None, P, P, None, None, None, 0, 3, 32, None) == 0
    assert lib.gnnpn_lstm_train_backward_f32(P, None, None, None, None, None, None, 0, 3, 256, None) == 0
    assert lib.gnnpn_lstm_train_forward_f32(P, P, P, P, P, P, 1, 0, 32, None) == E_ARG                     # L = 0

    def dec(**over):
        t = lib_mod.DecodeTrain()
        for name, _ in lib_mod.DecodeTrain._fields_:
            setattr(t, name, 64)
        t.latent_win = None
        for k, v in over.items():
            setattr(t, k, v)
        return t

    for n_per, H, rc in ((65, 32, E_ARG), (0, 32, E_ARG), (64, 64, E_UNSUP)):
        assert lib.gnnpn_decode_train_forward_f32(ctypes.byref(dec()), 2, 3, n_per, H, 10.0, 1, None) == rc
        assert lib.gnnpn_decode_train_backward_f32(ctypes.byref(dec()), P, P, P, P, P, P, 2, 3, n_per, H, 10.0, 1, None) == rc
    assert lib.gnnpn_decode_train_forward_f32(ctypes.byref(dec(x_all=None)), 2, 3, 4, 32, 10.0, 1, None) == E_ARG
    empty = {k: None for k in ("embedded", "enc_out", "h0", "c0", "idx", "x_all", "gates_pre", "c_all", "h_all", "z0", "probs", "logp")}
    assert lib.gnnpn_decode_train_forward_f32(ctypes.byref(dec(**empty)), 0, 3, 4, 32, 10.0, 1, None) == 0

    def attn(G=1, bah=0, **over):
        t = lib_mod.DecodeAttnTrain()
        t.base = dec(**over)
        t.bahdanau, t.n_glimpses = bah, G
        for name, _ in lib_mod.DecodeAttnTrain._fields_[3:]:
            setattr(t, name, 64)
        return t

    fwd = lambda t, T, n_per, H=32: lib.gnnpn_decode_attn_train_forward_f32(ctypes.byref(t), 1, T, n_per, H, 10.0, 1, None)  # noqa: E731
    bwd = lambda t, T, n_per, H=32: lib.gnnpn_decode_attn_train_backward_f32(ctypes.byref(t), P, P, P, P, P, P, 1, T, n_per, H,  # noqa: E731
                                                                              10.0, 1, None)
    for T, n_per in ((251, 51), (12801, 1), (201, 64)):    # 12801 and 12864 positions: past the LDS the kernels are sized for
        assert fwd(attn(), T, n_per) == E_UNSUP and bwd(attn(), T, n_per) == E_UNSUP
    assert fwd(attn(G=9), 4, 4) == E_ARG and fwd(attn(G=-1), 4, 4) == E_ARG
    assert fwd(attn(), 4, 65) == E_ARG and fwd(attn(), 4, 4, H=64) == E_UNSUP
    t = attn(G=1)
    t.a_all = None
    assert fwd(t, 4, 4) == E_ARG                                                     # glimpse rounds need a_all
    t = attn(G=0, bah=1)
    t.p_ref = None
    assert fwd(t, 4, 4) == E_ARG
