"""-m gpu: the kernels of the two training steps (csrc/train.hip, train_attn.hip, train_ml.hip, gnnpn_gemm_f32 of dense.hip and
the evaluation helpers precision_at_k / attention_logits) one by one against float64 references on the CPU, at the shapes and
edges where tiled and strided kernels go wrong.  Reductions are checked twice: on small-integer inputs, where every fp32 product
and partial sum is exact and the kernel must equal the fp64 result bit for bit, and on random floats, bounded by the size of the
terms or by a yardstick (the same computation in torch fp32 on the CPU).  Every kernel is run twice on the same inputs and
must give the same bits (sumsq excepted, see there).  The worst ratios go to the agreement records train_kernels_*."""
import math

import pytest
import torch
import torch.nn.functional as F

from kernel_checks import D, F32, I32, TINY, U, Recorder, exact as _exact, same_bits as _same_bits

pytestmark = pytest.mark.gpu
_REC = Recorder("train_kernels")     # the helpers live in tests/kernel_checks.py (shared with test_gpu_kernel_builds.py)
WORST = _REC.worst                   # kernel -> {measure: worst value}
_note, _bounded, _yardstick = _REC.note, _REC.bounded, _REC.yardstick


def _ops():
    from gnnpn_sc_amd import ops
    return ops


def _twice(fn):
    """fn() run twice on the same inputs: every tensor it returns must repeat bit for bit."""
    r1, r2 = fn(), fn()
    t1 = r1 if isinstance(r1, (tuple, list)) else (r1,)
    t2 = r2 if isinstance(r2, (tuple, list)) else (r2,)
    for x, y in zip(t1, t2):
        if isinstance(x, torch.Tensor):
            assert _same_bits(x, y), "two runs on the same inputs differ"
    return r1


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F32)


# ---- gemm ---------------------------------------------------------------------------------------------------------------------
def _gemm_case(dev, M, N, K, a_km, b_km, exact, g):
    ops = _ops()
    Aop = _ints((M, K), -4, 4, g) if exact else torch.randn(M, K, generator=g)
    Bop = _ints((N, K), -4, 4, g) if exact else torch.randn(N, K, generator=g)
    a = (Aop.t() if a_km else Aop).contiguous().to(dev)
    b = (Bop.t() if b_km else Bop).contiguous().to(dev)
    c = _twice(lambda: ops.gemm(a, b, a_km, b_km))
    assert c.shape == (M, N)
    ref = Aop.double() @ Bop.double().t()
    if exact:         # |products| <= 16, |sums| <= 16 K < 2^24: every partial sum exact in any order
        assert _exact(c, ref.float()), f"gemm {M}x{N}x{K} ({a_km},{b_km}) not exact"
        _note("gemm", exact_cases=1)
    else:
        absprod = Aop.double().abs() @ Bop.double().abs().t()
        _bounded("gemm", "random", c, ref, 8 * math.sqrt(K) * U * absprod + 1e-35)


GEMM_MN = [(1, 1), (31, 65), (64, 64), (65, 31), (200, 1), (1, 200), (65, 200)]


@pytest.mark.parametrize("a_km,b_km", [(False, False), (False, True), (True, False), (True, True)])
def test_gemm_tiles_and_layouts(dev, a_km, b_km):
    g = torch.Generator().manual_seed(11 + 2 * a_km + b_km)
    for M, N in GEMM_MN:
        for K in (1, 31, 32, 33, 2047, 2048):
            for exact in (True, False):
                _gemm_case(dev, M, N, K, a_km, b_km, exact, g)


@pytest.mark.parametrize("a_km,b_km", [(False, False), (False, True), (True, False), (True, True)])
def test_gemm_split_k(dev, a_km, b_km):
    ops = _ops()
    g = torch.Generator().manual_seed(21 + 2 * a_km + b_km)
    cases = [(200, 65, 60160), (1, 1, 60160), (31, 65, 5000), (64, 64, 2048), (65, 200, 4100)]
    assert ops.gemm_split(200, 65, 60160) == 64 and ops.gemm_split(1, 1, 60160) == 64     # k_chunk 960: slice 63 starts past K
    assert ops.gemm_split(31, 65, 5000) == 9 and 5000 % (9 * 32)                          # K not a multiple of split * 32
    assert ops.gemm_split(64, 64, 2048) == 4 and ops.gemm_split(65, 200, 4100) == 8
    for M, N, K in cases:
        for exact in (True, False):
            _gemm_case(dev, M, N, K, a_km, b_km, exact, g)


def test_gemm_direct_split_and_padding(dev):
    """gnnpn_gemm_f32 itself: explicit split_k up to 1024 (empty slices write zeros), leading dimensions past the minimum with
    the padding poisoned with NaN (never read; C's padding never written)."""
    from gnnpn_sc_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    for (M, N, K, a_km, b_km, split) in ((65, 65, 2048, True, True, 1024), (200, 31, 999, False, True, 7),
                                         (33, 64, 4096, True, False, 64), (1, 200, 60160, False, False, 3)):
        Aop, Bop = _ints((M, K), -4, 4, g), _ints((N, K), -4, 4, g)
        pa, pb, pc = 5, 3, 7
        A = torch.full((K, M + pa) if a_km else (M, K + pa), float("nan"))
        B = torch.full((K, N + pb) if b_km else (N, K + pb), float("nan"))
        if a_km:
            A[:, :M] = Aop.t()
        else:
            A[:, :K] = Aop
        if b_km:
            B[:, :N] = Bop.t()
        else:
            B[:, :K] = Bop
        A, B = A.to(dev), B.to(dev)
        ldc = N + pc

        def run():
            C = torch.full((split, M, ldc), float("nan"), device=dev)
            _lib.check(lib.gnnpn_gemm_f32(_lib.dev_ptr(A, F32, "A"), A.shape[1], int(a_km), _lib.dev_ptr(B, F32, "B"), B.shape[1],
                                          int(b_km), _lib.dev_ptr(C, F32, "C"), ldc, M, N, K, split, _lib.stream_ptr()), "gemm")
            return C
        C = _twice(run).cpu()
        assert torch.isnan(C[:, :, N:]).all(), "padding columns of C written"
        k_chunk = -(-(-(-K // split)) // 32) * 32
        for z in range(split):
            k0, k1 = min(K, z * k_chunk), min(K, (z + 1) * k_chunk)
            want = Aop[:, k0:k1].double() @ Bop[:, k0:k1].double().t()
            assert _exact(C[z, :, :N], want.float()), f"slice {z} of {split} (k {k0}..{k1})"
        assert _exact(C[:, :, :N].double().sum(0).float(), (Aop.double() @ Bop.double().t()).float())


def test_gemm_empty(dev):
    ops = _ops()
    for M, N, K in ((0, 5, 4096), (5, 0, 4096), (0, 5, 100), (5, 0, 100), (4, 6, 0)):
        c = ops.gemm(torch.empty(M, K, device=dev), torch.empty(N, K, device=dev))
        assert c.shape == (M, N) and c.is_cuda and torch.equal(c.cpu(), torch.zeros(M, N))
    from gnnpn_sc_amd import _lib
    x = torch.ones(64, device=dev)
    p = _lib.dev_ptr(x, F32, "x")
    assert _lib.load().gnnpn_gemm_f32(p, 4, 0, p, 4, 0, p, 5, 0, 5, 4, 1, None) == 0        # M = 0: nothing enqueued
    assert _lib.load().gnnpn_gemm_f32(p, 4, 0, p, 4, 0, p, 5, 4, 0, 4, 1, None) == -1       # N = 0: the C contract wants N > 0


# ---- colsum -------------------------------------------------------------------------------------------------------------------
def _colsum_case(dev, rows, cols, ld, exact, g):
    ops = _ops()
    X = _ints((rows, cols), -8, 8, g) if exact else torch.randn(rows, cols, generator=g)
    buf = torch.full((rows, ld), float("nan"))
    buf[:, :cols] = X
    flat = buf.reshape(-1)[: max((rows - 1) * ld + cols, 0)].contiguous() if rows else torch.empty(0)
    xd = flat.to(dev)
    out = _twice(lambda: ops.colsum(xd, rows, cols, ld))
    ref = X.double().sum(0)
    if exact:         # |sums| <= 8 * 70000 < 2^24
        assert _exact(out, ref.float()), f"colsum rows={rows} cols={cols} ld={ld}"
    else:
        _bounded("colsum", "random", out, ref, 8 * math.sqrt(max(rows, 1)) * U * X.double().abs().sum(0) + 1e-35)


@pytest.mark.parametrize("rows", [0, 1, 3, 4, 5, 4095, 4096, 4097, 70000])
def test_colsum(dev, rows):
    ops = _ops()
    g = torch.Generator().manual_seed(rows)
    plan = ops.colsum_chunking(rows)
    assert (plan is None) == (rows < 4096)                # one pass below 4096 rows, two from there on
    for cols in ((1, 63, 64, 65, 1024) if rows <= 4097 else (1, 65)):
        for exact in (True, False):
            _colsum_case(dev, rows, cols, cols, exact, g)
            if rows:
                _colsum_case(dev, rows, cols, cols + 3, exact, g)        # strided: the gap poisoned with NaN


def test_colsum_strided_like_the_start_input(dev):
    """trainPNHigh.py: colsum(dx, rows=B, cols=H, ld=T*H) — step 0 of every problem's decoder inputs."""
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    for B, T, H in ((3, 47, 256), (5000, 2, 32)):
        dx = torch.randn(B, T, H, generator=g)
        out = _twice(lambda: ops.colsum(dx.to(dev), rows=B, cols=H, ld=T * H))
        ref = dx[:, 0].double().sum(0)
        _bounded("colsum", "strided", out, ref, 8 * math.sqrt(B) * U * dx[:, 0].double().abs().sum(0) + 1e-35)


def test_colsum_chunks_partials(dev):
    from gnnpn_sc_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(9)
    for rows, cols, ld, per in ((4097, 65, 70, 33), (10, 1, 1, 3), (300, 64, 64, 300), (1000, 130, 131, 7)):
        buf = torch.full((rows, ld), float("nan"))
        X = _ints((rows, cols), -8, 8, g)
        buf[:, :cols] = X
        xd = buf.to(dev)
        chunks = -(-rows // per)

        def run():
            part = torch.full((chunks, cols), float("nan"), device=dev)
            _lib.check(lib.gnnpn_colsum_chunks_f32(_lib.dev_ptr(xd, F32, "x"), ld, rows, cols, per, _lib.dev_ptr(part, F32, "p"),
                                                   _lib.stream_ptr()), "colsum_chunks")
            return part
        part = _twice(run).cpu()
        for c in range(chunks):
            assert _exact(part[c], X[c * per:(c + 1) * per].double().sum(0).float()), f"chunk {c}"


# ---- sumsq / adam ------------------------------------------------------------------------------------------------------------
def test_grad_sumsq(dev):
    """The device double is accumulated by one atomicAdd per workgroup, in whatever order they finish: two runs may differ in
    the last bits (1.5e-15 relative has been seen over six calls of 1024 workgroups), so repeatability is asserted within the
    rounding that order can move, 2 * depth * 2^-53 relative (the kernel is not changed for it)."""
    ops = _ops()
    g = torch.Generator().manual_seed(1)
    sizes = [1, 255, 256, 257, 300_001, 1024 * 256 * 3 + 5]
    for exact in (True, False):
        gs = [(_ints((n,), -8, 8, g) if exact else torch.randn(n, generator=g)) for n in sizes]
        ref = sum(float(x.double().pow(2).sum()) for x in gs)
        outs = [float(ops.grad_sumsq([x.to(dev) for x in gs]).item()) for _ in range(2)]
        depth = 4 + 8 + 1024 + len(sizes)     # per thread <= 4 terms, 8 tree levels, <= 1024 atomics per call, 6 calls
        _note("sumsq", rel_run_to_run=abs(outs[0] - outs[1]) / ref)
        assert abs(outs[0] - outs[1]) <= 2 * depth * 2.0 ** -53 * ref
        if exact:
            assert outs[0] == ref                      # squares of small integers: every double sum exact
        else:
            # squares exact in double: the error of a depth-deep sum of positive terms
            rel = abs(outs[0] - ref) / ref
            _note("sumsq", rel_err_vs_fp64=rel, rel_err_over_bound=rel / (depth * 2.0 ** -53))
            assert rel <= depth * 2.0 ** -53
    z = ops.grad_sumsq([torch.zeros(0, device=dev), torch.ones(3, device=dev)])     # an empty gradient adds nothing
    assert float(z.item()) == 3.0


@pytest.mark.parametrize("n", [1, 256, 2048 * 256 + 77])
def test_adam_step_with_clipping(dev, n):
    """clip_grad_norm_ + torch.optim.Adam on fp64 copies, 6 steps: clipped (the global norm beyond max_grad_norm, part of it
    from other parameters), not clipped, a zero gradient (norm 0, clip factor 1).  Step 1 is unclipped: there Adam is nearly
    blind to the gradient's scale.  On every clipped step the unclipped fp64 update must lie outside the tolerance."""
    ops = _ops()
    g = torch.Generator().manual_seed(n)
    lr, max_norm = 1e-2, 2.0
    tol = 1e-3 * lr
    p0 = torch.rand(n, generator=g) * 2 - 1
    p64 = p0.double().clone().requires_grad_(True)
    other = torch.zeros(1, dtype=D, requires_grad=True)          # stands for the other parameters' share of the norm
    opt = torch.optim.Adam([p64, other], lr=lr)
    p, m, v = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    # (norm of this gradient, norm of the rest): total 0.5 (no clip), 5 (clip), 0, 50 (clip), 1.9 (no clip), 3 (clip)
    plan = [(0.5, 0.0), (3.0, 4.0), (0.0, 0.0), (30.0, 40.0), (1.9, 0.0), (1.0, math.sqrt(8.0))]
    for step, (gn, rest) in enumerate(plan, 1):
        gr = torch.randn(n, generator=g)
        gr = (gr * (gn / float(gr.double().norm()))).float() if gn else torch.zeros(n)
        sumsq = torch.tensor([float(gr.double().pow(2).sum()) + rest * rest], dtype=D, device=dev)
        gd = gr.to(dev)
        before = (p64.detach().clone(), {k: t.clone() for k, t in opt.state[p64].items()} if step > 1 else None)
        p64.grad, other.grad = gr.double().clone(), torch.tensor([rest], dtype=D)
        total = float(torch.nn.utils.clip_grad_norm_([p64, other], max_norm))
        opt.step()
        ops.adam_step(p, gd, m, v, sumsq, max_norm, lr, step)
        err = float((p.cpu().double() - p64.detach()).abs().max())
        _note("adam_step", err_over_tol=err / tol)
        assert err <= tol, f"step {step}: |p - p64| = {err:.3e} > {tol:.3e}"
        if total > max_norm:                                     # what the update would have been without the clip
            q = before[0].clone().requires_grad_(True)
            o2 = torch.optim.Adam([q], lr=lr)
            if before[1] is not None:
                o2.state[q] = {k: t.clone() for k, t in before[1].items()}
            q.grad = gr.double().clone()
            o2.step()
            assert float((q.detach() - p64.detach()).abs().max()) > 2 * tol, f"step {step}: the clip is not visible"
    # repeatability: the same step from the same state gives the same bits
    gd, sumsq = torch.randn(n, generator=g).to(dev), torch.tensor([9.0], dtype=D, device=dev)
    outs = []
    for _ in range(2):
        pp, mm, vv = p.clone(), m.clone(), v.clone()
        ops.adam_step(pp, gd, mm, vv, sumsq, max_norm, lr, 7)
        outs.append((pp, mm, vv))
    assert all(_same_bits(a, b) for a, b in zip(*outs))


# ---- BatchNorm / BCE / dot / embed_grad / scatter_dx -------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [2, 3, 5, 1001, 5014])
def test_bn_train_forward_backward(dev, rows):
    ops = _ops()
    g = torch.Generator().manual_seed(rows)
    for cols in (1, 63, 64, 65, 256):
        for relu in (False, True):
            x = torch.randn(rows, cols, generator=g) * 3 + 0.5
            gamma, beta = torch.rand(cols, generator=g) + 0.5, torch.randn(cols, generator=g)
            rm, rv = torch.randn(cols, generator=g), torch.rand(cols, generator=g) + 0.5
            dy = torch.randn(rows, cols, generator=g)
            xd, gd, bd, dyd = x.to(dev), gamma.to(dev), beta.to(dev), dy.to(dev)

            def fwd():
                rmd, rvd = rm.to(dev), rv.to(dev)
                y, xhat, invstd = ops.bn_train_forward(xd, gd, bd, relu, rmd, rvd)
                return y, xhat, invstd, rmd, rvd
            y, xhat, invstd, rmd, rvd = _twice(fwd)
            dx, dgam, dbet = _twice(lambda: ops.bn_train_backward(dyd, y, xhat, gd, invstd, relu))
            x64 = x.double().requires_grad_(True)
            g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
            rm64, rv64 = rm.double(), rv.double()
            ylin = F.batch_norm(x64, rm64, rv64, g64, b64, training=True, momentum=0.1, eps=1e-5)
            y64 = F.relu(ylin) if relu else ylin
            # the ReLU gate as the kernel's y set it: a y within rounding of 0 may fall on either side of it
            mask = (y.cpu() > 0) if relu else torch.ones_like(dy, dtype=torch.bool)
            ylin.backward(dy.double() * mask)
            mean, var = x.double().mean(0), x.double().var(0, unbiased=False)
            inv64 = 1.0 / torch.sqrt(var + 1e-5)
            xh64 = (x.double() - mean) * inv64
            # fp32 sums of `rows` terms in 4 sequential partials: a statistical bound, relative to the size of the terms
            t = 8 * math.sqrt(rows) * U
            # x - mean cancels where a column's spread is small against its values: errors of |x| u grow by invstd
            amp = 1 + ((x.double().abs() + x.double().abs().mean(0)) * inv64).max(0).values
            _bounded("bn_train_forward", "xhat", xhat, xh64, t * 4 * (xh64.abs() + 1) * amp + 1e-30)
            _bounded("bn_train_forward", "y", y, y64.detach(),
                     t * 4 * (gamma.double().abs() * (xh64.abs() + 1) * amp + beta.double().abs()))
            _bounded("bn_train_forward", "invstd", invstd, inv64, t * 4 * inv64 * amp)
            _bounded("bn_train_forward", "running_mean", rmd, rm64, t * (rm.double().abs() + 0.1 * x.double().abs().max(0).values))
            _bounded("bn_train_forward", "running_var", rvd, rv64, t * 4 * (rv.double().abs() + 0.1 * x.double().var(0)))
            d = dy.double() * mask
            sc = gamma.double().abs() * inv64 * (d.abs().max(0).values + d.abs().mean(0) * (1 + xh64.abs().max(0).values))
            _bounded("bn_train_backward", "dx", dx, x64.grad, t * 8 * sc * amp + 1e-30)
            _bounded("bn_train_backward", "dgamma", dgam, g64.grad, t * 4 * (d.abs() * (xh64.abs() + 1)).sum(0) * amp + 1e-30)
            _bounded("bn_train_backward", "dbeta", dbet, b64.grad, t * (d.abs()).sum(0) + 1e-30)


def test_bn_train_forward_rejects_one_row(dev):
    ops = _ops()
    x = torch.randn(1, 8, device=dev)
    with pytest.raises(ops.GnnpnError, match="rows >= 2"):
        ops.bn_train_forward(x, torch.ones(8, device=dev), torch.zeros(8, device=dev), False, torch.zeros(8, device=dev),
                             torch.ones(8, device=dev))


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 12535])
def test_bce_sigmoid(dev, n):
    ops = _ops()
    g = torch.Generator().manual_seed(n)
    p = torch.rand(n, generator=g)
    y = torch.rand(n, generator=g)
    y[torch.rand(n, generator=g) < 0.4] = 0.0
    y[torch.rand(n, generator=g) < 0.4] = 1.0
    specials = torch.tensor([0.0, 1.0, 1e-44, 3e-44, 1 - 2 ** -24, 2 ** -30, 0.5])     # exact 0 / 1, below e^-100, near 1
    k = min(n, specials.numel())
    p[:k] = specials[:k]
    loss, dz = _twice(lambda: ops.bce_sigmoid(p.to(dev), y.to(dev)))
    p64, y64 = p.double(), y.double()
    loss64 = F.binary_cross_entropy(p64, y64)
    go = torch.ones((), dtype=D)
    gp = torch.ops.aten.binary_cross_entropy_backward(go, p64, y64, None, 1)            # reduction = mean, as autograd forms it
    dz64 = torch.ops.aten.sigmoid_backward(gp, p64)
    terms = -(y64 * torch.clamp(torch.log(p64), min=-100) + (1 - y64) * torch.clamp(torch.log1p(-p64), min=-100))
    assert torch.allclose(terms.mean(), loss64, rtol=1e-12)
    _bounded("bce_sigmoid", "loss", loss, loss64.reshape(1), 8 * U * terms.abs().mean() + U * loss64.abs() + 1e-30)
    _bounded("bce_sigmoid", "dz", dz, dz64, 8 * U * dz64.abs() + 2.0 ** -126)


def test_dot(dev):
    ops = _ops()
    g = torch.Generator().manual_seed(2)
    for n in (0, 1, 1025, 10 ** 6):
        for exact in (True, False):
            a = _ints((n,), -8, 8, g) if exact else torch.randn(n, generator=g)
            b = _ints((n,), -8, 8, g) if exact else torch.randn(n, generator=g)
            out = _twice(lambda: ops.dot(a.to(dev), b.to(dev)))
            ref = (a.double() * b.double()).sum()
            if exact:
                assert _exact(out, ref.float().reshape(1))
            else:       # products exact in double, the double sum then one rounding to fp32
                _bounded("dot", "random", out, ref.reshape(1), U * ref.abs() + n * 2.0 ** -53 * (a.double() * b.double()).abs().sum() + 1e-40)


def test_embed_grad(dev):
    ops = _ops()
    g = torch.Generator().manual_seed(4)
    for vocab, rows, c, ldh, ldx in ((1, 5, 3, 4, 2), (7, 300, 16, 20, 9), (200, 1000, 8, 8, 3), (7, 0, 4, 6, 2), (200, 50, 65, 65, 1)):
        for exact in (True, False):
            ids = torch.randint(0, vocab, (rows,), generator=g)
            if rows >= 2:
                ids[0], ids[-1] = 0, vocab - 1                  # both ends of the table; most of 200 ids never occur
            x = torch.randn(rows, ldx, generator=g)
            x[:, 0] = ids.float()
            dh = _ints((rows, ldh), -8, 8, g) if exact else torch.randn(rows, ldh, generator=g)
            if ldh > c:
                dh[:, c:] = float("nan")                        # columns past c are never read
            out = _twice(lambda: ops.embed_grad(dh.to(dev), x.to(dev), c, vocab))
            ref = torch.zeros(vocab, c, dtype=D).index_add_(0, ids, dh[:, :c].double())
            if exact:
                assert _exact(out, ref.float())
            else:
                cnt = torch.bincount(ids, minlength=vocab).double().clamp(min=1).unsqueeze(1)
                mag = torch.zeros(vocab, c, dtype=D).index_add_(0, ids, dh[:, :c].double().abs())
                _bounded("embed_grad", "random", out, ref, 8 * cnt.sqrt() * U * mag + 1e-35)
            unused = torch.bincount(ids, minlength=vocab) == 0
            assert torch.equal(out.cpu()[unused], torch.zeros(int(unused.sum()), c))


def test_scatter_dx(dev):
    ops = _ops()
    g = torch.Generator().manual_seed(6)
    for B, T, K, H in ((3, 1, 4, 32), (3, 2, 5, 256), (4, 47, 3, 32), (100, 47, 2, 256)):
        L = T * K
        idx = (torch.arange(T) * K).unsqueeze(0) + torch.randint(0, K, (B, T), generator=g)   # one pick per window
        dx, pre = torch.randn(B, T, H, generator=g), torch.randn(B, L, H, generator=g)
        idxd, dxd = idx.int().to(dev), dx.to(dev)

        def run():
            d = pre.to(dev)
            ops.scatter_dx(dxd, idxd, d)
            return d
        out = _twice(run).cpu()
        ref = pre.clone()                                   # x_k = embedded[b, idx[b, k-1]]: one fp32 addition per element
        for k in range(1, T):
            ref[torch.arange(B), idx[:, k - 1]] += dx[:, k]
        assert _exact(out, ref), f"scatter_dx B={B} T={T} H={H}"
    assert 100 * 46 * 256 > 4096 * 256                       # the last shape runs the grid-stride loop


# ---- the recurrences ---------------------------------------------------------------------------------------------------------
def _cell(x_gates, h, c, whh, bhh):
    gates = x_gates + F.linear(h, whh, bhh)
    i, f, gg, o = gates.chunk(4, 1)
    c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    return gates, torch.sigmoid(o) * torch.tanh(c2), c2


def _lstm_ref(pre, whh, bhh, d_enc, dh0, dc0, dtype):
    pre = pre.detach().to(dtype).clone().requires_grad_(True)
    whh, bhh = whh.to(dtype), bhh.to(dtype)
    B, L, H4 = pre.shape
    h = torch.zeros(B, H4 // 4, dtype=dtype)
    c = torch.zeros_like(h)
    hs, cs, gs = [], [], []
    for t in range(L):
        gates, h, c = _cell(pre[:, t], h, c, whh, bhh)
        hs.append(h), cs.append(c), gs.append(gates)
    enc, call, gp = torch.stack(hs, 1), torch.stack(cs, 1), torch.stack(gs, 1)
    loss = (enc * d_enc.to(dtype)).sum() + (h * dh0.to(dtype)).sum() + (c * dc0.to(dtype)).sum()
    loss.backward()
    return enc.detach(), gp.detach(), call.detach(), pre.grad


@pytest.mark.parametrize("H", [32, 256])
def test_lstm_train_forward_backward(dev, H):
    ops = _ops()
    g = torch.Generator().manual_seed(H)
    s = 1 / math.sqrt(H)
    for B, L in ((1, 1), (3, 2), (3, 235), (1, 235)):
        whh = (torch.rand(4 * H, H, generator=g) * 2 - 1) * s
        bhh = (torch.rand(4 * H, generator=g) * 2 - 1) * s
        pre = torch.randn(B, L, 4 * H, generator=g) * 0.5
        d_enc = torch.randn(B, L, H, generator=g)
        for nonzero in (False, True):
            dh0 = torch.randn(B, H, generator=g) if nonzero else torch.zeros(B, H)
            dc0 = torch.randn(B, H, generator=g) if nonzero else torch.zeros(B, H)
            pd, wt, bd, whd = pre.to(dev), whh.t().contiguous().to(dev), bhh.to(dev), whh.to(dev)
            enc, gp, ca = _twice(lambda: ops.lstm_train_forward(pd, wt, bd))
            dg = _twice(lambda: ops.lstm_train_backward(whd, gp, ca, d_enc.to(dev), dh0.to(dev), dc0.to(dev)))
            r64 = _lstm_ref(pre, whh, bhh, d_enc, dh0, dc0, D)
            r32 = _lstm_ref(pre, whh, bhh, d_enc, dh0, dc0, F32)
            for what, got, a, b in zip(("enc_out", "gates_pre", "c_all", "dgates"), (enc, gp, ca, dg), r64, r32):
                _yardstick("lstm_train", what, got, a, b)


def test_lstm_train_edges(dev):
    ops = _ops()
    with pytest.raises(ops.GnnpnError, match=r"\(-2\)"):
        ops.lstm_train_forward(torch.zeros(1, 2, 256, device=dev), torch.zeros(64, 256, device=dev), torch.zeros(256, device=dev))
    enc, gp, ca = ops.lstm_train_forward(torch.zeros(0, 3, 128, device=dev), torch.zeros(32, 128, device=dev),
                                         torch.zeros(128, device=dev))
    assert enc.shape == (0, 3, 32) and gp.shape == (0, 3, 128)
    dg = ops.lstm_train_backward(torch.zeros(128, 32, device=dev), gp, ca, enc, torch.zeros(0, 32, device=dev),
                                 torch.zeros(0, 32, device=dev))
    assert dg.shape == (0, 3, 128)


def _att(bah, q, ref, wq, bq, v, qps):
    """oracle/pn_train.py::_attention's logits with ref = W_ref(enc_out) + b_ref GIVEN ([B,L,H]; enc_out itself for 'Dot') and
    per-problem V ([B,H]), so that autograd reaches d ref, d V per problem and (through qps) the projected queries."""
    if bah:
        qp = F.linear(q, wq, bq)
        qp.retain_grad()
        qps.append(qp)
        return (v.unsqueeze(1) * torch.tanh(qp.unsqueeze(1) + ref)).sum(2)
    return torch.bmm(ref, q.unsqueeze(2)).squeeze(2)


def _decode_ref(w, idx, T, K, C, use_tanh, gscale, dtype, bah=False, G=0):
    """Teacher-forced decode from the given enc_out / h0 / c0, as oracle/pn_train.py::pick_log_probs from its :82 on, in `dtype`
    with autograd: forward saves and every gradient the kernels leave."""
    leaf = lambda v: v.detach().to(dtype).clone().requires_grad_(True)   # noqa: E731  (never the caller's tensor itself)
    lv = {k: (leaf(v) if v is not None and v.is_floating_point() else v) for k, v in w.items()}
    B, L, H = lv["enc_out"].shape
    for k in ("p_v", "g_v"):                             # V per problem: the kernels leave its gradient per problem
        if k in w:
            lv[k] = leaf(w[k].unsqueeze(0).repeat(B, 1))
    rows = torch.arange(B)
    h, c = lv["h0"], lv["c0"]
    xs, gates_l, hs, cs, z0s, probs, logps, qp_p, qp_g = [], [], [], [], [], [], [], [], []
    x = lv["start"].detach().unsqueeze(0).repeat(B, 1).requires_grad_(True)
    pref = lv["p_ref"] if bah else lv["enc_out"]
    gref = lv["g_ref"] if (bah and G) else lv["enc_out"]
    for k in range(T):
        xs.append(x)
        gates = F.linear(x, lv["wih"], lv["bih"]) + F.linear(h, lv["whh"], lv["bhh"])
        gates.retain_grad()
        gates_l.append(gates)
        i, f, gg, o = gates.chunk(4, 1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        hs.append(h), cs.append(c)
        q = h
        if G:
            chosen = torch.zeros(B, L, dtype=torch.bool)
            if k:
                chosen[rows.unsqueeze(1), idx[:, :k]] = True
            for _ in range(G):
                u = _att(bah, q, gref, lv.get("g_wq"), lv.get("g_bq"), lv.get("g_v"), qp_g).masked_fill(chosen, float("-inf"))
                q = torch.bmm(F.softmax(u, 1).unsqueeze(1), gref).squeeze(1)
        z = _att(bah, q, pref[:, k * K:(k + 1) * K], lv.get("p_wq"), lv.get("p_bq"), lv.get("p_v"), qp_p)
        if use_tanh:
            z = C * torch.tanh(z)
        z0s.append(z)
        if lv.get("latent") is not None:
            z = z + lv["latent"][:, k]
        lp = F.log_softmax(z, 1)
        probs.append(lp.exp())
        logps.append(lp[rows, idx[:, k] - k * K])
        x = lv["embedded"][rows, idx[:, k]].detach().requires_grad_(True)
    logp = torch.stack(logps, 1)
    (logp.sum(1) * gscale.to(dtype)).sum().backward()
    out = {"logp": logp, "probs": torch.stack(probs, 1), "z0": torch.stack(z0s, 1), "gates_pre": torch.stack(gates_l, 1),
           "c_all": torch.stack(cs, 1), "h_all": torch.stack(hs, 1), "x_all": torch.stack(xs, 1),
           "dgates": torch.stack([t.grad for t in gates_l], 1), "dx": torch.stack([t.grad for t in xs], 1),
           "dh0": lv["h0"].grad, "dc0": lv["c0"].grad}
    out["d_enc_out"] = lv["enc_out"].grad if lv["enc_out"].grad is not None else torch.zeros(B, L, H, dtype=dtype)
    if bah:
        out["d_p_ref"], out["d_p_v"] = lv["p_ref"].grad, lv["p_v"].grad
        out["d_p_qp"] = torch.stack([t.grad for t in qp_p], 1)
        if G:
            out["d_g_ref"], out["d_g_v"] = lv["g_ref"].grad, lv["g_v"].grad
            out["d_g_qp"] = torch.stack([t.grad for t in qp_g], 1).view(B, T, G, H)
    return {k: v.detach() for k, v in out.items()}


def _decode_inputs(B, T, K, H, latent, g, bah=False, G=0):
    L, s = T * K, 1 / math.sqrt(H)
    u = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1)        # noqa: E731
    w = {"enc_out": u(B, L, H) * 0.6, "embedded": u(B, L, H), "h0": u(B, H) * 0.5, "c0": u(B, H), "start": u(H),
         "wih": u(4 * H, H) * s, "whh": u(4 * H, H) * s, "bih": u(4 * H) * s, "bhh": u(4 * H) * s,
         "latent": u(B, T, K) * 3 if latent else None}
    if bah:
        for tag in ("p",) + (("g",) if G else ()):
            w[f"{tag}_wq"], w[f"{tag}_bq"], w[f"{tag}_v"] = u(H, H) * s, u(H) * s, u(H)
            w[f"{tag}_ref"] = w["enc_out"] * (2.0 if tag == "p" else 0.5)      # W_ref = 2 I / 0.5 I, b_ref = 0: exact in fp32
    idx = (torch.arange(T) * K).unsqueeze(0) + torch.randint(0, K, (B, T), generator=g)
    gscale = torch.tensor([0.0, -0.7, 1.3, -2.0][:B]) if B > 1 else torch.tensor([0.9])
    return w, idx, gscale


DECODE_CASES = [  # H, B, T, n_per, use_tanh, tanh_c, latent
    (32, 3, 1, 1, 1, 10.0, False), (32, 3, 2, 2, 0, 1.0, True), (32, 3, 47, 17, 1, 7.5, True), (32, 2, 47, 64, 1, 10.0, False),
    (256, 3, 47, 16, 1, 10.0, True), (256, 3, 2, 63, 0, 1.0, False), (256, 3, 1, 64, 1, 2.5, True), (256, 2, 47, 1, 1, 10.0, True)]


@pytest.mark.parametrize("H,B,T,K,use_tanh,C,latent", DECODE_CASES)
def test_decode_train_forward_backward(dev, H, B, T, K, use_tanh, C, latent):
    ops = _ops()
    g = torch.Generator().manual_seed(H * 1000 + T * 70 + K)
    w, idx, gscale = _decode_inputs(B, T, K, H, latent, g)
    dv = {k: (v.to(dev) if v is not None else None) for k, v in w.items()}
    idxd = idx.int().to(dev)
    tr = lambda t: t.t().contiguous()                                   # noqa: E731  the forward takes [H,4H]

    def fwd():
        return ops.decode_train_forward(dv["embedded"], dv["enc_out"], dv["h0"], dv["c0"], dv["start"], tr(dv["wih"]), tr(dv["whh"]),
                                        dv["bih"], dv["bhh"], dv["latent"], idxd, T, K, C, bool(use_tanh))
    d1, d2 = fwd(), fwd()
    saves = ("x_all", "gates_pre", "c_all", "h_all", "z0", "probs", "logp")
    assert all(_same_bits(d1[k], d2[k]) for k in saves)
    d1.update(wih=dv["wih"], whh=dv["whh"])
    de, dg, dx, dh0, dc0 = _twice(lambda: ops.decode_train_backward(d1, gscale.to(dev)))
    r64 = _decode_ref(w, idx, T, K, C, use_tanh, gscale, D)
    r32 = _decode_ref(w, idx, T, K, C, use_tanh, gscale, F32)
    got = dict(zip(saves, (d1[k] for k in saves)), d_enc_out=de, dgates=dg, dx=dx, dh0=dh0, dc0=dc0)
    for k, v in got.items():
        _yardstick("decode_train", k, v, r64[k], r32[k])
    assert torch.equal(dg.cpu()[gscale == 0], torch.zeros_like(dg.cpu()[gscale == 0]))   # gscale 0: no gradient at all


def test_decode_train_rejects_65_per_window(dev):
    ops = _ops()
    g = torch.Generator().manual_seed(1)
    w, idx, _ = _decode_inputs(1, 2, 65, 32, False, g)
    dv = {k: (v.to(dev) if v is not None else None) for k, v in w.items()}
    with pytest.raises(ops.GnnpnError, match="bad shape"):
        ops.decode_train_forward(dv["embedded"], dv["enc_out"], dv["h0"], dv["c0"], dv["start"], dv["wih"].t().contiguous(),
                                 dv["whh"].t().contiguous(), dv["bih"], dv["bhh"], None, idx.int().to(dev), 2, 65)


def _attn_run(dev, w, idx, T, K, C, use_tanh, gscale, bah, G):
    ops = _ops()
    H = w["enc_out"].shape[2]
    dv = {k: (v.to(dev) if v is not None else None) for k, v in w.items()}
    tr = lambda t: t.t().contiguous()                                   # noqa: E731
    side = lambda tag: ({"wq": dv[f"{tag}_wq"], "bq": dv[f"{tag}_bq"], "v": dv[f"{tag}_v"],               # noqa: E731
                         "wref": torch.eye(H, device=dev).view(H, H, 1) * (2.0 if tag == "p" else 0.5), "bref": torch.zeros(H, device=dev)}
                        if bah and f"{tag}_wq" in dv else None)
    d = ops.decode_attn_train_forward(dv["embedded"], dv["enc_out"], dv["h0"], dv["c0"], dv["start"], tr(dv["wih"]), tr(dv["whh"]),
                                      dv["bih"], dv["bhh"], dv["latent"], idx.int().to(dev), T, K, "Bahdanau" if bah else "Dot", G,
                                      side("p"), side("g"), C, bool(use_tanh))
    return d, dv


ATTN_CASES = [  # H, B, T, n_per, bahdanau, G, use_tanh, tanh_c, latent
    (32, 3, 5, 1, False, 1, 1, 10.0, True), (32, 2, 3, 64, False, 2, 0, 1.0, False), (256, 2, 4, 16, False, 8, 1, 10.0, True),
    (32, 3, 5, 1, True, 0, 1, 10.0, True), (256, 2, 3, 64, True, 1, 1, 5.0, False), (32, 2, 4, 17, True, 8, 0, 1.0, True),
    (32, 2, 2, 64, True, 1, 1, 10.0, True)]


@pytest.mark.parametrize("H,B,T,K,bah,G,use_tanh,C,latent", ATTN_CASES)
def test_decode_attn_train_forward_backward(dev, H, B, T, K, bah, G, use_tanh, C, latent):
    ops = _ops()
    g = torch.Generator().manual_seed(H * 100 + T * 10 + K + G)
    w, idx, gscale = _decode_inputs(B, T, K, H, latent, g, bah, G)
    saves = ("x_all", "gates_pre", "c_all", "h_all", "z0", "probs", "logp")
    outs = []
    for _ in range(2):
        d, dv = _attn_run(dev, w, idx, T, K, C, use_tanh, gscale, bah, G)
        d.update(wih=dv["wih"], whh=dv["whh"])
        back = ops.decode_attn_train_backward(d, gscale.to(dev))
        outs.append((d, back))
    (d, back), (d2, back2) = outs
    assert all(_same_bits(d[k], d2[k]) for k in saves + ("q_all",))
    assert all(_same_bits(a, b) for a, b in zip(back, back2))
    grads = ("d_p_ref", "d_p_qp", "d_p_v") + (("d_g_ref", "d_g_qp", "d_g_v") if G else ()) if bah else ()
    assert all(_same_bits(d[k], d2[k]) for k in grads)
    r64 = _decode_ref(w, idx, T, K, C, use_tanh, gscale, D, bah, G)
    r32 = _decode_ref(w, idx, T, K, C, use_tanh, gscale, F32, bah, G)
    got = dict({k: d[k] for k in saves + grads}, d_enc_out=back[0], dgates=back[1], dx=back[2], dh0=back[3], dc0=back[4])
    for k, v in got.items():
        _yardstick("decode_attn_train", k, v, r64[k], r32[k], floor_rel=1e-5)   # d ref: += over steps and rounds


def test_decode_attn_train_lds_limit(dev):
    """12,800 positions (T = 200, n_per = 64; H = 32, B = 1, one glimpse): the most the kernels take — past 64 KB of dynamic LDS
    in the backward — against the fp64 reference; 12,801 positions are refused before any launch."""
    ops = _ops()
    g = torch.Generator().manual_seed(128)
    T, K, H = 200, 64, 32
    w, idx, gscale = _decode_inputs(1, T, K, H, True, g, False, 1)
    d, dv = _attn_run(dev, w, idx, T, K, 10.0, 1, gscale, False, 1)
    d.update(wih=dv["wih"], whh=dv["whh"])
    back = ops.decode_attn_train_backward(d, gscale.to(dev))
    r64 = _decode_ref(w, idx, T, K, 10.0, 1, gscale, D, False, 1)
    r32 = _decode_ref(w, idx, T, K, 10.0, 1, gscale, F32, False, 1)
    for k, v in dict({k: d[k] for k in ("probs", "logp", "h_all")}, d_enc_out=back[0], dgates=back[1], dh0=back[3]).items():
        _yardstick("decode_attn_train_12800", k, v, r64[k], r32[k])
    w, idx, gscale = _decode_inputs(1, 251, 51, H, False, g, False, 1)
    with pytest.raises(ops.GnnpnError, match=r"\(-2\).*12801 positions"):
        _attn_run(dev, w, idx, 251, 51, 10.0, 1, gscale, False, 1)


# ---- evaluation helpers ------------------------------------------------------------------------------------------------------
def test_precision_at_k(dev):
    ops = _ops()
    g = torch.Generator().manual_seed(8)
    B, S = 37, 9
    ranking = torch.stack([torch.randperm(S, generator=g) for _ in range(B)]).int()
    labels = torch.tensor([0.0, 1.0, 2.0, 0.5, -1.0])[torch.randint(0, 5, (B, S), generator=g)]
    ks = (1, 5, S, S + 3)
    out = _twice(lambda: ops.precision_at_k(ranking.to(dev), labels.to(dev), ks)).cpu()
    for b in range(B):                                       # trainML.py:62-70: indices[:k] (all S where k > S), pat / k
        for i, k in enumerate(ks):
            hits = sum(1 for idx in ranking[b, :k].tolist() if labels[b, idx] == 1)
            assert out[b, i].item() == torch.tensor(hits / k, dtype=F32).item()
    from gnnpn_sc_amd import _lib
    lib = _lib.load()
    kt = torch.tensor([1, 0], dtype=I32, device=dev)
    o = torch.empty(B, 2, device=dev)
    r, lab = ranking.to(dev), labels.to(dev)
    args = lambda ld, kk: (_lib.dev_ptr(r, I32, "r"), ld, _lib.dev_ptr(lab, F32, "l"), S, B, S, _lib.dev_ptr(kk, I32, "k"), kk.numel(),   # noqa: E731
                           _lib.dev_ptr(o, F32, "o"), _lib.stream_ptr())
    assert lib.gnnpn_precision_at_k(*args(S, kt)) == -1                                  # k = 0 refused (the reference divides by it)
    assert lib.gnnpn_precision_at_k(*args(4, torch.tensor([1, 5], dtype=I32, device=dev))) == -1    # reads 5 entries of a 4-wide row
    assert lib.gnnpn_precision_at_k(*args(S, torch.tensor([1, 5], dtype=I32, device=dev))) == 0
    torch.cuda.synchronize()


def test_attention_logits(dev):
    ops = _ops()
    g = torch.Generator().manual_seed(12)
    B, T, K, H = 3, 5, 7, 256
    L = T * K
    enc, q = torch.randn(B, L, H, generator=g) * 0.1, torch.randn(B, T, H, generator=g) * 0.1
    idx = ((torch.arange(T) * K).unsqueeze(0) + torch.randint(0, K, (B, T), generator=g)).int()
    ed, qd, idd = enc.to(dev), q.to(dev), idx.to(dev)
    for step in (0, 2, T - 1):                               # ld_q = T * H > H: step selects the query row
        for use_tanh, C in ((True, 10.0), (False, 1.0)):
            out = _twice(lambda: ops.attention_logits(ed, qd, step, idd, C, use_tanh)).cpu()
            dot = torch.bmm(enc.double(), q[:, step].double().unsqueeze(2)).squeeze(2)
            ref = C * torch.tanh(dot) if use_tanh else dot
            mag = torch.bmm(enc.double().abs(), q[:, step].double().abs().unsqueeze(2)).squeeze(2)
            masked = torch.zeros(B, L, dtype=torch.bool)
            masked[torch.arange(B).unsqueeze(1), idx[:, :step].long()] = True
            assert torch.equal(out[masked], torch.full((int(masked.sum()),), float("-inf")))
            _bounded("attention_logits", "dot", out[~masked], ref[~masked], (C * 8 * math.sqrt(H) * U * mag + 4 * U * C * ref.abs().clamp(min=1e-3))[~masked])
    # 'Bahdanau': V . tanh(qp + ref) — against the fp32 yardstick
    qp, ref, v = torch.randn(B, H, generator=g) * 0.5, torch.randn(B, L, H, generator=g) * 0.5, torch.randn(H, generator=g) * 0.1
    for step in (0, T - 1):
        out = _twice(lambda: ops.attention_logits_bahdanau(ref.to(dev), qp.to(dev), v.to(dev), step, idd, 10.0, True)).cpu()
        f = lambda dt: 10.0 * torch.tanh((v.to(dt) * torch.tanh(qp.to(dt).unsqueeze(1) + ref.to(dt))).sum(2))   # noqa: E731
        masked = torch.zeros(B, L, dtype=torch.bool)
        masked[torch.arange(B).unsqueeze(1), idx[:, :step].long()] = True
        assert torch.isinf(out[masked]).all() and (out[masked] < 0).all()
        _yardstick("attention_logits_bahdanau", "logits", out[~masked], f(D)[~masked], f(F32)[~masked])
    with pytest.raises(ops.GnnpnError, match="dtype"):
        ops.attention_logits(ed, qd.double(), 1, idd)
    with pytest.raises(ops.GnnpnError, match="step"):
        ops.attention_logits(ed, qd, T, idd)
