"""-m gpu: one case per kernel BUILD (template instantiation) of the inference path that the rest of the suite does not reach, or
reaches without a CPU reference of its own (tests/golden/agreement_kernel_builds.json, tools/kernel_coverage.py).  Which build a
call gets is decided by host predicates on shape, alignment and options; every case here is named after the build it selects,
restates the predicate it relies on, compares the build's OWN output with a reference computed on the CPU in the same test
(float64, or the oracle's ordered fp32 restatement where the kernel is bit-exact by design) and runs the kernel twice for the
same bits.  Worst error / bound and yardstick ratios go to the agreement records kernel_builds_<family>."""
import numpy as np
import pytest
import torch

from kernel_checks import U, Recorder, twice
from oracle import ml as oml, pn as opn, tile_plan as otile
from parity import LOGIT_ATOL, TAU, TAU_DRAW, assert_R_parity, prefix_parity

pytestmark = pytest.mark.gpu
REC = Recorder("kernel_builds")
F32, I32 = torch.float32, torch.int32


def _ops():
    import gnnpn_sc_amd.custom_ops  # noqa: F401  (the C++ operators the model classes call)
    import gnnpn_sc_amd.ops as ops
    return ops


# ---- dense: linear_f32_kernel<BM, BN> -----------------------------------------------------------------------------------------
def dense_build(M, N, K):
    """The tile build gnnpn_linear_f32 launches for [M,K] x [N,K]^T (csrc/dense.hip), restated."""
    if -(-M // 128) * -(-N // 128) >= 256 and K >= 512 and N >= 256:
        return "128x128"
    if N % 128 == 0 and M >= 64 * 512:
        return "64x128"
    return "64x64"


# ragged M, N on both sides of the build's tile, K = 512 exactly and 515, k-tails of 1..3 (K % 4) and of the 32-wide k-tile,
# odd K (rows that start at 4-byte but not 8- or 16-byte aligned addresses: 135, 515), K below one vector (3)
DENSE_SHAPES = {
    "64x64": [(63, 65, 135), (65, 63, 515), (64, 64, 512), (127, 129, 33), (129, 127, 34), (70, 90, 35), (200, 130, 3), (1, 257, 7)],
    "64x128": [(32768, 128, 135), (32769, 256, 33), (32831, 128, 515), (32800, 128, 34), (32769, 128, 35), (32770, 128, 512)],
    "128x128": [(2048, 2048, 512), (2049, 1921, 515), (1999, 2050, 513), (16385, 256, 514), (2047, 2049, 647), (4000, 1025, 545)],
}


def _offset_view(t, dev, lead=1):
    """A copy of ``t`` on the device whose first element lies ``lead`` floats past a 16-byte aligned address."""
    flat = torch.empty(t.numel() + 4, dtype=F32, device=dev)
    assert flat.data_ptr() % 16 == 0
    v = flat[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * lead and v.is_contiguous()
    return v


def _linear_abi(dev, A, W, bias, scale, shift, act, pads, lead):
    """gnnpn_linear_f32 itself with lda = K + pads[0], ldw = K + pads[1], ldc = N + pads[2], the padding columns holding NaN (never
    read; C's never written) and every operand starting ``lead`` floats past a 16-byte boundary.  -> C [M,N] (a copy)."""
    from gnnpn_sc_amd import _lib
    from gnnpn_sc_amd._lib import check, dev_ptr, stream_ptr
    (M, K), N = A.shape, W.shape[0]
    pa, pw, pc = pads
    Ap = torch.full((M, K + pa), float("nan"))
    Ap[:, :K] = A
    Wp = torch.full((N, K + pw), float("nan"))
    Wp[:, :K] = W
    Ad, Wd = _offset_view(Ap, dev, lead), _offset_view(Wp, dev, lead)
    Cd = _offset_view(torch.full((M, N + pc), float("nan")), dev, lead)
    opt = [None if t is None else t.to(dev) for t in (bias, scale, shift)]
    check(_lib.load().gnnpn_linear_f32(dev_ptr(Ad, F32, "a"), K + pa, dev_ptr(Wd, F32, "w"), K + pw, dev_ptr(opt[0], F32, "bias", True),
                                       dev_ptr(opt[1], F32, "scale", True), dev_ptr(opt[2], F32, "shift", True), act,
                                       dev_ptr(Cd, F32, "c"), N + pc, M, N, K, stream_ptr()), "gnnpn_linear_f32")
    out = Cd.cpu()
    assert bool(torch.isnan(out[:, N:]).all()), "linear wrote into the padding columns of C"
    return out[:, :N].contiguous()


@pytest.mark.parametrize("build", sorted(DENSE_SHAPES))
def test_linear_build(dev, build):
    """Each tile build of gnnpn_linear_f32 on its own shapes.  Small-integer operands: every product and partial sum is exact in
    fp32 (|sum| <= 16 K + 4 < 2^24, the BN affine by small integers too), so the result must EQUAL the float64 one.  Random
    floats: |error| <= (K + 4) u (|A| |W|^T + |b|), u = 2^-24 — a bound of any summation order of K products, the bias add and
    slack for second-order terms, so it needs no measurement; through the BN affine the same quantity times |scale| plus one
    rounding of the result (the product's own rounding u |v scale| is inside the slack: the sum uses K + 1 of the K + 4);
    through the sigmoid (slope <= 1/4) a quarter of it plus the 1.5e-7 absolute of test_cell_activations."""
    ops = _ops()
    g = torch.Generator().manual_seed(len(build))
    for case, (M, N, K) in enumerate(DENSE_SHAPES[build]):
        assert dense_build(M, N, K) == build, (M, N, K)
        # exact: the C ABI with leading dimensions past the logical width and NaN in the padding, misaligned bases
        A, W = (torch.randint(-4, 5, s, generator=g).to(F32) for s in ((M, K), (N, K)))
        b, sc, sh = (torch.randint(-3, 4, (N,), generator=g).to(F32) for _ in range(3))
        lin = A.double() @ W.double().t() + b.double()
        pads = ((5, 3, 7), (1, 2, 3), (0, 0, 0))[case % 3]
        lead = (1, 3, 2)[case % 3]
        got = twice(lambda: _linear_abi(dev, A, W, b, None, None, ops.ACT_NONE, pads, lead))
        assert torch.equal(got, lin.float()), f"linear<{build}> {M}x{N}x{K}: integer product not exact"
        got = twice(lambda: _linear_abi(dev, A, W, b, sc, sh, ops.ACT_RELU, pads, lead))
        assert torch.equal(got, torch.relu(lin * sc.double() + sh.double()).float()), f"linear<{build}> {M}x{N}x{K}: BN+ReLU epilogue not exact"
        REC.note(f"linear_{build}", exact_cases=2)
        # random floats
        A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
        b, sh = torch.randn(N, generator=g), torch.randn(N, generator=g)
        sc = (torch.rand(N, generator=g) + 0.5) * (1 - 2 * (torch.rand(N, generator=g) < 0.3).float())
        prod = A.double() @ W.double().t()
        absprod = A.double().abs() @ W.double().abs().t()
        bound = (K + 4) * U * (absprod + b.double().abs()) + 1e-38
        lin = prod + b.double()
        # plain + bias, operands one float past a 16-byte boundary (the 16-byte loads of tile_load at 4-byte alignment)
        Ad, Wd = _offset_view(A, dev, 1 + case % 3), _offset_view(W, dev, 3 - case % 3)
        got = twice(lambda: ops.linear(Ad, Wd, b.to(dev)))
        REC.bounded(f"linear_{build}", "bias", got, lin, bound)
        # BN affine + ReLU, aligned operands through the wrapper
        aff = lin * sc.double() + sh.double()
        got = twice(lambda: ops.linear(A.to(dev), W.to(dev), b.to(dev), sc.to(dev), sh.to(dev), ops.ACT_RELU))
        REC.bounded(f"linear_{build}", "bn_relu", got, torch.relu(aff), bound * sc.double().abs() + U * aff.abs())
        # sigmoid without bias, padded leading dimensions
        got = twice(lambda: _linear_abi(dev, A, W, None, None, None, ops.ACT_SIGMOID, pads, lead))
        REC.bounded(f"linear_{build}", "sigmoid", got, torch.sigmoid(prod), 0.25 * (K + 4) * U * absprod + 1.5e-7)


# ---- the tiled aggregate: csr_aggregate_tiled_kernel<PASSES, HREGS, PAIRS> ---------------------------------------------------------
def _block_graph(S, copies, degree, seed, weighted, ragged=False):
    """``copies`` block-diagonal copies of a random graph of S rows whose neighbour lists are sorted by source (the reference's
    emission order) and end with the self loop; the last block optionally shorter.  -> rowptr, col, w (CPU), n."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 2 * degree + 1, S)
    deg[rng.integers(0, S, 3)] = 40 * degree                    # a few hub rows: many quads in one unit
    cols = [np.sort(rng.integers(0, S, d)) for d in deg]
    n = copies * S - (S // 3 if ragged else 0)
    rp, col = [0], []
    for r in range(n):
        b, i = divmod(r, S)
        c = cols[i] + b * S
        c = c[c < n]
        col.append(np.concatenate([c[c != r], [r]]))             # the self loop last (add_remaining_self_loops)
        rp.append(rp[-1] + len(col[-1]))
    col = np.concatenate(col)
    w = torch.from_numpy(rng.random(len(col), dtype=np.float32) + 0.05) if weighted else None
    return torch.tensor(rp, dtype=I32), torch.from_numpy(col.astype(np.int32)), w, n


def _aggregate_reference(rp, col, w, x, bias=None, scale=None, shift=None, relu=False, eps=None):
    """The oracle's ordered fp32 sum (oml.scatter_sum: each destination accumulates its messages in edge order, product and
    sum rounded separately) and the epilogue, on the CPU."""
    n = rp.numel() - 1
    dst = torch.repeat_interleave(torch.arange(n), (rp[1:] - rp[:-1]).long())
    msg = x[col.long()] if w is None else w.view(-1, 1) * x[col.long()]
    y = oml.scatter_sum(msg, dst, n)
    if eps is not None:
        y = y + (1 + eps) * x
    if bias is not None:
        y = y + bias
    if scale is not None:
        y = y * scale + shift
    return torch.relu(y) if relu else y


def tiled_build(S, n, pairs):
    """(PASSES, HREGS, PAIRS) gnnpn_csr_aggregate_tiled_f32 launches for blocks of S rows (csrc/graph_tiled.hip), from the oracle's
    geometry: 64 (source tile, pass) headers fit one register per lane, more need two — only with 7 or 8 source tiles."""
    g = otile.geometry(n, S)
    return g["passes"], (2 if g["passes"] >= 9 and g["NT"] * g["passes"] > 64 else 1), pairs


# every (PASSES, HREGS) the plan can produce: passes p = ceil(ceil16(S) / 256) for S <= 2560 (one source tile); two header
# registers need NT * passes > 64: S = 18000 -> 8 tiles x 9 passes, S = 20000 -> 8 x 10
TILED_S = {(p, 1): 256 * p - 9 for p in range(1, 11)}
TILED_S.update({(9, 2): 18000, (10, 2): 20000})
TILED_BUILDS = [(p, h, pairs) for (p, h) in sorted(TILED_S) for pairs in (False, True)]


@pytest.mark.parametrize("passes,hregs,pairs", TILED_BUILDS, ids=[f"{p}-{h}-{'pairs' if q else 'quads'}" for p, h, q in TILED_BUILDS])
def test_csr_aggregate_tiled_build(dev, monkeypatch, passes, hregs, pairs):
    """Each build of the tiled aggregate against the oracle's edge-order fp32 sums, bit for bit.  The walk (quads / pairs) is a
    speed choice of the launcher — pairs from three source tiles on — so a build of the other walk is only reachable through
    GNNPN_TILED_WALK: where the case sets it, it asserts that the default rule would have taken the other walk."""
    ops = _ops()
    S = TILED_S[(passes, hregs)]
    copies, C, ragged = (1, 16, False) if hregs == 2 else (3, 32, True)
    rp, col, w, n = _block_graph(S, copies, 5, 100 * passes + hregs, weighted=passes % 2 == 1, ragged=ragged)
    assert tiled_build(S, n, pairs) == (passes, hregs, pairs)
    default_pairs = otile.geometry(n, S)["NT"] >= 3
    if pairs != default_pairs:
        monkeypatch.setenv("GNNPN_TILED_WALK", "pairs" if pairs else "quads")     # the default call takes the other walk
    else:
        monkeypatch.delenv("GNNPN_TILED_WALK", raising=False)
    g = torch.Generator().manual_seed(S)
    x = torch.randn(n, C, generator=g)
    bias, scale, shift = (torch.randn(C, generator=g) for _ in range(3))
    rpd, cold, wd = rp.to(dev), col.to(dev), None if w is None else w.to(dev)
    plan = ops.csr_tile_plan(rpd, cold, wd, S)
    assert plan.valid and plan.geom["passes"] == passes and plan.geom["src_tiles"] == otile.geometry(n, S)["NT"], plan.stats
    got = twice(lambda: plan.aggregate(x.to(dev), None, bias.to(dev), scale.to(dev), shift.to(dev), ops.ACT_RELU))
    assert torch.equal(got.cpu(), _aggregate_reference(rp, col, w, x, bias, scale, shift, relu=True))
    eps = torch.tensor([0.125])
    got = twice(lambda: plan.aggregate(x.to(dev), eps.to(dev)))                   # the GIN self term, no epilogue
    assert torch.equal(got.cpu(), _aggregate_reference(rp, col, w, x, eps=eps))
    REC.note("csr_aggregate_tiled", exact_cases=2)


# ---- the LDS-staged aggregate: csr_aggregate_lds_kernel<LPR, WEIGHTED> -----------------------------------------------------------
def lds_build(S, C, weighted):
    """(lanes per row, weighted) of gnnpn_csr_aggregate_blocks_f32 (csrc/graph.hip): the widest slice of 16 / 8 / 4 channels that
    divides C and whose block of S + 1 rows fits 160 KB of LDS."""
    return next(c for c in (4, 2, 1) if C % (4 * c) == 0 and (S + 1) * 16 * c <= 160 * 1024), weighted


LDS_CASES = {(4, True): (700, 32), (4, False): (333, 48), (2, True): (2700, 32), (2, False): (300, 24), (1, True): (5200, 16),
             (1, False): (300, 20)}


@pytest.mark.parametrize("lpr,weighted", sorted(LDS_CASES))
def test_csr_aggregate_lds_build(dev, lpr, weighted):
    """Each build of the whole-block LDS-staged aggregate (the C entry point itself, with and without the row order) against the
    oracle's edge-order sums, bit for bit: slices of 16, 8 and 4 channels, picked by divisibility of C and by the block size."""
    ops = _ops()
    from gnnpn_sc_amd import _lib
    from gnnpn_sc_amd._lib import check, dev_ptr, stream_ptr
    S, C = LDS_CASES[(lpr, weighted)]
    assert lds_build(S, C, weighted) == (lpr, weighted)
    rp, col, w, n = _block_graph(S, 3, 6, 7 * S + C, weighted, ragged=True)
    g = torch.Generator().manual_seed(C)
    x, bias = torch.randn(n, C, generator=g), torch.randn(C, generator=g)
    want = _aggregate_reference(rp, col, w, x, bias, relu=True)
    rpd, cold, wd, xd, bd = rp.to(dev), col.to(dev), None if w is None else w.to(dev), x.to(dev), bias.to(dev)
    # the row order is a schedule (csr_block_order_kernel): per block the rows by descending number of edges, ties by ascending row
    deg = (rp[1:] - rp[:-1]).long()
    want_order = torch.cat([b0 + torch.sort(deg[b0:b0 + S], descending=True, stable=True).indices for b0 in range(0, n, S)])
    order_dev = twice(lambda: ops.csr_block_row_order(rpd, S))
    assert torch.equal(order_dev.cpu().long(), want_order)
    for order in (order_dev, None):
        def run():
            y = torch.full_like(xd, float("nan"))
            check(_lib.load().gnnpn_csr_aggregate_blocks_f32(
                dev_ptr(rpd, I32, "rp"), dev_ptr(cold, I32, "col"), dev_ptr(wd, F32, "w", True), dev_ptr(xd, F32, "x"), C, None,
                dev_ptr(bd, F32, "b"), None, None, ops.ACT_RELU, dev_ptr(y, F32, "y"), C, n, C, S, dev_ptr(order, I32, "order", True),
                stream_ptr()), "gnnpn_csr_aggregate_blocks_f32")
            return y
        assert torch.equal(twice(run).cpu(), want)
    REC.note("csr_aggregate_lds", exact_cases=2)


# ---- the streaming encoder: lstm_encode_kernel<H, BT> ------------------------------------------------------------------------------
def encode_bt(B, nets):
    """Problems per workgroup of the streaming encoder (csrc/lstm.hip launch_encode)."""
    bt = 1
    while bt < 8 and B * nets // (bt * 2) >= 256:
        bt *= 2
    return bt


ENCODE_B = {1: 3, 2: 259, 4: 515, 8: 1029}     # two nets: B * 2 = 6, 518, 1030, 2058; the last workgroup holds 1, 3 and 5 problems


@pytest.mark.parametrize("H,BT", [(H, BT) for H in (256, 32) for BT in (1, 2, 4, 8)])
def test_lstm_encode_streaming_build(dev, H, BT):
    """Each build of the per-workgroup encoder against the same recurrence in float64 on the CPU (torch.nn.LSTM in double),
    held to the yardstick of torch's own fp32 LSTM on the same inputs (factor 4, floor 2e-6).  Batch sizes select BT by the
    launcher's rule and leave the last workgroup partly filled (b0 + p >= B for some p); two different nets in one launch."""
    ops = _ops()
    B, L, nets = ENCODE_B[BT], 7, 2
    assert encode_bt(B, nets) == BT and (BT == 1 or B % BT != 0)
    # H = 256 with a workspace takes the cooperative form by default: the streaming form (the reference of the bit-for-bit
    # comparisons, and the fallback on partitioned devices) has to be asked for; H = 32 has no other form
    assert ops.coop_supported(H) == (H == 256)
    impl = 1 if H == 256 else 0
    x = torch.randn(B, L, H, generator=torch.Generator().manual_seed(H + BT)) * 0.5
    args, refs = [], []
    for seed in (5, 6):
        sd = opn.make_state_dict(H, seed)
        with torch.no_grad():
            o32, (h32, c32) = opn._lstm_module(sd, "encoder", H)(x)
            o64, (h64, c64) = opn._lstm_module(sd, "encoder", H).double()(x.double())
        refs.append(((o64, o32), (h64[0], h32[0]), (c64[0], c32[0])))
        pre = ops.linear(x.view(B * L, H).to(dev), sd["actor.encoder.weight_ih_l0"].to(dev), sd["actor.encoder.bias_ih_l0"].to(dev))
        args.append({"pregates": pre.view(B, L, 4 * H), "whh": ops.pack_lstm_weight(sd["actor.encoder.weight_hh_l0"]).to(dev),
                     "bhh": sd["actor.encoder.bias_hh_l0"].to(dev)})
    enc, h_n, c_n = twice(lambda: ops.lstm_encode(args, impl=impl))
    for n in range(nets):
        for what, got, (r64, r32) in zip(("enc_out", "h_n", "c_n"), (enc[n], h_n[n], c_n[n]), refs[n]):
            assert got.shape == r64.shape
            REC.yardstick(f"lstm_encode_{H}_{BT}", what, got, r64, r32)


# ---- the streaming decoder: pointer_decode_kernel<H, BT, REP> -----------------------------------------------------------------------
def decode_bt(rows):
    """Problems (replica rows) per workgroup of the streaming decoder (csrc/decode.hip launch_decode)."""
    bt = 1
    while bt < 4 and rows // (bt * 2) >= 256:
        bt *= 2
    return bt


def _pn_models(H, T, K, dev):
    from gnnpn_sc_amd.modelPN import CombinatorialRL, reward
    nets = []
    for level, seed in (("Low", 1), ("High", 2)):
        m = CombinatorialRL(0, H, T * K, 0, 10, 1, reward, "Dot", K, T, use_cuda=True, level=level)
        m.load_state_dict(opn.make_state_dict(H, seed), strict=True)
        nets.append(m.to(dev).eval())
    return nets[0], nets[1], opn.make_state_dict(H, 1), opn.make_state_dict(H, 2)


def _robust_share(ref, tau_high=TAU):
    """Share of a case's decisions that lie before their problem's first fragile decision, from the ORACLE alone."""
    frag = (np.asarray(ref["margin_low"]) <= TAU) | (np.asarray(ref["margin_high"]) <= tau_high)
    T = frag.shape[1]
    return float(np.where(frag.any(1), frag.argmax(1), T).sum()) / frag.size


def _check_against_oracle(name, what, out, ref, x, tau_high=None):
    """prefix_parity (no decision before a problem's first fragile one may differ) + window logits, actions and R on the problems
    followed to the end.  ``out``: idx_low, idx_high, R and optionally win_low / win_high."""
    rec = prefix_parity(out["idx_low"], out["idx_high"], ref, what, rows=x, tau_high=tau_high)
    s = rec.pop("same_mask")
    assert rec["identical_decisions"] >= rec["robust_prefix_decisions"] > 0
    assert s.any()
    if "win_low" in out:
        assert float((out["win_low"].cpu()[s] - ref["win_low"][s]).abs().max()) < LOGIT_ATOL
        assert float((out["win_high"].cpu()[s] - ref["win_high"][s]).abs().max()) < LOGIT_ATOL
    rec["max_dR_units"] = assert_R_parity(out["R"], ref["R"], what, mask=s)
    REC.note(name, identical_share=rec["identical_decisions"] / (2 * rec["problems"] * rec["steps"]), flips=rec["flips"],
             max_dR_units=rec["max_dR_units"])
    return rec


# greedy builds: (H, BT) -> (B, T, K); robust-prefix shares of these cases from the oracle: 0.86 .. 0.99 (asserted >= 0.8 below)
DECODE_GREEDY = {(256, 1): (41, 6, 3), (256, 2): (521, 5, 8), (256, 4): (1030, 6, 3), (32, 1): (41, 9, 16), (32, 2): (521, 5, 8),
                 (32, 4): (1030, 6, 3)}


@pytest.mark.parametrize("H,BT", sorted(DECODE_GREEDY))
def test_pointer_decode_streaming_build(dev, H, BT):
    """Each greedy build of the per-workgroup decoder against oracle.pn.two_level_greedy.  The batch selects BT by the
    launcher's rule with a partly filled last workgroup.  So that prefix_parity (which stops following a problem at its first
    fragile decision) cannot hide a failure, the robust prefix — computed from the oracle alone, before the kernel runs —
    must hold at least 80 % of the case's decisions; every decision in it must be identical."""
    from gnnpn_sc_amd.modelPN import two_level_greedy
    from pn_inputs import pn_inputs
    ops = _ops()
    B, T, K = DECODE_GREEDY[(H, BT)]
    assert decode_bt(B) == BT and (BT == 1 or B % BT != 0)
    low, high, sd_low, sd_high = _pn_models(H, T, K, dev)
    x = pn_inputs(B, T, K, 7)
    ref = opn.two_level_greedy(sd_low, sd_high, x, T, K)
    share = _robust_share(ref)
    assert share >= 0.8, share
    # H = 256, n_per <= 16 takes the cooperative decoder by default: the streaming form has to be asked for
    assert ops.coop_supported(H, K) == (H == 256)
    xd = x.to(dev)
    out = twice(lambda: two_level_greedy(low, high, xd, precision="f32", decode_impl=1 if H == 256 else 0))
    ops.check_status(dev)
    out = dict(out, win_high=out["win_high_raw"] + out["win_low"])
    _check_against_oracle(f"pointer_decode_{H}_{BT}_greedy", f"decode<{H},{BT},false>", out, ref, x)
    same = (out["idx_high"].cpu().long() == ref["idx_high"]).all(1)
    assert torch.equal(out["actions"].cpu()[same], ref["actions"][same])          # the rows of the picks, gathered in the kernel
    REC.note(f"pointer_decode_{H}_{BT}_greedy", robust_prefix_share=share)


# weights scaled until window logits tie EXACTLY: at H = 256 the recurrent weights x 6 saturate 10 * tanh to 10.0f (the recipe of
# the pn_saturated fixture); 32-term dots do not get there, so at H = 32 embedding2 is scaled too, x 100
SATURATE = {256: (6.0, ("encoder", "decoder.")), 32: (100.0, ("encoder", "decoder.", "embedding2"))}


@pytest.mark.parametrize("H,BT", sorted(DECODE_GREEDY))
def test_pointer_decode_streaming_build_first_max(dev, H, BT):
    """Exact ties inside a window: torch.max on the CPU takes the FIRST maximum, and so must every greedy build.  Wherever a
    problem's history equals the oracle's and the kernel's Low window shows the same set of tied maxima as the oracle's (two
    or more), the pick must be the oracle's; at least three such ties per case (a tie has margin 0, so prefix_parity alone
    would class a wrong pick there as fragile)."""
    from gnnpn_sc_amd.modelPN import CombinatorialRL, reward, two_level_greedy
    from pn_inputs import pn_inputs
    B, T, K = DECODE_GREEDY[(H, BT)]
    assert decode_bt(B) == BT
    scale, keys = SATURATE[H]
    nets, sds = [], []
    for level, seed in (("Low", 1), ("High", 2)):
        sd = opn.make_state_dict(H, seed)
        for k in sd:
            if any(part in k for part in keys):
                sd[k] = sd[k] * scale
        m = CombinatorialRL(0, H, T * K, 0, 10, 1, reward, "Dot", K, T, use_cuda=True, level=level)
        m.load_state_dict(sd, strict=True)
        nets.append(m.to(dev).eval())
        sds.append(sd)
    x = pn_inputs(B, T, K, 7)
    ref = opn.two_level_greedy(sds[0], sds[1], x, T, K)
    out = twice(lambda: two_level_greedy(nets[0], nets[1], x.to(dev), fold=False, precision="f32", decode_impl=1 if H == 256 else 0))
    got, want = out["idx_low"].cpu().long(), ref["idx_low"]
    same_before = torch.cat([torch.ones(B, 1, dtype=torch.bool), (got == want).cumprod(1).bool()[:, :-1]], 1)   # history equal up to the step
    tie_ref = ref["win_low"] == ref["win_low"].max(-1, keepdim=True).values
    win = out["win_low"].cpu()
    tie_got = win == win.max(-1, keepdim=True).values
    comparable = same_before & (tie_ref.sum(-1) >= 2) & (tie_got == tie_ref).all(-1)
    assert int(comparable.sum()) >= 3, f"only {int(comparable.sum())} exact ties were comparable"
    first = torch.arange(T).view(1, T) * K + tie_ref.int().argmax(-1)
    assert torch.equal(want[comparable], first[comparable])                 # the oracle's rule is the first maximum
    assert torch.equal(got[comparable], want[comparable]), f"decode<{H},{BT},false>: a tie was not resolved to the first maximum"
    REC.note(f"pointer_decode_{H}_{BT}_greedy", ties_checked=int(comparable.sum()))


# replica builds: (H, BT) -> (B, samples, T, K); rows = B * (samples - 1) = 63, 515, 1035
DECODE_REPLICAS = {(256, 1): (21, 4, 6, 3), (256, 2): (103, 6, 5, 8), (256, 4): (207, 6, 6, 3), (32, 1): (21, 4, 6, 3),
                   (32, 2): (103, 6, 5, 8), (32, 4): (207, 6, 9, 16)}


@pytest.mark.parametrize("H,BT", sorted(DECODE_REPLICAS))
def test_pointer_decode_replica_build(dev, H, BT):
    """Each replica (REP = true) build of the per-workgroup decoder: replica j of one best-of launch against the oracle's sampled
    forward with sample_seed = replica_seed(seed, j) (Low greedy, High drawn from the same counter-based stream), under
    prefix_parity with the draw margin TAU_DRAW; the same 80 % condition on every replica, from the oracle alone."""
    from gnnpn_sc_amd.modelPN import two_level_best_of
    from pn_inputs import pn_inputs
    ops = _ops()
    B, N, T, K = DECODE_REPLICAS[(H, BT)]
    rows = B * (N - 1)
    assert decode_bt(rows) == BT and (BT == 1 or rows % BT != 0)
    low, high, sd_low, sd_high = _pn_models(H, T, K, dev)
    x = pn_inputs(B, T, K, 7)
    seed = 0xB0F + H + BT
    refs = [opn.two_level_greedy(sd_low, sd_high, x, T, K, sample_high_seed=ops.replica_seed(seed, j)) for j in range(1, N)]
    shares = [_robust_share(r, TAU_DRAW) for r in refs]
    assert min(shares) >= 0.8, shares
    assert ops.coop_supported(H, K) == (H == 256)        # the default call takes the cooperative replica launch at H = 256
    xd = x.to(dev)
    out = twice(lambda: two_level_best_of(low, high, xd, N, seed=seed, precision="f32", decode_impl=1 if H == 256 else 0))
    differs = 0
    for j, ref in enumerate(refs, start=1):
        got = {"idx_low": out["idx_low"], "idx_high": out["idx_all"][:, j], "R": out["R_all"][:, j]}
        _check_against_oracle(f"pointer_decode_{H}_{BT}_replicas", f"decode<{H},{BT},true> replica {j}", got, ref, x, tau_high=TAU_DRAW)
        differs += int((out["idx_all"][:, j] != out["idx_all"][:, 0]).any(1).sum())
    assert differs > 0.05 * rows                          # the draws are not the argmax
    REC.note(f"pointer_decode_{H}_{BT}_replicas", robust_prefix_share=min(shares))


# ---- the cooperative encoder: lstm_encode_coop_kernel<PREC, PRE, DIAG> --------------------------------------------------------------
ENCODE_COOP = [("f32", False, False), ("f32", True, False), ("f32", False, True), ("f16", False, False), ("f16", True, False),
               ("split", False, False), ("split", True, False), ("split", False, True)]


@pytest.mark.parametrize("precision,pre,diag", ENCODE_COOP, ids=[f"{p}-{'pregates' if q else 'folded'}{'-stamps' if d else ''}" for p, q, d in ENCODE_COOP])
def test_lstm_encode_cooperative_build(dev, precision, pre, diag):
    """Each build of the cooperative encoder (arithmetic of the recurrent product x input side x the phase-stamp diagnostic
    build) against the float64 evaluation of embedding2 -> LSTM on the CPU, two nets in one launch.  "f32" and "split" (exact
    three-piece operands) are held to the fp32 yardstick (factor 4, floor 2e-6).  "f16" rounds W_hh and h to fp16 by design
    (unit roundoff 2^-11 per operand): it is held to 10 x 2^-11 = 4.9e-3 absolute — the bar the project set for this option
    (5e-3 against the fp32 path) read against float64 — and must differ from the fp32 build (else the option did nothing).
    The stamped builds (timing diagnostics: GNNPN_ABLATE_ENC_STAMPS, folded input side only) give results like any other build."""
    from pn_inputs import pn_inputs
    ops = _ops()
    H, B, T, K = 256, 37, 6, 3
    low, high, sd_low, sd_high = _pn_models(H, T, K, dev)
    x = pn_inputs(B, T, K, 7)
    xd = x.to(dev)
    args = [m.actor.encode_args(xd, fold=not pre)[0] for m in (low, high)]
    assert all((a.get("pregates") is not None) == pre for a in args)
    assert ops.coop_supported(H)                                      # the default form at H = 256: nothing is forced
    try:
        if diag:
            ops.set_option("lstm_ablate", ops.GNNPN_ABLATE_ENC_STAMPS)   # the only way into the stamped builds (tools/ablate_encode.py)
        enc, h_n, c_n = twice(lambda: ops.lstm_encode(args, precision=precision))
        ops.check_status(dev)
    finally:
        ops.set_option("lstm_ablate", 0)
    f32 = ops.lstm_encode(args)[0] if precision == "f16" else None
    name = f"lstm_encode_coop_{precision}_{'pre' if pre else 'fold'}{'_diag' if diag else ''}"
    for n, sd in enumerate((sd_low, sd_high)):
        with torch.no_grad():
            emb32 = torch.nn.functional.linear(x, sd["actor.embedding2.weight"], sd["actor.embedding2.bias"])
            emb64 = torch.nn.functional.linear(x.double(), sd["actor.embedding2.weight"].double(), sd["actor.embedding2.bias"].double())
            o32, (h32, c32) = opn._lstm_module(sd, "encoder", H)(emb32)
            o64, (h64, c64) = opn._lstm_module(sd, "encoder", H).double()(emb64)
        for what, got, r64, r32 in (("enc_out", enc[n], o64, o32), ("h_n", h_n[n], h64[0], h32[0]), ("c_n", c_n[n], c64[0], c32[0])):
            if precision == "f16":
                REC.bounded(name, what, got, r64, torch.full_like(r64, 10 * 2.0 ** -11))
            else:
                REC.yardstick(name, what, got, r64, r32)
        if precision == "f16":
            assert float((enc[n] - f32[n]).abs().max()) > 0


# ---- the cooperative decoders: pointer_decode_lean_kernel<SPLIT, OCC, EVH, DIAG>, pointer_decode_coop_kernel<FOLD, SAMPLE> ----------
# build -> (precision, decode_impl, K, fold, stamps, sampled).  decode_lean.hip: OCC = 2 is the 256-register build for two
# workgroups per CU (impl 4), EVH = 1 the wide windows (n_per 9..16), DIAG the phase-stamp build (GNNPN_ABLATE_DEC_STAMPS, n_per <= 8).
# decode_coop.hip: <false,false> the literal two-stage input side (fold off), <true,true> every High pick drawn.
DECODE_COOP = {
    "lean<false,1,1,false>": ("f32", 2, 10, True, False, False), "lean<false,1,2,false>": ("f32", 2, 3, True, False, False),
    "lean<false,1,2,true>": ("f32", 2, 3, True, True, False), "lean<false,2,1,false>": ("f32", 4, 10, True, False, False),
    "lean<false,2,2,false>": ("f32", 4, 3, True, False, False), "lean<true,1,1,false>": ("split", 2, 10, True, False, False),
    "lean<true,1,2,false>": ("split", 2, 3, True, False, False), "lean<true,1,2,true>": ("split", 2, 3, True, True, False),
    "lean<true,2,1,false>": ("split", 4, 10, True, False, False), "lean<true,2,2,false>": ("split", 4, 3, True, False, False),
    "coop<false,false>": ("f32", 2, 3, False, False, False), "coop<true,true>": ("f32", 2, 3, True, False, True),
}


@pytest.mark.parametrize("build", sorted(DECODE_COOP))
def test_pointer_decode_cooperative_build(dev, build):
    """Each build of the cooperative decoders against oracle.pn.two_level_greedy (the sampling build: the oracle's sampled
    forward on the same stream), under prefix_parity with the 80 % robust-prefix condition computed from the oracle alone.  The
    batch (70 problems: 4 full tiles of 16 and one of 6) is decoded by the cooperative form by default; decode_impl 4 and the
    stamp bit are the only ways into the 2-per-CU and the stamped builds, which no default call picks."""
    from gnnpn_sc_amd.modelPN import two_level_greedy
    from pn_inputs import pn_inputs
    ops = _ops()
    precision, impl, K, fold, stamps, sampled = DECODE_COOP[build]
    H, B, T = 256, 70, 6 if K == 3 else 4
    low, high, sd_low, sd_high = _pn_models(H, T, K, dev)
    x = pn_inputs(B, T, K, 7)
    seed = 0xC0DE if sampled else None
    ref = opn.two_level_greedy(sd_low, sd_high, x, T, K, sample_high_seed=seed)
    tau_high = TAU_DRAW if sampled else None
    share = _robust_share(ref, TAU_DRAW if sampled else TAU)
    assert share >= 0.8, share
    assert ops.coop_supported(H, K)
    xd = x.to(dev)
    try:
        if stamps:
            ops.set_option("lstm_ablate", ops.GNNPN_ABLATE_DEC_STAMPS)
        out = twice(lambda: two_level_greedy(low, high, xd, fold=fold, precision=precision, decode_impl=impl, sample_high_seed=seed))
        ops.check_status(dev)
    finally:
        ops.set_option("lstm_ablate", 0)
    out = dict(out, win_high=out["win_high_raw"] + out["win_low"])
    name = "pointer_decode_" + build.replace("<", "_").replace(">", "").replace(",", "_")
    _check_against_oracle(name, build, out, ref, x, tau_high=tau_high)
    REC.note(name, robust_prefix_share=share)


# ---- the request branch: gin_request_branch_kernel<LAYERS> --------------------------------------------------------------------------
@pytest.mark.parametrize("n_gin", [1, 2, 3, 4])
def test_request_branch_build(dev, n_gin):
    """The fused GIN branch with 1..4 layers (one build each; 4 is also the build of deeper stacks) against the oracle's
    request embedding on the CPU, at the tolerance the suite holds this branch to (1e-5 on O(1) values: the dense layers are
    k-ordered fp32 chains, the oracle's are MKL's), graphs of 1..11 nodes."""
    import gnnpn_sc_amd.synth as synth
    from gnnpn_sc_amd.modelML import Net
    from gnnpn_sc_amd.pipeline import DeviceBatch
    T, S, B, n_t = 20, 80, 37, 10
    table = synth.make_service_table(T, S, seed=1, degree=4)
    pb = synth.make_problem_batch(table, B, seed=B + n_gin, tasks_per_problem=n_t)
    sd = oml.make_state_dict(128, 20, n_gin, 2, seed=3)
    net = Net(128, S, 20, n_gin, 2)
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    batch = DeviceBatch.from_problems(pb, dev)
    assert 0 < batch.max_nodes <= 16                                   # the fused form is what the model takes for such graphs
    got = twice(lambda: net.request_embedding(batch.x, batch.wf_csr, batch.seg_ptr, batch.max_nodes))
    ref = oml.request_embedding(sd, torch.from_numpy(pb.x), torch.from_numpy(pb.edge_index), torch.from_numpy(pb.batch), B, n_gin)
    err = float((got.cpu() - ref).abs().max())
    REC.note(f"gin_request_branch_{n_gin}", max_abs_err=err, scale=float(ref.abs().max()))
    assert got.shape == ref.shape and err < 1e-5, err


# ---- candidate selection: select_candidates16_kernel<8>, <16>, select_candidates_kernel -----------------------------------------------
def select_build(n_per, S, T):
    """Which launch gnnpn_select_candidates takes (csrc/select.hip): 8 lanes per (problem, category) for n_per <= 8 where the
    categories average at most 8 services, 16 lanes for n_per <= 16, else a whole wave."""
    return "16<8>" if n_per <= 8 and S <= 8 * T else "16<16>" if n_per <= 16 else "wave"


SELECT_CASES = {"16<8>": [(12, 60, 5), (10, 80, 8), (9, 30, 1)], "16<16>": [(6, 120, 12), (6, 120, 5), (5, 100, 16)],
                "wave": [(6, 180, 20), (4, 300, 64), (5, 40, 17)]}


@pytest.mark.parametrize("build", sorted(SELECT_CASES))
def test_select_candidates_build(dev, build):
    """Each launch of the candidate reduction against oracle.data.reduce_candidates (the reference's loadDataPN with rank
    order defined) on synthetic tables in the reference's formats: absent categories (fewer tasks than categories), bounds
    tight enough to leave categories with nothing feasible (dummy rows) or fewer feasible services than n_per (cyclic
    padding), categories smaller than n_per, and score ties (lowest id first)."""
    import gnnpn_sc_amd.synth as synth
    from parity import oracle_candidate_rows
    ops = _ops()
    seen = {"dummy": 0, "cyclic": 0, "ties": 0}
    for case, (T, S, K) in enumerate(SELECT_CASES[build]):
        assert select_build(K, S, T) == build
        B = 11
        table = synth.make_service_table(T, S, seed=20 + case, degree=4)
        pb = synth.make_problem_batch(table, B, seed=30 + case, tasks_per_problem=max(1, T - 2), lo_range=((0.93, 0.99), (0.85, 0.96), (0.97, 0.999))[case])
        g = torch.Generator().manual_seed(S + K)
        scores = torch.randint(0, 24, (B, S), generator=g).float() / 24          # many exact ties
        rank = oml.rank_services(scores).numpy()
        want = oracle_candidate_rows(pb, table, rank, K, pb.x.shape[0] // B)
        rows, ids = twice(lambda: ops.select_candidates(
            scores.to(dev), torch.from_numpy(table.cat_ptr).to(dev), torch.from_numpy(table.qos).to(dev),
            torch.from_numpy(pb.local_bounds).to(dev), torch.from_numpy(pb.present).to(dev), torch.from_numpy(pb.global_bounds).to(dev), K))
        assert torch.equal(rows.cpu().view(want.shape), want), (T, S, K)
        idv = ids.cpu().view(B, T, K)
        seen["dummy"] += int((idv == -1).all(-1).sum())
        repeats = (np.diff(np.sort(idv.numpy(), -1), axis=-1) == 0).any(-1) if K > 1 else np.zeros((B, T), bool)
        seen["cyclic"] += int((repeats & (idv[:, :, 0] >= 0).numpy()).sum())          # fewer feasible than n_per: emitted cyclically
        seen["ties"] += int((np.diff(np.sort(scores.numpy(), 1), axis=1) == 0).sum())
    assert seen["dummy"] > 0 and seen["ties"] > 0 and seen["cyclic"] > 0, seen
    REC.note("select_candidates_" + build.replace("<", "_").replace(">", ""), exact_cases=len(SELECT_CASES[build]), **seen)


# ---- the fused GIN layer: gin_layer_kernel<WITH_LIN> ---------------------------------------------------------------------------------
@pytest.mark.parametrize("with_lin", [False, True])
def test_gin_layer_build(dev, with_lin):
    """Both builds of the fused fp32 GIN layer (with and without the closing nodeLin) against a float64 evaluation on the CPU
    from the oracle's ordered fp32 aggregate (oml.scatter_sum + (1 + eps) x: bit for bit what the kernel's first stage forms;
    the [rows x 256] intermediate rounded to fp32 where the kernel holds it in fp32), held to the yardstick of the same layer
    in torch fp32 on the CPU (factor 4, floor 2e-6).  Chain graphs with a ragged last row tile and long-range edges."""
    from gnnpn_sc_amd import graph
    ops = _ops()
    n, c_in, nodes_per_graph = 1237, 26 if with_lin else 128, 50
    g = torch.Generator().manual_seed(n + c_in)
    i = torch.arange(n - 1)
    keep = (i + 1) % nodes_per_graph != 0
    src = torch.stack([i[keep], i[keep] + 1], 1).reshape(-1)
    dst = torch.stack([i[keep] + 1, i[keep]], 1).reshape(-1)
    ei = torch.cat([torch.stack([src, dst]), torch.randint(0, n, (2, n // 3), generator=g)], 1)
    x = torch.randn(n, c_in, generator=g)
    eps = torch.tensor([0.07])
    mk = lambda *s: torch.randn(*s, generator=g) / s[-1] ** 0.5   # noqa: E731
    w1, b1, w2, b2, w3, b3 = mk(256, c_in), mk(256), mk(128, 256), mk(128), mk(128, 128), mk(128)
    a1, s1, a2, s2 = torch.rand(256, generator=g) + 0.5, mk(256), torch.rand(128, generator=g) + 0.5, mk(128)
    agg = oml.scatter_sum(x[ei[0]], ei[1], n) + (1 + eps) * x
    refs = []
    for cast in (torch.double, torch.float):
        c = lambda t: t.to(cast)   # noqa: E731
        t = torch.relu((c(agg) @ c(w1).t() + c(b1)) * c(a1) + c(s1)).float().to(cast)
        r = torch.relu((t @ c(w2).t() + c(b2)) * c(a2) + c(s2))
        if with_lin:
            r = r.float().to(cast) @ c(w3).t() + c(b3)
        refs.append(r)
    csr = graph.csr_by_destination(ei, n).to(dev)
    d = lambda t: t.to(dev)   # noqa: E731
    q1, q2, q3 = (ops.pack_mfma_b32(d(w)) for w in (w1, w2, w3))
    got = twice(lambda: ops.gin_layer(csr.rowptr, csr.col, d(x), d(eps), q1, d(b1), d(a1), d(s1), q2, d(b2), d(a2), d(s2),
                                      q3 if with_lin else None, d(b3) if with_lin else None))
    assert got.shape == refs[0].shape
    REC.yardstick(f"gin_layer_{'lin' if with_lin else 'plain'}", "out", got, refs[0], refs[1])


# ---- whh_split operands ----------------------------------------------------------------------------------------------------------
def test_whh_split_of_the_wrong_size_is_refused(dev):
    """The split-weight image of a net is read in full by the kernels (gnnpn_lstm_split_weights_bytes() bytes): an operand of any
    other size, or on another device than its weights, is refused by the C++ operators and by the ctypes wrappers before
    anything is launched (the outputs are not even allocated); the image the model makes is accepted."""
    from gnnpn_sc_amd import _lib, custom_ops
    from pn_inputs import pn_inputs
    ops = _ops()
    H, T, K = 256, 3, 2
    low, high, _, _ = _pn_models(H, T, K, dev)
    x = pn_inputs(5, T, K, 7).to(dev)
    need = int(_lib.load().gnnpn_lstm_split_weights_bytes())
    enc_args, emb = low.actor.encode_args(x)
    assert enc_args["whh_split"].numel() == need and enc_args["whh_split"].dtype == torch.uint8
    enc, h_n, c_n = custom_ops.lstm_encode([enc_args], precision="split")
    dec_args = low.actor.decode_args(emb, enc[0], h_n[0], c_n[0])
    assert dec_args["whh_split"].numel() == need
    custom_ops.pointer_decode([dec_args], x, T, K, precision="split")
    ops.check_status(dev)
    for bad in (torch.zeros(need - 16, dtype=torch.uint8, device=dev), torch.zeros(need + 16, dtype=torch.uint8, device=dev),
                torch.zeros(need // 4, dtype=torch.float32, device=dev), torch.zeros(need, dtype=torch.uint8)):
        for mod in (custom_ops, ops):
            with pytest.raises(RuntimeError, match="whh_split"):
                mod.lstm_encode([dict(enc_args, whh_split=bad)], precision="split")
            with pytest.raises(RuntimeError, match="whh_split"):
                mod.pointer_decode([dict(dec_args, whh_split=bad)], x, T, K, precision="split")
    ops.check_status(dev)


# ---- the ES-WOA search: eswoa_kernel, eswoa_wide_kernel, each through the ragged and the fixed entry points -------------------------------
@pytest.mark.parametrize("build,entry,sizes,per_size", [
    pytest.param("lanes", "ragged", (1, 3, 10, 33, 64, 7), 2, id="lanes-sizes0"),
    pytest.param("wide", "ragged", (5, 64, 65, 100, 2, 130), 2, id="wide-sizes1"),
    pytest.param("lanes", "fixed", (7,), 3, id="lanes-fixed"),
    pytest.param("wide", "fixed", (65,), 2, id="wide-fixed")])
def test_eswoa_ragged_build(dev, build, entry, sizes, per_size):
    """Problems of different sizes in one ragged launch (ops.eswoa_ragged), and problems of one size in one fixed launch
    (ops.eswoa: the same kernel with uniform counts), against oracle/woa.py run live on each of them: the same draws, the same
    float64 history bit for bit, the same final composition.  With at most 64 categories per problem the launch is the
    lane-per-category kernel; one problem beyond 64 makes it the workgroup-per-problem ("wide") kernel."""
    import copy
    from oracle import woa as owoa
    from test_gpu_refine import _pack
    from test_gpu_woa import _random_problems
    ops = _ops()
    assert (max(sizes) > 64) == (build == "wide")
    g = np.random.default_rng(sum(sizes) + 1)
    problems = []
    for T in sizes:
        problems += _random_problems(g, T, per_size)
    seeds = [77 + 3 * i for i in range(len(problems))]
    pop, iters = 10, 7
    prob_ptr, cand_ptr, flat, len0, start, bounds = _pack(problems)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev)      # noqa: E731
    tables = (t(cand_ptr, torch.int32), t(len0, torch.int32), t(flat, torch.float64).reshape(-1, 4), t(bounds, torch.float64),
              t(start, torch.int32), pop, iters, t(seeds, torch.int64))
    if entry == "ragged":
        fit, pos, hist, draws, rows = twice(lambda: ops.eswoa_ragged(t(prob_ptr, torch.int32), *tables))
        rows = rows.cpu().tolist()
    else:
        fit, pos, hist, draws = twice(lambda: ops.eswoa(*tables, sizes[0]))
    fit, pos, hist, draws = fit.cpu().tolist(), pos.cpu().tolist(), hist.cpu().tolist(), draws.cpu().tolist()
    for p, (services, cons, sol) in enumerate(problems):
        T = len(services)
        want = owoa.eswoa(services, cons, copy.deepcopy(sol), pop, iters, owoa.DrawStream(seeds[p]))
        assert draws[p] == want["draws"] and hist[p] == want["history"] and fit[p] == want["best_fitness"], p
        assert pos[p][:T] == [int(v) for v in want["best_pos"]], p
        if entry == "ragged":
            assert [tuple(r) for r in rows[p][:T]] == [tuple(r[:4]) for r in want["best_rows"]], p
    REC.note(f"eswoa_{entry}_{build}", exact_cases=len(problems))


def test_eswoa_refuses_a_problem_beyond_max_cand(dev):
    """The lane-per-category kernel copies a problem's candidate table into LDS sized for max_cand rows.  Through the C entry
    points (ops computes the exact maximum itself): 3 problems of 3 categories with 6, 9 and 6 candidates in a launch sized for
    6, once through gnnpn_eswoa_f64 and once through gnnpn_eswoa_ragged_f64.  Problem 1 is not searched (best_fitness NaN,
    draws -1, its best_pos and history rows untouched); problems 0 and 2 run as the oracle does."""
    import copy
    import ctypes
    import math
    from gnnpn_sc_amd import _lib
    from oracle import woa as owoa
    from test_gpu_refine import _pack
    T, pop, iters, max_cand, sentinel = 3, 4, 2, 6, -12345
    g = np.random.default_rng(6096)
    problems = []
    for p, per_cat in enumerate((2, 3, 2)):
        services = [[tuple(float(v) for v in np.r_[g.random(2), 1.0 - g.random(2) * 0.2 / T]) for _ in range(per_cat)] for _ in range(T)]
        sol = [list(cat[int(g.integers(0, per_cat))]) for cat in services] if p == 0 else None      # a seed among its own candidates
        problems.append((services, [[[0.5, 1.0]], [[0.5, 1.0]]], sol))
    seeds = [901, 902, 903]
    prob_ptr, cand_ptr, flat, len0, start, bounds = _pack(problems)
    assert prob_ptr == [0, 3, 6, 9] and [cand_ptr[3 * (p + 1)] - cand_ptr[3 * p] for p in range(3)] == [6, 9, 6]
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev)      # noqa: E731
    prob_ptr, cand_ptr, len0, start, seeds_d = (t(a, dt) for a, dt in ((prob_ptr, torch.int32), (cand_ptr, torch.int32),
                                                (len0, torch.int32), (start, torch.int32), (seeds, torch.int64)))
    flat, bounds = t(flat, torch.float64).reshape(-1, 4), t(bounds, torch.float64)
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())      # noqa: E731
    lib, stream = _lib.load(), _lib.stream_ptr()
    want = {p: owoa.eswoa(problems[p][0], problems[p][1], copy.deepcopy(problems[p][2]), pop, iters, owoa.DrawStream(seeds[p]))
            for p in (0, 2)}
    for entry in ("fixed", "ragged"):
        fit = torch.zeros(3, dtype=torch.float64, device=dev)
        pos = torch.full((3, T), sentinel, dtype=torch.int32, device=dev)
        hist = torch.full((3, iters), float(sentinel), dtype=torch.float64, device=dev)
        draws = torch.zeros(3, dtype=torch.int64, device=dev)
        if entry == "fixed":
            rc = lib.gnnpn_eswoa_f64(3, T, ptr(cand_ptr), ptr(len0), ptr(flat), ptr(bounds), ptr(start), pop, iters, ptr(seeds_d),
                                     max_cand, ptr(fit), ptr(pos), ptr(hist), ptr(draws), stream)
        else:
            rc = lib.gnnpn_eswoa_ragged_f64(3, ptr(prob_ptr), 9, T, max_cand, ptr(cand_ptr), ptr(len0), ptr(flat), ptr(bounds),
                                            ptr(start), pop, iters, ptr(seeds_d), 0, None, 0, ptr(fit), ptr(pos), None, ptr(hist),
                                            ptr(draws), stream)
        _lib.check(rc, f"eswoa ({entry})")
        fit, pos, hist, draws = fit.cpu().tolist(), pos.cpu().tolist(), hist.cpu().tolist(), draws.cpu().tolist()
        assert math.isnan(fit[1]) and draws[1] == -1, entry
        assert pos[1] == [sentinel] * T and hist[1] == [float(sentinel)] * iters, entry
        for p in (0, 2):
            assert draws[p] == want[p]["draws"] and hist[p] == want[p]["history"] and fit[p] == want[p]["best_fitness"], (entry, p)
            assert pos[p] == [int(v) for v in want[p]["best_pos"]], (entry, p)
