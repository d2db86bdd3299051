"""-m gpu: the LAYOUTS the C entry points of include/gnnpn_hip.h promise to accept or refuse — leading dimensions past the logical
width, bases that are not 16-byte aligned, NaN in every padding float — which the wrappers (ops.py, torch_ops.cpp: ld == width,
fresh 16-byte aligned tensors) never produce.  Every accepted layout is held to the CPU reference the entry's own test uses AND
must give the bits of the contiguous, aligned call; the output's padding must still hold NaN; every refused layout must return
its code, name the entry in gnnpn_last_error() and launch nothing.  Which build a layout selects is a host predicate on strides
and addresses: the cases restate it and check the kernel that was launched by its name (the profiler's kernel records).
Worst ratios go to the agreement records abi_layout_<kernel>.

Signed zeros: the ranking keys of csrc/select.hip order scores as a stable descending sort does, so -0.0 and +0.0 tie
(test_rank_rows_signed_zeros, test_select_candidates_signed_zeros).

Every reinterpret_cast to a 16-byte vector type on a CALLER's pointer in csrc/, with what guards it (host check) or covers it:
  graph.hip:56,100        csr_aggregate_kernel<true>, x / y          agg_rows_vec4 (graph_lds.h:17) at graph.hip:116 picks the scalar
                                                                      build instead: test_csr_aggregate_layouts
  graph.hip:153,157       lds_agg_fetch, col / w                     types declared packed, aligned(4): plain 16-byte global loads at
                                                                      4-byte alignment by design (row starts are arbitrary):
                                                                      test_csr_aggregate_blocks_layouts
  graph.hip:238,285       csr_aggregate_lds_kernel, x / y            agg_rows_vec4 at graph.hip:298 -> GNNPN_E_UNSUP:
                                                                      test_csr_aggregate_blocks_refusals
  graph_tiled.hip:330,503,569   tiled kernel, x / y                  agg_rows_vec4 at graph_tiled.hip:656 -> GNNPN_E_UNSUP:
                                                                      test_csr_aggregate_tiled_refusals
  graph_tiled.hip:268,269,418,450,451,469,470   the plan's stream    gnnpn_aligned(batches, 16) at graph_tiled.hip:633 and :656
  gin_aggregate.h:34      both GIN layers, x                         gin_layer.hip:162 (x 16-byte aligned, else GNNPN_E_UNSUP) and the
                                                                      kernel's own switch :98 (c_in % 4, ldx % 4); gin_layer_split.hip:445
                                                                      (host `vec`): test_gin_layer_layouts, test_gin_layer_split_layouts
  gin_layer_split.hip:46-48     packed weight records                gnnpn_aligned(w1 / w2 / w3, 16) at :447
  gin_layer_split.hip:143,156   col_inv, bias, scale, shift          gnnpn_aligned(..., 16) at :448-450
  gin_layer_split.hip:184       out                                  ldo % 4 and gnnpn_aligned(out, 16) at :447:
                                                                      test_gin_layer_split_refusals
  gin_layer_split.hip:404,405,410   the packer's image               gnnpn_aligned(packed, 16) at :425
  select_keys.h:76        emit_row (every select build), out_rows    GNNPN_REQUIRE at select.hip:122 (score_select.hip:255 for the
                                                                      fused launch): test_select_candidates_refusal
  decode.hip:295,296      attention_logits, enc_out / queries        H % 4, ld_q % 4 at decode.hip:337 and gnnpn_aligned at :341:
                                                                      test_attention_logits_refusals
  decode.hip:390          qos_reward_kernel, actions                 NO host check.  A plain 16-byte global load into registers (no
                                                                      LDS access, no vector store) at 4-byte alignment — the access of
                                                                      tile_load in dense.hip, which test_linear_build runs:
                                                                      test_qos_reward_misaligned_base
  lstm_coop.hip:310,383   cooperative encoder, enc_out (a STORE)     was unguarded: gnnpn_lstm_encode_f32 now requires enc_out 16-byte
                                                                      aligned (lstm.hip:105), as the decoders did: test_lstm_encode_refuses_
                                                                      a_misaligned_enc_out
  decode_glimpse.hip:39,41      W_ref(enc_out), V of 'Bahdanau'      no host check; plain 16-byte global loads (not on the fast path,
                                                                      outside this file's scope)
  lstm.hip:21, decode.hip:43,44, decode_glimpse.hip:75,76, decode_coop.hip:348,367, decode_shared.h:58, lstm_coop.hip:425,
  coop_common.h:501,658, request_branch.hip:55: whole weight images, enc_out and embedded of the recurrent kernels and the
  request branch — GNNPN_REQUIRE(gnnpn_aligned(..., 16)) at lstm.hip:104,112, decode_shared.h:45, decode.hip:176, lstm_coop.hip:435,
  request_branch.hip:258,261 (no leading dimensions: outside this file's scope).  The remaining casts are on LDS.
Padded strides already covered elsewhere: gnnpn_linear_f32 (test_gpu_kernel_builds.py::test_linear_build); in
test_gpu_train_kernels.py gnnpn_gemm_f32 (test_gemm_direct_split_and_padding), gnnpn_colsum_f32
(test_colsum_strided_like_the_start_input), gnnpn_embed_grad_f32 (test_embed_grad), gnnpn_precision_at_k (test_precision_at_k)
and gnnpn_attention_logits_f32 (test_attention_logits: ld_q = T * H through the wrapper)."""

import numpy as np
import pytest
import torch

from kernel_checks import Recorder, same_bits, twice
from oracle import ml as oml
from test_gpu_kernel_builds import _aggregate_reference, _block_graph, _offset_view, lds_build, select_build

pytestmark = pytest.mark.gpu
REC = Recorder("abi_layout")
F32, I32, U8, F64 = torch.float32, torch.int32, torch.uint8, torch.float64
NAN = float("nan")
E_ARG, E_UNSUP = -1, -2


def _lib():
    from gnnpn_sc_amd import _lib as L
    return L


def _ops():
    import gnnpn_sc_amd.ops as ops
    return ops


def _p(t, dtype=F32, none=False):
    return _lib().dev_ptr(t, dtype, "operand", none)


# ---- the shared operand ---------------------------------------------------------------------------------------------------------
def padded(t, ld, lead, dev):
    """The CPU tensor ``t`` [rows, width] as a device operand with leading dimension ``ld`` >= width whose first element lies
    ``lead`` (0..3) elements past a 16-byte boundary: a buffer of lead + rows * ld + 4 elements, all NaN (-7 for integers), the
    logical columns copied in.  -> (the [rows, ld] view, contiguous, so that dev_ptr takes it; ld)."""
    rows, width = t.shape
    assert ld >= width and 0 <= lead <= 3 and t.element_size() == 4
    flat = torch.full((lead + rows * ld + 4,), NAN if t.is_floating_point() else -7, dtype=t.dtype, device=dev)
    assert flat.data_ptr() % 16 == 0
    view = flat[lead:lead + rows * ld].view(rows, ld)
    view[:, :width] = t.to(dev)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * lead and view._base is flat
    return view, ld


def blank(rows, width, ld, lead, dev):
    """An output operand: ``padded`` with nothing but NaN in it."""
    return padded(torch.full((rows, width), NAN), ld, lead, dev)[0]


def logical(view, width):
    """The logical columns of an operand of ``padded`` (a CPU copy), after asserting that every other element of its buffer —
    the lead, the padding columns, the tail — still holds what ``padded`` put there: nothing wrote outside the logical part."""
    flat = view._base
    host = flat.cpu()
    lead = (view.data_ptr() - flat.data_ptr()) // 4
    rows, ld = view.shape
    outside = torch.ones(host.numel(), dtype=torch.bool)
    outside[lead:lead + rows * ld].view(rows, ld)[:, :width] = False
    fill = host[outside]
    assert bool(torch.isnan(fill).all() if host.is_floating_point() else (fill == -7).all()), "a kernel wrote into the padding"
    return host[lead:lead + rows * ld].view(rows, ld)[:, :width].contiguous()


def launched(fn, stem):
    """fn() -> (its result, the names of the kernels with ``stem`` in their name that it launched, in launch order: the profiler's
    device-side records)."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        r = fn()
        torch.cuda.synchronize()
    ev = sorted((e for e in prof.events() if e.device_type == DeviceType.CUDA), key=lambda e: e.time_range.start)
    return r, [e.name for e in ev if stem in e.name]


def is_build(name, stem, arg):
    """Whether a kernel record names build ``stem<arg>`` (demangled, or the Itanium spelling of a bool / int template argument)."""
    mangled = {"true": "ILb1E", "false": "ILb0E"}.get(arg, f"ILi{arg}E")
    return stem in name and (f"{stem}<{arg}>" in name or f"{stem}{mangled}" in name)


def refused(rc, code, entry, *outputs):
    """The return code, the entry's name in the thread's error text, and outputs that still hold their sentinel."""
    assert rc == code, (rc, _lib().load().gnnpn_last_error())
    assert entry in _lib().load().gnnpn_last_error().decode(), _lib().load().gnnpn_last_error()
    for out in outputs:
        host = (out._base if out._base is not None else out).cpu()
        assert bool(torch.isnan(host).all() if host.is_floating_point() else (host == -7).all()), f"{entry} wrote before refusing"


# ---- A1. gnnpn_csr_aggregate_f32: csr_aggregate_kernel<VEC4> -----------------------------------------------------------------------
def aggregate_build(x, ldx, y, ldy, C):
    """The build gnnpn_csr_aggregate_f32 launches (agg_rows_vec4, csrc/graph_lds.h), restated."""
    return "true" if C % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0 else "false"


GATHER_DEGREES = (0, 1, 3, 4, 5, 63, 64, 65, 130)   # nothing, the tail loop alone, groups of 4 + tail, one chunk of 64 -1 / +0 / +1, three chunks
# (ldx - C, ldy - C, lead of x, lead of y) -> VEC4 of the build for a C that is a multiple of 4
GATHER_LAYOUTS = [((0, 0, 0, 0), "true"), ((4, 8, 0, 0), "true"), ((1, 0, 0, 0), "false"), ((0, 2, 0, 0), "false"),
                  ((0, 0, 1, 0), "false"), ((0, 0, 0, 2), "false")]


def _gather_graph(n=70, seed=3):
    rng = np.random.default_rng(seed)
    deg = np.array([GATHER_DEGREES[i % len(GATHER_DEGREES)] for i in range(n)])
    rp = np.concatenate([[0], np.cumsum(deg)])
    col = rng.integers(0, n, rp[-1])
    w = rng.random(rp[-1], dtype=np.float32) + 0.05
    return torch.tensor(rp, dtype=I32), torch.from_numpy(col.astype(np.int32)), torch.from_numpy(w), n


@pytest.mark.parametrize("C", [8, 260, 6])
def test_csr_aggregate_layouts(dev, C):
    """The gather aggregate on 70 rows of 0 .. 130 edges, weighted and not, GIN self term and bias / BN / ReLU epilogue, against
    the oracle's edge-order fp32 sums bit for bit — at C = 8, 260 (a second 256-channel pass with 4 live channels) and 6, in
    six layouts: the vector build with padded rows, and the scalar build that a vector-width C gets for an odd ldx, an odd ldy,
    a misaligned x, a misaligned y."""
    lib, L = _lib().load(), _lib()
    rp, col, w, n = _gather_graph()
    g = torch.Generator().manual_seed(C)
    x = torch.randn(n, C, generator=g)
    eps = torch.tensor([0.125])
    bias, scale, shift = (torch.randn(C, generator=g) for _ in range(3))
    rpd, cold, wd = rp.to(dev), col.to(dev), w.to(dev)
    epi = [t.to(dev) for t in (eps, bias, scale, shift)]
    for weighted in (True, False):
        want = _aggregate_reference(rp, col, w if weighted else None, x, bias, scale, shift, relu=True, eps=eps)
        base = None
        for (dx, dy, lead_x, lead_y), vec4 in GATHER_LAYOUTS:
            xv, ldx = padded(x, C + dx, lead_x, dev)
            ldy = C + dy

            def run():
                y = blank(n, C, ldy, lead_y, dev)
                L.check(lib.gnnpn_csr_aggregate_f32(_p(rpd, I32), _p(cold, I32), _p(wd if weighted else None, F32, True), _p(xv), ldx,
                                                    *(_p(t) for t in epi), 1, _p(y), ldy, n, C, L.stream_ptr()), "gnnpn_csr_aggregate_f32")
                return y
            y, names = launched(lambda: twice(run), "csr_aggregate")
            build = aggregate_build(xv, ldx, y, ldy, C)
            assert build == (vec4 if C % 4 == 0 else "false"), (C, dx, dy, lead_x, lead_y)
            assert len(names) == 2 and all(is_build(k, "csr_aggregate_kernel", build) for k in names), (names, build)
            got = logical(y, C)
            assert torch.equal(got, want), f"csr_aggregate C={C} ldx={ldx} ldy={ldy} leads {lead_x},{lead_y} (VEC4 {build})"
            base = got if base is None else base
            assert same_bits(got, base), "the layout changed a bit"
    REC.note("csr_aggregate", exact_cases=2 * len(GATHER_LAYOUTS))


# ---- A2. gnnpn_csr_aggregate_blocks_f32 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 8, 4])
def test_csr_aggregate_blocks_layouts(dev, C):
    """The LDS-staged aggregate (4, 2, 1 lanes per row) on block-diagonal copies of a 40-row graph with a ragged last block, at
    (ldx, ldy) = (C + 4, C + 8), with and without the row order: the oracle's sums and the bits of the contiguous call."""
    lib, L, ops = _lib().load(), _lib(), _ops()
    S, weighted = 40, C != 8
    assert lds_build(S, C, weighted) == ({16: 4, 8: 2, 4: 1}[C], weighted)
    rp, col, w, n = _block_graph(S, 3, 3, 11 + C, weighted, ragged=True)
    assert n % S != 0
    g = torch.Generator().manual_seed(C)
    x, bias = torch.randn(n, C, generator=g), torch.randn(C, generator=g)
    eps = torch.tensor([0.3])
    want = _aggregate_reference(rp, col, w, x, bias, relu=True, eps=eps)
    rpd, cold, wd, bd, ed = rp.to(dev), col.to(dev), None if w is None else w.to(dev), bias.to(dev), eps.to(dev)
    order = ops.csr_block_row_order(rpd, S)
    base = None
    for ldx, ldy in ((C, C), (C + 4, C + 8)):
        xv, _ = padded(x, ldx, 0, dev)
        for row_order in (order, None):
            def run():
                y = blank(n, C, ldy, 0, dev)
                L.check(lib.gnnpn_csr_aggregate_blocks_f32(_p(rpd, I32), _p(cold, I32), _p(wd, F32, True), _p(xv), ldx, _p(ed), _p(bd), None,
                                                           None, 1, _p(y), ldy, n, C, S, _p(row_order, I32, True), L.stream_ptr()),
                        "gnnpn_csr_aggregate_blocks_f32")
                return y
            got = logical(twice(run), C)
            assert torch.equal(got, want), (C, ldx, ldy, row_order is not None)
            base = got if base is None else base
            assert same_bits(got, base)
    REC.note("csr_aggregate_lds", exact_cases=4)


def test_csr_aggregate_blocks_refusals(dev):
    """Rows that a lane cannot read or write 16 bytes at a time — ldx = C + 1, ldy = C + 2, x one float past a 16-byte boundary —
    are GNNPN_E_UNSUP for the LDS-staged form (the caller takes gnnpn_csr_aggregate_f32); nothing is launched."""
    lib, L = _lib().load(), _lib()
    S, C = 40, 16
    rp, col, w, n = _block_graph(S, 2, 3, 5, False)
    rpd, cold = rp.to(dev), col.to(dev)
    x = torch.randn(n, C, generator=torch.Generator().manual_seed(1))
    for dx, dy, lead_x in ((1, 0, 0), (0, 2, 0), (0, 0, 1)):
        xv, ldx = padded(x, C + dx, lead_x, dev)
        y = blank(n, C, C + dy, 0, dev)
        rc = lib.gnnpn_csr_aggregate_blocks_f32(_p(rpd, I32), _p(cold, I32), None, _p(xv), ldx, None, None, None, None, 0, _p(y), C + dy, n, C,
                                                S, None, L.stream_ptr())
        refused(rc, E_UNSUP, "csr_aggregate_blocks", y)


# ---- A3. gnnpn_csr_aggregate_tiled_f32 ----------------------------------------------------------------------------------------------
def _tiled_call(lib, L, plan, xv, ldx, epi, act, y, ldy, n, C, S):
    return lib.gnnpn_csr_aggregate_tiled_f32(_p(plan.header, I32), _p(plan.order, I32), _p(plan.selfw), _p(plan.batches, U8), _p(xv), ldx,
                                             *(_p(t, F32, True) for t in epi), act, _p(y), ldy, n, C, S, L.stream_ptr())


@pytest.mark.parametrize("S", [40, 256 + 7])
@pytest.mark.parametrize("C", [16, 32])
def test_csr_aggregate_tiled_layouts(dev, C, S):
    """The tiled aggregate called directly with a TilePlan's arrays, blocks of 40 rows (one pass) and of 263 (two), ragged last
    block, at (ldx, ldy) = (C + 4, C + 12) — the kernel narrows both to int inside a block: the oracle's sums and the bits of
    the contiguous call."""
    lib, L, ops = _lib().load(), _lib(), _ops()
    weighted = C == 16
    rp, col, w, n = _block_graph(S, 3, 3, S + C, weighted, ragged=True)
    g = torch.Generator().manual_seed(S + C)
    x = torch.randn(n, C, generator=g)
    eps = torch.tensor([0.125])
    bias, scale, shift = (torch.randn(C, generator=g) for _ in range(3))
    want = _aggregate_reference(rp, col, w, x, bias, scale, shift, relu=True, eps=eps)
    rpd, cold, wd = rp.to(dev), col.to(dev), None if w is None else w.to(dev)
    plan = ops.csr_tile_plan(rpd, cold, wd, S)
    assert plan.valid and plan.geom["passes"] == (1 if S == 40 else 2), plan.stats
    epi = [t.to(dev) for t in (eps, bias, scale, shift)]
    base = None
    for ldx, ldy in ((C, C), (C + 4, C + 12)):
        xv, _ = padded(x, ldx, 0, dev)

        def run():
            y = blank(n, C, ldy, 0, dev)
            L.check(_tiled_call(lib, L, plan, xv, ldx, epi, 1, y, ldy, n, C, S), "gnnpn_csr_aggregate_tiled_f32")
            return y
        got = logical(twice(run), C)
        assert torch.equal(got, want), (C, S, ldx, ldy)
        base = got if base is None else base
        assert same_bits(got, base)
    REC.note("csr_aggregate_tiled", exact_cases=2)


def test_csr_aggregate_tiled_refusals(dev):
    """GNNPN_E_UNSUP for rows that are not 16-byte pieces (ldx = C + 1, x one float past a boundary) and for C = 8 (no 16-channel
    slice); the bad-shape code where a block's rows would span 2^29 elements or more — the 32-bit offsets inside a block
    (csrc/graph_tiled.hip: the GNNPN_REQUIRE stands in front of the form's checks and of the launch, so the claimed ldx is never
    used as an address)."""
    lib, L, ops = _lib().load(), _lib(), _ops()
    S, C = 40, 16
    rp, col, w, n = _block_graph(S, 2, 3, 6, False)
    rpd, cold = rp.to(dev), col.to(dev)
    plan = ops.csr_tile_plan(rpd, cold, None, S)
    assert plan.valid
    x = torch.randn(n, C, generator=torch.Generator().manual_seed(2))
    none = (None, None, None, None)
    for c, dx, lead_x in ((C, 1, 0), (C, 0, 1), (8, 0, 0)):
        xv, ldx = padded(x[:, :c].contiguous(), c + dx, lead_x, dev)
        y = blank(n, c, c, 0, dev)
        refused(_tiled_call(lib, L, plan, xv, ldx, none, 0, y, c, n, c, S), E_UNSUP, "csr_aggregate_tiled", y)
    claimed = (-(-(1 << 29) // S) + 3) // 4 * 4                     # the smallest multiple of 4 with S * ldx >= 2^29
    assert S * claimed >= 1 << 29 > S * (claimed - 4)
    xv, _ = padded(x, C, 0, dev)
    y = blank(n, C, C, 0, dev)
    refused(_tiled_call(lib, L, plan, xv, claimed, none, 0, y, C, n, C, S), E_ARG, "csr_aggregate_tiled", y)
    refused(_tiled_call(lib, L, plan, xv, C, none, 0, y, claimed, n, C, S), E_ARG, "csr_aggregate_tiled", y)


# ---- A4. gnnpn_segment_mean_f32 -----------------------------------------------------------------------------------------------------
SEGMENTS = (0, 1, 7, 8, 9, 31, 32, 33, 41)        # both sides of the 8- and 32-row unrolls, an empty segment


@pytest.mark.parametrize("C", [1, 64, 65, 130])
def test_segment_mean_layouts(dev, C):
    """Segment means at (ldx, ldo) = (C + 3, C + 5), x one float past a 16-byte boundary, against a sequential fp32 chain over
    each segment's rows (the order of scatter_add) divided by the count; the bits of the contiguous call."""
    lib, L = _lib().load(), _lib()
    n = sum(SEGMENTS)
    x = torch.randn(n, C, generator=torch.Generator().manual_seed(C))
    want = torch.zeros(len(SEGMENTS), C)
    r = 0
    for s, size in enumerate(SEGMENTS):
        acc = torch.zeros(C)
        for _ in range(size):
            acc = acc + x[r]
            r += 1
        want[s] = acc / float(max(size, 1))
    batch = torch.repeat_interleave(torch.arange(len(SEGMENTS)), torch.tensor(SEGMENTS))
    assert torch.equal(want, oml.scatter_mean(x, batch, len(SEGMENTS)))                     # the oracle's restatement of the same chain
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(SEGMENTS)]), dtype=I32).to(dev)
    base = None
    for ldx, ldo, lead in ((C, C, 0), (C + 3, C + 5, 1)):
        xv, _ = padded(x, ldx, lead, dev)

        def run():
            out = blank(len(SEGMENTS), C, ldo, 0, dev)
            L.check(lib.gnnpn_segment_mean_f32(_p(ptr, I32), _p(xv), ldx, _p(out), ldo, len(SEGMENTS), C, L.stream_ptr()), "gnnpn_segment_mean_f32")
            return out
        got = logical(twice(run), C)
        assert torch.equal(got, want), (C, ldx, ldo)
        base = got if base is None else base
        assert same_bits(got, base)
    REC.note("segment_mean", exact_cases=2)


# ---- A5 / A6. the one-launch GIN layers ----------------------------------------------------------------------------------------------
def _chain_graph(n, nodes_per_graph, g):
    """Chains of ``nodes_per_graph`` nodes (both directions) and n // 3 long-range edges -> edge_index."""
    i = torch.arange(n - 1)
    keep = (i + 1) % nodes_per_graph != 0
    src = torch.stack([i[keep], i[keep] + 1], 1).reshape(-1)
    dst = torch.stack([i[keep] + 1, i[keep]], 1).reshape(-1)
    return torch.cat([torch.stack([src, dst]), torch.randint(0, n, (2, n // 3), generator=g)], 1)


def _gin_weights(g, c_in):
    mk = lambda *s: torch.randn(*s, generator=g) / s[-1] ** 0.5   # noqa: E731
    p = {"w1": mk(256, c_in), "b1": mk(256), "w2": mk(128, 256), "b2": mk(128), "w3": mk(128, 128), "b3": mk(128)}
    p.update(a1=torch.rand(256, generator=g) + 0.5, s1=mk(256), a2=torch.rand(128, generator=g) + 0.5, s2=mk(128))
    return p


def _gin_reference(agg, p, with_lin, cast):
    """The layer behind the fp32 aggregate in ``cast`` arithmetic, intermediates rounded to fp32 where the kernels hold them in
    fp32 (tests/test_gpu_kernel_builds.py::test_gin_layer_build, tests/test_gpu_ops.py::test_gin_layer_split_against_fp64)."""
    c = lambda t: t.to(cast)   # noqa: E731
    t = torch.relu((c(agg) @ c(p["w1"]).t() + c(p["b1"])) * c(p["a1"]) + c(p["s1"])).float().to(cast)
    r = torch.relu((t @ c(p["w2"]).t() + c(p["b2"])) * c(p["a2"]) + c(p["s2"]))
    if with_lin:
        r = r.float().to(cast) @ c(p["w3"]).t() + c(p["b3"])
    return r


@pytest.mark.parametrize("with_lin", [False, True])
def test_gin_layer_layouts(dev, with_lin):
    """gnnpn_gin_layer_f32, both builds, on 2 * 32 + 5 rows: c_in = 8 at ldx = 8, 12 (the kernel's vector aggregate) and ldx = 9
    (its scalar one for a vector-width c_in), c_in = 26 at ldx = 26, 29; ldo = 132.  Against the float64 layer from the oracle's
    ordered fp32 aggregate under the fp32 yardstick (factor 4, floor 2e-6: the bound of test_gin_layer_build); the layouts of one
    c_in give the same bits, which are those of gnnpn_csr_aggregate_f32 + gnnpn_linear_f32 in sequence (the header's promise)."""
    from gnnpn_sc_amd import graph
    lib, L, ops = _lib().load(), _lib(), _ops()
    n, width = 2 * 32 + 5, 128
    for c_in, ldxs in ((8, (8, 12, 9)), (26, (26, 29))):
        g = torch.Generator().manual_seed(n + c_in)
        ei = _chain_graph(n, 7, g)
        x = torch.randn(n, c_in, generator=g)
        eps = torch.tensor([0.07])
        p = _gin_weights(g, c_in)
        agg = oml.scatter_sum(x[ei[0]], ei[1], n) + (1 + eps) * x
        ref64, ref32 = _gin_reference(agg, p, with_lin, torch.double), _gin_reference(agg, p, with_lin, torch.float)
        csr = graph.csr_by_destination(ei, n).to(dev)
        d = {k: v.to(dev) for k, v in p.items()}
        q1, q2, q3 = (ops.pack_mfma_b32(d[k]) for k in ("w1", "w2", "w3"))
        ed = eps.to(dev)
        base = None
        for ldx in ldxs:
            xv, _ = padded(x, ldx, 0, dev)

            def run():
                out = blank(n, width, width + 4, 0, dev)
                L.check(lib.gnnpn_gin_layer_f32(_p(csr.rowptr, I32), _p(csr.col, I32), _p(xv), ldx, c_in, _p(ed), _p(q1), _p(d["b1"]), _p(d["a1"]),
                                                _p(d["s1"]), 256, _p(q2), _p(d["b2"]), _p(d["a2"]), _p(d["s2"]), 128,
                                                _p(q3 if with_lin else None, F32, True), _p(d["b3"] if with_lin else None, F32, True),
                                                128 if with_lin else 0, _p(out), width + 4, n, L.stream_ptr()), "gnnpn_gin_layer_f32")
                return out
            got = logical(twice(run), width)
            REC.yardstick("gin_layer_f32", f"out_{'lin' if with_lin else 'plain'}", got, ref64, ref32)
            base = got if base is None else base
            assert same_bits(got, base), f"gin_layer c_in={c_in}: ldx={ldx} changed a bit"
        xd = x.to(dev)
        t = ops.linear(ops.csr_aggregate(csr.rowptr, csr.col, None, xd, self_coef=ed), d["w1"], d["b1"], d["a1"], d["s1"], ops.ACT_RELU)
        sep = ops.linear(t, d["w2"], d["b2"], d["a2"], d["s2"], ops.ACT_RELU)
        sep = ops.linear(sep, d["w3"], d["b3"]) if with_lin else sep
        assert same_bits(base, sep.cpu()), "gin_layer is not csr_aggregate + linear bit for bit"


def test_gin_layer_refusals(dev):
    """gnnpn_gin_layer_f32: x one float past a 16-byte boundary and an ldo below the output width are GNNPN_E_UNSUP."""
    from gnnpn_sc_amd import graph
    lib, L, ops = _lib().load(), _lib(), _ops()
    n, c_in = 37, 8
    g = torch.Generator().manual_seed(9)
    csr = graph.csr_by_destination(_chain_graph(n, 7, g), n).to(dev)
    x = torch.randn(n, c_in, generator=g)
    d = {k: v.to(dev) for k, v in _gin_weights(g, c_in).items()}
    q1, q2 = ops.pack_mfma_b32(d["w1"]), ops.pack_mfma_b32(d["w2"])
    ed = torch.tensor([0.07], device=dev)
    for lead, ldo in ((1, 128), (0, 127)):
        xv, _ = padded(x, c_in, lead, dev)
        out = blank(n, 128, 128, 0, dev)                              # (sized for ldo = 128: a launch with 127 would stay inside it)
        rc = lib.gnnpn_gin_layer_f32(_p(csr.rowptr, I32), _p(csr.col, I32), _p(xv), c_in, c_in, _p(ed), _p(q1), _p(d["b1"]), _p(d["a1"]),
                                     _p(d["s1"]), 256, _p(q2), _p(d["b2"]), _p(d["a2"]), _p(d["s2"]), 128, None, None, 0, _p(out), ldo, n,
                                     L.stream_ptr())
        refused(rc, E_UNSUP, "gin_layer", out)


def _split_call(lib, L, csr, xv, ldx, c_in, ed, d, pk, with_lin, out, ldo, n):
    (w1, i1), (w2, i2), (w3, i3) = pk
    return lib.gnnpn_gin_layer_split(
        _p(csr.rowptr, I32), _p(csr.col, I32), _p(xv), ldx, c_in, _p(ed), _p(w1, U8), _p(i1), _p(d["b1"]), _p(d["a1"]), _p(d["s1"]), 256,
        _p(w2, U8), _p(i2), _p(d["b2"]), _p(d["a2"]), _p(d["s2"]), 128, _p(w3 if with_lin else None, U8, True),
        _p(i3 if with_lin else None, F32, True), _p(d["b3"] if with_lin else None, F32, True), 128 if with_lin else 0, _p(out), ldo, n,
        L.stream_ptr())


@pytest.mark.parametrize("with_lin", [False, True])
def test_gin_layer_split_layouts(dev, with_lin):
    """gnnpn_gin_layer_split, both builds, on 2 * 48 + 5 rows: c_in = 8 at ldx = 8, 12 (vector aggregate) and 9 (the scalar one,
    c_in <= 32), c_in = 32 at ldx = 32 and 33; ldo = 132.  Held to the bound of test_gin_layer_split_against_fp64 — per-row
    scaled error against the float64 layer at most 1.25 x the fp32 layer's (+ 1e-7 on the maximum, + 1e-9 on the mean) and below
    5e-6 — and the layouts of one c_in give the same bits."""
    from gnnpn_sc_amd import graph
    lib, L, ops = _lib().load(), _lib(), _ops()
    n, width = 2 * 48 + 5, 128
    for c_in, ldxs in ((8, (8, 12, 9)), (32, (32, 33))):
        g = torch.Generator().manual_seed(n + c_in)
        ei = _chain_graph(n, 7, g)
        x = torch.randn(n, c_in, generator=g) * torch.exp(2 * torch.randn(n, 1, generator=g))      # rows of very different magnitude
        x[5] = 0.0
        eps = torch.tensor([0.07])
        p = _gin_weights(g, c_in)
        agg = oml.scatter_sum(x[ei[0]], ei[1], n) + (1 + eps) * x
        ref = _gin_reference(agg, p, with_lin, torch.double)
        csr = graph.csr_by_destination(ei, n).to(dev)
        d = {k: v.to(dev) for k, v in p.items()}
        ed = eps.to(dev)
        pk = [ops.pack_split_weights(d[k]) for k in ("w1", "w2", "w3")]
        f32 = ops.gin_layer(csr.rowptr, csr.col, x.to(dev), ed, ops.pack_mfma_b32(d["w1"]), d["b1"], d["a1"], d["s1"], ops.pack_mfma_b32(d["w2"]),
                            d["b2"], d["a2"], d["s2"], ops.pack_mfma_b32(d["w3"]) if with_lin else None, d["b3"] if with_lin else None).cpu()
        scale = ref.abs().amax(1, keepdim=True).clamp_min(1e-30)
        e_f32 = (f32.double() - ref).abs() / scale
        base = None
        for ldx in ldxs:
            xv, _ = padded(x, ldx, 0, dev)

            def run():
                out = blank(n, width, width + 4, 0, dev)
                L.check(_split_call(lib, L, csr, xv, ldx, c_in, ed, d, pk, with_lin, out, width + 4, n), "gnnpn_gin_layer_split")
                return out
            got = logical(twice(run), width)
            e_split = (got.double() - ref).abs() / scale
            b_max, b_mean = 1.25 * e_f32.max().item() + 1e-7, 1.25 * e_f32.mean().item() + 1e-9
            REC.note("gin_layer_split", max_err_over_bound=e_split.max().item() / b_max, mean_err_over_bound=e_split.mean().item() / b_mean,
                     max_rel_err_vs_fp64=e_split.max().item())
            assert torch.isfinite(got).all()
            assert e_split.max().item() <= b_max and e_split.mean().item() <= b_mean, (c_in, ldx, e_split.max().item(), e_f32.max().item())
            assert e_split.max().item() < 5e-6
            base = got if base is None else base
            assert same_bits(got, base), f"gin_layer_split c_in={c_in}: ldx={ldx} changed a bit"


def test_gin_layer_split_refusals(dev):
    """gnnpn_gin_layer_split: more than 32 channels in rows that are not 16-byte pieces (c_in = 36 at ldx = 37), output rows that
    are not (ldo = 130, out one float past a boundary) are GNNPN_E_UNSUP."""
    from gnnpn_sc_amd import graph
    lib, L, ops = _lib().load(), _lib(), _ops()
    n = 37
    g = torch.Generator().manual_seed(10)
    csr = graph.csr_by_destination(_chain_graph(n, 7, g), n).to(dev)
    ed = torch.tensor([0.07], device=dev)
    for c_in, ldx, ldo, lead_out in ((36, 37, 128, 0), (8, 8, 130, 0), (8, 8, 128, 1)):
        x = torch.randn(n, c_in, generator=g)
        d = {k: v.to(dev) for k, v in _gin_weights(g, c_in).items()}
        pk = [ops.pack_split_weights(d[k]) for k in ("w1", "w2", "w3")]
        xv, _ = padded(x, ldx, 0, dev)
        out = blank(n, 128, ldo, lead_out, dev)
        refused(_split_call(lib, L, csr, xv, ldx, c_in, ed, d, pk, False, out, ldo, n), E_UNSUP, "gin_layer_split", out)


# ---- A7. gnnpn_pack_split_weights_f16 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(256, 26), (128, 256), (16, 1)])
def test_pack_split_weights_layout(dev, N, K):
    """The packer at ldw = K + 3 (NaN behind every row): image and col_inv byte for byte those of the contiguous call, and the
    pieces sum to the weights bit for bit (the reference of test_gin_layer_split_against_fp64)."""
    from test_gpu_ops import _unpack_split_weights
    lib, L, ops = _lib().load(), _lib(), _ops()
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(N + K)) / K ** 0.5
    want_pk, want_inv = ops.pack_split_weights(w.to(dev))
    wv, ldw = padded(w, K + 3, 0, dev)

    def run():
        pk = torch.zeros_like(want_pk)
        inv = torch.full_like(want_inv, NAN)
        L.check(lib.gnnpn_pack_split_weights_f16(_p(wv), ldw, N, K, _p(pk, U8), _p(inv), L.stream_ptr()), "gnnpn_pack_split_weights_f16")
        return pk, inv
    pk, inv = twice(run)
    assert torch.equal(pk, want_pk) and same_bits(inv, want_inv)
    assert np.array_equal(_unpack_split_weights(pk, inv, N, K), w.double().numpy())
    REC.note("pack_split_weights", exact_cases=1)


# ---- A8. gnnpn_select_candidates ---------------------------------------------------------------------------------------------------------
SELECT_KERNEL = {"16<8>": ("select_candidates16_kernel", "8"), "16<16>": ("select_candidates16_kernel", "16"), "wave": ("select_candidates_kernel", None)}


def _select_problem(T, S, B, seed, lo_range=(0.93, 0.99)):
    import gnnpn_sc_amd.synth as synth
    table = synth.make_service_table(T, S, seed=seed, degree=4)
    pb = synth.make_problem_batch(table, B, seed=seed + 10, tasks_per_problem=max(1, T - 2), lo_range=lo_range)
    return table, pb


def _select_device(table, pb, dev):
    return [torch.from_numpy(a).to(dev) for a in (table.cat_ptr, table.qos, pb.local_bounds, pb.present, pb.global_bounds)]


def _select_abi(dev, scores, ld, dv, T, K):
    """gnnpn_select_candidates on a score matrix of leading dimension ``ld`` with NaN behind every row -> rows, ids."""
    lib, L = _lib().load(), _lib()
    B = scores.shape[0]
    sv, _ = padded(scores, ld, 0, dev)
    rows = torch.full((B, T * K, 8), NAN, device=dev)
    ids = torch.full((B, T * K), -7, dtype=I32, device=dev)
    L.check(lib.gnnpn_select_candidates(_p(sv), ld, _p(dv[0], I32), _p(dv[1], F64), _p(dv[2], F64), _p(dv[3], U8), _p(dv[4], F64), _p(rows), _p(ids, I32),
                                        B, T, K, L.stream_ptr()), "gnnpn_select_candidates")
    return rows, ids


@pytest.mark.parametrize("T,S,K,lds", [(12, 60, 5, (60, 97)), (6, 180, 20, (180, 185))])
def test_select_candidates_layouts(dev, T, S, K, lds):
    """The candidate reduction on a padded score matrix with NaN in the padding (a NaN that was read would outrank every score):
    the rows of oracle.data.reduce_candidates, many exact ties.  The launcher reads the number of services off the stride:
    (12, 60, 5) is the 8-lane build at ld_scores = 60 and the 16-lane build at 97 > 8 T — asserted on the launched kernel."""
    from parity import oracle_candidate_rows
    B = 5
    table, pb = _select_problem(T, S, B, 20 + K)
    scores = torch.randint(0, 24, (B, S), generator=torch.Generator().manual_seed(S + K)).float() / 24
    assert int((np.diff(np.sort(scores.numpy(), 1), axis=1) == 0).sum()) > B * S // 2
    want = oracle_candidate_rows(pb, table, oml.rank_services(scores).numpy(), K, pb.x.shape[0] // B)
    dv = _select_device(table, pb, dev)
    base, builds = None, []
    for ld in lds:
        (rows, ids), names = launched(lambda: twice(lambda: _select_abi(dev, scores, ld, dv, T, K)), "select_candidates")
        build = select_build(K, ld, T)
        stem, arg = SELECT_KERNEL[build]
        assert len(names) == 2 and all(is_build(k, stem, arg) if arg else (stem in k) for k in names), (names, build)
        builds.append(build)
        assert torch.equal(rows.cpu().view(want.shape), want), (T, S, K, ld)
        base = (rows.cpu(), ids.cpu()) if base is None else base
        assert same_bits(rows.cpu(), base[0]) and torch.equal(ids.cpu(), base[1])
    assert builds == (["16<8>", "16<16>"] if K == 5 else ["wave", "wave"])
    REC.note("select_candidates", exact_cases=len(lds))


def test_select_candidates_refusal(dev):
    """out_rows one float past a 16-byte boundary is refused (GNNPN_E_ARG: the rows leave as 16-byte stores)."""
    lib, L = _lib().load(), _lib()
    T, S, K, B = 6, 30, 3, 4
    table, pb = _select_problem(T, S, B, 3)
    dv = _select_device(table, pb, dev)
    scores = torch.rand(B, S, generator=torch.Generator().manual_seed(1)).to(dev)
    rows = blank(B, T * K * 8, T * K * 8, 1, dev)
    ids = torch.full((B, T * K), -7, dtype=I32, device=dev)
    rc = lib.gnnpn_select_candidates(_p(scores), S, _p(dv[0], I32), _p(dv[1], F64), _p(dv[2], F64), _p(dv[3], U8), _p(dv[4], F64), _p(rows), _p(ids, I32),
                                     B, T, K, L.stream_ptr())
    refused(rc, E_ARG, "select_candidates", rows, ids)


# ---- A9. gnnpn_rank_rows ----------------------------------------------------------------------------------------------------------------
def _rank_abi(dev, scores, ld):
    lib, L = _lib().load(), _lib()
    B, S = scores.shape
    sv, _ = padded(scores, ld, 0, dev)
    ranking = torch.full((B, S), -7, dtype=I32, device=dev)
    L.check(lib.gnnpn_rank_rows(_p(sv), ld, _p(ranking, I32), B, S, L.stream_ptr()), "gnnpn_rank_rows")
    return ranking


@pytest.mark.parametrize("S", [40, 16385])
def test_rank_rows_layout(dev, S):
    """The ranking (S = 16385: the kernel that sorts ids and forms keys from the row) at ld_scores = S + 3 with NaN in the padding,
    exact ties: oml.rank_services."""
    B = 2
    scores = torch.rand(B, S, generator=torch.Generator().manual_seed(S))
    scores[:, : S // 4] = scores[:, S // 2: S // 2 + S // 4]
    want = oml.rank_services(scores)
    base = None
    for ld in (S, S + 3):
        got = twice(lambda: _rank_abi(dev, scores, ld)).cpu().long()
        assert torch.equal(got, want), (S, ld)
        base = got if base is None else base
        assert torch.equal(got, base)
    REC.note("rank_rows", exact_cases=2)


# ---- A10. gnnpn_woa_candidates_count / _fill ---------------------------------------------------------------------------------------------
def test_woa_candidates_x_ld(dev, tmp_path, monkeypatch):
    """The ES-WOA tables of test_candidates_equal_host_on_the_driver_fixture's problems with the node rows in a [N, 9] buffer
    (x_ld = 9, NaN in the two extra columns): every table identical to the x_ld = 7 call, and equal to the host path's."""
    from test_gpu_refine import _assert_tables_equal, _device_batch, _host_tables, _woa_driver
    ops = _ops()
    fx, ds, actions, n_train = _woa_driver(tmp_path, monkeypatch)
    host, _sols, _mins = _host_tables("QWS", actions, 0)
    svc, batch = _device_batch(ds, n_train, dev)
    a = torch.from_numpy(actions).to(dev)
    assert batch.x.shape[1] == 7
    x9 = torch.full((batch.x.shape[0], 9), NAN, device=dev)
    x9[:, :7] = batch.x
    call = lambda x: ops.woa_candidates(svc.cat_ptr, svc.qos, x, batch.seg_ptr, batch.local_bounds, batch.global_bounds, a, check_status=False)   # noqa: E731
    t7, t9 = twice(lambda: call(batch.x)), twice(lambda: call(x9))
    assert sorted(t7) == sorted(t9)
    for k in t7:
        assert same_bits(t7[k], t9[k]) if isinstance(t7[k], torch.Tensor) else t7[k] == t9[k], k
    _assert_tables_equal(t9, host)


# ---- A11. gnnpn_qos_reward_f32 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 64, 65])
def test_qos_reward_misaligned_base(dev, T):
    """The reward of a contiguous actions tensor that starts 1, 2, 3 floats past a 16-byte boundary — what the wrappers let
    through (dev_ptr asks for contiguity only); the kernel reads the rows with plain 16-byte global loads — against the
    oracle's reward as in test_qos_reward_batches_of_64_rows: Low exact, High to 1.0001e-5."""
    from oracle import pn as opn
    ops = _ops()
    B = 9
    g = torch.Generator().manual_seed(T)
    act = torch.rand(B, T, 8, generator=g)
    act[:, :, 2:4] = 1.0 - act[:, :, 2:4] * (2.0 / max(T, 2))
    act[:, :, 4:] = 0.0
    act[:, 0, 4:8] = torch.tensor([0.2, 0.9, 0.2, 0.9])
    act[1, :, 0:4] = torch.tensor([0.0, 1.0, 1.0, 1.0])
    act[1, T // 2, 0] = 0.4
    rows = [act[:, t] for t in range(T)]
    want_low, want_high = opn.reward(rows, "Low"), opn.reward(rows, "High")
    base = [ops.qos_reward(act.to(dev), level).cpu() for level in ("Low", "High")]
    for lead in (1, 2, 3):
        av = _offset_view(act, dev, lead)
        low, high = (twice(lambda: ops.qos_reward(av, level)).cpu() for level in ("Low", "High"))
        assert torch.equal(low, want_low), (T, lead)
        assert float((high - want_high).abs().max()) <= 1.0001e-5, (T, lead)
        assert same_bits(low, base[0]) and same_bits(high, base[1])
    REC.note("qos_reward", exact_cases=3)


# ---- B. the remaining refusals -----------------------------------------------------------------------------------------------------------
def test_attention_logits_refusals(dev):
    """gnnpn_attention_logits_f32 reads enc_out and the queries 16 bytes at a time: ld_q = H + 2 and queries one float past a
    16-byte boundary are refused (GNNPN_E_ARG)."""
    lib, L = _lib().load(), _lib()
    B, Lp, H = 3, 5, 32
    g = torch.Generator().manual_seed(4)
    enc = torch.randn(B, Lp, H, generator=g).to(dev)
    q = torch.randn(B, H, generator=g)
    for ld_q, lead in ((H + 2, 0), (H, 1)):
        qv, _ = padded(q, ld_q, lead, dev)
        logits = blank(B, Lp, Lp, 0, dev)
        rc = lib.gnnpn_attention_logits_f32(_p(enc), _p(qv), ld_q, None, 10.0, 1, _p(logits), B, Lp, H, 0, 0, L.stream_ptr())
        refused(rc, E_ARG, "attention_logits", logits)


def test_lstm_encode_refuses_a_misaligned_enc_out(dev):
    """The cooperative encoder stores enc_out 16 bytes at a time (and the decoders require it 16-byte aligned): an enc_out one
    float past a boundary is GNNPN_E_ARG before anything is launched, whichever form the call would take."""
    lib, L = _lib().load(), _lib()
    B, Lp, H = 2, 3, 256
    pre = torch.zeros(B, Lp, 4 * H, device=dev)
    whh, bhh = torch.zeros(H // 4, 4, H, 4, device=dev), torch.zeros(4 * H, device=dev)
    enc = blank(B, Lp * H, Lp * H, 1, dev)
    h_n, c_n = blank(B, H, H, 0, dev), blank(B, H, H, 0, dev)
    nets = (L.EncodeNet * 1)()
    for field, t in (("pregates", pre), ("whh_packed", whh), ("bhh", bhh), ("enc_out", enc), ("h_n", h_n), ("c_n", c_n)):
        setattr(nets[0], field, _p(t).value)
    rc = lib.gnnpn_lstm_encode_f32(1, nets, B, Lp, H, 8, 0, None, None, 0, L.stream_ptr())
    refused(rc, E_ARG, "lstm_encode", enc, h_n, c_n)


# ---- C. signed zeros in the ranking keys ---------------------------------------------------------------------------------------------------
def _zero_mix(shape, seed):
    """Scores drawn from {-0.0, +0.0, 0.25, 0.5, 1.0}: both zeros in every row, many ties."""
    values = torch.tensor([-0.0, 0.0, 0.25, 0.5, 1.0])
    s = values[torch.randint(0, 5, shape, generator=torch.Generator().manual_seed(seed))]
    assert bool(((s == 0) & torch.signbit(s)).any(1).all()) and bool(((s == 0) & ~torch.signbit(s)).any(1).all())
    return s


def test_signed_zero_order_of_the_oracle():
    """What the kernels are held to: the stable descending sort treats -0.0 and +0.0 as equal (ties: lowest index first)."""
    row = torch.tensor([[0.5, -0.0, 0.0, -0.0, 0.0, 0.25]])
    assert oml.rank_services(row).tolist() == [[0, 5, 1, 2, 3, 4]]


@pytest.mark.parametrize("S", [40, 16385])
def test_rank_rows_signed_zeros(dev, S):
    """gnnpn_rank_rows on scores that mix +0.0, -0.0 and tied positive values, both kernels: oml.rank_services (a key that puts
    -0.0 below +0.0 ranks every +0.0 in front of the -0.0 of lower index)."""
    ops = _ops()
    row = torch.tensor([[0.5, -0.0, 0.0, -0.0, 0.0, 0.25]])
    if S == 40:
        assert twice(lambda: ops.rank_rows(row.to(dev))).cpu().tolist() == [[0, 5, 1, 2, 3, 4]]
    scores = _zero_mix((2, S), S)
    got = twice(lambda: ops.rank_rows(scores.to(dev))).cpu().long()
    assert torch.equal(got, oml.rank_services(scores))


@pytest.mark.parametrize("build,T,S,K", [("16<8>", 12, 60, 5), ("16<16>", 6, 120, 12), ("wave", 6, 180, 20)])
def test_select_candidates_signed_zeros(dev, build, T, S, K):
    """The three launches of gnnpn_select_candidates on the same kind of scores: the rows of oracle.data.reduce_candidates under
    the oracle's ranking."""
    from parity import oracle_candidate_rows
    ops = _ops()
    assert select_build(K, S, T) == build
    B = 5
    table, pb = _select_problem(T, S, B, 40 + K, lo_range=(0.85, 0.96))
    scores = _zero_mix((B, S), S + K)
    want = oracle_candidate_rows(pb, table, oml.rank_services(scores).numpy(), K, pb.x.shape[0] // B)
    below = torch.where((scores == 0) & torch.signbit(scores), torch.full_like(scores, -1e-30), scores)       # -0.0 ranked below +0.0
    assert not torch.equal(want, oracle_candidate_rows(pb, table, oml.rank_services(below).numpy(), K, pb.x.shape[0] // B)), \
        "the case does not tell the two orders apart"
    dv = _select_device(table, pb, dev)
    rows, ids = twice(lambda: ops.select_candidates(scores.to(dev), *dv, K))
    assert torch.equal(rows.cpu().view(want.shape), want), build
