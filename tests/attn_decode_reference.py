"""Helper of the general attention decoder's tests (not a test file): modelPN.py:204-239 for ONE pointer net restated in plain
torch, forward only, in a given dtype — the forward half of test_gpu_train_kernels.py::_decode_ref.  Per step: the decoder LSTM
cell; the glimpse rounds over all L positions with -inf at the positions chosen before the step; the window logits (C*tanh, then
+ latent, then softmax).  For 'Bahdanau' ``ref = W_ref(enc_out) + b_ref`` is taken as given.  Driven along a GIVEN ``idx`` (the
kernel's own path replayed), or free-running: ``idx`` is then the first maximum of its own ``z``, or, with a sample seed, the draw
rule of the decoders on its own probabilities.

Also here, so that the GPU test (test_gpu_pn.py) and the no-GPU test of its preconditions (test_attn_decode_host.py) use the same
ones: the seeded inputs, the cases, the allowance ``eps`` a case's logits get, and the decision rules."""
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import pn as opn
from parity import TAU_DRAW

D, F32 = torch.float64, torch.float32

Case = namedtuple("Case", "id H B T K bah G use_tanh C latent sample_seed seed")

# NT (threads of a workgroup) is 64 at H = 32 and 256 at H = 256; one wavefront per position in the logits, NT / 64 of them
CASES = [
    Case("h32_dot_g1_one_position", 32, 3, 1, 1, False, 1, 1, 10.0, False, None, 1),       # L = 1: one position, empty strides
    Case("h32_dot_g2_T70_forced", 32, 2, 70, 1, False, 2, 1, 10.0, True, None, 2),         # T > NT = 64: second stride of the mask loop
    Case("h32_bah_g1_K64", 32, 2, 3, 64, True, 1, 1, 5.0, False, None, 3),                 # the whole of win[64]
    Case("h32_bah_g3_K17_no_tanh", 32, 3, 5, 17, True, 3, 0, 1.0, True, None, 4),          # three rounds, no tanh, odd window
    Case("h32_bah_g0_L63", 32, 3, 9, 7, True, 0, 1, 10.0, True, None, 5),                  # L = 63, one short of a wave; no glimpse
    Case("h256_dot_g1_T258_forced", 256, 2, 258, 1, False, 1, 1, 10.0, True, None, 6),     # T > NT = 256
    Case("h256_dot_g2_L3", 256, 3, 1, 3, False, 2, 1, 10.0, False, None, 207),             # L = 3 < 4 waves
    Case("h256_dot_g8_L259", 256, 2, 7, 37, False, 8, 1, 2.5, True, None, 8),              # L = 259, just past NT; eight rounds
    Case("h256_bah_g1_K64", 256, 2, 3, 64, True, 1, 1, 10.0, False, None, 9),              # full window, wide H
    Case("h256_bah_g2_K16_no_tanh", 256, 3, 4, 16, True, 2, 0, 1.0, True, None, 10),
    Case("h32_bah_g2_sampled", 32, 3, 13, 5, True, 2, 1, 10.0, True, 7, 911),              # net.sample through this kernel
    Case("h256_dot_g1_sampled", 256, 3, 6, 10, False, 1, 1, 10.0, True, 11, 112),
    Case("h32_dot_g1_B300", 32, 300, 4, 3, False, 1, 1, 10.0, True, None, 13),             # many workgroups, b*L*H offsets
]

# the dynamic-LDS limit of the launch: (L + T) * 4 bytes <= 120 KB.  T = 480, n_per = 63 is 30 720 words, exactly 120 KB, the most the
# launch takes; T = 480, n_per = 64 is refused.  The accepted shape that is RUN is smaller (see test_attention_decode_lds_limit for the
# measured time of the exact edge): T = 257, n_per = 63, the fewest steps whose dynamic LDS is still past 64 KB
LDS_EDGE = Case("h32_dot_g1_lds_past_64k", 32, 1, 257, 63, False, 1, 1, 10.0, True, None, 14)
LDS_MOST, LDS_REFUSED = (480, 63), (480, 64)


def decode_inputs(c):
    """Seeded operands of one case, in the style of test_gpu_train_kernels.py::_decode_inputs: enc_out scaled by 0.6, weights by
    1/sqrt(H), latent by 3; 'Bahdanau' sides with W_ref = 2 I (pointer) / 0.5 I (glimpse) and b_ref = 0, so that ref is exact in
    fp32.  V is a weight here, scaled like the others (as the model's own initialisation, oracle.pn.make_state_dict): V of order
    1 sums H tanh values to logits of order sqrt(H) / 3, which C*tanh rounds to +-C at H = 256 — a window of ties in fp32 and of
    margins below any allowance in float64, where no decision can be checked.  ``inputs`` [B,L,8]: random rows, pairwise distinct
    within a problem (a pick is recognised by its action row)."""
    g = torch.Generator().manual_seed(c.seed)
    B, T, K, H = c.B, c.T, c.K, c.H
    L, s = T * K, 1 / math.sqrt(H)
    u = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1)        # noqa: E731
    w = {"enc_out": u(B, L, H) * 0.6, "embedded": u(B, L, H), "h0": u(B, H) * 0.5, "c0": u(B, H), "start": u(H),
         "wih": u(4 * H, H) * s, "whh": u(4 * H, H) * s, "bih": u(4 * H) * s, "bhh": u(4 * H) * s,
         "latent": u(B, T, K) * 3 if c.latent else None}
    if c.bah:
        for tag in ("p",) + (("g",) if c.G else ()):
            w[f"{tag}_wq"], w[f"{tag}_bq"], w[f"{tag}_v"] = u(H, H) * s, u(H) * s, u(H) * s
    w["inputs"] = torch.rand(B, L, 8, generator=g)
    for b in range(B):
        assert len({r.tobytes() for r in w["inputs"][b].numpy()}) == L, "input rows must be pairwise distinct"
    return with_refs(w)


W_REF_SCALE = {"p": 2.0, "g": 0.5}


def with_refs(w):
    """(Re)derive the 'Bahdanau' refs of ``w`` from its enc_out: W_ref = 2 I / 0.5 I, b_ref = 0."""
    for tag in ("p", "g"):
        if f"{tag}_wq" in w:
            w[f"{tag}_ref"] = w["enc_out"] * W_REF_SCALE[tag]
    return w


def draw_pick(probs_row, u):
    """The decoders' draw: the first r with u < cdf_r (running sum in probs_row's dtype), else the last r of positive probability."""
    cdf = torch.cumsum(probs_row, 0)
    below = (float(u) < cdf).nonzero()
    if len(below):
        return int(below[0])
    return int((probs_row > 0).nonzero()[-1])


@torch.no_grad()
def replay(w, c, dtype, idx=None):
    """The decode of case ``c`` in ``dtype`` along ``idx`` [B,T] (global positions), or free-running when idx is None.
    -> {"z0" [B,T,K] C*tanh(logits) (what win_logits holds), "z" [B,T,K] (+ latent), "probs" [B,T,K], "q" [B,T,H] (the query after
    the glimpse rounds), "idx" [B,T] (the path taken)}."""
    B, T, K, G, bah = c.B, c.T, c.K, c.G, c.bah
    f = lambda k: w[k].to(dtype) if w.get(k) is not None else None      # noqa: E731
    enc, emb, wih, whh, bih, bhh, latent = (f(k) for k in ("enc_out", "embedded", "wih", "whh", "bih", "bhh", "latent"))
    L = enc.shape[1]
    rows = torch.arange(B)
    h, cc = f("h0"), f("c0")
    x = f("start").unsqueeze(0).repeat(B, 1)
    pref = f("p_ref") if bah else enc
    gref = f("g_ref") if (bah and G) else enc

    def logits(tag, q, ref):
        if bah:
            qp = F.linear(q, f(f"{tag}_wq"), f(f"{tag}_bq"))
            return (f(f"{tag}_v") * torch.tanh(qp.unsqueeze(1) + ref)).sum(2)
        return torch.bmm(ref, q.unsqueeze(2)).squeeze(2)

    path = torch.zeros(B, T, dtype=torch.long)
    chosen = torch.zeros(B, L, dtype=torch.bool)
    z0s, zs, ps, qs = [], [], [], []
    for k in range(T):
        gates = F.linear(x, wih, bih) + F.linear(h, whh, bhh)
        i, fg, gg, o = gates.chunk(4, 1)
        cc = torch.sigmoid(fg) * cc + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(cc)
        q = h
        for _ in range(G):
            uu = logits("g", q, gref).masked_fill(chosen, float("-inf"))
            q = torch.bmm(F.softmax(uu, 1).unsqueeze(1), gref).squeeze(1)
        z = logits("p", q, pref[:, k * K:(k + 1) * K])
        if c.use_tanh:
            z = c.C * torch.tanh(z)
        z0s.append(z)
        if latent is not None:
            z = z + latent[:, k]
        p = F.softmax(z, 1)
        zs.append(z), ps.append(p), qs.append(q)
        if idx is not None:
            pick = idx[:, k].long() - k * K
        elif c.sample_seed is not None:
            pick = torch.tensor([draw_pick(p[b], opn.stream_uniform24(c.sample_seed, b * T + k)) for b in range(B)])
        else:
            pick = torch.from_numpy(np.argmax(z.numpy(), 1))            # numpy: the first maximum
        path[:, k] = k * K + pick
        chosen[rows, path[:, k]] = True
        x = emb[rows, path[:, k]]
    return {"z0": torch.stack(z0s, 1), "z": torch.stack(zs, 1), "probs": torch.stack(ps, 1), "q": torch.stack(qs, 1), "idx": path}


def allowance(r64, r32):
    """eps of a case: what its logits themselves are allowed against float64 (the yardstick's statement, factor 4, floor 2e-6),
    from the two replays of one path."""
    z64 = r64["z"]
    return 4.0 * float((r32["z"].double() - z64).abs().max()) + 2e-6 * float(z64.abs().max())


def margins(z64):
    """top-1 - top-2 of every decision [B,T] (K > 1)."""
    top = torch.topk(z64, 2, dim=2).values
    return top[..., 0] - top[..., 1]


def check_greedy(pick, z64, eps):
    """Every decision: the pick's float64 logit within 2 eps of the window's float64 maximum.  pick [B,T] window positions."""
    at = torch.gather(z64, 2, pick.long().unsqueeze(2)).squeeze(2)
    short = z64.max(2).values - at
    bad = (short > 2 * eps).nonzero().tolist()
    assert not bad, f"picks beyond 2 eps = {2 * eps:.3e} of the float64 maximum at (b, k) {bad[:8]}: short by {short.max():.3e}"


def draw_distance(probs64_row, u):
    """Distance of the draw to the nearest cdf boundary that separates two positions."""
    cdf = torch.cumsum(probs64_row, 0)[:-1]
    return float((cdf - float(u)).abs().min()) if len(cdf) else float("inf")


def check_sampled(pick, probs64, seed):
    """Every decision: the pick is the draw rule's on the float64 cdf; where u lies within TAU_DRAW of the boundary between that
    position and a neighbour, the neighbour is accepted too.  pick [B,T] window positions."""
    B, T, _ = probs64.shape
    for b in range(B):
        for k in range(T):
            u = opn.stream_uniform24(seed, b * T + k)
            want, got = draw_pick(probs64[b, k], u), int(pick[b, k])
            if got == want:
                continue
            cdf = torch.cumsum(probs64[b, k], 0)
            near = abs(got - want) == 1 and abs(float(cdf[min(got, want)]) - float(u)) <= TAU_DRAW
            assert near, f"draw (b={b}, k={k}): u={float(u):.8f} picks {want} on the float64 cdf, the kernel picked {got}"


def bite(c, r64, eps):
    """What gives the decision rules their bite, from float64 alone: the shares the tests hold against their thresholds.
    Greedy: the share of decisions (K > 1) whose float64 margin exceeds 2 eps.  Sampled: the share of picks that are not the
    argmax, and the share of draws within TAU_DRAW of a cdf boundary."""
    out = {}
    if c.K > 1:
        out["margin_share"] = float((margins(r64["z"]) > 2 * eps).double().mean())
    if c.sample_seed is not None:
        pick = r64["idx"] - torch.arange(c.T) * c.K
        out["not_argmax_share"] = float((pick != torch.from_numpy(np.argmax(r64["z"].numpy(), 2))).double().mean())
        d = [draw_distance(r64["probs"][b, k], opn.stream_uniform24(c.sample_seed, b * c.T + k))
             for b in range(c.B) for k in range(c.T)]
        out["near_boundary_share"] = float(np.mean([x <= TAU_DRAW for x in d]))
    return out


def assert_bite(c, r64, eps):
    m = bite(c, r64, eps)
    assert m.get("margin_share", 1.0) >= 0.98, (c.id, m, eps)
    if c.sample_seed is not None:
        assert m["not_argmax_share"] >= 0.30 and m["near_boundary_share"] <= 0.02, (c.id, m)
    return m


# ---- exact ties: T = 4, K = 6, one glimpse round.  Window EQUAL_WINDOW holds K copies of one row (equal latent): K logits equal bit
# for bit, the pick is the window's first position.  Window PAIR_WINDOW holds one row at the positions PAIR only, with the latent at
# the top of its range there and below 0 elsewhere, the row scaled by PAIR_SCALE, so that the two are the float64 maximum by more than 2 eps (test_attn_decode_host.py holds
# that): the pick is the first of them
PAIR_WINDOW, PAIR, EQUAL_WINDOW = 1, (1, 4), 2
FIRST_MAX_CASES = [Case("h32_dot", 32, 2, 4, 6, False, 1, 1, 10.0, True, None, 21),
                   Case("h32_bah", 32, 2, 4, 6, True, 1, 1, 10.0, True, None, 22),
                   Case("h256_dot", 256, 2, 4, 6, False, 1, 1, 10.0, True, None, 23),
                   Case("h256_bah", 256, 2, 4, 6, True, 1, 1, 10.0, True, None, 24)]
PAIR_SCALE = 3.0


def equal_rows_inputs(c):
    w = decode_inputs(c)
    K = c.K
    for b in range(c.B):
        row = w["enc_out"][b, PAIR_WINDOW * K + PAIR[0]] * PAIR_SCALE
        w["latent"][b, PAIR_WINDOW] = -w["latent"][b, PAIR_WINDOW].abs()      # the rest of the window: latent below 0
        for r in PAIR:
            w["enc_out"][b, PAIR_WINDOW * K + r] = row
            w["latent"][b, PAIR_WINDOW, r] = 3.0                              # the pair: the top of the latent's range
        w["enc_out"][b, EQUAL_WINDOW * K:(EQUAL_WINDOW + 1) * K] = w["enc_out"][b, EQUAL_WINDOW * K].clone()
        w["latent"][b, EQUAL_WINDOW] = w["latent"][b, EQUAL_WINDOW, 0].clone()
    return with_refs(w)


def pair_margin(r64):
    """[B]: how far the float64 logits of the PAIR positions stand above the rest of their window."""
    z = r64["z"][:, PAIR_WINDOW]
    rest = [r for r in range(z.shape[1]) if r not in PAIR]
    return z[:, list(PAIR)].min(1).values - z[:, rest].max(1).values
