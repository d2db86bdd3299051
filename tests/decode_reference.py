"""Helper of the production pointer decoders' tests (not a test file): what test_gpu_decode_replay.py (GPU) and
test_decode_replay_host.py (no GPU) share.  The decoders are the shipped 'Dot' configuration without glimpses (modelPN.py:204-239):
pointer_decode_lean_kernel + pick_prob_kernel, pointer_decode_coop_kernel<false,false> / <true,true> and the streaming
pointer_decode_kernel<H,BT,REP>, all behind ops.pointer_decode.  Their reference is attn_decode_reference.replay with bah=False,
G=0; the allowance, the decision rules and the bite conditions are that module's, used as they stand.  Added here, because the
production forms need them: the operands of a net from a seed with the decoder input DERIVED (embedded = inputs . emb_w^T + emb_b,
formed in the replay's own dtype), the device dictionary of a net with the folded input side of modelPN.PointerNet.packed(), the
two-level replay (High's latent = the Low replay's z0 in the same dtype), the cases, and the planted exact ties."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

import attn_decode_reference as adr

D, F32 = adr.D, adr.F32
LEVELS = ("low", "high")

# form: "lean" (folded, greedy: pointer_decode_lean_kernel + pick_prob_kernel), "coop" (pointer_decode_coop_kernel<false,false>:
# emb_w / emb_b only, no folded side), "sampled" (pointer_decode_coop_kernel<true,true>: folded, the LAST net draws), "streaming"
# (pointer_decode_kernel<H,BT,false>, impl 1).  nets: 1, or 2 = Low plus High with latent_from=0.  latent: a latent_win tensor
# (u * 3) given to the single net.  sample_seed: the last net draws from that stream.  bt: the BT a streaming case selects.
# enc_scale: enc_out = u * enc_scale.  0.6 everywhere but in the sampled cases at H = 256: there Low's and High's C * tanh of dots of
# deviation 2 both sit near +-10, their sum leaves one or two candidates with nearly all of the probability, and the expected
# share of draws that are not the argmax is 0.17 .. 0.23 whatever the seed (198 draws: 0.30 is four deviations away).  At 0.15 it is
# about 0.5, so the bar of 0.30 holds by the case's construction and not by its seed.
Case = namedtuple("Case", "id form H B T K nets latent use_tanh C sample_seed seed bt enc_scale", defaults=(None, 0.6))

# A tile is 16 problems (COOP_ROWS), a group 8 members; the lean kernel takes EVH = 2 for K <= 8 and EVH = 1 for K 9..16.
CASES = [
    Case("L1", "lean", 256, 17, 6, 16, 2, False, True, 10.0, None, 101),      # full wide window; the second tile holds one row
    Case("L2", "lean", 256, 16, 3, 9, 2, False, True, 10.0, None, 102),       # first wide width; exactly one tile
    Case("L3", "lean", 256, 70, 6, 8, 2, False, True, 10.0, None, 103),       # full narrow window; 420 rows for pick_prob_kernel
    Case("L4", "lean", 256, 1, 1, 1, 2, False, True, 10.0, None, 104),        # one row, one step, one candidate
    Case("L5", "lean", 256, 33, 2, 3, 1, False, True, 10.0, None, 105),       # one net, no latent
    Case("L6", "lean", 256, 17, 4, 5, 1, True, False, 10.0, None, 106),       # latent_win tensor; raw dots as logits
    Case("L7", "lean", 256, 18, 1, 16, 2, False, True, 2.5, None, 107),       # T = 1 with High one step behind Low; tanh_c 2.5
    Case("C1", "coop", 256, 17, 6, 16, 2, False, True, 10.0, None, 111),
    Case("C2", "coop", 256, 70, 6, 8, 2, False, True, 10.0, None, 112),
    Case("S1", "sampled", 256, 33, 6, 10, 2, False, True, 10.0, 7, 121, enc_scale=0.15),
    Case("S2", "sampled", 256, 17, 4, 16, 2, False, True, 10.0, 11, 122, enc_scale=0.15),
    Case("P1", "streaming", 32, 41, 2, 3, 2, False, True, 10.0, None, 131, 1),
    Case("P1_K17", "streaming", 32, 41, 2, 17, 2, False, True, 10.0, None, 132, 1),     # a window past 16: only this form takes it
    Case("P2", "streaming", 32, 521, 2, 3, 2, False, True, 10.0, None, 133, 2),
    Case("P3", "streaming", 32, 1030, 2, 3, 2, False, True, 10.0, None, 134, 4),
    Case("P4", "streaming", 256, 41, 2, 3, 2, False, True, 10.0, None, 135, 1),
    Case("P4_K17", "streaming", 256, 41, 2, 17, 2, False, True, 10.0, None, 136, 1),
    Case("P5", "streaming", 256, 521, 2, 3, 2, False, True, 10.0, None, 137, 2),
    Case("P6", "streaming", 256, 1030, 2, 3, 2, False, True, 10.0, None, 138, 4),
    Case("P7", "streaming", 32, 41, 6, 10, 2, False, True, 10.0, 13, 141, 1),
    Case("P8", "streaming", 256, 41, 6, 10, 2, False, True, 10.0, 17, 142, 1, 0.15),
]
BY_ID = {c.id: c for c in CASES}

# the lean builds: (precision, impl, stamps).  impl 4 is the 256-register build for two workgroups per CU (OCC = 2), the stamp bit
# (GNNPN_ABLATE_DEC_STAMPS, n_per <= 8) the diagnostic build.  With EVH by the case's K: the eight unstamped builds and the two stamped
LEAN_RUNS = [(c, "f32", 2, False) for c in ("L1", "L2", "L3", "L4", "L5", "L6", "L7")] + \
            [(c, p, i, False) for c in ("L1", "L2", "L3", "L6") for p, i in (("split", 2), ("f32", 4), ("split", 4))] + \
            [("L3", "f32", 2, True), ("L3", "split", 2, True)]


def decode_bt(rows):
    """Problems per workgroup of the streaming decoder (csrc/decode.hip launch_decode)."""
    bt = 1
    while bt < 4 and rows // (bt * 2) >= 256:
        bt *= 2
    return bt


def decode_inputs(c):
    """Seeded operands of one case, in the style of attn_decode_reference.decode_inputs: ``inputs`` [B,L,8] random with pairwise
    distinct rows inside a problem (a pick is recognised by its action row), shared by the nets; per net enc_out scaled by c.enc_scale (0.6), h0
    by 0.5, the LSTM weights and emb_b by 1/sqrt(H), emb_w [H,8] by 1/sqrt(8) (its fan-in); a single net's latent by 3.
    -> {"inputs", "nets": [operands of Low(, of High)]}."""
    g = torch.Generator().manual_seed(c.seed)
    B, T, K, H = c.B, c.T, c.K, c.H
    L, s = T * K, 1 / math.sqrt(H)
    u = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1)        # noqa: E731
    inputs = torch.rand(B, L, 8, generator=g)
    assert rows_distinct(inputs), "input rows must be pairwise distinct"
    nets = []
    for _ in range(c.nets):
        nets.append({"enc_out": u(B, L, H) * c.enc_scale, "h0": u(B, H) * 0.5, "c0": u(B, H), "start": u(H),
                     "wih": u(4 * H, H) * s, "whh": u(4 * H, H) * s, "bih": u(4 * H) * s, "bhh": u(4 * H) * s,
                     "emb_w": u(H, 8) / math.sqrt(8), "emb_b": u(H) * s, "latent": u(B, T, K) * 3 if c.latent else None})
    return {"inputs": inputs, "nets": nets}


def rows_distinct(inputs):
    return all(len({r.tobytes() for r in x.numpy()}) == x.shape[0] for x in inputs)


def net_case(c, level):
    """The attn_decode_reference.Case of one net of ``c``: 'Dot', no glimpse; only the last net of a sampled case draws."""
    draws = c.sample_seed is not None and level == LEVELS[c.nets - 1]
    latent = c.latent or level == "high"
    return adr.Case(f"{c.id}/{level}", c.H, c.B, c.T, c.K, False, 0, int(c.use_tanh), c.C, latent, c.sample_seed if draws else None, c.seed)


@torch.no_grad()
def replay_net(w, inputs, nc, dtype, idx=None, latent=None):
    """attn_decode_reference.replay of one net with its decoder input derived in ``dtype`` (embedding2, modelPN.py:190) and the
    latent either the net's own tensor or the one handed in."""
    wd = dict(w)
    wd["embedded"] = F.linear(inputs.to(dtype), w["emb_w"].to(dtype), w["emb_b"].to(dtype))
    wd["latent"] = w["latent"] if latent is None else latent
    return adr.replay(wd, nc, dtype, idx=idx)


@torch.no_grad()
def replay(ins, c, dtype, idx=None):
    """The decode of case ``c`` in ``dtype``: Low along idx[0] and, with two nets, High along idx[1] with latent = the Low replay's
    z0 (what the kernels add: Low's window logits before Low's own latent, modelPN.py:215-218); free-running when idx is None.
    -> [replay dict of Low(, of High)]."""
    out = []
    for n, level in enumerate(LEVELS[:c.nets]):
        out.append(replay_net(ins["nets"][n], ins["inputs"], net_case(c, level), dtype, None if idx is None else idx[n],
                              out[0]["z0"] if n else None))
    return out


def device_net(w, dev, fold, latent_from=-1, sample_seed=None, split=False):
    """The dictionary of one net for ops.pointer_decode: weights through ops.pack_lstm_weight; with ``fold`` the folded input side
    xw_fold = W_ih W_e, xb_fold = W_ih b_e + b_ih, start_fold = W_ih start + b_ih, formed in float64 and rounded once exactly as
    modelPN.PointerNet.packed() does (modelPN.py:182-192, restated); with ``split`` the exact split of W_hh made once per model
    (ops.pack_lstm_split_weights), else the kernels split for themselves."""
    from gnnpn_sc_amd import ops
    d = {k: w[k].to(dev) for k in ("enc_out", "h0", "c0", "start", "bih", "bhh", "emb_w", "emb_b")}
    d.update(wih=ops.pack_lstm_weight(w["wih"]).to(dev), whh=ops.pack_lstm_weight(w["whh"]).to(dev),
             latent_win=None if w["latent"] is None else w["latent"].to(dev), latent_from=latent_from)
    if split:
        d["whh_split"] = ops.pack_lstm_split_weights(d["whh"])
    if fold:
        back = lambda t: t.float().contiguous().to(dev)                   # noqa: E731
        d_ih, w_e, b_e, d_b = (w[k].double() for k in ("wih", "emb_w", "emb_b", "bih"))
        d.update(xw_fold=back(d_ih @ w_e), xb_fold=back(d_ih @ b_e + d_b), start_fold=back(d_ih @ w["start"].double() + d_b))
    if sample_seed is not None:
        d.update(sample=True, sample_seed=int(sample_seed))
    return d


def device_nets(ins, c, dev, split=False):
    """The ``nets`` list of ops.pointer_decode for case ``c``."""
    fold = c.form in ("lean", "sampled")
    nets = []
    for n in range(c.nets):
        last = n == c.nets - 1
        nets.append(device_net(ins["nets"][n], dev, fold, latent_from=0 if n else -1, sample_seed=c.sample_seed if last else None,
                               split=split))
    return nets


# ---- exact ties, T = 4.  Window EQUAL_WINDOW of every net holds K copies of one enc_out row: K logits equal bit for bit in Low, so
# in the latent High adds, so in High; the pick of both nets is the window's first position.  Window PAIR_WINDOW holds one row at the
# two positions (p_b, q_b) of the problem: the row of that window with the largest |dot| against the step's float64 query, times
# +-PAIR_SCALE so that its dot is positive — three times the largest dot of the window, in each net, so the pair is the float64
# maximum of both nets (test_decode_replay_host.py holds the margin against 2 eps) and the pick is p_b.
PAIR_WINDOW, EQUAL_WINDOW, PAIR_SCALE = adr.PAIR_WINDOW, adr.EQUAL_WINDOW, adr.PAIR_SCALE
TIE_B, TIE_T = 17, 4
TIE_CASES = [Case(f"lean_K{K}", "lean", 256, TIE_B, TIE_T, K, 2, False, True, 10.0, None, seed) for K, seed in ((16, 201), (6, 202))] + \
            [Case("coop_K16", "coop", 256, TIE_B, TIE_T, 16, 2, False, True, 10.0, None, 203)] + \
            [Case(f"streaming_h{H}_K{K}", "streaming", H, TIE_B, TIE_T, K, 2, False, True, 10.0, None, seed, 1)
             for H, K, seed in ((32, 6, 204), (32, 17, 205), (256, 6, 206), (256, 17, 207))]
TIE_BY_ID = {c.id: c for c in TIE_CASES}
TIE_RUNS = [(c, p, i) for c in ("lean_K16", "lean_K6") for p in ("f32", "split") for i in (2, 4)] + [("coop_K16", "f32", 2)] + \
           [(c.id, "f32", 1) for c in TIE_CASES if c.form == "streaming"]


def tie_pairs(B, K):
    """(p_b, q_b), p_b < q_b, per problem.  The distances q_b - p_b cycle through the DPP rotation distances below K (1, 2, 4, 8);
    the four problems that share a wavefront of a tile (rows 4w .. 4w + 3) get four different p_b — lanes of one ballot that must
    disagree; the last problem's q_b is K - 1."""
    dist = [d for d in (1, 2, 4, 8) if d < K]
    pairs = []
    for b in range(B):
        used = {p for p, _ in pairs[b - b % 4:b]}
        for shift in range(len(dist)):
            d = dist[(b + shift) % len(dist)]
            free = [p for p in ((b % 4 + b // 4 + j) % (K - d) for j in range(K - d)) if p not in used]
            if free:
                pairs.append((free[0], free[0] + d))
                break
        else:
            raise AssertionError(f"no pair left for problem {b} at K = {K}")
    d = pairs[-1][1] - pairs[-1][0]
    if (B - 1) % 4 == 0:                         # alone in its wavefront: free to take the window's last position
        pairs[-1] = (K - 1 - d, K - 1)
    return pairs


def tie_inputs(c):
    """decode_inputs(c) with the equal window and the pair window planted in the enc_out of every net.  -> (ins, pairs)."""
    ins = decode_inputs(c)
    K = c.K
    pairs = tie_pairs(c.B, K)
    for w in ins["nets"]:
        e = w["enc_out"]
        e[:, EQUAL_WINDOW * K:(EQUAL_WINDOW + 1) * K] = e[:, EQUAL_WINDOW * K:EQUAL_WINDOW * K + 1].clone()
    # the query of step PAIR_WINDOW depends on the picks before it only: none of them looks at this window's enc_out
    q = [r["q"][:, PAIR_WINDOW] for r in replay(ins, c, D)]
    for w, qn in zip(ins["nets"], q):
        e = w["enc_out"]
        win = e[:, PAIR_WINDOW * K:(PAIR_WINDOW + 1) * K]
        dots = torch.einsum("bkh,bh->bk", win.double(), qn)
        for b, (p, r) in enumerate(pairs):
            j = int(dots[b].abs().argmax())
            row = win[b, j].clone() * (PAIR_SCALE if dots[b, j] > 0 else -PAIR_SCALE)
            win[b, p] = row
            win[b, r] = row
    return ins, pairs


def pair_margin(r64, pairs):
    """[B]: how far the float64 logits of the pair stand above the rest of their window (one net's replay)."""
    z = r64["z"][:, PAIR_WINDOW]
    out = []
    for b, (p, r) in enumerate(pairs):
        rest = [j for j in range(z.shape[1]) if j not in (p, r)]
        out.append(min(z[b, p], z[b, r]) - z[b, rest].max())
    return torch.stack(out)
