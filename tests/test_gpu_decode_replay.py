"""The production pointer decoders behind ops.pointer_decode — pointer_decode_lean_kernel<SPLIT, OCC, EVH, DIAG> with
pick_prob_kernel, pointer_decode_coop_kernel<false,false> and <true,true>, the streaming pointer_decode_kernel<H, BT, false> —
each against a float64 replay of its own path: tests/decode_reference.py holds the seeded operands, the cases, the two-level
replay and the planted ties; tests/attn_decode_reference.py the reference, the allowance and the decision rules;
tests/test_decode_replay_host.py holds the cases to what gives these rules their bite, on the CPU.

Every case calls ops.pointer_decode directly on the seeded operands, twice (the same bits in every output), with the queries asked
for.  Per net, with the kernel's own picks replayed in float64 and in float32:
  path      every pick lies in its step's window; every action row is the pick's input row, bit for bit;
  numeric   kernel_checks.Recorder.yardstick with its defaults (factor 4, floor 2e-6) for win_logits against z0, queries against q
            and pick_prob against the replay's softmax gathered at the pick — the exact-split builds are held to the same bar;
  decision  every one: a greedy pick's float64 logit lies within 2 eps of the window's float64 maximum, eps = 4 max|z32 - z64| +
            2e-6 max|z64| (attn_decode_reference.allowance); a drawn pick is the draw rule's on the float64 cdf (a neighbour where
            u is within parity.TAU_DRAW of the boundary);
  bite      from float64 alone: at least 98 % of the decisions with K > 1 have a margin above 2 eps; of the drawn picks at least
            30 % are not the argmax and at most 2 % of the draws lie within TAU_DRAW of a cdf boundary."""
import pytest
import torch

import attn_decode_reference as adr
import decode_reference as dr
from kernel_checks import Recorder, same_bits, twice

pytestmark = pytest.mark.gpu

REC = Recorder("agreement_decode_replay")
KEYS = ("idx", "win_logits", "pick_prob", "actions", "queries")


def _ops():
    from gnnpn_sc_amd import ops
    return ops


def _decode(dev, ins, c, precision="f32", impl=0, stamps=False):
    """ops.pointer_decode on the operands of case ``c``, twice; for a cooperative form the status follows.  The call must take the
    form the case names: ops.coop_supported says which one (H, K, impl) selects, so a fall-through to another form fails here.
    -> the outputs of every net on the host."""
    ops = _ops()
    assert ops.coop_supported(c.H, c.K, impl) == (c.form != "streaming"), (c.id, impl)
    nets = dr.device_nets(ins, c, dev, split=precision == "split" and impl == 4)   # impl 2: the kernel splits W_hh for itself
    x = ins["inputs"].to(dev)
    try:
        if stamps:
            ops.set_option("lstm_ablate", ops.GNNPN_ABLATE_DEC_STAMPS)            # the only way into the stamped builds
        outs = twice(lambda: ops.pointer_decode(nets, x, c.T, c.K, tanh_c=c.C, use_tanh=c.use_tanh, want_queries=True,
                                                precision=precision, impl=impl))
        if c.form != "streaming":
            ops.check_status(dev)
    finally:
        ops.set_option("lstm_ablate", 0)
    return [{k: o[k].cpu() for k in KEYS} for o in outs]


def _check(ins, c, outs, name, bite=True):
    """The statement of this file for one run.  -> (float64 replays, eps) per net."""
    B, T, K = c.B, c.T, c.K
    lo = torch.arange(T) * K
    idx = [o["idx"].long() for o in outs]
    for level, got, i in zip(dr.LEVELS, outs, idx):
        assert bool(((i >= lo) & (i < lo + K)).all()), f"{level}: a pick outside its window"
        assert same_bits(got["actions"], ins["inputs"][torch.arange(B).unsqueeze(1), i]), f"{level}: an action row is not the pick's input row"
    r64, r32 = dr.replay(ins, c, dr.D, idx=idx), dr.replay(ins, c, dr.F32, idx=idx)
    failures, eps = [], []
    for level, got, i, a, b in zip(dr.LEVELS, outs, idx, r64, r32):
        pick = i - lo
        at = lambda r: torch.gather(r["probs"], 2, pick.unsqueeze(2)).squeeze(2)      # noqa: E731
        for what, g, ref64, ref32 in (("win_logits", got["win_logits"], a["z0"], b["z0"]), ("queries", got["queries"], a["q"], b["q"]),
                                      ("pick_prob", got["pick_prob"], at(a), at(b))):
            assert bool(torch.isfinite(g).all()), (level, what)
            try:
                REC.yardstick(name, what, g, ref64, ref32)
            except AssertionError as e:                                               # every quantity is measured before the test fails
                failures.append(f"{level}: {e}")
        eps.append(adr.allowance(a, b))
    print(f"{name} [{c.id}]:", {k: f"{v:.3g}" for k, v in REC.worst[name].items()})
    assert not failures, failures
    for level, i, a, e in zip(dr.LEVELS, idx, r64, eps):
        nc = dr.net_case(c, level)
        if nc.sample_seed is None:
            adr.check_greedy(i - lo, a["z"], e)
        else:
            adr.check_sampled(i - lo, a["probs"], nc.sample_seed)
        if bite:
            adr.assert_bite(nc, a, e)
    return r64, eps


def _lean_name(precision, impl, stamps=False):
    return f"lean_{precision}_impl{impl}" + ("_stamps" if stamps else "")


@pytest.mark.parametrize("cid,precision,impl,stamps", dr.LEAN_RUNS,
                         ids=[f"{c}-{p}-impl{i}" + ("-stamps" if s else "") for c, p, i, s in dr.LEAN_RUNS])
def test_lean_decode_vs_float64_replay(dev, cid, precision, impl, stamps):
    """pointer_decode_lean_kernel + pick_prob_kernel, the decoder of every benchmark step and every ML2PNPipeline.run: L1 the full
    wide window with a second tile of one row, L2 the first wide width on exactly one tile, L3 the full narrow window (EVH = 2) with
    420 (problem, step) rows, so that pick_prob_kernel's second workgroup starts at a step other than 0, L4 one row, one step, one
    candidate, L5 one net without latent, L6 one net with a latent_win tensor and raw dots as logits, L7 T = 1 with tanh_c 2.5,
    where High runs one step behind Low.  L1, L2, L3 and L6 in fp32 and exact-split arithmetic, one and two workgroups per CU
    (impl 2 and 4): the eight unstamped builds; L3 under the stamp bit: the two stamped ones."""
    c = dr.BY_ID[cid]
    ins = dr.decode_inputs(c)
    outs = _decode(dev, ins, c, precision, impl, stamps)
    _check(ins, c, outs, _lean_name(precision, impl, stamps))
    if cid == "L4":                                                                   # one candidate: nothing to round
        for o in outs:
            assert int(o["idx"]) == 0 and float(o["pick_prob"]) == 1.0


@pytest.mark.parametrize("cid", ["C1", "C2"])
def test_two_stage_coop_decode_vs_float64_replay(dev, cid):
    """pointer_decode_coop_kernel<false,false>: no folded side, the picked rows embedded in the kernel from emb_w / emb_b, at the
    full wide and the full narrow window."""
    c = dr.BY_ID[cid]
    ins = dr.decode_inputs(c)
    _check(ins, c, _decode(dev, ins, c, impl=2), "coop_two_stage")


@pytest.mark.parametrize("cid", ["S1", "S2"])
def test_sampled_coop_decode_vs_float64_replay(dev, cid):
    """pointer_decode_coop_kernel<true,true>: Low greedy, every High pick drawn from the window softmax."""
    c = dr.BY_ID[cid]
    ins = dr.decode_inputs(c)
    _check(ins, c, _decode(dev, ins, c, impl=2), "coop_sampled")


STREAMING = [c.id for c in dr.CASES if c.form == "streaming"]


@pytest.mark.parametrize("cid", STREAMING)
def test_streaming_decode_vs_float64_replay(dev, cid):
    """pointer_decode_kernel<H, BT, false>, H = 32 and 256 at the batch sizes that select 1, 2 and 4 problems per workgroup with a
    partly filled last workgroup; windows of 17 candidates, which only this form takes; P7 and P8 with every High pick drawn."""
    c = dr.BY_ID[cid]
    assert dr.decode_bt(c.B) == c.bt and (c.bt == 1 or c.B % c.bt != 0)
    ins = dr.decode_inputs(c)
    _check(ins, c, _decode(dev, ins, c, impl=1), f"streaming_h{c.H}")


@pytest.mark.parametrize("cid,precision,impl", dr.TIE_RUNS, ids=[f"{c}-{p}-impl{i}" for c, p, i in dr.TIE_RUNS])
def test_decode_first_maximum_on_planted_ties(dev, cid, precision, impl):
    """Exact ties in front of every greedy pick rule (the lean kernel's four fmaxf DPP rotations, ballot, shift and ffs; the coop
    kernel's key reduction; the streaming form's strict '>'), in Low and in High.  One window of K equal enc_out rows: K logits
    equal bit for bit, the pick is the window's first position.  One window with one row at the positions (p_b, q_b) only, the
    float64 maximum by more than 2 eps: the pick is p_b.  The pairs differ from problem to problem — distances 1, 2, 4, 8, four
    different p_b among the rows that share a wavefront, one q_b = K - 1 — so that a rotation left out, a ballot read at the wrong
    shift or a last-maximum rule each move a pick.  The numeric and decision checks run too."""
    c = dr.TIE_BY_ID[cid]
    K, pw, ew = c.K, dr.PAIR_WINDOW, dr.EQUAL_WINDOW
    ins, pairs = dr.tie_inputs(c)
    outs = _decode(dev, ins, c, precision, impl)
    name = (_lean_name(precision, impl) if c.form == "lean" else "coop_two_stage" if c.form == "coop" else f"streaming_h{c.H}") + "_ties"
    r64, eps = _check(ins, c, outs, name, bite=False)                                  # half of the windows are ties on purpose
    first = torch.tensor([p for p, _ in pairs])
    rows = torch.arange(c.B)
    for level, got, a, e in zip(dr.LEVELS, outs, r64, eps):
        win = got["win_logits"]
        assert same_bits(win[:, ew], win[:, ew, :1].expand(-1, K).contiguous()), f"{level}: equal rows, different logits"
        assert torch.equal(got["idx"][:, ew].long(), torch.full((c.B,), ew * K)), (level, got["idx"][:, ew])
        p, q = first, torch.tensor([q for _, q in pairs])
        assert same_bits(win[rows, pw, p], win[rows, pw, q]), f"{level}: the pair's logits differ"
        assert float(dr.pair_margin(a, pairs).min()) > 2 * e, level
        assert torch.equal(got["idx"][:, pw].long(), pw * K + first), (level, got["idx"][:, pw], first)
