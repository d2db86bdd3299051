"""-m "not gpu": what the production decoders' GPU tests (test_gpu_decode_replay.py) presuppose of their committed cases, from the
free-running float64 and float32 replays alone (tests/decode_reference.py): decisions with a margin, draws that are draws, distinct
input rows, the BT a streaming case claims, ties that are ties where and how they are meant to be — and the two-level replay held
against the oracle's own two-level forward."""
import pytest
import torch

import attn_decode_reference as adr
import decode_reference as dr
from oracle import pn as opn
from parity import robust_problems


def _free_run(ins, c):
    """float64 free-running, float32 along the same paths, and the allowance of each net."""
    r64 = dr.replay(ins, c, dr.D)
    r32 = dr.replay(ins, c, dr.F32, idx=[r["idx"] for r in r64])
    return r64, r32, [adr.allowance(a, b) for a, b in zip(r64, r32)]


@pytest.mark.parametrize("c", dr.CASES, ids=[c.id for c in dr.CASES])
def test_decode_cases_have_bite(c):
    ins = dr.decode_inputs(c)
    assert dr.rows_distinct(ins["inputs"])
    r64, r32, eps = _free_run(ins, c)
    for level, a, e in zip(dr.LEVELS, r64, eps):
        nc = dr.net_case(c, level)
        assert 0 < e < 1e-3, (level, e)                                   # of order 1e-5 against logits of order C
        m = adr.assert_bite(nc, a, e)
        pick = a["idx"] - torch.arange(c.T) * c.K
        assert bool(((pick >= 0) & (pick < c.K)).all())
        if nc.sample_seed is None:
            adr.check_greedy(pick, a["z"], e)
            if c.K > 1 and c.B * c.T >= 8:
                assert len(torch.unique(pick)) > 1, "every decision picks the same window position"
        else:
            adr.check_sampled(pick, a["probs"], nc.sample_seed)
        assert torch.isfinite(a["q"]).all() and torch.isfinite(a["z"]).all(), m


def test_decode_cases_cover_their_paths():
    """The shapes the cases are there for, against the kernels' constants: tiles of 16 problems, windows of at most 8 (EVH = 2) and
    of 9..16 (EVH = 1) candidates in the lean kernel, 256 (problem, step) rows per workgroup of pick_prob_kernel, BT by the
    streaming launcher's rule."""
    by = dr.BY_ID
    assert by["L1"].K == 16 and by["L1"].B % 16 == 1 and by["L2"].K == 9 and by["L2"].B == 16
    assert by["L3"].K == 8 and by["L3"].B * by["L3"].T > 256 and 256 % by["L3"].T != 0
    assert (by["L4"].B, by["L4"].T, by["L4"].K, by["L4"].nets) == (1, 1, 1, 2)
    assert by["L5"].nets == 1 and not by["L5"].latent and by["L6"].nets == 1 and by["L6"].latent and not by["L6"].use_tanh
    assert by["L7"].T == 1 and by["L7"].nets == 2 and by["L7"].C == 2.5
    assert [(by[i].B, by[i].T, by[i].K) for i in ("C1", "C2")] == [(17, 6, 16), (70, 6, 8)]
    assert [(by[i].B, by[i].T, by[i].K) for i in ("S1", "S2")] == [(33, 6, 10), (17, 4, 16)]
    for c in dr.CASES:
        assert c.H == 256 or c.form == "streaming"
        assert c.K <= 16 or c.form == "streaming"
        assert (c.sample_seed is not None) == (c.form == "sampled" or c.id in ("P7", "P8"))
        if c.form == "streaming":
            assert dr.decode_bt(c.B) == c.bt and (c.bt == 1 or c.B % c.bt != 0), c.id
    assert {(c.H, c.bt) for c in dr.CASES if c.form == "streaming"} == {(h, bt) for h in (32, 256) for bt in (1, 2, 4)}
    assert {c.H for c in dr.CASES if c.K == 17} == {32, 256}
    # the ten lean builds <SPLIT, OCC, EVH, DIAG>: every unstamped one by (precision, impl, K <= 8), the stamped ones at K <= 8
    builds = {(p == "split", 2 if i == 4 else 1, 2 if by[cid].K <= 8 else 1, s) for cid, p, i, s in dr.LEAN_RUNS}
    assert builds == {(sp, occ, evh, False) for sp in (False, True) for occ in (1, 2) for evh in (1, 2)} | {(False, 1, 2, True), (True, 1, 2, True)}


@pytest.mark.parametrize("c", dr.TIE_CASES, ids=[c.id for c in dr.TIE_CASES])
def test_decode_tie_cases_are_ties(c):
    """The windows of test_decode_first_maximum_on_planted_ties: equal rows where they are meant to be in both nets, the pair the
    float64 maximum of its window by more than 2 eps in both nets, the float64 path through the first of the equals; over the batch
    the pair distances cover the DPP rotation distances below K, one pair ends at K - 1, and the four problems of a wavefront
    disagree about the first tied position."""
    K, B, pw, ew = c.K, c.B, dr.PAIR_WINDOW, dr.EQUAL_WINDOW
    assert (B, c.T) == (17, 4) and c.nets == 2 and c.sample_seed is None
    if c.form == "streaming":
        assert dr.decode_bt(B) == c.bt == 1
    ins, pairs = dr.tie_inputs(c)
    assert dr.rows_distinct(ins["inputs"])
    assert all(0 <= p < q < K for p, q in pairs) and len(pairs) == B
    assert {q - p for p, q in pairs} >= {d for d in (1, 2, 4, 8) if d < K}
    assert any(q == K - 1 for _, q in pairs)
    for b0 in range(0, B, 4):
        group = [p for p, _ in pairs[b0:b0 + 4]]
        assert len(set(group)) == len(group), (b0, group)                 # rows 4w .. 4w+3 share a wavefront: one ballot, four answers
    assert all(pairs[b][0] != pairs[b + 1][0] for b in range(B - 1) if (b + 1) % 16)
    r64, r32, eps = _free_run(ins, c)
    first = torch.tensor([p for p, _ in pairs])
    for w, a, e in zip(ins["nets"], r64, eps):
        rows = w["enc_out"][:, ew * K:(ew + 1) * K]
        assert bool((rows == rows[:, :1]).all())
        for b, (p, q) in enumerate(pairs):
            win = w["enc_out"][b, pw * K:(pw + 1) * K]
            assert torch.equal(win[p], win[q])
            assert not any(torch.equal(win[j], win[p]) for j in range(K) if j not in (p, q))
            assert torch.equal(a["z"][b, pw, p], a["z"][b, pw, q])
        assert bool((a["z"][:, ew] == a["z"][:, ew, :1]).all())
        assert float(dr.pair_margin(a, pairs).min()) > 2 * e, (float(dr.pair_margin(a, pairs).min()), e)
        # the windows before the pair window decide which query meets it: no fragile decision there
        assert float(adr.margins(a["z"])[:, :pw].min()) > 2 * e
        assert torch.equal(a["idx"][:, pw], pw * K + first)
        assert bool((a["idx"][:, ew] == ew * K).all())


def test_two_level_replay_is_the_oracles_forward():
    """The two-level replay, free-running in float32 on weights of oracle.pn.make_state_dict and the oracle's own encoder outputs,
    against oracle.pn.two_level_greedy (the imported reference's forward, nn.LSTM included): the same picks of both nets on the
    problems whose every decision has a margin (parity.robust_problems), Low's window logits to float32 rounding."""
    H, T, K, B = 32, 5, 4, 12
    sds = [opn.make_state_dict(H, 31), opn.make_state_dict(H, 32)]
    x = torch.rand(B, T * K, 8, generator=torch.Generator().manual_seed(5))
    ref = opn.two_level_greedy(sds[0], sds[1], x, T, K)
    nets = []
    for sd in sds:
        emb = torch.nn.functional.linear(x, sd["actor.embedding2.weight"], sd["actor.embedding2.bias"])
        with torch.no_grad():
            enc_out, (h_n, c_n) = opn._lstm_module(sd, "encoder", H)(emb)
        nets.append({"enc_out": enc_out, "h0": h_n[0], "c0": c_n[0], "start": sd["actor.decoder_start_input"],
                     "wih": sd["actor.decoder.weight_ih_l0"], "whh": sd["actor.decoder.weight_hh_l0"],
                     "bih": sd["actor.decoder.bias_ih_l0"], "bhh": sd["actor.decoder.bias_hh_l0"],
                     "emb_w": sd["actor.embedding2.weight"], "emb_b": sd["actor.embedding2.bias"], "latent": None})
    c = dr.Case("oracle", "streaming", H, B, T, K, 2, False, True, 10.0, None, 0)
    low, high = dr.replay({"inputs": x, "nets": nets}, c, dr.F32)
    robust = robust_problems(ref["margin_low"], ref["margin_high"])
    assert int(robust.sum()) >= B // 2
    assert torch.equal(low["idx"][robust], ref["idx_low"][robust])
    assert torch.equal(high["idx"][robust], ref["idx_high"][robust])
    assert float((low["z0"][robust] - ref["win_low"][robust]).abs().max()) < 1e-4
    assert float((high["z"][robust] - ref["win_high"][robust]).abs().max()) < 1e-4
