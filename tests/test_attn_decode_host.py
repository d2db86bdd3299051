"""-m "not gpu": what the general attention decoder's GPU tests (test_gpu_pn.py::test_attention_decode_*) presuppose of their
committed cases, from the float64 reference alone (tests/attn_decode_reference.py, free-running): decisions with a margin, draws
that are draws, inputs that hit the paths they are there for — and the reference held against the oracle's own forward."""
import pytest
import torch

import attn_decode_reference as adr
from oracle import pn as opn


def _free_run(c):
    """float64 free-running, float32 along the same path, and the case's allowance."""
    w = adr.decode_inputs(c)
    r64 = adr.replay(w, c, adr.D)
    r32 = adr.replay(w, c, adr.F32, idx=r64["idx"])
    return w, r64, r32, adr.allowance(r64, r32)


@pytest.mark.parametrize("c", adr.CASES, ids=[c.id for c in adr.CASES])
def test_attention_decode_cases_have_bite(c):
    w, r64, r32, eps = _free_run(c)
    assert 0 < eps < 1e-3, eps                                            # of order 1e-5 against logits of order C
    m = adr.assert_bite(c, r64, eps)
    pick = r64["idx"] - torch.arange(c.T) * c.K
    assert bool(((pick >= 0) & (pick < c.K)).all())
    if c.sample_seed is None:
        adr.check_greedy(pick, r64["z"], eps)
        if c.K > 1:
            assert len(torch.unique(pick)) > 1, "every decision picks the same window position"
    else:
        adr.check_sampled(pick, r64["probs"], c.sample_seed)
    assert torch.isfinite(r64["q"]).all() and torch.isfinite(r64["z"]).all(), m


def test_attention_decode_cases_cover_their_paths():
    """The shapes the cases are there for, against the kernel's constants: NT = 64 (H = 32) / 256 (H = 256) threads, NT / 64
    wavefronts, win[64], (L + T) * 4 bytes of dynamic LDS up to 120 KB."""
    by = {c.id: c for c in adr.CASES}
    nt = lambda c: max(64, c.H)                                           # noqa: E731
    assert {(c.H, c.bah) for c in adr.CASES} == {(32, False), (32, True), (256, False), (256, True)}
    assert all(sum(1 for c in adr.CASES if (c.H, c.bah) == hb) >= 2 for hb in ((32, False), (32, True), (256, False), (256, True)))
    for name in ("h32_dot_g2_T70_forced", "h256_dot_g1_T258_forced"):
        assert by[name].T > nt(by[name]) and by[name].K == 1 and by[name].G >= 1    # the mask loop's second stride
    assert by["h32_dot_g1_one_position"].T * by["h32_dot_g1_one_position"].K == 1
    assert by["h256_dot_g2_L3"].T * by["h256_dot_g2_L3"].K < nt(by["h256_dot_g2_L3"]) // 64
    assert by["h32_bah_g0_L63"].T * by["h32_bah_g0_L63"].K == 63 and by["h32_bah_g0_L63"].G == 0
    assert by["h256_dot_g8_L259"].T * by["h256_dot_g8_L259"].K == 259 and by["h256_dot_g8_L259"].G == 8
    assert by["h32_bah_g1_K64"].K == by["h256_bah_g1_K64"].K == 64
    assert by["h32_bah_g3_K17_no_tanh"].G == 3 and not by["h32_bah_g3_K17_no_tanh"].use_tanh
    assert by["h256_bah_g2_K16_no_tanh"].K % (256 // 64) == 0 and by["h32_bah_g3_K17_no_tanh"].K % 4
    assert {c.C for c in adr.CASES} >= {10.0, 5.0, 2.5, 1.0}
    assert {(c.H, c.bah, c.latent) for c in adr.CASES} == {(h, b, lat) for h in (32, 256) for b in (False, True) for lat in (False, True)}
    assert [c.sample_seed for c in adr.CASES if c.sample_seed is not None] == [7, 11]
    assert by["h32_dot_g1_B300"].B == 300
    lds = lambda T, K: (T * K + T) * 4                                    # noqa: E731
    e = adr.LDS_EDGE
    assert 64 * 1024 < lds(e.T, e.K) <= 120 * 1024 and lds(e.T - 1, e.K) <= 64 * 1024 and e.K == 63
    assert lds(*adr.LDS_MOST) == 120 * 1024 and lds(*adr.LDS_REFUSED) > 120 * 1024 and adr.LDS_REFUSED[1] <= 64


def test_attention_decode_mask_matters_where_the_window_is_forced():
    """K = 1: every pick is forced, so a glimpse that misses the mask shows only in the query.  Without -inf at the positions chosen
    so far — here: with a mask loop of one stride, NT positions — the float64 query of the last step moves by about its own size
    (0.8 and 1.2 of max |q|; the bar is several percent): far beyond what the yardstick allows."""
    for name in ("h32_dot_g2_T70_forced", "h256_dot_g1_T258_forced"):
        c = next(x for x in adr.CASES if x.id == name)
        w = adr.decode_inputs(c)
        r64 = adr.replay(w, c, adr.D)
        assert torch.equal(r64["idx"], torch.arange(c.T).expand(c.B, c.T))
        nt = max(64, c.H)
        # the query of the last step with only the first NT chosen positions masked (a mask loop of one stride)
        h_last = _unmasked_query(w, c, masked=nt)
        rel = float((h_last - r64["q"][:, -1]).abs().max() / r64["q"][:, -1].abs().max())
        assert rel > 0.05, (name, rel)


def _unmasked_query(w, c, masked):
    """The float64 query of the last step when only the first ``masked`` chosen positions are masked in the glimpse rounds."""
    B, T = c.B, c.T
    d = {k: (v.double() if v is not None and v.is_floating_point() else v) for k, v in w.items()}
    rows = torch.arange(B)
    h, cc, x = d["h0"], d["c0"], d["start"].unsqueeze(0).repeat(B, 1)
    for k in range(T):
        h, cc = opn.lstm_cell_explicit(x, h, cc, d["wih"], d["whh"], d["bih"], d["bhh"])
        x = d["embedded"][rows, k]
    q = h
    chosen = torch.zeros(B, T, dtype=torch.bool)
    chosen[:, :min(masked, T - 1)] = True
    for _ in range(c.G):
        u = torch.bmm(d["enc_out"], q.unsqueeze(2)).squeeze(2).masked_fill(chosen, float("-inf"))
        q = torch.bmm(torch.softmax(u, 1).unsqueeze(1), d["enc_out"]).squeeze(1)
    return q


@pytest.mark.parametrize("att,ng", [("Dot", 1), ("Bahdanau", 0), ("Bahdanau", 2)])
def test_attention_decode_reference_is_the_oracles_forward(att, ng):
    """The restatement against oracle.pn.pointer_forward (the imported reference's forward, nn.LSTM and Conv1d included) on a
    state dict of the oracle's: same picks, window logits to float32 rounding."""
    H, T, K, B = 32, 5, 4, 3
    sd = opn.make_state_dict(H, 21, attention=att)
    x = torch.rand(B, T * K, 8, generator=torch.Generator().manual_seed(3))
    _, o_idx, o_logits = opn.pointer_forward(sd, x, T, K, attention=att, n_glimpses=ng)
    emb = torch.nn.functional.linear(x, sd["actor.embedding2.weight"], sd["actor.embedding2.bias"])
    enc = opn._lstm_module(sd, "encoder", H)
    with torch.no_grad():
        enc_out, (h_n, c_n) = enc(emb)
    w = {"enc_out": enc_out, "embedded": emb, "h0": h_n[0], "c0": c_n[0], "start": sd["actor.decoder_start_input"],
         "wih": sd["actor.decoder.weight_ih_l0"], "whh": sd["actor.decoder.weight_hh_l0"], "bih": sd["actor.decoder.bias_ih_l0"],
         "bhh": sd["actor.decoder.bias_hh_l0"], "latent": None}
    bah = att == "Bahdanau"
    if bah:
        for tag, mod in (("p", "pointer"), ("g", "glimpse")):
            w[f"{tag}_wq"], w[f"{tag}_bq"] = sd[f"actor.{mod}.W_query.weight"], sd[f"actor.{mod}.W_query.bias"]
            w[f"{tag}_v"] = sd[f"actor.{mod}.V"]
            w[f"{tag}_ref"] = torch.nn.functional.linear(enc_out, sd[f"actor.{mod}.W_ref.weight"].squeeze(2), sd[f"actor.{mod}.W_ref.bias"])
    c = adr.Case("oracle", H, B, T, K, bah, ng, 1, 10.0, False, None, 0)
    r = adr.replay(w, c, adr.F32)
    assert torch.equal(r["idx"], torch.stack(o_idx, 1))
    for k in range(T):
        want = o_logits[k][:, k * K:(k + 1) * K]
        assert float((r["z0"][:, k] - want).abs().max()) < 1e-4


@pytest.mark.parametrize("c", adr.FIRST_MAX_CASES, ids=[c.id for c in adr.FIRST_MAX_CASES])
def test_attention_decode_tie_cases_are_ties(c):
    """The windows of test_attention_decode_first_maximum_on_equal_rows: equal rows and latents where they are meant to be, the pair
    the float64 maximum of its window by more than 2 eps, and the float64 path through the first of the equals."""
    w = adr.equal_rows_inputs(c)
    K = c.K
    r64 = adr.replay(w, c, adr.D)
    eps = adr.allowance(r64, adr.replay(w, c, adr.F32, idx=r64["idx"]))
    e = w["enc_out"][:, adr.EQUAL_WINDOW * K:(adr.EQUAL_WINDOW + 1) * K]
    assert bool((e == e[:, :1]).all()) and bool((w["latent"][:, adr.EQUAL_WINDOW] == w["latent"][:, adr.EQUAL_WINDOW, :1]).all())
    a, b = (w["enc_out"][:, adr.PAIR_WINDOW * K + r] for r in adr.PAIR)
    assert torch.equal(a, b)
    others = [r for r in range(K) if r not in adr.PAIR]
    assert not bool((w["enc_out"][:, adr.PAIR_WINDOW * K:(adr.PAIR_WINDOW + 1) * K][:, others] == a.unsqueeze(1)).all(2).any())
    assert float(adr.pair_margin(r64).min()) > 2 * eps
    assert torch.equal(r64["z"][:, adr.PAIR_WINDOW, adr.PAIR[0]], r64["z"][:, adr.PAIR_WINDOW, adr.PAIR[1]])
    assert bool((r64["idx"][:, adr.PAIR_WINDOW] == adr.PAIR_WINDOW * K + adr.PAIR[0]).all())
    assert bool((r64["idx"][:, adr.EQUAL_WINDOW] == adr.EQUAL_WINDOW * K).all())
