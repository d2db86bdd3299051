"""-m gpu: the pointer-network mirror (CombinatorialRL / two_level_greedy) against the golden
vectors produced by the imported reference (tests/golden/pn_*.npz) and against the oracle."""
import numpy as np
import pytest
import torch

import attn_decode_reference as adr
from conftest import golden
from oracle import pn as opn
from parity import LOGIT_ATOL, R_ATOL, assert_index_parity, assert_R_parity, prefix_parity, robust_problems

pytestmark = pytest.mark.gpu


def build(fx_or_cfg, dev):
    from gnnpn_sc_amd.modelPN import CombinatorialRL, reward
    H, T, K = int(fx_or_cfg["hidden"]), int(fx_or_cfg["n_cat"]), int(fx_or_cfg["n_per"])
    nets = []
    for level, seed in (("Low", int(fx_or_cfg["seed_low"])), ("High", int(fx_or_cfg["seed_high"]))):
        m = CombinatorialRL(0, H, T * K, 0, 10, 1, reward, "Dot", K, T, use_cuda=True, level=level)
        m.load_state_dict(opn.make_state_dict(H, seed), strict=True)
        nets.append(m.to(dev).eval())
    return nets


@pytest.mark.parametrize("name,precision", [("small", "f32"), ("dummy", "f32"), ("qws", "f32"), ("normal", "f32"),
                                            ("qws", "split"), ("normal", "split")])
def test_two_level_greedy_golden(dev, name, precision):
    """precision="split" (the recurrent products from exact three-piece fp16 operands, fp32 accumulate) is held to
    exactly the same bar against the reference's golden vectors as the fp32 path."""
    from gnnpn_sc_amd.modelPN import two_level_greedy
    fx = golden(f"pn_{name}.npz")
    low, high = build(fx, dev)
    x = torch.from_numpy(fx["inputs"]).to(dev)
    out = two_level_greedy(low, high, x, precision=precision)
    robust = robust_problems(fx["margin_low"], fx["margin_high"])
    same_low = assert_index_parity(out["idx_low"], fx["idx_low"], robust, f"{name}/low", 0.7, fx["inputs"])
    same = assert_index_parity(out["idx_high"], fx["idx_high"], robust, f"{name}/high", 0.7, fx["inputs"]) & same_low
    assert bool(robust.any()), "fixture has no robust problem"
    # on problems whose picks agree the float outputs must agree within tolerance
    s = same.numpy()
    assert np.abs(out["win_low"].cpu().numpy()[s] - fx["win_low"][s]).max() < LOGIT_ATOL
    win_high = (out["win_high_raw"] + out["win_low"]).cpu().numpy()
    assert np.abs(win_high[s] - fx["win_high"][s]).max() < LOGIT_ATOL
    assert np.abs(out["R"].cpu().numpy()[s] - fx["R"][s]).max() <= R_ATOL
    assert np.array_equal(out["actions"].cpu().numpy()[s], fx["actions"][s])
    assert np.abs(out["action_probs"].cpu().numpy()[s] - fx["action_probs"][s]).max() < 1e-4


@pytest.mark.parametrize("name", ["dot_g1_small", "bahdanau_g0_small", "bahdanau_g2_small", "dot_g1_qws", "bahdanau_g1_qws"])
def test_attention_forms_golden(dev, name):
    """'Bahdanau' attention and glimpse rounds (gnnpn_pointer_decode_attn_f32) against fixtures the real
    modelPN.py produced with those switches on; same bar as the shipped configuration (per-decision margins)."""
    from conftest import record_agreement
    from gnnpn_sc_amd.modelPN import CombinatorialRL, reward, two_level_greedy
    fx = golden(f"pn_attn_{name}.npz")
    H, T, K = int(fx["hidden"]), int(fx["n_cat"]), int(fx["n_per"])
    att, ng = str(fx["attention"]), int(fx["n_glimpses"])
    nets = []
    for level, seed in (("Low", int(fx["seed_low"])), ("High", int(fx["seed_high"]))):
        m = CombinatorialRL(0, H, T * K, ng, 10, 1, reward, att, K, T, use_cuda=True, level=level)
        m.load_state_dict(opn.make_state_dict(H, seed, attention=att), strict=True)
        nets.append(m.to(dev).eval())
    x = torch.from_numpy(fx["inputs"]).to(dev)
    out = two_level_greedy(nets[0], nets[1], x)
    rec = prefix_parity(out["idx_low"], out["idx_high"], fx, f"attn/{name}", rows=fx["inputs"])
    s = rec["same_mask"]
    assert s.sum() >= 0.7 * len(s), rec
    assert np.abs(out["win_low"].cpu().numpy()[s] - fx["win_low"][s]).max() < LOGIT_ATOL
    win_high = (out["win_high_raw"] + out["win_low"]).cpu().numpy()
    assert np.abs(win_high[s] - fx["win_high"][s]).max() < LOGIT_ATOL
    assert_R_parity(out["R"], fx["R"], f"attn/{name}", mask=s)
    assert np.array_equal(out["actions"].cpu().numpy()[s], fx["actions"][s])
    assert np.abs(out["action_probs"].cpu().numpy()[s] - fx["action_probs"][s]).max() < 1e-4
    rec.update(attention=att, n_glimpses=ng)
    record_agreement(f"attention_forms/{name}", rec)
    # reference-style calls give the same picks (CombinatorialRL.forward, Low "SL" -> latent -> High)
    _, _, _, idx_l, latent = nets[0](x, None, sample="greedy", training="SL")
    R, _, _, idx_h, _ = nets[1](x, None, latent, sample="greedy")
    assert torch.equal(torch.stack(idx_l, 1).int(), out["idx_low"]) and torch.equal(torch.stack(idx_h, 1).int(), out["idx_high"])
    assert torch.equal(R, out["R"])
    # the returned logits (modelPN.py:239) of these forms, materialised on demand (round 5: used to raise): full length, -inf at the
    # positions chosen before the step (:165-173), against the oracle's on the problems whose Low picks equal the oracle's
    sd_low = opn.make_state_dict(H, int(fx["seed_low"]), attention=att)
    _, o_idx, o_logits = opn.pointer_forward(sd_low, x.cpu(), T, K, attention=att, n_glimpses=ng)
    eq = (torch.stack(idx_l, 1).cpu() == torch.stack(o_idx, 1)).all(1)
    for k in (0, 1, T - 1):
        mine, want = latent[k].cpu(), o_logits[k]
        assert mine.shape == want.shape == (x.shape[0], T * K)
        assert torch.equal(torch.isinf(mine)[eq], torch.isinf(want)[eq]) and int(torch.isinf(want[eq]).sum()) == k * int(eq.sum())
        fin = ~torch.isinf(want)
        assert float((mine - want)[eq][fin[eq]].abs().max()) < LOGIT_ATOL, (name, k)
    if H == 256:
        # round 5: a non-fp32 precision with the general attention forms = that arithmetic in the L-step ENCODER recurrences (the
        # cooperative encoder), fp32 in the general decode kernel — against the same reference fixture, by the same rule
        for prec in ("split", "f16"):
            o2 = two_level_greedy(nets[0], nets[1], x, precision=prec)
            r2 = prefix_parity(o2["idx_low"], o2["idx_high"], fx, f"attn/{name}/{prec}", rows=fx["inputs"])
            s2 = r2["same_mask"]
            assert s2.sum() >= 0.7 * len(s2), r2
            assert np.abs(o2["win_low"].cpu().numpy()[s2] - fx["win_low"][s2]).max() < (LOGIT_ATOL if prec == "split" else 5e-3)
            assert_R_parity(o2["R"], fx["R"], f"attn/{name}/{prec}", mask=s2)
            record_agreement(f"attention_forms/{name}_{prec}_encoder", {k: v for k, v in r2.items()})


@pytest.mark.parametrize("name", ["bahdanau_g1_small", "dot_g2_small", "embed_small", "bahdanau_g1_qws", "embed_qws"])
def test_sampled_attention_and_embedding_forms_golden(dev, name):
    """The sampling mode (modelPN.py:227-228) combined with 'Bahdanau' attention, glimpse rounds and the category embedding
    (:183-188,208-211): the general decode kernel (gnnpn_pointer_decode_attn_f32) and the streaming decoder draw every High pick
    from the window softmax out of the counter-based stream — against fixtures the REAL modelPN.py produced in that mode with
    Tensor.multinomial routed to the same stream.  Picks identical up to a problem's first fragile decision (a Low near-tie or a
    draw within 1e-5 of a cdf boundary), action rows (with the category column) identical, action_probs within 1e-5, R."""
    from conftest import record_agreement
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.modelPN import CombinatorialRL, reward, two_level_greedy
    from parity import TAU_DRAW
    fx = golden(f"pn_sample_{name}.npz")
    H, T, K, B, E = int(fx["hidden"]), int(fx["n_cat"]), int(fx["n_per"]), int(fx["B"]), int(fx["embedding_size"])
    att, ng, seed = str(fx["attention"]), int(fx["n_glimpses"]), int(fx["sample_seed"])
    nets = []
    for level, sd_seed in (("Low", int(fx["seed_low"])), ("High", int(fx["seed_high"]))):
        m = CombinatorialRL(E, H, T * K, ng, 10, 1, reward, att, K, T, use_cuda=True, level=level)
        m.load_state_dict(opn.make_state_dict(H, sd_seed, attention=att, embedding_size=E, n_cat=T), strict=True)
        nets.append(m.to(dev).eval())
    x = torch.from_numpy(fx["inputs"]).to(dev)
    out = two_level_greedy(nets[0], nets[1], x, sample_high_seed=seed)
    ops.check_status(dev)
    rec = prefix_parity(out["idx_low"], out["idx_high"], fx, f"sample/{name}", fx["inputs"][:, :, -8:], tau_high=TAU_DRAW)
    s = rec["same_mask"]
    assert rec["identical_problems"] >= B - 2 and rec["robust_identical"] == rec["robust_problems"] > 0, rec
    assert np.abs(out["action_probs"].cpu().numpy()[s] - fx["action_probs"][s]).max() < 1e-5
    assert np.array_equal(out["actions"].cpu().numpy()[s], fx["actions"][s])
    assert_R_parity(out["R"], fx["R"], f"sample/{name}", s)
    rec.update(attention=att, n_glimpses=ng, embedding_size=E)
    record_agreement(f"sampled_forms/{name}", rec)
    greedy = two_level_greedy(nets[0], nets[1], x)
    assert float((greedy["idx_high"] != out["idx_high"]).float().mean()) > 0.3          # the draws are not the argmax
    # the reference's own entry point, default sample="sample": a function of (sample_seed, call number) of the actor
    _, _, _, _, latent = nets[0](x, None, sample="greedy", training="SL")
    nets[1].actor.sample_seed, nets[1].actor.sample_calls = 9, 0
    R1, probs1, _, idx1, _ = nets[1](x, None, latent)
    nets[1].actor.sample_calls = 0
    R2, probs2, _, idx2, _ = nets[1](x, None, latent)
    assert torch.equal(torch.stack(idx1), torch.stack(idx2)) and torch.equal(R1, R2) and torch.equal(torch.stack(probs1), torch.stack(probs2))
    p = torch.stack(probs1, 1)
    assert bool(((p > 0) & (p <= 1)).all())


@pytest.mark.parametrize("name", ["small", "qws"])
def test_category_embedding_golden(dev, name):
    """embedding_size != 0 (embeddingTag=1; modelPN.py:153-154,183-188): rows [category | 8 floats], the category embedded and
    concatenated in front of embedding2 (gnnpn_embed_concat_f32 + the literal two-stage input side), against fixtures the
    real modelPN.py produced — picks by the per-decision rule, action rows WITH their category column, R, logits."""
    from conftest import record_agreement
    from gnnpn_sc_amd.modelPN import CombinatorialRL, reward, two_level_greedy
    fx = golden(f"pn_embed_{name}.npz")
    H, T, K, E = int(fx["hidden"]), int(fx["n_cat"]), int(fx["n_per"]), int(fx["embedding_size"])
    nets = []
    for level, seed in (("Low", int(fx["seed_low"])), ("High", int(fx["seed_high"]))):
        m = CombinatorialRL(E, H, T * K, 0, 10, 1, reward, "Dot", K, T, use_cuda=True, level=level)
        m.load_state_dict(opn.make_state_dict(H, seed, embedding_size=E, n_cat=T), strict=True)
        nets.append(m.to(dev).eval())
    x = torch.from_numpy(fx["inputs"]).to(dev)
    out = two_level_greedy(nets[0], nets[1], x)
    rec = prefix_parity(out["idx_low"], out["idx_high"], fx, f"embed/{name}", rows=fx["inputs"])
    s = rec["same_mask"]
    assert s.sum() >= 0.7 * len(s), rec
    assert np.abs(out["win_low"].cpu().numpy()[s] - fx["win_low"][s]).max() < LOGIT_ATOL
    assert np.abs((out["win_high_raw"] + out["win_low"]).cpu().numpy()[s] - fx["win_high"][s]).max() < LOGIT_ATOL
    assert_R_parity(out["R"], fx["R"], f"embed/{name}", mask=s)
    assert out["actions"].shape[2] == 9 and np.array_equal(out["actions"].cpu().numpy()[s], fx["actions"][s])
    record_agreement(f"category_embedding/{name}", rec)
    # reference-style calls (CombinatorialRL.forward, Low "SL" -> latent -> High) give the same picks and reward
    _, _, _, idx_l, latent = nets[0](x, None, sample="greedy", training="SL")
    R, _, actions, idx_h, _ = nets[1](x, None, latent, sample="greedy")
    assert torch.equal(torch.stack(idx_l, 1).int(), out["idx_low"]) and torch.equal(torch.stack(idx_h, 1).int(), out["idx_high"])
    assert torch.equal(R, out["R"]) and actions[0].shape == (x.shape[0], 9)
    if H == 256:      # the category embedding with the exact-split encoder (pregates form of the cooperative encoder), fp32 decoder
        o2 = two_level_greedy(nets[0], nets[1], x, precision="split")
        r2 = prefix_parity(o2["idx_low"], o2["idx_high"], fx, f"embed/{name}/split", rows=fx["inputs"])
        s2 = r2["same_mask"]
        assert s2.sum() >= 0.7 * len(s2), r2
        assert np.abs(o2["win_low"].cpu().numpy()[s2] - fx["win_low"][s2]).max() < LOGIT_ATOL
        assert_R_parity(o2["R"], fx["R"], f"embed/{name}/split", mask=s2)
        record_agreement(f"category_embedding/{name}_split_encoder", r2)


def test_general_kernel_on_the_shipped_configuration_equals_the_streaming_decoder(dev):
    """'Dot' without glimpses through the general kernel is the streaming decoder's arithmetic: same picks, same window
    logits bit for bit (the two kernels share the cell, the dot order and the argmax rule)."""
    from gnnpn_sc_amd import ops
    fx = golden("pn_qws.npz")
    low, high = build(fx, dev)
    x = torch.from_numpy(fx["inputs"]).to(dev)
    T, K = int(fx["n_cat"]), int(fx["n_per"])
    a = low.actor
    enc_args, embedded = a.encode_args(x, fold=False)
    enc, h_n, c_n = ops.lstm_encode([enc_args])
    d = a.decode_args(embedded, enc[0], h_n[0], c_n[0], fold=False)
    ref = ops.pointer_decode([d], x, T, K, impl=1)[0]
    got = ops.pointer_decode_attn(d, x, T, K, "Dot", 0)
    for key in ("idx", "win_logits", "pick_prob", "actions"):
        assert torch.equal(ref[key], got[key]), key


@pytest.mark.parametrize("name", ["small", "qws"])
def test_reference_style_calls(dev, name):
    """Drive the mirror exactly as trainPNHigh.py:138-139 drives the reference."""
    from gnnpn_sc_amd.modelPN import two_level_greedy
    fx = golden(f"pn_{name}.npz")
    low, high = build(fx, dev)
    x = torch.from_numpy(fx["inputs"]).to(dev)
    T, K = int(fx["n_cat"]), int(fx["n_per"])
    probs_l, aprob_l, actions_l, idx_l, latent = low(x, None, sample="greedy", training="SL")
    R, aprob, actions, idx, latent_h = high(x, None, latent, sample="greedy")
    fused = two_level_greedy(low, high, x)
    assert torch.equal(torch.stack(idx_l, 1).int(), fused["idx_low"])
    assert torch.equal(torch.stack(idx, 1).int(), fused["idx_high"])
    assert torch.equal(R, fused["R"]) and R.dtype == torch.float32 and R.shape == (x.shape[0],)
    assert idx[0].dtype == torch.int64 and len(idx) == T and actions[0].shape == (x.shape[0], 8)
    assert len(latent) == T and len(probs_l) == T
    # the reference's full-length latent (list of [B,L]) works as input too, and gives the same picks
    as_list = [latent[k] for k in range(T)]
    R2, _, _, idx2, _ = high(x, None, as_list, sample="greedy")
    assert torch.equal(torch.stack(idx2, 1), torch.stack(idx, 1)) and torch.equal(R2, R)
    # full-length view of step 1: -inf exactly at the step-0 picks (modelPN.py:172), values as golden
    lat1 = latent[1].cpu()
    same0 = (fused["idx_low"][:, 0].cpu().numpy() == fx["idx_low"][:, 0])
    want = torch.from_numpy(fx["latent_step1"])
    assert torch.equal(torch.isinf(lat1)[same0], torch.isinf(want)[same0])
    fin = ~torch.isinf(want)
    assert float((lat1[fin] - want[fin]).abs().max()) < 5e-4
    p0 = probs_l[0].cpu()
    assert p0.shape == (x.shape[0], T * K) and torch.allclose(p0.sum(1), torch.ones(x.shape[0]), atol=1e-5)
    assert float(p0[:, K:].abs().max()) == 0.0
    low_R = low(x, None, sample="greedy", training="RL")[0].cpu().numpy()
    s = (fused["idx_low"].cpu().numpy() == fx["idx_low"]).all(1)
    assert np.array_equal(low_R[s], fx["R_low"][s])


def test_unsupported_modes_fail_loudly(dev):
    from gnnpn_sc_amd.modelPN import CombinatorialRL, reward
    from gnnpn_sc_amd.modelPN import two_level_greedy
    e = CombinatorialRL(20, 32, 18, 0, 10, 1, reward, "Dot", 3, 6).to(dev)      # the category embedding: greedy and sampled (round 4)
    xe = torch.cat([torch.arange(6.0).repeat_interleave(3).view(1, 18, 1).expand(2, 18, 1), torch.rand(2, 18, 8)], 2).to(dev)
    assert e(xe, None)[2][0].shape == (2, 9)                                    # default sample="sample"
    assert e(xe, None, sample="greedy")[2][0].shape == (2, 9)
    with pytest.raises(NotImplementedError):
        CombinatorialRL(0, 32, 18, 0, 10, 1, reward, "Luong", 3, 6)             # modelPN.py:116-117
    g = CombinatorialRL(0, 32, 18, 1, 10, 1, reward, "Bahdanau", 3, 6).to(dev)  # the general forms: greedy and sampled (round 4)
    assert len(g(torch.rand(2, 18, 8, device=dev), None)[3]) == 6               # default sample="sample"
    from gnnpn_sc_amd import ops
    with pytest.raises(ops.GnnpnError):                                         # a non-fp32 encoder needs the cooperative form (H = 256); at
        two_level_greedy(g, g, torch.rand(2, 18, 8, device=dev), precision="split")   # H = 256 the general forms take it (test_attention_forms_golden)
    m = CombinatorialRL(0, 32, 18, 0, 10, 1, reward, "Dot", 3, 6).to(dev)
    R, probs, actions, idxs, _ = m(torch.rand(2, 18, 8, device=dev), None)   # default sample="sample": the sampling forward
    assert R.shape == (2,) and len(idxs) == 6 and probs[0].shape == (2,)
    with pytest.raises(AssertionError):
        m(torch.rand(2, 17, 8, device=dev), None, sample="greedy")   # seq_len assert (modelPN.py:182)


def test_cpu_tensors_are_rejected(dev):
    """There is no CPU fallback: host tensors raise instead of silently running elsewhere."""
    from gnnpn_sc_amd import ops
    with pytest.raises(ops.GnnpnError):
        ops.linear(torch.rand(4, 8), torch.rand(3, 8))


def test_cpp_operators_validate_their_operands(dev):
    """The C++ operators refuse what the ctypes wrappers refuse: wrong dtype, non-contiguous and host operands, inconsistent
    shapes, a cooperative launch without its workspace — as exceptions, before anything is enqueued."""
    from gnnpn_sc_amd import custom_ops                                        # loads libgnnpn_torch.so: the operators register themselves
    a, w = torch.rand(4, 8, device=dev), torch.rand(3, 8, device=dev)
    assert torch.ops.gnnpn.linear(a, w).shape == (4, 3)
    with pytest.raises(RuntimeError, match="dtype"):
        torch.ops.gnnpn.linear(a.double(), w)
    with pytest.raises(RuntimeError, match="contiguous"):
        torch.ops.gnnpn.linear(torch.rand(8, 4, device=dev).t(), w)
    with pytest.raises(RuntimeError, match="K mismatch"):
        torch.ops.gnnpn.linear(a, torch.rand(3, 7, device=dev))
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.gnnpn.linear(a.cpu(), w.cpu())
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch.ops.gnnpn.linear(a, w, bias=torch.rand(3))                       # one host operand among device ones
    cfg = {"hidden": 256, "n_cat": 3, "n_per": 2, "seed_low": 1, "seed_high": 2}
    low, _ = build(cfg, dev)
    args, _ = low.actor.encode_args(torch.rand(2, 6, 8, device=dev), None)
    flat = [args.get(k) for k in custom_ops.ENCODE_KEYS]
    with pytest.raises(RuntimeError, match="workspace"):
        torch.ops.gnnpn.lstm_encode(flat, 1)                                   # H = 256: the cooperative form needs its workspace
    with pytest.raises(RuntimeError, match="precision"):
        torch.ops.gnnpn.lstm_encode(flat, 1, "bf16")


def test_fresh_oracle_batch(dev):
    """A batch that is not a stored fixture: oracle run live on the CPU vs the HIP path."""
    from gnnpn_sc_amd.modelPN import two_level_greedy
    cfg = {"hidden": 256, "n_cat": 12, "n_per": 4, "seed_low": 101, "seed_high": 102}
    low, high = build(cfg, dev)
    g = torch.Generator().manual_seed(77)
    x = torch.rand(16, 48, 8, generator=g)
    x[:, :, 2:4] = 0.9 + 0.1 * x[:, :, 2:4]
    x[:, 4:, 4:] = 0
    ref = opn.two_level_greedy(opn.make_state_dict(256, 101), opn.make_state_dict(256, 102), x, 12, 4)
    out = two_level_greedy(low, high, x.to(dev))
    robust = robust_problems(ref["margin_low"], ref["margin_high"])
    s = assert_index_parity(out["idx_high"], ref["idx_high"], robust, "fresh/high", 0.8, x) & \
        assert_index_parity(out["idx_low"], ref["idx_low"], robust, "fresh/low", 0.8, x)
    assert float((out["R"].cpu()[s] - ref["R"][s]).abs().max()) <= R_ATOL


@pytest.mark.parametrize("B,T,K", [(1, 3, 1), (17, 1, 4), (16, 6, 3), (40, 47, 5), (256, 47, 5), (300, 12, 10),
                                   (23, 9, 16), (530, 5, 8)])
def test_decode_cooperative_vs_streaming(dev, B, T, K):
    """Cooperative decoder (both nets in one launch, weights in registers, per-step hand-off) vs the
    per-workgroup streaming decoder on the same encoder outputs.  The LSTM cells are the same fma
    chains; only the 256-term attention dots are summed in a different order, so window logits agree
    to ~1e-5 and picks agree wherever the streaming decision margin exceeds that."""
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.modelPN import two_level_greedy
    cfg = {"hidden": 256, "n_cat": T, "n_per": K, "seed_low": 5 + B, "seed_high": 6 + B}
    low, high = build(cfg, dev)
    g = torch.Generator().manual_seed(B * T)
    x = torch.rand(B, T * K, 8, generator=g)
    x[:, :, 2:4] = 0.9 + 0.1 * x[:, :, 2:4]
    x[:, K:, 4:] = 0
    x = x.to(dev)
    ref = two_level_greedy(low, high, x, decode_impl=1)
    out8 = two_level_greedy(low, high, x, decode_impl=2)    # 8-CU groups
    out4 = two_level_greedy(low, high, x, decode_impl=4)    # 8-CU groups, 256-register build (co-resident with another cooperative launch)
    out = out8
    out2 = two_level_greedy(low, high, x, decode_impl=2)
    out3 = two_level_greedy(low, high, x, decode_impl=2, write_through=True)   # the placement-independent hand-off
    ops.check_status(dev)
    for k in ("idx_low", "idx_high", "R", "win_low", "win_high_raw", "actions", "action_probs"):
        assert torch.equal(out[k], out2[k]), k                    # deterministic across launches
        assert torch.equal(out[k], out3[k]), k                    # and across the two hand-off paths
    win_ref = torch.stack([ref["win_low"], ref["win_high_raw"] + ref["win_low"]]).cpu()
    m = opn.decision_margin(win_ref[0], x.cpu()), opn.decision_margin(win_ref[1], x.cpu())
    robust = (m[0] > 1e-3).all(1) & (m[1] > 1e-3).all(1)
    same = assert_index_parity(out["idx_low"], ref["idx_low"], robust, "coop/low", 0.8, x.cpu()) & \
        assert_index_parity(out["idx_high"], ref["idx_high"], robust, "coop/high", 0.8, x.cpu())
    assert bool(robust.any())
    s = same.to(dev)
    assert float((out["win_low"][s] - ref["win_low"][s]).abs().max()) < 1e-4
    assert float((out["win_high_raw"][s] - ref["win_high_raw"][s]).abs().max()) < 1e-4
    assert float((out["R"][s] - ref["R"][s]).abs().max()) <= R_ATOL
    assert float((out["action_probs"][s] - ref["action_probs"][s]).abs().max()) < 1e-4
    s8 = (assert_index_parity(out8["idx_low"], ref["idx_low"], robust, "coop8/low", 0.8, x.cpu()) &
          assert_index_parity(out8["idx_high"], ref["idx_high"], robust, "coop8/high", 0.8, x.cpu())).to(dev)
    assert float((out8["win_low"][s8] - ref["win_low"][s8]).abs().max()) < 1e-4
    assert float((out8["R"][s8] - ref["R"][s8]).abs().max()) <= R_ATOL
    # the pick's probability: the 256-register build forms it in a kernel of its own (pick_prob_kernel, one lane per (problem,
    # step)), the other builds inside the decoder (lane 0 of a 16-lane DPP reduction) — the same tree of sums, so wherever the
    # logits and picks of two builds are the same bits, so are the probabilities
    for other in (out8, out3):
        eq = (out4["idx_high"] == other["idx_high"]).all(1) & (out4["win_high_raw"] == other["win_high_raw"]).flatten(1).all(1) & \
            (out4["win_low"] == other["win_low"]).flatten(1).all(1)
        if K <= 8:
            assert bool(eq.any())
        assert torch.equal(out4["action_probs"][eq], other["action_probs"][eq])
    s4 = (assert_index_parity(out4["idx_low"], ref["idx_low"], robust, "coop8x2/low", 0.8, x.cpu()) &
          assert_index_parity(out4["idx_high"], ref["idx_high"], robust, "coop8x2/high", 0.8, x.cpu())).to(dev)
    assert float((out4["win_low"][s4] - ref["win_low"][s4]).abs().max()) < 1e-4
    assert float((out4["win_high_raw"][s4] - ref["win_high_raw"][s4]).abs().max()) < 1e-4
    assert float((out4["R"][s4] - ref["R"][s4]).abs().max()) <= R_ATOL


@pytest.mark.parametrize("name", ["qws", "normal"])
def test_folded_vs_two_stage_input_projection(dev, name):
    """FOLD_INPUT_PROJECTION (W_ih.W_e as one [4H,8] matrix, evaluated in-kernel) against the literal
    two-stage order of the reference (embedding2, then W_ih): same picks on robust problems, logits
    within the usual tolerance, and both within tolerance of the golden vectors."""
    from gnnpn_sc_amd.modelPN import two_level_greedy
    fx = golden(f"pn_{name}.npz")
    low, high = build(fx, dev)
    x = torch.from_numpy(fx["inputs"]).to(dev)
    a = two_level_greedy(low, high, x, fold=True)
    b = two_level_greedy(low, high, x, fold=False)
    robust = robust_problems(fx["margin_low"], fx["margin_high"])
    for out, tag in ((a, "fold"), (b, "two-stage")):
        s = assert_index_parity(out["idx_high"], fx["idx_high"], robust, f"{name}/{tag}", 0.7, fx["inputs"]).numpy() & \
            assert_index_parity(out["idx_low"], fx["idx_low"], robust, f"{name}/{tag}", 0.7, fx["inputs"]).numpy()
        assert np.abs(out["win_low"].cpu().numpy()[s] - fx["win_low"][s]).max() < LOGIT_ATOL
    same = ((a["idx_low"] == b["idx_low"]).all(1) & (a["idx_high"] == b["idx_high"]).all(1))
    assert float((a["win_low"][same] - b["win_low"][same]).abs().max()) < LOGIT_ATOL
    # High sampled on the two-stage input side: the general cooperative decoder has no such build and refuses the call before it
    # books any work, so the auto choice (impl 0) falls through to the streaming form with the proof of work intact
    from gnnpn_sc_amd import ops
    ws = ops.new_workspaces(dev)
    auto = two_level_greedy(low, high, x, fold=False, sample_high_seed=7, ws=ws)
    ws.check()
    streaming = two_level_greedy(low, high, x, fold=False, sample_high_seed=7, decode_impl=1, ws=ops.new_workspaces(dev))
    for key in ("idx_low", "idx_high", "actions", "action_probs"):
        assert torch.equal(auto[key], streaming[key]), key


def test_saturated_logits_first_max_wins(dev):
    """10*tanh(x) rounds to exactly 10.0f once |x| is large: exact ties inside a window, which torch.max
    (CPU) resolves to the FIRST maximum.  Fixture pn_saturated (recurrent weights x6, generated by the
    reference) has such ties; both cooperative decoder forms and the streaming form must make the same
    pick wherever they see the same tie."""
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.modelPN import CombinatorialRL, reward, two_level_greedy
    fx = golden("pn_saturated.npz")
    H, T, K = int(fx["hidden"]), int(fx["n_cat"]), int(fx["n_per"])
    nets = []
    for level, seed in (("Low", int(fx["seed_low"])), ("High", int(fx["seed_high"]))):
        sd = opn.make_state_dict(H, seed)
        for k in sd:
            if "encoder" in k or "decoder." in k:
                sd[k] = sd[k] * float(fx["weight_scale"])
        m = CombinatorialRL(0, H, T * K, 0, 10, 1, reward, "Dot", K, T, level=level)
        m.load_state_dict(sd)
        nets.append(m.to(dev).eval())
    x = torch.from_numpy(fx["inputs"]).to(dev)
    ties_checked = 0
    for impl in (1, 2):
        out = two_level_greedy(nets[0], nets[1], x, fold=False, decode_impl=impl)   # literal two-stage order: closest to the fixture
        got_low, win = out["idx_low"].cpu().numpy(), out["win_low"].cpu().numpy()
        for b in range(x.shape[0]):
            for t in range(T):
                if (got_low[b, :t] != fx["idx_low"][b, :t]).any():
                    break                                           # history diverged: later steps not comparable
                w_ref, w_got = fx["win_low"][b, t], win[b, t]
                top = w_ref.max()
                if (w_ref == top).sum() >= 2 and (w_got == w_got.max()).sum() >= 2 and \
                        np.array_equal(w_got == w_got.max(), w_ref == top):
                    assert got_low[b, t] == fx["idx_low"][b, t] == t * K + int(np.argmax(w_ref == top))
                    ties_checked += 1
    assert ties_checked >= 3, f"only {ties_checked} exact ties were comparable"


def test_all_dummy_problem_gives_nan_reward_like_numpy(dev):
    """A problem whose every action is a dummy row has no real service: the reference divides by zero
    (modelPN.py:29, numpy float32 -> nan, and round(nan) stays nan); so does the kernel."""
    from gnnpn_sc_amd import ops
    act = torch.zeros(2, 4, 8)
    act[:, :, 0:4] = torch.tensor([0.0, 1.0, 1.0, 1.0])
    act[1, 2, 0] = 0.3                                   # second problem has one real service
    act[:, 0, 4:8] = torch.tensor([0.5, 1.0, 0.5, 1.0])
    want = opn.reward([act[:, t] for t in range(4)], "High")
    got = ops.qos_reward(act.to(dev), "High").cpu()
    assert torch.isnan(want[0]) and torch.isnan(got[0])
    assert abs(float(got[1]) - float(want[1])) <= R_ATOL


def test_fp16_encoder_option_agreement(dev):
    """Opt-in reduced precision (BASELINE configs[4]): fp16 operands in the encoder's recurrent product.
    Not parity-exact by design; gate = encoder outputs within 5e-3 of the fp32 path and >= 99 % of the
    decisions identical on a QWS-shaped batch (measured: 99.9 %, 96-98 % of problems fully identical)."""
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.modelPN import two_level_greedy
    cfg = {"hidden": 256, "n_cat": 47, "n_per": 5, "seed_low": 3, "seed_high": 4}
    low, high = build(cfg, dev)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(64, 235, 8, generator=g)
    x[:, :, 2:4] = 0.9 + 0.1 * x[:, :, 2:4]
    x[:, 5:, 4:] = 0
    x = x.to(dev)
    a = two_level_greedy(low, high, x)
    b = two_level_greedy(low, high, x, precision="f16")
    c = two_level_greedy(low, high, x)                         # the option does not leak into later calls
    ops.check_status(dev)
    assert torch.equal(a["idx_high"], c["idx_high"]) and torch.equal(a["R"], c["R"])
    assert float((a["idx_high"] == b["idx_high"]).float().mean()) >= 0.99
    assert float((a["idx_low"] == b["idx_low"]).float().mean()) >= 0.99
    enc_args, _ = low.actor.encode_args(x)
    e32 = ops.lstm_encode([enc_args])[0][0]
    e16 = ops.lstm_encode([enc_args], precision="f16")[0][0]
    assert 0 < float((e32 - e16).abs().max()) < 5e-3


def test_split_encoder_matches_fp32_accuracy(dev):
    """The split-operand encoder against an fp64 LSTM: its error must not exceed the fp32 chain's by more than
    a rounding or two (measured: 9.5e-8 vs 1.07e-7 max, 7.8e-9 vs 8.6e-9 mean at QWS shape), and the two paths
    must agree to 1e-6 and pick identically."""
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.modelPN import two_level_greedy
    cfg = {"hidden": 256, "n_cat": 47, "n_per": 5, "seed_low": 3, "seed_high": 4}
    low, high = build(cfg, dev)
    g = torch.Generator().manual_seed(6)
    x = torch.rand(32, 235, 8, generator=g)
    x[:, :, 2:4] = 0.9 + 0.1 * x[:, :, 2:4]
    x[:, 5:, 4:] = 0
    sd = {k: v.detach().cpu().double() for k, v in low.state_dict().items()}
    emb = x.double() @ sd["actor.embedding2.weight"].T + sd["actor.embedding2.bias"]
    lstm = torch.nn.LSTM(256, 256, batch_first=True).double()
    lstm.load_state_dict({k.replace("actor.encoder.", ""): v for k, v in sd.items() if k.startswith("actor.encoder.")})
    with torch.no_grad():
        ref, _ = lstm(emb)
    xd = x.to(dev)
    enc_args, _ = low.actor.encode_args(xd)
    e32 = ops.lstm_encode([enc_args])[0][0]
    esp = ops.lstm_encode([enc_args], precision="split")[0][0]
    ops.check_status(dev)
    err32 = (e32.double().cpu() - ref).abs()
    errsp = (esp.double().cpu() - ref).abs()
    assert float(errsp.max()) < 2 * float(err32.max()) + 1e-8 and float(errsp.max()) < 5e-7
    assert float(errsp.mean()) < 1.5 * float(err32.mean()) + 1e-10
    assert float((e32 - esp).abs().max()) < 1e-6
    a = two_level_greedy(low, high, xd)
    b = two_level_greedy(low, high, xd, precision="split")
    same = (a["actions"] == b["actions"]).all(-1).all(1)
    assert bool(same.all())                                            # measured: 32 of 32 (floor was 0.95)
    s = same.cpu()
    assert float((a["R"] - b["R"]).abs()[s].max()) <= R_ATOL


@pytest.mark.parametrize("B,T,K", [(1, 3, 1), (17, 1, 4), (40, 47, 5), (300, 12, 10), (23, 9, 16)])
def test_split_precision_ragged_shapes(dev, B, T, K):
    """precision="split" in both cooperative decoder forms and the encoder on ragged shapes (batch not a multiple
    of the 16-problem tile, one category, one candidate, K = 16): window logits within 1e-5 of the fp32 path, picks
    identical wherever the fp32 decision margin exceeds 1e-4, and deterministic across launches."""
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.modelPN import two_level_greedy
    cfg = {"hidden": 256, "n_cat": T, "n_per": K, "seed_low": 15 + B, "seed_high": 16 + B}
    low, high = build(cfg, dev)
    g = torch.Generator().manual_seed(B * T + 1)
    x = torch.rand(B, T * K, 8, generator=g)
    x[:, :, 2:4] = 0.9 + 0.1 * x[:, :, 2:4]
    x[:, K:, 4:] = 0
    x = x.to(dev)
    ref = two_level_greedy(low, high, x)
    outs = [two_level_greedy(low, high, x, precision="split", decode_impl=impl) for impl in (2, 2, 2, 4)]
    ops.check_status(dev)
    for k in ("idx_low", "idx_high", "R", "win_low", "win_high_raw", "actions"):
        assert torch.equal(outs[1][k], outs[2][k]), k
    win_ref = torch.stack([ref["win_low"], ref["win_high_raw"] + ref["win_low"]]).cpu()
    m = opn.decision_margin(win_ref[0], x.cpu()), opn.decision_margin(win_ref[1], x.cpu())
    robust = (m[0] > 1e-4).all(1) & (m[1] > 1e-4).all(1)
    for tag, out in (("split8", outs[0]), ("split8x2", outs[3])):
        same = assert_index_parity(out["idx_low"], ref["idx_low"], robust, tag + "/low", 0.8, x.cpu()) & \
            assert_index_parity(out["idx_high"], ref["idx_high"], robust, tag + "/high", 0.8, x.cpu())
        s = same.to(dev)
        if bool(s.any()):
            assert float((out["win_low"][s] - ref["win_low"][s]).abs().max()) < 1e-5
            assert float((out["win_high_raw"][s] - ref["win_high_raw"][s]).abs().max()) < 1e-5
            assert float((out["R"][s] - ref["R"][s]).abs().max()) <= R_ATOL


@pytest.mark.parametrize("B,T,K", [(40, 47, 5), (17, 9, 16)])
def test_presplit_weights_change_nothing(dev, B, T, K):
    """The recurrent weights split ONCE per model (ops.pack_lstm_split_weights -> whh_split of the nets, ABI 9) against the split
    every "split" launch makes for itself when it is absent: the packed image is written by the same device function, so every
    output of the encoder and of both cooperative decoder builds is bit-identical with and without it — and the image itself holds,
    per lane, pieces that sum to the fp32 weight (spot check through gnnpn_recurrent_product's col_inv is test_split3's; here: the
    two paths agree on everything they produce)."""
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.modelPN import two_level_greedy
    cfg = {"hidden": 256, "n_cat": T, "n_per": K, "seed_low": 115 + B, "seed_high": 116 + B}
    low, high = build(cfg, dev)
    g = torch.Generator().manual_seed(B * T + 7)
    x = torch.rand(B, T * K, 8, generator=g)
    x[:, :, 2:4] = 0.9 + 0.1 * x[:, :, 2:4]
    x = x.to(dev)
    for m in (low, high):
        w = m.actor.packed()
        assert w["enc_whh_split"].numel() == w["dec_whh_split"].numel() == 8 * 10368 * 16 and w["enc_whh_split"].dtype == torch.uint8
    with_split = [two_level_greedy(low, high, x, precision="split", decode_impl=impl) for impl in (2, 4)]
    for m in (low, high):                                                # the same weights without the packed image: split in the kernels
        m.actor.packed().pop("enc_whh_split")
        m.actor.packed().pop("dec_whh_split")
    without = [two_level_greedy(low, high, x, precision="split", decode_impl=impl) for impl in (2, 4)]
    ops.check_status(dev)
    for a, b in zip(with_split, without):
        for k in ("idx_low", "idx_high", "R", "win_low", "win_high_raw", "actions"):
            assert torch.equal(a[k], b[k]), k
    # the encoder alone, enc_out / h_n / c_n bit for bit
    args = low.actor.encode_args(x)[0]
    assert args.get("whh_split") is None
    e0, h0, c0 = ops.lstm_encode([args], precision="split")
    args2 = dict(args, whh_split=ops.pack_lstm_split_weights(args["whh"]))
    e1, h1, c1 = ops.lstm_encode([args2], precision="split")
    ops.check_status(dev)
    assert torch.equal(e0[0], e1[0]) and torch.equal(h0[0], h1[0]) and torch.equal(c0[0], c1[0])
    with pytest.raises(ops.GnnpnError):
        ops.pack_lstm_split_weights(torch.zeros(8, 4, 32, 4, device=dev))   # H = 32: the cooperative kernels are built for H = 256


def test_split_precision_needs_the_cooperative_form(dev):
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.modelPN import two_level_greedy
    cfg = {"hidden": 32, "n_cat": 4, "n_per": 3, "seed_low": 1, "seed_high": 2}
    low, high = build(cfg, dev)
    x = torch.rand(3, 12, 8).to(dev)
    with pytest.raises(ops.GnnpnError):
        two_level_greedy(low, high, x, precision="split")
    two_level_greedy(low, high, x)                     # and the failed call left no option behind
    ops.check_status(dev)


def test_a_launch_on_a_dirty_workspace_is_loud(dev):
    """coop_place's check that the status area was clean when the launch began (status code 8): with the per-launch zeroing
    switched off (test hook: GNNPN_ABLATE_KEEP_WORKSPACE) a second encoder launch on the same workspace finds the first one's seat and
    arrival counters — every workgroup would leave as surplus and the outputs would be garbage with nothing timing out; instead the
    launch's own word and the sticky word carry code 8 and ops.check_status raises.  (Seen for real: DESIGN.md section 4.4; profiles/LOG_r01_r04.md section 13.3.)"""
    from gnnpn_sc_amd import custom_ops, ops
    cfg = {"hidden": 256, "n_cat": 6, "n_per": 4, "seed_low": 1, "seed_high": 2}
    low, high = build(cfg, dev)
    x = torch.rand(32, 24, 8).to(dev)
    ws = ops.new_workspaces(dev)
    args, _ = low.actor.encode_args(x, None)
    enc0 = custom_ops.lstm_encode([args], ws=ws)[0][0].clone()
    ws.check()
    try:
        ops.set_option("lstm_ablate", ops.GNNPN_ABLATE_KEEP_WORKSPACE)
        custom_ops.lstm_encode([args], ws=ws)
        torch.cuda.synchronize()
        assert int(ws._encode[:4].view(torch.int32).item()) & 8 and int(ws.status[0].item()) & 8
        with pytest.raises(ops.GnnpnError, match="not clean"):
            ws.check()
    finally:
        ops.set_option("lstm_ablate", 0)
    assert torch.equal(custom_ops.lstm_encode([args], ws=ws)[0][0], enc0)       # and the next ordinary launch is fine again
    ws.check()


# ---- proof of work (round 5): a cooperative launch that did not do its work cannot pass a check ------------------------------
# layout of a workspace's status area in 32-bit words (csrc/coop_common.h, named in ops): 0 the launch's error word, 4 staffing
# state, 5 XCDs whose seats are all taken, 512.. CU claim statistics, then from COOP_TAKEN_OFFSET the seat flags (64 per XCD), and
# from COOP_XCDCNT_OFFSET / COOP_ARRIVE_OFFSET the seats taken / arrivals per XCD, one counter every COOP_XCD_STRIDE words
def _poison(kind, words, gen):
    """Patterns for the status area of a workspace that the launch then does NOT zero (test hook).  The first two are what the
    failure record of round 4 showed (profiles/r04_handoff_timeouts_on_some_boxes.jsonl): the PREVIOUS launch's totals."""
    from gnnpn_sc_amd import ops
    cnt, arr, taken, stride = ops.COOP_XCDCNT_OFFSET // 4, ops.COOP_ARRIVE_OFFSET // 4, ops.COOP_TAKEN_OFFSET // 4, ops.COOP_XCD_STRIDE
    p = torch.zeros(words, dtype=torch.int32)
    if kind in ("previous_totals", "previous_totals_some_xcds"):
        xcds = range(8) if kind == "previous_totals" else (1, 4, 6)
        for x in xcds:
            p[cnt + stride * x] = 32              # the XCD's 32 seats taken
            p[arr + stride * x] = 96              # every workgroup of the 3 x over-subscribed launch arrived
            p[taken + 64 * x:taken + 64 * x + 32] = 1
        p[4], p[5] = 2, len(list(xcds))          # "staffed", XCDs complete
    elif kind == "seat_counters_only":
        p[cnt:cnt + 8 * stride:stride] = 32
    elif kind == "seat_flags_only":
        p[taken:taken + 8 * 64:3] = 1            # every third seat looks taken: those members can never be seated
    elif kind == "staffing_word":
        p[4] = 1
    elif kind == "random_dense":
        p = torch.randint(-2**31, 2**31 - 1, (words,), generator=gen, dtype=torch.int64).to(torch.int32)
    elif kind == "random_sparse":
        idx = torch.randint(0, words, (40,), generator=gen)
        p[idx] = torch.randint(1, 200, (40,), generator=gen, dtype=torch.int64).to(torch.int32)
    else:
        raise KeyError(kind)
    return p


POISONS = ["previous_totals", "previous_totals_some_xcds", "seat_counters_only", "seat_flags_only", "staffing_word", "random_dense",
           "random_sparse"]


@pytest.mark.parametrize("kind", POISONS)
@pytest.mark.parametrize("which", ["encoder", "decoder"])
def test_poisoned_status_area_ends_loud_or_correct(dev, which, kind):
    """The silent failure of round 4: a launch that began on the previous launch's seat counters — every workgroup left as
    surplus, nothing ran, nothing timed out, status 0, outputs garbage.  Now every seated workgroup adds the tiles it FINISHED to
    the caller's status block and the launch books the tiles it is EXPECTED to finish (include/gnnpn_hip.h, GNNPN_STATUS_*);
    ``Workspaces.poll`` compares them (and the host's own count of the launches it made).  Whatever the status area holds when
    a launch begins — the previous launch's totals, on all XCDs or some; stale flags; random words — the launch ends in a
    CORRECT result or a NON-ZERO status, never in silence.  QWS-sized batch (32 seats per XCD, as in the failure record)."""
    from gnnpn_sc_amd import _lib, custom_ops, ops
    T, K, B = 6, 4, 256
    cfg = {"hidden": 256, "n_cat": T, "n_per": K, "seed_low": 1, "seed_high": 2}
    low, high = build(cfg, dev)
    x = torch.rand(B, T * K, 8, generator=torch.Generator().manual_seed(3)).to(dev)
    ws = ops.new_workspaces(dev)
    gen = torch.Generator().manual_seed(hash((which, kind)) % 1000)

    def launch():
        args = [m.actor.encode_args(x, None)[0] for m in (low, high)]
        if which == "encoder":
            return torch.stack(custom_ops.lstm_encode(args, ws=ws)[0])
        from gnnpn_sc_amd.modelPN import two_level_greedy
        out = two_level_greedy(low, high, x, precision="f32", ws=ws)
        return torch.cat([out["idx_low"], out["idx_high"]]).float()
    ref = launch().clone()
    assert ws.poll() == 0 and all(p["finished"] == p["expected"] == p["host_expected"] for p in ws.last_progress.values())
    assert ws.last_progress[which]["expected"] == ops.Workspaces.coop_units(2, B)
    buf = ws._encode if which == "encoder" else ws._decode
    try:
        # the workspaces as a per-launch zeroing would leave them, then the poison; the test hook (GNNPN_ABLATE_KEEP_WORKSPACE) makes the
        # launches skip their own zeroing (the decode call's encoder launch included: its workspace is clean)
        ws._encode.zero_()
        if ws._decode is not None:
            ws._decode.zero_()
        buf[:ops.COOP_STATUS_BYTES].view(torch.int32).copy_(_poison(kind, ops.COOP_STATUS_BYTES // 4, gen))
        torch.cuda.synchronize()
        ops.set_option("lstm_ablate", ops.GNNPN_ABLATE_KEEP_WORKSPACE)
        got = launch()
        torch.cuda.synchronize()
        ops.set_option("lstm_ablate", 0)
        word = ws.poll()
        assert word != 0 or torch.equal(got, ref), f"{which}/{kind}: status 0 and a wrong result: {ws.last_progress}"
        if kind in ("previous_totals", "seat_counters_only", "random_dense"):
            assert word != 0                        # these cannot run: every workgroup finds the launch "staffed"
    finally:
        ops.set_option("lstm_ablate", 0)
        assert _lib.load().gnnpn_coop_reset_staffing() == 0
    again = launch()                               # and the next ordinary launch on the same workspace is fine
    assert ws.poll() == 0 and torch.equal(again, ref)


def test_a_launch_that_does_nothing_is_a_shortfall(dev):
    """The bare mechanism: seat counters that say "staffed" and arrival counters of a FINISHED launch are what no failure code
    catches from inside (every workgroup is surplus) unless a workgroup happens to look — with code 8 masked out of the
    comparison the shortfall alone must raise: finished 0 of 256 expected."""
    from gnnpn_sc_amd import custom_ops, ops
    cfg = {"hidden": 256, "n_cat": 6, "n_per": 4, "seed_low": 1, "seed_high": 2}
    low, high = build(cfg, dev)
    x = torch.rand(256, 24, 8).to(dev)
    ws = ops.new_workspaces(dev)
    args = [m.actor.encode_args(x, None)[0] for m in (low, high)]
    custom_ops.lstm_encode(args, ws=ws)
    ws.check()
    try:
        ops.set_option("lstm_ablate", ops.GNNPN_ABLATE_KEEP_WORKSPACE)
        custom_ops.lstm_encode(args, ws=ws)         # on the counters the first launch left behind
        word, prog = ws._read()
        assert prog["encoder"]["expected"] == 2 * ops.Workspaces.coop_units(2, 256) == prog["encoder"]["host_expected"]
        assert prog["encoder"]["finished"] == ops.Workspaces.coop_units(2, 256)          # the second launch finished nothing
        assert word & ops.Workspaces.SHORTFALL
        with pytest.raises(ops.GnnpnError, match="finished != expected"):
            ws.check()
    finally:
        ops.set_option("lstm_ablate", 0)
    custom_ops.lstm_encode(args, ws=ws)
    ws.check()


def test_weights_outside_fp16_range(dev):
    """A recurrent weight beyond fp16's largest finite number: the plain-fp16 encoder ("f16") refuses it; the exact split
    scales every gate column by its own power of two and takes it, as fp32 does — same picks, logits within 1e-5."""
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.modelPN import two_level_greedy
    cfg = {"hidden": 256, "n_cat": 3, "n_per": 2, "seed_low": 1, "seed_high": 2}
    low, high = build(cfg, dev)
    with torch.no_grad():
        high.actor.decoder.weight_hh_l0[5, 7] = 7.0e4
        low.actor.encoder.weight_hh_l0[300, 9] = -1.0e5
        low.actor.encoder.weight_hh_l0[301, :] *= 1e-9               # and a column 2^-30 below the others
    x = torch.rand(4, 6, 8).to(dev)
    with pytest.raises(ops.GnnpnError):
        two_level_greedy(low, high, x, precision="f16")
    a = two_level_greedy(low, high, x)      # plain fp32 takes any finite weight
    b = two_level_greedy(low, high, x, precision="split")
    ops.check_status(dev)
    assert torch.equal(a["idx_low"], b["idx_low"]) and torch.equal(a["idx_high"], b["idx_high"])
    assert float((a["win_low"] - b["win_low"]).abs().max()) < 1e-5


@pytest.mark.parametrize("name", ["small", "qws"])
def test_sampling_mode_forward_golden(dev, name):
    """sample='sample' — every pick DRAWN from the window softmax inside the decode
    kernel (modelPN.py:227-228) — against fixtures produced by the real modelPN.py with Tensor.multinomial routed to the
    same counter-based stream.  Low greedy -> latent -> High sampled, exactly the forward of a PNHigh training step
    (trainPNHigh.py:83-84).  Picks are identical until a problem's first FRAGILE decision (a Low near-tie, or a High
    draw within 1e-5 of a cdf boundary); action_probs (the log-prob gather of :297-299) within 1e-5."""
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.modelPN import two_level_greedy
    from parity import TAU_DRAW, assert_R_parity, prefix_parity
    from pn_inputs import pn_inputs
    fx = golden(f"pn_sample_{name}.npz")
    low, high = build(fx, dev)
    T, K, B = int(fx["n_cat"]), int(fx["n_per"]), int(fx["B"])
    x = pn_inputs(B, T, K, int(fx["seed_inputs"])).to(dev)
    seed = int(fx["sample_seed"])
    out = two_level_greedy(low, high, x, sample_high_seed=seed)
    ops.check_status(dev)
    rec = prefix_parity(out["idx_low"], out["idx_high"], fx, f"sample/{name}", x.cpu(), tau_high=TAU_DRAW)
    s = rec["same_mask"]
    assert rec["identical_problems"] >= B - 2 and rec["robust_identical"] == rec["robust_problems"] > 0
    assert np.abs(out["action_probs"].cpu().numpy()[s] - fx["action_probs"][s]).max() < 1e-5
    assert np.array_equal(out["actions"].cpu().numpy()[s], fx["actions"][s])
    assert_R_parity(out["R"], fx["R"], f"sample/{name}", s)
    # the reference's own entry points: CombinatorialRL.forward with its default sample="sample"
    high.actor.sample_seed, high.actor.sample_calls = 5, 0
    _, _, _, _, latent = low(x, None, sample="greedy", training="SL")
    R1, probs1, actions1, idx1, _ = high(x, None, latent)                        # call 1 of the stream (5, ...)
    R2, _, _, idx2, _ = high(x, None, latent)                                    # call 2: new draws
    high.actor.sample_calls = 0
    R3, probs3, _, idx3, _ = high(x, None, latent)                               # call 1 again: the same draws
    assert torch.equal(torch.stack(idx1), torch.stack(idx3)) and torch.equal(R1, R3) and torch.equal(torch.stack(probs1), torch.stack(probs3))
    assert not torch.equal(torch.stack(idx1), torch.stack(idx2))
    assert len(probs1) == T and probs1[0].shape == (B,) and idx1[0].dtype == torch.int64
    p = torch.stack(probs1, 1)
    assert bool(((p > 0) & (p <= 1)).all())
    greedy = two_level_greedy(low, high, x)
    assert float((greedy["idx_high"] != out["idx_high"]).float().mean()) > 0.3  # the draws are not the argmax
    # empirical distribution of step 0 over many seeds ~ the window softmax of step 0 (first problem)
    if name == "small":
        counts = torch.zeros(K)
        for sd in range(300):
            o = two_level_greedy(low, high, x[:1], sample_high_seed=1000 + sd)
            counts[int(o["idx_high"][0, 0])] += 1
        want = torch.softmax((greedy["win_high_raw"] + greedy["win_low"])[0, 0].cpu(), 0)
        assert float((counts / 300 - want).abs().max()) < 0.12


def test_empty_and_degenerate_shapes(dev):
    """Edge shapes of the decode path: an EMPTY batch (every entry point returns empty outputs, no launch), one problem,
    one category, windows of one candidate (K = 1: the pick is forced, margin = +inf in the oracle)."""
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.modelPN import CombinatorialRL, reward, two_level_greedy
    H = 256
    for T, K, B in ((5, 3, 0), (1, 4, 3), (6, 1, 5), (1, 1, 1)):
        nets = []
        for level, seed in (("Low", 1), ("High", 2)):
            m = CombinatorialRL(0, H, T * K, 0, 10, 1, reward, "Dot", K, T, level=level)
            m.load_state_dict(opn.make_state_dict(H, seed), strict=True)
            nets.append(m.to(dev).eval())
        x = torch.rand(B, T * K, 8, generator=torch.Generator().manual_seed(T * 10 + K)).to(dev)
        out = two_level_greedy(nets[0], nets[1], x)
        ops.check_status(dev)
        assert out["idx_high"].shape == (B, T) and out["R"].shape == (B,) and out["actions"].shape == (B, T, 8)
        if B:
            ref = opn.two_level_greedy(opn.make_state_dict(H, 1), opn.make_state_dict(H, 2), x.cpu(), T, K)
            rec = prefix_parity(out["idx_low"], out["idx_high"], ref, f"edge/T{T}K{K}B{B}", rows=x.cpu())
            s = rec["same_mask"]
            assert_R_parity(out["R"], ref["R"], "edge", mask=s)
            if K == 1:
                assert s.all() and torch.equal(out["idx_high"].cpu().long(), torch.arange(T).expand(B, T))
        # the reference-style call on the same shape
        R, probs, actions, idxs, _ = nets[1](x, None, nets[0](x, None, sample="greedy", training="SL")[4], sample="greedy")
        assert R.shape == (B,) and len(idxs) == T and idxs[0].shape == (B,)


# ---- the general attention decoder (pointer_decode_glimpse_kernel<H, BAHDANAU>), build by build, against a float64 replay of its
# own path: tests/attn_decode_reference.py holds the reference, the seeded inputs, the cases and the decision rules;
# tests/test_attn_decode_host.py holds the cases to what gives these rules their bite, on the CPU
_ATTN_REC = None


def _attn_recorder():
    global _ATTN_REC
    if _ATTN_REC is None:
        from kernel_checks import Recorder
        _ATTN_REC = Recorder("attn_decode")
    return _ATTN_REC


def _attn_decode_run(dev, w, c, repeat=True):
    """ops.pointer_decode_attn on the operands ``w`` of case ``c``, twice (the same bits in every output; once without ``repeat``),
    status clean; the outputs on the host."""
    from gnnpn_sc_amd import ops
    from kernel_checks import twice
    H = c.H
    d = {k: v.to(dev) for k, v in w.items() if v is not None}
    net = {k: d[k] for k in ("embedded", "enc_out", "h0", "c0", "start", "bih", "bhh")}
    net.update(wih=ops.pack_lstm_weight(d["wih"]), whh=ops.pack_lstm_weight(d["whh"]), latent_win=d.get("latent"))
    if c.sample_seed is not None:
        net.update(sample=True, sample_seed=c.sample_seed)

    def side(tag):
        if f"{tag}_wq" not in d:
            return None
        return {"wq": d[f"{tag}_wq"], "bq": d[f"{tag}_bq"], "v": d[f"{tag}_v"], "bref": torch.zeros(H, device=dev),
                "wref": torch.eye(H, device=dev) * adr.W_REF_SCALE[tag]}
    run = lambda: ops.pointer_decode_attn(net, d["inputs"], c.T, c.K, "Bahdanau" if c.bah else "Dot", c.G, pointer=side("p"),   # noqa: E731
                                          glimpse=side("g"), tanh_c=c.C, use_tanh=bool(c.use_tanh), want_queries=True)
    out = twice(run) if repeat else run()
    ops.check_status(dev)
    return {k: out[k].cpu() for k in ("idx", "win_logits", "pick_prob", "actions", "queries")}


def _attn_decode_check(dev, w, c, kernel, floor_rel=2e-6, pick_prob=True, repeat=True, bite=True):
    """The statement of test_attention_decode_build_vs_float64_replay for one case.  -> (outputs, float64 replay, eps)."""
    from kernel_checks import same_bits
    B, T, K = c.B, c.T, c.K
    got = _attn_decode_run(dev, w, c, repeat)
    # exact: every pick inside its step's window, every action row the input row of the pick
    idx = got["idx"].long()
    lo = torch.arange(T) * K
    assert bool(((idx >= lo) & (idx < lo + K)).all()), "a pick outside its window"
    assert same_bits(got["actions"], w["inputs"][torch.arange(B).unsqueeze(1), idx]), "an action row is not the pick's input row"
    pick = idx - lo
    # numeric: the kernel's own path replayed in float64 and in float32
    r64, r32 = adr.replay(w, c, adr.D, idx=idx), adr.replay(w, c, adr.F32, idx=idx)
    at = lambda r: torch.gather(r["probs"], 2, pick.unsqueeze(2)).squeeze(2)      # noqa: E731
    rec = _attn_recorder()
    quantities = [("win_logits", got["win_logits"], r64["z0"], r32["z0"]), ("queries", got["queries"], r64["q"], r32["q"])]
    if pick_prob:
        quantities.append(("pick_prob", got["pick_prob"], at(r64), at(r32)))
    failures = []
    for what, g, a, b in quantities:
        assert bool(torch.isfinite(g).all()), what
        try:
            rec.yardstick(kernel, what, g, a, b, floor_rel=floor_rel)
        except AssertionError as e:                                               # every quantity is measured before the test fails
            failures.append(str(e))
    print(f"{kernel} [{c.id}]:", {k: f"{v:.3g}" for k, v in rec.worst[kernel].items()})
    assert not failures, failures
    # decisions: every one of them, none left out
    eps = adr.allowance(r64, r32)
    if c.sample_seed is None:
        adr.check_greedy(pick, r64["z"], eps)
    else:
        adr.check_sampled(pick, r64["probs"], c.sample_seed)
    if bite:
        adr.assert_bite(c, r64, eps)                                              # what gives the rule its bite, from float64 alone
    return got, r64, eps


def _attn_kernel_name(c):
    return f"pointer_decode_glimpse_{c.H}_{'bahdanau' if c.bah else 'dot'}"


@pytest.mark.parametrize("c", adr.CASES, ids=[c.id for c in adr.CASES])
def test_attention_decode_build_vs_float64_replay(dev, c):
    """pointer_decode_glimpse_kernel<H, BAHDANAU> (ops.pointer_decode_attn; 'Dot' and 'Bahdanau' at H = 32 and 256) at the shapes
    and switch settings where its loops change shape: T beyond one stride of the mask loop, sequences shorter than a workgroup and
    than its wave count, full / forced / odd windows, 0 to 8 glimpse rounds, no tanh, other tanh_c, with and without the latent,
    drawn picks, 300 workgroups.  The kernel's own picks are replayed through the reference in float64 and float32.
    Exact: two runs give the same bits; every pick lies in its window; every action row is the pick's input row; clean status.
    Numeric (kernel_checks.Recorder.yardstick, its defaults): the error of win_logits, queries and pick_prob against float64 is
    at most four times torch's own fp32 error plus 2e-6 of the scale.  The longest sums here run over 259 positions (one fmaf chain
    per query element): sqrt(259) * 2^-24 < 1e-6, so the default floor stands for every quantity.
    Decisions, every one: eps = 4 max|z32 - z64| + 2e-6 max|z64| is what the logits themselves are allowed; a greedy pick's
    float64 logit is within 2 eps of the window's float64 maximum; a drawn pick is the draw rule's on the float64 cdf (a neighbour
    where u is within parity.TAU_DRAW of the boundary).  The shares that give these rules their bite (margins above 2 eps in
    >= 98 % of the decisions; >= 30 % of the drawn picks not the argmax, <= 2 % of the draws near a boundary) are asserted from
    float64 alone, here and on the CPU (test_attn_decode_host.py)."""
    _attn_decode_check(dev, adr.decode_inputs(c), c, _attn_kernel_name(c))


@pytest.mark.parametrize("c", adr.FIRST_MAX_CASES, ids=[c.id for c in adr.FIRST_MAX_CASES])
def test_attention_decode_first_maximum_on_equal_rows(dev, c):
    """Equal rows of enc_out (and so of ref) with equal latents give logits equal bit for bit, and the pick is the FIRST maximum
    (torch.max on the CPU): a window of K copies is picked at its first position; a window with copies at positions 1 and 4 only,
    which stand above the rest by more than 2 eps in float64, is picked at position 1.  Exact assertions."""
    from kernel_checks import same_bits
    K, pw, ew = c.K, adr.PAIR_WINDOW, adr.EQUAL_WINDOW
    w = adr.equal_rows_inputs(c)
    got, r64, eps = _attn_decode_check(dev, w, c, _attn_kernel_name(c) + "_ties", bite=False)   # half of the windows are ties on purpose
    win = got["win_logits"]
    assert same_bits(win[:, ew], win[:, ew, :1].expand(-1, K).contiguous()), "equal rows, different logits"
    assert torch.equal(got["idx"][:, ew].long(), torch.full((c.B,), ew * K)), got["idx"]
    assert same_bits(win[:, pw, adr.PAIR[0]], win[:, pw, adr.PAIR[1]])
    assert float(adr.pair_margin(r64).min()) > 2 * eps
    assert torch.equal(got["idx"][:, pw].long(), torch.full((c.B,), pw * K + adr.PAIR[0])), got["idx"]


def test_attention_decode_lds_limit(dev, monkeypatch):
    """The dynamic-LDS limit of the launch, (L + T) * 4 bytes <= 120 KB (H = 32, B = 1, 'Dot', one glimpse round).
    Refused: T = 480, n_per = 64, with code -2 and before any launch — the outputs the call allocated still hold what they held.
    Accepted and run: T = 257, n_per = 63, 65 792 bytes, the fewest steps whose dynamic LDS is still past 64 KB (the launch has to
    ask for more than the default), held to the float64 replay of its path like every other case: win_logits and queries by
    yardstick with its defaults, every decision by the 2 eps rule; one run.  The exact edge, T = 480 and n_per = 63 (30 720 words =
    120 KB), was measured once on an MI355X: accepted, its picks within 2 eps of the float64 maxima, win_logits and queries within
    0.24 and 0.38 of a yardstick with the floor 1e-5 — and 12.3 s for two runs and the two replays (one wavefront walks 30 240
    positions in each of 480 steps), too long for this suite; the case that stays does about (257 / 480)^2 of that work, 1.8 s."""
    from gnnpn_sc_amd import ops
    c = adr.LDS_EDGE
    assert 64 * 1024 < (c.T * c.K + c.T) * 4 <= 120 * 1024
    _attn_decode_check(dev, adr.decode_inputs(c), c, "pointer_decode_glimpse_32_dot_lds_past_64k", pick_prob=False, repeat=False)
    over = c._replace(T=adr.LDS_REFUSED[0], K=adr.LDS_REFUSED[1])
    w = adr.decode_inputs(over)
    made, outputs = [], ops._decode_outputs

    def sentinel_outputs(*a):
        out = outputs(*a)
        out["idx"].fill_(-7)
        for k in ("win_logits", "pick_prob", "actions"):
            out[k].fill_(-7.0)
        made.append(out)
        return out
    monkeypatch.setattr(ops, "_decode_outputs", sentinel_outputs)
    d = {k: v.to(dev) for k, v in w.items() if v is not None}
    net = {k: d[k] for k in ("embedded", "enc_out", "h0", "c0", "start", "bih", "bhh")}
    net.update(wih=ops.pack_lstm_weight(d["wih"]), whh=ops.pack_lstm_weight(d["whh"]), latent_win=d["latent"])
    with pytest.raises(ops.GnnpnError, match=r"\(-2\).*does not fit the LDS buffer"):
        ops.pointer_decode_attn(net, d["inputs"], over.T, over.K, "Dot", 1)
    torch.cuda.synchronize()
    ops.check_status(dev)
    assert len(made) == 1
    assert bool((made[0]["idx"] == -7).all()) and all(bool((made[0][k] == -7.0).all()) for k in ("win_logits", "pick_prob", "actions"))
