"""-m gpu: best-of-N decoding of the High level (modelPN.two_level_best_of, ML2PNPipeline.best_of, main.py --samples=N).

Replica 0 is two_level_greedy's answer; replica j >= 1 must be, bit for bit, the existing one-net sampled decode of the same
problems with sample_seed = replica_seed(S, j) (the draws already pinned to the reference's multinomial by the pn_sample_*
fixtures); the answer is the replica with the smallest R, the lowest index on ties."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (T, S, K, B, N): the QWS shape at B = 256, N = 16 (3840 replica rows = 240 tiles of 16: more than the 64 groups of one
# pass take), and the Normal shape
SHAPES = {"qws": (47, 2507, 5, 256, 16), "normal": (50, 5000, 10, 96, 8)}


@pytest.fixture(scope="module", params=sorted(SHAPES))
def case(request):
    import gnnpn_sc_amd.synth as synth
    from bench import build_models
    from gnnpn_sc_amd.pipeline import DeviceBatch, DeviceServices, ML2PNPipeline
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    T, S, K, B, N = SHAPES[request.param]
    table = synth.make_service_table(T, S, seed=0, degree=32)
    pb = synth.make_problem_batch(table, B, seed=1, tasks_per_problem=10)
    net, low, high = build_models(T, S, K, dev)
    pipe = ML2PNPipeline(net, low, high, K)
    svc, batch = DeviceServices.from_table(table, dev), DeviceBatch.from_problems(pb, dev)
    rows = pipe.run(svc, batch)["pn_inputs"]
    return dict(name=request.param, T=T, K=K, B=B, N=N, pipe=pipe, svc=svc, batch=batch, low=low, high=high, rows=rows, dev=dev)


def test_one_sample_is_the_greedy_pass(case):
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.modelPN import two_level_best_of, two_level_greedy
    low, high, rows = case["low"], case["high"], case["rows"]
    g = two_level_greedy(low, high, rows)
    b = two_level_best_of(low, high, rows, 1, seed=11)
    for k, v in g.items():
        assert torch.equal(b[k], v), k
    assert bool((b["sample_index"] == 0).all())
    assert torch.equal(b["R_all"][:, 0], g["R"]) and torch.equal(b["idx_all"][:, 0], g["idx_high"])
    run = case["pipe"].run(case["svc"], case["batch"])
    best = case["pipe"].best_of(case["svc"], case["batch"], 1)
    for k, v in run.items():
        assert torch.equal(best[k], v), k
    assert bool((best["sample_index"] == 0).all())
    ops.check_status(case["dev"])


@pytest.mark.parametrize("enc_precision", ["f32", "split"])
def test_replicas_are_the_one_net_sampled_decode(case, enc_precision):
    """Replica j of the one replica launch == custom_ops.pointer_decode of the High net alone with sample_seed =
    replica_seed(S, j), on the same encoder outputs and Low window logits (the decoder is fp32 in both)."""
    from conftest import record_agreement
    from gnnpn_sc_amd import custom_ops, ops
    from gnnpn_sc_amd.modelPN import _two_level_fused
    low, high, rows = case["low"], case["high"], case["rows"]
    T, K, N = case["T"], case["K"], case["N"]
    ha = high.actor
    S = 0x5EED0 + N
    g, (enc_h, h_h, c_h, emb_h) = _two_level_fused(low, high, rows, None, enc_precision, 0, 0, False, None, None, False)
    net = ha.decode_args(emb_h, enc_h, h_h, c_h, latent_win=g["win_low"])
    rep = ops.pointer_decode_replicas(net, rows, T, K, N - 1, S, first=1, tanh_c=ha.C, use_tanh=ha.use_tanh)
    for j in range(1, N):
        one = custom_ops.pointer_decode([ha.decode_args(emb_h, enc_h, h_h, c_h, latent_win=g["win_low"],
                                                        sample_seed=ops.replica_seed(S, j))],
                                        rows, T, K, ha.C, ha.use_tanh, precision="f32")[0]
        for k in ("idx", "pick_prob", "actions", "win_logits"):
            assert torch.equal(rep[k][:, j - 1], one[k]), (j, k)
    ops.check_status(case["dev"])
    assert float((rep["idx"][:, 0] != g["idx_high"]).float().mean()) > 0.05      # the draws are not the argmax
    if enc_precision != "f32":
        return
    # the fused two-level call that samples High (the training forward) at "f32": its Low pass runs in the sampling build of
    # the cooperative decoder, the greedy pass above in the production build — the High picks agree wherever Low's window
    # logits do; the problems where they do not are counted, not hidden
    from gnnpn_sc_amd.modelPN import two_level_greedy
    rec = {"shape": case["name"], "replicas_checked": 0, "low_window_differs": [], "high_picks_differ": []}
    for j in (1, 2, N - 1):
        t = two_level_greedy(low, high, rows, precision="f32", sample_high_seed=ops.replica_seed(S, j))
        same_low = (t["win_low"] == g["win_low"]).flatten(1).all(1)
        same_pick = (t["idx_high"] == rep["idx"][:, j - 1]).all(1)
        rec["replicas_checked"] += 1
        rec["low_window_differs"].append(int((~same_low).sum()))
        rec["high_picks_differ"].append(int((~same_pick).sum()))
        assert bool(same_pick[same_low].all()), j
    print(f"best_of/{case['name']}: problems whose Low window logits differ between the builds: {rec['low_window_differs']}, "
          f"High picks differing: {rec['high_picks_differ']}")
    record_agreement(f"best_of/low_window_{case['name']}", rec)
    ops.check_status(case["dev"])


def test_selection_is_min_R_lowest_index(case):
    from gnnpn_sc_amd import ops
    low, high, rows = case["low"], case["high"], case["rows"]
    B, N, T = case["B"], case["N"], case["T"]
    out = case["pipe"].best_of(case["svc"], case["batch"], N, seed=2024)
    R_all = out["R_all"].cpu().numpy()
    assert R_all.shape == (B, N) and out["idx_all"].shape == (B, N, T)
    want = np.argmin(np.where(np.isnan(R_all), np.inf, R_all), axis=1)          # first minimum: lowest index on ties
    w = out["sample_index"].cpu().numpy()
    assert np.array_equal(w, want)
    assert np.array_equal(out["R"].cpu().numpy(), R_all[np.arange(B), w])
    assert bool((out["R"] <= out["R_all"][:, 0]).all())                           # never worse than greedy
    assert torch.equal(out["idx_high"], out["idx_all"][torch.arange(B, device=rows.device), out["sample_index"].long()])
    # the winner's actions are the rows of its picks in pn_inputs, and its R is their reward
    gathered = torch.gather(out["pn_inputs"], 1, out["idx_high"].long().unsqueeze(-1).expand(-1, -1, 8))
    assert torch.equal(out["actions"], gathered)
    assert torch.equal(ops.qos_reward(out["actions"].contiguous(), "High"), out["R"])
    p = out["action_probs"]
    assert bool(((p > 0) & (p <= 1)).all())
    ties = int(((R_all[:, 1:] == R_all[:, :1]).any(1)).sum())
    print(f"best_of/{case['name']}: N={N}: {int((w > 0).sum())}/{B} problems improved by a sample, {ties} with a tie against "
          f"greedy; mean R greedy {R_all[:, 0].mean():.5f} -> best {out['R'].float().mean().item():.5f}")


def test_same_seed_same_answer_other_seed_other_samples(case):
    low, high, rows, N = case["low"], case["high"], case["rows"], case["N"]
    from gnnpn_sc_amd.modelPN import two_level_best_of
    a = two_level_best_of(low, high, rows, N, seed=77)
    b = two_level_best_of(low, high, rows, N, seed=77)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    c = two_level_best_of(low, high, rows, N, seed=78)
    assert not torch.equal(a["idx_all"][:, 1:], c["idx_all"][:, 1:])
    assert torch.equal(a["idx_all"][:, 0], c["idx_all"][:, 0])


def test_one_encode_one_replica_launch_no_replicated_state(case, monkeypatch):
    """One call: ONE lstm_encode launch (both nets), the fused greedy decode and ONE replica decode launch — counted at the
    wrappers and in the workspace's proof-of-work tally; peak memory grows by far less than one [B*N, L, H] enc_out."""
    from gnnpn_sc_amd import custom_ops, ops
    from gnnpn_sc_amd.modelPN import two_level_best_of, two_level_greedy
    low, high, rows, N, B = case["low"], case["high"], case["rows"], case["N"], case["B"]
    calls = {"lstm_encode": 0, "pointer_decode": 0, "pointer_decode_replicas": 0}

    def counted(mod, name):
        fn = getattr(mod, name)

        def call(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        monkeypatch.setattr(mod, name, call)
    counted(custom_ops, "lstm_encode")
    counted(custom_ops, "pointer_decode")
    counted(ops, "pointer_decode_replicas")
    wg, wb = ops.new_workspaces(case["dev"]), ops.new_workspaces(case["dev"])

    def peak_growth(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base
    g_growth = peak_growth(lambda: two_level_greedy(low, high, rows, ws=wg))
    L, H = rows.shape[1], 256
    for k in calls:
        calls[k] = 0
    growth = peak_growth(lambda: two_level_best_of(low, high, rows, N, seed=3, ws=wb)) - g_growth
    assert calls == {"lstm_encode": 1, "pointer_decode": 1, "pointer_decode_replicas": 1}, calls
    assert wb.launched[0] == wg.launched[0]                                    # the same encoder launch as the greedy pass
    assert wb.launched[1] - wg.launched[1] == ops.Workspaces.coop_units(1, B * (N - 1))
    wg.check(), wb.check()
    replicated = B * N * L * H * 4
    assert growth < replicated // 8, (growth, replicated)
    print(f"best_of/{case['name']}: peak allocation grew by {growth / 2**20:.1f} MiB more than the greedy pass's; one replicated enc_out would be "
          f"{replicated / 2**20:.1f} MiB")


def test_streaming_replicas_are_the_one_net_sampled_decode(case):
    """The per-workgroup streaming form (devices / nets the cooperative form does not take): same row -> problem indirection."""
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.modelPN import _two_level_fused
    low, high = case["low"], case["high"]
    rows = case["rows"][:24].contiguous()
    T, K = case["T"], case["K"]
    ha = high.actor
    g, (enc_h, h_h, c_h, emb_h) = _two_level_fused(low, high, rows, None, "f32", 0, 0, False, None, None, False)
    net = ha.decode_args(emb_h, enc_h, h_h, c_h, latent_win=g["win_low"])
    rep = ops.pointer_decode_replicas(net, rows, T, K, 3, 99, first=1, tanh_c=ha.C, use_tanh=ha.use_tanh, impl=1)
    for j in range(1, 4):
        one = ops.pointer_decode([ha.decode_args(emb_h, enc_h, h_h, c_h, latent_win=g["win_low"], sample_seed=ops.replica_seed(99, j))],
                                 rows, T, K, ha.C, ha.use_tanh, impl=1)[0]
        for k in ("idx", "pick_prob", "actions", "win_logits"):
            assert torch.equal(rep[k][:, j - 1], one[k]), (j, k)


def test_main_cli_samples_writes_actions_no_worse_than_greedy(tmp_path, monkeypatch):
    """`main.py QWS ML+2PN -1 --infer --random-init --samples=4 --seed 7` on a small synthetic data set: ML2PN.check scores the
    artefacts, and every test problem's R of the written actions is at most the greedy run's on the same weights.  The check
    score is reported, not asserted: it is not the reward (it drops dummy rows and takes the ranking rows' constraints)."""
    import gnnpn_sc_amd.synth as synth
    import main as cli
    from gnnpn_sc_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    T, S, P, K, H = 6, 60, 16, 3, 256
    ds = synth.make_dataset(T, S, P, seed=3, tasks_per_problem=3, lo_range=(0.80, 0.955))
    synth.write_dataset(str(tmp_path), "QWS", ds)
    monkeypatch.chdir(tmp_path)
    with open("environment.ini", "w") as f:
        f.write("[QWS-ML]\nnumLayersGIN = 2\nnumLayersGCN = 2\nhiddenChannels = 128\nembeddingChannels = 20\ndropout = 0.0\n"
                f"[QWS-PNHigh]\nserNumber = {K}\nhidden_size = {H}\nn_glimpses = 0\ntanh_exploration = 10\nuse_tanh = 1\n"
                f"[QWS-ML+2PN]\nserviceCategory = {T}\nepoch = -1\n")
    from gnnpn_sc_amd import ML2PN
    act_path = ML2PN.artifact_paths("QWS", -1)[1]

    def run(*extra):
        if os.path.exists(act_path):
            os.remove(act_path)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            assert cli.main(["main.py", "QWS", "ML+2PN", "-1", "--infer", "--random-init", *extra]) == 0
        with open(act_path) as fh:
            acts = torch.tensor(json.load(fh), dtype=torch.float32).permute(1, 0, 2).contiguous()   # [nTest, T, 8]
        return float(buf.getvalue().strip().splitlines()[-1].split()[1]), acts
    score_g, act_g = run()
    score_b, act_b = run("--samples=4", "--seed", "7")
    score_b2, act_b2 = run("--samples=4", "--seed", "7")
    assert torch.equal(act_b, act_b2) and score_b == score_b2
    dev = torch.device("cuda:0")
    R_g = ops.qos_reward(act_g.to(dev), "High")
    R_b = ops.qos_reward(act_b.to(dev), "High")
    assert act_b.shape == act_g.shape == (P // 4, T, 8)
    assert bool((R_b <= R_g).all()), (R_b, R_g)
    assert np.isfinite(score_b) and np.isfinite(score_g)
    print(f"best_of/cli: check score greedy {score_g:.6f}, best-of-4 {score_b:.6f}; mean R greedy {R_g.mean().item():.5f}, "
          f"best-of-4 {R_b.mean().item():.5f}")
