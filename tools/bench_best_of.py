#!/usr/bin/env python3
"""Best-of-N decoding of the High level (modelPN.two_level_best_of): answers per second and mean R against N, at the QWS and
Normal shapes, B problems per call (default 256), N in {1, 2, 4, 8, 16, 32}:

    qws     47 categories, 5 candidates each (L = 235), 2507 services
    normal  50 categories, 10 candidates each (L = 500), 5000 services

The PN input rows come from one ML2PNPipeline.run over a synthetic batch (its front end is not timed).  Per N the call is
timed whole (answers/s = B / wall time of one call, the final status check included) and split by HIP events into
encode + greedy decode (the fused two-level pass with its reward), replica decode (one launch of N-1 sampled High rows per
problem) and reward + select.  Mean R of the greedy answer (replica 0) and of the best-of answer are reported.  Weights:
the seeded random weights of bench.build_models unless --weights DIR gives <DIR>/<ds>-{ML.pt,PNLow.model,PNHigh.model}
(the reference's checkpoint formats); the JSON line says which.  Random weights show the mechanics, not the quality.
--score DATASET additionally runs ML2PN.infer / ML2PN.check on ./data/DATASET for each N (the `main.py --samples=N` path).

    python tools/bench_best_of.py [--configs qws,normal] [--batch 256] [--samples 1,2,4,8,16,32] [--repeat 5] [--weights DIR]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

CONFIGS = {"qws": dict(T=47, S=2507, K=5, ds="QWS"), "normal": dict(T=50, S=5000, K=10, ds="Normal")}


def _load_weights(wdir, ds, net, low, high):
    import main as cli
    net.load_state_dict(cli._load_ml_checkpoint(os.path.join(wdir, f"{ds}-ML.pt")))
    for m, n in ((low, "PNLow"), (high, "PNHigh")):
        ck = torch.load(os.path.join(wdir, f"{ds}-{n}.model"), map_location="cpu", weights_only=True)
        m.load_state_dict(ck["model"] if "model" in ck else ck)


def _timed_call(low, high, rows, N, seed, precision):
    """One best-of call with HIP events around its three phases (the same steps as two_level_best_of)."""
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.modelPN import _select, _two_level_fused, qosandcons
    ha = high.actor
    B, T, K = rows.shape[0], ha.serCategory, ha.serNumber
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    g, (enc_h, h_h, c_h, emb_h) = _two_level_fused(low, high, rows, None, precision, 0, 0, False, None, None, False)
    ev[1].record()
    sam = None
    if N > 1:
        net = ha.decode_args(emb_h, enc_h, h_h, c_h, latent_win=g["win_low"])
        rep = ops.pointer_decode_replicas(net, rows, T, K, N - 1, seed, first=1, tanh_c=ha.C, use_tanh=ha.use_tanh)
    ev[2].record()
    if N > 1:
        R_s = torch.ops.gnnpn.qos_reward(rep["actions"].view(B * (N - 1), T, qosandcons), 1)
        sam = {"R": R_s.view(B, N - 1), "idx": rep["idx"], "actions": rep["actions"], "probs": rep["pick_prob"]}
    sel = _select(g, sam, qosandcons)
    ev[3].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(3)], g["R"], sel["R"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="qws,normal")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--samples", default="1,2,4,8,16,32")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--weights", default=None)
    ap.add_argument("--precision", default=None, help="encoder / greedy precision (default: the pipeline's, 'split')")
    ap.add_argument("--score", default=None, help="also run ML2PN.infer + check on ./data/DATASET per N")
    a = ap.parse_args()
    import gnnpn_sc_amd.synth as synth
    from bench import build_models
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.modelPN import two_level_best_of
    from gnnpn_sc_amd.pipeline import DeviceBatch, DeviceServices, ML2PNPipeline
    dev = torch.device("cuda:0")
    Ns = [int(x) for x in a.samples.split(",")]
    res = {"tool": "bench_best_of", "batch": a.batch, "weights": a.weights or "random (bench.build_models, seed 0)", "configs": {}}
    for name in a.configs.split(","):
        c = CONFIGS[name]
        T, S, K = c["T"], c["S"], c["K"]
        table = synth.make_service_table(T, S, seed=0, degree=32)
        pb = synth.make_problem_batch(table, a.batch, seed=1, tasks_per_problem=10)
        net, low, high = build_models(T, S, K, dev)
        if a.weights:
            _load_weights(a.weights, c["ds"], net, low, high)
        pipe = ML2PNPipeline(net, low, high, K, precision=a.precision)
        svc, batch = DeviceServices.from_table(table, dev), DeviceBatch.from_problems(pb, dev)
        rows = pipe.run(svc, batch)["pn_inputs"]
        rows_cfg = []
        for N in Ns:
            two_level_best_of(low, high, rows, N, seed=a.seed, precision=pipe.precision)      # warm-up (workspaces, packing)
            torch.cuda.synchronize()
            walls, parts = [], []
            for r in range(a.repeat):
                t0 = time.perf_counter()
                out = two_level_best_of(low, high, rows, N, seed=a.seed + r, precision=pipe.precision)
                torch.cuda.synchronize()
                walls.append(time.perf_counter() - t0)
                p, Rg, Rb = _timed_call(low, high, rows, N, a.seed + r, pipe.precision)
                parts.append(p)
            ops.check_status(dev)
            wall = sorted(walls)[len(walls) // 2]
            med = [sorted(x[i] for x in parts)[len(parts) // 2] for i in range(3)]
            row = {"N": N, "answers_per_s": round(a.batch / wall, 1), "ms_per_call": round(wall * 1e3, 3),
                   "ms_encode_greedy": round(med[0], 3), "ms_replicas": round(med[1], 3), "ms_reward_select": round(med[2], 3),
                   "mean_R_greedy": round(float(out["R_all"][:, 0].mean()), 5), "mean_R_best": round(float(out["R"].mean()), 5),
                   "improved": int((out["sample_index"] > 0).sum())}
            if N > 1:
                row["us_replica_decode_per_row"] = round(med[1] * 1e3 / (a.batch * (N - 1)), 3)
            rows_cfg.append(row)
            print(f"{name} N={N:3d}: {row['answers_per_s']:9.1f} answers/s  encode+greedy {med[0]:.3f} ms  replicas "
                  f"{med[1]:.3f} ms  reward+select {med[2]:.3f} ms  mean R {row['mean_R_greedy']:.5f} -> {row['mean_R_best']:.5f}",
                  file=sys.stderr)
        res["configs"][name] = rows_cfg
        if a.score and c["ds"].lower() == a.score.lower():
            from gnnpn_sc_amd import ML2PN
            res.setdefault("score", {})
            for N in Ns:
                ML2PN.infer(c["ds"], net, low, high, K, -1, samples=N, sample_seed=a.seed)
                res["score"][str(N)] = ML2PN.check(c["ds"], T, -1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
