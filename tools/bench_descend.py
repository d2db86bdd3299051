#!/usr/bin/env python3
"""The one-swap descent beside the ES-WOA refinement it precedes, on the two configurations and the generators of
tools/bench_refine.py (tools/search_bench.py holds them; 1000 synthetic test problems each):

    qws     47 categories, 2507 services, 10 tasks, reduct 0,    pop 50, 250 iterations
    normal  50 categories, 5000 services, 10 tasks, reduct 0.55, pop 60, 500 iterations

Problems/s by HIP events for the table builder (gnnpn_woa_candidates_count + _fill), descent alone (gnnpn_descend_ragged_f64),
ES-WOA alone (gnnpn_eswoa_ragged_f64 from the tables' start) and descent + ES-WOA (ES-WOA from the descended composition); and,
for the start, descent, ES-WOA and descent + ES-WOA, the mean best_fitness with descent's mean sweeps and moves.  Prints one
JSON line.

    python tools/bench_descend.py [--problems 1000] [--configs qws,normal] [--repeat 3] [--sweeps 16] [--wide]

``--wide``: the workgroup form of both searches (``wide=True`` to ops.descend_ragged and ops.eswoa_ragged).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from search_bench import CONFIGS, _seed_rows, mean, setup, timed          # noqa: E402


def run_config(cfg, n_test, repeat, sweeps, dev, wide=None):
    import torch
    from gnnpn_sc_amd import ops
    ds, svc, batch, _first, sd = setup(cfg, n_test, dev)
    a = torch.from_numpy(_seed_rows(ds, cfg["reduct"], np.random.default_rng(2))).to(dev)

    def build():
        return ops.woa_candidates(svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds, a,
                                  reduct=cfg["reduct"])

    def eswoa(tabs, start_pos=None):
        return tabs.eswoa(cfg["pop"], cfg["iters"], sd, start_pos, wide=wide)

    tabs = build()                                                                     # warm-up of the three stages
    descended_pos = tabs.flat(tabs.descend(sweeps, wide)["best_pos"])
    eswoa(tabs)
    ms = {"builder": [], "descent": [], "eswoa": [], "eswoa_after_descent": []}
    for _ in range(repeat):
        tabs, t = timed(build, dev)
        ms["builder"].append(t)
        des, t = timed(lambda: tabs.descend(sweeps, wide), dev)
        ms["descent"].append(t)
        alone, t = timed(lambda: eswoa(tabs), dev)
        ms["eswoa"].append(t)
        both, t = timed(lambda: eswoa(tabs, descended_pos), dev)
        ms["eswoa_after_descent"].append(t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    per_s = lambda t: round(n_test / (t * 1e-3), 1)                 # noqa: E731
    return {"problems": n_test, **cfg, "max_sweeps": sweeps, "mean_slots": mean(tabs["n_slots"]),
            "mean_candidates": round(tabs["cand"].shape[0] / n_test, 2),
            "builder_ms": round(med["builder"], 3), "descent_ms": round(med["descent"], 3), "eswoa_ms": round(med["eswoa"], 3),
            "eswoa_after_descent_ms": round(med["eswoa_after_descent"], 3),
            "builder_problems_per_s": per_s(med["builder"]), "descent_problems_per_s": per_s(med["descent"]),
            "eswoa_problems_per_s": per_s(med["eswoa"]),
            "descent_plus_eswoa_problems_per_s": per_s(med["descent"] + med["eswoa_after_descent"]),
            "descent_faster_than_eswoa": med["descent"] < med["eswoa"],
            "start": {"mean_best_fitness": mean(des["start_fitness"])},
            "descent": {"mean_best_fitness": mean(des["best_fitness"]), "mean_sweeps": mean(des["sweeps"]), "mean_moves": mean(des["moves"])},
            "eswoa": {"mean_best_fitness": mean(alone[0])},
            "descent_plus_eswoa": {"mean_best_fitness": mean(both[0]), "mean_sweeps": mean(des["sweeps"]), "mean_moves": mean(des["moves"])}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=1000)
    ap.add_argument("--configs", default="qws,normal")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--sweeps", type=int, default=16)
    ap.add_argument("--wide", action="store_true")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    out = {"metric": "descend", "configs": {}}
    for name in args.configs.split(","):
        out["configs"][name] = run_config(CONFIGS[name], args.problems, args.repeat, args.sweeps, dev, wide=args.wide or None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
