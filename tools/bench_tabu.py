#!/usr/bin/env python3
"""The tabu walk beside the searches around it, on the two configurations, the generators and the 1000 problems of
tools/bench_descend.py (tools/search_bench.py holds them):

    qws     47 categories, 2507 services, 10 tasks, reduct 0,    pop 50, 250 iterations
    normal  50 categories, 5000 services, 10 tasks, reduct 0.55, pop 60, 500 iterations

In one run: one-swap descent (gnnpn_descend_ragged_f64), pair descent (gnnpn_descend_pairs_ragged_f64, 4 rounds), pair descent over
shortlists of 8 (gnnpn_descend_pairs_shortlist_ragged_f64), ES-WOA from the tables' start, and the tabu walk
(gnnpn_descend_tabu_ragged_f64) at max_steps 8, 32 and 128 with --tenure, and at max_steps 32 with every tenure of TENURES.  Per
column the time by HIP events (median of --repeat after a warm-up of every launch) and the mean best_fitness; for the tabu columns
also the share of problems that end below one-swap descent and below the full pair sweep, the mean steps and best_step, the stalled
share, and the time of one step (the walk's time beyond descent's, over its mean steps) against one descent sweep (descent's time
over its mean sweeps).  ``default_tenure``: the tenure of the sweep with the lowest mean merit over the configurations run, the
smaller one on a tie — what ops.DEFAULT_TENURE is set from.  Figures of one box and one session; no test holds any of them.
Prints one JSON line; --out writes it to a file.

    python tools/bench_tabu.py [--problems 1000] [--configs qws,normal] [--repeat 3] [--sweeps 16] [--tenure 8] [--out profiles/r13_tabu_bench.json]
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

from search_bench import CONFIGS, _seed_rows, mean, setup, share, timed          # noqa: E402

STEPS = (8, 32, 128)
TENURES = (1, 2, 4, 8, 16)
SWEEP_STEPS = 32


def run_config(cfg, n_test, repeat, sweeps, tenure, dev):
    import torch
    from gnnpn_sc_amd import ops
    ds, svc, batch, _first, sd = setup(cfg, n_test, dev)
    a = torch.from_numpy(_seed_rows(ds, cfg["reduct"], np.random.default_rng(2))).to(dev)
    tabs = ops.woa_candidates(svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds, a, reduct=cfg["reduct"])
    calls = {"descent": lambda: tabs.descend(sweeps), "pairs_4": lambda: tabs.descend_pairs(sweeps, 4),
             "pairs_shortlist_8": lambda: tabs.descend_pairs_shortlist(sweeps, 4, 0, 8),
             "eswoa": lambda: {"best_fitness": tabs.eswoa(cfg["pop"], cfg["iters"], sd)[0]}}
    for s in STEPS:
        calls[f"tabu_s{s}"] = lambda s=s: tabs.descend_tabu(sweeps, s, tenure)
    for t in TENURES:
        calls[f"tabu_s{SWEEP_STEPS}_t{t}"] = lambda t=t: tabs.descend_tabu(sweeps, SWEEP_STEPS, t)
    ms, res = {k: [] for k in calls}, {}
    for fn in calls.values():                                                          # warm-up of every launch
        fn()
    for _ in range(repeat):
        for name, fn in calls.items():
            res[name], t = timed(fn, dev)
            ms[name].append(t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    one, pairs = res["descent"]["best_fitness"], res["pairs_4"]["best_fitness"]
    sweep_ms = med["descent"] / max(mean(res["descent"]["sweeps"]), 1e-9)
    cols = {}
    for name, r in res.items():
        col = {"ms": round(med[name], 3), "ms_all": [round(v, 3) for v in ms[name]], "mean_best_fitness": mean(r["best_fitness"]),
               "violated_share": share(r["best_fitness"] >= 1.0)}
        if "sweeps" in r:
            col.update(mean_sweeps=mean(r["sweeps"]), mean_moves=mean(r["moves"]))
        if "steps" in r:
            steps = mean(r["steps"])
            col.update(below_descent_share=share(r["best_fitness"] < one), below_pairs_share=share(r["best_fitness"] < pairs),
                       above_pairs_share=share(r["best_fitness"] > pairs), above_descent_share=share(r["best_fitness"] > one),
                       mean_steps=steps, mean_best_step=mean(r["best_step"]), stalled_share=share(r["stalled"] > 0),
                       step_ms=round((med[name] - med["descent"]) / max(steps, 1e-9), 5),
                       step_over_descent_sweep=round((med[name] - med["descent"]) / max(steps, 1e-9) / sweep_ms, 3))
        cols[name] = col
    return {"problems": n_test, **cfg, "max_sweeps": sweeps, "tenure": tenure, "mean_slots": mean(tabs["n_slots"]),
            "mean_candidates": round(tabs["cand"].shape[0] / n_test, 2), "start_mean_best_fitness": mean(res["descent"]["start_fitness"]),
            "descent_sweep_ms": round(sweep_ms, 5), "columns": cols,
            "tenure_sweep": {str(t): cols[f"tabu_s{SWEEP_STEPS}_t{t}"]["mean_best_fitness"] for t in TENURES}}


def default_tenure(configs):
    """The tenure of the sweep with the lowest mean merit over the configurations, the smaller one on a tie."""
    total = {t: sum(c["tenure_sweep"][str(t)] for c in configs.values()) / len(configs) for t in TENURES}
    return min(TENURES, key=lambda t: (total[t], t)), {str(t): round(v, 6) for t, v in total.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=1000)
    ap.add_argument("--configs", default="qws,normal")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--sweeps", type=int, default=16)
    ap.add_argument("--tenure", type=int, default=None, help="the tenure of the max_steps columns (default: ops.DEFAULT_TENURE)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from gnnpn_sc_amd import ops
    dev = torch.device("cuda:0")
    tenure = ops.DEFAULT_TENURE if args.tenure is None else args.tenure
    out = {"metric": "descend_tabu", "device": torch.cuda.get_device_name(dev), "configs": {}}
    for name in args.configs.split(","):
        out["configs"][name] = run_config(CONFIGS[name], args.problems, args.repeat, args.sweeps, tenure, dev)
    out["default_tenure"], out["tenure_sweep_mean_over_configs"] = default_tenure(out["configs"])
    out["note"] = "figures of one box and one session; no test holds any of them"
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
