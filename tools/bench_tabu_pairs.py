#!/usr/bin/env python3
"""The tabu walk over pair moves beside its two parents, on the two configurations, the generators and the 1000 problems of
tools/bench_descend.py (tools/search_bench.py holds them):

    qws     47 categories, 2507 services, 10 tasks, reduct 0
    normal  50 categories, 5000 services, 10 tasks, reduct 0.55

In one run: one-swap descent (gnnpn_descend_ragged_f64), the tabu walk (gnnpn_descend_tabu_ragged_f64) at 32 and 128 steps, the pair
sweep over shortlists of 8 (gnnpn_descend_pairs_shortlist_ragged_f64, 4 rounds), the full pair sweep (gnnpn_descend_pairs_ragged_f64,
4 rounds), and the walk over pair moves (gnnpn_descend_tabu_pairs_ragged_f64) at 32 steps with every rank of RANKS; all walks at
--tenure.  Per column the time by HIP events (median of --repeat timed rounds after a settling round of every launch) and the mean
best_fitness; for the new walk's columns also the share of problems that end below and above each of the other columns, the mean
steps, best_step and pair_steps, the stalled share, and the time of one step (the walk's time beyond descent's, over its mean
steps) as a ratio of one step of the tabu walk at 32 steps.  ``default_rank``: the rank of the sweep with the lowest mean merit
over the configurations run, the smaller one on a tie — what ops.DEFAULT_PAIR_RANK is set from.  Figures of one box and one
session: only ratios within the run mean anything, and no test holds any of them.  Prints one JSON line; --out writes it to a file.

    python tools/bench_tabu_pairs.py [--problems 1000] [--configs qws,normal] [--repeat 3] [--sweeps 16] [--tenure 16] [--out profiles/r14_tabu_pairs_bench.json]
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

RANKS = (1, 2, 4, 8)
STEPS = 32
OTHERS = ("descent", "tabu_s32", "tabu_s128", "pairs_shortlist_8", "pairs_4")


def run_config(cfg, n_test, repeat, sweeps, tenure, dev):
    import torch
    from gnnpn_sc_amd import ops
    ds, svc, batch, _first, _sd = setup(cfg, n_test, dev)
    a = torch.from_numpy(_seed_rows(ds, cfg["reduct"], np.random.default_rng(2))).to(dev)
    tabs = ops.woa_candidates(svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds, a, reduct=cfg["reduct"])
    calls = {"descent": lambda: tabs.descend(sweeps), "tabu_s32": lambda: tabs.descend_tabu(sweeps, 32, tenure),
             "tabu_s128": lambda: tabs.descend_tabu(sweeps, 128, tenure),
             "pairs_shortlist_8": lambda: tabs.descend_pairs_shortlist(sweeps, 4, 0, 8), "pairs_4": lambda: tabs.descend_pairs(sweeps, 4)}
    for m in RANKS:
        calls[f"tabu_pairs_s{STEPS}_r{m}"] = lambda m=m: tabs.descend_tabu_pairs(sweeps, STEPS, tenure, m)
    ms, res = {k: [] for k in calls}, {}
    for fn in calls.values():                                                          # a settling round of every launch
        fn()
    for _ in range(repeat):
        for name, fn in calls.items():
            res[name], t = timed(fn, dev)
            ms[name].append(t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    tabu_step_ms = (med["tabu_s32"] - med["descent"]) / max(mean(res["tabu_s32"]["steps"]), 1e-9)
    cols = {}
    for name, r in res.items():
        col = {"ms": round(med[name], 3), "ms_all": [round(v, 3) for v in ms[name]], "mean_best_fitness": mean(r["best_fitness"]),
               "violated_share": share(r["best_fitness"] >= 1.0), "mean_sweeps": mean(r["sweeps"]), "mean_moves": mean(r["moves"])}
        if "steps" in r:
            steps = mean(r["steps"])
            col.update(mean_steps=steps, mean_best_step=mean(r["best_step"]), stalled_share=share(r["stalled"] > 0),
                       step_ms=round((med[name] - med["descent"]) / max(steps, 1e-9), 5))
        if "pair_steps" in r:
            col.update(mean_pair_steps=mean(r["pair_steps"]), step_over_tabu_step=round(col["step_ms"] / max(tabu_step_ms, 1e-12), 3),
                       **{f"below_{o}_share": share(r["best_fitness"] < res[o]["best_fitness"]) for o in OTHERS},
                       **{f"above_{o}_share": share(r["best_fitness"] > res[o]["best_fitness"]) for o in OTHERS})
        cols[name] = col
    return {"problems": n_test, **cfg, "max_sweeps": sweeps, "tenure": tenure, "max_steps": STEPS, "mean_slots": mean(tabs["n_slots"]),
            "mean_candidates": round(tabs["cand"].shape[0] / n_test, 2), "start_mean_best_fitness": mean(res["descent"]["start_fitness"]),
            "tabu_step_ms": round(tabu_step_ms, 5), "columns": cols,
            "rank_sweep": {str(m): cols[f"tabu_pairs_s{STEPS}_r{m}"]["mean_best_fitness"] for m in RANKS}}


def default_rank(configs):
    """The rank of the sweep with the lowest mean merit over the configurations, the smaller one on a tie."""
    total = {m: sum(c["rank_sweep"][str(m)] for c in configs.values()) / len(configs) for m in RANKS}
    return min(RANKS, key=lambda m: (total[m], m)), {str(m): round(v, 6) for m, v in total.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=1000)
    ap.add_argument("--configs", default="qws,normal")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--sweeps", type=int, default=16)
    ap.add_argument("--tenure", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    out = {"metric": "descend_tabu_pairs", "device": torch.cuda.get_device_name(dev), "configs": {}}
    for name in args.configs.split(","):
        out["configs"][name] = run_config(CONFIGS[name], args.problems, args.repeat, args.sweeps, args.tenure, dev)
    out["default_rank"], out["rank_sweep_mean_over_configs"] = default_rank(out["configs"])
    out["note"] = "figures of one box and one session: only ratios within the run mean anything; no test holds any of them"
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
