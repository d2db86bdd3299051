#!/usr/bin/env python3
"""The pair-swap descent beside the one-swap descent it extends and the ES-WOA refinement both precede, on the two configurations,
the generators and the 1000 problems of tools/bench_descend.py (tools/search_bench.py holds them):

    qws     47 categories, 2507 services, 10 tasks, reduct 0,    pop 50, 250 iterations
    normal  50 categories, 5000 services, 10 tasks, reduct 0.55, pop 60, 500 iterations

Columns: the table builder, descent (gnnpn_descend_ragged_f64), pair descent with 1 and with 4 rounds allowed
(gnnpn_descend_pairs_ragged_f64), ES-WOA from the tables' start, ES-WOA from the descended and from the pair-descended (4 rounds)
composition.  Per column the time by HIP events (median of --repeat after a warm-up of every launch), the mean best_fitness and
the share of problems whose final merit still holds a violation (best_fitness >= 1); for the pair columns also the mean rounds and
pair_moves, the share of problems with pair_moves > 0 and the share that converged.  Prints one JSON line; --out writes it to a file.

    python tools/bench_pairs.py [--problems 1000] [--configs qws,normal] [--repeat 3] [--sweeps 16] [--out profiles/r09_pairs_bench.json]
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

ROUNDS = (1, 4)


def run_config(cfg, n_test, repeat, sweeps, dev):
    import torch
    from gnnpn_sc_amd import ops
    ds, svc, batch, _first, sd = setup(cfg, n_test, dev)
    a = torch.from_numpy(_seed_rows(ds, cfg["reduct"], np.random.default_rng(2))).to(dev)

    def build():
        return ops.woa_candidates(svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds, a,
                                  reduct=cfg["reduct"])

    tabs = build()                                                                     # warm-up of every launch
    descended_pos = tabs.flat(tabs.descend(sweeps)["best_pos"])
    paired_pos = {r: tabs.flat(tabs.descend_pairs(sweeps, r)["best_pos"]) for r in ROUNDS}[ROUNDS[-1]]
    tabs.eswoa(cfg["pop"], cfg["iters"], sd)
    names = ["builder", "descent"] + [f"pairs_{r}" for r in ROUNDS] + ["eswoa", "eswoa_after_descent", "eswoa_after_pairs"]
    ms, res = {k: [] for k in names}, {}
    for _ in range(repeat):
        tabs, t = timed(build, dev)
        ms["builder"].append(t)
        res["descent"], t = timed(lambda: tabs.descend(sweeps), dev)
        ms["descent"].append(t)
        for r in ROUNDS:
            res[f"pairs_{r}"], t = timed(lambda: tabs.descend_pairs(sweeps, r), dev)          # noqa: B023
            ms[f"pairs_{r}"].append(t)
        for name, start in (("eswoa", None), ("eswoa_after_descent", descended_pos), ("eswoa_after_pairs", paired_pos)):
            out, t = timed(lambda: tabs.eswoa(cfg["pop"], cfg["iters"], sd, start), dev)       # noqa: B023
            res[name] = {"best_fitness": out[0]}
            ms[name].append(t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    cols = {"builder": {"ms": round(med["builder"], 3)}}
    for name in names[1:]:
        r = res[name]
        col = {"ms": round(med[name], 3), "ms_all": [round(v, 3) for v in ms[name]], "mean_best_fitness": mean(r["best_fitness"]),
               "violated_share": share(r["best_fitness"] >= 1.0)}
        if "sweeps" in r:
            col.update(mean_sweeps=mean(r["sweeps"]), mean_moves=mean(r["moves"]))
        if "rounds" in r:
            col.update(mean_rounds=mean(r["rounds"]), mean_pair_moves=mean(r["pair_moves"]), moved_by_pairs_share=share(r["pair_moves"] > 0),
                       converged_share=share(r["converged"] > 0))
        cols[name] = col
    last = f"pairs_{ROUNDS[-1]}"
    return {"problems": n_test, **cfg, "max_sweeps": sweeps, "mean_slots": mean(tabs["n_slots"]),
            "mean_candidates": round(tabs["cand"].shape[0] / n_test, 2), "start_mean_best_fitness": mean(res["descent"]["start_fitness"]),
            "columns": cols,
            "pairs_over_descent": {f"rounds_{r}": round(med[f"pairs_{r}"] / med["descent"], 2) for r in ROUNDS},
            "pairs_over_eswoa": {f"rounds_{r}": round(med[f"pairs_{r}"] / med["eswoa"], 4) for r in ROUNDS},
            "pairs_never_worse_than_descent": bool((res[last]["best_fitness"] <= res["descent"]["best_fitness"]).all().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=1000)
    ap.add_argument("--configs", default="qws,normal")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--sweeps", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    out = {"metric": "descend_pairs", "device": torch.cuda.get_device_name(dev), "configs": {}}
    for name in args.configs.split(","):
        out["configs"][name] = run_config(CONFIGS[name], args.problems, args.repeat, args.sweeps, dev)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
