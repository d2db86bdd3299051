#!/usr/bin/env python3
"""Pair-swap descent over shortlists of each slot's best candidates (gnnpn_descend_pairs_shortlist_ragged_f64): what a rank costs
in time and what it keeps of the full pair sweep's gain, every figure against the rank-0 column (the full sweep) of the SAME run.

Lane form: the two configurations, the generators and the 1000 problems of tools/bench_pairs.py (tools/search_bench.py holds them),
ranks 2, 4, 8, 16 and 0 at 1 and at 4 rounds allowed, beside one-swap descent.  Workgroup form: the planted problems of
tools/bench_pairs_window.py at 100 and 300 slots, span 16, the same ranks and rounds.

Per cell: the time by HIP events (median of --repeat after a warm-up; the wrapper's read-back of the longest list, which clamps the
rank, is inside it), the mean best_fitness, ``gain_kept`` = (descent - cell) / (descent - full sweep) over the means — the share of
the full sweep's gain over one-swap descent that the rank keeps — the mean rounds and pair_moves, the time over the full sweep's
and over one-swap descent's.  Prints one JSON line; --out writes it to a file.

    python tools/bench_pairs_shortlist.py [--problems 1000] [--configs qws,normal] [--wide-problems 32] [--slots 100,300] [--repeat 3]
                                          [--out profiles/r11_pairs_shortlist_bench.json]
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

from bench_pairs_window import flat_tables                                  # noqa: E402
from search_bench import CONFIGS, _seed_rows, mean, setup, timed            # noqa: E402

RANKS = (2, 4, 8, 16, 0)
ROUNDS = (1, 4)
SPAN = 16


def cells(tabs, sweeps, span, wide, repeat, dev):
    """{"descent": ..., "rounds_<r>": {"top_<m>": ...}} over one SearchTables."""
    def measure(fn):
        fn()                                                                           # warm-up
        ms, res = [], None
        for _ in range(repeat):
            res, t = timed(fn, dev)
            ms.append(t)
        return res, float(np.median(ms)), [round(v, 3) for v in ms]

    one, one_ms, one_all = measure(lambda: tabs.descend(sweeps, wide=wide))
    out = {"descent": {"ms": round(one_ms, 3), "ms_all": one_all, "mean_best_fitness": mean(one["best_fitness"])}}
    base = float(one["best_fitness"].double().mean().item())
    for r in ROUNDS:
        col = {}
        for m in RANKS:
            res, ms, ms_all = measure(lambda: tabs.descend_pairs_shortlist(sweeps, r, span, m, wide=wide))      # noqa: B023
            col[f"top_{m}"] = {"ms": round(ms, 3), "ms_all": ms_all, "mean_best_fitness": mean(res["best_fitness"]),
                               "fit": float(res["best_fitness"].double().mean().item()), "mean_rounds": mean(res["rounds"]),
                               "mean_pair_moves": mean(res["pair_moves"])}
        full = col["top_0"]
        for c in col.values():
            gain = base - full["fit"]
            c["gain_kept"] = round((base - c["fit"]) / gain, 4) if gain > 0 else None
            c["ms_over_full"] = round(c["ms"] / full["ms"], 3)
            c["ms_over_descent"] = round(c["ms"] / one_ms, 2)
        for c in col.values():
            del c["fit"]
        out[f"rounds_{r}"] = col
    return out


def run_config(cfg, n_test, repeat, sweeps, dev):
    import torch
    from gnnpn_sc_amd import ops
    ds, svc, batch, _first, _sd = setup(cfg, n_test, dev)
    a = torch.from_numpy(_seed_rows(ds, cfg["reduct"], np.random.default_rng(2))).to(dev)
    tabs = ops.woa_candidates(svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds, a, reduct=cfg["reduct"])
    lens = (tabs["cand_ptr"][1:] - tabs["cand_ptr"][:-1]).double()
    return {"problems": n_test, **cfg, "form": "lane", "span": 0, "max_sweeps": sweeps, "mean_slots": mean(tabs["n_slots"]),
            "mean_candidates_per_slot": round(float(lens.mean().item()), 2), "longest_list": int(lens.max().item()),
            **cells(tabs, sweeps, 0, None, repeat, dev)}


def run_slots(n_slots, n_test, repeat, sweeps, dev):
    tabs = flat_tables(n_slots, n_test, dev)
    lens = (tabs["cand_ptr"][1:] - tabs["cand_ptr"][:-1]).double()
    return {"problems": n_test, "slots": n_slots, "form": "workgroup", "span": SPAN, "max_sweeps": sweeps,
            "mean_candidates_per_slot": round(float(lens.mean().item()), 2), "longest_list": int(lens.max().item()),
            **cells(tabs, sweeps, SPAN, True, repeat, dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=1000)
    ap.add_argument("--configs", default="qws,normal")
    ap.add_argument("--wide-problems", type=int, default=32)
    ap.add_argument("--slots", default="100,300")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--sweeps", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    out = {"metric": "descend_pairs_shortlist", "device": torch.cuda.get_device_name(dev), "ranks": list(RANKS), "configs": {}, "slots": {}}
    for name in [c for c in args.configs.split(",") if c]:
        out["configs"][name] = run_config(CONFIGS[name], args.problems, args.repeat, args.sweeps, dev)
    for n in [s for s in args.slots.split(",") if s]:
        out["slots"][n] = run_slots(int(n), args.wide_problems, args.repeat, args.sweeps, dev)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
