#!/usr/bin/env python3
"""What naming the services of a searched composition costs, and what scoring one given as ids costs, beside the builder and the
descent of the SAME run (gnnpn_woa_candidates_services, gnnpn_search_services, gnnpn_services_merit_f64).

Lane form: the two configurations, the generators and the 1000 problems of tools/bench_pairs.py (tools/search_bench.py holds them):
the builder alone (ops.woa_candidates), the builder with its ids (ops.woa_candidates_named: one launch more), one-swap descent,
the mapping of its result (SearchTables.services) and the scorer (ops.services_merit) over what the mapping named.  Workgroup
form: the planted problems of tools/bench_pairs_window.py at 100 and 300 slots — flat tables that no builder made, so the ids
are the candidates' own positions in the table, which stands for the service table: descent, mapping and scorer.

Per cell the time by HIP events (median of --repeat after a warm-up; a wrapper's small copies to the host are inside it).  The
scorer's merit is compared with the descent's best_fitness on the way (``certified``: equal bit for bit in every problem — with
foreign rows left unnamed in the lane runs, those problems are counted apart).  Prints one JSON line; --out writes it to a file.

    python tools/bench_services.py [--problems 1000] [--configs qws,normal] [--wide-problems 32] [--slots 100,300] [--repeat 5]
                                   [--out profiles/r12_services_bench.json]
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
from search_bench import CONFIGS, _seed_rows, setup, timed                  # noqa: E402


def measure(fn, repeat, dev):
    fn()                                                                               # warm-up
    ms, res = [], None
    for _ in range(repeat):
        res, t = timed(fn, dev)
        ms.append(t)
    return res, {"ms": round(float(np.median(ms)), 3), "ms_all": [round(v, 3) for v in ms]}


def certified(merit, fit):
    """(problems whose merit is the descent's best_fitness bit for bit, the others) among the searched ones."""
    import torch
    searched = ~fit.isnan()
    same = merit.view(torch.int64) == fit.view(torch.int64)
    return int((same & searched).sum().item()), int((~same & searched).sum().item())


def run_config(cfg, n_test, repeat, sweeps, dev):
    import torch
    from gnnpn_sc_amd import ops
    ds, svc, batch, _first, _sd = setup(cfg, n_test, dev)
    a = torch.from_numpy(_seed_rows(ds, cfg["reduct"], np.random.default_rng(2))).to(dev)
    operands = (svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds, a)
    N = batch.x.shape[0]
    _tabs, t_build = measure(lambda: ops.woa_candidates(*operands, reduct=cfg["reduct"]), repeat, dev)
    tabs, t_named = measure(lambda: ops.woa_candidates_named(*operands, reduct=cfg["reduct"]), repeat, dev)
    res, t_descent = measure(lambda: tabs.descend(sweeps), repeat, dev)
    got, t_map = measure(lambda: tabs.services(res, batch.seg_ptr, N), repeat, dev)
    (merit, _n), t_score = measure(lambda: ops.services_merit(batch.seg_ptr, got["node_services"], svc.qos, batch.global_bounds, True,
                                                              max_slots=tabs["max_slots"]), repeat, dev)
    pos = tabs.flat(res["best_pos"])
    unnamed = (got["best_services"] < 0) & (torch.arange(tabs["max_slots"], device=dev)[None, :] < tabs["n_slots"][:, None])
    same, other = certified(merit, res["best_fitness"])
    return {"problems": n_test, **cfg, "form": "lane", "max_sweeps": sweeps, "nodes": N, "lists": int(pos.numel()),
            "candidates": int(tabs["cand"].shape[0]), "builder": t_build, "builder_named": t_named, "descent": t_descent,
            "mapping": t_map, "scorer": t_score,
            "naming_over_builder_and_descent": round((t_named["ms"] - t_build["ms"] + t_map["ms"]) / (t_build["ms"] + t_descent["ms"]), 4),
            "scorer_over_builder_and_descent": round(t_score["ms"] / (t_build["ms"] + t_descent["ms"]), 4),
            "problems_with_an_unnamed_foreign_row": int(unnamed.any(1).sum().item()), "certified": same, "not_certified": other}


def run_slots(n_slots, n_test, repeat, sweeps, dev):
    import torch
    from gnnpn_sc_amd import ops
    tabs = flat_tables(n_slots, n_test, dev)
    I32 = torch.int32
    n_cand = tabs["cand"].shape[0]
    tabs.update(cand_service=torch.arange(n_cand, dtype=I32, device=dev), slot_cat=torch.zeros(n_test * n_slots, dtype=I32, device=dev),
                slot_node=(torch.arange(n_slots, dtype=I32, device=dev) + 1).repeat(n_test).contiguous())
    seg_ptr = (torch.arange(n_test + 1, dtype=I32, device=dev) * (n_slots + 1)).contiguous()
    N = n_test * (n_slots + 1)
    res, t_descent = measure(lambda: tabs.descend(sweeps, wide=True), repeat, dev)
    got, t_map = measure(lambda: tabs.services(res, seg_ptr, N), repeat, dev)
    (merit, _n), t_score = measure(lambda: ops.services_merit(seg_ptr, got["node_services"], tabs["cand"], tabs["bounds"], False,
                                                              max_slots=n_slots), repeat, dev)
    same, other = certified(merit, res["best_fitness"])
    return {"problems": n_test, "slots": n_slots, "form": "workgroup", "max_sweeps": sweeps, "candidates": int(n_cand), "descent": t_descent,
            "mapping": t_map, "scorer": t_score, "mapping_over_descent": round(t_map["ms"] / t_descent["ms"], 4),
            "scorer_over_descent": round(t_score["ms"] / t_descent["ms"], 4), "certified": same, "not_certified": other}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=1000)
    ap.add_argument("--configs", default="qws,normal")
    ap.add_argument("--wide-problems", type=int, default=32)
    ap.add_argument("--slots", default="100,300")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    out = {"metric": "services", "device": torch.cuda.get_device_name(dev), "configs": {}, "slots": {}}
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
