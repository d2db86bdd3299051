#!/usr/bin/env python3
"""The one-swap descent beside the ES-WOA refinement it precedes, on the two configurations and the generators of
tools/bench_refine.py (1000 synthetic test problems each):

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

from bench_refine import CONFIGS, _seed_rows          # noqa: E402  (the same configurations, the same generators)


def run_config(cfg, n_test, repeat, sweeps, dev, wide=None):
    import torch
    import gnnpn_sc_amd.synth as synth
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.loadData import tables_from_dataset
    from gnnpn_sc_amd.pipeline import DeviceBatch, DeviceServices
    P = n_test * 4
    first = P // 4 * 3
    ds = synth.make_dataset(cfg["T"], cfg["S"], P, seed=1, tasks_per_problem=cfg["tasks"])
    acts = _seed_rows(ds, cfg["reduct"], np.random.default_rng(2))
    table, pb = tables_from_dataset(ds, first, None)
    svc, batch = DeviceServices.from_table(table, dev), DeviceBatch.from_problems(pb, dev)
    a = torch.from_numpy(acts).to(dev)
    sd = torch.tensor([1000 + first + i for i in range(n_test)], dtype=torch.int64, device=dev)

    def build():
        return ops.woa_candidates(svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds, a,
                                  reduct=cfg["reduct"])

    def descend(tabs):
        return ops.descend_ragged(tabs["prob_ptr"], tabs["cand_ptr"], tabs["cand"], tabs["bounds"], tabs["start_pos"], sweeps,
                                  max_slots=tabs["max_slots"], max_cand=tabs["max_cand"], wide=wide)

    def eswoa(tabs, start_pos):
        return ops.eswoa_ragged(tabs["prob_ptr"], tabs["cand_ptr"], tabs["len_init"], tabs["cand"], tabs["bounds"], start_pos,
                                cfg["pop"], cfg["iters"], sd, max_slots=tabs["max_slots"], max_cand=tabs["max_cand"], wide=wide)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return out, e0.elapsed_time(e1)

    tabs = build()                                                                     # warm-up of the three stages
    slots = torch.arange(tabs["max_slots"], device=dev)[None, :] < tabs["n_slots"][:, None]
    des = descend(tabs)
    descended_pos = des["best_pos"][slots].contiguous()
    eswoa(tabs, tabs["start_pos"])
    ms = {"builder": [], "descent": [], "eswoa": [], "eswoa_after_descent": []}
    for _ in range(repeat):
        tabs, t = timed(build)
        ms["builder"].append(t)
        des, t = timed(lambda: descend(tabs))
        ms["descent"].append(t)
        alone, t = timed(lambda: eswoa(tabs, tabs["start_pos"]))
        ms["eswoa"].append(t)
        both, t = timed(lambda: eswoa(tabs, descended_pos))
        ms["eswoa_after_descent"].append(t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    mean = lambda t: round(float(t.double().mean().item()), 6)      # noqa: E731
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
