#!/usr/bin/env python3
"""Multi-start descent — descent from N start compositions per problem, the lowest local optimum kept — on the two configurations
and the generators of tools/search_bench.py, over tools/bench_descend.py's 1000 synthetic test problems and over the first 256 of them:

    qws     47 categories, 2507 services, 10 tasks, reduct 0,    pop 50, 250 iterations
    normal  50 categories, 5000 services, 10 tasks, reduct 0.55, pop 60, 500 iterations

Starts: replica 0 is bench_descend's ``_seed_rows(ds, reduct, default_rng(2))`` (so the N = 1 row repeats its descent row on the same
box), replica r the same generator seeded 2 + r.  They are SYNTHETIC: random members of every task's candidate list, not samples of a
trained policy (the repository has no trained weights) — what a policy's samples are worth stays unmeasured.

For N in --replicas: the three stages by HIP events (median of --repeat after a warm-up of each shape) — the table builder over B * N
rows (gnnpn_woa_candidates_replicas_count + _fill), one descent launch over the rows (gnnpn_descend_ragged_f64), the selection
(gnnpn_descend_select_f64) — problems/s, the mean merit of the winners, the share of problems won by a replica >= 1, and the time
over the N = 1 time of the same run.  Beside them, in the same run: ES-WOA alone and descent (N = 1) + ES-WOA.  Prints one JSON line.
One box, one session: only the ratios within a run mean anything.

    python tools/bench_multistart.py [--problems 1000,256] [--configs qws,normal] [--replicas 1,2,4,8,16] [--repeat 3] [--sweeps 16]
"""
import argparse
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from search_bench import CONFIGS, _seed_rows, dataset, mean, setup, timed          # noqa: E402

N_TEST = 1000       # bench_descend's problems: the test quarter of a data set of 4000


def _start_rows(job):
    name, r = job
    cfg = CONFIGS[name]
    return _seed_rows(dataset(cfg, N_TEST), cfg["reduct"], np.random.default_rng(2 + r))


def make_starts(names, n_replicas):
    """{config: [N_TEST, n_replicas, T, 8] float64}; on the host, in worker processes, before the GPU is opened."""
    jobs = [(name, r) for name in names for r in range(n_replicas)]
    with ProcessPoolExecutor(max_workers=min(8, len(jobs))) as ex:
        rows = list(ex.map(_start_rows, jobs))
    return {name: np.stack([rows[i] for i, (n, _r) in enumerate(jobs) if n == name], axis=1) for name in names}


def run_config(cfg, ds, starts, n_test, replicas, repeat, sweeps, dev):
    import torch
    from gnnpn_sc_amd import ops
    _ds, svc, batch, _first, sd = setup(cfg, N_TEST, dev, last=n_test, ds=ds)
    a_all = torch.from_numpy(starts[:n_test]).to(dev)
    operands = (svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds)
    rows = []
    for N in replicas:
        a = a_all[:, :N].contiguous()
        build = lambda: ops.woa_candidates_replicas(*operands, a, reduct=cfg["reduct"])      # noqa: E731
        tabs = build()                                                                     # warm-up of the three stages at this shape
        per_row = tabs.descend(sweeps)
        win = ops.descend_select(per_row, a, tabs["n_slots"])
        ms = {"builder": [], "descent": [], "select": []}
        for _ in range(repeat):
            tabs, t = timed(build, dev)
            ms["builder"].append(t)
            per_row, t = timed(lambda: tabs.descend(sweeps), dev)
            ms["descent"].append(t)
            win, t = timed(lambda: ops.descend_select(per_row, a, tabs["n_slots"]), dev)
            ms["select"].append(t)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        total = sum(med.values())
        rows.append({"replicas": N, "builder_ms": round(med["builder"], 3), "descent_ms": round(med["descent"], 3),
                     "select_ms": round(med["select"], 3), "total_ms": round(total, 3), "problems_per_s": round(n_test / (total * 1e-3), 1),
                     "mean_candidates_per_row": round(tabs["cand"].shape[0] / (n_test * N), 2),
                     "mean_winner_merit": mean(win["best_fitness"]), "mean_winner_start_merit": mean(win["start_fitness"]),
                     "won_by_replica_ge_1": round(float((win["start_index"] > 0).double().mean().item()), 4),
                     "mean_sweeps_per_row": mean(per_row["sweeps"])})
    for r in rows:      # the ratios the run is for: N starts over one start, within this run
        r["total_over_one_start"] = round(r["total_ms"] / rows[0]["total_ms"], 3) if rows[0]["replicas"] == 1 else None
        r["descent_over_one_start"] = round(r["descent_ms"] / rows[0]["descent_ms"], 3) if rows[0]["replicas"] == 1 else None

    # the comparison of tools/bench_descend.py in the same run: ES-WOA alone, and descent (one start) + ES-WOA
    tabs = ops.woa_candidates(*operands, a_all[:, 0].contiguous(), reduct=cfg["reduct"])
    des = tabs.descend(sweeps)
    descended_pos = tabs.flat(des["best_pos"])
    tabs.eswoa(cfg["pop"], cfg["iters"], sd)
    ms = {"eswoa": [], "eswoa_after_descent": []}
    for _ in range(repeat):
        alone, t = timed(lambda: tabs.eswoa(cfg["pop"], cfg["iters"], sd), dev)
        ms["eswoa"].append(t)
        both, t = timed(lambda: tabs.eswoa(cfg["pop"], cfg["iters"], sd, descended_pos), dev)
        ms["eswoa_after_descent"].append(t)
    return {"problems": n_test, **cfg, "max_sweeps": sweeps, "mean_slots": mean(tabs["n_slots"]),
            "start": {"mean_best_fitness": mean(des["start_fitness"])}, "multistart": rows,
            "eswoa": {"ms": round(float(np.median(ms["eswoa"])), 3), "mean_best_fitness": mean(alone[0])},
            "descent_plus_eswoa": {"eswoa_ms": round(float(np.median(ms["eswoa_after_descent"])), 3), "mean_best_fitness": mean(both[0])}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="1000,256")
    ap.add_argument("--configs", default="qws,normal")
    ap.add_argument("--replicas", default="1,2,4,8,16")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--sweeps", type=int, default=16)
    args = ap.parse_args()
    names = args.configs.split(",")
    replicas = [int(v) for v in args.replicas.split(",")]
    starts = make_starts(names, max(replicas))
    import torch
    dev = torch.device("cuda:0")
    out = {"metric": "multistart", "starts": "synthetic (_seed_rows, default_rng(2 + replica)): no trained policy", "configs": {}}
    for name in names:
        ds = dataset(CONFIGS[name], N_TEST)
        out["configs"][name] = {str(n): run_config(CONFIGS[name], ds, starts[name], int(n), replicas, args.repeat, args.sweeps, dev)
                                for n in args.problems.split(",")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
