#!/usr/bin/env python3
"""The ES-WOA refinement of ML+2PN solutions: the host path (loadDataOther + WOA._prepare + WOA.fine_tune, what
`main.py <ds> WOA` runs) against pipeline.refine = ML2PNPipeline.refine (candidate builder + ragged search on the device), in problems/s over
1000 synthetic test problems, in two configurations:

    qws     47 categories, 2507 services, 10 tasks, reduct 0,    pop 50, 250 iterations
    normal  50 categories, 5000 services, 10 tasks, reduct 0.55, pop 60, 500 iterations

The seed rows are members of each task's candidate list (a tenth foreign), dummy rows for absent categories.  The device
figures split the builder (gnnpn_woa_candidates_count + _fill, its one read-back of the totals included) from the search
(gnnpn_eswoa_ragged_f64) by HIP events; the host figures are wall clock (its search is the same kernel, one launch per
task count).  Both paths are also checked to give the same qualities.  Prints one JSON line.

    python tools/bench_refine.py [--problems 1000] [--configs qws,normal] [--repeat 3]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from search_bench import CONFIGS, _seed_rows          # noqa: E402,F401  (re-exported: whoever imported them from here still can)


def run_config(name, cfg, n_test, repeat, dev):
    import torch
    import gnnpn_sc_amd.synth as synth
    from gnnpn_sc_amd import WOA, ops
    from gnnpn_sc_amd.loadData import loadDataOther, tables_from_dataset
    from gnnpn_sc_amd.pipeline import DeviceBatch, DeviceServices, refine
    P = n_test * 4
    ds = synth.make_dataset(cfg["T"], cfg["S"], P, seed=1, tasks_per_problem=cfg["tasks"])
    tmp = tempfile.mkdtemp(prefix="bench_refine_")
    synth.write_dataset(tmp, "QWS", ds)
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        first = P // 4 * 3
        acts = _seed_rows(ds, cfg["reduct"], np.random.default_rng(2))
        seeds = [1000 + first + i for i in range(n_test)]
        # host path, as WOA.WOA.start runs it (the rows already in memory: the JSON round trip is not counted)
        t0 = time.perf_counter()
        sols = [[r for r in acts[b, :, :4].tolist() if sum(r) != 3] for b in range(n_test)]
        ssets = [{tuple(round(v, 5) for v in r) for r in s} for s in sols]
        feats, cons, mins = loadDataOther("QWS", cfg["reduct"], sSetList=ssets)
        t1 = time.perf_counter()
        res = WOA.fine_tune([(feats[i], cons[i], sols[i] or None) for i in range(n_test)], cfg["pop"], cfg["iters"], seeds, dev)
        t2 = time.perf_counter()
        host_q = [mins[first + i] / r["bestFitness"] for i, r in enumerate(res)]
        # device path
        table, pb = tables_from_dataset(ds, first, None)
        svc, batch = DeviceServices.from_table(table, dev), DeviceBatch.from_problems(pb, dev)
        a = torch.from_numpy(acts).to(dev)
        sd = torch.tensor(seeds, dtype=torch.int64, device=dev)
        mc = torch.tensor(mins[first:first + n_test], dtype=torch.float64, device=dev)
        out = refine(svc, batch, {"actions": a}, cfg["pop"], cfg["iters"], reduct=cfg["reduct"], seeds=sd, min_cost=mc)  # warm-up
        same = out["quality"].cpu().tolist() == host_q
        walls, builds, searches = [], [], []
        for _ in range(repeat):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            torch.cuda.synchronize(dev)
            w0 = time.perf_counter()
            e0.record()
            tabs = ops.woa_candidates(svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds, a,
                                      reduct=cfg["reduct"])
            e1.record()
            tabs.eswoa(cfg["pop"], cfg["iters"], sd)
            e2.record()
            torch.cuda.synchronize(dev)
            walls.append(time.perf_counter() - w0)
            builds.append(e0.elapsed_time(e1))
            searches.append(e1.elapsed_time(e2))
            torch.cuda.synchronize(dev)
        w0 = time.perf_counter()
        refine(svc, batch, {"actions": a}, cfg["pop"], cfg["iters"], reduct=cfg["reduct"], seeds=sd, min_cost=mc)["quality"].cpu()
        refine_wall = time.perf_counter() - w0
    finally:
        os.chdir(cwd)
    med = lambda v: float(np.median(v))      # noqa: E731
    return {"problems": n_test, **cfg,
            "host_problems_per_s": round(n_test / (t2 - t0), 1), "host_prep_s": round(t1 - t0, 3), "host_search_s": round(t2 - t1, 3),
            "device_problems_per_s": round(n_test / med(walls), 1), "device_wall_ms": round(1e3 * med(walls), 3),
            "builder_ms": round(med(builds), 3), "search_ms": round(med(searches), 3),
            "refine_call_ms": round(1e3 * refine_wall, 3), "same_quality_as_host": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=1000)
    ap.add_argument("--configs", default="qws,normal")
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    out = {"metric": "eswoa_refine", "configs": {}}
    for name in args.configs.split(","):
        out["configs"][name] = run_config(name, CONFIGS[name], args.problems, args.repeat, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
