#!/usr/bin/env python3
"""The windowed pair-swap descent in its workgroup form at large slot counts, beside the two stages that already run there — wide
one-swap descent and wide ES-WOA — on the same problems in the same run.  Problems of T = 100, 300 and 1000 slots with about 5
candidates per slot: the per-slot shape of bench.py's synth4 workload (1000 tasks, 5000 services in 1000 categories).  The table
builder follows the reference's addS, which holds 50 categories, so problems beyond 64 slots reach the searches as flat tables only
(as in the tests of the wide kernels); tools/search_bench.py has no generator of those, ``flat_tables`` below is one: 3 .. 7 rows
(u1, 0.9 + 0.1 u2, 1, 1) per slot and a random member as the start, and per problem three planted slot pairs that no single swap
takes (a violated bound on each product, and column 1's minimum), their slots 1, 3, 10 or 40 apart — so a span of 1, 4 or 16
reaches some of them and the full sweep all.  Random tables alone show nothing here: at 65 slots and more their one-swap optima
leave no improving pair.

Columns per T: descent (gnnpn_descend_ragged_f64, wide), pairs_span_1 / 4 / 16 (gnnpn_descend_pairs_windowed_ragged_f64, wide, --rounds
rounds allowed), pairs_full (span 0) where its time, estimated from the span-16 column by the number of pairs, stays under
--full-limit-s, and eswoa (gnnpn_eswoa_ragged_f64, wide, pop 50, 250 iterations, from the same start).  Per column the time by HIP events (median of
--repeat after a warm-up), the mean best_fitness and the share of problems that still hold a violation; for the pair columns also
the mean rounds and pair_moves and the share that converged.  Prints one JSON line; --out writes it to a file.

    python tools/bench_pairs_window.py [--problems 32] [--slots 100,300,1000] [--repeat 3] [--out profiles/r10_pairs_window_bench.json]
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

from search_bench import mean, share, timed          # noqa: E402

POP, ITERS = 50, 250                                  # the qws configuration's ES-WOA budget
SPANS = (1, 4, 16)
GAPS = (1, 3, 10, 40)                                 # how far apart a planted pair's slots lie: within span 1, 4, 16, or none of them
# What only a pair move leaves (rows of two slots, both starting at row 0).  2 / 3: a wall on that column — its product must lie in
# [0.2, 0.3], the start gives 0.81, either single swap 0.45 and a worse objective, both swaps 0.25.  1: the two slots share column
# 1's minimum, so only raising both helps.
PLANTED = {2: [(0.5, 0.95, 0.9, 1.0), (0.6, 0.95, 0.5, 1.0)], 3: [(0.5, 0.95, 1.0, 0.9), (0.6, 0.95, 1.0, 0.5)],
           1: [(0.30, 0.2, 1.0, 1.0), (0.35, 0.92, 1.0, 1.0)]}


def flat_tables(n_slots, n_problems, dev, seed=3):
    """A SearchTables of ``n_problems`` problems of ``n_slots`` slots each (see above), on ``dev``."""
    import torch
    from gnnpn_sc_amd import ops
    g = np.random.default_rng(seed + n_slots)
    lens = g.integers(3, 8, size=n_problems * n_slots)
    start = (g.random(lens.size) * lens).astype(np.int64)
    rows, bounds = [], np.tile([0.2, 0.3, 0.2, 0.3], (n_problems, 1))
    for p in range(n_problems):
        planted = {}
        for kind, gap in zip((2, 3, 1), g.choice(GAPS, size=3)):         # a wall on column 2, one on column 3, the shared minimum
            free = [s for s in range(n_slots - gap) if s not in planted and s + gap not in planted]
            s = int(g.choice(free))
            planted[s] = planted[s + gap] = kind
        for s in range(n_slots):
            q = p * n_slots + s
            if s in planted:
                lens[q], start[q] = 2, 0
                rows += PLANTED[planted[s]]
            else:
                rows += [(g.random(), 0.9 + 0.1 * g.random(), 1.0, 1.0) for _ in range(lens[q])]
    cand_ptr = np.r_[0, np.cumsum(lens)]
    cand = np.asarray(rows, dtype=np.float64)
    t = lambda arr, dt: torch.as_tensor(np.ascontiguousarray(arr), dtype=dt).to(dev)      # noqa: E731
    I32, F64 = torch.int32, torch.float64
    per_problem = cand_ptr[n_slots::n_slots] - cand_ptr[:-1:n_slots]
    return ops.SearchTables(prob_ptr=t(np.arange(n_problems + 1) * n_slots, I32), n_slots=t(np.full(n_problems, n_slots), I32),
                            cand_ptr=t(cand_ptr, I32), len_init=t(lens, I32), cand=t(cand, F64), start_pos=t(start, I32),
                            bounds=t(bounds, F64), max_slots=n_slots, max_cand=int(per_problem.max()))


def run_slots(n_slots, n_test, repeat, sweeps, rounds, full_limit_s, dev):
    import torch
    tabs = flat_tables(n_slots, n_test, dev)
    sd = torch.arange(1000, 1000 + n_test, dtype=torch.int64, device=dev)
    calls = {"descent": lambda: tabs.descend(sweeps, wide=True)}
    for s in SPANS:
        calls[f"pairs_span_{s}"] = lambda s=s: tabs.descend_pairs_windowed(sweeps, rounds, s, wide=True)
    calls["eswoa"] = lambda: {"best_fitness": tabs.eswoa(POP, ITERS, sd, wide=True)[0]}
    ms, res, skipped = {}, {}, {}

    def measure(name, fn):
        fn()                                                                           # warm-up
        ms[name] = []
        for _ in range(repeat):
            res[name], t = timed(fn, dev)
            ms[name].append(t)

    for name, fn in calls.items():
        measure(name, fn)
    # the full sweep has T (T - 1) / 2 pairs where span s has about T s: estimate before running it
    last = SPANS[-1]
    est_s = float(np.median(ms[f"pairs_span_{last}"])) / 1000.0 * max(1.0, (n_slots - 1) / (2.0 * last))
    if est_s <= full_limit_s:
        measure("pairs_full", lambda: tabs.descend_pairs_windowed(sweeps, rounds, 0, wide=True))
    else:
        skipped["pairs_full"] = f"estimated {round(est_s, 1)} s per launch from the span-{last} column, above --full-limit-s {full_limit_s}"
    cols = {}
    for name, r in res.items():
        col = {"ms": round(float(np.median(ms[name])), 3), "ms_all": [round(v, 3) for v in ms[name]],
               "mean_best_fitness": mean(r["best_fitness"]), "violated_share": share(r["best_fitness"] >= 1.0)}
        if "sweeps" in r:
            col.update(mean_sweeps=mean(r["sweeps"]), mean_moves=mean(r["moves"]))
        if "rounds" in r:
            col.update(mean_rounds=mean(r["rounds"]), mean_pair_moves=mean(r["pair_moves"]), converged_share=share(r["converged"] > 0))
        cols[name] = col
    return {"problems": n_test, "slots": n_slots, "pop": POP, "iters": ITERS, "max_sweeps": sweeps, "max_rounds": rounds, "mean_slots": mean(tabs["n_slots"]),
            "max_slots": tabs["max_slots"], "mean_candidates_per_slot": round(tabs["cand"].shape[0] / max(int(tabs["n_slots"].sum().item()), 1), 2),
            "start_mean_best_fitness": mean(res["descent"]["start_fitness"]), "columns": cols, "skipped": skipped}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=32)
    ap.add_argument("--slots", default="100,300,1000")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--sweeps", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--full-limit-s", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    out = {"metric": "descend_pairs_windowed", "device": torch.cuda.get_device_name(dev), "slots": {}}
    for n in args.slots.split(","):
        out["slots"][n] = run_slots(int(n), args.problems, args.repeat, args.sweeps, args.rounds, args.full_limit_s, dev)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
