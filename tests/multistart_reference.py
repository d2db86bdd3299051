"""Helper of the multi-start descent tests (not a test file): the selection rule of gnnpn_descend_select_f64 and the whole stage —
tests/descent_reference.py's descent per replica, then the selection — in plain Python, and the replica tables the host and GPU
tests share."""
import functools

import numpy as np

import descent_reference as ref


def select(rows):
    """The winning replica among ``rows`` (dicts with best_fitness): the smallest value under plain <, the lowest replica among
    equals (-0.0 == 0.0); a NaN never wins; every row NaN: replica 0."""
    best = None
    for r, row in enumerate(rows):
        f = row["best_fitness"]
        if f == f and (best is None or f < rows[best]["best_fitness"]):
            best = r
    return 0 if best is None else best


def descend_starts(tables_per_replica, max_sweeps=16):
    """tables_per_replica: [(cats, bounds, start | None)] of ONE problem, one entry per replica.  Returns the winner's
    descent_reference.descend dict plus start_index and fitness_all / start_fitness_all / sweeps_all / moves_all (lists over replicas)."""
    runs = [ref.descend(*tab, max_sweeps=max_sweeps) for tab in tables_per_replica]
    w = select(runs)
    out = dict(runs[w], start_index=w)
    for key, field in (("fitness_all", "best_fitness"), ("start_fitness_all", "start_fitness"), ("sweeps_all", "sweeps"), ("moves_all", "moves")):
        out[key] = [r[field] for r in runs]
    return out


@functools.lru_cache(maxsize=None)
def replica_tables(seed, sizes, per_size, R, permute=False):
    """Per problem of test_gpu_woa._random_problems (T in ``sizes``, ``per_size`` each) R tables (cats, bounds, start): replica 0 is the
    problem's own table (a member start, a foreign pick appended to its list, or no start), replicas >= 1 start from random positions of
    replica 0's lists, and from R >= 3 on the last replica repeats replica 1 — two replicas with the same local optimum, a tie."""
    from test_gpu_woa import _random_problems
    g = np.random.default_rng(seed)
    problems = []
    for T in sizes:
        problems += _random_problems(g, T, per_size)
    if permute:
        problems = [problems[i] for i in g.permutation(len(problems))]
    out = []
    for cats, bounds, start in ref.prepare(problems):
        reps = [(cats, bounds, start)]
        for _ in range(1, R):
            reps.append((cats, bounds, [int(g.integers(0, len(c))) for c in cats]))
        if R >= 3:
            reps[-1] = reps[1]
        out.append(tuple(reps))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def replica_runs(seed, sizes, per_size, R, permute=False, max_sweeps=16):
    return tuple(descend_starts(reps, max_sweeps) for reps in replica_tables(seed, sizes, per_size, R, permute))
