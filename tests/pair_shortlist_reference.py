"""Helper of the shortlist pair-swap descent tests (not a test file): the search of gnnpn_descend_pairs_shortlist_ragged_f64 in plain
Python — pair_window_reference.descend_pairs whose pair sweeps look only at a shortlist of each slot's best candidates — built on
descent_reference.descend and merit, a planted wall whose repairing row ranks third in its list, and the cases the host and the GPU
tests share (reference runs cached per session)."""
import functools
import math

import numpy as np

from descent_reference import descend, merit, prepare
from pair_descent_reference import _settled
from pair_window_reference import WALL, planted


def shortlists(cats, bounds, cur, m):
    """Per slot s the min(m, len) candidates c with the lowest merit of ``cur`` with slot s alone replaced by c — ordered by (merit,
    position) under plain <, a NaN after every number and NaNs by position, -0.0 equal to 0.0 — as ascending positions."""
    rows = [cats[s][cur[s]] for s in range(len(cats))]
    out = []
    for s, cat in enumerate(cats):
        keyed = []
        for c, row in enumerate(cat):
            rows[s] = row
            f = merit(rows, bounds)
            keyed.append((f != f, 0.0 if f != f else f, c))
        rows[s] = cat[cur[s]]
        out.append(sorted(c for _n, _f, c in sorted(keyed)[:m]))
    return out


def descend_pairs(cats, bounds, start, max_sweeps=16, max_rounds=4, max_span=0, max_rank=0):
    """pair_window_reference.descend_pairs whose pair sweep, where max_rank = m > 0, forms ``shortlists`` of the composition it starts
    from and tries only (a, b) of S_i x S_j, in the order of k = ia * |S_j| + ib, the lowest k among equals; the shortlists stay as
    formed through the sweep.  The dict gains ``shortlist``: the last sweep's shortlists (None: no pair sweep ran, or m = 0)."""
    T = len(cats)
    r = descend(cats, bounds, start, max_sweeps)
    cur, fit, start_fitness = list(r["best_pos"]), r["best_fitness"], r["start_fitness"]
    sweeps, moves, settled = r["sweeps"], r["moves"], _settled(r)
    rounds, pair_moves, round_history, moved, lists = 0, 0, [], True, None
    for _ in range(max_rounds):
        moved = False
        rows = [cats[s][cur[s]] for s in range(T)]
        lists = shortlists(cats, bounds, cur, max_rank) if max_rank > 0 else None
        short = lists if lists is not None else [range(len(cat)) for cat in cats]
        for i in range(T):
            for j in range(i + 1, min(T, i + max_span + 1) if max_span > 0 else T):
                best_f, best_ab = math.inf, None
                for a in short[i]:
                    rows[i] = cats[i][a]
                    for b in short[j]:
                        rows[j] = cats[j][b]
                        f = merit(rows, bounds)
                        if f < best_f:
                            best_f, best_ab = f, (a, b)
                if best_ab is not None and best_f < fit:         # strictly
                    cur[i], cur[j] = best_ab
                    fit = best_f
                    pair_moves += 1
                    moved = True
                rows[i], rows[j] = cats[i][cur[i]], cats[j][cur[j]]
        rounds += 1
        if moved:
            r = descend(cats, bounds, cur, max_sweeps)
            cur, fit = list(r["best_pos"]), r["best_fitness"]
            sweeps += r["sweeps"]
            moves += r["moves"]
            settled = _settled(r)
        round_history.append(fit)
        if not moved:
            break
    round_history += [fit] * (max(max_rounds, 1) - len(round_history))
    return {"best_fitness": fit, "start_fitness": start_fitness, "best_pos": cur,
            "best_rows": [tuple(cats[s][cur[s]]) for s in range(T)], "sweeps": sweeps, "moves": moves, "rounds": rounds,
            "pair_moves": pair_moves, "round_history": round_history, "converged": int(rounds > 0 and not moved and settled),
            "shortlist": lists}


def shortlist_rows(want, max_slots, m):
    """``want["shortlist"]`` as the [max_slots][m] rows of the C entry's output: -1 past a shortlist's length and past T, all -1
    where no pair sweep ran (``want`` None: a problem that is not searched)."""
    lists = (want or {}).get("shortlist") or []
    rows = []
    for s in range(max_slots):
        kept = list(lists[s])[:m] if s < len(lists) else []
        rows.append(kept + [-1] * (m - len(kept)))
    return rows


THIRD = (0.55, 0.95, 0.9, 1.0)      # between WALL[2]'s two rows in the objective, with the poor row's factor in column 2


def rank_three_wall(seed, T, i, j, nfill=2):
    """planted(seed, T, wall2=(i, j)) whose two wall lists are [poor, fix, THIRD]: from the start (poor, poor) the single swaps rank
    poor < THIRD < fix in both lists (all three leave the violation, the objective grows with column 0), so the repairing row at
    position 1 ranks exactly third: shortlists of two hold positions [0, 2] and the wall stays, shortlists of three let it go."""
    cats, bounds, start = planted(seed, T, wall2=(i, j), nfill=nfill)
    poor, fix = WALL[2]
    for s in (i, j):
        cats[s] = [poor, fix, THIRD]
    return cats, bounds, start


def duplicated_rows():
    """(cats, bounds, start) of three slots whose lists repeat rows: pair_descent_reference.wall_problem(twice=True)'s two walls
    [poor, fix, fix] with a worse row behind them, and a filler list whose best row stands twice.  The single swaps rank poor, fix
    (position 1), fix (position 2), worse: shortlists of two keep the LOWER of the two equal rows, shortlists of three keep both, and
    of the four tied pairs the lowest k wins."""
    a, b, z = (0.5, 0.5, 0.9, 1.0), (0.6, 0.5, 0.5, 1.0), (0.9, 0.5, 0.9, 1.0)
    fill = [(0.4, 0.9, 1.0, 1.0), (0.2, 0.9, 1.0, 1.0), (0.2, 0.9, 1.0, 1.0), (0.3, 0.9, 1.0, 1.0)]
    return [[a, b, b, z], fill, [a, b, b, z]], [0.2, 0.3, 0.0, 1.0], [0, 0, 0]


def nan_row_problem():
    """Four slots; the second list holds two rows whose column 0 is NaN (positions 0 and 2 of five) and starts at a finite row: their
    single-swap merits are NaN (np.sum), every other figure of the composition is finite.  NaNs rank last, by position."""
    g = np.random.default_rng(77)
    cats = [[(float(g.random()), 0.9 + 0.1 * float(g.random()), 1.0, 1.0) for _ in range(5)] for _ in range(4)]
    cats[1][0] = (math.nan,) + cats[1][0][1:]
    cats[1][2] = (math.nan,) + cats[1][2][1:]
    return cats, [0.0, 1.0, 0.0, 1.0], [1, 1, 2, 3]


def seeds_tables():
    """The 20 tables of test_pair_descend_host.SEEDS (T = 2, 3, 7, 8, 9; lists of 1 .. 8)."""
    from test_gpu_woa import _random_problems
    from test_pair_descend_host import SEEDS
    out = []
    for seed, sizes, per, mc in SEEDS:
        g = np.random.default_rng(seed)
        for T in sizes:
            out += prepare(_random_problems(g, T, per, mc))
    return out


@functools.lru_cache(maxsize=None)
def _seeds_tables():
    return tuple(seeds_tables())


def _long_tables():
    """One problem of three slots with lists of 139, 70 and 5 rows (139: two chunks of 64 and a rest of 11 in the lane form), rows
    and bounds as test_gpu_woa._random_problems draws them."""
    g = np.random.default_rng(139)
    cats = [[tuple(float(v) for v in np.r_[g.random(2), 1.0 - g.random(2) * 0.2 / 3]) for _ in range(n)] for n in (139, 70, 5)]
    return ((cats, [0.95, 1.0, 0.95, 1.0], [int(g.integers(0, len(c))) for c in cats]),)


def _t64_tables():
    from test_gpu_descend import _tables
    return _tables(1964, (64,), 2, 7)          # 64 slots, lists of 1 .. 6 (+ a foreign pick)


def long_list_wide(T=70, s=20, n=300):
    """planted(T) with one list of ``n`` rows (more than the 256 threads of the workgroup form): objectives fall towards the end of
    the list, so the best single swaps stand in its second chunk."""
    cats, bounds, start = planted(1900 + T, T, wall2=(3, 8), nfill=4)
    g = np.random.default_rng(1901)
    cats[s] = [(0.9 - 0.002 * c + 0.001 * float(g.random()), 0.95, 1.0, 1.0) for c in range(n)]
    start[s] = 5
    return cats, bounds, start


# name -> (tables, dict(max_span=, max_rank=, ...), wide)
def _cases():
    c = {}
    for m in (1, 2, 4, 8):
        c[f"seeds_m{m}"] = (_seeds_tables(), dict(max_rank=m), None)
    c["t64_m2"] = (_t64_tables(), dict(max_rank=2), None)
    c["long_m8"] = (_long_tables(), dict(max_rank=8), None)
    c["long_m65"] = (_long_tables(), dict(max_rank=65), None)
    c["dup_m2"] = ((duplicated_rows(),), dict(max_rank=2), None)
    c["dup_m2_first_sweep"] = ((duplicated_rows(),), dict(max_rank=2, max_rounds=1), None)
    c["dup_m3"] = ((duplicated_rows(),), dict(max_rank=3), None)
    c["nan_m4"] = ((nan_row_problem(),), dict(max_rank=4), None)
    for span in (1, 3):
        c[f"seeds_span{span}_m2"] = (_seeds_tables(), dict(max_rank=2, max_span=span), None)
    c["wide65_m2"] = ((planted(6501, 65, wall2=(3, 40), mins=(10, 64), nfill=6),), dict(max_rank=2), True)
    c["wide129_m2"] = ((planted(12901, 129, wall2=(63, 64), wall3=(0, 128), mins=(70, 100), nfill=6),), dict(max_rank=2), True)
    c["wide257_span8_m3"] = ((planted(25701, 257, wall2=(127, 128), wall3=(191, 192), mins=(200, 207), nfill=6),),
                             dict(max_rank=3, max_span=8), True)
    c["wide_long_m8"] = ((long_list_wide(),), dict(max_rank=8, max_span=8), True)
    c["third129_m2"] = ((rank_three_wall(12902, 129, 63, 64, nfill=1),), dict(max_rank=2), True)
    c["third129_m3"] = ((rank_three_wall(12902, 129, 63, 64, nfill=1),), dict(max_rank=3), True)
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def case_want(name):
    tables, kw, _wide = CASES[name]
    return tuple(descend_pairs(*tab, **kw) for tab in tables)
