"""Helper of the shortlist pair-swap descent tests (not a test file): the search of gnnpn_descend_pairs_shortlist_ragged_f64 in plain
Python is pair_descent_reference's one statement with a rank (``descend_pairs`` here, with the ``shortlist`` key; ``shortlists``
beside it); this module holds a planted wall whose repairing row ranks third in its list, and the cases the host and the GPU
tests share (reference runs cached per session)."""
import functools
import math

import numpy as np

from descent_reference import prepare
import pair_descent_reference
from pair_descent_reference import shortlists          # noqa: F401
from pair_window_reference import WALL, planted

descend_pairs = functools.partial(pair_descent_reference.descend_pairs, with_shortlist=True)      # the shortlist entry: (..., max_span=0, max_rank=0)


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
