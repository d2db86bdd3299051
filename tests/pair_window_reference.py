"""Helper of the windowed pair-swap descent tests (not a test file): the search of gnnpn_descend_pairs_windowed_ragged_f64 in plain
Python is pair_descent_reference's one statement with the slot window (``descend_pairs`` here); this module holds the planted
problems whose one-swap optima only a pair leaves, and the cases the host and the GPU tests share (reference runs cached per session)."""
import functools

import numpy as np

from pair_descent_reference import descend_pairs          # noqa: F401  the windowed entry: (..., max_span=0), the ten fields


WALL = {2: [(0.5, 0.95, 0.9, 1.0), (0.6, 0.95, 0.5, 1.0)], 3: [(0.5, 0.95, 1.0, 0.9), (0.6, 0.95, 1.0, 0.5)]}
MINS = [(0.30, 0.2, 1.0, 1.0), (0.35, 0.92, 1.0, 1.0)]


def planted(seed, T, wall2=None, wall3=None, mins=None, nfill=2):
    """(cats, bounds, start) of T slots with up to three planted pairs that no single swap takes.  Fillers: 1 .. nfill rows
    (u, 0.9 + 0.1 u', 1.0, 1.0) per slot and a random start — columns 2 and 3 are 1.0, so the products stay exact.  wall2 = (i, j):
    both slots hold WALL[2] and start at 0, column 2's product must lie in [0.2, 0.3]: the start gives 0.81 (one violation), either
    single swap 0.45 and a worse objective, both swaps 0.25.  wall3: the same on column 3.  A column without a wall is bounded by
    [0, 1].  mins = (i, j): both slots hold MINS and start at 0; they share column 1's minimum, so only raising both helps."""
    g = np.random.default_rng(seed)
    cats, start = [], []
    for _ in range(T):
        n = int(g.integers(1, nfill + 1))
        cats.append([(float(g.random()), 0.9 + 0.1 * float(g.random()), 1.0, 1.0) for _ in range(n)])
        start.append(int(g.integers(0, n)))
    bounds = [0.0, 1.0, 0.0, 1.0]
    for col, wall in ((2, wall2), (3, wall3)):
        if wall is not None:
            for s in wall:
                cats[s], start[s] = list(WALL[col]), 0
            bounds[2 * (col - 2):2 * (col - 2) + 2] = [0.2, 0.3]
    if mins is not None:
        for s in mins:
            cats[s], start[s] = list(MINS), 0
    return cats, bounds, start


# ---- the cases of tests/test_gpu_pair_window.py: name -> (max_span, [planted(...) arguments]) ------------------------------------------------
# np.sum's leaf blocks: T <= 128 one; 129: [0, 64) [64, 129); 257: [0, 128) [128, 192) [192, 257); 520: [0, 128) [128, 256)
# [256, 384) [384, 448) [448, 520).  The planted pairs straddle each kind of boundary; one per case lies inside a leaf.
SIZE_CASES = {
    65: (0, [dict(seed=6501, T=65, wall2=(3, 40), mins=(10, 64), nfill=2)]),
    128: (0, [dict(seed=12801, T=128, wall3=(0, 127), mins=(63, 64), nfill=1)]),
    129: (0, [dict(seed=12901, T=129, wall2=(63, 64), wall3=(0, 128), mins=(70, 100), nfill=1)]),
    257: (8, [dict(seed=25701, T=257, wall2=(127, 128), wall3=(191, 192), mins=(200, 207), nfill=2),
              dict(seed=25702, T=257, wall2=(126, 133), wall3=(190, 193), mins=(248, 256), nfill=2)]),
    520: (2, [dict(seed=52001, T=520, wall2=(255, 256), wall3=(383, 384), mins=(447, 448), nfill=2),
              dict(seed=52002, T=520, wall2=(127, 128), wall3=(300, 302), mins=(518, 519), nfill=2)]),
}
BEYOND = (8, [dict(seed=25703, T=257, wall2=(0, 200), wall3=(190, 193), mins=(250, 256), nfill=2)])      # wall2 lies beyond the span


def leaf_of(T, s):
    """(offset, length) of np.sum's leaf block of element s among T (numpy's pairwise recursion)."""
    off, ln = 0, T
    while ln > 128:
        n2 = ln // 2
        n2 -= n2 % 8
        if s < off + n2:
            ln = n2
        else:
            off, ln = off + n2, ln - n2
    return off, ln


@functools.lru_cache(maxsize=None)
def size_tables(T):
    return tuple(planted(**kw) for kw in SIZE_CASES[T][1])


@functools.lru_cache(maxsize=None)
def size_want(T):
    return tuple(descend_pairs(*tab, max_span=SIZE_CASES[T][0]) for tab in size_tables(T))


@functools.lru_cache(maxsize=None)
def beyond_tables():
    return tuple(planted(**kw) for kw in BEYOND[1])


@functools.lru_cache(maxsize=None)
def beyond_want():
    return tuple(descend_pairs(*tab, max_span=BEYOND[0]) for tab in beyond_tables())
