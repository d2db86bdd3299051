"""-m gpu: the eight descent builds at the edge of a CU's LDS.  The host asks for the bytes that the kernels' own carve-up takes
(descend.hip: lane_carve, wide_carve), so the byte counts are checked where they decide something: at the largest size the formulas
below accept — the layout written out as plain arithmetic, not read off the code under test — one problem runs and equals the
plain-Python restatement of its search in every float64 and position, ``==``; one size up is refused before any launch, GNNPN_E_UNSUP,
with the byte count in the message.  In these problems all candidates but one per other slot stand in one long list, so a sweep costs
thousands of evaluations, and the shortlists, the tabu table and the best composition lie at the far end of what was asked for."""
import math

import numpy as np
import pytest

import descent_reference as ref
import pair_descent_reference as pref
import tabu_reference as tref
from pair_window_reference import planted
from test_gpu_pair_descend import _operands

pytestmark = pytest.mark.gpu

LIMIT = 160 * 1024 - 1024          # what search_launch gives a problem: a CU's LDS less 1 KB
HINT = "; wide=1 keeps the candidate table in global memory"


def lane_bytes(n):
    """Four columns [4][64] and bounds [4] f64, base / len / cur [64] i32, the table [n][4] f64."""
    return (260 + 4 * n) * 8 + 3 * 64 * 4


def wide_bytes(T, sib_rows):
    """Four columns [T], red [8], bounds [4], sib [sib_rows][32] f64; cnt [4], base / len [T] i32."""
    return (4 * T + 12 + 32 * sib_rows) * 8 + (2 * T + 4) * 4


# build -> (bytes(T = max_slots, n = max_cand, m = rank) per form, the entry's name in its messages per form)
BYTES = {
    "one_swap": ({"lane": lambda T, n, m: lane_bytes(n), "wide": lambda T, n, m: wide_bytes(T, 1)}, "descend_ragged", "descend_ragged"),
    "pairs": ({"lane": lambda T, n, m: lane_bytes(n), "wide": lambda T, n, m: wide_bytes(T, 3)},
              "descend_pairs_ragged", "descend_pairs_windowed_ragged"),
    # ... plus mer [n] f64, rk [n] i32, list [T][m] i32
    "shortlist": ({"lane": lambda T, n, m: lane_bytes(n) + 12 * n + 4 * T * m, "wide": lambda T, n, m: wide_bytes(T, 3) + 12 * n + 4 * T * m},
                  "descend_pairs_shortlist_ragged", "descend_pairs_shortlist_ragged"),
    # ... plus expire [n] i32, best [64 | T] i32
    "tabu": ({"lane": lambda T, n, m: lane_bytes(n) + 4 * (n + 64), "wide": lambda T, n, m: wide_bytes(T, 1) + 4 * (n + T)},
             "descend_tabu_ragged", "descend_tabu_ragged"),
}
RANK = {"shortlist": 2}
# (build, form, the size taken to the edge): the lane form by its candidates, the workgroup form by its slots — and, where its
# candidates size something too, by them as well
CASES = [(b, "lane", "cand") for b in BYTES] + [(b, "wide", "slots") for b in BYTES] + [("shortlist", "wide", "cand"), ("tabu", "wide", "cand")]


def _largest(fits):
    """The largest size ``fits`` accepts (it is monotone)."""
    lo, hi = 1, 1 << 20
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


def _long_list(seed, n, T=3):
    """(cats, bounds, start) of T slots and n candidates: a list of n - T + 1 rows, then lists of one row; bounds some products break."""
    g = np.random.default_rng(seed)
    row = lambda: (float(g.random()), float(g.random()), 0.5 + 0.5 * float(g.random()), 0.5 + 0.5 * float(g.random()))      # noqa: E731
    cats = [[row() for _ in range(n - T + 1)]] + [[row()] for _ in range(T - 1)]
    return cats, [0.3, 0.8, 0.3, 0.8], [int(g.integers(0, n - T + 1))] + [0] * (T - 1)


def _case(build, form, edge):
    """(table, max_slots, max_cand, rank, the edge's size one up as (max_slots, max_cand)) of a case."""
    nbytes, m = BYTES[build][0][form], RANK.get(build, 0)
    if form == "lane":
        T = 3
        n = _largest(lambda n: nbytes(T, n, min(m, n)) <= LIMIT)
        return _long_list(4000 + len(build), n, T), T, n, m, (T, n + 1)
    table = planted(12900 + len(build), 129, wall2=(63, 64), wall3=(0, 128), mins=(70, 72), nfill=2)      # np.sum's recursion: two leaves
    n_own = sum(len(c) for c in table[0])
    if edge == "slots":
        T = _largest(lambda T: nbytes(T, n_own, m) <= LIMIT)
        return table, T, n_own, m, (T + 1, n_own)
    n = _largest(lambda n: nbytes(129, n, m) <= LIMIT)
    return table, 129, n, m, (129, n + 1)


def test_the_edges_are_where_the_layout_puts_them():
    """The sizes the cases run at, by hand: 4999 candidates fill the lane form ((260 + 4 n) 8 + 768 <= 162816)."""
    assert LIMIT == 162816 and lane_bytes(4999) == 162816 and _case("one_swap", "lane", "cand")[2] == _case("pairs", "lane", "cand")[2] == 4999
    assert _case("tabu", "lane", "cand")[2] == 4436 and lane_bytes(4436) + 4 * 4500 == 162800          # 36 n + 3104
    assert _case("shortlist", "lane", "cand")[2] == 3635 and lane_bytes(3635) + 12 * 3635 + 4 * 3 * 2 == 162812      # 44 n + 2872
    assert _case("one_swap", "wide", "slots")[1] == 4061 and wide_bytes(4061, 1) == 162808            # 40 T + 368
    assert _case("pairs", "wide", "slots")[1] == 4048 and wide_bytes(4048, 3) == 162800               # 40 T + 880


SEARCH = {"max_sweeps": 3}
OPTIONS = {"one_swap": {}, "pairs": {"max_rounds": 1}, "shortlist": {"max_rounds": 1, "max_span": 2}, "tabu": {"max_steps": 4, "tenure": 2}}


def _want(build, table, rank):
    cats, bounds, start = table
    if build == "one_swap":
        return ref.descend(cats, bounds, start, **SEARCH)
    if build == "tabu":
        return tref.descend_tabu(cats, bounds, start, **SEARCH, **OPTIONS[build])
    return pref.descend_pairs(cats, bounds, start, **SEARCH, **OPTIONS[build], max_rank=rank)


def _run(dev, build, form, table, max_slots, max_cand, rank):
    from gnnpn_sc_amd import ops
    kw = dict(SEARCH, **OPTIONS[build], max_slots=max_slots, max_cand=max_cand)
    if build == "pairs" and form == "lane":
        res = ops.descend_pairs_ragged(*_operands(dev, [table]), **kw)                        # the entry with the lane form only
    else:
        entry = {"one_swap": ops.descend_ragged, "pairs": ops.descend_pairs_windowed_ragged, "shortlist": ops.descend_pairs_shortlist_ragged,
                 "tabu": ops.descend_tabu_ragged}[build]
        res = entry(*_operands(dev, [table]), **kw, **({"max_rank": rank} if build == "shortlist" else {}), wide=form == "wide")
    return {k: v.cpu().tolist() for k, v in res.items()}


def _message(build, form, nbytes, T, n, rank):
    who = BYTES[build][1 if form == "lane" else 2]
    if build == "shortlist":
        return f"{who}: {nbytes} B of LDS per problem ({T} slots, {n} candidates, shortlists of {rank}) exceed a CU (160 KB)" + HINT * (form == "lane")
    if build == "tabu":
        return f"{who}: {nbytes} B of LDS per problem ({T} slots, {n} candidates) exceed a CU (160 KB)" + HINT * (form == "lane")
    if form == "wide":
        return f"{who}: {T} slots need {nbytes} B of LDS for the four QoS columns (a CU has 160 KB)"
    return f"{who}: {nbytes} B of LDS per problem ({n} candidates) exceed a CU" + HINT * (build == "one_swap")


@pytest.mark.parametrize("build,form,edge", CASES)
def test_a_build_runs_at_the_edge_and_is_refused_one_size_up(dev, build, form, edge):
    from gnnpn_sc_amd import _lib, ops
    table, max_slots, max_cand, rank, (up_slots, up_cand) = _case(build, form, edge)
    nbytes = BYTES[build][0][form]
    assert nbytes(max_slots, max_cand, rank) <= LIMIT < nbytes(up_slots, up_cand, rank)
    T = len(table[0])
    want = _want(build, table, rank)
    got = _run(dev, build, form, table, max_slots, max_cand, rank)
    print(build, form, edge, "max_slots", max_slots, "max_cand", max_cand, "bytes", nbytes(max_slots, max_cand, rank),
          {k: want[k] for k in ("best_fitness", "start_fitness", "sweeps", "moves")})
    for k, w in want.items():
        g = got[k][0]
        if k == "best_pos":
            assert g[:T] == w and len(g) == max_slots
        elif k == "best_rows":
            assert [tuple(r) for r in g[:T]] == w
        elif k == "walk":
            assert g[:len(w)] == w and all(math.isnan(v) for v in g[len(w):])
        else:
            assert g == w, (k, g, w)                                                           # the merits, the counters, the histories
    assert want["moves"] > 0                                                                   # something was searched
    with pytest.raises(ops.GnnpnError) as e:                                                  # refused on the host: nothing is launched
        _run(dev, build, form, table, up_slots, up_cand, rank)
    entry = str(e.value).split(" failed ")[0]
    assert str(e.value) == f"{entry} failed ({_lib.E_UNSUP}): " + _message(build, form, nbytes(up_slots, up_cand, rank), up_slots, up_cand, rank)
