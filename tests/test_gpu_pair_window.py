"""-m gpu: the windowed pair-swap descent on the device — gnnpn_descend_pairs_windowed_ragged_f64 in its workgroup form
(descend_pairs_wide_kernel: 256 threads per problem, any slot count) and its lane form (descend_pairs_kernel with a span),
ops.descend_pairs_windowed_ragged, pipeline.descend_pairs_windowed and `main.py ... --descend --pairs --span=N` — against the
plain-Python restatement of the search (tests/pair_window_reference.py): every float64, every position and every counter, ``==``."""
import contextlib
import functools
import io
import json

import numpy as np
import pytest
import torch

import pair_window_reference as wref
from test_gpu_descend import N_TRAIN, P_, _tables, chain      # noqa: F401  (chain: the module-scoped fixture, set up once here)
from test_gpu_pair_descend import RAGGED, _assert_equal, _call_entry, _operands, _write_cli_ini
from test_gpu_pair_descend import _want as _pair_want

pytestmark = pytest.mark.gpu


def _launch(dev, tables, max_sweeps=16, max_rounds=4, max_span=0, **kw):
    from gnnpn_sc_amd import ops
    res = ops.descend_pairs_windowed_ragged(*_operands(dev, tables), max_sweeps=max_sweeps, max_rounds=max_rounds, max_span=max_span, **kw)
    return {k: v.cpu().tolist() for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def _want(key, max_span, max_sweeps=16, max_rounds=4):
    return tuple(wref.descend_pairs(*tab, max_sweeps=max_sweeps, max_rounds=max_rounds, max_span=max_span) for tab in _tables(*key))


# ---- 1. slot counts in the workgroup form, planted pairs ----------------------------------------------------------------------------------

@pytest.mark.parametrize("T", sorted(wref.SIZE_CASES))
def test_pair_window_workgroup_sizes(dev, T):
    """65 and 128: one leaf block of np.sum through the workgroup code.  129: two leaves.  257: three, the paths of a pair part at
    the root or one level down.  520: five leaves, an uneven tree of depth 3.  Full sweeps up to 129, span 8 at 257, span 2 at 520;
    the planted pairs straddle every leaf boundary and one per case lies inside a leaf (test_pair_window_host.py asserts it)."""
    span = wref.SIZE_CASES[T][0]
    tables, want = wref.size_tables(T), wref.size_want(T)
    got = _launch(dev, list(tables), max_span=span)
    _assert_equal(got, tables, want)
    assert all(m > 0 for m in got["pair_moves"]) and got["converged"] == [1] * len(tables)


# ---- 2. the window in both forms -------------------------------------------------------------------------------------------------------------

LANE = (1500, (2, 5, 9, 33), 2, 6, True)


@pytest.mark.parametrize("span", [1, 3, 0])
def test_pair_window_lane_form_spans(dev, span):
    from gnnpn_sc_amd import ops
    tables, want = _tables(*LANE), _want(LANE, span)
    got = _launch(dev, tables, max_span=span)
    _assert_equal(got, tables, want)
    if span == 0:                                          # the existing entry, field for field
        old = {k: v.cpu().tolist() for k, v in ops.descend_pairs_ragged(*_operands(dev, tables)).items()}
        assert set(old) == set(got) and all(old[k] == got[k] for k in old)
        assert any(w["pair_moves"] > 0 for w in want)
    else:                                                  # ... and the workgroup form keeps to the same window
        _assert_equal(_launch(dev, tables, max_span=span, wide=True), tables, want)


def test_the_spans_differ_on_the_lane_batch():
    runs = [_want(LANE, s) for s in (1, 3, 0)]
    assert any(a["best_pos"] != b["best_pos"] for a, b in zip(runs[0], runs[2])) and any(w["pair_moves"] > 0 for w in runs[0])


def test_pair_window_wall_beyond_the_span_remains(dev):
    tables, want = wref.beyond_tables(), wref.beyond_want()
    got = _launch(dev, list(tables), max_span=wref.BEYOND[0])
    _assert_equal(got, tables, want)
    assert got["converged"] == [1] and 1.0 < got["best_fitness"][0] < 2.0 and got["best_pos"][0][0] == 0 and got["best_pos"][0][200] == 0


# ---- 3. both forms agree ------------------------------------------------------------------------------------------------------------------

def test_pair_window_both_forms_agree(dev):
    """The ragged batch of the pair-swap test (sizes 1 .. 33, every kind of start) through the workgroup form: the lane form's result
    and the reference's."""
    tables, want = _tables(*RAGGED), _pair_want(RAGGED)
    wide, lane = _launch(dev, tables, wide=True), _launch(dev, tables)
    _assert_equal(wide, tables, want)
    assert set(wide) == set(lane) and all(wide[k] == lane[k] for k in wide)


# ---- 4. a mixed ragged batch ----------------------------------------------------------------------------------------------------------------

MIXED = (1600, (1, 2, 33, 64, 65, 130), 4, 4, True)       # four per size: every fourth problem of a size has no start
MIXED_SPAN = 3
MIXED_PLANTED = (dict(seed=1601, T=65, wall2=(61, 64), mins=(30, 31), nfill=1), dict(seed=1602, T=130, wall3=(63, 64), mins=(126, 129), nfill=1))


@functools.lru_cache(maxsize=None)
def _mixed():
    tables = list(_tables(*MIXED)) + [wref.planted(**kw) for kw in MIXED_PLANTED]
    order = np.random.default_rng(1603).permutation(len(tables))
    tables = tuple(tables[i] for i in order)
    return tables, tuple(wref.descend_pairs(*tab, max_span=MIXED_SPAN) for tab in tables)


def test_pair_window_mixed_ragged_batch(dev):
    tables, want = _mixed()
    assert sorted({len(t[0]) for t in tables}) == [1, 2, 33, 64, 65, 130]
    assert any(t[2] is None for t in tables) and sum(w["pair_moves"] > 0 for w in want) >= 2
    _assert_equal(_launch(dev, list(tables), max_span=MIXED_SPAN), tables, want)


# ---- 5. pair products beyond the workgroup ---------------------------------------------------------------------------------------------------

def _long_lists(T, i, j):
    """A wall on column 2 between slots i and j whose lists hold 40 rows: the repairing row stands at positions 6 and 25 of each, so
    the four tied best products k = a * 40 + b are 246, 265, 1006 and 1025 — four different chunks of 256 in the workgroup form (in
    waves 3, 0, 3, 0: the lowest k sits in a higher wave than the next), four different chunks of 64 in the lane form; the lowest
    (a, b) = (6, 6) wins."""
    cats, bounds, start = wref.planted(1700 + T, T, nfill=1)
    poor, fix = wref.WALL[2]
    for s in (i, j):
        cats[s] = [poor] + [(0.9 - 0.001 * c, 0.95, 0.9, 1.0) for c in range(39)]      # worse objectives, the same product
        cats[s][6] = cats[s][25] = fix
        start[s] = 0
    bounds[0:2] = [0.2, 0.3]
    return cats, bounds, start


def test_pair_window_products_beyond_the_workgroup(dev):
    tabs = [_long_lists(70, 10, 50), _long_lists(12, 2, 9)]
    want = [wref.descend_pairs(*t) for t in tabs]
    for t, w in zip(tabs, want):
        assert len(t[0][10 if len(t[0]) == 70 else 2]) == 40 and w["pair_moves"] == 1
    assert [want[0]["best_pos"][s] for s in (10, 50)] == [6, 6] and [want[1]["best_pos"][s] for s in (2, 9)] == [6, 6]
    ks = [a * 40 + b for a in (6, 25) for b in (6, 25)]
    assert len({k // 256 for k in ks}) == 4 and [(k % 256) // 64 for k in ks] == [3, 0, 3, 0] and len({k // 64 for k in ks}) == 4
    assert 40 * 40 > 6 * 256                                                        # seven chunks of the workgroup
    _assert_equal(_launch(dev, tabs[:1]), tabs[:1], want[:1])                        # 70 slots: the workgroup form
    _assert_equal(_launch(dev, tabs[1:]), tabs[1:], want[1:])                        # its lane-form twin
    _assert_equal(_launch(dev, tabs[1:], wide=True), tabs[1:], want[1:])


# ---- 6. cut-offs ---------------------------------------------------------------------------------------------------------------------

def test_pair_window_cut_offs(dev):
    from gnnpn_sc_amd import ops
    tables, full = wref.size_tables(129), wref.size_want(129)
    assert full[0]["rounds"] == 2                                                   # one round moves, the next finds nothing
    zero = _launch(dev, list(tables), max_rounds=0)
    one = {k: v.cpu().tolist() for k, v in ops.descend_ragged(*_operands(dev, tables), wide=True).items()}
    for k in ("best_fitness", "start_fitness", "best_pos", "best_rows", "sweeps", "moves"):
        assert zero[k] == one[k], k
    assert zero["round_history"] == [[f] for f in one["best_fitness"]]
    assert zero["rounds"] == [0] and zero["pair_moves"] == [0] and zero["converged"] == [0]
    cut = _launch(dev, list(tables), max_rounds=1)
    _assert_equal(cut, tables, [wref.descend_pairs(*t, max_rounds=1) for t in tables])
    assert cut["converged"] == [0] and cut["rounds"] == [1] and cut["round_history"] == [[full[0]["best_fitness"]]]
    tables = wref.size_tables(65)
    pairs_only = _launch(dev, list(tables), max_sweeps=0)
    _assert_equal(pairs_only, tables, [wref.descend_pairs(*t, max_sweeps=0) for t in tables])
    assert pairs_only["sweeps"] == [0] and pairs_only["moves"] == [0] and pairs_only["converged"] == [0] and pairs_only["pair_moves"][0] > 0


# ---- 7. a problem the launch was not sized for -------------------------------------------------------------------------------------------

def test_pair_window_not_searched(dev):
    """The C entry itself, over buffers filled with a sentinel: a batch sized max_slots = 65 whose prob_ptr gives one problem 66 slots.
    That row is NaN / -1 / 0 with rounds -1 and every round_history entry NaN, its best_pos / best_rows rows untouched; the
    neighbours are right and nothing past a row's count is written."""
    small, big, mid = _tables(1207, (7,), 4, 8)[2], wref.planted(1801, 66, wall2=(0, 65), nfill=1), wref.size_tables(65)[0]
    tables = [small, big, mid]
    assert [len(t[0]) for t in tables] == [7, 66, 65]
    for max_rounds, ld in ((0, 1), (3, 3)):
        got = _call_entry(dev, "gnnpn_descend_pairs_windowed_ragged_f64", tables, 65, 0, 16, max_rounds, (0, 0))
        want = [wref.descend_pairs(*t, max_rounds=max_rounds) for t in (small, mid)]
        _assert_equal({k: [v[0], v[2]] for k, v in got.items()}, [small, mid], want)
        assert np.isnan(got["best_fitness"][1]) and np.isnan(got["start_fitness"][1]) and all(np.isnan(h) for h in got["round_history"][1])
        assert len(got["round_history"][1]) == ld
        assert (got["sweeps"][1], got["moves"][1], got["rounds"][1], got["pair_moves"][1], got["converged"][1]) == (-1, 0, -1, 0, 0)
        assert set(got["best_pos"][1]) == {-7} and set(np.asarray(got["best_rows"][1]).ravel()) == {-7.0}
        assert -7.0 not in [h for row in got["round_history"] for h in row]
        assert got["best_pos"][0][7:] == [-7] * 58 and set(np.asarray(got["best_rows"][0][7:]).ravel()) == {-7.0}


# ---- 8. through the layers ------------------------------------------------------------------------------------------------------------------

def test_pipeline_descend_pairs_windowed_after_run(dev, chain):      # noqa: F811
    from gnnpn_sc_amd.pipeline import descend_pairs_windowed
    pipe, host, mins = chain["pipe"], chain["host"], chain["mins"]
    assert not any(isinstance(h, Exception) for h in host)
    tables = [(cats, bounds, start) for cats, _l, start, bounds in host]
    for span in (1, 0):
        res = pipe.descend_pairs_windowed(chain["svc"], chain["batch"], chain["out"], max_span=span, min_cost=mins[N_TRAIN:])
        got = {k: v.cpu().tolist() for k, v in res.items()}
        want = [wref.descend_pairs(*t, max_span=span) for t in tables]
        _assert_equal(got, tables, want)
        assert got["n_slots"] == [len(cats) for cats, _b, _s in tables]
        assert got["quality"] == [mins[N_TRAIN + b] / w["best_fitness"] for b, w in enumerate(want)]
        again = descend_pairs_windowed(chain["svc"], chain["batch"], chain["out"], max_sweeps=16, max_rounds=4, max_span=span)
        assert all(torch.equal(again[k], res[k]) for k in again)
    old = pipe.descend_pairs(chain["svc"], chain["batch"], chain["out"], min_cost=mins[N_TRAIN:])
    assert set(old) == set(res) and all(torch.equal(old[k], res[k]) for k in old)                # span 0 is descend_pairs


def test_main_cli_infer_descend_pairs_span(dev, chain, monkeypatch):      # noqa: F811
    from test_gpu_refine import _actions_array, _host_tables
    tmp = chain["tmp"]
    monkeypatch.chdir(tmp)
    _write_cli_ini(tmp)
    import main as cli
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["main.py", "QWS", "ML+2PN", "-1", "--infer", "--random-init", "--descend=4", "--pairs", "--span=2"]) == 0
    with open("./solutions/WOA/QWS/ML+2PN+pairs.txt") as f:
        pairs = json.load(f)
    with open("./solutions/pretrained/QWS-PNHigh.txt") as f:
        actions = _actions_array(json.load(f))
    host, _sols, mins = _host_tables("QWS", actions, 0)
    assert not any(isinstance(h, Exception) for h in host)
    want = [wref.descend_pairs(cats, bounds, start, max_sweeps=4, max_rounds=4, max_span=2) for cats, _l, start, bounds in host]
    n = P_ - N_TRAIN
    assert list(pairs) == ["quality", "time", "averageQ", "averageT", "rounds", "pair_moves", "converged", "span"] and pairs["span"] == 2
    assert pairs["quality"] == [mins[N_TRAIN + b] / w["best_fitness"] for b, w in enumerate(want)]
    assert len(pairs["quality"]) == n and pairs["averageQ"] == sum(pairs["quality"]) / n
    for k in ("rounds", "pair_moves", "converged"):
        assert pairs[k] == [w[k] for w in want], k
