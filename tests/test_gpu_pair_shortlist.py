"""-m gpu: pair-swap descent over shortlists on the device — gnnpn_descend_pairs_shortlist_ragged_f64 in its lane form
(descend_pairs_shortlist_kernel) and its workgroup form (descend_pairs_shortlist_wide_kernel), ops.descend_pairs_shortlist_ragged,
pipeline.descend_pairs_shortlist / descend_starts_pairs_shortlist and `main.py ... --descend --pairs --top=M` — against the
plain-Python restatement of the search (tests/pair_shortlist_reference.py): every float64, every position, every counter and every
shortlist entry, ``==``."""
import contextlib
import functools
import io
import json

import numpy as np
import pytest
import torch

import multistart_reference as mref
import pair_shortlist_reference as sref
import pair_window_reference as wref
from test_gpu_descend import N_TRAIN, P_, _tables, chain      # noqa: F401  (chain: the module-scoped fixture, set up once here)
from test_gpu_pair_descend import FIELDS, RAGGED, _assert_equal, _call_entry, _operands, _replicas, _write_cli_ini

pytestmark = pytest.mark.gpu


def _launch(dev, tables, **kw):
    from gnnpn_sc_amd import ops
    res = ops.descend_pairs_shortlist_ragged(*_operands(dev, tables), return_shortlist=True, **kw)
    return {k: v.cpu().tolist() for k, v in res.items()}


def _assert_all(got, tables, want, max_rank):
    """Every field of descend_pairs_ragged's dict, and the shortlist rows [max_slots][m] (m: the rank clamped to the longest list)."""
    _assert_equal(got, tables, want)
    max_slots = max(len(t[0]) for t in tables)
    m = min(max_rank, max(len(c) for t in tables for c in t[0]))
    for p, w in enumerate(want):
        assert got["shortlist"][p] == sref.shortlist_rows(w, max_slots, m), (p, len(tables[p][0]))


# ---- 1. the shared cases, each in the form it names ------------------------------------------------------------------------------------------

LANE_CASES = [n for n, c in sref.CASES.items() if c[2] is None]
WIDE_CASES = [n for n, c in sref.CASES.items() if c[2]]


@pytest.mark.parametrize("name", LANE_CASES)
def test_shortlist_lane_form(dev, name):
    """descend_pairs_shortlist_kernel: the 20 SEEDS tables at m = 1, 2, 4 and a full rank, with spans 1 and 3; 64 slots; a list of 139
    at m = 8 (ranked over three chunks of the wave) and m = 65 (more than a wave kept); duplicated rows; NaN merits."""
    tables, kw, _wide = sref.CASES[name]
    _assert_all(_launch(dev, list(tables), **kw), tables, sref.case_want(name), kw["max_rank"])


@pytest.mark.parametrize("name", WIDE_CASES)
def test_shortlist_workgroup_form(dev, name):
    """descend_pairs_shortlist_wide_kernel: planted(nfill=6) at 65 and 129 slots (m = 2) and 257 (span 8, m = 3); a list of 300 (ranked
    over two chunks of the workgroup); the rank-three wall across two leaf blocks of np.sum, staying at m = 2 and going at m = 3."""
    tables, kw, _wide = sref.CASES[name]
    got = _launch(dev, list(tables), **kw)
    _assert_all(got, tables, sref.case_want(name), kw["max_rank"])
    if name.startswith("third129"):
        assert got["pair_moves"] == [0 if kw["max_rank"] == 2 else 1] and got["best_pos"][0][63:65] == ([0, 0] if kw["max_rank"] == 2 else [1, 1])


# ---- 2. both forms agree ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ragged_want(max_rank, max_span=0, max_sweeps=16, max_rounds=4):
    return tuple(sref.descend_pairs(*t, max_sweeps=max_sweeps, max_rounds=max_rounds, max_span=max_span, max_rank=max_rank)
                 for t in _tables(*RAGGED))


def test_shortlist_both_forms_agree(dev):
    """The ragged batch of the pair-swap test (sizes 1 .. 33, every kind of start) at m = 3 through both forms."""
    tables, want = _tables(*RAGGED), _ragged_want(3)
    lane, wide = _launch(dev, tables, max_rank=3), _launch(dev, tables, max_rank=3, wide=True)
    _assert_all(lane, tables, want, 3)
    assert set(wide) == set(lane) and all(wide[k] == lane[k] for k in wide)
    assert any(w["pair_moves"] > 0 for w in want)


# ---- 3. a mixed ragged batch, through the C entry over sentinel-filled buffers ------------------------------------------------------------------

def _call(dev, tables, max_slots, max_cand, max_sweeps, max_rounds, max_span, max_rank, wide, shortlist=True):
    return _call_entry(dev, "gnnpn_descend_pairs_shortlist_ragged_f64", tables, max_slots, max_cand, max_sweeps, max_rounds,
                       (max_span, max_rank, wide), short=(max_rank if shortlist else None,))


@functools.lru_cache(maxsize=None)
def _mixed():
    """A one-slot problem, a problem whose every list is shorter than m = 4 (the wall), two random ones, and one of 12 slots in a
    launch sized for 9: not searched."""
    from pair_descent_reference import wall_problem
    one = ([[(0.3, 0.5, 0.9, 0.9), (0.2, 0.6, 0.9, 0.9), (0.25, 0.6, 0.9, 0.9), (0.1, 0.4, 0.9, 0.9), (0.15, 0.5, 0.9, 0.9)]], [0.0, 1.0, 0.0, 1.0], [0])
    big = wref.planted(2101, 12, wall2=(0, 11), nfill=3)
    tables = (one, wall_problem(), sref.seeds_tables()[16], big, sref.seeds_tables()[19])
    return tables, tuple(None if len(t[0]) > 9 else sref.descend_pairs(*t, max_rank=4, max_rounds=r) for r in (3, 0) for t in tables)


@pytest.mark.parametrize("wide", [0, 1])
def test_shortlist_mixed_ragged_batch(dev, wide):
    tables, wants = _mixed()
    assert [len(t[0]) for t in tables] == [1, 2, 9, 12, 9] and all(len(c) < 4 for c in tables[1][0]) and len(tables[0][0][0]) > 4
    max_cand = max(sum(len(c) for c in t[0]) for t in tables)
    for n, max_rounds in enumerate((3, 0)):
        want = wants[5 * n:5 * n + 5]
        got = _call(dev, list(tables), 9, max_cand, 16, max_rounds, 0, 4, wide)
        keep = [0, 1, 2, 4]
        _assert_equal({k: [v[p] for p in keep] for k, v in got.items()}, [tables[p] for p in keep], [want[p] for p in keep])
        for p in range(5):
            assert got["shortlist"][p] == sref.shortlist_rows(want[p], 9, 4), (p, max_rounds)     # not searched, no rounds: all -1
        assert np.isnan(got["best_fitness"][3]) and np.isnan(got["start_fitness"][3]) and all(np.isnan(h) for h in got["round_history"][3])
        assert (got["sweeps"][3], got["moves"][3], got["rounds"][3], got["pair_moves"][3], got["converged"][3]) == (-1, 0, -1, 0, 0)
        assert set(got["best_pos"][3]) == {-7} and set(np.asarray(got["best_rows"][3]).ravel()) == {-7.0}
        assert got["best_pos"][1][2:] == [-7] * 7 and -7 not in [x for p in range(5) for row in got["shortlist"][p] for x in row]
        if max_rounds == 0:
            assert all(set(x for row in got["shortlist"][p] for x in row) == {-1} for p in range(5)) and got["rounds"] == [0, 0, 0, -1, 0]
        else:
            assert -1 not in got["shortlist"][0][0] and got["shortlist"][0][1:] == [[-1] * 4] * 8 and got["shortlist"][1][:2] == [[0, 1, -1, -1]] * 2


# ---- 4. cut-offs, the optional output, no rank --------------------------------------------------------------------------------------------------

def test_shortlist_cut_offs(dev):
    tables = _tables(*RAGGED)
    for kw in ({"max_sweeps": 0}, {"max_rounds": 1}):
        want = _ragged_want(2, **kw)
        _assert_all(_launch(dev, tables, max_rank=2, **kw), tables, want, 2)
        _assert_all(_launch(dev, tables, max_rank=2, wide=True, **kw), tables, want, 2)
    assert all(w["rounds"] == 1 for w in _ragged_want(2, max_rounds=1)) and all(w["sweeps"] == 0 for w in _ragged_want(2, max_sweeps=0))


def test_shortlist_null_output_and_no_rank(dev):
    from gnnpn_sc_amd import ops
    tables = list(sref.seeds_tables())
    max_slots, max_cand = 9, max(sum(len(c) for c in t[0]) for t in tables)
    for wide in (0, 1):
        with_out, without = (_call(dev, tables, max_slots, max_cand, 16, 4, 0, 2, wide, shortlist=s) for s in (True, False))
        assert set(with_out) - set(without) == {"shortlist"} and all(with_out[k] == without[k] for k in without)
    plain = {k: v.cpu().tolist() for k, v in ops.descend_pairs_shortlist_ragged(*_operands(dev, tables), max_rank=2).items()}
    assert "shortlist" not in plain
    _assert_equal(plain, tables, sref.case_want("seeds_m2"))
    for span, wide in ((0, None), (2, None), (2, True)):      # m = 0: the windowed entry's launch, key for key
        zero = ops.descend_pairs_shortlist_ragged(*_operands(dev, tables), max_span=span, max_rank=0, wide=wide, return_shortlist=True)
        old = ops.descend_pairs_windowed_ragged(*_operands(dev, tables), max_span=span, wide=wide)
        assert zero.pop("shortlist").shape == (20, 9, 0)
        assert set(zero) == set(old) and all(torch.equal(zero[k], old[k]) for k in old)


# ---- 5. through the layers ------------------------------------------------------------------------------------------------------------------

def test_pipeline_descend_pairs_shortlist_after_run(dev, chain):      # noqa: F811
    from gnnpn_sc_amd.pipeline import descend_pairs_shortlist
    pipe, host, mins = chain["pipe"], chain["host"], chain["mins"]
    assert not any(isinstance(h, Exception) for h in host)
    tables = [(cats, bounds, start) for cats, _l, start, bounds in host]
    for span, rank in ((0, 2), (1, 1), (0, 0)):
        res = pipe.descend_pairs_shortlist(chain["svc"], chain["batch"], chain["out"], max_span=span, max_rank=rank, min_cost=mins[N_TRAIN:])
        got = {k: v.cpu().tolist() for k, v in res.items()}
        want = [sref.descend_pairs(*t, max_span=span, max_rank=rank) for t in tables]
        _assert_equal(got, tables, want)
        assert got["n_slots"] == [len(cats) for cats, _b, _s in tables]
        assert got["quality"] == [mins[N_TRAIN + b] / w["best_fitness"] for b, w in enumerate(want)]
        again = descend_pairs_shortlist(chain["svc"], chain["batch"], chain["out"], max_sweeps=16, max_rounds=4, max_span=span, max_rank=rank)
        assert all(torch.equal(again[k], res[k]) for k in again)
    old = pipe.descend_pairs(chain["svc"], chain["batch"], chain["out"], min_cost=mins[N_TRAIN:])
    assert set(old) == set(res) and all(torch.equal(old[k], res[k]) for k in old)                # no span, no rank: descend_pairs


@pytest.mark.parametrize("span,rank", [(0, 0), (2, 2)])
def test_pipeline_descend_starts_pairs_shortlist(dev, chain, monkeypatch, span, rank):      # noqa: F811
    from gnnpn_sc_amd.pipeline import descend_starts_pairs
    from test_gpu_refine import _host_tables
    pipe, svc, batch, mins = chain["pipe"], chain["svc"], chain["batch"], chain["mins"]
    monkeypatch.chdir(chain["tmp"])
    B, R = P_ - N_TRAIN, 3
    seen = _replicas(chain["ds"], chain["out"]["actions"].double().cpu().numpy(), R)
    starts = torch.from_numpy(seen).to(dev)
    host = [_host_tables("QWS", seen[:, r], 0)[0] for r in range(R)]
    assert not any(isinstance(h, Exception) for hr in host for h in hr)
    res = pipe.descend_starts_pairs_shortlist(svc, batch, starts, pair_rounds=2, pair_span=span, pair_rank=rank, min_cost=mins[N_TRAIN:])
    got = {k: v.cpu().tolist() for k, v in res.items()}
    for b in range(B):
        runs = [sref.descend_pairs(host[r][b][0], host[r][b][3], host[r][b][2], max_sweeps=16, max_rounds=2, max_span=span, max_rank=rank)
                for r in range(R)]
        w = mref.select(runs)
        T = len(host[w][b][0])
        assert got["start_index"][b] == w and got["n_slots"][b] == T, b
        for k in FIELDS:
            assert got[k][b] == runs[w][k], (b, k)
        assert got["best_pos"][b][:T] == runs[w]["best_pos"] and [tuple(r) for r in got["best_rows"][b][:T]] == runs[w]["best_rows"], b
        for k, field in (("fitness_all", "best_fitness"), ("start_fitness_all", "start_fitness"), ("sweeps_all", "sweeps"),
                         ("moves_all", "moves"), ("rounds_all", "rounds"), ("pair_moves_all", "pair_moves")):
            assert got[k][b] == [r[field] for r in runs], (b, k)
        assert got["quality"][b] == mins[N_TRAIN + b] / runs[w]["best_fitness"], b
    if span == 0 and rank == 0:                                  # descend_starts_pairs' result in every shared field
        old = descend_starts_pairs(svc, batch, starts, pair_rounds=2, min_cost=mins[N_TRAIN:])
        assert set(old) == set(res) and all(torch.equal(old[k], res[k]) for k in old)


def test_main_cli_infer_descend_pairs_top(dev, chain, monkeypatch):      # noqa: F811
    from test_gpu_refine import _actions_array, _host_tables
    tmp = chain["tmp"]
    monkeypatch.chdir(tmp)
    _write_cli_ini(tmp)
    import main as cli
    base = ["main.py", "QWS", "ML+2PN", "-1", "--infer", "--random-init", "--descend=4", "--pairs"]
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(base + ["--span=2", "--top=2"]) == 0
    with open("./solutions/WOA/QWS/ML+2PN+pairs.txt") as f:
        pairs = json.load(f)
    with open("./solutions/pretrained/QWS-PNHigh.txt") as f:
        actions = _actions_array(json.load(f))
    host, _sols, mins = _host_tables("QWS", actions, 0)
    assert not any(isinstance(h, Exception) for h in host)
    want = [sref.descend_pairs(cats, bounds, start, max_sweeps=4, max_rounds=4, max_span=2, max_rank=2) for cats, _l, start, bounds in host]
    n = P_ - N_TRAIN
    assert list(pairs) == ["quality", "time", "averageQ", "averageT", "rounds", "pair_moves", "converged", "span", "top"]
    assert pairs["span"] == 2 and pairs["top"] == 2
    assert pairs["quality"] == [mins[N_TRAIN + b] / w["best_fitness"] for b, w in enumerate(want)]
    assert len(pairs["quality"]) == n and pairs["averageQ"] == sum(pairs["quality"]) / n
    for k in ("rounds", "pair_moves", "converged"):
        assert pairs[k] == [w[k] for w in want], k
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(base + ["--top=2", "--samples=3", "--all-starts", "--seed", "3"]) == 0
    with open("./solutions/WOA/QWS/ML+2PN+multistart+pairs.txt") as f:
        multi = json.load(f)
    assert list(multi) == ["quality", "time", "averageQ", "averageT", "rounds", "pair_moves", "converged", "span", "top"]
    assert multi["span"] == 0 and multi["top"] == 2 and len(multi["quality"]) == n and all(q > 0 for q in multi["quality"])
    assert all(c in (0, 1) for c in multi["converged"]) and all(1 <= r <= 4 for r in multi["rounds"])
