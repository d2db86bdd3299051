"""-m gpu: the tabu walk over pair moves on the device — gnnpn_descend_tabu_pairs_ragged_f64 in its lane form
(descend_tabu_pairs_kernel) and its workgroup form (descend_tabu_pairs_wide_kernel), ops.descend_tabu_pairs_ragged,
pipeline.descend_tabu_pairs / descend_starts_tabu_pairs and `main.py ... --descend --tabu --pair-moves` — against the plain-Python
restatement of the search (tests/tabu_pairs_reference.py): every float64, every position and every counter of every problem, ``==``."""
import contextlib
import io
import json
import math

import numpy as np
import pytest
import torch

import multistart_reference as mref
import pair_descent_reference as pref
import pair_shortlist_reference as sref
import tabu_pairs_reference as tpref
import tabu_reference as tref
from test_gpu_descend import N_TRAIN, P_, chain      # noqa: F401  (chain: the module-scoped fixture, set up once here)
from test_gpu_pair_descend import _operands, _replicas, _write_cli_ini

pytestmark = pytest.mark.gpu


def _launch(dev, tables, **kw):
    from gnnpn_sc_amd import ops
    res = ops.descend_tabu_pairs_ragged(*_operands(dev, list(tables)), **kw)
    return {k: v.cpu().tolist() for k, v in res.items()}


def _assert_problem(got, p, cats, w, max_steps):
    """Every field of problem ``p`` against the reference run ``w``: history over its max_steps columns, walk over the steps taken
    and NaN behind them."""
    T = len(cats)
    for k in tpref.FIELDS:
        assert got[k][p] == w[k], (p, T, k, got[k][p], w[k])
    assert got["best_pos"][p][:T] == w["best_pos"], (p, T)
    assert [tuple(r) for r in got["best_rows"][p][:T]] == w["best_rows"], (p, T)
    assert got["history"][p] == w["history"][:max_steps], (p, T)
    assert len(got["walk"][p]) == max_steps and got["walk"][p][:w["steps"]] == w["walk"], (p, T, got["walk"][p], w["walk"])
    assert all(math.isnan(v) for v in got["walk"][p][w["steps"]:]), (p, T)


def _assert_all(got, tables, want, max_steps):
    assert len(got["steps"]) == len(tables) == len(want)
    for p, ((cats, _b, _s), w) in enumerate(zip(tables, want)):
        _assert_problem(got, p, cats, w, max_steps)


def _same(a, b):
    """Two result dicts of tensors, bit for bit (NaN equal to NaN)."""
    return set(a) == set(b) and all(torch.equal(a[k].view(torch.int64) if a[k].dtype == torch.float64 else a[k],
                                                b[k].view(torch.int64) if b[k].dtype == torch.float64 else b[k]) for k in a)


# ---- 1. the shared cases, each in the form it names ------------------------------------------------------------------------------------------

LANE_CASES = [n for n, c in tpref.CASES.items() if c[2] is None]
WIDE_CASES = [n for n, c in tpref.CASES.items() if c[2]]


@pytest.mark.parametrize("name", LANE_CASES)
def test_tabu_pairs_lane_form(dev, name):
    """descend_tabu_pairs_kernel: the 20 SEEDS tables as one ragged batch at no steps, at two steps (the polish), at 32 steps with
    ranks 1, 2, 4 (with a span of 1) and whole lists (no tenure), once without phase 0; duplicated rows (a single before an equal
    pair), NaN merits, T = 1, lists of one row, the wall (crossed in one step); 64 slots; lists of 139 / 70 / 5 ranked in chunks."""
    tables, kw, _wide = tpref.CASES[name]
    _assert_all(_launch(dev, tables, **kw), tables, tpref.case_want(name), kw["max_steps"])


@pytest.mark.parametrize("name", WIDE_CASES)
def test_tabu_pairs_workgroup_form(dev, name):
    """descend_tabu_pairs_wide_kernel: the lane cases' batches again (the same reference runs: both forms give the same walk); a list
    of 300 (more than the workgroup); planted(nfill=6) at 65, 129 and 257 slots — a pair 37 slots apart, a pair across two leaves of
    np.sum, three leaf blocks with the parting node above the leaves; the wall across two leaves at 131 slots, taken as one pair."""
    tables, kw, _wide = tpref.CASES[name]
    got = _launch(dev, tables, wide=True, **kw)
    _assert_all(got, tables, tpref.case_want(name), kw["max_steps"])
    if name == "wall131":
        assert got["best_step"] == [1] and got["pair_steps"] == [1] and got["stalled"] == [1] and got["best_pos"][0][63:65] == [1, 1]


def test_tabu_pairs_both_forms_and_two_runs_give_identical_tensors(dev):
    from gnnpn_sc_amd import ops
    operands = _operands(dev, list(sref._seeds_tables()))
    lane, again, wide = (ops.descend_tabu_pairs_ragged(*operands, max_steps=32, tenure=3, max_rank=2, wide=w) for w in (None, None, True))
    assert _same(lane, again) and _same(lane, wide)
    assert lane["history"].shape == (20, 32) and lane["walk"].shape == (20, 32) and lane["walk"].dtype == torch.float64
    assert lane["pair_steps"].shape == (20,) and lane["pair_steps"].dtype == torch.int32 and int(lane["pair_steps"].sum()) > 0


def test_tabu_pairs_no_steps_is_descend_ragged(dev):
    from gnnpn_sc_amd import ops
    operands = _operands(dev, list(sref._seeds_tables()))
    for wide in (None, True):
        one = ops.descend_ragged(*operands, wide=wide)
        got = ops.descend_tabu_pairs_ragged(*operands, max_steps=0, tenure=3, max_rank=2, wide=wide)
        for k in ("best_fitness", "start_fitness", "best_pos", "best_rows", "sweeps", "moves"):
            assert torch.equal(got[k], one[k]), k
        assert got["history"].shape == (20, 0) and got["walk"].shape == (20, 0)
        assert got["steps"].tolist() == [0] * 20 and got["best_step"].tolist() == [0] * 20 and got["stalled"].tolist() == [0] * 20
        assert got["pair_steps"].tolist() == [0] * 20


# ---- 2. a ragged batch with a problem that is not searched, through the C entry over sentinel-filled buffers ---------------------------------

def _call(dev, tables, max_slots, max_cand, max_sweeps, max_steps, tenure, max_span, max_rank, wide):
    from gnnpn_sc_amd import _lib, ops
    ops_in = _operands(dev, list(tables))
    B, ld = len(tables), max(max_steps, 1)
    F64, I32 = torch.float64, torch.int32
    f = {"best_fitness": torch.full((B,), -7.0, dtype=F64, device=dev), "start_fitness": torch.full((B,), -7.0, dtype=F64, device=dev),
         "best_rows": torch.full((B, max_slots, 4), -7.0, dtype=F64, device=dev), "history": torch.full((B, ld), -7.0, dtype=F64, device=dev),
         "walk": torch.full((B, ld), -7.0, dtype=F64, device=dev)}
    i = {k: torch.full((B,), -7, dtype=I32, device=dev) for k in ("sweeps", "moves", "steps", "best_step", "stalled", "pair_steps")}
    i["best_pos"] = torch.full((B, max_slots), -7, dtype=I32, device=dev)
    ops.check(_lib.load().gnnpn_descend_tabu_pairs_ragged_f64(
        B, ops.dev_ptr(ops_in[0], I32, "prob_ptr"), ops_in[4].numel(), max_slots, max_cand, ops.dev_ptr(ops_in[1], I32, "cand_ptr"),
        ops.dev_ptr(ops_in[2], F64, "cand"), ops.dev_ptr(ops_in[3], F64, "bounds"), ops.dev_ptr(ops_in[4], I32, "start_pos"),
        max_sweeps, max_steps, tenure, max_span, max_rank, wide, ops.dev_ptr(f["best_fitness"], F64, "f"),
        ops.dev_ptr(f["start_fitness"], F64, "s"), ops.dev_ptr(i["best_pos"], I32, "p"), ops.dev_ptr(f["best_rows"], F64, "r"),
        ops.dev_ptr(f["history"], F64, "h"), ops.dev_ptr(i["sweeps"], I32, "sw"), ops.dev_ptr(i["moves"], I32, "m"),
        ops.dev_ptr(f["walk"], F64, "w"), ops.dev_ptr(i["steps"], I32, "st"), ops.dev_ptr(i["best_step"], I32, "bs"),
        ops.dev_ptr(i["stalled"], I32, "sd"), ops.dev_ptr(i["pair_steps"], I32, "ps"), ops.stream_ptr()),
        "gnnpn_descend_tabu_pairs_ragged_f64")
    return {k: v.cpu().tolist() for k, v in {**f, **i}.items()}


@pytest.mark.parametrize("wide", [0, 1])
def test_tabu_pairs_ragged_batch_with_a_start_outside_its_list(dev, wide):
    """Two SEEDS tables around the wall problem with a start outside its second list: it is not searched (NaN / -1 fields, the
    sentinel left in its rows) while its neighbours are; with no steps the one history entry holds phase 0's merit and walk NaN."""
    seeds = sref._seeds_tables()
    tables = (seeds[16], tref.outside_start(), pref.wall_problem(), seeds[19])
    max_cand = max(sum(len(c) for c in t[0]) for t in tables)
    for max_steps in (8, 0):
        got = _call(dev, tables, 9, max_cand, 16, max_steps, 2, 0, 2, wide)
        ld = max(max_steps, 1)
        for p in (0, 2, 3):
            w = tpref.descend_tabu_pairs(*tables[p], max_steps=max_steps, tenure=2, max_rank=2)
            T = len(tables[p][0])
            for k in tpref.FIELDS:
                assert got[k][p] == w[k], (p, k)
            assert got["best_pos"][p][:T] == w["best_pos"] and [tuple(r) for r in got["best_rows"][p][:T]] == w["best_rows"], p
            assert got["history"][p] == w["history"] and got["walk"][p][:w["steps"]] == w["walk"], p
            assert all(math.isnan(v) for v in got["walk"][p][w["steps"]:]) and len(got["walk"][p]) == ld, p
            assert got["best_pos"][p][T:] == [-7] * (9 - T), p
        assert math.isnan(got["best_fitness"][1]) and math.isnan(got["start_fitness"][1])
        assert all(math.isnan(v) for v in got["history"][1] + got["walk"][1]) and len(got["history"][1]) == ld
        assert (got["sweeps"][1], got["moves"][1], got["steps"][1], got["best_step"][1], got["stalled"][1], got["pair_steps"][1]) == \
            (-1, 0, -1, 0, 0, 0)
        assert set(got["best_pos"][1]) == {-7} and set(np.asarray(got["best_rows"][1]).ravel()) == {-7.0}
    assert tpref.descend_tabu_pairs(*tables[2], max_steps=8, tenure=2, max_rank=2)["pair_steps"] == 1


def test_tabu_pairs_launch_sized_too_small(dev):
    """More candidates than max_cand sizes the tabu table and the merit buffer for: not searched, in the workgroup form too."""
    seeds = sref._seeds_tables()
    tables = (pref.wall_problem(), seeds[19])
    for wide in (0, 1):
        got = _call(dev, tables, 9, 4, 16, 4, 2, 0, 2, wide)
        assert got["steps"] == [1, -1] and got["pair_steps"] == [1, 0] and math.isnan(got["best_fitness"][1]) and got["best_pos"][0][:2] == [1, 1]


# ---- 3. nothing to launch, too much to launch --------------------------------------------------------------------------------------------------

def test_tabu_pairs_empty_batch(dev):
    from gnnpn_sc_amd import ops
    e = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=dev)      # noqa: E731
    res = ops.descend_tabu_pairs_ragged(e(1), e(1), e(0, 4, dt=torch.float64), e(0, 4, dt=torch.float64), e(0), max_steps=5, tenure=2, max_rank=2)
    assert res["best_fitness"].shape == (0,) and res["walk"].shape == (0, 5) and res["history"].shape == (0, 5) and res["steps"].shape == (0,)
    assert res["pair_steps"].shape == (0,)


def test_tabu_pairs_lds_beyond_a_cu_raises_and_launches_nothing(dev):
    from gnnpn_sc_amd import ops
    operands = _operands(dev, [pref.wall_problem()])
    kw = dict(max_steps=4, tenure=2, max_rank=2)
    with pytest.raises(ops.GnnpnError, match=r"descend_tabu_pairs_ragged: \d+ B of LDS per problem \(2 slots, 6000 candidates, shortlists of 2\) "
                                             r"exceed a CU.*wide=1"):
        ops.descend_tabu_pairs_ragged(*operands, max_slots=2, max_cand=6000, **kw)
    with pytest.raises(ops.GnnpnError, match=r"descend_tabu_pairs_ragged: \d+ B of LDS per problem \(5000 slots, 50 candidates, shortlists of 2\) "
                                             r"exceed a CU"):
        ops.descend_tabu_pairs_ragged(*operands, max_slots=5000, max_cand=50, **kw)
    with pytest.raises(ops.GnnpnError, match=r"\(2 slots, 50000 candidates, shortlists of 2\) exceed a CU"):
        ops.descend_tabu_pairs_ragged(*operands, max_slots=2, max_cand=50000, wide=True, **kw)
    torch.cuda.synchronize(dev)


# ---- 4. through the layers -----------------------------------------------------------------------------------------------------------------------

def test_pipeline_descend_tabu_pairs_after_run(dev, chain):      # noqa: F811
    from gnnpn_sc_amd.pipeline import descend_tabu_pairs
    pipe, host, mins = chain["pipe"], chain["host"], chain["mins"]
    assert not any(isinstance(h, Exception) for h in host)
    tables = [(cats, bounds, start) for cats, _l, start, bounds in host]
    for steps, tenure, rank, span in ((8, 2, 2, 0), (3, 0, 0, 1)):
        res = pipe.descend_tabu_pairs(chain["svc"], chain["batch"], chain["out"], max_steps=steps, tenure=tenure, max_rank=rank, max_span=span,
                                      min_cost=mins[N_TRAIN:])
        got = {k: v.cpu().tolist() for k, v in res.items()}
        want = [tpref.descend_tabu_pairs(*t, max_steps=steps, tenure=tenure, max_rank=rank, max_span=span) for t in tables]
        _assert_all(got, tables, want, steps)
        assert got["n_slots"] == [len(cats) for cats, _b, _s in tables]
        assert got["quality"] == [mins[N_TRAIN + b] / w["best_fitness"] for b, w in enumerate(want)]
        again = descend_tabu_pairs(chain["svc"], chain["batch"], chain["out"], max_sweeps=16, max_steps=steps, tenure=tenure, max_rank=rank,
                                   max_span=span, min_cost=mins[N_TRAIN:])
        assert _same(again, res)
    zero = pipe.descend_tabu_pairs(chain["svc"], chain["batch"], chain["out"], max_steps=0, tenure=2, max_rank=2, min_cost=mins[N_TRAIN:])
    one = pipe.descend(chain["svc"], chain["batch"], chain["out"], min_cost=mins[N_TRAIN:])
    assert set(one) - set(zero) == set() and all(torch.equal(zero[k], one[k]) for k in one if k != "history")


def test_pipeline_descend_starts_tabu_pairs(dev, chain, monkeypatch):      # noqa: F811
    from test_gpu_refine import _host_tables
    pipe, svc, batch, mins = chain["pipe"], chain["svc"], chain["batch"], chain["mins"]
    monkeypatch.chdir(chain["tmp"])
    B, R, steps, tenure, rank = P_ - N_TRAIN, 3, 6, 2, 2
    seen = _replicas(chain["ds"], chain["out"]["actions"].double().cpu().numpy(), R)
    starts = torch.from_numpy(seen).to(dev)
    host = [_host_tables("QWS", seen[:, r], 0)[0] for r in range(R)]
    assert not any(isinstance(h, Exception) for hr in host for h in hr)
    res = pipe.descend_starts_tabu_pairs(svc, batch, starts, max_steps=steps, tenure=tenure, max_rank=rank, min_cost=mins[N_TRAIN:])
    got = {k: v.cpu().tolist() for k, v in res.items()}
    assert res["pair_steps_all"].shape == (B, R)
    for b in range(B):
        runs = [tpref.descend_tabu_pairs(host[r][b][0], host[r][b][3], host[r][b][2], max_steps=steps, tenure=tenure, max_rank=rank)
                for r in range(R)]
        w = mref.select(runs)
        assert got["start_index"][b] == w and got["n_slots"][b] == len(host[w][b][0]), b
        _assert_problem(got, b, host[w][b][0], runs[w], steps)
        for k, field in (("fitness_all", "best_fitness"), ("start_fitness_all", "start_fitness"), ("sweeps_all", "sweeps"),
                         ("moves_all", "moves"), ("steps_all", "steps"), ("best_step_all", "best_step"), ("pair_steps_all", "pair_steps")):
            assert got[k][b] == [r[field] for r in runs], (b, k)
        assert got["quality"][b] == mins[N_TRAIN + b] / runs[w]["best_fitness"], b


def test_main_cli_infer_descend_tabu_pair_moves(dev, chain, monkeypatch):      # noqa: F811
    from test_gpu_refine import _actions_array, _host_tables
    tmp = chain["tmp"]
    monkeypatch.chdir(tmp)
    _write_cli_ini(tmp)
    import main as cli
    base = ["main.py", "QWS", "ML+2PN", "-1", "--infer", "--random-init", "--descend=4", "--tabu=8", "--tenure=2", "--pair-moves=2", "--pair-span=1"]
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(base) == 0
    with open("./solutions/WOA/QWS/ML+2PN+tabu+pairs.txt") as f:
        doc = json.load(f)
    with open("./solutions/pretrained/QWS-PNHigh.txt") as f:
        actions = _actions_array(json.load(f))
    host, _sols, mins = _host_tables("QWS", actions, 0)
    assert not any(isinstance(h, Exception) for h in host)
    want = [tpref.descend_tabu_pairs(cats, bounds, start, max_sweeps=4, max_steps=8, tenure=2, max_rank=2, max_span=1)
            for cats, _l, start, bounds in host]
    settings = {"tabu_steps": 8, "tenure": 2, "top": 2, "span": 1}
    assert list(doc) == ["quality", "time", "averageQ", "averageT", "steps", "best_step", "pair_steps", "stalled", *settings]
    assert {k: doc[k] for k in settings} == settings and len(doc["quality"]) == P_ - N_TRAIN
    assert doc["quality"] == [mins[N_TRAIN + b] / w["best_fitness"] for b, w in enumerate(want)]
    for k in ("steps", "best_step", "pair_steps", "stalled"):
        assert doc[k] == [w[k] for w in want], k
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(base + ["--samples=3", "--all-starts", "--seed", "5"]) == 0
    with open("./solutions/WOA/QWS/ML+2PN+multistart+tabu+pairs.txt") as f:
        multi = json.load(f)
    assert list(multi) == list(doc) and {k: multi[k] for k in settings} == settings and len(multi["pair_steps"]) == P_ - N_TRAIN
