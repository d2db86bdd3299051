"""-m gpu: the one-swap descent on the device — gnnpn_descend_ragged_f64 in its lane form (one candidate per lane) and its workgroup
form, ops.descend_ragged, pipeline.descend / refine(descend=k) and `main.py ... --infer --descend` — against the plain-Python
restatement of the search over oracle.woa.objective (tests/descent_reference.py): every float64 and every position, ``==``."""
import contextlib
import functools
import io
import json

import numpy as np
import pytest
import torch

import descent_reference as ref

pytestmark = pytest.mark.gpu


# ---- helpers: problems, their reference runs (computed once, shared), one launch -----------------------------------------------

@functools.lru_cache(maxsize=None)
def _tables(seed, sizes, per_size, max_cand=8, permute=False):
    from test_gpu_woa import _random_problems
    g = np.random.default_rng(seed)
    problems = []
    for T in sizes:
        problems += _random_problems(g, T, per_size, max_cand)
    if permute:
        problems = [problems[i] for i in g.permutation(len(problems))]
    return tuple(ref.prepare(problems))


@functools.lru_cache(maxsize=None)
def _want(seed, sizes, per_size, max_cand=8, permute=False, max_sweeps=16):
    return tuple(ref.descend(*tab, max_sweeps=max_sweeps) for tab in _tables(seed, sizes, per_size, max_cand, permute))


def _launch(dev, tables, max_sweeps=16, wide=None, **kw):
    from gnnpn_sc_amd import ops
    prob_ptr, cand_ptr, flat, bounds, start = ref.pack(tables)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev)      # noqa: E731
    res = ops.descend_ragged(t(prob_ptr, torch.int32), t(cand_ptr, torch.int32), t(flat, torch.float64).reshape(-1, 4),
                             t(bounds, torch.float64), t(start, torch.int32), max_sweeps=max_sweeps, wide=wide, **kw)
    return {k: v.cpu().tolist() for k, v in res.items()}


def _assert_equal(got, tables, want):
    for p, ((cats, _b, _s), w) in enumerate(zip(tables, want)):
        T = len(cats)
        for k in ("best_fitness", "start_fitness", "history", "sweeps", "moves"):
            assert got[k][p] == w[k], (p, T, k, got[k][p], w[k])
        assert got["best_pos"][p][:T] == w["best_pos"], (p, T)
        assert [tuple(r) for r in got["best_rows"][p][:T]] == w["best_rows"], (p, T)


# ---- 1. lane form, and the same problems through the workgroup form ------------------------------------------------------------

@pytest.mark.parametrize("wide", [None, True])
@pytest.mark.parametrize("T", [1, 2, 7, 8, 9, 33, 63, 64])
def test_descend_lane_sizes(dev, T, wide):
    """7 / 8 / 9 straddle numpy's switch to eight accumulators, 64 fills the wave."""
    key = (200 + T, (T,), 3)
    _assert_equal(_launch(dev, _tables(*key), wide=wide), _tables(*key), _want(*key))


@pytest.mark.parametrize("wide", [None, True])
@pytest.mark.parametrize("T", [3, 9])
def test_descend_lists_longer_than_a_wave(dev, T, wide):
    """Lists of up to 139 candidates: up to three chunks of 64 per slot; four problems, so one has no start."""
    key = (300 + T, (T,), 4, 140)
    tables = _tables(*key)
    assert max(len(c) for cats, _b, _s in tables for c in cats) > 128
    _assert_equal(_launch(dev, tables, wide=wide), tables, _want(*key))


def test_the_lane_cases_cover_every_kind_of_start():
    from test_gpu_woa import _random_problems
    kinds = set()
    for seed, T, n, mc in [(200 + T, T, 3, 8) for T in (1, 2, 7, 8, 9, 33, 63, 64)] + [(300 + T, T, 4, 140) for T in (3, 9)]:
        problems = _random_problems(np.random.default_rng(seed), T, n, mc)
        for (services, _c, sol), (cats, _b, start) in zip(problems, _tables(seed, (T,), n, mc)):
            foreign = start is not None and any(len(c) > len(s) for c, s in zip(cats, services))
            kinds.add("none" if start is None else "foreign" if foreign else "member")
    assert kinds == {"none", "foreign", "member"}


# ---- 2. workgroup form ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,n,sweeps", [(65, 2, 16), (127, 2, 16), (128, 2, 16), (129, 2, 16), (300, 2, 16), (1000, 1, 2)])
def test_descend_workgroup_sizes(dev, T, n, sweeps):
    """Above 128 terms np.sum recurses: 129, 300 and 1000 cut column 0 differently."""
    key = (400 + T, (T,), n, 8, False, sweeps)
    tables = _tables(*key[:5])
    _assert_equal(_launch(dev, tables, max_sweeps=sweeps), tables, _want(*key))


# ---- 3. ragged batches ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", [(1, 3, 10, 33, 64, 7), (5, 64, 65, 100, 2, 130)])
def test_descend_ragged_batch(dev, sizes):
    key = (sum(sizes), sizes, 3, 8, True)
    tables = _tables(*key)
    _assert_equal(_launch(dev, tables), tables, _want(*key))


# ---- 4. ties and strictness, on hand-built tables --------------------------------------------------------------------------------

GOOD, POOR = (0.1, 0.9, 0.99, 0.99), (0.8, 0.2, 0.99, 0.99)
BOUNDS = [0.5, 1.0, 0.5, 1.0]


@pytest.mark.parametrize("wide", [None, True])
def test_descend_ties_and_strictness(dev, wide):
    tables = [([[POOR, GOOD, POOR, GOOD], [POOR]], BOUNDS, [0, 0]),      # the best row twice: the lower position
              ([[GOOD, GOOD], [POOR]], BOUNDS, [1, 0]),                  # the only alternative has exactly the current merit
              ([[POOR] + [GOOD] * 70 + [POOR], [POOR]], BOUNDS, [71, 0])]   # equal best rows in two chunks of the lane form
    want = [ref.descend(*tab) for tab in tables]
    assert want[0]["best_pos"] == [1, 0] and want[2]["best_pos"] == [1, 0]
    got = _launch(dev, tables, wide=wide)
    _assert_equal(got, tables, want)
    assert got["best_pos"][0] == [1, 0] and got["moves"][0] == 1
    assert got["best_pos"][1] == [1, 0] and got["moves"][1] == 0 and got["sweeps"][1] == 1


# ---- 5. cut-off --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wide", [None, True])
def test_descend_cut_off(dev, wide):
    key = (5, (7,), 4)
    full = _want(*key)
    p = next(i for i, r in enumerate(full) if r["sweeps"] >= 3)
    tab = _tables(*key)[p]
    one = _launch(dev, [tab], max_sweeps=1, wide=wide)
    _assert_equal(one, [tab], [ref.descend(*tab, max_sweeps=1)])
    assert one["history"][0] == [full[p]["history"][0]] and one["sweeps"] == [1]
    zero = _launch(dev, [tab], max_sweeps=0, wide=wide)
    _assert_equal(zero, [tab], [ref.descend(*tab, max_sweeps=0)])
    assert zero["sweeps"] == [0] and zero["moves"] == [0] and zero["history"] == [[]]
    assert zero["best_fitness"] == zero["start_fitness"] == [full[p]["start_fitness"]] and zero["best_pos"][0] == (list(tab[2]) if tab[2] is not None else [0] * 7)
    whole = _launch(dev, [tab], wide=wide)
    n = whole["sweeps"][0]
    assert 3 <= n < 16 and whole["history"][0][n - 1:] == [whole["best_fitness"][0]] * (17 - n)      # the tail repeats the final value


@pytest.mark.parametrize("wide", [0, 1])
def test_descend_writes_every_history_entry(dev, wide):
    """The C entry itself, over a history buffer filled with a sentinel: with max_sweeps = 0 the one entry per problem that the ABI
    asks for holds the start's merit, and a problem that is not searched gets NaN; nothing of the buffer keeps the sentinel."""
    from gnnpn_sc_amd import _lib, ops
    small, big = _tables(207, (7,), 3)[1], _tables(233, (33,), 3)[1]
    prob_ptr, cand_ptr, flat, bounds, start = ref.pack([small, big])
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev)      # noqa: E731
    ops_in = [t(prob_ptr, torch.int32), t(cand_ptr, torch.int32), t(flat, torch.float64).reshape(-1, 4), t(bounds, torch.float64),
              t(start, torch.int32)]
    F64, I32 = torch.float64, torch.int32
    for max_sweeps, ld in ((0, 1), (3, 3)):
        fit, start_fit = torch.empty(2, dtype=F64, device=dev), torch.empty(2, dtype=F64, device=dev)
        pos, rows = torch.zeros(2, 7, dtype=I32, device=dev), torch.zeros(2, 7, 4, dtype=F64, device=dev)
        hist = torch.full((2, ld), -7.0, dtype=F64, device=dev)
        sweeps, moves = torch.empty(2, dtype=I32, device=dev), torch.empty(2, dtype=I32, device=dev)
        ops.check(_lib.load().gnnpn_descend_ragged_f64(
            2, ops.dev_ptr(ops_in[0], I32, "prob_ptr"), len(start), 7, sum(len(c) for c in small[0]), ops.dev_ptr(ops_in[1], I32, "cand_ptr"),
            ops.dev_ptr(ops_in[2], F64, "cand"), ops.dev_ptr(ops_in[3], F64, "bounds"), ops.dev_ptr(ops_in[4], I32, "start_pos"),
            max_sweeps, wide, ops.dev_ptr(fit, F64, "f"), ops.dev_ptr(start_fit, F64, "s"), ops.dev_ptr(pos, I32, "p"),
            ops.dev_ptr(rows, F64, "r"), ops.dev_ptr(hist, F64, "h"), ops.dev_ptr(sweeps, I32, "sw"), ops.dev_ptr(moves, I32, "m"),
            ops.stream_ptr()), "gnnpn_descend_ragged_f64")
        want = ref.descend(*small, max_sweeps=max_sweeps)
        h = hist.cpu().tolist()
        assert h[0] == (want["history"] if max_sweeps else [want["start_fitness"]]), (max_sweeps, h)
        assert all(np.isnan(v) for v in h[1]) and sweeps.cpu().tolist() == [want["sweeps"], -1], (max_sweeps, h)


# ---- 6. a problem the launch was not sized for ------------------------------------------------------------------------------------

def test_descend_unsupported_and_unfit(dev):
    from gnnpn_sc_amd import ops
    g = np.random.default_rng(12)
    row = lambda: tuple(float(v) for v in np.r_[g.random(2), 1.0 - g.random(2) * 0.05])      # noqa: E731
    big = ([[row() for _ in range(1750)] for _ in range(3)], BOUNDS, [5, 1700, 0])         # 5250 rows x 32 B: beyond a CU's LDS
    with pytest.raises(ops.GnnpnError, match="wide"):
        _launch(dev, [big])
    want = ref.descend(*big)
    assert want["moves"] > 0
    _assert_equal(_launch(dev, [big], wide=True), [big], [want])
    # sized too small: more slots / more candidates than the launch was told, and a start outside its list
    small, wide_one = _tables(207, (7,), 3)[1], _tables(233, (33,), 3)[1]
    outside = (small[0], small[1], [len(small[0][0])] + list(small[2][1:]))
    tables = [small, wide_one, outside]
    for kw in ({"max_slots": 7}, {"max_slots": 7, "wide": True}):
        got = _launch(dev, tables, max_cand=sum(len(c) for c in wide_one[0]), **kw)
        _assert_equal(got, tables[:1], [ref.descend(*small)])
        for p in (1, 2):
            assert np.isnan(got["best_fitness"][p]) and np.isnan(got["start_fitness"][p]) and got["sweeps"][p] == -1, (kw, p)
            assert got["moves"][p] == 0 and len(got["history"][p]) == 16 and all(np.isnan(h) for h in got["history"][p]), (kw, p)
            assert not any(got["best_pos"][p]) and not np.asarray(got["best_rows"][p]).any(), (kw, p)      # the wrapper's zeros
    got = _launch(dev, [small, wide_one], max_cand=sum(len(c) for c in small[0]))
    assert got["sweeps"][0] >= 1 and got["sweeps"][1] == -1 and np.isnan(got["best_fitness"][1])


# ---- 7. the pipeline: descend after run, refine(descend=k), the CLI -----------------------------------------------------------------

T_, S_, K_, H_, P_ = 6, 60, 3, 256, 96
N_TRAIN = P_ // 4 * 3


@pytest.fixture(scope="module")
def chain(dev, tmp_path_factory):
    """The synthetic data set of test_refine_after_run_equals_fine_tune, one run of the two-level pass over its test quarter and
    the host path's tables for the actions of that run."""
    import os
    import gnnpn_sc_amd.synth as synth
    from gnnpn_sc_amd.modelML import Net
    from gnnpn_sc_amd.modelPN import CombinatorialRL, reward
    from gnnpn_sc_amd.pipeline import ML2PNPipeline
    from oracle import ml as oml, pn as opn
    from test_gpu_refine import _device_batch, _host_tables
    tmp = tmp_path_factory.mktemp("descend_chain")
    ds = synth.make_dataset(T_, S_, P_, seed=21, tasks_per_problem=3, lo_range=(0.85, 0.96))
    synth.write_dataset(str(tmp), "QWS", ds)
    svc, batch = _device_batch(ds, N_TRAIN, dev)
    net = Net(128, S_, 20, 2, 2)
    net.load_state_dict(oml.make_state_dict(128, 20, 2, 2, seed=7))
    low = CombinatorialRL(0, H_, T_ * K_, 0, 10, 1, reward, "Dot", K_, T_, level="Low")
    high = CombinatorialRL(0, H_, T_ * K_, 0, 10, 1, reward, "Dot", K_, T_, level="High")
    low.load_state_dict(opn.make_state_dict(H_, 8))
    high.load_state_dict(opn.make_state_dict(H_, 9))
    pipe = ML2PNPipeline(net.to(dev).eval(), low.to(dev).eval(), high.to(dev).eval(), K_)
    out = pipe.run(svc, batch)
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        host, _sols, mins = _host_tables("QWS", out["actions"].double().cpu().numpy(), 0)
    finally:
        os.chdir(cwd)
    return {"tmp": tmp, "ds": ds, "svc": svc, "batch": batch, "pipe": pipe, "out": out, "host": host, "mins": mins}


def _host_want(host, max_sweeps):
    return [ref.descend(cats, bounds, start, max_sweeps=max_sweeps) for cats, _len0, start, bounds in host]


def test_pipeline_descend_after_run(dev, chain):
    from gnnpn_sc_amd import WOA
    pipe, host, mins = chain["pipe"], chain["host"], chain["mins"]
    if any(isinstance(h, Exception) for h in host):
        with pytest.raises(WOA.GnnpnError, match="problem"):
            pipe.descend(chain["svc"], chain["batch"], chain["out"])
        return
    res = pipe.descend(chain["svc"], chain["batch"], chain["out"], min_cost=mins[N_TRAIN:])
    got = {k: v.cpu().tolist() for k, v in res.items()}
    tables = [(cats, bounds, start) for cats, _l, start, bounds in host]
    want = _host_want(host, 16)
    _assert_equal(got, tables, want)
    assert got["n_slots"] == [len(cats) for cats, _b, _s in tables]
    assert got["quality"] == [mins[N_TRAIN + b] / w["best_fitness"] for b, w in enumerate(want)]


def test_refine_from_the_descended_composition(dev, chain):
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.pipeline import refine
    svc, batch, out, host = chain["svc"], chain["batch"], chain["out"], chain["host"]
    assert not any(isinstance(h, Exception) for h in host)
    B = P_ - N_TRAIN
    seeds = torch.tensor([77 + i for i in range(B)], dtype=torch.int64, device=dev)
    res = refine(svc, batch, out, 10, 12, seeds=seeds, descend=4)
    tabs = ops.woa_candidates(svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds, out["actions"])
    want4 = _host_want(host, 4)
    tables = [(cats, bounds, start) for cats, _l, start, bounds in host]
    _assert_equal({k: v.cpu().tolist() for k, v in res["descent"].items()}, tables, want4)
    start_pos = torch.tensor([x for w in want4 for x in w["best_pos"]], dtype=torch.int32, device=dev)
    fit, _pos, hist, draws, rows = ops.eswoa_ragged(tabs["prob_ptr"], tabs["cand_ptr"], tabs["len_init"], tabs["cand"], tabs["bounds"],
                                                    start_pos, 10, 12, seeds, max_slots=tabs["max_slots"], max_cand=tabs["max_cand"])
    assert res["best_fitness"].cpu().tolist() == fit.cpu().tolist()
    assert res["history"].cpu().tolist() == hist.cpu().tolist()
    assert res["draws"].cpu().tolist() == draws.cpu().tolist()
    assert res["best_rows"].cpu().tolist() == rows.cpu().tolist()
    refined, descended = res["best_fitness"].cpu().tolist(), res["descent"]["best_fitness"].cpu().tolist()
    started = res["descent"]["start_fitness"].cpu().tolist()
    assert all(r <= d <= s for r, d, s in zip(refined, descended, started))
    plain = refine(svc, batch, out, 10, 12, seeds=seeds)                          # descend=0: today's result, no descent entry
    assert "descent" not in plain


def test_main_cli_infer_descend(dev, chain, monkeypatch):
    from test_gpu_refine import _actions_array, _host_tables
    tmp = chain["tmp"]
    monkeypatch.chdir(tmp)
    (tmp / "environment.ini").write_text(
        f"[QWS-PNHigh]\nembeddingTag = 0\nUSE_CUDA = 1\nserCategory = {T_}\nepochDiv = 1\nserNumber = {K_}\nhidden_size = {H_}\n"
        "n_glimpses = 0\ntanh_exploration = 10\nuse_tanh = 1\nbeta = 0.9\nmax_grad_norm = 2.\nlr = 0.5e-4\nepochML = -1\nepochPNLow = -1\n"
        f"[QWS-ML+2PN]\nserviceCategory = {T_}\nepoch = -1\n")
    import main as cli
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["main.py", "QWS", "ML+2PN", "-1", "--infer", "--random-init", "--descend=4"]) == 0
    with open("./solutions/WOA/QWS/ML+2PN+descent.txt") as f:
        written = json.load(f)
    with open("./solutions/pretrained/QWS-PNHigh.txt") as f:
        actions = _actions_array(json.load(f))
    host, _sols, mins = _host_tables("QWS", actions, 0)
    assert not any(isinstance(h, Exception) for h in host)
    want = _host_want(host, 4)
    assert written["quality"] == [mins[N_TRAIN + b] / w["best_fitness"] for b, w in enumerate(want)]
    assert len(written["quality"]) == P_ - N_TRAIN and written["averageQ"] == sum(written["quality"]) / len(written["quality"])
    # with --woa beside it ES-WOA starts from the descended composition; each file books the time of its own stages
    with open("environment.ini", "a") as f:
        f.write(f"[QWS-WOA]\nserCategory = {T_}\nMLESWOAtest = 0\nML2PNWOATest = 1\nMLWOATest = 0\nESWOAtest = 0\n"
                "serviceNumber = 4\nreduct = 0\nepoch = -1\nMAX_Iter = 5\npopSize = 6\n")
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["main.py", "QWS", "ML+2PN", "-1", "--infer", "--random-init", "--descend=4", "--woa", "--seed", "3"]) == 0
    with open("./solutions/WOA/QWS/ML+2PN+descent.txt") as f:
        again = json.load(f)
    with open("./solutions/WOA/QWS/ML+2PN+WOA.txt") as f:
        refined = json.load(f)
    with open("./solutions/pretrained/QWS-PNHigh.txt") as f:
        assert (_actions_array(json.load(f)) == actions).all()                       # the same start (random-init is seeded)
    assert again["quality"] == written["quality"]
    # refined <= descended per problem, so min_cost / fitness does not fall (fitness > 0 here)
    assert all(r >= d > 0 for r, d in zip(refined["quality"], again["quality"]))
    assert len(set(again["time"])) == len(set(refined["time"])) == 1 and again["time"][0] > 0 and refined["time"][0] > 0
