"""-m gpu: the third stage on the device — ES-WOA inputs built by gnnpn_woa_candidates_count / _fill, the ragged search of
gnnpn_eswoa_ragged_f64 and ML2PNPipeline.refine — against the host path it replaces (loadDataOther + WOA._prepare +
WOA.fine_tune), which tests/golden/woa_driver.json pins to the reference's own output."""
import contextlib
import io
import json
import math
import os
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


# ---- 1. rounding -----------------------------------------------------------------------------------------------------------

def test_round5_equals_python_round(dev):
    from gnnpn_sc_amd import ops
    import gnnpn_sc_amd.synth as synth
    g = np.random.default_rng(11)
    parts = [g.random(300000),                                                          # uniform in [0, 1]
             g.random(200000).astype(np.float32).astype(np.float64),                   # f32 widened (the actions)
             -g.random(100000) * 10.0 ** g.integers(-6, 6, 100000)]                     # negatives over many scales
    k = g.integers(0, 10 ** 7, 60000)
    ties = (k + 0.5) / 1e5                                                              # constructed near-ties
    near = [ties]
    for d in range(1, 5):
        up, dn = ties.copy(), ties.copy()
        for _ in range(d):
            up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
        near += [up, dn]
    parts += near + [-np.concatenate(near)]
    for T, S, seed in ((47, 2507, 1), (50, 5000, 2), (5, 30, 17)):                     # QoS values of the test data sets
        parts.append(synth.make_service_table(T, S, seed=seed, degree=1).qos.ravel())
    big = 2.0 ** 52 / 1e5
    parts += [big * (0.5 + 2 * g.random(20000)), -big * (0.5 + 2 * g.random(20000)),  # around and beyond the range limit
              10.0 ** g.uniform(11, 300, 5000),
              np.array([0.0, -0.0, 5e-324, -5e-324, 1e-300, np.inf, -np.inf, 2.5e-5, -2.5e-5, 1.5e-5, 0.000125, 1e308])]
    x = np.concatenate(parts)
    assert x.size >= 10 ** 6
    got = ops.debug_round5(torch.from_numpy(x).to(dev)).cpu().numpy()
    want = np.array([round(float(v), 5) for v in x])
    diff = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert diff.size == 0, [(repr(x[i]), repr(got[i]), repr(want[i])) for i in diff[:5]]
    assert math.isnan(ops.debug_round5(torch.tensor([math.nan], dtype=torch.float64, device=dev)).item())


# ---- helpers: the host path and the device tables of one data set ------------------------------------------------------------

def _host_tables(name, actions, reduct, patches=()):
    """WOA.start's preparation (rows, pick sets, loadDataOther, _prepare) per test problem: a tuple (cats, len0, start,
    bounds) or the exception the host path raises for it."""
    from gnnpn_sc_amd import WOA
    from gnnpn_sc_amd.loadData import loadDataOther
    n, T = actions.shape[0], actions.shape[1]
    sols, ssets = [], []
    for b in range(n):
        rows = [actions[b, c, :4].tolist() for c in range(T)]
        rows = [r for r in rows if sum(r) != 3]
        sols.append(rows)
        ssets.append({tuple(round(v, 5) for v in r) for r in rows})
    feats, cons, mins = loadDataOther(name, reduct, sSetList=ssets, train=False)
    out = []
    for b in range(n):
        try:
            cats, len0, start, _rows, bounds = WOA._prepare(feats[b], cons[b], sols[b] if sols[b] else None, patches)
            if not cats:
                raise WOA.GnnpnError("no categories")
            out.append((cats, len0, start, bounds))
        except WOA.GnnpnError as e:
            out.append(e)
    return out, sols, mins


def _device_batch(ds, first, dev):
    from gnnpn_sc_amd.loadData import tables_from_dataset
    from gnnpn_sc_amd.pipeline import DeviceBatch, DeviceServices
    table, pb = tables_from_dataset(ds, first, None)
    return DeviceServices.from_table(table, dev), DeviceBatch.from_problems(pb, dev)


def _assert_tables_equal(tabs, host):
    status = tabs["status"].cpu().tolist()
    prob_ptr, cand_ptr = tabs["prob_ptr"].cpu().tolist(), tabs["cand_ptr"].cpu().tolist()
    len_init, start_pos = tabs["len_init"].cpu().tolist(), tabs["start_pos"].cpu().tolist()
    cand = tabs["cand"].cpu().numpy().view(np.uint64)
    bounds, n_slots = tabs["bounds"].cpu().numpy(), tabs["n_slots"].cpu().tolist()
    for b, h in enumerate(host):
        if isinstance(h, Exception):
            assert status[b] in (1, 3), (b, status[b], h)
            assert prob_ptr[b + 1] == prob_ptr[b] and n_slots[b] == 0
            continue
        cats, len0, start, hb = h
        assert status[b] == 0, b
        assert prob_ptr[b + 1] - prob_ptr[b] == len(cats) == n_slots[b], b
        assert bounds[b].tolist() == hb, b
        for j, cat in enumerate(cats):
            s = prob_ptr[b] + j
            assert len_init[s] == len0[j], (b, j)
            assert start_pos[s] == (start[j] if start is not None else -1), (b, j)
            rows = cand[cand_ptr[s]:cand_ptr[s + 1]]
            assert rows.shape[0] == len(cat), (b, j)
            assert rows.ravel().tolist() == [_bits(v) for t in cat for v in t], (b, j)


def _actions_array(actions_T_nTest_8):
    return np.asarray(actions_T_nTest_8, dtype=np.float64).transpose(1, 0, 2).copy()


def _woa_driver(tmp_path, monkeypatch):
    from test_host_logic import _woa_driver_setup
    import gnnpn_sc_amd.synth as synth
    monkeypatch.chdir(tmp_path)
    fx, actions, n_train = _woa_driver_setup(str(tmp_path))
    p = fx["params"]
    ds = synth.make_dataset(p["T"], p["S"], p["P"], seed=p["seed"], tasks_per_problem=p["tasks_per_problem"],
                            lo_range=tuple(p["lo_range"]))
    return fx, ds, _actions_array(actions), n_train


# ---- 2. candidate tables against the host --------------------------------------------------------------------------------

@pytest.mark.parametrize("reduct", [0, 0.55])
def test_candidates_equal_host_on_the_driver_fixture(dev, tmp_path, monkeypatch, reduct):
    from gnnpn_sc_amd import ops
    fx, ds, actions, n_train = _woa_driver(tmp_path, monkeypatch)
    host, _sols, _mins = _host_tables("QWS", actions, reduct)
    svc, batch = _device_batch(ds, n_train, dev)
    for dt in (torch.float64,) if reduct else (torch.float64, torch.float32):
        a = torch.from_numpy(actions).to(dev, dt)
        if dt == torch.float32:               # f32 actions: what run() returns; the host sees them widened
            host, _s, _m = _host_tables("QWS", a.double().cpu().numpy(), reduct)
        tabs = ops.woa_candidates(svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds, a,
                                  reduct=reduct, check_status=False)
        _assert_tables_equal(tabs, host)


def _qws_like(tmp_path, n_problems=1100, seed=1, n_cat=47, n_services=2507, tasks=10):
    import gnnpn_sc_amd.synth as synth
    ds = synth.make_dataset(n_cat, n_services, n_problems, seed=seed, tasks_per_problem=tasks)
    synth.write_dataset(str(tmp_path), "QWS", ds)
    return ds


def _slot_lists(ds, reduct):
    """addS's list of every task slot of the test problems, empty ones included (loadDataOther without the drop)."""
    from gnnpn_sc_amd.loadData import addS
    sf = ds["serviceFeature"]
    n_cat = len(sf)
    div, mod = [], []
    for key in sf:
        div += [int(key) - 1] * len(sf[key])
        mod += list(range(len(sf[key])))
    P = len(ds["nodefeatures"])
    out = []
    for nodes in ds["nodefeatures"][P // 4 * 3:]:
        cons = {c: [0] * 8 for c in range(1, n_cat + 1)}
        for node in nodes:
            pair = node[-5:-3] + node[-2:]
            if node[0] == 1:
                for c in cons:
                    cons[c][-4:] = pair
            else:
                cons[node[:-6].index(1)][-8:-4] = pair
        out.append(addS(range(len(div)), sf, cons, [n[:-6].index(1) - 1 for n in nodes][1:], div, mod, reduct, None))
    return out


def _picks(ds, reduct, g, foreign=0.1):
    """Action rows [nTest, T, 8]: per task a member of its candidate list at ``reduct`` (without picks: for reduct != 0 the
    front itself), some foreign rows, dummy rows (0,1,1,1) for absent categories and for tasks whose list is empty."""
    P = len(ds["nodefeatures"])
    n_train = P // 4 * 3
    T = len(ds["serviceFeature"])
    acts = np.zeros((P - n_train, T, 8))
    acts[:, :, 1:4] = 1.0
    for b, (nodes, lists) in enumerate(zip(ds["nodefeatures"][n_train:], _slot_lists(ds, reduct))):
        for node, lst in zip(nodes[1:], lists):
            c = node[:-6].index(1) - 1
            if not lst:
                continue
            if g.random() < foreign:
                acts[b, c, :4] = np.r_[g.random(2), 0.9 + 0.1 * g.random(2)]
            else:
                acts[b, c, :4] = lst[int(g.integers(0, len(lst)))]
    return acts


def test_candidates_equal_host_qws_sized(dev, tmp_path, monkeypatch):
    from gnnpn_sc_amd import ops
    monkeypatch.chdir(tmp_path)
    ds = _qws_like(tmp_path)
    n_train = len(ds["nodefeatures"]) // 4 * 3
    acts = _picks(ds, 0, np.random.default_rng(5))
    assert acts.shape[0] >= 256
    svc, batch = _device_batch(ds, n_train, dev)
    for reduct in (0, 0.55):
        host, _s, _m = _host_tables("QWS", acts, reduct)
        tabs = ops.woa_candidates(svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds,
                                  torch.from_numpy(acts).to(dev), reduct=reduct, check_status=False)
        _assert_tables_equal(tabs, host)
        assert sum(1 for h in host if not isinstance(h, Exception)) > 200


def test_adds_front_randomized_differential(dev, tmp_path, monkeypatch):
    """addS's front (reduct in (0, 1)) with picks drawn from the front itself, so that members equal to a pick are skipped:
    >= 10^4 (problem, slot) scans against the host."""
    from gnnpn_sc_amd import ops
    monkeypatch.chdir(tmp_path)
    ds = _qws_like(tmp_path, n_problems=1100, seed=3, n_cat=30, n_services=1500)
    n_train = len(ds["nodefeatures"]) // 4 * 3
    svc, batch = _device_batch(ds, n_train, dev)
    g = np.random.default_rng(8)
    scans = 0
    for reduct in g.uniform(0.02, 0.98, 5):
        reduct = float(reduct)
        acts = _picks(ds, reduct, g, foreign=0.05)
        host, _s, _m = _host_tables("QWS", acts, reduct)
        tabs = ops.woa_candidates(svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds,
                                  torch.from_numpy(acts).to(dev), reduct=reduct, check_status=False)
        _assert_tables_equal(tabs, host)
        scans += int((batch.seg_ptr[1:] - batch.seg_ptr[:-1] - 1).sum())
    assert scans >= 10 ** 4


# ---- 3. ragged search ----------------------------------------------------------------------------------------------------

def _pack(problems, patches=()):
    from gnnpn_sc_amd import WOA
    prep = [WOA._prepare(s, c, sol, patches) for s, c, sol in problems]
    prob_ptr, cand_ptr, flat, len0, start, bounds = [0], [0], [], [], [], []
    for cats, l0, st, _r, bd in prep:
        for cat in cats:
            flat.extend(cat)
            cand_ptr.append(cand_ptr[-1] + len(cat))
        prob_ptr.append(prob_ptr[-1] + len(cats))
        len0.extend(l0)
        start.extend(st if st is not None else [-1] * len(cats))
        bounds.append(bd)
    return prob_ptr, cand_ptr, flat, len0, start, bounds


@pytest.mark.parametrize("sizes,wide", [((1, 3, 10, 33, 64, 7), None), ((1, 3, 10, 33, 64, 7), True),
                                        ((5, 64, 65, 100, 2, 130), None)])
def test_eswoa_ragged_equals_fine_tune(dev, sizes, wide):
    from gnnpn_sc_amd import WOA, ops
    from test_gpu_woa import _random_problems
    g = np.random.default_rng(sum(sizes))
    problems = []
    for T in sizes:
        problems += _random_problems(g, T, 3)
    order = g.permutation(len(problems))
    problems = [problems[i] for i in order]
    seeds = [321 + 5 * i for i in range(len(problems))]
    want = [WOA.fine_tune([p], popSize=12, MAX_Iter=9, seeds=[s], device=dev)[0] for p, s in zip(problems, seeds)]
    prob_ptr, cand_ptr, flat, len0, start, bounds = _pack(problems)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev)      # noqa: E731
    fit, pos, hist, draws, rows = ops.eswoa_ragged(t(prob_ptr, torch.int32), t(cand_ptr, torch.int32), t(len0, torch.int32),
                                                   t(flat, torch.float64).reshape(-1, 4), t(bounds, torch.float64),
                                                   t(start, torch.int32), 12, 9, t(seeds, torch.int64), wide=wide)
    fit, pos, hist, draws, rows = fit.cpu().tolist(), pos.cpu().tolist(), hist.cpu().tolist(), draws.cpu().tolist(), rows.cpu().tolist()
    for p, (w, (s, _c, _sol)) in enumerate(zip(want, problems)):
        T = len(s)
        assert fit[p] == w["bestFitness"], p
        assert hist[p] == w["bestFitnesses"], p
        assert draws[p] == w["draws"], p
        assert pos[p][:T] == [int(v) for v in w["bestPops"]], p
        assert [tuple(r) for r in rows[p][:T]] == [tuple(r) for r in w["bestSolutions"]], p


# ---- 4. the reference's own result ----------------------------------------------------------------------------------------

def test_refine_reproduces_the_reference_qualities(dev, tmp_path, monkeypatch):
    from gnnpn_sc_amd.pipeline import refine
    fx, ds, actions, n_train = _woa_driver(tmp_path, monkeypatch)
    p = fx["params"]
    svc, batch = _device_batch(ds, n_train, dev)
    n = actions.shape[0]
    for reduct in (0, 0.55):
        res = refine(svc, batch, {"actions": torch.from_numpy(actions).to(dev)}, p["popSize"], p["MAX_Iter"], reduct=reduct,
                          seeds=[p["base_seed"] + n_train + i for i in range(n)], min_cost=ds["minCostList"][n_train:])
        assert res["quality"].cpu().tolist() == fx["modes"][str(reduct)]["quality"], reduct


# ---- 5. chained on a real run -----------------------------------------------------------------------------------------------

def test_refine_after_run_equals_fine_tune(dev, tmp_path, monkeypatch):
    import gnnpn_sc_amd.synth as synth
    from gnnpn_sc_amd import WOA
    from gnnpn_sc_amd.loadData import loadDataOther
    from gnnpn_sc_amd.modelML import Net
    from gnnpn_sc_amd.modelPN import CombinatorialRL, reward
    from gnnpn_sc_amd.pipeline import ML2PNPipeline
    from oracle import ml as oml, pn as opn
    monkeypatch.chdir(tmp_path)
    T, S, K, H, P = 6, 60, 3, 256, 96
    ds = synth.make_dataset(T, S, P, seed=21, tasks_per_problem=3, lo_range=(0.85, 0.96))
    synth.write_dataset(str(tmp_path), "QWS", ds)
    n_train = P // 4 * 3
    svc, batch = _device_batch(ds, n_train, dev)
    net = Net(128, S, 20, 2, 2)
    net.load_state_dict(oml.make_state_dict(128, 20, 2, 2, seed=7))
    low = CombinatorialRL(0, H, T * K, 0, 10, 1, reward, "Dot", K, T, level="Low")
    high = CombinatorialRL(0, H, T * K, 0, 10, 1, reward, "Dot", K, T, level="High")
    low.load_state_dict(opn.make_state_dict(H, 8))
    high.load_state_dict(opn.make_state_dict(H, 9))
    pipe = ML2PNPipeline(net.to(dev).eval(), low.to(dev).eval(), high.to(dev).eval(), K)
    out = pipe.run(svc, batch)
    seeds = [77 + i for i in range(P - n_train)]
    actions = out["actions"].double().cpu().numpy()
    host, sols, mins = _host_tables("QWS", actions, 0)
    feats, cons, _m = loadDataOther("QWS", 0, sSetList=[{tuple(round(v, 5) for v in r) for r in s} for s in sols])
    if any(isinstance(h, Exception) for h in host):
        with pytest.raises(WOA.GnnpnError, match="problem"):
            pipe.refine(svc, batch, out, 10, 12, seeds=seeds)
        return
    res = pipe.refine(svc, batch, out, 10, 12, seeds=seeds, min_cost=mins[n_train:])
    want = WOA.fine_tune([(feats[b], cons[b], sols[b] or None) for b in range(P - n_train)], 10, 12, seeds, dev)
    fit, hist, draws = res["best_fitness"].cpu().tolist(), res["history"].cpu().tolist(), res["draws"].cpu().tolist()
    rows, n_slots, quality = res["best_rows"].cpu().tolist(), res["n_slots"].cpu().tolist(), res["quality"].cpu().tolist()
    for b, w in enumerate(want):
        assert fit[b] == w["bestFitness"] and hist[b] == w["bestFitnesses"] and draws[b] == w["draws"], b
        assert [tuple(r) for r in rows[b][:n_slots[b]]] == [tuple(r) for r in w["bestSolutions"]], b
        assert quality[b] == mins[n_train + b] / w["bestFitness"], b


# ---- 6. failure paths --------------------------------------------------------------------------------------------------------

def test_row_count_mismatch_raises_like_the_host(dev, tmp_path, monkeypatch):
    from gnnpn_sc_amd import WOA
    from gnnpn_sc_amd.pipeline import refine
    fx, ds, actions, n_train = _woa_driver(tmp_path, monkeypatch)
    nodes = ds["nodefeatures"][n_train + 7]
    present = {n[:-6].index(1) - 1 for n in nodes[1:]}
    absent = next(c for c in range(actions.shape[1]) if c not in present)
    actions[7, absent, :4] = [0.25, 0.5, 0.95, 0.97]                                   # one row more than lists
    host, _s, _m = _host_tables("QWS", actions, 0)
    assert isinstance(host[7], WOA.GnnpnError)
    svc, batch = _device_batch(ds, n_train, dev)
    with pytest.raises(WOA.GnnpnError, match="problem 7"):
        refine(svc, batch, {"actions": torch.from_numpy(actions).to(dev)}, 4, 3, seeds=list(range(1000)))


def test_category_beyond_fifty_is_unsupported(dev, tmp_path, monkeypatch):
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.loadData import loadDataOther
    monkeypatch.chdir(tmp_path)
    ds = _qws_like(tmp_path, n_problems=40, seed=4, n_cat=53, n_services=600, tasks=12)
    n_train = 30
    with pytest.raises(IndexError):
        loadDataOther("QWS", 0)
    svc, batch = _device_batch(ds, n_train, dev)
    acts = torch.zeros(10, 53, 8, dtype=torch.float64, device=dev)
    acts[:, :, 1:4] = 1.0
    tabs = ops.woa_candidates(svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds, acts,
                              check_status=False)
    high = [any(n[:-6].index(1) - 1 >= 50 for n in nodes[1:]) for nodes in ds["nodefeatures"][n_train:]]
    assert any(high)
    status = tabs["status"].cpu().tolist()
    for b, h in enumerate(high):
        if h:
            assert status[b] == -2, b                                                   # GNNPN_E_UNSUP
    first = next(b for b, st in enumerate(status) if st != 0)
    with pytest.raises(ops.GnnpnError, match=f"problem {first}: status {status[first]}"):
        ops.woa_candidates(svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds, acts)


# ---- 7. CLI ------------------------------------------------------------------------------------------------------------------

def test_main_cli_infer_woa_equals_the_woa_approach(dev, tmp_path, monkeypatch):
    from test_host_logic import _woa_driver_setup
    monkeypatch.chdir(tmp_path)
    fx, _a, _n = _woa_driver_setup(str(tmp_path))
    p = fx["params"]
    (tmp_path / "environment.ini").write_text(
        f"[QWS-WOA]\nserCategory = {p['T']}\nMLESWOAtest = 0\nML2PNWOATest = 1\nMLWOATest = 0\nESWOAtest = 0\n"
        f"serviceNumber = 4\nreduct = 0\nepoch = -1\nMAX_Iter = {p['MAX_Iter']}\npopSize = {p['popSize']}\n")
    import main as cli
    path = "./solutions/WOA/QWS//ML+2PN+WOA.txt"
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["main.py", "QWS", "ML+2PN", "--infer", "--random-init", "--woa", "--seed", str(p["base_seed"])]) == 0
    with open(path) as f:
        device = json.load(f)
    os.remove(path)
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["main.py", "QWS", "WOA", "--seed", str(p["base_seed"])]) == 0
    with open(path) as f:
        host = json.load(f)
    assert len(device["quality"]) == 1000
    assert device["quality"] == host["quality"]
    assert device["averageQ"] == host["averageQ"]
