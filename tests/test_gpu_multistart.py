"""-m gpu: multi-start descent on the device — the candidate tables of B * R (problem, replica) rows
(gnnpn_woa_candidates_replicas_count / _fill) against the host path of every replica, the selection (gnnpn_descend_select_f64)
against tests/multistart_reference.py on hand-made fields, descent over replicas, pipeline.descend_starts after best_of and
`main.py ... --infer --samples=N --descend --all-starts`.  Every float64 and every position is compared with ``==``."""
import contextlib
import io
import json
import math

import numpy as np
import pytest
import torch

import descent_reference as ref
import multistart_reference as mref
from test_gpu_descend import H_, K_, N_TRAIN, P_, T_, chain      # noqa: F401  (chain: the module-scoped fixture, set up once for this file)
from test_multistart_host import RAGGED

pytestmark = pytest.mark.gpu


# ---- 1. candidate tables of replicas against the host path of every replica ------------------------------------------------------

FOREIGN = [0.25, 0.5, 0.95, 0.97]
ROW_FOREIGN, ROW_NO_START, ROW_RAISES = (3, 1), (5, 2), (7, 1)      # (problem, replica)


def _real(row):
    return sum(row[:4].tolist()) != 3          # the host's test for a dummy row (WOA.py:194-208)


def _replicas(ds, actions, n_train, R):
    """[n, R, T, 8] float64: replica 0 = ``actions``; in replicas >= 1 every pick is replaced by a random member of its category; one
    foreign row, one replica of all dummy rows, and (replica 1 of problem 7) a row in an absent category: the host raises."""
    g = np.random.default_rng(41)
    sf = ds["serviceFeature"]
    n, T = actions.shape[:2]
    out = np.repeat(actions[:, None], R, axis=1).copy()
    for r in range(1, R):
        for b in range(n):
            for c in range(T):
                if _real(out[b, r, c]):
                    members = sf[str(c + 1)]
                    out[b, r, c, :4] = members[int(g.integers(0, len(members)))]
    if R > ROW_FOREIGN[1]:
        b, r = ROW_FOREIGN
        out[b, r, next(c for c in range(T) if _real(out[b, r, c])), :4] = FOREIGN
    if R > ROW_NO_START[1]:
        b, r = ROW_NO_START
        out[b, r, :, :4] = [0.0, 1.0, 1.0, 1.0]
    if R > ROW_RAISES[1]:
        b, r = ROW_RAISES
        present = {nd[:-6].index(1) - 1 for nd in ds["nodefeatures"][n_train + b][1:]}
        out[b, r, next(c for c in range(T) if c not in present), :4] = FOREIGN      # one row more than lists
    return out


@pytest.mark.parametrize("reduct", [0, 0.55])
def test_replica_tables_equal_host_on_the_driver_fixture(dev, tmp_path, monkeypatch, reduct):
    from gnnpn_sc_amd import WOA, ops
    from test_gpu_refine import _assert_tables_equal, _device_batch, _host_tables, _woa_driver
    fx, ds, actions, n_train = _woa_driver(tmp_path, monkeypatch)
    svc, batch = _device_batch(ds, n_train, dev)
    n = actions.shape[0]
    reps = _replicas(ds, actions, n_train, 5)
    operands = (svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds)
    for dt in (torch.float64,) if reduct else (torch.float64, torch.float32):
        a_all = torch.from_numpy(reps).to(dev, dt)
        seen = a_all.double().cpu().numpy()             # f32 actions: the host sees them widened
        host = [_host_tables("QWS", seen[:, r], reduct)[0] for r in range(5)]
        for R in (1, 2, 5):
            a = a_all[:, :R].contiguous()
            tabs = ops.woa_candidates_replicas(*operands, a, reduct=reduct, check_status=False)
            assert tabs["replicas"] == R and tabs["status"].numel() == n * R
            rows = [host[q % R][q // R] for q in range(n * R)]                   # row q = b * R + r
            _assert_tables_equal(tabs, rows)
            assert tabs["max_slots"] == max(len(h[0]) for h in rows if not isinstance(h, Exception))
            if R == 1:
                one = ops.woa_candidates(*operands, a[:, 0].contiguous(), reduct=reduct, check_status=False)
                assert set(one) | {"replicas"} == set(tabs)
                for k, v in one.items():
                    assert torch.equal(v, tabs[k]) if isinstance(v, torch.Tensor) else v == tabs[k], k
                continue
            # the rows made on purpose: a foreign pick appended, no start at all, a replica the host raises on
            b, r = ROW_FOREIGN
            cats, len0, start, _bd = rows[b * R + r]
            assert any(len(c) == l0 + 1 for c, l0 in zip(cats, len0)) and start is not None
            bad = ROW_RAISES[0] * R + ROW_RAISES[1]
            assert isinstance(rows[bad], WOA.GnnpnError) and tabs["status"][bad].item() == 1
            first = next(q for q, h in enumerate(rows) if isinstance(h, Exception))
            with pytest.raises(ops.GnnpnError, match=f"problem {first // R} replica {first % R}: status"):
                ops.woa_candidates_replicas(*operands, a, reduct=reduct)
            if R > ROW_NO_START[1]:
                b, r = ROW_NO_START
                assert rows[b * R + r][2] is None
        if reduct:      # the kept lists depend on the replica's picks: tables cannot be shared between the replicas of a problem
            kept = lambda h: [cat[:l0] for cat, l0 in zip(h[0], h[1])]      # noqa: E731
            assert any(not isinstance(host[r][b], Exception) and not isinstance(host[s][b], Exception) and kept(host[r][b]) != kept(host[s][b])
                       for b in range(n) for r in range(5) for s in range(r + 1, 5))


# ---- 2. the selection on hand-made fields ---------------------------------------------------------------------------------------------

def _fitness(case, R, g):
    """One problem's best_fitness over R replicas.  0: the minimum twice, in two different 64-lane strides where R allows (else twice
    in one stride); 1: a NaN below and above the winner; 2: -0.0 first, 0.0 and -0.0 after it; 3: every row NaN; 4: 0.0 first, -0.0 after."""
    f = g.choice([0.25, 0.5, 0.75, 1.0], R)
    nan = math.nan
    if case == 0 and R >= 2:
        i, j = (69, 129) if R >= 130 else (3, 64) if R >= 65 else (R // 2 if R > 2 else 0, R - 1)
        f[i] = f[j] = 0.125
    elif case == 1:
        if R >= 3:
            f[0] = f[R - 1] = nan
            f[R // 2] = 0.125
            if R >= 66:
                f[R // 2 - 64 if R // 2 >= 64 else 1] = nan      # a NaN in the winner's own lane too
        else:
            f[0] = nan
    elif case in (2, 4) and R >= 3:
        f += 1.0
        f[R // 2], f[R - 1] = 0.0, -0.0
        if case == 2:
            f[0] = -0.0
    elif case == 3:
        f[:] = nan
    return f


SELECT_CASES = [(1, 1, 1, 1, 2, torch.float32, (3,)), (1, 1, 7, 16, 3, torch.float64, (0,)), (3, 2, 7, 1, 5, torch.float64, (0, 1, 4)),
                (3, 63, 64, 16, 6, torch.float32, (0, 1, 2)), (3, 64, 65, 1, 64, torch.float64, (0, 1, 3)),
                (1, 65, 300, 16, 7, torch.float32, (0,)), (3, 65, 1, 16, 2, torch.float64, (2, 4, 0)),
                (3, 130, 65, 16, 9, torch.float32, (0, 1, 2)), (1, 130, 300, 1, 301, torch.float64, (1,)),
                (3, 130, 7, 1, 3, torch.float64, (4, 3, 2))]


@pytest.mark.parametrize("B,R,max_slots,hist_ld,aT,dt,cases", SELECT_CASES)
def test_selection_is_the_reference_rule(dev, B, R, max_slots, hist_ld, aT, dt, cases):
    from gnnpn_sc_amd import ops
    g = np.random.default_rng(B * 1000 + R)
    Q = B * R
    fit = np.concatenate([_fitness(c, R, g) for c in cases])
    f = {"best_fitness": fit, "start_fitness": g.random(Q) + 1.0, "sweeps": np.where(np.isnan(fit), -1, g.integers(1, 17, Q)).astype(np.int32),
         "moves": g.integers(0, 40, Q).astype(np.int32), "best_pos": g.integers(0, 9, (Q, max_slots)).astype(np.int32),
         "best_rows": g.random((Q, max_slots, 4)), "history": g.random((Q, hist_ld))}
    f["start_fitness"][np.isnan(fit)] = math.nan
    n_slots = g.integers(1, max_slots + 1, Q).astype(np.int32)
    actions = g.random((B, R, aT, 8)).astype(np.float32 if dt == torch.float32 else np.float64)
    got = ops.descend_select({k: torch.from_numpy(v).to(dev) for k, v in f.items()}, torch.from_numpy(actions).to(dev),
                             torch.from_numpy(n_slots).to(dev))
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert got["actions"].dtype == actions.dtype and got["actions"].shape == (B, aT, 8)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)      # noqa: E731  (NaN == NaN by bits)
    for b in range(B):
        rows = [{"best_fitness": float(v)} for v in fit[b * R:(b + 1) * R]]
        w = mref.select(rows)
        q = b * R + w
        assert got["start_index"][b] == w, (b, w)
        for k in ("best_fitness", "start_fitness", "best_rows", "history"):
            assert (bits(got[k][b]) == bits(f[k][q])).all(), (b, k)
        for k in ("sweeps", "moves", "best_pos"):
            assert (got[k][b] == f[k][q]).all(), (b, k)
        assert got["n_slots"][b] == n_slots[q] and (bits(got["actions"][b]) == bits(actions[b, w])).all(), b
    # what the cases are there for: the expected winners, written down
    for b, c in enumerate(cases):
        w = int(got["start_index"][b])
        if c == 0 and R >= 2:
            assert w == (69 if R >= 130 else 3 if R >= 65 else R // 2 if R > 2 else 0) and fit[b * R + w] == 0.125
            assert np.count_nonzero(fit[b * R:(b + 1) * R] == 0.125) >= 2
        if c == 1:
            assert w == (R // 2 if R >= 3 else 1 if R == 2 else 0)
        if c == 2 and R >= 3:
            assert w == 0 and math.copysign(1.0, got["best_fitness"][b]) == -1.0 and fit[b * R + R // 2] == 0.0
        if c == 4 and R >= 3:
            assert w == R // 2 and math.copysign(1.0, got["best_fitness"][b]) == 1.0 and math.copysign(1.0, fit[b * R + R - 1]) == -1.0
        if c == 3 or (c == 1 and R == 1):
            assert w == 0 and math.isnan(got["best_fitness"][b]) and got["sweeps"][b] == -1


# ---- 3. descent over replicas: one descend_ragged over B * R rows, then the selection ----------------------------------------------

def _descend_rows(dev, tables, R, max_sweeps):
    """tables: per problem R (cats, bounds, start).  -> (per-row dict, winners' dict), as lists."""
    from gnnpn_sc_amd import ops
    flat = [tab for reps in tables for tab in reps]                       # row q = b * R + r
    prob_ptr, cand_ptr, cand, bounds, start = ref.pack(flat)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev)      # noqa: E731
    per_row = ops.descend_ragged(t(prob_ptr, torch.int32), t(cand_ptr, torch.int32), t(cand, torch.float64).reshape(-1, 4),
                                 t(bounds, torch.float64), t(start, torch.int32), max_sweeps=max_sweeps)
    actions = torch.arange(len(tables) * R * 2 * 8, dtype=torch.float32, device=dev).view(len(tables), R, 2, 8)
    n_slots = t([len(tab[0]) for tab in flat], torch.int32)
    win = ops.descend_select(per_row, actions, n_slots)
    assert torch.equal(win["actions"], actions[torch.arange(len(tables), device=dev), win["start_index"].long()])
    return {k: v.cpu().tolist() for k, v in per_row.items()}, {k: v.cpu().tolist() for k, v in win.items()}


def _assert_winners(per_row, win, tables, want, R):
    for b, (reps, w) in enumerate(zip(tables, want)):
        T = len(reps[w["start_index"]][0])
        for k in ("start_index", "best_fitness", "start_fitness", "history", "sweeps", "moves"):
            assert win[k][b] == w[k], (b, T, k, win[k][b], w[k])
        assert win["n_slots"][b] == T and win["best_pos"][b][:T] == w["best_pos"], (b, T)
        assert [tuple(r) for r in win["best_rows"][b][:T]] == w["best_rows"], (b, T)
        for k, field in (("fitness_all", "best_fitness"), ("start_fitness_all", "start_fitness"), ("sweeps_all", "sweeps"), ("moves_all", "moves")):
            assert per_row[field][b * R:(b + 1) * R] == w[k], (b, T, k)


@pytest.mark.parametrize("max_sweeps", [16, 1])
@pytest.mark.parametrize("R", [2, 5])
@pytest.mark.parametrize("T", [1, 7, 9, 64, 65, 129])
def test_descent_over_replicas(dev, T, R, max_sweeps):
    """T <= 64: the lane form; 65 and 129: the workgroup form (129: np.sum recurses)."""
    key = (700 + T, (T,), 3 if T <= 64 else 2, R)
    tables = mref.replica_tables(*key)
    _assert_winners(*_descend_rows(dev, tables, R, max_sweeps), tables, mref.replica_runs(*key, False, max_sweeps), R)


@pytest.mark.parametrize("max_sweeps", [16, 1])
def test_descent_over_replicas_ragged(dev, max_sweeps):
    R = RAGGED[3]
    tables = mref.replica_tables(*RAGGED)
    _assert_winners(*_descend_rows(dev, tables, R, max_sweeps), tables, mref.replica_runs(*RAGGED, max_sweeps), R)


# ---- 4. the pipeline: best_of(return_all=True) -> descend_starts -> refine --------------------------------------------------------------

def _list(res):
    return {k: v.cpu().tolist() for k, v in res.items()}


def test_pipeline_descend_starts_after_best_of(dev, chain, monkeypatch):      # noqa: F811
    from gnnpn_sc_amd import WOA
    from gnnpn_sc_amd.pipeline import descend, descend_starts, refine
    from test_gpu_refine import _host_tables
    pipe, svc, batch, mins = chain["pipe"], chain["svc"], chain["batch"], chain["mins"]
    monkeypatch.chdir(chain["tmp"])
    B, N = P_ - N_TRAIN, 4
    assert B == 24
    out = pipe.best_of(svc, batch, N, seed=5, return_all=True)
    all_rows = out["actions_all"]
    assert all_rows.shape[:3] == (B, N, T_) and torch.equal(all_rows[:, 0], pipe.run(svc, batch)["actions"])      # replica 0: the greedy rows
    seen = all_rows[..., -8:].double().cpu().numpy()
    host = [_host_tables("QWS", seen[:, r], 0)[0] for r in range(N)]
    if any(isinstance(h, Exception) for hr in host for h in hr):
        with pytest.raises(WOA.GnnpnError, match="problem .* replica"):
            pipe.descend_starts(svc, batch, out)
        return
    res = pipe.descend_starts(svc, batch, out, min_cost=mins[N_TRAIN:])
    got = _list(res)
    tables = [[(host[r][b][0], host[r][b][3], host[r][b][2]) for r in range(N)] for b in range(B)]
    want = [mref.descend_starts(reps) for reps in tables]
    per_row = {f: [v for b in range(B) for v in got[k][b]] for k, f in (("fitness_all", "best_fitness"), ("start_fitness_all", "start_fitness"),
                                                                        ("sweeps_all", "sweeps"), ("moves_all", "moves"))}
    _assert_winners(per_row, got, tables, want, N)
    print("descend_starts: start_index", got["start_index"], "mean merit", sum(got["best_fitness"]) / B)
    assert got["quality"] == [mins[N_TRAIN + b] / w["best_fitness"] for b, w in enumerate(want)]
    idx = res["start_index"].long()
    assert torch.equal(res["actions"], all_rows[..., -8:][torch.arange(B, device=dev), idx])
    assert res["fitness_all"].shape == (B, N) and res["fitness_all"].dtype == torch.float64 and res["sweeps_all"].dtype == torch.int32
    # never worse than descent from the greedy rows alone, and equal where the greedy replica wins
    greedy = descend(svc, batch, {"actions": all_rows[:, 0].contiguous()})["best_fitness"].cpu().tolist()
    for b in range(B):
        assert got["best_fitness"][b] <= greedy[b], b
        if got["start_index"][b] == 0:
            assert got["best_fitness"][b] == greedy[b], b
    # the starts as a plain tensor, and as a method of the pipeline: the same result
    again = descend_starts(svc, batch, all_rows)
    assert all(torch.equal(again[k], res[k]) for k in again)
    # ES-WOA from the winner: refine rebuilds its tables and repeats its descent
    seeds = torch.tensor([77 + i for i in range(B)], dtype=torch.int64, device=dev)
    refined = refine(svc, batch, res, 10, 12, seeds=seeds, descend=16)
    m = min(refined["descent"]["best_pos"].shape[1], res["best_pos"].shape[1])      # max_slots: of the winners there, of all rows here
    assert torch.equal(refined["descent"]["best_pos"][:, :m], res["best_pos"][:, :m]) and not res["best_pos"][:, m:].any()
    for k in ("best_fitness", "history"):
        assert torch.equal(refined["descent"][k], res[k]), k
    assert all(r <= d for r, d in zip(refined["best_fitness"].cpu().tolist(), got["best_fitness"]))
    # return_all=False: today's result, key for key
    plain = pipe.best_of(svc, batch, N, seed=5)
    assert "actions_all" not in plain and set(plain) | {"actions_all"} == set(out)
    for k, v in plain.items():
        assert torch.equal(v, out[k]), k


# ---- 5. the CLI -----------------------------------------------------------------------------------------------------------------------

def test_main_cli_infer_all_starts(dev, chain, monkeypatch):      # noqa: F811
    tmp = chain["tmp"]
    monkeypatch.chdir(tmp)
    (tmp / "environment.ini").write_text(
        f"[QWS-PNHigh]\nembeddingTag = 0\nUSE_CUDA = 1\nserCategory = {T_}\nepochDiv = 1\nserNumber = {K_}\nhidden_size = {H_}\n"
        "n_glimpses = 0\ntanh_exploration = 10\nuse_tanh = 1\nbeta = 0.9\nmax_grad_norm = 2.\nlr = 0.5e-4\nepochML = -1\nepochPNLow = -1\n"
        f"[QWS-ML+2PN]\nserviceCategory = {T_}\nepoch = -1\n"
        f"[QWS-WOA]\nserCategory = {T_}\nMLESWOAtest = 0\nML2PNWOATest = 1\nMLWOATest = 0\nESWOAtest = 0\n"
        "serviceNumber = 4\nreduct = 0\nepoch = -1\nMAX_Iter = 5\npopSize = 6\n")
    import main as cli
    base = ["main.py", "QWS", "ML+2PN", "-1", "--infer", "--random-init", "--samples=4", "--descend=4", "--seed", "3"]

    def run(*extra):
        with contextlib.redirect_stdout(io.StringIO()):
            assert cli.main(base + list(extra)) == 0
        out = {}
        for name in ("descent", "multistart", "WOA"):
            with contextlib.suppress(FileNotFoundError), open(f"./solutions/WOA/QWS/ML+2PN+{name}.txt") as f:
                out[name] = json.load(f)
        return out
    one = run()
    assert "multistart" not in one                                     # without the flag nothing changes
    multi = run("--all-starts")
    n = P_ - N_TRAIN
    m, d = multi["multistart"]["quality"], one["descent"]["quality"]
    print("mean quality: descent", sum(d) / len(d), "multistart", sum(m) / len(m))
    assert len(m) == len(d) == n and multi["multistart"]["averageQ"] == sum(m) / n
    assert multi["descent"] == one["descent"]                          # multistart.txt takes its place: descent.txt is not rewritten
    # the best-of winner by R is one of the starts, and merits here are positive: quality = min_cost / merit does not fall
    assert all(a >= b > 0 for a, b in zip(m, d))
    both = run("--all-starts", "--woa")
    assert both["multistart"]["quality"] == m
    assert all(r >= a for r, a in zip(both["WOA"]["quality"], m))
