"""-m gpu: the pair-swap descent on the device — gnnpn_descend_pairs_ragged_f64 (descend_pairs_kernel: one wavefront per problem),
ops.descend_pairs_ragged, pipeline.descend_pairs / descend_starts_pairs / refine(pair_rounds=r) and `main.py ... --descend --pairs` —
against the plain-Python restatement of the search (tests/pair_descent_reference.py, built on descent_reference): every float64,
every position and every counter, ``==``."""
import contextlib
import functools
import io
import json

import numpy as np
import pytest
import torch

import descent_reference as ref
import multistart_reference as mref
import pair_descent_reference as pref
from test_gpu_descend import H_, K_, N_TRAIN, P_, T_, _tables, chain      # noqa: F401  (chain: the module-scoped fixture, set up once here)

pytestmark = pytest.mark.gpu

FIELDS = ("best_fitness", "start_fitness", "round_history", "sweeps", "moves", "rounds", "pair_moves", "converged")


# ---- helpers: the reference runs (computed once, shared), one launch --------------------------------------------------------------

def _key(T):
    return (1264, (64,), 2, 6) if T == 64 else (1200 + T, (T,), 4, 8)


LONG = (1300, (3,), 4, 140)
RAGGED = (1400, (1, 3, 10, 33, 7, 2), 4, 8, True)        # four per size: every fourth problem of a size has no start


@functools.lru_cache(maxsize=None)
def _want(key, max_sweeps=16, max_rounds=4):
    return tuple(pref.descend_pairs(*tab, max_sweeps=max_sweeps, max_rounds=max_rounds) for tab in _tables(*key))


def _operands(dev, tables):
    prob_ptr, cand_ptr, flat, bounds, start = ref.pack(tables)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev)      # noqa: E731
    return [t(prob_ptr, torch.int32), t(cand_ptr, torch.int32), t(flat, torch.float64).reshape(-1, 4), t(bounds, torch.float64),
            t(start, torch.int32)]


def _launch(dev, tables, max_sweeps=16, max_rounds=4, **kw):
    from gnnpn_sc_amd import ops
    res = ops.descend_pairs_ragged(*_operands(dev, tables), max_sweeps=max_sweeps, max_rounds=max_rounds, **kw)
    return {k: v.cpu().tolist() for k, v in res.items()}


def _assert_equal(got, tables, want, fields=FIELDS):
    for p, ((cats, _b, _s), w) in enumerate(zip(tables, want)):
        T = len(cats)
        for k in fields:
            assert got[k][p] == w[k], (p, T, k, got[k][p], w[k])
        assert got["best_pos"][p][:T] == w["best_pos"], (p, T)
        assert [tuple(r) for r in got["best_rows"][p][:T]] == w["best_rows"], (p, T)


def _call_entry(dev, entry, tables, max_slots, max_cand, max_sweeps, max_rounds, tail=(), short=()):
    """The pair entry ``entry`` of the C ABI itself, over buffers filled with the sentinel -7: ``tail`` the scalars it has behind
    max_rounds, ``short`` = (columns,) for the entry with a shortlist output ((None,): a NULL pointer).  Returns the dict of lists."""
    from gnnpn_sc_amd import _lib, ops
    ops_in = _operands(dev, tables)
    B = len(tables)
    F64, I32 = torch.float64, torch.int32
    f = {k: torch.full((B,), -7.0, dtype=F64, device=dev) for k in ("best_fitness", "start_fitness")}
    i = {k: torch.full((B,), -7, dtype=I32, device=dev) for k in ("sweeps", "moves", "rounds", "pair_moves", "converged")}
    pos, rows = torch.full((B, max_slots), -7, dtype=I32, device=dev), torch.full((B, max_slots, 4), -7.0, dtype=F64, device=dev)
    hist = torch.full((B, max(max_rounds, 1)), -7.0, dtype=F64, device=dev)
    more = {"shortlist": None if m is None else torch.full((B, max_slots, m), -7, dtype=I32, device=dev) for m in short}
    ops.check(getattr(_lib.load(), entry)(
        B, ops.dev_ptr(ops_in[0], I32, "prob_ptr"), ops_in[4].numel(), max_slots, max_cand, ops.dev_ptr(ops_in[1], I32, "cand_ptr"),
        ops.dev_ptr(ops_in[2], F64, "cand"), ops.dev_ptr(ops_in[3], F64, "bounds"), ops.dev_ptr(ops_in[4], I32, "start_pos"),
        max_sweeps, max_rounds, *tail, ops.dev_ptr(f["best_fitness"], F64, "f"), ops.dev_ptr(f["start_fitness"], F64, "s"),
        ops.dev_ptr(pos, I32, "p"), ops.dev_ptr(rows, F64, "r"), ops.dev_ptr(hist, F64, "h"), ops.dev_ptr(i["sweeps"], I32, "sw"),
        ops.dev_ptr(i["moves"], I32, "m"), ops.dev_ptr(i["rounds"], I32, "ro"), ops.dev_ptr(i["pair_moves"], I32, "pm"),
        ops.dev_ptr(i["converged"], I32, "c"), *(ops.dev_ptr(t, I32, "sl", allow_none=True) for t in more.values()), ops.stream_ptr()), entry)
    return {**{k: v.cpu().tolist() for k, v in {**f, **i}.items()}, "best_pos": pos.cpu().tolist(), "best_rows": rows.cpu().tolist(),
            "round_history": hist.cpu().tolist(), **{k: t.cpu().tolist() for k, t in more.items() if t is not None}}


def _write_cli_ini(tmp):
    """The environment.ini of the `main.py QWS ML+2PN -1 --infer ...` runs of the pair-swap tests, into ``tmp``."""
    (tmp / "environment.ini").write_text(
        f"[QWS-PNHigh]\nembeddingTag = 0\nUSE_CUDA = 1\nserCategory = {T_}\nepochDiv = 1\nserNumber = {K_}\nhidden_size = {H_}\n"
        "n_glimpses = 0\ntanh_exploration = 10\nuse_tanh = 1\nbeta = 0.9\nmax_grad_norm = 2.\nlr = 0.5e-4\nepochML = -1\nepochPNLow = -1\n"
        f"[QWS-ML+2PN]\nserviceCategory = {T_}\nepoch = -1\n"
        f"[QWS-WOA]\nserCategory = {T_}\nMLESWOAtest = 0\nML2PNWOATest = 1\nMLWOATest = 0\nESWOAtest = 0\n"
        "serviceNumber = 4\nreduct = 0\nepoch = -1\nMAX_Iter = 5\npopSize = 6\n")


# ---- 1. slot counts ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 2, 3, 7, 8, 9, 33, 64])
def test_pair_descend_sizes(dev, T):
    """T = 1 has no pair; 7 / 8 / 9 straddle numpy's switch to eight accumulators with two replaced elements; 64 fills the wave."""
    key = _key(T)
    want = _want(key)
    _assert_equal(_launch(dev, _tables(*key)), _tables(*key), want)
    if T == 1:
        assert all(w["rounds"] == 1 and w["pair_moves"] == 0 and w["converged"] == 1 for w in want)


def test_the_size_cases_move_by_pairs():
    """What keeps the comparisons above from being trivial: at every T >= 2 of the list a pair sweep moves in some problem, all
    runs converge within the four rounds, and somewhere a pair removes a violation."""
    for T in (2, 3, 7, 8, 9, 33, 64):
        want = _want(_key(T))
        assert any(w["pair_moves"] > 0 for w in want), T
        assert all(w["converged"] == 1 for w in want), T
    gains = [ref.descend(*tab)["best_fitness"] - w["best_fitness"] for T in (3, 7) for tab, w in zip(_tables(*_key(T)), _want(_key(T)))]
    assert max(gains) > 0.5
    assert any(w["rounds"] >= 3 for w in _want(_key(7)))


def test_pair_descend_lists_longer_than_a_wave(dev):
    """Lists of up to 139 candidates: pair products of up to 19 321, in chunks of 64."""
    tables = _tables(*LONG)
    assert max(len(a) * len(b) for cats, _b, _s in tables for i, a in enumerate(cats) for b in cats[i + 1:]) > 64 * 128
    assert any(w["pair_moves"] > 0 for w in _want(LONG))
    _assert_equal(_launch(dev, tables), tables, _want(LONG))


# ---- 2. a ragged batch -----------------------------------------------------------------------------------------------------------------

def test_pair_descend_ragged_batch(dev):
    tables = _tables(*RAGGED)
    _assert_equal(_launch(dev, tables), tables, _want(RAGGED))


def test_the_ragged_batch_covers_every_kind_of_start():
    from test_gpu_woa import _random_problems
    seed, sizes, n, mc, _permute = RAGGED
    g = np.random.default_rng(seed)
    problems = []
    for T in sizes:
        problems += _random_problems(g, T, n, mc)
    problems = [problems[i] for i in g.permutation(len(problems))]
    kinds = set()
    for (services, _c, _sol), (cats, _b, start) in zip(problems, _tables(*RAGGED)):
        foreign = start is not None and any(len(c) > len(s) for c, s in zip(cats, services))
        kinds.add("none" if start is None else "foreign" if foreign else "member")
    assert kinds == {"none", "foreign", "member"}
    assert sorted({len(cats) for cats, _b, _s in _tables(*RAGGED)}) == sorted(sizes)
    assert any(w["pair_moves"] > 0 for w in _want(RAGGED))


# ---- 3. walls, ties and strictness, on hand-built tables --------------------------------------------------------------------------------

GOOD, POOR = (0.1, 0.9, 0.99, 0.99), (0.8, 0.2, 0.99, 0.99)
BOUNDS = [0.5, 1.0, 0.5, 1.0]


def test_pair_descend_wall_ties_and_strictness(dev):
    tables = [pref.wall_problem(),                                       # a violated bound that exactly one pair repairs
              pref.wall_problem(twice=True),                             # the same best pair four times: the lowest (a, b)
              ([[GOOD, GOOD], [POOR, POOR]], BOUNDS, [1, 1]),            # every pair has exactly the current merit
              ([[POOR] + [GOOD] * 70, [POOR] * 3 + [GOOD] * 66], BOUNDS, [0, 0])]      # equal best pairs in many chunks
    want = [pref.descend_pairs(*tab) for tab in tables]
    one = ref.descend(*tables[0])
    assert one["moves"] == 0 and pref.improving_pairs(tables[0][0], tables[0][1], one["best_pos"], one["best_fitness"]) == [(0, 1, 1, 1)]
    got = _launch(dev, tables)
    _assert_equal(got, tables, want)
    assert got["pair_moves"][0] == 1 and got["start_fitness"][0] - got["best_fitness"][0] > 0.5 and got["best_pos"][0] == [1, 1]
    assert got["rounds"][0] == 2 and got["converged"][0] == 1
    assert got["best_pos"][1][:2] == [1, 1] and got["pair_moves"][1] == 1
    assert got["best_pos"][2][:2] == [1, 1] and got["pair_moves"][2] == 0 and got["rounds"][2] == 1 and got["converged"][2] == 1
    assert got["best_pos"][3][:2] == [1, 3] and got["pair_moves"][3] == 0            # the one-swap sweeps got there first
    pairs_only = _launch(dev, tables[3:], max_sweeps=0)                              # ... and without them one pair move does
    _assert_equal(pairs_only, tables[3:], [pref.descend_pairs(*tables[3], max_sweeps=0)])
    assert pairs_only["best_pos"][0][:2] == [1, 3] and pairs_only["pair_moves"] == [1] and pairs_only["moves"] == [0]


# ---- 4. cut-offs ---------------------------------------------------------------------------------------------------------------------

def test_pair_descend_without_rounds_is_descend_ragged(dev):
    from gnnpn_sc_amd import ops
    tables = _tables(*RAGGED)
    zero = _launch(dev, tables, max_rounds=0)
    one = {k: v.cpu().tolist() for k, v in ops.descend_ragged(*_operands(dev, tables)).items()}
    for k in ("best_fitness", "start_fitness", "best_pos", "best_rows", "sweeps", "moves"):
        assert zero[k] == one[k], k
    assert zero["round_history"] == [[f] for f in one["best_fitness"]]
    assert not any(zero["rounds"]) and not any(zero["pair_moves"]) and not any(zero["converged"])
    _assert_equal(zero, tables, _want(RAGGED, 16, 0))


def test_pair_descend_cut_off(dev):
    key = _key(7)
    p = next(i for i, w in enumerate(_want(key)) if w["rounds"] >= 3)
    tab, full = _tables(*key)[p], _want(key)[p]
    one = _launch(dev, [tab], max_rounds=1)
    _assert_equal(one, [tab], [pref.descend_pairs(*tab, max_rounds=1)])
    assert one["converged"] == [0] and one["rounds"] == [1] and one["round_history"] == [[full["round_history"][0]]]
    two = _launch(dev, [tab], max_rounds=2)
    _assert_equal(two, [tab], [pref.descend_pairs(*tab, max_rounds=2)])
    assert two["round_history"] == [full["round_history"][:2]] and two["converged"] == [0]
    whole = _launch(dev, [tab], max_rounds=6)
    n = full["rounds"]
    assert whole["rounds"] == [n] and whole["round_history"][0][n - 1:] == [full["best_fitness"]] * (7 - n)      # the tail repeats
    # max_sweeps = 0: pair sweeps only (the pair neighbourhood holds every single swap, but nothing settles a one-swap phase)
    tables = _tables(*key)
    pairs_only = _launch(dev, tables, max_sweeps=0)
    want = [pref.descend_pairs(*t, max_sweeps=0) for t in tables]
    _assert_equal(pairs_only, tables, want)
    assert not any(pairs_only["sweeps"]) and not any(pairs_only["moves"]) and not any(pairs_only["converged"]) and any(pairs_only["pair_moves"])
    # one sweep per phase
    _assert_equal(_launch(dev, tables, max_sweeps=1), tables, [pref.descend_pairs(*t, max_sweeps=1) for t in tables])


# ---- 5. a problem the launch was not sized for ------------------------------------------------------------------------------------------

def test_pair_descend_not_searched(dev):
    """The C entry itself, over buffers filled with a sentinel: a batch sized max_slots = 64 whose prob_ptr gives one problem 65 slots.
    That row is NaN / -1 / 0 with every round_history entry written, its best_pos / best_rows rows untouched; the neighbours are right."""
    from gnnpn_sc_amd import ops
    small, big, mid = _tables(*_key(7))[2], _tables(465, (65,), 2)[0], _tables(*_key(33))[0]
    tables = [small, big, mid]
    assert [len(t[0]) for t in tables] == [7, 65, 33]
    max_cand = max(sum(len(c) for c in t[0]) for t in (small, mid))
    with pytest.raises(ops.GnnpnError, match="gnnpn_descend_ragged_f64"):
        ops.descend_pairs_ragged(*_operands(dev, tables))                  # sized by the batch itself: 65 slots, refused
    for max_rounds, ld in ((0, 1), (3, 3)):
        got = _call_entry(dev, "gnnpn_descend_pairs_ragged_f64", tables, 64, max_cand, 16, max_rounds)
        want = [pref.descend_pairs(*t, max_rounds=max_rounds) for t in (small, mid)]
        _assert_equal({k: [v[0], v[2]] for k, v in got.items()}, [small, mid], want)
        assert np.isnan(got["best_fitness"][1]) and np.isnan(got["start_fitness"][1]) and all(np.isnan(h) for h in got["round_history"][1])
        assert len(got["round_history"][1]) == ld
        assert (got["sweeps"][1], got["moves"][1], got["rounds"][1], got["pair_moves"][1], got["converged"][1]) == (-1, 0, -1, 0, 0)
        assert set(got["best_pos"][1]) == {-7} and set(np.asarray(got["best_rows"][1]).ravel()) == {-7.0}
        assert -7.0 not in [h for row in got["round_history"] for h in row]
        assert got["best_pos"][0][7:] == [-7] * 57                         # nothing past a problem's count is written


# ---- 6. through the layers: descend_pairs, descend_starts_pairs, refine(pair_rounds=r), the CLI ----------------------------------------

def _list(res):
    return {k: v.cpu().tolist() for k, v in res.items()}


def _host_want(host, max_sweeps, max_rounds):
    return [pref.descend_pairs(cats, bounds, start, max_sweeps=max_sweeps, max_rounds=max_rounds) for cats, _len0, start, bounds in host]


def test_pipeline_descend_pairs_after_run(dev, chain):      # noqa: F811
    pipe, host, mins = chain["pipe"], chain["host"], chain["mins"]
    assert not any(isinstance(h, Exception) for h in host)
    res = pipe.descend_pairs(chain["svc"], chain["batch"], chain["out"], min_cost=mins[N_TRAIN:])
    got = _list(res)
    tables = [(cats, bounds, start) for cats, _l, start, bounds in host]
    want = _host_want(host, 16, 4)
    _assert_equal(got, tables, want)
    assert got["n_slots"] == [len(cats) for cats, _b, _s in tables]
    assert got["quality"] == [mins[N_TRAIN + b] / w["best_fitness"] for b, w in enumerate(want)]
    print("descend_pairs on the driver fixture: pair_moves", got["pair_moves"], "rounds", got["rounds"])
    from gnnpn_sc_amd.pipeline import descend_pairs
    again = descend_pairs(chain["svc"], chain["batch"], chain["out"], max_sweeps=16, max_rounds=4)
    assert all(torch.equal(again[k], res[k]) for k in again)


def _replicas(ds, actions, R):
    """[n, R, T, 8] float64: replica 0 = ``actions``; in replicas >= 1 every pick is a random member of its category; the last
    replica of R >= 3 repeats replica 1 (a tie between two replicas)."""
    g = np.random.default_rng(43)
    sf = ds["serviceFeature"]
    n, T = actions.shape[:2]
    out = np.repeat(actions[:, None], R, axis=1).copy()
    for r in range(1, R):
        for b in range(n):
            for c in range(T):
                if sum(out[b, r, c, :4].tolist()) != 3:                       # the host's test for a dummy row
                    members = sf[str(c + 1)]
                    out[b, r, c, :4] = members[int(g.integers(0, len(members)))]
    if R >= 3:
        out[:, R - 1] = out[:, 1]
    return out


@pytest.mark.parametrize("R", [1, 3])
def test_pipeline_descend_starts_pairs(dev, chain, monkeypatch, R):      # noqa: F811
    from gnnpn_sc_amd.pipeline import descend_starts, descend_starts_pairs
    from test_gpu_refine import _host_tables
    pipe, svc, batch, mins = chain["pipe"], chain["svc"], chain["batch"], chain["mins"]
    monkeypatch.chdir(chain["tmp"])
    B = P_ - N_TRAIN
    seen = _replicas(chain["ds"], chain["out"]["actions"].double().cpu().numpy(), R)
    starts = torch.from_numpy(seen).to(dev)
    host = [_host_tables("QWS", seen[:, r], 0)[0] for r in range(R)]
    assert not any(isinstance(h, Exception) for hr in host for h in hr)
    res = pipe.descend_starts_pairs(svc, batch, starts, pair_rounds=2, min_cost=mins[N_TRAIN:])
    got = _list(res)
    for b in range(B):
        runs = [pref.descend_pairs(host[r][b][0], host[r][b][3], host[r][b][2], max_sweeps=16, max_rounds=2) for r in range(R)]
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
    assert "history" not in res and res["round_history"].shape == (B, 2) and res["rounds"].dtype == torch.int32
    assert torch.equal(res["actions"], starts[torch.arange(B, device=dev), res["start_index"].long()])
    # pair_rounds = 0: today's call, key for key
    zero, today = descend_starts_pairs(svc, batch, starts, pair_rounds=0), descend_starts(svc, batch, starts)
    assert set(zero) == set(today) and all(torch.equal(zero[k], today[k]) for k in today)


def test_refine_from_the_pair_descended_composition(dev, chain):      # noqa: F811
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd.pipeline import refine
    svc, batch, out, host = chain["svc"], chain["batch"], chain["out"], chain["host"]
    B = P_ - N_TRAIN
    seeds = torch.tensor([77 + i for i in range(B)], dtype=torch.int64, device=dev)
    res = refine(svc, batch, out, 10, 12, seeds=seeds, descend=4, pair_rounds=2)
    tabs = ops.woa_candidates(svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds, out["actions"])
    want = _host_want(host, 4, 2)
    tables = [(cats, bounds, start) for cats, _l, start, bounds in host]
    _assert_equal(_list(res["descent"]), tables, want)
    start_pos = torch.tensor([x for w in want for x in w["best_pos"]], dtype=torch.int32, device=dev)
    fit, _pos, hist, draws, rows = ops.eswoa_ragged(tabs["prob_ptr"], tabs["cand_ptr"], tabs["len_init"], tabs["cand"], tabs["bounds"],
                                                    start_pos, 10, 12, seeds, max_slots=tabs["max_slots"], max_cand=tabs["max_cand"])
    assert res["best_fitness"].cpu().tolist() == fit.cpu().tolist() and res["history"].cpu().tolist() == hist.cpu().tolist()
    assert res["draws"].cpu().tolist() == draws.cpu().tolist() and res["best_rows"].cpu().tolist() == rows.cpu().tolist()
    assert all(r <= d for r, d in zip(res["best_fitness"].cpu().tolist(), res["descent"]["best_fitness"].cpu().tolist()))
    today = refine(svc, batch, out, 10, 12, seeds=seeds, descend=4)                 # pair_rounds = 0: today's path
    assert "rounds" not in today["descent"] and "history" in today["descent"]
    zero = refine(svc, batch, out, 10, 12, seeds=seeds, descend=4, pair_rounds=0)
    assert all(torch.equal(zero[k], today[k]) for k in today if k != "descent")
    assert all(torch.equal(zero["descent"][k], today["descent"][k]) for k in today["descent"])


def test_main_cli_infer_descend_pairs(dev, chain, monkeypatch):      # noqa: F811
    from test_gpu_refine import _actions_array, _host_tables
    tmp = chain["tmp"]
    monkeypatch.chdir(tmp)
    _write_cli_ini(tmp)
    import main as cli
    base = ["main.py", "QWS", "ML+2PN", "-1", "--infer", "--random-init", "--descend=4"]

    def run(*extra):
        with contextlib.redirect_stdout(io.StringIO()):
            assert cli.main(base + list(extra)) == 0

    def read(name, raw=False):
        with open(f"./solutions/WOA/QWS/ML+2PN+{name}.txt") as f:
            return f.read() if raw else json.load(f)
    import os
    for name in ("pairs", "multistart+pairs"):
        with contextlib.suppress(FileNotFoundError):
            os.remove(f"./solutions/WOA/QWS/ML+2PN+{name}.txt")
    run()                                                              # the parent's flags: the descent artefact, nothing new
    descent_text = read("descent", raw=True)
    descent = json.loads(descent_text)
    assert list(descent) == ["quality", "time", "averageQ", "averageT"] and not os.path.exists("./solutions/WOA/QWS/ML+2PN+pairs.txt")
    with open("./solutions/pretrained/QWS-PNHigh.txt") as f:
        actions = _actions_array(json.load(f))
    host, _sols, mins = _host_tables("QWS", actions, 0)
    assert not any(isinstance(h, Exception) for h in host)
    one_swap = [ref.descend(cats, bounds, start, max_sweeps=4) for cats, _l, start, bounds in host]
    assert descent["quality"] == [mins[N_TRAIN + b] / w["best_fitness"] for b, w in enumerate(one_swap)]      # what the parent writes
    run("--pairs")                                                     # four rounds unless given
    pairs = read("pairs")
    want = _host_want(host, 4, 4)
    n = P_ - N_TRAIN
    assert list(pairs) == ["quality", "time", "averageQ", "averageT", "rounds", "pair_moves", "converged"]
    assert pairs["quality"] == [mins[N_TRAIN + b] / w["best_fitness"] for b, w in enumerate(want)]
    assert len(pairs["quality"]) == n and pairs["averageQ"] == sum(pairs["quality"]) / n
    for k in ("rounds", "pair_moves", "converged"):
        assert pairs[k] == [w[k] for w in want], k
    assert read("descent", raw=True) == descent_text                   # pairs.txt takes its place: descent.txt is not rewritten
    assert all(a >= b > 0 for a, b in zip(pairs["quality"], descent["quality"]))
    run("--pairs=1", "--woa", "--seed", "3")                           # ES-WOA starts from the pair-descended composition
    cut = read("pairs")
    want1 = _host_want(host, 4, 1)
    assert cut["quality"] == [mins[N_TRAIN + b] / w["best_fitness"] for b, w in enumerate(want1)]
    assert cut["rounds"] == [1] * n and cut["converged"] == [w["converged"] for w in want1]
    assert all(r >= a for r, a in zip(read("WOA")["quality"], cut["quality"]))
    run("--pairs=2", "--samples=3", "--all-starts", "--seed", "3")
    multi = read("multistart+pairs")
    assert list(multi) == list(pairs) and len(multi["quality"]) == n and all(q > 0 for q in multi["quality"])
    assert all(c in (0, 1) for c in multi["converged"]) and all(1 <= r <= 2 for r in multi["rounds"])
