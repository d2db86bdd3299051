"""-m gpu: which services a searched composition consists of, and the merit of a composition given as ids —
gnnpn_woa_candidates_services (and its replica form), gnnpn_search_services, gnnpn_services_merit_f64 in its two forms,
ops.woa_candidates_named / SearchTables.services / services_merit, pipeline.name_services / score_services and
`main.py ... --infer --descend --services` — against tests/services_reference.py (the host path over indices), ``==`` throughout.
tests/test_services_host.py holds the reference against the host path and the conditions on the batches used here."""
import contextlib
import io
import json
import math

import numpy as np
import pytest
import torch

import candidate_tables_reference as ctr
import services_reference as sref
from kernel_checks import twice
from test_candidate_tables_host import PICK_SEED
from test_gpu_candidate_tables import _world
from test_gpu_descend import K_, N_TRAIN, P_, T_, H_, chain  # noqa: F401  (chain: the small pipeline fixture)

pytestmark = pytest.mark.gpu

TABLE_KEYS = ("prob_ptr", "n_slots", "cand_ptr", "len_init", "cand", "start_pos", "bounds", "status")
BUILDER_SEED, BUILDER_COUNTS = 9, ctr.SEARCH_COUNTS + (1, 64, 128, 129)      # the seed: the problem of one task node keeps its list


def _t(a, dev, dt=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)


@pytest.fixture(scope="module")
def world(dev, tmp_path_factory):
    """The search problems (3 .. 200 task nodes) and those of 1, 64, 128 and 129, the all-infeasible ones in the batch's middle."""
    return _world(dev, tmp_path_factory, "services_builder", ctr.make_dataset(BUILDER_SEED, BUILDER_COUNTS, ctr.ALL_INFEASIBLE))


@pytest.fixture(scope="module")
def named(dev, tmp_path_factory):
    """The named batch (a failed problem between good ones, every other one seeded, every foreign row a service with an id, the
    twin services), its device tables with ids and the reference's."""
    from gnnpn_sc_amd import ops
    ds, _cat, twin = sref.named_dataset()
    w = _world(dev, tmp_path_factory, "services_named", ds)
    w["acts"], w["ids"] = sref.named_picks(ds, twin=twin)
    w["twin"] = twin
    w["a"], w["aid"] = _t(w["acts"], dev, torch.float64), _t(w["ids"], dev)
    w["tabs"] = twice(lambda: ops.woa_candidates_named(*w["operands"], w["a"], check_status=False, action_ids=w["aid"]))
    w["ref"] = sref.named_tables(ds, w["acts"], 0, action_ids=w["ids"])
    w["ref_bare"] = sref.named_tables(ds, w["acts"], 0)
    w["rows"] = sref.service_rows(ds)[0]
    w["n_nodes"] = [len(p) for p in ctr.problems_of(ds)]
    return w


def _assert_names(tabs, want):
    node, cat, cand = sref.flat(want)
    assert tabs["slot_node"].cpu().tolist() == node
    assert tabs["slot_cat"].cpu().tolist() == cat
    assert tabs["cand_service"].cpu().tolist() == cand
    assert tabs["status"].cpu().tolist().count(0) == sum(t is not None for t in want)
    assert [int(s != 0) for s in tabs["status"].cpu().tolist()] == [int(t is None) for t in want]


def _assert_same_tables(named_tabs, plain):
    for k in TABLE_KEYS:
        a, b = named_tabs[k], plain[k]
        if a.dtype == torch.float64:
            a, b = a.view(torch.int64), b.view(torch.int64)
        assert torch.equal(a, b), k
    assert (named_tabs["max_slots"], named_tabs["max_cand"]) == (plain["max_slots"], plain["max_cand"])


# ---- 1. the builder's ids ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_ids", [False, True], ids=["no_ids", "ids"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("reduct", [0, 0.55])
def test_builder_ids_equal_reference(world, reduct, dtype, with_ids):
    """Problems of 1 .. 200 task nodes (one to four passes of the slot loop, empty lists between kept ones), 200 action rows (four
    passes of the row compaction), failed problems in the batch's middle: slot_node, slot_cat and cand_service against the host
    path over indices; the four tables of the named call are woa_candidates' bit for bit."""
    from gnnpn_sc_amd import ops
    dev = world["dev"]
    acts = ctr.make_picks(world["ds"], reduct, 200, PICK_SEED, mismatch=False)
    a = _t(acts, dev, dtype)
    seen = a.double().cpu().numpy()
    ids = np.random.default_rng(5).integers(0, ctr.N_SERVICES, acts.shape[:2]).astype(np.int32) if with_ids else None
    tabs = twice(lambda: ops.woa_candidates_named(*world["operands"], a, reduct=reduct, check_status=False,
                                                  action_ids=None if ids is None else _t(ids, dev)))
    _assert_same_tables(tabs, ops.woa_candidates(*world["operands"], a, reduct=reduct, check_status=False))
    want = sref.named_tables(world["ds"], seen, reduct, action_ids=ids)
    _assert_names(tabs, want)
    sizes = [len(t["slot_node"]) for t in want if t is not None]
    assert None in want[1:-1] and max(sizes) > 128 and min(sizes) == 1 and any(64 < n <= 128 for n in sizes)
    bare = want if ids is None else sref.named_tables(world["ds"], seen, reduct)
    appended = sum(k.count(-1) for t in bare if t for k in t["cand_service"])
    assert any(not t["seeded"] for t in want if t) and appended > 0                     # unseeded problems; appended foreign rows
    if not with_ids:
        assert (tabs["cand_service"] >= -1).all() and (tabs["cand_service"] == -1).any()


def test_builder_ids_with_patches(world):
    """A patch moves a picked member out of its list (its appended row carries the pick's id) and a foreign row into it."""
    from gnnpn_sc_amd import ops
    from test_gpu_candidate_tables import NO_MATCH
    dev, ds = world["dev"], world["ds"]
    acts = ctr.make_picks(ds, 0, 200, PICK_SEED, mismatch=False)
    plain = sref.named_tables(ds, acts, 0)
    b = max(range(len(plain)), key=lambda i: len(plain[i]["slot_node"]) if plain[i] and plain[i]["seeded"] else 0)
    j = max(j for j, (s, k) in enumerate(zip(plain[b]["start"], plain[b]["cand_service"])) if s < len(k) and k[-1] != -1)
    assert j >= 64
    patches = [NO_MATCH, (tuple(ctr.rounded(acts[b, j])), 0, 0.98765)]
    ids = np.arange(acts.shape[0] * acts.shape[1], dtype=np.int32).reshape(acts.shape[:2]) % ctr.N_SERVICES
    want = sref.named_tables(ds, acts, 0, patches, action_ids=ids)
    assert len(want[b]["cand_service"][j]) == len(plain[b]["cand_service"][j]) + 1 and want[b]["cand_service"][j][-1] == ids[b, j]
    tabs = twice(lambda: ops.woa_candidates_named(*world["operands"], _t(acts, dev, torch.float64), patches=patches, check_status=False,
                                                  action_ids=_t(ids, dev)))
    _assert_same_tables(tabs, ops.woa_candidates(*world["operands"], _t(acts, dev, torch.float64), patches=patches, check_status=False))
    _assert_names(tabs, want)


def test_builder_ids_of_replicas(world):
    """R = 3, every replica with picks and ids of its own: row b * R + r holds what the per-problem call gives for actions_all[:, r] —
    the batch is read by indirection."""
    from gnnpn_sc_amd import ops
    dev, ds, R, reduct = world["dev"], world["ds"], 3, 0.55
    acts_all = np.stack([ctr.make_picks(ds, reduct, 200, PICK_SEED + r, mismatch=r == 1) for r in range(R)], 1)
    ids_all = np.random.default_rng(6).integers(0, ctr.N_SERVICES, acts_all.shape[:3]).astype(np.int32)
    a = _t(acts_all, dev, torch.float64)
    tabs = twice(lambda: ops.woa_candidates_replicas_named(*world["operands"], a, reduct=reduct, check_status=False, action_ids=_t(ids_all, dev)))
    _assert_same_tables(tabs, ops.woa_candidates_replicas(*world["operands"], a, reduct=reduct, check_status=False))
    assert tabs["replicas"] == R
    per = [sref.named_tables(ds, acts_all[:, r], reduct, action_ids=ids_all[:, r]) for r in range(R)]
    assert per[0] != per[1] != per[2]
    _assert_names(tabs, [per[q % R][q // R] for q in range(acts_all.shape[0] * R)])
    with pytest.raises(ops.GnnpnError, match="action_ids"):
        ops.woa_candidates_replicas_named(*world["operands"], a, reduct=reduct, check_status=False, action_ids=_t(ids_all[:, 0], dev))


# ---- 2. from positions to services ------------------------------------------------------------------------------------------------------------

def _assert_mapping(w, got, res, ref_tabs, ld=None):
    """best_services / node_services against the reference's mapping of the device's own positions."""
    fit, pos = res["best_fitness"].cpu().tolist(), res["best_pos"].cpu().tolist()
    best, nodes = got["best_services"].cpu().tolist(), got["node_services"].cpu().tolist()
    seg = w["batch"].seg_ptr.cpu().tolist()
    assert len(nodes) == w["batch"].x.shape[0] == seg[-1]
    for b, tab in enumerate(ref_tabs):
        want_best, want_nodes = sref.map_services(tab, fit[b], pos[b], w["n_nodes"][b], len(pos[b]))
        assert best[b] == want_best, b
        assert nodes[seg[b]:seg[b + 1]] == want_nodes, b
    return fit, pos, best, nodes


def _assert_promise(w, res, best, seeded=True):
    """An id s >= 0: row s of the table, rounded where the tables were seeded, is best_rows there.  Returns the number of ids."""
    rows = res["best_rows"].cpu().tolist()
    n = 0
    for b, ids in enumerate(best):
        for l, s in enumerate(ids):
            if s >= 0:
                want = tuple(round(v, 5) for v in w["rows"][s]) if seeded else w["rows"][s]
                assert tuple(rows[b][l]) == want, (b, l, s)
                n += 1
    return n


@pytest.mark.parametrize("wide", [None, True], ids=["lane", "workgroup"])
def test_mapping_after_descend(named, wide):
    """Lane form: the launch is sized for 64 slots, the larger problems are not searched (NaN) and yield -1 throughout, as the
    failed one does.  Workgroup form: the whole batch."""
    from gnnpn_sc_amd import ops
    tabs, seg, N = named["tabs"], named["batch"].seg_ptr, named["batch"].x.shape[0]
    if wide:
        res = tabs.descend(wide=True)
    else:
        small = [sum(len(k) for k in t["cand_service"]) for t in named["ref"] if t is not None and len(t["slot_node"]) <= 64]
        res = ops.descend_ragged(tabs["prob_ptr"], tabs["cand_ptr"], tabs["cand"], tabs["bounds"], tabs["start_pos"], max_slots=64,
                                 max_cand=max(small))
    got = twice(lambda: tabs.services(res, seg, N))
    fit, _pos, best, nodes = _assert_mapping(named, got, res, named["ref"])
    searched = [b for b, f in enumerate(fit) if f == f]
    skipped = [b for b, t in enumerate(named["ref"]) if t is not None and b not in searched]
    assert searched and bool(skipped) == (not wide) and all(len(named["ref"][b]["slot_node"]) > 64 for b in skipped)
    assert all(set(best[b]) == {-1} for b in range(len(fit)) if b not in searched)
    assert _assert_promise(named, res, best) == sum(len(named["ref"][b]["slot_node"]) for b in searched)
    assert got["best_services"].shape == res["best_pos"].shape and min(nodes) == -1


def test_mapping_after_pair_shortlist_at_130_slots(named):
    tabs = named["tabs"]
    res = tabs.descend_pairs_shortlist(max_sweeps=4, max_rounds=1, max_span=2, max_rank=2)
    got = tabs.services(res, named["batch"].seg_ptr, named["batch"].x.shape[0])
    fit, _pos, best, _nodes = _assert_mapping(named, got, res, named["ref"])
    assert any(len(t["slot_node"]) > 128 and fit[b] == fit[b] for b, t in enumerate(named["ref"]) if t)
    assert _assert_promise(named, res, best) > 300 and res["pair_moves"].sum().item() >= 0


def test_mapping_of_the_winner_of_three_starts(named):
    """descend_starts' stages over R = 3 named replica tables: every problem reads the tables of its winner's row."""
    from gnnpn_sc_amd import ops
    dev, ds, R = named["dev"], named["ds"], 3
    more = [sref.named_picks(ds, seed=sref.NAMED_PICK_SEED + r, foreign=0.3) for r in range(1, R)]
    acts_all = np.stack([named["acts"]] + [m[0] for m in more], 1)
    ids_all = np.stack([named["ids"]] + [m[1] for m in more], 1)
    a = _t(acts_all, dev, torch.float64)
    tabs = ops.woa_candidates_replicas_named(*named["operands"], a, check_status=False, action_ids=_t(ids_all, dev))
    per_row = tabs.descend()
    sel = ops.descend_select(per_row, a, tabs["n_slots"])
    got = twice(lambda: tabs.services(sel, named["batch"].seg_ptr, named["batch"].x.shape[0], start_index=sel["start_index"]))
    win = sel["start_index"].cpu().tolist()
    assert len(set(win)) > 1
    per = [sref.named_tables(ds, acts_all[:, r], 0, action_ids=ids_all[:, r]) for r in range(R)]
    _fit, _pos, best, nodes = _assert_mapping(named, got, sel, [per[win[b]][b] for b in range(len(win))])
    assert _assert_promise(named, sel, best) > 300
    # without start_index replica 0's tables are read: a different answer wherever another replica won with other rows
    zero = tabs.services({**sel, "best_pos": per_row["best_pos"][::R].contiguous(), "best_fitness": per_row["best_fitness"][::R].contiguous()},
                         named["batch"].seg_ptr, named["batch"].x.shape[0])
    _assert_mapping(named, zero, {"best_fitness": per_row["best_fitness"][::R], "best_pos": per_row["best_pos"][::R]}, per[0])
    # the winner's services score the winner's merit
    merit, n_rows = ops.services_merit(named["batch"].seg_ptr, got["node_services"], named["svc"].qos, named["batch"].global_bounds, True)
    fit = sel["best_fitness"].cpu().tolist()
    assert [m for m, f in zip(merit.cpu().tolist(), fit) if f == f] == [f for f in fit if f == f]


def test_mapping_after_refine_and_of_python_positions(named):
    """refine returns ES-WOA's positions, negative ones from the end of the list; a hand-made best_pos with the same positions
    Python's way names the same services, one past its list names -1."""
    from gnnpn_sc_amd import ops
    from gnnpn_sc_amd import pipeline as pl
    dev, svc, batch = named["dev"], named["svc"], named["batch"]
    good = [b for b, t in enumerate(named["ref"]) if t is not None]
    # refine raises on a failed problem: the good problems of the batch through the tables' own ES-WOA, the failed one stays NaN
    tabs = named["tabs"]
    seeds = torch.arange(len(named["ref"]), dtype=torch.int64, device=dev) + 91
    fit, pos, _hist, _draws, rows = tabs.eswoa(6, 5, seeds)
    res = {"best_fitness": fit, "best_pos": pos, "best_rows": rows}
    got = tabs.services(res, batch.seg_ptr, batch.x.shape[0])
    _fit, posl, best, _nodes = _assert_mapping(named, got, res, named["ref"])
    assert _assert_promise(named, res, best) > 300
    lens = [[len(k) for k in t["cand_service"]] if t else [] for t in named["ref"]]
    hand = [list(p) for p in posl]
    for b in good:
        hand[b][:len(lens[b])] = [(p % n) - n if l % 2 else p % n for l, (p, n) in enumerate(zip(posl[b], lens[b]))]
    res2 = {"best_fitness": fit, "best_pos": _t(np.asarray(hand, dtype=np.int32), dev)}
    got2 = tabs.services(res2, batch.seg_ptr, batch.x.shape[0])
    assert min(min(h) for h in hand) < 0 and torch.equal(got2["best_services"], got["best_services"])
    assert torch.equal(got2["node_services"], got["node_services"])
    b, l = max(good, key=lambda i: len(lens[i])), 1
    other = next(i for i in good if i != b)
    hand[b][l], hand[other][0] = lens[b][l], -lens[other][0] - 1                        # one past the end; one before the start
    res3 = {"best_fitness": fit, "best_pos": _t(np.asarray(hand, dtype=np.int32), dev)}
    got3 = tabs.services(res3, batch.seg_ptr, batch.x.shape[0])
    _assert_mapping(named, got3, res3, named["ref"])
    assert got3["best_services"][b, l].item() == -1 and got3["best_services"][other, 0].item() == -1
    assert (got3["best_services"] != got["best_services"]).sum().item() == 2
    # pipeline.refine itself, over the good problems after the failed one (a batch of its own would need its own data set)
    with pytest.raises(ops.GnnpnError, match="problem"):
        pl.refine(svc, batch, {"actions": named["a"]}, 6, 5, seeds=seeds)


def test_promise_without_action_ids(named):
    """Without action_ids the foreign rows that survive the descent are -1 and nothing else is; with them every slot has an id."""
    from gnnpn_sc_amd import ops
    tabs = named["tabs"]
    bare = ops.woa_candidates_named(*named["operands"], named["a"], check_status=False)
    _assert_names(bare, named["ref_bare"])
    res = tabs.descend()
    seg, N = named["batch"].seg_ptr, named["batch"].x.shape[0]
    with_ids, without = tabs.services(res, seg, N), bare.services(res, seg, N)
    _assert_mapping(named, without, res, named["ref_bare"])
    pos, len_init = res["best_pos"].cpu().tolist(), tabs["len_init"].cpu().tolist()
    prob_ptr, best = tabs["prob_ptr"].cpu().tolist(), without["best_services"].cpu().tolist()
    full = with_ids["best_services"].cpu().tolist()
    foreign = 0
    for b, t in enumerate(named["ref"]):
        for l in range(len(t["slot_node"]) if t else 0):
            kept = pos[b][l] < len_init[prob_ptr[b] + l]
            assert (best[b][l] >= 0) == kept and full[b][l] >= 0 and (not kept or best[b][l] == full[b][l]), (b, l)
            foreign += not kept
    assert foreign > 0
    # the twin services: a pick of the second names the first kept one wherever descent left the start
    first, twin = named["twin"]
    start = tabs["start_pos"].cpu().tolist()
    stayed = [full[b][l] for b, t in enumerate(named["ref"]) if t for l, k in enumerate(t["cand_service"])
              if first in k and twin in k and pos[b][l] == start[prob_ptr[b] + l]]
    assert stayed and set(stayed) == {first}


def test_promise_on_unseeded_tables(world):
    """A problem without action rows keeps its lists unrounded: its ids name best_rows bit for bit, and score best_fitness with
    rounded = 0."""
    from gnnpn_sc_amd import ops
    dev, ds = world["dev"], world["ds"]
    acts = np.zeros((len(ctr.problems_of(ds)), 4, 8))
    acts[:, :, 1:4] = 1.0                                                               # dummy rows only: no seed anywhere
    tabs = ops.woa_candidates_named(*world["operands"], _t(acts, dev, torch.float64), check_status=False)
    want = sref.named_tables(ds, acts, 0)
    _assert_names(tabs, want)
    assert not any(t["seeded"] for t in want if t) and None in want
    res = tabs.descend()
    w = dict(world, rows=sref.service_rows(ds)[0], n_nodes=[len(p) for p in ctr.problems_of(ds)])
    got = tabs.services(res, world["batch"].seg_ptr, world["batch"].x.shape[0])
    fit, _pos, best, _nodes = _assert_mapping(w, got, res, want)
    assert _assert_promise(w, res, best, seeded=False) == sum(len(t["slot_node"]) for t in want if t)
    merit, n_rows = ops.services_merit(world["batch"].seg_ptr, got["node_services"], world["svc"].qos, world["batch"].global_bounds, False)
    merit, n_rows = merit.cpu().tolist(), n_rows.cpu().tolist()
    for b, t in enumerate(want):
        if t is None:
            assert fit[b] != fit[b] and merit[b] != merit[b] and n_rows[b] == 0, b
        else:
            assert merit[b] == fit[b] and n_rows[b] == len(t["slot_node"]), b


# ---- 3. the scorer -------------------------------------------------------------------------------------------------------------------------------

ROW_COUNTS = (1, 7, 8, 9, 63, 64, 65, 128, 129, 200)


def _compositions(dev, seed=17, n_services=300):
    """One problem per row count plus one of 40 rows over 150 nodes (the node loop compacts across its passes): random ids between
    nodes without a service, a random table, bounds that the products meet, miss on one side or on both."""
    g = np.random.default_rng(seed)
    qos = np.c_[g.random((n_services, 2)), 0.99 + 0.01 * g.random((n_services, 2))]
    seg, ids, bounds = [0], [], []
    for k, n in enumerate(ROW_COUNTS + (40,)):
        n_nodes = 150 if n == 40 else n + 1 + int(g.integers(0, 5))
        nodes = np.full(n_nodes, -1)
        nodes[np.sort(g.choice(np.arange(1, n_nodes), n, replace=False))] = g.integers(0, n_services, n)
        ids += nodes.tolist()
        seg.append(len(ids))
        p2, p3 = np.prod(qos[nodes[nodes >= 0], 2]), np.prod(qos[nodes[nodes >= 0], 3])
        bounds.append([(0.0, 1.0, 0.0, 1.0), (p2 * 1.01, 1.0, 0.0, 1.0), (0.0, p2 * 0.99, p3 * 1.01, 1.0)][k % 3])
    return {"qos": qos, "seg": seg, "ids": ids, "bounds": bounds,
            "dev": (_t(np.asarray(seg, dtype=np.int32), dev), _t(np.asarray(ids, dtype=np.int32), dev), _t(qos, dev, torch.float64),
                    _t(np.asarray(bounds), dev, torch.float64))}


@pytest.mark.parametrize("rounded", [0, 1])
@pytest.mark.parametrize("wide", [None, True], ids=["lane", "workgroup"])
def test_scorer_equals_reference(dev, wide, rounded):
    """1 .. 200 rows: 7 / 8 / 9 straddle numpy's switch to eight accumulators, 64 fills the wave, 129 and 200 take np.sum's recursion.
    Lane form: sized for 64 rows, the larger problems are not scored (NaN, -1).  The workgroup form at 64 rows gives the lane form's bits."""
    from gnnpn_sc_amd import ops
    c = _compositions(dev)
    merit, n_rows = twice(lambda: ops.services_merit(*c["dev"], rounded, max_slots=None if wide else 64, wide=wide))
    merit, n_rows = merit.cpu().tolist(), n_rows.cpu().tolist()
    rows = [tuple(r) for r in c["qos"].tolist()]
    violated = set()
    for b, bd in enumerate(c["bounds"]):
        ids = c["ids"][c["seg"][b]:c["seg"][b + 1]]
        want, n = sref.score(rows, ids, list(bd), rounded)
        if not wide and n > 64:
            assert merit[b] != merit[b] and n_rows[b] == -1, b
        else:
            assert merit[b] == want and n_rows[b] == n, (b, n, merit[b], want)
            violated.add(int(want))
    assert violated == {0, 1, 2}
    if wide:
        lane, _n = ops.services_merit(*c["dev"], rounded, max_slots=64)
        assert [a for a, n in zip(lane.cpu().tolist(), n_rows) if n <= 64] == [m for m, n in zip(merit, n_rows) if n <= 64]


@pytest.mark.parametrize("wide", [None, True], ids=["lane", "workgroup"])
def test_scorer_refusals(dev, wide):
    """An id of n_services, an id below -1, no rows, more rows than max_slots: NaN each, n_rows 0 for no rows alone; the
    neighbours are scored."""
    from gnnpn_sc_amd import ops
    g = np.random.default_rng(3)
    qos = np.c_[g.random((20, 2)), 0.95 + 0.05 * g.random((20, 2))]
    ids = [[-1, 3, 4, 5], [-1, 3, 20, 5], [-1, -1, -1], [-1, 6, -2, 7], [-1, 1, 2, 3, 4, 5, 6], [], [-1, 19, 0]]
    seg = np.cumsum([0] + [len(i) for i in ids]).astype(np.int32)
    bounds = [[0.0, 1.0, 0.0, 1.0]] * len(ids)
    merit, n_rows = ops.services_merit(_t(seg, dev), _t(np.asarray(sum(ids, []), dtype=np.int32), dev), _t(qos, dev, torch.float64),
                                       _t(np.asarray(bounds), dev, torch.float64), 1, max_slots=5, wide=wide)
    merit, n_rows = merit.cpu().tolist(), n_rows.cpu().tolist()
    rows = [tuple(r) for r in qos.tolist()]
    assert n_rows == [3, -1, 0, -1, -1, 0, 2]
    for b in (0, 6):
        assert (merit[b], n_rows[b]) == sref.score(rows, ids[b], bounds[b])
    assert all(math.isnan(merit[b]) for b in (1, 2, 3, 4, 5))
    assert [sref.score(rows, ids[b], bounds[b])[1] for b in (1, 2, 3, 5)] == [-1, 0, -1, 0]


def test_certificate_scoring_the_named_services_gives_best_fitness(named):
    """With action_ids and no patches: score_services(node_services) == best_fitness, bit for bit, for every searched problem of
    the batch (compositions that keep a foreign row among them: test_services_host.py); the failed one has no rows."""
    from gnnpn_sc_amd import pipeline as pl
    tabs, svc, batch = named["tabs"], named["svc"], named["batch"]
    for res in (tabs.descend(), tabs.descend_pairs_shortlist(max_sweeps=4, max_rounds=1, max_span=2, max_rank=2)):
        got = tabs.services(res, batch.seg_ptr, batch.x.shape[0])
        merit, n_rows = twice(lambda: pl.score_services(svc, batch, got["node_services"]))
        merit, n_rows, fit = merit.cpu().tolist(), n_rows.cpu().tolist(), res["best_fitness"].cpu().tolist()
        pos, len_init, prob_ptr = res["best_pos"].cpu().tolist(), tabs["len_init"].cpu().tolist(), tabs["prob_ptr"].cpu().tolist()
        foreign = 0
        for b, t in enumerate(named["ref"]):
            if t is None:
                assert fit[b] != fit[b] and merit[b] != merit[b] and n_rows[b] == 0, b
                continue
            assert merit[b] == fit[b] and n_rows[b] == len(t["slot_node"]), (b, merit[b], fit[b])
            foreign += sum(pos[b][l] >= len_init[prob_ptr[b] + l] for l in range(len(t["slot_node"])))
        assert foreign > 0


# ---- 4. the pipeline and the command line --------------------------------------------------------------------------------------------------------

def _chain_reference(chain, actions):  # noqa: F811
    ds = chain["ds"]
    return sref.named_tables(ds, actions, 0), sref.service_rows(ds)[0], [len(p) for p in ctr.problems_of(ds)]


def test_name_services_on_a_run_result(dev, chain):  # noqa: F811
    """run() -> descend / descend_pairs / refine -> name_services: run's candidate_ids gathered by idx_high are rows of the service
    table (the float32 action rows are those rows), the ids are the reference's, and they score the stage's best_fitness."""
    from gnnpn_sc_amd import pipeline as pl
    pipe, svc, batch, out = chain["pipe"], chain["svc"], chain["batch"], chain["out"]
    assert not any(isinstance(h, Exception) for h in chain["host"])
    aid = pl.action_ids_of(out)
    assert aid.shape == out["actions"].shape[:2] and aid.dtype == torch.int32
    real = aid >= 0
    assert real.any() and torch.equal(svc.qos[aid[real].long()].float(), out["actions"][..., :4].float()[real])
    assert bool((out["actions"][..., :4].double().sum(-1)[~real] == 3).all())
    acts = out["actions"].double().cpu().numpy()
    ref_tabs, rows, n_nodes = _chain_reference(chain, acts)
    w = {"batch": batch, "rows": rows, "n_nodes": n_nodes}
    seeds = torch.arange(batch.n_problems, dtype=torch.int64, device=dev) + 5
    for res in (pipe.descend(svc, batch, out), pl.descend_pairs(svc, batch, out, max_rounds=2),
                pl.refine(svc, batch, out, 6, 5, seeds=seeds, descend=4)):
        got = twice(lambda: pipe.name_services(svc, batch, out, res))
        assert got["action_ids_used"] is True and set(res) < set(got)
        assert all(got[k] is res[k] for k in res)
        _fit, _pos, best, _nodes = _assert_mapping(w, got, res, ref_tabs)
        assert _assert_promise(w, res, best) == int(res["n_slots"].sum().item())
        merit, n_rows = pl.score_services(svc, batch, got["node_services"])
        assert merit.cpu().tolist() == res["best_fitness"].cpu().tolist() and torch.equal(n_rows, res["n_slots"])
    bare = pl.name_services(svc, batch, {"actions": out["actions"]}, res)
    assert bare["action_ids_used"] is False and torch.equal(bare["best_services"], got["best_services"])     # no foreign row here
    # a multi-start result: the tables of res["actions"], the winner's start rows, named by idx_all read at the winner
    starts = {"actions_all": torch.stack([out["actions"], out["actions"]], 1).contiguous(), "candidate_ids": out["candidate_ids"],
              "idx_all": torch.stack([out["idx_high"], out["idx_high"]], 1).contiguous()}
    multi = pl.descend_starts(svc, batch, starts)
    got = pl.name_services(svc, batch, starts, multi)
    assert got["action_ids_used"] is True and "start_index" in got
    _assert_mapping(w, got, multi, _chain_reference(chain, multi["actions"].double().cpu().numpy())[0])
    assert pl.name_services(svc, batch, starts["actions_all"], multi)["action_ids_used"] is False


def test_main_cli_services(dev, chain, monkeypatch):  # noqa: F811
    """--descend=4 --services: the descent artefact as without the flag, and ML+2PN+services.txt whose merits are the descent's.
    The descent artefact holds quality = minCost / best_fitness, one IEEE division; the merit is held to it in that direction —
    minCost / merit == quality, and merit == the file's own best_fitness, both to the last bit — because minCost / quality, the same
    identity turned round, is a second rounding and no identity in float64."""
    from test_gpu_refine import _actions_array
    tmp = chain["tmp"]
    monkeypatch.chdir(tmp)
    (tmp / "environment.ini").write_text(
        f"[QWS-PNHigh]\nembeddingTag = 0\nUSE_CUDA = 1\nserCategory = {T_}\nepochDiv = 1\nserNumber = {K_}\nhidden_size = {H_}\n"
        "n_glimpses = 0\ntanh_exploration = 10\nuse_tanh = 1\nbeta = 0.9\nmax_grad_norm = 2.\nlr = 0.5e-4\nepochML = -1\nepochPNLow = -1\n"
        f"[QWS-ML+2PN]\nserviceCategory = {T_}\nepoch = -1\n")
    import main as cli
    base = ["main.py", "QWS", "ML+2PN", "-1", "--infer", "--random-init", "--descend=4"]
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(base) == 0
    with open("./solutions/WOA/QWS/ML+2PN+descent.txt") as f:
        plain = json.load(f)
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(base + ["--services"]) == 0
    with open("./solutions/WOA/QWS/ML+2PN+descent.txt") as f:
        descent = json.load(f)
    with open("./solutions/WOA/QWS/ML+2PN+services.txt") as f:
        doc = json.load(f)
    with open("./solutions/pretrained/QWS-PNHigh.txt") as f:
        actions = _actions_array(json.load(f))
    assert descent["quality"] == plain["quality"] and set(descent) == set(plain)
    B = P_ - N_TRAIN
    mins = chain["mins"][N_TRAIN:]
    assert len(doc["merit"]) == len(doc["services"]) == B and doc["action_ids_used"] is True
    assert doc["merit"] == doc["best_fitness"]
    assert [mc / m for mc, m in zip(mins, doc["merit"])] == descent["quality"]
    off = [b for b in range(B) if mins[b] / descent["quality"][b] != doc["merit"][b]]
    print("minCost / quality != merit (a second rounding) in", len(off), "of", B, "problems")
    assert all(abs(mins[b] / descent["quality"][b] - doc["merit"][b]) <= 2 * math.ulp(doc["merit"][b]) for b in off)
    ref_tabs, rows, _n = _chain_reference(chain, actions)
    for b, (t, listed) in enumerate(zip(ref_tabs, doc["services"])):
        nodes = ctr.problems_of(chain["ds"])[b]
        assert [e[0] for e in listed] == list(range(1, len(nodes))), b
        assert [e[1] for e in listed] == [n[:-6].index(1) - 1 for n in nodes[1:]], b
        named_ids = {n: s for n, _c, s in listed if s >= 0}
        assert sorted(named_ids) == t["slot_node"] and doc["n_rows"][b] == len(t["slot_node"]), b
        assert all(s in t["cand_service"][t["slot_node"].index(n)] for n, s in named_ids.items()), b
        assert sref.score(rows, [-1] + [e[2] for e in listed], chain["host"][b][3]) == (doc["merit"][b], doc["n_rows"][b]), b
    # the other routes to the flag: descent from every best-of-N start, and ES-WOA behind the descent (the last stage is named)
    with open("environment.ini", "a") as f:
        f.write(f"[QWS-WOA]\nserCategory = {T_}\nMLESWOAtest = 0\nML2PNWOATest = 1\nMLWOATest = 0\nESWOAtest = 0\n"
                "serviceNumber = 4\nreduct = 0\nepoch = -1\nMAX_Iter = 5\npopSize = 6\n")
    for extra, artefact in ((["--samples=3", "--all-starts", "--seed", "3"], "ML+2PN+multistart.txt"),
                            (["--pairs=2", "--woa", "--seed", "3"], "ML+2PN+WOA.txt")):
        with contextlib.redirect_stdout(io.StringIO()):
            assert cli.main(base + extra + ["--services"]) == 0
        with open("./solutions/WOA/QWS/" + artefact) as f:
            stage = json.load(f)
        with open("./solutions/WOA/QWS/ML+2PN+services.txt") as f:
            doc = json.load(f)
        assert doc["action_ids_used"] is True and doc["merit"] == doc["best_fitness"] and len(doc["merit"]) == B, extra
        assert [mc / m for mc, m in zip(mins, doc["merit"])] == stage["quality"], extra
        assert [sum(s >= 0 for _n, _c, s in listed) for listed in doc["services"]] == doc["n_rows"], extra
