"""-m gpu: the candidate tables of gnnpn_woa_candidates_count / _fill (and their replica forms) beyond 64 slots — problems with
repeated categories (tests/candidate_tables_reference.py: up to 200 task nodes, 166 non-empty lists, empty ones between them),
more than 64 action rows, patches, float32 actions with reduct != 0 and the status words of failed problems inside a batch —
against the host path (loadDataOther + WOA._prepare), every field ``==`` and the candidates by their bits; then the searches on
the tables the device built.  tests/test_candidate_tables_host.py holds the conditions on these inputs."""
import numpy as np
import pytest
import torch

import candidate_tables_reference as ctr
import descent_reference as ref
import pair_window_reference as wref
from kernel_checks import twice
from test_candidate_tables_host import PICK_SEED
from test_gpu_refine import _assert_tables_equal, _device_batch, _host_tables

pytestmark = pytest.mark.gpu


# ---- helpers: the data sets (written once), one build run twice, the tightened comparison ------------------------------------------

def _world(dev, tmp_path_factory, name, ds):
    import gnnpn_sc_amd.synth as synth
    tmp = tmp_path_factory.mktemp(name)
    synth.write_dataset(str(tmp), "QWS", ds)
    svc, batch = _device_batch(ds, ctr.n_train(ds), dev)
    operands = (svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds)
    return {"root": str(tmp), "ds": ds, "svc": svc, "batch": batch, "operands": operands, "dev": dev}


@pytest.fixture(scope="module")
def world(dev, tmp_path_factory):
    return _world(dev, tmp_path_factory, "candidate_tables", ctr.make_dataset())


@pytest.fixture(scope="module")
def search_world(dev, tmp_path_factory):
    """A smaller batch on which the host path raises for no problem (test_candidate_tables_host.py), its tables and the host's."""
    from gnnpn_sc_amd import ops
    w = _world(dev, tmp_path_factory, "candidate_tables_search", ctr.make_dataset(ctr.SEARCH_SEED, ctr.SEARCH_COUNTS, ()))
    w["acts"] = ctr.make_picks(w["ds"], 0, 200, PICK_SEED, mismatch=False)
    w["host"] = ctr.host_tables(w["root"], w["acts"], 0)[0]
    w["tabs"] = ops.woa_candidates(*w["operands"], torch.from_numpy(w["acts"]).to(dev))          # raises on a non-zero status
    _assert_matches_host(w["tabs"], w["host"])
    w["tables"] = [(cats, bounds, start) for cats, _len0, start, bounds in w["host"]]
    return w


def _build(w, acts, reduct, patches=(), dtype=torch.float64):
    """(tables, the rows the host sees): woa_candidates — woa_candidates_replicas for [B, R, T, 8] rows — run twice, bit for bit."""
    from gnnpn_sc_amd import ops
    a = torch.from_numpy(np.ascontiguousarray(acts)).to(w["dev"], dtype)
    entry = ops.woa_candidates if a.dim() == 3 else ops.woa_candidates_replicas
    tabs = twice(lambda: entry(*w["operands"], a, reduct=reduct, patches=patches, check_status=False))
    return tabs, a.double().cpu().numpy()


def _assert_matches_host(tabs, host):
    """_assert_tables_equal, then: the specific status word where the host raised, prob_ptr and cand_ptr whole (a failed problem
    leaves its neighbours' ranges where the host's counts put them), and the sizes the searches size their launches by."""
    _assert_tables_equal(tabs, host)
    lay = ctr.layout(host)
    assert None not in lay["status"]
    assert tabs["status"].cpu().tolist() == lay["status"]
    assert tabs["prob_ptr"].cpu().tolist() == lay["prob_ptr"]
    assert tabs["cand_ptr"].cpu().tolist() == lay["cand_ptr"]
    assert tabs["cand"].shape[0] == lay["cand_ptr"][-1] and tabs["len_init"].numel() == tabs["start_pos"].numel() == lay["prob_ptr"][-1]
    assert (tabs["max_slots"], tabs["max_cand"]) == (lay["max_slots"], lay["max_cand"])
    return lay


# ---- 1. device tables == host tables ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("reduct", ctr.REDUCTS)
def test_tables_equal_host_beyond_64_slots(world, reduct, dtype):
    """200 action rows (four passes of the row loop), up to 166 lists (three passes of the slot loops), float32 rows with reduct != 0:
    the pick set comes from the widened rows."""
    acts = ctr.make_picks(world["ds"], reduct, 200, PICK_SEED)
    tabs, seen = _build(world, acts, reduct, dtype=dtype)
    lay = _assert_matches_host(tabs, ctr.host_tables(world["root"], seen, reduct)[0])
    assert {ctr.STATUS_OK, ctr.STATUS_ROWS_MISMATCH, ctr.STATUS_NO_SLOTS} == set(lay["status"]) and lay["max_slots"] > 128


@pytest.mark.parametrize("reduct", [0, 0.55])
@pytest.mark.parametrize("a_T", ctr.A_TS)
def test_tables_equal_host_at_row_counts(world, a_T, reduct):
    """65 rows: the second pass of the row loop holds one row.  130: three passes, problems of 65 .. 130 lists keep their rows."""
    acts = ctr.make_picks(world["ds"], reduct, a_T, PICK_SEED)
    tabs, seen = _build(world, acts, reduct)
    _assert_matches_host(tabs, ctr.host_tables(world["root"], seen, reduct)[0])


def test_tables_equal_host_at_1024_rows(world):
    """The most rows the count launch takes: 64 KB of dynamic LDS, sixteen passes of the row loop."""
    acts = ctr.make_picks(world["ds"], 0, 1024, PICK_SEED)
    tabs, seen = _build(world, acts, 0)
    _assert_matches_host(tabs, ctr.host_tables(world["root"], seen, 0)[0])


def test_driver_fixture_float32_with_reduct(dev, tmp_path, monkeypatch):
    """test_gpu_refine.test_candidates_equal_host_on_the_driver_fixture's float32 leg at reduct = 0.55."""
    from gnnpn_sc_amd import ops
    from test_gpu_refine import _woa_driver
    _fx, ds, actions, n_train = _woa_driver(tmp_path, monkeypatch)
    svc, batch = _device_batch(ds, n_train, dev)
    a = torch.from_numpy(actions).to(dev, torch.float32)
    host, _s, _m = _host_tables("QWS", a.double().cpu().numpy(), 0.55)
    tabs = twice(lambda: ops.woa_candidates(svc.cat_ptr, svc.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds, a,
                                            reduct=0.55, check_status=False))
    _assert_matches_host(tabs, host)
    assert sum(1 for h in host if not isinstance(h, Exception)) > len(host) // 2


def test_replica_tables_equal_host_beyond_64_slots(world):
    """R = 3 replicas with their own picks, replica 1 alone mismatched in two problems of more than 64 lists: row b * R + r holds
    woa_candidates' tables for actions_all[:, r], the status word per row."""
    from gnnpn_sc_amd import ops
    R, reduct = 3, 0.55
    acts_all = np.stack([ctr.make_picks(world["ds"], reduct, 200, PICK_SEED + r, mismatch=r == 1) for r in range(R)], 1)
    tabs, seen = _build(world, acts_all, reduct)
    B = seen.shape[0]
    assert tabs["replicas"] == R and tabs["status"].numel() == B * R
    host = [ctr.host_tables(world["root"], seen[:, r], reduct)[0] for r in range(R)]
    lay = _assert_matches_host(tabs, [host[q % R][q // R] for q in range(B * R)])
    status = np.asarray(lay["status"]).reshape(B, R)
    assert any(status[b].tolist() == [0, ctr.STATUS_ROWS_MISMATCH, 0] for b in range(B))
    prob_ptr, cand_ptr = tabs["prob_ptr"].cpu().tolist(), tabs["cand_ptr"].cpu().tolist()
    for r in range(R):
        one = ops.woa_candidates(*world["operands"], torch.from_numpy(np.ascontiguousarray(seen[:, r])).to(world["dev"]), reduct=reduct,
                                 check_status=False)
        rows = torch.arange(B) * R + r
        for k in ("status", "n_slots", "bounds"):
            assert torch.equal(tabs[k].cpu()[rows], one[k].cpu()), (r, k)
        p1, c1 = one["prob_ptr"].cpu().tolist(), one["cand_ptr"].cpu().tolist()
        for b in range(B):
            q = b * R + r
            assert prob_ptr[q + 1] - prob_ptr[q] == p1[b + 1] - p1[b], (b, r)
            s, s1, n = prob_ptr[q], p1[b], p1[b + 1] - p1[b]
            for k in ("len_init", "start_pos"):
                assert torch.equal(tabs[k][s:s + n], one[k][s1:s1 + n]), (b, r, k)
            assert [v - cand_ptr[s] for v in cand_ptr[s:s + n + 1]] == [v - c1[s1] for v in c1[s1:s1 + n + 1]], (b, r)
            assert torch.equal(tabs["cand"][cand_ptr[s]:cand_ptr[s + n]].view(torch.int64),
                               one["cand"][c1[s1]:c1[s1 + n]].view(torch.int64)), (b, r)


# ---- 2. patches ---------------------------------------------------------------------------------------------------------------------------

NO_MATCH = ((0.5, 0.5, 0.5, 0.5), 1, 0.7)


def _patch_case(w, reduct=0):
    """Action rows and patches over one problem of at most 50 lists and one of more than 64 (there in slots >= 64): (acts, patches,
    host tables without the patches, {problem: the four slots}).  Slot j1: a patch whose ``want`` is a picked member's rounded row
    (column 0).  j2: a foreign row that a patch (column 3) turns into the member at position 0 of the slot's list.  j3: two chained
    patches (columns 0 and 3), the first one's result the second one's ``want``.  j4: a row holding 0.0 under a ``want`` holding -0.0."""
    ds = w["ds"]
    acts = ctr.make_picks(ds, reduct, 200, PICK_SEED)
    plain = ctr.host_tables(w["root"], acts, reduct)[0]
    counts = ctr.task_counts(ds)
    patches, slots = [NO_MATCH], {}
    for k, b in enumerate((counts.index(40), counts.index(150))):
        cats, len0, start, _bd = plain[b]
        assert start is not None and (8 <= len(cats) <= 50 or len(cats) > 72)
        members = [j for j in range(len(cats)) if start[j] < len0[j]][::-1]              # from the last slot down: beyond 64 where there are
        j1 = members[0]
        j3 = next(j for j in members[1:] if ctr.rounded(acts[b, j]) != ctr.rounded(acts[b, j1]))
        j2, j4 = [j for j in range(len(cats) - 1, -1, -1) if j not in (j1, j3)][:2]
        a = ctr.rounded(acts[b, j3])
        first = [(0.11111, 0.31111)[k]] + a[1:]
        member = list(cats[j2][0])
        acts[b, j2, :4] = member[:3] + [0.5]
        acts[b, j4, :4] = [0.0, 0.3, 0.95, 0.96]
        patches += [(tuple(ctr.rounded(acts[b, j1])), 0, 0.98765), (tuple(member[:3] + [0.5]), 3, member[3]),
                    (tuple(a), 0, first[0]), (tuple(first), 3, 0.22222), ((-0.0, 0.3, 0.95, 0.96), 1, 0.44444)]
        slots[b] = (j1, j2, j3, j4, tuple(first[:3] + [0.22222]))
    return acts, patches, plain, slots


def test_patches_equal_host(world):
    """reduct = 0 (the lists do not depend on the picks): what each patch does is asserted on the host's tables first."""
    acts, patches, plain, slots = _patch_case(world)
    host = ctr.host_tables(world["root"], acts, 0, patches)[0]
    for b, (j1, j2, j3, j4, chained) in slots.items():
        cats, len0, start, _bd = host[b]
        assert start[j1] == len0[j1] and len(cats[j1]) == len0[j1] + 1 and cats[j1][-1][0] == 0.98765      # a member made foreign
        assert start[j2] == 0 and len(cats[j2]) == len0[j2]                                               # a foreign row made a member
        assert start[j3] == len0[j3] and cats[j3][-1] == chained                                          # both patches, in order
        assert start[j4] == len0[j4] and cats[j4][-1] == (0.0, 0.44444, 0.95, 0.96)                       # -0.0 == 0.0
        assert len(cats) <= 50 or min(j1, j2, j3, j4) >= 64
    swapped = patches[:3] + [patches[4], patches[3]] + patches[5:]
    assert ctr.host_tables(world["root"], acts, 0, swapped)[0][min(slots)][0] != host[min(slots)][0]      # order matters
    tabs, _seen = _build(world, acts, 0, patches)
    _assert_matches_host(tabs, host)
    tabs, _seen = _build(world, acts, 0, swapped)
    _assert_matches_host(tabs, ctr.host_tables(world["root"], acts, 0, swapped)[0])
    tabs, _seen = _build(world, acts, 0, [NO_MATCH])
    _assert_matches_host(tabs, ctr.host_tables(world["root"], acts, 0)[0])


def _protected_case(w, reduct=0.55):
    """Rows with, in a problem of at most 50 lists and in one of more than 64, a pick that addS skips by, and a patch of that
    row: the pick set holds the unpatched row on both paths, and the lists would differ had it been patched too."""
    acts = ctr.make_picks(w["ds"], reduct, 200, PICK_SEED)
    counts = ctr.task_counts(w["ds"])
    patches, planted = [], {}
    for k, b in enumerate((counts.index(40), counts.index(150))):
        val = 0.12345 + 0.1 * k
        acts, j, key = ctr.protected_pick(w["ds"], b, reduct, acts, 0, val)
        patches.append((tuple(key), 0, val))
        planted[b] = (j, tuple(key), (val,) + tuple(key[1:]))
    return acts, patches, planted


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_patches_leave_the_pick_set_alone(world, dtype):
    acts, patches, planted = _protected_case(world)
    tabs, seen = _build(world, acts, 0.55, patches, dtype=dtype)
    host = ctr.host_tables(world["root"], seen, 0.55, patches)[0]
    for b, (j, key, moved) in planted.items():                      # the host first: the list follows the unpatched pick ...
        cats, len0, start, _bd = host[b]
        assert key in cats[j][:len0[j]] and start[j] == len0[j] and cats[j][-1] == moved                  # ... the start the patched row
    _assert_matches_host(tabs, host)


def test_patches_through_replicas(world):
    """Replica 0: the patch case's rows; replica 1: the plain picks, which the same patches leave as they are or change as well."""
    acts, patches, _plain, _slots = _patch_case(world)
    both = np.stack([acts, ctr.make_picks(world["ds"], 0, 200, PICK_SEED + 1)], 1)
    tabs, seen = _build(world, both, 0, patches)
    host = [ctr.host_tables(world["root"], seen[:, r], 0, patches)[0] for r in range(2)]
    _assert_matches_host(tabs, [host[q % 2][q // 2] for q in range(2 * seen.shape[0])])
    acts, patches, _planted = _protected_case(world)
    both = np.stack([ctr.make_picks(world["ds"], 0.55, 200, PICK_SEED + 1, mismatch=False), acts], 1)
    tabs, seen = _build(world, both, 0.55, patches)
    host = [ctr.host_tables(world["root"], seen[:, r], 0.55, patches)[0] for r in range(2)]
    _assert_matches_host(tabs, [host[q % 2][q // 2] for q in range(2 * seen.shape[0])])


def test_refine_with_patches_equals_fine_tune(search_world):
    """pipeline.refine(..., patches=...) against WOA.fine_tune(..., patches=...) on the host-built problems, problems of 3 .. 166 lists."""
    from gnnpn_sc_amd import WOA
    from gnnpn_sc_amd.pipeline import refine
    w, dev = search_world, search_world["dev"]
    acts, host = w["acts"], w["host"]
    patches = [NO_MATCH]
    for b, (cats, len0, start, _bd) in enumerate(host):
        if start is not None and len(cats) > 64:
            j = max(j for j in range(len(cats)) if start[j] < len0[j])
            patches += [(tuple(ctr.rounded(acts[b, j])), 0, 0.98765), ((0.98765,) + tuple(ctr.rounded(acts[b, j])[1:]), 3, 0.91919)]
    assert len(patches) >= 5
    patched = ctr.host_tables(w["root"], acts, 0, patches)[0]
    assert any(p[0] != h[0] for p, h in zip(patched, host))
    B = acts.shape[0]
    seeds = [77 + i for i in range(B)]
    res = refine(w["svc"], w["batch"], {"actions": torch.from_numpy(acts).to(dev)}, 10, 12, seeds=seeds, patches=patches)
    want = WOA.fine_tune(ctr.host_problems(w["root"], acts, 0), 10, 12, seeds, dev, patches=patches)
    fit, hist, draws = res["best_fitness"].cpu().tolist(), res["history"].cpu().tolist(), res["draws"].cpu().tolist()
    rows, n_slots, pos = res["best_rows"].cpu().tolist(), res["n_slots"].cpu().tolist(), res["best_pos"].cpu().tolist()
    for b, wb in enumerate(want):
        assert n_slots[b] == len(patched[b][0]), b
        assert fit[b] == wb["bestFitness"] and hist[b] == wb["bestFitnesses"] and draws[b] == wb["draws"], b
        assert pos[b][:n_slots[b]] == [int(v) for v in wb["bestPops"]], b
        assert [tuple(r) for r in rows[b][:n_slots[b]]] == [tuple(r) for r in wb["bestSolutions"]], b


# ---- 3. the searches on tables the device built ---------------------------------------------------------------------------------------------

def test_descend_on_device_built_tables(search_world):
    from test_gpu_descend import _assert_equal
    got = {k: v.cpu().tolist() for k, v in twice(search_world["tabs"].descend).items()}
    _assert_equal(got, search_world["tables"], [ref.descend(*tab) for tab in search_world["tables"]])
    assert any(m > 0 for m in got["moves"])


def test_descend_pairs_windowed_on_device_built_tables(search_world):
    from test_gpu_pair_descend import _assert_equal
    tables = search_world["tables"]
    want = [wref.descend_pairs(*tab, max_span=4) for tab in tables]
    got = {k: v.cpu().tolist() for k, v in twice(lambda: search_world["tabs"].descend_pairs_windowed(max_span=4)).items()}
    _assert_equal(got, tables, want)


def test_eswoa_on_device_built_tables(search_world):
    from gnnpn_sc_amd import WOA
    w, dev = search_world, search_world["dev"]
    problems = ctr.host_problems(w["root"], w["acts"], 0)
    seeds = [321 + 5 * i for i in range(len(problems))]
    want = [WOA.fine_tune([p], popSize=12, MAX_Iter=9, seeds=[s], device=dev)[0] for p, s in zip(problems, seeds)]
    fit, pos, hist, draws, rows = twice(lambda: w["tabs"].eswoa(12, 9, torch.tensor(seeds, dtype=torch.int64, device=dev)))
    fit, pos, hist, draws, rows = fit.cpu().tolist(), pos.cpu().tolist(), hist.cpu().tolist(), draws.cpu().tolist(), rows.cpu().tolist()
    for p, (wp, (cats, _b, start)) in enumerate(zip(want, w["tables"])):
        T = len(cats)
        assert fit[p] == wp["bestFitness"] and hist[p] == wp["bestFitnesses"] and draws[p] == wp["draws"], p
        if wp["bestPops"] is not None:
            assert pos[p][:T] == [int(v) for v in wp["bestPops"]], p
            assert [tuple(r) for r in rows[p][:T]] == [tuple(r) for r in wp["bestSolutions"]], p
