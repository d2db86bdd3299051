"""-m "not gpu": tests/services_reference.py held against the host path itself (the rows its indices name are what addS and
WOA._prepare keep), the conditions on the batch that tests/test_gpu_services.py leans on — asserted here, not assumed there —,
the signatures of the new names beside the unchanged old ones, the four entries in header and binding, and the refusals of the
command line."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import candidate_tables_reference as ctr
import descent_reference as ref
import services_reference as sref
from conftest import ROOT
from test_candidate_tables_host import PICK_SEED

NEW_ENTRIES = ("gnnpn_woa_candidates_services", "gnnpn_woa_candidates_replicas_services", "gnnpn_search_services",
               "gnnpn_services_merit_f64")


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    import gnnpn_sc_amd.synth as synth
    tmp = tmp_path_factory.mktemp("services_host")
    synth.write_dataset(str(tmp), "QWS", ctr.make_dataset())
    return str(tmp)


@pytest.fixture(scope="module")
def named(tmp_path_factory):
    """The named batch, its picks, the host's tables and the reference's, and the reference descent of every problem."""
    import gnnpn_sc_amd.synth as synth
    ds, cat, twin = sref.named_dataset()
    tmp = tmp_path_factory.mktemp("services_named")
    synth.write_dataset(str(tmp), "QWS", ds)
    acts, ids = sref.named_picks(ds, twin=twin)
    host = ctr.host_tables(str(tmp), acts, 0)[0]
    tabs = sref.named_tables(ds, acts, 0, action_ids=ids)
    runs = [None if isinstance(h, Exception) else ref.descend(h[0], h[3], h[2]) for h in host]
    return {"ds": ds, "cat": cat, "twin": twin, "acts": acts, "ids": ids, "host": host, "tabs": tabs, "runs": runs}


# ---- the reference against the host path ---------------------------------------------------------------------------------------------------

def test_service_rows_are_the_rows_of_the_device_table():
    from gnnpn_sc_amd.loadData import tables_from_dataset
    for ds in (ctr.make_dataset(), sref.named_dataset()[0]):
        rows, cat_ptr = sref.service_rows(ds)
        table, _pb = tables_from_dataset(ds, ctr.n_train(ds), None)
        assert np.asarray(table.qos, dtype=np.float64).tolist() == [list(r) for r in rows]
        assert np.asarray(table.cat_ptr).tolist() == cat_ptr


@pytest.mark.parametrize("reduct", ctr.REDUCTS)
def test_the_indices_name_the_rows_addS_keeps(reduct):
    ds = ctr.make_dataset()
    rows, _cat_ptr = sref.service_rows(ds)
    ssets = ctr.pick_sets(ctr.make_picks(ds, reduct, 200, PICK_SEED))
    for picks in (None, ssets):
        want = ctr.slot_lists(ds, reduct, picks)
        got = sref.slot_ids(ds, reduct, picks)
        assert len(want) == len(got)
        for b, (lists, (_index, ids)) in enumerate(zip(want, got)):
            assert [[rows[s] for s in k] for k in ids] == [[tuple(r) for r in lst] for lst in lists], b
            assert all(len(set(k)) == len(k) for k in ids), b
    if reduct:
        assert want != ctr.slot_lists(ds, reduct)                     # the picks change lists: the pick-set path was walked


@pytest.mark.parametrize("reduct", ctr.REDUCTS)
def test_named_tables_are_the_host_tables(root, reduct):
    """WOA._prepare's lists, lengths and starts from the indices: the kept part of every list rounds to the host's rows (unrounded
    without a seed), an appended row is where the host appended one, a problem the host raises on has no tables."""
    ds = ctr.make_dataset()
    rows, _cat_ptr = sref.service_rows(ds)
    acts = ctr.make_picks(ds, reduct, 200, PICK_SEED)
    host = ctr.host_tables(root, acts, reduct)[0]
    tabs = sref.named_tables(ds, acts, reduct)
    appended = 0
    for b, (h, t) in enumerate(zip(host, tabs)):
        assert isinstance(h, Exception) == (t is None), b
        if t is None:
            continue
        cats, len0, start, _bounds = h
        assert len(cats) == len(t["cand_service"]) == len(t["slot_node"]) == len(t["slot_cat"]), b
        assert t["seeded"] == (start is not None) and (start is None or t["start"] == start), b
        nodes = ctr.problems_of(ds)[b]
        assert t["slot_node"] == sorted(t["slot_node"]) and all(1 <= n < len(nodes) for n in t["slot_node"]), b
        assert t["slot_cat"] == [nodes[n][:-6].index(1) - 1 for n in t["slot_node"]], b
        for j, (cat, ids) in enumerate(zip(cats, t["cand_service"])):
            assert len(ids) == len(cat) and [s >= 0 for s in ids[:len0[j]]] == [True] * len0[j], (b, j)
            named = [tuple(round(v, 5) for v in rows[s]) if t["seeded"] else rows[s] for s in ids[:len0[j]]]
            assert named == [tuple(r) for r in cat[:len0[j]]], (b, j)
            assert ids[len0[j]:] == [-1] * (len(cat) - len0[j]), (b, j)
            appended += len(cat) - len0[j]
    assert appended > 0


def test_the_reference_takes_patches_as_the_host_does(root):
    from test_gpu_candidate_tables import _patch_case
    acts, patches, _plain, _slots = _patch_case({"ds": ctr.make_dataset(), "root": root})
    host = ctr.host_tables(root, acts, 0, patches)[0]
    tabs = sref.named_tables(ctr.make_dataset(), acts, 0, patches)
    for h, t in zip(host, tabs):
        assert isinstance(h, Exception) == (t is None)
        if t is not None and h[2] is not None:
            assert t["start"] == h[2] and [len(i) for i in t["cand_service"]] == [len(c) for c in h[0]]


# ---- the conditions the GPU tests lean on ------------------------------------------------------------------------------------------------------

def test_conditions_on_the_named_batch(named):
    host, tabs, runs, ids = named["host"], named["tabs"], named["runs"], named["ids"]
    ok = [b for b, h in enumerate(host) if not isinstance(h, Exception)]
    failed = [b for b in range(len(host)) if b not in ok]
    # a failed problem between good ones, and nothing else failed; every good problem is seeded (the scorer rounds the whole batch)
    assert failed and all(0 < b < len(host) - 1 and b - 1 in ok and b + 1 in ok for b in failed)
    assert [t is None for t in tabs] == [b in failed for b in range(len(host))]
    assert all(host[b][2] is not None for b in ok)
    sizes = [len(host[b][0]) for b in ok]
    assert min(sizes) <= 3 and sum(1 for n in sizes if 64 < n <= 128) >= 1 and max(sizes) > 128
    # the final composition of the reference descent keeps a foreign row in one problem at least, none in another, and leaves
    # some foreign start rows behind: descent moved
    keeps, free, left = [], [], 0
    for b in ok:
        _cats, len0, start, _bd = host[b]
        final = [p >= n for p, n in zip(runs[b]["best_pos"], len0)]
        (keeps if any(final) else free).append(b)
        left += sum(1 for s, n, f in zip(start, len0, final) if s >= n and not f)
    assert keeps and free and left > 0 and any(runs[b]["moves"] > 0 for b in ok)
    assert any(len(host[b][0]) > 64 for b in keeps)
    # every foreign row has an id, which is no member of its list, and every id names the action row bit for bit
    rows, _cat_ptr = sref.service_rows(named["ds"])
    for b in ok:
        assert all(s >= 0 for k in tabs[b]["cand_service"] for s in k), b
        real = [k for k in range(ids.shape[1]) if ids[b, k] >= 0]
        assert len(real) == len(host[b][0]) and [rows[ids[b, k]] for k in real] == [tuple(named["acts"][b, k, :4]) for k in real], b


def test_the_twin_services_round_to_one_row_and_the_first_is_named(named):
    """Two services of one category with equal rounded rows: a list that keeps both starts, for a pick of the second, at the first."""
    ds, (first, twin) = named["ds"], named["twin"]
    rows, cat_ptr = sref.service_rows(ds)
    assert cat_ptr[named["cat"]] <= first and twin == first + 1 < cat_ptr[named["cat"] + 1] and rows[first] != rows[twin]
    assert tuple(round(v, 5) for v in rows[first]) == tuple(round(v, 5) for v in rows[twin])
    hits = 0
    for b, t in enumerate(named["tabs"]):
        for j, k in enumerate(t["cand_service"] if t else ()):
            if first in k and twin in k:
                real = [c for c in range(named["ids"].shape[1]) if named["ids"][b, c] >= 0]
                assert named["ids"][b, real[j]] == twin and k[t["start"][j]] == first and k.index(first) < k.index(twin), (b, j)
                hits += 1
    assert hits > 0


def test_mapping_and_scoring_reference(named):
    """The certificate on the host: the services the reference descent ends on score its best_fitness, bit for bit — and a
    not-searched problem, a Python position and a position outside its list map as the header says."""
    rows, _cat_ptr = sref.service_rows(named["ds"])
    for b, (h, t, run) in enumerate(zip(named["host"], named["tabs"], named["runs"])):
        n_nodes = len(ctr.problems_of(named["ds"])[b])
        if t is None:
            assert sref.map_services(None, 0.5, [], n_nodes, 4) == ([-1] * 4, [-1] * n_nodes)
            continue
        n = len(t["slot_node"])
        best, nodes = sref.map_services(t, run["best_fitness"], run["best_pos"], n_nodes, n + 2)
        assert best[n:] == [-1, -1] and min(best[:n]) >= 0 and nodes[0] == -1
        assert [s for s in nodes if s >= 0] == best[:n]
        assert [tuple(round(v, 5) for v in rows[s]) for s in best[:n]] == [tuple(r) for r in run["best_rows"]], b
        assert sref.score(rows, nodes, h[3]) == (run["best_fitness"], n), b
        assert sref.map_services(t, math.nan, run["best_pos"], n_nodes, n) == ([-1] * n, [-1] * n_nodes)
        pos = [p - len(k) for p, k in zip(run["best_pos"], t["cand_service"])]                 # the same positions, Python's way
        assert sref.map_services(t, 0.5, pos, n_nodes, n) == (best[:n], nodes)
        pos[0] = len(t["cand_service"][0])
        assert sref.map_services(t, 0.5, pos, n_nodes, n)[0] == [-1] + best[1:n]
    assert sref.score(rows, [-1, len(rows)], [0, 1, 0, 1]) == (pytest.approx(math.nan, nan_ok=True), -1)
    assert sref.score(rows, [-1, -1], [0, 1, 0, 1])[1] == 0 and sref.score(rows, [-2], [0, 1, 0, 1])[1] == -1


# ---- names, signatures, the C entries ---------------------------------------------------------------------------------------------------------

def _defaults(f):
    return {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}


def test_signatures_new_and_old():
    from gnnpn_sc_amd import ML2PN, ops
    from gnnpn_sc_amd import pipeline as pl
    old = ["cat_ptr", "qos", "x", "seg_ptr", "local_bounds", "global_bounds", "actions", "reduct", "patches", "check_status"]
    assert list(inspect.signature(ops.woa_candidates).parameters) == old
    assert list(inspect.signature(ops.woa_candidates_named).parameters) == old + ["action_ids"]
    old_r = old[:6] + ["actions_all"] + old[7:]
    assert list(inspect.signature(ops.woa_candidates_replicas).parameters) == old_r
    assert list(inspect.signature(ops.woa_candidates_replicas_named).parameters) == old_r + ["action_ids"]
    for f in (ops.woa_candidates, ops.woa_candidates_replicas):
        assert _defaults(f) == {"reduct": 0, "patches": (), "check_status": True}
    for f in (ops.woa_candidates_named, ops.woa_candidates_replicas_named):
        assert _defaults(f) == {"reduct": 0, "patches": (), "check_status": True, "action_ids": None}
    assert list(inspect.signature(ops.SearchTables.services).parameters) == ["self", "res", "seg_ptr", "n_nodes", "start_index"]
    assert _defaults(ops.SearchTables.services) == {"start_index": None}
    assert list(inspect.signature(ops.services_merit).parameters) == ["seg_ptr", "node_services", "qos", "bounds", "rounded", "max_slots", "wide"]
    assert _defaults(ops.services_merit) == {"max_slots": None, "wide": None}
    sig = inspect.signature(pl.name_services)
    assert list(sig.parameters) == ["services", "batch", "out", "res", "reduct", "patches"] and _defaults(pl.name_services) == {"reduct": 0, "patches": ()}
    assert list(inspect.signature(pl.ML2PNPipeline.name_services).parameters)[1:] == list(sig.parameters)
    assert _defaults(pl.ML2PNPipeline.name_services) == _defaults(pl.name_services)
    assert list(inspect.signature(pl.score_services).parameters) == ["services", "batch", "node_services", "rounded"]
    assert _defaults(pl.score_services) == {"rounded": True}
    # the search stages keep their signatures, and ML2PN.infer its pinned one: the services come under a name of their own
    assert list(inspect.signature(pl.descend).parameters) == ["services", "batch", "out", "max_sweeps", "reduct", "min_cost", "patches"]
    assert list(inspect.signature(pl.refine).parameters) == ["services", "batch", "out", "popSize", "MAX_Iter", "reduct", "seeds", "min_cost",
                                                             "patches", "descend", "pair_rounds"]
    assert "services" not in inspect.signature(ML2PN.infer).parameters
    assert list(inspect.signature(ML2PN.infer_services).parameters) == [
        "dataset", "net", "low", "high", "n_per", "epoch", "device", "batch_size", "precision", "woa", "samples", "sample_seed", "descend",
        "all_starts", "pair_rounds", "pair_span", "pair_rank"]
    assert list(inspect.signature(ML2PN.refine_test_quarter).parameters) == ["dataset", "ds", "pipe", "svc", "actions", "popSize", "MAX_Iter",
                                                                             "reduct", "seed", "descend", "starts", "pair_rounds"]


def _prototype(header, name):
    m = re.search(r"^int " + name + r"\((.*?)\);", header, re.S | re.M)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_and_binding_agree_on_the_four_entries():
    import ctypes
    from gnnpn_sc_amd import _lib
    with open(os.path.join(ROOT, "include", "gnnpn_hip.h")) as f:
        header = f.read()
    kinds = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    for name in NEW_ENTRIES:
        assert name in _lib.EXPORTS
        res, args = _lib._SIGNATURES[name]
        want = [ctypes.c_void_p if "*" in a else kinds[a.rsplit(" ", 1)[0]] for a in _prototype(header, name)]
        assert res is ctypes.c_int and args == want, name
    assert "GNNPN_ABI_VERSION 9 " in header and _lib.ABI_VERSION == 9          # new entries, no changed one: as the earlier search entries
    one, rep = _prototype(header, NEW_ENTRIES[0]), _prototype(header, NEW_ENTRIES[1])
    assert rep == one[:1] + ["int32_t R"] + one[1:]                            # the replica form: the same operands behind R


def test_entries_refuse_bad_arguments_before_any_launch():
    """An empty batch launches nothing; null operands and bad sizes are refused on the host (no GPU is touched either way)."""
    from gnnpn_sc_amd import _lib
    lib = _lib.load()
    P = 1 << 20                                                                # a pointer that is never read: every case fails first
    assert lib.gnnpn_abi_version() == 9
    merit = lambda B=2, n_nodes=6, n_services=4, rounded=1, max_slots=3, wide=0, seg=P, qos=P: lib.gnnpn_services_merit_f64(   # noqa: E731
        B, seg, n_nodes, P, qos, n_services, P, rounded, max_slots, wide, P, P, None)
    for kw in ({"B": -1}, {"n_nodes": -1}, {"n_services": -1}, {"rounded": 2}, {"max_slots": 0}):
        assert merit(**kw) == -1 and b"bad argument" in lib.gnnpn_last_error(), kw
    assert merit(seg=None) == -1 and b"null" in lib.gnnpn_last_error()
    assert merit(qos=None) == -1 and b"null" in lib.gnnpn_last_error()
    assert merit(qos=P + 4) == -1 and b"misaligned" in lib.gnnpn_last_error()
    assert merit(max_slots=5000) == _lib.E_UNSUP and b"5000 rows" in lib.gnnpn_last_error()
    assert merit(B=0, seg=None) == 0
    names = lambda B=2, R=1, ld=3, fit=P, pos=P, node=P: lib.gnnpn_search_services(   # noqa: E731
        B, R, None, fit, pos, ld, P, 4, P, 9, P, P, P, 6, P, node, None)
    for kw in ({"B": -1}, {"R": 0}, {"ld": 0}, {"B": 1 << 20, "R": 1 << 12}):
        assert names(**kw) == -1 and b"bad argument" in lib.gnnpn_last_error(), kw
    for kw in ({"fit": None}, {"pos": None}, {"node": None}):
        assert names(**kw) == -1 and b"null" in lib.gnnpn_last_error(), kw
    assert names(B=0, fit=None) == 0
    built = lambda B=2, a_T=3, ids=None, acts=P, ws=P, ws_bytes=1 << 30, f64=1: lib.gnnpn_woa_candidates_services(   # noqa: E731
        B, 6, P, P, acts, f64, a_T, ids, 5, ws, ws_bytes, P, P, 4, 9, P, P, P, None)
    for kw in ({"B": -1}, {"a_T": 0}, {"f64": 2}):
        assert built(**kw) == -1 and b"bad argument" in lib.gnnpn_last_error(), kw
    assert built(ids=P, acts=None) == -1 and b"null" in lib.gnnpn_last_error()
    assert built(ws_bytes=8) == -1 and b"workspace" in lib.gnnpn_last_error()
    assert built(a_T=20000) == _lib.E_UNSUP and b"action rows" in lib.gnnpn_last_error()
    assert built(B=0, ws=None) == 0
    assert lib.gnnpn_woa_candidates_replicas_services(2, 0, 6, P, P, P, 1, 3, None, 5, P, 1 << 30, P, P, 4, 9, P, P, P, None) == -1


def test_wrappers_refuse_host_tensors_and_tables_without_ids():
    from gnnpn_sc_amd import ML2PN, ops
    from gnnpn_sc_amd import pipeline as pl
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)   # noqa: E731
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        ops.services_merit(i32([0, 3, 6]), i32([-1, 0, 1, -1, 2, 3]), f64(4, 4), f64(2, 4), True)
    with pytest.raises(ops.GnnpnError, match=r"bounds \[B, 4\]"):
        ops.services_merit(i32([0, 3, 6]), i32([-1, 0, 1, -1, 2, 3]), f64(4, 4), f64(3, 4), True)
    tabs = ops.SearchTables(prob_ptr=i32([0, 2, 3]), cand_ptr=i32([0, 1, 2, 3]), max_slots=2, max_cand=2)
    res = {"best_fitness": f64(2), "best_pos": torch.zeros(2, 2, dtype=torch.int32)}
    with pytest.raises(ops.GnnpnError, match="tables without ids"):
        tabs.services(res, i32([0, 3, 6]), 6)
    tabs.update(cand_service=i32([0, 1, 2]), slot_node=i32([1, 2, 1]), slot_cat=i32([0, 0, 0]))
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        tabs.services(res, i32([0, 3, 6]), 6)
    with pytest.raises(ops.GnnpnError, match="3 problems x 1 rows expected"):
        tabs.services(res, i32([0, 3, 6, 9]), 9)

    class Svc:
        cat_ptr, qos = i32([0, 2, 4, 6]), f64(6, 4)

    class Batch:
        n_problems = 2
        x, seg_ptr = torch.zeros(6, 7), i32([0, 3, 6])
        local_bounds, global_bounds = f64(2, 3, 4), f64(2, 4)
    out = {"actions": torch.zeros(2, 3, 8)}
    for f in (pl.name_services, lambda *a, **k: pl.ML2PNPipeline.name_services(None, *a, **k)):
        with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
            f(Svc, Batch, out, res)
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        pl.score_services(Svc, Batch, i32([-1, 0, 1, -1, 2, 3]))
    assert pl.action_ids_of(out) is None and pl.action_ids_of(torch.zeros(2, 3, 8)) is None
    ids = pl.action_ids_of({"candidate_ids": i32([[4, 5, 6, 7], [0, 1, 2, 3]]), "idx_high": i32([[3, 0], [1, 1]])})
    assert ids.dtype == torch.int32 and ids.tolist() == [[7, 4], [1, 1]]
    for kw in ({}, {"descend": 4, "pair_span": 2}, {"descend": 4, "pair_rounds": 2, "pair_span": -1},
               {"descend": 4, "pair_rounds": 2, "pair_span": 1, "pair_rank": -1}, {"woa": {}, "pair_rounds": 2, "pair_span": 1, "pair_rank": 1}):
        with pytest.raises(ValueError, match="ML2PN.infer_services"):
            ML2PN.infer_services("QWS", None, None, None, 3, **kw)


def test_main_cli_refuses_services_before_any_file_is_read(capsys, tmp_path, monkeypatch):
    import main as cli
    monkeypatch.chdir(tmp_path)                            # no ./data here: reading a file would raise, not return 1
    base = ["main.py", "QWS", "ML+2PN", "-1", "--infer"]
    assert cli.main(base + ["--services"]) == 1
    assert cli.main(base + ["--services", "--samples=3"]) == 1
    assert capsys.readouterr().out.count("--services: needs --descend[=SWEEPS] or --woa") == 2
    assert cli.main(base + ["--services", "--pairs"]) == 1                                       # --pairs' own refusal comes first
    assert "--pairs[=ROUNDS]: needs --descend" in capsys.readouterr().out
    assert cli.main(base + ["--services", "--descend", "--all-starts"]) == 1
    assert "--all-starts: needs --samples=N" in capsys.readouterr().out
    for more in (["--descend"], ["--woa"], ["--descend=4", "--pairs", "--span=2", "--top=3"], ["--descend", "--woa", "--pairs"],
                 ["--descend", "--samples=3", "--all-starts"]):
        with pytest.raises(FileNotFoundError):
            cli.main(base + ["--services"] + more)                                               # accepted: goes on to the data
