"""-m "not gpu": pair-swap descent over shortlists (gnnpn_descend_pairs_shortlist_ragged_f64, ops.descend_pairs_shortlist_ragged,
SearchTables.descend_pairs_shortlist, pipeline.descend_pairs_shortlist / descend_starts_pairs_shortlist, ML2PN.infer_pairs_shortlist,
`main.py ... --pairs --top=M`) rejects bad arguments and host tensors before any launch, and the plain-Python reference the GPU
tests compare with (tests/pair_shortlist_reference.py) has the properties that make those comparisons meaningful."""
import ctypes
import inspect

import pytest
import torch

import descent_reference as ref
import pair_descent_reference as pref
import pair_shortlist_reference as sref
import pair_window_reference as wref

P = ctypes.c_void_p(64)          # a non-null stand-in: every call below fails before it is dereferenced


# ---- the reference ----------------------------------------------------------------------------------------------------------------------

def _shared(r):
    return {k: v for k, v in r.items() if k != "shortlist"}


def test_no_rank_and_a_full_rank_are_the_windowed_reference():
    """Every field, on the 20 tables of the pair-swap host test, at three cut-offs; with a span too."""
    tables = sref.seeds_tables()
    assert len(tables) == 20
    for tab in tables:
        longest = max(len(c) for c in tab[0])
        for kw in ({}, {"max_rounds": 1}, {"max_sweeps": 0}):
            want = wref.descend_pairs(*tab, **kw)
            assert want == pref.descend_pairs(*tab, **kw)
            for m in (0, longest, longest + 3):
                assert _shared(sref.descend_pairs(*tab, max_rank=m, **kw)) == want, (m, kw)
        assert _shared(sref.descend_pairs(*tab, max_span=2, max_rank=longest)) == wref.descend_pairs(*tab, max_span=2)
        full = sref.descend_pairs(*tab, max_rank=longest)["shortlist"]
        assert full == [list(range(len(c))) for c in tab[0]]                    # a full rank keeps every position, in order
        assert sref.descend_pairs(*tab, max_rank=0)["shortlist"] is None and sref.descend_pairs(*tab, max_rank=2, max_rounds=0)["shortlist"] is None


def test_the_one_reference_replays_the_record_of_the_three():
    """tests/golden/pair_descent_reference_record.json: what the three reference functions returned while they were three loops
    (the plain one for span 0 and rank 0, the windowed one for rank 0, the shortlist one otherwise) on the 20 tables, at three
    cut-offs.  The one loop they are bound to now returns the same, float64 values bit for bit (float.hex)."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_descent_reference_record.json")) as f:
        record = json.load(f)
    tables = sref.seeds_tables()
    assert len(record["runs"]) == 20 * 3 * 5 and {r["table"] for r in record["runs"]} == set(range(20))
    assert {(r["max_span"], r["max_rank"]) for r in record["runs"]} == {(0, 0), (1, 0), (0, 1), (0, 2), (2, 2)}
    for run in record["runs"]:
        tab, kw, span, rank = tables[run["table"]], record["settings"][run["setting"]], run["max_span"], run["max_rank"]
        if rank:
            got = sref.descend_pairs(*tab, max_span=span, max_rank=rank, **kw)
        else:
            got = wref.descend_pairs(*tab, max_span=span, **kw) if span else pref.descend_pairs(*tab, **kw)
        assert got.pop("best_rows") == [tuple(tab[0][s][p]) for s, p in enumerate(got["best_pos"])]
        got.update(best_fitness=got["best_fitness"].hex(), start_fitness=got["start_fitness"].hex(),
                   round_history=[h.hex() for h in got["round_history"]])
        want = {k: v for k, v in run.items() if k not in ("table", "setting", "max_span", "max_rank")}
        assert got == want, (run["table"], kw, span, rank)


def test_a_shortlist_of_one_never_moves_by_pairs():
    """The one-swap optimum's own member is each slot's best single swap (the lowest position among equals is what descent took or
    kept), so S_i x S_j is the current pair: nothing is strictly below the current merit."""
    for tab in sref.seeds_tables():
        r, one = sref.descend_pairs(*tab, max_rank=1), ref.descend(*tab)
        assert r["pair_moves"] == 0 and r["rounds"] == 1 and r["best_fitness"] == one["best_fitness"] and r["best_pos"] == one["best_pos"]
        assert all(len(s) == 1 for s in r["shortlist"])


def test_a_shortlist_of_two_moves_and_loses():
    tables = sref.seeds_tables()
    two, full = [sref.descend_pairs(*t, max_rank=2) for t in tables], [wref.descend_pairs(*t) for t in tables]
    assert sum(r["pair_moves"] > 0 for r in two) >= 1 and sum(r["pair_moves"] > 0 for r in full) > sum(r["pair_moves"] > 0 for r in two)
    assert sum(a["best_fitness"] != b["best_fitness"] for a, b in zip(two, full)) >= 1
    assert all(a["best_fitness"] >= b["best_fitness"] or a["best_pos"] != b["best_pos"] for a, b in zip(two, full))


def test_the_wall_needs_two():
    tab = pref.wall_problem()
    stay, go = sref.descend_pairs(*tab, max_rank=1), sref.descend_pairs(*tab, max_rank=2)
    assert stay["best_pos"] == [0, 0] and stay["pair_moves"] == 0 and stay["converged"] == 1 and stay["best_fitness"] > 1.0
    assert go["best_pos"] == [1, 1] and go["pair_moves"] == 1 and go["best_fitness"] < 1.0
    assert _shared(go) == pref.descend_pairs(*tab)


def test_the_rank_three_wall():
    """The repairing row (position 1 of [poor, fix, THIRD]) ranks exactly third: two keep [0, 2] and the wall stays, three let it go.
    At T = 129 the two slots lie in different leaf blocks of np.sum."""
    for T, i, j in ((9, 2, 6), (129, 63, 64)):
        tab = sref.rank_three_wall(12902, T, i, j, nfill=1)
        one = ref.descend(*tab)
        assert one["best_pos"][i] == 0 and one["best_pos"][j] == 0 and one["best_fitness"] > 1.0
        lists = sref.shortlists(tab[0], tab[1], one["best_pos"], 2)
        assert lists[i] == [0, 2] and lists[j] == [0, 2]
        assert sref.shortlists(tab[0], tab[1], one["best_pos"], 3)[i] == [0, 1, 2]
        stay, go = sref.descend_pairs(*tab, max_rank=2), sref.descend_pairs(*tab, max_rank=3)
        assert stay["pair_moves"] == 0 and stay["best_fitness"] == one["best_fitness"] and stay["converged"] == 1
        assert go["pair_moves"] == 1 and go["best_pos"][i] == 1 and go["best_pos"][j] == 1 and go["best_fitness"] < 1.0
    assert wref.leaf_of(129, 63) != wref.leaf_of(129, 64)


def test_ties_go_to_the_lower_position_and_the_lowest_k():
    cats, bounds, start = sref.duplicated_rows()
    assert cats[0][1] == cats[0][2] and cats[1][1] == cats[1][2]
    assert sref.shortlists(cats, bounds, start, 2) == [[0, 1], [1, 2], [0, 1]]      # of two equal rows the lower one
    assert sref.shortlists(cats, bounds, start, 3) == [[0, 1, 2], [1, 2, 3], [0, 1, 2]]
    first = sref.descend_pairs(cats, bounds, start, max_rank=2, max_rounds=1)
    one = ref.descend(cats, bounds, start)
    assert first["shortlist"] == sref.shortlists(cats, bounds, one["best_pos"], 2) and first["shortlist"][0] == [0, 1]
    three = sref.descend_pairs(cats, bounds, start, max_rank=3)
    assert three["best_pos"][0] == 1 and three["best_pos"][2] == 1 and three["pair_moves"] == 1    # (1, 1): k = 4 of the tied 4, 5, 7, 8
    assert _shared(three) == wref.descend_pairs(cats, bounds, start)


def test_nan_merits_rank_last_by_position():
    cats, bounds, start = sref.nan_row_problem()
    lists = sref.shortlists(cats, bounds, start, 4)
    assert lists[1] == [0, 1, 3, 4]                                                 # three numbers, then the NaN at position 0, not 2
    assert sref.shortlists(cats, bounds, start, 3)[1] == [1, 3, 4] and sref.shortlists(cats, bounds, start, 5)[1] == [0, 1, 2, 3, 4]
    r = sref.descend_pairs(cats, bounds, start, max_rank=4)
    assert r["best_fitness"] == r["best_fitness"] and r["best_pos"][1] not in (0, 2)    # a NaN never wins


def test_the_gpu_cases_are_not_vacuous():
    """In every GPU case some list is longer than the rank (the full-rank cases apart, which say so in their names), and the shortlist
    changes the result of some case; both forms and a span are among them."""
    differs = 0
    for name, (tables, kw, _wide) in sref.CASES.items():
        m = kw["max_rank"]
        if name in ("seeds_m8", "third129_m3"):
            assert all(len(c) <= m for t in tables for c in t[0]), name
            continue
        assert all(any(len(c) > m for c in t[0]) for t in tables), name
        if name.startswith(("seeds_m", "dup", "third129_m2")):
            for t, w in zip(tables, sref.case_want(name)):
                differs += w["best_fitness"] != wref.descend_pairs(*t, max_span=kw.get("max_span", 0), max_rounds=kw.get("max_rounds", 4))["best_fitness"]
    assert differs >= 3
    assert any(w["pair_moves"] > 0 for w in sref.case_want("wide129_m2")) and any(w["pair_moves"] > 0 for w in sref.case_want("t64_m2"))
    tables, _kw, _w = sref.CASES["long_m65"]
    assert [len(c) for c in tables[0][0]] == [139, 70, 5] and len(sref.case_want("long_m65")[0]["shortlist"][0]) == 65
    assert any(c >= 128 for c in sref.case_want("long_m8")[0]["shortlist"][0])          # kept from the third chunk of the wave
    assert max(len(c) for c in sref.CASES["wide_long_m8"][0][0][0]) == 300
    w = sref.case_want("wide_long_m8")[0]
    assert max(w["shortlist"][20]) >= 256                                               # kept from the second chunk of the workgroup


# ---- the C entry ------------------------------------------------------------------------------------------------------------------------

def test_shortlist_entry_rejects_bad_arguments():
    from gnnpn_sc_amd import _lib
    lib = _lib.load()
    names = ("prob_ptr", "cand_ptr", "cand", "bounds", "start_pos", "best_fitness", "start_fitness", "best_pos", "best_rows",
             "round_history", "sweeps", "moves", "rounds", "pair_moves", "converged", "shortlist")

    def call(B=3, n_lists=12, max_slots=5, max_cand=20, max_sweeps=4, max_rounds=2, max_span=0, max_rank=2, wide=0, **null):
        a = {n: (None if n in null else P) for n in names}
        return lib.gnnpn_descend_pairs_shortlist_ragged_f64(
            B, a["prob_ptr"], n_lists, max_slots, max_cand, a["cand_ptr"], a["cand"], a["bounds"], a["start_pos"], max_sweeps, max_rounds,
            max_span, max_rank, wide, a["best_fitness"], a["start_fitness"], a["best_pos"], a["best_rows"], a["round_history"], a["sweeps"],
            a["moves"], a["rounds"], a["pair_moves"], a["converged"], a["shortlist"], None)
    for n in names:
        if n not in ("best_rows", "shortlist"):             # the two optional outputs
            for m in (0, 2):
                assert call(max_rank=m, **{n: True}) == -1 and b"null" in lib.gnnpn_last_error(), n
    for kw in ({"B": -1}, {"n_lists": -1}, {"max_slots": 0}, {"max_sweeps": -1}, {"max_rounds": -1}, {"max_span": -1}, {"max_rank": -1}):
        assert call(**kw) == -1 and b"bad argument" in lib.gnnpn_last_error(), kw
    for m in (0, 2):                                        # the lane form: its table, with or without a shortlist
        assert call(max_cand=0, max_rank=m) == _lib.E_UNSUP and b"max_cand" in lib.gnnpn_last_error()
        assert call(max_cand=6000, max_rank=m) == _lib.E_UNSUP and b"LDS" in lib.gnnpn_last_error()
    assert call(max_cand=4200, max_rank=4200) == _lib.E_UNSUP and b"LDS" in lib.gnnpn_last_error()      # the table fits, the buffers do not
    for kw in ({"max_slots": 5000, "max_rank": 0}, {"max_slots": 5000, "wide": 1, "max_cand": 0, "max_rank": 0}):   # the workgroup form
        assert call(**kw) == _lib.E_UNSUP and b"5000 slots" in lib.gnnpn_last_error(), kw
    assert call(max_slots=5000, max_rank=2) == _lib.E_UNSUP and b"5000 slots" in lib.gnnpn_last_error()
    assert call(max_slots=100, max_cand=0, max_rank=2) == _lib.E_UNSUP and b"max_cand" in lib.gnnpn_last_error()
    assert call(max_slots=100, max_cand=20000, max_rank=2) == _lib.E_UNSUP and b"LDS" in lib.gnnpn_last_error()     # the merit buffer
    assert call(max_slots=2000, max_cand=2000, max_rank=2000) == _lib.E_UNSUP and b"shortlists of 2000" in lib.gnnpn_last_error()
    assert call(B=0) == 0 and call(B=0, prob_ptr=True, cand=True, max_slots=5000) == 0          # an empty batch launches nothing
    assert "gnnpn_descend_pairs_shortlist_ragged_f64" in _lib.EXPORTS
    assert lib.gnnpn_abi_version() == 9


# ---- the Python layers --------------------------------------------------------------------------------------------------------------------

def _defaults(f):
    return {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}


def test_signatures_and_defaults():
    from gnnpn_sc_amd import ML2PN, ops
    from gnnpn_sc_amd.pipeline import ML2PNPipeline, descend_pairs_shortlist, descend_starts_pairs_shortlist
    sig = inspect.signature(ops.descend_pairs_shortlist_ragged)
    assert list(sig.parameters) == ["prob_ptr", "cand_ptr", "cand", "bounds", "start_pos", "max_sweeps", "max_rounds", "max_span", "max_rank",
                                    "max_slots", "max_cand", "wide", "return_shortlist"]
    assert _defaults(ops.descend_pairs_shortlist_ragged) == {"max_sweeps": 16, "max_rounds": 4, "max_span": 0, "max_rank": 0, "max_slots": None,
                                                             "max_cand": None, "wide": None, "return_shortlist": False}
    assert list(inspect.signature(ops.SearchTables.descend_pairs_shortlist).parameters) == ["self", "max_sweeps", "max_rounds", "max_span",
                                                                                           "max_rank", "wide"]
    assert _defaults(ops.SearchTables.descend_pairs_shortlist) == {"max_sweeps": 16, "max_rounds": 4, "max_span": 0, "max_rank": 0, "wide": None}
    sig = inspect.signature(descend_pairs_shortlist)
    assert list(sig.parameters) == ["services", "batch", "out", "max_sweeps", "max_rounds", "max_span", "max_rank", "reduct", "min_cost", "patches"]
    assert _defaults(descend_pairs_shortlist) == {"max_sweeps": 16, "max_rounds": 4, "max_span": 0, "max_rank": 0, "reduct": 0, "min_cost": None,
                                                  "patches": ()}
    assert list(inspect.signature(ML2PNPipeline.descend_pairs_shortlist).parameters)[1:] == list(sig.parameters)
    assert _defaults(ML2PNPipeline.descend_pairs_shortlist) == _defaults(descend_pairs_shortlist)
    sig = inspect.signature(descend_starts_pairs_shortlist)
    assert list(sig.parameters) == ["services", "batch", "starts", "max_sweeps", "pair_rounds", "pair_span", "pair_rank", "reduct", "min_cost",
                                    "patches"]
    assert _defaults(descend_starts_pairs_shortlist) == {"max_sweeps": 16, "pair_rounds": 4, "pair_span": 0, "pair_rank": 0, "reduct": 0,
                                                         "min_cost": None, "patches": ()}
    assert list(inspect.signature(ML2PNPipeline.descend_starts_pairs_shortlist).parameters)[1:] == list(sig.parameters)
    assert _defaults(ML2PNPipeline.descend_starts_pairs_shortlist) == _defaults(descend_starts_pairs_shortlist)
    # ML2PN.infer's parameter list is pinned by tests/test_search_tables_host.py, so the rank comes under a name of its own
    assert "pair_rank" not in inspect.signature(ML2PN.infer).parameters and "pair_rank" not in inspect.signature(ML2PN.infer_pairs_windowed).parameters
    assert list(inspect.signature(ML2PN.infer_pairs_shortlist).parameters) == [
        "dataset", "net", "low", "high", "n_per", "epoch", "device", "batch_size", "precision", "samples", "sample_seed", "descend",
        "all_starts", "pair_rounds", "pair_span", "pair_rank"]
    assert _defaults(ML2PN.infer_pairs_shortlist) == {"epoch": -1, "device": "cuda:0", "batch_size": 128, "precision": "f32", "samples": 1,
                                                      "sample_seed": None, "descend": 16, "all_starts": False, "pair_rounds": 4,
                                                      "pair_span": 0, "pair_rank": 0}


def test_wrappers_reject_host_tensors_and_negative_arguments():
    from gnnpn_sc_amd import ML2PN, ops
    from gnnpn_sc_amd.pipeline import ML2PNPipeline, descend_pairs_shortlist, descend_starts_pairs_shortlist
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)   # noqa: E731
    operands = (i32([0, 2, 3]), i32([0, 1, 2, 3]), f64(3, 4), f64(2, 4), i32([0, 0, 0]))
    for kw in ({"max_slots": 2, "max_cand": 2}, {"max_rank": 2}, {"max_span": 1, "max_rank": 1, "wide": True}, {"max_rank": 2, "return_shortlist": True},
               {"max_slots": 70, "max_cand": 2, "max_rank": 3}):
        with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
            ops.descend_pairs_shortlist_ragged(*operands, **kw)
    for kw in ({"max_rounds": -1}, {"max_span": -1}, {"max_sweeps": -1}, {"max_rank": -1}):
        with pytest.raises(ops.GnnpnError, match="inconsistent"):
            ops.descend_pairs_shortlist_ragged(*operands, **kw)
    with pytest.raises(ops.GnnpnError, match="inconsistent"):
        ops.descend_pairs_shortlist_ragged(*operands[:4], i32([0, 0]), max_rank=2)
    tabs = ops.SearchTables(prob_ptr=operands[0], cand_ptr=operands[1], cand=operands[2], bounds=operands[3], start_pos=operands[4],
                            max_slots=2, max_cand=2)
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        tabs.descend_pairs_shortlist(4, 2, 1, 2)

    class Svc:
        cat_ptr, qos = i32([0, 2, 4, 6]), f64(6, 4)

    class Batch:
        n_problems = 2
        x, seg_ptr = torch.zeros(6, 7), i32([0, 3, 6])
        local_bounds, global_bounds = f64(2, 3, 4), f64(2, 4)
    out = {"actions": torch.zeros(2, 3, 8)}
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        descend_pairs_shortlist(Svc, Batch, out, max_rank=2)
    for f in (descend_pairs_shortlist, lambda *a, **k: ML2PNPipeline.descend_pairs_shortlist(None, *a, **k)):
        for kw in ({"max_span": -1}, {"max_rank": -1}, {"max_rounds": -1}):
            with pytest.raises(ops.GnnpnError, match="the span and the rank must be >= 0"):
                f(Svc, Batch, out, **kw)
    starts = torch.zeros(2, 3, 3, 8)
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        descend_starts_pairs_shortlist(Svc, Batch, starts, pair_rank=2)
    for f in (descend_starts_pairs_shortlist, lambda *a, **k: ML2PNPipeline.descend_starts_pairs_shortlist(None, *a, **k)):
        for kw in ({"pair_span": -1}, {"pair_rank": -1}, {"pair_rounds": -1}):
            with pytest.raises(ops.GnnpnError, match="the span and the rank must be >= 0"):
                f(Svc, Batch, starts, **kw)
    for kw in ({"pair_rank": -1}, {"pair_span": -1}, {"pair_rank": 2, "pair_rounds": 0}, {"pair_rank": 2, "descend": None}, {"pair_rank": None}):
        with pytest.raises(ValueError, match="pair_rank"):
            ML2PN.infer_pairs_shortlist("QWS", None, None, None, 3, **kw)


def test_main_cli_refuses_top_before_any_file_is_read(capsys, tmp_path, monkeypatch):
    import main as cli
    monkeypatch.chdir(tmp_path)                            # no ./data here: reading a file would raise, not return 1
    base = ["main.py", "QWS", "ML+2PN", "-1", "--infer"]
    assert cli.main(base + ["--descend", "--top=2"]) == 1                                        # without --pairs
    assert cli.main(base + ["--descend", "--pairs", "--top=-1"]) == 1                            # a negative number
    assert cli.main(base + ["--descend", "--pairs", "--top"]) == 1                               # no number
    assert cli.main(base + ["--descend", "--pairs", "--span=2", "--top=x"]) == 1
    assert capsys.readouterr().out.count("--top=M: needs --pairs[=ROUNDS] and M >= 0") == 4
    assert cli.main(base + ["--descend", "--pairs", "--top=2", "--woa"]) == 1
    assert cli.main(base + ["--descend", "--pairs", "--span=2", "--top=2", "--woa"]) == 1
    assert capsys.readouterr().out.count("--top=M: not with --woa") == 2
    assert cli.main(base + ["--pairs", "--top=2"]) == 1                                          # --pairs' own refusal comes first
    assert "--pairs[=ROUNDS]: needs --descend" in capsys.readouterr().out
    assert cli.main(base + ["--descend", "--pairs", "--top=2", "--all-starts"]) == 1             # --all-starts' own refusal
    assert "--all-starts: needs --samples=N" in capsys.readouterr().out
    assert cli.main(base + ["--descend", "--pairs", "--span=2", "--samples=3", "--all-starts"]) == 1    # the span alone still refuses it
    assert cli.main(base + ["--descend", "--pairs", "--span=2", "--woa"]) == 1
    assert capsys.readouterr().out.count("--span=N: not with --all-starts or --woa") == 2
    for more in (["--top=0"], ["--top=2", "--span=1"], ["--top=2", "--span=1", "--samples=3", "--all-starts"]):
        with pytest.raises(FileNotFoundError):
            cli.main(base + ["--descend", "--pairs"] + more)                                     # accepted: goes on to the data
