"""-m "not gpu": ops.SearchTables (what woa_candidates returns) is a dict whose methods reach the search wrappers' own refusals, the
selection carries a pair descent's round_history, and the public names of the search stack keep their parameter lists."""
import inspect

import pytest
import torch


def _host_tables():
    from gnnpn_sc_amd import ops
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)   # noqa: E731
    return ops.SearchTables(prob_ptr=i32([0, 2, 3]), n_slots=i32([2, 1]), cand_ptr=i32([0, 1, 2, 3]), len_init=i32([1, 1, 1]), cand=f64(3, 4),
                            start_pos=i32([0, 0, 0]), bounds=f64(2, 4), status=i32([0, 0]), max_slots=2, max_cand=2)


def test_search_tables_is_a_dict_and_its_methods_reach_the_wrappers():
    from gnnpn_sc_amd import ops
    tabs = _host_tables()
    assert isinstance(tabs, dict) and issubclass(ops.SearchTables, dict)
    assert tabs["max_slots"] == 2 and "replicas" not in tabs and list(tabs)[:2] == ["prob_ptr", "n_slots"]
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        tabs.descend()
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        tabs.descend_pairs()
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        tabs.eswoa(4, 3, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ops.GnnpnError, match="descend_pairs_ragged: inconsistent"):
        tabs.descend_pairs(16, -1)
    # flat: a problem's first n_slots entries, problem after problem (host tensors will do: it launches nothing of the library's)
    assert tabs.flat(torch.tensor([[5, 6], [7, 9]], dtype=torch.int32)).tolist() == [5, 6, 7]


def test_descend_select_takes_a_round_history():
    from gnnpn_sc_amd import ops
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)   # noqa: E731
    res = {"best_fitness": f64(4), "start_fitness": f64(4), "best_pos": torch.zeros(4, 3, dtype=torch.int32), "best_rows": f64(4, 3, 4),
           "sweeps": i32([1] * 4), "moves": i32([0] * 4), "round_history": f64(4, 4), "rounds": i32([1] * 4), "pair_moves": i32([0] * 4),
           "converged": i32([1] * 4)}
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):
        ops.descend_select(res, torch.zeros(2, 2, 3, 8), i32([3] * 4))
    with pytest.raises(ops.GnnpnError, match="2 x 3 rows"):
        ops.descend_select(res, torch.zeros(2, 3, 3, 8), i32([3] * 4))


def test_public_signatures_of_the_search_stack():
    from gnnpn_sc_amd import ML2PN, WOA, ops
    from gnnpn_sc_amd import pipeline as pl
    params = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    defaults = lambda f: {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}      # noqa: E731
    tables = ["cat_ptr", "qos", "x", "seg_ptr", "local_bounds", "global_bounds"]
    assert params(ops.woa_candidates) == tables + ["actions", "reduct", "patches", "check_status"]
    assert params(ops.woa_candidates_replicas) == tables + ["actions_all", "reduct", "patches", "check_status"]
    assert defaults(ops.woa_candidates) == defaults(ops.woa_candidates_replicas) == {"reduct": 0, "patches": (), "check_status": True}
    assert params(ops.eswoa_ragged) == ["prob_ptr", "cand_ptr", "len_init", "cand", "bounds", "start_pos", "pop", "max_iter", "seeds",
                                        "max_slots", "max_cand", "wide"]
    assert defaults(ops.eswoa_ragged) == {"max_slots": None, "max_cand": None, "wide": None}
    assert params(ops.descend_ragged) == ["prob_ptr", "cand_ptr", "cand", "bounds", "start_pos", "max_sweeps", "max_slots", "max_cand", "wide"]
    assert defaults(ops.descend_ragged) == {"max_sweeps": 16, "max_slots": None, "max_cand": None, "wide": None}
    assert params(ops.descend_pairs_ragged) == ["prob_ptr", "cand_ptr", "cand", "bounds", "start_pos", "max_sweeps", "max_rounds", "max_slots",
                                                "max_cand"]
    assert defaults(ops.descend_pairs_ragged) == {"max_sweeps": 16, "max_rounds": 4, "max_slots": None, "max_cand": None}
    assert params(ops.descend_select) == ["res", "actions_all", "n_slots"] and defaults(ops.descend_select) == {}
    assert params(ops.SearchTables.descend) == ["self", "max_sweeps", "wide"]
    assert params(ops.SearchTables.descend_pairs) == ["self", "max_sweeps", "max_rounds"]
    assert params(ops.SearchTables.eswoa) == ["self", "pop", "max_iter", "seeds", "start_pos", "wide"]
    assert params(ops.SearchTables.flat) == ["self", "best_pos"]
    assert defaults(ops.SearchTables.descend) == {"max_sweeps": 16, "wide": None}
    assert defaults(ops.SearchTables.descend_pairs) == {"max_sweeps": 16, "max_rounds": 4}
    assert defaults(ops.SearchTables.eswoa) == {"start_pos": None, "wide": None}

    tail = {"reduct": 0, "min_cost": None, "patches": ()}
    assert params(pl.descend) == ["services", "batch", "out", "max_sweeps", "reduct", "min_cost", "patches"]
    assert defaults(pl.descend) == {"max_sweeps": 16, **tail}
    assert params(pl.descend_pairs) == ["services", "batch", "out", "max_sweeps", "max_rounds", "reduct", "min_cost", "patches"]
    assert defaults(pl.descend_pairs) == {"max_sweeps": 16, "max_rounds": 4, **tail}
    assert params(pl.descend_starts) == ["services", "batch", "starts", "max_sweeps", "reduct", "min_cost", "patches"]
    assert defaults(pl.descend_starts) == {"max_sweeps": 16, **tail}
    assert params(pl.descend_starts_pairs) == ["services", "batch", "starts", "max_sweeps", "pair_rounds", "reduct", "min_cost", "patches"]
    assert defaults(pl.descend_starts_pairs) == {"max_sweeps": 16, "pair_rounds": 4, **tail}
    assert params(pl.refine) == ["services", "batch", "out", "popSize", "MAX_Iter", "reduct", "seeds", "min_cost", "patches", "descend",
                                 "pair_rounds"]
    assert defaults(pl.refine) == {"reduct": 0, "seeds": None, "min_cost": None, "patches": (), "descend": 0, "pair_rounds": 0}
    assert params(pl._descend_tables) == ["tabs", "max_sweeps", "pair_rounds"] and defaults(pl._descend_tables) == {"pair_rounds": None}
    for name in ("descend", "descend_pairs", "descend_starts", "descend_starts_pairs"):
        method, function = getattr(pl.ML2PNPipeline, name), getattr(pl, name)
        assert params(method) == ["self"] + params(function) and defaults(method) == defaults(function), name
    assert params(pl.ML2PNPipeline.refine) == ["self"] + params(pl.refine)[:-2]          # deliberately without descend / pair_rounds
    assert defaults(pl.ML2PNPipeline.refine) == {"reduct": 0, "seeds": None, "min_cost": None, "patches": ()}

    assert params(ML2PN.infer) == ["dataset", "net", "low", "high", "n_per", "epoch", "device", "batch_size", "precision", "woa", "samples",
                                   "sample_seed", "descend", "all_starts", "pair_rounds"]
    assert defaults(ML2PN.infer) == {"epoch": -1, "device": "cuda:0", "batch_size": 128, "precision": "f32", "woa": None, "samples": 1,
                                     "sample_seed": None, "descend": None, "all_starts": False, "pair_rounds": None}
    assert params(ML2PN.refine_test_quarter) == ["dataset", "ds", "pipe", "svc", "actions", "popSize", "MAX_Iter", "reduct", "seed", "descend",
                                                 "starts", "pair_rounds"]
    assert defaults(ML2PN.refine_test_quarter) == {"seed": None, "descend": None, "starts": None, "pair_rounds": None}
    assert params(WOA.write_ml2pn_woa) == ["dataset", "quality", "per_problem", "first", "times", "name", "extra"]
    assert defaults(WOA.write_ml2pn_woa) == {"times": 0, "name": "ML+2PN+WOA.txt", "extra": None}
