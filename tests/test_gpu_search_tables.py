"""-m gpu: ops.SearchTables' methods return exactly what the search wrappers return on the unpacked operands, and the selection
(ops.descend_select) carries a pair descent's round_history and counters: the winner's rows of the per-row dict.  ``torch.equal``."""
import numpy as np
import pytest
import torch

import descent_reference as ref
import multistart_reference as mref
from test_gpu_descend import _tables

pytestmark = pytest.mark.gpu


def _search_tables(dev, tables):
    """[(cats, bounds, start | None)] as a SearchTables on the device (len_init: the whole list)."""
    from gnnpn_sc_amd import ops
    prob_ptr, cand_ptr, flat, bounds, start = ref.pack(tables)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev)      # noqa: E731
    return ops.SearchTables(prob_ptr=t(prob_ptr, torch.int32), n_slots=t(np.diff(prob_ptr), torch.int32), cand_ptr=t(cand_ptr, torch.int32),
                            len_init=t(np.diff(cand_ptr), torch.int32), cand=t(flat, torch.float64).reshape(-1, 4),
                            start_pos=t(start, torch.int32), bounds=t(bounds, torch.float64),
                            max_slots=max(len(c) for c, _b, _s in tables), max_cand=max(sum(map(len, c)) for c, _b, _s in tables))


def _same(got, want):
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


def test_methods_equal_the_wrappers_on_the_unpacked_operands(dev):
    from gnnpn_sc_amd import ops
    tables = _tables(1500, (1, 3, 10), 4)
    assert len(tables) == 12 and [s is None for _c, _b, s in tables].count(True) == 3
    tabs = _search_tables(dev, tables)
    five = (tabs["prob_ptr"], tabs["cand_ptr"], tabs["cand"], tabs["bounds"], tabs["start_pos"])
    sizes = {"max_slots": tabs["max_slots"], "max_cand": tabs["max_cand"]}
    one = ops.descend_ragged(*five, 16, **sizes)
    _same(tabs.descend(16), one)
    _same(tabs.descend(16, wide=True), ops.descend_ragged(*five, 16, wide=True, **sizes))
    _same(tabs.descend_pairs(16, 4), ops.descend_pairs_ragged(*five, 16, 4, **sizes))
    seeds = torch.arange(900, 900 + len(tables), dtype=torch.int64, device=dev)
    want = ops.eswoa_ragged(five[0], five[1], tabs["len_init"], *five[2:], 8, 5, seeds, **sizes)
    got = tabs.eswoa(8, 5, seeds)
    assert len(got) == len(want) == 5 and all(g.dtype == w.dtype and torch.equal(g, w) for g, w in zip(got, want))
    # flat: the mask gather, and ES-WOA from it is ES-WOA from those start positions
    slots = torch.arange(tabs["max_slots"], device=dev)[None, :] < tabs["n_slots"][:, None]
    flat = tabs.flat(one["best_pos"])
    assert flat.dtype == torch.int32 and flat.shape == tabs["start_pos"].shape and torch.equal(flat, one["best_pos"][slots].contiguous())
    want = ops.eswoa_ragged(five[0], five[1], tabs["len_init"], five[2], five[3], flat, 8, 5, seeds, **sizes)
    assert all(torch.equal(g, w) for g, w in zip(tabs.eswoa(8, 5, seeds, flat), want))
    assert one["moves"].any()          # (descent moved somewhere: the two ES-WOA runs differ in their start)


def test_descend_select_carries_the_pair_descent_fields(dev):
    from gnnpn_sc_amd import ops
    R = 3
    reps = mref.replica_tables(1602, (1, 7, 9), 4, R)          # (by the reference: two problems go to replica 1, one with other counters)
    B = len(reps)
    tabs = _search_tables(dev, [tab for rep in reps for tab in rep])          # row q = b * R + r
    per_row = tabs.descend_pairs(16, 4)
    keys = list(per_row)
    actions = torch.arange(B * R * 2 * 8, dtype=torch.float32, device=dev).view(B, R, 2, 8)
    win = ops.descend_select(per_row, actions, tabs["n_slots"])
    assert list(per_row) == keys and "history" not in win and "history" not in per_row
    q = torch.arange(B, device=dev) * R + win["start_index"].long()
    for k in ("round_history", "rounds", "pair_moves", "converged", "best_fitness", "start_fitness", "best_pos", "best_rows", "sweeps", "moves"):
        assert win[k].dtype == per_row[k].dtype and torch.equal(win[k], per_row[k][q]), k
    assert torch.equal(win["n_slots"], tabs["n_slots"][q]) and torch.equal(win["actions"], actions.view(B * R, 2, 8)[q])
    # the winner by the selection rule, and not always replica 0 (the gather has something to get wrong)
    fit = per_row["best_fitness"].view(B, R).cpu().tolist()
    assert win["start_index"].cpu().tolist() == [mref.select([{"best_fitness": f} for f in row]) for row in fit]
    assert win["start_index"].any() and not torch.equal(win["rounds"], per_row["rounds"].view(B, R)[:, 0])
    # a one-swap dict goes through as before: history, and nothing gathered beside the seven
    plain = ops.descend_select(tabs.descend(16), actions, tabs["n_slots"])
    assert set(plain) == {"best_fitness", "start_fitness", "best_pos", "best_rows", "history", "sweeps", "moves", "start_index", "actions", "n_slots"}
