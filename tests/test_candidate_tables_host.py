"""The conditions that tests/test_gpu_candidate_tables.py relies on, checked on the host path alone (loadDataOther + WOA._prepare
over the problems of tests/candidate_tables_reference.py): were the generator to drift, this fails before anything is compared on
the device.  The cap and the floors below are conditions on the inputs, not measurements."""
import numpy as np
import pytest

import candidate_tables_reference as ctr

PICK_SEED = 11          # the GPU tests' picks: make_picks(ds, reduct, a_T, PICK_SEED + replica)


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    import gnnpn_sc_amd.synth as synth
    tmp = tmp_path_factory.mktemp("candidate_tables")
    synth.write_dataset(str(tmp), "QWS", ctr.make_dataset())
    return str(tmp)


def test_the_task_counts_straddle_the_passes():
    ds = ctr.make_dataset()
    counts = ctr.task_counts(ds)
    assert set(ctr.TASK_COUNTS) <= set(counts) and set(ctr.TASK_COUNTS) >= {1, 3, 63, 64, 65, 127, 128, 129, 130, 200}
    assert len(ds["nodefeatures"]) == 4 * len(counts)
    repeated = [nodes for nodes in ctr.problems_of(ds) if len({n[:-6].index(1) for n in nodes[1:]}) < len(nodes) - 1]
    assert len(repeated) >= len(counts) // 2                       # categories are drawn with replacement
    empty = [b for b in range(len(counts)) if not any(ctr.slot_lists(ds, 0, only=b)[0])]
    assert any(counts[b] > 64 and 0 < b < len(counts) - 1 for b in empty)      # a large problem without lists, inside the batch
    assert ds is ctr.make_dataset() and ds == ctr.make_dataset.__wrapped__()   # deterministic from the seed


@pytest.mark.parametrize("reduct", ctr.REDUCTS)
def test_conditions_on_the_problems_and_their_picks(root, reduct):
    ds = ctr.make_dataset()
    acts = ctr.make_picks(ds, reduct, 200, PICK_SEED)
    host, sols, _mins = ctr.host_tables(root, acts, reduct)
    lay = ctr.layout(host)
    assert None not in lay["status"]
    ok = [b for b, st in enumerate(lay["status"]) if st == ctr.STATUS_OK]
    n_lists = {b: len(host[b][0]) for b in ok}
    # (a) at most one quarter of the test problems raise on the host path
    assert 4 * (len(host) - len(ok)) <= len(host)
    # (b) more than 64 non-empty lists at least twice, more than 128 at least once
    assert sum(1 for n in n_lists.values() if n > 64) >= 2 and sum(1 for n in n_lists.values() if n > 128) >= 1
    # (c) in a problem of more than 64 slots: an empty list before a non-empty one inside the second 64-slot pass, and an empty list
    # of the first pass before a non-empty one of the second
    inside = across = False
    lists_all = ctr.slot_lists(ds, reduct, ctr.pick_sets(acts))
    for b in ok:
        full = [bool(lst) for lst in lists_all[b]]
        assert sum(full) == n_lists[b]
        if len(full) <= 64:
            continue
        second = full[64:128]
        inside |= any(not second[i] and any(second[i + 1:]) for i in range(len(second)))
        across |= not all(full[:64]) and any(second)
    assert inside and across
    # (d) seeded and unseeded problems among those with more than 64 lists
    big = [b for b in ok if n_lists[b] > 64]
    assert any(host[b][2] is not None for b in big) and any(host[b][2] is None for b in big)
    # (e) a foreign pick (appended: start == len_init) in a slot with index >= 64; one before it too
    foreign = [j for b in big if host[b][2] is not None for j, (n, s) in enumerate(zip(host[b][1], host[b][2])) if s == n]
    assert any(j >= 64 for j in foreign) and any(j < 64 for j in foreign)
    # both status words, each next to problems that did not raise; a mismatch in a problem of more than 64 lists, in both directions
    for word in (ctr.STATUS_ROWS_MISMATCH, ctr.STATUS_NO_SLOTS):
        assert any(st == word and lay["status"][b - 1] == lay["status"][b + 1] == ctr.STATUS_OK
                   for b, st in enumerate(lay["status"][:-1]) if b > 0)
    full_counts = [sum(1 for lst in lists if lst) for lists in lists_all]
    off = {len(sols[b]) - full_counts[b] for b, st in enumerate(lay["status"]) if st == ctr.STATUS_ROWS_MISMATCH and full_counts[b] > 64}
    assert off == {1, -1}
    if reduct:      # the pick skip: a picked member at a front position other than 0, and lists that the picks change on either side of slot 64
        assert any(0 < s < n for b in ok if host[b][2] is not None for n, s in zip(host[b][1], host[b][2]))
        bare = ctr.slot_lists(ds, reduct)
        changed = [s for b in big for s, (with_picks, without) in enumerate(zip(lists_all[b], bare[b])) if with_picks != without]
        assert any(s >= 64 for s in changed) and any(s < 64 for s in changed)


@pytest.mark.parametrize("a_T", [65, 130, 1024])
def test_conditions_at_the_other_row_counts(root, a_T):
    """More than 64 real rows where the row count allows a problem of more than 64 lists its rows; at 65 rows the one problem that
    keeps 65 rows of more is mismatched, the other large ones are unseeded."""
    ds = ctr.make_dataset()
    acts = ctr.make_picks(ds, 0, a_T, PICK_SEED)
    host, sols, _mins = ctr.host_tables(root, acts, 0)
    lay = ctr.layout(host)
    assert None not in lay["status"] and 4 * sum(1 for st in lay["status"] if st) <= len(host)
    assert max(len(s) for s in sols) > 64
    seeded_big = [b for b, h in enumerate(host) if not isinstance(h, Exception) and h[2] is not None and len(h[0]) > 64]
    assert bool(seeded_big) == (a_T > 65)
    if a_T == 130:
        assert any(len(host[b][0]) > 64 and host[b][2] is None for b in range(len(host)) if not isinstance(host[b], Exception))


@pytest.mark.parametrize("R", [3])
def test_conditions_on_the_replicas(root, R):
    """The replicas' picks differ, and exactly one replica is mismatched where the others are not, in a problem of more than 64 lists."""
    ds = ctr.make_dataset()
    lays = []
    for r in range(R):
        acts = ctr.make_picks(ds, 0.55, 200, PICK_SEED + r, mismatch=r == 1)
        lays.append(ctr.layout(ctr.host_tables(root, acts, 0.55)[0])["status"])
    only_one = [b for b in range(len(lays[0])) if [lay[b] for lay in lays] == [0, ctr.STATUS_ROWS_MISMATCH, 0]]
    assert only_one
    counts = [sum(1 for lst in lists if lst) for lists in ctr.slot_lists(ds, 0.55)]
    assert any(counts[b] > 64 for b in only_one)


def test_the_search_batch_has_problems_beyond_64_and_128_slots(root, tmp_path):
    import gnnpn_sc_amd.synth as synth
    ds = ctr.make_dataset(ctr.SEARCH_SEED, ctr.SEARCH_COUNTS, ())
    synth.write_dataset(str(tmp_path), "QWS", ds)
    acts = ctr.make_picks(ds, 0, 200, PICK_SEED, mismatch=False)
    host, _s, _m = ctr.host_tables(str(tmp_path), acts, 0)
    sizes = [len(h[0]) for h in host if not isinstance(h, Exception)]
    assert len(sizes) == len(host) and min(sizes) <= 3 and sum(1 for n in sizes if n > 64) >= 2 and max(sizes) > 128
    assert any(h[2] is None for h in host) and any(h[2] is not None and len(h[0]) > 64 for h in host)


def test_protected_pick_is_what_adds_skips_by(root):
    """The patch cases with reduct != 0: a pick whose slot's list differs between the pick set as it is and the pick set with the
    patched row in its place — the lists must follow the unpatched set."""
    ds = ctr.make_dataset()
    acts = ctr.make_picks(ds, 0.55, 200, PICK_SEED)
    counts = ctr.task_counts(ds)
    for b in (counts.index(40), counts.index(150)):
        found = ctr.protected_pick(ds, b, 0.55, acts, 0, 0.12345)
        assert found is not None
        planted, j, key = found
        assert key == ctr.rounded(planted[b, j]) and np.isfinite(key).all()
        assert (np.delete(planted[b], j, 0) == np.delete(acts[b], j, 0)).all() and (np.delete(planted, b, 0) == np.delete(acts, b, 0)).all()
