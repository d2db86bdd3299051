"""-m "not gpu": what the descent entries refuse on the host, where no launch follows — the sizes one past the edge of a CU's LDS of
tests/test_gpu_lds_boundary.py (its formulas, its messages), each with GNNPN_E_UNSUP and the byte count, and the max_cand >= 1 rule
of every entry and form with its own code and sentence."""
import pytest

import test_gpu_lds_boundary as edge

P = 1 << 20          # a pointer that is never read: every call here is refused first


def _call(build, form, max_slots, max_cand, rank=0, lane_only=False):
    """The entry of ``build`` with two problems of never-read operands; (return code, message)."""
    from gnnpn_sc_amd import _lib
    lib = _lib.load()
    head = (2, P, 6, max_slots, max_cand, P, P, P, P, 3)
    wide = int(form == "wide")
    pair_out = (P,) * 10
    if build == "one_swap":
        rc = lib.gnnpn_descend_ragged_f64(*head, wide, P, P, P, P, P, P, P, None)
    elif build == "tabu":
        rc = lib.gnnpn_descend_tabu_ragged_f64(*head, 4, 2, wide, *(P,) * 11, None)
    elif build == "shortlist":
        rc = lib.gnnpn_descend_pairs_shortlist_ragged_f64(*head, 1, 2, rank, wide, *pair_out, None, None)
    elif lane_only:
        rc = lib.gnnpn_descend_pairs_ragged_f64(*head, 1, *pair_out, None)
    else:
        rc = lib.gnnpn_descend_pairs_windowed_ragged_f64(*head, 1, 0, wide, *pair_out, None)
    return rc, lib.gnnpn_last_error().decode()


@pytest.mark.parametrize("build,form,size", edge.CASES)
def test_one_size_past_the_edge_is_refused_with_its_byte_count(build, form, size):
    from gnnpn_sc_amd import _lib
    _table, max_slots, max_cand, rank, (up_slots, up_cand) = edge._case(build, form, size)
    nbytes = edge.BYTES[build][0][form]
    assert nbytes(max_slots, max_cand, rank) <= edge.LIMIT < nbytes(up_slots, up_cand, rank)
    rc, message = _call(build, form, up_slots, up_cand, rank, lane_only=form == "lane")
    assert rc == _lib.E_UNSUP
    assert message == edge._message(build, form, nbytes(up_slots, up_cand, rank), up_slots, up_cand, rank)


def test_far_past_the_edge_the_count_is_still_the_layouts():
    """Sizes whose byte count no int holds: the host's arithmetic is size_t."""
    from gnnpn_sc_amd import _lib
    n = 2 ** 31 - 1
    for build, form, T, rank in (("one_swap", "lane", 3, 0), ("tabu", "lane", 3, 0), ("shortlist", "lane", 64, 5), ("shortlist", "wide", 70, n),
                                 ("tabu", "wide", 70, 0), ("one_swap", "wide", n, 0), ("pairs", "wide", n, 0)):
        m = min(rank, n)
        rc, message = _call(build, form, T, n, rank)
        assert rc == _lib.E_UNSUP and message == edge._message(build, form, edge.BYTES[build][0][form](T, n, m), T, n, m), (build, form)


def test_max_cand_below_one_by_entry_and_form():
    from gnnpn_sc_amd import _lib
    sizes = " (it sizes {} in LDS)"
    assert _call("one_swap", "lane", 3, 0) == (-1, "descend_ragged: max_cand must be >= 1 for the lane form")
    assert _call("pairs", "lane", 3, 0, lane_only=True) == (_lib.E_UNSUP, "descend_pairs_ragged: max_cand must be >= 1" + sizes.format("the table"))
    assert _call("pairs", "lane", 3, 0) == (_lib.E_UNSUP, "descend_pairs_windowed_ragged: max_cand must be >= 1" + sizes.format("the table"))
    for form in ("lane", "wide"):
        assert _call("shortlist", form, 3, 0, 2) == (_lib.E_UNSUP, "descend_pairs_shortlist_ragged: max_cand must be >= 1" +
                                                   sizes.format("the merit buffer, and in the lane form the table,"))
        assert _call("tabu", form, 3, -1) == (_lib.E_UNSUP, "descend_tabu_ragged: max_cand must be >= 1" +
                                              sizes.format("the tabu table, and in the lane form the candidate table,"))
    assert _call("shortlist", "lane", 3, 0, 0)[1] == "descend_pairs_shortlist_ragged: max_cand must be >= 1" + sizes.format("the table")      # no rank: the pair build
    rc, message = _call("pairs", "lane", 65, 10, lane_only=True)
    assert rc == _lib.E_UNSUP and message.startswith("descend_pairs_ragged: 65 slots: the pair sweep has the lane form only")
