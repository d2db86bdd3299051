"""-m "not gpu": the chunk planner of the fused score product + candidate reduction (gnnpn-sc_amd/score_plan.py): every category
in exactly one chunk, chunks contiguous, balance within one category's size; where the kernel applies; the chunk count asked of the planner; and the entry point's
refusals, which return before any launch."""
import ctypes

import numpy as np
import pytest

from gnnpn_sc_amd import score_plan


def _tables():
    rng = np.random.default_rng(0)
    yield np.concatenate([[0], np.cumsum([1, 15, 16, 17, 53, 64, 256])])
    yield np.concatenate([[0], np.cumsum(rng.integers(30, 80, 47))])                 # the QWS shape: 47 categories of about 53
    yield np.concatenate([[0], np.cumsum(rng.integers(16, 25, 200))])
    yield np.concatenate([[0], np.cumsum([256] * 9)])
    yield np.concatenate([[0], np.cumsum([20, 0, 0, 40, 17, 0, 90])])                # empty categories


@pytest.mark.parametrize("n_chunks", [1, 2, 3, 7, 16, 47, 64, 300])
def test_chunks_partition_the_categories_and_balance(n_chunks):
    for cat in _tables():
        T, S = len(cat) - 1, int(cat[-1])
        bounds = score_plan.chunk_bounds(cat, n_chunks)
        assert bounds.dtype == np.int32 and len(bounds) == n_chunks + 1
        assert bounds[0] == 0 and bounds[-1] == T and (np.diff(bounds) >= 0).all()   # contiguous runs: every category in exactly one
        owner = np.concatenate([np.full(bounds[k + 1] - bounds[k], k) for k in range(n_chunks)])
        assert len(owner) == T and (np.diff(owner) >= 0).all()
        services = np.diff(cat[bounds])
        assert services.sum() == S
        assert np.abs(services - S / n_chunks).max() <= np.diff(cat).max()            # within one category's size of the ideal share


def test_plan_words_and_fit():
    cat = np.concatenate([[0], np.cumsum([1, 15, 16, 17, 53, 64, 256])])
    plan = score_plan.plan_chunks(cat, 3)
    assert plan.fits() and plan.n_chunks == 3 and plan.n_tiles == 1 + 1 + 1 + 2 + 4 + 4 + 16
    w = plan.words
    assert w.dtype == np.int32 and list(w[:4]) == [7, 3, 29, 422] and len(w) == 4 + 8 + 8 + 4 + 3 * 8
    assert list(w[4:12]) == list(cat) and list(w[12:20]) == [0, 1, 2, 3, 5, 9, 13, 29] and list(w[20:24]) == list(plan.chunk_ptr) == [0, 6, 6, 7]
    assert w[24:].reshape(3, 8).tolist() == [[0, 6, 0, 13, 0, 166, 0, 0], [6, 6, 13, 0, 166, 166, 0, 0], [6, 7, 13, 16, 166, 422, 0, 0]]
    # a chunk count whose chunks would not fit a workgroup is raised until they do
    big = np.concatenate([[0], np.cumsum([256] * 9)])                                # 16 tiles each: one per chunk
    plan = score_plan.plan_chunks(big, 2)
    assert plan.fits() and plan.n_chunks > 2 and plan.chunk_tiles().max() <= score_plan.MAX_TILES
    assert score_plan.plan_chunks(np.array([0, 300, 600]), 2) is None                # a category above the cap: no plan
    many = score_plan.plan_chunks(np.arange(0, 16 * 40 + 1, 16), 1)                  # 40 categories of one tile: at most 16 per chunk
    assert many.fits() and np.diff(many.chunk_ptr).max() <= score_plan.MAX_CHUNK_CATEGORIES


def test_where_the_fused_kernel_applies():
    qws = np.concatenate([[0], np.cumsum([53] * 47)])
    assert score_plan.applies(qws, 128, 5) and score_plan.applies(qws, 128, 16)
    assert not score_plan.applies(qws, 64, 5) and not score_plan.applies(qws, 128, 17) and not score_plan.applies(qws, 128, 0)
    assert not score_plan.applies(np.arange(0, 5001, 5), 128, 5)                     # the 1000-task shape: 5 services per category
    assert not score_plan.applies(np.arange(0, 20001, 10), 128, 5)                   # the 2000-task shape: 10
    assert not score_plan.applies(np.array([0, 257, 600]), 128, 5)                   # above the cap
    assert score_plan.applies(np.array([0, 256, 300]), 128, 5)


def test_chunk_count_rule():
    """About one workgroup per CU over the tiles of 16 problems: n_cu // ceil(B / 16), at least 1, at most one chunk per category."""
    assert score_plan.chunk_count(47, 256, 256) == 16                                # 16 tiles of problems on 256 CUs
    assert score_plan.chunk_count(47, 257, 256) == 15 and score_plan.chunk_count(47, 272, 256) == 15      # a ragged 17th tile counts
    assert score_plan.chunk_count(47, 16, 256) == 47 and score_plan.chunk_count(47, 1, 256) == 47         # capped by the categories
    assert score_plan.chunk_count(300, 16, 256) == 256 and score_plan.chunk_count(300, 17, 256) == 128
    assert score_plan.chunk_count(47, 16 * 256, 256) == 1 and score_plan.chunk_count(47, 100000, 256) == 1    # never below one
    assert score_plan.chunk_count(47, 0, 256) == 47 and score_plan.chunk_count(1, 256, 256) == 1          # an empty batch; one category
    for T in (1, 7, 47, 300):
        for B in (0, 1, 15, 16, 17, 255, 256, 4096, 5000):
            for n_cu in (1, 64, 256, 304):
                n = score_plan.chunk_count(T, B, n_cu)
                tiles = max(1, -(-B // 16))
                assert 1 <= n <= T and isinstance(n, int)
                assert n == T or n * tiles <= max(n_cu, tiles)                       # below the cap: the grid stays within the CUs
                assert n == T or (n + 1) * tiles > n_cu                              # ... and one more chunk would leave them


def test_unfused_switch(monkeypatch):
    monkeypatch.delenv("GNNPN_UNFUSED_FRONT", raising=False)
    assert not score_plan.unfused_front()
    monkeypatch.setenv("GNNPN_UNFUSED_FRONT", "1")
    assert score_plan.unfused_front()


def test_entry_refuses_before_any_launch():
    """The plan is checked on the host and the unsupported shapes are reported: no device is touched."""
    from gnnpn_sc_amd import _lib
    lib = _lib.load()
    plan = score_plan.plan_chunks(np.concatenate([[0], np.cumsum([20, 40, 30])]), 2)
    words = np.ascontiguousarray(plan.words)
    p = words.ctypes.data_as(ctypes.c_void_p)
    nil = ctypes.c_void_p(16)

    def call(words_p, n_words, hidden, n_per):
        return lib.gnnpn_score_select_f32(nil, 128, nil, words_p, nil, n_words, nil, nil, nil, nil, nil, 90, nil, nil, 4, hidden, n_per, None)
    assert call(p, len(words), 64, 5) == _lib.E_UNSUP and b"hidden" in lib.gnnpn_last_error()
    assert call(p, len(words), 128, 17) == _lib.E_UNSUP
    assert call(p, len(words) - 1, 128, 5) == -1 and b"does not hold" in lib.gnnpn_last_error()
    assert call(None, 0, 128, 5) == -1 and b"null plan" in lib.gnnpn_last_error()
    bad = words.copy()
    bad[4 + 2 * (plan.n_categories + 1) + plan.n_chunks] -= 1                        # chunk_ptr's last entry: no longer T
    assert call(bad.ctypes.data_as(ctypes.c_void_p), len(bad), 128, 5) == -1 and b"do not span" in lib.gnnpn_last_error()
    wide = score_plan.ScorePlan(np.array([0, 300]), np.array([0, 1])).words
    assert call(wide.ctypes.data_as(ctypes.c_void_p), len(wide), 128, 5) == _lib.E_UNSUP and b"300 services" in lib.gnnpn_last_error()
    # a good plan with a null operand stops at the operand check (every call above and this one returns before the launch)
    assert lib.gnnpn_score_select_f32(None, 128, nil, p, nil, len(words), nil, nil, nil, nil, nil, 90, nil, nil, 4, 128, 5, None) == -1
    assert b"null operand" in lib.gnnpn_last_error()
