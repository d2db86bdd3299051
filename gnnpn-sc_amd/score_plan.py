"""Host side of the fused score product + candidate reduction (csrc/score_select.hip, gnnpn_score_select_f32): where it applies,
the chunk plan of a service table and the B-fragment-packed service embedding.  All three depend on the service table (and the
weights) only, so pipeline.py builds them once per ``DeviceServices`` and keeps them beside the service embedding (``OperandCache``).

The kernel's grid is (tiles of 16 problems) x (chunks of whole categories); a chunk is a contiguous run of categories, and the
chunks are balanced by service count.  Numpy only up to ``pack_embedding`` / ``ScorePlan.to``: the planner runs without a GPU.
"""
import os

import numpy as np

HIDDEN = 128            # the hidden size the kernel is built for
MAX_N_PER = 16
MAX_CATEGORY = 256      # GNNPN_SCORE_SELECT_MAX_CATEGORY: services of the largest category (a lane holds 16 keys)
MAX_TILES = 24          # GNNPN_SCORE_SELECT_MAX_TILES: 16-column tiles of one chunk (its scores and QoS rows stay in LDS)
MAX_CHUNK_CATEGORIES = 16   # GNNPN_SCORE_SELECT_MAX_CHUNK_CATEGORIES (so do the 16 problems' bounds of every category of the chunk)
MIN_MEAN_CATEGORY = 16  # below: the two-launch path (its 8-lane form is built for the 5- and 10-service categories)


def unfused_front():
    """GNNPN_UNFUSED_FRONT=1: the pipeline keeps the two launches (linear + segment_topk_feasible) everywhere."""
    return os.environ.get("GNNPN_UNFUSED_FRONT", "0") == "1"


def applies(cat_ptr, hidden, n_per):
    """Whether the fused kernel is built for this table: hidden 128, n_per <= 16, mean category >= 16, largest <= MAX_CATEGORY."""
    cat = np.asarray(cat_ptr, dtype=np.int64)
    sizes = np.diff(cat)
    return bool(int(hidden) == HIDDEN and 1 <= int(n_per) <= MAX_N_PER and len(sizes) > 0 and cat[0] == 0 and (sizes >= 0).all() and
                cat[-1] >= MIN_MEAN_CATEGORY * len(sizes) and sizes.max() <= MAX_CATEGORY)


def chunk_bounds(cat_ptr, n_chunks):
    """chunk_ptr [n_chunks + 1]: boundary i is the category boundary nearest to i * S / n_chunks services (the lower one of two
    equally near), so every chunk is a contiguous run of whole categories, every category lies in exactly one chunk, and a chunk's
    service count differs from S / n_chunks by at most one category's size.  More chunks than categories leaves some empty."""
    cat = np.asarray(cat_ptr, dtype=np.int64)
    n = int(n_chunks)
    if n < 1 or len(cat) < 2:
        raise ValueError("chunk_bounds: at least one chunk and one category")
    S = int(cat[-1])
    targets = np.arange(n + 1, dtype=np.float64) * (S / n)
    hi = np.clip(np.searchsorted(cat, targets, side="left"), 0, len(cat) - 1)
    lo = np.clip(hi - 1, 0, len(cat) - 1)
    bounds = np.where(np.abs(cat[lo] - targets) <= np.abs(cat[hi] - targets), lo, hi)
    bounds[0], bounds[-1] = 0, len(cat) - 1
    return np.maximum.accumulate(bounds).astype(np.int32)


class ScorePlan:
    """The plan words of gnnpn_score_select_f32 (include/gnnpn_hip.h): T, n_chunks, n_tiles, S, cat_ptr, tile_ptr, chunk_ptr,
    chunk_info (per chunk: first / end category, first tile, tiles, first / end service, 0, 0)."""

    def __init__(self, cat_ptr, chunk_ptr):
        cat = np.asarray(cat_ptr, dtype=np.int32)
        chunk = np.asarray(chunk_ptr, dtype=np.int32)
        tile = np.concatenate([[0], np.cumsum((np.diff(cat.astype(np.int64)) + 15) // 16)]).astype(np.int32)
        self.cat_ptr, self.tile_ptr, self.chunk_ptr = cat, tile, chunk
        self.n_categories, self.n_chunks, self.n_tiles, self.n_services = len(cat) - 1, len(chunk) - 1, int(tile[-1]), int(cat[-1])
        lo, hi = chunk[:-1], chunk[1:]
        zero = np.zeros(self.n_chunks, dtype=np.int32)
        self.chunk_info = np.stack([lo, hi, tile[lo], tile[hi] - tile[lo], cat[lo], cat[hi], zero, zero], 1).astype(np.int32)
        self.words = np.concatenate([[self.n_categories, self.n_chunks, self.n_tiles, self.n_services], cat, tile, chunk,
                                     self.chunk_info.reshape(-1)]).astype(np.int32)

    def chunk_tiles(self):
        return np.diff(self.tile_ptr[self.chunk_ptr].astype(np.int64))

    def chunk_services(self):
        return np.diff(self.cat_ptr[self.chunk_ptr].astype(np.int64))

    def fits(self):
        return bool(self.chunk_tiles().max() <= MAX_TILES and np.diff(self.chunk_ptr).max() <= MAX_CHUNK_CATEGORIES and
                    np.diff(self.cat_ptr.astype(np.int64)).max() <= MAX_CATEGORY)

    def tensors(self, device):
        """(plan_host, plan): the words as an int32 host tensor and its copy on ``device`` (the operator's two plan operands)."""
        import torch
        host = torch.from_numpy(self.words.copy())
        return host, host.to(device)


def plan_chunks(cat_ptr, n_chunks):
    """A ScorePlan of about ``n_chunks`` balanced chunks whose chunks all fit a workgroup (<= MAX_TILES tiles, <= MAX_CHUNK_CATEGORIES categories): more chunks are taken
    until they do — one category per chunk at the latest, which fits whenever ``applies``.  None where no plan fits."""
    cat = np.asarray(cat_ptr, dtype=np.int64)
    T = len(cat) - 1
    n = max(1, int(n_chunks))
    while True:
        plan = ScorePlan(cat, chunk_bounds(cat, n) if n != T else np.arange(T + 1))
        if plan.fits():
            return plan
        if n == T:
            return None
        n = T if n > T else min(T, n + max(1, n // 4))


def chunk_count(n_categories, n_problems, n_cu):
    """The chunks to ask ``plan_chunks`` for: about one workgroup per CU over the batch's tiles of 16 problems — at least one, and
    no more than there are categories."""
    return min(int(n_categories), max(1, int(n_cu) // max(1, (int(n_problems) + 15) // 16)))


def pack_embedding(emb, plan):
    """[S, 128] service embedding -> v_mfma_f32_16x16x4_f32 B-fragments [n_tiles, 8, 64, 4], every category its own run of
    16-column tiles: packed[t][kb][lane][j] = emb[first service of tile t + lane % 16][16 kb + 4 j + lane // 16], 0 behind the
    category's last service.  A layout change (a gather and a permute), no arithmetic — ops.pack_mfma_b's layout, per category."""
    import torch
    S, K = emb.shape
    if K != HIDDEN or S != plan.n_services:
        raise ValueError(f"pack_embedding: [{plan.n_services}, {HIDDEN}] expected, got {tuple(emb.shape)}")
    sizes = np.diff(plan.cat_ptr.astype(np.int64))
    n_t = (sizes + 15) // 16
    cat_of_tile = np.repeat(np.arange(len(sizes)), n_t)
    first = plan.cat_ptr[cat_of_tile].astype(np.int64) + 16 * (np.arange(plan.n_tiles) - plan.tile_ptr[cat_of_tile])
    rows = first[:, None] + np.arange(16)[None, :]                                   # [n_tiles, 16] service of every column
    rows = np.where(rows < plan.cat_ptr[cat_of_tile + 1][:, None], rows, S)          # S: the zero row appended below
    padded = torch.cat([emb, torch.zeros((1, K), dtype=emb.dtype, device=emb.device)])
    v = padded[torch.from_numpy(rows.reshape(-1)).to(emb.device)].view(plan.n_tiles, 16, K // 16, 4, 4)   # [t, c, kb, j, kq]
    return v.permute(0, 2, 4, 1, 3).reshape(plan.n_tiles, K // 16, 64, 4).contiguous()                    # [t, kb, (kq, c), j]


class OperandCache:
    """The kernel's operands for one service table, kept beside it (``DeviceServices.score_cache``): whether the kernel applies per
    (hidden, n_per), the plan and its two tensors per chunk count, and the packed embedding, which follows the embedding object it
    was packed from (one per (weights, table))."""

    def __init__(self, cat_ptr, device):
        self.cat_ptr, self.device, self.n_categories = cat_ptr, device, len(cat_ptr) - 1
        self._applies, self._plans, self._emb, self._packed = {}, {}, None, None

    def applies(self, hidden, n_per):
        key = (int(hidden), int(n_per))
        if key not in self._applies:
            self._applies[key] = applies(self.cat_ptr, *key)
        return self._applies[key]

    def plan(self, n_chunks):
        """(ScorePlan, plan_host, plan) for about ``n_chunks`` chunks, or None where no plan fits."""
        if n_chunks not in self._plans:
            plan = plan_chunks(self.cat_ptr, n_chunks)
            self._plans[n_chunks] = None if plan is None else (plan, *plan.tensors(self.device))
        return self._plans[n_chunks]

    def packed(self, emb, plan):
        if self._emb is not emb:
            self._emb, self._packed = emb, pack_embedding(emb, plan)                 # (the tile layout is the same in every plan)
        return self._packed
