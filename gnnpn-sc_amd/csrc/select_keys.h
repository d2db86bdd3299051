// The candidate reduction's rules, each stated once: the ranking key and its maximum over a group of lanes, the bounds test, the
// pick rounds and the writer of the emitted rows.  Shared by select.hip (scores read back from HBM) and score_select.hip (scores
// still in LDS behind the product), so that every form picks the same services for the same scores and emits the same rows.
#pragma once
#include "common.h"

// float_order_key puts -0 below +0; a ranking must not: score + (+0), rounded to nearest, is +0 for either zero and the score itself
// for every other value (denormals are kept; a NaN stays a NaN and still sorts above +inf).
__device__ __forceinline__ unsigned long long rank_key(float score, uint32_t id) {
    return ((unsigned long long)float_order_key(__fadd_rn(score, 0.0f)) << 32) | (0xffffffffu - id);
}
// The service id of a key (its low word holds the inverted id: of equal scores the lowest id is the largest key).
__device__ __forceinline__ int key_id(unsigned long long key) { return (int)(0xffffffffu - (uint32_t)(key & 0xffffffffu)); }

// The maximum over the 16 lanes of a DPP row: four rotations instead of six cross-wave shuffles on each key half.
__device__ __forceinline__ unsigned long long row16_max_u64(unsigned long long v) {
#define GNNPN_MAX_STEP(CTRL)                                                                                       \
    {                                                                                                              \
        const unsigned lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xF, 0xF, true);                \
        const unsigned hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xF, 0xF, true);        \
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;                                          \
        v = o > v ? o : v;                                                                                         \
    }
    GNNPN_MAX_STEP(0x121) GNNPN_MAX_STEP(0x122) GNNPN_MAX_STEP(0x124) GNNPN_MAX_STEP(0x128)   // row_ror:1, 2, 4, 8
    return v;
}
// ... and over groups of 8 lanes: the neighbour, the other pair (quad_perm), the other quad (row_half_mirror); a maximum does
// not depend on the order it is formed in
__device__ __forceinline__ unsigned long long row8_max_u64(unsigned long long v) {
    GNNPN_MAX_STEP(0xB1) GNNPN_MAX_STEP(0x4E) GNNPN_MAX_STEP(0x141)
    return v;
#undef GNNPN_MAX_STEP
}

// The local bounds of a (problem, category) cell and the one test against them: a NaN on either side fails it.
struct CellBounds {
    double lo_c, hi_c, lo_q, hi_q;
};
__device__ __forceinline__ CellBounds cell_bounds(const double* lb) { return {lb[0], lb[1], lb[2], lb[3]}; }
__device__ __forceinline__ bool feasible(double cost, double qual, const CellBounds& lb) {
    return lb.lo_c <= cost && cost <= lb.hi_c && lb.lo_q <= qual && qual <= lb.hi_q;
}

// The pick rounds of one cell on its group of lanes: round r takes the group's largest key below round r - 1's, until n_per are
// found or none is left (key 0: no service).  local_best(last) is the lane's best key below `last` — over registers or by a
// rescan of memory — and group_max its maximum over the group.  Lane `slot` == r keeps the r-th pick's id in my_pick; returns
// the number of picks found.
template <typename LocalBest, typename GroupMax>
__device__ __forceinline__ int pick_rounds(int n_per, int slot, int& my_pick, LocalBest local_best, GroupMax group_max) {
    unsigned long long last = ~0ull;
    int r = 0;   // rounds done = picks found
    for (; r < n_per; ++r) {
        const unsigned long long best = group_max(local_best(last));
        if (best == 0ull) break;
        if (slot == r) my_pick = key_id(best);
        last = best;
    }
    return r;
}

// The row of a cell without a feasible service (loadData.py:148).
__device__ __forceinline__ float4 dummy_row() { return make_float4(0.f, 1.f, 1.f, 1.f); }

// A QoS row (or a problem's global bounds) as it is emitted: four doubles narrowed to float.
__device__ __forceinline__ float4 qos_row_f32(const double* q) { return make_float4((float)q[0], (float)q[1], (float)q[2], (float)q[3]); }

// The id lane `slot` emits: the picks repeated cyclically (loadData.py:137-141) — what lane group_base + slot % n_found kept.
__device__ __forceinline__ int cyclic_pick(int my_pick, int n_found, int group_base, int slot) {
    return __shfl(my_pick, group_base + (n_found > 0 ? slot % n_found : 0), 64);
}

// The writer of one emitted row (16-byte aligned out_rows: the launchers check it): the pick's QoS row `q` and its id, or the
// dummy row and -1 where the cell has no feasible service (q is not read then); behind it the problem's global bounds at
// category 0 — tail0, which a caller need not load for any other — and zeros elsewhere.
__device__ __forceinline__ void emit_row(int n_found, int id, float4 q, int c, float4 tail0, int64_t pos, float* out_rows, int32_t* out_ids) {
    float4* dst = reinterpret_cast<float4*>(out_rows + pos * 8);
    dst[0] = n_found > 0 ? q : dummy_row();
    dst[1] = c == 0 ? tail0 : make_float4(0.f, 0.f, 0.f, 0.f);
    out_ids[pos] = n_found > 0 ? id : -1;
}
