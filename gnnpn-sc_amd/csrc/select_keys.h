// The ranking key of the candidate reduction and its maximum over a group of lanes: shared by select.hip (scores read back from
// HBM) and score_select.hip (scores still in LDS behind the product), so that both pick the same service for the same scores.
#pragma once
#include "common.h"

// float_order_key puts -0 below +0; a ranking must not: score + (+0), rounded to nearest, is +0 for either zero and the score itself
// for every other value (denormals are kept; a NaN stays a NaN and still sorts above +inf).
__device__ __forceinline__ unsigned long long rank_key(float score, uint32_t id) {
    return ((unsigned long long)float_order_key(__fadd_rn(score, 0.0f)) << 32) | (0xffffffffu - id);
}

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
