// The neighbour aggregate of the one-launch GIN layers (gin_layer.hip, gin_layer_split.hip), vector form: written once, so that the
// sums the fp16-split layer decomposes are the function tests/test_gpu_ops.py holds bit for bit to csr_aggregate_kernel through the
// fp32 layer (test_gin_layer_equals_the_separate_kernels).
#pragma once
#include "common.h"

template <int NCH>
struct GinRowSum {
    float4 chunk[NCH];
};

// sum_j x[col[e]] over the row's edges e0 .. e1 - 1 in CSR order, then + (1 + eps) * x[row], for this lane's channels: 8 lanes per
// row (`sub` = the lane's place among them), float4 chunks dealt round-robin — chunk i holds channels 4 (sub + 8 i) .. + 3, for
// c_in <= 32 NCH channels, c_in and ldx multiples of 4, x 16-byte aligned.  The edge loop is the OUTER one, so that a lane has all its
// chunks of a neighbour row in flight at once; every add and the product with 1 + eps round on their own.  Chunks beyond c_in, and
// every chunk of a row beyond the last (row >= M; pass e0 = e1 = 0), stay zero.
// The sums live in a local array and are copied out at the end: accumulated in the caller's memory (a reference parameter, or the
// returned object itself) the compiler keeps a second register set for the loop — gin_layer_kernel 83 -> 112 registers.
template <int NCH>
__device__ __forceinline__ GinRowSum<NCH> gin_aggregate_row(const int32_t* __restrict__ col, const float* __restrict__ x, int64_t ldx,
                                                            int c_in, int64_t row, int64_t M, int e0, int e1, int sub,
                                                            float one_plus_eps) {
    float4 acc[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int nch = (c_in / 4 - sub + 7) / 8;             // this lane's chunks: 4 * (sub + 8 i) < c_in
    for (int e = e0; e <= e1; ++e) {                      // e == e1: the row itself, scaled by 1 + eps, AFTER the neighbours
        if (row >= M) break;
        const bool own = e == e1;
        const float* src = x + (own ? row : (int64_t)col[e]) * ldx + 4 * sub;
        float4 t[NCH];
#pragma unroll
        for (int i = 0; i < NCH; ++i)
            if (i < nch) t[i] = *reinterpret_cast<const float4*>(src + 32 * i);
#pragma unroll
        for (int i = 0; i < NCH; ++i)
            if (i < nch) {
                if (own) {
                    t[i].x = __fmul_rn(one_plus_eps, t[i].x);
                    t[i].y = __fmul_rn(one_plus_eps, t[i].y);
                    t[i].z = __fmul_rn(one_plus_eps, t[i].z);
                    t[i].w = __fmul_rn(one_plus_eps, t[i].w);
                }
                acc[i].x = __fadd_rn(acc[i].x, t[i].x);
                acc[i].y = __fadd_rn(acc[i].y, t[i].y);
                acc[i].z = __fadd_rn(acc[i].z, t[i].z);
                acc[i].w = __fadd_rn(acc[i].w, t[i].w);
            }
    }
    GinRowSum<NCH> sum;
#pragma unroll
    for (int i = 0; i < NCH; ++i) sum.chunk[i] = acc[i];
    return sum;
}
