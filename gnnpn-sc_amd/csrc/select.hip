// Candidate reduction (per problem x category top-K of the feasible services) and the full
// per-row ranking.  Integer/compare work, HBM-bound on the score rows: one wavefront per
// (problem, category) segment, each lane scanning a strided share of the segment; the K picks are
// K wave-wide max-reductions over 64-bit keys (order bits of the score, its zero canonicalised : inverted id), so equal scores —
// -0.0 and +0.0 are equal, as for the stable descending sort of the oracle — resolve to
// the lowest service id and the result does not depend on lane count or launch geometry.  The two full-ranking kernels share one
// bitonic network (bitonic_sort_desc): on 64-bit keys, or on ids that form their keys from the score row.
#include <vector>

#include "common.h"
#include "select_keys.h"   // rank_key, feasible, pick_rounds, cyclic_pick, emit_row: the reduction's rules

// A lane's best key below `last` among the feasible services s_first, s_first + stride, ... of a category: the rescan of the
// score row and the QoS table that a round of the memory forms makes.
__device__ __forceinline__ unsigned long long rescan_best(const float* __restrict__ srow, const double* __restrict__ qos, const CellBounds& lb,
                                                          int s_first, int s_end, int stride, unsigned long long last) {
    unsigned long long best = 0ull;
    for (int s = s_first; s < s_end; s += stride) {
        const bool feas = feasible(qos[(int64_t)s * 4 + 2], qos[(int64_t)s * 4 + 3], lb);
        const unsigned long long key = rank_key(srow[s], (uint32_t)s);
        if (feas && key < last && key > best) best = key;
    }
    return best;
}

// Problem b's global bounds for emit_row, loaded only where it writes them: at category 0.
__device__ __forceinline__ float4 global_tail(int c, const double* __restrict__ global_bounds, int b) {
    return c == 0 ? qos_row_f32(global_bounds + (int64_t)b * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(256) void select_candidates_kernel(
    const float* __restrict__ scores, int64_t ld_scores, const int32_t* __restrict__ cat_ptr,
    const double* __restrict__ qos, const double* __restrict__ local_bounds, const uint8_t* __restrict__ present,
    const double* __restrict__ global_bounds, float* __restrict__ out_rows, int32_t* __restrict__ out_ids,
    int32_t B, int32_t T, int32_t n_per) {
    const int lane = threadIdx.x & 63;
    const int64_t seg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= (int64_t)B * T) return;
    const int b = (int)(seg / T), c = (int)(seg - (int64_t)b * T);
    const int s_begin = cat_ptr[c], s_end = cat_ptr[c + 1];
    const bool pres = present[seg] != 0;
    const CellBounds lb = cell_bounds(local_bounds + seg * 4);
    const float* srow = scores + (int64_t)b * ld_scores;

    int my_pick = -1;   // lane r keeps the r-th pick
    int n_found = 0;
    if (pres)
        n_found = pick_rounds(n_per, lane, my_pick, [&](unsigned long long last) { return rescan_best(srow, qos, lb, s_begin + lane, s_end, 64, last); },
                              [](unsigned long long v) { return wave_max_u64(v); });
    const int id = cyclic_pick(my_pick, n_found, 0, lane);
    if (lane < n_per) {
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n_found > 0) q = qos_row_f32(qos + (int64_t)id * 4);
        emit_row(n_found, id, q, c, global_tail(c, global_bounds, b), (int64_t)b * T * n_per + (int64_t)c * n_per + lane, out_rows, out_ids);
    }
}

// The same reduction with 16 lanes per (problem, category) segment, four segments per wave, for n_per <= 16: the row-wide
// maximum is four DPP rotations instead of six cross-wave shuffles on each key half, and a category of 5 services (the
// 1000-task shapes) no longer occupies a whole wave.  Same keys, same rounds, same writer (select_keys.h).
// W = 16 or 8 lanes per segment; 8 (n_per <= 8, categories of about 8 services or fewer: the 1000-task shapes have 5) puts eight
// segments into a wave — the kernel is bound by its vector instructions, which are per wave.
template <int W>
__global__ __launch_bounds__(256) void select_candidates16_kernel(
    const float* __restrict__ scores, int64_t ld_scores, const int32_t* __restrict__ cat_ptr,
    const double* __restrict__ qos, const double* __restrict__ local_bounds, const uint8_t* __restrict__ present,
    const double* __restrict__ global_bounds, float* __restrict__ out_rows, int32_t* __restrict__ out_ids,
    int32_t B, int32_t T, int32_t n_per) {
    const int lane = threadIdx.x & 63, sub = lane & (W - 1), group = lane & ~(W - 1);
    const int64_t seg = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / W) + lane / W;
    if (seg >= (int64_t)B * T) return;                                  // whole W-lane groups leave together
    const int b = (int64_t)B * T <= 0x7fffffffll ? (int)((unsigned)seg / (unsigned)T) : (int)(seg / T);   // (a 64-bit division per lane is ~100 instructions)
    const int c = (int)(seg - (int64_t)b * T);
    const int s_begin = cat_ptr[c], s_end = cat_ptr[c + 1];
    const bool pres = present[seg] != 0;
    const CellBounds lb = cell_bounds(local_bounds + seg * 4);
    const float* srow = scores + (int64_t)b * ld_scores;

    auto group_max = [](unsigned long long v) { return W == 16 ? row16_max_u64(v) : row8_max_u64(v); };
    int my_pick = -1;   // lane r of the group keeps the r-th pick
    int n_found = 0;
    const bool small = s_end - s_begin <= W;
    float4 own = dummy_row();                                          // this lane's service's QoS row (small categories; a lane without one is nobody's owner)
    if (pres && small) {
        // a category of at most W services (the 1000-task shapes: 5): every lane forms its ONE key once — 0 if the service is
        // infeasible or absent — and the rounds are max-reductions over registers (no re-read of the scores and bounds per pick);
        // the lane keeps its service's whole QoS row, so the emitted rows come from a lane exchange, not from a second,
        // dependent round of loads
        unsigned long long key = 0ull;
        const int s = s_begin + sub;
        if (s < s_end) {
            const double* qs = qos + (int64_t)s * 4;
            own = qos_row_f32(qs);
            if (feasible(qs[2], qs[3], lb)) key = rank_key(srow[s], (uint32_t)s);
        }
        n_found = pick_rounds(n_per, sub, my_pick, [&](unsigned long long last) { return key < last ? key : 0ull; }, group_max);
    } else if (pres) {
        n_found = pick_rounds(n_per, sub, my_pick, [&](unsigned long long last) { return rescan_best(srow, qos, lb, s_begin + sub, s_end, W, last); }, group_max);
    }
    const int id = cyclic_pick(my_pick, n_found, group, sub);
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (small) {                                                       // (the whole group of W lanes takes this branch together)
        const int owner = n_found > 0 ? group + (id - s_begin) : lane;
        q = make_float4(__shfl(own.x, owner, 64), __shfl(own.y, owner, 64), __shfl(own.z, owner, 64), __shfl(own.w, owner, 64));
    } else if (n_found > 0 && sub < n_per) {
        q = qos_row_f32(qos + (int64_t)id * 4);
    }
    if (sub < n_per) {
        emit_row(n_found, id, q, c, global_tail(c, global_bounds, b), (int64_t)b * T * n_per + (int64_t)c * n_per + sub, out_rows, out_ids);
    }
}

extern "C" int gnnpn_select_candidates(const float* scores, int64_t ld_scores, const int32_t* cat_ptr,
                                       const double* qos, const double* local_bounds, const uint8_t* present,
                                       const double* global_bounds, float* out_rows, int32_t* out_ids, int32_t B,
                                       int32_t T, int32_t n_per, void* stream) {
    GNNPN_REQUIRE(B >= 0 && T > 0, "select_candidates: bad shape");
    if (B == 0) return GNNPN_OK;
    GNNPN_REQUIRE(scores && cat_ptr && qos && local_bounds && present && global_bounds && out_rows && out_ids,
                  "select_candidates: null operand");
    GNNPN_REQUIRE(n_per >= 1 && n_per <= 64, "select_candidates: n_per must be in [1,64], got %d", n_per);
    GNNPN_REQUIRE(gnnpn_aligned(out_rows, 16), "select_candidates: out_rows must be 16-byte aligned");
    const int64_t n_seg = (int64_t)B * T;
    auto launch = [&](auto kernel, int segs_per_workgroup) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((n_seg + segs_per_workgroup - 1) / segs_per_workgroup)), dim3(256), 0, (hipStream_t)stream,
                           scores, ld_scores, cat_ptr, qos, local_bounds, present, global_bounds, out_rows, out_ids, B, T, n_per);
    };
    if (n_per <= 8 && ld_scores <= 8ll * T) launch(select_candidates16_kernel<8>, 32);      // (ld_scores >= the number of services: mean category <= 8)
    else if (n_per <= 16) launch(select_candidates16_kernel<16>, 16);
    else launch(select_candidates_kernel, 4);
    GNNPN_CHECK_LAUNCH("select_candidates");
    return GNNPN_OK;
}

// ---------------------------------------------------------------------------------------------
// The bitonic network of a workgroup over the P (a power of two) slots in LDS, descending by `less` on two slot values.  Every
// thread of the workgroup calls it, after a barrier behind the slots' initialisation; it ends with a barrier.
template <typename Slot, typename Less>
__device__ __forceinline__ void bitonic_sort_desc(Slot* __restrict__ slots, int P, Less less) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += blockDim.x) {
                const int i = 2 * t - (t & (j - 1));   // lower index of the pair (bit j clear)
                const int p = i + j;
                const bool desc = (i & k) == 0;        // descending blocks first -> overall descending
                const Slot a = slots[i], b = slots[p];
                if (less(a, b) == desc) {
                    slots[i] = b;
                    slots[p] = a;
                }
            }
            __syncthreads();
        }
    }
}

// Full ranking of one score row per workgroup: bitonic sort of 64-bit keys in LDS (descending; ties -> lowest id).
__global__ __launch_bounds__(1024) void rank_rows_kernel(const float* __restrict__ scores, int64_t ld_scores,
                                                         int32_t* __restrict__ ranking, int32_t S, int32_t P) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
    const float* srow = scores + (int64_t)blockIdx.x * ld_scores;
    for (int i = threadIdx.x; i < P; i += blockDim.x) keys[i] = i < S ? rank_key(srow[i], (uint32_t)i) : 0ull;
    __syncthreads();
    bitonic_sort_desc(keys, P, [](unsigned long long a, unsigned long long b) { return a < b; });
    int32_t* out = ranking + (int64_t)blockIdx.x * S;
    for (int i = threadIdx.x; i < S; i += blockDim.x) out[i] = key_id(keys[i]);
}

// Rows of 16385..32768 services (BASELINE configs[4]: S = 20000): the 64-bit keys no longer fit the LDS, so the
// same bitonic network runs on 32-bit service ids in LDS and forms each key from the (L2-resident) score row
// when it compares.  Identical order by construction; only used on the artefact path.
__global__ __launch_bounds__(1024) void rank_rows_indirect_kernel(const float* __restrict__ scores, int64_t ld_scores,
                                                                  int32_t* __restrict__ ranking, int32_t S, int32_t P) {
    extern __shared__ __attribute__((aligned(16))) unsigned int ids[];
    const float* srow = scores + (int64_t)blockIdx.x * ld_scores;
    auto key_of = [&](unsigned int i) { return i < (unsigned)S ? rank_key(srow[i], i) : 0ull; };
    for (int i = threadIdx.x; i < P; i += blockDim.x) ids[i] = (unsigned)i;
    __syncthreads();
    bitonic_sort_desc(ids, P, [&](unsigned int ia, unsigned int ib) { return key_of(ia) < key_of(ib); });
    int32_t* out = ranking + (int64_t)blockIdx.x * S;
    for (int i = threadIdx.x; i < S; i += blockDim.x) out[i] = (int32_t)ids[i];
}

extern "C" int gnnpn_rank_rows(const float* scores, int64_t ld_scores, int32_t* ranking, int32_t B, int32_t S,
                               void* stream) {
    GNNPN_REQUIRE(B >= 0 && S > 0 && ld_scores >= S, "rank_rows: bad shape");
    if (B == 0) return GNNPN_OK;
    GNNPN_REQUIRE(scores && ranking, "rank_rows: null operand");
    if (S > 32768) GNNPN_FAIL(GNNPN_E_UNSUP, "rank_rows: S=%d exceeds the single-workgroup LDS sort (32768)", S);
    int P = 2;
    while (P < S) P <<= 1;
    const bool indirect = S > 16384;                                   // the 64-bit keys no longer fit the LDS: sort ids
    const size_t lds = (size_t)P * (indirect ? sizeof(unsigned int) : sizeof(unsigned long long));
    if (const int rc = gnnpn_launch_lds(indirect ? rank_rows_indirect_kernel : rank_rows_kernel, dim3(B), dim3(1024), lds,
                                        (hipStream_t)stream, "rank_rows", scores, ld_scores, ranking, S, P))
        return rc;
    GNNPN_CHECK_LAUNCH("rank_rows");
    return GNNPN_OK;
}

// ---------------------------------------------------------------------------------------------
// P@k of TrainML.test (trainML.py:63-70): fraction of the top-k ranked services whose label is 1.
__global__ void precision_at_k_kernel(const int32_t* __restrict__ ranking, int64_t ld_rank,
                                      const float* __restrict__ labels, int64_t ld_lab, int32_t B, int32_t S,
                                      const int32_t* __restrict__ ks, int32_t n_k, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * n_k) return;
    const int b = i / n_k, k = ks[i - b * n_k];
    int hits = 0;
    for (int j = 0; j < k && j < S; ++j) {
        const int s = ranking[(int64_t)b * ld_rank + j];
        hits += (s >= 0 && s < S && labels[(int64_t)b * ld_lab + s] == 1.0f);
    }
    out[i] = (float)hits / (float)k;
}

extern "C" int gnnpn_precision_at_k(const int32_t* ranking, int64_t ld_rank, const float* labels, int64_t ld_lab,
                                    int32_t B, int32_t S, const int32_t* ks, int32_t n_k, float* out, void* stream) {
    GNNPN_REQUIRE(B >= 0 && S > 0 && n_k > 0 && ld_rank >= 1 && ld_lab >= S, "precision_at_k: bad shape");
    GNNPN_REQUIRE(ks, "precision_at_k: null ks");
    // the kernel reads min(k, S) ranking entries per row and divides by k: every k is checked before the launch (a stream-ordered
    // copy of the n_k values, then a wait for it; this evaluation path is never captured into a graph)
    std::vector<int32_t> kh((size_t)n_k);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(kh.data(), ks, sizeof(int32_t) * (size_t)n_k, hipMemcpyDefault, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        GNNPN_FAIL(GNNPN_E_LAUNCH, "precision_at_k: reading ks failed");
    int32_t kmax = 0;
    for (int32_t k : kh) {
        GNNPN_REQUIRE(k >= 1, "precision_at_k: k = %d (every k must be >= 1)", k);
        kmax = k > kmax ? k : kmax;
    }
    GNNPN_REQUIRE(ld_rank >= (kmax < S ? kmax : S), "precision_at_k: ld_rank %lld < min(max k, S) = %d", (long long)ld_rank,
                  kmax < S ? kmax : S);
    if (B == 0) return GNNPN_OK;
    GNNPN_REQUIRE(ranking && labels && out, "precision_at_k: null operand");
    hipLaunchKernelGGL(precision_at_k_kernel, dim3((B * n_k + 127) / 128), dim3(128), 0, s, ranking,
                       ld_rank, labels, ld_lab, B, S, ks, n_k, out);
    GNNPN_CHECK_LAUNCH("precision_at_k");
    return GNNPN_OK;
}
