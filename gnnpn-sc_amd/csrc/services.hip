// A searched composition as service ids, and the figure of merit of a composition given as ids.
//   search_services_kernel — from the positions a search stage returns (best_pos: positions inside the candidate lists of one
//       call) to rows of the service table, through the ids the builder wrote beside its tables (woa_prep.hip:
//       woa_services_kernel): per slot (best_services) and per node of the batch (node_services).
//   services_merit_kernel / services_merit_wide_kernel — violate + objFunc of the rows qos[id] of a problem's nodes, in node
//       order, each value through round(v, 5) where the tables of the search were seeded.  The evaluation is woa_eval.h's
//       (figure_of_merit, wide_merit): the merit a search stage reports for the same rows, bit for bit.
// One wavefront (lane form) or one workgroup (workgroup form) per problem, no atomics, plain stores, every loop bounded by a
// node or slot count.
#include "round5.h"
#include "woa_eval.h"

#include <climits>

namespace {

constexpr int NO_ROWS = 0;        // n_rows of a problem without a single id >= 0: its merit is NaN (objFunc divides by the count)
constexpr int NOT_SCORED = -1;    // n_rows of a problem with an id outside [-1, n_services), more rows than max_slots, or a bad segment

__global__ __launch_bounds__(64) void search_services_kernel(int32_t R, const int32_t* __restrict__ start_index,
                                                             const double* __restrict__ best_fitness,
                                                             const int32_t* __restrict__ best_pos, int32_t ld,
                                                             const int32_t* __restrict__ prob_ptr, int32_t n_lists,
                                                             const int32_t* __restrict__ cand_ptr, int32_t n_cand,
                                                             const int32_t* __restrict__ cand_service,
                                                             const int32_t* __restrict__ slot_node, const int32_t* __restrict__ seg_ptr,
                                                             int32_t n_nodes, int32_t* __restrict__ best_services,
                                                             int32_t* __restrict__ node_services) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int n0 = seg_ptr[b], n1 = seg_ptr[b + 1];
    if (n0 < 0 || n1 < n0 || n1 > n_nodes) n0 = n1 = 0;         // a bad segment owns no node
    const int nn = n1 - n0;
    const int r = start_index ? start_index[b] : 0;
    int p0 = 0, n = 0;
    if (r >= 0 && r < R) {
        const size_t q = (size_t)b * R + r;
        p0 = prob_ptr[q];
        n = prob_ptr[q + 1] - p0;
    }
    const double f = best_fitness[b];
    // not searched, not sized for, failed in the builder: the merit says so (a position of -1 is a valid Python position)
    if (f != f || n <= 0 || n > ld || p0 < 0 || p0 + n > n_lists) {
        for (int l = lane; l < ld; l += 64) best_services[(size_t)b * ld + l] = -1;
        for (int k = lane; k < nn; k += 64) node_services[n0 + k] = -1;
        return;
    }
    // slots are in node order: slot l names its own node and fills the nodes between the previous slot's and its own (the
    // last slot: to the end of the segment too), so that every node is written once
    for (int l = lane; l < ld; l += 64) {
        if (l >= n) {
            best_services[(size_t)b * ld + l] = -1;
            continue;
        }
        const int j = p0 + l;
        const int base = cand_ptr[j], len = cand_ptr[j + 1] - base;
        int p = best_pos[(size_t)b * ld + l];
        if (p < 0) p += len;                                    // Python list indexing (refine's ES-WOA positions)
        int s = -1;
        if (p >= 0 && p < len && base >= 0 && base + p < n_cand) s = cand_service[base + p];
        best_services[(size_t)b * ld + l] = s;
        const int node = slot_node[j];
        const int prev = l > 0 ? slot_node[j - 1] : -1;
        const int gap_end = node < nn ? node : nn;
        for (int k = prev + 1 > 0 ? prev + 1 : 0; k < gap_end; ++k) node_services[n0 + k] = -1;
        if (node >= 0 && node < nn && node > prev) node_services[n0 + node] = s;
        if (l == n - 1)
            for (int k = node + 1 > 0 ? node + 1 : 0; k < nn; ++k) node_services[n0 + k] = -1;
    }
}

// What both forms do first, by ONE wave (lane of 64): the ids >= 0 of the problem's nodes, in node order, into ids[0 .. cap-1].
// Returns the row count, NOT_SCORED for an id outside [-1, n_services) or a bad segment; a count above cap is returned as it is
// (the ids past cap are not stored).
__device__ int gather_ids(const int32_t* seg_ptr, int32_t n_nodes, const int32_t* node_services, int32_t n_services, int b, int lane,
                          int* ids, int cap) {
    const int n0 = seg_ptr[b], n1 = seg_ptr[b + 1];
    if (n0 < 0 || n1 < n0 || n1 > n_nodes) return NOT_SCORED;
    const unsigned long long below = (1ull << lane) - 1ull;
    int n = 0;
    bool bad = false;
    for (int g0 = n0; g0 < n1; g0 += 64) {
        const int g = g0 + lane;
        const int id = g < n1 ? node_services[g] : -1;
        if (id < -1 || id >= n_services) bad = true;
        const bool has = id >= 0 && id < n_services;
        const unsigned long long m = __ballot(has);
        const int at = n + __popcll(m & below);
        if (has && at < cap) ids[at] = id;
        n += __popcll(m);
    }
    return __ballot(bad) != 0ull ? NOT_SCORED : n;
}

__device__ __forceinline__ void load_row(const double* qos, int id, int rounded, double (&q)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double v = qos[(size_t)id * 4 + c];
        q[c] = rounded ? round5(v) : v;
    }
}

__device__ __forceinline__ void not_scored(int b, int n, double* merit, int32_t* n_rows) {
    merit[b] = NAN;
    n_rows[b] = n == NO_ROWS ? NO_ROWS : NOT_SCORED;
}

// lane form: at most 64 rows, row j in lane j (figure_of_merit)
__global__ __launch_bounds__(64) void services_merit_kernel(const int32_t* __restrict__ seg_ptr, int32_t n_nodes,
                                                            const int32_t* __restrict__ node_services,
                                                            const double* __restrict__ qos, int32_t n_services,
                                                            const double* __restrict__ bounds, int32_t rounded, int32_t max_slots,
                                                            double* __restrict__ merit, int32_t* __restrict__ n_rows) {
    __shared__ double col[4 * 64];
    __shared__ int ids[64];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = gather_ids(seg_ptr, n_nodes, node_services, n_services, b, lane, ids, 64);
    __syncthreads();
    if (n <= 0 || n > 64 || n > max_slots) {
        if (lane == 0) not_scored(b, n, merit, n_rows);
        return;
    }
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    if (lane < n) load_row(qos, ids[lane], rounded, q);
    const double f = figure_of_merit(q, n, lane, col, bounds + (size_t)b * 4);
    if (lane == 0) {
        merit[b] = f;
        n_rows[b] = n;
    }
}

// workgroup form: the rows in LDS as a table of one candidate per slot, which wide_merit evaluates at position 0 of every list.
// Dynamic LDS (services_wide_lds_bytes): WideLds for T = max_slots with 4 T doubles more (the rows), and T ints behind its own
// (the positions, all 0).
__host__ __device__ inline size_t services_wide_lds_bytes(int T) {
    return ((size_t)7 * T + 12) * sizeof(double) + ((size_t)3 * T + 4) * sizeof(int);
}

__global__ __launch_bounds__(WNT) void services_merit_wide_kernel(const int32_t* __restrict__ seg_ptr, int32_t n_nodes,
                                                                  const int32_t* __restrict__ node_services,
                                                                  const double* __restrict__ qos, int32_t n_services,
                                                                  const double* __restrict__ bounds, int32_t rounded, int32_t max_slots,
                                                                  double* __restrict__ merit, int32_t* __restrict__ n_rows) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int b = blockIdx.x, tid = threadIdx.x;
    WideLds L;
    double* rows = L.carve(lds_raw, max_slots, 4 * max_slots);
    int* zero = L.len + max_slots;
    if (tid < 64) {                                            // wave 0: the ids, kept in L.len until the rows are loaded
        const int n = gather_ids(seg_ptr, n_nodes, node_services, n_services, b, tid, L.len, max_slots);
        if (tid == 0) L.cnt[0] = n;
    }
    __syncthreads();
    const int n = L.cnt[0];
    if (n <= 0 || n > max_slots) {
        if (tid == 0) not_scored(b, n, merit, n_rows);
        return;
    }
    for (int j = tid; j < n; j += WNT) {
        double q[4];
        load_row(qos, L.len[j], rounded, q);
#pragma unroll
        for (int c = 0; c < 4; ++c) rows[(size_t)j * 4 + c] = q[c];
    }
    if (tid < 4) L.bounds[tid] = bounds[(size_t)b * 4 + tid];
    __syncthreads();
    for (int j = tid; j < n; j += WNT) {
        L.base[j] = j;
        L.len[j] = 1;
        zero[j] = 0;
    }
    __syncthreads();
    const double f = wide_merit(L, zero, rows, n, tid);
    if (tid == 0) {
        merit[b] = f;
        n_rows[b] = n;
    }
}

}  // namespace

extern "C" int gnnpn_search_services(int32_t B, int32_t R, const int32_t* start_index, const double* best_fitness, const int32_t* best_pos,
                                     int32_t pos_ld, const int32_t* prob_ptr, int32_t n_lists, const int32_t* cand_ptr, int32_t n_cand,
                                     const int32_t* cand_service, const int32_t* slot_node, const int32_t* seg_ptr, int32_t n_nodes,
                                     int32_t* best_services, int32_t* node_services, void* stream) {
    GNNPN_REQUIRE(B >= 0 && R >= 1 && pos_ld >= 1 && n_lists >= 0 && n_cand >= 0 && n_nodes >= 0 && (int64_t)B * R <= INT32_MAX,
                  "search_services: bad argument");
    if (B == 0) return GNNPN_OK;
    GNNPN_REQUIRE(best_fitness && best_pos && prob_ptr && cand_ptr && seg_ptr && best_services && (n_nodes == 0 || node_services) &&
                  (n_lists == 0 || slot_node) && (n_cand == 0 || cand_service), "search_services: null operand");
    GNNPN_REQUIRE(gnnpn_aligned(best_fitness, 8), "search_services: misaligned best_fitness");
    hipLaunchKernelGGL(search_services_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, R, start_index, best_fitness, best_pos, pos_ld,
                       prob_ptr, n_lists, cand_ptr, n_cand, cand_service, slot_node, seg_ptr, n_nodes, best_services, node_services);
    GNNPN_CHECK_LAUNCH("search_services");
    return GNNPN_OK;
}

extern "C" int gnnpn_services_merit_f64(int32_t B, const int32_t* seg_ptr, int32_t n_nodes, const int32_t* node_services, const double* qos,
                                        int32_t n_services, const double* bounds, int32_t rounded, int32_t max_slots, int32_t wide,
                                        double* merit, int32_t* n_rows, void* stream) {
    GNNPN_REQUIRE(B >= 0 && n_nodes >= 0 && n_services >= 0 && max_slots >= 1 && (rounded == 0 || rounded == 1),
                  "services_merit_f64: bad argument");
    if (B == 0) return GNNPN_OK;
    GNNPN_REQUIRE(seg_ptr && bounds && merit && n_rows && (n_nodes == 0 || node_services) && (n_services == 0 || qos),
                  "services_merit_f64: null operand");
    GNNPN_REQUIRE(gnnpn_aligned(qos, 8) && gnnpn_aligned(bounds, 8) && gnnpn_aligned(merit, 8), "services_merit_f64: misaligned operand");
    const bool use_wide = wide || max_slots > 64;
    const size_t lds = use_wide ? services_wide_lds_bytes(max_slots) : 0;
    auto too_large = [&]() -> int {
        GNNPN_FAIL(GNNPN_E_UNSUP, "services_merit_f64: %d rows need %zu B of LDS (a CU has 160 KB)", max_slots, lds);
    };
    return search_launch(lds, too_large, use_wide ? services_merit_wide_kernel : services_merit_kernel, B, use_wide ? WNT : 64, stream,
                         use_wide ? "services_merit_f64 (workgroup form)" : "services_merit_f64", seg_ptr, n_nodes, node_services, qos,
                         n_services, bounds, rounded, max_slots, merit, n_rows);
}
