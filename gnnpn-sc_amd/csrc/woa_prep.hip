// ES-WOA inputs built on the device from an ML+2PN batch: the restatement of what the reference's `WOA.start` does between
// reading the High-level actions and calling ESWOA (src/baselines/WOA.py:194-208, 55-69; src/loadData.py:155-276, `addS` and
// `loadDataOther`) and of this package's host form of it (loadData.addS / loadDataOther + WOA._prepare).
//
// Three launches per call, one wavefront per problem in the two big ones, one lane per task slot (a task node of the problem's
// workflow graph, node order; slots above 64 loop):
//   count  — every slot scans its category's services in table order and keeps what `addS` keeps (the local-bounds filter,
//            or with reduct != 0 the "front" with its sentinel (1,0,1,1), replace-or-append and the skip of members that are
//            pointer-network picks), as indices into the category, in the workspace; the non-empty lists are ranked in node
//            order and paired BY POSITION with the problem's action rows (category order, dummy rows of absent categories —
//            float64 sum == 3 — dropped); rows and candidates are rounded to 5 decimals exactly as Python's round(v, 5); a
//            row absent from its list is appended, start = its first position;
//   scan   — one workgroup: exclusive scans over the problems (lists -> prob_ptr, candidates -> offsets) and the totals the
//            caller sizes the tables by (one small copy to the host);
//   fill   — the tables of gnnpn_eswoa_ragged_f64: cand_ptr, len_init, cand, start_pos.
// Every value is written with plain stores.  A problem the host path would raise on gets a status word instead (header).
#include "common.h"
#include "round5.h"

#include <climits>

namespace {

__device__ __forceinline__ bool same4(const double* a, const double* b) {   // Python tuple equality of floats (-0.0 == 0.0)
    return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3];
}

// exclusive prefix sum over the wave (every lane must call); *total = the sum of all lanes
__device__ __forceinline__ int wave_excl_scan(int v, int lane, int* total) {
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    *total = __shfl(x, 63);
    return x - v;
}

constexpr int ADDS_CATEGORIES = 50;   // addS sizes its per-category lists for 50 categories (loadData.py:156-163)

// The workspace of one call (gnnpn_woa_candidates_workspace_bytes): per NODE g (a slot is its task node) the paired row and
// the scan's results; per problem the counts.  Front and kept lists hold positions in the category (-1: the sentinel).
// With R replicas per problem (gnnpn_woa_candidates_replicas_*) "problem" below is a row q = b * R + r (B * R of them) and "node" a
// (replica, node) pair r * n_nodes + g (n_nodes * R of them): the tables of a problem's replicas differ (their pick sets do).
struct PrepWs {
    double* row;       // [N][4] rounded (and patched) action row paired with the slot's list
    int* front;        // [N][cap]
    int* kept;         // [N][cap]
    int* cat;          // [N]
    int* n_kept;       // [N] kept by addS (len_init)
    int* n_len;        // [N] with the appended row
    int* off;          // [N] offset of the list inside its problem's candidates
    int* rank;         // [N] position among the problem's non-empty lists, -1: empty (dropped)
    int* start;        // [N] start position, -1: no seed
    int* p_lists;      // [B]
    int* p_cand;       // [B]
    int* p_seeded;     // [B]
    int* cand_off;     // [B+1]
};

__host__ __device__ inline int64_t prep_ws_bytes(int64_t B, int64_t N, int64_t cap) {
    return N * 4 * (int64_t)sizeof(double) + (2 * N * cap + 6 * N + 4 * B + 1) * (int64_t)sizeof(int32_t);
}

__host__ __device__ inline PrepWs prep_ws(void* base, int64_t B, int64_t N, int64_t cap) {
    PrepWs w;
    w.row = reinterpret_cast<double*>(base);
    int* q = reinterpret_cast<int*>(w.row + N * 4);
    w.front = q; q += N * cap;
    w.kept = q; q += N * cap;
    w.cat = q; q += N;
    w.n_kept = q; q += N;
    w.n_len = q; q += N;
    w.off = q; q += N;
    w.rank = q; q += N;
    w.start = q; q += N;
    w.p_lists = q; q += B;
    w.p_cand = q; q += B;
    w.p_seeded = q; q += B;
    w.cand_off = q;
    return w;
}

__device__ __forceinline__ void load_member(int m, const double* qos_cat, double (&v)[4]) {
    if (m < 0) {                                               // the sentinel (1, 0, 1, 1) of loadData.py:164
        v[0] = 1.0; v[1] = 0.0; v[2] = 1.0; v[3] = 1.0;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = qos_cat[(size_t)m * 4 + c];
    }
}

__device__ __forceinline__ bool in_set(const double (&v)[4], const double* set, int n) {
    double k[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) k[c] = round5(v[c]);
    for (int i = 0; i < n; ++i)
        if (same4(k, set + (size_t)i * 4)) return true;
    return false;
}

// addS for one slot (loadData.py:166-197).  Returns the kept count, or -1 where the reference raises IndexError (a
// replacement at a position past the end of the kept list: possible once a pick was appended while the sentinel stood).
__device__ int adds_scan(const double* qos_cat, int n_srv, const double* lb, double reduct, const double* sset, int n_sset,
                         int* front, int* kept) {
    int nf = 1, nk = 0;
    front[0] = -1;
    for (int i = 0; i < n_srv; ++i) {
        const double* q = qos_cat + (size_t)i * 4;
        const double q0 = q[0], q1 = q[1], cost = q[2], quality = q[3];
        if (!(lb[0] <= cost && cost <= lb[1] && lb[2] <= quality && quality <= lb[3])) continue;
        if (reduct == 0.0) {
            kept[nk++] = i;
            continue;
        }
        bool replaced = false;
        for (int x = 0; x < nf; ++x) {
            double m[4];
            load_member(front[x], qos_cat, m);
            if (n_sset > 0 && in_set(m, sset, n_sset)) continue;
            if (q0 < m[0] && q1 > m[1] && m[1] < reduct) {
                front[x] = i;
                if (nk == 0) kept[nk++] = i;
                else if (x < nk) kept[x] = i;
                else return -1;
                replaced = true;
                break;
            }
            if ((q0 > m[0] && q1 < m[1]) || (q1 > reduct && reduct > q0)) break;
        }
        if (!replaced) {
            double v[4] = {q0, q1, cost, quality};
            if ((n_sset > 0 && in_set(v, sset, n_sset)) || (q1 > reduct && reduct > q0)) {
                front[nf++] = i;
                kept[nk++] = i;
            }
        }
    }
    return nk;
}

template <class A>
__global__ __launch_bounds__(64) void woa_count_kernel(int32_t N, int32_t R, const float* __restrict__ x, int32_t x_ld,
                                                       const int32_t* __restrict__ seg_ptr, const double* __restrict__ local_bounds,
                                                       const double* __restrict__ global_bounds, int32_t n_cat,
                                                       const int32_t* __restrict__ cat_ptr, const double* __restrict__ qos,
                                                       const A* __restrict__ actions, int32_t a_T, double reduct,
                                                       const double* __restrict__ patches, int32_t n_patches, int32_t cap, PrepWs w,
                                                       int32_t* __restrict__ n_slots, double* __restrict__ bounds,
                                                       int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double* sset = reinterpret_cast<double*>(lds_raw);         // [a_T][4] rounded rows (the pick set sSet)
    double* prow = sset + (size_t)a_T * 4;                     // [a_T][4] rounded rows after the patches (_prepare)
    // row rq = replica rq % R of problem b = rq / R: the row's own actions, outputs and workspace; the problem's x, segment and bounds
    const int rq = blockIdx.x, b = rq / R, lane = threadIdx.x;
    const int wq = (rq - b * R) * N;                            // the row's nodes in the workspace: wq + g
    const unsigned long long below = (1ull << lane) - 1ull;

    // the seed solution's rows: category order, dummy rows (float64 sum == 3) dropped (WOA.py:194-208)
    int n_rows = 0;
    for (int c0 = 0; c0 < a_T; c0 += 64) {
        const int c = c0 + lane;
        double r[4] = {0.0, 0.0, 0.0, 0.0};
        bool real = false;
        if (c < a_T) {
            const A* a = actions + ((size_t)rq * a_T + c) * 8;
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = (double)a[k];
            real = __dadd_rn(__dadd_rn(__dadd_rn(r[0], r[1]), r[2]), r[3]) != 3.0;
        }
        const unsigned long long m = __ballot(real);
        if (real) {
            double* s = sset + (size_t)(n_rows + __popcll(m & below)) * 4;
            double* t = prow + (size_t)(n_rows + __popcll(m & below)) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] = t[k] = round5(r[k]);
            for (int i = 0; i < n_patches; ++i) {              // _prepare's patches, in order
                const double* pt = patches + (size_t)i * 6;
                const int col = (int)pt[4];
                if (col >= 0 && col < 4 && same4(t, pt)) t[col] = pt[5];
            }
        }
        n_rows += __popcll(m);
    }
    __syncthreads();

    const int n0 = seg_ptr[b], n1 = seg_ptr[b + 1];
    const bool bad_segment = n0 < 0 || n1 < n0 || n1 > N;
    const int ns = !bad_segment && n1 - n0 > 1 ? n1 - n0 - 1 : 0;   // serviceIndex = the nodes after the first (loadData.py:251-257)
    int n_lists = 0;
    bool unsup = bad_segment, index_error = false;
    for (int s0 = 0; s0 < ns; s0 += 64) {
        const int s = s0 + lane;
        const int g = n0 + 1 + s;
        int nk = 0;
        if (s < ns) {
            const int cat = (int)x[(size_t)g * x_ld] - 1;
            w.cat[wq + g] = cat;
            if (cat < 0 || cat >= ADDS_CATEGORIES || cat >= n_cat) {
                unsup = true;
            } else {
                const int c0 = cat_ptr[cat];
                nk = adds_scan(qos + (size_t)c0 * 4, cat_ptr[cat + 1] - c0, local_bounds + ((size_t)b * n_cat + cat) * 4, reduct,
                               sset, n_rows, w.front + (size_t)(wq + g) * cap, w.kept + (size_t)(wq + g) * cap);
                if (nk < 0) {
                    index_error = true;
                    nk = 0;
                }
            }
            w.n_kept[wq + g] = nk;
        }
        const unsigned long long m = __ballot(nk > 0);
        if (s < ns) w.rank[wq + g] = nk > 0 ? n_lists + __popcll(m & below) : -1;
        n_lists += __popcll(m);
    }
    unsup = __ballot(unsup) != 0ull;
    index_error = __ballot(index_error) != 0ull;
    int st = GNNPN_WOA_OK;
    if (unsup) st = GNNPN_E_UNSUP;
    else if (index_error) st = GNNPN_WOA_INDEX_ERROR;
    else if (n_rows > 0 && n_rows != n_lists) st = GNNPN_WOA_ROWS_MISMATCH;
    else if (n_lists == 0) st = GNNPN_WOA_NO_SLOTS;
    const bool seeded = n_rows > 0;

    // pairing by position, rounding, the appended row, start positions, and each list's offset
    int n_cand = 0;
    for (int s0 = 0; s0 < ns && st == GNNPN_WOA_OK; s0 += 64) {
        const int s = s0 + lane;
        const int g = n0 + 1 + s;
        const int l = s < ns ? w.rank[wq + g] : -1;
        int len = 0;
        if (l >= 0) {
            const int nk = w.n_kept[wq + g];
            const double* qc = qos + (size_t)cat_ptr[w.cat[wq + g]] * 4;
            len = nk;
            int start = -1;
            if (seeded) {
                const double* key = prow + (size_t)l * 4;
                for (int i = 0; i < nk && start < 0; ++i) {
                    const double* q = qc + (size_t)w.kept[(size_t)(wq + g) * cap + i] * 4;
                    double v[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[c] = round5(q[c]);
                    if (same4(v, key)) start = i;
                }
                if (start < 0) {                               // a foreign pick: appended (WOA.py:62-69)
                    start = nk;
                    len = nk + 1;
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) w.row[(size_t)(wq + g) * 4 + c] = key[c];
            }
            w.n_len[wq + g] = len;
            w.start[wq + g] = start;
        }
        int total;
        const int off = wave_excl_scan(len, lane, &total);
        if (l >= 0) w.off[wq + g] = n_cand + off;
        n_cand += total;
    }
    if (lane == 0) {
        const bool ok = st == GNNPN_WOA_OK;
        w.p_lists[rq] = ok ? n_lists : 0;
        w.p_cand[rq] = ok ? n_cand : 0;
        w.p_seeded[rq] = seeded ? 1 : 0;
        n_slots[rq] = ok ? n_lists : 0;
        status[rq] = st;
    }
    if (lane < 4) bounds[(size_t)rq * 4 + lane] = global_bounds[(size_t)b * 4 + lane];   // constraintsList (loadData.py:268-273)
}

// exclusive scans over the problems; totals = {lists, candidates, max lists of a problem, max candidates of a problem,
// problems with a non-zero status, the first of them or -1}
constexpr int SCAN_THREADS = 256;
__global__ __launch_bounds__(SCAN_THREADS) void woa_scan_kernel(int32_t B, PrepWs w, const int32_t* __restrict__ status,
                                                                 int32_t* __restrict__ prob_ptr, int32_t* __restrict__ totals) {
    __shared__ int part_l[SCAN_THREADS], part_c[SCAN_THREADS], part_ml[SCAN_THREADS], part_mc[SCAN_THREADS];
    __shared__ int part_bad[SCAN_THREADS], part_first[SCAN_THREADS];
    const int t = threadIdx.x;
    const int per = (B + SCAN_THREADS - 1) / SCAN_THREADS;
    const int lo = t * per < B ? t * per : B, hi = lo + per < B ? lo + per : B;
    int sl = 0, sc = 0, ml = 0, mc = 0, bad = 0, first = -1;
    for (int b = lo; b < hi; ++b) {
        sl += w.p_lists[b];
        sc += w.p_cand[b];
        ml = max(ml, w.p_lists[b]);
        mc = max(mc, w.p_cand[b]);
        if (status[b] != GNNPN_WOA_OK) {
            if (first < 0) first = b;
            ++bad;
        }
    }
    part_l[t] = sl; part_c[t] = sc; part_ml[t] = ml; part_mc[t] = mc; part_bad[t] = bad; part_first[t] = first;
    __syncthreads();
    if (t == 0) {                                              // 256 partials: sequential is plenty
        int al = 0, ac = 0, aml = 0, amc = 0, abad = 0, afirst = -1;
        for (int i = 0; i < SCAN_THREADS; ++i) {
            const int l = part_l[i], c = part_c[i];
            part_l[i] = al; part_c[i] = ac;
            al += l; ac += c;
            aml = max(aml, part_ml[i]);
            amc = max(amc, part_mc[i]);
            abad += part_bad[i];
            if (afirst < 0) afirst = part_first[i];
        }
        totals[0] = al; totals[1] = ac; totals[2] = aml; totals[3] = amc; totals[4] = abad; totals[5] = afirst;
        prob_ptr[B] = al;
        w.cand_off[B] = ac;
    }
    __syncthreads();
    int al = part_l[t], ac = part_c[t];
    for (int b = lo; b < hi; ++b) {
        prob_ptr[b] = al;
        w.cand_off[b] = ac;
        al += w.p_lists[b];
        ac += w.p_cand[b];
    }
}

__global__ __launch_bounds__(64) void woa_fill_kernel(int32_t B, int32_t N, int32_t R, const int32_t* __restrict__ seg_ptr, const int32_t* __restrict__ cat_ptr,
                                                      const double* __restrict__ qos, int32_t cap, PrepWs w,
                                                      const int32_t* __restrict__ status, const int32_t* __restrict__ prob_ptr,
                                                      int32_t n_lists, int32_t n_cand, int32_t* __restrict__ cand_ptr,
                                                      int32_t* __restrict__ len_init, double* __restrict__ cand,
                                                      int32_t* __restrict__ start_pos) {
    const int rq = blockIdx.x, b = rq / R, lane = threadIdx.x;   // B rows here: row rq of problem b, as in woa_count_kernel
    const int wq = (rq - b * R) * N;
    if (rq == B - 1 && lane == 0 && prob_ptr[B] == n_lists) cand_ptr[n_lists] = w.cand_off[B];
    if (status[rq] != GNNPN_WOA_OK) return;
    const int n0 = seg_ptr[b], n1 = seg_ptr[b + 1];
    const int ns = n1 - n0 > 1 ? n1 - n0 - 1 : 0;             // a bad segment has a non-zero status: not reached
    const bool seeded = w.p_seeded[rq] != 0;
    for (int s = lane; s < ns; s += 64) {
        const int g = n0 + 1 + s;
        const int l = w.rank[wq + g];
        if (l < 0) continue;
        const int j = prob_ptr[rq] + l, off = w.cand_off[rq] + w.off[wq + g];
        const int nk = w.n_kept[wq + g], len = w.n_len[wq + g];
        if (j >= n_lists || off + len > n_cand) continue;      // never for the totals this call was sized by
        cand_ptr[j] = off;
        len_init[j] = nk;
        start_pos[j] = seeded ? w.start[wq + g] : -1;
        const double* qc = qos + (size_t)cat_ptr[w.cat[wq + g]] * 4;
        for (int i = 0; i < nk; ++i) {
            const double* q = qc + (size_t)w.kept[(size_t)(wq + g) * cap + i] * 4;
            double* o = cand + (size_t)(off + i) * 4;
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = seeded ? round5(q[c]) : q[c];
        }
        if (len > nk) {
            double* o = cand + (size_t)(off + nk) * 4;
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = w.row[(size_t)(wq + g) * 4 + c];
        }
    }
}

// Which services the tables of woa_fill_kernel consist of, from the same workspace: per list its task node (position inside
// the workflow graph, >= 1: node 0 is the request node) and category, per candidate the row of qos it was read from.  The
// appended foreign row is no row of qos: it gets the id the caller gave for the action row paired with its list (action_ids
// [rows, a_T], compacted as woa_count_kernel compacts the rows — dummy rows, float64 sum == 3, dropped; the ballot compaction is
// restated here so that the count kernel compiles to what it did), or -1.  One wavefront per row, plain stores only.
__global__ __launch_bounds__(64) void woa_services_kernel(int32_t N, int32_t R, const int32_t* __restrict__ seg_ptr,
                                                          const int32_t* __restrict__ cat_ptr, const void* __restrict__ actions,
                                                          int32_t actions_f64, int32_t a_T, const int32_t* __restrict__ action_ids,
                                                          int32_t cap, PrepWs w, const int32_t* __restrict__ status,
                                                          const int32_t* __restrict__ prob_ptr, int32_t n_lists, int32_t n_cand,
                                                          int32_t* __restrict__ slot_node, int32_t* __restrict__ slot_cat,
                                                          int32_t* __restrict__ cand_service) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    int* row_id = reinterpret_cast<int*>(lds_raw);             // [a_T] the ids of the rows that are no dummy rows
    const int rq = blockIdx.x, b = rq / R, lane = threadIdx.x;
    const int wq = (rq - b * R) * N;
    if (status[rq] != GNNPN_WOA_OK) return;
    const unsigned long long below = (1ull << lane) - 1ull;
    int n_rows = 0;
    for (int c0 = 0; c0 < a_T && action_ids; c0 += 64) {
        const int c = c0 + lane;
        bool real = false;
        if (c < a_T) {
            const size_t at = ((size_t)rq * a_T + c) * 8;
            double r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                r[k] = actions_f64 ? static_cast<const double*>(actions)[at + k] : (double)static_cast<const float*>(actions)[at + k];
            real = __dadd_rn(__dadd_rn(__dadd_rn(r[0], r[1]), r[2]), r[3]) != 3.0;
        }
        const unsigned long long m = __ballot(real);
        if (real) row_id[n_rows + __popcll(m & below)] = action_ids[(size_t)rq * a_T + c];
        n_rows += __popcll(m);
    }
    __syncthreads();
    const int n0 = seg_ptr[b], n1 = seg_ptr[b + 1];
    const int ns = n1 - n0 > 1 ? n1 - n0 - 1 : 0;             // a bad segment has a non-zero status: not reached
    for (int s = lane; s < ns; s += 64) {
        const int g = n0 + 1 + s;
        const int l = w.rank[wq + g];
        if (l < 0) continue;
        const int j = prob_ptr[rq] + l, off = w.cand_off[rq] + w.off[wq + g];
        const int nk = w.n_kept[wq + g], len = w.n_len[wq + g];
        if (j >= n_lists || off + len > n_cand) continue;      // never for the totals this call was sized by
        const int cat = w.cat[wq + g];
        slot_node[j] = g - n0;
        slot_cat[j] = cat;
        for (int i = 0; i < nk; ++i) cand_service[off + i] = cat_ptr[cat] + w.kept[(size_t)(wq + g) * cap + i];
        if (len > nk) cand_service[off + nk] = l < n_rows ? row_id[l] : -1;
    }
}

__global__ void round5_kernel(const double* __restrict__ x, double* __restrict__ y, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = round5(x[i]);
}

size_t count_lds_bytes(int a_T) { return (size_t)a_T * 8 * sizeof(double); }

// B problems x R replicas: the kernels count rows and (replica, node) pairs in int32
bool rows_fit(int64_t B, int64_t R, int64_t n_nodes) { return B * R <= INT32_MAX && n_nodes * R <= INT32_MAX; }

// One launcher for the per-problem entries (R = 1) and the per-replica ones: B * R rows, the workspace of B * R rows over
// n_nodes * R (replica, node) pairs.  `who` names the entry in the messages.
int count_launch(const char* who, int32_t B, int32_t R, int32_t n_nodes, const float* x, int32_t x_ld, const int32_t* seg_ptr,
                 const double* local_bounds, const double* global_bounds, int32_t n_cat, const int32_t* cat_ptr, const double* qos,
                 const void* actions, int32_t actions_f64, int32_t actions_T, double reduct, const double* patches, int32_t n_patches,
                 int32_t max_cat_size, void* workspace, int64_t workspace_bytes, int32_t* prob_ptr, int32_t* n_slots, double* bounds,
                 int32_t* status, int32_t* totals, void* stream) {
    GNNPN_REQUIRE(B >= 0 && R >= 1 && n_nodes >= 0 && x_ld >= 1 && n_cat >= 1 && actions_T >= 1 && n_patches >= 0 && max_cat_size >= 0 &&
                  (actions_f64 == 0 || actions_f64 == 1), "%s: bad argument", who);
    GNNPN_REQUIRE(rows_fit(B, R, n_nodes), "%s: bad argument: %d problems / %d nodes x %d replicas exceed int32", who, B, n_nodes, R);
    GNNPN_REQUIRE(prob_ptr && totals && cat_ptr && qos, "%s: null operand", who);
    GNNPN_REQUIRE(B == 0 || (x && seg_ptr && local_bounds && global_bounds && actions && n_slots && bounds && status),
                  "%s: null operand", who);
    GNNPN_REQUIRE(n_patches == 0 || patches, "%s: null patches", who);
    const int32_t rows = B * R;
    const int64_t need = prep_ws_bytes(rows, (int64_t)n_nodes * R, (int64_t)max_cat_size + 1);
    GNNPN_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace of %lld B, %lld B needed", who, (long long)workspace_bytes,
                  (long long)need);
    GNNPN_REQUIRE(gnnpn_aligned(workspace, 8), "%s: misaligned workspace", who);
    const size_t lds = count_lds_bytes(actions_T);
    if (lds > 64 * 1024) GNNPN_FAIL(GNNPN_E_UNSUP, "%s: %d action rows per problem (at most 1024)", who, actions_T);
    const PrepWs w = prep_ws(workspace, rows, (int64_t)n_nodes * R, (int64_t)max_cat_size + 1);
    hipStream_t s = (hipStream_t)stream;
    if (rows > 0) {
        if (actions_f64)
            hipLaunchKernelGGL(woa_count_kernel<double>, dim3(rows), dim3(64), lds, s, n_nodes, R, x, x_ld, seg_ptr, local_bounds,
                               global_bounds, n_cat, cat_ptr, qos, static_cast<const double*>(actions), actions_T, reduct, patches,
                               n_patches, max_cat_size + 1, w, n_slots, bounds, status);
        else
            hipLaunchKernelGGL(woa_count_kernel<float>, dim3(rows), dim3(64), lds, s, n_nodes, R, x, x_ld, seg_ptr, local_bounds,
                               global_bounds, n_cat, cat_ptr, qos, static_cast<const float*>(actions), actions_T, reduct, patches,
                               n_patches, max_cat_size + 1, w, n_slots, bounds, status);
        GNNPN_CHECK_LAUNCH(who);
    }
    hipLaunchKernelGGL(woa_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, rows, w, status, prob_ptr, totals);
    GNNPN_CHECK_LAUNCH(who);
    return GNNPN_OK;
}

int fill_launch(const char* who, int32_t B, int32_t R, int32_t n_nodes, const int32_t* seg_ptr, const int32_t* cat_ptr, const double* qos,
                int32_t max_cat_size, const void* workspace, int64_t workspace_bytes, const int32_t* status, const int32_t* prob_ptr,
                int32_t n_lists, int32_t n_cand, int32_t* cand_ptr, int32_t* len_init, double* cand, int32_t* start_pos, void* stream) {
    GNNPN_REQUIRE(B >= 0 && R >= 1 && n_nodes >= 0 && max_cat_size >= 0 && n_lists >= 0 && n_cand >= 0, "%s: bad argument", who);
    GNNPN_REQUIRE(rows_fit(B, R, n_nodes), "%s: bad argument: %d problems / %d nodes x %d replicas exceed int32", who, B, n_nodes, R);
    GNNPN_REQUIRE(cand_ptr, "%s: null operand", who);
    if (B == 0) return GNNPN_OK;
    GNNPN_REQUIRE(seg_ptr && cat_ptr && qos && status && prob_ptr && (n_lists == 0 || (len_init && start_pos)) && (n_cand == 0 || cand),
                  "%s: null operand", who);
    const int32_t rows = B * R;
    const int64_t need = prep_ws_bytes(rows, (int64_t)n_nodes * R, (int64_t)max_cat_size + 1);
    GNNPN_REQUIRE(workspace && workspace_bytes >= need && gnnpn_aligned(workspace, 8), "%s: workspace of %lld B, %lld B needed", who,
                  (long long)workspace_bytes, (long long)need);
    const PrepWs w = prep_ws(const_cast<void*>(workspace), rows, (int64_t)n_nodes * R, (int64_t)max_cat_size + 1);
    hipLaunchKernelGGL(woa_fill_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, rows, n_nodes, R, seg_ptr, cat_ptr, qos,
                       max_cat_size + 1, w, status, prob_ptr, n_lists, n_cand, cand_ptr, len_init, cand, start_pos);
    GNNPN_CHECK_LAUNCH(who);
    return GNNPN_OK;
}

int services_launch(const char* who, int32_t B, int32_t R, int32_t n_nodes, const int32_t* seg_ptr, const int32_t* cat_ptr,
                    const void* actions, int32_t actions_f64, int32_t actions_T, const int32_t* action_ids, int32_t max_cat_size,
                    const void* workspace, int64_t workspace_bytes, const int32_t* status, const int32_t* prob_ptr, int32_t n_lists,
                    int32_t n_cand, int32_t* slot_node, int32_t* slot_cat, int32_t* cand_service, void* stream) {
    GNNPN_REQUIRE(B >= 0 && R >= 1 && n_nodes >= 0 && max_cat_size >= 0 && n_lists >= 0 && n_cand >= 0 && actions_T >= 1 &&
                  (actions_f64 == 0 || actions_f64 == 1), "%s: bad argument", who);
    GNNPN_REQUIRE(rows_fit(B, R, n_nodes), "%s: bad argument: %d problems / %d nodes x %d replicas exceed int32", who, B, n_nodes, R);
    if (B == 0) return GNNPN_OK;
    GNNPN_REQUIRE(seg_ptr && cat_ptr && status && prob_ptr && (!action_ids || actions) && (n_lists == 0 || (slot_node && slot_cat)) &&
                  (n_cand == 0 || cand_service), "%s: null operand", who);
    const int32_t rows = B * R;
    const int64_t need = prep_ws_bytes(rows, (int64_t)n_nodes * R, (int64_t)max_cat_size + 1);
    GNNPN_REQUIRE(workspace && workspace_bytes >= need && gnnpn_aligned(workspace, 8), "%s: workspace of %lld B, %lld B needed", who,
                  (long long)workspace_bytes, (long long)need);
    const size_t lds = (size_t)actions_T * sizeof(int32_t);
    if (lds > 64 * 1024) GNNPN_FAIL(GNNPN_E_UNSUP, "%s: %d action rows per problem (at most 1024)", who, actions_T);
    const PrepWs w = prep_ws(const_cast<void*>(workspace), rows, (int64_t)n_nodes * R, (int64_t)max_cat_size + 1);
    hipLaunchKernelGGL(woa_services_kernel, dim3(rows), dim3(64), lds, (hipStream_t)stream, n_nodes, R, seg_ptr, cat_ptr, actions,
                       actions_f64, actions_T, action_ids, max_cat_size + 1, w, status, prob_ptr, n_lists, n_cand, slot_node, slot_cat,
                       cand_service);
    GNNPN_CHECK_LAUNCH(who);
    return GNNPN_OK;
}

}  // namespace

extern "C" int gnnpn_woa_candidates_replicas_services(int32_t B, int32_t R, int32_t n_nodes, const int32_t* seg_ptr,
                                                      const int32_t* cat_ptr, const void* actions, int32_t actions_f64,
                                                      int32_t actions_T, const int32_t* action_ids, int32_t max_cat_size,
                                                      const void* workspace, int64_t workspace_bytes, const int32_t* status,
                                                      const int32_t* prob_ptr, int32_t n_lists, int32_t n_cand, int32_t* slot_node,
                                                      int32_t* slot_cat, int32_t* cand_service, void* stream) {
    return services_launch("woa_candidates_replicas_services", B, R, n_nodes, seg_ptr, cat_ptr, actions, actions_f64, actions_T, action_ids,
                           max_cat_size, workspace, workspace_bytes, status, prob_ptr, n_lists, n_cand, slot_node, slot_cat, cand_service,
                           stream);
}

extern "C" int gnnpn_woa_candidates_services(int32_t B, int32_t n_nodes, const int32_t* seg_ptr, const int32_t* cat_ptr,
                                             const void* actions, int32_t actions_f64, int32_t actions_T, const int32_t* action_ids,
                                             int32_t max_cat_size, const void* workspace, int64_t workspace_bytes, const int32_t* status,
                                             const int32_t* prob_ptr, int32_t n_lists, int32_t n_cand, int32_t* slot_node,
                                             int32_t* slot_cat, int32_t* cand_service, void* stream) {
    return services_launch("woa_candidates_services", B, 1, n_nodes, seg_ptr, cat_ptr, actions, actions_f64, actions_T, action_ids,
                           max_cat_size, workspace, workspace_bytes, status, prob_ptr, n_lists, n_cand, slot_node, slot_cat, cand_service,
                           stream);
}

extern "C" int64_t gnnpn_woa_candidates_replicas_workspace_bytes(int32_t B, int32_t R, int32_t n_nodes, int32_t max_cat_size) {
    if (B < 0 || R < 1 || n_nodes < 0 || max_cat_size < 0 || !rows_fit(B, R, n_nodes)) return -1;
    return prep_ws_bytes((int64_t)B * R, (int64_t)n_nodes * R, (int64_t)max_cat_size + 1);
}

extern "C" int64_t gnnpn_woa_candidates_workspace_bytes(int32_t B, int32_t n_nodes, int32_t max_cat_size) {
    return gnnpn_woa_candidates_replicas_workspace_bytes(B, 1, n_nodes, max_cat_size);
}

extern "C" int gnnpn_woa_candidates_replicas_count(int32_t B, int32_t R, int32_t n_nodes, const float* x, int32_t x_ld,
                                                   const int32_t* seg_ptr, const double* local_bounds, const double* global_bounds,
                                                   int32_t n_cat, const int32_t* cat_ptr, const double* qos, const void* actions,
                                                   int32_t actions_f64, int32_t actions_T, double reduct, const double* patches,
                                                   int32_t n_patches, int32_t max_cat_size, void* workspace, int64_t workspace_bytes,
                                                   int32_t* prob_ptr, int32_t* n_slots, double* bounds, int32_t* status, int32_t* totals,
                                                   void* stream) {
    return count_launch("woa_candidates_replicas_count", B, R, n_nodes, x, x_ld, seg_ptr, local_bounds, global_bounds, n_cat, cat_ptr, qos,
                        actions, actions_f64, actions_T, reduct, patches, n_patches, max_cat_size, workspace, workspace_bytes, prob_ptr,
                        n_slots, bounds, status, totals, stream);
}

extern "C" int gnnpn_woa_candidates_count(int32_t B, int32_t n_nodes, const float* x, int32_t x_ld, const int32_t* seg_ptr,
                                          const double* local_bounds, const double* global_bounds, int32_t n_cat,
                                          const int32_t* cat_ptr, const double* qos, const void* actions, int32_t actions_f64,
                                          int32_t actions_T, double reduct, const double* patches, int32_t n_patches,
                                          int32_t max_cat_size, void* workspace, int64_t workspace_bytes, int32_t* prob_ptr,
                                          int32_t* n_slots, double* bounds, int32_t* status, int32_t* totals, void* stream) {
    return count_launch("woa_candidates_count", B, 1, n_nodes, x, x_ld, seg_ptr, local_bounds, global_bounds, n_cat, cat_ptr, qos, actions,
                        actions_f64, actions_T, reduct, patches, n_patches, max_cat_size, workspace, workspace_bytes, prob_ptr, n_slots,
                        bounds, status, totals, stream);
}

extern "C" int gnnpn_woa_candidates_replicas_fill(int32_t B, int32_t R, int32_t n_nodes, const int32_t* seg_ptr, const int32_t* cat_ptr,
                                                  const double* qos, int32_t max_cat_size, const void* workspace, int64_t workspace_bytes,
                                                  const int32_t* status, const int32_t* prob_ptr, int32_t n_lists, int32_t n_cand,
                                                  int32_t* cand_ptr, int32_t* len_init, double* cand, int32_t* start_pos, void* stream) {
    return fill_launch("woa_candidates_replicas_fill", B, R, n_nodes, seg_ptr, cat_ptr, qos, max_cat_size, workspace, workspace_bytes, status,
                       prob_ptr, n_lists, n_cand, cand_ptr, len_init, cand, start_pos, stream);
}

extern "C" int gnnpn_woa_candidates_fill(int32_t B, int32_t n_nodes, const int32_t* seg_ptr, const int32_t* cat_ptr, const double* qos,
                                         int32_t max_cat_size, const void* workspace, int64_t workspace_bytes, const int32_t* status,
                                         const int32_t* prob_ptr, int32_t n_lists, int32_t n_cand, int32_t* cand_ptr,
                                         int32_t* len_init, double* cand, int32_t* start_pos, void* stream) {
    return fill_launch("woa_candidates_fill", B, 1, n_nodes, seg_ptr, cat_ptr, qos, max_cat_size, workspace, workspace_bytes, status, prob_ptr,
                       n_lists, n_cand, cand_ptr, len_init, cand, start_pos, stream);
}

extern "C" int gnnpn_debug_round5_f64(const double* x, double* y, int64_t n, void* stream) {
    GNNPN_REQUIRE(n >= 0, "debug_round5: bad argument");
    if (n == 0) return GNNPN_OK;
    GNNPN_REQUIRE(x && y, "debug_round5: null operand");
    hipLaunchKernelGGL(round5_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, n);
    GNNPN_CHECK_LAUNCH("debug_round5_f64");
    return GNNPN_OK;
}
