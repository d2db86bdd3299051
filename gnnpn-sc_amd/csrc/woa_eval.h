// The float64 evaluation orders of the ES-WOA figure of merit, shared by the searches over it (woa.hip: ES-WOA, descend.hip:
// one-swap descent): violate + objFunc of a composition exactly as numpy evaluates it in oracle/woa.py `objective` — np.cumprod =
// one sequential chain per QoS column, np.sum = the 8-accumulator pairwise block up to 128 terms and numpy's recursion above,
// np.min exact — and the shape of a (ragged) batch of problems.
#pragma once
#include "common.h"

namespace {
__device__ __forceinline__ double wave_bcast(double v, int lane) {
    const int lo = __shfl(__double2loint(v), lane), hi = __shfl(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// violate + objFunc from the five figures of a composition: the two cumprod ends against their bounds, and
// (np.sum / serviceNum + 1 - np.min) / 2 with one rounding per operation.
__device__ __forceinline__ double merit_of(double sum, int n_real, double mn, double prod2, double prod3, const double* bounds) {
    int violate = 0;
    if (prod2 < bounds[0] || prod2 > bounds[1]) ++violate;
    if (prod3 < bounds[2] || prod3 > bounds[3]) ++violate;
    double obj = sum / (double)n_real;
    obj = __dadd_rn(obj, 1.0);
    obj = __dsub_rn(obj, mn);
    obj = obj / 2.0;
    return __dadd_rn((double)violate, obj);
}

// np.sum's block (pairwise_sum, n <= 128: n < 8 sequential; else eight accumulators, their tree, the tail), stated twice: by one
// wave over a[0..n-1], the result in every lane, and (pw_leaf_swapped) by ONE thread with a[jj] replaced by v.
__device__ double pw_leaf(const double* a, int n, int lane) {
    double sum = 0.0;
    if (n < 8) {
        if (lane == 0) {
            sum = a[0];
            for (int i = 1; i < n; ++i) sum = __dadd_rn(sum, a[i]);
        }
        return wave_bcast(sum, 0);
    }
    double r = 0.0;
    const int body = n - (n % 8);
    if (lane < 8) {
        r = a[lane];
        for (int i = 8; i < body; i += 8) r = __dadd_rn(r, a[i + lane]);
    }
    const double r0 = wave_bcast(r, 0), r1 = wave_bcast(r, 1), r2 = wave_bcast(r, 2), r3 = wave_bcast(r, 3);
    const double r4 = wave_bcast(r, 4), r5 = wave_bcast(r, 5), r6 = wave_bcast(r, 6), r7 = wave_bcast(r, 7);
    sum = __dadd_rn(__dadd_rn(__dadd_rn(r0, r1), __dadd_rn(r2, r3)), __dadd_rn(__dadd_rn(r4, r5), __dadd_rn(r6, r7)));
    for (int i = body; i < n; ++i) sum = __dadd_rn(sum, a[i]);
    return sum;
}
// pw_leaf_swapped: a[jj] replaced by v and a[kk] by w (kk < 0: one element only).
__device__ __forceinline__ double pw_leaf_swapped(const double* a, int n, int jj, double v, int kk, double w) {
    auto at = [&](int i) { return i == jj ? v : i == kk ? w : a[i]; };
    if (n < 8) {
        double s = at(0);
        for (int i = 1; i < n; ++i) s = __dadd_rn(s, at(i));
        return s;
    }
    double r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = at(k);
    const int body = n - (n % 8);
    for (int i = 8; i < body; i += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = __dadd_rn(r[k], at(i + k));
    }
    double s = __dadd_rn(__dadd_rn(__dadd_rn(r[0], r[1]), __dadd_rn(r[2], r[3])), __dadd_rn(__dadd_rn(r[4], r[5]), __dadd_rn(r[6], r[7])));
    for (int i = body; i < n; ++i) s = __dadd_rn(s, at(i));
    return s;
}
__device__ double pw_leaf_swapped(const double* a, int n, int jj, double v) { return pw_leaf_swapped(a, n, jj, v, -1, 0.0); }

// violate + objFunc of the composition whose category-j row is (q[0..3]) in lane j (lanes >= T idle).
// `col` = 4 x 64 doubles of LDS scratch, which holds the composition's four columns afterwards.
__device__ double figure_of_merit(const double (&q)[4], int T, int lane, double* col, const double* bounds) {
    if (lane < T) {
#pragma unroll
        for (int c = 0; c < 4; ++c) col[c * 64 + lane] = q[c];
    }
    __syncthreads();
    // np.cumprod of columns 2 and 3: lanes 0 and 1 run the two sequential chains
    double prod = 1.0;
    if (lane < 2) {
        const double* a = col + (2 + lane) * 64;
        prod = a[0];
        for (int i = 1; i < T; ++i) prod = __dmul_rn(prod, a[i]);
    }
    const double sum = pw_leaf(col, T, lane);                         // np.sum of column 0: T <= 64 is one block
    const double prod2 = wave_bcast(prod, 0), prod3 = wave_bcast(prod, 1);
    // serviceNum and np.min(column 1): exact reductions
    const unsigned long long real = __ballot(lane < T && q[0] > 0.0);
    const int n_real = __popcll(real);
    double mn = lane < T ? q[1] : INFINITY;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = fmin(mn, wave_bcast(mn, (lane + o) & 63));
    mn = wave_bcast(mn, 0);
    const double f = merit_of(sum, n_real, mn, prod2, prod3, bounds);
    __syncthreads();
    return f;
}

__device__ __forceinline__ void gather_row(const double* cand, int base, int len, int pos, double (&q)[4]) {
    const int idx = base + (pos < 0 ? pos + len : pos);      // Python list indexing
#pragma unroll
    for (int c = 0; c < 4; ++c) q[c] = cand[(size_t)idx * 4 + c];
}
}  // namespace

// Where a problem's categories come from: ONE shape for every entry point.  Problem p owns entries first(p) .. first(p) +
// count(p) - 1 of cand_ptr / len_init / start_pos and row p (of `stride` entries) of best_pos / best_rows.  prob_ptr [B+1] gives a
// ragged batch (gnnpn_eswoa_ragged_f64, gnnpn_descend_ragged_f64: problem p owns prob_ptr[p] .. prob_ptr[p+1]-1); prob_ptr == NULL is the same launch with
// uniform counts (gnnpn_eswoa_f64, gnnpn_eswoa_wide_f64: T categories each, stride = T, the host has checked T).  Either way a
// problem that does not fit what the launch was sized for is not searched (fits, fits_cand: best_fitness NaN, draws -1, no LDS
// touched), and the best composition's rows are written where best_rows is given.
struct Shape {
    const int32_t* prob_ptr;   // [B+1], or NULL: every problem has T categories
    int32_t T;                 // categories per problem where prob_ptr is NULL
    int32_t stride;            // row length of best_pos / best_rows, and the largest count the launch is sized for
    int32_t max_T;             // 64 for the lane-per-category form, stride for the workgroup form
    int32_t max_cand;          // lane-per-category form: candidates of the largest problem (LDS); workgroup form: 0, unused
    int32_t n_lists;           // entries of len_init / start_pos (cand_ptr has one more)
    double* best_rows;         // [B, stride, 4] or NULL
    __device__ __forceinline__ int count(int p) const { return prob_ptr ? prob_ptr[p + 1] - prob_ptr[p] : T; }
    __device__ __forceinline__ size_t first(int p) const { return prob_ptr ? (size_t)prob_ptr[p] : (size_t)p * T; }
    __device__ __forceinline__ size_t out_row(int p) const { return (size_t)p * stride; }
    __device__ __forceinline__ bool fits(int p, int n) const {
        return !prob_ptr || (n >= 1 && n <= max_T && n <= stride && prob_ptr[p] >= 0 && prob_ptr[p + 1] <= n_lists);
    }
    __device__ __forceinline__ bool fits_cand(int n_cand) const { return max_cand <= 0 || n_cand <= max_cand; }
    __device__ __forceinline__ double* rows_out(int p) const { return best_rows ? best_rows + (size_t)p * stride * 4 : nullptr; }
};

namespace {
constexpr int WNT = 256;

// What a problem that is not searched leaves behind, by every thread of its workgroup (tid of nt).  ES-WOA: nothing else is touched.
__device__ __forceinline__ void not_searched(int p, int tid, double* best_fitness, long long* draws) {
    if (tid != 0) return;
    best_fitness[p] = NAN;
    draws[p] = -1;
}
// Descent: the history row is NaN too, so no entry of it is left unwritten.
__device__ __forceinline__ void not_searched(int p, int tid, int nt, double* best_fitness, double* start_fitness, double* history,
                                             int hist_ld, int32_t* sweeps, int32_t* moves) {
    for (int s = tid; s < hist_ld; s += nt) history[(size_t)p * hist_ld + s] = NAN;
    if (tid != 0) return;
    best_fitness[p] = NAN;
    start_fitness[p] = NAN;
    sweeps[p] = -1;
    moves[p] = 0;
}

// np.sum of n doubles (pairwise_sum): post-order walk of the recursion with an explicit stack (depth <= log2(n / 128) + 1)
__device__ double pw_sum(const double* a, int n, int lane) {
    int off[24], len[24], st[24];
    double left[24];
    int sp = 0;
    off[0] = 0; len[0] = n; st[0] = 0; left[0] = 0.0;
    double ret = 0.0;
    sp = 1;
    while (sp > 0) {
        const int f = sp - 1;
        if (len[f] <= 128) {
            ret = pw_leaf(a + off[f], len[f], lane);
            --sp;
        } else {
            int n2 = len[f] / 2;
            n2 -= n2 % 8;
            if (st[f] == 0) {
                st[f] = 1;
                off[sp] = off[f]; len[sp] = n2; st[sp] = 0;
                ++sp;
            } else if (st[f] == 1) {
                left[f] = ret;
                st[f] = 2;
                off[sp] = off[f] + n2; len[sp] = len[f] - n2; st[sp] = 0;
                ++sp;
            } else {
                ret = __dadd_rn(left[f], ret);
                --sp;
            }
        }
    }
    return ret;
}

struct WideLds {
    double* col0;      // [T] column 0 (np.sum)
    double* col2;      // [T] column 2 (np.cumprod)
    double* col3;      // [T]
    double* red;       // [8]: min per wave (4), results: sum, prod2, prod3
    int* cnt;          // [4] real services per wave
    int* base;         // [T]
    int* len;          // [T]
    double* bounds;    // [4]
    // The carve-up of a problem's dynamic LDS, the one statement of the layout the host's *_wide_lds_bytes size: the doubles
    // (three columns, red, bounds, then `extra` more for the caller, returned), then the ints.  Host code too: descend.hip sizes
    // its launches by carving a null base.
    __host__ __device__ __forceinline__ double* carve(unsigned char* raw, int T, size_t extra = 0) {
        col0 = reinterpret_cast<double*>(raw);
        col2 = col0 + T;
        col3 = col2 + T;
        red = col3 + T;
        bounds = red + 8;
        double* more = bounds + 4;
        cnt = reinterpret_cast<int*>(more + extra);
        base = cnt + 4;
        len = base + T;
        return more;
    }
};

// figure of merit of the composition pos[j] (j < T), every thread returns it
__device__ double wide_merit(const WideLds& L, const int* pos, const double* cand, int T, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    double mn = INFINITY;
    int real = 0;
    for (int j = tid; j < T; j += WNT) {
        const int x = pos[j], ln = L.len[j];
        const double* q = cand + (size_t)(L.base[j] + (x < 0 ? x + ln : x)) * 4;
        const double q0 = q[0], q1 = q[1];
        L.col0[j] = q0;
        L.col2[j] = q[2];
        L.col3[j] = q[3];
        mn = fmin(mn, q1);
        real += q0 > 0.0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fmin(mn, wave_bcast(mn, (lane + o) & 63));
        real += __shfl(real, (lane + o) & 63);
    }
    if (lane == 0) {
        L.red[wave] = mn;
        L.cnt[wave] = real;
    }
    __syncthreads();
    if (wave == 0) {
        if (lane < 2) {                                   // np.cumprod: one sequential chain per column
            const double* a = lane == 0 ? L.col2 : L.col3;
            double prod = a[0];
            for (int i = 1; i < T; ++i) prod = __dmul_rn(prod, a[i]);
            L.red[5 + lane] = prod;
        }
    } else if (wave == 1) {
        const double sum = pw_sum(L.col0, T, lane);
        if (lane == 0) L.red[4] = sum;
    }
    __syncthreads();
    const double sum = L.red[4], prod2 = L.red[5], prod3 = L.red[6];
    mn = fmin(fmin(L.red[0], L.red[1]), fmin(L.red[2], L.red[3]));
    const int n_real = L.cnt[0] + L.cnt[1] + L.cnt[2] + L.cnt[3];
    const double f = merit_of(sum, n_real, mn, prod2, prod3, L.bounds);
    __syncthreads();                                      // the columns and red[] are free again
    return f;
}

// The one launch of a search kernel (host side): one workgroup of `nt` threads per problem with `lds` bytes of dynamic LDS.  Above
// what a CU can give, `too_large` writes the entry point's message and returns its code; nothing is launched then.
template <class TooLarge, typename... P, typename... A>
int search_launch(size_t lds, TooLarge too_large, void (*kernel)(P...), int32_t B, int nt, void* stream, const char* entry,
                  const A&... args) {
    if (lds > 160 * 1024 - 1024) return too_large();
    const int rc = gnnpn_launch_lds(kernel, dim3(B), dim3(nt), lds, (hipStream_t)stream, entry, args...);
    if (rc != GNNPN_OK) return rc;
    GNNPN_CHECK_LAUNCH(entry);
    return GNNPN_OK;
}
}  // namespace
