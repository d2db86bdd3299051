// ES-WOA fine-tuner (reference src/baselines/WOA.py:8-162), one wavefront per problem.
//
// The search is sequential in the individuals (every accepted individual moves the recorded best that the next one is
// attracted to) and its random draws are consumed in a data-dependent order, so the parallelism is across problems
// (embarrassingly: 1000 test problems = 1000 waves) and, inside a problem, across the T service categories: lane j owns
// category j's position of every individual.  All state of a problem lives in LDS (positions pop x T int32, the
// problem's candidate table n x 4 float64).
//
// Every draw is draw k of the counter-based stream of oracle/woa.py (splitmix64 of seed + k*golden), so a run is a pure
// function of (inputs, seed) and can be compared draw for draw with the restatement that is pinned against the real
// reference class.  The float64 figure of merit reproduces numpy's evaluation orders: np.cumprod = one sequential
// chain per QoS column, np.sum = the 8-accumulator pairwise block (n <= 128), np.min exact.  Python semantics restated:
// round-half-even (rint), modulo with the divisor's sign, negative positions index from the end, and the reference's
// list aliasing between the recorded best and the individual it was taken from (`alias`).
#include "woa_eval.h"

namespace {
constexpr double PE = 0.2;
constexpr unsigned long long GOLDEN = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ double draw_uniform(unsigned long long seed, unsigned long long k) {
    unsigned long long z = seed + GOLDEN * k;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ int draw_below(unsigned long long seed, unsigned long long k, int n) {
    return (int)__dmul_rn(draw_uniform(seed, k), (double)n);
}
}  // namespace

__global__ __launch_bounds__(64) void eswoa_kernel(Shape sh, const int32_t* __restrict__ cand_ptr,
                                                   const int32_t* __restrict__ len_init, const double* __restrict__ cand_g,
                                                   const double* __restrict__ bounds_g, const int32_t* __restrict__ start_pos,
                                                   int32_t pop, int32_t max_iter, const unsigned long long* __restrict__ seeds,
                                                   double* __restrict__ best_fitness, int32_t* __restrict__ best_pos_out,
                                                   double* __restrict__ history, long long* __restrict__ draws_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int p = blockIdx.x, lane = threadIdx.x;
    const int T = sh.count(p);
    const size_t s0 = sh.first(p);
    const bool fits = sh.fits(p, T);
    const int c0 = fits ? cand_ptr[s0] : 0, n_cand = fits ? cand_ptr[s0 + T] - c0 : 0;
    if (!fits || !sh.fits_cand(n_cand)) {                             // not what the launch was sized for: no search
        not_searched(p, lane, best_fitness, draws_out);
        return;
    }
    double* col = reinterpret_cast<double*>(lds_raw);                 // [4][64]
    double* bounds = col + 256;                                       // [4]
    double* cand = bounds + 4;                                        // [n_cand][4]
    int* pos = reinterpret_cast<int*>(cand + (size_t)n_cand * 4);     // [pop][T]
    for (int i = lane; i < n_cand * 4; i += 64) cand[i] = cand_g[(size_t)c0 * 4 + i];
    if (lane < 4) bounds[lane] = bounds_g[(size_t)p * 4 + lane];
    const bool live = lane < T;
    const int base = live ? cand_ptr[s0 + lane] - c0 : 0;
    const int len = live ? cand_ptr[s0 + lane + 1] - cand_ptr[s0 + lane] : 1;
    const int len0 = live ? len_init[s0 + lane] : 1;
    const unsigned long long seed = seeds[p];
    unsigned long long k = 0;                                         // draws consumed so far (wave-uniform)
    __syncthreads();

    // initial population (WOA.py:51-52): individual i, category j <- draw k + i*T + j + 1, lengths BEFORE the append
    for (int i = 0; i < pop; ++i)
        if (live) pos[i * T + lane] = draw_below(seed, k + (unsigned long long)i * T + lane + 1, len0);
    k += (unsigned long long)pop * T;
    __syncthreads();

    double q[4] = {0.0, 0.0, 0.0, 0.0};
    double best_fit = 3.0;                                            // :71
    int best = 0;                                                     // this lane's category of the recorded best
    int alias = -1;                                                   // individual whose list the record shares
    if (start_pos[s0] >= 0) {                                         // :55-69
        best = live ? start_pos[s0 + lane] : 0;
        if (live) gather_row(cand, base, len, best, q);
        best_fit = figure_of_merit(q, T, lane, col, bounds);
    }
    for (int i = 0; i < pop; ++i) {                                   // :77-85
        const int x = live ? pos[i * T + lane] : 0;
        if (live) gather_row(cand, base, len, x, q);
        const double f = figure_of_merit(q, T, lane, col, bounds);
        if (best_fit > f) {
            best_fit = f;
            best = x;
            alias = i;
        }
    }

    for (int t = 0; t < max_iter; ++t) {                              // :107-161
        const double prob = __dmul_rn(0.2, __dsub_rn(1.0, (double)t / (double)max_iter));
        for (int i = 0; i < pop; ++i) {                               // global phase
            if (draw_uniform(seed, ++k) < prob) {
                const int j = draw_below(seed, ++k, T);
                const int kk = draw_below(seed, ++k, __shfl(len, j));
                if (lane == j) {
                    pos[i * T + lane] = kk;
                    if (alias == i) best = kk;                        // same list object in the reference
                }
                __syncthreads();
                const int x = live ? pos[i * T + lane] : 0;
                if (live) gather_row(cand, base, len, x, q);
                const double f = figure_of_merit(q, T, lane, col, bounds);
                if (best_fit > f) {
                    best_fit = f;
                    best = x;
                    alias = i;
                }
            }
        }
        if (PE > draw_uniform(seed, ++k)) {                           // :125-129
            if (lane == 0) history[(size_t)p * max_iter + t] = best_fit;
            continue;
        }
        const double a = __dsub_rn(2.0, __dmul_rn(2.0, (double)t) / (double)max_iter);
        for (int i = 0; i < pop; ++i) {                               // local phase
            const double r = draw_uniform(seed, ++k);
            const double A = __dsub_rn(__dmul_rn(__dmul_rn(2.0, a), r), a);
            const double C = __dmul_rn(2.0, r);
            const double l = draw_uniform(seed, ++k);
            const double pp = draw_uniform(seed, ++k);
            const int x = live ? pos[i * T + lane] : 0;
            bool moved = false;
            double nv = 0.0;
            if (pp < 0.5) {
                if (fabs(A) < 1.0) {                                  // round(b - A * (C*b - x))
                    moved = true;
                    nv = __dsub_rn((double)best, __dmul_rn(A, __dsub_rn(__dmul_rn(C, (double)best), (double)x)));
                }
            } else {                                                  // round((x - b) * e^l * cos(2 pi l) + b)
                moved = true;
                const double e = exp(l), c = cos(__dmul_rn(__dmul_rn(2.0, 3.141592653589793), l));
                nv = __dadd_rn(__dmul_rn(__dmul_rn((double)(x - best), e), c), (double)best);
            }
            if (moved) {
                long long nx = (long long)rint(nv);                   // Python round: half to even
                if (llabs(nx) >= len) {                               // Python %: sign of the divisor
                    nx %= len;
                    if (nx < 0) nx += len;
                }
                if (live) pos[i * T + lane] = (int)nx;
                if (alias == i) alias = -1;                           // rebinding: the record keeps the old list
                __syncthreads();
                if (live) gather_row(cand, base, len, (int)nx, q);
                const double f = figure_of_merit(q, T, lane, col, bounds);
                if (best_fit > f) {
                    best_fit = f;
                    best = (int)nx;
                    alias = i;
                }
            }
        }
        if (lane == 0) history[(size_t)p * max_iter + t] = best_fit;
    }
    if (live) best_pos_out[sh.out_row(p) + lane] = best;
    if (double* rows = sh.rows_out(p)) {                              // the recorded best's rows (Python indexing)
        if (live) {
            gather_row(cand, base, len, best, q);
#pragma unroll
            for (int c = 0; c < 4; ++c) rows[(size_t)lane * 4 + c] = q[c];
        }
    }
    if (lane == 0) {
        best_fitness[p] = best_fit;
        draws_out[p] = (long long)k;
    }
}

// ---- T > 64: one WORKGROUP (4 waves) per problem, thread tid owns categories tid, tid + 256, ... ---------------------------
// Same search, same draws, same float64 evaluation orders; what changes is where things live.  The positions of the
// population (pop x T int32: 800 KB at T = 2000, pop = 100) and the candidate table stay in global memory (L2), the
// recorded best IS the output row; LDS holds the three QoS columns of the composition under evaluation (np.sum needs
// column 0 as a whole — numpy's pairwise recursion splits at n/2 rounded down to a multiple of 8 until a block has at most
// 128 elements — and np.cumprod columns 2 and 3 in order) and the per-category base / length tables.  One evaluation = a
// parallel gather, then the two sequential product chains (lanes 0 and 1 of wave 0: T dependent multiplies each, the
// floor of this kernel — bit parity with np.cumprod leaves no other order) while wave 1 forms the pairwise sum.

__global__ __launch_bounds__(WNT) void eswoa_wide_kernel(Shape sh, const int32_t* __restrict__ cand_ptr,
                                                         const int32_t* __restrict__ len_init, const double* __restrict__ cand_g,
                                                         const double* __restrict__ bounds_g, const int32_t* __restrict__ start_pos,
                                                         int32_t pop, int32_t max_iter, const unsigned long long* __restrict__ seeds,
                                                         int32_t* __restrict__ pos_ws, double* __restrict__ best_fitness,
                                                         int32_t* __restrict__ best_pos_out, double* __restrict__ history,
                                                         long long* __restrict__ draws_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int T = sh.count(p);
    const size_t s0 = sh.first(p);
    if (!sh.fits(p, T)) {                                             // not what the launch was sized for: no search
        not_searched(p, tid, best_fitness, draws_out);
        return;
    }
    WideLds L;
    L.carve(lds_raw, T);
    const int c0 = cand_ptr[s0];
    const double* cand = cand_g + (size_t)c0 * 4;
    int* pos = pos_ws + (size_t)pop * s0;                 // [pop][T]
    int* best = best_pos_out + sh.out_row(p);             // the recorded best composition (a COPY: see `alias`)
    for (int j = tid; j < T; j += WNT) {
        L.base[j] = cand_ptr[s0 + j] - c0;
        L.len[j] = cand_ptr[s0 + j + 1] - cand_ptr[s0 + j];
    }
    if (tid < 4) L.bounds[tid] = bounds_g[(size_t)p * 4 + tid];
    const unsigned long long seed = seeds[p];
    unsigned long long k = 0;

    // initial population (WOA.py:51-52): individual i, category j <- draw k + i*T + j + 1, lengths BEFORE the append
    for (int i = 0; i < pop; ++i)
        for (int j = tid; j < T; j += WNT)
            pos[(size_t)i * T + j] = draw_below(seed, k + (unsigned long long)i * T + j + 1, len_init[s0 + j]);
    k += (unsigned long long)pop * T;
    __syncthreads();

    double best_fit = 3.0;                                            // :71
    int alias = -1;                                                   // individual whose list the record shares
    auto record = [&](int i) {                                        // best <- a copy of individual i
        for (int j = tid; j < T; j += WNT) best[j] = pos[(size_t)i * T + j];
        alias = i;
    };
    if (start_pos[s0] >= 0) {                                         // :55-69
        for (int j = tid; j < T; j += WNT) best[j] = start_pos[s0 + j];
        __syncthreads();
        best_fit = wide_merit(L, best, cand, T, tid);
    } else {
        for (int j = tid; j < T; j += WNT) best[j] = 0;
    }
    for (int i = 0; i < pop; ++i) {                                   // :77-85
        const double f = wide_merit(L, pos + (size_t)i * T, cand, T, tid);
        if (best_fit > f) {
            best_fit = f;
            record(i);
        }
    }
    __syncthreads();

    for (int t = 0; t < max_iter; ++t) {                              // :107-161
        const double prob = __dmul_rn(0.2, __dsub_rn(1.0, (double)t / (double)max_iter));
        for (int i = 0; i < pop; ++i) {                               // global phase
            if (draw_uniform(seed, ++k) < prob) {
                const int j = draw_below(seed, ++k, T);
                const int kk = draw_below(seed, ++k, L.len[j]);
                if (tid == 0) {
                    pos[(size_t)i * T + j] = kk;
                    if (alias == i) best[j] = kk;                     // same list object in the reference
                }
                __syncthreads();
                const double f = wide_merit(L, pos + (size_t)i * T, cand, T, tid);
                if (best_fit > f) {
                    best_fit = f;
                    record(i);
                    __syncthreads();
                }
            }
        }
        if (PE > draw_uniform(seed, ++k)) {                           // :125-129
            if (tid == 0) history[(size_t)p * max_iter + t] = best_fit;
            continue;
        }
        const double a = __dsub_rn(2.0, __dmul_rn(2.0, (double)t) / (double)max_iter);
        for (int i = 0; i < pop; ++i) {                               // local phase
            const double r = draw_uniform(seed, ++k);
            const double A = __dsub_rn(__dmul_rn(__dmul_rn(2.0, a), r), a);
            const double C = __dmul_rn(2.0, r);
            const double l = draw_uniform(seed, ++k);
            const double pp = draw_uniform(seed, ++k);
            const bool spiral = !(pp < 0.5);
            if (!spiral && !(fabs(A) < 1.0)) continue;
            const double e = exp(l), cs = cos(__dmul_rn(__dmul_rn(2.0, 3.141592653589793), l));
            for (int j = tid; j < T; j += WNT) {
                const int x = pos[(size_t)i * T + j], b = best[j], ln = L.len[j];
                double nv;
                if (!spiral) nv = __dsub_rn((double)b, __dmul_rn(A, __dsub_rn(__dmul_rn(C, (double)b), (double)x)));   // round(b - A (C b - x))
                else nv = __dadd_rn(__dmul_rn(__dmul_rn((double)(x - b), e), cs), (double)b);                             // round((x - b) e^l cos(2 pi l) + b)
                long long nx = (long long)rint(nv);                   // Python round: half to even
                if (llabs(nx) >= ln) {                                // Python %: sign of the divisor
                    nx %= ln;
                    if (nx < 0) nx += ln;
                }
                pos[(size_t)i * T + j] = (int)nx;
            }
            if (alias == i) alias = -1;                               // rebinding: the record keeps the old list
            __syncthreads();
            const double f = wide_merit(L, pos + (size_t)i * T, cand, T, tid);
            if (best_fit > f) {
                best_fit = f;
                record(i);
                __syncthreads();
            }
        }
        if (tid == 0) history[(size_t)p * max_iter + t] = best_fit;
    }
    if (double* rows = sh.rows_out(p)) {                              // the recorded best's rows (Python indexing)
        __syncthreads();
        for (int j = tid; j < T; j += WNT) {
            const int x = best[j], ln = L.len[j];
            const double* q = cand + (size_t)(L.base[j] + (x < 0 ? x + ln : x)) * 4;
            for (int c = 0; c < 4; ++c) rows[(size_t)j * 4 + c] = q[c];
        }
    }
    if (tid == 0) {
        best_fitness[p] = best_fit;
        draws_out[p] = (long long)k;
    }
}

// LDS bytes one problem needs (host side).  Workgroup form: three columns, red[8] + bounds[4], base / len tables, cnt[4].
// Lane form: scratch + bounds + its candidate table + the population's positions.
static size_t eswoa_wide_lds_bytes(int T) { return ((size_t)3 * T + 12) * sizeof(double) + ((size_t)2 * T + 4) * sizeof(int); }
static size_t eswoa_lds_bytes(int n_cand, int pop, int T) {
    return (256 + 4) * sizeof(double) + (size_t)n_cand * 4 * sizeof(double) + (size_t)pop * T * sizeof(int);
}

// The one launch of both forms (`wide`: the workgroup form, positions in `workspace`), sized for sh.stride categories per
// problem; `who` names the entry point in the messages, `entry` in a launch error (search_launch, woa_eval.h).
static int eswoa_launch(const char* who, const char* entry, bool wide, int32_t B, const Shape& sh, const int32_t* cand_ptr,
                        const int32_t* len_init, const double* cand, const double* bounds, const int32_t* start_pos, int32_t pop,
                        int32_t max_iter, const uint64_t* seeds, void* workspace, double* best_fitness, int32_t* best_pos,
                        double* history, int64_t* draws, void* stream) {
    const int T = sh.stride;
    const size_t lds = wide ? eswoa_wide_lds_bytes(T) : eswoa_lds_bytes(sh.max_cand, pop, T);
    auto too_large = [&]() -> int {
        if (wide)
            GNNPN_FAIL(GNNPN_E_UNSUP, "%s: %s%d categories need %zu B of LDS for the three QoS columns (a CU has 160 KB)", who,
                       sh.prob_ptr ? "" : "T=", T, lds);
        GNNPN_FAIL(GNNPN_E_UNSUP, "%s: %zu B of LDS per problem (population %d x %d, %d candidates) exceed a CU", who, lds, pop, T,
                   sh.max_cand);
    };
    const auto* sd = reinterpret_cast<const unsigned long long*>(seeds);
    auto* dr = reinterpret_cast<long long*>(draws);
    return wide ? search_launch(lds, too_large, eswoa_wide_kernel, B, WNT, stream, entry, sh, cand_ptr, len_init, cand, bounds, start_pos,
                                pop, max_iter, sd, reinterpret_cast<int32_t*>(workspace), best_fitness, best_pos, history, dr)
                : search_launch(lds, too_large, eswoa_kernel, B, 64, stream, entry, sh, cand_ptr, len_init, cand, bounds, start_pos, pop,
                                max_iter, sd, best_fitness, best_pos, history, dr);
}

extern "C" int64_t gnnpn_eswoa_wide_workspace_bytes(int32_t P, int32_t T, int32_t pop) {
    return (int64_t)(P > 0 ? P : 0) * (int64_t)(pop > 0 ? pop : 0) * (int64_t)(T > 0 ? T : 0) * (int64_t)sizeof(int32_t);
}

extern "C" int gnnpn_eswoa_wide_f64(int32_t P, int32_t T, const int32_t* cand_ptr, const int32_t* len_init, const double* cand,
                                    const double* bounds, const int32_t* start_pos, int32_t pop, int32_t max_iter,
                                    const uint64_t* seeds, void* workspace, int64_t workspace_bytes, double* best_fitness,
                                    int32_t* best_pos, double* history, int64_t* draws, void* stream) {
    GNNPN_REQUIRE(cand_ptr && len_init && cand && bounds && start_pos && seeds && best_fitness && best_pos && history && draws,
                  "eswoa_wide: null operand");
    GNNPN_REQUIRE(P >= 0 && T >= 1 && pop > 0 && max_iter >= 0, "eswoa_wide: bad argument");
    if (P == 0) return GNNPN_OK;
    GNNPN_REQUIRE(workspace && workspace_bytes >= gnnpn_eswoa_wide_workspace_bytes(P, T, pop), "eswoa_wide: workspace too small");
    return eswoa_launch("eswoa_wide", "eswoa_wide_f64", true, P, Shape{nullptr, T, T, T, 0, 0, nullptr}, cand_ptr, len_init, cand,
                        bounds, start_pos, pop, max_iter, seeds, workspace, best_fitness, best_pos, history, draws, stream);
}

extern "C" int gnnpn_eswoa_f64(int32_t P, int32_t T, const int32_t* cand_ptr, const int32_t* len_init, const double* cand,
                               const double* bounds, const int32_t* start_pos, int32_t pop, int32_t max_iter,
                               const uint64_t* seeds, int32_t max_cand, double* best_fitness, int32_t* best_pos,
                               double* history, int64_t* draws, void* stream) {
    GNNPN_REQUIRE(cand_ptr && len_init && cand && bounds && start_pos && seeds && best_fitness && best_pos && history && draws,
                  "eswoa: null operand");
    GNNPN_REQUIRE(P >= 0 && pop > 0 && max_iter >= 0 && max_cand > 0, "eswoa: bad argument");
    if (T < 1 || T > 64) GNNPN_FAIL(GNNPN_E_UNSUP, "eswoa: T=%d categories (this form maps one category to one lane: 1..64; gnnpn_eswoa_wide_f64 takes any T)", T);
    if (P == 0) return GNNPN_OK;
    return eswoa_launch("eswoa", "eswoa_f64", false, P, Shape{nullptr, T, T, 64, max_cand, 0, nullptr}, cand_ptr, len_init, cand,
                        bounds, start_pos, pop, max_iter, seeds, nullptr, best_fitness, best_pos, history, draws, stream);
}

// ---- a ragged batch: problem p has prob_ptr[p+1] - prob_ptr[p] categories, all problems in ONE launch ----------------------
extern "C" int64_t gnnpn_eswoa_ragged_workspace_bytes(int32_t n_lists, int32_t max_slots, int32_t pop, int32_t wide) {
    if (!(wide || max_slots > 64)) return 0;
    return gnnpn_eswoa_wide_workspace_bytes(1, n_lists, pop);
}

extern "C" int gnnpn_eswoa_ragged_f64(int32_t B, const int32_t* prob_ptr, int32_t n_lists, int32_t max_slots, int32_t max_cand,
                                      const int32_t* cand_ptr, const int32_t* len_init, const double* cand, const double* bounds,
                                      const int32_t* start_pos, int32_t pop, int32_t max_iter, const uint64_t* seeds, int32_t wide,
                                      void* workspace, int64_t workspace_bytes, double* best_fitness, int32_t* best_pos,
                                      double* best_rows, double* history, int64_t* draws, void* stream) {
    GNNPN_REQUIRE(B >= 0 && n_lists >= 0 && pop > 0 && max_iter >= 0 && max_slots >= 1, "eswoa_ragged: bad argument");
    if (B == 0) return GNNPN_OK;
    GNNPN_REQUIRE(prob_ptr && cand_ptr && len_init && cand && bounds && start_pos && seeds && best_fitness && best_pos && history &&
                  draws, "eswoa_ragged: null operand");
    const bool use_wide = wide || max_slots > 64;
    if (use_wide)
        GNNPN_REQUIRE(workspace && workspace_bytes >= gnnpn_eswoa_ragged_workspace_bytes(n_lists, max_slots, pop, wide),
                      "eswoa_ragged: the workgroup form needs a workspace of gnnpn_eswoa_ragged_workspace_bytes");
    else
        GNNPN_REQUIRE(max_cand >= 1, "eswoa_ragged: max_cand must be >= 1 for the lane-per-category form");
    const Shape sh{prob_ptr, 0, max_slots, use_wide ? max_slots : 64, use_wide ? 0 : max_cand, n_lists, best_rows};
    return eswoa_launch("eswoa_ragged", use_wide ? "eswoa_ragged_f64 (workgroup form)" : "eswoa_ragged_f64", use_wide, B, sh, cand_ptr,
                        len_init, cand, bounds, start_pos, pop, max_iter, seeds, workspace, best_fitness, best_pos, history, draws,
                        stream);
}
