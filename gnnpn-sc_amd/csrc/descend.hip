// One-swap coordinate descent over the ES-WOA figure of merit: the deterministic stage between the greedy decode and ES-WOA.
//
// From a problem's start composition, sweep the slots in order; at slot j evaluate the composition with slot j replaced by EVERY
// candidate of list j, take the smallest merit (the lowest position among equals) and move there if it is strictly below the
// current merit; stop after a sweep without a move, or after max_sweeps.  Every merit is bit for bit the violate + objFunc of
// oracle/woa.py `objective` (woa_eval.h), so a run is a pure function of its inputs and equals the plain Python restatement of
// the search (tests/descent_reference.py) in every float64 and every position.
//
// figure_of_merit runs the two np.cumprod chains of ONE composition on 2 of 64 lanes.  The candidates of one slot differ in a
// single row, so here they run one candidate per lane: the chain prefix up to slot j, the smallest two entries of column 1 and the
// count of real services are carried wave-uniformly across j; a lane multiplies its own row onto the prefix and continues both
// chains through cur[j+1 .. T-1] (every lane reads the same LDS address: broadcasts), and forms np.sum of column 0 in numpy's
// order with element j replaced.  No atomics, no waits on other workgroups; every loop is bounded by max_sweeps, T or a list length.
//
// Pair-swap descent (descend_pairs_kernel, descend_pairs_wide_kernel) goes on from the one-swap optimum: a swap that breaks a product
// bound costs +1 and is never taken alone, even where a second swap restores the bound.  A pair sweep tries, for every two slots (or
// every two at most max_span apart), every pair of their candidates (one pair per thread, the same carried prefix, two rows replaced),
// and the one-swap sweeps run again after a sweep that moved — the same sweeps, not a second statement of them
// (tests/pair_descent_reference.py and, with the span, tests/pair_window_reference.py are its Python restatements).
//
// Over shortlists (descend_pairs_shortlist_kernel, descend_pairs_shortlist_wide_kernel): before every pair sweep each slot keeps the
// max_rank candidates whose single swap into the current composition has the lowest merit — the one-swap sweep's own evaluation
// (slot_path, one_swap_merit), ranked by counting in LDS — and the sweep tries only pairs of kept candidates
// (tests/pair_shortlist_reference.py).  The four builds without shortlists compile none of it.
//
// The tabu walk (descend_tabu_kernel, descend_tabu_wide_kernel) leaves the one-swap optimum on purpose: every step takes the best
// single swap of the whole composition — the shortlist pass's slot loop over slot_path / one_swap_merit, one (value, key) argmin per
// step — whether or not it lowers the merit, bars the position the slot left for `tenure` steps unless the swap beats the best merit
// seen, and remembers the best composition; the one-swap sweeps polish it where the walk was cut there (tests/tabu_reference.py).
// No draws: a pure function of the tables.  The six descent builds compile none of it.
//
// The tabu walk over pair moves (descend_tabu_pairs_kernel, descend_tabu_pairs_wide_kernel) is that walk whose step may also take a
// pair: the step's slot loop forms the shortlists of the current composition from the same single-swap merits that the singles'
// argmin reads, a pair pass over the shortlists follows — the evaluation of one (i, j, a, b) is the pair sweeps' (pair_path,
// pair_rest, pair_merit), stated once — and ONE argmin over (merit, single before pair, key) ends the step; a pair is tabu where
// either of its positions is, and both slots bar the positions they leave (tests/tabu_pairs_reference.py).  It crosses in one step
// the wall that costs the tabu walk two, and goes on where the pair sweeps stop.  The eight other builds compile none of the pass.
#include "woa_eval.h"

#include <climits>
#include <limits>
#include <type_traits>

namespace {
// What a slot's candidates share: the smallest (min1, at `owner`), second smallest (min2, at `owner2`) and third smallest (min3)
// entry of column 1 and the number of real services (column 0 > 0) of the current composition.  Thread-uniform: every thread scans
// the same LDS columns.  The one-swap sweeps use min1 / min2 / owner; the pair sweep takes two slots out and needs all five.
struct Carried {
    double min1, min2, min3;
    int owner, owner2, n_real;
    __device__ void scan(const double* col0, const double* col1, int T) {
        min1 = min2 = min3 = INFINITY;
        owner = owner2 = -1;
        n_real = 0;
        for (int i = 0; i < T; ++i) {
            const double v = col1[i];
            if (v < min1) {
                min3 = min2;
                min2 = min1;
                owner2 = owner;
                min1 = v;
                owner = i;
            } else if (v < min2) {
                min3 = min2;
                min2 = v;
                owner2 = i;
            } else if (v < min3) {
                min3 = v;
            }
            n_real += col0[i] > 0.0;
        }
    }
    __device__ __forceinline__ double min_with(int j, double q1) const { return fmin(owner == j ? min2 : min1, q1); }
    __device__ __forceinline__ int real_with(double old0, double q0) const { return n_real - (old0 > 0.0) + (q0 > 0.0); }
    // np.min of column 1 without slots i != j: the smallest entry neither of them owns (callers fmin their two new entries onto it)
    __device__ __forceinline__ double min_without(int i, int j) const {
        const double m1 = min1, m2 = min2, m3 = min3;                 // read first: the choice is among values, not addresses
        const bool out1 = owner == i || owner == j, out2 = owner2 == i || owner2 == j;
        return out1 ? (out2 ? m3 : m2) : m1;
    }
};

// (value, position) order: the smaller merit, the lower position among equals.  A NaN merit never enters (callers keep +inf for it).
template <class K>
__device__ __forceinline__ void take_better(double& f, K& c, double of, K oc) {
    if (of < f || (of == f && oc < c)) {
        f = of;
        c = oc;
    }
}
__device__ __forceinline__ void wave_argmin(double& f, int& c, int lane) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double of = wave_bcast(f, (lane + o) & 63);
        const int oc = __shfl(c, (lane + o) & 63);
        take_better(f, c, of, oc);
    }
}

// The same with a 64-bit position (the workgroup form's pair products: a * len_j + b over lists only int32 cand_ptr bounds).
__device__ __forceinline__ void wave_argmin(double& f, long long& c, int lane) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double of = wave_bcast(f, (lane + o) & 63);
        const long long oc = __double_as_longlong(wave_bcast(__longlong_as_double(c), (lane + o) & 63));      // a move of bits
        take_better(f, c, of, oc);
    }
}

constexpr int SIB_MAX = 32;        // levels of np.sum's recursion: a block halves (to within 7 terms) per level

// Where a problem's state lives: the columns of cur (L.col0, col1, L.col2, L.col3), the base / len tables and the bounds in LDS;
// cur, in LDS or the problem's best_pos row; the candidate table's LDS copy (lane form); red / cnt / sib (workgroup form).  The
// shortlist builds add mer / rk (one list's single-swap merits and their ranks) and list (every slot's shortlist), the tabu builds
// expire and best, the pair-move walk's builds all five, all in LDS.  A build fills what it uses (lane_carve, wide_carve) and reads
// nothing else.
struct DescendMem {
    WideLds L;
    double* col1;      // [T] column 1 (np.min)
    double* sib;       // [SIB_MAX] sums of the sibling blocks on np.sum's path to the current slot (pair sweep: three such rows)
    int* cur;          // [T]
    double* table;     // [n_cand][4]
    double* mer;       // [max_cand] shortlist builds: the single-swap merit of every candidate of the slot being ranked
    int* rk;           // [max_cand] ... and its rank in the (merit, position) order
    int* list;         // [T][rank] ... every slot's shortlist, positions ascending, -1 past its length
    int rank;          // row length of list: min(max_rank, max_cand)
    int* expire;       // [max_cand] tabu builds: candidate base[j] + c may not return to slot j at steps t <= expire (0: never left)
    int* best;         // [T] ... the best composition the walk has seen
};

// The five builds of each form, by what they search with: it decides the sibling rows and what comes on top of the search state.
enum class Build { one_swap, pairs, shortlist, tabu, tabu_pairs };
__host__ __device__ __forceinline__ bool has_shortlists(Build b) { return b == Build::shortlist || b == Build::tabu_pairs; }
__host__ __device__ __forceinline__ bool has_tabu_table(Build b) { return b == Build::tabu || b == Build::tabu_pairs; }

// The ints on top of a form's tables: rk [max_cand] and list [slots][rank] (shortlists), then expire [max_cand] and best [slots]
// (tabu table); the pair-move walk has both.
__host__ __device__ __forceinline__ int* carve_ints(DescendMem& M, int* at, Build build, int slots, int max_cand, int rank) {
    if (has_shortlists(build)) {
        M.rk = at;
        M.list = M.rk + max_cand;
        M.rank = rank;
        at = M.list + (size_t)slots * rank;
    }
    if (has_tabu_table(build)) {
        M.expire = at;
        M.best = M.expire + max_cand;
        at = M.best + slots;
    }
    return at;
}

// The LDS layout of a problem, stated once per form: the kernels carve `raw` with it, and the host asks for the bytes it returns
// on a null base with the launch's maxima (descend_lds_bytes), so the two cannot part.
// Lane form: the four columns of cur [4][64] (figure_of_merit's layout), bounds [4], base / len / cur [64] each, the candidate table
// [max_cand][4]; behind it mer [max_cand] f64, rk and list [max_slots][rank] (shortlist), or expire and best [64] (tabu), or all of
// them with best [max_slots] (the pair-move walk).
__host__ __device__ __forceinline__ size_t lane_carve(DescendMem& M, unsigned char* raw, Build build, int max_slots, int max_cand, int rank) {
    double* col = reinterpret_cast<double*>(raw);
    int* tab = reinterpret_cast<int*>(col + 260);
    M.L = WideLds{col, col + 128, col + 192, nullptr, nullptr, tab, tab + 64, col + 256};
    M.col1 = col + 64;
    M.sib = nullptr;
    M.cur = tab + 128;
    M.table = reinterpret_cast<double*>(tab + 192);
    double* top = M.table + (size_t)max_cand * 4;
    if (has_shortlists(build)) {
        M.mer = top;
        top += max_cand;
    }
    int* end = carve_ints(M, reinterpret_cast<int*>(top), build, build == Build::tabu ? 64 : max_slots, max_cand, rank);
    return reinterpret_cast<unsigned char*>(end) - raw;
}

// Workgroup form, T slots (the problem's own in a kernel, max_slots on the host): WideLds with column 1 [T], the sibling sums
// [1 | 3][SIB_MAX] (one row for the one-swap sweeps, three where there is a pair sweep) and, shortlist, mer [max_cand] among its
// doubles; behind its base / len tables rk and list [T][rank] (shortlist), or expire and best [T] (tabu), or all four (the pair-move
// walk, which also has the three sibling rows and mer).  cur is the problem's best_pos row, the table stays in global memory.
__host__ __device__ __forceinline__ size_t wide_carve(DescendMem& M, unsigned char* raw, Build build, int T, int max_cand, int rank, int32_t* cur) {
    const int sibs = (build == Build::pairs || has_shortlists(build) ? 3 : 1) * SIB_MAX;
    M.col1 = M.L.carve(raw, T, (size_t)T + sibs + (has_shortlists(build) ? max_cand : 0));
    M.sib = M.col1 + T;
    if (has_shortlists(build)) M.mer = M.sib + sibs;
    M.cur = cur;
    M.table = nullptr;
    int* end = carve_ints(M, M.L.len + T, build, T, max_cand, rank);
    return reinterpret_cast<unsigned char*>(end) - raw;
}

// A problem's search state between the three parts below, thread-uniform: its slot count, its candidate table (LDS or global), the
// current composition's merit and what its slots' candidates share.  The composition itself is M.cur and the columns in LDS.
struct DescendState {
    int T;
    const double* cand;
    double fit;
    Carried cr;
};

// The search in three parts, each by the NT threads of a problem's workgroup — load and validate, one-swap sweeps from the state in
// LDS, write the outputs — which descend_problem (both one-swap kernels) and descend_pairs_problem (both pair kernels) call.  TABLE_IN_LDS: the problem's
// candidate table is copied to M.table and cur is LDS too (else the table stays in global memory and cur IS the output row).
// NT = 64 is one wave whose columns are [4][64]: at most 64 slots, so np.sum is always one leaf and nothing crosses waves.

// Part 1: validates the problem's lists and start, fills the LDS tables, forms the start's merit (-> start_fitness) and `Carried`.
// False: the problem is not searched and nothing but L.base / L.len was touched; the caller writes what such a problem leaves.
template <int NT, bool TABLE_IN_LDS>
__device__ __forceinline__ bool descend_load(const DescendMem& M, const Shape& sh, const int32_t* __restrict__ cand_ptr,
                                             const double* __restrict__ cand_g, const double* __restrict__ bounds_g,
                                             const int32_t* __restrict__ start_pos, double* __restrict__ start_fitness, DescendState& S) {
    constexpr bool WAVES = NT > 64;
    const WideLds& L = M.L;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int T = sh.count(p);
    const size_t s0 = sh.first(p);
    const bool fits = sh.fits(p, T);
    const int c0 = fits ? cand_ptr[s0] : 0, n_cand = fits ? cand_ptr[s0 + T] - c0 : 0;
    const bool seeded = fits && start_pos[s0] >= 0;
    // not what the launch was sized for, a list outside the table, an empty list, a start outside its list: no search.  One test
    // after the loop, so that all these loads are in flight together.
    int bad = !fits || n_cand < 0 || !sh.fits_cand(n_cand);
    for (int j = tid; j < (fits ? T : 0); j += NT) {
        const int b = cand_ptr[s0 + j] - c0, ln = cand_ptr[s0 + j + 1] - cand_ptr[s0 + j], x = seeded ? start_pos[s0 + j] : 0;
        bad |= b < 0 || ln < 1 || b + ln > n_cand || x < 0 || x >= ln;
        L.base[j] = b;
        L.len[j] = ln;
    }
    if constexpr (WAVES) bad = __syncthreads_or(bad);
    else bad = __any(bad);
    if (bad) return false;
    const double* cand = cand_g + (size_t)c0 * 4;
    if constexpr (TABLE_IN_LDS) {
        for (int i = tid; i < n_cand * 4; i += NT) M.table[i] = cand[i];
        cand = M.table;
    }
    if (tid < 4) L.bounds[tid] = bounds_g[(size_t)p * 4 + tid];
    for (int j = tid; j < T; j += NT) {
        const int x = seeded ? start_pos[s0 + j] : 0;
        M.cur[j] = x;
        if constexpr (WAVES) M.col1[j] = cand[(size_t)(L.base[j] + x) * 4 + 1];
    }
    __syncthreads();
    double fit;                                                       // the start's merit; leaves the columns of cur in LDS
    if constexpr (WAVES) {
        fit = wide_merit(L, M.cur, cand, T, tid);
    } else {
        double q[4] = {0.0, 0.0, 0.0, 0.0};
        if (lane < T) gather_row(cand, L.base[lane], L.len[lane], M.cur[lane], q);
        fit = figure_of_merit(q, T, lane, L.col0, L.bounds);
    }
    if (tid == 0) start_fitness[p] = fit;
    S.T = T;
    S.cand = cand;
    S.fit = fit;
    S.cr.scan(L.col0, M.col1, T);
    return true;
}

// Part 2: up to max_sweeps one-swap sweeps from the state in LDS, thread = one candidate of the current slot; adds to `sweeps` and
// `moves`, `settled` = the last sweep moved nothing (unchanged where max_sweeps = 0); hist (or NULL) takes the merit after every sweep.
// Above 128 slots np.sum follows numpy's recursion: only the block of at most 128 terms that holds slot j changes with the
// candidate, so a thread sums that block with its own value in it and adds the sums of the untouched sibling blocks (`sib`, formed
// once per slot by pw_sum) on the way up, deepest first — the same additions as the recursion (a + b rounds as b + a).  The two
// pieces below (slot_path, one_swap_merit) are that evaluation; the shortlist pass (form_shortlists) calls them too.

// np.sum's leaf block of slot j and, in the workgroup form, the length of its path from the root: M.sib[0 .. depth - 1] get the
// sums of the untouched sibling blocks, root first (wave 0 forms them by pw_sum), and a barrier follows.  Workgroup-uniform.
struct SlotPath {
    int off, ln, depth;
};
template <int NT>
__device__ __forceinline__ SlotPath slot_path(const DescendMem& M, int T, int j) {
    int off = 0, ln = T, depth = 0;
    if constexpr (NT > 64) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        while (ln > 128 && depth < SIB_MAX) {
            int n2 = ln / 2;
            n2 -= n2 % 8;
            int so, sl;
            if (j < off + n2) {
                so = off + n2; sl = ln - n2; ln = n2;
            } else {
                so = off; sl = n2; off += n2; ln -= n2;
            }
            if (wave == 0) {
                const double v = pw_sum(M.L.col0 + so, sl, lane);
                if (lane == 0) M.sib[depth] = v;
            }
            ++depth;
        }
        __syncthreads();                                              // sib is written
    }
    return SlotPath{off, ln, depth};
}

// The merit of the current composition with slot j alone replaced by row r, by ONE thread: the one statement of the single-swap
// evaluation, for the one-swap sweeps and for the ranking behind the shortlists.  pre2 / pre3: np.cumprod up to slot j - 1; the
// thread continues both chains through cur[j+1 .. T-1] and forms np.sum with element j replaced (its leaf, then the siblings up).
template <int NT>
__device__ __forceinline__ double one_swap_merit(const DescendMem& M, const Carried& cr, const double* r, int T, int j, const SlotPath& sp,
                                                 double old0, double pre2, double pre3) {
    const WideLds& L = M.L;
    const double q0 = r[0], q1 = r[1];
    double p2 = j == 0 ? r[2] : __dmul_rn(pre2, r[2]), p3 = j == 0 ? r[3] : __dmul_rn(pre3, r[3]);
    for (int i = j + 1; i < T; ++i) {
        p2 = __dmul_rn(p2, L.col2[i]);
        p3 = __dmul_rn(p3, L.col3[i]);
    }
    double sum = pw_leaf_swapped(L.col0 + sp.off, sp.ln, j - sp.off, q0);
    if constexpr (NT > 64)
        for (int d = sp.depth - 1; d >= 0; --d) sum = __dadd_rn(sum, M.sib[d]);
    return merit_of(sum, cr.real_with(old0, q0), cr.min_with(j, q1), p2, p3, L.bounds);
}

template <int NT>
__device__ __forceinline__ void one_swap_sweeps(const DescendMem& M, DescendState& S, int32_t max_sweeps, double* __restrict__ hist,
                                                int& sweeps, int& moves, bool& settled) {
    constexpr bool WAVES = NT > 64;
    const WideLds& L = M.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = S.T;
    const double* cand = S.cand;
    double fit = S.fit;
    Carried cr = S.cr;
    for (int s = 0; s < max_sweeps; ++s) {
        bool improved = false;
        double pre2 = 1.0, pre3 = 1.0;                                // np.cumprod of columns 2 and 3 up to slot j - 1
        for (int j = 0; j < T; ++j) {
            const SlotPath sp = slot_path<NT>(M, T, j);               // (workgroup form: red / cnt of slot j - 1 are read behind it)
            const int bj = L.base[j], lj = L.len[j];
            const double old0 = L.col0[j];
            double bf = INFINITY;
            int bc = INT_MAX;
            for (int c = tid; c < lj; c += NT) {                      // lists longer than the workgroup: chunks, lowest position first
                const double f = one_swap_merit<NT>(M, cr, cand + (size_t)(bj + c) * 4, T, j, sp, old0, pre2, pre3);
                if (f < bf) {
                    bf = f;
                    bc = c;
                }
            }
            wave_argmin(bf, bc, lane);
            if constexpr (WAVES) {
                if (lane == 0) {
                    L.red[wave] = bf;
                    L.cnt[wave] = bc;
                }
                __syncthreads();
                bf = L.red[0];
                bc = L.cnt[0];
                for (int w = 1; w < NT / 64; ++w) take_better(bf, bc, L.red[w], L.cnt[w]);
            }
            if (bf < fit) {                                           // workgroup-uniform
                if (tid == 0) {
                    const double* r = cand + (size_t)(bj + bc) * 4;
                    M.cur[j] = bc;
                    L.col0[j] = r[0];
                    M.col1[j] = r[1];
                    L.col2[j] = r[2];
                    L.col3[j] = r[3];
                }
                fit = bf;
                ++moves;
                improved = true;
                __syncthreads();
                cr.scan(L.col0, M.col1, T);
            }
            pre2 = j == 0 ? L.col2[0] : __dmul_rn(pre2, L.col2[j]);
            pre3 = j == 0 ? L.col3[0] : __dmul_rn(pre3, L.col3[j]);
        }
        ++sweeps;
        settled = !improved;
        if (hist && tid == 0) hist[s] = fit;
        if (!improved) break;
    }
    S.fit = fit;
    S.cr = cr;
}

// Part 3: the composition in LDS and its merit to best_pos / best_rows / best_fitness.
template <int NT, bool TABLE_IN_LDS>
__device__ __forceinline__ void descend_store(const DescendMem& M, const Shape& sh, const DescendState& S,
                                              double* __restrict__ best_fitness, int32_t* __restrict__ best_pos_out) {
    const WideLds& L = M.L;
    const int p = blockIdx.x, tid = threadIdx.x, T = S.T;
    double* rows = sh.rows_out(p);
    for (int j = tid; j < T; j += NT) {
        if constexpr (TABLE_IN_LDS) best_pos_out[sh.out_row(p) + j] = M.cur[j];
        if (rows) {
            rows[(size_t)j * 4 + 0] = L.col0[j];
            rows[(size_t)j * 4 + 1] = M.col1[j];
            rows[(size_t)j * 4 + 2] = L.col2[j];
            rows[(size_t)j * 4 + 3] = L.col3[j];
        }
    }
    if (tid == 0) best_fitness[p] = S.fit;
}

// One-swap descent: the three parts, the history tail and the counters.
template <int NT, bool TABLE_IN_LDS>
__device__ __forceinline__ void descend_problem(const DescendMem& M, const Shape& sh, const int32_t* __restrict__ cand_ptr,
                                                const double* __restrict__ cand_g, const double* __restrict__ bounds_g,
                                                const int32_t* __restrict__ start_pos, int32_t max_sweeps,
                                                double* __restrict__ best_fitness, double* __restrict__ start_fitness,
                                                int32_t* __restrict__ best_pos_out, double* __restrict__ history,
                                                int32_t* __restrict__ sweeps_out, int32_t* __restrict__ moves_out) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const int hist_ld = max_sweeps > 1 ? max_sweeps : 1;           // history has at least one entry per problem
    DescendState S;
    if (!descend_load<NT, TABLE_IN_LDS>(M, sh, cand_ptr, cand_g, bounds_g, start_pos, start_fitness, S)) {
        not_searched(p, tid, NT, best_fitness, start_fitness, history, hist_ld, sweeps_out, moves_out);
        return;
    }
    int sweeps = 0, moves = 0;
    bool settled = false;
    double* hist = history + (size_t)p * hist_ld;
    one_swap_sweeps<NT>(M, S, max_sweeps, hist, sweeps, moves, settled);
    for (int s = sweeps + tid; s < hist_ld; s += NT) hist[s] = S.fit;                               // max_sweeps = 0: the start
    descend_store<NT, TABLE_IN_LDS>(M, sh, S, best_fitness, best_pos_out);
    if (tid == 0) {
        sweeps_out[p] = sweeps;
        moves_out[p] = moves;
    }
}

// (merit, position) order of the shortlists, is (f2, c2) before (f, c): plain < on the merits, the lower position among equals
// (-0.0 and 0.0 are equal), a NaN after every number and NaNs among themselves by position.
__device__ __forceinline__ bool ranks_before(double f2, int c2, double f, int c) {
    if (f2 < f) return true;
    if (f < f2) return false;
    const bool n2 = f2 != f2, n = f != f;
    return n2 == n ? c2 < c : n;
}

// A slot's shortlist from the merits of its list in M.mer[0 .. lj - 1] (written, and a barrier passed): every candidate's rank by counting
// the candidates before it (lj reads of M.mer, every thread the same address) into M.rk; a kept candidate's place = the kept ones at
// lower positions.  row[0 .. keep - 1] = the kept positions, ascending.  lj, keep and the barrier are workgroup-uniform.
template <int NT>
__device__ __forceinline__ void keep_lowest(const DescendMem& M, int* row, int lj, int keep) {
    const int tid = threadIdx.x;
    for (int c = tid; c < lj; c += NT) {
        const double f = M.mer[c];
        int r = 0;
        for (int c2 = 0; c2 < lj; ++c2) r += ranks_before(M.mer[c2], c2, f, c);
        M.rk[c] = r;
    }
    __syncthreads();
    for (int c = tid; c < lj; c += NT) {
        if (M.rk[c] >= keep) continue;
        int at = 0;
        for (int c2 = 0; c2 < c; ++c2) at += M.rk[c2] < keep;
        row[at] = c;
    }
}

// The shortlists of one pair sweep, from the state in LDS by the NT threads of the problem's workgroup: per slot j the min(rank,
// len_j) candidates whose single swap into the CURRENT composition has the lowest merit, positions ascending, into M.list[j][..]
// (-1 behind them).  Per slot: the merits of the list (one_swap_merit, thread = one candidate, chunks beyond the workgroup) into
// M.mer, then keep_lowest.  A list no longer than `rank` is kept whole and nothing is evaluated.
// Nothing moves here.  Bounded by T and list lengths; j, keep and every barrier are workgroup-uniform.
template <int NT>
__device__ __forceinline__ void form_shortlists(const DescendMem& M, const DescendState& S) {
    const WideLds& L = M.L;
    const int tid = threadIdx.x, T = S.T, rank = M.rank;
    const double* cand = S.cand;
    double pre2 = 1.0, pre3 = 1.0;                                    // np.cumprod of columns 2 and 3 up to slot j - 1
    for (int j = 0; j < T; ++j) {
        const int bj = L.base[j], lj = L.len[j];
        const int keep = lj < rank ? lj : rank;
        int* row = M.list + (size_t)j * rank;
        if (keep == lj) {
            for (int c = tid; c < lj; c += NT) row[c] = c;
        } else {
            const SlotPath sp = slot_path<NT>(M, T, j);
            const double old0 = L.col0[j];
            for (int c = tid; c < lj; c += NT) M.mer[c] = one_swap_merit<NT>(M, S.cr, cand + (size_t)(bj + c) * 4, T, j, sp, old0, pre2, pre3);
            __syncthreads();
            keep_lowest<NT>(M, row, lj, keep);
        }
        for (int k = keep + tid; k < rank; k += NT) row[k] = -1;
        __syncthreads();                                              // the row stands; mer / rk / sib are free for slot j + 1
        pre2 = j == 0 ? L.col2[0] : __dmul_rn(pre2, L.col2[j]);
        pre3 = j == 0 ? L.col3[0] : __dmul_rn(pre3, L.col3[j]);
    }
}

// A pair product's position k = a * len_j + b: an int where the table is in LDS (a CU's LDS holds under 5000 candidates), 64 bits in
// the workgroup form, whose lists only the int32 cand_ptr bounds (len_i + len_j < 2^31, so k < 2^62).
template <int NT>
using pair_key_t = std::conditional_t<(NT > 64), long long, int>;

// The evaluation of one pair (i, j, a, b), stated once for the pair sweeps and the pair-move walk: pair_path (what np.sum needs of the
// slot pair), pair_rest (what np.min and the count of real services keep of the other slots) and pair_merit (one thread's merit).

// np.sum's blocks of the slot pair i < j.  Lane form: one leaf, nothing to form.  Workgroup form, above 128 slots: the block that
// holds both slots (off, ln) and its n_up untouched siblings up to the root in M.sib[0 ..]; `two`: the paths part, each slot has
// its own leaf (off_i, ln_i / off_j, ln_j) and n_i / n_j siblings below the parting node in M.sib[SIB_MAX ..] / M.sib[2 SIB_MAX ..].
// The sibling sums are formed by pw_sum, the waves taking them in turn, and a barrier follows.  Workgroup-uniform.
struct PairPath {
    int off, ln, n_up, off_i, ln_i, n_i, off_j, ln_j, n_j;
    bool two;
};
template <int NT>
__device__ __forceinline__ PairPath pair_path(const DescendMem& M, int T, int i, int j) {
    PairPath pp{0, T, 0, 0, 0, 0, 0, 0, 0, false};
    if constexpr (NT > 64) {
        const WideLds& L = M.L;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        // One walk in three stretches (part 0: the common path from the root, 1: slot i's below the parting node, 2: slot
        // j's), so that pw_sum stands once; the waves take the siblings in turn.  Thread-uniform, no barrier inside.
        int part = 0, o = 0, l = T, d = 0, turn = 0, right_o = 0, right_l = 0;
        for (int step = 0; step < 3 * SIB_MAX + 4; ++step) {
            if (l <= 128 || d >= SIB_MAX) {                            // a leaf block ends the stretch
                if (part == 0) {
                    pp.off = o; pp.ln = l; pp.n_up = d;
                    break;
                }
                if (part == 2) {
                    pp.off_j = o; pp.ln_j = l; pp.n_j = d;
                    break;
                }
                pp.off_i = o; pp.ln_i = l; pp.n_i = d;
                part = 2; o = right_o; l = right_l; d = 0;
                continue;
            }
            int n2 = l / 2;
            n2 -= n2 % 8;
            if (part == 0 && i < o + n2 && j >= o + n2) {              // i left, j right: the paths part here
                pp.two = true;
                pp.n_up = d;
                right_o = o + n2; right_l = l - n2;
                part = 1; l = n2; d = 0;
                continue;
            }
            int so, sl;
            if ((part == 2 ? j : i) < o + n2) {                        // (common path: both slots are on slot i's side)
                so = o + n2; sl = l - n2; l = n2;
            } else {
                so = o; sl = n2; o += n2; l -= n2;
            }
            if (wave == (turn & (NT / 64 - 1))) {
                const double v = pw_sum(L.col0 + so, sl, lane);
                if (lane == 0) M.sib[part * SIB_MAX + d] = v;
            }
            ++turn;
            ++d;
        }
        __syncthreads();                                               // sib is written
    }
    return pp;
}

// np.min of column 1 and the number of real services without slots i and j.
struct PairRest {
    double min;
    int real;
};
__device__ __forceinline__ PairRest pair_rest(const DescendMem& M, const Carried& cr, int i, int j) {
    return PairRest{cr.min_without(i, j), cr.n_real - (M.L.col0[i] > 0.0) - (M.L.col0[j] > 0.0)};
}

// The merit of the current composition with slots i < j replaced by rows ra and rb, by ONE thread.  pre2 / pre3: np.cumprod up to
// slot i - 1; the thread continues both chains with row a, cur[i+1 .. j-1], row b, cur[j+1 .. T-1], one __dmul_rn each (numpy's
// order), and forms np.sum with the two elements replaced: in one leaf both at once; in two leaves each leaf with its own, the
// untouched siblings of each path up to the parting node, left + right; then the common path up to the root.
template <int NT>
__device__ __forceinline__ double pair_merit(const DescendMem& M, const PairRest& rest, const double* ra, const double* rb, int T, int i, int j,
                                             const PairPath& pp, double pre2, double pre3) {
    const WideLds& L = M.L;
    const double a0 = ra[0], a1 = ra[1], b0 = rb[0], b1 = rb[1];
    double p2 = i == 0 ? ra[2] : __dmul_rn(pre2, ra[2]), p3 = i == 0 ? ra[3] : __dmul_rn(pre3, ra[3]);
    for (int m = i + 1; m < j; ++m) {
        p2 = __dmul_rn(p2, L.col2[m]);
        p3 = __dmul_rn(p3, L.col3[m]);
    }
    p2 = __dmul_rn(p2, rb[2]);
    p3 = __dmul_rn(p3, rb[3]);
    for (int m = j + 1; m < T; ++m) {
        p2 = __dmul_rn(p2, L.col2[m]);
        p3 = __dmul_rn(p3, L.col3[m]);
    }
    double sum;
    if constexpr (NT > 64) {
        if (pp.two) {
            double left = pw_leaf_swapped(L.col0 + pp.off_i, pp.ln_i, i - pp.off_i, a0);
            for (int d = pp.n_i - 1; d >= 0; --d) left = __dadd_rn(left, M.sib[SIB_MAX + d]);
            double right = pw_leaf_swapped(L.col0 + pp.off_j, pp.ln_j, j - pp.off_j, b0);
            for (int d = pp.n_j - 1; d >= 0; --d) right = __dadd_rn(right, M.sib[2 * SIB_MAX + d]);
            sum = __dadd_rn(left, right);
        } else {
            sum = pw_leaf_swapped(L.col0 + pp.off, pp.ln, i - pp.off, a0, j - pp.off, b0);
        }
        for (int d = pp.n_up - 1; d >= 0; --d) sum = __dadd_rn(sum, M.sib[d]);
    } else {
        sum = pw_leaf_swapped(L.col0, T, i, a0, j, b0);
    }
    const int n_real = rest.real + (a0 > 0.0) + (b0 > 0.0);
    return merit_of(sum, n_real, fmin(fmin(rest.min, a1), b1), p2, p3, L.bounds);
}

// One pair sweep from the state in LDS by the NT threads of the problem's workgroup: for every slot pair i < j in order (max_span = s
// > 0: only j <= i + s), threads stride over k = a * len_j + b — the composition with slots i and j replaced by candidates a and b of
// their lists, current members included — lowest k first, each keeping its best under strict <; the argmin over the workgroup is by
// (value, k); the pair is taken if it is strictly below the current merit.  A thread evaluates its products by pair_merit with the
// carried prefix pre2 / pre3 (np.cumprod up to slot i - 1).  Returns the number of pairs taken.  Bounded by T and list lengths;
// (i, j) and every barrier are workgroup-uniform, the k loop has no barrier.
//
// np.sum above 128 slots (workgroup form only) replaces two elements of numpy's recursion tree (pair_path, pair_merit): where the
// slots lie in two leaves, the tree node where their paths part (the lowest common ancestor) has slot i in its left child and slot
// j in its right, and the additions are the recursion's own (a + b rounds as b + a).
//
// SHORT: the sweep runs over the shortlists M.list (form_shortlists, formed by the caller before the sweep and left as they are
// through it): a and b are the ia-th and ib-th kept position of their lists, k = ia * |S_j| + ib; everything else is the same code.
template <int NT, bool SHORT = false>
__device__ __forceinline__ int pair_sweep(const DescendMem& M, DescendState& S, int32_t max_span) {
    constexpr bool WAVES = NT > 64;
    using Key = pair_key_t<NT>;
    const WideLds& L = M.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = S.T;
    const double* cand = S.cand;
    int taken = 0;
    double pre2 = 1.0, pre3 = 1.0;
    for (int i = 0; i < T; ++i) {
        const int bi = L.base[i], li = SHORT && M.rank < L.len[i] ? M.rank : L.len[i];      // SHORT: |S_i|
        const int* si = SHORT ? M.list + (size_t)i * M.rank : nullptr;
        const int j_end = max_span > 0 && max_span < T - 1 - i ? i + max_span + 1 : T;
        for (int j = i + 1; j < j_end; ++j) {
            const PairPath pp = pair_path<NT>(M, T, i, j);             // (workgroup form: red of the pair before is read behind it)
            const int bj = L.base[j], lj = SHORT && M.rank < L.len[j] ? M.rank : L.len[j];
            const int* sj = SHORT ? M.list + (size_t)j * M.rank : nullptr;
            const Key n = (Key)li * lj;
            const PairRest rest = pair_rest(M, S.cr, i, j);
            double bf = INFINITY;
            Key bk = std::numeric_limits<Key>::max();
            for (Key k = tid; k < n; k += NT) {                        // products beyond the workgroup: chunks, lowest k first
                const int ia = (int)(k / lj), ib = (int)(k - (Key)ia * lj);
                const int a = SHORT ? si[ia] : ia, b = SHORT ? sj[ib] : ib;
                const double f = pair_merit<NT>(M, rest, cand + (size_t)(bi + a) * 4, cand + (size_t)(bj + b) * 4, T, i, j, pp, pre2, pre3);
                if (f < bf) {
                    bf = f;
                    bk = k;
                }
            }
            wave_argmin(bf, bk, lane);
            if constexpr (WAVES) {
                Key* red_k = reinterpret_cast<Key*>(L.red + 4);        // red[4 .. 7]: the waves' 64-bit positions (cnt holds ints)
                if (lane == 0) {
                    L.red[wave] = bf;
                    red_k[wave] = bk;
                }
                __syncthreads();
                bf = L.red[0];
                bk = red_k[0];
                for (int w = 1; w < NT / 64; ++w) take_better(bf, bk, L.red[w], red_k[w]);
            }
            if (bf < S.fit) {                                          // workgroup-uniform
                if (tid == 0) {
                    const int ia = (int)(bk / lj), ib = (int)(bk - (Key)ia * lj);
                    const int a = SHORT ? si[ia] : ia, b = SHORT ? sj[ib] : ib;
                    const double* ra = cand + (size_t)(bi + a) * 4;
                    const double* rb = cand + (size_t)(bj + b) * 4;
                    M.cur[i] = a;
                    M.cur[j] = b;
                    L.col0[i] = ra[0]; M.col1[i] = ra[1]; L.col2[i] = ra[2]; L.col3[i] = ra[3];
                    L.col0[j] = rb[0]; M.col1[j] = rb[1]; L.col2[j] = rb[2]; L.col3[j] = rb[3];
                }
                S.fit = bf;
                ++taken;
                __syncthreads();
                S.cr.scan(L.col0, M.col1, T);
            }
        }
        pre2 = i == 0 ? L.col2[0] : __dmul_rn(pre2, L.col2[i]);
        pre3 = i == 0 ? L.col3[0] : __dmul_rn(pre3, L.col3[i]);
    }
    return taken;
}

// Pair-swap descent of one problem, both forms: phase 0 = the one-swap sweeps; then up to max_rounds rounds of one pair sweep and,
// where it moved, the one-swap sweeps again.  A round whose pair sweep moved nothing is the last (it is counted).  round_history[r] =
// the merit after round r, past the last round the final value (max_rounds = 0: its one entry is phase 0's merit); converged = the
// last pair sweep moved nothing and the last one-swap phase ended with a sweep that moved nothing (with a span: no pair within it).
struct PairOut {
    double* best_fitness; double* start_fitness; int32_t* best_pos; double* round_history;
    int32_t* sweeps; int32_t* moves; int32_t* rounds; int32_t* pair_moves; int32_t* converged;
};

// SHORT (the shortlist builds): every pair sweep is preceded by form_shortlists and runs over what it formed; so.shortlist (or NULL)
// [B, stride, max_rank] takes the shortlists of the last pair sweep that ran: row s of a problem = M.list[s], -1 past its length,
// past the LDS row (max_rank > M.rank: no list is that long) and past T; all -1 where no pair sweep ran or nothing was searched.
struct ShortOut {
    int32_t* shortlist;
    int32_t max_rank;
};

template <int NT>
__device__ __forceinline__ void shortlist_store(const DescendMem& M, const Shape& sh, const ShortOut& so, int T, bool formed) {
    if (!so.shortlist) return;
    const size_t n = (size_t)sh.stride * so.max_rank;
    int32_t* out = so.shortlist + (size_t)blockIdx.x * n;
    for (size_t x = threadIdx.x; x < n; x += NT) {
        const int s = (int)(x / so.max_rank), k = (int)(x - (size_t)s * so.max_rank);
        out[x] = formed && s < T && k < M.rank ? M.list[(size_t)s * M.rank + k] : -1;
    }
}

template <int NT, bool TABLE_IN_LDS, bool SHORT = false>
__device__ __forceinline__ void descend_pairs_problem(const DescendMem& M, const Shape& sh, const int32_t* __restrict__ cand_ptr,
                                                      const double* __restrict__ cand_g, const double* __restrict__ bounds_g,
                                                      const int32_t* __restrict__ start_pos, int32_t max_sweeps, int32_t max_rounds,
                                                      int32_t max_span, const PairOut& o, const ShortOut& so = ShortOut{nullptr, 0}) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const int rh_ld = max_rounds > 1 ? max_rounds : 1;             // round_history has at least one entry per problem
    double* rh = o.round_history + (size_t)p * rh_ld;
    DescendState S;
    if (!descend_load<NT, TABLE_IN_LDS>(M, sh, cand_ptr, cand_g, bounds_g, start_pos, o.start_fitness, S)) {
        not_searched(p, tid, NT, o.best_fitness, o.start_fitness, o.round_history, rh_ld, o.sweeps, o.moves);
        if (tid == 0) {
            o.rounds[p] = -1;
            o.pair_moves[p] = 0;
            o.converged[p] = 0;
        }
        if constexpr (SHORT) shortlist_store<NT>(M, sh, so, 0, false);
        return;
    }
    int sweeps = 0, moves = 0, rounds = 0, pair_moves = 0;
    bool settled = false, still = false;                           // still: the last pair sweep moved nothing
    one_swap_sweeps<NT>(M, S, max_sweeps, nullptr, sweeps, moves, settled);
    while (rounds < max_rounds) {
        if constexpr (SHORT) form_shortlists<NT>(M, S);
        const int taken = pair_sweep<NT, SHORT>(M, S, max_span);
        pair_moves += taken;
        still = taken == 0;
        if (!still) {
            settled = false;                                       // max_sweeps = 0: no sweep follows the move
            one_swap_sweeps<NT>(M, S, max_sweeps, nullptr, sweeps, moves, settled);
        }
        if (tid == 0) rh[rounds] = S.fit;
        ++rounds;
        if (still) break;
    }
    for (int r = rounds + tid; r < rh_ld; r += NT) rh[r] = S.fit;
    descend_store<NT, TABLE_IN_LDS>(M, sh, S, o.best_fitness, o.best_pos);
    if constexpr (SHORT) shortlist_store<NT>(M, sh, so, S.T, rounds > 0);
    if (tid == 0) {
        o.sweeps[p] = sweeps;
        o.moves[p] = moves;
        o.rounds[p] = rounds;
        o.pair_moves[p] = pair_moves;
        o.converged[p] = still && settled;
    }
}

// ---- tabu walk: leave the one-swap optimum by the best single swap — or (pair-move walk) single or pair swap — improving or not --------------
struct TabuOut {
    double* best_fitness; double* start_fitness; int32_t* best_pos; double* history; int32_t* sweeps; int32_t* moves;
    double* walk; int32_t* steps; int32_t* best_step; int32_t* stalled;
    int32_t* pair_steps;       // the pair-move walk only
};

// A step's key.  The tabu walk: base[j] + c of the single swap, an int; INT_MAX: no admissible move.  The pair-move walk: 64 bits —
// a single's base[j] + c as it is, a pair (i, j, ia, ib) as PAIR_MOVE | (i * T + j) << 32 | ia * |S_j| + ib, so every single comes
// before every pair and the pairs in the order of (i, j, a, b): the shortlists are ascending.  The fields cannot overflow: a form's
// LDS holds T doubles per column and max_cand merits, so i * T + j < 2^30 and ia * |S_j| + ib <= max_cand^2 < 2^31.
template <bool PAIRS>
using tabu_key_t = std::conditional_t<PAIRS, long long, int>;
constexpr long long PAIR_MOVE = 1ll << 62;

// One step's evaluation, form_shortlists' slot loop: for every slot j in order, thread = one candidate c != cur[j] of its list (chunks
// beyond the workgroup, lowest position first), the single-swap merit f by slot_path / one_swap_merit with pre2 / pre3 carried across
// the slots and S.cr constant.  (j, c) is admissible where expire[base[j] + c] < t, or f < best_f (aspiration).  A thread keeps its
// best admissible (f, key) under strict < — its keys only grow, so the lowest stays among equals, and a NaN never enters — and ONE
// (value, key) argmin over the workgroup ends the step.  key = the type's maximum: no admissible move.  Nothing moves here.
// Bounded by T, list lengths and the rank; j, (i, j) of the workgroup form and every barrier are workgroup-uniform.
//
// PAIRS (the pair-move walk): the same slot loop also forms the shortlists of the current composition — a list longer than the rank
// leaves its merits, cur[j]'s among them, in M.mer for keep_lowest — and the pair pass follows: every i < j (max_span = s > 0: only
// j <= i + s), every (ia, ib) of S_i x S_j with a != cur[i] and b != cur[j], f by pair_merit; the pair is admissible where neither
// position is tabu, or f < best_f.  Lane form: np.sum is one leaf and nothing is shared per slot pair, so the lanes stride over ALL
// (i, j, ia, ib) of the step — a lane walks the slot pairs with its offset k into the current one and carries its own prefix —
// and a pair's few products do not leave most lanes idle.  Workgroup form: the sibling sums are per (i, j) (pair_path), the threads
// stride over a pair's products and a barrier frees the sums for the next pair.
template <int NT, bool PAIRS>
__device__ __forceinline__ void tabu_step(const DescendMem& M, const DescendState& S, const int* expire, int t, double best_f, int32_t max_span,
                                          double& f_out, tabu_key_t<PAIRS>& key_out) {
    using Key = tabu_key_t<PAIRS>;
    const WideLds& L = M.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = S.T;
    const double* cand = S.cand;
    double pre2 = 1.0, pre3 = 1.0;                                    // np.cumprod of columns 2 and 3 up to slot j - 1
    double bf = INFINITY;
    Key bk = std::numeric_limits<Key>::max();
    for (int j = 0; j < T; ++j) {
        const SlotPath sp = slot_path<NT>(M, T, j);
        const int bj = L.base[j], lj = L.len[j], cj = M.cur[j];
        const double old0 = L.col0[j];
        const bool ranked = PAIRS && M.rank < lj;                     // the list is longer than its shortlist: every merit is wanted
        for (int c = tid; c < lj; c += NT) {
            if (c == cj && !ranked) continue;
            const double f = one_swap_merit<NT>(M, S.cr, cand + (size_t)(bj + c) * 4, T, j, sp, old0, pre2, pre3);
            if constexpr (PAIRS)
                if (ranked) M.mer[c] = f;
            if (c != cj && (expire[bj + c] < t || f < best_f) && f < bf) {
                bf = f;
                bk = bj + c;
            }
        }
        if constexpr (PAIRS) {
            int* row = M.list + (size_t)j * M.rank;
            const int keep = ranked ? M.rank : lj;
            if (ranked) {
                __syncthreads();
                keep_lowest<NT>(M, row, lj, keep);
            } else {
                for (int c = tid; c < lj; c += NT) row[c] = c;
            }
            for (int k = keep + tid; k < M.rank; k += NT) row[k] = -1;
            __syncthreads();                                          // the row stands; mer / rk / sib are free for slot j + 1
        } else if constexpr (NT > 64) {
            if (sp.depth > 0) __syncthreads();                        // sib is free for slot j + 1
        }
        pre2 = j == 0 ? L.col2[0] : __dmul_rn(pre2, L.col2[j]);
        pre3 = j == 0 ? L.col3[0] : __dmul_rn(pre3, L.col3[j]);
    }
    if constexpr (PAIRS) {
        const int rank = M.rank;
        // product k of the slot pair (i, j), |S_j| = lj: evaluated unless it leaves a slot where it is, kept if admissible and better
        auto try_pair = [&](int i, int j, int lj, long long k, const PairPath& pp, const PairRest& rest, double p2, double p3) {
            const int ia = (int)(k / lj), ib = (int)(k - (long long)ia * lj);
            const int a = M.list[(size_t)i * rank + ia], b = M.list[(size_t)j * rank + ib];
            if (a == M.cur[i] || b == M.cur[j]) return;
            const int ka = L.base[i] + a, kb = L.base[j] + b;
            const double f = pair_merit<NT>(M, rest, cand + (size_t)ka * 4, cand + (size_t)kb * 4, T, i, j, pp, p2, p3);
            if (((expire[ka] < t && expire[kb] < t) || f < best_f) && f < bf) {
                bf = f;
                bk = PAIR_MOVE | (long long)(i * T + j) << 32 | k;
            }
        };
        auto kept = [&](int s) { return rank < L.len[s] ? rank : L.len[s]; };      // |S_s|
        pre2 = pre3 = 1.0;                                            // np.cumprod up to slot i - 1
        if constexpr (NT > 64) {
            for (int i = 0; i < T; ++i) {
                const int li = kept(i);
                const int j_end = max_span > 0 && max_span < T - 1 - i ? i + max_span + 1 : T;
                for (int j = i + 1; j < j_end; ++j) {
                    const PairPath pp = pair_path<NT>(M, T, i, j);
                    const PairRest rest = pair_rest(M, S.cr, i, j);
                    const int lj = kept(j);
                    const long long n = (long long)li * lj;
                    for (long long k = tid; k < n; k += NT) try_pair(i, j, lj, k, pp, rest, pre2, pre3);
                    __syncthreads();                                  // sib is free for the next pair
                }
                pre2 = i == 0 ? L.col2[0] : __dmul_rn(pre2, L.col2[i]);
                pre3 = i == 0 ? L.col3[0] : __dmul_rn(pre3, L.col3[i]);
            }
        } else {
            // Every turn either passes a slot pair whose products lie before this lane's next one or evaluates one product: bounded by
            // the number of slot pairs plus the lane's share of the products.  No barrier and no shuffle inside: the lanes part here.
            const PairPath pp = pair_path<NT>(M, T, 0, 1);            // one leaf: the same for every pair
            int i = 0, j = 1;
            long long k = tid;                                        // this lane's next product, counted from the first one of (i, j)
            while (i < T - 1) {
                const int lj = kept(j);
                const long long n = (long long)kept(i) * lj;
                if (k < n) {
                    try_pair(i, j, lj, k, pp, pair_rest(M, S.cr, i, j), pre2, pre3);
                    k += NT;
                    continue;
                }
                k -= n;
                if (++j < (max_span > 0 && max_span < T - 1 - i ? i + max_span + 1 : T)) continue;
                pre2 = i == 0 ? L.col2[0] : __dmul_rn(pre2, L.col2[i]);
                pre3 = i == 0 ? L.col3[0] : __dmul_rn(pre3, L.col3[i]);
                ++i;
                j = i + 1;
            }
        }
    }
    wave_argmin(bf, bk, lane);
    if constexpr (NT > 64) {
        Key* red_k = PAIRS ? reinterpret_cast<Key*>(L.red + 4) : reinterpret_cast<Key*>(L.cnt);      // 64-bit keys: red[4 .. 7], as pair_sweep
        if (lane == 0) {
            L.red[wave] = bf;
            red_k[wave] = bk;
        }
        __syncthreads();
        bf = L.red[0];
        bk = red_k[0];
        for (int w = 1; w < NT / 64; ++w) take_better(bf, bk, L.red[w], red_k[w]);
    }
    f_out = bf;
    key_out = bk;
}

// The tabu walk of one problem, both forms (tests/tabu_reference.py is its Python restatement).  Phase 0 = the one-swap sweeps.  Step
// t = 1 .. max_steps: tabu_step's move is taken whether or not it is below the current merit, and the position the slot leaves is
// tabu through step t + tenure; no admissible move ends the walk (stalled, the step is not counted).  best / best_f / best_step
// follow the walk under strict <.  Then best goes back into cur and the columns, and where the walk was cut at its best (the last
// step taken is best_step, and it did not stall) the one-swap sweeps run once more from there: best need not be a one-swap optimum.
// history[t - 1] = the best merit after step t (past the last step the last such value, before the polish; max_steps = 0: phase
// 0's merit), walk[t - 1] = the current merit after step t, NaN past the last step.
//
// PAIRS: the pair-move walk (tests/tabu_pairs_reference.py) — the same walk whose step may take a pair of the slots' shortlists
// (tabu_step); both slots of a pair bar the positions they leave, and pair_steps counts the steps that took one.
template <int NT, bool TABLE_IN_LDS, bool PAIRS = false>
__device__ __forceinline__ void descend_tabu_problem(const DescendMem& M, const Shape& sh, const int32_t* __restrict__ cand_ptr,
                                                     const double* __restrict__ cand_g, const double* __restrict__ bounds_g,
                                                     const int32_t* __restrict__ start_pos, int32_t max_sweeps, int32_t max_steps,
                                                     int32_t tenure, const TabuOut& o, int32_t max_span = 0) {
    const WideLds& L = M.L;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int ld = max_steps > 1 ? max_steps : 1;                  // history and walk have at least one entry per problem
    double* hist = o.history + (size_t)p * ld;
    double* walk = o.walk + (size_t)p * ld;
    DescendState S;
    if (!descend_load<NT, TABLE_IN_LDS>(M, sh, cand_ptr, cand_g, bounds_g, start_pos, o.start_fitness, S)) {
        not_searched(p, tid, NT, o.best_fitness, o.start_fitness, o.history, ld, o.sweeps, o.moves);
        for (int s = tid; s < ld; s += NT) walk[s] = NAN;
        if (tid == 0) {
            o.steps[p] = -1;
            o.best_step[p] = 0;
            o.stalled[p] = 0;
            if constexpr (PAIRS) o.pair_steps[p] = 0;
        }
        return;
    }
    const int T = S.T;
    const double* cand = S.cand;
    const int n_cand = L.base[T - 1] + L.len[T - 1];               // the lists are contiguous (descend_load checked them)
    for (int i = tid; i < n_cand; i += NT) M.expire[i] = 0;
    __syncthreads();
    int sweeps = 0, moves = 0, steps = 0, best_step = 0, stalled = 0, pair_steps = 0;
    bool settled = false;
    one_swap_sweeps<NT>(M, S, max_sweeps, nullptr, sweeps, moves, settled);
    double best_f = S.fit;
    for (int j = tid; j < T; j += NT) M.best[j] = M.cur[j];
    for (int t = 1; t <= max_steps; ++t) {
        double f;
        tabu_key_t<PAIRS> key;
        tabu_step<NT, PAIRS>(M, S, M.expire, t, best_f, max_span, f, key);
        if (key == std::numeric_limits<tabu_key_t<PAIRS>>::max()) {   // workgroup-uniform
            stalled = 1;
            break;
        }
        auto move = [&](int j, int c) {                                // slot j goes to position c and bars the one it leaves
            const double* r = cand + (size_t)(L.base[j] + c) * 4;
            M.expire[L.base[j] + M.cur[j]] = tenure > INT_MAX - t ? INT_MAX : t + tenure;
            M.cur[j] = c;
            L.col0[j] = r[0];
            M.col1[j] = r[1];
            L.col2[j] = r[2];
            L.col3[j] = r[3];
        };
        bool pair = false;
        if constexpr (PAIRS) pair = key >= PAIR_MOVE;
        if (pair) {                                                   // workgroup-uniform; the shortlists stand as the step formed them
            if constexpr (PAIRS) {
                if (tid == 0) {
                    const int ij = (int)((key ^ PAIR_MOVE) >> 32), i = ij / T, j = ij - i * T, k = (int)(key & 0x7fffffff);
                    const int lj = M.rank < L.len[j] ? M.rank : L.len[j], ia = k / lj, ib = k - ia * lj;
                    move(i, M.list[(size_t)i * M.rank + ia]);
                    move(j, M.list[(size_t)j * M.rank + ib]);
                }
                ++pair_steps;
            }
        } else {
            for (int j = tid; j < T; j += NT) {                        // the one thread whose slot owns the key moves
                const int c = (int)key - L.base[j];
                if (c >= 0 && c < L.len[j]) move(j, c);
            }
        }
        S.fit = f;
        steps = t;
        __syncthreads();
        S.cr.scan(L.col0, M.col1, T);
        if (f < best_f) {
            best_f = f;
            best_step = t;
            for (int j = tid; j < T; j += NT) M.best[j] = M.cur[j];
        }
        if (tid == 0) {
            hist[t - 1] = best_f;
            walk[t - 1] = f;
        }
    }
    for (int s = steps + tid; s < ld; s += NT) {
        hist[s] = best_f;
        walk[s] = NAN;
    }
    __syncthreads();                                                  // best stands
    if (best_step < steps) {                                          // the walk went on past its best: back to it
        for (int j = tid; j < T; j += NT) {
            const int c = M.best[j];
            const double* r = cand + (size_t)(L.base[j] + c) * 4;
            M.cur[j] = c;
            L.col0[j] = r[0];
            M.col1[j] = r[1];
            L.col2[j] = r[2];
            L.col3[j] = r[3];
        }
        S.fit = best_f;
        __syncthreads();
        S.cr.scan(L.col0, M.col1, T);
    } else if (steps > 0 && !stalled) {                               // cut at its best: the polish
        one_swap_sweeps<NT>(M, S, max_sweeps, nullptr, sweeps, moves, settled);
    }
    descend_store<NT, TABLE_IN_LDS>(M, sh, S, o.best_fitness, o.best_pos);
    if (tid == 0) {
        o.sweeps[p] = sweeps;
        o.moves[p] = moves;
        o.steps[p] = steps;
        o.best_step[p] = best_step;
        o.stalled[p] = stalled;
        if constexpr (PAIRS) o.pair_steps[p] = pair_steps;
    }
}
}  // namespace

// ---- lane form: one wavefront per problem (<= 64 slots), LDS as lane_carve lays it out --------------------------------------------------
__device__ __forceinline__ DescendMem lane_mem(unsigned char* lds_raw, Build build, const Shape& sh, int rank = 0) {
    DescendMem M;
    lane_carve(M, lds_raw, build, sh.stride, sh.max_cand, rank);
    return M;
}

__global__ __launch_bounds__(64) void descend_kernel(Shape sh, const int32_t* __restrict__ cand_ptr, const double* __restrict__ cand_g,
                                                     const double* __restrict__ bounds_g, const int32_t* __restrict__ start_pos,
                                                     int32_t max_sweeps, double* __restrict__ best_fitness,
                                                     double* __restrict__ start_fitness, int32_t* __restrict__ best_pos_out,
                                                     double* __restrict__ history, int32_t* __restrict__ sweeps_out,
                                                     int32_t* __restrict__ moves_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    descend_problem<64, true>(lane_mem(lds_raw, Build::one_swap, sh), sh, cand_ptr, cand_g, bounds_g, start_pos, max_sweeps, best_fitness,
                              start_fitness, best_pos_out, history, sweeps_out, moves_out);
}

// ---- pair-swap descent, lane form: one wavefront per problem (<= 64 slots) ---------------------------------------------------------------
// No atomics, no waits on other workgroups; loops bounded by max_rounds, max_sweeps, T, list lengths.
__global__ __launch_bounds__(64) void descend_pairs_kernel(Shape sh, const int32_t* __restrict__ cand_ptr, const double* __restrict__ cand_g,
                                                           const double* __restrict__ bounds_g, const int32_t* __restrict__ start_pos,
                                                           int32_t max_sweeps, int32_t max_rounds, int32_t max_span, PairOut o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    descend_pairs_problem<64, true>(lane_mem(lds_raw, Build::pairs, sh), sh, cand_ptr, cand_g, bounds_g, start_pos, max_sweeps, max_rounds,
                                    max_span, o);
}

// ---- pair-swap descent over shortlists, lane form: descend_pairs_kernel with the shortlist pass before every pair sweep -------------------
// No atomics, no waits on other workgroups; loops bounded by max_rounds, max_sweeps, T, list lengths, max_rank.
__global__ __launch_bounds__(64) void descend_pairs_shortlist_kernel(Shape sh, const int32_t* __restrict__ cand_ptr,
                                                                     const double* __restrict__ cand_g, const double* __restrict__ bounds_g,
                                                                     const int32_t* __restrict__ start_pos, int32_t max_sweeps,
                                                                     int32_t max_rounds, int32_t max_span, int32_t rank, PairOut o, ShortOut so) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    descend_pairs_problem<64, true, true>(lane_mem(lds_raw, Build::shortlist, sh, rank), sh, cand_ptr, cand_g, bounds_g, start_pos, max_sweeps,
                                          max_rounds, max_span, o, so);
}

// ---- workgroup form: any slot count, 256 threads per problem, LDS as wide_carve lays it out for the problem's own slot count --------------
__device__ __forceinline__ DescendMem wide_mem(unsigned char* lds_raw, Build build, const Shape& sh, int32_t* best_pos, int rank = 0) {
    DescendMem M;
    wide_carve(M, lds_raw, build, sh.count(blockIdx.x), sh.max_cand, rank, best_pos + sh.out_row(blockIdx.x));
    return M;
}

__global__ __launch_bounds__(WNT) void descend_wide_kernel(Shape sh, const int32_t* __restrict__ cand_ptr,
                                                           const double* __restrict__ cand_g, const double* __restrict__ bounds_g,
                                                           const int32_t* __restrict__ start_pos, int32_t max_sweeps,
                                                           double* __restrict__ best_fitness, double* __restrict__ start_fitness,
                                                           int32_t* __restrict__ best_pos_out, double* __restrict__ history,
                                                           int32_t* __restrict__ sweeps_out, int32_t* __restrict__ moves_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const DescendMem M = wide_mem(lds_raw, Build::one_swap, sh, best_pos_out);
    descend_problem<WNT, false>(M, sh, cand_ptr, cand_g, bounds_g, start_pos, max_sweeps, best_fitness, start_fitness, best_pos_out,
                                history, sweeps_out, moves_out);
}

// Pair-swap descent, workgroup form: the same rounds over the same state, the pair products spread over the 256 threads.
__global__ __launch_bounds__(WNT) void descend_pairs_wide_kernel(Shape sh, const int32_t* __restrict__ cand_ptr,
                                                                 const double* __restrict__ cand_g, const double* __restrict__ bounds_g,
                                                                 const int32_t* __restrict__ start_pos, int32_t max_sweeps,
                                                                 int32_t max_rounds, int32_t max_span, PairOut o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const DescendMem M = wide_mem(lds_raw, Build::pairs, sh, o.best_pos);
    descend_pairs_problem<WNT, false>(M, sh, cand_ptr, cand_g, bounds_g, start_pos, max_sweeps, max_rounds, max_span, o);
}

// Pair-swap descent over shortlists, workgroup form.
__global__ __launch_bounds__(WNT) void descend_pairs_shortlist_wide_kernel(Shape sh, const int32_t* __restrict__ cand_ptr,
                                                                           const double* __restrict__ cand_g,
                                                                           const double* __restrict__ bounds_g,
                                                                           const int32_t* __restrict__ start_pos, int32_t max_sweeps,
                                                                           int32_t max_rounds, int32_t max_span, int32_t rank, PairOut o,
                                                                           ShortOut so) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const DescendMem M = wide_mem(lds_raw, Build::shortlist, sh, o.best_pos, rank);
    descend_pairs_problem<WNT, false, true>(M, sh, cand_ptr, cand_g, bounds_g, start_pos, max_sweeps, max_rounds, max_span, o, so);
}

// ---- tabu walk, lane form ----------------------------------------------------------------------------------------------------------------
// No atomics, no waits on other workgroups; loops bounded by max_steps, max_sweeps, T, list lengths.
__global__ __launch_bounds__(64) void descend_tabu_kernel(Shape sh, const int32_t* __restrict__ cand_ptr, const double* __restrict__ cand_g,
                                                          const double* __restrict__ bounds_g, const int32_t* __restrict__ start_pos,
                                                          int32_t max_sweeps, int32_t max_steps, int32_t tenure, TabuOut o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    descend_tabu_problem<64, true>(lane_mem(lds_raw, Build::tabu, sh), sh, cand_ptr, cand_g, bounds_g, start_pos, max_sweeps, max_steps, tenure, o);
}

// Tabu walk, workgroup form.
__global__ __launch_bounds__(WNT) void descend_tabu_wide_kernel(Shape sh, const int32_t* __restrict__ cand_ptr,
                                                                const double* __restrict__ cand_g, const double* __restrict__ bounds_g,
                                                                const int32_t* __restrict__ start_pos, int32_t max_sweeps,
                                                                int32_t max_steps, int32_t tenure, TabuOut o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const DescendMem M = wide_mem(lds_raw, Build::tabu, sh, o.best_pos);
    descend_tabu_problem<WNT, false>(M, sh, cand_ptr, cand_g, bounds_g, start_pos, max_sweeps, max_steps, tenure, o);
}

// ---- pair-move tabu walk, lane form: one wavefront per problem (<= 64 slots) -----------------------------------------------------------------
// No atomics, no waits on other workgroups; loops bounded by max_steps, max_sweeps, T, list lengths, the rank.
__global__ __launch_bounds__(64) void descend_tabu_pairs_kernel(Shape sh, const int32_t* __restrict__ cand_ptr, const double* __restrict__ cand_g,
                                                                const double* __restrict__ bounds_g, const int32_t* __restrict__ start_pos,
                                                                int32_t max_sweeps, int32_t max_steps, int32_t tenure, int32_t max_span,
                                                                int32_t rank, TabuOut o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    descend_tabu_problem<64, true, true>(lane_mem(lds_raw, Build::tabu_pairs, sh, rank), sh, cand_ptr, cand_g, bounds_g, start_pos, max_sweeps,
                                         max_steps, tenure, o, max_span);
}

// Pair-move tabu walk, workgroup form.
__global__ __launch_bounds__(WNT) void descend_tabu_pairs_wide_kernel(Shape sh, const int32_t* __restrict__ cand_ptr,
                                                                      const double* __restrict__ cand_g, const double* __restrict__ bounds_g,
                                                                      const int32_t* __restrict__ start_pos, int32_t max_sweeps,
                                                                      int32_t max_steps, int32_t tenure, int32_t max_span, int32_t rank,
                                                                      TabuOut o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const DescendMem M = wide_mem(lds_raw, Build::tabu_pairs, sh, o.best_pos, rank);
    descend_tabu_problem<WNT, false, true>(M, sh, cand_ptr, cand_g, bounds_g, start_pos, max_sweeps, max_steps, tenure, o, max_span);
}

// LDS bytes one problem needs (host side): what the form's carve-up takes from a null base with the launch's maxima.
static size_t descend_lds_bytes(bool use_wide, Build build, int max_slots, int max_cand, int rank) {
    DescendMem M;
    return use_wide ? wide_carve(M, nullptr, build, max_slots, max_cand, rank, nullptr) : lane_carve(M, nullptr, build, max_slots, max_cand, rank);
}

// The operands every descent entry has, under their names in include/gnnpn_hip.h (wide: 0 where the entry has none).
struct DescendArgs {
    int32_t B; const int32_t* prob_ptr; int32_t n_lists, max_slots, max_cand; const int32_t* cand_ptr; const double* cand;
    const double* bounds; const int32_t* start_pos; int32_t max_sweeps, wide; double* best_rows; void* stream;
};

// The six descent entries: their argument checks (`who` names the entry in every message; options_ok / operands_given: the entry's
// own options are >= 0, its own outputs not NULL) and the one launch of `build` — `lane` or `wide`, whose parameters behind
// max_sweeps are `rest`.  Lane form: the table in LDS, so max_cand >= 1 and within a CU; workgroup form: the columns of max_slots
// slots within a CU.  The shortlist, tabu and pair-move builds size buffers of their own by max_cand (and `rank`, the shortlists' row) in
// both forms.
template <typename... P, typename... A>
static int descend_entry(const char* who, Build build, bool lane_only, const DescendArgs& a, int rank, bool options_ok, bool operands_given,
                         void (*lane)(P...), void (*wide)(P...), const A&... rest) {
    GNNPN_REQUIRE(a.B >= 0 && a.n_lists >= 0 && a.max_sweeps >= 0 && options_ok && a.max_slots >= 1, "%s: bad argument", who);
    if (a.B == 0) return GNNPN_OK;
    GNNPN_REQUIRE(a.prob_ptr && a.cand_ptr && a.cand && a.bounds && a.start_pos && operands_given, "%s: null operand", who);
    if (lane_only && a.max_slots > 64)
        GNNPN_FAIL(GNNPN_E_UNSUP, "%s: %d slots: the pair sweep has the lane form only (at most 64 slots per problem); "
                   "gnnpn_descend_ragged_f64 descends larger problems by single swaps", who, a.max_slots);
    const bool use_wide = a.wide || a.max_slots > 64, own = has_shortlists(build) || has_tabu_table(build);
    const int max_slots = a.max_slots, max_cand = a.max_cand;
    if (max_cand < 1 && (own || !use_wide)) {
        if (build == Build::one_swap) GNNPN_FAIL(GNNPN_E_ARG, "%s: max_cand must be >= 1 for the lane form", who);
        GNNPN_FAIL(GNNPN_E_UNSUP, "%s: max_cand must be >= 1 (it sizes %s in LDS)", who,
                   build == Build::pairs       ? "the table"
                   : build == Build::shortlist ? "the merit buffer, and in the lane form the table,"
                   : build == Build::tabu      ? "the tabu table, and in the lane form the candidate table,"
                                               : "the tabu table and the merit buffer, and in the lane form the candidate table,");
    }
    const size_t lds = descend_lds_bytes(use_wide, build, max_slots, max_cand, rank);
    auto too_large = [&]() -> int {
        const char* hint = use_wide || build == Build::pairs ? "" : "; wide=1 keeps the candidate table in global memory";
        if (has_shortlists(build))
            GNNPN_FAIL(GNNPN_E_UNSUP, "%s: %zu B of LDS per problem (%d slots, %d candidates, shortlists of %d) exceed a CU (160 KB)%s", who, lds,
                       max_slots, max_cand, rank, hint);
        if (build == Build::tabu)
            GNNPN_FAIL(GNNPN_E_UNSUP, "%s: %zu B of LDS per problem (%d slots, %d candidates) exceed a CU (160 KB)%s", who, lds, max_slots,
                       max_cand, hint);
        if (use_wide)
            GNNPN_FAIL(GNNPN_E_UNSUP, "%s: %d slots need %zu B of LDS for the four QoS columns (a CU has 160 KB)", who, max_slots, lds);
        GNNPN_FAIL(GNNPN_E_UNSUP, "%s: %zu B of LDS per problem (%d candidates) exceed a CU%s", who, lds, max_cand, hint);
    };
    char entry[80];
    snprintf(entry, sizeof(entry), "%s_f64%s", who, use_wide ? " (workgroup form)" : "");
    const Shape sh{a.prob_ptr, 0, max_slots, use_wide ? max_slots : 64, own || !use_wide ? max_cand : 0, a.n_lists, a.best_rows};
    return search_launch(lds, too_large, use_wide ? wide : lane, a.B, use_wide ? WNT : 64, a.stream, entry, sh, a.cand_ptr, a.cand, a.bounds,
                         a.start_pos, a.max_sweeps, rest...);
}

extern "C" int gnnpn_descend_ragged_f64(int32_t B, const int32_t* prob_ptr, int32_t n_lists, int32_t max_slots, int32_t max_cand,
                                        const int32_t* cand_ptr, const double* cand, const double* bounds, const int32_t* start_pos,
                                        int32_t max_sweeps, int32_t wide, double* best_fitness, double* start_fitness,
                                        int32_t* best_pos, double* best_rows, double* history, int32_t* sweeps, int32_t* moves,
                                        void* stream) {
    return descend_entry("descend_ragged", Build::one_swap, false,
                         {B, prob_ptr, n_lists, max_slots, max_cand, cand_ptr, cand, bounds, start_pos, max_sweeps, wide, best_rows, stream}, 0, true,
                         best_fitness && start_fitness && best_pos && history && sweeps && moves, descend_kernel, descend_wide_kernel,
                         best_fitness, start_fitness, best_pos, history, sweeps, moves);
}

// Tabu walk (new: no reference counterpart).  max_cand >= 1 in both forms: it sizes expire.
extern "C" int gnnpn_descend_tabu_ragged_f64(int32_t B, const int32_t* prob_ptr, int32_t n_lists, int32_t max_slots, int32_t max_cand,
                                             const int32_t* cand_ptr, const double* cand, const double* bounds, const int32_t* start_pos,
                                             int32_t max_sweeps, int32_t max_steps, int32_t tenure, int32_t wide, double* best_fitness,
                                             double* start_fitness, int32_t* best_pos, double* best_rows, double* history, int32_t* sweeps,
                                             int32_t* moves, double* walk, int32_t* steps, int32_t* best_step, int32_t* stalled,
                                             void* stream) {
    const TabuOut o{best_fitness, start_fitness, best_pos, history, sweeps, moves, walk, steps, best_step, stalled, nullptr};
    return descend_entry("descend_tabu_ragged", Build::tabu, false,
                         {B, prob_ptr, n_lists, max_slots, max_cand, cand_ptr, cand, bounds, start_pos, max_sweeps, wide, best_rows, stream}, 0,
                         max_steps >= 0 && tenure >= 0,
                         best_fitness && start_fitness && best_pos && history && sweeps && moves && walk && steps && best_step && stalled,
                         descend_tabu_kernel, descend_tabu_wide_kernel, max_steps, tenure, o);
}

// Tabu walk over pair moves (new: no reference counterpart): gnnpn_descend_tabu_ragged_f64 whose step takes the best admissible single
// swap or pair swap of the slots' shortlists.  max_rank = 0, or above max_cand: whole lists (run with the rank max_cand: no list is
// longer than its problem's table).  max_cand >= 1 in both forms: it sizes expire and the merit buffer.
extern "C" int gnnpn_descend_tabu_pairs_ragged_f64(int32_t B, const int32_t* prob_ptr, int32_t n_lists, int32_t max_slots, int32_t max_cand,
                                                   const int32_t* cand_ptr, const double* cand, const double* bounds,
                                                   const int32_t* start_pos, int32_t max_sweeps, int32_t max_steps, int32_t tenure,
                                                   int32_t max_span, int32_t max_rank, int32_t wide, double* best_fitness,
                                                   double* start_fitness, int32_t* best_pos, double* best_rows, double* history,
                                                   int32_t* sweeps, int32_t* moves, double* walk, int32_t* steps, int32_t* best_step,
                                                   int32_t* stalled, int32_t* pair_steps, void* stream) {
    const TabuOut o{best_fitness, start_fitness, best_pos, history, sweeps, moves, walk, steps, best_step, stalled, pair_steps};
    const int rank = max_rank > 0 && max_rank < max_cand ? max_rank : max_cand;
    return descend_entry("descend_tabu_pairs_ragged", Build::tabu_pairs, false,
                         {B, prob_ptr, n_lists, max_slots, max_cand, cand_ptr, cand, bounds, start_pos, max_sweeps, wide, best_rows, stream}, rank,
                         max_steps >= 0 && tenure >= 0 && max_span >= 0 && max_rank >= 0,
                         best_fitness && start_fitness && best_pos && history && sweeps && moves && walk && steps && best_step && stalled &&
                             pair_steps,
                         descend_tabu_pairs_kernel, descend_tabu_pairs_wide_kernel, max_steps, tenure, max_span, rank, o);
}

// The three pair entries, each with 0 / NULL where it has no span, rank, wide (in `a`) or shortlist.  max_rank = 0: the same launch
// from every entry, nothing extra.  max_rank > 0: the shortlist builds, run with the rank clamped to max_cand (no list is longer than
// its problem's table).
static int descend_pairs_entry(const char* who, bool lane_only, const DescendArgs& a, int32_t max_rounds, int32_t max_span, int32_t max_rank,
                               const PairOut& o, int32_t* shortlist) {
    const bool options_ok = max_rounds >= 0 && max_span >= 0 && max_rank >= 0;
    const bool given = o.best_fitness && o.start_fitness && o.best_pos && o.round_history && o.sweeps && o.moves && o.rounds && o.pair_moves &&
                       o.converged;
    if (max_rank == 0)
        return descend_entry(who, Build::pairs, lane_only, a, 0, options_ok, given, descend_pairs_kernel, descend_pairs_wide_kernel, max_rounds,
                             max_span, o);
    const int rank = max_rank < a.max_cand ? max_rank : a.max_cand;
    return descend_entry(who, Build::shortlist, lane_only, a, rank, options_ok, given, descend_pairs_shortlist_kernel,
                         descend_pairs_shortlist_wide_kernel, max_rounds, max_span, rank, o, ShortOut{shortlist, max_rank});
}

extern "C" int gnnpn_descend_pairs_ragged_f64(int32_t B, const int32_t* prob_ptr, int32_t n_lists, int32_t max_slots, int32_t max_cand,
                                              const int32_t* cand_ptr, const double* cand, const double* bounds, const int32_t* start_pos,
                                              int32_t max_sweeps, int32_t max_rounds, double* best_fitness, double* start_fitness,
                                              int32_t* best_pos, double* best_rows, double* round_history, int32_t* sweeps, int32_t* moves,
                                              int32_t* rounds, int32_t* pair_moves, int32_t* converged, void* stream) {
    return descend_pairs_entry("descend_pairs_ragged", true,
        {B, prob_ptr, n_lists, max_slots, max_cand, cand_ptr, cand, bounds, start_pos, max_sweeps, 0, best_rows, stream}, max_rounds, 0, 0,
        {best_fitness, start_fitness, best_pos, round_history, sweeps, moves, rounds, pair_moves, converged}, nullptr);
}

extern "C" int gnnpn_descend_pairs_windowed_ragged_f64(int32_t B, const int32_t* prob_ptr, int32_t n_lists, int32_t max_slots,
                                                       int32_t max_cand, const int32_t* cand_ptr, const double* cand, const double* bounds,
                                                       const int32_t* start_pos, int32_t max_sweeps, int32_t max_rounds, int32_t max_span,
                                                       int32_t wide, double* best_fitness, double* start_fitness, int32_t* best_pos,
                                                       double* best_rows, double* round_history, int32_t* sweeps, int32_t* moves,
                                                       int32_t* rounds, int32_t* pair_moves, int32_t* converged, void* stream) {
    return descend_pairs_entry("descend_pairs_windowed_ragged", false,
        {B, prob_ptr, n_lists, max_slots, max_cand, cand_ptr, cand, bounds, start_pos, max_sweeps, wide, best_rows, stream}, max_rounds, max_span, 0,
        {best_fitness, start_fitness, best_pos, round_history, sweeps, moves, rounds, pair_moves, converged}, nullptr);
}

extern "C" int gnnpn_descend_pairs_shortlist_ragged_f64(int32_t B, const int32_t* prob_ptr, int32_t n_lists, int32_t max_slots,
                                                        int32_t max_cand, const int32_t* cand_ptr, const double* cand, const double* bounds,
                                                        const int32_t* start_pos, int32_t max_sweeps, int32_t max_rounds, int32_t max_span,
                                                        int32_t max_rank, int32_t wide, double* best_fitness, double* start_fitness,
                                                        int32_t* best_pos, double* best_rows, double* round_history, int32_t* sweeps,
                                                        int32_t* moves, int32_t* rounds, int32_t* pair_moves, int32_t* converged,
                                                        int32_t* shortlist, void* stream) {
    return descend_pairs_entry("descend_pairs_shortlist_ragged", false,
        {B, prob_ptr, n_lists, max_slots, max_cand, cand_ptr, cand, bounds, start_pos, max_sweeps, wide, best_rows, stream}, max_rounds, max_span,
        max_rank, {best_fitness, start_fitness, best_pos, round_history, sweeps, moves, rounds, pair_moves, converged}, shortlist);
}


// ---- selection among the replicas of a problem: one wavefront per problem -----------------------------------------------------------
// Rows are problem-major (row b * R + r = replica r of problem b, what one gnnpn_descend_ragged_f64 launch over B * R rows wrote).
// Lane l looks at replicas l, l + 64, ...; the key is (best_fitness, replica) under take_better's plain <, so a NaN never wins, equal
// merits (-0.0 and 0.0 among them) go to the lowest replica, and where every row is NaN (not searched) replica 0 is the answer and its
// NaN / -1 fields are what the caller sees.  Then the lanes copy the winner's fields; the start rows as 32-bit words, so float32 and
// float64 actions are one build.  No atomics, nothing shared with other workgroups; loops bounded by R, max_slots, hist_ld, actions_T.
struct SelectIo {
    const double* fit; const double* start_fit; const int32_t* sweeps; const int32_t* moves; const int32_t* n_slots;
    const int32_t* pos; const double* rows; const double* hist; const uint32_t* actions;
    double* fit_o; double* start_fit_o; int32_t* sweeps_o; int32_t* moves_o; int32_t* n_slots_o;
    int32_t* pos_o; double* rows_o; double* hist_o; uint32_t* actions_o; int32_t* start_index;
};

__global__ __launch_bounds__(64) void descend_select_kernel(int32_t R, int32_t max_slots, int32_t hist_ld, int32_t action_words, SelectIo io) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const size_t q0 = (size_t)b * R;
    double bf = INFINITY;
    int bc = INT_MAX;
    for (int r = lane; r < R; r += 64) take_better(bf, bc, io.fit[q0 + r], r);
    wave_argmin(bf, bc, lane);
    bc = __shfl(bc, 0);
    const int win = bc == INT_MAX ? 0 : bc;                           // every row NaN: replica 0
    const size_t q = q0 + win;
    if (lane == 0) {
        io.fit_o[b] = io.fit[q];
        io.start_fit_o[b] = io.start_fit[q];
        io.sweeps_o[b] = io.sweeps[q];
        io.moves_o[b] = io.moves[q];
        io.n_slots_o[b] = io.n_slots[q];
        io.start_index[b] = win;
    }
    for (int i = lane; i < max_slots; i += 64) io.pos_o[(size_t)b * max_slots + i] = io.pos[q * max_slots + i];
    for (int i = lane; i < max_slots * 4; i += 64) io.rows_o[(size_t)b * max_slots * 4 + i] = io.rows[q * max_slots * 4 + i];
    for (int i = lane; i < hist_ld; i += 64) io.hist_o[(size_t)b * hist_ld + i] = io.hist[q * hist_ld + i];
    for (int i = lane; i < action_words; i += 64) io.actions_o[(size_t)b * action_words + i] = io.actions[q * action_words + i];
}

extern "C" int gnnpn_descend_select_f64(int32_t B, int32_t R, int32_t max_slots, int32_t hist_ld, int32_t actions_T, int32_t action_row_words,
                                        const double* best_fitness, const double* start_fitness, const int32_t* sweeps, const int32_t* moves,
                                        const int32_t* n_slots, const int32_t* best_pos, const double* best_rows, const double* history,
                                        const void* actions, double* best_fitness_out, double* start_fitness_out, int32_t* sweeps_out,
                                        int32_t* moves_out, int32_t* n_slots_out, int32_t* best_pos_out, double* best_rows_out,
                                        double* history_out, void* actions_out, int32_t* start_index, void* stream) {
    GNNPN_REQUIRE(B >= 0 && R >= 1 && max_slots >= 1 && hist_ld >= 0 && actions_T >= 0 && action_row_words >= 1, "descend_select: bad argument");
    GNNPN_REQUIRE((int64_t)B * R <= INT32_MAX, "descend_select: bad argument: %d problems x %d replicas exceed int32", B, R);
    GNNPN_REQUIRE((int64_t)max_slots * 4 <= INT32_MAX && (int64_t)actions_T * action_row_words <= INT32_MAX,
                  "descend_select: bad argument: a row of %d slots or %d x %d action words exceeds int32", max_slots, actions_T, action_row_words);
    if (B == 0) return GNNPN_OK;
    GNNPN_REQUIRE(best_fitness && start_fitness && sweeps && moves && n_slots && best_pos && best_rows && best_fitness_out &&
                  start_fitness_out && sweeps_out && moves_out && n_slots_out && best_pos_out && best_rows_out && start_index,
                  "descend_select: null operand");
    GNNPN_REQUIRE(hist_ld == 0 || (history && history_out), "descend_select: null operand (history)");
    GNNPN_REQUIRE(actions_T == 0 || (actions && actions_out), "descend_select: null operand (actions)");
    GNNPN_REQUIRE(actions_T == 0 || (gnnpn_aligned(actions, 4) && gnnpn_aligned(actions_out, 4)), "descend_select: misaligned actions");
    const SelectIo io{best_fitness, start_fitness, sweeps, moves, n_slots, best_pos, best_rows, history, static_cast<const uint32_t*>(actions),
                      best_fitness_out, start_fitness_out, sweeps_out, moves_out, n_slots_out, best_pos_out, best_rows_out, history_out,
                      static_cast<uint32_t*>(actions_out), start_index};
    hipLaunchKernelGGL(descend_select_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, R, max_slots, hist_ld, actions_T * action_row_words, io);
    GNNPN_CHECK_LAUNCH("descend_select_f64");
    return GNNPN_OK;
}
