// Score product + candidate reduction of an inference step in ONE launch (hidden size 128, n_per <= 16, categories of 16
// services and more on average): what linear_f32_kernel (dense.hip, sigmoid epilogue) followed by select_candidates16_kernel
// (select.hip) compute, without the second kernel reading the [B, S] scores back and without its n_per rescans of a category.
//
// Grid: (tiles of 16 problems) x (chunks of whole categories).  The chunks are planned on the host from the service table alone
// (about one workgroup per CU; at most MAX_TILES 16-column tiles and MAX_CATS categories per chunk) and the service embedding arrives packed as
// v_mfma_f32_16x16x4_f32 B-fragments, one run of 16-column tiles per category (zero columns behind a category's last service):
// a layout change made once per (weights, service table), no arithmetic.
//   1. product: every wave takes 16-column tiles of the chunk in turn — 32 MFMAs, k ascending from zero accumulators, which is
//      the per-element fma chain linear_f32_kernel forms with 32x32x2 (request_branch.hip rests on the same equivalence) — then
//      epilogue_element(sigmoid) unchanged; the tile goes to `scores` AND stays in LDS.
//   2. selection: one 16-lane DPP row per (problem, category), so the workgroup reduces 16 segments at once.  The chunk's QoS
//      rows were staged in LDS once for all 16 problems; a lane forms the rank_key of its services ONCE (0: infeasible)
//      and the n_per rounds (pick_rounds) are row16_max_u64 over those registers under the `key < last` filter.  Rows and ids
//      leave through select.hip's writer too (select_keys.h: cyclic_pick, emit_row).
#include "common.h"
#include "select_keys.h"

typedef float ss_f32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int PT = 16;                      // problems per workgroup (MFMA M)
// Threads of a workgroup: NT / 64 waves share the chunk's tiles, NT / 256 categories are reduced side by side (16 rows of 16 lanes
// each).  256, one wave per SIMD: beside the other slot's cooperative workgroup (about 250 registers per lane, one wave per SIMD) a
// second wave of this kernel's 136 registers does not fit a SIMD — the 512-thread build is 3 us shorter alone (11.3 against
// 14.2 us at the QWS shape) and made the two-slot step 20 % slower, its workgroups waiting for CUs without a cooperative one.
constexpr int NT = 256;
constexpr int NW = NT / 64, CSLOTS = NT / 256;
constexpr int HID = 128;                    // hiddenChannels
constexpr int KB = HID / 16;                // B-fragment wave-loads (1 KiB each) per 16-column tile
constexpr int LDA = HID + 2;                // request rows in LDS: (row*2 + kq) distinct banks for the A-fragment reads
constexpr int MAX_TILES = GNNPN_SCORE_SELECT_MAX_TILES;   // 16-column tiles of one chunk
constexpr int MAX_CATS = GNNPN_SCORE_SELECT_MAX_CHUNK_CATEGORIES;
constexpr int LDSC = MAX_TILES * 16 + 16;   // score rows in LDS: the four rows of a wave start 16 banks apart
constexpr int CAP = GNNPN_SCORE_SELECT_MAX_CATEGORY;      // services of the largest category
constexpr int KPL = CAP / 16;               // keys a lane holds

struct ScoreSelectArgs {
    const float* xr;                        // [B, ldx] request embedding
    const float4* emb;                      // packed service embedding [n_tiles][KB][64] float4
    const int32_t* cat_ptr;                 // [T + 1]            (the plan's copy, on the device)
    const int32_t* tile_ptr;                // [T + 1]   first tile of a category
    const int32_t* chunk_info;              // [n_chunks][8]  c0, c1, t0, n_tiles, s0, s1 of a chunk
    const double* qos;
    const double* local_bounds;
    const uint8_t* present;
    const double* global_bounds;
    float* scores;
    float* out_rows;
    int32_t* out_ids;
    int64_t ldx, ld_scores;
    int32_t B, T, n_per;
};

// The picks of one (problem, category) on a 16-lane row, the category's services dealt to the lanes NK to each (NK * 16 >= n):
// every lane reads its services' cost, quality and score from LDS at once (an index behind the category reads the last service
// and is discarded), forms each rank_key ONCE — 0: infeasible, absent or behind the category — and the n_per rounds reduce those
// registers.  Lane r of the row returns the r-th pick in `my_pick`; returns the number of picks found.
template <int NK>
__device__ __forceinline__ int select_row(const float* srow, const double* q4, const double* lb, bool pres, int s_begin, int n, int sub,
                                          int n_per, int& my_pick) {
    const CellBounds bounds = cell_bounds(lb);
    double cost[NK], qual[NK];
    float score[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) {
        const int sl = min(sub + 16 * j, n - 1);
        cost[j] = q4[sl * 4 + 2], qual[j] = q4[sl * 4 + 3], score[j] = srow[sl];
    }
    unsigned long long key[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) {
        const bool ok = pres && sub + 16 * j < n && feasible(cost[j], qual[j], bounds);
        const unsigned long long k = rank_key(score[j], (uint32_t)(s_begin + sub + 16 * j));
        key[j] = ok ? k : 0ull;
    }
    auto local_best = [&](unsigned long long last) {
        unsigned long long best = 0ull;
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            const unsigned long long k = key[j] < last ? key[j] : 0ull;
            best = k > best ? k : best;
        }
        return best;
    };
    return pick_rounds(n_per, sub, my_pick, local_best, [](unsigned long long v) { return row16_max_u64(v); });
}
}  // namespace

// Every global READ of a workgroup is requested in its first phase — the chunk's record, then at once the fragments of the first
// tiles, the request rows, the chunk's QoS rows, its category pointers and the 16 problems' bounds and presence bytes — so the
// kernel pays two memory round trips; the product and the selection behind them run out of LDS and registers and only store.
__global__ __launch_bounds__(NT) void score_select_kernel(ScoreSelectArgs a) {
    __shared__ float As[PT * LDA];
    __shared__ float sc[PT * LDSC];
    __shared__ double qs4[MAX_TILES * 16 * 4];                          // the chunk's QoS rows
    __shared__ double lbs[MAX_CATS * PT * 4];                           // local bounds of (category of the chunk, problem)
    __shared__ int cat_s[MAX_CATS + 1], cat_t[MAX_CATS + 1];            // first service / first tile of the chunk's categories
    __shared__ int tile_s[MAX_TILES], tile_e[MAX_TILES];                // first service of a tile, end of its category
    __shared__ unsigned char pres_s[MAX_CATS * PT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * PT;
    const int32_t* info = a.chunk_info + 8 * blockIdx.y;
    const int c0 = info[0], c1 = info[1], t0 = info[2], nt = info[3], s0 = info[4], s1 = info[5];
    if (c0 >= c1) return;                                               // an empty chunk: the whole workgroup
    const int nc = c1 - c0;                                             // <= MAX_CATS, nt <= MAX_TILES (checked by the host)

    const float4* wv = a.emb + (size_t)t0 * KB * 64 + lane;
    float4 bnext[KB];
    if (wave < nt) {
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) bnext[kb] = wv[((size_t)wave * KB + kb) * 64];
    }
    // ---- the 16 request rows (zero rows behind the batch), the chunk's QoS rows, its pointers, the problems' bounds -> LDS
    for (int f = tid; f < PT * (HID / 4); f += NT) {
        const int r = f >> 5, k4 = f & 31;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b0 + r < a.B) v = *reinterpret_cast<const float4*>(a.xr + (int64_t)(b0 + r) * a.ldx + 4 * k4);
        float* d = As + r * LDA + 4 * k4;
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    }
    for (int i = tid; i < 2 * (s1 - s0); i += NT)
        *reinterpret_cast<double2*>(qs4 + 2 * i) = *reinterpret_cast<const double2*>(a.qos + (int64_t)s0 * 4 + 2 * i);
    if (tid <= nc) {
        const int cs = a.cat_ptr[c0 + tid], ct = a.tile_ptr[c0 + tid];
        cat_s[tid] = cs;
        cat_t[tid] = ct - t0;
        if (tid < nc) {
            const int ce = a.cat_ptr[c0 + tid + 1], te = a.tile_ptr[c0 + tid + 1];
            for (int t = ct; t < te; ++t) tile_s[t - t0] = cs + 16 * (t - ct), tile_e[t - t0] = ce;
        }
    }
    for (int i = tid; i < nc * PT; i += NT) {
        const int cl = i >> 4, pp = i & 15;
        pres_s[i] = b0 + pp < a.B ? a.present[(int64_t)(b0 + pp) * a.T + c0 + cl] : (unsigned char)0;
    }
    for (int i = tid; i < nc * PT * 2; i += NT) {
        const int cl = i >> 5, pp = (i >> 1) & 15, h = i & 1;
        double2 v = make_double2(0.0, 0.0);
        if (b0 + pp < a.B) v = *reinterpret_cast<const double2*>(a.local_bounds + ((int64_t)(b0 + pp) * a.T + c0 + cl) * 4 + 2 * h);
        *reinterpret_cast<double2*>(lbs + (cl * PT + pp) * 4 + 2 * h) = v;
    }
    float4 tail0 = make_float4(0.f, 0.f, 0.f, 0.f);                     // the global bounds: the tail of category 0's rows
    if (c0 == 0 && b0 + ((tid >> 4) & 15) < a.B) tail0 = qos_row_f32(a.global_bounds + (int64_t)(b0 + ((tid >> 4) & 15)) * 4);
    __syncthreads();

    // ---- 1. product: this wave's tiles; accumulator register r = problem 4*kq + r, column c16
    const int c16 = lane & 15, kq = lane >> 4;
    float afrag[KB][4];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int j = 0; j < 4; ++j) afrag[kb][j] = As[c16 * LDA + 16 * kb + 4 * j + kq];
    for (int tl = wave; tl < nt; tl += NW) {
        float4 bf[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) bf[kb] = bnext[kb];
        if (tl + NW < nt) {                                             // the next tile's fragments travel under these MFMAs
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) bnext[kb] = wv[((size_t)(tl + NW) * KB + kb) * 64];
        }
        ss_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(afrag[kb][0], bf[kb].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(afrag[kb][1], bf[kb].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(afrag[kb][2], bf[kb].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(afrag[kb][3], bf[kb].w, acc, 0, 0, 0);
        }
        const int s = tile_s[tl] + c16;                                 // this lane's service
        const bool col_ok = s < tile_e[tl];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = epilogue_element(acc[r], false, 0.0f, false, 1.0f, 0.0f, GNNPN_ACT_SIGMOID);
            const int p = 4 * kq + r;
            sc[p * LDSC + 16 * tl + c16] = v;
            if (col_ok && b0 + p < a.B) a.scores[(int64_t)(b0 + p) * a.ld_scores + s] = v;
        }
    }
    __syncthreads();

    // ---- 2. selection: a row of 16 lanes = problem b0 + p of one category; CSLOTS categories of the chunk side by side (the four
    // rows of a wave work on the same category)
    const int p = (tid >> 4) & 15, sub = tid & 15;
    const int b = b0 + p;
    const bool valid = b < a.B;
    const int n_per = a.n_per, T = a.T;
    for (int cl = tid >> 8; cl < nc; cl += CSLOTS) {
        const int c = c0 + cl;
        // (the same in the whole wave: in scalar registers, so that ONE size form of select_row runs)
        const int s_begin = __builtin_amdgcn_readfirstlane(cat_s[cl]);
        const int n = __builtin_amdgcn_readfirstlane(cat_s[cl + 1]) - s_begin;     // n <= CAP (checked by the host)
        const int nk = (n + 15) >> 4;
        const float* srow = sc + p * LDSC + 16 * __builtin_amdgcn_readfirstlane(cat_t[cl]);
        const double* q4 = qs4 + (s_begin - s0) * 4;
        const bool pres = pres_s[cl * PT + p] != 0;                     // (0 behind the batch)
        int my_pick = -1;   // lane r of the row keeps the r-th pick
        int n_found = 0;
        if (n > 0) {                                                    // nk: the same in every lane, so one form runs
            const double* lb = lbs + (cl * PT + p) * 4;
            if (nk <= 1) n_found = select_row<1>(srow, q4, lb, pres, s_begin, n, sub, n_per, my_pick);
            else if (nk <= 2) n_found = select_row<2>(srow, q4, lb, pres, s_begin, n, sub, n_per, my_pick);
            else if (nk <= 4) n_found = select_row<4>(srow, q4, lb, pres, s_begin, n, sub, n_per, my_pick);
            else if (nk <= 8) n_found = select_row<8>(srow, q4, lb, pres, s_begin, n, sub, n_per, my_pick);
            else n_found = select_row<KPL>(srow, q4, lb, pres, s_begin, n, sub, n_per, my_pick);
        }
        const int id = cyclic_pick(my_pick, n_found, lane & ~15, sub);
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n_found > 0 && sub < n_per) q = qos_row_f32(qs4 + (id - s0) * 4);          // the LDS copy of qos + id * 4
        if (valid && sub < n_per)
            emit_row(n_found, id, q, c, tail0, (int64_t)b * T * n_per + (int64_t)c * n_per + sub, a.out_rows, a.out_ids);
    }
}

// plan words (int32): T, n_chunks, n_tiles, S, then cat_ptr [T+1], tile_ptr [T+1], chunk_ptr [n_chunks+1], chunk_info [n_chunks][8]
extern "C" int gnnpn_score_select_f32(const float* xr, int64_t ldx, const float* emb_packed, const int32_t* plan_host,
                                      const int32_t* plan_dev, int32_t plan_words, const double* qos, const double* local_bounds,
                                      const uint8_t* present, const double* global_bounds, float* scores, int64_t ld_scores,
                                      float* out_rows, int32_t* out_ids, int32_t B, int32_t hidden, int32_t n_per, void* stream) {
    GNNPN_REQUIRE(B >= 0, "score_select: bad shape");
    GNNPN_REQUIRE(plan_host && plan_words >= 4, "score_select: null plan");
    const int32_t T = plan_host[0], n_chunks = plan_host[1], n_tiles = plan_host[2], S = plan_host[3];
    GNNPN_REQUIRE(T > 0 && n_chunks > 0 && n_tiles > 0 && S > 0 && (int64_t)plan_words == 4 + 2 * ((int64_t)T + 1) + 9 * (int64_t)n_chunks + 1,
                  "score_select: plan of %d words does not hold T=%d, n_chunks=%d", plan_words, T, n_chunks);
    if (hidden != HID || n_per < 1 || n_per > 16)
        GNNPN_FAIL(GNNPN_E_UNSUP, "score_select: built for hidden = %d and n_per in [1,16] (got hidden %d, n_per %d): use linear + select_candidates",
                   HID, hidden, n_per);
    const int32_t* cat = plan_host + 4;
    const int32_t* tile = cat + T + 1;
    const int32_t* chunk = tile + T + 1;
    const int32_t* info = chunk + n_chunks + 1;
    // everything the kernel indexes with is checked here: the plan decides what it reads and writes
    GNNPN_REQUIRE(cat[0] == 0 && cat[T] == S && tile[0] == 0 && tile[T] == n_tiles && chunk[0] == 0 && chunk[n_chunks] == T,
                  "score_select: the plan's pointers do not span S=%d services, %d tiles, T=%d categories", S, n_tiles, T);
    for (int32_t c = 0; c < T; ++c) {
        const int32_t n = cat[c + 1] - cat[c];
        GNNPN_REQUIRE(n >= 0 && tile[c + 1] - tile[c] == (n + 15) / 16, "score_select: category %d: %d services in %d tiles", c, n, tile[c + 1] - tile[c]);
        if (n > CAP) GNNPN_FAIL(GNNPN_E_UNSUP, "score_select: category %d has %d services, the kernel holds %d: use linear + select_candidates", c, n, CAP);
    }
    for (int32_t k = 0; k < n_chunks; ++k) {
        GNNPN_REQUIRE(chunk[k] >= 0 && chunk[k] <= chunk[k + 1] && chunk[k + 1] <= T, "score_select: chunk %d is not a run of categories", k);
        const int32_t c0 = chunk[k], c1 = chunk[k + 1];
        GNNPN_REQUIRE(tile[c1] - tile[c0] <= MAX_TILES, "score_select: chunk %d has %d tiles, a workgroup holds %d", k, tile[c1] - tile[c0], MAX_TILES);
        GNNPN_REQUIRE(c1 - c0 <= MAX_CATS, "score_select: chunk %d has %d categories, a workgroup holds %d", k, c1 - c0, MAX_CATS);
        const int32_t* r = info + 8 * k;
        GNNPN_REQUIRE(r[0] == c0 && r[1] == c1 && r[2] == tile[c0] && r[3] == tile[c1] - tile[c0] && r[4] == cat[c0] && r[5] == cat[c1],
                      "score_select: the record of chunk %d does not repeat the plan's pointers", k);
    }
    if (B == 0) return GNNPN_OK;
    GNNPN_REQUIRE(xr && emb_packed && plan_dev && qos && local_bounds && present && global_bounds && scores && out_rows && out_ids,
                  "score_select: null operand");
    GNNPN_REQUIRE(ldx >= HID && ldx % 4 == 0 && gnnpn_aligned(xr, 16) && gnnpn_aligned(emb_packed, 16) && gnnpn_aligned(qos, 16),
                  "score_select: the request embedding, the packed service embedding and qos must be 16-byte aligned (ldx a multiple of 4)");
    GNNPN_REQUIRE(ld_scores >= S, "score_select: ld_scores %lld < S = %d", (long long)ld_scores, S);
    GNNPN_REQUIRE(gnnpn_aligned(out_rows, 16), "score_select: out_rows must be 16-byte aligned");
    const unsigned ptiles = (unsigned)(((int64_t)B + PT - 1) / PT);
    GNNPN_REQUIRE(n_chunks <= 65535, "score_select: at most 65535 chunks");
    ScoreSelectArgs a{};
    a.xr = xr;
    a.emb = reinterpret_cast<const float4*>(emb_packed);
    a.cat_ptr = plan_dev + 4;
    a.tile_ptr = a.cat_ptr + T + 1;
    a.chunk_info = a.tile_ptr + T + 1 + n_chunks + 1;
    a.qos = qos;
    a.local_bounds = local_bounds;
    a.present = present;
    a.global_bounds = global_bounds;
    a.scores = scores;
    a.out_rows = out_rows;
    a.out_ids = out_ids;
    a.ldx = ldx;
    a.ld_scores = ld_scores;
    a.B = B;
    a.T = T;
    a.n_per = n_per;
    hipLaunchKernelGGL(score_select_kernel, dim3(ptiles, (unsigned)n_chunks), dim3(NT), gnnpn_front_lds_pad((const void*)score_select_kernel),
                       (hipStream_t)stream, a);
    GNNPN_CHECK_LAUNCH("score_select_f32");
    return GNNPN_OK;
}
