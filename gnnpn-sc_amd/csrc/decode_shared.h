// Argument blocks shared by the decoder implementations (decode.hip, decode_coop.hip, decode_lean.hip, decode_glimpse.hip), what
// every entry point checks of a net, and the step stages the two per-workgroup kernels share.
#pragma once
#include "common.h"
#include "lstm_shared.h"   // CoopOpts

// device-side view of gnnpn_decode_net_t (same field order; see include/gnnpn_hip.h)
struct DecodeNet {
    const float* embedded;
    const float* enc_out;
    const float* h0;
    const float* c0;
    const float* start;
    const float* wih;
    const float* whh;
    const float* bih;
    const float* bhh;
    const float* latent_win;
    const float* emb_w;
    const float* emb_b;
    const float* xw_fold;
    const float* xb_fold;
    const float* start_fold;
    int32_t* idx;
    float* win_logits;
    float* pick_prob;
    float* actions;
    float* queries;
    int32_t latent_from;
    int32_t sample;
    uint64_t sample_seed;
    const void* whh_split;       // or nullptr (gnnpn_lstm_pack_split_weights_f32)
};
static_assert(sizeof(DecodeNet) == sizeof(gnnpn_decode_net_t), "DecodeNet must mirror gnnpn_decode_net_t");

// What every decode entry point asks of a net (`who`: the entry point; each adds its own rules: where the decoder inputs come
// from, latent_from, queries)
inline int decode_net_check(const gnnpn_decode_net_t& d, const char* who, int n) {
    GNNPN_REQUIRE(d.enc_out && d.h0 && d.c0 && d.start && d.wih_packed && d.whh_packed && d.bih && d.bhh,
                  "%s: null input of net %d (enc_out, h0, c0, start and the decoder weights are required)", who, n);
    GNNPN_REQUIRE(d.idx && d.win_logits && d.pick_prob && d.actions, "%s: null output of net %d", who, n);
    GNNPN_REQUIRE((d.xw_fold != nullptr) == (d.xb_fold != nullptr) && (d.xw_fold != nullptr) == (d.start_fold != nullptr),
                  "%s: net %d: xw_fold, xb_fold and start_fold go together", who, n);
    GNNPN_REQUIRE(d.sample == 0 || d.sample == 1, "%s: net %d: sample must be 0 (greedy) or 1 (multinomial)", who, n);
    GNNPN_REQUIRE(gnnpn_aligned(d.wih_packed, 16) && gnnpn_aligned(d.whh_packed, 16) && gnnpn_aligned(d.enc_out, 16) &&
                      (!d.embedded || gnnpn_aligned(d.embedded, 16)),
                  "%s: weights / enc_out / embedded must be 16-byte aligned", who);
    return GNNPN_OK;
}

// ---- stages of a decode step shared by the per-workgroup kernels (decode.hip, decode_glimpse.hip) ---------------------------
// One lane's share of row . q over H floats by a wavefront (row: global, q: LDS, both 16-byte aligned): 16 B per lane and pass,
// elements ascending; wave_sum of it is the dot product
template <int H>
__device__ __forceinline__ float lane_dot4(const float* __restrict__ row, const float* q) {
    float part = 0.0f;
    for (int e = (threadIdx.x & 63) * 4; e < H; e += 256) {
        const float4 rv = *reinterpret_cast<const float4*>(row + e);
        const float4 qv = *reinterpret_cast<const float4*>(q + e);
        part = fmaf(rv.x, qv.x, part);
        part = fmaf(rv.y, qv.y, part);
        part = fmaf(rv.z, qv.z, part);
        part = fmaf(rv.w, qv.w, part);
    }
    return part;
}

// The pick of one step by one thread, from the K raw window logits in LDS `lg` (overwritten with what the softmax sees):
// C*tanh (modelPN.py:119-120) -> win_logits[wbase + r], + latent_win[lbase + r] (High net; or null), softmax over the window, then
// the first maximum (torch.max on CPU returns the first maximal index) or, with `sample`, multinomial(1) of the softmax (:227-228):
// the first r with u < cdf_r, u = draw `ctr` of the stream of `seed`, else the last entry of positive probability.
// Returns the pick's position in the window, its probability in `prob`.
__device__ __forceinline__ int window_pick(float* lg, int K, float tanh_c, int use_tanh, float* __restrict__ win_logits, int64_t wbase,
                                           const float* __restrict__ latent_win, int64_t lbase, int sample, unsigned long long seed,
                                           unsigned long long ctr, float& prob) {
    float best = 0.0f;
    int best_r = -1;
    for (int r = 0; r < K; ++r) {
        float v = lg[r];
        if (use_tanh) v = __fmul_rn(tanh_c, tanhf(v));
        win_logits[wbase + r] = v;
        if (latent_win) v = __fadd_rn(v, latent_win[lbase + r]);
        lg[r] = v;
        if (best_r < 0 || v > best) {   // strict '>' keeps the first maximum
            best = v;
            best_r = r;
        }
    }
    float denom = 0.0f;
    for (int r = 0; r < K; ++r) denom = __fadd_rn(denom, expf(__fsub_rn(lg[r], best)));
    prob = 1.0f / denom;                              // exp(best-best)/sum
    if (sample) {
        const float u = stream_uniform24(seed, ctr);
        float cdf = 0.0f;
        int pick = -1, last_pos = 0;
        for (int r = 0; r < K; ++r) {
            const float pr = expf(__fsub_rn(lg[r], best)) / denom;
            cdf = __fadd_rn(cdf, pr);
            if (pr > 0.0f) last_pos = r;
            if (pick < 0 && u < cdf) pick = r;
        }
        if (pick < 0) pick = last_pos;
        best_r = pick;
        prob = expf(__fsub_rn(lg[pick], best)) / denom;
    }
    return best_r;
}

#define GNNPN_MAX_DECODE_NETS 2

struct DecodeArgs {
    DecodeNet net[GNNPN_MAX_DECODE_NETS];
    const float* inputs;
    float tanh_c;
    int use_tanh;
    int32_t B, T, K;
};

// Sampled replicas (gnnpn_pointer_decode_replicas_f32): R = 0 — rows are problems, draws from net.sample_seed (every other
// call); R >= 1 — args.B counts rows, row b is replica first + b % R of problem b / R, whose inputs it reads, drawing from
// replica_seed(net.sample_seed, first + b % R) at key (b / R) * T + k.  Read only by the sampling builds.
struct ReplicaMap {
    int32_t R;
    int32_t first;
};

bool gnnpn_decode_coop_supported(int32_t H, int32_t n_per);
int64_t gnnpn_decode_coop_workspace_need(int64_t rows, int32_t T, int32_t n_per);   // decode_coop.hip, no device call
int gnnpn_launch_decode_coop(const DecodeArgs& args, int n_nets, int precision, bool shared_cu, const CoopOpts& opts,
                             void* workspace, int64_t workspace_bytes, hipStream_t s, ReplicaMap rep = ReplicaMap{0, 0});
// decode_lean.hip: the production build of the cooperative form (folded input side, greedy picks; fp32 and exact split)
int gnnpn_launch_decode_lean(const DecodeArgs& args, int n_nets, int precision, bool shared_cu, const CoopOpts& opts,
                             void* workspace, int64_t workspace_bytes, hipStream_t s);
int64_t gnnpn_decode_lean_workspace_bytes(int32_t B, int32_t T, int32_t n_per);
