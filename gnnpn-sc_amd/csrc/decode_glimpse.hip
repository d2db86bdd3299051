// Pointer decode with the attention forms the reference's configurations leave switched off:
// 'Bahdanau' attention (modelPN.py:80-90,103-109) and glimpse rounds (:208-211), for either attention name.
//
// General form, one workgroup per problem for all T steps (as decode.hip, no inter-workgroup communication); the
// shipped configuration ('Dot', no glimpses) never comes here.  Per step k (modelPN.py:204-239):
//   decoder LSTM cell                       two k-ordered fmaf-chain GEMVs streamed from L2 (recurrent.h)
//   query = h; n_glimpses times:            logits over ALL L positions (a glimpse is not windowed), -inf at the positions
//                                           chosen so far (:165-173), softmax over L, query = ref' . softmax  (:209-211)
//   pointer logits of the step's window     the only positions the window mask keeps (:220-222); C*tanh (:119-120)
//   + latent (High net), softmax over the window, first-max argmax, gather of the next input and of the action row.
// Attention (modelPN.py:92-122):  Dot:      logits_l = ref_l . q,                      ref' = ref
//                                 Bahdanau: logits_l = V . tanh(W_query q + b + R_l),  ref' = R = W_ref(ref) + b_ref
// R (the 1x1 Conv1d of enc_out) does not depend on the step and is precomputed by the caller with gnnpn_linear_f32.
#include "common.h"
#include <string.h>
#include "recurrent.h"
#include "decode_shared.h"

namespace {

struct AttnSide {          // one Attention module
    const float* wq;       // [H,H] W_query.weight (row-major, as stored)      Bahdanau only
    const float* bq;       // [H]
    const float* ref;      // [B,L,H] W_ref(enc_out) + bias                     Bahdanau only
    const float* v;        // [H]
};

// logits of positions [l0, l0+n) for query q (LDS), one wavefront per position; out[i] for position l0+i
template <int H, int NT, bool BAHDANAU>
__device__ __forceinline__ void attention_logits(const float* __restrict__ enc_b, const AttnSide& a, const float* ref_b,
                                                 const float* q, const float* qw, int l0, int n, float* out) {
    constexpr int NW = NT / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < n; i += NW) {
        const float* row = (BAHDANAU ? ref_b : enc_b) + (int64_t)(l0 + i) * H;
        float part = 0.0f;
        if constexpr (BAHDANAU) {
            for (int e = lane * 4; e < H; e += 256) {
                const float4 rv = *reinterpret_cast<const float4*>(row + e);
                const float4 qv = *reinterpret_cast<const float4*>(qw + e);
                const float4 vv = *reinterpret_cast<const float4*>(a.v + e);
                part = fmaf(vv.x, tanhf(__fadd_rn(qv.x, rv.x)), part);
                part = fmaf(vv.y, tanhf(__fadd_rn(qv.y, rv.y)), part);
                part = fmaf(vv.z, tanhf(__fadd_rn(qv.z, rv.z)), part);
                part = fmaf(vv.w, tanhf(__fadd_rn(qv.w, rv.w)), part);
            }
        } else {
            part = lane_dot4<H>(row, q);
        }
        const float dot = wave_sum(part);
        if (lane == 0) out[i] = dot;
    }
}

template <int H, bool BAHDANAU>
__global__ __launch_bounds__((H < 64 ? 64 : H)) void pointer_decode_glimpse_kernel(DecodeNet net, AttnSide ptr, AttnSide gl,
                                                                                  const float* __restrict__ inputs,
                                                                                  int n_glimpses, float tanh_c, int use_tanh,
                                                                                  int32_t B, int32_t T, int32_t n_per) {
    constexpr int NT = H < 64 ? 64 : H;
    extern __shared__ __attribute__((aligned(16))) float dyn[];   // lg[L] (glimpse logits / probabilities), chosen[T]
    __shared__ __attribute__((aligned(16))) float xs[1][H];
    __shared__ __attribute__((aligned(16))) float hs[2][1][H];
    __shared__ __attribute__((aligned(16))) float qv[H];
    __shared__ __attribute__((aligned(16))) float qw[H];
    __shared__ float win[64];
    __shared__ float red[NT / 64];
    __shared__ int sel;

    const int j = threadIdx.x, b = blockIdx.x;
    const bool owner = j < H;
    const int L = T * n_per;
    float* lg = dyn;
    int* chosen = reinterpret_cast<int*>(dyn + L);
    const float4* __restrict__ Wi = reinterpret_cast<const float4*>(net.wih);
    const float4* __restrict__ Wh = reinterpret_cast<const float4*>(net.whh);
    const float* enc_b = net.enc_out + (int64_t)b * L * H;
    const float* pref_b = BAHDANAU ? ptr.ref + (int64_t)b * L * H : nullptr;
    const float* gref_b = BAHDANAU ? gl.ref + (int64_t)b * L * H : nullptr;

    float bi[4], bh[4], c[1], h[1];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        bi[g] = owner ? net.bih[g * H + j] : 0.0f;
        bh[g] = owner ? net.bhh[g * H + j] : 0.0f;
    }
    c[0] = owner ? net.c0[(int64_t)b * H + j] : 0.0f;
    h[0] = owner ? net.h0[(int64_t)b * H + j] : 0.0f;
    if (owner) {
        hs[0][0][j] = h[0];
        xs[0][j] = net.start[j];
    }
    __syncthreads();

    int cur = 0;
    for (int k = 0; k < T; ++k) {
        // ---- decoder LSTM cell (modelPN.py:205)
        if (owner) {
            float ai[1][4] = {{0.f, 0.f, 0.f, 0.f}}, ah[1][4] = {{0.f, 0.f, 0.f, 0.f}};
            gemv_chain<H, 1>(Wi, xs, j, ai);
            gemv_chain<H, 1>(Wh, hs[cur], j, ah);
            float gate[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) gate[g] = __fadd_rn(__fadd_rn(ah[0][g], bh[g]), __fadd_rn(ai[0][g], bi[g]));
            lstm_cell_update(gate[0], gate[1], gate[2], gate[3], c[0], h[0]);
            hs[cur ^ 1][0][j] = h[0];
            qv[j] = h[0];                                              // query = hidden (:207)
        }
        __syncthreads();
        cur ^= 1;

        // ---- glimpse rounds (:208-211)
        for (int g = 0; g < n_glimpses; ++g) {
            if constexpr (BAHDANAU) {   // W_query q + b: one fmaf chain per output, inputs ascending
                if (owner) {
                    float acc = 0.0f;
                    const float* wr = gl.wq + (int64_t)j * H;
                    for (int i = 0; i < H; ++i) acc = fmaf(wr[i], qv[i], acc);
                    qw[j] = __fadd_rn(acc, gl.bq[j]);
                }
                __syncthreads();
            }
            attention_logits<H, NT, BAHDANAU>(enc_b, gl, gref_b, qv, qw, 0, L, lg);
            __syncthreads();
            for (int i = j; i < k; i += NT) lg[chosen[i]] = -INFINITY;   // the positions chosen so far (:169-172)
            __syncthreads();
            float m = -INFINITY;
            for (int l = j; l < L; l += NT) m = fmaxf(m, lg[l]);
            m = block_max<NT>(m, red);
            float s = 0.0f;
            for (int l = j; l < L; l += NT) {
                const float e = expf(__fsub_rn(lg[l], m));
                lg[l] = e;
                s = __fadd_rn(s, e);
            }
            s = block_sum<NT>(s, red);
            __syncthreads();
            // query = ref' . softmax (:211): thread j owns output j, positions ascending
            if (owner) {
                const float* rp = (BAHDANAU ? gref_b : enc_b) + j;
                float acc = 0.0f;
                for (int l = 0; l < L; ++l) acc = fmaf(rp[(int64_t)l * H], lg[l] / s, acc);
                qw[j] = acc;                                           // qv is still being read by the others
            }
            __syncthreads();
            if (owner) qv[j] = qw[j];
            __syncthreads();
        }

        // the query the pointer sees (after the glimpse rounds): what the full-length logits of the step are formed from on demand
        if (owner && net.queries) net.queries[((int64_t)b * T + k) * H + j] = qv[j];
        // ---- pointer logits of the step's window (:213; every other position is -inf after :220-222)
        if constexpr (BAHDANAU) {
            if (owner) {
                float acc = 0.0f;
                const float* wr = ptr.wq + (int64_t)j * H;
                for (int i = 0; i < H; ++i) acc = fmaf(wr[i], qv[i], acc);
                qw[j] = __fadd_rn(acc, ptr.bq[j]);
            }
            __syncthreads();
        }
        attention_logits<H, NT, BAHDANAU>(enc_b, ptr, pref_b, qv, qw, k * n_per, n_per, win);
        __syncthreads();

        // ---- C*tanh, latent bias, softmax, first-max argmax
        if (j == 0) {
            const int64_t wbase = ((int64_t)b * T + k) * n_per;
            float prob;   // the draw of decode.hip: problem b, step k -> counter b * T + k of the stream of sample_seed
            const int best_r = window_pick(win, n_per, tanh_c, use_tanh, net.win_logits, wbase, net.latent_win, wbase,
                                           net.sample, net.sample_seed, (unsigned long long)b * T + k, prob);
            net.pick_prob[(int64_t)b * T + k] = prob;
            net.idx[(int64_t)b * T + k] = k * n_per + best_r;
            sel = k * n_per + best_r;
            chosen[k] = k * n_per + best_r;
        }
        __syncthreads();

        // ---- gathers: next decoder input (:235) and the action row (:293-295)
        const int64_t row = (int64_t)b * L + sel;
        if (owner) xs[0][j] = net.embedded[row * H + j];
        if (j < 8) net.actions[((int64_t)b * T + k) * 8 + j] = inputs[row * 8 + j];
        __syncthreads();
    }
}

template <int H>
int launch_glimpse(const DecodeNet& net, const AttnSide& ptr, const AttnSide& gl, const float* inputs, int attention,
                   int n_glimpses, float tanh_c, int use_tanh, int32_t B, int32_t T, int32_t n_per, hipStream_t s) {
    constexpr int NT = H < 64 ? 64 : H;
    const size_t dyn = ((size_t)T * n_per + (size_t)T) * 4;
    if (dyn > 120 * 1024) GNNPN_FAIL(GNNPN_E_UNSUP, "pointer_decode_attn: seq_len %d does not fit the LDS buffer", T * n_per);
    return gnnpn_launch_lds(attention == 1 ? pointer_decode_glimpse_kernel<H, true> : pointer_decode_glimpse_kernel<H, false>, dim3(B),
                            dim3(NT), dyn, s, "pointer_decode_attn_f32", net, ptr, gl, inputs, n_glimpses, tanh_c, use_tanh, B, T, n_per);
}

}  // namespace

extern "C" int gnnpn_pointer_decode_attn_f32(const gnnpn_decode_net_t* net_in, const gnnpn_attention_t* attn,
                                             const float* inputs, float tanh_c, int use_tanh, int32_t B, int32_t T,
                                             int32_t n_per, int32_t H, void* stream) {
    GNNPN_REQUIRE(B >= 0 && T >= 1 && n_per >= 1 && n_per <= 64, "pointer_decode_attn: B >= 0, T >= 1, 1 <= n_per <= 64");
    if (B == 0) return GNNPN_OK;
    GNNPN_REQUIRE(net_in && attn && inputs, "pointer_decode_attn: null argument");
    GNNPN_REQUIRE(H == 256 || H == 32, "pointer_decode_attn: built for H = 256 and H = 32, got %d", H);
    GNNPN_REQUIRE(attn->attention == 0 || attn->attention == 1, "pointer_decode_attn: attention 0 ('Dot') or 1 ('Bahdanau')");
    GNNPN_REQUIRE(attn->n_glimpses >= 0, "pointer_decode_attn: n_glimpses >= 0");
    if (const int rc = decode_net_check(*net_in, "pointer_decode_attn", 0)) return rc;
    GNNPN_REQUIRE(net_in->embedded, "pointer_decode_attn: the embedded tensor is required");
    DecodeNet net;
    memcpy(&net, net_in, sizeof(net));
    AttnSide ptr{attn->pointer_wq, attn->pointer_bq, attn->pointer_ref, attn->pointer_v};
    AttnSide gl{attn->glimpse_wq, attn->glimpse_bq, attn->glimpse_ref, attn->glimpse_v};
    if (attn->attention == 1) {
        GNNPN_REQUIRE(ptr.wq && ptr.bq && ptr.ref && ptr.v, "pointer_decode_attn: 'Bahdanau' needs the pointer's W_query, bias, W_ref(enc_out) and V");
        if (attn->n_glimpses > 0)
            GNNPN_REQUIRE(gl.wq && gl.bq && gl.ref && gl.v, "pointer_decode_attn: 'Bahdanau' glimpses need the glimpse's W_query, bias, W_ref(enc_out) and V");
    }
    hipStream_t s = (hipStream_t)stream;
    int rc;
    GNNPN_FOR_H(H, rc = launch_glimpse<HH>(net, ptr, gl, inputs, attn->attention, attn->n_glimpses, tanh_c, use_tanh, B, T, n_per, s));
    if (rc != GNNPN_OK) return rc;
    GNNPN_CHECK_LAUNCH("pointer_decode_attn_f32");
    return GNNPN_OK;
}
