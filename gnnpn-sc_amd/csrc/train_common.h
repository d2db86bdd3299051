// Device helpers shared by the training kernels (train.hip: the shipped decoder; train_attn.hip: 'Bahdanau' attention / glimpses):
// one thread per hidden unit, weight matrices streamed from L2 with coalesced reads along the unit index.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// acc[g] += sum_k W[g*H + j][k] * v[k]  (forward product) from the TRANSPOSED matrix Wt[k][g*H + j] (k-major [H,4H]): for a
// fixed k the threads j of a wave read consecutive floats; k-ascending fma chain per gate
template <int H>
__device__ __forceinline__ void matvec_rows(const float* __restrict__ Wt, const float* v, int j, float (&acc)[4]) {
#pragma unroll 4
    for (int k = 0; k < H; ++k) {
        const float vk = v[k];
        const float* row = Wt + (size_t)k * (4 * H) + j;
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = fmaf(row[g * H], vk, acc[g]);
    }
}
// sum_gu W[gu][j] * d[gu]  (transposed product: column j of W, coalesced across the threads of a wave)
template <int H>
__device__ __forceinline__ float matvec_cols(const float* __restrict__ W, const float* d, int j) {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    for (int gu = 0; gu < 4 * H; gu += 4) {
        a0 = fmaf(W[(size_t)(gu + 0) * H + j], d[gu + 0], a0);
        a1 = fmaf(W[(size_t)(gu + 1) * H + j], d[gu + 1], a1);
        a2 = fmaf(W[(size_t)(gu + 2) * H + j], d[gu + 2], a2);
        a3 = fmaf(W[(size_t)(gu + 3) * H + j], d[gu + 3], a3);
    }
    return (a0 + a1) + (a2 + a3);
}

// logits of the positions [i0, i0 + n) against the query in LDS: one wavefront per position, one float per lane and pass (elements
// ascending per lane), fixed butterfly.  bah: V . tanh(qp + ref_i); else enc_i . q
template <int H, int NT>
__device__ __forceinline__ void attention_logits(bool bah, const float* __restrict__ rows, const float* qv, const float* __restrict__ v,
                                                 int i0, int n, float* out) {
    constexpr int NW = NT / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < n; i += NW) {
        const float* row = rows + (size_t)(i0 + i) * H;
        float part = 0.0f;
        for (int e = lane; e < H; e += 64) part = bah ? fmaf(v[e], tanhf(qv[e] + row[e]), part) : fmaf(row[e], qv[e], part);
        const float dot = wave_sum(part);
        if (lane == 0) out[i] = dot;
    }
}

// LSTM cell forward for one unit from its pre-activation gates: c updated, returns h
__device__ __forceinline__ float cell_forward(const float (&gate)[4], float& c) {
    c = sigm(gate[1]) * c + sigm(gate[0]) * tanhf(gate[2]);
    return sigm(gate[3]) * tanhf(c);
}

// The decoder's LSTM cell of step `step` (= b * T + k) for unit j, input xs and state hs in LDS: saves the input, the
// pre-activation gates, c and h in t's buffers (what the backward reads); c updated, returns h
template <int H>
__device__ __forceinline__ float decoder_cell_forward(const gnnpn_decode_train_t& t, const float* xs, const float* hs, int64_t step,
                                                      int j, float& c) {
    float gi[4] = {0.f, 0.f, 0.f, 0.f}, gh[4] = {0.f, 0.f, 0.f, 0.f};
    matvec_rows<H>(t.wih, xs, j, gi);
    matvec_rows<H>(t.whh, hs, j, gh);
    float gate[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        gate[g] = (gh[g] + t.bhh[g * H + j]) + (gi[g] + t.bih[g * H + j]);
        t.gates_pre[step * (4 * H) + g * H + j] = gate[g];
    }
    t.x_all[step * H + j] = xs[j];
    const float h = cell_forward(gate, c);
    t.c_all[step * H + j] = c;
    t.h_all[step * H + j] = h;
    return h;
}

// Window softmax of step `step` (= b * T + k) by one thread, from the K raw window logits in LDS `lg` (overwritten): C*tanh -> z0,
// + latent (a constant of the graph), softmax -> probs, log-probability of the given pick -> logp
__device__ __forceinline__ void window_softmax_logp(const gnnpn_decode_train_t& t, float* lg, int64_t step, int k, int K, float tanh_c,
                                                    int use_tanh) {
    const int64_t wb = step * K;
    float best = -INFINITY;
    for (int r = 0; r < K; ++r) {
        float v = use_tanh ? tanh_c * tanhf(lg[r]) : lg[r];
        t.z0[wb + r] = v;
        if (t.latent_win) v += t.latent_win[wb + r];
        lg[r] = v;
        best = fmaxf(best, v);
    }
    float denom = 0.0f;
    for (int r = 0; r < K; ++r) denom += expf(lg[r] - best);
    const int pick = t.idx[step] - k * K;
    for (int r = 0; r < K; ++r) t.probs[wb + r] = expf(lg[r] - best) / denom;
    t.logp[step] = (lg[pick] - best) - logf(denom);
}

// softmax -> (+ latent: constant) -> C*tanh backward of one window entry: d loss / d (its raw logit) from its probability p, its
// z0 = C*tanh(logit) (or the logit), whether it is the step's pick, and gs = d loss / d logp
__device__ __forceinline__ float window_du(float p, float z, bool picked, float gs, float tanh_c, int use_tanh) {
    const float dz = gs * ((picked ? 1.0f : 0.0f) - p);
    return use_tanh ? dz * (tanh_c - z * z / tanh_c) : dz;
}

// LSTM cell backward for one unit: pre-activation gates (gi,gf,gg,go), c_prev, c; dh, dc (in: gradient wrt h_t, c_t incl. the
// recurrent parts; out: dc = gradient wrt c_{t-1}); returns the four pre-activation gate gradients
__device__ __forceinline__ void cell_backward(float gi, float gf, float gg, float go, float c_prev, float c, float dh, float& dc,
                                              float (&dg)[4]) {
    const float i = sigm(gi), f = sigm(gf), g = tanhf(gg), o = sigm(go), tc = tanhf(c);
    const float dct = dc + dh * o * (1.0f - tc * tc);
    dg[0] = dct * g * i * (1.0f - i);
    dg[1] = dct * c_prev * f * (1.0f - f);
    dg[2] = dct * i * (1.0f - g * g);
    dg[3] = dh * tc * o * (1.0f - o);
    dc = dct * f;
}

// One reverse step of an LSTM for the whole workgroup (thread j < H = unit j; every thread calls it): the cell backward of saved
// row `row` (of gates_pre [rows,4H], c_all [rows,H]) from dh, dc (dc updated) and c_prev, the cell state the row started from,
// with the gate gradients stored to dgates and to LDS dgs [4H]; then the transposed products: dx[row] = W_ih^T . dg (skipped
// without wih) and the return value W_hh^T . dg = the recurrent part of dh of the row before.
// decode_train_backward_kernel (train.hip) keeps these statements written out: through this function its H = 256 build takes 66
// VGPRs instead of 62 and loses a wave per SIMD.
template <int H>
__device__ __forceinline__ float cell_backward_step(const float* gates_pre, const float* c_all, int64_t row, float c_prev, float dh,
                                                    float& dc, float* dgs, float* dgates, const float* wih, float* dx,
                                                    const float* whh, int j) {
    const bool owner = j < H;
    if (owner) {
        const int64_t base = row * (4 * H);
        float dg[4];
        cell_backward(gates_pre[base + j], gates_pre[base + H + j], gates_pre[base + 2 * H + j], gates_pre[base + 3 * H + j], c_prev,
                      c_all[row * H + j], dh, dc, dg);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            dgs[g * H + j] = dg[g];
            dgates[base + g * H + j] = dg[g];
        }
    }
    __syncthreads();
    if (owner) {
        if (wih) dx[row * H + j] = matvec_cols<H>(wih, dgs, j);
        dh = matvec_cols<H>(whh, dgs, j);
    }
    __syncthreads();
    return dh;
}
}  // namespace
