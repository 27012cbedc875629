// qcart_actor.hip — batched DQN actor: the reference's direct_DQN action selection
// for B envs per launch, fused fc1 -> fc2 -> fc31 -> fc41 -> argmax -> epsilon-greedy.
//
// Reference: inverted harmonic oscillator/RL.py:80-111 (direct_DQN), layers.py:7-79 (FactorizedNoisy),
// layers.py:97-103 (Linear_weight_normalize), main_parallel.py:208-219 (epsilon-greedy in the actor) and
// :414-440 (the inference process: argmax of the action values).
//
// The network itself (workgroup shape, fragment GEMMs, the noisy-layer scheme, the noise layout) is
// qcart_dqn.hpp's; this file holds the actor's epilogues, the measurement network's convolutions and the handles.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/qcart.h"
#include "qcart_dqn.hpp"
#include "qcart_host.hpp"
#include "qcart_learner.hpp"

namespace qcart {
namespace actor {

using namespace qcart::dqn;

struct Layer {
    const float* u;      // fragments of the (effective) weight
    const float* s;      // fragments of sigma_w (noisy) or null
    const float* ub;     // bias, padded to tiles*32
    const float* sb;     // sigma_b, padded, or null
};

struct ActArgs {
    Layer L[4];
    int in_len, in_pad, n_act;
    int64_t B, env_offset;
    const float* obs;
    int noisy;
    const float* noise;   // [noise_len][B] feature-major (internal layout)
    int64_t noise_ld;     // leading dimension of the noise buffer (>= B)
    float eps;
    uint64_t seed, counter;
    int32_t* actions;
    float* q_out;
    int32_t* random_out;
    // measurement network (DQN_measurement): the 256-wide fc1 output, feature-major [256][h_ld], enters
    // as H2; fc1 / fc2 of direct_DQN are skipped and L[2] / L[3] hold fc21 / fc31
    const float* h_in;
    int64_t h_ld;
};

__device__ __forceinline__ float noise_at(const ActArgs& a, int f, int64_t e) {
    return a.noise[(int64_t)f * a.noise_ld + e];
}

// W2: fc2's width (qcart_dqn.hpp). The measurement network's tail (h_in) exists at W2 = 256 only
// W2C = W2 + kChunkTag: in_pad > kChunkIn (the 'wavefunction' input), fc1 over X0 in chunks (dense4_chunked); the rest
// is the same
template <int W2C>
__global__ __launch_bounds__(kThreads) void k_actor_act(const ActArgs a) {
    constexpr int W2 = W2C & ~kChunkTag;
    constexpr bool CHUNK = (W2C & kChunkTag) != 0;
    constexpr int kEpsIn31 = NoiseAt<W2>::kEpsIn31, kEpsOut31 = NoiseAt<W2>::kEpsOut31,
                  kEpsIn41 = NoiseAt<W2>::kEpsIn41, kEpsOut41 = NoiseAt<W2>::kEpsOut41;
    constexpr bool kWide = W2 != kH2;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* RA = lds;                      // H1 [512][32]; later H3 [256][32] + H3e [256][32]
    float* RB = lds + kH1 * kE;           // X0 [in_pad][32]; later H2 [256][32] + H2e [256][32], or H2 [512][32]
    float* RC = lds + 2 * kH1 * kE;       // fc41 sigma partial
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t e0 = (int64_t)blockIdx.x * kE;
    const int env = lane & 31;
    const int64_t eg = e0 + env;          // this lane's env (D column)
    const bool env_ok = eg < a.B;

    float* H2 = RB;
    float* H2e = kWide ? RA : RB + kH2 * kE;   // wide: over H1, once fc2 is complete
    const bool n31 = a.noisy && a.L[2].s != nullptr;
    if (!kWide && a.h_in) {
        // DQN_measurement: relu(fc1(x)) from HBM (coalesced 32-env rows) -> H2, eps_in(fc21) o H2
        for (int i = tid; i < kH2 * kE; i += kThreads) {
            const int k = i / kE, e = i % kE;
            const bool ok = e0 + e < a.B;
            const float h = ok ? a.h_in[(int64_t)k * a.h_ld + e0 + e] : 0.f;
            H2[i] = h;
            if (n31) H2e[i] = ok ? h * noise_at(a, kEpsIn31 + k, e0 + e) : 0.f;
        }
        __syncthreads();
    } else {
        if constexpr (CHUNK) {
            // ---- input and fc1 (ReLU), X0 through RB one chunk of rows at a time
            dense4_chunked(
                a.L[0].u, RB, a.in_pad, tid,
                [&](int k, int e) { return (k < a.in_len && e0 + e < a.B) ? a.obs[(e0 + e) * a.in_len + k] : 0.f; },
                [&](int o, float y) { RA[o * kE + env] = fmaxf(y + a.L[0].ub[o], 0.f); });
        } else {
        // ---- input: the fp32 network input (IHO/main_parallel.py:131,241) -> X0[k][env]
        for (int i = tid; i < a.in_pad * kE; i += kThreads) {
            const int k = i / kE, e = i % kE;
            RB[i] = (k < a.in_len && e0 + e < a.B) ? a.obs[(e0 + e) * a.in_len + k] : 0.f;
        }
        __syncthreads();
        // ---- fc1: ReLU
        dense4(a.L[0].u, nullptr, RB, nullptr, kH1, a.in_pad, lane, wave, [&](int o, float y, float) {
            RA[o * kE + env] = fmaxf(y + a.L[0].ub[o], 0.f);
        });
        }
        __syncthreads();
        // ---- fc2: ReLU; also eps_in(fc31) o H2 for the noisy GEMM
        dense4(a.L[1].u, nullptr, RA, nullptr, W2, kH1, lane, wave, [&](int o, float y, float) {
            const float h = fmaxf(y + a.L[1].ub[o], 0.f);
            H2[o * kE + env] = h;
            if (!kWide && n31) H2e[o * kE + env] = env_ok ? h * noise_at(a, kEpsIn31 + o, eg) : 0.f;
        });
        __syncthreads();
        if (kWide && n31) {
            for (int i = tid; i < W2 * kE; i += kThreads) {
                const int k = i / kE, e = i % kE;
                H2e[i] = e0 + e < a.B ? H2[i] * noise_at(a, kEpsIn31 + k, e0 + e) : 0.f;
            }
            __syncthreads();
        }
    }

    // ---- fc31 (noisy or weight-normalised): ReLU; eps_in(fc41) o H3
    float* H3 = RA;
    float* H3e = RA + kH3 * kE;
    const bool n41 = a.noisy && a.L[3].s != nullptr;
    auto act31 = [&](int o, float yu, float ys) {
        float y = yu + a.L[2].ub[o];
        if (n31) y += env_ok ? noise_at(a, kEpsOut31 + o, eg) * (ys + a.L[2].sb[o]) : 0.f;
        return fmaxf(y, 0.f);
    };
    auto put3 = [&](int o, float h) {
        H3[o * kE + env] = h;
        if (n41) H3e[o * kE + env] = env_ok ? h * noise_at(a, kEpsIn41 + o, eg) : 0.f;
    };
    if constexpr (kWide) {
        float hold[2][16];
        dense4_hold2(a.L[2].u, n31 ? a.L[2].s : nullptr, H2, H2e, W2, lane, wave, hold, act31);
        __syncthreads();   // every wave is done reading H2 / H2e: RA is free
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) put3((wave + 4 * j) * 32 + drow(r, lane), hold[j][r]);
    } else {
        dense4(a.L[2].u, n31 ? a.L[2].s : nullptr, H2, H2e, kH3, W2, lane, wave,
               [&](int o, float yu, float ys) { put3(o, act31(o, yu, ys)); });
    }
    __syncthreads();

    // ---- fc41 -> action values, argmax (lowest index among equal maxima)
    float best = -INFINITY;
    int besti = 0x7fffffff;
    const bool w0 = fc41(a.L[3].u, n41 ? a.L[3].s : nullptr, H3, H3e, RC, a.n_act, lane, wave,
                         [&](int o, float yu, float ys) {
                             float q = yu + a.L[3].ub[o];
                             if (n41) q += env_ok ? noise_at(a, kEpsOut41 + o, eg) * (ys + a.L[3].sb[o]) : 0.f;
                             if (a.q_out && env_ok) a.q_out[eg * a.n_act + o] = q;
                             if (q > best || (q == best && o < besti)) {
                                 best = q;
                                 besti = o;
                             }
                         },
                         [] {});
    if (!w0) return;
    // ---- epsilon-greedy
    const float ob = __shfl_xor(best, 32, 64);
    const int oi = __shfl_xor(besti, 32, 64);
    if (ob > best || (ob == best && oi < besti)) besti = oi;
    if (lane < 32 && env_ok) {
        int act = besti;
        int rnd = 0;
        if (a.eps > 0.f) {
            uint32_t c[4] = {(uint32_t)a.counter, (uint32_t)(a.counter >> 32), (uint32_t)(a.env_offset + eg), 0x200u};
            philox10(c, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
            const float u1 = (float)(c[0] >> 8) * 0x1.0p-24f, u2 = (float)(c[1] >> 8) * 0x1.0p-24f;
            if (u1 < a.eps) {   // random.random() < eps_threshold -> random.randrange(21)
                act = min((int)(u2 * (float)a.n_act), a.n_act - 1);
                rnd = 1;
            }
        }
        a.actions[eg] = act;
        if (a.random_out) a.random_out[eg] = rnd;
    }
}

// NoisyNet noise, feature-major [noise_len][ld]: f(z) = sign(z) sqrt|z| (layers.py:77-79) of Philox
// normals keyed by (seed, env_offset + e), counter, tag 0x100 + pair
__global__ __launch_bounds__(256) void k_actor_noise(float* out, int64_t ld, int64_t B, int noise_len,
                                                     int64_t env_offset, uint64_t seed, uint64_t counter) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int p = blockIdx.y;
    if (e >= B) return;
    const float2 f = noise_pair(seed, counter, (uint32_t)(env_offset + e), p);
    out[(int64_t)(2 * p) * ld + e] = f.x;
    if (2 * p + 1 < noise_len) out[(int64_t)(2 * p + 1) * ld + e] = f.y;
}

// injected noise [B][noise_len] -> feature-major [noise_len][ld]
__global__ __launch_bounds__(256) void k_actor_transpose(const float* in, float* out, int64_t ld, int64_t B,
                                                         int noise_len) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * noise_len) return;
    const int64_t e = i / noise_len;
    const int f = (int)(i % noise_len);
    out[(int64_t)f * ld + e] = in[i];
}

// effective weight (W g / ||W||_F, or W) -> fragments [tile][step][64]; bias padded to tiles*32
// split = 0: MFMA k-step s pairs k = 2s, 2s + 1 (lane halves); split = 1: k = s, s + Kpad / 2 (the
// convolutions: the upper half of K is then a fixed input offset, see k_mconv)
__global__ __launch_bounds__(1024) void k_actor_prep(const float* W, const float* g, int O, int K, int Kpad,
                                                     float* frag, const float* bias, float* bias_pad, int split) {
    __shared__ double part[1024];
    double ss = 0.0;
    if (g) {
        for (int i = threadIdx.x; i < O * K; i += 1024) ss += (double)W[i] * (double)W[i];
    }
    ss = block_sum(ss, part);
    const float sc = g ? wn_scale(g[0], ss) : 1.f;
    const int T = tiles(O), S = ksteps(Kpad);
    for (int i = threadIdx.x; i < T * S * 64; i += 1024) {
        int o, k;
        frag_ok(i, S, split, o, k);
        frag[i] = (o < O && k < K) ? W[(size_t)o * K + k] * sc : 0.f;
    }
    if (bias_pad)
        for (int i = threadIdx.x; i < T * 32; i += 1024) bias_pad[i] = (i < O && bias) ? bias[i] : 0.f;
}

// ---- DQN_measurement (IHO/RL.py:29-78): Conv1d stack as implicit GEMMs on f32 MFMA ----------------
// Y[b][co][t] = relu(bias[co] + sum_{ci, j} W[co][ci][j] X[b][ci][S t + j]): M = co (MT tiles of 32),
// N = (env, position) flattened (32 columns per wave), K = ci * KS in pairs (k = ci * KS + j, the
// PyTorch weight order). A = weight fragments (k_actor_prep order), B = the input gathered per lane
// from HBM / L2 (column base X[b] + S t; row offset ci * Tin + j, wave-uniform per k-step half).
// Loads run one batch of kQ k-steps ahead of the MFMAs (two register sets, no copies); every load is
// unconditional (columns past the end read the workgroup's first env, whose results are not stored).
// Output: env-major [b][co][t] (32 consecutive t per store: one 128-B run); conv3's is transposed
// afterwards by k_mtr into fc1's feature-major operand (written directly, every lane's store hit its own
// cache line: 4.6 M partial-line writes per chunk). NT column tiles per wave: every weight fragment
// feeds NT MFMAs, every input value MT. (A polyphase activation layout that turns the stride-S gathers into
// contiguous runs was measured: conv2/conv3 unchanged, conv1's scattered stores +23 %; not kept.)
constexpr int kNTs[3] = {QCART_MCONV_NT};   // (knob defaults: qcart_expt.hpp)
constexpr int kNT1 = kNTs[0], kNT2 = kNTs[1], kNT3 = kNTs[2];
constexpr int kNAs[3] = {QCART_MCONV_NA};
constexpr int kNA1 = kNAs[0], kNA2 = kNAs[1], kNA3 = kNAs[2];
constexpr int kQs[3] = {QCART_MCONV_Q};   // k-steps per load batch
constexpr int kQ1 = kQs[0], kQ2 = kQs[1], kQ3 = kQs[2];
template <int CI, int KS, int S, int MT, int NT, int NA, int kQ>
__global__ __launch_bounds__(256) void k_mconv(const float* __restrict__ X, int Tin, const float* __restrict__ Wf,
                                               const float* __restrict__ bias, float* __restrict__ Y, int Tout,
                                               int64_t n_total) {
    constexpr int K = CI * KS, STEPS = K / 2;
    static_assert(CI % 2 == 0, "split-K pairing: k and k + K/2 are channels ci and ci + CI/2");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hi = lane >> 5;
    // buffer descriptor at the workgroup's first env: every lane offset is a small 32-bit VGPR, the
    // k-step's row offset is wave-uniform (SGPR), so a load costs no VALU
    const int64_t b0 = (int64_t)blockIdx.x * 128 * NT / Tout;
    const rsrc_t rx = make_rsrc(X + b0 * CI * Tin, 0xFFFFFFFFu);
    const rsrc_t rw = make_rsrc(Wf, 0xFFFFFFFFu);
    bool col_ok[NT];
    int64_t bb[NT];
    int tt[NT];
    int vx[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        const int64_t n = (((int64_t)blockIdx.x * 4 + wave) * NT + c) * 32 + (lane & 31);
        col_ok[c] = n < n_total;
        bb[c] = col_ok[c] ? n / Tout : b0;
        tt[c] = col_ok[c] ? (int)(n - bb[c] * Tout) : 0;
        vx[c] = (int)(((bb[c] - b0) * CI * Tin + S * tt[c] + hi * (CI / 2) * Tin) * 4);
    }
    const int vw = lane * 4;
    // NA accumulator sets for alternating k-steps: NA * MT * NT independent MFMA chains (an MFMA that
    // accumulates onto the previous one's result waits for it)
    f32x16 acc[NA][MT][NT];
#pragma unroll
    for (int q = 0; q < NA; ++q)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int c = 0; c < NT; ++c) acc[q][m][c] = f32x16{};
    // k-step s pairs k = s (lanes 0-31) and k = s + K/2 (lanes 32-63); clamped into range (a prefetch
    // past the end reloads the last step, unused)
    auto fetch = [&](int s, float (&x)[kQ][NT], float (&w)[kQ][MT]) {
#pragma unroll
        for (int u = 0; u < kQ; ++u) {
            const int sc = min(s + u, STEPS - 1);
            const int so = ((sc / KS) * Tin + sc % KS) * 4;   // ci * Tin + j
#pragma unroll
            for (int c = 0; c < NT; ++c) x[u][c] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, vx[c], so, 0));
#pragma unroll
            for (int m = 0; m < MT; ++m)
                w[u][m] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rw, vw, (m * STEPS + sc) * 256, 0));
        }
    };
    auto mma = [&](int n, const float (&x)[kQ][NT], const float (&w)[kQ][MT]) {
#pragma unroll
        for (int u = 0; u < kQ; ++u)
            if (u < n)
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int c = 0; c < NT; ++c)
                        acc[u % NA][m][c] =
                            __builtin_amdgcn_mfma_f32_32x32x2f32(w[u][m], x[u][c], acc[u % NA][m][c], 0, 0, 0);
    };
    float xa[kQ][NT], wa[kQ][MT], xb[kQ][NT], wb[kQ][MT];
    fetch(0, xa, wa);
    int s = 0;
    // the next batch's loads interleaved one by one with this batch's MFMAs (sched_group_barrier:
    // VMEM read 0x020, MFMA 0x008), so the load issue never holds the MFMA stream back
    constexpr int NLD = kQ * (NT + MT), NMF = kQ * MT * NT;
    auto interleave = [&]() {
#pragma unroll
        for (int i = 0; i < (NLD > NMF ? NLD : NMF); ++i) {
            if (i < NLD) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
            if (i < NMF) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        }
    };
    for (; s + 2 * kQ <= STEPS; s += 2 * kQ) {
        fetch(s + kQ, xb, wb);
        mma(kQ, xa, wa);
        interleave();
        __builtin_amdgcn_sched_barrier(0);
        fetch(s + 2 * kQ, xa, wa);
        mma(kQ, xb, wb);
        interleave();
        __builtin_amdgcn_sched_barrier(0);
    }
    if (s + kQ <= STEPS) {   // one full batch (in xa) and a partial one
        fetch(s + kQ, xb, wb);
        mma(kQ, xa, wa);
        mma(STEPS - s - kQ, xb, wb);
    } else {
        mma(STEPS - s, xa, wa);
    }
#pragma unroll
    for (int q = 1; q < NA; ++q)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int c = 0; c < NT; ++c) acc[0][m][c] += acc[q][m][c];
    float bv[MT][16];   // bias of this lane's output rows, loaded as one batch before the stores
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) bv[m][r] = bias[m * 32 + drow(r, lane)];
    // stores through a descriptor at the workgroup's first env: per-lane offset (env, position, the lane
    // half's 4-row shift) in a VGPR, the output row's (m 32 + (r & 3) + 8 (r >> 2)) Tout wave-uniform
    const rsrc_t ry = make_rsrc(Y + b0 * (MT * 32) * Tout, 0xFFFFFFFFu);
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        if (!col_ok[c]) continue;
        const int vy = (int)((((bb[c] - b0) * (MT * 32) + 4 * hi) * Tout + tt[c]) * 4);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m * 32 + (r & 3) + 8 * (r >> 2);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(fmaxf(acc[0][m][c][r] + bv[m][r], 0.f)), ry, vy,
                                                      row * Tout * 4, 0);
            }
    }
}

// conv3's env-major chunk output [nb][F] -> fc1's feature-major operand [F][ld] at env column c0: 64x64
// tiles through LDS, coalesced on both sides
__global__ __launch_bounds__(256) void k_mtr(const float* __restrict__ in, float* __restrict__ out, int F,
                                             int64_t nb, int64_t ld, int64_t c0) {
    __shared__ float t[64][65];
    const int64_t b0 = (int64_t)blockIdx.y * 64;
    const int f0 = blockIdx.x * 64, tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int64_t b = b0 + r;
        t[r][tx] = (b < nb && f0 + tx < F) ? in[b * F + f0 + tx] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int f = f0 + r;
        if (f < F && b0 + tx < nb) out[(int64_t)f * ld + c0 + b0 + tx] = t[tx][r];
    }
}

// fc1 (nn.Linear K -> 256) + ReLU: B = the feature-major conv output X[k][x_ld] (one coalesced 128-B row
// per k-step half and column tile). A wave computes MT of the 8 output tiles for NT * 32 envs; the 8 / MT
// waves that share an env group sit in one workgroup (their B reads coincide in L1 / L2). Weight
// traffic per env is 8 / (MT * NT) tile streams of K: (MT, NT) = (8, 1) streams the 4.6 MB weight
// matrix once per 32 envs — more than one XCD's L2, so from MALL. Buffer loads with wave-uniform
// k-step offsets, batches of kQF k-steps loaded one batch ahead of the MFMAs.
constexpr int kMfcMT = QCART_MFC_MT, kMfcNT = QCART_MFC_NT, kQF = 4;
template <int MT, int NT>
__global__ __launch_bounds__(256) void k_mfc(const float* __restrict__ X, int64_t x_ld, int K,
                                             const float* __restrict__ Wf, const float* __restrict__ bias,
                                             float* __restrict__ H, int64_t B) {
    constexpr int MP = 8 / MT;   // waves per env group
    static_assert(4 % MP == 0, "the waves of an env group share a workgroup");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform: descriptors stay in SGPRs
    const int mp = wave % MP;
    const int64_t e0 = ((int64_t)blockIdx.x * (4 / MP) + wave / MP) * NT * 32;
    const int steps = K / 2, hi = lane >> 5;   // K = 64 T3 is even
    const rsrc_t rx = make_rsrc(X + e0, 0xFFFFFFFFu);
    const rsrc_t rw = make_rsrc(Wf + (size_t)mp * MT * steps * 64, 0xFFFFFFFFu);
    bool ok[NT];
    int vx[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        const int64_t e = e0 + c * 32 + (lane & 31);
        ok[c] = e < B;
        vx[c] = (int)(((ok[c] ? c * 32 + (lane & 31) : 0) + (int64_t)hi * x_ld) * 4);   // row k = 2 s + hi
    }
    const int vw = lane * 4;
    f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int c = 0; c < NT; ++c) acc[m][c] = f32x16{};
    auto fetch = [&](int s, float (&x)[kQF][NT], float (&w)[kQF][MT]) {
#pragma unroll
        for (int u = 0; u < kQF; ++u) {
            const int sc = min(s + u, steps - 1);
            const int xo = (int)((uint32_t)(2 * sc) * (uint32_t)x_ld * 4u);   // < 4 GiB: checked at create
#pragma unroll
            for (int c = 0; c < NT; ++c) x[u][c] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, vx[c], xo, 0));
#pragma unroll
            for (int m = 0; m < MT; ++m)
                w[u][m] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rw, vw, (m * steps + sc) * 256, 0));
        }
    };
    auto mma = [&](const float (&x)[kQF][NT], const float (&w)[kQF][MT]) {
#pragma unroll
        for (int u = 0; u < kQF; ++u)
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int c = 0; c < NT; ++c)
                    acc[m][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[u][m], x[u][c], acc[m][c], 0, 0, 0);
    };
    float xa[kQF][NT], wa[kQF][MT], xb[kQF][NT], wb[kQF][MT];
    // runtime K (= 64 T3 >= 64, so at least one double batch): whole double batches, then single steps
    const int full = steps / (2 * kQF) * (2 * kQF);
    int s = 0;
    fetch(0, xa, wa);
    do {
        fetch(s + kQF, xb, wb);
        __builtin_amdgcn_sched_barrier(0);
        mma(xa, wa);
        __builtin_amdgcn_sched_barrier(0);
        fetch(s + 2 * kQF, xa, wa);   // past the end: clamped re-reads, unused
        __builtin_amdgcn_sched_barrier(0);
        mma(xb, wb);
        __builtin_amdgcn_sched_barrier(0);
        s += 2 * kQF;
    } while (s < full);
    for (; s < steps; ++s) {
        float x1[NT], w1[MT];
#pragma unroll
        for (int c = 0; c < NT; ++c)
            x1[c] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, vx[c], (int)((uint32_t)(2 * s) * (uint32_t)x_ld * 4u), 0));
#pragma unroll
        for (int m = 0; m < MT; ++m) w1[m] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rw, vw, (m * steps + s) * 256, 0));
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int c = 0; c < NT; ++c) acc[m][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[m], x1[c], acc[m][c], 0, 0, 0);
    }
    float bv[MT][16];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) bv[m][r] = bias[(mp * MT + m) * 32 + drow(r, lane)];
    // feature-major [256][ld] through a descriptor at (row 0, env e0): per-lane offset (column, the
    // lane half's 4-row shift) in a VGPR, the row's offset ((mp MT + m) 32 + (r & 3) + 8 (r >> 2)) x_ld
    // wave-uniform (SGPR)
    const rsrc_t rh = make_rsrc(H + e0, 0xFFFFFFFFu);
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        if (!ok[c]) continue;
        const int vh = (int)((c * 32 + (lane & 31) + (int64_t)4 * hi * x_ld) * 4);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t row = (uint32_t)((mp * MT + m) * 32 + (r & 3) + 8 * (r >> 2));
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(fmaxf(acc[m][c][r] + bv[m][r], 0.f)), rh, vh,
                                                      (int)(row * (uint32_t)x_ld * 4u), 0);
            }
    }
}

}  // namespace actor
}  // namespace qcart

using namespace qcart::actor;
using namespace qcart::host;

// what both actor handles hold, and act_tail works on
struct ActorCore {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    bool loaded = false;
    int n_act = 0, noise_len = 0;
    int w2 = kH2;                // fc2's width (k_actor_act's instantiation); the measurement actor's tail: 256
    bool chunked = false;        // data_length above kChunkIn: k_actor_act<w2 + kChunkTag>
    int64_t max_batch = 0;       // also the noise buffer's leading dimension
    uint64_t seed = 0;
    float* d_w = nullptr;        // all fragments + padded biases
    size_t w_floats = 0;         // its length
    float* d_noise = nullptr;    // [noise_len][max_batch]
    Layer L[4]{};                // k_actor_act's layers (s / sb null where loaded without sigma)
};

struct qc_actor : ActorCore {
    qc_dqn_params p{};
    int in_pad = 0;
    size_t off_u[4]{}, off_s[4]{}, off_ub[4]{}, off_sb[4]{};
};

namespace {
CreateError g_actor_err, g_mactor_err;

constexpr LayerRule kActorRules[] = {
    {0b0011, states_where([](bool wn, bool sw, bool) { return !wn || sw; }),
     "fc1 / fc2 are Linear_weight_normalize layers (weight_norm required, no sigma)"},
    {0b1111, kSigmaApart, kSigmaApartText},
    {0b1111, states_where([](bool wn, bool sw, bool) { return sw && wn; }), "a noisy layer has no weight_norm"},
    {0b1111, states_where([](bool wn, bool sw, bool) { return !sw && !wn; }), "a deterministic layer needs weight_norm"},
};
constexpr LayerRule kMactorRules[] = {
    {0b000111, states_where([](bool, bool sw, bool) { return sw; }),
     "conv1..3 are Conv1d or Conv1d_weight_normalize layers (no sigma)"},
    {0b001000, states_where([](bool wn, bool sw, bool) { return sw || wn; }),
     "fc1 is a plain Linear layer (no weight_norm, no sigma)"},
    {0b111111, kSigmaApart, kSigmaApartText},
    {0b110000, states_where([](bool wn, bool sw, bool) { return !sw && !wn; }),
     "fc21 / fc31: FactorizedNoisy or Linear_weight_normalize"},
};

using ActKernel = void (*)(const ActArgs);
ActKernel act_kernel(int w2, bool chunked) {
    if (chunked) return w2 == kH2Wide ? k_actor_act<kH2Wide + kChunkTag> : k_actor_act<kH2 + kChunkTag>;
    return w2 == kH2Wide ? k_actor_act<kH2Wide> : k_actor_act<kH2>;
}

bool enable_act_lds(int w2, bool chunked = false) {
    return hipFuncSetAttribute((const void*)act_kernel(w2, chunked), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)kActLdsBytes) == hipSuccess;
}

// the end of an act call: the noise (injected and transposed, or drawn), then k_actor_act; k holds the input side
int act_tail(ActorCore* a, ActArgs& k, const char* what, int64_t B, int64_t env_offset, int32_t noisy,
             const float* noise, double eps, uint64_t counter, int32_t* actions, float* q_out, int32_t* random_out) {
    const int64_t ld = a->max_batch;
    const bool need_noise = noisy && (a->L[2].s || a->L[3].s);
    if (need_noise) {
        if (noise) {
            const int64_t n = B * a->noise_len;
            hipLaunchKernelGGL(k_actor_transpose, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, a->stream, noise,
                               a->d_noise, ld, B, a->noise_len);
        } else {
            hipLaunchKernelGGL(k_actor_noise, dim3((unsigned)((B + 255) / 256), (unsigned)((a->noise_len + 1) / 2)),
                               dim3(256), 0, a->stream, a->d_noise, ld, B, a->noise_len, env_offset, a->seed, counter);
        }
    }
    for (int l = 0; l < 4; ++l) k.L[l] = a->L[l];
    k.n_act = a->n_act;
    k.B = B;
    k.env_offset = env_offset;
    k.noisy = need_noise ? 1 : 0;
    k.noise = a->d_noise;
    k.noise_ld = ld;
    k.eps = (float)eps;
    k.seed = a->seed;
    k.counter = counter;
    k.actions = actions;
    k.q_out = q_out;
    k.random_out = random_out;
    const dim3 grid((unsigned)((B + kE - 1) / kE));
    hipLaunchKernelGGL(act_kernel(a->w2, a->chunked), grid, dim3(kThreads), kActLdsBytes, a->stream, k);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(a->err, e, what);
    return QC_OK;
}
}  // namespace

extern "C" {

int qc_actor_create(const qc_dqn_params* p, int device, qc_actor** out) {
    if (!out || !p) return QC_EINVAL;
    *out = nullptr;
    if (const char* m = bad_net_size(p->data_length, p->n_actions)) return g_actor_err.fail(m, QC_EINVAL);
    if (p->max_batch < 1) return g_actor_err.fail("max_batch must be >= 1", QC_EINVAL);
    const int w2 = fc2_width(p->hidden2);
    if (!w2) return g_actor_err.fail("hidden2 must be 0, 256 or 512 (fc2's width)", QC_EINVAL);
    if (const int rc = check_device(device, g_actor_err, "the actor")) return rc;
    qc_actor* a = new qc_actor();
    a->p = *p;
    a->device = device;
    a->n_act = p->n_actions;
    a->max_batch = p->max_batch;
    a->seed = p->seed;
    a->in_pad = in_pad(p->data_length);
    a->w2 = w2;
    a->chunked = a->in_pad > kChunkIn;
    a->noise_len = noise_len(w2, p->n_actions);
    const int K[4] = {a->in_pad, kH1, w2, kH3};
    const int O[4] = {kH1, w2, kH3, p->n_actions};
    // fc31 / fc41 may be loaded either way; fc1 / fc2 never use their sigma regions, but without them fc2's
    // fragments start off a 4 KiB boundary and k_actor_act measures 1.3 % slower (65 536 envs)
    const bool noisy[4] = {true, true, true, true};
    const size_t floats = frag_layout(4, O, K, noisy, a->off_u, a->off_s, a->off_ub, a->off_sb);
    Dev g(device);
    a->w_floats = floats;
    hipError_t e = hipMalloc(&a->d_w, floats * sizeof(float));
    if (e == hipSuccess) e = hipMemset(a->d_w, 0, floats * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&a->d_noise, (size_t)a->noise_len * (size_t)p->max_batch * sizeof(float));
    const bool lds_ok = e == hipSuccess && enable_act_lds(w2, a->chunked);
    if (!lds_ok) {
        if (a->d_w) (void)hipFree(a->d_w);
        if (a->d_noise) (void)hipFree(a->d_noise);
        delete a;
        return e != hipSuccess ? g_actor_err.fail("device allocation failed", QC_ENOMEM)
                               : g_actor_err.fail("cannot enable 140 KiB of LDS for the actor kernel", QC_EHIP);
    }
    *out = a;
    return QC_OK;
}

void qc_actor_destroy(qc_actor* a) {
    if (!a) return;
    {
        Dev g(a->device);
        (void)hipDeviceSynchronize();
        if (a->d_w) (void)hipFree(a->d_w);
        if (a->d_noise) (void)hipFree(a->d_noise);
    }
    delete a;
}

const char* qc_actor_last_error(const qc_actor* a) { return a ? a->err.c_str() : g_actor_err.text(); }

int qc_actor_set_stream(qc_actor* a, void* stream) {
    if (!a) return QC_EINVAL;
    a->stream = (hipStream_t)stream;
    return QC_OK;
}

int qc_actor_noise_len(const qc_actor* a) { return a ? a->noise_len : QC_EINVAL; }

int qc_actor_load(qc_actor* a, const qc_dqn_layer layers[4]) {
    if (!a || !layers) return QC_EINVAL;
    if (const int rc = validate_layers(layers, 4, kActorRules, 4, a->err)) return rc;
    const int K[4] = {a->p.data_length, kH1, a->w2, kH3};
    const int Kp[4] = {a->in_pad, kH1, a->w2, kH3};
    const int O[4] = {kH1, a->w2, kH3, a->p.n_actions};
    Dev g(a->device);
    float* w = a->d_w;
    for (int l = 0; l < 4; ++l) {
        const qc_dqn_layer& L = layers[l];
        hipLaunchKernelGGL(k_actor_prep, dim3(1), dim3(1024), 0, a->stream, L.weight, L.weight_norm, O[l], K[l], Kp[l],
                           w + a->off_u[l], L.bias, w + a->off_ub[l], 0);
        if (L.sigma_w)
            hipLaunchKernelGGL(k_actor_prep, dim3(1), dim3(1024), 0, a->stream, L.sigma_w, (const float*)nullptr, O[l],
                               K[l], Kp[l], w + a->off_s[l], L.sigma_b, w + a->off_sb[l], 0);
        a->L[l] = Layer{w + a->off_u[l], L.sigma_w ? w + a->off_s[l] : nullptr, w + a->off_ub[l],
                        L.sigma_w ? w + a->off_sb[l] : nullptr};
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(a->err, e, "actor weight preparation");
    a->loaded = true;
    return QC_OK;
}

int qc_actor_act(qc_actor* a, int64_t B, int64_t env_offset, const float* obs, int32_t noisy, const float* noise,
                 double eps, uint64_t counter, int32_t* actions, float* q_out, int32_t* random_out) {
    if (!a) return QC_EINVAL;
    if (!a->loaded) { a->err = "qc_actor_load has not been called"; return QC_EINVAL; }
    if (B < 0 || B > a->p.max_batch) { a->err = "B must be in [0, max_batch]"; return QC_EINVAL; }
    if (B == 0) return QC_OK;
    if (!obs || !actions) { a->err = "obs and actions are required"; return QC_EINVAL; }
    Dev g(a->device);
    ActArgs k{};
    k.in_len = a->p.data_length;
    k.in_pad = a->in_pad;
    k.obs = obs;
    return act_tail(a, k, "actor launch", B, env_offset, noisy, noise, eps, counter, actions, q_out, random_out);
}

}  // extern "C"

// ---- the measurement-input actor (DQN_measurement, IHO/RL.py:29-78) --------------------------------
struct qc_mactor : ActorCore {
    qc_mdqn_params p{};
    int T1 = 0, T2 = 0, T3 = 0, flat = 0, chunk = 0;
    size_t off_w[6]{}, off_b[6]{}, off_s[6]{}, off_sb[6]{};
    float *d_y1 = nullptr, *d_y2 = nullptr, *d_y3e = nullptr, *d_y3 = nullptr, *d_h1 = nullptr;
};

namespace {
// layer shapes: conv1 (32, 2, 13, /5), conv2 (64, 32, 11, /4), conv3 (64, 64, 9, /4) (RL.py:36-45)
constexpr int kC1 = 32, kC2 = 64, kC3 = 64;
int conv_out(int n, int k, int s) { return (n - (k - 1) + (s - 1)) / s; }   // calculate_next_layer_dim (RL.py:49-50)
}  // namespace

extern "C" {

int qc_mactor_create(const qc_mdqn_params* p, int device, qc_mactor** out) {
    if (!out || !p) return QC_EINVAL;
    *out = nullptr;
    if (const char* m = bad_net_size(-1, p->n_actions)) return g_mactor_err.fail(m, QC_EINVAL);
    if (p->max_batch < 1) return g_mactor_err.fail("max_batch must be >= 1", QC_EINVAL);
    const int T1 = conv_out(p->read_length, 13, 5), T2 = conv_out(T1, 11, 4), T3 = conv_out(T2, 9, 4);
    if (p->read_length < 1 || T3 < 1)
        return g_mactor_err.fail("read_length too short for the three convolutions", QC_EINVAL);
    if ((uint64_t)(kC3 * T3) * (uint64_t)p->max_batch * sizeof(float) >= (1ull << 32))   // 32-bit buffer offsets
        return g_mactor_err.fail("max_batch too large: fc1's operand [64 T3][max_batch] must stay below 4 GiB", QC_EINVAL);
    if (const int rc = check_device(device, g_mactor_err, "the actor")) return rc;
    qc_mactor* a = new qc_mactor();
    a->p = *p;
    a->device = device;
    a->n_act = p->n_actions;
    a->max_batch = p->max_batch;
    a->seed = p->seed;
    a->T1 = T1; a->T2 = T2; a->T3 = T3;
    a->flat = kC3 * T3;
    a->noise_len = noise_len(kH2, p->n_actions);
    a->chunk = (int)std::min<int64_t>(p->max_batch, p->chunk > 0 ? p->chunk : 2048);
    const int O[6] = {kC1, kC2, kC3, kH2, kH3, p->n_actions};
    const int K[6] = {2 * 13, kC1 * 11, kC2 * 9, a->flat, kH2, kH3};
    const bool noisy[6] = {false, false, false, false, true, true};
    const size_t floats = frag_layout(6, O, K, noisy, a->off_w, a->off_s, a->off_b, a->off_sb);
    Dev g(device);
    const size_t mb = (size_t)p->max_batch, ch = (size_t)a->chunk;
    a->w_floats = floats;
    hipError_t e = hipMalloc(&a->d_w, floats * sizeof(float));
    if (e == hipSuccess) e = hipMemset(a->d_w, 0, floats * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&a->d_y1, ch * kC1 * a->T1 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&a->d_y2, ch * kC2 * a->T2 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&a->d_y3e, (size_t)a->flat * ch * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&a->d_y3, (size_t)a->flat * mb * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&a->d_h1, (size_t)kH2 * mb * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&a->d_noise, (size_t)a->noise_len * mb * sizeof(float));
    if (e != hipSuccess || !enable_act_lds(kH2)) {
        qc_mactor_destroy(a);
        return g_mactor_err.fail("device allocation failed", QC_ENOMEM);
    }
    *out = a;
    return QC_OK;
}

void qc_mactor_destroy(qc_mactor* a) {
    if (!a) return;
    {
        Dev g(a->device);
        (void)hipDeviceSynchronize();
        for (float* q : {a->d_w, a->d_y1, a->d_y2, a->d_y3e, a->d_y3, a->d_h1, a->d_noise})
            if (q) (void)hipFree(q);
    }
    delete a;
}

const char* qc_mactor_last_error(const qc_mactor* a) { return a ? a->err.c_str() : g_mactor_err.text(); }

int qc_mactor_set_stream(qc_mactor* a, void* stream) {
    if (!a) return QC_EINVAL;
    a->stream = (hipStream_t)stream;
    return QC_OK;
}

int qc_mactor_noise_len(const qc_mactor* a) { return a ? a->noise_len : QC_EINVAL; }
int qc_mactor_flat_len(const qc_mactor* a) { return a ? a->flat : QC_EINVAL; }

int qc_mactor_load(qc_mactor* a, const qc_dqn_layer layers[6]) {
    if (!a || !layers) return QC_EINVAL;
    if (const int rc = validate_layers(layers, 6, kMactorRules, 4, a->err)) return rc;
    const int O[6] = {kC1, kC2, kC3, kH2, kH3, a->p.n_actions};
    const int K[6] = {2 * 13, kC1 * 11, kC2 * 9, a->flat, kH2, kH3};
    Dev g(a->device);
    float* w = a->d_w;
    for (int l = 0; l < 6; ++l) {
        const qc_dqn_layer& L = layers[l];
        const int Kp = in_pad(K[l]);
        const bool sigma = l >= 4 && L.sigma_w;
        hipLaunchKernelGGL(k_actor_prep, dim3(1), dim3(1024), 0, a->stream, L.weight, L.weight_norm, O[l], K[l], Kp,
                           w + a->off_w[l], L.bias, w + a->off_b[l], l < 3 ? 1 : 0);
        if (sigma)
            hipLaunchKernelGGL(k_actor_prep, dim3(1), dim3(1024), 0, a->stream, L.sigma_w, (const float*)nullptr, O[l],
                               K[l], Kp, w + a->off_s[l], L.sigma_b, w + a->off_sb[l], 0);
        if (l >= 4)   // fc21 / fc31 are k_actor_act's layers 2 / 3
            a->L[l - 2] = Layer{w + a->off_w[l], sigma ? w + a->off_s[l] : nullptr, w + a->off_b[l],
                                sigma ? w + a->off_sb[l] : nullptr};
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(a->err, e, "measurement actor weight preparation");
    a->loaded = true;
    return QC_OK;
}

int qc_mactor_act(qc_mactor* a, int64_t B, int64_t env_offset, const float* obs, int32_t noisy, const float* noise,
                  double eps, uint64_t counter, int32_t* actions, float* q_out, int32_t* random_out) {
    if (!a) return QC_EINVAL;
    if (!a->loaded) { a->err = "qc_mactor_load has not been called"; return QC_EINVAL; }
    if (B < 0 || B > a->p.max_batch) { a->err = "B must be in [0, max_batch]"; return QC_EINVAL; }
    if (B == 0) return QC_OK;
    if (!obs || !actions) { a->err = "obs and actions are required"; return QC_EINVAL; }
    Dev g(a->device);
    const int L = a->p.read_length;
    const float* w = a->d_w;
    const int64_t ld = a->p.max_batch;
    for (int64_t c0 = 0; c0 < B; c0 += a->chunk) {   // conv stack per env chunk (its activations stay in L2 / MALL)
        const int64_t nb = std::min<int64_t>(a->chunk, B - c0);
        const int64_t n1 = nb * a->T1, n2 = nb * a->T2, n3 = nb * a->T3;
        hipLaunchKernelGGL((k_mconv<2, 13, 5, 1, kNT1, kNA1, kQ1>), dim3((unsigned)((n1 + 128 * kNT1 - 1) / (128 * kNT1))),
                           dim3(256), 0, a->stream, obs + c0 * 2 * L, L, w + a->off_w[0], w + a->off_b[0], a->d_y1,
                           a->T1, n1);
        hipLaunchKernelGGL((k_mconv<32, 11, 4, 2, kNT2, kNA2, kQ2>), dim3((unsigned)((n2 + 128 * kNT2 - 1) / (128 * kNT2))),
                           dim3(256), 0, a->stream, a->d_y1, a->T1, w + a->off_w[1], w + a->off_b[1], a->d_y2, a->T2,
                           n2);
        hipLaunchKernelGGL((k_mconv<64, 9, 4, 2, kNT3, kNA3, kQ3>), dim3((unsigned)((n3 + 128 * kNT3 - 1) / (128 * kNT3))),
                           dim3(256), 0, a->stream, a->d_y2, a->T2, w + a->off_w[2], w + a->off_b[2], a->d_y3e, a->T3,
                           n3);
        hipLaunchKernelGGL(k_mtr, dim3((unsigned)((a->flat + 63) / 64), (unsigned)((nb + 63) / 64)), dim3(256), 0,
                           a->stream, a->d_y3e, a->d_y3, a->flat, nb, ld, c0);
    }
    {
        constexpr int envs_per_wg = (4 / (8 / kMfcMT)) * kMfcNT * 32;
        hipLaunchKernelGGL((k_mfc<kMfcMT, kMfcNT>), dim3((unsigned)((B + envs_per_wg - 1) / envs_per_wg)), dim3(256), 0,
                           a->stream, a->d_y3, ld, a->flat, w + a->off_w[3], w + a->off_b[3], a->d_h1, B);
    }
    ActArgs k{};
    k.h_in = a->d_h1;
    k.h_ld = ld;
    return act_tail(a, k, "measurement actor launch", B, env_offset, noisy, noise, eps, counter, actions, q_out,
                    random_out);
}

}  // extern "C"

// ---- exported state of both actors (the blob's header: qcart_state.hpp). An actor holds no natural-layout weights,
// so the payload is d_w as it is (the effective weights' fragments and the padded biases, for the measurement
// actor the convolutions' too), which of k_actor_act's four layers carry sigma fragments, and the seed. The seed is
// state, not geometry: an import takes the blob's.
namespace {
namespace st = qcart::state;
struct ActorHead {
    uint64_t seed;
    uint32_t sigma_mask;   // bit l: L[l].s / L[l].sb are set
    uint32_t pad;
};

st::Header actor_header(const qc_actor& a) {
    st::Header h = st::make(st::kActor);
    st::put_i(h, "data_length", a.p.data_length);
    st::put_i(h, "n_actions", a.n_act);
    st::put_i(h, "hidden2", a.w2);
    st::put_i(h, "max_batch", a.max_batch);
    st::put_i(h, "weight_floats", (int64_t)a.w_floats);
    h.payload_bytes = sizeof(ActorHead) + a.w_floats * sizeof(float);
    return h;
}
st::Header mactor_header(const qc_mactor& a) {
    st::Header h = st::make(st::kMactor);
    st::put_i(h, "read_length", a.p.read_length);
    st::put_i(h, "n_actions", a.n_act);
    st::put_i(h, "max_batch", a.max_batch);
    st::put_i(h, "chunk", a.chunk);
    st::put_i(h, "weight_floats", (int64_t)a.w_floats);
    h.payload_bytes = sizeof(ActorHead) + a.w_floats * sizeof(float);
    return h;
}

int actor_state_bytes(ActorCore* a, const st::Header& h, uint64_t* n) {
    Dev g(a->device);
    const hipError_t e = hipStreamSynchronize(a->stream);
    if (e != hipSuccess) return hip_fail(a->err, e, "actor state_bytes");
    *n = sizeof(st::Header) + h.payload_bytes;
    return QC_OK;
}

int actor_state_export(ActorCore* a, const st::Header& h, void* dst, uint64_t n) {
    const std::string who = std::string(st::kind_name(h.kind)) + "_state_export: ";
    if (!a->loaded) { a->err = who + "no weights have been loaded: there is no state to save"; return QC_EINVAL; }
    if (n != sizeof(st::Header) + h.payload_bytes) {
        a->err = who + "n is " + std::to_string(n) + ", state_bytes gives " +
                 std::to_string(sizeof(st::Header) + h.payload_bytes);
        return QC_EINVAL;
    }
    ActorHead s{};
    s.seed = a->seed;
    for (int l = 0; l < 4; ++l)
        if (a->L[l].s) s.sigma_mask |= 1u << l;
    std::memcpy(dst, &h, sizeof(h));
    st::Cursor cur(dst);
    std::memcpy(cur.take(sizeof(s)), &s, sizeof(s));
    Dev g(a->device);
    hipError_t e = hipStreamSynchronize(a->stream);
    if (e == hipSuccess) e = hipMemcpy(cur.take(a->w_floats * sizeof(float)), a->d_w, a->w_floats * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(a->err, e, "actor state export");
    return QC_OK;
}

// validates, then copies d_w in; *head: the payload's head for the caller to rebuild L from
int actor_state_import(ActorCore* a, const st::Header& mine, const void* src, uint64_t n, ActorHead* head) {
    st::Header h;
    std::string bad = st::validate(src, n, mine, &h);
    if (bad.empty() && h.payload_bytes != mine.payload_bytes)
        bad = std::string(st::kind_name(mine.kind)) + "_state_import: payload_bytes: blob " +
              std::to_string(h.payload_bytes) + ", handle " + std::to_string(mine.payload_bytes);
    if (bad.empty()) {
        std::memcpy(head, (const unsigned char*)src + sizeof(st::Header), sizeof(*head));
        if (head->sigma_mask > 15u || head->pad != 0)
            bad = std::string(st::kind_name(mine.kind)) + "_state_import: sigma_mask: blob " +
                  std::to_string(head->sigma_mask) + ", expected below 16";
    }
    if (!bad.empty()) { a->err = bad; return QC_EINVAL; }
    Dev g(a->device);
    hipError_t e = hipStreamSynchronize(a->stream);
    if (e == hipSuccess)
        e = hipMemcpy(a->d_w, (const unsigned char*)src + sizeof(st::Header) + sizeof(ActorHead),
                      a->w_floats * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(a->err, e, "actor state import");
    a->seed = head->seed;
    a->loaded = true;
    return QC_OK;
}
}  // namespace

extern "C" {

int qc_actor_state_bytes(qc_actor* a, uint64_t* n) { return a && n ? actor_state_bytes(a, actor_header(*a), n) : QC_EINVAL; }

int qc_actor_state_export(qc_actor* a, void* host_dst, uint64_t n) {
    return a && host_dst ? actor_state_export(a, actor_header(*a), host_dst, n) : QC_EINVAL;
}

int qc_actor_state_import(qc_actor* a, const void* host_src, uint64_t n) {
    if (!a) return QC_EINVAL;
    ActorHead s{};
    if (const int rc = actor_state_import(a, actor_header(*a), host_src, n, &s)) return rc;
    a->p.seed = s.seed;
    float* w = a->d_w;
    for (int l = 0; l < 4; ++l) {
        const bool sigma = (s.sigma_mask >> l & 1) != 0;
        a->L[l] = Layer{w + a->off_u[l], sigma ? w + a->off_s[l] : nullptr, w + a->off_ub[l],
                        sigma ? w + a->off_sb[l] : nullptr};
    }
    return QC_OK;
}

int qc_mactor_state_bytes(qc_mactor* a, uint64_t* n) { return a && n ? actor_state_bytes(a, mactor_header(*a), n) : QC_EINVAL; }

int qc_mactor_state_export(qc_mactor* a, void* host_dst, uint64_t n) {
    return a && host_dst ? actor_state_export(a, mactor_header(*a), host_dst, n) : QC_EINVAL;
}

int qc_mactor_state_import(qc_mactor* a, const void* host_src, uint64_t n) {
    if (!a) return QC_EINVAL;
    ActorHead s{};
    if (const int rc = actor_state_import(a, mactor_header(*a), host_src, n, &s)) return rc;
    a->p.seed = s.seed;
    float* w = a->d_w;
    for (int l = 4; l < 6; ++l) {   // fc21 / fc31 are k_actor_act's layers 2 / 3 (qc_mactor_load)
        const bool sigma = (s.sigma_mask >> (l - 2) & 1) != 0;
        a->L[l - 2] = Layer{w + a->off_w[l], sigma ? w + a->off_s[l] : nullptr, w + a->off_b[l],
                            sigma ? w + a->off_sb[l] : nullptr};
    }
    return QC_OK;
}

}  // extern "C"

// ---- the measurement network's forward stack for the measurement learner (qcart_learner.hpp) ----
namespace qcart {
namespace actor {
void launch_mtr(hipStream_t s, const float* in, float* out, int F, int64_t nb, int64_t ld, int64_t c0) {
    hipLaunchKernelGGL(k_mtr, dim3((unsigned)((F + 63) / 64), (unsigned)((nb + 63) / 64)), dim3(256), 0, s, in, out, F, nb,
                       ld, c0);
}
void launch_mnet_fwd(hipStream_t s, const MnetFwd& a) {
    const int64_t n1 = a.nb * a.T1, n2 = a.nb * a.T2, n3 = a.nb * a.T3;
    const int flat = 64 * a.T3;
    hipLaunchKernelGGL((k_mconv<2, 13, 5, 1, kNT1, kNA1, kQ1>), dim3((unsigned)((n1 + 128 * kNT1 - 1) / (128 * kNT1))),
                       dim3(256), 0, s, a.x, a.L, a.wf[0], a.bias[0], a.y1, a.T1, n1);
    hipLaunchKernelGGL((k_mconv<32, 11, 4, 2, kNT2, kNA2, kQ2>), dim3((unsigned)((n2 + 128 * kNT2 - 1) / (128 * kNT2))),
                       dim3(256), 0, s, a.y1, a.T1, a.wf[1], a.bias[1], a.y2, a.T2, n2);
    hipLaunchKernelGGL((k_mconv<64, 9, 4, 2, kNT3, kNA3, kQ3>), dim3((unsigned)((n3 + 128 * kNT3 - 1) / (128 * kNT3))),
                       dim3(256), 0, s, a.y2, a.T2, a.wf[2], a.bias[2], a.y3e, a.T3, n3);
    launch_mtr(s, a.y3e, a.y3f, flat, a.nb, a.ld, a.c0);
    constexpr int envs_per_wg = (4 / (8 / kMfcMT)) * kMfcNT * 32;
    hipLaunchKernelGGL((k_mfc<kMfcMT, kMfcNT>), dim3((unsigned)((a.nb + envs_per_wg - 1) / envs_per_wg)), dim3(256), 0, s,
                       a.y3f + a.c0, a.ld, flat, a.wf[3], a.bias[3], a.h + a.c0, a.nb);
}
}  // namespace actor
}  // namespace qcart
