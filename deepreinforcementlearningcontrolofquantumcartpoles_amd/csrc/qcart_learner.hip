// qcart_learner.hip — the device DQN learner: the reference's TrainDQN.__call__ (inverted harmonic
// oscillator/RL.py:159-232) with its LaProp optimizer (optimizer.py) for the 'xp' network direct_DQN
// (RL.py:80-106, layers.py), one update per call on a batch of B transitions, fp32 throughout.
// The four drivers' RL.py differ in fc2's width (256 / 512: the W2 template argument of k_learner_fwd / k_learner_bwd),
// in the TD target (k_learner_loss's mode, QC_TD_*) and in LaProp's betas: all three are handle parameters.
//
// Launches per update (plain launches on the handle's stream, no atomics on any gradient, so the same
// inputs give bit-identical parameters):
//   1 k_learner_noise  the 32 chunks' noise (injected, or Philox) -> feature-major [noise_len][32]
//   2 k_learner_fwd    3 B/32 workgroups: online/next, online/prev, target/next. The network of qcart_dqn.hpp
//                      (the actor's) plus the mean head fc32 / fc42; the online/prev pass
//                      also writes X, h1, h2, a3, r32 and the eps_in-scaled h2 / a3 feature-major to HBM
//   3 k_learner_loss   one workgroup: argmax (first index on ties), gathers, ul, dQ, dm, the loss sum
//   4 k_learner_bwd    B/32 workgroups: dX = W^T dY down the net from transposed fragments, ReLU masks from
//                      the stored activations; writes every layer's dY (and eps_out o dY) feature-major
//   5 k_learner_dw     one wave per 32x32 tile of every dW = dY X^T (K = B, the wave walks the whole batch
//                      in a fixed order) and the bias gradients (row sums of dY)
//   6 k_learner_wndot  <G, W> of the four weight-normalised layers (fixed-order tree, fp64; one workgroup per layer)
//   7 k_learner_opt    weight-norm chain rule + LaProp over the flat parameter / state buffers
//   8 k_learner_prep   ||W||_F, effective weights -> forward and transposed fragments
// The target network is a copy of the parameters and of the forward fragments (two device-to-device
// copies every backup_period updates).
// The table-driven kernels (noise, loss, dw, wndot, opt, prep) and the <256, true> instantiations of k_learner_fwd /
// k_learner_bwd (the measurement network's tail) also serve the measurement learner (qcart_mlearner.hip) through the
// launchers at the end of the namespace (qcart_learner.hpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/qcart.h"
#include "qcart_dqn.hpp"
#include "qcart_host.hpp"
#include "qcart_learner.hpp"

namespace qcart {
namespace learner {

using namespace qcart::dqn;
constexpr int kNT = 20;            // direct_DQN's parameter tensors

__device__ __forceinline__ float nz(const LArgs& a, int f, int row) { return a.noise[f * kChunks + row / a.rpc]; }

// W2: fc2's width. At W2 = 512 the LDS plan is the wide actor's (qcart_dqn.hpp): eps_in o H2 over the dead H1,
// fc31's output held in registers across one barrier; fc32 reads H2 before that barrier
// HIN: the measurement network's tail (DQN_measurement, RL.py:68-74): fc1 / fc2 are skipped, relu(fc1) of
// the convolutional stack (a.h_in, feature-major) enters as H2 at W2 = 256, and fo's fc31 / fc41 / fc32 / fc42
// slots hold fc21 / fc31 / fc22 / fc32
// W2C = W2 + kChunkTag: in_pad > kChunkIn (the 'wavefunction' input), fc1 over X0 in chunks (dense4_chunked); the
// online/prev pass still writes every X0 row to the workspace, so fc1's weight gradient is k_learner_dw's as at any length
template <int W2C, bool HIN = false>
__global__ __launch_bounds__(kThreads) void k_learner_fwd(const LArgs a) {
    constexpr int W2 = W2C & ~kChunkTag;
    constexpr bool CHUNK = (W2C & kChunkTag) != 0;
    static_assert(!HIN || W2 == kH2, "the measurement network's tail exists at H2 = 256 only");
    static_assert(!(HIN && CHUNK), "the measurement network's tail has no fc1");
    constexpr int kEpsIn31 = NoiseAt<W2>::kEpsIn31, kEpsOut31 = NoiseAt<W2>::kEpsOut31,
                  kEpsIn41 = NoiseAt<W2>::kEpsIn41, kEpsOut41 = NoiseAt<W2>::kEpsOut41;
    constexpr bool kWide = W2 != kH2;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* RA = lds;                      // H1 [512][32]; later H3 [256][32] + H3e [256][32]
    float* RB = lds + kH1 * kE;           // X0 [in_pad][32]; later H2 [256][32] + H2e [256][32], or H2 [512][32]
    float* RC = lds + 2 * kH1 * kE;       // fc41 sigma partial, as D registers
    float* RD = RC + 16 * 64;             // R32 [128][32]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = a.B / kE;
    const int pass = blockIdx.x / nb;     // 0 online / next, 1 online / prev, 2 target / next
    const int e0 = (blockIdx.x % nb) * kE;
    const int env = lane & 31, eg = e0 + env;
    const float* F = pass == 2 ? a.FT : a.F;
    const bool ws = pass == 1;
    const int B = a.B;

    float* H2 = RB;
    float* H2e = kWide ? RA : RB + kH2 * kE;   // wide: over H1, once fc2 is complete
    if constexpr (HIN) {
        // ---- relu(fc1) from HBM (coalesced 32-column rows) -> H2, eps_in(fc21) o H2
        for (int i = tid; i < kH2 * kE; i += kThreads) {
            const int k = i / kE, e = i % kE;
            const float h = a.h_in[(size_t)k * a.h_ld + (size_t)pass * B + e0 + e];
            const float he = h * nz(a, kEpsIn31 + k, e0 + e);
            H2[i] = h;
            H2e[i] = he;
            if (ws) {
                a.H2[(size_t)k * B + e0 + e] = h;
                a.H2e[(size_t)k * B + e0 + e] = he;
            }
        }
        __syncthreads();
    } else {
    if constexpr (CHUNK) {
        // ---- input and fc1 (ReLU), X0 through RB one chunk of rows at a time
        dense4_chunked(
            F + a.fo.u[0], RB, a.in_pad, tid,
            [&](int k, int e) {
                if (k >= a.in_len) return 0.f;
                const float x = a.trans[(size_t)(e0 + e) * a.row_len + (pass == 1 ? 0 : a.in_len) + k];
                if (ws) a.X0[(size_t)k * B + e0 + e] = x;
                return x;
            },
            [&](int o, float y) {
                const float h = fmaxf(y + F[a.fo.ub[0] + o], 0.f);
                RA[o * kE + env] = h;
                if (ws) a.H1[(size_t)o * B + eg] = h;
            });
    } else {
    for (int i = tid; i < a.in_pad * kE; i += kThreads) {
        const int k = i / kE, e = i % kE;
        const float x = k < a.in_len ? a.trans[(size_t)(e0 + e) * a.row_len + (pass == 1 ? 0 : a.in_len) + k] : 0.f;
        RB[i] = x;
        if (ws && k < a.in_len) a.X0[(size_t)k * B + e0 + e] = x;
    }
    __syncthreads();

    // ---- fc1: ReLU
    dense4(F + a.fo.u[0], nullptr, RB, nullptr, kH1, a.in_pad, lane, wave, [&](int o, float y, float) {
        const float h = fmaxf(y + F[a.fo.ub[0] + o], 0.f);
        RA[o * kE + env] = h;
        if (ws) a.H1[(size_t)o * B + eg] = h;
    });
    }
    __syncthreads();

    // ---- fc2: ReLU; eps_in(fc31) o H2
    dense4(F + a.fo.u[1], nullptr, RA, nullptr, W2, kH1, lane, wave, [&](int o, float y, float) {
        const float h = fmaxf(y + F[a.fo.ub[1] + o], 0.f);
        if constexpr (kWide) {
            H2[o * kE + env] = h;
            if (ws) a.H2[(size_t)o * B + eg] = h;
        } else {
            const float he = h * nz(a, kEpsIn31 + o, eg);
            H2[o * kE + env] = h;
            H2e[o * kE + env] = he;
            if (ws) {
                a.H2[(size_t)o * B + eg] = h;
                a.H2e[(size_t)o * B + eg] = he;
            }
        }
    });
    __syncthreads();
    if constexpr (kWide) {
        for (int i = tid; i < W2 * kE; i += kThreads) {
            const int k = i / kE, e = i % kE;
            const float he = H2[i] * nz(a, kEpsIn31 + k, e0 + e);
            H2e[i] = he;
            if (ws) a.H2e[(size_t)k * B + e0 + e] = he;
        }
        __syncthreads();
    }
    }   // !HIN

    // ---- fc31 (noisy): ReLU; eps_in(fc41) o H3
    float* H3 = RA;
    float* H3e = RA + kH3 * kE;
    auto act31 = [&](int o, float yu, float ys) {
        const float y = yu + F[a.fo.ub[2] + o] + nz(a, kEpsOut31 + o, eg) * (ys + F[a.fo.sb[2] + o]);
        return fmaxf(y, 0.f);
    };
    auto put3 = [&](int o, float h) {
        const float he = h * nz(a, kEpsIn41 + o, eg);
        H3[o * kE + env] = h;
        H3e[o * kE + env] = he;
        if (ws) {
            a.A3[(size_t)o * B + eg] = h;
            a.A3e[(size_t)o * B + eg] = he;
        }
    };
    float hold[kWide ? 2 : 1][16];
    if constexpr (kWide)
        dense4_hold2(F + a.fo.u[2], F + a.fo.s[2], H2, H2e, W2, lane, wave, hold, act31);
    else
        dense4(F + a.fo.u[2], F + a.fo.s[2], H2, H2e, kH3, W2, lane, wave,
               [&](int o, float yu, float ys) { put3(o, act31(o, yu, ys)); });
    // ---- fc32 (mean head): 4 tiles, 1 per wave; ReLU (the next-state argmax pass needs no mean)
    if (pass != 0)
        dense4(F + a.fo.u[4], nullptr, H2, nullptr, kHM, W2, lane, wave, [&](int o, float y, float) {
            const float h = fmaxf(y + F[a.fo.ub[4] + o], 0.f);
            RD[o * kE + env] = h;
            if (ws) a.R32[(size_t)o * B + eg] = h;
        });
    __syncthreads();
    if constexpr (kWide) {   // every wave is done reading H2 / H2e: RA is free
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) put3((wave + 4 * j) * 32 + drow(r, lane), hold[j][r]);
        __syncthreads();
    }

    // ---- fc41 -> Q; beside it fc42 on wave 2 (row 0 of its tile) -> M
    fc41(F + a.fo.u[3], F + a.fo.s[3], H3, H3e, RC, a.n_act, lane, wave,
         [&](int o, float yu, float ys) {
             a.Q[((size_t)pass * B + eg) * 32 + o] =
                 yu + F[a.fo.ub[3] + o] + nz(a, kEpsOut41 + o, eg) * (ys + F[a.fo.sb[3] + o]);
         },
         [&] {
             if (wave != 2 || pass == 0) return;
             f32x16 m = {};
             gemm_tile(m, F + a.fo.u[5], RD, ksteps(kHM), lane);
             if (lane < 32) a.M[(size_t)pass * B + eg] = m[0] + F[a.fo.ub[5]];
         });
}

// argmax of Q_online(next) (first index among equal maxima), the two gathers, the TD target, ul, the loss
// mean and the head gradients dQ [32][B] (rows >= n_act exact zeros), eps_out(fc41) o dQ, dm [B]. MODE: the TD
// target, QC_TD_ALIVE / QC_TD_REWARD_FAIL / QC_TD_REWARD (include/qcart.h)
template <int MODE>
__global__ __launch_bounds__(1024) void k_learner_loss(const LossArgs a) {
    __shared__ float part[1024];
    float lsum = 0.f;
    for (int b = threadIdx.x; b < a.B; b += 1024) {
        const float* q0 = a.Q + (size_t)b * 32;
        const float* q1 = a.Q + ((size_t)a.B + b) * 32;
        const float* q2 = a.Q + ((size_t)2 * a.B + b) * 32;
        int best = 0;
        float bq = q0[0], s1 = 0.f, s2 = 0.f;
        for (int j = 0; j < a.n_act; ++j) {
            if (q0[j] > bq) {
                bq = q0[j];
                best = j;
            }
            s1 += q1[j];
            s2 += q2[j];
        }
        const float* row = a.trans + (size_t)b * a.row_len;
        int act = (int)row[2 * a.in_len];
        if (act < 0 || act >= a.n_act) {
            a.cnt[1] = 1;
            act = act < 0 ? 0 : a.n_act - 1;
        }
        const float sav = q1[act] + a.M[a.B + b] - s1 * a.inv_A;
        const float nsv = q2[best] + a.M[2 * a.B + b] - s2 * a.inv_A;
        float y;
        if constexpr (MODE == QC_TD_ALIVE) {   // IHO / IQO RL.py: the alive reward, 0 on a failing row
            y = nsv * a.gamma + a.rew;
            if (row[2 * a.in_len + 1] == a.failing) y = 0.f;
        } else {                               // QO / HO RL.py: the row's own reward
            const float r = row[2 * a.in_len + 1];
            y = nsv * a.gamma + a.omg * r;
            if (MODE == QC_TD_REWARD_FAIL && r <= a.failing) y = r;
        }
        const float d = sav - y;
        const float ul = d * d;
        a.ul[b] = ul;
        lsum += ul * a.w[b];
        const float delta = 2.f * d * a.w[b] * a.inv_B;
        a.dM[b] = delta;
        const int c = b / a.rpc;
        for (int j = 0; j < 32; ++j) {
            const float g = j < a.n_act ? delta * ((j == act ? 1.f : 0.f) - a.inv_A) : 0.f;
            a.dQ[(size_t)j * a.B + b] = g;
            a.dQe[(size_t)j * a.B + b] = j < a.n_act ? g * a.noise[(a.eps_out41 + j) * kChunks + c] : 0.f;
        }
    }
    lsum = block_sum(lsum, part);
    if (threadIdx.x == 0) {
        const float loss = lsum * a.inv_B;
        a.loss[0] = loss;
        if (a.loss_user) a.loss_user[0] = loss;
        if (!isfinite(loss)) a.cnt[0] += 1;
    }
}

// dX down the online net for 32 rows: LDS holds dQ / dQe [32][32], dZ3 / dZ3e [256][32], dZ32 [128][32], dZ2 [W2][32]
// (120 KiB at W2 = 256, 152 KiB at 512)
constexpr int bwd_lds_floats(int w2) { return (32 + 32 + 2 * kH3 + kHM + w2) * kE; }
// HIN (the measurement network's tail): stops at dZ2, the gradient at fc1's pre-activation
template <int W2, bool HIN = false>
__global__ __launch_bounds__(kThreads) void k_learner_bwd(const LArgs a) {
    constexpr int kEpsIn31 = NoiseAt<W2>::kEpsIn31, kEpsOut31 = NoiseAt<W2>::kEpsOut31,
                  kEpsIn41 = NoiseAt<W2>::kEpsIn41;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* DQ = lds;
    float* DQe = DQ + 32 * kE;
    float* D3 = DQe + 32 * kE;
    float* D3e = D3 + kH3 * kE;
    float* D32 = D3e + kH3 * kE;
    float* D2 = D32 + kHM * kE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e0 = blockIdx.x * kE, env = lane & 31, eg = e0 + env, B = a.B;
    const float* F = a.F;

    for (int i = tid; i < 32 * kE; i += kThreads) {
        const int j = i / kE, e = i % kE;
        DQ[i] = a.dQ[(size_t)j * B + e0 + e];
        DQe[i] = a.dQe[(size_t)j * B + e0 + e];
    }
    // fc42 / fc32's ReLU: dZ32[o] = W42_eff[o] dm (r32[o] > 0)
    for (int i = tid; i < kHM * kE; i += kThreads) {
        const int o = i / kE, e = i % kE;
        const float g = a.R32[(size_t)o * B + e0 + e] > 0.f ? F[a.fo.w42 + o] * a.dM[e0 + e] : 0.f;
        D32[i] = g;
        a.dZ32[(size_t)o * B + e0 + e] = g;
    }
    __syncthreads();

    // ---- fc41^T: dA3 = u_w^T dQ + eps_in o (sigma_w^T (eps_out o dQ)); ReLU mask of a3
    dense4(F + a.fo.t41u, F + a.fo.t41s, DQ, DQe, kH3, 32, lane, wave, [&](int o, float yu, float ys) {
        const float g = a.A3[(size_t)o * B + eg] > 0.f ? yu + nz(a, kEpsIn41 + o, eg) * ys : 0.f;
        const float ge = g * nz(a, kEpsOut31 + o, eg);
        D3[o * kE + env] = g;
        D3e[o * kE + env] = ge;
        a.dZ3[(size_t)o * B + eg] = g;
        a.dZ3e[(size_t)o * B + eg] = ge;
    });
    __syncthreads();

    // ---- fc31^T and fc32^T meet in h2: dH2 = u_w^T dZ3 + W32_eff^T dZ32 + eps_in o (sigma_w^T dZ3e)
    for (int t = wave; t < tiles(W2); t += 4) {
        f32x16 acc = {}, accs = {};
        gemm_tile(acc, F + a.fo.t31u + (size_t)t * ksteps(kH3) * 64, D3, ksteps(kH3), lane);
        gemm_tile(acc, F + a.fo.t32 + (size_t)t * ksteps(kHM) * 64, D32, ksteps(kHM), lane);
        gemm_tile(accs, F + a.fo.t31s + (size_t)t * ksteps(kH3) * 64, D3e, ksteps(kH3), lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = t * 32 + drow(r, lane);
            const float g = a.H2[(size_t)o * B + eg] > 0.f ? acc[r] + nz(a, kEpsIn31 + o, eg) * accs[r] : 0.f;
            D2[o * kE + env] = g;
            a.dZ2[(size_t)o * B + eg] = g;
        }
    }
    if constexpr (HIN) return;
    __syncthreads();

    // ---- fc2^T: dH1 = W2_eff^T dZ2; ReLU mask of h1
    dense4(F + a.fo.t2, nullptr, D2, nullptr, kH1, W2, lane, wave, [&](int o, float y, float) {
        a.dZ1[(size_t)o * B + eg] = a.H1[(size_t)o * B + eg] > 0.f ? y : 0.f;
    });
}

// one wave per 32x32 output tile; the contraction runs over the whole batch in one fixed order: k-step
// (j, i) pairs rows b = 8j + i (lanes 0-31) and 8j + 4 + i (lanes 32-63), i = 0..3, from one 16-B load per lane
__global__ __launch_bounds__(kThreads) void k_learner_dw(const DwJob* __restrict__ jobs, const int4* __restrict__ tl,
                                                         int ntiles, int B) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = blockIdx.x * 4 + wave;
    if (t >= ntiles) return;
    const int4 T = tl[t];
    const DwJob J = jobs[T.x];
    const int r = lane & 31, h = lane >> 5;
    const float4* ap = reinterpret_cast<const float4*>(J.A + (size_t)(T.y * 32 + r) * B + 4 * h);
    const float4* xp = reinterpret_cast<const float4*>(J.X + (size_t)(T.z * 32 + r) * B + 4 * h);
    f32x16 acc0 = {}, acc1 = {};
    float rs = 0.f;
    const int n = B / 8;
    float4 av = ap[0], xv = xp[0];
    for (int j = 0; j < n; ++j) {
        const int jn = j + 1 < n ? j + 1 : j;
        const float4 an = ap[2 * jn], xn = xp[2 * jn];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, xv.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, xv.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, xv.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, xv.w, acc1, 0, 0, 0);
        rs += (av.x + av.y) + (av.z + av.w);
        av = an;
        xv = xn;
    }
    acc0 += acc1;
    rs += __shfl_xor(rs, 32, 64);
    if (T.z == 0 && J.bias && h == 0 && T.y * 32 + r < J.O) J.bias[T.y * 32 + r] = rs;
    const int k = T.z * 32 + r;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int o = T.y * 32 + drow(q, lane);
        if (o < J.O && k < J.K) J.out[(size_t)o * J.K + k] = acc0[q];
    }
}

// <G, W> over a weight-normalised layer's weight (G = the gradient of the effective weight): fp64, fixed
// order; tensor ti + 2 is the layer's weight_norm g
__global__ __launch_bounds__(1024) void k_learner_wndot(const float* __restrict__ P, const float* __restrict__ G,
                                                        const WnTensors wt /* tensor index per block */,
                                                        const TensorTable tt, double* __restrict__ dot) {
    __shared__ double part[1024];
    const int ti = wt.t[blockIdx.x];
    const Tensor T = tt.t[ti];
    double s = 0.0;
    for (int i = threadIdx.x; i < T.n; i += 1024) s += (double)G[T.off + i] * (double)P[T.off + i];
    s = block_sum(s, part);
    if (threadIdx.x == 0) {
        dot[T.wn] = s;
        dot[kMaxWN + T.wn] = (double)P[tt.t[ti + 2].off];   // g before the step: the optimizer updates it in the same launch as W
    }
}

// LaProp (optimizer.py:62-100, centered, no amsgrad, no weight decay) over every tensor; blockIdx.y = tensor
__global__ __launch_bounds__(256) void k_learner_opt(const OptArgs a, const TensorTable tt) {
    const Tensor T = tt.t[blockIdx.y];
    float c1 = 0.f, c2 = 0.f, dg = 0.f;
    if (a.chain && T.kind) {
        const double n = (double)a.norm[T.wn], d = a.dot[T.wn];
        if (T.kind == 1) {
            const double g = a.dot[kMaxWN + T.wn];
            c1 = (float)(g / n);
            c2 = (float)(d / (n * n));
        } else {
            dg = (float)(d / n);
        }
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < T.n; i += gridDim.x * 256) {
        const int x = T.off + i;
        float g = a.G[x];
        float p = a.P[x];
        if (a.chain && T.kind) {
            g = T.kind == 1 ? c1 * (g - c2 * p) : dg;
            a.G[x] = g;
        }
        const float v = a.V[x] * a.beta2 + a.omb2 * (g * g);
        const float mu = a.MU[x] * a.beta2 + a.omb2 * g;
        float den = a.centered ? v - mu * mu : v;
        den = sqrtf(den / a.l2) + a.eps;
        const float e = a.E[x] * a.beta1 + a.elr * (g / den);
        p -= a.step_size * e;
        a.V[x] = v;
        a.MU[x] = mu;
        a.E[x] = e;
        a.P[x] = p;
    }
}

// effective weight (W g / ||W||_F, or W) -> fragments / a plain vector; bias padded to tiles * 32
__global__ __launch_bounds__(1024) void k_learner_prep(const float* __restrict__ P, float* __restrict__ F,
                                                       const PrepJob* __restrict__ jobs, float* __restrict__ norm) {
    __shared__ double part[1024];
    const PrepJob J = jobs[blockIdx.x];
    const float* W = P + J.w_off;
    double ss = 0.0;
    if (J.g_off >= 0) {
        for (int i = threadIdx.x; i < J.O * J.K; i += 1024) ss += (double)W[i] * (double)W[i];
    }
    ss = block_sum(ss, part);
    const float sc = J.g_off >= 0 ? wn_scale(P[J.g_off], ss) : 1.f;
    if (J.mode != 1 && J.wn >= 0 && blockIdx.y == 0 && threadIdx.x == 0) norm[J.wn] = (float)sqrt(ss);
    float* out = F + J.out_off;
    const int first = blockIdx.y * 1024 + threadIdx.x, stride = kPrepParts * 1024;
    if (J.mode == 2) {
        for (int i = first; i < J.O * J.K; i += stride) out[i] = W[i] * sc;
        return;
    }
    const int Om = J.mode == 0 ? J.O : J.K, Km = J.mode == 0 ? J.K : J.O;   // the fragment matrix [Om][Km]
    const int T = tiles(Om), S = ksteps(J.Kpad);
    for (int i = first; i < T * S * 64; i += stride) {
        int o, k;
        frag_ok(i, S, 0, o, k);
        out[i] = (o < Om && k < Km) ? W[J.mode == 0 ? (size_t)o * J.K + k : (size_t)k * J.K + o] * sc : 0.f;
    }
    if (J.bias_pad_off >= 0)
        for (int i = first; i < tiles(J.O) * 32; i += stride)
            F[J.bias_pad_off + i] = (i < J.O && J.bias_off >= 0) ? P[J.bias_off + i] : 0.f;
}

// the 32 chunks' noise -> feature-major [noise_len][32]: injected [32][noise_len], or f(z) = sign(z) sqrt|z|
// (layers.py:82-83) of Philox normals keyed by (seed, chunk), counter, tag 0x100 + pair (k_actor_noise's draw)
__global__ __launch_bounds__(256) void k_learner_noise(const float* __restrict__ in, float* __restrict__ out,
                                                       int noise_len, uint64_t seed, uint64_t counter) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (in) {
        if (i < kChunks * noise_len) out[(i % noise_len) * kChunks + i / noise_len] = in[i];
        return;
    }
    const int np = (noise_len + 1) / 2;
    if (i >= kChunks * np) return;
    const int c = i % kChunks, p = i / kChunks;
    const float2 f = noise_pair(seed, counter, (uint32_t)c, p);
    out[(2 * p) * kChunks + c] = f.x;
    if (2 * p + 1 < noise_len) out[(2 * p + 1) * kChunks + c] = f.y;
}

// ---- the launchers of qcart_learner.hpp (the measurement learner drives the same kernels) ----
void launch_noise(hipStream_t s, const float* in, float* out, int noise_len, uint64_t seed, uint64_t counter) {
    const int n = in ? kChunks * noise_len : kChunks * ((noise_len + 1) / 2);
    hipLaunchKernelGGL(k_learner_noise, dim3((n + 255) / 256), dim3(256), 0, s, in, out, noise_len, seed, counter);
}
void launch_loss(hipStream_t s, int target_mode, const LossArgs& a) {
    if (target_mode == QC_TD_REWARD_FAIL)
        hipLaunchKernelGGL(k_learner_loss<QC_TD_REWARD_FAIL>, dim3(1), dim3(1024), 0, s, a);
    else if (target_mode == QC_TD_REWARD)
        hipLaunchKernelGGL(k_learner_loss<QC_TD_REWARD>, dim3(1), dim3(1024), 0, s, a);
    else
        hipLaunchKernelGGL(k_learner_loss<QC_TD_ALIVE>, dim3(1), dim3(1024), 0, s, a);
}
void launch_dw(hipStream_t s, const DwJob* jobs, const int4* tl, int ntiles, int B) {
    hipLaunchKernelGGL(k_learner_dw, dim3((ntiles + 3) / 4), dim3(kThreads), 0, s, jobs, tl, ntiles, B);
}
void launch_wndot(hipStream_t s, int n_layers, const float* P, const float* G, const WnTensors& wn_tensors,
                  const TensorTable& tt, double* dot) {
    hipLaunchKernelGGL(k_learner_wndot, dim3(n_layers), dim3(1024), 0, s, P, G, wn_tensors, tt, dot);
}
void launch_opt(hipStream_t s, const OptArgs& o, const TensorTable& tt, int nt) {
    hipLaunchKernelGGL(k_learner_opt, dim3(64, nt), dim3(256), 0, s, o, tt);
}
void launch_prep(hipStream_t s, const float* P, float* F, const PrepJob* jobs, int njobs, float* norm) {
    hipLaunchKernelGGL(k_learner_prep, dim3(njobs, kPrepParts), dim3(1024), 0, s, P, F, jobs, norm);
}
bool enable_mtail_lds() {
    return hipFuncSetAttribute((const void*)k_learner_fwd<kH2, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               kLdsFloats * (int)sizeof(float)) == hipSuccess &&
           hipFuncSetAttribute((const void*)k_learner_bwd<kH2, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               bwd_lds_floats(kH2) * (int)sizeof(float)) == hipSuccess;
}
void launch_mtail_fwd(hipStream_t s, const LArgs& a) {
    hipLaunchKernelGGL((k_learner_fwd<kH2, true>), dim3(3 * a.B / kE), dim3(kThreads), kLdsFloats * sizeof(float), s, a);
}
void launch_mtail_bwd(hipStream_t s, const LArgs& a) {
    hipLaunchKernelGGL((k_learner_bwd<kH2, true>), dim3(a.B / kE), dim3(kThreads), bwd_lds_floats(kH2) * sizeof(float), s, a);
}

}  // namespace learner
}  // namespace qcart

using namespace qcart::learner;
using namespace qcart::host;

struct qc_learner {
    qc_learner_params p{};
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    bool loaded = false;
    int in_pad = 0, noise_len = 0, A = 0, L = 0, B = 0;
    int w2 = kH2;             // fc2's width: the instantiation of k_learner_fwd / k_learner_bwd
    bool chunked = false;     // data_length above kChunkIn: k_learner_fwd<w2 + kChunkTag>
    double b1 = 0, b2 = 0;    // LaProp's betas
    // host-side schedule and LaProp scalars (optimizer.py:69-80)
    int64_t updates = 0, step = 0;
    int backup_counter = 0;
    double lr = 0, l1 = 0, l2 = 0;
    int launches = 0;         // launches of the last update
    TensorTable tt{};
    int np = 0;               // floats in one parameter buffer
    int nf = 0, nf_fwd = 0;   // floats in the fragment buffer / its forward part
    FragOff fo{};
    float *P = nullptr, *PT = nullptr, *G = nullptr, *E = nullptr, *V = nullptr, *MU = nullptr;
    float *F = nullptr, *FT = nullptr;
    float* ws = nullptr;      // workspace: Q, M, noise, activations, dY
    size_t ws_floats = 0;
    LArgs k{};
    float *d_noise = nullptr, *d_loss = nullptr, *d_norm = nullptr;
    double* d_dot = nullptr;
    int32_t* d_cnt = nullptr;
    DwJob* d_dwjobs = nullptr;
    int4* d_tiles = nullptr;
    int ntiles = 0;
    PrepJob* d_prep = nullptr;
    int nprep = 0;
    WnTensors wn_tensors{};
};

namespace {
CreateError g_learner_err;

using FwdKernel = void (*)(const LArgs);
FwdKernel fwd_kernel(int w2, bool chunked) {
    if (chunked) return w2 == kH2Wide ? k_learner_fwd<kH2Wide + kChunkTag> : k_learner_fwd<kH2 + kChunkTag>;
    return w2 == kH2Wide ? k_learner_fwd<kH2Wide> : k_learner_fwd<kH2>;
}

// tensor indices of layer l (fc1, fc2, fc31, fc41, fc32, fc42): weight, bias, then g | sigma_w, sigma_b
constexpr int kFirst[6] = {0, 3, 6, 10, 14, 17};
constexpr bool kNoisy[6] = {false, false, true, true, false, false};
constexpr LayerRule kLearnerRules[] = {
    {0b001100, states_where([](bool wn, bool sw, bool sb) { return !sw || !sb || wn; }),
     "fc31 / fc41 are FactorizedNoisy layers (sigma_w and sigma_b, no weight_norm): the learner "
     "implements direct_DQN(noisy_layers=2)"},
    {0b110011, states_where([](bool wn, bool sw, bool sb) { return !wn || sw || sb; }),
     "fc1 / fc2 / fc32 / fc42 are Linear_weight_normalize layers (weight_norm, no sigma)"},
};

// the six layers' tensors inside one flat buffer (the parameters, the target's, or the gradients)
void layer_views(const qc_learner* l, const float* base, qc_dqn_layer out[6]) {
    for (int j = 0; j < 6; ++j) {
        const Tensor* T = &l->tt.t[kFirst[j]];
        out[j] = qc_dqn_layer{base + T[0].off, base + T[1].off, kNoisy[j] ? nullptr : base + T[2].off,
                              kNoisy[j] ? base + T[2].off : nullptr, kNoisy[j] ? base + T[3].off : nullptr};
    }
}

void free_all(qc_learner* l) {
    for (void* q : {(void*)l->P, (void*)l->PT, (void*)l->G, (void*)l->E, (void*)l->V, (void*)l->MU, (void*)l->F,
                    (void*)l->FT, (void*)l->ws, (void*)l->d_dot, (void*)l->d_cnt, (void*)l->d_dwjobs,
                    (void*)l->d_tiles, (void*)l->d_prep})
        if (q) (void)hipFree(q);
}

// optimizer step + fragment preparation (the tail of an update, and qc_learner_apply)
void optimizer_and_prep(qc_learner* l, int chain) {
    l->step += 1;
    l->l1 = l->l1 * l->b1 + (1 - l->b1) * l->lr;
    l->l2 = l->l2 * l->b2 + (1 - l->b2);
    OptArgs o{};
    o.P = l->P; o.G = l->G; o.E = l->E; o.V = l->V; o.MU = l->MU;
    o.dot = l->d_dot;
    o.norm = l->d_norm;
    o.chain = chain;
    o.centered = l->step > kCenteredAfter ? 1 : 0;
    o.beta1 = (float)l->b1;
    o.beta2 = (float)l->b2;
    o.omb2 = (float)(1 - l->b2);
    o.l2 = (float)l->l2;
    o.elr = (float)((1 - l->b1) * l->lr);
    o.step_size = (float)(l->lr != 0. ? 1. / (l->l1 / l->lr) : 1.);
    o.eps = (float)kEps;
    hipLaunchKernelGGL(k_learner_opt, dim3(64, kNT), dim3(256), 0, l->stream, o, l->tt);
    hipLaunchKernelGGL(k_learner_prep, dim3(l->nprep, kPrepParts), dim3(1024), 0, l->stream, l->P, l->F, l->d_prep,
                       l->d_norm);
}
}  // namespace

extern "C" {

int qc_learner_create(const qc_learner_params* p, int device, qc_learner** out) {
    if (!out || !p) return QC_EINVAL;
    *out = nullptr;
    auto fail = [](const char* m, int rc) { return g_learner_err.fail(m, rc); };
    if (const char* m = bad_net_size(p->data_length, p->n_actions)) return fail(m, QC_EINVAL);
    if (p->batch_size < 128 || p->batch_size > 4096 || p->batch_size % 128 != 0)
        return fail("batch_size must be a multiple of 128 in [128, 4096]: the learner implements FactorizedNoisy's "
                    "32-chunk noise branch (layers.py:57-74), not the per-row branch of other batch sizes",
                    QC_EINVAL);
    if (p->backup_period < 1) return fail("backup_period must be >= 1", QC_EINVAL);
    if (!(p->lr >= 0.)) return fail("lr must be >= 0", QC_EINVAL);
    const int w2 = fc2_width(p->hidden2);
    if (!w2) return fail("hidden2 must be 0, 256 or 512 (fc2's width)", QC_EINVAL);
    if (p->target_mode != QC_TD_ALIVE && p->target_mode != QC_TD_REWARD_FAIL && p->target_mode != QC_TD_REWARD)
        return fail("target_mode must be QC_TD_ALIVE, QC_TD_REWARD_FAIL or QC_TD_REWARD", QC_EINVAL);
    if (!(p->beta1 >= 0. && p->beta1 < 1.)) return fail("beta1 must be in [0, 1) (0: 0.9)", QC_EINVAL);
    if (!(p->beta2 >= 0. && p->beta2 < 1.)) return fail("beta2 must be in [0, 1) (0: 0.9995)", QC_EINVAL);
    if (const int rc = check_device(device, g_learner_err, "the learner")) return rc;

    qc_learner* l = new qc_learner();
    l->p = *p;
    l->device = device;
    l->lr = p->lr;
    const int L = l->L = p->data_length, A = l->A = p->n_actions, B = l->B = p->batch_size;
    l->in_pad = in_pad(L);
    l->w2 = w2;
    l->chunked = l->in_pad > kChunkIn;
    l->b1 = p->beta1 != 0. ? p->beta1 : kBeta1;
    l->b2 = p->beta2 != 0. ? p->beta2 : kBeta2;
    l->noise_len = noise_len(w2, A);

    // ---- parameter tensors (offsets in multiples of 4 floats)
    const int O[6] = {kH1, w2, kH3, A, kHM, 1};
    const int K[6] = {L, kH1, w2, kH3, w2, kHM};
    int off = 0, nwn = 0;
    int wn_of[6] = {-1, -1, -1, -1, -1, -1};
    auto add = [&](int ti, int n, int kind, int wn, int w_off) {
        l->tt.t[ti] = Tensor{off, n, kind, wn, w_off};
        off += (n + 3) & ~3;
    };
    for (int j = 0; j < 6; ++j) {
        const int t0 = kFirst[j];
        if (kNoisy[j]) {
            add(t0, O[j] * K[j], 0, -1, 0);
            add(t0 + 1, O[j], 0, -1, 0);
            add(t0 + 2, O[j] * K[j], 0, -1, 0);
            add(t0 + 3, O[j], 0, -1, 0);
        } else {
            wn_of[j] = nwn;
            l->wn_tensors.t[nwn] = t0;
            const int w_off = off;
            add(t0, O[j] * K[j], 1, nwn, w_off);
            add(t0 + 1, O[j], 0, -1, 0);
            add(t0 + 2, 1, 2, nwn, w_off);
            ++nwn;
        }
    }
    l->np = off;

    // ---- fragment buffer: forward fragments and padded biases, then the transposed fragments
    const int Kp[6] = {l->in_pad, kH1, w2, kH3, w2, kHM};
    int fo = frag_layout(6, O, Kp, kNoisy, l->fo.u, l->fo.s, l->fo.ub, l->fo.sb);
    l->nf_fwd = fo;
    auto tfrag = [&](int j, int kpad) {   // fragments of W_j^T: [K_j rows][O_j pad kpad]
        const int at = fo;
        fo += tiles(K[j]) * ksteps(kpad) * 64;
        return at;
    };
    l->fo.t2 = tfrag(1, w2);
    l->fo.t31u = tfrag(2, kH3);
    l->fo.t31s = tfrag(2, kH3);
    l->fo.t41u = tfrag(3, 32);
    l->fo.t41s = tfrag(3, 32);
    l->fo.t32 = tfrag(4, kHM);
    l->fo.w42 = fo; fo += kHM;
    l->nf = fo;

    std::vector<PrepJob> prep;
    for (int j = 0; j < 6; ++j) {
        const Tensor* T = &l->tt.t[kFirst[j]];
        const int g_off = kNoisy[j] ? -1 : T[2].off;
        prep.push_back(PrepJob{T[0].off, g_off, wn_of[j], O[j], K[j], 0, Kp[j], l->fo.u[j], T[1].off, l->fo.ub[j]});
        if (kNoisy[j])
            prep.push_back(PrepJob{T[2].off, -1, -1, O[j], K[j], 0, Kp[j], l->fo.s[j], T[3].off, l->fo.sb[j]});
    }
    auto tjob = [&](int j, int sigma, int kpad, int out_off) {
        const Tensor* T = &l->tt.t[kFirst[j]];
        prep.push_back(PrepJob{T[sigma ? 2 : 0].off, kNoisy[j] ? -1 : T[2].off, -1, O[j], K[j], 1, kpad, out_off, -1, -1});
    };
    tjob(1, 0, w2, l->fo.t2);
    tjob(2, 0, kH3, l->fo.t31u);
    tjob(2, 1, kH3, l->fo.t31s);
    tjob(3, 0, 32, l->fo.t41u);
    tjob(3, 1, 32, l->fo.t41s);
    tjob(4, 0, kHM, l->fo.t32);
    prep.push_back(PrepJob{l->tt.t[17].off, l->tt.t[19].off, -1, 1, kHM, 2, kHM, l->fo.w42, -1, -1});
    l->nprep = (int)prep.size();

    // ---- workspace (floats): every feature-major array has its rows padded to 32 and its pad rows zero
    const int x0_rows = tiles(L) * 32;
    size_t w = 0;
    auto take = [&](size_t n) {
        const size_t at = w;
        w += (n + 3) & ~(size_t)3;
        return at;
    };
    const size_t oQ = take((size_t)3 * B * 32), oM = take((size_t)3 * B), oN = take((size_t)l->noise_len * kChunks);
    const size_t oX0 = take((size_t)x0_rows * B), oH1 = take((size_t)kH1 * B), oH2 = take((size_t)w2 * B),
                 oH2e = take((size_t)w2 * B), oA3 = take((size_t)kH3 * B), oA3e = take((size_t)kH3 * B),
                 oR32 = take((size_t)kHM * B), odQ = take((size_t)32 * B), odQe = take((size_t)32 * B),
                 odM = take((size_t)32 * B), odZ3 = take((size_t)kH3 * B), odZ3e = take((size_t)kH3 * B),
                 odZ32 = take((size_t)kHM * B), odZ2 = take((size_t)w2 * B), odZ1 = take((size_t)kH1 * B);
    const size_t oLoss = take(4), oNorm = take(kMaxWN);
    l->ws_floats = w;

    Dev g(device);
    const size_t pb = (size_t)l->np * sizeof(float);
    hipError_t e = hipSuccess;
    for (float** q : {&l->P, &l->PT, &l->G, &l->E, &l->V, &l->MU}) {
        if (e == hipSuccess) e = hipMalloc(q, pb);
        if (e == hipSuccess) e = hipMemset(*q, 0, pb);
    }
    if (e == hipSuccess) e = hipMalloc(&l->F, (size_t)l->nf * sizeof(float));
    if (e == hipSuccess) e = hipMemset(l->F, 0, (size_t)l->nf * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&l->FT, (size_t)l->nf_fwd * sizeof(float));
    if (e == hipSuccess) e = hipMemset(l->FT, 0, (size_t)l->nf_fwd * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&l->ws, w * sizeof(float));
    if (e == hipSuccess) e = hipMemset(l->ws, 0, w * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&l->d_dot, 2 * kMaxWN * sizeof(double));
    if (e == hipSuccess) e = hipMemset(l->d_dot, 0, 2 * kMaxWN * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&l->d_cnt, 2 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(l->d_cnt, 0, 2 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&l->d_prep, prep.size() * sizeof(PrepJob));
    if (e == hipSuccess) e = hipMemcpy(l->d_prep, prep.data(), prep.size() * sizeof(PrepJob), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        free_all(l);
        delete l;
        return fail("device allocation failed", QC_ENOMEM);
    }
    float* W = l->ws;
    LArgs& k = l->k;
    k.F = l->F;
    k.FT = l->FT;
    k.fo = l->fo;
    k.in_len = L; k.in_pad = l->in_pad; k.n_act = A; k.B = B; k.row_len = 2 * L + 2; k.rpc = B / kChunks;
    k.noise = l->d_noise = W + oN;
    k.Q = W + oQ; k.M = W + oM;
    k.X0 = W + oX0; k.H1 = W + oH1; k.H2 = W + oH2; k.H2e = W + oH2e; k.A3 = W + oA3; k.A3e = W + oA3e; k.R32 = W + oR32;
    k.dQ = W + odQ; k.dQe = W + odQe; k.dM = W + odM; k.dZ3 = W + odZ3; k.dZ3e = W + odZ3e; k.dZ32 = W + odZ32;
    k.dZ2 = W + odZ2; k.dZ1 = W + odZ1;
    l->d_loss = W + oLoss;
    l->d_norm = W + oNorm;

    // ---- the dW jobs and their tiles (dY, X, gradient tensor, bias gradient tensor)
    float* G = l->G;
    auto gt = [&](int ti) { return G + l->tt.t[ti].off; };
    const DwJob jobs[8] = {
        {k.dZ1, k.X0, gt(0), gt(1), kH1, L},        {k.dZ2, k.H1, gt(3), gt(4), w2, kH1},
        {k.dZ3, k.H2, gt(6), gt(7), kH3, w2},       {k.dZ3e, k.H2e, gt(8), gt(9), kH3, w2},
        {k.dQ, k.A3, gt(10), gt(11), A, kH3},       {k.dQe, k.A3e, gt(12), gt(13), A, kH3},
        {k.dZ32, k.H2, gt(14), gt(15), kHM, w2},   {k.dM, k.R32, gt(17), gt(18), 1, kHM},
    };
    std::vector<int4> tl;
    for (int j = 0; j < 8; ++j)
        for (int to = 0; to < tiles(jobs[j].O); ++to)
            for (int tk = 0; tk < tiles(jobs[j].K); ++tk) tl.push_back(int4{j, to, tk, 0});
    l->ntiles = (int)tl.size();
    e = hipMalloc(&l->d_dwjobs, sizeof(jobs));
    if (e == hipSuccess) e = hipMemcpy(l->d_dwjobs, jobs, sizeof(jobs), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&l->d_tiles, tl.size() * sizeof(int4));
    if (e == hipSuccess) e = hipMemcpy(l->d_tiles, tl.data(), tl.size() * sizeof(int4), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)fwd_kernel(w2, l->chunked), hipFuncAttributeMaxDynamicSharedMemorySize,
                                kLdsFloats * (int)sizeof(float));
    if (e == hipSuccess)
        e = hipFuncSetAttribute(w2 == kH2Wide ? (const void*)k_learner_bwd<kH2Wide> : (const void*)k_learner_bwd<kH2>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, bwd_lds_floats(w2) * (int)sizeof(float));
    if (e != hipSuccess) {
        free_all(l);
        delete l;
        return fail("device setup failed (job tables / LDS size of the learner kernels)", QC_EHIP);
    }
    *out = l;
    return QC_OK;
}

void qc_learner_destroy(qc_learner* l) {
    if (!l) return;
    {
        Dev g(l->device);
        (void)hipDeviceSynchronize();
        free_all(l);
    }
    delete l;
}

const char* qc_learner_last_error(const qc_learner* l) { return l ? l->err.c_str() : g_learner_err.text(); }

int qc_learner_set_stream(qc_learner* l, void* stream) {
    if (!l) return QC_EINVAL;
    l->stream = (hipStream_t)stream;
    return QC_OK;
}

int qc_learner_noise_len(const qc_learner* l) { return l ? l->noise_len : QC_EINVAL; }

int qc_learner_load(qc_learner* l, const qc_dqn_layer layers[6]) {
    if (!l || !layers) return QC_EINVAL;
    if (const int rc = validate_layers(layers, 6, kLearnerRules, 2, l->err)) return rc;
    Dev g(l->device);
    hipError_t e = hipSuccess;
    auto put = [&](int ti, const float* src) {
        const Tensor& T = l->tt.t[ti];
        if (e == hipSuccess)
            e = hipMemcpyAsync(l->P + T.off, src, (size_t)T.n * sizeof(float), hipMemcpyDeviceToDevice, l->stream);
    };
    for (int j = 0; j < 6; ++j) {
        const qc_dqn_layer& Y = layers[j];
        put(kFirst[j], Y.weight);
        put(kFirst[j] + 1, Y.bias);
        if (kNoisy[j]) {
            put(kFirst[j] + 2, Y.sigma_w);
            put(kFirst[j] + 3, Y.sigma_b);
        } else {
            put(kFirst[j] + 2, Y.weight_norm);
        }
    }
    const size_t pb = (size_t)l->np * sizeof(float);
    for (float* q : {l->E, l->V, l->MU, l->G})
        if (e == hipSuccess) e = hipMemsetAsync(q, 0, pb, l->stream);
    if (e != hipSuccess) return hip_fail(l->err, e, "learner parameter copy");
    hipLaunchKernelGGL(k_learner_prep, dim3(l->nprep, kPrepParts), dim3(1024), 0, l->stream, l->P, l->F, l->d_prep,
                       l->d_norm);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(l->err, e, "learner weight preparation");
    l->step = 0;
    l->l1 = l->l2 = 0.;
    l->backup_counter = 0;
    l->loaded = true;
    return QC_OK;
}

int qc_learner_layers(qc_learner* l, int target, qc_dqn_layer out[6]) {
    if (!l || !out) return QC_EINVAL;
    layer_views(l, target ? l->PT : l->P, out);
    return QC_OK;
}

int qc_learner_grads(qc_learner* l, qc_dqn_layer out[6]) {
    if (!l || !out) return QC_EINVAL;
    layer_views(l, l->G, out);
    return QC_OK;
}

int qc_learner_set_lr(qc_learner* l, double lr) {
    if (!l) return QC_EINVAL;
    if (!(lr >= 0.)) { l->err = "lr must be >= 0"; return QC_EINVAL; }
    l->lr = lr;
    return QC_OK;
}

int qc_learner_update(qc_learner* l, const float* transitions, const float* is_weights, const float* noise,
                      uint64_t counter, float* unweighted_loss, float* loss) {
    if (!l) return QC_EINVAL;
    if (!l->loaded) { l->err = "qc_learner_load has not been called"; return QC_EINVAL; }
    if (!transitions || !is_weights || !unweighted_loss) {
        l->err = "transitions, is_weights and unweighted_loss are required";
        return QC_EINVAL;
    }
    Dev g(l->device);
    int launches = 0;
    // the target network follows the online one every backup_period updates (RL.py:164-169)
    if (l->backup_counter == 0) {
        hipError_t e = hipMemcpyAsync(l->PT, l->P, (size_t)l->np * sizeof(float), hipMemcpyDeviceToDevice, l->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(l->FT, l->F, (size_t)l->nf_fwd * sizeof(float), hipMemcpyDeviceToDevice, l->stream);
        if (e != hipSuccess) return hip_fail(l->err, e, "target network copy");
        launches += 2;
    }
    l->backup_counter = (l->backup_counter + 1) % l->p.backup_period;

    const int B = l->B;
    {
        const int n = noise ? kChunks * l->noise_len : kChunks * ((l->noise_len + 1) / 2);
        hipLaunchKernelGGL(k_learner_noise, dim3((n + 255) / 256), dim3(256), 0, l->stream, noise, l->d_noise,
                           l->noise_len, l->p.seed, counter);
    }
    LArgs k = l->k;
    k.trans = transitions;
    const bool wide = l->w2 == kH2Wide;
    hipLaunchKernelGGL(fwd_kernel(l->w2, l->chunked), dim3(3 * B / kE), dim3(kThreads), kLdsFloats * sizeof(float),
                       l->stream, k);
    LossArgs s{};
    s.Q = k.Q; s.M = k.M; s.trans = transitions; s.w = is_weights; s.noise = l->d_noise;
    s.B = B; s.n_act = l->A; s.in_len = l->L; s.row_len = k.row_len; s.rpc = k.rpc;
    s.eps_out41 = l->w2 + 2 * kH3;
    s.omg = (float)(1. - l->p.gamma);
    s.gamma = (float)l->p.gamma;
    s.rew = (float)((1. - l->p.gamma) * l->p.alive_reward);
    s.failing = (float)l->p.failing_reward;
    s.inv_B = (float)(1. / B);
    s.inv_A = (float)(1. / l->A);
    s.dQ = k.dQ; s.dQe = k.dQe; s.dM = k.dM; s.ul = unweighted_loss; s.loss = l->d_loss; s.loss_user = loss;
    s.cnt = l->d_cnt;
    if (l->p.target_mode == QC_TD_REWARD_FAIL)
        hipLaunchKernelGGL(k_learner_loss<QC_TD_REWARD_FAIL>, dim3(1), dim3(1024), 0, l->stream, s);
    else if (l->p.target_mode == QC_TD_REWARD)
        hipLaunchKernelGGL(k_learner_loss<QC_TD_REWARD>, dim3(1), dim3(1024), 0, l->stream, s);
    else
        hipLaunchKernelGGL(k_learner_loss<QC_TD_ALIVE>, dim3(1), dim3(1024), 0, l->stream, s);
    if (wide)
        hipLaunchKernelGGL(k_learner_bwd<kH2Wide>, dim3(B / kE), dim3(kThreads), bwd_lds_floats(kH2Wide) * sizeof(float),
                           l->stream, k);
    else
        hipLaunchKernelGGL(k_learner_bwd<kH2>, dim3(B / kE), dim3(kThreads), bwd_lds_floats(kH2) * sizeof(float), l->stream, k);
    hipLaunchKernelGGL(k_learner_dw, dim3((l->ntiles + 3) / 4), dim3(kThreads), 0, l->stream, l->d_dwjobs, l->d_tiles,
                       l->ntiles, B);
    hipLaunchKernelGGL(k_learner_wndot, dim3(4), dim3(1024), 0, l->stream, l->P, l->G, l->wn_tensors, l->tt, l->d_dot);
    optimizer_and_prep(l, 1);
    launches += 8;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(l->err, e, "learner update launch");
    l->updates += 1;
    l->launches = launches;
    return QC_OK;
}

int qc_learner_apply(qc_learner* l, const qc_dqn_layer grads[6]) {
    if (!l || !grads) return QC_EINVAL;
    if (!l->loaded) { l->err = "qc_learner_load has not been called"; return QC_EINVAL; }
    Dev g(l->device);
    hipError_t e = hipSuccess;
    auto put = [&](int ti, const float* src) {
        const Tensor& T = l->tt.t[ti];
        if (!src) { l->err = "every gradient tensor is required"; e = hipErrorInvalidValue; return; }
        if (e == hipSuccess)
            e = hipMemcpyAsync(l->G + T.off, src, (size_t)T.n * sizeof(float), hipMemcpyDeviceToDevice, l->stream);
    };
    for (int j = 0; j < 6 && e == hipSuccess; ++j) {
        const qc_dqn_layer& Y = grads[j];
        put(kFirst[j], Y.weight);
        put(kFirst[j] + 1, Y.bias);
        if (kNoisy[j]) {
            put(kFirst[j] + 2, Y.sigma_w);
            put(kFirst[j] + 3, Y.sigma_b);
        } else {
            put(kFirst[j] + 2, Y.weight_norm);
        }
    }
    if (e == hipErrorInvalidValue) return QC_EINVAL;
    if (e != hipSuccess) return hip_fail(l->err, e, "learner gradient copy");
    optimizer_and_prep(l, 0);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(l->err, e, "learner optimizer launch");
    return QC_OK;
}

int qc_learner_stats(qc_learner* l, qc_learner_stats_t* out) {
    if (!l || !out) return QC_EINVAL;
    Dev g(l->device);
    int32_t cnt[2] = {0, 0};
    hipError_t e = hipStreamSynchronize(l->stream);
    if (e == hipSuccess) e = hipMemcpy(cnt, l->d_cnt, sizeof(cnt), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(l->err, e, "learner stats");
    out->updates = l->updates;
    out->step = l->step;
    out->backup_counter = l->backup_counter;
    out->launches_per_update = l->launches;
    out->l1 = l->l1;
    out->l2 = l->l2;
    out->lr = l->lr;
    out->nonfinite = cnt[0];
    if (cnt[1]) {
        // as qc_take_errors: report once, then clear the word
        const int32_t zero = 0;
        (void)hipMemcpy(l->d_cnt + 1, &zero, sizeof(zero), hipMemcpyHostToDevice);
        l->err = "an update since the last qc_learner_stats saw an action outside [0, n_actions) (clamped on the device)";
        return QC_EINVAL;
    }
    return QC_OK;
}

}  // extern "C"
