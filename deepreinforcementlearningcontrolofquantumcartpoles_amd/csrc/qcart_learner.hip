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
// launchers behind the kernels (qcart_learner.hpp). Behind those, LearnerCore's functions: the host side of the
// pipeline (create-time checks, tensor table, fragment and workspace layout, load, target sync, loss arguments,
// LaProp step, stats) that qc_learner below and qc_mlearner are both written in; each handle adds its own kernels.
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

// ---- LearnerCore's functions (qcart_learner.hpp): the host side both handles are written in ----
std::string bad_params(int max_batch, int batch_size, int backup_period, double lr, int target_mode, double beta1,
                       double beta2) {
    if (batch_size < 128 || batch_size > max_batch || batch_size % 128 != 0)
        return "batch_size must be a multiple of 128 in [128, " + std::to_string(max_batch) +
               "]: the learner implements FactorizedNoisy's 32-chunk noise branch (layers.py:57-74), not the per-row "
               "branch of other batch sizes";
    if (backup_period < 1) return "backup_period must be >= 1";
    if (!(lr >= 0.)) return "lr must be >= 0";
    if (target_mode != QC_TD_ALIVE && target_mode != QC_TD_REWARD_FAIL && target_mode != QC_TD_REWARD)
        return "target_mode must be QC_TD_ALIVE, QC_TD_REWARD_FAIL or QC_TD_REWARD";
    if (!(beta1 >= 0. && beta1 < 1.)) return "beta1 must be in [0, 1) (0: 0.9)";
    if (!(beta2 >= 0. && beta2 < 1.)) return "beta2 must be in [0, 1) (0: 0.9995)";
    return {};
}

void build_tensors(LearnerCore& c, int n, const int* O, const int* K, const bool* noisy, const bool* wnorm) {
    int off = 0;
    auto add = [&](int len, int kind, int wn, int w_off) {
        c.tt.t[c.nt++] = Tensor{off, len, kind, wn, w_off};
        off += (len + 3) & ~3;
    };
    c.n_layers = n;
    for (int j = 0; j < n; ++j) {
        c.O[j] = O[j]; c.K[j] = K[j]; c.noisy[j] = noisy[j]; c.wnorm[j] = wnorm[j];
        c.first[j] = c.nt;
        c.wn_of[j] = -1;
        if (noisy[j]) {
            add(O[j] * K[j], 0, -1, 0);
            add(O[j], 0, -1, 0);
            add(O[j] * K[j], 0, -1, 0);
            add(O[j], 0, -1, 0);
        } else if (wnorm[j]) {
            c.wn_of[j] = c.nwn;
            c.wn_tensors.t[c.nwn] = c.nt;
            const int w_off = off;
            add(O[j] * K[j], 1, c.nwn, w_off);
            add(O[j], 0, -1, 0);
            add(1, 2, c.nwn, w_off);
            ++c.nwn;
        } else {
            add(O[j] * K[j], 0, -1, 0);
            add(O[j], 0, -1, 0);
        }
    }
    c.np = off;
}

void build_tail_frags(LearnerCore& c, const int* Kpad, int j0, int fc2) {
    int fo = c.nf_fwd = host::frag_layout(c.n_layers, c.O, Kpad, c.noisy, c.u, c.s, c.ub, c.sb);
    FragOff& f = c.k.fo;
    for (int j = 0; j < 6; ++j) {
        const int l = fc2 - 1 + j;
        f.u[j] = c.u[l]; f.s[j] = c.s[l]; f.ub[j] = c.ub[l]; f.sb[j] = c.sb[l];
    }
    auto tfrag = [&](int j, int kpad) {   // fragments of W_j^T: [K_j rows][O_j pad kpad]
        const int at = fo;
        fo += tiles(c.K[j]) * ksteps(kpad) * 64;
        return at;
    };
    const int w2 = c.K[fc2 + 1];
    f.t2 = tfrag(fc2, w2);
    f.t31u = tfrag(fc2 + 1, kH3);
    f.t31s = tfrag(fc2 + 1, kH3);
    f.t41u = tfrag(fc2 + 2, 32);
    f.t41s = tfrag(fc2 + 2, 32);
    f.t32 = tfrag(fc2 + 3, kHM);
    f.w42 = fo; fo += kHM;
    c.nf = fo;

    for (int j = j0; j < c.n_layers; ++j) {
        const Tensor* T = &c.tt.t[c.first[j]];
        const int g_off = c.wnorm[j] ? T[2].off : -1;
        c.prep.push_back(PrepJob{T[0].off, g_off, c.wn_of[j], c.O[j], c.K[j], 0, Kpad[j], c.u[j], T[1].off, c.ub[j]});
        if (c.noisy[j])
            c.prep.push_back(PrepJob{T[2].off, -1, -1, c.O[j], c.K[j], 0, Kpad[j], c.s[j], T[3].off, c.sb[j]});
    }
    auto tjob = [&](int j, int sigma, int kpad, int out_off) {
        const Tensor* T = &c.tt.t[c.first[j]];
        c.prep.push_back(PrepJob{T[sigma ? 2 : 0].off, c.wnorm[j] ? T[2].off : -1, -1, c.O[j], c.K[j], 1, kpad, out_off, -1, -1});
    };
    tjob(fc2, 0, w2, f.t2);
    tjob(fc2 + 1, 0, kH3, f.t31u);
    tjob(fc2 + 1, 1, kH3, f.t31s);
    tjob(fc2 + 2, 0, 32, f.t41u);
    tjob(fc2 + 2, 1, 32, f.t41s);
    tjob(fc2 + 3, 0, kHM, f.t32);
    const Tensor* T42 = &c.tt.t[c.first[fc2 + 4]];
    c.prep.push_back(PrepJob{T42[0].off, T42[2].off, -1, 1, kHM, 2, kHM, f.w42, -1, -1});
}

// every feature-major array has its rows padded to 32 and its pad rows zero
size_t tail_workspace(LearnerCore& c, int w2, int in_len, float* W) {
    Carve take;
    auto at = [&](size_t n) {
        const size_t o = take(n);
        return W ? W + o : nullptr;
    };
    const size_t B = (size_t)c.B;
    LArgs& k = c.k;
    k.Q = at(3 * B * 32); k.M = at(3 * B);
    k.noise = c.d_noise = at((size_t)c.noise_len * kChunks);
    if (in_len) {
        k.X0 = at((size_t)tiles(in_len) * 32 * B);
        k.H1 = at(kH1 * B);
    }
    k.H2 = at(w2 * B); k.H2e = at(w2 * B); k.A3 = at(kH3 * B); k.A3e = at(kH3 * B); k.R32 = at(kHM * B);
    k.dQ = at(32 * B); k.dQe = at(32 * B); k.dM = at(32 * B);
    k.dZ3 = at(kH3 * B); k.dZ3e = at(kH3 * B); k.dZ32 = at(kHM * B); k.dZ2 = at(w2 * B);
    if (in_len) k.dZ1 = at(kH1 * B);
    c.d_loss = at(4);
    c.d_norm = at(kMaxWN);
    return take.w;
}

void free_all(LearnerCore& c) {
    for (void* q : c.allocs) (void)hipFree(q);
    c.allocs.clear();
}

hipError_t alloc_core(LearnerCore& c, int w2, int in_len, size_t ws_floats) {
    hipError_t e = hipSuccess;
    for (float** q : {&c.P, &c.PT, &c.G, &c.E, &c.V, &c.MU})
        if (e == hipSuccess) e = dalloc(c, q, (size_t)c.np);
    if (e == hipSuccess) e = dalloc(c, &c.F, (size_t)c.nf);
    if (e == hipSuccess) e = dalloc(c, &c.FT, (size_t)c.nf_fwd);
    if (e == hipSuccess) e = dalloc(c, &c.ws, ws_floats);
    if (e == hipSuccess) e = dalloc(c, &c.d_dot, 2 * kMaxWN);
    if (e == hipSuccess) e = dalloc(c, &c.d_cnt, 2);
    if (e == hipSuccess) e = dalloc(c, &c.d_prep, c.prep.size());
    if (e == hipSuccess) e = hipMemcpy(c.d_prep, c.prep.data(), c.prep.size() * sizeof(PrepJob), hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
    c.nprep = (int)c.prep.size();
    tail_workspace(c, w2, in_len, c.ws);
    c.k.F = c.F;
    c.k.FT = c.FT;
    c.k.n_act = c.A; c.k.B = c.B; c.k.rpc = c.B / kChunks;
    return hipSuccess;
}

hipError_t upload_dw(LearnerCore& c, const DwJob* jobs, int n) {
    std::vector<int4> tl;
    for (int j = 0; j < n; ++j)
        for (int to = 0; to < tiles(jobs[j].O); ++to)
            for (int tk = 0; tk < tiles(jobs[j].K); ++tk) tl.push_back(int4{j, to, tk, 0});
    c.ntiles = (int)tl.size();
    hipError_t e = dalloc(c, &c.d_dwjobs, (size_t)n);
    if (e == hipSuccess) e = hipMemcpy(c.d_dwjobs, jobs, n * sizeof(DwJob), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = dalloc(c, &c.d_tiles, tl.size());
    if (e == hipSuccess) e = hipMemcpy(c.d_tiles, tl.data(), tl.size() * sizeof(int4), hipMemcpyHostToDevice);
    return e;
}

void destroy_core(LearnerCore& c) {
    host::Dev g(c.device);
    (void)hipDeviceSynchronize();
    free_all(c);
}

void layer_views(const LearnerCore& c, const float* base, qc_dqn_layer* out) {
    for (int j = 0; j < c.n_layers; ++j) {
        const Tensor* T = &c.tt.t[c.first[j]];
        out[j] = qc_dqn_layer{base + T[0].off, base + T[1].off, c.wnorm[j] ? base + T[2].off : nullptr,
                              c.noisy[j] ? base + T[2].off : nullptr, c.noisy[j] ? base + T[3].off : nullptr};
    }
}

int set_lr(LearnerCore& c, double lr) {
    if (!(lr >= 0.)) { c.err = "lr must be >= 0"; return QC_EINVAL; }
    c.lr = lr;
    return QC_OK;
}

int set_backup_period(LearnerCore& c, int period) {
    if (period < 1) { c.err = "backup_period must be >= 1"; return QC_EINVAL; }
    c.backup_period = period;
    c.backup_counter %= period;
    return QC_OK;
}

namespace {
// the layers' tensors -> dst (the parameters or the gradients), device to device on the stream; stops at a missing
// tensor with hipErrorInvalidValue
hipError_t copy_in(LearnerCore& c, float* dst, const qc_dqn_layer* layers) {
    hipError_t e = hipSuccess;
    auto put = [&](int ti, const float* src) {
        const Tensor& T = c.tt.t[ti];
        if (e == hipSuccess)
            e = src ? hipMemcpyAsync(dst + T.off, src, (size_t)T.n * sizeof(float), hipMemcpyDeviceToDevice, c.stream)
                    : hipErrorInvalidValue;
    };
    for (int j = 0; j < c.n_layers; ++j) {
        const qc_dqn_layer& Y = layers[j];
        put(c.first[j], Y.weight);
        put(c.first[j] + 1, Y.bias);
        if (c.noisy[j]) {
            put(c.first[j] + 2, Y.sigma_w);
            put(c.first[j] + 3, Y.sigma_b);
        } else if (c.wnorm[j]) {
            put(c.first[j] + 2, Y.weight_norm);
        }
    }
    return e;
}

int not_loaded(LearnerCore& c) {
    c.err = std::string(c.name) + "_load has not been called";
    return QC_EINVAL;
}
}  // namespace

int load_core(LearnerCore& c, const qc_dqn_layer* layers) {
    host::Dev g(c.device);
    hipError_t e = copy_in(c, c.P, layers);
    const size_t pb = (size_t)c.np * sizeof(float);
    for (float* q : {c.E, c.V, c.MU, c.G})
        if (e == hipSuccess) e = hipMemsetAsync(q, 0, pb, c.stream);
    if (e != hipSuccess) return host::hip_fail(c.err, e, "learner parameter copy");
    launch_prep(c.stream, c.P, c.F, c.d_prep, c.nprep, c.d_norm);
    e = hipGetLastError();
    if (e != hipSuccess) return host::hip_fail(c.err, e, "learner weight preparation");
    c.step = 0;
    c.l1 = c.l2 = 0.;
    c.backup_counter = 0;
    c.loaded = true;
    return QC_OK;
}

int begin_update(LearnerCore& c, const float* transitions, const float* is_weights, const float* unweighted_loss,
                 const float* noise, uint64_t counter) {
    if (!c.loaded) return not_loaded(c);
    if (!transitions || !is_weights || !unweighted_loss) {
        c.err = "transitions, is_weights and unweighted_loss are required";
        return QC_EINVAL;
    }
    c.launches = 0;
    // the target network follows the online one every backup_period updates (RL.py:164-169)
    if (c.backup_counter == 0) {
        hipError_t e = hipMemcpyAsync(c.PT, c.P, (size_t)c.np * sizeof(float), hipMemcpyDeviceToDevice, c.stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(c.FT, c.F, (size_t)c.nf_fwd * sizeof(float), hipMemcpyDeviceToDevice, c.stream);
        if (e != hipSuccess) return host::hip_fail(c.err, e, "target network copy");
        c.launches = 2;
    }
    c.backup_counter = (c.backup_counter + 1) % c.backup_period;
    launch_noise(c.stream, noise, c.d_noise, c.noise_len, c.seed, counter);
    return QC_OK;
}

int end_update(LearnerCore& c, int n) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return host::hip_fail(c.err, e, "learner update launch");
    c.updates += 1;
    c.launches += n;
    return QC_OK;
}

LossArgs loss_args(const LearnerCore& c, const float* trans, int in_len, int w2, const float* is_weights,
                   float* unweighted_loss, float* loss) {
    const LArgs& k = c.k;
    LossArgs s{};
    s.Q = k.Q; s.M = k.M; s.trans = trans; s.w = is_weights; s.noise = c.d_noise;
    s.B = c.B; s.n_act = c.A; s.in_len = in_len; s.row_len = k.row_len; s.rpc = k.rpc;
    s.eps_out41 = w2 + 2 * kH3;
    s.omg = (float)(1. - c.gamma);
    s.gamma = (float)c.gamma;
    s.rew = (float)((1. - c.gamma) * c.alive_reward);
    s.failing = (float)c.failing_reward;
    s.inv_B = (float)(1. / c.B);
    s.inv_A = (float)(1. / c.A);
    s.dQ = k.dQ; s.dQe = k.dQe; s.dM = k.dM; s.ul = unweighted_loss; s.loss = c.d_loss; s.loss_user = loss;
    s.cnt = c.d_cnt;
    return s;
}

void opt_step(LearnerCore& c, int chain) {
    c.step += 1;
    c.l1 = c.l1 * c.b1 + (1 - c.b1) * c.lr;
    c.l2 = c.l2 * c.b2 + (1 - c.b2);
    OptArgs o{};
    o.P = c.P; o.G = c.G; o.E = c.E; o.V = c.V; o.MU = c.MU;
    o.dot = c.d_dot;
    o.norm = c.d_norm;
    o.chain = chain;
    o.centered = c.step > kCenteredAfter ? 1 : 0;
    o.beta1 = (float)c.b1;
    o.beta2 = (float)c.b2;
    o.omb2 = (float)(1 - c.b2);
    o.l2 = (float)c.l2;
    o.elr = (float)((1 - c.b1) * c.lr);
    o.step_size = (float)(c.lr != 0. ? 1. / (c.l1 / c.lr) : 1.);
    o.eps = (float)kEps;
    launch_opt(c.stream, o, c.tt, c.nt);
    launch_prep(c.stream, c.P, c.F, c.d_prep, c.nprep, c.d_norm);
}

int apply_core(LearnerCore& c, const qc_dqn_layer* grads) {
    if (!c.loaded) return not_loaded(c);
    host::Dev g(c.device);
    hipError_t e = copy_in(c, c.G, grads);
    if (e == hipErrorInvalidValue) { c.err = "every gradient tensor is required"; return QC_EINVAL; }
    if (e != hipSuccess) return host::hip_fail(c.err, e, "learner gradient copy");
    opt_step(c, 0);
    e = hipGetLastError();
    if (e != hipSuccess) return host::hip_fail(c.err, e, "learner optimizer launch");
    return QC_OK;
}

int stats_core(LearnerCore& c, qc_learner_stats_t* out) {
    host::Dev g(c.device);
    int32_t cnt[2] = {0, 0};
    hipError_t e = hipStreamSynchronize(c.stream);
    if (e == hipSuccess) e = hipMemcpy(cnt, c.d_cnt, sizeof(cnt), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return host::hip_fail(c.err, e, "learner stats");
    out->updates = c.updates;
    out->step = c.step;
    out->backup_counter = c.backup_counter;
    out->launches_per_update = c.launches;
    out->l1 = c.l1;
    out->l2 = c.l2;
    out->lr = c.lr;
    out->nonfinite = cnt[0];
    if (cnt[1]) {
        // as qc_take_errors: report once, then clear the word
        const int32_t zero = 0;
        (void)hipMemcpy(c.d_cnt + 1, &zero, sizeof(zero), hipMemcpyHostToDevice);
        c.err = std::string("an update since the last ") + c.name +
                "_stats saw an action outside [0, n_actions) (clamped on the device)";
        return QC_EINVAL;
    }
    return QC_OK;
}

// ---- exported state ----
namespace {
// the payload's head; the device buffers follow in state_parts' order
struct StateHead {
    int64_t updates, step;
    double lr, l1, l2;
    int32_t backup_counter;
    int32_t backup_period_set;   // the period in use where set_backup_period changed it, else 0 (as every earlier blob)
    int32_t cnt[2];   // d_cnt: non-finite losses, the out-of-range-action flag
};
struct StatePart {
    void* p;
    size_t bytes;
};
// F, FT and d_norm are saved as they are: a copy is bitwise by construction, whereas rebuilding them would run
// k_learner_prep (and the measurement learner's own preparation behind it) on P and on PT
int state_parts(const LearnerCore& c, StatePart* out) {
    const size_t pb = (size_t)c.np * sizeof(float);
    int n = 0;
    for (float* q : {c.P, c.PT, c.E, c.V, c.MU}) out[n++] = StatePart{q, pb};
    out[n++] = StatePart{c.F, (size_t)c.nf * sizeof(float)};
    out[n++] = StatePart{c.FT, (size_t)c.nf_fwd * sizeof(float)};
    out[n++] = StatePart{c.d_norm, kMaxWN * sizeof(float)};
    return n;
}
uint64_t state_payload(const LearnerCore& c) {
    StatePart part[8];
    const int n = state_parts(c, part);
    uint64_t b = sizeof(StateHead);
    for (int i = 0; i < n; ++i) b += part[i].bytes;
    return b;
}
}  // namespace

void put_core_fields(const LearnerCore& c, state::Header& h) {
    state::put_i(h, "n_actions", c.A);
    state::put_i(h, "batch_size", c.B);
    state::put_i(h, "backup_period", c.backup_period0);
    state::put_i(h, "target_mode", c.target_mode);
    state::put_f(h, "gamma", c.gamma);
    state::put_f(h, "alive_reward", c.alive_reward);
    state::put_f(h, "failing_reward", c.failing_reward);
    state::put_f(h, "beta1", c.b1);
    state::put_f(h, "beta2", c.b2);
    state::put_u(h, "seed", c.seed);
    state::put_i(h, "param_floats", c.np);
    state::put_i(h, "fragment_floats", c.nf);
    state::put_i(h, "target_frag_floats", c.nf_fwd);
    h.payload_bytes = state_payload(c);
}

int state_bytes_core(LearnerCore& c, uint64_t* n) {
    host::Dev g(c.device);
    const hipError_t e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) return host::hip_fail(c.err, e, "learner state_bytes");
    *n = sizeof(state::Header) + state_payload(c);
    return QC_OK;
}

int state_export_core(LearnerCore& c, state::Header h, void* host_dst, uint64_t n) {
    if (!c.loaded) {
        c.err = std::string(c.name) + "_state_export: " + c.name + "_load has not been called: there is no state to save";
        return QC_EINVAL;
    }
    if (n != sizeof(state::Header) + h.payload_bytes) {
        c.err = std::string(c.name) + "_state_export: n is " + std::to_string(n) + ", " + c.name + "_state_bytes gives " +
                std::to_string(sizeof(state::Header) + h.payload_bytes);
        return QC_EINVAL;
    }
    host::Dev g(c.device);
    StateHead s{};
    s.updates = c.updates; s.step = c.step;
    s.lr = c.lr; s.l1 = c.l1; s.l2 = c.l2;
    s.backup_counter = c.backup_counter;
    s.backup_period_set = c.backup_period != c.backup_period0 ? c.backup_period : 0;
    hipError_t e = hipStreamSynchronize(c.stream);
    if (e == hipSuccess) e = hipMemcpy(s.cnt, c.d_cnt, sizeof(s.cnt), hipMemcpyDeviceToHost);
    std::memcpy(host_dst, &h, sizeof(h));
    state::Cursor cur(host_dst);
    std::memcpy(cur.take(sizeof(s)), &s, sizeof(s));
    StatePart part[8];
    const int np = state_parts(c, part);
    for (int i = 0; i < np; ++i) {
        unsigned char* at = cur.take(part[i].bytes);
        if (e == hipSuccess) e = hipMemcpy(at, part[i].p, part[i].bytes, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) return host::hip_fail(c.err, e, "learner state export");
    return QC_OK;
}

int state_import_core(LearnerCore& c, const state::Header& mine, const void* host_src, uint64_t n) {
    state::Header h;
    std::string bad = state::validate(host_src, n, mine, &h);
    if (bad.empty() && h.payload_bytes != mine.payload_bytes)
        bad = std::string(c.name) + "_state_import: payload_bytes: blob " + std::to_string(h.payload_bytes) +
              ", handle " + std::to_string(mine.payload_bytes);
    StateHead s{};
    if (bad.empty()) {
        std::memcpy(&s, (const unsigned char*)host_src + sizeof(state::Header), sizeof(s));
        const std::string who = std::string(c.name) + "_state_import: ";
        const int period = s.backup_period_set > 0 ? s.backup_period_set : c.backup_period0;
        if (s.backup_period_set < 0)
            bad = who + "backup_period in use: blob " + std::to_string(s.backup_period_set) + ", expected >= 0";
        else if (s.backup_counter < 0 || s.backup_counter >= period)
            bad = who + "backup_counter: blob " + std::to_string(s.backup_counter) + ", handle's backup_period " +
                  std::to_string(period);
        else if (s.step < 0 || s.updates < 0)
            bad = who + "step / updates: blob " + std::to_string(s.step) + " / " + std::to_string(s.updates) +
                  ", expected >= 0";
        else if (!(s.lr >= 0.))
            bad = who + "lr: blob " + std::to_string(s.lr) + ", expected >= 0";
    }
    if (!bad.empty()) {
        c.err = bad;
        return QC_EINVAL;
    }
    host::Dev g(c.device);
    hipError_t e = hipStreamSynchronize(c.stream);
    state::Cursor cur(const_cast<void*>(host_src));
    cur.take(sizeof(s));
    StatePart part[8];
    const int np = state_parts(c, part);
    for (int i = 0; i < np; ++i) {
        const unsigned char* at = cur.take(part[i].bytes);
        if (e == hipSuccess) e = hipMemcpy(part[i].p, at, part[i].bytes, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMemcpy(c.d_cnt, s.cnt, sizeof(s.cnt), hipMemcpyHostToDevice);
    // the gradients of the last update are introspection only (every update writes all of G before it reads it)
    if (e == hipSuccess) e = hipMemsetAsync(c.G, 0, (size_t)c.np * sizeof(float), c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) return host::hip_fail(c.err, e, "learner state import");
    c.updates = s.updates; c.step = s.step;
    c.lr = s.lr; c.l1 = s.l1; c.l2 = s.l2;
    c.backup_counter = s.backup_counter;
    c.backup_period = s.backup_period_set > 0 ? s.backup_period_set : c.backup_period0;
    c.loaded = true;
    return QC_OK;
}

}  // namespace learner
}  // namespace qcart

using namespace qcart::learner;
using namespace qcart::host;

// the direct learner's own: which k_learner_fwd / k_learner_bwd it runs
struct qc_learner : LearnerCore {
    int in_pad = 0;
    int w2 = kH2;             // fc2's width: the instantiation of k_learner_fwd / k_learner_bwd
    bool chunked = false;     // data_length above kChunkIn: k_learner_fwd<w2 + kChunkTag>
};

namespace {
CreateError g_learner_err;

using Kernel = void (*)(const LArgs);
Kernel fwd_kernel(int w2, bool chunked) {
    if (chunked) return w2 == kH2Wide ? k_learner_fwd<kH2Wide + kChunkTag> : k_learner_fwd<kH2 + kChunkTag>;
    return w2 == kH2Wide ? k_learner_fwd<kH2Wide> : k_learner_fwd<kH2>;
}
Kernel bwd_kernel(int w2) { return w2 == kH2Wide ? k_learner_bwd<kH2Wide> : k_learner_bwd<kH2>; }

// fc1, fc2, fc31, fc41, fc32, fc42: 3 + 3 + 4 + 4 + 3 + 3 = 20 parameter tensors, four weight-normalised layers
constexpr bool kNoisy[6] = {false, false, true, true, false, false};
constexpr bool kWnorm[6] = {true, true, false, false, true, true};
constexpr LayerRule kLearnerRules[] = {
    {0b001100, states_where([](bool wn, bool sw, bool sb) { return !sw || !sb || wn; }),
     "fc31 / fc41 are FactorizedNoisy layers (sigma_w and sigma_b, no weight_norm): the learner "
     "implements direct_DQN(noisy_layers=2)"},
    {0b110011, states_where([](bool wn, bool sw, bool sb) { return !wn || sw || sb; }),
     "fc1 / fc2 / fc32 / fc42 are Linear_weight_normalize layers (weight_norm, no sigma)"},
};
}  // namespace

extern "C" {

int qc_learner_create(const qc_learner_params* p, int device, qc_learner** out) {
    if (!out || !p) return QC_EINVAL;
    *out = nullptr;
    auto fail = [](const std::string& m, int rc) { return g_learner_err.fail(m, rc); };
    if (const char* m = bad_net_size(p->data_length, p->n_actions)) return fail(m, QC_EINVAL);
    const int w2 = fc2_width(p->hidden2);
    if (!w2) return fail("hidden2 must be 0, 256 or 512 (fc2's width)", QC_EINVAL);
    const std::string bad =
        bad_params(4096, p->batch_size, p->backup_period, p->lr, p->target_mode, p->beta1, p->beta2);
    if (!bad.empty()) return fail(bad, QC_EINVAL);
    if (const int rc = check_device(device, g_learner_err, "the learner")) return rc;

    qc_learner* l = new qc_learner();
    const int L = p->data_length, A = p->n_actions;
    take_params(*l, "qc_learner", *p, device, noise_len(w2, A));
    l->in_pad = in_pad(L);
    l->w2 = w2;
    l->chunked = l->in_pad > kChunkIn;

    const int O[6] = {kH1, w2, kH3, A, kHM, 1};
    const int K[6] = {L, kH1, w2, kH3, w2, kHM};
    const int Kp[6] = {l->in_pad, kH1, w2, kH3, w2, kHM};
    build_tensors(*l, 6, O, K, kNoisy, kWnorm);
    build_tail_frags(*l, Kp, 0, 1);

    Dev g(device);
    if (alloc_core(*l, w2, L, tail_workspace(*l, w2, L, nullptr)) != hipSuccess) {
        free_all(*l);
        delete l;
        return fail("device allocation failed", QC_ENOMEM);
    }
    LArgs& k = l->k;
    k.in_len = L; k.in_pad = l->in_pad; k.row_len = 2 * L + 2;

    // ---- the dW jobs (dY, X, gradient tensor, bias gradient tensor)
    auto gt = [&](int j, int i) { return l->G + l->tt.t[l->first[j] + i].off; };
    const DwJob jobs[8] = {
        {k.dZ1, k.X0, gt(0, 0), gt(0, 1), kH1, L},       {k.dZ2, k.H1, gt(1, 0), gt(1, 1), w2, kH1},
        {k.dZ3, k.H2, gt(2, 0), gt(2, 1), kH3, w2},      {k.dZ3e, k.H2e, gt(2, 2), gt(2, 3), kH3, w2},
        {k.dQ, k.A3, gt(3, 0), gt(3, 1), A, kH3},        {k.dQe, k.A3e, gt(3, 2), gt(3, 3), A, kH3},
        {k.dZ32, k.H2, gt(4, 0), gt(4, 1), kHM, w2},     {k.dM, k.R32, gt(5, 0), gt(5, 1), 1, kHM},
    };
    hipError_t e = upload_dw(*l, jobs, 8);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)fwd_kernel(w2, l->chunked), hipFuncAttributeMaxDynamicSharedMemorySize,
                                kLdsFloats * (int)sizeof(float));
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)bwd_kernel(w2), hipFuncAttributeMaxDynamicSharedMemorySize,
                                bwd_lds_floats(w2) * (int)sizeof(float));
    if (e != hipSuccess) {
        free_all(*l);
        delete l;
        return fail("device setup failed (job tables / LDS size of the learner kernels)", QC_EHIP);
    }
    *out = l;
    return QC_OK;
}

void qc_learner_destroy(qc_learner* l) {
    if (!l) return;
    destroy_core(*l);
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
    return load_core(*l, layers);
}

int qc_learner_layers(qc_learner* l, int target, qc_dqn_layer out[6]) {
    if (!l || !out) return QC_EINVAL;
    layer_views(*l, target ? l->PT : l->P, out);
    return QC_OK;
}

int qc_learner_grads(qc_learner* l, qc_dqn_layer out[6]) {
    if (!l || !out) return QC_EINVAL;
    layer_views(*l, l->G, out);
    return QC_OK;
}

int qc_learner_set_lr(qc_learner* l, double lr) { return l ? set_lr(*l, lr) : QC_EINVAL; }
int qc_learner_set_backup_period(qc_learner* l, int32_t period) { return l ? set_backup_period(*l, period) : QC_EINVAL; }

int qc_learner_update(qc_learner* l, const float* transitions, const float* is_weights, const float* noise,
                      uint64_t counter, float* unweighted_loss, float* loss) {
    if (!l) return QC_EINVAL;
    Dev g(l->device);
    if (const int rc = begin_update(*l, transitions, is_weights, unweighted_loss, noise, counter)) return rc;
    const int B = l->B;
    hipStream_t s = l->stream;
    LArgs k = l->k;
    k.trans = transitions;
    hipLaunchKernelGGL(fwd_kernel(l->w2, l->chunked), dim3(3 * B / kE), dim3(kThreads), kLdsFloats * sizeof(float), s, k);
    launch_loss(s, l->target_mode, loss_args(*l, transitions, k.in_len, l->w2, is_weights, unweighted_loss, loss));
    hipLaunchKernelGGL(bwd_kernel(l->w2), dim3(B / kE), dim3(kThreads), bwd_lds_floats(l->w2) * sizeof(float), s, k);
    launch_dw(s, l->d_dwjobs, l->d_tiles, l->ntiles, B);
    launch_wndot(s, l->nwn, l->P, l->G, l->wn_tensors, l->tt, l->d_dot);
    opt_step(*l, 1);
    return end_update(*l, 8);
}

int qc_learner_apply(qc_learner* l, const qc_dqn_layer grads[6]) { return l && grads ? apply_core(*l, grads) : QC_EINVAL; }

int qc_learner_stats(qc_learner* l, qc_learner_stats_t* out) { return l && out ? stats_core(*l, out) : QC_EINVAL; }

static qcart::state::Header learner_header(const qc_learner& l) {
    qcart::state::Header h = qcart::state::make(qcart::state::kLearner);
    qcart::state::put_i(h, "data_length", l.k.in_len);
    qcart::state::put_i(h, "hidden2", l.w2);
    put_core_fields(l, h);
    return h;
}

int qc_learner_state_bytes(qc_learner* l, uint64_t* n) { return l && n ? state_bytes_core(*l, n) : QC_EINVAL; }

int qc_learner_state_export(qc_learner* l, void* host_dst, uint64_t n) {
    return l && host_dst ? state_export_core(*l, learner_header(*l), host_dst, n) : QC_EINVAL;
}

int qc_learner_state_import(qc_learner* l, const void* host_src, uint64_t n) {
    return l ? state_import_core(*l, learner_header(*l), host_src, n) : QC_EINVAL;
}

}  // extern "C"
