// qcart_mlearner.hip — the device learner of the measurement-input network: the reference's TrainDQN.__call__
// (inverted harmonic oscillator/RL.py:159-232) for DQN_measurement (RL.py:29-78) with centred LaProp, one
// update per call on a batch of B replay rows (qc_record's layout), fp32 throughout. The convolutions are plain
// Conv1d layers (the inverted harmonic driver's net) or, on a handle created with conv_weight_norm = 1,
// Conv1d_weight_normalize layers (the harmonic driver's, harmonic oscillator/RL.py:29-75, layers.py:86-94):
// effective weight W g / ||W||_F with one scalar g per layer.
//
// The forward stack is the measurement actor's (k_mconv / k_mtr / k_mfc, qcart_actor.hip); the tail, the loss, the
// dense weight gradients, the optimizer and the dense fragment preparation are the direct learner's kernels
// (qcart_learner.hip) driven through qcart_learner.hpp. New here: the state assembly, the backward of fc1 and
// of the convolutions (all GEMMs on v_mfma_f32_32x32x2_f32, exact fp32), the split-K reduction and the
// convolutions' fragment preparation. The host side is LearnerCore's (qcart_learner.hpp: checks, tensor table,
// the tail's fragments and workspace, load, target sync, loss arguments, LaProp step, stats); qc_mlearner adds
// the geometry, the convolutional stack's buffers and job tables, and launches k_mlearner_prep itself behind
// every shared fragment preparation.
//
// Launches per update (plain launches on the handle's stream; no atomic touches a gradient):
//    1 k_learner_noise     the 32 chunks' noise
//    2 k_mlearner_states   rows -> X [2B][2][L]: next states, then previous states
//    3-7   k_mconv x3, k_mtr, k_mfc   online net on the 2B states
//    8-12  the same               target net on the B next states
//   13 k_mtr               the previous states' y3 -> feature-major [64 T3][B] (fc1's dW operand, fc1^T's mask)
//   14 k_learner_fwd<256, true>   the tail's three passes (fc21, fc31, fc22, fc32) from relu(fc1)
//   15 k_learner_loss
//   16 k_learner_bwd<256, true>   the tail's backward down to dZ2
//   17 k_mlearner_fc1t     dY3 = W_fc1^T dZ2, masked by y3 > 0, env-major and zero-padded
//   18 k_mlearner_convt    conv3^T: dY2, masked by y2 > 0
//   19 k_mlearner_convt    conv2^T: dY1, masked by y1 > 0
//   20-22 k_mlearner_convdw   split-K partial dW / db of conv3, conv2, conv1
//   23 k_mlearner_reduce   fixed-order sum of the partials
//   24 k_learner_dw        fc1 and the tail
//   25 k_learner_wndot     fc22, fc32
//   26 k_learner_opt       22 tensors
//   27 k_learner_prep      fc1, fc1^T, the tail's fragments
//   28 k_mlearner_prep     the convolutions' forward and per-phase transposed fragments
// and two device-to-device copies (parameters, forward fragments) when the target network follows the online one.
//
// A weight-normalised handle takes the same 28 launches. Three more jobs of k_learner_prep (27) write each
// convolution's effective weight W g / ||W||_F in the natural layout (its plain scaled copy, mode 2) and the fp64
// norm; k_mlearner_prep (28) builds its fragments from those instead of from the parameters, so the forward
// stack, the transposed convolutions and, through the copy of the forward fragments, the target net all see
// effective weights. The convolutions' dW (20-23) is then the gradient G of the effective weight:
// k_learner_wndot (25) takes <G, W> of five layers, and k_learner_opt (26, 25 tensors) applies the chain rule
// dW = (g / n)(G - <G, W> W / n^2), dg = <G, W> / n as it does for fc22 / fc32.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/qcart.h"
#include "qcart_dqn.hpp"
#include "qcart_host.hpp"
#include "qcart_learner.hpp"

namespace qcart {
namespace mlearner {

using namespace qcart::dqn;
using namespace qcart::learner;

constexpr int kPad = 2;   // leading zeros of a padded dY row: the transposed convolutions read t = q - i, i <= 2

// replay rows -> the network inputs (RL.py:180-192): X [2B][2][L], env b's next state at b, its previous state
// at B + b. Pure copies; every row element is read once (the K + 1 forces through LDS)
__global__ __launch_bounds__(256) void k_mlearner_states(const float* __restrict__ tr, float* __restrict__ X, int L,
                                                         int m, int K, int row_len, int B) {
    extern __shared__ float f[];
    const int b = blockIdx.x;
    const float* row = tr + (size_t)b * row_len;
    float* nx = X + (size_t)b * 2 * L;
    float* pv = X + (size_t)(B + b) * 2 * L;
    for (int i = threadIdx.x; i <= K; i += 256) f[i] = row[L + m + i];
    for (int i = threadIdx.x; i < L + m; i += 256) {
        const float v = row[i];
        if (i < L) nx[i] = v;
        if (i >= m) pv[i - m] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < L; i += 256) {
        const int k = i / m;
        nx[L + i] = f[k];
        pv[L + i] = f[k + 1];
    }
}

// fc1^T: dY3[f][b] = sum_o W_fc1[o][f] dZ2[o][b] (M = 64 T3, K = 256, N = B), masked by y3 > 0. A = the
// fragments of W_fc1^T, B = a 32-column block of dZ2 in LDS (32 KiB), one wave per output tile (two tiles per
// wave and workgroup). Written env-major and zero-padded, dY3 [b][co][kPad + t], as conv3^T and conv3's dW read it
__global__ __launch_bounds__(kThreads) void k_mlearner_fc1t(const float* __restrict__ Wt, const float* __restrict__ dZ2,
                                                            const float* __restrict__ y3p, float* __restrict__ dY3,
                                                            int T3, int Tp3, int flat, int B) {
    __shared__ __attribute__((aligned(16))) float D2[kH2 * kE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e0 = blockIdx.x * kE, eg = e0 + (lane & 31);
    for (int i = tid; i < kH2 * kE; i += kThreads) D2[i] = dZ2[(size_t)(i / kE) * B + e0 + i % kE];
    __syncthreads();
    const int S = ksteps(kH2);
#pragma unroll 1
    for (int j = 0; j < 2; ++j) {
        const int t = (blockIdx.y * 2 + j) * 4 + wave;
        if (t >= tiles(flat)) continue;
        f32x16 acc = {};
        gemm_tile(acc, Wt + (size_t)t * S * 64, D2, S, lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = t * 32 + drow(r, lane);   // < flat: flat is a multiple of 64
            const int co = f / T3, tt = f - co * T3;
            const float g = y3p[(size_t)f * B + eg] > 0.f ? acc[r] : 0.f;
            dY3[((size_t)eg * 64 + co) * Tp3 + kPad + tt] = g;
        }
    }
}

// Transposed convolution: dX[b][ci][s] = sum_co sum_{j : s = S t + j} W[co][ci][j] dY[b][co][t], masked by the
// stored activation X > 0. Input positions of one phase p = s mod S share their taps j = p + S i, so per phase
// it is a GEMM: M = ci, N = (b, q) with s = S q + p, K = (i, co), t = q - i. blockIdx.y = phase; a wave takes
// 32 columns and all CI / 32 row tiles. A = per-phase fragments (k_mlearner_prep; taps j >= KS are zero
// fragments), B = dY gathered per lane from its zero-padded rows [b][co][kPad + t]: every load is
// unconditional, t outside [0, Tout) reads padding, so positions no output window covers get exact zeros.
// Columns past the end read env 0 and are not stored. dX is written zero-padded too (the next layer's dY)
template <int CI, int CO, int KS, int S>
__global__ __launch_bounds__(kThreads) void k_mlearner_convt(const float* __restrict__ dY, const float* __restrict__ Wt,
                                                             const float* __restrict__ X, float* __restrict__ dX, int Tin,
                                                             int Tpo, int Tpi, int Qn, int64_t n_total) {
    constexpr int MT = CI / 32, NI = (KS + S - 1) / S, STEPS = NI * CO / 2;
    static_assert(CO % 2 == 0 && CI % 32 == 0, "k-step pairs co, co + 1 of one tap");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hi = lane >> 5;
    const int p = blockIdx.y;
    const int64_t n = ((int64_t)blockIdx.x * 4 + wave) * 32 + (lane & 31);
    const bool ok = n < n_total;
    const int64_t b = ok ? n / Qn : 0;
    const int q = ok ? (int)(n - b * Qn) : 0;
    const float* yl = dY + ((size_t)b * CO + hi) * Tpo + kPad + q;
    const float* wl = Wt + (size_t)p * MT * STEPS * 64 + lane;
    f32x16 acc[2][MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[0][m] = acc[1][m] = f32x16{};
    constexpr int U = 8;
    static_assert(STEPS % U == 0, "whole batches");
    for (int s0 = 0; s0 < STEPS; s0 += U) {
        float x[U], w[U][MT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = 2 * (s0 + u), i = k / CO, co = k - i * CO;   // k = i CO + co; the lane halves: co, co + 1
            x[u] = yl[co * Tpo - i];
#pragma unroll
            for (int m = 0; m < MT; ++m) w[u][m] = wl[(size_t)(m * STEPS + s0 + u) * 64];
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int m = 0; m < MT; ++m)
                acc[u & 1][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[u][m], x[u], acc[u & 1][m], 0, 0, 0);
    }
    const int sp = S * q + p;
    if (!ok || sp >= Tin) return;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const f32x16 a = acc[0][m] + acc[1][m];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ci = m * 32 + drow(r, lane);
            const float xv = X[((size_t)b * CI + ci) * Tin + sp];
            dX[((size_t)b * CI + ci) * Tpi + kPad + sp] = xv > 0.f ? a[r] : 0.f;
        }
    }
}

// Convolution weight gradient, split-K: dW[co][ci][j] = sum_{b, t} dY[b][co][t] X[b][ci][S t + j] and
// db[co] = sum_{b, t} dY[b][co][t]: M = co, N = (ci, j), K = (b, t). A chunk of K is epc envs x a segment of
// tl positions; a wave computes one 32 x 32 tile of one chunk's partial sum (the lane halves take two envs of
// a pair, so an MFMA k-step is one position t of both) and writes it to part [chunk][co][ci KS] /
// partb [chunk][co]; k_mlearner_reduce sums the chunks in a fixed order
template <int CI, int CO, int KS, int S>
__global__ __launch_bounds__(kThreads) void k_mlearner_convdw(const float* __restrict__ dY, const float* __restrict__ X,
                                                              float* __restrict__ part, float* __restrict__ partb,
                                                              int Tin, int Tout, int Tpo, int epc, int tl, int nseg,
                                                              int nwaves) {
    constexpr int NCOL = CI * KS, NTL = (NCOL + 31) / 32, MTL = CO / 32;
    const int lane = threadIdx.x & 63, hi = lane >> 5;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nwaves) return;
    const int chunk = w / (MTL * NTL), rem = w - chunk * (MTL * NTL), mt = rem / NTL, nt = rem - mt * NTL;
    const int eb = chunk / nseg, seg = chunk - eb * nseg;
    const int t0 = seg * tl, t1 = min(Tout, t0 + tl);
    const int col = nt * 32 + (lane & 31);
    const bool col_ok = col < NCOL;
    const int ci = col_ok ? col / KS : 0, j = col_ok ? col - ci * KS : 0;
    const int co = mt * 32 + (lane & 31);
    f32x16 acc0 = {}, acc1 = {};
    float rs = 0.f;
    for (int pr = 0; pr < epc / 2; ++pr) {
        const size_t b = (size_t)eb * epc + 2 * pr + hi;
        const float* ap = dY + (b * CO + co) * Tpo + kPad;
        const float* xp = X + (b * CI + ci) * Tin + j;
        int t = t0;
        for (; t + 4 <= t1; t += 4) {
            const float a0 = ap[t], a1 = ap[t + 1], a2 = ap[t + 2], a3 = ap[t + 3];
            const float x0 = xp[S * t], x1 = xp[S * (t + 1)], x2 = xp[S * (t + 2)], x3 = xp[S * (t + 3)];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, x0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, x1, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, x2, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, x3, acc1, 0, 0, 0);
            rs += (a0 + a1) + (a2 + a3);
        }
        for (; t < t1; ++t) {
            const float a0 = ap[t];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, xp[S * t], acc0, 0, 0, 0);
            rs += a0;
        }
    }
    acc0 += acc1;
    rs += __shfl_xor(rs, 32, 64);
    if (nt == 0 && hi == 0) partb[(size_t)chunk * CO + co] = rs;
    if (!col_ok) return;
#pragma unroll
    for (int r = 0; r < 16; ++r)
        part[((size_t)chunk * CO + mt * 32 + drow(r, lane)) * NCOL + col] = acc0[r];
}

// out[e] = sum_c part[c][e] in one fixed order: a workgroup takes 32 gradient elements x 8 slices of the chunk
// range; a slice sums its chunks ascending, then slice 0's threads add the 8 slice sums ascending (through LDS)
struct RedJob {
    const float* part;
    float* out;
    int n, nchunks;
};
struct RedJobs {
    RedJob j[6];
    int first_block[7];
};
constexpr int kRedSlices = 8;
__global__ __launch_bounds__(256) void k_mlearner_reduce(const RedJobs J) {
    __shared__ float sl[kRedSlices][32];
    int k = 0;
    while (k < 5 && (int)blockIdx.x >= J.first_block[k + 1]) ++k;
    const RedJob R = J.j[k];
    const int x = threadIdx.x & 31, q = threadIdx.x >> 5;
    const int e = ((int)blockIdx.x - J.first_block[k]) * 32 + x;
    float s = 0.f;
    if (e < R.n) {
        const int c0 = (int)((int64_t)q * R.nchunks / kRedSlices), c1 = (int)((int64_t)(q + 1) * R.nchunks / kRedSlices);
#pragma unroll 4
        for (int c = c0; c < c1; ++c) s += R.part[(size_t)c * R.n + e];
    }
    sl[q][x] = s;
    __syncthreads();
    if (q != 0 || e >= R.n) return;
    float t = sl[0][x];
#pragma unroll
    for (int i = 1; i < kRedSlices; ++i) t += sl[i][x];
    R.out[e] = t;
}

// the convolutions' fragments from the natural-layout weights W [CO][CI][KS]:
//   mode 0  forward, the measurement actor's layout (k_actor_prep, split = 1) and the bias padded to tiles * 32
//   mode 1  transposed, per phase p: the matrix [ci][k = i CO + co] = W[co][ci][p + S i] (0 where p + S i >= KS)
//           in k-step pairs (2 s, 2 s + 1): [p][ci tile][step][64]
// Wb + w_off: the weights the fragments are made of, the parameters themselves (Wb = P) or, on a weight-normalised
// handle, the effective weights k_learner_prep has just written behind the fragments (Wb = F); the biases are P's
struct ConvPrepJob {
    int w_off, bias_off, out_off, bias_pad_off;
    int CO, CI, KS, S, mode, n;   // n: fragment floats
};
struct ConvPrepJobs {
    ConvPrepJob j[5];
};
__global__ __launch_bounds__(256) void k_mlearner_prep(const float* __restrict__ P, const float* Wb, float* F,
                                                       const ConvPrepJobs jobs) {
    const ConvPrepJob J = jobs.j[blockIdx.y];
    const float* W = Wb + J.w_off;
    const int K = J.CI * J.KS;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < J.n; i += gridDim.x * 256) {
        float v = 0.f;
        if (J.mode == 0) {
            int o, k;
            frag_ok(i, K / 2, 1, o, k);
            if (o < J.CO && k < K) v = W[(size_t)o * K + k];
        } else {
            const int NI = (J.KS + J.S - 1) / J.S, steps = NI * J.CO / 2, MT = J.CI / 32;
            const int l = i & 63, s = (i >> 6) % steps, m = ((i >> 6) / steps) % MT, p = (i >> 6) / (steps * MT);
            const int ci = m * 32 + (l & 31), k = 2 * s + (l >> 5), it = k / J.CO, co = k - it * J.CO;
            const int tap = p + J.S * it;
            if (tap < J.KS) v = W[((size_t)co * J.CI + ci) * J.KS + tap];
        }
        F[J.out_off + i] = v;
    }
    if (J.mode == 0)
        for (int i = blockIdx.x * 256 + threadIdx.x; i < tiles(J.CO) * 32; i += gridDim.x * 256)
            F[J.bias_pad_off + i] = i < J.CO ? P[J.bias_off + i] : 0.f;
}

}  // namespace mlearner
}  // namespace qcart

using namespace qcart::mlearner;
using namespace qcart::host;

namespace {
// parameter tensors: 6 conv, 2 fc1, 4 + 4 noisy, 3 + 3 weight-normalised = 22; a weight-normalised convolution
// stack adds one g per convolution: 25 (LearnerCore::nt). The layers are conv1, conv2, conv3, fc1, fc21, fc31,
// fc22, fc32
constexpr int kC[3] = {32, 64, 64}, kCI[3] = {2, 32, 64}, kKS[3] = {13, 11, 9}, kS[3] = {5, 4, 4};
constexpr bool kNoisy[8] = {false, false, false, false, true, true, false, false};
constexpr bool kWnormTail[8] = {false, false, false, false, false, false, true, true};
const char* const kName[8] = {"conv1", "conv2", "conv3", "fc1", "fc21", "fc31", "fc22", "fc32"};
int conv_out(int n, int k, int s) { return (n - (k - 1) + (s - 1)) / s; }   // calculate_next_layer_dim (RL.py:49-50)
}  // namespace

// the measurement learner's own: the geometry, the convolutional stack's activations, gradients and job tables
struct qc_mlearner : LearnerCore {
    int L = 0, m = 0, Kf = 0, row_len = 0;   // Kf = L / m forces per state
    int T[4] = {0, 0, 0, 0};     // L, T1, T2, T3
    int Tp[4] = {0, 0, 0, 0};    // padded row length of dY1, dY2, dY3 (index 1..3)
    int flat = 0;
    bool cwn = false;            // weight-normalised convolutions (qc_mlearner_params::conv_weight_norm)
    int weff[3] = {0, 0, 0};     // cwn: the convolutions' effective weights [CO][CI KS], behind the fragments in F
    int tconv[3] = {0, 0, 0};    // conv2^T, conv3^T per-phase fragments (index 1, 2); fc1^T is k.fo.t2
    float *X = nullptr, *y[4] = {nullptr, nullptr, nullptr, nullptr};   // y[1..3]: [3B] env-major activations
    float *y3f = nullptr, *h1 = nullptr, *y3p = nullptr;                // [flat][3B], [256][3B], [flat][B]
    float* dY[4] = {nullptr, nullptr, nullptr, nullptr};                // padded [B][C][Tp], index 1..3
    float *part[3] = {nullptr, nullptr, nullptr}, *partb[3] = {nullptr, nullptr, nullptr};
    int epc[3] = {2, 2, 8}, tl[3] = {128, 0, 0}, nseg[3] = {1, 1, 1}, nchunks[3] = {0, 0, 0};
    ConvPrepJobs cprep{};
    int cprep_blocks = 0;
    RedJobs red{};
};

namespace {
CreateError g_mlearner_err;

// behind every k_learner_prep (load, and the LaProp step of update and apply): the convolutions' fragments
void launch_conv_prep(qc_mlearner* l) {
    hipLaunchKernelGGL(k_mlearner_prep, dim3(l->cprep_blocks, 5), dim3(256), 0, l->stream, l->P,
                       l->cwn ? l->F : l->P, l->F, l->cprep);
}

template <int CI, int CO, int KS, int S>
void launch_convt(qc_mlearner* l, int layer /* 1: conv2, 2: conv3 */) {
    const int Tin = l->T[layer], Qn = (Tin + S - 1) / S;
    const int64_t n = (int64_t)l->B * Qn;
    const size_t Bo = (size_t)l->B;   // the previous states' activations: envs B .. 2B
    hipLaunchKernelGGL((k_mlearner_convt<CI, CO, KS, S>), dim3((unsigned)((n + 127) / 128), S), dim3(kThreads), 0, l->stream,
                       l->dY[layer + 1], l->F + l->tconv[layer], l->y[layer] + Bo * CI * Tin, l->dY[layer], Tin,
                       l->Tp[layer + 1], l->Tp[layer], Qn, n);
}

template <int CI, int CO, int KS, int S>
void launch_convdw(qc_mlearner* l, int layer /* 0..2 */) {
    constexpr int NTL = (CI * KS + 31) / 32, MTL = CO / 32;
    const int nw = l->nchunks[layer] * MTL * NTL;
    const float* X = layer == 0 ? l->X + (size_t)l->B * 2 * l->L : l->y[layer] + (size_t)l->B * CI * l->T[layer];
    hipLaunchKernelGGL((k_mlearner_convdw<CI, CO, KS, S>), dim3((nw + 3) / 4), dim3(kThreads), 0, l->stream,
                       l->dY[layer + 1], X, l->part[layer], l->partb[layer], l->T[layer], l->T[layer + 1],
                       l->Tp[layer + 1], l->epc[layer], l->tl[layer], l->nseg[layer], nw);
}
}  // namespace

extern "C" {

int qc_mlearner_create(const qc_mlearner_params* p, int device, qc_mlearner** out) {
    if (!out || !p) return QC_EINVAL;
    *out = nullptr;
    auto fail = [](const std::string& m, int rc) { return g_mlearner_err.fail(m, rc); };
    if (const char* m = bad_net_size(-1, p->n_actions)) return fail(m, QC_EINVAL);
    if (p->read_length < 1 || p->read_step_length < 1 || p->read_length % p->read_step_length != 0)
        return fail("read_length must be a positive multiple of read_step_length (the reference's view of the "
                    "force channel, RL.py:190-191)", QC_EINVAL);
    const int T1 = conv_out(p->read_length, 13, 5), T2 = conv_out(T1, 11, 4), T3 = conv_out(T2, 9, 4);
    if (T3 < 1) return fail("read_length too short for the three convolutions (T3 < 1)", QC_EINVAL);
    const std::string bad =
        bad_params(1024, p->batch_size, p->backup_period, p->lr, p->target_mode, p->beta1, p->beta2);
    if (!bad.empty()) return fail(bad, QC_EINVAL);
    if (p->conv_weight_norm != 0 && p->conv_weight_norm != 1)
        return fail("conv_weight_norm must be 0 (plain Conv1d) or 1 (Conv1d_weight_normalize on conv1..3)", QC_EINVAL);
    if ((uint64_t)(64 * T3) * (uint64_t)(3 * p->batch_size) * sizeof(float) >= (1ull << 32))   // 32-bit buffer offsets
        return fail("read_length too large: fc1's operand [64 T3][3 batch_size] must stay below 4 GiB", QC_EINVAL);
    if (const int rc = check_device(device, g_mlearner_err, "the learner")) return rc;

    qc_mlearner* l = new qc_mlearner();
    const int L = l->L = p->read_length, A = p->n_actions, B = p->batch_size;
    take_params(*l, "qc_mlearner", *p, device, noise_len(kH2, A));
    l->m = p->read_step_length;
    l->Kf = L / l->m;
    l->row_len = L + l->m + l->Kf + 3;
    l->T[0] = L; l->T[1] = T1; l->T[2] = T2; l->T[3] = T3;
    const int flat = l->flat = 64 * T3;
    // padded dY rows: kPad zeros, Tout values, then zeros up to the last q a transposed convolution reads
    for (int j = 1; j <= 3; ++j) {
        const int Qn = (l->T[j - 1] + kS[j - 1] - 1) / kS[j - 1];
        l->Tp[j] = kPad + std::max(l->T[j], Qn);
    }

    const int O[8] = {kC[0], kC[1], kC[2], kH2, kH3, A, kHM, 1};
    const int Kin[8] = {kCI[0] * kKS[0], kCI[1] * kKS[1], kCI[2] * kKS[2], flat, kH2, kH3, kH2, kHM};
    l->cwn = p->conv_weight_norm == 1;
    bool wnorm[8];
    for (int j = 0; j < 8; ++j) wnorm[j] = kWnormTail[j] || (l->cwn && j < 3);
    build_tensors(*l, 8, O, Kin, kNoisy, wnorm);
    const int* first = l->first;

    // ---- fragment buffer: the forward fragments (the measurement actor's layout; copied to the target), the
    // transposed ones of fc1 and the tail, then the convolutions' per-phase ones (and effective weights)
    build_tail_frags(*l, Kin, 3, 3);
    int cfrag_n[3] = {0, 0, 0};
    for (int j = 1; j < 3; ++j) {
        const int NI = (kKS[j] + kS[j] - 1) / kS[j];
        cfrag_n[j] = kS[j] * (kCI[j] / 32) * (NI * kC[j] / 2) * 64;
        l->tconv[j] = l->nf;
        l->nf += cfrag_n[j];
    }
    // weight-normalised convolutions: the effective weights in the natural layout (and the norms for the optimizer);
    // k_mlearner_prep, launched after k_learner_prep, makes the fragments from them
    if (l->cwn)
        for (int j = 0; j < 3; ++j) {
            l->weff[j] = l->nf;
            l->nf += (kC[j] * Kin[j] + 3) & ~3;
            const Tensor* T = &l->tt.t[first[j]];
            l->prep.push_back(PrepJob{T[0].off, T[2].off, l->wn_of[j], kC[j], Kin[j], 2, Kin[j], l->weff[j], -1, -1});
        }
    int cmax = 0;
    auto conv_w = [&](int j) { return l->cwn ? l->weff[j] : l->tt.t[first[j]].off; };   // offset from k_mlearner_prep's Wb
    for (int j = 0; j < 3; ++j) {
        const int n = tiles(kC[j]) * (Kin[j] / 2) * 64;
        l->cprep.j[j] = ConvPrepJob{conv_w(j), l->tt.t[first[j] + 1].off, l->u[j], l->ub[j],
                                    kC[j], kCI[j], kKS[j], kS[j], 0, n};
        cmax = std::max(cmax, n);
    }
    for (int j = 1; j < 3; ++j) {
        l->cprep.j[2 + j] = ConvPrepJob{conv_w(j), -1, l->tconv[j], -1, kC[j], kCI[j], kKS[j], kS[j], 1,
                                        cfrag_n[j]};
        cmax = std::max(cmax, cfrag_n[j]);
    }
    l->cprep_blocks = std::min(64, (cmax + 255) / 256);

    // ---- the split-K shape of the convolutions' dW: envs per chunk, positions per segment
    for (int j = 0; j < 3; ++j) {
        if (l->tl[j] <= 0 || l->tl[j] > l->T[j + 1]) l->tl[j] = l->T[j + 1];
        l->nseg[j] = (l->T[j + 1] + l->tl[j] - 1) / l->tl[j];
        l->nchunks[j] = B / l->epc[j] * l->nseg[j];
    }

    // ---- workspace: behind the shared head, the convolutional stack's arrays
    Carve take{tail_workspace(*l, kH2, 0, nullptr)};
    const size_t Bs = (size_t)B;
    const size_t oX = take(2 * Bs * 2 * L);
    size_t oy[4] = {0, 0, 0, 0}, ody[4] = {0, 0, 0, 0}, opart[3], opartb[3];
    for (int j = 1; j <= 3; ++j) oy[j] = take(3 * Bs * kC[j - 1] * l->T[j]);
    const size_t oy3f = take((size_t)flat * 3 * Bs), oh1 = take(kH2 * 3 * Bs), oy3p = take((size_t)flat * Bs);
    for (int j = 1; j <= 3; ++j) ody[j] = take(Bs * kC[j - 1] * l->Tp[j]);
    for (int j = 0; j < 3; ++j) {
        opart[j] = take((size_t)l->nchunks[j] * kC[j] * Kin[j]);
        opartb[j] = take((size_t)l->nchunks[j] * kC[j]);
    }

    Dev g(device);
    if (alloc_core(*l, kH2, 0, take.w) != hipSuccess) {
        free_all(*l);
        delete l;
        return fail("device allocation failed", QC_ENOMEM);
    }
    float* W = l->ws;
    LArgs& k = l->k;
    k.in_len = 0; k.in_pad = 0; k.row_len = l->row_len;
    l->X = W + oX;
    for (int j = 1; j <= 3; ++j) {
        l->y[j] = W + oy[j];
        l->dY[j] = W + ody[j];
    }
    l->y3f = W + oy3f; l->h1 = W + oh1; l->y3p = W + oy3p;
    k.h_in = l->h1;
    k.h_ld = 3 * B;
    auto gt = [&](int j, int i) { return l->G + l->tt.t[first[j] + i].off; };
    for (int j = 0; j < 3; ++j) {
        l->part[j] = W + opart[j];
        l->partb[j] = W + opartb[j];
    }
    int blk = 0;
    for (int j = 0; j < 3; ++j) {
        l->red.j[2 * j] = RedJob{l->part[j], gt(j, 0), kC[j] * Kin[j], l->nchunks[j]};
        l->red.j[2 * j + 1] = RedJob{l->partb[j], gt(j, 1), kC[j], l->nchunks[j]};
        for (int q = 0; q < 2; ++q) {
            l->red.first_block[2 * j + q] = blk;
            blk += (l->red.j[2 * j + q].n + 31) / 32;
        }
    }
    l->red.first_block[6] = blk;

    // ---- the dense dW jobs (dY, X, gradient tensor, bias gradient tensor)
    const DwJob jobs[7] = {
        {k.dZ2, l->y3p, gt(3, 0), gt(3, 1), kH2, flat},   {k.dZ3, k.H2, gt(4, 0), gt(4, 1), kH3, kH2},
        {k.dZ3e, k.H2e, gt(4, 2), gt(4, 3), kH3, kH2},    {k.dQ, k.A3, gt(5, 0), gt(5, 1), A, kH3},
        {k.dQe, k.A3e, gt(5, 2), gt(5, 3), A, kH3},       {k.dZ32, k.H2, gt(6, 0), gt(6, 1), kHM, kH2},
        {k.dM, k.R32, gt(7, 0), gt(7, 1), 1, kHM},
    };
    if (upload_dw(*l, jobs, 7) != hipSuccess || !enable_mtail_lds()) {
        free_all(*l);
        delete l;
        return fail("device setup failed (job tables / LDS size of the learner kernels)", QC_EHIP);
    }
    *out = l;
    return QC_OK;
}

void qc_mlearner_destroy(qc_mlearner* l) {
    if (!l) return;
    destroy_core(*l);
    delete l;
}

const char* qc_mlearner_last_error(const qc_mlearner* l) { return l ? l->err.c_str() : g_mlearner_err.text(); }

int qc_mlearner_set_stream(qc_mlearner* l, void* stream) {
    if (!l) return QC_EINVAL;
    l->stream = (hipStream_t)stream;
    return QC_OK;
}

int qc_mlearner_noise_len(const qc_mlearner* l) { return l ? l->noise_len : QC_EINVAL; }

int qc_mlearner_load(qc_mlearner* l, const qc_dqn_layer layers[8]) {
    if (!l || !layers) return QC_EINVAL;
    // not validate_layers / LayerRule (qcart_host.hpp): these texts name the layer, and conv1..3's depend on the handle
    for (int j = 0; j < 8; ++j) {
        const qc_dqn_layer& Y = layers[j];
        if (!Y.weight || !Y.bias) {
            l->err = std::string(kName[j]) + ": weight and bias are required";
            return QC_EINVAL;
        }
        if (j == 3 && Y.weight_norm) {
            l->err = "fc1 carries a weight_norm: fc1 is a plain Linear layer in every driver";
            return QC_EINVAL;
        }
        if (j < 3 && !l->cwn && Y.weight_norm) {
            l->err = std::string(kName[j]) + " carries a weight_norm, but the handle was created with "
                     "conv_weight_norm = 0: conv1..3 are plain Conv1d layers (Conv1d_weight_normalize, the harmonic "
                     "driver's stack, needs conv_weight_norm = 1 and a weight_norm on all three)";
            return QC_EINVAL;
        }
        if (j < 3 && l->cwn && !Y.weight_norm) {
            l->err = std::string(kName[j]) + " has no weight_norm, but the handle was created with "
                     "conv_weight_norm = 1: conv1..3 are Conv1d_weight_normalize layers";
            return QC_EINVAL;
        }
        if (j < 4 && (Y.sigma_w || Y.sigma_b)) {
            l->err = std::string(kName[j]) + " is a plain layer (no sigma)";
            return QC_EINVAL;
        }
        if (kNoisy[j] && (!Y.sigma_w || !Y.sigma_b || Y.weight_norm)) {
            l->err = std::string(kName[j]) + " must be a FactorizedNoisy layer (sigma_w and sigma_b, no weight_norm)";
            return QC_EINVAL;
        }
        if (kWnormTail[j] && (!Y.weight_norm || Y.sigma_w || Y.sigma_b)) {
            l->err = std::string(kName[j]) + " must be a Linear_weight_normalize layer (weight_norm, no sigma)";
            return QC_EINVAL;
        }
    }
    Dev g(l->device);
    if (const int rc = load_core(*l, layers)) return rc;
    launch_conv_prep(l);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? QC_OK : hip_fail(l->err, e, "learner weight preparation");
}

int qc_mlearner_layers(qc_mlearner* l, int target, qc_dqn_layer out[8]) {
    if (!l || !out) return QC_EINVAL;
    layer_views(*l, target ? l->PT : l->P, out);
    return QC_OK;
}

int qc_mlearner_grads(qc_mlearner* l, qc_dqn_layer out[8]) {
    if (!l || !out) return QC_EINVAL;
    layer_views(*l, l->G, out);
    return QC_OK;
}

int qc_mlearner_set_lr(qc_mlearner* l, double lr) { return l ? set_lr(*l, lr) : QC_EINVAL; }
int qc_mlearner_set_backup_period(qc_mlearner* l, int32_t period) { return l ? set_backup_period(*l, period) : QC_EINVAL; }

int qc_mlearner_states(qc_mlearner* l, const float* transitions, float* next_out, float* prev_out) {
    if (!l || !transitions || !next_out || !prev_out) return QC_EINVAL;
    Dev g(l->device);
    const size_t n = (size_t)l->B * 2 * l->L;
    hipLaunchKernelGGL(k_mlearner_states, dim3(l->B), dim3(256), (l->Kf + 1) * sizeof(float), l->stream, transitions, l->X,
                       l->L, l->m, l->Kf, l->row_len, l->B);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(next_out, l->X, n * sizeof(float), hipMemcpyDeviceToDevice, l->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(prev_out, l->X + n, n * sizeof(float), hipMemcpyDeviceToDevice, l->stream);
    if (e != hipSuccess) return hip_fail(l->err, e, "state assembly");
    return QC_OK;
}

int qc_mlearner_update(qc_mlearner* l, const float* transitions, const float* is_weights, const float* noise,
                       uint64_t counter, float* unweighted_loss, float* loss) {
    if (!l) return QC_EINVAL;
    Dev g(l->device);
    if (const int rc = begin_update(*l, transitions, is_weights, unweighted_loss, noise, counter)) return rc;
    hipStream_t s = l->stream;
    const int B = l->B, L = l->L;
    hipLaunchKernelGGL(k_mlearner_states, dim3(B), dim3(256), (l->Kf + 1) * sizeof(float), s, transitions, l->X, L, l->m,
                       l->Kf, l->row_len, B);
    // ---- forward: the online net on next | prev (envs 0 .. 2B), the target net on next (envs 2B .. 3B)
    for (int tgt = 0; tgt < 2; ++tgt) {
        const float* Fw = tgt ? l->FT : l->F;
        const size_t e0 = tgt ? 2 * (size_t)B : 0;
        qcart::actor::MnetFwd a{};
        a.x = l->X;
        a.L = L; a.T1 = l->T[1]; a.T2 = l->T[2]; a.T3 = l->T[3];
        for (int j = 0; j < 4; ++j) {
            a.wf[j] = Fw + l->u[j];
            a.bias[j] = Fw + l->ub[j];
        }
        a.y1 = l->y[1] + e0 * kC[0] * l->T[1];
        a.y2 = l->y[2] + e0 * kC[1] * l->T[2];
        a.y3e = l->y[3] + e0 * kC[2] * l->T[3];
        a.y3f = l->y3f;
        a.h = l->h1;
        a.nb = tgt ? B : 2 * B;
        a.ld = 3 * B;
        a.c0 = (int64_t)e0;
        qcart::actor::launch_mnet_fwd(s, a);
    }
    qcart::actor::launch_mtr(s, l->y[3] + (size_t)B * l->flat, l->y3p, l->flat, B, B, 0);
    LArgs k = l->k;
    k.trans = transitions;
    launch_mtail_fwd(s, k);
    // k_learner_loss reads the action at row[2 in_len] and the reward after it: in_len = 0 on rows that start
    // at the action column
    launch_loss(s, l->target_mode,
                loss_args(*l, transitions + (l->row_len - 2), 0, kH2, is_weights, unweighted_loss, loss));
    launch_mtail_bwd(s, k);
    // ---- backward of fc1 and of the convolutions
    hipLaunchKernelGGL(k_mlearner_fc1t, dim3(B / kE, (tiles(l->flat) + 7) / 8), dim3(kThreads), 0, s, l->F + k.fo.t2, k.dZ2,
                       l->y3p, l->dY[3], l->T[3], l->Tp[3], l->flat, B);
    launch_convt<64, 64, 9, 4>(l, 2);
    launch_convt<32, 64, 11, 4>(l, 1);
    launch_convdw<64, 64, 9, 4>(l, 2);
    launch_convdw<32, 64, 11, 4>(l, 1);
    launch_convdw<2, 32, 13, 5>(l, 0);
    hipLaunchKernelGGL(k_mlearner_reduce, dim3(l->red.first_block[6]), dim3(256), 0, s, l->red);
    launch_dw(s, l->d_dwjobs, l->d_tiles, l->ntiles, B);
    launch_wndot(s, l->nwn, l->P, l->G, l->wn_tensors, l->tt, l->d_dot);
    opt_step(*l, 1);
    launch_conv_prep(l);
    return end_update(*l, 28);
}

int qc_mlearner_apply(qc_mlearner* l, const qc_dqn_layer grads[8]) {
    if (!l || !grads) return QC_EINVAL;
    Dev g(l->device);
    if (const int rc = apply_core(*l, grads)) return rc;
    launch_conv_prep(l);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? QC_OK : hip_fail(l->err, e, "learner optimizer launch");
}

int qc_mlearner_stats(qc_mlearner* l, qc_learner_stats_t* out) { return l && out ? stats_core(*l, out) : QC_EINVAL; }

// F holds the convolutions' fragments (and, weight-normalised, their effective weights) behind the tail's, so
// the core's payload covers what k_mlearner_prep made
static qcart::state::Header mlearner_header(const qc_mlearner& l) {
    qcart::state::Header h = qcart::state::make(qcart::state::kMlearner);
    qcart::state::put_i(h, "read_length", l.L);
    qcart::state::put_i(h, "read_step_length", l.m);
    qcart::state::put_i(h, "conv_weight_norm", l.cwn ? 1 : 0);
    put_core_fields(l, h);
    return h;
}

int qc_mlearner_state_bytes(qc_mlearner* l, uint64_t* n) { return l && n ? state_bytes_core(*l, n) : QC_EINVAL; }

int qc_mlearner_state_export(qc_mlearner* l, void* host_dst, uint64_t n) {
    return l && host_dst ? state_export_core(*l, mlearner_header(*l), host_dst, n) : QC_EINVAL;
}

int qc_mlearner_state_import(qc_mlearner* l, const void* host_src, uint64_t n) {
    return l ? state_import_core(*l, mlearner_header(*l), host_src, n) : QC_EINVAL;
}

}  // extern "C"

