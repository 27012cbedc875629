// qcart_dqn.hpp — the one device-side definition of the reference's direct_DQN (RL.py:80-111, layers.py)
// that the actor (qcart_actor.hip) and the learner (qcart_learner.hip) share: the network constants and
// noise layout, the dense layer of a 4-wave workgroup on the fragments of qcart_mfma.hpp, the fc41 wave
// split, the NoisyNet noise draw, the 1024-thread tree sum and the weight-norm scale.
//
// One workgroup = 32 columns (envs / batch rows) x 4 waves; activations live in LDS as [feature][32] and
// never leave the CU. A factorised noisy layer is two GEMMs per tile, u_w X and sigma_w (eps_in o X):
//   y = u_w x + u_b + eps_out o (sigma_w (eps_in o x) + sigma_b)   (== (u_w + sigma_w o eps_out eps_in^T) x + ...)
// The kernels' epilogues spell that sum themselves: how it is written fixes its rounding (-ffp-contract=on).
#pragma once
#include "qcart_kernels.hpp"
#include "qcart_mfma.hpp"

namespace qcart {
namespace dqn {

using namespace qcart::mfma;   // kE, f32x16, tiles / ksteps, gemm_tile, drow

constexpr int kH1 = 512, kH2 = 256, kH3 = 256, kHM = 128;   // fc1, fc2, fc31, fc32 widths
// fc2's width is the one that differs between the reference's drivers: 256 (harmonic, inverted harmonic: kH2)
// or 512 (quartic, inverted quartic: kH2Wide); the kernels take it as a template argument W2
constexpr int kH2Wide = 512;
// a params struct's hidden2 field -> the width (0: the narrow net), or 0 where it is neither
inline int fc2_width(int hidden2) { return hidden2 == 0 || hidden2 == kH2 ? kH2 : hidden2 == kH2Wide ? kH2Wide : 0; }
// X0 lives in LDS as [in_pad][32] fp32 inside one 64 KiB region: up to kChunkIn rows at once. A longer input (the
// 'wavefunction' input: 2 (x_n - 20) floats, 1002 for the inverted quartic driver) passes through that region in
// chunks of kChunkIn rows, fc1 accumulating over them in registers (dense4_chunked). That form of k_actor_act /
// k_learner_fwd is the instantiation at W2 + kChunkTag (257 / 513): the tag rides on the width argument so that the
// unchunked instantiations keep their template arguments, and with them their symbol names and their code
constexpr int kChunkIn = 512;
constexpr int kChunkTag = 1;
constexpr int kMaxIn = 1024;     // data_length limit
constexpr int kThreads = 256;    // 4 waves
__host__ __device__ constexpr int in_pad(int data_length) { return (data_length + 1) & ~1; }
// the create-time range checks (data_length < 0: the handle has none); null when the sizes are fine
inline const char* bad_net_size(int data_length, int n_actions) {
    static_assert(kMaxIn == 1024, "the text below names the limit");
    if (data_length >= 0 && (data_length < 1 || data_length > kMaxIn)) return "data_length must be in [1, 1024]";
    if (n_actions < 1 || n_actions > 32) return "n_actions must be in [1, 32]";
    return nullptr;
}

// one noise sample, as FactorizedNoisy draws it: eps_in [W2] / eps_out [256] of fc31, then eps_in [256] /
// eps_out [n_actions] of fc41
template <int W2>
struct NoiseAt {
    static constexpr int kEpsIn31 = 0, kEpsOut31 = kEpsIn31 + W2, kEpsIn41 = kEpsOut31 + kH3, kEpsOut41 = kEpsIn41 + kH3;
};
__host__ __device__ constexpr int noise_len(int w2, int n_actions) { return w2 + 2 * kH3 + n_actions; }

// k_actor_act's LDS: RA = H1 [512][32], later H3 + eps_in o H3; RB = X0 [in_pad][32], later H2 + eps_in o H2;
// RC = fc41's sigma partial as D registers [16][64]. At W2 = 512 H2 fills RB, so eps_in o H2 goes over the
// dead H1 in RA, fc31's output waits in registers (dense4_hold2) until both are dead, and H3 + eps_in o H3
// then go to RA: the same two 64 KiB regions, two barriers more
constexpr int kActLdsFloats = 2 * kH1 * kE + 16 * 64;
constexpr size_t kActLdsBytes = kActLdsFloats * sizeof(float);

// Y = W X for one layer, on 4 waves: wave w takes the output tiles w, w + 4, ... (X: LDS [K][32]); where sf is
// given, also Ys = sigma_w Xe on the sigma fragments. epi(o, y_u, y_sigma) gets each of the lane's 16 D
// elements (output o, column lane & 31) and adds bias / noise, applies ReLU, stores.
template <class Epi>
__device__ __forceinline__ void dense4(const float* __restrict__ uf, const float* __restrict__ sf, const float* x,
                                       const float* xe, int O, int K, int lane, int wave, Epi epi) {
    const int S = ksteps(K);
    for (int t = wave; t < tiles(O); t += 4) {
        f32x16 acc = {}, accs = {};
        gemm_tile(acc, uf + (size_t)t * S * 64, x, S, lane);
        if (sf) gemm_tile(accs, sf + (size_t)t * S * 64, xe, S, lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) epi(t * 32 + drow(r, lane), acc[r], accs[r]);
    }
}

// A 256-output layer whose results cannot go to LDS yet (its operands fill both regions): wave w computes
// tiles w and w + 4 as dense4 does and keeps hold[j][r] = epi(o, y_u, y_sigma) for tile w + 4 j, D element r
// (output o = (w + 4 j) 32 + drow(r, lane)); the caller stores them after its next barrier
template <class Epi>
__device__ __forceinline__ void dense4_hold2(const float* __restrict__ uf, const float* __restrict__ sf, const float* x,
                                             const float* xe, int K, int lane, int wave, float (&hold)[2][16],
                                             Epi epi) {
    static_assert(tiles(kH3) == 8, "two tiles for each of the 4 waves");
    const int S = ksteps(K);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int t = wave + 4 * j;
        f32x16 acc = {}, accs = {};
        gemm_tile(acc, uf + (size_t)t * S * 64, x, S, lane);
        if (sf) gemm_tile(accs, sf + (size_t)t * S * 64, xe, S, lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) hold[j][r] = epi(t * 32 + drow(r, lane), acc[r], accs[r]);
    }
}

// One chunk of X0 into LDS: xb[k][e] = load(c0 + k, e) for k < rows, e < 32 (load answers 0 past the input's
// end or the batch's). QCART_FC1_STAGE_K = 0: lanes along the column index e, as the unchunked kernels stage
// (conflict-free LDS writes; every lane reads from its own input row). 1: lanes along k in runs of 8 (a wave covers
// 8 rows x 8 columns: each run is one 32-B piece of an input row; the transposed LDS writes meet 4 to a bank), rows
// rounded up to 8 (<= kChunkIn, inside xb)
template <class Load>
__device__ __forceinline__ void stage_chunk(float* xb, int c0, int rows, int tid, Load load) {
#if QCART_FC1_STAGE_K
    const int n = ((rows + 7) & ~7) * kE;
    for (int i = tid; i < n; i += kThreads) {
        const int b = i >> 6, k = (b >> 2) * 8 + (i & 7), e = (b & 3) * 8 + ((i >> 3) & 7);
        xb[k * kE + e] = load(c0 + k, e);
    }
#else
    for (int i = tid; i < rows * kE; i += kThreads) xb[i] = load(c0 + i / kE, i % kE);
#endif
}

// fc1 for K = in_pad > kChunkIn: X0 passes through xb (LDS [kChunkIn][32]) in chunks of kChunkIn rows, staged by
// stage_chunk between two barriers; wave w keeps its four output tiles w, w + 4, w + 8, w + 12 in registers across
// the chunks (dense4_hold2's idea) and walks each tile's fragments [tile][k-step][64] from the chunk's first k-step.
// epi(o, y) as dense4's, once per output after the last chunk. Every wave must call it
template <class Load, class Epi>
__device__ __forceinline__ void dense4_chunked(const float* __restrict__ uf, float* xb, int K, int tid, Load load,
                                               Epi epi) {
    static_assert(tiles(kH1) == 16, "four tiles for each of the 4 waves");
    static_assert(kChunkIn % 2 == 0, "a chunk starts at a k-step");
    const int lane = tid & 63, wave = tid >> 6;
    const int S = ksteps(K);
    f32x16 acc[4] = {};
    for (int c0 = 0; c0 < K; c0 += kChunkIn) {
        const int rows = K - c0 < kChunkIn ? K - c0 : kChunkIn;   // even: K is
        if (c0) __syncthreads();   // every wave is done reading the previous chunk
        stage_chunk(xb, c0, rows, tid, load);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j)
            gemm_tile(acc[j], uf + ((size_t)(wave + 4 * j) * S + c0 / 2) * 64, xb, rows / 2, lane);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) epi((wave + 4 * j) * 32 + drow(r, lane), acc[j][r]);
}

// fc41, one 32-row tile: wave 0 computes u_w H3, wave 1 sigma_w (eps_in o H3), handed over through the LDS
// partial rc. Every wave must call it (it holds a barrier); only wave 0 returns true, after epi(o, y_u, y_sigma)
// for each of its lane's outputs o = drow(r, lane) < n_act. Waves 2 and 3 may run `other` beside the two GEMMs.
template <class Epi, class Other>
__device__ __forceinline__ bool fc41(const float* __restrict__ uf, const float* __restrict__ sf, const float* h3,
                                     const float* h3e, float* rc, int n_act, int lane, int wave, Epi epi,
                                     Other other) {
    if (wave == 1 && sf) {
        f32x16 accs = {};
        gemm_tile(accs, sf, h3e, ksteps(kH3), lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) rc[r * 64 + lane] = accs[r];
    }
    f32x16 acc = {};
    if (wave == 0) gemm_tile(acc, uf, h3, ksteps(kH3), lane);
    if (wave >= 2) other();
    __syncthreads();
    if (wave != 0) return false;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = drow(r, lane);
        if (o < n_act) epi(o, acc[r], sf ? rc[r * 64 + lane] : 0.f);
    }
    return true;
}

// NoisyNet noise pair `pair` of stream `key` (an env, or a learner chunk): f(z) = sign(z) sqrt|z|
// (layers.py:77-79) of two Philox normals keyed by (seed, key), counter, tag 0x100 + pair. Box-Muller in fp32
// (hardware log / sin / cos): the network noise is fp32 and has no oracle stream
__device__ __forceinline__ float2 noise_pair(uint64_t seed, uint64_t counter, uint32_t key, int pair) {
    uint32_t c[4] = {(uint32_t)counter, (uint32_t)(counter >> 32), key, 0x100u + (uint32_t)pair};
    philox10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u1 = ((float)(c[0] >> 8) + 0.5f) * 0x1.0p-24f, u2 = (float)(c[1] >> 8) * 0x1.0p-24f;
    const float rad = sqrtf(-2.f * __logf(u1));
    float sn, cs;
    __sincosf(6.283185307f * u2, &sn, &cs);
    const float f0 = rad * cs, f1 = rad * sn;
    return float2{copysignf(sqrtf(fabsf(f0)), f0), copysignf(sqrtf(fabsf(f1)), f1)};
}

// sum of v over a 1024-thread workgroup in a fixed order (halving from 512, partner + w); part: LDS [1024]
template <class T>
__device__ __forceinline__ T block_sum(T v, T* part) {
    part[threadIdx.x] = v;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    return part[0];
}

// Linear_weight_normalize (layers.py:97-103): W_eff = W g / ||W||_F, from g and ss = sum W^2
__device__ __forceinline__ float wn_scale(float g, double ss) { return (float)((double)g / sqrt(ss)); }

}  // namespace dqn
}  // namespace qcart
