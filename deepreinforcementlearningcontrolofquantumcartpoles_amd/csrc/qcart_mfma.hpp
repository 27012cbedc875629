// qcart_mfma.hpp — the f32-input MFMA pieces the DQN actor (qcart_actor.hip) and the DQN learner
// (qcart_learner.hip) share: the weight fragment layout, the LDS-operand GEMM tile and the D-tile map.
//
// Every layer is Y[o][col] = W[o][k] X[k][col] on v_mfma_f32_32x32x2_f32 (exact f32 accumulation):
// A = the weights, stored once per load in fragment order [tile][k-step][64 lanes] (one coalesced 256-B
// read per MFMA), B = the activations in LDS as [feature][32 columns] (one conflict-free ds_read_b32
// per MFMA), D = a 32-feature x 32-column tile whose rows land in the 16 accumulator registers.
#pragma once
#include <hip/hip_runtime.h>

namespace qcart {
namespace mfma {

constexpr int kE = 32;                 // columns (envs / batch rows) per workgroup: one MFMA column block
using f32x16 = float __attribute__((ext_vector_type(16)));

// fragment buffer of one [O][K] matrix: tiles of 32 outputs x K/2 steps x 64 lanes
__host__ __device__ constexpr int tiles(int O) { return (O + 31) / 32; }
__host__ __device__ constexpr int ksteps(int K) { return (K + 1) / 2; }

// element i of a fragment buffer with S k-steps per tile -> (output o, input k) of the matrix.
// split = 0: MFMA k-step s pairs k = 2s, 2s + 1 (lane halves); split = 1: k = s, s + S (the
// convolutions: the upper half of K is then a fixed input offset, see k_mconv)
__device__ __forceinline__ void frag_ok(int i, int S, int split, int& o, int& k) {
    const int l = i & 63, s = (i >> 6) % S, t = (i >> 6) / S;
    o = t * 32 + (l & 31);
    k = split ? s + (l >> 5) * S : 2 * s + (l >> 5);
}

// acc += A_frag(W) . X  over `steps` k-steps (X: LDS [k][32]; lane reads X[2s + (lane>>5)][lane&31]).
// The weight fragments come from L2: batches of kP steps, the next batch's loads issued before the
// current batch's MFMAs (kP x 64 cycles of MFMA cover the L2 latency at one wave per SIMD).
constexpr int kP = 16;
__device__ __forceinline__ void gemm_tile(f32x16& acc, const float* __restrict__ wf, const float* x, int steps,
                                          int lane) {
    const float* xl = x + (lane >> 5) * kE + (lane & 31);
    const float* wl = wf + lane;
    const int full = steps / kP * kP;
    f32x16 acc1 = {};   // second accumulator chain (odd steps): halves the dependent-MFMA chain
    float a[kP];
    if (full > 0) {
#pragma unroll
        for (int u = 0; u < kP; ++u) a[u] = wl[u * 64];
    }
    for (int s = 0; s < full; s += kP) {
        float an[kP];
        const int sn = s + kP < full ? s + kP : s;   // last batch: harmless reload of the same fragments
#pragma unroll
        for (int u = 0; u < kP; ++u) an[u] = wl[(sn + u) * 64];
        __builtin_amdgcn_sched_barrier(0);   // keep the next batch's loads ahead of this batch's MFMAs
#pragma unroll
        for (int u = 0; u < kP; u += 2) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], xl[(s + u) * 2 * kE], acc, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u + 1], xl[(s + u + 1) * 2 * kE], acc1, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kP; ++u) a[u] = an[u];
    }
    for (int s = full; s < steps; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wl[s * 64], xl[s * 2 * kE], acc, 0, 0, 0);
    acc += acc1;
}

// D-tile element r of this lane: output row (within the tile) and column lane & 31
__device__ __forceinline__ int drow(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

}  // namespace mfma
}  // namespace qcart
