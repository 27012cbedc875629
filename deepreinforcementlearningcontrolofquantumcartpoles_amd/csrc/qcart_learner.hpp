// qcart_learner.hpp — what the two device learners share: the argument structs and job tables of the
// table-driven learner kernels (qcart_learner.hip) and host-side launchers for them, so that the
// measurement-input learner (qcart_mlearner.hip) drives the same kernels, and a launcher for the
// measurement network's forward stack (k_mconv / k_mtr / k_mfc, qcart_actor.hip). The kernels stay in
// the translation units that define them. Internal: not part of the C ABI (include/qcart.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "qcart_dqn.hpp"

namespace qcart {
namespace learner {

constexpr int kChunks = 32;        // FactorizedNoisy.forward: n = 32 noise samples per batch (layers.py:58)
constexpr int kMaxNT = 25;         // parameter tensors: 20 (direct_DQN), 22 / 25 (DQN_measurement, plain / weight-normalised convolutions)
constexpr int kMaxWN = 8;          // weight-normalised layers of one net: 4 (direct_DQN), 2 / 5 (DQN_measurement)
constexpr int kLdsFloats = dqn::kActLdsFloats + dqn::kHM * dqn::kE;   // the actor's plan, then R32 [128][32]

// offsets into the fragment buffer (floats): forward part first (copied to the target), then transposed
struct FragOff {
    int u[6], s[6], ub[6], sb[6];   // fc1, fc2, fc31, fc41, fc32, fc42
    int t2, t31u, t31s, t41u, t41s, t32, w42;
};

struct LArgs {
    const float* F;      // online fragments
    const float* FT;     // target fragments (forward part)
    FragOff fo;
    int in_len, in_pad, n_act, B, row_len, rpc;   // rpc: rows per noise chunk = B / 32
    const float* trans;
    const float* noise;  // [noise_len][32]
    float* Q;            // [3][B][32]
    float* M;            // [3][B]
    // feature-major [rows][B] workspace of the online/prev pass and of the backward
    float *X0, *H1, *H2, *H2e, *A3, *A3e, *R32;
    float *dQ, *dQe, *dM, *dZ3, *dZ3e, *dZ32, *dZ2, *dZ1;
    // the measurement network's tail (k_learner_fwd / k_learner_bwd <256, true>): relu(fc1) of the three passes,
    // feature-major [256][h_ld], pass p's rows at columns p B ..; enters as H2
    const float* h_in;
    int h_ld;
};

struct LossArgs {
    const float* Q;
    const float* M;
    const float* trans;
    const float* w;
    const float* noise;
    int B, n_act, in_len, row_len, rpc;
    int eps_out41;   // NoiseAt<W2>::kEpsOut41 of the handle's net
    float gamma, rew /* (1 - gamma) alive_reward */, omg /* 1 - gamma */, failing, inv_B, inv_A;
    float *dQ, *dQe, *dM, *ul, *loss, *loss_user;
    int32_t* cnt;   // [0] non-finite losses, [1] rows with an action outside [0, n_act)
};

// dW = dY X^T: A = dY [O pad 32][B], X [K pad 32][B] (feature-major, pad rows zero), out [O][K] natural layout
struct DwJob {
    const float* A;
    const float* X;
    float* out;
    float* bias;   // row sums of A (the bias gradient), written by the k-tile-0 waves; may be null
    int O, K;
};

// parameter tensor table
struct Tensor {
    int off, n;
    int kind;   // 0 plain, 1 weight of a weight-normalised layer, 2 its weight_norm g
    int wn;     // weight-normalised layer index (kind 1 / 2) or -1
    int w_off;  // kind 2: offset of the layer's weight
};
struct TensorTable {
    Tensor t[kMaxNT];
};
// the weight tensor of each weight-normalised layer (k_learner_wndot: one workgroup per entry)
struct WnTensors {
    int t[kMaxWN];
};

struct OptArgs {
    float *P, *G, *E, *V, *MU;
    const double* dot;    // [kMaxWN] <G, W>, then [kMaxWN] the layers' g (k_learner_wndot)
    const float* norm;    // [kMaxWN] ||W||_F of the parameters the gradients were taken at
    int chain;            // 1: G holds effective-weight gradients: apply the weight-norm chain rule first
    int centered;         // step > 10
    float beta1, beta2, omb2, l2, elr /* (1 - beta1) lr */, step_size /* 1 / (l1 / lr), or 1 */, eps;
};

// effective weight (W g / ||W||_F, or W) -> fragments / a plain vector; bias padded to tiles * 32
struct PrepJob {
    int w_off, g_off /* -1: none */, wn /* -1 */, O, K;
    int mode;        // 0 forward fragments of W [O][K pad], 1 fragments of W^T [K][O pad], 2 plain scaled copy
    int Kpad;        // padded contraction length of the fragment matrix
    int out_off;
    int bias_off /* -1: none */, bias_pad_off;
};
constexpr int kPrepParts = 8;

// LaProp's host-side scalars (optimizer.py:69-80), shared by the two handles
constexpr double kBeta1 = 0.9, kBeta2 = 0.9995, kEps = 1e-15;   // the defaults: IHO / IQO / QO RL.py:144-145
constexpr int kCenteredAfter = 10;                               // optimizer.py:9

// ---- launchers of qcart_learner.hip's kernels (each: one launch on `s`) ----
void launch_noise(hipStream_t s, const float* in, float* out, int noise_len, uint64_t seed, uint64_t counter);
void launch_loss(hipStream_t s, int target_mode, const LossArgs& a);
void launch_dw(hipStream_t s, const DwJob* jobs, const int4* tiles, int ntiles, int B);
void launch_wndot(hipStream_t s, int n_layers, const float* P, const float* G, const WnTensors& wn_tensors,
                  const TensorTable& tt, double* dot);
void launch_opt(hipStream_t s, const OptArgs& o, const TensorTable& tt, int nt);
void launch_prep(hipStream_t s, const float* P, float* F, const PrepJob* jobs, int njobs, float* norm);
// the measurement network's tail: direct_DQN from fc31 on at H2 = 256, entered with a.h_in (3 B / 32
// workgroups), and its backward down to dZ2 (B / 32 workgroups)
bool enable_mtail_lds();
void launch_mtail_fwd(hipStream_t s, const LArgs& a);
void launch_mtail_bwd(hipStream_t s, const LArgs& a);

}  // namespace learner

namespace actor {

// DQN_measurement's forward up to relu(fc1) for nb envs, as qc_mactor_act launches it (five launches):
// x [nb][2][L] -> y1 [nb][32][T1] -> y2 [nb][64][T2] -> y3e [nb][64 T3] (env-major), y3e transposed into
// columns c0 .. of y3f [64 T3][ld], h [256][ld] columns c0 ..; wf / bias: the four layers' forward
// fragments (split = 1 for the convolutions) and padded biases
struct MnetFwd {
    const float* x;
    int L, T1, T2, T3;
    const float* wf[4];
    const float* bias[4];
    float *y1, *y2, *y3e, *y3f, *h;
    int64_t nb, ld, c0;
};
void launch_mnet_fwd(hipStream_t s, const MnetFwd& a);
void launch_mtr(hipStream_t s, const float* in, float* out, int F, int64_t nb, int64_t ld, int64_t c0);

}  // namespace actor
}  // namespace qcart
