// qcart_learner.hpp — what the two device learners share: the argument structs and job tables of the
// table-driven learner kernels (qcart_learner.hip) and host-side launchers for them, so that the
// measurement-input learner (qcart_mlearner.hip) drives the same kernels, LearnerCore (the host state of one
// update pipeline: schedule, LaProp scalars, tensor table, buffers, job tables) with the free functions both
// handles are written in, and a launcher for the measurement network's forward stack (k_mconv / k_mtr / k_mfc,
// qcart_actor.hip). Kernels and functions stay in the translation units that define them (the core's:
// qcart_learner.hip). Internal: not part of the C ABI (include/qcart.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/qcart.h"
#include "qcart_dqn.hpp"
#include "qcart_state.hpp"

namespace qcart {
namespace learner {

constexpr int kChunks = 32;        // FactorizedNoisy.forward: n = 32 noise samples per batch (layers.py:58)
constexpr int kMaxNT = 25;         // parameter tensors: 20 (direct_DQN), 22 / 25 (DQN_measurement, plain / weight-normalised convolutions)
constexpr int kMaxLayers = 8;      // layers of one net: 6 (direct_DQN), 8 (DQN_measurement)
constexpr int kMaxWN = 8;          // weight-normalised layers of one net: 4 (direct_DQN), 2 / 5 (DQN_measurement)
constexpr int kLdsFloats = dqn::kActLdsFloats + dqn::kHM * dqn::kE;   // the actor's plan, then R32 [128][32]

// offsets into the fragment buffer (floats): forward part first (copied to the target), then transposed
struct FragOff {
    int u[6], s[6], ub[6], sb[6];   // fc1, fc2, fc31, fc41, fc32, fc42 (the measurement net: conv3, fc1, then its tail)
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

// ---- what both learner handles hold, and the functions below work on (the counterpart of ActorCore) ----
struct LearnerCore {
    const char* name = "";    // "qc_learner" / "qc_mlearner": the handle's functions in error texts
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    bool loaded = false;
    int A = 0, B = 0, noise_len = 0;
    // what an update needs from the handle's params
    int backup_period = 1, target_mode = QC_TD_ALIVE;
    int backup_period0 = 1;   // the create-time period: what the state header carries (set_backup_period changes backup_period)
    double gamma = 0, alive_reward = 0, failing_reward = 0;
    uint64_t seed = 0;
    double b1 = 0, b2 = 0;    // LaProp's betas
    // host-side schedule and LaProp scalars (optimizer.py:69-80)
    int64_t updates = 0, step = 0;
    int backup_counter = 0;
    double lr = 0, l1 = 0, l2 = 0;
    int launches = 0;         // launches of the last update
    // the layers: a layer's tensors are weight, bias, then g (wnorm) | sigma_w, sigma_b (noisy)
    int n_layers = 0, O[kMaxLayers]{}, K[kMaxLayers]{}, first[kMaxLayers]{} /* its first tensor */, wn_of[kMaxLayers]{};
    bool noisy[kMaxLayers]{}, wnorm[kMaxLayers]{};
    int nt = 0, nwn = 0;      // tensors; weight-normalised layers
    TensorTable tt{};
    WnTensors wn_tensors{};
    int np = 0;               // floats in one parameter buffer
    int nf = 0, nf_fwd = 0;   // floats in the fragment buffer / its forward part
    int u[kMaxLayers]{}, s[kMaxLayers]{}, ub[kMaxLayers]{}, sb[kMaxLayers]{};   // forward fragments / padded biases
    float *P = nullptr, *PT = nullptr, *G = nullptr, *E = nullptr, *V = nullptr, *MU = nullptr;
    float *F = nullptr, *FT = nullptr;
    float* ws = nullptr;      // workspace: Q, M, noise, activations, dY, then the handle's own arrays
    LArgs k{};
    float *d_noise = nullptr, *d_loss = nullptr, *d_norm = nullptr;
    double* d_dot = nullptr;
    int32_t* d_cnt = nullptr;
    DwJob* d_dwjobs = nullptr;
    int4* d_tiles = nullptr;
    int ntiles = 0;
    std::vector<PrepJob> prep;   // k_learner_prep's jobs until alloc_core uploads them to d_prep
    PrepJob* d_prep = nullptr;
    int nprep = 0;
    std::vector<void*> allocs;   // every device allocation (free_all)
};

// the create-time checks both params structs share (empty: none failed); max_batch: 4096 / 1024
std::string bad_params(int max_batch, int batch_size, int backup_period, double lr, int target_mode, double beta1,
                       double beta2);
// the fields both params structs share
template <class Params>
void take_params(LearnerCore& c, const char* name, const Params& p, int device, int noise_len) {
    c.name = name;
    c.device = device;
    c.A = p.n_actions; c.B = p.batch_size; c.noise_len = noise_len;
    c.backup_period = c.backup_period0 = p.backup_period; c.target_mode = p.target_mode;
    c.gamma = p.gamma; c.alive_reward = p.alive_reward; c.failing_reward = p.failing_reward;
    c.seed = p.seed;
    c.lr = p.lr;
    c.b1 = p.beta1 != 0. ? p.beta1 : kBeta1;
    c.b2 = p.beta2 != 0. ? p.beta2 : kBeta2;
}
// the parameter tensor table (offsets in multiples of 4 floats) of n layers [O][K]: first, wn_of, nt, nwn, tt,
// wn_tensors, np
void build_tensors(LearnerCore& c, int n, const int* O, const int* K, const bool* noisy, const bool* wnorm);
// the fragment buffer's forward part (every layer at contraction length Kpad) and, for the layer `fc2` and the
// four after it (k_learner_fwd / k_learner_bwd's fc2, fc31, fc41, fc32, fc42 slots of k.fo), the transposed
// fragments and w42; k_learner_prep's jobs for the forward fragments of layers j0.. and for the transposed ones.
// Leaves nf at the end of what it laid out: the handle may append
void build_tail_frags(LearnerCore& c, const int* Kpad, int j0, int fc2);
// a bump allocator over the workspace, in floats, 16-byte steps
struct Carve {
    size_t w = 0;
    size_t operator()(size_t n) {
        const size_t at = w;
        w += (n + 3) & ~(size_t)3;
        return at;
    }
};
// the workspace's shared head, k_learner_fwd / k_learner_bwd's arrays: Q, M, noise, the activations and dY at fc2 width
// w2 (in_len > 0: fc1 / fc2's too, for an input of in_len; 0: the tail's only), loss, norms. Returns its floats
size_t tail_workspace(LearnerCore& c, int w2, int in_len, float* W /* null: measure only */);
// a zeroed, tracked device allocation of n T
template <class T>
hipError_t dalloc(LearnerCore& c, T** q, size_t n) {
    hipError_t e = hipMalloc(q, n * sizeof(T));
    if (e != hipSuccess) return e;
    c.allocs.push_back(*q);
    return hipMemset(*q, 0, n * sizeof(T));
}
void free_all(LearnerCore& c);
// the parameter / state / fragment buffers, the workspace of ws_floats (>= tail_workspace's) and the uploaded prep
// jobs; points k and d_noise / d_loss / d_norm into them
hipError_t alloc_core(LearnerCore& c, int w2, int in_len, size_t ws_floats);
// the dW jobs with one tile per 32 x 32 block of each, uploaded
hipError_t upload_dw(LearnerCore& c, const DwJob* jobs, int n);
// sync, free_all (the caller deletes the handle)
void destroy_core(LearnerCore& c);
// the layers' tensors inside one flat buffer (the parameters, the target's, or the gradients)
void layer_views(const LearnerCore& c, const float* base, qc_dqn_layer* out);
int set_lr(LearnerCore& c, double lr);
// the target network's period from the next update on (Main_System's temporary 100, IHO main_parallel.py:480-481,
// 546-547); backup_counter is reduced modulo the new period
int set_backup_period(LearnerCore& c, int period);
// qc_*_load after the layers' validation: copies, zeroed optimizer state, k_learner_prep, schedule reset
int load_core(LearnerCore& c, const qc_dqn_layer* layers);
// qc_*_update's head: the refusals, the target sync at backup_counter == 0, the noise launch; and its end after n launches
int begin_update(LearnerCore& c, const float* transitions, const float* is_weights, const float* unweighted_loss,
                 const float* noise, uint64_t counter);
int end_update(LearnerCore& c, int n);
// k_learner_loss's arguments: the action sits at trans[row][2 in_len], the reward behind it
LossArgs loss_args(const LearnerCore& c, const float* trans, int in_len, int w2, const float* is_weights,
                   float* unweighted_loss, float* loss);
// one LaProp step and the fragment preparation (k_learner_opt, k_learner_prep); chain: G holds effective-weight gradients
void opt_step(LearnerCore& c, int chain);
// qc_*_apply up to and including opt_step
int apply_core(LearnerCore& c, const qc_dqn_layer* grads);
int stats_core(LearnerCore& c, qc_learner_stats_t* out);

// ---- qc_*_state_bytes / _export / _import of both learners (the blob's header: qcart_state.hpp). The payload is
// the host schedule (updates, step, backup_counter, the period set_backup_period left or 0, lr, l1, l2), the device counters behind qc_*_stats, then P, PT,
// E, V, MU, F, FT and d_norm as they are. The handle passes its own header: its geometry fields first;
// put_core_fields appends what both params structs share and the buffer sizes
void put_core_fields(const LearnerCore& c, state::Header& h);
int state_bytes_core(LearnerCore& c, uint64_t* n);
int state_export_core(LearnerCore& c, state::Header h, void* host_dst, uint64_t n);
int state_import_core(LearnerCore& c, const state::Header& mine, const void* host_src, uint64_t n);

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
