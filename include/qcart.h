/*
 * qcart.h — C ABI of libqcart.so, the MI355X-native quantum-cartpole env.step() hot path.
 *
 * Drop-in boundary for the reference CPython extension `simulation` (one module per physical
 * system, compiled by each directory setupC.py with -D macros). Each entry point below names the reference
 * function it replaces (file:line; aliases as in SURVEY.md: HO/ IHO/ QO/ IQO/ =
 * "implementation codes/{harmonic, inverted harmonic, quartic, inverted quartic} oscillator/").
 *
 * Conventions
 *  - Plain C types only. Every psi / output pointer is a DEVICE pointer (hipMalloc'd or a torch
 *    tensor's data_ptr()) on the handle's device unless stated otherwise.
 *  - psi layout: [B][N] complex fp64, interleaved (re, im) — the numpy complex128 layout the
 *    reference takes (IHO/simulation_i.cpp:374-376), batched env-major.
 *  - All launches are asynchronous on the handle's stream (qc_set_stream; default: the null
 *    stream); qc_sync() fences.
 *  - Return value: 0 on success, < 0 on error (never aborts); qc_last_error() explains.
 *    Reference counterpart: Python exceptions (TypeError/ValueError/RuntimeError,
 *    IHO/simulation_i.cpp:340-372, QO/simulation_quart.cpp:288-323, :517).
 */
#ifndef QCART_H
#define QCART_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QC_ABI_VERSION 1

/* physical systems (one reference directory each) */
enum qc_family {
    QC_HO = 0,   /* harmonic cooling, Fock basis, H = omega (n + 1/2)       HO/simulation.cpp        */
    QC_IHO = 1,  /* inverted harmonic cartpole, H = -omega/2 (a+^2 + a^2)   IHO/simulation_i.cpp     */
    QC_QO = 2,   /* quartic cooling, 8th-order FD grid, lambda > 0          QO/simulation_quart.cpp  */
    QC_IQO = 3   /* inverted quartic cartpole, lambda < 0                   IQO/simulation_quart.cpp */
};

/* semantics of the dt^3..dt^6 correction product term7 = A . D1 */
enum qc_a_mode {
    QC_A_REFERENCE = 0, /* the reference's MKL descriptor: IHO HERMITIAN/UPPER mirror, others exact */
    QC_A_EXACT = 1      /* the intended complex-symmetric A                                          */
};

enum qc_status {
    QC_OK = 0,
    QC_EINVAL = -1,     /* bad argument / shape (reference: ValueError)                 */
    QC_ENOMEM = -2,
    QC_EHIP = -3,       /* HIP runtime error                                            */
    QC_EPIVOT = -4,     /* band LU would need row interchanges       */
    QC_ESINGULAR = -5,
    QC_ENOTBUILT = -6   /* no kernel instantiated for this (family, N)                  */
};

/* Runtime replacement of setupC.py's compile-time macros (HO/setupC.py:49, QO/setupC.py:55)
 * plus the per-call step() arguments dt / gamma that are fixed for a batch. */
/* working precision of the step (psi storage and arithmetic) */
enum qc_precision { QC_FP64 = 0, QC_FP32 = 1 };

typedef struct qc_params {
    int32_t family;        /* enum qc_family                                                     */
    int32_t n_max;         /* Fock: N = n_max + 1  (N_MAX macro)                                 */
    double omega;          /* Fock: OMEGA macro (the drivers pass pi)                           */
    double x_max;          /* grid: X_MAX;  x_n = 2*int(x_max/grid_size + 0.5) + 1              */
    double grid_size;      /* grid: GRID_SIZE (h)                                                */
    double lambda_;        /* grid: LAMBDA (already multiplied by pi, IQO/main_parallel.py:29)  */
    double mass;           /* grid: MASS (already divided by pi)                                 */
    int32_t moment_order;  /* grid: MOMENT macro (default 5 -> 20 observables); 1..16: up to 9 */
                           /* one observable per lane of the env's 64-lane wave, above that   */
                           /* up to 3 per lane ((2+m+1)m/2 <= 152) (QO/setupC.py:16,38        */
                           /* compiles any m >= 1; m >= 17 is refused, QC_EINVAL; the step    */
                           /* server serves m <= 9)                                           */
    int32_t a_mode;        /* enum qc_a_mode                                                     */
    double gamma;          /* measurement strength (step() argument; the drivers pass args.gamma*pi) */
    double dt;             /* time step (step() argument; 1/time_steps)                         */
    double f_max;          /* action -> force map F = (a - 10) * f_max / 10 (IHO/RL.py:107-111)  */
    int32_t n_actions;     /* 21 (2*10 + 1, IHO/RL.py:81,94)                                     */
    int32_t precision;     /* enum qc_precision: 0 fp64 (default, the reference's), 1 fp32 (config C5;
                              Fock families; psi buffers are then complex64)                     */
    int64_t batch;         /* B envs held by this handle (this rank's shard)                   */
    int64_t env_offset;    /* global id of env 0 (multi-GPU sharding keeps noise invariant)    */
    uint64_t seed;         /* Philox key (QC_NOISE_PHILOX; MT19937: qc_set_seed_mt19937)       */
    double xth;            /* IQO per-step outside-probability window half-width (0 = off)      */
} qc_params;

typedef struct qc_handle qc_handle;

/* Module init: Set_World ctor + PyInit (IHO/simulation_i.cpp:26-151, :643-653;
 * QO/simulation_quart.cpp:28-209). Builds the operator bands and the per-action factor tables
 * (reset_ab, IHO:227-277 / QO:394-432) for all n_actions forces on `device`. */
int qc_create(const qc_params* p, int device, qc_handle** out);
void qc_destroy(qc_handle* h);
const char* qc_last_error(const qc_handle* h);   /* h may be NULL: last qc_create failure */
int qc_abi_version(void);

/* check_settings() (IHO/simulation_i.cpp:581-583, QO/simulation_quart.cpp:652-654) */
int qc_get_params(const qc_handle* h, qc_params* out);
int qc_dim(const qc_handle* h);                  /* N = n_max+1 or x_n */
int qc_n_obs(const qc_handle* h);                /* 5 (Fock 'xp') or (2+m+1)*m/2 (grid) */

/* Stream binding (a hipStream_t passed as void*; NULL = default stream). */
int qc_set_stream(qc_handle* h, void* stream);
int qc_sync(qc_handle* h);

/* Noise of the stochastic step (the two N(0,1) draws per go_one_step, IHO/simulation_i.cpp:435).
 * Two sources, per handle:
 *   QC_NOISE_PHILOX   (default) counter-based Philox4x32-10 keyed by (seed, env_offset + e); env e's
 *                     counter is its own: it starts at 0 and advances by the steps env e takes, so an
 *                     env's trajectory never depends on the other envs of the handle or on sharding.
 *   QC_NOISE_MT19937  the reference's stream: set_seed(seed) = vslNewStream(VSL_BRNG_MT19937, seed) +
 *                     vdRngGaussian(VSL_RNG_METHOD_GAUSSIAN_BOXMULLER) (IHO/simulation_i.cpp:574-579,
 *                     :435), one stream per env (the reference runs one env per process with its own
 *                     seed, IHO/main_parallel.py:173-178,358): init_by_array({seed}), two words per
 *                     normal, x = sqrt(-2 ln u1) sin(2 pi u2), u = word * 2^-32 — MKL's uniform bits
 *                     exactly and its Gaussians to <= 1 ulp of the MKL_CBWR=COMPATIBLE path
 *                     (tests/golden/mkl_*.npz; MKL's default vector-math path differs by <= 5e-8).
 * An injected `noise` array in qc_step overrides both and advances neither stream. */
enum qc_noise_mode { QC_NOISE_PHILOX = 0, QC_NOISE_MT19937 = 1 };

/* set_seed(int) (IHO/simulation_i.cpp:574-579), Philox mode: re-keys the counter-based noise and resets
 * every env's counter to 0. */
int qc_set_seed(qc_handle* h, uint64_t seed);
/* set every env's Philox counter to `step` / read env 0's counter (synchronises) */
int qc_set_step_counter(qc_handle* h, uint64_t step);
uint64_t qc_get_step_counter(const qc_handle* h);
/* per-env Philox counters (device uint64 [B]): copied to `out` and/or replaced from `in` (either may be
 * NULL; checkpoint / resume of a batch) */
int qc_env_counters(qc_handle* h, uint64_t* out, const uint64_t* in);
/* set_seed for every env in MT19937 mode: seeds device uint32 [B], env e's stream
 * vslNewStream(VSL_BRNG_MT19937, seeds[e]) */
int qc_set_seed_mt19937(qc_handle* h, const uint32_t* seeds);
/* set_seed for the envs with mask[e] != 0 only (mask: device uint8 [B]); the others keep their streams — one
 * actor process's set_seed under the step server (qc_server_*). Needs the handle in MT19937 mode. */
int qc_set_seed_mt19937_envs(qc_handle* h, const uint32_t* seeds, const uint8_t* mask);
int qc_noise_mode(const qc_handle* h);
/* the next normals of every env's MT19937 stream (the reference's vdRngGaussian draws, IHO/simulation_i.cpp:435)
 * into `noise` (device double [n_steps][B][2], qc_step's injected layout): min(n_steps, env_steps[e]) steps for env e (env_steps NULL: n_steps each), the stream advancing by the
 * words drawn — what qc_step draws itself when it is given no noise. With pre / has_pre (device double [B][2], uint8
 * [B]; both or neither) an env with has_pre[e] != 0 has already drawn its next step's pair into pre[e] (an earlier
 * call with n_steps = 1): it becomes step 0 and only the remaining steps are drawn. The step server prefetches each
 * env's next pair this way after a tick, off the next tick's critical path. */
int qc_mt19937_normals(qc_handle* h, int32_t n_steps, const int32_t* env_steps, const double* pre,
                       const uint8_t* has_pre, double* noise);
/* per-env MT19937 states (device uint32 [B][qc_mt19937_words()]: 624 state words, read index, pad):
 * copied to `out` and/or replaced from `in` */
int qc_mt19937_state(qc_handle* h, uint32_t* out, const uint32_t* in);
int qc_mt19937_words(void);

/* Change dt / gamma (step()'s per-call arguments; reset_ab on dt change, IHO:377-383). */
int qc_set_dynamics(qc_handle* h, double dt, double gamma);

/* Register an arbitrary force (step(state, dt, force, gamma) with a force off the 21-level grid,
 * e.g. the reference's analytic controllers before rounding). Returns a slot >= n_actions usable
 * as an action index, or < 0. Slots are cached by force value. */
int qc_add_force(qc_handle* h, double force);

/*
 * step() / simulate_10_steps() (IHO/simulation_i.cpp:358-421, HO/simulation.cpp:339-402,
 * QO/simulation_quart.cpp:493-558), batched and fused over n_steps physics steps:
 *   psi       [B][N] complex128, advanced in place (the reference mutates `state` in place).
 *   actions   [B] int32 action index per env (0..n_actions-1 or a qc_add_force slot);
 *             NULL -> every env uses `default_action`.
 *   env_steps [B] int32 per-env step budget: env e advances min(n_steps, env_steps[e]) steps (0 =
 *             frozen, e.g. a finished episode awaiting reset); NULL -> n_steps for every env.
 *   noise     [n_steps][B][2] fp64 N(0,1) draws to inject (parity tests), or NULL for the handle's
 *             stream (qc_noise_mode: in-kernel Philox keyed by (seed, env_offset + e, env e's counter),
 *             or env e's MT19937); only the first min(n_steps, env_steps[e]) steps of env e are read.
 *   q_out, xmean_out  [n_steps][B] per-step (q, x_mean) outputs of step(), or NULL.
 *   fail_step [B]: 1-based index of the first step after which Fail (check_boundary_error) held,
 *             0 if none; NULL to skip.
 *   term_step [B]: IQO outside-probability criterion (IQO/main_parallel.py:78-81,199-200) on the
 *             states before each step and after the last: first k in [0, n_steps] with
 *             P_out > 0.5, -1 if none; requires params.xth > 0; NULL to skip.
 *   obs_out   [B][n_obs] fp64 observation of the final state (same as qc_moments), or NULL.
 * Env e's noise stream advances by the min(n_steps, env_steps[e]) steps it takes.
 */
int qc_step(qc_handle* h, void* psi, const int32_t* actions, int32_t default_action, int32_t n_steps,
            const int32_t* env_steps, const double* noise, double* q_out, double* xmean_out, int32_t* fail_step,
            int32_t* term_step, double* obs_out);

/* Step-kernel timing (measurement, bench.py): with timing on, every qc_step records a HIP event pair on the
 * handle's stream around its k_step launch only (not the grouping or noise kernels); qc_step_kernel_time
 * synchronises the stream and returns the summed kernel time and the number of launches since the last
 * call (then restarts the count). */
int qc_set_timing(qc_handle* h, int on);
int qc_step_kernel_time(qc_handle* h, double* total_ms, int64_t* launches);

/* get_moments(state, out) (QO/simulation_quart.cpp:363-388) for grids; the Fock 'xp' vector
 * get_data_xp (IHO/main_parallel.py:129-131) for HO/IHO. out [B][n_obs] fp64. */
int qc_moments(qc_handle* h, const void* psi, double* out);

/* x_expectation(state) (IHO/simulation_i.cpp:204-215, QO/simulation_quart.cpp:244-258): out [B] */
int qc_x_expectation(qc_handle* h, const void* psi, double* out);

/* calculate_outside_probability(state, xth) (IQO/main_parallel.py:78-81): out [B] */
int qc_outside_prob(qc_handle* h, const void* psi, double xth, double* out);

/* check_boundary_error (IHO/simulation_i.cpp:422-426, QO/simulation_quart.cpp:559-565): out [B] */
int qc_boundary_fail(qc_handle* h, const void* psi, int32_t* out);

/* cal_energy(state, Hamil) (QO/main_parallel.py:52-53, quartic reward) = Re<psi|H|psi> w with the
 * force-free H: out [B] */
int qc_energy(qc_handle* h, const void* psi, double* out);

/* Hamiltonian_dot_psi(state) (IHO/simulation_i.cpp:585-601, HO/simulation.cpp:566-582): psi <- H psi in place for
 * every env, H the force-free Hamiltonian (mkl_sparse_z_mv of harmonic_Hamil; grid families: their kinetic +
 * potential H, which the reference's grid modules do not export) */
int qc_hamiltonian_dot_psi(qc_handle* h, void* psi);

/* phonon_number(state) (HO/main_parallel.py:88-89, harmonic-cooling reward) = sum n |psi_n|^2: out [B] */
int qc_phonon_number(qc_handle* h, const void* psi, double* out);

/* get_data_wavefunction (args.input == 'wavefunction'): hstack(Re, Im) of state[:-10] (HO,
 * HO/main_parallel.py:132-134), state[:-20] (IHO, IHO/main_parallel.py:133-135) or state[10:-10] (grid,
 * QO/main_parallel.py:132-133, IQO/main_parallel.py:136-137), cast to float32 and
 * times input_scaling in float32 (IHO:241,247): out [B][qc_wavefunction_len()] float32 (device) */
int qc_wavefunction_len(const qc_handle* h);
int qc_wavefunction_obs(qc_handle* h, const void* psi, double input_scaling, float* out);

/* Episode reset of psi for envs with mask[e] != 0 (mask NULL = all; device uint8 [B]):
 *   QC_RESET_GROUND   Fock |0> (IHO/main_parallel.py:231-232, HO/main_parallel.py:226-227)
 *   QC_RESET_RANDOM   Fock: normalised complex Gaussian amplitudes on levels < arg0 (synthetic
 *                     benchmark input), Philox stream tag 1 keyed by global env id
 *   QC_RESET_GAUSSIAN grid: Gaussian_packet(wavelength=1/k, mean, std) (IQO/main_parallel.py:75-76,
 *                     182-183) with per-env k/mean/std (device fp64 [B] arrays, may be NULL ->
 *                     arg0/arg1/arg2 scalars) */
enum qc_reset_kind { QC_RESET_GROUND = 0, QC_RESET_RANDOM = 1, QC_RESET_GAUSSIAN = 2 };
int qc_reset(qc_handle* h, void* psi, int32_t kind, const uint8_t* mask, double arg0, double arg1,
             double arg2, const double* k_arr, const double* mean_arr, const double* std_arr);

/* Analytic baseline controllers, one action per env from the current state:
 *   QC_CTL_LQG           Fock: the actor's args.LQG branch of call_force (IHO/main_parallel.py:194-206,
 *                        HO/main_parallel.py:192-203) on the network input data = float32 get_data_xp(state)
 *                        * input_scaling (pass 1.0 for the unscaled get_data_xp of a non-'xp' input,
 *                        IHO/main_parallel.py:261-262); control_time = 1 / n_con.
 *                        grid: controllers.LinearQuadratic(state, k = lambda_ * con_parameter)
 *                        (QO/controllers.py:16-20, QO/main_parallel.py:168)
 *   QC_CTL_DAMPING       grid: controllers.steepest_descent(state, damping = con_parameter) (:7-14)
 *   QC_CTL_SEMICLASSICAL grid: controllers.Gaussian_approx(state) (:22-29)
 * Grid forces use the drivers' space_def operators (full Delta_1 p_hat) and control_time =
 * 1 / controls_per_unit_time; force = F / pi (Fock: F / omega) is clipped to +-F_max and rounded to the
 * action grid with Python round() semantics (analytic_controls, QO/main_parallel.py:170-181).
 * actions [B] int32 (device) receive round(force / spacing) + n_actions/2; force_out [B] fp64 (optional)
 * the rounded force passed to step(). A NaN force (Gaussian_approx with a negative root argument,
 * where the reference raises a math domain error) yields action -1 and force NaN. */
enum qc_control_strategy { QC_CTL_LQG = 0, QC_CTL_DAMPING = 1, QC_CTL_SEMICLASSICAL = 2 };
int qc_control(qc_handle* h, const void* psi, int32_t strategy, double con_parameter, double control_time,
               double input_scaling, int32_t* actions, double* force_out);

/* Measurement-record input mode: args.input == 'measurements' of the Fock drivers
 * (IHO/main_parallel.py:143-151,270-309; HO/main_parallel.py:142-150,259-292), for B envs in place on
 * the device. Per env (device float32):
 *   hist   [B][2][read_length]  the network input np.array([measurements_input[::-1],
 *                               forces_along_measurements_input[::-1]]): measurements newest first, and
 *                               force * input_scaling applied during each
 *   forces [B][K + 1]           forces_to_store after the control step's append, newest first,
 *                               K = read_length / m, m = n_steps / coarse_grain
 * One call closes one control interval of n_steps physics steps: q [n_steps][B] fp64 are the q outputs of
 * qc_step for it (q_out), actions [B] (or default_action) the actions applied during it. Each group of
 * coarse_grain steps adds sum(q) / coarse_grain * input_scaling; the histories shift by m.
 * mode [B] (device uint8, NULL = all 1): 0 leaves the env untouched, 1 records, 2 records into a fresh
 * (zero) history (a new episode, IHO:271-272). rows [B][qc_record_row_len()] (optional) receive the
 * experience row hstack(measurements_input[::-1] (read_length + m), forces_to_store[::-1] (K + 1),
 * last_action, reward) (IHO:279-283, TrainDQN reads it at RL.py:180-192); the reward column is written
 * only when reward [B] is given. The drivers' values: read_length = round(n_periods * 2 * 1440) with
 * n_periods 2 (IHO, 5760) or 1.5 (HO, 4320), coarse_grain = time_steps / 1440. An out-of-range action
 * is clamped on the device and raises the handle's error word: the next qc_take_errors reports it (as for
 * qc_step). */
int qc_record_row_len(int32_t read_length, int32_t interval, int32_t coarse_grain);
int qc_record(qc_handle* h, int32_t read_length, int32_t coarse_grain, double input_scaling, const double* q,
              int32_t n_steps, const int32_t* actions, int32_t default_action, const uint8_t* mode, float* hist,
              float* forces, const float* reward, float* rows);

/* Host-side introspection of the factor tables (tests): number of Kogge-Stone levels kept for
 * action a (forward, backward), and the truncation bound used. */
int qc_scan_levels(const qc_handle* h, int32_t action, int32_t* fwd, int32_t* bwd);

/* Deferred input errors: qc_step does not synchronise to validate its actions; an action outside
 * [0, n_slots) of an env with a step budget raises a device error word (the kernels clamp it). This call
 * synchronises the handle's stream, returns QC_EINVAL (message via qc_last_error) if any qc_step since the
 * last call saw such an action, and clears the word; QC_OK otherwise. */
int qc_take_errors(qc_handle* h);

/* Introspection (tests, diagnostics): the workgroup layout of the last grouped qc_step call (k_group).
 * Copies up to order_len entries of the single-slot workgroup list and up to mixed_len of the two-slot list
 * (workgroups of qc_step_group_size() envs each, -1 = idle wave) into host buffers (either may be NULL) and
 * returns the number of two-slot workgroup slots (0 when the handle does not use them). Synchronises. */
int qc_step_group_size(const qc_handle* h);
int qc_group_layout(qc_handle* h, int32_t* order, int64_t order_len, int32_t* mixed, int64_t mixed_len);

/* ---------------------------------------------------------------------------------------------
 * Batched DQN actor: the reference's direct_DQN action selection
 * (inverted harmonic oscillator/RL.py:80-111 + layers.py FactorizedNoisy / Linear_weight_normalize),
 * evaluated for B envs at once on the device, with the actor's epsilon-greedy choice
 * (IHO/main_parallel.py:208-219), replacing the per-actor pipe to the inference process
 * (IHO/main_parallel.py:414-440). Layers: fc1 (in -> 512), fc2 (512 -> H2), fc31 (H2 -> 256),
 * fc41 (256 -> n_actions), ReLU between; actions = argmax of fc41 (the mean branch fc32/fc42 does not
 * enter the action). H2 = 256 is the harmonic and inverted harmonic drivers' net, H2 = 512 the quartic and
 * inverted quartic drivers' (their RL.py:87-93); it is fixed at create. fp32 throughout (the reference
 * net's dtype), f32-input MFMA. */
typedef struct qc_actor qc_actor;

typedef struct qc_dqn_params {
    int32_t data_length;   /* network input length in [1, 1024]: 5 for the 'xp' input (IHO/main_parallel.py:137-138);
                              the 'wavefunction' input's 2 (kept rows of psi): 122 (HO), 302 (QO), 322 (IHO), 1002
                              (IQO) at the drivers' defaults. Above 512 fc1 runs over the input in chunks of 512 */
    int32_t n_actions;     /* 21 */
    int64_t max_batch;     /* largest B passed to qc_actor_act */
    uint64_t seed;         /* Philox key of the NoisyNet noise and the epsilon-greedy draws */
    int32_t hidden2;       /* H2, fc2's width: 0 or 256, or 512; anything else is QC_EINVAL */
} qc_dqn_params;

/* One layer's parameters (device fp32 pointers, the reference state_dict tensors):
 * Linear_weight_normalize: weight [out][in], bias [out], weight_norm (scalar g; effective weight
 *   W g / ||W||_F, layers.py:97-103); sigma_w = sigma_b = NULL.
 * FactorizedNoisy: weight = u_w [out][in], bias = u_b, sigma_w [out][in], sigma_b [out],
 *   weight_norm = NULL (layers.py:7-79). */
typedef struct qc_dqn_layer {
    const float* weight;
    const float* bias;
    const float* weight_norm;
    const float* sigma_w;
    const float* sigma_b;
} qc_dqn_layer;

int qc_actor_create(const qc_dqn_params* p, int device, qc_actor** out);
void qc_actor_destroy(qc_actor* a);
const char* qc_actor_last_error(const qc_actor* a);
int qc_actor_set_stream(qc_actor* a, void* stream);
/* (re)load fc1, fc2, fc31, fc41 (the trainer's periodic state_dict push, IHO/main_parallel.py:400-405):
 * computes the effective weights and stores them in the kernels' fragment order on the device */
int qc_actor_load(qc_actor* a, const qc_dqn_layer layers[4]);

/* Noise of the factorised noisy layers per env: eps_in(fc31)[H2], eps_out(fc31)[256],
 * eps_in(fc41)[256], eps_out(fc41)[n_actions], each f(z) = sign(z) sqrt|z| of a standard normal z
 * (layers.py:77-79): qc_actor_noise_len() = H2 + 512 + n_actions floats per env (789 / 1045 at 21 actions). */
int qc_actor_noise_len(const qc_actor* a);

/* One action per env: obs [B][data_length] fp32 (device): the network input exactly as the actor hands it
 * over (get_data(state) * input_scaling in float32, IHO/main_parallel.py:131,241,247; BatchedEnv.obs),
 * actions [B] int32 (device). noisy = 0 evaluates the mean weights
 * (layers.py:41-43); noise NULL draws the NoisyNet noise in-kernel (Philox keyed by seed and
 * env_offset + e, counter `counter`), else injected [B][noise_len] fp32. With probability eps an env
 * takes a uniform random action instead (random_out[e] = 1). q_out [B][n_actions] fp32 and
 * random_out [B] int32 are optional. */
int qc_actor_act(qc_actor* a, int64_t B, int64_t env_offset, const float* obs, int32_t noisy,
                 const float* noise, double eps, uint64_t counter, int32_t* actions, float* q_out,
                 int32_t* random_out);

/* The measurement-input actor (SURVEY §8f rank 1 for args.input == 'measurements'): DQN_measurement
 * (inverted harmonic oscillator/RL.py:29-78) for B envs: conv1 Conv1d(2, 32, 13, stride 5), conv2
 * Conv1d(32, 64, 11, 4), conv3 Conv1d(64, 64, 9, 4) with ReLU, flatten, fc1 Linear(64 T3, 256) + ReLU,
 * fc21 FactorizedNoisy(256, 256) + ReLU, fc31 FactorizedNoisy(256, n_actions) -> argmax, epsilon-greedy;
 * the harmonic driver's net is the same with weight-normalised convolutions (qc_mactor_load).
 * The convolutions run as implicit GEMMs on f32 MFMA over env chunks; the noise layout and the
 * epsilon-greedy draw are qc_actor's (noise_len = 789 at 21 actions). */
typedef struct qc_mdqn_params {
    int32_t read_length;   /* network input length per channel (5760 IHO, 4320 HO; MeasurementRecord) */
    int32_t n_actions;     /* 21 */
    int64_t max_batch;
    uint64_t seed;
    int32_t chunk;         /* envs per convolution chunk (0: 2048) */
} qc_mdqn_params;
typedef struct qc_mactor qc_mactor;
int qc_mactor_create(const qc_mdqn_params* p, int device, qc_mactor** out);
void qc_mactor_destroy(qc_mactor* a);
const char* qc_mactor_last_error(const qc_mactor* a);
int qc_mactor_set_stream(qc_mactor* a, void* stream);
int qc_mactor_noise_len(const qc_mactor* a);
int qc_mactor_flat_len(const qc_mactor* a);   /* 64 * T3, fc1's input length */
/* layers[6] = conv1, conv2, conv3, fc1 (weight [out][in(*kernel)], bias; sigma = NULL), fc21, fc31
 * (FactorizedNoisy u_w/u_b/sigma_w/sigma_b, or Linear_weight_normalize) — the state_dict. A convolution whose
 * weight_norm is not NULL is a Conv1d_weight_normalize layer (the harmonic driver's stack, harmonic
 * oscillator/RL.py:29-75, layers.py:86-94): its effective weight is W g / ||W||_F with the one scalar g, each of
 * conv1..3 decided by its own pointer. fc1 is nn.Linear in every driver: a weight_norm on it is refused. */
int qc_mactor_load(qc_mactor* a, const qc_dqn_layer layers[6]);
/* obs [B][2][read_length] fp32 (device): the network input (MeasurementRecord.hist); the rest as
 * qc_actor_act */
int qc_mactor_act(qc_mactor* a, int64_t B, int64_t env_offset, const float* obs, int32_t noisy,
                  const float* noise, double eps, uint64_t counter, int32_t* actions, float* q_out,
                  int32_t* random_out);

/* ---------------------------------------------------------------------------------------------
 * Prioritized experience replay on the device: the reference's SumTree + Memory
 * (inverted harmonic oscillator/RL.py:234-475), fed by BatchedEnv without leaving HBM.
 * Layout as the reference: tree float64 [n_nodes + capacity] heap-indexed, leaf of slot d at n_nodes + d;
 * data float32 [capacity][row_len]. All pointers below are device pointers; calls are asynchronous on
 * the memory's stream (qc_replay_stats synchronises). */
typedef struct qc_replay qc_replay;

typedef struct qc_replay_params {
    int64_t capacity;             /* round(size_of_replay_memory * n_con * 100) (IHO/main_parallel.py:595) */
    int32_t row_len;              /* data_size of one row: 2 * obs_len + 2 ('xp'), qc_record_row_len ('measurements') */
    int32_t policy;               /* 0 'sequential', 1 'random' (the drivers: 'random', main_parallel.py:598) */
    double passes_before_random;  /* 0.2 (main_parallel.py:598); SumTree.passes starts at minus this */
    double alpha;                 /* 0.2  Memory.alpha (RL.py:372)                    */
    double beta;                  /* 0.2  Memory.beta, initial (RL.py:373)            */
    double beta_increment;        /* 0.001 per sample (RL.py:374)                     */
    double abs_err_upper;         /* 1.0 (RL.py:375)                                  */
    double epsilon_scale;         /* 1e-5: epsilon = 1e-5 * max (RL.py:442)           */
    uint64_t seed;                /* Philox key: random-policy positions, sampling uniforms */
} qc_replay_params;

typedef struct qc_replay_stats_t {
    int64_t len;                  /* len(memory) (RL.py:415-416)  */
    int64_t data_pointer;
    double passes;
    double max;                   /* Memory.max                    */
    double beta;                  /* Memory.beta after the last sample */
    double total_p;               /* SumTree.total_p = tree[0]     */
    int64_t n_nodes, tree_size;
} qc_replay_stats_t;

int qc_replay_create(const qc_replay_params* p, int device, qc_replay** out);
void qc_replay_destroy(qc_replay* r);
const char* qc_replay_last_error(const qc_replay* r);   /* r may be NULL: last create failure */
int qc_replay_set_stream(qc_replay* r, void* stream);
/* Memory.store for each row e < n with valid[e] != 0 (valid NULL = all), in index order (RL.py:417-420,
 * SumTree.add :273-288): priority max (or abs_err_upper while max == 0); 'sequential' slots while
 * passes < 1, then random slots (Philox); a slot hit twice in one call keeps the later row. */
int qc_replay_store(qc_replay* r, int64_t n, const uint8_t* valid, const float* rows /*[n][row_len]*/);
/* the same, assembling the 'xp' experience row np.hstack((last_data, data, [last_action], [reward]))
 * (IHO/main_parallel.py:250-257) from its parts: last_obs/obs [n][obs_len] fp32, action [n] int32,
 * reward [n] fp32; row_len must be 2 * obs_len + 2 */
int qc_replay_store_xp(qc_replay* r, int64_t n, const uint8_t* valid, const float* last_obs, const float* obs,
                       int32_t obs_len, const int32_t* action, const float* reward);
/* Memory.obtain_sample(n) / compiled_sampling (RL.py:423-432, :449-469): beta += increment (max 1),
 * stratified v_i = (i + u_i) * total / n with u [n] injected (NULL: Philox), tree_idx [n] int32 leaf
 * indices, is_weights [n] fp32 = (p / (total / len))^-beta, transitions [n][row_len] fp32 (NULL: skip the
 * gather). Requires len >= 1 (the reference returns nothing while len < n). */
int qc_replay_sample(qc_replay* r, int32_t n, const double* u, float* transitions, int32_t* tree_idx,
                     float* is_weights);
/* Memory.batch_update (RL.py:438-446, :471-475): abs_errors [n] fp32 (the per-sample losses); a tree_idx
 * outside the leaves [n_nodes, n_nodes + capacity) is skipped (no write, no ancestor update) */
int qc_replay_update(qc_replay* r, int32_t n, const int32_t* tree_idx, const float* abs_errors);
/* Memory.clean / recalculate_structure (RL.py:312-331, :421-422): every parent recomputed */
int qc_replay_rebuild(qc_replay* r);
int qc_replay_stats(qc_replay* r, qc_replay_stats_t* out);
/* device pointers of the tree and the row storage (introspection, tests) */
int qc_replay_buffers(const qc_replay* r, const double** tree, const float** data);

/* ---------------------------------------------------------------------------------------------
 * Device DQN learner: the reference's TrainDQN.__call__ (inverted harmonic oscillator/RL.py:159-232)
 * with its LaProp optimizer (optimizer.py; centered, betas (0.9, 0.9995), eps 1e-15, RL.py:145) for the
 * 'xp' network direct_DQN(data_length, noisy_layers = 2): fc1, fc2, fc31 (noisy), fc41 (noisy) and the mean
 * head fc32, fc42, fp32 throughout on f32-input MFMA. fc2's width H2 (hidden2), the TD target (target_mode)
 * and LaProp's betas are what the reference's four drivers differ in; the zero defaults are the inverted
 * harmonic driver's (H2 = 256, QC_TD_ALIVE, betas (0.9, 0.9995)). One update: the target network follows the online
 * one when backup_counter == 0, then backup_counter = (backup_counter + 1) % backup_period; double-DQN
 * target a* = argmax Q_online(next), sav = Q(prev)[a] + m(prev) - mean Q(prev), nsv the same of the target
 * net at a*, the target y by target_mode (below), ul = (sav - y)^2,
 * loss = mean(ul w); backward through the online pass on prev; one LaProp step. The NoisyNet noise is
 * FactorizedNoisy's batched branch (layers.py:57-74): the batch is 32 contiguous chunks of B / 32 rows,
 * one (eps_in, eps_out) pair per chunk and noisy layer, shared by the three forward passes. That branch
 * needs B % 128 == 0; other batch sizes (the reference's per-row branch) are refused with QC_EINVAL.
 * Gradients use no atomics: the same inputs give bit-identical parameters. All pointers are device
 * pointers; every call is asynchronous on the learner's stream except qc_learner_stats. */
typedef struct qc_learner qc_learner;
/* The TD target y of a row with reward r (the last column of a transition):
 *   QC_TD_ALIVE        y = gamma nsv + (1 - gamma) alive_reward; y = 0 where r == failing_reward (IHO, IQO)
 *   QC_TD_REWARD_FAIL  y = gamma nsv + (1 - gamma) r;            y = r where r <= failing_reward (QO)
 *   QC_TD_REWARD       y = gamma nsv + (1 - gamma) r             (HO; alive_reward / failing_reward unused) */
enum { QC_TD_ALIVE = 0, QC_TD_REWARD_FAIL = 1, QC_TD_REWARD = 2 };
typedef struct qc_learner_params {
    int32_t data_length, n_actions; /* data_length in [1, 1024], as qc_dqn_params ('xp': 5; 'wavefunction': up to 1002) */
    int32_t batch_size;            /* multiple of 128, <= 4096 */
    int32_t backup_period;
    double gamma, lr, alive_reward, failing_reward;
    uint64_t seed;                 /* Philox key of the in-kernel noise */
    int32_t hidden2;               /* H2, fc2's width: 0 or 256, or 512 (as qc_dqn_params) */
    int32_t target_mode;           /* QC_TD_*; others are QC_EINVAL */
    double beta1, beta2;           /* LaProp's betas in [0, 1); 0: 0.9 and 0.9995 */
} qc_learner_params;

typedef struct qc_learner_stats_t {
    int64_t updates;               /* qc_learner_update calls */
    int64_t step;                  /* LaProp state['step'] */
    int64_t nonfinite;             /* updates whose loss was not finite (the reference's NaN assert, RL.py:230) */
    double l1, l2, lr;             /* exp_avg_lr_1, exp_avg_lr_2, the current lr */
    int32_t backup_counter;
    int32_t launches_per_update;   /* kernel launches + copies of the last update */
} qc_learner_stats_t;

int qc_learner_create(const qc_learner_params* p, int device, qc_learner** out);
void qc_learner_destroy(qc_learner* l);
const char* qc_learner_last_error(const qc_learner* l);   /* l may be NULL: last create failure */
int qc_learner_set_stream(qc_learner* l, void* stream);
int qc_learner_noise_len(const qc_learner* l);            /* qc_actor_noise_len's layout, per chunk */
/* layers[6] = fc1, fc2, fc31, fc41, fc32, fc42 (the state_dict tensors, as qc_actor_load); resets the
 * optimizer state and backup_counter */
int qc_learner_load(qc_learner* l, const qc_dqn_layer layers[6]);
/* device pointers to the learner's own natural-layout parameters (target != 0: the target network's):
 * qc_actor_load takes out[0..3] as they are, so the weight push is device to device */
int qc_learner_layers(qc_learner* l, int target, qc_dqn_layer out[6]);
/* transitions [B][2 data_length + 2] (prev, next, action as float, reward), is_weights [B], noise
 * [32][noise_len] already f-transformed (NULL: Philox keyed by seed, chunk, counter), unweighted_loss [B]
 * (out, the per-sample losses for qc_replay_update), loss: optional device scalar (out). An action outside
 * [0, n_actions) is clamped on the device and reported by the next qc_learner_stats. */
int qc_learner_update(qc_learner* l, const float* transitions, const float* is_weights, const float* noise,
                      uint64_t counter, float* unweighted_loss, float* loss);
int qc_learner_set_lr(qc_learner* l, double lr);
/* the target network's period from the next update on (Main_System's temporary 100 before learning starts,
 * IHO/main_parallel.py:480-481, 546-547); backup_counter is reduced modulo the new period. The state header keeps
 * the create-time value; the period in use travels in the payload. A learner on which this is never called
 * behaves, and exports, exactly as before. */
int qc_learner_set_backup_period(qc_learner* l, int32_t period);
/* synchronises the stream; QC_EINVAL (once, message via qc_learner_last_error) if an update since the last
 * call saw an out-of-range action, with *out filled either way */
int qc_learner_stats(qc_learner* l, qc_learner_stats_t* out);
/* introspection (tests): device pointers to the gradients of the last update, same shapes (the
 * weight_norm slot holds dg); and one LaProp step on injected gradients */
int qc_learner_grads(qc_learner* l, qc_dqn_layer out[6]);
int qc_learner_apply(qc_learner* l, const qc_dqn_layer grads[6]);

/* ---------------------------------------------------------------------------------------------
 * Device learner of the measurement-input network: one TrainDQN.__call__ update (RL.py:159-232) of
 * DQN_measurement (RL.py:29-78), the inverted harmonic driver's or (conv_weight_norm = 1) the harmonic driver's:
 * Conv1d(2, 32, 13, /5) -> (32, 64, 11, /4) -> (64, 64, 9, /4), ReLU each, flatten, Linear(64 T3, 256) + ReLU, fc21 / fc31 FactorizedNoisy, the mean head
 * fc22 / fc32 Linear_weight_normalize; centred LaProp, fp32 throughout on f32-input MFMA, the loss and the noise
 * as qc_learner (H2 = 256). A transition is a row of qc_record: K = read_length / read_step_length,
 *   row = [measurements (read_length + read_step_length, newest first) | forces (K + 1, newest first) | action | reward]
 * and the states are next[0] = row[0 : L], prev[0] = row[m : m + L], next[1][k m : (k + 1) m] = forces[k],
 * prev[1][k m : (k + 1) m] = forces[k + 1] (RL.py:180-192). Gradients use no atomics: the same inputs give
 * bit-identical parameters. All pointers are device pointers; every call is asynchronous on the handle's stream
 * except qc_mlearner_stats.
 * conv_weight_norm = 0: conv1..3 are plain Conv1d layers, and a convolution with a weight_norm is refused by name.
 * conv_weight_norm = 1: conv1..3 are Conv1d_weight_normalize layers (harmonic oscillator/RL.py:29-75,
 * layers.py:86-94; effective weight W g / ||W||_F, one scalar g per layer): qc_mlearner_load and qc_mlearner_apply
 * require a weight_norm on all three, qc_mlearner_layers and qc_mlearner_grads return it (25 tensors instead of
 * 22; in the gradients the slot holds dg, as for fc22 / fc32). fc1 with a weight_norm is refused on both. The
 * harmonic driver's handle is conv_weight_norm = 1, QC_TD_REWARD, betas (0.9, 0.999), L = 4320, m = 80. */
typedef struct qc_mlearner qc_mlearner;
typedef struct qc_mlearner_params {
    int32_t read_length;           /* L */
    int32_t read_step_length;      /* m; L % m == 0 */
    int32_t n_actions;
    int32_t batch_size;            /* multiple of 128 in [128, 1024] */
    int32_t backup_period;
    int32_t target_mode;           /* QC_TD_* */
    double gamma, lr, alive_reward, failing_reward;
    double beta1, beta2;           /* LaProp's betas in [0, 1); 0: 0.9 and 0.9995 */
    uint64_t seed;                 /* Philox key of the in-kernel noise */
    int32_t conv_weight_norm;      /* 0: plain Conv1d stack, 1: Conv1d_weight_normalize on conv1..3 */
} qc_mlearner_params;
int qc_mlearner_create(const qc_mlearner_params* p, int device, qc_mlearner** out);
void qc_mlearner_destroy(qc_mlearner* l);
const char* qc_mlearner_last_error(const qc_mlearner* l);   /* l may be NULL: last create failure */
int qc_mlearner_set_stream(qc_mlearner* l, void* stream);
int qc_mlearner_noise_len(const qc_mlearner* l);            /* per chunk, at H2 = 256: 789 at 21 actions */
/* layers[8] = conv1, conv2, conv3, fc1, fc21, fc31, fc22, fc32 (conv weights as [out][in * kernel]); resets the
 * optimizer state and backup_counter */
int qc_mlearner_load(qc_mlearner* l, const qc_dqn_layer layers[8]);
/* device pointers to the natural-layout parameters (target != 0: the target network's): qc_mactor_load takes
 * out[0..5] as they are */
int qc_mlearner_layers(qc_mlearner* l, int target, qc_dqn_layer out[8]);
/* as qc_learner_update; transitions [B][L + m + K + 3] */
int qc_mlearner_update(qc_mlearner* l, const float* transitions, const float* is_weights, const float* noise,
                       uint64_t counter, float* unweighted_loss, float* loss);
int qc_mlearner_set_lr(qc_mlearner* l, double lr);
int qc_mlearner_set_backup_period(qc_mlearner* l, int32_t period);   /* as qc_learner_set_backup_period */
int qc_mlearner_stats(qc_mlearner* l, qc_learner_stats_t* out);   /* as qc_learner_stats */
int qc_mlearner_grads(qc_mlearner* l, qc_dqn_layer out[8]);
int qc_mlearner_apply(qc_mlearner* l, const qc_dqn_layer grads[8]);
/* tests: the assembled states of a batch, next_out / prev_out [B][2][L] */
int qc_mlearner_states(qc_mlearner* l, const float* transitions, float* next_out, float* prev_out);

/* ---- checkpoint: export / import of a handle's whole state --------------------------------------------------
 * For each of the five handle kinds that hold state of their own: qc_<kind>_state_bytes gives the size n of the
 * handle's state as one host buffer now, qc_<kind>_state_export writes it (n as returned; QC_EINVAL on another n),
 * qc_<kind>_state_import reads it back into a handle created with the same params, after which every later call
 * gives bit for bit what it would have given on the exporting handle. All three synchronise the handle's stream
 * (export and import also copy between host and device before they return); host_dst / host_src are host
 * pointers. The stepper (qc_handle) needs none: qc_get_step_counter / qc_set_step_counter, qc_env_counters,
 * qc_mt19937_state, qc_noise_mode, qc_set_dynamics and qc_add_force expose its state.
 *
 * A blob is a fixed-size header and a payload. The header carries a magic, the blob format version, the handle
 * kind, the payload length and, as named fields, the handle's create-time params and the geometry derived from
 * them. Import compares every field with the receiving handle (device and stream are not part of it) and returns
 * QC_EINVAL on the first difference, qc_<kind>_last_error naming the field and both values; a truncated or padded
 * buffer, a wrong magic or kind and a newer format version are refused the same way. A refused import leaves the
 * handle exactly as it was. Importing into a handle whose qc_<kind>_load was never called is allowed and marks it
 * loaded; exporting from one is QC_EINVAL (there is nothing to save).
 *   qc_actor / qc_mactor: the prepared weights as the kernels read them (the effective weights' fragments, the
 *     padded biases; a natural-layout copy does not exist), which layers carry sigma, and the seed. The seed is
 *     taken from the blob, not compared.
 *   qc_replay: beta, the sampling counter, the device State (data_pointer, len, passes, max, the two Philox
 *     counters, the store epoch), the whole tree and the rows. Rows at and past len are left out only while State
 *     proves them never written (every add so far sequential and len < capacity), else all capacity rows are
 *     saved: the blob's size depends on the state. The owner tags are not saved (an import zeroes them; a later
 *     store's tags are above every earlier one's either way).
 *   qc_learner / qc_mlearner: updates, step, backup_counter, lr (as qc_*_set_lr left it; the create-time lr is
 *     not compared), l1, l2, the non-finite and out-of-range counters behind qc_*_stats, the parameters, the target
 *     network's, LaProp's exp_avg, exp_avg_sq and exp_mean_avg, and the prepared fragments of both networks with
 *     the weight norms, copied as they are. The gradients of the last update (qc_*_grads) are not saved: an
 *     import zeroes them. */
int qc_actor_state_bytes(qc_actor* a, uint64_t* n);
int qc_actor_state_export(qc_actor* a, void* host_dst, uint64_t n);
int qc_actor_state_import(qc_actor* a, const void* host_src, uint64_t n);
int qc_mactor_state_bytes(qc_mactor* a, uint64_t* n);
int qc_mactor_state_export(qc_mactor* a, void* host_dst, uint64_t n);
int qc_mactor_state_import(qc_mactor* a, const void* host_src, uint64_t n);
int qc_replay_state_bytes(qc_replay* r, uint64_t* n);
int qc_replay_state_export(qc_replay* r, void* host_dst, uint64_t n);
int qc_replay_state_import(qc_replay* r, const void* host_src, uint64_t n);
int qc_learner_state_bytes(qc_learner* l, uint64_t* n);
int qc_learner_state_export(qc_learner* l, void* host_dst, uint64_t n);
int qc_learner_state_import(qc_learner* l, const void* host_src, uint64_t n);
int qc_mlearner_state_bytes(qc_mlearner* l, uint64_t* n);
int qc_mlearner_state_export(qc_mlearner* l, void* host_dst, uint64_t n);
int qc_mlearner_state_import(qc_mlearner* l, const void* host_src, uint64_t n);

/* ---- batched episode loop: the per-control-step bookkeeping of Control.do_episode --------------------------
 * (IHO/main_parallel.py:242-268, IQO/main_parallel.py:190-221; the cartpoles, described first) for every env after a
 * step call of one control interval, on the device (BatchedEnv reset="deferred"): pending[e] (in) marks the envs
 * whose call was their reset interval (the zero-th step without control): their time restarts at one interval,
 * return at 0, no valid transition; an episode over at that first control step is reported with return 0 (the
 * i != control_interval guard, IHO:250). Other envs: t += interval dt, done = Fail in the interval or out of
 * bounds (IHO |<x>| > xth: |obs[e][0]| > xth; IQO: term_step[e] >= 0), reward failing_reward / 1, valid,
 * return += reward. Done envs: (return, t) appended to the ring fin [2][fin_cap + 1] at *fin_n (env order; the
 * reference's result queue, IHO:300-327) and pending[e] (out) = 1: they reset in the next call. All device
 * pointers; obs32 [B][n_obs] = float(obs) * input_scaling (NULL: skip). No host synchronisation.
 * kind == QC_HO selects the cooling accounting (HO/main_parallel.py:222-292) on quantity[e], the phonon number
 * after the step: a pending env's episode is already over iff Fail or quantity > cutoff (no truncation check at
 * the first control step, HO:240-246). Other envs: t += interval dt, done = Fail or !(quantity <= cutoff) (a NaN
 * quantity ends the episode here, not in the pending branch) or t >= t_trunc; reward = -quantity *
 * reward_multiply; valid = !done (the terminal transition of a cooling episode is not stored); return += reward
 * where valid, the product and the sum each rounded once. obs may be NULL for QC_HO when obs32 is NULL. The
 * fields after fin_n are read for QC_HO only, except rec_mode, which every kind writes when it is not NULL; a
 * struct that leaves them zero with kind QC_IHO or QC_IQO behaves as before they existed.
 * kind == QC_QO (BatchedEnv reset="warmup") is the quartic cooling accounting (QO/main_parallel.py:169-232) with a
 * rolling warm-up: QO's reset (QO:177-198: a packet of wavenumber k ~ U[-0.3, 0.3] evolved freely for U[init_lo,
 * init_hi] time units and redrawn until energy < init_energy_cutoff with no Fail) is no one-interval reset, so it
 * runs inside the step launches of the following calls, budget[e] <= interval physics steps per call (qc_step's
 * env_steps), while the other envs are controlled. The fields after rec_mode carry it; a struct that leaves them
 * zero is refused with kind QC_QO as before they existed. quantity[e] is qc_energy after the step. Per env:
 *   - warm_left[e] > 0 on entry (warming; the caller stepped it budget[e] steps at zero force): left = warm_left -
 *     budget, warm_fail |= fail_step > 0; reward 0, not done, not valid. left > 0: warm_left = left, budget =
 *     min(left, interval). left == 0 and no Fail and quantity < init_energy_cutoff (strict: a NaN rejects): the
 *     env goes live: warm_left = warm_fail = 0, t = 0, steps = 0, return = 0, budget = interval, reset_out = 1 —
 *     this call's observation is the episode's first (QO decides at i = 0, QO:208, where the energy is not
 *     checked against cutoff). Otherwise the env redraws.
 *   - live: t += interval dt, steps += interval, done = Fail or !(quantity < cutoff) or t >= t_trunc; reward =
 *     -quantity * reward_multiply; valid = !done; return += reward where valid, the product and the sum each
 *     rounded once; budget = interval. A done env is appended to the ring (return, t) in env order and redraws;
 *     its t and return keep the finished episode's values until it goes live again.
 *   - redraw: n = draws[e], draws[e] = n + 1; (w0, w1, w2, w3) = Philox4x32-10 with key (seed_lo, seed_hi) at
 *     counter (n_lo, n_hi, env_offset + e, 0x400); u_k = ((w0 << 32 | w1) >> 11) 2^-53, u_t likewise from (w2,
 *     w3); k[e] = u_k 0.6 - 0.3; init_t = init_lo + u_t (init_hi - init_lo), each operation rounded once;
 *     warm_left = ceil(init_t / dt) clamped to [1, 2^31 - 1]; warm_fail = 0; budget = min(warm_left, interval);
 *     pending = 1: the caller writes the packet (qc_reset QC_RESET_GAUSSIAN, mask = pending, k_arr = k, mean 0,
 *     std 1) before its next qc_step. pending (out) is 0 for every other env; reset_out is 0 unless the env went
 *     live. rec_mode, when given, is written as for the other kinds.
 * qc_env_warmup_draw starts the warm-up of the envs with mask[e] != 0 (mask NULL: all) by the same draw and zeroes
 * their t, steps and return; it reads B, kind (QC_QO), interval, dt, pending, t, steps, episode_return and the
 * fields after rec_mode except init_energy_cutoff and reset_out.
 * perf != NULL (QC_HO and QC_QO; a cartpole kind, or perf_sum or perf_n NULL, is QC_EINVAL) adds the episode's
 * performance, the mean of quantity over the late part of the episode (the drivers' avg_phonon / avg_energy,
 * HO/main_parallel.py:247-248, 274-275, 294-295; QO/main_parallel.py:221, 231-232). A struct that leaves the four
 * fields zero behaves as before they existed.
 *   - episode start (QC_HO: pending on entry; QC_QO: the env goes live; qc_env_warmup_draw): perf_sum = 0, perf_n = 0.
 *   - a live control step that does not end the episode (QC_HO's pending first control step included) and whose new
 *     episode time t satisfies t > perf_from: perf_sum += quantity (rounded once), perf_n += 1. A step that ends the
 *     episode adds nothing: the reference breaks before it accumulates, and at t_max its loop ends first.
 *   - a finished episode: p = perf_sum / perf_n (rounded once) when t >= t_trunc and perf_n > 0, else cutoff (the
 *     reference's avg = accu / counter if t == t_max else cutoff; with perf_n == 0 it would divide by zero). p goes
 *     to perf[i % fin_cap], i the episode's position in fin; perf[fin_cap] is a sink the kernel never writes.
 *   - a warming QC_QO env touches neither accumulator. */
typedef struct qc_env_tail_args {
    int64_t B;
    int32_t kind;             /* enum qc_family: QC_IHO or QC_IQO (cartpoles), QC_HO or QC_QO (cooling) */
    int32_t n_obs, interval;  /* observables per env; physics steps per control interval */
    int32_t pad;
    double dt, xth, input_scaling, failing_reward;
    const int32_t* fail_step; /* [B] qc_step's fail_step */
    const int32_t* term_step; /* [B] qc_step's term_step (IQO) or NULL */
    const double* obs;        /* [B][n_obs] qc_step's obs_out */
    uint8_t* pending;         /* [B] in: reset interval in this call; out: resets in the next call */
    double* t;                /* [B] episode time */
    int64_t* steps;           /* [B] physics steps of the episode */
    double* episode_return;   /* [B] */
    float* obs32;             /* [B][n_obs] or NULL */
    float* reward;            /* [B] the reference's reward-row value */
    uint8_t* done;            /* [B] */
    uint8_t* valid;           /* [B] transitions the reference stores */
    double* fin;              /* [2][fin_cap + 1] finished (return, length) */
    int64_t fin_cap;
    int64_t* fin_n;           /* [1] episodes appended so far */
    const double* quantity;   /* [B] QC_HO: qc_phonon_number of the states after the step; cartpoles: unused */
    double cutoff;            /* QC_HO: the episode ends when quantity > cutoff */
    double t_trunc;           /* QC_HO: the episode is truncated when t >= t_trunc (t_max - 0.01 dt) */
    double reward_multiply;   /* QC_HO: reward = -quantity * reward_multiply */
    uint8_t* rec_mode;        /* [B] or NULL: qc_record's mode, 2 for an env pending on entry, else 1 */
    int32_t* warm_left;       /* [B] QC_QO: physics steps of free evolution still to run; warming iff > 0 */
    uint8_t* warm_fail;       /* [B] QC_QO: a Fail was seen during this warm-up */
    int64_t* draws;           /* [B] QC_QO: reset draws the env has consumed */
    double* k;                /* [B] QC_QO: the packet's wavenumber */
    int32_t* budget;          /* [B] QC_QO: in: the steps of this call (qc_step's env_steps); out: the next call's */
    double init_energy_cutoff;/* QC_QO: a warm-up is accepted when quantity < init_energy_cutoff and no Fail */
    double init_lo, init_hi;  /* QC_QO: the free evolution lasts U[init_lo, init_hi) time units */
    uint64_t seed;            /* QC_QO: Philox key of the draws */
    int64_t env_offset;       /* QC_QO: global id of env 0 (Philox counter word 2 = env_offset + e) */
    uint8_t* reset_out;       /* [B] QC_QO: 1 where the env went live in this call */
    double* perf_sum;         /* [B] QC_HO, QC_QO with perf: sum of quantity over the episode's counted control steps */
    int64_t* perf_n;          /* [B] QC_HO, QC_QO with perf: how many were counted */
    double* perf;             /* [fin_cap + 1] or NULL: the finished episodes' performance, entry i at i % fin_cap */
    double perf_from;         /* a control step is counted when its new episode time is > perf_from */
} qc_env_tail_args;
int qc_env_tail(qc_handle* h, const qc_env_tail_args* a);
int qc_env_warmup_draw(qc_handle* h, const qc_env_tail_args* a, const uint8_t* mask);

/* ---- training schedule: what the drivers decide from the stream of finished episodes ----------------------
 * The loader loop of each driver's RL.py (IHO:497-535, IQO:495-533, HO:491-538, QO:477-527) and one pass of
 * Main_System.__call__ with adjust_learning_rate, scale_up_actor_update_time and receive_net's save count
 * (IHO/main_parallel.py:369-405, 482-559), as one single-workgroup launch per control step that reads the
 * finished-episode ring qc_env_tail appends to. The host never reads the ring: each tick copies one snapshot into a
 * pinned slot of its own and records an event; qc_sched_poll waits on that event alone. A tick:
 *   1. rows = the number of set bytes in valid[0, B); total_rows += rows; pending += rows * 8 / 256 (rows are
 *      credited in the call that stores them; the reference credits them when their episode ends);
 *   2. the ring entries [read, *fin_n) in ring order, each through the rule's loader-loop body: episode += 1,
 *      t_done += t, the rule. If more than fin_cap entries are new the ring was overrun: the sticky error word is
 *      raised and the walk starts at the oldest entry still present;
 *   3. one Main_System pass: the updates due (at most max_updates_per_tick, the rest stays pending), the actor push,
 *      the learning rate and the target period, the save flag, the stop rule;
 *   4. with train == 0, count / sum / sum of squares of the episode times (mean, sem, n of the snapshot).
 * Every arithmetic operation is rounded once (no fused multiply-add), in the order csrc/qcart_sched.hpp writes
 * them, so a host restatement gives the same bits. */
enum { QC_SCHED_CARTPOLE = 0, QC_SCHED_COOLING = 1 };
#define QC_SCHED_MAX_LR_STEPS 8
#define QC_SCHED_MAX_RUNGS 4
typedef struct qc_sched_params {
    int32_t rule;                  /* QC_SCHED_*                                                          */
    int32_t train;                 /* 0: the --test / --LQG accounting: learning in progress is set at the   */
                                   /* first episode, the rule is not run; no updates, pushes or saves     */
    double start_time, fall_time;  /* cartpole: the EMA of the episode time starts learning at >= start_time */
                                   /* and clears it at < fall_time (IHO 20 / 5, IQO 12 / 4)               */
    double t_full;                 /* cooling: an episode counts as t == t_max iff t >= t_full (the env's    */
                                   /* t_trunc, t_max - 0.01 dt)                                           */
    double first_interval_time;    /* cooling: an episode stored no row iff t <= 1.5 first_interval_time     */
                                   /* (HO/RL.py:499 sets learning in progress on one); 0: no such rule    */
    int32_t fail_limit;            /* cooling: successive failures that clear learning (HO 10, QO 40)     */
    int32_t batch_size;
    double n_times_per_sample;     /* an update is due per D = (8 / n_times_per_sample) (batch_size / 256) pending */
    int64_t max_updates_per_tick;  /* >= 1                                                                */
    int64_t min_rows;              /* no update is due while total_rows < min_rows                        */
    int64_t num_episodes, give_up_episodes;
    double lr_init;
    double lr_cap;                 /* lr = min(lr_cap, lr) when learning is first in progress (4e-4; QO 1e-3) */
    int32_t n_lr_steps, n_rungs;
    int64_t lr_episode[QC_SCHED_MAX_LR_STEPS];   /* strictly increasing                                   */
    double lr_value[QC_SCHED_MAX_LR_STEPS];
    int32_t backup_period, warm_backup_period;   /* the emitted period is warm_backup_period (100) until   */
                                                 /* learning is first in progress                         */
    int64_t save_interval;
    double actor_update_time;      /* its initial value (10)                                              */
    /* scale_up_actor_update_time's rungs in the order it tests them: the first with last_achieved >           */
    /* rung_achieved[i] and actor_update_time <= rung_below[i] sets actor_update_time = rung_time[i]      */
    double rung_achieved[QC_SCHED_MAX_RUNGS], rung_below[QC_SCHED_MAX_RUNGS], rung_time[QC_SCHED_MAX_RUNGS];
} qc_sched_params;
typedef struct qc_sched_snapshot {
    int64_t tick;                  /* 0 for the first qc_sched_tick                                       */
    int64_t n_updates;
    int32_t push, save, stop, learning;
    double lr;
    int64_t backup_period;
    int64_t episode;
    double last_achieved, t_done, pending, actor_update_time;
    int64_t total_episodes, total_rows;
    int64_t error;                 /* sticky; bit 0: the ring was overrun                                 */
    double mean, sem;              /* train == 0: of the episode times so far (sem 0 below two)           */
    int64_t n;
} qc_sched_snapshot;
typedef struct qc_sched qc_sched;
int qc_sched_create(const qc_sched_params* p, int device, qc_sched** out);
void qc_sched_destroy(qc_sched* s);
const char* qc_sched_last_error(const qc_sched* s);
int qc_sched_set_stream(qc_sched* s, void* stream);
/* asynchronous: one launch, one copy of the snapshot into the tick's pinned slot, one event record. All pointers
 * are device pointers: fin [2][fin_cap + 1] and fin_n as qc_env_tail_args has them (the length row is read),
 * valid [B] (NULL with B == 0: no rows). The first tick has index 0. */
int qc_sched_tick(qc_sched* s, const double* fin, int64_t fin_cap, const int64_t* fin_n, const uint8_t* valid,
                  int64_t B);
/* asynchronous, one small launch: the walk starts at the ring's present end, *fin_n (a device pointer): entries
 * appended before are not this schedule's (an evaluation on an env that has already run) */
int qc_sched_seek(qc_sched* s, const int64_t* fin_n);
/* waits on the event of that tick only (never a device or stream synchronisation) and copies its snapshot out;
 * the last two ticks are kept, any other is QC_EINVAL */
int qc_sched_poll(qc_sched* s, int64_t tick, qc_sched_snapshot* out);
/* as the other kinds' (above): the header fields are the create-time params (the lr schedule and the rungs as
 * their lengths and a hash of their values), the payload the device state and the tick count */
int qc_sched_state_bytes(qc_sched* s, uint64_t* n);
int qc_sched_state_export(qc_sched* s, void* host_dst, uint64_t n);
int qc_sched_state_import(qc_sched* s, const void* host_src, uint64_t n);

/* ---- model ranking: the cooling drivers' receive_net on the device --------------------------------------------
 * worker_manager.receive_net (QO/main_parallel.py:283-329, HO/main_parallel.py:348-388) on the ring of the finished
 * episodes' performances (qc_env_tail_args.perf): the cooling drivers keep their num_of_saves best models, ranked by
 * the mean of the last `window` performances seen when a new net arrives. qc_monitor_receive is one launch of one
 * wave, one asynchronous copy of the snapshot into the call's pinned slot and one event record, as qc_sched_tick.
 * train == 1 (a net has arrived): fresh = *fin_n - read (negative: 0); count = fresh; episode_passed += fresh; read =
 * *fin_n. If episode_passed > min_episodes and count >= min_count: new_avg = the mean of the last k = min(count,
 * window) ring entries, oldest first, summed in numpy's order for these lengths (below 8 a running sum; from 8 on
 * ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)), with 16 values a[j] + a[8 + j] in place of a[j], then the
 * values past the last whole block of 8 one by one; each operation rounded once), divided by k. If new_avg <
 * good[num_of_saves - 1] the new entry takes rank = the number of the other num_of_saves - 1 entries <= new_avg (the
 * stable sort of good_actors.sort: ties go behind), the entries from rank on move down by one with their filled
 * flags, filled[rank] = 1 and episode_passed = 0. count = 0 after every receive (performances.clear()). Only the
 * last min(fresh, window) entries are read: window <= fin_cap is required, so they are always present and the work
 * per call is constant; an overrun ring is no error here.
 * train == 0 (--test): every fresh entry goes into n / sum / sum of squares in ring order; mean and sem as
 * qc_sched's. More than fin_cap fresh entries raise error bit 0 and the walk starts at the oldest entry present. */
#define QC_MONITOR_MAX_SAVES 64
#define QC_MONITOR_MAX_WINDOW 16
typedef struct qc_monitor_params {
    int32_t train;                 /* 1: the ranking; 0: the --test sums                                  */
    int32_t window;                /* performances averaged (QO 8, HO 10); 1 .. 16                        */
    int32_t min_count;             /* performances needed since the last receive (QO 8, HO 9); 1 .. window */
    int32_t num_of_saves;          /* 1 .. 64                                                             */
    int64_t min_episodes;          /* episodes since the last record must be > min_episodes (50)          */
    double initial;                /* the table's initial values (QO energy_cutoff / 2, HO phonon_cutoff)   */
} qc_monitor_params;
typedef struct qc_monitor_snapshot {
    int64_t call;                  /* 0 for the first qc_monitor_receive                                  */
    int64_t rank;                  /* the new record's position in the table, -1: none                    */
    double new_avg;                /* the window mean when the rule was evaluated, else 0                 */
    int64_t count;                 /* the fresh entries of this receive                                   */
    int64_t episode_passed;        /* after this receive                                                  */
    int64_t n_filled;              /* table entries that hold a model                                     */
    int64_t total_episodes;
    int64_t error;                 /* sticky; bit 0: the ring was overrun (train == 0)                    */
    double mean, sem;              /* train == 0: of the performances so far (sem 0 below two)            */
    int64_t n;
} qc_monitor_snapshot;
typedef struct qc_monitor qc_monitor;
int qc_monitor_create(const qc_monitor_params* p, int device, qc_monitor** out);
void qc_monitor_destroy(qc_monitor* m);
const char* qc_monitor_last_error(const qc_monitor* m);
int qc_monitor_set_stream(qc_monitor* m, void* stream);
/* asynchronous. perf [fin_cap + 1] and fin_n are device pointers as qc_env_tail_args has them */
int qc_monitor_receive(qc_monitor* m, const double* perf, int64_t fin_cap, const int64_t* fin_n);
/* asynchronous, one small launch: read = *fin_n, the ring's present end */
int qc_monitor_seek(qc_monitor* m, const int64_t* fin_n);
/* waits on the event of that receive only; the last two are kept, any other is QC_EINVAL */
int qc_monitor_poll(qc_monitor* m, int64_t call, qc_monitor_snapshot* out);
/* good [num_of_saves] and filled [num_of_saves] (host pointers, either may be NULL); synchronises the stream */
int qc_monitor_table(qc_monitor* m, double* good, int32_t* filled);
int qc_monitor_state_bytes(qc_monitor* m, uint64_t* n);
int qc_monitor_state_export(qc_monitor* m, void* host_dst, uint64_t n);
int qc_monitor_state_import(qc_monitor* m, const void* host_src, uint64_t n);

/* ---- position-space view: the drivers' spatial_repr and probability on the device ---------------------------------
 * HO/main_parallel.py:47-51, 82-86, 100-102 (IHO alike): the wavefunction of a Fock-basis state on a grid x,
 * phi[b][j] = sum_n E[j][n] c[b][n] with the table E[j][n] = psi_n(x[j]) of the normalised harmonic-oscillator
 * eigenfunctions (hbar = m = omega = 1), and its density p[b][j] = fl(fl(Re phi^2) + fl(Im phi^2)). The table is built
 * on the host at create time in long double by the upward three-term recurrence and rounded once to fp64
 * (csrc/qcart_spatial.hpp): n_levels in [1, 2048], x_n in [1, 4096], every x finite with |x| <= 128.
 * n_levels == 0 makes a grid view (QO / IQO, whose state already lives on x): no table, n_state must equal x_n,
 * probability is |psi_j|^2 by the same formula, repr is refused (the state is its own representation).
 * psi is [B][n_state] complex128 on the device, n_state <= n_levels: a shorter state uses the table's first columns.
 * threshold >= 0: a level takes part only if hypot(Re c, Im c) > threshold (the drivers' display mask is 1e-4); a
 * masked level contributes an exact zero; a grid view ignores it. phi[b] does not depend on B or on where env b sits.
 * qc_spatial_mean: m[j] = (sum over the envs b with mask[b] != 0 (mask NULL: all) of p[b][j]) / count, and count
 * itself; count == 0 gives zeros. The order of the sum is fixed by (B, X) alone: the envs form groups of 32 (group
 * g = envs 32 g .. 32 g + 31; envs past B and masked envs enter as +0); within a group s[q] (q = 0 .. 3) = the running
 * sum, from +0, of p of the group's envs q, q + 4, .., q + 28 in that order, and the group's partial is
 * (s[0] + s[1]) + (s[2] + s[3]); the same rule one level up: r[t] (t = 0 .. 3) = the running sum, from +0, of the
 * partials of the groups t, t + 4, t + 8, .. in that order, and m[j] = ((r[0] + r[1]) + (r[2] + r[3])) /
 * (double)count. Every operation is rounded once; no atomics. The partials live in a buffer the handle owns (it grows
 * with B). All calls are asynchronous on the bound stream. */
typedef struct qc_spatial qc_spatial;
int qc_spatial_create(int32_t n_levels, const double* x /* host [x_n] */, int32_t x_n, int device, qc_spatial** out);
void qc_spatial_destroy(qc_spatial* s);
const char* qc_spatial_last_error(const qc_spatial* s);
int qc_spatial_set_stream(qc_spatial* s, void* stream);
/* out: device [x_n][n_levels], a copy of the table; a grid view has none (QC_EINVAL) */
int qc_spatial_table(const qc_spatial* s, double* out);
/* out: device [B][x_n] complex128 */
int qc_spatial_repr(qc_spatial* s, const void* psi, int32_t B, int32_t n_state, double threshold, void* out);
/* out: device [B][x_n] */
int qc_spatial_probability(qc_spatial* s, const void* psi, int32_t B, int32_t n_state, double threshold, double* out);
/* mask: device uint8 [B] or NULL; out: device [x_n]; count: device, may be NULL */
int qc_spatial_mean(qc_spatial* s, const void* psi, int32_t B, int32_t n_state, const uint8_t* mask, double threshold,
                    double* out, int64_t* count);
/* The change of basis of density matrices, Fock -> position: sigma_m = scale * E rho_m E^T,
 *   sigma[i][j] = scale * sum_{m, n < n_state} E[i][m] rho[m][n] E[j][n],
 * rho [M][n_state][n_state] complex128 and sigma [M][x_n][x_n] complex128 on the device (they must not overlap), E the
 * handle's table, which is real. With scale = h, the spacing of a uniform x, sigma has qc_ensemble's grid normalisation
 * (Tr sigma = 1 for Tr rho = 1 when the grid holds the states) and Re sigma[i][i] / h is the position density. The
 * input is ASSUMED Hermitian and is not checked: all of rho is read as it stands, and the output is the exactly
 * Hermitian matrix whose lower triangle is that of the product: sigma[i][j] for j <= i and sigma[j][i] are written from
 * the same values (the sign bit of the imaginary part flipped), the diagonal's imaginary part is +0.0. Two kernels on
 * v_mfma_f64_16x16x4_f64 in the manner of qc_lindblad_congruence, Zt = (E rho)^T (all of it), then the elements of
 * Zt^T E^T on or below the diagonal. The order of every sum is a function of n_state alone: the contraction index k
 * runs in ascending groups of four from accumulators that start at +0, one matrix instruction per group and
 * accumulator (rows and k past the matrix enter as exact zeros selected by address; what memory holds there is never
 * multiplied):
 *   Zt[r][c]:  re += Re rho[k][r] * E[c][k];  im += Im rho[k][r] * E[c][k];
 *   acc[i][j]: re += Re Zt[k][i] * E[j][k];   im += Im Zt[k][i] * E[j][k];
 * then sigma[i][j] = (fl(scale * re), fl(scale * im)). Element (m, i, j) does not depend on M, on where rho_m sits in
 * the batch or on the other matrices of the call (a launch of fewer than 2048 blocks of 32 x 32 elements runs one
 * 16 x 16 tile per workgroup instead of 2 x 2: the same instructions in the same order). No atomics. Zt lives in a
 * buffer of the handle that grows with M (the only allocation the call may make). Refused with a text, before anything
 * is launched: a grid view, n_state outside [1, n_levels], M < 1, null pointers, a scale that is not finite,
 * M x_n^2 > 2^27. */
int qc_spatial_congruence(qc_spatial* s, const void* rho, int32_t n_state, int32_t M, double scale, void* sigma);

/* ---- phase-space view: the Wigner function of a batch of wavefunctions on the device --------------------------------
 * For a wavefunction phi sampled on a uniform grid (phi_i = phi(x_0 + i h), sum_i h |phi_i|^2 = 1) and momenta p[P]:
 *   K_i = min(i, x_n - 1 - i),  c_ik = conj(phi_{i+k}) phi_{i-k},
 *   W[i][j] = (h / pi) ( |phi_i|^2 + 2 sum_{k = 1 .. K_i} ( Re c_ik cos(2 p_j k h) - Im c_ik sin(2 p_j k h) ) ),
 * which is (1 / pi) int conj(phi(x + y)) phi(x - y) e^{2 i p y} dy with hbar = 1, y = k h and phi = 0 off the grid: a
 * packet e^{+i p0 x} sits at p = +p0. x_n in [1, 4096], h finite and > 0, P in [1, 1024], every p finite with
 * |p_j| h <= pi (one period of the grid's momentum); anything else is refused with a text. The table
 * (cos, sin)(2 p_j h k), k = 1 .. (x_n - 1) / 2, is built on the host at create time in long double and rounded once
 * to fp64 (csrc/qcart_wigner.hpp): each entry within 2^-53 + 2^-62 |a| of the cos / sin of the exact a = 2 p_j h k.
 * phi is [B][x_n] complex128 on the device (for Fock states: qc_spatial_repr's output on the same grid).
 * qc_wigner_eval writes W [B][x_n][P] (64-bit offsets); W[b] does not depend on B or on where env b sits. An element
 * is fl(s * acc), s = fl(2 h / pi), acc the fp64 matrix pipe's sum over the lags in ascending steps of four, lag 0
 * entering with the weight 1/2.
 * qc_wigner_mean: m[i][j] = (sum over the envs b with mask[b] != 0 (mask NULL: all) of W[b][i][j]) / count, and count
 * itself; count == 0 gives zeros. No per-env W is written: the env index is one more index of the contraction. The
 * order of the sum is fixed by (B, x_n, P) alone: the envs form chunks of E = qc_wigner_chunk(x_n) consecutive envs
 * (2 for x_n <= 512, else 1; envs past B and masked envs enter as zero operands); there are
 * S = qc_wigner_splits(B, x_n, P) = min(ceil(B / E), 256, max(1, 2^23 / (x_n P))) splits, split s owns the chunks s,
 * s + S, s + 2 S, ..; its accumulator runs, from +0, over its chunks in that order, within a chunk over the lags in
 * ascending steps of four, within a step over the chunk's envs in ascending order; then t = the running sum, from +0,
 * of the splits' accumulators 0, 1, .., S - 1 and m = fl(fl(s * t) / (double)count). No atomics. The splits'
 * accumulators live in a buffer the handle owns, made at create time for the largest S (at most 64 MiB): no call
 * allocates or waits. All calls are asynchronous on the bound stream. */
typedef struct qc_wigner qc_wigner;
int qc_wigner_create(int32_t x_n, double h, const double* p /* host [P] */, int32_t P, int device, qc_wigner** out);
void qc_wigner_destroy(qc_wigner* w);
const char* qc_wigner_last_error(const qc_wigner* w);
int qc_wigner_set_stream(qc_wigner* w, void* stream);
/* phi: device [B][x_n] complex128; out: device [B][x_n][P] */
int qc_wigner_eval(qc_wigner* w, const void* phi, int32_t B, double* out);
/* mask: device uint8 [B] or NULL; out: device [x_n][P]; count: device, may be NULL */
int qc_wigner_mean(qc_wigner* w, const void* phi, int32_t B, const uint8_t* mask, double* out, int64_t* count);
/* the mean's order (above): envs per chunk, and the number of splits (0 for arguments out of range) */
int qc_wigner_chunk(int32_t x_n);
int qc_wigner_splits(int32_t B, int32_t x_n, int32_t P);
/* The Wigner function of density matrices on the grid. rho [M][x_n][x_n] complex128 on the device, normalised as
 * qc_ensemble normalises a grid family's (sum_i rho[i][i] = 1: a pure state is rho = h phi phi^†). With
 * L_ik = rho[i + k][i - k], an element of the LOWER triangle,
 *   W[i][j] = (1 / pi) ( Re rho[i][i] + 2 sum_{k = 1 .. K_i} ( Re L_ik cos(2 p_j k h) + Im L_ik sin(2 p_j k h) ) ),
 * which is the W above with conj(phi_{i+k}) phi_{i-k} = rho[i-k][i+k] / h read through Hermiticity. The input is
 * ASSUMED Hermitian and is not checked: only the elements with row >= col and an even row - col are read, and the
 * imaginary part of the diagonal is ignored (what the rest of memory holds, NaN included, does not matter). out is
 * W [M][x_n][P] (64-bit offsets). An element is fl(s * acc), s = fl(2 / pi), acc the fp64 matrix pipe's sum, from +0,
 * over the lags in ascending steps of four, per step first (Re L, cos) and then (Im L, sin), lag 0 entering as
 * (Re rho[i][i], 1/2) and (+0, 0); lags past K_i enter as exact zeros selected by address. Element (m, i, j) depends
 * on rho_m alone: not on M, nor on where matrix m sits. It uses the handle's table and allocates nothing. M < 1, null
 * pointers and M x_n^2 > 2^27 are refused with a text before anything is launched. Asynchronous. */
int qc_wigner_eval_rho(qc_wigner* w, const void* rho, int32_t M, double* out);

/* ---- ensemble view: the density matrix of a batch of states on the device -------------------------------------------
 * For states psi [B][N] complex128 (contiguous, on the device), N in [1, 2048]:
 *   t[m][n]   = sum over the envs b with mask[b] != 0 (mask NULL: all) of psi_b[m] * conj(psi_b[n]),
 *   rho[m][n] = fl( fl(scale * t[m][n]) / count ),   count = the number of set mask bytes (no mask: B),
 * the unconditional state of the ensemble. scale is a positive finite double fixed at create time: 1 for Fock states,
 * the grid spacing h for the grid families' continuum-normalised states (sum h |psi|^2 = 1). The states are not
 * renormalised: Tr rho is the mean of scale * ||psi_b||^2 over the live envs, which is 1 for normalised states. count
 * is written as one int64 on the device; with count == 0 every element is zero and nothing is divided. A masked env,
 * and the env past B that pads an odd B's last chunk, is a row of exact zeros as an operand: zeros are selected for
 * it, its memory (which may hold NaN or Inf) is never multiplied. N outside [1, 2048], a scale that is not finite and
 * > 0, B < 1 and null pointers are refused with a text, the create arguments before the device is touched.
 * The output is the full [N][N] complex128 matrix (row-major, rho[m][n] at m N + n) and is exactly Hermitian: only
 * elements with n <= m are accumulated (64 x 32 blocks of 16 x 16 fp64 matrix-pipe tiles on or below the diagonal);
 * the second stage writes rho[m][n] = (re, im) and rho[n][m] = (re, -im) from the same values (the sign bit flipped:
 * -0.0 where im is +0.0), and +0.0 as the imaginary part of the diagonal, where the accumulation b a + (-a) b leaves
 * a rounding residue.
 * The order of the sum is fixed by (B, N) alone, never by the mask's content: the envs form chunks of
 * E = qc_ensemble_chunk(N) = 2 consecutive envs (the K = 4 of one v_mfma_f64_16x16x4_f64 is 2 envs x (re, im));
 * there are S = qc_ensemble_splits(B, N) = min(ceil(B / E), 256, max(1, floor(2^22 / N^2))) splits, split s owns the
 * chunks s, s + S, s + 2 S, ..; its accumulators run, from +0, over its chunks in that order, one matrix instruction
 * per chunk and tile; then t = the running sum, from +0, of the splits' accumulators 0, 1, .., S - 1, separately for
 * the real and the imaginary part, and rho as above. No atomics. The splits' accumulators live in a buffer the handle
 * owns, made at create time for the largest S ([S][2][N][N] doubles, at most 64 MiB): no call allocates or waits.
 * All calls are asynchronous on the bound stream. */
typedef struct qc_ensemble qc_ensemble;
int qc_ensemble_create(int32_t N, double scale, int device, qc_ensemble** out);
void qc_ensemble_destroy(qc_ensemble* h);
const char* qc_ensemble_last_error(const qc_ensemble* h);
int qc_ensemble_set_stream(qc_ensemble* h, void* stream);
/* psi: device [B][N] complex128; mask: device uint8 [B] or NULL; rho: device [N][N] complex128; count: device, may be
 * NULL */
int qc_ensemble_density(qc_ensemble* h, const void* psi, int32_t B, const uint8_t* mask, void* rho, int64_t* count);
/* the order (above): envs per chunk, and the number of splits (0 for arguments out of range) */
int qc_ensemble_chunk(int32_t N);
int qc_ensemble_splits(int32_t B, int32_t N);

/* ---- energy-level view: eigenstates of the force-free Hamiltonian, level populations of a batch of states ----------
 * qc_levels_solve (host only; never touches a device): the lowest K eigenpairs of the real symmetric band H that the
 * library builds for p's family and physics (HO: the diagonal omega (n + 1/2); QO: the 9-point kinetic stencil plus
 * lambda x^4 on the grid). K in [1, min(N, 256)], N = the state length (qc_dim). energies[K] ascending; vectors[K][N],
 * row k = level k with unit l2 norm, the last entry j with |V[k][j]| > 2^-26 max_j |V[k][j]| positive (the outermost
 * lobe on the +x side, the convention of qc_spatial's table). Computed in long double (bisection on the band's
 * inertia, inverse iteration, Rayleigh-quotient refinement; csrc/qcart_levels.hpp) and rounded once to fp64; the same
 * bits on every call. HO: energies[k] is the band's diagonal entry bit for bit, vectors the identity exactly. IHO and
 * IQO are refused ("no bound levels: H is not bounded below": their truncated matrices have edge-localised, pairwise
 * near-degenerate lowest vectors; pass a table of your own to qc_levels_create instead). A level that does not
 * converge, or two of the K levels closer than 2^-20 ||H||_inf, give QC_ESINGULAR, never garbage.
 * qc_levels_create takes any real table V [K][N] (host; neither orthogonality nor norm is checked) and a scale:
 * N in [1, 2048], K in [1, min(N, 256)], scale finite and > 0, every entry finite; anything else, B < 1 and null
 * pointers are refused with a text, the create arguments before the device is touched. For the grid families'
 * continuum-normalised states (sum h |psi|^2 = 1) and unit-norm rows, scale = sqrt(h) makes sum_k p[b][k] the in-band
 * part of sum_j h |psi_b[j]|^2. psi is [B][N] complex128 (contiguous, on the device).
 *   a[b][k] = ( fl(scale * s_re), fl(scale * s_im) ),  s_re = the fp64 matrix pipe's sum of V[k][j] * Re psi_b[j] over
 *             j in ascending groups of four, from +0, one v_mfma_f64_16x16x4_f64 per group (the device table is padded
 *             with zeros to whole groups), s_im the same over Im. a[b] does not depend on B or on where env b sits.
 *   p[b][k] = fl( fl(re * re) + fl(im * im) ) of exactly that a[b][k].
 *   m[k]    = (sum over the envs b with mask[b] != 0 (mask NULL: all) of p[b][k]) / count, and count itself;
 *             count == 0 gives zeros and nothing is divided. No per-env p is written.
 * The order of the mean's sum is fixed by (B, K, N) alone, never by the mask's content: the envs form groups of 64
 * (group g = envs 64 g .. 64 g + 63), each of four sub-groups of 16 consecutive envs. A masked env, and an env past B,
 * enters as a row of exact zero operands (zeros are selected for it by address; its memory, which may hold NaN or Inf,
 * is never multiplied), so its p is +0. Within a sub-group s[q] (q = 0 .. 3) = the running sum, from +0, of p of the
 * sub-group's envs q, q + 4, q + 8, q + 12 in that order, and the sub-group's sum is (s[0] + s[1]) + (s[2] + s[3]);
 * the group's partial is (u[0] + u[1]) + (u[2] + u[3]) of its four sub-groups' sums; then the same rule once more:
 * r[t] (t = 0 .. 3) = the running sum, from +0, of the partials of the groups t, t + 4, t + 8, .. in that order, and
 * m[k] = ((r[0] + r[1]) + (r[2] + r[3])) / (double)count. Every operation is rounded once; no atomics. The partials
 * live in a buffer the handle owns (it grows with B). All calls are asynchronous on the bound stream. */
typedef struct qc_levels qc_levels;
/* host only: energies host [K], vectors host [K][N] */
int qc_levels_solve(const qc_params* p, int32_t K, double* energies, double* vectors);
int qc_levels_create(int32_t N, int32_t K, double scale, const double* vectors /* host [K][N] */, int device,
                     qc_levels** out);
void qc_levels_destroy(qc_levels* h);
/* h NULL: the text of the last failed qc_levels_solve / qc_levels_create */
const char* qc_levels_last_error(const qc_levels* h);
int qc_levels_set_stream(qc_levels* h, void* stream);
/* psi: device [B][N] complex128; out: device [B][K] complex128 */
int qc_levels_amplitudes(qc_levels* h, const void* psi, int32_t B, void* out);
/* out: device [B][K] */
int qc_levels_populations(qc_levels* h, const void* psi, int32_t B, double* out);
/* mask: device uint8 [B] or NULL; out: device [K]; count: device, may be NULL */
int qc_levels_mean(qc_levels* h, const void* psi, int32_t B, const uint8_t* mask, double* out, int64_t* count);

/* ---- master equation: the open-loop evolution of density matrices --------------------------------------------------
 * The average of the library's stochastic Schroedinger equation over the record, for a force F that does not depend
 * on it, is closed:
 *   d rho / dt = -i [H_F, rho] - (gamma / 4) [X, [X, rho]],   H_F = H - c F X
 * (H, X, c as qc_create builds them for p's family and physics). The scheme works in the eigenbasis of the truncated
 * position operator, X = W diag(xi) W^T (Fock families: W real orthogonal, xi ascending; grid families: W = I, xi the
 * grid points), where the measurement term is elementwise. One step of length dt is the Strang composition
 *   sigma <- G½ o sigma,  sigma <- T sigma T^†,  sigma <- G½ o sigma      (o: the elementwise product)
 *   T = W^T C W,  C = (I + i dt/2 H_F)^-1 (I - i dt/2 H_F)   (the Cayley propagator of the step kernels' own matrix),
 *   G½_ij = exp(-gamma dt (xi_i - xi_j)^2 / 8),  G_ij = exp(-gamma dt (xi_i - xi_j)^2 / 4),
 * with the inner half-steps of consecutive steps merged:
 *   evolve(rho, n):  sigma = W^T rho W (Fock only);  sigma <- G½ o sigma;
 *                    n times: sigma <- g o (T sigma T^†), g = G, and G½ in the last repetition;
 *                    rho = W sigma W^T (Fock only).
 * C is unitary and G, G½ are positive-semidefinite kernels with a unit diagonal, so every step is an exact quantum
 * channel: trace, Hermiticity and positivity hold up to rounding. Second order in dt; the reference's dt^3 .. dt^6
 * drift corrections are deliberately absent (they would break the unitarity).
 * qc_lindblad_tables (host only; never touches a device) gives the tables of one force, each computed in long double
 * and rounded once to fp64 (csrc/qcart_lindblad.hpp): xi and W by qc_levels_solve's band solver on the tridiagonal X
 * with K = N (the sign of column k by its convention; therefore Fock N <= 256), C by a partially pivoted complex band
 * LU, T from the fp64 W, G and G½ by expl from the long double xi (the Rayleigh quotients of W's columns, whose rounding
 * the returned xi is; G is not the square of the rounded G½; both symmetric with a unit diagonal exactly). Any output may be NULL. The same bits on every call. Fock N > 256, a grid outside
 * [9, 2048] points, fp32 physics (precision == 1), a dt that is not finite and > 0, a gamma that is not finite and
 * >= 0 and a force that is not finite are refused with a text.
 * qc_lindblad_create builds the tables of J forces (slot s = forces[s]; J in [1, 32], J N^2 <= 2^25); its arguments
 * are refused before the device is touched.
 * The building block is the batched Hermitian congruence
 *   Y_m = g o (A_s(m) X_m A_s(m)^†),  m < M,  X_m [N][N] complex128, A_s complex [N][N], g real symmetric or none,
 * in two kernels on v_mfma_f64_16x16x4_f64: Z = A X (all of it), then Y = g o (Z A^†) for the elements on or below
 * the diagonal only. The input is ASSUMED Hermitian and is not checked: the left product reads all of X as it
 * stands, and the output is the exactly Hermitian matrix whose lower triangle is that of g o (A X A^†): Y[i][j] for
 * j <= i and Y[j][i] = conj(Y[i][j]) are written from the same values (the sign bit of the imaginary part flipped),
 * the diagonal's imaginary part is +0.0. y may equal x. M N^2 <= 2^27; Z lives in a buffer of the handle that grows
 * with M (the only allocation any call makes).
 * The order of every sum is a function of N alone. With a = A[i][k], x = X[k][j], the contraction index k runs in
 * ascending groups of four from accumulators that start at +0, one matrix instruction per group and chain (rows,
 * columns and k past N enter as exact zeros selected by address: what memory holds there, NaN or Inf included, is
 * never multiplied), and per group the two accumulators of an element take their chains in this order:
 *   Z:  re += x_re a_re;  re += (-x_im) a_im;  im += x_re a_im;  im += x_im a_re;
 *   Y (z = Z[i][k], a = A[j][k]):  re += z_re a_re;  re += z_im a_im;  im += z_im a_re;  im += (-z_re) a_im;
 * then Y = (fl(g_ij re), fl(g_ij im)), or (re, im) without g. Element (m, i, j) does not depend on M, on where X_m
 * sits in the batch, or on which other matrices are in the call (a launch of fewer than 2048 blocks of 32 x 32 elements
 * runs one 16 x 16 tile per workgroup instead of 2 x 2: that changes which workgroup computes an element, never its
 * instructions or their order). No atomics; everything is asynchronous on the bound stream and nothing waits on the
 * host.
 * qc_lindblad_evolve works in place on rho [M][N][N] in the states' basis with qc_ensemble's normalisation
 * (Tr rho = 1): 2 n_steps matrix launches and one elementwise launch, for Fock also the two basis changes (two
 * congruences with the real W widened to a complex operand at create time). slots (device int32 [M]) picks the force
 * of each rho; NULL: default_slot for all. A slot outside [0, J) leaves that rho untouched and raises the handle's
 * device error flag: qc_lindblad_take_errors (synchronises, as qc_take_errors) reports it once. n_steps = 0 launches
 * nothing and returns QC_OK. M < 1, n_steps < 0 and null pointers are refused with a text. */
typedef struct qc_lindblad qc_lindblad;
/* host only: xi host [N], W host [N][N] (grid: the identity), T host [N][N] complex128, g_half and g_full host [N][N] */
int qc_lindblad_tables(const qc_params* p, double dt, double gamma, double force, double* xi, double* W, void* T,
                       double* g_half, double* g_full);
int qc_lindblad_create(const qc_params* p, double dt, double gamma, const double* forces /* host [J] */, int32_t J,
                       int device, qc_lindblad** out);
void qc_lindblad_destroy(qc_lindblad* h);
/* h NULL: the text of the last failed qc_lindblad_tables / qc_lindblad_create */
const char* qc_lindblad_last_error(const qc_lindblad* h);
int qc_lindblad_set_stream(qc_lindblad* h, void* stream);
int qc_lindblad_dim(const qc_lindblad* h);
/* rho: device [M][N][N] complex128, in place; slots: device int32 [M] or NULL */
int qc_lindblad_evolve(qc_lindblad* h, void* rho, int32_t M, const int32_t* slots, int32_t default_slot,
                       int32_t n_steps);
/* A: device [N][N] complex128; g: device [N][N] or NULL; x, y: device [M][N][N] complex128, y may equal x */
int qc_lindblad_congruence(qc_lindblad* h, const void* A, const double* g, const void* x, void* y, int32_t M);
int qc_lindblad_take_errors(qc_lindblad* h);

/* ---- conditional master equation: rho along a measurement record seen with detection efficiency eta ---------------
 *   d rho = -i [H_F, rho] dt - (gamma / 4) [X, [X, rho]] dt + sqrt(eta gamma / 2) {X - <X>, rho} dW
 * between the step kernels' pure states (eta = 1) and qc_lindblad_evolve (eta = 0). It works in qc_lindblad_evolve's
 * basis (sigma = W^T rho W for Fock, taken there and back once per call; the grid itself otherwise) on its tables. With
 * a = eta gamma dt / 2 and s = 1 / sqrt(4 a) (each formed in long double and rounded once), step n of matrix m is
 *   1. sigma <- G^(1-eta) o (T_s sigma T_s^†): the congruence above, unchanged, with the table
 *      G^(1-eta)_ij = exp(-gamma (1 - eta) dt (xi_i - xi_j)^2 / 4) (expl from the long double xi, gamma (1 - eta) in
 *      long double) as g; no g at eta = 1.
 *   2. the outcome (not in filtering mode): d_i = Re sigma_ii where that is not below 0, else 0 (a NaN stays); c_i its
 *      inclusive prefix sums; I = min { i : c_i > u c_(N-1) } (N - 1 where no c_i is: u = 1 after rounding);
 *      y = fma(z, s, xi_I). That samples p(y) = sum_i sigma_ii sqrt(2 a / pi) exp(-2 a (xi_i - y)^2) exactly; y is in
 *      the units of the step kernels' measurement outcome q: E y = Tr(sigma X), noise variance 1 / (2 eta gamma dt).
 *   3. e_i = (xi_i - y)^2, e0 = min_i e_i, w_i = exp(-(a (e_i - e0))), Z = sum_i (w_i w_i) d_i, v_i = w_i / sqrt(Z),
 *      sigma_ij <- (v_i v_j) sigma_ij with the product v_i v_j formed first (a Hermitian-by-bit-pattern sigma with a
 *      +0.0 diagonal imaginary part stays so). Tr sigma = 1 after every step up to rounding; nothing accumulates.
 * The average over y of 2-3 is G^eta o sigma, so the mean over records of n steps is (G o T . T^†)^n sigma_0 exactly:
 * every step is an exact quantum instrument. At eta = 1 a pure sigma stays pure. The input is ASSUMED Hermitian, as
 * qc_lindblad_congruence assumes it.
 * The order of the sums c and Z (one routine, a function of N alone): indices in chunks of 256 ascending; inside a
 * chunk the doubling t_i <- t_i + t_(i-s) for s = 1, 2, 4 .. 128, every i >= s of the chunk at once, elements past N
 * entering as +0; c_i = carry + t_i with carry the c of the previous chunk's last element (+0 for the first); Z is the
 * last element of the sums of (w_i w_i) d_i. min is exact. Two launches per step after the congruence's two
 * (k_filter_draw: one workgroup per matrix; k_filter_apply: one element per thread); one device copy of rho into a
 * buffer of the handle before the first step and one launch after the last (below). No atomics, nothing waits on the
 * host.
 * Random numbers: Philox4x32-10 keyed by seed at counter (step_lo, step_hi, stream id, tag), step = first_step + n,
 * stream id = streams[m] (device int32 [M]; NULL: m): u = ((w0 << 32 | w1) >> 11 + 0.5) 2^-53 of the block at tag
 * 0x500, z = the step kernels' normal r0 of the block at tag 0x501. Nothing is stored between calls: a matrix's
 * trajectory depends on (seed, stream id, step) alone, not on M or its place in the batch, and n steps in one call give
 * the record of two calls of n / 2 with first_step bit for bit, and for the grid families the same rho bit for bit (a
 * Fock rho goes to sigma and back once per call: two calls round the two basis changes once more and agree with one
 * call within rounding). draws (device [n_steps][M][2]: u, z) overrides Philox. Filtering
 * mode: record_in (device [n_steps][M]) supplies y and nothing is drawn; record_in together with draws is refused.
 * record_out (device [n_steps][M] or NULL) receives y.
 * qc_lindblad_filter_draws (host only) gives the (u, z) the device draws at (seed, stream id, step): u exactly, z
 * within rounding (< 1e-15) of the device's.
 * A matrix that cannot be stepped (c_(N-1), y or Z not finite, c_(N-1) or Z not > 0; in filtering mode Z = 0 means
 * the record contradicts the state) is left as the call found it, bit for bit (the launch after the last step writes
 * the copy back), its record entries from that step on are NaN, and it raises a second bit of the handle's error
 * flag, which qc_lindblad_take_errors reports once with its own text. A slot outside [0, J) is handled as
 * qc_lindblad_evolve handles it.
 * qc_lindblad_set_efficiency(h, eta), eta in (0, 1] and the handle's gamma > 0 (refused with a text otherwise),
 * builds G^(1-eta) on the host, waits for the handle's stream and uploads it (it may synchronise).
 * qc_lindblad_efficiency gives eta, -1 while unset. qc_lindblad_evolve_conditional's limits are
 * qc_lindblad_evolve's; first_step >= 0; n_steps = 0 launches nothing; a call before qc_lindblad_set_efficiency is
 * refused before the device is touched; every pointer except rho may be NULL. */
int qc_lindblad_set_efficiency(qc_lindblad* h, double eta);
/* *eta: the efficiency, -1 while unset */
int qc_lindblad_efficiency(const qc_lindblad* h, double* eta);
/* rho: device [M][N][N] complex128, in place; slots, streams: device int32 [M] or NULL; draws: device
 * [n_steps][M][2] or NULL; record_in, record_out: device [n_steps][M] or NULL */
int qc_lindblad_evolve_conditional(qc_lindblad* h, void* rho, int32_t M, const int32_t* slots, int32_t default_slot,
                                   int32_t n_steps, uint64_t seed, const int32_t* streams, int64_t first_step,
                                   const double* draws, const double* record_in, double* record_out);
/* xi: device [N]: a copy of the handle's own eigenvalues of X, asynchronous on the bound stream */
int qc_lindblad_xi(qc_lindblad* h, double* xi);
/* host only: the table qc_lindblad_set_efficiency uploads (the unit matrix at eta = 1, where it is not read), g host
 * [N][N]; refusals as qc_lindblad_tables' and qc_lindblad_set_efficiency's, with a text (qc_lindblad_last_error(NULL)) */
int qc_lindblad_efficiency_table(const qc_params* p, double dt, double gamma, double eta, double* g);
/* host only */
int qc_lindblad_filter_draws(uint64_t seed, uint32_t stream, uint64_t step, double* u, double* z);

/* ---- step server: the reference's process model on one GPU ------------------------------------------------
 * The drivers run 30-40 actor processes, each with its own `simulation` module stepping ONE env per call
 * (IHO/main_parallel.py:345-359, :264). A step server owns one handle of batch max_clients (env e = client slot
 * e, MT19937 noise per env) and a POSIX shared-memory object `name` ("/..."); actor processes attach with
 * libqcart_client.so (include/qcart_client.h, no HIP) and post step / simulate_10_steps / set_seed /
 * x_expectation / get_moments requests. Each tick steps every pending env in one batched launch (per-env step
 * budgets keep the others frozen); the tick waits up to batch_wait_us (<= 0: 40 us) after its first request for
 * the other owned slots' requests. Results equal the plain drop-in's (the same kernels, the same per-env
 * MT19937 stream). Fock modules: while qc_server_run serves, a resident kernel (one wave per slot) answers the
 * clients' step(state, dt, force, gamma) calls on the action grid directly from the shared object, without a
 * launch or a tick (qcart_shm.h); the ticks carry the other calls. */
typedef struct qc_server qc_server;
int qc_server_create(const qc_params* p, int device, int32_t max_clients, const char* name, double batch_wait_us,
                     qc_server** out);
/* serve on the calling thread until qc_server_stop (another thread) or `seconds` (> 0) have passed */
int qc_server_run(qc_server* s, double seconds);
int qc_server_stop(qc_server* s);
int qc_server_stats(const qc_server* s, int64_t* ticks, int64_t* calls);
/* out[4]: microseconds summed over the ticks — batching wait, host launches, GPU (until the stream sync
 * returned), publishing the results */
int qc_server_timing(const qc_server* s, double* out);
/* 1 when the server serves one-step calls on its resident kernel (fp64 modules at the drivers' sizes;
 * QCART_SERVER_RESIDENT=0 turns it off), else 0; *calls: the requests the resident path has answered since the object
 * was created; *launches: resident kernel launches (each lives one lease, QCART_RESIDENT_LEASE_MS, default 20 ms) */
int qc_server_resident(const qc_server* s, int64_t* calls, int64_t* launches);
const char* qc_server_last_error(const qc_server* s);
/* marks the object dead (waiting clients fail with QCC_ENOSERVER) and unlinks it */
void qc_server_destroy(qc_server* s);

#ifdef __cplusplus
}
#endif
#endif
