"""ctypes binding of libqcart.so (include/qcart.h).

The library is the only compute path: if it is missing or no HIP device is present, every call
raises. There is deliberately no CPU fallback in this package.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# QCART_LIB selects an alternative in-tree build (A/B experiments); default: the package's libqcart.so
LIB_PATH = os.environ.get("QCART_LIB") or os.path.join(_HERE, "libqcart.so")

QC_HO, QC_IHO, QC_QO, QC_IQO = 0, 1, 2, 3
QC_A_REFERENCE, QC_A_EXACT = 0, 1
QC_RESET_GROUND, QC_RESET_RANDOM, QC_RESET_GAUSSIAN = 0, 1, 2
QC_CTL_LQG, QC_CTL_DAMPING, QC_CTL_SEMICLASSICAL = 0, 1, 2
QC_NOISE_PHILOX, QC_NOISE_MT19937 = 0, 1
CONTROL_STRATEGIES = {"LQG": QC_CTL_LQG, "damping": QC_CTL_DAMPING, "semiclassical": QC_CTL_SEMICLASSICAL}

STATUS = {
    0: "QC_OK", -1: "QC_EINVAL", -2: "QC_ENOMEM", -3: "QC_EHIP", -4: "QC_EPIVOT", -5: "QC_ESINGULAR",
    -6: "QC_ENOTBUILT",
}

# every symbol include/qcart.h declares (checked by tests/test_abi.py)
EXPORTS = (
    "qc_create", "qc_destroy", "qc_last_error", "qc_abi_version", "qc_get_params", "qc_dim", "qc_n_obs",
    "qc_set_stream", "qc_sync", "qc_set_seed", "qc_set_step_counter", "qc_get_step_counter",
    "qc_env_counters", "qc_set_seed_mt19937", "qc_noise_mode", "qc_mt19937_state", "qc_mt19937_words",
    "qc_set_dynamics", "qc_add_force", "qc_step", "qc_moments", "qc_x_expectation", "qc_outside_prob",
    "qc_boundary_fail", "qc_energy", "qc_hamiltonian_dot_psi", "qc_phonon_number", "qc_reset", "qc_control", "qc_record_row_len", "qc_record",
    "qc_scan_levels", "qc_take_errors", "qc_step_group_size", "qc_group_layout", "qc_wavefunction_len", "qc_wavefunction_obs", "qc_set_timing", "qc_step_kernel_time",
    "qc_actor_create", "qc_actor_destroy", "qc_actor_last_error", "qc_actor_set_stream", "qc_actor_load",
    "qc_actor_noise_len", "qc_actor_act",
    "qc_mactor_create", "qc_mactor_destroy", "qc_mactor_last_error", "qc_mactor_set_stream", "qc_mactor_noise_len",
    "qc_mactor_flat_len", "qc_mactor_load", "qc_mactor_act",
    "qc_replay_create", "qc_replay_destroy", "qc_replay_last_error", "qc_replay_set_stream", "qc_replay_store",
    "qc_replay_store_xp", "qc_replay_sample", "qc_replay_update", "qc_replay_rebuild", "qc_replay_stats",
    "qc_replay_buffers", "qc_set_seed_mt19937_envs", "qc_mt19937_normals",
    "qc_server_create", "qc_server_run", "qc_server_stop", "qc_server_stats", "qc_server_timing", "qc_server_resident",
    "qc_server_last_error",
    "qc_server_destroy", "qc_env_tail", "qc_env_warmup_draw",
    "qc_learner_create", "qc_learner_destroy", "qc_learner_last_error", "qc_learner_set_stream",
    "qc_learner_noise_len", "qc_learner_load", "qc_learner_layers", "qc_learner_update", "qc_learner_set_lr",
    "qc_learner_stats", "qc_learner_grads", "qc_learner_apply",
    "qc_mlearner_create", "qc_mlearner_destroy", "qc_mlearner_last_error", "qc_mlearner_set_stream",
    "qc_mlearner_noise_len", "qc_mlearner_load", "qc_mlearner_layers", "qc_mlearner_update", "qc_mlearner_set_lr",
    "qc_mlearner_stats", "qc_mlearner_grads", "qc_mlearner_apply", "qc_mlearner_states",
    "qc_learner_set_backup_period", "qc_mlearner_set_backup_period",
    "qc_sched_create", "qc_sched_destroy", "qc_sched_last_error", "qc_sched_set_stream", "qc_sched_tick",
    "qc_sched_poll", "qc_sched_seek",
    "qc_monitor_create", "qc_monitor_destroy", "qc_monitor_last_error", "qc_monitor_set_stream", "qc_monitor_receive",
    "qc_monitor_poll", "qc_monitor_seek", "qc_monitor_table",
    "qc_spatial_create", "qc_spatial_destroy", "qc_spatial_last_error", "qc_spatial_set_stream", "qc_spatial_table",
    "qc_spatial_repr", "qc_spatial_probability", "qc_spatial_mean", "qc_spatial_congruence",
    "qc_wigner_create", "qc_wigner_destroy", "qc_wigner_last_error", "qc_wigner_set_stream", "qc_wigner_eval",
    "qc_wigner_mean", "qc_wigner_chunk", "qc_wigner_splits", "qc_wigner_eval_rho",
    "qc_ensemble_create", "qc_ensemble_destroy", "qc_ensemble_last_error", "qc_ensemble_set_stream",
    "qc_ensemble_density", "qc_ensemble_chunk", "qc_ensemble_splits",
    "qc_levels_solve", "qc_levels_create", "qc_levels_destroy", "qc_levels_last_error", "qc_levels_set_stream",
    "qc_levels_amplitudes", "qc_levels_populations", "qc_levels_mean",
    "qc_lindblad_tables", "qc_lindblad_create", "qc_lindblad_destroy", "qc_lindblad_last_error",
    "qc_lindblad_set_stream", "qc_lindblad_dim", "qc_lindblad_evolve", "qc_lindblad_congruence",
    "qc_lindblad_take_errors", "qc_lindblad_set_efficiency", "qc_lindblad_efficiency",
    "qc_lindblad_evolve_conditional", "qc_lindblad_filter_draws", "qc_lindblad_efficiency_table", "qc_lindblad_xi",
) + tuple(f"qc_{kind}_state_{op}" for kind in ("actor", "mactor", "replay", "learner", "mlearner", "sched", "monitor")
          for op in ("bytes", "export", "import"))   # checkpoint: a handle's whole state as one host buffer


class QcParams(ctypes.Structure):
    _fields_ = [
        ("family", ctypes.c_int32),
        ("n_max", ctypes.c_int32),
        ("omega", ctypes.c_double),
        ("x_max", ctypes.c_double),
        ("grid_size", ctypes.c_double),
        ("lambda_", ctypes.c_double),
        ("mass", ctypes.c_double),
        ("moment_order", ctypes.c_int32),
        ("a_mode", ctypes.c_int32),
        ("gamma", ctypes.c_double),
        ("dt", ctypes.c_double),
        ("f_max", ctypes.c_double),
        ("n_actions", ctypes.c_int32),
        ("precision", ctypes.c_int32),   # 0 fp64, 1 fp32 (Fock families; complex64 states)
        ("batch", ctypes.c_int64),
        ("env_offset", ctypes.c_int64),
        ("seed", ctypes.c_uint64),
        ("xth", ctypes.c_double),
    ]


class QcEnvTailArgs(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int64),
        ("kind", ctypes.c_int32),
        ("n_obs", ctypes.c_int32),
        ("interval", ctypes.c_int32),
        ("pad", ctypes.c_int32),
        ("dt", ctypes.c_double),
        ("xth", ctypes.c_double),
        ("input_scaling", ctypes.c_double),
        ("failing_reward", ctypes.c_double),
        ("fail_step", ctypes.c_void_p),
        ("term_step", ctypes.c_void_p),
        ("obs", ctypes.c_void_p),
        ("pending", ctypes.c_void_p),
        ("t", ctypes.c_void_p),
        ("steps", ctypes.c_void_p),
        ("episode_return", ctypes.c_void_p),
        ("obs32", ctypes.c_void_p),
        ("reward", ctypes.c_void_p),
        ("done", ctypes.c_void_p),
        ("valid", ctypes.c_void_p),
        ("fin", ctypes.c_void_p),
        ("fin_cap", ctypes.c_int64),
        ("fin_n", ctypes.c_void_p),
        # the cooling accounting (kind == QC_HO) and qc_record's per-env mode; zero / NULL for the cartpoles
        ("quantity", ctypes.c_void_p),
        ("cutoff", ctypes.c_double),
        ("t_trunc", ctypes.c_double),
        ("reward_multiply", ctypes.c_double),
        ("rec_mode", ctypes.c_void_p),
        # the rolling warm-up of the quartic cooling driver (kind == QC_QO); zero / NULL otherwise
        ("warm_left", ctypes.c_void_p),
        ("warm_fail", ctypes.c_void_p),
        ("draws", ctypes.c_void_p),
        ("k", ctypes.c_void_p),
        ("budget", ctypes.c_void_p),
        ("init_energy_cutoff", ctypes.c_double),
        ("init_lo", ctypes.c_double),
        ("init_hi", ctypes.c_double),
        ("seed", ctypes.c_uint64),
        ("env_offset", ctypes.c_int64),
        ("reset_out", ctypes.c_void_p),
        # the cooling kinds' per-episode performance; zero / NULL: none
        ("perf_sum", ctypes.c_void_p),
        ("perf_n", ctypes.c_void_p),
        ("perf", ctypes.c_void_p),
        ("perf_from", ctypes.c_double),
    ]


class QcDqnParams(ctypes.Structure):
    _fields_ = [
        ("data_length", ctypes.c_int32),
        ("n_actions", ctypes.c_int32),
        ("max_batch", ctypes.c_int64),
        ("seed", ctypes.c_uint64),
        ("hidden2", ctypes.c_int32),
    ]


class QcMdqnParams(ctypes.Structure):
    _fields_ = [
        ("read_length", ctypes.c_int32),
        ("n_actions", ctypes.c_int32),
        ("max_batch", ctypes.c_int64),
        ("seed", ctypes.c_uint64),
        ("chunk", ctypes.c_int32),
    ]


class QcDqnLayer(ctypes.Structure):
    _fields_ = [
        ("weight", ctypes.c_void_p),
        ("bias", ctypes.c_void_p),
        ("weight_norm", ctypes.c_void_p),
        ("sigma_w", ctypes.c_void_p),
        ("sigma_b", ctypes.c_void_p),
    ]


class QcLearnerParams(ctypes.Structure):
    _fields_ = [
        ("data_length", ctypes.c_int32),
        ("n_actions", ctypes.c_int32),
        ("batch_size", ctypes.c_int32),
        ("backup_period", ctypes.c_int32),
        ("gamma", ctypes.c_double),
        ("lr", ctypes.c_double),
        ("alive_reward", ctypes.c_double),
        ("failing_reward", ctypes.c_double),
        ("seed", ctypes.c_uint64),
        ("hidden2", ctypes.c_int32),
        ("target_mode", ctypes.c_int32),
        ("beta1", ctypes.c_double),
        ("beta2", ctypes.c_double),
    ]


class QcMlearnerParams(ctypes.Structure):
    _fields_ = [
        ("read_length", ctypes.c_int32),
        ("read_step_length", ctypes.c_int32),
        ("n_actions", ctypes.c_int32),
        ("batch_size", ctypes.c_int32),
        ("backup_period", ctypes.c_int32),
        ("target_mode", ctypes.c_int32),
        ("gamma", ctypes.c_double),
        ("lr", ctypes.c_double),
        ("alive_reward", ctypes.c_double),
        ("failing_reward", ctypes.c_double),
        ("beta1", ctypes.c_double),
        ("beta2", ctypes.c_double),
        ("seed", ctypes.c_uint64),
        ("conv_weight_norm", ctypes.c_int32),
    ]


TD_TARGETS = {"alive": 0, "reward_fail": 1, "reward": 2}   # QC_TD_ALIVE, QC_TD_REWARD_FAIL, QC_TD_REWARD


class QcLearnerStats(ctypes.Structure):
    _fields_ = [
        ("updates", ctypes.c_int64),
        ("step", ctypes.c_int64),
        ("nonfinite", ctypes.c_int64),
        ("l1", ctypes.c_double),
        ("l2", ctypes.c_double),
        ("lr", ctypes.c_double),
        ("backup_counter", ctypes.c_int32),
        ("launches_per_update", ctypes.c_int32),
    ]


QC_SCHED_CARTPOLE, QC_SCHED_COOLING = 0, 1
QC_SCHED_MAX_LR_STEPS, QC_SCHED_MAX_RUNGS = 8, 4
QC_SCHED_ERR_OVERRUN = 1


class QcSchedParams(ctypes.Structure):
    _fields_ = [
        ("rule", ctypes.c_int32),
        ("train", ctypes.c_int32),
        ("start_time", ctypes.c_double),
        ("fall_time", ctypes.c_double),
        ("t_full", ctypes.c_double),
        ("first_interval_time", ctypes.c_double),
        ("fail_limit", ctypes.c_int32),
        ("batch_size", ctypes.c_int32),
        ("n_times_per_sample", ctypes.c_double),
        ("max_updates_per_tick", ctypes.c_int64),
        ("min_rows", ctypes.c_int64),
        ("num_episodes", ctypes.c_int64),
        ("give_up_episodes", ctypes.c_int64),
        ("lr_init", ctypes.c_double),
        ("lr_cap", ctypes.c_double),
        ("n_lr_steps", ctypes.c_int32),
        ("n_rungs", ctypes.c_int32),
        ("lr_episode", ctypes.c_int64 * QC_SCHED_MAX_LR_STEPS),
        ("lr_value", ctypes.c_double * QC_SCHED_MAX_LR_STEPS),
        ("backup_period", ctypes.c_int32),
        ("warm_backup_period", ctypes.c_int32),
        ("save_interval", ctypes.c_int64),
        ("actor_update_time", ctypes.c_double),
        ("rung_achieved", ctypes.c_double * QC_SCHED_MAX_RUNGS),
        ("rung_below", ctypes.c_double * QC_SCHED_MAX_RUNGS),
        ("rung_time", ctypes.c_double * QC_SCHED_MAX_RUNGS),
    ]


class QcSchedSnapshot(ctypes.Structure):
    _fields_ = [
        ("tick", ctypes.c_int64),
        ("n_updates", ctypes.c_int64),
        ("push", ctypes.c_int32),
        ("save", ctypes.c_int32),
        ("stop", ctypes.c_int32),
        ("learning", ctypes.c_int32),
        ("lr", ctypes.c_double),
        ("backup_period", ctypes.c_int64),
        ("episode", ctypes.c_int64),
        ("last_achieved", ctypes.c_double),
        ("t_done", ctypes.c_double),
        ("pending", ctypes.c_double),
        ("actor_update_time", ctypes.c_double),
        ("total_episodes", ctypes.c_int64),
        ("total_rows", ctypes.c_int64),
        ("error", ctypes.c_int64),
        ("mean", ctypes.c_double),
        ("sem", ctypes.c_double),
        ("n", ctypes.c_int64),
    ]


QC_MONITOR_MAX_SAVES, QC_MONITOR_MAX_WINDOW = 64, 16
QC_MONITOR_ERR_OVERRUN = 1


class QcMonitorParams(ctypes.Structure):
    _fields_ = [
        ("train", ctypes.c_int32),
        ("window", ctypes.c_int32),
        ("min_count", ctypes.c_int32),
        ("num_of_saves", ctypes.c_int32),
        ("min_episodes", ctypes.c_int64),
        ("initial", ctypes.c_double),
    ]


class QcMonitorSnapshot(ctypes.Structure):
    _fields_ = [
        ("call", ctypes.c_int64),
        ("rank", ctypes.c_int64),
        ("new_avg", ctypes.c_double),
        ("count", ctypes.c_int64),
        ("episode_passed", ctypes.c_int64),
        ("n_filled", ctypes.c_int64),
        ("total_episodes", ctypes.c_int64),
        ("error", ctypes.c_int64),
        ("mean", ctypes.c_double),
        ("sem", ctypes.c_double),
        ("n", ctypes.c_int64),
    ]


class QcReplayParams(ctypes.Structure):
    _fields_ = [
        ("capacity", ctypes.c_int64),
        ("row_len", ctypes.c_int32),
        ("policy", ctypes.c_int32),
        ("passes_before_random", ctypes.c_double),
        ("alpha", ctypes.c_double),
        ("beta", ctypes.c_double),
        ("beta_increment", ctypes.c_double),
        ("abs_err_upper", ctypes.c_double),
        ("epsilon_scale", ctypes.c_double),
        ("seed", ctypes.c_uint64),
    ]


class QcReplayStats(ctypes.Structure):
    _fields_ = [
        ("len", ctypes.c_int64),
        ("data_pointer", ctypes.c_int64),
        ("passes", ctypes.c_double),
        ("max", ctypes.c_double),
        ("beta", ctypes.c_double),
        ("total_p", ctypes.c_double),
        ("n_nodes", ctypes.c_int64),
        ("tree_size", ctypes.c_int64),
    ]


class QCartError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code


_lib = None


def _preload_torch_hip():
    # Reuse torch's HIP runtime (same SONAME libamdhip64.so.7) so that torch tensors and libqcart
    # share one runtime, one context and one stream namespace.
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not built: run `make` (or __graft_entry__.build()); this package has no CPU fallback")
    _preload_torch_hip()
    L = _Tolerant(ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)) if os.environ.get("QCART_LIB") else \
        ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    P, vp = ctypes.POINTER, ctypes.c_void_p
    i32, i64, u64, d = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
    L.qc_create.argtypes = [P(QcParams), ctypes.c_int, P(vp)]
    L.qc_destroy.argtypes = [vp]
    L.qc_destroy.restype = None
    L.qc_last_error.argtypes = [vp]
    L.qc_last_error.restype = ctypes.c_char_p
    L.qc_abi_version.argtypes = []
    L.qc_get_params.argtypes = [vp, P(QcParams)]
    L.qc_dim.argtypes = [vp]
    L.qc_n_obs.argtypes = [vp]
    L.qc_set_stream.argtypes = [vp, vp]
    L.qc_sync.argtypes = [vp]
    L.qc_set_seed.argtypes = [vp, u64]
    L.qc_set_step_counter.argtypes = [vp, u64]
    L.qc_get_step_counter.argtypes = [vp]
    L.qc_get_step_counter.restype = u64
    L.qc_env_counters.argtypes = [vp, vp, vp]
    L.qc_set_seed_mt19937.argtypes = [vp, vp]
    L.qc_set_seed_mt19937_envs.argtypes = [vp, vp, vp]
    L.qc_mt19937_normals.argtypes = [vp, ctypes.c_int32, vp, vp, vp, vp]
    L.qc_env_tail.argtypes = [vp, P(QcEnvTailArgs)]
    L.qc_env_warmup_draw.argtypes = [vp, P(QcEnvTailArgs), vp]
    L.qc_server_create.argtypes = [P(QcParams), ctypes.c_int, i32, ctypes.c_char_p, d, P(vp)]
    L.qc_server_run.argtypes = [vp, d]
    L.qc_server_stop.argtypes = [vp]
    L.qc_server_stats.argtypes = [vp, P(i64), P(i64)]
    L.qc_server_timing.argtypes = [vp, vp]
    L.qc_server_resident.argtypes = [vp, P(i64), P(i64)]
    L.qc_server_last_error.argtypes = [vp]
    L.qc_server_last_error.restype = ctypes.c_char_p
    L.qc_server_destroy.argtypes = [vp]
    L.qc_server_destroy.restype = None
    L.qc_noise_mode.argtypes = [vp]
    L.qc_mt19937_state.argtypes = [vp, vp, vp]
    L.qc_mt19937_words.argtypes = []
    L.qc_set_dynamics.argtypes = [vp, d, d]
    L.qc_add_force.argtypes = [vp, d]
    L.qc_step.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.qc_moments.argtypes = [vp, vp, vp]
    L.qc_x_expectation.argtypes = [vp, vp, vp]
    L.qc_outside_prob.argtypes = [vp, vp, d, vp]
    L.qc_boundary_fail.argtypes = [vp, vp, vp]
    L.qc_energy.argtypes = [vp, vp, vp]
    L.qc_hamiltonian_dot_psi.argtypes = [vp, vp]
    L.qc_phonon_number.argtypes = [vp, vp, vp]
    L.qc_reset.argtypes = [vp, vp, i32, vp, d, d, d, vp, vp, vp]
    L.qc_control.argtypes = [vp, vp, i32, d, d, d, vp, vp]
    L.qc_record_row_len.argtypes = [i32, i32, i32]
    L.qc_record.argtypes = [vp, i32, i32, d, vp, i32, vp, i32, vp, vp, vp, vp, vp]
    L.qc_set_timing.argtypes = [vp, i32]
    L.qc_step_kernel_time.argtypes = [vp, P(d), P(i64)]
    L.qc_wavefunction_len.argtypes = [vp]
    L.qc_wavefunction_obs.argtypes = [vp, vp, d, vp]
    L.qc_scan_levels.argtypes = [vp, i32, P(i32), P(i32)]
    L.qc_step_group_size.argtypes = [vp]
    L.qc_group_layout.argtypes = [vp, vp, i64, vp, i64]
    for name in ("qc_take_errors",):   # (older in-tree builds in A/B runs lack them)
        if hasattr(L, name):
            getattr(L, name).argtypes = [vp]
    L.qc_actor_create.argtypes = [P(QcDqnParams), ctypes.c_int, P(vp)]
    L.qc_actor_destroy.argtypes = [vp]
    L.qc_actor_destroy.restype = None
    L.qc_actor_last_error.argtypes = [vp]
    L.qc_actor_last_error.restype = ctypes.c_char_p
    L.qc_actor_set_stream.argtypes = [vp, vp]
    L.qc_actor_load.argtypes = [vp, P(QcDqnLayer)]
    L.qc_actor_noise_len.argtypes = [vp]
    L.qc_actor_act.argtypes = [vp, i64, i64, vp, i32, vp, d, u64, vp, vp, vp]
    L.qc_mactor_create.argtypes = [P(QcMdqnParams), ctypes.c_int, P(vp)]
    L.qc_mactor_destroy.argtypes = [vp]
    L.qc_mactor_destroy.restype = None
    L.qc_mactor_last_error.argtypes = [vp]
    L.qc_mactor_last_error.restype = ctypes.c_char_p
    L.qc_mactor_set_stream.argtypes = [vp, vp]
    L.qc_mactor_noise_len.argtypes = [vp]
    L.qc_mactor_flat_len.argtypes = [vp]
    L.qc_mactor_load.argtypes = [vp, P(QcDqnLayer)]
    L.qc_mactor_act.argtypes = [vp, i64, i64, vp, i32, vp, d, u64, vp, vp, vp]
    L.qc_replay_create.argtypes = [P(QcReplayParams), ctypes.c_int, P(vp)]
    L.qc_replay_destroy.argtypes = [vp]
    L.qc_replay_destroy.restype = None
    L.qc_replay_last_error.argtypes = [vp]
    L.qc_replay_last_error.restype = ctypes.c_char_p
    L.qc_replay_set_stream.argtypes = [vp, vp]
    L.qc_replay_store.argtypes = [vp, i64, vp, vp]
    L.qc_replay_store_xp.argtypes = [vp, i64, vp, vp, vp, i32, vp, vp]
    L.qc_replay_sample.argtypes = [vp, i32, vp, vp, vp, vp]
    L.qc_replay_update.argtypes = [vp, i32, vp, vp]
    L.qc_replay_rebuild.argtypes = [vp]
    L.qc_replay_stats.argtypes = [vp, P(QcReplayStats)]
    L.qc_replay_buffers.argtypes = [vp, P(vp), P(vp)]
    L.qc_learner_create.argtypes = [P(QcLearnerParams), ctypes.c_int, P(vp)]
    L.qc_learner_destroy.argtypes = [vp]
    L.qc_learner_destroy.restype = None
    L.qc_learner_last_error.argtypes = [vp]
    L.qc_learner_last_error.restype = ctypes.c_char_p
    L.qc_learner_set_stream.argtypes = [vp, vp]
    L.qc_learner_noise_len.argtypes = [vp]
    L.qc_learner_load.argtypes = [vp, P(QcDqnLayer)]
    L.qc_learner_layers.argtypes = [vp, ctypes.c_int, P(QcDqnLayer)]
    L.qc_learner_update.argtypes = [vp, vp, vp, vp, u64, vp, vp]
    L.qc_learner_set_lr.argtypes = [vp, d]
    L.qc_learner_stats.argtypes = [vp, P(QcLearnerStats)]
    L.qc_learner_grads.argtypes = [vp, P(QcDqnLayer)]
    L.qc_learner_apply.argtypes = [vp, P(QcDqnLayer)]
    L.qc_mlearner_create.argtypes = [P(QcMlearnerParams), ctypes.c_int, P(vp)]
    L.qc_mlearner_destroy.argtypes = [vp]
    L.qc_mlearner_destroy.restype = None
    L.qc_mlearner_last_error.argtypes = [vp]
    L.qc_mlearner_last_error.restype = ctypes.c_char_p
    L.qc_mlearner_set_stream.argtypes = [vp, vp]
    L.qc_mlearner_noise_len.argtypes = [vp]
    L.qc_mlearner_load.argtypes = [vp, P(QcDqnLayer)]
    L.qc_mlearner_layers.argtypes = [vp, ctypes.c_int, P(QcDqnLayer)]
    L.qc_mlearner_update.argtypes = [vp, vp, vp, vp, u64, vp, vp]
    L.qc_mlearner_set_lr.argtypes = [vp, d]
    L.qc_learner_set_backup_period.argtypes = [vp, i32]
    L.qc_mlearner_set_backup_period.argtypes = [vp, i32]
    L.qc_sched_create.argtypes = [P(QcSchedParams), ctypes.c_int, P(vp)]
    L.qc_sched_destroy.argtypes = [vp]
    L.qc_sched_destroy.restype = None
    L.qc_sched_last_error.argtypes = [vp]
    L.qc_sched_last_error.restype = ctypes.c_char_p
    L.qc_sched_set_stream.argtypes = [vp, vp]
    L.qc_sched_tick.argtypes = [vp, vp, i64, vp, vp, i64]
    L.qc_sched_poll.argtypes = [vp, i64, P(QcSchedSnapshot)]
    L.qc_sched_seek.argtypes = [vp, vp]
    L.qc_monitor_create.argtypes = [P(QcMonitorParams), ctypes.c_int, P(vp)]
    L.qc_monitor_destroy.argtypes = [vp]
    L.qc_monitor_destroy.restype = None
    L.qc_monitor_last_error.argtypes = [vp]
    L.qc_monitor_last_error.restype = ctypes.c_char_p
    L.qc_monitor_set_stream.argtypes = [vp, vp]
    L.qc_monitor_receive.argtypes = [vp, vp, i64, vp]
    L.qc_monitor_poll.argtypes = [vp, i64, P(QcMonitorSnapshot)]
    L.qc_monitor_seek.argtypes = [vp, vp]
    L.qc_monitor_table.argtypes = [vp, vp, vp]
    L.qc_spatial_create.argtypes = [i32, vp, i32, ctypes.c_int, P(vp)]
    L.qc_spatial_destroy.argtypes = [vp]
    L.qc_spatial_destroy.restype = None
    L.qc_spatial_last_error.argtypes = [vp]
    L.qc_spatial_last_error.restype = ctypes.c_char_p
    L.qc_spatial_set_stream.argtypes = [vp, vp]
    L.qc_spatial_table.argtypes = [vp, vp]
    L.qc_spatial_repr.argtypes = [vp, vp, i32, i32, d, vp]
    L.qc_spatial_probability.argtypes = [vp, vp, i32, i32, d, vp]
    L.qc_spatial_mean.argtypes = [vp, vp, i32, i32, vp, d, vp, vp]
    L.qc_spatial_congruence.argtypes = [vp, vp, i32, i32, d, vp]
    L.qc_wigner_create.argtypes = [i32, d, vp, i32, ctypes.c_int, P(vp)]
    L.qc_wigner_destroy.argtypes = [vp]
    L.qc_wigner_destroy.restype = None
    L.qc_wigner_last_error.argtypes = [vp]
    L.qc_wigner_last_error.restype = ctypes.c_char_p
    L.qc_wigner_set_stream.argtypes = [vp, vp]
    L.qc_wigner_eval.argtypes = [vp, vp, i32, vp]
    L.qc_wigner_mean.argtypes = [vp, vp, i32, vp, vp, vp]
    L.qc_wigner_eval_rho.argtypes = [vp, vp, i32, vp]
    L.qc_wigner_chunk.argtypes = [i32]
    L.qc_wigner_splits.argtypes = [i32, i32, i32]
    L.qc_ensemble_create.argtypes = [i32, d, ctypes.c_int, P(vp)]
    L.qc_ensemble_destroy.argtypes = [vp]
    L.qc_ensemble_destroy.restype = None
    L.qc_ensemble_last_error.argtypes = [vp]
    L.qc_ensemble_last_error.restype = ctypes.c_char_p
    L.qc_ensemble_set_stream.argtypes = [vp, vp]
    L.qc_ensemble_density.argtypes = [vp, vp, i32, vp, vp, vp]
    L.qc_ensemble_chunk.argtypes = [i32]
    L.qc_ensemble_splits.argtypes = [i32, i32]
    L.qc_levels_solve.argtypes = [P(QcParams), i32, vp, vp]
    L.qc_levels_create.argtypes = [i32, i32, d, vp, ctypes.c_int, P(vp)]
    L.qc_levels_destroy.argtypes = [vp]
    L.qc_levels_destroy.restype = None
    L.qc_levels_last_error.argtypes = [vp]
    L.qc_levels_last_error.restype = ctypes.c_char_p
    L.qc_levels_set_stream.argtypes = [vp, vp]
    L.qc_levels_amplitudes.argtypes = [vp, vp, i32, vp]
    L.qc_levels_populations.argtypes = [vp, vp, i32, vp]
    L.qc_levels_mean.argtypes = [vp, vp, i32, vp, vp, vp]
    L.qc_lindblad_tables.argtypes = [P(QcParams), d, d, d, vp, vp, vp, vp, vp]
    L.qc_lindblad_create.argtypes = [P(QcParams), d, d, vp, i32, ctypes.c_int, P(vp)]
    L.qc_lindblad_destroy.argtypes = [vp]
    L.qc_lindblad_destroy.restype = None
    L.qc_lindblad_last_error.argtypes = [vp]
    L.qc_lindblad_last_error.restype = ctypes.c_char_p
    L.qc_lindblad_set_stream.argtypes = [vp, vp]
    L.qc_lindblad_dim.argtypes = [vp]
    L.qc_lindblad_evolve.argtypes = [vp, vp, i32, vp, i32, i32]
    L.qc_lindblad_congruence.argtypes = [vp, vp, vp, vp, vp, i32]
    L.qc_lindblad_take_errors.argtypes = [vp]
    L.qc_lindblad_set_efficiency.argtypes = [vp, d]
    L.qc_lindblad_efficiency.argtypes = [vp, P(d)]
    L.qc_lindblad_evolve_conditional.argtypes = [vp, vp, i32, vp, i32, i32, u64, vp, i64, vp, vp, vp]
    L.qc_lindblad_filter_draws.argtypes = [u64, ctypes.c_uint32, u64, P(d), P(d)]
    L.qc_lindblad_xi.argtypes = [vp, vp]
    L.qc_lindblad_efficiency_table.argtypes = [P(QcParams), d, d, d, vp]
    L.qc_mlearner_stats.argtypes = [vp, P(QcLearnerStats)]
    L.qc_mlearner_grads.argtypes = [vp, P(QcDqnLayer)]
    L.qc_mlearner_apply.argtypes = [vp, P(QcDqnLayer)]
    L.qc_mlearner_states.argtypes = [vp, vp, vp, vp]
    for kind in ("actor", "mactor", "replay", "learner", "mlearner", "sched", "monitor"):
        getattr(L, f"qc_{kind}_state_bytes").argtypes = [vp, P(u64)]
        getattr(L, f"qc_{kind}_state_export").argtypes = [vp, vp, u64]
        getattr(L, f"qc_{kind}_state_import").argtypes = [vp, vp, u64]
    if isinstance(L, _Tolerant):
        L = L.lib
    for name in EXPORTS:
        # every declared entry point must resolve in the shipped library (a stale build fails here); an
        # explicit QCART_LIB (A/B runs against older builds) may lack the newest ones
        if os.environ.get("QCART_LIB") and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        if fn.restype is ctypes.c_int:   # default
            fn.restype = ctypes.c_int
    _lib = L
    return L


class _Tolerant:
    """An older in-tree build named by QCART_LIB (A/B runs): signatures of entry points it lacks are skipped."""

    class _Sink:
        argtypes = restype = None

    def __init__(self, lib):
        object.__setattr__(self, "lib", lib)

    def __getattr__(self, name):
        return getattr(self.lib, name) if hasattr(self.lib, name) else _Tolerant._Sink()


def _checker(prefix: str):
    """check(rc, handle=None) for the handle family `prefix`: a negative status raises QCartError with
    <prefix>_last_error(handle) (handle None: the text of a failed <prefix>_create)."""
    def check(rc: int, handle=None) -> int:
        if rc < 0:
            msg = getattr(lib(), prefix + "_last_error")(handle)
            raise QCartError(rc, msg.decode() if msg else "")
        return rc
    return check


check = _checker("qc")
check_actor = _checker("qc_actor")
check_mactor = _checker("qc_mactor")
check_learner = _checker("qc_learner")
check_mlearner = _checker("qc_mlearner")
check_replay = _checker("qc_replay")
check_sched = _checker("qc_sched")
check_monitor = _checker("qc_monitor")
check_spatial = _checker("qc_spatial")
check_wigner = _checker("qc_wigner")
check_ensemble = _checker("qc_ensemble")
check_levels = _checker("qc_levels")
check_lindblad = _checker("qc_lindblad")


class DeviceHandle:
    """Owner of one libqcart handle `self._h` on `self.device`, for the handle family `_prefix`
    (<prefix>_destroy / _set_stream / _last_error)."""

    _prefix = "qc"
    _h = None

    def _check(self, rc: int) -> int:
        return _checker(self._prefix)(rc, self._h)

    def close(self):
        if self._h:
            getattr(lib(), self._prefix + "_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _export_state(self):
        """The handle's whole state (qc_<kind>_state_export) as a uint8 CPU tensor; synchronises its stream."""
        import torch
        self._bind_stream()
        n = ctypes.c_uint64()
        self._check(getattr(lib(), self._prefix + "_state_bytes")(self._h, ctypes.byref(n)))
        blob = torch.empty(n.value, dtype=torch.uint8)
        self._check(getattr(lib(), self._prefix + "_state_export")(self._h, ctypes.c_void_p(blob.data_ptr()), n.value))
        return blob

    def _import_state(self, blob):
        """qc_<kind>_state_import of a tensor `_export_state` made; a refusal raises QCartError (QC_EINVAL) naming the
        field that differs and leaves the handle as it was."""
        import torch
        if not isinstance(blob, torch.Tensor) or blob.dtype != torch.uint8 or blob.dim() != 1:
            raise ValueError("the state blob must be a 1-d uint8 tensor")
        blob = blob.cpu().contiguous()
        self._bind_stream()
        self._check(getattr(lib(), self._prefix + "_state_import")(self._h, ctypes.c_void_p(blob.data_ptr()),
                                                                  blob.numel()))

    def _bind_stream(self):
        """Later launches of this handle go to torch's current stream of its device."""
        import torch
        s = torch.cuda.current_stream(self.device).cuda_stream
        self._check(getattr(lib(), self._prefix + "_set_stream")(self._h, ctypes.c_void_p(s)))


def check_echo(who: str, state, mine: dict, payload=()):
    """The refusal rule of every load_state_dict: `state` must carry each of `mine`'s fields with the same value
    (the first that differs is named) and the payload keys."""
    if not isinstance(state, dict):
        raise ValueError(f"{who}: a state is a dict, not {type(state).__name__}")
    for k, v in mine.items():
        if k not in state:
            raise ValueError(f"{who}: the state has no field {k!r} (made by another class?)")
        got = tuple(state[k]) if isinstance(state[k], list) else state[k]
        if got != v:
            raise ValueError(f"{who}: {k} differs: the state was made for {state[k]!r}, this object for {v!r}")
    for k in payload:
        if k not in state:
            raise ValueError(f"{who}: the state has no {k!r}")


def fill_layer(slot: "QcDqnLayer", tensors) -> None:
    """Write a layer's (weight, bias, weight_norm, sigma_w, sigma_b) device tensors (None where the layer has
    none) into a QcDqnLayer; the caller keeps the tensors alive."""
    for (name, _), t in zip(QcDqnLayer._fields_, tensors):
        setattr(slot, name, t.data_ptr() if t is not None else None)
