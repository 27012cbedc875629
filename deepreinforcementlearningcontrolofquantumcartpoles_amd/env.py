"""BatchedEnv: the reference actors' episode loop (Control.do_episode) for B environments at once,
on device tensors, one control interval per step().

Reference semantics reproduced per family ('xp' observation input):
  * cartpoles (IHO, IQO): IHO/main_parallel.py:227-268, IQO/main_parallel.py:172-222
      - reset: IHO |0>, IQO Gaussian_packet(inf, 0, 1); force 0 for the first control interval
        (no control at the zero-th step), first decision at i = control_interval
      - done when the boundary Fail flag fired during the interval (numerical_failure) or, at the
        control step, |<x>| > xth = F_max (IHO) / the outside probability exceeded 0.5 at any
        physics step (IQO, checked every step); reward row value 1 (alive) or failing_reward (-1)
  * cooling (HO, QO): HO/main_parallel.py:222-292, QO/main_parallel.py:169-232
      - reset: HO |0>; QO Gaussian(k ~ U[-0.3,0.3]) evolved U[15,20] time units at F = 0, redrawn
        until energy < 7.5 and no Fail (QO/main_parallel.py:177-198)
      - first decision at i = control_interval after a zero-force interval (HO:238, like the
        cartpoles) / at i = 0 (QO:208); at each control step the transition is stored with reward
        -phonon*scale (HO) / -energy*scale (QO) while phonon <= cutoff / energy < cutoff and no Fail;
        otherwise the episode ends without storing it; the episode is truncated at t_max = 100
The experience row layout is the reference's: [last_obs, obs, last_action, reward]
(IHO/main_parallel.py:250-257), so the deep-Q consumer drops in unchanged. With input='wavefunction'
the observation is get_data_wavefunction(state) * input_scaling: float32 hstack(Re, Im) of state[:-10]
(HO, HO/main_parallel.py:132-134), state[:-20] (IHO, IHO/main_parallel.py:133-135) or state[10:-10]
(grid, IQO/main_parallel.py:136-137)
(qc_wavefunction_obs). With input='measurements'
(HO, IHO; IHO/main_parallel.py:143-151,270-309) the observation is the device measurement record
[B][2][read_length] (measurements.MeasurementRecord, updated in place by the qc_record kernel) and the
experience rows [B][row_len] come from the same kernel (info['rows']).

Auto-reset modes (reset="deferred": HO, IHO and IQO with every input they have; QO's reset is hundreds of control
intervals, no one-interval reset: it has "immediate" and "warmup"):
  * reset="immediate" (default): a finished env is reset and runs its zero-force first interval inside the same
    step() call, so the returned obs of a done env is already the next episode's first observation (the terminal
    one is info['terminal_obs']) — the reference actor's own interleaving; one more (partial) step launch and a few
    host synchronisations per call.
  * reset="deferred": a finished env returns its terminal obs and runs its reset interval (|0> / the IQO packet at
    F = 0) in the NEXT call, inside the same step launch as the other envs (its action of that call is ignored,
    info['reset'] marks it, no valid transition); the per-control-step bookkeeping (reward, done, return, episode
    time, the finished-episode ring) is one device kernel (qc_env_tail) and the call never synchronises with the
    host. Every env's own sequence — reset, zero-force interval, decisions on its observations, per-env noise — is
    the immediate mode's (tests/test_gpu_env.py: per-env episodes bitwise equal); only the calls they fall in
    differ, and every call advances every env exactly one control interval. HO: qc_phonon_number runs before the
    tail, which applies the cooling rules (cutoff, truncation at t_max, reward -phonon * scale, the terminal
    transition not valid). 'wavefunction': the returned and stored observation is qc_wavefunction_obs of the
    states after the call. 'measurements': the tail also writes qc_record's per-env mode (fresh history for an
    env in its reset interval, append otherwise); obs is the record, which holds a done env's terminal record
    until the next call restarts it, and info['rows'] / info['valid'] are the immediate mode's
    (tests/test_gpu_env_deferred_inputs.py: per-env rows and episodes bitwise equal).
  * reset="warmup" (QO only, 'xp' and 'wavefunction'): a finished env, or one whose warm-up was rejected, draws a
    new packet (k, evolution time from init_time) on the device and runs its free evolution inside the following
    calls' step launches, control_interval physics steps per call (the last call fewer: per-env step budgets), while
    the other envs are controlled. Every call is one masked packet reset, one step, one energy and one tail kernel
    (qc_env_tail, kind QC_QO) and never synchronises with the host. A warming env's action is ignored
    (info['warming']), it returns reward 0, done False and no valid transition; in the call that ends an accepted
    warm-up info['reset'] is set and the returned observation is the episode's first (QO decides at i = 0). A
    transition is valid exactly when the env was live on entry and is not done. reset() only starts the warm-ups
    and returns the observation buffer as it is. The draws come from the env's own Philox stream, not
    from the immediate mode's torch generator, and the warm-up runs in control intervals instead of 1440-step
    launches: the scheme is the immediate mode's, the trajectories are not bitwise its.

performance_from (HO and QO, optional): the cooling drivers' per-episode performance, the mean phonon number / energy
over the control steps whose episode time is past it (HO/main_parallel.py:247-248, 294-295; QO/main_parallel.py:221,
231-232): a step that ends the episode is not counted, and only an episode truncated at t_max with at least one counted
step reports its mean, every other one the cutoff. It goes to a ring beside the finished-episode ring, at the same
position (performance_ring, finished_performances): qc_env_tail keeps it in the deferred and warm-up modes, the
immediate mode by the same add and divide in torch, so an env's performances are bitwise the same in both.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib as L
from . import config as cfg
from .core import Stepper
from .measurements import MeasurementRecord


class BatchedEnv:
    def __init__(self, physics: cfg.Physics, batch: int, device: int | str | torch.device = 0, seed: int = 0,
                 env_offset: int = 0, input_scaling: float = 1.0, failing_reward: float = -1.0,
                 reward_multiply: float = 1.0, t_max: float = 100.0, phonon_cutoff: float = 20.0,
                 energy_cutoff: float = 12.0, init_energy_cutoff: float = 7.5, auto_reset: bool = True,
                 reset_kind: str = "reference", input: str = "xp", read_length: Optional[int] = None,
                 reset: str = "immediate", init_time: tuple = (15.0, 20.0),
                 performance_from: Optional[float] = None):
        self.ph = physics
        self.B = int(batch)
        self.st = Stepper(physics, self.B, device, seed=seed, env_offset=env_offset)
        self.dev = self.st.device
        self.psi = self.st.new_state()
        self.ci = physics.control_interval
        self.half = physics.n_actions // 2
        self.input_scaling = input_scaling
        self.failing_reward = failing_reward
        self.reward_multiply = reward_multiply
        self.t_max = t_max
        self.phonon_cutoff = phonon_cutoff
        self.energy_cutoff = energy_cutoff
        self.init_energy_cutoff = init_energy_cutoff
        # QO: the free evolution of a reset lasts U[init_time] time units (QO/main_parallel.py:186)
        self.init_time = (float(init_time[0]), float(init_time[1]))
        if not 0.0 <= self.init_time[0] <= self.init_time[1] < float("inf"):
            raise ValueError("init_time must be (lo, hi) with 0 <= lo <= hi")
        self.auto_reset = auto_reset
        self.reset_kind = reset_kind
        self.cartpole = physics.family in (cfg.IHO, cfg.IQO)
        # no control at the zero-th step: the first decision follows one zero-force interval (IHO:250,
        # IQO:201, HO:238); QO decides at i = 0 (QO:208)
        self.first_interval = physics.family != cfg.QO
        if input not in ("xp", "wavefunction", "measurements"):
            raise ValueError("input must be 'xp', 'wavefunction' or 'measurements'")
        if input == "measurements" and not physics.fock:
            raise ValueError("the 'measurements' input exists for the Fock families (HO, IHO) only")
        self.input = input
        if reset not in ("immediate", "deferred", "warmup"):
            raise ValueError("reset must be 'immediate', 'deferred' or 'warmup'")
        if reset == "warmup" and physics.family != cfg.QO:
            raise ValueError("reset='warmup' is the quartic cooling driver's (QO) rolling reset; HO, IHO and IQO have "
                             "a one-interval reset: use reset='deferred'")
        if reset == "warmup" and not auto_reset:
            raise ValueError("reset='warmup' is an auto-reset mode: it needs auto_reset")
        if reset == "deferred" and physics.family == cfg.QO:
            raise ValueError("reset='deferred' needs a one-interval reset: QO's is a random packet evolved freely for "
                             "U[15, 20] time units and redrawn until accepted (QO/main_parallel.py:177-198), hundreds "
                             "of control intervals; use reset='warmup' (or 'immediate')")
        if reset == "deferred" and not auto_reset:
            raise ValueError("reset='deferred' is an auto-reset mode (HO, IHO, IQO): it needs auto_reset")
        self.reset_mode = reset
        # the cooling drivers' per-episode performance: the mean phonon number (HO) / energy (QO) over the control
        # steps past this episode time (HO:247-248, 294-295; QO:221, 231-232); None: not kept
        if performance_from is not None and self.cartpole:
            raise ValueError("performance_from is the cooling drivers' (HO, QO) per-episode performance: the "
                             "cartpoles (IHO, IQO) are measured by their episode time")
        self.performance_from = None if performance_from is None else float(performance_from)
        # what a state_dict echoes and load_state_dict compares (the stepper and the record add their own)
        self._made = {"kind": "BatchedEnv", "family": physics.family, "B": self.B, "env_offset": int(env_offset),
                      "input": input, "reset": reset, "reset_kind": reset_kind, "seed": int(seed),
                      "auto_reset": bool(auto_reset), "input_scaling": float(input_scaling),
                      "failing_reward": float(failing_reward), "reward_multiply": float(reward_multiply),
                      "t_max": float(t_max), "phonon_cutoff": float(phonon_cutoff),
                      "energy_cutoff": float(energy_cutoff), "init_energy_cutoff": float(init_energy_cutoff),
                      "init_time": self.init_time}
        if self.performance_from is not None:
            self._made["performance_from"] = self.performance_from
        self._pending = torch.zeros(self.B, dtype=torch.uint8, device=self.dev)
        self._calls = 0
        self.rec = None
        if input == "measurements":
            self.rec = MeasurementRecord(self.st, read_length, input_scaling=input_scaling)
            self.rows = torch.empty((self.B, self.rec.row_len), dtype=torch.float32, device=self.dev)
        self.gen = torch.Generator(device=self.dev).manual_seed(int(seed) * 7919 + int(env_offset))
        z = lambda dt: torch.zeros(self.B, dtype=dt, device=self.dev)  # noqa: E731
        self.t = z(torch.float64)                 # episode time
        self.steps = z(torch.int64)               # physics steps in the episode
        self.last_action = torch.full((self.B,), self.half, dtype=torch.int32, device=self.dev)
        obs_len = self.st.wavefunction_len() if input == "wavefunction" else self.st.n_obs
        self.obs = (self.rec.hist if self.rec is not None else
                    torch.zeros((self.B, obs_len), dtype=torch.float32, device=self.dev))
        self.episode_return = z(torch.float64)
        # finished episodes (return, length) compacted on the device into a ring of _fin_cap entries
        # (slot _fin_cap is the sink of the not-finished envs): no boolean indexing, no dynamic shapes and
        # no host copy per step; read through finished_returns
        self._fin_cap = max(1 << 16, 16 * self.B)
        self._fin = torch.zeros((2, self._fin_cap + 1), dtype=torch.float64, device=self.dev)
        self._fin_n = torch.zeros((), dtype=torch.int64, device=self.dev)
        self._fin_read = 0
        self._fin_host: list = []
        if self.performance_from is not None:
            # the running sum and count of the episode, and the finished episodes' performance at the ring
            # position of their (return, length) (slot _fin_cap: the sink)
            self._perf_sum = z(torch.float64)
            self._perf_n = z(torch.int64)
            self._perf = torch.zeros(self._fin_cap + 1, dtype=torch.float64, device=self.dev)
            self._perf_read = 0
            self._perf_host: list = []
        if reset == "warmup":
            # per-env warm-up state, advanced by qc_env_tail (kind QC_QO) and started by qc_env_warmup_draw
            self._seed, self._env_offset = int(seed), int(env_offset)
            self._warm_left = z(torch.int32)      # physics steps of free evolution still to run; warming iff > 0
            self._warm_fail = z(torch.uint8)      # a Fail was seen during this warm-up
            self._draws = z(torch.int64)          # reset draws consumed
            self._k = z(torch.float64)            # the packet's wavenumber
            self._budget = torch.full((self.B,), self.ci, dtype=torch.int32, device=self.dev)   # next call's env_steps
            self._mean0, self._std1 = z(torch.float64), torch.ones(self.B, dtype=torch.float64, device=self.dev)

    @property
    def finished_returns(self) -> list:
        """(returns, lengths) float64 CPU tensors of the episodes finished so far, one entry per read
        that found new ones (the reference's per-actor result queue, main_parallel.py:300-327). At most
        the last _fin_cap episodes between two reads are kept."""
        n = int(self._fin_n)
        if n > self._fin_read:
            lo = max(self._fin_read, n - self._fin_cap)
            idx = torch.arange(lo, n, device=self.dev) % self._fin_cap
            vals = self._fin[:, idx].cpu()
            self._fin_host.append((vals[0], vals[1]))
            self._fin_read = n
        return self._fin_host

    def finished_ring(self):
        """(fin, fin_cap, fin_n): the device ring of finished episodes as qc_env_tail writes it, fin [2, fin_cap + 1]
        float64 (returns, lengths; entry i at column i % fin_cap) and fin_n, the int64 device scalar of episodes
        appended so far. No copy and no synchronisation: a device consumer (train.Schedule) reads it in stream order."""
        return self._fin, self._fin_cap, self._fin_n

    def performance_ring(self):
        """(perf, fin_cap, fin_n): the device ring of the finished episodes' performance, perf [fin_cap + 1] float64
        with entry i at column i % fin_cap, the position of its (return, length) in finished_ring(). No copy and no
        synchronisation. Needs performance_from."""
        if self.performance_from is None:
            raise ValueError("this env keeps no performance: make it with performance_from")
        return self._perf, self._fin_cap, self._fin_n

    @property
    def finished_performances(self) -> list:
        """float64 CPU tensors of the performances of the episodes finished so far, one entry per read that found
        new ones, with a read position of its own (finished_returns' is not moved). At most the last _fin_cap
        episodes between two reads are kept. Needs performance_from."""
        if self.performance_from is None:
            raise ValueError("this env keeps no performance: make it with performance_from")
        n = int(self._fin_n)
        if n > self._perf_read:
            lo = max(self._perf_read, n - self._fin_cap)
            idx = torch.arange(lo, n, device=self.dev) % self._fin_cap
            self._perf_host.append(self._perf[idx].cpu())
            self._perf_read = n
        return self._perf_host

    def _push_finished(self, done: torch.Tensor, ret: torch.Tensor, length: torch.Tensor,
                       perf: Optional[torch.Tensor] = None):
        """Append the finished episodes (env order) to the device ring, no host sync."""
        pos = self._fin_n + torch.cumsum(done, 0) - 1
        slot = torch.where(done, pos % self._fin_cap, torch.full_like(pos, self._fin_cap))
        self._fin[0].index_copy_(0, slot, ret)   # duplicates only into the sink
        self._fin[1].index_copy_(0, slot, length)
        if perf is not None:
            self._perf.index_copy_(0, slot, perf)
        self._fin_n += done.sum()

    # ------------------------------------------------------------------ observation
    def _observe(self) -> torch.Tensor:
        if self.input == "wavefunction":
            return self.st.wavefunction_obs(self.psi, self.input_scaling)
        return self.st.moments(self.psi).to(torch.float32) * self.input_scaling

    def _quantity(self) -> torch.Tensor:
        """cooling reward quantity: phonon number (HO) / energy (QO)."""
        if self.ph.family == cfg.HO:
            return self.st.phonon_number(self.psi)
        return self.st.energy(self.psi)

    # ------------------------------------------------------------------ reset
    def _reset_states(self, mask: torch.Tensor):
        m8 = mask.to(torch.uint8)
        fam = self.ph.family
        if fam in (cfg.HO, cfg.IHO):
            if self.reset_kind == "synthetic":
                self.st.reset(self.psi, 1, mask=m8, arg0=16)
            else:
                self.st.reset(self.psi, 0, mask=m8)
        elif fam == cfg.IQO:
            self.st.reset(self.psi, 2, mask=m8, arg0=0.0, arg1=0.0, arg2=1.0)
        else:
            self._reset_quartic_cooling(mask)

    def _reset_quartic_cooling(self, mask: torch.Tensor):
        """QO/main_parallel.py:177-198: random-k packet, free evolution for U[15,20] time units, redrawn
        until energy < init_energy_cutoff and no Fail."""
        todo = mask.clone()
        dt = self.ph.dt
        rounds = 0
        while bool(todo.any()):
            rounds += 1
            if rounds > 1000:   # the reference redraws without bound; a broken scheme would spin forever
                raise RuntimeError("quartic cooling reset: no acceptable initial state after 1000 redraws")
            k = (torch.rand(self.B, generator=self.gen, device=self.dev, dtype=torch.float64) * 0.6 - 0.3)
            mu = torch.zeros(self.B, dtype=torch.float64, device=self.dev)
            sg = torch.ones(self.B, dtype=torch.float64, device=self.dev)
            self.st.reset(self.psi, 2, mask=todo.to(torch.uint8), k=k, mean=mu, std=sg)
            lo, hi = self.init_time
            init_t = torch.rand(self.B, generator=self.gen, device=self.dev, dtype=torch.float64) * (hi - lo) + lo
            budget = torch.where(todo, torch.ceil(init_t / dt).to(torch.int32), torch.zeros_like(init_t, dtype=torch.int32))
            failed = torch.zeros(self.B, dtype=torch.bool, device=self.dev)
            chunk = 1440
            while bool((budget > 0).any()):
                out = self.st.step(self.psi, None, chunk, default_action=self.half,
                                   env_steps=torch.clamp(budget, max=chunk).to(torch.int32))
                failed |= out["fail_step"] > 0
                budget = torch.clamp(budget - chunk, min=0)
            ok = (self._quantity() < self.init_energy_cutoff) & ~failed
            todo = todo & ~ok

    def reset(self, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Start new episodes (all, or where mask); returns the observation at the first decision."""
        if mask is None:
            mask = torch.ones(self.B, dtype=torch.bool, device=self.dev)
        mask = mask.to(device=self.dev, dtype=torch.bool)
        if self.reset_mode == "warmup":
            # the masked envs start a warm-up (a pending packet of an earlier draw is replaced by the new one); the
            # first real observation of an env is the one flagged by info['reset']
            a = self._warmup_args()
            self.st._bind_stream()
            m8 = mask.to(torch.uint8).contiguous()
            L.check(L.lib().qc_env_warmup_draw(self.st._h, ctypes.byref(a), ctypes.c_void_p(m8.data_ptr())),
                    self.st._h)
            self.last_action = torch.where(mask, torch.full_like(self.last_action, self.half), self.last_action)
            return self.obs
        self._pending.masked_fill_(mask, 0)   # (reset='deferred': a pending reset is done here instead)
        self._reset_states(mask)
        self.t = torch.where(mask, torch.zeros_like(self.t), self.t)
        self.steps = torch.where(mask, torch.zeros_like(self.steps), self.steps)
        self.episode_return = torch.where(mask, torch.zeros_like(self.episode_return), self.episode_return)
        self.last_action = torch.where(mask, torch.full_like(self.last_action, self.half), self.last_action)
        keep_perf = self.performance_from is not None
        if keep_perf:   # a new episode's performance starts from nothing
            self._perf_sum = torch.where(mask, torch.zeros_like(self._perf_sum), self._perf_sum)
            self._perf_n = torch.where(mask, torch.zeros_like(self._perf_n), self._perf_n)
        first_q = None
        if self.first_interval:
            # no control at the zero-th step: one zero-force interval first (IHO:242-268, IQO:190-221,
            # HO:237-257). An episode that already ends at i = control_interval stores no transition
            # (i != control_interval guard, IHO:250) but is still reported with its length t (the
            # (experience, t, numerical_failure) / (t,) queue puts, IHO:312-313) and restarted here.
            fam = self.ph.family
            todo = mask.clone()
            while bool(todo.any()):
                budget = torch.where(todo, torch.full_like(self.last_action, self.ci), torch.zeros_like(self.last_action))
                out = self.st.step(self.psi, None, self.ci, default_action=self.half, env_steps=budget,
                                   want_term=(fam == cfg.IQO), want_obs=True, want_q=self.rec is not None)
                if self.rec is not None:   # the record starts at i = 0 from empty lists (IHO:271-272)
                    self.rec.record(out["q"], None, self.half, mode=todo.to(torch.uint8) * 2)
                bad = out["fail_step"] > 0
                if fam == cfg.IQO:
                    bad |= out["term_step"] >= 0
                elif fam == cfg.IHO:
                    bad |= out["obs"][:, 0].abs() > self.ph.xth
                else:   # HO: phonon > cutoff at the first control step ends the episode (HO:240-246)
                    # (every pass steps only the envs it redoes, so the last pass's value is every masked env's
                    # phonon number after its own first interval)
                    first_q = self.st.phonon_number(self.psi)
                    bad |= first_q > self.phonon_cutoff
                bad &= todo
                if bool(bad.any()):
                    length = torch.where(mask, self.t + self.ci * self.ph.dt, self.t)
                    # (nothing was counted yet: such an episode's performance is the cutoff)
                    self._push_finished(bad, torch.zeros_like(self.t), length,
                                        torch.full_like(self.t, self.phonon_cutoff) if keep_perf else None)
                    self._reset_states(bad)
                todo = bad
            self.t = torch.where(mask, self.t + self.ci * self.ph.dt, self.t)
            self.steps = torch.where(mask, self.steps + self.ci, self.steps)
            if keep_perf and first_q is not None:
                # HO's first control step is a live one (HO:247-248): it counts when it is past performance_from
                acc = mask & (self.t > self.performance_from)
                self._perf_sum = torch.where(acc, self._perf_sum + first_q, self._perf_sum)
                self._perf_n = self._perf_n + acc
        if self.rec is not None:
            self.obs = self.rec.hist
            return self.obs
        obs = self._observe()
        self.obs = torch.where(mask[:, None], obs, self.obs)
        return self.obs

    # ------------------------------------------------------------------ step
    def _step_deferred(self, actions: torch.Tensor):
        """reset='deferred': the envs finished in the previous call take their reset interval now (reset kernel +
        the zero force in the same step launch), then qc_env_tail does the bookkeeping on the device."""
        fam = self.ph.family
        pend = self._pending
        reset_now = pend.clone().view(torch.bool)
        self._reset_states(reset_now)   # the immediate mode's reset (reset_kind included), masked
        acts = torch.where(reset_now, torch.full_like(actions, self.half), actions)
        # the immediate mode's step call (the same outputs asked for, so the same kernels)
        out = self.st.step(self.psi, acts, self.ci, want_fail=True, want_obs=True, want_term=(fam == cfg.IQO),
                           want_q=self.rec is not None)
        B, n = self.B, self.st.n_obs
        cooling = fam == cfg.HO
        quantity = self.st.phonon_number(self.psi) if cooling else None
        obs = torch.empty((B, n), dtype=torch.float32, device=self.dev) if self.input == "xp" else None
        rec_mode = torch.empty(B, dtype=torch.uint8, device=self.dev) if self.rec is not None else None
        reward = torch.empty(B, dtype=torch.float32, device=self.dev)
        done = torch.empty(B, dtype=torch.uint8, device=self.dev)
        valid = torch.empty(B, dtype=torch.uint8, device=self.dev)
        p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        a = L.QcEnvTailArgs(B=B, kind=fam, n_obs=n, interval=self.ci, dt=self.ph.dt, xth=self.ph.xth,
                            input_scaling=self.input_scaling, failing_reward=self.failing_reward,
                            fail_step=p(out["fail_step"]), term_step=p(out.get("term_step")), obs=p(out["obs"]),
                            pending=p(pend), t=p(self.t), steps=p(self.steps), episode_return=p(self.episode_return),
                            obs32=p(obs), reward=p(reward), done=p(done), valid=p(valid), fin=p(self._fin),
                            fin_cap=self._fin_cap, fin_n=p(self._fin_n), quantity=p(quantity),
                            cutoff=self.phonon_cutoff if cooling else 0.0,
                            t_trunc=self.t_max - 0.01 * self.ph.dt if cooling else 0.0,
                            reward_multiply=self.reward_multiply if cooling else 0.0, rec_mode=p(rec_mode),
                            **self._perf_args())
        self.st._bind_stream()
        L.check(L.lib().qc_env_tail(self.st._h, ctypes.byref(a)), self.st._h)
        valid_b = valid.view(torch.bool)
        info = {"valid": valid_b, "reset": reset_now}
        last_obs = self.obs
        if self.rec is not None:
            # mode 2 (pending on entry) starts the history from empty lists (IHO:271-272), mode 1 appends; the
            # hist of a done env holds its terminal record until the next call restarts it
            self.rec.record(out["q"], acts, self.half, mode=rec_mode, reward=reward, rows=self.rows)
            info["rows"] = self.rows
            obs = self.rec.hist
            last_obs = None   # (the record is updated in place: the rows carry both control steps)
        elif self.input == "wavefunction":
            obs = self.st.wavefunction_obs(self.psi, self.input_scaling)
        self.obs = obs
        self.last_action = acts
        self._calls += 1
        if self._calls % 16 == 0:   # deferred action-range errors, at most 16 calls late (synchronises)
            self.st.check()
        done_b = done.view(torch.bool)
        info.update({"t": self.t.clone(), "last_obs": last_obs, "fail_step": out["fail_step"],
                     "numerical_failure": done_b & (out["fail_step"] > 0)})
        return obs, reward, done_b, info

    def _perf_args(self) -> dict:
        """qc_env_tail_args' performance fields (none without performance_from)."""
        if self.performance_from is None:
            return {}
        return dict(perf_sum=self._perf_sum.data_ptr(), perf_n=self._perf_n.data_ptr(), perf=self._perf.data_ptr(),
                    perf_from=self.performance_from)

    def _warmup_args(self, **kw):
        """qc_env_tail_args of the warm-up mode: the per-env state and the draw parameters (kw: the per-call fields)."""
        p = lambda t: t.data_ptr()   # noqa: E731
        return L.QcEnvTailArgs(
            B=self.B, kind=cfg.QO, n_obs=self.st.n_obs, interval=self.ci, dt=self.ph.dt,
            input_scaling=self.input_scaling, pending=p(self._pending), t=p(self.t), steps=p(self.steps),
            episode_return=p(self.episode_return), fin=p(self._fin), fin_cap=self._fin_cap, fin_n=p(self._fin_n),
            cutoff=self.energy_cutoff, t_trunc=self.t_max - 0.01 * self.ph.dt, reward_multiply=self.reward_multiply,
            warm_left=p(self._warm_left), warm_fail=p(self._warm_fail), draws=p(self._draws), k=p(self._k),
            budget=p(self._budget), init_energy_cutoff=self.init_energy_cutoff, init_lo=self.init_time[0],
            init_hi=self.init_time[1], seed=self._seed, env_offset=self._env_offset, **self._perf_args(), **kw)

    def _step_warmup(self, actions: torch.Tensor):
        """reset='warmup' (QO): the packets of the new draws, one step launch with per-env budgets (a warming env at
        zero force), the energy, then qc_env_tail's QO branch: accounting, warm-up bookkeeping and redraws."""
        warming = self._warm_left > 0
        self.st.reset(self.psi, L.QC_RESET_GAUSSIAN, mask=self._pending, k=self._k, mean=self._mean0, std=self._std1)
        acts = torch.where(warming, torch.full_like(actions, self.half), actions)
        out = self.st.step(self.psi, acts, self.ci, env_steps=self._budget, want_fail=True, want_obs=True)
        energy = self.st.energy(self.psi)
        B = self.B
        obs = torch.empty((B, self.st.n_obs), dtype=torch.float32, device=self.dev) if self.input == "xp" else None
        reward = torch.empty(B, dtype=torch.float32, device=self.dev)
        done = torch.empty(B, dtype=torch.uint8, device=self.dev)
        valid = torch.empty(B, dtype=torch.uint8, device=self.dev)
        went_live = torch.empty(B, dtype=torch.uint8, device=self.dev)
        a = self._warmup_args(fail_step=out["fail_step"].data_ptr(), obs=out["obs"].data_ptr(),
                              obs32=obs.data_ptr() if obs is not None else None, reward=reward.data_ptr(),
                              done=done.data_ptr(), valid=valid.data_ptr(), quantity=energy.data_ptr(),
                              reset_out=went_live.data_ptr())
        self.st._bind_stream()
        L.check(L.lib().qc_env_tail(self.st._h, ctypes.byref(a)), self.st._h)
        if self.input == "wavefunction":
            obs = self.st.wavefunction_obs(self.psi, self.input_scaling)
        last_obs = self.obs
        self.obs = obs
        self.last_action = acts
        self._calls += 1
        if self._calls % 16 == 0:   # deferred action-range errors, at most 16 calls late (synchronises)
            self.st.check()
        done_b = done.view(torch.bool)
        info = {"valid": valid.view(torch.bool), "reset": went_live.view(torch.bool), "warming": warming,
                "t": self.t.clone(), "last_obs": last_obs, "fail_step": out["fail_step"],
                "numerical_failure": done_b & (out["fail_step"] > 0)}
        return obs, reward, done_b, info

    def step(self, actions: torch.Tensor):
        """Apply per-env actions for one control interval. Returns (obs, reward, done, info):
        reward is the reference's stored reward-row value, info['valid'] marks transitions the
        reference would store, info['numerical_failure'] the Fail-terminated episodes."""
        actions = actions.to(device=self.dev, dtype=torch.int32).contiguous()
        if self.reset_mode == "deferred":
            return self._step_deferred(actions)
        if self.reset_mode == "warmup":
            return self._step_warmup(actions)
        last_obs = self.obs
        fam = self.ph.family
        out = self.st.step(self.psi, actions, self.ci, want_fail=True, want_obs=True,
                           want_term=(fam == cfg.IQO), want_q=self.rec is not None)
        fail = out["fail_step"] > 0
        if self.input == "wavefunction":
            obs = self.st.wavefunction_obs(self.psi, self.input_scaling)
        else:
            obs = out["obs"].to(torch.float32) * self.input_scaling
        self.t = self.t + self.ci * self.ph.dt
        self.steps = self.steps + self.ci
        if self.cartpole:
            numerical = fail                                     # Fail during the interval (IHO:243-267)
            if fam == cfg.IHO:
                out_of_bounds = out["obs"][:, 0].abs() > self.ph.xth   # |x_expectation| > xth (IHO:246)
            else:
                out_of_bounds = out["term_step"] >= 0                 # outside prob > 0.5 (IQO:199-200)
            done = numerical | out_of_bounds
            reward = torch.where(done, torch.full_like(self.t, self.failing_reward), torch.ones_like(self.t))
            valid = torch.ones_like(done)
        else:
            q = self._quantity()
            cutoff = self.phonon_cutoff if fam == cfg.HO else self.energy_cutoff
            ok = (q <= cutoff) if fam == cfg.HO else (q < cutoff)
            truncated = self.t >= self.t_max - 0.01 * self.ph.dt
            done = fail | ~ok | truncated
            reward = -q * self.reward_multiply
            valid = ~done
            numerical = fail
            if self.performance_from is not None:
                # one add and one divide under qc_env_tail's conditions: a terminal step adds nothing, and only a
                # truncated episode that counted something reports its mean, every other one the cutoff
                acc = valid & (self.t > self.performance_from)
                self._perf_sum = torch.where(acc, self._perf_sum + q, self._perf_sum)
                self._perf_n = self._perf_n + acc
                perf = torch.where(truncated & (self._perf_n > 0), self._perf_sum / self._perf_n.to(torch.float64),
                                   torch.full_like(q, cutoff))
        self.episode_return = self.episode_return + torch.where(valid, reward, torch.zeros_like(reward))
        info = {"valid": valid, "numerical_failure": numerical & done, "t": self.t.clone(),
                "last_obs": last_obs if self.rec is None else None, "fail_step": out["fail_step"]}
        if self.rec is not None:
            # the continuous record of the two control steps, forces and (action, reward) (IHO:270-283)
            self.rec.record(out["q"], actions, self.half, reward=reward.to(torch.float32), rows=self.rows)
            info["rows"] = self.rows
            obs = self.rec.hist
        self.last_action = actions
        self.obs = obs
        self.st.check()   # deferred action-range errors of this interval's step (synchronises, as done.any() does)
        if bool(done.any()):
            if self.rec is None:   # measurement mode: the rows hold the terminal record
                info["terminal_obs"] = obs.clone()
            info["episode_return"] = self.episode_return.clone()
            info["episode_length"] = self.t.clone()
            if self.performance_from is not None:
                info["episode_performance"] = perf.clone()
                self._push_finished(done, self.episode_return, self.t, perf)
            else:
                self._push_finished(done, self.episode_return, self.t)
            if self.auto_reset:
                self.reset(done)
        return self.obs, reward.to(torch.float32), done, info

    # ------------------------------------------------------------------ checkpoint
    _WARM = ("_warm_left", "_warm_fail", "_draws", "_k", "_budget", "_mean0", "_std1")

    def _state_tensors(self) -> list:
        names = ["psi", "_pending", "t", "steps", "last_action", "episode_return", "_fin", "_fin_n"]
        if self.rec is None:
            names.append("obs")    # ('measurements': obs is the record's hist)
        else:
            names.append("rows")
        if self.reset_mode == "warmup":
            names += self._WARM
        if self.performance_from is not None:
            names += ["_perf_sum", "_perf_n", "_perf"]
        return names

    def _made_for(self) -> dict:
        return {**self._made, "read_length": self.rec.read_length if self.rec is not None else None}

    def state_dict(self) -> dict:
        """The whole env as CPU values (checkpoint.save): psi and every per-env tensor (pending resets, episode time,
        steps and return, last action, the observation or the measurement rows, the warm-up mode's draw state), the
        finished-episode ring with its write and read positions (so that finished_returns reports no episode twice;
        the list of already-read ones is the caller's and is not saved), the call count, the torch generator of the
        immediate mode's resets, the record's and the stepper's state; and what the env was made for, which
        load_state_dict compares. Synchronises the device."""
        st = dict(self._made_for())
        for name in self._state_tensors():
            st[name] = getattr(self, name).cpu()
        st["_fin_read"] = int(self._fin_read)
        if self.performance_from is not None:
            st["_perf_read"] = int(self._perf_read)
        st["_calls"] = int(self._calls)
        st["generator"] = self.gen.get_state().cpu()
        st["record"] = self.rec.state_dict() if self.rec is not None else None
        st["stepper"] = self.st.state_dict()
        return st

    def check_state_dict(self, state: dict):
        """Raise ValueError naming the first field of `state` this env was not made for (family and physics, B,
        env_offset, input, reset mode, reset_kind, read_length, seed, the episode rules), or a tensor of another
        shape. Changes nothing."""
        names = self._state_tensors()
        keep_perf = self.performance_from is not None
        if not keep_perf and isinstance(state, dict) and "performance_from" in state:
            raise ValueError(f"BatchedEnv: performance_from differs: the state was made for "
                             f"{state['performance_from']!r}, this object for None")
        L.check_echo("BatchedEnv", state, self._made_for(),
                    names + ["_fin_read", "_calls", "generator", "record", "stepper"]
                    + (["_perf_read"] if keep_perf else []))
        self.st.check_state_dict(state["stepper"])
        if self.rec is not None:
            self.rec.check_state_dict(state["record"])
        for name in names:
            have, got = getattr(self, name), state[name]
            if got.shape != have.shape or got.dtype != have.dtype:
                raise ValueError(f"BatchedEnv: {name} is {got.dtype} {tuple(got.shape)}, not {have.dtype} "
                                 f"{tuple(have.shape)}")

    def load_state_dict(self, state: dict):
        """Continue from a `state_dict()`: every later step() gives bit for bit what the saved env would have.
        An env made with other arguments is refused with a ValueError naming the first difference, before anything
        changes (nothing is converted: not the batch, the input, the reset mode or env_offset)."""
        self.check_state_dict(state)
        self.st.load_state_dict(state["stepper"])
        if self.rec is not None:
            self.rec.load_state_dict(state["record"])
        for name in self._state_tensors():
            have = getattr(self, name)
            if name in ("obs", "last_action", "t", "steps", "episode_return", "_perf_sum", "_perf_n"):
                # replaced, not written, by step()
                setattr(self, name, state[name].to(self.dev))
            else:
                have.copy_(state[name])
        self._fin_read = int(state["_fin_read"])
        if self.performance_from is not None:
            self._perf_read = int(state["_perf_read"])
        self._calls = int(state["_calls"])
        self.gen.set_state(state["generator"])
        if self.rec is not None:
            self.obs = self.rec.hist

    def analytic_actions(self, strategy: str = "LQG", con_parameter: float = 0.0) -> torch.Tensor:
        """Actions of the reference's analytic baseline controllers for the current states (qc_control):
        Fock args.LQG on the 'xp' network input (IHO/main_parallel.py:194-206), grid
        args.control_strategy in {'LQG', 'damping', 'semiclassical'} (QO/main_parallel.py:165-181)."""
        # the 'xp' input hands the scaled network input to call_force; other inputs pass the unscaled
        # get_data_xp(state) (IHO:259-262)
        sc = self.input_scaling if self.input == "xp" else 1.0
        act, _ = self.st.control(self.psi, strategy, con_parameter, input_scaling=sc)
        return act

    def probability(self, view, mean: bool = False, mask: Optional[torch.Tensor] = None):
        """The position-space density of the current states through a spatial.SpatialView made for this physics
        (SpatialView.for_physics): `view.probability(self.psi)` [B, X], or with mean = True
        `view.mean_probability(self.psi, mask)`, the pair (ensemble mean [X], count) over the envs whose mask is set.
        Reads psi only: the env's state is unchanged."""
        if mean:
            return view.mean_probability(self.psi, mask)
        if mask is not None:
            raise ValueError("BatchedEnv.probability: mask goes with mean = True")
        return view.probability(self.psi)

    def wigner(self, view, mean: bool = False, mask: Optional[torch.Tensor] = None):
        """The Wigner function of the current states through a wigner.WignerView made for this physics
        (WignerView.for_physics): `view.wigner(self.psi)` [B, X, P], or with mean = True
        `view.mean_wigner(self.psi, mask)`, the pair (ensemble mean [X, P], count) over the envs whose mask is set.
        Reads psi only: the env's state is unchanged."""
        if mean:
            return view.mean_wigner(self.psi, mask)
        if mask is not None:
            raise ValueError("BatchedEnv.wigner: mask goes with mean = True")
        return view.wigner(self.psi)

    def density_matrix(self, view, mask: Optional[torch.Tensor] = None):
        """The ensemble density matrix of the current states through an ensemble.EnsembleView made for this physics
        (EnsembleView.for_physics): `view.density_matrix(self.psi, mask)`, the pair (rho [N, N], count) over the envs
        whose mask is set. Reads psi only: the env's state is unchanged."""
        return view.density_matrix(self.psi, mask)

    def level_populations(self, view, mean: bool = False, mask: Optional[torch.Tensor] = None):
        """The energy-level populations of the current states through a levels.LevelView made for this physics
        (LevelView.for_physics): `view.populations(self.psi)` [B, K], or with mean = True
        `view.mean_populations(self.psi, mask)`, the pair (ensemble mean [K], count) over the envs whose mask is set.
        Reads psi only: the env's state is unchanged."""
        if mean:
            return view.mean_populations(self.psi, mask)
        if mask is not None:
            raise ValueError("BatchedEnv.level_populations: mask goes with mean = True")
        return view.populations(self.psi)

    def master_equation(self, forces=None):
        """A lindblad.MasterEquation for this env's physics, dt, gamma and device (forces None: the discrete forces,
        slot = action): the open-loop evolution of density matrices. It never reads or writes the env's states."""
        from .lindblad import MasterEquation
        return MasterEquation(self.ph, forces, device=self.dev)

    @staticmethod
    def experience(last_obs: torch.Tensor, obs: torch.Tensor, action: torch.Tensor, reward: torch.Tensor):
        """Experience rows in the reference layout np.hstack((last_data, data, [last_action], [reward]))."""
        return torch.cat([last_obs, obs, action.to(torch.float32)[:, None], reward.to(torch.float32)[:, None]], 1)
