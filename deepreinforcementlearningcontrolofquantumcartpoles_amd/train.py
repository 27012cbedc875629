"""The drivers' training run on one device: the schedule the reference decides from the stream of finished episodes,
kept on the device (`Schedule`, csrc/qcart_sched.hip), and the loop that obeys it (`Trainer`).

What the reference spreads over two processes is one kernel launch per control step here:
- the loader loop of each driver's RL.py (IHO:497-535, IQO:495-533, HO:491-538, QO:477-527): update pacing
  (pending_training_updates, 8/256 per stored row), "learning in progress" (the cartpoles' exponential average of the
  episode time with a start and a fall threshold; the cooling drivers' t_max rule with 10 / 40 successive failures);
- Main_System.__call__ with adjust_learning_rate, scale_up_actor_update_time and receive_net
  (IHO/main_parallel.py:369-405, 482-559): the updates due, the lr schedule over episodes with the cap at learning
  start, the temporary backup_period = 100, the actor's update cadence, the model saves and the stop rule.

`Schedule.tick` reads BatchedEnv's finished-episode ring where qc_env_tail left it (no host copy); the host reads one
small snapshot per control step, one step late (`Schedule.poll`), as `qc_take_errors` does for action errors. Two
departures from the reference, both fixed parts of the definition: rows are credited to the pacing in the call that
stores them (the reference credits an episode's rows when it ends), and every decision is acted on one tick after
the tick that took it, which keeps the loop free of synchronisation and makes the run deterministic.

    schedule = Schedule.for_driver(physics, batch_size=512)
    trainer = Trainer(env, actor, memory, learner, schedule, save_dir="models")
    env.reset()
    trainer.run()

`python -m deepreinforcementlearningcontrolofquantumcartpoles_amd.train --system iho` builds the objects with the
drivers' argument names and runs it (one GPU).

`Monitor` (csrc/qcart_monitor.hip) is the cooling drivers' receive_net on the device: the table of their best models,
ranked by the mean of the last performances of a BatchedEnv made with `performance_from`. A Trainer given one saves
the outgoing model of a push under its rank, one step late, and evaluates by the performance.
"""
from __future__ import annotations

import ctypes
import os
import tempfile
from typing import Callable, Mapping, Optional

import torch

from . import _lib as L
from . import checkpoint
from . import config as cfg
from .actor import DQNActor

# scale_up_actor_update_time's rungs as (achieved above, actor_update_time at most, new time), in the order the
# drivers test them: IHO/main_parallel.py:532-542 (IQO:438-447 the same), HO:518-527, QO:452-459
_RUNGS = {
    cfg.IHO: ((50., 150., 800.), (20., 50., 150.), (10., 25., 50.), (5., 10., 25.)),
    cfg.IQO: ((50., 150., 800.), (20., 50., 150.), (10., 25., 50.), (5., 10., 25.)),
    cfg.HO: ((80., 150., 1000.), (20., 50., 150.), (10., 25., 50.), (5., 10., 25.)),
    cfg.QO: ((80., 150., 800.), (10., 25., 50.), (5., 10., 25.)),
}
# per driver: (default episodes, lr schedule, init_lr, lr cap at learning start, maximum_trails_before_giveup)
# (arguments.py: IHO:85-86, 46-48; IQO:90-92, 54-56; HO:85-86, 48-50; QO:92-93, 58-60; the cap: main_parallel.py
# IHO:548-549, IQO:452-453, QO:464-465; HO has neither the cap nor the temporary period: HO:469, 529-536)
_DRIVER = {
    cfg.IHO: (20000, ((6000, 8e-5), (11000, 2e-5), (15000, 4e-6), (17000, 8e-7), (19000, 2e-7), (21000, 0.)), 4e-4, 4e-4, 50000),
    cfg.IQO: (20000, ((4000, 8e-5), (9000, 2e-5), (14000, 4e-6), (16000, 8e-7), (18000, 2e-7), (20000, 0.)), 2e-3, 4e-4, 40000),
    cfg.HO: (9000, ((1000, 4e-5), (3000, 8e-6), (5000, 2e-6), (6500, 4e-7), (8000, 1e-7), (9000, 0.)), 4e-4, float("inf"), 20000),
    cfg.QO: (11000, ((1000, 4e-4), (2000, 8e-5), (5000, 2e-5), (7000, 4e-6), (8500, 8e-7), (10000, 2e-7), (11000, 0.)), 1e-3, 1e-3, 20000),
}
# "learning in progress": the cartpoles' (start, fall) of the averaged episode time (IHO/RL.py:525, 532;
# IQO/RL.py:523, 530); the cooling drivers' successive failures (HO/RL.py:532, QO/RL.py:518)
_THRESHOLDS = {cfg.IHO: (20., 5.), cfg.IQO: (12., 4.)}
_FAIL_LIMIT = {cfg.HO: 10, cfg.QO: 40}

_PARAM_NAMES = ("rule", "train", "start_time", "fall_time", "t_full", "first_interval_time", "fail_limit", "batch_size",
                "n_times_per_sample", "max_updates_per_tick", "min_rows", "num_episodes", "give_up_episodes", "lr_init",
                "lr_cap", "lr_schedule", "backup_period", "warm_backup_period", "save_interval", "actor_update_time",
                "rungs")


class Schedule(L.DeviceHandle):
    """The device training schedule (qc_sched, include/qcart.h). Keyword arguments are qc_sched_params' fields, with
    `lr_schedule` a sequence of up to 8 (episode, lr) pairs and `rungs` of up to 4 (achieved above,
    actor_update_time at most, new time) triples; `for_driver` fills a driver's. A refused value raises QCartError
    with the library's text."""

    _prefix = "qc_sched"
    DEFAULTS = dict(rule=L.QC_SCHED_CARTPOLE, train=1, start_time=20., fall_time=5., t_full=0., first_interval_time=0.,
                    fail_limit=10, batch_size=512, n_times_per_sample=8., max_updates_per_tick=8, min_rows=0,
                    num_episodes=20000, give_up_episodes=50000, lr_init=4e-4, lr_cap=4e-4, lr_schedule=(),
                    backup_period=300, warm_backup_period=100, save_interval=200, actor_update_time=10.,
                    rungs=_RUNGS[cfg.IHO])

    def __init__(self, device: int | str | torch.device = 0, **params):
        unknown = set(params) - set(_PARAM_NAMES)
        if unknown:
            raise ValueError(f"Schedule: unknown parameter(s) {sorted(unknown)}")
        if not torch.cuda.is_available():
            raise RuntimeError("libqcart needs a HIP device (no CPU fallback)")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        p = dict(self.DEFAULTS, **params)
        p["lr_schedule"] = tuple((int(e), float(v)) for e, v in p["lr_schedule"])
        p["rungs"] = tuple(tuple(float(v) for v in r) for r in p["rungs"])
        if any(len(r) != 3 for r in p["rungs"]):
            raise ValueError("Schedule: a rung is (achieved above, actor_update_time at most, new time)")
        self.params = p
        c = L.QcSchedParams()
        for k in _PARAM_NAMES:
            if k not in ("lr_schedule", "rungs"):
                setattr(c, k, type(self.DEFAULTS[k])(p[k]))
        # longer tables than the struct holds are passed on as their length: the library refuses them with its text
        c.n_lr_steps, c.n_rungs = len(p["lr_schedule"]), len(p["rungs"])
        for i, (e, v) in enumerate(p["lr_schedule"][:L.QC_SCHED_MAX_LR_STEPS]):
            c.lr_episode[i], c.lr_value[i] = e, v
        for i, r in enumerate(p["rungs"][:L.QC_SCHED_MAX_RUNGS]):
            c.rung_achieved[i], c.rung_below[i], c.rung_time[i] = r
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.init()
            L.check_sched(L.lib().qc_sched_create(ctypes.byref(c), self.device.index, ctypes.byref(h)))
        self._h = h
        self.ticks = 0        # ticks enqueued: tick() returns the index of the one it ran

    @classmethod
    def for_driver(cls, physics: cfg.Physics, batch_size: int = 512, n_times_per_sample: float = 8.,
                   train_episodes_multiplicative: float = 1., init_lr: Optional[float] = None,
                   backup_period: int = 300, save_interval: int = 200, t_max: float = 100.,
                   max_updates_per_tick: int = 8, min_rows: Optional[int] = None, train: bool = True,
                   device: int | str | torch.device = 0, **overrides) -> "Schedule":
        """The schedule of the driver of `physics.family` with the drivers' argument names: the thresholds 20 / 5
        (IHO), 12 / 4 (IQO), 10 (HO) and 40 (QO) successive failures, num_episodes, lr_schedule and save_interval
        scaled by train_episodes_multiplicative (arguments.py:85-87), the lr cap, the rungs, and for the cooling
        drivers t_full = t_max - 0.01 dt (BatchedEnv's t_trunc) and HO's zero-sample rule at one control interval.
        HO has no lr cap and no temporary target period (warm_backup_period = backup_period), and steps its lr while
        last_achieved_time == t_max (HO/main_parallel.py:531) where this schedule, like the other three drivers, asks for
        learning in progress. The cooling drivers save their best models by performance: a Trainer given a
        `Monitor` ignores this schedule's save flag; without one every driver saves by `save_interval`.
        min_rows defaults to batch_size (TrainDQN returns None below it, RL.py:161)."""
        fam = physics.family
        episodes, sched, lr0, cap, give_up = _DRIVER[fam]
        mult = float(train_episodes_multiplicative)
        kw = dict(train=int(bool(train)), batch_size=int(batch_size), n_times_per_sample=float(n_times_per_sample),
                  max_updates_per_tick=int(max_updates_per_tick),
                  min_rows=int(batch_size if min_rows is None else min_rows),
                  num_episodes=round(episodes * mult), give_up_episodes=give_up,
                  lr_init=float(lr0 if init_lr is None else init_lr), lr_cap=cap,
                  lr_schedule=tuple((round(e * mult), v) for e, v in sched),
                  backup_period=int(backup_period), save_interval=max(1, round(save_interval * mult)),
                  rungs=_RUNGS[fam])
        if fam in _THRESHOLDS:
            kw.update(rule=L.QC_SCHED_CARTPOLE, start_time=_THRESHOLDS[fam][0], fall_time=_THRESHOLDS[fam][1])
        else:
            if fam == cfg.HO:
                kw["warm_backup_period"] = int(backup_period)
            kw.update(rule=L.QC_SCHED_COOLING, start_time=0., fall_time=0., fail_limit=_FAIL_LIMIT[fam],
                      t_full=float(t_max) - 0.01 * physics.dt,
                      # HO/main_parallel.py:242: no row at the first control step; QO decides at i = 0 (QO:208)
                      first_interval_time=physics.control_interval * physics.dt if fam == cfg.HO else 0.)
        kw.update(overrides)
        return cls(device=device, **kw)

    # ------------------------------------------------------------------ ticks
    def tick_raw(self, fin: torch.Tensor, fin_cap: int, fin_n: torch.Tensor, valid: Optional[torch.Tensor]) -> int:
        """qc_sched_tick on a ring [2, fin_cap + 1] float64, its int64 count and a uint8 / bool mask (or None);
        asynchronous. Returns the tick's index."""
        if fin.dtype != torch.float64 or tuple(fin.shape) != (2, fin_cap + 1) or not fin.is_contiguous():
            raise ValueError("fin must be a contiguous float64 [2, fin_cap + 1] tensor")
        if fin_n.dtype != torch.int64 or fin_n.numel() != 1:
            raise ValueError("fin_n must be one int64")
        if fin.device != self.device or fin_n.device != self.device:
            raise ValueError(f"the ring must live on {self.device}")
        B = 0
        if valid is not None:
            if valid.dtype == torch.bool:
                valid = valid.view(torch.uint8)
            if valid.dtype != torch.uint8 or valid.dim() != 1 or not valid.is_contiguous() or valid.device != self.device:
                raise ValueError(f"valid must be a contiguous 1-d bool / uint8 tensor on {self.device}")
            B = valid.numel()
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_sched_tick(self._h, vp(fin.data_ptr()), int(fin_cap), vp(fin_n.data_ptr()),
                                              vp(valid.data_ptr()) if B else None, B))
        self.ticks += 1
        return self.ticks - 1

    def tick(self, env, valid: Optional[torch.Tensor]) -> int:
        """One tick on `env`'s finished-episode ring (BatchedEnv.finished_ring) and this call's `valid` mask of
        stored rows. Asynchronous: one launch, one snapshot copy, one event. Returns the tick's index."""
        fin, cap, n = env.finished_ring()
        return self.tick_raw(fin, cap, n, valid)

    def seek(self, env):
        """Start the walk at the ring's present end: episodes `env` finished before are not this schedule's
        (qc_sched_seek; asynchronous)."""
        _, _, n = env.finished_ring()
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_sched_seek(self._h, ctypes.c_void_p(n.data_ptr())))

    def poll(self, tick: int) -> dict:
        """The snapshot of `tick` (one of the last two) as a dict of qc_sched_snapshot's fields; waits for that tick's
        event only."""
        s = L.QcSchedSnapshot()
        self._check(L.lib().qc_sched_poll(self._h, int(tick), ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in L.QcSchedSnapshot._fields_}

    def stats(self) -> dict:
        """The last tick's snapshot (waits for it). Raises QCartError if the ring was overrun since the schedule was
        made: more than fin_cap episodes finished between two ticks, and the oldest were not counted."""
        if self.ticks == 0:
            raise ValueError("Schedule.stats: no tick yet")
        s = self.poll(self.ticks - 1)
        if s["error"] & L.QC_SCHED_ERR_OVERRUN:
            raise L.QCartError(-1, "Schedule: the finished-episode ring was overrun between two ticks (more than "
                                   "fin_cap new episodes); the walk went on from the oldest entry still present")
        return s

    # ------------------------------------------------------------------ checkpoint
    def _made_for(self) -> dict:
        return {k: self.params[k] for k in _PARAM_NAMES}

    def state_dict(self) -> dict:
        """The schedule's whole state as CPU values (checkpoint.save): the handle's blob (qc_sched_state_export) with
        the echo of the params it was made for. Synchronises the schedule's stream."""
        with torch.cuda.device(self.device):
            blob = self._export_state()
        return {"kind": self._prefix, **self._made_for(), "blob": blob}

    def check_state_dict(self, state: dict):
        """Raise ValueError naming the first param of `state` this schedule was not made with; changes nothing."""
        if isinstance(state, dict):   # a file holds lists where the params hold tuples
            state = {k: (tuple(tuple(x) for x in v) if k in ("lr_schedule", "rungs") else v) for k, v in state.items()}
        L.check_echo(type(self).__name__, state, {"kind": self._prefix, **self._made_for()}, ("blob",))

    def load_state_dict(self, state: dict):
        """Continue from a `state_dict()`: the next tick gives bit for bit what the saved schedule's would have. The
        ticks before stay with the schedule that ran them: `poll` serves only ticks run after the load."""
        self.check_state_dict(state)
        with torch.cuda.device(self.device):
            self._import_state(state["blob"])
        self.ticks = int.from_bytes(bytes(state["blob"][-8:].tolist()), "little", signed=True)   # the payload's tail


_MONITOR_NAMES = ("train", "window", "min_count", "min_episodes", "num_of_saves", "initial")
# receive_net's rule per cooling driver: (performances averaged, needed since the last net) (QO/main_parallel.py:311-312,
# HO/main_parallel.py:373-374)
_MONITOR_RULE = {cfg.QO: (8, 8), cfg.HO: (10, 9)}


def performance_from(physics: cfg.Physics, input: str = "xp") -> float:
    """The episode time past which the cooling drivers count a control step into the episode's performance: the
    reference's literals, t > 30 (HO 'xp' and 'wavefunction', HO/main_parallel.py:247), t > 30 - 0.01 dt (HO
    'measurements', :274) and t > 50 - 0.01 dt (QO/main_parallel.py:221). BatchedEnv's performance_from."""
    if physics.family == cfg.HO:
        return 30. - 0.01 * physics.dt if input == "measurements" else 30.
    if physics.family == cfg.QO:
        return 50. - 0.01 * physics.dt
    raise ValueError("the cartpole drivers (IHO, IQO) have no per-episode performance")


class Monitor(L.DeviceHandle):
    """The cooling drivers' model ranking on the device (qc_monitor, include/qcart.h): worker_manager.receive_net's
    table of the num_of_saves best means of the last `window` episode performances, fed from the performance ring of
    a BatchedEnv made with performance_from. Keyword arguments are qc_monitor_params' fields; `for_driver` fills a
    driver's. A refused value raises QCartError with the library's text."""

    _prefix = "qc_monitor"
    DEFAULTS = dict(train=1, window=8, min_count=8, min_episodes=50, num_of_saves=20, initial=6.)

    def __init__(self, device: int | str | torch.device = 0, **params):
        unknown = set(params) - set(_MONITOR_NAMES)
        if unknown:
            raise ValueError(f"Monitor: unknown parameter(s) {sorted(unknown)}")
        if not torch.cuda.is_available():
            raise RuntimeError("libqcart needs a HIP device (no CPU fallback)")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        p = dict(self.DEFAULTS, **params)
        self.params = {k: type(self.DEFAULTS[k])(p[k]) for k in _MONITOR_NAMES}
        c = L.QcMonitorParams(**self.params)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.init()
            L.check_monitor(L.lib().qc_monitor_create(ctypes.byref(c), self.device.index, ctypes.byref(h)))
        self._h = h
        self.calls = 0        # receives enqueued: receive() returns the index of the one it ran

    @classmethod
    def for_driver(cls, physics: cfg.Physics, num_of_saves: int = 20, energy_cutoff: float = 12.,
                   phonon_cutoff: float = 20., train: bool = True, device: int | str | torch.device = 0,
                   **overrides) -> "Monitor":
        """The ranking of the cooling driver of `physics.family`: QO the last 8 performances with at least 8 new
        ones, the table starting at energy_cutoff / 2 (QO/main_parallel.py:283, 311-312); HO the last 10 with at
        least 9 new ones, starting at phonon_cutoff (HO/main_parallel.py:348, 373-374); more than 50 episodes since
        the last record. The cartpole drivers save by save_interval and have none."""
        if physics.family not in _MONITOR_RULE:
            raise ValueError("Monitor.for_driver: the cooling drivers (HO, QO) rank their models by performance; the "
                             "cartpole drivers (IHO, IQO) save by save_interval")
        window, min_count = _MONITOR_RULE[physics.family]
        kw = dict(train=int(bool(train)), window=window, min_count=min_count, min_episodes=50,
                  num_of_saves=int(num_of_saves),
                  initial=float(energy_cutoff) / 2. if physics.family == cfg.QO else float(phonon_cutoff))
        kw.update(overrides)
        return cls(device=device, **kw)

    # ------------------------------------------------------------------ receives
    def receive_raw(self, perf: torch.Tensor, fin_cap: int, fin_n: torch.Tensor) -> int:
        """qc_monitor_receive on a performance ring [fin_cap + 1] float64 and its int64 count; asynchronous. Returns
        the receive's index."""
        if perf.dtype != torch.float64 or tuple(perf.shape) != (fin_cap + 1,) or not perf.is_contiguous():
            raise ValueError("perf must be a contiguous float64 [fin_cap + 1] tensor")
        if fin_n.dtype != torch.int64 or fin_n.numel() != 1:
            raise ValueError("fin_n must be one int64")
        if perf.device != self.device or fin_n.device != self.device:
            raise ValueError(f"the ring must live on {self.device}")
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_monitor_receive(self._h, vp(perf.data_ptr()), int(fin_cap), vp(fin_n.data_ptr())))
        self.calls += 1
        return self.calls - 1

    def receive(self, env) -> int:
        """One receive on `env`'s performance ring (BatchedEnv.performance_ring). Asynchronous: one launch, one
        snapshot copy, one event. Returns the receive's index."""
        perf, cap, n = env.performance_ring()
        return self.receive_raw(perf, cap, n)

    def seek(self, env):
        """Start at the ring's present end: episodes `env` finished before are not this monitor's (qc_monitor_seek;
        asynchronous)."""
        _, _, n = env.performance_ring()
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_monitor_seek(self._h, ctypes.c_void_p(n.data_ptr())))

    def poll(self, call: int) -> dict:
        """The snapshot of receive `call` (one of the last two) as a dict of qc_monitor_snapshot's fields; waits for
        that receive's event only."""
        s = L.QcMonitorSnapshot()
        self._check(L.lib().qc_monitor_poll(self._h, int(call), ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in L.QcMonitorSnapshot._fields_}

    def stats(self) -> dict:
        """The last receive's snapshot (waits for it). Raises QCartError if a train = 0 monitor's ring was overrun:
        more than fin_cap episodes finished between two receives, and the oldest were not counted."""
        if self.calls == 0:
            raise ValueError("Monitor.stats: no receive yet")
        s = self.poll(self.calls - 1)
        if s["error"] & L.QC_MONITOR_ERR_OVERRUN:
            raise L.QCartError(-1, "Monitor: the performance ring was overrun between two receives (more than "
                                   "fin_cap new episodes); the walk went on from the oldest entry still present")
        return s

    def table(self):
        """(good, filled): the table's num_of_saves values in increasing order and which of them hold a model, as
        lists. Synchronises the monitor's stream."""
        n = self.params["num_of_saves"]
        good, filled = (ctypes.c_double * n)(), (ctypes.c_int32 * n)()
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_monitor_table(self._h, good, filled))
        return list(good), list(filled)

    # ------------------------------------------------------------------ checkpoint
    def _made_for(self) -> dict:
        return dict(self.params)

    def state_dict(self) -> dict:
        """The monitor's whole state as CPU values: the handle's blob (qc_monitor_state_export) with the echo of the
        params it was made for. Synchronises the monitor's stream."""
        with torch.cuda.device(self.device):
            blob = self._export_state()
        return {"kind": self._prefix, **self._made_for(), "blob": blob}

    def check_state_dict(self, state: dict):
        """Raise ValueError naming the first param of `state` this monitor was not made with; changes nothing."""
        L.check_echo(type(self).__name__, state, {"kind": self._prefix, **self._made_for()}, ("blob",))

    def load_state_dict(self, state: dict):
        """Continue from a `state_dict()`: the next receive gives bit for bit what the saved monitor's would have.
        The receives before stay with the monitor that ran them: `poll` serves only receives run after the load."""
        self.check_state_dict(state)
        with torch.cuda.device(self.device):
            self._import_state(state["blob"])
        self.calls = int.from_bytes(bytes(state["blob"][-8:].tolist()), "little", signed=True)   # the payload's tail


class Trainer:
    """The drivers' training loop on the device objects: `step()` is one control step,

    1. `actor.act` on the env's observation with the epsilon schedule `eps(steps_done)`; steps_done += env.B;
    2. `env.step`;
    3. the transition into the replay (`store` for the 'measurements' input, else `store_xp` with the terminal
       observation where the reset mode reports one);
    4. `schedule.tick`;
    5. the snapshot of the previous tick, acted on in this order: set_lr if the lr changed, set_backup_period if
       the period changed, n_updates x learner.step(memory), push if flagged, a model save if flagged; `stop` is
       returned.

    The constructor applies the schedule's initial lr and its warm backup period to the learner (Main_System.__init__,
    IHO/main_parallel.py:480-481). Saves go to `save_dir` as 1.pth (newest) .. num_of_saves.pth like receive_net
    (:391-397), each written to a temporary name and renamed.

    With `monitor` (the cooling drivers, QO/main_parallel.py:283-329) the saves are the monitor's table instead: a
    push calls `monitor.receive(env)` and keeps the outgoing model, the one the actor was acting on; the next step()
    polls that receive and, if it set a record of rank r, moves r+1.pth .. up by one and writes the kept model as
    {r+1}.pth, so 1.pth is the best model. The schedule's save flag is ignored, and evaluate() reports the episodes'
    performance."""

    def __init__(self, env, actor, memory, learner, schedule: Schedule, save_dir: Optional[str] = None,
                 eps: Callable[[float], float] = DQNActor.eps_threshold, num_of_saves: int = 20,
                 monitor: Optional[Monitor] = None):
        self.env, self.actor, self.memory, self.learner, self.schedule = env, actor, memory, learner, schedule
        self.save_dir, self.eps, self.num_of_saves = save_dir, eps, int(num_of_saves)
        if self.num_of_saves < 1:
            raise ValueError("num_of_saves must be >= 1")
        self.monitor = monitor
        if monitor is not None:
            if int(monitor.params["num_of_saves"]) != self.num_of_saves:
                raise ValueError(f"Trainer: num_of_saves is {self.num_of_saves}, the monitor's "
                                 f"{monitor.params['num_of_saves']}: the files are the monitor's table")
            self._model = self._clone_model()     # the model the actor is acting on (receive_net's `net`)
            self._stash: Optional[dict] = None    # the outgoing model of the last push, until its receive is polled
            self._recv = -1                       # that receive's index (-1: none is pending)
            self._recv_carried: Optional[dict] = None   # a checkpoint's snapshot of its pending receive
            self.n_filled = 0                     # table entries that hold a model = files 1.pth .. n_filled.pth
        self.meas = env.input == "measurements"
        self.steps_done = 0
        self.tick_index = -1          # the last tick run
        self.acted: Optional[dict] = None     # the last snapshot acted on
        self._carried: Optional[dict] = None  # a checkpoint's snapshot of its last tick, acted on by the next step
        self.saves: list = []         # file names in save_dir, newest first
        self.losses: list = []        # the unweighted losses of the last step's updates (device tensors)
        p = schedule.params
        self.lr = float(p["lr_init"])
        self.backup_period = int(p["warm_backup_period"] if p["train"] else p["backup_period"])
        learner.set_lr(self.lr)
        learner.set_backup_period(self.backup_period)

    def objects(self) -> dict:
        """The five stateful objects under the names checkpoint.save / load take them by (six with a monitor)."""
        out = {"env": self.env, "actor": self.actor, "memory": self.memory, "learner": self.learner,
               "schedule": self.schedule}
        if self.monitor is not None:
            out["monitor"] = self.monitor
        return out

    # ------------------------------------------------------------------ one control step
    def _store(self, a, obs, reward, done, info):
        if self.meas:
            self.memory.store(info["rows"], info["valid"])
        else:
            nxt = torch.where(done[:, None], info["terminal_obs"], obs) if "terminal_obs" in info else obs
            self.memory.store_xp(info["last_obs"], nxt, a, reward, info["valid"])

    def step(self) -> bool:
        env = self.env
        a = self.actor.act(env.obs, eps=self.eps(self.steps_done))
        self.steps_done += env.B
        obs, reward, done, info = env.step(a)
        self._store(a, obs, reward, done, info)
        self.last = (a, reward, done, info)
        prev = self.tick_index
        self.tick_index = self.schedule.tick(env, info["valid"])
        if self._carried is not None:
            snap, self._carried = self._carried, None
        elif prev >= 0:
            snap = self.schedule.poll(prev)
        else:
            self.losses = []
            return False
        if self.monitor is not None:
            self._act_on_receive()
        return self._obey(snap)

    # ------------------------------------------------------------------ ranked saves (a monitor is attached)
    def _clone_model(self) -> dict:
        return dict(self.learner.state_dict())    # (device copies already: the learner's own tensors stay its own)

    def _act_on_receive(self):
        """The receive of the last push, one step late: a record writes the outgoing model of that push as
        {rank + 1}.pth, the files from there on moving up by one (receive_net, QO/main_parallel.py:313-322)."""
        if self._recv_carried is not None:
            s, self._recv_carried = self._recv_carried, None
        elif self._recv >= 0:
            s = self.monitor.poll(self._recv)
        else:
            return
        self._recv = -1
        if s["rank"] >= 0:
            if self.save_dir is not None:
                self._save_ranked(int(s["rank"]))
            self.n_filled = int(s["n_filled"])
            self.saves = [f"{i}.pth" for i in range(1, self.n_filled + 1)]
        self._stash = None

    def _save_ranked(self, rank: int):
        os.makedirs(self.save_dir, exist_ok=True)
        model = {k: v.cpu() for k, v in self._stash.items()}
        fd, tmp = tempfile.mkstemp(prefix="model.", suffix=".tmp", dir=self.save_dir)
        try:
            with os.fdopen(fd, "wb") as f:
                torch.save(model, f)
            # files rank + 1 .. n_filled move up by one; the one beyond num_of_saves falls out
            for i in range(min(self.n_filled, self.num_of_saves - 1), rank, -1):
                os.replace(os.path.join(self.save_dir, f"{i}.pth"), os.path.join(self.save_dir, f"{i + 1}.pth"))
            os.replace(tmp, os.path.join(self.save_dir, f"{rank + 1}.pth"))
        except BaseException:
            try:
                os.unlink(tmp)
            except OSError:
                pass
            raise

    def _obey(self, s: dict) -> bool:
        if s["lr"] != self.lr:
            self.lr = s["lr"]
            self.learner.set_lr(self.lr)
        if s["backup_period"] != self.backup_period:
            self.backup_period = int(s["backup_period"])
            self.learner.set_backup_period(self.backup_period)
        self.losses = [self.learner.step(self.memory) for _ in range(s["n_updates"])]
        if s["push"]:
            if self.monitor is not None:
                # the outgoing net produced the performances seen so far: it is what a record saves
                self._recv = self.monitor.receive(self.env)
                self._stash = self._model
            self.learner.push(self.actor)
            if self.monitor is not None:
                self._model = self._clone_model()
        if s["save"] and self.save_dir is not None and self.monitor is None:   # (a monitor saves by performance)
            self._save_model()
        self.acted = s
        return bool(s["stop"])

    def _save_model(self):
        os.makedirs(self.save_dir, exist_ok=True)
        model = {k: v.cpu() for k, v in self.learner.state_dict().items()}
        fd, tmp = tempfile.mkstemp(prefix="model.", suffix=".tmp", dir=self.save_dir)
        try:
            with os.fdopen(fd, "wb") as f:
                torch.save(model, f)
            # the ring moves up by one, the oldest falls out (save_models[-num_of_saves:], main_parallel.py:394)
            for i in range(min(len(self.saves), self.num_of_saves - 1), 0, -1):
                os.replace(os.path.join(self.save_dir, f"{i}.pth"), os.path.join(self.save_dir, f"{i + 1}.pth"))
            os.replace(tmp, os.path.join(self.save_dir, "1.pth"))
        except BaseException:
            try:
                os.unlink(tmp)
            except OSError:
                pass
            raise
        self.saves = [f"{i}.pth" for i in range(1, min(len(self.saves) + 1, self.num_of_saves) + 1)]

    def run(self, max_steps: Optional[int] = None, report_every: int = 0) -> int:
        """step() until the schedule says stop (or max_steps); returns the steps run. report_every = N prints one
        line per N steps from the snapshot last acted on."""
        n = 0
        while max_steps is None or n < max_steps:
            stop = self.step()
            n += 1
            if report_every and n % report_every == 0 and self.acted is not None:
                s = self.acted
                print(f"tick {s['tick']}\tepisode {s['episode']}\tt = {s['last_achieved']:.2f}\tlr {s['lr']:.2g}\t"
                      f"learning {s['learning']}\tupdates due {s['pending']:.1f}", flush=True)
            if stop:
                break
        return n

    # ------------------------------------------------------------------ checkpoint
    def state_dict(self) -> dict:
        """The Trainer's own state (the five objects keep theirs): steps_done, the tick index, the last snapshot
        acted on, the last tick's snapshot (not yet acted on; waits for it), the lr and period in force and the save
        ring's file names. With `objects()` it goes through checkpoint.save as `extra`."""
        pending = self._carried
        if pending is None and self.tick_index >= 0:
            pending = self.schedule.poll(self.tick_index)
        out = {"kind": "Trainer", "steps_done": int(self.steps_done), "tick_index": int(self.tick_index),
               "acted": self.acted, "pending": pending, "lr": float(self.lr),
               "backup_period": int(self.backup_period), "saves": list(self.saves)}
        if self.monitor is not None:
            # the receive still to be acted on (waits for it) and the two models a resumed run needs for it
            recv = self._recv_carried
            if recv is None and self._recv >= 0:
                recv = self.monitor.poll(self._recv)
            cpu = lambda m: None if m is None else {k: v.cpu() for k, v in m.items()}   # noqa: E731
            out.update(monitor_pending=recv, monitor_stash=cpu(self._stash), monitor_model=cpu(self._model),
                       n_filled=int(self.n_filled))
        return out

    def load_state_dict(self, state: dict):
        """After checkpoint.load of `objects()`: continue the saved run bit for bit. Re-applies the period in force to
        the learner."""
        L.check_echo("Trainer", state, {"kind": "Trainer"},
                     ("steps_done", "tick_index", "acted", "pending", "lr", "backup_period", "saves"))
        if int(state["tick_index"]) != self.schedule.ticks - 1:
            raise ValueError(f"Trainer: the state's last tick is {state['tick_index']}, the schedule's "
                             f"{self.schedule.ticks - 1} (load the schedule first)")
        self.steps_done, self.tick_index = int(state["steps_done"]), int(state["tick_index"])
        self.acted, self._carried = state["acted"], state["pending"]
        self.lr, self.backup_period = float(state["lr"]), int(state["backup_period"])
        self.saves = list(state["saves"])
        self.learner.set_backup_period(self.backup_period)
        if self.monitor is not None:
            L.check_echo("Trainer", state, {}, ("monitor_pending", "monitor_stash", "monitor_model", "n_filled"))
            dev = lambda m: None if m is None else {k: v.to(self.monitor.device) for k, v in m.items()}   # noqa: E731
            self._recv, self._recv_carried = -1, state["monitor_pending"]
            self._stash, self._model = dev(state["monitor_stash"]), dev(state["monitor_model"])
            self.n_filled = int(state["n_filled"])

    def save_checkpoint(self, path):
        checkpoint.save(path, self.objects(), extra=self.state_dict())

    def load_checkpoint(self, path):
        self.load_state_dict(checkpoint.load(path, self.objects()))

    # ------------------------------------------------------------------ --test
    def evaluate(self, params: Optional[Mapping[str, torch.Tensor]], episodes: int, path: Optional[str] = None,
                 max_steps: Optional[int] = None, density=None, wigner=None,
                 controller: Optional[tuple] = None, ensemble=None, rho_every: int = 0, levels=None):
        """The drivers' --test mode (IHO/main_parallel.py:367-377, 442-445): `params` (a state_dict; None: the
        actor's current weights) act greedily without parameter noise (eps = 0, noisy = False: net.eval(),
        layers.py:40) under a schedule made as this one with train = 0, until at least `episodes` episodes have
        finished. Returns (mean, sem, n) of the episode times of all n episodes finished by then and, given `path`,
        writes the reference's '{} +- {}' line. Nothing is stored or learned; the env goes on from where it is. With a
        monitor attached the statistic is the cooling drivers': (mean, sem, n) of the episodes' performance.
        `density` (a spatial.SpatialView for the env's physics): every control step appends the ensemble mean
        position-space density of the envs that were live at that step (info['valid']) to `self.density_trace`, a
        list of device [X] tensors that starts empty with each call; nothing in the loop waits for them and the
        returned tuple is the same. `wigner` (a wigner.WignerView for the env's physics) does the same with the
        ensemble mean Wigner function, [X, P] tensors in `self.wigner_trace`. `ensemble` (an ensemble.EnsembleView for
        the env's physics) takes the density matrix rho of the live envs once per control step and appends its purity
        (a 0-d tensor) to `self.purity_trace` and its populations ([N]) to `self.population_trace`; with
        rho_every = k > 0 the full rho of the control steps 0, k, 2 k, .. goes to `self.rho_trace` and their indices to
        `self.rho_steps` (a full rho per step at 521 points over an evaluation is gigabytes: it is opt-in).
        `levels` (a levels.LevelView for the env's physics): every control step appends the mean energy-level
        populations [K] of the envs that were live at that step to `self.level_trace`, in the same manner.
        `controller` = (strategy, con_parameter): the drivers' baseline runs (--control_strategy / --con_parameter,
        QO/main_parallel.py:166-176; --LQG, IHO/main_parallel.py:194-206): the actions come from
        env.analytic_actions(strategy, con_parameter) and the actor is not touched; `params` must be None."""
        if controller is not None:
            if params is not None:
                raise ValueError("Trainer.evaluate: params and controller exclude each other (a baseline has no net)")
            strategy, con_parameter = controller
            act = lambda env: env.analytic_actions(strategy, float(con_parameter))   # noqa: E731
        else:
            if params is not None:
                self.actor.load(params)
            act = lambda env: self.actor.act(env.obs, eps=0.0, noisy=False)   # noqa: E731
        self.density_trace: list = []
        self.wigner_trace: list = []
        self.purity_trace: list = []
        self.population_trace: list = []
        self.rho_trace: list = []
        self.rho_steps: list = []
        self.level_trace: list = []
        if rho_every < 0:
            raise ValueError("Trainer.evaluate: rho_every must be >= 0")
        if self.monitor is not None:
            return self._evaluate_performance(episodes, path, max_steps, density, wigner, act, ensemble, rho_every,
                                              levels)
        sched = Schedule(device=self.schedule.device, **dict(self.schedule.params, train=0))
        env = self.env
        try:
            sched.seek(env)          # the ring's earlier episodes are not this evaluation's
            tick, n_steps = -1, 0
            while max_steps is None or n_steps < max_steps:
                info = env.step(act(env))[3]
                if density is not None:
                    self.density_trace.append(env.probability(density, mean=True, mask=info["valid"])[0])
                if wigner is not None:
                    self.wigner_trace.append(env.wigner(wigner, mean=True, mask=info["valid"])[0])
                if ensemble is not None:
                    self._record_rho(ensemble, rho_every, info["valid"], n_steps)
                if levels is not None:
                    self.level_trace.append(env.level_populations(levels, mean=True, mask=info["valid"])[0])
                n_steps += 1
                prev, tick = tick, sched.tick(env, None)
                if prev >= 0 and sched.poll(prev)["n"] >= episodes:
                    break
            s = sched.stats()
        finally:
            sched.close()
        if path is not None:
            with open(path, "w") as f:
                f.write("{} +- {}\n".format(s["mean"], s["sem"]))
        return s["mean"], s["sem"], s["n"]

    def open_loop(self, me, n_control: int, slot: Optional[int] = None, wigner=None) -> dict:
        """The no-control (fixed-force) curve of this loop: the ensemble density matrix of the env's current states
        (through `me.ensemble`, the master equation's own ensemble.EnsembleView, which `me.close()` closes) evolved
        `n_control` control intervals by the master equation `me` (lindblad.MasterEquation, env.master_equation())
        at one slot (None: the F = 0 slot). Returns per-control-step traces [n_control + 1] (entry 0: the starting
        rho) of 'trace', 'purity', 'x', 'x2', 'h', 'boundary' and, for the Fock families, 'n', as device tensors:
        nothing is waited on, the env and whatever evaluate() returns are untouched. `wigner` (a wigner.WignerView for
        the env's physics) adds 'wigner' [n_control + 1, X, P], the Wigner function of rho at every entry
        (WignerView.wigner_of), and 'negativity' [n_control + 1], its negative volume; the other keys are the same
        tensors with or without it."""
        from .ensemble import EnsembleView
        if isinstance(n_control, bool) or not isinstance(n_control, int) or n_control < 0:
            raise ValueError("Trainer.open_loop: n_control must be an int >= 0")
        env = self.env
        rho = env.density_matrix(me.ensemble)[0]
        names = ("x", "x2", "h") + (("n",) if env.ph.fock else ())
        out: dict = {k: [] for k in ("trace", "purity", "boundary") + names}

        if wigner is not None:
            out["wigner"], out["negativity"] = [], []

        def record():
            if wigner is not None:
                W = wigner.wigner_of(rho)
                out["wigner"].append(W)
                out["negativity"].append(wigner.negative_volume(W))
            out["trace"].append(torch.diagonal(rho).real.sum())
            out["purity"].append(EnsembleView.purity(rho))
            out["boundary"].append(me.boundary_weight(rho))
            for k in names:
                out[k].append(EnsembleView.expectation(rho, me.operator(k)).real)

        record()
        for _ in range(n_control):
            me.evolve(rho, env.ci, slot)
            record()
        return {k: torch.stack(v) for k, v in out.items()}

    def filtered_loop(self, me, n_control: int, *, eta: float, controller: Optional[tuple] = None,
                      M: Optional[int] = None, seed: int = 0, source: str = "states") -> dict:
        """The loop an observer with a detector of efficiency `eta` would run: M density matrices, each conditioned on
        its own sampled measurement record (me.evolve_conditional), under the baseline
        `controller` = (strategy, con_parameter) acting on rho itself (me.analytic_slots; None: the F = 0 slot).
        source = 'states': the pure rho of the env's first M states (M None: all); 'ensemble': M copies (M None: 1) of
        the ensemble density matrix of the env's current states. Control interval k takes the steps
        first_step = k * env.ci of the records' streams. Returns device traces [n_control + 1, M] (entry 0: the start)
        of 'x', 'x2', 'h', 'purity', 'boundary' (Fock also 'n') and 'slots' int32 [n_control, M]. The loop itself
        waits on nothing; the setup may synchronise once (me.set_efficiency where `eta` is not the handle's already,
        the first upload of the controllers' operators). The env and whatever evaluate() and open_loop() return are
        untouched."""
        if isinstance(n_control, bool) or not isinstance(n_control, int) or n_control < 0:
            raise ValueError("Trainer.filtered_loop: n_control must be an int >= 0")
        if source not in ("states", "ensemble"):
            raise ValueError("Trainer.filtered_loop: source must be 'states' or 'ensemble'")
        env = self.env
        if M is not None and (isinstance(M, bool) or not isinstance(M, int) or M < 1
                              or (source == "states" and M > env.B)):
            raise ValueError("Trainer.filtered_loop: M must be an int >= 1" +
                             (f" and <= the env's batch {env.B}" if source == "states" else ""))
        if me.eta != float(eta):                       # (builds and uploads a table: may synchronise)
            me.set_efficiency(eta)
        if controller is None and me.zero_force_slot is None:
            raise ValueError("Trainer.filtered_loop: the forces do not contain 0.0 and no controller is given")
        if source == "states":
            psi = env.psi[:env.B if M is None else M]
            rho = (me.ensemble.scale * psi[:, :, None] * psi.conj()[:, None, :]).contiguous()
        else:
            rho = env.density_matrix(me.ensemble)[0][None].repeat(1 if M is None else M, 1, 1).contiguous()
        count = int(rho.shape[0])
        names = ("x", "x2", "h") + (("n",) if env.ph.fock else ())
        out: dict = {k: [] for k in ("purity", "boundary", "slots") + names}

        def record():
            out["purity"].append((rho.real * rho.real + rho.imag * rho.imag).sum(dim=(-2, -1)))
            out["boundary"].append(me.boundary_weight(rho))
            for k in names:
                out[k].append(me.expectations(rho, me.operator(k)))

        record()
        for k in range(n_control):
            if controller is None:
                slots = torch.full((count,), me.zero_force_slot, dtype=torch.int32, device=rho.device)
            else:
                slots = me.analytic_slots(rho, controller[0], float(controller[1]))
            out["slots"].append(slots)
            me.evolve_conditional(rho, env.ci, slots, seed=seed, first_step=k * env.ci)
            record()
        none = torch.empty((0, count), dtype=torch.int32, device=rho.device)
        return {k: torch.stack(v) if v else none for k, v in out.items()}

    def _record_rho(self, ensemble, rho_every: int, valid, step: int):
        """One control step's entries of evaluate(ensemble=...): asynchronous, nothing waits."""
        rho = self.env.density_matrix(ensemble, mask=valid)[0]
        self.purity_trace.append(ensemble.purity(rho))
        self.population_trace.append(ensemble.populations(rho))
        if rho_every > 0 and step % rho_every == 0:
            self.rho_trace.append(rho)
            self.rho_steps.append(step)

    def _evaluate_performance(self, episodes: int, path: Optional[str], max_steps: Optional[int], density=None,
                              wigner=None, act=None, ensemble=None, rho_every: int = 0, levels=None):
        """evaluate() with a monitor attached: the cooling drivers' --test statistic (QO/main_parallel.py:288-296,
        364-367), mean and sem of the episodes' performance, from a monitor made as the Trainer's with train = 0 that
        starts at the ring's end and receives once per control step; the stop condition counts its n."""
        mon = Monitor(device=self.monitor.device, **dict(self.monitor.params, train=0))
        env = self.env
        if act is None:
            act = lambda env: self.actor.act(env.obs, eps=0.0, noisy=False)   # noqa: E731
        try:
            mon.seek(env)
            call, n_steps = -1, 0
            while max_steps is None or n_steps < max_steps:
                info = env.step(act(env))[3]
                if density is not None:
                    self.density_trace.append(env.probability(density, mean=True, mask=info["valid"])[0])
                if wigner is not None:
                    self.wigner_trace.append(env.wigner(wigner, mean=True, mask=info["valid"])[0])
                if ensemble is not None:
                    self._record_rho(ensemble, rho_every, info["valid"], n_steps)
                if levels is not None:
                    self.level_trace.append(env.level_populations(levels, mean=True, mask=info["valid"])[0])
                n_steps += 1
                prev, call = call, mon.receive(env)
                if prev >= 0 and mon.poll(prev)["n"] >= episodes:
                    break
            s = mon.stats()
        finally:
            mon.close()
        if path is not None:
            with open(path, "w") as f:
                f.write("{} +- {}\n".format(s["mean"], s["sem"]))
        return s["mean"], s["sem"], s["n"]


def main(argv=None):
    """python -m deepreinforcementlearningcontrolofquantumcartpoles_amd.train: the drivers' run on one GPU."""
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--system", choices=("ho", "iho", "qo", "iqo"), default="iho")
    ap.add_argument("--input", choices=("xp", "wavefunction", "measurements"), default="xp")
    ap.add_argument("--batch_size", type=int, default=512)
    ap.add_argument("--n_times_per_sample", type=int, default=8)
    ap.add_argument("--train_episodes_multiplicative", type=float, default=1.)
    ap.add_argument("--init_lr", type=float, default=None)
    ap.add_argument("--save_dir", default="models")
    ap.add_argument("--test", action="store_true")
    ap.add_argument("--load_dir", default=None, help="--test: the folder whose N.pth models are evaluated")
    ap.add_argument("--num_of_test_episodes", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--max_updates_per_tick", type=int, default=8)
    ap.add_argument("--num_of_saves", type=int, default=20)
    ap.add_argument("--test_energy_cutoff", type=float, default=100., help="qo --test: the episodes' energy cutoff")
    ap.add_argument("--checkpoint", metavar="PATH", default=None, help="written when the run ends")
    ap.add_argument("--resume", metavar="PATH", default=None)
    ap.add_argument("--max_steps", type=int, default=None)
    ap.add_argument("--report_every", type=int, default=100)
    ap.add_argument("--density_out", metavar="PATH", default=None,
                    help="--test: x and the ensemble density per control step of the first model evaluated, one .npz")
    ap.add_argument("--wigner_out", metavar="PATH", default=None,
                    help="--test: x, p and the ensemble mean Wigner function per control step of the first model "
                         "evaluated, one .npz")
    ap.add_argument("--rho_out", metavar="PATH", default=None,
                    help="--test: purity and populations of the ensemble density matrix per control step of the first "
                         "model evaluated (with --rho_every K > 0 also rho and rho_steps of every K-th step), one .npz")
    ap.add_argument("--rho_every", type=int, default=0)
    ap.add_argument("--levels_out", metavar="PATH", default=None,
                    help="--test (ho / qo): energies [K] of the lowest --levels levels of the force-free Hamiltonian and "
                         "the ensemble mean populations [T, K] per control step of the first model evaluated, one .npz")
    ap.add_argument("--levels", type=int, default=32, metavar="K")
    ap.add_argument("--open_loop_out", metavar="PATH", default=None,
                    help="--test: the no-control curve of the driver, one .npz: the master equation's traces (trace, "
                         "purity, x, x2, h, boundary; ho / iho also n) of the envs' starting ensemble over "
                         "--open_loop_steps control intervals at zero force, and t")
    ap.add_argument("--open_loop_steps", type=int, default=90, metavar="T")
    ap.add_argument("--open_loop_wigner", action="store_true",
                    help="--open_loop_out: also wigner [T + 1, X, P], the Wigner function of the master equation's rho "
                         "per control interval, negativity [T + 1], its negative volume, and the axes wigner_x, "
                         "wigner_p (the key x there is <x>)")
    ap.add_argument("--filtered_out", metavar="PATH", default=None,
                    help="--test: the loop of an observer with detection efficiency --eta, one .npz: the conditional "
                         "master equation's traces (x, x2, h, purity, boundary; ho / iho also n) [T + 1, M], slots "
                         "[T, M] and t over --open_loop_steps control intervals from the first --filtered_M envs' "
                         "states, under --control_strategy's baseline controller acting on rho (DQN: zero force)")
    ap.add_argument("--eta", type=float, default=None, help="--filtered_out: the detection efficiency in (0, 1]")
    ap.add_argument("--filtered_M", type=int, default=8, metavar="M")
    ap.add_argument("--control_strategy", choices=("DQN", "LQG", "damping", "semiclassical"), default="DQN",
                    help="other than DQN: one evaluation of the analytic baseline controller (ho / iho take LQG only, "
                         "the drivers' --LQG)")
    ap.add_argument("--con_parameter", type=float, default=0.9)
    args = ap.parse_args(argv)
    if args.system in ("ho", "iho") and args.control_strategy not in ("DQN", "LQG"):
        ap.error(f"--control_strategy {args.control_strategy}: the Fock systems take only DQN or LQG")
    if args.open_loop_wigner and not args.open_loop_out:
        ap.error("--open_loop_wigner adds to the file of --open_loop_out, which is not given")
    if args.filtered_out and args.eta is None:
        ap.error("--filtered_out needs --eta")
    if args.levels_out and args.system in ("iho", "iqo"):
        ap.error(f"--levels_out: --system {args.system} has no bound levels (H is not bounded below)")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("train: one GPU only; WORLD_SIZE > 1 is refused (multi-GPU training is not built)")

    from .actor import MeasurementActor, random_direct_dqn, random_dqn_measurement
    from .env import BatchedEnv
    from .learner import DQNLearner, MeasurementLearner
    from .replay import PrioritizedReplay

    fam = {"ho": cfg.HO, "iho": cfg.IHO, "qo": cfg.QO, "iqo": cfg.IQO}[args.system]
    ph = cfg.DEFAULTS[fam]
    B, seed = args.envs, args.seed
    training = not args.test and args.control_strategy == "DQN"
    env_kw, monitor = {}, None
    if fam in (cfg.HO, cfg.QO):
        # the cooling drivers are measured and saved by the episodes' performance (receive_net)
        env_kw["performance_from"] = performance_from(ph, args.input)
        train_cutoff = 12.      # QO/arguments.py: --energy_cutoff
        if fam == cfg.QO:
            # QO/main_parallel.py:206: args.energy_cutoff if args.train else args.test_energy_cutoff; a baseline run
            # is not a training run (QO/arguments.py:99), so it is judged at the test cutoff like --test
            env_kw["energy_cutoff"] = train_cutoff if training else args.test_energy_cutoff
        monitor = Monitor.for_driver(ph, num_of_saves=args.num_of_saves, energy_cutoff=train_cutoff)
    env = BatchedEnv(ph, B, 0, seed=seed, input=args.input, reset="warmup" if fam == cfg.QO else "deferred", **env_kw)
    # the drivers' learner table: fc2's width, the TD target, LaProp's betas
    hidden2 = 512 if fam in (cfg.QO, cfg.IQO) else 256
    target = {cfg.IHO: "alive", cfg.IQO: "alive", cfg.QO: "reward_fail", cfg.HO: "reward"}[fam]
    betas = (0.9, 0.999) if fam == cfg.HO else (0.9, 0.9995)
    schedule = Schedule.for_driver(ph, batch_size=args.batch_size, n_times_per_sample=args.n_times_per_sample,
                                   train_episodes_multiplicative=args.train_episodes_multiplicative,
                                   init_lr=args.init_lr, t_max=env.t_max,
                                   max_updates_per_tick=args.max_updates_per_tick, train=training)
    kw = dict(batch_size=args.batch_size, lr=schedule.params["lr_init"], target=target, betas=betas, device=0,
              seed=seed + 4)
    if fam == cfg.QO:
        kw["failing_reward"] = -env.energy_cutoff * env.reward_multiply
    if args.input == "measurements":
        rec = env.rec
        w = random_dqn_measurement(read_length=rec.read_length, seed=seed + 1, conv_weight_norm=fam == cfg.HO)
        actor = MeasurementActor(w, read_length=rec.read_length, max_batch=B, seed=seed + 2)
        learner = MeasurementLearner(w, rec.read_length, rec.m, **kw)
        row_len, capacity = int(env.rows.shape[1]), 262144
    else:
        Lobs = int(env.obs.shape[1])
        w = random_direct_dqn(data_length=Lobs, seed=seed + 1, hidden2=hidden2)
        actor = DQNActor(w, data_length=Lobs, max_batch=B, seed=seed + 2)
        learner = DQNLearner(w, **kw)
        # the drivers' 7000 x n_con x 100 rows (IHO/main_parallel.py:595) for 'xp'; 65 536 wavefunction rows
        row_len, capacity = 2 * Lobs + 2, (7000 * 18 * 100 if args.input == "xp" else 65536)
    memory = PrioritizedReplay(capacity, row_len, "random", 0.2, device=0, seed=seed + 3)
    trainer = Trainer(env, actor, memory, learner, schedule, save_dir=args.save_dir, num_of_saves=args.num_of_saves,
                      monitor=monitor)
    if args.resume:
        trainer.load_checkpoint(args.resume)
    else:
        env.reset()
    baseline = args.control_strategy != "DQN"
    if args.test or baseline:
        import numpy as np
        n_test = args.num_of_test_episodes or {cfg.IHO: 4000, cfg.IQO: 4000, cfg.HO: 500, cfg.QO: 300}[fam]
        view = wview = eview = lview = None
        if args.density_out:
            from .spatial import SpatialView
            view = SpatialView.for_physics(ph)
        if args.wigner_out:
            from .wigner import WignerView
            wview = WignerView.for_physics(ph)
        if args.rho_out:
            from .ensemble import EnsembleView
            eview = EnsembleView.for_physics(ph)
        if args.levels_out:
            from .levels import LevelView
            lview = LevelView.for_physics(ph, args.levels)
        if args.open_loop_out:
            # before the evaluation moves the envs; it reads their states only
            me = env.master_equation()
            olview, axes = None, {}
            if args.open_loop_wigner:
                from .wigner import WignerView
                olview = WignerView.for_physics(ph)
                axes = dict(wigner_x=olview.x.cpu().numpy(), wigner_p=olview.p.cpu().numpy())
            curve = trainer.open_loop(me, args.open_loop_steps, wigner=olview)
            np.savez(args.open_loop_out, t=np.arange(args.open_loop_steps + 1) * (env.ci * ph.dt),
                     **{k: v.cpu().numpy() for k, v in curve.items()}, **axes)
            me.close()
            if olview is not None:
                olview.close()
        if args.filtered_out:
            # before the evaluation moves the envs; it reads their states only
            me = env.master_equation()
            con = None if args.control_strategy == "DQN" else (args.control_strategy, args.con_parameter)
            curve = trainer.filtered_loop(me, args.open_loop_steps, eta=args.eta, controller=con,
                                          M=min(args.filtered_M, B), seed=seed)
            np.savez(args.filtered_out, t=np.arange(args.open_loop_steps + 1) * (env.ci * ph.dt), eta=args.eta,
                     **{k: v.cpu().numpy() for k, v in curve.items()})
            me.close()

        def write_traces():
            if view is not None:
                np.savez(args.density_out, x=view.x.cpu().numpy(),
                         density=torch.stack(trainer.density_trace).cpu().numpy())
            if wview is not None:
                np.savez(args.wigner_out, x=wview.x.cpu().numpy(), p=wview.p.cpu().numpy(),
                         wigner=torch.stack(trainer.wigner_trace).cpu().numpy())
            if eview is not None:
                out = dict(purity=torch.stack(trainer.purity_trace).cpu().numpy(),
                           populations=torch.stack(trainer.population_trace).cpu().numpy())
                if args.rho_every > 0:
                    out.update(rho=torch.stack(trainer.rho_trace).cpu().numpy(),
                               rho_steps=np.array(trainer.rho_steps, dtype=np.int64))
                np.savez(args.rho_out, **out)
            if lview is not None:
                np.savez(args.levels_out, energies=lview.energies.cpu().numpy(),
                         populations=torch.stack(trainer.level_trace).cpu().numpy())

        if baseline:
            # the reference's file name: 'LQG' (IHO/main_parallel.py:610-612), 'semiclassical', or the strategy with
            # str(con_parameter) (QO/main_parallel.py:534-537)
            if ph.fock or args.control_strategy == "semiclassical":
                name = args.control_strategy
            else:
                name = args.control_strategy + str(args.con_parameter)
            os.makedirs(args.save_dir, exist_ok=True)
            mean, sem, n = trainer.evaluate(None, n_test, path=os.path.join(args.save_dir, name + ".txt"),
                                            max_steps=args.max_steps, density=view, wigner=wview,
                                            controller=(args.control_strategy, args.con_parameter),
                                            ensemble=eview, rho_every=args.rho_every, levels=lview)
            print(f"{name}: {mean} +- {sem} ({n} episodes)", flush=True)
            write_traces()
            return 0
        folder = args.load_dir or args.save_dir
        names = sorted((f for f in os.listdir(folder) if f.endswith(".pth")), key=lambda f: int(f[:-4]))
        for i, name in enumerate(names):
            model = torch.load(os.path.join(folder, name), map_location="cuda", weights_only=True)
            mean, sem, n = trainer.evaluate(model, n_test, path=os.path.join(folder, name[:-4] + ".txt"),
                                            density=view if i == 0 else None, wigner=wview if i == 0 else None,
                                            ensemble=eview if i == 0 else None, rho_every=args.rho_every,
                                            levels=lview if i == 0 else None)
            print(f"{name}: {mean} +- {sem} ({n} episodes)", flush=True)
            if i == 0:
                write_traces()
        return 0
    steps = trainer.run(args.max_steps, report_every=args.report_every)
    s = trainer.schedule.stats()
    print(f"ended after {steps} control steps: episode {s['episode']}, learning {s['learning']}, lr {s['lr']:.2g}",
          flush=True)
    if args.checkpoint:
        trainer.save_checkpoint(args.checkpoint)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
