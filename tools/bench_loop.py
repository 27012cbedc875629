#!/usr/bin/env python3
"""End-to-end actor loop on one GPU (SURVEY §8f rank 1 measured in place): BatchedEnv (IHO N = 512) +
DQNActor (direct_DQN, random-initialised weights of the reference architecture) for K control steps:
act -> step (80 physics steps) -> experience rows stored in the device prioritized replay (the drivers'
capacity 7000 x 18 x 100 = 12.6 M rows, qc_replay_store_xp) -> one sample(512) + batch_update, the
trainer's per-step memory traffic (RL.py:172, :224), with auto-reset of finished episodes.
With --input measurements: BatchedEnv(input='measurements') (the measurement record, qc_record) +
MeasurementActor (DQN_measurement) + the replay storing the reference's 5 915-float rows (capacity
--capacity rows; the drivers' 2.7 M-row memory is 64 GB, the bench default keeps 262 144 rows).
With --input wavefunction: BatchedEnv(input='wavefunction') (float32 hstack(Re, Im) of the kept rows of psi) +
DQNActor at that length (122 / 302 / 322 / 1002 floats for --physics ho / qo / iho / iqo at the drivers' defaults;
fc2 512 wide for the quartic drivers) + the replay storing rows of 2 L + 2 floats (capacity --capacity rows,
default 65 536: the drivers' 12.6 M rows of 2 006 floats would be 100 GB).
Prints one JSON line: RL steps/s (decisions), env-steps/s and the actor's / replay's share of the loop.
With --physics qo --reset warmup the finished envs warm up inside the following calls (BatchedEnv reset='warmup');
--t-max and --init-time set the episode truncation and the reset's free-evolution time.
--checkpoint PATH saves env, actor, memory and learner (checkpoint.save) after the timed loop and reports
checkpoint_save_ms and checkpoint_bytes; --resume PATH loads such a file before the warm-up (checkpoint.load, into
objects built with the same options) and reports checkpoint_load_ms.
--trainer K runs the same objects through train.Trainer.step (the device schedule's tick, its snapshot copy and the
one-tick-late poll on top of act / step / store) with max_updates_per_tick = K and a pacing constant that makes exactly
K updates due each tick; 'xp' input only. The A/B against --learn K is tools/ab_trainer.sh.
usage: python tools/bench_loop.py [--batch B] [--steps K] [--input xp|wavefunction|measurements] [--physics iho|iqo|ho|qo]
       [--reset immediate|deferred|warmup] [--t-max T] [--init-time LO HI] [--checkpoint PATH] [--resume PATH]
       [--learn K | --trainer K]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deepreinforcementlearningcontrolofquantumcartpoles_amd import checkpoint  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd import config as cfg  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd.actor import (  # noqa: E402
    DQNActor, MeasurementActor, random_direct_dqn, random_dqn_measurement)
from deepreinforcementlearningcontrolofquantumcartpoles_amd.env import BatchedEnv  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd.replay import PrioritizedReplay  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)   # ~0.5 s: a fresh box ramps its clock over the first launches
    ap.add_argument("--capacity", type=int, default=0)   # xp: 7000 x 18 x 100 (IHO/arguments.py:80, main_parallel.py:595)
    ap.add_argument("--input", choices=("xp", "wavefunction", "measurements"), default="xp")
    ap.add_argument("--physics", choices=("iho", "iqo", "ho", "qo"), default="iho",
                    help="with --input wavefunction: the driver whose defaults the env runs (the other inputs run "
                         "the metric's IHO N = 512)")
    ap.add_argument("--reset", choices=("immediate", "deferred", "warmup"), default=None,
                    help="BatchedEnv auto-reset mode (deferred: finished envs reset in the next call's launch, no host "
                         "sync; every input of --physics ho / iho / iqo, not qo; the default for 'xp', immediate for "
                         "the other inputs; warmup: --physics qo only, finished envs run their free evolution inside "
                         "the following calls' launches)")
    ap.add_argument("--t-max", type=float, default=None,
                    help="episode truncation time (BatchedEnv t_max; the cooling drivers; default: the env's 100)")
    ap.add_argument("--init-time", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="--physics qo: the reset's free evolution lasts U[LO, HI] time units (default: the driver's "
                         "15 20)")
    ap.add_argument("--marker", action="store_true",
                    help="wrap the timed steps in a roctx range 'timed' (tools/loop_breakdown.py, rocprofv3 --marker-trace)")
    ap.add_argument("--learn", type=int, default=0,
                    help="device learner steps (DQNLearner.step / MeasurementLearner.step: sample(512) -> update -> "
                         "batch_update) plus one weight push into the actor per control step; 0: none (the default)")
    ap.add_argument("--trainer", type=int, default=0, metavar="K",
                    help="run the loop through train.Trainer.step with exactly K updates due per tick (input xp)")
    ap.add_argument("--monitor", action="store_true",
                    help="--trainer K --physics ho: the env keeps the episodes' performance and the Trainer takes a "
                         "train.Monitor (ranked saves; the A/B is tools/ab_trainer_monitor.sh)")
    ap.add_argument("--checkpoint", metavar="PATH", default=None,
                    help="save env, actor, memory and learner after the timed loop (checkpoint.save)")
    ap.add_argument("--resume", metavar="PATH", default=None,
                    help="load a --checkpoint file of a run with the same options before the warm-up")
    args = ap.parse_args()
    if args.reset is None:
        args.reset = "deferred" if args.input == "xp" else "immediate"
    if args.trainer:
        if args.input != "xp" or args.learn or args.checkpoint or args.resume or args.reset == "immediate":
            ap.error("--trainer K runs the 'xp' loop in a device reset mode, without --learn / --checkpoint / --resume")
        if args.physics not in ("iho", "ho") or (args.monitor and args.physics != "ho"):
            ap.error("--trainer K runs the iho or the ho loop; --monitor is the cooling loop's (--physics ho)")
        return trainer_loop(args)
    B = args.batch
    meas = args.input == "measurements"
    wave = args.input == "wavefunction"
    if args.physics != "iho" and not wave:
        ap.error("--physics other than iho is built for --input wavefunction")
    fam = {"iho": cfg.IHO, "iqo": cfg.IQO, "ho": cfg.HO, "qo": cfg.QO}[args.physics]
    ph = cfg.DEFAULTS[fam] if wave else cfg.DEFAULTS[cfg.IHO].with_(n_max=511)
    hidden2 = 512 if fam in (cfg.QO, cfg.IQO) else 256
    env_kw = {}
    if args.t_max is not None:
        env_kw["t_max"] = args.t_max
    if args.init_time is not None:
        env_kw["init_time"] = tuple(args.init_time)
    env = BatchedEnv(ph, B, 0, seed=1, input=args.input, reset=args.reset, **env_kw)
    L = int(env.obs.shape[1]) if wave else 5
    if meas:
        actor = MeasurementActor({k: v.cuda() for k, v in random_dqn_measurement(seed=1).items()}, max_batch=B, seed=2)
        row_len = int(env.rows.shape[1])
        mem = PrioritizedReplay(args.capacity or 262144, row_len, "random", 0.2, device=0, seed=3)
    elif wave:
        wnet = random_direct_dqn(data_length=L, seed=1, hidden2=hidden2)
        actor = DQNActor({k: v.cuda() for k, v in wnet.items()}, data_length=L, max_batch=B, seed=2)
        mem = PrioritizedReplay(args.capacity or 65536, 2 * L + 2, "random", 0.2, device=0, seed=3)
    else:
        actor = DQNActor({k: v.cuda() for k, v in random_direct_dqn(seed=1).items()}, max_batch=B, seed=2)
        mem = PrioritizedReplay(args.capacity or 7000 * 18 * 100, 2 * 5 + 2, "random", 0.2, device=0, seed=3)
    learner = None
    if args.learn and meas:
        from deepreinforcementlearningcontrolofquantumcartpoles_amd.learner import MeasurementLearner
        rec = env.rec      # the env's MeasurementRecord: its read_length and control-step length m
        learner = MeasurementLearner(random_dqn_measurement(seed=1), rec.read_length, rec.m, batch_size=512, device=0,
                                     seed=4)
        assert learner.row_len == row_len
    elif args.learn:
        from deepreinforcementlearningcontrolofquantumcartpoles_amd.learner import DQNLearner
        learner = DQNLearner(wnet if wave else random_direct_dqn(seed=1), batch_size=512, device=0, seed=4)
    objects = {"env": env, "actor": actor, "memory": mem}
    if learner is not None:
        objects["learner"] = learner
    extra = {}
    if args.resume:
        torch.cuda.synchronize()
        tl = time.perf_counter()
        saved = checkpoint.load(args.resume, objects)
        extra["checkpoint_load_ms"] = (time.perf_counter() - tl) * 1e3
        obs, steps_done = env.obs, int(saved["steps_done"])
    else:
        obs = env.reset()
        steps_done = 0
    ev = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731
    marks = []                                          # (actor start, end, replay start, end) per timed step
    rows = torch.zeros((), dtype=torch.int64, device="cuda")
    n_done = torch.zeros((), dtype=torch.int64, device="cuda")
    n_warming = torch.zeros((), dtype=torch.int64, device="cuda")
    # no host synchronisation inside the timed loop (device counters, events read afterwards): the loop's own
    # cost is what the GPU sees
    for it in range(args.warmup + args.steps):
        if it == args.warmup:
            torch.cuda.synchronize()
            if args.marker:
                torch.cuda.nvtx.range_push("timed")
            t0 = time.perf_counter()
            rows.zero_()
            n_done.zero_()
            n_warming.zero_()
        m = [ev(), ev(), ev(), ev()]
        m[0].record()
        a = actor.act(obs, eps=DQNActor.eps_threshold(steps_done))
        m[1].record()
        steps_done += B
        obs, reward, done, info = env.step(a)
        rows += info["valid"].sum()
        n_done += done.sum()
        if "warming" in info:
            n_warming += info["warming"].sum()
        m[2].record()
        if meas:
            mem.store(info["rows"], info["valid"])
        else:
            # the row of a done env holds its terminal observation (IHO/main_parallel.py:250-257); in the immediate
            # mode the returned obs of a done env is already the next episode's
            nxt = torch.where(done[:, None], info["terminal_obs"], obs) if "terminal_obs" in info else obs
            mem.store_xp(info["last_obs"], nxt, a, reward, info["valid"])
        smp = mem.obtain_sample(512) if it > 0 else None
        if smp is not None:
            mem.batch_update(smp[0], torch.rand(512, device="cuda"))
        m[3].record()
        if learner is not None and it > 0:
            for _ in range(args.learn):
                learner.step(mem)
            learner.push(actor)
        if it >= args.warmup:
            marks.append(m)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.marker:
        torch.cuda.nvtx.range_pop()
    actor_ms = sum(m[0].elapsed_time(m[1]) for m in marks)
    replay_ms = sum(m[2].elapsed_time(m[3]) for m in marks)
    rows = int(rows)
    done_frac = int(n_done) / (B * args.steps)
    K = args.steps
    net = "DQN_measurement" if meas else "direct_DQN"
    what = f"{args.physics.upper()} driver defaults" if wave else "IHO N=512"
    if args.checkpoint:
        ts = time.perf_counter()
        checkpoint.save(args.checkpoint, objects, extra={"steps_done": steps_done})
        extra["checkpoint_save_ms"] = (time.perf_counter() - ts) * 1e3
        extra["checkpoint_bytes"] = os.path.getsize(args.checkpoint)
    if args.reset == "warmup":   # share of the batch in its free evolution (not controlled) per call
        extra["warming_fraction_per_control_step"] = int(n_warming) / (B * K)
    if args.t_max is not None:
        extra["t_max"] = args.t_max
    if args.init_time is not None:
        extra["init_time"] = list(args.init_time)
    if learner is not None:
        learn_ms = sum(a[3].elapsed_time(b[0]) for a, b in zip(marks[:-1], marks[1:]))
        extra.update({"learn_steps_per_control_step": args.learn,
                      "learner_ms_per_control_step": learn_ms / max(K - 1, 1),
                      "learner_nonfinite": learner.stats()["nonfinite"]})
    print(json.dumps({"metric": f"actor loop RL steps/s (BatchedEnv {what} input={args.input} reset={args.reset} + device {net} actor)",
                      "value": B * K / dt, "unit": "decisions/s", "env_steps_per_s": B * K * ph.control_interval / dt,
                      # physics env-steps actually taken: the immediate mode adds the reset intervals of the envs
                      # finished in each call (deferred: they are among the B per call)
                      "physics_env_steps_per_s": (B * K + (int(n_done) if args.reset == "immediate" else 0))
                      * ph.control_interval / dt,
                      "batch": B, "control_steps": K, "ms_per_control_step": dt / K * 1e3,
                      "actor_ms_per_control_step": actor_ms / K, "actor_share": actor_ms / (dt * 1e3),
                      "replay_ms_per_control_step": replay_ms / K, "replay_share": replay_ms / (dt * 1e3),
                      "replay_len": len(mem),
                      "done_fraction_per_control_step": done_frac,
                      "experience_rows_per_s": rows / dt,
                      "row_len": mem.data_size, **({"data_length": L, "hidden2": hidden2} if wave else {}), **extra,
                      "data": f"synthetic: |0> resets, random-initialised {net} weights"}), flush=True)


def trainer_loop(args):
    """The --learn K loop's objects through Trainer.step. Every row counts rows * 8 / 256 towards the pacing and an
    update is due per D = (8 / n_times_per_sample) (512 / 256): n_times_per_sample = 1024 K / B makes B / 2 rows
    worth K updates (a call stores one row per env except those that ended in the call before), and
    max_updates_per_tick = K holds every tick at exactly K; the surplus stays pending."""
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.learner import DQNLearner
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.train import Monitor, Schedule, Trainer, performance_from
    B, K = args.batch, args.trainer
    cooling = args.physics == "ho"
    ph = cfg.DEFAULTS[cfg.HO] if cooling else cfg.DEFAULTS[cfg.IHO].with_(n_max=511)
    env_kw = {}
    if args.t_max is not None:
        env_kw["t_max"] = args.t_max
    if args.monitor:   # the reference's threshold, or the same share of a shortened episode
        env_kw["performance_from"] = performance_from(ph) if args.t_max is None else 0.3 * args.t_max
    env = BatchedEnv(ph, B, 0, seed=1, input="xp", reset=args.reset, **env_kw)
    net = random_direct_dqn(seed=1)
    actor = DQNActor({k: v.cuda() for k, v in net.items()}, max_batch=B, seed=2)
    mem = PrioritizedReplay(args.capacity or 7000 * 18 * 100, 2 * 5 + 2, "random", 0.2, device=0, seed=3)
    learner_kw = dict(target="reward", betas=(0.9, 0.999)) if cooling else {}
    learner = DQNLearner(net, batch_size=512, device=0, seed=4, **learner_kw)
    schedule = Schedule.for_driver(ph, batch_size=512, n_times_per_sample=1024. * K / B, max_updates_per_tick=K,
                                   num_episodes=1 << 40, give_up_episodes=1 << 40, t_max=env.t_max)
    monitor = Monitor.for_driver(ph, phonon_cutoff=env.phonon_cutoff) if args.monitor else None
    trainer = Trainer(env, actor, mem, learner, schedule, save_dir=None, monitor=monitor)
    env.reset()
    updates = 0
    for it in range(args.warmup + args.steps):
        if it == args.warmup:
            torch.cuda.synchronize()
            if args.marker:
                torch.cuda.nvtx.range_push("timed")
            t0 = time.perf_counter()
            updates = 0
        trainer.step()
        updates += len(trainer.losses)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.marker:
        torch.cuda.nvtx.range_pop()
    s = schedule.stats()
    what = "HO driver defaults" if cooling else "IHO N=512"
    extra = {"t_max": env.t_max} if cooling else {}
    if monitor is not None:
        extra.update(monitor_receives=monitor.calls, monitor_filled=trainer.n_filled)
    print(json.dumps({"metric": f"trainer loop RL steps/s (train.Trainer.step, BatchedEnv {what} input=xp reset={args.reset}"
                                f"{', performance + monitor' if monitor is not None else ''})", **extra,
                      "value": B * args.steps / dt, "unit": "decisions/s", "batch": B, "control_steps": args.steps,
                      "ms_per_control_step": dt / args.steps * 1e3, "updates_per_control_step": updates / args.steps,
                      "max_updates_per_tick": K, "episodes": s["total_episodes"], "rows": s["total_rows"],
                      "pending_updates": s["pending"], "learner_nonfinite": learner.stats()["nonfinite"],
                      "replay_len": len(mem), "data": "synthetic: |0> resets, random-initialised direct_DQN weights"}),
          flush=True)


if __name__ == "__main__":
    main()
