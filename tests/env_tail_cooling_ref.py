"""Plain numpy / Python restatement of the batched episode loop's per-control-step bookkeeping for the harmonic
cooling driver (kind == QC_HO of qc_env_tail_args, include/qcart.h; Control.do_episode, HO/main_parallel.py:222-292)
and BatchedEnv's immediate-mode cooling accounting (env.py: step, reset, _push_finished), one env at a time in env
order.

TEST INFRASTRUCTURE ONLY: the checker of qc_env_tail's cooling branch (csrc/qcart_env.hip), imported by tests/ only.
Per env e after a step call of one control interval, with quantity[e] the phonon number after it:
  * pending[e] (in) set: the call was the env's reset interval: t = interval dt, steps = interval, return 0,
    reward 0, transition not valid; the episode is already over iff fail_step > 0 or quantity > cutoff (a NaN
    quantity does not end it, and there is no truncation check);
  * otherwise: t += interval dt, steps += interval, over = fail_step > 0 or not (quantity <= cutoff) (a NaN
    quantity ends it) or t >= t_trunc; reward = float32(-quantity * reward_multiply); the transition is valid
    iff not over; return += -quantity * reward_multiply where valid, else + 0.0 (float64, the product and the sum
    rounded separately);
  * over: (return, t) appended to the ring fin [2][fin_cap + 1] at fin_n % fin_cap (slot fin_cap of each half is
    a sink the bookkeeping never writes), done = pending (out) = 1;
  * rec_mode = 2 for an env pending on entry, else 1; obs32 = float32(obs) * float32(input_scaling).
"""
from __future__ import annotations

import numpy as np

HO = 0   # enum qc_family of the harmonic cooling driver (config.HO)


def env_tail_cooling_ref(interval, dt, input_scaling, cutoff, t_trunc, reward_multiply, fail_step, quantity, obs,
                         pending, t, steps, episode_return, fin, fin_cap, fin_n):
    """Returns a dict of new arrays (the inputs are not modified): pending, t, steps, episode_return, obs32,
    reward, done, valid, rec_mode, fin, fin_n."""
    B = len(pending)
    assert fin.shape == (2, fin_cap + 1)
    with np.errstate(over="ignore"):   # an observable beyond float32's range becomes inf, as in C
        obs32 = np.asarray(obs, np.float64).astype(np.float32) * np.float32(input_scaling)
    o = dict(pending=np.zeros(B, np.uint8), t=np.array(t, np.float64), steps=np.array(steps, np.int64),
             episode_return=np.array(episode_return, np.float64), reward=np.zeros(B, np.float32),
             done=np.zeros(B, np.uint8), valid=np.zeros(B, np.uint8), rec_mode=np.zeros(B, np.uint8),
             fin=np.array(fin, np.float64), obs32=obs32)
    fin_n = int(fin_n)
    ci_dt = np.float64(interval) * np.float64(dt)
    cutoff, t_trunc, rm = np.float64(cutoff), np.float64(t_trunc), np.float64(reward_multiply)
    for e in range(B):
        fail = fail_step[e] > 0
        q = np.float64(quantity[e])
        if pending[e]:
            over = bool(fail or q > cutoff)
            o["t"][e] = ci_dt
            o["steps"][e] = interval
            o["episode_return"][e] = 0.0
            o["reward"][e] = 0.0
            o["valid"][e] = 0
            o["rec_mode"][e] = 2
        else:
            tt = np.float64(t[e]) + ci_dt
            over = bool(fail or not (q <= cutoff) or tt >= t_trunc)
            with np.errstate(over="ignore", invalid="ignore"):
                r = -q * rm                                   # one rounding
                o["reward"][e] = np.float32(r)
                o["episode_return"][e] = np.float64(episode_return[e]) + (np.float64(0.0) if over else r)   # another
            o["t"][e] = tt
            o["steps"][e] = int(steps[e]) + interval
            o["valid"][e] = 0 if over else 1
            o["rec_mode"][e] = 1
        o["done"][e] = o["pending"][e] = 1 if over else 0
        if over:
            pos = fin_n % fin_cap
            o["fin"][0, pos] = o["episode_return"][e]
            o["fin"][1, pos] = o["t"][e]
            fin_n += 1
    o["fin_n"] = fin_n
    return o
