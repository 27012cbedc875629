"""Plain numpy / Python restatement of the batched episode loop's per-control-step bookkeeping: the header
comment of qc_env_tail_args (include/qcart.h) and BatchedEnv's immediate-mode accounting (env.py: step,
reset, _push_finished), one env at a time in env order.

TEST INFRASTRUCTURE ONLY: the checker of qc_env_tail (csrc/qcart_env.hip), imported by tests/ only.
Per env e after a step call of one control interval:
  * over = Fail in the interval (fail_step > 0) or out of bounds (IHO: |obs[e][0]| > xth, strictly;
    IQO: term_step[e] >= 0);
  * pending[e] (in) set: the call was the env's reset interval: t = interval dt, steps = interval, return 0,
    reward 0, transition not valid;
  * otherwise: t += interval dt, steps += interval, reward = failing_reward when over else 1 (float32 in the
    row, float64 in the return), transition valid;
  * over: (return, t) appended to the ring fin [2][fin_cap + 1] at fin_n % fin_cap (slot fin_cap of each
    half is a sink the bookkeeping never writes), done = pending (out) = 1.
"""
from __future__ import annotations

import numpy as np

IHO, IQO = 1, 3   # enum qc_family of the two cartpoles (config.IHO, config.IQO)


def env_tail_ref(kind, interval, dt, xth, input_scaling, failing_reward, fail_step, term_step, obs, pending, t,
                 steps, episode_return, fin, fin_cap, fin_n):
    """Returns a dict of new arrays (the inputs are not modified): pending, t, steps, episode_return, obs32,
    reward, done, valid, fin, fin_n."""
    B = len(pending)
    assert kind in (IHO, IQO) and fin.shape == (2, fin_cap + 1)
    with np.errstate(over="ignore"):   # an observable beyond float32's range becomes inf, as in C
        obs32 = np.asarray(obs, np.float64).astype(np.float32) * np.float32(input_scaling)
    o = dict(pending=np.zeros(B, np.uint8), t=np.array(t, np.float64), steps=np.array(steps, np.int64),
             episode_return=np.array(episode_return, np.float64), reward=np.zeros(B, np.float32),
             done=np.zeros(B, np.uint8), valid=np.zeros(B, np.uint8), fin=np.array(fin, np.float64),
             obs32=obs32)
    fin_n = int(fin_n)
    ci_dt = interval * dt
    for e in range(B):
        fail = fail_step[e] > 0
        oob = term_step[e] >= 0 if kind == IQO else abs(float(obs[e][0])) > xth
        over = bool(fail or oob)
        if pending[e]:
            o["t"][e] = ci_dt
            o["steps"][e] = interval
            o["episode_return"][e] = 0.0
            o["reward"][e] = 0.0
            o["valid"][e] = 0
        else:
            rw = failing_reward if over else 1.0
            o["t"][e] = float(t[e]) + ci_dt
            o["steps"][e] = int(steps[e]) + interval
            o["episode_return"][e] = float(episode_return[e]) + rw
            o["reward"][e] = np.float32(rw)
            o["valid"][e] = 1
        o["done"][e] = o["pending"][e] = 1 if over else 0
        if over:
            pos = fin_n % fin_cap
            o["fin"][0, pos] = o["episode_return"][e]
            o["fin"][1, pos] = o["t"][e]
            fin_n += 1
    o["fin_n"] = fin_n
    return o
