"""Plain numpy / Python restatement of the batched episode loop's per-control-step bookkeeping for the quartic
cooling driver with a rolling warm-up (kind == QC_QO of qc_env_tail_args and qc_env_warmup_draw, written from the
header comment in include/qcart.h; Control.do_episode, QO/main_parallel.py:169-232), one env at a time in env order.

TEST INFRASTRUCTURE ONLY: the checker of qc_env_tail's QO branch (csrc/qcart_env.hip), imported by tests/ only.
Per env e after a step call in which it took budget[e] physics steps, with quantity[e] the energy after it:
  * warm_left[e] > 0 on entry (warming): left = warm_left - budget, warm_fail |= fail_step > 0; reward 0, not done,
    not valid. left > 0: warm_left = left, budget = min(left, interval). Else, no Fail and quantity <
    init_energy_cutoff (strict, a NaN rejects): live, warm_left = warm_fail = 0, t = steps = return = 0, budget =
    interval, reset = 1. Else a redraw;
  * live: t += interval dt, steps += interval, over = fail_step > 0 or not (quantity < cutoff) or t >= t_trunc;
    reward = float32(-quantity * reward_multiply); valid = not over; return += the float64 product where valid, else
    + 0.0 (the product and the sum rounded separately); budget = interval; over: (return, t) appended to the ring
    fin [2][fin_cap + 1] at fin_n % fin_cap (slot fin_cap of each half is a sink never written), done = 1, and a
    redraw (t and return keep the finished episode's values);
  * redraw (warmup_draw): n = draws[e], draws[e] += 1; Philox4x32-10, key (seed_lo, seed_hi), counter (n_lo, n_hi,
    env_offset + e, 0x400); u = ((w_hi << 32 | w_lo) >> 11) 2^-53 from (w0, w1) and (w2, w3); k = u_k 0.6 - 0.3;
    init_t = lo + u_t (hi - lo); warm_left = max(1, ceil(init_t / dt)); warm_fail = 0; budget = min(warm_left,
    interval); pending = 1. pending (out) is 0 for every env that does not redraw;
  * obs32 = float32(obs) * float32(input_scaling).
"""
from __future__ import annotations

import math

import numpy as np

from oracle.oracle import philox

QO = 2            # enum qc_family of the quartic cooling driver (config.QO)
WARM_TAG = 0x400  # Philox counter word 3 of the warm-up draws
STATE = ("warm_left", "warm_fail", "draws", "k", "budget", "pending", "t", "steps", "episode_return")


def warmup_draw(seed, env_id, n, lo, hi, dt, interval):
    """Draw n of the env with global id env_id: (k, init_t, warm_left, budget)."""
    seed, n = int(seed), int(n)
    w = philox([n & 0xFFFFFFFF, (n >> 32) & 0xFFFFFFFF, int(env_id) & 0xFFFFFFFF, WARM_TAG],
               [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    u_k = np.float64(((int(w[0]) << 32) | int(w[1])) >> 11) * np.float64(2.0 ** -53)
    u_t = np.float64(((int(w[2]) << 32) | int(w[3])) >> 11) * np.float64(2.0 ** -53)
    k = u_k * np.float64(0.6) - np.float64(0.3)
    init_t = np.float64(lo) + u_t * (np.float64(hi) - np.float64(lo))
    left = max(1, int(math.ceil(init_t / np.float64(dt))))
    return k, init_t, left, min(left, int(interval))


def new_state(B, interval, fin_cap):
    """The state BatchedEnv(reset='warmup') starts from, before any draw."""
    return dict(warm_left=np.zeros(B, np.int32), warm_fail=np.zeros(B, np.uint8), draws=np.zeros(B, np.int64),
                k=np.zeros(B, np.float64), budget=np.full(B, interval, np.int32), pending=np.zeros(B, np.uint8),
                t=np.zeros(B, np.float64), steps=np.zeros(B, np.int64), episode_return=np.zeros(B, np.float64),
                fin=np.zeros((2, fin_cap + 1), np.float64), fin_n=0)


def _redraw(o, e, seed, env_offset, lo, hi, dt, interval):
    k, _, left, bud = warmup_draw(seed, env_offset + e, o["draws"][e], lo, hi, dt, interval)
    o["draws"][e] += 1
    o["k"][e], o["warm_left"][e], o["warm_fail"][e], o["budget"][e], o["pending"][e] = k, left, 0, bud, 1


def env_warmup_draw_ref(s, mask, seed, env_offset, lo, hi, dt, interval):
    """qc_env_warmup_draw: the masked envs start a warm-up, their t, steps and return back to zero. Returns the new
    state (the input is not modified)."""
    o = {k: np.array(v) for k, v in s.items()}
    for e in range(len(o["pending"])):
        if mask is None or mask[e]:
            _redraw(o, e, seed, env_offset, lo, hi, dt, interval)
            o["t"][e], o["steps"][e], o["episode_return"][e] = 0.0, 0, 0.0
    return o


def env_tail_warmup_ref(s, interval, dt, input_scaling, cutoff, t_trunc, reward_multiply, init_energy_cutoff, lo, hi,
                        seed, env_offset, fail_step, quantity, obs):
    """One call of the QO branch on the state dict s (STATE arrays, fin, fin_n). Returns a dict of new arrays (the
    inputs are not modified): the STATE arrays, fin, fin_n, obs32, reward, done, valid, reset."""
    B = len(s["pending"])
    fin_cap = s["fin"].shape[1] - 1
    with np.errstate(over="ignore"):   # an observable beyond float32's range becomes inf, as in C
        obs32 = np.asarray(obs, np.float64).astype(np.float32) * np.float32(input_scaling)
    o = {k: np.array(s[k]) for k in STATE}
    o.update(pending=np.zeros(B, np.uint8), fin=np.array(s["fin"], np.float64), obs32=obs32,
             reward=np.zeros(B, np.float32), done=np.zeros(B, np.uint8), valid=np.zeros(B, np.uint8),
             reset=np.zeros(B, np.uint8))
    fin_n = int(s["fin_n"])
    ci_dt = np.float64(interval) * np.float64(dt)
    cutoff, t_trunc, rm = np.float64(cutoff), np.float64(t_trunc), np.float64(reward_multiply)
    for e in range(B):
        fail = fail_step[e] > 0
        q = np.float64(quantity[e])
        redraw = False
        if s["warm_left"][e] > 0:
            left = int(s["warm_left"][e]) - int(s["budget"][e])
            wfail = bool(s["warm_fail"][e]) or fail
            if left > 0:
                o["warm_left"][e], o["warm_fail"][e], o["budget"][e] = left, int(wfail), min(left, interval)
            elif not wfail and q < np.float64(init_energy_cutoff):
                o["warm_left"][e] = o["warm_fail"][e] = 0
                o["budget"][e] = interval
                o["t"][e], o["steps"][e], o["episode_return"][e] = 0.0, 0, 0.0
                o["reset"][e] = 1
            else:
                redraw = True
        else:
            tt = np.float64(s["t"][e]) + ci_dt
            over = bool(fail or not (q < cutoff) or tt >= t_trunc)
            with np.errstate(over="ignore", invalid="ignore"):
                r = -q * rm                                   # one rounding
                o["reward"][e] = np.float32(r)
                o["episode_return"][e] = np.float64(s["episode_return"][e]) + (np.float64(0.0) if over else r)
            o["t"][e] = tt
            o["steps"][e] = int(s["steps"][e]) + interval
            o["valid"][e] = 0 if over else 1
            o["done"][e] = 1 if over else 0
            o["budget"][e] = interval
            if over:
                pos = fin_n % fin_cap
                o["fin"][0, pos] = o["episode_return"][e]
                o["fin"][1, pos] = tt
                fin_n += 1
                redraw = True
        if redraw:
            _redraw(o, e, seed, env_offset, lo, hi, dt, interval)
    o["fin_n"] = fin_n
    return o
