"""Plain numpy / Python restatement of the per-episode performance that qc_env_tail keeps for the cooling drivers
(the perf_sum, perf_n, perf and perf_from fields of qc_env_tail_args, include/qcart.h; the drivers' avg_phonon /
avg_energy, HO/main_parallel.py:247-248, 274-275, 294-295, QO/main_parallel.py:221, 231-232). It wraps the existing
restatements of the two cooling kinds (tests/env_tail_cooling_ref.py, tests/env_tail_warmup_ref.py), whose outputs
it leaves as they are, and adds the three performance fields, one env at a time in env order.

TEST INFRASTRUCTURE ONLY: the checker of qc_env_tail's performance accounting (csrc/qcart_env.hip) and of
BatchedEnv(performance_from=...), imported by tests/ only.
Per env e:
  * an episode starts (HO: pending on entry; QO: the env goes live; qc_env_warmup_draw): perf_sum = 0, perf_n = 0;
  * a live control step (HO's pending first control step is one, QO's go-live call is not) that does not end the
    episode and whose new episode time t is > perf_from: perf_sum += quantity (one rounding), perf_n += 1;
  * a finished episode: p = perf_sum / perf_n (one rounding) when t >= t_trunc and perf_n > 0, else cutoff; p goes
    to perf[i % fin_cap], i its position in fin (slot fin_cap is a sink never written);
  * a warming QO env touches nothing.
"""
from __future__ import annotations

import numpy as np

from tests.env_tail_cooling_ref import env_tail_cooling_ref
from tests.env_tail_warmup_ref import env_tail_warmup_ref, env_warmup_draw_ref

PERF = ("perf_sum", "perf_n", "perf")


def new_perf(B, fin_cap, fill=0.0):
    """The performance fields BatchedEnv(performance_from=...) starts from."""
    return dict(perf_sum=np.zeros(B, np.float64), perf_n=np.zeros(B, np.int64),
                perf=np.full(fin_cap + 1, fill, np.float64))


def _account(o, p, fin_n, fin_cap, start, live, quantity, cutoff, t_trunc, perf_from):
    """The performance pass over the outputs o of a base restatement: start[e] / live[e] say whether env e's
    episode started in this call and whether the call was a live control step of it."""
    out = {k: np.array(p[k]) for k in PERF}
    fin_n = int(fin_n)
    for e in range(len(start)):
        if not (start[e] or live[e]):
            continue
        ps = np.float64(0.0) if start[e] else np.float64(p["perf_sum"][e])
        pn = 0 if start[e] else int(p["perf_n"][e])
        over = bool(o["done"][e])
        tt = np.float64(o["t"][e])
        if live[e] and not over and tt > np.float64(perf_from):
            with np.errstate(over="ignore", invalid="ignore"):
                ps = ps + np.float64(quantity[e])          # one rounding
            pn += 1
        out["perf_sum"][e], out["perf_n"][e] = ps, pn
        if over:
            with np.errstate(over="ignore", invalid="ignore"):
                val = ps / np.float64(pn) if (tt >= np.float64(t_trunc) and pn > 0) else np.float64(cutoff)
            out["perf"][fin_n % fin_cap] = val
            fin_n += 1
    assert fin_n == int(o["fin_n"])
    return out


def env_tail_cooling_perf_ref(interval, dt, input_scaling, cutoff, t_trunc, reward_multiply, fail_step, quantity, obs,
                              pending, t, steps, episode_return, fin, fin_cap, fin_n, p, perf_from):
    """kind QC_HO with perf: env_tail_cooling_ref's outputs plus perf_sum, perf_n and perf from the dict p."""
    o = env_tail_cooling_ref(interval, dt, input_scaling, cutoff, t_trunc, reward_multiply, fail_step, quantity, obs,
                             pending, t, steps, episode_return, fin, fin_cap, fin_n)
    start = np.asarray(pending) != 0
    o.update(_account(o, p, fin_n, fin_cap, start, np.ones(len(start), bool), quantity, cutoff, t_trunc, perf_from))
    return o


def env_tail_warmup_perf_ref(s, interval, dt, input_scaling, cutoff, t_trunc, reward_multiply, init_energy_cutoff, lo,
                             hi, seed, env_offset, fail_step, quantity, obs, perf_from):
    """kind QC_QO with perf: env_tail_warmup_ref on the state dict s, which also holds perf_sum, perf_n and perf."""
    o = env_tail_warmup_ref(s, interval, dt, input_scaling, cutoff, t_trunc, reward_multiply, init_energy_cutoff, lo,
                            hi, seed, env_offset, fail_step, quantity, obs)
    warming = np.asarray(s["warm_left"]) > 0
    start = warming & (o["reset"] != 0)
    fin_cap = s["fin"].shape[1] - 1
    o.update(_account(o, s, s["fin_n"], fin_cap, start, ~warming, quantity, cutoff, t_trunc, perf_from))
    return o


def env_warmup_draw_perf_ref(s, mask, seed, env_offset, lo, hi, dt, interval):
    """qc_env_warmup_draw with perf: the masked envs' sums go back to zero with their t, steps and return."""
    o = env_warmup_draw_ref({k: v for k, v in s.items() if k not in PERF}, mask, seed, env_offset, lo, hi, dt, interval)
    for k in PERF:
        o[k] = np.array(s[k])
    for e in range(len(o["pending"])):
        if mask is None or mask[e]:
            o["perf_sum"][e], o["perf_n"][e] = 0.0, 0
    return o
