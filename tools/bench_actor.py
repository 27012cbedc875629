#!/usr/bin/env python3
"""Measurement of the device DQN actor: one qc_actor_act over the per-GPU metric batch
(65 536 envs, 'xp' input, noisy_layers = 2, in-kernel NoisyNet noise), timed with HIP events on the
actor's stream; roofline against the f32-input MFMA peak (MI355X_MICROARCH.md: 157.3 TF).
--hidden2 512 measures the quartic drivers' net (fc2 512 -> 512). --data-length L measures another input length (the
'wavefunction' input: 122 / 302 / 322 / 1002 floats for the HO / QO / IHO / IQO drivers; above 512 fc1 runs over the
input in chunks). --torch adds the same forward (per-env factorised noise drawn with torch.randn, argmax) as torch
ops on the same GPU, timed the same way in alternating rounds.
Prints one JSON line.
usage: python tools/bench_actor.py [--batch B] [--reps K] [--hidden2 {256,512}] [--data-length L] [--torch]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deepreinforcementlearningcontrolofquantumcartpoles_amd.actor import DQNActor, random_direct_dqn  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def flops_per_env(data_length=5, n_actions=21, noisy=True, hidden2=256):
    macs = data_length * 512 + 512 * hidden2 + (2 if noisy else 1) * hidden2 * 256 + (2 if noisy else 1) * 256 * n_actions
    return 2 * macs


def torch_act(p, obs, hidden2):
    """direct_DQN's action selection as torch ops: weight-normalised fc1 / fc2, factorised-noisy fc31 / fc41 with
    one noise sample per env (what the device actor draws in-kernel), argmax."""
    def wn(name, x):
        w = p[f"{name}.weight"]
        return torch.addmm(p[f"{name}.bias"], x, (w * (p[f"{name}.weight_norm"] / w.norm())).T)

    def f(n):
        z = torch.randn((obs.shape[0], n), device=obs.device)
        return z.sign() * z.abs().sqrt()

    def noisy(name, x, i, o):
        return (torch.addmm(p[f"{name}.u_b"], x, p[f"{name}.u_w"].T)
                + f(o) * torch.addmm(p[f"{name}.sigma_b"], f(i) * x, p[f"{name}.sigma_w"].T))

    h2 = torch.relu(wn("fc2", torch.relu(wn("fc1", obs))))
    q = noisy("fc41", torch.relu(noisy("fc31", h2, hidden2, 256)), 256, p["fc41.u_b"].shape[0])
    return q.max(1)[1]


def timed(fn, reps):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hidden2", type=int, default=256, choices=(256, 512), help="fc2's width")
    ap.add_argument("--data-length", type=int, default=5, help="the network input's length")
    ap.add_argument("--torch", action="store_true", help="also time the same forward as torch ops on this GPU")
    args = ap.parse_args()
    B, L = args.batch, args.data_length
    params = {k: v.cuda() for k, v in random_direct_dqn(data_length=L, seed=1, hidden2=args.hidden2).items()}
    actor = DQNActor(params, data_length=L, max_batch=B, seed=2)
    obs = torch.randn((B, L), device="cuda")
    actor.act(obs, eps=0.01)
    torch.cuda.synchronize()
    extra = {}
    if args.torch:
        # alternate the two paths (one process, the same clock state), keep each path's best round
        torch_act(params, obs, args.hidden2)
        torch.cuda.synchronize()
        d_ms, t_ms = [], []
        for _ in range(3):
            d_ms.append(timed(lambda: actor.act(obs, eps=0.01), args.reps))
            t_ms.append(timed(lambda: torch_act(params, obs, args.hidden2), args.reps))
        ms = min(d_ms)
        extra = {"device_ms_rounds": d_ms, "torch_ms_rounds": t_ms, "torch_ms_per_call": min(t_ms),
                 "speedup": min(t_ms) / ms}
    else:
        ms = timed(lambda: actor.act(obs, eps=0.01), args.reps)
    fpe = flops_per_env(data_length=L, hidden2=args.hidden2)
    fl = fpe * B
    print(json.dumps({"metric": "DQN actor decisions/s (one qc_actor_act over the batch)", "value": B / ms * 1e3,
                      "unit": "decisions/s", "batch": B, "hidden2": args.hidden2, "data_length": L, "ms_per_call": ms,
                      "dtype": "f32", **extra,
                      "roofline": {"bound": "mfma", "achieved": fl / (ms * 1e-3) / 1e12,
                                   "peak": PEAK_F32_MFMA / 1e12, "unit": "TFLOP/s",
                                   "frac": fl / (ms * 1e-3) / PEAK_F32_MFMA, "flops_per_decision": fpe},
                      "note": "time includes the in-kernel NoisyNet noise draw (k_actor_noise) and epsilon-greedy"}),
          flush=True)


if __name__ == "__main__":
    main()
