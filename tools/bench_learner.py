#!/usr/bin/env python3
"""The device DQN learner beside the same update written in torch, on one GPU.

Device path: DQNLearner.update (csrc/qcart_learner.hip, eight launches per update). Baseline: what
INTEGRATION.md §3 made users do before: direct_DQN with the chunked NoisyNet noise, the TD loss, autograd and
the reference's LaProp as per-tensor torch ops (tests/learner_ref.py's restatement, on the same GPU, fp32).
Both run the same fixed batch with injected noise; per batch size: warmup updates, then `--steps` timed
updates between two synchronisations (wall clock, so the host's launch cost counts, as it does in a loop).
Prints one JSON line: ms per update at B = 128 and 512 for both paths and the learner's launches per update.
--hidden2 512 measures the quartic drivers' net (fc2 512 -> 512; tests/dqn_variants_ref.py's restatement as baseline).
--data-length L measures another input length (the 'wavefunction' input: 122 / 302 / 322 / 1002 floats for the HO / QO /
IHO / IQO drivers), with tests/dqn_variants_ref.py's batches and restatement at either width.
usage: python tools/bench_learner.py [--steps K] [--warmup W] [--hidden2 {256,512}] [--data-length L]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deepreinforcementlearningcontrolofquantumcartpoles_amd.actor import random_direct_dqn  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd.learner import DQNLearner  # noqa: E402
from tests import dqn_variants_ref as V  # noqa: E402
from tests import learner_ref as R  # noqa: E402


class TorchLearner:
    """TrainDQN.__call__ + LaProp (centered, betas (0.9, 0.9995)) as torch ops on the device."""

    def __init__(self, params, lr=4e-4, backup_period=300):
        narrow_xp = params["fc2.weight"].shape[0] == 256 and params["fc1.weight"].shape[1] == 5
        self.td_loss = R.td_loss if narrow_xp else V.td_loss
        self.p = {k: v.detach().cuda().float().clone().requires_grad_(True) for k, v in params.items()}
        self.state = {k: [torch.zeros_like(v), torch.zeros_like(v), torch.zeros_like(v)] for k, v in self.p.items()}
        self.lr, self.step_count, self.l1, self.l2 = lr, 0, 0.0, 0.0
        self.backup_period, self.backup_counter, self.target = backup_period, 0, None

    def update(self, tr, w, noise):
        if self.backup_counter == 0:
            self.target = {k: v.detach().clone() for k, v in self.p.items()}
        self.backup_counter = (self.backup_counter + 1) % self.backup_period
        loss, ul, _ = self.td_loss(self.p, self.target, tr, w, noise)
        loss.backward()
        b1, b2, lr = 0.9, 0.9995, self.lr
        self.step_count += 1
        self.l1 = self.l1 * b1 + (1 - b1) * lr
        self.l2 = self.l2 * b2 + (1 - b2)
        step_size = 1.0 / (self.l1 / lr if lr != 0.0 else 1.0)
        with torch.no_grad():
            for k, p in self.p.items():
                g = p.grad
                e, v, mu = self.state[k]
                v.mul_(b2).addcmul_(g, g, value=1 - b2)
                mu.mul_(b2).add_(g, alpha=1 - b2)
                den = v - mu ** 2 if self.step_count > 10 else v
                den = den.div(self.l2).sqrt_().add_(1e-15)
                e.mul_(b1).add_(g / den, alpha=(1 - b1) * lr)
                p.add_(e, alpha=-step_size)
                p.grad = None
        return ul.detach()


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--hidden2", type=int, default=256, choices=(256, 512), help="fc2's width")
    ap.add_argument("--data-length", type=int, default=5, help="the network input's length")
    args = ap.parse_args()
    L = args.data_length
    params = random_direct_dqn(data_length=L, seed=11, hidden2=args.hidden2)
    out = {"metric": "DQN learner ms per update (direct_DQN, LaProp; device learner vs torch on the same GPU)",
           "unit": "ms/update", "steps": args.steps, "warmup": args.warmup, "hidden2": args.hidden2,
           "data_length": L}
    for B in (128, 512):
        tr, w, nz = (torch.as_tensor(a).cuda() for a in
                      (R.make_batch(B, 2) if args.hidden2 == 256 and L == 5
                       else V.make_batch(B, 2, L=L, hidden2=args.hidden2)))
        dev = DQNLearner(params, batch_size=B)
        ref = TorchLearner(params)
        # alternate the two paths (one process, the same clock state), keep each path's best round
        d_ms, t_ms = [], []
        for _ in range(3):
            d_ms.append(timed(lambda: dev.update(tr, w, noise=nz), args.warmup, args.steps))
            t_ms.append(timed(lambda: ref.update(tr, w, nz), args.warmup, args.steps))
        st = dev.stats()
        out[f"device_ms_B{B}"] = min(d_ms)
        out[f"torch_ms_B{B}"] = min(t_ms)
        out[f"device_ms_rounds_B{B}"] = d_ms
        out[f"torch_ms_rounds_B{B}"] = t_ms
        out[f"speedup_B{B}"] = min(t_ms) / min(d_ms)
        out["launches_per_update"] = st["launches_per_update"]
        assert st["nonfinite"] == 0
    out["value"] = out["device_ms_B512"]
    out["data"] = "synthetic: one fixed batch (tests/learner_ref.make_batch), random-initialised direct_DQN, injected noise"
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
