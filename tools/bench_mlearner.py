#!/usr/bin/env python3
"""The device measurement learner beside the same update written in torch, on one GPU.

Device path: MeasurementLearner.update (csrc/qcart_mlearner.hip, 28 launches per update). Baseline: the same
update as torch ops on the same GPU in the same run (tests/mlearner_ref.py's restatement in fp32: F.conv1d /
F.linear, the chunked NoisyNet noise, the TD loss, autograd, LaProp as per-tensor ops). Both run one fixed batch
with injected noise at L = `--read-length` (5760; the harmonic driver's is 4320), m = 80; per batch size: warmup
updates, then `--steps` timed updates between two synchronisations (wall clock), best of 3 alternating rounds.
`--conv-weight-norm` adds, in the same rounds, the harmonic driver's handle (weight-normalised convolutions, target
"reward", betas (0.9, 0.999)) and its torch baseline (F.conv1d on W g / ||W||_F), and reports its cost over the plain
handle's. Prints one JSON line.
usage: python tools/bench_mlearner.py [--steps K] [--warmup W] [--read-length L] [--conv-weight-norm]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deepreinforcementlearningcontrolofquantumcartpoles_amd.learner import MeasurementLearner  # noqa: E402
from tests import mlearner_ref as M  # noqa: E402
from tests import mlearner_wn_ref as W  # noqa: E402

L, MS = 5760, 80   # L: --read-length
PEAK_F32_MFMA = 157.3e12


class TorchLearner:
    """TrainDQN.__call__ + LaProp (centered) as torch ops on the device; convolutions with a weight_norm key are
    F.conv1d on W g / ||W||_F (mlearner_wn_ref.effective)."""

    def __init__(self, params, lr=4e-4, backup_period=300, target="alive", betas=(0.9, 0.9995)):
        self.td_target, self.betas = target, betas
        self.p = {k: v.detach().cuda().float().clone().requires_grad_(True) for k, v in params.items()}
        self.state = {k: [torch.zeros_like(v), torch.zeros_like(v), torch.zeros_like(v)] for k, v in self.p.items()}
        self.lr, self.step_count, self.l1, self.l2 = lr, 0, 0.0, 0.0
        self.backup_period, self.backup_counter, self.target = backup_period, 0, None

    def update(self, tr, w, noise):
        if self.backup_counter == 0:
            self.target = {k: v.detach().clone() for k, v in self.p.items()}
        self.backup_counter = (self.backup_counter + 1) % self.backup_period
        loss, ul, _ = W.td_loss(self.p, self.target, tr, w, noise, L, MS, target=self.td_target)
        loss.backward()
        (b1, b2), lr = self.betas, self.lr
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


def gemm_flops(B):
    """FLOPs per update of each GEMM family (2 MACs): forward on 3 B states, backward on B."""
    t = M.dims(L)
    fwd = sum(2 * co * ci * k * t[j + 1] for j, (ci, co, k, _) in enumerate(M.CONV)) + 2 * 64 * t[3] * 256
    dw = sum(2 * co * ci * k * t[j + 1] for j, (ci, co, k, _) in enumerate(M.CONV))
    dx = sum(2 * co * ci * k * t[j + 1] for j, (ci, co, k, _) in enumerate(M.CONV) if j > 0)
    return {"forward_3B": 3 * B * fwd, "conv_dw": B * dw, "conv_dx": B * dx, "fc1_t_and_dw": B * 2 * 2 * 64 * t[3] * 256}


def main():
    global L
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--device-only", action="store_true", help="only the device learner (for a kernel trace)")
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--read-length", type=int, default=L, help="L (a multiple of 80): 5760 inverted harmonic, 4320 harmonic")
    ap.add_argument("--conv-weight-norm", action="store_true",
                    help="also the harmonic driver's handle (weight-normalised convolutions) and its torch baseline")
    args = ap.parse_args()
    L = args.read_length
    params = M.random_params(L, seed=5)
    ho = {"target": "reward", "betas": (0.9, 0.999)}
    out = {"metric": "measurement learner ms per update (DQN_measurement, LaProp; device learner vs torch on the same GPU)",
           "unit": "ms/update", "steps": args.steps, "warmup": args.warmup, "read_length": L, "read_step_length": MS,
           "conv_weight_norm": bool(args.conv_weight_norm)}
    for B in args.batches:
        tr, w, nz = (torch.as_tensor(a).cuda() for a in M.make_batch(B, 3, L, MS))
        dev = MeasurementLearner(params, L, MS, batch_size=B)
        ref = None if args.device_only else TorchLearner(params)
        wdev = wref = None
        if args.conv_weight_norm:
            wparams = W.random_params(L, seed=5)
            wtr = torch.as_tensor(W.make_batch(B, 3, L, MS, "reward")[0]).cuda()
            wdev = MeasurementLearner(wparams, L, MS, batch_size=B, **ho)
            wref = None if args.device_only else TorchLearner(wparams, **ho)
        d_ms, t_ms, wd_ms, wt_ms = [], [], [], []
        for _ in range(1 if args.device_only else 3):
            d_ms.append(timed(lambda: dev.update(tr, w, noise=nz), args.warmup, args.steps))
            if wdev is not None:
                wd_ms.append(timed(lambda: wdev.update(wtr, w, noise=nz), args.warmup, args.steps))
            if ref is not None:
                t_ms.append(timed(lambda: ref.update(tr, w, nz), max(2, args.warmup // 4), max(5, args.steps // 4)))
            if wref is not None:
                wt_ms.append(timed(lambda: wref.update(wtr, w, nz), max(2, args.warmup // 4), max(5, args.steps // 4)))
        st = dev.stats()
        if wdev is not None:
            wst = wdev.stats()
            assert wst["nonfinite"] == 0
            out[f"device_wn_ms_B{B}"] = min(wd_ms)
            out[f"device_wn_ms_rounds_B{B}"] = wd_ms
            out[f"wn_minus_plain_us_B{B}"] = (min(wd_ms) - min(d_ms)) * 1e3
            out[f"wn_over_plain_B{B}"] = min(wd_ms) / min(d_ms)
            out["launches_per_update_wn"] = wst["launches_per_update"]
            if wt_ms:
                out[f"torch_wn_ms_B{B}"] = min(wt_ms)
                out[f"torch_wn_ms_rounds_B{B}"] = wt_ms
                out[f"speedup_wn_B{B}"] = min(wt_ms) / min(wd_ms)
        out[f"device_ms_B{B}"] = min(d_ms)
        out[f"device_ms_rounds_B{B}"] = d_ms
        if t_ms:
            out[f"torch_ms_B{B}"] = min(t_ms)
            out[f"torch_ms_rounds_B{B}"] = t_ms
            out[f"speedup_B{B}"] = min(t_ms) / min(d_ms)
        fl = gemm_flops(B)
        out[f"gemm_flops_B{B}"] = fl
        out[f"update_frac_of_f32_mfma_peak_B{B}"] = sum(fl.values()) / (min(d_ms) * 1e-3) / PEAK_F32_MFMA
        out["launches_per_update"] = st["launches_per_update"]
        assert st["nonfinite"] == 0
        del dev, ref, wdev, wref
    out["value"] = out[f"device_ms_B{args.batches[-1]}"]
    out["data"] = "synthetic: one fixed batch (tests/mlearner_ref.make_batch), random-initialised DQN_measurement, injected noise"
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
