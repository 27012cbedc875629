#!/usr/bin/env python3
"""Times the phase-space view (wigner.WignerView) against torch's own route on one GPU, in one session:

    yardstick   c[b, i, k] = conj(phi[b, i + k]) phi[b, i - k] gathered by index (zero past K_i),
                W = (2 h / pi) Re(torch.matmul(c, Z)), Z[k][j] = e^{2 i p_j k h} (Z[0] = 1/2), then mean(0);
                chunked over the envs so that c stays below 1 GiB

at x_n = 250 points (the drivers' grid) and P = 128 momenta: `wigner` and `mean_wigner` at B in {1024, 4096}, and the
`mean_wigner` of the evaluation loop at B = 65 536. Each round times, in this order and with device events around
back-to-back calls, the view's call and then the yardstick's, so the two sides alternate and share whatever else the
machine is doing. Reported per entry: the rounds' times per call (ms), their median, min and max; for the view's calls
the achieved fp64 rate, counting the triangular contraction's sum_i 4 K_i P real operations per env, against the
78.6 TF/s peak. The outputs are compared once before timing. Writes one JSON file.

    python tools/bench_wigner.py --out profiles/wigner_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP64_TFLOPS = 78.6


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def summary(ms):
    return {"ms": [round(v, 5) for v in ms], "median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5),
            "max_ms": round(max(ms), 5)}


class Yardstick:
    """torch's route on the same table."""

    def __init__(self, view, chunk):
        X, h = view.x_n, view.h
        K = (X - 1) // 2
        i, k = torch.arange(X, device="cuda")[:, None], torch.arange(K + 1, device="cuda")[None, :]
        ok = k <= torch.minimum(i, X - 1 - i)
        self.up = torch.where(ok, i + k, X)          # (index X: the zero column appended to phi)
        self.dn = torch.where(ok, i - k, X)
        ang = 2.0 * h * torch.arange(K + 1, device="cuda", dtype=torch.float64)[:, None] * view.p[None, :]
        self.Z = torch.polar(torch.ones_like(ang), ang)
        self.Z[0] = 0.5
        self.scale, self.chunk = 2.0 * h / np.pi, chunk

    def wigner(self, phi):
        pad = torch.cat([phi, torch.zeros_like(phi[:, :1])], dim=1)
        c = pad[:, self.up].conj() * pad[:, self.dn]
        return torch.matmul(c, self.Z).real * self.scale

    def each(self, phi):
        """Every env's W, chunk after chunk (kept only until the next chunk: the batch's W need not fit)."""
        last = None
        for b0 in range(0, phi.shape[0], self.chunk):
            last = self.wigner(phi[b0:b0 + self.chunk])
        return last

    def mean(self, phi):
        total = None
        for b0 in range(0, phi.shape[0], self.chunk):
            s = self.wigner(phi[b0:b0 + self.chunk]).sum(0)
            total = s if total is None else total + s
        return total / phi.shape[0]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--loop_batch", type=int, default=65536)
    ap.add_argument("--momenta", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=1024, help="envs per chunk of the yardstick")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wigner_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_wigner: no GPU (nothing is measured on the CPU)")
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.wigner import WignerView

    view = WignerView(None, np.linspace(-12, 12, args.momenta))
    X, P = view.x_n, view.p_n
    i = np.arange(X)
    flop_env = float(4 * np.minimum(i, X - 1 - i).sum() * P)
    yard = Yardstick(view, args.chunk)
    result = {"device": torch.cuda.get_device_name(0), "points": X, "momenta": P, "rounds": args.rounds,
              "timer": "device events around back-to-back calls, the view's and the yardstick's alternating",
              "peak_fp64_tflops": PEAK_FP64_TFLOPS, "flop_model": "sum_i 4 K_i P per env", "flop_per_env": flop_env,
              "yardstick_chunk": args.chunk, "batches": {}}
    for B in list(args.batches) + [args.loop_batch]:
        loop_only = B == args.loop_batch and B not in args.batches
        iters = args.iters if B <= 4096 else 2
        gen = torch.Generator(device="cuda").manual_seed(B)
        phi = torch.randn(B, X, dtype=torch.complex128, device="cuda", generator=gen)
        phi /= (phi.abs().pow(2).sum(1, keepdim=True) * view.h).sqrt()
        calls = {}
        if not loop_only:
            calls["wigner"] = lambda: view.wigner(phi)
            calls["yardstick_wigner"] = lambda: yard.each(phi)
        calls["mean_wigner"] = lambda: view.mean_wigner(phi)
        calls["yardstick_mean"] = lambda: yard.mean(phi)
        # the two routes compute the same thing
        entry = {"batch": B, "iters_per_timing": iters,
                 "max_abs_diff_mean_vs_yardstick": (calls["mean_wigner"]()[0] - calls["yardstick_mean"]()).abs().max().item()}
        if not loop_only:
            n = min(B, args.chunk)
            entry["max_abs_diff_wigner_vs_yardstick"] = (view.wigner(phi[:n]) - yard.wigner(phi[:n])).abs().max().item()
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, fn in calls.items():
                times[k].append(timed(fn, iters))
        for k, ms in times.items():
            entry[k] = summary(ms)
            if not k.startswith("yardstick"):
                tf = flop_env * B / (statistics.median(ms) * 1e-3) / 1e12
                entry[k]["achieved_fp64_tflops"] = round(tf, 3)
                entry[k]["share_of_peak"] = round(tf / PEAK_FP64_TFLOPS, 4)
        pairs = [("mean_wigner", "yardstick_mean")] + ([] if loop_only else [("wigner", "yardstick_wigner")])
        for ours, theirs in pairs:
            entry[ours]["yardstick_over_view"] = round(entry[theirs]["median_ms"] / entry[ours]["median_ms"], 3)
        m, y = entry["mean_wigner"], entry["yardstick_mean"]
        m["not_slower_than_yardstick_beyond_both_spreads"] = \
            m["median_ms"] <= y["median_ms"] + (y["max_ms"] - y["min_ms"]) + (m["max_ms"] - m["min_ms"])
        result["batches"][str(B)] = entry
        print(json.dumps({k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "ms"})
                          for k, v in entry.items()}), flush=True)
        del phi
        torch.cuda.empty_cache()
    view.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
