#!/usr/bin/env python3
"""Times the ensemble density matrix (ensemble.EnsembleView.density_matrix) against torch's own route on one GPU, in one
session, on the same states and mask:

    yardstick_einsum   live = psi[mask] (no gather when every env is live), then
                       torch.einsum('bm,bn->mn', live, live.conj()) * scale / len(live): what a user writes today
    yardstick_matmul   the same with (live.mH @ live).T, one conjugate-transposing complex GEMM without a materialised
                       conjugate: the best torch route found

at (N, B) = (181, 4096), (513, 65 536) and (171, 4096), each with all envs live and with about half masked. Each round
times, in this order and with device events around back-to-back calls, the view's call and then the yardsticks', so the
sides alternate and share whatever else the machine is doing. These are call times (launches, the output's allocation
and, for the yardstick's gather, its synchronisation included), not profiler kernel times. Reported per entry: the
rounds' times per call (ms), their median, min and max; for the view the achieved fp64 rate counting the useful
operations 8 N (N + 1) / 2 count against the 78.6 TF/s matrix peak. The outputs are compared once before timing.
Writes one JSON file.

    python tools/bench_ensemble.py --out profiles/ensemble_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP64_TFLOPS = 78.6
SIZES = ((181, 4096, 1.0), (513, 65536, 0.05), (171, 4096, 0.1))      # (N, B, scale)


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


def yardstick_einsum(psi, mask, scale):
    live = psi if mask is None else psi[mask]
    return torch.einsum("bm,bn->mn", live, live.conj()) * scale / live.shape[0]


def yardstick_matmul(psi, mask, scale):
    live = psi if mask is None else psi[mask]
    return (live.mH @ live).T * scale / live.shape[0]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble: no GPU (nothing is measured on the CPU)")
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import _lib
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.ensemble import EnsembleView

    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "timer": "device events around back-to-back calls, the view's and the yardsticks' alternating; call "
                       "times, not profiler kernel times",
              "peak_fp64_tflops": PEAK_FP64_TFLOPS, "flop_model": "8 N (N + 1) / 2 count", "entries": []}
    for N, B, scale in SIZES:
        view = EnsembleView(N, scale)
        iters = args.iters if B <= 4096 else 2
        gen = torch.Generator(device="cuda").manual_seed(B + N)
        psi = torch.randn(B, N, dtype=torch.complex128, device="cuda", generator=gen)
        psi /= (psi.abs().pow(2).sum(1, keepdim=True) * scale).sqrt()
        half = torch.rand(B, device="cuda", generator=gen) < 0.5
        for name, mask in (("all live", None), ("about half masked", half)):
            count = B if mask is None else int(mask.sum())
            calls = {"density_matrix": lambda: view.density_matrix(psi, mask),
                     "yardstick_einsum": lambda: yardstick_einsum(psi, mask, scale),
                     "yardstick_matmul": lambda: yardstick_matmul(psi, mask, scale)}
            rho = calls["density_matrix"]()[0]
            entry = {"N": N, "batch": B, "mask": name, "count": count, "scale": scale,
                     "splits": _lib.lib().qc_ensemble_splits(B, N), "iters_per_timing": iters,
                     "max_abs_diff_vs_einsum": (rho - calls["yardstick_einsum"]()).abs().max().item(),
                     "max_abs_diff_vs_matmul": (rho - calls["yardstick_matmul"]()).abs().max().item()}
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
            m = entry["density_matrix"]
            tf = 8.0 * N * (N + 1) / 2 * count / (m["median_ms"] * 1e-3) / 1e12
            m["useful_fp64_tflops"] = round(tf, 3)
            m["share_of_peak"] = round(tf / PEAK_FP64_TFLOPS, 4)
            best = min(("yardstick_einsum", "yardstick_matmul"), key=lambda k: entry[k]["median_ms"])
            y = entry[best]
            m["best_yardstick"] = best
            m["yardstick_over_view"] = round(y["median_ms"] / m["median_ms"], 3)
            m["not_slower_than_yardstick_beyond_both_spreads"] = \
                m["median_ms"] <= y["median_ms"] + (y["max_ms"] - y["min_ms"]) + (m["max_ms"] - m["min_ms"])
            result["entries"].append(entry)
            print(json.dumps({k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "ms"})
                              for k, v in entry.items()}), flush=True)
        view.close()
        del psi
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
