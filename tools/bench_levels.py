#!/usr/bin/env python3
"""Times the energy-level view (levels.LevelView.populations and .mean_populations) against torch's own route on one
GPU, in one session, on the same states, table and mask:

    yardstick_complex   psi @ V.T.to(complex128) (the table's conversion included), then abs() ** 2
    yardstick_real      torch.view_as_real(psi) as [B, N, 2], contracted with V over N by a real matmul (the permuting
                        copies included), then re^2 + im^2
    for the mean        the faster of the two on the gather psi[mask] (no gather when every env is live), then .mean(0)

each times scale^2, at K = 32 and (N, B) = (171, 4096), (171, 65 536), (1025, 16 384), and at K = 64 and (171, 65 536),
each with all envs live and with about half masked (a mask does not change `populations`: it is measured once per size).
Each round times, in this order and with device events around back-to-back calls, the view's call and then the
yardsticks', so the sides alternate and share whatever else the machine is doing. These are call times (launches, the
output's allocation and, for the yardstick's gather, its synchronisation included), not profiler kernel times. Reported
per entry: the rounds' times per call (ms), their median, min and max; for the view the time against psi's bytes
(16 B N) over 8 TB/s and the useful operations 4 B N K against the 78.6 TF/s fp64 matrix peak, and which of the two
bounds is the larger at that size. The outputs are compared once before timing. Writes one JSON file.

    python tools/bench_levels.py --out profiles/levels_bench.json
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
PEAK_HBM_TBS = 8.0
SIZES = ((171, 4096, 32), (171, 65536, 32), (1025, 16384, 32), (171, 65536, 64))      # (N, B, K)


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


def pops_complex(psi, V, scale):
    return (psi @ V.T.to(torch.complex128)).abs() ** 2 * (scale * scale)


def pops_real(psi, V, scale):
    a = torch.view_as_real(psi).permute(0, 2, 1) @ V.T           # [B, 2, K]
    return (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) * (scale * scale)


def mean_of(pops, psi, V, scale, mask):
    live = psi if mask is None else psi[mask]
    return pops(live, V, scale).mean(0)


def compare(entry, view_key, yard_keys):
    m = entry[view_key]
    best = min(yard_keys, key=lambda k: entry[k]["median_ms"])
    y = entry[best]
    m["best_yardstick"] = best
    m["yardstick_over_view"] = round(y["median_ms"] / m["median_ms"], 3)
    m["not_slower_than_yardstick_beyond_both_spreads"] = \
        m["median_ms"] <= y["median_ms"] + (y["max_ms"] - y["min_ms"]) + (m["max_ms"] - m["min_ms"])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "levels_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_levels: no GPU (nothing is measured on the CPU)")
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.levels import LevelView

    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "timer": "device events around back-to-back calls, the view's and the yardsticks' alternating; call "
                       "times, not profiler kernel times",
              "peak_fp64_tflops": PEAK_FP64_TFLOPS, "peak_hbm_tb_per_s": PEAK_HBM_TBS,
              "flop_model": "4 B N K (live envs only for the mean)", "byte_model": "16 B N (live envs only for the mean)",
              "entries": []}
    for N, B, K in SIZES:
        scale = 0.1 ** 0.5
        gen = torch.Generator(device="cuda").manual_seed(B + N + K)
        V = torch.randn(K, N, dtype=torch.float64, device="cuda", generator=gen)
        V /= V.norm(dim=1, keepdim=True)
        view = LevelView(V.cpu(), scale)
        iters = args.iters if B * N <= 4096 * 1025 else 3
        psi = torch.randn(B, N, dtype=torch.complex128, device="cuda", generator=gen)
        psi /= psi.abs().pow(2).sum(1, keepdim=True).sqrt()
        half = torch.rand(B, device="cuda", generator=gen) < 0.5
        for name, mask in (("all live", None), ("about half masked", half)):
            count = B if mask is None else int(mask.sum())
            calls = {"mean_populations": lambda: view.mean_populations(psi, mask),
                     "mean_yardstick_complex": lambda: mean_of(pops_complex, psi, V, scale, mask),
                     "mean_yardstick_real": lambda: mean_of(pops_real, psi, V, scale, mask)}
            if mask is None:
                calls.update({"populations": lambda: view.populations(psi),
                              "yardstick_complex": lambda: pops_complex(psi, V, scale),
                              "yardstick_real": lambda: pops_real(psi, V, scale)})
            entry = {"N": N, "batch": B, "K": K, "mask": name, "count": count, "scale": scale,
                     "iters_per_timing": iters,
                     "mean_max_abs_diff_vs_complex":
                         (calls["mean_populations"]()[0] - calls["mean_yardstick_complex"]()).abs().max().item()}
            if mask is None:
                entry["max_abs_diff_vs_complex"] = \
                    (calls["populations"]() - calls["yardstick_complex"]()).abs().max().item()
                entry["max_abs_diff_vs_real"] = (calls["populations"]() - calls["yardstick_real"]()).abs().max().item()
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
            for key, envs in (("mean_populations", count), ("populations", B)):
                if key not in entry:
                    continue
                m = entry[key]
                t_bytes = 16.0 * envs * N / (PEAK_HBM_TBS * 1e12) * 1e3
                t_flops = 4.0 * envs * N * K / (PEAK_FP64_TFLOPS * 1e12) * 1e3
                m["ms_of_psi_bytes_at_peak"] = round(t_bytes, 5)
                m["ms_of_useful_flops_at_peak"] = round(t_flops, 5)
                m["larger_bound"] = "psi bytes" if t_bytes >= t_flops else "matrix pipe"
                m["share_of_larger_bound"] = round(max(t_bytes, t_flops) / m["median_ms"], 4)
            compare(entry, "mean_populations", ("mean_yardstick_complex", "mean_yardstick_real"))
            if mask is None:
                compare(entry, "populations", ("yardstick_complex", "yardstick_real"))
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
