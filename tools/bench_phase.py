#!/usr/bin/env python3
"""Times the phase-space view of density matrices (WignerView.wigner_of) against torch's own route on one GPU, in one
session, on the same tensors:

    yardstick   an index gather of the anti-diagonals rho[i + k][i - k] into [M, X, K + 1] (the indices and the mask of
                the lags past K_i are built once outside the timing), `matmul` against the complex table
                w_k e^{-2 i p_j k h} [K + 1, P] (w_0 = 1/2), then .real and the scale 2 / pi; for Fock-basis input the
                change of basis h (Phi @ rho @ Phi^T) in complex128 before it

at the drivers' sizes, the QO grid (171 points), the IQO grid (521) and Fock n = 71 and n = 181 on the drivers' 250
points, with M in {1, 21} matrices and P in {128, 193} momenta. Each round times, in this order and with device events
around back-to-back calls, every call of the entry once, so the sides alternate and share whatever else the machine is
doing. These are call times (launches and the output's allocation included), not profiler kernel times. Reported per
entry: the rounds' times per call (ms), their median, min and max; for Fock the change of basis
(SpatialView.density_matrix_of) and the contraction (wigner_of of sigma on a grid view) separately too; for
information the useful operations sum_i 4 K_i P per matrix against the 78.6 TF/s fp64 matrix peak, and `wigner` of
B = M wavefunctions. The outputs are compared once before timing. Writes one JSON file.

    python tools/bench_phase.py --out profiles/phase_bench.json
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
    """torch's route on a grid of X points with the spacing h and the momenta p."""

    def __init__(self, X, h, p):
        K = (X - 1) // 2
        i = torch.arange(X, device="cuda")[:, None]
        k = torch.arange(K + 1, device="cuda")[None, :]
        live = k <= torch.minimum(i, X - 1 - i)
        self.rows = torch.where(live, i + k, 0)
        self.cols = torch.where(live, i - k, 0)
        self.live = live
        ang = 2 * h * k.reshape(-1, 1).to(torch.float64) * p[None, :]
        w = torch.ones(K + 1, 1, dtype=torch.float64, device="cuda")
        w[0] = 0.5
        self.table = torch.complex(w * torch.cos(ang), -w * torch.sin(ang))

    def __call__(self, rho):
        L = rho[:, self.rows, self.cols]
        L = torch.where(self.live, L, torch.zeros((), dtype=L.dtype, device=L.device))
        return (L @ self.table).real * (2 / torch.pi)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_phase: no GPU (nothing is measured on the CPU)")
    import numpy as np
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import config as cfg
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.wigner import WignerView

    D = cfg.DEFAULTS
    systems = (("QO", D[cfg.QO]), ("IQO", D[cfg.IQO]), ("HO", D[cfg.HO]), ("IHO", D[cfg.IHO]))
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "timer": "device events around back-to-back calls, the entry's calls alternating; call times, not "
                       "profiler kernel times",
              "peak_fp64_tflops": PEAK_FP64_TFLOPS,
              "flop_model": "sum_i 4 K_i P real operations per matrix (the contraction alone)",
              "entries": []}
    for name, ph in systems:
        for P in (128, 193):
            p = np.linspace(-12, 12, P)
            view = WignerView.for_physics(ph, p)
            X, n = view.x_n, ph.dim
            gridv = WignerView(view.x, p) if ph.fock else view
            yard_w = Yardstick(X, view.h, view.p)
            Phi = view.spatial.table().to(torch.complex128) if ph.fock else None
            Ki = np.minimum(np.arange(X), X - 1 - np.arange(X))
            for M in (1, 21):
                gen = torch.Generator(device="cuda").manual_seed(1000 * n + 10 * P + M)
                a = torch.randn(M, n, 4, dtype=torch.complex128, device="cuda", generator=gen)
                rho = a @ a.conj().transpose(-1, -2)
                rho = (rho / torch.diagonal(rho, dim1=-2, dim2=-1).real.sum(-1)[:, None, None]).contiguous()
                psi = a[:, :, 0].contiguous()
                psi = psi / torch.linalg.norm(psi, dim=1, keepdim=True) / (1. if ph.fock else view.h ** 0.5)

                def yard():
                    sigma = view.h * (Phi @ rho @ Phi.mT) if ph.fock else rho
                    return yard_w(sigma)

                calls = {"wigner_of": lambda: view.wigner_of(rho), "yardstick": yard,
                         "wigner_of_states": lambda: view.wigner(psi)}
                if ph.fock:
                    sigma = view.spatial.density_matrix_of(rho)
                    calls["congruence"] = lambda: view.spatial.density_matrix_of(rho)
                    calls["contraction"] = lambda: gridv.wigner_of(sigma)
                    calls["yardstick_congruence"] = lambda: view.h * (Phi @ rho @ Phi.mT)
                    calls["yardstick_contraction"] = lambda: yard_w(sigma)
                entry = {"system": name, "x_n": X, "n": n, "fock": bool(ph.fock), "M": M, "P": P,
                         "iters_per_timing": args.iters,
                         "max_abs_diff_vs_yardstick": (calls["wigner_of"]() - yard()).abs().max().item()}
                for fn in calls.values():
                    for _ in range(args.warmup):
                        fn()
                torch.cuda.synchronize()
                times = {k: [] for k in calls}
                for _ in range(args.rounds):
                    for k, fn in calls.items():
                        times[k].append(timed(fn, args.iters))
                for k, ms in times.items():
                    entry[k] = summary(ms)
                m, y = entry["wigner_of"], entry["yardstick"]
                t_flops = 4.0 * float(Ki.sum()) * P * M / (PEAK_FP64_TFLOPS * 1e12) * 1e3
                m["ms_of_useful_flops_at_peak"] = round(t_flops, 7)
                m["share_of_peak"] = round(t_flops / (entry["contraction"] if ph.fock else m)["median_ms"], 5)
                m["yardstick_over_wigner_of"] = round(y["median_ms"] / m["median_ms"], 3)
                m["not_slower_than_yardstick_beyond_both_spreads"] = \
                    m["median_ms"] <= y["median_ms"] + (y["max_ms"] - y["min_ms"]) + (m["max_ms"] - m["min_ms"])
                result["entries"].append(entry)
                print(json.dumps({k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "ms"})
                                  for k, v in entry.items()}), flush=True)
                del rho, a, psi
            if gridv is not view:
                gridv.close()
            view.close()
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
