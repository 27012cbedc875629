#!/usr/bin/env python3
"""Cost of a step-kernel workgroup boundary from the boundary stamps build
(make expt EXPT=-DQCART_BSTAMPS NAME=bstamps; run with QCART_LIB=<pkg>/libqcart_bstamps.so; with
-DQCART_PAIR_BALANCE=0 beside it: the hardware's own arbitration between the two waves of a SIMD).

Every wave that ran a tile left four s_memtime values (entry, loop begin, loop end, exit) and its hardware id in a
record of its own (qcart_expt.hpp). Printed, in shader cycles: per wave entry -> loop, the loop, loop end -> exit;
per CU the gap between the last exit of one tile's waves and the first entry of the next tile's; per wave index
of the workgroup and per SIMD how far apart the waves of one tile finish. The stamps add four scalar clock reads and
six stores per wave and fence nothing inside the loop.

  diag_boundaries.py [config=metric] [batch] [n_steps]
"""
import ctypes
import os
import sys

import numpy as np

MAX_WAVES = 1 << 17


def analyse(buf, W):
    """buf: uint64 [n][8] records (t_entry, t_loop, t_loop_end, t_exit, xcc << 32 | HW_ID, workgroup, -, -), record
    t * W + w = wave w of tile t, all-zero records = waves that ran nothing. Returns a dict of arrays (cycles)."""
    buf = np.asarray(buf)
    used = buf[:, 0] != 0
    r = buf[used].astype(np.int64)
    widx = np.nonzero(used)[0]
    t0, t1, t2, t3 = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    hw, xcc = r[:, 4] & 0xFFFFFFFF, r[:, 4] >> 32
    # HW_ID: wave [3:0], SIMD [5:4], pipe [7:6], CU [11:8], SH [12], SE [15:13]
    simd, cu, sh, se = (hw >> 4) & 0x3, (hw >> 8) & 0xF, (hw >> 12) & 0x1, (hw >> 13) & 0x7
    cuid = ((xcc * 8 + se) * 2 + sh) * 16 + cu
    tile, wave = widx // W, widx % W
    o = np.lexsort((t0, tile))
    tl, first = np.unique(tile[o], return_index=True)
    t_in = np.minimum.reduceat(t0[o], first)
    t_out = np.maximum.reduceat(t3[o], first)
    t_out_first = np.minimum.reduceat(t3[o], first)
    t_cu = cuid[o][first]
    gaps, spans, tiles_per_cu, busy = [], [], [], []
    for c in np.unique(t_cu):
        m = t_cu == c
        k = np.argsort(t_in[m])
        a, b = t_in[m][k], t_out[m][k]
        tiles_per_cu.append(len(a))
        gaps.extend((a[1:] - b[:-1]).tolist())          # last exit -> the CU's next tile's first entry
        spans.extend((a[1:] - a[:-1]).tolist())         # a tile's slot on its CU: entry -> the next tile's entry
        busy.append(b[-1] - a[0])
    # per (tile, SIMD): the cycles with fewer waves on the SIMD than the tile put there (exit of its last wave
    # minus exit of its first)
    key = tile * 4 + simd
    ko = np.lexsort((t3, key))
    _, kf, kc = np.unique(key[ko], return_index=True, return_counts=True)
    pair = kc >= 2
    simd_skew = (np.maximum.reduceat(t3[ko], kf) - np.minimum.reduceat(t3[ko], kf))[pair]
    in_of_wave = t_in[np.searchsorted(tl, tile)]
    return dict(n_waves=len(r), n_tiles=len(tl), n_cus=len(np.unique(cuid)), n_wgs=len(np.unique(r[:, 5])),
                entry=t1 - t0, loop=t2 - t1, exit=t3 - t2, tile_len=t_out - t_in, tile_skew=t_out - t_out_first,
                gaps=np.asarray(gaps, dtype=np.int64), spans=np.asarray(spans, dtype=np.int64),
                tiles_per_cu=np.asarray(tiles_per_cu), busy=np.asarray(busy), simd_skew=simd_skew,
                waves_per_simd=kc, wave=wave, simd=simd, exit_at=t3 - in_of_wave, launch=t_out.max() - t_in.min())


def dist(name, v, ref=None):
    v = np.asarray(v, dtype=np.float64)
    if v.size == 0:
        print(f"  {name:26s} (none)")
        return 0.0
    q = np.percentile(v, [5, 50, 95])
    share = f"  {100 * v.mean() / ref:5.2f} % of a tile's slot" if ref else ""
    print(f"  {name:26s} mean {v.mean():9.0f}  p5 {q[0]:9.0f}  median {q[1]:9.0f}  p95 {q[2]:9.0f}  max {v.max():9.0f}"
          f"{share}")
    return float(v.mean())


def report(s, W):
    slot = float(s["spans"].mean()) if s["spans"].size else float(s["tile_len"].mean())
    print(f"  {s['n_waves']} stamped waves, {s['n_tiles']} tiles, {s['n_cus']} CUs, {s['n_wgs']} workgroups; tiles per CU "
          f"{s['tiles_per_cu'].min()}..{s['tiles_per_cu'].max()}; a CU's first entry -> last exit: mean "
          f"{s['busy'].mean():.0f}, max {s['busy'].max()} cycles")
    print(f"  a tile's slot on its CU (entry -> the CU's next tile's entry): mean {slot:.0f} cycles")
    print("per wave:")
    e = dist("entry -> loop", s["entry"], slot)
    dist("loop", s["loop"], slot)
    x = dist("loop end -> exit", s["exit"], slot)
    print("per tile:")
    dist("first entry -> last exit", s["tile_len"], slot)
    dist("last exit - first exit", s["tile_skew"], slot)
    g = dist("gap to the CU's next tile", s["gaps"], slot)
    print(f"  outside the loop per slot: entry {e:.0f} + exit {x:.0f} + gap {g:.0f} = {e + x + g:.0f} cycles = "
          f"{100 * (e + x + g) / slot:.2f} % of the slot")
    print("per wave index of the workgroup (SIMD it ran on; loop cycles; exit after the tile's first entry):")
    for w in range(W):
        m = s["wave"] == w
        if not m.any():
            continue
        sim = np.bincount(s["simd"][m], minlength=4)
        print(f"  wave {w}: SIMD {int(sim.argmax())} ({100 * sim.max() / m.sum():3.0f} %)  loop mean {s['loop'][m].mean():9.0f}"
              f"  exit at mean {s['exit_at'][m].mean():9.0f}")
    print(f"per tile and SIMD ({np.bincount(s['waves_per_simd']).tolist()} SIMDs by wave count):")
    dist("last exit - first exit", s["simd_skew"], slot)


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    from deepreinforcementlearningcontrolofquantumcartpoles_amd import _lib
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import config as cfg
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.core import Stepper

    name = sys.argv[1] if len(sys.argv) > 1 else "metric"
    conf = cfg.BENCH_CONFIGS[name]
    ph = conf["physics"]
    B = int(sys.argv[2]) if len(sys.argv) > 2 else conf["batch"]
    n_steps = int(sys.argv[3]) if len(sys.argv) > 3 else ph.control_interval
    st = Stepper(ph, B, 0, seed=42)
    psi = st.new_state()
    if ph.fock:
        st.reset(psi, 1, arg0=16)
    else:
        st.reset(psi, 2, arg0=0.0, arg1=0.0, arg2=1.0)
    g = torch.Generator(device="cpu").manual_seed(7)
    acts = [torch.randint(0, ph.n_actions, (B,), generator=g, dtype=torch.int32).cuda() for _ in range(3)]
    f = _lib.lib().qc_debug_bstamps
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint]
    buf = np.zeros((MAX_WAVES, 8), dtype=np.uint64)

    def run(a):
        st.step(psi, a, n_steps, want_fail=True, want_obs=True)
        torch.cuda.synchronize()
        if f(buf.ctypes.data_as(ctypes.c_void_p), MAX_WAVES) != 0:
            sys.exit("qc_debug_bstamps failed")

    run(acts[0])   # warm-up (code object load, first touch of the tables)
    run(acts[1])
    run(acts[2])   # the reported launch
    W = int(_lib.lib().qc_step_group_size(st._h))   # waves (envs) per tile
    print(f"{name}: family {ph.family} N={ph.dim} B={B} n_steps={n_steps}, {W} waves per tile "
          f"({os.path.basename(_lib.LIB_PATH)})")
    report(analyse(buf, W), W)


if __name__ == "__main__":
    main()
