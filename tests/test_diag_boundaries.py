"""tools/diag_boundaries.py's reader on synthetic boundary-stamp records (no GPU): the per-wave phases, the per-CU gap
between one tile's last exit and the next tile's first entry, and the per-SIMD exit skew come out as constructed,
and waves that ran nothing (all-zero records) are left out."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import diag_boundaries as D  # noqa: E402

W = 8


def hw_word(xcc, se, sh, cu, simd, wave=0):
    return (xcc << 32) | (se << 13) | (sh << 12) | (cu << 8) | (simd << 4) | wave


def records():
    """Two CUs (same CU number on two XCDs). CU A runs tiles 0 and 2, CU B tiles 1 and 3; tile 3 has 5 waves.
    Wave w of a tile: entry at T + w, loop from +100 to +1100 (waves 0-3) or +1600 (waves 4-7), exit 10 later."""
    buf = np.zeros((6 * W, 8), dtype=np.uint64)   # tiles 4 and 5 ran nothing
    start = {0: 1000, 2: 1000 + 1610 + 7 + 50, 1: 5000, 3: 5000 + 1610 + 7 + 20}
    cu_of = {0: (0, 1, 0, 3), 2: (0, 1, 0, 3), 1: (5, 1, 0, 3), 3: (5, 1, 0, 3)}
    for t, T in start.items():
        for w in range(W if t != 3 else 5):
            e = T + w
            end = e + 100 + (1000 if w < 4 else 1500)
            buf[t * W + w] = (e, e + 100, end, end + 10, hw_word(*cu_of[t], simd=w % 4, wave=w), t, 0, 0)
    return buf


def test_phases_gaps_and_simd_skew():
    s = D.analyse(records(), W)
    assert s["n_waves"] == 3 * W + 5 and s["n_tiles"] == 4 and s["n_cus"] == 2 and s["n_wgs"] == 4
    assert (s["entry"] == 100).all() and (s["exit"] == 10).all()
    assert sorted(set(s["loop"].tolist())) == [1000, 1500]
    assert s["tiles_per_cu"].tolist() == [2, 2]
    # last exit of tile 0: wave 7 at 1000 + 7 + 1610; tile 2 enters 50 later (tile 3: 20 after tile 1)
    assert sorted(s["gaps"].tolist()) == [20, 50]
    assert sorted(s["spans"].tolist()) == [1610 + 7 + 20, 1610 + 7 + 50]
    # full tiles: waves w and w + 4 share a SIMD and exit 504 apart; tile 3 has one such pair (waves 0 and 4)
    assert s["simd_skew"].tolist().count(504) == 3 * 4 + 1 and len(s["simd_skew"]) == 13
    assert np.bincount(s["waves_per_simd"]).tolist() == [0, 3, 13]
    assert (s["tile_skew"][:3] == 507).all()
    # a wave's exit relative to its tile's first entry
    assert s["exit_at"][(s["wave"] == 7)].tolist() == [7 + 1610] * 3


def test_report_prints_the_outside_loop_share(capsys):
    D.report(D.analyse(records(), W), W)
    out = capsys.readouterr().out
    slot = (1610 + 7 + 20 + 1610 + 7 + 50) / 2
    assert f"= {100 * (100 + 10 + 35) / slot:.2f} % of the slot" in out
    assert "wave 7: SIMD 3 (100 %)" in out
