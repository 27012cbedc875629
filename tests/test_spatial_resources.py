"""The position-space kernels' code objects (csrc/qcart_spatial.hip), read on the CPU from the compiler's resource
metadata inside the built libqcart.so (tools/kernel_resources.py), in the manner of tests/test_monitor_resources.py:
k_spatial_repr, k_spatial_probability and k_spatial_mean are present, use no scratch and spill nothing (the 2 x 4 x 2
f64 MFMA accumulator tiles are 128 registers of a wave's 512), and so are the grid-mode kernels and the mean's second
stage."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deepreinforcementlearningcontrolofquantumcartpoles_amd", "libqcart.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))

MFMA_KERNELS = ("k_spatial_repr", "k_spatial_probability", "k_spatial_mean")
OTHER_KERNELS = ("k_spatial_grid_probability", "k_spatial_grid_mean", "k_spatial_finish")


def test_spatial_kernels_use_no_scratch_and_do_not_spill():
    if not os.path.exists(LIB):
        pytest.skip("libqcart.so not built")
    import kernel_resources as K
    rows = [(name, int(v), int(s), int(scr), int(sp), int(ssp)) for name, v, s, scr, sp, ssp in K.kernels(LIB)
            if "k_spatial_" in name]
    for kernel in MFMA_KERNELS + OTHER_KERNELS:
        found = [r for r in rows if re_name(kernel, r[0])]
        assert len(found) == 1, (kernel, rows)
        _, vgpr, sgpr, scratch, vspill, sspill = found[0]
        assert (scratch, vspill, sspill) == (0, 0, 0), found
        # a 256-thread workgroup is one wave per SIMD: up to 512 registers each
        assert vgpr <= (512 if kernel in MFMA_KERNELS else 128), found
    assert len(rows) == len(MFMA_KERNELS + OTHER_KERNELS), rows


def re_name(kernel: str, mangled: str) -> bool:
    """`kernel` is the function's whole name inside the mangled symbol (its length prefix precedes it)."""
    return f"{len(kernel)}{kernel}E" in mangled
