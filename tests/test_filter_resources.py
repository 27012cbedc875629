"""The conditional master equation's code objects (csrc/qcart_filter.hip), read on the CPU from the compiler's resource
metadata inside the built libqcart.so (tools/kernel_resources.py), in the manner of tests/test_lindblad_resources.py:
k_filter_begin, k_filter_draw, k_filter_apply and k_filter_restore are each present exactly once, use no scratch, spill
nothing and stay within 128 registers; the master equation's own six k_lindblad* kernels are still six."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deepreinforcementlearningcontrolofquantumcartpoles_amd", "libqcart.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("14k_filter_beginE", "13k_filter_drawE", "14k_filter_applyE", "16k_filter_restoreE")


def test_filter_kernels_use_no_scratch_and_do_not_spill():
    if not os.path.exists(LIB):
        pytest.skip("libqcart.so not built")
    import kernel_resources as K
    every = [(name, int(v), int(s), int(scr), int(sp), int(ssp)) for name, v, s, scr, sp, ssp in K.kernels(LIB)]
    rows = [r for r in every if "k_filter" in r[0]]
    for kernel in KERNELS:
        # (the function's length-prefixed name inside the mangled symbol)
        found = [r for r in rows if kernel in r[0]]
        assert len(found) == 1, (kernel, rows)
        _, vgpr, sgpr, scratch, vspill, sspill = found[0]
        assert (scratch, vspill, sspill) == (0, 0, 0), found
        assert vgpr <= 128, found
    assert len(rows) == len(KERNELS), rows
    assert len([r for r in every if "k_lindblad" in r[0]]) == 6
