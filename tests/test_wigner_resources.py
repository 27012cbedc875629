"""The phase-space kernels' code objects (csrc/qcart_wigner.hip), read on the CPU from the compiler's resource metadata
inside the built libqcart.so (tools/kernel_resources.py), in the manner of tests/test_spatial_resources.py: k_wigner and
both k_wigner_mean instantiations are present, use no scratch and spill nothing within the 256 registers of two waves
per SIMD (the 4 x 4 f64 MFMA accumulator tiles are 128 of them), and so are the count and the mean's second stage."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deepreinforcementlearningcontrolofquantumcartpoles_amd", "libqcart.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))

MFMA_KERNELS = ("8k_wignerE", "13k_wigner_meanILi1EE", "13k_wigner_meanILi2EE")
OTHER_KERNELS = ("14k_wigner_countE", "15k_wigner_finishE")


def test_wigner_kernels_use_no_scratch_and_do_not_spill():
    if not os.path.exists(LIB):
        pytest.skip("libqcart.so not built")
    import kernel_resources as K
    rows = [(name, int(v), int(s), int(scr), int(sp), int(ssp)) for name, v, s, scr, sp, ssp in K.kernels(LIB)
            if "k_wigner" in name]
    for kernel in MFMA_KERNELS + OTHER_KERNELS:
        # (the function's length-prefixed name inside the mangled symbol)
        found = [r for r in rows if kernel in r[0]]
        assert len(found) == 1, (kernel, rows)
        _, vgpr, sgpr, scratch, vspill, sspill = found[0]
        assert (scratch, vspill, sspill) == (0, 0, 0), found
        assert vgpr <= (256 if kernel in MFMA_KERNELS else 128), found
    assert len(rows) == len(MFMA_KERNELS + OTHER_KERNELS), rows
