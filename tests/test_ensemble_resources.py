"""The ensemble kernels' code objects (csrc/qcart_ensemble.hip), read on the CPU from the compiler's resource metadata
inside the built libqcart.so (tools/kernel_resources.py), in the manner of tests/test_wigner_resources.py: k_ensemble,
k_ensemble_count and k_ensemble_finish are each present exactly once, use no scratch and spill nothing; k_ensemble stays
within the 256 registers of two waves per SIMD (the 4 x 2 x {Re, Im} f64 MFMA accumulator tiles are 128 of them), the
other two within 128."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deepreinforcementlearningcontrolofquantumcartpoles_amd", "libqcart.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))

MFMA_KERNELS = ("10k_ensembleE",)
OTHER_KERNELS = ("16k_ensemble_countE", "17k_ensemble_finishE")


def test_ensemble_kernels_use_no_scratch_and_do_not_spill():
    if not os.path.exists(LIB):
        pytest.skip("libqcart.so not built")
    import kernel_resources as K
    rows = [(name, int(v), int(s), int(scr), int(sp), int(ssp)) for name, v, s, scr, sp, ssp in K.kernels(LIB)
            if "k_ensemble" in name]
    for kernel in MFMA_KERNELS + OTHER_KERNELS:
        # (the function's length-prefixed name inside the mangled symbol)
        found = [r for r in rows if kernel in r[0]]
        assert len(found) == 1, (kernel, rows)
        _, vgpr, sgpr, scratch, vspill, sspill = found[0]
        assert (scratch, vspill, sspill) == (0, 0, 0), found
        assert vgpr <= (256 if kernel in MFMA_KERNELS else 128), found
    assert len(rows) == len(MFMA_KERNELS + OTHER_KERNELS), rows
