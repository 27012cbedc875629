"""The code objects of the phase-space view of density matrices (csrc/qcart_phase.hip), read on the CPU from the
compiler's resource metadata inside the built libqcart.so (tools/kernel_resources.py), in the manner of
tests/test_lindblad_resources.py: k_phase_wigner, k_phase_left, k_phase_right and the one-tile variants k_phase_left16
and k_phase_right16 are each present exactly once, use no scratch and spill nothing, and stay within 256 registers
(k_phase_wigner runs two waves per SIMD: its 4 x 4 f64 accumulator tiles are 128 of them)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deepreinforcementlearningcontrolofquantumcartpoles_amd", "libqcart.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))

MFMA_KERNELS = ("14k_phase_wignerE", "12k_phase_leftE", "13k_phase_rightE", "14k_phase_left16E", "15k_phase_right16E")


def test_phase_kernels_use_no_scratch_and_do_not_spill():
    if not os.path.exists(LIB):
        pytest.skip("libqcart.so not built")
    import kernel_resources as K
    rows = [(name, int(v), int(s), int(scr), int(sp), int(ssp)) for name, v, s, scr, sp, ssp in K.kernels(LIB)
            if "k_phase" in name]
    for kernel in MFMA_KERNELS:
        # (the function's length-prefixed name inside the mangled symbol)
        found = [r for r in rows if kernel in r[0]]
        assert len(found) == 1, (kernel, rows)
        _, vgpr, sgpr, scratch, vspill, sspill = found[0]
        assert (scratch, vspill, sspill) == (0, 0, 0), found
        assert vgpr <= 256, found
    assert len(rows) == len(MFMA_KERNELS), rows

