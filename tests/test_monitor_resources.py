"""The monitor kernel's code object (csrc/qcart_monitor.hip), read on the CPU from the compiler's resource metadata
inside the built libqcart.so (tools/kernel_resources.py), in the manner of tests/test_sched_resources.py: the kernel
is present, uses no scratch and spills nothing (the table is indexed in global memory, the ring entries go through
LDS)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deepreinforcementlearningcontrolofquantumcartpoles_amd", "libqcart.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_monitor_kernel_uses_no_scratch_and_does_not_spill():
    if not os.path.exists(LIB):
        pytest.skip("libqcart.so not built")
    import kernel_resources as K
    found = {name: (int(v), int(s), int(scr), int(sp), int(ssp))
             for name, v, s, scr, sp, ssp in K.kernels(LIB) if "k_monitor_receive" in name}
    assert len(found) == 1, found
    (vgpr, sgpr, scratch, vspill, sspill), = found.values()
    assert (scratch, vspill, sspill) == (0, 0, 0), found
    assert vgpr <= 128, found          # one wave, far from the register file's limit
