"""Scratch / spill budgets of the measurement learner's kernels (csrc/qcart_mlearner.hip, and the tail entries of
k_learner_fwd / k_learner_bwd in csrc/qcart_learner.hip), read on the CPU from the compiler's resource metadata
inside the built libqcart.so (tools/kernel_resources.py), in the manner of tests/test_learner_resources.py: every
new kernel is present, uses no scratch, spills no VGPR or SGPR and stays within 512 VGPRs."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deepreinforcementlearningcontrolofquantumcartpoles_amd", "libqcart.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))

# substrings of the mangled names; ILi256ELb1EE: the <256, true> instantiations (the measurement tail)
KERNELS = ("k_mlearner_states", "k_mlearner_fc1t", "k_mlearner_reduce", "k_mlearner_prep",
           "k_mlearner_convtILi64ELi64ELi9ELi4EE", "k_mlearner_convtILi32ELi64ELi11ELi4EE",
           "k_mlearner_convdwILi64ELi64ELi9ELi4EE", "k_mlearner_convdwILi32ELi64ELi11ELi4EE",
           "k_mlearner_convdwILi2ELi32ELi13ELi5EE", "k_learner_fwdILi256ELb1EE", "k_learner_bwdILi256ELb1EE")


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB):
        pytest.skip("libqcart.so not built")
    import kernel_resources as K
    out = {}
    for name, v, s, scr, sp, ssp in K.kernels(LIB):
        for k in KERNELS:
            if k in name:
                out[k] = (int(v), int(s), int(scr), int(sp), int(ssp))
    return out


def test_every_new_kernel_is_present(kernels):
    assert set(kernels) == set(KERNELS)


def test_no_scratch_no_spills_and_vgprs_within_budget(kernels):
    bad = {k: r for k, r in kernels.items() if r[2] != 0 or r[3] != 0 or r[4] != 0 or r[0] > 512}
    assert not bad, f"(vgpr, sgpr, scratch bytes, vgpr spills, sgpr spills) over budget: {bad}"
