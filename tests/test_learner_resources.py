"""Scratch / spill budgets of the DQN learner's kernels (csrc/qcart_learner.hip), read on the CPU from the
compiler's resource metadata inside the built libqcart.so (tools/kernel_resources.py), in the manner of
tests/test_kernel_resources.py: every learner kernel is present, uses no scratch and spills no VGPR; the two
MFMA kernels that hold their activations in LDS stay within one workgroup's register budget (256 threads)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deepreinforcementlearningcontrolofquantumcartpoles_amd", "libqcart.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("k_learner_noise", "k_learner_fwd", "k_learner_loss", "k_learner_bwd", "k_learner_dw", "k_learner_wndot",
           "k_learner_opt", "k_learner_prep")


@pytest.fixture(scope="module")
def learner_kernels():
    if not os.path.exists(LIB):
        pytest.skip("libqcart.so not built")
    import kernel_resources as K
    out = {}
    for name, v, s, scr, sp, ssp in K.kernels(LIB):
        for k in KERNELS:
            if k in name:
                out[k] = (int(v), int(s), int(scr), int(sp), int(ssp))
    return out


def test_every_learner_kernel_is_present(learner_kernels):
    assert set(learner_kernels) == set(KERNELS)


def test_learner_kernels_use_no_scratch_and_do_not_spill(learner_kernels):
    bad = {k: r for k, r in learner_kernels.items() if r[2] != 0 or r[3] != 0 or r[4] != 0}
    assert not bad, f"(vgpr, sgpr, scratch bytes, vgpr spills, sgpr spills) over budget: {bad}"


def test_learner_mfma_kernels_fit_one_wave_per_simd(learner_kernels):
    for k in ("k_learner_fwd", "k_learner_bwd", "k_learner_dw"):
        assert learner_kernels[k][0] <= 512, (k, learner_kernels[k])
