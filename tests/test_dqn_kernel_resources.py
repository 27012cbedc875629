"""Register, spill, scratch and LDS budgets of every instantiation of the two fused DQN forward kernels, k_actor_act
<W2C> (qcart_actor.hip) and k_learner_fwd <W2C, HIN> (qcart_learner.hip), read on the CPU from the code objects
inside the built libqcart.so (tools/kernel_resources.py, as tests/test_kernel_resources.py does for the step
kernels). W2C is fc2's width, 256 or 512, plus 1 (qcart_dqn.hpp kChunkTag) for the chunked form: inputs above 512
floats, fc1 over X0 in chunks with four output tiles per wave held in registers across the chunks.

All of them run one wave per SIMD (256 threads, one workgroup per CU: their LDS plan leaves room for no second), so
the register file allows 512 VGPRs; the budget is no VGPR or SGPR spill and no scratch. The chunked instantiations
must be present and stay inside the same budget, and inside the same LDS: the dynamic plan the host asks for
(qcart_dqn.hpp kActLdsBytes, qcart_learner.hpp kLdsFloats) plus whatever the kernel declares itself stays within
the CU's 160 KiB.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deepreinforcementlearningcontrolofquantumcartpoles_amd", "libqcart.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))

ACT = re.compile(r"11k_actor_actILi(\d+)EE")
FWD = re.compile(r"13k_learner_fwdILi(\d+)ELb([01])EE")
LDS_CU = 160 * 1024
# the dynamic LDS of a launch: RA and RB [512][32] fp32 each, RC [16][64] (qcart_dqn.hpp kActLdsFloats); the learner's
# forward adds R32 [128][32] (qcart_learner.hpp kLdsFloats)
ACT_LDS = (2 * 512 * 32 + 16 * 64) * 4
FWD_LDS = ACT_LDS + 128 * 32 * 4

# (W2C) and (W2C, HIN): the shipped instantiations; 257 / 513 are the chunked forms of 256 / 512
ACT_WANT = {(256,), (512,), (257,), (513,)}
FWD_WANT = {(256, 0), (512, 0), (256, 1), (257, 0), (513, 0)}


@pytest.fixture(scope="module")
def dqn_kernels():
    if not os.path.exists(LIB):
        pytest.skip("libqcart.so not built")
    import kernel_resources as K
    lds = dict(K.static_lds(LIB))
    act, fwd = {}, {}
    for name, v, s, scr, sp, ssp in K.kernels(LIB):
        row = (int(v), int(s), int(scr), int(sp), int(ssp), int(lds[name]))
        for pat, table in ((ACT, act), (FWD, fwd)):
            m = pat.search(name)
            if m:
                table[tuple(int(g) for g in m.groups())] = row
    return act, fwd


def test_every_instantiation_is_present(dqn_kernels):
    act, fwd = dqn_kernels
    assert set(act) == ACT_WANT, sorted(act)
    assert set(fwd) == FWD_WANT, sorted(fwd)


def test_chunked_instantiations_are_present(dqn_kernels):
    act, fwd = dqn_kernels
    assert {k for k in act if k[0] & 1} == {(257,), (513,)}
    assert {k for k in fwd if k[0] & 1} == {(257, 0), (513, 0)}


def test_no_spills_no_scratch_and_lds_within_the_cu(dqn_kernels):
    act, fwd = dqn_kernels
    assert act and fwd
    bad = []
    for what, table, dyn in (("k_actor_act", act, ACT_LDS), ("k_learner_fwd", fwd, FWD_LDS)):
        for k, (v, s, scr, sp, ssp, static) in sorted(table.items()):
            print(f"{what}{k}: vgpr {v} sgpr {s} scratch {scr} vgpr_spill {sp} sgpr_spill {ssp} "
                  f"lds {static} + {dyn} B")
            if sp or ssp or scr or v > 512 or static + dyn > LDS_CU:
                bad.append((what, k, v, s, scr, sp, ssp, static + dyn))
    assert not bad, bad
