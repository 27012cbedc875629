"""The step kernel's pair balance (kPairBalance, qcart_kernels.hpp: the two waves of a SIMD trade issue priority by
their step index, through LDS words above the slot image) changes no result: the IHO and HO N = 512 kernels (R = 8)
track the oracle with all eight waves of a workgroup stepping, and an env's trajectory, Fail step, q / x_mean and
noise counter are bitwise the same whatever its SIMD partner does — stepping beside it, out of budget early, frozen,
or idle."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from deepreinforcementlearningcontrolofquantumcartpoles_amd import config as cfg  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd.core import Stepper  # noqa: E402

CASES = {
    "iho512": cfg.DEFAULTS[cfg.IHO].with_(n_max=511),
    "ho512": cfg.DEFAULTS[cfg.HO].with_(n_max=511),
}
# calls of more than 10 steps keep the slot image in LDS (shorter ones on small batches read the tables from L2)
STEPS = 12


def fresh(ph, B, seed):
    st = Stepper(ph, B, 0, seed=seed)
    psi = st.new_state()
    st.reset(psi, 1, arg0=16)
    return st, psi


@pytest.mark.parametrize("case", sorted(CASES))
def test_full_workgroups_track_the_oracle(case):
    """Two full single-slot workgroups (every SIMD holds a stepping pair) and a two-slot one against the oracle, at
    smoke()'s bound for this kernel (1e-10 on psi after 80 steps; here 30)."""
    from oracle import oracle as O
    ph = CASES[case]
    B, steps = 24, 30
    acts = np.array([3] * 12 + [17] * 12, np.int32)   # tiles: 8 x slot 3, 4 + 4 (two slots), 8 x slot 17
    st, psi = fresh(ph, B, 42)
    ref = psi.cpu().numpy().copy()
    st.step(psi, torch.from_numpy(acts).cuda(), steps)
    torch.cuda.synchronize()
    s = O.OracleSystem(ph.family, n_max=ph.n_max, omega=ph.omega)
    s.run_batch(ref, acts, ph.f_max, steps, ph.dt, ph.gamma, seed=42, n_threads=4)
    err = float(np.abs(psi.cpu().numpy() - ref).max())
    print(f"{case}: max|dpsi| = {err:.3e}")
    assert err < 1e-10


@pytest.mark.parametrize("case", sorted(CASES))
def test_results_do_not_depend_on_the_simd_partner(case):
    """45 envs on three slots (full tiles, two-slot tiles and a partial last tile), budgets 3 / 7 / 12 mixed: one call
    on all envs against two calls that freeze every other env (the stepping envs are regrouped, so every wave gets
    another partner or none). Bitwise equal per env."""
    ph = CASES[case]
    B = 45
    rng = np.random.default_rng(11)
    acts_np = rng.permutation(np.concatenate([np.full(19, 4), np.full(17, 9), np.full(9, 15)]).astype(np.int32))
    budget_np = rng.choice(np.array([3, 7, STEPS], np.int32), B)
    acts, budget = torch.from_numpy(acts_np).cuda(), torch.from_numpy(budget_np).cuda()
    even = (torch.arange(B, device="cuda") % 2) == 0

    st, psi_a = fresh(ph, B, 9)
    out_a = st.step(psi_a, acts, STEPS, env_steps=budget, want_q=True, want_fail=True)
    torch.cuda.synchronize()
    ctr_a = st.env_counters()

    st, psi_b = fresh(ph, B, 9)
    zero = torch.zeros_like(budget)
    outs = []
    for half in (even, ~even):
        before = psi_b.clone()
        outs.append(st.step(psi_b, acts, STEPS, env_steps=torch.where(half, budget, zero), want_q=True, want_fail=True))
        torch.cuda.synchronize()
        assert torch.equal(psi_b[~half], before[~half])   # a frozen env's psi bytes stay
    ctr_b = st.env_counters()

    assert torch.equal(psi_a, psi_b)
    assert torch.equal(ctr_a, ctr_b) and torch.equal(ctr_a.cpu(), torch.from_numpy(budget_np.astype(np.int64)))
    ran = torch.arange(STEPS, device="cuda")[:, None] < budget[None, :]   # rows past an env's budget are not written
    for half, out_b in zip((even, ~even), outs):
        m = ran & half[None, :]
        for name in ("q", "x_mean"):
            assert torch.equal(out_a[name][m], out_b[name][m]), name
        assert torch.equal(out_a["fail_step"][half], out_b["fail_step"][half])
