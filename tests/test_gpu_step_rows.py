"""The step kernel (k_step of csrc/qcart_kernels.hpp) at every <family, rows per lane, precision> instantiation on
states that fill every lane, against the oracle, and the fp32 kernels' step bookkeeping bitwise.

Parity: one ragged size per instantiation (tests/step_rows_ref.py: percontrol_ref.CASES, 19 fp64 and 6 fp32), a batch
of 7, injected noise, a force slot of its own per env; per state set (tail, edge, lane-boundary sweep, flat) one call
of 1 step and one call of 8 steps from the same states, with q, x_mean, the Fail step and the fused observation,
against OracleSystem.run_batch on the same states widened to complex128. tests/test_step_rows_cpu.py shows that the
oracle is within 1e-12 of the dense restatement on these states, that none of them sits at the Fail threshold, and that
they see a lost lane halo at every boundary, a dropped row or lane and a shifted table row by 1000 x the bars below.
(Calls of up to 10 steps on a small batch read their tables from L2, MODE 0; the LDS placements run in the bitwise
tests below, which hold MODE 0 to the parity bar against them.)

fp64 bars: psi 1e-11 in the weighted 2-norm (test_psi_parity_every_rows_per_lane's), compared past a Fail too (these
states Fail by construction; within 8 steps both sides compute the same arithmetic); x_mean 1e-9 and q 1e-7
(run_pair's) times max(1, sum |t_i|) of <x> on the state the step starts from (percontrol_ref.Sum: a flat or edge
state makes the terms of <x> large); the Fail step exact. The fused observation after a step is held to the standalone
kernel on the stored state within the moments' own bar (rtol 1e-10, atol 1e-11): on the Fock families for every
state, on the grids for the tail states (a few-row or flat grid state has order-5 moments that vanish while their
terms reach h^-5, tests/test_gpu_percontrol.py).

fp32 bars: complex64 states; psi within F32_FACTOR[case] x r32, where r32 is the largest distance over the case's
states between the fp32 restatement of the step (step_rows_ref.step at float32: fp32 rounding alone, computed on the
CPU, never from the kernel) and the oracle; x_mean, q and the five fused observables the same factor on their own
r32; the Fail step exact. The factor is the project's 8 (KIND2_BAR's margin over a measured rounding figure: the
kernel's band factorisation and parallel scan sum in another order than the restatement's sequential solve).
Measured on an MI355X, the kernel's largest distance over r32, after 1 step / 8 steps: iho401_R8_f32 0.45 / 1.73,
iho701_R16_f32 0.84 / 1.16, iho1500_R32_f32 0.87 / 0.40, ho201_R4_f32 0.77 / 0.60, ho401_R8_f32 0.80 / 1.19,
ho600_R32_f32 1.03 / 0.96; x_mean and q at most 1.42, an observable at most 3.03 times its own r32: no case needs
more than the 8. (After one step r32 is 2.4e-7 to 7.2e-7; after eight the states with weight on the top Fock
levels have amplified it to 1.6e-6 .. 4.1e-4, the kernel's error alike.) fp64: at most 1.4e-15 after one step on any
state of any case, 1.4e-13 after eight.

Other envs' rows: the 7 flat states in another env order give every env's rows, q, x_mean and Fail step bitwise.

fp32 bookkeeping, bitwise (the fp64 bitwise tests of tests/test_gpu_parity.py do not reach the fp32 body: per-step
normalisation, no frozen-env skip, its own table placement by size): step budgets, split calls and the counter, batch
composition and sharding, table placements; from the flat and tail states tiled over the batch.
"""
from functools import lru_cache

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from deepreinforcementlearningcontrolofquantumcartpoles_amd.core import Stepper  # noqa: E402
from tests import percontrol_ref as PR  # noqa: E402
from tests import step_rows_ref as SR  # noqa: E402
from tests.step_rows_ref import BY_ID, F32_IDS, IDS, KINDS, STEPS  # noqa: E402

B = SR.BATCH
F32_FACTOR = {case: SR.F32_FACTOR for case in F32_IDS}


@lru_cache(maxsize=None)
def handle(case, batch=B, seed=1234, env_offset=0):
    ph = BY_ID[case][1]
    st = Stepper(ph, batch, 0, seed=seed, env_offset=env_offset)
    assert st.N == ph.dim and st.state_dtype == (torch.complex64 if ph.precision == 1 else torch.complex128)
    return st


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_call(st, states, acts, noise, idx, n):
    """The states idx stepped n steps in batches of B (the last one padded): psi, q, x_mean, fail, obs per state, and
    the standalone observation kernel on the stored result."""
    out = {"psi": [], "q": [], "xm": [], "fail": [], "obs": [], "obs_alone": []}
    for m, c in SR.chunks(idx):
        psi = dev(states[c])
        res = st.step(psi, dev(acts[c]), n, noise=dev(noise[:n, c]), want_q=True, want_fail=True, want_obs=True)
        alone = st.moments(psi)
        out["psi"].append(psi.cpu().numpy()[:m])
        out["q"].append(res["q"].cpu().numpy()[:, :m])
        out["xm"].append(res["x_mean"].cpu().numpy()[:, :m])
        out["fail"].append(res["fail_step"].cpu().numpy()[:m])
        out["obs"].append(res["obs"].cpu().numpy()[:m])
        out["obs_alone"].append(alone.cpu().numpy()[:m])
    return {k: np.concatenate(v, axis=1 if k in ("q", "xm") else 0) for k, v in out.items()}


@pytest.mark.parametrize("case", IDS)
def test_step_parity_on_states_that_fill_every_lane(oracle_mod, case):
    ph = BY_ID[case][1]
    st = handle(case)
    f32 = ph.precision == 1
    for n in STEPS:
        r = SR.r32(oracle_mod, case, n) if f32 else None
        fac = F32_FACTOR.get(case)
        worst = {}
        for kind in KINDS:
            states, acts, noise = SR.plan(case, kind)
            k = SR.kept(case, kind, n)
            o = SR.oracle_run(oracle_mod, case, kind)
            got = gpu_call(st, states, acts, noise, k, n)
            assert got["psi"].dtype == PR.state_dtype(ph)
            d = SR.wnorm(ph, got["psi"].astype(np.complex128) - o.psi[n][k])
            dx, dq = np.abs(got["xm"] - o.xm[n][:, k]), np.abs(got["q"] - o.q[n][:, k])
            if f32:
                dob = np.abs(got["obs"] - o.obs[n][k]).max(axis=0)
                worst[kind] = (d.max(), d.max() / r.by_kind[kind])
                print(f"{case} {kind} {n} steps: |dpsi| {d.max():.2e} = {d.max() / r.psi:.2f} x r32 {r.psi:.2e} "
                      f"({d.max() / r.by_kind[kind]:.2f} x this set's {r.by_kind[kind]:.2e}); x_mean "
                      f"{dx.max() / r.xm:.2f} x {r.xm:.2e}; q {dq.max() / r.q:.2f} x {r.q:.2e}; obs "
                      f"{(dob / r.obs).max():.2f} x {r.obs}")
                assert d.max() <= fac * r.psi, (kind, n, int(k[d.argmax()]), d.max(), r.psi)
                assert dx.max() <= fac * r.xm and dq.max() <= fac * r.q, (kind, n, dx.max(), r.xm, dq.max(), r.q)
                assert (dob <= fac * r.obs).all(), (kind, n, dob, r.obs)
            else:
                print(f"{case} {kind} {n} steps: |dpsi| {d.max():.2e}")
                assert d.max() <= SR.PSI_BAR_FP64, (kind, n, int(k[d.argmax()]), d.max())
                scale = o.x_scale(n)[:, k]
                assert (dx <= 1e-9 * scale).all() and (dq <= 1e-7 * scale).all(), (kind, n, (dx / scale).max(),
                                                                                   (dq / scale).max())
                if ph.fock or kind == "tail":
                    bar = np.stack([PR.moment_bar(m, ph.moment_order) for m in got["obs_alone"]])
                    assert (np.abs(got["obs"] - got["obs_alone"]) <= bar).all(), (kind, n)
            assert np.array_equal(got["fail"], o.fail[n][k]), (kind, n, got["fail"], o.fail[n][k])


@pytest.mark.parametrize("case", IDS)
def test_other_envs_rows_are_bitwise_unchanged(case):
    st = handle(case)
    states, acts, noise = SR.plan(case, "flat")
    perm = np.roll(np.arange(B), 3)
    n = max(STEPS)
    a = gpu_call(st, states, acts, noise, np.arange(B), n)
    b = gpu_call(st, states, acts, noise, perm, n)
    def raw(x):
        return np.ascontiguousarray(x).view(np.uint8)

    assert np.array_equal(raw(b["psi"]), raw(a["psi"][perm]))
    for key in ("q", "xm"):
        assert np.array_equal(raw(b[key]), raw(a[key][:, perm])), key
    assert np.array_equal(b["fail"], a["fail"][perm]) and np.array_equal(raw(b["obs"]), raw(a["obs"][perm]))


# ---- fp32 step bookkeeping, bitwise -----------------------------------------------------------------------------
def tiled(case, batch):
    """The flat and the tail states tiled over the batch."""
    s = SR.state_sets(case)
    both = np.concatenate([s["flat"], s["tail"]])
    return dev(both[np.arange(batch) % len(both)])


def bits(t):
    """Bit patterns (a NaN equals itself)."""
    return torch.view_as_real(t).contiguous().view(torch.int32) if t.is_complex() else t


def same(a, b):
    return torch.equal(bits(a), bits(b))


def actions(batch, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 21, (batch,), generator=g, device="cuda", dtype=torch.int32)


@pytest.mark.parametrize("case", F32_IDS)
def test_fp32_step_budgets_bitwise(case):
    """Budgets of 0, 40 and 80 steps in rotation with per-env actions: frozen envs bitwise untouched (the fp32 kernel
    has no frozen-env skip), partial-budget envs equal a 40-step call, full-budget envs an unbudgeted call; the Fail
    step of a frozen env is 0."""
    batch = 100
    st = handle(case, batch, 21)
    psi0 = tiled(case, batch)
    acts = actions(batch, 4)
    budget = torch.tensor([[0, 40, 80][i % 3] for i in range(batch)], dtype=torch.int32, device="cuda")
    st.step_counter = 0
    a = psi0.clone()
    out = st.step(a, acts, 80, env_steps=budget, want_fail=True)
    st.step_counter = 0
    full = psi0.clone()
    st.step(full, acts, 80)
    st.step_counter = 0
    part = psi0.clone()
    st.step(part, acts, 40)
    bz = budget.cpu().numpy()
    for e in range(batch):
        want = {0: psi0, 40: part, 80: full}[int(bz[e])]
        assert same(a[e], want[e]), e
    assert not same(part, full) and not same(part, psi0)
    assert int(out["fail_step"][budget == 0].abs().sum()) == 0


def _split_runs(case):
    """(200 steps, 120 + 80 steps, the state after the 120, handle, actions) of in-kernel Philox from counter 0."""
    batch = 14
    st = handle(case, batch, 5)
    psi0 = tiled(case, batch)
    acts = actions(batch, 6)
    st.step_counter = 0
    a = psi0.clone()
    st.step(a, acts, 200)
    assert st.step_counter == 200
    st.step_counter = 0
    b = psi0.clone()
    st.step(b, acts, 120)
    mid = b.clone()
    assert st.step_counter == 120
    st.step(b, acts, 80)
    assert st.step_counter == 200 and (st.env_counters() == 200).all()
    return a, b, mid, st, acts, psi0


@pytest.mark.parametrize("case", F32_IDS)
def test_fp32_repeat_from_counter_bitwise(case):
    """A repeat from step_counter = 0 is bitwise the same, and so is a second call repeated from the first call's
    state with the counter set to where that call left it."""
    a, b, mid, st, acts, psi0 = _split_runs(case)
    st.step_counter = 0
    c = psi0.clone()
    st.step(c, acts, 200)
    assert same(a, c)
    st.step_counter = 120
    d = mid.clone()
    st.step(d, acts, 80)
    assert same(b, d)


@pytest.mark.parametrize("case", F32_IDS)
def test_fp32_second_call_continues_the_noise_stream(oracle_mod, case):
    """1 + 1 steps of in-kernel Philox equal 2 steps, and the test can tell: with the first step's draw repeated in
    the second call psi moves by about sqrt(gamma dt), 0.05 and more, over 100 times the one-step parity bar."""
    ph = BY_ID[case][1]
    batch = 14
    st = handle(case, batch, 5)
    psi0 = tiled(case, batch)
    acts = actions(batch, 6)
    st.step_counter = 0
    a = psi0.clone()
    st.step(a, acts, 2)
    st.step_counter = 0
    b = psi0.clone()
    st.step(b, acts, 1)
    st.step(b, acts, 1)
    assert st.step_counter == 2
    st.step_counter = 1          # the same draw twice instead
    c = psi0.clone()
    st.step(c, acts, 1)
    st.step_counter = 1
    st.step(c, acts, 1)
    d = SR.wnorm(ph, (a - b).cpu().numpy())
    wrong = SR.wnorm(ph, (a - c).cpu().numpy())
    bar = F32_FACTOR[case] * SR.r32(oracle_mod, case, 1).psi
    print(f"{case}: 1 + 1 against 2 steps {d.max():.2e} (bar {bar:.2e}); with a repeated draw {np.median(wrong):.2e}")
    assert same(a, b)
    assert np.median(wrong) > 100 * bar


@pytest.mark.parametrize("case", F32_IDS)
def test_fp32_split_calls_bitwise(case):
    """120 + 80 steps of in-kernel Philox equal 200 steps bitwise. The fp32 step forms X psi and <x> at the head of
    every step from the rounded psi that the step before stored or would have stored, the first step of a call and
    a later one by the same expressions (the fp64 kernel carries them from the normalisation's reduction inside a
    call and is held to 1e-13 instead, test_gpu_parity.test_split_calls_equal_and_deterministic). Before that, the
    fp32 kernel carried them too, one float32 rounding away from a call's first step, and from these top-heavy
    states 80 further steps amplified the rounding to 5.5e-5 (N = 201) .. 0.61."""
    a, b, *_ = _split_runs(case)
    print(f"{case}: 120 + 80 against 200 steps: max |dpsi_r| {float((a - b).abs().max()):.2e}")
    assert same(a, b)


@pytest.mark.parametrize("case", F32_IDS)
def test_fp32_batch_composition_and_sharding_bitwise(case):
    """Env 5 of a 37-env handle equals the same env alone in a 1-env handle with env_offset = 5; 1 handle x 8 envs
    equals 2 handles x 4 envs with env_offset."""
    st = handle(case, 37, 11)
    psi0 = tiled(case, 37)
    acts = actions(37, 7)
    st.step_counter = 0
    x = psi0.clone()
    st.step(x, acts, 40)
    one = handle(case, 1, 11, 5)
    one.step_counter = 0
    y = psi0[5:6].clone()
    one.step(y, acts[5:6].contiguous(), 40)
    assert same(y[0], x[5])
    full, s0, s1 = handle(case, 8, 3), handle(case, 4, 3, 0), handle(case, 4, 3, 4)
    a = psi0[:8].clone()
    b0, b1 = a[:4].clone(), a[4:].clone()
    for h in (full, s0, s1):
        h.step_counter = 0
    full.step(a, acts[:8].contiguous(), 100)
    s0.step(b0, acts[:4].contiguous(), 100)
    s1.step(b1, acts[4:8].contiguous(), 100)
    assert same(a, torch.cat([b0, b1]))


def native_tab_mode(case, st):
    """base_args' placement of an fp32 Fock handle (csrc/qcart_api.cpp; the C ABI does not report it): MODE 2 when
    the slot image with 4 scan levels per direction fits 160 KiB and no slot needs more levels, else MODE 1 when the
    image without composites fits, else MODE 0. QCART_TAB_MODE caps it."""
    _, ph, R = BY_ID[case]
    kl, es, lanes = PR.KL[ph.family], 8, 64
    tf = 2 * es * lanes * kl * R + es * lanes * R + (es // 2 * lanes * 10 * R if ph.family == SR.IHO else 0)
    t2 = tf + (2 * 4 + 2) * kl * kl * lanes * es
    lv = [st.scan_levels(a) for a in range(ph.n_actions)]
    fits2 = t2 <= 160 * 1024 and max(f for f, _ in lv) <= 4 and max(b for _, b in lv) <= 4
    return 2 if fits2 else (1 if tf <= 160 * 1024 else 0)


def test_fp32_cases_reach_both_lds_placements():
    """QCART_TAB_MODE is a cap: a handle that cannot reach a mode passes the placement test trivially. By size the
    R = 32 inverted-oscillator handle runs MODE 1 and the smaller ones MODE 2, so every case runs MODE 1 under the
    cap of 1 and at least one runs MODE 2."""
    native = {case: native_tab_mode(case, handle(case, 37, 11)) for case in F32_IDS}
    assert native["iho1500_R32_f32"] == 1, native
    assert 2 in native.values() and min(native.values()) >= 1, native


@pytest.mark.parametrize("case", F32_IDS)
def test_fp32_table_placements(oracle_mod, monkeypatch, case):
    """QCART_TAB_MODE = 2, 1 and 0 on 37 envs of mixed force slots over 40 steps: the two LDS placements are
    bit-identical (the fp32 translation unit is built with -ffp-contract=on and every placement runs the same source
    expressions), and the L2 placement is within the fp32 parity bar of them."""
    ph = BY_ID[case][1]
    st = handle(case, 37, 11)
    psi0 = tiled(case, 37)
    acts = actions(37, 7)
    outs = []
    for mode in ("2", "1", "0"):
        monkeypatch.setenv("QCART_TAB_MODE", mode)
        st.step_counter = 0
        x = psi0.clone()
        st.step(x, acts, 40)
        outs.append(x)
    torch.cuda.synchronize()
    assert same(outs[0], outs[1])
    d = SR.wnorm(ph, (outs[0] - outs[2]).cpu().numpy())
    print(f"{case}: MODE 0 against MODE 2 after 40 steps: {d.max():.2e}")
    assert d.max() <= F32_FACTOR[case] * SR.r32(oracle_mod, case, max(STEPS)).psi
