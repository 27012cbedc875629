"""The conditional master equation on the device (csrc/qcart_filter.hip, MasterEquation.evolve_conditional; DESIGN
§9n): one and several steps against the longdouble restatement (tests/filter_ref.py) with injected draws inside the
a-priori elementwise bound, the record, the Philox stream against the host mirror, batch independence / first_step /
filtering mode by bit pattern, the matrices that cannot be stepped, the physics (the mean over 4096 records is the
unconditional scheme within five standard errors; a filter on the step kernels' own record follows their state), the
baseline controllers on rho against the env's, Trainer.filtered_loop and train --filtered_out, and the refusals."""
import ctypes
import hashlib
import math

import numpy as np
import pytest
import torch

from tests import filter_ref as F
from tests import lindblad_ref as R
from tests.checkpoint_loop import same_bits

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
LD, CLD = F.LD, F.CLD


def _pkg():
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import _lib
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import config as cfg
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.core import make_params
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.lindblad import MasterEquation
    return locals()


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def host(t):
    return t.cpu().numpy()


def sha(t):
    return hashlib.sha256(host(t).tobytes()).hexdigest()


def random_rho(N, M, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((M, N, 3)) + 1j * rng.standard_normal((M, N, 3))
    a[:, N - N // 4:, :] = 0                           # (nothing at the edge)
    rho = a @ a.conj().transpose(0, 2, 1)
    rho = (rho + rho.conj().transpose(0, 2, 1)) / 2
    return rho / np.trace(rho, axis1=1, axis2=2).real[:, None, None]


def assert_hermitian_bits(y):
    re, im = y.real, y.imag
    assert same_bits(re, np.ascontiguousarray(np.swapaxes(re, -1, -2)))
    off = ~np.eye(y.shape[-1], dtype=bool)
    flipped = np.ascontiguousarray(np.swapaxes(im, -1, -2)).view(np.uint64) ^ np.uint64(1 << 63)
    assert np.array_equal(im.view(np.uint64)[..., off], flipped[..., off])
    d = np.ascontiguousarray(np.diagonal(im, axis1=-2, axis2=-1))
    assert not d.view(np.uint64).any()


def physics(cfg, name):
    D = cfg.DEFAULTS
    if name.startswith("HO"):
        return D[cfg.HO].with_(n_max=int(name[2:]) - 1)
    return {"IHO16": D[cfg.IHO].with_(n_max=15), "QO17": D[cfg.QO].with_(x_max=1.0, grid_size=0.125),
            "IQO261": D[cfg.IQO].with_(x_max=6.5), "IQO521": D[cfg.IQO]}[name]


_SETUPS = {}


@pytest.fixture(scope="module", autouse=True)
def close_handles():
    yield
    for s in _SETUPS.values():
        s["me"].close()
    _SETUPS.clear()


def setup(name):
    """Per case, once: the handle (forces 0 and F_max / 2), the device's own tables of slot 1 and the longdouble xi."""
    if name not in _SETUPS:
        P = _pkg()
        ph = physics(P["cfg"], name)
        me = P["MasterEquation"](ph, forces=[0.0, ph.f_max / 2])
        tab = P["MasterEquation"].tables(ph, ph.f_max / 2)
        xi_ld = R.xi_longdouble(tab["W"], R.operators(ph)[1]) if ph.fock else tab["xi"].astype(LD)
        _SETUPS[name] = dict(P=P, ph=ph, me=me, tab=tab, xi_ld=xi_ld)
    return _SETUPS[name]


def efficiency(s, eta):
    """Sets eta on the handle; (a in longdouble, the library's own G^(1-eta) table or None)."""
    s["me"].set_efficiency(eta)
    assert s["me"].eta == eta
    a, _ = F.constants(eta, s["ph"].gamma, s["ph"].dt)
    if eta == 1.0:
        return a, None
    P, ph = s["P"], s["ph"]
    g = np.zeros((ph.dim, ph.dim))
    assert P["_lib"].lib().qc_lindblad_efficiency_table(ctypes.byref(P["make_params"](ph, 1)), ph.dt, ph.gamma, eta,
                                                        ctypes.c_void_p(g.ctypes.data)) == 0
    return a, g


# ---------------------------------------------------------------- 1. steps against the restatement, injected draws
CASES = [("HO5", 21, (1, 8)), ("HO16", 21, (1, 8)), ("HO17", 21, (1, 8)), ("HO33", 21, (1, 8)), ("HO65", 21, (1, 8)),
         ("IHO16", 21, (1, 8)), ("QO17", 21, (1, 8)), ("IQO261", 21, (1, 8)), ("IQO521", 2, (2,))]


@pytest.mark.parametrize("eta", (1.0, 0.5))
@pytest.mark.parametrize("name,M,steps", CASES, ids=[c[0] for c in CASES])
def test_steps_against_the_restatement(name, M, steps, eta):
    s = setup(name)
    ph, me, tab = s["ph"], s["me"], s["tab"]
    N = ph.dim
    a, g = efficiency(s, eta)
    # A longdouble congruence takes 0.3 s at N = 261 and 2.5 s at N = 521. At 261 (the diagonal crosses a chunk) the
    # first two matrices at n = 1 and the first at n = 8 are held to the bound itself against longdouble; the other
    # matrices there, and N = 521, have the same scheme in fp64 as reference, whose own error obeys the same bound, so
    # the device is held to twice the bound.
    def reference(n, m):
        if N <= 65 or (N == 261 and m < (2 if n == 1 else 1)):
            return CLD, 1
        return np.complex128, 2
    rng = np.random.default_rng(1000 + N)
    rho0 = random_rho(N, M, 600 + N)
    xi_max = float(np.abs(tab["xi"]).max())
    for n in steps:
        draws = np.stack([rng.random((n, M)), rng.standard_normal((n, M))], axis=2)
        rho = dev(rho0)
        out, y = me.evolve_conditional(rho, n, 1, draws=dev(draws), want_record=True)
        assert out is rho
        got, y = host(rho), host(y)
        me.take_errors()
        worst = worst_y = worst_ld = 0.0
        for m in range(M):
            dtype, slack = reference(n, m)
            want = F.evolve(rho0[m], n, tab, g, a, ph.fock, draws=draws[:, m], dtype=dtype)
            assert want["margin"].min() >= 1e-9, (name, n, m)       # no draw sits on a rounding tie: none is left out
            tol_y = (N + 8) * EPS * (xi_max + np.abs(want["y"]).astype(np.float64))
            err_y = np.abs(y[:, m].astype(LD) - want["y"]).astype(np.float64)
            assert np.all(err_y <= tol_y), (name, n, m)
            worst_y = max(worst_y, float((err_y / tol_y).max()))
            err = np.maximum(np.abs(got[m].real.astype(LD) - want["rho"].real),
                             np.abs(got[m].imag.astype(LD) - want["rho"].imag)).astype(np.float64)
            bound = slack * want["bound"]
            assert np.all(err <= bound), (name, n, m, float((err / np.maximum(bound, 1e-300)).max()))
            some = bound > 0
            worst = max(worst, float((err[some] / bound[some]).max()))
            if slack == 1:
                worst_ld = max(worst_ld, float((err[some] / bound[some]).max()))
            assert abs(float(np.trace(got[m]).real) - 1) <= (4 * N + 16) * EPS * (n + 2)
        print(f"{name} eta = {eta} n = {n}: largest error / bound = {worst:.2e} (against longdouble alone "
              f"{worst_ld:.2e}), record error / tolerance = {worst_y:.2e}")
        assert_hermitian_bits(got)


def test_the_philox_record_is_the_host_mirrors_draws_through_the_restatement():
    s = setup("HO16")
    ph, me, tab = s["ph"], s["me"], s["tab"]
    a, g = efficiency(s, 0.5)
    M, n, seed, first = 3, 4, 20240607, 2 ** 33 + 5
    streams = np.array([7, 0, 2 ** 31 - 1], dtype=np.int32)
    rho0 = random_rho(16, M, 77)
    rho = dev(rho0)
    _, y = me.evolve_conditional(rho, n, 1, seed=seed, streams=dev(streams), first_step=first, want_record=True)
    y, got = host(y), host(rho)
    draws = F.philox_draws(s["P"]["_lib"].lib(), seed, streams, first, n)
    xi_max = float(np.abs(tab["xi"]).max())
    s_const = float(F.constants(0.5, ph.gamma, ph.dt)[1])
    for m in range(M):
        want = F.evolve(rho0[m], n, tab, g, a, True, draws=draws[:, m])
        assert want["margin"].min() >= 1e-9
        # the record's tolerance, and the mirror's normal within 1e-15 (1 + |z|-ish radius <= 10) of the device's
        tol = (16 + 8) * EPS * (xi_max + np.abs(want["y"]).astype(np.float64)) + 1e-14 * s_const
        assert np.all(np.abs(y[:, m].astype(LD) - want["y"]).astype(np.float64) <= tol)
        assert np.abs(got[m] - want["rho"].astype(np.complex128)).max() <= 1e-11
    # the default streams are 0, 1, 2, ..
    rho = dev(rho0)
    _, y_default = me.evolve_conditional(rho, n, 1, seed=seed, first_step=first, want_record=True)
    assert same_bits(host(y_default)[:, 1], host(me.evolve_conditional(
        dev(rho0[1:2]), n, 1, seed=seed, streams=dev(np.array([1], dtype=np.int32)), first_step=first,
        want_record=True)[1])[:, 0])


# ---------------------------------------------------------------- 2. by bit pattern
@pytest.mark.parametrize("name", ("HO17", "IQO261"))
def test_batch_position_split_calls_and_filtering_by_bit_pattern(name):
    s = setup(name)
    me, N = s["me"], s["ph"].dim
    efficiency(s, 0.5)
    M, n, seed = 21, 8, 99
    rho0 = random_rho(N, M, 900 + N)
    slots = dev((np.arange(M) % 2).astype(np.int32))

    def run(rows, first=0, steps=n, record=None, streams="rows", sl="rows"):
        rho = dev(rho0[rows])
        st = dev(np.asarray(rows, dtype=np.int32)) if streams == "rows" else streams
        out = me.evolve_conditional(rho, steps, slots[torch.as_tensor(rows).cuda()].contiguous() if sl == "rows" else sl,
                                    seed=seed, streams=st, first_step=first, record=record, want_record=True)
        return host(out[0]), host(out[1])

    every = list(range(M))
    full, y = run(every)
    assert np.isfinite(full.view(np.float64)).all() and np.isfinite(y).all()
    assert_hermitian_bits(full)
    for k in (1, 2, 3):                                # prefixes of the batch; the default streams are 0, 1, 2
        r, yk = run(every[:k], streams=None)
        assert same_bits(r, full[:k]) and same_bits(yk, np.ascontiguousarray(y[:, :k]))
    perm = list(np.random.default_rng(5).permutation(M))
    r, yp = run(perm)                                  # where a matrix sits, with its stream
    assert same_bits(r, full[perm]) and same_bits(yp, np.ascontiguousarray(y[:, perm]))
    r, yr = run(every)                                 # a repeat (after smaller batches: stale values behind them)
    assert same_bits(r, full) and same_bits(yr, y)
    few, _ = run(every[:4])                            # ... and a smaller batch after a larger one
    assert same_bits(few, full[:4])
    # one call of 8 steps is two of 4 with first_step
    rho = dev(rho0)
    st = dev(np.arange(M, dtype=np.int32))
    _, ya = me.evolve_conditional(rho, 4, slots, seed=seed, streams=st, want_record=True)
    _, yb = me.evolve_conditional(rho, 4, slots, seed=seed, streams=st, first_step=4, want_record=True)
    # the record depends on sigma through the picked index alone, so it is the same bits either way
    assert same_bits(np.concatenate([host(ya), host(yb)]), y)
    if not s["ph"].fock:
        assert same_bits(host(rho), full)
    else:
        # A Fock rho is taken to sigma and back once per CALL: two calls round W sigma W^T and W^T rho W once more
        # than one call does, so they agree within the two runs' a-priori bounds, not by bit pattern.
        split = host(rho)
        P, ph = s["P"], s["ph"]
        a_ld = F.constants(0.5, ph.gamma, ph.dt)[0]
        g = efficiency(s, 0.5)[1]
        tabs = [P["MasterEquation"].tables(ph, f) for f in me.forces]
        draws = F.philox_draws(P["_lib"].lib(), seed, range(5), 0, n)
        for m in range(5):
            tab = tabs[m % 2]
            one = F.evolve(rho0[m], n, tab, g, a_ld, True, draws=draws[:, m])
            half = F.evolve(rho0[m], 4, tab, g, a_ld, True, draws=draws[:4, m])
            two = F.evolve(half["rho"], 4, tab, g, a_ld, True, draws=draws[4:, m], E0=half["bound"])
            assert min(one["margin"].min(), half["margin"].min(), two["margin"].min()) >= 1e-9
            err = np.maximum(np.abs(split[m].real - full[m].real), np.abs(split[m].imag - full[m].imag))
            both = one["bound"] + two["bound"]
            assert np.all(err <= both), m
            print(f"HO17 matrix {m}: one call against two, largest difference {err.max():.2e}, "
                  f"largest difference / bound {float((err / both).max()):.2e}")
    # n_steps = 0
    rho = dev(rho0)
    before = sha(rho)
    out = me.evolve_conditional(rho, 0, slots, want_record=True)
    assert sha(rho) == before and tuple(out[1].shape) == (0, M)
    # filtering mode fed the record of the sampling run reproduces it
    r, yf = run(every, record=dev(y))
    assert same_bits(r, full) and same_bits(yf, y)
    me.take_errors()


# ---------------------------------------------------------------- 3. matrices that cannot be stepped
def test_bad_inputs_leave_their_matrix_untouched_and_are_reported_once():
    s = setup("QO17")
    P, me, N = s["P"], s["me"], 17
    efficiency(s, 0.5)
    M, n, seed = 6, 5, 4
    rho0 = random_rho(N, M, 31)
    clean = dev(rho0)
    _, y_clean = me.evolve_conditional(clean, n, 1, seed=seed, want_record=True)
    clean, y_clean = host(clean), host(y_clean)
    me.take_errors()

    # sampling: a slot out of range (matrix 1) and a NaN in a diagonal (matrix 3)
    bad = rho0.copy()
    bad[3, 4, 4] = complex(float("nan"), 0.0)
    slots = dev(np.array([1, 7, 1, 1, 1, 1], dtype=np.int32))
    rho = dev(bad)
    hashes = [sha(rho[m]) for m in range(M)]
    _, y = me.evolve_conditional(rho, n, slots, seed=seed, want_record=True)
    for m in (1, 3):
        assert sha(rho[m]) == hashes[m]
        assert np.isnan(host(y)[:, m]).all()
    others = [0, 2, 4, 5]
    assert same_bits(host(rho)[others], clean[others]) and same_bits(host(y)[:, others], y_clean[:, others])
    with pytest.raises(P["_lib"].QCartError) as e:
        me.take_errors()
    assert "a slot out of [0, J)" in str(e.value) and "could not be stepped" in str(e.value)
    me.take_errors()                                   # reported once

    # filtering: a record far outside the support where the state has no weight (matrix 2: Z = 0), a NaN record (4)
    bad = rho0.copy()
    bad[2, N - 1, N - 1] = -0.5                        # (clamped to d = 0: the state has nothing at the last point)
    record = y_clean.copy()
    record[2, 2] = 1e12                                # every other point's weight underflows: Z = w_last^2 * 0
    record[1, 4] = float("nan")
    rho = dev(bad)
    hashes = [sha(rho[m]) for m in range(M)]
    _, y = me.evolve_conditional(rho, n, 1, record=dev(record), want_record=True)
    y = host(y)
    for m, first_bad in ((2, 2), (4, 1)):
        assert sha(rho[m]) == hashes[m]
        assert np.isnan(y[first_bad:, m]).all() and same_bits(y[:first_bad, m], record[:first_bad, m])
    others = [0, 1, 3, 5]
    assert same_bits(host(rho)[others], clean[others]) and same_bits(y[:, others], y_clean[:, others])
    with pytest.raises(P["_lib"].QCartError) as e:
        me.take_errors()
    assert "could not be stepped" in str(e.value) and "a slot out of" not in str(e.value)
    me.take_errors()
    # the plain evolve's own report is unchanged
    me.evolve(dev(rho0), 1, slots)
    with pytest.raises(P["_lib"].QCartError, match="a slot out of") as e:
        me.take_errors()
    assert "could not be stepped" not in str(e.value)


# ---------------------------------------------------------------- 4. exact in expectation
@pytest.mark.parametrize("eta", (1.0, 0.5, 0.1))
def test_the_mean_over_records_is_the_unconditional_scheme(eta):
    P = _pkg()
    cfg = P["cfg"]
    ph = cfg.DEFAULTS[cfg.HO].with_(n_max=15)
    N, M, n = 16, 4096, 10
    me = P["MasterEquation"](ph, forces=[0.0, 2.0])
    try:
        me.set_efficiency(eta)
        tab = P["MasterEquation"].tables(ph, 2.0)
        W = tab["W"]
        rho0 = R.pure(R.trajectory_start(ph))
        rho = dev(np.repeat(rho0[None], M, axis=0))
        _, y = me.evolve_conditional(rho, n, 1, seed=1234 + int(100 * eta), want_record=True)
        # the exact side on the device: (G o T . T^†)^n sigma_0 by the handle's own congruence
        T, gf = dev(tab["T"]), dev(tab["g_full"])
        sigma = dev(W.T @ rho0 @ W)
        xi = tab["xi"]
        mean_y = []
        for _ in range(n):
            mean_y.append(float((xi * np.diagonal(host(me.congruence(T, sigma))).real).sum()))
            sigma = me.congruence(T, sigma, gf)
        exact = W @ host(sigma) @ W.T
        got, y = host(rho), host(y)
        me.take_errors()
    finally:
        me.close()
    mean = got.mean(axis=0)
    purity = (np.abs(got) ** 2).sum(axis=(1, 2))
    se = math.sqrt(max(float(purity.mean()) - float((np.abs(mean) ** 2).sum()), 0.0) / M)
    dev_f = float(np.linalg.norm(mean - exact))
    print(f"eta = {eta}: |mean - exact|_F / standard error = {dev_f / se:.3f}")
    assert dev_f <= 5 * se
    for k in range(n):
        d, sy = abs(float(y[k].mean()) - mean_y[k]), float(y[k].std(ddof=1)) / math.sqrt(M)
        assert d <= 5 * sy, (k, d / sy)
    print(f"eta = {eta}: largest |mean y - Tr(rho X)| / standard error = "
          f"{max(abs(float(y[k].mean()) - mean_y[k]) / (float(y[k].std(ddof=1)) / math.sqrt(M)) for k in range(n)):.3f}")
    if eta == 1.0:
        assert np.abs(purity - 1).max() <= 10 * (4 * N + 16) * EPS * N


# ---------------------------------------------------------------- 5. the Python refusals
def test_python_refusals():
    P = _pkg()
    cfg = P["cfg"]
    ph = cfg.DEFAULTS[cfg.HO].with_(n_max=15)
    me = P["MasterEquation"](ph, forces=[0.0, 1.0])
    quiet = P["MasterEquation"](ph, forces=[0.0], gamma=0.0)
    try:
        good = dev(random_rho(16, 3, 1))
        assert me.eta is None
        with pytest.raises(ValueError, match="the efficiency is not set"):
            me.evolve_conditional(good, 1, 0)
        lib, vp = P["_lib"].lib(), ctypes.c_void_p
        assert lib.qc_lindblad_evolve_conditional(me._h, vp(good.data_ptr()), 3, None, 0, 1, 0, None, 0, None, None,
                                                  None) == -1
        assert b"qc_lindblad_evolve_conditional: the efficiency is not set" in lib.qc_lindblad_last_error(me._h)
        for eta in (0.0, 1.5, float("nan")):
            with pytest.raises(ValueError, match=r"qc_lindblad_set_efficiency: eta must be in \(0, 1\]"):
                me.set_efficiency(eta)
        with pytest.raises(ValueError, match="gamma must be > 0 for a conditional evolution"):
            quiet.set_efficiency(0.5)
        me.set_efficiency(0.25)
        assert me.eta == 0.25
        assert same_bits(host(me.xi), P["MasterEquation"].tables(ph, 0.0)["xi"])
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")   # noqa: E731
        i32 = lambda a: torch.tensor(a, dtype=torch.int32, device="cuda")   # noqa: E731
        for kw, text in ((dict(rho=good.to(torch.complex64)), "must be complex128"),
                         (dict(rho=good.cpu()), "must live on"),
                         (dict(rho=good.transpose(1, 2)), "must be contiguous"),
                         (dict(rho=good[:, :8, :8].contiguous()), r"rho must be \[16, 16\] or \[M, 16, 16\]"),
                         (dict(n_steps=-1), "n_steps must be an int >= 0"),
                         (dict(first_step=-1), "first_step must be an int >= 0"),
                         (dict(seed=-1), "seed must be an int in"),
                         (dict(slots=2), r"slot 2 is outside \[0, 2\)"),
                         (dict(streams=i32([0, 1])), r"streams must be an int32 \[3\] tensor"),
                         (dict(streams=i32([0, 1, 2]).cpu()), "streams must live on"),
                         (dict(draws=f64(2, 3)), r"draws must be a float64 \[2, 3, 2\] tensor"),
                         (dict(draws=f64(2, 3, 2).cpu()), "draws must live on"),
                         (dict(draws=f64(2, 3, 4)[:, :, ::2]), "draws must be contiguous"),
                         (dict(record=f64(3, 3)), r"record must be a float64 \[2, 3\] tensor"),
                         (dict(record=f64(2, 3).to(torch.float32)), r"record must be a float64 \[2, 3\] tensor"),
                         (dict(record=f64(2, 3), draws=f64(2, 3, 2)), "record and draws exclude each other")):
            args = dict(rho=good, n_steps=2, slots=0)
            args.update(kw)
            with pytest.raises(ValueError, match=text):
                me.evolve_conditional(**args)
        assert same_bits(host(good), random_rho(16, 3, 1))                     # nothing was evolved
        with pytest.raises(ValueError, match="analytic_slots needs the physics' own action grid"):
            me.analytic_slots(good)
        me.take_errors()
    finally:
        me.close()
        quiet.close()


# ---------------------------------------------------------------- 6. against the step kernels
def test_the_filter_follows_the_steppers_own_record():
    """B = 64 envs stepped one control interval from one state under injected normals; |psi_0><psi_0| filtered at
    eta = 1 on the stepper's record q ends on the stepper's state: 1 - <psi_b|rho_b|psi_b> is the distance of two
    different O(dt) schemes (the step kernels' SSE integrator, the exact instrument between Cayley steps). The CPU twin
    (the oracle's steps with the same normals through the restatement, tests/filter_ref.twin_infidelity) measures
    max 4.3e-6 / mean 5.9e-7 at dt = 1/1440 and max 4.9e-7 / mean 1.0e-7 at dt / 2 (it falls with dt); the same
    normals give the same trajectories up to rounding, so the device is held to 1.5 x the twin's maximum at dt."""
    P = _pkg()
    cfg = P["cfg"]
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.core import Stepper
    ph = cfg.DEFAULTS[cfg.HO].with_(n_max=15)
    B, n, action = 64, ph.control_interval, 14
    psi0 = R.trajectory_start(ph)
    noise = np.random.default_rng(2024).standard_normal((n, B, 2))
    twin = F.twin_infidelity(ph, psi0, action, noise)
    st = Stepper(ph, B, 0, seed=1)
    me = P["MasterEquation"](ph, forces=[ph.force(action)])
    try:
        psi = st.new_state()
        psi[:] = dev(psi0)
        q = st.step(psi, None, n, default_action=action, noise=dev(noise), want_q=True)["q"]
        me.set_efficiency(1.0)
        rho = dev(np.repeat(R.pure(psi0)[None], B, axis=0))
        me.evolve_conditional(rho, n, 0, record=q.contiguous())
        me.take_errors()
        ps = psi / torch.linalg.norm(psi, dim=1, keepdim=True)
        infidelity = host(1 - torch.einsum("bi,bij,bj->b", ps.conj(), rho, ps).real)
    finally:
        me.close()
        st.close()
    print(f"infidelity: device max {infidelity.max():.3e} mean {infidelity.mean():.3e}; "
          f"CPU twin max {twin.max():.3e} mean {twin.mean():.3e}")
    assert infidelity.max() <= 1.5 * twin.max()


# ---------------------------------------------------------------- 7. the loop
def spread_states(env, seed):
    """Moves the env's states apart with a few random actions."""
    rng = np.random.default_rng(seed)
    env.reset()
    for _ in range(4):
        env.step(dev(rng.integers(0, env.ph.n_actions, env.B).astype(np.int32)))


def slots_against_the_env(ph, strategies, env_kw):
    P = _pkg()
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.env import BatchedEnv
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.lindblad import baseline_force
    env = BatchedEnv(ph, 64, 0, seed=23, input="xp", **env_kw)
    me = env.master_equation()
    try:
        spread_states(env, 7)
        rho = (me.ensemble.scale * env.psi[:, :, None] * env.psi.conj()[:, None, :]).contiguous()
        for strategy, con in strategies:
            F_ = host(baseline_force(ph, lambda k: me.expectations(rho, me.controller_operator(k)), strategy, con))
            unit = ph.f_max / (ph.n_actions // 2)
            inside = np.abs(F_) < ph.f_max
            # no env's force is within 1e-3 action spacings of a rounding tie: none is left out
            assert np.all(np.abs((F_[inside] / unit) % 1 - 0.5) >= 1e-3), strategy
            got = host(me.analytic_slots(rho, strategy, con))
            assert np.array_equal(got, host(env.analytic_actions(strategy, con))), strategy
            assert len(set(got.tolist())) > 2, strategy
    finally:
        me.close()
        env.st.close()


def test_analytic_slots_are_the_envs_analytic_actions_harmonic():
    cfg = _pkg()["cfg"]
    slots_against_the_env(cfg.DEFAULTS[cfg.HO], (("LQG", 0.0),), dict(reset="deferred"))


def test_analytic_slots_are_the_envs_analytic_actions_quartic():
    cfg = _pkg()["cfg"]
    slots_against_the_env(cfg.DEFAULTS[cfg.QO], (("LQG", 0.9), ("damping", 0.9), ("semiclassical", 0.0)),
                          dict(reset="warmup"))


def filtered_loop_on(loop, tmp_path, controller):
    tr = loop.trainer(tmp_path / "models")
    env, ph = loop.env, loop.c["ph"]
    env.reset()
    for _ in range(4):
        env.step(loop.actor.act(env.obs, eps=0.05))
    tr.save_checkpoint(tmp_path / "start.pt")
    before = sha(env.psi)
    me = env.master_equation()
    T, M = 3, 8
    out = tr.filtered_loop(me, T, eta=0.5, controller=controller, M=M, seed=3)
    keys = {"x", "x2", "h", "purity", "boundary", "slots"} | ({"n"} if ph.fock else set())
    assert set(out) == keys
    assert all(v.shape == ((T, M) if k == "slots" else (T + 1, M)) and v.is_cuda for k, v in out.items())
    assert out["slots"].dtype == torch.int32 and int(out["slots"].min()) >= 0 \
        and int(out["slots"].max()) < ph.n_actions
    assert sha(env.psi) == before
    me.take_errors()
    # entry 0 is the env states' own moments
    x0 = host(env.st.x_expectation(env.psi))[:M]
    norm = host((env.psi[:M].abs() ** 2).sum(dim=1)) * me.ensemble.scale
    assert np.abs(host(out["x"][0]) - x0).max() <= 1e-12 * (1 + np.abs(x0).max())
    assert np.abs(host(out["purity"][0]) - norm ** 2).max() <= 1e-12
    again = tr.filtered_loop(me, T, eta=0.5, controller=controller, M=M, seed=3)
    assert all(same_bits(host(again[k]), host(out[k])) for k in keys)              # a function of the seed
    ens = tr.filtered_loop(me, 1, eta=0.5, controller=controller, M=2, source="ensemble")
    assert ens["x"].shape == (2, 2) and float(ens["purity"][0, 0]) <= 1 + 1e-12
    # evaluate's and open_loop's results are bit for bit the ones without a filtered loop before them
    with_e, with_o = tr.evaluate(None, 10 ** 6, max_steps=6), None
    tr.load_checkpoint(tmp_path / "start.pt")
    tr.filtered_loop(me, 1, eta=1.0, controller=controller, M=2)
    with_o = tr.open_loop(me, 2)
    tr.load_checkpoint(tmp_path / "start.pt")
    plain_o = tr.open_loop(me, 2)
    plain_e = tr.evaluate(None, 10 ** 6, max_steps=6)
    assert np.array(with_e).tobytes() == np.array(plain_e).tobytes()
    assert all(same_bits(host(with_o[k]), host(plain_o[k])) for k in plain_o)
    for kw, text in ((dict(n_control=-1), "n_control must be an int >= 0"), (dict(source="dqn"), "source must be"),
                     (dict(M=0), "M must be an int >= 1"), (dict(M=10 ** 6), "M must be an int >= 1 and <= the env's"),
                     (dict(eta=0.0), r"eta must be in \(0, 1\]")):
        args = dict(n_control=1, eta=0.5)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            tr.filtered_loop(me, args.pop("n_control"), **args)
    me.close()


def test_filtered_loop_on_the_harmonic_loop(tmp_path):
    from tests.test_gpu_trainer import Loop
    loop = Loop("ho")
    filtered_loop_on(loop, tmp_path, ("LQG", 0.0))
    loop.close()


def test_filtered_loop_on_the_quartic_loop(tmp_path):
    from tests.test_gpu_trainer_monitor import Loop
    loop = Loop("qo")
    filtered_loop_on(loop, tmp_path, None)
    loop.close()


def test_command_line_writes_the_filtered_npz(tmp_path):
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import train
    out = tmp_path / "filtered.npz"
    common = ["--system", "ho", "--control_strategy", "LQG", "--envs", "32", "--num_of_test_episodes", "4",
              "--max_steps", "5"]
    assert train.main(common + ["--save_dir", str(tmp_path / "a"), "--filtered_out", str(out), "--eta", "0.5",
                                "--filtered_M", "4", "--open_loop_steps", "3"]) == 0
    z = np.load(out)
    assert sorted(z.files) == sorted(["t", "eta", "x", "x2", "h", "n", "purity", "boundary", "slots"])
    assert z["x"].shape == (4, 4) and z["slots"].shape == (3, 4) and z["slots"].dtype == np.int32
    assert float(z["eta"]) == 0.5 and np.allclose(z["t"], np.arange(4) / 18)
    assert train.main(common + ["--save_dir", str(tmp_path / "b")]) == 0
    assert (tmp_path / "a" / "LQG.txt").read_text() == (tmp_path / "b" / "LQG.txt").read_text()
    with pytest.raises(SystemExit):
        train.main(common + ["--save_dir", str(tmp_path / "c"), "--filtered_out", str(out)])
