"""The conditional master equation without a GPU: the scheme's identities on the longdouble restatement
(tests/filter_ref.py) — the instrument identity by quadrature over the outcome, purity at eta = 1, the mean over 4096
records against the unconditional scheme within five standard errors, a plain fp64 evaluation inside the a-priori bound
— the library's host side (the Philox mirror against an independent Philox and libm, the table G^(1-eta) against
longdouble, the refusals with their texts before any device), the header as a stand-alone sanitised program
(tests/diag/filter_check.cpp), the baseline controllers' formulas on rho against oracle/controllers.py, and the
surface."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from deepreinforcementlearningcontrolofquantumcartpoles_amd import _lib
from deepreinforcementlearningcontrolofquantumcartpoles_amd import config as cfg
from deepreinforcementlearningcontrolofquantumcartpoles_amd import lindblad as LB
from deepreinforcementlearningcontrolofquantumcartpoles_amd.core import make_params
from oracle import controllers as OC
from tests import filter_ref as F
from tests import lindblad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "diag", "filter_check.cpp")
LD, CLD, EPS = F.LD, F.CLD, F.EPS
HO, IHO, QO, IQO = (cfg.DEFAULTS[k] for k in (cfg.HO, cfg.IHO, cfg.QO, cfg.IQO))
needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libqcart.so not built")


def random_rho(N, seed, rank=3):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((N, rank)) + 1j * rng.standard_normal((N, rank))
    rho = a @ a.conj().T
    return rho / np.trace(rho).real


def ho_tables(n_max, force):
    ph = HO.with_(n_max=n_max)
    H, X, c, fock = R.operators(ph)
    return ph, R.tables(H, X, c, force, ph.dt, ph.gamma, fock)


# ---------------------------------------------------------------- the scheme's identities
@pytest.mark.parametrize("N", (5, 16))
def test_the_average_over_outcomes_is_the_dephasing_factor(N):
    """int dy M_y sigma M_y = G^eta o sigma with M_y = diag((2 a / pi)^(1/4) exp(-a (xi_i - y)^2)): the trapezoid rule
    on a grid far finer than the Gaussians' width converges geometrically, so 1e-12 is the quadrature's own error."""
    rng = np.random.default_rng(N)
    xi = np.sort(rng.uniform(-3, 3, N)).astype(LD)
    sigma = random_rho(N, 10 + N).astype(CLD)
    gamma, dt, eta = LD(2.0), LD(0.05), LD(0.4)
    a = eta * gamma * dt / 2
    width = 1 / np.sqrt(a)
    y = np.linspace(float(xi[0] - 12 * width), float(xi[-1] + 12 * width), 6001).astype(LD)
    m = (2 * a / LD(np.pi)) ** LD(0.25) * np.exp(-a * (xi[None, :] - y[:, None]) ** 2)          # [Y, N]
    kernel = np.einsum("yi,yj->ij", m, m) * (y[1] - y[0])
    want = F.g_power(xi, dt, gamma, eta) * sigma
    assert np.abs(kernel * sigma - want).max() <= 1e-12
    # and the normalised post-state's weight is the density the outcome is drawn from
    p = np.einsum("yi,i->y", m * m, sigma.diagonal().real)
    assert abs(float((p * (y[1] - y[0])).sum()) - 1) <= 1e-12


def test_a_pure_state_stays_pure_at_full_efficiency():
    ph, tab = ho_tables(15, 2.0)
    a, _ = F.constants(1.0, ph.gamma, ph.dt)
    rho = R.pure(R.trajectory_start(ph))
    rng = np.random.default_rng(3)
    draws = np.stack([rng.random(10), rng.standard_normal(10)], axis=1)
    out = F.evolve(rho, 10, tab, None, a, True, draws=draws)
    purity = float((np.abs(out["rho"]) ** 2).sum())
    assert abs(float(np.trace(out["rho"]).real) - 1) <= 1e-15 and abs(purity - 1) <= 2e-15, purity
    # a mixed one's purity rises under eta = 1 and its trace stays 1
    mixed = F.evolve(random_rho(16, 5), 10, tab, None, a, True, draws=draws)
    assert abs(float(np.trace(mixed["rho"]).real) - 1) <= 1e-15


def batch_step(s, T, g, xi, a, u, z):
    """One step of a batch [M, N, N] in fp64 numpy (the prototype the issue measured)."""
    p = T @ s @ T.conj().T
    if g is not None:
        p = g * p
    d = np.maximum(np.einsum("mii->mi", p).real, 0)
    c = np.cumsum(d, axis=1)
    I = (c > (u * c[:, -1])[:, None]).argmax(axis=1)
    y = xi[I] + z / math.sqrt(4 * a)
    e = (xi[None, :] - y[:, None]) ** 2
    w = np.exp(-a * (e - e.min(axis=1, keepdims=True)))
    v = w / np.sqrt((w * w * d).sum(axis=1, keepdims=True))
    return (v[:, :, None] * v[:, None, :]) * p, y


@pytest.mark.parametrize("eta", (1.0, 0.5, 0.1))
def test_the_mean_over_records_is_the_unconditional_scheme(eta):
    ph, tab = ho_tables(15, 2.0)
    M, n = 4096, 10
    a = float(F.constants(eta, ph.gamma, ph.dt)[0])
    xi_ld = R.xi_longdouble(tab["W"], R.operators(ph)[1])
    g = None if eta == 1.0 else F.g_power(xi_ld, ph.dt, ph.gamma, 1 - eta).astype(np.float64)
    W, T = tab["W"], tab["T"]
    s0 = W.T @ R.pure(R.trajectory_start(ph)) @ W
    s = np.repeat(s0[None], M, axis=0)
    rng = np.random.default_rng(int(eta * 100))
    for _ in range(n):
        s, _ = batch_step(s, T, g, tab["xi"], a, rng.random(M), rng.standard_normal(M))
    exact = s0
    for _ in range(n):
        exact = tab["g_full"] * (T @ exact @ T.conj().T)
    mean = s.mean(axis=0)
    purity = float((np.abs(s) ** 2).sum(axis=(1, 2)).mean())
    se = math.sqrt(max(purity - float((np.abs(mean) ** 2).sum()), 0.0) / M)
    dev = float(np.linalg.norm(mean - exact))
    print(f"eta = {eta}: |mean - exact|_F / standard error = {dev / se:.3f}")
    assert dev <= 5 * se
    if eta == 1.0:
        assert abs(float((np.abs(s) ** 2).sum(axis=(1, 2)).max()) - 1) <= 1e-13


@pytest.mark.parametrize("eta", (1.0, 0.5))
def test_an_fp64_evaluation_stays_inside_the_bound(eta):
    ph, tab = ho_tables(16, 1.5)
    N, n, M = 17, 8, 5
    a_ld, _ = F.constants(eta, ph.gamma, ph.dt)
    xi_ld = R.xi_longdouble(tab["W"], R.operators(ph)[1])
    g = None if eta == 1.0 else F.g_power(xi_ld, ph.dt, ph.gamma, 1 - eta).astype(np.float64)
    rng = np.random.default_rng(17)
    worst = 0.0
    for m in range(M):
        rho = random_rho(N, 40 + m)
        draws = np.stack([rng.random(n), rng.standard_normal(n)], axis=1)
        want = F.evolve(rho, n, tab, g, a_ld, True, draws=draws)
        assert want["margin"].min() >= 1e-9
        s = tab["W"].T @ rho @ tab["W"]
        for k in range(n):
            s, _ = batch_step(s[None], tab["T"], g, tab["xi"], float(a_ld), draws[k:k + 1, 0], draws[k:k + 1, 1])
            s = s[0]
        got = tab["W"] @ s @ tab["W"].T
        err = np.maximum(np.abs(got.real - want["rho"].real), np.abs(got.imag - want["rho"].imag)).astype(np.float64)
        assert np.all(err <= want["bound"]), (eta, m, float((err / want["bound"]).max()))
        worst = max(worst, float((err / want["bound"]).max()))
    print(f"eta = {eta}: largest fp64 error / bound = {worst:.4f}")


# ---------------------------------------------------------------- the library's host side
MASK = 0xFFFFFFFF


def philox(ctr, key):
    c, (k0, k1) = list(ctr), key
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & MASK, (p0 >> 32) ^ c[3] ^ k1, p0 & MASK]
    return c


def unit(hi, lo):
    return (float(((hi << 32) | lo) >> 11) + 0.5) * 2.0 ** -53


@needs_lib
def test_the_host_mirror_of_the_draws_reproduces_known_words():
    assert philox([0] * 4, (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert philox([MASK] * 4, (MASK, MASK)) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    lib = _lib.lib()
    for seed, stream, step in ((0, 0, 0), (42, 7, 3), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 40 + 5), (12345, 20, 79)):
        u, z = F.host_draws(lib, seed, stream, step)
        key = (seed & MASK, seed >> 32)
        w = philox([step & MASK, step >> 32, stream, 0x500], key)
        assert u == unit(w[0], w[1])
        w = philox([step & MASK, step >> 32, stream, 0x501], key)
        rad = math.sqrt(-2 * math.log(unit(w[0], w[1])))
        assert abs(z - rad * math.cos(2 * math.pi * unit(w[2], w[3]))) <= 2e-15 * (1 + rad)
    assert lib.qc_lindblad_filter_draws(0, 0, 0, None, None) == -1


def efficiency_table(ph, eta, dt=None, gamma=None):
    g = np.full((ph.dim, ph.dim), -1.0)
    rc = _lib.lib().qc_lindblad_efficiency_table(ctypes.byref(make_params(ph, 1)), ph.dt if dt is None else dt,
                                                 ph.gamma if gamma is None else gamma, eta,
                                                 ctypes.c_void_p(g.ctypes.data))
    return rc, g


@needs_lib
@pytest.mark.parametrize("ph", (HO.with_(n_max=15), IHO.with_(n_max=64), QO.with_(x_max=1.0, grid_size=0.125)),
                         ids=("HO15", "IHO64", "QO17"))
def test_the_efficiency_table_against_longdouble(ph):
    tab = LB.MasterEquation.tables(ph, 0.0)
    xi_ld = R.xi_longdouble(tab["W"], R.operators(ph)[1]) if ph.fock else tab["xi"].astype(LD)
    for eta in (0.5, 0.1, 0.999):
        rc, g = efficiency_table(ph, eta)
        assert rc == 0
        want = F.g_power(xi_ld, ph.dt, ph.gamma, LD(1) - LD(eta))
        assert np.array_equal(g, g.T) and np.all(np.diag(g) == 1.0)
        assert np.all(np.abs(g.astype(LD) - want) <= np.spacing(g))          # within one ulp
    rc, g = efficiency_table(ph, 1.0)
    assert rc == 0 and np.all(g == 1.0)


@needs_lib
def test_refusals_before_the_device():
    lib = _lib.lib()
    for eta in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        rc, g = efficiency_table(HO, eta)
        assert rc == -1 and np.all(g == -1.0)
        got = lib.qc_lindblad_last_error(None)
        assert got.startswith(b"qc_lindblad_efficiency_table: ") and b"eta must be in (0, 1]" in got, got
    rc, _ = efficiency_table(HO, 0.5, gamma=0.0)
    assert rc == -1 and b"gamma must be > 0 for a conditional evolution" in lib.qc_lindblad_last_error(None)
    rc, _ = efficiency_table(HO, 0.5, dt=0.0)
    assert rc == -1 and b"dt must be finite and > 0" in lib.qc_lindblad_last_error(None)
    rc, _ = efficiency_table(IHO.with_(n_max=511), 0.5)
    assert rc == -1 and b"the Fock families are evolved up to N = 256" in lib.qc_lindblad_last_error(None)
    assert lib.qc_lindblad_efficiency_table(None, 1e-3, 1.0, 0.5, None) == -1
    assert b"params and g are required" in lib.qc_lindblad_last_error(None)
    # null handles
    assert lib.qc_lindblad_set_efficiency(None, 0.5) == -1
    assert lib.qc_lindblad_efficiency(None, None) == -1
    assert lib.qc_lindblad_evolve_conditional(None, None, 1, None, 0, 1, 0, None, 0, None, None, None) == -1


# ---------------------------------------------------------------- the host header as a sanitised program
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("filter_check")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run([cxx, *flags, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0 \
            or subprocess.run([str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot build or run -fsanitize=address,undefined programs here")
    out = tmp / "filter_check"
    subprocess.run([cxx, *flags, "-Wall", "-Wextra", "-Werror", SRC, "-o", str(out)], check=True)
    return str(out)


def run(exe, *words):
    r = subprocess.run([exe, *[str(w) for w in words]], capture_output=True, text=True, timeout=120)
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    return r


def test_the_host_functions_under_the_sanitisers(exe):
    r = run(exe)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stdout[-300:], r.stderr[-300:])


#                rho M  N  slots default J steps eta first draws record
GOOD = ("conditional", 1, 1, 16, 0, 0, 1, 1, 0.5, 0, 0, 0)


def but(**kw):
    names = ("mode", "rho", "M", "N", "slots", "default", "J", "steps", "eta", "first", "draws", "record")
    return tuple(kw.get(k, v) for k, v in zip(names, GOOD))


REFUSALS = [
    (("efficiency", 0.0, 1.0), "eta must be in (0, 1]"),
    (("efficiency", -1.0, 1.0), "eta must be in (0, 1]"),
    (("efficiency", float(np.nextafter(1.0, 2.0)).hex(), 1.0), "eta must be in (0, 1]"),
    (("efficiency", "nan", 1.0), "eta must be in (0, 1]"),
    (("efficiency", "inf", 1.0), "eta must be in (0, 1]"),
    (("efficiency", 0.5, 0.0), "gamma must be > 0 for a conditional evolution (nothing is measured)"),
    (but(rho=0), "rho is required"),
    (but(M=0), "M must be >= 1"),
    (but(M=33, N=2048), "M N^2 must be <= 2^27"),
    (but(steps=-1), "n_steps must be >= 0"),
    (but(default=1), "default_slot must be in [0, J)"),
    (but(first=-1), "first_step must be >= 0"),
    (but(first=2 ** 63 - 1), "first_step must be >= 0"),
    (but(draws=1, record=1), "record_in and draws exclude each other"),
    (but(eta=-1.0), "the efficiency is not set (qc_lindblad_set_efficiency first)"),
]


@pytest.mark.parametrize("words,text", REFUSALS, ids=[f"{w[0]}-{i}" for i, (w, _) in enumerate(REFUSALS)])
def test_refusals_with_their_texts(exe, words, text):
    r = run(exe, *words)
    assert r.returncode == 2 and r.stdout.strip() == "refused: " + text, (r.returncode, r.stdout[-300:])


def test_the_bounds_themselves_are_accepted(exe):
    assert run(exe, "efficiency", 1.0, 1.0).stdout == "accepted\n"
    assert run(exe, "efficiency", float(5e-324).hex(), float(5e-324).hex()).stdout == "accepted\n"
    assert run(exe, *GOOD).stdout == "accepted\n"
    assert run(exe, *but(steps=0, draws=1)).stdout == "accepted\n"
    assert run(exe, *but(record=1, slots=1, default=99)).stdout == "accepted\n"
    assert run(exe, *but(first=2 ** 63 - 2)).stdout == "accepted\n"
    assert run(exe, *but(M=32, N=2048)).stdout == "accepted\n"


# ---------------------------------------------------------------- the baseline controllers on rho
def expectations_of(ph, states, scale):
    rho = torch.from_numpy(np.stack([scale * np.outer(s, s.conj()) for s in states]))
    return lambda name: LB.MasterEquation.expectations(rho, torch.from_numpy(LB.controller_operator(ph, name)))


def test_fock_lqg_on_pure_rho_against_the_formula_in_fp64():
    rng = np.random.default_rng(8)
    for ph in (HO.with_(n_max=15), IHO.with_(n_max=24)):
        N = ph.dim
        states = rng.standard_normal((64, N)) + 1j * rng.standard_normal((64, N))
        states[:, 8:] = 0
        states *= rng.uniform(0.02, 0.5, (64, 1))                        # (forces inside and outside the grid)
        states[:, 0] += 1
        states /= np.linalg.norm(states, axis=1, keepdims=True)
        got = LB.baseline_slots(ph, expectations_of(ph, states, 1.0), "LQG").numpy()
        ops = OC.fock_ops(N - 1)
        dt, w = 1. / ph.n_con, ph.omega
        for b, s in enumerate(states):
            ex = lambda op: float(np.real(np.conj(s).dot(op.dot(s))))   # noqa: E731
            x, p = ex(ops[0]), ex(ops[1])
            if ph.family == cfg.IHO:                                     # (oracle/controllers.py fock_lqg, in fp64)
                Fc = -(x + p) * (1 + w * dt + 0.5 * w * w * dt * dt) / (dt + w * dt * dt / 2)
            else:
                Fc = -((x + p) + (p - x) * w * dt) / dt
            action, _ = OC._round_force(Fc / w, ph.f_max)
            tie = abs((Fc / w) / (ph.f_max / 10) % 1 - 0.5)
            assert got[b] == action or tie < 1e-9, (ph.family, b)
        assert len(set(got.tolist())) > 3
    with pytest.raises(ValueError, match="the Fock families take only 'LQG'"):
        LB.baseline_slots(HO, lambda k: torch.zeros(1, dtype=torch.float64), "damping")


def test_grid_controllers_on_pure_rho_against_the_oracle():
    ph = QO.with_(x_max=4.0, grid_size=0.125)
    N = ph.dim
    grid = OC.Grid(ph.x_max, N)
    rng = np.random.default_rng(9)
    states = []
    for _ in range(64):
        x0, k0, sd = rng.uniform(-1.5, 1.5), rng.uniform(-0.6, 0.6), rng.uniform(0.4, 0.9)
        s = np.exp(-(grid.x - x0) ** 2 / (4 * sd * sd) + 1j * k0 * grid.x)
        states.append(s / math.sqrt(float((np.abs(s) ** 2).sum() * grid.grid_size)))
    ex = expectations_of(ph, states, ph.grid_size)
    for strategy, con in (("LQG", 0.9), ("damping", 0.9), ("semiclassical", 0.0)):
        got = LB.baseline_slots(ph, ex, strategy, con).numpy()
        for b, s in enumerate(states):
            Fc = OC.grid_force(grid, s, strategy, con, ph.lambda_, ph.mass, ph.n_con)
            action, _ = OC.grid_control(grid, s, strategy, con, ph.lambda_, ph.mass, ph.n_con, ph.f_max)
            tie = abs((Fc / math.pi) / (ph.f_max / 10) % 1 - 0.5)
            assert got[b] == action or tie < 1e-9, (strategy, b)
        assert len(set(got.tolist())) > 3, strategy
    with pytest.raises(ValueError, match="no strategy 'pid'"):
        LB.baseline_slots(ph, ex, "pid")
    with pytest.raises(ValueError, match="no controller operator 'h'"):
        LB.controller_operator(ph, "h")


# ---------------------------------------------------------------- the surface
NAMES = ["qc_lindblad_set_efficiency", "qc_lindblad_efficiency", "qc_lindblad_evolve_conditional",
         "qc_lindblad_filter_draws", "qc_lindblad_efficiency_table", "qc_lindblad_xi"]


def test_new_entry_points_in_header_binding_and_library():
    assert set(NAMES) <= set(_lib.EXPORTS) and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    header = open(os.path.join(ROOT, "include", "qcart.h")).read()
    for n in NAMES:
        assert re.search(rf"\b{n}\(", header), n
    if os.path.exists(_lib.LIB_PATH):
        so = ctypes.CDLL(_lib.LIB_PATH)
        for n in NAMES:
            assert hasattr(so, n), n
    for tag in ("0x500", "0x501"):
        assert tag in header and tag in open(os.path.join(ROOT, "DESIGN.md")).read()
