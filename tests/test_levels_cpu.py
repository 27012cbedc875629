"""The energy-level view without a GPU: the host solve (qc_levels_solve, csrc/qcart_levels.hpp) through ctypes against
its definition in longdouble, mpmath and numpy; the refusals with their texts before any device; the header as a
stand-alone program (tests/diag/levels_check.cpp, its own main, built with AddressSanitizer + UBSan, run as a plain
executable); the restatement tests/levels_ref.py on closed forms; and the new entry points in the header, the binding
and the library."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from deepreinforcementlearningcontrolofquantumcartpoles_amd import _lib
from deepreinforcementlearningcontrolofquantumcartpoles_amd import config as cfg
from tests import levels_ref as R
from tests import refmath

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "diag", "levels_check.cpp")
EPS = 2.0 ** -53
QO = cfg.DEFAULTS[cfg.QO]

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libqcart.so not built")


def solve(physics, k):
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.levels import LevelView
    return LevelView.solve(physics, k)


def grid_case(x_max, h):
    ph = QO.with_(x_max=x_max, grid_size=h)
    H = refmath.grid_ops(ph.x_max, ph.grid_size, ph.lambda_, ph.mass)["H"]
    assert H.shape[0] == ph.dim
    return ph, H


CASES = [(4.0, 0.2, 41, 12), (3.2, 0.1, 65, 16), (QO.x_max, QO.grid_size, 171, 32), (QO.x_max, QO.grid_size, 171, 64)]
_solved = {}


def solved(case):
    """One solve per case, shared and left unchanged."""
    if case not in _solved:
        x_max, h, n, k = case
        ph, H = grid_case(x_max, h)
        assert ph.dim == n
        E, V = solve(ph, k)
        E.setflags(write=False)
        V.setflags(write=False)
        _solved[case] = (H, E, V)
    return _solved[case]


# ---------------------------------------------------------------- the solver against its definition
@needs_lib
@pytest.mark.parametrize("case", CASES, ids=[f"N{c[2]}-K{c[3]}" for c in CASES])
def test_residual_orthonormality_order_sign_and_parity(case):
    H, E, V = solved(case)
    n, k = case[2], case[3]
    assert E.shape == (k,) and V.shape == (k, n)
    norm = R.norm_inf(H)
    res = R.residual(H, E, V)
    print(f"N = {n}, K = {k}: residual / (2^-53 ||H||) = {res / (EPS * norm):.3f}, ||H|| = {norm:.1f}")
    assert res <= 2 * EPS * norm
    Vl = V.astype(np.longdouble)
    assert float(np.abs(Vl @ Vl.T - np.eye(k)).max()) <= (n + 4) * EPS
    assert np.all(np.diff(E) > 0)
    for row in V:                                     # the sign convention, exactly
        big = np.abs(row).max()
        last = np.nonzero(np.abs(row) > 2.0 ** -26 * big)[0][-1]
        assert row[last] > 0
    # parity alternates even, odd, ..: against the vector bound 2 sqrt(N) r / gap + 2^-53 for each of the two
    gaps = np.minimum(np.diff(E, prepend=-np.inf), np.diff(E, append=np.inf))
    r = 2 * EPS * norm
    for lvl in range(k):
        tol = 2 * (2 * math.sqrt(n) * r / gaps[lvl] + EPS)
        assert np.abs(V[lvl] - (-1) ** lvl * V[lvl][::-1]).max() <= tol, lvl


@needs_lib
def test_default_levels_are_the_documented_ones():
    _, E, _ = solved(CASES[3])
    assert np.abs(E[:5] - np.array([0.71769, 2.57175, 5.04628, 7.88158, 11.00658])).max() <= 5e-6
    assert np.diff(E).min() >= 1.854
    assert E[4] < 12 < E[5] and E[23] < 100 < E[25]


@needs_lib
def test_against_mpmath_at_40_digits():
    mp = pytest.importorskip("mpmath")
    case = CASES[0]
    H, E, V = solved(case)
    n, k = case[2], case[3]
    with mp.workdps(40):
        Emp, Q = mp.eigsy(mp.matrix(H.tolist()))
        order = sorted(range(n), key=lambda i: Emp[i])
        r = 2 * EPS * R.norm_inf(H)
        levels = [Emp[i] for i in order]
        for lvl in range(k):
            assert abs(mp.mpf(float(E[lvl])) - levels[lvl]) <= math.sqrt(n) * r
            gap = float(min(levels[lvl] - levels[lvl - 1] if lvl else mp.inf, levels[lvl + 1] - levels[lvl]))
            col = [Q[j, order[lvl]] for j in range(n)]
            sign = 1 if sum(col[j] * mp.mpf(float(V[lvl][j])) for j in range(n)) > 0 else -1
            err = max(abs(mp.mpf(float(V[lvl][j])) - sign * col[j]) for j in range(n))
            assert err <= 2 * math.sqrt(n) * r / gap + EPS, (lvl, float(err))


@needs_lib
def test_against_numpy_eigh_with_both_residuals_in_the_bound():
    H, E, V = solved(CASES[3])
    n, k = 171, 64
    norm = R.norm_inf(H)
    r = 2 * EPS * norm
    w, Q = np.linalg.eigh(H)
    r_np = R.residual(H, w[:k], Q[:, :k].T)
    print(f"numpy eigh residual / (2^-53 ||H||) = {r_np / (EPS * norm):.2f}")
    rr = r + r_np                                     # (both vectors lie within sqrt(N) residual / gap of the true one)
    gaps = np.minimum(np.diff(w[:k + 1], prepend=-np.inf)[:k], np.diff(w[:k + 1]))
    assert np.abs(E - w[:k]).max() <= math.sqrt(n) * rr
    for lvl in range(k):
        q = Q[:, lvl] * (1 if Q[:, lvl] @ V[lvl] > 0 else -1)
        assert np.abs(V[lvl] - q).max() <= 2 * math.sqrt(n) * rr / gaps[lvl] + 2 * EPS, lvl


@needs_lib
def test_ho_levels_are_the_diagonal_and_the_identity_exactly():
    ph = cfg.DEFAULTS[cfg.HO]
    assert ph.n_max == 70
    E, V = solve(ph, 71)
    want = np.array([ph.omega * (0.5 + float(k)) for k in range(71)])
    assert E.tobytes() == want.tobytes()
    assert V.tobytes() == np.eye(71).tobytes()
    E8, V8 = solve(ph, 8)
    assert E8.tobytes() == want[:8].tobytes() and V8.tobytes() == np.eye(71)[:8].tobytes()


@needs_lib
def test_two_calls_give_equal_bytes():
    _, E, V = solved(CASES[2])
    E2, V2 = solve(QO, 32)
    assert E.tobytes() == E2.tobytes() and V.tobytes() == V2.tobytes()


# ---------------------------------------------------------------- refusals through the C ABI, before any device
def params(physics):
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.core import make_params
    return make_params(physics, 1)


@needs_lib
def test_solve_refusals_with_their_texts():
    lib = _lib.lib()
    buf_e = np.zeros(300)
    buf_v = np.zeros((300, 200))
    pe, pv = ctypes.c_void_p(buf_e.ctypes.data), ctypes.c_void_p(buf_v.ctypes.data)

    def refused(physics, k, text, e=pe, v=pv, p=True):
        rc = lib.qc_levels_solve(ctypes.byref(params(physics)) if p else None, k, e, v)
        assert rc == -1, (rc, text)
        assert text in lib.qc_levels_last_error(None), lib.qc_levels_last_error(None)

    refused(cfg.DEFAULTS[cfg.IHO], 8, b"qc_levels_solve: no bound levels: H is not bounded below")
    refused(cfg.DEFAULTS[cfg.IQO], 8, b"qc_levels_solve: no bound levels: H is not bounded below")
    for k in (0, 172, 257, -1):                       # N = 171: K = N + 1, and past 256
        refused(QO, k, b"qc_levels_solve: K must be in [1, min(N, 256)]")
    refused(cfg.DEFAULTS[cfg.HO], 72, b"qc_levels_solve: K must be in [1, min(N, 256)]")
    refused(QO.with_(x_max=20.0), 257, b"qc_levels_solve: K must be in [1, min(N, 256)]")     # N = 401 > 256
    refused(QO, 8, b"params, energies and vectors are required", e=None)
    refused(QO, 8, b"params, energies and vectors are required", v=None)
    refused(QO, 8, b"params, energies and vectors are required", p=False)
    assert not buf_e.any() and not buf_v.any()        # nothing was written


@needs_lib
def test_python_solve_raises_value_error_with_the_librarys_text():
    for fam in (cfg.IHO, cfg.IQO):
        with pytest.raises(ValueError, match="no bound levels: H is not bounded below"):
            solve(cfg.DEFAULTS[fam], 8)
    with pytest.raises(ValueError, match=r"K must be in \[1, min\(N, 256\)\]"):
        solve(QO, 0)


@needs_lib
def test_create_refuses_before_the_device():
    lib = _lib.lib()
    h = ctypes.c_void_p()
    table = np.full((4, 8), 0.25)
    bad = table.copy()
    bad[3, 7] = np.nan
    tp, bp = ctypes.c_void_p(table.ctypes.data), ctypes.c_void_p(bad.ctypes.data)
    for args, text in (((0, 1, 1.0, tp), b"qc_levels_create: N must be in [1, 2048]"),
                       ((2049, 1, 1.0, tp), b"qc_levels_create: N must be in [1, 2048]"),
                       ((8, 0, 1.0, tp), b"qc_levels_create: K must be in [1, min(N, 256)]"),
                       ((8, 9, 1.0, tp), b"qc_levels_create: K must be in [1, min(N, 256)]"),
                       ((300, 257, 1.0, tp), b"qc_levels_create: K must be in [1, min(N, 256)]"),
                       ((8, 4, 0.0, tp), b"qc_levels_create: scale must be finite and > 0"),
                       ((8, 4, float("inf"), tp), b"qc_levels_create: scale must be finite and > 0"),
                       ((8, 4, float("nan"), tp), b"qc_levels_create: scale must be finite and > 0"),
                       ((8, 4, 1.0, None), b"qc_levels_create: vectors are required"),
                       ((8, 4, 1.0, bp), b"qc_levels_create: every table entry must be finite")):
        rc = lib.qc_levels_create(*args, 0, ctypes.byref(h))
        assert rc == -1 and not h.value, args
        assert text in lib.qc_levels_last_error(None), (args, lib.qc_levels_last_error(None))
    assert lib.qc_levels_create(8, 4, 1.0, tp, 0, None) == -1
    assert b"out is required" in lib.qc_levels_last_error(None)


# ---------------------------------------------------------------- the host header as a sanitised program
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("levels_check")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run([cxx, *flags, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0 \
            or subprocess.run([str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot build or run -fsanitize=address,undefined programs here")
    out = tmp / "levels_check"
    subprocess.run([cxx, *flags, "-Wall", "-Wextra", "-Werror", SRC, "-o", str(out)], check=True)
    return str(out)


def run(exe, *words):
    r = subprocess.run([exe, *[str(w) for w in words]], capture_output=True, text=True, timeout=120)
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    return r


def test_solves_over_every_size_under_the_sanitisers(exe):
    r = run(exe)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stdout[-300:], r.stderr[-300:])


REFUSALS = [
    (("solve", 1, 181, 8), "no bound levels: H is not bounded below"),
    (("solve", 3, 521, 8), "no bound levels: H is not bounded below"),
    (("solve", 7, 41, 8), "unknown family"),
    (("solve", 2, 171, 0), "K must be in [1, min(N, 256)]"),
    (("solve", 2, 171, 172), "K must be in [1, min(N, 256)]"),
    (("solve", 2, 401, 257), "K must be in [1, min(N, 256)]"),
    (("solve", 2, 0, 1), "N must be in [1, 2048]"),
    (("solve", 2, 2049, 1), "N must be in [1, 2048]"),
    (("create", 0, 1, 1.0, 1), "N must be in [1, 2048]"),
    (("create", 2049, 1, 1.0, 1), "N must be in [1, 2048]"),
    (("create", 8, 0, 1.0, 1), "K must be in [1, min(N, 256)]"),
    (("create", 8, 9, 1.0, 1), "K must be in [1, min(N, 256)]"),
    (("create", 8, 4, 0.0, 1), "scale must be finite and > 0"),
    (("create", 8, 4, -1.0, 1), "scale must be finite and > 0"),
    (("create", 8, 4, "nan", 1), "scale must be finite and > 0"),
    (("create", 8, 4, "inf", 1), "scale must be finite and > 0"),
    (("create", 8, 4, 1.0, 0), "vectors are required"),
    (("create", 8, 4, 1.0, 2), "every table entry must be finite"),
    (("call", 0, 4, 1), "psi and out are required"),
    (("call", 1, 4, 0), "psi and out are required"),
    (("call", 1, 0, 1), "B must be >= 1"),
    (("call", 1, -7, 1), "B must be >= 1"),
]


@pytest.mark.parametrize("words,text", REFUSALS, ids=[f"{w[0]}-{i}" for i, (w, _) in enumerate(REFUSALS)])
def test_refusals_with_their_texts(exe, words, text):
    r = run(exe, *words)
    assert r.returncode == 2 and r.stdout.strip() == "refused: " + text, (r.returncode, r.stdout[-300:])


def test_the_bounds_themselves_are_accepted(exe):
    assert run(exe, "solve", 2, 171, 171).stdout == "accepted\n"
    assert run(exe, "solve", 0, 2048, 256).stdout == "accepted\n"
    assert run(exe, "create", 2048, 256, float(5e-324).hex(), 1).stdout == "accepted\n"
    assert run(exe, "create", 1, 1, 1.0, 1).stdout == "accepted\n"
    assert run(exe, "call", 1, 1, 1).stdout == "accepted\n"


# ---------------------------------------------------------------- the restatement on closed forms
def test_restated_mean_is_the_plain_mean_where_sums_are_exact():
    """Small integers add exactly in any order: the documented order must then give the plain masked mean, at sizes
    on both sides of a sub-group, a group and the four running sums."""
    rng = np.random.default_rng(5)
    for B in (1, 15, 16, 17, 63, 64, 65, 257, 1100):
        p = rng.integers(0, 8, size=(B, 5)).astype(np.float64)
        mask = rng.random(B) < 0.6
        m, n = R.mean_documented_order(p, mask)
        assert n == int(mask.sum())
        want = p[mask].sum(axis=0) / n if n else np.zeros(5)
        assert m.tobytes() == (want + 0.0).tobytes(), B
        m, n = R.mean_documented_order(p)
        assert n == B and m.tobytes() == (p.sum(axis=0) / B).tobytes()
    m, n = R.mean_documented_order(np.ones((70, 3)), np.zeros(70, dtype=bool))
    assert n == 0 and not m.any()


def test_restated_amplitudes_of_a_basis_table():
    """An identity table returns the state; the bound is then (N + 4) 2^-53 |part psi|."""
    rng = np.random.default_rng(6)
    psi = rng.standard_normal((3, 9)) + 1j * rng.standard_normal((3, 9))
    re, im = R.amplitudes_longdouble(psi, np.eye(9)[:4], 2.0)
    assert np.array_equal(re.astype(np.float64), 2 * psi.real[:, :4])
    assert np.array_equal(im.astype(np.float64), 2 * psi.imag[:, :4])
    bre, bim = R.bound(psi, np.eye(9)[:4], 2.0)
    assert np.allclose(bre, 13 * EPS * 2 * np.abs(psi.real[:, :4]), rtol=1e-15)
    assert np.array_equal(R.populations_of(np.array([3 + 4j])), np.array([25.0]))


# ---------------------------------------------------------------- the surface
NAMES = ["qc_levels_solve", "qc_levels_create", "qc_levels_destroy", "qc_levels_last_error", "qc_levels_set_stream",
         "qc_levels_amplitudes", "qc_levels_populations", "qc_levels_mean"]


def test_new_entry_points_in_header_binding_and_library():
    assert set(NAMES) <= set(_lib.EXPORTS) and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    assert callable(_lib.check_levels)
    header = open(os.path.join(ROOT, "include", "qcart.h")).read()
    for n in NAMES:
        assert re.search(rf"\b{n}\(", header), n
    if os.path.exists(_lib.LIB_PATH):
        so = ctypes.CDLL(_lib.LIB_PATH)
        for n in NAMES:
            assert hasattr(so, n), n


def test_package_exports_the_view_lazily():
    import deepreinforcementlearningcontrolofquantumcartpoles_amd as pkg
    assert "LevelView" in pkg.__all__
    assert pkg.LevelView.__name__ == "LevelView"
