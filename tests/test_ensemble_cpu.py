"""The ensemble density matrix without a GPU: the restatement tests/ensemble_ref.py against closed forms; a float64 numpy
evaluation inside the a-priori bound the device is held to (tests/test_gpu_ensemble.py); the order functions and the
argument checks (csrc/qcart_ensemble.hpp) from a stand-alone program (tests/diag/ensemble_check.cpp, its own main, built
with AddressSanitizer + UBSan, run as a plain executable); and the new entry points in the header, the binding and the
library."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from deepreinforcementlearningcontrolofquantumcartpoles_amd import _lib
from tests import ensemble_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "diag", "ensemble_check.cpp")


# ---------------------------------------------------------------- the restatement against closed forms
def purity(rho):
    return float((np.abs(rho) ** 2).sum())


def test_restatement_copies_of_one_state_are_pure():
    rng = np.random.default_rng(1)
    psi = rng.standard_normal(33) + 1j * rng.standard_normal(33)
    psi /= np.linalg.norm(psi)
    rho, n = R.density_longdouble(np.tile(psi, (7, 1)))
    assert n == 7
    wide = psi.astype(np.clongdouble)                # (a few 2^-64 roundings of elements below 0.1)
    assert np.abs(rho - np.outer(wide, wide.conj())).max() <= 1e-18
    assert abs(purity(rho) - 1) <= 1e-15


def test_restatement_basis_states_give_the_identity():
    K = 12
    rho, n = R.density_longdouble(np.eye(K, dtype=np.complex128) * np.exp(1j * np.arange(K))[:, None])
    # (the float64 phases have a modulus within a few 2^-53 of 1; the inputs' roundings, not the restatement's, set
    # these tolerances and those below)
    assert n == K and np.abs(rho - np.eye(K) / K).max() <= 1e-16
    assert abs(purity(rho) - 1 / K) <= 1e-15
    # with a mask over the first three, and the grid normalisation: scale h, states of norm 1 / sqrt(h)
    h = 0.1
    mask = np.arange(K) < 3
    rho, n = R.density_longdouble(np.eye(K, dtype=np.complex128) / np.sqrt(h), mask, scale=h)
    want = np.diag(mask / 3.0)
    assert n == 3 and np.abs(rho - want).max() <= 1e-15 and abs(float(np.trace(rho).real) - 1) <= 1e-15
    rho, n = R.density_longdouble(np.eye(K, dtype=np.complex128), np.zeros(K, dtype=bool))
    assert n == 0 and not np.any(rho)


def test_restatement_coherent_state_has_poisson_populations():
    alpha, N = 1.3 - 0.4j, 60
    amp = np.array([np.exp(-abs(alpha) ** 2 / 2) * alpha ** k / math.sqrt(math.factorial(k)) for k in range(N)])
    rho, _ = R.density_longdouble(np.stack([amp, amp * np.exp(0.7j)]))       # a global phase does not show
    lam = abs(alpha) ** 2
    poisson = np.array([math.exp(-lam) * lam ** k / math.factorial(k) for k in range(N)])
    assert np.abs(np.diag(rho).real.astype(np.float64) - poisson).max() <= 1e-15
    assert abs(float((np.arange(N) * np.diag(rho).real).sum()) - lam) <= 1e-14


def test_float64_evaluation_stays_inside_the_a_priori_bound():
    """The bound the device is held to, tried on a plain float64 evaluation (numpy's matmul, another order): a small
    fraction of it. Measured here: 0.001 at (1100, 65), 0.03 at (33, 181), 0.16 at (3, 513)."""
    rng = np.random.default_rng(11)
    for B, N in ((1100, 65), (33, 181), (3, 513)):
        psi = rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N))
        psi /= np.linalg.norm(psi, axis=1, keepdims=True)
        got = (psi.T @ psi.conj()) / B
        want, n = R.density_longdouble(psi)
        b = R.bound(psi)
        ratio = float((np.abs(got - want).astype(np.float64) / b).max())
        print(f"(B, N) = ({B}, {N}): max err / bound = {ratio:.3f}")
        assert n == B and ratio <= 1.0


def test_documented_splits():
    assert [R.splits(B, N) for B, N in ((1, 71), (2, 71), (3, 71), (5, 71), (33, 71), (1100, 71), (1100, 250),
                                        (4096, 181), (65536, 513), (3, 2048))] == \
        [1, 1, 2, 3, 17, 256, 67, 128, 15, 1]


# ---------------------------------------------------------------- the host header as a sanitised program
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("ensemble_check")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run([cxx, *flags, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0 \
            or subprocess.run([str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot build or run -fsanitize=address,undefined programs here")
    out = tmp / "ensemble_check"
    subprocess.run([cxx, *flags, "-Wall", "-Wextra", "-Werror", SRC, "-o", str(out)], check=True)
    return str(out)


def run(exe, *words):
    r = subprocess.run([exe, *[str(w) for w in words]], capture_output=True, text=True, timeout=120)
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    return r


def test_order_functions_over_every_shape(exe):
    r = run(exe)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stdout[-300:], r.stderr[-300:])


REFUSALS = [
    (("create", 0, 1.0), "N must be in [1, 2048]"),
    (("create", -3, 1.0), "N must be in [1, 2048]"),
    (("create", 2049, 1.0), "N must be in [1, 2048]"),
    (("create", 8, 0.0), "scale must be finite and > 0"),
    (("create", 8, -0.5), "scale must be finite and > 0"),
    (("create", 8, "nan"), "scale must be finite and > 0"),
    (("create", 8, "inf"), "scale must be finite and > 0"),
    (("call", 0, 4, 1), "psi and rho are required"),
    (("call", 1, 4, 0), "psi and rho are required"),
    (("call", 1, 0, 1), "B must be >= 1"),
    (("call", 1, -7, 1), "B must be >= 1"),
]


@pytest.mark.parametrize("words,text", REFUSALS, ids=[f"{w[0]}-{i}" for i, (w, _) in enumerate(REFUSALS)])
def test_refusals_with_their_texts(exe, words, text):
    r = run(exe, *words)
    assert r.returncode == 2 and r.stdout.strip() == "refused: " + text, (r.returncode, r.stdout[-300:])


def test_the_bounds_themselves_are_accepted(exe):
    r = run(exe, "create", 1, float(5e-324).hex())
    assert r.returncode == 0 and r.stdout.splitlines() == ["accepted", "chunk 2 max_splits 256 doubles 512"]
    r = run(exe, "create", 2048, 1.0)
    assert r.returncode == 0 and r.stdout.splitlines() == ["accepted", f"chunk 2 max_splits 1 doubles {2 ** 23}"]
    assert run(exe, "call", 1, 1, 1).stdout == "accepted\n"


# ---------------------------------------------------------------- the surface
NAMES = ["qc_ensemble_create", "qc_ensemble_destroy", "qc_ensemble_last_error", "qc_ensemble_set_stream",
         "qc_ensemble_density", "qc_ensemble_chunk", "qc_ensemble_splits"]


def test_new_entry_points_in_header_binding_and_library():
    assert set(NAMES) <= set(_lib.EXPORTS) and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    assert callable(_lib.check_ensemble)
    header = open(os.path.join(ROOT, "include", "qcart.h")).read()
    for n in NAMES:
        assert re.search(rf"\b{n}\(", header), n
    if os.path.exists(_lib.LIB_PATH):
        so = ctypes.CDLL(_lib.LIB_PATH)
        for n in NAMES:
            assert hasattr(so, n), n


def test_create_refuses_before_the_device():
    """The refusals reach the C ABI with their text, before any device is touched."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libqcart.so not built")
    lib = _lib.lib()
    h = ctypes.c_void_p()
    for args, text in (((0, 1.0), b"qc_ensemble_create: N must be in [1, 2048]"),
                       ((2049, 1.0), b"qc_ensemble_create: N must be in [1, 2048]"),
                       ((181, 0.0), b"qc_ensemble_create: scale must be finite and > 0"),
                       ((181, float("nan")), b"qc_ensemble_create: scale must be finite and > 0"),
                       ((181, float("inf")), b"qc_ensemble_create: scale must be finite and > 0")):
        rc = lib.qc_ensemble_create(*args, 0, ctypes.byref(h))
        assert rc == -1 and not h.value
        assert text in lib.qc_ensemble_last_error(None), (args, lib.qc_ensemble_last_error(None))
    assert lib.qc_ensemble_create(181, 1.0, 0, None) == -1


def test_the_order_is_a_function_of_the_shape():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libqcart.so not built")
    lib = _lib.lib()
    assert [lib.qc_ensemble_chunk(n) for n in (0, 1, 181, 2048, 2049)] == [0, 2, 2, 2, 0]
    for B, N in ((1, 71), (2, 71), (3, 71), (5, 71), (33, 71), (1100, 71), (1100, 250), (4096, 181), (65536, 513),
                 (3, 2048), (2 ** 31 - 3, 1)):
        assert lib.qc_ensemble_splits(B, N) == R.splits(B, N), (B, N)
    assert lib.qc_ensemble_splits(0, 181) == 0 and lib.qc_ensemble_splits(4, 2049) == 0


def test_package_exports_the_view_lazily():
    import deepreinforcementlearningcontrolofquantumcartpoles_amd as pkg
    assert "EnsembleView" in pkg.__all__
    assert pkg.EnsembleView.__name__ == "EnsembleView"
