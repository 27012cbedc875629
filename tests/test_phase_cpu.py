"""The definitions behind the phase-space view of density matrices, checked with no GPU: the longdouble restatement
(tests/phase_ref.py) against the wavefunctions' restatement (tests/wigner_ref.py) for pure states and mixtures, the
position marginal, the closed forms through the Fock route on the drivers' 250 points, a float64 evaluation against
the a-priori bound (largest ratio seen: 0.17, printed), and that the mistakes the GPU tests must catch move W by
at least 1000 bounds."""
import numpy as np
import pytest

from tests import phase_ref as PR
from tests import spatial_ref as SR
from tests import wigner_ref as R

LD = np.longdouble
DRIVER_GRID = np.linspace(-14, 14, 250)
DEFAULT_P = np.linspace(-12, 12, 193)


def grid(X):
    return np.linspace(-3, 3, X)


def states(B, X, seed):
    rng = np.random.default_rng(seed)
    phi = rng.standard_normal((B, X)) + 1j * rng.standard_normal((B, X))
    h = 6. / (X - 1)
    return phi / np.sqrt(h * (np.abs(phi) ** 2).sum(axis=1, keepdims=True)), h


def pure_longdouble(phi, h, weights=None):
    """(Re, Im) of sum_b w_b h phi_b phi_b^† in longdouble (w: 1 / B)."""
    re, im = phi.real.astype(LD), phi.imag.astype(LD)
    w = np.full(len(phi), LD(1) / len(phi)) if weights is None else np.asarray(weights, dtype=LD)
    rr = sum(wb * (np.outer(a, a) + np.outer(b, b)) for wb, a, b in zip(w, re, im)) * LD(h)
    ri = sum(wb * (np.outer(b, a) - np.outer(a, b)) for wb, a, b in zip(w, re, im)) * LD(h)
    return rr, ri


@pytest.mark.parametrize("X,P", [(17, 5), (64, 16), (65, 17)])
def test_pure_states_and_mixtures_equal_the_wavefunctions_restatement(X, P):
    phi, h = states(3, X, 7 + X)
    p = np.linspace(-0.9 * np.pi / h, 0.9 * np.pi / h, P)
    Wphi = R.wigner_longdouble(phi, h, p)
    # both sides are longdouble sums of the same terms: 2^-11 of the float64 bound each
    tol = R.wigner_bound(phi, h, p) * 2.0 ** -10
    for b in range(3):
        W = PR.wigner_of_longdouble(pure_longdouble(phi[b:b + 1], h), h, p)[0]
        assert np.all(np.abs(W - Wphi[b]) <= tol[b])
    w = np.array([0.5, 0.3, 0.2])
    W = PR.wigner_of_longdouble(pure_longdouble(phi, h, w), h, p)[0]
    want = sum(LD(wb) * Wb for wb, Wb in zip(w, Wphi))
    assert np.all(np.abs(W - want) <= (w[:, None, None] * tol).sum(axis=0) * 2)
    # float64 evaluation of the formula on the rounded mean rho against the mean of the states' W
    rho = PR.pure(phi, h).mean(axis=0)
    err = np.abs(PR.wigner_of_float64(rho, h, p)[0] - Wphi.mean(axis=0)).astype(np.float64)
    print(f"x_n={X} P={P}: float64 formula against the states' mean: {err.max():.2e}")
    assert err.max() < 4e-15


def test_position_marginal_on_a_full_period():
    X = 33
    rho = PR.random_hermitian(2, X, 5)
    h = 6. / (X - 1)
    for P in (X, 2 * X + 1):
        # (the phases are 2 p k h: W has the period pi / h in p, half the allowed range)
        p = -np.pi / (2 * h) + np.pi / (P * h) * np.arange(P)
        W = PR.wigner_of_longdouble(rho, h, p)
        marginal = W.sum(axis=2) * LD(np.pi / (P * h))
        want = np.diagonal(rho, axis1=1, axis2=2).real / h
        assert np.max(np.abs(marginal - want)) < 1e-13 * np.abs(want).max()


def fock_route(rho):
    E = SR.table_longdouble(rho.shape[-1], DRIVER_GRID)
    h = 28. / 249
    return PR.wigner_of_longdouble(PR.congruence_longdouble(E, rho, h), h, DEFAULT_P)[0], h


def test_closed_forms_through_the_fock_route():
    W0, _ = fock_route(np.array([[1.]], dtype=np.complex128))
    assert np.max(np.abs(W0 - R.fock_wigner(0, DRIVER_GRID, DEFAULT_P))) < 1e-15
    Wm, _ = fock_route(np.diag([0.5, 0.5]).astype(np.complex128))
    want = (R.fock_wigner(0, DRIVER_GRID, DEFAULT_P) + R.fock_wigner(1, DRIVER_GRID, DEFAULT_P)) / 2
    assert np.max(np.abs(Wm - want)) < 1e-15
    c, rho = coherent(1.1 - 0.7j, 60)
    Wc, _ = fock_route(rho)
    want = R.gaussian_wigner(DRIVER_GRID, DEFAULT_P, x0=np.sqrt(2) * 1.1, p0=np.sqrt(2) * -0.7)
    print(f"coherent state: {float(np.max(np.abs(Wc - want))):.2e}")
    assert np.max(np.abs(Wc - want)) < 1e-14


def coherent(alpha, n):
    """(c [n], rho = c c^†) of the coherent state |alpha> cut at n levels: <x> = sqrt(2) Re alpha, <p> = sqrt(2) Im
    alpha."""
    c = np.zeros(n, dtype=np.complex128)
    c[0] = np.exp(-abs(alpha) ** 2 / 2)
    for k in range(1, n):
        c[k] = c[k - 1] * alpha / np.sqrt(k)
    return c, np.outer(c, c.conj())


@pytest.mark.parametrize("X,P", [(17, 5), (64, 16), (65, 17), (250, 16)])
def test_float64_evaluation_lies_within_the_bound(X, P):
    rho = PR.random_hermitian(3, X, 30 + X)
    h = 6. / (X - 1)
    p = np.linspace(-0.999 * np.pi / h, 0.999 * np.pi / h, P)
    err = np.abs(PR.wigner_of_float64(rho, h, p) - PR.wigner_of_longdouble(rho, h, p)).astype(np.float64)
    bound = PR.wigner_of_bound(rho, h, p)
    print(f"x_n={X} P={P}: max err {err.max():.2e}, max err/bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)


def test_the_mistakes_move_w_by_a_thousand_bounds():
    X = P = 17
    rho = PR.random_hermitian(2, X, 91, zero_tails=False)
    h = 6. / (X - 1)
    p = np.linspace(-0.9 * np.pi / h, 0.8 * np.pi / h, P)
    W = PR.wigner_of_longdouble(rho, h, p)
    floor = 1000 * PR.wigner_of_bound(rho, h, p).max()
    mistakes = {
        "upper triangle": PR.wigner_of_longdouble(rho.transpose(0, 2, 1), h, p),
        "dropped h": PR.wigner_of_longdouble(rho / h, h, p),
        "factor 2 in the angle": PR.wigner_of_longdouble(rho, h / 2, p),
        "transposed output": W.transpose(0, 2, 1),
    }
    for name, wrong in mistakes.items():
        moved = float(np.max(np.abs(wrong - W)))
        print(f"{name}: moves W by {moved:.2e} (floor {floor:.2e})")
        assert moved >= floor, name


def test_congruence_restatement_and_bound():
    """sigma = h Phi rho Phi^T of a pure Fock state is h phi phi^† of its wavefunction, and a float64 evaluation lies
    within (2 n + 8) 2^-53 h (|Phi| |rho| |Phi|^T)."""
    n = 17
    E = SR.table_longdouble(n, DRIVER_GRID)
    rng = np.random.default_rng(3)
    c = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    c /= np.linalg.norm(c)
    rho = np.outer(c, c.conj())
    h = 28. / 249
    sr, si = PR.congruence_longdouble(E, rho, h)
    re, im = SR.repr_longdouble(E, c[None])
    want_r = LD(h) * (np.outer(re[0], re[0]) + np.outer(im[0], im[0]))
    want_i = LD(h) * (np.outer(im[0], re[0]) - np.outer(re[0], im[0]))
    bound = PR.congruence_bound(E, rho, h)[0]
    # (rho is the rounded outer product: 2^-53 relative per element, inside the bound's (2 n + 8))
    assert np.all(np.abs(sr[0] - want_r) <= bound) and np.all(np.abs(si[0] - want_i) <= bound)
    Ed = E.astype(np.float64)
    got = h * (Ed @ rho @ Ed.T)
    err = np.maximum(np.abs(got.real - sr[0]), np.abs(got.imag - si[0])).astype(np.float64)
    print(f"float64 congruence: max err/bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
