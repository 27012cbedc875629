"""Restatements for the tests of the phase-space view of density matrices (csrc/qcart_phase.hip,
WignerView.wigner_of, SpatialView.density_matrix_of), written from the definitions in include/qcart.h alone.

`wigner_of_longdouble` is the lag sum over the LOWER triangle of a grid density matrix in numpy longdouble,
    W[i][j] = (1 / pi) (Re rho_ii + 2 sum_{k = 1 .. K_i} (Re L_ik cos(2 p_j k h) + Im L_ik sin(2 p_j k h))),
    L_ik = rho[i + k][i - k],  K_i = min(i, x_n - 1 - i),
`wigner_of_bound` the a-priori bound on a float64 evaluation in any order with a table within 2^-53 + 2^-62 |a| of the
exact one (2 K_i + 2 accumulations, one table rounding, the scale and the product by fl(2 / pi)),
    bound_ij = (1 / pi) S_i ((2 K_i + 8) 2^-53 + 2 |p_j| h K_i 2^-62),   S_i = |Re rho_ii| + 2 sum_k (|Re L_ik| + |Im L_ik|),
`congruence_longdouble` the change of basis sigma = h Phi rho Phi^T and `congruence_bound` its bound
(2 n + 8) 2^-53 h (|Phi| |rho| |Phi|^T). tests/test_phase_cpu.py checks them against tests/wigner_ref.py and the closed
forms."""
import numpy as np

from tests.wigner_ref import LD, PI, lags


def lower_antidiagonals(rho):
    """(re, im) [M][X][Kmax + 1] float64: L_ik = rho[i + k][i - k] for k <= K_i, zero beyond; im of k = 0 is zero (the
    imaginary part of the diagonal is ignored)."""
    rho = np.asarray(rho)
    rho = rho[None] if rho.ndim == 2 else rho
    M, X, _ = rho.shape
    kmax = (X - 1) // 2
    re, im = np.zeros((M, X, kmax + 1)), np.zeros((M, X, kmax + 1))
    i = np.arange(X)
    re[:, :, 0] = rho[:, i, i].real
    for k in range(1, kmax + 1):
        ii = np.arange(k, X - k)
        re[:, ii, k] = rho[:, ii + k, ii - k].real
        im[:, ii, k] = rho[:, ii + k, ii - k].imag
    return re, im


def wigner_of_longdouble(rho, h, p):
    """W [M][X][P] in longdouble from rho [M][X][X] complex128 (or (Re, Im) longdouble arrays of that shape), the
    spacing h and the momenta p (float64, taken exactly). Only elements with row >= col are read."""
    if isinstance(rho, tuple):
        rr, ri = (np.asarray(a, dtype=LD) for a in rho)
    else:
        rho = np.asarray(rho)
        rr, ri = rho.real.astype(LD), rho.imag.astype(LD)
    if rr.ndim == 2:
        rr, ri = rr[None], ri[None]
    M, X, _ = rr.shape
    pl = np.asarray(p, dtype=np.float64).astype(LD)
    a1 = 2 * pl * LD(h)
    i = np.arange(X)
    W = np.zeros((M, X, pl.size), dtype=LD)
    W += rr[:, i, i][:, :, None]
    for k in range(1, (X - 1) // 2 + 1):
        ii = np.arange(k, X - k)
        ang = a1 * k
        W[:, k:X - k, :] += 2 * (rr[:, ii + k, ii - k][:, :, None] * np.cos(ang)
                                 + ri[:, ii + k, ii - k][:, :, None] * np.sin(ang))
    return W / PI


def wigner_of_terms(rho):
    """S [M][X] = |Re rho_ii| + 2 sum_k (|Re L_ik| + |Im L_ik|) in float64."""
    re, im = lower_antidiagonals(rho)
    return np.abs(re[:, :, 0]) + 2 * (np.abs(re[:, :, 1:]) + np.abs(im[:, :, 1:])).sum(axis=2)


def wigner_of_bound(rho, h, p, extra=0.):
    """bound [M][X][P] = (1 / pi) S_i ((2 K_i + 8 + extra) 2^-53 + 2 |p_j| h K_i 2^-62)."""
    S = wigner_of_terms(rho)
    K = lags(S.shape[1]).astype(np.float64)
    ap = np.abs(np.asarray(p, dtype=np.float64))
    fac = (2 * K + 8 + extra)[:, None] * 2.0 ** -53 + 2 * ap[None, :] * h * K[:, None] * 2.0 ** -62
    return (1 / np.pi) * S[:, :, None] * fac[None]


def wigner_of_float64(rho, h, p):
    """The formula in plain numpy float64, with the library's kind of table: cos / sin of the longdouble angle,
    rounded once."""
    re, im = lower_antidiagonals(rho)
    k = np.arange(re.shape[2])
    ang = 2 * np.asarray(p, dtype=np.float64).astype(LD)[None, :] * LD(h) * k[:, None]
    C, S = np.cos(ang).astype(np.float64), np.sin(ang).astype(np.float64)
    C[0] = 0.5
    S[0] = 0.
    return (2 / np.pi) * (re @ C + im @ S)


def pure(phi, h):
    """rho = h phi phi^† [M][X][X] complex128 of wavefunctions phi [M][X]."""
    phi = np.atleast_2d(phi)
    return h * phi[:, :, None] * phi[:, None, :].conj()


def congruence_longdouble(Phi, rho, h):
    """(Re, Im) longdouble [M][X][X] of sigma = h Phi[:, :n] rho Phi[:, :n]^T; Phi real (any float type), rho
    complex128 [M][n][n] or a (Re, Im) pair of longdouble arrays."""
    if isinstance(rho, tuple):
        rr, ri = (np.asarray(a, dtype=LD) for a in rho)
    else:
        rho = np.asarray(rho)
        rr, ri = rho.real.astype(LD), rho.imag.astype(LD)
    if rr.ndim == 2:
        rr, ri = rr[None], ri[None]
    n = rr.shape[1]
    F = np.asarray(Phi, dtype=LD)[:, :n]
    Ft = np.ascontiguousarray(F.T)
    return (np.stack([LD(h) * (F @ r @ Ft) for r in rr]), np.stack([LD(h) * (F @ r @ Ft) for r in ri]))


def congruence_bound(Phi, rho, h):
    """(2 n + 8) 2^-53 h (|Phi| |rho| |Phi|^T) [M][X][X] float64."""
    rho = np.asarray(rho)
    rho = rho[None] if rho.ndim == 2 else rho
    n = rho.shape[1]
    F = np.abs(np.asarray(Phi, dtype=np.float64)[:, :n])
    return (2 * n + 8) * 2.0 ** -53 * h * np.stack([F @ np.abs(r) @ F.T for r in rho])


def random_hermitian(M, X, seed, zero_tails=True):
    """Seeded random Hermitian [M][X][X] complex128 of unit trace (not positive: the kernels do not care); every odd
    matrix has zero tails (only a middle window of rows and columns is set)."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((M, X, X)) + 1j * rng.standard_normal((M, X, X))
    rho = a + a.conj().transpose(0, 2, 1)
    if zero_tails:
        lo, hi = X // 4, X - X // 3
        if hi - lo >= 1:
            rho[1::2, :lo, :] = 0
            rho[1::2, hi:, :] = 0
            rho[1::2, :, :lo] = 0
            rho[1::2, :, hi:] = 0
    i = np.arange(X)
    rho[:, i, i] = np.abs(rho[:, i, i].real) + 0.1
    tr = rho[:, i, i].real.sum(axis=1)
    return np.ascontiguousarray(rho / tr[:, None, None])


def negative_volume_longdouble(W, h, dp):
    """sum max(-W, 0) h dp over the last two axes, in longdouble."""
    W = np.asarray(W, dtype=LD)
    return np.where(W < 0, -W, LD(0)).sum(axis=(-2, -1)) * LD(h) * LD(dp)
