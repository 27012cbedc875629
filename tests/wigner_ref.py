"""Restatements for the phase-space view's tests (csrc/qcart_wigner.hpp, csrc/qcart_wigner.hip), written for the tests
from the definition in include/qcart.h alone.

`wigner_longdouble` is the lag sum in numpy longdouble, `wigner_bound` the a-priori bound on a float64 evaluation in
any order with a table within 2^-53 + 2^-62 |a| of the exact one, `table_mp` the table in mpmath. The closed forms
(Gaussians, Fock states via Laguerre polynomials) are here too; tests/test_wigner_cpu.py checks the restatement
against them."""
import numpy as np

LD = np.longdouble
PI = LD("3.14159265358979323846264338327950288")


def lags(x_n):
    """K_i = min(i, x_n - 1 - i)."""
    i = np.arange(x_n)
    return np.minimum(i, x_n - 1 - i)


def wigner_longdouble(phi, h, p):
    """W [B][X][P] in longdouble from phi [B][X] complex128, the spacing h and the momenta p (float64, taken
    exactly): (h / pi) (|phi_i|^2 + 2 sum_{k = 1 .. K_i} (Re c_ik cos(2 p_j k h) - Im c_ik sin(2 p_j k h))),
    c_ik = conj(phi_{i+k}) phi_{i-k}. phi may also be a pair (Re, Im) of longdouble arrays."""
    if isinstance(phi, tuple):
        re, im = np.atleast_2d(phi[0]).astype(LD), np.atleast_2d(phi[1]).astype(LD)
    else:
        phi = np.atleast_2d(phi)
        re, im = phi.real.astype(LD), phi.imag.astype(LD)
    B, X = re.shape
    pl = np.asarray(p, dtype=np.float64).astype(LD)
    a1 = 2 * pl * LD(h)
    W = np.zeros((B, X, pl.size), dtype=LD)
    W += (re * re + im * im)[:, :, None]
    for k in range(1, (X - 1) // 2 + 1):
        up_r, up_i = re[:, 2 * k:], im[:, 2 * k:]               # phi_{i+k} for i = k .. X - 1 - k
        dn_r, dn_i = re[:, :X - 2 * k], im[:, :X - 2 * k]       # phi_{i-k}
        c_re = up_r * dn_r + up_i * dn_i
        c_im = up_r * dn_i - up_i * dn_r
        ang = a1 * k
        W[:, k:X - k, :] += 2 * (c_re[:, :, None] * np.cos(ang) - c_im[:, :, None] * np.sin(ang))
    return W * (LD(h) / PI)


def wigner_terms(phi):
    """S [B][X] = |phi_i|^2 + 4 sum_k |phi_{i+k}| |phi_{i-k}| in float64."""
    phi = np.atleast_2d(phi)
    X = phi.shape[1]
    mag = np.abs(phi)
    S = mag * mag
    for k in range(1, (X - 1) // 2 + 1):
        S[:, k:X - k] += 4 * mag[:, 2 * k:] * mag[:, :X - 2 * k]
    return S


def wigner_bound(phi, h, p):
    """bound [B][X][P] = (h / pi) S_i ((2 K_i + 8) 2^-53 + 2 |p_j| h K_i 2^-62)."""
    phi = np.atleast_2d(phi)
    K = lags(phi.shape[1]).astype(np.float64)
    S = wigner_terms(phi)
    ap = np.abs(np.asarray(p, dtype=np.float64))
    fac = (2 * K + 8)[:, None] * 2.0 ** -53 + 2 * ap[None, :] * h * K[:, None] * 2.0 ** -62
    return (h / np.pi) * S[:, :, None] * fac[None]


def cross_terms(mag, delta):
    """[B][X]: 4 sum_k (|phi_{i+k}| delta_{i-k} + |phi_{i-k}| delta_{i+k}), the first-order change of the lag sum when
    every phi_i moves by at most delta_i."""
    X = mag.shape[1]
    out = np.zeros_like(mag)
    for k in range(1, (X - 1) // 2 + 1):
        out[:, k:X - k] += 4 * (mag[:, 2 * k:] * delta[:, :X - 2 * k] + mag[:, :X - 2 * k] * delta[:, 2 * k:])
    return out


def table_mp(x_n, h, p, dps=60):
    """[k - 1][j] -> (cos, sin)(2 p_j h k) as mpmath numbers, k = 1 .. (x_n - 1) // 2; h and p are floats, taken
    exactly. Also the angles."""
    import mpmath as mp
    with mp.workdps(dps):
        rows, angles = [], []
        for k in range(1, (x_n - 1) // 2 + 1):
            a = [2 * mp.mpf(float(pj)) * mp.mpf(float(h)) * k for pj in p]
            angles.append(a)
            rows.append([(mp.cos(v), mp.sin(v)) for v in a])
        return rows, angles


# ---------------------------------------------------------------- closed forms (hbar = m = omega = 1)
def gaussian_packet(x, x0=0., p0=0., var=0.5):
    """The normalised Gaussian of position variance `var` at (x0, p0), complex128."""
    x = np.asarray(x, dtype=np.float64)
    return (2 * np.pi * var) ** -0.25 * np.exp(-(x - x0) ** 2 / (4 * var) + 1j * p0 * x)


def gaussian_wigner(x, p, x0=0., p0=0., var=0.5):
    """(1 / pi) exp(-(x - x0)^2 / (2 var) - 2 var (p - p0)^2): the minimum-uncertainty packet's Wigner function."""
    x, p = np.asarray(x, dtype=LD)[:, None], np.asarray(p, dtype=LD)[None, :]
    return np.exp(-(x - x0) ** 2 / (2 * LD(var)) - 2 * LD(var) * (p - p0) ** 2) / PI


def laguerre(n, z):
    """L_n(z) by (m + 1) L_{m+1} = (2 m + 1 - z) L_m - m L_{m-1}, in z's arithmetic."""
    prev, cur = z * 0 + 1, 1 - z
    if n == 0:
        return prev
    for m in range(1, n):
        prev, cur = cur, ((2 * m + 1 - z) * cur - m * prev) / (m + 1)
    return cur


def fock_wigner(n, x, p):
    """((-1)^n / pi) exp(-r^2) L_n(2 r^2), r^2 = x^2 + p^2."""
    x, p = np.asarray(x, dtype=LD)[:, None], np.asarray(p, dtype=LD)[None, :]
    r2 = x * x + p * p
    return (-1) ** n * np.exp(-r2) * laguerre(n, 2 * r2) / PI


def momentum_density(phi, x, p):
    """|phi~(p_j)|^2, phi~(p) = h / sqrt(2 pi) sum_i phi_i e^{-i p x_i}, in longdouble."""
    x, pl = np.asarray(x, dtype=LD), np.asarray(p, dtype=LD)
    h = (x[-1] - x[0]) / (x.size - 1)
    ang = pl[:, None] * x[None, :]
    c, s = np.cos(ang), np.sin(ang)
    re, im = phi.real.astype(LD), phi.imag.astype(LD)
    fr = c @ re + s @ im            # Re sum phi (cos - i sin)
    fi = c @ im - s @ re
    return (fr * fr + fi * fi) * h * h / (2 * PI)
