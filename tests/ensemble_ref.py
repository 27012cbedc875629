"""The ensemble density matrix restated in numpy extended precision (np.longdouble / np.clongdouble): the sum of the
live envs' outer products, times scale, divided by their count; the a-priori bound the device is held to; and the
documented number of splits."""
import numpy as np

LD = np.longdouble


def splits(B: int, N: int) -> int:
    """S = min(ceil(B / 2), 256, max(1, floor(2^22 / N^2))) (include/qcart.h)."""
    return min((B + 1) // 2, 256, max(1, 2 ** 22 // (N * N)))


def density_longdouble(psi, mask=None, scale=1.0):
    """(rho [N, N] clongdouble, count): rho_mn = scale * sum_live psi_b[m] conj(psi_b[n]) / count; count 0: zeros."""
    psi = np.asarray(psi, dtype=np.complex128)
    if psi.ndim == 1:
        psi = psi[None]
    live = psi if mask is None else psi[np.asarray(mask, dtype=bool)]
    n, N = live.shape
    rho = np.zeros((N, N), dtype=np.clongdouble)
    if n == 0:
        return rho, 0
    a, b = live.real.astype(LD), live.imag.astype(LD)
    rho.real = a.T @ a + b.T @ b
    rho.imag = b.T @ a - a.T @ b
    return rho * LD(scale) / LD(n), n


def magnitude_sum(psi, mask=None):
    """T_mn = sum_live |psi_b[m]| |psi_b[n]| (float64: it only scales the bound)."""
    psi = np.asarray(psi, dtype=np.complex128)
    if psi.ndim == 1:
        psi = psi[None]
    live = np.abs(psi if mask is None else psi[np.asarray(mask, dtype=bool)])
    return live.T @ live


def bound(psi, mask=None, scale=1.0, S=None):
    """sqrt(2) (2 B + S + 4) 2^-53 scale T_mn / count per element: 2 B products per real part with
    |a_m a_n| + |b_m b_n| <= |psi_m| |psi_n|, S split additions, the scaling and the division, sqrt(2) for the modulus.
    B is the batch (masked envs are zero operands of the same chain)."""
    psi = np.asarray(psi)
    B, N = (1, psi.shape[0]) if psi.ndim == 1 else psi.shape
    count = B if mask is None else int(np.asarray(mask, dtype=bool).sum())
    if count == 0:
        return np.zeros((N, N))
    S = splits(B, N) if S is None else S
    return np.sqrt(2.0) * (2 * B + S + 4) * 2.0 ** -53 * scale * magnitude_sum(psi, mask) / count
