"""Restatements for the position-space view's tests (csrc/qcart_spatial.hpp, csrc/qcart_spatial.hip), written for the
tests from the definitions alone.

`eigenfunctions` is the table E[j][n] = psi_n(x_j) of the normalised harmonic-oscillator eigenfunctions (hbar = m =
omega = 1) in any arithmetic handed to it: mpmath numbers at >= 60 digits for the table's check, numpy longdouble
arrays for the wide checks. Its conventions are tested against closed forms in tests/test_spatial_cpu.py.
`mean_in_documented_order` is the order of qc_spatial_mean as include/qcart.h states it, in numpy float64."""
import numpy as np

GROUP = 32


def eigenfunctions(n_levels, x, sqrt, exp, pi):
    """[psi_0(x), .., psi_{n_levels - 1}(x)] (x a number or an array) by psi_0 = pi^(-1/4) exp(-x^2 / 2),
    psi_1 = sqrt(2) x psi_0, psi_{n+1} = sqrt(2 / (n + 1)) x psi_n - sqrt(n / (n + 1)) psi_{n-1}."""
    one = x * 0 + 1
    out = [one / sqrt(sqrt(pi * one)) * exp(-x * x / 2)]
    if n_levels > 1:
        out.append(sqrt(2 * one) * x * out[0])
    for n in range(1, n_levels - 1):
        out.append(sqrt(2 * one / (n + 1)) * x * out[n] - sqrt(n * one / (n + 1)) * out[n - 1])
    return out


def table_mp(n_levels, xs, dps=60):
    """The table as a list (points) of lists (levels) of mpmath numbers; xs are floats, taken exactly."""
    import mpmath as mp
    with mp.workdps(dps):
        return [eigenfunctions(n_levels, mp.mpf(float(x)), mp.sqrt, mp.exp, mp.pi) for x in xs]


def table_longdouble(n_levels, xs):
    """The table [X][n_levels] in numpy longdouble (x86: 64-bit mantissa)."""
    x = np.asarray(xs, dtype=np.float64).astype(np.longdouble)
    pi = np.longdouble("3.14159265358979323846264338327950288")
    return np.stack(eigenfunctions(n_levels, x, np.sqrt, np.exp, pi), axis=1)


def repr_longdouble(E_ld, psi):
    """phi [B][X] as two longdouble arrays (Re, Im): E_ld[:, :n_state] against the complex128 states, summed in
    longdouble."""
    n = psi.shape[1]
    Et = np.ascontiguousarray(E_ld[:, :n].T)
    return psi.real.astype(np.longdouble) @ Et, psi.imag.astype(np.longdouble) @ Et


def repr_bound(E_ld, psi):
    """The a-priori bound on |phi - phi_exact| per element [B][X] for any summation order in fp64 with a table within
    2^-52 of the exact one: (n_state + 2) 2^-53 sum_n |E_jn| (|Re c_n| + |Im c_n|) + 2^-52 sum_n |c_n|."""
    n = psi.shape[1]
    absE = np.abs(E_ld[:, :n]).astype(np.float64)
    return (n + 2) * 2.0 ** -53 * ((np.abs(psi.real) + np.abs(psi.imag)) @ absE.T) \
        + 2.0 ** -52 * np.abs(psi).sum(axis=1)[:, None]


def mean_in_documented_order(p, mask=None):
    """(m [X], count) from the per-env densities p [B][X] float64 in qc_spatial_mean's order: groups of 32 envs (envs
    past B and masked envs enter as +0); in a group s[q] = the running sum from +0 of the envs q, q + 4, .., q + 28,
    the partial (s[0] + s[1]) + (s[2] + s[3]); r[t] = the running sum from +0 of the partials of the groups t, t + 4,
    ..; m = ((r[0] + r[1]) + (r[2] + r[3])) / count."""
    p = np.asarray(p, dtype=np.float64)
    B, X = p.shape
    live = np.ones(B, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    groups = -(-B // GROUP)
    padded = np.zeros((groups * GROUP, X))
    padded[:B][live] = p[live]
    r = np.zeros((4, X))
    for g in range(groups):
        rows = padded[g * GROUP:(g + 1) * GROUP].reshape(GROUP // 4, 4, X)
        s = np.zeros((4, X))
        for i in range(GROUP // 4):
            s = s + rows[i]
        r[g % 4] = r[g % 4] + ((s[0] + s[1]) + (s[2] + s[3]))
    total = (r[0] + r[1]) + (r[2] + r[3])
    count = int(live.sum())
    return (total / np.float64(count) if count else np.zeros(X)), count
