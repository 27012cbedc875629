"""The energy-level view's definitions (include/qcart.h, qc_levels) in numpy: the amplitudes in longdouble with the
a-priori bound the device is held to, the populations' formula, and the mean's documented order restated operation by
operation in float64."""
import numpy as np

EPS = 2.0 ** -53


def amplitudes_longdouble(psi, V, scale=1.0):
    """a[b][k] = scale * sum_j V[k][j] psi_b[j], each part in longdouble."""
    psi = np.asarray(psi)
    Vl = np.asarray(V, dtype=np.longdouble)
    re = psi.real.astype(np.longdouble) @ Vl.T
    im = psi.imag.astype(np.longdouble) @ Vl.T
    return np.longdouble(scale) * re, np.longdouble(scale) * im


def bound(psi, V, scale=1.0):
    """(N + 4) 2^-53 scale sum_j |V[k][j]| |part psi_b[j]| for the real and the imaginary part: N - 1 additions and N
    products of the sum in any order, the scaling and the comparison's own roundings."""
    psi = np.asarray(psi)
    n = psi.shape[-1]
    Va = np.abs(np.asarray(V, dtype=np.float64))
    return ((n + 4) * EPS * scale * (np.abs(psi.real) @ Va.T), (n + 4) * EPS * scale * (np.abs(psi.imag) @ Va.T))


def populations_of(a):
    """fl(fl(re * re) + fl(im * im)) of float64 amplitudes, every operation rounded once."""
    a = np.asarray(a)
    re, im = np.ascontiguousarray(a.real), np.ascontiguousarray(a.imag)
    return re * re + im * im


def join4(s):
    return (s[0] + s[1]) + (s[2] + s[3])


def mean_documented_order(p, mask=None):
    """(m [K], count) of per-env populations p [B][K] float64 by the order include/qcart.h documents: groups of 64
    envs, each of four sub-groups of 16; within a sub-group s[q] = the running sum, from +0, over its envs q, q + 4,
    q + 8, q + 12; the sub-group's sum (s0 + s1) + (s2 + s3); the group's partial the same join of its four sub-groups;
    r[t] = the running sum, from +0, of the partials of the groups t, t + 4, ..; m = ((r0 + r1) + (r2 + r3)) / count.
    A masked env and an env past B enter as +0."""
    p = np.asarray(p, dtype=np.float64)
    B, K = p.shape
    live = np.ones(B, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    count = int(live.sum())
    groups = (B + 63) // 64
    padded = np.zeros((groups * 64, K), dtype=np.float64)
    padded[:B][live] = p[live]
    r = [np.zeros(K, dtype=np.float64) for _ in range(4)]
    for g in range(groups):
        subs = []
        for u in range(4):
            base = 64 * g + 16 * u
            s = [np.zeros(K, dtype=np.float64) for _ in range(4)]
            for q in range(4):
                for i in range(4):
                    s[q] = s[q] + padded[base + q + 4 * i]
            subs.append(join4(s))
        r[g % 4] = r[g % 4] + join4(subs)
    m = join4(r)
    return (m / float(count) if count > 0 else np.zeros(K, dtype=np.float64)), count


def unit_rows(rng, K, N):
    """A random table: unit-norm Gaussian rows."""
    V = rng.standard_normal((K, N))
    return V / np.linalg.norm(V, axis=1, keepdims=True)


def residual(H, E, V):
    """max_k ||H v_k - E_k v_k||_inf in longdouble."""
    Hl = np.asarray(H, dtype=np.longdouble)
    Vl = np.asarray(V, dtype=np.longdouble)
    El = np.asarray(E, dtype=np.longdouble)
    return float(np.abs(Vl @ Hl.T - El[:, None] * Vl).max())


def norm_inf(H):
    return float(np.abs(np.asarray(H)).sum(axis=1).max())
