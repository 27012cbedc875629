"""The conditional master equation restated in numpy longdouble (include/qcart.h "conditional master equation",
csrc/qcart_filter.hip): one step and n steps on given tables with given (u, z) or a given record y, a plain ascending
prefix sum, the relative margin of every pick, and the a-priori elementwise error bound of the device's fp64 evaluation
(DESIGN §9n):
    congruence    (4 N + 16) eps g (|T| |sigma| |T|^T) per step (tests/lindblad_ref.congruence_ld's bound);
    conditioning  (N + 68 a e_max + 16) eps |sigma'_ij|, e_max the largest (xi_i - y)^2 the step saw;
    carried over  an earlier error E goes through a step as (v_i v_j) g (|T| E |T|^T) + |sigma'| sum_i w_i^2 E_ii / Z
                  (the second term: the normalisation Z is a sum over the diagonal, which carries E too).
`dtype` np.complex128 evaluates the same scheme in fp64 (the picks and the conditioning stay longdouble on the
diagonal): the CPU twin, and the reference of the sizes whose longdouble products take minutes."""
import ctypes

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
EPS = 2.0 ** -53


def absum(a):
    return np.abs(a.real).astype(np.float64) + np.abs(a.imag).astype(np.float64)


def congruence(A, s, g=None):
    y = A @ s @ A.conj().T
    return y if g is None else g.astype(y.real.dtype) * y


def constants(eta, gamma, dt):
    """(a, s) in longdouble: a = eta gamma dt / 2, s = 1 / sqrt(4 a)."""
    a = LD(eta) * LD(gamma) * LD(dt) / 2
    return a, 1 / np.sqrt(4 * a)


def g_power(xi_ld, dt, gamma, power):
    """G^power in longdouble from the longdouble xi: exp(-gamma power dt (xi_i - xi_j)^2 / 4)."""
    x = np.asarray(xi_ld, dtype=LD)
    return np.exp(-(LD(gamma) * LD(power) * LD(dt)) * (x[:, None] - x[None, :]) ** 2 / 4)


def measure(p, xi, a, u=None, z=None, y=None):
    """Steps 2-3 on the propagated sigma p: dict(sigma, y, I, margin, e_max, v, Z, w, d). Raises ValueError where the
    device marks the matrix dead."""
    xi = np.asarray(xi, dtype=LD)
    d = np.maximum(np.asarray(p.diagonal().real, dtype=LD), 0)
    c = np.cumsum(d)
    if not (np.isfinite(c[-1]) and c[-1] > 0):
        raise ValueError("c_(N-1)")
    I, margin = -1, np.inf
    if y is None:
        thr = LD(u) * c[-1]
        I = int(np.argmax(c > thr))
        margin = float(np.abs(thr - c).min() / c[-1])
        y = xi[I] + LD(z) / np.sqrt(4 * LD(a))
    y = LD(y)
    if not np.isfinite(y):
        raise ValueError("y")
    e = (xi - y) ** 2
    w = np.exp(-LD(a) * (e - e.min()))
    Z = (w * w * d).sum()
    if not (np.isfinite(Z) and Z > 0):
        raise ValueError("Z")
    v = w / np.sqrt(Z)
    vv = v[:, None] * v[None, :]
    return dict(sigma=vv.astype(p.real.dtype) * p, y=y, I=I, margin=margin, e_max=float(e.max()), v=v, Z=Z, w=w, d=d,
                vv=vv.astype(np.float64))


def step(s, T, g, xi, a, u=None, z=None, y=None, E=None):
    """One conditional step of sigma s; E: the error bound s carries (None: exact). Adds 'bound' to measure's dict."""
    N = s.shape[0]
    p = congruence(T, s, g)
    Tb = absum(T)
    gg = 1.0 if g is None else np.abs(g).astype(np.float64)
    b = (4 * N + 16) * EPS * gg * (Tb @ absum(s) @ Tb.T)
    if E is not None:
        b = b + gg * (Tb @ E @ Tb.T)
    m = measure(p, xi, a, u, z, y)
    after = absum(m["sigma"])
    carried = float(((m["w"] ** 2).astype(np.float64) * np.diag(b)).sum() / float(m["Z"]))
    m["bound"] = m["vv"] * b + after * carried + (N + 68 * float(a) * m["e_max"] + 16) * EPS * after
    return m


def evolve(rho, n, tab, g, a, fock, draws=None, record=None, dtype=CLD, E0=None):
    """n conditional steps of one rho on the tables tab (xi, W, T) with g = G^(1-eta) (None at eta = 1); draws [n, 2]
    or record [n]; E0: the elementwise error bound rho itself carries (None: exact). dict(rho, y [n], I [n],
    margin [n], bound [N, N], e_max)."""
    N = rho.shape[0]
    T, W = tab["T"].astype(dtype), tab["W"].astype(dtype)
    s = np.asarray(rho).astype(dtype)
    E = np.zeros((N, N)) if E0 is None else np.asarray(E0, dtype=np.float64)
    Wb = np.abs(tab["W"])
    if fock:
        E = Wb.T @ E @ Wb + (4 * N + 16) * EPS * (Wb.T @ absum(s) @ Wb)
        s = W.T @ s @ W
    ys, Is, margins, e_max = [], [], [], 0.0
    for k in range(n):
        m = step(s, T, g, tab["xi"], a, *(draws[k] if draws is not None else (None, None)),
                 y=None if record is None else record[k], E=E)
        s, E = m["sigma"], m["bound"]
        ys.append(m["y"])
        Is.append(m["I"])
        margins.append(m["margin"])
        e_max = max(e_max, m["e_max"])
    if fock:
        E = Wb @ E @ Wb.T + (4 * N + 16) * EPS * (Wb @ absum(s) @ Wb.T)
        s = W @ s @ W.T
    return dict(rho=s, y=np.array(ys, dtype=LD), I=np.array(Is), margin=np.array(margins), bound=E, e_max=e_max)


def unconditional(rho, n, tab, g_full, fock, dtype=np.complex128):
    """(G o T . T^†)^n in evolve's basis: what the mean over records of n conditional steps is, exactly."""
    T, W = tab["T"].astype(dtype), tab["W"].astype(dtype)
    s = np.asarray(rho).astype(dtype)
    if fock:
        s = W.T @ s @ W
    for _ in range(n):
        s = congruence(T, s, g_full)
    return W @ s @ W.T if fock else s


def host_draws(lib, seed, stream, step):
    """(u, z) of the library's host mirror of the device's Philox draws."""
    u, z = ctypes.c_double(), ctypes.c_double()
    assert lib.qc_lindblad_filter_draws(seed, stream, step, ctypes.byref(u), ctypes.byref(z)) == 0
    return u.value, z.value


def philox_draws(lib, seed, streams, first_step, n):
    """[n, M, 2] of the host mirror."""
    return np.array([[host_draws(lib, seed, int(s), first_step + k) for s in streams] for k in range(n)])


def twin_infidelity(ph, psi0, action, noise, substeps=1):
    """The CPU twin of the filter-against-stepper check: the oracle steps psi0 under noise [n, B, 2] at dt / substeps
    (one control force), the restatement (fp64 products) filters |psi0><psi0| at eta = 1 on the oracle's own record q
    with lindblad_ref's numpy tables; the infidelities 1 - <psi_b| rho_b |psi_b> [B]."""
    from oracle import oracle as O
    from tests import lindblad_ref as R
    dt, force = ph.dt / substeps, ph.force(action)
    H, X, c, fock = R.operators(ph)
    tab = R.tables(H, X, c, force, dt, ph.gamma, fock)
    a, _ = constants(1.0, ph.gamma, dt)
    system = O.OracleSystem(ph.family, n_max=ph.n_max, omega=ph.omega)
    out = []
    for b in range(noise.shape[1]):
        psi = np.array(psi0, dtype=np.complex128)
        q = [system.step(psi, dt, force, ph.gamma, noise[k, b])[0] for k in range(noise.shape[0])]
        rho = evolve(np.outer(psi0, np.conj(psi0)), len(q), tab, None, a, fock, record=np.array(q),
                     dtype=np.complex128)["rho"]
        psi = psi / np.linalg.norm(psi)
        out.append(1 - float(np.real(np.conj(psi) @ rho @ psi)))
    return np.array(out)
