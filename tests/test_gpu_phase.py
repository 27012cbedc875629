"""The phase-space view of density matrices on the device (csrc/qcart_phase.hip; WignerView.wigner_of,
SpatialView.density_matrix_of, WignerView.negative_volume, Trainer.open_loop(wigner=...)).

`wigner_of` on a grid view against the longdouble restatement (tests/phase_ref.py) within the a-priori bound
    bound_ij = (1 / pi) S_i ((2 K_i + 8) 2^-53 + 2 |p_j| h K_i 2^-62),  S_i = |Re rho_ii| + 2 sum_k (|Re L_ik| + |Im L_ik|)
(largest error / bound seen on the device: printed by the test, recorded in DESIGN §9m), bit patterns (what is never
read, batch invariance, surroundings), the shipped paths (`wigner` of the pure state, `mean_wigner` against the ensemble
rho), the Fock route sigma = h Phi rho Phi^T within (2 n + 8) 2^-53 h (|Phi| |rho| |Phi|^T), the closed forms, the
physics, the loop and the refusals."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

from tests import phase_ref as PR
from tests import spatial_ref as SR
from tests import wigner_ref as R
from tests.checkpoint_loop import same_bits

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = 2.0 ** -53
DRIVER_GRID = np.linspace(-14, 14, 250)
DEFAULT_P = np.linspace(-12, 12, 193)
H250 = float((DRIVER_GRID[-1] - DRIVER_GRID[0]) / 249)


def _pkg():
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import _lib
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import config as cfg
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.ensemble import EnsembleView
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.lindblad import MasterEquation
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.spatial import SpatialView
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.wigner import WignerView
    return locals()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def grid(X):
    return np.linspace(-3, 3, X) if X > 1 else np.array([0.25])


def spacing(x):
    return float((x[-1] - x[0]) / (x.size - 1)) if x.size > 1 else 1.0


def momenta(h):
    """128 momenta over (almost) the whole allowed range |p| h <= pi in a fixed shuffled order, the largest first, so
    that the first P of them are a spread-out set for every P."""
    p = np.linspace(-0.999 * np.pi / h, 0.999 * np.pi / h, 128)
    order = np.random.default_rng(77).permutation(128)
    order = np.concatenate(([127], order[order != 127]))
    return p[order]


def ratio(err, bound):
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)))


_REF = {}


def reference(X):
    """Per x_n, once: 21 random Hermitian matrices (every odd one with zero tails), 128 momenta, the longdouble W and
    the bound; smaller M and P are prefixes."""
    if X not in _REF:
        x = grid(X)
        h = spacing(x)
        p = momenta(h)
        rho = PR.random_hermitian(21, X, 300 + X)
        _REF[X] = (x, h, p, rho, PR.wigner_of_longdouble(rho, h, p), PR.wigner_of_bound(rho, h, p))
    return _REF[X]


# ---------------------------------------------------------------- 1. wigner_of against the restatement
@pytest.mark.parametrize("P", [1, 16, 17, 65, 128])
@pytest.mark.parametrize("X", [1, 2, 16, 17, 64, 65, 250])
@pytest.mark.parametrize("M", [1, 2, 3, 21])
def test_wigner_of_equals_the_longdouble_restatement_within_the_bound(M, X, P):
    x, h, p, rho, W, bound = reference(X)
    view = _pkg()["WignerView"](x, p[:P])
    got = host(view.wigner_of(dev(rho[:M])))
    view.close()
    assert got.shape == (M, X, P) and got.dtype == np.float64
    err = np.abs(got - W[:M, :, :P]).astype(np.float64)
    b = bound[:M, :, :P]
    print(f"M={M} x_n={X} P={P}: max err {err.max():.3e}, max err/bound {ratio(err, b):.3f}")
    assert np.all(err <= b)
    # the edge rows have no lags: rho_ii / pi whatever p is
    edge = np.abs(np.diagonal(rho[:M], axis1=1, axis2=2).real[:, [0, -1]]) / np.pi
    assert np.all(np.abs(np.abs(got[:, [0, -1], :]) - edge[:, :, None]) <= 8 * EPS * edge[:, :, None])


def test_wigner_of_on_the_longest_grid():
    X, P = 4096, 2
    x = grid(X)
    h = spacing(x)
    p = momenta(h)[:P]
    rho = PR.random_hermitian(1, X, 4096, zero_tails=False)
    view = _pkg()["WignerView"](x, p)
    got = host(view.wigner_of(dev(rho)))
    view.close()
    err = np.abs(got - PR.wigner_of_longdouble(rho, h, p)).astype(np.float64)
    b = PR.wigner_of_bound(rho, h, p)
    print(f"x_n=4096: max err {err.max():.3e}, max err/bound {ratio(err, b):.3f}")
    assert got.shape == (1, X, P) and np.all(err <= b)


# ---------------------------------------------------------------- 2. bit patterns
@pytest.mark.parametrize("X,P", [(17, 5), (65, 17), (250, 65)])
def test_what_is_never_read_and_the_batch_do_not_matter(X, P):
    x, h, p, rho, _, _ = reference(X)
    view = _pkg()["WignerView"](x, p[:P])
    full = host(view.wigner_of(dev(rho)))
    # NaN in the strict upper triangle and in the diagonal's imaginary part
    poisoned = rho.copy()
    upper = np.triu(np.ones((X, X), dtype=bool), 1)
    poisoned[:, upper] = complex(np.nan, np.nan)
    i = np.arange(X)
    poisoned.imag[:, i, i] = np.nan
    # and in the lower triangle's elements of odd row - col, which belong to no (position, lag)
    odd = np.tril(np.ones((X, X), dtype=bool), -1) & (((i[:, None] - i[None, :]) % 2) == 1)
    poisoned[:, odd] = complex(np.nan, np.nan)
    assert same_bits(host(view.wigner_of(dev(poisoned))), full)
    # prefixes, one matrix without a batch axis, a permutation, a repeat
    for M in (1, 2, 3):
        assert same_bits(host(view.wigner_of(dev(rho[:M]))), full[:M])
    one = view.wigner_of(dev(rho[4]))
    assert one.shape == (X, P) and same_bits(host(one), full[4])
    perm = np.random.default_rng(X).permutation(21)
    assert same_bits(host(view.wigner_of(dev(rho[perm]))), full[perm])
    assert same_bits(host(view.wigner_of(dev(rho))), full)
    # a non-contiguous input is made contiguous
    wide = dev(np.concatenate([rho, rho], axis=2))
    assert same_bits(host(view.wigner_of(wide[:, :, :X])), full)
    # stale values behind the batch are untouched
    lib, vp = _pkg()["_lib"].lib(), ctypes.c_void_p
    out = torch.full((4 * X * P + 64,), -7.25, dtype=torch.float64, device="cuda")
    d = dev(rho[:3])
    assert lib.qc_wigner_eval_rho(view._h, vp(d.data_ptr()), 3, vp(out.data_ptr())) == 0
    o = host(out)
    assert same_bits(o[:3 * X * P].reshape(3, X, P), full[:3]) and np.all(o[3 * X * P:] == -7.25)
    view.close()


# ---------------------------------------------------------------- 3. against the shipped paths
def wavefunctions(B, X, seed):
    rng = np.random.default_rng(seed)
    phi = rng.standard_normal((B, X)) + 1j * rng.standard_normal((B, X))
    lo, hi = X // 4, X - X // 3
    phi[1::2, :lo] = 0
    phi[1::2, hi:] = 0
    h = spacing(grid(X))
    return phi / np.sqrt(h * (np.abs(phi) ** 2).sum(axis=1, keepdims=True))


@pytest.mark.parametrize("X,P", [(17, 5), (65, 17), (250, 16)])
def test_pure_states_against_wigner(X, P):
    x = grid(X)
    h = spacing(x)
    p = momenta(h)[:P]
    phi = wavefunctions(5, X, 50 + X)
    rho = PR.pure(phi, h)
    view = _pkg()["WignerView"](x, p)
    a, b = host(view.wigner_of(dev(rho))), host(view.wigner(dev(phi)))
    view.close()
    tol = R.wigner_bound(phi, h, p) + PR.wigner_of_bound(rho, h, p)
    err = np.abs(a - b)
    print(f"x_n={X} P={P}: max |wigner_of(h phi phi^†) - wigner(phi)| / tolerance {ratio(err, tol):.3f}")
    assert np.all(err <= tol)


@pytest.fixture(scope="module")
def big():
    """B = 1100 wavefunctions on 65 points and 17 momenta with their longdouble W and bound, once."""
    x = grid(65)
    h = spacing(x)
    p = momenta(h)[:17]
    phi = wavefunctions(1100, 65, 5)
    P = _pkg()
    view, ens = P["WignerView"](x, p), P["EnsembleView"](65, h)
    yield view, ens, h, p, phi, dev(phi), R.wigner_longdouble(phi, h, p), R.wigner_bound(phi, h, p)
    view.close()
    ens.close()


def cross_tolerance(mag, W, bound, sel, h, p):
    """§9i's bound on the mean of the selected states' W plus the rho route's: the bound on
    Rbar = h sum_b |phi_b| |phi_b|^T / count with the factor (2 K_i + 8) + (count + 4) (the ensemble sum's roundings on
    top of the contraction's)."""
    n = int(sel.sum())
    mean_tol = bound[sel].sum(axis=0) / n + (n + 2) * EPS * np.abs(W[sel]).astype(np.float64).sum(axis=0) / n
    m = mag[sel]
    rbar = h * np.einsum("bi,bj->ij", m, m) / n
    return mean_tol + PR.wigner_of_bound(rbar.astype(np.complex128), h, p, extra=n + 4)[0]


@pytest.mark.parametrize("name", ["all", "random"])
def test_the_ensemble_rho_against_mean_wigner(big, name):
    view, ens, h, p, phi, d, W, bound = big
    sel = np.ones(1100, dtype=bool) if name == "all" else np.random.default_rng(6).random(1100) < 0.4
    dmask = None if name == "all" else dev(sel)
    rho = ens.density_matrix(d, dmask)[0]
    a, b = host(view.wigner_of(rho)), host(view.mean_wigner(d, dmask)[0])
    tol = cross_tolerance(np.abs(phi), W, bound, sel, h, p)
    err = np.abs(a - b)
    print(f"mask {name}: count {int(sel.sum())}, max err / tolerance {ratio(err, tol):.3f}")
    assert a.shape == (65, 17) and np.all(err <= tol)
    # and each side against the longdouble mean
    want = W[sel].sum(axis=0) / int(sel.sum())
    assert np.all(np.abs(a - want).astype(np.float64) <= tol)


def test_the_ensemble_rho_with_no_env_set_is_zero(big):
    view, ens, h, p, phi, d, W, bound = big
    none = dev(np.zeros(1100, dtype=bool))
    a, b = view.wigner_of(ens.density_matrix(d, none)[0]), view.mean_wigner(d, none)[0]
    assert not np.any(host(a)) and not np.any(host(b))


# ---------------------------------------------------------------- 4. the Fock route and the congruence
_FOCK = {}


@pytest.fixture(scope="module", autouse=True)
def _close_fock_views():
    yield
    for view, _ in _FOCK.values():
        view.close()
    _FOCK.clear()


def fock_view(n_levels):
    """(WignerView on the drivers' grid, the device's own table in longdouble)."""
    if n_levels not in _FOCK:
        view = _pkg()["WignerView"](DRIVER_GRID, DEFAULT_P, n_levels=n_levels)
        _FOCK[n_levels] = (view, host(view.spatial.table()).astype(LD))
    return _FOCK[n_levels]


def fock_rho(M, n, seed):
    """Random Fock-basis density matrices of rank 3 (positive, unit trace)."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((M, 3, n)) + 1j * rng.standard_normal((M, 3, n))
    rho = np.einsum("mri,mrj->mij", c, c.conj())
    rho = (rho + rho.conj().transpose(0, 2, 1)) / 2
    return np.ascontiguousarray(rho / np.trace(rho, axis1=1, axis2=2).real[:, None, None])


def assert_hermitian_bits(y):
    re, im = np.ascontiguousarray(y.real), np.ascontiguousarray(y.imag)
    assert same_bits(re, np.ascontiguousarray(np.swapaxes(re, -1, -2)))
    off = ~np.eye(y.shape[-1], dtype=bool)
    flipped = np.ascontiguousarray(np.swapaxes(im, -1, -2)).view(np.uint64) ^ np.uint64(1 << 63)
    assert np.array_equal(im.view(np.uint64)[..., off], flipped[..., off])
    assert not np.ascontiguousarray(np.diagonal(im, axis1=-2, axis2=-1)).view(np.uint64).any()


def check_congruence(sv, E, h, rho, label):
    got = host(sv.density_matrix_of(dev(rho)))
    sr, si = PR.congruence_longdouble(E, rho, h)
    bound = PR.congruence_bound(E, rho, h)
    err = np.maximum(np.abs(got.real - sr), np.abs(got.imag - si)).astype(np.float64)
    print(f"{label}: max err {err.max():.3e}, max err/bound {ratio(err, bound):.3f}")
    assert got.shape == (rho.shape[0], E.shape[0], E.shape[0]) and np.all(err <= bound)
    assert_hermitian_bits(got)
    return got


@pytest.mark.parametrize("M", [1, 21])
@pytest.mark.parametrize("n_levels,n", [(71, 1), (71, 5), (71, 16), (71, 17), (71, 61), (71, 71), (181, 181)])
def test_density_matrix_of_against_longdouble(n_levels, n, M):
    view, E = fock_view(n_levels)
    rho = fock_rho(M, n, 1000 * n_levels + n)
    got = check_congruence(view.spatial, E, H250, rho, f"n_levels={n_levels} n={n} M={M}")
    one = view.spatial.density_matrix_of(dev(rho[0]))
    assert one.shape == (250, 250) and same_bits(host(one), got[0])


def test_density_matrix_of_on_a_second_grid_and_both_block_shapes():
    """33 points; and M = 32 on 250 points, where the launch reaches 2048 blocks of 32 x 32 and takes the wide kernels:
    the same bits as the matrices one by one (the narrow kernels)."""
    P = _pkg()
    x = np.linspace(-4, 4, 33)
    sv = P["SpatialView"](17, x)
    E = host(sv.table()).astype(LD)
    check_congruence(sv, E, 0.25, fock_rho(3, 17, 33), "33 points")
    check_congruence(sv, E, 0.25, fock_rho(2, 9, 34), "33 points, n = 9")
    sv.close()
    view, E = fock_view(71)
    rho = fock_rho(32, 37, 99)
    wide = check_congruence(view.spatial, E, H250, rho, "M = 32 (wide)")
    for m in (0, 13, 31):
        assert same_bits(host(view.spatial.density_matrix_of(dev(rho[m]))), wide[m])
    perm = np.random.default_rng(1).permutation(32)
    assert same_bits(host(view.spatial.density_matrix_of(dev(rho[perm]))), wide[perm])
    assert same_bits(host(view.spatial.density_matrix_of(dev(rho[:21]))), wide[:21])


def sigma_error_to_w(dsigma):
    """[M][X]: what an elementwise error dsigma [M][X][X] of Re and of Im sigma can move the lag sum by, times pi:
    d_ii + 2 sum_k 2 d[i + k][i - k]."""
    M, X, _ = dsigma.shape
    i = np.arange(X)
    out = dsigma[:, i, i].copy()
    for k in range(1, (X - 1) // 2 + 1):
        ii = np.arange(k, X - k)
        out[:, ii] += 4 * dsigma[:, ii + k, ii - k]
    return out


def test_closed_forms_through_the_fock_route():
    view, _ = fock_view(71)
    rho = np.zeros((3, 60, 60), dtype=np.complex128)
    rho[0, 0, 0] = 1
    rho[1, 0, 0] = rho[1, 1, 1] = 0.5
    alpha = 1.1 - 0.7j
    c = np.zeros(60, dtype=np.complex128)
    c[0] = np.exp(-abs(alpha) ** 2 / 2)
    for k in range(1, 60):
        c[k] = c[k - 1] * alpha / np.sqrt(k)
    rho[2] = np.outer(c, c.conj())
    got = host(view.wigner_of(dev(rho)))
    w0, w1 = R.fock_wigner(0, DRIVER_GRID, DEFAULT_P), R.fock_wigner(1, DRIVER_GRID, DEFAULT_P)
    want = [w0, (w0 + w1) / 2, R.gaussian_wigner(DRIVER_GRID, DEFAULT_P, x0=np.sqrt(2) * 1.1, p0=np.sqrt(2) * -0.7)]
    for m, name in enumerate(("|0><0|", "(|0><0| + |1><1|) / 2", "coherent")):
        err = float(np.max(np.abs(got[m] - want[m])))
        print(f"{name}: max |W - closed form| = {err:.2e}")
        assert err <= 1e-13


@pytest.mark.parametrize("n_levels,n", [(71, 5), (71, 61), (181, 181)])
def test_pure_fock_states_against_wigner(n_levels, n):
    view, E = fock_view(n_levels)
    rng = np.random.default_rng(n)
    c = rng.standard_normal((4, n)) + 1j * rng.standard_normal((4, n))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    rho = c[:, :, None] * c[:, None, :].conj()
    a, b = host(view.wigner_of(dev(rho))), host(view.wigner(dev(c)))
    # wigner(psi): its own tolerance (tests/test_gpu_wigner.py); wigner_of: the bound on sigma plus sigma's own error
    re, im = SR.repr_longdouble(E, c)
    mag = np.hypot(re, im).astype(np.float64)
    tol_psi = R.wigner_bound(mag, H250, DEFAULT_P) \
        + ((H250 / np.pi) * R.cross_terms(mag, SR.repr_bound(E, c)))[:, :, None]
    sigma = H250 * mag[:, :, None] * mag[:, None, :]
    dsigma = PR.congruence_bound(E, rho, H250) + 4 * EPS * sigma      # (rho itself is a rounded outer product)
    tol_rho = PR.wigner_of_bound(sigma.astype(np.complex128), H250, DEFAULT_P) \
        + (sigma_error_to_w(dsigma) / np.pi)[:, :, None]
    err = np.abs(a - b)
    print(f"n_levels={n_levels} n={n}: max err / tolerance {ratio(err, tol_psi + tol_rho):.3f}")
    assert np.all(err <= tol_psi + tol_rho)


# ---------------------------------------------------------------- 5. physics
def test_vacuum_under_measurement_stays_non_negative_and_the_negativity_of_one_phonon():
    P = _pkg()
    cfg = P["cfg"]
    ph = cfg.DEFAULTS[cfg.HO].with_(n_max=31)
    me = P["MasterEquation"](ph, forces=[0.0])
    view = P["WignerView"].for_physics(ph)
    E = host(view.spatial.table()).astype(LD)
    rho = torch.zeros(32, 32, dtype=torch.complex128, device="cuda")
    rho[0, 0] = 1.0
    me.evolve(rho, 80)
    W = host(view.wigner_of(rho))
    r = host(rho)
    sr, si = PR.congruence_longdouble(E, r, view.h)
    sigma = (sr + 1j * si).astype(np.complex128)[0]
    bound = PR.wigner_of_bound(sigma, view.h, DEFAULT_P)[0] \
        + (sigma_error_to_w(PR.congruence_bound(E, r[None], view.h)) / np.pi)[0][:, None]
    # The kernels' part, strict: W lies within the bound of the exact W of the very rho that was evolved.
    exact = PR.wigner_of_longdouble((sr[0], si[0]), view.h, DEFAULT_P)[0]
    err = np.abs(W - exact).astype(np.float64)
    print(f"against the exact W of the evolved rho: max err / bound {ratio(err, bound):.3f}")
    assert np.all(err <= bound)
    # The input's part: the evolved rho is positive only up to the channel's rounding. Its negative part rho_- gives
    # sigma_- = h Phi rho_- Phi^T >= 0 and lowers W[i][j] by at most (1 / pi) sum_{|k| <= K_i} |sigma_-[i+k][i-k]| <=
    # (1 / pi) sum_{|k| <= K_i} sqrt(d_{i+k} d_{i-k}), d = diag sigma_- (Cauchy-Schwarz on a positive matrix): per
    # position, nothing uniform. rho_- is taken from the spectrum of the 32 x 32 matrix on the host, whose eigenvalues
    # eigh resolves to 32 * 2^-53 ||rho||: that much of the identity is added to it.
    lam, V = np.linalg.eigh((r + r.conj().T) / 2)
    minus = -(V * np.minimum(lam, 0.)) @ V.conj().T + 32 * EPS * np.abs(lam).max() * np.eye(32)
    Ed = E.astype(np.float64)
    d = view.h * np.einsum("im,mn,in->i", Ed, minus, Ed).real
    K = R.lags(250)
    own = np.array([sum(np.sqrt(d[i + k] * d[i - k]) for k in range(-K[i], K[i] + 1)) for i in range(250)]) / np.pi
    allowed = bound + own[:, None]
    at = np.unravel_index(W.argmin(), W.shape)
    print(f"lambda_min = {lam.min():.3e}; min W = {W.min():.3e}, the bound there {bound[at]:.3e}, rho_-'s share there "
          f"{own[at[0]]:.3e}; max -W / bound = {float(np.max(-W / bound)):.3f}, max -W / (bound + share) = "
          f"{float(np.max(-W / allowed)):.3f}")
    assert np.all(W >= -allowed)
    dp = 24. / 192
    total = float(W.sum() * view.h * dp)
    trace = float(np.trace(sigma).real)
    print(f"sum W h dp = {total:.15f}, Tr sigma = {trace:.15f}")
    assert abs(total - trace) <= 1e-12
    assert float(view.negative_volume(dev(W))) <= float(allowed.sum() * view.h * dp)
    # |1><1|: the negative volume on the same grid
    one = torch.zeros(2, 2, dtype=torch.complex128, device="cuda")
    one[1, 1] = 1.0
    W1 = view.wigner_of(one)
    got = float(view.negative_volume(W1))
    e1 = np.zeros((2, 2), dtype=np.complex128)
    e1[1, 1] = 1
    want = PR.negative_volume_longdouble(
        PR.wigner_of_longdouble(PR.congruence_longdouble(E, e1, view.h), view.h, DEFAULT_P)[0], view.h, dp)
    print(f"negative volume of |1><1|: {got:.15f} (longdouble {float(want):.15f})")
    assert abs(got - float(want)) <= 1e-12 and got > 0.1
    stacked = view.negative_volume(torch.stack([W1, dev(W)]))
    assert stacked.shape == (2,) and abs(float(stacked[0]) - got) <= 1e-15
    me.close()
    view.close()


# ---------------------------------------------------------------- 6. the loop
def digest(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def open_loop_on(loop, tmp_path):
    P = _pkg()
    tr = loop.trainer(tmp_path / "models")
    env = loop.env
    ph = loop.c["ph"]
    env.reset()
    for _ in range(4):
        env.step(loop.actor.act(env.obs, eps=0.05))
    before = digest(env.psi)
    me = env.master_equation()
    view = P["WignerView"].for_physics(ph)
    T = 3
    plain = tr.open_loop(me, T)
    curve = tr.open_loop(me, T, wigner=view)
    assert set(curve) == set(plain) | {"wigner", "negativity"}
    assert curve["wigner"].shape == (T + 1, view.x_n, view.p_n) and curve["negativity"].shape == (T + 1,)
    assert curve["wigner"].dtype == torch.float64 and curve["wigner"].is_cuda
    for k in plain:
        assert same_bits(host(curve[k]), host(plain[k])), k
    assert digest(env.psi) == before
    for k in range(T + 1):
        assert float(curve["negativity"][k]) == float(view.negative_volume(curve["wigner"][k]))
    # entry 0 is the ensemble's Wigner function: mean_wigner of the env's states, within the cross-check's tolerance
    psi = host(env.psi)
    B = psi.shape[0]
    sel = np.ones(B, dtype=bool)
    p = host(view.p)
    if ph.fock:
        E = host(view.spatial.table()).astype(LD)
        re, im = SR.repr_longdouble(E, psi)
        mag = np.hypot(re, im).astype(np.float64)
        W = R.wigner_longdouble((re, im), view.h, p)
        bound = R.wigner_bound(mag, view.h, p) + ((view.h / np.pi) * R.cross_terms(mag, SR.repr_bound(E, psi)))[:, :, None]
        tol = cross_tolerance(mag, W, bound, sel, view.h, p)
        # sigma's own error: the congruence's on the ensemble's |rho|, whose sum adds (B + 4) roundings
        absrho = np.einsum("bi,bj->ij", np.abs(psi), np.abs(psi))[None] / B
        n = psi.shape[1]
        dsigma = PR.congruence_bound(E, absrho, view.h) * ((2 * n + 8 + B + 4) / (2 * n + 8))
        tol = tol + (sigma_error_to_w(dsigma) / np.pi)[0][:, None]
    else:
        W, bound = R.wigner_longdouble(psi, view.h, p), R.wigner_bound(psi, view.h, p)
        tol = cross_tolerance(np.abs(psi), W, bound, sel, view.h, p)
    m = host(view.mean_wigner(env.psi)[0])
    err = np.abs(host(curve["wigner"][0]) - m)
    print(f"{ph.family}: entry 0 against mean_wigner: max err {err.max():.3e}, max err/tolerance {ratio(err, tol):.3f}")
    assert np.all(err <= tol)
    me.close()
    view.close()


def test_open_loop_wigner_on_the_harmonic_loop(tmp_path):
    from tests.test_gpu_trainer import Loop
    loop = Loop("ho")
    open_loop_on(loop, tmp_path)
    loop.close()


def test_open_loop_wigner_on_the_quartic_loop(tmp_path):
    from tests.test_gpu_trainer_monitor import Loop
    loop = Loop("qo")
    open_loop_on(loop, tmp_path)
    loop.close()


def test_command_line_adds_the_wigner_keys(tmp_path):
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import train
    out = tmp_path / "open_loop.npz"
    common = ["--system", "ho", "--control_strategy", "LQG", "--envs", "32", "--num_of_test_episodes", "4",
              "--max_steps", "5", "--save_dir", str(tmp_path / "a")]
    assert train.main(common + ["--open_loop_out", str(out), "--open_loop_steps", "3", "--open_loop_wigner"]) == 0
    z = np.load(out)
    scalars = ["t", "trace", "purity", "boundary", "x", "x2", "h", "n", "negativity"]
    assert sorted(z.files) == sorted(scalars + ["wigner", "wigner_x", "wigner_p"])
    assert all(z[k].shape == (4,) and z[k].dtype == np.float64 for k in scalars)
    assert z["wigner"].shape == (4, 250, 193) and z["wigner_x"].shape == (250,) and z["wigner_p"].shape == (193,)
    assert np.array_equal(z["wigner_x"], DRIVER_GRID) and np.array_equal(z["wigner_p"], DEFAULT_P)
    assert np.all(np.abs(z["wigner"].sum(axis=(1, 2)) * H250 * 0.125 - z["trace"]) <= 1e-9)
    with pytest.raises(SystemExit):
        train.main(common + ["--open_loop_wigner"])


# ---------------------------------------------------------------- 7. refusals
def test_python_refusals():
    P = _pkg()
    view = P["WignerView"](grid(17), np.linspace(-2, 2, 5))
    good = torch.zeros(3, 17, 17, dtype=torch.complex128, device="cuda")
    for bad, text in ((good.cpu(), "must live on"), (good.to(torch.complex64), "must be complex128"),
                      (good.real.contiguous(), "must be complex128"), (host(good), "torch tensor"),
                      (good[:, :16, :16], "takes density matrices of 17 points, not 16"),
                      (good[:, :, :16], r"rho must be \[M, x_n, x_n\]"), (good[0, 0], r"rho must be \[M, x_n, x_n\]"),
                      (good[:0], r"rho must be \[M, x_n, x_n\]"), (good[None], r"rho must be \[M, x_n, x_n\]")):
        with pytest.raises(ValueError, match=text):
            view.wigner_of(bad)
    with pytest.raises(ValueError, match=r"W must be \[..., 17, 5\]"):
        view.negative_volume(torch.zeros(5, 17, device="cuda"))
    view.close()
    uneven = P["WignerView"](grid(17), np.array([-1.0, 0.0, 0.5]))
    with pytest.raises(ValueError, match="negative_volume needs uniform momenta"):
        uneven.negative_volume(torch.zeros(17, 3, dtype=torch.float64, device="cuda"))
    uneven.close()
    big = P["WignerView"](grid(4096), np.array([0.0]))
    with pytest.raises(ValueError, match=r"M x_n\^2 must be <= 2\^27"):
        big.wigner_of(torch.zeros(1, dtype=torch.complex128, device="cuda").expand(9, 4096, 4096))
    big.close()
    fock = P["WignerView"](DRIVER_GRID, DEFAULT_P[:4], n_levels=8)
    g8 = torch.zeros(2, 8, 8, dtype=torch.complex128, device="cuda")
    for bad, text in ((torch.zeros(2, 9, 9, dtype=torch.complex128, device="cuda"), r"n_state must be in \[1, 8\], not 9"),
                      (g8[:, :, :7], r"rho must be \[M, n, n\]"), (g8.cpu(), "must live on"),
                      (g8.to(torch.complex64), "must be complex128"), (host(g8), "torch tensor"),
                      (g8[0, 0], r"rho must be \[M, n, n\]")):
        for call in (fock.wigner_of, fock.spatial.density_matrix_of):
            with pytest.raises(ValueError, match=text):
                call(bad)
    assert fock.wigner_of(g8[:, :5, :5]).shape == (2, 250, 4)
    fock.close()
    gridview = P["SpatialView"](0, grid(17))
    with pytest.raises(ValueError, match="a grid view's density matrix lives on the grid already"):
        gridview.density_matrix_of(good)
    gridview.close()
    crooked = P["SpatialView"](4, np.array([0.0, 0.1, 0.3]))
    with pytest.raises(ValueError, match="uniform ascending grid"):
        crooked.density_matrix_of(torch.zeros(4, 4, dtype=torch.complex128, device="cuda"))
    crooked.close()


def test_c_abi_refusals_carry_a_text():
    P = _pkg()
    lib, vp = P["_lib"].lib(), ctypes.c_void_p
    view = P["WignerView"](grid(4096), np.array([0.0]))
    buf = torch.zeros(64, dtype=torch.complex128, device="cuda")
    ptr = vp(buf.data_ptr())
    for call, text in ((lambda: lib.qc_wigner_eval_rho(view._h, None, 1, ptr), b"rho and out are required"),
                       (lambda: lib.qc_wigner_eval_rho(view._h, ptr, 1, None), b"rho and out are required"),
                       (lambda: lib.qc_wigner_eval_rho(view._h, ptr, 0, ptr), b"M must be >= 1"),
                       (lambda: lib.qc_wigner_eval_rho(view._h, ptr, 9, ptr), b"M x_n^2 must be <= 2^27")):
        assert call() == -1 and b"qc_wigner_eval_rho: " + text in lib.qc_wigner_last_error(view._h)
    assert lib.qc_wigner_eval_rho(None, ptr, 1, ptr) == -1
    view.close()
    sv = P["SpatialView"](8, grid(4096))
    for call, text in ((lambda: lib.qc_spatial_congruence(sv._h, None, 4, 1, 1.0, ptr), b"rho and sigma are required"),
                       (lambda: lib.qc_spatial_congruence(sv._h, ptr, 4, 1, 1.0, None), b"rho and sigma are required"),
                       (lambda: lib.qc_spatial_congruence(sv._h, ptr, 4, 0, 1.0, ptr), b"M must be >= 1"),
                       (lambda: lib.qc_spatial_congruence(sv._h, ptr, 9, 1, 1.0, ptr),
                        b"n_state must be in [1, n_levels = 8], not 9"),
                       (lambda: lib.qc_spatial_congruence(sv._h, ptr, 0, 1, 1.0, ptr),
                        b"n_state must be in [1, n_levels = 8], not 0"),
                       (lambda: lib.qc_spatial_congruence(sv._h, ptr, 4, 1, float("nan"), ptr), b"scale must be finite"),
                       (lambda: lib.qc_spatial_congruence(sv._h, ptr, 4, 9, 1.0, ptr), b"M x_n^2 must be <= 2^27")):
        assert call() == -1 and b"qc_spatial_congruence: " + text in lib.qc_spatial_last_error(sv._h)
    sv.close()
    gv = P["SpatialView"](0, grid(17))
    assert lib.qc_spatial_congruence(gv._h, ptr, 4, 1, 1.0, ptr) == -1
    assert b"a grid view's density matrix lives on the grid already" in lib.qc_spatial_last_error(gv._h)
    gv.close()
