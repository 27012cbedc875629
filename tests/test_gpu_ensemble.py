"""The ensemble density matrix on the device (csrc/qcart_ensemble.hip, ensemble.EnsembleView): rho against the longdouble
restatement (tests/ensemble_ref.py) within the a-priori per-element bound
    sqrt(2) (2 B + S + 4) 2^-53 scale T_mn / count,   T_mn = sum_live |psi_b[m]| |psi_b[n]|
(2 B products per real part with |a_m a_n| + |b_m b_n| <= |psi_m| |psi_n|; S split additions; the scaling and the
division; sqrt(2) for the modulus; a float64 numpy evaluation stays below 0.2 of it, tests/test_ensemble_cpu.py; the
device's largest error / bound measured is 0.217, at (B, N) = (3, 2048), and 0.003 at B = 1100), the
output's structure by bit pattern, the conventions against the views and observables the project already has, the
helpers, the refusals, and the public additions (BatchedEnv.density_matrix, Trainer.evaluate(ensemble=...),
train --rho_out)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ensemble_ref as R
from tests.checkpoint_loop import flatten, same_bits

pytestmark = pytest.mark.gpu


def _pkg():
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import _lib
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import config as cfg
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.core import Stepper
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.ensemble import EnsembleView
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.env import BatchedEnv
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.spatial import SpatialView
    return locals()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scale_of(N):
    """Fock normalisation for even N, a grid spacing for odd N."""
    return 1.0 if N % 2 == 0 else 0.1


def states(B, N, seed):
    """Seeded complex Gaussians with scale * ||psi||^2 = 1; every odd env has zero tails (only a middle window set)."""
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N))
    lo, hi = N // 4, N - N // 3
    if hi - lo >= 1:
        psi[1::2, :lo] = 0
        psi[1::2, hi:] = 0
    return psi / np.sqrt(scale_of(N) * (np.abs(psi) ** 2).sum(axis=1, keepdims=True))


_STATES, _VIEWS = {}, {}


def batch(N):
    """Per N, once: 1100 states; smaller batches are prefixes."""
    if N not in _STATES:
        _STATES[N] = states(1100, N, 300 + N)
    return _STATES[N]


def view_of(N):
    if N not in _VIEWS:
        _VIEWS[N] = _pkg()["EnsembleView"](N, scale_of(N))
    return _VIEWS[N]


@pytest.fixture(scope="module", autouse=True)
def _close_views():
    yield
    for v in _VIEWS.values():
        v.close()
    _VIEWS.clear()
    _STATES.clear()


def held_to_the_bound(psi, mask, N, what):
    """One call against the restatement; returns the largest error / bound."""
    B = psi.shape[0]
    view = view_of(N)
    S = _pkg()["_lib"].lib().qc_ensemble_splits(B, N)
    assert S == R.splits(B, N)
    rho, count = view.density_matrix(dev(psi), None if mask is None else dev(mask))
    want, n = R.density_longdouble(psi, mask, view.scale)
    assert rho.shape == (N, N) and rho.dtype == torch.complex128 and count.dtype == torch.int64 and int(count) == n
    got = rho.cpu().numpy()
    b = R.bound(psi, mask, view.scale, S)
    err = np.abs(got - want).astype(np.float64)
    ratio = float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1), 0)))
    print(f"{what}: S = {S}, count = {n}, max err {err.max():.3e}, max err / bound {ratio:.3f}")
    assert np.all(err <= b)                          # (b = 0: both operands' columns are zero for every live env)
    # the states are normalised (scale ||psi||^2 = 1 within a few roundings): Tr rho = 1 within the diagonal's bounds
    assert abs(float(np.trace(got).real) - 1) <= float(np.trace(b)) + 8 * 2.0 ** -53
    assert float(np.trace(got).imag) == 0.0
    return ratio


# ---------------------------------------------------------------- 1. rho against the restatement
@pytest.mark.parametrize("N", [1, 2, 15, 16, 17, 33, 71, 181, 250])
@pytest.mark.parametrize("B", [1, 2, 3, 5, 33, 1100])
def test_rho_equals_the_longdouble_restatement_within_the_bound(B, N):
    """One tile, the tile edge -1 / +1, a column block's edge + 1, more than one row block and an odd chunk tail, every
    split count from 1 upward (B = 1, 2: one; 3: two; 5: three; 33: 17; 1100: 256, or 132 / 67 where the partials cap
    it), and with B = 1100 more chunks than splits."""
    held_to_the_bound(batch(N)[:B], None, N, f"B={B} N={N}")


@pytest.mark.parametrize("B,N", [(3, 513), (3, 2048)])
def test_rho_within_the_bound_at_the_wide_sizes(B, N):
    held_to_the_bound(states(B, N, 7 + N), None, N, f"B={B} N={N}")
    _VIEWS.pop(N).close()                            # (N = 2048 holds 64 MiB of partials)


@pytest.mark.parametrize("B,N", [(5, 17), (33, 181), (1100, 71)])
def test_rho_within_the_bound_under_a_mask(B, N):
    mask = np.random.default_rng(B + N).random(B) < 0.5
    assert 0 < mask.sum() < B
    held_to_the_bound(batch(N)[:B], mask, N, f"B={B} N={N} masked")


# ---------------------------------------------------------------- 2. structure by bit pattern
def words(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("B,N", [(37, 100), (1100, 71)])
def test_structure_by_bit_pattern(B, N):
    psi = batch(N if N == 71 else 250)[:B, :N].copy()
    view = view_of(N)
    mask = np.random.default_rng(5).random(B) < 0.6
    d, dmask = dev(psi), dev(mask)
    rho, count = view.density_matrix(d, dmask)
    got = rho.cpu().numpy()
    n = int(mask.sum())
    assert int(count) == n
    # exactly Hermitian: rho[n][m] is the conjugate of rho[m][n] (the sign bit of the imaginary part flipped)
    off = ~np.eye(N, dtype=bool)
    assert same_bits(got.T.conj()[off], got[off])
    # the diagonal's imaginary part is +0.0, its real part positive
    assert not np.any(words(got.imag.diagonal().copy())) and np.all(got.real.diagonal() >= 0)
    # a repeat, and the mask as uint8, give the same bits
    again, _ = view.density_matrix(d, dmask.to(torch.uint8))
    assert same_bits(again.cpu().numpy(), got)
    # what a masked env holds is not read: zeros or NaNs there, and NaNs behind the batch where an odd B's last chunk
    # is padded, give the same bits
    zeroed = psi.copy()
    zeroed[~mask] = 0
    rz, nz = view.density_matrix(dev(zeroed), dmask)
    assert int(nz) == n and same_bits(rz.cpu().numpy(), got)
    poisoned = np.full((B + 2, N), np.nan + 1j * np.nan)
    poisoned[:B][mask] = psi[mask]
    poisoned[:B][~mask] = np.array([np.nan + 1j * np.inf])
    rp, _ = view.density_matrix(dev(poisoned)[:B], dmask)
    assert same_bits(rp.cpu().numpy(), got)
    # a masked env contributes what a zero state contributes: without the mask the zeroed batch runs the same
    # accumulation and has the same sum t, divided by B instead of the count. Each is fl(fl(scale t) / count), so the
    # sums recovered by one more multiplication agree within 2 roundings each.
    ra, na = view.density_matrix(dev(zeroed))
    assert int(na) == B
    s1, s2 = got * n, ra.cpu().numpy() * B
    assert np.all(np.abs(s1 - s2) <= 4 * 2.0 ** -53 * np.abs(s1))
    # only the last env live: its own outer product, the bits of that state alone
    last = np.zeros(B, dtype=bool)
    last[B - 1] = True
    rl, nl = view.density_matrix(d, dev(last))
    alone, one = view.density_matrix(d[B - 1])       # one [N] state is B = 1
    assert int(nl) == 1 and int(one) == 1
    if B % 2 == 1:                                   # (the same operand slot of the matrix instruction)
        assert same_bits(rl.cpu().numpy(), alone.cpu().numpy())
    want = view.scale * np.outer(psi[B - 1], psi[B - 1].conj())
    assert np.abs(rl.cpu().numpy() - want).max() <= 8 * 2.0 ** -53 * np.abs(want).max()
    assert np.abs(alone.cpu().numpy() - want).max() <= 8 * 2.0 ** -53 * np.abs(want).max()
    # none live: zeros and count 0
    r0, n0 = view.density_matrix(dev(poisoned)[:B], dev(np.zeros(B, dtype=bool)))
    assert int(n0) == 0 and r0.shape == (N, N) and not np.any(r0.cpu().numpy())


# ---------------------------------------------------------------- 3. conventions against what the project has
def test_fock_conventions_against_the_spatial_view_and_the_observables():
    P = _pkg()
    cfg = P["cfg"]
    ph = cfg.DEFAULTS[cfg.IHO]
    st = P["Stepper"](ph, 17, 0, seed=3)
    view = P["EnsembleView"].for_physics(ph)
    sv = P["SpatialView"].for_physics(ph)
    assert view.n == ph.n_max + 1 == 181 and view.scale == 1.0
    psi = st.new_state()
    st.reset(psi, P["_lib"].QC_RESET_RANDOM, arg0=8)
    mask = dev(np.arange(17) % 3 != 1)
    sel = mask.cpu().numpy()
    rho, count = view.density_matrix(psi, mask)
    assert int(count) == int(sel.sum()) == 11
    r = rho.cpu().numpy()
    assert abs(np.trace(r).real - 1) <= 1e-12
    E = sv.table().cpu().numpy()                     # [X, 181]
    dens, _ = sv.mean_probability(psi, mask)
    got = np.einsum("jm,mn,jn->j", E, r, E)
    d_err = np.abs(got.real - dens.cpu().numpy()).max()
    # <x> and <p>: X in the Fock basis by quadrature of the table on the drivers' grid (the 8 occupied levels decay
    # far inside it), P from [x, p] = i: P_{n+1, n} = i X_{n+1, n} / (2 X_01^2) = -P_{n, n+1}
    x = sv.x.cpu().numpy()
    h = float(x[1] - x[0])
    X = h * (E[:, :12].T * x) @ E[:, :12]
    lam = X[0, 1]
    Pm = 1j * (np.tril(X, -1) - np.triu(X, 1)) / (2 * lam * lam)
    xe = st.x_expectation(psi).cpu().numpy()
    mom = st.moments(psi).cpu().numpy()
    assert np.abs(mom[:, 0] - xe).max() <= 1e-13 and np.abs(mom[sel, 1]).max() > 0.05
    Xd = torch.zeros(181, 181, dtype=torch.float64, device="cuda")
    Xd[:12, :12] = dev(X)
    Pd = torch.zeros(181, 181, dtype=torch.complex128, device="cuda")
    Pd[:12, :12] = dev(Pm)
    x_got, p_got = view.expectation(rho, Xd), view.expectation(rho, Pd)
    x_err = abs(complex(x_got) - xe[sel].mean())
    p_err = abs(complex(p_got) - mom[sel, 1].mean())
    print(f"Fock conventions: density {d_err:.3e}, <x> {x_err:.3e}, <p> {p_err:.3e}")
    assert d_err <= 1e-12 and x_err <= 1e-12 and p_err <= 1e-12
    view.close()
    sv.close()
    st.close()


def test_grid_conventions_against_the_spatial_view_and_the_observables():
    P = _pkg()
    cfg = P["cfg"]
    ph = cfg.DEFAULTS[cfg.QO]
    env = P["BatchedEnv"](ph, 24, 0, seed=9, input="xp", reset="warmup")
    env.reset()
    rng = np.random.default_rng(2)
    info = None
    for _ in range(3):
        info = env.step(dev(rng.integers(0, ph.n_actions, 24).astype(np.int32)))[3]
    view = P["EnsembleView"].for_physics(ph)
    sv = P["SpatialView"].for_physics(ph)
    assert view.n == ph.dim and view.scale == ph.grid_size
    mask = dev(np.arange(24) % 4 != 2)
    sel = mask.cpu().numpy()
    rho, count = env.density_matrix(view, mask)
    r = rho.cpu().numpy()
    assert int(count) == 18
    t_err = abs(np.trace(r).real - 1)                # Tr rho = 1 after env steps (the states stay normalised)
    dens, _ = sv.mean_probability(env.psi, mask)
    d_err = np.abs(np.diag(r).real / ph.grid_size - dens.cpu().numpy()).max()
    x = sv.x
    xe = env.st.x_expectation(env.psi).cpu().numpy()
    x_err = abs(complex(view.expectation(rho, torch.diag(x))) - xe[sel].mean())
    print(f"grid conventions: trace {t_err:.3e}, density {d_err:.3e}, <x> {x_err:.3e}")
    assert t_err <= 1e-12 and d_err <= 1e-12 and x_err <= 1e-12
    # all envs, through info['valid'] of a step
    rho_v, count_v = env.density_matrix(view, info["valid"])
    assert int(count_v) == int(info["valid"].sum())
    view.close()
    sv.close()
    env.st.close()


# ---------------------------------------------------------------- 4. the helpers
def test_helpers_equal_numpy_on_the_copied_rho():
    N, B = 71, 33
    psi = batch(N)[:B]
    view = view_of(N)
    rho, _ = view.density_matrix(dev(psi))
    r = rho.cpu().numpy()
    pur = view.purity(rho)
    assert pur.dim() == 0 and pur.dtype == torch.float64
    assert abs(float(pur) - float((np.abs(r) ** 2).sum())) <= 1e-15
    assert abs(float(pur) - np.trace(r @ r).real) <= 1e-15 and 1 / N <= float(pur) <= 1 + 1e-12
    pop = view.populations(rho)
    assert pop.shape == (N,) and pop.dtype == torch.float64 and same_bits(pop.cpu().numpy(), np.diag(r).real.copy())
    targets = batch(N)[40:43]
    f = view.fidelity(rho, dev(targets))
    want = np.array([(t.conj() @ r @ t).real * view.scale for t in targets])
    assert f.shape == (3,) and np.abs(f.cpu().numpy() - want).max() <= 1e-15
    f1 = view.fidelity(rho, dev(targets[1]))
    assert f1.dim() == 0 and abs(float(f1) - want[1]) <= 1e-15
    pure, _ = view.density_matrix(dev(np.tile(psi[4], (6, 1))))
    assert abs(float(view.fidelity(pure, dev(psi[4]))) - 1) <= 1e-13 and abs(float(view.purity(pure)) - 1) <= 1e-13
    rng = np.random.default_rng(8)
    op = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    e = view.expectation(rho, dev(op))
    assert e.dim() == 0 and abs(complex(e) - np.trace(r @ op)) <= 1e-13
    # the basis states: rho = I / K, purity 1 / K
    K = 16
    basis = view_of(K)
    rho_b, _ = basis.density_matrix(dev(np.eye(K, dtype=np.complex128)))
    assert np.array_equal(rho_b.cpu().numpy(), np.eye(K) / K) and float(basis.purity(rho_b)) == 1 / K


# ---------------------------------------------------------------- 5. refusals
def test_refusals():
    P = _pkg()
    EV, QE = P["EnsembleView"], P["_lib"].QCartError
    with pytest.raises(QE, match=r"N must be in \[1, 2048\]"):
        EV(0)
    with pytest.raises(QE, match=r"N must be in \[1, 2048\]"):
        EV(2049)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(QE, match="scale must be finite and > 0"):
            EV(8, bad)
    view = EV(9, 0.5)
    assert view.n == 9 and view.scale == 0.5
    good = dev(states(4, 9, 1))
    with pytest.raises(ValueError, match="complex128.*complex64 states are not viewed"):
        view.density_matrix(good.to(torch.complex64))
    with pytest.raises(ValueError, match="9 components"):
        view.density_matrix(dev(states(4, 8, 1)))
    with pytest.raises(ValueError, match="must live on"):
        view.density_matrix(good.cpu())
    with pytest.raises(ValueError):
        view.density_matrix(good[:, None, :])
    with pytest.raises(ValueError, match="torch tensor"):
        view.density_matrix(good.cpu().numpy())
    with pytest.raises(ValueError, match="mask"):
        view.density_matrix(good, torch.ones(5, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="mask"):
        view.density_matrix(good, torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="mask"):
        view.density_matrix(good, torch.ones(4, dtype=torch.int32, device="cuda"))
    # the library's own refusals, below the Python checks
    lib, vp = P["_lib"].lib(), ctypes.c_void_p
    out = torch.empty(9, 9, dtype=torch.complex128, device="cuda")
    assert lib.qc_ensemble_density(view._h, vp(good.data_ptr()), 0, None, vp(out.data_ptr()), None) == -1
    assert b"qc_ensemble_density: B must be >= 1" in lib.qc_ensemble_last_error(view._h)
    assert lib.qc_ensemble_density(view._h, None, 4, None, vp(out.data_ptr()), None) == -1
    assert b"qc_ensemble_density: psi and rho are required" in lib.qc_ensemble_last_error(view._h)
    assert lib.qc_ensemble_density(view._h, vp(good.data_ptr()), 4, None, None, None) == -1
    assert b"qc_ensemble_density: psi and rho are required" in lib.qc_ensemble_last_error(view._h)
    assert lib.qc_ensemble_density(None, vp(good.data_ptr()), 4, None, vp(out.data_ptr()), None) == -1
    # a call without a count pointer uses the handle's own
    assert lib.qc_ensemble_density(view._h, vp(good.data_ptr()), 4, None, vp(out.data_ptr()), None) == 0
    assert same_bits(out.cpu().numpy(), view.density_matrix(good)[0].cpu().numpy())
    view.close()


# ---------------------------------------------------------------- 6. BatchedEnv.density_matrix
def test_env_density_matrix_is_the_view_on_psi_and_has_no_side_effect():
    P = _pkg()
    cfg = P["cfg"]
    ph = cfg.DEFAULTS[cfg.IHO]
    view = P["EnsembleView"].for_physics(ph)
    envs = [P["BatchedEnv"](ph, 33, 0, seed=17, input="xp", reset="deferred") for _ in range(2)]
    acts = [dev(np.random.default_rng(40 + i).integers(0, 21, 33).astype(np.int32)) for i in range(4)]
    mask = dev(np.random.default_rng(44).random(33) < 0.5)
    for env in envs:
        env.reset()
        for a in acts[:3]:
            env.step(a)
    env = envs[0]
    rho, count = env.density_matrix(view, mask)
    rho2, count2 = view.density_matrix(env.psi, mask)
    assert int(count) == int(count2) == int(mask.sum()) and same_bits(rho.cpu().numpy(), rho2.cpu().numpy())
    sel = mask.cpu().numpy()
    psi = env.psi.cpu().numpy()[sel]
    plain = np.einsum("bm,bn->mn", psi, psi.conj()) / sel.sum()
    assert np.abs(rho.cpu().numpy() - plain).max() <= 1e-14
    whole, n_all = env.density_matrix(view)
    assert int(n_all) == 33 and abs(np.trace(whole.cpu().numpy()).real - 1) <= 1e-12
    for e in envs:                                   # and the env goes on as the one never asked
        e.step(acts[3])
    a, b = {}, {}
    flatten("env", envs[0].state_dict(), a)
    flatten("env", envs[1].state_dict(), b)
    assert sorted(a) == sorted(b)
    for k in a:
        assert same_bits(a[k], b[k]), k
    view.close()
    for e in envs:
        e.st.close()


# ---------------------------------------------------------------- 7. Trainer.evaluate(ensemble=view)
def evaluate_with_traces(loop, tmp_path, N, monitored):
    P = _pkg()
    tr = loop.trainer(tmp_path / "models")
    assert (tr.monitor is not None) == monitored
    env = loop.env
    env.reset()
    for _ in range(6):
        env.step(loop.actor.act(env.obs, eps=0.05))
    tr.save_checkpoint(tmp_path / "start.pt")
    view = P["EnsembleView"].for_physics(loop.c["ph"])
    assert view.n == N
    with_trace = tr.evaluate(None, 10 ** 6, max_steps=11, ensemble=view, rho_every=3)
    assert len(tr.purity_trace) == len(tr.population_trace) == 11 and tr.rho_steps == [0, 3, 6, 9]
    assert len(tr.rho_trace) == 4 and tr.density_trace == [] and tr.wigner_trace == []
    pur = torch.stack(tr.purity_trace).cpu().numpy()
    pop = torch.stack(tr.population_trace).cpu().numpy()
    rhos = [t.cpu().numpy() for t in tr.rho_trace]
    print(f"purity trace: {pur.min():.4f} .. {pur.max():.4f}")
    # (a control step at which no env of the cooling loop's few is valid has count 0: zeros, purity 0)
    empty = np.zeros(11, dtype=bool) if not monitored else pop.sum(axis=1) == 0
    assert pur.shape == (11,) and np.all(pur[~empty] > 0) and np.all(pur <= 1 + 1e-12) and not np.any(pur[empty])
    assert not empty[0] and empty.sum() <= 5
    assert pop.shape == (11, N) and np.abs(pop[~empty].sum(axis=1) - 1).max() <= 1e-9 and np.all(pop >= 0)
    for step, r in zip(tr.rho_steps, rhos):
        assert r.shape == (N, N) and same_bits(np.diag(r).real.copy(), pop[step])
        assert float((np.abs(r) ** 2).sum()) == pytest.approx(pur[step], abs=1e-14)
    assert not same_bits(rhos[0], rhos[1])           # the ensemble moves
    # the first entry: the ensemble after the first control step from the start state, under that step's mask
    tr.load_checkpoint(tmp_path / "start.pt")
    info = env.step(loop.actor.act(env.obs, eps=0.0, noisy=False))[3]
    first, _ = view.density_matrix(env.psi, info["valid"])
    assert same_bits(first.cpu().numpy(), rhos[0])
    # the returned tuple is bit for bit the one without the view, and the traces start empty with each call
    tr.load_checkpoint(tmp_path / "start.pt")
    plain = tr.evaluate(None, 10 ** 6, max_steps=11)
    assert tr.purity_trace == [] and tr.population_trace == [] and tr.rho_trace == [] and tr.rho_steps == []
    assert np.array(with_trace).tobytes() == np.array(plain).tobytes()
    tr.load_checkpoint(tmp_path / "start.pt")
    tr.evaluate(None, 10 ** 6, max_steps=4, ensemble=view)
    assert len(tr.purity_trace) == 4 and tr.rho_trace == []       # the full matrix is opt-in
    with pytest.raises(ValueError, match="rho_every"):
        tr.evaluate(None, 1, max_steps=1, ensemble=view, rho_every=-1)
    view.close()
    return with_trace


def test_evaluate_with_an_ensemble_trace(tmp_path):
    from tests.test_gpu_trainer import Loop
    loop = Loop("iho")
    with_trace = evaluate_with_traces(loop, tmp_path, 64, False)
    assert with_trace[2] > 0
    loop.close()


def test_evaluate_performance_with_an_ensemble_trace(tmp_path):
    """The loop with a monitor attached (the cooling drivers' statistic)."""
    from tests.test_gpu_trainer_monitor import Loop
    loop = Loop("ho")
    evaluate_with_traces(loop, tmp_path, 64, True)
    loop.close()


# ---------------------------------------------------------------- 8. the command line
def test_command_line_writes_the_npz(tmp_path):
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import train
    out, wout = tmp_path / "rho.npz", tmp_path / "w.npz"
    rc = train.main(["--system", "iho", "--control_strategy", "LQG", "--envs", "32", "--num_of_test_episodes", "4",
                     "--max_steps", "7", "--save_dir", str(tmp_path / "run"), "--rho_out", str(out), "--rho_every", "2",
                     "--wigner_out", str(wout)])
    assert rc == 0
    z = np.load(out)
    assert sorted(z.files) == ["populations", "purity", "rho", "rho_steps"]
    steps = z["purity"].shape[0]
    assert 1 <= steps <= 7 and z["purity"].dtype == np.float64 and z["populations"].shape == (steps, 181)
    assert z["rho_steps"].tolist() == list(range(0, steps, 2)) and z["rho"].shape == (len(z["rho_steps"]), 181, 181)
    assert z["rho"].dtype == np.complex128 and np.load(wout)["wigner"].shape[0] == steps
    rc = train.main(["--system", "iho", "--control_strategy", "LQG", "--envs", "32", "--num_of_test_episodes", "4",
                     "--max_steps", "3", "--save_dir", str(tmp_path / "run"), "--rho_out", str(out)])
    assert rc == 0 and sorted(np.load(out).files) == ["populations", "purity"]
