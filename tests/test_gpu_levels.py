"""The energy-level view on the device (csrc/qcart_levels.hip, levels.LevelView): the amplitudes against the longdouble
restatement (tests/levels_ref.py) within the a-priori bound (N + 4) 2^-53 scale sum_j |V[k][j]| |part psi_b[j]| per
part (largest error / bound measured on the device: 0.280, at N = 5; 0.027 at N = 171; at most 0.003 at the wide
sizes); the populations, the batch independence and the mean's documented order by bit pattern; the conventions against
the views and observables the project already has; the refusals; and the public additions
(BatchedEnv.level_populations, Trainer.evaluate(levels=...), train --levels_out)."""
import ctypes
import hashlib
import math

import numpy as np
import pytest
import torch

from tests import levels_ref as R
from tests.checkpoint_loop import same_bits

pytestmark = pytest.mark.gpu


def _pkg():
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import _lib
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import config as cfg
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.core import Stepper
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.ensemble import EnsembleView
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.env import BatchedEnv
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.levels import LevelView
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.spatial import SpatialView
    return locals()


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def scale_of(N):
    return 1.0 if N % 2 == 0 else math.sqrt(0.1)


def states(B, N, seed):
    """Seeded complex Gaussians of unit l2 norm; every odd env has zero tails (only a middle window set)."""
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N))
    lo, hi = N // 4, N - N // 3
    if hi - lo >= 1:
        psi[1::2, :lo] = 0
        psi[1::2, hi:] = 0
    return psi / np.sqrt((np.abs(psi) ** 2).sum(axis=1, keepdims=True))


_STATES, _TABLES, _VIEWS = {}, {}, {}


def batch(N):
    """Per N, once: 1100 states; smaller batches are prefixes."""
    if N not in _STATES:
        _STATES[N] = states(1100, N, 700 + N)
        _STATES[N].setflags(write=False)
    return _STATES[N]


def table(N):
    """Per N, once: min(N, 256) unit-norm Gaussian rows; a K-level table is its first K rows."""
    if N not in _TABLES:
        _TABLES[N] = R.unit_rows(np.random.default_rng(900 + N), min(N, 256), N)
        _TABLES[N].setflags(write=False)
    return _TABLES[N]


def view_of(N, K):
    if (N, K) not in _VIEWS:
        _VIEWS[(N, K)] = _pkg()["LevelView"](table(N)[:K], scale_of(N))
    return _VIEWS[(N, K)]


@pytest.fixture(scope="module", autouse=True)
def _close_views():
    yield
    for v in _VIEWS.values():
        v.close()
    _VIEWS.clear()
    _STATES.clear()
    _TABLES.clear()


def words(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint64)


def amplitude_ratio(psi, N, K):
    """One call against the restatement: the largest error / bound of either part."""
    view = view_of(N, K)
    a = view.amplitudes(dev(psi))
    assert a.shape == (psi.shape[0], K) and a.dtype == torch.complex128
    got = a.cpu().numpy()
    wre, wim = R.amplitudes_longdouble(psi, table(N)[:K], view.scale)
    bre, bim = R.bound(psi, table(N)[:K], view.scale)
    worst = 0.0
    for g, w, b in ((got.real, wre, bre), (got.imag, wim, bim)):
        err = np.abs(g - w).astype(np.float64)
        assert np.all(err <= b), (N, K, psi.shape[0], float(err.max()))     # (b = 0: every product is zero)
        worst = max(worst, float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1), 0))))
    return worst


# ---------------------------------------------------------------- 1. amplitudes against the restatement
BS = (1, 2, 15, 16, 17, 33, 65, 1100)
KS = (1, 2, 15, 16, 17, 33, 64)


@pytest.mark.parametrize("N", [1, 3, 4, 5, 15, 16, 17, 41, 171])
def test_amplitudes_equal_the_longdouble_restatement_within_the_bound(N):
    """Every B in BS x K in KS with K <= N. Largest error / bound measured on the device: see DESIGN §9k."""
    worst = 0.0
    for K in KS:
        if K > N:
            continue
        for B in BS:
            worst = max(worst, amplitude_ratio(batch(N)[:B], N, K))
    print(f"N = {N}: max err / bound = {worst:.4f}")


@pytest.mark.parametrize("B,N,K", [(3, 513, 65), (3, 2048, 256), (3, 1025, 32)])
def test_amplitudes_within_the_bound_at_the_wide_sizes(B, N, K):
    print(f"(B, N, K) = ({B}, {N}, {K}): max err / bound = {amplitude_ratio(batch(N)[:B], N, K):.4f}")


# ---------------------------------------------------------------- 2. by bit pattern
@pytest.mark.parametrize("B,N,K", [(37, 41, 17), (1100, 171, 32), (70, 171, 64), (5, 513, 65)])
def test_populations_and_batch_independence_by_bit_pattern(B, N, K):
    view = view_of(N, K)
    psi = batch(N)[:B]
    a = view.amplitudes(dev(psi))
    p = view.populations(dev(psi))
    assert p.shape == (B, K) and p.dtype == torch.float64
    assert same_bits(p.cpu().numpy(), R.populations_of(a.cpu().numpy()))
    # a repeat gives the same bits
    assert same_bits(words(view.amplitudes(dev(psi))), words(a)) and same_bits(words(view.populations(dev(psi))), words(p))
    # the rows one at a time, and in another order in another batch
    rows = [0, B - 1, B // 2]
    for b in rows:
        one = view.amplitudes(dev(psi[b]))
        assert one.shape == (1, K) and same_bits(words(one)[0], words(a)[b]), b
    perm = np.random.default_rng(B).permutation(B)
    shuffled = view.amplitudes(dev(psi[perm]))
    assert same_bits(words(shuffled), words(a)[perm])
    # NaN behind the batch changes nothing
    longer = np.concatenate([psi, np.full((3, N), np.nan + 1j * np.nan)])
    whole = dev(longer)
    assert same_bits(words(view.amplitudes(whole[:B])), words(a))
    assert same_bits(words(view.mean_populations(whole[:B])[0]), words(view.mean_populations(dev(psi))[0]))


def masks(B, rng):
    out = {"none": None, "all": np.ones(B, dtype=bool), "random": rng.random(B) < 0.5,
           "one": np.arange(B) == B // 3, "last": np.arange(B) == B - 1, "empty": np.zeros(B, dtype=bool)}
    return out


@pytest.mark.parametrize("B", [1, 31, 32, 33, 65, 1100])
def test_mean_equals_the_documented_order_on_the_devices_own_populations(B):
    N, K = 171, 33
    view = view_of(N, K)
    psi = batch(N)[:B]
    p = view.populations(dev(psi)).cpu().numpy()
    for name, mask in masks(B, np.random.default_rng(B)).items():
        m, count = view.mean_populations(dev(psi), None if mask is None else dev(mask))
        want, n = R.mean_documented_order(p, mask)
        assert m.shape == (K,) and m.dtype == torch.float64 and count.dtype == torch.int64
        assert int(count) == n, name
        assert same_bits(m.cpu().numpy(), want), (B, name)
        if mask is not None and name != "all":
            # a uint8 mask is the same mask; a masked env holding NaN / Inf gives the bits of one holding zeros
            m8, _ = view.mean_populations(dev(psi), dev(mask.astype(np.uint8) * 7))
            assert same_bits(m8.cpu().numpy(), want)
            poisoned, zeroed = psi.copy(), psi.copy()
            poisoned[~mask] = np.nan + 1j * np.inf
            zeroed[~mask] = 0
            mp, _ = view.mean_populations(dev(poisoned), dev(mask))
            mz, _ = view.mean_populations(dev(zeroed), dev(mask))
            assert same_bits(mp.cpu().numpy(), want) and same_bits(mz.cpu().numpy(), want), (B, name)
    # more than one level block: K = 65 at N = 171
    wide = view_of(N, 65)
    mw, _ = wide.mean_populations(dev(psi))
    assert same_bits(mw.cpu().numpy(), R.mean_documented_order(wide.populations(dev(psi)).cpu().numpy())[0])


# ---------------------------------------------------------------- 3. the conventions
def test_quartic_conventions_against_the_stepper_and_the_ensemble_view():
    P = _pkg()
    cfg = P["cfg"]
    ph = cfg.DEFAULTS[cfg.QO]
    K, B, h = 16, 24, ph.grid_size
    view = P["LevelView"].for_physics(ph, K)
    assert (view.n, view.k) == (ph.dim, K) and view.scale == math.sqrt(h)
    assert view.vectors.shape == (K, ph.dim) and view.energies.shape == (K,) and view.energies.is_cuda
    E, V = P["LevelView"].solve(ph, K)
    assert same_bits(view.vectors.cpu().numpy(), V) and same_bits(view.energies.cpu().numpy(), E)
    rng = np.random.default_rng(3)
    c = rng.standard_normal((B, K)) + 1j * rng.standard_normal((B, K))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    psi = dev((c @ V) / math.sqrt(h))
    a = view.amplitudes(psi)
    p = view.populations(psi)
    a_err = np.abs(a.cpu().numpy() - c).max()
    s_err = np.abs(p.sum(dim=1).cpu().numpy() - 1).max()
    st = P["Stepper"](ph, B, 0, seed=1)
    e_err = np.abs(view.mean_energy(p).cpu().numpy() - st.energy(psi).cpu().numpy()).max()
    print(f"quartic conventions: amplitudes {a_err:.3e}, sum {s_err:.3e}, energy {e_err:.3e}")
    assert a_err <= 1e-9 and s_err <= 1e-9 and e_err <= 1e-9
    # the density matrix in the level basis: EnsembleView(K) on the amplitudes, and V rho_x V^T
    mask = dev(np.arange(B) % 4 != 1)
    m, count = view.mean_populations(psi, mask)
    ev = P["EnsembleView"](K, 1.0)
    rho_k, n = ev.density_matrix(a, mask)
    assert int(n) == int(count) == 18
    assert np.abs(ev.populations(rho_k).cpu().numpy() - m.cpu().numpy()).max() <= 1e-9
    ex = P["EnsembleView"].for_physics(ph)
    rho_x, _ = ex.density_matrix(psi, mask)
    Vc = view.vectors.to(torch.complex128)
    moved = Vc @ rho_x @ Vc.T                         # (the states carry 1 / sqrt(h) each, rho_x the factor h)
    assert np.abs(moved.cpu().numpy() - rho_k.cpu().numpy()).max() <= 1e-9
    for o in (view, ev, ex, st):
        o.close()


def test_harmonic_conventions():
    P = _pkg()
    cfg = P["cfg"]
    ph = cfg.DEFAULTS[cfg.HO]
    view = P["LevelView"].for_physics(ph, 71)
    assert (view.n, view.k, view.scale) == (71, 71, 1.0)
    psi = states(40, 71, 5)
    p = view.populations(dev(psi))
    assert np.abs(p.cpu().numpy() - np.abs(psi) ** 2).max() <= 1e-9
    mask = dev(np.arange(40) % 3 != 0)
    m, _ = view.mean_populations(dev(psi), mask)
    ev = P["EnsembleView"].for_physics(ph)
    rho, _ = ev.density_matrix(dev(psi), mask)
    assert np.abs(m.cpu().numpy() - ev.populations(rho).cpu().numpy()).max() <= 1e-9
    want = (np.abs(psi) ** 2 * ph.omega * (0.5 + np.arange(71))).sum(axis=1)
    assert np.abs(view.mean_energy(p).cpu().numpy() - want).max() <= 1e-9
    view.close()
    ev.close()


def test_the_table_route_through_the_spatial_views_table():
    """Fock amplitudes of grid states relative to a reference oscillator: SpatialView's table as the level table."""
    P = _pkg()
    cfg = P["cfg"]
    ph = cfg.DEFAULTS[cfg.QO]
    h, X, n = ph.grid_size, ph.dim, 12
    x = (np.arange(X) - (X - 1) // 2) * h
    sv = P["SpatialView"](n, x)
    tab = sv.table().cpu().numpy().T[:n]              # [12, X]
    view = P["LevelView"](np.ascontiguousarray(tab), scale=h)
    rng = np.random.default_rng(12)
    c = rng.standard_normal((9, n)) + 1j * rng.standard_normal((9, n))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    phi = sv.repr(dev(c))
    a = view.amplitudes(phi).cpu().numpy()
    f = phi.cpu().numpy()
    wre, wim = R.amplitudes_longdouble(f, tab, h)
    bre, bim = R.bound(f, tab, h)
    assert np.all(np.abs(a.real - wre) <= bre) and np.all(np.abs(a.imag - wim) <= bim)
    print(f"table route: |a - c| = {np.abs(a - c).max():.3e} (the grid's quadrature error)")
    assert np.abs(a - c).max() <= 1e-6                # (the same states, up to the quadrature error of the grid)
    sv.close()
    view.close()


def test_populations_of_a_stepped_quartic_env_stay_in_band():
    P = _pkg()
    cfg = P["cfg"]
    ph = cfg.DEFAULTS[cfg.QO]
    B = 64
    env = P["BatchedEnv"](ph, B, 0, seed=9, input="xp", reset="warmup")
    env.reset()
    rng = np.random.default_rng(2)
    for _ in range(3):
        env.step(dev(rng.integers(0, ph.n_actions, B).astype(np.int32)))
    view = P["LevelView"].for_physics(ph)
    assert view.k == 32
    p = env.level_populations(view).cpu().numpy()
    assert p.shape == (B, 32) and p.min() >= 0 and p.max() <= 1 + 1e-12
    print(f"stepped env: 1 - sum_k p in [{(1 - p.sum(axis=1)).min():.3e}, {(1 - p.sum(axis=1)).max():.3e}]")
    assert (1 - p.sum(axis=1)).min() >= -1e-12
    view.close()
    env.st.close()


# ---------------------------------------------------------------- 4. refusals
def test_refusals():
    P = _pkg()
    LV, QE = P["LevelView"], P["_lib"].QCartError
    good_table = R.unit_rows(np.random.default_rng(1), 4, 9)
    with pytest.raises(ValueError, match="float64"):
        LV(good_table.astype(np.float32))
    with pytest.raises(ValueError, match="float64"):
        LV(good_table[0])
    with pytest.raises(ValueError, match="CPU tensor"):
        LV(torch.from_numpy(good_table).cuda())
    with pytest.raises(ValueError, match="energies"):
        LV(good_table, energies=np.zeros(5))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(QE, match="scale must be finite and > 0"):
            LV(good_table, bad)
    with pytest.raises(QE, match=r"K must be in \[1, min\(N, 256\)\]"):
        LV(np.zeros((10, 9)))
    with pytest.raises(QE, match="every table entry must be finite"):
        LV(np.where(np.arange(36).reshape(4, 9) == 7, np.nan, good_table))
    cfg = P["cfg"]
    for fam in (cfg.IHO, cfg.IQO):
        with pytest.raises(ValueError, match="no bound levels: H is not bounded below"):
            LV.for_physics(cfg.DEFAULTS[fam])
    view = LV(torch.from_numpy(good_table), 0.5)      # a CPU tensor is taken
    assert (view.n, view.k, view.scale, view.energies) == (9, 4, 0.5, None)
    with pytest.raises(ValueError, match="without energies"):
        view.mean_energy(torch.zeros(4, dtype=torch.float64, device="cuda"))
    good = dev(states(4, 9, 1))
    for call in (view.amplitudes, view.populations, view.mean_populations):
        with pytest.raises(ValueError, match="complex128.*complex64 states are not viewed"):
            call(good.to(torch.complex64))
        with pytest.raises(ValueError, match="9 components"):
            call(dev(states(4, 8, 1)))                # a view of another N
        with pytest.raises(ValueError, match="must live on"):
            call(good.cpu())
        with pytest.raises(ValueError):
            call(good[:, None, :])
        with pytest.raises(ValueError, match="torch tensor"):
            call(good.cpu().numpy())
    with pytest.raises(ValueError, match="mask"):
        view.mean_populations(good, torch.ones(5, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="mask"):
        view.mean_populations(good, torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="mask"):
        view.mean_populations(good, torch.ones(4, dtype=torch.int32, device="cuda"))
    # the library's own refusals, below the Python checks
    lib, vp = P["_lib"].lib(), ctypes.c_void_p
    out = torch.empty(4, 4, dtype=torch.complex128, device="cuda")
    assert lib.qc_levels_amplitudes(view._h, vp(good.data_ptr()), 0, vp(out.data_ptr())) == -1
    assert b"qc_levels_amplitudes: B must be >= 1" in lib.qc_levels_last_error(view._h)
    assert lib.qc_levels_populations(view._h, None, 4, vp(out.data_ptr())) == -1
    assert b"qc_levels_populations: psi and out are required" in lib.qc_levels_last_error(view._h)
    assert lib.qc_levels_mean(view._h, vp(good.data_ptr()), 4, None, None, None) == -1
    assert b"qc_levels_mean: psi and out are required" in lib.qc_levels_last_error(view._h)
    assert lib.qc_levels_amplitudes(None, vp(good.data_ptr()), 4, vp(out.data_ptr())) == -1
    # a call without a count pointer is fine
    m = torch.empty(4, dtype=torch.float64, device="cuda")
    assert lib.qc_levels_mean(view._h, vp(good.data_ptr()), 4, None, vp(m.data_ptr()), None) == 0
    assert same_bits(m.cpu().numpy(), view.mean_populations(good)[0].cpu().numpy())
    one = view.populations(good[2])                   # one [n] state is B = 1
    assert one.shape == (1, 4) and same_bits(one.cpu().numpy()[0], view.populations(good).cpu().numpy()[2])
    view.close()
    view.close()


# ---------------------------------------------------------------- 5. BatchedEnv.level_populations
def digest(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def test_env_level_populations_is_the_view_on_psi_and_has_no_side_effect():
    P = _pkg()
    cfg = P["cfg"]
    ph = cfg.DEFAULTS[cfg.QO]
    B = 33
    view = P["LevelView"].for_physics(ph, 16)
    envs = [P["BatchedEnv"](ph, B, 0, seed=17, input="xp", reset="warmup") for _ in range(2)]
    acts = [dev(np.random.default_rng(40 + i).integers(0, ph.n_actions, B).astype(np.int32)) for i in range(4)]
    mask = dev(np.random.default_rng(44).random(B) < 0.5)
    for env in envs:
        env.reset()
        for a in acts[:3]:
            env.step(a)
    env = envs[0]
    before = digest(env.psi)
    p = env.level_populations(view)
    m, count = env.level_populations(view, mean=True, mask=mask)
    assert same_bits(p.cpu().numpy(), view.populations(env.psi).cpu().numpy())
    m2, count2 = view.mean_populations(env.psi, mask)
    assert int(count) == int(count2) == int(mask.sum()) and same_bits(m.cpu().numpy(), m2.cpu().numpy())
    assert np.abs(m.cpu().numpy() - p.cpu().numpy()[mask.cpu().numpy()].mean(axis=0)).max() <= 1e-14
    with pytest.raises(ValueError, match="mask goes with mean = True"):
        env.level_populations(view, mask=mask)
    assert digest(env.psi) == before == digest(envs[1].psi)
    for e in envs:                                   # and the env goes on as the twin never asked
        e.step(acts[3])
    assert digest(envs[0].psi) == digest(envs[1].psi) and digest(envs[0].obs) == digest(envs[1].obs)
    view.close()
    for e in envs:
        e.st.close()


# ---------------------------------------------------------------- 6. Trainer.evaluate(levels=view)
def evaluate_with_levels(loop, tmp_path, K):
    P = _pkg()
    tr = loop.trainer(tmp_path / "models")
    env = loop.env
    env.reset()
    for _ in range(6):
        env.step(loop.actor.act(env.obs, eps=0.05))
    tr.save_checkpoint(tmp_path / "start.pt")
    view = P["LevelView"].for_physics(loop.c["ph"], K)
    with_trace = tr.evaluate(None, 10 ** 6, max_steps=9, levels=view)
    assert len(tr.level_trace) == 9 and tr.density_trace == [] and tr.purity_trace == []
    pops = torch.stack(tr.level_trace).cpu().numpy()
    assert pops.shape == (9, K) and np.all(pops >= 0) and np.all(pops.sum(axis=1) <= 1 + 1e-12)
    assert pops.sum(axis=1).max() > 0.5              # (a step without a valid env has count 0: zeros)
    print(f"level trace: ground state {pops[:, 0].min():.4f} .. {pops[:, 0].max():.4f}, "
          f"in band {pops.sum(axis=1).min():.6f} .. {pops.sum(axis=1).max():.6f}")
    # the first entry: the ensemble after the first control step from the start state, under that step's mask
    tr.load_checkpoint(tmp_path / "start.pt")
    info = env.step(loop.actor.act(env.obs, eps=0.0, noisy=False))[3]
    first, _ = view.mean_populations(env.psi, info["valid"])
    assert same_bits(first.cpu().numpy(), pops[0])
    # the returned tuple is bit for bit the one without the view, and the trace starts empty with each call
    tr.load_checkpoint(tmp_path / "start.pt")
    plain = tr.evaluate(None, 10 ** 6, max_steps=9)
    assert tr.level_trace == []
    assert np.array(with_trace).tobytes() == np.array(plain).tobytes()
    view.close()


def test_evaluate_performance_with_a_level_trace_on_the_quartic_loop(tmp_path):
    from tests.test_gpu_trainer_monitor import Loop
    loop = Loop("qo")
    assert loop.monitor is not None
    evaluate_with_levels(loop, tmp_path, 32)
    loop.close()


def test_evaluate_with_a_level_trace_on_the_harmonic_loop(tmp_path):
    from tests.test_gpu_trainer import Loop
    loop = Loop("ho")
    evaluate_with_levels(loop, tmp_path, 64)
    loop.close()


# ---------------------------------------------------------------- 7. the command line
def test_command_line_writes_the_npz(tmp_path):
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import train
    out = tmp_path / "levels.npz"
    rc = train.main(["--system", "qo", "--control_strategy", "damping", "--envs", "32", "--num_of_test_episodes", "4",
                     "--max_steps", "5", "--save_dir", str(tmp_path / "run"), "--levels_out", str(out),
                     "--levels", "24"])
    assert rc == 0
    z = np.load(out)
    assert sorted(z.files) == ["energies", "populations"]
    steps = z["populations"].shape[0]
    assert 1 <= steps <= 5 and z["populations"].shape == (steps, 24) and z["populations"].dtype == np.float64
    assert z["energies"].shape == (24,) and abs(z["energies"][0] - 0.71769) <= 5e-6
    with pytest.raises(SystemExit):
        train.main(["--system", "iho", "--control_strategy", "LQG", "--envs", "32", "--max_steps", "2",
                    "--save_dir", str(tmp_path / "run"), "--levels_out", str(out)])
