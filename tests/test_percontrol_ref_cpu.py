"""CPU checks of tests/percontrol_ref.py, the checker of the per-control-step kernels (k_obs, k_aux, k_control,
k_reset; tests/test_gpu_percontrol.py): the extended-precision reference is pinned to the C oracle on the states and
sizes the GPU tests use, the states are shown to see every class of kernel bug the GPU tests are meant to catch
(each bug applied to the reference), and the controller probes are shown to sit on a known side of their rounding
boundary on the oracle's own path. No disagreement between the reference and the oracle was found.
"""
import numpy as np
import pytest

from oracle import controllers as OC
from tests import percontrol_ref as PR
from tests.percontrol_ref import BY_ID, GRID_IDS, IDS, moment_bar, oracle_sys, xths


def all_states(ph):
    xth = None if ph.fock else xths(ph)[0]
    return [("tail", PR.tail_states(ph, PR.BATCH)), ("edge", PR.edge_states(ph, xth)[1]),
            ("thr", PR.threshold_states(ph)[1])]


def moment_states(ph, order):
    """The states the GPU test runs through the moments at this order."""
    xth = None if ph.fock else xths(ph)[0]
    edge = PR.edge_states(ph, xth)[1] if order > 9 else PR.default_order_edge_states(ph, xth)[1]
    return [("tail", PR.tail_states(ph, PR.BATCH)), ("edge", edge)]


def test_case_table():
    assert len(IDS) == len(set(IDS)) == 25 and sum(i.endswith("_f32") for i in IDS) == 6
    for name, ph, R in PR.CASES:
        assert PR.rows_per_lane(ph) == R and 64 * R >= ph.dim, name
        assert -(-ph.dim // R) < 64, name     # idle lanes (and a part-filled last lane where R does not divide N)
    assert {i: BY_ID[i][1].dim for i in GRID_IDS} == {"qo35_R1": 35, "qo87_R2": 87, "qo171_R3": 171, "qo285_R5": 285,
                                                      "qo567_R9": 567, "qo1063_R17": 1063, "iqo301_R5": 301,
                                                      "iqo513_R9": 513}
    lanes = {i: -(-BY_ID[i][1].dim // BY_ID[i][2]) for i in IDS}
    assert lanes["ho257_R8"] == 33 and lanes["iho65_R2"] == 33 and lanes["ho600_R32_f32"] == 19


@pytest.mark.parametrize("case", IDS)
def test_states_have_weight_on_every_row_and_stay_tame(case):
    _, ph, R = BY_ID[case]
    ref, N = PR.ref_of(ph), ph.dim
    ts = PR.tail_states(ph, PR.BATCH)
    assert ts.dtype == PR.state_dtype(ph) and (np.abs(ts) > 0).all()
    assert np.array_equal(ts, PR.tail_states(ph, PR.BATCH))      # seeded
    for p in ts:
        w = p.astype(np.complex128)
        assert 1e-6 < np.linalg.norm(w[N - PR.top_rows(N):]) / np.linalg.norm(w) < 1e-3
        assert abs(np.linalg.norm(w) ** 2 * PR.weight(ph) - 1) < 1e-6
    rows = PR.edge_rows(ph, None if ph.fock else xths(ph)[0])
    want = {0, R - 1, R, N - 1, ((N - 1) // R) * R, ref.bnd_len - 1, ref.bnd_len, N - ref.bnd_len - 1, N - ref.bnd_len}
    assert want <= set(rows)
    if not ph.fock:
        lo, hi = ref.window(xths(ph)[0])
        assert 0 < lo - 1 and hi < N and {lo - 1, lo, hi - 1, hi} <= set(rows)
    factors, th = PR.threshold_states(ph)
    for (fu, fl), p in zip(factors, th):
        fail, top, bot = ref.boundary_fail(p)
        for f, nrm in ((fu, top), (fl, bot)):
            assert abs(nrm / ref.fail_thr - f) < 1e-6 * max(f, 1) and not 1 / 1.01 < nrm / ref.fail_thr < 1.01
        assert fail == int(fu > 1 or (fl > 1 and not ph.fock))


@pytest.mark.parametrize("case", IDS)
def test_reference_matches_oracle(oracle_mod, case):
    """Every scalar within the derived bound (N + 64) 2^-53 sum |t_i| of the oracle's fp64 value, the flags equal,
    H psi within (2 kl + 8) 2^-53 sum |H_rc psi_c| per row, the moments within a tenth of the project's bar."""
    _, ph, _ = BY_ID[case]
    ref, osys = PR.ref_of(ph), oracle_sys(oracle_mod, ph)
    o10 = None if ph.fock else oracle_sys(oracle_mod, ph, 10)
    H = osys.dense_h()
    assert np.abs(H - ref.H64).max() <= 4 * 2.0 ** -53 * np.abs(H).max()
    for kind, states in all_states(ph):
        for p in states:
            w = p.astype(np.complex128)
            for s, o in ((ref.x_expectation(p), osys.x_expectation(w)), (ref.energy(p), osys.energy(w))):
                assert abs(s.value - o) <= s.tol, (kind, s.value, o, s.tol)
            if ph.fock:
                s = ref.phonon(p)
                assert abs(s.value - osys.phonon(w)) <= min(s.tol, 1e-13 * max(abs(s.value), 1))
            else:
                for xth in xths(ph):
                    s = ref.outside_prob(p, xth)
                    assert abs(s.value - osys.outside_prob(w, xth)) <= min(s.tol, 1e-13)
            assert ref.boundary_fail(p)[0] == osys.boundary_fail(w)
            hp, tol = ref.h_psi(p)
            assert (np.abs((H @ w) - hp.astype(np.complex128)) <= tol * 2).all()     # (re and im: sqrt(2) <= 2)
            if not ph.fock and kind != "thr":
                m = ref.moments(p, 10).astype(np.float64)
                assert (np.abs(o10.moments(w) - m) <= 0.1 * moment_bar(m, 10)).all(), kind
    # the default order: on the tail states and on the edge probes that Ref.moments_within_fp64 admits; every one of
    # these states is admitted, and every grid keeps probes on both sides of its first lane boundary
    for kind, states in moment_states(ph, ph.moment_order):
        assert len(states) >= PR.BATCH and all(ph.fock or ref.moments_within_fp64(p) for p in states), kind
    for kind, states in moment_states(ph, ph.moment_order):
        for p in states:
            m = ref.moments(p).astype(np.float64)
            err = np.abs(osys.moments(p.astype(np.complex128)) - m)
            assert (err <= 0.1 * moment_bar(m, ph.moment_order)).all(), (kind, (err / moment_bar(m, 5)).max())


@pytest.mark.parametrize("case", [i for i in IDS if BY_ID[i][1].fock])
def test_fock_resets_match_oracle(oracle_mod, case):
    _, ph, _ = BY_ID[case]
    ref, osys = PR.ref_of(ph), oracle_sys(oracle_mod, ph)
    for levels in (1, 16, ph.dim, ph.dim + 5):
        for e in (0, 3):
            v = ref.reset_random(osys, 1234, 10 + e, levels)
            assert np.abs(v.astype(np.complex128) - osys.fock_random_state(1234, 10 + e, levels)).max() < 1e-15
            assert np.count_nonzero(v) == min(levels, ph.dim)
    g = ref.reset_ground()
    assert g[0] == 1 and np.count_nonzero(g) == 1


def test_kind2_bar_is_eight_times_the_measured_libm_error(oracle_mod):
    """The Gaussian packet in extended precision against the oracle's libm exp / sin / cos on every packet the GPU
    test resets to: measured worst |difference| 2.5e-16 (where the fp64 phase 2 pi (x - mean) k is large the envelope
    is small), recorded as 3e-16; the bar of reset kind 2 is 8 x 3e-16 = 2.4e-15, so that two libraries may differ from
    the exact value by a few ulp each. At (0, 0, 1) the packet is real and the project's 1e-15 holds."""
    worst = 0.0
    for case in GRID_IDS:
        ph = BY_ID[case][1]
        ref, osys = PR.ref_of(ph), oracle_sys(oracle_mod, ph)
        k, mu, sg = PR.kind2_env_params(PR.BATCH)
        for a, b, c in PR.KIND2_PARAMS + list(zip(k, mu, sg)) + [(x, 0.0, 1.0) for x in k]:
            d = np.abs(ref.reset_packet(a, b, c).astype(np.complex128) - osys.gaussian_packet(a, b, c)).max()
            worst = max(worst, d)
            if (a, b, c) == (0.0, 0.0, 1.0):
                assert d < 1e-15
    print("worst |longdouble packet - oracle packet| =", worst)
    assert PR.KIND2_MEASURED / 2 <= worst <= PR.KIND2_MEASURED and PR.KIND2_BAR == 8 * PR.KIND2_MEASURED, worst


# ---- sensitivity: each class of kernel bug, applied to the reference --------------------------------------------
def _outputs(ref, p, xth):
    """{name: (value, tolerance)} of every scalar and stored output the GPU test compares."""
    out = {"x": ref.x_expectation(p), "E": ref.energy(p)}
    out.update({"n": ref.phonon(p)} if ref.fock else {"out": ref.outside_prob(p, xth)})
    out = {k: (np.array([s.value]), np.array([s.tol])) for k, s in out.items()}
    hp, tol = ref.h_psi(p)
    out["Hre"], out["Him"] = (hp.real.astype(np.float64), tol), (hp.imag.astype(np.float64), tol)
    order = ref.ph.moment_order if ref.fock else 10
    m = ref.moments(p, order).astype(np.float64)
    out["mom"] = (m, moment_bar(m, order))
    return out


def _moved(a, b):
    """Some output differs by more than 100 x its tolerance, or the Fail flag flips."""
    return any((np.abs(a[k][0] - b[k][0]) > 100 * a[k][1]).any() for k in a)


def _seen(ph, mutate=None, cut=None):
    """Does any tail or edge state see the bug? mutate(psi) edits the loaded rows, cut removes one halo."""
    good, bad = PR.ref_of(ph), (PR.Ref(ph, cut=cut) if cut is not None else PR.ref_of(ph))
    xth = None if ph.fock else xths(ph)[0]
    hits = {}
    for kind, states in all_states(ph)[:2]:
        for p in states:
            q = mutate(p.copy()) if mutate else p
            flip = good.boundary_fail(p)[0] != bad.boundary_fail(q)[0]
            if flip or _moved(_outputs(good, p, xth), _outputs(bad, q, xth)):
                hits[kind] = hits.get(kind, 0) + 1
    return hits


def _moments_see(ph, mutate=None, cut=None):
    """Per moments instantiation the GPU test runs (Fock: the 5 observables; grid: the default order and order 10),
    the kinds of its own states on which the bug moves a moment by more than 100 x the bar."""
    good, bad = PR.ref_of(ph), (PR.Ref(ph, cut=cut) if cut is not None else PR.ref_of(ph))
    out = {}
    for order in [ph.moment_order] + ([] if ph.fock else [10]):
        hits = set()
        for kind, states in moment_states(ph, order):
            for p in states:
                a = good.moments(p, order).astype(np.float64)
                b = bad.moments(mutate(p.copy()) if mutate else p, order).astype(np.float64)
                if (np.abs(a - b) > 100 * moment_bar(a, order)).any():
                    hits.add(kind)
        out[order] = hits
    return out


def _zero_from(r):
    def f(p):
        p[r:] = 0
        return p
    return f


@pytest.mark.parametrize("case", IDS)
def test_dropped_rows_are_seen(case):
    """A guard that loses the last row, or every row of the last active lane: seen by the tail states (every one of
    them) and by the edge states."""
    _, ph, R = BY_ID[case]
    N = ph.dim
    for first in (N - 1, ((N - 1) // R) * R):
        hits = _seen(ph, mutate=_zero_from(first))
        assert hits.get("tail", 0) == PR.BATCH and hits.get("edge", 0) >= 1, (first, hits)
        # each moments kernel's own states: at order 10 the edge states (the bar's share of the largest entry hides one
        # row of a tail), at the default order the tail states (on a fine grid no few-row state at the top is within
        # fp64's reach of the order-5 bar)
        for order, kinds in _moments_see(ph, mutate=_zero_from(first)).items():
            assert ("edge" if order > 9 else "tail") in kinds and (kinds == {"tail", "edge"} or not ph.fock), \
                (first, order, kinds)


@pytest.mark.parametrize("case", IDS)
def test_lost_halo_is_seen(case):
    """The coupling across the first lane boundary, and across the last active lane's, set to zero."""
    _, ph, R = BY_ID[case]
    for b in (R, ((ph.dim - 1) // R) * R):
        hits = _seen(ph, cut=b)
        assert hits.get("edge", 0) >= 1, (b, hits)
        if b == R:
            assert hits.get("tail", 0) >= 1, (b, hits)     # (the packet lives on the low rows)
        # each moments kernel's own states (the grid moments' truncated band has no entry on row or column N - 1:
        # with one row in the last lane there is no halo to lose)
        for order, kinds in _moments_see(ph, cut=b).items():
            want = "edge" if ph.fock or order > 9 else ("edge" if b == R else "tail")
            assert (want in kinds) == (ph.fock or b < ph.dim - 1), (b, order, kinds)


@pytest.mark.parametrize("case", IDS)
def test_shifted_windows_are_seen(case):
    _, ph, _ = BY_ID[case]
    ref = PR.ref_of(ph)
    xth = None if ph.fock else xths(ph)[0]
    es, th = PR.edge_states(ph, xth)[1], PR.threshold_states(ph)[1]
    shifts = [dict(shift_top=1), dict(shift_top=-1)] + ([] if ph.fock else [dict(shift_bot=1), dict(shift_bot=-1)])
    for kw in shifts:
        assert any(ref.boundary_fail(p)[0] != ref.boundary_fail(p, **kw)[0] for p in es), kw
    # (the one-row states are the windows' probes; the threshold states pin the threshold itself, at 0.5 x and 2 x)
    assert {ref.boundary_fail(p)[0] for p in th} == {0, 1}
    if not ph.fock:
        for x in xths(ph):
            for kw in (dict(shift_lo=1), dict(shift_lo=-1), dict(shift_hi=1), dict(shift_hi=-1)):
                es_x = PR.edge_states(ph, x)[1]
                d = [abs(ref.outside_prob(p, x).value - ref.outside_prob(p, x, **kw).value)
                     - 100 * ref.outside_prob(p, x).tol for p in es_x]
                assert max(d) > 0, (x, kw)
        if ph.grid_size == 0.5:     # the ties: round(2.5) = 2 and round(3.5) = 4
            assert ref.window(1.25) == (ph.dim // 2 - 2, ph.dim // 2 + 2)
            assert ref.window(1.75) == (ph.dim // 2 - 4, ph.dim // 2 + 4)


# ---- controller probes ------------------------------------------------------------------------------------------
def _oracle_control(ph, state, strategy, kw, fops):
    """oracle/controllers.py on its own path: float32 data for the Fock families, fp64 dense sums for the grids."""
    w = state.astype(np.complex128)
    if ph.fock:
        return OC.fock_lqg(w, ph.family, ph.omega, ph.n_con, ph.f_max, kw["input_scaling"], fops)
    T = kw.get("control_time", 1.0 / ph.n_con)
    return OC.grid_control(PR.DeviceGrid(ph), w, strategy, kw.get("con_parameter", 0.0), ph.lambda_, ph.mass,
                           ph.n_con, ph.f_max, control_time=T)


@pytest.mark.parametrize("case", IDS)
def test_probes_sit_on_a_known_side_of_their_boundary(case):
    """Every probed env of every strategy has its probe (none is excluded), the oracle's own path gives the expected
    action and force on both sides at eps, eps / 2 and 2 eps, the asserted envs span at least four unsaturated action
    levels and the last env saturates."""
    _, ph, _ = BY_ID[case]
    ref = PR.ref_of(ph)
    eps = PR.EPS_FOCK if ph.fock else PR.EPS_GRID
    ts = PR.tail_states(ph, PR.BATCH)
    fops = OC.fock_ops(ph.n_max) if ph.fock else None
    for strategy in PR.strategies(ph):
        levels = set()
        for e in range(PR.BATCH):
            k = "sat" if e == PR.BATCH - 1 else e
            for f in (1.0, 0.5, 2.0):
                pr = PR.probe(ref, ts[e], strategy, k, eps * f)
                assert pr is not None, (strategy, e)
                for kw, act, force in pr:
                    assert ref.control(ts[e], strategy, **kw) == (act, force)
                    assert _oracle_control(ph, ts[e], strategy, kw, fops) == (act, force), (strategy, e, f, kw)
                    if k == "sat":
                        assert act in (0, 20) and abs(force) == ph.f_max
                    else:
                        levels.add(act)
                if k != "sat":
                    assert abs(pr[0][1] - pr[1][1]) == 1
        assert len(levels - {0, 20}) >= 4, (strategy, levels)
    if ph.family == PR.IQO:
        act, force = ref.control(ts[0], "semiclassical")
        assert act == -1 and np.isnan(force)
        assert np.isnan(ref.grid_force(ts[0], "LQG", 1.0))       # lambda * con_parameter < 0


@pytest.mark.parametrize("case", GRID_IDS)
def test_truncated_momentum_band_flips_every_top_band_probe(case):
    """The controllers use space_def's full antisymmetric p band; with the moments' truncated Hermitian band in its
    place every probed env of the top-band states misses an expected action (on the tail states, whose phase varies
    slowly from row to row, the two bands differ by less than eps on most grids). The probes are the oracle's own on
    both sides."""
    _, ph, _ = BY_ID[case]
    ref = PR.ref_of(ph)
    tb = PR.top_band_states(ph)
    assert len(tb) == PR.BATCH
    for strategy in PR.TOP_BAND_STRATEGIES[ph.family]:
        levels = set()
        for e in range(PR.BATCH):
            pr = PR.probe(ref, tb[e], strategy, e % 6, PR.EPS_GRID)
            assert pr is not None, (strategy, e)
            for kw, act, force in pr:
                assert _oracle_control(ph, tb[e], strategy, kw, None) == (act, force), (strategy, e)
                levels.add(act)
            # (the truncated band's force hardly moves between the two sides: it cannot give both expected actions)
            assert any(ref.control(tb[e], strategy, truncated=True, **kw)[0] != act for kw, act, _ in pr), (strategy, e)
        assert len(levels - {0, 20}) >= 4
