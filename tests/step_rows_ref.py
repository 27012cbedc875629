"""The step kernel (k_step of csrc/qcart_kernels.hpp) under states that fill every lane (test infrastructure): the
cases, the states, one step of SURVEY.md Appendix A read by diagonal at either working precision, and the kernel
bugs the states are there to see, applied to that restatement.

Cases: percontrol_ref.CASES, one ragged size per <family, rows per lane, precision> instantiation (19 fp64 and 6
fp32); the two fine grids run at the time step of test_gpu_parity.EDGE_SIZES (1/5760 and 1/11520: the scheme is
unstable there at 1/1440).

States (state_sets): percontrol_ref's tail_states and edge_states as they stand, and two new sets. sweep_states: per
lane boundary b = k R, 0 < b < N, the two-row state 0.8 |b - 1> + 0.6 e^{i pi / 4} |b>; it carries the stencils' and
the solve's couplings across that boundary, for every lane of the wave (the edge states reach the first and the last).
flat_states: |psi_r| equal on every row with independent uniform phases; anything wrong on any row, lane or scan carry
moves them by about 1 / sqrt(N) times the coupling. plan() gives every state its own force slot and its own Wiener
noise, so a state's trajectory does not depend on the batch it runs in.

The restatement (Ops, step): refmath.dense_step with the operators held as diagonals (applied like
percontrol_ref._mv, in the state's precision) and LAPACK's banded solver in place of the dense one. H_F, X, A_eff
(refmath.correction_A under refmath.mirror's descriptor semantics) and M = I + i dt / 2 H_F are built in fp64. At
RT = float64 this is the dense fp64 restatement (tests/test_step_rows_cpu.py pins it to refmath.dense_step). At
RT = float32 it follows DESIGN.md §4's fp32 rules: the operators rounded once to float32 / complex64, all vector
arithmetic complex64, the means, the norm and the per-step scalars (dW, dZ, the SRK coefficients) fp64. The fp32
restatement is not a second reference: its distance to the fp64 oracle, r32, is "fp32 rounding alone" on that state,
the scale of the fp32 kernels' bar.

Bug injectors (inject): the operators cut at a row b (a lost lane halo), the rows from `first` on dropped (first =
N - 1: the last row; the first row of the last active lane: that lane), and the solve's table rows of the last active
lane shifted by one towards the padding (row r reads row r + 1's coefficients, the last row the padding's identity
row: csrc/qcart_tables.cpp pads lc / uc with 0 and 1 / U_rr with 1).
"""
from __future__ import annotations

from functools import lru_cache
from math import pi, sqrt

import numpy as np
import scipy.sparse as sp
from scipy.linalg import solve_banded

from tests import percontrol_ref as PR
from tests import refmath as RM
from tests.percontrol_ref import HO, IHO, IQO, QO  # noqa: F401

FINE_DT = {"qo567_R9": 5760, "qo1063_R17": 11520}     # test_gpu_parity.EDGE_SIZES


def _cases():
    return [(name, ph.with_(time_steps=FINE_DT[name]) if name in FINE_DT else ph, r) for name, ph, r in PR.CASES]


CASES = _cases()
IDS = [c[0] for c in CASES]
BY_ID = {c[0]: c for c in CASES}
F32_IDS = [i for i in IDS if BY_ID[i][1].precision == 1]
BATCH = PR.BATCH
STEPS = (1, 8)               # the GPU test's two calls per state set
KINDS = ("tail", "edge", "sweep", "flat")
PSI_BAR_FP64 = 1e-11         # test_psi_parity_every_rows_per_lane's
F32_FACTOR = 8               # over r32 (KIND2_BAR's margin over a measured rounding figure)
SEED = 20


# ================================================================================================
# states
# ================================================================================================
def lane_boundaries(ph):
    R = PR.rows_per_lane(ph)
    return list(range(R, ph.dim, R))


def two_row_state(ph, b):
    """0.8 |b - 1> + 0.6 e^{i pi / 4} |b>, normalised with the family's weight."""
    psi = np.zeros(ph.dim, dtype=np.complex128)
    s = 1.0 / sqrt(PR.weight(ph))
    psi[b - 1], psi[b] = 0.8 * s, 0.6 * s * np.exp(0.25j * pi)
    return psi


def sweep_states(ph):
    return np.stack([two_row_state(ph, b) for b in lane_boundaries(ph)]).astype(PR.state_dtype(ph))


def flat_states(ph, B=BATCH, seed=0):
    rng = np.random.default_rng([seed, 5, ph.family, ph.dim])
    N = ph.dim
    psi = np.exp(2j * pi * rng.uniform(size=(B, N))) / sqrt(N * PR.weight(ph))
    return psi.astype(PR.state_dtype(ph))


def sixteen_level_states(ph, oracle_mod, n):
    """What the older stepping tests start from (test_gpu_parity.init_states): fock_random_state(seed, e, 16)."""
    osys = PR.oracle_sys(oracle_mod, ph)
    return np.stack([osys.fock_random_state(1234, e, 16) for e in range(n)])


@lru_cache(maxsize=None)
def state_sets(case):
    ph = BY_ID[case][1]
    xth = None if ph.fock else PR.xths(ph)[0]
    out = {"tail": PR.tail_states(ph, BATCH), "edge": PR.edge_states(ph, xth)[1], "sweep": sweep_states(ph),
           "flat": flat_states(ph)}
    for v in out.values():
        v.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def plan(case, kind):
    """(states, force slot per state, noise [max(STEPS)][states][2]): seeded by the case and the kind. The slots are
    drawn from 7..13 for the inverted oscillator (its pole falls under full pushes), from 0..20 otherwise."""
    ph = BY_ID[case][1]
    states = state_sets(case)[kind]
    rng = np.random.default_rng([SEED, IDS.index(case), KINDS.index(kind)])
    lo, hi = (7, 13) if ph.family == IHO else (0, 20)
    acts = rng.integers(lo, hi + 1, size=len(states)).astype(np.int32)
    noise = rng.standard_normal((max(STEPS), len(states), 2))
    return states, acts, noise


# States left out of the 8-step call (they stay in the 1-step call). At N >= 400 the explicit measurement terms of
# the scheme amplify a rounding error on the top Fock levels from step to step (dt gamma / 4 <x^2> nears 1; the
# long runs of tests/test_gpu_parity.py blow up there after ~700 steps), by a factor that depends on the state's
# noise draw: on these states the fp64 restatement and the oracle, which differ by 1e-15 after one step, are more
# than 1e-13 apart after eight (up to 2.7e-10), so neither is a reference to 1e-12 there. Every other state stays
# within 1e-13 (tests/test_step_rows_cpu.py asserts the issue's 1e-12 on them).
ILL_CONDITIONED_AT_8 = {
    "iho401_R8": {"edge": [20], "sweep": [46, 47]},
    "iho701_R16": {"edge": [15, 16, 17, 20, 22, 26], "sweep": [22, 30, 35, 37, 40], "flat": [3]},
    "iho401_R8_f32": {"edge": [26], "flat": [4]},
    "iho701_R16_f32": {"edge": [15, 19, 21, 23, 25], "sweep": [33, 34, 42], "flat": [0]},
    "iho1500_R32_f32": {"tail": [2, 5], "edge": [18, 19, 27], "sweep": [25, 26, 28, 29, 33, 35, 36, 37, 40, 42],
                        "flat": [2, 6]},
    "ho600_R32_f32": {"edge": [17, 18, 23, 24, 26, 28], "sweep": [17]},
}


def kept(case, kind, n_steps):
    """Indices of the plan's states that the call of n_steps runs."""
    n = len(state_sets(case)[kind])
    out = ILL_CONDITIONED_AT_8.get(case, {}).get(kind, []) if n_steps > 1 else []
    return np.array([i for i in range(n) if i not in out])


def chunks(idx, B=BATCH):
    """(count, index array of exactly B states: the last chunk padded with its first state), over the states idx: a
    handle's batch is fixed."""
    idx = [int(i) for i in idx]
    out = []
    for i in range(0, len(idx), B):
        c = idx[i:i + B]
        out.append((len(c), np.array(c + c[:1] * (B - len(c)))))
    return out


# ================================================================================================
# operators by diagonal
# ================================================================================================
def _fock_diags(ph):
    """refmath.fock_ops's x and H, entry by entry the same expressions."""
    n = ph.n_max
    sqrt_n = np.array([sqrt(i) for i in range(1, n + 1)])
    xo = sqrt(1 / 2) * sqrt_n
    X = {1: xo, -1: xo.copy()}
    if ph.family == IHO:
        ho = -1 / 2 * ph.omega * (sqrt_n[1:] * sqrt_n[:-1])
        H = {2: ho, -2: ho.copy()}
    else:
        H = {0: ph.omega * (1 / 2 + np.arange(n + 1, dtype=np.float64))}
    return X, H


def _grid_diags(ph):
    g = RM.grid_ops(ph.x_max, ph.grid_size, ph.lambda_, ph.mass)
    return {0: g["x"].copy()}, {d: np.diagonal(g["H"], d).copy() for d in range(-4, 5)}


def _sparse(diags, N):
    ks = sorted(diags)
    return sp.diags([diags[k] for k in ks], ks, shape=(N, N), format="csr")


def _to_diags(M, band):
    M = M.todia()
    out = {}
    for d in range(-band, band + 1):
        v = np.asarray(M.diagonal(d))
        if np.any(v):
            out[d] = v
    return out


def _row(d, size):
    """Row index of every entry of diagonal d (its column is row + d)."""
    return np.arange(size) + max(0, -d)


class Ops:
    """X, H_F, A_eff and M of one case and force, as {offset: diagonal}, in fp64."""

    def __init__(self, ph, force):
        self.ph, self.N, self.w = ph, ph.dim, PR.weight(ph)
        self.kl = PR.KL[ph.family]
        N, dt = self.N, ph.dt
        X, H = _fock_diags(ph) if ph.fock else _grid_diags(ph)
        c = ph.omega if ph.fock else pi
        HF = _sparse(H, N) - (c * force) * _sparse(X, N)
        H2 = HF @ HF
        H3 = H2 @ HF
        H4 = H2 @ H2
        H5 = H2 @ H3
        A = dt ** 3 / 12 * H2 - 1j * dt ** 4 / 24 * H3 - dt ** 5 / 80 * H4 + 1j * dt ** 6 / 360 * H5
        if ph.a_mode == 0:          # refmath.mirror: the upper triangle and its (conjugate, IHO) mirror image
            U, L = sp.triu(A), sp.triu(A, 1).T
            A = U + (L.conj() if ph.family == IHO else L)
        M = sp.identity(N, dtype=np.complex128) + (1j * dt / 2) * HF
        self.X, self.HF = X, _to_diags(HF, self.kl)
        self.A, self.M = _to_diags(A, 5 * self.kl), _to_diags(M, self.kl)

    def dense(self):
        """(H_F, X, A_eff, M) dense, for the comparison with refmath.dense_step."""
        return tuple(_sparse(d, self.N).toarray() for d in (self.HF, self.X, self.A, self.M))


@lru_cache(maxsize=None)
def ops_of(case, action):
    ph = BY_ID[case][1]
    return Ops(ph, ph.force(int(action)))


class Work:
    """An Ops at the working precision RT (np.float64: as built; np.float32: every diagonal rounded once), with an
    optional bug applied: ("cut", b), ("drop", first) or ("shift", first)."""

    def __init__(self, ops, RT=np.float64, bug=None):
        self.ops, self.RT, self.N, self.w, self.kl = ops, RT, ops.N, ops.w, ops.kl
        self.CT = np.complex64 if RT == np.float32 else np.complex128
        X, HF, A, M = ops.X, ops.HF, ops.A, ops.M
        self.keep = self.N
        if bug is not None:
            X, HF, A, M = inject(bug, self.N, self.kl, X, HF, A, M)
            if bug[0] == "drop":
                self.keep = bug[1]
        rnd = lambda v: v.astype(self.CT if np.iscomplexobj(v) else RT)  # noqa: E731
        self.X, self.HF, self.A = ({d: rnd(v) for d, v in D.items()} for D in (X, HF, A))
        n, kl = self.keep, self.kl
        self.ab = np.zeros((2 * kl + 1, n), dtype=self.CT)      # LAPACK band storage: ab[kl + i - j, j] = M[i, j]
        for d, v in M.items():
            r = _row(d, v.size)
            self.ab[kl - d, r + d] = rnd(v)


def inject(bug, N, kl, X, HF, A, M):
    kind, at = bug
    if kind == "cut":
        return tuple(PR._cut(D, at) for D in (X, HF, A, M))
    if kind == "drop":          # the rows from `at` on are neither read nor written
        def trunc(D):
            return {d: v[:at - abs(d)] for d, v in D.items() if at - abs(d) > 0}
        return tuple(trunc(D) for D in (X, HF, A, M))
    if kind == "shift":         # the solve's rows at.. read the next row's coefficients, the last one the padding's
        rows = np.zeros((N + 1, 2 * kl + 1), dtype=np.complex128)
        rows[N, kl] = 1.0
        for d, v in M.items():
            rows[_row(d, v.size), d + kl] = v
        rows[at:N] = rows[at + 1:N + 1]
        out = {}
        for d in range(-kl, kl + 1):
            r = _row(d, N - abs(d))
            out[d] = rows[r, d + kl].copy()
        return X, HF, A, out
    raise ValueError(kind)


def mv(diags, v):
    """percontrol_ref._mv in the vector's own precision."""
    n = v.size
    out = np.zeros(n, dtype=v.dtype)
    for d, a in diags.items():
        if d >= 0:
            out[:n - d] += a * v[d:]
        else:
            out[-d:] += a * v[:n + d]
    return out


def fock_p_diags(ph, RT):
    """refmath.fock_ops's p = i sqrt(1/2) (a+ - a)."""
    po = sqrt(1 / 2) * np.array([sqrt(i) for i in range(1, ph.n_max + 1)])
    CT = np.complex64 if RT == np.float32 else np.complex128
    return {1: (-1j * po).astype(CT), -1: (1j * po).astype(CT)}


# ================================================================================================
# one step (refmath.dense_step)
# ================================================================================================
def step(W: Work, psi, gamma, dt, r):
    """(psi', q, x_mean). Vector arithmetic in W's precision; means, norm and per-step scalars in fp64, each scalar
    rounded to the working precision where it meets a vector."""
    RT, CT, w = W.RT, W.CT, W.w
    n = W.keep
    full = psi
    psi = np.ascontiguousarray(psi[:n]).astype(CT)
    S = lambda x: RT(x)  # noqa: E731
    X, HF = W.X, W.HF
    beta, sdt = sqrt(gamma / 2), sqrt(dt)
    dW = r[0] * sdt
    dZ = sdt * dt * 0.5 * (r[0] + r[1] / sqrt(3.0))

    def mean(v):
        xv = mv(X, v)
        return float(np.real(np.vdot(v.astype(np.complex128), xv.astype(np.complex128)))) * w

    xm = mean(psi)
    q = xm + dW / sqrt(2 * gamma) / dt if gamma > 0 else xm
    rel = mv(X, psi) - S(xm) * psi
    D1 = -1j * mv(HF, psi) - S(gamma / 4) * (mv(X, rel) - S(xm) * rel)
    D2 = S(beta) * rel
    Yp = psi + S(dt) * D1 + S(sdt) * D2
    Ym = psi + S(dt) * D1 - S(sdt) * D2

    def parts(Y):
        ym = mean(Y)
        rl = mv(X, Y) - S(ym) * Y
        return -1j * mv(HF, Y), -S(gamma / 4) * (mv(X, rl) - S(ym) * rl), S(beta) * rl

    Ip, Rp, D2p = parts(Yp)
    Im, Rm, D2m = parts(Ym)
    dIm = Ip - Im
    Php = Yp + S(sdt) * D2p
    Phm = Yp - S(sdt) * D2p

    def d2fresh(P):
        pm = mean(P)
        return S(beta) * (mv(X, P) - S(pm) * P)

    D2Pp, D2Pm = d2fresh(Php), d2fresh(Phm)
    rhs = (psi + D2 * S(dW) + S(0.5 / sdt * dZ) * (dIm + Rp - Rm) + S(0.25 * dt) * (Rp + S(2) * D1 + Rm)
           + S(0.25 / sdt * (dW * dW - dt)) * (D2p - D2m)
           + S(0.5 / dt * (dW * dt - dZ)) * (D2p + D2m - S(2) * D2)
           + S(0.25 / dt * (dW * dW / 3 - dt) * dW) * (D2Pp - D2Pm - D2p + D2m) - S(0.25 * sdt * dW) * dIm
           + mv(W.A, D1))
    assert rhs.dtype == CT
    new = solve_banded((W.kl, W.kl), W.ab, rhs, check_finite=False)
    assert new.dtype == CT
    nrm = sqrt(float(np.sum(new.real.astype(np.float64) ** 2 + new.imag.astype(np.float64) ** 2)))
    if nrm > 0:         # (a dropped-rows bug leaves nothing of a state that lives on those rows)
        new = new * S(1.0 / (nrm * sqrt(w)))
    if n < full.size:
        new = np.concatenate([new, np.zeros(full.size - n, dtype=CT)])
    return new, q, xm


def fock_obs(ph, psi, RT):
    """get_data_xp's five observables as the fp32 step kernel's epilogue forms them (X psi and P psi in the working
    precision, the products' sums and the combinations in fp64)."""
    CT = np.complex64 if RT == np.float32 else np.complex128
    v = psi.astype(CT)
    X, _ = _fock_diags(ph)
    xv = mv({d: a.astype(RT) for d, a in X.items()}, v).astype(np.complex128)
    pv = mv(fock_p_diags(ph, RT), v).astype(np.complex128)
    v = v.astype(np.complex128)
    x, p = np.vdot(v, xv).real, np.vdot(v, pv).real
    return np.array([x, p, np.vdot(xv, xv).real - x * x, np.vdot(pv, pv).real - p * p, np.vdot(xv, pv).real - x * p])


def run(case, states, acts, noise, n_steps, RT=np.float64, bug=None):
    """Every state stepped n_steps with its own slot and noise: (psi [S][N], q [n][S], x_mean [n][S])."""
    ph = BY_ID[case][1]
    S = len(states)
    out = np.zeros((S, ph.dim), dtype=np.complex64 if RT == np.float32 else np.complex128)
    q, xm = np.zeros((n_steps, S)), np.zeros((n_steps, S))
    work = {}
    for i in range(S):
        a = int(acts[i])
        if a not in work:
            work[a] = Work(ops_of(case, a), RT, bug)
        psi = states[i]
        for k in range(n_steps):
            psi, q[k, i], xm[k, i] = step(work[a], psi, ph.gamma, ph.dt, noise[k, i])
        out[i] = psi
    return out, q, xm


def one_step(case, state, action, nz, RT=np.float64, bug=None):
    """One step of one state, widened to complex128 (the sensitivity tests' good and bugged runs)."""
    ph = BY_ID[case][1]
    return step(Work(ops_of(case, int(action)), RT, bug), state, ph.gamma, ph.dt, nz)[0].astype(np.complex128)


def wnorm(ph, v):
    return np.linalg.norm(np.asarray(v, dtype=np.complex128), axis=-1) * sqrt(PR.weight(ph))


# ================================================================================================
# the oracle on the plan's states
# ================================================================================================
class OracleRun:
    """OracleSystem.run_batch on a plan's states widened to complex128, for 1 and for max(STEPS) steps, and (traj)
    the state after every step of the longer run."""

    def __init__(self, oracle_mod, case, kind):
        ph = BY_ID[case][1]
        self.ph, self.case = ph, case
        states, acts, noise = plan(case, kind)
        osys = PR.oracle_sys(oracle_mod, ph)
        self.psi, self.fail, self.q, self.xm = {}, {}, {}, {}
        for n in STEPS:
            ref = np.ascontiguousarray(states.astype(np.complex128))
            f, q, xm = osys.run_batch(ref, acts, ph.f_max, n, ph.dt, ph.gamma, noise=noise[:n], want_q=True,
                                      n_threads=8)
            self.psi[n], self.fail[n], self.q[n], self.xm[n] = ref, f, q, xm
        n = max(STEPS)
        self.traj = np.zeros((n + 1,) + states.shape, dtype=np.complex128)
        self.traj[0] = states
        for i in range(len(states)):
            p = np.ascontiguousarray(states[i].astype(np.complex128))
            for k in range(n):
                osys.step(p, ph.dt, ph.force(int(acts[i])), ph.gamma, noise[k, i])
                self.traj[k + 1, i] = p
        self.obs = {m: np.stack([osys.moments(p) for p in self.psi[m]]) for m in STEPS}

    def boundary_norms(self):
        """[steps][states][2]: the upper and lower boundary norms after every step (the lower one 0 for a Fock
        family, which has no lower Fail band)."""
        b = PR.BND_LEN[self.ph.family]
        t = self.traj[1:]
        top = np.linalg.norm(t[..., self.ph.dim - b:], axis=-1)
        bot = np.zeros_like(top) if self.ph.fock else np.linalg.norm(t[..., :b], axis=-1)
        return np.stack([top, bot], axis=-1)

    def x_scale(self, n):
        """[n][states]: max(1, sum |t_i|) of <x> on the state each step starts from (percontrol_ref.Sum.abs_sum): the
        scale of the x_mean and q bars where a flat or edge state makes the terms of <x> large."""
        ref = PR.ref_of(PR.BY_ID[self.case][1])
        return np.array([[max(1.0, ref.x_expectation(p).abs_sum) for p in self.traj[k]] for k in range(n)])


_ORACLE_RUNS: dict = {}


def oracle_run(oracle_mod, case, kind) -> OracleRun:
    if (case, kind) not in _ORACLE_RUNS:
        _ORACLE_RUNS[case, kind] = OracleRun(oracle_mod, case, kind)
    return _ORACLE_RUNS[case, kind]


class R32:
    """fp32 rounding alone, per case and step count: the distance of the fp32 restatement to the fp64 oracle, its
    largest value over every state of the case. psi in the weighted 2-norm, x_mean and q over every step, the five
    observables of the final state per component."""

    def __init__(self, oracle_mod, case, n):
        ph = BY_ID[case][1]
        assert ph.precision == 1
        self.by_kind = {}
        self.psi = self.xm = self.q = 0.0
        self.obs = np.zeros(5)
        for kind in KINDS:
            states, acts, noise = plan(case, kind)
            k = kept(case, kind, n)
            o = oracle_run(oracle_mod, case, kind)
            psi, q, xm = run(case, states[k], acts[k], noise[:, k], n, np.float32)
            d = wnorm(ph, psi.astype(np.complex128) - o.psi[n][k])
            self.by_kind[kind] = float(d.max())
            self.psi = max(self.psi, float(d.max()))
            self.xm = max(self.xm, float(np.abs(xm - o.xm[n][:, k]).max()))
            self.q = max(self.q, float(np.abs(q - o.q[n][:, k]).max()))
            ob = np.stack([fock_obs(ph, p, np.float32) for p in psi])
            self.obs = np.maximum(self.obs, np.abs(ob - o.obs[n][k]).max(axis=0))


_R32: dict = {}


def r32(oracle_mod, case, n) -> R32:
    if (case, n) not in _R32:
        _R32[case, n] = R32(oracle_mod, case, n)
    return _R32[case, n]


def psi_bar(oracle_mod, case, n, factor=F32_FACTOR):
    """The GPU test's bar on psi after n steps: 1e-11 at fp64, factor x r32 at fp32."""
    if BY_ID[case][1].precision == 0:
        return PSI_BAR_FP64
    return factor * r32(oracle_mod, case, n).psi
