"""MasterEquation: the open-loop evolution of density matrices on the device (qc_lindblad, include/qcart.h).

The average of the library's stochastic Schroedinger equation over the measurement record, for a force that does not
depend on it, is the master equation of continuous position measurement,

    d rho / dt = -i [H_F, rho] - (gamma / 4) [X, [X, rho]],      H_F = H - c F X.

It is the B -> infinity limit of the open-loop ensemble without sampling noise, the exact "no control" / fixed-force
curve every controller is compared against (the measurement heating of the cooling drivers, the fall-off of the
cartpoles), and the physics check of the step kernels: `EnsembleView.density_matrix` of B stepped trajectories agrees
with it within sampling error. Every step is an exact quantum channel (a unitary Cayley propagator between two
elementwise Gaussian half-steps in the eigenbasis of X), second order in dt. The scheme, the order of every sum and the
Hermitian-input assumption are documented in include/qcart.h and DESIGN §9l.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import config as cfg
from .core import make_params


def _value_error(rc: int):
    msg = L.lib().qc_lindblad_last_error(None)
    text = msg.decode() if msg else ""
    if rc == -1:
        raise ValueError(text)
    raise L.QCartError(rc, text)


class MasterEquation(L.DeviceHandle):
    """Evolves density matrices rho [N, N] (or a batch [M, N, N]) complex128 in the states' basis with EnsembleView's
    normalisation (Tr rho = 1) under fixed forces. `forces` (a sequence of floats, at most 32; None: the physics'
    n_actions discrete forces, so slot = action) get one table each at create time; `dt` defaults to
    1 / physics.time_steps and `gamma` to physics.gamma. A refused argument raises ValueError, a refusal of the library
    QCartError with its text."""

    _prefix = "qc_lindblad"
    _ensemble = None

    def __init__(self, physics: cfg.Physics, forces: Optional[Sequence[float]] = None, dt: Optional[float] = None,
                 gamma: Optional[float] = None, device: int | str | torch.device = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("libqcart needs a HIP device (no CPU fallback)")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.physics = physics
        if forces is None:
            forces = [physics.force(a) for a in range(physics.n_actions)]
        self.forces = tuple(float(f) for f in forces)
        self.dt = float(physics.dt if dt is None else dt)
        self.gamma = float(physics.gamma if gamma is None else gamma)
        self.n = int(physics.dim)
        fs = np.array(self.forces, dtype=np.float64)
        p = make_params(physics, 1)
        hd = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.init()
            rc = L.lib().qc_lindblad_create(ctypes.byref(p), self.dt, self.gamma, ctypes.c_void_p(fs.ctypes.data),
                                            len(self.forces), self.device.index, ctypes.byref(hd))
        if rc < 0:
            _value_error(rc)
        self._h = hd
        self._ops: dict = {}
        self._ensemble = None

    @property
    def ensemble(self):
        """An ensemble.EnsembleView for this physics on this device, made on first use and closed by `close`: what
        turns a batch of states into the rho this object evolves."""
        if self._ensemble is None:
            from .ensemble import EnsembleView
            self._ensemble = EnsembleView.for_physics(self.physics, self.device)
        return self._ensemble

    def close(self):
        if self._ensemble is not None:
            self._ensemble.close()
            self._ensemble = None
        super().close()

    # ------------------------------------------------------------------ the host tables
    @staticmethod
    def tables(physics: cfg.Physics, force: float, dt: Optional[float] = None, gamma: Optional[float] = None) -> dict:
        """The tables of one force as numpy arrays: xi [N], W [N, N] (the grid's: the identity), T [N, N] complex128,
        g_half and g_full [N, N]. Host only: no GPU is touched. A refusal is a ValueError with the library's text."""
        n = max(int(physics.dim), 1)
        out = dict(xi=np.zeros(n), W=np.zeros((n, n)), T=np.zeros((n, n), dtype=np.complex128),
                   g_half=np.zeros((n, n)), g_full=np.zeros((n, n)))
        p = make_params(physics, 1)
        vp = ctypes.c_void_p
        rc = L.lib().qc_lindblad_tables(ctypes.byref(p), float(physics.dt if dt is None else dt),
                                        float(physics.gamma if gamma is None else gamma), float(force),
                                        vp(out["xi"].ctypes.data), vp(out["W"].ctypes.data), vp(out["T"].ctypes.data),
                                        vp(out["g_half"].ctypes.data), vp(out["g_full"].ctypes.data))
        if rc < 0:
            _value_error(rc)
        return out

    # ------------------------------------------------------------------ arguments
    def _matrices(self, rho, what: str = "rho") -> torch.Tensor:
        if not isinstance(rho, torch.Tensor):
            raise ValueError(f"{what} must be a torch tensor")
        if rho.dtype != torch.complex128:
            raise ValueError(f"{what} must be complex128, not {rho.dtype}")
        if rho.device != self.device:
            raise ValueError(f"{what} must live on {self.device}, not {rho.device}")
        if rho.dim() not in (2, 3) or tuple(rho.shape[-2:]) != (self.n, self.n) or rho.shape[0] < 1:
            raise ValueError(f"{what} must be [{self.n}, {self.n}] or [M, {self.n}, {self.n}]")
        if not rho.is_contiguous():
            raise ValueError(f"{what} must be contiguous (the call works in place: a copy would be evolved instead)")
        return rho

    @property
    def zero_force_slot(self) -> Optional[int]:
        """The slot whose force is 0.0, or None."""
        return self.forces.index(0.0) if 0.0 in self.forces else None

    # ------------------------------------------------------------------ the evolution
    def evolve(self, rho: torch.Tensor, n_steps: int, slots=None) -> torch.Tensor:
        """rho after n_steps steps of length dt, in place (returns rho). slots: an int (one slot for all), a device
        int32 [M] tensor (one per matrix), or None: the F = 0 slot (ValueError if the forces do not contain 0.0). A
        slot outside [0, J) in a tensor leaves that rho untouched and is reported by `take_errors`. Asynchronous."""
        rho = self._matrices(rho)
        M = 1 if rho.dim() == 2 else int(rho.shape[0])
        if isinstance(n_steps, bool) or not isinstance(n_steps, int) or n_steps < 0:
            raise ValueError("n_steps must be an int >= 0")
        sp, default = self._slots(slots, M)
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_lindblad_evolve(self._h, vp(rho.data_ptr()), M,
                                                   vp(sp.data_ptr()) if sp is not None else None, default, n_steps))
        return rho

    def _slots(self, slots, M: int):
        """(the device int32 [M] tensor or None, the slot for all) of `evolve`'s slots argument."""
        sp, default = None, 0
        if slots is None:
            if self.zero_force_slot is None:
                raise ValueError("slots is required: the forces do not contain 0.0")
            default = self.zero_force_slot
        elif isinstance(slots, torch.Tensor):
            if slots.dtype != torch.int32 or tuple(slots.shape) != (M,):
                raise ValueError(f"slots must be an int or an int32 [{M}] tensor")
            if slots.device != self.device:
                raise ValueError(f"slots must live on {self.device}, not {slots.device}")
            sp = slots.contiguous()
        elif isinstance(slots, int) and not isinstance(slots, bool):
            if not 0 <= slots < len(self.forces):
                raise ValueError(f"slot {slots} is outside [0, {len(self.forces)})")
            default = slots
        else:
            raise ValueError(f"slots must be an int or an int32 [{M}] tensor")
        return sp, default

    def congruence(self, A: torch.Tensor, x: torch.Tensor, g: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """y = g o (A x A^†) for every matrix of x ([N, N] or [M, N, N]); A complex128 [N, N], g float64 [N, N]
        (symmetric) or None. x is assumed Hermitian; y is the exactly Hermitian matrix whose lower triangle is that of
        the product. out: the result's tensor (may be x itself); None: a new one. Asynchronous."""
        x = self._matrices(x, "x")
        A = self._matrices(A, "A")
        if A.dim() != 2:
            raise ValueError(f"A must be [{self.n}, {self.n}]")
        if g is not None:
            if not isinstance(g, torch.Tensor) or g.dtype != torch.float64 or tuple(g.shape) != (self.n, self.n):
                raise ValueError(f"g must be a float64 [{self.n}, {self.n}] tensor")
            if g.device != self.device:
                raise ValueError(f"g must live on {self.device}, not {g.device}")
            if not g.is_contiguous():
                raise ValueError("g must be contiguous")
        if out is None:
            out = torch.empty_like(x)
        else:
            out = self._matrices(out, "out")
            if out.shape != x.shape:
                raise ValueError("out must have x's shape")
        M = 1 if x.dim() == 2 else int(x.shape[0])
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_lindblad_congruence(self._h, vp(A.data_ptr()),
                                                       vp(g.data_ptr()) if g is not None else None,
                                                       vp(x.data_ptr()), vp(out.data_ptr()), M))
        return out

    def take_errors(self) -> None:
        """Raises QCartError if a slot outside [0, J) has reached `evolve` or `evolve_conditional`, or a rho that
        `evolve_conditional` could not step, since the last call. Synchronises."""
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_lindblad_take_errors(self._h))

    # ------------------------------------------------------------------ the conditional evolution
    def set_efficiency(self, eta: float) -> None:
        """The detection efficiency eta in (0, 1] of `evolve_conditional`: builds the table G^(1 - eta) on the host and
        uploads it (may synchronise). A refused eta (or a handle whose gamma is 0) raises ValueError."""
        with torch.cuda.device(self.device):
            self._bind_stream()
            rc = L.lib().qc_lindblad_set_efficiency(self._h, float(eta))
        if rc == -1:
            raise ValueError(L.lib().qc_lindblad_last_error(self._h).decode())
        self._check(rc)

    @property
    def eta(self) -> Optional[float]:
        """The detection efficiency, None while unset."""
        e = ctypes.c_double(-1.0)
        self._check(L.lib().qc_lindblad_efficiency(self._h, ctypes.byref(e)))
        return None if e.value < 0 else e.value

    @property
    def xi(self) -> torch.Tensor:
        """X's eigenvalues, float64 [N] on the device: the measurement basis of `evolve` and `evolve_conditional`
        (ascending for the Fock families, the grid points otherwise): a copy of the handle's own, made once.
        Asynchronous."""
        if "xi" not in self._ops:
            xi = torch.empty(self.n, dtype=torch.float64, device=self.device)
            with torch.cuda.device(self.device):
                self._bind_stream()
                self._check(L.lib().qc_lindblad_xi(self._h, ctypes.c_void_p(xi.data_ptr())))
            self._ops["xi"] = xi
        return self._ops["xi"]

    def _per_step(self, t, what: str, n_steps: int, M: int, last: tuple = ()) -> torch.Tensor:
        shape = (n_steps, M) + last
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != shape:
            raise ValueError(f"{what} must be a float64 {list(shape)} tensor")
        if t.device != self.device:
            raise ValueError(f"{what} must live on {self.device}, not {t.device}")
        if not t.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
        return t

    def evolve_conditional(self, rho: torch.Tensor, n_steps: int, slots=None, *, seed: int = 0, streams=None,
                           first_step: int = 0, draws=None, record=None, want_record: bool = False):
        """rho after n_steps steps of the conditional master equation at the efficiency of `set_efficiency`, in place:
        rho along one measurement record per matrix (include/qcart.h). The record is sampled from Philox
        keyed by `seed` at (first_step + n, streams[m]) (streams: a device int32 [M] tensor, None: m), or from
        `draws` (float64 [n_steps, M, 2]: u in (0, 1) and a standard normal z), or it is given: `record` (float64
        [n_steps, M], the outcomes y) makes the call a filter and nothing is drawn; `record` with `draws` is refused.
        slots as `evolve`'s. Returns rho, or with want_record = True (rho, y [n_steps, M]). A rho that cannot be
        stepped (a slot out of range, a diagonal that is not finite, a record that contradicts it) is left untouched,
        its y are NaN from that step on, and `take_errors` reports it. Asynchronous."""
        rho = self._matrices(rho)
        M = 1 if rho.dim() == 2 else int(rho.shape[0])
        if isinstance(n_steps, bool) or not isinstance(n_steps, int) or n_steps < 0:
            raise ValueError("n_steps must be an int >= 0")
        if isinstance(first_step, bool) or not isinstance(first_step, int) or first_step < 0:
            raise ValueError("first_step must be an int >= 0")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
            raise ValueError("seed must be an int in [0, 2^64)")
        if self.eta is None:
            raise ValueError("the efficiency is not set (set_efficiency first)")
        if draws is not None and record is not None:
            raise ValueError("record and draws exclude each other")
        sp, default = self._slots(slots, M)
        if streams is not None:
            if not isinstance(streams, torch.Tensor) or streams.dtype != torch.int32 or tuple(streams.shape) != (M,):
                raise ValueError(f"streams must be an int32 [{M}] tensor")
            if streams.device != self.device:
                raise ValueError(f"streams must live on {self.device}, not {streams.device}")
            streams = streams.contiguous()
        if draws is not None:
            draws = self._per_step(draws, "draws", n_steps, M, (2,))
        if record is not None:
            record = self._per_step(record, "record", n_steps, M)
        y = torch.empty((n_steps, M), dtype=torch.float64, device=self.device) if want_record else None
        vp = ctypes.c_void_p
        ptr = lambda t: vp(t.data_ptr()) if t is not None else None   # noqa: E731
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_lindblad_evolve_conditional(self._h, vp(rho.data_ptr()), M, ptr(sp), default,
                                                               n_steps, seed, ptr(streams), first_step, ptr(draws),
                                                               ptr(record), ptr(y)))
        return (rho, y) if want_record else rho

    def controller_operator(self, name: str) -> torch.Tensor:
        """`controller_operator` (this module) of the handle's physics on its device, made once per name."""
        key = "c:" + name
        if key not in self._ops:
            self._ops[key] = torch.from_numpy(controller_operator(self.physics, name)).to(self.device)
        return self._ops[key]

    @staticmethod
    def expectations(rho: torch.Tensor, op: torch.Tensor) -> torch.Tensor:
        """Re Tr(rho_m op) of every matrix of a batch [M, N, N] (EnsembleView.expectation's quantity per matrix): a
        float64 [M] tensor."""
        return (rho * op.to(rho.dtype).transpose(0, 1)).sum(dim=(-2, -1)).real

    def analytic_slots(self, rho: torch.Tensor, strategy: str = "LQG", con_parameter: float = 0.0) -> torch.Tensor:
        """The slots (= actions) of the drivers' analytic baseline controllers on a batch of rho, int32 [M]: the
        formulas of IHO/main_parallel.py:194-206 (Fock 'LQG') and QO/controllers.py:7-29 with QO/main_parallel.py:165-181
        (grid 'LQG', 'damping', 'semiclassical'), with Tr(rho O) in the place of <psi|O|psi>, evaluated in float64 torch
        on the device (`baseline_slots`). It is NOT a reproduction of the Fock branch's float32 network input (the
        reference, and `BatchedEnv.analytic_actions`, round x and p to float32 first): the two agree wherever the force
        is not within float32 rounding of a tie between two actions. Valid only for a handle whose forces are the
        physics' own action grid (slot = action); refused otherwise. Asynchronous."""
        ph = self.physics
        if self.forces != tuple(float(ph.force(a)) for a in range(ph.n_actions)):
            raise ValueError("analytic_slots needs the physics' own action grid as the handle's forces (slot = action)")
        rho = self._matrices(rho)
        if rho.dim() == 2:
            rho = rho[None]
        return baseline_slots(ph, lambda k: self.expectations(rho, self.controller_operator(k)), strategy,
                              con_parameter)

    # ------------------------------------------------------------------ operators and what rho gives
    def operator(self, name: str) -> torch.Tensor:
        """A dense [N, N] complex128 operator in the states' basis, for EnsembleView.expectation(rho, op): 'x', 'x2'
        (the square of the truncated X), 'h' (the force-free Hamiltonian; for the grid Tr(rho h) is Stepper.energy's
        quantity) and, for the Fock families, 'n' (the phonon number)."""
        if name in self._ops:
            return self._ops[name]
        ph, n = self.physics, self.n
        if name not in ("x", "x2", "h") + (("n",) if ph.fock else ()):
            raise ValueError(f"no operator {name!r} (x, x2, h" + (", n" if ph.fock else "") + ")")
        if ph.fock:
            up = np.array([math.sqrt(float(i + 1)) * math.sqrt(0.5) for i in range(n - 1)])
            X = np.diag(up, 1) + np.diag(up, -1)
            if ph.family == cfg.HO:
                H = np.diag(np.array([ph.omega * (0.5 + float(i)) for i in range(n)]))
            else:
                v = np.array([(-0.5 * ph.omega) * (math.sqrt(float(i + 1)) * math.sqrt(float(i + 2)))
                              for i in range(n - 2)])
                H = np.diag(v, 2) + np.diag(v, -2)
        else:
            h, half = ph.grid_size, (n - 1) // 2
            x = h * (np.arange(n) - half).astype(np.float64)
            X = np.diag(x)
            H = np.diag((1. / (2. * ph.mass)) * (14350. / 5040. / (h * h)) + (x * x) * (x * x) * ph.lambda_)
            for d, num in ((1, 8064.), (2, -1008.), (3, 128.), (4, -9.)):
                v = np.full(n - d, (1. / (2. * ph.mass)) * (-(num / 5040. / (h * h))))
                H = H + np.diag(v, d) + np.diag(v, -d)
        m = {"x": X, "x2": X @ X, "h": H, "n": np.diag(np.arange(n, dtype=np.float64))}[name]
        self._ops[name] = torch.from_numpy(m.astype(np.complex128)).to(self.device)
        return self._ops[name]

    def boundary_weight(self, rho: torch.Tensor) -> torch.Tensor:
        """The population of the entries the families' Fail test watches (the last 5 Fock levels; the first and the
        last 6 grid points): a real 0-d tensor, or [M] for a batch."""
        d = torch.diagonal(self._matrices(rho), dim1=-2, dim2=-1).real
        if self.physics.fock:
            return d[..., -5:].sum(dim=-1)
        return d[..., :6].sum(dim=-1) + d[..., -6:].sum(dim=-1)


def controller_operator(ph: cfg.Physics, name: str) -> np.ndarray:
    """The dense [N, N] complex128 operators the drivers' baseline controllers take expectation values of, in the
    states' basis: 'x', 'x2', 'p', 'p2', 'xp' (= x p + p x), 'x3', 'xpx' (= x p x), built from the truncated X and P
    (Fock: x = sqrt(1/2) (a^† + a), p = i sqrt(1/2) (a^† - a); grid: x the points, p = -i D1, the 8th-order
    first-difference stencil over the grid spacing)."""
    if name not in ("x", "x2", "p", "p2", "xp", "x3", "xpx"):
        raise ValueError(f"no controller operator {name!r} (x, x2, p, p2, xp, x3, xpx)")
    n = int(ph.dim)
    if ph.fock:
        up = np.array([math.sqrt(float(i + 1)) * math.sqrt(0.5) for i in range(n - 1)])
        X = np.diag(up, 1) + np.diag(up, -1)
        Pm = 1.0j * (np.diag(up, -1) - np.diag(up, 1))
    else:
        X = np.diag(ph.grid_size * (np.arange(n) - (n - 1) // 2).astype(np.float64))
        d = np.zeros((n, n))
        for k, c in ((1, 672 / 840), (2, -168 / 840), (3, 32 / 840), (4, -3 / 840)):
            d += np.diag(np.full(n - k, c), k) - np.diag(np.full(n - k, c), -k)
        Pm = -1.0j * (d / ph.grid_size)
    m = {"x": lambda: X, "x2": lambda: X @ X, "p": lambda: Pm, "p2": lambda: Pm @ Pm,
         "xp": lambda: X @ Pm + Pm @ X, "x3": lambda: X @ X @ X, "xpx": lambda: X @ Pm @ X}[name]()
    return np.ascontiguousarray(m).astype(np.complex128)


def baseline_force(ph: cfg.Physics, ex, strategy: str = "LQG", con_parameter: float = 0.0) -> torch.Tensor:
    """float64 [M]: the analytic baseline controllers' force before it is clipped and rounded, F / omega (Fock) or
    F / pi (grid), from ex(name) -> float64 [M] expectation values of `controller_operator`'s operators (torch tensors
    on any device)."""
    T = 1. / ph.n_con
    if ph.fock:
        if strategy != "LQG":
            raise ValueError(f"the Fock families take only 'LQG', not {strategy!r}")
        w = ph.omega
        x, p = ex("x"), ex("p")
        if ph.family == cfg.IHO:
            F = -(x + p) * (1 + w * T + 0.5 * w * w * T * T) / (T + w * T * T / 2)
        else:
            F = -((x + p) + (p - x) * w * T) / T
        F = F / w
    else:
        lam, mass = ph.lambda_, ph.mass
        if strategy == "damping":
            pp = ex("p") - 4. * lam * ex("x3") * T - T ** 2 * 2. * lam * 3. * ex("xpx") / mass
            F = -pp / T * float(con_parameter)
        elif strategy == "LQG":
            k = lam * float(con_parameter)
            x3 = ex("x3")
            xq = ex("x") + ex("p") / mass * T - T ** 2 * 2. * lam * x3 / mass
            pq = ex("p") - 4. * lam * x3 * T - T ** 2 * 2. * lam * 3. * ex("xpx") / mass
            F = -(math.sqrt(k * mass) * xq + pq) / T
        elif strategy == "semiclassical":
            x = ex("x")
            var = ex("x2") - x ** 2
            F = (-torch.sqrt(2 * mass * (6 * lam * var + lam * x ** 2)) * x - ex("p")) / T
        else:
            raise ValueError(f"no strategy {strategy!r} (LQG, damping, semiclassical)")
        F = F / math.pi
    return F


def baseline_slots(ph: cfg.Physics, ex, strategy: str = "LQG", con_parameter: float = 0.0) -> torch.Tensor:
    """int32 [M] actions of the analytic baseline controllers: `baseline_force` clipped to +-f_max and rounded
    half-to-even to the action grid, as the drivers do."""
    F = baseline_force(ph, ex, strategy, con_parameter)
    half = ph.n_actions // 2
    unit = ph.f_max / half
    return (torch.round(torch.clamp(F, -ph.f_max, ph.f_max) / unit) + half).to(torch.int32)
