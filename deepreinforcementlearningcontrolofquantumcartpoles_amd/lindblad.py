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
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_lindblad_evolve(self._h, vp(rho.data_ptr()), M,
                                                   vp(sp.data_ptr()) if sp is not None else None, default, n_steps))
        return rho

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
        """Raises QCartError if a slot outside [0, J) has reached `evolve` since the last call. Synchronises."""
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_lindblad_take_errors(self._h))

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
