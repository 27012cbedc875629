"""WignerView: the phase-space view of a batch of states on the device (qc_wigner, include/qcart.h).

The Wigner function W(x, p) = (1 / pi) int conj(phi(x + y)) phi(x - y) e^{2 i p y} dy (hbar = 1) of every env's
wavefunction on a uniform grid x and momenta p, and its ensemble mean over the (masked) envs in one fused pass that
never writes a per-env W. Everything the controllers act on lives here: <x>, <p> and the covariances of the 'xp' input,
the LQG law on x + p, the Gaussian baselines of the quartic drivers; negativity, squeezing and the momentum marginal
show where a state stops being Gaussian, which a position density cannot. A packet e^{+i p0 x} sits at p = +p0;
sum_j W dp is the position density and sum_i W h the momentum density when p covers one period of the grid. The
definition, the table and the mean's order are documented in include/qcart.h and DESIGN §9i.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import config as cfg
from .spatial import SpatialView, driver_grid


def default_momenta() -> np.ndarray:
    return np.linspace(-12, 12, 193)


class WignerView(L.DeviceHandle):
    """The Wigner function of states on the uniform points `x` (None: the drivers' grid) at the momenta `p` (None:
    np.linspace(-12, 12, 193)). n_levels = 0: the states are wavefunctions on `x`, complex128 [B, x_n] (or one
    [x_n]), continuum-normalised (sum h |phi|^2 = 1). n_levels > 0: the states are Fock states [B, n_state <= n_levels]
    and the view owns a SpatialView(n_levels, x) whose `repr` writes phi once before the Wigner kernels read it. One
    point has no spacing: h = 1. A refused argument raises ValueError, a refusal of the library QCartError with its
    text."""

    _prefix = "qc_wigner"

    def __init__(self, x=None, p=None, n_levels: int = 0, device: int | str | torch.device = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("libqcart needs a HIP device (no CPU fallback)")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        xs, h = self.uniform_grid(driver_grid() if x is None else x)
        ps = np.ascontiguousarray(default_momenta() if p is None else
                                  (p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else p), dtype=np.float64)
        if ps.ndim != 1:
            raise ValueError("p must be one-dimensional")
        self.n_levels, self.x_n, self.p_n, self.h = int(n_levels), int(xs.size), int(ps.size), h
        if self.n_levels < 0:
            raise ValueError("n_levels must be >= 0")
        hd = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.init()
            L.check_wigner(L.lib().qc_wigner_create(self.x_n, h, ctypes.c_void_p(ps.ctypes.data), self.p_n,
                                                    self.device.index, ctypes.byref(hd)))
        self._h = hd
        self._ps = ps
        self._dp = None                              # the spacing of uniform momenta, found by negative_volume
        self.spatial = None
        try:
            if self.n_levels > 0:
                self.spatial = SpatialView(self.n_levels, xs, self.device)
        except Exception:
            self.close()                             # the Wigner handle is not left to the finaliser
            raise
        self.x = torch.from_numpy(xs).to(self.device)
        self.p = torch.from_numpy(ps).to(self.device)

    @staticmethod
    def uniform_grid(x):
        """(x as a float64 array, its spacing h = (x[-1] - x[0]) / (x_n - 1)); ValueError unless every
        |x_j - (x_0 + j h)| <= 1e-12 max(1, max |x|) and h > 0."""
        xs = np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)
        if xs.ndim != 1 or xs.size < 1:
            raise ValueError("x must be one-dimensional with at least one point")
        if not np.all(np.isfinite(xs)):
            raise ValueError("x must be finite")
        if xs.size == 1:
            return xs, 1.0
        h = float((xs[-1] - xs[0]) / (xs.size - 1))
        off = np.abs(xs - (xs[0] + np.arange(xs.size) * h)).max()
        if not h > 0. or off > 1e-12 * max(1., float(np.abs(xs).max())):
            raise ValueError(f"x must be a uniform ascending grid: it departs from x[0] + j h by {off:.3e}")
        return xs, h

    @classmethod
    def for_physics(cls, physics: cfg.Physics, p=None, device: int | str | torch.device = 0) -> "WignerView":
        """The view of `physics`' states: HO / IHO Fock states of its n_max + 1 levels on the drivers' grid; QO / IQO
        the wavefunctions on the simulation's own points."""
        if physics.fock:
            return cls(None, p, physics.n_max + 1, device)
        half = (physics.dim - 1) // 2
        return cls((np.arange(physics.dim) - half) * physics.grid_size, p, 0, device)

    def close(self):
        if self.spatial is not None:
            self.spatial.close()
            self.spatial = None
        super().close()

    # ------------------------------------------------------------------ arguments
    def _wavefunctions(self, psi: torch.Tensor):
        """phi [B, x_n] complex128 contiguous of the states (Fock states through the owned SpatialView), and whether
        one state was given."""
        if self.spatial is not None:
            one = isinstance(psi, torch.Tensor) and psi.dim() == 1
            phi = self.spatial.repr(psi)             # (its refusals: dtype, device, shape, n_state)
            return (phi[None] if one else phi), one
        if not isinstance(psi, torch.Tensor):
            raise ValueError("psi must be a torch tensor")
        if psi.dtype != torch.complex128:
            raise ValueError(f"psi must be complex128, not {psi.dtype} (the fp32 handles' complex64 states are not "
                             "viewed)")
        if psi.device != self.device:
            raise ValueError(f"psi must live on {self.device}, not {psi.device}")
        one = psi.dim() == 1
        if one:
            psi = psi[None]
        if psi.dim() != 2 or psi.shape[0] < 1:
            raise ValueError("psi must be [B, x_n] (or one [x_n] wavefunction)")
        if int(psi.shape[1]) != self.x_n:
            raise ValueError(f"a grid view takes states of {self.x_n} points, not {int(psi.shape[1])}")
        return psi.contiguous(), one

    # ------------------------------------------------------------------ transforms
    def wigner(self, psi: torch.Tensor) -> torch.Tensor:
        """W [B, X, P] float64 (one state: [X, P]). W[b] does not depend on the batch. Asynchronous."""
        phi, one = self._wavefunctions(psi)
        B = int(phi.shape[0])
        out = torch.empty(B, self.x_n, self.p_n, dtype=torch.float64, device=self.device)
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_wigner_eval(self._h, vp(phi.data_ptr()), B, vp(out.data_ptr())))
        return out[0] if one else out

    def wigner_of(self, rho: torch.Tensor) -> torch.Tensor:
        """W [M, X, P] float64 (one matrix: [X, P]) of density matrices. A grid view takes rho [M, x_n, x_n] complex128
        with EnsembleView's / MasterEquation's grid normalisation (sum_i rho_ii = 1: a pure state is h phi phi^†); a
        view with n_levels > 0 takes Fock-basis rho [M, n, n], n <= n_levels, and brings it to the grid through its
        SpatialView's `density_matrix_of` first. rho is assumed Hermitian: only its lower triangle is read and the
        imaginary part of the diagonal is ignored (include/qcart.h). W[m] does not depend on the batch.
        Asynchronous."""
        if self.spatial is not None:
            one = isinstance(rho, torch.Tensor) and rho.dim() == 2
            sigma = self.spatial.density_matrix_of(rho)      # (its refusals: dtype, device, shape, n)
            sigma = sigma[None] if one else sigma
        else:
            if not isinstance(rho, torch.Tensor):
                raise ValueError("rho must be a torch tensor")
            if rho.dtype != torch.complex128:
                raise ValueError(f"rho must be complex128, not {rho.dtype}")
            if rho.device != self.device:
                raise ValueError(f"rho must live on {self.device}, not {rho.device}")
            one = rho.dim() == 2
            sigma = rho[None] if one else rho
            if sigma.dim() != 3 or sigma.shape[0] < 1 or sigma.shape[1] != sigma.shape[2]:
                raise ValueError("rho must be [M, x_n, x_n] (or one [x_n, x_n] density matrix)")
            if int(sigma.shape[1]) != self.x_n:
                raise ValueError(f"a grid view takes density matrices of {self.x_n} points, not {int(sigma.shape[1])}")
            if int(sigma.shape[0]) * self.x_n * self.x_n > 1 << 27:
                raise ValueError(f"M x_n^2 must be <= 2^27 (M = {int(sigma.shape[0])}, x_n = {self.x_n})")
            sigma = sigma.contiguous()
        M = int(sigma.shape[0])
        out = torch.empty(M, self.x_n, self.p_n, dtype=torch.float64, device=self.device)
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_wigner_eval_rho(self._h, vp(sigma.data_ptr()), M, vp(out.data_ptr())))
        return out[0] if one else out

    def negative_volume(self, W: torch.Tensor) -> torch.Tensor:
        """sum max(-W, 0) h dp over the last two dimensions of W [..., X, P]: the negative volume of a Wigner function,
        zero for a Gaussian state. dp is the spacing of `p`, which must be uniform by `uniform_grid`'s criterion (one
        momentum: dp = 1); ValueError otherwise. Pure torch, nothing is waited on."""
        if self._dp is None:
            try:
                self._dp = self.uniform_grid(self._ps)[1]
            except ValueError as e:
                raise ValueError(f"negative_volume needs uniform momenta: p as {e}") from None
        if not isinstance(W, torch.Tensor) or W.dim() < 2 or tuple(W.shape[-2:]) != (self.x_n, self.p_n):
            raise ValueError(f"W must be [..., {self.x_n}, {self.p_n}]")
        return torch.clamp(-W, min=0.).sum(dim=(-2, -1)) * (self.h * self._dp)

    def mean_wigner(self, psi: torch.Tensor, mask: Optional[torch.Tensor] = None):
        """(mean [X, P] float64, count int64 scalar tensor): the mean of `wigner` over the envs whose mask is set (bool
        or uint8 [B]; None: all), summed in the fixed order include/qcart.h documents; count = 0 gives zeros. No
        per-env W is written. Asynchronous: both results are device tensors."""
        phi, _ = self._wavefunctions(psi)
        B = int(phi.shape[0])
        m8 = None
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) \
                    or tuple(mask.shape) != (B,):
                raise ValueError(f"mask must be a bool or uint8 [{B}] tensor")
            if mask.device != self.device:
                raise ValueError(f"mask must live on {self.device}, not {mask.device}")
            m8 = mask.contiguous()
            m8 = m8.view(torch.uint8) if m8.dtype == torch.bool else m8
        out = torch.empty(self.x_n, self.p_n, dtype=torch.float64, device=self.device)
        count = torch.empty((), dtype=torch.int64, device=self.device)
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_wigner_mean(self._h, vp(phi.data_ptr()), B,
                                               vp(m8.data_ptr()) if m8 is not None else None,
                                               vp(out.data_ptr()), vp(count.data_ptr())))
        return out, count
