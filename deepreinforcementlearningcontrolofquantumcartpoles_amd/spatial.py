"""SpatialView: the drivers' spatial_repr and probability on the device (qc_spatial, include/qcart.h).

HO/main_parallel.py:47-51, 82-86: the position-space wavefunction of a Fock-basis state on x = np.linspace(-14, 14,
250), phi = eigen_states[:, :state.size] @ state, and its density |phi|^2 (for QO / IQO, whose state already lives on
a grid, |psi|^2 itself): what the drivers' plot module draws. Here for a whole batch next to psi: `repr`,
`probability`, and `mean_probability`, the ensemble density of the (masked) envs in one fused pass that never writes
phi. The table and the sum's order are documented in include/qcart.h and DESIGN §9h.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import config as cfg


def driver_grid() -> np.ndarray:
    """The drivers' x (HO/main_parallel.py:34-35)."""
    return np.linspace(-14, 14, 250)


class SpatialView(L.DeviceHandle):
    """The position-space view of states with up to `n_levels` Fock levels on the points `x` (None: the drivers'
    grid). n_levels = 0 is a grid view: the states are wavefunctions on `x` already, `probability` is |psi|^2 and
    `repr` is refused. States are complex128 [B, n_state] tensors (or one [n_state] state) on the view's device; a
    refused argument raises ValueError, a refusal of the library QCartError with its text."""

    _prefix = "qc_spatial"

    def __init__(self, n_levels: int, x=None, device: int | str | torch.device = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("libqcart needs a HIP device (no CPU fallback)")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        xs = np.ascontiguousarray(driver_grid() if x is None else
                                  (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x), dtype=np.float64)
        if xs.ndim != 1:
            raise ValueError("x must be one-dimensional")
        self.n_levels, self.x_n = int(n_levels), int(xs.size)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.init()
            L.check_spatial(L.lib().qc_spatial_create(self.n_levels, ctypes.c_void_p(xs.ctypes.data), self.x_n,
                                                      self.device.index, ctypes.byref(h)))
        self._h = h
        self._xs = xs
        self._spacing = None                         # of a uniform x, found on the first density_matrix_of
        self.x = torch.from_numpy(xs).to(self.device)

    @classmethod
    def for_physics(cls, physics: cfg.Physics, x=None, device: int | str | torch.device = 0) -> "SpatialView":
        """The view of `physics`' states: HO / IHO the table of its n_max + 1 levels on `x` (None: the drivers'
        grid); QO / IQO a grid view on the simulation's own points (x: None, or those points' coordinates)."""
        if physics.fock:
            return cls(physics.n_max + 1, x, device)
        if x is None:
            half = (physics.dim - 1) // 2
            x = (np.arange(physics.dim) - half) * physics.grid_size
        return cls(0, x, device)

    @property
    def grid(self) -> bool:
        return self.n_levels == 0

    # ------------------------------------------------------------------ arguments
    def _states(self, psi: torch.Tensor):
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
            raise ValueError("psi must be [B, n_state] (or one [n_state] state)")
        n = int(psi.shape[1])
        if self.grid and n != self.x_n:
            raise ValueError(f"a grid view takes states of {self.x_n} points, not {n}")
        if not self.grid and not 1 <= n <= self.n_levels:
            raise ValueError(f"n_state must be in [1, {self.n_levels}], not {n}")
        return psi.contiguous(), one

    @staticmethod
    def _threshold(threshold: float) -> float:
        t = float(threshold)
        if not t >= 0.:
            raise ValueError("threshold must be >= 0")
        return t

    # ------------------------------------------------------------------ transforms
    def repr(self, psi: torch.Tensor, threshold: float = 0.) -> torch.Tensor:
        """phi [B, X] complex128: spatial_repr of every state; levels with |c| <= threshold are left out (the
        drivers' display mask is 1e-4). Asynchronous."""
        if self.grid:
            raise ValueError("SpatialView.repr: a grid view's state is its own representation")
        psi, one = self._states(psi)
        t = self._threshold(threshold)
        out = torch.empty(psi.shape[0], self.x_n, dtype=torch.complex128, device=self.device)
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_spatial_repr(self._h, vp(psi.data_ptr()), psi.shape[0], psi.shape[1], t,
                                                vp(out.data_ptr())))
        return out[0] if one else out

    def probability(self, psi: torch.Tensor, threshold: float = 0.) -> torch.Tensor:
        """p [B, X] float64: Re(phi)^2 + Im(phi)^2 of `repr` (a grid view: of psi itself), each operation rounded
        once; phi is not written. Asynchronous."""
        psi, one = self._states(psi)
        t = self._threshold(threshold)
        out = torch.empty(psi.shape[0], self.x_n, dtype=torch.float64, device=self.device)
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_spatial_probability(self._h, vp(psi.data_ptr()), psi.shape[0], psi.shape[1], t,
                                                       vp(out.data_ptr())))
        return out[0] if one else out

    def mean_probability(self, psi: torch.Tensor, mask: Optional[torch.Tensor] = None, threshold: float = 0.):
        """(mean [X] float64, count int64 scalar tensor): the mean of `probability` over the envs whose mask is set
        (bool or uint8 [B]; None: all), summed in the fixed order include/qcart.h documents; count = 0 gives zeros.
        Neither phi nor p is written. Asynchronous: both results are device tensors."""
        psi, _ = self._states(psi)
        t = self._threshold(threshold)
        B = int(psi.shape[0])
        m8 = None
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) \
                    or tuple(mask.shape) != (B,):
                raise ValueError(f"mask must be a bool or uint8 [{B}] tensor")
            if mask.device != self.device:
                raise ValueError(f"mask must live on {self.device}, not {mask.device}")
            m8 = mask.contiguous()
            m8 = m8.view(torch.uint8) if m8.dtype == torch.bool else m8
        out = torch.empty(self.x_n, dtype=torch.float64, device=self.device)
        count = torch.empty((), dtype=torch.int64, device=self.device)
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_spatial_mean(self._h, vp(psi.data_ptr()), B, psi.shape[1],
                                                vp(m8.data_ptr()) if m8 is not None else None, t,
                                                vp(out.data_ptr()), vp(count.data_ptr())))
        return out, count

    def _density_matrices(self, rho):
        """rho [M, n, n] complex128 contiguous, and whether one matrix was given."""
        if not isinstance(rho, torch.Tensor):
            raise ValueError("rho must be a torch tensor")
        if rho.dtype != torch.complex128:
            raise ValueError(f"rho must be complex128, not {rho.dtype}")
        if rho.device != self.device:
            raise ValueError(f"rho must live on {self.device}, not {rho.device}")
        one = rho.dim() == 2
        if one:
            rho = rho[None]
        if rho.dim() != 3 or rho.shape[0] < 1 or rho.shape[1] != rho.shape[2]:
            raise ValueError("rho must be [M, n, n] (or one [n, n] density matrix)")
        n = int(rho.shape[1])
        if not 1 <= n <= self.n_levels:
            raise ValueError(f"n_state must be in [1, {self.n_levels}], not {n}")
        if int(rho.shape[0]) * self.x_n * self.x_n > 1 << 27:
            raise ValueError(f"M x_n^2 must be <= 2^27 (M = {int(rho.shape[0])}, x_n = {self.x_n})")
        return rho.contiguous(), one

    def density_matrix_of(self, rho: torch.Tensor) -> torch.Tensor:
        """sigma [M, X, X] complex128 (one matrix: [X, X]): the Fock-basis density matrices rho [M, n, n], n <=
        n_levels, in position space, sigma = h E rho E^T with h the spacing of the view's points, which must be
        uniform (wigner.WignerView.uniform_grid's criterion): EnsembleView's grid normalisation, so
        torch.diagonal(sigma).real / h is the position density of rho. rho is assumed Hermitian; sigma is exactly
        Hermitian with a +0.0 imaginary diagonal (include/qcart.h). Fock views only. Asynchronous."""
        if self.grid:
            raise ValueError("SpatialView.density_matrix_of: a grid view's density matrix lives on the grid already")
        rho, one = self._density_matrices(rho)
        if self._spacing is None:
            from .wigner import WignerView
            self._spacing = WignerView.uniform_grid(self._xs)[1]
        M, n = int(rho.shape[0]), int(rho.shape[1])
        out = torch.empty(M, self.x_n, self.x_n, dtype=torch.complex128, device=self.device)
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_spatial_congruence(self._h, vp(rho.data_ptr()), n, M, self._spacing,
                                                      vp(out.data_ptr())))
        return out[0] if one else out

    def table(self) -> torch.Tensor:
        """E [X, n_levels] float64, E[j, n] = psi_n(x[j]): a copy of the device table."""
        if self.grid:
            raise ValueError("SpatialView.table: a grid view has no table")
        out = torch.empty(self.x_n, self.n_levels, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_spatial_table(self._h, ctypes.c_void_p(out.data_ptr())))
        return out
