"""LevelView: the energy-level view of a batch of states on the device (qc_levels, include/qcart.h).

What a cooling run is judged by: how much of the state sits in the ground state of the Hamiltonian, and how the rest
spreads over the excited levels. `LevelView.solve` gives the lowest k eigenpairs of the force-free Hamiltonian the
library builds for a physics (a host solve in long double, no GPU needed); a view projects a whole batch of states onto
a real level table: `amplitudes` a[b, k] = scale * sum_j V[k, j] psi[b, j], `populations` |a|^2, and
`mean_populations`, their ensemble mean over the (masked) envs in one fused pass that never writes the per-env
populations. The table is an argument, so the same kernels give any real-basis projection of grid states (for example
the Fock distribution of an inverted-quartic state relative to a reference oscillator, through SpatialView's table).
The definitions and the fixed order of the mean's sum are documented in include/qcart.h and DESIGN §9k.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import config as cfg
from .core import make_params


class LevelView(L.DeviceHandle):
    """Projections of states psi [B, n] complex128 (or one [n] state) onto the rows of `vectors` [k, n] float64 (numpy
    or a CPU tensor; neither orthogonality nor norm is checked), times `scale`. `energies` [k] (optional) are kept
    for `mean_energy`. A refused argument raises ValueError, a refusal of the library QCartError with its text."""

    _prefix = "qc_levels"

    def __init__(self, vectors, scale: float = 1.0, energies=None, device: int | str | torch.device = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("libqcart needs a HIP device (no CPU fallback)")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if isinstance(vectors, torch.Tensor):
            if vectors.device.type != "cpu":
                raise ValueError("vectors must be a numpy array or a CPU tensor (the table is uploaded at create time)")
            vectors = vectors.detach().numpy()
        vectors = np.asarray(vectors)
        if vectors.dtype != np.float64 or vectors.ndim != 2:
            raise ValueError("vectors must be a float64 [k, n] table")
        table = np.array(vectors, dtype=np.float64, order="C", copy=True)
        self.k, self.n = int(table.shape[0]), int(table.shape[1])
        self.scale = float(scale)
        e = None
        if energies is not None:
            e = np.asarray(energies.detach().cpu().numpy() if isinstance(energies, torch.Tensor) else energies,
                           dtype=np.float64)
            if e.shape != (self.k,):
                raise ValueError(f"energies must be [{self.k}], one per level")
        hd = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.init()
            L.check_levels(L.lib().qc_levels_create(self.n, self.k, self.scale, ctypes.c_void_p(table.ctypes.data),
                                                    self.device.index, ctypes.byref(hd)))
        self._h = hd
        self.vectors = torch.from_numpy(table).to(self.device)
        self.energies = torch.from_numpy(e.copy()).to(self.device) if e is not None else None

    # ------------------------------------------------------------------ the host solve
    @staticmethod
    def solve(physics: cfg.Physics, k: int = 32):
        """(energies [k], vectors [k, n]) as numpy arrays: the lowest k levels of `physics`' force-free Hamiltonian,
        rows of unit l2 norm with the outermost lobe on the +x side positive. Host only. HO: omega (n + 1/2) and the
        identity; QO: the grid Hamiltonian's levels; IHO / IQO are refused (ValueError with the library's text)."""
        p = make_params(physics, 1)
        n = physics.dim
        kk = int(k)
        energies = np.empty(max(kk, 1), dtype=np.float64)
        vectors = np.empty((max(kk, 1), max(n, 1)), dtype=np.float64)
        rc = L.lib().qc_levels_solve(ctypes.byref(p), kk, ctypes.c_void_p(energies.ctypes.data),
                                     ctypes.c_void_p(vectors.ctypes.data))
        if rc < 0:
            msg = L.lib().qc_levels_last_error(None)
            text = msg.decode() if msg else ""
            if rc == -1:
                raise ValueError(text)
            raise L.QCartError(rc, text)
        return energies[:kk], vectors[:kk]

    @classmethod
    def for_physics(cls, physics: cfg.Physics, k: int = 32, device: int | str | torch.device = 0) -> "LevelView":
        """The view of `physics`' own levels: QO with scale = sqrt(grid spacing), so that sum_k p is the in-band part
        of sum_j h |psi_j|^2; HO with scale 1 (the Fock basis is the energy basis). IHO / IQO have no bound levels:
        ValueError with the library's text (pass a table of your own instead)."""
        energies, vectors = cls.solve(physics, k)
        scale = 1.0 if physics.fock else math.sqrt(physics.grid_size)
        return cls(vectors, scale, energies, device)

    # ------------------------------------------------------------------ the projections
    def _states(self, psi: torch.Tensor) -> torch.Tensor:
        if not isinstance(psi, torch.Tensor):
            raise ValueError("psi must be a torch tensor")
        if psi.dtype != torch.complex128:
            raise ValueError(f"psi must be complex128, not {psi.dtype} (the fp32 handles' complex64 states are not "
                             "viewed)")
        if psi.device != self.device:
            raise ValueError(f"psi must live on {self.device}, not {psi.device}")
        if psi.dim() == 1:
            psi = psi[None]
        if psi.dim() != 2 or psi.shape[0] < 1:
            raise ValueError("psi must be [B, n] (or one [n] state)")
        if int(psi.shape[1]) != self.n:
            raise ValueError(f"this view takes states of {self.n} components, not {int(psi.shape[1])}")
        return psi.contiguous()

    def amplitudes(self, psi: torch.Tensor) -> torch.Tensor:
        """a [B, k] complex128: scale * V psi_b for every state. Asynchronous."""
        psi = self._states(psi)
        out = torch.empty(psi.shape[0], self.k, dtype=torch.complex128, device=self.device)
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_levels_amplitudes(self._h, vp(psi.data_ptr()), psi.shape[0], vp(out.data_ptr())))
        return out

    def populations(self, psi: torch.Tensor) -> torch.Tensor:
        """p [B, k] float64: fl(fl(Re a^2) + fl(Im a^2)) of exactly `amplitudes`' values. Asynchronous."""
        psi = self._states(psi)
        out = torch.empty(psi.shape[0], self.k, dtype=torch.float64, device=self.device)
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_levels_populations(self._h, vp(psi.data_ptr()), psi.shape[0], vp(out.data_ptr())))
        return out

    def mean_populations(self, psi: torch.Tensor, mask: Optional[torch.Tensor] = None):
        """(m [k] float64, count int64 scalar tensor): the mean of the populations over the envs whose mask is set
        (bool or uint8 [B]; None: all), summed in the fixed order include/qcart.h documents; count = 0 gives zeros. No
        per-env populations are written. Asynchronous: both results are device tensors and nothing waits."""
        psi = self._states(psi)
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
        out = torch.empty(self.k, dtype=torch.float64, device=self.device)
        count = torch.empty((), dtype=torch.int64, device=self.device)
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_levels_mean(self._h, vp(psi.data_ptr()), B,
                                               vp(m8.data_ptr()) if m8 is not None else None,
                                               vp(out.data_ptr()), vp(count.data_ptr())))
        return out, count

    def mean_energy(self, pops: torch.Tensor) -> torch.Tensor:
        """sum_k E_k pops[..., k]: the energy of a level distribution (in band). Pure torch, no synchronisation."""
        if self.energies is None:
            raise ValueError("this view was made without energies")
        return (pops * self.energies).sum(dim=-1)
