"""EnsembleView: the ensemble density matrix of a batch of states on the device (qc_ensemble, include/qcart.h).

rho = (1 / count) sum over the live envs b of |psi_b><psi_b| is the unconditional state of the closed loop: what an
experimenter who does not keep the measurement record has. Its diagonal in the Fock basis is the phonon-number
distribution, Tr rho^2 the purity (how far control plus measurement back-action spread the ensemble), <phi|rho|phi> the
fidelity to any target and Tr(rho A) any observable's ensemble mean; the ensemble mean density (spatial.SpatialView)
and the mean Wigner function (wigner.WignerView) are linear images of it. The definition, the Hermitian output and the
fixed order of the sum are documented in include/qcart.h and DESIGN §9j.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib as L
from . import config as cfg


class EnsembleView(L.DeviceHandle):
    """rho [n, n] of states psi [B, n] complex128 (or one [n] state). `scale` multiplies the outer products: 1 for Fock
    states, the grid spacing h for the grid families' continuum-normalised states (sum h |psi|^2 = 1), so that
    Tr rho = 1 for both; the states are not renormalised. A refused argument raises ValueError, a refusal of the
    library QCartError with its text."""

    _prefix = "qc_ensemble"

    def __init__(self, n: int, scale: float = 1.0, device: int | str | torch.device = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("libqcart needs a HIP device (no CPU fallback)")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n, self.scale = int(n), float(scale)
        hd = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.init()
            L.check_ensemble(L.lib().qc_ensemble_create(self.n, self.scale, self.device.index, ctypes.byref(hd)))
        self._h = hd

    @classmethod
    def for_physics(cls, physics: cfg.Physics, device: int | str | torch.device = 0) -> "EnsembleView":
        """The view of `physics`' states: HO / IHO the n_max + 1 Fock levels with scale 1; QO / IQO the simulation's
        own points with scale = the grid spacing."""
        if physics.fock:
            return cls(physics.n_max + 1, 1.0, device)
        return cls(physics.dim, physics.grid_size, device)

    # ------------------------------------------------------------------ the density matrix
    def density_matrix(self, psi: torch.Tensor, mask: Optional[torch.Tensor] = None):
        """(rho [n, n] complex128, count int64 scalar tensor): rho = scale * sum_b psi_b psi_b^dagger / count over the
        envs whose mask is set (bool or uint8 [B]; None: all), exactly Hermitian with a +0.0 imaginary diagonal,
        summed in the fixed order include/qcart.h documents; count = 0 gives zeros. Asynchronous: both results are
        device tensors, nothing is allocated besides them and nothing waits."""
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
        psi = psi.contiguous()
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
        rho = torch.empty(self.n, self.n, dtype=torch.complex128, device=self.device)
        count = torch.empty((), dtype=torch.int64, device=self.device)
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_ensemble_density(self._h, vp(psi.data_ptr()), B,
                                                    vp(m8.data_ptr()) if m8 is not None else None,
                                                    vp(rho.data_ptr()), vp(count.data_ptr())))
        return rho, count

    # ------------------------------------------------------------------ what rho gives (pure torch, no synchronisation)
    @staticmethod
    def purity(rho: torch.Tensor) -> torch.Tensor:
        """Tr rho^2 = sum_mn |rho_mn|^2 of a Hermitian rho: a real 0-d tensor."""
        return (rho.real * rho.real + rho.imag * rho.imag).sum()

    @staticmethod
    def populations(rho: torch.Tensor) -> torch.Tensor:
        """The real diagonal [n]: in the Fock basis the phonon-number distribution."""
        return torch.diagonal(rho).real.clone()

    def fidelity(self, rho: torch.Tensor, phi: torch.Tensor) -> torch.Tensor:
        """Re <phi|rho|phi> * scale for a target [n] (a 0-d tensor) or targets [K, n] ([K]) in the same normalisation
        as the states: 1 for rho = |phi><phi| of a normalised phi."""
        one = phi.dim() == 1
        p = (phi[None] if one else phi).to(torch.complex128)
        f = ((p.conj() @ rho) * p).sum(dim=1).real * self.scale
        return f[0] if one else f

    @staticmethod
    def expectation(rho: torch.Tensor, op: torch.Tensor) -> torch.Tensor:
        """Tr(rho op) for a dense [n, n] operator in the states' basis (for the grid families, a function f of position
        is op = diag(f(x))): a complex 0-d tensor."""
        return (rho * op.to(rho.dtype).transpose(0, 1)).sum()
