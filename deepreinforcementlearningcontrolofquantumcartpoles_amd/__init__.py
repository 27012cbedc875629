"""MI355X-native quantum-cartpole environment (env.step() hot path in HIP for gfx950).

Modules:
  _lib        ctypes binding of libqcart.so (include/qcart.h)
  config      physics presets of the four reference systems
  core        Stepper: one libqcart handle + device tensors
  simulation  drop-in surface of the reference `simulation` extension (B = 1)
  env         BatchedEnv: reset/step/observation semantics of the reference drivers, batched
  distributed env sharding over ranks + RCCL gather of episode returns
  learner     DQNLearner / MeasurementLearner: the reference's TrainDQN update on the device
  spatial     SpatialView: the drivers' spatial_repr / probability (position-space density) of a batch of states, and
              the Fock -> position change of basis of density matrices
  wigner      WignerView: the Wigner function (phase-space view) of a batch of states, its ensemble mean, and the
              Wigner function and negative volume of density matrices
  ensemble    EnsembleView: the ensemble density matrix of a batch of states; purity, populations, fidelity
  levels      LevelView: eigenstates of the force-free Hamiltonian (host solve) and the level populations of a batch
  lindblad    MasterEquation: the open-loop evolution of density matrices (the ensemble limit, the no-control curve)
  checkpoint  save / load of the whole device loop; the resumed run is the uninterrupted one bit for bit
"""
from .config import DEFAULTS, HO, IHO, IQO, QO, Physics  # noqa: F401

__all__ = ["DEFAULTS", "HO", "IHO", "QO", "IQO", "Physics", "DQNLearner", "MeasurementLearner", "SpatialView",
           "WignerView", "EnsembleView", "LevelView", "MasterEquation"]


def __getattr__(name):
    # the learners need torch: imported on first use, so `import <package>` stays light
    if name in ("DQNLearner", "MeasurementLearner"):
        from . import learner
        return getattr(learner, name)
    if name == "SpatialView":
        from . import spatial
        return spatial.SpatialView
    if name == "WignerView":
        from . import wigner
        return wigner.WignerView
    if name == "EnsembleView":
        from . import ensemble
        return ensemble.EnsembleView
    if name == "LevelView":
        from . import levels
        return levels.LevelView
    if name == "MasterEquation":
        from . import lindblad
        return lindblad.MasterEquation
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
