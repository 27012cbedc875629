"""Device DQN learner: the reference's TrainDQN.__call__ with its LaProp optimizer on the device.

The reference learns in one process that samples `batch_size` transitions from the prioritized memory,
evaluates direct_DQN three times (online on the next and previous states, target on the next states),
backpropagates the importance-weighted TD loss and takes one LaProp step (inverted harmonic
oscillator/RL.py:159-232, optimizer.py). `DQNLearner` does one such update in eight HIP launches
(csrc/qcart_learner.hip, `qc_learner_update`) without leaving the device:

    learner = DQNLearner(net.state_dict(), batch_size=512, lr=4e-4)
    while training:
        ...                                   # env.step / memory.store_xp, see BatchedEnv / PrioritizedReplay
        for _ in range(n_learn):
            learner.step(memory)              # obtain_sample -> update -> batch_update
        learner.push(actor)                   # device-to-device weight push into a DQNActor

`batch_size` must be a multiple of 128 (at most 4096): the learner implements FactorizedNoisy's batched
branch, 32 noise samples per batch, one per chunk of batch_size / 32 rows (layers.py:57-74); other batch sizes
take the reference's per-row branch, which is refused (ValueError). Only direct_DQN(noisy_layers=2) is covered.

The reference's four drivers differ in fc2's width, the TD target and LaProp's betas; the constructor takes all
three (defaults: the inverted harmonic driver's):

    driver               hidden2   target          betas
    inverted harmonic    256       "alive"         (0.9, 0.9995)
    inverted quartic     512       "alive"         (0.9, 0.9995)
    quartic              512       "reward_fail"   (0.9, 0.9995)
    harmonic             256       "reward"        (0.9, 0.999)

"alive": y = gamma nsv + (1 - gamma) alive_reward, 0 where the row's reward == failing_reward; "reward_fail":
y = gamma nsv + (1 - gamma) reward, the reward itself where it is <= failing_reward; "reward": the same with no
fail rule.
"""
from __future__ import annotations

import ctypes
from typing import Mapping, Optional

import torch

from . import _lib as L
from .actor import M_CONV, _layer_tensors, fc2_width, measurement_flat_len
from .replay import _view

LAYERS = ("fc1", "fc2", "fc31", "fc41", "fc32", "fc42")
NOISY = (False, False, True, True, False, False)


def _shapes(data_length: int, n_actions: int, hidden2: int = 256):
    return ((512, data_length), (hidden2, 512), (256, hidden2), (n_actions, 256), (128, hidden2), (1, 128))


class _Learner(L.DeviceHandle):
    """What the two learners share over one libqcart handle family `_prefix`: the constructor's checks, and every
    call that differs between them only in that prefix. A subclass supplies `_prefix`, `_n_layers`, `_max_batch`,
    `_layer_array`, `_tensors` and `push`, and sets `batch_size`, `row_len` and `n_actions` before `_create`."""

    _n_layers = 0
    _max_batch = 0

    def _fn(self, name: str):
        return getattr(L.lib(), f"{self._prefix}_{name}")

    def _layers(self):
        return (L.QcDqnLayer * self._n_layers)()

    def _resolve(self, device, batch_size: int):
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs on a HIP device only (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if batch_size % 128 != 0 or not 128 <= batch_size <= self._max_batch:
            raise ValueError(f"batch_size must be a multiple of 128 in [128, {self._max_batch}] (FactorizedNoisy's "
                             "32-chunk noise branch; the per-row branch of other sizes is not implemented)")

    def _schedule(self, target: str, betas):
        if target not in L.TD_TARGETS:
            raise ValueError(f"target must be one of {sorted(L.TD_TARGETS)}, not {target!r}")
        self.target = target
        self.betas = (float(betas[0]), float(betas[1]))
        for name, b in zip(("beta1", "beta2"), self.betas):
            if not 0. < b < 1.:
                raise ValueError(f"{name} (betas) must be in (0, 1), not {b}")

    def _create(self, p, params, gamma, lr, alive_reward, failing_reward, backup_period, seed):
        """Fill the fields the two params structs share, create the handle and load `params`."""
        p.n_actions, p.batch_size = self.n_actions, self.batch_size
        p.backup_period, p.target_mode = int(backup_period), L.TD_TARGETS[self.target]
        p.gamma, p.lr = float(gamma), float(lr)
        p.alive_reward, p.failing_reward, p.seed = float(alive_reward), float(failing_reward), int(seed)
        p.beta1, p.beta2 = self.betas
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.init()
            self._check(self._fn("create")(ctypes.byref(p), self.device.index, ctypes.byref(h)))
        self._h = h
        self._made = {"gamma": p.gamma, "alive_reward": p.alive_reward, "failing_reward": p.failing_reward,
                      "backup_period": p.backup_period, "seed": p.seed}   # what a train_state echoes besides the net
        self.noise_len = int(self._fn("noise_len")(h))
        self.counter = 0
        self.last_loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._keep = []
        self.load_state_dict(params)

    def _send(self, fn: str, params: Mapping[str, torch.Tensor]):
        layers, keep = self._layer_array(params)
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(self._fn(fn)(self._h, layers))
        self._keep = keep   # the copies read them on the current stream

    def load_state_dict(self, params: Mapping[str, torch.Tensor]):
        """Load the layers from a state_dict (the reference net's, or actor.random_direct_dqn's /
        actor.random_dqn_measurement's; a MeasurementLearner's must have the handle's kind of convolutions);
        resets the optimizer state and the target schedule."""
        self._send("load", params)

    def _copies(self, fn: str, *args) -> dict:
        layers = self._layers()
        self._check(self._fn(fn)(self._h, *args, layers))
        with torch.cuda.device(self.device):
            return {k: v.clone() for k, v in self._tensors(layers).items()}

    def state_dict(self, target: bool = False) -> dict:
        """The online (or target) parameters under the reference's key names, as device copies."""
        return self._copies("layers", 1 if target else 0)

    def grads(self) -> dict:
        """Gradients of the last update under the parameters' key names (weight_norm: dg), as device copies."""
        return self._copies("grads")

    def apply(self, grads: Mapping[str, torch.Tensor]):
        """One LaProp step on injected gradients (tests)."""
        self._send("apply", grads)

    def set_lr(self, lr: float):
        self._check(self._fn("set_lr")(self._h, float(lr)))

    def set_backup_period(self, n: int):
        """The target network's period from the next update on (Main_System's temporary 100 before learning starts,
        IHO/main_parallel.py:480-481, 546-547); backup_counter is reduced modulo n. A train_state keeps echoing the
        create-time period and carries the one in use in its blob."""
        self._check(self._fn("set_backup_period")(self._h, int(n)))

    def _rows(self, transitions: torch.Tensor) -> torch.Tensor:
        if transitions.dim() != 2 or tuple(transitions.shape) != (self.batch_size, self.row_len):
            raise ValueError(f"transitions must be [{self.batch_size}, {self.row_len}]")
        return transitions.to(device=self.device, dtype=torch.float32).contiguous()

    def update(self, transitions: torch.Tensor, is_weights: torch.Tensor, noise: Optional[torch.Tensor] = None,
               counter: Optional[int] = None) -> torch.Tensor:
        """One update on transitions [batch_size, row_len] (DQNLearner: row_len = 2 data_length + 2;
        MeasurementLearner: rows of MeasurementRecord) and IS weights [batch_size]. noise: optional
        [32, noise_len], already f-transformed, the actor's layout per chunk; else Philox (seed, chunk, counter).
        Returns unweighted_loss [batch_size] (device); the scalar loss stays in `last_loss` (device).
        Asynchronous: an action outside [0, n_actions) is clamped and raised by the next `stats()`."""
        tr = self._rows(transitions)
        if is_weights.numel() != self.batch_size:
            raise ValueError(f"is_weights must be [{self.batch_size}]")
        w = is_weights.to(device=self.device, dtype=torch.float32).contiguous()
        nz = None
        if noise is not None:
            if tuple(noise.shape) != (32, self.noise_len):
                raise ValueError(f"noise must be [32, {self.noise_len}]")
            nz = noise.to(device=self.device, dtype=torch.float32).contiguous()
        if counter is None:
            counter = self.counter
            self.counter += 1
        ul = torch.empty(self.batch_size, dtype=torch.float32, device=self.device)
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(self._fn("update")(
                self._h, vp(tr.data_ptr()), vp(w.data_ptr()), vp(nz.data_ptr()) if nz is not None else None,
                int(counter), vp(ul.data_ptr()), vp(self.last_loss.data_ptr())))
        return ul

    def step(self, memory, counter: Optional[int] = None):
        """TrainDQN.__call__: obtain_sample -> update -> memory.batch_update(tree_idx, unweighted_loss). None
        while len(memory) < batch_size (RL.py:161)."""
        smp = memory.obtain_sample(self.batch_size)
        if smp is None:
            return None
        tree_idx, is_weights, transitions = smp
        ul = self.update(transitions, is_weights, counter=counter)
        memory.batch_update(tree_idx, ul)
        return ul

    def _push(self, actor, load, check):
        """The online layers into an actor handle through `load`, device to device (no host copy)."""
        layers = self._layers()
        self._check(self._fn("layers")(self._h, 0, layers))
        with torch.cuda.device(self.device):
            actor._bind_stream()
            check(load(actor._h, layers), actor._h)

    def _made_for(self) -> dict:
        raise NotImplementedError

    def train_state(self) -> dict:
        """Everything the next `update` reads, as CPU values (checkpoint.save) — `state_dict()` stays the weights
        in the reference's keys. The handle's blob (online and target parameters, LaProp's three moment buffers,
        the prepared fragments, updates, step, backup_counter, lr, l1, l2; qc_*_state_export) and the Philox call
        `counter`. Synchronises the learner's stream."""
        with torch.cuda.device(self.device):
            blob = self._export_state()
        return {"kind": self._prefix, **self._made_for(), "blob": blob, "counter": int(self.counter)}

    def check_train_state(self, state: dict):
        """Raise ValueError naming the first field of `state` this learner was not made for; changes nothing. (The
        library compares the blob's own header, with gamma, the rewards, betas and seed, again on import.)"""
        L.check_echo(type(self).__name__, state, {"kind": self._prefix, **self._made_for()}, ("blob", "counter"))

    def load_train_state(self, state: dict):
        """Continue from a `train_state()`: every later update, push and state_dict gives bit for bit what the saved
        learner would have. A learner made with other parameters is refused (ValueError / QCartError, nothing
        changed); the learning rate is state (`set_lr`) and is restored, not compared."""
        self.check_train_state(state)
        with torch.cuda.device(self.device):
            self._import_state(state["blob"])
        self.counter = int(state["counter"])
        self._keep = []

    def stats(self) -> dict:
        """Synchronises. Raises QCartError if an update since the last call saw an out-of-range action."""
        s = L.QcLearnerStats()
        self._check(self._fn("stats")(self._h, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in L.QcLearnerStats._fields_}


class DQNLearner(_Learner):
    """TrainDQN for direct_DQN(data_length, noisy_layers=2) with LaProp(centered, betas); hidden2 (None: from
    `fc2.weight`), target and betas select the driver (module docstring)."""

    _prefix = "qc_learner"
    _n_layers = 6
    _max_batch = 4096

    def __init__(self, params: Mapping[str, torch.Tensor], batch_size: int = 512, gamma: float = 0.998,
                 lr: float = 4e-4, alive_reward: float = 10., failing_reward: float = -1., backup_period: int = 300,
                 device: int | str | torch.device = 0, seed: int = 0, data_length: Optional[int] = None,
                 n_actions: Optional[int] = None, hidden2: Optional[int] = None, target: str = "alive",
                 betas=(0.9, 0.9995)):
        self._resolve(device, batch_size)
        if "fc1.weight" not in params or "fc41.u_w" not in params:
            raise ValueError("params must be a direct_DQN(noisy_layers=2) state_dict (fc1.weight, ..., fc41.u_w)")
        if "fc2.weight" not in params:
            raise ValueError("params must be a direct_DQN(noisy_layers=2) state_dict (fc2.weight is missing)")
        self.hidden2 = fc2_width(params, hidden2)
        self._schedule(target, betas)
        self.data_length = int(data_length if data_length is not None else params["fc1.weight"].shape[1])
        self.n_actions = int(n_actions if n_actions is not None else params["fc41.u_w"].shape[0])
        self.batch_size = int(batch_size)
        self.row_len = 2 * self.data_length + 2
        p = L.QcLearnerParams()
        p.data_length, p.hidden2 = self.data_length, self.hidden2
        self._create(p, params, gamma, lr, alive_reward, failing_reward, backup_period, seed)

    def _made_for(self) -> dict:
        return {"data_length": self.data_length, "n_actions": self.n_actions, "hidden2": self.hidden2,
                "batch_size": self.batch_size, "target": self.target, "betas": self.betas, **self._made}

    def _layer_array(self, params: Mapping[str, torch.Tensor]):
        layers = self._layers()
        keep = []
        for i, (name, shape) in enumerate(zip(LAYERS, _shapes(self.data_length, self.n_actions, self.hidden2))):
            if NOISY[i] != (f"{name}.u_w" in params):
                raise ValueError(f"{name}: the learner covers direct_DQN(noisy_layers=2) only")
            t = _layer_tensors(params, name, self.device)
            if tuple(t[0].shape) != shape:
                raise ValueError(f"{name}: weight shape {tuple(t[0].shape)} != {shape}")
            keep += t
            L.fill_layer(layers[i], t)
        return layers, keep

    def _tensors(self, layers) -> dict:
        out = {}
        for i, (name, (o, k)) in enumerate(zip(LAYERS, _shapes(self.data_length, self.n_actions, self.hidden2))):
            ly = layers[i]
            if NOISY[i]:
                out[f"{name}.u_w"] = _view(ly.weight, o * k, torch.float32, self.device).view(o, k)
                out[f"{name}.sigma_w"] = _view(ly.sigma_w, o * k, torch.float32, self.device).view(o, k)
                out[f"{name}.u_b"] = _view(ly.bias, o, torch.float32, self.device)
                out[f"{name}.sigma_b"] = _view(ly.sigma_b, o, torch.float32, self.device)
            else:
                out[f"{name}.weight"] = _view(ly.weight, o * k, torch.float32, self.device).view(o, k)
                out[f"{name}.bias"] = _view(ly.bias, o, torch.float32, self.device)
                out[f"{name}.weight_norm"] = _view(ly.weight_norm, 1, torch.float32, self.device).view(())
        return out

    def push(self, actor):
        """Load the online fc1, fc2, fc31, fc41 into a DQNActor, device to device (no host copy). The actor's
        net must be the learner's: the load reads the tensors at the actor's own sizes."""
        if (actor.hidden2, actor.data_length, actor.n_actions) != (self.hidden2, self.data_length, self.n_actions):
            raise ValueError(f"push: the actor's net (hidden2 {actor.hidden2}, data_length {actor.data_length}, "
                             f"n_actions {actor.n_actions}) is not the learner's (hidden2 {self.hidden2}, "
                             f"data_length {self.data_length}, n_actions {self.n_actions})")
        self._push(actor, L.lib().qc_actor_load, L.check_actor)


M_LEARNER_LAYERS = ("conv1", "conv2", "conv3", "fc1", "fc21", "fc31", "fc22", "fc32")
_M_KIND = ("conv", "conv", "conv", "plain", "noisy", "noisy", "wn", "wn")   # conv: plain, or weight-normalised


def measurement_row_len(read_length: int, read_step_length: int) -> int:
    """Length of a 'measurements' replay row (qc_record): L + m measurements, K + 1 forces, action, reward."""
    return read_length + read_step_length + read_length // read_step_length + 3


class MeasurementLearner(_Learner):
    """TrainDQN for DQN_measurement (the 'measurements' input, RL.py:29-78 and :159-232) with centred LaProp: one
    update per call on `batch_size` rows of MeasurementRecord (csrc/qcart_mlearner.hip, `qc_mlearner_update`),
    without leaving the device:

        learner = MeasurementLearner(net.state_dict(), rec.read_length, rec.m, batch_size=512)
        while training:
            ...                               # MeasurementRecord.record(rows=...) -> memory.store
            learner.step(memory)              # obtain_sample -> update -> batch_update
            learner.push(mactor)              # device-to-device weight push into a MeasurementActor

    The two drivers that train this net differ in the convolutions, the TD target, LaProp's betas and the geometry:

        driver               conv1..3                   target     betas            read_length, m
        inverted harmonic    Conv1d                     "alive"    (0.9, 0.9995)    5760, 80
        harmonic             Conv1d_weight_normalize    "reward"   (0.9, 0.999)     4320, 80

    The convolutions are taken from the state_dict: with a `convN.weight_norm` on all three the handle is a
    weight-normalised one (`conv_weight_norm`; effective weight W g / ||W||_F, 25 parameter tensors instead of 22,
    the three g learned through the chain rule), with none a plain one. A state_dict with some of the three lands
    on a plain handle, which refuses it naming the layer; fc1 is nn.Linear in both drivers and a weight_norm on it
    is refused. batch_size: a multiple of 128 in [128, 1024]."""

    _prefix = "qc_mlearner"
    _n_layers = 8
    _max_batch = 1024

    def __init__(self, params: Mapping[str, torch.Tensor], read_length: int, read_step_length: int,
                 batch_size: int = 512, gamma: float = 0.998, lr: float = 4e-4, alive_reward: float = 10.,
                 failing_reward: float = -1., backup_period: int = 300, target: str = "alive",
                 betas=(0.9, 0.9995), device: int | str | torch.device = 0, seed: int = 0):
        self._resolve(device, batch_size)
        if "conv1.weight" not in params or "fc31.u_w" not in params:
            raise ValueError("params must be a DQN_measurement state_dict (conv1.weight, ..., fc31.u_w)")
        if read_step_length < 1 or read_length % read_step_length != 0:
            raise ValueError(f"read_length {read_length} must be a multiple of read_step_length {read_step_length}")
        self._schedule(target, betas)
        self.read_length, self.read_step_length = int(read_length), int(read_step_length)
        self.n_actions = int(params["fc31.u_w"].shape[0])
        self.batch_size = int(batch_size)
        self.conv_weight_norm = all(f"conv{j}.weight_norm" in params for j in (1, 2, 3))
        self.flat_len = measurement_flat_len(self.read_length)
        self.row_len = measurement_row_len(self.read_length, self.read_step_length)
        p = L.QcMlearnerParams()
        p.read_length, p.read_step_length = self.read_length, self.read_step_length
        p.conv_weight_norm = 1 if self.conv_weight_norm else 0
        self._create(p, params, gamma, lr, alive_reward, failing_reward, backup_period, seed)

    def _made_for(self) -> dict:
        return {"read_length": self.read_length, "read_step_length": self.read_step_length,
                "n_actions": self.n_actions, "conv_weight_norm": bool(self.conv_weight_norm),
                "batch_size": self.batch_size, "target": self.target, "betas": self.betas, **self._made}

    def _shapes(self):
        return [(o, i, k) for i, o, k, _ in M_CONV] + [(256, self.flat_len), (256, 256), (self.n_actions, 256),
                                                       (128, 256), (1, 128)]

    def _layer_array(self, params: Mapping[str, torch.Tensor]):
        layers = self._layers()
        keep = []
        for i, (name, shape) in enumerate(zip(M_LEARNER_LAYERS, self._shapes())):
            if _M_KIND[i] in ("conv", "plain"):
                if f"{name}.weight" not in params:
                    raise ValueError(f"{name}.weight is missing: not a DQN_measurement state_dict")

                def t(key):
                    return params[f"{name}.{key}"].detach().to(device=self.device, dtype=torch.float32).contiguous()
                g = t("weight_norm").reshape(1) if f"{name}.weight_norm" in params else None
                # the library decides: a weight_norm the handle has no use for, or a missing one, is refused by name
                ts = (t("weight"), t("bias"), g, None, None)
            else:
                if (_M_KIND[i] == "noisy") != (f"{name}.u_w" in params):
                    raise ValueError(f"{name}: the learner covers DQN_measurement's fc21 / fc31 FactorizedNoisy and "
                                     "fc22 / fc32 Linear_weight_normalize only")
                ts = _layer_tensors(params, name, self.device)
            if tuple(ts[0].shape) != shape:
                raise ValueError(f"{name}: weight shape {tuple(ts[0].shape)} != {shape}")
            keep += ts
            L.fill_layer(layers[i], ts)
        return layers, keep

    def _tensors(self, layers) -> dict:
        out = {}
        for i, (name, shape) in enumerate(zip(M_LEARNER_LAYERS, self._shapes())):
            ly, o = layers[i], shape[0]
            n = 1
            for d in shape:
                n *= d
            w = _view(ly.weight, n, torch.float32, self.device).view(*shape)
            b = _view(ly.bias, o, torch.float32, self.device)
            if _M_KIND[i] == "noisy":
                out[f"{name}.u_w"] = w
                out[f"{name}.sigma_w"] = _view(ly.sigma_w, n, torch.float32, self.device).view(*shape)
                out[f"{name}.u_b"] = b
                out[f"{name}.sigma_b"] = _view(ly.sigma_b, o, torch.float32, self.device)
            else:
                out[f"{name}.weight"] = w
                out[f"{name}.bias"] = b
                if _M_KIND[i] == "wn" or (_M_KIND[i] == "conv" and self.conv_weight_norm):
                    out[f"{name}.weight_norm"] = _view(ly.weight_norm, 1, torch.float32, self.device).view(())
        return out

    def states(self, transitions: torch.Tensor):
        """(next, prev) [batch_size, 2, read_length]: the states the update assembles from the rows (tests)."""
        tr = self._rows(transitions)
        nxt = torch.empty((self.batch_size, 2, self.read_length), dtype=torch.float32, device=self.device)
        prv = torch.empty_like(nxt)
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(L.lib().qc_mlearner_states(self._h, vp(tr.data_ptr()), vp(nxt.data_ptr()), vp(prv.data_ptr())))
        return nxt, prv

    def push(self, mactor):
        """Load the online conv1..3, fc1, fc21, fc31 into a MeasurementActor, device to device."""
        if (mactor.read_length, mactor.n_actions) != (self.read_length, self.n_actions):
            raise ValueError(f"push: the actor's net (read_length {mactor.read_length}, n_actions {mactor.n_actions}) "
                             f"is not the learner's (read_length {self.read_length}, n_actions {self.n_actions})")
        self._push(mactor, L.lib().qc_mactor_load, L.check_mactor)
