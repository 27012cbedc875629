"""Batched DQN actor on the device.

The reference evaluates its deep-Q network for the actors in one inference process that collects the
actors' inputs through pipes and answers with `action_values.max(1)[1]`
(inverted harmonic oscillator/main_parallel.py:414-440), while each actor applies its epsilon-greedy
choice (main_parallel.py:208-219). `DQNActor` does both for a whole `BatchedEnv` batch in one HIP launch
(csrc/qcart_actor.hip, `qc_actor_act`): direct_DQN's fc1 -> fc2 -> fc31 -> fc41 on f32-input MFMA,
argmax, epsilon-greedy. The parameters are the reference module's state_dict tensors (RL.py:80-111,
layers.py), so a trained `direct_DQN` drops in through `DQNActor(net.state_dict())`.

    actor = DQNActor(net.state_dict(), device=0, seed=seed)
    obs = env.reset()
    while True:
        actions = actor.act(obs, eps=DQNActor.eps_threshold(steps_done))
        obs, reward, done, info = env.step(actions)
"""
from __future__ import annotations

import ctypes
import math
from typing import Mapping, Optional

import torch

from . import _lib as L

LAYERS = ("fc1", "fc2", "fc31", "fc41")
HIDDEN = (512, 256, 256)
HIDDEN2 = (256, 512)   # fc2's width: the harmonic / inverted harmonic net, the quartic / inverted quartic net


def fc2_width(params: Mapping[str, torch.Tensor], hidden2: Optional[int]) -> int:
    """fc2's width of a handle: `hidden2`, or (None) the parameters' own."""
    w = int(params["fc2.weight"].shape[0]) if hidden2 is None else int(hidden2)
    if w not in HIDDEN2:
        raise ValueError(f"hidden2 must be 256 or 512 (fc2's width), not {w}")
    return w


def _layer_tensors(params: Mapping[str, torch.Tensor], name: str, dev: torch.device):
    """(weight, bias, weight_norm, sigma_w, sigma_b) of one layer as contiguous fp32 device tensors:
    Linear_weight_normalize (weight, bias, weight_norm) or FactorizedNoisy (u_w, u_b, sigma_w, sigma_b)."""
    def t(key):
        v = params[f"{name}.{key}"]
        return v.detach().to(device=dev, dtype=torch.float32).contiguous()
    if f"{name}.u_w" in params:
        return t("u_w"), t("u_b"), None, t("sigma_w"), t("sigma_b")
    return t("weight"), t("bias"), t("weight_norm").reshape(1), None, None


class _ActorHandle(L.DeviceHandle):
    """What DQNActor and MeasurementActor share: the handle, and `act` up to the observation's shape."""

    def _create(self, p, device, n_actions: int, max_batch: int):
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs on a HIP device only (no CPU fallback)")
        self.n_actions, self.max_batch = int(n_actions), int(max_batch)
        p.n_actions, p.max_batch = self.n_actions, self.max_batch
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            create = getattr(L.lib(), self._prefix + "_create")
            self._check(create(ctypes.byref(p), self.device.index or 0, ctypes.byref(h)))   # (no handle yet)
        self._h = h
        self.noise_len = int(getattr(L.lib(), self._prefix + "_noise_len")(h))
        self.counter = 0
        self._keep = []

    def _load(self, layers, keep):
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(getattr(L.lib(), self._prefix + "_load")(self._h, layers))
        self._keep = keep   # the prep kernels read them on the current stream

    def act(self, obs: torch.Tensor, eps: float = 0.0, noisy: bool = True, counter: Optional[int] = None,
            noise: Optional[torch.Tensor] = None, env_offset: int = 0, want_q: bool = False,
            want_random: bool = False):
        """Actions [B] int32 for obs [B, data_length] (fp32, the network input; MeasurementActor:
        [B, 2, read_length], the measurement record). noise: optional injected
        NoisyNet noise [B, noise_len] (already f-transformed, layers.py:77-79); else drawn in-kernel
        with Philox (seed, env_offset + e, counter). Returns actions, or (actions, extras) when q / random
        flags are requested."""
        self._check_obs(obs)
        B = obs.shape[0]
        if B > self.max_batch:
            raise ValueError(f"B = {B} exceeds max_batch = {self.max_batch}")
        obs = obs.to(device=self.device, dtype=torch.float32).contiguous()
        if counter is None:
            counter = self.counter
            self.counter += 1
        nz = None
        if noise is not None:
            if tuple(noise.shape) != (B, self.noise_len):
                raise ValueError(f"noise must be [B, {self.noise_len}]")
            nz = noise.to(device=self.device, dtype=torch.float32).contiguous()
        actions = torch.empty(B, dtype=torch.int32, device=self.device)
        q = torch.empty((B, self.n_actions), dtype=torch.float32, device=self.device) if want_q else None
        rnd = torch.empty(B, dtype=torch.int32, device=self.device) if want_random else None
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            self._bind_stream()
            self._check(getattr(L.lib(), self._prefix + "_act")(
                self._h, B, int(env_offset), vp(obs.data_ptr()), 1 if noisy else 0,
                vp(nz.data_ptr()) if nz is not None else None, float(eps), int(counter),
                vp(actions.data_ptr()), vp(q.data_ptr()) if q is not None else None,
                vp(rnd.data_ptr()) if rnd is not None else None))
        if want_q or want_random:
            return actions, {"q": q, "random": rnd}
        return actions


    def _made_for(self) -> dict:
        raise NotImplementedError

    def state_dict(self) -> dict:
        """Everything the next `act` reads, as CPU values (checkpoint.save): the handle's blob (the prepared weights
        as the kernels read them, which layers are noisy, the seed; qc_*_state_export) and the Philox call
        `counter`. Synchronises the actor's stream."""
        with torch.cuda.device(self.device):
            blob = self._export_state()
        return {"kind": self._prefix, **self._made_for(), "blob": blob, "counter": int(self.counter)}

    def check_state_dict(self, state: dict):
        """Raise ValueError naming the first field of `state` this actor was not made for; changes nothing. (The
        library compares the blob's own header again on import.)"""
        L.check_echo(type(self).__name__, state, {"kind": self._prefix, **self._made_for()}, ("blob", "counter"))

    def load_state_dict(self, state: dict):
        """Continue from a `state_dict()`: afterwards `act` gives bit for bit what the saved actor would have.
        Refused (ValueError / QCartError, nothing changed) for an actor of another net or max_batch."""
        self.check_state_dict(state)
        with torch.cuda.device(self.device):
            self._import_state(state["blob"])
        self.counter = int(state["counter"])
        self._keep = []


class DQNActor(_ActorHandle):
    """Device-side action selection for B envs with a reference direct_DQN's parameters. hidden2: fc2's width,
    256 (the harmonic and inverted harmonic drivers' net) or 512 (the quartic and inverted quartic drivers');
    None takes it from `fc2.weight`. It is fixed for the handle's life: `load` refuses the other net."""

    _prefix = "qc_actor"

    def __init__(self, params: Mapping[str, torch.Tensor], data_length: int = 5, n_actions: int = 21,
                 max_batch: int = 65536, device: int | str | torch.device = 0, seed: int = 0,
                 hidden2: Optional[int] = None):
        self.data_length = int(data_length)
        self.hidden2 = fc2_width(params, hidden2)
        p = L.QcDqnParams()
        p.data_length, p.seed, p.hidden2 = self.data_length, int(seed), self.hidden2
        self._create(p, device, n_actions, max_batch)
        self.load(params)

    def _made_for(self) -> dict:
        return {"data_length": self.data_length, "n_actions": self.n_actions, "hidden2": self.hidden2,
                "max_batch": self.max_batch}

    def load(self, params: Mapping[str, torch.Tensor]):
        """(Re)load fc1, fc2, fc31, fc41 from a state_dict (the trainer's periodic push,
        main_parallel.py:400-405). Noisy / weight-normalised layers are recognised by their keys."""
        layers = (L.QcDqnLayer * 4)()
        keep = []
        hidden = (HIDDEN[0], self.hidden2, HIDDEN[2])
        for i, name in enumerate(LAYERS):
            t = _layer_tensors(params, name, self.device)
            out_f = hidden[i] if i < 3 else self.n_actions
            in_f = self.data_length if i == 0 else hidden[i - 1]
            if tuple(t[0].shape) != (out_f, in_f):
                raise ValueError(f"{name}: weight shape {tuple(t[0].shape)} != {(out_f, in_f)}")
            keep += t
            L.fill_layer(layers[i], t)
        self._load(layers, keep)

    @staticmethod
    def eps_threshold(steps_done: float, start: float = 0.1, end: float = 0.003,
                      decay: float = 18 * 100 * 300) -> float:
        """The actor's epsilon schedule (IHO/main_parallel.py:186-189,208-210; decay = n_con*100*300)."""
        return (start - end) * math.exp(-1.0 * steps_done / decay) + end

    def _check_obs(self, obs):
        if obs.dim() != 2 or obs.shape[1] != self.data_length:
            raise ValueError(f"obs must be [B, {self.data_length}]")


def random_direct_dqn(data_length: int = 5, n_actions: int = 21, noisy_layers: int = 2, seed: int = 0,
                      device: str | torch.device = "cpu", hidden2: int = 256) -> dict:
    """Random-initialised parameters of the reference direct_DQN (RL.py:80-111) as a state_dict, with
    the reference's initialisers: nn.Linear's default for Linear_weight_normalize (weight_norm = the
    initial ||W||_F, layers.py:97-100) and FactorizedNoisy's kaiming-uniform u_w, zero u_b and
    sigma = 0.5 / sqrt(in) (layers.py:22-29). hidden2 = 512 gives the quartic drivers' net (fc2 512 -> 512,
    fc31 512 -> 256, fc32 512 -> 128). Synthetic weights for tests and benchmarks."""
    if hidden2 not in HIDDEN2:
        raise ValueError(f"hidden2 must be 256 or 512 (fc2's width), not {hidden2}")
    g = torch.Generator().manual_seed(seed)
    h2 = int(hidden2)

    def linear(name, i, o):
        bound = 1.0 / math.sqrt(i)
        w = (torch.rand((o, i), generator=g) * 2 - 1) * bound
        b = (torch.rand(o, generator=g) * 2 - 1) * bound
        return {f"{name}.weight": w, f"{name}.bias": b, f"{name}.weight_norm": w.norm()}

    def noisy(name, i, o):
        bound = math.sqrt(6.0 / i)   # kaiming_uniform_, fan_in, relu gain
        s = 0.5 / math.sqrt(i)
        return {f"{name}.u_w": (torch.rand((o, i), generator=g) * 2 - 1) * bound,
                f"{name}.sigma_w": torch.full((o, i), s), f"{name}.u_b": torch.zeros(o),
                f"{name}.sigma_b": torch.full((o,), s)}

    p = {}
    p.update(linear("fc1", data_length, 512))
    p.update(linear("fc2", 512, h2))
    p.update(noisy("fc31", h2, 256) if noisy_layers >= 2 else linear("fc31", h2, 256))
    p.update(linear("fc32", h2, 128))
    p.update(noisy("fc41", 256, n_actions) if noisy_layers >= 1 else linear("fc41", 256, n_actions))
    p.update(linear("fc42", 128, 1))
    return {k: v.to(device=device, dtype=torch.float32) for k, v in p.items()}


M_LAYERS = ("conv1", "conv2", "conv3", "fc1", "fc21", "fc31")
M_CONV = ((2, 32, 13, 5), (32, 64, 11, 4), (64, 64, 9, 4))   # (in, out, kernel, stride), RL.py:36-45


def conv_out(n: int, k: int, s: int) -> int:
    """calculate_next_layer_dim (IHO/RL.py:49-50)."""
    return (n - (k - 1) + (s - 1)) // s


def measurement_flat_len(read_length: int) -> int:
    n = read_length
    for _, _, k, s in M_CONV:
        n = conv_out(n, k, s)
    return 64 * n


class MeasurementActor(_ActorHandle):
    """Device-side action selection for B envs with a reference DQN_measurement's parameters (the
    'measurements' input, IHO/RL.py:29-78): obs = MeasurementRecord.hist [B, 2, read_length]. A convolution with
    a `convN.weight_norm` key is the harmonic driver's Conv1d_weight_normalize (HO/RL.py:29-75, layers.py:86-94):
    it acts on W g / ||W||_F. fc1 is nn.Linear in every driver; a weight_norm on it is refused."""

    _prefix = "qc_mactor"

    def __init__(self, params: Mapping[str, torch.Tensor], read_length: int = 5760, n_actions: int = 21,
                 max_batch: int = 65536, device: int | str | torch.device = 0, seed: int = 0, chunk: int = 0):
        self.read_length = int(read_length)
        p = L.QcMdqnParams()
        p.read_length, p.seed, p.chunk = self.read_length, int(seed), int(chunk)
        self._create(p, device, n_actions, max_batch)
        self.flat_len = int(L.lib().qc_mactor_flat_len(self._h))
        self.load(params)

    def _made_for(self) -> dict:
        return {"read_length": self.read_length, "n_actions": self.n_actions, "max_batch": self.max_batch}

    def load(self, params: Mapping[str, torch.Tensor]):
        layers = (L.QcDqnLayer * 6)()
        keep = []
        shapes = [(o, i * k) for i, o, k, _ in M_CONV] + [(256, self.flat_len), (256, 256), (self.n_actions, 256)]
        for j, name in enumerate(M_LAYERS):
            if j < 4:
                w = params[f"{name}.weight"].detach().to(device=self.device, dtype=torch.float32)
                w = w.reshape(w.shape[0], -1).contiguous()
                b = params[f"{name}.bias"].detach().to(device=self.device, dtype=torch.float32).contiguous()
                g = None
                if f"{name}.weight_norm" in params:
                    g = params[f"{name}.weight_norm"].detach().to(device=self.device, dtype=torch.float32).reshape(1)
                t = (w, b, g, None, None)
            else:
                t = _layer_tensors(params, name, self.device)
            if tuple(t[0].shape) != shapes[j]:
                raise ValueError(f"{name}: weight shape {tuple(t[0].shape)} != {shapes[j]}")
            keep += t
            L.fill_layer(layers[j], t)
        self._load(layers, keep)

    def _check_obs(self, obs):
        if obs.dim() != 3 or obs.shape[1] != 2 or obs.shape[2] != self.read_length:
            raise ValueError(f"obs must be [B, 2, {self.read_length}]")


def random_dqn_measurement(read_length: int = 5760, n_actions: int = 21, seed: int = 0,
                           device: str | torch.device = "cpu", conv_weight_norm: bool = False) -> dict:
    """Random-initialised parameters of the reference DQN_measurement (RL.py:29-78) as a state_dict:
    PyTorch's default Conv1d / Linear initialisers (conv biases zeroed, RL.py:46-48), FactorizedNoisy as
    in random_direct_dqn, and the unused mean branch fc22 / fc32. conv_weight_norm: the harmonic driver's
    Conv1d_weight_normalize stack, convN.weight_norm = the initial ||W||_F (layers.py:86-94); the other tensors
    are the same. Synthetic weights for tests / benches."""
    g = torch.Generator().manual_seed(seed)

    def uni(shape, bound):
        return (torch.rand(shape, generator=g) * 2 - 1) * bound

    p = {}
    for j, (ci, co, k, _) in enumerate(M_CONV):
        bound = 1.0 / math.sqrt(ci * k)
        p[f"conv{j + 1}.weight"] = uni((co, ci, k), bound)
        p[f"conv{j + 1}.bias"] = torch.zeros(co)
    flat = measurement_flat_len(read_length)
    p["fc1.weight"] = uni((256, flat), 1.0 / math.sqrt(flat))
    p["fc1.bias"] = uni((256,), 1.0 / math.sqrt(flat))

    def noisy(name, i, o):
        s = 0.5 / math.sqrt(i)
        return {f"{name}.u_w": uni((o, i), math.sqrt(6.0 / i)), f"{name}.sigma_w": torch.full((o, i), s),
                f"{name}.u_b": torch.zeros(o), f"{name}.sigma_b": torch.full((o,), s)}

    def linear(name, i, o):
        w = uni((o, i), 1.0 / math.sqrt(i))
        return {f"{name}.weight": w, f"{name}.bias": uni((o,), 1.0 / math.sqrt(i)), f"{name}.weight_norm": w.norm()}

    p.update(noisy("fc21", 256, 256))
    p.update(noisy("fc31", 256, n_actions))
    p.update(linear("fc22", 256, 128))
    p.update(linear("fc32", 128, 1))
    if conv_weight_norm:
        for j in (1, 2, 3):
            p[f"conv{j}.weight_norm"] = p[f"conv{j}.weight"].norm()
    return {k: v.to(device=device, dtype=torch.float32) for k, v in p.items()}
