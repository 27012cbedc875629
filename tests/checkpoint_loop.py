"""The training loop tests/test_gpu_checkpoint.py cuts and resumes, small enough for a few seconds per run, and the
child process of its fresh-process case (python -m tests.checkpoint_loop NAME CHECKPOINT OUT.npz).

One call of the loop: actor.act on the env's observation, env.step, the store into the replay, two learner.step(mem),
and a weight push into the actor every fourth call. Everything is built from fixed initial weights and seeds, so two
Loop(name) objects are the same run."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from deepreinforcementlearningcontrolofquantumcartpoles_amd import checkpoint  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd import config as cfg  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd.actor import (  # noqa: E402
    DQNActor, MeasurementActor, random_direct_dqn, random_dqn_measurement)
from deepreinforcementlearningcontrolofquantumcartpoles_amd.env import BatchedEnv  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd.learner import DQNLearner, MeasurementLearner  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd.replay import PrioritizedReplay  # noqa: E402

# the short warm-up of tests/test_gpu_env_warmup.py, restated: QO at the driver's physics with a free evolution of
# U[0.2, 0.5] time units (4 to 9 calls), its cutoffs, and episodes truncated at t_max = 0.5 (9 calls)
QO_SHORT = dict(init_energy_cutoff=2.0, energy_cutoff=12.0, t_max=0.5, init_time=(0.2, 0.5), reward_multiply=0.37,
                input_scaling=0.7)
# the measurement record's shortest length: read_length must be a multiple of the control-step length m = 80 and long
# enough for the three convolutions (T3 >= 1 needs read_length >= 223): 240. (160, two control steps, is what the
# env-only tests use; the network refuses it.)
READ_LENGTH = 240

IHO63 = cfg.DEFAULTS[cfg.IHO].with_(n_max=63)
CONFIGS = {
    # 1. the ring still in its sequential phase at the cut, random positions after it; set_lr before the cut. The
    # twelfth call fills the ring exactly (len == capacity, data_pointer back at 0), so the cut one call earlier
    # (1a: 948 of 1024 rows written, only those travel) is what covers a ring that is not yet full
    "iho_xp_deferred": dict(ph=IHO63, input="xp", reset="deferred", B=96, capacity=1024, n1=12, n2=12,
                            backup_period=3, set_lr=(5, 1e-4)),
    "iho_xp_deferred_not_full": dict(ph=IHO63, input="xp", reset="deferred", B=96, capacity=1024, n1=11, n2=13,
                                     backup_period=3, set_lr=(5, 1e-4)),
    # 2. the cut after the ring is full; MT19937 noise streams
    "iho_xp_deferred_full_mt": dict(ph=IHO63, input="xp", reset="deferred", B=96, capacity=1024, n1=20, n2=6,
                                    backup_period=3, set_lr=(5, 1e-4), mt=True),
    # 3. the measurement input: record, MeasurementActor, MeasurementLearner
    "iho_measurements": dict(ph=cfg.DEFAULTS[cfg.IHO].with_(n_max=127), input="measurements", reset="deferred", B=40,
                             capacity=512, n1=8, n2=8, env_kw=dict(read_length=READ_LENGTH, input_scaling=0.7)),
    # 3b. the harmonic driver's weight-normalised convolutions, reward target and betas
    "ho_measurements_wn": dict(ph=cfg.DEFAULTS[cfg.HO].with_(n_max=63), input="measurements", reset="deferred", B=40,
                               capacity=512, n1=8, n2=8, env_kw=dict(read_length=READ_LENGTH, input_scaling=0.7),
                               conv_weight_norm=True, target="reward", betas=(0.9, 0.999)),
    # 4. the rolling warm-up; the quartic drivers' 512-wide fc2 and the reward_fail target
    "qo_wavefunction_warmup": dict(ph=cfg.DEFAULTS[cfg.QO], input="wavefunction", reset="warmup", B=24, capacity=512,
                                   n1=26, n2=8, env_kw=QO_SHORT, hidden2=512, target="reward_fail"),
    # 5. the immediate mode: resets on the host inside step()
    "ho_xp_immediate": dict(ph=cfg.DEFAULTS[cfg.HO].with_(n_max=63), input="xp", reset="immediate", B=16,
                            capacity=256, n1=12, n2=8, target="reward", betas=(0.9, 0.999)),
    # 5b. the immediate mode of the quartic cooling driver: its resets draw from the env's torch.Generator
    "qo_xp_immediate": dict(ph=cfg.DEFAULTS[cfg.QO], input="xp", reset="immediate", B=8, capacity=256, n1=20, n2=8,
                            env_kw=QO_SHORT, hidden2=512, target="reward_fail"),
    # 6. IQO x_max = 6.4: a grid of 257 points, 'wavefunction' input of 2 (257 - 20) = 474 floats: at most 512, so
    # the unchunked actor and learner kernels
    "iqo_wavefunction_immediate": dict(ph=cfg.DEFAULTS[cfg.IQO].with_(x_max=6.4), input="wavefunction",
                                       reset="immediate", B=8, capacity=256, n1=20, n2=6, hidden2=512),
}
BATCH = 128
EPS = 0.05


def bits(t) -> np.ndarray:
    """A tensor / array / scalar as a numpy array whose bytes are compared (NaNs and signed zeros count)."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu()
        if t.dtype == torch.bool:
            t = t.to(torch.uint8)
        return t.numpy().copy()
    return np.asarray(t)


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def flatten(prefix: str, state, out: dict):
    """Every tensor and number of a (nested) state dict under a dotted name."""
    if isinstance(state, dict):
        for k, v in state.items():
            flatten(f"{prefix}.{k}", v, out)
    elif isinstance(state, (list, tuple)):
        for i, v in enumerate(state):
            flatten(f"{prefix}.{i}", v, out)
    elif isinstance(state, str):
        out[prefix] = np.frombuffer(state.encode(), dtype=np.uint8)
    elif state is not None:
        out[prefix] = bits(state)


class Loop:
    def __init__(self, name: str):
        c = self.c = CONFIGS[name]
        ph, B = c["ph"], c["B"]
        self.name, self.B, self.calls = name, B, 0
        self.meas = c["input"] == "measurements"
        self.env = BatchedEnv(ph, B, 0, seed=11, input=c["input"], reset=c["reset"], **c.get("env_kw", {}))
        kw = dict(batch_size=BATCH, backup_period=c.get("backup_period", 4), target=c.get("target", "alive"),
                  betas=c.get("betas", (0.9, 0.9995)), seed=41, device=0)
        if self.meas:
            rec = self.env.rec
            w = random_dqn_measurement(read_length=rec.read_length, seed=5,
                                       conv_weight_norm=c.get("conv_weight_norm", False))
            self.actor = MeasurementActor(w, read_length=rec.read_length, max_batch=B, seed=21)
            self.learner = MeasurementLearner(w, rec.read_length, rec.m, **kw)
            row_len = int(self.env.rows.shape[1])
            assert self.learner.row_len == row_len
            self.fixed_obs = torch.randn((B, 2, rec.read_length), generator=torch.Generator().manual_seed(3))
        else:
            L = int(self.env.obs.shape[1])
            h2 = c.get("hidden2", 256)
            w = random_direct_dqn(data_length=L, seed=5, hidden2=h2)
            self.actor = DQNActor(w, data_length=L, max_batch=B, seed=21)
            self.learner = DQNLearner(w, **kw)
            row_len = 2 * L + 2
            self.fixed_obs = torch.randn((B, L), generator=torch.Generator().manual_seed(3))
        self.mem = PrioritizedReplay(c["capacity"], row_len, "random", 0.2, device=0, seed=31)

    def objects(self) -> dict:
        return {"env": self.env, "actor": self.actor, "memory": self.mem, "learner": self.learner}

    def start(self):
        if self.c.get("mt"):
            self.env.st.set_seed_mt19937([1000 + 7 * e for e in range(self.B)])
        self.env.reset()

    def call(self) -> dict:
        env, c = self.env, self.c
        a = self.actor.act(env.obs, eps=EPS)
        obs, reward, done, info = env.step(a)
        if self.meas:
            self.mem.store(info["rows"], info["valid"])
        else:
            nxt = torch.where(done[:, None], info["terminal_obs"], obs) if "terminal_obs" in info else obs
            self.mem.store_xp(info["last_obs"], nxt, a, reward, info["valid"])
        out = {"actions": bits(a), "reward": bits(reward), "done": bits(done), "valid": bits(info["valid"])}
        for j in range(2):
            ul = self.learner.step(self.mem)
            out[f"loss{j}"] = bits(ul) if ul is not None else np.zeros(0, np.float32)
        self.calls += 1
        if self.calls % 4 == 0:
            self.learner.push(self.actor)
        if c.get("set_lr") and self.calls == c["set_lr"][0]:
            self.learner.set_lr(c["set_lr"][1])
        return out

    def final(self, fin_from: int) -> dict:
        out = {}
        flatten("env", self.env.state_dict(), out)
        tree, data = self.mem.buffers()
        out["mem.tree"], out["mem.data"] = bits(tree), bits(data)
        flatten("mem.stats", self.mem.stats(), out)
        flatten("learner.state_dict", self.learner.state_dict(), out)
        flatten("learner.target", self.learner.state_dict(target=True), out)
        flatten("learner.train_state", self.learner.train_state(), out)
        flatten("learner.stats", self.learner.stats(), out)
        flatten("actor.state", self.actor.state_dict(), out)
        a, ex = self.actor.act(self.fixed_obs.cuda(), eps=EPS, counter=777, want_q=True)
        out["actor.fixed_actions"], out["actor.fixed_q"] = bits(a), bits(ex["q"])
        fin = self.env.finished_returns[fin_from:]
        out["finished.returns"] = np.concatenate([bits(r) for r, _ in fin] + [np.zeros(0)])
        out["finished.lengths"] = np.concatenate([bits(n) for _, n in fin] + [np.zeros(0)])
        return out

    def close(self):
        for o in (self.actor, self.mem, self.learner, self.env.st):
            o.close()


def main(argv):
    """The second half of run B in a process of its own: fresh objects, checkpoint.load, n2 calls, an .npz of every
    call's outputs and the final state."""
    name, path, out_path = argv
    loop = Loop(name)
    extra = checkpoint.load(path, loop.objects())
    loop.calls = int(extra["calls"])
    out = {}
    for i in range(CONFIGS[name]["n2"]):
        for k, v in loop.call().items():
            out[f"call{i}.{k}"] = v
    for k, v in loop.final(0).items():
        out["final." + k] = v
    np.savez(out_path, **out)
    torch.cuda.synchronize()
    loop.close()


if __name__ == "__main__":
    main(sys.argv[1:])
