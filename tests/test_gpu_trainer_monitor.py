"""train.Trainer with a train.Monitor attached, on the HO and QO loops of tests/test_gpu_trainer.py (HO n_max = 63,
16 envs, t_max = 0.5; QO with the rolling warm-up and QO_SHORT, 24 envs) with performance_from = 0.2: against a serial
loop written here from the public pieces plus tests/sched_ref.py and tests/monitor_ref.py, bit for bit, the ranked
files included; checkpoint and resume with a receive still to be acted on; evaluate on the performance; the refusal
of another num_of_saves; and a Trainer without a monitor, which writes the files it wrote before.

The monitor's constants are scaled to these loops (window = min_count = 2, more than 3 episodes between two records),
read from a first run. HO ends its 16 episodes together every ninth step and pushes after each such burst, at 16, 32,
48 and 64 episodes: the window means 1.63, 5.76 and a third fill a table of 3 from the front, the fourth goes ahead
of filled entries and one falls out. QO_SHORT pushes at 14, 19, 26, 31, 34 and 42 episodes with window means 3.67,
3.00, 2.40 (each ahead of the last), 4.30 (behind the three filled entries of a table of 4), then too few new
episodes, then 7.2 (refused)."""
import os

import numpy as np
import pytest
import torch

from tests import monitor_ref as M
from tests import sched_ref as R
from tests import test_gpu_trainer as T
from tests.checkpoint_loop import bits

pytestmark = pytest.mark.gpu

PERF_FROM = 0.2
MON = {"ho": M.params(window=2, min_count=2, min_episodes=3, num_of_saves=3, initial=20.0),
       "qo": M.params(window=2, min_count=2, min_episodes=3, num_of_saves=4, initial=6.0)}


class Loop(T.Loop):
    """tests/test_gpu_trainer.py's objects of one case, the env made with performance_from, and a monitor."""

    def __init__(self, name, with_schedule=True, with_monitor=True, num_of_saves=None):
        P = self.P = T._pkg()
        from deepreinforcementlearningcontrolofquantumcartpoles_amd.train import Monitor
        c = self.c = T.cases(P["cfg"])[name]
        B = self.B = c["B"]
        self.env = P["BatchedEnv"](c["ph"], B, 0, seed=11, input="xp", reset=c["reset"], performance_from=PERF_FROM,
                                   **c["env_kw"])
        n_in = int(self.env.obs.shape[1])
        w = P["random_direct_dqn"](data_length=n_in, seed=5, hidden2=c["hidden2"])
        self.actor = P["DQNActor"](w, data_length=n_in, max_batch=B, seed=21)
        self.learner = P["DQNLearner"](w, batch_size=T.BATCH, backup_period=c["sched"]["backup_period"], seed=41,
                                       device=0, lr=c["sched"]["lr_init"], **c["learner_kw"])
        self.mem = P["PrioritizedReplay"](c["capacity"], 2 * n_in + 2, "random", 0.2, device=0, seed=31)
        self.schedule = P["Schedule"](device=0, **c["sched"]) if with_schedule else None
        self.num_of_saves = MON[name]["num_of_saves"] if num_of_saves is None else num_of_saves
        self.monitor = Monitor(device=0, **dict(MON[name], num_of_saves=self.num_of_saves)) if with_monitor else None

    def trainer(self, save_dir, num_of_saves=None):
        num_of_saves = self.num_of_saves if num_of_saves is None else num_of_saves
        return self.P["Trainer"](self.env, self.actor, self.mem, self.learner, self.schedule, save_dir=str(save_dir),
                                 eps=T.eps, num_of_saves=num_of_saves, monitor=self.monitor)

    def final(self, save_dir) -> dict:
        out = super().final(save_dir)
        out.pop("env._perf_read", None)     # how far finished_performances has been read: the serial loop reads it
        return out

    def close(self):
        super().close()
        if self.monitor is not None:
            self.monitor.close()


_RUNS = {}


def trainer_run(name, tmp_path_factory):
    """The uninterrupted run of a case with a monitor, once per session."""
    if name not in _RUNS:
        save_dir = tmp_path_factory.mktemp(f"trainer_monitor_{name}") / "models"
        loop = Loop(name)
        tr = loop.trainer(save_dir)
        assert sorted(tr.objects()) == ["actor", "env", "learner", "memory", "monitor", "schedule"]
        loop.env.reset()
        calls, acted, pending, filled = [], [], [], []
        for _ in range(loop.c["n"]):
            tr.step()
            calls.append(T.call_record(tr))
            acted.append(dict(tr.acted) if tr.acted is not None else None)
            pending.append(tr._recv >= 0)
            filled.append(tr.n_filled)
        _RUNS[name] = dict(calls=calls, acted=acted, pending=pending, filled=filled, final=loop.final(save_dir),
                           saves=list(tr.saves), table=loop.monitor.table(), trainer_state=tr.state_dict())
        loop.close()
    return _RUNS[name]


def _clone(learner):
    return {k: v.detach().clone() for k, v in learner.state_dict().items()}


@pytest.mark.parametrize("name", ["ho", "qo"])
def test_trainer_with_a_monitor_equals_the_serial_loop(name, tmp_path_factory, tmp_path):
    run = trainer_run(name, tmp_path_factory)
    loop = Loop(name, with_schedule=False, with_monitor=False)
    c, env, actor, mem, learner = loop.c, loop.env, loop.actor, loop.mem, loop.learner
    p = c["sched"]
    ref, mref = R.SchedRef(p), M.MonitorRef(MON[name])
    save_dir = tmp_path / "models"
    lr, period = p["lr_init"], p["warm_backup_period"]
    learner.set_lr(lr)
    learner.set_backup_period(period)
    env.reset()
    model = _clone(learner)                          # the model the actor acts on
    steps_done, seen, prev, received, n_files, events = 0, 0, None, None, 0, []
    push_at, perfs = [], []
    for i in range(c["n"]):
        a = actor.act(env.obs, eps=T.eps(steps_done))
        steps_done += loop.B
        obs, reward, done, info = env.step(a)
        nxt = torch.where(done[:, None], info["terminal_obs"], obs) if "terminal_obs" in info else obs
        mem.store_xp(info["last_obs"], nxt, a, reward, info["valid"])
        fr = env.finished_returns
        lens = (torch.cat([n for _, n in fr]) if fr else torch.zeros(0, dtype=torch.float64))[seen:]
        seen += len(lens)
        snap = ref.tick(lens.tolist(), int(info["valid"].sum()), env._fin_cap)
        rec = {"actions": bits(a), "reward": bits(reward), "done": bits(done), "valid": bits(info["valid"])}
        if prev is not None:                       # one tick late, in Trainer's order
            if received is not None:               # the last push's receive, one step late
                ms, outgoing, pushed = received
                received = None
                if ms["rank"] >= 0:
                    os.makedirs(save_dir, exist_ok=True)
                    rank = ms["rank"]
                    for k in range(min(n_files, loop.num_of_saves - 1), rank, -1):
                        os.replace(save_dir / f"{k}.pth", save_dir / f"{k + 1}.pth")
                    torch.save({k: v.cpu() for k, v in outgoing.items()}, save_dir / f"{rank + 1}.pth")
                    events.append("ahead" if rank < n_files else "behind")
                    n_files = ms["n_filled"]
                    # the file is the outgoing model of that push, not the pushed one
                    assert any(not torch.equal(outgoing[k], pushed[k]) for k in outgoing), i
            if prev["lr"] != lr:
                lr = prev["lr"]
                learner.set_lr(lr)
            if prev["backup_period"] != period:
                period = prev["backup_period"]
                learner.set_backup_period(period)
            for j in range(prev["n_updates"]):
                ul = learner.step(mem)
                rec[f"loss{j}"] = bits(ul) if ul is not None else np.zeros(0, np.float32)
            if prev["push"]:
                fp = env.finished_performances
                perfs = torch.cat(fp).tolist() if fp else []
                ms = mref.receive(perfs, env._fin_cap, len(perfs))     # (fewer than fin_cap episodes: no wrap)
                push_at.append(len(perfs))
                outgoing = model
                learner.push(actor)
                model = _clone(learner)
                received = (ms, outgoing, model)
            assert R.snapshot_bits(run["acted"][i]) == R.snapshot_bits(prev), (i, run["acted"][i], prev)
        T.assert_same(rec, run["calls"][i], (name, "call", i))
        assert run["filled"][i] == n_files, (i, run["filled"][i], n_files)
        prev = snap
    print(f"{name}: insertions {events}, table {mref.good}, pushes {ref.hits['push']}")
    print(f"{name}: episodes at the pushes {push_at}, performances {[round(v, 4) for v in perfs]}")
    # what the constants were scaled for: within the run an insertion ahead of a filled entry (files shift) and one
    # behind the filled ones
    assert "ahead" in events and "behind" in events[1:], events
    assert run["saves"] == [f"{k}.pth" for k in range(1, n_files + 1)] == sorted(os.listdir(save_dir))
    T.assert_same(loop.final(save_dir), run["final"], (name, "final"))
    if received is None:       # (a receive still pending at the end has not moved the host's view of the table)
        assert [M.dbits(v) for v in run["table"][0]] == [M.dbits(v) for v in mref.good]
        assert run["table"][1] == mref.filled
    loop.close()


@pytest.mark.parametrize("name", ["ho", "qo"])
def test_checkpoint_and_resume_with_a_receive_still_to_be_acted_on(name, tmp_path_factory, tmp_path):
    run = trainer_run(name, tmp_path_factory)
    P = T._pkg()
    # cut right after a step that pushed: its receive is polled by the first step of the resumed run, which writes
    # a record's file from the checkpoint's stashed model
    cuts = [i + 1 for i in range(len(run["pending"]) - 1) if run["pending"][i]]
    assert cuts, "no push"
    n1 = cuts[len(cuts) // 2]
    save_dir, path = tmp_path / "models", tmp_path / "run.ckpt"
    loop = Loop(name)
    tr = loop.trainer(save_dir)
    loop.env.reset()
    for i in range(n1):
        tr.step()
    assert tr._recv >= 0 and tr._stash is not None
    state = tr.state_dict()
    assert state["monitor_pending"]["call"] == tr._recv and state["n_filled"] == run["filled"][n1 - 1]
    assert all(v.device.type == "cpu" for v in state["monitor_stash"].values())
    P["checkpoint"].save(path, tr.objects(), extra=state)
    loop.close()

    loop = Loop(name)
    tr = loop.trainer(save_dir)
    tr.load_state_dict(P["checkpoint"].load(path, tr.objects()))
    for i in range(n1, loop.c["n"]):
        tr.step()
        T.assert_same(T.call_record(tr), run["calls"][i], (name, "after the cut", i))
        assert tr.n_filled == run["filled"][i], i
    T.assert_same(loop.final(save_dir), run["final"], (name, "final"))
    assert tr.saves == run["saves"] and loop.monitor.table() == run["table"]
    loop.close()


def test_a_plain_trainer_state_has_no_monitor_keys_and_a_mismatch_is_refused(tmp_path):
    loop = Loop("ho", num_of_saves=4)
    with pytest.raises(ValueError, match="num_of_saves is 3, the monitor's 4"):
        loop.trainer(tmp_path / "m", num_of_saves=3)
    loop.monitor.close()
    loop.monitor = None
    tr = loop.trainer(tmp_path / "m")
    assert sorted(tr.objects()) == ["actor", "env", "learner", "memory", "schedule"]
    assert sorted(tr.state_dict()) == sorted(["kind", "steps_done", "tick_index", "acted", "pending", "lr",
                                              "backup_period", "saves"])
    loop.close()


def test_a_trainer_without_a_monitor_writes_the_files_it_wrote_before(tmp_path_factory, tmp_path):
    """HO, the env made with performance_from but no monitor: the files are bitwise those of
    tests/test_gpu_trainer.py's run (no performance, no monitor), written by save_interval."""
    want = T.trainer_run("ho", tmp_path_factory)["final"]
    loop = Loop("ho", with_monitor=False)
    assert loop.num_of_saves == 3                    # (as tests/test_gpu_trainer.py's Trainer)
    tr = loop.trainer(tmp_path / "models")
    loop.env.reset()
    for _ in range(loop.c["n"]):
        tr.step()
    got = loop.final(tmp_path / "models")
    keys = [k for k in want if k.startswith("saves.")]
    assert len(keys) > 1 and keys == [k for k in got if k.startswith("saves.")]
    T.assert_same({k: got[k] for k in keys}, {k: want[k] for k in keys}, "saves")
    for k in want:                                   # and everything else the env shares with that run
        if not k.startswith("env."):
            assert T.same_bits(got[k], want[k]), k
    loop.close()


def test_evaluate_reports_the_performance(tmp_path):
    P = T._pkg()
    loop = Loop("ho")
    tr = loop.trainer(tmp_path / "models")
    env = loop.env
    env.reset()
    for _ in range(10):                             # episodes before the evaluation are not its own
        env.step(loop.actor.act(env.obs, eps=0.05))
    before = sum(len(x) for x in env.finished_performances)
    assert before > 0
    weights = {k: v.clone() for k, v in P["random_direct_dqn"](data_length=int(env.obs.shape[1]), seed=9).items()}
    mean, sem, n = tr.evaluate(weights, 30, path=tmp_path / "1.txt")
    perfs = torch.cat(env.finished_performances)[before:].tolist()
    assert n == len(perfs) >= 30
    ref = M.MonitorRef(dict(MON["ho"], train=0))
    want = ref.receive(perfs, env._fin_cap, len(perfs))
    assert (mean, sem, n) == (want["mean"], want["sem"], want["n"]) and sem > 0
    lens = torch.cat([x for _, x in env.finished_returns]).numpy()
    assert mean != lens[before:].mean()              # (not the episode times)
    assert open(tmp_path / "1.txt").read() == "{} +- {}\n".format(mean, sem)
    assert loop.learner.stats()["updates"] == 0 and len(loop.mem) == 0 and loop.monitor.calls == 0
    loop.close()
