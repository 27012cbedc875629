"""The training schedule's tick (qc_sched_tick, include/qcart.h) restated in plain Python: the same params and
snapshot, Python floats, one operation per rounding. Test infrastructure only.

Each branch cites the reference line it restates (IHO = inverted harmonic oscillator, HO = harmonic oscillator:
RL.py is the loader loop, main_parallel.py is Main_System) and counts itself in `hits`, so a test can assert that its
script reached it."""
import math
from collections import Counter

CARTPOLE, COOLING = 0, 1
ERR_OVERRUN = 1
SNAPSHOT_FIELDS = ("tick", "n_updates", "push", "save", "stop", "learning", "lr", "backup_period", "episode",
                   "last_achieved", "t_done", "pending", "actor_update_time", "total_episodes", "total_rows", "error",
                   "mean", "sem", "n")
# the four rungs of IHO/main_parallel.py:532-542 as (achieved above, actor_update_time at most, new time)
IHO_RUNGS = ((50., 150., 800.), (20., 50., 150.), (10., 25., 50.), (5., 10., 25.))


def params(**kw) -> dict:
    """A params dict with the inverted harmonic driver's values where `kw` names none."""
    p = dict(rule=CARTPOLE, train=1, start_time=20., fall_time=5., t_full=0., first_interval_time=0., fail_limit=10,
             batch_size=512, n_times_per_sample=8., max_updates_per_tick=8, min_rows=0, num_episodes=20000,
             give_up_episodes=50000, lr_init=4e-4, lr_cap=4e-4,
             lr_schedule=((6000, 8e-5), (11000, 2e-5), (15000, 4e-6), (17000, 8e-7), (19000, 2e-7), (21000, 0.)),
             backup_period=300, warm_backup_period=100, save_interval=200, actor_update_time=10., rungs=IHO_RUNGS)
    unknown = set(kw) - set(p)
    assert not unknown, unknown
    p.update(kw)
    return p


class SchedRef:
    def __init__(self, p: dict):
        self.p = dict(p)
        self.pending = 0.
        self.t_done = 0.
        self.last_achieved = 0.
        self.actor_update_time = float(p["actor_update_time"])
        self.lr = float(p["lr_init"])
        self.simulated = 0.
        self.sum = self.sumsq = 0.
        self.episode = self.total_episodes = self.total_rows = 0
        self.read = 0
        self.episodes_since_save = 0
        self.n_test = 0
        self.ticks = 0
        self.learning = self.switched = self.started = 0
        self.failure_counter = 0
        self.lr_step = 0
        self.error = 0
        self.hits = Counter()
        self._last_lr_tick = -2

    def _episode(self, t: float):
        p, hit = self.p, self.hits
        self.episode += 1                                  # RL.py:502
        self.total_episodes += 1
        self.read += 1
        if not p["train"]:                                 # IHO/RL.py:505
            hit["train0"] += 1
            self.learning = 1
            self.n_test += 1
            self.sum = self.sum + t
            tt = t * t
            self.sumsq = self.sumsq + tt
        if p["rule"] == COOLING and p["train"] and not self.learning and t <= 1.5 * p["first_interval_time"]:
            hit["zero_sample"] += 1                        # HO/RL.py:499
            self.learning = 1
        self.t_done = self.t_done + t                      # RL.py:516
        half = t / 2.
        self.simulated = self.simulated + half             # main_parallel.py:385
        if not p["train"]:
            return
        if p["rule"] == CARTPOLE:
            a, b = self.last_achieved * 0.98, 0.02 * t
            self.last_achieved = a + b                     # IHO/RL.py:523
            if self.last_achieved >= p["start_time"] and not self.learning:     # :525-529
                hit["cartpole_restart" if hit["cartpole_start"] else "cartpole_start"] += 1
                self.learning = 1
                self.episode = 1
            elif self.learning and self.last_achieved < p["fall_time"]:         # :532-534
                hit["cartpole_fall"] += 1
                self.learning = 0
        else:
            full, last_full = t >= p["t_full"], self.last_achieved >= p["t_full"]
            if not last_full:                              # HO/RL.py:517
                if self.last_achieved < t:
                    if not full:                           # :520
                        hit["cooling_better"] += 1
                        self.last_achieved = t
                    else:                                  # :522-526
                        hit["cooling_first_full"] += 1
                        self.episode = 1
                        self.failure_counter = 0
                        self.last_achieved = t
                        self.learning = 1
            elif not full:                                 # :527-532
                self.failure_counter += 1
                hit["cooling_failure"] += 1
                if self.failure_counter == p["fail_limit"]:
                    hit["cooling_fail_limit"] += 1
                    self.last_achieved = t
                    self.learning = 0
            elif self.failure_counter != 0:                # :533
                if self.failure_counter == p["fail_limit"] - 1:
                    hit["cooling_reset_at_limit_minus_one"] += 1
                hit["cooling_counter_reset"] += 1
                self.failure_counter = 0

    def tick(self, new_lengths, rows: int, fin_cap=None) -> dict:
        """One tick: `rows` rows stored by this call; `new_lengths`: the episode times appended to the ring since
        the last tick, in ring order (with fin_cap and more than fin_cap of them, the ring was overrun: only the
        last fin_cap are still there)."""
        p, hit = self.p, self.hits
        # 1. rows (RL.py:518, credited per call)
        self.total_rows += rows
        due = float(rows) * 8. / 256.
        self.pending = self.pending + due
        # 2. the walk
        new_lengths = [float(t) for t in new_lengths]
        if fin_cap is not None and len(new_lengths) > fin_cap:
            hit["overrun"] += 1
            self.error |= ERR_OVERRUN
            self.read += len(new_lengths) - fin_cap
            new_lengths = new_lengths[-fin_cap:]
        for t in new_lengths:
            self._episode(t)
        # 3. Main_System.__call__ (IHO/main_parallel.py:490-503)
        n_updates = 0
        if p["train"] and self.total_rows < p["min_rows"] and self.pending > 0.:
            hit["min_rows_hold"] += 1
        if p["train"] and self.total_rows >= p["min_rows"]:
            d0, d1 = 8. / p["n_times_per_sample"], float(p["batch_size"]) / 256.
            D = d0 * d1
            q = self.pending / D
            want = math.floor(q)
            n = float(min(want, p["max_updates_per_tick"]))
            if n >= 1.:
                if want > p["max_updates_per_tick"]:
                    hit["updates_capped"] += 1
                n_updates = int(n)
                spent = n * D
                self.pending = self.pending - spent
                self.started = 1
        push = 0
        if self.t_done >= self.actor_update_time:          # :511-517
            for i, (ach, below, new) in enumerate(p["rungs"]):     # :532-542
                if self.last_achieved > ach and self.actor_update_time <= below:
                    hit[f"rung{i}"] += 1
                    self.actor_update_time = float(new)
                    break
            if self.started:
                hit["push"] += 1
                push = 1
                self.t_done = 0.
            else:
                hit["push_not_started"] += 1
        if not self.switched and self.learning:            # :546-552
            hit["backup_switch"] += 1
            self.switched = 1
            if p["lr_cap"] < self.lr:
                hit["lr_cap"] += 1
                self.lr = float(p["lr_cap"])
        sch = p["lr_schedule"]
        if self.lr_step < len(sch) and self.learning and self.episode > sch[self.lr_step][0]:   # :553-558
            hit["lr_step"] += 1
            if self._last_lr_tick == self.ticks - 1:
                hit["lr_steps_consecutive"] += 1
            self._last_lr_tick = self.ticks
            if sch[self.lr_step][1] < self.lr:
                self.lr = float(sch[self.lr_step][1])
            self.lr_step += 1
        self.episodes_since_save += len(new_lengths)       # :386-395
        save = 0
        if push and self.episodes_since_save >= p["save_interval"]:
            hit["save"] += 1
            save = 1
            self.episodes_since_save = 0
        elif self.episodes_since_save >= p["save_interval"]:
            hit["save_waits_for_push"] += 1
        go_on = self.episode < p["num_episodes"] or (self.episode < p["give_up_episodes"] and not self.learning)   # :492
        if not go_on:
            hit["stop_done" if self.episode >= p["num_episodes"] and self.learning else "stop_give_up"] += 1
        mean = sem = 0.
        if self.n_test > 0:                                # main_parallel.py:445
            n = float(self.n_test)
            mean = self.sum / n
            if self.n_test > 1:
                sm = self.sum * mean
                dev, n1 = self.sumsq - sm, n - 1.
                var = dev / n1
                if var < 0.:
                    var = 0.
                sem = math.sqrt(var) / math.sqrt(n)
        snap = dict(tick=self.ticks, n_updates=n_updates, push=push, save=save, stop=int(not go_on),
                    learning=self.learning, lr=self.lr,
                    backup_period=p["backup_period"] if self.switched else p["warm_backup_period"],
                    episode=self.episode, last_achieved=self.last_achieved, t_done=self.t_done, pending=self.pending,
                    actor_update_time=self.actor_update_time, total_episodes=self.total_episodes,
                    total_rows=self.total_rows, error=self.error, mean=mean, sem=sem, n=self.n_test)
        self.ticks += 1
        return snap


# ---- scripted tick sequences shared by the CPU and the GPU tests: (params, fin_cap, [(rows, lengths), ...]) ----
# the inverted harmonic driver's constants divided by 10 (times) so that a few hundred short episodes reach every rung
SCALED_RUNGS = ((5., 15., 80.), (2., 5., 15.), (1., 2.5, 5.), (0.5, 1., 2.5))
SNAP_LINE = ("q", "q", "i", "i", "i", "i", "d", "q", "q", "d", "d", "d", "d", "q", "q", "q", "d", "d", "q")


def scripts() -> dict:
    out = {}
    # cartpole: min_rows holds the first updates back (a push falls due before any update: no push), start with the lr
    # cap and the period switch, two lr steps on consecutive ticks, every rung, a save only on a push tick, 37 rows a
    # tick against D = 0.5 and two updates a tick (the remainder grows until the cap binds), a fall, a restart, and
    # the stop at num_episodes
    p = params(start_time=2., fall_time=0.5, rungs=SCALED_RUNGS, actor_update_time=1., lr_init=1e-3, lr_cap=4e-4,
               lr_schedule=((3, 8e-5), (4, 2e-5), (30, 4e-6)), backup_period=3, warm_backup_period=100, save_interval=5,
               num_episodes=40, give_up_episodes=1000, max_updates_per_tick=2, min_rows=50, batch_size=128)
    ticks = [(37, [1.5])]
    ticks += [(37, [30.25 + 0.125 * i]) for i in range(6)]           # the EMA passes 0.5, 1 and 2 (start): three rungs
    ticks += [(37, [29.5] * 6), (37, []), (37, [31.] * 2)]           # episode passes 3 and 4: two lr steps
    ticks += [(37, [30.] * 2) for _ in range(8)]                     # the EMA passes 5: the last rung
    ticks += [(0, [0.0625] * 200), (3, [0.0625] * 100)]              # the EMA falls below 0.5
    ticks += [(37, [33.] * 3) for _ in range(3)]                     # restart, episode = 1 again
    ticks += [(37, [33.] * 7) for _ in range(7)]                     # until num_episodes
    out["cartpole"] = (p, 256, ticks)
    # cartpole that never starts: the give-up stop
    p = params(start_time=2., fall_time=0.5, rungs=SCALED_RUNGS, actor_update_time=1., num_episodes=10,
               give_up_episodes=30, batch_size=128)
    out["give_up"] = (p, 128, [(16, [0.25] * 7) for _ in range(6)])
    # cooling: an episode without a row, better and better times, the first full episode, nine failures then a
    # success, fail_limit failures, a full episode again
    p = params(rule=COOLING, t_full=9.99, fail_limit=10, first_interval_time=0.2, start_time=0., fall_time=0.,
               rungs=SCALED_RUNGS, actor_update_time=1., lr_init=4e-4, lr_schedule=((5, 4e-5), (200, 8e-6)),
               backup_period=4, save_interval=8, num_episodes=60, give_up_episodes=400, max_updates_per_tick=3,
               batch_size=128, min_rows=0)
    ticks = [(16, [0.25]), (16, [3., 2., 5.]), (16, [10.]), (16, [4.] * 9), (16, [10., 10.]), (16, [4.5] * 6),
             (16, [4.5] * 4), (16, [6.]), (16, [10.] * 3)]
    ticks += [(16, [10.] * 8) for _ in range(8)]
    out["cooling"] = (p, 128, ticks)
    # the --test accounting
    p = params(train=0, start_time=2., fall_time=0.5, rungs=SCALED_RUNGS, actor_update_time=1., batch_size=128,
               num_episodes=12, give_up_episodes=12)
    out["test_mode"] = (p, 128, [(16, []), (16, [3.5]), (16, [1.25, 7.75]), (16, [0.1 * i for i in range(1, 12)])])
    return out


def script_text(p: dict, fin_cap: int, ticks) -> str:
    """The script tests/diag/sched_check.cpp reads; doubles as C99 hex."""
    h = lambda v: float(v).hex()   # noqa: E731
    lines = [" ".join(["P", str(p["rule"]), str(p["train"]), h(p["start_time"]), h(p["fall_time"]), h(p["t_full"]),
                       h(p["first_interval_time"]), str(p["fail_limit"]), str(p["batch_size"]),
                       h(p["n_times_per_sample"]), str(p["max_updates_per_tick"]), str(p["min_rows"]),
                       str(p["num_episodes"]), str(p["give_up_episodes"]), h(p["lr_init"]), h(p["lr_cap"]),
                       str(p["backup_period"]), str(p["warm_backup_period"]), str(p["save_interval"]),
                       h(p["actor_update_time"])])]
    lines.append(" ".join(["L", str(len(p["lr_schedule"]))] + [w for e, v in p["lr_schedule"] for w in (str(e), h(v))]))
    lines.append(" ".join(["R", str(len(p["rungs"]))] + [h(v) for r in p["rungs"] for v in r]))
    lines.append(f"C {fin_cap}")
    for rows, ts in ticks:
        lines.append(" ".join(["T", str(rows), str(len(ts))] + [h(t) for t in ts]))
    return "\n".join(lines) + "\n"


def snapshot_bits(snap: dict) -> tuple:
    """A snapshot as a tuple of ints: integers as they are, doubles as their bit patterns."""
    import struct
    return tuple(struct.unpack("<q", struct.pack("<d", float(snap[k])))[0] if f == "d" else int(snap[k])
                 for k, f in zip(SNAPSHOT_FIELDS, SNAP_LINE))
