"""Plain-Python restatement of the cooling drivers' model ranking (qc_monitor, include/qcart.h;
worker_manager.receive_net, QO/main_parallel.py:283-329, HO/main_parallel.py:348-388), written from the header
comment: Python floats are IEEE doubles and every operation below is one rounded operation.

TEST INFRASTRUCTURE ONLY: the checker of csrc/qcart_monitor.hpp / qcart_monitor.hip, imported by tests/ only.
"""
from __future__ import annotations

import math
import struct

SNAPSHOT_FIELDS = ("call", "rank", "new_avg", "count", "episode_passed", "n_filled", "total_episodes", "error",
                   "mean", "sem", "n")
SNAP_LINE = "iidiiiiiddi"            # per field: i integer, d a double printed as its bit pattern
ERR_OVERRUN = 1
QO = dict(train=1, window=8, min_count=8, min_episodes=50, num_of_saves=20, initial=6.0)
HO = dict(train=1, window=10, min_count=9, min_episodes=50, num_of_saves=20, initial=20.0)
PARAM_NAMES = ("train", "window", "min_count", "min_episodes", "num_of_saves", "initial")


def params(**kw) -> dict:
    p = dict(QO)
    p.update(kw)
    return p


def window_mean(a) -> float:
    """np.mean's summation order for up to 16 values (numpy's pairwise sum: blocks of 8 from 8 values on)."""
    k = len(a)
    if k < 8:
        res = 0.0
        for v in a:
            res = res + v
    else:
        r = list(a[:8])
        i = 8
        while i + 8 <= k:
            for j in range(8):
                r[j] = r[j] + a[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < k:
            res = res + a[i]
            i += 1
    return res / float(k)


class MonitorRef:
    def __init__(self, p: dict):
        self.p = dict(p)
        n = p["num_of_saves"]
        self.good = [float(p["initial"])] * n
        self.filled = [0] * n
        self.count = self.episode_passed = self.read = self.n = self.calls = self.total_episodes = self.error = 0
        self.sum = self.sumsq = 0.0
        self.hits = dict(below_min_episodes=0, below_min_count=0, refused=0, refused_equal=0, tie_behind=0,
                         rank0_part_filled=0, fell_out=0, inserted=0, overrun=0)

    def receive(self, ring, fin_cap: int, fin_n: int) -> dict:
        """ring: the fin_cap ring entries (entry i at i % fin_cap); fin_n: entries appended so far."""
        p = self.p
        fresh = max(0, fin_n - self.read)
        out = dict(rank=-1, new_avg=0.0, mean=0.0, sem=0.0, n=0)
        if p["train"]:
            self.count = fresh
            self.episode_passed += fresh
            self.total_episodes += fresh
            self.read = fin_n
            if not self.episode_passed > p["min_episodes"]:
                self.hits["below_min_episodes"] += 1
            elif not self.count >= p["min_count"]:
                self.hits["below_min_count"] += 1
            else:
                k = min(self.count, p["window"])
                avg = window_mean([ring[(fin_n - k + j) % fin_cap] for j in range(k)])
                out["new_avg"] = avg
                last = p["num_of_saves"] - 1
                if avg < self.good[last]:
                    rank = sum(1 for v in self.good[:last] if v <= avg)
                    self.hits["tie_behind"] += any(v == avg for v in self.good[:last])
                    self.hits["rank0_part_filled"] += rank == 0 and 0 < sum(self.filled) < len(self.filled)
                    self.hits["fell_out"] += self.filled[last]
                    self.good[rank + 1:] = self.good[rank:last]
                    self.filled[rank + 1:] = self.filled[rank:last]
                    self.good[rank], self.filled[rank] = avg, 1
                    self.episode_passed = 0
                    out["rank"] = rank
                    self.hits["inserted"] += 1
                else:
                    self.hits["refused"] += 1
                    self.hits["refused_equal"] += avg == self.good[last]
            out["count"] = self.count
            self.count = 0
        else:
            if fresh > fin_cap:
                self.error |= ERR_OVERRUN
                self.read = fin_n - fin_cap
                fresh = fin_cap
                self.hits["overrun"] += 1
            for i in range(fresh):
                v = ring[(self.read + i) % fin_cap]
                self.n += 1
                self.sum = self.sum + v
                vv = v * v
                self.sumsq = self.sumsq + vv
            self.read += fresh
            self.total_episodes += fresh
            self.episode_passed += fresh
            self.count = 0
            out["count"] = fresh
            if self.n > 0:
                n = float(self.n)
                out["mean"] = self.sum / n
                if self.n > 1:
                    sm = self.sum * out["mean"]
                    var = (self.sumsq - sm) / (n - 1.0)
                    if var < 0.0:
                        var = 0.0
                    out["sem"] = math.sqrt(var) / math.sqrt(n)
            out["n"] = self.n
        out["call"] = self.calls
        self.calls += 1
        out.update(episode_passed=self.episode_passed, n_filled=sum(self.filled), total_episodes=self.total_episodes,
                   error=self.error)
        return out


def dbits(v: float) -> int:
    return struct.unpack("<q", struct.pack("<d", float(v)))[0]


def snapshot_bits(s: dict) -> tuple:
    return tuple(dbits(s[k]) if f == "d" else int(s[k]) for k, f in zip(SNAPSHOT_FIELDS, SNAP_LINE))


def script_text(p: dict, fin_cap: int, receives) -> str:
    """The script tests/diag/monitor_check.cpp reads: receives is a list of lists of performances appended to the
    ring before each receive."""
    lines = ["P " + " ".join(str(int(p[k])) for k in PARAM_NAMES[:-1]) + " " + float(p["initial"]).hex(),
             f"C {fin_cap}"]
    for vals in receives:
        lines.append(f"T {len(vals)} " + " ".join(float(v).hex() for v in vals))
    return "\n".join(lines) + "\n"


def run_script(p: dict, fin_cap: int, receives):
    """The script through the restatement: (snapshots, tables after every receive, the MonitorRef)."""
    ref = MonitorRef(p)
    ring, fin_n, snaps, tables = [0.0] * fin_cap, 0, [], []
    for vals in receives:
        for v in vals:
            ring[fin_n % fin_cap] = float(v)
            fin_n += 1
        snaps.append(ref.receive(ring, fin_cap, fin_n))
        tables.append((list(ref.good), list(ref.filled)))
    return snaps, tables, ref


def _vals(rng, n, lo, hi):
    return [lo + (hi - lo) * rng.random() for _ in range(n)]


def scripts() -> dict:
    """name -> (params, fin_cap, receives). Together they reach 0 / 1 / 7 / 8 / 9 / 10 / 11 / 200 fresh entries,
    episode_passed exactly at min_episodes and one above, a candidate equal to good[last] (refused), a tie with an
    earlier entry (ranked behind it), rank 0 into a part-filled table, the table filling and an entry falling out,
    and the train == 0 sums with a single episode and an overrun."""
    import random
    rng = random.Random(7)
    out = {}
    # QO's rule with a table of 3: window 8, min_count 8, min_episodes 50
    p = params(num_of_saves=3, initial=6.0)
    r = []
    r.append(_vals(rng, 42, 3.0, 5.0))      # episode_passed 42: below min_episodes
    r.append(_vals(rng, 8, 3.0, 5.0))       # 50: exactly at min_episodes, the test is strict
    r.append([])                            # 0 fresh
    r.append([4.0])                         # 51 > 50 but count 1 < 8
    r.append(_vals(rng, 7, 3.0, 5.0))       # count 7 < 8
    r.append([4.0] * 8)                     # 66 passed, count 8: mean 4.0 < 6.0 -> rank 0, table [4, 6, 6]
    r.append(_vals(rng, 50, 1.0, 2.0))      # episode_passed back at 50: not > 50
    r.append([6.0] * 9)                     # 59, count 9: the mean of the last 8 is 6.0 == good[last]: refused
    r.append([4.0] * 10)                    # count 10: mean 4.0 ties entry 0: rank 1 (behind), table [4, 4, 6]
    r.append(_vals(rng, 40, 1.0, 2.0))
    r.append([3.0] * 11)                    # 51, count 11: mean 3.0 -> rank 0 into a part-filled table [3, 4, 4]: full
    r.append(_vals(rng, 200, 5.0, 9.0))     # 200 fresh (more than the ring of 128): mean > good[last]: refused
    r.append([3.5] * 8)                     # rank 1: [3, 3.5, 4], a filled entry falls out
    r.append(_vals(rng, 60, 0.5, 0.75))     # rank 0 with random values: [x, 3, 3.5]
    out["quartic"] = (p, 128, r)
    # HO's rule: window 10, min_count 9, random performances, a table of 4
    p = params(window=10, min_count=9, num_of_saves=4, initial=20.0, min_episodes=5)
    r = [_vals(rng, n, 0.0, 25.0) for n in (3, 9, 10, 11, 8, 9, 16, 0, 1, 7, 12, 9, 10, 33, 9, 9, 10)]
    out["harmonic"] = (p, 32, r)
    # window 16: numpy's two blocks of 8
    p = params(window=16, min_count=1, num_of_saves=64, initial=10.0, min_episodes=0)
    r = [_vals(rng, n, 0.0, 9.0) for n in list(range(1, 20)) + [16] * 70]
    out["window16"] = (p, 16, r)
    # train == 0: a single episode (sem 0), more, 0 fresh, and an overrun of the ring of 20
    p = params(train=0)
    r = [[2.5], _vals(rng, 7, 0.0, 3.0), [], _vals(rng, 19, 0.0, 3.0), _vals(rng, 45, 0.0, 3.0), _vals(rng, 20, 0.0, 3.0)]
    out["test_mode"] = (p, 20, r)
    return out
