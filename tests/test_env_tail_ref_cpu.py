"""CPU checks of tests/env_tail_ref.py (the checker of qc_env_tail) on hand-written envs: pending and not
pending, Fail / out of bounds / both / neither, the first-interval episode (return 0, length interval dt), the
strict |x| > xth bound, IQO's term_step, the ring order, its wrap and the untouched sink slots."""
import numpy as np

from tests.env_tail_ref import IHO, IQO, env_tail_ref


def _call(kind, pending, fail, x, term, t, steps, ret, fin, fin_cap, fin_n, xth=8.0):
    obs = np.zeros((len(x), 5))
    obs[:, 0] = x
    obs[:, 1] = 0.25
    return env_tail_ref(kind, 80, 1 / 1440, xth, 0.7, -1.0, np.array(fail, np.int32), np.array(term, np.int32), obs,
                        np.array(pending, np.uint8), np.array(t, np.float64), np.array(steps, np.int64),
                        np.array(ret, np.float64), fin, fin_cap, fin_n)


def test_hand_written_envs():
    ci_dt = 80 * (1 / 1440)
    #          0: alive   1: fail  2: oob   3: both  4: at xth  5: pending alive  6: pending, over (first interval)
    pending = [0,         0,       0,       0,       0,         1,                1]
    fail    = [0,         17,      0,       3,       0,         0,                0]
    x       = [0.5,       0.1,     -8.5,    9.0,     -8.0,      0.2,              8.000001]
    t       = [1.0,       2.0,     3.0,     4.0,     5.0,       6.0,              7.0]
    steps   = [80,        160,     240,     320,     400,       480,              560]
    ret     = [3.0,       4.0,     5.0,     6.0,     7.0,       8.0,              9.0]
    fin = np.full((2, 5), -7.0)
    o = _call(IHO, pending, fail, x, [-1] * 7, t, steps, ret, fin, 4, 2)
    assert list(o["done"]) == [0, 1, 1, 1, 0, 0, 1] and list(o["pending"]) == list(o["done"])
    assert list(o["valid"]) == [1, 1, 1, 1, 1, 0, 0]
    assert list(o["reward"]) == [1, -1, -1, -1, 1, 0, 0] and o["reward"].dtype == np.float32
    assert list(o["episode_return"]) == [4.0, 3.0, 4.0, 5.0, 8.0, 0.0, 0.0]
    assert list(o["t"]) == [1.0 + ci_dt, 2.0 + ci_dt, 3.0 + ci_dt, 4.0 + ci_dt, 5.0 + ci_dt, ci_dt, ci_dt]
    assert list(o["steps"]) == [160, 240, 320, 400, 480, 80, 80]
    # envs 1, 2, 3, 6 finish, from fin_n = 2 into a ring of 4: slots 2, 3, 0, 1 in env order; the sinks keep -7
    assert o["fin_n"] == 6
    assert list(o["fin"][0]) == [5.0, 0.0, 3.0, 4.0, -7.0]
    assert list(o["fin"][1]) == [4.0 + ci_dt, ci_dt, 2.0 + ci_dt, 3.0 + ci_dt, -7.0]
    assert o["obs32"].dtype == np.float32
    assert o["obs32"][2, 0] == np.float32(-8.5) * np.float32(0.7) and o["obs32"][0, 1] == np.float32(0.25) * np.float32(0.7)
    assert (fin == -7.0).all()   # the inputs are not modified


def test_inverted_quartic_uses_term_step():
    fin = np.zeros((2, 9))
    # |x| beyond xth does not end an IQO episode; term_step >= 0 (step 0 included) or Fail does
    o = _call(IQO, [0, 0, 0, 1], [0, 0, 2, 0], [99.0, 0.0, 0.0, 0.0], [-1, 0, -1, 5], [1.0] * 4, [80] * 4, [2.0] * 4,
              fin, 8, 0, xth=1.0)
    assert list(o["done"]) == [0, 1, 1, 1] and o["fin_n"] == 3
    assert list(o["fin"][0][:3]) == [1.0, 1.0, 0.0]
    assert list(o["fin"][1][:3]) == [1.0 + 80 / 1440, 1.0 + 80 / 1440, 80 * (1 / 1440)]


def test_nothing_finishes():
    fin = np.arange(6.0).reshape(2, 3)
    o = _call(IHO, [0, 1], [0, 0], [0.0, 0.0], [-1, -1], [1.0, 1.0], [80, 80], [1.0, 1.0], fin, 2, 7)
    assert o["fin_n"] == 7 and np.array_equal(o["fin"], fin) and not o["done"].any()
