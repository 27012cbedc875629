"""CPU checks of tests/env_tail_cooling_ref.py (the checker of qc_env_tail's cooling branch) on hand-written envs:
pending and not pending, the phonon number exactly at the cutoff (not over) and one ulp above it, a NaN phonon
number in both branches, an episode time exactly at t_trunc (truncated) and one ulp below it, Fail only, the
unfused product and sum of the return, the record mode, the ring order, its wrap and the untouched sink slots."""
import numpy as np

from tests.env_tail_cooling_ref import env_tail_cooling_ref

CI, DT = 36, 1 / 1440
CI_DT = np.float64(CI) * np.float64(DT)
CUT = 20.0
UP = np.nextafter(CUT, np.inf)


def _call(pending, fail, q, t, steps, ret, fin, fin_cap, fin_n, t_trunc=100.0 - 0.01 * DT, rm=0.5):
    obs = np.zeros((len(q), 5))
    obs[:, 1] = 0.25
    return env_tail_cooling_ref(CI, DT, 0.7, CUT, t_trunc, rm, np.array(fail, np.int32), np.array(q, np.float64),
                                obs, np.array(pending, np.uint8), np.array(t, np.float64),
                                np.array(steps, np.int64), np.array(ret, np.float64), fin, fin_cap, fin_n)


def test_hand_written_envs():
    nan = float("nan")
    #          0: alive  1: at cutoff  2: ulp above  3: NaN   4: fail only  5: pend alive  6: pend ulp above
    #          7: pend NaN (not over)  8: pend fail  9: pend at cutoff
    pending = [0,        0,            0,            0,       0,            1,             1,  1,   1,   1]
    fail    = [0,        0,            0,            0,       7,            0,             0,  0,   3,   0]
    q       = [1.5,      CUT,          UP,           nan,     0.25,         0.5,           UP, nan, 0.1, CUT]
    t       = [1.0,      2.0,          3.0,          4.0,     5.0,          6.0,           7.0, 8.0, 9.0, 10.0]
    steps   = [36,       72,           108,          144,     180,          216,           252, 288, 324, 360]
    ret     = [-3.0,     -4.0,         -5.0,         -6.0,    -7.0,         -8.0,          -9.0, -1.0, -2.0, -3.0]
    fin = np.full((2, 5), -7.0)
    o = _call(pending, fail, q, t, steps, ret, fin, 4, 2)
    assert list(o["done"]) == [0, 0, 1, 1, 1, 0, 1, 0, 1, 0] and list(o["pending"]) == list(o["done"])
    assert list(o["valid"]) == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert list(o["rec_mode"]) == [1, 1, 1, 1, 1, 2, 2, 2, 2, 2]
    rw = o["reward"]
    assert rw.dtype == np.float32
    assert list(rw[:3]) == [np.float32(-0.75), np.float32(-10.0), np.float32(-UP * 0.5)]
    assert np.isnan(rw[3]) and rw[4] == np.float32(-0.125) and list(rw[5:]) == [0.0] * 5
    # the terminal transition adds nothing to the return; a reset interval restarts it at 0
    assert list(o["episode_return"]) == [-3.75, -14.0, -5.0, -6.0, -7.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert list(o["t"]) == [x + CI_DT for x in t[:5]] + [CI_DT] * 5
    assert list(o["steps"]) == [72, 108, 144, 180, 216, 36, 36, 36, 36, 36]
    # envs 2, 3, 4, 6, 8 finish, from fin_n = 2 into a ring of 4: slots 2, 3, 0, 1, 2 in env order (env 8
    # overwrites env 2's entry); the sinks keep -7
    assert o["fin_n"] == 7
    assert list(o["fin"][0]) == [-7.0, 0.0, 0.0, -6.0, -7.0]
    assert list(o["fin"][1]) == [5.0 + CI_DT, CI_DT, CI_DT, 4.0 + CI_DT, -7.0]
    assert o["obs32"].dtype == np.float32 and o["obs32"][0, 1] == np.float32(0.25) * np.float32(0.7)
    assert (fin == -7.0).all()   # the inputs are not modified


def test_truncation_is_at_or_after_t_trunc_and_not_in_the_reset_interval():
    t0 = 11.0
    t_trunc = np.float64(t0) + CI_DT
    fin = np.zeros((2, 9))
    # 0: t' == t_trunc exactly: truncated; 1: one ulp below: not; 2: pending with a late t: restarted, not truncated
    o = _call([0, 0, 1], [0, 0, 0], [1.0, 1.0, 1.0], [t0, np.nextafter(t0, 0.0), 99.0], [36] * 3, [-2.0] * 3, fin, 8, 0,
              t_trunc=t_trunc)
    assert o["t"][0] == t_trunc and o["t"][1] < t_trunc
    assert list(o["done"]) == [1, 0, 0] and list(o["valid"]) == [0, 1, 0]
    assert list(o["episode_return"]) == [-2.0, -2.5, 0.0]
    assert o["fin_n"] == 1 and o["fin"][0, 0] == -2.0 and o["fin"][1, 0] == t_trunc


def test_return_rounds_the_product_and_the_sum_separately():
    # q * rm = (1 + 2^-30)^2 = 1 + 2^-29 + 2^-60 rounds to 1 + 2^-29; a fused multiply-add against -1 would
    # keep the 2^-60
    x = 1.0 + 2.0 ** -30
    fin = np.zeros((2, 3))
    o = _call([0], [0], [x], [1.0], [36], [1.0 + 2.0 ** -29], fin, 2, 0, rm=x)
    assert o["episode_return"][0] == 0.0 and o["valid"][0] == 1


def test_nothing_finishes():
    fin = np.arange(6.0).reshape(2, 3)
    o = _call([0, 1], [0, 0], [0.0, 0.0], [1.0, 1.0], [36, 36], [-1.0, -1.0], fin, 2, 7)
    assert o["fin_n"] == 7 and np.array_equal(o["fin"], fin) and not o["done"].any()
