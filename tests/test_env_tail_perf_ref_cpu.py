"""CPU checks of tests/env_tail_perf_ref.py (the checker of qc_env_tail's per-episode performance) on hand-written
envs: the threshold crossed in the middle of an episode (the step exactly at it is not counted, the next one is),
an episode truncated with counted steps and one with none, a failed episode (the cutoff), an episode that fails in
the call in which its time reaches t_trunc (t_trunc wins: the mean), a NaN quantity, HO's pending first control
step, QO going live (which only zeroes), a warming QO env (untouched), the draw kernel, the ring position and the
sink; and that the wrapped restatements' own outputs are unchanged."""
import numpy as np

from tests.env_tail_cooling_ref import env_tail_cooling_ref
from tests.env_tail_perf_ref import (env_tail_cooling_perf_ref, env_tail_warmup_perf_ref, env_warmup_draw_perf_ref,
                                     new_perf)
from tests.env_tail_warmup_ref import env_tail_warmup_ref, new_state

CI, DT = 36, 1 / 1440
CI_DT = np.float64(CI) * np.float64(DT)
CUT = 20.0
NAN = float("nan")


def _ho(pending, fail, q, t, p, perf_from, fin_cap=4, fin_n=2, t_trunc=100.0 - 0.01 * DT):
    B = len(q)
    obs = np.zeros((B, 5))
    args = (CI, DT, 0.7, CUT, t_trunc, 0.5, np.array(fail, np.int32), np.array(q, np.float64), obs,
            np.array(pending, np.uint8), np.array(t, np.float64), np.full(B, 36, np.int64), np.full(B, -2.0),
            np.full((2, fin_cap + 1), -7.0), fin_cap, fin_n)
    o = env_tail_cooling_perf_ref(*args, p, perf_from)
    base = env_tail_cooling_ref(*args)
    for k, v in base.items():   # the wrapped restatement's outputs stay as they are
        assert np.array_equal(np.asarray(o[k]), np.asarray(v), equal_nan=True), k
    return o


def _p(perf_sum, perf_n, fin_cap=4):
    p = new_perf(len(perf_sum), fin_cap, fill=-9.0)
    p["perf_sum"][:] = perf_sum
    p["perf_n"][:] = perf_n
    return p


def test_threshold_is_strict_and_crossed_mid_episode():
    # one env through three calls, perf_from exactly the time after the second: counted in the third only
    pf = np.float64(1.0) + CI_DT + CI_DT
    p = _p([0.0], [0])
    t = np.float64(1.0)
    for call, (q, want_sum, want_n) in enumerate([(1.5, 0.0, 0), (2.5, 0.0, 0), (0.1, 0.1, 1)]):
        o = _ho([0], [0], [q], [t], p, pf)
        assert o["done"][0] == 0 and o["perf_sum"][0] == want_sum and o["perf_n"][0] == want_n, call
        assert (o["perf"] == -9.0).all()
        p, t = o, o["t"][0]
    assert t > pf


def test_harmonic_hand_written_envs():
    t0 = 11.0
    t_trunc = np.float64(t0) + CI_DT
    x = 0.1 + 0.2            # the sum rounds once: 0.30000000000000004 + 0.7 in float64
    #          0: truncated, counted  1: truncated, none counted  2: over the cutoff  3: Fail and t_trunc at once
    #          4: NaN (ends, not truncated)  5: alive, counted  6: pending alive past perf_from  7: pending over
    #          8: alive, its first counted step  9: Fail before t_trunc
    pending = [0,    0,    0,    0,    0,    0,    1,    1,    0,    0]
    fail =    [0,    0,    0,    4,    0,    0,    0,    0,    0,    2]
    q =       [5.0,  5.0,  21.0, 1.0,  NAN,  0.7,  0.25, 30.0, 0.7,  0.5]
    t =       [t0,   t0,   3.0,  t0,   3.0,  3.0,  9.0,  9.0,  3.0,  3.0]
    psum =    [9.0,  0.0,  4.0,  7.0,  4.0,  x,    55.0, 55.0, 0.0,  6.0]
    pn =      [4,    0,    2,    2,    2,    2,    9,    9,    0,    3]
    o = _ho(pending, fail, q, t, _p(psum, pn, 8), 0.01, fin_cap=8, fin_n=6, t_trunc=t_trunc)
    assert list(o["done"]) == [1, 1, 1, 1, 1, 0, 0, 1, 0, 1]
    # a terminal step adds nothing; the pending branch restarts the sums and its first control step counts
    assert list(o["perf_sum"]) == [9.0, 0.0, 4.0, 7.0, 4.0, x + 0.7, 0.25, 0.0, 0.7, 6.0]
    assert o["perf_sum"][5] == np.float64(x) + np.float64(0.7)
    assert list(o["perf_n"]) == [4, 0, 2, 2, 2, 3, 1, 0, 1, 3]
    # finished: envs 0 1 2 3 4 7 9 from fin_n = 6 into a ring of 8: slots 6 7 0 1 2 3 4
    assert o["fin_n"] == 13
    want = {6: 9.0 / 4, 7: CUT, 0: CUT, 1: 7.0 / 2, 2: CUT, 3: CUT, 4: CUT}
    for slot in range(9):
        assert o["perf"][slot] == want.get(slot, -9.0), slot
    assert o["perf"][8] == -9.0     # the sink
    # the same ring positions as (return, length)
    assert o["fin"][1, 6] == t_trunc and o["fin"][1, 3] == CI_DT


def test_harmonic_pending_first_step_before_the_threshold_is_not_counted():
    o = _ho([1, 1], [0, 0], [0.25, 0.5], [9.0, 9.0], _p([3.0, 3.0], [2, 2]), CI_DT)   # t' == perf_from: strict
    assert list(o["perf_sum"]) == [0.0, 0.0] and list(o["perf_n"]) == [0, 0]
    o = _ho([1], [0], [0.25], [9.0], _p([3.0], [2]), np.nextafter(CI_DT, 0.0))
    assert list(o["perf_sum"]) == [0.25] and list(o["perf_n"]) == [1]


# ------------------------------------------------------------------ QO with the rolling warm-up
QCI = 80
QCI_DT = np.float64(QCI) * np.float64(DT)
QCUT, INIT_CUT, LO, HI, SEED, OFF = 12.0, 2.0, 0.2, 0.5, 3, 40


def _qo_state(warm_left, budget, t, psum, pn, fin_cap=4, fin_n=3):
    B = len(warm_left)
    s = new_state(B, QCI, fin_cap)
    s.update(warm_left=np.array(warm_left, np.int32), budget=np.array(budget, np.int32), t=np.array(t, np.float64),
             episode_return=np.full(B, -3.0), draws=np.arange(1, B + 1, dtype=np.int64),
             fin=np.full((2, fin_cap + 1), -7.0), fin_n=fin_n)
    s.update(new_perf(B, fin_cap, fill=-9.0))
    s["perf_sum"][:] = psum
    s["perf_n"][:] = pn
    return s


def _qo(s, fail, q, perf_from, t_trunc):
    obs = np.zeros((len(q), 5))
    args = (QCI, DT, 0.7, QCUT, t_trunc, 0.5, INIT_CUT, LO, HI, SEED, OFF, np.array(fail, np.int32),
            np.array(q, np.float64), obs)
    o = env_tail_warmup_perf_ref(s, *args, perf_from)
    base = env_tail_warmup_ref(s, *args)
    for k, v in base.items():
        assert np.array_equal(np.asarray(o[k]), np.asarray(v), equal_nan=True), k
    return o


def test_quartic_hand_written_envs():
    t0 = 50.0
    t_trunc = np.float64(t0) + QCI_DT
    #            0: warming  1: goes live  2: rejected  3: live counted  4: live before  5: truncated  6: energy bound
    #            7: Fail at t_trunc  8: live NaN  9: truncated, nothing counted
    warm_left = [200,  37,   37,   0,    0,    0,    0,    0,    0,    0]
    budget =    [80,   37,   37,   80,   80,   80,   80,   80,   80,   80]
    fail =      [0,    0,    0,    0,    0,    0,    0,    6,    0,    0]
    q =         [99.0, 1.5,  5.0,  1.25, 1.25, 1.0,  QCUT, 1.0,  NAN,  1.0]
    t =         [7.0,  7.0,  7.0,  30.0, 1.0,  t0,   30.0, t0,   30.0, t0]
    psum =      [8.0,  8.0,  8.0,  2.0,  0.0,  6.0,  6.0,  9.0,  6.0,  0.0]
    pn =        [3,    3,    3,    1,    0,    4,    4,    2,    4,    0]
    s = _qo_state(warm_left, budget, t, psum, pn)
    o = _qo(s, fail, q, 20.0, t_trunc)
    assert list(o["reset"]) == [0, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert list(o["done"]) == [0, 0, 0, 0, 0, 1, 1, 1, 1, 1]
    # warming and rejected envs keep their sums, going live zeroes and counts nothing (t = 0), a live step counts
    assert list(o["perf_sum"]) == [8.0, 0.0, 8.0, 3.25, 0.0, 6.0, 6.0, 9.0, 6.0, 0.0]
    assert list(o["perf_n"]) == [3, 0, 3, 2, 0, 4, 4, 2, 4, 0]
    # finished: envs 5 6 7 8 9 from fin_n = 3 into a ring of 4: slots 3 0 1 2 3 (env 9 overwrites env 5's entry)
    assert o["fin_n"] == 8
    assert list(o["perf"]) == [QCUT, 9.0 / 2, QCUT, QCUT, -9.0]
    assert (s["perf"] == -9.0).all()   # the inputs are not modified


def test_quartic_go_live_counts_nothing_even_with_a_negative_threshold():
    s = _qo_state([37], [37], [7.0], [8.0], [3])
    o = _qo(s, [0], [1.5], -1.0, 100.0)
    assert o["reset"][0] == 1 and o["perf_sum"][0] == 0.0 and o["perf_n"][0] == 0


def test_warmup_draw_zeroes_the_masked_envs_sums():
    s = _qo_state([0, 0, 5], [80, 80, 5], [1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [1, 2, 3])
    o = env_warmup_draw_perf_ref(s, np.array([1, 0, 1], np.uint8), SEED, OFF, LO, HI, DT, QCI)
    assert list(o["perf_sum"]) == [0.0, 5.0, 0.0] and list(o["perf_n"]) == [0, 2, 0]
    assert list(o["pending"]) == [1, 0, 1] and list(o["t"]) == [0.0, 2.0, 0.0]
    assert (o["perf"] == -9.0).all()
