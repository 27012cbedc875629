"""CPU checks of tests/env_tail_warmup_ref.py (the checker of qc_env_tail's QO branch and of qc_env_warmup_draw) on
hand-written envs: a warming env with steps left, the last warm-up call accepted, rejected by energy, by Fail (in
this call and in an earlier one) and by NaN, a live env that continues, done by the strict energy bound, by
truncation and by Fail, the ring order and wrap, the draw counter, and the range of the draws."""
import numpy as np

from tests.env_tail_warmup_ref import (env_tail_warmup_ref, env_warmup_draw_ref, new_state, warmup_draw)

CI, DT = 80, 1 / 1440
CI_DT = np.float64(CI) * np.float64(DT)
CUT, INIT_CUT = 12.0, 2.0
LO, HI = 0.2, 0.5
SEED, OFF = 3, 40


def _call(s, fail, q, t_trunc=100.0 - 0.01 * DT, rm=0.5):
    obs = np.zeros((len(q), 5))
    obs[:, 1] = 0.25
    return env_tail_warmup_ref(s, CI, DT, 0.7, CUT, t_trunc, rm, INIT_CUT, LO, HI, SEED, OFF,
                               np.array(fail, np.int32), np.array(q, np.float64), obs)


def _state(warm_left, budget, warm_fail, t, ret, draws, fin_cap=4, fin_n=2):
    B = len(warm_left)
    s = new_state(B, CI, fin_cap)
    s.update(warm_left=np.array(warm_left, np.int32), budget=np.array(budget, np.int32),
             warm_fail=np.array(warm_fail, np.uint8), t=np.array(t, np.float64),
             episode_return=np.array(ret, np.float64), draws=np.array(draws, np.int64),
             steps=np.arange(B, dtype=np.int64) * CI, k=np.full(B, 0.125), pending=np.ones(B, np.uint8),
             fin=np.full((2, fin_cap + 1), -7.0), fin_n=fin_n)
    return s


def test_hand_written_envs():
    nan = float("nan")
    below, trunc_t = np.nextafter(CUT, 0.0), 50.0
    t_trunc = np.float64(trunc_t) + CI_DT
    #            0: warming  1: accepted  2: energy   3: Fail now  4: Fail earlier  5: NaN  6: live   7: at the bound
    #            8: ulp below the bound   9: truncated  10: Fail  11: live NaN  12: accepted exactly below init cutoff
    warm_left = [200,        37,          37,         80,          12,              80,     0,        0,
                 0,                       0,            0,        0,            80]
    budget =    [80,         37,          37,         80,          12,              80,     80,       80,
                 80,                      80,           80,       80,           80]
    warm_fail = [0,          0,           0,          0,           1,               0,      0,        0,
                 0,                       0,            0,        0,            0]
    fail =      [5,          0,           0,          9,           0,               0,      0,        0,
                 0,                       0,            3,        0,            0]
    q =         [99.0,       1.5,         INIT_CUT,   1.0,         1.0,             nan,    1.5,      CUT,
                 below,                   1.0,          0.25,     nan,          np.nextafter(INIT_CUT, 0.0)]
    t =         [7.0,        7.0,         7.0,        7.0,         7.0,             7.0,    1.0,      2.0,
                 3.0,                     trunc_t,      5.0,      6.0,          7.0]
    ret = [-3.0] * 13
    draws = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13]
    s = _state(warm_left, budget, warm_fail, t, ret, draws)
    o = _call(s, fail, q, t_trunc=t_trunc)
    assert list(o["done"]) == [0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 1, 1, 0]
    assert list(o["valid"]) == [0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0]
    assert list(o["reset"]) == [0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    redrawn = [0, 0, 1, 1, 1, 1, 0, 1, 0, 1, 1, 1, 0]
    assert list(o["pending"]) == redrawn
    assert list(o["draws"]) == [d + r for d, r in zip(draws, redrawn)]          # the draw counter
    # 0: 120 steps left, the Fail remembered; 1, 12: live
    assert (o["warm_left"][0], o["warm_fail"][0], o["budget"][0]) == (120, 1, 80)
    for e in (1, 12):
        assert (o["warm_left"][e], o["warm_fail"][e], o["budget"][e]) == (0, 0, CI)
        assert (o["t"][e], o["steps"][e], o["episode_return"][e]) == (0.0, 0, 0.0)
    # the redrawn envs carry draw number draws[e] of their own stream
    for e in np.nonzero(redrawn)[0]:
        k, init_t, left, bud = warmup_draw(SEED, OFF + e, draws[e], LO, HI, DT, CI)
        assert LO <= init_t < HI and -0.3 <= k < 0.3
        assert (o["k"][e], o["warm_left"][e], o["budget"][e], o["warm_fail"][e]) == (k, left, bud, 0)
        assert left == int(np.ceil(init_t / DT)) and bud == min(left, CI) and 288 <= left <= 720
    assert o["k"][0] == 0.125 and o["k"][6] == 0.125
    # warming envs: no reward, time and return untouched unless they went live; live envs: the cooling accounting
    rw = o["reward"]
    assert rw.dtype == np.float32 and list(rw[:6]) == [0.0] * 6 and rw[12] == 0.0
    assert list(rw[6:11]) == [np.float32(-0.75), np.float32(-6.0), np.float32(-below * 0.5), np.float32(-0.5),
                              np.float32(-0.125)] and np.isnan(rw[11])
    assert list(o["t"][[0, 2, 3, 4, 5]]) == [7.0] * 5 and list(o["episode_return"][[0, 2, 3, 4, 5]]) == [-3.0] * 5
    assert list(o["t"][6:12]) == [x + CI_DT for x in t[6:12]] and o["t"][9] == t_trunc
    assert list(o["episode_return"][6:12]) == [-3.75, -3.0, -3.0 - below * 0.5, -3.0, -3.0, -3.0]
    assert list(o["steps"][6:12]) == [(e + 1) * CI for e in range(6, 12)]
    assert list(o["steps"][[0, 2, 3, 4, 5]]) == [0, 2 * CI, 3 * CI, 4 * CI, 5 * CI]
    # envs 7, 9, 10, 11 finish, from fin_n = 2 into a ring of 4: slots 2, 3, 0, 1 in env order; the sinks keep -7
    assert o["fin_n"] == 6
    assert list(o["fin"][0]) == [-3.0, -3.0, -3.0, -3.0, -7.0]
    assert list(o["fin"][1]) == [5.0 + CI_DT, 6.0 + CI_DT, 2.0 + CI_DT, t_trunc, -7.0]
    assert o["obs32"].dtype == np.float32 and o["obs32"][0, 1] == np.float32(0.25) * np.float32(0.7)
    assert (s["fin"] == -7.0).all() and list(s["draws"]) == draws   # the inputs are not modified


def test_truncation_one_ulp_below_t_trunc_continues():
    t0 = 11.0
    s = _state([0, 0], [CI, CI], [0, 0], [t0, np.nextafter(t0, 0.0)], [-2.0, -2.0], [0, 0], fin_cap=8, fin_n=0)
    o = _call(s, [0, 0], [1.0, 1.0], t_trunc=np.float64(t0) + CI_DT)
    assert list(o["done"]) == [1, 0] and list(o["valid"]) == [0, 1] and list(o["episode_return"]) == [-2.0, -2.5]
    assert o["fin_n"] == 1 and o["fin"][0, 0] == -2.0 and o["fin"][1, 0] == np.float64(t0) + CI_DT


def test_return_rounds_the_product_and_the_sum_separately():
    x = 1.0 + 2.0 ** -30
    s = _state([0], [CI], [0], [1.0], [1.0 + 2.0 ** -29], [0])
    o = _call(s, [0], [x], rm=x)
    assert o["episode_return"][0] == 0.0 and o["valid"][0] == 1


def test_ring_wraps_and_a_chain_of_calls_walks_a_whole_warm_up():
    """reset(mask) then calls until the env goes live: the budgets add up to warm_left and the last call is the
    remainder; a rejected warm-up takes the next draw of the same stream."""
    s = new_state(3, CI, 4)
    s = env_warmup_draw_ref(s, np.array([1, 0, 1]), SEED, OFF, LO, HI, DT, CI)
    assert list(s["pending"]) == [1, 0, 1] and list(s["draws"]) == [1, 0, 1] and s["warm_left"][1] == 0
    left0 = int(s["warm_left"][0])
    assert left0 == warmup_draw(SEED, OFF, 0, LO, HI, DT, CI)[2]
    took, calls = 0, 0
    while s["warm_left"][0] > 0:
        took += int(s["budget"][0])
        calls += 1
        # env 2 reports a Fail in its first call: rejected at the end of its warm-up whatever the energy
        s = _call(s, [0, 0, 1 if calls == 1 else 0], [1.0, 1.0, 1.0])
        assert calls < 20
    assert took == left0 and calls == -(-left0 // CI) and s["reset"][0] == 1 and s["draws"][0] == 1
    assert s["draws"][2] >= 2 or s["warm_left"][2] > 0     # env 2 redrew (or is still in its first warm-up)
    assert s["valid"][1] == 1                              # env 1 was live throughout


def test_draws_cover_their_ranges():
    rng = np.random.default_rng(0)
    ks, ts = [], []
    for env, n in zip(rng.integers(0, 2 ** 32, 10_000), rng.integers(0, 2 ** 40, 10_000)):
        k, init_t, left, bud = warmup_draw(SEED, env, n, LO, HI, DT, CI)
        ks.append(k)
        ts.append(init_t)
        assert left == max(1, int(np.ceil(init_t / DT))) and bud == min(left, CI)
    ks, ts = np.array(ks), np.array(ts)
    assert ks.min() >= -0.3 and ks.max() < 0.3 and ts.min() >= LO and ts.max() < HI
    assert ks.min() < -0.29 and ks.max() > 0.29 and ts.min() < LO + 0.01 and ts.max() > HI - 0.01
    assert abs(ks.mean()) < 0.01 and abs(ts.mean() - (LO + HI) / 2) < 0.005
    # a different draw index, env or seed gives a different draw
    a = warmup_draw(SEED, 7, 0, LO, HI, DT, CI)
    assert a != warmup_draw(SEED, 7, 1, LO, HI, DT, CI) and a != warmup_draw(SEED, 8, 0, LO, HI, DT, CI)
    assert a != warmup_draw(SEED + 1, 7, 0, LO, HI, DT, CI) and a != warmup_draw(SEED, 7, 1 << 32, LO, HI, DT, CI)
