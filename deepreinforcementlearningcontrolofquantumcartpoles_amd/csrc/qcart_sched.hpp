// qcart_sched.hpp — the training schedule's state machine (qc_sched, include/qcart.h), written once for the device
// kernel (qcart_sched.hip) and for plain C++ programs (tests/diag/sched_check.cpp): the state, the per-episode body of
// the drivers' loader loop (*/RL.py: IHO:497-535, IQO:495-533, HO:491-538, QO:477-527), one pass of
// Main_System.__call__ (IHO/main_parallel.py:492-526) with adjust_learning_rate (:544-558),
// scale_up_actor_update_time (:532-543) and receive_net's save count (:369-399), and the create-time checks. No HIP
// runtime type appears here. Every arithmetic operation is rounded once: the library is built with
// -ffp-contract=on, so each function body turns contraction off (a host compiler takes -ffp-contract=off).
// Internal: not part of the C ABI.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/qcart.h"
#include "qcart_state.hpp"

#if defined(__HIPCC__)
#define QC_SCHED_HD __host__ __device__
#else
#define QC_SCHED_HD
#endif
#if defined(__clang__)
#define QC_SCHED_ROUND_EACH _Pragma("clang fp contract(off)")
#else
#define QC_SCHED_ROUND_EACH
#endif

namespace qcart {
namespace sched {

constexpr int64_t kErrOverrun = 1;   // qc_sched_snapshot.error bit 0

struct State {
    double pending;             // pending_training_updates (RL.py:518), less what the ticks have issued
    double t_done;              // simulated time since the last push (RL.py:516, main_parallel.py:511-516)
    double last_achieved;       // last_achieved_time: the EMA (cartpole) / the best or last full time (cooling)
    double actor_update_time;   // main_parallel.py:456, 532-542
    double lr;                  // args.lr
    double simulated;           // simulated_oscillations (main_parallel.py:385)
    double sum, sumsq;          // train == 0: of the episode times, in walk order
    int64_t episode;            // episode.value: reset to 1 when learning starts
    int64_t total_episodes, total_rows;
    int64_t read;               // ring entries consumed so far
    int64_t episodes_since_save;   // episode_passed (main_parallel.py:386-395)
    int64_t n_test;
    int64_t tick;               // ticks run
    int32_t learning;           // learning_in_progress_event
    int32_t switched;           // train.backup_period == self.backup_period (main_parallel.py:546-547)
    int32_t started;            // an update has been issued (main_parallel.py:503)
    int32_t failure_counter;    // cooling (HO/RL.py:530)
    int32_t lr_step;
    int32_t error;              // sticky
};
static_assert(sizeof(State) == 8 * 8 + 7 * 8 + 6 * 4, "qc_sched state layout");

inline void init(State& s, const qc_sched_params& p) {
    s = State{};
    s.lr = p.lr_init;
    s.actor_update_time = p.actor_update_time;
}

// the first refusal of the params, or nullptr
inline const char* bad_params(const qc_sched_params* p) {
    if (!p) return "params is NULL";
    if (p->rule != QC_SCHED_CARTPOLE && p->rule != QC_SCHED_COOLING)
        return "rule must be QC_SCHED_CARTPOLE or QC_SCHED_COOLING";
    if (p->train != 0 && p->train != 1) return "train must be 0 or 1";
    if (p->rule == QC_SCHED_CARTPOLE) {
        if (!(p->fall_time > 0.)) return "fall_time must be > 0";
        if (!(p->start_time > p->fall_time)) return "start_time must be above fall_time";
        if (!std::isfinite(p->start_time)) return "start_time must be finite";
    } else {
        if (!(p->t_full > 0.) || !std::isfinite(p->t_full)) return "t_full must be finite and > 0";
        if (p->fail_limit < 1) return "fail_limit must be >= 1";
        if (!(p->first_interval_time >= 0.) || !(1.5 * p->first_interval_time < p->t_full))
            return "first_interval_time must be >= 0 and 1.5 first_interval_time below t_full";
    }
    if (p->batch_size < 1) return "batch_size must be >= 1";
    if (!(p->n_times_per_sample > 0.) || !std::isfinite(p->n_times_per_sample))
        return "n_times_per_sample must be finite and > 0";
    if (p->max_updates_per_tick < 1) return "max_updates_per_tick must be >= 1";
    if (p->min_rows < 0) return "min_rows must be >= 0";
    if (p->num_episodes < 1) return "num_episodes must be >= 1";
    if (p->give_up_episodes < 0) return "give_up_episodes must be >= 0";
    if (!(p->lr_init >= 0.) || !std::isfinite(p->lr_init)) return "lr_init must be finite and >= 0";
    if (!(p->lr_cap > 0.)) return "lr_cap must be > 0";
    if (p->n_lr_steps < 0 || p->n_lr_steps > QC_SCHED_MAX_LR_STEPS) return "lr_schedule holds at most 8 pairs";
    for (int i = 0; i < p->n_lr_steps; ++i) {
        if (p->lr_episode[i] < 0) return "lr_schedule episodes must be >= 0";
        if (i > 0 && p->lr_episode[i] <= p->lr_episode[i - 1]) return "lr_schedule episodes must be strictly increasing";
        if (!(p->lr_value[i] >= 0.) || !std::isfinite(p->lr_value[i])) return "lr_schedule rates must be finite and >= 0";
    }
    if (p->backup_period < 1 || p->warm_backup_period < 1) return "backup_period and warm_backup_period must be >= 1";
    if (p->save_interval < 1) return "save_interval must be >= 1";
    if (!(p->actor_update_time > 0.) || !std::isfinite(p->actor_update_time))
        return "actor_update_time must be finite and > 0";
    if (p->n_rungs < 0 || p->n_rungs > QC_SCHED_MAX_RUNGS) return "scale_up_actor_update_time has at most 4 rungs";
    for (int i = 0; i < p->n_rungs; ++i)
        if (!(p->rung_achieved[i] >= 0.) || !(p->rung_below[i] > 0.) || !(p->rung_time[i] > p->rung_below[i]))
            return "a rung needs achieved >= 0, below > 0 and a time above below";
    return nullptr;
}

inline uint64_t fnv(const void* q, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char* b = (const unsigned char*)q;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

// the exported state's header (qc_sched_state_export): the create-time params, the two tables as their lengths and
// a hash of the entries in use; the payload is the State and the tick count
inline state::Header header(const qc_sched_params& p) {
    namespace st = state;
    st::Header h = st::make(st::kSched);
    st::put_i(h, "rule", p.rule);
    st::put_i(h, "train", p.train);
    st::put_f(h, "start_time", p.start_time);
    st::put_f(h, "fall_time", p.fall_time);
    st::put_f(h, "t_full", p.t_full);
    st::put_f(h, "first_interval_time", p.first_interval_time);
    st::put_i(h, "fail_limit", p.fail_limit);
    st::put_i(h, "batch_size", p.batch_size);
    st::put_f(h, "n_times_per_sample", p.n_times_per_sample);
    st::put_i(h, "max_updates_per_tick", p.max_updates_per_tick);
    st::put_i(h, "min_rows", p.min_rows);
    st::put_i(h, "num_episodes", p.num_episodes);
    st::put_i(h, "give_up_episodes", p.give_up_episodes);
    st::put_f(h, "lr_init", p.lr_init);
    st::put_f(h, "lr_cap", p.lr_cap);
    st::put_i(h, "backup_period", p.backup_period);
    st::put_i(h, "warm_backup_period", p.warm_backup_period);
    st::put_i(h, "save_interval", p.save_interval);
    st::put_f(h, "actor_update_time", p.actor_update_time);
    st::put_i(h, "lr_schedule_len", p.n_lr_steps);
    uint64_t hs = fnv(p.lr_episode, sizeof(int64_t) * (size_t)p.n_lr_steps);
    st::put_u(h, "lr_schedule_hash", fnv(p.lr_value, sizeof(double) * (size_t)p.n_lr_steps, hs));
    st::put_i(h, "rungs_len", p.n_rungs);
    hs = fnv(p.rung_achieved, sizeof(double) * (size_t)p.n_rungs);
    hs = fnv(p.rung_below, sizeof(double) * (size_t)p.n_rungs, hs);
    st::put_u(h, "rungs_hash", fnv(p.rung_time, sizeof(double) * (size_t)p.n_rungs, hs));
    h.payload_bytes = sizeof(State) + sizeof(int64_t);
    return h;
}

// step 1 of a tick: the rows stored by this call (RL.py:518, credited here and not at the episode's end)
QC_SCHED_HD inline void credit_rows(State& s, int64_t rows) {
    QC_SCHED_ROUND_EACH
    s.total_rows += rows;
    const double due = (double)rows * 8. / 256.;
    s.pending = s.pending + due;
}

// step 2's start: how many ring entries are new; an overrun raises the error word and skips to the oldest present
QC_SCHED_HD inline int64_t ring_begin(State& s, int64_t fin_n, int64_t fin_cap) {
    int64_t fresh = fin_n - s.read;
    if (fresh < 0) fresh = 0;   // a ring that went backwards (another env's): nothing to walk
    if (fresh > fin_cap) {
        s.error |= (int32_t)kErrOverrun;
        s.read = fin_n - fin_cap;
        fresh = fin_cap;
    }
    return fresh;
}

// what the per-episode body reads of the params, by value: the kernel keeps it in registers over the whole walk
struct EpisodeRule {
    int32_t rule, train, fail_limit;
    double start_time, fall_time, t_full;
    double zero_sample_t;   // 1.5 first_interval_time (HO/RL.py:499: no row was stored up to there)
};
QC_SCHED_HD inline EpisodeRule episode_rule(const qc_sched_params& p) {
    QC_SCHED_ROUND_EACH
    EpisodeRule r;
    r.rule = p.rule; r.train = p.train; r.fail_limit = p.fail_limit;
    r.start_time = p.start_time; r.fall_time = p.fall_time; r.t_full = p.t_full;
    r.zero_sample_t = 1.5 * p.first_interval_time;
    return r;
}

// step 2: one finished episode of length t through the loader loop's body. kTrain / kCartpole are the rule's train
// and rule == QC_SCHED_CARTPOLE as compile-time constants, so a walk runs the one body its schedule needs
template <bool kTrain, bool kCartpole>
QC_SCHED_HD inline void episode_as(State& s, const EpisodeRule& p, double t) {
    QC_SCHED_ROUND_EACH
    s.episode += 1;                                   // RL.py:502
    if (!kTrain) {                                    // IHO/RL.py:505
        s.learning = 1;
        s.n_test += 1;
        s.sum = s.sum + t;
        const double tt = t * t;
        s.sumsq = s.sumsq + tt;
    }
    if (kTrain && !kCartpole && !s.learning && t <= p.zero_sample_t)
        s.learning = 1;                               // HO/RL.py:499: an episode that stored nothing
    s.t_done = s.t_done + t;                          // RL.py:516
    const double half = t * 0.5;                      // t / 2, exactly
    s.simulated = s.simulated + half;                 // main_parallel.py:385
    if (!kTrain) return;
    if (kCartpole) {
        const double a = s.last_achieved * 0.98, b = 0.02 * t;
        s.last_achieved = a + b;                      // IHO/RL.py:523
        if (s.last_achieved >= p.start_time && !s.learning) {   // :525-529
            s.learning = 1;
            s.episode = 1;
        } else if (s.learning && s.last_achieved < p.fall_time) {   // :532-534
            s.learning = 0;
        }
    } else {
        const bool full = t >= p.t_full, last_full = s.last_achieved >= p.t_full;
        if (!last_full) {                             // HO/RL.py:517
            if (s.last_achieved < t) {
                if (!full) {
                    s.last_achieved = t;              // :520
                } else {                              // :522-526: the first full episode
                    s.episode = 1;
                    s.failure_counter = 0;
                    s.last_achieved = t;
                    s.learning = 1;
                }
            }
        } else if (!full) {                           // :527-532
            s.failure_counter += 1;
            if (s.failure_counter == p.fail_limit) {
                s.last_achieved = t;
                s.learning = 0;
            }
        } else if (s.failure_counter != 0) {          // :533
            s.failure_counter = 0;
        }
    }
}

// step 2 for the n entries t_of(0) .. t_of(n - 1), in that order, and the ring position and episode total behind them
template <class Get>
QC_SCHED_HD inline void walk(State& s, const EpisodeRule& p, int64_t n, Get t_of) {
    if (!p.train)
        for (int64_t i = 0; i < n; ++i) episode_as<false, false>(s, p, t_of(i));
    else if (p.rule == QC_SCHED_CARTPOLE)
        for (int64_t i = 0; i < n; ++i) episode_as<true, true>(s, p, t_of(i));
    else
        for (int64_t i = 0; i < n; ++i) episode_as<true, false>(s, p, t_of(i));
    s.read += n;
    s.total_episodes += n;
}

// steps 3 and 4: one pass of Main_System.__call__'s loop body and the snapshot
QC_SCHED_HD inline void main_pass(State& s, const qc_sched_params& p, int64_t tick_episodes, qc_sched_snapshot& out) {
    QC_SCHED_ROUND_EACH
    // main_parallel.py:490, 494-503
    int64_t n_updates = 0;
    if (p.train && s.total_rows >= p.min_rows) {
        const double d0 = 8. / p.n_times_per_sample, d1 = (double)p.batch_size / 256.;
        const double D = d0 * d1;
        const double q = s.pending / D;
        double due = floor(q);
        if (due > (double)p.max_updates_per_tick) due = (double)p.max_updates_per_tick;
        if (due >= 1.) {
            n_updates = (int64_t)due;
            const double spent = due * D;
            s.pending = s.pending - spent;
            s.started = 1;
        }
    }
    // :511-517
    int32_t push = 0;
    if (s.t_done >= s.actor_update_time) {
        for (int i = 0; i < p.n_rungs; ++i)           // :532-542, the first rung that applies
            if (s.last_achieved > p.rung_achieved[i] && s.actor_update_time <= p.rung_below[i]) {
                s.actor_update_time = p.rung_time[i];
                break;
            }
        if (s.started) {
            push = 1;
            s.t_done = 0.;
        }
    }
    // :544-558
    if (!s.switched && s.learning) {
        s.switched = 1;
        if (p.lr_cap < s.lr) s.lr = p.lr_cap;
    }
    if (s.lr_step < p.n_lr_steps && s.learning && s.episode > p.lr_episode[s.lr_step]) {
        const double v = p.lr_value[s.lr_step];
        if (v < s.lr) s.lr = v;
        s.lr_step += 1;
    }
    // :386-395: counted when a new net arrives
    s.episodes_since_save += tick_episodes;
    int32_t save = 0;
    if (push && s.episodes_since_save >= p.save_interval) {
        save = 1;
        s.episodes_since_save = 0;
    }
    out.tick = s.tick;
    s.tick += 1;
    out.n_updates = n_updates;
    out.push = push;
    out.save = save;
    out.stop = !(s.episode < p.num_episodes || (s.episode < p.give_up_episodes && !s.learning));   // :492
    out.learning = s.learning;
    out.lr = s.lr;
    out.backup_period = s.switched ? p.backup_period : p.warm_backup_period;
    out.episode = s.episode;
    out.last_achieved = s.last_achieved;
    out.t_done = s.t_done;
    out.pending = s.pending;
    out.actor_update_time = s.actor_update_time;
    out.total_episodes = s.total_episodes;
    out.total_rows = s.total_rows;
    out.error = s.error;
    // main_parallel.py:445: mean and std(ddof = 1) / sqrt(n), from the running sums
    out.n = s.n_test;
    double mean = 0., sem = 0.;
    if (s.n_test > 0) {
        const double n = (double)s.n_test;
        mean = s.sum / n;
        if (s.n_test > 1) {                           // one episode has no spread: sem stays 0
            const double sm = s.sum * mean;
            const double dev = s.sumsq - sm, n1 = n - 1.;
            double var = dev / n1;
            if (var < 0.) var = 0.;
#if defined(__HIP_DEVICE_COMPILE__)
            sem = __dsqrt_rn(var) / __dsqrt_rn(n);
#else
            sem = std::sqrt(var) / std::sqrt(n);
#endif
        }
    }
    out.mean = mean;
    out.sem = sem;
}

}  // namespace sched
}  // namespace qcart
