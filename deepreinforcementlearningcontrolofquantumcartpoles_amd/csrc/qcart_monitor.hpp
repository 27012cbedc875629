// qcart_monitor.hpp — the cooling drivers' model ranking (qc_monitor, include/qcart.h), written once for the device
// kernel (qcart_monitor.hip) and for plain C++ programs (tests/diag/monitor_check.cpp): worker_manager.receive_net
// (QO/main_parallel.py:283-329, HO/main_parallel.py:348-388) on the stream of finished episodes' performances —
// the table of the num_of_saves best window means, the "enough new episodes" rule and, with train == 0, the running
// count / sum / sum of squares of the --test mode. No HIP runtime type appears here. Every arithmetic operation is
// rounded once: the library is built with -ffp-contract=on, so each function body turns contraction off (a host
// compiler takes -ffp-contract=off).
// Internal: not part of the C ABI.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/qcart.h"
#include "qcart_state.hpp"

#if defined(__HIPCC__)
#define QC_MON_HD __host__ __device__
#else
#define QC_MON_HD
#endif
#if defined(__clang__)
#define QC_MON_ROUND_EACH _Pragma("clang fp contract(off)")
#else
#define QC_MON_ROUND_EACH
#endif

namespace qcart {
namespace monitor {

constexpr int64_t kErrOverrun = 1;   // qc_monitor_snapshot.error bit 0 (train == 0 only)

struct State {
    double good[QC_MONITOR_MAX_SAVES];       // good_actors' values, increasing; entries past num_of_saves unused
    int32_t filled[QC_MONITOR_MAX_SAVES];    // 1 where the entry holds a model (type(actor[1]) != float)
    double sum, sumsq;                       // train == 0: of the performances, in ring order
    int64_t count;                           // len(performances) since the last receive
    int64_t episode_passed;
    int64_t read;                            // ring entries consumed so far
    int64_t n;                               // train == 0: performances counted
    int64_t calls;                           // receives run
    int64_t total_episodes;
    int32_t error;                           // sticky
    int32_t pad;
};
static_assert(sizeof(State) == QC_MONITOR_MAX_SAVES * 12 + 2 * 8 + 6 * 8 + 8, "qc_monitor state layout");

inline void init(State& s, const qc_monitor_params& p) {
    s = State{};
    for (int i = 0; i < QC_MONITOR_MAX_SAVES; ++i) s.good[i] = p.initial;
}

// the first refusal of the params, or nullptr
inline const char* bad_params(const qc_monitor_params* p) {
    if (!p) return "params is NULL";
    if (p->train != 0 && p->train != 1) return "train must be 0 or 1";
    if (p->window < 1 || p->window > QC_MONITOR_MAX_WINDOW) return "window must be in [1, 16]";
    if (p->min_count < 1 || p->min_count > p->window) return "min_count must be in [1, window]";
    if (p->min_episodes < 0) return "min_episodes must be >= 0";
    if (p->num_of_saves < 1 || p->num_of_saves > QC_MONITOR_MAX_SAVES) return "num_of_saves must be in [1, 64]";
    if (!std::isfinite(p->initial)) return "initial must be finite";
    return nullptr;
}

// the exported state's header (qc_monitor_state_export): the create-time params; the payload is the State and the
// receive count
inline state::Header header(const qc_monitor_params& p) {
    namespace st = state;
    st::Header h = st::make(st::kMonitor);
    st::put_i(h, "train", p.train);
    st::put_i(h, "window", p.window);
    st::put_i(h, "min_count", p.min_count);
    st::put_i(h, "min_episodes", p.min_episodes);
    st::put_i(h, "num_of_saves", p.num_of_saves);
    st::put_f(h, "initial", p.initial);
    h.payload_bytes = sizeof(State) + sizeof(int64_t);
    return h;
}

// np.mean of the k <= 16 values a_of(0) .. a_of(k - 1) in numpy's summation order: below 8 values a running sum from
// 0; from 8 on eight partial sums r[j] = a[j] (+ a[8 + j] with 16 values) combined as ((r0 + r1) + (r2 + r3)) +
// ((r4 + r5) + (r6 + r7)), then the values past the last whole block of 8 one by one; each operation rounded once
template <class Get>
QC_MON_HD inline double window_mean(int k, Get a_of) {
    QC_MON_ROUND_EACH
    double res;
    if (k < 8) {
        res = 0.;
        for (int i = 0; i < k; ++i) res = res + a_of(i);
    } else {
        double r0 = a_of(0), r1 = a_of(1), r2 = a_of(2), r3 = a_of(3), r4 = a_of(4), r5 = a_of(5), r6 = a_of(6),
               r7 = a_of(7);
        int i = 8;
        for (; i + 8 <= k; i += 8) {
            r0 = r0 + a_of(i); r1 = r1 + a_of(i + 1); r2 = r2 + a_of(i + 2); r3 = r3 + a_of(i + 3);
            r4 = r4 + a_of(i + 4); r5 = r5 + a_of(i + 5); r6 = r6 + a_of(i + 6); r7 = r7 + a_of(i + 7);
        }
        const double a = r0 + r1, b = r2 + r3, c = r4 + r5, d = r6 + r7;
        const double ab = a + b, cd = c + d;
        res = ab + cd;
        for (; i < k; ++i) res = res + a_of(i);
    }
    return res / (double)k;
}

// how many ring entries are new since the last receive (a ring that went backwards: none)
QC_MON_HD inline int64_t fresh_of(const State& s, int64_t fin_n) {
    const int64_t fresh = fin_n - s.read;
    return fresh < 0 ? 0 : fresh;
}
// of those, how many receive_train reads: the last min(fresh, window)
QC_MON_HD inline int window_len(const qc_monitor_params& p, int64_t fresh) {
    return fresh < (int64_t)p.window ? (int)fresh : p.window;
}

QC_MON_HD inline void fill_common(const State& s, const qc_monitor_params& p, qc_monitor_snapshot& out) {
    int64_t nf = 0;
    for (int i = 0; i < p.num_of_saves; ++i) nf += s.filled[i];
    out.n_filled = nf;
    out.episode_passed = s.episode_passed;
    out.total_episodes = s.total_episodes;
    out.error = s.error;
}

// train == 1: receive_net when a net has arrived. a_of(j), j in [0, window_len), is the j-th oldest of the last
// window_len(fresh) performances
template <class Get>
QC_MON_HD inline void receive_train(State& s, const qc_monitor_params& p, int64_t fin_n, Get a_of,
                                    qc_monitor_snapshot& out) {
    QC_MON_ROUND_EACH
    const int64_t fresh = fresh_of(s, fin_n);
    s.count = fresh;                                  // the performances appended since the last clear()
    s.episode_passed += fresh;
    s.total_episodes += fresh;
    s.read = fin_n;
    out.rank = -1;
    out.new_avg = 0.;
    if (s.episode_passed > p.min_episodes && s.count >= (int64_t)p.min_count) {   // QO:311, HO:373
        const double avg = window_mean(window_len(p, fresh), a_of);
        out.new_avg = avg;
        const int last = p.num_of_saves - 1;
        if (avg < s.good[last]) {                     // (a NaN mean is no record)
            // good_actors[-1] = (avg, net); good_actors.sort(): stable, so the new entry goes behind its equals
            int rank = 0;
            for (int i = 0; i < last; ++i) rank += s.good[i] <= avg ? 1 : 0;
            for (int i = last; i > rank; --i) {
                s.good[i] = s.good[i - 1];
                s.filled[i] = s.filled[i - 1];
            }
            s.good[rank] = avg;
            s.filled[rank] = 1;
            s.episode_passed = 0;
            out.rank = rank;
        }
    }
    out.count = s.count;
    s.count = 0;                                      // performances.clear()
    out.call = s.calls;
    s.calls += 1;
    out.mean = 0.;
    out.sem = 0.;
    out.n = 0;
    fill_common(s, p, out);
}

// train == 0: the walk's bounds, from the state as it is (it is not changed: every lane of the kernel computes them,
// test_finish applies them). More than fin_cap new entries are an overrun: the walk starts at the oldest still present
struct Walk {
    int64_t fresh, first;
    int32_t overrun;
};
QC_MON_HD inline Walk test_walk(const State& s, int64_t fin_n, int64_t fin_cap) {
    Walk w{fresh_of(s, fin_n), s.read, 0};
    if (w.fresh > fin_cap) {
        w.overrun = 1;
        w.first = fin_n - fin_cap;
        w.fresh = fin_cap;
    }
    return w;
}

// the running sums the walk carries in registers
struct Sums {
    double sum, sumsq;
    int64_t n;
};
QC_MON_HD inline void test_add(Sums& a, double v) {
    QC_MON_ROUND_EACH
    a.n += 1;
    a.sum = a.sum + v;
    const double vv = v * v;
    a.sumsq = a.sumsq + vv;
}

// train == 0, end: the sums back into the state and the snapshot: mean and std(ddof = 1) / sqrt(n)
QC_MON_HD inline void test_finish(State& s, const qc_monitor_params& p, const Sums& a, const Walk& w,
                                  qc_monitor_snapshot& out) {
    QC_MON_ROUND_EACH
    const int64_t fresh = w.fresh;
    if (w.overrun) s.error |= (int32_t)kErrOverrun;
    s.sum = a.sum;
    s.sumsq = a.sumsq;
    s.n = a.n;
    s.read = w.first + fresh;
    s.total_episodes += fresh;
    s.episode_passed += fresh;
    s.count = 0;
    out.rank = -1;
    out.new_avg = 0.;
    out.count = fresh;
    out.call = s.calls;
    s.calls += 1;
    double mean = 0., sem = 0.;
    if (s.n > 0) {
        const double n = (double)s.n;
        mean = s.sum / n;
        if (s.n > 1) {                                // one episode has no spread: sem stays 0
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
    out.n = s.n;
    fill_common(s, p, out);
}

}  // namespace monitor
}  // namespace qcart
