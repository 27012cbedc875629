// qcart_env.hip — the batched episode loop's per-control-step bookkeeping (reset="deferred" and "warmup") in one
// kernel, so that PyTorch only holds the tensors: the cartpoles' termination, reward and return accounting of
// Control.do_episode (IHO/main_parallel.py:242-268, IQO/main_parallel.py:190-221) for every env of the batch,
// and the append of the finished episodes (return, length) to a device ring in env order (the reference's
// per-actor result queue, IHO/main_parallel.py:300-327) — no host synchronisation.
//
// Per env e, after a step call of one control interval:
//   * pending[e] set: this call was env e's reset interval (|0> / the IQO packet at F = 0, the zero-th step
//     without control, IHO:231-232, :250): its episode time restarts at one interval, its return at 0, no
//     transition is valid; an episode already over at that first control step (Fail or out of bounds) is
//     reported with return 0 and restarts again in the next call (the i != control_interval guard, IHO:250,
//     and the queue puts, IHO:312-313);
//   * otherwise: t += interval dt, done = Fail during the interval (numerical_failure, IHO:243-247) or out of
//     bounds (IHO |<x>| > xth, IHO:246; IQO the outside probability passed 0.5 at some physics step,
//     IQO:199-200); reward = failing_reward when done else 1, every transition valid, return += reward; a done
//     env is reported (return, t) and resets in the next call.
// kind == QC_HO: the cooling accounting (HO/main_parallel.py:222-292) on the phonon number `quantity`:
//   * pending[e] set: as above; the episode is already over iff Fail or quantity > cutoff (no truncation check
//     at the first control step, HO:240-246);
//   * otherwise: t += interval dt, done = Fail or !(quantity <= cutoff) (a NaN ends the episode) or
//     t >= t_trunc; reward = -quantity * reward_multiply; the terminal transition is not stored (valid = !done)
//     and adds nothing to the return.
// kind == QC_QO: the quartic cooling driver with a rolling warm-up (BatchedEnv reset="warmup"; the reset of
// QO/main_parallel.py:177-198, a packet of k ~ U[-0.3, 0.3] evolved freely for U[init_lo, init_hi] time units and
// redrawn until energy < init_energy_cutoff with no Fail, run inside the step launches of the following calls, at
// most one control interval per call). `quantity` is the energy after the call, budget[e] the steps env e took:
//   * warm_left[e] > 0 on entry (warming): left = warm_left - budget, warm_fail |= Fail; no reward, not done, no
//     valid transition; left > 0: budget = min(left, interval); left == 0, no Fail and energy < init_energy_cutoff
//     (strict: a NaN rejects): the env goes live, t = steps = return = 0, budget = interval, reset_out = 1 (this
//     call's observation is the episode's first; QO decides at i = 0, QO:208); otherwise it redraws;
//   * live: t += interval dt, done = Fail or !(energy < cutoff) or t >= t_trunc, reward = -energy *
//     reward_multiply, valid = !done, return += reward where valid (two rounded operations); a done env is
//     reported (return, t) and redraws;
//   * redraw (warmup_draw, also behind qc_env_warmup_draw): draw n = draws[e]++ of the env's own Philox stream
//     (tag kWarmTag) gives k and the evolution time; warm_left = ceil(init_t / dt), budget = min(warm_left,
//     interval), pending = 1: the caller writes the packet before the next step launch.
// perf (optional, HO and QO): the episode's performance, the mean of `quantity` over the live, non-terminal control
// steps whose new episode time is past perf_from (HO:247-248, 274-275, 294-295; QO:221, 231-232). perf_sum / perf_n
// restart at an episode's start (HO's pending branch, QO's go-live and every draw), a step that ends the episode adds
// nothing, and a finished episode's performance goes to the ring perf at the position of its (return, length):
// perf_sum / perf_n when it was truncated (t >= t_trunc) with perf_n > 0, else cutoff. Warming envs touch nothing
// (qc_env_warmup_draw zeroes both; a redraw inside the tail leaves them to the go-live branch).
// rec_mode[e] (optional) = 2 for an env pending on entry, else 1: qc_record's per-env mode (fresh history /
// append) for the 'measurements' input.
// One workgroup walks the batch in chunks of its 1024 threads, a workgroup scan per chunk placing the finished
// episodes of the chunk after the previous ones (env order, deterministic).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qcart_kernels.hpp"

namespace qcart {
namespace {

constexpr int kTailThreads = 1024;
constexpr int kFamQO = 2;              // enum qc_family
constexpr uint32_t kWarmTag = 0x400u;   // Philox counter word 3 of the warm-up draws

// Reset draw n of env e (QO/main_parallel.py:181-186): the packet's wavenumber k = u_k 0.6 - 0.3 and the free
// evolution time init_t = lo + u_t (hi - lo), every operation rounded once (no fused multiply-add), from one
// Philox4x32-10 block keyed by the seed at counter (n_lo, n_hi, global env id, kWarmTag). The env then warms
// up for ceil(init_t / dt) physics steps (at least 1, at most 2^31 - 1), `budget` of them in the next call.
__device__ __forceinline__ void warmup_draw(const EnvTailArgs& a, int64_t e) {
    const uint64_t n = (uint64_t)a.draws[e];
    a.draws[e] = (int64_t)(n + 1);
    uint32_t c[4] = {(uint32_t)n, (uint32_t)(n >> 32), (uint32_t)(a.env_offset + e), kWarmTag};
    philox10(c, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
    const double u_k = (double)(((((uint64_t)c[0]) << 32) | c[1]) >> 11) * 0x1.0p-53;
    const double u_t = (double)(((((uint64_t)c[2]) << 32) | c[3]) >> 11) * 0x1.0p-53;
    a.k[e] = __dadd_rn(__dmul_rn(u_k, 0.6), -0.3);
    const double init_t = __dadd_rn(a.init_lo, __dmul_rn(u_t, __dadd_rn(a.init_hi, -a.init_lo)));
    const double s = ceil(__ddiv_rn(init_t, a.dt));
    const int32_t left = s >= 1.0 ? (s < 2147483647.0 ? (int32_t)s : 2147483647) : 1;   // (a NaN gives 1)
    a.warm_left[e] = left;
    a.warm_fail[e] = 0;
    a.budget[e] = left < a.interval ? left : a.interval;
    a.pending[e] = 1;
}

// qc_env_warmup_draw: the masked envs start a warm-up, their episode accounting back to zero
__global__ __launch_bounds__(256) void k_warmup_draw(const EnvTailArgs a, const uint8_t* mask) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.B || (mask && !mask[e])) return;
    warmup_draw(a, e);
    a.t[e] = 0.0;
    a.steps[e] = 0;
    a.episode_return[e] = 0.0;
    if (a.perf) {
        a.perf_sum[e] = 0.0;
        a.perf_n[e] = 0;
    }
}

__global__ __launch_bounds__(kTailThreads) void k_env_tail(const EnvTailArgs a) {
    __shared__ int32_t wsum[kTailThreads / 64];
    __shared__ int64_t base;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) base = *a.fin_n;
    __syncthreads();
    const double ci_dt = (double)a.interval * a.dt;
    for (int64_t c0 = 0; c0 < a.B; c0 += kTailThreads) {
        const int64_t e = c0 + t;
        int fin = 0;
        double f_ret = 0.0, f_len = 0.0, f_perf = 0.0;
        if (e < a.B) {
            const bool pend = a.pending[e] != 0;
            const bool fail = a.fail_step[e] > 0;
            bool redraw = false;
            if (a.obs32)
                for (int i = 0; i < a.n_obs; ++i)
                    a.obs32[(size_t)e * a.n_obs + i] = (float)a.obs[(size_t)e * a.n_obs + i] * (float)a.input_scaling;
            if (a.rec_mode) a.rec_mode[e] = pend ? 2 : 1;   // qc_record: fresh history / append
            bool over;
            double tt, ret;
            float rw;
            // the performance's accounting (a.perf, cooling kinds): bit 0 an episode starts, bit 1 a live control step
            int pmode = 0;
            double pq = 0.0;
            if (a.kind == kFamQO) {   // QO cooling with the rolling warm-up
                const double q = a.quantity[e];
                const int32_t wl = a.warm_left[e];
                tt = a.t[e];
                ret = a.episode_return[e];
                rw = 0.0f;
                over = false;
                int go_live = 0;
                if (wl > 0) {
                    const int32_t left = wl - a.budget[e];
                    const bool wfail = a.warm_fail[e] != 0 || fail;
                    a.valid[e] = 0;
                    if (left > 0) {
                        a.warm_left[e] = left;
                        a.warm_fail[e] = wfail ? 1 : 0;
                        a.budget[e] = left < a.interval ? left : a.interval;
                    } else if (!wfail && q < a.init_energy_cutoff) {   // strict: a NaN energy rejects
                        a.warm_left[e] = 0;
                        a.warm_fail[e] = 0;
                        a.budget[e] = a.interval;
                        a.steps[e] = 0;
                        tt = 0.0;
                        ret = 0.0;
                        go_live = 1;
                        pmode = 1;
                    } else {
                        redraw = true;
                    }
                } else {
                    tt = __dadd_rn(tt, ci_dt);
                    over = fail || !(q < a.cutoff) || tt >= a.t_trunc;
                    const double r = __dmul_rn(-q, a.reward_multiply);
                    rw = (float)r;
                    ret = __dadd_rn(ret, over ? 0.0 : r);
                    a.steps[e] += a.interval;
                    a.valid[e] = over ? 0 : 1;
                    a.budget[e] = a.interval;
                    redraw = over;
                    pmode = 2;
                    pq = q;
                }
                a.reset_out[e] = go_live;
            } else if (a.kind == 0) {   // HO cooling
                const double q = a.quantity[e];
                pmode = pend ? 3 : 2;   // HO's first control step is a live one (HO:247-248)
                pq = q;
                if (pend) {
                    tt = ci_dt;
                    ret = 0.0;
                    rw = 0.0f;
                    over = fail || q > a.cutoff;   // no truncation at the first control step (HO:240-246)
                    a.steps[e] = a.interval;
                    a.valid[e] = 0;
                } else {
                    tt = __dadd_rn(a.t[e], ci_dt);
                    over = fail || !(q <= a.cutoff) || tt >= a.t_trunc;
                    // two rounded operations, as BatchedEnv's immediate mode does them (never one fused multiply-add)
                    const double r = __dmul_rn(-q, a.reward_multiply);
                    rw = (float)r;
                    ret = __dadd_rn(a.episode_return[e], over ? 0.0 : r);
                    a.steps[e] += a.interval;
                    a.valid[e] = over ? 0 : 1;   // the terminal transition of a cooling episode is not stored
                }
            } else {
                const bool oob =
                    a.kind == 3 ? (a.term_step[e] >= 0) : (fabs(a.obs[(size_t)e * a.n_obs]) > a.xth);
                over = fail || oob;
                if (pend) {
                    tt = ci_dt;
                    ret = 0.0;
                    rw = 0.0f;
                    a.steps[e] = a.interval;
                    a.valid[e] = 0;
                } else {
                    tt = a.t[e] + ci_dt;
                    rw = over ? (float)a.failing_reward : 1.0f;
                    // the return accumulates the float64 reward values, as BatchedEnv's immediate mode does
                    ret = a.episode_return[e] + (over ? a.failing_reward : 1.0);
                    a.steps[e] += a.interval;
                    a.valid[e] = 1;
                }
            }
            a.t[e] = tt;
            a.episode_return[e] = ret;
            a.reward[e] = rw;
            a.done[e] = over ? 1 : 0;
            if (a.perf && pmode) {
                double ps = (pmode & 1) ? 0.0 : a.perf_sum[e];
                int64_t pn = (pmode & 1) ? 0 : a.perf_n[e];
                if ((pmode & 2) && !over && tt > a.perf_from) {   // a terminal step adds nothing (the reference breaks first)
                    ps = __dadd_rn(ps, pq);
                    pn += 1;
                }
                a.perf_sum[e] = ps;
                a.perf_n[e] = pn;
                f_perf = (tt >= a.t_trunc && pn > 0) ? __ddiv_rn(ps, (double)pn) : a.cutoff;
            }
            if (a.kind == kFamQO) {   // pending: the packet of a new draw is to be written before the next step
                a.pending[e] = 0;
                if (redraw) warmup_draw(a, e);
            } else {
                a.pending[e] = over ? 1 : 0;
            }
            fin = over ? 1 : 0;
            f_ret = ret;
            f_len = tt;
        }
        // workgroup exclusive scan of fin (wave ballot + per-wave counts)
        const uint64_t m = __ballot(fin);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 63) wsum[w] = __popcll(m);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int i = 0; i < kTailThreads / 64; ++i) {
            const int v = wsum[i];
            woff += i < w ? v : 0;
            tot += v;
        }
        if (fin) {
            const int64_t pos = (base + woff + before) % a.fin_cap;
            a.fin[pos] = f_ret;
            a.fin[a.fin_cap + 1 + pos] = f_len;
            if (a.perf) a.perf[pos] = f_perf;
        }
        __syncthreads();
        if (t == 0) base += tot;
        __syncthreads();
    }
    if (t == 0) *a.fin_n = base;
}

}  // namespace

int launch_warmup_draw(const EnvTailArgs& a, const uint8_t* mask, void* stream) {
    if (a.B <= 0) return 0;
    hipLaunchKernelGGL(k_warmup_draw, dim3((unsigned)((a.B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, mask);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_env_tail(const EnvTailArgs& a, void* stream) {
    if (a.B <= 0) return 0;
    hipLaunchKernelGGL(k_env_tail, dim3(1), dim3(kTailThreads), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace qcart
