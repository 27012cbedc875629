// qcart_sched.hip — the training schedule on the device (qc_sched, include/qcart.h): one single-workgroup launch per
// control step that counts the stored rows, walks the finished-episode ring's new entries through the drivers' loader
// loop body and runs one Main_System pass (the state machine: qcart_sched.hpp), then one asynchronous copy of the
// snapshot into the tick's pinned host slot and one event record. qc_sched_poll waits on that event alone. Every
// loop of the kernel is bounded by B or fin_cap; nothing polls or waits.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/qcart.h"
#include "qcart_host.hpp"
#include "qcart_sched.hpp"
#include "qcart_state.hpp"

namespace qcart {
namespace sched {

constexpr int kThreads = 256, kWave = 64;

struct TickArgs {
    State* st;
    const qc_sched_params* p;
    qc_sched_snapshot* snap;
    const double* len;       // the ring's length row: fin + fin_cap + 1
    int64_t fin_cap;
    const int64_t* fin_n;
    const uint8_t* valid;
    int64_t B;
};

__device__ inline int wave_sum(int v) {
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}

__global__ __launch_bounds__(kThreads) void k_sched_tick(TickArgs a) {
    __shared__ int wsum[kThreads / kWave];
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;

    // 1. the rows of this call: set bytes of valid[0, B), four at a time where the mask is word aligned
    int cnt = 0;
    const bool words = ((uintptr_t)a.valid & 3) == 0;
    const int64_t nw = words ? a.B / 4 : 0;
    const uint32_t* vw = (const uint32_t*)a.valid;
    for (int64_t i = tid; i < nw; i += kThreads) {
        const uint32_t w = vw[i];
        const uint32_t nz = (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;   // bit 7 of each non-zero byte
        cnt += __popc(nz);
    }
    for (int64_t i = nw * 4 + tid; i < a.B; i += kThreads) cnt += a.valid[i] != 0;
    cnt = wave_sum(cnt);
    if (lane == 0) wsum[wv] = cnt;
    __syncthreads();
    if (wv != 0) return;
    // The rest is wave 0's. All 64 lanes carry the same state through the same arithmetic (control flow stays uniform,
    // so every lane's register is defined where another lane reads it); lane 0 alone writes the results.
    const EpisodeRule rule = episode_rule(*a.p);   // by value: no load inside the walk
    State s = *a.st;
    int64_t rows = 0;
    for (int w = 0; w < kThreads / kWave; ++w) rows += wsum[w];
    credit_rows(s, rows);
    const int64_t fresh = ring_begin(s, *a.fin_n, a.fin_cap), first = s.read;

    // 2. the new ring entries, 64 at a time: one coalesced load, a lane each, then the walk in ring order with entry j
    // read out of lane j's registers
    for (int64_t c = 0; c < fresh; c += kWave) {
        const int64_t left = fresh - c;
        const int m = left < kWave ? (int)left : kWave;
        const double mine = lane < m ? a.len[(first + c + lane) % a.fin_cap] : 0.;
        const int lo = __double2loint(mine), hi = __double2hiint(mine);
        walk(s, rule, m, [&](int64_t j) {
            return __hiloint2double(__builtin_amdgcn_readlane(hi, (int)j), __builtin_amdgcn_readlane(lo, (int)j));
        });
    }

    // 3., 4. the Main_System pass and the snapshot
    qc_sched_snapshot out;
    main_pass(s, *a.p, fresh, out);
    if (lane == 0) {
        *a.snap = out;
        *a.st = s;
    }
}

__global__ void k_sched_seek(State* st, const int64_t* fin_n) {
    if (threadIdx.x == 0 && blockIdx.x == 0) st->read = *fin_n;
}

}  // namespace sched
}  // namespace qcart

using namespace qcart::sched;
namespace st = qcart::state;

struct qc_sched {
    qc_sched_params p{};
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    int64_t ticks = 0;                       // ticks enqueued
    int64_t first_tick = 0;                  // the first tick this handle ran itself (the tick count of an import)
    State* d_st = nullptr;
    qc_sched_params* d_p = nullptr;
    qc_sched_snapshot* d_snap = nullptr;     // [2]: tick t writes slot t & 1
    qc_sched_snapshot* h_snap = nullptr;     // pinned [2]
    hipEvent_t ev[2] = {nullptr, nullptr};
};

namespace {

using qcart::host::Dev;
qcart::host::CreateError g_sched_err;

int sfail(qc_sched* s, int code, const std::string& msg) {
    s->err = msg;
    return code;
}

}  // namespace

extern "C" {

int qc_sched_create(const qc_sched_params* p, int device, qc_sched** out) {
    if (!out) return QC_EINVAL;
    *out = nullptr;
    if (const char* bad = bad_params(p)) return g_sched_err.fail(std::string("qc_sched_create: ") + bad, QC_EINVAL);
    if (const int rc = qcart::host::check_device(device, g_sched_err, "the schedule")) return rc;
    qc_sched* s = new qc_sched();
    s->p = *p;
    s->device = device;
    Dev g(device);
    State init_state;
    init(init_state, s->p);
    hipError_t e = hipMalloc((void**)&s->d_st, sizeof(State));
    if (e == hipSuccess) e = hipMalloc((void**)&s->d_p, sizeof(qc_sched_params));
    if (e == hipSuccess) e = hipMalloc((void**)&s->d_snap, 2 * sizeof(qc_sched_snapshot));
    if (e == hipSuccess) e = hipHostMalloc((void**)&s->h_snap, 2 * sizeof(qc_sched_snapshot), hipHostMallocDefault);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&s->ev[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemcpy(s->d_st, &init_state, sizeof(State), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_p, &s->p, sizeof(qc_sched_params), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(s->d_snap, 0, 2 * sizeof(qc_sched_snapshot));
    if (e != hipSuccess) {
        const std::string msg = std::string("qc_sched_create: ") + hipGetErrorString(e);
        qc_sched_destroy(s);
        return g_sched_err.fail(msg, QC_EHIP);
    }
    std::memset(s->h_snap, 0, 2 * sizeof(qc_sched_snapshot));
    *out = s;
    return QC_OK;
}

void qc_sched_destroy(qc_sched* s) {
    if (!s) return;
    {
        Dev g(s->device);
        (void)hipDeviceSynchronize();
        for (void* q : {(void*)s->d_st, (void*)s->d_p, (void*)s->d_snap})
            if (q) (void)hipFree(q);
        if (s->h_snap) (void)hipHostFree(s->h_snap);
        for (hipEvent_t ev : s->ev)
            if (ev) (void)hipEventDestroy(ev);
    }
    delete s;
}

const char* qc_sched_last_error(const qc_sched* s) { return s ? s->err.c_str() : g_sched_err.text(); }

int qc_sched_set_stream(qc_sched* s, void* stream) {
    if (!s) return QC_EINVAL;
    s->stream = (hipStream_t)stream;
    return QC_OK;
}

int qc_sched_tick(qc_sched* s, const double* fin, int64_t fin_cap, const int64_t* fin_n, const uint8_t* valid,
                  int64_t B) {
    if (!s) return QC_EINVAL;
    if (!fin || !fin_n || fin_cap < 1) return sfail(s, QC_EINVAL, "qc_sched_tick: fin, fin_n and fin_cap >= 1 are required");
    if (B < 0 || B > ((int64_t)1 << 30) || (B > 0 && !valid))
        return sfail(s, QC_EINVAL, "qc_sched_tick: B must be in [0, 2^30], with valid where B > 0");
    Dev g(s->device);
    const int slot = (int)(s->ticks & 1);
    TickArgs a{};
    a.st = s->d_st;
    a.p = s->d_p;
    a.snap = s->d_snap + slot;
    a.len = fin + fin_cap + 1;
    a.fin_cap = fin_cap;
    a.fin_n = fin_n;
    a.valid = valid;
    a.B = B;
    hipLaunchKernelGGL(k_sched_tick, dim3(1), dim3(kThreads), 0, s->stream, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpyAsync(s->h_snap + slot, s->d_snap + slot, sizeof(qc_sched_snapshot), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipEventRecord(s->ev[slot], s->stream);
    if (e != hipSuccess) return qcart::host::hip_fail(s->err, e, "qc_sched_tick");
    s->ticks += 1;
    return QC_OK;
}

int qc_sched_seek(qc_sched* s, const int64_t* fin_n) {
    if (!s) return QC_EINVAL;
    if (!fin_n) return sfail(s, QC_EINVAL, "qc_sched_seek: fin_n is required");
    Dev g(s->device);
    hipLaunchKernelGGL(k_sched_seek, dim3(1), dim3(1), 0, s->stream, s->d_st, fin_n);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? QC_OK : qcart::host::hip_fail(s->err, e, "qc_sched_seek");
}

int qc_sched_poll(qc_sched* s, int64_t tick, qc_sched_snapshot* out) {
    if (!s || !out) return QC_EINVAL;
    if (tick < s->first_tick || tick >= s->ticks || tick < s->ticks - 2)
        return sfail(s, QC_EINVAL, "qc_sched_poll: tick " + std::to_string(tick) + " is not one of the last two of " +
                                       std::to_string(s->ticks) + " ticks (ticks before a state import stay with the handle that ran them)");
    Dev g(s->device);
    const int slot = (int)(tick & 1);
    const hipError_t e = hipEventSynchronize(s->ev[slot]);
    if (e != hipSuccess) return qcart::host::hip_fail(s->err, e, "qc_sched_poll");
    *out = s->h_snap[slot];
    return QC_OK;
}

int qc_sched_state_bytes(qc_sched* s, uint64_t* n) {
    if (!s || !n) return QC_EINVAL;
    *n = sizeof(st::Header) + sizeof(State) + sizeof(int64_t);
    return QC_OK;
}

int qc_sched_state_export(qc_sched* s, void* host_dst, uint64_t n) {
    if (!s || !host_dst) return QC_EINVAL;
    const st::Header h = header(s->p);
    if (n != sizeof(st::Header) + h.payload_bytes)
        return sfail(s, QC_EINVAL, "qc_sched_state_export: n differs from what qc_sched_state_bytes gives");
    Dev g(s->device);
    State cur;
    hipError_t e = hipStreamSynchronize(s->stream);
    if (e == hipSuccess) e = hipMemcpy(&cur, s->d_st, sizeof(State), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return qcart::host::hip_fail(s->err, e, "qc_sched_state_export");
    std::memcpy(host_dst, &h, sizeof(h));
    st::Cursor c(host_dst);
    std::memcpy(c.take(sizeof(State)), &cur, sizeof(State));
    std::memcpy(c.take(sizeof(int64_t)), &s->ticks, sizeof(int64_t));
    return QC_OK;
}

int qc_sched_state_import(qc_sched* s, const void* host_src, uint64_t n) {
    if (!s) return QC_EINVAL;
    const st::Header mine = header(s->p);
    st::Header h;
    std::string bad = st::validate(host_src, n, mine, &h);
    const std::string who = "qc_sched_state_import: ";
    if (bad.empty() && h.payload_bytes != mine.payload_bytes)
        bad = who + "payload_bytes: blob " + std::to_string(h.payload_bytes) + ", handle " +
              std::to_string(mine.payload_bytes);
    State in;
    int64_t ticks = 0;
    if (bad.empty()) {
        const unsigned char* at = (const unsigned char*)host_src + sizeof(st::Header);
        std::memcpy(&in, at, sizeof(State));
        std::memcpy(&ticks, at + sizeof(State), sizeof(int64_t));
        if (ticks < 0 || in.tick != ticks)
            bad = who + "tick count: blob " + std::to_string(ticks) + ", its state " + std::to_string(in.tick);
        else if (in.read < 0 || in.episode < 0 || in.total_episodes < 0 || in.total_rows < 0 || in.n_test < 0 ||
                 in.episodes_since_save < 0)
            bad = who + "a counter of the blob's state is negative";
        else if (in.lr_step < 0 || in.lr_step > s->p.n_lr_steps)
            bad = who + "lr_step: blob " + std::to_string(in.lr_step) + ", the handle's schedule has " +
                  std::to_string(s->p.n_lr_steps) + " steps";
    }
    if (!bad.empty()) return sfail(s, QC_EINVAL, bad);
    Dev g(s->device);
    hipError_t e = hipStreamSynchronize(s->stream);
    if (e == hipSuccess) e = hipMemcpy(s->d_st, &in, sizeof(State), hipMemcpyHostToDevice);
    if (e != hipSuccess) return qcart::host::hip_fail(s->err, e, "qc_sched_state_import");
    s->ticks = s->first_tick = ticks;
    return QC_OK;
}

}  // extern "C"
