// qcart_monitor.hip — the cooling drivers' model ranking on the device (qc_monitor, include/qcart.h): one launch of
// one wave per receive that reads the new entries of the performance ring qc_env_tail appends to and runs
// receive_net's rule on the table of best window means (the state machine: qcart_monitor.hpp), then one asynchronous
// copy of the snapshot into the call's pinned host slot and one event record. qc_monitor_poll waits on that event
// alone. With train == 1 the kernel reads at most `window` entries; with train == 0 its walk is bounded by fin_cap.
// Nothing polls or waits.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/qcart.h"
#include "qcart_host.hpp"
#include "qcart_monitor.hpp"
#include "qcart_state.hpp"

namespace qcart {
namespace monitor {

constexpr int kWave = 64;

struct ReceiveArgs {
    State* st;
    const qc_monitor_params* p;
    qc_monitor_snapshot* snap;
    const double* perf;
    int64_t fin_cap;
    const int64_t* fin_n;
};

// The lanes load the ring entries, one each and coalesced, into LDS; lane 0 alone runs the state machine on the
// state in global memory (the table is indexed by a run-time rank: it stays in memory, not in registers).
__global__ __launch_bounds__(kWave) void k_monitor_receive(ReceiveArgs a) {
    __shared__ double buf[kWave];
    const int lane = (int)threadIdx.x;
    const qc_monitor_params p = *a.p;
    const int64_t fin_n = *a.fin_n;
    if (p.train) {
        const int64_t fresh = fresh_of(*a.st, fin_n);
        const int k = window_len(p, fresh);           // <= window <= 16 <= fin_cap: all present
        if (lane < k) buf[lane] = a.perf[(fin_n - k + lane) % a.fin_cap];
        __syncthreads();
        if (lane == 0) {
            qc_monitor_snapshot out;
            receive_train(*a.st, p, fin_n, [&](int j) { return buf[j]; }, out);
            *a.snap = out;
        }
        return;
    }
    // every lane takes the walk's bounds from the state as it was; lane 0 writes the state after the walk
    State& s = *a.st;
    const Walk w = test_walk(s, fin_n, a.fin_cap);
    Sums acc{s.sum, s.sumsq, s.n};
    __syncthreads();
    for (int64_t c = 0; c < w.fresh; c += kWave) {
        const int64_t left = w.fresh - c;
        const int m = left < kWave ? (int)left : kWave;
        if (lane < m) buf[lane] = a.perf[(w.first + c + lane) % a.fin_cap];
        __syncthreads();
        if (lane == 0)
            for (int j = 0; j < m; ++j) test_add(acc, buf[j]);
        __syncthreads();
    }
    if (lane == 0) {
        qc_monitor_snapshot out;
        test_finish(s, p, acc, w, out);
        *a.snap = out;
    }
}

__global__ void k_monitor_seek(State* st, const int64_t* fin_n) {
    if (threadIdx.x == 0 && blockIdx.x == 0) st->read = *fin_n;
}

}  // namespace monitor
}  // namespace qcart

using namespace qcart::monitor;
namespace st = qcart::state;

struct qc_monitor {
    qc_monitor_params p{};
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    int64_t calls = 0;                       // receives enqueued
    int64_t first_call = 0;                  // the first receive this handle ran itself (the count of an import)
    State* d_st = nullptr;
    qc_monitor_params* d_p = nullptr;
    qc_monitor_snapshot* d_snap = nullptr;   // [2]: call c writes slot c & 1
    qc_monitor_snapshot* h_snap = nullptr;   // pinned [2]
    hipEvent_t ev[2] = {nullptr, nullptr};
};

namespace {

using qcart::host::Dev;
qcart::host::CreateError g_monitor_err;

int mfail(qc_monitor* m, int code, const std::string& msg) {
    m->err = msg;
    return code;
}

}  // namespace

extern "C" {

int qc_monitor_create(const qc_monitor_params* p, int device, qc_monitor** out) {
    if (!out) return QC_EINVAL;
    *out = nullptr;
    if (const char* bad = bad_params(p)) return g_monitor_err.fail(std::string("qc_monitor_create: ") + bad, QC_EINVAL);
    if (const int rc = qcart::host::check_device(device, g_monitor_err, "the monitor")) return rc;
    qc_monitor* m = new qc_monitor();
    m->p = *p;
    m->device = device;
    Dev g(device);
    State init_state;
    init(init_state, m->p);
    hipError_t e = hipMalloc((void**)&m->d_st, sizeof(State));
    if (e == hipSuccess) e = hipMalloc((void**)&m->d_p, sizeof(qc_monitor_params));
    if (e == hipSuccess) e = hipMalloc((void**)&m->d_snap, 2 * sizeof(qc_monitor_snapshot));
    if (e == hipSuccess) e = hipHostMalloc((void**)&m->h_snap, 2 * sizeof(qc_monitor_snapshot), hipHostMallocDefault);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&m->ev[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemcpy(m->d_st, &init_state, sizeof(State), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m->d_p, &m->p, sizeof(qc_monitor_params), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(m->d_snap, 0, 2 * sizeof(qc_monitor_snapshot));
    if (e != hipSuccess) {
        const std::string msg = std::string("qc_monitor_create: ") + hipGetErrorString(e);
        qc_monitor_destroy(m);
        return g_monitor_err.fail(msg, QC_EHIP);
    }
    std::memset(m->h_snap, 0, 2 * sizeof(qc_monitor_snapshot));
    *out = m;
    return QC_OK;
}

void qc_monitor_destroy(qc_monitor* m) {
    if (!m) return;
    {
        Dev g(m->device);
        (void)hipDeviceSynchronize();
        for (void* q : {(void*)m->d_st, (void*)m->d_p, (void*)m->d_snap})
            if (q) (void)hipFree(q);
        if (m->h_snap) (void)hipHostFree(m->h_snap);
        for (hipEvent_t ev : m->ev)
            if (ev) (void)hipEventDestroy(ev);
    }
    delete m;
}

const char* qc_monitor_last_error(const qc_monitor* m) { return m ? m->err.c_str() : g_monitor_err.text(); }

int qc_monitor_set_stream(qc_monitor* m, void* stream) {
    if (!m) return QC_EINVAL;
    m->stream = (hipStream_t)stream;
    return QC_OK;
}

int qc_monitor_receive(qc_monitor* m, const double* perf, int64_t fin_cap, const int64_t* fin_n) {
    if (!m) return QC_EINVAL;
    if (!perf || !fin_n) return mfail(m, QC_EINVAL, "qc_monitor_receive: perf and fin_n are required");
    if (fin_cap < m->p.window)
        return mfail(m, QC_EINVAL, "qc_monitor_receive: fin_cap must be at least the window (" +
                                       std::to_string(m->p.window) + "): the last window entries must be present");
    Dev g(m->device);
    const int slot = (int)(m->calls & 1);
    ReceiveArgs a{};
    a.st = m->d_st;
    a.p = m->d_p;
    a.snap = m->d_snap + slot;
    a.perf = perf;
    a.fin_cap = fin_cap;
    a.fin_n = fin_n;
    hipLaunchKernelGGL(k_monitor_receive, dim3(1), dim3(kWave), 0, m->stream, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpyAsync(m->h_snap + slot, m->d_snap + slot, sizeof(qc_monitor_snapshot), hipMemcpyDeviceToHost,
                           m->stream);
    if (e == hipSuccess) e = hipEventRecord(m->ev[slot], m->stream);
    if (e != hipSuccess) return qcart::host::hip_fail(m->err, e, "qc_monitor_receive");
    m->calls += 1;
    return QC_OK;
}

int qc_monitor_seek(qc_monitor* m, const int64_t* fin_n) {
    if (!m) return QC_EINVAL;
    if (!fin_n) return mfail(m, QC_EINVAL, "qc_monitor_seek: fin_n is required");
    Dev g(m->device);
    hipLaunchKernelGGL(k_monitor_seek, dim3(1), dim3(1), 0, m->stream, m->d_st, fin_n);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? QC_OK : qcart::host::hip_fail(m->err, e, "qc_monitor_seek");
}

int qc_monitor_poll(qc_monitor* m, int64_t call, qc_monitor_snapshot* out) {
    if (!m || !out) return QC_EINVAL;
    if (call < m->first_call || call >= m->calls || call < m->calls - 2)
        return mfail(m, QC_EINVAL, "qc_monitor_poll: call " + std::to_string(call) + " is not one of the last two of " +
                                       std::to_string(m->calls) + " receives (receives before a state import stay with the handle that ran them)");
    Dev g(m->device);
    const int slot = (int)(call & 1);
    const hipError_t e = hipEventSynchronize(m->ev[slot]);
    if (e != hipSuccess) return qcart::host::hip_fail(m->err, e, "qc_monitor_poll");
    *out = m->h_snap[slot];
    return QC_OK;
}

int qc_monitor_table(qc_monitor* m, double* good, int32_t* filled) {
    if (!m) return QC_EINVAL;
    Dev g(m->device);
    State cur;
    hipError_t e = hipStreamSynchronize(m->stream);
    if (e == hipSuccess) e = hipMemcpy(&cur, m->d_st, sizeof(State), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return qcart::host::hip_fail(m->err, e, "qc_monitor_table");
    if (good) std::memcpy(good, cur.good, sizeof(double) * (size_t)m->p.num_of_saves);
    if (filled) std::memcpy(filled, cur.filled, sizeof(int32_t) * (size_t)m->p.num_of_saves);
    return QC_OK;
}

int qc_monitor_state_bytes(qc_monitor* m, uint64_t* n) {
    if (!m || !n) return QC_EINVAL;
    *n = sizeof(st::Header) + sizeof(State) + sizeof(int64_t);
    return QC_OK;
}

int qc_monitor_state_export(qc_monitor* m, void* host_dst, uint64_t n) {
    if (!m || !host_dst) return QC_EINVAL;
    const st::Header h = header(m->p);
    if (n != sizeof(st::Header) + h.payload_bytes)
        return mfail(m, QC_EINVAL, "qc_monitor_state_export: n differs from what qc_monitor_state_bytes gives");
    Dev g(m->device);
    State cur;
    hipError_t e = hipStreamSynchronize(m->stream);
    if (e == hipSuccess) e = hipMemcpy(&cur, m->d_st, sizeof(State), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return qcart::host::hip_fail(m->err, e, "qc_monitor_state_export");
    std::memcpy(host_dst, &h, sizeof(h));
    st::Cursor c(host_dst);
    std::memcpy(c.take(sizeof(State)), &cur, sizeof(State));
    std::memcpy(c.take(sizeof(int64_t)), &m->calls, sizeof(int64_t));
    return QC_OK;
}

int qc_monitor_state_import(qc_monitor* m, const void* host_src, uint64_t n) {
    if (!m) return QC_EINVAL;
    const st::Header mine = header(m->p);
    st::Header h;
    std::string bad = st::validate(host_src, n, mine, &h);
    const std::string who = "qc_monitor_state_import: ";
    if (bad.empty() && h.payload_bytes != mine.payload_bytes)
        bad = who + "payload_bytes: blob " + std::to_string(h.payload_bytes) + ", handle " +
              std::to_string(mine.payload_bytes);
    State in;
    int64_t calls = 0;
    if (bad.empty()) {
        const unsigned char* at = (const unsigned char*)host_src + sizeof(st::Header);
        std::memcpy(&in, at, sizeof(State));
        std::memcpy(&calls, at + sizeof(State), sizeof(int64_t));
        if (calls < 0 || in.calls != calls)
            bad = who + "receive count: blob " + std::to_string(calls) + ", its state " + std::to_string(in.calls);
        else if (in.read < 0 || in.count < 0 || in.episode_passed < 0 || in.n < 0 || in.total_episodes < 0)
            bad = who + "a counter of the blob's state is negative";
        else
            for (int i = 0; i < QC_MONITOR_MAX_SAVES && bad.empty(); ++i)
                if (in.filled[i] != 0 && (in.filled[i] != 1 || i >= m->p.num_of_saves))
                    bad = who + "filled[" + std::to_string(i) + "]: blob " + std::to_string(in.filled[i]) +
                          ", a flag of the handle's " + std::to_string(m->p.num_of_saves) + " entries is 0 or 1";
    }
    if (!bad.empty()) return mfail(m, QC_EINVAL, bad);
    Dev g(m->device);
    hipError_t e = hipStreamSynchronize(m->stream);
    if (e == hipSuccess) e = hipMemcpy(m->d_st, &in, sizeof(State), hipMemcpyHostToDevice);
    if (e != hipSuccess) return qcart::host::hip_fail(m->err, e, "qc_monitor_state_import");
    m->calls = m->first_call = calls;
    return QC_OK;
}

}  // extern "C"
