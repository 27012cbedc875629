// qcart_wigner.hip — the phase-space view of a batch of wavefunctions (qc_wigner, include/qcart.h): the Wigner function
// W[b][i][j] on the grid's own points x_i and the momenta p_j.
//
// With c_ik = conj(phi_{i+k}) phi_{i-k} the lag sum is a real contraction over (k, Re / Im):
//     W[i][j] = (2 h / pi) sum_{k = 0 .. K_i} ( Re c_ik * C[k][j] - Im c_ik * S[k][j] ),
// C[0] = 1/2, S[0] = 0 (the k = 0 term is |phi_i|^2, counted once), C, S[k >= 1] the table of qcart_wigner.hpp. It runs
// on v_mfma_f64_16x16x4_f64: A[row = position][k] is formed on the fly from the env's phi row held in LDS (lane
// (row, q) makes Re c and -Im c of lag k0 + q: two 16-byte LDS reads, four multiplies), B[k][col = momentum] is the
// table, one MFMA with (Re c, C) and one with (-Im c, S) per four lags and 16 x 16 outputs.
//
// A workgroup is one wave. It owns a quad of position tiles (16 positions each) and 64 momenta (4 column tiles): with
// T = ceil(x_n / 16) tiles, pair u = tiles (u, T - 1 - u) (mirror images: the same lag range), U = ceil(T / 2) pairs,
// quad v = pairs (v, U - 1 - v): a short pair next to a long one, so every quad does the same work although the
// contraction is triangular. A tile's lag loop stops at its largest K_i; a row with k > K_i, or past x_n, feeds exact
// zeros. The table operands of a lag step (4 lags x 64 momenta x (C, S): 8 doubles per lane) are loaded once and used
// by every tile of the quad and, in the mean, by every env of the LDS chunk; the next step's are in flight behind the
// MFMAs. The device table is padded with zeros to whole steps (4 lags) and whole column groups (64 momenta), so its
// loads need no guard; the epilogue's stores are guarded per element. Lanes of one q write 16 consecutive doubles of
// a row (128 bytes), so the output needs no transpose.
//
// k_wigner: one env per workgroup, W = scale * acc. k_wigner_mean<E>: the env index is one more contraction index; the
// accumulators run over the envs of the workgroup's split (order: include/qcart.h), E envs' rows in LDS at a time; an
// env past B or with a clear mask byte is a row of zeros. The splits' sums go to the handle's partials, which
// k_wigner_finish adds in order, scales and divides by the count k_wigner_count made. No per-env W is written.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/qcart.h"
#include "qcart_host.hpp"
#include "qcart_phase.hpp"
#include "qcart_wigner.hpp"
#include "qcart_wigner_tiles.hpp"

namespace qcart {
namespace wigner {

constexpr int kWave = 64;
constexpr int kMaxSplits = 256;
constexpr size_t kPartialCap = (size_t)1 << 23;   // doubles: the splits shrink so that the partials stay below this
using f64x4 = double __attribute__((ext_vector_type(4)));

struct Args {
    const double2* phi;      // [B][X]
    const double* T;         // [round_up(rows + 1, 4)][2][ldP]: row k = C[k][.], S[k][.]; zero outside [rows + 1][P]
    int B, X, P, ldP;        // ldP = round_up(P, 64)
    double scale;            // fl(2 h / pi)
    double* out;             // k_wigner: [B][X][P]
    const uint8_t* mask;     // mean: [B] or NULL
    double* partial;         // mean: [splits][X][P]
    int splits, chunks;      // mean: chunks = ceil(B / E); split s takes the chunks s, s + splits, ..
};

template <int E, bool MEAN>
__device__ __forceinline__ void body(const Args& a) {
    extern __shared__ double2 sPhi[];                // [E][X]
    const int lane = (int)threadIdx.x, row = lane & 15, q = lane >> 4;
    const int X = a.X, T = (X + 15) / 16, U = (T + 1) / 2;
    const int v = (int)blockIdx.y, j0 = (int)blockIdx.z * kTP;
    const int tile[4] = {v, T - 1 - v, U - 1 - v, T - 1 - (U - 1 - v)};
    const bool two = U - 1 - v != v;
    const bool on[4] = {true, tile[1] != tile[0], two, two && tile[3] != tile[2]};
    int kmax[4], pos[4], Ki[4], kend = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        kmax[t] = on[t] ? tile_kmax(16 * tile[t], X) : -1;
        kend = kmax[t] > kend ? kmax[t] : kend;
        pos[t] = 16 * tile[t] + row;
        const int far = X - 1 - pos[t];
        Ki[t] = pos[t] < X ? (pos[t] < far ? pos[t] : far) : -1;
    }
    f64x4 acc[4][kNT];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt) acc[t][nt] = f64x4{0., 0., 0., 0.};

    // the table operands of the step at lag k0: C and S of lag k0 + q at the momenta j0 + 16 nt + row
    // (k0 <= rows, so k0 + q < round_up(rows + 1, 4); j0 + 16 nt + row < ldP: inside the padded table)
    auto fetch = [&](int k0, double (&c)[kNT], double (&s)[kNT]) {
        const double* tp = a.T + (size_t)(k0 + q) * 2 * (size_t)a.ldP + (size_t)(j0 + row);
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt) {
            c[nt] = tp[16 * nt];
            s[nt] = tp[(size_t)a.ldP + 16 * nt];
        }
    };

    const int first = MEAN ? (int)blockIdx.x : 0, stride = MEAN ? a.splits : 1, chunks = MEAN ? a.chunks : 1;
    for (int chunk = first; chunk < chunks; chunk += stride) {
        __syncthreads();                             // the previous chunk's reads are done
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int b = MEAN ? chunk * E + e : (int)blockIdx.x;
            bool live = b < a.B;
            if (MEAN && live && a.mask != nullptr) live = a.mask[b] != 0;
            const double2* src = a.phi + (size_t)(live ? b : 0) * (size_t)X;
            for (int i = lane; i < X; i += kWave) sPhi[e * X + i] = live ? src[i] : make_double2(0., 0.);
        }
        __syncthreads();
        double tc[kNT], ts[kNT], nc[kNT], ns[kNT];
        fetch(0, tc, ts);
        for (int k0 = 0; k0 <= kend; k0 += kStep) {
            const bool more = k0 + kStep <= kend;
            if (more) fetch(k0 + kStep, nc, ns);     // in flight behind this step's MFMAs
            const int k = k0 + q;
#pragma unroll
            for (int e = 0; e < E; ++e) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (k0 > kmax[t]) continue;      // (wave-uniform; an absent tile has kmax = -1)
                    double re = 0., im = 0.;
                    if (k <= Ki[t]) {
                        const double2 up = sPhi[e * X + pos[t] + k], dn = sPhi[e * X + pos[t] - k];
                        re = up.x * dn.x + up.y * dn.y;
                        im = up.y * dn.x - up.x * dn.y;          // -Im(conj(up) dn)
                    }
#pragma unroll
                    for (int nt = 0; nt < kNT; ++nt) {
                        acc[t][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(re, tc[nt], acc[t][nt], 0, 0, 0);
                        acc[t][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(im, ts[nt], acc[t][nt], 0, 0, 0);
                    }
                }
            }
            if (more) {
#pragma unroll
                for (int nt = 0; nt < kNT; ++nt) {
                    tc[nt] = nc[nt];
                    ts[nt] = ns[nt];
                }
            }
        }
    }

    // D element r of tile (t, nt): position 16 tile[t] + q + 4 r, momentum j0 + 16 nt + row
    double* base = MEAN ? a.partial + (size_t)blockIdx.x * (size_t)X * (size_t)a.P
                        : a.out + (size_t)blockIdx.x * (size_t)X * (size_t)a.P;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (!on[t]) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * tile[t] + q + 4 * r;
#pragma unroll
            for (int nt = 0; nt < kNT; ++nt) {
                const int j = j0 + 16 * nt + row;
                if (i < X && j < a.P)
                    base[(size_t)i * (size_t)a.P + (size_t)j] = MEAN ? acc[t][nt][r] : a.scale * acc[t][nt][r];
            }
        }
    }
}

// (two waves per SIMD, 256 registers each with the 128 of the accumulators: one wave's LDS fill and table loads hide
// behind the other's MFMAs)
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(2))) void k_wigner(Args a) {
    body<1, false>(a);
}
template <int E>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(2))) void k_wigner_mean(Args a) {
    body<E, true>(a);
}

// count = the envs whose mask byte is set (no mask: B); one workgroup
constexpr int kThreads = 256;
__global__ __launch_bounds__(kThreads) void k_wigner_count(const uint8_t* mask, int B, int64_t* count) {
    __shared__ long long cnt[kThreads];
    const int tid = (int)threadIdx.x;
    long long c = 0;
    if (mask != nullptr)
        for (int b = tid; b < B; b += kThreads) c += mask[b] != 0 ? 1 : 0;
    cnt[tid] = c;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (tid < w) cnt[tid] += cnt[tid + w];
        __syncthreads();
    }
    if (tid == 0) *count = mask != nullptr ? (int64_t)cnt[0] : (int64_t)B;
}

// out[e] = fl(fl(scale * t) / count), t = the running sum, from +0, of the splits' partials 0, 1, 2, .. in that order;
// count == 0: zeros, no division
__global__ __launch_bounds__(kThreads) void k_wigner_finish(const double* partial, int splits, size_t n, double scale,
                                                            const int64_t* count, double* out) {
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    const int64_t c = *count;
    double t = 0.;
#pragma unroll 8
    for (int s = 0; s < splits; ++s) t = t + partial[(size_t)s * n + e];
    const double w = scale * t;
    out[e] = c > 0 ? w / (double)c : 0.;
}

}  // namespace wigner
}  // namespace qcart

using namespace qcart::wigner;

struct qc_wigner {
    int32_t x_n = 0, P = 0, ldP = 0;
    double h = 0., scale = 0.;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    double* d_T = nullptr;       // [round_up(rows + 1, 4)][2][ldP]
    double* d_partial = nullptr; // [max_splits][x_n][P], made at create time: no call allocates
    int max_splits = 0;          // qc_wigner_splits of any B is at most this
    int64_t* d_count = nullptr;  // the count of a mean whose caller asked for none
};

namespace {

using qcart::host::Dev;
qcart::host::CreateError g_wigner_err;

int wfail(qc_wigner* w, int code, const std::string& msg) {
    w->err = msg;
    return code;
}

int check_call(qc_wigner* w, const char* who, const void* phi, int32_t B, const void* out) {
    const std::string pre = std::string(who) + ": ";
    if (!phi || !out) return wfail(w, QC_EINVAL, pre + "phi and out are required");
    // (the upper end keeps the env index of a chunk's padding inside int32)
    if (B < 1 || B > INT32_MAX - 8) return wfail(w, QC_EINVAL, pre + "B must be >= 1");
    return QC_OK;
}

Args make_args(const qc_wigner* w, const void* phi, int32_t B) {
    Args a{};
    a.phi = (const double2*)phi;
    a.T = w->d_T;
    a.B = B;
    a.X = w->x_n;
    a.P = w->P;
    a.ldP = w->ldP;
    a.scale = w->scale;
    return a;
}

// the quads of position tiles and the groups of 64 momenta
unsigned quads(int32_t X) { return tile_quads(X); }
unsigned groups(int32_t P) { return momentum_groups(P); }

int launched(qc_wigner* w, const char* who) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? QC_OK : qcart::host::hip_fail(w->err, e, who);
}

}  // namespace

extern "C" {

int qc_wigner_create(int32_t x_n, double h, const double* p, int32_t P, int device, qc_wigner** out) {
    if (!out) return QC_EINVAL;
    *out = nullptr;
    if (const char* bad = bad_wigner(x_n, h, p, P))
        return g_wigner_err.fail(std::string("qc_wigner_create: ") + bad, QC_EINVAL);
    const int32_t rows = table_rows(x_n), ldP = (P + kTP - 1) / kTP * kTP;
    const int32_t padded_rows = (rows + 1 + kStep - 1) / kStep * kStep;
    std::vector<double> table((size_t)(rows > 0 ? rows : 1) * (size_t)P * 2);
    const char* why = nullptr;
    if (qc_wigner_build_table(x_n, h, p, P, table.data(), &why) != QC_OK)
        return g_wigner_err.fail(std::string("qc_wigner_create: ") + (why ? why : "table"), QC_EINVAL);
    std::vector<double> padded((size_t)padded_rows * 2 * (size_t)ldP, 0.);
    for (int32_t j = 0; j < P; ++j) padded[(size_t)j] = 0.5;      // lag 0: |phi_i|^2 counted once, no sine
    for (int32_t k = 1; k <= rows; ++k)
        for (int32_t j = 0; j < P; ++j) {
            const double* at = table.data() + ((size_t)(k - 1) * (size_t)P + (size_t)j) * 2;
            padded[((size_t)k * 2 + 0) * (size_t)ldP + (size_t)j] = at[0];
            padded[((size_t)k * 2 + 1) * (size_t)ldP + (size_t)j] = at[1];
        }
    if (const int rc = qcart::host::check_device(device, g_wigner_err, "the phase-space view")) return rc;
    qc_wigner* w = new qc_wigner();
    w->x_n = x_n;
    w->P = P;
    w->ldP = ldP;
    w->h = h;
    w->scale = (double)(2.0L * (long double)h / 3.14159265358979323846264338327950288L);
    w->device = device;
    Dev g(device);
    hipError_t e = hipMalloc((void**)&w->d_T, padded.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(w->d_T, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&w->d_count, sizeof(int64_t));
    // the mean's partials for the largest number of splits any B can ask for (at most 2^23 doubles, 64 MiB)
    w->max_splits = qc_wigner_splits(INT32_MAX, x_n, P);
    if (e == hipSuccess)
        e = hipMalloc((void**)&w->d_partial, (size_t)w->max_splits * (size_t)x_n * (size_t)P * sizeof(double));
    if (e != hipSuccess) {
        const std::string msg = std::string("qc_wigner_create: ") + hipGetErrorString(e);
        qc_wigner_destroy(w);
        return g_wigner_err.fail(msg, QC_EHIP);
    }
    *out = w;
    return QC_OK;
}

void qc_wigner_destroy(qc_wigner* w) {
    if (!w) return;
    {
        Dev g(w->device);
        (void)hipDeviceSynchronize();
        if (w->d_T) (void)hipFree(w->d_T);
        if (w->d_partial) (void)hipFree(w->d_partial);
        if (w->d_count) (void)hipFree(w->d_count);
    }
    delete w;
}

const char* qc_wigner_last_error(const qc_wigner* w) { return w ? w->err.c_str() : g_wigner_err.text(); }

int qc_wigner_set_stream(qc_wigner* w, void* stream) {
    if (!w) return QC_EINVAL;
    w->stream = (hipStream_t)stream;
    return QC_OK;
}

int qc_wigner_eval(qc_wigner* w, const void* phi, int32_t B, double* out) {
    if (!w) return QC_EINVAL;
    if (const int rc = check_call(w, "qc_wigner_eval", phi, B, out)) return rc;
    Dev g(w->device);
    Args a = make_args(w, phi, B);
    a.out = out;
    hipLaunchKernelGGL(k_wigner, dim3((unsigned)B, quads(w->x_n), groups(w->P)), dim3(kWave),
                       (size_t)w->x_n * sizeof(double2), w->stream, a);
    return launched(w, "qc_wigner_eval");
}

int qc_wigner_mean(qc_wigner* w, const void* phi, int32_t B, const uint8_t* mask, double* out, int64_t* count) {
    if (!w) return QC_EINVAL;
    if (const int rc = check_call(w, "qc_wigner_mean", phi, B, out)) return rc;
    Dev g(w->device);
    const int E = qc_wigner_chunk(w->x_n);
    const int chunks = (int)(((int64_t)B + E - 1) / E);
    const int splits = qc_wigner_splits(B, w->x_n, w->P);
    const size_t n = (size_t)w->x_n * (size_t)w->P;
    if (splits < 1 || splits > w->max_splits) return wfail(w, QC_EINVAL, "qc_wigner_mean: the splits exceed the partials");
    int64_t* cnt = count ? count : w->d_count;
    hipLaunchKernelGGL(k_wigner_count, dim3(1), dim3(kThreads), 0, w->stream, mask, B, cnt);
    if (const int rc = launched(w, "qc_wigner_mean")) return rc;
    Args a = make_args(w, phi, B);
    a.mask = mask;
    a.partial = w->d_partial;
    a.splits = splits;
    a.chunks = chunks;
    const dim3 grid((unsigned)splits, quads(w->x_n), groups(w->P));
    const size_t lds = (size_t)E * (size_t)w->x_n * sizeof(double2);
    if (E == 2)
        hipLaunchKernelGGL(k_wigner_mean<2>, grid, dim3(kWave), lds, w->stream, a);
    else
        hipLaunchKernelGGL(k_wigner_mean<1>, grid, dim3(kWave), lds, w->stream, a);
    if (const int rc = launched(w, "qc_wigner_mean")) return rc;
    hipLaunchKernelGGL(k_wigner_finish, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, w->stream,
                       (const double*)w->d_partial, splits, n, w->scale, (const int64_t*)cnt, out);
    return launched(w, "qc_wigner_mean");
}

int qc_wigner_eval_rho(qc_wigner* w, const void* rho, int32_t M, double* out) {
    if (!w) return QC_EINVAL;
    const char* who = "qc_wigner_eval_rho";
    if (!rho || !out) return wfail(w, QC_EINVAL, std::string(who) + ": rho and out are required");
    if (M < 1) return wfail(w, QC_EINVAL, std::string(who) + ": M must be >= 1");
    if ((int64_t)M * w->x_n * w->x_n > ((int64_t)1 << 27))
        return wfail(w, QC_EINVAL, std::string(who) + ": M x_n^2 must be <= 2^27");
    Dev g(w->device);
    // (the table of the handle, its lag-0 row (1/2, 0) included; the scale fl(2 / pi) has no h: rho carries it)
    const hipError_t e = qcart::phase::launch_wigner(w->d_T, w->x_n, w->P, w->ldP, rho, M, out, w->stream);
    return e == hipSuccess ? QC_OK : qcart::host::hip_fail(w->err, e, who);
}

int qc_wigner_chunk(int32_t x_n) { return x_n <= 512 ? 2 : 1; }

int qc_wigner_splits(int32_t B, int32_t x_n, int32_t P) {
    if (B < 1 || x_n < 1 || P < 1) return 0;
    const int E = qc_wigner_chunk(x_n);
    const size_t chunks = ((size_t)B + (size_t)E - 1) / (size_t)E, fit = kPartialCap / ((size_t)x_n * (size_t)P);
    size_t s = chunks < (size_t)kMaxSplits ? chunks : (size_t)kMaxSplits;
    if (s > fit) s = fit;
    return s < 1 ? 1 : (int)s;
}

}  // extern "C"
