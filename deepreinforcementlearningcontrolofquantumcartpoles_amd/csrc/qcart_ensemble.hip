// qcart_ensemble.hip — the ensemble density matrix of a batch of states (qc_ensemble, include/qcart.h):
//     rho[m][n] = fl(fl(scale * t[m][n]) / count),  t[m][n] = sum over the live envs b of psi_b[m] conj(psi_b[n]).
//
// With psi = a + i b the complex rank-B update is a real contraction over (env, re / im):
//     Re t[m][n] = sum_b (a_m a_n + b_m b_n),   Im t[m][n] = sum_b (b_m a_n - a_m b_n).
// It runs on v_mfma_f64_16x16x4_f64, the K = 4 of one MFMA being 2 envs x (re, im): lane (row, q) holds k = q, env
// q >> 1 of the chunk, part q & 1. The B operand of a column tile is B[k][col] = (a, b)[part] of psi_env[n0 + col], the
// A operand of the real part is the same (a, b)[part] of the row tile's element, the A operand of the imaginary part
// is (b, -a)[part]. The operands come straight from global memory / L2: the 16 lanes of one q read 16 consecutive
// complex elements (a row operand: 256 contiguous bytes; a column operand: one double of each); a workgroup is one
// wave, so there is nothing LDS could share, and the next chunk's operands are in flight behind the current chunk's
// MFMAs.
//
// A workgroup is one wave. It owns a block of 64 rows x 32 columns x {Re, Im} (4 x 2 x 2 accumulator tiles, 128
// registers) on or below the diagonal and one split of the envs: block t of the triangular list is row block I,
// column block J <= 2 I + 1 with t = I (I + 1) + J; blocks strictly above the diagonal are not launched, tiles
// strictly above it inside a diagonal block, and tiles that start past N, are skipped. A row or column past N, a
// masked env and an env past B feed exact zeros (selected, never multiplied: what their memory holds does not come
// through). The accumulators go to the handle's partials [S][2][N][N]; stores are guarded per element, 64-bit offsets.
//
// k_ensemble_count counts the mask. k_ensemble_finish takes the running sum of the splits' partials in order, scales,
// divides, writes rho[m][n] for n <= m and rho[n][m] = conj(rho[m][n]) from the same value, and +0.0 as the
// diagonal's imaginary part (the chain b a + (-a) b leaves a rounding residue there).
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "../../include/qcart.h"
#include "qcart_ensemble.hpp"
#include "qcart_host.hpp"

namespace qcart {
namespace ensemble {

constexpr int kWave = 64;
constexpr int kMT = 4, kNT = 2;        // row tiles and column tiles of a block: 64 x 32
using f64x4 = double __attribute__((ext_vector_type(4)));

struct Args {
    const double2* psi;      // [B][N]
    const uint8_t* mask;     // [B], or the handle's constant 1 with mask_stride = 0
    int mask_stride;
    const double2* zero;     // one complex zero (the handle's)
    double* partial;         // [splits][2][N][N]
    int B, N;
    int splits, chunks;      // chunks = ceil(B / 2); split s takes the chunks s, s + splits, ..
};

struct Operands {
    double2 r[kMT];          // the row tiles' elements of this lane's env
    double c[kNT];           // the column tiles' elements, this lane's part
};

__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(2))) void k_ensemble(Args a) {
    const int lane = (int)threadIdx.x, row = lane & 15, q = lane >> 4, env = q >> 1, part = q & 1;
    const int N = a.N;
    // block t = I (I + 1) + J, 0 <= J <= 2 I + 1
    const int t = (int)blockIdx.x;
    int I = (int)((sqrtf(4.f * (float)t + 1.f) - 1.f) * 0.5f);
    while (I * (I + 1) > t) --I;
    while ((I + 1) * (I + 2) <= t) ++I;
    const int J = t - I * (I + 1);
    const int m0 = 64 * I, n0 = 32 * J;
    if (n0 >= N) return;                             // (the last row block's columns may end before 2 I + 1)

    int ri[kMT], ci[kNT];
    bool rok[kMT], cok[kNT], on[kMT][kNT];
#pragma unroll
    for (int i = 0; i < kMT; ++i) {
        ri[i] = m0 + 16 * i + row;
        rok[i] = ri[i] < N;
    }
#pragma unroll
    for (int j = 0; j < kNT; ++j) {
        ci[j] = n0 + 16 * j + row;
        cok[j] = ci[j] < N;
    }
#pragma unroll
    for (int i = 0; i < kMT; ++i)
#pragma unroll
        for (int j = 0; j < kNT; ++j)
            on[i][j] = 2 * J + j <= 4 * I + i && m0 + 16 * i < N && n0 + 16 * j < N;

    f64x4 re[kMT][kNT], im[kMT][kNT];
#pragma unroll
    for (int i = 0; i < kMT; ++i)
#pragma unroll
        for (int j = 0; j < kNT; ++j) re[i][j] = im[i][j] = f64x4{0., 0., 0., 0.};

    // Whether this lane's env of chunk c enters: inside B with its mask byte set. Without a mask the byte read is the
    // handle's constant 1 (mask_stride = 0); the index is clamped, so the load needs no guard.
    auto live_byte = [&](int c) -> uint8_t {
        const long long b = 2ll * c + env;
        return a.mask[(size_t)(b < (long long)a.B ? b : 0) * (size_t)a.mask_stride];
    };
    auto inside = [&](int c) -> bool { return 2ll * c + env < (long long)a.B; };
    // The operands of chunk c. A lane whose env does not enter, or whose row / column lies past N, reads the handle's
    // zeros instead: the address is selected, so every load is unconditional and nothing is multiplied by 0.
    auto fetch = [&](int c, bool live, Operands& o) {
        const double2* src = a.psi + (size_t)(2ll * c + env) * (size_t)N;
#pragma unroll
        for (int i = 0; i < kMT; ++i) o.r[i] = *(live && rok[i] ? src + ri[i] : a.zero);
#pragma unroll
        for (int j = 0; j < kNT; ++j)
            o.c[j] = *((const double*)(live && cok[j] ? src + ci[j] : a.zero) + part);
    };

    // Chunk c's MFMAs run while chunk c + S's operands and chunk c + 2 S's mask byte are in flight: every load of an
    // iteration is unconditional (past the split's last chunk the chunk index is clamped and the lanes read the zeros)
    // and is first needed at the iteration's end. A block with every tile on (FULL) runs a loop of one basic block.
    Operands cur, nxt;
    const int first = (int)blockIdx.y, stride = a.splits;
    if (first >= a.chunks) return;                   // (S <= chunks: not taken)
    fetch(first, inside(first) && live_byte(first) != 0, cur);
    bool live1 = first + stride < a.chunks && inside(first + stride) && live_byte(first + stride) != 0;
    __builtin_amdgcn_s_waitcnt(0);                   // nothing is pending at the loop's head
    auto run = [&](auto full) {
        constexpr bool FULL = decltype(full)::value;
        for (int c = first; c < a.chunks; c += stride) {
            const bool more = c + stride < a.chunks, more2 = more && c + 2 * stride < a.chunks;
            const int c1 = more ? c + stride : c, c2 = more2 ? c + 2 * stride : c;
            const uint8_t byte2 = live_byte(c2);
            fetch(c1, live1, nxt);
#pragma unroll
            for (int i = 0; i < kMT; ++i) {
                const double are = part ? cur.r[i].y : cur.r[i].x;       // (a, b)
                const double aim = part ? -cur.r[i].x : cur.r[i].y;      // (b, -a)
#pragma unroll
                for (int j = 0; j < kNT; ++j) {
                    if (!FULL && !on[i][j]) continue;                    // (wave-uniform)
                    re[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(are, cur.c[j], re[i][j], 0, 0, 0);
                    im[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(aim, cur.c[j], im[i][j], 0, 0, 0);
                }
            }
            cur = nxt;
            live1 = more2 && inside(c2) && byte2 != 0;
        }
    };
    bool all_on = true;
#pragma unroll
    for (int i = 0; i < kMT; ++i)
#pragma unroll
        for (int j = 0; j < kNT; ++j) all_on = all_on && on[i][j];
    if (all_on)
        run(std::true_type{});
    else
        run(std::false_type{});

    // D element r of tile (i, j): row m0 + 16 i + q + 4 r, column n0 + 16 j + row
    const size_t plane = (size_t)N * (size_t)N;
    double* base = a.partial + (size_t)blockIdx.y * 2 * plane;
#pragma unroll
    for (int i = 0; i < kMT; ++i)
#pragma unroll
        for (int j = 0; j < kNT; ++j) {
            if (!on[i][j]) continue;
            const int n = n0 + 16 * j + row;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + 16 * i + q + 4 * r;
                if (m < N && n < N) {
                    const size_t at = (size_t)m * (size_t)N + (size_t)n;
                    base[at] = re[i][j][r];
                    base[plane + at] = im[i][j][r];
                }
            }
        }
}

// count = the envs whose mask byte is set (no mask: B); one workgroup
constexpr int kThreads = 256;
__global__ __launch_bounds__(kThreads) void k_ensemble_count(const uint8_t* mask, int B, int64_t* count) {
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

// For n <= m: v = fl(fl(scale * t) / count) of the real and of the imaginary part, t = the running sum, from +0, of
// the splits' partials 0, 1, 2, .. in that order; rho[m][n] = (v_re, v_im), rho[n][m] = (v_re, -v_im); on the diagonal
// the imaginary part is +0.0. count == 0: v = +0, no division.
__global__ __launch_bounds__(kThreads) void k_ensemble_finish(const double* partial, int splits, int N, double scale,
                                                              const int64_t* count, double2* rho) {
#pragma clang fp contract(off)
    const size_t plane = (size_t)N * (size_t)N;
    const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= plane) return;
    const int m = (int)(e / (size_t)N), n = (int)(e % (size_t)N);
    if (n > m) return;
    const int64_t c = *count;
    double tr = 0., ti = 0.;
#pragma unroll 4
    for (int s = 0; s < splits; ++s) {
        const double* p = partial + (size_t)s * 2 * plane + e;
        tr = tr + p[0];
        ti = ti + p[plane];
    }
    const double wr = scale * tr, wi = scale * ti;
    const double vr = c > 0 ? wr / (double)c : 0., vi = c > 0 ? wi / (double)c : 0.;
    if (m == n) {
        rho[e] = make_double2(vr, 0.);
    } else {
        rho[e] = make_double2(vr, vi);
        rho[(size_t)n * (size_t)N + (size_t)m] = make_double2(vr, -vi);
    }
}

}  // namespace ensemble
}  // namespace qcart

using namespace qcart::ensemble;

struct qc_ensemble {
    int32_t N = 0;
    double scale = 0.;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    double* d_partial = nullptr; // [max_splits][2][N][N], made at create time: no call allocates
    int max_splits = 0;          // qc_ensemble_splits of any B is at most this
    int64_t* d_count = nullptr;  // the count of a call whose caller asked for none
    uint8_t* d_const = nullptr;  // 16 zero bytes (the operand of what does not enter), then one byte 1 (no mask)
};

namespace {

using qcart::host::Dev;
qcart::host::CreateError g_ensemble_err;

int efail(qc_ensemble* h, int code, const std::string& msg) {
    h->err = msg;
    return code;
}

int launched(qc_ensemble* h, const char* who) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? QC_OK : qcart::host::hip_fail(h->err, e, who);
}

// the blocks of 64 x 32 on or below the diagonal: row block I has the column blocks 0 .. 2 I + 1
unsigned blocks(int32_t N) {
    const unsigned rb = (unsigned)((N + 63) / 64);
    return rb * (rb + 1);
}

}  // namespace

extern "C" {

int qc_ensemble_create(int32_t N, double scale, int device, qc_ensemble** out) {
    if (!out) return QC_EINVAL;
    *out = nullptr;
    if (const char* bad = bad_create(N, scale))
        return g_ensemble_err.fail(std::string("qc_ensemble_create: ") + bad, QC_EINVAL);
    if (const int rc = qcart::host::check_device(device, g_ensemble_err, "the ensemble view")) return rc;
    qc_ensemble* h = new qc_ensemble();
    h->N = N;
    h->scale = scale;
    h->device = device;
    h->max_splits = max_splits(N);
    Dev g(device);
    hipError_t e = hipMalloc((void**)&h->d_count, sizeof(int64_t));
    const uint8_t consts[32] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_const, sizeof(consts));
    if (e == hipSuccess) e = hipMemcpy(h->d_const, consts, sizeof(consts), hipMemcpyHostToDevice);
    // the partials for the largest number of splits any B can ask for (at most 2^23 doubles, 64 MiB)
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_partial, partial_doubles(N) * sizeof(double));
    if (e != hipSuccess) {
        const std::string msg = std::string("qc_ensemble_create: ") + hipGetErrorString(e);
        qc_ensemble_destroy(h);
        return g_ensemble_err.fail(msg, QC_EHIP);
    }
    *out = h;
    return QC_OK;
}

void qc_ensemble_destroy(qc_ensemble* h) {
    if (!h) return;
    {
        Dev g(h->device);
        (void)hipDeviceSynchronize();
        if (h->d_partial) (void)hipFree(h->d_partial);
        if (h->d_count) (void)hipFree(h->d_count);
        if (h->d_const) (void)hipFree(h->d_const);
    }
    delete h;
}

const char* qc_ensemble_last_error(const qc_ensemble* h) { return h ? h->err.c_str() : g_ensemble_err.text(); }

int qc_ensemble_set_stream(qc_ensemble* h, void* stream) {
    if (!h) return QC_EINVAL;
    h->stream = (hipStream_t)stream;
    return QC_OK;
}

int qc_ensemble_density(qc_ensemble* h, const void* psi, int32_t B, const uint8_t* mask, void* rho, int64_t* count) {
    if (!h) return QC_EINVAL;
    if (const char* bad = bad_call(psi, B, rho)) return efail(h, QC_EINVAL, std::string("qc_ensemble_density: ") + bad);
    const int S = splits(B, h->N);
    if (S < 1 || S > h->max_splits) return efail(h, QC_EINVAL, "qc_ensemble_density: the splits exceed the partials");
    Dev g(h->device);
    int64_t* cnt = count ? count : h->d_count;
    hipLaunchKernelGGL(k_ensemble_count, dim3(1), dim3(kThreads), 0, h->stream, mask, B, cnt);
    if (const int rc = launched(h, "qc_ensemble_density")) return rc;
    Args a{};
    a.psi = (const double2*)psi;
    a.mask = mask ? mask : h->d_const + 16;
    a.mask_stride = mask ? 1 : 0;
    a.zero = (const double2*)h->d_const;
    a.partial = h->d_partial;
    a.B = B;
    a.N = h->N;
    a.splits = S;
    a.chunks = (int)chunks(B);
    hipLaunchKernelGGL(k_ensemble, dim3(blocks(h->N), (unsigned)S), dim3(kWave), 0, h->stream, a);
    if (const int rc = launched(h, "qc_ensemble_density")) return rc;
    const size_t plane = (size_t)h->N * (size_t)h->N;
    hipLaunchKernelGGL(k_ensemble_finish, dim3((unsigned)((plane + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       h->stream, (const double*)h->d_partial, S, (int)h->N, h->scale, (const int64_t*)cnt,
                       (double2*)rho);
    return launched(h, "qc_ensemble_density");
}

int qc_ensemble_chunk(int32_t N) { return chunk(N); }

int qc_ensemble_splits(int32_t B, int32_t N) { return splits(B, N); }

}  // extern "C"
