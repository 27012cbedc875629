// qcart_spatial.hip — the position-space view of a batch of states (qc_spatial, include/qcart.h): the drivers'
// spatial_repr and probability (HO/main_parallel.py:47-51, 82-86) next to psi on the device.
//
// Fock mode: phi[b][j] = sum_n E[j][n] c[b][n], a dense fp64 contraction [B][n_state] complex x [n_state][X] real on
// v_mfma_f64_16x16x4_f64. A = the states (rows = envs), B = the table (columns = points), two accumulator sets (Re,
// Im) sharing the E operand. A workgroup of four waves owns 32 envs x 256 points; wave w owns the points
// 64 w .. 64 w + 63 as 2 x 4 MFMA tiles. psi and E go through LDS in chunks of 16 levels; the next chunk's global
// loads are issued before the current chunk's MFMAs and land in registers behind them. The ragged edges: the device
// table is padded with zeros to whole tiles (256 points, 16 levels), so its loads need no guard and stay inside the
// allocation; a psi load is guarded (b < B, n < n_state), a lane out of range does not load and puts a zero into
// LDS, as does a level with |c| <= threshold; the epilogue's stores are guarded per element. The K order of an output
// element is fixed: chunk after chunk, within a chunk one MFMA per four levels, so phi[b] does not depend on B or on
// env b's place in a tile. One body, three epilogues: k_spatial_repr writes phi, k_spatial_probability writes
// fl(fl(Re^2) + fl(Im^2)), both through an LDS transpose so that a row of the output is written by consecutive
// lanes; k_spatial_mean adds the densities over the workgroup's 32 envs (order: include/qcart.h) into the handle's
// partials, which k_spatial_finish, one workgroup, adds in order. Grid mode (n_levels == 0) has the same formula and
// order on psi itself.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/qcart.h"
#include "qcart_host.hpp"
#include "qcart_phase.hpp"
#include "qcart_spatial.hpp"

namespace qcart {
namespace spatial {

constexpr int kThreads = 256;
constexpr int kTB = 32;          // envs per workgroup: two MFMA row tiles; also the group of the mean's first stage
constexpr int kTX = 256;         // points per workgroup: four waves x four MFMA column tiles
constexpr int kKC = 16;          // levels per LDS chunk
constexpr int kLd = kKC + 1;     // LDS row stride in doubles
constexpr int kSt = kTX + 1;     // row stride of the epilogue's transpose, which reuses the E tile's LDS
static_assert(16 * kSt <= kTX * kLd, "the epilogue stages 16 rows of doubles (8 of complex) in the E tile");
using f64x4 = double __attribute__((ext_vector_type(4)));

enum { kRepr = 0, kProb = 1, kMean = 2 };

struct Args {
    const double2* psi;      // [B][n_state]
    const double* E;         // [round_up(X, 256)][ldE], zero outside [X][n_levels]
    int B, n_state, ldE, X;  // ldE = round_up(n_levels, 16)
    double threshold;
    double2* phi;            // kRepr: [B][X]
    double* p;               // kProb: [B][X]
    const uint8_t* mask;     // kMean: [B] or NULL
    double* partial;         // kMean: [ceil(B / 32)][X]
};

__device__ __forceinline__ double density(double re, double im) {
#pragma clang fp contract(off)
    const double a = re * re, b = im * im;
    return a + b;
}

// the sum of four running sums, here and one level up: (s[0] + s[1]) + (s[2] + s[3])
__device__ __forceinline__ double join4(double s0, double s1, double s2, double s3) {
#pragma clang fp contract(off)
    const double a = s0 + s1, b = s2 + s3;
    return a + b;
}

template <int MODE>
__device__ __forceinline__ void body(const Args& a) {
    __shared__ double sRe[kTB * kLd], sIm[kTB * kLd], sE[kTX * kLd];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = (int)blockIdx.x * kTB, j0 = (int)blockIdx.y * kTX;
    const int lk = tid & 15, lr = tid >> 4;          // the loaders: level within the chunk, row 0 .. 15
    const int row = lane & 15, q = lane >> 4;        // MFMA operands: A[row][k = q], B[k = q][col = row]
    f64x4 accRe[2][4], accIm[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) accRe[mt][nt] = accIm[mt][nt] = f64x4{0., 0., 0., 0.};

    // one chunk in registers: this thread's 2 amplitudes and 16 table entries of level k0 + lk
    double2 c[kTB / 16];
    double e[kTX / 16];
    auto fetch = [&](int k0) {
        const int k = k0 + lk;
#pragma unroll
        for (int i = 0; i < kTB / 16; ++i) {
            const int b = b0 + lr + 16 * i;
            c[i] = make_double2(0., 0.);
            if (k < a.n_state && b < a.B) c[i] = a.psi[(size_t)b * (size_t)a.n_state + (size_t)k];
        }
        // (row j0 + lr + 16 i < round_up(X, 256), column k < round_up(n_state, 16) <= ldE: inside the padded table)
        const double* ep = a.E + (size_t)(j0 + lr) * (size_t)a.ldE + (size_t)k;
#pragma unroll
        for (int i = 0; i < kTX / 16; ++i) e[i] = ep[(size_t)(16 * i) * (size_t)a.ldE];
    };

    // kMean: thread t < 32 reads whether env b0 + t takes part (one guarded load, in flight behind the main loop)
    __shared__ unsigned char sLive[kTB];
    unsigned char mine = tid < kTB && b0 + tid < a.B ? 1 : 0;
    if (MODE == kMean && a.mask != nullptr && mine) mine = a.mask[b0 + tid];

    fetch(0);
    for (int k0 = 0; k0 < a.n_state; k0 += kKC) {
        __syncthreads();                              // the previous chunk's reads are done
#pragma unroll
        for (int i = 0; i < kTB / 16; ++i) {
            const bool keep = hypot(c[i].x, c[i].y) > a.threshold;
            sRe[(lr + 16 * i) * kLd + lk] = keep ? c[i].x : 0.;
            sIm[(lr + 16 * i) * kLd + lk] = keep ? c[i].y : 0.;
        }
#pragma unroll
        for (int i = 0; i < kTX / 16; ++i) sE[(lr + 16 * i) * kLd + lk] = e[i];
        __syncthreads();
        if (k0 + kKC < a.n_state) fetch(k0 + kKC);    // in flight behind this chunk's MFMAs
        const int left = a.n_state - k0, kend = left < kKC ? left : kKC;
        for (int kk = 0; kk < kend; kk += 4) {       // (levels kk .. kk + 3 < kKC: zero amplitudes past n_state)
            double ar[2], ai[2], eb[4];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                ar[mt] = sRe[(mt * 16 + row) * kLd + kk + q];
                ai[mt] = sIm[(mt * 16 + row) * kLd + kk + q];
            }
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) eb[nt] = sE[(wave * 64 + nt * 16 + row) * kLd + kk + q];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    accRe[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[mt], eb[nt], accRe[mt][nt], 0, 0, 0);
                    accIm[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[mt], eb[nt], accIm[mt][nt], 0, 0, 0);
                }
        }
    }

    // D element r of tile (mt, nt): env b0 + 16 mt + q + 4 r, point j0 + 64 wave + 16 nt + row
    if constexpr (MODE == kMean) {
        if (tid < kTB) sLive[tid] = mine;
        __syncthreads();
        bool live[2][4];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) live[mt][r] = sLive[mt * 16 + q + 4 * r] != 0;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            double s = 0.;
            {
#pragma clang fp contract(off)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        s = s + (live[mt][r] ? density(accRe[mt][nt][r], accIm[mt][nt][r]) : 0.);
            }
            // every lane takes part in the exchange: s[q ^ 1], then the other pair's sum
            const double t = s + __shfl_xor(s, 16);
            const double u = t + __shfl_xor(t, 32);
            const int j = j0 + wave * 64 + nt * 16 + row;
            if (q == 0 && j < a.X) a.partial[(size_t)blockIdx.x * (size_t)a.X + (size_t)j] = u;
        }
    } else {
        // kRows env rows at a time through LDS (the E tile's, free now): thread t then writes point j0 + t of each row
        constexpr int kRows = MODE == kRepr ? 8 : 16;
        double* stage = sE;
#pragma unroll
        for (int pass = 0; pass < kTB / kRows; ++pass) {
            __syncthreads();                          // the MFMA loop's, or the previous pass's, reads are done
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // local env 16 mt + q + 4 r belongs to pass (16 mt + 4 r) / kRows, whatever q < 4 is
                    if ((16 * mt + 4 * r) / kRows != pass) continue;
                    const int lrow = 16 * mt + 4 * r - pass * kRows + q;
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        const int col = wave * 64 + nt * 16 + row;
                        if (MODE == kRepr) {
                            stage[lrow * kSt + col] = accRe[mt][nt][r];
                            stage[(kRows + lrow) * kSt + col] = accIm[mt][nt][r];
                        } else {
                            stage[lrow * kSt + col] = density(accRe[mt][nt][r], accIm[mt][nt][r]);
                        }
                    }
                }
            __syncthreads();
            const int j = j0 + tid;
            if (j < a.X) {
#pragma unroll
                for (int lrow = 0; lrow < kRows; ++lrow) {
                    const int b = b0 + pass * kRows + lrow;
                    if (b < a.B) {
                        const size_t at = (size_t)b * (size_t)a.X + (size_t)j;
                        if (MODE == kRepr)
                            a.phi[at] = make_double2(stage[lrow * kSt + tid], stage[(kRows + lrow) * kSt + tid]);
                        else
                            a.p[at] = stage[lrow * kSt + tid];
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_spatial_repr(Args a) { body<kRepr>(a); }
__global__ __launch_bounds__(kThreads) void k_spatial_probability(Args a) { body<kProb>(a); }
__global__ __launch_bounds__(kThreads) void k_spatial_mean(Args a) { body<kMean>(a); }

// grid mode: the state is its own representation
__global__ __launch_bounds__(kThreads) void k_spatial_grid_probability(const double2* psi, size_t n, double* p) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) {
        const double2 c = psi[i];
        p[i] = density(c.x, c.y);
    }
}

// grid mode, the mean's first stage in the Fock kernel's order: one thread per (group, point)
__global__ __launch_bounds__(kThreads) void k_spatial_grid_mean(const double2* psi, int B, int X, const uint8_t* mask,
                                                                double* partial) {
#pragma clang fp contract(off)
    const int j = (int)blockIdx.y * kThreads + (int)threadIdx.x, b0 = (int)blockIdx.x * kTB;
    if (j >= X) return;
    double s[4];
    for (int q = 0; q < 4; ++q) {
        s[q] = 0.;
        for (int i = 0; i < kTB / 4; ++i) {
            const int b = b0 + q + 4 * i;
            double v = 0.;
            if (b < B && (mask == nullptr || mask[b] != 0)) {
                const double2 c = psi[(size_t)b * (size_t)X + (size_t)j];
                v = density(c.x, c.y);
            }
            s[q] = s[q] + v;
        }
    }
    partial[(size_t)blockIdx.x * (size_t)X + (size_t)j] = join4(s[0], s[1], s[2], s[3]);
}

// the second stage, one workgroup of 4 x 256 threads: count = the envs whose mask is set (all B without a mask);
// thread (s, j) keeps r[s] = the running sum, from +0, of the partials of the groups s, s + 4, s + 8, ..; out[j] =
// ((r[0] + r[1]) + (r[2] + r[3])) / count: the first stage's rule one level up. count == 0: zeros, no division
constexpr int kFinish = 4 * kThreads;
__global__ __launch_bounds__(kFinish) void k_spatial_finish(const double* partial, int groups, int X,
                                                            const uint8_t* mask, int B, double* out, int64_t* count) {
#pragma clang fp contract(off)
    __shared__ long long cnt[kFinish];
    __shared__ double r[4][kThreads];
    const int tid = (int)threadIdx.x, s = tid / kThreads, jj = tid % kThreads;
    long long c = 0;
    if (mask != nullptr)
        for (int b = tid; b < B; b += kFinish) c += mask[b] != 0 ? 1 : 0;
    cnt[tid] = c;
    __syncthreads();
    for (int w = kFinish / 2; w > 0; w >>= 1) {
        if (tid < w) cnt[tid] += cnt[tid + w];
        __syncthreads();
    }
    const long long n = mask != nullptr ? cnt[0] : (long long)B;
    if (tid == 0 && count != nullptr) *count = (int64_t)n;
    for (int jb = 0; jb < X; jb += kThreads) {       // (every thread runs every block: the barriers are uniform)
        const int j = jb + jj;
        double sum = 0.;
        if (j < X) {
#pragma unroll 8
            for (int g = s; g < groups; g += 4) sum = sum + partial[(size_t)g * (size_t)X + (size_t)j];
        }
        r[s][jj] = sum;
        __syncthreads();
        if (s == 0 && j < X) {
            const double m = join4(r[0][jj], r[1][jj], r[2][jj], r[3][jj]);
            out[j] = n > 0 ? m / (double)n : 0.;
        }
        __syncthreads();
    }
}

}  // namespace spatial
}  // namespace qcart

using namespace qcart::spatial;

struct qc_spatial {
    int32_t n_levels = 0;       // 0: grid mode
    int32_t x_n = 0;
    int32_t ldE = 0;            // the device table's row stride: n_levels rounded up to whole chunks
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    double* d_E = nullptr;      // [round_up(x_n, 256)][ldE], zero outside [x_n][n_levels]
    double* d_partial = nullptr;
    size_t partial_cap = 0;     // doubles
    // qc_spatial_congruence (the kernels are qcart_phase.hip's)
    int32_t ldX = 0;            // x_n rounded up to whole blocks of 256 points
    double* d_Et = nullptr;     // the transposed table [ldE][ldX], d_Et[n][j] = E[j][n], zero outside [n_levels][x_n],
                                // and one complex zero behind it: the operand of what does not enter
    void* d_Z = nullptr;        // [z_cap][n_levels][x_n] complex128, of the largest M seen
    size_t z_cap = 0;
};

namespace {

using qcart::host::Dev;
qcart::host::CreateError g_spatial_err;

int sfail(qc_spatial* s, int code, const std::string& msg) {
    s->err = msg;
    return code;
}

// the checks every transform shares; QC_OK or the refusal
int check_call(qc_spatial* s, const char* who, const void* psi, int32_t B, int32_t n_state, double threshold,
               const void* out) {
    const std::string w = std::string(who) + ": ";
    if (!psi || !out) return sfail(s, QC_EINVAL, w + "psi and out are required");
    if (B < 1) return sfail(s, QC_EINVAL, w + "B must be >= 1");
    if (!(threshold >= 0.)) return sfail(s, QC_EINVAL, w + "threshold must be >= 0");
    if (s->n_levels == 0) {
        if (n_state != s->x_n)
            return sfail(s, QC_EINVAL, w + "a grid view takes states of x_n = " + std::to_string(s->x_n) +
                                           " points, not " + std::to_string(n_state));
    } else if (n_state < 1 || n_state > s->n_levels) {
        return sfail(s, QC_EINVAL, w + "n_state must be in [1, n_levels = " + std::to_string(s->n_levels) + "], not " +
                                       std::to_string(n_state));
    }
    return QC_OK;
}

Args make_args(const qc_spatial* s, const void* psi, int32_t B, int32_t n_state, double threshold) {
    Args a{};
    a.psi = (const double2*)psi;
    a.E = s->d_E;
    a.B = B;
    a.n_state = n_state;
    a.ldE = s->ldE;
    a.X = s->x_n;
    a.threshold = threshold;
    return a;
}

dim3 tiles(int32_t B, int32_t X) { return dim3((unsigned)((B + kTB - 1) / kTB), (unsigned)((X + kTX - 1) / kTX)); }

int launched(qc_spatial* s, const char* who) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? QC_OK : qcart::host::hip_fail(s->err, e, who);
}

}  // namespace

extern "C" {

int qc_spatial_create(int32_t n_levels, const double* x, int32_t x_n, int device, qc_spatial** out) {
    if (!out) return QC_EINVAL;
    *out = nullptr;
    if (n_levels < 0)
        return g_spatial_err.fail("qc_spatial_create: n_levels must be in [1, 2048], or 0 for a grid view", QC_EINVAL);
    // (a grid view has no table: its x is checked as a one-level table's)
    if (const char* bad = bad_table(n_levels == 0 ? 1 : n_levels, x, x_n))
        return g_spatial_err.fail(std::string("qc_spatial_create: ") + bad, QC_EINVAL);
    const int32_t ldE = (n_levels + kKC - 1) / kKC * kKC, rows = (x_n + kTX - 1) / kTX * kTX;
    std::vector<double> padded;
    if (n_levels > 0) {
        std::vector<double> table((size_t)x_n * (size_t)n_levels);
        const char* why = nullptr;
        if (qc_spatial_build_table(n_levels, x, x_n, table.data(), &why) != QC_OK)
            return g_spatial_err.fail(std::string("qc_spatial_create: ") + (why ? why : "table"), QC_EINVAL);
        padded.assign((size_t)rows * (size_t)ldE, 0.);
        for (int32_t j = 0; j < x_n; ++j)
            for (int32_t n = 0; n < n_levels; ++n)
                padded[(size_t)j * (size_t)ldE + (size_t)n] = table[(size_t)j * (size_t)n_levels + (size_t)n];
    }
    if (const int rc = qcart::host::check_device(device, g_spatial_err, "the spatial view")) return rc;
    qc_spatial* s = new qc_spatial();
    s->n_levels = n_levels;
    s->x_n = x_n;
    s->ldE = ldE;
    s->ldX = rows;
    s->device = device;
    Dev g(device);
    if (n_levels > 0) {
        std::vector<double> turned((size_t)ldE * (size_t)rows + 2, 0.);
        for (int32_t j = 0; j < x_n; ++j)
            for (int32_t n = 0; n < n_levels; ++n)
                turned[(size_t)n * (size_t)rows + (size_t)j] = padded[(size_t)j * (size_t)ldE + (size_t)n];
        hipError_t e = hipMalloc((void**)&s->d_E, padded.size() * sizeof(double));
        if (e == hipSuccess) e = hipMemcpy(s->d_E, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc((void**)&s->d_Et, turned.size() * sizeof(double));
        if (e == hipSuccess)
            e = hipMemcpy(s->d_Et, turned.data(), turned.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            const std::string msg = std::string("qc_spatial_create: ") + hipGetErrorString(e);
            qc_spatial_destroy(s);
            return g_spatial_err.fail(msg, QC_EHIP);
        }
    }
    *out = s;
    return QC_OK;
}

void qc_spatial_destroy(qc_spatial* s) {
    if (!s) return;
    {
        Dev g(s->device);
        (void)hipDeviceSynchronize();
        if (s->d_E) (void)hipFree(s->d_E);
        if (s->d_partial) (void)hipFree(s->d_partial);
        if (s->d_Et) (void)hipFree(s->d_Et);
        if (s->d_Z) (void)hipFree(s->d_Z);
    }
    delete s;
}

const char* qc_spatial_last_error(const qc_spatial* s) { return s ? s->err.c_str() : g_spatial_err.text(); }

int qc_spatial_set_stream(qc_spatial* s, void* stream) {
    if (!s) return QC_EINVAL;
    s->stream = (hipStream_t)stream;
    return QC_OK;
}

int qc_spatial_table(const qc_spatial* cs, double* out) {
    qc_spatial* s = const_cast<qc_spatial*>(cs);
    if (!s) return QC_EINVAL;
    if (!out) return sfail(s, QC_EINVAL, "qc_spatial_table: out is required");
    if (s->n_levels == 0) return sfail(s, QC_EINVAL, "qc_spatial_table: a grid view has no table");
    Dev g(s->device);
    // the unpadded [x_n][n_levels] corner of the device table
    const size_t width = (size_t)s->n_levels * sizeof(double);
    const hipError_t e = hipMemcpy2DAsync(out, width, s->d_E, (size_t)s->ldE * sizeof(double), width, (size_t)s->x_n,
                                          hipMemcpyDeviceToDevice, s->stream);
    return e == hipSuccess ? QC_OK : qcart::host::hip_fail(s->err, e, "qc_spatial_table");
}

int qc_spatial_repr(qc_spatial* s, const void* psi, int32_t B, int32_t n_state, double threshold, void* out) {
    if (!s) return QC_EINVAL;
    if (s->n_levels == 0)
        return sfail(s, QC_EINVAL, "qc_spatial_repr: a grid view's state is its own representation");
    if (const int rc = check_call(s, "qc_spatial_repr", psi, B, n_state, threshold, out)) return rc;
    Dev g(s->device);
    Args a = make_args(s, psi, B, n_state, threshold);
    a.phi = (double2*)out;
    hipLaunchKernelGGL(k_spatial_repr, tiles(B, s->x_n), dim3(kThreads), 0, s->stream, a);
    return launched(s, "qc_spatial_repr");
}

int qc_spatial_probability(qc_spatial* s, const void* psi, int32_t B, int32_t n_state, double threshold, double* out) {
    if (!s) return QC_EINVAL;
    if (const int rc = check_call(s, "qc_spatial_probability", psi, B, n_state, threshold, out)) return rc;
    Dev g(s->device);
    if (s->n_levels == 0) {
        const size_t n = (size_t)B * (size_t)s->x_n;
        hipLaunchKernelGGL(k_spatial_grid_probability, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                           s->stream, (const double2*)psi, n, out);
        return launched(s, "qc_spatial_probability");
    }
    Args a = make_args(s, psi, B, n_state, threshold);
    a.p = out;
    hipLaunchKernelGGL(k_spatial_probability, tiles(B, s->x_n), dim3(kThreads), 0, s->stream, a);
    return launched(s, "qc_spatial_probability");
}

int qc_spatial_mean(qc_spatial* s, const void* psi, int32_t B, int32_t n_state, const uint8_t* mask, double threshold,
                    double* out, int64_t* count) {
    if (!s) return QC_EINVAL;
    if (const int rc = check_call(s, "qc_spatial_mean", psi, B, n_state, threshold, out)) return rc;
    Dev g(s->device);
    const int groups = (B + kTB - 1) / kTB;
    const size_t need = (size_t)groups * (size_t)s->x_n;
    if (need > s->partial_cap) {
        // (hipFree waits for the device: no launch still reads the old buffer)
        if (s->d_partial) (void)hipFree(s->d_partial);
        s->d_partial = nullptr;
        s->partial_cap = 0;
        const hipError_t e = hipMalloc((void**)&s->d_partial, need * sizeof(double));
        if (e != hipSuccess) return qcart::host::hip_fail(s->err, e, "qc_spatial_mean");
        s->partial_cap = need;
    }
    if (s->n_levels == 0) {
        hipLaunchKernelGGL(k_spatial_grid_mean, dim3((unsigned)groups, (unsigned)((s->x_n + kThreads - 1) / kThreads)),
                           dim3(kThreads), 0, s->stream, (const double2*)psi, B, s->x_n, mask, s->d_partial);
    } else {
        Args a = make_args(s, psi, B, n_state, threshold);
        a.mask = mask;
        a.partial = s->d_partial;
        hipLaunchKernelGGL(k_spatial_mean, tiles(B, s->x_n), dim3(kThreads), 0, s->stream, a);
    }
    if (const int rc = launched(s, "qc_spatial_mean")) return rc;
    hipLaunchKernelGGL(k_spatial_finish, dim3(1), dim3(kFinish), 0, s->stream, (const double*)s->d_partial, groups,
                       s->x_n, mask, B, out, count);
    return launched(s, "qc_spatial_mean");
}

int qc_spatial_congruence(qc_spatial* s, const void* rho, int32_t n_state, int32_t M, double scale, void* sigma) {
    if (!s) return QC_EINVAL;
    const std::string w = "qc_spatial_congruence: ";
    if (s->n_levels == 0) return sfail(s, QC_EINVAL, w + "a grid view's density matrix lives on the grid already");
    if (!rho || !sigma) return sfail(s, QC_EINVAL, w + "rho and sigma are required");
    if (M < 1) return sfail(s, QC_EINVAL, w + "M must be >= 1");
    if (n_state < 1 || n_state > s->n_levels)
        return sfail(s, QC_EINVAL, w + "n_state must be in [1, n_levels = " + std::to_string(s->n_levels) + "], not " +
                                       std::to_string(n_state));
    if (!std::isfinite(scale)) return sfail(s, QC_EINVAL, w + "scale must be finite");
    if ((int64_t)M * s->x_n * s->x_n > ((int64_t)1 << 27)) return sfail(s, QC_EINVAL, w + "M x_n^2 must be <= 2^27");
    Dev g(s->device);
    if ((size_t)M > s->z_cap) {
        // (hipFree waits for the device: no launch still reads the old buffer)
        if (s->d_Z) (void)hipFree(s->d_Z);
        s->d_Z = nullptr;
        s->z_cap = 0;
        const size_t bytes = (size_t)M * (size_t)s->n_levels * (size_t)s->x_n * 2 * sizeof(double);
        const hipError_t e = hipMalloc(&s->d_Z, bytes);
        if (e != hipSuccess) return qcart::host::hip_fail(s->err, e, "qc_spatial_congruence");
        s->z_cap = (size_t)M;
    }
    const double* zero = s->d_Et + (size_t)s->ldE * (size_t)s->ldX;
    const hipError_t e = qcart::phase::launch_congruence(s->d_Et, s->ldX, zero, s->x_n, n_state, rho, M, scale, s->d_Z,
                                                         sigma, s->stream);
    return e == hipSuccess ? QC_OK : qcart::host::hip_fail(s->err, e, "qc_spatial_congruence");
}

}  // extern "C"
