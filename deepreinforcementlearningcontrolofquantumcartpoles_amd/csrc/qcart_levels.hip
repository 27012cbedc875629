// qcart_levels.hip — the energy-level view of a batch of grid (or Fock) states (qc_levels, include/qcart.h): the
// amplitudes a[b][k] = scale * sum_j V[k][j] psi_b[j] on a real level table V [K][N], their populations
// p[b][k] = fl(fl(Re^2) + fl(Im^2)), and the ensemble mean of the populations in one fused pass.
//
// It is the algebra of qcart_spatial.hip with the roles swapped: the long index N (up to 2048) is contracted, the
// output K is narrow. A dense fp64 contraction [B][N] complex x [N][K] real on v_mfma_f64_16x16x4_f64: A = the states
// (rows = envs), B = the table (columns = levels), two accumulator sets (Re, Im) sharing the table operand. A
// workgroup of four waves owns 64 envs x one block of up to 64 levels (blockIdx.y: K > 64 takes more blocks); wave w
// owns the envs 16 w .. 16 w + 15 as 1 x 4 MFMA tiles, of which only the tiles that start below K are computed. psi
// is read once per level block (once in all for K <= 64); psi and the table chunk go through LDS in chunks of 16
// points, the table chunk shared by the four waves; the next chunk's global loads are issued before the current
// chunk's MFMAs and land in registers behind them. The ragged edges: the device table is padded with zeros to whole
// tiles (64 levels, 16 points), so its loads need no guard and stay inside the allocation; a psi element past B or
// past N, and in the mean a masked env's, is read from the handle's zeros instead (the address is selected: every load
// is unconditional, nothing is multiplied by a mask); stores are guarded per element, offsets are 64-bit. The order
// of an output element's sum is fixed: chunk after chunk, within a chunk one MFMA per four points, from +0, so a[b]
// does not depend on B or on env b's place in a tile. One body, three epilogues: k_levels_amplitudes,
// k_levels_populations, and k_levels_mean, which adds the populations over the workgroup's 64 envs (order:
// include/qcart.h) into the handle's partials and, with a mask, leaves the group's number of live envs next to them;
// k_levels_finish adds the partials in order and the counts, and divides.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/qcart.h"
#include "qcart_host.hpp"
#include "qcart_levels.hpp"
#include "qcart_tables.hpp"

namespace qcart {
namespace levels {

constexpr int kThreads = 256;
constexpr int kTB = 64;          // envs per workgroup: four waves x one MFMA row tile; the group of the mean's stages
constexpr int kTK = 64;          // levels per workgroup: four MFMA column tiles
constexpr int kKC = 16;          // points per LDS chunk
constexpr int kLd = kKC + 1;     // LDS row stride in doubles
using f64x4 = double __attribute__((ext_vector_type(4)));

enum { kAmp = 0, kPop = 1, kMean = 2 };

struct Args {
    const double2* psi;      // [B][N]
    const double* V;         // [round_up(K, 64)][ldV], zero outside [K][N]
    const double2* zero;     // one complex zero (the handle's)
    int B, N, ldV, K;        // ldV = round_up(N, 16)
    double scale;
    double2* amp;            // kAmp: [B][K]
    double* p;               // kPop: [B][K]
    const uint8_t* mask;     // kMean: [B] or NULL
    double* partial;         // kMean: [ceil(B / 64)][K]
    int* live;               // kMean with a mask: [ceil(B / 64)], the group's envs that enter
};

__device__ __forceinline__ double density(double re, double im) {
#pragma clang fp contract(off)
    const double a = re * re, b = im * im;
    return a + b;
}

// the sum of four running sums, at every stage of the mean: (s[0] + s[1]) + (s[2] + s[3])
__device__ __forceinline__ double join4(double s0, double s1, double s2, double s3) {
#pragma clang fp contract(off)
    const double a = s0 + s1, b = s2 + s3;
    return a + b;
}

template <int MODE>
__device__ __forceinline__ void body(const Args& a) {
    __shared__ double sRe[kTB * kLd], sIm[kTB * kLd], sV[kTK * kLd];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = (int)blockIdx.x * kTB, k0 = (int)blockIdx.y * kTK;
    const int lj = tid & 15, lr = tid >> 4;          // the loaders: point within the chunk, row 0 .. 15
    const int row = lane & 15, q = lane >> 4;        // MFMA operands: A[row][k = q], B[k = q][col = row]
    const int left_k = a.K - k0;
    const int ntiles = left_k >= kTK ? kTK / 16 : (left_k + 15) / 16;    // the column tiles that start below K
    const bool rows_on = b0 + 16 * wave < a.B;                           // (wave-uniform)
    f64x4 accRe[kTK / 16], accIm[kTK / 16];
#pragma unroll
    for (int nt = 0; nt < kTK / 16; ++nt) accRe[nt] = accIm[nt] = f64x4{0., 0., 0., 0.};

    // whether this loader's four envs enter: inside B, and in the mean with their mask byte set
    bool take[kTB / 16];
#pragma unroll
    for (int i = 0; i < kTB / 16; ++i) {
        const int b = b0 + lr + 16 * i;
        take[i] = b < a.B;
        if (MODE == kMean && a.mask != nullptr && take[i]) take[i] = a.mask[b] != 0;
    }

    // one chunk in registers: this thread's 4 state elements and 4 table entries of point j0 + lj. What does not
    // enter reads the handle's zeros: the address is selected, the load is unconditional
    double2 c[kTB / 16];
    double v[kTK / 16];
    auto fetch = [&](int j0) {
        const int j = j0 + lj;
#pragma unroll
        for (int i = 0; i < kTB / 16; ++i) {
            const double2* src = take[i] && j < a.N ? a.psi + ((size_t)(b0 + lr + 16 * i) * (size_t)a.N + (size_t)j)
                                                    : a.zero;
            c[i] = *src;
        }
        // (row k0 + lr + 16 i < round_up(K, 64), column j < round_up(N, 16) = ldV: inside the padded table)
        const double* vp = a.V + (size_t)(k0 + lr) * (size_t)a.ldV + (size_t)j;
#pragma unroll
        for (int i = 0; i < kTK / 16; ++i) v[i] = vp[(size_t)(16 * i) * (size_t)a.ldV];
    };

    fetch(0);
    for (int j0 = 0; j0 < a.N; j0 += kKC) {
        __syncthreads();                              // the previous chunk's reads are done
#pragma unroll
        for (int i = 0; i < kTB / 16; ++i) {
            sRe[(lr + 16 * i) * kLd + lj] = c[i].x;
            sIm[(lr + 16 * i) * kLd + lj] = c[i].y;
        }
#pragma unroll
        for (int i = 0; i < kTK / 16; ++i) sV[(lr + 16 * i) * kLd + lj] = v[i];
        __syncthreads();
        if (j0 + kKC < a.N) fetch(j0 + kKC);          // in flight behind this chunk's MFMAs
        if (!rows_on) continue;                       // (this wave's envs all lie past B; it still loads and syncs)
        const int left = a.N - j0, jend = left < kKC ? left : kKC;
        for (int jj = 0; jj < jend; jj += 4) {       // (points jj .. jj + 3 < kKC: zeros past N)
            const double ar = sRe[(wave * 16 + row) * kLd + jj + q];
            const double ai = sIm[(wave * 16 + row) * kLd + jj + q];
#pragma unroll
            for (int nt = 0; nt < kTK / 16; ++nt) {
                if (nt >= ntiles) continue;           // (wave-uniform)
                const double vb = sV[(nt * 16 + row) * kLd + jj + q];
                accRe[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, vb, accRe[nt], 0, 0, 0);
                accIm[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, vb, accIm[nt], 0, 0, 0);
            }
        }
    }

    // D element r of tile nt: env b0 + 16 wave + q + 4 r, level k0 + 16 nt + row
    if constexpr (MODE == kMean) {
        // an env that does not enter fed zeros: its population is +0. s[q] = the running sum over the sub-group's envs
        // q, q + 4, q + 8, q + 12; the sub-group's sum (s[0] + s[1]) + (s[2] + s[3]) by two exchanges every lane takes
        // part in; the four sub-groups' sums through LDS, joined by the same rule
        __shared__ double sPart[kTB / 16][kTK];
        __shared__ int sLive[16];                     // one per loader row: its four envs that enter
        if (lj == 0) sLive[lr] = (int)take[0] + (int)take[1] + (int)take[2] + (int)take[3];
#pragma unroll
        for (int nt = 0; nt < kTK / 16; ++nt) {
            double s = 0.;
            {
#pragma clang fp contract(off)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double re = a.scale * accRe[nt][r], im = a.scale * accIm[nt][r];
                    s = s + density(re, im);
                }
            }
            const double t = s + __shfl_xor(s, 16);
            const double u = t + __shfl_xor(t, 32);
            if (q == 0) sPart[wave][nt * 16 + row] = u;
        }
        __syncthreads();
        if (tid < kTK && k0 + tid < a.K)
            a.partial[(size_t)blockIdx.x * (size_t)a.K + (size_t)(k0 + tid)] =
                join4(sPart[0][tid], sPart[1][tid], sPart[2][tid], sPart[3][tid]);
        if (tid == 0 && blockIdx.y == 0 && a.live != nullptr) {
            int n = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) n += sLive[i];
            a.live[blockIdx.x] = n;
        }
    } else {
        if (!rows_on) return;
#pragma unroll
        for (int nt = 0; nt < kTK / 16; ++nt) {
            if (nt >= ntiles) continue;
            const int k = k0 + nt * 16 + row;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int b = b0 + wave * 16 + q + 4 * r;
                if (b < a.B && k < a.K) {
                    const double re = a.scale * accRe[nt][r], im = a.scale * accIm[nt][r];
                    const size_t at = (size_t)b * (size_t)a.K + (size_t)k;
                    if (MODE == kAmp)
                        a.amp[at] = make_double2(re, im);
                    else
                        a.p[at] = density(re, im);
                }
            }
        }
    }
}

// four waves per SIMD (at most 128 registers): the kernel streams psi, so it is waves in flight that hide the loads
#define QCART_LEVELS_KERNEL __global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4)))
QCART_LEVELS_KERNEL void k_levels_amplitudes(Args a) { body<kAmp>(a); }
QCART_LEVELS_KERNEL void k_levels_populations(Args a) { body<kPop>(a); }
QCART_LEVELS_KERNEL void k_levels_mean(Args a) { body<kMean>(a); }
#undef QCART_LEVELS_KERNEL

// the mean's last stage, one workgroup of 4 x 64 threads per block of 64 levels: count = the envs whose mask is set,
// the sum of the groups' counts the first stage left (all B without a mask; every workgroup adds them up, the first
// writes the result); thread (t, k) keeps r[t] = the running sum,
// from +0, of the partials of the groups t, t + 4, t + 8, ..; out[k] = ((r[0] + r[1]) + (r[2] + r[3])) / count.
// count == 0: zeros, no division
__global__ __launch_bounds__(kThreads) void k_levels_finish(const double* partial, int groups, int K,
                                                            const int* live, int B, double* out, int64_t* count) {
#pragma clang fp contract(off)
    __shared__ long long cnt[kThreads];
    __shared__ double r[4][kTK];
    const int tid = (int)threadIdx.x, t = tid / kTK, kk = tid % kTK;
    long long c = 0;
    if (live != nullptr)
        for (int g = tid; g < groups; g += kThreads) c += live[g];
    cnt[tid] = c;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (tid < w) cnt[tid] += cnt[tid + w];
        __syncthreads();
    }
    const long long n = live != nullptr ? cnt[0] : (long long)B;
    if (tid == 0 && blockIdx.x == 0 && count != nullptr) *count = (int64_t)n;
    const int k = (int)blockIdx.x * kTK + kk;
    double sum = 0.;
    if (k < K) {
#pragma unroll 8
        for (int g = t; g < groups; g += 4) sum = sum + partial[(size_t)g * (size_t)K + (size_t)k];
    }
    r[t][kk] = sum;
    __syncthreads();
    if (t == 0 && k < K) {
        const double m = join4(r[0][kk], r[1][kk], r[2][kk], r[3][kk]);
        out[k] = n > 0 ? m / (double)n : 0.;
    }
}

}  // namespace levels
}  // namespace qcart

using namespace qcart::levels;

struct qc_levels {
    int32_t N = 0, K = 0;
    int32_t ldV = 0;             // the device table's row stride: N rounded up to whole chunks
    double scale = 0.;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    double* d_V = nullptr;       // [round_up(K, 64)][ldV], zero outside [K][N]
    double2* d_zero = nullptr;   // one complex zero: the operand of what does not enter
    double* d_partial = nullptr; // [ceil(B / 64)][K] doubles, then [ceil(B / 64)] ints, of the largest B seen
    size_t partial_cap = 0;      // groups
};

namespace {

using qcart::host::Dev;
qcart::host::CreateError g_levels_err;

int lfail(qc_levels* h, int code, const std::string& msg) {
    h->err = msg;
    return code;
}

int launched(qc_levels* h, const char* who) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? QC_OK : qcart::host::hip_fail(h->err, e, who);
}

Args make_args(const qc_levels* h, const void* psi, int32_t B) {
    Args a{};
    a.psi = (const double2*)psi;
    a.V = h->d_V;
    a.zero = h->d_zero;
    a.B = B;
    a.N = h->N;
    a.ldV = h->ldV;
    a.K = h->K;
    a.scale = h->scale;
    return a;
}

dim3 tiles(const qc_levels* h, int32_t B) {
    return dim3((unsigned)((B + kTB - 1) / kTB), (unsigned)((h->K + kTK - 1) / kTK));
}

}  // namespace

extern "C" {

int qc_levels_solve(const qc_params* p, int32_t K, double* energies, double* vectors) {
    if (!p || !energies || !vectors)
        return g_levels_err.fail("qc_levels_solve: params, energies and vectors are required", QC_EINVAL);
    if (const char* bad = bad_family(p->family))
        return g_levels_err.fail(std::string("qc_levels_solve: ") + bad, QC_EINVAL);
    qcart::OpHost op;
    std::string err;
    if (const int rc = qcart::build_ops(p->family, p->n_max, p->omega, p->x_max, p->grid_size, p->lambda_, p->mass,
                                        1 << 12, op, err))
        return g_levels_err.fail("qc_levels_solve: " + err, rc);
    if (const char* bad = bad_k(op.N, K)) return g_levels_err.fail(std::string("qc_levels_solve: ") + bad, QC_EINVAL);
    const char* why = nullptr;
    if (const int rc = solve(op.hband.data(), op.N, op.kl, K, energies, vectors, &why))
        return g_levels_err.fail(std::string("qc_levels_solve: ") + (why ? why : "failed"), rc);
    return QC_OK;
}

int qc_levels_create(int32_t N, int32_t K, double scale, const double* vectors, int device, qc_levels** out) {
    if (!out) return g_levels_err.fail("qc_levels_create: out is required", QC_EINVAL);
    *out = nullptr;
    if (const char* bad = bad_create(N, K, scale, vectors))
        return g_levels_err.fail(std::string("qc_levels_create: ") + bad, QC_EINVAL);
    if (const int rc = qcart::host::check_device(device, g_levels_err, "the level view")) return rc;
    const int32_t ldV = padded_cols(N), rows = padded_rows(K);
    std::vector<double> padded((size_t)rows * (size_t)ldV, 0.);
    for (int32_t k = 0; k < K; ++k)
        for (int32_t j = 0; j < N; ++j)
            padded[(size_t)k * (size_t)ldV + (size_t)j] = vectors[(size_t)k * (size_t)N + (size_t)j];
    qc_levels* h = new qc_levels();
    h->N = N;
    h->K = K;
    h->ldV = ldV;
    h->scale = scale;
    h->device = device;
    Dev g(device);
    hipError_t e = hipMalloc((void**)&h->d_V, padded.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(h->d_V, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_zero, sizeof(double2));
    if (e == hipSuccess) e = hipMemset(h->d_zero, 0, sizeof(double2));
    if (e != hipSuccess) {
        const std::string msg = std::string("qc_levels_create: ") + hipGetErrorString(e);
        qc_levels_destroy(h);
        return g_levels_err.fail(msg, QC_EHIP);
    }
    *out = h;
    return QC_OK;
}

void qc_levels_destroy(qc_levels* h) {
    if (!h) return;
    {
        Dev g(h->device);
        (void)hipDeviceSynchronize();
        if (h->d_V) (void)hipFree(h->d_V);
        if (h->d_zero) (void)hipFree(h->d_zero);
        if (h->d_partial) (void)hipFree(h->d_partial);
    }
    delete h;
}

const char* qc_levels_last_error(const qc_levels* h) { return h ? h->err.c_str() : g_levels_err.text(); }

int qc_levels_set_stream(qc_levels* h, void* stream) {
    if (!h) return QC_EINVAL;
    h->stream = (hipStream_t)stream;
    return QC_OK;
}

int qc_levels_amplitudes(qc_levels* h, const void* psi, int32_t B, void* out) {
    if (!h) return QC_EINVAL;
    if (const char* bad = bad_call(psi, B, out)) return lfail(h, QC_EINVAL, std::string("qc_levels_amplitudes: ") + bad);
    Dev g(h->device);
    Args a = make_args(h, psi, B);
    a.amp = (double2*)out;
    hipLaunchKernelGGL(k_levels_amplitudes, tiles(h, B), dim3(kThreads), 0, h->stream, a);
    return launched(h, "qc_levels_amplitudes");
}

int qc_levels_populations(qc_levels* h, const void* psi, int32_t B, double* out) {
    if (!h) return QC_EINVAL;
    if (const char* bad = bad_call(psi, B, out))
        return lfail(h, QC_EINVAL, std::string("qc_levels_populations: ") + bad);
    Dev g(h->device);
    Args a = make_args(h, psi, B);
    a.p = out;
    hipLaunchKernelGGL(k_levels_populations, tiles(h, B), dim3(kThreads), 0, h->stream, a);
    return launched(h, "qc_levels_populations");
}

int qc_levels_mean(qc_levels* h, const void* psi, int32_t B, const uint8_t* mask, double* out, int64_t* count) {
    if (!h) return QC_EINVAL;
    if (const char* bad = bad_call(psi, B, out)) return lfail(h, QC_EINVAL, std::string("qc_levels_mean: ") + bad);
    Dev g(h->device);
    const int groups = (B + kTB - 1) / kTB;
    if ((size_t)groups > h->partial_cap) {
        // (hipFree waits for the device: no launch still reads the old buffer)
        if (h->d_partial) (void)hipFree(h->d_partial);
        h->d_partial = nullptr;
        h->partial_cap = 0;
        const hipError_t e =
            hipMalloc((void**)&h->d_partial, (size_t)groups * ((size_t)h->K * sizeof(double) + sizeof(int)));
        if (e != hipSuccess) return qcart::host::hip_fail(h->err, e, "qc_levels_mean");
        h->partial_cap = (size_t)groups;
    }
    Args a = make_args(h, psi, B);
    a.mask = mask;
    a.partial = h->d_partial;
    a.live = mask ? (int*)(h->d_partial + (size_t)groups * (size_t)h->K) : nullptr;
    hipLaunchKernelGGL(k_levels_mean, tiles(h, B), dim3(kThreads), 0, h->stream, a);
    if (const int rc = launched(h, "qc_levels_mean")) return rc;
    hipLaunchKernelGGL(k_levels_finish, dim3((unsigned)((h->K + kTK - 1) / kTK)), dim3(kThreads), 0, h->stream,
                       (const double*)h->d_partial, groups, (int)h->K, (const int*)a.live, B, out, count);
    return launched(h, "qc_levels_mean");
}

}  // extern "C"
