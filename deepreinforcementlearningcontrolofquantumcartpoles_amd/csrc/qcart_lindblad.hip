// qcart_lindblad.hip — the master equation of continuous position measurement on density matrices (qc_lindblad,
// include/qcart.h). The hot path is the batched Hermitian congruence Y_m = g o (A_s(m) X_m A_s(m)^†) in two kernels on
// v_mfma_f64_16x16x4_f64:
//     k_lindblad_left:   Zt[j][i] = sum_k X[k][j] At[k][i]               (Zt = (A X)^T, all of it)
//     k_lindblad_right:  Y[i][j]  = g[i][j] * sum_k Zt[k][i] conj(At[k][j])   (j <= i, mirrored)
// with At[k][i] = A[i][k] the transposed operand the handle keeps (the tables are uploaded transposed at create time;
// k_lindblad_widen transposes qc_lindblad_congruence's A and widens the real W). Both kernels then contract over the
// leading index of two row-major operands: lane (row, q) of a wave reads element k0 + q of 16 consecutive columns, so
// the 16 lanes of one q read 256 contiguous bytes of either operand. The operands come straight from global memory /
// L2 (a workgroup is one wave, so there is nothing LDS could share), one group of four k ahead of the MFMAs.
//
// A workgroup is one wave and owns a block of 32 x 32 complex elements (2 x 2 tiles x {re, im}: 8 accumulator tiles,
// 64 registers) of one matrix of the batch; the right kernel launches only the blocks on or below the diagonal (block
// t = I (I + 1) / 2 + J, J <= I) and skips the tile strictly above it inside a diagonal block. A launch of fewer than
// kWideFrom such blocks (the drivers' 71 .. 181 at M = 21) would leave most SIMDs without a wave while the others
// run long MFMA chains: it goes to k_lindblad_left16 / k_lindblad_right16, the same body with one tile per workgroup
// and four times the waves. An element's sums are the same instructions in the same order in both. A complex product is
// four real MFMA chains into two accumulators, in the order include/qcart.h documents; rows, columns and k past N feed
// exact zeros selected by address. Stores are guarded per element, with 64-bit offsets. A slot outside [0, J) makes
// every workgroup of that matrix return before it reads or writes anything; the left kernel raises the error flag.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/qcart.h"
#include "qcart_filter.hpp"
#include "qcart_host.hpp"
#include "qcart_lindblad.hpp"
#include "qcart_tables.hpp"

namespace qcart {
namespace lindblad {

constexpr int kLanes = 64;
constexpr int kWideFrom = 2048;        // 32 x 32 blocks from this many of them per launch on; below: 16 x 16
using f64x4 = double __attribute__((ext_vector_type(4)));

struct Args {
    const double2* p;        // [M][N][N], contracted over its leading index: left X, right Zt
    double2* out;            // [M][N][N]: left Zt, right Y
    const double2* at;       // the transposed operands: at[s * at_stride + k * N + c] = A_s[c][k]
    size_t at_stride;        // N^2, or 0 where one operand serves every slot
    const double* g;         // [N][N] or null (right only)
    const int32_t* slots;    // [M] or null
    int32_t default_slot, J;
    const double2* zero;     // one complex zero (the handle's)
    int32_t* flag;
    int N, rb, nb;           // rb = ceil(N / block); nb = the blocks of one matrix
};

template <int T>
struct Operands {
    double2 p[T], q[T];
};

// T x T tiles per workgroup: a block of 16 T rows and columns
template <bool RIGHT, int T>
__device__ __forceinline__ void product(const Args& a) {
    constexpr int kBlock = 16 * T;
    const int lane = (int)threadIdx.x, row = lane & 15, q = lane >> 4;
    const int N = a.N;
    const unsigned m = blockIdx.x / (unsigned)a.nb, t = blockIdx.x % (unsigned)a.nb;
    const int slot = a.slots ? a.slots[m] : a.default_slot;
    if (slot < 0 || slot >= a.J) {
        if (!RIGHT && t == 0 && lane == 0) *a.flag = 1;
        return;
    }
    int I, Jb;
    if (RIGHT) {
        I = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
        while (I * (I + 1) / 2 > (int)t) --I;
        while ((I + 1) * (I + 2) / 2 <= (int)t) ++I;
        Jb = (int)t - I * (I + 1) / 2;
    } else {
        I = (int)t / a.rb;
        Jb = (int)t % a.rb;
    }
    const int r0 = kBlock * I, c0 = kBlock * Jb;
    const size_t plane = (size_t)N * (size_t)N;
    const double2* P = a.p + (size_t)m * plane;
    const double2* Q = a.at + (size_t)slot * a.at_stride;

    int ri[T], ci[T];
    bool rok[T], cok[T], on[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i) {
        ri[i] = r0 + 16 * i + row;
        rok[i] = ri[i] < N;
        ci[i] = c0 + 16 * i + row;
        cok[i] = ci[i] < N;
    }
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
            on[i][j] = r0 + 16 * i < N && c0 + 16 * j < N && !(RIGHT && I == Jb && j > i);

    f64x4 re[T][T], im[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) re[i][j] = im[i][j] = f64x4{0., 0., 0., 0.};

    // The operands of the group at k0: a lane whose k, row or column lies past N reads the handle's zero instead (the
    // address is selected, so every load is unconditional and nothing is multiplied by 0).
    auto fetch = [&](int k0, Operands<T>& o) {
        const int k = k0 + q;
        const bool kok = k < N;
        const size_t base = kok ? (size_t)k * (size_t)N : 0;
#pragma unroll
        for (int i = 0; i < T; ++i) {
            o.p[i] = *(kok && rok[i] ? P + base + ri[i] : a.zero);
            o.q[i] = *(kok && cok[i] ? Q + base + ci[i] : a.zero);
        }
    };

    Operands<T> cur, nxt;
    fetch(0, cur);
    for (int k0 = 0; k0 < N; k0 += 4) {
        fetch(k0 + 4, nxt);                          // (past the end: zeros, not used)
        // chain by chain over the tiles, so that consecutive MFMAs do not wait on one accumulator; an accumulator
        // still takes its chains in the documented order
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    if (!on[i][j]) continue;                             // (wave-uniform)
                    const double pr = cur.p[i].x, pi = cur.p[i].y, qr = cur.q[j].x, qi = cur.q[j].y;
                    if (c == 0) re[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(pr, qr, re[i][j], 0, 0, 0);
                    if (c == 1) re[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(RIGHT ? pi : -pi, qi, re[i][j], 0, 0, 0);
                    if (c == 2) im[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(RIGHT ? pi : pr, RIGHT ? qr : qi, im[i][j], 0, 0, 0);
                    if (c == 3) im[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(RIGHT ? -pr : pi, RIGHT ? qi : qr, im[i][j], 0, 0, 0);
                }
        cur = nxt;
    }

    // D element e of tile (i, j): row r0 + 16 i + q + 4 e, column c0 + 16 j + row
    double2* out = a.out + (size_t)m * plane;
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) {
            if (!on[i][j]) continue;
            const int c = c0 + 16 * j + row;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = r0 + 16 * i + q + 4 * e;
                if (r >= N || c >= N) continue;
                const size_t at = (size_t)r * (size_t)N + (size_t)c;
                double vr = re[i][j][e], vi = im[i][j][e];
                if (!RIGHT) {
                    out[at] = make_double2(vr, vi);
                    continue;
                }
                if (c > r) continue;                                     // (a diagonal tile's upper half)
                if (a.g != nullptr) {
                    const double gv = a.g[at];
                    vr = gv * vr;
                    vi = gv * vi;
                }
                if (c == r) {
                    out[at] = make_double2(vr, 0.);
                } else {
                    out[at] = make_double2(vr, vi);
                    out[(size_t)c * (size_t)N + (size_t)r] = make_double2(vr, -vi);
                }
            }
        }
}

__global__ __launch_bounds__(kLanes) void k_lindblad_left(Args a) { product<false, 2>(a); }
__global__ __launch_bounds__(kLanes) void k_lindblad_right(Args a) { product<true, 2>(a); }
// one tile per workgroup: four times the waves, for launches that would leave most of the device idle
__global__ __launch_bounds__(kLanes) void k_lindblad_left16(Args a) { product<false, 1>(a); }
__global__ __launch_bounds__(kLanes) void k_lindblad_right16(Args a) { product<true, 1>(a); }

// rho_m <- g o rho_m for every matrix whose slot is inside [0, J)
constexpr int kThreads = 256;
__global__ __launch_bounds__(kThreads) void k_lindblad_scale(double2* rho, const double* g, const int32_t* slots,
                                                             int32_t default_slot, int32_t J, int N, int M) {
    const size_t plane = (size_t)N * (size_t)N;
    const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= plane * (size_t)M) return;
    const size_t m = e / plane;
    const int slot = slots ? slots[m] : default_slot;
    if (slot < 0 || slot >= J) return;
    const double gv = g[e - m * plane];
    const double2 v = rho[e];
    rho[e] = make_double2(gv * v.x, gv * v.y);
}

// out [N][N] complex = src (real [N][N] or complex [N][N]), transposed or not
__global__ __launch_bounds__(kThreads) void k_lindblad_widen(const void* src, int is_complex, int transpose, int N,
                                                             double2* out) {
    const size_t plane = (size_t)N * (size_t)N;
    const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= plane) return;
    const size_t i = e / (size_t)N, j = e % (size_t)N;
    const size_t s = transpose ? j * (size_t)N + i : e;
    out[e] = is_complex ? ((const double2*)src)[s] : make_double2(((const double*)src)[s], 0.);
}

}  // namespace lindblad
}  // namespace qcart

using namespace qcart::lindblad;

struct qc_lindblad {
    int32_t N = 0, J = 0;
    bool fock = false;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    double2* d_T = nullptr;      // [J][N][N], transposed: d_T[s][k][i] = T_s[i][k]
    double* d_gh = nullptr;      // G½ [N][N]
    double* d_gf = nullptr;      // G [N][N]
    double2* d_W = nullptr;      // Fock: W as a complex operand (the transposed operand of A = W^T)
    double2* d_Wt = nullptr;     // Fock: W^T (the transposed operand of A = W)
    double2* d_A = nullptr;      // qc_lindblad_congruence's transposed operand [N][N]
    double2* d_Z = nullptr;      // [z_cap][N][N], of the largest M seen
    size_t z_cap = 0;
    double2* d_zero = nullptr;   // one complex zero: the operand of what does not enter
    int32_t* d_flag = nullptr;   // [3]: [0] raised by a slot outside [0, J), [1] by a matrix the conditional evolution
                                 // could not step, [2] where its congruences' own slot word goes (never read)
    // the conditional evolution (qc_lindblad_set_efficiency, qc_lindblad_evolve_conditional)
    double dt = 0., gamma = 0., eta = -1.;
    double a = 0., s = 0.;       // eta gamma dt / 2 and 1 / sqrt(4 a)
    std::vector<ld> xi;          // X's eigenvalues in long double
    double* d_xi = nullptr;      // [N]
    double* d_ge = nullptr;      // G^(1 - eta) [N][N] (not read at eta = 1)
    double2* d_backup = nullptr; // [m_cap][N][N]: rho as a call found it
    double* d_v = nullptr;       // [m_cap][N]
    int32_t* d_eff = nullptr;    // [m_cap] the slots the call's congruences read, then [m_cap] status words
    size_t m_cap = 0;
};

namespace {

using qcart::host::Dev;
qcart::host::CreateError g_lindblad_err;

int lfail(qc_lindblad* h, int code, const std::string& msg) {
    h->err = msg;
    return code;
}

int launched(qc_lindblad* h, const char* who) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? QC_OK : qcart::host::hip_fail(h->err, e, who);
}

// p's operators as the tables' source; QC_OK or the refusal with its text in err
int make_source(const qc_params* p, qcart::OpHost& op, Source& s, std::string& err) {
    if (const char* bad = bad_precision(p->precision)) {
        err = bad;
        return QC_EINVAL;
    }
    if (const int rc = qcart::build_ops(p->family, p->n_max, p->omega, p->x_max, p->grid_size, p->lambda_, p->mass,
                                        1 << 12, op, err))
        return rc;
    s.fock = op.fock;
    s.N = op.N;
    s.kl = op.kl;
    s.hband = op.hband.data();
    s.x = op.fock ? op.xu.data() : op.xg.data();
    s.c = op.c;
    if (const char* bad = bad_dim(s.fock, s.N)) {
        err = bad;
        return QC_EINVAL;
    }
    return QC_OK;
}

int grow_z(qc_lindblad* h, int32_t M, const char* who) {
    if ((size_t)M <= h->z_cap) return QC_OK;
    // (hipFree waits for the device: no launch still reads the old buffer)
    if (h->d_Z) (void)hipFree(h->d_Z);
    h->d_Z = nullptr;
    h->z_cap = 0;
    const hipError_t e = hipMalloc((void**)&h->d_Z, (size_t)M * (size_t)h->N * (size_t)h->N * sizeof(double2));
    if (e != hipSuccess) return qcart::host::hip_fail(h->err, e, who);
    h->z_cap = (size_t)M;
    return QC_OK;
}

// the conditional evolution's per-matrix buffers, of the largest M seen
int grow_m(qc_lindblad* h, int32_t M, const char* who) {
    if ((size_t)M <= h->m_cap) return QC_OK;
    void* old[] = {h->d_backup, h->d_v, h->d_eff};
    for (void* p : old)
        if (p) (void)hipFree(p);                       // (waits for the device)
    h->d_backup = nullptr;
    h->d_v = nullptr;
    h->d_eff = nullptr;
    h->m_cap = 0;
    const size_t N = (size_t)h->N;
    hipError_t e = hipMalloc((void**)&h->d_backup, (size_t)M * N * N * sizeof(double2));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_v, (size_t)M * N * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_eff, (size_t)M * 2 * sizeof(int32_t));
    if (e != hipSuccess) return qcart::host::hip_fail(h->err, e, who);
    h->m_cap = (size_t)M;
    return QC_OK;
}

// y = g o (A x A^†) for the transposed operands at (stride 0: one for every slot); flag: the word a slot outside
// [0, J) raises (null: the handle's)
int congruence(qc_lindblad* h, const double2* at, size_t at_stride, const double* g, const double2* x, double2* y,
               int32_t M, const int32_t* slots, int32_t default_slot, int32_t J, const char* who,
               int32_t* flag = nullptr) {
    Args a{};
    a.at = at;
    a.at_stride = at_stride;
    a.slots = slots;
    a.default_slot = default_slot;
    a.J = J;
    a.zero = h->d_zero;
    a.flag = flag ? flag : h->d_flag;
    a.N = h->N;
    // the block shape changes which workgroup computes an element, never the element: its sums run in the same order
    const int rb32 = (h->N + 31) / 32;
    const bool wide = (int64_t)rb32 * rb32 * M >= kWideFrom;
    a.rb = wide ? rb32 : (h->N + 15) / 16;
    a.p = x;
    a.out = h->d_Z;
    a.nb = a.rb * a.rb;
    hipLaunchKernelGGL(wide ? k_lindblad_left : k_lindblad_left16, dim3((unsigned)a.nb * (unsigned)M), dim3(kLanes), 0,
                       h->stream, a);
    if (const int rc = launched(h, who)) return rc;
    a.p = h->d_Z;
    a.out = y;
    a.g = g;
    a.nb = a.rb * (a.rb + 1) / 2;
    hipLaunchKernelGGL(wide ? k_lindblad_right : k_lindblad_right16, dim3((unsigned)a.nb * (unsigned)M), dim3(kLanes),
                       0, h->stream, a);
    return launched(h, who);
}

}  // namespace

extern "C" {

int qc_lindblad_tables(const qc_params* p, double dt, double gamma, double force, double* xi, double* W, void* T,
                       double* g_half, double* g_full) {
    if (!p) return g_lindblad_err.fail("qc_lindblad_tables: params are required", QC_EINVAL);
    const char* bad = bad_step(dt, gamma);
    if (!bad) bad = bad_force(force);
    if (bad) return g_lindblad_err.fail(std::string("qc_lindblad_tables: ") + bad, QC_EINVAL);
    qcart::OpHost op;
    Source s;
    std::string err;
    if (const int rc = make_source(p, op, s, err)) return g_lindblad_err.fail("qc_lindblad_tables: " + err, rc);
    const char* why = nullptr;
    if (const int rc = tables(s, dt, gamma, force, xi, W, (double*)T, g_half, g_full, &why))
        return g_lindblad_err.fail(std::string("qc_lindblad_tables: ") + (why ? why : "failed"), rc);
    return QC_OK;
}

int qc_lindblad_create(const qc_params* p, double dt, double gamma, const double* forces, int32_t J, int device,
                       qc_lindblad** out) {
    if (!out) return g_lindblad_err.fail("qc_lindblad_create: out is required", QC_EINVAL);
    *out = nullptr;
    if (!p || !forces) return g_lindblad_err.fail("qc_lindblad_create: params and forces are required", QC_EINVAL);
    if (const char* bad = bad_step(dt, gamma))
        return g_lindblad_err.fail(std::string("qc_lindblad_create: ") + bad, QC_EINVAL);
    if (J < 1 || J > kMaxJ) return g_lindblad_err.fail(std::string("qc_lindblad_create: ") + bad_slots(J, 1), QC_EINVAL);
    for (int32_t s = 0; s < J; ++s)
        if (const char* bad = bad_force(forces[s]))
            return g_lindblad_err.fail(std::string("qc_lindblad_create: ") + bad, QC_EINVAL);
    qcart::OpHost op;
    Source src;
    std::string err;
    if (const int rc = make_source(p, op, src, err)) return g_lindblad_err.fail("qc_lindblad_create: " + err, rc);
    const int32_t N = src.N;
    if (const char* bad = bad_slots(J, N))
        return g_lindblad_err.fail(std::string("qc_lindblad_create: ") + bad, QC_EINVAL);
    if (const int rc = qcart::host::check_device(device, g_lindblad_err, "the master equation")) return rc;

    // the tables: xi, W, G½, G once, T per force (uploaded transposed)
    const size_t plane = (size_t)N * (size_t)N;
    std::vector<double> W(plane), gh(plane), gf(plane), T(2 * plane), Tt((size_t)J * 2 * plane);
    const char* why = nullptr;
    Basis basis_;                                      // (X's eigenpairs: once for all forces)
    if (const int rc = make_basis(src, basis_, &why))
        return g_lindblad_err.fail(std::string("qc_lindblad_create: ") + (why ? why : "failed"), rc);
    for (int32_t s = 0; s < J; ++s) {
        const bool first = s == 0;
        if (const int rc = tables_on(src, basis_, dt, gamma, forces[s], nullptr, first ? W.data() : nullptr, T.data(),
                                     first ? gh.data() : nullptr, first ? gf.data() : nullptr, &why))
            return g_lindblad_err.fail(std::string("qc_lindblad_create: ") + (why ? why : "failed"), rc);
        double* tt = Tt.data() + (size_t)s * 2 * plane;
        for (int32_t i = 0; i < N; ++i)
            for (int32_t k = 0; k < N; ++k) {
                tt[2 * ((size_t)k * N + i)] = T[2 * ((size_t)i * N + k)];
                tt[2 * ((size_t)k * N + i) + 1] = T[2 * ((size_t)i * N + k) + 1];
            }
    }

    qc_lindblad* h = new qc_lindblad();
    h->N = N;
    h->J = J;
    h->fock = src.fock;
    h->device = device;
    h->dt = dt;
    h->gamma = gamma;
    h->xi = basis_.xi;
    std::vector<double> xi64((size_t)N);
    for (int32_t i = 0; i < N; ++i) xi64[(size_t)i] = (double)basis_.xi[(size_t)i];
    Dev g(device);
    const size_t cbytes = plane * sizeof(double2), rbytes = plane * sizeof(double);
    hipError_t e = hipMalloc((void**)&h->d_T, (size_t)J * cbytes);
    if (e == hipSuccess) e = hipMemcpy(h->d_T, Tt.data(), (size_t)J * cbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_gh, rbytes);
    if (e == hipSuccess) e = hipMemcpy(h->d_gh, gh.data(), rbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_gf, rbytes);
    if (e == hipSuccess) e = hipMemcpy(h->d_gf, gf.data(), rbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_A, cbytes);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_zero, sizeof(double2));
    if (e == hipSuccess) e = hipMemset(h->d_zero, 0, sizeof(double2));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_flag, 3 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(h->d_flag, 0, 3 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_xi, (size_t)N * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(h->d_xi, xi64.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && h->fock) {
        // the real W, staged in d_A's memory, widened to the two complex operands of the basis changes
        e = hipMalloc((void**)&h->d_W, cbytes);
        if (e == hipSuccess) e = hipMalloc((void**)&h->d_Wt, cbytes);
        if (e == hipSuccess) e = hipMemcpy(h->d_A, W.data(), rbytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            const dim3 grid((unsigned)((plane + kThreads - 1) / kThreads));
            hipLaunchKernelGGL(k_lindblad_widen, grid, dim3(kThreads), 0, nullptr, (const void*)h->d_A, 0, 0, (int)N,
                               h->d_W);
            hipLaunchKernelGGL(k_lindblad_widen, grid, dim3(kThreads), 0, nullptr, (const void*)h->d_A, 0, 1, (int)N,
                               h->d_Wt);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipDeviceSynchronize();
        }
    }
    if (e != hipSuccess) {
        const std::string msg = std::string("qc_lindblad_create: ") + hipGetErrorString(e);
        qc_lindblad_destroy(h);
        return g_lindblad_err.fail(msg, QC_EHIP);
    }
    *out = h;
    return QC_OK;
}

void qc_lindblad_destroy(qc_lindblad* h) {
    if (!h) return;
    {
        Dev g(h->device);
        (void)hipDeviceSynchronize();
        void* all[] = {h->d_T,    h->d_gh,   h->d_gf, h->d_W,  h->d_Wt,     h->d_A, h->d_Z,
                       h->d_zero, h->d_flag, h->d_xi, h->d_ge, h->d_backup, h->d_v, h->d_eff};
        for (void* p : all)
            if (p) (void)hipFree(p);
    }
    delete h;
}

const char* qc_lindblad_last_error(const qc_lindblad* h) { return h ? h->err.c_str() : g_lindblad_err.text(); }

int qc_lindblad_set_stream(qc_lindblad* h, void* stream) {
    if (!h) return QC_EINVAL;
    h->stream = (hipStream_t)stream;
    return QC_OK;
}

int qc_lindblad_dim(const qc_lindblad* h) { return h ? h->N : QC_EINVAL; }

int qc_lindblad_evolve(qc_lindblad* h, void* rho, int32_t M, const int32_t* slots, int32_t default_slot,
                       int32_t n_steps) {
    if (!h) return QC_EINVAL;
    if (const char* bad = bad_evolve(rho, M, h->N, slots, default_slot, h->J, n_steps))
        return lfail(h, QC_EINVAL, std::string("qc_lindblad_evolve: ") + bad);
    if (n_steps == 0) return QC_OK;
    const char* who = "qc_lindblad_evolve";
    Dev g(h->device);
    if (const int rc = grow_z(h, M, who)) return rc;
    double2* r = (double2*)rho;
    const size_t plane = (size_t)h->N * (size_t)h->N;
    if (h->fock)                                       // sigma = W^T rho W: A = W^T, whose transposed operand is W
        if (const int rc = congruence(h, h->d_W, 0, nullptr, r, r, M, slots, default_slot, h->J, who)) return rc;
    hipLaunchKernelGGL(k_lindblad_scale, dim3((unsigned)((plane * (size_t)M + kThreads - 1) / kThreads)), dim3(kThreads),
                       0, h->stream, r, (const double*)h->d_gh, slots, default_slot, h->J, (int)h->N, (int)M);
    if (const int rc = launched(h, who)) return rc;
    for (int32_t n = 0; n < n_steps; ++n)
        if (const int rc = congruence(h, h->d_T, plane, n + 1 == n_steps ? h->d_gh : h->d_gf, r, r, M, slots,
                                      default_slot, h->J, who))
            return rc;
    if (h->fock)                                       // rho = W sigma W^T
        if (const int rc = congruence(h, h->d_Wt, 0, nullptr, r, r, M, slots, default_slot, h->J, who)) return rc;
    return QC_OK;
}

int qc_lindblad_congruence(qc_lindblad* h, const void* A, const double* g, const void* x, void* y, int32_t M) {
    if (!h) return QC_EINVAL;
    if (const char* bad = bad_congruence(A, x, y, M, h->N))
        return lfail(h, QC_EINVAL, std::string("qc_lindblad_congruence: ") + bad);
    const char* who = "qc_lindblad_congruence";
    Dev gd(h->device);
    if (const int rc = grow_z(h, M, who)) return rc;
    const size_t plane = (size_t)h->N * (size_t)h->N;
    hipLaunchKernelGGL(k_lindblad_widen, dim3((unsigned)((plane + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       h->stream, A, 1, 1, (int)h->N, h->d_A);
    if (const int rc = launched(h, who)) return rc;
    return congruence(h, h->d_A, 0, g, (const double2*)x, (double2*)y, M, nullptr, 0, 1, who);
}

int qc_lindblad_take_errors(qc_lindblad* h) {
    if (!h) return QC_EINVAL;
    Dev g(h->device);
    int32_t flag[2] = {0, 0};
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipMemcpy(flag, h->d_flag, sizeof(flag), hipMemcpyDeviceToHost);
    if (e == hipSuccess && (flag[0] || flag[1])) e = hipMemset(h->d_flag, 0, sizeof(flag));
    if (e != hipSuccess) return qcart::host::hip_fail(h->err, e, "qc_lindblad_take_errors");
    if (!flag[0] && !flag[1]) return QC_OK;
    const char* slot = "a slot out of [0, J) reached qc_lindblad_evolve (that rho was left untouched)";
    const char* dead = "a rho could not be stepped by qc_lindblad_evolve_conditional: its diagonal's sum, the outcome "
                       "or the outcome's weight Z was not finite and > 0 (that rho was left untouched)";
    return lfail(h, QC_EINVAL, flag[0] && flag[1] ? std::string(slot) + "; " + dead : flag[0] ? slot : dead);
}

int qc_lindblad_set_efficiency(qc_lindblad* h, double eta) {
    if (!h) return QC_EINVAL;
    if (const char* bad = qcart::filter::bad_efficiency(eta, h->gamma))
        return lfail(h, QC_EINVAL, std::string("qc_lindblad_set_efficiency: ") + bad);
    const char* who = "qc_lindblad_set_efficiency";
    const size_t plane = (size_t)h->N * (size_t)h->N;
    Dev g(h->device);
    if (eta < 1.) {
        // G^(1 - eta): the dephasing the record does not account for, gamma (1 - eta) formed in long double
        std::vector<double> ge(plane);
        qcart::filter::efficiency_table(h->N, h->xi.data(), h->dt, h->gamma, eta, ge.data());
        hipError_t e = hipStreamSynchronize(h->stream);                  // (no launch still reads the old table)
        if (e == hipSuccess && !h->d_ge) e = hipMalloc((void**)&h->d_ge, plane * sizeof(double));
        if (e == hipSuccess) e = hipMemcpy(h->d_ge, ge.data(), plane * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) return qcart::host::hip_fail(h->err, e, who);
    }
    h->eta = eta;
    qcart::filter::constants(eta, h->gamma, h->dt, &h->a, &h->s);
    return QC_OK;
}

int qc_lindblad_efficiency(const qc_lindblad* h, double* eta) {
    if (!h || !eta) return QC_EINVAL;
    *eta = h->eta;
    return QC_OK;
}

int qc_lindblad_xi(qc_lindblad* h, double* xi) {
    if (!h) return QC_EINVAL;
    if (!xi) return lfail(h, QC_EINVAL, "qc_lindblad_xi: xi is required");
    Dev g(h->device);
    const hipError_t e = hipMemcpyAsync(xi, h->d_xi, (size_t)h->N * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
    return e == hipSuccess ? QC_OK : qcart::host::hip_fail(h->err, e, "qc_lindblad_xi");
}

int qc_lindblad_efficiency_table(const qc_params* p, double dt, double gamma, double eta, double* g) {
    const char* who = "qc_lindblad_efficiency_table: ";
    if (!p || !g) return g_lindblad_err.fail(std::string(who) + "params and g are required", QC_EINVAL);
    const char* bad = bad_step(dt, gamma);
    if (!bad) bad = qcart::filter::bad_efficiency(eta, gamma);
    if (bad) return g_lindblad_err.fail(std::string(who) + bad, QC_EINVAL);
    qcart::OpHost op;
    Source s;
    std::string err;
    if (const int rc = make_source(p, op, s, err)) return g_lindblad_err.fail(who + err, rc);
    Basis b;
    const char* why = nullptr;
    if (const int rc = make_basis(s, b, &why)) return g_lindblad_err.fail(std::string(who) + (why ? why : "failed"), rc);
    qcart::filter::efficiency_table(s.N, b.xi.data(), dt, gamma, eta, g);
    return QC_OK;
}

int qc_lindblad_filter_draws(uint64_t seed, uint32_t stream, uint64_t step, double* u, double* z) {
    if (!u || !z) return QC_EINVAL;
    qcart::filter::draws(seed, stream, step, u, z);
    return QC_OK;
}

int qc_lindblad_evolve_conditional(qc_lindblad* h, void* rho, int32_t M, const int32_t* slots, int32_t default_slot,
                                   int32_t n_steps, uint64_t seed, const int32_t* streams, int64_t first_step,
                                   const double* draws, const double* record_in, double* record_out) {
    if (!h) return QC_EINVAL;
    if (const char* bad = qcart::filter::bad_conditional(rho, M, h->N, slots, default_slot, h->J, n_steps, h->eta,
                                                         first_step, draws, record_in))
        return lfail(h, QC_EINVAL, std::string("qc_lindblad_evolve_conditional: ") + bad);
    if (n_steps == 0) return QC_OK;
    const char* who = "qc_lindblad_evolve_conditional";
    Dev g(h->device);
    if (const int rc = grow_z(h, M, who)) return rc;
    if (const int rc = grow_m(h, M, who)) return rc;
    double2* r = (double2*)rho;
    const size_t plane = (size_t)h->N * (size_t)h->N;
    qcart::filter::Call c{};
    c.sigma = rho;
    c.xi = h->d_xi;
    c.N = h->N;
    c.M = M;
    c.J = h->J;
    c.slots = slots;
    c.default_slot = default_slot;
    c.eff = h->d_eff;
    c.status = h->d_eff + M;
    c.flags = h->d_flag;
    c.v = h->d_v;
    c.a = h->a;
    c.s = h->s;
    c.seed = seed;
    c.streams = streams;
    c.stream = h->stream;
    auto hip = [&](hipError_t e) { return e == hipSuccess ? QC_OK : qcart::host::hip_fail(h->err, e, who); };
    if (const int rc = hip(hipMemcpyAsync(h->d_backup, rho, (size_t)M * plane * sizeof(double2),
                                          hipMemcpyDeviceToDevice, h->stream)))
        return rc;
    if (const int rc = hip(qcart::filter::launch_begin(c))) return rc;
    // the congruences read the call's own slots (eff: -1 from the moment a matrix is dead) and raise a word nobody reads
    int32_t* quiet = h->d_flag + 2;
    if (h->fock)
        if (const int rc = congruence(h, h->d_W, 0, nullptr, r, r, M, c.eff, 0, h->J, who, quiet)) return rc;
    const double* ge = h->eta < 1. ? h->d_ge : nullptr;
    for (int32_t n = 0; n < n_steps; ++n) {
        if (const int rc = congruence(h, h->d_T, plane, ge, r, r, M, c.eff, 0, h->J, who, quiet)) return rc;
        const size_t at = (size_t)n * (size_t)M;
        if (const int rc = hip(qcart::filter::launch_draw(c, (uint64_t)first_step + (uint64_t)n,
                                                          draws ? draws + 2 * at : nullptr,
                                                          record_in ? record_in + at : nullptr,
                                                          record_out ? record_out + at : nullptr)))
            return rc;
        if (const int rc = hip(qcart::filter::launch_apply(c))) return rc;
    }
    if (h->fock)
        if (const int rc = congruence(h, h->d_Wt, 0, nullptr, r, r, M, c.eff, 0, h->J, who, quiet)) return rc;
    return hip(qcart::filter::launch_restore(c, h->d_backup));
}

}  // extern "C"
