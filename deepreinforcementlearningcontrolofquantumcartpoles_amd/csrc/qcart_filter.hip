// qcart_filter.hip — the measurement half of the conditional master equation (qc_lindblad_evolve_conditional,
// include/qcart.h), in the eigenbasis of X where a Gaussian position measurement of strength a = eta gamma dt / 2 is the
// rank-one elementwise factor sigma_ij <- (v_i v_j) sigma_ij:
//     k_filter_begin:    the slots of a new call (eff, status), a slot out of range raised
//     k_filter_draw:     one workgroup of 256 threads per matrix: the diagonal d at stride N + 1, its inclusive prefix
//                        sums c, the picked index I and the outcome y (or the given record), e0 = min e_i,
//                        w_i = exp(-a (e_i - e0)), Z = sum w_i^2 d_i, v_i = w_i / sqrt(Z)
//     k_filter_apply:    sigma_ij <- (v_i v_j) sigma_ij, one element per thread (grid x: the elements of one matrix,
//                        (y, z): the matrices)
//     k_filter_restore:  a matrix that could not be stepped gets the bytes it had before the call
// The order of the sums (c and Z are the same routine): indices in chunks of 256 ascending; inside a chunk the
// Hillis-Steele doubling t_i <- t_i + t_(i - s) for s = 1, 2, 4 .. 128 (every i >= s of the chunk at once, elements
// past N enter as +0); c_i = carry + t_i with carry the c of the previous chunk's last element (+0 for the first). A
// function of N alone. Reductions go through LDS with workgroup barriers: nothing assumes a wave's width, no atomics.
// A matrix is dead when c_(N-1), y or Z is not finite or c_(N-1) or Z is not > 0: the draw kernel then writes status 1,
// eff -1 (the congruences of the later steps skip it as they skip a slot out of range), flags[1] and NaN to the record,
// all plain stores of one thread; every decision is taken from LDS values the whole workgroup sees, so its barriers are
// uniform. k_filter_apply reads sigma's own element, v and status (both of an earlier launch) only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qcart_filter.hpp"
#include "qcart_kernels.hpp"

namespace qcart {
namespace filter {

constexpr int kT = 256;
constexpr int kMaxN = lindblad::kMaxGrid;              // (>= the Fock limit)
constexpr unsigned kGridY = 65535;                     // matrices per grid row of the elementwise kernels

struct DrawArgs {
    const double2* sigma;
    const double* xi;
    int32_t N;
    int32_t* eff;
    int32_t* status;
    int32_t* flags;
    double* v;
    double a, s;
    uint64_t seed, step;
    const int32_t* streams;
    const double* draws;       // [M][2] of this step, or null
    const double* record_in;   // [M] of this step, or null
    double* record_out;        // [M] of this step, or null
};

// the inclusive prefix sums of term(0 .. N - 1) into out (LDS), in the order the file's head documents; returns c_(N-1)
template <class F>
__device__ __forceinline__ double scan(int N, F term, double* sh, double* out) {
    const int t = (int)threadIdx.x;
    double carry = 0.;
    for (int base = 0; base < N; base += kT) {
        const int i = base + t;
        double x = i < N ? term(i) : 0.;
        sh[t] = x;
        __syncthreads();
        for (int s = 1; s < kT; s <<= 1) {
            const double y = t >= s ? sh[t - s] : 0.;
            __syncthreads();
            if (t >= s) {
                x = x + y;
                sh[t] = x;
            }
            __syncthreads();
        }
        if (i < N) out[i] = carry + x;
        carry = carry + sh[kT - 1];
        __syncthreads();
    }
    return out[N - 1];
}

__device__ __forceinline__ double weight(double xi, double y, double e0, double a) {
    const double d = xi - y, e = d * d;
    return exp(-(a * (e - e0)));
}

__global__ __launch_bounds__(kT) void k_filter_draw(DrawArgs a) {
    __shared__ double csum[kMaxN];
    __shared__ double sh[kT];
    __shared__ int shi[kT];
    __shared__ double bc[2];
    __shared__ int alive;
    const int t = (int)threadIdx.x, N = a.N;
    const size_t m = blockIdx.x;
    if (t == 0) alive = a.status[m] == 0;
    __syncthreads();
    const double nan = __builtin_nan("");
    if (!alive) {
        if (t == 0 && a.record_out) a.record_out[m] = nan;
        return;
    }
    const double2* S = a.sigma + m * (size_t)N * (size_t)N;
    // d_i: Re sigma_ii where that is not below 0 (a NaN stays and reaches c_(N-1))
    auto diag = [&](int i) {
        const double re = S[(size_t)i * (size_t)(N + 1)].x;
        return re < 0. ? 0. : re;
    };
    const double total = scan(N, diag, sh, csum);
    bool ok = total > 0. && total <= DBL_MAX;
    double y = nan;
    if (ok) {
        if (a.record_in) {
            y = a.record_in[m];
        } else {
            if (t == 0) {
                double u, z;
                if (a.draws) {
                    u = a.draws[2 * m];
                    z = a.draws[2 * m + 1];
                } else {
                    const uint32_t stream = a.streams ? (uint32_t)a.streams[m] : (uint32_t)m;
                    uint32_t c[4] = {(uint32_t)a.step, (uint32_t)(a.step >> 32), stream, kTagPick};
                    qcart::philox10(c, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
                    u = ((double)(((((uint64_t)c[0]) << 32) | c[1]) >> 11) + 0.5) * 0x1.0p-53;
                    double r1;
                    qcart::normals(a.seed, stream, a.step, kTagNoise, z, r1);
                }
                bc[0] = u;
                bc[1] = z;
            }
            __syncthreads();
            // I = min { i : c_i > u c_(N-1) }; N - 1 where no c_i is (u = 1 after rounding)
            const double thresh = bc[0] * total;
            int mine = N - 1;
            for (int i = t; i < N; i += kT)
                if (csum[i] > thresh) {
                    mine = i;
                    break;
                }
            shi[t] = mine;
            __syncthreads();
            for (int s = kT / 2; s > 0; s >>= 1) {
                if (t < s) shi[t] = min(shi[t], shi[t + s]);
                __syncthreads();
            }
            y = fma(bc[1], a.s, a.xi[shi[0]]);
        }
        ok = y >= -DBL_MAX && y <= DBL_MAX;
    }
    double Z = 0., e0 = 0.;
    if (ok) {
        double mine = DBL_MAX;
        for (int i = t; i < N; i += kT) {
            const double d = a.xi[i] - y;
            mine = fmin(mine, d * d);
        }
        __syncthreads();                               // (the pick's reads of sh / shi are over)
        sh[t] = mine;
        __syncthreads();
        for (int s = kT / 2; s > 0; s >>= 1) {
            if (t < s) sh[t] = fmin(sh[t], sh[t + s]);
            __syncthreads();
        }
        e0 = sh[0];
        __syncthreads();
        auto term = [&](int i) {
            const double w = weight(a.xi[i], y, e0, a.a);
            return (w * w) * diag(i);
        };
        Z = scan(N, term, sh, csum);
        ok = Z > 0. && Z <= DBL_MAX;
    }
    if (!ok) {
        if (t == 0) {
            a.status[m] = 1;
            a.eff[m] = -1;
            a.flags[1] = 1;
            if (a.record_out) a.record_out[m] = nan;
        }
        return;
    }
    const double root = sqrt(Z);
    for (int i = t; i < N; i += kT) a.v[m * (size_t)N + (size_t)i] = weight(a.xi[i], y, e0, a.a) / root;
    if (t == 0 && a.record_out) a.record_out[m] = y;
}

__global__ __launch_bounds__(kT) void k_filter_apply(double2* sigma, const double* v, const int32_t* status, int N,
                                                     int M) {
    // the matrix is the block's (y, z), the element inside it the block's x: no 64-bit division
    const unsigned m = blockIdx.z * kGridY + blockIdx.y, r = blockIdx.x * kT + threadIdx.x;
    const unsigned plane = (unsigned)N * (unsigned)N;              // (N <= 2048)
    if (m >= (unsigned)M || r >= plane) return;
    if (status[m] != 0) return;
    const unsigned i = r / (unsigned)N, j = r - i * (unsigned)N;
    const size_t e = (size_t)m * plane + r;
    const double* vm = v + (size_t)m * (size_t)N;
    const double f = vm[i] * vm[j];
    const double2 x = sigma[e];
    sigma[e] = make_double2(f * x.x, f * x.y);
}

__global__ __launch_bounds__(kT) void k_filter_begin(const int32_t* slots, int32_t default_slot, int32_t J, int M,
                                                     int32_t* eff, int32_t* status, int32_t* flags) {
    const int m = (int)(blockIdx.x * kT + threadIdx.x);
    if (m >= M) return;
    const int32_t slot = slots ? slots[m] : default_slot;
    const bool in = slot >= 0 && slot < J;
    eff[m] = in ? slot : -1;
    status[m] = in ? 0 : 1;
    if (!in) flags[0] = 1;
}

__global__ __launch_bounds__(kT) void k_filter_restore(double2* rho, const double2* backup, const int32_t* status,
                                                       int N, int M) {
    const unsigned m = blockIdx.z * kGridY + blockIdx.y, r = blockIdx.x * kT + threadIdx.x;
    const unsigned plane = (unsigned)N * (unsigned)N;
    if (m >= (unsigned)M || r >= plane) return;
    if (status[m] == 0) return;
    const size_t e = (size_t)m * plane + r;
    rho[e] = backup[e];
}

namespace {
unsigned blocks(size_t n) { return (unsigned)((n + kT - 1) / kT); }
// the elementwise kernels' grid: x over one matrix's elements, (y, z) over the matrices
dim3 per_matrix(const Call& c) {
    const unsigned M = (unsigned)c.M;
    return dim3(blocks((size_t)c.N * (size_t)c.N), M < kGridY ? M : kGridY, (M + kGridY - 1) / kGridY);
}
}  // namespace

hipError_t launch_begin(const Call& c) {
    hipLaunchKernelGGL(k_filter_begin, dim3(blocks((size_t)c.M)), dim3(kT), 0, c.stream, c.slots, c.default_slot, c.J,
                       (int)c.M, c.eff, c.status, c.flags);
    return hipGetLastError();
}

hipError_t launch_draw(const Call& c, uint64_t step, const double* draws, const double* record_in,
                       double* record_out) {
    DrawArgs a{};
    a.sigma = (const double2*)c.sigma;
    a.xi = c.xi;
    a.N = c.N;
    a.eff = c.eff;
    a.status = c.status;
    a.flags = c.flags;
    a.v = c.v;
    a.a = c.a;
    a.s = c.s;
    a.seed = c.seed;
    a.step = step;
    a.streams = c.streams;
    a.draws = draws;
    a.record_in = record_in;
    a.record_out = record_out;
    hipLaunchKernelGGL(k_filter_draw, dim3((unsigned)c.M), dim3(kT), 0, c.stream, a);
    return hipGetLastError();
}

hipError_t launch_apply(const Call& c) {
    hipLaunchKernelGGL(k_filter_apply, per_matrix(c), dim3(kT), 0, c.stream, (double2*)c.sigma,
                       (const double*)c.v, (const int32_t*)c.status, (int)c.N, (int)c.M);
    return hipGetLastError();
}

hipError_t launch_restore(const Call& c, const void* backup) {
    hipLaunchKernelGGL(k_filter_restore, per_matrix(c), dim3(kT), 0, c.stream, (double2*)c.sigma,
                       (const double2*)backup, (const int32_t*)c.status, (int)c.N, (int)c.M);
    return hipGetLastError();
}

}  // namespace filter
}  // namespace qcart
