// qcart_phase.hip — the phase-space view of density matrices (qc_wigner_eval_rho and qc_spatial_congruence,
// include/qcart.h): the Wigner function of a batch of grid density matrices, and the Fock -> position change of basis
// sigma = s Phi rho Phi^T that brings a Fock-basis rho to the grid first.
//
// k_phase_wigner. With L_ik = rho[i + k][i - k] (the lower triangle) the lag sum is qcart_wigner.hip's contraction,
//     W[i][j] = (2 / pi) sum_{k = 0 .. K_i} ( Re L_ik * C[k][j] + Im L_ik * S[k][j] ),
// C[0] = 1/2, S[0] = 0, on v_mfma_f64_16x16x4_f64 with the handle's own padded table as the B operand and the same
// triangular balancing: a workgroup is one wave, owns a quad of position tiles (tiles (v, T - 1 - v) and their
// short-plus-long partners (U - 1 - v, T - 1 - (U - 1 - v))) and 64 momenta, and a tile's lag loop stops at its
// largest K_i. The A operand is not a product formed from an LDS row of phi: lane (row, q) takes the element
// rho[pos + k][pos - k], k = k0 + q, as it stands. Across a tile these loads are strided ((x_n + 1) elements between
// positions, (x_n - 1) between lags), and every element of rho belongs to exactly one (position, lag): a workgroup
// has nothing to share, so rho is not staged through LDS (a coalesced band would fetch the elements of odd row - col,
// which are never used, and still leave every element with one reader). The lanes gather their elements straight
// from L2. Every load of the loop is unconditional, so the number in flight is known: the gathers and the table
// operands of step k0 + 4 are issued before the MFMAs of step k0, which do not wait for them; the register copies at the
// end of the step do. A row with k > K_i, or past x_n, or of a tile the quad does not have, reads the table's lag-0
// sine row instead (exact zeros: the address is selected, the element is never loaded); the imaginary part of the
// diagonal is replaced by +0 by a select. Stores are guarded per element. The tiling is qcart_wigner_tiles.hpp's.
//
// k_phase_left / k_phase_right: the rectangular real congruence in the manner of qcart_lindblad.hip,
//     left:   Zt[r][c]   = sum_k rho[k][r] Phit[k][c]              (Zt = (Phi rho)^T, [n][x_n], all of it)
//     right:  sigma[i][j] = s * sum_k Zt[k][i] Phit[k][j]          (j <= i, mirrored)
// with Phit[k][c] = Phi[c][k] the transposed table the qc_spatial handle keeps, padded with zeros to whole blocks of
// columns so that its loads need no guard. The operand is real, so each of re and im is one MFMA chain per group of
// four k, not two. A workgroup is one wave and owns 32 x 32 complex elements (2 x 2 tiles x {re, im}), or one 16 x 16
// tile (k_phase_left16 / k_phase_right16) when the launch would have fewer than kWideFrom blocks: the same instructions
// in the same order for every element. Rows and k past the matrix feed exact zeros selected by address.
#include <hip/hip_runtime.h>

#include "qcart_phase.hpp"
#include "qcart_wigner_tiles.hpp"

namespace qcart {
namespace phase {

constexpr int kWave = 64;
using wigner::kNT;                     // the tiling of the contraction is qcart_wigner.hip's
using wigner::kStep;
using wigner::kTP;
using wigner::tile_kmax;
constexpr int kWideFrom = 2048;        // 32 x 32 blocks from this many of them per launch on; below: 16 x 16
using f64x4 = double __attribute__((ext_vector_type(4)));

struct WArgs {
    const double2* rho;      // [M][X][X]
    const double* T;         // the handle's table: [round_up(rows + 1, 4)][2][ldP]
    const double2* zero;     // the table's lag-0 sine row: zeros
    int X, P, ldP;
    double scale;            // fl(2 / pi)
    double* out;             // [M][X][P]
};

// (two waves per SIMD, 256 registers each with the 128 of the accumulators)
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(2))) void k_phase_wigner(WArgs a) {
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
        Ki[t] = on[t] && pos[t] < X ? (pos[t] < far ? pos[t] : far) : -1;
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
    // the anti-diagonal elements of that step: rho[pos + k][pos - k], k = k0 + q (k <= K_i: the row is at most
    // X - 1, the column at least 0); a lane with k > K_i, and every lane of an absent tile, reads the zero. Every load
    // is unconditional, so the number of loads in flight is known at every point of the loop
    const double2* R = a.rho + (size_t)blockIdx.x * (size_t)X * (size_t)X;
    auto gather = [&](int k0, double2 (&g)[4]) {
        const int k = k0 + q;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            g[t] = *(k <= Ki[t] ? R + (size_t)(pos[t] + k) * (size_t)X + (size_t)(pos[t] - k) : a.zero);
    };

    double tc[kNT], ts[kNT], nc[kNT], ns[kNT];
    double2 gc[4], gn[4];
    fetch(0, tc, ts);
    gather(0, gc);
    for (int k0 = 0; k0 <= kend; k0 += kStep) {
        // the next step's operands, in flight behind this step's MFMAs (the last step loads its own again: inside
        // the table and the matrix, not used)
        const int kn = k0 + kStep <= kend ? k0 + kStep : k0;
        fetch(kn, nc, ns);
        gather(kn, gn);
        const bool diag = k0 + q == 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (k0 > kmax[t]) continue;              // (wave-uniform; an absent tile has kmax = -1)
            const double re = gc[t].x, im = diag ? 0. : gc[t].y;
#pragma unroll
            for (int nt = 0; nt < kNT; ++nt) {
                acc[t][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(re, tc[nt], acc[t][nt], 0, 0, 0);
                acc[t][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(im, ts[nt], acc[t][nt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt) {
            tc[nt] = nc[nt];
            ts[nt] = ns[nt];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) gc[t] = gn[t];
    }

    // D element r of tile (t, nt): position 16 tile[t] + q + 4 r, momentum j0 + 16 nt + row
    double* base = a.out + (size_t)blockIdx.x * (size_t)X * (size_t)a.P;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (!on[t]) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * tile[t] + q + 4 * r;
#pragma unroll
            for (int nt = 0; nt < kNT; ++nt) {
                const int j = j0 + 16 * nt + row;
                if (i < X && j < a.P) base[(size_t)i * (size_t)a.P + (size_t)j] = a.scale * acc[t][nt][r];
            }
        }
    }
}

struct CArgs {
    const double2* p;        // [M][K][R], contracted over its leading index: left rho (R = K), right Zt (R = C)
    double2* out;            // left Zt [M][K][C]; right sigma [M][C][C]
    const double* phit;      // [>= round_up(K, 4)][ldX]: phit[k * ldX + c] = Phi[c][k], zero for c >= C
    const double2* zero;     // one complex zero (the handle's)
    size_t pstride, ostride; // the elements of one matrix of p and of out
    int K, R, C, ldX;        // R: the rows of the output; C = x_n: its columns
    int cb, nb;              // left: the column blocks; the blocks of one matrix
    double scale;            // right only
};

template <int T>
struct Operands {
    double2 p[T];
    double q[T];
};

// T x T tiles per workgroup: a block of 16 T rows and columns
template <bool RIGHT, int T>
__device__ __forceinline__ void product(const CArgs& a) {
    constexpr int kBlock = 16 * T;
    const int lane = (int)threadIdx.x, row = lane & 15, q = lane >> 4;
    const int K = a.K, R = a.R, C = a.C;
    const unsigned m = blockIdx.x / (unsigned)a.nb, t = blockIdx.x % (unsigned)a.nb;
    int I, Jb;
    if (RIGHT) {
        I = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
        while (I * (I + 1) / 2 > (int)t) --I;
        while ((I + 1) * (I + 2) / 2 <= (int)t) ++I;
        Jb = (int)t - I * (I + 1) / 2;
    } else {
        I = (int)t / a.cb;
        Jb = (int)t % a.cb;
    }
    const int r0 = kBlock * I, c0 = kBlock * Jb;
    const double2* P = a.p + (size_t)m * a.pstride;

    int ri[T], ci[T];
    bool rok[T], on[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i) {
        ri[i] = r0 + 16 * i + row;
        rok[i] = ri[i] < R;
        ci[i] = c0 + 16 * i + row;                   // (< round_up(C, 32) <= ldX: inside the padded table)
    }
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
            on[i][j] = r0 + 16 * i < R && c0 + 16 * j < C && !(RIGHT && I == Jb && j > i);

    f64x4 re[T][T], im[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) re[i][j] = im[i][j] = f64x4{0., 0., 0., 0.};

    // The operands of the group at k0: a lane whose k or row lies past the matrix reads the handle's zero instead (the
    // address is selected, so every load is unconditional and nothing is multiplied by 0); it takes the table's row 0,
    // a finite value that meets that zero.
    auto fetch = [&](int k0, Operands<T>& o) {
        const int k = k0 + q;
        const bool kok = k < K;
        const size_t base = kok ? (size_t)k * (size_t)R : 0;
        const double* tp = a.phit + (kok ? (size_t)k * (size_t)a.ldX : 0);
#pragma unroll
        for (int i = 0; i < T; ++i) {
            o.p[i] = *(kok && rok[i] ? P + base + ri[i] : a.zero);
            o.q[i] = tp[ci[i]];
        }
    };

    Operands<T> cur, nxt;
    fetch(0, cur);
    for (int k0 = 0; k0 < K; k0 += 4) {
        fetch(k0 + 4, nxt);                          // (past the end: zeros, not used)
        // chain by chain over the tiles, so that consecutive MFMAs do not wait on one accumulator
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    if (!on[i][j]) continue;                             // (wave-uniform)
                    if (c == 0) re[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur.p[i].x, cur.q[j], re[i][j], 0, 0, 0);
                    if (c == 1) im[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur.p[i].y, cur.q[j], im[i][j], 0, 0, 0);
                }
        cur = nxt;
    }

    // D element e of tile (i, j): row r0 + 16 i + q + 4 e, column c0 + 16 j + row
    double2* out = a.out + (size_t)m * a.ostride;
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) {
            if (!on[i][j]) continue;
            const int c = c0 + 16 * j + row;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = r0 + 16 * i + q + 4 * e;
                if (r >= R || c >= C) continue;
                const size_t at = (size_t)r * (size_t)C + (size_t)c;
                if (!RIGHT) {
                    out[at] = make_double2(re[i][j][e], im[i][j][e]);
                    continue;
                }
                if (c > r) continue;                                     // (a diagonal tile's upper half)
                const double vr = a.scale * re[i][j][e], vi = a.scale * im[i][j][e];
                if (c == r) {
                    out[at] = make_double2(vr, 0.);
                } else {
                    out[at] = make_double2(vr, vi);
                    out[(size_t)c * (size_t)C + (size_t)r] = make_double2(vr, -vi);
                }
            }
        }
}

__global__ __launch_bounds__(kWave) void k_phase_left(CArgs a) { product<false, 2>(a); }
__global__ __launch_bounds__(kWave) void k_phase_right(CArgs a) { product<true, 2>(a); }
// one tile per workgroup: four times the waves, for launches that would leave most of the device idle
__global__ __launch_bounds__(kWave) void k_phase_left16(CArgs a) { product<false, 1>(a); }
__global__ __launch_bounds__(kWave) void k_phase_right16(CArgs a) { product<true, 1>(a); }

hipError_t launch_wigner(const double* T, int32_t X, int32_t P, int32_t ldP, const void* rho, int32_t M, double* out,
                         hipStream_t stream) {
    WArgs a{};
    a.rho = (const double2*)rho;
    a.T = T;
    a.zero = (const double2*)(T + ldP);
    a.X = X;
    a.P = P;
    a.ldP = ldP;
    a.scale = (double)(2.0L / 3.14159265358979323846264338327950288L);
    a.out = out;
    const unsigned quads = wigner::tile_quads(X), groups = wigner::momentum_groups(P);
    hipLaunchKernelGGL(k_phase_wigner, dim3((unsigned)M, quads, groups), dim3(kWave), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_congruence(const double* phit, int32_t ldX, const void* zero, int32_t X, int32_t n, const void* rho,
                             int32_t M, double scale, void* Z, void* sigma, hipStream_t stream) {
    CArgs a{};
    a.phit = phit;
    a.ldX = ldX;
    a.zero = (const double2*)zero;
    a.K = n;
    a.C = X;
    a.scale = scale;
    // the block shape changes which workgroup computes an element, never the element: its sums run in the same order
    const int cb32 = (X + 31) / 32;
    const bool wide = (int64_t)cb32 * cb32 * M >= kWideFrom;
    const int block = wide ? 32 : 16;
    a.cb = (X + block - 1) / block;
    a.p = (const double2*)rho;
    a.out = (double2*)Z;
    a.R = n;
    a.pstride = (size_t)n * (size_t)n;
    a.ostride = (size_t)n * (size_t)X;
    a.nb = (n + block - 1) / block * a.cb;
    hipLaunchKernelGGL(wide ? k_phase_left : k_phase_left16, dim3((unsigned)a.nb * (unsigned)M), dim3(kWave), 0, stream,
                       a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    a.p = (const double2*)Z;
    a.out = (double2*)sigma;
    a.R = X;
    a.pstride = (size_t)n * (size_t)X;
    a.ostride = (size_t)X * (size_t)X;
    a.nb = a.cb * (a.cb + 1) / 2;
    hipLaunchKernelGGL(wide ? k_phase_right : k_phase_right16, dim3((unsigned)a.nb * (unsigned)M), dim3(kWave), 0,
                       stream, a);
    return hipGetLastError();
}

}  // namespace phase
}  // namespace qcart
