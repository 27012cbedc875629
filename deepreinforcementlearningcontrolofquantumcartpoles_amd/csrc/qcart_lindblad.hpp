// qcart_lindblad.hpp — the host side of the master equation (qc_lindblad, include/qcart.h): the tables of one step of
//     d rho / dt = -i [H_F, rho] - (gamma / 4) [X, [X, rho]],   H_F = H - c F X,
// and the argument checks of the handle; written once for the library (qcart_lindblad.hip) and for plain C++ programs
// (tests/diag/lindblad_check.cpp). No HIP type appears here. Internal: not part of the C ABI.
//
// Everything is computed in long double and rounded once to fp64:
//   * xi, W: X = W diag(xi) W^T. Fock: all N eigenpairs of the symmetric tridiagonal X[i][i + 1] = x[i] by
//     qcart_levels.hpp's band solver with K = N (xi ascending, the sign of column k by its convention; its K <= 256
//     bounds the Fock size). The solver returns fp64 only, so the long double xi_k is recovered as the Rayleigh quotient
//     w_k^T X w_k / w_k^T w_k of the returned column (its error is the square of the column's, far below 2^-64); the
//     fp64 xi is that value rounded. Grid: xi = x, W = I exactly.
//   * C = (I + i dt/2 H_F)^-1 (I - i dt/2 H_F) by a partially pivoted complex band LU against the N columns of the right
//     side, H_F[i][i + d] = hband - (c F) X; T = W^T C W from the fp64 W (grid: T = C).
//   * G_ij = exp(-gamma dt (xi_i - xi_j)^2 / 4) and G½_ij = exp(-gamma dt (xi_i - xi_j)^2 / 8), each by expl from the
//     long double xi (G is not the square of the rounded G½); the argument is formed once for i > j and mirrored, the diagonal
//     is 1 exactly.
// Deterministic: no randomness, no threads.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/qcart.h"
#include "qcart_levels.hpp"

namespace qcart {
namespace lindblad {

using ld = long double;

constexpr int32_t kMaxFock = 256;                      // (qcart_levels.hpp's K <= 256)
constexpr int32_t kMinGrid = 9, kMaxGrid = 2048;
constexpr int32_t kMaxJ = 32;
constexpr int64_t kMaxTable = (int64_t)1 << 25;        // J N^2
constexpr int64_t kMaxBatch = (int64_t)1 << 27;        // M N^2 (the handle's Z buffer: 2 GiB)

// the first refusal, or nullptr
inline const char* bad_step(double dt, double gamma) {
    if (!std::isfinite(dt) || !(dt > 0.)) return "dt must be finite and > 0";
    if (!std::isfinite(gamma) || !(gamma >= 0.)) return "gamma must be finite and >= 0";
    return nullptr;
}
inline const char* bad_force(double force) { return std::isfinite(force) ? nullptr : "every force must be finite"; }
inline const char* bad_precision(int32_t precision) {
    return precision == 0 ? nullptr : "fp32 physics is not evolved (precision must be 0)";
}
inline const char* bad_dim(bool fock, int32_t N) {
    if (fock) return N >= 1 && N <= kMaxFock ? nullptr : "the Fock families are evolved up to N = 256";
    return N >= kMinGrid && N <= kMaxGrid ? nullptr : "the grid must have 9 to 2048 points";
}
inline const char* bad_slots(int32_t J, int32_t N) {
    if (J < 1 || J > kMaxJ) return "J must be in [1, 32]";
    if ((int64_t)J * N * N > kMaxTable) return "J N^2 must be <= 2^25";
    return nullptr;
}
inline const char* bad_batch(int32_t M, int32_t N) {
    if (M < 1) return "M must be >= 1";
    if ((int64_t)M * N * N > kMaxBatch) return "M N^2 must be <= 2^27";
    return nullptr;
}
inline const char* bad_evolve(const void* rho, int32_t M, int32_t N, const void* slots, int32_t default_slot, int32_t J,
                              int32_t n_steps) {
    if (!rho) return "rho is required";
    if (const char* bad = bad_batch(M, N)) return bad;
    if (n_steps < 0) return "n_steps must be >= 0";
    if (!slots && (default_slot < 0 || default_slot >= J)) return "default_slot must be in [0, J)";
    return nullptr;
}
inline const char* bad_congruence(const void* A, const void* x, const void* y, int32_t M, int32_t N) {
    if (!A || !x || !y) return "A, x and y are required";
    return bad_batch(M, N);
}

struct cld {
    ld re = 0, im = 0;
};
inline cld operator*(cld a, cld b) { return cld{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
inline cld operator-(cld a, cld b) { return cld{a.re - b.re, a.im - b.im}; }
inline cld operator/(cld a, cld b) {                   // (Smith's division)
    if (fabsl(b.re) >= fabsl(b.im)) {
        const ld t = b.im / b.re, d = b.re + b.im * t;
        return cld{(a.re + a.im * t) / d, (a.im - a.re * t) / d};
    }
    const ld t = b.re / b.im, d = b.re * t + b.im;
    return cld{(a.re * t + a.im) / d, (a.im * t - a.re) / d};
}
inline ld abs1(cld a) { return fabsl(a.re) + fabsl(a.im); }

// What the tables are made from: the real band hband[(d + kl) * N + i] = H[i][i + d] (qcart_tables.hpp's op.hband),
// x = op.xu (Fock: X[i][i + 1], i < N - 1) or op.xg (grid: x_i), c = op.c.
struct Source {
    bool fock = true;
    int32_t N = 0, kl = 0;
    const double* hband = nullptr;
    const double* x = nullptr;
    double c = 0.;
};

inline const char* bad_source(const Source& s) {
    if (!s.hband || !s.x) return "the band and x are required";
    if (const char* bad = bad_dim(s.fock, s.N)) return bad;
    if (s.kl < 1 || s.kl > 16) return "the half bandwidth must be in [1, 16]";
    return nullptr;
}

// Fock: xi [N] in long double and W [N][N] (W[j][k] = component j of eigenvector k); QC_OK, or the refusal with *why set
inline int basis(const Source& s, ld* xi, double* W, const char** why) {
    const int N = s.N;
    if (N == 1) {
        xi[0] = 0;
        W[0] = 1.;
        return QC_OK;
    }
    std::vector<double> band((size_t)3 * N, 0.), V((size_t)N * N);
    for (int i = 0; i + 1 < N; ++i) {
        band[(size_t)2 * N + i] = s.x[i];              // X[i][i + 1]
        band[(size_t)i + 1] = s.x[i];                  // X[i + 1][i]
    }
    std::vector<double> e((size_t)N);
    if (const int rc = levels::solve(band.data(), N, 1, N, e.data(), V.data(), why)) return rc;
    for (int k = 0; k < N; ++k) {
        const double* v = &V[(size_t)k * N];
        ld num = 0, den = 0;
        for (int j = 0; j < N; ++j) {
            if (j + 1 < N) num += 2 * (ld)s.x[j] * (ld)v[j] * (ld)v[j + 1];
            den += (ld)v[j] * (ld)v[j];
            W[(size_t)j * N + k] = v[j];
        }
        xi[k] = num / den;
    }
    return QC_OK;
}

// the partially pivoted complex band LU of I + i dt/2 H_F (row i holds the columns i - kl .. i + 2 kl)
struct BandLU {
    int N = 0, kl = 0, w = 0;
    std::vector<cld> b;
    std::vector<int> piv;
    cld& at(int i, int col) { return b[(size_t)i * (size_t)w + (size_t)(col - i + kl)]; }

    // false: a zero pivot
    bool factor(int N_, int kl_, const std::vector<ld>& hf /* [N][2 kl + 1] */, ld half_dt) {
        N = N_;
        kl = kl_;
        w = 3 * kl + 1;
        b.assign((size_t)N * (size_t)w, cld{});
        piv.assign((size_t)N, 0);
        for (int i = 0; i < N; ++i)
            for (int d = -kl; d <= kl; ++d)
                if (i + d >= 0 && i + d < N)
                    at(i, i + d) = cld{d == 0 ? (ld)1 : (ld)0, half_dt * hf[(size_t)i * (size_t)(2 * kl + 1) + (size_t)(d + kl)]};
        for (int j = 0; j < N; ++j) {
            const int rmax = j + kl < N - 1 ? j + kl : N - 1, cmax = j + 2 * kl < N - 1 ? j + 2 * kl : N - 1;
            int p = j;
            for (int r = j + 1; r <= rmax; ++r)
                if (abs1(at(r, j)) > abs1(at(p, j))) p = r;
            piv[(size_t)j] = p;
            if (p != j)
                for (int c = j; c <= cmax; ++c) {
                    const cld t = at(j, c);
                    at(j, c) = at(p, c);
                    at(p, c) = t;
                }
            const cld d = at(j, j);
            if (d.re == 0 && d.im == 0) return false;
            for (int r = j + 1; r <= rmax; ++r) {
                const cld m = at(r, j) / d;
                at(r, j) = m;
                if (m.re != 0 || m.im != 0)
                    for (int c = j + 1; c <= cmax; ++c) at(r, c) = at(r, c) - m * at(j, c);
            }
        }
        return true;
    }

    void solve(cld* x) {
        for (int j = 0; j < N; ++j) {
            const int p = piv[(size_t)j];
            if (p != j) {
                const cld t = x[j];
                x[j] = x[p];
                x[p] = t;
            }
            const int rmax = j + kl < N - 1 ? j + kl : N - 1;
            for (int r = j + 1; r <= rmax; ++r) x[r] = x[r] - at(r, j) * x[j];
        }
        for (int j = N - 1; j >= 0; --j) {
            const int cmax = j + 2 * kl < N - 1 ? j + 2 * kl : N - 1;
            cld s = x[j];
            for (int c = j + 1; c <= cmax; ++c) s = s - at(j, c) * x[c];
            x[j] = s / at(j, j);
        }
    }
};

// H_F [N][2 kl + 1] in long double: hband - (c F) X
inline std::vector<ld> force_band(const Source& s, double force) {
    const int N = s.N, kl = s.kl, wd = 2 * kl + 1;
    std::vector<ld> hf((size_t)N * (size_t)wd, 0);
    const ld cf = (ld)s.c * (ld)force;
    for (int i = 0; i < N; ++i)
        for (int d = -kl; d <= kl; ++d) {
            const int j = i + d;
            if (j < 0 || j >= N) continue;
            ld x = 0;
            if (s.fock) {
                if (d == 1) x = (ld)s.x[i];
                if (d == -1) x = (ld)s.x[j];
            } else if (d == 0) {
                x = (ld)s.x[i];
            }
            hf[(size_t)i * (size_t)wd + (size_t)(d + kl)] = (ld)s.hband[(size_t)(d + kl) * (size_t)N + (size_t)i] - cf * x;
        }
    return hf;
}

// T [N][N] (re, im interleaved) = W^T C W of one force; W: basis()'s (grid: not read). QC_OK or the refusal.
inline int propagator(const Source& s, double dt, double force, const double* W, double* T, const char** why) {
    const int N = s.N, kl = s.kl, wd = 2 * kl + 1;
    const std::vector<ld> hf = force_band(s, force);
    const ld half_dt = (ld)dt / 2;
    BandLU lu;
    if (!lu.factor(N, kl, hf, half_dt)) {
        *why = "I + i dt/2 H_F is singular";
        return QC_ESINGULAR;
    }
    std::vector<cld> col((size_t)N), C;
    if (s.fock) C.assign((size_t)N * N, cld{});
    for (int j = 0; j < N; ++j) {
        // column j of I - i dt/2 H_F: H_F[i][j] for |i - j| <= kl
        for (int i = 0; i < N; ++i) col[(size_t)i] = cld{};
        for (int d = -kl; d <= kl; ++d) {
            const int i = j - d;                       // H_F[i][i + d], i + d = j
            if (i < 0 || i >= N) continue;
            col[(size_t)i] = cld{d == 0 ? (ld)1 : (ld)0, -(half_dt * hf[(size_t)i * (size_t)wd + (size_t)(d + kl)])};
        }
        lu.solve(col.data());
        for (int i = 0; i < N; ++i) {
            if (s.fock) {
                C[(size_t)i * N + j] = col[(size_t)i];
            } else {
                T[2 * ((size_t)i * N + j)] = (double)col[(size_t)i].re;
                T[2 * ((size_t)i * N + j) + 1] = (double)col[(size_t)i].im;
            }
        }
    }
    if (!s.fock) return QC_OK;
    // D = C W, then T = W^T D
    std::vector<cld> D((size_t)N * N);
    for (int i = 0; i < N; ++i)
        for (int k = 0; k < N; ++k) {
            const cld c = C[(size_t)i * N + k];
            if (c.re == 0 && c.im == 0) continue;
            const double* wk = W + (size_t)k * N;
            cld* di = &D[(size_t)i * N];
            for (int j = 0; j < N; ++j) {
                di[j].re += c.re * (ld)wk[j];
                di[j].im += c.im * (ld)wk[j];
            }
        }
    std::vector<cld> row((size_t)N);
    for (int i = 0; i < N; ++i) {
        for (int j = 0; j < N; ++j) row[(size_t)j] = cld{};
        for (int k = 0; k < N; ++k) {
            const ld w = (ld)W[(size_t)k * N + i];
            const cld* dk = &D[(size_t)k * N];
            for (int j = 0; j < N; ++j) {
                row[(size_t)j].re += w * dk[j].re;
                row[(size_t)j].im += w * dk[j].im;
            }
        }
        for (int j = 0; j < N; ++j) {
            T[2 * ((size_t)i * N + j)] = (double)row[(size_t)j].re;
            T[2 * ((size_t)i * N + j) + 1] = (double)row[(size_t)j].im;
        }
    }
    return QC_OK;
}

// G½ and G [N][N] from the long double xi (either may be null)
// (dt and gamma in long double: a double converts exactly; the conditional evolution passes gamma (1 - eta) unrounded)
inline void gauss(int32_t N, const ld* xi, ld dt, ld gamma, double* g_half, double* g_full) {
    const ld gd = gamma * dt;
    for (int i = 0; i < N; ++i)
        for (int j = 0; j <= i; ++j) {
            const ld d = xi[i] - xi[j], a = gd * d * d;
            const double h = i == j ? 1. : (double)expl(-a / 8), f = i == j ? 1. : (double)expl(-a / 4);
            if (g_half) g_half[(size_t)i * N + j] = g_half[(size_t)j * N + i] = h;
            if (g_full) g_full[(size_t)i * N + j] = g_full[(size_t)j * N + i] = f;
        }
}

// What does not depend on dt, gamma or the force: xi in long double and W (empty for the grid: the identity)
struct Basis {
    std::vector<ld> xi;
    std::vector<double> W;
};

// checks the source and builds its basis; QC_OK, or the refusal with *why set to its text
inline int make_basis(const Source& s, Basis& b, const char** why) {
    if ((*why = bad_source(s))) return QC_EINVAL;
    const int N = s.N;
    for (int i = 0; i < N; ++i) {
        if (!std::isfinite(s.x[i])) *why = "every table entry must be finite";
        for (int d = -s.kl; d <= s.kl; ++d)
            if (i + d >= 0 && i + d < N && !std::isfinite(s.hband[(size_t)(d + s.kl) * (size_t)N + (size_t)i]))
                *why = "every table entry must be finite";
    }
    if (*why) return QC_EINVAL;
    b.xi.assign((size_t)N, 0);
    b.W.clear();
    if (s.fock) {
        b.W.assign((size_t)N * N, 0.);
        return basis(s, b.xi.data(), b.W.data(), why);
    }
    for (int i = 0; i < N; ++i) b.xi[(size_t)i] = s.x[i];
    return QC_OK;
}

// The table set of one force on a basis made once (a handle's forces share it); any output may be null.
inline int tables_on(const Source& s, const Basis& b, double dt, double gamma, double force, double* xi, double* W,
                     double* T, double* g_half, double* g_full, const char** why) {
    if ((*why = bad_step(dt, gamma)) || (*why = bad_force(force))) return QC_EINVAL;
    const int N = s.N;
    if (T)
        if (const int rc = propagator(s, dt, force, s.fock ? b.W.data() : nullptr, T, why)) return rc;
    if (xi)
        for (int i = 0; i < N; ++i) xi[i] = (double)b.xi[(size_t)i];
    if (W)
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j)
                W[(size_t)i * N + j] = s.fock ? b.W[(size_t)i * N + j] : i == j ? 1. : 0.;
    if (g_half || g_full) gauss(N, b.xi.data(), dt, gamma, g_half, g_full);
    return QC_OK;
}

// The whole table set of one force; any output may be null. QC_OK, or the refusal with *why set to its text.
inline int tables(const Source& s, double dt, double gamma, double force, double* xi, double* W, double* T,
                  double* g_half, double* g_full, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    *why = nullptr;
    if ((*why = bad_source(s)) || (*why = bad_step(dt, gamma)) || (*why = bad_force(force))) return QC_EINVAL;
    Basis b;
    if (const int rc = make_basis(s, b, why)) return rc;
    return tables_on(s, b, dt, gamma, force, xi, W, T, g_half, g_full, why);
}

}  // namespace lindblad
}  // namespace qcart
