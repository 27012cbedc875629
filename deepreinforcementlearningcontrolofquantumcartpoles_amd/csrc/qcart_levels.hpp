// qcart_levels.hpp — the host side of the energy-level view (qc_levels, include/qcart.h): the lowest K eigenpairs of a
// real symmetric band matrix (the force-free Hamiltonian's op.hband of qcart_tables.cpp), and the argument checks of
// the handle; written once for the library (qcart_levels.hip) and for plain C++ programs
// (tests/diag/levels_check.cpp). No HIP type appears here. Internal: not part of the C ABI.
//
// The solve, in long double throughout and rounded once to fp64 at the end:
//   * a band without any off-diagonal entry splits into 1 x 1 blocks: the levels are the diagonal entries in
//     ascending order (ties broken by index) and the vectors the unit vectors, exactly (the HO family);
//   * otherwise level k is bracketed by bisection on the inertia of the band L D L^T of H - sigma (the number of
//     negative pivots = the number of eigenvalues below sigma; a zero pivot is replaced by a tiny one), O(N kl^2) per
//     shift, down to a bracket of 2^-40 ||H||_inf;
//   * its vector by inverse iteration with a partially pivoted band LU of H - sigma from a fixed start vector,
//     orthogonalised against the levels already found, the shift moved to the Rayleigh quotient after each solve,
//     until ||H x - rho x||_inf <= 2^-58 ||H||_inf;
//   * a level that does not get there, whose Rayleigh quotient leaves the bracket, or two levels closer than
//     2^-20 ||H||_inf, refuse the whole solve (QC_ESINGULAR): never garbage.
// Sign: the last entry j with |V[k][j]| > 2^-26 max_j |V[k][j]| is positive (decided on the rounded values).
// The working storage is O(N kl + K N): nothing proportional to N^2. Deterministic: no randomness, no threads.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/qcart.h"

namespace qcart {
namespace levels {

#if !defined(__HIP_DEVICE_COMPILE__)   // (host code only: the device pass of a HIP compile has no extended type)
static_assert(LDBL_MANT_DIG >= 64, "the levels are computed in an extended long double and rounded once to fp64");
#endif

using ld = long double;

constexpr int32_t kMaxN = 2048;
constexpr int32_t kMaxK = 256;
constexpr int32_t kMaxB = INT32_MAX - 64;              // (a workgroup's padding stays inside int32)

// the first refusal of a solve's (family, N, K), or nullptr
inline const char* bad_family(int32_t family) {
    if (family == QC_IHO || family == QC_IQO) return "no bound levels: H is not bounded below";
    if (family != QC_HO && family != QC_QO) return "unknown family";
    return nullptr;
}
inline const char* bad_k(int32_t N, int32_t K) {
    if (N < 1 || N > kMaxN) return "N must be in [1, 2048]";
    if (K < 1 || K > N || K > kMaxK) return "K must be in [1, min(N, 256)]";
    return nullptr;
}

// the first refusal of the create arguments, or nullptr
inline const char* bad_create(int32_t N, int32_t K, double scale, const double* vectors) {
    if (const char* bad = bad_k(N, K)) return bad;
    if (!std::isfinite(scale) || !(scale > 0.)) return "scale must be finite and > 0";
    if (!vectors) return "vectors are required";
    const size_t n = (size_t)K * (size_t)N;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(vectors[i])) return "every table entry must be finite";
    return nullptr;
}

// the first refusal of a call's arguments, or nullptr
inline const char* bad_call(const void* psi, int32_t B, const void* out) {
    if (!psi || !out) return "psi and out are required";
    if (B < 1 || B > kMaxB) return "B must be >= 1";
    return nullptr;
}

// the padded device table: [round_up(K, 64)][round_up(N, 16)], zero outside [K][N]
inline int32_t padded_rows(int32_t K) { return (K + 63) / 64 * 64; }
inline int32_t padded_cols(int32_t N) { return (N + 15) / 16 * 16; }

// A real symmetric band in long double: at(i, d) = H[i][i + d], |d| <= kl, zero outside the matrix.
struct Band {
    int N = 0, kl = 0;
    std::vector<ld> a;   // [N][2 kl + 1]
    ld norm = 0;         // ||H||_inf
    ld at(int i, int d) const { return a[(size_t)i * (size_t)(2 * kl + 1) + (size_t)(d + kl)]; }
};

// hband[(d + kl) * N + i] = H[i][i + d]; only the entries inside the matrix are read
inline Band make_band(const double* hband, int N, int kl) {
    Band b;
    b.N = N;
    b.kl = kl;
    b.a.assign((size_t)N * (size_t)(2 * kl + 1), 0);
    for (int i = 0; i < N; ++i) {
        ld row = 0;
        for (int d = -kl; d <= kl; ++d) {
            if (i + d < 0 || i + d >= N) continue;
            const ld v = (ld)hband[(size_t)(d + kl) * (size_t)N + (size_t)i];
            b.a[(size_t)i * (size_t)(2 * kl + 1) + (size_t)(d + kl)] = v;
            row += fabsl(v);
        }
        if (row > b.norm) b.norm = row;
    }
    return b;
}

// y = H x
inline void apply(const Band& h, const ld* x, ld* y) {
    for (int i = 0; i < h.N; ++i) {
        ld s = 0;
        const int lo = i - h.kl < 0 ? -i : -h.kl, hi = i + h.kl >= h.N ? h.N - 1 - i : h.kl;
        for (int d = lo; d <= hi; ++d) s += h.at(i, d) * x[i + d];
        y[i] = s;
    }
}

// the number of eigenvalues of H below sigma: the negative pivots of the band L D L^T of H - sigma.
// w: workspace [N][kl + 1], w[j][t] = the current entry (j + t, j)
inline int count_below(const Band& h, ld sigma, ld tiny, std::vector<ld>& w) {
    const int N = h.N, kl = h.kl, ld_ = kl + 1;
    for (int j = 0; j < N; ++j)
        for (int t = 0; t <= kl; ++t) w[(size_t)j * ld_ + t] = j + t < N ? h.at(j + t, -t) : (ld)0;
    int neg = 0;
    for (int j = 0; j < N; ++j) {
        ld d = w[(size_t)j * ld_] - sigma;
        if (d == 0) d = -tiny;
        if (d < 0) ++neg;
        const int km = N - 1 - j < kl ? N - 1 - j : kl;
        for (int t = 1; t <= km; ++t) {
            const ld lt = w[(size_t)j * ld_ + t] / d;
            // entry (j + s, j + t), s >= t, loses a[j + s][j] * a[j + t][j] / d
            for (int s = t; s <= km; ++s) w[(size_t)(j + t) * ld_ + (s - t)] -= w[(size_t)j * ld_ + s] * lt;
        }
    }
    return neg;
}

// the partially pivoted band LU of H - sigma (rows i hold the columns i - kl .. i + 2 kl), and its solves
struct BandLU {
    int N = 0, kl = 0, w = 0;
    std::vector<ld> b;       // [N][3 kl + 1]
    std::vector<int> piv;    // [N]
    ld& at(int i, int col) { return b[(size_t)i * (size_t)w + (size_t)(col - i + kl)]; }

    void factor(const Band& h, ld sigma, ld tiny) {
        N = h.N;
        kl = h.kl;
        w = 3 * kl + 1;
        b.assign((size_t)N * (size_t)w, 0);
        piv.assign((size_t)N, 0);
        for (int i = 0; i < N; ++i)
            for (int d = -kl; d <= kl; ++d)
                if (i + d >= 0 && i + d < N) at(i, i + d) = h.at(i, d) - (d == 0 ? sigma : (ld)0);
        for (int j = 0; j < N; ++j) {
            const int rmax = j + kl < N - 1 ? j + kl : N - 1, cmax = j + 2 * kl < N - 1 ? j + 2 * kl : N - 1;
            int p = j;
            for (int r = j + 1; r <= rmax; ++r)
                if (fabsl(at(r, j)) > fabsl(at(p, j))) p = r;
            piv[(size_t)j] = p;
            if (p != j)
                for (int c = j; c <= cmax; ++c) {
                    const ld t = at(j, c);
                    at(j, c) = at(p, c);
                    at(p, c) = t;
                }
            if (at(j, j) == 0) at(j, j) = tiny;
            const ld d = at(j, j);
            for (int r = j + 1; r <= rmax; ++r) {
                const ld m = at(r, j) / d;
                at(r, j) = m;
                if (m != 0)
                    for (int c = j + 1; c <= cmax; ++c) at(r, c) -= m * at(j, c);
            }
        }
    }

    void solve(ld* x) {
        for (int j = 0; j < N; ++j) {
            const int p = piv[(size_t)j];
            if (p != j) {
                const ld t = x[j];
                x[j] = x[p];
                x[p] = t;
            }
            const int rmax = j + kl < N - 1 ? j + kl : N - 1;
            for (int r = j + 1; r <= rmax; ++r) x[r] -= at(r, j) * x[j];
        }
        for (int j = N - 1; j >= 0; --j) {
            const int cmax = j + 2 * kl < N - 1 ? j + 2 * kl : N - 1;
            ld s = x[j];
            for (int c = j + 1; c <= cmax; ++c) s -= at(j, c) * x[c];
            x[j] = s / at(j, j);
        }
    }
};

inline ld dot(const ld* a, const ld* b, int n) {
    ld s = 0;
    for (int i = 0; i < n; ++i) s += a[i] * b[i];
    return s;
}

// The lowest K eigenpairs of the band (hband, N, kl): energies [K] ascending, vectors [K][N]. QC_OK, or the refusal
// with *why set to its text.
inline int solve(const double* hband, int32_t N, int32_t kl, int32_t K, double* energies, double* vectors,
                 const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    *why = nullptr;
    if (!hband || !energies || !vectors) {
        *why = "band, energies and vectors are required";
        return QC_EINVAL;
    }
    if (const char* bad = bad_k(N, K)) {
        *why = bad;
        return QC_EINVAL;
    }
    if (kl < 0 || kl > 16) {
        *why = "the half bandwidth must be in [0, 16]";
        return QC_EINVAL;
    }
    for (int i = 0; i < N; ++i)
        for (int d = -kl; d <= kl; ++d)
            if (i + d >= 0 && i + d < N && !std::isfinite(hband[(size_t)(d + kl) * (size_t)N + (size_t)i])) {
                *why = "every band entry must be finite";
                return QC_EINVAL;
            }
    const Band h = make_band(hband, N, kl);
    const ld close = ldexpl(h.norm, -20);

    bool diagonal = true;
    for (int i = 0; i < N && diagonal; ++i)
        for (int d = 1; d <= kl && i + d < N; ++d)
            if (h.at(i, d) != 0) {
                diagonal = false;
                break;
            }
    if (diagonal) {
        // 1 x 1 blocks: selection of the K smallest diagonal entries, ties by index
        std::vector<int> order((size_t)N);
        for (int i = 0; i < N; ++i) order[(size_t)i] = i;
        for (int k = 0; k < K; ++k) {
            int best = k;
            for (int i = k + 1; i < N; ++i)
                if (h.at(order[(size_t)i], 0) < h.at(order[(size_t)best], 0) ||
                    (h.at(order[(size_t)i], 0) == h.at(order[(size_t)best], 0) && order[(size_t)i] < order[(size_t)best]))
                    best = i;
            const int t = order[(size_t)k];
            order[(size_t)k] = order[(size_t)best];
            order[(size_t)best] = t;
        }
        for (int k = 1; k < K; ++k)
            if (h.at(order[(size_t)k], 0) - h.at(order[(size_t)k - 1], 0) < close || h.norm == 0) {
                *why = "two levels are closer than 2^-20 ||H||";
                return QC_ESINGULAR;
            }
        for (int k = 0; k < K; ++k) {
            energies[k] = (double)h.at(order[(size_t)k], 0);
            for (int j = 0; j < N; ++j) vectors[(size_t)k * (size_t)N + (size_t)j] = j == order[(size_t)k] ? 1. : 0.;
        }
        return QC_OK;
    }

    const ld tiny = ldexpl(h.norm, -80);
    const ld bracket = ldexpl(h.norm, -40), done = ldexpl(h.norm, -58);
    std::vector<ld> work((size_t)N * (size_t)(kl + 1));
    std::vector<ld> V((size_t)K * (size_t)N), E((size_t)K), x((size_t)N), y((size_t)N);
    BandLU lu;
    const ld edge = h.norm + ldexpl(h.norm, -10);          // every eigenvalue lies inside (-edge, edge)
    ld floor_ = -edge;
    for (int k = 0; k < K; ++k) {
        // count(lo) <= k < count(hi)
        ld lo = floor_, hi = edge;
        while (hi - lo > bracket) {
            const ld mid = lo + (hi - lo) / 2;
            if (count_below(h, mid, tiny, work) <= k)
                lo = mid;
            else
                hi = mid;
        }
        floor_ = lo;                                       // level k + 1 is not below level k
        ld sigma = lo + (hi - lo) / 2, rho = sigma, res = h.norm;
        // the fixed start vector: a linear congruential sequence in [0.5, 1.5)
        uint32_t seed = 12345u + 977u * (uint32_t)k;
        for (int i = 0; i < N; ++i) {
            seed = seed * 1664525u + 1013904223u;
            x[(size_t)i] = (ld)0.5 + (ld)(seed >> 8) / (ld)(1u << 24);
        }
        bool ok = false;
        for (int it = 0; it < 16 && !ok; ++it) {
            lu.factor(h, sigma, tiny);
            lu.solve(x.data());
            // twice is enough: the second pass removes what the first one's rounding left
            for (int pass = 0; pass < 2; ++pass)
                for (int m = 0; m < k; ++m) {
                    const ld* vm = &V[(size_t)m * (size_t)N];
                    const ld c = dot(vm, x.data(), N);
                    for (int i = 0; i < N; ++i) x[(size_t)i] -= c * vm[i];
                }
            ld big = 0;
            for (int i = 0; i < N; ++i) big = fabsl(x[(size_t)i]) > big ? fabsl(x[(size_t)i]) : big;
            if (!(big > 0) || !(big <= LDBL_MAX)) break;
            for (int i = 0; i < N; ++i) x[(size_t)i] /= big;      // (keeps the squares below inside the range)
            const ld nrm = sqrtl(dot(x.data(), x.data(), N));
            for (int i = 0; i < N; ++i) x[(size_t)i] /= nrm;
            apply(h, x.data(), y.data());
            rho = dot(x.data(), y.data(), N);
            res = 0;
            for (int i = 0; i < N; ++i) {
                const ld r = fabsl(y[(size_t)i] - rho * x[(size_t)i]);
                res = r > res ? r : res;
            }
            if (!(rho >= lo - bracket && rho <= hi + bracket)) {
                if (it >= 2) break;                        // (the first solves from the start vector may still be off)
                continue;
            }
            ok = res <= done;
            sigma = rho;
        }
        if (!ok) {
            *why = "a level did not converge";
            return QC_ESINGULAR;
        }
        E[(size_t)k] = rho;
        for (int i = 0; i < N; ++i) V[(size_t)k * (size_t)N + (size_t)i] = x[(size_t)i];
        if (k > 0 && E[(size_t)k] - E[(size_t)k - 1] < close) {
            *why = "two levels are closer than 2^-20 ||H||";
            return QC_ESINGULAR;
        }
    }
    for (int k = 0; k < K; ++k) {
        energies[k] = (double)E[(size_t)k];
        double* v = vectors + (size_t)k * (size_t)N;
        double big = 0.;
        for (int j = 0; j < N; ++j) {
            v[j] = (double)V[(size_t)k * (size_t)N + (size_t)j];
            big = std::fabs(v[j]) > big ? std::fabs(v[j]) : big;
        }
        const double cut = std::ldexp(big, -26);
        int last = -1;
        for (int j = 0; j < N; ++j)
            if (std::fabs(v[j]) > cut) last = j;
        if (last >= 0 && v[last] < 0.)
            for (int j = 0; j < N; ++j) v[j] = 0. - v[j];      // (no -0.0)
    }
    return QC_OK;
}

}  // namespace levels
}  // namespace qcart
