// qcart_spatial.hpp — the table behind the position-space view of Fock states (qc_spatial, include/qcart.h), written
// once for the library (qcart_spatial.hip fills the device table from it) and for plain C++ programs
// (tests/diag/spatial_check.cpp): E[j][n] = psi_n(x_j), the normalised harmonic-oscillator eigenfunctions in the
// drivers' units (hbar = m = omega = 1; HO/main_parallel.py:82-86, the exp(-x^2 / 2) of
// common_factor_of_1Dharmonics), by the three-term recurrence in long double, each entry rounded once to fp64. The
// upward recurrence is the stable direction inside and outside the classical region. No HIP type appears here.
// Internal: not part of the C ABI.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/qcart.h"

namespace qcart {
namespace spatial {

#if !defined(__HIP_DEVICE_COMPILE__)   // (host code only: the device pass of a HIP compile has no extended type)
static_assert(LDBL_MANT_DIG >= 64, "the table is computed in an extended long double and rounded once to fp64");
#endif

constexpr int32_t kMaxLevels = 2048;
constexpr int32_t kMaxPoints = 4096;
constexpr double kMaxAbsX = 128.;   // exp(-x^2 / 2) stays a normal long double

// the first refusal of the arguments, or nullptr
inline const char* bad_table(int32_t n_levels, const double* x, int32_t x_n) {
    if (n_levels < 1 || n_levels > kMaxLevels) return "n_levels must be in [1, 2048]";
    if (x_n < 1 || x_n > kMaxPoints) return "x_n must be in [1, 4096]";
    if (!x) return "x is NULL";
    for (int32_t j = 0; j < x_n; ++j)
        if (!std::isfinite(x[j]) || std::fabs(x[j]) > kMaxAbsX) return "every x must be finite with |x| <= 128";
    return nullptr;
}

// out[j * n_levels + n] = psi_n(x[j]); QC_EINVAL with *why set (if given) when bad_table refuses, out untouched
inline int qc_spatial_build_table(int32_t n_levels, const double* x, int32_t x_n, double* out,
                                  const char** why = nullptr) {
    const char* bad = out ? bad_table(n_levels, x, x_n) : "out is NULL";
    if (why) *why = bad;
    if (bad) return QC_EINVAL;
    const long double pi = 3.14159265358979323846264338327950288L;
    const long double c0 = 1.0L / sqrtl(sqrtl(pi));   // pi^(-1/4)
    const long double r2 = sqrtl(2.0L);
    for (int32_t j = 0; j < x_n; ++j) {
        const long double xj = (long double)x[j];
        double* row = out + (size_t)j * (size_t)n_levels;
        long double prev = c0 * expl(-0.5L * xj * xj);   // psi_0
        row[0] = (double)prev;
        if (n_levels == 1) continue;
        long double cur = r2 * xj * prev;                // psi_1
        row[1] = (double)cur;
        for (int32_t n = 1; n + 1 < n_levels; ++n) {
            const long double np1 = (long double)(n + 1);
            const long double next = sqrtl(2.0L / np1) * xj * cur - sqrtl((long double)n / np1) * prev;
            prev = cur;
            cur = next;
            row[n + 1] = (double)cur;
        }
    }
    return QC_OK;
}

}  // namespace spatial
}  // namespace qcart
