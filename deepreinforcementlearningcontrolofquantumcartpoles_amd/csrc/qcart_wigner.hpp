// qcart_wigner.hpp — the table behind the phase-space view (qc_wigner, include/qcart.h), written once for the library
// (qcart_wigner.hip fills the device table from it) and for plain C++ programs (tests/diag/wigner_check.cpp):
// T[k][j] = (cos, sin)(2 p_j h k) for k = 1 .. (x_n - 1) / 2, the phases of the Wigner transform's lag sum on a uniform
// grid of spacing h. The angle a = 2 p_j h k is formed in long double from the given doubles (two roundings of 2^-64
// relative: |a_ld - a| <= 2^-63 |a|), cosl / sinl are taken of it and the result is rounded once to fp64, so an entry
// lies within 2^-53 + 2^-62 |a| of the cos / sin of the exact real a. No HIP type appears here. Internal: not part of
// the C ABI.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/qcart.h"

namespace qcart {
namespace wigner {

#if !defined(__HIP_DEVICE_COMPILE__)   // (host code only: the device pass of a HIP compile has no extended type)
static_assert(LDBL_MANT_DIG >= 64, "the table is computed in an extended long double and rounded once to fp64");
#endif

constexpr int32_t kMaxPoints = 4096;
constexpr int32_t kMaxMomenta = 1024;

// the lags of the longest row: k = 1 .. table_rows(x_n)
inline int32_t table_rows(int32_t x_n) { return (x_n - 1) / 2; }

// the first refusal of the arguments, or nullptr
inline const char* bad_wigner(int32_t x_n, double h, const double* p, int32_t P) {
    if (x_n < 1 || x_n > kMaxPoints) return "x_n must be in [1, 4096]";
    if (!std::isfinite(h) || !(h > 0.)) return "h must be finite and > 0";
    if (P < 1 || P > kMaxMomenta) return "P must be in [1, 1024]";
    if (!p) return "p is NULL";
    const long double pi = 3.14159265358979323846264338327950288L;
    for (int32_t j = 0; j < P; ++j)
        if (!std::isfinite(p[j]) || !(fabsl((long double)p[j] * (long double)h) <= pi))
            return "every p must be finite with |p| h <= pi";
    return nullptr;
}

// out[((k - 1) * P + j) * 2 + {0, 1}] = {cos, sin}(2 p[j] h k), k = 1 .. table_rows(x_n); QC_EINVAL with *why set (if
// given) when bad_wigner refuses, out untouched
inline int qc_wigner_build_table(int32_t x_n, double h, const double* p, int32_t P, double* out,
                                 const char** why = nullptr) {
    const char* bad = out ? bad_wigner(x_n, h, p, P) : "out is NULL";
    if (why) *why = bad;
    if (bad) return QC_EINVAL;
    const int32_t rows = table_rows(x_n);
    for (int32_t j = 0; j < P; ++j) {
        const long double a1 = 2.0L * (long double)p[j] * (long double)h;
        for (int32_t k = 1; k <= rows; ++k) {
            const long double a = a1 * (long double)k;
            double* at = out + ((size_t)(k - 1) * (size_t)P + (size_t)j) * 2;
            at[0] = (double)cosl(a);
            at[1] = (double)sinl(a);
        }
    }
    return QC_OK;
}

}  // namespace wigner
}  // namespace qcart
