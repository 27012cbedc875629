// qcart_ensemble.hpp — the order and the argument checks behind the ensemble density matrix (qc_ensemble,
// include/qcart.h), written once for the library (qcart_ensemble.hip) and for plain C++ programs
// (tests/diag/ensemble_check.cpp). The order of the sum over the envs is a function of (B, N) alone: chunks of
// kChunk consecutive envs, S = splits(B, N) splits, split s owning the chunks s, s + S, s + 2 S, ..; the splits'
// partial sums ([S][2][N][N] doubles: Re and Im planes) fit a buffer of at most kPartialCap doubles (64 MiB) that the
// handle makes at create time for the largest S. No HIP type appears here. Internal: not part of the C ABI.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/qcart.h"

namespace qcart {
namespace ensemble {

constexpr int32_t kMaxN = 2048;
constexpr int32_t kChunk = 2;                          // envs per MFMA step: K = 4 = 2 envs x (re, im)
constexpr int32_t kMaxSplits = 256;
constexpr size_t kPartialCap = (size_t)1 << 23;        // doubles: 64 MiB
constexpr int32_t kMaxB = INT32_MAX - kChunk;          // (a chunk's padding stays inside int32)

// envs per chunk (0 for N out of range)
inline int32_t chunk(int32_t N) { return N >= 1 && N <= kMaxN ? kChunk : 0; }

// the chunks of B envs
inline int64_t chunks(int32_t B) { return ((int64_t)B + kChunk - 1) / kChunk; }

// S = min(ceil(B / E), 256, max(1, floor(2^22 / N^2))); 0 for arguments out of range
inline int32_t splits(int32_t B, int32_t N) {
    if (B < 1 || B > kMaxB || N < 1 || N > kMaxN) return 0;
    const int64_t fit = (int64_t)(kPartialCap / 2) / ((int64_t)N * (int64_t)N);
    int64_t s = chunks(B);
    if (s > kMaxSplits) s = kMaxSplits;
    if (s > fit) s = fit;
    return s < 1 ? 1 : (int32_t)s;
}

// the largest S any B can ask for, and the doubles of the partials' buffer made for it
inline int32_t max_splits(int32_t N) { return splits(kMaxB, N); }
inline size_t partial_doubles(int32_t N) { return (size_t)max_splits(N) * 2 * (size_t)N * (size_t)N; }

// the split that owns chunk c
inline int32_t split_of_chunk(int64_t c, int32_t S) { return (int32_t)(c % S); }

// the first refusal of the create arguments, or nullptr
inline const char* bad_create(int32_t N, double scale) {
    if (N < 1 || N > kMaxN) return "N must be in [1, 2048]";
    if (!std::isfinite(scale) || !(scale > 0.)) return "scale must be finite and > 0";
    return nullptr;
}

// the first refusal of a call's arguments, or nullptr
inline const char* bad_call(const void* psi, int32_t B, const void* rho) {
    if (!psi || !rho) return "psi and rho are required";
    if (B < 1 || B > kMaxB) return "B must be >= 1";
    return nullptr;
}

}  // namespace ensemble
}  // namespace qcart
