// qcart_phase.hpp — the launchers of qcart_phase.hip (the phase-space view of density matrices), called by the entry
// points that own the handles: qc_wigner_eval_rho (qcart_wigner.hip) and qc_spatial_congruence (qcart_spatial.hip).
// Declarations only; the arguments are checked by the callers. Internal: not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace qcart {
namespace phase {

// W [M][X][P] of rho [M][X][X] complex128 with the qc_wigner handle's padded table T (row stride ldP); the error of the
// launch
hipError_t launch_wigner(const double* T, int32_t X, int32_t P, int32_t ldP, const void* rho, int32_t M, double* out,
                         hipStream_t stream);

// sigma [M][X][X] = scale Phi rho Phi^T of rho [M][n][n] complex128. phit [>= round_up(n, 4)][ldX] is the transposed
// table, phit[k * ldX + c] = Phi[c][k], zero for c in [X, ldX), ldX a multiple of 32 and >= X; zero: one complex zero;
// Z: room for M n X complex128. The error of the first launch that failed
hipError_t launch_congruence(const double* phit, int32_t ldX, const void* zero, int32_t X, int32_t n, const void* rho,
                             int32_t M, double scale, void* Z, void* sigma, hipStream_t stream);

}  // namespace phase
}  // namespace qcart
