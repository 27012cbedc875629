// qcart_wigner_tiles.hpp — the tiling of the Wigner contraction, shared by the kernels that run it: k_wigner /
// k_wigner_mean (qcart_wigner.hip, wavefunctions) and k_phase_wigner (qcart_phase.hip, density matrices). A workgroup
// is one wave that owns a quad of position tiles (16 positions each) and kTP momenta: with T = ceil(x_n / 16) tiles,
// pair u = tiles (u, T - 1 - u), U = ceil(T / 2) pairs, quad v = pairs (v, U - 1 - v). Both kernels read the same
// padded table, so the shape of a step and of a launch is written once. HIP only. Internal: not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace qcart {
namespace wigner {

constexpr int kNT = 4;                 // column tiles per workgroup
constexpr int kTP = 16 * kNT;          // momenta per workgroup
constexpr int kStep = 4;               // lags per MFMA

// the largest K_i = min(i, X - 1 - i) of the rows i0 .. min(i0 + 15, X - 1)
__device__ __forceinline__ int tile_kmax(int i0, int X) {
    const int n1 = X - 1, i1 = i0 + 15 < n1 ? i0 + 15 : n1, mid = n1 / 2;
    const int a = i0 < n1 - i0 ? i0 : n1 - i0, b = i1 < n1 - i1 ? i1 : n1 - i1;
    const int m = a > b ? a : b;
    return i0 <= mid && mid <= i1 ? mid : m;
}

// the launch: the quads of position tiles and the groups of kTP momenta
inline unsigned tile_quads(int32_t X) { return (unsigned)((((X + 15) / 16 + 1) / 2 + 1) / 2); }
inline unsigned momentum_groups(int32_t P) { return (unsigned)((P + kTP - 1) / kTP); }

}  // namespace wigner
}  // namespace qcart
