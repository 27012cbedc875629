// qcart_filter.hpp — the conditional master equation (qc_lindblad_evolve_conditional, include/qcart.h): the host side
// (argument checks, the step's two constants, the host mirror of the two Philox draws of a step), written once for the
// library (qcart_lindblad.hip) and for plain C++ programs (tests/diag/filter_check.cpp), and, for HIP translation
// units only, the launchers of qcart_filter.hip. No HIP type appears in the host part. Internal: not part of the C ABI.
#pragma once
#include <cmath>
#include <cstdint>

#include "qcart_lindblad.hpp"

namespace qcart {
namespace filter {

using lindblad::ld;

// The Philox tags of a conditional step: counter (step_lo, step_hi, stream id, tag)
constexpr uint32_t kTagPick = 0x500;                   // u: which eigenvalue of X the outcome is centred on
constexpr uint32_t kTagNoise = 0x501;                  // z: the outcome's Gaussian noise (normals' r0)

// the first refusal, or nullptr
inline const char* bad_efficiency(double eta, double gamma) {
    if (!std::isfinite(eta) || !(eta > 0.) || !(eta <= 1.)) return "eta must be in (0, 1]";
    if (!(gamma > 0.)) return "gamma must be > 0 for a conditional evolution (nothing is measured)";
    return nullptr;
}
inline const char* bad_conditional(const void* rho, int32_t M, int32_t N, const void* slots, int32_t default_slot,
                                   int32_t J, int32_t n_steps, double eta, int64_t first_step, const void* draws,
                                   const void* record_in) {
    if (const char* bad = lindblad::bad_evolve(rho, M, N, slots, default_slot, J, n_steps)) return bad;
    if (first_step < 0 || first_step > INT64_MAX - (int64_t)n_steps) return "first_step must be >= 0";
    if (draws && record_in) return "record_in and draws exclude each other";
    if (!(eta > 0.)) return "the efficiency is not set (qc_lindblad_set_efficiency first)";
    return nullptr;
}

// a = eta gamma dt / 2 and s = 1 / sqrt(4 a), each formed in long double and rounded once
inline void constants(double eta, double gamma, double dt, double* a, double* s) {
    const ld al = (ld)eta * (ld)gamma * (ld)dt / 2;
    *a = (double)al;
    *s = (double)(1 / sqrtl(4 * al));
}

// G^(1-eta) [N][N]: lindblad::gauss's full table with gamma (1 - eta) formed in long double (the dephasing the record
// does not account for)
inline void efficiency_table(int32_t N, const ld* xi, double dt, double gamma, double eta, double* g) {
    lindblad::gauss(N, xi, (ld)dt, (ld)gamma * ((ld)1 - (ld)eta), nullptr, g);
}

// ---- the host mirror of the device's draws (qcart_kernels.hpp's philox10, log_unit, sincospi_unit and normals restated
// operation by operation; the device contracts a * b + c where one expression writes it, so the normals agree within
// rounding, < 1e-15, not by bit pattern; u is exact)
inline void philox10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t lo0 = (uint32_t)p0, hi0 = (uint32_t)(p0 >> 32), lo1 = (uint32_t)p1, hi1 = (uint32_t)(p1 >> 32);
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
    }
}
inline void block(uint64_t seed, uint32_t stream, uint64_t step, uint32_t tag, uint32_t c[4]) {
    c[0] = (uint32_t)step;
    c[1] = (uint32_t)(step >> 32);
    c[2] = stream;
    c[3] = tag;
    philox10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}
inline double unit(uint32_t hi, uint32_t lo) {
    return ((double)(((((uint64_t)hi) << 32) | lo) >> 11) + 0.5) * 0x1.0p-53;
}
inline double log_unit(double x) {
    int k;
    double m = std::frexp(x, &k);
    if (m < 0.70710678118654752440) {
        m += m;
        k -= 1;
    }
    const double f = m - 1.0;
    const double s = f / (2.0 + f), z = s * s, w = z * z;
    const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01));
    const double t2 = z * (6.666666666666735130e-01 +
                           w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)));
    const double Rr = t2 + t1, hfsq = 0.5 * f * f, dk = (double)k;
    return dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + Rr) + dk * 1.90821492927058770002e-10)) - f);
}
inline double cospi_unit(double t) {
    const double n = std::rint(2.0 * t);
    const double r = std::fma(-0.5, n, t);
    const double x = r * 3.141592653589793, z = x * x;
    double ps = 2.8114572543455206e-15;
    ps = std::fma(ps, z, -7.647163731819816e-13);
    ps = std::fma(ps, z, 1.6059043836821613e-10);
    ps = std::fma(ps, z, -2.505210838544172e-08);
    ps = std::fma(ps, z, 2.7557319223985893e-06);
    ps = std::fma(ps, z, -0.0001984126984126984);
    ps = std::fma(ps, z, 0.008333333333333333);
    ps = std::fma(ps, z, -0.16666666666666666);
    const double S = std::fma(x * z, ps, x);
    double pc = -1.5619206968586225e-16;
    pc = std::fma(pc, z, 4.779477332387385e-14);
    pc = std::fma(pc, z, -1.1470745597729725e-11);
    pc = std::fma(pc, z, 2.08767569878681e-09);
    pc = std::fma(pc, z, -2.755731922398589e-07);
    pc = std::fma(pc, z, 2.48015873015873e-05);
    pc = std::fma(pc, z, -0.001388888888888889);
    pc = std::fma(pc, z, 0.041666666666666664);
    const double C = std::fma(z * z, pc, std::fma(-0.5, z, 1.0));
    const int q = (int)n & 3;
    return q == 0 ? C : (q == 1 ? -S : (q == 2 ? -C : S));
}
// (u, z) of step `step` of stream `stream`: u from the first two words of the block at kTagPick, z = normals' r0 of the
// block at kTagNoise
inline void draws(uint64_t seed, uint32_t stream, uint64_t step, double* u, double* z) {
    uint32_t c[4];
    block(seed, stream, step, kTagPick, c);
    *u = unit(c[0], c[1]);
    block(seed, stream, step, kTagNoise, c);
    const double u1 = unit(c[0], c[1]), u2 = unit(c[2], c[3]);
    *z = std::sqrt(-2.0 * log_unit(u1)) * cospi_unit(2.0 * u2);
}

}  // namespace filter
}  // namespace qcart

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace qcart {
namespace filter {

// What one call's launches share. All pointers are device pointers; the arguments were checked by the caller.
struct Call {
    void* sigma;               // [M][N][N] complex128, in place
    const double* xi;          // [N]
    int32_t N, M, J;
    const int32_t* slots;      // [M] or null: the caller's
    int32_t default_slot;
    int32_t* eff;              // [M]: the slot the congruences of this call read; -1 from the moment a matrix is dead
    int32_t* status;           // [M]: 0 alive, 1 dead
    int32_t* flags;            // [2]: [0] a slot out of range, [1] a matrix that could not be stepped
    double* v;                 // [M][N]
    double a, s;               // eta gamma dt / 2, 1 / sqrt(4 a)
    uint64_t seed;
    const int32_t* streams;    // [M] or null: stream id m
    hipStream_t stream;
};

// eff and status of a new call; raises flags[0] for a slot outside [0, J)
hipError_t launch_begin(const Call& c);
// one step's outcome and v: draws (u, z) [M][2] or null, record_in [M] or null (both null: Philox at `step`),
// record_out [M] or null, all of this step
hipError_t launch_draw(const Call& c, uint64_t step, const double* draws, const double* record_in, double* record_out);
// sigma_ij <- (v_i v_j) sigma_ij of every live matrix
hipError_t launch_apply(const Call& c);
// rho_m <- backup_m for every matrix whose status is not 0 (one whose slot was out of range was never written: the
// same bytes)
hipError_t launch_restore(const Call& c, const void* backup);

}  // namespace filter
}  // namespace qcart
#endif
