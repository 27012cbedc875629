// qcart_expt.hpp — diagnostic hooks of the step kernel, compiled out of the shipped library.
//
// -DQCART_STAMPS (a diagnostic build only, tools/diag_stamps.py): per-phase cycle shares of the step loop
// (s_memtime at each QC_STAMP(phase) site of qcart_kernels.hpp), summed over all waves into qc_stamps[] and
// read back by qc_debug_stamps. -DQCART_BSTAMPS (tools/diag_boundaries.py): four stamps per wave around the loop, for
// the cost of a workgroup boundary. Without either every hook below expands to nothing.
//
// Experiment knobs: compile-time defaults of the shipped build that an experiment build (make expt / expt_actor
// EXPT=-D...) overrides for an A/B. Each default is the measured winner.
#pragma once
#include <hip/hip_runtime.h>

// step kernel: the largest rows-per-lane R (fp64-equivalent) that runs 8-wave workgroups (two waves per SIMD),
// Fock families / grid
#ifndef QCART_W8_MAX_R
#define QCART_W8_MAX_R 8
#endif
#ifndef QCART_W8_MAX_RG
#define QCART_W8_MAX_RG 9
#endif
// grid step kernels up to R = 9: the host-folded step constants of the Fock kernels (HC; round 6, alternating
// same-call pairs: C4 9.09 -> 8.91 ms; C3's R = 17 kernel with them, 150.2 -> 149.0 ms, computed wrong values, k_step
// comment). QCART_GRID_KAR: the per-step kernarg re-read for R = 17 too (A/B knob; with HC: C3's spilled SGPRs
// 260 -> 109, 151.2 vs 149.8 ms against the shipped kernel)
#ifndef QCART_GRID_HC
#define QCART_GRID_HC 1
#endif
#ifndef QCART_GRID_KAR
#define QCART_GRID_KAR 0
#endif
// band solve: the fp32 Fock kernels' whole-wave Kogge-Stone (no row carry) for up to this many kept levels (0: off;
// 3: C5 -1.6 %)
#ifndef QCART_WKS_F32
#define QCART_WKS_F32 3
#endif
// step kernel: the fp32 R = 32 kernel's Y+- means in two reductions (1; C5 46.7 -> 43.2 ms) or one (0)
#ifndef QCART_SPLITM
#define QCART_SPLITM 1
#endif
// step kernel: the 64-step noise refill parked in a 1 KiB per-wave LDS buffer, read back one step at a time (1), or
// held in 4 VGPRs across the step loop (0) — fp64 kernels with LDS tables (MODE >= 1)
#ifndef QCART_NZ_LDS
#define QCART_NZ_LDS 1
#endif
// step kernel, 8-wave fp64 Fock workgroups with LDS tables: the two waves of a SIMD balanced by progress — each
// publishes its step index in LDS and the one behind issues at s_setprio 1 (kPairBalance, qcart_kernels.hpp; 0: the
// hardware's older-first arbitration. Metric, four alternating same-call pairs: 23.64 -> 22.74 ms per launch,
// profiles/r07_pair_balance_ab.txt), for kernels of at least QCART_PAIR_BALANCE_MIN_R rows per lane (8: IHO N = 512,
// the measured shape, and HO N = 512; smaller R not measured)
#ifndef QCART_PAIR_BALANCE
#define QCART_PAIR_BALANCE 1
#endif
#ifndef QCART_PAIR_BALANCE_MIN_R
#define QCART_PAIR_BALANCE_MIN_R 8
#endif
// measurement actor (qcart_actor.hip): conv1..3 column tiles per wave, accumulator sets, k-steps per load batch;
// fc1 output tiles x env tiles per wave
#ifndef QCART_MCONV_NT
#define QCART_MCONV_NT 2, 2, 1
#endif
#ifndef QCART_MCONV_NA
#define QCART_MCONV_NA 2, 1, 2
#endif
#ifndef QCART_MCONV_Q
#define QCART_MCONV_Q 4, 4, 4
#endif
#ifndef QCART_MFC_MT
#define QCART_MFC_MT 2
#endif
#ifndef QCART_MFC_NT
#define QCART_MFC_NT 2
#endif
// DQN actor / learner, inputs above 512 floats (qcart_dqn.hpp, stage_chunk): X0's chunks staged with lanes along the
// column index (0) or along k in runs of 8 (1; L = 1002, three alternating pairs: actor round 2.320 -> 2.312 ms,
// learner update 0.820 -> 0.815 ms, profiles/dqn_wavefunction_ab.json)
#ifndef QCART_FC1_STAGE_K
#define QCART_FC1_STAGE_K 1
#endif

#ifdef QCART_STAMPS
namespace qcart {
__device__ unsigned long long qc_stamps[20];
}
#define QC_STAMP(ph)                                                                                 \
    do {                                                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                           \
        unsigned long long t_;                                                                       \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                   \
        __builtin_amdgcn_sched_barrier(0);                                                           \
        st_acc[st_ph] += t_ - st_t;                                                                  \
        st_t = t_;                                                                                   \
        st_ph = (ph);                                                                                \
    } while (0)
// the step kernel's stamp state, declared before its loop and flushed after it
#define QC_STAMP_BEGIN()                                                                             \
    unsigned long long st_acc[16] = {0}, st_t = 0;                                                   \
    int st_ph = 9;                                                                                   \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_t)::"memory");                     \
    const unsigned long long st_loop0 = st_t
// wave entry (k_step) and exit (after the write-back): slots 16 (entry -> loop), 17 (loop end -> exit),
// 18 (wave count)
#define QC_KSTAMP_ENTRY()                                                                            \
    unsigned long long kst_t0;                                                                       \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(kst_t0)::"memory")
#define QC_KSTAMP_EXIT(lane)                                                                         \
    do {                                                                                             \
        unsigned long long t_;                                                                       \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                   \
        if ((lane) == 0) {                                                                           \
            atomicAdd(&qc_stamps[16], st_loop0 - kst_t0);                                            \
            atomicAdd(&qc_stamps[17], t_ - st_t);                                                    \
            atomicAdd(&qc_stamps[18], 1ull);                                                         \
        }                                                                                            \
    } while (0)
#define QC_STAMP_END(lane)                                                                           \
    do {                                                                                             \
        QC_STAMP(9);                                                                                 \
        if ((lane) == 0)                                                                             \
            for (int i_ = 0; i_ < 16; ++i_) atomicAdd(&qc_stamps[i_], st_acc[i_]);                   \
    } while (0)
// the band solve's stamps use the caller's state
#define QC_SOLVE_STAMP_ARGS , unsigned long long (&st_acc)[16], unsigned long long& st_t, int& st_ph
#define QC_SOLVE_STAMP_PASS , st_acc, st_t, st_ph

// read and clear the per-phase cycle sums (weak: an experiment build stamps one family TU)
extern "C" __attribute__((weak)) int qc_debug_stamps(unsigned long long* out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(qcart::qc_stamps), sizeof(unsigned long long) * 20) != hipSuccess) return -1;
    unsigned long long z[20] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(qcart::qc_stamps), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#elif defined(QCART_BSTAMPS)
// -DQCART_BSTAMPS (a diagnostic build only, tools/diag_boundaries.py): the cost of a workgroup boundary. Every wave
// that runs a tile reads s_memtime at kernel (tile) entry, loop begin, loop end and exit, and lane 0 writes the four
// values and the wave's hardware id (HW_ID: CU / SH / SE, and XCC_ID) with plain vector stores into the wave's own
// record of qc_bstamps — no atomics, nothing shared between waves. Record of tile t's wave w: (t * W + w) * 8 words
// (tile: the workgroup's place in the launch, the a.n_mixed two-slot tiles first). qc_debug_bstamps copies the
// records out and clears them.
namespace qcart {
constexpr unsigned kBStampWaves = 1u << 17;
__device__ unsigned long long qc_bstamps[kBStampWaves * 8];
}
#define QC_STAMP(ph) \
    do {             \
    } while (0)
#define QC_BSTAMP_READ(t_) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory")
#define QC_KSTAMP_ENTRY()        \
    unsigned long long bst_t0;   \
    QC_BSTAMP_READ(bst_t0)
#define QC_STAMP_BEGIN()         \
    unsigned long long bst_t1;   \
    QC_BSTAMP_READ(bst_t1)
#define QC_STAMP_END(lane)       \
    unsigned long long bst_t2;   \
    QC_BSTAMP_READ(bst_t2)
// (blk, a, ei, MODE and W are step_body's: the tile index counts the a.n_mixed two-slot tiles first)
#define QC_KSTAMP_EXIT(lane)                                                                         \
    do {                                                                                             \
        unsigned long long t_;                                                                       \
        QC_BSTAMP_READ(t_);                                                                          \
        const unsigned w_ = ((MODE == 3 ? 0u : a.n_mixed) + (unsigned)(blk)) * (unsigned)W + (unsigned)ei; \
        if ((lane) == 0 && w_ < kBStampWaves) {                                                      \
            const unsigned hw_ = __builtin_amdgcn_s_getreg(4 | (31 << 11));   /* HW_ID[31:0] */      \
            const unsigned xc_ = __builtin_amdgcn_s_getreg(20 | (3 << 11));   /* XCC_ID[3:0] */      \
            unsigned long long* p_ = qc_bstamps + (size_t)w_ * 8;                                    \
            p_[0] = bst_t0;                                                                          \
            p_[1] = bst_t1;                                                                          \
            p_[2] = bst_t2;                                                                          \
            p_[3] = t_;                                                                              \
            p_[4] = ((unsigned long long)xc_ << 32) | hw_;                                           \
            p_[5] = blockIdx.x;                                                                      \
        }                                                                                            \
    } while (0)
#define QC_SOLVE_STAMP_ARGS
#define QC_SOLVE_STAMP_PASS
// copy the first n_waves records out (8 words each) and clear them (weak: an experiment build stamps one family TU)
extern "C" __attribute__((weak)) int qc_debug_bstamps(unsigned long long* out, unsigned n_waves) {
    if (n_waves > qcart::kBStampWaves) return -1;
    const size_t bytes = sizeof(unsigned long long) * 8 * (size_t)n_waves;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(qcart::qc_bstamps), bytes) != hipSuccess) return -1;
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(qcart::qc_bstamps)) != hipSuccess) return -1;
    return hipMemset(p, 0, bytes) == hipSuccess ? 0 : -1;
}
#else
#define QC_STAMP(ph) \
    do {             \
    } while (0)
#define QC_STAMP_BEGIN() \
    do {                 \
    } while (0)
#define QC_STAMP_END(lane) \
    do {                   \
    } while (0)
#define QC_KSTAMP_ENTRY() \
    do {                  \
    } while (0)
#define QC_KSTAMP_EXIT(lane) \
    do {                     \
    } while (0)
#define QC_SOLVE_STAMP_ARGS
#define QC_SOLVE_STAMP_PASS
#endif

// the fp32 R = 32 kernel's mirror bands read in pipelined half-band batches (k_step MPIPE; A/B)
#ifndef QCART_MPIPE
#define QCART_MPIPE 1
#endif
#ifndef QCART_MPIPE_ROWS
#define QCART_MPIPE_ROWS 16
#endif
#ifndef QCART_MPIPE_DEPTH
#define QCART_MPIPE_DEPTH 2
#endif

// -DQCART_RES_STAMPS (a diagnostic build only, tools/probe_resident_lat.py --stamps): the resident kernel sums, per
// slot, the s_memrealtime ticks (10 ns) of its request phases — acquire, the pair, the step, the results + release —
// into the slot's err bytes (unused by the resident path) as 5 uint64: count, then the four sums
#ifndef QCART_RES_STAMPS
#define QCART_RES_STAMPS 0
#endif
