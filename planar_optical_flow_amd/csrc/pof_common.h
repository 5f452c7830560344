// Shared device/host helpers for libpof_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pof_abi.h"

#define POF_WAVE 64

// hipGetLastError() reports (and clears) the last error of ANY earlier HIP call of this thread -- e.g. one
// raised by the caller's own previous launch.  Every entry point takes that state first, so that
// POF_CHECK_LAUNCH() only sees its own launches -- but it does not swallow it: the code is parked in a
// thread-local slot that the caller reads (and clears) with pof_take_stale_error().
extern thread_local int pof_stale_error_slot;
#define POF_CLEAR_STALE_ERROR()                                  \
    do {                                                         \
        const hipError_t stale_ = hipGetLastError();             \
        if (stale_ != hipSuccess) pof_stale_error_slot = (int)stale_; \
    } while (0)

#define POF_CHECK_LAUNCH()                                   \
    do {                                                     \
        if (hipGetLastError() != hipSuccess) return POF_E_LAUNCH; \
    } while (0)

static inline hipStream_t pof_stream(pof_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// The translation units are built with -ffp-contract=off: a*b+c is two
// roundings unless fma() is written out.  That is what makes the float64 index
// math of the cutout and the association distances bit-identical to NumPy.

// Correctly rounded x / c for a divisor known per launch; `rc` = RN(1/c).
// q0 = RN(x*rc) is within 1 ulp of x/c; the exact FMA residual and one FMA
// correction give RN(x/c) (Markstein).  Checked against '/' on 1.2e9 random
// operands for the divisors this library uses (tools/divconst_check.c).
__device__ __forceinline__ double pof_div_const(double x, double c, double rc)
{
    double q = x * rc;
    double r = fma(-q, c, x);
    return fma(r, rc, q);
}

// A4: one flow vector between the scanner frame and the canonical frame of a scan point whose angle has cosine c
// and sine s (src/utils/utils.py:62-105).  Evaluated in float64 and rounded to T once; to_canonical = 0 is
// canonical_to_global_flow.  pof_rotate_flow and pof_person_flow both go through here, so they agree bit for bit.
template <typename T>
__device__ __forceinline__ void pof_rotate_flow_point(double c, double s, T fx_in, T fy_in, int to_canonical,
                                                      T &ox, T &oy)
{
    const double fx = (double)fx_in, fy = (double)fy_in;
    double gx, gy;
    if (to_canonical) {
        gx = c * fx + (-s) * fy;
        gy = s * fx + c * fy;
    } else {
        gx = c * fx + s * fy;
        gy = (-s) * fx + c * fy;
    }
    ox = (T)gx;
    oy = (T)gy;
}

// The pose terms pof_person_flow reads, of sensor b at the pose (x, y, phi) that this step moved by (dx, dy):
// rot = R(phi) row-major in float, trans = (x, y), flow_trans = (dx, dy).  A null pointer is skipped.
// pof_pose_advance and the keyframe kernel both write them here.
__device__ __forceinline__ void pof_write_pose_terms(int b, double x, double y, double phi, double dx, double dy,
                                                     float *rot, double *trans, double *flow_trans)
{
    if (rot) {
        double s1, c1;
        sincos(phi, &s1, &c1);
        rot[4 * b] = (float)c1;
        rot[4 * b + 1] = (float)(-s1);
        rot[4 * b + 2] = (float)s1;
        rot[4 * b + 3] = (float)c1;
    }
    if (trans) {
        trans[2 * b] = x;
        trans[2 * b + 1] = y;
    }
    if (flow_trans) {
        flow_trans[2 * b] = dx;
        flow_trans[2 * b + 1] = dy;
    }
}

// Orders the LDS traffic of a workgroup of THREADS: what a thread wrote in front of it, every thread reads behind it.
// A workgroup of one wave needs no s_barrier for that: the hardware executes a wave's LDS operations in program
// order, so it is enough that the compiler neither moves them across this point (the two fences) nor lets the lanes
// of the wave drift apart around it (wave_barrier).  More than one wave meet in __syncthreads().
template <int THREADS>
__device__ __forceinline__ void pof_lds_order()
{
    if (THREADS == 64) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

__device__ __forceinline__ double wave_max_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum of K values over a workgroup of THREADS (64: one wave), the same bits in every thread: a butterfly stage adds
// the same two numbers in both lanes, and the wave totals go through LDS and every thread adds them in wave order.
// `part` is [K][THREADS / 64] doubles of LDS (unused by the one-wave form).
template <int THREADS, int K>
__device__ __forceinline__ void group_sum(double (&v)[K], double *part)
{
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum_f64(v[k]);
    if (THREADS > 64) {
        constexpr int kWaves = THREADS / 64;
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) part[k * kWaves + wave] = v[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double s = part[k * kWaves];
#pragma unroll
            for (int j = 1; j < kWaves; ++j) s += part[k * kWaves + j];
            v[k] = s;
        }
        __syncthreads();                                       // the next sum overwrites the partials
    }
}

__device__ __forceinline__ float wave_sum_f32(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float wave_max_f32(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Sum over the 64 lanes on the vector pipe only (no LDS-pipe shuffles): four row_shr adds inside each row of 16
// lanes, then row_bcast15 / row_bcast31 carry the row totals upwards.  The total is valid in LANE 63 only.
__device__ __forceinline__ float wave_sum_to_lane63_f32(float v)
{
#define POF_DPP_ADD(ctrl, rmask, bctl) \
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, rmask, 0xF, bctl))
    POF_DPP_ADD(0x111, 0xF, true);    // row_shr:1
    POF_DPP_ADD(0x112, 0xF, true);    // row_shr:2
    POF_DPP_ADD(0x114, 0xF, true);    // row_shr:4
    POF_DPP_ADD(0x118, 0xF, true);    // row_shr:8   -> lane 15 of every row holds the row's sum
    POF_DPP_ADD(0x142, 0xA, false);   // row_bcast15 into rows 1 and 3
    POF_DPP_ADD(0x143, 0xC, false);   // row_bcast31 into rows 2 and 3 -> lane 63 holds the wave's sum
#undef POF_DPP_ADD
    return v;
}
