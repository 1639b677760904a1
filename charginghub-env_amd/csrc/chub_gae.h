// chub_gae.h -- generalised advantage estimation, stated once.  For the host (chub_runtime.cpp): the launch arguments of chub_gae.hip's
// kernels.  For the kernels of chub_gae.hip, chub_lagrange.hip and chub_retnorm.hip: one step of the recurrence, the (reward, done) pair
// of a packed row, the fixed LDS tree over a workgroup's f64 words and the fold of the workgroups' partials.  Every user is built with
// -ffp-contract=off; where an operation's rounding is part of the definition it is written as the _rn intrinsic.
#ifndef CHUB_GAE_H
#define CHUB_GAE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace chub {

constexpr int kGaeLanes = 256;  // a workgroup: one lane per env
constexpr int kGaeAhead = 8;    // steps whose loads are in flight before the serial chain consumes them

// chub_rollout_gae_device and chub_return_norm_gae_device (include/chub.h)
struct GaeArgs {
    int64_t n_envs, T;
    int32_t D;                    // reward at column D, done at D + 1 of a packed row of D + 2
    float gamma, gl;              // gl = gamma * lambda, formed once in f32
    const float *packed;          // [T][N][D + 2]
    const float *values;          // [T + 1][N]
    const float *final_values;    // [N] or null
    const uint8_t *mask;          // [N] or null
    float *adv, *ret;             // [T][N]; ret may be null
    double *partials;             // [blocks][3] or null: count, sum, sum of squares per workgroup
    double *stats;                // [3] or null
    const float *scale;           // [1], read inside the kernel, or null: rewards as they are (clip is not read)
    float clip;                   // bounds a scaled reward to [-clip, clip]; 0: no bound
};
void launch_gae(const GaeArgs &a, hipStream_t stream);

#if defined(__HIPCC__)
// reward and done: the last two floats of a packed row as one 8-byte load (4-byte aligned: a row is D + 2 floats)
struct __attribute__((packed, aligned(4))) GaeRewardDone {
    float r, d;
};

// one step of the recurrence, t descending: from the step's reward, done and value and the running (v_next, adv) to the step's advantage
// and return adv + v; the caller keeps them and makes v its next v_next.  Every operation is rounded once: a numpy f32 restatement gives
// the same bits.  S, the type of fin, v_next and adv, is float where they are a lane's scalars (k_gae) and const float * where they are
// elements of per-constraint arrays (k_cost_gae), which are then read inside the select that wants them, as the caller's own statement
// would read them: only so both callers compile to the code they had with the recurrence written out
struct GaeStep {
    float adv, ret;
};
__device__ __forceinline__ float gae_operand(float x) { return x; }
__device__ __forceinline__ float gae_operand(const float *x) { return *x; }

template <class S>
__device__ __forceinline__ GaeStep gae_step(float r, bool done, float v, S fin, float gamma, float gl, S v_next, S adv) {
    const float vn = done ? gae_operand(fin) : gae_operand(v_next);
    const float delta = __fsub_rn(__fadd_rn(r, __fmul_rn(gamma, vn)), v);
    GaeStep s;
    s.adv = __fadd_rn(delta, __fmul_rn(gl, done ? 0.0f : gae_operand(adv)));
    s.ret = __fadd_rn(s.adv, v);
    return s;
}

// the sums of a workgroup's LANES lanes in a fixed LDS tree: lane l takes lane l + h, h = LANES / 2 .. 1; every lane leaves with the sums.
// A caller that writes red again places its own barrier first
template <int WORDS, int LANES>
__device__ __forceinline__ void block_sum(double (*red)[LANES], int tid, double (&w)[WORDS]) {
#pragma unroll
    for (int i = 0; i < WORDS; i++) red[i][tid] = w[i];
    __syncthreads();
    for (int h = LANES / 2; h > 0; h >>= 1) {
        if (tid < h) {
#pragma unroll
            for (int i = 0; i < WORDS; i++) red[i][tid] += red[i][tid + h];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < WORDS; i++) w[i] = red[i][0];
}

// the workgroups' partials in ONE workgroup: lane l takes rows l, l + LANES, .. in ascending order (row b's WORDS words lie at
// rows + b * stride), then the tree
template <int WORDS, int LANES>
__device__ __forceinline__ void partials_sum(double (*red)[LANES], int tid, const double *rows, int64_t n_rows, int64_t stride, double (&w)[WORDS]) {
#pragma unroll
    for (int i = 0; i < WORDS; i++) w[i] = 0.0;
    for (int64_t b = tid; b < n_rows; b += LANES) {
        const double *p = rows + b * stride;
#pragma unroll
        for (int i = 0; i < WORDS; i++) w[i] += p[i];
    }
    block_sum(red, tid, w);
}
#endif

}  // namespace chub
#endif
