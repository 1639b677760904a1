// chub_retnorm.h -- what the reward scaling's kernels (chub_retnorm.hip) and the host (chub_runtime.cpp) share: the launch arguments of
// include/chub.h's section "reward scaling on the device" and the merge of a call's sums into the running state with the scale that
// follows from it, which the merge kernel and the host form (chub_return_norm_fold) both run.  Every f64 operation below is one rounded
// operation (-ffp-contract=off); division and square root are IEEE on both sides.
#ifndef CHUB_RETNORM_H
#define CHUB_RETNORM_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#if !defined(__HIP_DEVICE_COMPILE__)
#include <cmath>
#endif

namespace chub {

constexpr int kRetLanes = 256;  // a workgroup of every kernel of the unit
constexpr int kRetAhead = 8;    // steps of k_return_moments whose loads are in flight before the serial chain consumes them
constexpr int kRetStreamBlocks = 1024;  // the reset kernels' grid cap: a lane takes entries i, i + 1024 * 256, ..

__host__ __device__ inline double retnorm_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}

__host__ __device__ inline double retnorm_sqrt(double a) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(a);
#else
    return std::sqrt(a);
#endif
}

// the scale of a state: the population variance of the discounted return, as VecNormalize divides by sqrt(ret_rms.var + eps)
__host__ __device__ inline float return_norm_scale(double n, double m2, double eps) {
    return n == 0.0 ? 1.0f : (float) retnorm_div(1.0, retnorm_sqrt(retnorm_div(m2, n) + eps));
}

// the sums of n_b counted values around the pivot K into state = {n, mean, M2} ("running feature statistics", Chan et al.), then the
// scale.  n_b == 0 writes nothing
__host__ __device__ inline void return_norm_fold(double *state, float *scale, double n_b, double K, double S1, double S2, double eps) {
    if (!(n_b > 0.0)) return;
    const double n = state[0];
    const double t = S2 - retnorm_div(S1 * S1, n_b);
    const double m2b = t < 0.0 ? 0.0 : t;  // (a NaN stays one)
    const double n1 = n + n_b;
    double mean, m2;
    if (n > 0.0) {
        const double db = retnorm_div(S1, n_b);
        mean = K + retnorm_div(S1, n1);
        m2 = (state[2] + m2b) + (db * db) * retnorm_div(n * n_b, n1);
    } else {
        mean = K + retnorm_div(S1, n_b);
        m2 = m2b;
    }
    state[0] = n1;
    state[1] = mean;
    state[2] = m2;
    *scale = return_norm_scale(n1, m2, eps);
}

// k_return_moments and k_return_merge
struct ReturnMomentsArgs {
    int64_t n_envs, T;
    int32_t D;                 // reward at column D, done at D + 1 of a packed row of D + 2
    float gamma;
    double eps;
    const float *packed;       // [T][N][D + 2]
    const uint8_t *mask;       // [N] or null
    float *carry;              // [N]
    double *partials;          // [blocks][3]: n_b, S1, S2
    double *pivot;             // [2]: the n and the K launch 1 used
    double *state;             // [3]: n, mean, M2
    float *scale;              // [1]
};

void launch_return_moments(const ReturnMomentsArgs &a, hipStream_t stream);
void launch_return_reset_carry(float *carry, const uint8_t *mask, int64_t n_envs, hipStream_t stream);
void launch_return_reset(double *state, float *scale, float *carry, int64_t n_envs, hipStream_t stream);

}  // namespace chub
#endif
