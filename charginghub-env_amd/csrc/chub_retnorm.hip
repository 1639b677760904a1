// chub_retnorm.hip -- reward scaling on the device (include/chub.h): the running variance of the discounted return over a rollout's blocks
// (k_return_moments and its one-workgroup merge) and the two reset streams.  The GAE that multiplies every reward by the scale that state
// gives is chub_gae.hip's k_gae<true>.  The launch arguments and the merge's arithmetic are chub_retnorm.h's; the (reward, done) pair and
// the reductions are chub_gae.h's.  No atomics anywhere: two calls give the same bits.  Built with -ffp-contract=off; where an operation's rounding is part of the definition it is written as the _rn intrinsic.
#include "chub_retnorm.h"

#include "chub_gae.h"

namespace chub {

static_assert(kRetLanes == kGaeLanes, "the return's sums meet in the tree the GAE's statistics take");

// ---- the discounted return's sums.  One lane per env, consecutive lanes on consecutive envs, forward in t.  Only g is serial in t: the
// (reward, done) loads of kRetAhead steps are issued before the chain that consumes them, with NO branch around a load -- a step past
// T - 1 reads step T - 1 again and a select drops it (loads under per-step branches are waited for one by one).  g is f32,
// every operation rounded once; a lane keeps n_b, S1 and S2 of d = (double) g - K in f64 in the order it forms them.  Workgroup 0 copies
// the n and the pivot every workgroup used: the merge reads those, so the lane that writes the state's n races no reader.
__global__ __launch_bounds__(kRetLanes) void k_return_moments(const ReturnMomentsArgs a) {
    __shared__ double red[3][kRetLanes];
    const int tid = (int) threadIdx.x;
    const int64_t e = (int64_t) blockIdx.x * kRetLanes + tid, N = a.n_envs;
    const double n0 = a.state[0];
    const double K = n0 > 0.0 ? a.state[1] : (double) a.packed[a.D];  // (uniform loads; block 0's row 0 serves whether env 0 is masked or not)
    if (blockIdx.x == 0 && tid == 0) {
        a.pivot[0] = n0;
        a.pivot[1] = K;
    }
    const bool live = e < N && (!a.mask || a.mask[e] != 0);
    double w[3] = {0.0, 0.0, 0.0};  // n_b, S1, S2
    if (live) {
        const int64_t row = (int64_t) a.D + 2, step = N * row, last = a.T - 1;
        const float *p = a.packed + e * row + a.D;  // (step t's pair lies at p + t * step)
        float g = a.carry[e];
        for (int64_t t0 = 0; t0 < a.T; t0 += kRetAhead) {
            GaeRewardDone rd[kRetAhead];
#pragma unroll
            for (int k = 0; k < kRetAhead; k++) {
                const int64_t t = t0 + k;
                rd[k] = *(const GaeRewardDone *) (p + (t > last ? last : t) * step);
            }
#pragma unroll
            for (int k = 0; k < kRetAhead; k++) {
                const bool ok = t0 + k <= last;
                const float gn = __fadd_rn(__fmul_rn(a.gamma, g), rd[k].r);
                const double d = __dsub_rn((double) gn, K);
                w[1] = ok ? __dadd_rn(w[1], d) : w[1];
                w[2] = ok ? __dadd_rn(w[2], __dmul_rn(d, d)) : w[2];
                g = ok ? (rd[k].d != 0.0f ? 0.0f : gn) : g;  // (zeroed AFTER it was counted: VecNormalize's order)
            }
        }
        a.carry[e] = g;
        w[0] = (double) a.T;
    }
    block_sum(red, tid, w);
    if (tid == 0) {
        double *q = a.partials + (size_t) blockIdx.x * 3;
        q[0] = w[0]; q[1] = w[1]; q[2] = w[2];
    }
}

// the workgroups' partials in ONE workgroup (chub_gae.h, partials_sum); lane 0 merges into the state and writes the scale.  n and K are launch 1's copies
__global__ __launch_bounds__(kRetLanes) void k_return_merge(const double *partials, int64_t blocks, const double *pivot, double *state, float *scale,
                                                            double eps) {
    __shared__ double red[3][kRetLanes];
    const int tid = (int) threadIdx.x;
    double w[3];
    partials_sum(red, tid, partials, blocks, 3, w);
    if (tid == 0 && w[0] > 0.0) {
        double st[3] = {pivot[0], state[1], state[2]};
        float sc = 1.0f;
        return_norm_fold(st, &sc, w[0], pivot[1], w[1], w[2], eps);
        state[0] = st[0]; state[1] = st[1]; state[2] = st[2];
        *scale = sc;
    }
}

// ---- the resets: streams over the carry.  With a mask only the named envs' entries are zeroed
__global__ __launch_bounds__(kRetLanes) void k_return_reset_carry(float *carry, const uint8_t *mask, int64_t n) {
    const int64_t stride = (int64_t) gridDim.x * kRetLanes;
    for (int64_t i = (int64_t) blockIdx.x * kRetLanes + threadIdx.x; i < n; i += stride)
        if (!mask || mask[i] != 0) carry[i] = 0.0f;
}

__global__ __launch_bounds__(kRetLanes) void k_return_reset(double *state, float *scale, float *carry, int64_t n) {
    const int64_t stride = (int64_t) gridDim.x * kRetLanes;
    const int64_t i0 = (int64_t) blockIdx.x * kRetLanes + threadIdx.x;
    if (i0 < 3) state[i0] = 0.0;
    if (i0 == 3) *scale = 1.0f;
    for (int64_t i = i0; i < n; i += stride) carry[i] = 0.0f;
}

static unsigned ret_stream_blocks(int64_t n) {
    int64_t nb = (n + kRetLanes - 1) / kRetLanes;
    if (nb > kRetStreamBlocks) nb = kRetStreamBlocks;
    return (unsigned) (nb < 1 ? 1 : nb);
}

void launch_return_moments(const ReturnMomentsArgs &a, hipStream_t stream) {
    if (a.n_envs <= 0) return;
    const int64_t nb = (a.n_envs + kRetLanes - 1) / kRetLanes;
    hipLaunchKernelGGL(k_return_moments, dim3((unsigned) nb), dim3(kRetLanes), 0, stream, a);
    hipLaunchKernelGGL(k_return_merge, dim3(1), dim3(kRetLanes), 0, stream, (const double *) a.partials, nb, (const double *) a.pivot, a.state, a.scale,
                       a.eps);
}

void launch_return_reset_carry(float *carry, const uint8_t *mask, int64_t n_envs, hipStream_t stream) {
    if (n_envs <= 0) return;
    hipLaunchKernelGGL(k_return_reset_carry, dim3(ret_stream_blocks(n_envs)), dim3(kRetLanes), 0, stream, carry, mask, n_envs);
}

void launch_return_reset(double *state, float *scale, float *carry, int64_t n_envs, hipStream_t stream) {
    hipLaunchKernelGGL(k_return_reset, dim3(ret_stream_blocks(n_envs)), dim3(kRetLanes), 0, stream, state, scale, carry, n_envs);
}

}  // namespace chub
