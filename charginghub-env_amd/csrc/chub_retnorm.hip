// chub_retnorm.hip -- reward scaling on the device (include/chub.h): the running variance of the discounted return over a rollout's blocks
// (k_return_moments and its one-workgroup merge), the GAE that multiplies every reward by the scale that state gives (k_gae_scaled) and
// the two reset streams.  The launch arguments and the merge's arithmetic are chub_retnorm.h's.  No atomics anywhere: two calls give the
// same bits.  Built with -ffp-contract=off; where an operation's rounding is part of the definition it is written as the _rn intrinsic.
#include "chub_retnorm.h"

namespace chub {

// reward and done: the last two floats of a packed row as one 8-byte load (4-byte aligned: a row is D + 2 floats), as k_gae fetches them
struct __attribute__((packed, aligned(4))) RetRewardDone {
    float r, d;
};

// the tree k_gae's statistics take (chub_policy.hip, gae_block_sum): lane l takes lane l + h, h = 128 .. 1
__device__ __forceinline__ void ret_block_sum(double (*red)[kRetLanes], int tid, double &c, double &s, double &q) {
    red[0][tid] = c; red[1][tid] = s; red[2][tid] = q;
    __syncthreads();
    for (int h = kRetLanes / 2; h > 0; h >>= 1) {
        if (tid < h) {
#pragma unroll
            for (int i = 0; i < 3; i++) red[i][tid] += red[i][tid + h];
        }
        __syncthreads();
    }
    c = red[0][0]; s = red[1][0]; q = red[2][0];
}

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
    double cnt = 0.0, s1 = 0.0, s2 = 0.0;
    if (live) {
        const int64_t row = (int64_t) a.D + 2, step = N * row, last = a.T - 1;
        const float *p = a.packed + e * row + a.D;  // (step t's pair lies at p + t * step)
        float g = a.carry[e];
        for (int64_t t0 = 0; t0 < a.T; t0 += kRetAhead) {
            RetRewardDone rd[kRetAhead];
#pragma unroll
            for (int k = 0; k < kRetAhead; k++) {
                const int64_t t = t0 + k;
                rd[k] = *(const RetRewardDone *) (p + (t > last ? last : t) * step);
            }
#pragma unroll
            for (int k = 0; k < kRetAhead; k++) {
                const bool ok = t0 + k <= last;
                const float gn = __fadd_rn(__fmul_rn(a.gamma, g), rd[k].r);
                const double d = __dsub_rn((double) gn, K);
                s1 = ok ? __dadd_rn(s1, d) : s1;
                s2 = ok ? __dadd_rn(s2, __dmul_rn(d, d)) : s2;
                g = ok ? (rd[k].d != 0.0f ? 0.0f : gn) : g;  // (zeroed AFTER it was counted: VecNormalize's order)
            }
        }
        a.carry[e] = g;
        cnt = (double) a.T;
    }
    ret_block_sum(red, tid, cnt, s1, s2);
    if (tid == 0) {
        double *q = a.partials + (size_t) blockIdx.x * 3;
        q[0] = cnt; q[1] = s1; q[2] = s2;
    }
}

// the workgroups' partials in ONE workgroup: lane l takes partials l, l + 256, .. in ascending order, then the same tree; lane 0 merges
// into the state and writes the scale.  n and K are launch 1's copies
__global__ __launch_bounds__(kRetLanes) void k_return_merge(const double *partials, int64_t blocks, const double *pivot, double *state, float *scale,
                                                            double eps) {
    __shared__ double red[3][kRetLanes];
    const int tid = (int) threadIdx.x;
    double c = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t b = tid; b < blocks; b += kRetLanes) {
        c += partials[b * 3]; s1 += partials[b * 3 + 1]; s2 += partials[b * 3 + 2];
    }
    ret_block_sum(red, tid, c, s1, s2);
    if (tid == 0 && c > 0.0) {
        double st[3] = {pivot[0], state[1], state[2]};
        float sc = 1.0f;
        return_norm_fold(st, &sc, c, pivot[1], s1, s2, eps);
        state[0] = st[0]; state[1] = st[1]; state[2] = st[2];
        *scale = sc;
    }
}

// ---- the scaled GAE: k_gae (chub_policy.hip) restated, its layout, its recurrence operation for operation and its reduction, with the
// reward replaced by r' = r * scale32, clipped by selects (a NaN stays a NaN).  scale32 is ONE uniform load from the object's word: a
// replayed graph multiplies by what the update launched before it left there.
__global__ __launch_bounds__(kRetLanes) void k_gae_scaled(const ScaledGaeArgs a) {
    __shared__ double red[3][kRetLanes];
    const int tid = (int) threadIdx.x;
    const int64_t e = (int64_t) blockIdx.x * kRetLanes + tid, N = a.n_envs;
    const bool live = e < N && (!a.mask || a.mask[e] != 0);
    const float scale = *a.scale, clip = a.clip, nclip = -a.clip;
    double cnt = 0.0, sum = 0.0, sq = 0.0;
    if (live) {
        const int64_t row = (int64_t) a.D + 2;
        const float fin = a.final_values ? a.final_values[e] : 0.0f;
        float v_next = a.values[a.T * N + e], adv = 0.0f;
        for (int64_t t1 = a.T; t1 > 0; t1 -= kRetAhead) {
            float v[kRetAhead];
            RetRewardDone rd[kRetAhead];
#pragma unroll
            for (int k = 0; k < kRetAhead; k++) {
                const int64_t t = t1 - 1 - k;
                if (t >= 0) {
                    v[k] = a.values[t * N + e];
                    rd[k] = *(const RetRewardDone *) (a.packed + (t * N + e) * row + a.D);
                }
            }
#pragma unroll
            for (int k = 0; k < kRetAhead; k++) {
                const int64_t t = t1 - 1 - k;
                if (t >= 0) {
                    const bool done = rd[k].d != 0.0f;
                    float r = __fmul_rn(rd[k].r, scale);
                    if (clip != 0.0f) r = r > clip ? clip : (r < nclip ? nclip : r);
                    const float vn = done ? fin : v_next;
                    const float delta = __fsub_rn(__fadd_rn(r, __fmul_rn(a.gamma, vn)), v[k]);
                    adv = __fadd_rn(delta, __fmul_rn(a.gl, done ? 0.0f : adv));
                    a.adv[t * N + e] = adv;
                    if (a.ret) a.ret[t * N + e] = __fadd_rn(adv, v[k]);
                    sum += (double) adv;
                    sq += (double) adv * (double) adv;
                    v_next = v[k];
                }
            }
        }
        cnt = (double) a.T;
    }
    if (a.partials) {
        ret_block_sum(red, tid, cnt, sum, sq);
        if (tid == 0) {
            double *p = a.partials + (size_t) blockIdx.x * 3;
            p[0] = cnt; p[1] = sum; p[2] = sq;
        }
    }
}

// k_gae_stats restated: the workgroups' partials in one workgroup, the same order
__global__ __launch_bounds__(kRetLanes) void k_gae_scaled_stats(const double *partials, int64_t blocks, double *stats) {
    __shared__ double red[3][kRetLanes];
    const int tid = (int) threadIdx.x;
    double c = 0.0, s = 0.0, q = 0.0;
    for (int64_t b = tid; b < blocks; b += kRetLanes) {
        c += partials[b * 3]; s += partials[b * 3 + 1]; q += partials[b * 3 + 2];
    }
    ret_block_sum(red, tid, c, s, q);
    if (tid == 0) {
        stats[0] = c; stats[1] = s; stats[2] = q;
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

void launch_gae_scaled(const ScaledGaeArgs &a, hipStream_t stream) {
    if (a.n_envs <= 0) return;
    const int64_t nb = (a.n_envs + kRetLanes - 1) / kRetLanes;
    hipLaunchKernelGGL(k_gae_scaled, dim3((unsigned) nb), dim3(kRetLanes), 0, stream, a);
    if (a.partials && a.stats)
        hipLaunchKernelGGL(k_gae_scaled_stats, dim3(1), dim3(kRetLanes), 0, stream, (const double *) a.partials, nb, a.stats);
}

void launch_return_reset_carry(float *carry, const uint8_t *mask, int64_t n_envs, hipStream_t stream) {
    if (n_envs <= 0) return;
    hipLaunchKernelGGL(k_return_reset_carry, dim3(ret_stream_blocks(n_envs)), dim3(kRetLanes), 0, stream, carry, mask, n_envs);
}

void launch_return_reset(double *state, float *scale, float *carry, int64_t n_envs, hipStream_t stream) {
    hipLaunchKernelGGL(k_return_reset, dim3(ret_stream_blocks(n_envs)), dim3(kRetLanes), 0, stream, state, scale, carry, n_envs);
}

}  // namespace chub
