// chub_lagrange.hip -- constrained PPO on the device (include/chub.h): the cost advantages and episode costs of a collected rollout
// (k_cost_gae and its one-workgroup merge), the multipliers' projected ascent (k_lagrange_step) and the combined advantage
// (k_lagrange_combine).  The launch arguments and the step rule are chub_lagrange.h's; the recurrence's step and the reductions are
// chub_gae.h's, shared with the reward's GAE.  No atomics anywhere: two calls give the same bits.
// Built with -ffp-contract=off; where an operation's rounding is part of the definition it is written as the _rn intrinsic.
#include "chub_lagrange.h"

#include "chub_gae.h"

namespace chub {

static_assert(kLagLanes == kGaeLanes, "the cost advantages' statistics take the tree the reward advantages' take");

// a wave-uniform base plus a lane's 32-bit byte offset: the lane keeps one offset per array, not a 64-bit address per load in flight
template <class T>
__device__ __forceinline__ T *lag_at(T *base, uint32_t byte_offset) {
    return (T *) ((uintptr_t) base + byte_offset);
}

// ---- cost advantages and episode costs.  One lane per env, consecutive lanes on consecutive envs: done, V, adv and ret are read and written
// as k_gae reads and writes them; a cost is ONE float of a terms row, so a wave's cost load touches 64 rows C floats apart (callers collect
// only the columns they constrain).  Only the recurrences are serial in t: the loads of kGaeAhead steps -- done once, a cost and a value per
// constraint -- are issued before the chain that consumes them, with no branch around a load (a step before t = 0 reads step 0 again and a
// select drops it).  All K constraints share the pass over done.  K is a template argument: every per-constraint array is indexed by
// constants and stays in registers.
template <int K>
__global__ __launch_bounds__(kLagLanes) void k_cost_gae(const CostGaeArgs a) {
    __shared__ double red[kLagStats][kLagLanes];
    const int tid = (int) threadIdx.x;
    const int64_t e = (int64_t) blockIdx.x * kLagLanes + tid, N = a.n_envs;
    const bool live = e < N && (!a.mask || a.mask[e] != 0);
    double w[K][kLagStats];
#pragma unroll
    for (int c = 0; c < K; c++)
#pragma unroll
        for (int i = 0; i < kLagStats; i++) w[c][i] = 0.0;
    if (live) {
        const int64_t row = (int64_t) a.D + 2, C = a.C;
        // the lane's BYTE offsets inside a step's block (the host has checked that a block's bytes fit 32 bits)
        const uint32_t o_env = (uint32_t) e * 4u, o_done = (uint32_t) (e * row + a.D + 1) * 4u, o_terms = (uint32_t) (e * C) * 4u;
        float fin[K], v_next[K], adv[K];
        double seg[K], carry_in[K], carry_out[K];
        bool open = true;
#pragma unroll
        for (int c = 0; c < K; c++) {
            fin[c] = a.final_values[c] ? a.final_values[c][e] : 0.0f;
            v_next[c] = a.values[c] ? a.values[c][a.T * N + e] : 0.0f;
            carry_in[c] = a.carry ? a.carry[e * K + c] : 0.0;
            adv[c] = 0.0f;
            seg[c] = 0.0;
            carry_out[c] = 0.0;
        }
        for (int64_t t1 = a.T; t1 > 0; t1 -= kGaeAhead) {
            float d[kGaeAhead], cost[kGaeAhead][K], v[kGaeAhead][K];
#pragma unroll
            for (int k = 0; k < kGaeAhead; k++) {
                const int64_t t = t1 - 1 - k, tt = t < 0 ? 0 : t;
                d[k] = *lag_at(a.packed + tt * N * row, o_done);  // (a uniform base and the lane's 32-bit offset: one address register per array)
#pragma unroll
                for (int c = 0; c < K; c++) {
                    cost[k][c] = *lag_at(a.terms + tt * N * C + a.column[c], o_terms);
                    v[k][c] = a.values[c] ? *lag_at(a.values[c] + tt * N, o_env) : 0.0f;
                }
            }
#pragma unroll
            for (int k = 0; k < kGaeAhead; k++) {
                const int64_t t = t1 - 1 - k;
                if (t >= 0) {
                    const bool done = d[k] != 0.0f;
#pragma unroll
                    for (int c = 0; c < K; c++) {
                        const float ct = a.kind[c] == COST_AT_DONE && !done ? 0.0f : cost[k][c];
                        const GaeStep s = gae_step<const float *>(ct, done, v[k][c], &fin[c], a.gamma, a.gl, &v_next[c], &adv[c]);
                        adv[c] = s.adv;
                        *lag_at(a.adv[c] + t * N, o_env) = adv[c];
                        if (a.ret[c]) *lag_at(a.ret[c] + t * N, o_env) = s.ret;
                        w[c][1] += (double) adv[c];
                        w[c][2] += __dmul_rn((double) adv[c], (double) adv[c]);
                        v_next[c] = v[k][c];
                        if (done) {
                            if (open) {
                                carry_out[c] = seg[c];
                            } else {
                                w[c][3] += 1.0;
                                w[c][4] += seg[c];
                                w[c][5] += __dmul_rn(seg[c], seg[c]);
                            }
                            seg[c] = (double) ct;
                        } else {
                            seg[c] = __dadd_rn(seg[c], (double) ct);
                        }
                    }
                    if (done) open = false;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < K; c++) {
            const double x = __dadd_rn(carry_in[c], seg[c]);
            if (open) {
                carry_out[c] = x;
            } else {
                w[c][3] += 1.0;
                w[c][4] += x;
                w[c][5] += __dmul_rn(x, x);
            }
            if (a.carry) a.carry[e * K + c] = carry_out[c];
            w[c][0] = (double) a.T;
        }
    }
#pragma unroll
    for (int c = 0; c < K; c++) {
        block_sum(red, tid, w[c]);
        __syncthreads();  // (the next constraint's words overwrite red)
        if (tid == 0) {
            double *p = a.partials + ((size_t) blockIdx.x * K + c) * kLagStats;
#pragma unroll
            for (int i = 0; i < kLagStats; i++) p[i] = w[c][i];
        }
    }
}

// the workgroups' partials in ONE workgroup (chub_gae.h, partials_sum), constraint by constraint
__global__ __launch_bounds__(kLagLanes) void k_cost_gae_merge(const double *partials, int64_t blocks, int K, double *stats) {
    __shared__ double red[kLagStats][kLagLanes];
    const int tid = (int) threadIdx.x;
    for (int c = 0; c < K; c++) {
        double w[kLagStats];
        partials_sum(red, tid, partials + c * kLagStats, blocks, (int64_t) K * kLagStats, w);
        __syncthreads();  // (the next constraint's words overwrite red)
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < kLagStats; i++) stats[c * kLagStats + i] = w[i];
        }
    }
}

// ---- the multipliers: one wave, lane k per constraint; reads only what earlier launches wrote
__global__ __launch_bounds__(64) void k_lagrange_step(const LagrangeStepArgs a) {
    const int k = (int) threadIdx.x;
    if (k < a.K) lagrange_step(a.lambda + k, a.words + k * kLagWords, a.stats + k * kLagStats, a.limit[k], a.lr[k], a.lambda_max[k]);
}

__global__ __launch_bounds__(64) void k_lagrange_set_lambda(double *lambda, const double *src, int K) {
    const int k = (int) threadIdx.x;
    if (k < K) lambda[k] = src[k];
}

// ---- the combined advantage: a streaming launch, a lane per entry and grid pass.  The constants are formed by every lane from words an
// earlier launch wrote (uniform loads).  out may be adv: a lane reads its entry before it writes it and no lane reads another's.
__global__ __launch_bounds__(kLagLanes) void k_lagrange_combine(const LagrangeCombineArgs a) {
    float m32 = 0.0f, s32 = 1.0f;
    if (a.adv_stats) {  // (chub_policy_grad_device's "Advantage" paragraph, operation for operation)
        const double cnt = a.adv_stats[0], m = __ddiv_rn(a.adv_stats[1], cnt);
        double var = __dsub_rn(__ddiv_rn(a.adv_stats[2], cnt), __dmul_rn(m, m));
        var = var > 0.0 ? var : 0.0;
        m32 = (float) m;
        s32 = (float) __ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(var, 1e-8)));
    }
    float l32[kLagMaxK], mc32[kLagMaxK];
    double lsum = 0.0;
#pragma unroll
    for (int k = 0; k < kLagMaxK; k++) {
        l32[k] = 0.0f;
        mc32[k] = 0.0f;
        if (k < a.K) {
            l32[k] = (float) a.lambda[k];
            mc32[k] = (float) __ddiv_rn(a.stats[k * kLagStats + 1], a.stats[k * kLagStats]);
            lsum = __dadd_rn(lsum, (double) l32[k]);
        }
    }
    const float inv32 = (float) __ddiv_rn(1.0, __dadd_rn(1.0, lsum));
    const int64_t stride = (int64_t) gridDim.x * kLagLanes;
    for (int64_t i = (int64_t) blockIdx.x * kLagLanes + threadIdx.x; i < a.n; i += stride) {
        float c[kLagMaxK];
#pragma unroll
        for (int k = 0; k < kLagMaxK; k++) c[k] = k < a.K && l32[k] != 0.0f ? a.advc[k][i] : 0.0f;
        float x = a.adv[i];
        if (a.adv_stats) x = __fmul_rn(__fsub_rn(x, m32), s32);
#pragma unroll
        for (int k = 0; k < kLagMaxK; k++)
            if (k < a.K && l32[k] != 0.0f) x = __fsub_rn(x, __fmul_rn(l32[k], __fsub_rn(c[k], mc32[k])));
        a.out[i] = __fmul_rn(x, inv32);
    }
}

void launch_cost_gae(const CostGaeArgs &a, hipStream_t stream) {
    if (a.n_envs <= 0) return;
    const int64_t nb = (a.n_envs + kLagLanes - 1) / kLagLanes;
    const dim3 grid((unsigned) nb), block(kLagLanes);
    switch (a.K) {
    case 1: hipLaunchKernelGGL(k_cost_gae<1>, grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL(k_cost_gae<2>, grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL(k_cost_gae<3>, grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL(k_cost_gae<4>, grid, block, 0, stream, a); break;
    }
    hipLaunchKernelGGL(k_cost_gae_merge, dim3(1), block, 0, stream, (const double *) a.partials, nb, (int) a.K, a.stats);
}

void launch_lagrange_step(const LagrangeStepArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(k_lagrange_step, dim3(1), dim3(64), 0, stream, a);
}

void launch_lagrange_set_lambda(double *lambda, const double *src, int K, hipStream_t stream) {
    hipLaunchKernelGGL(k_lagrange_set_lambda, dim3(1), dim3(64), 0, stream, lambda, src, K);
}

void launch_lagrange_combine(const LagrangeCombineArgs &a, hipStream_t stream) {
    if (a.n <= 0) return;
    int64_t nb = (a.n + kLagLanes - 1) / kLagLanes;
    if (nb > kLagCombineBlocks) nb = kLagCombineBlocks;
    hipLaunchKernelGGL(k_lagrange_combine, dim3((unsigned) nb), dim3(kLagLanes), 0, stream, a);
}

}  // namespace chub
