// chub_gae.hip -- generalised advantage estimation over a rollout's blocks (include/chub.h: chub_rollout_gae_device, and with the reward
// scaled chub_return_norm_gae_device).  The launch arguments, the recurrence's step and the reductions are chub_gae.h's.  No atomics
// anywhere: two calls give the same bits.  Built with -ffp-contract=off.
#include "chub_gae.h"

namespace chub {

// One lane per env, consecutive lanes on consecutive envs: V, adv and ret are coalesced rows of [t][N]; reward and done are the last two
// floats of a packed row, fetched as one 8-byte load.  Only the adv recurrence is serial in t, so the loads of kGaeAhead steps are issued
// before the chain that consumes them.
// SCALED: the reward is r' = r * scale32, clipped by selects (a NaN stays a NaN).  scale32 is ONE uniform load from the caller's word: a
// replayed graph multiplies by what the update launched before it left there.  The unscaled kernel reads neither scale nor clip.
// Statistics: a lane sums its env's advantages and their squares in f64 in the order it writes them, the workgroup's lanes meet in the
// tree, the workgroups' partials are summed by ONE workgroup of a second launch in a fixed order.
template <bool SCALED>
__global__ __launch_bounds__(kGaeLanes) void k_gae(const GaeArgs a) {
    __shared__ double red[3][kGaeLanes];
    const int tid = (int) threadIdx.x;
    const int64_t e = (int64_t) blockIdx.x * kGaeLanes + tid, N = a.n_envs;
    const bool live = e < N && (!a.mask || a.mask[e] != 0);
    [[maybe_unused]] const float scale = SCALED ? *a.scale : 1.0f, clip = SCALED ? a.clip : 0.0f, nclip = -clip;
    double cnt = 0.0, sum = 0.0, sq = 0.0;
    if (live) {
        const int64_t row = (int64_t) a.D + 2;
        const float fin = a.final_values ? a.final_values[e] : 0.0f;
        float v_next = a.values[a.T * N + e], adv = 0.0f;
        for (int64_t t1 = a.T; t1 > 0; t1 -= kGaeAhead) {
            float v[kGaeAhead];
            GaeRewardDone rd[kGaeAhead];
#pragma unroll
            for (int k = 0; k < kGaeAhead; k++) {
                const int64_t t = t1 - 1 - k;
                if (t >= 0) {
                    v[k] = a.values[t * N + e];
                    rd[k] = *(const GaeRewardDone *) (a.packed + (t * N + e) * row + a.D);
                }
            }
#pragma unroll
            for (int k = 0; k < kGaeAhead; k++) {
                const int64_t t = t1 - 1 - k;
                if (t >= 0) {
                    float r = rd[k].r;
                    if constexpr (SCALED) {
                        r = __fmul_rn(r, scale);
                        if (clip != 0.0f) r = r > clip ? clip : (r < nclip ? nclip : r);
                    }
                    const GaeStep s = gae_step(r, rd[k].d != 0.0f, v[k], fin, a.gamma, a.gl, v_next, adv);
                    adv = s.adv;
                    a.adv[t * N + e] = adv;
                    if (a.ret) a.ret[t * N + e] = s.ret;
                    sum += (double) adv;
                    sq += (double) adv * (double) adv;
                    v_next = v[k];
                }
            }
        }
        cnt = (double) a.T;
    }
    if (a.partials) {
        double w[3] = {cnt, sum, sq};
        block_sum(red, tid, w);
        if (tid == 0) {
            double *p = a.partials + (size_t) blockIdx.x * 3;
            p[0] = w[0]; p[1] = w[1]; p[2] = w[2];
        }
    }
}

__global__ __launch_bounds__(kGaeLanes) void k_gae_stats(const double *partials, int64_t blocks, double *stats) {
    __shared__ double red[3][kGaeLanes];
    const int tid = (int) threadIdx.x;
    double w[3];
    partials_sum(red, tid, partials, blocks, 3, w);
    if (tid == 0) {
        stats[0] = w[0]; stats[1] = w[1]; stats[2] = w[2];
    }
}

void launch_gae(const GaeArgs &a, hipStream_t stream) {
    if (a.n_envs <= 0) return;
    const int64_t nb = (a.n_envs + kGaeLanes - 1) / kGaeLanes;
    hipLaunchKernelGGL(a.scale ? k_gae<true> : k_gae<false>, dim3((unsigned) nb), dim3(kGaeLanes), 0, stream, a);
    if (a.partials && a.stats) hipLaunchKernelGGL(k_gae_stats, dim3(1), dim3(kGaeLanes), 0, stream, (const double *) a.partials, nb, a.stats);
}

}  // namespace chub
