// chub_lagrange.h -- what the constrained learner's kernels (chub_lagrange.hip) and the host (chub_runtime.cpp) share: the launch arguments of
// include/chub.h's section "constrained PPO on the device" and the multiplier's step rule, which the kernel and the host form
// (chub_lagrange_fold) both run.  Every f64 operation below is one rounded operation (-ffp-contract=off).
#ifndef CHUB_LAGRANGE_H
#define CHUB_LAGRANGE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace chub {

// include/chub.h's CHUB_COST_* and CHUB_LAG_*, restated; chub_runtime.cpp asserts that they agree
enum CostKind { COST_STEP = 0, COST_AT_DONE, COST_KIND_COUNT };
constexpr int kLagMaxK = 4;     // constraints of one object
constexpr int kLagStats = 6;    // per constraint: count, sum, sum of squares of the advantages; episodes, sum and sum of squares of their costs
constexpr int kLagWords = 3;    // per constraint: J_last, steps taken, steps skipped
constexpr int kLagLanes = 256;  // a workgroup of k_cost_gae, of its merge and of k_lagrange_combine
constexpr int kLagCombineBlocks = 2048;  // the streaming launch's grid cap: a lane takes entries i, i + 2048 * 256, ..

// the step rule on one constraint: lambda, its three words, its six stats
__host__ __device__ inline void lagrange_step(double *lambda, double *w3, const double *st6, double limit, double lr, double lambda_max) {
    const double n = st6[3];
    const double J = st6[4] / n;
    if (n == 0.0 || !__builtin_isfinite(J)) {
        w3[2] = w3[2] + 1.0;
        return;
    }
    double l = *lambda + lr * (J - limit);
    l = l < 0.0 ? 0.0 : l;
    if (lambda_max != 0.0) l = l > lambda_max ? lambda_max : l;
    if (l != l) {  // (a multiplier that was set to NaN or an infinite one against lr = 0)
        w3[2] = w3[2] + 1.0;
        return;
    }
    *lambda = l;
    w3[1] = w3[1] + 1.0;
    w3[0] = J;
}

// k_cost_gae and its merge.  The reduction order is k_gae's: a lane sums in the order it writes (t descending), the workgroup's 256 lanes meet
// in the tree h = 128 .. 1 (lane l takes lane l + h), the merge's lane l takes partials l, l + 256, .. ascending, then the same tree
struct CostGaeArgs {
    int64_t n_envs, T;
    int32_t D, C, K;              // done at column D + 1 of a packed row of D + 2; a terms row has C floats
    float gamma, gl;              // gl = gamma * lambda, formed once in f32
    const float *terms;           // [T][N][C]
    const float *packed;          // [T][N][D + 2]
    const uint8_t *mask;          // [N] or null
    double *carry;                // [N][K] or null
    double *partials;             // [blocks][K][6]
    double *stats;                // [K][6]
    const float *values[kLagMaxK];        // [T + 1][N] or null
    const float *final_values[kLagMaxK];  // [N] or null
    float *adv[kLagMaxK], *ret[kLagMaxK]; // [T][N]; ret may be null
    int32_t column[kLagMaxK], kind[kLagMaxK];
};

struct LagrangeStepArgs {
    int32_t K;
    double *lambda, *words;       // [K], [K][3]
    const double *stats;          // [K][6]
    double limit[kLagMaxK], lr[kLagMaxK], lambda_max[kLagMaxK];
};

struct LagrangeCombineArgs {
    int64_t n;
    int32_t K;
    const float *adv;
    const double *adv_stats;      // [3] or null
    const double *lambda, *stats; // [K], [K][6]
    const float *advc[kLagMaxK];
    float *out;                   // may be adv
};

void launch_cost_gae(const CostGaeArgs &a, hipStream_t stream);
void launch_lagrange_step(const LagrangeStepArgs &a, hipStream_t stream);
void launch_lagrange_combine(const LagrangeCombineArgs &a, hipStream_t stream);
void launch_lagrange_set_lambda(double *lambda, const double *src, int K, hipStream_t stream);

}  // namespace chub
#endif
