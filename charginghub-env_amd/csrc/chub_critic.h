// chub_critic.h -- what the critic kernels (chub_critic.hip) and the host (chub_runtime.cpp) share: the argument blocks of include/chub.h's
// section "a critic on the device".  The weight layout (PolicyLayer), the LDS images of stride 33, the dW tiles and the partials' layout
// are the actor gradient's (chub_policy.h: GradLayer and the kGrad* constants); the head is one linear output in one tile of 32.
#ifndef CHUB_CRITIC_H
#define CHUB_CRITIC_H

#include "chub_policy.h"

namespace chub {

// the CHUB_VLOSS_* enum of include/chub.h (chub_runtime.cpp asserts the two agree)
enum ValueLoss { VLOSS_MSE = 0, VLOSS_CLIPPED, VLOSS_COUNT };
constexpr int kCriticStats = 6;   // f64 partials per workgroup: rows, loss terms, clipped rows, (ret - v)^2, ret, ret^2
constexpr int kCriticValueBlocks = 1024;  // workgroups of the values call at most (a row's value does not depend on the count)

struct CriticArgs {
    int64_t R, rows_total;
    const int64_t *rows;          // [R] or null
    const float *x;               // [.][F] raw, row stride ld
    int64_t ld;
    const float *ret, *v_old;     // [rows_total]; null in a forward-only call (v_old: read under VLOSS_CLIPPED only)
    const float *mean, *inv_std;  // [F], read when normalize != 0
    GradLayer layer[kPolicyMaxLayers];
    float *values;                // [R] or null
    float *part;                  // [blocks][part_floats]: per dW tile [16 registers][64 lanes], then the bias block
    double *part64;               // [blocks][kCriticStats]
    float clip, clip_eps;
    int32_t n_layers, F, x_rows, d_row0[2], s_row0;
    int32_t hidden_act, normalize;
    int32_t loss, stats, backward, n_pairs, part_floats, bias_floats;  // stats == 0: the values call (ret is not read, nothing is summed)
};

struct CriticMergeArgs {
    const float *part;
    const double *part64;
    float *gW[kPolicyMaxLayers], *gb[kPolicyMaxLayers];
    double *stats;
    int64_t R;
    int64_t param0[kPolicyMaxLayers + 1];  // first flat parameter of layer l: out * (in + 1) each
    int32_t in[kPolicyMaxLayers], it[kPolicyMaxLayers], pair0[kPolicyMaxLayers], bias0[kPolicyMaxLayers];
    int32_t n_layers, blocks, part_floats, bias_base, backward;
};

// host-only: the largest dynamic LDS the critic kernel may be launched with (set once per process and device)
int critic_prepare();
// the forward alone: one launch of k_critic with backward = 0 and no merge
void launch_critic_values(const CriticArgs &a, int blocks, int lds_rows, hipStream_t stream);
// [launch 1, backward only] the row-major copies from the live device weights; [launch 2] k_critic on `blocks` workgroups with lds_rows
// rows of LDS; [launch 3] the merge
void launch_critic_grad(const CriticArgs &a, const CriticMergeArgs &m, int blocks, int lds_rows, bool in_registers, hipStream_t stream);

}  // namespace chub
#endif
