// chub_policy.h -- what the actor kernel (chub_policy.hip) and the host (chub_runtime.cpp) share: the kernel's argument block, the
// device weight layout and the enums of include/chub.h's section "an actor on the device", restated for device code.
#ifndef CHUB_POLICY_H
#define CHUB_POLICY_H

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace chub {

// the CHUB_PIN_* / CHUB_PACT_* / CHUB_PHEAD_* / CHUB_PSQ_* / CHUB_PRUN_* enums of include/chub.h (chub_runtime.cpp asserts the two agree)
enum PolicyInput { PIN_OBS = 0, PIN_PILE_OBS, PIN_STATION_PROFILE, PIN_FORECAST, PIN_COUNT };
enum PolicyAct { PACT_TANH = 0, PACT_RELU, PACT_COUNT };
enum PolicyHead { PHEAD_PILES = 0, PHEAD_LOADS, PHEAD_COUNT };
enum PolicySquash { PSQ_TANH = 0, PSQ_CLIP, PSQ_COUNT };
enum PolicyRun { PRUN_LOCKSTEP = 0, PRUN_AUTORESET, PRUN_COUNT };

constexpr int kPolicyMaxInputs = 4, kPolicyMaxLayers = 4, kPolicyMaxHidden = 256;
constexpr int kPolicyEnvTile = 32;    // envs per workgroup: the column count of v_mfma_f32_32x32x2_f32
constexpr int kPolicyOutTile = 32;    // outputs per accumulator tile: its row count
constexpr int kPolicyMaxWaves = 4;    // waves per workgroup at most (one output tile per wave and round)
// The activations of a tile live in two LDS images, [row][32 envs] f32: P holds the feature row and the outputs of the odd layers, Q the
// outputs of the even layers.  Together at most 512 rows (64 KiB, what a launch gets without asking for more).
constexpr int kPolicyLdsRows = 512;
// Sampling (include/chub.h, "sampling from the device actor"): the Philox site of the policy's noise (SITE_POLICY of chub_device.h) and the
// LDS rows behind the two images in which the waves' log-probability partials meet, [wave][32 envs].  They count towards the same 512
// rows: chub_policy_set_exploration refuses a policy whose images leave fewer (the deterministic fit rule is unchanged)
constexpr uint32_t kPolicySite = 15u;
constexpr int kPolicyLogpRows = kPolicyMaxWaves;
// A population (include/chub.h, "a population of actors"): the Philox site of the perturbation noise (SITE_POPULATION of chub_device.h)
constexpr uint32_t kPopulationSite = 16u;

// Device weight layout of one layer (built by k_policy_relayout from the trainer's row-major [out][in]): per tile of 32 outputs the
// transposed block [k_pad][32], zero beyond `in` and `out` -- lane l of a wave reads element 64 s + l of a tile at k-step s, which is
// W[32 tile + (l & 31)][2 s + (l >> 5)]: the A operand of the f32-input MFMA.  Biases are [32 tiles] with zeros beyond `out`.
struct PolicyLayer {
    const float *w;   // [tiles][k_pad][32]
    const float *b;   // [tiles * 32]
    int32_t k_pad;    // inputs, rounded up to the MFMA's k step (2); the LDS rows beyond `in` hold zeros
    int32_t tiles;    // output tiles of 32
};

struct PolicyBlock {
    const float *p;   // [N] rows of `width` floats with row stride ld
    int64_t ld;
    int32_t width;
    int32_t pad_;
};

struct PolicyArgs {
    static constexpr bool kSample = false;
    static constexpr bool kSet = false;
    int64_t n_envs;
    PolicyBlock in[kPolicyMaxInputs];
    PolicyLayer layer[kPolicyMaxLayers];
    const float *mean, *inv_std;  // [F], read when normalize != 0
    const uint8_t *mask;          // [N] or null
    float *actions;               // [N][A] or null (PILES)
    uint32_t *bits;               // [N][2 W] u32 = [N][W] u64, little-endian halves, or null (PILES)
    float *tail;                  // [N][2] or null: outputs S, S + 1 (PILES) / 2, 3 (LOADS)
    float *loads;                 // [N][2] (LOADS): outputs 0, 1
    float clip;
    int32_t n_inputs, n_layers, F, f_pad;
    int32_t q_row0;               // first row of the Q image
    int32_t hidden_act, squash, normalize, head;
    int32_t S, A, W;              // piles, outputs of the head, u64 words per env
};

// what the sampled instantiation of k_policy takes on top: the noise's counter and key, the Gaussian scale, the normal tables of the handle
// (chub_device.h: normal_icdf / normal_tail) and the outputs only a sampled call has
struct PolicySampleArgs : PolicyArgs {
    static constexpr bool kSample = true;
    const uint32_t *tick_base;    // the handle's device-side tick offset: the launch's Philox tick is tick + *tick_base, as a step's
    const float *log_std;         // [G], the policy's own buffer (never moves)
    const float *normal_icdf, *normal_tail;  // [4097] each
    float *u;                     // [N][G] or null: the pre-squash Gaussian samples
    float *logp;                  // [N]
    float *features;              // [N][F] or null: the raw feature row
    uint32_t key[2], tick, gid0;  // the policy's key, the host tick of the handle's next launch, global id of env 0
    int32_t G;                    // Gaussian outputs: 2 (PILES), 4 (LOADS)
    int32_t r_row0;               // first of the kPolicyLogpRows LDS rows of the log-probability partials
};

// the sampled instantiation whose log-probability counts a pile's Bernoulli term only where the pile's bit is in a set (include/chub.h,
// "pile sets"): the u32 word t of an env's set is exactly the 32 outputs of accumulator tile t.  Everything else is PolicySampleArgs' launch
struct PolicySampleSetArgs : PolicySampleArgs {
    static constexpr bool kSet = true;
    const uint32_t *set;          // [N][2 W] u32 = [N][W] u64, little-endian halves: chub_pile_set_device's words
};

// the deterministic launch over a population (include/chub.h, "a population of actors"): member m's weights serve the tiles of 32 envs
// m tiles_per_member .. (m + 1) tiles_per_member - 1 -- a tile belongs to one member -- and lie m w_stride[l] / m b_stride[l] floats
// behind layer[l].w / layer[l].b, which point at member 0.  Workgroup b takes tile xcd_order(b) (chub_kernels.hip): the workgroups of
// one XCD take a contiguous eighth of the tiles, so a member's tiles share an L2.  Everything else is PolicyArgs' launch
struct PolicyPopArgs : PolicyArgs {
    static constexpr bool kPop = true;
    int32_t tiles_per_member;     // E / 32
    int32_t pad_;
    int64_t w_stride[kPolicyMaxLayers], b_stride[kPolicyMaxLayers];
};

void launch_policy(const PolicyArgs &a, int waves, hipStream_t stream);
void launch_policy_pop(const PolicyPopArgs &a, int waves, hipStream_t stream);
void launch_policy_sample(const PolicySampleArgs &a, int waves, hipStream_t stream);
void launch_policy_sample_set(const PolicySampleSetArgs &a, int waves, hipStream_t stream);

// running feature statistics (include/chub.h, chub_moments_update_device).  A workgroup's 256 lanes lie along the columns of a row: lane
// r_in * L + c takes column c (and c + L where F > 256) of row r_in of the workgroup's pass, L = min(F, 256) lanes per row and
// RW = 256 / L rows per pass.  Workgroup b takes passes b, b + blocks, b + 2 blocks, ..: the rows a workgroup sees depend on (R, F) only.
struct MomentsArgs {
    const float *x;               // [R] rows of F floats with row stride ld
    int64_t ld, R, passes;        // passes = ceil(R / RW)
    int64_t n_envs, e_step;       // (mask) row r belongs to env r % N; e_step = (blocks * RW) % N
    const uint8_t *mask;          // [N] or null
    const double *state;          // [1 + 2F]: n | mean[F] | M2[F]
    double *partials;             // [blocks][1 + 2F]: count | S1[F] | S2[F] per workgroup
    double *pivot;                // [1 + F]: the state's n and the pivots K[F] of this call, left by workgroup 0 for the merge
    int32_t F, L, RW, blocks;
};
constexpr int kMomentsLanes = 256;
constexpr int kMomentsAhead = 8;        // passes a lane has in flight (measured against 4 and 16: DESIGN.md 6.21)
constexpr int kMomentsMergeCols = 32;   // columns per workgroup of the merge launch, kMomentsLanes / 32 groups of partials each
void launch_moments(const MomentsArgs &a, double *state, hipStream_t stream);
// the policy's normaliser from a moments state: mean32[f] = (float) mean[f], inv_std32[f] = (float) (1 / sqrt(M2[f] / n + eps)); n == 0: nothing
void launch_normalizer_from_moments(const double *state, int F, double eps, float *mean32, float *inv_std32, hipStream_t stream);
// W [out][in] row-major and b [out] in device memory -> the layout above
void launch_policy_relayout(const float *d_W, const float *d_b, float *d_w, float *d_bias, int out, int in, int k_pad, int tiles, hipStream_t stream);


// ---- a population's weights (include/chub.h, "a population of actors").  One layer of every member: member m's block of the layout above
// lies m * stride floats behind w / bias.  Layer l is the augmented matrix [W | b], columns k = 0 .. in (column `in` the bias); a lane
// owns (pair j, output row, column group k >> 2) and one Philox block: eps of column k is normal_from_word of word k & 3 of the block with
// counter (row << 8 | k >> 2, 16 << 16 | l, generation, j) under the population's key
struct PopLayerArgs {
    float *w, *bias;              // member 0's [tiles][k_pad][32] and [tiles * 32]
    int64_t stride;               // floats from a member's block to the next member's
    int32_t out, in, k_pad, tiles, layer;
    int32_t pairs;                // P / 2
    uint32_t key[2], generation;
    const float *normal_icdf, *normal_tail;  // [4097] each: the handle's tables
};
// theta + / - sigma eps into members 2j / 2j + 1, fused with the re-layout.  device_layout == 0: W [out][in], b [out] (the trainer's);
// != 0: W = a [tiles][k_pad][32] block, b = [tiles * 32] (the centre policy's own weights)
void launch_population_perturb(const PopLayerArgs &a, const float *W, const float *b, int device_layout, float sigma, hipStream_t stream);
// partial[c][item][4] f64: the sum over the pairs j of chunk c, ascending, of (util[2j] - util[2j + 1]) eps; item = row * groups + k >> 2,
// groups = in / 4 + 1.  Then g = (float) (the chunks' sum, ascending) in the trainer's layout
void launch_population_es_gradient(const PopLayerArgs &a, const float *d_util, int chunk_pairs, int chunks, double *partials, float *gW, float *gb,
                                   hipStream_t stream);
// the kernel's layout of one member's layer -> W [out][in], b [out]
void launch_policy_unlayout(const float *d_w, const float *d_bias, float *d_W, float *d_b, int out, int in, int k_pad, hipStream_t stream);
// member dst[i] <- member src[i], i = 0 .. count - 1, all sources read (into `stage`, [count][member_floats]) before any destination is
// written; a pair with an index outside 0 .. P - 1 is skipped; of two pairs with one destination the later wins
void launch_population_copy(float *params, float *stage, int64_t member_floats, int P, const int32_t *d_src, const int32_t *d_dst, int count,
                            hipStream_t stream);

// ---- actor gradients (include/chub.h, "actor gradients on the device").  A workgroup of four waves walks tiles of 32 rows b, b + blocks,
// ..; every image of a tile lives in LDS as [row][kGradRowStride] f32: the feature rows X, the output of EVERY hidden layer, two delta
// images and a few scratch rows.  The stride of 33 words keeps both read directions free of bank conflicts: across the 32 rows of the
// tile at one feature (the forward's and W^T delta's B operand: consecutive words) and across 32 features at one row of the tile (both
// operands of dW += delta h^T: word 33 i + e, every bank once).  No image is kept twice.
constexpr int kGradLanes = 256;
constexpr int kGradWaves = kGradLanes / 64;
constexpr int kGradRowStride = 33;
constexpr int kGradScratchRows = 16;     // [wave] logp partials, [wave] entropy partials, coefficient, entropy weight, [G] log_std terms, row indices
constexpr int kGradLdsBytes = 160 * 1024;  // what a CU has; the launch asks for its rows through the function attribute
constexpr int kGradMaxBlocks = 512;      // workgroups at most
constexpr size_t kGradPartialBytes = 256u << 20;  // .. and fewer where their f32 partials would come to more than this
constexpr int kGradRegSlots = 4;         // dW tiles of 32 x 32 a wave keeps in registers (else they live in the workgroup's partials)
constexpr int kGradStats = 6, kGradPart64 = kGradStats + 4;  // f64 partials per workgroup: the stats, then the log_std sums
enum PolicyLoss { PLOSS_COEF = 0, PLOSS_PPO_CLIP, PLOSS_COUNT };

struct GradLayer {
    const float *w, *b;   // the forward's layout (PolicyLayer)
    const float *wrm;     // [32 ot][32 it] row-major, zeros beyond out / in: the A operand of delta_in = W^T delta_out (null for layer 0)
    int32_t k_pad, in, out;
    int32_t ot, it;       // tiles of 32 outputs / inputs
    int32_t h_row0;       // first LDS row of the layer's output image (hidden layers)
    int32_t pair0;        // the layer's first dW tile among the call's: tile (t, c) is pair0 + t * it + c
    int32_t bias0;        // the layer's first float in the bias block of a workgroup's partials
};

struct PolicyGradArgs {
    int64_t R, rows_total;
    const int64_t *rows;          // [R] or null
    const float *features;        // [.][F] raw, row stride ld
    int64_t ld;
    const uint32_t *pile_bits, *set_bits;  // [.][2 W] u32 (PILES); set_bits null: every pile
    const float *u, *logp_old, *adv;
    const double *adv_stats;      // [3] or null
    const float *mean, *inv_std, *log_std;
    GradLayer layer[kPolicyMaxLayers];
    float *logp_new, *entropy;    // [R] or null
    float *part;                  // [blocks][part_floats]: per pair [16 registers][64 lanes], then the bias block
    double *part64;               // [blocks][kGradPart64]
    float clip, clip_eps, ent_coef;
    int32_t n_layers, F, x_rows, d_row0[2], s_row0;
    int32_t hidden_act, normalize, head, S, A, W, G;
    int32_t loss, backward, n_pairs, part_floats, bias_floats;
};

struct GradMergeArgs {
    const float *part;
    const double *part64;
    float *gW[kPolicyMaxLayers], *gb[kPolicyMaxLayers], *glog_std;
    double *stats;
    int64_t R;
    int64_t param0[kPolicyMaxLayers + 1];  // first flat parameter of layer l: out * (in + 1) each
    int32_t in[kPolicyMaxLayers], out[kPolicyMaxLayers], it[kPolicyMaxLayers], pair0[kPolicyMaxLayers], bias0[kPolicyMaxLayers];
    int32_t n_layers, blocks, part_floats, bias_base, G, backward;
};

// host-only: the largest dynamic LDS the gradient kernel may be launched with (set once per process and device)
int policy_grad_prepare();
// [launch 1, backward only] the row-major copies from the live device weights; [launch 2] k_policy_grad on `blocks` workgroups with
// lds_rows rows of LDS; [launch 3] the merge
void launch_policy_grad(const PolicyGradArgs &a, const GradMergeArgs &m, int blocks, int lds_rows, bool in_registers, hipStream_t stream);

}  // namespace chub
#endif
