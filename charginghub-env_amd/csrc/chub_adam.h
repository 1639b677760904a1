// chub_adam.h -- what the optimiser kernels (chub_adam.hip) and the host (chub_runtime.cpp) share: the argument blocks of include/chub.h's
// section "an optimiser on the device" and the row shuffle's definition, which the host form (chub_shuffle_rows) and the kernel both run.
// The parameters an optimiser steps are a policy's or a critic's LIVE device weights in PolicyLayer's layout (chub_policy.h).
#ifndef CHUB_ADAM_H
#define CHUB_ADAM_H

#include "chub_policy.h"

namespace chub {

// ---- the Adam step.  The flat parameter vector: for each layer W[l] [out][in] row-major, then b[l] [out]; a policy's log_std [G] last.
// Chunk c is entries c * kAdamChunk .. of it.  Both launches run workgroups of kAdamLanes lanes, at most kAdamMaxBlocks of them;
// workgroup b takes chunks b, b + blocks, ..  Within a chunk lane j takes entries j, j + 256, j + 512, j + 768.
constexpr int kAdamLanes = 256;
constexpr int kAdamPerLane = 4;
constexpr int kAdamChunk = kAdamLanes * kAdamPerLane;
constexpr int kAdamMaxBlocks = 64;
// the scalars of an optimiser, one block of f64 words in device memory (t is an int64 in its word)
enum AdamScalar {
    ADAM_LR = 0, ADAM_BETA1, ADAM_BETA2, ADAM_EPS, ADAM_WEIGHT_DECAY, ADAM_MAX_GRAD_NORM,
    ADAM_T, ADAM_P1, ADAM_P2,                 // what the last step left: written by lane 0 of workgroup 0 of the step launch alone
    ADAM_PREV_T, ADAM_PREV_P1, ADAM_PREV_P2,  // their copy, made by the norm launch: what every workgroup of the step launch reads
    ADAM_SCALARS
};
constexpr int kAdamStats = 4;  // t, norm, scale, 0 taken / 1 skipped / 2 held back by the gate

struct AdamArgs {
    float *w[kPolicyMaxLayers], *b[kPolicyMaxLayers];  // the target's live layers: [tiles][k_pad][32], [tiles * 32]
    float *log_std;                                    // [G] or null
    const float *gW[kPolicyMaxLayers], *gb[kPolicyMaxLayers], *glog_std;  // the trainer's layout
    int64_t param0[kPolicyMaxLayers + 1];  // first flat entry of layer l: out * (in + 1) each; param0[n_layers] is log_std's
    int64_t n;                             // entries of the vector
    int32_t in[kPolicyMaxLayers], out[kPolicyMaxLayers], k_pad[kPolicyMaxLayers];
    int32_t n_layers, chunks;
    float *m, *v;                          // [n] each
    double *scalars;                       // [ADAM_SCALARS]
    double *partials;                      // [chunks]: a chunk's sum of squares
    double *stats;                         // [kAdamStats] or null
    const int64_t *gate;                   // null, or a word in device memory: not 0 holds the step back (stats[3] = 2)
};

// [launch 1] the chunks' sums of squares and the copy of t, p1, p2; [launch 2] the step
void launch_adam_step(const AdamArgs &a, int norm_blocks, int step_blocks, hipStream_t stream);
// m = v = 0, t = 0, p1 = p2 = 1 (one launch)
void launch_adam_reset(float *m, float *v, int64_t n, double *scalars, hipStream_t stream);

// ---- the row shuffle (include/chub.h, chub_shuffle_rows_device): a six-round alternating unbalanced Feistel network over nb bits, its
// round function word 0 of Philox4x32-10, cycle-walked into 0 .. R - 1
constexpr uint32_t kShuffleSite = 17u;
constexpr int kShuffleRounds = 6;
constexpr int kShuffleWalkCap = 64;      // applications of E at most; an entry that has not landed by then is -1
constexpr int kShuffleLanes = 256;
constexpr int kShuffleMaxBlocks = 4096;  // a lane takes rows idx, idx + blocks * 256, ..

__host__ __device__ inline uint32_t shuffle_philox_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int i = 0; i < 10; i++) {
        const uint64_t p0 = (uint64_t) 0xD2511F53u * c0, p1 = (uint64_t) 0xCD9E8D57u * c2;
        const uint32_t h0 = (uint32_t) (p0 >> 32), l0 = (uint32_t) p0, h1 = (uint32_t) (p1 >> 32), l1 = (uint32_t) p1;
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// bit length of R - 1 (R >= 1)
__host__ __device__ inline int shuffle_bits(int64_t R) {
    int nb = 0;
    for (uint64_t x = (uint64_t) (R - 1); x; x >>= 1) nb++;
    return nb;
}

// E: a bijection of 0 .. 2^nb - 1
__host__ __device__ inline uint64_t shuffle_encrypt(uint64_t x, int nb, uint64_t key, uint64_t c) {
    const int lo = nb >> 1, hi = nb - lo;
    const uint32_t mask_lo = (uint32_t) ((1ull << lo) - 1ull), mask_hi = (uint32_t) ((1ull << hi) - 1ull);  // (nb <= 40: both fit a word)
    const uint32_t k0 = (uint32_t) key, k1 = (uint32_t) (key >> 32), c2 = (uint32_t) c, c3 = (uint32_t) (c >> 32);
    uint32_t left = (uint32_t) (x >> lo), right = (uint32_t) x & mask_lo;
    for (uint32_t i = 0; i < (uint32_t) kShuffleRounds; i++) {
        if (i & 1u) right ^= shuffle_philox_word0(left, (kShuffleSite << 16) | i, c2, c3, k0, k1) & mask_lo;
        else left ^= shuffle_philox_word0(right, (kShuffleSite << 16) | i, c2, c3, k0, k1) & mask_hi;
    }
    return ((uint64_t) left << lo) | (uint64_t) right;
}

// entry r of the permutation of 0 .. R - 1 under (key, c), or -1 past the walk's cap
__host__ __device__ inline int64_t shuffle_row(int64_t r, int64_t R, int nb, uint64_t key, uint64_t c) {
    if (nb == 0) return 0;
    uint64_t y = (uint64_t) r;
    for (int step = 0; step < kShuffleWalkCap; step++) {
        y = shuffle_encrypt(y, nb, key, c);
        if (y < (uint64_t) R) return (int64_t) y;
    }
    return -1;
}

void launch_shuffle_rows(uint64_t key, const int64_t *d_counter, int64_t offset, int64_t R, int64_t *d_rows, hipStream_t stream);

}  // namespace chub
#endif
