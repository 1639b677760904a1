// chub_policy.hip -- an MLP actor on the device (include/chub.h: "an actor on the device"): the observation the library already produces,
// through a few dense layers, to the action row or the pile bits the step already takes.  ONE launch per call.
//
// A workgroup takes a tile of 32 envs.  Their feature rows are gathered from up to four blocks (the caller's observation rows and the
// policy's scratch of the feature calls), normalised, and written into LDS as [feature][env].  Every layer is H_out^T = W . H_in^T on
// v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: bit for bit a k-ordered fmaf chain): the A operand is the layer's weights (output on
// the row, one f32 per lane straight from the device layout of chub_policy.h), the B operand the activations (env on the column, one f32
// per lane from LDS, 64 consecutive words per k-step: no bank conflict), the accumulator starts as the bias.  A wave owns one tile of 32
// outputs at a time; hidden activations go back to LDS for the next layer (two images, ping-pong), the head's accumulators are squashed
// and stored from registers: the action row, the tail pair and -- one ballot-free OR across the wave's two halves -- 32 pile bits per env.
//
// Numerics (the contract of the header): every product is rounded once and accumulated in f32; a layer's terms are added in ascending
// input index k = 0, 1, .. with the bias as the chain's initial value, for every env alike -- a column of the B operand never meets
// another column, so an env's outputs do not depend on N, the mask or its place in the tile.  Rows and columns beyond a layer's real
// size hold zeros (weights, biases and LDS rows), which add exactly nothing.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "chub_policy.h"

namespace chub {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the step kernels' own predicate on an action: a pile is on iff a >= this ((a + 1) / 2 >= 0.5 in f32; kActOnThreshold of chub_kernels.hip)
constexpr float kPolicyOnThreshold = -2.98023223876953125e-8f;

// accumulator register r of lane l holds output row (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the tile, for env column l & 31
__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

__global__ __launch_bounds__(64 * kPolicyMaxWaves) void k_policy(const PolicyArgs a) {
    extern __shared__ float lds[];
    const int tid = (int) threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int) (blockDim.x >> 6), nt = (int) blockDim.x;
    const int col = lane & 31, half = lane >> 5;
    const int64_t env0 = (int64_t) blockIdx.x * kPolicyEnvTile;
    float *const P = lds;
    float *const Q = lds + (size_t) a.q_row0 * kPolicyEnvTile;

    // ---- the feature rows of the tile: concatenate, normalise, transpose into P
    int f0 = 0;
#pragma unroll
    for (int b = 0; b < kPolicyMaxInputs; b++) {
        if (b < a.n_inputs) {
            const float *p = a.in[b].p;
            const int64_t ld = a.in[b].ld;
            const int width = a.in[b].width, total = kPolicyEnvTile * width;
            for (int idx = tid; idx < total; idx += nt) {
                const int j = idx / width, f = idx - j * width;
                const int64_t env = env0 + j;
                float x = 0.0f;  // (envs beyond N: zeros, never stored)
                if (env < a.n_envs) {
                    x = p[env * ld + f];
                    if (a.normalize) {
                        x = __fmul_rn(__fsub_rn(x, a.mean[f0 + f]), a.inv_std[f0 + f]);
                        x = fminf(fmaxf(x, -a.clip), a.clip);
                    }
                }
                P[(f0 + f) * kPolicyEnvTile + j] = x;
            }
            f0 += width;
        }
    }
    for (int idx = tid; idx < (a.f_pad - a.F) * kPolicyEnvTile; idx += nt) P[a.F * kPolicyEnvTile + idx] = 0.0f;
    __syncthreads();

    const int64_t env = env0 + col;
    const bool store = env < a.n_envs && (!a.mask || a.mask[env] != 0);

#pragma unroll
    for (int l = 0; l < kPolicyMaxLayers; l++) {
        if (l < a.n_layers) {
            const PolicyLayer L = a.layer[l];
            const bool last = l == a.n_layers - 1;
            const float *src = (l & 1) ? Q : P;
            float *dst = (l & 1) ? P : Q;
            const int ksteps = L.k_pad >> 1;
            for (int t = wave; t < L.tiles; t += nw) {
                f32x16 acc;
                const float *bt = L.b + t * kPolicyOutTile + 4 * half;
#pragma unroll
                for (int r = 0; r < 16; r++) acc[r] = bt[(r & 3) + 8 * (r >> 2)];
                const float *wt = L.w + (size_t) t * (size_t) L.k_pad * kPolicyOutTile + lane;
                const float *xs = src + lane;
                for (int s = 0; s < ksteps; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wt[64 * s], xs[64 * s], acc, 0, 0, 0);

                if (!last) {
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const float z = acc[r];
                        const float v = a.hidden_act == PACT_TANH ? tanhf(z) : fmaxf(z, 0.0f);
                        dst[(t * kPolicyOutTile + acc_row(r, half)) * kPolicyEnvTile + col] = v;
                    }
                } else {
                    uint32_t m = 0u;
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int n = t * kPolicyOutTile + acc_row(r, half);
                        const float z = acc[r];
                        const float v = a.squash == PSQ_TANH ? tanhf(z) : fminf(fmaxf(z, -1.0f), 1.0f);
                        if (a.head == PHEAD_PILES) {
                            if (n < a.S && v >= kPolicyOnThreshold) m |= 1u << (n & 31);
                            if (store && n < a.A) {
                                if (a.actions) a.actions[env * a.A + n] = v;
                                if (n >= a.S && a.tail) a.tail[env * 2 + (n - a.S)] = v;
                            }
                        } else if (store && n < 4) {
                            if (n < 2) a.loads[env * 2 + n] = v;
                            else a.tail[env * 2 + (n - 2)] = v;
                        }
                    }
                    if (a.head == PHEAD_PILES && a.bits) {
                        m |= (uint32_t) __shfl_xor((int) m, 32);
                        if (store && half == 0 && t < 2 * a.W) a.bits[env * (int64_t) (2 * a.W) + t] = m;
                    }
                }
            }
            __syncthreads();
        }
    }
}

void launch_policy(const PolicyArgs &a, int waves, hipStream_t stream) {
    if (a.n_envs <= 0) return;
    const int64_t nb = (a.n_envs + kPolicyEnvTile - 1) / kPolicyEnvTile;
    int q_rows = 0;  // (the Q image ends where the widest even hidden layer does)
    for (int l = 0; l + 1 < a.n_layers; l += 2) q_rows = a.layer[l].tiles * kPolicyOutTile > q_rows ? a.layer[l].tiles * kPolicyOutTile : q_rows;
    const size_t lds_bytes = (size_t) (a.q_row0 + q_rows) * kPolicyEnvTile * sizeof(float);
    hipLaunchKernelGGL(k_policy, dim3((unsigned) nb), dim3(64u * (unsigned) waves), lds_bytes, stream, a);
}

// the trainer's layout (nn.Linear: W [out][in] row-major, b [out]) -> the kernel's (chub_policy.h), zeros beyond `out` and `in`
__global__ void k_policy_relayout(const float *W, const float *b, float *w, float *bias, int out, int in, int k_pad, int tiles) {
    const int64_t total = (int64_t) tiles * k_pad * kPolicyOutTile;
    for (int64_t idx = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t) gridDim.x * blockDim.x) {
        const int i = (int) (idx & 31);
        const int64_t row = idx >> 5;
        const int k = (int) (row % k_pad), n = (int) (row / k_pad) * kPolicyOutTile + i;
        w[idx] = (n < out && k < in) ? W[(int64_t) n * in + k] : 0.0f;
    }
    for (int64_t idx = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; idx < (int64_t) tiles * kPolicyOutTile; idx += (int64_t) gridDim.x * blockDim.x)
        bias[idx] = idx < out ? b[idx] : 0.0f;
}

void launch_policy_relayout(const float *d_W, const float *d_b, float *d_w, float *d_bias, int out, int in, int k_pad, int tiles, hipStream_t stream) {
    const int64_t total = (int64_t) tiles * k_pad * kPolicyOutTile;
    int64_t nb = (total + 255) / 256;
    if (nb > 1024) nb = 1024;
    hipLaunchKernelGGL(k_policy_relayout, dim3((unsigned) nb), dim3(256), 0, stream, d_W, d_b, d_w, d_bias, out, in, k_pad, tiles);
}

}  // namespace chub
