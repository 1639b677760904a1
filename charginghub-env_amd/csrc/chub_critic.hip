// chub_critic.hip -- the critic of include/chub.h's section "a critic on the device": a feed-forward value network over rows of F floats,
// its forward, the value loss and the backward pass in one kernel for gfx950, and the merge of the workgroups' partials.
//
// A translation unit of its own: the kernels of chub_policy.hip and chub_kernels.hip are compiled from untouched text, so their listings
// cannot move.  The structure is k_policy_grad's (chub_policy.hip; the images and the partials' layout are chub_policy.h's):
// a workgroup of four waves walks tiles of 32 rows b, b + blocks, ..  Per tile: gather through d_rows and normalise into X as [feature][row];
// the forward as k_policy runs it (the same A operand from the same device layout, the same k order from the bias), every hidden layer into
// an image of its own; the head is ONE output row in one tile, computed by wave 0 into row 0 of delta image 0; 32 lanes form the rows'
// loss term and c = R dL/dv in place of v; then per layer, last to first, dW += delta h^T and db += delta 1 over the tile's 32 rows and
// delta_in = (W^T delta) act'(h) into the other delta image.  One MFMA form serves all three products (v_mfma_f32_32x32x2_f32, lane l gives
// A[l & 31][l >> 5] and B[l >> 5][l & 31]):
//   forward   C[out][row] : A = w[t][2 s + half][out]          B = h_in[2 s + half][row]      k = input
//   W^T delta C[in][row]  : A = wrm[2 s + half][32 c + in]      B = delta[2 s + half][row]     k = output
//   dW        C[out][in]  : A = delta[32 t + out][2 s + half]   B = h_in[32 c + in][2 s + half] k = row of the tile
// kSlots > 0: a wave's dW tiles (pair p belongs to wave p % 4, slot p / 4) stay in registers for the whole walk; kSlots == 0: they are
// read from and written to the workgroup's own slice of the partials around each tile's sixteen MFMAs, by the lane that owns them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "chub_critic.h"

namespace chub {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// register r of lane (col, half) of a 32 x 32 accumulator holds row (r & 3) + 8 (r >> 2) + 4 half at column col
__device__ __forceinline__ int critic_acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

__global__ void k_critic_wrm(const CriticArgs a) {
    for (int l = 1; l < a.n_layers; l++) {
        const GradLayer L = a.layer[l];
        const int ld = L.it * 32;
        const int64_t total = (int64_t) L.ot * 32 * ld;
        float *dst = const_cast<float *>(L.wrm);
        for (int64_t idx = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t) gridDim.x * blockDim.x) {
            const int n = (int) (idx / ld), k = (int) (idx - (int64_t) n * ld);
            dst[idx] = (n < L.out && k < L.in) ? L.w[((int64_t) (n >> 5) * L.k_pad + k) * kPolicyOutTile + (n & 31)] : 0.0f;
        }
    }
}

__device__ __forceinline__ f32x16 critic_dw_tile(f32x16 acc, const float *delta, const float *hin, int t, int c, int col, int half) {
    constexpr int RS = kGradRowStride;
    const float *as = delta + (t * 32 + col) * RS + half, *bs = hin + (c * 32 + col) * RS + half;
#pragma unroll
    for (int s = 0; s < 16; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[2 * s], bs[2 * s], acc, 0, 0, 0);
    return acc;
}

template <int kSlots>
__global__ __launch_bounds__(kGradLanes) void k_critic(const CriticArgs a) {
    constexpr int RS = kGradRowStride, nw = kGradWaves;
    extern __shared__ float lds[];
    const int tid = (int) threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    float *const X = lds;
    float *const D0 = lds + a.d_row0[0] * RS, *const D1 = lds + a.d_row0[1] * RS;
    float *const Sc = lds + a.s_row0 * RS;
    int64_t *const rowi = (int64_t *) (Sc + (kGradScratchRows - 2) * RS);  // (the last two scratch rows; s_row0 is even: 8-byte aligned)
    const int nl = a.n_layers;
    float *const mypart = a.part + (size_t) blockIdx.x * (size_t) a.part_floats;
    float *const mybias = mypart + (size_t) a.n_pairs * 1024;
    const float neg_eps = -a.clip_eps;

    f32x16 racc[kSlots > 0 ? kSlots : 1];
#pragma unroll
    for (int i = 0; i < (kSlots > 0 ? kSlots : 1); i++)
#pragma unroll
        for (int r = 0; r < 16; r++) racc[i][r] = 0.0f;
    if (a.backward) {
        if constexpr (kSlots == 0) {
            for (int p = wave; p < a.n_pairs; p += nw)
#pragma unroll
                for (int r = 0; r < 16; r++) mypart[((size_t) p * 16 + r) * 64 + lane] = 0.0f;
        }
        for (int l = 0; l < nl; l++)  // (the lane that zeroes a bias sum is the lane that adds to it)
            for (int n = tid; n < a.layer[l].ot * 32; n += kGradLanes) mybias[a.layer[l].bias0 + n] = 0.0f;
    }
    double st[kCriticStats] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

    const int64_t n_tiles = (a.R + 31) / 32;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        // ---- the tile's 32 row indices, resolved once (-1: past R, or an index outside the arrays)
        if (tid < 32) {
            const int64_t r = tile * 32 + tid;
            int64_t ri = -1;
            if (r < a.R) ri = a.rows ? a.rows[r] : r;
            rowi[tid] = (ri >= 0 && ri < a.rows_total) ? ri : -1;
        }
        __syncthreads();
        // ---- the rows of the tile, normalised with the critic's current normaliser, as [feature][row]
        for (int idx = tid; idx < 32 * a.F; idx += kGradLanes) {
            const int j = idx / a.F, f = idx - j * a.F;
            const int64_t ri = rowi[j];
            float x = 0.0f;
            if (ri >= 0) {
                x = a.x[ri * a.ld + f];
                if (a.normalize) {
                    x = __fmul_rn(__fsub_rn(x, a.mean[f]), a.inv_std[f]);
                    x = fminf(fmaxf(x, -a.clip), a.clip);
                }
            }
            X[f * RS + j] = x;
        }
        for (int idx = tid; idx < (a.x_rows - a.F) * 32; idx += kGradLanes) X[(a.F + (idx >> 5)) * RS + (idx & 31)] = 0.0f;
        const int64_t r_col = tile * 32 + col;
        const int64_t ri = rowi[col];
        const bool valid = ri >= 0;
        __syncthreads();

        // ---- the forward
#pragma unroll
        for (int l = 0; l < kPolicyMaxLayers; l++) {
            if (l < nl) {
                const GradLayer L = a.layer[l];
                const bool last = l == nl - 1;
                const float *src = l ? lds + a.layer[l ? l - 1 : 0].h_row0 * RS : X;
                float *dst = last ? D0 : lds + L.h_row0 * RS;
                const int ksteps = L.k_pad >> 1;
                for (int t = wave; t < L.ot; t += nw) {  // (the head has one tile: wave 0's)
                    f32x16 acc;
                    const float *bt = L.b + t * kPolicyOutTile + 4 * half;
#pragma unroll
                    for (int r = 0; r < 16; r++) acc[r] = bt[(r & 3) + 8 * (r >> 2)];
                    const float *wt = L.w + (size_t) t * (size_t) L.k_pad * kPolicyOutTile + lane;
                    const float *xs = src + half * RS + col;
                    for (int s = 0; s < ksteps; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wt[64 * s], xs[2 * RS * s], acc, 0, 0, 0);
                    if (!last) {
#pragma unroll
                        for (int r = 0; r < 16; r++) {
                            const float z = acc[r];
                            dst[(t * 32 + critic_acc_row(r, half)) * RS + col] = a.hidden_act == PACT_TANH ? tanhf(z) : fmaxf(z, 0.0f);
                        }
                    } else {
                        // output 0 is v; rows 1 .. 31 of the head's delta image are zeros whatever the padding multiplied
#pragma unroll
                        for (int r = 0; r < 16; r++) {
                            const int n = critic_acc_row(r, half);
                            dst[n * RS + col] = n == 0 ? acc[r] : 0.0f;
                        }
                    }
                }
                __syncthreads();
            }
        }
        // ---- per row: v, the loss term, c = R dL/dv in place of v
        if (tid < 32) {
            const float v = D0[col];
            float c = 0.0f;
            if (valid && a.stats) {
                const float ret = a.ret[ri];
                const float diff = __fsub_rn(v, ret);
                double term;
                bool active = true;
                if (a.loss == VLOSS_MSE) {
                    term = 0.5 * ((double) diff * (double) diff);
                } else {
                    const float vo = a.v_old[ri];
                    const float d = __fsub_rn(v, vo);
                    const float vc = __fadd_rn(vo, fminf(fmaxf(d, neg_eps), a.clip_eps));
                    const float dc = __fsub_rn(vc, ret);
                    const float e1 = __fmul_rn(diff, diff), e2 = __fmul_rn(dc, dc);
                    // (d > -eps and d < eps) or e1 >= e2, as selects (the two-clause form of such a predicate miscompiled in
                    // k_policy_grad: DESIGN.md 6.23); a NaN anywhere leaves the row inactive
                    const bool above = d > neg_eps, inside = above ? d < a.clip_eps : false;
                    const bool wins = e1 >= e2;
                    active = inside ? true : wins;
                    term = 0.5 * (double) fmaxf(e1, e2);
                }
                c = active ? diff : 0.0f;
                const double r64 = (double) ret, dr = r64 - (double) v;
                st[0] += 1.0;
                st[1] += term;
                st[2] += active ? 0.0 : 1.0;
                st[3] += dr * dr;
                st[4] += r64;
                st[5] += r64 * r64;
            }
            if (r_col < a.R && a.values) a.values[r_col] = valid ? v : 0.0f;
            D0[col] = c;
        }
        __syncthreads();
        if (!a.backward) continue;

        // ---- the backward, last layer first
        for (int l = nl - 1; l >= 0; l--) {
            const GradLayer L = a.layer[l];
            const float *Dc = ((nl - 1 - l) & 1) ? D1 : D0;
            float *Dn = ((nl - 1 - l) & 1) ? D0 : D1;
            const float *hin = l ? lds + a.layer[l ? l - 1 : 0].h_row0 * RS : X;
            const int np = L.ot * L.it;
            if constexpr (kSlots > 0) {
#pragma unroll
                for (int slot = 0; slot < kSlots; slot++) {
                    const int pl = slot * nw + wave - L.pair0;
                    if (pl >= 0 && pl < np) racc[slot] = critic_dw_tile(racc[slot], Dc, hin, pl / L.it, pl % L.it, col, half);
                }
            } else {
                for (int p = L.pair0 + (((wave - L.pair0) % nw) + nw) % nw; p < L.pair0 + np; p += nw) {
                    const int pl = p - L.pair0;
                    float *q = mypart + (size_t) p * 1024 + lane;
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; r++) acc[r] = q[r * 64];
                    acc = critic_dw_tile(acc, Dc, hin, pl / L.it, pl % L.it, col, half);
#pragma unroll
                    for (int r = 0; r < 16; r++) q[r * 64] = acc[r];
                }
            }
            for (int n = tid; n < L.ot * 32; n += kGradLanes) {
                float s = 0.0f;
                for (int e = 0; e < 32; e++) s = __fadd_rn(s, Dc[n * RS + e]);
                mybias[L.bias0 + n] = __fadd_rn(mybias[L.bias0 + n], s);
            }
            if (l > 0) {
                const int ld = L.it * 32, steps = (L.out + 1) >> 1;
                const float *hp = hin;
                for (int c = wave; c < L.it; c += nw) {
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
                    const float *wa = L.wrm + (size_t) half * ld + c * 32 + col;
                    const float *bs = Dc + half * RS + col;
                    for (int s = 0; s < steps; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[(size_t) 2 * s * ld], bs[2 * RS * s], acc, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int k = c * 32 + critic_acc_row(r, half);
                        const float h = hp[k * RS + col];
                        Dn[k * RS + col] = a.hidden_act == PACT_TANH ? __fmul_rn(acc[r], __fsub_rn(1.0f, __fmul_rn(h, h))) : (h > 0.0f ? acc[r] : 0.0f);
                    }
                }
            }
            __syncthreads();
        }
    }

    // ---- the workgroup's partials: the dW tiles a wave kept, the stats of its 32 row lanes in lane order
    if constexpr (kSlots > 0) {
        if (a.backward) {
#pragma unroll
            for (int slot = 0; slot < kSlots; slot++) {
                const int p = slot * nw + wave;
                if (p < a.n_pairs) {
#pragma unroll
                    for (int r = 0; r < 16; r++) mypart[((size_t) p * 16 + r) * 64 + lane] = racc[slot][r];
                }
            }
        }
    }
    if (!a.stats) return;
    __syncthreads();
    double *const red = (double *) Sc;  // (s_row0 is even: 8-byte aligned)
    if (tid < 32)
#pragma unroll
        for (int i = 0; i < kCriticStats; i++) red[i * 32 + tid] = st[i];
    __syncthreads();
    double *const p64 = a.part64 + (size_t) blockIdx.x * kCriticStats;
    if (tid < kCriticStats) {
        double s = 0.0;
        for (int e = 0; e < 32; e++) s += red[tid * 32 + e];
        p64[tid] = s;
    }
}

// the workgroups' partials, summed in f64 in block order, times 1 / R, rounded once: one lane per parameter in the trainer's layout
__global__ __launch_bounds__(256) void k_critic_merge(const CriticMergeArgs m) {
    const int64_t idx = (int64_t) blockIdx.x * 256 + threadIdx.x;
    const double R = (double) m.R;
    if (blockIdx.x == 0 && threadIdx.x < kCriticStats && m.stats) {
        const int i = (int) threadIdx.x;
        double s = 0.0;
        for (int b = 0; b < m.blocks; b++) s += m.part64[(size_t) b * kCriticStats + i];
        m.stats[i] = s;
    }
    if (!m.backward || idx >= m.param0[m.n_layers]) return;
    int l = 0;
    while (l + 1 < m.n_layers && idx >= m.param0[l + 1]) l++;
    const int64_t at = idx - m.param0[l];
    const int in = m.in[l], n = (int) (at / (in + 1)), k = (int) (at - (int64_t) n * (in + 1));
    float *dst = k < in ? (m.gW[l] ? m.gW[l] + (int64_t) n * in + k : nullptr) : (m.gb[l] ? m.gb[l] + n : nullptr);
    if (!dst) return;
    size_t off;
    if (k < in) {
        const int i = n & 31, r = (i & 3) + 4 * (i >> 3), hf = (i >> 2) & 1;
        off = ((size_t) (m.pair0[l] + (n >> 5) * m.it[l] + (k >> 5)) * 16 + r) * 64 + (k & 31) + 32 * hf;
    } else {
        off = (size_t) m.bias_base + m.bias0[l] + n;
    }
    double s = 0.0;
    for (int b = 0; b < m.blocks; b++) s += (double) m.part[(size_t) b * (size_t) m.part_floats + off];
    *dst = (float) __ddiv_rn(s, R);
}

int critic_prepare() {
    if (hipFuncSetAttribute((const void *) k_critic<0>, hipFuncAttributeMaxDynamicSharedMemorySize, kGradLdsBytes) != hipSuccess) return -1;
    if (hipFuncSetAttribute((const void *) k_critic<kGradRegSlots>, hipFuncAttributeMaxDynamicSharedMemorySize, kGradLdsBytes) != hipSuccess) return -1;
    return 0;
}

void launch_critic_values(const CriticArgs &a, int blocks, int lds_rows, hipStream_t stream) {
    const size_t lds_bytes = (size_t) lds_rows * kGradRowStride * sizeof(float);
    hipLaunchKernelGGL(k_critic<0>, dim3((unsigned) blocks), dim3(kGradLanes), lds_bytes, stream, a);
}

void launch_critic_grad(const CriticArgs &a, const CriticMergeArgs &m, int blocks, int lds_rows, bool in_registers, hipStream_t stream) {
    if (a.backward && a.n_layers > 1) hipLaunchKernelGGL(k_critic_wrm, dim3(64), dim3(256), 0, stream, a);
    const size_t lds_bytes = (size_t) lds_rows * kGradRowStride * sizeof(float);
    if (in_registers) hipLaunchKernelGGL(k_critic<kGradRegSlots>, dim3((unsigned) blocks), dim3(kGradLanes), lds_bytes, stream, a);
    else hipLaunchKernelGGL(k_critic<0>, dim3((unsigned) blocks), dim3(kGradLanes), lds_bytes, stream, a);
    const int64_t total = a.backward ? m.param0[m.n_layers] : 1;
    hipLaunchKernelGGL(k_critic_merge, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, stream, m);
}

}  // namespace chub
