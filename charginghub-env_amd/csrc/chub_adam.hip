// chub_adam.hip -- an optimiser on the device (include/chub.h): the Adam step on a policy's or a critic's LIVE device weights, and the
// counter-based row shuffle.  The definitions are include/chub.h's; the argument blocks and the shuffle's arithmetic are chub_adam.h's.
// Built with -ffp-contract=off: every f64 operation below is one rounded operation, as the definition says.
#include "chub_adam.h"

namespace chub {

// where entry i of the flat parameter vector lives: its weight in the kernels' layout, its gradient in the trainer's
struct AdamSlot {
    float *theta;
    const float *g;
    bool decays;  // an entry of a W
};

__device__ __forceinline__ AdamSlot adam_slot(const AdamArgs &a, int64_t i) {
    AdamSlot s;
    if (i >= a.param0[a.n_layers]) {
        const int64_t j = i - a.param0[a.n_layers];
        s.theta = a.log_std + j;
        s.g = a.glog_std + j;
        s.decays = false;
        return s;
    }
    int l = 0;
    while (l + 1 < a.n_layers && i >= a.param0[l + 1]) l++;
    const int off = (int) (i - a.param0[l]), in = a.in[l], nw = a.out[l] * in;
    if (off < nw) {
        const int o = off / in, k = off - o * in;
        s.theta = a.w[l] + ((int64_t) (o >> 5) * a.k_pad[l] + k) * kPolicyOutTile + (o & 31);
        s.g = a.gW[l] + off;
        s.decays = true;
    } else {
        s.theta = a.b[l] + (off - nw);
        s.g = a.gb[l] + (off - nw);
        s.decays = false;
    }
    return s;
}

// launch 1: partials[c] = the sum of g^2 over chunk c.  A lane adds its four entries in ascending order from 0, the 256 lanes meet in
// a tree over LDS (lane j += lane j + 128, then + 64, .. + 1): the order is a function of n alone.  Lane 0 of workgroup 0 copies t, p1, p2
// for the step launch, which reads the copy while it writes the originals
__global__ __launch_bounds__(kAdamLanes) void k_adam_norm(const AdamArgs a) {
    __shared__ double red[kAdamLanes];
    const int lane = threadIdx.x;
    if (blockIdx.x == 0 && lane == 0) {
        reinterpret_cast<int64_t *>(a.scalars)[ADAM_PREV_T] = reinterpret_cast<const int64_t *>(a.scalars)[ADAM_T];
        a.scalars[ADAM_PREV_P1] = a.scalars[ADAM_P1];
        a.scalars[ADAM_PREV_P2] = a.scalars[ADAM_P2];
    }
    for (int c = blockIdx.x; c < a.chunks; c += gridDim.x) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < kAdamPerLane; j++) {
            const int64_t i = (int64_t) c * kAdamChunk + j * kAdamLanes + lane;
            double gg = 0.0;
            if (i < a.n) {
                const double g = (double) *adam_slot(a, i).g;
                gg = g * g;
            }
            s = s + gg;
        }
        red[lane] = s;
        __syncthreads();
        for (int stride = kAdamLanes / 2; stride > 0; stride >>= 1) {
            if (lane < stride) red[lane] = red[lane] + red[lane + stride];
            __syncthreads();
        }
        if (lane == 0) a.partials[c] = red[0];
        __syncthreads();  // (red is written again in the next trip)
    }
}

// launch 2: every lane adds the chunks' partials in ascending order and forms the step's scalars from the COPY of t, p1, p2; lane 0 of
// workgroup 0 alone writes the new ones.  Then a lane owns one real parameter: it finds its place in the layout, reads it, writes it
__global__ __launch_bounds__(kAdamLanes) void k_adam_step(const AdamArgs a) {
    double sumsq = 0.0;
    for (int c = 0; c < a.chunks; c++) sumsq = sumsq + a.partials[c];
    const double norm = __dsqrt_rn(sumsq);
    const double *sc = a.scalars;
    const int64_t t0 = reinterpret_cast<const int64_t *>(sc)[ADAM_PREV_T];
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    const bool held = a.gate != nullptr && *a.gate != 0;  // (every workgroup reads the word: all of them return, or none)
    if (held || !isfinite(norm)) {  // held back or skipped: nothing but the stats is written
        if (first && a.stats) {
            a.stats[0] = (double) t0;
            a.stats[1] = norm;
            a.stats[2] = 0.0;
            a.stats[3] = held ? 2.0 : 1.0;
        }
        return;
    }
    const double lr = sc[ADAM_LR], beta1 = sc[ADAM_BETA1], beta2 = sc[ADAM_BETA2], eps = sc[ADAM_EPS], wd = sc[ADAM_WEIGHT_DECAY],
                 max_norm = sc[ADAM_MAX_GRAD_NORM];
    float scale = 1.0f;
    if (max_norm != 0.0) {
        const double r = max_norm / (norm + 1e-6);
        scale = (float) (r < 1.0 ? r : 1.0);
    }
    const int64_t t = t0 + 1;
    const double p1 = sc[ADAM_PREV_P1] * beta1, p2 = sc[ADAM_PREV_P2] * beta2;
    if (first) {
        reinterpret_cast<int64_t *>(a.scalars)[ADAM_T] = t;
        a.scalars[ADAM_P1] = p1;
        a.scalars[ADAM_P2] = p2;
        if (a.stats) {
            a.stats[0] = (double) t;
            a.stats[1] = norm;
            a.stats[2] = (double) scale;
            a.stats[3] = 0.0;
        }
    }
    const double omb1 = 1.0 - beta1, omb2 = 1.0 - beta2;
    const double step = lr / (1.0 - p1), root2 = __dsqrt_rn(1.0 - p2), keep = 1.0 - lr * wd;
    const double s64 = (double) scale;
    for (int c = blockIdx.x; c < a.chunks; c += gridDim.x) {
#pragma unroll
        for (int j = 0; j < kAdamPerLane; j++) {
            const int64_t i = (int64_t) c * kAdamChunk + j * kAdamLanes + threadIdx.x;
            if (i >= a.n) continue;
            const AdamSlot s = adam_slot(a, i);
            const double g = (double) *s.g * s64;  // (24 x 24 bits: exact)
            const float m32 = (float) (beta1 * (double) a.m[i] + omb1 * g);
            const float v32 = (float) (beta2 * (double) a.v[i] + omb2 * (g * g));
            a.m[i] = m32;
            a.v[i] = v32;
            const double denom = __dsqrt_rn((double) v32) / root2 + eps;
            double th = (double) *s.theta;
            if (s.decays && wd != 0.0) th = th * keep;
            th = th - step * ((double) m32 / denom);
            *s.theta = (float) th;
        }
    }
}

__global__ __launch_bounds__(kAdamLanes) void k_adam_reset(float *m, float *v, int64_t n, double *scalars) {
    for (int64_t i = (int64_t) blockIdx.x * kAdamLanes + threadIdx.x; i < n; i += (int64_t) gridDim.x * kAdamLanes) {
        m[i] = 0.0f;
        v[i] = 0.0f;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        reinterpret_cast<int64_t *>(scalars)[ADAM_T] = 0;
        scalars[ADAM_P1] = 1.0;
        scalars[ADAM_P2] = 1.0;
    }
}

void launch_adam_step(const AdamArgs &a, int norm_blocks, int step_blocks, hipStream_t stream) {
    hipLaunchKernelGGL(k_adam_norm, dim3((unsigned) norm_blocks), dim3(kAdamLanes), 0, stream, a);
    hipLaunchKernelGGL(k_adam_step, dim3((unsigned) step_blocks), dim3(kAdamLanes), 0, stream, a);
}

void launch_adam_reset(float *m, float *v, int64_t n, double *scalars, hipStream_t stream) {
    int64_t nb = (n + kAdamLanes - 1) / kAdamLanes;
    if (nb > kAdamMaxBlocks) nb = kAdamMaxBlocks;
    hipLaunchKernelGGL(k_adam_reset, dim3((unsigned) nb), dim3(kAdamLanes), 0, stream, m, v, n, scalars);
}

// one lane per row r; c = *counter + offset is read on the device, so a replayed graph follows the counter
__global__ __launch_bounds__(kShuffleLanes) void k_shuffle_rows(uint64_t key, const int64_t *counter, int64_t offset, int64_t R, int nb, int64_t *rows) {
    const uint64_t c = (counter ? (uint64_t) *counter : 0ull) + (uint64_t) offset;
    for (int64_t r = (int64_t) blockIdx.x * kShuffleLanes + threadIdx.x; r < R; r += (int64_t) gridDim.x * kShuffleLanes)
        rows[r] = shuffle_row(r, R, nb, key, c);
}

void launch_shuffle_rows(uint64_t key, const int64_t *d_counter, int64_t offset, int64_t R, int64_t *d_rows, hipStream_t stream) {
    int64_t nb = (R + kShuffleLanes - 1) / kShuffleLanes;
    if (nb > kShuffleMaxBlocks) nb = kShuffleMaxBlocks;
    hipLaunchKernelGGL(k_shuffle_rows, dim3((unsigned) nb), dim3(kShuffleLanes), 0, stream, key, d_counter, offset, R, shuffle_bits(R), d_rows);
}

}  // namespace chub
