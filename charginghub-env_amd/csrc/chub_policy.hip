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
//
// Sampling (the header's "sampling from the device actor") is a compile-time parameter of the same kernel: the argument block's type.
// k_policy<PolicyArgs> is the deterministic actor, instruction for instruction what it was before sampling existed;
// k_policy<PolicySampleArgs> runs the same chain to the pre-squash outputs and then, in the head, draws each pile from its logit and each
// Gaussian output around its mean with Philox noise under the policy's key and the tick of the handle's next launch.  A lane's sixteen
// accumulator rows are four runs of four consecutive rows from a multiple of four, so one Philox block serves each run with every word
// used.  The log-probability's terms are summed per lane, across the half-waves by a shuffle and across the waves through four LDS rows
// behind the two images, in wave order: no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "chub_policy.h"

namespace chub {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the step kernels' own predicate on an action: a pile is on iff a >= this ((a + 1) / 2 >= 0.5 in f32; kActOnThreshold of chub_kernels.hip)
constexpr float kPolicyOnThreshold = -2.98023223876953125e-8f;

// accumulator register r of lane l holds output row (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the tile, for env column l & 31
__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// ---- sampling (include/chub.h, "sampling from the device actor").  Philox4x32-10 and the tabulated normal are chub_kernels.hip's own
// (philox4x32_10, normal_from_word), restated here because the two files share no device header: the same rounds, the same tables.
struct PolicyU4 {
    uint32_t v[4];
};

__device__ __forceinline__ PolicyU4 policy_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const uint64_t p0 = (uint64_t) 0xD2511F53u * c0, p1 = (uint64_t) 0xCD9E8D57u * c2;
        const uint32_t h0 = (uint32_t) (p0 >> 32), l0 = (uint32_t) p0, h1 = (uint32_t) (p1 >> 32), l1 = (uint32_t) p1;
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    PolicyU4 r;
    r.v[0] = c0; r.v[1] = c1; r.v[2] = c2; r.v[3] = c3;
    return r;
}

// N(0,1) from one 32-bit word: 4096 cells of the inverse CDF, linear inside a cell; the outer 16 cells on either side through the second
// table with cells of 2^-20
__device__ __forceinline__ float policy_normal_from_word(const float *tz, const float *tl, uint32_t w) {
    const uint32_t cell = w >> 20;
    const bool hi = cell >= 4096u - 16u, lo = cell < 16u;
    const uint32_t m = hi ? ~w : w;
    const bool tail = hi || lo;
    const float *tab = tail ? tl : tz;
    const uint32_t idx = tail ? (m >> 12) : cell;
    const float frac = tail ? (float) (m & 0xFFFu) * (1.0f / 4096.0f) : (float) (w & 0xFFFFFu) * (1.0f / 1048576.0f);
    const float a = tab[idx], b = tab[idx + 1];
    const float z = __fadd_rn(a, __fmul_rn(__fsub_rn(b, a), frac));
    return hi ? -z : z;
}

constexpr float kHalfLn2Pi = 0.918938533204672742f;  // 0.5 ln 2 pi

// softplus(x) = max(x, 0) + log1pf(expf(-|x|))
__device__ __forceinline__ float policy_softplus(float x) { return __fadd_rn(fmaxf(x, 0.0f), log1pf(expf(-fabsf(x)))); }

// whether an argument block is a population's (Args::kPop, PolicyPopArgs only: the other blocks do not name the flag)
template <typename Args, typename = void>
struct PolicyIsPop {
    static constexpr bool value = false;
};
template <typename Args>
struct PolicyIsPop<Args, std::enable_if_t<Args::kPop>> {
    static constexpr bool value = true;
};

// Args = PolicyArgs: the deterministic actor.  Args = PolicyPopArgs: the same launch with the weights of the workgroup's member (a
// population: the chain, the order and the squash are the deterministic launch's; what differs is where w and b point and which tile
// of 32 envs a workgroup takes).  Args = PolicySampleArgs: the same chain to the pre-squash outputs z, then a draw from the actor's
// distribution, its log-probability and (if asked for) the raw feature row.  Args = PolicySampleSetArgs: the sampled launch with a
// pile's Bernoulli term added to the log-probability only where the pile's bit is in the env's set (one u32 word per accumulator tile); the
// draws, the outputs and the order of the terms that remain are the sampled launch's.
template <typename Args>
__global__ __launch_bounds__(64 * kPolicyMaxWaves) void k_policy(const Args a) {
    constexpr bool kSample = Args::kSample;
    [[maybe_unused]] constexpr bool kSet = Args::kSet;
    extern __shared__ float lds[];
    const int tid = (int) threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int) (blockDim.x >> 6), nt = (int) blockDim.x;
    const int col = lane & 31, half = lane >> 5;
    int64_t tile = (int64_t) blockIdx.x;
    if constexpr (PolicyIsPop<Args>::value) {
        // (a population) the dispatcher hands workgroup b to XCD b % 8, each with an L2 of its own: XCD x takes ONE contiguous eighth of
        // the tiles (xcd_order of chub_kernels.hip), so a member's tiles meet in one L2 and an XCD reads an eighth of the weights
        const uint32_t nb = gridDim.x, q = nb >> 3, r = nb & 7u, x = blockIdx.x & 7u;
        tile = (int64_t) (x * q + (x < r ? x : r) + (blockIdx.x >> 3));
    }
    const int64_t env0 = tile * kPolicyEnvTile;
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
                    if constexpr (kSample) {
                        if (a.features && (!a.mask || a.mask[env] != 0)) a.features[env * a.F + f0 + f] = x;
                    }
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
    [[maybe_unused]] int64_t member = 0;  // (a population) whose weights this workgroup's 32 envs are served with
    if constexpr (PolicyIsPop<Args>::value) member = tile / a.tiles_per_member;
    [[maybe_unused]] float logp = 0.0f;  // (sampling) this lane's terms: its rows of its wave's tiles, in ascending tile order

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
                if constexpr (PolicyIsPop<Args>::value) bt += member * a.b_stride[l];  // (a population: the block of the workgroup's member)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[r] = bt[(r & 3) + 8 * (r >> 2)];
                const float *wt = L.w + (size_t) t * (size_t) L.k_pad * kPolicyOutTile + lane;
                if constexpr (PolicyIsPop<Args>::value) wt += member * a.w_stride[l];
                const float *xs = src + lane;
                for (int s = 0; s < ksteps; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wt[64 * s], xs[64 * s], acc, 0, 0, 0);

                if (!last) {
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const float z = acc[r];
                        const float v = a.hidden_act == PACT_TANH ? tanhf(z) : fmaxf(z, 0.0f);
                        dst[(t * kPolicyOutTile + acc_row(r, half)) * kPolicyEnvTile + col] = v;
                    }
                } else if constexpr (kSample) {
                    // counter (block, site << 16 | kind, tick, global env id) under the policy's key: nothing of N, the mask or the tile enters
                    const uint32_t tick = a.tick + *a.tick_base, gid = a.gid0 + (uint32_t) env;
                    const bool piles = a.head == PHEAD_PILES;
                    const int g0 = piles ? a.S : 0;  // output g0 + i is Gaussian i
                    uint32_t m = 0u;
                    [[maybe_unused]] uint32_t in_set = 0u;  // (a pile set) the env's word of this tile: the piles whose terms count
                    if constexpr (kSet) {
                        if (piles && t < 2 * a.W && env < a.n_envs) in_set = a.set[env * (int64_t) (2 * a.W) + t];
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        // registers 4 q .. 4 q + 3 are four consecutive rows from a multiple of 4: the four words of one pile block
                        const int n0 = t * kPolicyOutTile + 8 * q + 4 * half;
                        PolicyU4 pb = {{0u, 0u, 0u, 0u}}, gb = {{0u, 0u, 0u, 0u}};
                        if (piles && n0 < a.S) pb = policy_philox4x32_10((uint32_t) (n0 >> 2), kPolicySite << 16, tick, gid, a.key[0], a.key[1]);
                        if (n0 + 3 >= g0 && n0 < g0 + a.G) gb = policy_philox4x32_10(0u, (kPolicySite << 16) | 1u, tick, gid, a.key[0], a.key[1]);
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const int n = n0 + j, i = n - g0;
                            const float z = acc[4 * q + j];
                            if (piles && n < a.S) {
                                const float U = (float) (pb.v[j] >> 8) * 5.9604644775390625e-8f;  // 2^-24: exact
                                const float p = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-z)));
                                const bool on = U < p;
                                if constexpr (kSet) {
                                    if ((in_set >> (n & 31)) & 1u) logp = __fsub_rn(logp, policy_softplus(on ? -z : z));
                                } else {
                                    logp = __fsub_rn(logp, policy_softplus(on ? -z : z));
                                }
                                if (on) m |= 1u << (n & 31);
                                if (store && a.actions) a.actions[env * a.A + n] = on ? 1.0f : -1.0f;
                            } else if (i >= 0 && i < a.G) {
                                const uint32_t w = i == 0 ? gb.v[0] : i == 1 ? gb.v[1] : i == 2 ? gb.v[2] : gb.v[3];
                                const float eps = policy_normal_from_word(a.normal_icdf, a.normal_tail, w);
                                const float ls = a.log_std[i];
                                const float u = __fadd_rn(z, __fmul_rn(expf(ls), eps));
                                const float v = a.squash == PSQ_TANH ? tanhf(u) : fminf(fmaxf(u, -1.0f), 1.0f);
                                logp = __fadd_rn(logp, __fsub_rn(__fsub_rn(__fmul_rn(-0.5f, __fmul_rn(eps, eps)), ls), kHalfLn2Pi));
                                if (store) {
                                    if (a.u) a.u[env * a.G + i] = u;
                                    if (piles) {
                                        if (a.actions) a.actions[env * a.A + n] = v;
                                        if (a.tail) a.tail[env * 2 + i] = v;
                                    } else if (i < 2) {
                                        a.loads[env * 2 + i] = v;
                                    } else {
                                        a.tail[env * 2 + (i - 2)] = v;
                                    }
                                }
                            }
                        }
                    }
                    if (piles && a.bits) {
                        m |= (uint32_t) __shfl_xor((int) m, 32);
                        if (store && half == 0 && t < 2 * a.W) a.bits[env * (int64_t) (2 * a.W) + t] = m;
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

    if constexpr (kSample) {
        // an env's log-probability: the two half-waves by a shuffle, then the waves' partials in wave order through LDS.  No atomics: the
        // order is the same for every env and every launch of this policy
        logp = __fadd_rn(logp, __shfl_xor(logp, 32));
        float *const R = lds + (size_t) a.r_row0 * kPolicyEnvTile;
        if (half == 0) R[wave * kPolicyEnvTile + col] = logp;
        __syncthreads();
        if (tid < kPolicyEnvTile) {
            float s = R[col];
            for (int w = 1; w < nw; w++) s = __fadd_rn(s, R[w * kPolicyEnvTile + col]);
            if (store) a.logp[env] = s;
        }
    }
}

// rows of the Q image: it ends where the widest even hidden layer does
static int policy_q_rows(const PolicyArgs &a) {
    int q_rows = 0;
    for (int l = 0; l + 1 < a.n_layers; l += 2) q_rows = a.layer[l].tiles * kPolicyOutTile > q_rows ? a.layer[l].tiles * kPolicyOutTile : q_rows;
    return q_rows;
}

void launch_policy(const PolicyArgs &a, int waves, hipStream_t stream) {
    if (a.n_envs <= 0) return;
    const int64_t nb = (a.n_envs + kPolicyEnvTile - 1) / kPolicyEnvTile;
    const size_t lds_bytes = (size_t) (a.q_row0 + policy_q_rows(a)) * kPolicyEnvTile * sizeof(float);
    hipLaunchKernelGGL(k_policy<PolicyArgs>, dim3((unsigned) nb), dim3(64u * (unsigned) waves), lds_bytes, stream, a);
}

// a population's launch: the deterministic launch's grid and LDS (the caller has checked that N = P tiles_per_member 32)
void launch_policy_pop(const PolicyPopArgs &a, int waves, hipStream_t stream) {
    if (a.n_envs <= 0) return;
    const int64_t nb = (a.n_envs + kPolicyEnvTile - 1) / kPolicyEnvTile;
    const size_t lds_bytes = (size_t) (a.q_row0 + policy_q_rows(a)) * kPolicyEnvTile * sizeof(float);
    hipLaunchKernelGGL(k_policy<PolicyPopArgs>, dim3((unsigned) nb), dim3(64u * (unsigned) waves), lds_bytes, stream, a);
}

// the sampled launch: the same grid, kPolicyLogpRows more rows of LDS behind the two images (the caller has checked that they fit)
void launch_policy_sample(const PolicySampleArgs &a, int waves, hipStream_t stream) {
    if (a.n_envs <= 0) return;
    const int64_t nb = (a.n_envs + kPolicyEnvTile - 1) / kPolicyEnvTile;
    PolicySampleArgs s = a;
    s.r_row0 = a.q_row0 + policy_q_rows(a);
    const size_t lds_bytes = (size_t) (s.r_row0 + kPolicyLogpRows) * kPolicyEnvTile * sizeof(float);
    hipLaunchKernelGGL(k_policy<PolicySampleArgs>, dim3((unsigned) nb), dim3(64u * (unsigned) waves), lds_bytes, stream, s);
}

void launch_policy_sample_set(const PolicySampleSetArgs &a, int waves, hipStream_t stream) {
    if (a.n_envs <= 0) return;
    const int64_t nb = (a.n_envs + kPolicyEnvTile - 1) / kPolicyEnvTile;
    PolicySampleSetArgs s = a;
    s.r_row0 = a.q_row0 + policy_q_rows(a);
    const size_t lds_bytes = (size_t) (s.r_row0 + kPolicyLogpRows) * kPolicyEnvTile * sizeof(float);
    hipLaunchKernelGGL(k_policy<PolicySampleSetArgs>, dim3((unsigned) nb), dim3(64u * (unsigned) waves), lds_bytes, stream, s);
}

// ---- running feature statistics (include/chub.h, "running feature statistics"; the lane layout is chub_policy.h's MomentsArgs).
// Launch 1 streams the rows: consecutive lanes read consecutive floats of a row, a lane keeps kAhead passes in flight, converts to f64,
// subtracts its column's pivot and adds d and d d to its own sums.  The loop has no branch around a load: a row that does not count (past
// R, or of a masked-out env) is NOT read -- its lane reads row 0 instead, the pivot row every call reads, and a select drops the value -- so
// every load of a pass is issued before the first is waited for.  (With the loads under per-row branches the compiler waited for each
// before issuing the next: a third of the rate)  The lanes of a workgroup that share a column then meet in LDS as a
// tree over the row index (row r + h joins row r, h = the power of two halving down: a fixed order), and the workgroup writes one row
// of partials.  Launch 2 adds the partials and merges.  No atomics anywhere: every sum's order is a function of (R, F, the grid) alone.
// kMask: a mask is given (the bytes of a pass are loaded first, the rows they admit next); kTwo: F > 256, two columns per lane.
template <int kAhead, bool kMask, bool kTwo>
__global__ __launch_bounds__(kMomentsLanes) void k_moments(const MomentsArgs a) {
    __shared__ double red[3][kMomentsLanes];
    const int tid = (int) threadIdx.x, L = a.L, RW = a.RW, F = a.F;
    const int r_in = tid / L, c = tid - r_in * L;
    const bool on = r_in < RW, two = kTwo && c + L < F;  // (two columns per lane only where F > 256: L = 256, RW = 1)
    const double n0 = a.state[0];
    double K0 = 0.0, K1 = 0.0;
    if (on) {
        K0 = n0 > 0.0 ? a.state[1 + c] : (double) a.x[c];
        if (two) K1 = n0 > 0.0 ? a.state[1 + c + L] : (double) a.x[c + L];
        if (blockIdx.x == 0 && r_in == 0) {
            a.pivot[1 + c] = K0;
            if (two) a.pivot[1 + c + L] = K1;
            if (c == 0) a.pivot[0] = n0;
        }
    }
    double s1a = 0.0, s2a = 0.0, s1b = 0.0, s2b = 0.0, cnt = 0.0;
    if (on) {
        const int64_t G = a.blocks, N = a.n_envs;
        // the lane's row and its offset move by one grid of passes per load: additions only
        const int64_t row_step = G * RW, q_step = row_step * a.ld;
        const int c1 = two ? L : 0;  // (the second column's offset; a lane without one reads its first again)
        int64_t row = (int64_t) blockIdx.x * RW + r_in, off = row * a.ld + c;
        [[maybe_unused]] int64_t e = kMask ? row % N : 0;
        for (int64_t p = blockIdx.x; p < a.passes; p += G * kAhead) {
            bool ok[kAhead];
            float va[kAhead];
            [[maybe_unused]] float vb[kAhead];
            [[maybe_unused]] uint8_t m[kAhead];
#pragma unroll
            for (int k = 0; k < kAhead; k++) {
                ok[k] = row + k * row_step < a.R;
                if constexpr (kMask) {
                    m[k] = a.mask[e];  // (e < N whatever the row)
                    e += a.e_step;
                    if (e >= N) e -= N;
                }
            }
#pragma unroll
            for (int k = 0; k < kAhead; k++) {
                if constexpr (kMask) ok[k] = ok[k] && m[k] != 0;
                const float *q = a.x + (ok[k] ? off + k * q_step : (int64_t) c);
                va[k] = q[0];
                if constexpr (kTwo) vb[k] = q[c1];
            }
            row += kAhead * row_step;
            off += kAhead * q_step;
#pragma unroll
            for (int k = 0; k < kAhead; k++) {
                const double d = ok[k] ? (double) va[k] - K0 : 0.0;
                s1a += d;
                s2a += d * d;
                if constexpr (kTwo) {
                    const double d1 = ok[k] && two ? (double) vb[k] - K1 : 0.0;
                    s1b += d1;
                    s2b += d1 * d1;
                }
                cnt += ok[k] ? 1.0 : 0.0;
            }
        }
    }
    if (RW > 1) {  // (uniform) the lanes of a column, rows 0 .. RW - 1 of the pass: a tree over the row index
        red[0][tid] = s1a; red[1][tid] = s2a; red[2][tid] = cnt;
        __syncthreads();
        int h = 1;
        while (h < RW) h <<= 1;
        for (h >>= 1; h > 0; h >>= 1) {
            if (r_in < h && r_in + h < RW) {
#pragma unroll
                for (int i = 0; i < 3; i++) red[i][tid] += red[i][tid + h * L];
            }
            __syncthreads();
        }
        s1a = red[0][tid]; s2a = red[1][tid]; cnt = red[2][tid];
    }
    if (on && r_in == 0) {
        double *p = a.partials + (size_t) blockIdx.x * (size_t) (1 + 2 * F);
        p[1 + c] = s1a;
        p[1 + F + c] = s2a;
        if (two) {
            p[1 + c + L] = s1b;
            p[1 + F + c + L] = s2b;
        }
        if (c == 0) p[0] = cnt;
    }
}

// the partials of `blocks` workgroups into the state: a workgroup takes kMomentsMergeCols columns; its lane group g adds the partials of
// blocks [blocks g / 8, blocks (g + 1) / 8) in ascending order, the groups meet in LDS in ascending g, and group 0 merges (Chan et al.).
// n and the pivots come from launch 1's copy: the lane that writes the state's n races nobody who reads it.
__global__ __launch_bounds__(kMomentsLanes) void k_moments_merge(const double *partials, int blocks, const double *pivot, double *state, int F) {
    constexpr int kGroups = kMomentsLanes / kMomentsMergeCols;
    __shared__ double red[3][kGroups][kMomentsMergeCols];
    const int tid = (int) threadIdx.x, cl = tid % kMomentsMergeCols, g = tid / kMomentsMergeCols;
    const int col = (int) blockIdx.x * kMomentsMergeCols + cl;
    const bool live = col < F;
    const size_t stride = (size_t) (1 + 2 * F);
    double c = 0.0, s1 = 0.0, s2 = 0.0;
    if (live) {
        const int b1 = (int) ((int64_t) blocks * (g + 1) / kGroups);
#pragma unroll 8
        for (int b = (int) ((int64_t) blocks * g / kGroups); b < b1; b++) {
            const double *p = partials + (size_t) b * stride;
            c += p[0];
            s1 += p[1 + col];
            s2 += p[1 + F + col];
        }
    }
    red[0][g][cl] = c; red[1][g][cl] = s1; red[2][g][cl] = s2;
    __syncthreads();
    if (g != 0 || !live) return;
    c = s1 = s2 = 0.0;
#pragma unroll
    for (int j = 0; j < kGroups; j++) {
        c += red[0][j][cl]; s1 += red[1][j][cl]; s2 += red[2][j][cl];
    }
    if (!(c > 0.0)) return;  // nobody counted: the state is left alone
    const double n = pivot[0], K = pivot[1 + col];
    const double t = s2 - (s1 * s1) / c;
    const double m2b = t < 0.0 ? 0.0 : t;  // (a NaN stays one)
    const double n1 = n + c;
    double mean, m2;
    if (n > 0.0) {
        const double db = s1 / c;
        mean = K + s1 / n1;
        m2 = (state[1 + F + col] + m2b) + (db * db) * ((n * c) / n1);
    } else {
        mean = K + s1 / c;
        m2 = m2b;
    }
    state[1 + col] = mean;
    state[1 + F + col] = m2;
    if (col == 0) state[0] = n1;
}

void launch_moments(const MomentsArgs &a, double *state, hipStream_t stream) {
    const dim3 grid((unsigned) a.blocks), block(kMomentsLanes);
    constexpr int kA = kMomentsAhead;
    if (a.mask && a.F > kMomentsLanes) hipLaunchKernelGGL((k_moments<kA, true, true>), grid, block, 0, stream, a);
    else if (a.mask) hipLaunchKernelGGL((k_moments<kA, true, false>), grid, block, 0, stream, a);
    else if (a.F > kMomentsLanes) hipLaunchKernelGGL((k_moments<kA, false, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((k_moments<kA, false, false>), grid, block, 0, stream, a);
    hipLaunchKernelGGL(k_moments_merge, dim3((unsigned) ((a.F + kMomentsMergeCols - 1) / kMomentsMergeCols)), dim3(kMomentsLanes), 0, stream,
                       (const double *) a.partials, (int) a.blocks, (const double *) a.pivot, state, (int) a.F);
}

// the policy's normaliser from a moments state, every f64 operation rounded once (IEEE division and square root); n == 0: nothing is written
__global__ void k_normalizer_from_moments(const double *state, int F, double eps, float *mean32, float *inv_std32) {
    const int f = (int) (blockIdx.x * blockDim.x + threadIdx.x);
    const double n = state[0];
    if (f >= F || !(n > 0.0)) return;
    mean32[f] = (float) state[1 + f];
    inv_std32[f] = (float) __ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(__ddiv_rn(state[1 + F + f], n), eps)));
}

void launch_normalizer_from_moments(const double *state, int F, double eps, float *mean32, float *inv_std32, hipStream_t stream) {
    hipLaunchKernelGGL(k_normalizer_from_moments, dim3((unsigned) ((F + 63) / 64)), dim3(64), 0, stream, state, F, eps, mean32, inv_std32);
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

// the way back: one layer in the kernel's layout -> W [out][in], b [out]; one lane per element of [W | b]
__global__ void k_policy_unlayout(const float *w, const float *bias, float *W, float *b, int out, int in, int k_pad) {
    const int64_t idx = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t) out * (in + 1)) return;
    const int n = (int) (idx / (in + 1)), k = (int) (idx - (int64_t) n * (in + 1));
    if (k < in) W[(int64_t) n * in + k] = w[((int64_t) (n >> 5) * k_pad + k) * kPolicyOutTile + (n & 31)];
    else b[n] = bias[n];
}

void launch_policy_unlayout(const float *d_w, const float *d_bias, float *d_W, float *d_b, int out, int in, int k_pad, hipStream_t stream) {
    const int64_t total = (int64_t) out * (in + 1);
    hipLaunchKernelGGL(k_policy_unlayout, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, stream, d_w, d_bias, d_W, d_b, out, in, k_pad);
}

// ---- a population's weights (include/chub.h, "a population of actors"; the lane layout is chub_policy.h's PopLayerArgs)
constexpr int kPopLanes = 256;

__device__ __forceinline__ PolicyU4 population_block(const PopLayerArgs &a, int row, int group, uint32_t pair) {
    return policy_philox4x32_10(((uint32_t) row << 8) | (uint32_t) group, (kPopulationSite << 16) | (uint32_t) a.layer, a.generation, pair, a.key[0],
                                a.key[1]);
}

// Lane (pair j, tile t, column group g, row i of the tile), i fastest: consecutive lanes write consecutive words of [k][32].  ONE Philox
// block gives the lane's four columns of both members of the pair; d = sigma eps is rounded once, theta + d and theta - d once each.
// Rows beyond `out` and the column beyond `in` of an odd layer are written as zeros: noise there would act as extra hidden units
__global__ __launch_bounds__(kPopLanes) void k_population_perturb(const PopLayerArgs a, const float *W, const float *b, int device_layout, float sigma) {
    const int groups = a.in / 4 + 1;
    const int64_t idx = (int64_t) blockIdx.x * kPopLanes + threadIdx.x;
    if (idx >= (int64_t) a.pairs * a.tiles * groups * kPolicyOutTile) return;
    const int i = (int) (idx & 31);
    int64_t q = idx >> 5;
    const int g = (int) (q % groups);
    q /= groups;
    const int t = (int) (q % a.tiles), j = (int) (q / a.tiles);
    const int row = t * kPolicyOutTile + i;
    const bool live = row < a.out;
    PolicyU4 blk = {{0u, 0u, 0u, 0u}};
    if (live) blk = population_block(a, row, g, (uint32_t) j);
    float *const w0 = a.w + (int64_t) (2 * j) * a.stride + (int64_t) t * a.k_pad * kPolicyOutTile + i, *const w1 = w0 + a.stride;
    float *const b0 = a.bias + (int64_t) (2 * j) * a.stride + row, *const b1 = b0 + a.stride;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int k = 4 * g + c;
        float plus = 0.0f, minus = 0.0f;
        if (live && k <= a.in) {
            float theta;
            if (k == a.in) theta = b[row];
            else theta = device_layout ? W[((int64_t) t * a.k_pad + k) * kPolicyOutTile + i] : W[(int64_t) row * a.in + k];
            const float d = __fmul_rn(sigma, policy_normal_from_word(a.normal_icdf, a.normal_tail, blk.v[c]));
            plus = __fadd_rn(theta, d);
            minus = __fsub_rn(theta, d);
        }
        if (k < a.k_pad) {
            w0[(int64_t) k * kPolicyOutTile] = k < a.in ? plus : 0.0f;
            w1[(int64_t) k * kPolicyOutTile] = k < a.in ? minus : 0.0f;
        }
        if (k == a.in) {
            *b0 = plus;
            *b1 = minus;
        }
    }
}

void launch_population_perturb(const PopLayerArgs &a, const float *W, const float *b, int device_layout, float sigma, hipStream_t stream) {
    const int64_t total = (int64_t) a.pairs * a.tiles * (a.in / 4 + 1) * kPolicyOutTile;
    hipLaunchKernelGGL(k_population_perturb, dim3((unsigned) ((total + kPopLanes - 1) / kPopLanes)), dim3(kPopLanes), 0, stream, a, W, b, device_layout,
                       sigma);
}

// The ES gradient estimate.  Launch 1: lane (chunk c = blockIdx.y, item = row groups + column group) regenerates the block of every pair
// of its chunk in ascending j and adds du_j eps to four f64 sums, product and sum each rounded once.  Launch 2: one lane per parameter adds
// the chunks' sums in ascending c, rounds once to f32 and stores in the trainer's layout.  No atomics: the order is a function of
// (P, the layer's shape, the chunk size) alone
__global__ __launch_bounds__(kPopLanes) void k_population_es_partial(const PopLayerArgs a, const float *util, int chunk_pairs, double *partials) {
    const int groups = a.in / 4 + 1, items = a.out * groups;
    const int item = (int) (blockIdx.x * kPopLanes + threadIdx.x), c = (int) blockIdx.y;
    if (item >= items) return;
    const int row = item / groups, g = item - row * groups;
    const int j0 = c * chunk_pairs, j1 = j0 + chunk_pairs < a.pairs ? j0 + chunk_pairs : a.pairs;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = j0; j < j1; j++) {
        const double du = __dsub_rn((double) util[2 * j], (double) util[2 * j + 1]);
        const PolicyU4 blk = population_block(a, row, g, (uint32_t) j);
#pragma unroll
        for (int w = 0; w < 4; w++)
            s[w] = __dadd_rn(s[w], __dmul_rn(du, (double) policy_normal_from_word(a.normal_icdf, a.normal_tail, blk.v[w])));
    }
    double *p = partials + ((int64_t) c * items + item) * 4;
#pragma unroll
    for (int w = 0; w < 4; w++) p[w] = s[w];
}

__global__ __launch_bounds__(kPopLanes) void k_population_es_merge(const double *partials, int chunks, float *gW, float *gb, int out, int in) {
    const int64_t idx = (int64_t) blockIdx.x * kPopLanes + threadIdx.x;
    if (idx >= (int64_t) out * (in + 1)) return;
    const int groups = in / 4 + 1;
    const int row = (int) (idx / (in + 1)), k = (int) (idx - (int64_t) row * (in + 1));
    const int64_t items = (int64_t) out * groups, at = ((int64_t) row * groups + (k >> 2)) * 4 + (k & 3);
    double s = 0.0;
    for (int c = 0; c < chunks; c++) s = __dadd_rn(s, partials[(int64_t) c * items * 4 + at]);
    if (k < in) gW[(int64_t) row * in + k] = (float) s;
    else gb[row] = (float) s;
}

void launch_population_es_gradient(const PopLayerArgs &a, const float *d_util, int chunk_pairs, int chunks, double *partials, float *gW, float *gb,
                                   hipStream_t stream) {
    const int items = a.out * (a.in / 4 + 1);
    hipLaunchKernelGGL(k_population_es_partial, dim3((unsigned) ((items + kPopLanes - 1) / kPopLanes), (unsigned) chunks), dim3(kPopLanes), 0, stream, a,
                       d_util, chunk_pairs, partials);
    const int64_t total = (int64_t) a.out * (a.in + 1);
    hipLaunchKernelGGL(k_population_es_merge, dim3((unsigned) ((total + kPopLanes - 1) / kPopLanes)), dim3(kPopLanes), 0, stream,
                       (const double *) partials, chunks, gW, gb, a.out, a.in);
}

// lane x takes float x of every member named: first every source into its column of the staging rows, then every destination from there.
// A lane meets no other lane's floats, so one launch reads all sources before it writes any destination (a swap is a swap)
__global__ __launch_bounds__(kPopLanes) void k_population_copy(float *params, float *stage, int64_t member_floats, int P, const int32_t *src,
                                                               const int32_t *dst, int count) {
    const int64_t x = (int64_t) blockIdx.x * kPopLanes + threadIdx.x;
    if (x >= member_floats) return;
    for (int i = 0; i < count; i++) {
        const int32_t s = src[i], d = dst[i];
        if (s >= 0 && s < P && d >= 0 && d < P) stage[(int64_t) i * member_floats + x] = params[(int64_t) s * member_floats + x];
    }
    for (int i = 0; i < count; i++) {
        const int32_t s = src[i], d = dst[i];
        if (s >= 0 && s < P && d >= 0 && d < P) params[(int64_t) d * member_floats + x] = stage[(int64_t) i * member_floats + x];
    }
}

void launch_population_copy(float *params, float *stage, int64_t member_floats, int P, const int32_t *d_src, const int32_t *d_dst, int count,
                            hipStream_t stream) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_population_copy, dim3((unsigned) ((member_floats + kPopLanes - 1) / kPopLanes)), dim3(kPopLanes), 0, stream, params, stage,
                       member_floats, P, d_src, d_dst, count);
}

// ---- actor gradients (include/chub.h, "actor gradients on the device"; the images and the partials' layout are chub_policy.h's)
//
// Per tile of 32 rows: gather through d_rows and normalise into X; the forward as k_policy runs it (the same A operand from the same device
// layout, the same k order from the bias), every hidden layer into an image of its own; the head's z into delta image 0 while each lane adds
// its rows' log-probability and entropy terms (the waves meet in LDS in wave order, as in k_policy); 32 lanes form the rows' advantage,
// ratio, loss term and the coefficient c = dL R / dlogp; the head's lanes turn z into delta z in place; then per layer, last to first,
// dW += delta h^T and db += delta 1 over the tile's 32 rows and delta_in = (W^T delta) act'(h) into the other delta image.
// One MFMA form serves all three products (v_mfma_f32_32x32x2_f32, lane l gives A[l & 31][l >> 5] and B[l >> 5][l & 31]):
//   forward   C[out][row] : A = w[t][2 s + half][out]          B = h_in[2 s + half][row]      k = input
//   W^T delta C[in][row]  : A = wrm[2 s + half][32 c + in]      B = delta[2 s + half][row]     k = output
//   dW        C[out][in]  : A = delta[32 t + out][2 s + half]   B = h_in[32 c + in][2 s + half] k = row of the tile
// kSlots > 0: a wave's dW tiles (pair p belongs to wave p % 4, slot p / 4) stay in registers for the whole walk; kSlots == 0: they are
// read from and written to the workgroup's own slice of the partials around each tile's sixteen MFMAs, by the lane that owns them.
__device__ __forceinline__ float grad_sigmoid(float z) { return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-z))); }

__global__ void k_policy_grad_wrm(const PolicyGradArgs a) {
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

__device__ __forceinline__ f32x16 grad_dw_tile(f32x16 acc, const float *delta, const float *hin, int t, int c, int col, int half) {
    constexpr int RS = kGradRowStride;
    const float *as = delta + (t * 32 + col) * RS + half, *bs = hin + (c * 32 + col) * RS + half;
#pragma unroll
    for (int s = 0; s < 16; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[2 * s], bs[2 * s], acc, 0, 0, 0);
    return acc;
}

template <int kSlots>
__global__ __launch_bounds__(kGradLanes) void k_policy_grad(const PolicyGradArgs a) {
    constexpr int RS = kGradRowStride, nw = kGradWaves;
    extern __shared__ float lds[];
    const int tid = (int) threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    float *const X = lds;
    float *const D0 = lds + a.d_row0[0] * RS, *const D1 = lds + a.d_row0[1] * RS;
    float *const Sc = lds + a.s_row0 * RS;
    int64_t *const rowi = (int64_t *) (Sc + (kGradScratchRows - 2) * RS);  // (the last two scratch rows; s_row0 is even: 8-byte aligned)
    const int nl = a.n_layers;
    const bool piles = a.head == PHEAD_PILES;
    const int g0 = piles ? a.S : 0;
    float *const mypart = a.part + (size_t) blockIdx.x * (size_t) a.part_floats;
    float *const mybias = mypart + (size_t) a.n_pairs * 1024;

    // the advantage's normaliser: mean and 1 / sqrt(var + 1e-8) in f64, every operation rounded once, each rounded once to f32
    float m32 = 0.0f, s32 = 1.0f;
    if (a.adv_stats) {
        const double cnt = a.adv_stats[0], m = __ddiv_rn(a.adv_stats[1], cnt);
        double var = __dsub_rn(__ddiv_rn(a.adv_stats[2], cnt), __dmul_rn(m, m));
        var = var > 0.0 ? var : 0.0;
        m32 = (float) m;
        s32 = (float) __ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(var, 1e-8)));
    }
    const float ratio_lo = __fsub_rn(1.0f, a.clip_eps), ratio_hi = __fadd_rn(1.0f, a.clip_eps);

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
    double st[kGradStats] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gls = 0.0;

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
        // ---- the feature rows of the tile, normalised with the policy's current normaliser, as [feature][row]
        for (int idx = tid; idx < 32 * a.F; idx += kGradLanes) {
            const int j = idx / a.F, f = idx - j * a.F;
            const int64_t ri = rowi[j];
            float x = 0.0f;
            if (ri >= 0) {
                x = a.features[ri * a.ld + f];
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
        float logp = 0.0f, ent = 0.0f;
#pragma unroll
        for (int l = 0; l < kPolicyMaxLayers; l++) {
            if (l < nl) {
                const GradLayer L = a.layer[l];
                const bool last = l == nl - 1;
                const float *src = l ? lds + a.layer[l ? l - 1 : 0].h_row0 * RS : X;
                float *dst = last ? D0 : lds + L.h_row0 * RS;
                const int ksteps = L.k_pad >> 1;
                for (int t = wave; t < L.ot; t += nw) {
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
                            dst[(t * 32 + acc_row(r, half)) * RS + col] = a.hidden_act == PACT_TANH ? tanhf(z) : fmaxf(z, 0.0f);
                        }
                    } else {
                        uint32_t on_w = 0u, set_w = 0xFFFFFFFFu;
                        if (piles && valid && t < 2 * a.W) {
                            on_w = a.pile_bits[ri * (int64_t) (2 * a.W) + t];
                            if (a.set_bits) set_w = a.set_bits[ri * (int64_t) (2 * a.W) + t];
                        }
#pragma unroll
                        for (int r = 0; r < 16; r++) {
                            const int n = t * 32 + acc_row(r, half), i = n - g0;
                            const float z = acc[r];
                            dst[n * RS + col] = z;
                            if (!valid) continue;
                            if (piles && n < a.S) {
                                if ((set_w >> (n & 31)) & 1u) {
                                    const bool on = (on_w >> (n & 31)) & 1u;
                                    logp = __fsub_rn(logp, policy_softplus(on ? -z : z));
                                    ent = __fadd_rn(ent, __fsub_rn(policy_softplus(z), __fmul_rn(z, grad_sigmoid(z))));
                                }
                            } else if (i >= 0 && i < a.G) {
                                const float ls = a.log_std[i];
                                const float eps = __fdiv_rn(__fsub_rn(a.u[ri * a.G + i], z), expf(ls));
                                logp = __fadd_rn(logp, __fsub_rn(__fsub_rn(__fmul_rn(-0.5f, __fmul_rn(eps, eps)), ls), kHalfLn2Pi));
                                ent = __fadd_rn(ent, __fadd_rn(__fadd_rn(0.5f, ls), kHalfLn2Pi));
                            }
                        }
                    }
                }
                if (!last) __syncthreads();
            }
        }
        // ---- a row's log-probability and entropy: the half-waves by a shuffle, the waves in wave order through LDS
        logp = __fadd_rn(logp, __shfl_xor(logp, 32));
        ent = __fadd_rn(ent, __shfl_xor(ent, 32));
        if (half == 0) {
            Sc[wave * RS + col] = logp;
            Sc[(nw + wave) * RS + col] = ent;
        }
        __syncthreads();
        if (tid < 32) {
            float lp = Sc[col], en = Sc[nw * RS + col];
            for (int w = 1; w < nw; w++) {
                lp = __fadd_rn(lp, Sc[w * RS + col]);
                en = __fadd_rn(en, Sc[(nw + w) * RS + col]);
            }
            float c = 0.0f;
            if (valid) {
                float A = a.adv[ri];
                if (a.adv_stats) A = __fmul_rn(__fsub_rn(A, m32), s32);
                float term;
                if (a.loss == PLOSS_COEF) {
                    c = -A;
                    term = __fsub_rn(-__fmul_rn(A, lp), __fmul_rn(a.ent_coef, en));
                } else {
                    const float lo = a.logp_old[ri];
                    const float ratio = expf(__fsub_rn(lp, lo));
                    const float rc = fminf(fmaxf(ratio, ratio_lo), ratio_hi);
                    const float surr = fminf(__fmul_rn(ratio, A), __fmul_rn(rc, A));
                    term = __fsub_rn(-surr, __fmul_rn(a.ent_coef, en));
                    // (A >= 0 and ratio < 1 + eps) or (A < 0 and ratio > 1 - eps), as two selects: written as the two-clause predicate the
                    // compiler's gfx950 code zeroed c in every lane of the second clause; a NaN advantage is inactive
                    const bool up = A >= 0.0f, inside = up ? ratio < ratio_hi : ratio > ratio_lo;
                    const bool active = inside && A == A;
                    const float nar = -__fmul_rn(A, ratio);
                    c = active ? nar : 0.0f;
                    st[3] += (double) lo - (double) lp;
                    st[4] += active ? 0.0 : 1.0;
                    st[5] += (double) ratio;
                }
                st[0] += 1.0;
                st[1] += (double) term;
                st[2] += (double) en;
            }
            if (r_col < a.R) {
                if (a.logp_new) a.logp_new[r_col] = valid ? lp : 0.0f;
                if (a.entropy) a.entropy[r_col] = valid ? en : 0.0f;
            }
            Sc[2 * nw * RS + col] = c;
            Sc[(2 * nw + 1) * RS + col] = valid ? -a.ent_coef : 0.0f;
        }
        __syncthreads();
        if (!a.backward) continue;

        // ---- the head's delta z, in place of z
        {
            const GradLayer L = a.layer[nl - 1];
            const float c = Sc[2 * nw * RS + col], ec = Sc[(2 * nw + 1) * RS + col];
            for (int t = wave; t < L.ot; t += nw) {
                uint32_t on_w = 0u, set_w = 0xFFFFFFFFu;
                if (piles && valid && t < 2 * a.W) {
                    on_w = a.pile_bits[ri * (int64_t) (2 * a.W) + t];
                    if (a.set_bits) set_w = a.set_bits[ri * (int64_t) (2 * a.W) + t];
                }
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int n = t * 32 + acc_row(r, half), i = n - g0;
                    const float z = D0[n * RS + col];
                    float d = 0.0f;
                    if (valid && piles && n < a.S) {
                        if ((set_w >> (n & 31)) & 1u) {
                            const float sg = grad_sigmoid(z), on = ((on_w >> (n & 31)) & 1u) ? 1.0f : 0.0f;
                            const float dh = -__fmul_rn(__fmul_rn(z, sg), __fsub_rn(1.0f, sg));
                            d = __fadd_rn(__fmul_rn(c, __fsub_rn(on, sg)), __fmul_rn(ec, dh));
                        }
                    } else if (valid && i >= 0 && i < a.G) {
                        const float sd = expf(a.log_std[i]);
                        const float eps = __fdiv_rn(__fsub_rn(a.u[ri * a.G + i], z), sd);
                        d = __fmul_rn(c, __fdiv_rn(eps, sd));
                        Sc[(2 * nw + 2 + i) * RS + col] = __fadd_rn(__fmul_rn(c, __fsub_rn(__fmul_rn(eps, eps), 1.0f)), ec);
                    } else if (!valid && i >= 0 && i < a.G) {
                        Sc[(2 * nw + 2 + i) * RS + col] = 0.0f;
                    }
                    D0[n * RS + col] = d;
                }
            }
        }
        __syncthreads();
        if (tid < a.G)
            for (int e = 0; e < 32; e++) gls += (double) Sc[(2 * nw + 2 + tid) * RS + e];

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
                    if (pl >= 0 && pl < np) racc[slot] = grad_dw_tile(racc[slot], Dc, hin, pl / L.it, pl % L.it, col, half);
                }
            } else {
                for (int p = L.pair0 + (((wave - L.pair0) % nw) + nw) % nw; p < L.pair0 + np; p += nw) {
                    const int pl = p - L.pair0;
                    float *q = mypart + (size_t) p * 1024 + lane;
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; r++) acc[r] = q[r * 64];
                    acc = grad_dw_tile(acc, Dc, hin, pl / L.it, pl % L.it, col, half);
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
                        const int k = c * 32 + acc_row(r, half);
                        const float h = hp[k * RS + col];
                        Dn[k * RS + col] = a.hidden_act == PACT_TANH ? __fmul_rn(acc[r], __fsub_rn(1.0f, __fmul_rn(h, h))) : (h > 0.0f ? acc[r] : 0.0f);
                    }
                }
            }
            __syncthreads();
        }
    }

    // ---- the workgroup's partials: the dW tiles a wave kept, the stats of its 32 row lanes in lane order, the log_std sums
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
    __syncthreads();
    double *const red = (double *) Sc;  // (s_row0 is even: 8-byte aligned)
    if (tid < 32)
#pragma unroll
        for (int i = 0; i < kGradStats; i++) red[i * 32 + tid] = st[i];
    __syncthreads();
    double *const p64 = a.part64 + (size_t) blockIdx.x * kGradPart64;
    if (tid < kGradStats) {
        double s = 0.0;
        for (int e = 0; e < 32; e++) s += red[tid * 32 + e];
        p64[tid] = s;
    }
    if (tid < 4) p64[kGradStats + tid] = tid < a.G ? gls : 0.0;  // (lane i < G summed log_std term i)
}

// the workgroups' partials, summed in f64 in block order, times 1 / R, rounded once: one lane per parameter in the trainer's layout
__global__ __launch_bounds__(256) void k_policy_grad_merge(const GradMergeArgs m) {
    const int64_t idx = (int64_t) blockIdx.x * 256 + threadIdx.x;
    const double R = (double) m.R;
    if (blockIdx.x == 0 && threadIdx.x < kGradPart64) {
        const int i = (int) threadIdx.x;
        double s = 0.0;
        for (int b = 0; b < m.blocks; b++) s += m.part64[(size_t) b * kGradPart64 + i];
        if (i < kGradStats) {
            if (m.stats) m.stats[i] = s;
        } else if (m.backward && m.glog_std && i - kGradStats < m.G) {
            m.glog_std[i - kGradStats] = (float) __ddiv_rn(s, R);
        }
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

int policy_grad_prepare() {
    if (hipFuncSetAttribute((const void *) k_policy_grad<0>, hipFuncAttributeMaxDynamicSharedMemorySize, kGradLdsBytes) != hipSuccess) return -1;
    if (hipFuncSetAttribute((const void *) k_policy_grad<kGradRegSlots>, hipFuncAttributeMaxDynamicSharedMemorySize, kGradLdsBytes) != hipSuccess) return -1;
    return 0;
}

void launch_policy_grad(const PolicyGradArgs &a, const GradMergeArgs &m, int blocks, int lds_rows, bool in_registers, hipStream_t stream) {
    if (a.backward && a.n_layers > 1) hipLaunchKernelGGL(k_policy_grad_wrm, dim3(64), dim3(256), 0, stream, a);
    const size_t lds_bytes = (size_t) lds_rows * kGradRowStride * sizeof(float);
    if (in_registers) hipLaunchKernelGGL(k_policy_grad<kGradRegSlots>, dim3((unsigned) blocks), dim3(kGradLanes), lds_bytes, stream, a);
    else hipLaunchKernelGGL(k_policy_grad<0>, dim3((unsigned) blocks), dim3(kGradLanes), lds_bytes, stream, a);
    const int64_t total = a.backward ? m.param0[m.n_layers] : 1;
    hipLaunchKernelGGL(k_policy_grad_merge, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, stream, m);
}

}  // namespace chub
