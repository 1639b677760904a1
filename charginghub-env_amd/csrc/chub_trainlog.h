// chub_trainlog.h -- what the training log's kernels (chub_trainlog.hip) and the host (chub_runtime.cpp) share: the words of include/chub.h's
// section "a training log and a KL stop on the device" and the fold's arithmetic, which the kernels and the host form
// (chub_train_log_fold) both run.  Every f64 operation below is one rounded operation (-ffp-contract=off).
#ifndef CHUB_TRAINLOG_H
#define CHUB_TRAINLOG_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace chub {

// the words of the log (include/chub.h's CHUB_TLOG_*, restated; chub_runtime.cpp asserts that they agree)
enum TrainLogWord {
    TLOG_COUNTED = 0,       // minibatches counted
    TLOG_AFTER_STOP = 1,    // minibatches recorded after the stop (not counted)
    TLOG_STOPPED = 2,       // 0 / 1
    TLOG_STOP_INDEX = 3,    // the record call that set the stop, from 0; -1: none
    TLOG_ACTOR = 4,         // [6] sums of the actor's stats
    TLOG_KL_MAX = 10,
    TLOG_KL_LAST = 11,
    TLOG_CRITIC = 12,       // [6] sums of the critic's stats
    TLOG_ACTOR_OPT = 18,    // [6] taken, skipped, held back, sum of norms, largest norm, steps with scale < 1
    TLOG_CRITIC_OPT = 24,   // [6] the same
    TLOG_WORDS = 30
};
enum TrainLogKl { KL_K1 = 0, KL_K3, KL_COUNT };
constexpr int kTrainLogGradStats = 6;  // a gradient call's stats block
constexpr int kTrainLogStepStats = 4;  // an optimiser step's: t, norm, scale, 0 taken / 1 skipped / 2 held back
constexpr int kTrainLogLanes = 64;     // every launch is one workgroup of one wave

__host__ __device__ inline void trainlog_begin(double *w, int64_t *gate) {
    for (int i = 0; i < TLOG_WORDS; i++) w[i] = 0.0;
    w[TLOG_STOP_INDEX] = -1.0;
    *gate = 0;
}

// the KL estimate of a minibatch from the actor's stats (rows, loss terms, entropies, sum (logp_old - logp_new), clipped rows, sum of ratios)
__host__ __device__ inline double trainlog_kl(const double *ps, int kind) {
    if (!ps) return 0.0;
    const double n = ps[0];
    if (n == 0.0) return 0.0;
    const double k1 = ps[3] / n;
    if (kind == KL_K1) return k1;
    return (ps[5] / n - 1.0) + k1;
}

// one minibatch, after its two gradient calls and before its steps
__host__ __device__ inline void trainlog_record(double *w, int64_t *gate, const double *ps, const double *cs, int kind, double kl_limit) {
    if (w[TLOG_STOPPED] != 0.0) {
        w[TLOG_AFTER_STOP] = w[TLOG_AFTER_STOP] + 1.0;
        return;
    }
    const double kl = trainlog_kl(ps, kind), index = w[TLOG_COUNTED];
    if (ps)
        for (int i = 0; i < kTrainLogGradStats; i++) w[TLOG_ACTOR + i] = w[TLOG_ACTOR + i] + ps[i];
    if (cs)
        for (int i = 0; i < kTrainLogGradStats; i++) w[TLOG_CRITIC + i] = w[TLOG_CRITIC + i] + cs[i];
    if (index == 0.0 || kl > w[TLOG_KL_MAX]) w[TLOG_KL_MAX] = kl;  // (the first counted minibatch sets it: a K1 estimate may be negative)
    w[TLOG_KL_LAST] = kl;
    w[TLOG_COUNTED] = index + 1.0;
    if (kl_limit > 0.0 && !(kl <= kl_limit)) {  // (a NaN estimate stops)
        w[TLOG_STOPPED] = 1.0;
        w[TLOG_STOP_INDEX] = index;
        *gate = 1;
    }
}

// one optimiser's six words after its step; st: that step's stats block
__host__ __device__ inline void trainlog_step(double *w6, const double *st) {
    if (!st) return;
    const double norm = st[1], scale = st[2], how = st[3];
    if (how == 0.0) {
        w6[0] = w6[0] + 1.0;
        if (scale < 1.0) w6[5] = w6[5] + 1.0;
    } else if (how == 1.0) {
        w6[1] = w6[1] + 1.0;
    } else {
        w6[2] = w6[2] + 1.0;
    }
    if (__builtin_isfinite(norm)) {
        w6[3] = w6[3] + norm;
        if (norm > w6[4]) w6[4] = norm;
    }
}

// one launch each, one workgroup each, on `stream`
void launch_trainlog_begin(double *words, int64_t *gate, hipStream_t stream);
void launch_trainlog_record(double *words, int64_t *gate, const double *pstats, const double *cstats, int kl_kind, double kl_limit, hipStream_t stream);
void launch_trainlog_steps(double *words, const double *astats_actor, const double *astats_critic, hipStream_t stream);

}  // namespace chub
#endif
