// chub_trainlog.hip -- a training log and a KL stop on the device (include/chub.h): three small launches that fold the stats blocks of a
// minibatch's gradient calls and optimiser steps into one block of f64 words and set the gate word the optimiser steps honour.  The
// arithmetic is chub_trainlog.h's, which the host form runs too.  Each launch is ONE workgroup: the log is read and written by lane 0
// alone (the fold is a chain of thirty dependent words), so no launch reads what another of its workgroups writes, and there are no
// atomics.  Built with -ffp-contract=off: every f64 operation is one rounded operation.
#include "chub_trainlog.h"

namespace chub {

// a lane per word; lane 0 clears the gate as well
__global__ __launch_bounds__(kTrainLogLanes) void k_trainlog_begin(double *words, int64_t *gate) {
    const int lane = threadIdx.x;
    if (lane < TLOG_WORDS) words[lane] = lane == TLOG_STOP_INDEX ? -1.0 : 0.0;
    if (lane == 0) *gate = 0;
}

__global__ __launch_bounds__(kTrainLogLanes) void k_trainlog_record(double *words, int64_t *gate, const double *pstats, const double *cstats, int kl_kind,
                                                                    double kl_limit) {
    if (threadIdx.x == 0) trainlog_record(words, gate, pstats, cstats, kl_kind, kl_limit);
}

__global__ __launch_bounds__(kTrainLogLanes) void k_trainlog_steps(double *words, const double *astats_actor, const double *astats_critic) {
    if (threadIdx.x == 0) trainlog_step(words + TLOG_ACTOR_OPT, astats_actor);
    if (threadIdx.x == 1) trainlog_step(words + TLOG_CRITIC_OPT, astats_critic);  // (the two optimisers' words are disjoint)
}

void launch_trainlog_begin(double *words, int64_t *gate, hipStream_t stream) {
    hipLaunchKernelGGL(k_trainlog_begin, dim3(1), dim3(kTrainLogLanes), 0, stream, words, gate);
}

void launch_trainlog_record(double *words, int64_t *gate, const double *pstats, const double *cstats, int kl_kind, double kl_limit, hipStream_t stream) {
    hipLaunchKernelGGL(k_trainlog_record, dim3(1), dim3(kTrainLogLanes), 0, stream, words, gate, pstats, cstats, kl_kind, kl_limit);
}

void launch_trainlog_steps(double *words, const double *astats_actor, const double *astats_critic, hipStream_t stream) {
    hipLaunchKernelGGL(k_trainlog_steps, dim3(1), dim3(kTrainLogLanes), 0, stream, words, astats_actor, astats_critic);
}

}  // namespace chub
