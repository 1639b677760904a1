"""CPU tests of the pair rule of chub_run_steps (chub_pair_plan, csrc/chub_plan.h: plan_pair_handle, plan_pair_call, pair_steps) -- which
handles send pairs of steps out with one tail launch, in which calls, and how many steps of a call go out as pairs -- and of the fact
tests/test_gpu_pair_tails.py builds its long-queue case on.  Expected values are worked out by hand from the rule, not recomputed from it."""
import ctypes as C

import numpy as np
import pytest

import orclib

HANDLE, CALL, STEPS = 0, 1, 2  # CHUB_PAIR_* (include/chub.h)
COMM, PER_ENV, TAPE, OUTPUTS, PROFILING = 1, 2, 4, 8, 16  # CHUB_PAIRF_*


def pair_plan_rc(stations, n_envs, rng="philox", env_params=0, flags=0, t=0, left=96, **options):
    import charginghub_env_amd as m
    from charginghub_env_amd import _lib
    lib = m.load_library()
    cfg = m.make_config(list(stations), ["fast", "slow"])
    opt = _lib.ChubOptions()
    for k, v in options.items():
        setattr(opt, k, v)
    out = (C.c_int64 * 3)()
    rc = lib.chub_pair_plan(C.byref(cfg), n_envs, _lib.RNG_MODES[rng], C.byref(opt), env_params, flags, t, left, out)
    return rc, list(out), lib.chub_last_error()


def pair_plan(*a, **kw):
    rc, out, err = pair_plan_rc(*a, **kw)
    assert rc == 0, err
    return out


@pytest.mark.parametrize("n_envs, on", [(8191, 0), (8192, 1), (65536, 1)])
def test_size_threshold(n_envs, on):
    # [64, 64]: 4 envs per workgroup of the small tile, the one-launch step up to 768 workgroups = 3072 envs: two launches at these sizes
    p = pair_plan([64, 64], n_envs)
    assert p[HANDLE] == on


@pytest.mark.parametrize("n_envs, on", [(8448, 0), (8449, 1), (32768, 1), (65536, 1)])
def test_default_hub_pairs_where_the_step_is_two_launches(n_envs, on):
    # [20, 25]: 11 envs per workgroup, the one-launch step up to 768 workgroups = 8448 envs (whose spans are one launch already)
    assert pair_plan([20, 25], n_envs)[HANDLE] == on


def test_forced_on_and_off_at_any_size():
    # chub_options.span_steps bounds the steps per tail launch of a handle on the two-launch step: 1 = never, 2 and more = at any size
    assert pair_plan([20, 25], 300, fused_step=1, span_steps=2)[HANDLE] == 1
    assert pair_plan([20, 25], 300, fused_step=1, span_steps=7)[HANDLE] == 1
    assert pair_plan([20, 25], 300, fused_step=1)[HANDLE] == 0
    assert pair_plan([20, 25], 300, span_steps=2)[HANDLE] == 0    # 28 workgroups: the one-launch step, whose spans are one launch already
    assert pair_plan([20, 25], 65536, span_steps=1)[HANDLE] == 0
    assert pair_plan([20, 25], 65536, fused_step=2)[HANDLE] == 0  # the one-launch step forced


def test_only_the_small_tile_of_the_packed_kernel():
    assert pair_plan([20, 25], 233016)[HANDLE] == 1   # 10 485 720 slots: the small tile still
    assert pair_plan([20, 25], 233017)[HANDLE] == 0   # the large tile
    assert pair_plan([20, 25], 65536, tile=2, span_steps=2)[HANDLE] == 0
    assert pair_plan([20, 25], 65536, slot_kernel=1, span_steps=2)[HANDLE] == 0  # the wave-local slot kernel
    assert pair_plan([100, 25], 65536, span_steps=2)[HANDLE] == 0   # a station of more than 64 piles
    assert pair_plan([20, 25], 65536, rng="compat", span_steps=2)[HANDLE] == 0
    assert pair_plan([20, 25], 65536, rng="philox_curves", span_steps=2)[HANDLE] == 0
    assert pair_plan([20, 25], 65536, env_params=1)[HANDLE] == 0  # per-env hub parameters: the tail reads each env's constants
    assert pair_plan([20, 25], 65536, env_params=1, span_steps=2)[HANDLE] == 0


@pytest.mark.parametrize("flag", [COMM, PER_ENV, TAPE, OUTPUTS, PROFILING])
def test_calls_that_keep_the_per_step_path(flag):
    assert pair_plan([20, 25], 65536)[CALL] == 1
    out = pair_plan([20, 25], 65536, flags=flag)
    assert out[HANDLE] == 1 and out[CALL] == 0 and out[STEPS] == 0


@pytest.mark.parametrize("t, left, steps", [(0, 96, 96), (0, 1, 0), (0, 2, 2), (0, 3, 2), (7, 96, 88), (7, 4, 4), (94, 96, 2), (95, 96, 0), (93, 96, 2),
                                            (0, 0, 0), (10, 1000, 86)])
def test_pairs_never_straddle_the_day_or_the_call(t, left, steps):
    # from slot t of the day, `left` steps asked for: whole pairs up to the day's end (96 - t steps) or the call's, whichever comes first
    assert pair_plan([20, 25], 65536, t=t, left=left)[STEPS] == steps


def test_the_long_queue_case_reaches_queues_above_four():
    """tests/test_gpu_pair_tails.py, hub [2, 2], seed 31, global env 0: the queues in front of steps 5, 7, 9, 11 and 13 of the first day hold more
    than 4 cars.  Step 5 is the second step of a pair where the span starts the day (the graph test), steps 7, 9, 11 and 13 in the program of
    spans (pairs (6, 7), (8, 9), (10, 11), (12, 13)): their draws are decoded from the raw form, with queue positions 4 .. 9 looked at"""
    cfg = orclib.make_config(piles=(2, 2), types=("fast", "slow"), fcev_permeate=0.02, renew_fluctuate=0.2, price_fluctuate=0.1)
    e = orclib.OrcEnv(cfg)
    e.seed_philox(31, 0)
    e.reset()
    lines = {}
    for i in range(13):  # steps 0 .. 12
        e.step(np.zeros(6, dtype=np.float32))
        t = e.telemetry()
        lines[i + 1] = (int(t[31]), int(t[36]))  # CHUB_T_LINE0, CHUB_T_LINE1: Station::line of both stations in front of step i + 1
    assert [lines[i] for i in (5, 7, 9, 11, 13)] == [(8, 5), (8, 4), (8, 4), (7, 5), (5, 5)]
