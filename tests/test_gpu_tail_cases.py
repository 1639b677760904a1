"""The production (PHILOX) per-env tail on its rare branches, in every form it is compiled in.

tests/tail_cases_lib.py designs a population of 96 envs (six hub configurations in blocks of 16, one hub shape [64, 64] fast) and a script
of tail actions that takes the tail to the brim of the tank, to a fuel cell short of hydrogen or at fc_max_power, to the grid clamp that
wraps to full power, to a hub without an electrolyser; tests/test_tail_cases_cpu.py asserts on the oracle that it does.  Here:

  against the CPU oracle (one trajectory, computed once), with the bars of test_gpu_parity._philox_parity -- slots and station scalars [:6]
  bit for bit, telemetry 19:24 and 28:38 bit for bit, the other columns, obs_f64 and reward_f64 at relative 1e-9 (telemetry absolute 1e-7),
  done equal, f32 obs within 1e-6 absolute:
    the handle with per-env rows (chub_create_params: k_env<.., ENV_PARAMS>), six homogeneous handles on the two-launch step (k_slot_packed +
    k_env), on the one-launch step (k_step_tailwave) and on the wave-local slot kernel;
  the device against itself, bit for bit:
    chub_run_steps's spans (k_steps_fused, k_steps_piped, every step a launch) against the eager one-launch step; chub_step_bits_device (the
    tail actions arrive through d_tail) against chub_step; every step through a device mask of ones (k_env<.., MULTI>) against lock-step;
    telemetry off (the CHUB_TEL stores skipped: what the benchmark runs) against telemetry on.

A failing comparison names the config, the step, the env and the branches the oracle took on that env-step."""
import ctypes as C
import functools

import numpy as np
import pytest

import tail_cases_lib as tc

pytestmark = pytest.mark.gpu

TIGHT = 1e-9
K = len(tc.CONFIGS)
STEPS = sum(tc.PLAN)
ONE_LAUNCH, SPAN_SIZE_OK, SPAN_PIPED = 6, 7, 8  # CHUB_PLAN_* (include/chub.h)
ALL = np.arange(tc.N)


def hub():
    import charginghub_env_amd as chub
    return chub


def block(k):
    return np.arange(k * tc.BLOCK, (k + 1) * tc.BLOCK)


@functools.lru_cache(maxsize=None)
def oracle():
    return tc.oracle_trajectory()


def where(i, env):
    """config, step, env and branch flags of env-step (i, env); i = None: a reset"""
    name = tc.NAMES[tc.config_of(env)]
    if i is None:
        return "config %s, env %d" % (name, env)
    ep, t = (0, i) if i < tc.PLAN[0] else (1, i - tc.PLAN[0])
    return "config %s, step %d (episode %d, step %d), env %d (local %d), branches %s" % (name, i, ep, t, env, env % tc.BLOCK, tc.flags_of(oracle().flags, (i, env)))


def no_bad(bad, i, envs, what, got=None, want=None):
    """bad: [len(envs), ...] bool -- names the first env-step that differs"""
    bad = np.asarray(bad).reshape(len(envs), -1)
    rows = np.nonzero(bad.any(axis=1))[0]
    if rows.size:
        j = rows[0]
        detail = "" if got is None else "; got %s, want %s" % (np.asarray(got)[j].reshape(-1)[bad[j]][:6], np.asarray(want)[j].reshape(-1)[bad[j]][:6])
        raise AssertionError("%s differs at %s (%d envs of this call differ)%s" % (what, where(i, int(envs[j])), rows.size, detail))


def same_bits(got, want, i, envs, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    no_bad(got.view(u) != want.view(u), i, envs, what, got, want)


def near(got, want, i, envs, what, rtol, atol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    no_bad(~np.isclose(got, want, rtol=rtol, atol=atol), i, envs, what, got, want)


def plan_of(kw, n, rows=False, **options):
    chub = hub()
    from charginghub_env_amd import _lib
    cfg = chub.make_config(kw["station_list"], kw["station_type_list"],
                           **{f: v for f, v in kw.items() if f not in ("station_list", "station_type_list")})
    opt = _lib.ChubOptions()
    for f, v in options.items():
        setattr(opt, f, v)
    out = (C.c_int32 * 16)()
    fn = chub.load_library().chub_launch_plan_params if rows else chub.load_library().chub_launch_plan
    assert fn(C.byref(cfg), n, _lib.RNG_PHILOX, C.byref(opt), out) == 0
    return list(out)


# ---- the handles: one with rows (96 envs), or six homogeneous ones (16 envs each at ENV_ID0 + 16 k)
def make_rows(**options):
    v = hub().VecChargingHub(tc.N, seed=tc.SEED, rng="philox", env_id0=tc.ENV_ID0, **tc.HUB, **tc.rows(), **options)
    assert v.has_env_params and not v.uses_fused_step and v.uses_packed_kernel
    assert plan_of(dict(tc.HUB), tc.N, rows=True)[ONE_LAUNCH] == 0
    return [(v, ALL)]


FORM_OPTIONS = {"two_launch": dict(fused_step="off"), "one_launch": dict(fused_step="on"), "wave": dict(slot_kernel="wave")}
FORM_PLAN = {"two_launch": (dict(fused_step=1), 0), "one_launch": (dict(fused_step=2), 2), "wave": (dict(slot_kernel=1), 0)}  # CHUB_PLAN_ONE_LAUNCH


def make_homogeneous(form, **options):
    out = []
    for k, (name, kw) in enumerate(tc.configs()):
        v = hub().VecChargingHub(tc.BLOCK, seed=tc.SEED, rng="philox", env_id0=tc.ENV_ID0 + tc.BLOCK * k, **kw, **FORM_OPTIONS[form], **options)
        # the form that was meant is the form that runs: a threshold that moved must not turn two forms into one
        assert not v.has_env_params
        assert v.uses_fused_step == (form == "one_launch"), (form, name)
        assert v.uses_packed_kernel == (form != "wave"), (form, name)
        opt, one = FORM_PLAN[form]
        assert plan_of(kw, tc.BLOCK, **opt)[ONE_LAUNCH] == one, (form, name)  # (2: k_step_tailwave -- 4 envs of 128 piles per workgroup)
        out.append((v, block(k)))
    return out


def make(form, **options):
    return make_rows(**options) if form == "rows" else make_homogeneous(form, **options)


def close_all(handles):
    for v, _ in handles:
        v.close()


# ---- device against the oracle
def against_oracle_reset(v, envs, ep):
    tr = oracle()
    near(v.obs_f64(), tr.reset_obs[ep, envs], None, envs, "reset %d: obs_f64" % ep, TIGHT, TIGHT)
    same_bits(v.station_scalars()[:, :, :6], tr.reset_scalars[ep, envs][:, :, :6], None, envs, "reset %d: station scalars" % ep)


def against_oracle_step(v, envs, i, obs, rew, done):
    tr = oracle()
    sl = v.slots()
    for k in (0, 1):
        same_bits(sl[k], tr.slots[k][i, envs], i, envs, "slots of station %d" % k)
    same_bits(v.station_scalars()[:, :, :6], tr.scalars[i, envs][:, :, :6], i, envs, "station scalars")
    tel, want = v.telemetry(), tr.tel[i, envs]
    same_bits(tel[:, 19:24], want[:, 19:24], i, envs, "telemetry 19:24 (forecourt, days)")
    same_bits(tel[:, 28:38], want[:, 28:38], i, envs, "telemetry 28:38 (station scalars)")
    for c in list(range(19)) + list(range(24, 28)):
        near(tel[:, c], want[:, c], i, envs, "telemetry column %d (%s)" % (c, tc.T_NAMES[c]), TIGHT, 1e-7)
    same_bits(np.asarray(done, dtype=bool), tr.done[i, envs], i, envs, "done")
    near(v.obs_f64(), tr.obs[i, envs], i, envs, "obs_f64", TIGHT, TIGHT)
    near(v.reward_f64(), tr.reward[i, envs], i, envs, "reward_f64", TIGHT, TIGHT)
    near(obs, tr.obs[i, envs], i, envs, "f32 obs", 0.0, 1e-6)
    near(rew, tr.reward[i, envs], i, envs, "f32 reward", 1e-6, 1e-6)  # (the f32 narrowing of a reward held to 1e-9 above)


def run_against_oracle(handles):
    for v, _ in handles:
        v.set_telemetry(True)
    for ep, t, i in tc.step_plan():
        if t == 0:
            for v, envs in handles:
                v.reset()
                against_oracle_reset(v, envs, ep)
        act = tc.actions(i)
        for v, envs in handles:
            obs, rew, done, _ = v.step(act[envs])
            against_oracle_step(v, envs, i, obs, rew, done)
    close_all(handles)


def test_handle_with_rows_matches_oracle():
    """chub_create_params, 96 envs: k_slot_packed + k_env<.., ENV_PARAMS>, every env on its own row"""
    run_against_oracle(make_rows())


@pytest.mark.parametrize("form", ["two_launch", "one_launch", "wave"])
def test_homogeneous_handles_match_oracle(form):
    """six handles of 16 envs: k_slot_packed + k_env / k_step_tailwave / the wave-local slot kernel + k_env"""
    run_against_oracle(make_homogeneous(form))


# ---- device against device, bit for bit
def end_state(v):
    t, ticks = v.env_clocks(ticks=True)
    return [("slots", np.concatenate([x.reshape(v.n_envs, -1) for x in v.slots()], axis=1)), ("station scalars", v.station_scalars().reshape(v.n_envs, -1)),
            ("clocks", t), ("ticks", ticks)]


def same_end_state(a, b, envs, what):
    for (name, x), (_, y) in zip(end_state(a), end_state(b)):
        same_bits(x, y, STEPS - 1, envs, "%s: %s after the run" % (what, name))


def same_outputs(got, want, i, envs, what):
    for name, x, y in zip(("f32 obs", "f32 reward", "done"), got, want):
        same_bits(np.asarray(x), np.asarray(y), i, envs, "%s: %s" % (what, name))


class Buffers(object):
    def __init__(self, v):
        from charginghub_env_amd import multi_gpu as mg
        n, D, A = v.n_envs, v.obs_dim, v.act_dim
        self.v, self.n, self.D = v, n, D
        self.act, self.mask = mg.DeviceBuffer(n * A * 4), mg.DeviceBuffer(n)
        self.bits, self.tail = mg.DeviceBuffer(n * v.bit_words * 8), mg.DeviceBuffer(n * 2 * 4)
        self.obs, self.rew, self.done = mg.DeviceBuffer(n * D * 4), mg.DeviceBuffer(n * 4), mg.DeviceBuffer(n)
        self.mask.from_host(np.ones(n, dtype=np.uint8))

    def outputs(self):
        return self.obs.to_host(np.float32, (self.n, self.D)), self.rew.to_host(np.float32, (self.n,)), self.done.to_host(np.uint8, (self.n,)).astype(bool)


SPAN_FORMS = {"same_wave": dict(span_tails="same_wave"), "own_wave": dict(span_tails="own_wave"), "every_step_a_launch": dict(span_steps="off")}
SPAN_PLAN = {"same_wave": (dict(span_tails=1), 0), "own_wave": (dict(span_tails=2), 1), "every_step_a_launch": (dict(span_steps=1), None)}


@pytest.mark.parametrize("form", list(SPAN_FORMS))
def test_spans_are_bit_identical_to_the_eager_one_launch_step(form):
    """chub_run_steps with the script's eight batches, in calls of 7 steps so that spans begin and end everywhere -- k_steps_fused (the tails on
    the workgroup's last slot wave), k_steps_piped (on a fifth wave, a step behind) and every step a launch -- against the same steps issued one
    by one on a fused_step = "on" handle: both packed blocks after every call, the reset observations, the end state"""
    chub = hub()
    from charginghub_env_amd import multi_gpu as mg
    from charginghub_env_amd._lib import check
    n, D, A = tc.BLOCK, tc.D, tc.A
    for k, (name, kw) in enumerate(tc.configs()):
        envs = block(k)
        opt, piped = SPAN_PLAN[form]
        p = plan_of(kw, n, fused_step=2, **opt)
        assert p[ONE_LAUNCH] == 2 and p[SPAN_SIZE_OK] == 1 and (piped is None or p[SPAN_PIPED] == piped), (form, p)
        runs = []
        for spans in (False, True):
            v = chub.VecChargingHub(n, seed=tc.SEED, rng="philox", env_id0=tc.ENV_ID0 + n * k, fused_step="on", **kw, **(SPAN_FORMS[form] if spans else {}))
            assert v.uses_fused_step and (v.obs_dim, v.act_dim) == (D, A)
            acts = [mg.DeviceBuffer(n * A * 4) for _ in range(tc.PERIOD)]
            for b, a in enumerate(acts):
                a.from_host(tc.action_batches()[b][envs])
            packed = [mg.DeviceBuffer(n * (D + 2) * 4) for _ in range(2)]
            obs0 = mg.DeviceBuffer(n * D * 4)
            c_acts = (C.c_void_p * tc.PERIOD)(*[a.ptr for a in acts])
            c_packed = (C.c_void_p * 2)(packed[0].ptr, packed[1].ptr)
            trace = []
            for first in range(0, STEPS, 7):
                count = min(7, STEPS - first)
                if spans:
                    check(v._lib.chub_run_steps(v._h, None, c_acts, tc.PERIOD, c_packed, None, obs0.ptr, first, count, None))
                else:
                    for i in range(first, first + count):
                        if i % 96 == 0:
                            v.reset_device(obs0.ptr)
                        v.step_device_packed(acts[i % tc.PERIOD].ptr, packed[i & 1].ptr)
                last = first + count - 1
                for i in (last - 1, last):  # the two blocks that remain: steps last - 1 and last
                    trace.append((i, "packed block of the step", packed[i & 1].to_host(np.float32, (n, D + 2))))
                trace.append((None, "reset observation", obs0.to_host(np.float32, (n, D))))
            runs.append((v, trace))
        (a, ta), (b, tb) = runs
        assert len(ta) == len(tb)
        for (i, what, x), (_, _, y) in zip(ta, tb):
            same_bits(y, x, i, envs, "spans (%s) vs eager: %s" % (form, what))
        same_end_state(b, a, envs, "spans (%s) vs eager" % form)
        a.close()
        b.close()


@pytest.mark.parametrize("form", ["two_launch", "one_launch", "rows"])
def test_step_bits_device_is_bit_identical_to_step(form):
    """chub_step_bits_device: one bit per pile, the two tail actions through d_tail (StationArrays::tail_act is not read; the one-launch
    step runs its BITS instantiation) -- against chub_step on the same action rows"""
    ha, hb = make(form), make(form)
    bufs = [Buffers(v) for v, _ in hb]
    for ep, t, i in tc.step_plan():
        if t == 0:
            for (a, envs), (b, _) in zip(ha, hb):
                same_bits(b.reset(), a.reset(), None, envs, "reset observation")
        act = tc.actions(i)
        for (a, envs), (b, _), d in zip(ha, hb, bufs):
            want = a.step(act[envs])[:3]
            bits, tail = b.pack_actions(act[envs])
            assert np.array_equal(tail, act[envs][:, tc.S:])
            d.bits.from_host(bits)
            d.tail.from_host(tail)
            b.step_bits_device(d.bits.ptr, d.tail.ptr, d.obs.ptr, d.rew.ptr, d.done.ptr)
            same_outputs(d.outputs(), want, i, envs, "step_bits_device vs step (%s)" % form)
    for (a, envs), (b, _) in zip(ha, hb):
        same_end_state(b, a, envs, "step_bits_device vs step (%s)" % form)
    close_all(ha + hb)


@pytest.mark.parametrize("form", ["two_launch", "rows"])
def test_per_env_clocks_are_bit_identical_to_lock_step(form):
    """after the common reset every step goes through chub_dmask_step_envs_device with a device mask of ones: k_env<.., MULTI>, one tick per
    call as a lock-step step, so the Philox ticks line up (tests/test_gpu_autoreset.py: a launch is a tick, whoever it serves)"""
    ha, hb = make(form), make(form)
    bufs = [Buffers(v) for v, _ in hb]
    for ep, t, i in tc.step_plan():
        if t == 0:
            for (a, envs), (b, _) in zip(ha, hb):
                same_bits(b.reset(), a.reset(), None, envs, "reset observation")
                assert b.clock_groups == 1
        act = tc.actions(i)
        for (a, envs), (b, _), d in zip(ha, hb, bufs):
            want = a.step(act[envs])[:3]
            d.act.from_host(act[envs])
            b.step_envs_dmask_device(d.mask.ptr, d.act.ptr, d.obs.ptr, d.rew.ptr, d.done.ptr)
            same_outputs(d.outputs(), want, i, envs, "device mask of ones vs lock-step (%s)" % form)
    for (a, envs), (b, _) in zip(ha, hb):
        same_end_state(b, a, envs, "device mask of ones vs lock-step (%s)" % form)
    close_all(ha + hb)


@pytest.mark.parametrize("form", ["two_launch", "one_launch", "wave", "rows"])
def test_telemetry_off_is_bit_identical_to_telemetry_on(form):
    """the form the benchmark runs skips the CHUB_TEL stores: f32 obs, reward and done are those of the telemetry-on run of the same form"""
    ha, hb = make(form), make(form)
    for v, _ in ha:
        v.set_telemetry(True)
    for ep, t, i in tc.step_plan():
        if t == 0:
            for (a, envs), (b, _) in zip(ha, hb):
                same_bits(b.reset(), a.reset(), None, envs, "reset observation")
        act = tc.actions(i)
        for (a, envs), (b, _) in zip(ha, hb):
            same_outputs(b.step(act[envs])[:3], a.step(act[envs])[:3], i, envs, "telemetry off vs on (%s)" % form)
    for (a, envs), (b, _) in zip(ha, hb):
        same_end_state(b, a, envs, "telemetry off vs on (%s)" % form)
    close_all(ha + hb)
