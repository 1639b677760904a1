"""rng_mode PHILOX_CURVES running free (k_slot_curves, its k_reset_levels + k_env<.., PHILOX> legs) against its own step-for-step
specification: the oracle's ORC_RNG_PHILOX_CURVES back-end (oracle/chub_oracle.c; pinned by itself in tests/test_oracle_curves_cpu.py).

tests/test_gpu_soc_curves.py holds the kernel to the reference's fixtures in tape mode (two envs), to the draw contract for new cars, to
the curve chain given the device's own charging flag, and to itself across launch forms.  Here every decision of the free-running mode is
compared with an independent implementation: the on / off decision (must_charge, the action threshold), the stay countdown and the
departure step, the slot an admitted car lands in (ballot rank inside a unit of H lanes that need not start at lane 0), the integer
butterfly sums and the station record of EVERY unit of a workgroup, the tail's observation / reward / telemetry, masked calls, restores.

The comparisons and their bars are those PHILOX is held to (tests/test_gpu_parity.py::_philox_parity, tests/test_gpu_env_clocks.py::Pair,
both taking the mode as `rng`): nine slot fields and the station records bit for bit, integer telemetry exact, float telemetry /
observation / reward to TIGHT = 1e-9, `done` exact, no oracle overflow flag.  They hold for the same reason: the same f32 curve arithmetic
on both sides and order-independent integer sums."""
import ctypes as C

import numpy as np
import pytest

import orclib
from orclib import orc, ptr
from test_gpu_env_clocks import KW, Pair, random_sequences_of_masked_calls, restore_into_a_fresh_handle, subset_resets_and_steps
from test_gpu_parity import PHILOX_CASES, TIGHT, _oracle_vec, _philox_parity, _user_series_parity, close, hub

pytestmark = pytest.mark.gpu

RNG = "philox_curves"

# ---------------------------------------------------------------------------------------------- 1. hub shapes, whole days
CURVES_CASES = [c for c in PHILOX_CASES if max(c[1]["station_list"]) <= 64]  # (the mode refuses stations of more than 64 piles)


def test_the_case_list_is_what_the_mode_takes():
    assert [c[0] for c in CURVES_CASES] == ["c2", "c3", "c5", "c3_xcd", "ragged", "one_pile", "max64", "constant", "fcev_stuck", "small_fast"]


@pytest.mark.parametrize("label,kw,n", CURVES_CASES, ids=[c[0] for c in CURVES_CASES])
def test_philox_curves_matches_oracle(label, kw, n):
    """every hub shape PHILOX is held to that this mode takes, same env counts (2048 for c3_xcd, 77 / 130 / 33 that fill no workgroup),
    same plan: two whole days, a cut-short one and a 30-step one"""
    _philox_parity(label + "_curves", kw, n, rng=RNG)


# ---------------------------------------------------------------------------------------------- 2. padding boundaries
# A unit is H = pow2 >= S lanes of a wave, 256 / H units per 256-lane workgroup, one station per workgroup.  Pile pairs on both sides of
# every power of two up to 64, a station without piles, in both type orders.  Env counts: 300 where both stations have at most 8 piles
# (H = 1, 2, 4, 8: 256, 128, 64, 32 units per workgroup, i.e. 2, 3, 5, 10 workgroups, the last one partly filled), 37 elsewhere (H = 8, 16,
# 32, 64: 32, 16, 8, 4 units per workgroup, i.e. 2, 3, 5, 10 workgroups, the last one holding 5, 5, 5, 1; the one-pile station of (63, 1)
# has a single, partly filled workgroup).
BOUNDARY_PILES = [(1, 2), (2, 3), (4, 5), (8, 9), (16, 17), (31, 32), (33, 64), (63, 1), (0, 7), (3, 0)]


@pytest.mark.parametrize("types", [("fast", "slow"), ("slow", "fast")], ids=["fast_slow", "slow_fast"])
@pytest.mark.parametrize("piles", BOUNDARY_PILES, ids=["%d_%d" % p for p in BOUNDARY_PILES])
def test_padding_boundaries_match_oracle(piles, types):
    kw = dict(station_list=list(piles), station_type_list=list(types), hydro_prod_rate=100.0, hydro_store_vlt=25.0,
              init_soc=0.2, fc_max_power=100.0, fcev_permeate=0.03)
    n = 300 if max(piles) <= 8 else 37
    _philox_parity("boundary_%d_%d_%s" % (piles + (types[0],)), kw, n, plan=(40, 12), rng=RNG)


# ---------------------------------------------------------------------------------------------- 3. every unit position, benchmark size
def test_every_unit_of_65536_envs_matches_oracle():
    """65 536 x [20 fast, 25 slow], the size the mode is benchmarked at: reset + 24 steps, ALL envs compared at every step (so every unit
    index within a workgroup, every workgroup incl. the last, every XCD), vectorised: the oracle's whole-batch accessors
    (orc_vec_slots / _station_scalars / _telemetry) against the library's, no per-env Python loop.  24 steps because the fast station's cars
    stay 3 .. 20 slots: departures and re-admissions into freed slots happen in both stations (asserted).  The oracle runs on 16
    threads (its 65 536 env objects take about 3 GB of host memory)."""
    chub = hub()
    kw = dict(PHILOX_CASES[1][1])
    for k, d in (("constant_charging", False), ("renew_fluctuate", 0.0), ("price_fluctuate", 0.0), ("hydro_loss", 0.0)):
        kw.setdefault(k, d)
    n, seed, env_id0, steps = 65536, 0xC0FFEE12345, 1000, 24
    S = kw["station_list"]
    v = chub.VecChargingHub(n, seed=seed, rng=RNG, env_id0=env_id0, **kw)
    v.set_telemetry(True)
    cfg, h = _oracle_vec(kw, n, env_id0, seed, rng=RNG)
    D, A = v.obs_dim, v.act_dim
    o_obs, o_rew, o_done = np.zeros((n, D)), np.zeros(n), np.zeros(n, dtype=np.uint8)
    want_sl = [np.zeros((n, 9, S[k]), dtype=np.float32) for k in (0, 1)]
    want_sc, want_tel = np.zeros((n, 2, 8)), np.zeros((n, 38))
    rs = np.random.RandomState(7)
    was_car = [np.zeros((n, S[k]), dtype=bool) for k in (0, 1)]
    departures, readmissions = [0, 0], [0, 0]

    def compare(label, with_step):
        sl, sc = v.slots(), v.station_scalars()
        orc.orc_vec_station_scalars(h, ptr(want_sc))
        for k in (0, 1):
            orc.orc_vec_slots(h, k, ptr(want_sl[k]))
            bad = np.nonzero(sl[k].view(np.uint32) != want_sl[k].view(np.uint32))
            assert bad[0].size == 0, (label, "slots of station", k, "first (env, field, slot)", [int(x[0]) for x in bad],
                                      bad[0].size, sl[k][bad][:5], want_sl[k][bad][:5])
            bad = np.nonzero((sc[:, k, :6] != want_sc[:, k, :6]).any(axis=1))[0]
            assert bad.size == 0, (label, "station record", k, bad[:5], sc[bad[:3], k], want_sc[bad[:3], k])
            car, new = want_sl[k][:, 0] > 0.5, (want_sl[k][:, 0] > 0.5) & (want_sl[k][:, 8] == 0)
            if with_step:
                departures[k] += int((was_car[k] & (~car | new)).sum())
                readmissions[k] += int((was_car[k] & new).sum())
            was_car[k][:] = car
        close(v.obs_f64(), o_obs, (label, "obs"), rtol=TIGHT, atol=TIGHT)
        if with_step:
            tel = v.telemetry()
            orc.orc_vec_telemetry(h, ptr(want_tel))
            assert np.array_equal(tel[:, 19:24], want_tel[:, 19:24]), (label, "integer telemetry")
            close(tel[:, :19], want_tel[:, :19], (label, "telemetry"), rtol=TIGHT, atol=1e-7)
            close(tel[:, 24:28], want_tel[:, 24:28], (label, "telemetry (after the fuel cell)"), rtol=TIGHT, atol=1e-7)
            assert np.array_equal(tel[:, 28:38], want_tel[:, 28:38]), (label, "telemetry (station scalars)")
            close(v.reward_f64(), o_rew, (label, "reward"), rtol=TIGHT, atol=TIGHT)

    v.reset()
    orc.orc_vec_reset(h, None, None, ptr(o_obs))
    compare("reset", False)
    for t in range(steps):
        act = rs.uniform(-1, 1, size=(n, A)).astype(np.float32)
        if t % 7 == 3:
            act[:, :S[0] + S[1]] = 1.0
        obs, rew, done, _ = v.step(act)
        orc.orc_vec_step(h, ptr(act), None, ptr(o_obs), ptr(o_rew), ptr(o_done), 16)
        assert np.array_equal(done, o_done.astype(bool))
        compare(("step", t), True)
        close(obs, o_obs, ("obs f32", t), atol=1e-6)
    assert orc.orc_vec_overflow(h) == 0
    assert min(departures) > n and min(readmissions) > n // 4, (departures, readmissions)
    orc.orc_vec_destroy(h)
    v.close()


# ---------------------------------------------------------------------------------------------- 4. masked calls, restores
CURVES_SHAPES = {
    "c3": KW,                                                      # 8 and 8 units per workgroup
    "tiny": dict(KW, station_list=[1, 2]),                         # units of one and two lanes
    "one_station": dict(KW, station_list=[0, 9], fcev_permeate=0.05),
    "full_wave": dict(KW, station_list=[64, 40]),                  # a unit is a whole wave
}


@pytest.mark.parametrize("shape", sorted(CURVES_SHAPES))
def test_subset_resets_and_steps_match_the_oracle(shape):
    subset_resets_and_steps(Pair(CURVES_SHAPES[shape], 44, rng=RNG))


@pytest.mark.parametrize("seed", [1, 2])
def test_random_sequences_of_masked_calls_match_the_oracle(seed):
    random_sequences_of_masked_calls(Pair(KW, 48, rng=RNG), seed)


@pytest.mark.parametrize("shape", ["c3", "one_station", "full_wave"])
def test_restore_into_a_fresh_handle_continues_the_oracle_run(shape):
    """state taken out mid-day / on diverged clocks / after resets, handle closed, fresh handle restored, the run continued against the
    SAME oracle object"""
    restore_into_a_fresh_handle(Pair(CURVES_SHAPES[shape], 36, rng=RNG))


# ---------------------------------------------------------------------------------------------- 5. user series
def test_philox_curves_user_series(tmp_path):
    _user_series_parity(tmp_path, rng=RNG)


# ---------------------------------------------------------------------------------------------- 6. launch forms against the oracle
@pytest.mark.parametrize("form", ["run_steps", "graph"])
def test_run_steps_and_graph_replay_match_the_oracle(form):
    """the steps issued by chub_run_steps / by ONE replay of a captured hipGraph (a day, a reset, 24 steps more), actions made on the
    device -- compared with the oracle fed the same action batches, not with steps issued one by one (that is
    test_gpu_soc_curves.py::test_graph_replay_and_run_steps_equal_eager_steps)"""
    chub = hub()
    from charginghub_env_amd import multi_gpu
    kw = dict(KW)
    n, seed, env_id0, total = 1000, 2024, 300, 120
    S0, S1 = kw["station_list"]
    v = chub.VecChargingHub(n, seed=seed, rng=RNG, env_id0=env_id0, **kw)
    v.set_telemetry(True)
    cfg, h = _oracle_vec(kw, n, env_id0, seed, rng=RNG)
    st = multi_gpu.Stream(0)
    acts = [multi_gpu.DeviceBuffer(n * v.act_dim * 4) for _ in range(4)]
    for bt, a in enumerate(acts):
        v.random_actions_device(a.ptr, 5, bt, st.ptr)
    host_acts = [np.ascontiguousarray(a.to_host(np.float32, (n, v.act_dim), st.ptr)) for a in acts]
    packed = [multi_gpu.DeviceBuffer(n * (v.obs_dim + 2) * 4) for _ in range(2)]
    obs0 = multi_gpu.DeviceBuffer(n * v.obs_dim * 4)
    if form == "graph":
        st.sync()
        v.graph_begin(st.ptr)
        for i in range(total):
            if i % 96 == 0:
                v.reset_device(obs0.ptr, stream=st.ptr)
            v.step_device_packed(acts[i % 4].ptr, packed[i & 1].ptr, stream=st.ptr)
        g = v.graph_end(st.ptr)
        v.graph_launch(g, st.ptr)
        st.sync()
        v.graph_destroy(g)
    else:
        c_acts = (C.c_void_p * 4)(*[a.ptr for a in acts])
        c_packed = (C.c_void_p * 2)(*[p.ptr for p in packed])
        chub._lib.check(v._lib.chub_run_steps(v._h, None, c_acts, 4, c_packed, None, obs0.ptr, 0, total, st.ptr))
    st.sync()
    o_obs, o_rew, o_done = np.zeros((n, v.obs_dim)), np.zeros(n), np.zeros(n, dtype=np.uint8)
    for i in range(total):
        if i % 96 == 0:
            orc.orc_vec_reset(h, None, None, ptr(o_obs))
        orc.orc_vec_step(h, ptr(host_acts[i % 4]), None, ptr(o_obs), ptr(o_rew), ptr(o_done), 8)
    last = packed[(total - 1) & 1].to_host(np.float32, (n, v.obs_dim + 2), st.ptr)
    sl, sc = v.slots(), v.station_scalars()
    want_sc = np.zeros((n, 2, 8))
    orc.orc_vec_station_scalars(h, ptr(want_sc))
    for k, nk in ((0, S0), (1, S1)):
        want = np.zeros((n, 9, nk), dtype=np.float32)
        orc.orc_vec_slots(h, k, ptr(want))
        assert np.array_equal(sl[k].view(np.uint32), want.view(np.uint32)), (form, "slots", k)
        assert np.array_equal(sc[:, k, :6], want_sc[:, k, :6]), (form, "station records", k)
    close(v.obs_f64(), o_obs, (form, "obs"), rtol=TIGHT, atol=TIGHT)
    close(v.reward_f64(), o_rew, (form, "reward"), rtol=TIGHT, atol=TIGHT)
    close(last[:, :v.obs_dim], o_obs, (form, "obs f32"), atol=1e-6)
    assert orc.orc_vec_overflow(h) == 0
    orc.orc_vec_destroy(h)
    v.close()
    st.destroy()


# ---------------------------------------------------------------------------------------------- 7. the urgency test on its boundary
def _whole_slot_needs(typ, cp, count):
    """cars whose need is a WHOLE number of slots in f32: (target level, need m >= 2, arrival SoC) with soc_to_time(target) - soc_to_time(soc)
    == m exactly -- found on the oracle's curves (bisection, then the f32 neighbours)"""
    import soc_curves_lib as scl
    out = []
    for lev in range(0, 1000, 7):
        tgt = np.float32(orc.orc_uniform_level(lev, 80.0, 100.0))
        tt = scl.curve(typ, 2, tgt, cp)
        for m in range(2, 12):
            goal, lo, hi = float(tt) - m, 25.0, 70.0
            if not float(scl.curve(typ, 2, lo, cp)) <= goal <= float(scl.curve(typ, 2, hi, cp)):
                continue
            for _ in range(60):
                mid = (lo + hi) / 2
                lo, hi = (mid, hi) if float(scl.curve(typ, 2, mid, cp)) < goal else (lo, mid)
            bits = int(np.float32(lo).view(np.uint32))
            for d in range(-40, 41):
                soc = np.uint32(bits + d).view(np.float32)
                ts = scl.curve(typ, 2, soc, cp)
                if float(tt) - float(ts) == m and np.float32(tt - ts) == np.float32(m):
                    out.append((lev, m, soc))
                    break
            if len(out) == count:
                return out
    return out


@pytest.mark.parametrize("cc", [False, True], ids=["curves", "constant"])
def test_urgency_decision_on_its_boundary(cc):
    """must_charge is `time_left <= ceil(need)` (CHS.hpp:883-890).  Where a car's need is a whole number m of slots, a car with time_left =
    m + 1 is NOT urgent and one with time_left = m is: the decision sits exactly on `need > time_left - 1`, where `>` and `>=` part.  Free
    runs meet such a tie about once in ten million car-steps, so it is made here: every pile of a [20 fast, 25 slow] hub is given, through
    the car tape of a tape reset (f32 bits of the arrival SoC, level | late << 16), a car whose need is whole, with an extra stay of 1
    (on the boundary at step 1, urgent at step 2) or 2 (on the boundary at step 2); every action is `off`, so the urgency test alone
    decides who charges.  Expected: the oracle's stations given the same cars (orc_station_put_car) and stepped with all-off actions -- the
    nine slot fields bit for bit for the two steps before the first car can leave (the fast curve's whole needs are 2 slots)."""
    chub = hub()
    kw = dict(KW, constant_charging=cc, fcev_permeate=0.0)
    S, types = kw["station_list"], [orclib.FAST, orclib.SLOW]
    n = 130  # 8 units per workgroup at H = 32: 17 workgroups per station, the last one holds 2
    v = chub.VecChargingHub(n, seed=3, rng=RNG, **kw)
    car = np.zeros((sum(S), 2), dtype=np.uint32)
    want, lates = [], []
    for k, off in ((0, 0), (1, S[0])):
        ties = _whole_slot_needs(types[k], cc, S[k])
        assert len(ties) >= 5, (k, cc, len(ties))
        st = orclib.OrcStation(types[k], S[k], wait=True, constant_charging=cc, index=k, slot_base=off)
        st.seed_philox(3, 0, curves=True)
        for j in range(S[k]):
            lev, m, soc = ties[j % len(ties)]
            late = 1 + j % 2
            car[off + j] = [np.float32(soc).view(np.uint32), lev | (late << 16)]
            st.put_car(j, soc, orc.orc_uniform_level(lev, 80.0, 100.0), late)
            lates.append(late)
        want.append(st)
    occ = np.stack([np.full(n, S[k] | (S[k] << 16), dtype=np.uint32) for k in (0, 1)])
    v.reset_tape(occ, np.repeat(car[None], n, axis=0))
    sl = v.slots()
    for k in (0, 1):
        w = want[k].slots()
        keep = [0, 3, 5, 6, 7, 8]  # (emergency and the situation's soc are calculate_output's, which the oracle's next step runs first)
        assert np.array_equal(sl[k][:, keep].view(np.uint32), np.repeat(w[None, keep], n, axis=0).view(np.uint32)), ("reset", k)
    off_act = np.full((n, v.act_dim), -1.0, dtype=np.float32)
    nobody = np.zeros((sum(S), 2), dtype=np.uint32)
    charging = []
    for step in range(2):  # (every stay is at least 2 + 1: nobody leaves in these two steps, so no pile asks for a new car)
        v.step_tape(off_act, np.zeros((2, n), dtype=np.uint64), np.repeat(nobody[None], n, axis=0))
        sl = v.slots()
        for k in (0, 1):
            want[k].set_tick(step + 2)
            want[k].step(np.zeros(S[k], dtype=np.float32))
            w = want[k].slots()
            assert w[0].all() and (w[7] - w[8] >= 1).all(), "a car left: the oracle's station would admit one of its own"
            bad = np.nonzero(sl[k].view(np.uint32) != np.repeat(w[None], n, axis=0).view(np.uint32))
            assert bad[0].size == 0, (cc, "step", step, "station", k, "first (env, field, slot)", [int(x[0]) for x in bad], sl[k][bad][:4])
            charging.append(w[1].copy())
        assert orc.orc_station_stay_overflow(want[0].s) == 0 and orc.orc_station_stay_overflow(want[1].s) == 0
    # the boundary was met from both sides: at step 1 nobody charges (extra stay 1: the tie), at step 2 exactly the cars with an extra stay
    # of 1 do (now urgent) and those with 2 do not (their tie)
    lates = np.array(lates)
    first, second = np.concatenate(charging[0:2]), np.concatenate(charging[2:4])
    assert not (first > 0.5).any() and np.array_equal(second > 0.5, lates == 1), (first, second, lates)
    v.close()
