"""The oracle's ORC_RNG_PHILOX_CURVES back-end (oracle/chub_oracle.c) is the step-for-step specification k_slot_curves is held to in
tests/test_gpu_soc_curves_oracle.py, so it is pinned here by itself, without a GPU:
  * the contract of include/chub.h (the PHILOX_CURVES paragraph) on the oracle alone, against ORC_RNG_PHILOX on the same seed and against
    the Philox words themselves;
  * the cars it admits and how it moves them, against the real reference's curves (oracle/_ref/libchs_ref.so, where it was built);
  * the whole-batch accessors the GPU tests read it through, against the per-env ones.
That ORC_RNG_PHILOX trajectories did not move is tests/test_oracle_golden.py / test_oracle_vs_ref.py / test_host_cpu.py, untouched."""
import ctypes as C
import os

import numpy as np
import pytest

import orclib
from orclib import orc, ptr
import soc_curves_lib as scl

SITE_SOC = 5
C3 = dict(piles=(20, 25), types=("fast", "slow"), hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2, fc_max_power=100.0,
          fcev_permeate=0.01)


def _vec(mode, n, env_id0, seed, **over):
    cfg = orclib.make_config(**dict(C3, **over))
    return cfg, orc.orc_vec_create(C.byref(cfg), orclib.tables(), n, env_id0, mode, seed)


def _slots(h, e, k, nk):
    out = np.zeros((9, nk), dtype=np.float32)
    orc.orc_station_slots(orc.orc_env_station(orc.orc_vec_env(h, e), k), ptr(out))
    return out


def _need(typ, target, soc, cp):
    """calculate_min_charging_time (CHS.hpp:933-937 / 1098-1102) on the oracle's f32 curves"""
    return np.float32(scl.curve(typ, 2, target, cp) - scl.curve(typ, 2, soc, cp))


def test_header_and_binding_agree_on_the_constant():
    import re
    hdr = open(os.path.join(orclib.ORACLE_DIR, "chub_oracle.h")).read()
    modes = dict((name, int(v)) for name, v in re.findall(r"\bORC_RNG_(\w+)\s*=\s*(\d+)", hdr))
    assert modes == {"COMPAT": orclib.COMPAT, "PHILOX": orclib.PHILOX, "PHILOX_CURVES": orclib.PHILOX_CURVES} == {"COMPAT": 0, "PHILOX": 1, "PHILOX_CURVES": 2}
    # ... and the library means the same by it: a vector created with the constant admits the continuous SoC (the next test), one seeded
    # through orc_rng_seed_philox_curves too (test_admitted_cars_follow_the_reference_curves)


def test_reset_is_philox_with_the_continuous_soc_and_then_the_runs_part():
    """chub.h: on one seed the cars, targets and extra stays at reset are those of PHILOX, each car's SoC lies inside its PHILOX class's
    cell of the table (nodes 2c .. 2c + 2) -- and IS soc_from_word of the block's word 0 --, everything else draws PHILOX's counters;
    trajectories part after the reset because a stay depends on the SoC"""
    n, env_id0, seed = 96, 700, 0xABCDEF0123
    icdf = np.fromfile(os.path.join(orclib.DATA_DIR, "soc_d_icdf_4097.f32"), dtype="<f4")
    t = orclib.tables()
    cfg, hp = _vec(orclib.PHILOX, n, env_id0, seed)
    _, hc = _vec(orclib.PHILOX_CURVES, n, env_id0, seed)
    D = orc.orc_env_obs_dim(C.byref(cfg))
    obs_p, obs_c = np.zeros((n, D)), np.zeros((n, D))
    orc.orc_vec_reset(hp, None, None, ptr(obs_p))
    orc.orc_vec_reset(hc, None, None, ptr(obs_c))
    cars = strictly_inside = 0
    for e in range(n):
        for k, nk, off in ((0, 20, 0), (1, 25, 20)):
            a, b = _slots(hc, e, k, nk), _slots(hp, e, k, nk)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[6], b[6]) and np.array_equal(a[8], b[8]), (e, k)
            for j in np.nonzero(a[0] > 0.5)[0]:
                w = scl.philox_word(seed, 1, env_id0 + e, SITE_SOC, off + int(j))
                soc = np.float32(orc.orc_soc_from_word(t, int(w[0])))
                assert a[5, j].view(np.uint32) == soc.view(np.uint32) and a[4, j] == a[5, j]
                c = int(w[0]) >> 21
                assert b[5, j] == np.float32(orc.orc_soc_level_value(t, c))
                lo, hi = (np.float32(75.0 - 5.0 * float(np.clip(x, 1.0, 10.0))) for x in (icdf[2 * c + 2], icdf[2 * c]))
                assert lo <= soc <= hi, (e, k, j, lo, soc, hi)
                strictly_inside += bool(lo < soc < hi and soc != b[5, j])
                late = orc.orc_late_from_word(t, int(w[2]))
                assert a[6, j] == np.float32(orc.orc_uniform_level(int(w[1]) % 1000, 80.0, 100.0))
                assert int(a[7, j]) - int(np.ceil(_need(k, a[6, j], a[5, j], 0))) == late, ("extra stay", e, k, j)
                assert int(b[7, j]) - int(np.ceil(_need(k, b[6, j], b[5, j], 0))) == late, ("extra stay, PHILOX", e, k, j)
                assert a[3, j] == scl.arrive(k, soc, 0)[0]
                cars += 1
    assert cars > 500 and strictly_inside > cars // 2, (cars, strictly_inside)
    # the station records at reset: occupancy, queue, flow (the sums differ with the powers)
    sp, sc = np.zeros((n, 2, 8)), np.zeros((n, 2, 8))
    orc.orc_vec_station_scalars(hp, ptr(sp))
    orc.orc_vec_station_scalars(hc, ptr(sc))
    assert np.array_equal(sp[:, :, 3:6], sc[:, :, 3:6])
    # ... and then they part, not only in the SoC values: a car whose need crosses a whole slot inside its class's cell (about one in a
    # thousand) stays a slot longer or shorter, and from there on other cars are admitted into other piles
    rs = np.random.RandomState(3)
    rew, done = np.zeros(n), np.zeros(n, dtype=np.uint8)
    parted_at = None
    occ = {id(hp): [np.zeros((n, 9, 20), np.float32), np.zeros((n, 9, 25), np.float32)],
           id(hc): [np.zeros((n, 9, 20), np.float32), np.zeros((n, 9, 25), np.float32)]}
    for step in range(96):
        act = rs.uniform(-1, 1, size=(n, 47)).astype(np.float32)
        orc.orc_vec_step(hp, ptr(act), None, ptr(obs_p), ptr(rew), ptr(done), 2)
        orc.orc_vec_step(hc, ptr(act), None, ptr(obs_c), ptr(rew), ptr(done), 2)
        for h in (hp, hc):
            for k in (0, 1):
                orc.orc_vec_slots(h, k, ptr(occ[id(h)][k]))
        same = all(np.array_equal(occ[id(hp)][k][:, f], occ[id(hc)][k][:, f]) for k in (0, 1) for f in (0, 6, 8))
        if parted_at is None and not same:
            parted_at = step
    assert parted_at is not None, "96 steps of %d C3 hubs: the same cars in the same piles as under PHILOX -- is this the new mode?" % n
    assert orc.orc_vec_overflow(hc) == 0 and orc.orc_vec_overflow(hp) == 0
    for e in range(n):
        env = orc.orc_vec_env(hc, e)
        assert orc.orc_env_stay_overflow(env) == 0 and orc.orc_env_q_overflow(env) == 0
        assert orc.orc_station_stay_overflow(orc.orc_env_station(env, 0)) == 0
    orc.orc_vec_destroy(hp)
    orc.orc_vec_destroy(hc)


def test_everything_but_the_arrival_soc_draws_philox_counters():
    """a hub whose stations hold no piles: no car is ever admitted, so the two back-ends must give the SAME run -- arrival counts, renege /
    balk, the forecourt, OU, days all come from PHILOX's counters"""
    n = 16
    over = dict(piles=(0, 0), fcev_permeate=0.2, renew_fluctuate=0.3, price_fluctuate=0.3)
    cfg, hp = _vec(orclib.PHILOX, n, 5, 99, **over)
    _, hc = _vec(orclib.PHILOX_CURVES, n, 5, 99, **over)
    D = orc.orc_env_obs_dim(C.byref(cfg))
    out = {}
    for name, h in (("p", hp), ("c", hc)):
        obs, rew, done = np.zeros((n, D)), np.zeros(n), np.zeros(n, dtype=np.uint8)
        orc.orc_vec_reset(h, None, None, ptr(obs))
        rs = np.random.RandomState(1)
        trace = [obs.copy()]
        for _ in range(100):
            act = rs.uniform(-1, 1, size=(n, 2)).astype(np.float32)
            orc.orc_vec_step(h, ptr(act), None, ptr(obs), ptr(rew), ptr(done), 1)
            tel, sc = np.zeros((n, 38)), np.zeros((n, 2, 8))
            orc.orc_vec_telemetry(h, ptr(tel))
            orc.orc_vec_station_scalars(h, ptr(sc))
            trace += [obs.copy(), rew.copy(), tel, sc]
        out[name] = trace
        orc.orc_vec_destroy(h)
    assert all(np.array_equal(a, b) for a, b in zip(out["p"], out["c"]))
    assert np.any(out["c"][-1][:, :, 4] > 0), "the queues of the pile-less stations never filled: nothing was drawn"


def test_whole_batch_accessors_equal_the_per_env_ones():
    n = 24
    cfg, h = _vec(orclib.PHILOX_CURVES, n, 0, 4)
    D = orc.orc_env_obs_dim(C.byref(cfg))
    obs, rew, done = np.zeros((n, D)), np.zeros(n), np.zeros(n, dtype=np.uint8)
    orc.orc_vec_reset(h, None, None, ptr(obs))
    rs = np.random.RandomState(2)
    for _ in range(12):
        act = rs.uniform(-1, 1, size=(n, 47)).astype(np.float32)
        orc.orc_vec_step(h, ptr(act), None, ptr(obs), ptr(rew), ptr(done), 3)
    sc, tel = np.zeros((n, 2, 8)), np.zeros((n, 38))
    orc.orc_vec_station_scalars(h, ptr(sc))
    orc.orc_vec_telemetry(h, ptr(tel))
    for k, nk in ((0, 20), (1, 25)):
        sl = np.full((n, 9, nk), np.nan, dtype=np.float32)
        orc.orc_vec_slots(h, k, ptr(sl))
        for e in range(n):
            assert np.array_equal(sl[e], _slots(h, e, k, nk))
            ws = np.zeros(8)
            orc.orc_station_scalars(orc.orc_env_station(orc.orc_vec_env(h, e), k), ptr(ws))
            assert np.array_equal(sc[e, k], ws)
    for e in range(n):
        wt = np.zeros(38)
        orc.orc_env_telemetry(orc.orc_vec_env(h, e), ptr(wt))
        assert np.array_equal(tel[e], wt)
    orc.orc_vec_destroy(h)


needs_ref = pytest.mark.skipif(not orclib.ref_available(), reason="oracle/_ref/libchs_ref.so (the real reference core) was not built here")


@needs_ref
@pytest.mark.parametrize("typ,piles,cc", [(orclib.FAST, 20, False), (orclib.SLOW, 25, False), (orclib.FAST, 7, True), (orclib.SLOW, 64, True)],
                         ids=["fast_20", "slow_25", "fast_7_constant", "slow_64_constant"])
def test_admitted_cars_follow_the_reference_curves(typ, piles, cc):
    """400 steps of one station under the new back-end.  The reference driver exports no entry point that puts a given car into a pile
    (the reference's add_car draws its own, CHS.hpp:864-877), so the comparison is per car, through the curve functions the REAL
    reference exports (ref_curve_fast / ref_curve_slow): for every car the back-end admitted -- its continuous arrival SoC, target and
    extra stay taken from the Philox block -- the reference's add_car results (power, stay), and then, step by step under the step's
    on / off vector, the reference's judge_feasibility + assign_on_off_piece decision, its car_step (power, SoC), calculate_needed
    (emergency) and remove_car (the countdown and the departure step).  Per-slot state bit for bit."""
    ref = orclib.ref()
    rc = ref.ref_curve_fast if typ == orclib.FAST else ref.ref_curve_slow
    f = lambda which, x: np.float32(rc(which, float(x), int(cc)))
    t = orclib.tables()
    seed, gid, base = 31337, 12, 3
    s = orclib.OrcStation(typ, piles, wait=True, constant_charging=cc, index=0, slot_base=base)
    s.seed_philox(seed, gid, curves=True)

    def emergency(soc, target, stay, already):  # calculate_needed, CHS.hpp:879-898 / 1044-1063
        need = np.float32(f(2, target) - f(2, soc))
        left = stay - already
        if not need > 0:
            return np.float32(0.0)
        if left <= np.ceil(need):
            return np.float32(10.0)
        return np.float32(float(np.float32(need / np.float32(left))) ** 2)

    def check_new(a, j, tick):  # add_car, CHS.hpp:864-877 / 1029-1042
        w = scl.philox_word(seed, tick, gid, SITE_SOC, base + int(j))
        soc = np.float32(orc.orc_soc_from_word(t, int(w[0])))
        tgt = np.float32(orc.orc_uniform_level(int(w[1]) % 1000, 80.0, 100.0))
        late = orc.orc_late_from_word(t, int(w[2]))
        assert a[5, j].view(np.uint32) == soc.view(np.uint32) and a[4, j] == soc and a[6, j] == tgt, (tick, j)
        need = np.float32(f(2, tgt) - f(2, soc))
        assert int(a[7, j]) == int(np.ceil(need)) + late and int(a[8, j]) == 0, (tick, j, a[7, j], need, late)
        assert a[3, j].view(np.uint32) == f(0, f(2, soc)).view(np.uint32), (tick, j)
        assert a[2, j].view(np.uint32) == emergency(soc, tgt, int(a[7, j]), 0).view(np.uint32), (tick, j)
        assert a[1, j] == 0

    s.set_tick(1)
    s.reset()
    prev = s.slots()
    for j in np.nonzero(prev[0] > 0.5)[0]:
        check_new(prev, j, 1)
    rs = np.random.RandomState(typ * 10 + piles)
    admitted = stepped = left = idle = forced = 0
    for step in range(400):
        tick = step + 2
        act = (rs.uniform(size=piles) < (0.5 if step % 5 else 1.0)).astype(np.float32)
        s.set_tick(tick)
        s.step(act)
        a = s.slots()
        for j in range(piles):
            was = prev[0, j] > 0.5
            if was:
                on = act[j] == 1 or prev[2, j] >= np.float32(1.01)  # judge_feasibility: CHS.hpp:1404-1413
                forced += bool(on and act[j] != 1)
                stay, already = int(prev[7, j]), int(prev[8, j]) + 1
                if stay - already <= 0:  # remove_car: the pile is cleared ... and may take a new car in the same step
                    left += 1
                    if a[0, j] > 0.5:
                        check_new(a, j, tick)
                        admitted += 1
                    else:
                        assert not a[:7, j].any() and a[7, j] == -1 and a[8, j] == -1, (step, j, a[:, j])
                    continue
                assert a[0, j] == 1 and int(a[7, j]) == stay and int(a[8, j]) == already, (step, j)
                assert a[1, j] == (1.0 if on else 0.0), ("on/off", step, j, act[j], prev[2, j])
                if on:  # car_step, CHS.hpp:900-909 / 1065-1074
                    tt = np.float32(f(2, prev[4, j]) + np.float32(1.0))
                    want_p, want_s = f(0, tt), f(1, tt)
                    stepped += 1
                else:
                    want_p, want_s = prev[3, j], prev[4, j]
                    idle += 1
                assert a[3, j].view(np.uint32) == np.float32(want_p).view(np.uint32), ("power", step, j)
                assert a[4, j].view(np.uint32) == np.float32(want_s).view(np.uint32), ("soc", step, j)
                assert a[5, j] == prev[5, j] and a[6, j] == prev[6, j]
                assert a[2, j].view(np.uint32) == emergency(a[4, j], a[6, j], stay, already).view(np.uint32), ("emergency", step, j)
            elif a[0, j] > 0.5:
                check_new(a, j, tick)
                admitted += 1
        prev = a
    assert orc.orc_station_stay_overflow(s.s) == 0
    assert admitted > 3 * piles and stepped > 20 * piles and left > 3 * piles and idle > piles and forced > 0, (admitted, stepped, left, idle, forced)


@pytest.mark.parametrize("typ,piles,cc", [(orclib.FAST, 20, False), (orclib.SLOW, 25, True)], ids=["fast", "slow_constant"])
def test_put_car_places_what_add_car_places(typ, piles, cc):
    """orc_station_put_car (the hook the GPU's tape-mode boundary test gives the oracle its cars through) is add_car behind the draws: a
    station filled with the cars another one drew for itself holds the same piles, and those cars then step the same way"""
    t = orclib.tables()
    a = orclib.OrcStation(typ, piles, wait=True, constant_charging=cc, index=0, slot_base=0)
    a.seed_philox(77, 3, curves=True)
    a.set_tick(1)
    a.reset()
    b = orclib.OrcStation(typ, piles, wait=True, constant_charging=cc, index=0, slot_base=0)
    b.seed_philox(77, 3, curves=True)
    sa = a.slots()
    cars = np.nonzero(sa[0] > 0.5)[0]
    assert len(cars) >= piles // 4
    for j in cars:
        late = orc.orc_late_from_word(t, int(scl.philox_word(77, 1, 3, SITE_SOC, int(j))[2]))
        b.put_car(j, sa[5, j], sa[6, j], late)
    keep = [0, 3, 5, 6, 7, 8]  # (emergency and the situation's soc are calculate_output's, which the next step runs first)
    assert np.array_equal(b.slots()[keep][:, cars].view(np.uint32), sa[keep][:, cars].view(np.uint32))
    act = (np.arange(piles) % 2).astype(np.float32)
    for s in (a, b):
        s.set_tick(2)
        s.step(act)
    sb, sa = b.slots(), a.slots()
    stay = cars[(sa[0, cars] > 0.5) & (sa[8, cars] == 1)]  # (the piles that were empty differ: `a` has a queue from its reset, `b` none)
    assert len(stay) >= len(cars) // 2 and np.array_equal(sb[:, stay].view(np.uint32), sa[:, stay].view(np.uint32))
