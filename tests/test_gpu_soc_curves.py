"""rng_mode PHILOX_CURVES (include/chub.h): PHILOX's draws with the reference's continuous EV arrival SoC (CHS.hpp:803-814) and car_step
evaluated on the device along the reference's curves (CHS.hpp:467-726) -- k_slot_curves in chub_kernels.hip.

What is pinned here: the reference's fixtures through the new slot kernel in tape mode; the draw contract of chub.h against the oracle's
Philox; every car's (power, SoC) against the host's f32 curve chain; the law of the arrival SoC; the whole process against COMPAT (the
reference's own streams) with k-SE bounds; the launch forms bit for bit; and what the mode refuses.

What is NOT pinned here -- every check above is either piecewise (new cars only; the curve chain given the device's OWN charging flag;
two envs in tape mode) or the kernel against itself: the free-running mode step for step against an independent implementation (the
on / off decision, countdown and departures, admission ranks in every unit of a workgroup, station sums and records, the tail, masked
calls, restores) lives in tests/test_gpu_soc_curves_oracle.py, against the oracle's ORC_RNG_PHILOX_CURVES back-end."""
import ctypes as C
import math

import numpy as np
import pytest

import orclib
from orclib import orc
import soc_curves_lib as scl

pytestmark = pytest.mark.gpu

HUB = dict(station_list=[20, 25], station_type_list=["fast", "slow"], hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2,
           fc_max_power=100.0, fcev_permeate=0.01)
SITE_SOC = 5


def hub():
    import charginghub_env_amd as chub
    return chub


def _acts(n, A, seed, t):
    return np.random.RandomState(seed * 1000 + t).uniform(-1, 1, (n, A)).astype(np.float32)


def _state(v):
    return [s.copy() for s in v.slots()], v.station_scalars().copy()


def _same(a, b, what):
    for k in (0, 1):
        assert np.array_equal(a[0][k].view(np.uint32), b[0][k].view(np.uint32)), (what, k)
    assert np.array_equal(a[1], b[1]), what


# ---------------------------------------------------------------------------------------------- 1. the reference's fixtures, tape mode
CURVES_FIXTURES = [n for n in orclib.GOLDEN_ENV if n != "env_big_100_70"]  # (stations of more than 64 piles are refused: test below)


@pytest.mark.parametrize("name", CURVES_FIXTURES)
def test_curves_kernel_replays_reference_fixture(name):
    """every reference fixture (evs_reset included) through k_slot_curves + k_env<.., PHILOX>: each recorded arrival SoC goes straight into
    the car tape -- no classes -- and the per-slot state (all nine fields, every car, every step) is the reference's bit for bit"""
    assert scl.replay_fixture(hub(), name) > 20


def test_stations_of_more_than_64_piles_are_refused():
    chub = hub()
    g = orclib.load_golden("env_big_100_70")
    kw = dict(HUB, station_list=[int(x) for x in g["kw_station_list"]])
    with pytest.raises(chub.ChubError, match=r"error -4: .*PHILOX_CURVES covers stations of at most 64 piles"):
        chub.VecChargingHub(2, seed=1, rng="philox_curves", **kw)


# ---------------------------------------------------------------------------------------------- 2. the draw contract
def test_draw_contract_against_the_oracle_and_philox():
    chub = hub()
    n, seed = 4096, 777
    S0, S1 = HUB["station_list"]
    t = orclib.tables()
    cur = chub.VecChargingHub(n, seed=seed, rng="philox_curves", **HUB)
    px = chub.VecChargingHub(n, seed=seed, rng="philox", **HUB)
    cur.reset()
    px.reset()
    a, b = cur.slots(), px.slots()
    ttab = [[scl.curve(k, 2, orc.orc_uniform_level(l, 80.0, 100.0), 0) for l in range(1000)] for k in (0, 1)]
    checked = 0
    for tick, label in ((1, "reset"), (2, "step")):
        if label == "step":
            act = _acts(n, cur.act_dim, 3, 0)
            cur.step(act)
            a = cur.slots()
        for k, off in ((0, 0), (1, S0)):
            sa, sb = a[k], b[k]
            if label == "reset":  # the same cars, targets and extra stays as PHILOX; the SoC inside its PHILOX class's cell
                assert np.array_equal(sa[:, 0], sb[:, 0]) and np.array_equal(sa[:, 6], sb[:, 6])
            env, s = np.nonzero((sa[:, 0] > 0.5) & (sa[:, 8] == 0))  # the cars admitted by this launch
            for e, j in zip(env[::7], s[::7]):  # (every 7th: ~25 000 Philox blocks on the host)
                w = scl.philox_word(seed, tick, int(e), SITE_SOC, off + int(j))
                soc = np.float32(orc.orc_soc_from_word(t, int(w[0])))
                assert np.float32(sa[e, 5, j]).view(np.uint32) == soc.view(np.uint32), (label, k, e, j)
                lev = int(w[1]) % 1000
                assert sa[e, 6, j] == np.float32(orc.orc_uniform_level(lev, 80.0, 100.0))
                late = orc.orc_late_from_word(t, int(w[2]))
                need = np.float32(ttab[k][lev] - scl.curve(k, 2, soc, 0))
                assert sa[e, 7, j] == min(int(np.ceil(need)) + late, 31), (label, k, e, j)
                if label == "reset":
                    assert sb[e, 5, j] == np.float32(orc.orc_soc_level_from_word(t, int(w[0])))
                    c = int(w[0]) >> 21
                    lo, hi = (np.float32(75 - 5 * np.float64(np.clip(t_, 1, 10))) for t_ in (_icdf(2 * c), _icdf(2 * c + 2)))
                    assert min(lo, hi) <= soc <= max(lo, hi)
                    need_b = np.float32(ttab[k][lev] - scl.curve(k, 2, sb[e, 5, j], 0))
                    assert sb[e, 7, j] == min(int(np.ceil(need_b)) + late, 31)
                checked += 1
    assert checked > 10000
    cur.close()
    px.close()


_ICDF = None


def _icdf(i):
    global _ICDF
    if _ICDF is None:
        import os
        _ICDF = np.fromfile(os.path.join(orclib.DATA_DIR, "soc_d_icdf_4097.f32"), dtype="<f4")
    return np.float32(_ICDF[i])


# ---------------------------------------------------------------------------------------------- 3. the curves on the device
@pytest.mark.parametrize("shape", ["c4", "fast_fast", "slow_slow", "constant"])
def test_every_car_follows_the_host_curve_chain(shape):
    """a whole day: each car's (power, soc) at every step is the f32 chain soc -> soc_to_time -> +1 -> time_to_soc / time_to_power from its
    arrival SoC, advanced once per step the car charged (the host's curves, the chain build_class_row tabulates for PHILOX)"""
    chub = hub()
    kw = dict(HUB)
    n, check_envs = 4096, 384
    if shape == "fast_fast":
        kw.update(station_list=[20, 25], station_type_list=["fast", "fast"])
        n = check_envs = 512
    elif shape == "slow_slow":
        kw.update(station_list=[20, 25], station_type_list=["slow", "slow"])
        n = check_envs = 512
    elif shape == "constant":
        kw.update(constant_charging=True)
        n = check_envs = 512
    types = [0 if s == "fast" else 1 for s in kw["station_type_list"]]
    cp = bool(kw.get("constant_charging", False))
    v = chub.VecChargingHub(n, seed=99, rng="philox_curves", **kw)
    v.reset()
    prev = None
    n_steps_seen = 0
    for t in range(97):
        if t:
            v.step(_acts(n, v.act_dim, 11, t))
        sl = v.slots()
        for k in (0, 1):
            s = sl[k][:check_envs]
            occ = s[:, 0] > 0.5
            new = occ & (s[:, 8] == 0)
            for e, j in zip(*np.nonzero(new)):
                pw, sc = scl.arrive(types[k], s[e, 5, j], cp)
                assert (s[e, 3, j], s[e, 4, j]) == (pw, sc), (shape, t, k, e, j)
            if prev is not None:
                p = prev[k][:check_envs]
                old = occ & ~new
                for e, j in zip(*np.nonzero(old)):
                    if s[e, 1, j] > 0.5:  # charged this step: one car_step from where the previous step left it
                        pw, sc = scl.car_step(types[k], p[e, 4, j], cp)
                        n_steps_seen += 1
                    else:
                        pw, sc = p[e, 3, j], p[e, 4, j]
                    assert np.float32(s[e, 3, j]).view(np.uint32) == np.float32(pw).view(np.uint32), (shape, t, k, e, j)
                    assert np.float32(s[e, 4, j]).view(np.uint32) == np.float32(sc).view(np.uint32), (shape, t, k, e, j)
        prev = sl
    assert n_steps_seen > 1000
    v.close()


# ---------------------------------------------------------------------------------------------- 4. the law of the arrival SoC
def test_arrival_soc_is_the_reference_law():
    """all arrival SoCs at reset of 65 536 x [20, 25]: Kolmogorov distance to 75 - 5 clip(N(7,3), 1, 10) within 1.63 / sqrt(n), and a
    continuum of values away from the two clip atoms (a class mode has at most 2048)"""
    chub = hub()
    v = chub.VecChargingHub(65536, seed=5, rng="philox_curves", **HUB)
    v.reset()
    sl = v.slots()
    x = np.concatenate([sl[k][:, 5][sl[k][:, 0] > 0.5] for k in (0, 1)]).astype(np.float64)
    v.close()
    n = x.size
    assert n > 500000
    x.sort()

    def cdf(s):  # P(75 - 5 clip(Z, 1, 10) <= s) with Z ~ N(7, 3): d = (75 - s) / 5, P(clip(Z) >= d)
        d = (75.0 - s) / 5.0
        if d <= 1.0:
            return 1.0
        if d > 10.0:
            return 0.0
        return 1.0 - 0.5 * (1.0 + math.erf((d - 7.0) / (3.0 * math.sqrt(2.0))))

    def cdf_left(s):  # P(SoC < s): differs from cdf(s) at the two atoms only
        if s == 25.0:
            return 0.0
        if s == 70.0:
            return 1.0 - 0.5 * (1.0 + math.erf((1.0 - 7.0) / (3.0 * math.sqrt(2.0))))
        return cdf(s)

    F = np.array([cdf(s) for s in x])
    FL = np.array([cdf_left(s) for s in x])
    i = np.arange(1, n + 1)
    # sup |F_n - F| over both sides of every jump: right limits at the last sample of a tie, left limits at the first
    ks = max(np.max(i / n - F), np.max(FL - (i - 1) / n))
    assert ks <= 1.63 / math.sqrt(n), (ks, n)
    inner = x[(x > 25.0) & (x < 70.0)]
    assert np.unique(inner).size > 50000, np.unique(inner).size


# ---------------------------------------------------------------------------------------------- 5. end to end against COMPAT
STAT_HUBS = {
    "c2": (dict(station_list=[16, 0], station_type_list=["fast", "slow"], hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2,
                fc_max_power=100.0, fcev_permeate=0.0), 8192),
    "c3": (dict(station_list=[20, 25], station_type_list=["fast", "slow"], hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2,
                fc_max_power=100.0, fcev_permeate=0.01), 8192),
    "c5": (dict(station_list=[32, 32], station_type_list=["fast", "slow"], hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2,
                fc_max_power=100.0, fcev_permeate=0.01, renew_fluctuate=0.3, price_fluctuate=0.3), 4096),
}


@pytest.mark.parametrize("policy", ["random", "all_on", "all_off"])
@pytest.mark.parametrize("hub_name", sorted(STAT_HUBS))
def test_philox_curves_is_statistically_the_reference_process(hub_name, policy):
    """as test_philox_is_statistically_the_reference_process_on_gpu (tests/test_gpu_parity.py), PHILOX_CURVES against COMPAT: per-env
    means of the episode return, occupancy, queue, arrivals, charging power and the tank's SoC within K = 4.5 of their own standard errors"""
    chub = hub()
    K = 4.5
    kw, n = STAT_HUBS[hub_name]
    S = sum(kw["station_list"])
    rs = np.random.RandomState(5)
    acts = []
    for _ in range(96):
        a = rs.uniform(-1, 1, (n, S + 2)).astype(np.float32)
        if policy == "all_on":
            a[:, :S] = 1.0
        elif policy == "all_off":
            a[:, :S] = -1.0
        acts.append(a)
    out = {}
    for mode in ("compat", "philox_curves"):
        v = chub.VecChargingHub(n, seed=4242, rng=mode, **kw)
        rz = np.random.RandomState(17)
        if mode == "compat":
            days = np.stack([rz.randint(0, 100, n), rz.randint(0, 150, n)], axis=1).astype(np.int32)
            v.reset(days, rz.normal(size=(n, 3)))
        else:
            v.reset()
        ret, cars, line, flow, power = (np.zeros(n) for _ in range(5))
        for t in range(96):
            o, r, d, _ = v.step(acts[t], rz.normal(size=(n, 3)) if mode == "compat" else None)
            ret += r
            sc = v.station_scalars()
            cars += sc[:, :, 3].sum(axis=1) / 96.0
            line += sc[:, :, 4].sum(axis=1) / 96.0
            flow += sc[:, :, 5].sum(axis=1)
            power += sc[:, :, 1].sum(axis=1) / 96.0
        out[mode] = dict(ret=ret, cars=cars, line=line, flow=flow, power=power, soc=o[:, -3].astype(np.float64))
        v.close()
    a, b = out["compat"], out["philox_curves"]
    for key in ("ret", "cars", "line", "flow", "power", "soc"):
        diff = b[key].mean() - a[key].mean()
        se = np.sqrt(a[key].var(ddof=1) / n + b[key].var(ddof=1) / n)
        print("%s / %s %s: %.4f vs %.4f (z %+.2f)" % (hub_name, policy, key, a[key].mean(), b[key].mean(), diff / se if se > 0 else 0.0))
        assert abs(diff) <= K * se + 1e-12, (hub_name, policy, key, a[key].mean(), b[key].mean(), se)


# ---------------------------------------------------------------------------------------------- 6. launch forms
def test_graph_replay_and_run_steps_equal_eager_steps():
    chub = hub()
    from charginghub_env_amd import multi_gpu
    n = 1000
    res = []
    for form in ("eager", "graph", "run_steps"):
        v = chub.VecChargingHub(n, seed=2024, rng="philox_curves", span_steps=8, **HUB)
        st = multi_gpu.Stream(0)
        acts = [multi_gpu.DeviceBuffer(n * v.act_dim * 4) for _ in range(4)]
        for bt, a in enumerate(acts):
            v.random_actions_device(a.ptr, 5, bt, st.ptr)
        packed = [multi_gpu.DeviceBuffer(n * (v.obs_dim + 2) * 4) for _ in range(2)]
        obs0 = multi_gpu.DeviceBuffer(n * v.obs_dim * 4)

        def days():
            for i in range(120):
                if i % 96 == 0:
                    v.reset_device(obs0.ptr, stream=st.ptr)
                v.step_device_packed(acts[i % 4].ptr, packed[i & 1].ptr, stream=st.ptr)

        if form == "eager":
            days()
        elif form == "graph":
            st.sync()
            v.graph_begin(st.ptr)
            days()
            g = v.graph_end(st.ptr)
            v.graph_launch(g, st.ptr)
            v.graph_destroy(g)
        else:
            c_acts = (C.c_void_p * 4)(*[a.ptr for a in acts])
            c_packed = (C.c_void_p * 2)(*[p.ptr for p in packed])
            chub._lib.check(v._lib.chub_run_steps(v._h, None, c_acts, 4, c_packed, None, obs0.ptr, 0, 120, st.ptr))
        st.sync()
        last = packed[1].to_host(np.float32, (n, v.obs_dim + 2), st.ptr)
        res.append((last, _state(v)))
        assert not v.uses_packed_kernel
        v.close()
    for r in res[1:]:
        assert np.array_equal(r[0].view(np.uint32), res[0][0].view(np.uint32))
        _same(r[1], res[0][1], "launch form")


def test_whole_batch_equals_its_halves_by_global_env_id_and_masks():
    chub = hub()
    n = 512
    whole = chub.VecChargingHub(n, seed=31, rng="philox_curves", **HUB)
    halves = [chub.VecChargingHub(n // 2, seed=31, rng="philox_curves", env_id0=h * (n // 2), **HUB) for h in (0, 1)]
    masked = chub.VecChargingHub(n, seed=31, rng="philox_curves", **HUB)
    ow = whole.reset()
    oh = [h.reset() for h in halves]
    om = masked.reset_envs(np.ones(n, bool))
    assert np.array_equal(ow, np.concatenate(oh)) and np.array_equal(ow, om)
    for t in range(30):
        a = _acts(n, whole.act_dim, 7, t)
        ow = whole.step(a)[0]
        oh = [h.step(a[i * (n // 2):(i + 1) * (n // 2)])[0] for i, h in enumerate(halves)]
        om = masked.step_envs(np.ones(n, bool), a)[0]
        assert np.array_equal(ow, np.concatenate(oh)), t
        assert np.array_equal(ow, om), t
    sw, sm = _state(whole), _state(masked)
    _same(sw, sm, "all-true mask")
    for k in (0, 1):
        sh = np.concatenate([h.slots()[k] for h in halves])
        assert np.array_equal(sw[0][k].view(np.uint32), sh.view(np.uint32))
    # a masked subset: the envs outside it do not move
    m = np.zeros(n, bool)
    m[::3] = True
    before = _state(masked)
    masked.step_envs(m, _acts(n, whole.act_dim, 8, 0))
    after = _state(masked)
    for k in (0, 1):
        assert np.array_equal(after[0][k][~m].view(np.uint32), before[0][k][~m].view(np.uint32))
        assert not np.array_equal(after[0][k][m].view(np.uint32), before[0][k][m].view(np.uint32))
    for v in [whole, masked] + halves:
        v.close()


def test_snapshot_round_trip_and_other_mode_refused():
    chub = hub()
    n = 256
    v = chub.VecChargingHub(n, seed=3, rng="philox_curves", **HUB)
    v.reset()
    for t in range(5):
        v.step(_acts(n, v.act_dim, 2, t))
    blob = v.get_state()
    runs = []
    for _ in range(2):
        outs = [v.step(_acts(n, v.act_dim, 4, t))[0].copy() for t in range(3)]
        runs.append((outs, _state(v)))
        v.set_state(blob)
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(a, b)
    _same(runs[0][1], runs[1][1], "restore")
    for mode in ("philox", "compat"):
        other = chub.VecChargingHub(n, seed=3, rng=mode, **HUB)
        with pytest.raises(chub.ChubError, match="different configuration"):
            other.set_state(blob)
        with pytest.raises(chub.ChubError, match="different configuration"):
            v.set_state(other.get_state())
        other.close()
    v.close()


# ---------------------------------------------------------------------------------------------- 7. what the mode refuses / supports
def test_refusals_are_explicit():
    chub = hub()
    n = 8
    v = chub.VecChargingHub(n, seed=1, rng="philox_curves", slot_kernel="packed", fused_step="auto", **HUB)
    assert not v.uses_packed_kernel and not v.uses_fused_step
    v.reset()
    with pytest.raises(chub.ChubError, match=r"error -4: .*scalar-load control"):
        v.step_load(np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32))
    with pytest.raises(chub.ChubError, match=r"error -4: .*scalar-load control"):
        v.step_load_envs(np.ones(n, bool), np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32))
    with pytest.raises(chub.ChubError, match=r"error -4: .*car tape carries each arrival SoC"):
        v.tape_register_soc(np.array([40.0], np.float32))
    with pytest.raises(chub.ChubError, match=r"error -4: .*chub_set_slots"):
        v.set_slots(np.full((n, v.n_slots, 6), -1, np.int32))
    with pytest.raises(ValueError):
        chub.VecChargingHub(n, seed=1, rng="curves", **HUB)
    v.step(np.zeros((n, v.act_dim), np.float32))  # (the refused calls changed nothing the handle needs)
    v.close()


def test_step_bits_equals_float_rows():
    chub = hub()
    n = 300
    a_, b_ = (chub.VecChargingHub(n, seed=12, rng="philox_curves", **HUB) for _ in range(2))
    a_.reset()
    b_.reset()
    for t in range(20):
        act = _acts(n, a_.act_dim, 9, t)
        oa = a_.step(act)[0]
        ob = b_.step_bits(*b_.pack_actions(act))[0]
        assert np.array_equal(oa, ob), t
    _same(_state(a_), _state(b_), "bits")
    a_.close()
    b_.close()


def test_dropin_class_takes_the_mode():
    import charginghub_env_amd as chub
    env = chub.EvcsspManagerEnv_v6(HUB["station_list"], HUB["station_type_list"], rng="philox_curves", seed=5)
    env.reset()
    for _ in range(3):
        env.step(np.zeros(sum(HUB["station_list"]) + 2, np.float32))
    with pytest.raises(ValueError):
        chub.EvcsspManagerEnv_v6(HUB["station_list"], HUB["station_type_list"], rng="nope")
