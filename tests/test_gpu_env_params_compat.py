"""Per-env hub parameters in COMPAT mode (include/chub.h, chub_create_params): nine reference fixtures, each recorded from the unmodified
reference with its own constructor kwargs, run side by side in ONE handle -- each env with its own row, its own constructor seeds and
chub_compat_replay_constructor, then its own program of reseeds, resets and steps on its own clock.  Every env must equal its recorded
single-env run at the bars of test_compat_matches_reference_golden: slots and station sums bit for bit, observation and reward to 1e-9,
hy_power_speed_list to 1e-13.  The references are the fixtures (tests/golden), not this code."""
import numpy as np
import pytest

import orclib
from test_gpu_parity import TIGHT, check_slots, close, kwargs_of

pytestmark = pytest.mark.gpu

FIXTURES = ["env_c1_envtest", "env_c3_random", "env_defaults", "env_fcev_queue", "env_fcev_queue_deep", "env_no_electrolyser", "env_past_done",
            "env_permeate_cap", "env_tank_floor"]
FIELDS = ("hydro_prod_rate", "hydro_store_vlt", "init_soc", "fc_max_power", "fcev_permeate", "renew_fluctuate", "price_fluctuate", "hydro_loss")


def hub():
    import charginghub_env_amd as chub
    return chub


def program(g):
    """the fixture's calls: the constructor's reset (MGR:120), then per episode a reset (after a reseed where the fixture has one) and its steps"""
    prog = [("reset", g["ctor_days"], g["ctor_z"], None)]
    i = 0
    for ep in range(int(g["episodes"])):
        prog.append(("reset", g["reset_days"][ep], g["reset_z"][ep], ep))
        for _ in range(int(g["steps_per_episode"])):
            prog.append(("step", i))
            i += 1
    return prog, i


# A handle with rows runs one COMPAT form at every batch size (one kernel per station, the unit's first lane walking the streams:
# chub_launch_plan_params); the sizes exercise one tail workgroup and several
@pytest.mark.parametrize("repeat", [1, 40])
def test_nine_reference_fixtures_in_one_compat_handle(repeat):
    chub = hub()
    gs = [orclib.load_golden(name) for name in FIXTURES]
    kws = [kwargs_of(g) for g in gs]
    for name, kw in zip(FIXTURES, kws):
        assert kw["station_list"] == [20, 25] and kw["station_type_list"] == ["fast", "slow"] and not kw["constant_charging"], name
    assert len({tuple(kw[f] for f in FIELDS) for kw in kws}) == 8  # (two of the nine fixtures were recorded with the same kwargs)
    n = len(FIXTURES) * repeat
    fx = np.arange(n) % len(FIXTURES)  # env e runs fixture fx[e]
    rows = {f: [kws[k][f] for k in fx] for f in FIELDS}
    v = chub.VecChargingHub(n, rng="compat", station_list=[20, 25], station_type_list=["fast", "slow"], **rows)
    assert v.has_env_params and not v.uses_fused_step
    scratch = chub.VecChargingHub(1, rng="compat", **kws[0])  # turns a seed pair into stream states
    v.set_telemetry(True)
    A = v.act_dim
    v.set_compat_seeds(np.stack([gs[k]["ctor_seeds"] for k in fx]))
    v.compat_replay_constructor()  # each env the reference's constructor with its own kwargs and streams
    for e in range(n):
        g = gs[fx[e]]
        close(v.hy_table(env=e), g["hy_table"], (FIXTURES[fx[e]], "hy_table", e), rtol=1e-13, atol=1e-12)
    progs = [program(g) for g in gs]
    seeds = [{int(ep): (int(a), int(b)) for ep, a, b in g["seeds"]} for g in gs]
    longest = max(len(p) for p, _ in progs)
    checked = np.zeros(n, dtype=np.int64)
    for tau in range(longest):
        ops = {e: progs[fx[e]][0][tau] for e in range(n) if tau < len(progs[fx[e]][0])}
        resets = [e for e, op in ops.items() if op[0] == "reset"]
        movers = [e for e, op in ops.items() if op[0] == "step"]
        if resets:
            mask = np.zeros(n, dtype=bool)
            days, z = np.zeros((n, 2), dtype=np.int32), np.zeros((n, 3))
            st = None
            for e in resets:
                _, d_, z_, ep = ops[e]
                if ep is not None and ep in seeds[fx[e]]:  # e.seed() / srand() of this env only
                    scratch.set_compat_seeds([seeds[fx[e]][ep]])
                    st = v.compat_state() if st is None else st
                    st[e] = scratch.compat_state()[0]
                mask[e], days[e], z[e] = True, d_, z_
            if st is not None:
                v.set_compat_state(st)
            v.reset_envs(mask, days, z)
            o64, sc = v.obs_f64(), v.station_scalars()
            for e in resets:
                ep, g, name = ops[e][3], gs[fx[e]], FIXTURES[fx[e]]
                if ep is None:
                    continue
                close(o64[e], g["reset_obs"][ep], (name, "reset obs", e, ep), rtol=TIGHT, atol=TIGHT)
                got = np.concatenate([sc[e, 0, :6], sc[e, 1, :6]])
                assert np.array_equal(got, g["reset_stations"][ep]), (name, "reset stations", e, ep, got)
        if movers:
            mask = np.zeros(n, dtype=bool)
            act, z = np.zeros((n, A), dtype=np.float32), np.zeros((n, 3))
            for e in movers:
                k, g = ops[e][1], gs[fx[e]]
                mask[e], act[e], z[e] = True, g["action"][k], g["exo_z"][k]
            obs, rew, done, _ = v.step_envs(mask, act, z)
            sl, sc, tel, o64, r64 = v.slots(), v.station_scalars(), v.telemetry(), v.obs_f64(), v.reward_f64()
            for e in movers:
                k, g, name = ops[e][1], gs[fx[e]], FIXTURES[fx[e]]
                check_slots(sl[0][e], g["slots0"][k], (name, e, k, "station0"))
                check_slots(sl[1][e], g["slots1"][k], (name, e, k, "station1"))
                got = np.concatenate([sc[e, 0, :6], sc[e, 1, :6]])
                assert np.array_equal(got, g["stations"][k]), (name, e, k, got, g["stations"][k])
                assert bool(done[e]) == bool(g["done"][k])
                assert np.array_equal(tel[e, 19:22], g["telem"][k][19:22]), (name, e, k, "fcev ints")
                close(o64[e], g["obs"][k], (name, "obs", e, k), rtol=TIGHT, atol=TIGHT)
                close(r64[e], g["reward"][k], (name, "reward", e, k), rtol=TIGHT, atol=TIGHT)
                close(tel[e, :19], g["telem"][k][:19], (name, "telemetry", e, k), rtol=TIGHT, atol=1e-7)
                checked[e] += 1
    for e in range(n):
        assert checked[e] == progs[fx[e]][1], (FIXTURES[fx[e]], e)
    v.close()
    scratch.close()


def test_compat_rows_equal_to_cfg_are_the_homogeneous_handle():
    """rows all equal to the config: every env as in a homogeneous COMPAT handle on the same form (one kernel per station), bit for bit,
    constructor replay included"""
    chub = hub()
    g = orclib.load_golden("env_fcev_queue")
    kw = kwargs_of(g)
    n = 300
    rows = {f: [kw[f]] * n for f in FIELDS}
    hs = [chub.VecChargingHub(n, rng="compat", seed=4, slot_kernel="wave", **kw),
          chub.VecChargingHub(n, rng="compat", seed=4, station_list=kw["station_list"], station_type_list=kw["station_type_list"], **rows)]
    rs = np.random.RandomState(2)
    for v in hs:
        v.compat_replay_constructor()
    for e in range(0, n, 37):
        assert np.array_equal(hs[0].hy_table(env=e).view(np.uint64), hs[1].hy_table(env=e).view(np.uint64)), e
    days = np.stack([rs.randint(0, 100, n), rs.randint(0, 150, n)], axis=1).astype(np.int32)
    z = rs.normal(size=(n, 3))
    outs = [v.reset(days, z) for v in hs]
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    for t in range(120):
        a = rs.uniform(-1, 1, (n, hs[0].act_dim)).astype(np.float32)
        z = rs.normal(size=(n, 3))
        if t == 60:
            outs = [v.reset(days, z) for v in hs]
            assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
            continue
        o = [v.step(a, z) for v in hs]
        for j in range(3):
            assert np.array_equal(np.asarray(o[0][j]).view(np.uint8), np.asarray(o[1][j]).view(np.uint8)), (t, j)
    for k in (0, 1):
        assert np.array_equal(hs[0].slots()[k].view(np.uint32), hs[1].slots()[k].view(np.uint32))
    assert np.array_equal(hs[0].station_scalars(), hs[1].station_scalars())
    for v in hs:
        v.close()
