"""A designed population for the per-env tail (env_tail, csrc/chub_kernels.hip) and its script -- numpy and the CPU oracle, no device.

The PHILOX parity cases drive the tail with uniform(-1, 1) actions and never take its rare branches: the tank at the brim, the fuel cell
limited by the hydrogen left or at fc_max_power, the grid clamp that finds index 0 and wraps to full power (MGR:168), a hub without an
electrolyser.  Here six hub configurations and a script of tail actions take them by design, on one hub shape -- two fast stations of 64
piles: full-on charging exceeds the 2000 kW grid limit, and every one-launch and span form takes stations of at most 64 piles.

Env i takes config i // 16 (N = 96, global env id ENV_ID0 + i).  The action tensor has period 8: actions(t) = batch[t % 8] -- what
chub_run_steps takes for its spans -- so the same eight arrays drive every launch form and the oracle.

tests/test_tail_cases_cpu.py asserts on the oracle alone that every config reaches its branches (MUST_REACH, at least MIN_HITS times);
tests/test_gpu_tail_cases.py holds the device to oracle_trajectory() in every form of the tail."""
import ctypes as C
import functools

import numpy as np

import orclib
from orclib import orc, ptr

HUB = dict(station_list=[64, 64], station_type_list=["fast", "fast"])
S = 128            # piles of the hub
A = S + 2          # an action row: the piles, then the electrolyser and the fuel-cell action (MGR:395-403)
D = 13             # 2 + 4 * 2 + 3
BLOCK = 16         # envs per config
PERIOD = 8         # action batches (chub_run_steps takes at most 8)
SEED = 0xC0FFEE12345
ENV_ID0 = 1000
ACTION_SEED = 20260
PLAN = (96, 40)    # reset + a day, reset + a cut-short episode
MIN_HITS = 4

FIELDS = ("hydro_prod_rate", "hydro_store_vlt", "init_soc", "fc_max_power", "fcev_permeate", "renew_fluctuate", "price_fluctuate", "hydro_loss")
DEFAULTS = dict(renew_fluctuate=0.0, price_fluctuate=0.0, hydro_loss=0.0)

# name, the eight scalars (DEFAULTS where not given), the tail script (electrolyser, fuel cell; None = free), piles all on / free
CONFIGS = [
    ("brim", dict(hydro_prod_rate=430.0, hydro_store_vlt=5.0, init_soc=1.0, fc_max_power=100.0, fcev_permeate=0.01), (1.0, None), False),
    ("h2_limited", dict(hydro_prod_rate=100.0, hydro_store_vlt=5.0, init_soc=0.1, fc_max_power=1000.0, fcev_permeate=0.0), (-1.0, 1.0), True),
    ("no_electrolyser", dict(hydro_prod_rate=0.0, hydro_store_vlt=25.0, init_soc=0.2, fc_max_power=100.0, fcev_permeate=0.01), (None, None), False),
    ("grid_wrap", dict(hydro_prod_rate=430.0, hydro_store_vlt=5000.0, init_soc=0.5, fc_max_power=100.0, fcev_permeate=0.01), (0.5, None), True),
    ("renew_covers", dict(hydro_prod_rate=10.0, hydro_store_vlt=5000.0, init_soc=0.5, fc_max_power=100.0, fcev_permeate=0.0), (-0.9, -1.0), False),
    ("loss_permeate", dict(hydro_prod_rate=430.0, hydro_store_vlt=400.0, init_soc=0.6, fc_max_power=100.0, fcev_permeate=1.5,
                           renew_fluctuate=0.3, price_fluctuate=0.3, hydro_loss=0.02), (None, None), False),
]
NAMES = [c[0] for c in CONFIGS]
N = BLOCK * len(CONFIGS)

# the branches each config must reach on the oracle at least MIN_HITS times ("every": on every step; "half": on more than half its steps)
MUST_REACH = {
    "brim": {"brim": MIN_HITS, "renew_covers": MIN_HITS, "fc_takes_all": MIN_HITS},
    "h2_limited": {"h2_limited": MIN_HITS, "fc_at_max": MIN_HITS, "floor": MIN_HITS},
    "no_electrolyser": {"no_gen": "every", "not_meet": MIN_HITS, "fc_on": MIN_HITS},
    "grid_wrap": {"clamp": MIN_HITS, "grid_wrap": MIN_HITS},
    "renew_covers": {"renew_covers": "half"},
    "loss_permeate": {"clamp": MIN_HITS, "grid_pays": MIN_HITS},
}

# telemetry columns, the CHUB_T_* enum of include/chub.h in order
T_NAMES = ["HY_ACT", "HY_FLOW_SPEED", "ALL_POWER_SECOND", "STORE_SOC", "CAPACITY", "TOTAL_MASS_NEED", "HY_USE", "NOT_MEET", "FC_POWER", "HY_TO_USE",
           "USED_RENEW", "EV0", "EV1", "HYDROGEN_POWER", "INCOME", "REWARD", "RE_PV", "RE_WD", "PRICE_NEXT", "HV_ARRIVE", "HV_LINE", "QUEUE_LEN",
           "PV_DAY", "WD_DAY", "EV0_NET", "EV1_NET", "EV_SUM_NET", "PRICE_NOW", "MIN0", "CHG0", "MAX0", "LINE0", "FLOW0", "MIN1", "CHG1", "MAX1",
           "LINE1", "FLOW1"]
T = {name: i for i, name in enumerate(T_NAMES)}
T_COUNT = len(T_NAMES)
FLAGS = ("clamp", "grid_wrap", "brim", "floor", "not_meet", "no_gen", "renew_covers", "grid_pays", "fc_on", "fc_takes_all", "fc_at_max", "h2_limited")


def config_of(env):
    return env // BLOCK


def config_kwargs(k):
    """config k's eight scalars, defaults filled in"""
    kw = dict(DEFAULTS)
    kw.update(CONFIGS[k][1])
    return kw


def configs():
    """per block: (name, the constructor kwargs of a homogeneous handle / the oracle's config: the hub shape + the eight scalars)"""
    return [(CONFIGS[k][0], dict(HUB, constant_charging=False, **config_kwargs(k))) for k in range(len(CONFIGS))]


def rows():
    """the eight per-env kwargs as sequences of N values, for chub_create_params (VecChargingHub takes them as they are)"""
    return {f: [config_kwargs(config_of(i))[f] for i in range(N)] for f in FIELDS}


@functools.lru_cache(maxsize=None)
def action_batches():
    """[PERIOD, N, A] f32: free entries uniform(-1, 1) from a seeded RandomState, scripted entries as CONFIGS says"""
    rs = np.random.RandomState(ACTION_SEED)
    batch = rs.uniform(-1, 1, size=(PERIOD, N, A)).astype(np.float32)
    for k, (_, _, (a_el, a_fc), all_on) in enumerate(CONFIGS):
        sel = slice(k * BLOCK, (k + 1) * BLOCK)
        if all_on:
            batch[:, sel, :S] = 1.0
        if a_el is not None:
            batch[:, sel, S] = a_el
        if a_fc is not None:
            batch[:, sel, S + 1] = a_fc
    batch.setflags(write=False)
    return batch


def actions(t):
    """the [N, A] action batch of step t (counted over the whole run, or within a day: 96 is a multiple of PERIOD)"""
    return action_batches()[t % PERIOD]


def classify(tel, a_el, a_fc, fc_max_power):
    """Which branches of the tail an env-step took: tel [..., 38] telemetry (CHUB_T_* order) of the step, a_el / a_fc the step's two tail
    actions as given (f32), fc_max_power the env's.  Returns {flag: bool array of tel's leading shape}."""
    tel = np.asarray(tel, dtype=np.float64)
    c = lambda name: tel[..., T[name]]
    want = (np.asarray(a_el, dtype=np.float32).astype(np.float64) + 1) / 2
    fc = c("FC_POWER")
    out = {
        "clamp": c("HY_ACT") != want,
        "brim": c("STORE_SOC") == 1,
        "floor": c("STORE_SOC") == 0.1,
        "not_meet": c("NOT_MEET") > 0,
        "no_gen": c("HY_FLOW_SPEED") <= 0.5,
        "renew_covers": (c("HYDROGEN_POWER") == 0) & (c("ALL_POWER_SECOND") > 0),
        "grid_pays": c("HYDROGEN_POWER") > 0,
        "fc_on": fc > 0,
        "fc_takes_all": (fc > 0) & (c("EV_SUM_NET") == 0),
        "fc_at_max": fc == np.asarray(fc_max_power, dtype=np.float64),
        "h2_limited": (fc > 0) & (c("HY_TO_USE") < fc * 1500 / 119.6),
    }
    out["grid_wrap"] = out["clamp"] & (c("HY_ACT") == 1.0)
    return out


def flags_of(flags, index):
    """the names of the flags set at `index` of classify()'s arrays: what a failing comparison prints"""
    return [f for f in FLAGS if flags[f][index]]


FC_MAX = np.array([config_kwargs(config_of(i))["fc_max_power"] for i in range(N)])


class Trajectory(object):
    """what the oracle leaves after every call of a script; steps are numbered over the whole run (sum(plan)).  The defaults are this
    population's: N envs of HUB through PLAN."""

    def __init__(self, steps, n=N, piles=None, d=D, episodes=len(PLAN)):
        piles = HUB["station_list"] if piles is None else piles
        self.reset_obs = np.zeros((episodes, n, d))
        self.reset_scalars = np.zeros((episodes, n, 2, 8))
        self.slots = [np.zeros((steps, n, 9, piles[k]), dtype=np.float32) for k in (0, 1)]
        self.scalars = np.zeros((steps, n, 2, 8))
        self.tel = np.zeros((steps, n, T_COUNT))
        self.obs = np.zeros((steps, n, d))
        self.reward = np.zeros((steps, n))
        self.done = np.zeros((steps, n), dtype=bool)
        self.q_overflow = 0
        self.flags = None

    def freeze(self):
        for a in [self.reset_obs, self.reset_scalars, self.scalars, self.tel, self.obs, self.reward, self.done] + self.slots:
            a.setflags(write=False)


def step_plan(plan=PLAN):
    """[(episode, step of the episode, step of the run)]"""
    out, i = [], 0
    for ep, steps in enumerate(plan):
        for t in range(steps):
            out.append((ep, t, i))
            i += 1
    return out


def run_oracle(cfgs, batches, plan, block, env_id0, seed, fc_max):
    """One oracle vec per entry of cfgs ([(name, hub shape + the eight scalars)], PHILOX back-end, `block` envs each at env_id0 + block * k)
    through reset + plan[0] steps, reset + plan[1] steps, ...; step i of the run takes batches[i % len(batches)] ([.., block * len(cfgs), A]
    f32).  Returns the frozen Trajectory, its flags classified with fc_max ([n])."""
    vecs = []
    for k, (name, kw) in enumerate(cfgs):
        cfg = orclib.make_config(piles=kw["station_list"], types=kw["station_type_list"],
                                 **{f: kw[f] for f in kw if f not in ("station_list", "station_type_list")})
        h = orc.orc_vec_create(C.byref(cfg), orclib.tables(), block, env_id0 + block * k, orclib.PHILOX, seed)
        assert h
        vecs.append((cfg, h))
    piles = list(cfgs[0][1]["station_list"])
    assert all(list(kw["station_list"]) == piles for _, kw in cfgs)
    n, d, s = block * len(cfgs), orc.orc_env_obs_dim(C.byref(vecs[0][0])), sum(piles)
    assert batches.shape[1:] == (n, s + 2) and batches.dtype == np.float32
    tr = Trajectory(sum(plan), n, piles, d, len(plan))
    o_obs, o_rew, o_done = np.zeros((block, d)), np.zeros(block), np.zeros(block, dtype=np.uint8)

    def records(dst_scalars):
        for k, (_, h) in enumerate(vecs):
            orc.orc_vec_station_scalars(h, ptr(dst_scalars[k * block:(k + 1) * block]))
            for e in range(block):
                tr.q_overflow += orc.orc_env_q_overflow(orc.orc_vec_env(h, e))

    i = 0
    for ep, steps in enumerate(plan):
        for k, (_, h) in enumerate(vecs):
            orc.orc_vec_reset(h, None, None, ptr(o_obs))
            tr.reset_obs[ep, k * block:(k + 1) * block] = o_obs
        records(tr.reset_scalars[ep])
        for t in range(steps):
            act = batches[i % len(batches)]
            for k, (_, h) in enumerate(vecs):
                sel = slice(k * block, (k + 1) * block)
                a = np.ascontiguousarray(act[sel])
                orc.orc_vec_step(h, ptr(a), None, ptr(o_obs), ptr(o_rew), ptr(o_done), 1)
                tr.obs[i, sel], tr.reward[i, sel], tr.done[i, sel] = o_obs, o_rew, o_done.astype(bool)
                for st in (0, 1):
                    orc.orc_vec_slots(h, st, ptr(tr.slots[st][i, sel]))
                orc.orc_vec_telemetry(h, ptr(tr.tel[i, sel]))
            records(tr.scalars[i])
            i += 1
    for _, h in vecs:
        orc.orc_vec_destroy(h)
    a_el = np.stack([batches[j % len(batches)][:, s] for j in range(i)])
    a_fc = np.stack([batches[j % len(batches)][:, s + 1] for j in range(i)])
    tr.flags = classify(tr.tel, a_el, a_fc, np.asarray(fc_max)[None, :])
    tr.freeze()
    return tr


@functools.lru_cache(maxsize=None)
def oracle_trajectory():
    """Six oracle vecs (PHILOX back-end, 16 envs each at ENV_ID0 + 16 k) through reset + 96 steps + reset + 40 steps of the script.
    Computed once per process and left unchanged."""
    return run_oracle(configs(), action_batches(), PLAN, BLOCK, ENV_ID0, SEED, FC_MAX)


def branch_counts(tr=None):
    """{config: {flag: env-steps of the run on which the oracle took it}} and the env-steps per config"""
    tr = tr or oracle_trajectory()
    out = {}
    for k, name in enumerate(NAMES):
        sel = slice(k * BLOCK, (k + 1) * BLOCK)
        out[name] = {f: int(tr.flags[f][:, sel].sum()) for f in FLAGS}
    return out, sum(PLAN) * BLOCK
