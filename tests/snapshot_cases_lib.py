"""The designed cases of the snapshot tests -- numpy and the CPU oracle, no device.

chub_get_state / chub_set_state copy a handle's arena: the envs' state and, riding along, what the last launch made ahead of the next step
(the station draws pk / drw, in COMPAT the shadow streams and counts of a walk that ran ahead).  A restore that got one of the host-side flags
wrong (predrawn, per_env, rng_cur, graph_base ...) gives a plausible but wrong trajectory, and only where there is state for it to be wrong
about: cars waiting in front of the stations (so that the next step's admissions depend on the queue the draws are decoded against), a
forecourt list with entries, the folded tail of a stuck forecourt.  The cases below are chosen so that there is, at every moment a snapshot
is taken; tests/test_snapshot_cases_cpu.py asserts that on the oracle alone, tests/test_gpu_snapshots.py holds the device to
oracle_trajectory() across restores.

A run is PLAN = (100, 40): a reset, a whole day and four steps past `done` without a reset (MGR:271-299), a reset, 40 steps of a second day.
Steps are numbered over the run; a MOMENT is a position p = the number of steps done when the snapshot is taken (p = 0: right after the reset;
p = 60: the afternoon, cars waiting in front of busy stations and piles falling free; p = 96: the step that returned `done` was the last one;
p = 97: one step past it; p = 133: the morning rush of the second day).  The action script is _philox_parity's (tests/test_gpu_parity.py):
uniform(-1, 1) rows from RandomState(7), every pile on on every seventh step.

What a moment can hold is the day's: the tables' traffic is a daytime one, so at slot 0 (p = 96, 97) only a station of two or three piles
still has cars waiting, and a reset empties the forecourt list (hy_reset, HYD:197-208).  The population is designed so that at every moment
SOME case holds each kind of state, and at the two moments that are free to choose (mid_day, second_day) the [20, 25] cases hold cars
waiting and admit cars in the same step."""
import ctypes as C
import functools

import numpy as np

import orclib
from orclib import orc, ptr

SEED = 0xC0FFEE12345
ENV_ID0 = 1000
ACTION_SEED = 7
PLAN = (100, 40)
TOTAL = sum(PLAN)
MOMENTS = {"after_reset": 0, "mid_day": 60, "at_done": 96, "past_done": 97, "second_day": 133}
MIN_HITS = 4
ORACLE_RNG = {"philox": orclib.PHILOX, "philox_curves": orclib.PHILOX_CURVES}

T_HV_ARRIVE, T_HV_LINE, T_QUEUE_LEN = 19, 20, 21  # CHUB_T_* (include/chub.h)
SC_LINE = 4                                       # orc_station_scalars / chub_get_station_scalars: the cars waiting in front of the station

_BASE = dict(constant_charging=False, renew_fluctuate=0.0, price_fluctuate=0.0, hydro_loss=0.0)
# name: (hub kwargs, envs, RNG modes).  Batches of 64 .. 130 envs; the launch forms are forced through chub_options, not through the size.
CASES = {
    # packed kernel, k_step_tailwave, the COMPAT split step with walks ahead
    "c3": (dict(_BASE, station_list=[20, 25], station_type_list=["fast", "slow"], hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2,
                fc_max_power=100.0, fcev_permeate=0.05, renew_fluctuate=0.2, price_fluctuate=0.1), 70, ("philox", "philox_curves")),
    # PHILOX_CASES' fcev_stuck: the forecourt's FIFO gets stuck and the list is folded (q_fold, q_fold_cnt are non-empty state)
    "fcev_stuck": (dict(_BASE, station_list=[20, 25], station_type_list=["fast", "slow"], hydro_prod_rate=100.0, hydro_store_vlt=400.0, init_soc=0.6,
                        fc_max_power=100.0, fcev_permeate=0.1), 64, ("philox", "philox_curves")),
    # fewer than 8 piles: k_step_fused; evs_reset of a 3-pile fast station can record a negative flow_in (CHS.hpp:1276, 832-842, 1617)
    "small_fast": (dict(_BASE, station_list=[3, 2], station_type_list=["fast", "fast"], hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2,
                        fc_max_power=100.0, fcev_permeate=0.05), 130, ("philox", "philox_curves")),
    # the largest shape PHILOX_CURVES and the one-launch forms take
    "max64": (dict(_BASE, station_list=[64, 64], station_type_list=["slow", "fast"], hydro_prod_rate=2000.0, hydro_store_vlt=5000.0, init_soc=0.5,
                   fc_max_power=100.0, fcev_permeate=0.2, hydro_loss=0.001), 65, ("philox", "philox_curves")),
    # units spanning waves (PHILOX and COMPAT only)
    "big_100_70": (dict(_BASE, station_list=[100, 70], station_type_list=["fast", "slow"], hydro_prod_rate=2000.0, hydro_store_vlt=5000.0,
                        init_soc=0.5, fc_max_power=100.0, fcev_permeate=0.05), 64, ("philox",)),
}
STUCK = "fcev_stuck"
CASE_MODES = [(name, rng) for name, (_, _, modes) in CASES.items() for rng in modes]


def case(name):
    kw, n, _ = CASES[name]
    return dict(kw), n


def dims(name):
    kw, n = case(name)
    s0, s1 = kw["station_list"]
    return n, s0, s1, s0 + s1 + 2, 2 + 4 * 2 + 3  # envs, piles, piles, action columns, observation columns


@functools.lru_cache(maxsize=None)
def action_script(name):
    """[TOTAL, n, A] f32, read-only: step i of the run takes action_script(name)[i]"""
    n, s0, s1, A, _ = dims(name)
    rs = np.random.RandomState(ACTION_SEED)
    acts = np.zeros((TOTAL, n, A), dtype=np.float32)
    for i in range(TOTAL):
        acts[i] = rs.uniform(-1, 1, size=(n, A)).astype(np.float32)
        if i % 7 == 0:
            acts[i, :, :s0 + s1] = 1.0
    acts.setflags(write=False)
    return acts


@functools.lru_cache(maxsize=None)
def other_actions(name):
    """[5, n, A] f32: what a handle is stepped with after its snapshot was taken, so that its arena and flags are those of another run"""
    n, _, _, A, _ = dims(name)
    acts = np.random.RandomState(ACTION_SEED + 1).uniform(-1, 1, size=(5, n, A)).astype(np.float32)
    acts.setflags(write=False)
    return acts


def episode_of(i):
    """step i of the run -> (episode, step of the episode)"""
    return (0, i) if i < PLAN[0] else (1, i - PLAN[0])


def explicit_capacity(fcev_permeate):
    """the entries of the FCEV waiting list the device keeps one by one (HubParams::qcap): 2 m - 1 with m the most arrivals a step can bring,
    round(0.3 * permeate * the largest arrival index of any slot of the day) (CHS:765-780) -- a longer list is a stuck one, kept folded"""
    m = max(orc.orc_count_hv(orc.orc_arrival_index(orclib.tables(), t, 999), 0.3, float(fcev_permeate)) for t in range(96))
    return max(1, 2 * m - 1)


class Trajectory(object):
    """what the oracle leaves after every call of the uninterrupted run"""

    def __init__(self, name):
        n, s0, s1, _, D = dims(name)
        self.reset_obs = np.zeros((len(PLAN), n, D))
        self.reset_scalars = np.zeros((len(PLAN), n, 2, 8))
        self.reset_slots = [np.zeros((len(PLAN), n, 9, s), dtype=np.float32) for s in (s0, s1)]
        self.slots = [np.zeros((TOTAL, n, 9, s), dtype=np.float32) for s in (s0, s1)]
        self.scalars = np.zeros((TOTAL, n, 2, 8))
        self.tel = np.zeros((TOTAL, n, 38))
        self.obs = np.zeros((TOTAL, n, D))
        self.reward = np.zeros((TOTAL, n))
        self.done = np.zeros((TOTAL, n), dtype=bool)
        self.overflow = 0

    def arrays(self):
        return [self.reset_obs, self.reset_scalars, self.scalars, self.tel, self.obs, self.reward, self.done] + self.reset_slots + self.slots

    def state_at(self, p):
        """(slots per station, station scalars, telemetry or None) as position p finds them: after the reset (p = 0) or after step p - 1"""
        if p == 0:
            return [s[0] for s in self.reset_slots], self.reset_scalars[0], None
        assert p != PLAN[0], "position %d is the last step of day one; the second day's reset comes before step %d" % (p, p)
        return [s[p - 1] for s in self.slots], self.scalars[p - 1], self.tel[p - 1]


@functools.lru_cache(maxsize=None)
def oracle_trajectory(name, rng="philox"):
    """The oracle (PHILOX or PHILOX_CURVES back-end) through the whole run, uninterrupted: what _philox_parity compares -- obs, reward, done,
    slots, station scalars, telemetry -- after every call.  Computed once per process and left unchanged."""
    kw, n = case(name)
    cfg = orclib.make_config(piles=kw["station_list"], types=kw["station_type_list"],
                             **{k: kw[k] for k in kw if k not in ("station_list", "station_type_list")})
    h = orc.orc_vec_create(C.byref(cfg), orclib.tables(), n, ENV_ID0, ORACLE_RNG[rng], SEED)
    assert h
    tr = Trajectory(name)
    acts = action_script(name)
    o_obs, o_rew, o_done = np.zeros_like(tr.obs[0]), np.zeros(n), np.zeros(n, dtype=np.uint8)
    for i in range(TOTAL):
        ep, t = episode_of(i)
        if t == 0:
            orc.orc_vec_reset(h, None, None, ptr(tr.reset_obs[ep]))
            orc.orc_vec_station_scalars(h, ptr(tr.reset_scalars[ep]))
            for k in (0, 1):
                orc.orc_vec_slots(h, k, ptr(tr.reset_slots[k][ep]))
        orc.orc_vec_step(h, ptr(acts[i]), None, ptr(o_obs), ptr(o_rew), ptr(o_done), 4)
        tr.obs[i], tr.reward[i], tr.done[i] = o_obs, o_rew, o_done.astype(bool)
        for k in (0, 1):
            orc.orc_vec_slots(h, k, ptr(tr.slots[k][i]))
        orc.orc_vec_station_scalars(h, ptr(tr.scalars[i]))
        orc.orc_vec_telemetry(h, ptr(tr.tel[i]))
        tr.overflow |= orc.orc_vec_overflow(h)
    orc.orc_vec_destroy(h)
    for a in tr.arrays():
        a.setflags(write=False)
    return tr


def coverage(name, rng, p):
    """what a snapshot at position p has to get right, counted on the oracle: station units with cars waiting, envs with a non-empty FCEV
    waiting list, envs whose list is longer than the device keeps entry by entry, and the cars step p admits (piles empty before it and
    occupied after: the draws made ahead are consumed)"""
    tr = oracle_trajectory(name, rng)
    kw, _ = case(name)
    slots, scalars, tel = tr.state_at(p)
    queue = np.zeros(scalars.shape[0]) if tel is None else tel[:, T_QUEUE_LEN]
    admitted = sum(int(((before[:, 0] == 0) & (tr.slots[k][p][:, 0] == 1)).sum()) for k, before in enumerate(slots))
    return {"units_with_line": int((scalars[:, :, SC_LINE] > 0).sum()), "envs_with_fcev_list": int((queue > 0).sum()),
            "envs_with_folded_list": int((queue > explicit_capacity(kw["fcev_permeate"])).sum()), "admitted_next_step": admitted}
