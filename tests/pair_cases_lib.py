"""Designed populations for the PAIRED tail launch (k_env_pair, k_pair_draws: chub_run_steps on a handle with chub_options.span_steps >= 2 on the
two-launch step) and their scripts -- numpy and the CPU oracle, no device.

A pair runs the tails of steps i and i + 1 in one launch: the second step takes the env's carried state from the first step's registers, not
from memory.  Whatever is held to the oracle must therefore be reached at BOTH positions of a pair.  A pair never straddles a day's end and a
day's first step can only be a pair's first step, so with the two alignments of tests/test_gpu_pair_cases.py (calls of two from the day's
step 0, or from its step 1) the steps that occupy both positions are those from an episode's second to its last but one: both_positions().
The coverage conditions of tests/test_pair_cases_cpu.py count there and nowhere else.

Part 1 -- the tail's rare branches.  The hub shape, block size, period-8 batches, classifier and oracle plumbing are tests/tail_cases_lib.py's;
the configs and the script are this file's, because tail_cases_lib's population reaches fc_at_max and grid_wrap on a day's FIRST step only
(steps 0 and 96 of its run), where no pair's second step can be.  Differences from tail_cases_lib.CONFIGS:
  h2_limited       the electrolyser action alternates over the batches, so that the tank leaves its floor and returns to it;
  no_electrolyser  the fuel-cell action is 1: fc_at_max and h2_limited after the first step;
  grid_wrap        the piles follow a per-batch script: see "grid_wrap" below.
A script entry is None (free: uniform(-1, 1) per env and batch), a number (every batch) or a tuple of PERIOD numbers / Nones (per batch).

Part 2 -- the forecourt: FORECOURT, the fcev_stuck config of tests/test_gpu_parity.py, 16 envs, seed 31, a day and twelve steps, uniform actions.
Part 3 -- the XCD-aware order of the level lanes: XCD_HUBS at 2048 and 4096 envs, XCD_PROGRAM.

grid_wrap (the clamp search finds index 0 and wraps to full power) needs charging >= 2000 kW + renewables, which 128 fast piles give only when
many cars that have not charged yet are switched on at once.  Scripts tried for the piles of the grid_wrap block, with the env-steps on the
branch at both_positions() (16 envs, this seed; "-" piles all off, "+" all on, one sign per batch):
  + + + + + + + +   0 (tail_cases_lib's script: the day's first step only)      - - - - - - + +   3 (steps 38, 134)
  - - - - - - - +   0 (step 135, an episode's last step, only)                   - - - + - - - +   0          - - + - - + - +   0
  - + - + - + - +   13 (steps 1 and 97)      - + + - - - + +   13      - + - - - - - +   13      - + - - - - + +   13 (taken)
The cars that reset() leaves are the reserve: one idle step and then every pile on reaches the branch on an episode's SECOND step -- the second
step of the pair (0, 1) in one alignment, the first step of the pair (1, 2) in the other -- in 7 of the 16 envs at step 1 and 6 at step 97.
With an electrolyser action of 1.0 in place of 0.5, the scripts - - - - - - + + and - - - - - - - + gave 0 (full power asked for and run is no
clamp).  The bar stays at MIN_HITS.

At 2048 envs (one level workgroup per XCD and segment) level_lane's XCD-aware order IS the plain order, lane for lane; the two differ from
4096 envs on.  Both sizes run both branches of the code; only 4096 can tell a lane of one order from the same lane of the other."""
import functools

import numpy as np

import tail_cases_lib as tc
from tail_cases_lib import A, BLOCK, D, ENV_ID0, FLAGS, HUB, MIN_HITS, PERIOD, PLAN, S, SEED, classify, flags_of  # noqa: F401 (the shared shape)

ACTION_SEED = 20261

# name, the eight scalars (tail_cases_lib.DEFAULTS where not given), the script: electrolyser, fuel cell, piles
CONFIGS = [
    ("brim", dict(hydro_prod_rate=430.0, hydro_store_vlt=5.0, init_soc=1.0, fc_max_power=100.0, fcev_permeate=0.01), (1.0, None, None)),
    ("h2_limited", dict(hydro_prod_rate=100.0, hydro_store_vlt=5.0, init_soc=0.1, fc_max_power=1000.0, fcev_permeate=0.0),
     ((1.0, -1.0, -1.0, 1.0, -1.0, -1.0, -1.0, 1.0), 1.0, 1.0)),
    ("no_electrolyser", dict(hydro_prod_rate=0.0, hydro_store_vlt=25.0, init_soc=0.2, fc_max_power=100.0, fcev_permeate=0.01), (None, 1.0, None)),
    ("grid_wrap", dict(hydro_prod_rate=430.0, hydro_store_vlt=5000.0, init_soc=0.5, fc_max_power=100.0, fcev_permeate=0.01),
     (0.5, None, (-1.0, 1.0, -1.0, -1.0, -1.0, -1.0, 1.0, 1.0))),
    ("renew_covers", dict(hydro_prod_rate=10.0, hydro_store_vlt=5000.0, init_soc=0.5, fc_max_power=100.0, fcev_permeate=0.0), (-0.9, -1.0, None)),
    ("loss_permeate", dict(hydro_prod_rate=430.0, hydro_store_vlt=400.0, init_soc=0.6, fc_max_power=100.0, fcev_permeate=1.5,
                           renew_fluctuate=0.3, price_fluctuate=0.3, hydro_loss=0.02), (None, None, None)),
]
NAMES = [c[0] for c in CONFIGS]
K = len(CONFIGS)
N = BLOCK * K

# the branches each config must reach on the oracle on at least MIN_HITS env-steps that occupy both positions of a pair
MUST_REACH = {
    "brim": ("brim", "renew_covers", "fc_takes_all"),
    "h2_limited": ("h2_limited", "floor", "fc_on"),
    "no_electrolyser": ("no_gen", "not_meet", "fc_on", "fc_at_max", "h2_limited"),
    "grid_wrap": ("clamp", "grid_wrap"),
    "renew_covers": ("renew_covers",),
    "loss_permeate": ("clamp", "grid_pays"),
}
GRID_WRAP_MIN = MIN_HITS
# a pair whose first step is on the branch and whose second is off it, and the reverse: (config, flag), at least MIN_HITS times each way
MUST_FLIP = (("brim", "brim"), ("h2_limited", "floor"), ("grid_wrap", "clamp"))


def config_kwargs(k):
    kw = dict(tc.DEFAULTS)
    kw.update(CONFIGS[k][1])
    return kw


def configs():
    """per block: (name, the constructor kwargs of a homogeneous handle / the oracle's config)"""
    return [(CONFIGS[k][0], dict(HUB, constant_charging=False, **config_kwargs(k))) for k in range(K)]


def _per_batch(entry):
    return list(entry) if isinstance(entry, tuple) else [entry] * PERIOD


@functools.lru_cache(maxsize=None)
def action_batches():
    """[PERIOD, N, A] f32: free entries uniform(-1, 1) from a seeded RandomState, scripted entries as CONFIGS says"""
    rs = np.random.RandomState(ACTION_SEED)
    batch = rs.uniform(-1, 1, size=(PERIOD, N, A)).astype(np.float32)
    for k, (_, _, (a_el, a_fc, piles)) in enumerate(CONFIGS):
        sel = slice(k * BLOCK, (k + 1) * BLOCK)
        for b in range(PERIOD):
            for col, entry in ((slice(0, S), piles), (S, a_el), (S + 1, a_fc)):
                v = _per_batch(entry)[b]
                if v is not None:
                    batch[b, sel, col] = v
    batch.setflags(write=False)
    return batch


def actions(t):
    return action_batches()[t % PERIOD]


FC_MAX = np.array([config_kwargs(i // BLOCK)["fc_max_power"] for i in range(N)])


@functools.lru_cache(maxsize=None)
def oracle_trajectory():
    """six oracle vecs through PLAN (reset + 96 steps, reset + 40) of this file's script; computed once per process and left unchanged"""
    return tc.run_oracle(configs(), action_batches(), PLAN, BLOCK, ENV_ID0, SEED, FC_MAX)


def both_positions(plan=PLAN):
    """bool [sum(plan)]: the steps of the run that are a pair's first step in one alignment and its second in the other -- from an
    episode's second step to its last but one"""
    out = np.zeros(sum(plan), dtype=bool)
    for ep, t, i in tc.step_plan(plan):
        out[i] = 1 <= t <= plan[ep] - 2
    return out


def pair_firsts(plan=PLAN):
    """the steps i of the run such that (i, i + 1) is a pair in one of the alignments: both in one episode"""
    sp = tc.step_plan(plan)
    return np.array([i for (ep, t, i) in sp if t + 1 < plan[ep]])


def branch_counts(tr=None):
    """{config: {flag: env-steps at both_positions() on which the oracle took it}}"""
    tr = tr or oracle_trajectory()
    both = both_positions()
    return {name: {f: int(tr.flags[f][both][:, k * BLOCK:(k + 1) * BLOCK].sum()) for f in FLAGS} for k, name in enumerate(NAMES)}


def flip_counts(tr=None):
    """{(config, flag): (pairs first-on second-off, pairs first-off second-on)} over every pair of either alignment"""
    tr = tr or oracle_trajectory()
    first = pair_firsts()
    out = {}
    for name, flag in MUST_FLIP:
        k = NAMES.index(name)
        f = tr.flags[flag][:, k * BLOCK:(k + 1) * BLOCK]
        out[(name, flag)] = (int((f[first] & ~f[first + 1]).sum()), int((~f[first] & f[first + 1]).sum()))
    return out


# ---- the calls of the two alignments and of the chains
def alignment_calls(align, plan=PLAN):
    """[(first step of the run, count)]: "even" -- calls of two from every episode's step 0; "odd" -- the episode's step 0 alone, calls of two
    from its step 1, and the odd step out at the episode's end alone"""
    return chain_calls(align, 2, plan)


def chain_calls(align, length, plan=PLAN):
    """calls of `length` steps from every episode's step 0 ("even") or, behind a call of one, from its step 1 ("odd"); the last call of an
    episode is as long as what is left of it"""
    out, base = [], 0
    for steps in plan:
        t = 0
        if align == "odd":
            out.append((base, 1))
            t = 1
        while t < steps:
            c = min(length, steps - t)
            out.append((base + t, c))
            t += c
        base += steps
    return out


def paired_steps(t, count):
    """how many of a call's steps go out as pairs, from slot t of the day: whole pairs up to the call's end or the day's"""
    k = min(count, 96 - t)
    return k - k % 2


# ---- Part 2: the forecourt
FORECOURT = dict(station_list=[20, 25], station_type_list=["fast", "slow"], hydro_prod_rate=100.0, hydro_store_vlt=400.0, init_soc=0.6,
                 fc_max_power=100.0, fcev_permeate=0.1)
FORECOURT_N, FORECOURT_SEED, FORECOURT_PLAN, FORECOURT_ACTION_SEED = 16, 31, (96, 12), 3100


def uniform_batches(n, a, seed):
    rs = np.random.RandomState(seed)
    batch = rs.uniform(-1, 1, size=(PERIOD, n, a)).astype(np.float32)
    batch.setflags(write=False)
    return batch


@functools.lru_cache(maxsize=None)
def forecourt_batches():
    return uniform_batches(FORECOURT_N, sum(FORECOURT["station_list"]) + 2, FORECOURT_ACTION_SEED)


@functools.lru_cache(maxsize=None)
def forecourt_trajectory():
    return tc.run_oracle([("fcev_stuck", FORECOURT)], forecourt_batches(), FORECOURT_PLAN, FORECOURT_N, 0, FORECOURT_SEED,
                         np.full(FORECOURT_N, FORECOURT["fc_max_power"]))


def forecourt_counts(tr=None):
    """env-steps at both_positions(FORECOURT_PLAN) with a line, a non-empty waiting list, two or more arrivals; the longest line and list"""
    tr = tr or forecourt_trajectory()
    tel = tr.tel[both_positions(FORECOURT_PLAN)]
    line, queue, arrive = tel[..., tc.T["HV_LINE"]], tel[..., tc.T["QUEUE_LEN"]], tel[..., tc.T["HV_ARRIVE"]]
    return dict(line=int((line > 0).sum()), queue=int((queue > 0).sum()), arrivals2=int((arrive >= 2).sum()), max_line=int(line.max()),
                max_queue=int(queue.max()))


# ---- Part 3: the XCD-aware order of the level lanes (level_lane: n_envs % 2048 == 0 and the tail workgroups a multiple of 8)
_XCD_TANK = dict(hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2, fc_max_power=100.0)
XCD_HUBS = {  # the hub shapes "tiny" and "c4_hub" of tests/test_gpu_pair_tails.py, every scalar given (the handle and the oracle take the same dict)
    "tiny": dict(_XCD_TANK, station_list=[3, 5], station_type_list=["slow", "fast"], fcev_permeate=0.05, renew_fluctuate=0.3, price_fluctuate=0.3, hydro_loss=0.001),
    "c4_hub": dict(_XCD_TANK, station_list=[20, 25], station_type_list=["fast", "slow"], fcev_permeate=0.02, renew_fluctuate=0.2, price_fluctuate=0.1, hydro_loss=0.0),
}
XCD_SIZES = (2048, 4096)
XCD_SEED, XCD_ACTION_SEED = 31, 4100
# ("run", first, count) -- chub_run_steps; ("step", i) -- one chub_step_device_packed
XCD_PROGRAM = (("run", 0, 1), ("run", 1, 2), ("run", 3, 6), ("step", 9), ("run", 10, 4))
XCD_STEPS = 14


@functools.lru_cache(maxsize=None)
def xcd_batches(name, n):
    return uniform_batches(n, sum(XCD_HUBS[name]["station_list"]) + 2, XCD_ACTION_SEED)


@functools.lru_cache(maxsize=1)
def xcd_trajectory(name, n):
    """(the last one asked for is kept: the tests of one hub and size stand next to each other)"""
    kw = XCD_HUBS[name]
    return tc.run_oracle([(name, kw)], xcd_batches(name, n), (XCD_STEPS,), n, 0, XCD_SEED, np.full(n, kw["fc_max_power"]))


def distinct_in_every_eighth(tr, n, step=2):
    """in each eighth of the env range, the number of envs whose slots after `step` equal another env's of the same eighth"""
    same = []
    for x in range(8):
        sel = slice(x * n // 8, (x + 1) * n // 8)
        rows = np.concatenate([tr.slots[k][step, sel].reshape(n // 8, -1) for k in (0, 1)], axis=1)
        same.append(n // 8 - len(np.unique(np.ascontiguousarray(rows).view(np.uint32), axis=0)))
    return same
