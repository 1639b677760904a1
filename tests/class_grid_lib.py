"""A made grid of cars for the PHILOX class tables, and what the CPU oracle makes of it -- numpy and the oracle, no device.

PHILOX evaluates no curve in the step: a pile's power, SoC and urgency are read from the per-class rows Tables::cls[k] (built on the host
by build_class_row), the per-class SoC rows (k_build_cls_soc) and ttab2[k][level].  Free-running trajectories meet a few thousand of the
2048 x 28 x 1000 (class, car_steps, level) triples; here every class meets 64 levels per station type, both ends of the level range
included, and the triples on which must_charge sits on its boundary (CHS.hpp:879-898: `time_left <= ceilf(needed)` with a WHOLE needed) are
found by search and made.

The grid: for a hub (S0 fast, S1 slow) and n envs the car in env e, hub slot j of station k has
    class (e + 7 j) % 2048, level LEVELS[type, mode][j % 64], extra stay (e // 3 + j) % 16
arrival SoC orc_soc_level_value(class), target orc_uniform_level(level, 80, 100).  With n = 2048 and a station of 64 piles every (class,
level of the list) pair occurs exactly once per station.

The expectation: the oracle's stations filled with these cars (orc_vec_fill_station: reset_position + place_car, what
orc_station_put_car does) and stepped (orc_vec_step_stations: orc_station_step) under a policy until every original car has left.  The
oracle admits cars of its own into piles that empty: such piles are masked (step >= stay_time of the original car), never compared;
station units are independent, so nothing else is affected.

tests/test_class_grid_cpu.py asserts on the oracle alone that the grid and the ties are what is claimed here; tests/test_gpu_class_grid.py
holds the device to expectation() / tie_case() in every launch form."""
import collections
import ctypes as C
import functools
import sys

import numpy as np

import orclib
from orclib import orc, ptr

N = 2048                 # envs
CLASSES = 2048           # ORC_SOC_LEVELS
ROW = 28                 # car_steps searched: stays are at most 12 + 15 = 27
SHAPE = (64, 64)         # fast, slow
TYPES = (orclib.FAST, orclib.SLOW)
TYPE_NAMES = ("fast", "slow")
HUB = dict(station_type_list=["fast", "slow"], hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2, fc_max_power=100.0,
           fcev_permeate=0.0, renew_fluctuate=0.0, price_fluctuate=0.0, hydro_loss=0.0)
POLICIES = ("off", "on", "random")
POLICY_SEED = 20261
THREADS = 8
EMPTY = np.array([0, 0, 0, 0, 0, 0, 0, -1, -1], dtype=np.float32)  # the pile defaults of the reference (reset_position, CHS.hpp:276-286)
FOUND = {("fast", False): 1, ("fast", True): 0, ("slow", False): 8, ("slow", True): 23}  # ties found when this file was written

# 64 distinct levels per (station type, constant_charging): 0, 1, 499, 500, 998, 999, every level tie_search() finds for that type and
# mode, the rest evenly spaced
LEVELS = {
    ("fast", False): [0, 1, 17, 34, 52, 69, 86, 103, 121, 138, 155, 172, 189, 207, 224, 241, 258, 276, 293, 310, 327, 344, 362, 379, 396, 413,
                      431, 448, 465, 482, 499, 500, 501, 517, 534, 551, 568, 586, 603, 620, 637, 655, 672, 689, 706, 723, 741, 758, 775, 792,
                      810, 827, 844, 861, 878, 896, 913, 930, 947, 965, 978, 982, 998, 999],
    ("fast", True): [0, 1, 17, 34, 51, 68, 85, 102, 119, 135, 152, 169, 186, 203, 220, 237, 254, 271, 288, 305, 322, 339, 356, 373, 389, 406,
                     423, 440, 457, 474, 491, 499, 500, 508, 525, 542, 559, 576, 593, 610, 626, 643, 660, 677, 694, 711, 728, 745, 762, 779,
                     796, 813, 830, 847, 864, 880, 897, 914, 931, 948, 965, 982, 998, 999],
    ("slow", False): [0, 1, 20, 39, 44, 47, 59, 78, 98, 118, 137, 157, 176, 196, 215, 235, 255, 274, 294, 313, 333, 353, 372, 392, 411, 431,
                      435, 451, 470, 490, 499, 500, 509, 519, 529, 548, 568, 569, 588, 607, 627, 646, 666, 686, 705, 725, 744, 764, 765, 784,
                      803, 823, 842, 862, 881, 893, 901, 919, 921, 940, 960, 979, 998, 999],
    ("slow", True): [0, 1, 18, 22, 36, 54, 73, 91, 109, 127, 145, 163, 182, 200, 210, 218, 236, 254, 272, 291, 309, 327, 345, 363, 381, 400,
                     418, 436, 454, 472, 490, 499, 500, 509, 527, 545, 563, 581, 599, 618, 624, 636, 654, 672, 690, 708, 727, 745, 763, 781,
                     799, 817, 828, 836, 854, 872, 890, 908, 926, 945, 963, 981, 998, 999],
}


def levels_of(k, cc):
    return np.array(LEVELS[TYPE_NAMES[k], bool(cc)], dtype=np.int32)


# ------------------------------------------------------------------------------------------------ the chains and the ties
@functools.lru_cache(maxsize=None)
def class_soc():
    """[2048] f32: the arrival SoC of every class"""
    out = np.array([orc.orc_soc_level_value(orclib.tables(), c) for c in range(CLASSES)], dtype=np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def chains(typ, cc):
    """(soc [2048, ROW], ts [2048, ROW], tt [1000]) f32 on the oracle's curves: a class's SoC and soc_to_time(SoC) after n car_steps -- the
    chain soc -> soc_to_time -> + 1 -> time_to_soc of car_step (CHS.hpp:900-905) -- and soc_to_time(target of level l)"""
    curve = orc.orc_curve_fast if typ == orclib.FAST else orc.orc_curve_slow
    soc, ts = np.zeros((CLASSES, ROW), dtype=np.float32), np.zeros((CLASSES, ROW), dtype=np.float32)
    for c in range(CLASSES):
        s = float(class_soc()[c])
        for n in range(ROW):
            t = np.float32(curve(2, s, int(cc)))
            soc[c, n], ts[c, n] = s, t
            s = curve(1, float(t + np.float32(1)), int(cc))
    tt = np.array([curve(2, orc.orc_uniform_level(l, 80.0, 100.0), int(cc)) for l in range(1000)], dtype=np.float32)
    for a in (soc, ts, tt):
        a.setflags(write=False)
    return soc, ts, tt


# a triple on the boundary: after n car_steps a car of class `cls` and level `level` needs exactly m slots.  `far` / `on`: (extra stay,
# steps stayed) of a car that has taken its n car_steps and has m + 1 slots left (not urgent) / m slots left (urgent)
Tie = collections.namedtuple("Tie", "cls n level m far on")


@functools.lru_cache(maxsize=None)
def tie_search(typ, cc):
    """every (class, n, level) of 2048 x ROW x 1000 with needed = tt[level] - ts[class, n] > 0 and needed == ceilf(needed) in f32"""
    soc, ts, tt = chains(typ, cc)
    need = tt[None, None, :] - ts[:, :, None]  # f32
    out = []
    for c, n, l in zip(*np.nonzero((need > 0) & (need == np.ceil(need)))):
        c, n, l = int(c), int(n), int(l)
        m = int(need[c, n, l])
        c0 = int(np.ceil(tt[l] - ts[c, 0]))  # the stay without the extra one (place_car)
        # stay_time = c0 + late and the car has charged in every step since it came: time_left = c0 + late - n
        late_far = m + 1 + n - c0
        assert 0 <= late_far <= 15, (c, n, l, m, c0)
        # one slot less to go: one slot less of extra stay -- or, where there is none to take away (the chain's rounding has made a car that
        # arrived urgent non-urgent after n forced steps), one more step stayed: the step it idles in on the far side of the boundary
        on = (late_far - 1, n) if late_far >= 1 else (0, n + 1)
        out.append(Tie(c, n, l, m, (late_far, n), on))
    return tuple(out)


def tie_counts():
    return {(TYPE_NAMES[k], cc): len(tie_search(TYPES[k], cc)) for k in (0, 1) for cc in (False, True)}


# ------------------------------------------------------------------------------------------------ the grid
Cars = collections.namedtuple("Cars", "cls level late soc target")  # each [n, S0 + S1], hub order


def cars_of(cls, level, late):
    soc = class_soc()[cls]
    target = np.array([orc.orc_uniform_level(l, 80.0, 100.0) for l in range(1000)], dtype=np.float32)[level]
    return Cars(cls.astype(np.int32), level.astype(np.int32), late.astype(np.int32), soc, target)


def grid(cc, shape=SHAPE, n=N):
    e = np.arange(n)[:, None]
    cols = []
    for k in (0, 1):
        j = np.arange(shape[k])[None, :]
        cols.append(((e + 7 * j) % CLASSES, np.broadcast_to(levels_of(k, cc)[j % 64], (n, shape[k])), (e // 3 + j) % 16))
    return cars_of(*[np.concatenate([c[f] for c in cols], axis=1) for f in range(3)])


# ------------------------------------------------------------------------------------------------ the oracle run
class Expectation(object):
    """what the oracle makes of a population of cars under per-(step, env, slot) action bits.  Kept whole but compact: of a pile that still
    holds its original car the fields car, init_soc, target_soc, stay_time and already_stay_time are 1, the car's own and the step count
    (asserted while the oracle runs); charge, emergency, power and soc are kept per step."""

    def __init__(self, shape, cars, stay, power0, bits, steps=None):
        self.shape, self.cars, self.stay, self.power0, self.bits, self.overflow = shape, cars, stay, power0, bits, 0
        self.n, self.S = stay.shape
        self.steps = int(stay.max()) if steps is None else steps  # (by default: until every original car has left)
        self.charge = np.zeros((self.steps, self.n, self.S), dtype=np.uint8)
        self.dyn = np.zeros((self.steps, 3, self.n, self.S), dtype=np.float32)  # emergency, power, soc

    def span(self, k):
        return slice(0, self.shape[0]) if k == 0 else slice(self.shape[0], self.S)

    def present(self, t):
        """[n, S] bool: after t steps (0: as filled) the pile still holds its original car"""
        return t < self.stay

    def fields(self, t, k):
        """station k after t >= 1 steps: ([n, 9, S_k] f32 as chub_get_slots lays them out -- a pile whose car has left shows the empty
        defaults, whatever the oracle has admitted there since -- and the mask [n, S_k] of piles still holding their original car)"""
        sp, mask = self.span(k), self.present(t)[:, self.span(k)]
        out = np.empty((self.n, 9, sp.stop - sp.start), dtype=np.float32)
        out[:, 0], out[:, 1] = 1, self.charge[t - 1][:, sp]
        out[:, 2:5] = self.dyn[t - 1][:, :, sp].transpose(1, 0, 2)
        out[:, 5], out[:, 6], out[:, 7], out[:, 8] = self.cars.soc[:, sp], self.cars.target[:, sp], self.stay[:, sp], t
        return np.where(mask[:, None, :], out, EMPTY[None, :, None]), mask

    def filled(self, k):
        """station k as filled, fields 0, 3, 5, 6, 7, 8 (emergency and the situation's soc are calculate_output's, which the oracle's next
        step runs first): [n, 6, S_k] f32"""
        sp = self.span(k)
        out = np.empty((self.n, 6, sp.stop - sp.start), dtype=np.float32)
        out[:, 0], out[:, 1], out[:, 2], out[:, 3] = 1, self.power0[:, sp], self.cars.soc[:, sp], self.cars.target[:, sp]
        out[:, 4], out[:, 5] = self.stay[:, sp], 0
        return out

    def station_sums(self, t):
        """[n, 2, 4] f64: min_power, charge_power, max_power, car_number of the original cars after t steps, by the rule of the production
        sums (calculate_output's exact_sums): every car's power to the nearest 2^-19 kW, added as integers, narrowed once to f32"""
        out = np.zeros((self.n, 2, 4))
        for k in (0, 1):
            f, mask = self.fields(t, k)
            q = np.rint(f[:, 3] * np.float32(524288.0)).astype(np.int64) * mask
            sums = [(q * (f[:, 2] > 8)).sum(axis=1), (q * ((f[:, 1] <= 1.1) & (f[:, 1] >= 0.9))).sum(axis=1), q.sum(axis=1)]
            for c, s in enumerate(sums):
                out[:, k, c] = s.astype(np.float32) * np.float32(1.0 / 524288.0)
            out[:, k, 3] = mask.sum(axis=1)
        return out

    def freeze(self):
        for a in (self.stay, self.power0, self.bits, self.charge, self.dyn) + tuple(self.cars):
            a.setflags(write=False)
        return self


def run_oracle(cc, shape, cars, bits, steps=None):
    """cars into the oracle's stations, then `steps` steps (default: until every original car has left) under bits [steps, n, S] u8"""
    n, S = cars.cls.shape
    cfg = orclib.make_config(piles=shape, types=("fast", "slow"), constant_charging=cc,
                             **{f: v for f, v in HUB.items() if f != "station_type_list"})
    h = orc.orc_vec_create(C.byref(cfg), orclib.tables(), n, 0, orclib.PHILOX, 1)
    assert h
    try:
        got, off = [np.zeros((n, 9, shape[k]), dtype=np.float32) for k in (0, 1)], (0, shape[0])
        for k in (0, 1):
            sp = slice(off[k], off[k] + shape[k])
            orc.orc_vec_fill_station(h, k, ptr(np.ascontiguousarray(cars.soc[:, sp])), ptr(np.ascontiguousarray(cars.target[:, sp])),
                                     ptr(np.ascontiguousarray(cars.late[:, sp], dtype=np.int32)))
            orc.orc_vec_slots(h, k, ptr(got[k]))
        whole = lambda f: np.concatenate([got[0][:, f], got[1][:, f]], axis=1)
        stay = whole(7).astype(np.int32)
        assert (whole(0) == 1).all() and np.array_equal(whole(5), cars.soc) and np.array_equal(whole(6), cars.target) and (whole(8) == 0).all()
        ex = Expectation(shape, cars, stay, whole(3).copy(), bits, steps)
        assert bits.shape[0] >= ex.steps and bits.shape[1:] == (n, S)
        for t in range(1, ex.steps + 1):
            orc.orc_vec_step_stations(h, ptr(np.ascontiguousarray(bits[t - 1], dtype=np.float32)), THREADS)
            for k in (0, 1):
                orc.orc_vec_slots(h, k, ptr(got[k]))
            here = ex.present(t)
            # the five fields that are not kept per step are what Expectation.fields() says they are
            assert (whole(0)[here] == 1).all() and (whole(8)[here] == t).all() and np.array_equal(whole(7)[here], stay[here])
            assert np.array_equal(whole(5)[here], cars.soc[here]) and np.array_equal(whole(6)[here], cars.target[here])
            ex.charge[t - 1] = whole(1)
            for c, f in enumerate((2, 3, 4)):
                ex.dyn[t - 1, c] = whole(f)
        ex.overflow = int(orc.orc_vec_overflow(h))
    finally:
        orc.orc_vec_destroy(h)
    return ex.freeze()


def policy_bits(policy, steps, n, S):
    """[steps, n, S] u8: all off (urgency alone decides), all on, or one fixed-seed random bit per (step, env, slot)"""
    if policy == "random":
        return np.random.RandomState(POLICY_SEED).randint(0, 2, size=(steps, n, S)).astype(np.uint8)
    return np.full((steps, n, S), 1 if policy == "on" else 0, dtype=np.uint8)


def action_rows(bits_t):
    """[n, S] bits -> [n, S + 2] f32 action rows (+1 on, -1 off; both tail actions 0)"""
    a = np.zeros((bits_t.shape[0], bits_t.shape[1] + 2), dtype=np.float32)
    a[:, :-2] = np.where(bits_t > 0, np.float32(1), np.float32(-1))
    return a


@functools.lru_cache(maxsize=3)
def expectation(cc, policy, shape=SHAPE, n=N):
    """one oracle run per key, shared by every launch form (three at a time are kept: the tests come policy by policy, mode by mode)"""
    cars, bits = grid(cc, shape, n), policy_bits(policy, ROW, n, sum(shape))
    if max(shape) > 256:  # (stations of more than 256 piles: the oracle compiled with room for them)
        with orclib.big_oracle(sys.modules[__name__]):
            return run_oracle(cc, shape, cars, bits)
    return run_oracle(cc, shape, cars, bits)


# ------------------------------------------------------------------------------------------------ the ties, made
TieCase = collections.namedtuple("TieCase", "pre ex slots rows")


@functools.lru_cache(maxsize=2)
def tie_case(cc, shape=SHAPE, n=N):
    """Every tie of both station types on both sides of the boundary, in every fourth pile; grid cars in the others.  A tie car comes
    `pre` steps before the step that decides, idles first (its extra stay is made long enough for that), then charges n steps, so that all
    cars meet the deciding all-off step together; a car without extra stay to spare charges its n steps first (it arrives urgent) and idles
    last.  Returns pre, the oracle run (pre + 1 steps), slots [(env, hub slot, tie, urgent)], and `rows` [n, S, 6] i32 for chub_set_slots:
    the oracle's piles after the pre steps (class, level, stay, stayed, car_steps = the steps it charged in, charging flag; -1 where the
    original car has left)."""
    base = grid(cc, shape, n)
    cls, level, late = base.cls.copy(), base.level.copy(), base.late.copy()
    pre = 1 + max([t.n for k in (0, 1) for t in tie_search(TYPES[k], cc)] + [0])
    bits = np.zeros((pre + 1, n, sum(shape)), dtype=np.uint8)
    slots = []
    for k, off in ((0, 0), (1, shape[0])):
        ties = tie_search(TYPES[k], cc)
        sides = [(t, urgent) for t in ties for urgent in (False, True)]
        for e in range(n if sides else 0):
            for j in range(0, shape[k], 4):
                t, urgent = sides[(e + j // 4) % len(sides)]
                extra, stayed = t.on if urgent else t.far
                idle_first = pre - stayed
                s = off + j
                cls[e, s], level[e, s], late[e, s] = t.cls, t.level, extra + idle_first
                assert late[e, s] <= 15 and (idle_first == 0 or late[e, s] >= 1)
                bits[idle_first:idle_first + t.n, e, s] = 1
                slots.append((e, s, ties.index(t), urgent))
    ex = run_oracle(cc, shape, cars_of(cls, level, late), bits, steps=pre + 1)
    present = ex.present(pre)
    rows = np.full((n, sum(shape), 6), -1, dtype=np.int32)
    rows[..., 0], rows[..., 1], rows[..., 2], rows[..., 3] = cls, level, ex.stay, pre
    rows[..., 4], rows[..., 5] = ex.charge[:pre].sum(axis=0), ex.charge[pre - 1]
    rows[~present] = -1
    rows.setflags(write=False)
    return TieCase(pre, ex, np.array(slots, dtype=np.int64).reshape(-1, 4), rows)
