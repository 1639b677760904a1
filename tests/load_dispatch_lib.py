"""The definition of chub_load_dispatch (include/chub.h) in numpy, vectorised over envs (TEST INFRASTRUCTURE).

One station: its piles' car, emergency and power as chub_pile_obs_device reports them, the f32 min_power / max_power of its
record, one target per env.  The target is clamped as catch_load clamps it (CHS.hpp:358-366), the piles are ordered by
emergency descending with ties by slot index (the reference's multimap keyed by -emergency, CHS.hpp:1324-1336), the powers
of the piles with a car are added to ONE f32 running sum along that order (rank_power_add, CHS.hpp:1375-1402: np.cumsum on
f32 is that sequential sum), and a car is on iff the target covers the sum up to and including itself -- with constant
charging iff fewer than roundf(load / constant_power) cars precede it -- or its emergency is 10 (judge_feasibility forces
it on when the row is stepped).
"""
import numpy as np

KW, FRACTION = 0, 1
F32 = np.float32
# constant_power of the two curves (CHS.hpp:621-637 fast, 495-511 slow), as the f32 the reference keeps
CONSTANT_POWER = {0: F32(36.44764034125146), 1: F32(5.254973139368931)}


def target(loads, mn, mx, units=KW):
    """[N] f32 targets -> the clamped kW target catch_load leaves, [N] f32"""
    a = np.asarray(loads, dtype=F32)
    mn, mx = np.asarray(mn, dtype=F32), np.asarray(mx, dtype=F32)
    if units == FRACTION:
        f = (a + F32(1)) / F32(2)
        f = np.minimum(np.maximum(f, F32(0)), F32(1)).astype(F32)
        a = (mn + (f * (mx - mn)).astype(F32)).astype(F32)  # every operation rounded to f32
    elif units != KW:
        raise ValueError("units")
    return np.where(a > mx, mx, np.where(a < mn, mn, a)).astype(F32)  # if load > mx: mx, else if load < mn: mn


def roundf(x):
    """C's roundf (half away from zero) on f32 values"""
    x = np.asarray(x, dtype=np.float64)
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def station_dispatch(car, emergency, power, mn, mx, loads, typ, constant_charging=False, units=KW, details=False):
    """car, emergency, power [N, S] f32; mn, mx, loads [N]; typ 0 fast / 1 slow -> on [N, S] bool.
    details=True: (on, beyond) with beyond [N] = number of must-charge cars the target alone would leave off."""
    car = np.asarray(car, dtype=F32) > 0.5
    em = np.asarray(emergency, dtype=F32)
    pw = np.where(car, np.asarray(power, dtype=F32), F32(0)).astype(F32)
    n, s = car.shape
    load = target(loads, mn, mx, units)
    if s == 0:
        return (np.zeros((n, 0), bool), np.zeros(n, np.int64)) if details else np.zeros((n, 0), bool)
    order = np.argsort(-em, axis=1, kind="stable")  # emergency descending, ties by slot index
    car_o = np.take_along_axis(car, order, axis=1)
    em_o = np.take_along_axis(em, order, axis=1)
    cum = np.cumsum(np.take_along_axis(pw, order, axis=1), axis=1, dtype=F32)  # sequential f32 (an empty pile adds 0: no change)
    if constant_charging:
        n_on = roundf((load / CONSTANT_POWER[typ]).astype(F32))
        before = np.cumsum(car_o, axis=1) - car_o
        by_load = car_o & (before < n_on[:, None])
    else:
        by_load = car_o & (load.astype(np.float64)[:, None] + 0.0001 >= cum.astype(np.float64))
    must = car_o & (em_o == F32(10))
    on = np.zeros((n, s), dtype=bool)
    np.put_along_axis(on, order, by_load | must, axis=1)
    if details:
        return on, (must & ~by_load).sum(axis=1)
    return on


def pack_bits(on):
    """on [N, S] bool -> chub_step_bits' words [N, ceil(S / 64)] u64 (bit b of word w = hub slot 64 w + b)"""
    n, s = on.shape
    w = max((s + 63) // 64, 0)
    padded = np.zeros((n, 64 * w), dtype=np.uint64)
    padded[:, :s] = on
    return (padded.reshape(n, w, 64) << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)


def hub_dispatch(cols, scalars, piles, types, constant_charging, loads, tail, units=KW, details=False):
    """A hub: cols = the (car, emergency, power) columns of pile_obs [N, 3, S]; scalars = station_scalars [N, 2, 8] f64 (columns 0 and 2 are
    the record's f32 min_power and max_power); piles, types per station (types: 0 fast, 1 slow); loads, tail [N, 2] ->
    (rows [N, S + 2] f32, bits [N, W] u64), with details=True also beyond [N, 2]."""
    cols = np.asarray(cols, dtype=F32)
    n = cols.shape[0]
    s0, s = piles[0], piles[0] + piles[1]
    on = np.zeros((n, s), dtype=bool)
    beyond = np.zeros((n, 2), dtype=np.int64)
    loads = np.asarray(loads, dtype=F32).reshape(n, 2)
    for k in range(2):
        if piles[k] == 0:
            continue
        sl = slice(0, s0) if k == 0 else slice(s0, s)
        on[:, sl], beyond[:, k] = station_dispatch(cols[:, 0, sl], cols[:, 1, sl], cols[:, 2, sl], scalars[:, k, 0].astype(F32),
                                                   scalars[:, k, 2].astype(F32), loads[:, k], types[k], constant_charging, units, details=True)
    rows = np.empty((n, s + 2), dtype=F32)
    rows[:, :s] = np.where(on, F32(1), F32(-1))
    rows[:, s:] = np.asarray(tail, dtype=F32).reshape(n, 2)
    return (rows, pack_bits(on), beyond) if details else (rows, pack_bits(on))
