"""The definition of chub_station_profile_device (include/chub.h) in numpy, from the nine per-pile columns chub_get_slots /
chub_pile_obs_device report.  It is the oracle of tests/test_gpu_station_profile.py and knows nothing of the kernel: a pile with a car and
`left = stay_time - already_stay_time` slots to go falls into bucket min(left, B) - 1 of its station; counts are exact, the four sums are
sums of rint(float64(x) * 2^q) in int64, written as float32(sum) * float32(2^-q)."""
import numpy as np

SP_NAMES = ("cars", "charging", "must_charge", "power", "power_charging", "emergency", "soc_gap")
SP_Q = {"power": 19, "power_charging": 19, "emergency": 20, "soc_gap": 16}  # a sum's quantum is 2^-q
CAR, CHARGE, EMERGENCY, POWER, SOC, INIT_SOC, TARGET_SOC, STAY_TIME, ALREADY_STAY = range(9)


def names_of(fields):
    """None, a bit mask or names -> the names in the order the columns come out"""
    if fields is None:
        return SP_NAMES
    if hasattr(fields, "__index__"):
        return tuple(n for i, n in enumerate(SP_NAMES) if int(fields) >> i & 1)
    if isinstance(fields, str):
        fields = (fields,)
    assert all(f in SP_NAMES for f in fields), fields
    return tuple(n for n in SP_NAMES if n in fields)


def fixed(x, q):
    """llrint((double) x * 2^q): round-half-even on the exact product"""
    return np.rint(np.asarray(x, dtype=np.float32).astype(np.float64) * 2.0 ** q).astype(np.int64)


def profile_from_columns(cols9, piles, fields, buckets):
    """cols9 [N][9][S] in hub-slot order (station 0's piles first) -> float32 [N, 2, C, B]"""
    cols9 = np.asarray(cols9, dtype=np.float32)
    N, nine, S = cols9.shape
    assert nine == 9 and S == piles[0] + piles[1] and 1 <= buckets <= 32
    names, B = names_of(fields), int(buckets)
    out = np.zeros((N, 2, len(names), B), dtype=np.float32)
    for k, (lo, hi) in enumerate(((0, piles[0]), (piles[0], S))):
        c = cols9[:, :, lo:hi]
        car = c[:, CAR] == 1
        left = (c[:, STAY_TIME] - c[:, ALREADY_STAY]).astype(np.int64)
        bucket = np.minimum(left, B) - 1
        chg = car & (c[:, CHARGE] == 1)
        for j, name in enumerate(names):
            if name == "cars":
                term = car.astype(np.int64)
            elif name == "charging":
                term = chg.astype(np.int64)
            elif name == "must_charge":
                term = (car & (c[:, EMERGENCY] == 10)).astype(np.int64)
            elif name == "power":
                term = np.where(car, fixed(c[:, POWER], 19), 0)
            elif name == "power_charging":
                term = np.where(chg, fixed(c[:, POWER], 19), 0)
            elif name == "emergency":
                term = np.where(car, fixed(c[:, EMERGENCY], 20), 0)
            else:
                term = np.where(car, fixed(c[:, TARGET_SOC] - c[:, SOC], 16), 0)  # (the difference is taken in float32)
            for b in range(B):
                total = np.where(car & (bucket == b), term, 0).sum(axis=1, dtype=np.int64)
                out[:, k, j, b] = total.astype(np.float32) * np.float32(2.0 ** -SP_Q.get(name, 0))
    return out
