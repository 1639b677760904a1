"""The made grid of tests/class_grid_lib.py is what it claims to be -- conditions on the INPUTS of tests/test_gpu_class_grid.py, checked
with the CPU oracle alone: the grid covers every class with every level of its lists, no stay passes 27 slots, the tie search finds at
least the triples it found when the lists were fixed and the lists hold their levels, the oracle meets every tie from both sides, the
`needed == 0` case occurs, and at least half of all (pile, step) pairs of the first 12 steps are compared."""
import numpy as np
import pytest

import class_grid_lib as cg

MODES = [False, True]
MODE_IDS = ["curves", "constant"]
WITH_TIES = [("fast", False), ("slow", False), ("slow", True)]
NO_TIES = [("fast", True)]  # named, not passed over: a fast station charging at constant power has no whole `needed` anywhere
TIE_IDS = ["%s_%s" % (t, "constant" if cc else "curves") for t, cc in WITH_TIES]


def test_the_grid_covers_every_class_with_every_level():
    assert cg.SHAPE == (64, 64) and cg.N == 2048
    for cc in MODES:
        cars = cg.grid(cc)
        for k, sp in ((0, slice(0, 64)), (1, slice(64, 128))):
            levels = cg.levels_of(k, cc)
            assert len(set(levels.tolist())) == 64 and {0, 1, 499, 500, 998, 999} <= set(levels.tolist()) and levels.min() == 0 and levels.max() == 999
            pairs = np.unique(cars.cls[:, sp].astype(np.int64) * 1000 + cars.level[:, sp])
            assert pairs.size == 2048 * 64  # every (class, level of the list) pair, each exactly once
            assert set(np.unique(cars.level[:, sp]).tolist()) == set(levels.tolist())
            assert cars.late[:, sp].min() == 0 and cars.late[:, sp].max() == 15
        # the arrival SoCs are the classes' own: 1678 distinct values from 25 to 70, both clips many classes wide
        soc = cg.class_soc()
        assert np.unique(soc).size == 1678 and soc.min() == 25.0 and soc.max() == 70.0
        assert (soc == 25.0).sum() == 325 and (soc == 70.0).sum() == 47
        assert np.array_equal(cars.soc, soc[cars.cls])


@pytest.mark.parametrize("policy", cg.POLICIES)
@pytest.mark.parametrize("cc", MODES, ids=MODE_IDS)
def test_stays_fit_and_enough_is_compared(cc, policy):
    ex = cg.expectation(cc, policy)
    assert 1 <= ex.stay.min() and ex.stay.max() <= 27 and ex.steps <= 27
    assert ex.overflow == 0
    # the share of (pile, step) pairs of the first 12 steps that is compared, i.e. whose original car is still there
    share = np.mean([ex.present(t).mean() for t in range(1, 13)])
    assert share >= 0.5, share
    assert not ex.present(ex.steps).any() and ex.present(ex.steps - 1).any()


def test_the_tie_search_finds_what_it_found():
    counts = cg.tie_counts()
    for key, found in cg.FOUND.items():
        assert counts[key] >= found, (key, counts[key], found)
    assert sorted(k for k, c in counts.items() if c == 0) == sorted(NO_TIES)
    assert sorted(k for k, c in counts.items() if c > 0) == sorted(WITH_TIES)


@pytest.mark.parametrize("typ,cc", WITH_TIES, ids=TIE_IDS)
def test_every_tie_is_in_the_level_lists(typ, cc):
    k = cg.TYPE_NAMES.index(typ)
    soc, ts, tt = cg.chains(cg.TYPES[k], cc)
    for t in cg.tie_search(cg.TYPES[k], cc):
        assert t.level in cg.LEVELS[typ, cc], t
        need = tt[t.level] - ts[t.cls, t.n]
        assert need.dtype == np.float32 and need == t.m and t.m >= 1
        for late, stayed in (t.far, t.on):
            assert 0 <= late <= 15 and t.n <= stayed <= t.n + 1


@pytest.mark.parametrize("cc", MODES, ids=MODE_IDS)
def test_the_grid_meets_arrival_ties_from_both_sides(cc):
    """a car whose need is whole on arrival (n = 0) and that has extra stay idles, all off, until it has m + 1 slots left -- the step in
    which `<=` and `<` part -- and charges from the next step on"""
    ex, cars = cg.expectation(cc, "off"), cg.grid(cc)
    met = 0
    for t in cg.tie_search(cg.TYPES[1], cc):
        if t.n:
            continue
        e, j = np.nonzero((cars.cls[:, 64:] == t.cls) & (cars.level[:, 64:] == t.level))
        assert e.size == 1
        e, s = int(e[0]), 64 + int(j[0])
        late = int(cars.late[e, s])
        assert ex.stay[e, s] == t.m + late
        if late == 0:
            continue
        assert not ex.charge[:late, e, s].any(), t          # m + 1 slots left before step `late` (counted from 1): not urgent
        assert ex.charge[late, e, s] == 1 and t.m >= 2, t   # m slots left: urgent (and still there afterwards)
        met += 1
    assert met >= 2, met


@pytest.mark.parametrize("cc", MODES, ids=MODE_IDS)
def test_the_made_ties_are_met_from_both_sides(cc):
    """tie_case(): before the deciding all-off step every tie car has taken exactly its n car_steps (its SoC is entry n of its class's
    chain) and has m + 1 or m slots left; the oracle calls exactly the latter urgent, and after the step exactly those have charged.  A
    car with one slot left leaves in that step (m = 1, urgent): its flag cannot be seen on any side and is not counted."""
    tc = cg.tie_case(cc)
    ex, pre = tc.ex, tc.pre
    seen, before, after = {}, ex.present(pre), ex.present(pre + 1)
    for k, off in ((0, 0), (1, 64)):
        ties = cg.tie_search(cg.TYPES[k], cc)
        soc = cg.chains(cg.TYPES[k], cc)[0]
        sl = tc.slots[(tc.slots[:, 1] >= off) & (tc.slots[:, 1] < off + 64)]
        assert (len(sl) > 0) == (len(ties) > 0)
        for e, s, i, urgent in sl:
            t = ties[i]
            assert before[e, s] and tc.rows[e, s, 4] == t.n and tc.rows[e, s, 3] == pre
            assert ex.dyn[pre - 1, 2, e, s] == soc[t.cls, t.n]
            assert ex.stay[e, s] - pre == t.m + (0 if urgent else 1)
            assert (ex.dyn[pre - 1, 0, e, s] == 10) == bool(urgent)   # calculate_needed's verdict at the end of the last step before
            if after[e, s]:
                assert ex.charge[pre, e, s] == urgent, (t, urgent)
                seen[(k, i, bool(urgent))] = True
            else:
                assert urgent and t.m == 1, t
        for i, t in enumerate(ties):
            assert (k, i, False) in seen and ((k, i, True) in seen or t.m == 1), t
    assert ex.overflow == 0


@pytest.mark.parametrize("cc", MODES, ids=MODE_IDS)
def test_needed_zero_occurs_under_all_on(cc):
    """a chain that has reached its target exactly (both 100 at level 999): `needed > 0` is false with needed == 0, the urgency is 0"""
    ex = cg.expectation(cc, "on")
    hits = 0
    for t in range(1, ex.steps + 1):
        here = ex.present(t)
        hits += int((here & (ex.dyn[t - 1, 0] == 0) & (ex.dyn[t - 1, 2] == ex.cars.target)).sum())
    assert hits >= 100, hits
