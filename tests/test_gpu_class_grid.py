"""The PHILOX class tables and the urgency decision, held to the CPU oracle on a made grid (tests/class_grid_lib.py; its claims about the
grid are asserted on the oracle alone in tests/test_class_grid_cpu.py).

PHILOX evaluates no curve in the step: Tables::cls[k] (build_class_row), the per-class SoC rows (k_build_cls_soc) and ttab2[k][level] are
all a pile's power, SoC and urgency come from.  Free runs and the fixtures' tapes meet those tables where trajectories happen to land.  Here
a hub of 64 fast + 64 slow piles x 2048 envs holds every one of the 2048 classes with 64 levels per station type (both ends of the level
range, every level on which must_charge can sit on its boundary), extra stays 0 .. 15, and is stepped until the last car has left:

  a. through tape mode -- the classes registered with chub_tape_register_soc (rows rebuilt by build_class_row from the SoCs), every pile
     admitted by chub_reset_tape (the device's own ceil for stay_time on every (class, level)), nobody arriving afterwards: all nine
     fields of every pile and the station sums after every step, in both launch forms of tape mode;
  b. free-running on the handle's OWN tables -- chub_set_slots with the grid's cars after an ordinary reset, ordinary steps: the piles that
     still hold their original car, all nine fields after every step (the device admits its own arrivals into emptied piles, as the oracle
     does: those are masked on both sides), in every slot kernel: packed small tile, large tile, wave-local, one launch, spans of
     chub_run_steps; and on (65, 200) and (65, 300) hubs for the kernels of stations of more than 64 and of more than 256 piles;
  c. the ties themselves: every (class, car_steps, level) whose need is a whole number of slots, placed with m + 1 and with m slots left
     through chub_set_slots, one all-off step: who charges is exactly who had m left.

Every comparison is bit for bit; there is no tolerance in this file."""
import ctypes as C

import numpy as np
import pytest

import class_grid_lib as cg

pytestmark = pytest.mark.gpu

SEED = 0xC1A55
MODES = [False, True]
PACKED, BIG_TILE, ONE_LAUNCH, SPAN_SIZE_OK, STATION0, STATION1 = 0, 1, 6, 7, 14, 15  # CHUB_PLAN_* (include/chub.h)
mode_id = lambda cc: "constant" if cc else "curves"


def hub():
    import charginghub_env_amd as chub
    return chub


def hub_kwargs(shape, cc):
    return dict(cg.HUB, station_list=list(shape), constant_charging=cc)


def plan_of(shape, n, cc, **options):
    chub = hub()
    from charginghub_env_amd import _lib
    kw = hub_kwargs(shape, cc)
    cfg = chub.make_config(kw["station_list"], kw["station_type_list"], **{f: v for f, v in kw.items() if f not in ("station_list", "station_type_list")})
    opt = _lib.ChubOptions()
    for f, v in options.items():
        setattr(opt, f, v)
    out = (C.c_int32 * 16)()
    assert chub.load_library().chub_launch_plan(C.byref(cfg), n, _lib.RNG_PHILOX, C.byref(opt), out) == 0
    return list(out)


# the launch forms: constructor options, the same as chub_options values, and what chub_launch_plan must say of them
FORMS = {
    "packed_small": (dict(fused_step="off", tile="small"), dict(fused_step=1, tile=1), {PACKED: 1, BIG_TILE: 0, ONE_LAUNCH: 0}),
    "large_tile": (dict(tile="large"), dict(tile=2), {PACKED: 3, BIG_TILE: 1, ONE_LAUNCH: 0}),
    "wave": (dict(slot_kernel="wave"), dict(slot_kernel=1), {PACKED: 0, ONE_LAUNCH: 0, STATION0: 0, STATION1: 0}),  # (0: k_slot)
    "one_launch": (dict(fused_step="on"), dict(fused_step=2), {PACKED: 1, BIG_TILE: 0, ONE_LAUNCH: 2}),
    "span": (dict(fused_step="on"), dict(fused_step=2), {PACKED: 1, ONE_LAUNCH: 2, SPAN_SIZE_OK: 1}),
    # stations of more than 64 piles: the packed kernel's form for them, and the wave-local unit kernel (1: k_slot_unit)
    "unit_default": (dict(), dict(), {PACKED: 2, ONE_LAUNCH: 0}),
    "unit_wave": (dict(slot_kernel="wave"), dict(slot_kernel=1), {PACKED: 0, ONE_LAUNCH: 0, STATION0: 1, STATION1: 1}),
    # ... and a station of more than 256 piles, which the wave-local form walks in chunks (2: k_slot_unit_any)
    "chunked_wave": (dict(slot_kernel="wave"), dict(slot_kernel=1), {PACKED: 0, ONE_LAUNCH: 0, STATION0: 1, STATION1: 2}),
}


def make(form, shape, n, cc):
    """a PHILOX handle in the form that was meant: a threshold that moved must not turn two forms into one"""
    kwargs, options, want = FORMS[form]
    plan = plan_of(shape, n, cc, **options)
    assert all(plan[i] == x for i, x in want.items()), (form, plan, want)
    v = hub().VecChargingHub(n, seed=SEED, rng="philox", **hub_kwargs(shape, cc), **kwargs)
    assert v.uses_packed_kernel == (want[PACKED] != 0) and v.uses_fused_step == (want[ONE_LAUNCH] != 0), form
    return v


def same_bits(got, want, mask, ex, off, what):
    """got, want [n, F, S_k] f32; mask [n, S_k] or None (every pile).  Names the first pile that differs and the car it held."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if mask is not None:
        bad &= mask[:, None, :]
    if bad.any():
        e, f, s = [int(x) for x in np.argwhere(bad)[0]]
        c = ex.cars
        raise AssertionError("%s: %d values differ; first at env %d, field %d, pile %d (class %d, level %d, extra stay %d, stay %d): got %r, want %r; "
                             "the pile: got %s, want %s" % (what, int(bad.sum()), e, f, s, c.cls[e, off + s], c.level[e, off + s], c.late[e, off + s],
                                                            ex.stay[e, off + s], got[e, f, s], want[e, f, s], got[e, :, s], want[e, :, s]))


def compare_step(v, ex, t, what, masked):
    """all nine fields after t steps: of the piles still holding their original car (masked), or of every pile -- departed ones must then
    show the empty defaults"""
    sl = v.slots()
    for k, off in ((0, 0), (1, ex.shape[0])):
        want, mask = ex.fields(t, k)
        same_bits(sl[k], want, mask if masked else None, ex, off, "%s, step %d, station %d" % (what, t, k))


# ---------------------------------------------------------------------------------------------- a. admission and the chain, tape mode
TAPE_CASES = [(cc, policy, fused) for cc in MODES for policy in cg.POLICIES for fused in ("off", "on")]


@pytest.mark.parametrize("cc,policy,fused", TAPE_CASES, ids=["%s-%s-fused_%s" % (mode_id(c), p, f) for c, p, f in TAPE_CASES])
def test_tape_admits_the_grid_and_follows_the_oracle(cc, policy, fused):
    ex = cg.expectation(cc, policy)
    n, (S0, S1) = ex.n, ex.shape
    v = make("one_launch" if fused == "on" else "packed_small", ex.shape, n, cc)
    ids = v.tape_register_soc(cg.class_soc())  # (the ids the call returns: equal SoCs may share a row)
    assert ids.shape == (cg.CLASSES,)
    car = np.stack([ids[ex.cars.cls], (ex.cars.level | (ex.cars.late << 16)).astype(np.uint32)], axis=2).astype(np.uint32)
    occ = np.stack([np.full(n, s | (s << 16), dtype=np.uint32) for s in (S0, S1)])
    v.reset_tape(occ, car)
    sl = v.slots()
    for k, off in ((0, 0), (1, S0)):
        # stay_time is the device's own ceil on every (class, level), the arrival ties included
        same_bits(sl[k][:, [0, 3, 5, 6, 7, 8]], ex.filled(k), None, ex, off, "after the tape reset, station %d (fields 0, 3, 5, 6, 7, 8)" % k)
    nobody_pk, nobody = np.zeros((2, n), dtype=np.uint64), np.zeros((n, S0 + S1, 2), dtype=np.uint32)
    for t in range(1, ex.steps + 1):
        v.step_tape(cg.action_rows(ex.bits[t - 1]), nobody_pk, nobody)
        compare_step(v, ex, t, "tape", masked=False)
        sc, want = v.station_scalars(), ex.station_sums(t)
        bad = np.argwhere(sc[:, :, :4] != want)
        assert bad.size == 0, ("station sums (min, charge, max power, car_number)", t, bad[0], sc[bad[0][0], bad[0][1]], want[bad[0][0], bad[0][1]])
        assert not sc[:, :, 4:6].any(), ("nobody queues, nobody arrives", t)
    assert not v.slots()[0][:, 0].any() and not v.slots()[1][:, 0].any()  # the hub is empty
    v.close()


# ---------------------------------------------------------------------------------------------- b. the handle's own tables, free-running
def grid_rows(ex):
    rows = np.zeros((ex.n, ex.S, 6), dtype=np.int32)
    rows[..., 0], rows[..., 1], rows[..., 2] = ex.cars.cls, ex.cars.level, ex.stay  # (the oracle's stay; the device's own ceil is held in a.)
    return rows


def place_grid(v, ex, rows):
    v.reset()
    v.set_slots(rows)
    v.set_station_queue(np.zeros((ex.n, 2), dtype=np.int32))


def run_steps_to(v, ex, bufs, first, last):
    """steps first .. last (counted from 1) through chub_run_steps: step i takes action batch i % 8"""
    from charginghub_env_amd._lib import check
    acts, packed, obs0 = bufs
    assert last - first + 1 <= len(acts)
    for i in range(first, last + 1):
        acts[i % len(acts)].from_host(cg.action_rows(ex.bits[i - 1]))
    c_acts = (C.c_void_p * len(acts))(*[a.ptr for a in acts])
    c_packed = (C.c_void_p * 2)(packed[0].ptr, packed[1].ptr)
    check(v._lib.chub_run_steps(v._h, None, c_acts, len(acts), c_packed, None, obs0.ptr, first, last - first + 1, None))
    v.sync()


def free_run(form, ex, cc):
    v = make(form, ex.shape, ex.n, cc)
    place_grid(v, ex, grid_rows(ex))
    sl = v.slots()
    for k, off in ((0, 0), (1, ex.shape[0])):
        # init_soc: class <-> SoC of the handle's own table; power: entry 0 of the class's row
        same_bits(sl[k][:, [0, 3, 5, 6, 7, 8]], ex.filled(k), None, ex, off, "%s: as placed, station %d (fields 0, 3, 5, 6, 7, 8)" % (form, k))
    if form == "span":
        from charginghub_env_amd import multi_gpu as mg
        bufs = ([mg.DeviceBuffer(ex.n * v.act_dim * 4) for _ in range(8)], [mg.DeviceBuffer(ex.n * (v.obs_dim + 2) * 4) for _ in range(2)],
                mg.DeviceBuffer(ex.n * v.obs_dim * 4))
        ends = [3, 8, 14, 21, ex.steps - 1]  # (after ex.steps steps nothing is left to compare)
        assert ends == sorted(set(ends)) and all(b - a <= 8 for a, b in zip([0] + ends, ends))
        for a, b in zip([0] + ends, ends):
            run_steps_to(v, ex, bufs, a + 1, b)
            compare_step(v, ex, b, form, masked=True)
    else:
        for t in range(1, ex.steps):
            v.step(cg.action_rows(ex.bits[t - 1]))
            compare_step(v, ex, t, form, masked=True)
    v.close()


FREE_CASES = [(cc, policy, form) for cc in MODES for policy in cg.POLICIES for form in ("packed_small", "large_tile", "wave", "one_launch", "span")]


@pytest.mark.parametrize("cc,policy,form", FREE_CASES, ids=["%s-%s-%s" % (mode_id(c), p, f) for c, p, f in FREE_CASES])
def test_own_tables_follow_the_oracle_in_every_slot_kernel(cc, policy, form):
    free_run(form, cg.expectation(cc, policy), cc)


UNIT_SHAPE, UNIT_N = (65, 200), 512
UNIT_CASES = [(cc, form) for cc in MODES for form in ("unit_default", "unit_wave")]


@pytest.mark.parametrize("cc,form", UNIT_CASES, ids=["%s-%s" % (mode_id(c), f) for c, f in UNIT_CASES])
def test_own_tables_follow_the_oracle_in_the_unit_kernels(cc, form):
    """stations of 65 and 200 piles (a unit is more than a wave; 200 is no multiple of 64), 512 envs, the random policy"""
    free_run(form, cg.expectation(cc, "random", UNIT_SHAPE, UNIT_N), cc)


BIG_SHAPE, BIG_N = (65, 300), 128
BIG_CASES = [(cc, form) for cc in MODES for form in ("unit_default", "chunked_wave")]


@pytest.mark.parametrize("cc,form", BIG_CASES, ids=["%s-%s" % (mode_id(c), f) for c, f in BIG_CASES])
def test_own_tables_follow_the_oracle_in_a_station_of_300_piles(cc, form):
    """65 + 300 piles x 128 envs, the random policy; the oracle with room for stations of more than 256 piles (orclib.big_oracle)"""
    free_run(form, cg.expectation(cc, "random", BIG_SHAPE, BIG_N), cc)


# ---------------------------------------------------------------------------------------------- c. the ties
TIE_CASES = [(cc, form) for cc in MODES for form in ("packed_small", "wave")]


@pytest.mark.parametrize("cc,form", TIE_CASES, ids=["%s-%s" % (mode_id(c), f) for c, f in TIE_CASES])
def test_the_urgency_decision_on_its_boundary(cc, form):
    """must_charge is `time_left <= ceilf(needed)` (CHS.hpp:879-898).  Every (class, car_steps, level) whose need is a whole number m of
    slots sits in every fourth pile, with m + 1 slots left (not urgent) and with m (urgent); every action is off, so the urgency test
    alone decides.  `<`, a ceil written as (int) x + 1 and a `needed >= 0` guard all part from the reference here and nowhere else.
    (fast, constant) has no such triple: its piles hold grid cars only.  A car with one slot left charges and leaves in the same step: the
    urgent side of a tie with m = 1 shows in no field, on no side (tests/test_class_grid_cpu.py says which those are)."""
    tc = cg.tie_case(cc)
    ex, pre = tc.ex, tc.pre
    v = make(form, ex.shape, ex.n, cc)
    place_grid(v, ex, tc.rows)
    compare_step(v, ex, pre, "%s: the ties as placed" % form, masked=True)
    v.step(cg.action_rows(ex.bits[pre]))
    assert not ex.bits[pre].any()
    compare_step(v, ex, pre + 1, "%s: the deciding step" % form, masked=True)
    # ... and said once more for the flag alone: of the tie cars still there, exactly those that had m slots left have charged
    sl = v.slots()
    charge = np.concatenate([sl[0][:, 1], sl[1][:, 1]], axis=1)
    e, s, _, urgent = tc.slots.T
    there = ex.present(pre + 1)[e, s]
    assert there.sum() > len(e) // 2 and (urgent[there] == 1).any() and (urgent[there] == 0).any()
    assert np.array_equal(charge[e, s][there] > 0.5, urgent[there] == 1)
    v.close()
