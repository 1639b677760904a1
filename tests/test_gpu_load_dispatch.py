"""Station-level control on the device (include/chub.h: chub_load_dispatch_device): one target per station in, an action row and / or one
bit per pile out, by one read-only launch.  Held here: (1) the outputs against tests/load_dispatch_lib.py's numpy definition applied to
the handle's own pile columns and station scalars, bit for bit, over hub shapes x RNG modes x moments x kinds of load x units; (2) twin
handles where chub_step_load exists: the scalar-load step against dispatch + the production step forms; (3) twin handles where it does not
(PHILOX_CURVES, per-env rows): the device's dispatch against host-computed rows through the auto-reset and device-mask steps; (4) manners:
masks, graphs, neutrality, determinism, refusals; (5) the torch adapter's control="station".  Every output buffer is pre-filled with a
pattern no kernel writes."""
import numpy as np
import pytest

import load_dispatch_lib as ldl
from charginghub_env_amd import _lib
from test_gpu_autoreset import Dev, buffers, same_state
from test_gpu_parity import hub
from test_gpu_pile_obs import BASE, CANARY, MODES, Driver, make, variates

pytestmark = pytest.mark.gpu

F32 = np.float32
TYPES = [0, 1]  # BASE: station 0 fast, station 1 slow
EXTRA = 64      # words behind each output that must keep the pattern
CANARY64 = np.uint64(0x7FC0BEEF7FC0BEEF)


class Disp(object):
    """device buffers of one dispatch call on n envs of a hub of S piles, pattern-filled before every call"""

    def __init__(self, v):
        mg = buffers()
        self.n, self.A, self.W = v.n_envs, v.act_dim, v.bit_words
        self.loads, self.tail, self.mask = mg.DeviceBuffer(self.n * 8), mg.DeviceBuffer(self.n * 8), mg.DeviceBuffer(self.n)
        self.rows, self.bits = mg.DeviceBuffer((self.n * self.A + EXTRA) * 4), mg.DeviceBuffer((self.n * self.W + EXTRA) * 8)

    def call(self, v, loads, tail, units="kw", mask=None, rows=True, bits=True):
        """-> (rows as uint32 words [N, A], bits uint64 [N, W]) as the buffers stand after the call; the words behind them are checked"""
        n, A, W = self.n, self.A, self.W
        self.loads.from_host(np.ascontiguousarray(loads, dtype=F32))
        self.tail.from_host(np.ascontiguousarray(tail, dtype=F32))
        self.rows.from_host(np.full(n * A + EXTRA, CANARY, dtype=np.uint32))
        self.bits.from_host(np.full(n * W + EXTRA, CANARY64, dtype=np.uint64))
        if mask is not None:
            self.mask.from_host(np.ascontiguousarray(mask, dtype=np.uint8))
        v.sync()
        v.load_dispatch_device(self.loads.ptr, self.tail.ptr, d_actions=self.rows.ptr if rows else 0, d_pile_bits=self.bits.ptr if bits else 0,
                               units=units, d_mask=self.mask.ptr if mask is not None else 0)
        v.sync()
        r, b = self.rows.to_host(np.uint32, (n * A + EXTRA,)), self.bits.to_host(np.uint64, (n * W + EXTRA,))
        assert (r[n * A:] == CANARY).all() and (b[n * W:] == CANARY64).all(), "the words past the outputs"
        return r[:n * A].reshape(n, A), b[:n * W].reshape(n, W)

    def free(self):
        for b in (self.loads, self.tail, self.mask, self.rows, self.bits):
            b.free()


def columns(v):
    return v.pile_obs(("car", "emergency", "power")), v.station_scalars()


def expected(v, loads, tail, units=ldl.KW, cc=False, details=False):
    cols, scal = columns(v)
    return ldl.hub_dispatch(cols, scal, v.piles, TYPES, cc, loads, tail, units, details)


def check(got, want, what):
    (rows, bits), (w_rows, w_bits) = got, want[:2]
    bad = np.nonzero(rows != w_rows.view(np.uint32))
    assert bad[0].size == 0, (what, "rows: first (env, entry)", [int(x[0]) for x in bad], bad[0].size)
    assert np.array_equal(bits, w_bits), (what, "bits", np.nonzero(bits != w_bits)[0][:5])


def running_sums(cols, piles):
    """per station [N, S_k] f32: the definition's running sum along the urgency order (0 where the station has no piles)"""
    out = []
    s0 = piles[0]
    for k in range(2):
        sl = slice(0, s0) if k == 0 else slice(s0, s0 + piles[1])
        car, em, pw = cols[:, 0, sl] > 0.5, cols[:, 1, sl], cols[:, 2, sl]
        order = np.argsort(-em, axis=1, kind="stable")
        out.append(np.cumsum(np.take_along_axis(np.where(car, pw, F32(0)).astype(F32), order, axis=1), axis=1, dtype=F32))
    return out


def kinds_of_load(v, rs, units, moment):
    """per env, by env index mod 6: inside the range, below, above, exactly mn, exactly mx, exactly the running sum of the j-th pile of the order
    (in fraction units: the action that comes nearest to it)"""
    n = v.n_envs
    cols, scal = columns(v)
    cums = running_sums(cols, v.piles)
    kind = np.arange(n) % 6
    loads = np.zeros((n, 2), dtype=F32)
    for k in range(2):
        mn, mx = scal[:, k, 0].astype(F32), scal[:, k, 2].astype(F32)
        u = rs.uniform(size=n).astype(F32)
        cum = cums[k][np.arange(n), (np.arange(n) // 6 + moment) % v.piles[k]] if v.piles[k] else np.zeros(n, dtype=F32)
        if units == ldl.KW:
            loads[:, k] = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [mn + u * (mx - mn), mn - F32(1) - u, mx + F32(1) + u, mn, mx], cum)
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                a_cum = np.nan_to_num(F32(2) * (cum - mn) / (mx - mn) - F32(1), nan=0.0, posinf=2.0, neginf=-2.0).astype(F32)
            loads[:, k] = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [F32(2) * u - F32(1), -F32(1.5) - u, F32(1.5) + u, F32(-1), F32(1)], a_cum)
    return loads


# ---- 1. device output == the definition
HUBS = ([1, 0], [0, 1], [3, 2], [20, 25], [64, 64], [65, 7], [255, 257], [300, 270])
SHAPES = [(rng, piles, False) for rng in MODES for piles in HUBS if not (rng == "philox_curves" and max(piles) > 64)] + \
         [(rng, [20, 25], True) for rng in MODES]


@pytest.mark.parametrize("rng,piles,cc", SHAPES, ids=lambda c: str(c).replace(" ", ""))
def test_outputs_equal_the_definition_on_the_handles_own_columns(rng, piles, cc):
    """n = 33: on [20, 25] one workgroup of 22 envs and one of 11, on [300, 270] seven envs per sort and a last group of five; after the
    reset and after 1, 2 and 30 steps of random actions; six kinds of load per station, both units; rows alone, bits alone and both."""
    n = 33
    v = make(rng, piles, n, constant_charging=cc)
    out = Disp(v)
    d = Driver(v, rng)
    d.reset()
    rs = np.random.RandomState(21)
    S, W = v.n_slots, v.bit_words
    seen = dict(on=0, off=0, must=0, partial=0)
    step = 0
    for moment in (0, 1, 2, 30):
        while step < moment:
            d.step()
            step += 1
        for units, name in ((ldl.KW, "kw"), (ldl.FRACTION, "fraction")):
            loads = kinds_of_load(v, rs, units, moment)
            tail = rs.uniform(-1, 1, size=(n, 2)).astype(F32)
            want = expected(v, loads, tail, units, cc, details=True)
            got = out.call(v, loads, tail, name)
            check(got, want, (rng, piles, cc, "step", moment, name))
            rows, bits = got
            assert np.array_equal(rows[:, S:], tail.view(np.uint32)), "the tail is passed through"
            on = rows.view(F32)[:, :S] == 1
            assert np.array_equal(np.where(on, F32(1), F32(-1)).view(np.uint32), rows[:, :S]), "pile entries are exactly +1 or -1"
            assert np.array_equal(ldl.pack_bits(on), bits), "rows and bits agree; bits from S up are zero"
            if S % 64:
                assert not (bits[:, W - 1] >> np.uint64(S % 64)).any()
            cols = columns(v)[0]
            assert not (on & (cols[:, 0] < 0.5)).any(), "an empty pile is never on"
            seen["on"] += int(on.sum())
            seen["off"] += int((~on & (cols[:, 0] > 0.5)).sum())
            seen["must"] += int(((cols[:, 1] == 10) & (cols[:, 0] > 0.5)).sum())
            seen["partial"] += int(((on.sum(axis=1) > 0) & ((~on & (cols[:, 0] > 0.5)).sum(axis=1) > 0)).sum())
            if moment == 2:  # one output at a time: the other buffer keeps its pattern
                r_only, b_none = out.call(v, loads, tail, name, bits=False)
                assert np.array_equal(r_only, rows) and (b_none == CANARY64).all()
                r_none, b_only = out.call(v, loads, tail, name, rows=False)
                assert np.array_equal(b_only, bits) and (r_none == CANARY).all()
    a, b = v.load_dispatch(loads, tail, units="fraction")
    check((a.view(np.uint32), b), want, (rng, piles, "the host form"))
    if piles == [20, 25]:
        assert seen["on"] > 100 and seen["off"] > 100 and seen["must"] > 10 and seen["partial"] > 10, seen
    out.free()
    v.close()


def test_a_station_of_4096_piles():
    """[4096, 3], 2 envs: two sorting passes per env (4099 piles do not fit one), the bit word at the stations' border written once"""
    v = make("philox", [4096, 3], 2)
    out = Disp(v)
    v.reset()
    rs = np.random.RandomState(2)
    for _ in range(3):
        v.step(rs.uniform(-1, 1, size=(2, v.act_dim)).astype(F32))
    scal = v.station_scalars()
    loads = np.stack([scal[:, 0, 0] + 0.37 * (scal[:, 0, 2] - scal[:, 0, 0]), scal[:, 1, 2]], axis=1).astype(F32)
    tail = np.array([[0.5, -0.25], [-1, 1]], dtype=F32)
    got = out.call(v, loads, tail)
    check(got, expected(v, loads, tail), "[4096, 3]")
    on = got[0].view(F32)[:, :4099] == 1
    assert 100 < on[:, :4096].sum() < (columns(v)[0][:, 0, :4096] > 0.5).sum() and got[1].shape == (2, 65)
    out.free()
    v.close()


def test_a_range_of_many_workgroups():
    """65 536 envs x [20, 25]: 2979 workgroups of 22 envs (the last holds 20)"""
    n = 65536
    v = make("philox", [20, 25], n)
    mg = buffers()
    d_act, packed = mg.DeviceBuffer(n * v.act_dim * 4), mg.DeviceBuffer(n * (v.obs_dim + 2) * 4)
    v.reset()
    for b in range(10):
        v.random_actions_device(d_act.ptr, 5, b)
        v.step_device_packed(d_act.ptr, packed.ptr)
    v.sync()
    rs = np.random.RandomState(3)
    loads, tail = rs.uniform(-1.2, 1.2, size=(n, 2)).astype(F32), rs.uniform(-1, 1, size=(n, 2)).astype(F32)
    out = Disp(v)
    got = out.call(v, loads, tail, "fraction")
    check(got, expected(v, loads, tail, ldl.FRACTION), "65 536 envs")
    on = got[0].view(F32)[:, :45] == 1
    assert on.sum() > 5 * n and on[-1].any() and (~on).sum() > 5 * n
    for b in (d_act, packed):
        b.free()
    out.free()
    v.close()


# ---- 2. twin handles, where chub_step_load exists
class Twin(object):
    """one handle stepped through a given form, with its device buffers"""

    def __init__(self, v, form):
        self.v, self.form, self.d, self.disp = v, form, Dev(v), Disp(v)

    def step(self, loads, tail, z):
        v, d, n = self.v, self.d, self.v.n_envs
        if z is not None:
            d.z.from_host(np.ascontiguousarray(z, dtype=np.float64))
        dz = d.z.ptr if z is not None else 0
        if self.form == "load":
            d.act.from_host(v.load_actions(loads, tail))
            v.step_load_device(d.act.ptr, d.obs.ptr, d.rew.ptr, d.done.ptr, d_exo_z=dz)
            v.sync()
            return d.obs.to_host(F32, (n, v.obs_dim)), d.rew.to_host(F32, (n,)), d.done.to_host(np.uint8, (n,)).astype(F32)
        self.disp.loads.from_host(np.ascontiguousarray(loads, dtype=F32))
        self.disp.tail.from_host(np.ascontiguousarray(tail, dtype=F32))
        if self.form == "rows":
            v.load_dispatch_device(self.disp.loads.ptr, self.disp.tail.ptr, d_actions=d.act.ptr)
            v.step_device_packed(d.act.ptr, d.packed.ptr, d_exo_z=dz)
        else:
            v.load_dispatch_device(self.disp.loads.ptr, self.disp.tail.ptr, d_pile_bits=self.disp.bits.ptr)
            v.step_bits_device_packed(self.disp.bits.ptr, self.disp.tail.ptr, d.packed.ptr, d_exo_z=dz)
        v.sync()
        p = d.packed.to_host(F32, (n, v.obs_dim + 2))
        return p[:, :v.obs_dim], p[:, v.obs_dim], p[:, v.obs_dim + 1]

    def state(self):
        return [np.concatenate([x.reshape(self.v.n_envs, -1) for x in self.v.slots()], axis=1), self.v.station_scalars().reshape(self.v.n_envs, -1)]

    def close(self):
        self.disp.free()
        self.v.close()


TWINS = [("compat", "auto", [20, 25], False), ("compat", "auto", [5, 3], True),
         ("philox", "off", [20, 25], False), ("philox", "on", [20, 25], False), ("philox", "off", [5, 3], True), ("philox", "on", [5, 3], True)]


@pytest.mark.parametrize("rng,fused,piles,cc", TWINS, ids=lambda c: str(c).replace(" ", ""))
def test_dispatch_then_step_equals_the_scalar_load_step(rng, fused, piles, cc):
    """A takes chub_step_load_device; B dispatch (rows) + chub_step_device_packed; in PHILOX a third twin dispatch (bits) +
    chub_step_bits_device_packed, B and C on the two-launch or the one-launch step.  64 envs, 120 steps with a reset at 96 (COMPAT: per-env
    seeds): state, obs, reward and done bit-identical throughout.  An env in which the definition finds a must-charge car beyond the load
    (the scalar-load step leaves it off, a stepped row cannot) leaves the comparison from that step on; at least 90 % must stay to the end
    (on the CPU oracle the case did not occur in 73 728 station-steps)."""
    n = 64
    compat = rng == "compat"
    extra = dict(constant_charging=cc)
    forms = ["load", "rows"] + ([] if compat else ["bits"])
    twins = [Twin(make(rng, piles, n, **(extra if form == "load" or compat else dict(extra, fused_step=fused))), form) for form in forms]
    if not compat:
        assert twins[1].v.uses_packed_kernel and twins[1].v.uses_fused_step == (fused == "on")
    rs = np.random.RandomState(31)
    compared = np.ones(n, dtype=bool)
    beyond_steps = 0

    def reset():
        days, z = variates(rs, n) if compat else (None, None)
        obs = [t.v.reset(days, z).copy() for t in twins]
        for o in obs[1:]:
            assert np.array_equal(obs[0][compared], o[compared])

    reset()
    for step in range(120):
        if step == 96:
            reset()
        ref = twins[1]
        scal = ref.v.station_scalars()
        loads = (rs.uniform(size=(n, 2)) * (1.2 * scal[:, :, 2] + 1)).astype(F32)
        tail = rs.uniform(-1, 1, size=(n, 2)).astype(F32)
        beyond = expected(ref.v, loads, tail, ldl.KW, cc, details=True)[2]
        beyond_steps += int((beyond[compared] > 0).sum())
        compared &= ~(beyond > 0).any(axis=1)
        z = rs.normal(size=(n, 3)) if compat else None
        outs = [t.step(loads, tail, z) for t in twins]
        states = [t.state() for t in twins]
        for t, o, s in zip(twins[1:], outs[1:], states[1:]):
            for k, (x, y) in enumerate(zip(outs[0] + tuple(states[0]), o + tuple(s))):
                assert np.array_equal(np.ascontiguousarray(x[compared]).view(np.uint8), np.ascontiguousarray(y[compared]).view(np.uint8)), \
                    (rng, fused, piles, t.form, "step", step, "array", k)
    print("unit-steps with a must-charge car beyond the load: %d; envs compared to the end: %d of %d" % (beyond_steps, compared.sum(), n))
    assert compared.mean() >= 0.9, (beyond_steps, compared.sum())
    for t in twins:
        t.close()


# ---- 3. twin handles, where chub_step_load does not exist
@pytest.mark.parametrize("rng,rows", [("philox_curves", False), ("philox", True), ("compat", True)], ids=["curves", "philox-rows", "compat-rows"])
def test_device_dispatch_equals_host_rows_where_the_scalar_load_step_is_refused(rng, rows):
    """A: dispatch on the device, then chub_autoreset_step_device; B: the rows the definition gives on B's own columns, fed to the same call.
    200 calls across a day's end on staggered clocks: the packed outputs are bit-identical; then once through chub_dmask_step_envs_device
    with one device mask shared by dispatch and step."""
    n = 24
    compat = rng == "compat"
    extra = {}
    if rows:
        r5 = np.random.RandomState(5)
        extra = dict(init_soc=list(r5.uniform(0.15, 0.6, n)), hydro_store_vlt=list(r5.uniform(20, 60, n)))
    a, b = make(rng, [20, 25], n, **extra), make(rng, [20, 25], n, **extra)
    assert a.has_env_params == rows
    rs = np.random.RandomState(41)
    days, z = variates(rs, n) if compat else (None, None)
    for v in (a, b):
        v.reset(days, z)
    with pytest.raises(hub().ChubError, match="error -4"):  # (what this test is about: no scalar-load step here; a refused call changes nothing)
        a.step_load(np.zeros((n, 2), F32), np.zeros((n, 2), F32), np.zeros((n, 3)) if compat else None)
    for k in range(1, 31):  # staggered clocks: env e is e % 3 * 15 slots ahead
        act = rs.uniform(-1, 1, size=(n, a.act_dim)).astype(F32)
        z = rs.normal(size=(n, 3)) if compat else None
        m = (np.arange(n) % 3) * 15 >= k
        for v in (a, b):
            v.step_envs(m, act, z)
    assert a.clock_groups == 3
    da, db, disp = Dev(a), Dev(b), Disp(a)
    ended = np.zeros(n, dtype=int)
    for call in range(200):
        loads, tail = rs.uniform(-1.3, 1.3, size=(n, 2)).astype(F32), rs.uniform(-1, 1, size=(n, 2)).astype(F32)
        z, rdays, rz = (rs.normal(size=(n, 3)),) + variates(rs, n) if compat else (None, None, None)
        want_rows = expected(b, loads, tail, ldl.FRACTION)[0]
        pb, _ = db.autoreset(want_rows, z, rdays, rz)
        disp.loads.from_host(loads)
        disp.tail.from_host(tail)
        if compat:
            da.z.from_host(z)
            da.rdays.from_host(rdays)
            da.rz.from_host(rz)
        a.load_dispatch_device(disp.loads.ptr, disp.tail.ptr, d_actions=da.act.ptr, units="fraction")
        a.step_autoreset_device(da.act.ptr, da.packed.ptr, da.final.ptr, d_exo_z=da.z.ptr if compat else 0,
                                d_reset_exo_days=da.rdays.ptr if compat else 0, d_reset_exo_z=da.rz.ptr if compat else 0)
        a.sync()
        pa = da.packed.to_host(F32, (n, a.obs_dim + 2))
        assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), (rng, "auto-reset call", call)
        assert np.array_equal(da.act.to_host(np.uint32, (n, a.act_dim)), want_rows.view(np.uint32)), (rng, "rows", call)
        ended += pa[:, -1] > 0.5
    assert (ended >= 2).all()
    # the same once through the device-mask step, the mask shared by dispatch and step
    mask = rs.uniform(size=n) < 0.5
    mask[0], mask[1] = True, False
    loads, tail = rs.uniform(-1.3, 1.3, size=(n, 2)).astype(F32), rs.uniform(-1, 1, size=(n, 2)).astype(F32)
    z = rs.normal(size=(n, 3)) if compat else None
    want_rows = expected(b, loads, tail, ldl.FRACTION)[0]
    ob = db.step_dmask(mask, want_rows, z)
    disp.loads.from_host(loads)
    disp.tail.from_host(tail)
    da.mask.from_host(mask.astype(np.uint8))
    da.act.from_host(np.full((n, a.act_dim), -3, dtype=F32))
    if compat:
        da.z.from_host(z)
    a.load_dispatch_device(disp.loads.ptr, disp.tail.ptr, d_actions=da.act.ptr, units="fraction", d_mask=da.mask.ptr)
    a.step_envs_dmask_device(da.mask.ptr, da.act.ptr, da.obs.ptr, da.rew.ptr, da.done.ptr, d_exo_z=da.z.ptr if compat else 0)
    a.sync()
    got_rows = da.act.to_host(F32, (n, a.act_dim))
    assert np.array_equal(got_rows[mask], want_rows[mask]) and (got_rows[~mask] == -3).all()
    oa = (da.obs.to_host(F32, (n, a.obs_dim)), da.rew.to_host(F32, (n,)), da.done.to_host(np.uint8, (n,)))
    for x, y in zip(oa, ob):
        assert np.array_equal(x[mask], y[mask]), (rng, "device-mask step")
    for x, y in zip(Twin.state(da), Twin.state(db)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (rng, "state after the device-mask step")
    disp.free()
    a.close()
    b.close()


# ---- 4. manners
@pytest.mark.parametrize("rng", MODES)
def test_a_device_mask_writes_only_the_rows_it_names(rng):
    n = 67
    v = make(rng, [20, 25], n)
    out = Disp(v)
    d = Driver(v, rng)
    d.reset()
    for _ in range(6):
        d.step()
    rs = np.random.RandomState(7)
    loads, tail = rs.uniform(-1, 1, size=(n, 2)).astype(F32), rs.uniform(-1, 1, size=(n, 2)).astype(F32)
    want = expected(v, loads, tail, ldl.FRACTION)
    check(out.call(v, loads, tail, "fraction"), want, rng)
    m = np.zeros(n, dtype=np.uint8)
    m[[0, 3, 21, 22, 64, 66]] = 1
    m[3] = 255  # (any non-zero byte names an env)
    for mask in (m, np.zeros(n, dtype=np.uint8), np.ones(n, dtype=np.uint8)):
        rows, bits = out.call(v, loads, tail, "fraction", mask=mask)
        on = mask != 0
        assert np.array_equal(rows[on], want[0].view(np.uint32)[on]) and np.array_equal(bits[on], want[1][on]), (rng, "named rows")
        assert (rows[~on] == CANARY).all() and (bits[~on] == CANARY64).all(), (rng, "every other row keeps the pattern")
    out.free()
    v.close()


def test_recorded_into_a_graph_it_equals_eager_on_a_twin():
    """18 x (dispatch, auto-reset step) captured on a handle at step 90 of its day (36 launches of env calls: the dispatches do not count),
    replayed 5 times with new loads (the day ends in the first replay), against the same calls made eagerly on a twin"""
    mg = buffers()
    n = 52

    def start():
        v = make("philox", [20, 25], n, seed=77)
        v.set_telemetry(True)  # (same_state reads the f64 observation and reward, which the telemetry keeps)
        v.reset()
        rs = np.random.RandomState(1)
        for _ in range(89):
            v.step(rs.uniform(-1, 1, size=(n, v.act_dim)).astype(F32))
        act = rs.uniform(-1, 1, size=(n, v.act_dim)).astype(F32)
        for half in (np.arange(n) < n // 2, np.arange(n) >= n // 2):  # (a capture of auto-reset calls starts on per-env clocks)
            v.step_envs(half, act)
        return v

    g, e = start(), start()
    st = mg.Stream(0)
    dg, de, xg, xe = Dev(g, st.ptr), Dev(e), Disp(g), Disp(e)
    st.sync()
    g.graph_begin(st.ptr)
    for k in range(18):
        g.load_dispatch_device(xg.loads.ptr, xg.tail.ptr, d_actions=dg.act.ptr, d_pile_bits=xg.bits.ptr, units="fraction", stream=st.ptr)
        g.step_autoreset_device(dg.act.ptr, dg.packed.ptr, dg.final.ptr, stream=st.ptr)
    graph = g.graph_end(st.ptr)
    rs = np.random.RandomState(8)
    for r in range(5):
        loads, tail = rs.uniform(-1.2, 1.2, size=(n, 2)).astype(F32), rs.uniform(-1, 1, size=(n, 2)).astype(F32)
        xg.loads.from_host(loads, st.ptr)
        xg.tail.from_host(tail, st.ptr)
        g.graph_launch(graph, st.ptr)
        xe.loads.from_host(loads)
        xe.tail.from_host(tail)
        for k in range(18):
            if k == 17:
                want = expected(e, loads, tail, ldl.FRACTION)
            e.load_dispatch_device(xe.loads.ptr, xe.tail.ptr, d_actions=de.act.ptr, d_pile_bits=xe.bits.ptr, units="fraction")
            e.step_autoreset_device(de.act.ptr, de.packed.ptr, de.final.ptr)
        e.sync()
        st.sync()
        got = (dg.act.to_host(np.uint32, (n, g.act_dim), st.ptr), xg.bits.to_host(np.uint64, (n, g.bit_words), st.ptr))
        check(got, want, ("replay", r, "the last dispatch against the definition on the twin"))
        assert np.array_equal(dg.packed.to_host(np.uint32, (n, g.obs_dim + 2), st.ptr), de.packed.to_host(np.uint32, (n, e.obs_dim + 2))), r
        same_state(g, e, ("replay", r))
    g.graph_destroy(graph)
    for x in (xg, xe):
        x.free()
    g.close()
    e.close()
    st.destroy()


@pytest.mark.parametrize("rng", MODES)
def test_the_call_leaves_no_trace_and_two_calls_agree(rng):
    """A twin that never dispatches ends in the same state and at the same tick; two calls on one state give identical bits; the snapshot
    of the handle is the same blob before and after a call."""
    n = 21
    v, w = make(rng, [20, 25], n, seed=3), make(rng, [20, 25], n, seed=3)
    for x in (v, w):
        x.set_telemetry(True)
    out = Disp(v)
    dv, dw = Driver(v, rng), Driver(w, rng)
    dv.reset()
    dw.reset()
    rs = np.random.RandomState(5)
    for t in range(12):
        loads, tail = rs.uniform(-1, 1, size=(n, 2)).astype(F32), rs.uniform(-1, 1, size=(n, 2)).astype(F32)
        out.call(v, loads, tail, "fraction")
        out.call(v, 30 * loads, tail, "kw", bits=False)
        ov, ow = dv.step(), dw.step()
        assert all(np.array_equal(p, q) for p, q in zip(ov[:3], ow[:3])), (rng, "step outputs", t)
    same_state(v, w, (rng, "a twin that never dispatches"))
    blob = v.get_state()
    first = out.call(v, loads, tail, "fraction")
    second = out.call(v, loads, tail, "fraction")
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    assert np.array_equal(blob, v.get_state()), (rng, "snapshot blobs")
    out.free()
    v.close()
    w.close()


def test_refusals():
    chub = hub()
    n = 8
    v = make("philox", [20, 25], n)
    out = Disp(v)
    lib, h = v._lib, v._h
    ld, tl, rw, bt = out.loads.ptr, out.tail.ptr, out.rows.ptr, out.bits.ptr
    dev = lib.chub_load_dispatch_device
    v.reset()
    assert dev(None, 0, ld, tl, None, rw, bt, None) == -1 and dev(h, 0, None, tl, None, rw, bt, None) == -1
    assert dev(h, 0, ld, tl, None, None, None, None) == -1 and "both" in lib.chub_last_error().decode()
    assert dev(h, 0, ld, None, None, rw, None, None) == -1 and "d_tail" in lib.chub_last_error().decode()
    assert dev(h, 2, ld, tl, None, rw, bt, None) == -1 and dev(h, -1, ld, tl, None, rw, bt, None) == -1
    assert dev(h, 1, ld, None, None, None, bt, None) == 0  # bits alone need no tail
    v.sync()
    with pytest.raises(ValueError, match="load units"):
        v.load_dispatch_device(ld, tl, d_actions=rw, units="percent")
    with pytest.raises(AssertionError):
        v.load_dispatch(np.zeros((n, 3), F32), np.zeros((n, 2), F32))
    with pytest.raises(chub.ChubError, match="error -1"):
        v.load_dispatch_device(ld, tl)
    size = v.get_state().size
    out.call(v, np.zeros((n, 2), F32), np.zeros((n, 2), F32))
    assert v.get_state().size == size
    v.tape_register_soc(np.array([50.0], dtype=F32))  # a tape handle from here on
    assert dev(h, 0, ld, tl, None, rw, bt, None) == -4 and "tape handle" in lib.chub_last_error().decode()
    with pytest.raises(chub.ChubError, match="tape handle"):
        v.load_dispatch(np.zeros((n, 2), F32), np.zeros((n, 2), F32))
    out.free()
    v.close()


# ---- 5. the torch adapter
TORCH_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["CHUB_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHUB_ROOT"], "tests"))
import torch  # before libchub: both must share one HIP runtime
if not torch.cuda.is_available():
    print("TORCH_WITHOUT_A_DEVICE")
    sys.exit(0)
torch.cuda.set_device(0)
import test_gpu_load_dispatch
test_gpu_load_dispatch.torch_adapter_station_control()
print("TORCH_LOAD_DISPATCH_OK")
"""


def test_torch_adapter():
    """in a child process that imports torch first (as tests/test_gpu_torch_side.py does); torch is not imported here: in a process that
    has already used libchub it may find no device, and whether it has one is the child's to say"""
    import importlib.util
    import os
    import subprocess
    import sys
    if importlib.util.find_spec("torch") is None:
        pytest.skip("no torch")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], env=dict(os.environ, CHUB_ROOT=root), capture_output=True, text=True, timeout=300)
    if r.returncode == 0 and "TORCH_WITHOUT_A_DEVICE" in r.stdout:
        pytest.skip("torch without a device")
    assert r.returncode == 0 and "TORCH_LOAD_DISPATCH_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def torch_adapter_station_control():
    import torch
    from charginghub_env_amd import wrappers
    n = 16
    kw = {k: BASE[k] for k in BASE if k != "station_type_list"}
    for autoreset in ("per_env", True, False):
        for units in ("fraction", "kw"):
            s = wrappers.TorchHubVecEnv(n, [20, 25], ["fast", "slow"], seed=13, autoreset=autoreset, control="station", load_units=units, **kw)
            p = wrappers.TorchHubVecEnv(n, [20, 25], ["fast", "slow"], seed=13, autoreset=autoreset, **kw)
            assert s.act_dim == 4 and p.act_dim == 47 and s.control == "station" and p.control == "pile"
            assert torch.equal(s.reset(), p.reset())
            g = torch.Generator(device="cuda").manual_seed(1)
            for t in range(100 if units == "fraction" else 10):
                act = torch.rand((n, 4), device="cuda", generator=g) * 2 - 1
                if units == "kw":
                    act[:, :2] = (act[:, :2] + 1) * 60
                host = act.cpu().numpy()
                rows = expected(p.vec, host[:, :2], host[:, 2:], _lib.LOAD_UNITS[units])[0]
                os_, rs_, ds_, _ = s.step(act)
                op, rp, dp, _ = p.step(torch.from_numpy(rows).cuda())
                assert torch.equal(s._rows.cpu(), torch.from_numpy(rows)), (autoreset, units, "rows", t)
                assert torch.equal(os_, op) and torch.equal(rs_, rp) and torch.equal(ds_, dp), (autoreset, units, "step", t)
                if t in (95, 96) and autoreset is not False:
                    assert torch.equal(s.last_obs, p.last_obs)
            with pytest.raises(RuntimeError, match="control='station'"):
                s.step_bits(torch.zeros((n, 1), dtype=torch.int64, device="cuda"), torch.zeros((n, 2), device="cuda"))
            with pytest.raises(AssertionError):
                s.step(torch.zeros((n, 47), device="cuda"))
            s.close()
            p.close()
