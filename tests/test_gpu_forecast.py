"""The exogenous look-ahead on the device (include/chub.h: chub_forecast_device): per env the next H slots of what is deterministic about
its day -- slot, time features, tariff, PV / wind profiles of its days, mean arrivals -- [N][C][H], written by one launch.  The expected
values are always tests/forecast_lib.py's numpy definition (held to the oracle's simulation by tests/test_forecast_cpu.py) on the clocks
chub_env_clocks reports and the days of the telemetry columns; the comparison is bit for bit and every output buffer is pre-filled with a
NaN no kernel writes, with a guard row behind it.  Held here: (1) RNG modes x horizons x field sets on a lock-step handle, and blocks that
straddle waves and workgroups; (2) per-env clocks, a wrapped day, the auto-reset step; (3) device masks; (4) per-env rows; (5) user series;
(6) neutrality; (7) captured graphs; (8) the anchor against the simulation; (9) the law of the FCEV count; (10) refusals; (11) the torch
adapter."""
import numpy as np
import pytest

import forecast_lib as fl
from charginghub_env_amd import _lib
from test_gpu_autoreset import Dev, buffers
from test_gpu_parity import hub
from test_gpu_pile_obs import BASE, CANARY, MODES, Driver, bits, make

pytestmark = pytest.mark.gpu

FC, T = _lib.FC, _lib.T
ALL = (1 << _lib.FC_COUNT) - 1
TYPES = ("fast", "slow")
GUARD = 256  # words behind the output that must keep the canary
FIELD_SETS = [ALL] + [1 << f for f in range(_lib.FC_COUNT)] + [1 << FC["price"] | 1 << FC["fcev"]]


def cols_of(fields):
    mask = _lib.fc_fields_mask(fields)
    return [f for f in range(_lib.FC_COUNT) if mask >> f & 1]


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(bits(got) != bits(want))
    assert bad[0].size == 0, (what, "first (env, column, h)", [int(x[0]) for x in bad], bad[0].size, got[bad][:5], want[bad][:5])


class Out(object):
    """a device buffer for up to `floats` floats, canary-filled before every call, with a guard row behind it"""

    def __init__(self, floats):
        self.floats = floats
        self.buf = buffers().DeviceBuffer((floats + GUARD) * 4)

    def raw(self, v, fields, H, d_mask=0, stream=0):
        """the call into a canary-filled buffer -> the N * C * H words it may write as uint32 [N, C, H]; everything behind them is intact"""
        C_ = len(cols_of(fields))
        count = v.n_envs * C_ * H
        assert count <= self.floats
        self.buf.from_host(np.full(self.floats + GUARD, CANARY, dtype=np.uint32))
        v.sync()
        v.forecast_device(self.buf.ptr, fields, H, d_mask=d_mask, stream=stream)
        v.sync()
        words = self.buf.to_host(np.uint32, (self.floats + GUARD,))
        assert (words[count:] == CANARY).all(), (fields, H, "the words past N * C * H")
        return words[:count].reshape(v.n_envs, C_, H)

    def call(self, v, fields=None, H=8):
        words = self.raw(v, fields, H)
        assert not (words == CANARY).any(), (fields, H, "every word of every block is written")
        return words.view(np.float32)

    def free(self):
        self.buf.free()


def where(v):
    """(clock, PV day, wind day) of every env: chub_env_clocks and the telemetry columns"""
    tel = v.telemetry()
    return v.env_clocks().astype(np.int64), tel[:, T["pv_day"]].astype(np.int64), tel[:, T["wd_day"]].astype(np.int64)


def expected(v, fields=None, H=8, at=None, data_dir=None, types=TYPES):
    t, pv, wd = at if at is not None else where(v)
    return fl.forecast(fl.data(data_dir), types, t, pv, wd, v.env_params()["fcev_permeate"], fields, H)


def made(rng, piles, n, **extra):
    v = make(rng, piles, n, **extra)
    v.set_telemetry(True)  # (the days an env drew are telemetry columns)
    return v


# ---- 1. modes x horizons x field sets, lock-step
@pytest.mark.parametrize("rng", MODES)
def test_lock_step_columns_equal_the_definition(rng):
    """6 envs x [3, 2]: right after the reset, after 3 steps and at clock 95; H = 1, 8 and 96; all fields, every single field and
    PRICE | FCEV.  The definition is evaluated once per moment (all fields, H = 96): a field set selects columns, a horizon a prefix."""
    n = 6
    v = made(rng, [3, 2], n)
    out = Out(n * 10 * 96)
    d = Driver(v, rng)
    d.reset()
    steps = 0
    for clock in (0, 3, 95):
        while steps < clock:
            d.step()
            steps += 1
        assert (v.env_clocks() == clock).all() and v.clock_groups == 1
        want = expected(v, None, 96)
        for H in (1, 8, 96):
            for fields in FIELD_SETS:
                assert v._lib.chub_forecast_size(fields, H) == len(cols_of(fields)) * H
                same(out.call(v, fields, H), want[:, cols_of(fields), :H], (rng, "clock", clock, "H", H, "fields", fields))
        same(v.forecast(None, 96), want, (rng, clock, "the host form"))
        same(v.forecast(("price", "fcev", "pv"), 5), want[:, cols_of(("pv", "price", "fcev")), :5], (rng, clock, "the host form by name"))
        if clock == 95:  # only h = 0 lies inside the day; the rest wraps with the current days
            assert (want[:, FC["valid"], 0] == 1).all() and (want[:, FC["valid"], 1:] == 0).all()
            assert (want[:, FC["slot"]] == ((95 + np.arange(96)) % 96)[None, :]).all()
            at0 = expected(v, None, 96, at=(np.zeros(n, dtype=np.int64),) + where(v)[1:])
            same(want[:, 2:, 1:], at0[:, 2:, :95], (rng, "the wrapped slots are those of clock 0 on the same days"))
    pv = want[:, FC["pv"]]
    assert (pv > 0).any() and (pv == 0).any() and len(set(where(v)[1])) > 1 and (want[:, FC["wind"]] > 0).any()
    out.free()
    v.close()


@pytest.mark.parametrize("rng", ("philox", "compat"))
def test_blocks_that_straddle_waves_and_workgroups(rng):
    """70 envs x [65, 0] (a station without piles still has its arrival column): blocks of 960 floats (H = 96, 263 workgroups), of 80
    (H = 8: wave boundaries inside blocks), of 3 (H = 3, one field) and of 7 (7 fields, H = 1)"""
    n = 70
    v = made(rng, [65, 0], n)
    out = Out(n * 10 * 96)
    d = Driver(v, rng)
    d.reset()
    for clock in (0, 3):
        while (v.env_clocks() < clock).any():
            d.step()
        want = expected(v, None, 96)
        for fields, H in ((ALL, 96), (ALL, 8), (1 << FC["pv"], 3), (0b1011101101, 1), (0b0101010010, 96)):
            same(out.call(v, fields, H), want[:, cols_of(fields), :H], (rng, clock, fields, H))
    assert (want[:, FC["arrivals1"]] > 0).any()
    out.free()
    v.close()


# ---- 2. per-env clocks
@pytest.mark.parametrize("rng", MODES)
def test_per_env_clocks_after_host_masked_steps(rng):
    """96 host-masked steps leave the six envs at six slots: one at 95, one stepped past `done` without a reset (96 steps: its clock has
    wrapped to 0 and it keeps its days), the others at 1, 5, 17 and 50"""
    n = 6
    target = np.array([95, 96, 1, 5, 17, 50])
    v = made(rng, [3, 2], n)
    out = Out(n * 10 * 96)
    d = Driver(v, rng)
    d.reset()
    days0 = where(v)[1:]
    for j in range(96):
        a, z = d.action()
        v.step_envs(target > j, a, z)
    t, pv, wd = where(v)
    assert list(t) == [95, 0, 1, 5, 17, 50] and v.clock_groups == 6
    assert np.array_equal(pv, days0[0]) and np.array_equal(wd, days0[1])
    for fields, H in ((ALL, 96), (ALL, 8), (1 << FC["valid"] | 1 << FC["wind"], 8)):
        got = out.call(v, fields, H)
        same(got, expected(v, fields, H), (rng, fields, H))
    got = out.call(v, ALL, 8)
    assert list(got[:, FC["slot"], 0]) == [95, 0, 1, 5, 17, 50] and list(got[0, FC["valid"]]) == [1] + [0] * 7 and (got[1:, FC["valid"]] == 1).all()
    same(v.forecast(None, 8), got, (rng, "the host form"))
    out.free()
    v.close()


@pytest.mark.parametrize("rng", ("philox", "philox_curves"))
def test_an_autoreset_step_at_the_days_end_shows_slot_0_and_the_new_days(rng):
    n = 6
    v = made(rng, [3, 2], n)
    out = Out(n * 10 * 96)
    d = Driver(v, rng)
    d.reset()
    for _ in range(90):
        d.step()
    first = np.arange(n) < 3
    for _ in range(5):
        v.step_envs(first, d.action()[0])
    t, pv0, wd0 = where(v)
    assert list(t) == [95, 95, 95, 90, 90, 90]
    same(out.call(v, ALL, 8), expected(v, None, 8), (rng, "before"))
    packed, _ = Dev(v).autoreset(d.action()[0])
    assert list(packed[:, -1] > 0.5) == [True] * 3 + [False] * 3
    t, pv, wd = where(v)
    assert list(t) == [0, 0, 0, 91, 91, 91]
    assert (pv[:3] != pv0[:3]).any() or (wd[:3] != wd0[:3]).any(), "the re-started envs drew new days"
    assert np.array_equal(pv[3:], pv0[3:]) and np.array_equal(wd[3:], wd0[3:])
    got = out.call(v, ALL, 96)
    same(got, expected(v, None, 96), (rng, "after"))
    assert (got[:3, FC["slot"], 0] == 0).all() and (got[:3, FC["valid"]] == 1).all()
    out.free()
    v.close()


# ---- 3. device masks
@pytest.mark.parametrize("rng", ("philox", "compat"))
def test_a_device_mask_writes_only_the_blocks_it_names(rng):
    mg = buffers()
    n = 70
    v = made(rng, [3, 2], n)
    out = Out(n * 10 * 8)
    d = Driver(v, rng)
    d.reset()
    for _ in range(4):
        d.step()
    full = out.call(v, ALL, 8)
    same(full, expected(v, None, 8), rng)
    m = np.zeros(n, dtype=np.uint8)
    m[[0, 3, 64, 69]] = 1
    m[3] = 255  # (any non-zero byte names an env)
    d_mask = mg.DeviceBuffer(n)
    some = 1 << FC["valid"] | 1 << FC["price"] | 1 << FC["fcev"]
    for mask_rows, fields in ((m, ALL), (m, some), (np.zeros(n, dtype=np.uint8), ALL), (np.ones(n, dtype=np.uint8), some)):
        d_mask.from_host(mask_rows)
        got = out.raw(v, fields, 8, d_mask=d_mask.ptr)  # (the guard behind N * C * H words is checked there: a subset writes no further)
        on = mask_rows != 0
        assert np.array_equal(got[on], bits(full[:, cols_of(fields)])[on]), (rng, fields, "named blocks")
        assert (got[~on] == CANARY).all(), (rng, fields, "every other block keeps the pattern")
    d_mask.free()
    out.free()
    v.close()


# ---- 4. per-env rows
@pytest.mark.parametrize("rng", MODES)
def test_per_env_rows_give_every_env_its_own_fcev_column(rng):
    """fcev_permeate per env: the default, three rates in between, 1.0 (the largest rate there is: 0.3 arrivals per index, 90 at index
    300 -- the clamp at 255 is out of reach of any permeate the reference's rule lets through) and 1.5, which the reference reads as 0.01"""
    n = 6
    perm = [0.01, 0.5, 1.0, 1.5, 0.25, 0.9]
    v = made(rng, [3, 2], n, fcev_permeate=perm)
    assert v.has_env_params
    plain = made(rng, [3, 2], n)
    out = Out(n * 10 * 96)
    for h in (v, plain):
        d = Driver(h, rng)
        d.reset()
        for _ in range(3):
            d.step()
    got = out.call(v, ALL, 96)
    same(got, expected(v, None, 96), (rng, "rows"))
    fcev = got[:, FC["fcev"]]
    assert np.array_equal(bits(fcev[3]), bits(fcev[0])) and (fcev[2] > fcev[5]).all() and (fcev[5] > fcev[1]).all() and (fcev[1] > fcev[4]).all()
    assert len(set(fcev[:, 0])) == 5
    ref = out.call(plain, ALL, 96)
    same(ref, expected(plain, None, 96), (rng, "homogeneous"))
    same(got[:, 2:5], ref[:, 2:5], (rng, "sin, cos, price do not depend on the rows"))
    same(got[:, 7:9], ref[:, 7:9], (rng, "nor do the stations' arrivals"))
    same(got[0, FC["fcev"]], ref[0, FC["fcev"]], (rng, "the summed histogram equals the handle's table at the same rate"))
    same(out.call(v, 1 << FC["fcev"], 8), got[:, [FC["fcev"]], :8], (rng, "FCEV alone"))
    # new rates for two envs: the next call follows, without a reset
    v.set_env_params(mask=np.array([1, 0, 1, 0, 0, 0], dtype=bool), fcev_permeate=0.7)
    assert list(v.env_params()["fcev_permeate"]) == [0.7, 0.5, 0.7, 1.5, 0.25, 0.9]
    after = out.call(v, ALL, 96)
    same(after, expected(v, None, 96), (rng, "after chub_set_env_params"))
    same(after[[1, 3, 4, 5]], got[[1, 3, 4, 5]], (rng, "the others keep theirs"))
    assert (after[0, FC["fcev"]] > got[0, FC["fcev"]]).all() and (after[2, FC["fcev"]] < got[2, FC["fcev"]]).all()
    out.free()
    plain.close()
    v.close()


# ---- 5. user-supplied series
def test_columns_follow_the_handles_own_tables(tmp_path):
    from charginghub_env_amd import data_io
    base = fl.data()
    price = base.price[::-1] * 1.25 + 0.01 * np.arange(96)
    pv = base.pv[::-1] * 0.5 + 1.0  # (never negative: every slot reports something)
    rates = 40 + 30 * np.sin(np.arange(96) / 96 * 2 * np.pi)
    dir_ = data_io.write_data_dir(str(tmp_path / "data"), arrival_cdf=data_io.cdf_from_rates(rates), price=price, pv=pv)
    n = 6
    v = made("philox", [3, 2], n, data_dir=dir_)
    out = Out(n * 10 * 96)
    v.reset()
    for _ in range(2):
        v.step(np.zeros((n, v.act_dim), dtype=np.float32))
    got = out.call(v, ALL, 96)
    same(got, expected(v, None, 96, data_dir=dir_), "the handle's tables")
    packaged = expected(v, None, 96)
    for name in ("price", "pv", "arrivals0", "arrivals1"):
        assert not np.array_equal(got[:, FC[name]], packaged[:, FC[name]]), name
    same(got[:, FC["wind"]], packaged[:, FC["wind"]], "the wind series is the packaged one")
    out.free()
    v.close()


# ---- 6. read-only
@pytest.mark.parametrize("rng", MODES)
def test_a_twin_that_never_calls_it_computes_the_same(rng):
    """two handles on one seed, 100 steps through a day's end; one of them calls chub_forecast_device between every pair of steps: the
    step outputs, the ticks and clocks agree, and on the calling handle a run from a snapshot ends in the same snapshot blob with and
    without the calls (blobs of two handles hold their own device addresses)"""
    n = 6
    a, b = made(rng, [3, 2], n, seed=21), made(rng, [3, 2], n, seed=21)
    size = a._lib.chub_state_size(a._h)
    assert size == b._lib.chub_state_size(b._h)
    out = Out(n * 10 * 96)
    da, db = Driver(a, rng), Driver(b, rng)
    oa, ob = da.reset(), db.reset()
    assert np.array_equal(oa, ob)
    start, rs_state = a.get_state(), da.rs.get_state()
    for t in range(100):
        out.call(a, ALL, 96)
        out.call(a, 1 << FC["fcev"], 8)
        ra, rb = da.step(), db.step()
        assert all(np.array_equal(x, y) for x, y in zip(ra[:3], rb[:3])), (rng, "step", t)
    for x, y in zip(a.env_clocks(ticks=True), b.env_clocks(ticks=True)):
        assert np.array_equal(x, y)
    assert np.array_equal(a.telemetry(), b.telemetry(), equal_nan=True) and np.array_equal(a.pile_obs(), b.pile_obs())
    assert a._lib.chub_state_size(a._h) == size == b._lib.chub_state_size(b._h) == a.get_state().size
    blob_with = a.get_state()
    a.set_state(start)
    da.rs.set_state(rs_state)
    for t in range(100):
        da.step()
    assert np.array_equal(blob_with, a.get_state()), (rng, "snapshot blobs")
    same(out.call(a, ALL, 8), expected(a, None, 8), (rng, "after set_state and 100 steps"))
    out.free()
    a.close()
    b.close()


# ---- 7. captured graphs
def test_a_captured_day_fills_a_ring_of_forecasts():
    """PHILOX, captured at clock 95: reset, forecast, 95 x (step, forecast) -- 96 resets + steps, an even number, and the graph ends at
    the clock it started from -- into a [96][N][C][H] ring.  Two replays: block k is the definition at clock k on that replay's days; the
    days change between the replays, the tariff and time columns do not."""
    mg = buffers()
    n, H = 6, 8
    v = made("philox", [3, 2], n, seed=31)
    rs = np.random.RandomState(3)
    v.reset()
    for _ in range(95):
        v.step(rs.uniform(-1, 1, size=(n, v.act_dim)).astype(np.float32))
    st = mg.Stream(0)
    dv = Dev(v, st.ptr)
    block = n * 10 * H
    ring = mg.DeviceBuffer((96 * block + GUARD) * 4)
    ring.from_host(np.full(96 * block + GUARD, CANARY, dtype=np.uint32), st.ptr)
    dv.act.from_host(rs.uniform(-1, 1, size=(n, v.act_dim)).astype(np.float32), st.ptr)
    st.sync()
    v.graph_begin(st.ptr)
    v.reset_device(dv.obs.ptr, stream=st.ptr)
    v.forecast_device(ring.ptr, ALL, H, stream=st.ptr)
    for k in range(1, 96):
        v.step_device_packed(dv.act.ptr, dv.packed.ptr, stream=st.ptr)
        v.forecast_device(ring.ptr + 4 * k * block, ALL, H, stream=st.ptr)
    graph = v.graph_end(st.ptr)
    assert (ring.to_host(np.uint32, (96 * block + GUARD,), st.ptr) == CANARY).all()  # nothing ran while recording
    rings, days = [], []
    for r in range(2):
        v.graph_launch(graph, st.ptr)
        st.sync()
        words = ring.to_host(np.uint32, (96 * block + GUARD,), st.ptr)
        assert (words[96 * block:] == CANARY).all() and not (words[:96 * block] == CANARY).any()
        got = words[:96 * block].view(np.float32).reshape(96, n, 10, H)
        t, pv, wd = where(v)
        assert (t == 95).all()
        for k in range(96):
            same(got[k], expected(v, None, H, at=(np.full(n, k), pv, wd)), ("replay", r, "block", k))
        rings.append(got.copy())
        days.append((pv, wd))
    assert not (np.array_equal(days[0][0], days[1][0]) and np.array_equal(days[0][1], days[1][1])), "a replayed episode draws new days"
    same(rings[0][:, :, :5], rings[1][:, :, :5], "slot, valid, sin, cos, price do not change between replays")
    assert not np.array_equal(rings[0][:, :, 5:7], rings[1][:, :, 5:7])
    v.graph_destroy(graph)
    ring.free()
    v.close()
    st.destroy()


def test_a_capture_on_per_env_clocks_reads_the_clocks_when_it_runs():
    """three envs at clock 95 and three at 94; two auto-reset calls are captured with a forecast behind each.  After the replay the first
    buffer shows the first three at slot 0 on their NEW days and the others at 95 on their old ones, the second buffer everybody one step
    on (the others now re-started too)."""
    mg = buffers()
    n, H = 6, 8
    v = made("philox", [3, 2], n, seed=41)
    rs = np.random.RandomState(4)
    act = lambda: rs.uniform(-1, 1, size=(n, v.act_dim)).astype(np.float32)
    v.reset()
    for _ in range(94):
        v.step(act())
    v.step_envs(np.arange(n) < 3, act())  # (per-env clocks from here on)
    t, pv0, wd0 = where(v)
    assert list(t) == [95] * 3 + [94] * 3
    st = mg.Stream(0)
    dv = Dev(v, st.ptr)
    block = n * 10 * H
    buf = mg.DeviceBuffer((2 * block + GUARD) * 4)
    buf.from_host(np.full(2 * block + GUARD, CANARY, dtype=np.uint32), st.ptr)
    dv.act.from_host(act(), st.ptr)
    st.sync()
    v.graph_begin(st.ptr)
    for k in range(2):
        v.step_autoreset_device(dv.act.ptr, dv.packed.ptr, dv.final.ptr, stream=st.ptr)
        v.forecast_device(buf.ptr + 4 * k * block, ALL, H, stream=st.ptr)
    graph = v.graph_end(st.ptr)
    assert (buf.to_host(np.uint32, (2 * block + GUARD,), st.ptr) == CANARY).all()
    v.graph_launch(graph, st.ptr)
    st.sync()
    words = buf.to_host(np.uint32, (2 * block + GUARD,), st.ptr)
    assert (words[2 * block:] == CANARY).all()
    got = words[:2 * block].view(np.float32).reshape(2, n, 10, H)
    t, pv, wd = where(v)
    assert list(t) == [1] * 3 + [0] * 3
    same(got[1], expected(v, None, H), "behind the second call")
    mid = (np.array([0] * 3 + [95] * 3), np.concatenate([pv[:3], pv0[3:]]), np.concatenate([wd[:3], wd0[3:]]))
    same(got[0], expected(v, None, H, at=mid), "behind the first call")
    assert (pv != pv0).any() or (wd != wd0).any()
    v.graph_destroy(graph)
    buf.free()
    v.close()
    st.destroy()


# ---- 8. the anchor against the simulation
@pytest.mark.parametrize("rng", MODES)
def test_h0_is_the_slot_the_step_has_just_made_the_state_of(rng):
    """after the reset and after every one of 96 steps: SIN[h = 0] is the bits of observation column 0, and on the odd PV days (which
    the reference leaves free of noise, REN:38-43) PV[h = 0] is f32(telemetry RE_PV)"""
    n = 24
    v = made(rng, [3, 2], n)
    out = Out(n * 2 * 1)
    d = Driver(v, rng)
    obs = d.reset()
    fields = 1 << FC["sin"] | 1 << FC["pv"]
    lit = 0
    for k in range(97):
        if k:
            obs = d.step()[0]
        got = out.call(v, fields, 1)
        tel = v.telemetry()
        odd = tel[:, T["pv_day"]].astype(int) % 2 == 1
        assert odd.sum() >= 4
        assert np.array_equal(bits(got[:, 0, 0]), bits(obs[:, 0])), (rng, "sin", k)
        assert np.array_equal(bits(got[odd, 1, 0]), bits(tel[odd, T["re_pv_power"]].astype(np.float32))), (rng, "pv", k)
        lit += int((got[odd, 1, 0] > 0).sum())
    assert lit > 100
    out.free()
    v.close()


# ---- 9. the law of the FCEV count
def test_the_fcev_column_is_the_mean_of_what_the_tail_draws():
    """4096 PHILOX envs at fcev_permeate 0.5.  For each of the first 8 steps the mean over the envs of the step's FCEV arrivals
    (telemetry) lies within 6 sqrt(var_s / 4096) of FCEV[h = 0] before the step, var_s the variance over the 1000 levels of slot s's
    counts -- a bound from the table, not from a run; a slot whose counts are constant must match exactly."""
    n, perm = 4096, 0.5
    counts = fl.fcev_counts(fl.data(), perm)[:8]
    var = counts.var(axis=1)
    assert (var > 0).sum() >= 6, var
    v = made("philox", [3, 2], n, seed=51, fcev_permeate=perm)
    out = Out(n)
    v.reset()
    zero = np.zeros((n, v.act_dim), dtype=np.float32)
    for s in range(8):
        col = out.call(v, 1 << FC["fcev"], 1)[:, 0, 0]
        assert (col == col[0]).all() and bits(col[0]) == bits(fl.mean_by_levels(counts)[s]), s
        v.step(zero)
        mean = v.telemetry()[:, T["fcev_arrive_number"]].mean()
        bound = 6 * np.sqrt(var[s] / n)
        print("slot %d: mean arrivals %.4f, FCEV[h=0] %.4f, bound %.4f" % (s, mean, col[0], bound))
        assert abs(mean - float(col[0])) <= bound, (s, mean, float(col[0]), bound)
    out.free()
    v.close()


# ---- 10. refusals
def test_refusals():
    chub = hub()
    n = 6
    v = made("philox", [3, 2], n)
    v.reset()
    out = Out(n * 10 * 96)
    lib = v._lib
    out.buf.from_host(np.full(out.floats + GUARD, CANARY, dtype=np.uint32))
    for fields, H in ((0, 8), (1 << 10, 8), (ALL | 1 << 10, 8), (ALL, 0), (ALL, 97), (ALL, -1)):
        assert lib.chub_forecast_device(v._h, fields, H, None, out.buf.ptr, None) == -1
    assert lib.chub_forecast_device(v._h, ALL, 8, None, None, None) == -1
    assert lib.chub_forecast_device(None, ALL, 8, None, out.buf.ptr, None) == -1
    host = np.full((n, 10, 8), 7, dtype=np.float32)
    assert lib.chub_forecast(v._h, ALL, 97, host.ctypes.data) == -1 and (host == 7).all()
    v.sync()
    assert (out.buf.to_host(np.uint32, (out.floats + GUARD,)) == CANARY).all(), "nothing was written"
    with pytest.raises(ValueError):
        v.forecast(("pv", "solar"))
    with pytest.raises(chub.ChubError, match="horizon"):
        v.forecast(horizon=97)
    out.call(v)
    v.tape_register_soc(np.array([50.0], dtype=np.float32))  # a tape handle from here on
    assert lib.chub_forecast_device(v._h, ALL, 8, None, out.buf.ptr, None) == -4
    assert "tape handle" in lib.chub_last_error().decode()
    with pytest.raises(chub.ChubError, match="tape handle"):
        v.forecast()
    out.free()
    v.close()


# ---- 11. the torch adapter
TORCH_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["CHUB_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHUB_ROOT"], "tests"))
import torch  # before libchub: both must share one HIP runtime
torch.cuda.set_device(0)
import test_gpu_forecast
test_gpu_forecast.torch_adapter_forecast()
print("TORCH_FORECAST_OK")
"""


def test_torch_adapter():
    """in a child process that imports torch first (as tests/test_gpu_torch_side.py does; nothing of torch is touched in this one)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], env=dict(os.environ, CHUB_ROOT=root), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "TORCH_FORECAST_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def torch_adapter_forecast():
    import inspect

    import torch
    from charginghub_env_amd import vec_env, wrappers
    n = 16
    names = ("valid", "cos", "price", "pv", "wind")
    kw = {k: BASE[k] for k in BASE if k != "station_type_list"}
    for autoreset, control in (("per_env", "station"), (True, "pile"), (False, "pile")):
        env = wrappers.TorchHubVecEnv(n, [3, 2], ["fast", "slow"], seed=13, autoreset=autoreset, control=control,
                                      forecast=dict(fields=("wind", "pv", "price", "cos", "valid"), horizon=8), **kw)
        env.vec.set_telemetry(True)
        assert env.forecast_names == names
        env.reset()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):  # the adapter fills on torch's CURRENT stream
            side.wait_stream(torch.cuda.default_stream())
            p = env.forecast()
            side.synchronize()
        assert tuple(p.shape) == (n, 5, 8) and p.dtype == torch.float32 and p.is_cuda
        same(p.cpu().numpy(), expected(env.vec, names, 8), (autoreset, "after reset(), on a side stream"))
        same(p.cpu().numpy(), env.vec.forecast(names, 8), (autoreset, "VecChargingHub.forecast"))
        torch.cuda.default_stream().wait_stream(side)
        g = torch.Generator(device="cuda").manual_seed(1)
        for t in range(100 if autoreset == "per_env" else 20):
            env.step(torch.rand((n, env.act_dim), device="cuda", generator=g) * 2 - 1)
            q = env.forecast()
            assert q.data_ptr() == p.data_ptr()  # one buffer the adapter owns
            if t % 10 == 9 or t in (94, 95, 96):
                same(q.cpu().numpy(), env.vec.forecast(names, 8), (autoreset, "step", t, "VecChargingHub.forecast"))
                same(q.cpu().numpy(), expected(env.vec, names, 8), (autoreset, "step", t))
        env.close()
    for fn in (wrappers.TorchHubVecEnv.forecast, vec_env.VecChargingHub.forecast_device):  # an enqueue and nothing else
        src = inspect.getsource(fn)
        assert "sync" not in src.split('"""')[-1] and "cpu()" not in src and "to_host" not in src, fn
    default = wrappers.TorchHubVecEnv(8, [3, 2], ["fast", "slow"], seed=1, forecast=dict(), **kw)  # all fields, H = 8
    default.reset()
    assert default.forecast_names == _lib.FC_NAMES and tuple(default.forecast().shape) == (8, 10, 8)
    default.close()
    off = wrappers.TorchHubVecEnv(8, [3, 2], ["fast", "slow"], seed=1)
    with pytest.raises(RuntimeError):
        off.forecast()
    off.close()
