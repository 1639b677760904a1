"""Pins the oracle (oracle/chub_oracle.c) against the REAL reference C++ core compiled from its
own sources (oracle/_ref/libchs_ref.so).  Where that library exists (build() compiles it where the
reference's sources are at hand) every test checks the oracle against it call by call; everywhere, each
test checks a digest of what it saw against the digest of the reference's own outputs recorded in
tests/golden/oracle_vs_ref.json, so no test needs the reference to run.  The recording:
CHUB_RECORD_REF_DIGESTS=tests/golden/oracle_vs_ref.json pytest tests/test_oracle_vs_ref.py, with the library present."""
import hashlib
import json
import os

import numpy as np
import pytest

import orclib
from orclib import FAST, SLOW, orc, ptr

GOLDEN = os.path.join(orclib.GOLDEN_DIR, "oracle_vs_ref.json")
RECORD = os.environ.get("CHUB_RECORD_REF_DIGESTS")
_golden = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
_recorded = {}


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _ref():
    """the reference's core where it was built, else None (the tests then hold the oracle to the recorded digests)"""
    if RECORD:
        assert orclib.ref_available(), "recording the reference's digests needs oracle/_ref/libchs_ref.so"
    return orclib.ref() if orclib.ref_available() else None


class Digest(object):
    """a digest of a sequence of outputs: f32 by their bits, integers as int64, f64 as they are"""

    def __init__(self):
        self.h = hashlib.blake2b(digest_size=16)

    def add(self, x):
        a = np.asarray(x)
        if a.dtype == np.float32:
            a = a.view(np.uint32)
        if a.dtype.kind in "iub":
            a = a.astype(np.int64)
        self.h.update(np.ascontiguousarray(a).tobytes())


def _check(key, digest):
    """the outputs seen (the reference's where it ran, else the oracle's) against the reference's recorded digest"""
    got = digest.h.hexdigest()
    if RECORD:
        _recorded[key] = got
        return
    assert key in _golden, "no recorded digest for %s in %s" % (key, GOLDEN)
    assert got == _golden[key], (key, got, _golden[key])


def _recorded_value(key, value):
    """a small recorded output of the reference itself (not a digest), for the tests that hand state over to it"""
    if RECORD:
        _recorded[key] = value
        return value
    assert key in _golden, "no recorded value for %s in %s" % (key, GOLDEN)
    return _golden[key]


@pytest.fixture(scope="module", autouse=True)
def _write_recording():
    yield
    if RECORD:
        old = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
        old.update(_recorded)
        with open(RECORD, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
            f.write("\n")


def test_csv_parser_and_table_bit_exact():
    r = _ref()
    t = orclib.tables()
    got = np.array([[orc.orc_tables_cdf(t, i, j) for j in range(301)] for i in range(96)], dtype=np.float32)
    rec = Digest()
    if r is not None:
        want = np.array([[r.ref_cdf(i, j) for j in range(301)] for i in range(96)])
        assert all(r.ref_cdf_cols(i) == 301 for i in range(96))
        assert np.array_equal(got.astype(np.float64), want)  # reference stores the f32 parse widened
    rec.add(want if r is not None else got.astype(np.float64))
    for s in [b"0.0001", b"0.00011881552713086621", b"1", b"0.9999999999", b"12.5", b"3", b"0.1"]:
        g = bits(orc.orc_parse_float(s, len(s)))
        if r is not None:
            assert g == bits(r.ref_parse_float(s))
        rec.add(bits(r.ref_parse_float(s)) if r is not None else g)
    _check("csv_parser_and_table", rec)


def test_glibc_and_minstd_streams():
    r = _ref()
    g = orc.orc_rng_alloc()
    rec = Digest()
    for seed in (1, 2, 12345, 0xFFFFFFFF):
        orc.orc_rng_seed_compat(g, seed, seed)
        b = [orc.orc_glibc_rand(g) for _ in range(3000)]
        if r is not None:
            r.ref_seed(seed, seed)
            a = [r.ref_c_rand() for _ in range(3000)]
            assert a == b
        rec.add(a if r is not None else b)
        b = [orc.orc_minstd_next(g) for _ in range(3000)]
        if r is not None:
            a = [r.ref_minstd_next() for _ in range(3000)]
            assert a == b
        rec.add(a if r is not None else b)
    orc.orc_rng_free(g)
    _check("glibc_and_minstd_streams", rec)


def test_variates_match_reference_in_mixed_order():
    r = _ref()
    g = orc.orc_rng_alloc()
    if r is not None:
        r.ref_seed(7, 9)
    orc.orc_rng_seed_compat(g, 7, 9)
    rs = np.random.RandomState(0)
    rec = Digest()
    for it in range(20000):
        op = rs.randint(0, 5)
        if op == 0:
            got, want = bits(orc.orc_mk_soc(g)), (lambda: bits(r.ref_mk_soc()))
        elif op == 1:
            got, want = orc.orc_mk_late_time(g), (lambda: r.ref_mk_late_time(0))
        elif op == 2:
            mu = int(rs.randint(0, 40))
            got, want = orc.orc_init_station_car_number(g, orclib.tables(), 0, mu), (lambda: r.ref_init_station_car_number(mu))
        elif op == 3:
            k = orc.orc_draw_k(g, 1, 0, 0)
            got, want = bits(orc.orc_uniform_level(k, 80, 100)), (lambda: bits(r.ref_uniform_rand(80, 100)))
        else:
            k = orc.orc_draw_k(g, 1, 0, 0)
            got, want = bits(orc.orc_uniform_level(k, 0, 1)), (lambda: bits(r.ref_uniform_rand(0, 1)))
        if r is not None:
            want = want()
            assert want == got
            got = want
        rec.add(got)
    orc.orc_rng_free(g)
    _check("variates_in_mixed_order", rec)


def test_rng_state_transplant_roundtrip():
    """oracle <-> reference stream hand-over (used to multiplex envs through the one global stream)."""
    r = _ref()
    g = orc.orc_rng_alloc()
    orc.orc_rng_seed_compat(g, 99, 5)
    for _ in range(17):
        orc.orc_glibc_rand(g)
    buf = np.zeros(132 + 8, dtype=np.uint8)
    orc.orc_rng_export_glibc128(g, ptr(buf))
    live_rand = live_minstd = live_next = live_saved = None
    if r is not None:
        r.ref_rng_load(ptr(buf))
        live_rand, live_minstd = [r.ref_c_rand() for _ in range(100)], [r.ref_minstd_next() for _ in range(10)]
    # what the reference draws from the oracle's exported state
    a_rand = _recorded_value("transplant.ref_c_rand_after_load", live_rand)
    a_minstd = _recorded_value("transplant.ref_minstd_after_load", live_minstd)
    assert live_rand in (None, a_rand) and live_minstd in (None, a_minstd)
    assert a_rand == [orc.orc_glibc_rand(g) for _ in range(100)]
    assert a_minstd == [orc.orc_minstd_next(g) for _ in range(10)]
    if r is not None:
        buf2 = np.zeros(132 + 8, dtype=np.uint8)
        r.ref_rng_save(ptr(buf2))
        live_saved, live_next = buf2.tobytes().hex(), [r.ref_c_rand() for _ in range(100)]
    # the reference's saved state, and what it draws next from it
    saved = _recorded_value("transplant.ref_saved_state_hex", live_saved)
    a_next = _recorded_value("transplant.ref_c_rand_after_save", live_next)
    assert live_saved in (None, saved) and live_next in (None, a_next)
    buf2 = np.frombuffer(bytes.fromhex(saved), dtype=np.uint8).copy()
    g2 = orc.orc_rng_alloc()
    orc.orc_rng_import_glibc128(g2, ptr(buf2))
    assert a_next == [orc.orc_glibc_rand(g2) for _ in range(100)]
    orc.orc_rng_free(g)
    orc.orc_rng_free(g2)


def test_arrival_lookup_all_cells():
    r = _ref()
    t = orclib.tables()
    # every (time, level): replay the reference with a forced rand() level by brute force over the stream
    # -> instead compare through the uniform level directly: n(t,k) only depends on k = rand()%1000
    g = orc.orc_rng_alloc()
    if r is not None:
        r.ref_seed(3, 3)
    orc.orc_rng_seed_compat(g, 3, 3)
    rec = Digest()
    for it in range(30000):
        tt = it % 96
        k = orc.orc_draw_k(g, 1, 0, 0)
        n = orc.orc_arrival_index(t, tt, k)
        which = it % 4
        if which == 0:
            got, want = n, (lambda: r.ref_give_car_number(tt))
        elif which == 1:
            got, want = orc.orc_count_fast(n), (lambda: r.ref_ev_fast(tt))
        elif which == 2:
            got, want = orc.orc_count_slow(n), (lambda: r.ref_ev_slow(tt))
        else:
            got, want = orc.orc_count_hv(n, 0.3, 0.05), (lambda: r.ref_hv(tt, 0.3, 0.05))
        if r is not None:
            want = want()
            assert want == got
            got = want
        rec.add(got)
    orc.orc_rng_free(g)
    _check("arrival_lookup_all_cells", rec)


@pytest.mark.parametrize("cp", [0, 1])
def test_curves_bit_exact_on_grids(cp):
    r = _ref()
    tgrid = np.arange(-1.0, 16.0, 0.003, dtype=np.float64).astype(np.float32)
    sgrid = np.arange(-5.0, 105.0, 0.01, dtype=np.float64).astype(np.float32)
    rs = np.random.RandomState(1)
    tgrid = np.concatenate([tgrid, rs.uniform(-1, 16, 20000).astype(np.float32)])
    sgrid = np.concatenate([sgrid, rs.uniform(-5, 105, 20000).astype(np.float32)])
    rec = Digest()
    for which, grid in ((0, tgrid), (1, tgrid), (2, sgrid)):
        for name in ("slow", "fast"):
            fo = getattr(orc, "orc_curve_" + name)
            got = np.array([fo(which, float(x), cp) for x in grid], dtype=np.float32)
            if r is not None:
                fr = getattr(r, "ref_curve_" + name)
                want = np.array([fr(which, float(x), cp) for x in grid], dtype=np.float32)
                bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
                assert bad.size == 0, (name, which, grid[bad[:5]], got[bad[:5]], want[bad[:5]])
                got = want
            rec.add(got)
    _check("curves_on_grids[%d]" % cp, rec)


def _action_program(kind, step, n, rs):
    if kind == "ones":
        return np.ones(n, dtype=np.float32)
    if kind == "zeros":
        return np.zeros(n, dtype=np.float32)
    return (rs.rand(n) < 0.5).astype(np.float32)


def _same_station(a, b, rec, *where):
    """the oracle station b against the reference's a (where it runs); what was seen goes into the digest"""
    sb, cb = b.slots(), b.scalars()
    if a is not None:
        sa, ca = a.slots(), a.scalars()
        assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32)), where
        assert np.array_equal(ca, cb), where + (ca, cb)
        sb, cb = sa, ca
    rec.add(sb)
    rec.add(cb)


@pytest.mark.parametrize("typ,piles", [(FAST, 16), (SLOW, 16), (FAST, 20), (SLOW, 25), (FAST, 32), (SLOW, 32),
                                       (FAST, 1), (SLOW, 3), (FAST, 0), (SLOW, 64),
                                       (FAST, 100), (SLOW, 170), (FAST, 256)])  # the reference takes any size (CHS.hpp:1148, 1458)
@pytest.mark.parametrize("kind", ["ones", "zeros", "random"])
def test_station_trajectories(typ, piles, kind):
    r = _ref()
    rs = np.random.RandomState(piles * 7 + typ)
    seed_g, seed_m = 1000 + piles, 2000 + typ
    a = None
    if r is not None:
        r.ref_seed(seed_g, seed_m)
        a = orclib.RefStation(typ, piles)   # constructor runs one evs_reset (consumes draws)
    b = orclib.OrcStation(typ, piles)
    b.seed_compat(seed_g, seed_m)
    b.reset()                               # mirror the constructor's evs_reset
    rec = Digest()
    for ep in range(3):
        if a is not None:
            a.reset()
        b.reset()
        _same_station(a, b, rec, ep)
        for step in range(96):
            act = _action_program(kind, step, piles, rs)
            if a is not None:
                a.step(act)
            b.step(act)
            _same_station(a, b, rec, ep, step)
    _check("station_trajectories[%d-%d-%s]" % (typ, piles, kind), rec)


@pytest.mark.parametrize("typ,piles,kind", [(FAST, 300, "random"), (SLOW, 1000, "random"), (SLOW, 1500, "zeros"), (FAST, 4096, "ones")])
def test_station_trajectories_beyond_256_piles(typ, piles, kind):
    """Round 6: liboracle_big.so (the same source, ORC_MAX_PILES = 4096) against the reference on stations of more than 256 piles
    -- evs_reset then admits more cars than the balk test's exp(-0.01 (line + j)) leaves any level but 0 (j > 690)."""
    with orclib.big_oracle():
        test_station_trajectories(typ, piles, kind)


@pytest.mark.parametrize("typ,piles,cc", [(FAST, 300, False), (SLOW, 700, True), (FAST, 1100, False)])
def test_station_scalar_load_mode_beyond_256_piles(typ, piles, cc):
    with orclib.big_oracle():
        test_station_scalar_load_mode(typ, piles, cc)


@pytest.mark.parametrize("typ,piles", [(FAST, 20), (SLOW, 25), (FAST, 100), (SLOW, 170)])
@pytest.mark.parametrize("cc", [False, True])
def test_station_scalar_load_mode(typ, piles, cc):
    """evs_step(float): the other operator of the boundary."""
    r = _ref()
    rs = np.random.RandomState(5)
    a = None
    if r is not None:
        r.ref_seed(11, 12)
        a = orclib.RefStation(typ, piles, True, cc)
    b = orclib.OrcStation(typ, piles, True, cc)
    b.seed_compat(11, 12)
    b.reset()
    rec = Digest()
    for step in range(200):
        load = float(np.float32(rs.uniform(0, (a if a is not None else b).scalars()[2] * 1.2 + 1)))
        if a is not None:
            a.step_load(load)
        b.step_load(load)
        _same_station(a, b, rec, step)
    _check("station_scalar_load_mode[%d-%d-%d]" % (typ, piles, int(cc)), rec)


def test_constant_charging_vector_mode():
    r = _ref()
    rs = np.random.RandomState(6)
    rec = Digest()
    for typ, piles in ((FAST, 20), (SLOW, 25)):
        a = None
        if r is not None:
            r.ref_seed(21, 22)
            a = orclib.RefStation(typ, piles, True, True)
        b = orclib.OrcStation(typ, piles, True, True)
        b.seed_compat(21, 22)
        b.reset()
        for step in range(192):
            act = (rs.rand(piles) < 0.6).astype(np.float32)
            if a is not None:
                a.step(act)
            b.step(act)
            _same_station(a, b, rec, step)
    _check("constant_charging_vector_mode", rec)
