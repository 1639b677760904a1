"""chub_copy_envs / chub_copy_envs_device: env j becomes a clone of env i, by index, on the device.

The oracle is the specification.  Its envs are plain data, so a clone there is a memmove of one orc_env over another; in the Philox modes
the clone is then given its OWN stream identity again (the destination handle's seed, its own global env id) and, before every call, the
tick the library reports for that env -- exactly how tests/test_gpu_env_clocks.py drives the oracle for masked calls.  In COMPAT the
streams are state and the memmove alone is the clone.  Bars as in _philox_parity / Pair: the nine slot fields and the station records bit
for bit, done exact, f64 observation and reward to TIGHT, orc_vec_overflow == 0."""
import ctypes as C

import numpy as np
import pytest

import orclib
from orclib import orc, ptr
from test_gpu_parity import ORACLE_RNG, TIGHT, check_slots, close, hub

pytestmark = pytest.mark.gpu

orc.orc_sizeof_env.restype = C.c_long
orc.orc_sizeof_env.argtypes = []

KW = dict(station_list=[20, 25], station_type_list=["fast", "slow"], hydro_prod_rate=100.0, hydro_store_vlt=25.0,
          init_soc=0.2, fc_max_power=100.0, fcev_permeate=0.01, constant_charging=False, renew_fluctuate=0.3,
          price_fluctuate=0.3, hydro_loss=0.001)
FIELDS = ("hydro_prod_rate", "hydro_store_vlt", "init_soc", "fc_max_power", "fcev_permeate", "renew_fluctuate", "price_fluctuate", "hydro_loss")


def orc_cfg(kw):
    return orclib.make_config(piles=kw["station_list"], types=kw["station_type_list"],
                              **{k: kw[k] for k in kw if k not in ("station_list", "station_type_list")})


def digest(v):
    """everything the introspection shows of a handle's state"""
    parts = [x.copy() for x in v.slots()] + [v.station_scalars(), v.env_clocks()]
    if v.rng_mode == 0:
        parts.append(v.compat_state())
    return parts


def same(a, b, what, rows=None):
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = (x, y) if rows is None else (x[rows], y[rows])
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (what, k)


class Mirror(object):
    """one library handle (Philox modes) and one oracle env per library env, driven with the same calls; kws: one kwargs dict per env
    (a handle with per-env hub parameters) or None (a homogeneous handle built from kw)"""

    def __init__(self, kw, n, rng="philox", seed=0xFEED5EED, env_id0=4000, kws=None, rs_seed=11, **opts):
        chub = hub()
        self.n, self.kw, self.rng, self.seed, self.env_id0 = n, kw, rng, seed, env_id0
        if kws is None:
            self.v = chub.VecChargingHub(n, seed=seed, rng=rng, env_id0=env_id0, **opts, **kw)
            kws = [kw] * n
        else:
            rows = {f: [k[f] for k in kws] for f in FIELDS}
            self.v = chub.VecChargingHub(n, seed=seed, rng=rng, env_id0=env_id0, **opts,
                                         **dict({k: kw[k] for k in kw if k not in FIELDS}, **rows))
        self.v.set_telemetry(True)
        self.cfgs = [orc_cfg(k) for k in kws]  # (kept alive: the oracle env points at its config)
        self.h = [orc.orc_vec_create(C.byref(c), orclib.tables(), 1, env_id0 + i, ORACLE_RNG[rng], seed) for i, c in enumerate(self.cfgs)]
        self.envs = [orc.orc_vec_env(h, 0) for h in self.h]
        self.D, self.A = self.v.obs_dim, self.v.act_dim
        self.o_obs = np.zeros((n, self.D))
        self.o_rew = np.zeros(n)
        self.o_done = np.zeros(n, dtype=np.int32)
        self.t = np.zeros(n, dtype=np.int64)
        self.rs = np.random.RandomState(rs_seed)

    def _tick(self, e, tick):
        orc.orc_rng_set_tick(orc.orc_env_rng(self.envs[e]), int(tick) - 1)  # the oracle counts up at the start of a call

    def compare(self, rows, label, with_reward=True):
        S0, S1 = self.kw["station_list"]
        sl, sc, g64 = self.v.slots(), self.v.station_scalars(), self.v.obs_f64()
        for e in rows:
            for k, nk in ((0, S0), (1, S1)):
                want = np.zeros((9, nk), dtype=np.float32)
                orc.orc_station_slots(orc.orc_env_station(self.envs[e], k), ptr(want))
                check_slots(sl[k][e], want, (label, e, k))
                ws = np.zeros(8)
                orc.orc_station_scalars(orc.orc_env_station(self.envs[e], k), ptr(ws))
                assert np.array_equal(sc[e, k, :6], ws[:6]), (label, e, k, sc[e, k], ws)
        close(g64[rows], self.o_obs[rows], (label, "obs"), rtol=TIGHT, atol=TIGHT)
        if with_reward:
            close(self.v.reward_f64()[rows], self.o_rew[rows], (label, "reward"), rtol=TIGHT, atol=TIGHT)

    def compare_state(self, rows, label):
        """slots and station records only (what a copy moves; the telemetry block of the last step is left alone)"""
        S0, S1 = self.kw["station_list"]
        sl, sc = self.v.slots(), self.v.station_scalars()
        for e in rows:
            for k, nk in ((0, S0), (1, S1)):
                want = np.zeros((9, nk), dtype=np.float32)
                orc.orc_station_slots(orc.orc_env_station(self.envs[e], k), ptr(want))
                check_slots(sl[k][e], want, (label, e, k))
                ws = np.zeros(8)
                orc.orc_station_scalars(orc.orc_env_station(self.envs[e], k), ptr(ws))
                assert np.array_equal(sc[e, k, :6], ws[:6]), (label, e, k)

    def reset(self, mask=None, label=""):
        rows = np.arange(self.n) if mask is None else np.nonzero(mask)[0]
        obs = self.v.reset() if mask is None else self.v.reset_envs(mask)
        t, ticks = self.v.env_clocks(ticks=True)
        for e in rows:
            self._tick(e, ticks[e])
            orc.orc_env_reset(self.envs[e], None, None, ptr(self.o_obs[e]))
        self.t[rows] = 0
        assert np.array_equal(t, self.t), (label, t, self.t)
        self.compare(rows, ("reset", label), False)
        close(obs[rows], self.o_obs[rows], (label, "reset obs f32"), atol=1e-6)

    def step(self, mask=None, label="", tick_of=None):
        rows = np.arange(self.n) if mask is None else np.nonzero(mask)[0]
        S = sum(self.kw["station_list"])
        act = self.rs.uniform(-1, 1, size=(self.n, self.A)).astype(np.float32)
        if self.rs.randint(5) == 0:
            act[:, :S] = 1.0
        obs, rew, done, _ = self.v.step(act) if mask is None else self.v.step_envs(mask, act)
        t, ticks = self.v.env_clocks(ticks=True)
        for e in rows:
            self._tick(e, ticks[e])
            d, r = C.c_int(0), C.c_double(0.0)
            orc.orc_env_step(self.envs[e], ptr(act[e]), None, ptr(self.o_obs[e]), C.byref(r), C.byref(d))
            self.o_rew[e], self.o_done[e] = r.value, d.value
        self.t[rows] = (self.t[rows] + 1) % 96
        assert np.array_equal(t, self.t), (label, t, self.t)
        assert np.array_equal(done[rows], self.o_done[rows].astype(bool)), (label, "done", done[rows], self.o_done[rows])
        self.compare(rows, ("step", label), True)
        close(obs[rows], self.o_obs[rows], (label, "obs f32"), atol=1e-6)
        return done

    def copy_from(self, src, src_idx, dst_idx):
        """the library's copy and its mirror on the oracle: memmove, then the destination's own stream identity"""
        self.v.copy_envs(src_idx, dst_idx, source=None if src is self else src.v)
        reseed = orc.orc_rng_seed_philox_curves if self.rng == "philox_curves" else orc.orc_rng_seed_philox
        for s, d in zip(src_idx, dst_idx):
            C.memmove(self.envs[d], src.envs[s], orc.orc_sizeof_env())
            reseed(orc.orc_env_rng(self.envs[d]), self.seed, self.env_id0 + int(d))
            self.o_obs[d], self.o_rew[d], self.o_done[d], self.t[d] = src.o_obs[s], src.o_rew[s], src.o_done[s], src.t[s]

    def overflow(self):
        return max(orc.orc_vec_overflow(h) for h in self.h)

    def close(self):
        for h in self.h:
            orc.orc_vec_destroy(h)
        self.v.close()


# ---- 1. the clone is exact -------------------------------------------------------------------------------------------------------

SHAPES = {"c3": [20, 25], "tiny": [1, 2], "one_station": [0, 9], "wide": [64, 40], "big": [300, 20]}
CLONE_CASES = [(rng, s) for rng in ("philox", "philox_curves", "compat") for s in sorted(SHAPES) if not (rng == "philox_curves" and s == "big")]


def _drive(v, rs, n, k, compat):
    for _ in range(k):
        a = rs.uniform(-1, 1, size=(n, v.act_dim)).astype(np.float32)
        v.step(a, rs.normal(size=(n, 3)) if compat else None)


@pytest.mark.parametrize("rng,shape", CLONE_CASES, ids=["%s-%s" % c for c in CLONE_CASES])
def test_clone_is_exact(rng, shape):
    chub = hub()
    n, compat = 40, rng == "compat"
    kw = dict(KW, station_list=SHAPES[shape], fcev_permeate=0.05)
    vs = [chub.VecChargingHub(n, seed=77, rng=rng, env_id0=10, **kw) for _ in range(2)]
    src, dst = np.array([3, 3, 17, 39, 8]), np.array([0, 21, 4, 5, 38])
    for v in vs:
        rs = np.random.RandomState(5)
        if compat:
            v.compat_replay_constructor()
            v.reset(np.stack([rs.randint(0, 100, n), rs.randint(0, 150, n)], axis=1).astype(np.int32), rs.normal(size=(n, 3)))
        else:
            v.reset()
        _drive(v, rs, n, 37, compat)
    before = digest(vs[0])
    same(before, digest(vs[1]), "twins before the copy")
    assert any(not np.array_equal(x[src], x[dst]) for x in before[:2]), "sources and destinations hold the same state already"
    tabs = [vs[0].hy_table(env=int(s)) for s in src]
    vs[0].copy_envs(src, dst)
    after = digest(vs[0])
    for k, x in enumerate(after):
        assert np.array_equal(x[dst].view(np.uint8), x[src].view(np.uint8)), ("destination differs from its source", k)
    others = np.setdiff1d(np.arange(n), dst)
    same(after, before, "an env that was no destination changed", rows=others)
    assert vs[0].clock_groups == 1 and np.array_equal(vs[0].env_clocks(), np.full(n, 37))
    for s, d, tab in zip(src, dst, tabs):
        assert np.array_equal(vs[0].hy_table(env=int(d)), tab)
    # ... and the run goes on: the envs that were no destination agree with the twin that never copied
    outs = []
    for v in vs:
        rs = np.random.RandomState(6)
        a = rs.uniform(-1, 1, size=(n, v.act_dim)).astype(np.float32)
        outs.append(v.step(a, rs.normal(size=(n, 3)) if compat else None)[:3])
    for x, y in zip(*outs):
        assert np.array_equal(np.asarray(x)[others], np.asarray(y)[others])
    same(digest(vs[0]), digest(vs[1]), "after one more step", rows=others)
    for v in vs:
        v.close()


# ---- 2. the future matches the oracle ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rng", ["philox", "philox_curves"])
def test_future_of_clones_matches_the_oracle(rng):
    n = 20
    p = Mirror(KW, n, rng=rng)
    q = Mirror(KW, 12, rng=rng, seed=0xABCDEF12345, env_id0=90000, rs_seed=3)  # the scratch handle: another seed, other env ids
    p.reset(label="all")
    q.reset(label="scratch")
    for i in range(30):
        p.step(label=("before", i))
        q.step(label=("scratch before", i))
    p.copy_from(p, [2, 2, 2, 9], [5, 11, 19, 0])        # fan-out 1 -> 3 within the handle
    q.copy_from(p, [2, 7, 7, 13], [1, 4, 6, 11])        # ... and across handles
    p.compare_state(range(n), "after the copy")
    q.compare_state(range(12), "scratch after the copy")
    assert p.v.clock_groups == 1 and q.v.clock_groups == 1
    for i in range(120):
        for m, name in ((p, "main"), (q, "scratch")):
            if i == 50:
                m.reset(label=(name, "reset"))
            d = m.step(label=(name, "after", i))
            if d.any():
                m.reset(d, (name, "reset at done", i))
    assert p.overflow() == 0 and q.overflow() == 0
    # clones part from their source: their own counters
    sl = p.v.slots()[1]
    assert not np.array_equal(sl[5], sl[11])
    p.close()
    q.close()


class CompatMirror(object):
    """a COMPAT handle and one oracle env per library env (its own constructor seeds), same calls, every env compared after every call.
    Ties: a clone that is given its source's inputs (actions, exo_z, a reset's days) must stay bit-identical to it.  `tie` pairs (s, d) lie
    within this handle; `borrow` pairs (s, d) tie env d of this handle to env s of `other`, the record of another handle's call."""

    def __init__(self, kw, n, rs_seed=21, **opts):
        chub = hub()
        self.n, self.kw = n, kw
        self.rs = np.random.RandomState(rs_seed)
        self.v = chub.VecChargingHub(n, rng="compat", **opts, **kw)
        self.v.set_telemetry(True)
        seeds = np.stack([self.rs.randint(1, 2**31 - 1, n), self.rs.randint(1, 2**31 - 1, n)], axis=1).astype(np.uint32)
        self.v.set_compat_seeds(seeds)
        self.v.compat_replay_constructor()
        self.cfg = orc_cfg(kw)
        self.o = [orclib.OrcEnv(self.cfg, ctor_seeds=(int(a), int(b))) for a, b in seeds]
        self.o_obs, self.o_rew = np.zeros((n, self.v.obs_dim)), np.zeros(n)

    def compare(self, label, with_reward=True, with_obs=True):
        sl, sc = self.v.slots(), self.v.station_scalars()
        for e, o in enumerate(self.o):
            for k in (0, 1):
                check_slots(sl[k][e], o.station_slots(k), (label, e, k))
                assert np.array_equal(sc[e, k, :6], o.station_scalars(k)[:6]), (label, e, k)
        if not with_obs:  # (obs64 / reward64 are the last step's telemetry: a copy leaves them alone)
            return
        close(self.v.obs_f64(), self.o_obs, (label, "obs"), rtol=TIGHT, atol=TIGHT)
        if with_reward:
            close(self.v.reward_f64(), self.o_rew, (label, "reward"), rtol=TIGHT, atol=TIGHT)

    @staticmethod
    def _tied(arrays, tie, borrow, other):
        for s, d in tie:
            for x in arrays:
                x[d] = x[s]
        for s, d in borrow:
            for x, y in zip(arrays, other["in"]):
                x[d] = y[s]

    @staticmethod
    def _identical(outs, tie, borrow, other, label):
        for pairs, theirs in ((tie, outs), (borrow, other["out"] if other else None)):
            for s, d in pairs:
                for x, y in zip(outs, theirs):
                    assert np.asarray(x[d]).tobytes() == np.asarray(y[s]).tobytes(), (label, "a clone left its source", s, d)

    def reset(self, label, tie=(), borrow=(), other=None):
        n = self.n
        days = np.stack([self.rs.randint(0, 100, n), self.rs.randint(0, 150, n)], axis=1).astype(np.int32)
        z = self.rs.normal(size=(n, 3))
        self._tied((days, z), tie, borrow, other)
        obs = self.v.reset(days, z)
        for e, o in enumerate(self.o):
            self.o_obs[e] = o.reset(days[e], z[e])
        self.compare(label, False)
        self._identical((obs,), tie, borrow, other, label)
        return {"in": (days, z), "out": (obs,)}

    def step(self, label, tie=(), borrow=(), other=None):
        n = self.n
        act = self.rs.uniform(-1, 1, size=(n, self.v.act_dim)).astype(np.float32)
        z = self.rs.normal(size=(n, 3))
        self._tied((act, z), tie, borrow, other)
        obs, rew, done, _ = self.v.step(act, z)
        for e, o in enumerate(self.o):
            self.o_obs[e], self.o_rew[e], dn = o.step(act[e], z[e])
            assert bool(done[e]) == dn, (label, e)
        self.compare(label)
        self._identical((obs, rew, done), tie, borrow, other, label)
        return {"in": (act, z), "out": (obs, rew, done)}

    def copy_from(self, src, src_idx, dst_idx):
        self.v.copy_envs(src_idx, dst_idx, source=None if src is self else src.v)
        for s, d in zip(src_idx, dst_idx):
            C.memmove(self.o[d].e, src.o[s].e, orc.orc_sizeof_env())  # the streams are state: the memmove is the clone
            self.o_obs[d], self.o_rew[d] = src.o_obs[s], src.o_rew[s]


def _differing(sc_src, sc_dst, sources, taken=()):
    """for each source env a destination whose stations hold other numbers of cars (so other counts of empty slots) or other queues"""
    pairs, used = [], set(taken)
    for s in sources:
        for d in range(len(sc_dst)):
            differs = (sc_dst[d, :, 3] != sc_src[s, :, 3]).all() or (sc_dst[d, :, 4] != sc_src[s, :, 4]).any()
            if d not in used and d not in sources and differs:
                pairs.append((s, d))
                used.add(d)
                break
    return pairs


@pytest.mark.parametrize("form,n", [("auto", 24), ("wave", 24), ("auto", 300), ("own_walks", 300)])
def test_future_of_compat_clones_matches_the_oracle_and_their_sources(form, n):
    """COMPAT: both launch forms, and a batch large enough for the split step with its walks ahead (one and two steps ahead of the slots).
    Within a handle (fan-out 1 -> 3) and across two handles that have committed different numbers of walks, so that their committed streams
    sit in different buffers of the rotation (rng_cur); the scratch handle is on the same slot of day, so both stay in lock-step and go on
    walking ahead.  Sources and destinations differ in cars held (the empty-slot counts a walk ahead has used) or in queues: asserted.
    120 steps with a reset; every clone gets its source's actions, exo_z and days throughout and stays bit-identical to it."""
    opts = dict(slot_kernel="packed", walk_ahead="off") if form == "own_walks" else dict(slot_kernel=form)
    kw = dict(KW, fcev_permeate=0.02)
    nq = 40 if n > 24 else 16
    m, q = CompatMirror(kw, n, **opts), CompatMirror(kw, nq, rs_seed=5, **opts)
    m.reset("first")
    q.reset("scratch first")
    for i in range(4):
        q.step(("scratch, a first day cut short", i))
    q.reset("scratch second")  # five launches more than the main handle: another buffer of the rotation
    for i in range(25):
        m.step(("before", i))
        q.step(("scratch before", i))
    sc_m, sc_q = m.v.station_scalars(), q.v.station_scalars()
    fan = _differing(sc_m, sc_m, [2, 2, 2, 9])
    across = _differing(sc_m, sc_q, [2, 7, 7, 13])
    assert len(fan) == 4 and len(across) == 4, (fan, across)
    m.copy_from(m, [s for s, _ in fan], [d for _, d in fan])
    q.copy_from(m, [s for s, _ in across], [d for _, d in across])
    m.compare("after the copy", with_obs=False)
    q.compare("scratch after the copy", with_obs=False)
    assert m.v.clock_groups == 1 and q.v.clock_groups == 1 and m.v.clock == q.v.clock == 25
    sm, sq = m.v.compat_state(), q.v.compat_state()
    for s, d in fan:
        assert np.array_equal(sm[s], sm[d])
    for s, d in across:
        assert np.array_equal(sm[s], sq[d])
    for i in range(120):
        if i == 60:
            rec = m.reset("in between", tie=fan)
            q.reset("scratch in between", borrow=across, other=rec)
        rec = m.step(("after", i), tie=fan)
        q.step(("scratch after", i), borrow=across, other=rec)
    assert all(o.q_overflow() == 0 for o in m.o + q.o)
    m.v.close()
    q.v.close()


# ---- 3. draws made one launch ahead are not reused ----------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["packed_two_launches", "one_launch", "wave"])
def test_the_step_after_a_copy_admits_against_the_new_queue(form):
    """pk (the station draws of the next step, decoded one launch ahead against the queue the last step left) belongs to the destination's
    OLD queue: a copy between envs whose queues differ must be followed by a step that decodes afresh"""
    opts = {"packed_two_launches": dict(slot_kernel="packed", fused_step="off"), "one_launch": dict(slot_kernel="packed", fused_step="on"),
            "wave": dict(slot_kernel="wave")}[form]
    n = 64
    kw = dict(KW, station_list=[3, 5])  # small stations: cars queue
    p = Mirror(kw, n, **opts)
    assert p.v.uses_fused_step == (form == "one_launch") and p.v.uses_packed_kernel == (form != "wave")
    p.reset(label="all")
    src, dst = [], []
    for i in range(70):
        p.step(label=("before", i))
        line = p.v.station_scalars()[:, :, 4]
        src, dst = [], []
        for d in range(n):  # pair envs whose queues differ
            cand = [s for s in range(n) if s != d and s not in dst and s not in src and d not in src and (line[s] != line[d]).any()]
            if cand and len(src) < 12:
                src.append(cand[0])
                dst.append(d)
        if i >= 20 and len(dst) >= 6:
            break
    assert len(dst) >= 6 and all((line[s] != line[d]).any() for s, d in zip(src, dst)), (line, src, dst)
    assert not set(src) & set(dst)
    p.copy_from(p, src, dst)
    assert p.v.clock_groups == 1 and p.v.uses_fused_step == (form == "one_launch")
    for i in range(3):
        p.step(label=("the very next steps", i))
    assert p.overflow() == 0
    p.close()


# ---- 4. different clocks -----------------------------------------------------------------------------------------------------------

def test_a_copy_brings_the_sources_clock_along():
    n = 16
    p = Mirror(KW, n)
    late = np.arange(n) >= n // 2
    p.reset(label="all")
    for i in range(33):
        p.step(label=("head start", i))
    p.reset(late, "second half starts again")
    for i in range(7):
        p.step(label=("both", i))
    assert p.v.clock_groups == 2 and p.t[0] == 40 and p.t[-1] == 7
    p.copy_from(p, [0, 1, 12], [9, 15, 3])  # slot 40 over slot 7 (twice), slot 7 over slot 40
    want = np.where(late, 7, 40)
    want[[9, 15]], want[3] = 40, 7
    assert np.array_equal(p.v.env_clocks(), want) and p.v.clock_groups == 2
    p.compare_state(range(n), "after the copy")
    ends = {}
    for i in range(100):
        d = p.step(label=("run", i))
        if d.any():
            assert np.array_equal(d, p.t == 0)
            for e in np.nonzero(d)[0]:
                ends[int(e)] = i
            p.reset(d, ("reset at done", i))
    assert all(ends[e] == (55 if want[e] == 40 else 88) for e in range(n)), ends
    p.reset(label="everybody")
    assert p.v.clock_groups == 1
    p.close()

    # a lock-step handle whose copy comes from a handle on another clock goes onto per-env clocks; from one on the same clock it does not
    chub = hub()
    a, b, c = [chub.VecChargingHub(8, seed=s, **KW) for s in (1, 2, 3)]
    rs = np.random.RandomState(0)
    for v, k in ((a, 5), (b, 5), (c, 9)):
        v.reset()
        for _ in range(k):
            v.step(rs.uniform(-1, 1, size=(8, v.act_dim)).astype(np.float32))
    a.copy_envs([1], [2], source=b)
    assert a.clock_groups == 1 and a.clock == 5
    a.copy_envs([1, 3], [2, 7], source=c)
    assert a.clock_groups == 2 and np.array_equal(a.env_clocks(), [5, 5, 9, 5, 5, 5, 5, 9])
    a.reset()
    assert a.clock_groups == 1
    for v in (a, b, c):
        v.close()


# ---- 5. handles with per-env hub parameters -----------------------------------------------------------------------------------------

def test_rows_and_tables_come_along():
    n = 12
    kws = [dict(KW, hydro_prod_rate=60.0 + 25 * (i % 5), hydro_store_vlt=20.0 + 7 * (i % 3), init_soc=0.2 + 0.05 * (i % 4), fc_max_power=50.0 + 10 * (i % 6),
                fcev_permeate=0.01 * (1 + i % 3), renew_fluctuate=0.1 * (i % 4), price_fluctuate=0.05 * (i % 5), hydro_loss=0.001 * (i % 2))
           for i in range(n)]
    p = Mirror(KW, n, kws=kws)
    q = Mirror(KW, 6, kws=kws[6:], seed=99, env_id0=700, rs_seed=8)
    for m in (p, q):
        m.reset(label="all")
        for i in range(12):
            m.step(label=("before", i))
    src, dst = [1, 1, 8], [4, 10, 0]
    tabs = [p.v.hy_table(env=s) for s in src]
    rows = p.v.env_params()
    p.copy_from(p, src, dst)
    q.copy_from(p, [2, 3], [5, 0])
    for m, pairs in ((p, zip(src, dst)), (q, [(2, 5), (3, 0)])):
        got = m.v.env_params()
        for s, d in pairs:
            for f in FIELDS:
                assert got[f][d] == rows[f][s], (f, s, d)
            assert np.array_equal(m.v.hy_table(env=d), p.v.hy_table(env=s))
    for tab, d in zip(tabs, dst):
        assert np.array_equal(p.v.hy_table(env=d), tab)
    for i in range(96):
        for m, name in ((p, "main"), (q, "scratch")):
            d = m.step(label=(name, "after", i))
            if d.any():
                m.reset(d, (name, "reset at done", i))
    assert p.overflow() == 0 and q.overflow() == 0
    q.close()
    p.close()

    # a source row beyond the destination handle's FCEV arrival bound is refused, as chub_set_env_params refuses it
    chub = hub()
    big = chub.VecChargingHub(4, station_list=[20, 25], station_type_list=["fast", "slow"], fcev_permeate=[0.01, 0.01, 0.9, 0.01])
    small = chub.VecChargingHub(4, station_list=[20, 25], station_type_list=["fast", "slow"], fcev_permeate=[0.01, 0.02, 0.01, 0.02])
    for v in (big, small):
        v.reset()
    before = digest(small)
    with pytest.raises(chub.ChubError, match=r"libchub error -1: src_idx\[1\] = 2.*FCEV arrivals"):
        small.copy_envs([0, 2], [1, 3], source=big)
    same(digest(small), before, "a refused copy wrote")
    small.copy_envs([0, 1], [1, 3], source=big)
    assert np.array_equal(small.env_params()["fcev_permeate"], [0.01, 0.01, 0.01, 0.01])
    for v in (big, small):
        v.close()


# ---- 6. the device form, from torch -----------------------------------------------------------------------------------------------

TORCH_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["CHUB_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHUB_ROOT"], "tests"))
import numpy as np
import torch  # before libchub is loaded: both share one HIP runtime
import charginghub_env_amd as chub
from test_gpu_copy_envs import KW, digest, same
n, k = 512, 40
kw = dict(KW)
env = chub.wrappers.TorchHubVecEnv(n, kw.pop("station_list"), kw.pop("station_type_list"), seed=31, autoreset=False, **kw)
twin = chub.VecChargingHub(n, seed=31, **KW)
gen = torch.Generator(device="cpu").manual_seed(4)
acts = [(torch.rand((n, env.act_dim), generator=gen) * 2 - 1) for _ in range(16)]
dev = [a.cuda() for a in acts]
env.reset()
twin.reset()
for i in range(6):
    obs, rew, done, _ = env.step(dev[i])
    t_obs, t_rew, _, _ = twin.step(acts[i].numpy())
# no host read between the step and the copy: the ranking, the indices and the copy are all enqueued on torch's stream
best = torch.topk(rew, k).indices
worst = torch.topk(rew, k, largest=False).indices
cur = env.copy_envs(best, worst)
obs_after = cur.clone()
nxt = env.step(dev[6])
order = np.argsort(-t_rew, kind="stable")
b, w = best.cpu().numpy(), worst.cpu().numpy()
assert np.array_equal(np.sort(t_rew[b]), np.sort(t_rew[order[:k]]))  # (ties aside, torch picked the twin's top k)
twin.copy_envs(b, w)
assert np.array_equal(obs_after.cpu().numpy()[w], t_obs[b])  # the cached observation rows came along
t_nxt = twin.step(acts[6].numpy())
assert np.array_equal(nxt[0].cpu().numpy(), t_nxt[0]) and np.array_equal(nxt[1].cpu().numpy(), t_nxt[1])
same(digest(env.vec), digest(twin), "device form against host form")
assert env.vec.clock_groups == 1  # (per-env clocks, all equal)
# a snapshot taken after a copy restores and continues identically
snap = env.vec.get_state()
run1 = [tuple(x.cpu().numpy().copy() for x in env.step(dev[i])[:3]) for i in range(7, 12)]
env.vec.set_state(snap)
run2 = [tuple(x.cpu().numpy().copy() for x in env.step(dev[i])[:3]) for i in range(7, 12)]
for x, y in zip(run1, run2):
    for u, v in zip(x, y):
        assert np.array_equal(u, v)
# an index out of range is skipped by the kernel; nobody else is touched
before = digest(env.vec)
bad_s = torch.tensor([1, n + 5, -1], dtype=torch.int64, device="cuda")
bad_d = torch.tensor([n, 3, 4], dtype=torch.int64, device="cuda")
env.vec.copy_envs_device(bad_s.data_ptr(), bad_d.data_ptr(), 3, stream=torch.cuda.current_stream().cuda_stream)
same(digest(env.vec), before, "pairs with an index out of range must be skipped")
env.close()
twin.close()
print("COPY_TORCH_OK")
'''


def test_device_form_from_torch_topk_equals_the_host_form():
    """in a child process (torch initialises the HIP runtime first, as in tests/test_gpu_torch_side.py)"""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], env=dict(os.environ, CHUB_ROOT=root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "COPY_TORCH_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing():
    chub = hub()
    lib = chub._lib.load_library()
    n = 10
    v = chub.VecChargingHub(n, seed=3, **KW)
    rs = np.random.RandomState(1)
    v.reset()
    for _ in range(5):
        v.step(rs.uniform(-1, 1, size=(n, v.act_dim)).astype(np.float32))
    before = digest(v)

    def refused(code, pattern, fn):
        with pytest.raises(chub.ChubError, match=r"libchub error %d: .*%s" % (code, pattern)):
            fn()
        same(digest(v), before, ("a refused copy wrote", pattern))

    idx = lambda *a: np.array(a, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    one = idx(1)
    for args in ((None, v._h, p(one), p(one), 1), (v._h, None, p(one), p(one), 1), (v._h, v._h, None, p(one), 1), (v._h, v._h, p(one), None, 1)):
        refused(-1, "null argument", lambda: chub._lib.check(lib.chub_copy_envs(*args)))
        refused(-1, "null argument", lambda: chub._lib.check(lib.chub_copy_envs_device(*args, None)))
    refused(-1, "count < 0", lambda: chub._lib.check(lib.chub_copy_envs(v._h, v._h, p(one), p(one), -1)))
    refused(-1, r"src_idx\[1\] = 10 is out of range", lambda: v.copy_envs([0, 10], [1, 2]))
    refused(-1, r"src_idx\[0\] = -1 is out of range", lambda: v.copy_envs([-1], [1]))
    refused(-1, r"dst_idx\[2\] = 10 is out of range", lambda: v.copy_envs([0, 0, 0], [1, 2, 10]))
    refused(-1, r"dst_idx\[2\] = 4 names a destination a second time", lambda: v.copy_envs([0, 1, 2], [4, 5, 4]))
    refused(-1, r"src_idx\[1\] = 4 is also a destination", lambda: v.copy_envs([0, 4], [4, 5]))
    refused(-1, r"src_idx\[0\] = 3 is also a destination", lambda: v.copy_envs([3], [3]))
    others = {"RNG modes": dict(rng="philox_curves"), "station_list": dict(station_list=[20, 24]), "station_list, station_type": dict(station_type_list=["slow", "slow"]),
              "constant_charging": dict(constant_charging=True), "chub_config scalars": dict(init_soc=0.3),
              "per-env hub parameters": dict(init_soc=[0.2] * n)}
    for pattern, change in others.items():
        o = chub.VecChargingHub(n, seed=3, **dict(KW, **change))
        refused(-1, pattern, lambda: v.copy_envs([1], [2], source=o))
        with pytest.raises(chub.ChubError, match=r"libchub error -1: .*%s" % pattern):
            o.copy_envs([1], [2], source=v)
        o.close()
    # tape handles and handles inside a capture
    tape = chub.VecChargingHub(n, seed=3, **KW)
    tape.tape_register_soc([30.0])
    refused(-4, "tape handle", lambda: v.copy_envs([1], [2], source=tape))
    with pytest.raises(chub.ChubError, match="libchub error -4: .*tape handle"):
        tape.copy_envs([1], [2], source=v)
    tape.close()
    stream = C.c_void_p()
    chub._lib.check(lib.chub_stream_create(0, C.byref(stream)))
    v.graph_begin(stream)
    with pytest.raises(chub.ChubError, match="libchub error -4: .*chub_graph_begin"):
        v.copy_envs([1], [2])
    with pytest.raises(chub.ChubError):  # (an empty capture is no graph; the handle is back where chub_graph_begin found it)
        v.graph_end(stream)
    chub._lib.check(lib.chub_stream_destroy(0, stream))
    same(digest(v), before, "the refused copy inside the capture wrote")
    # count == 0 is a no-op; and a handle without the arena copies like any other (the copy does not need it)
    v.copy_envs([], [])
    chub._lib.check(lib.chub_copy_envs_device(v._h, v._h, p(one), p(one), 0, None))
    same(digest(v), before, "count == 0 wrote")
    assert v.clock_groups == 1
    loose = chub.VecChargingHub(n, seed=3, no_arena=True, **KW)
    loose.reset()
    loose.copy_envs([1, 1], [2, 3], source=v)
    got = digest(loose)
    for k, x in enumerate(before):
        assert np.array_equal(got[k][[2, 3]], x[[1, 1]]), k
    loose.close()
    v.close()


# ---- 8. benchmark size ------------------------------------------------------------------------------------------------------------

def test_worst_tenth_overwritten_by_the_best_at_65536_envs():
    chub = hub()
    n, k, seed = 65536, 6554, 0xC0FFEE
    kw = dict(station_list=[20, 25], station_type_list=["fast", "slow"], hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2,
              fc_max_power=100.0, fcev_permeate=0.01)
    v = chub.VecChargingHub(n, seed=seed, **kw)
    v.set_telemetry(True)
    cfg = orc_cfg(kw)
    h = orc.orc_vec_create(C.byref(cfg), orclib.tables(), n, 0, orclib.PHILOX, seed)
    D, A = v.obs_dim, v.act_dim
    o_obs, o_rew, o_done = np.zeros((n, D)), np.zeros(n), np.zeros(n, dtype=np.uint8)
    rs = np.random.RandomState(9)
    v.reset()
    orc.orc_vec_reset(h, None, None, ptr(o_obs))
    rew = None
    for i in range(3):
        act = rs.uniform(-1, 1, size=(n, A)).astype(np.float32)
        rew = v.step(act)[1]
        orc.orc_vec_step(h, ptr(act), None, ptr(o_obs), ptr(o_rew), ptr(o_done), 16)
    order = np.argsort(rew, kind="stable")
    worst, best = order[:k], order[-k:]
    v.copy_envs(best, worst)
    size = orc.orc_sizeof_env()
    for s, d in zip(best, worst):
        C.memmove(orc.orc_vec_env(h, int(d)), orc.orc_vec_env(h, int(s)), size)
        orc.orc_rng_seed_philox(orc.orc_env_rng(orc.orc_vec_env(h, int(d))), seed, int(d))
        orc.orc_rng_set_tick(orc.orc_env_rng(orc.orc_vec_env(h, int(d))), 4)  # one reset + three steps so far, as every other env
    assert v.clock_groups == 1
    act = rs.uniform(-1, 1, size=(n, A)).astype(np.float32)
    obs, rew, done, _ = v.step(act)
    orc.orc_vec_step(h, ptr(act), None, ptr(o_obs), ptr(o_rew), ptr(o_done), 16)
    S0, S1 = kw["station_list"]
    sl = v.slots()
    for kk, nk in ((0, S0), (1, S1)):
        want = np.zeros((n, 9, nk), dtype=np.float32)
        orc.orc_vec_slots(h, kk, ptr(want))
        assert np.array_equal(sl[kk].view(np.uint32), want.view(np.uint32)), kk
    ws = np.zeros((n, 2, 8))
    orc.orc_vec_station_scalars(h, ptr(ws))
    assert np.array_equal(v.station_scalars()[:, :, :6], ws[:, :, :6])
    assert np.array_equal(done.astype(np.uint8), o_done)
    close(v.obs_f64(), o_obs, "obs", rtol=TIGHT, atol=TIGHT)
    close(v.reward_f64(), o_rew, "reward", rtol=TIGHT, atol=TIGHT)
    assert orc.orc_vec_overflow(h) == 0
    orc.orc_vec_destroy(h)
    v.close()
