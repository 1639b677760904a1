"""Masks in device memory (chub_dmask_reset_envs_device / chub_dmask_step_envs_device) and the step that resets whoever finished
(chub_autoreset_step_device), on the GPU.  The reference behaviour at stake: every EvcsspManagerEnv_v6 is its own object with its own
clock (evcssp_manager.py:137-140, 271-273, 299, 304-316) -- a vector of them at different times of day ends its days one env at a time,
and a trainer resets each when ITS done fires.  Held here against (1) the host-mask calls, bit for bit; (2) the oracle, whose envs are
separate objects, each given the Philox tick the library reports for it; (3) the call's definition -- a step of everybody at tick T, a
reset of those done at T + 1 -- on the oracle; snapshots, captured graphs, the torch adapter, the benchmark size, refusals."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import orclib
from orclib import orc, ptr
from test_gpu_env_clocks import KW, Pair
from test_gpu_parity import _oracle_vec, close, hub

pytestmark = pytest.mark.gpu


def buffers():
    from charginghub_env_amd import multi_gpu
    return multi_gpu


class Dev(object):
    """a VecChargingHub with device buffers for the device-pointer calls"""

    def __init__(self, v, stream=0):
        mg = buffers()
        self.v, self.n, self.D, self.A = v, v.n_envs, v.obs_dim, v.act_dim
        n, D, A = self.n, self.D, self.A
        self.st = stream
        self.mask, self.act = mg.DeviceBuffer(n), mg.DeviceBuffer(n * A * 4)
        self.obs, self.rew, self.done = mg.DeviceBuffer(n * D * 4), mg.DeviceBuffer(n * 4), mg.DeviceBuffer(n)
        self.packed, self.final = mg.DeviceBuffer(n * (D + 2) * 4), mg.DeviceBuffer(n * D * 4)
        self.z, self.days = mg.DeviceBuffer(n * 3 * 8), mg.DeviceBuffer(n * 2 * 4)
        self.rz, self.rdays = mg.DeviceBuffer(n * 3 * 8), mg.DeviceBuffer(n * 2 * 4)
        for b, dt, shape in ((self.obs, np.float32, (n, D)), (self.rew, np.float32, (n,)), (self.done, np.uint8, (n,)),
                             (self.packed, np.float32, (n, D + 2)), (self.final, np.float32, (n, D))):
            b.from_host(np.full(shape, 7, dtype=dt))  # a pattern no kernel writes: untouched rows show

    def reset_dmask(self, mask, days=None, z=None):
        self.mask.from_host(np.ascontiguousarray(mask, dtype=np.uint8), self.st)
        if days is not None:
            self.days.from_host(np.ascontiguousarray(days, dtype=np.int32), self.st)
            self.z.from_host(np.ascontiguousarray(z, dtype=np.float64), self.st)
        self.v.reset_envs_dmask_device(self.mask.ptr, self.obs.ptr, self.days.ptr if days is not None else 0,
                                       self.z.ptr if days is not None else 0, stream=self.st)
        return self.obs.to_host(np.float32, (self.n, self.D), self.st)

    def step_dmask(self, mask, act, z=None):
        self.mask.from_host(np.ascontiguousarray(mask, dtype=np.uint8), self.st)
        self.act.from_host(act, self.st)
        if z is not None:
            self.z.from_host(np.ascontiguousarray(z, dtype=np.float64), self.st)
        self.v.step_envs_dmask_device(self.mask.ptr, self.act.ptr, self.obs.ptr, self.rew.ptr, self.done.ptr,
                                      d_exo_z=self.z.ptr if z is not None else 0, stream=self.st)
        return (self.obs.to_host(np.float32, (self.n, self.D), self.st), self.rew.to_host(np.float32, (self.n,), self.st),
                self.done.to_host(np.uint8, (self.n,), self.st))

    def autoreset(self, act, z=None, rdays=None, rz=None, final=True):
        self.act.from_host(act, self.st)
        if z is not None:
            self.z.from_host(np.ascontiguousarray(z, dtype=np.float64), self.st)
            self.rdays.from_host(np.ascontiguousarray(rdays, dtype=np.int32), self.st)
            self.rz.from_host(np.ascontiguousarray(rz, dtype=np.float64), self.st)
        self.v.step_autoreset_device(self.act.ptr, self.packed.ptr, self.final.ptr if final else 0, d_exo_z=self.z.ptr if z is not None else 0,
                                     d_reset_exo_days=self.rdays.ptr if z is not None else 0, d_reset_exo_z=self.rz.ptr if z is not None else 0,
                                     stream=self.st)
        return self.packed.to_host(np.float32, (self.n, self.D + 2), self.st), self.final.to_host(np.float32, (self.n, self.D), self.st)


def state_arrays(v):
    t, ticks = v.env_clocks(ticks=True)
    return [np.concatenate([x.reshape(v.n_envs, -1) for x in v.slots()], axis=1), v.station_scalars().reshape(v.n_envs, -1), t, ticks,
            v.obs_f64(), v.reward_f64()]


def same_state(a, b, label):
    for k, (x, y) in enumerate(zip(state_arrays(a), state_arrays(b))):
        assert np.array_equal(x, y, equal_nan=True), (label, "state array", k)


def random_mask(rs, n):
    """neither empty nor full"""
    m = rs.uniform(size=n) < rs.choice([0.1, 0.5, 0.9])
    m[rs.randint(n)] = True
    m[(np.nonzero(m)[0][0] + 1) % n] = False
    assert 0 < m.sum() < n
    return m


def make_pair_of_handles(rng, piles, n, rows=False, seed=99):
    chub = hub()
    kw = dict(KW, station_list=list(piles))
    if rows:
        rs = np.random.RandomState(5)
        kw.update(hydro_prod_rate=list(rs.uniform(80, 200, n)), hydro_store_vlt=list(rs.uniform(20, 60, n)), init_soc=list(rs.uniform(0.15, 0.6, n)))
    out = []
    for _ in range(2):
        v = chub.VecChargingHub(n, seed=seed, rng=rng, env_id0=300, **kw)
        v.set_telemetry(True)
        if rng == "compat":
            rs = np.random.RandomState(3)
            v.set_compat_seeds(np.stack([rs.randint(1, 2**31 - 1, n), rs.randint(1, 2**31 - 1, n)], axis=1).astype(np.uint32))
            v.compat_replay_constructor()
        out.append(v)
    return out


CASES = [(rng, piles, False) for rng in ("philox", "philox_curves", "compat") for piles in ([20, 25], [16, 0], [3, 5])] + [("philox", [20, 25], True)]


# ---- 1. device mask == host mask
@pytest.mark.parametrize("rng,piles,rows", CASES, ids=lambda c: str(c).replace(" ", ""))
def test_device_mask_equals_host_mask(rng, piles, rows):
    n = 77
    vh, vd = make_pair_of_handles(rng, piles, n, rows)
    d = Dev(vd)
    rs = np.random.RandomState(17)
    compat = rng == "compat"

    def variates():
        return (np.stack([rs.randint(0, 100, n), rs.randint(0, 150, n)], axis=1).astype(np.int32), rs.normal(size=(n, 3))) if compat else (None, None)

    days, z = variates()
    vh.reset(days, z)
    vd.reset(days, z)
    A = vh.act_dim
    for i in range(40):
        m = random_mask(rs, n)
        days, z = variates()
        if rs.randint(4) == 0:
            oh = vh.reset_envs(m, days, z).copy()
            od = d.reset_dmask(m, days, z)
            assert np.array_equal(oh[m], od[m]), (i, "reset obs")
            assert (od[~m] == 7).all() or i > 0  # (rows of envs the first masked call does not name are untouched)
        else:
            act = rs.uniform(-1, 1, size=(n, A)).astype(np.float32)
            oh, rh, dh, _ = vh.step_envs(m, act, z)
            od, rd, dd = d.step_dmask(m, act, z)
            assert np.array_equal(oh[m], od[m]) and np.array_equal(rh[m], rd[m]) and np.array_equal(dh[m], dd[m].astype(bool)), (i, "step outputs")
        same_state(vh, vd, (rng, piles, i))
        assert vd.clock_groups == vh.clock_groups
    if compat:
        assert np.array_equal(vh.compat_state(), vd.compat_state())
    vh.close()
    vd.close()


# ---- 2. against the oracle, all-zero and all-ones masks included
class DPair(Pair):
    """test_gpu_env_clocks.Pair with the masked calls going through device masks"""

    def __init__(self, kw, n, rng="philox"):
        Pair.__init__(self, kw, n, rng=rng)
        self.d = Dev(self.v)
        self.calls = 0  # launches so far = the handle's Philox tick

    def reset(self, mask=None, label=""):
        self.calls += 1
        if mask is None:
            return Pair.reset(self, None, label)
        rows = np.nonzero(mask)[0]
        before = self.d.obs.to_host(np.float32, (self.n, self.D))
        obs = self.d.reset_dmask(mask)
        t, ticks = self.v.env_clocks(ticks=True)
        assert (ticks[rows] == self.calls).all(), (label, ticks, self.calls)  # the tick the launch really had, for exactly the envs it served
        for e in rows:
            self._oracle_tick(e, ticks[e])
            orc.orc_env_reset(orc.orc_vec_env(self.h, e), None, None, ptr(self.o_obs[e]))
        self.t[rows] = 0
        assert np.array_equal(t, self.t), (label, t, self.t)
        assert np.array_equal(obs[~np.asarray(mask, dtype=bool)], before[~np.asarray(mask, dtype=bool)]), (label, "rows of other envs written")
        self._compare(np.arange(self.n), ("reset", label), False)  # EVERY env: the ones not served must not have moved
        close(obs[rows], self.o_obs[rows], (label, "reset obs f32"), atol=1e-6)

    def step(self, mask=None, label=""):
        self.calls += 1
        if mask is None:
            return Pair.step(self, None, label)
        mask = np.asarray(mask, dtype=bool)
        rows = np.nonzero(mask)[0]
        act = self.rs.uniform(-1, 1, size=(self.n, self.A)).astype(np.float32)
        before = [b.copy() for b in (self.d.obs.to_host(np.float32, (self.n, self.D)), self.d.rew.to_host(np.float32, (self.n,)),
                                     self.d.done.to_host(np.uint8, (self.n,)))]
        obs, rew, done = self.d.step_dmask(mask, act)
        t, ticks = self.v.env_clocks(ticks=True)
        assert (ticks[rows] == self.calls).all(), (label, ticks, self.calls)
        for e in rows:
            self._oracle_tick(e, ticks[e])
            dn, r = C.c_int(0), C.c_double(0.0)
            orc.orc_env_step(orc.orc_vec_env(self.h, e), ptr(act[e]), None, ptr(self.o_obs[e]), C.byref(r), C.byref(dn))
            self.o_rew[e], self.o_done[e] = r.value, dn.value
        self.t[rows] = (self.t[rows] + 1) % 96
        assert np.array_equal(t, self.t), (label, t, self.t)
        for got, old in zip((obs, rew, done), before):
            assert np.array_equal(got[~mask], old[~mask]), (label, "rows of other envs written")
        assert np.array_equal(done[rows].astype(bool), self.o_done[rows].astype(bool)), (label, "done")
        self._compare(np.arange(self.n), ("step", label), False)
        close(obs[rows], self.o_obs[rows], (label, "obs f32"), atol=1e-6)
        close(rew[rows], self.o_rew[rows], (label, "reward f32"), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("rng", ["philox", "philox_curves"])
def test_device_masks_against_the_oracle(rng):
    n = 44
    p = DPair(KW, n, rng=rng)
    idx = np.arange(n)
    none, everybody = np.zeros(n, dtype=bool), np.ones(n, dtype=bool)
    p.reset(label="all")
    for i in range(3):
        p.step(label=("lock-step", i))
    p.step(idx % 3 == 0, "every third env")
    p.step(none, "nobody: a tick, nothing else")       # (the next call's tick is checked to have moved on by it)
    p.step(idx < n // 2, "first half")
    p.reset(none, "nobody reset")
    p.reset(idx % 5 == 1, "a scattered subset")
    p.step(everybody, "everybody, through a device mask")
    assert p.v.clock_groups > 1
    p.reset(everybody, "everybody reset through a device mask")
    assert p.v.clock_groups == 1
    t, ticks = p.v.env_clocks(ticks=True)
    assert (ticks == p.calls).all()
    p.step(idx % 2 == 0, "still on per-env clocks")     # a device mask naming everybody did not return the handle to lock-step:
    assert p.v.clock_groups == 2
    for i in range(3):
        p.step(label=("everybody", i))
    p.reset(label="chub_reset of everybody")            # ... this does
    p.step(label="lock-step again")
    assert p.v.clock_groups == 1
    assert orc.orc_vec_overflow(p.h) == 0
    p.close()


# ---- 3. auto-reset == its definition, on the oracle's separate env objects
class APair(DPair):
    def head_start(self, groups, apart):
        """group g of the envs (contiguous) goes g * apart slots ahead: masked steps, as StaggeredHub.reset does"""
        g = np.arange(self.n) * groups // self.n
        for k in range(1, (groups - 1) * apart + 1):
            self.step(g * apart >= k, ("head start", k))
        return g

    def autoreset(self, label, resets):
        T = self.calls + 1
        self.calls += 2  # always two ticks
        act = self.rs.uniform(-1, 1, size=(self.n, self.A)).astype(np.float32)
        old_final = self.d.final.to_host(np.float32, (self.n, self.D))
        packed, final = self.d.autoreset(act)
        o_final = np.zeros((self.n, self.D))
        for e in range(self.n):
            self._oracle_tick(e, T)
            dn, r = C.c_int(0), C.c_double(0.0)
            env = orc.orc_vec_env(self.h, e)
            orc.orc_env_step(env, ptr(act[e]), None, ptr(self.o_obs[e]), C.byref(r), C.byref(dn))
            self.o_rew[e], self.o_done[e] = r.value, dn.value
            if dn.value:
                o_final[e] = self.o_obs[e]
                self._oracle_tick(e, T + 1)
                orc.orc_env_reset(env, None, None, ptr(self.o_obs[e]))
        done = self.o_done.astype(bool)
        self.t = np.where(done, 0, self.t + 1)
        assert np.array_equal(done, self.t == 0), label
        t, ticks = self.v.env_clocks(ticks=True)
        assert np.array_equal(t, self.t), (label, t, self.t)
        assert np.array_equal(ticks, np.where(done, T + 1, T)), (label, ticks, T)
        D = self.D
        assert np.array_equal(packed[:, D + 1], done.astype(np.float32)), (label, "done column")
        close(packed[:, :D], self.o_obs, (label, "obs f32"), atol=1e-6)
        close(packed[:, D], self.o_rew, (label, "reward f32"), rtol=1e-5, atol=1e-6)
        close(final[done], o_final[done], (label, "terminal observation"), atol=1e-6)
        assert np.array_equal(final[~done], old_final[~done]), (label, "terminal rows of other envs written")
        self._compare(np.arange(self.n), ("autoreset", label), False)  # slots and records bit for bit, obs64 to 1e-9
        # (the f64 reward of a reset env is the reset's 0, as after chub_reset_envs; its step's reward is in the packed row, checked above)
        close(self.v.reward_f64()[~done], self.o_rew[~done], (label, "reward f64"), rtol=1e-9, atol=1e-9)
        assert (self.v.reward_f64()[done] == 0).all(), label
        resets += done
        return int(done.sum())


@pytest.mark.parametrize("rng", ["philox", "philox_curves"])
def test_autoreset_equals_step_then_reset_of_the_done(rng):
    n = 35
    p = APair(KW, n, rng=rng)
    p.reset(label="all")
    g = p.head_start(7, 13)
    assert p.v.clock_groups == 7 and len(np.unique(p.t)) == 7
    resets = np.zeros(n, dtype=int)
    nobody = 0
    for i in range(200):
        nobody += p.autoreset(i, resets) == 0
    assert (resets >= 2).all(), resets
    assert nobody >= 50, nobody
    assert p.v.clock_groups == 7
    # a smoke check only: at this permeate no forecourt gets stuck, and the oracle exposes no count of its own to compare a non-zero one with
    # (the forecourt state itself -- queue length, line -- is in the observation and the telemetry compared above, every call)
    assert p.v.fcev_stuck_count() == 0
    assert orc.orc_vec_overflow(p.h) == 0
    p.close()


def test_autoreset_from_lock_step_and_without_final_obs():
    """valid on a lock-step handle (it moves onto per-env clocks first); d_final_obs may be null"""
    n = 20
    p = APair(KW, n)
    p.reset(label="all")
    for i in range(93):
        p.step(label=("lock-step", i))
    assert p.v.clock_groups == 1
    resets = np.zeros(n, dtype=int)
    counts = [p.autoreset(i, resets) for i in range(5)]
    assert counts == [0, 0, n, 0, 0]
    act = p.rs.uniform(-1, 1, size=(n, p.A)).astype(np.float32)
    before = p.d.final.to_host(np.float32, (n, p.D))
    p.d.autoreset(act, final=False)
    assert np.array_equal(before, p.d.final.to_host(np.float32, (n, p.D)))
    p.close()


# ... on COMPAT streams: a clone group replays a reference fixture on shifted clocks
@pytest.mark.parametrize("name,form,rows", [("env_c3_random", "packed", False), ("env_c3_random", "wave", False), ("env_c3_random", "packed", True),
                                            ("env_c2_random", "packed", False), ("env_one_pile", "packed", False)])
def test_compat_clone_group_replays_the_reference_fixture_through_autoreset(name, form, rows):
    """The reference's recorded two-day trajectory (tests/golden: reseed, reset, 96 steps, reset WITHOUT a reseed, 96 steps).  Env 0 runs
    ahead alone; envs 1 .. 4 are clones of it (chub_copy_envs: in COMPAT the streams are state) taken 3, 7, 20 and 47 steps into the day, so
    the five envs cross the day's end in five different auto-reset calls.  Each call feeds env e the fixture's action and normals of ITS
    step; the reset rows of d_reset_exo_days / d_reset_exo_z carry the fixture's second reset for the envs that finish in that call and
    NaN for everybody else (only the rows of the reset envs may be read).  Every env stays bit-exact against the recorded run.
    rows: the same hub built by chub_create_params with every row the fixture's kwargs (k_env<.., ENV_PARAMS>)."""
    from test_gpu_parity import TIGHT, check_slots, kwargs_of
    chub = hub()
    g = orclib.load_golden(name)
    kw = kwargs_of(g)
    assert int(g["episodes"]) == 2 and int(g["steps_per_episode"]) == 96 and [int(x[0]) for x in g["seeds"]] == [0]
    clone_at = {3: 1, 7: 2, 20: 3, 47: 4}
    n, head = 5, 50
    if rows:
        from charginghub_env_amd._lib import ENV_PARAM_FIELDS
        kw = {k: ([v] * n if k in ENV_PARAM_FIELDS else v) for k, v in kw.items()}
    v = chub.VecChargingHub(n, rng="compat", slot_kernel=form, **kw)
    assert v.has_env_params == rows
    v.set_telemetry(True)
    d = Dev(v)
    A, D = v.act_dim, v.obs_dim
    rep = lambda a: np.repeat(np.asarray(a)[None, :], n, axis=0)
    v.set_compat_seeds(rep(g["ctor_seeds"]))
    v.compat_replay_constructor()
    v.reset(rep(g["ctor_days"]).astype(np.int32), rep(g["ctor_z"]))
    v.set_compat_seeds(rep([int(g["seeds"][0][1]), int(g["seeds"][0][2])]))
    v.reset(rep(g["reset_days"][0]).astype(np.int32), rep(g["reset_z"][0]))
    close(v.obs_f64(), rep(g["reset_obs"][0]), (name, "first reset"), rtol=TIGHT, atol=TIGHT)
    idx = np.zeros(n, dtype=int)

    def check_step(e, k, label):
        sl, sc, tel = v.slots(), v.station_scalars(), v.telemetry()
        check_slots(sl[0][e], g["slots0"][k], (name, label, e, k, "station0"))
        check_slots(sl[1][e], g["slots1"][k], (name, label, e, k, "station1"))
        assert np.array_equal(np.concatenate([sc[e, 0, :6], sc[e, 1, :6]]), g["stations"][k]), (name, label, e, k)
        assert np.array_equal(tel[e, 19:22], g["telem"][k][19:22]), (name, label, e, k, "fcev ints")
        close(v.obs_f64()[e], g["obs"][k], (name, label, "obs", e, k), rtol=TIGHT, atol=TIGHT)
        close(v.reward_f64()[e], g["reward"][k], (name, label, "reward", e, k), rtol=TIGHT, atol=TIGHT)

    only0 = np.arange(n) == 0
    for k in range(head):  # env 0 alone, through device masks; the clones are taken on the way
        if k in clone_at:
            v.copy_envs([0], [clone_at[k]])
            idx[clone_at[k]] = k
        d.step_dmask(only0, rep(g["action"][k]).astype(np.float32), rep(g["exo_z"][k]))
        check_step(0, k, "head start")
        idx[0] += 1
    assert sorted(idx) == [3, 7, 20, 47, 50] and v.clock_groups == 5
    alive = np.ones(n, dtype=bool)
    crossed, nobody, calls = 0, 0, 0
    while alive[0]:
        k = idx.copy()
        act = np.stack([g["action"][i] for i in k]).astype(np.float32)
        z = np.stack([g["exo_z"][i] for i in k])
        done = np.array([bool(g["done"][i]) for i in k])
        rdays, rz = np.zeros((n, 2), dtype=np.int32), np.full((n, 3), np.nan)
        rdays[done], rz[done] = g["reset_days"][1], g["reset_z"][1]
        packed, final = d.autoreset(act, z, rdays, rz)
        calls += 1
        nobody += not done.any()
        assert np.array_equal(packed[alive, D + 1], done[alive].astype(np.float32)), (name, calls)
        sc, o64 = v.station_scalars(), v.obs_f64()
        for e in np.nonzero(alive)[0]:
            close(packed[e, D], g["reward"][k[e]], (name, "packed reward", e, k[e]), rtol=1e-6, atol=1e-6)
            if not done[e]:
                check_step(e, k[e], "autoreset")
                close(packed[e, :D], g["obs"][k[e]], (name, "packed obs", e, k[e]), atol=1e-6)
                idx[e] += 1
            elif k[e] == 95:  # the day's end: reset in the same call, no reseed -- the fixture's second reset
                close(o64[e], g["reset_obs"][1], (name, "reset obs", e), rtol=TIGHT, atol=TIGHT)
                assert np.array_equal(np.concatenate([sc[e, 0, :6], sc[e, 1, :6]]), g["reset_stations"][1]), (name, "reset stations", e)
                close(packed[e, :D], g["reset_obs"][1], (name, "packed: first observation of the new episode", e), atol=1e-6)
                close(final[e], g["obs"][95], (name, "terminal observation", e), atol=1e-6)
                idx[e], crossed = 96, crossed + 1
            else:  # the end of the recording
                assert k[e] == 191
                alive[e] = False
    assert crossed == n and nobody >= 50 and calls == 192 - head, (crossed, nobody, calls)
    assert np.isfinite(v.obs_f64()).all()  # (no NaN row of the reset variates was read)
    v.close()


# ... and against its definition issued call by call, where no oracle run is set up: per-env parameter rows, COMPAT at random
@pytest.mark.parametrize("rng,piles,rows", [("philox", [20, 25], True), ("philox_curves", [20, 25], False), ("compat", [20, 25], False),
                                            ("compat", [16, 0], True)], ids=lambda c: str(c).replace(" ", ""))
def test_autoreset_equals_step_then_device_mask_reset(rng, piles, rows):
    n = 40
    va, vb = make_pair_of_handles(rng, piles, n, rows)
    da, db = Dev(va), Dev(vb)
    rs = np.random.RandomState(23)
    compat = rng == "compat"
    D, A = va.obs_dim, va.act_dim

    def variates():
        return (np.stack([rs.randint(0, 100, n), rs.randint(0, 150, n)], axis=1).astype(np.int32), rs.normal(size=(n, 3))) if compat else (None, None)

    days, z = variates()
    va.reset(days, z)
    vb.reset(days, z)
    grp = np.arange(n) * 5 // n
    for k in range(1, 4 * 19 + 1):
        act = rs.uniform(-1, 1, size=(n, A)).astype(np.float32)
        _, z = variates()
        da.step_dmask(grp * 19 >= k, act, z)
        db.step_dmask(grp * 19 >= k, act, z)
    nobody, resets = 0, np.zeros(n, dtype=int)
    for i in range(130):
        act = rs.uniform(-1, 1, size=(n, A)).astype(np.float32)
        _, z = variates()
        rdays, rz = variates()
        packed, final = da.autoreset(act, z, rdays, rz)
        db.act.from_host(act)
        if compat:
            db.z.from_host(z)
        vb.step_device_packed(db.act.ptr, db.packed.ptr, d_exo_z=db.z.ptr if compat else 0)
        pk = db.packed.to_host(np.float32, (n, D + 2))
        done = pk[:, D + 1] > 0.5
        new = db.reset_dmask(done, rdays, rz)
        pk[done, :D] = new[done]
        assert np.array_equal(packed, pk), i
        same_state(va, vb, (rng, i))
        nobody += not done.any()
        resets += done
    assert nobody >= 50 and (resets >= 1).all()
    if compat:
        assert np.array_equal(va.compat_state(), vb.compat_state())
    va.close()
    vb.close()


# ---- 4. snapshot after auto-reset calls -> a fresh handle -> continue
def test_snapshot_after_autoreset_restores_and_continues():
    chub = hub()
    n = 40
    kw = dict(seed=5, rng="philox", env_id0=10, **KW)
    rs = np.random.RandomState(2)
    acts = [rs.uniform(-1, 1, size=(n, 47)).astype(np.float32) for _ in range(160)]
    masks = [random_mask(rs, n) for _ in range(160)]

    def run(v, d, lo, hi):
        out = []
        for i in range(lo, hi):
            packed, final = d.autoreset(acts[i])
            out.append(packed)
            out.append(final[packed[:, -1] > 0.5])
            if i % 7 == 3:
                out.extend(x[masks[i]] for x in d.step_dmask(masks[i], acts[i]))
        return out

    def start():
        v = chub.VecChargingHub(n, **kw)
        v.set_telemetry(True)
        v.reset()
        for k in range(1, 61):
            v.step_envs(np.arange(n) * 4 // n * 20 >= k, acts[k])
        return v

    a = start()
    da = Dev(a)
    ra = run(a, da, 0, 160)
    b = start()
    db = Dev(b)
    run(b, db, 0, 70)
    snap = b.get_state()
    b.close()
    c = chub.VecChargingHub(n, **kw)
    c.set_telemetry(True)
    c.set_state(snap)
    dc = Dev(c)
    rc = run(c, dc, 70, 160)
    assert len(rc) > 180
    for k, (x, y) in enumerate(zip(ra[len(ra) - len(rc):], rc)):
        assert np.array_equal(x, y), ("output", k, "of the continued run")
    same_state(a, c, "after the restored run")
    a.close()
    c.close()


# ---- 5. a captured graph of auto-reset calls and device-mask steps, replayed with its inputs rewritten in place
def test_graph_of_autoreset_calls_equals_eager():
    chub = hub()
    mg = buffers()
    n = 52
    kw = dict(seed=77, rng="philox", env_id0=0, **KW)
    rs = np.random.RandomState(8)

    def start():
        v = chub.VecChargingHub(n, **kw)
        v.set_telemetry(True)
        v.reset()
        head = rs_head.uniform(-1, 1, size=(n, v.act_dim)).astype(np.float32)
        for k in range(1, 79):
            v.step_envs(np.arange(n) * 7 // n * 13 >= k, head)
        return v

    rs_head = np.random.RandomState(1)
    g = start()
    rs_head = np.random.RandomState(1)
    e = start()
    assert g.clock_groups == 7
    st = mg.Stream(0)
    dg, de = Dev(g, st.ptr), Dev(e)
    # the capture: 8 auto-reset calls + 2 device-mask steps = 18 launches
    dg.act.from_host(np.zeros((n, g.act_dim), dtype=np.float32), st.ptr)
    dg.mask.from_host(np.zeros(n, dtype=np.uint8), st.ptr)
    st.sync()
    g.graph_begin(st.ptr)
    for k in range(8):
        g.step_autoreset_device(dg.act.ptr, dg.packed.ptr, dg.final.ptr, stream=st.ptr)
    for k in range(2):
        g.step_envs_dmask_device(dg.mask.ptr, dg.act.ptr, dg.obs.ptr, dg.rew.ptr, dg.done.ptr, stream=st.ptr)
    graph = g.graph_end(st.ptr)
    for r in range(30):
        act = rs.uniform(-1, 1, size=(n, g.act_dim)).astype(np.float32)
        mask = np.zeros(n, dtype=bool) if r == 11 else np.ones(n, dtype=bool) if r == 12 else random_mask(rs, n)
        dg.act.from_host(act, st.ptr)
        dg.mask.from_host(mask.astype(np.uint8), st.ptr)
        g.graph_launch(graph, st.ptr)
        for k in range(8):
            pe, fe = de.autoreset(act)
        for k in range(2):
            oe, re_, dne = de.step_dmask(mask, act)
        st.sync()
        if r % 10 == 9 or r in (0, 11, 12):
            assert np.array_equal(dg.packed.to_host(np.float32, (n, g.obs_dim + 2), st.ptr), pe), r
            assert np.array_equal(dg.final.to_host(np.float32, (n, g.obs_dim), st.ptr), fe), r
            assert np.array_equal(dg.obs.to_host(np.float32, (n, g.obs_dim), st.ptr), oe), r
            assert np.array_equal(dg.rew.to_host(np.float32, (n,), st.ptr), re_), r
            same_state(g, e, ("replay", r))  # slots, records, clocks and the final ticks included
    t, ticks = g.env_clocks(ticks=True)
    assert ticks.max() == 1 + 78 + 30 * 18
    g.graph_destroy(graph)
    g.close()
    e.close()
    st.destroy()


# ---- 6. the torch adapter on per-env clocks
TORCH_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["CHUB_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHUB_ROOT"], "tests"))
import torch  # before libchub: both must share one HIP runtime
torch.cuda.set_device(0)
import test_gpu_autoreset
test_gpu_autoreset.torch_adapter_per_env_mode()
print("TORCH_ADAPTER_OK")
"""


def test_torch_adapter_per_env_mode():
    """in a child process that imports torch first (as tests/test_gpu_torch_side.py does)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], env=dict(os.environ, CHUB_ROOT=root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TORCH_ADAPTER_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def torch_adapter_per_env_mode():
    import torch
    chub = hub()
    from charginghub_env_amd import wrappers
    n, kw = 48, dict(KW)
    src = wrappers.TorchHubVecEnv(n, seed=21, autoreset="per_env", **kw)
    dst = wrappers.TorchHubVecEnv(n, seed=22, autoreset="per_env", **kw)
    r_src = chub.VecChargingHub(n, seed=21, rng="philox", **kw)  # the reference run: the same calls issued from the host, masks read back
    r_dst = chub.VecChargingHub(n, seed=22, rng="philox", **kw)
    rs = np.random.RandomState(4)
    A, D = src.act_dim, src.obs_dim
    acts = [rs.uniform(-1, 1, size=(n, A)).astype(np.float32) for _ in range(8)]
    t_acts = [torch.from_numpy(a).cuda() for a in acts]
    d_ref = Dev(r_dst)

    def ref_step(v, d, act):
        """The reference run, driven from the host: step of everybody, done read back, reset through the mask.  The mask the host built goes
        through chub_dmask_reset_envs_device, not chub_reset_envs_device: a host mask that names nobody is no call and takes no tick, while
        the auto-reset call always takes two, so the two runs' Philox ticks would part on the first step in which nobody finishes.  (The
        device-mask reset is held to the host-mask reset bit for bit in test_device_mask_equals_host_mask; it shares neither the done count,
        nor the terminal rows, nor the packed output with the auto-reset call.)"""
        d.act.from_host(act)
        v.step_device_packed(d.act.ptr, d.packed.ptr)
        pk = d.packed.to_host(np.float32, (n, D + 2))
        done = pk[:, D + 1] > 0.5
        d.mask.from_host(done.astype(np.uint8))
        v.reset_envs_dmask_device(d.mask.ptr, d.obs.ptr)
        new = d.obs.to_host(np.float32, (n, D))
        first = np.where(done[:, None], new, pk[:, :D])
        return first, pk[:, D], done, pk[:, :D]

    d_rsrc = Dev(r_src)
    src.reset()
    dst.reset()
    r_src.reset_device(d_rsrc.obs.ptr)
    r_dst.reset_device(d_ref.obs.ptr)
    for i in range(30):
        src.step(t_acts[i % 8])
        ref_step(r_src, d_rsrc, acts[i % 8])
    for i in range(5):
        dst.step(t_acts[i % 8])
        ref_step(r_dst, d_ref, acts[i % 8])
    s_idx = torch.arange(0, 16, dtype=torch.int64, device="cuda")
    d_idx = torch.arange(10, 42, 2, dtype=torch.int64, device="cuda")
    dst.copy_envs(s_idx, d_idx, source=src)  # from an adapter at another slot of day
    r_dst.copy_envs(s_idx.cpu().numpy(), d_idx.cpu().numpy(), source=r_src)
    clock = np.full(n, 5)
    clock[d_idx.cpu().numpy()] = 30
    torch.cuda.synchronize()

    # no host read and no wait inside the adapter's step: only the enqueue-only entry point is called, and anything that would synchronise raises
    calls = []
    real = dst.vec.step_autoreset_device
    dst.vec.step_autoreset_device = lambda *a, **k: (calls.append("step_autoreset_device"), real(*a, **k))[1]
    for name in ("reset_device", "step_device_packed", "env_clocks", "sync", "reset_envs", "step_envs"):
        setattr(dst.vec, name, lambda *a, _n=name, **k: (_ for _ in ()).throw(AssertionError("the adapter called " + _n)))

    def forbidden(*a, **k):
        raise AssertionError("the adapter's step synchronised or read the device")

    patched = [(torch.cuda, "synchronize"), (torch.Tensor, "cpu"), (torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.Tensor, "numpy"),
               (torch.cuda.Stream, "synchronize"), (torch.cuda.Event, "synchronize"), (torch.Tensor, "__bool__")]
    outs = []
    for i in range(200):
        saved = [(o, nme, getattr(o, nme)) for o, nme in patched]
        try:
            for o, nme in patched:
                setattr(o, nme, forbidden)
            obs, reward, done, info = dst.step(t_acts[i % 8])
        finally:
            for o, nme, fn in saved:
                setattr(o, nme, fn)
        outs.append((obs.cpu().numpy().copy(), reward.cpu().numpy().copy(), done.cpu().numpy().copy(), dst.last_obs.cpu().numpy().copy()))
    assert calls == ["step_autoreset_device"] * 200
    last = np.zeros((n, D), dtype=np.float32)
    fired = np.zeros(n, dtype=int)
    for i in range(200):
        clock += 1
        want_done = clock == 96
        clock[want_done] = 0
        first, rew, done, term = ref_step(r_dst, d_ref, acts[i % 8])
        obs, reward, dn, last_obs = outs[i]
        assert np.array_equal(dn, want_done), i  # each env's own 96th step
        assert np.array_equal(done, want_done), i
        fired += want_done
        last[want_done] = term[want_done]
        assert np.array_equal(obs, first) and np.array_equal(reward, rew), i
        assert np.array_equal(last_obs, last), i  # rows valid where done (kept until the env's next episode end)
    assert (fired >= 2).all()
    for x in (src, dst, r_src, r_dst):
        x.close()


# ---- 7. the benchmark size
def digest(*arrays):
    h = hashlib.blake2b(digest_size=16)
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_full_size_day_of_autoreset_calls():
    """65 536 x [20, 25], PHILOX, 8 clock groups, one day: the auto-reset call on the production kernels (packed slot kernel, XCD-aware order)
    against its definition issued call by call on the wave-local slot kernel -- per-call digests and the end state array for array -- and
    the first 256 envs against the oracle."""
    chub = hub()
    mg = buffers()
    n, groups, apart = 65536, 8, 12
    kw = dict(KW)
    st = mg.Stream(0)
    grp = np.arange(n) * groups // n
    acts = []
    runs = []
    for form in ("auto", "wave"):
        v = chub.VecChargingHub(n, seed=31, rng="philox", slot_kernel=form, **kw)
        d = Dev(v, st.ptr)
        if not acts:
            for b in range(4):
                a = mg.DeviceBuffer(n * v.act_dim * 4)
                v.random_actions_device(a.ptr, 99, b, st.ptr)
                acts.append(a)
        D = v.obs_dim
        v.reset_device(d.obs.ptr, stream=st.ptr)
        for k in range(1, (groups - 1) * apart + 1):
            d.mask.from_host((grp * apart >= k).astype(np.uint8), st.ptr)
            v.step_envs_dmask_device(d.mask.ptr, acts[k % 4].ptr, d.obs.ptr, d.rew.ptr, d.done.ptr, stream=st.ptr)
        calls, n_done = [], []
        for i in range(96):
            if form == "auto":
                v.step_autoreset_device(acts[i % 4].ptr, d.packed.ptr, d.final.ptr, stream=st.ptr)
                pk = d.packed.to_host(np.float32, (n, D + 2), st.ptr)
            else:  # the definition
                v.step_device_packed(acts[i % 4].ptr, d.packed.ptr, stream=st.ptr)
                pk = d.packed.to_host(np.float32, (n, D + 2), st.ptr)
                done = pk[:, D + 1] > 0.5
                d.mask.from_host(done.astype(np.uint8), st.ptr)
                v.reset_envs_dmask_device(d.mask.ptr, d.obs.ptr, stream=st.ptr)
                pk[done, :D] = d.obs.to_host(np.float32, (n, D), st.ptr)[done]
            calls.append(digest(pk))
            n_done.append(int((pk[:, D + 1] > 0.5).sum()))
            if i == 50 and form == "auto":
                prefix = (pk[:256].copy(), )
        end = [np.concatenate([x.reshape(n, -1) for x in v.slots()], axis=1), v.station_scalars().reshape(n, -1)] + list(v.env_clocks(ticks=True))
        runs.append((calls, n_done, end))
        v.close()
    (ca, na, ea), (cw, nw, ew) = runs
    assert len(set(ca)) == 96
    assert sorted(x for x in na if x) == [n // groups] * groups and na.count(0) == 96 - groups  # every group ends its own day once
    first = [k for k, (a, b) in enumerate(zip(ca, cw)) if a != b]
    assert not first, ("first differing call", first[0])
    for k, (a, b) in enumerate(zip(ea, ew)):
        assert np.array_equal(a, b, equal_nan=True), ("end state array", k)
    # the first 256 envs against the oracle
    m = 256
    cfg, h = _oracle_vec(kw, m, 0, 31)
    o_obs = np.zeros((m, 15 - 2))
    host_acts = [a.to_host(np.float32, (n, 47), st.ptr)[:m].copy() for a in acts]

    def tick(e, t):
        orc.orc_rng_set_tick(orc.orc_env_rng(orc.orc_vec_env(h, e)), int(t) - 1)

    T = 1
    for e in range(m):
        tick(e, T)
        orc.orc_env_reset(orc.orc_vec_env(h, e), None, None, ptr(o_obs[e]))
    for k in range(1, (groups - 1) * apart + 1):
        T += 1
        for e in range(m):
            if grp[e] * apart >= k:
                tick(e, T)
                dn, r = C.c_int(0), C.c_double(0.0)
                orc.orc_env_step(orc.orc_vec_env(h, e), ptr(host_acts[k % 4][e]), None, ptr(o_obs[e]), C.byref(r), C.byref(dn))
    for i in range(51):
        T += 1
        for e in range(m):
            tick(e, T)
            dn, r = C.c_int(0), C.c_double(0.0)
            orc.orc_env_step(orc.orc_vec_env(h, e), ptr(host_acts[i % 4][e]), None, ptr(o_obs[e]), C.byref(r), C.byref(dn))
            if dn.value:
                tick(e, T + 1)
                orc.orc_env_reset(orc.orc_vec_env(h, e), None, None, ptr(o_obs[e]))
        T += 1
    close(prefix[0][:, :13], o_obs, "the first 256 envs after 51 calls", atol=1e-6)
    orc.orc_vec_destroy(h)
    st.destroy()


# ---- 8. refusals
def test_refusals():
    chub = hub()
    v = chub.VecChargingHub(8, seed=1, rng="philox", **KW)
    d = Dev(v)
    v.reset()
    lib, h = v._lib, v._h
    for rc in (lib.chub_dmask_reset_envs_device(h, None, None, None, d.obs.ptr, None),
               lib.chub_dmask_step_envs_device(h, None, d.act.ptr, None, d.obs.ptr, d.rew.ptr, d.done.ptr, None),
               lib.chub_autoreset_step_device(h, d.act.ptr, None, None, None, None, d.final.ptr, None)):
        assert rc == -1 and lib.chub_last_error().decode() == "null argument"
    assert v.clock_groups == 1 and v.env_clocks(ticks=True)[1].max() == 1  # nothing ran
    v.tape_register_soc(np.array([50.0], dtype=np.float32))  # a tape handle from here on
    for call in (lambda: v.reset_envs_dmask_device(d.mask.ptr, d.obs.ptr), lambda: v.step_envs_dmask_device(d.mask.ptr, d.act.ptr, d.obs.ptr, d.rew.ptr, d.done.ptr),
                 lambda: v.step_autoreset_device(d.act.ptr, d.packed.ptr)):
        with pytest.raises(chub.ChubError, match="libchub error -4: .*tape handle"):
            call()
    v.close()
    c = chub.VecChargingHub(8, seed=1, rng="compat", **KW)
    dc = Dev(c)
    c.reset(np.zeros((8, 2), dtype=np.int32), np.zeros((8, 3)))
    with pytest.raises(chub.ChubError, match="libchub error -1: .*d_reset_exo_days"):
        c.step_autoreset_device(dc.act.ptr, dc.packed.ptr, d_exo_z=dc.z.ptr)
    c.close()
