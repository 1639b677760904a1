"""Reward scaling on the device (include/chub.h, "reward scaling on the device"), bit for bit against tests/return_norm_lib.py unless said
otherwise: (1) the update from an empty state on every made case, with and without a carry and a mask, run twice, canaries in the carry;
(2) the carry across calls: two updates over halves against one over the whole, and three updates on random floats, within 6.21's derived
bounds of the definition applied to the state the device started from; (3) the scale's edge cases; (4) the scaled GAE on the made cases
with states set through set_state, the clip's edges, and scale 1 without a clip against chub_rollout_gae_device; (5) one recorded
iteration replayed three times against three eager ones; (6) the checkpoint blob; (7) the torch adapter's methods in a child process;
(8) refusals and ownership."""
import numpy as np
import pytest

import return_norm_lib as rl
from charginghub_env_amd import _lib
from test_gpu_autoreset import buffers
from test_gpu_lagrange import dbuf, stagger
from test_gpu_pile_obs import BASE, CANARY, make
from test_gpu_pile_set import RollSet
from test_gpu_policy import gaussian_layers
from test_gpu_policy_sample import close_all
from test_return_norm_cpu import IDS, VARIANTS, masked

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
CANARY_F64 = np.uint64(0x7FF8BEEF0000BEEF)  # a NaN no kernel writes
HANDLES = {}


def handle(n):
    """one small hub per batch size for the made-data tests (the calls read N and D of it and nothing else)"""
    if n not in HANDLES:
        HANDLES[n] = make("philox", (2, 3), n)
    return HANDLES[n]


@pytest.fixture(scope="module", autouse=True)
def close_handles():
    yield
    for v in HANDLES.values():
        v.close()
    HANDLES.clear()


def f32_of(u):
    return np.ascontiguousarray(u).view(F32)


def canaried(carry, mask, N):
    """the carry a test installs: the case's (zeros without one), a canary where the env is masked out"""
    c = np.zeros(N, dtype=F32) if carry is None else carry.copy()
    if mask is not None:
        c.view(np.uint32)[mask == 0] = CANARY
    return c


def install(rn, N, state=(0.0, 0.0, 0.0), scale=1.0, carry=None):
    rn.set_state(rl.blob_of(N, state, F32(scale), np.zeros(N, dtype=F32) if carry is None else carry))


def parts(rn):
    """(state [3] f64, scale f32, carry [N] f32) through the blob; synchronises"""
    magic, N, state, scale, carry = rl.blob_parts(rn.get_state())
    assert magic == rl.MAGIC
    return state, scale, carry


def check_update(got, want, mask, carry0, what):
    state, scale, carry = got
    assert np.array_equal(rl.bits(state), rl.bits(want["state"])), (what, "state", state, want["state"])
    assert rl.bits(F32(scale)) == rl.bits(F32(want["scale"])), (what, "scale", scale, want["scale"])
    live = want["live"]
    assert np.array_equal(rl.bits(carry)[live], rl.bits(want["carry"])[live]), (what, "carry")
    assert np.array_equal(rl.bits(carry)[~live], rl.bits(carry0)[~live]), (what, "a masked-out env's carry moved")
    if mask is not None and (~live).any():
        assert (rl.bits(carry)[~live] == CANARY).all()


# ---- 1. the update from an empty state
@pytest.mark.parametrize("case,carry", VARIANTS, ids=IDS)
def test_update_from_an_empty_state_equals_the_restatement_bit_for_bit(case, carry):
    a = rl.case_arrays(case, carry=carry, mask=masked(case, carry))
    N, T = case["N"], case["T"]
    v = handle(N)
    rn = v.make_return_norm(gamma=case["gamma"], eps=rl.EPS, clip=10.0)
    st0, sc0, c0 = parts(rn)
    assert (st0 == 0).all() and rl.bits(F32(sc0)) == rl.bits(F32(1.0)) and (rl.bits(c0) == 0).all(), "after create: empty, scale 1.0f"
    packed = dbuf(rl.packed_of(a["reward"], a["done"], v.obs_dim))
    mask = None if a["mask"] is None else dbuf(a["mask"])
    carry0 = canaried(a["carry"], a["mask"], N)
    want = rl.update([0.0, 0.0, 0.0], 1.0, a["carry"], a["reward"], a["done"], case["gamma"], rl.EPS, a["mask"])
    runs = []
    for again in range(2):
        install(rn, N, carry=carry0)
        rn.update_device(T, packed.ptr, d_mask=0 if mask is None else mask.ptr)
        runs.append(parts(rn))
        check_update(runs[-1], want, a["mask"], carry0, (case["name"], carry, again))
    assert all(np.array_equal(rl.bits(x), rl.bits(y)) for x, y in zip(runs[0], runs[1])), "equal inputs, identical bits"
    assert runs[0][0][0] == T * int(want["live"].sum())
    close_all(rn, packed, *([] if mask is None else [mask]))


def test_an_all_zero_mask_writes_nothing_and_the_reset_empties():
    case = rl.case_named("n257-t9-last-g1")
    a = rl.case_arrays(case, carry=True)
    N, T = case["N"], case["T"]
    v = handle(N)
    rn = v.make_return_norm(gamma=1.0, eps=rl.EPS, clip=0.0)
    packed, nobody = dbuf(rl.packed_of(a["reward"], a["done"], v.obs_dim)), dbuf(np.zeros(N, dtype=np.uint8))
    rn.update_device(T, packed.ptr, d_mask=nobody.ptr)
    st, sc, c = parts(rn)
    assert (rl.bits(st) == 0).all() and rl.bits(F32(sc)) == rl.bits(F32(1.0)) and (rl.bits(c) == 0).all(), "n == 0: the scale is 1.0f"
    assert rn.scale() == 1.0 and rn.state().tolist() == [0.0, 0.0, 0.0]
    # a state that is not empty keeps its bits under an all-zero mask, the installed scale included
    install(rn, N, state=(12.0, -3.5, 99.0), scale=0.125, carry=a["carry"])
    before = rn.get_state()
    rn.update_device(T, packed.ptr, d_mask=nobody.ptr)
    assert rn.get_state() == before
    # reset_carry with a mask, then without; reset_device
    some = (np.arange(N) % 3 == 0).astype(np.uint8)
    d_some = dbuf(some)
    rn.reset_carry_device(d_mask=d_some.ptr)
    st, sc, c = parts(rn)
    assert st.tolist() == [12.0, -3.5, 99.0] and sc == F32(0.125)
    assert (rl.bits(c)[some != 0] == 0).all() and np.array_equal(rl.bits(c)[some == 0], rl.bits(a["carry"])[some == 0])
    rn.reset_carry_device()
    assert (rl.bits(parts(rn)[2]) == 0).all() and parts(rn)[0].tolist() == [12.0, -3.5, 99.0]
    install(rn, N, state=(12.0, -3.5, 99.0), scale=0.125, carry=a["carry"])
    rn.reset_device()
    st, sc, c = parts(rn)
    assert (rl.bits(st) == 0).all() and rl.bits(F32(sc)) == rl.bits(F32(1.0)) and (rl.bits(c) == 0).all()
    close_all(rn, packed, nobody, d_some)


# ---- 2. the carry across calls
def within_bounds(state, state0, g, live, what):
    want, b_mean, b_m2 = rl.merge_bounds(state0, g, live)
    print(what, "mean", state[1], "want", want[1], "bound", b_mean, "M2", state[2], "want", want[2], "bound", b_m2)
    assert state[0] == want[0], (what, "n")
    assert abs(state[1] - want[1]) <= b_mean, (what, "mean", state[1], want[1], b_mean)
    assert abs(state[2] - want[2]) <= b_m2, (what, "M2", state[2], want[2], b_m2)


@pytest.mark.parametrize("name,with_mask", [("n513-t17-edge-g1", False), ("n256-t17-random9-g05", True), ("n257-t17-twice-g1", True),
                                            ("n513-t17-none-g1", False)])
def test_two_updates_over_halves_against_one_over_the_whole(name, with_mask):
    """T = 17 split 8 + 9, at the first chunk's edge.  The carry and n are equal on bits; mean and M2 of the second half, which starts
    from a state that is not empty, are held to the definition in exact rationals applied to the state the device STARTED from"""
    case = rl.case_named(name)
    a = rl.case_arrays(case, carry=True, mask=with_mask)
    N, T = case["N"], case["T"]
    v = handle(N)
    D = v.obs_dim
    full = rl.packed_of(a["reward"], a["done"], D)
    whole, first, second = dbuf(full), dbuf(full[:8]), dbuf(full[8:])
    mask = None if a["mask"] is None else dbuf(a["mask"])
    d_mask = 0 if mask is None else mask.ptr
    carry0 = canaried(a["carry"], a["mask"], N)
    one, two = v.make_return_norm(gamma=case["gamma"], eps=rl.EPS), v.make_return_norm(gamma=case["gamma"], eps=rl.EPS)
    install(one, N, carry=carry0)
    install(two, N, carry=carry0)
    one.update_device(T, whole.ptr, d_mask=d_mask)
    two.update_device(8, first.ptr, d_mask=d_mask)
    mid = parts(two)
    w1 = rl.update([0.0, 0.0, 0.0], 1.0, a["carry"], a["reward"][:8], a["done"][:8], case["gamma"], rl.EPS, a["mask"])
    check_update(mid, w1, a["mask"], carry0, (name, "first half"))
    two.update_device(T - 8, second.ptr, d_mask=d_mask)
    got1, got2 = parts(one), parts(two)
    assert np.array_equal(rl.bits(got1[2]), rl.bits(got2[2])), "the carry"
    assert got1[0][0] == got2[0][0] == T * int(w1["live"].sum()), "n"
    w2 = rl.update(mid[0], mid[1], w1["carry"], a["reward"][8:], a["done"][8:], case["gamma"], rl.EPS, a["mask"])
    assert np.array_equal(rl.bits(got2[2])[w1["live"]], rl.bits(w2["carry"])[w1["live"]])
    within_bounds(got2[0], mid[0], w2["g"], w2["live"], (name, "second half"))
    # and the two roads meet within the same bounds of each other's definition
    within_bounds(got1[0], [0.0, 0.0, 0.0], rl.update([0.0] * 3, 1.0, a["carry"], a["reward"], a["done"], case["gamma"], rl.EPS, a["mask"])["g"],
                  w1["live"], (name, "whole"))
    close_all(one, two, whole, first, second, *([] if mask is None else [mask]))


def test_three_successive_updates_on_random_floats():
    rs = np.random.RandomState(17)
    N, T = 513, 17
    v = handle(N)
    rn = v.make_return_norm(gamma=0.99, eps=rl.EPS)
    state, scale, carry = np.zeros(3), F32(1.0), None
    for it in range(3):
        reward = (rs.normal(size=(T, N)) * 300.0 + 40.0).astype(F32)
        done = rs.rand(T, N) < 0.1
        packed = dbuf(rl.packed_of(reward, done, v.obs_dim, seed=it))
        rn.update_device(T, packed.ptr)
        got = parts(rn)
        want = rl.update(state, scale, carry, reward, done, 0.99, rl.EPS)
        assert np.array_equal(rl.bits(got[2]), rl.bits(want["carry"])), (it, "the carry is f32 arithmetic: on bits")
        within_bounds(got[0], state, want["g"], want["live"], ("random floats", it))
        assert rl.bits(F32(got[1])) == rl.bits(rl.scale_of(got[0][0], got[0][2], rl.EPS)), "the scale follows from the state the device holds"
        state, scale, carry = got  # (the next call's definition starts from what the device holds)
        packed.free()
    rn.close()


# ---- 3. the scale's edge cases
def test_a_constant_reward_and_a_nan_reward():
    N, T = 257, 9
    v = handle(N)
    D = v.obs_dim
    rn = v.make_return_norm(gamma=0.0, eps=1e-4, clip=10.0)
    reward, done = np.full((T, N), 2.5, dtype=F32), np.zeros((T, N), dtype=bool)
    packed = dbuf(rl.packed_of(reward, done, D))
    rn.update_device(T, packed.ptr)
    st, sc, c = parts(rn)
    assert st[0] == T * N and st[1] == 2.5 and rl.bits(st)[2] == 0, "a constant: M2 == 0 exactly"
    assert rl.bits(F32(sc)) == rl.bits(F32(F64(1.0) / np.sqrt(F64(1e-4)))), "scale32 == (float) (1 / sqrt(eps))"
    # a NaN reward: NaN in the state, and a NaN -- not +-clip -- in the advantage of its step
    rn.reset_device()
    reward = (np.arange(T * N).reshape(T, N) % 7).astype(F32)
    reward[3, 100] = np.nan
    done[3, 100] = True
    packed2 = dbuf(rl.packed_of(reward, done, D))
    rn.update_device(T, packed2.ptr)
    st, sc, c = parts(rn)
    assert st[0] == T * N and np.isnan(st[1]) and np.isnan(st[2]) and np.isnan(sc)
    assert c[100] == 0.0 and np.isfinite(np.delete(c, 100)).all(), "the NaN was counted, then done zeroed it: it does not travel in the carry"
    install(rn, N, state=(4.0, 0.0, 4.0), scale=1e4)
    values = dbuf(np.zeros((T + 1, N), dtype=F32))
    adv = dbuf(np.full((T, N), CANARY, dtype=np.uint32))
    rn.gae_device(T, packed2.ptr, values.ptr, adv.ptr, gamma=0.0, lam=0.0)
    v.sync()
    got = f32_of(adv.to_host(np.uint32, (T, N)))
    assert np.isnan(got[3, 100]) and rl.bits(got[3:4, 100])[0] != CANARY
    ok = np.ones((T, N), dtype=bool)
    ok[:4, 100] = False  # (and the steps before it: 0 * NaN is NaN, so the recurrence carries it back to t = 0)
    assert np.isnan(got[:4, 100]).all()
    assert np.array_equal(got[ok], np.where(reward[ok] > 0, F32(10.0), F32(0.0))), "every other step: 1e4 r clipped to 10"
    close_all(rn, packed, packed2, values, adv)


# ---- 4. the scaled GAE
SCALES = (1.0, 0.5, 3.0, 1e4)


class Gae(object):
    """a made case's blocks, values and outputs in device memory, outputs canary-filled"""

    def __init__(self, case, a, with_final=True, with_ret=True, seed=0):
        self.v = v = handle(case["N"])
        self.T, self.N = T, N = case["T"], case["N"]
        rs = np.random.RandomState(70 + seed)
        self.values = (rs.normal(size=(T + 1, N)) * 3.0).astype(F32)
        self.final = (rs.normal(size=N) * 3.0).astype(F32) if with_final else None
        self.a = a
        self.d = dict(packed=dbuf(rl.packed_of(a["reward"], a["done"], v.obs_dim)), values=dbuf(self.values),
                      adv=dbuf(np.full((T, N), CANARY, dtype=np.uint32)), stats=dbuf(np.full(3, CANARY_F64, dtype=np.uint64)))
        if with_final:
            self.d["final"] = dbuf(self.final)
        if with_ret:
            self.d["ret"] = dbuf(np.full((T, N), CANARY, dtype=np.uint32))
        if a["mask"] is not None:
            self.d["mask"] = dbuf(a["mask"])

    def run(self, call, gamma, lam, stats=True, stream=0):
        p = lambda k: self.d[k].ptr if k in self.d else 0
        call(self.T, p("packed"), p("values"), p("adv"), d_ret=p("ret"), d_final_values=p("final"), gamma=gamma, lam=lam, d_mask=p("mask"),
             d_stats=p("stats") if stats else 0, stream=stream)

    def read(self):
        self.v.sync()
        return dict(adv=self.d["adv"].to_host(np.uint32, (self.T, self.N)),
                    ret=self.d["ret"].to_host(np.uint32, (self.T, self.N)) if "ret" in self.d else None, stats=self.d["stats"].to_host(np.uint64, (3,)))

    def refill(self):
        for k in ("adv", "ret"):
            if k in self.d:
                self.d[k].from_host(np.full((self.T, self.N), CANARY, dtype=np.uint32))
        self.d["stats"].from_host(np.full(3, CANARY_F64, dtype=np.uint64))

    def check(self, got, scale, clip, gamma, lam, what):
        a = self.a
        adv, ret, st = rl.scaled_gae(a["reward"], a["done"], self.values, self.final, gamma, lam, scale, clip, a["mask"])
        live = np.ones(self.N, dtype=bool) if a["mask"] is None else a["mask"] != 0
        for name, want in (("adv", adv), ("ret", ret)):
            if got[name] is None:
                continue
            bad = np.nonzero(got[name][:, live] != rl.bits(want)[:, live])
            assert bad[0].size == 0, (what, name, "first (t, live env)", [int(x[0]) for x in bad], bad[0].size)
            assert (got[name][:, ~live] == CANARY).all(), (what, name, "a masked-out env's column was written")
        assert np.array_equal(got["stats"], rl.bits(st)), (what, "stats", got["stats"].view(F64), st)

    def free(self):
        close_all(*self.d.values())


@pytest.mark.parametrize("case", rl.CASES, ids=[c["name"] for c in rl.CASES])
def test_scaled_gae_equals_the_recurrence_fed_the_scaled_reward(case):
    """states set through set_state; the scale, the clip, the final values, d_ret and the mask alternate over the list"""
    i = rl.CASES.index(case)
    a = rl.case_arrays(case, carry=False, mask=i % 2 == 1)
    scale, clip = SCALES[i % 4], (10.0, 0.0, 2.0)[i % 3]
    m = Gae(case, a, with_final=i % 4 < 2, with_ret=i % 5 != 3, seed=i)
    rn = m.v.make_return_norm(gamma=0.99, eps=rl.EPS, clip=clip)
    install(rn, case["N"], state=(5.0, 1.0, 2.0), scale=scale)
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0)):
        m.refill()
        m.run(rn.gae_device, gamma, lam)
        m.check(m.read(), scale, clip, gamma, lam, (case["name"], scale, clip, gamma, lam))
    close_all(rn)
    m.free()


def test_rewards_that_land_on_the_clip_and_no_clip_at_all():
    case = rl.case_named("n513-t9-random-g05")
    a = rl.case_arrays(case)
    m = Gae(case, a)
    r2 = rl.scaled_reward(a["reward"], 0.5, 2.0)
    assert (a["reward"] == 4.0).any() and (a["reward"] == -4.0).any() and (r2 == 2.0).any() and (r2 == -2.0).any(), "r' exactly on +clip and on -clip"
    for scale, clip in ((0.5, 2.0), (4.0, 2.0), (1e4, 0.0), (3.0, 0.0)):
        rn = m.v.make_return_norm(gamma=0.5, eps=rl.EPS, clip=clip)
        install(rn, case["N"], state=(5.0, 1.0, 2.0), scale=scale)
        m.refill()
        m.run(rn.gae_device, 0.99, 0.95)
        m.check(m.read(), scale, clip, 0.99, 0.95, (scale, clip))
        rn.close()
    m.free()


@pytest.mark.parametrize("name", ["n513-t17-edge-g1", "n257-t7-twice-g05", "n1-t1-none-g1"])
def test_scale_one_without_a_clip_is_the_unscaled_call_on_bits(name):
    case = rl.case_named(name)
    i = rl.CASES.index(case)
    a = rl.case_arrays(case, mask=i % 2 == 0)
    a["reward"] = (a["reward"] * F32(37.25) + F32(0.1)).astype(F32)  # (no longer halves: any float survives a product with 1.0f)
    m = Gae(case, a, with_final=i % 3 != 0, seed=i)
    rn = m.v.make_return_norm(gamma=0.99, eps=rl.EPS, clip=0.0)
    m.run(rn.gae_device, 0.99, 0.95)
    scaled = m.read()
    m.refill()
    m.run(m.v.gae_device, 0.99, 0.95)
    plain = m.read()
    for k in ("adv", "ret", "stats"):
        assert np.array_equal(scaled[k], plain[k]), (name, k)
    assert not (plain["stats"] == CANARY_F64).any()
    # and with no d_stats the stats block is not written
    m.refill()
    m.run(rn.gae_device, 0.99, 0.95, stats=False)
    again = m.read()
    assert np.array_equal(again["adv"], plain["adv"]) and (again["stats"] == CANARY_F64).all()
    close_all(rn)
    m.free()


# ---- 5. one recorded iteration
class Iteration(object):
    """collect (auto-reset, T = 20, hub [3, 2], N = 33, clocks 85, 80 and 15 by thirds), the critic's values, the update, the scaled GAE"""
    T, N = 20, 33

    def __init__(self):
        rs = np.random.RandomState(11)
        self.v = v = make("philox", [3, 2], self.N, seed=6)
        D, T, N = v.obs_dim, self.T, self.N
        self.pol = v.make_policy(gaussian_layers(rs, [D, 32, v.act_dim]))
        self.pol.set_exploration(77, np.array([-0.5, 0.0], dtype=F32))
        self.crit = v.make_critic(gaussian_layers(rs, [D, 16, 1]), max_rows=(T + 1) * N)
        self.r = RollSet(v, self.pol, T)
        stagger(v, self.r)
        self.rn = v.make_return_norm(gamma=0.99, eps=rl.EPS, clip=10.0)
        mg = buffers()
        self.values, self.final = mg.DeviceBuffer((T + 1) * N * 4), mg.DeviceBuffer(N * 4)
        self.adv, self.ret, self.stats = mg.DeviceBuffer(T * N * 4), mg.DeviceBuffer(T * N * 4), mg.DeviceBuffer(24)

    def run(self, stream=0):
        v, r, T, N, D = self.v, self.r, self.T, self.N, self.v.obs_dim
        r.collect_set("autoreset", "decidable", stream=stream)
        self.crit.values_device(N, N, r.ptr("obs0"), self.values.ptr, ld=D, stream=stream)
        self.crit.values_device(T * N, T * N, r.ptr("packed"), self.values.ptr + 4 * N, ld=D + 2, stream=stream)
        self.crit.values_device(N, N, r.ptr("final"), self.final.ptr, ld=D, stream=stream)
        self.rn.update_device(T, r.ptr("packed"), stream=stream)
        self.rn.gae_device(T, r.ptr("packed"), self.values.ptr, self.adv.ptr, d_ret=self.ret.ptr, d_final_values=self.final.ptr, d_stats=self.stats.ptr,
                           stream=stream)

    def snapshot(self):
        self.v.sync()
        T, N = self.T, self.N
        return dict(blob=np.frombuffer(self.rn.get_state(), dtype=np.uint8).copy(), adv=self.adv.to_host(np.uint32, (T, N)),
                    ret=self.ret.to_host(np.uint32, (T, N)), stats=self.stats.to_host(np.uint64, (3,)), packed=self.r.host()["packed"],
                    values=self.values.to_host(np.uint32, (T + 1, N)), final=self.final.to_host(np.uint32, (N,)))

    def free(self):
        close_all(self.rn, self.values, self.final, self.adv, self.ret, self.stats, self.r, self.crit, self.pol, self.v)


def test_a_recorded_iteration_replays_as_eager_ones():
    """recorded on a created stream (a recording runs nothing) and replayed three times, against three eager iterations on a twin.  The
    envs move on, so every rollout is its own -- and every replay's advantages are scaled by the scale of ITS rollout's update"""
    mg = buffers()
    a, b = Iteration(), Iteration()
    st = mg.Stream(0)
    eager = []
    for it in range(3):
        a.run(stream=st.ptr)
        st.sync()
        eager.append(a.snapshot())
    before = b.snapshot()
    b.v.graph_begin(st.ptr)
    b.run(stream=st.ptr)
    for call in (lambda: b.v.make_return_norm(), b.rn.get_state, lambda: b.rn.set_state(before["blob"].tobytes()), b.rn.close):
        with pytest.raises(_lib.ChubError, match="chub_graph_begin and chub_graph_end"):
            call()
    graph = b.v.graph_end(st.ptr)
    st.sync()
    after = b.snapshot()
    assert all(np.array_equal(before[k], after[k]) for k in before), "a recording runs nothing"
    for it in range(3):
        b.v.graph_launch(graph, st.ptr)
        st.sync()
        got = b.snapshot()
        for k in got:
            assert np.array_equal(got[k], eager[it][k]), ("replay", it, k)
    # each iteration against the definition: the state within 6.21's bounds from the state before it, the carry and the advantages on bits
    D = a.v.obs_dim
    state, scale, carry, scales, dones = np.zeros(3), F32(1.0), None, [], []
    for it in range(3):
        packed = f32_of(eager[it]["packed"])
        reward, done = packed[:, :, D], packed[:, :, D + 1] != 0
        magic, N, got_state, got_scale, got_carry = rl.blob_parts(eager[it]["blob"].tobytes())
        want = rl.update(state, scale, carry, reward, done, 0.99, rl.EPS)
        assert np.array_equal(rl.bits(got_carry), rl.bits(want["carry"])), it
        within_bounds(got_state, state, want["g"], want["live"], ("iteration", it))
        assert rl.bits(F32(got_scale)) == rl.bits(rl.scale_of(got_state[0], got_state[2], rl.EPS))
        adv, ret, stats = rl.scaled_gae(reward, done, f32_of(eager[it]["values"]), f32_of(eager[it]["final"]), 0.99, 0.95, got_scale, 10.0)
        assert np.array_equal(eager[it]["adv"], rl.bits(adv)) and np.array_equal(eager[it]["ret"], rl.bits(ret)), (it, "scaled by its own rollout's scale")
        assert np.array_equal(eager[it]["stats"], rl.bits(stats))
        state, scale, carry = got_state, got_scale, got_carry
        scales.append(float(got_scale))
        dones.append(int(done.sum()))
    assert len(set(scales)) == 3 and dones[0] > 0, (scales, dones)
    b.v.graph_destroy(graph)
    a.free()
    b.free()
    st.destroy()


# ---- 6. the checkpoint
def test_the_state_blob_round_trips_and_another_n_is_refused():
    case = rl.case_named("n257-t17-twice-g1")
    a = rl.case_arrays(case, carry=True)
    N, T = case["N"], case["T"]
    v, w = handle(N), handle(255)
    rn, twin, other = v.make_return_norm(gamma=1.0), v.make_return_norm(gamma=1.0), w.make_return_norm(gamma=1.0)
    packed = dbuf(rl.packed_of(a["reward"], a["done"], v.obs_dim))
    install(rn, N, carry=a["carry"])
    rn.update_device(T, packed.ptr)
    blob = rn.get_state()
    assert len(blob) == rl.BLOB_HEAD + 4 * N and rl.blob_parts(blob)[:2] == (rl.MAGIC, N)
    twin.set_state(blob)
    assert twin.get_state() == blob, "identical bits round trip"
    # the twin goes on as the original does
    rn.update_device(T, packed.ptr)
    twin.update_device(T, packed.ptr)
    assert twin.get_state() == rn.get_state() and twin.get_state() != blob
    kept = other.get_state()
    with pytest.raises(_lib.ChubError, match="another N"):
        other.set_state(blob)
    bad = bytearray(blob)
    bad[0] ^= 1
    with pytest.raises(_lib.ChubError, match="magic"):
        twin.set_state(bytes(bad))
    with pytest.raises(ValueError):
        twin.set_state(blob[:-4])
    with pytest.raises(ValueError):
        twin.set_state(b"\0" * 8)
    assert other.get_state() == kept and twin.get_state() == rn.get_state(), "a refused blob writes nothing"
    close_all(rn, twin, other, packed)


# ---- 7. the torch adapter, in a child process that imports torch first
TORCH_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["CHUB_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHUB_ROOT"], "tests"))
import torch  # before libchub: both must share one HIP runtime
torch.cuda.set_device(0)
import test_gpu_return_norm
getattr(test_gpu_return_norm, os.environ["CHUB_CHILD"])()
print("TORCH_RETURN_NORM_OK")
"""


def test_the_adapters_methods_equal_the_c_calls():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], env=dict(os.environ, CHUB_ROOT=root, CHUB_CHILD="adapter_methods"), capture_output=True,
                       text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "TORCH_RETURN_NORM_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def adapter_methods():
    """make_reward_normalizer, update_reward_normalizer, advantages(reward_norm=) and reward_scale on one adapter against the restatement fed
    the adapter's own rollout; advantages without a normaliser is the path it was"""
    import torch
    from charginghub_env_amd import wrappers
    kw = {k: BASE[k] for k in BASE if k != "station_type_list"}
    T, N = 12, 40
    rs = np.random.RandomState(5)
    layers = gaussian_layers(rs, [13, 32, 47])
    envs = []
    for _ in range(2):
        env = wrappers.TorchHubVecEnv(N, [20, 25], ["fast", "slow"], seed=13, rng="philox", autoreset="per_env", **kw)
        pol = env.load_policy(layers)
        pol.set_exploration(9, np.array([-0.3, 0.2], dtype=F32))
        env.reset()
        for _ in range(90):  # (a day's end inside the rollout)
            env.step(torch.zeros((N, env.act_dim), device=env.device))
        envs.append((env, pol))
    (env, pol), (env2, pol2) = envs
    rn = env.make_reward_normalizer(gamma=0.98, eps=1e-6, clip=5.0)
    scale = env.reward_scale(rn)
    assert tuple(scale.shape) == (1,) and scale.dtype == torch.float32 and scale.data_ptr() == rn.scale_address and float(scale[0]) == 1.0
    host = lambda t: None if t is None else t.cpu().numpy()
    D = env.obs_dim
    state, sc, carry = np.zeros(3), F32(1.0), None
    for it, mask in enumerate((None, torch.arange(N, device=env.device) % 3 != 0)):
        ro = env.collect(pol, T, logp_piles="decidable")
        values, final = torch.randn((T + 1, N), device=env.device), torch.randn((N,), device=env.device)
        plain = [t.clone() for t in env.advantages(ro, values, final, gamma=0.98, lam=0.9, stats=True)]
        assert env.update_reward_normalizer(ro, rn, mask=mask) is rn
        adv, ret, stats = env.advantages(ro, values, final, gamma=0.98, lam=0.9, stats=True, reward_norm=rn)
        torch.cuda.synchronize()
        reward, done = host(ro["reward"]), host(ro["done"]) != 0
        assert it == 1 or done.any()
        want = rl.update(state, sc, carry, reward, done, 0.98, 1e-6, None if mask is None else host(mask).astype(np.uint8))
        st, got_sc, got_carry = rn.state(), rn.scale(), rn.carry()
        within_bounds(st, state, want["g"], want["live"], ("adapter", it))
        assert np.array_equal(rl.bits(got_carry), rl.bits(want["carry"])) and rl.bits(F32(got_sc)) == rl.bits(rl.scale_of(st[0], st[2], 1e-6))
        assert rl.bits(host(scale))[0] == rl.bits(F32(got_sc)), "the tensor is the object's word"
        a32, r32, s64 = rl.scaled_gae(reward, done, host(values), host(final), 0.98, 0.9, got_sc, 5.0)
        assert np.array_equal(rl.bits(host(adv)), rl.bits(a32)) and np.array_equal(rl.bits(host(ret)), rl.bits(r32))
        assert np.array_equal(rl.bits(host(stats)), rl.bits(s64))
        # the default path: chub_rollout_gae_device, as before
        a0, r0, s0 = rl.scaled_gae(reward, done, host(values), host(final), 0.98, 0.9, 1.0, 0.0)
        assert np.array_equal(rl.bits(host(plain[0])), rl.bits(a0)) and np.array_equal(rl.bits(host(plain[1])), rl.bits(r0))
        assert np.array_equal(rl.bits(host(plain[2])), rl.bits(s0)) and not np.array_equal(a0, a32)
        state, sc, carry = st, got_sc, got_carry
    ro2 = env2.collect(pol2, T, logp_piles="decidable")
    for call in (lambda: env2.update_reward_normalizer(ro2, rn), lambda: env2.reward_scale(rn),
                 lambda: env2.advantages(ro2, values, final, reward_norm=rn)):
        with pytest.raises(ValueError, match="another handle"):
            call()
    with pytest.raises(AssertionError):
        env.update_reward_normalizer(ro, rn, mask=torch.zeros((N + 1,), dtype=torch.bool, device=env.device))
    rn.close()
    env.close()
    env2.close()


# ---- 8. refusals and ownership
def test_every_refusal_leaves_the_outputs_untouched():
    case = rl.case_named("n255-t7-all-g05")
    a = rl.case_arrays(case, carry=True)
    m = Gae(case, a)
    v, N, T = m.v, case["N"], case["T"]
    nan, inf = float("nan"), float("inf")
    for text, kw in (("gamma", dict(gamma=1.5)), ("gamma", dict(gamma=-0.5)), ("gamma", dict(gamma=nan)), ("eps", dict(eps=0.0)), ("eps", dict(eps=-1.0)),
                     ("eps", dict(eps=inf)), ("eps", dict(eps=nan)), ("clip", dict(clip=-1.0)), ("clip", dict(clip=nan))):
        with pytest.raises(_lib.ChubError, match=text):
            v.make_return_norm(**kw)
    rn = v.make_return_norm(gamma=0.5, eps=rl.EPS, clip=2.0)
    install(rn, N, state=(9.0, 1.0, 4.0), scale=0.25, carry=a["carry"])
    before = rn.get_state()
    p = lambda k: m.d[k].ptr
    for text, call in (("null argument", lambda: rn.update_device(T, 0)), ("T >= 1", lambda: rn.update_device(0, p("packed"))),
                       ("T >= 1", lambda: rn.update_device(-3, p("packed"))),
                       ("are required", lambda: rn.gae_device(T, 0, p("values"), p("adv"))),
                       ("are required", lambda: rn.gae_device(T, p("packed"), 0, p("adv"))),
                       ("are required", lambda: rn.gae_device(T, p("packed"), p("values"), 0)),
                       ("T >= 1", lambda: rn.gae_device(0, p("packed"), p("values"), p("adv"))),
                       ("\\[0, 1\\]", lambda: rn.gae_device(T, p("packed"), p("values"), p("adv"), gamma=1.5)),
                       ("\\[0, 1\\]", lambda: rn.gae_device(T, p("packed"), p("values"), p("adv"), lam=-0.1)),
                       ("\\[0, 1\\]", lambda: rn.gae_device(T, p("packed"), p("values"), p("adv"), gamma=nan))):
        with pytest.raises(_lib.ChubError, match=text) as err:
            call()
        assert "error -1:" in str(err.value), (text, str(err.value))
    lib = _lib.load_library()
    assert lib.chub_return_norm_gae_device(rn._g, None, None) == -1 and lib.chub_return_norm_set_state(rn._g, None) == -1
    assert lib.chub_return_norm_get_state(rn._g, None) == -1 and lib.chub_return_norm_state_size(rn._g, None) == -1
    # a tape handle: create and every call on an object made before the handle became one
    t = make("philox", (2, 3), 8)
    early = t.make_return_norm()
    t.tape_register_soc(np.array([50.0], dtype=np.float32))  # a tape handle from here on
    small = dbuf(np.zeros((2, 8, t.obs_dim + 2), dtype=F32))
    for call in (t.make_return_norm, lambda: early.update_device(2, small.ptr), lambda: early.gae_device(2, small.ptr, small.ptr, small.ptr),
                 early.reset_carry_device, early.reset_device, early.get_state, lambda: early.set_state(b"\0" * 80)):
        with pytest.raises(_lib.ChubError, match="tape handle") as err:
            call()
        assert "error -4:" in str(err.value), str(err.value)
    got = m.read()
    assert (got["adv"] == CANARY).all() and (got["ret"] == CANARY).all() and (got["stats"] == CANARY_F64).all()
    assert rn.get_state() == before, "state, scale and carry keep their bits"
    close_all(early, small, t, rn)
    m.free()


def test_destroying_the_handle_takes_an_object_and_a_graph_in_its_stride():
    """chub_destroy with a chub_return_norm and a recorded graph alive: CHUB_OK, and a fresh handle works"""
    mg = buffers()
    lib = _lib.load_library()
    it = Iteration()
    st = mg.Stream(0)
    v = it.v
    v.graph_begin(st.ptr)
    it.run(stream=st.ptr)
    graph = v.graph_end(st.ptr)
    st.sync()
    more = v.make_return_norm(gamma=0.9)
    assert lib.chub_destroy(v._h) == 0, lib.chub_last_error()
    v._h = None  # (what v.close() does; the objects went with the handle, so their close() calls nothing)
    v.graph_destroy(graph)
    more.close()
    it.free()
    st.destroy()
    w = make("philox", (2, 3), 8)
    rn = w.make_return_norm()
    packed = dbuf(rl.packed_of(np.ones((3, 8), dtype=F32), np.zeros((3, 8), dtype=bool), w.obs_dim))
    rn.update_device(3, packed.ptr)
    assert rn.state()[0] == 24.0 and rn.scale() > 0
    close_all(rn, packed, w)
