"""Pile sets and advantages on the device (include/chub.h: chub_pile_set_device, chub_policy_sample_set_device, chub_policy_collect_set,
chub_rollout_gae_device), held to tests/pile_set_lib.py: (1) the sets against the pile columns of the same handle, in the three RNG modes,
under a device mask, after auto-reset steps and copies, in a replayed graph; (2) the step ignores every bit outside DECIDABLE; (3) the
set-aware sampled launch against the plain one and against the f64 sum over the set; (4) collect_set against collect and against the
calls one by one, eagerly and in a graph; (5) GAE bit for bit, its statistics, and end to end on a collected day; (6) every refusal;
(7) the torch adapter.  N = 70: two full env tiles of the actor and one of 6."""
import ctypes as C

import numpy as np
import pytest

import pile_set_lib as psl
import policy_lib as pl
import policy_sample_lib as ps
from charginghub_env_amd import _lib
from test_gpu_autoreset import Dev, buffers
from test_gpu_parity import hub
from test_gpu_pile_obs import BASE, CANARY, MODES, Driver, make
from test_gpu_policy import CANARY64, EXTRA, f32, gaussian_layers, same_state
from test_gpu_policy_sample import NAMES, Roll, Smp, close_all

pytestmark = pytest.mark.gpu

F32 = np.float32
N = psl.N_ENVS
WHICH = psl.PSET_NAMES
hub_id = lambda p: "%dx%d" % tuple(p) if isinstance(p, list) else str(p)


def lib_sets(v):
    """the three sets by the lib's definition from the car / emergency columns of the same handle"""
    cols = v.pile_obs(("car", "emergency"))
    return psl.sets_from_columns(cols[:, 0], cols[:, 1])


class SetBuf(object):
    """[N][W] u64 in device memory with words behind it that must keep the pattern"""

    def __init__(self, v):
        mg = buffers()
        self.v, self.words = v, v.n_envs * v.bit_words
        self.buf, self.mask = mg.DeviceBuffer((self.words + EXTRA) * 8), mg.DeviceBuffer(v.n_envs)

    def fill(self):
        self.buf.from_host(np.full(self.words + EXTRA, CANARY64, dtype=np.uint64))

    def read(self):
        raw = self.buf.to_host(np.uint64, (self.words + EXTRA,))
        assert (raw[self.words:] == CANARY64).all(), "the words past N * W"
        return raw[:self.words].reshape(self.v.n_envs, self.v.bit_words)

    def call(self, which, mask=None, stream=0):
        self.fill()
        if mask is not None:
            self.mask.from_host(np.ascontiguousarray(mask, dtype=np.uint8))
        self.v.sync()
        self.v.pile_set_device(self.buf.ptr, which, d_mask=self.mask.ptr if mask is not None else 0, stream=stream)
        self.v.sync()
        return self.read()

    def free(self):
        self.buf.free()
        self.mask.free()


def check_sets(v, sb, what, mask=None):
    want = lib_sets(v)
    for which in WHICH:
        got = sb.call(which, mask)
        w = psl.words(want[which])
        if mask is None:
            assert np.array_equal(got, w), (what, which, np.nonzero(got != w)[0][:5])
            assert np.array_equal(v.pile_set(which), want[which]), (what, which, "the host form")
        else:
            on = np.asarray(mask) != 0
            assert np.array_equal(got[on], w[on]) and (got[~on] == CANARY64).all(), (what, which, "under a mask")
    return want


# ---- 1. the sets
@pytest.mark.parametrize("piles", psl.HUBS, ids=hub_id)
@pytest.mark.parametrize("rng", MODES)
def test_sets_equal_the_definition_on_the_pile_columns(rng, piles):
    """right after a reset, several steps into the day and 60+ steps into it (forced-on cars), all envs and under a device mask; bits from
    S up are zero (the lib's words hold zeros there)"""
    v = make(rng, piles, N)
    d, sb = Driver(v, rng), SetBuf(v)
    d.reset()
    seen = {k: [] for k in WHICH}
    mask = np.arange(N) % 3 == 1
    mask_bytes = np.where(mask, 255, 0).astype(np.uint8)
    for t in range(67):
        if t in (0, 5, 60, 63, 66):
            want = check_sets(v, sb, (rng, piles, t))
            for k in WHICH:
                seen[k].append(want[k])
            if t in (5, 66):
                check_sets(v, sb, (rng, piles, t, "mask"), mask_bytes)
                check_sets(v, sb, (rng, piles, t, "empty mask"), np.zeros(N, dtype=np.uint8))
        d.step()
    psl.sets_differ({k: np.concatenate(x) for k, x in seen.items()}, need_forced_on=True)
    sb.free()
    v.close()


def test_sets_of_a_big_station_and_of_many_workgroups():
    """[300, 3]: a workgroup per env whose lanes stride over the piles, five words; 4099 x [20, 25]: 820 workgroups of five envs"""
    for piles, n in (([300, 3], 9), ([20, 25], 4099)):
        v = make("philox", piles, n)
        d, sb = Driver(v, "philox"), SetBuf(v)
        d.reset()
        for _ in range(8):
            d.step()
        want = check_sets(v, sb, (piles, n))
        psl.sets_differ(want)
        sb.free()
        v.close()


def test_sets_after_autoreset_steps_and_copies():
    """16 envs, 4 of them cloned in at another time of day: 97 auto-reset steps, so that the clones end their day at step 66 and the others
    at step 96 (the re-started envs show their new episode's sets)"""
    n = 16
    v, src = make("philox", [20, 25], n, seed=5), make("philox", [20, 25], n, seed=6)
    rs = np.random.RandomState(9)
    act = lambda: rs.uniform(-1, 1, size=(n, v.act_dim)).astype(F32)
    src.reset()
    for _ in range(30):
        src.step(act())
    v.reset()
    v.copy_envs([0, 1, 2, 3], [12, 13, 14, 15], source=src)
    sb, ss = SetBuf(v), SetBuf(src)
    for which in WHICH:
        assert np.array_equal(sb.call(which)[12:], ss.call(which)[:4]), "clones show their sources' sets"
    check_sets(v, sb, "after the copy")
    d = Dev(v)
    seen = {k: [] for k in WHICH}
    for t in range(1, 98):
        packed, _ = d.autoreset(act())
        done = packed[:, -1] > 0.5
        if done.any() or t % 8 == 0 or t == 97:
            want = check_sets(v, sb, ("auto-reset step", t))
            for k in WHICH:
                seen[k].append(want[k])
        if t == 66:
            assert done[12:].all() and not done[:12].any()
    psl.sets_differ({k: np.concatenate(x) for k, x in seen.items()}, need_forced_on=True)
    close_all(sb, ss, v, src)


def test_sets_recorded_into_a_graph_follow_the_state_and_take_no_tick():
    mg = buffers()
    n = 64
    ticks = []
    for with_calls in (True, False):
        v = make("philox", [40, 30], n, seed=77)
        st = mg.Stream(0)
        acts = [mg.DeviceBuffer(n * v.act_dim * 4) for _ in range(4)]
        for b, a in enumerate(acts):
            v.random_actions_device(a.ptr, 5, b, st.ptr)
        packed, obs0 = mg.DeviceBuffer(n * (v.obs_dim + 2) * 4), mg.DeviceBuffer(n * v.obs_dim * 4)
        outs = {which: SetBuf(v) for which in WHICH}
        for o in outs.values():
            o.fill()
        st.sync()
        v.graph_begin(st.ptr)
        for i in range(192):
            if i % 96 == 0:
                v.reset_device(obs0.ptr, stream=st.ptr)
            v.step_device_packed(acts[i % 4].ptr, packed.ptr, stream=st.ptr)
            if with_calls and i == 160:
                for which, o in outs.items():
                    v.pile_set_device(o.buf.ptr, which, stream=st.ptr)
        g = v.graph_end(st.ptr)
        if with_calls:
            assert all((o.read() == CANARY64).all() for o in outs.values())  # nothing ran while recording
        for replay in range(2):
            v.graph_launch(g, st.ptr)
            st.sync()
        ticks.append(v.env_clocks(ticks=True))
        if with_calls:  # the sets of the state 65 steps into the second day of the LAST replay: an eager twin that runs the same ticks
            w = make("philox", [40, 30], n, seed=77)
            packed_w = mg.DeviceBuffer(n * (w.obs_dim + 2) * 4)
            for i in range(192 + 161):
                if i % 96 == 0:
                    w.reset_device(obs0.ptr)
                w.step_device_packed(acts[i % 4].ptr, packed_w.ptr)
            w.sync()
            want = lib_sets(w)
            psl.sets_differ(want)
            for which, o in outs.items():
                assert np.array_equal(o.read(), psl.words(want[which])), ("replayed", which)
            packed_w.free()
            w.close()
        v.graph_destroy(g)
        close_all(*outs.values())
        v.close()
        st.destroy()
    assert np.array_equal(ticks[0][0], ticks[1][0]) and np.array_equal(ticks[0][1], ticks[1][1])


# ---- 2. the step ignores the complement
@pytest.mark.parametrize("piles", psl.HUBS, ids=hub_id)
@pytest.mark.parametrize("rng", ["philox", "philox_curves"])
def test_the_step_ignores_every_bit_outside_decidable(rng, piles):
    """two handles on the same seeds; 8 bits-form steps with B and with B XOR (random bits outside DECIDABLE), the set recomputed each step:
    four right after the reset (empty piles) and, 62 steps into the day, four more (forced-on cars): identical outputs and chub_get_slots
    state, bit for bit"""
    S = sum(piles)
    va, vb = make(rng, piles, N, seed=21), make(rng, piles, N, seed=21)
    da, db = Driver(va, rng), Driver(vb, rng)
    da.reset()
    db.reset()
    sb = SetBuf(va)
    rs = np.random.RandomState(31)
    seen = {k: [] for k in WHICH}
    for t in range(8):
        if t == 4:
            for _ in range(58):
                da.step()
                db.step()
        want = lib_sets(va)
        for k in WHICH:
            seen[k].append(want[k])
        dec = sb.call("decidable")
        assert np.array_equal(dec, psl.words(want["decidable"]))
        B = psl.words(rs.rand(N, S) < 0.5)
        flips = psl.words(rs.rand(N, S) < 0.5) & ~dec & psl.words(np.ones((N, S), dtype=bool))
        assert flips.any()
        tail = rs.uniform(-1, 1, size=(N, 2)).astype(F32)
        ra, rb = va.step_bits(B, tail), vb.step_bits(B ^ flips, tail)
        assert all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(ra[:3], rb[:3])), (rng, piles, "outputs", t)
        same_state(va, vb, (rng, piles, "state", t))
    psl.sets_differ({k: np.concatenate(x) for k, x in seen.items()}, need_forced_on=True)
    close_all(sb, va, vb)


# ---- 3. the set-aware sampled launch
class SmpSet(Smp):
    """Smp with a pile set: chub_policy_sample_set_device, the set into a buffer of its own"""

    def __init__(self, v, pol):
        Smp.__init__(self, v, pol)
        self.set = SetBuf(v)

    def call_set(self, piles, obs=None, mask=None, only=NAMES, own_set=True):
        if obs is not None:
            self.obs.from_host(np.ascontiguousarray(obs, dtype=F32))
        self.fill()
        self.set.fill()
        if mask is not None:
            self.mask.from_host(np.ascontiguousarray(mask, dtype=np.uint8))
        self.v.sync()
        p = {k: (self.buf[k].ptr if k in only else 0) for k in NAMES}
        self.pol.sample_device(self.obs.ptr, self.D, d_logp=p["logp"], d_actions=p["rows"], d_pile_bits=p["bits"], d_tail=p["tail"], d_u=p["u"],
                               d_features=p["feat"], d_mask=self.mask.ptr if mask is not None else 0, logp_piles=piles,
                               d_set_bits=self.set.buf.ptr if own_set else 0)
        self.v.sync()
        return self.read(), self.set.read()

    def free(self):
        Smp.free(self)
        self.set.free()


def steps_in(rng, piles, steps, seed=11):
    v = make(rng, piles, N, seed=seed)
    d = Driver(v, rng)
    d.reset()
    for _ in range(steps):
        d.step()
    return v


def sixty_four_steps_in(rng, piles, seed=11):
    return steps_in(rng, piles, 64, seed)


@pytest.mark.parametrize("piles", psl.HUBS, ids=hub_id)
@pytest.mark.parametrize("steps", [0, 64], ids=["after_the_reset", "64_steps_in"])
def test_sampling_with_a_set_changes_logp_alone(piles, steps):
    """right after the reset piles stand empty, 64 steps into the day cars are forced on (and the small hubs are full)"""
    S = sum(piles)
    v = steps_in("philox", piles, steps)
    layers, obs, ls = ps.general_case(piles, (64, 64))
    pol = v.make_policy(layers)
    pol.set_exploration(ps.KEY, ls)
    out, sb = SmpSet(v, pol), SetBuf(v)
    want = lib_sets(v)
    if steps == 0:
        psl.sets_differ(want)
    else:
        assert (want["occupied"] & ~want["decidable"]).any(), "no forced-on pile in this state"
    plain = out.call(obs)
    z, err = ps.pre_squash(obs, layers, "tanh")
    d = ps.Sample(z, err, "piles", S, ps.KEY, v.next_tick(), np.arange(N), ls)
    on = pl.unpack_bits(plain["bits"], S)
    mask = np.arange(N) % 3 != 0
    for which in WHICH:
        got, words = out.call_set(which, obs)
        assert np.array_equal(words, sb.call(which)) and np.array_equal(words, psl.words(want[which])), (which, "d_set_bits")
        for k in NAMES:
            if k != "logp" or which == "all":
                assert np.array_equal(got[k], plain[k]), (which, k, "bit for bit the plain sampled call's")
        value, bound = psl.masked_logp(d, on, want[which])
        lerr = np.abs(f32(got["logp"]).astype(np.float64) - value)
        print("%s %s: logp max error %.3g, worst error / bound %.3g, terms left out %d of %d" % (piles, which, lerr.max(), (lerr / bound).max(), (~want[which]).sum(), want[which].size))
        assert (lerr <= bound).all(), (which, "logp beyond its bound", lerr.max(), bound.max())
        again, words2 = out.call_set(which, obs)
        assert all(np.array_equal(got[k], again[k]) for k in NAMES) and np.array_equal(words, words2), (which, "two calls")
        scratch, untouched = out.call_set(which, obs, own_set=False)  # the set in the policy's own scratch
        assert all(np.array_equal(got[k], scratch[k]) for k in NAMES) and (untouched == CANARY64).all(), (which, "d_set_bits = NULL")
        m, mw = out.call_set(which, obs, mask=mask)
        for k in NAMES:
            canary = CANARY64 if k == "bits" else CANARY
            assert np.array_equal(m[k][mask], got[k][mask]) and (m[k][~mask] == canary).all(), (which, k, "under a mask")
        assert np.array_equal(mw[mask], words[mask]) and (mw[~mask] == CANARY64).all(), (which, "the set under a mask")
    if (~want["decidable"]).any():
        a, b = out.call_set("all", obs)[0], out.call_set("decidable", obs)[0]
        assert not np.array_equal(a["logp"], b["logp"])
    close_all(out, sb, pol, v)


def test_sampling_with_a_set_under_the_loads_head_and_in_the_curves_mode():
    piles = [20, 25]
    v = sixty_four_steps_in("philox_curves", piles)
    layers, obs, ls = ps.general_case(piles, (64, 64), "loads")
    pol = v.make_policy(layers, head="loads")
    pol.set_exploration(ps.KEY, ls)
    out = SmpSet(v, pol)
    plain = out.call(obs)
    got, words = out.call_set("all", obs)
    assert all(np.array_equal(got[k], plain[k]) for k in NAMES), "LOADS with ALL: the plain sampled call"
    assert np.array_equal(words, psl.words(np.ones((N, 45), dtype=bool)))
    layers, obs, ls = ps.general_case(piles, (64, 64))
    pp = v.make_policy(layers)
    pp.set_exploration(ps.KEY, ls)
    op = SmpSet(v, pp)
    want = lib_sets(v)
    plain = op.call(obs)
    got, words = op.call_set("decidable", obs)
    assert np.array_equal(words, psl.words(want["decidable"]))
    assert all(np.array_equal(got[k], plain[k]) for k in NAMES if k != "logp")
    z, err = ps.pre_squash(obs, layers, "tanh")
    d = ps.Sample(z, err, "piles", 45, ps.KEY, v.next_tick(), np.arange(N), ls)
    value, bound = psl.masked_logp(d, pl.unpack_bits(plain["bits"], 45), want["decidable"])
    assert (np.abs(f32(got["logp"]).astype(np.float64) - value) <= bound).all()
    close_all(out, op, pol, pp, v)


# ---- 4. collect_set
class RollSet(Roll):
    """Roll with the sets [T][N][W] kept"""

    def __init__(self, v, pol, T):
        Roll.__init__(self, v, pol, T)
        mg = buffers()
        self.shape["set"] = (T, v.n_envs, v.bit_words)
        self.buf["set"] = mg.DeviceBuffer(int(np.prod(self.shape["set"])) * 8)
        self.buf["set"].from_host(np.full(self.shape["set"], CANARY64, dtype=np.uint64))

    def ptr(self, k, t=0):
        return self.buf[k].ptr + t * int(np.prod(self.shape[k][1:])) * (8 if k in ("bits", "set") else 4)

    def host(self):
        self.v.sync()
        return {k: self.buf[k].to_host(np.uint64 if k in ("bits", "set") else np.uint32, s) for k, s in self.shape.items()}

    def collect_set(self, mode, which, first=0, T=None, stream=0):
        self.pol.collect(self.T if T is None else T, self.ptr("obs0"), self.ptr("packed"), self.ptr("bits"), self.ptr("tail"), self.ptr("u"),
                         self.ptr("logp"), d_features=self.ptr("feat"), d_final_obs=self.ptr("final") if mode == "autoreset" else 0,
                         first_step=first, mode=mode, stream=stream, logp_piles=which, d_set_bits=self.ptr("set"))

    def by_hand_set(self, mode, which, first=0, T=None, stream=0):
        """single chub_policy_sample_set_device calls interleaved with steps"""
        v, D = self.v, self.v.obs_dim
        if mode == "lockstep" and first % 96 == 0:
            v.reset_device(self.ptr("obs0"), stream=stream)
        for t in range(self.T if T is None else T):
            src, ld = (self.ptr("packed", t - 1), D + 2) if t else (self.ptr("obs0"), D)
            self.pol.sample_device(src, ld, d_logp=self.ptr("logp", t), d_actions=self.rows.ptr if mode == "autoreset" else 0,
                                   d_pile_bits=self.ptr("bits", t), d_tail=self.ptr("tail", t), d_u=self.ptr("u", t), d_features=self.ptr("feat", t),
                                   stream=stream, logp_piles=which, d_set_bits=self.ptr("set", t))
            if mode == "lockstep":
                v.step_bits_device_packed(self.ptr("bits", t), self.ptr("tail", t), self.ptr("packed", t), stream=stream)
            else:
                v.step_autoreset_device(self.rows.ptr, self.ptr("packed", t), self.ptr("final"), stream=stream)


def triplets(rng, piles, T, seed=6, key=77):
    rs = np.random.RandomState(29)
    vs = [make(rng, piles, N, seed=seed) for _ in range(3)]
    layers = gaussian_layers(rs, [vs[0].obs_dim, 64, 33, vs[0].act_dim])
    pols = [v.make_policy(layers) for v in vs]
    for p in pols:
        p.set_exploration(key, np.array([-0.5, 0.0], dtype=F32))
    return vs, pols, [RollSet(v, p, T) for v, p in zip(vs, pols)]


def compare(ra, rb, rc, which, T, what):
    """a: collect_set; b: collect on a twin; c: the set-aware calls one by one on a third"""
    ha, hb, hc = ra.host(), rb.host(), rc.host()
    cut = lambda h, k: h[k] if k in ("final", "obs0") else h[k][:T]
    for k in ha:
        if k not in ("logp", "set"):
            assert np.array_equal(cut(ha, k), cut(hb, k)), (what, k, "collect_set against collect")
        assert np.array_equal(cut(ha, k), cut(hc, k)), (what, k, "collect_set against the calls one by one")
    assert (hb["set"] == CANARY64).all()
    if which == "all":
        assert np.array_equal(cut(ha, "logp"), cut(hb, "logp"))
    else:
        assert not np.array_equal(cut(ha, "logp"), cut(hb, "logp"))
    return ha


@pytest.mark.parametrize("piles", [[20, 25], [40, 30], [0, 33]], ids=hub_id)
@pytest.mark.parametrize("mode", ["lockstep", "autoreset"])
def test_collect_set_mid_day(mode, piles):
    """ten plain collected steps from the reset on three handles, then T = 6 from step 10"""
    (va, vb, vc), pols, (ra, rb, rc) = triplets("philox", piles, 10)
    D, S = va.obs_dim, sum(piles)
    for v, r in ((va, ra), (vb, rb), (vc, rc)):
        if mode == "autoreset":
            v.reset_device(r.ptr("obs0"))
        r.collect(mode)
        last = r.host()["packed"][9, :, :D].copy()
        r.buf["obs0"].from_host(last)
    for which in ("decidable", "occupied", "all"):
        first = 10 if which == "decidable" else 16 if which == "occupied" else 22
        ra.collect_set(mode, which, first=first, T=6)
        rb.collect(mode, first=first, T=6)
        rc.by_hand_set(mode, which, first=first, T=6)
        h = compare(ra, rb, rc, which, 6, (mode, piles, which))
        same_state(va, vb, (mode, piles, which))
        same_state(va, vc, (mode, piles, which))
        assert (h["set"][6:] == CANARY64).all() and not (h["set"][:6] == CANARY64).any()
        if S % 64:
            assert (h["set"][:6, :, -1] >> np.uint64(S % 64) == 0).all(), "bits from S up are zero"
        for r in (ra, rb, rc):
            r.buf["obs0"].from_host(r.host()["packed"][5, :, :D].copy())
    close_all(ra, rb, rc, *pols, va, vb, vc)


@pytest.mark.parametrize("mode", ["lockstep", "autoreset"])
def test_collect_set_of_a_whole_day(mode):
    piles, T = [20, 25], 96
    (va, vb, vc), pols, (ra, rb, rc) = triplets("philox", piles, T)
    if mode == "autoreset":
        for v, r in ((va, ra), (vb, rb), (vc, rc)):
            v.reset_device(r.ptr("obs0"))
    ra.collect_set(mode, "decidable")
    rb.collect(mode)
    rc.by_hand_set(mode, "decidable")
    h = compare(ra, rb, rc, "decidable", T, (mode, "a day"))
    same_state(va, vb, (mode, "a day"))
    sets = pl.unpack_bits(h["set"].reshape(T * N, -1), 45).reshape(T, N, 45)
    assert not np.array_equal(sets[0], sets[40]) and not np.array_equal(sets[40], sets[41]), "the sets follow the state"
    D = va.obs_dim
    assert (f32(h["packed"])[T - 1, :, D + 1] == 1).all()
    close_all(ra, rb, rc, *pols, va, vb, vc)


def test_collect_set_in_a_graph_replayed_twice():
    """two lock-step days of collect_set recorded once and replayed twice: each replay equals an eager twin's run of the same ticks (new
    noise, and the sets of the states that noise leads to)"""
    mg = buffers()
    T = 96
    (va, vb, vc), pols, (ra, rb, rc) = triplets("philox", [20, 25], T)
    ra2, rb2 = RollSet(va, pols[0], T), RollSet(vb, pols[1], T)
    st = mg.Stream(0)
    ra.collect_set("lockstep", "decidable", stream=st.ptr)  # (to the clock the capture starts and ends at)
    rb.collect_set("lockstep", "decidable")
    st.sync()
    va.graph_begin(st.ptr)
    ra.collect_set("lockstep", "decidable", stream=st.ptr)
    ra2.collect_set("lockstep", "decidable", stream=st.ptr)
    graph = va.graph_end(st.ptr)
    st.sync()
    seen = []
    for replay in range(2):
        va.graph_launch(graph, st.ptr)
        rb.collect_set("lockstep", "decidable")
        rb2.collect_set("lockstep", "decidable")
        st.sync()
        for x, y, day in ((ra, rb, 1), (ra2, rb2, 2)):
            hx, hy = x.host(), y.host()
            for k in hx:
                assert np.array_equal(hx[k], hy[k]), ("replay", replay, "day", day, k)
        same_state(va, vb, ("replay", replay))
        seen.append(ra.host())
    assert not np.array_equal(seen[0]["bits"], seen[1]["bits"]) and not np.array_equal(seen[0]["set"], seen[1]["set"])
    assert not np.array_equal(seen[0]["logp"], seen[1]["logp"])
    va.graph_destroy(graph)
    close_all(ra, rb, rc, ra2, rb2, *pols, va, vb, vc)
    st.destroy()


# ---- 5. advantages
class Gae(object):
    """device buffers of chub_rollout_gae_device on a handle of N envs and D = 13"""

    def __init__(self, v, T):
        mg = buffers()
        n, D = v.n_envs, v.obs_dim
        self.v, self.T, self.n, self.D = v, T, n, D
        self.packed, self.values, self.final = mg.DeviceBuffer(T * n * (D + 2) * 4), mg.DeviceBuffer((T + 1) * n * 4), mg.DeviceBuffer(n * 4)
        self.adv, self.ret = mg.DeviceBuffer((T * n + EXTRA) * 4), mg.DeviceBuffer((T * n + EXTRA) * 4)
        self.stats, self.mask = mg.DeviceBuffer((3 + EXTRA) * 8), mg.DeviceBuffer(n)

    def call(self, packed, values, final, gamma, lam, ret=True, mask=None, stats=False):
        T, n = self.T, self.n
        self.packed.from_host(np.ascontiguousarray(packed, dtype=F32))
        self.values.from_host(np.ascontiguousarray(values, dtype=F32))
        if final is not None:
            self.final.from_host(np.ascontiguousarray(final, dtype=F32))
        if mask is not None:
            self.mask.from_host(np.ascontiguousarray(mask, dtype=np.uint8))
        for b in (self.adv, self.ret):
            b.from_host(np.full(T * n + EXTRA, CANARY, dtype=np.uint32))
        self.stats.from_host(np.full(3 + EXTRA, CANARY64, dtype=np.uint64))
        self.v.sync()
        self.v.gae_device(T, self.packed.ptr, self.values.ptr, self.adv.ptr, d_ret=self.ret.ptr if ret else 0,
                          d_final_values=self.final.ptr if final is not None else 0, gamma=gamma, lam=lam,
                          d_mask=self.mask.ptr if mask is not None else 0, d_stats=self.stats.ptr if stats else 0)
        self.v.sync()
        adv, rt, st = self.adv.to_host(np.uint32, (T * n + EXTRA,)), self.ret.to_host(np.uint32, (T * n + EXTRA,)), self.stats.to_host(np.uint64, (3 + EXTRA,))
        assert (adv[T * n:] == CANARY).all() and (rt[T * n:] == CANARY).all() and (st[3:] == CANARY64).all(), "the words past the outputs"
        return adv[:T * n].reshape(T, n), rt[:T * n].reshape(T, n), st[:3]

    def free(self):
        close_all(self.packed, self.values, self.final, self.adv, self.ret, self.stats, self.mask)


@pytest.fixture(scope="module")
def gae_handle():
    v = make("philox", [20, 25], N)
    yield v
    v.close()


@pytest.mark.parametrize("T", psl.GAE_T)
def test_gae_is_the_f32_definition_bit_for_bit(gae_handle, T):
    v = gae_handle
    g = Gae(v, T)
    D = v.obs_dim
    assert D == 13
    for dones in psl.GAE_DONES:
        for with_final in (False, True):
            packed, values, final = psl.gae_case(T, dones, with_final, D=D)
            for gamma, lam in psl.GAE_FACTORS:
                want_a, want_r = psl.gae_f32(packed[:, :, D], packed[:, :, D + 1], values, final, gamma, lam)
                adv, ret, st = g.call(packed, values, final, gamma, lam)
                what = (T, dones, with_final, gamma, lam)
                assert np.array_equal(adv, want_a.view(np.uint32)), (what, "adv", np.nonzero(adv != want_a.view(np.uint32))[0][:4])
                assert np.array_equal(ret, want_r.view(np.uint32)), (what, "ret")
                assert (st == CANARY64).all(), (what, "no statistics asked for")
            adv, ret, _ = g.call(packed, values, final, 0.99, 0.95, ret=False)
            assert np.array_equal(adv, psl.gae_f32(packed[:, :, D], packed[:, :, D + 1], values, final, 0.99, 0.95)[0].view(np.uint32))
            assert (ret == CANARY).all(), "d_ret = NULL"
            mask = np.where(np.arange(N) % 4 == 1, 7, 0).astype(np.uint8)
            adv_m, ret_m, _ = g.call(packed, values, final, 0.99, 0.95, mask=mask)
            on = mask != 0
            assert np.array_equal(adv_m[:, on], adv[:, on]) and (adv_m[:, ~on] == CANARY).all() and (ret_m[:, ~on] == CANARY).all(), "a device mask"
            assert not (ret_m[:, on] == CANARY).any()
    g.free()


def test_gae_statistics(gae_handle):
    import math
    v = gae_handle
    for T in (5, 96):
        g = Gae(v, T)
        packed, values, final = psl.gae_case(T, "last", True, D=v.obs_dim)
        for mask in (None, np.where(np.arange(N) % 4 != 1, 1, 0).astype(np.uint8)):
            adv, _, st = g.call(packed, values, final, 0.99, 0.95, mask=mask, stats=True)
            _, _, st2 = g.call(packed, values, final, 0.99, 0.95, mask=mask, stats=True)
            assert np.array_equal(st, st2), "two calls give identical bits"
            on = np.ones(N, dtype=bool) if mask is None else mask != 0
            x = f32(adv)[:, on]
            want, bound = psl.stats_of(x)
            got = st.view(np.float64)
            print("T %d: count %g, sum %.17g (fsum %.17g), squares %.17g (fsum %.17g)" % (T, got[0], got[1], want[1], got[2], want[2]))
            assert got[0] == want[0] == T * on.sum(), "the count is exact"
            assert abs(got[1] - want[1]) <= bound[1] and abs(got[2] - want[2]) <= bound[2], (got, want, bound)
            assert got[1] != 0 and math.isfinite(got[2])
        g.free()


def test_gae_end_to_end_on_a_collected_day_of_staggered_envs():
    """a third of the envs re-started 30 steps into the day and a third 61 steps into it, then an auto-reset collect_set of T = 96: done fires
    at three different steps; random values and final values; the device GAE of the recorded blocks equals the lib's, bit for bit"""
    mg = buffers()
    T, piles = 96, [20, 25]
    rs = np.random.RandomState(51)
    v = make("philox", piles, N, seed=9)
    D = v.obs_dim
    pol = v.make_policy(gaussian_layers(rs, [D, 64, 33, v.act_dim]))
    pol.set_exploration(5, np.array([-0.5, 0.0], dtype=F32))
    dv = Dev(v)
    r = RollSet(v, pol, T)
    v.reset_device(r.ptr("obs0"))
    group = np.arange(N) % 3
    for i in range(61):
        if i == 31:
            dv.reset_dmask(group == 1)
        dv.act.from_host(rs.uniform(-1, 1, size=(N, v.act_dim)).astype(F32))
        v.step_autoreset_device(dv.act.ptr, dv.packed.ptr, dv.final.ptr)
    dv.reset_dmask(group == 2)
    v.step_autoreset_device(dv.act.ptr, dv.packed.ptr, dv.final.ptr)
    v.sync()
    r.buf["obs0"].from_host(dv.packed.to_host(np.float32, (N, D + 2))[:, :D].copy())
    r.collect_set("autoreset", "decidable")
    h = r.host()
    packed = f32(h["packed"])
    done = packed[:, :, D + 1] != 0
    at = done.argmax(axis=0)
    assert (done.sum(axis=0) == 1).all() and len(set(at.tolist())) == 3, "every env ends its day once, at one of three steps"
    assert not (h["final"] == CANARY).any()
    values, final = (rs.normal(size=(T + 1, N)) * 4).astype(F32), (rs.normal(size=N) * 4).astype(F32)
    d_values, d_final = mg.DeviceBuffer((T + 1) * N * 4), mg.DeviceBuffer(N * 4)
    d_values.from_host(values)
    d_final.from_host(final)
    adv, ret, st = mg.DeviceBuffer(T * N * 4), mg.DeviceBuffer(T * N * 4), mg.DeviceBuffer(24)
    # (the rollout's own blocks, where the collect left them)
    v.gae_device(T, r.ptr("packed"), d_values.ptr, adv.ptr, d_ret=ret.ptr, d_final_values=d_final.ptr, gamma=0.99, lam=0.95, d_stats=st.ptr)
    v.sync()
    want_a, want_r = psl.gae_f32(packed[:, :, D], packed[:, :, D + 1], values, final, 0.99, 0.95)
    got_a = adv.to_host(np.float32, (T, N))
    assert np.array_equal(got_a.view(np.uint32), want_a.view(np.uint32)) and np.array_equal(ret.to_host(np.uint32, (T, N)), want_r.view(np.uint32))
    a64, _ = psl.gae_f64(packed[:, :, D], packed[:, :, D + 1], values, final, 0.99, 0.95)
    ba, _ = psl.gae_bound(packed[:, :, D], packed[:, :, D + 1], values, final, 0.99, 0.95, want_a, want_r)
    assert (np.abs(got_a.astype(np.float64) - a64) <= ba).all()
    want, bound = psl.stats_of(got_a)
    got = st.to_host(np.float64, (3,))
    assert got[0] == T * N and abs(got[1] - want[1]) <= bound[1] and abs(got[2] - want[2]) <= bound[2]
    close_all(d_values, d_final, adv, ret, st, r, pol, v)


# ---- 6. every refusal
def test_every_refusal_and_the_next_step_is_unchanged():
    n = 8
    rs = np.random.RandomState(43)
    v, twin, other = make("philox", [20, 25], n), make("philox", [20, 25], n), make("philox", [20, 25], n)
    for h in (v, twin):
        h.reset()
        h.step(np.zeros((n, h.act_dim), dtype=F32))
    D, A = v.obs_dim, v.act_dim
    lib = v._lib
    pol = v.make_policy(gaussian_layers(rs, [D, 16, A]))
    loads = v.make_policy(gaussian_layers(rs, [D, 16, 4]), head="loads")
    out, roll, sb = Smp(v, pol), RollSet(v, pol, 4), SetBuf(v)
    out.fill()
    sb.fill()
    tick = v.next_tick()

    def refused(code, text, rc):
        assert rc == code and text.encode() in lib.chub_last_error(), (rc, lib.chub_last_error())

    so = lambda **kw: _lib.ChubPolicySampleOut(**dict(dict(d_actions=out.buf["rows"].ptr, d_pile_bits=out.buf["bits"].ptr, d_tail=out.buf["tail"].ptr,
                                                             d_u=out.buf["u"].ptr, d_logp=out.buf["logp"].ptr, d_features=out.buf["feat"].ptr), **kw))
    sample = lambda h, p, obs, ld, which, o: lib.chub_policy_sample_set_device(h, p, obs, ld, None, which, sb.buf.ptr, C.byref(o) if o is not None else None, None)
    ro = lambda T=4, **kw: _lib.ChubRollout(**dict(dict(T=T, d_packed=roll.ptr("packed"), d_pile_bits=roll.ptr("bits"), d_tail=roll.ptr("tail"),
                                                        d_u=roll.ptr("u"), d_logp=roll.ptr("logp")), **kw))
    collect = lambda h, p, mode, which, r, sets, obs0, first: lib.chub_policy_collect_set(h, p, mode, which, C.byref(r), sets, obs0, first, None)
    # the pile set call
    refused(-1, "null argument", lib.chub_pile_set_device(None, 0, None, sb.buf.ptr, None))
    refused(-1, "null argument", lib.chub_pile_set_device(v._h, 0, None, None, None))
    for bad in (-1, 3, 99):
        refused(-1, "CHUB_PSET", lib.chub_pile_set_device(v._h, bad, None, sb.buf.ptr, None))
    # before set_exploration: what chub_policy_sample_device refuses
    refused(-1, "chub_policy_set_exploration first", sample(v._h, pol._p, out.obs.ptr, D, 2, so()))
    refused(-1, "chub_policy_set_exploration first", collect(v._h, pol._p, 1, 2, ro(), roll.ptr("set"), roll.ptr("obs0"), 0))
    pol.set_exploration(5, np.zeros(2, dtype=F32))
    loads.set_exploration(5, np.zeros(4, dtype=F32))
    for bad in (-1, 3):
        refused(-1, "CHUB_PSET", sample(v._h, pol._p, out.obs.ptr, D, bad, so()))
        refused(-1, "CHUB_PSET", collect(v._h, pol._p, 1, bad, ro(), roll.ptr("set"), roll.ptr("obs0"), 0))
    for which in (1, 2):
        refused(-1, "CHUB_PHEAD_LOADS", sample(v._h, loads._p, out.obs.ptr, D, which, so()))
        refused(-1, "CHUB_PHEAD_LOADS", collect(v._h, loads._p, 1, which, ro(), roll.ptr("set"), roll.ptr("obs0"), 0))
    refused(-1, "null argument", sample(None, pol._p, out.obs.ptr, D, 2, so()))
    refused(-1, "null argument", sample(v._h, pol._p, out.obs.ptr, D, 2, None))
    refused(-1, "null argument", sample(v._h, pol._p, None, D, 2, so()))
    refused(-1, "ld_obs", sample(v._h, pol._p, out.obs.ptr, D - 1, 2, so()))
    refused(-1, "made for another handle", sample(other._h, pol._p, out.obs.ptr, D, 2, so()))
    refused(-1, "d_logp is required", sample(v._h, pol._p, out.obs.ptr, D, 2, so(d_logp=None)))
    refused(-1, "pile bits need d_tail", sample(v._h, pol._p, out.obs.ptr, D, 2, so(d_tail=None)))
    refused(-1, "null argument", collect(v._h, pol._p, 1, 2, ro(), None, roll.ptr("obs0"), 0))
    refused(-1, "null argument", collect(v._h, pol._p, 1, 2, ro(), roll.ptr("set"), None, 0))
    refused(-1, "made for another handle", collect(other._h, pol._p, 1, 2, ro(), roll.ptr("set"), roll.ptr("obs0"), 0))
    refused(-1, "mode:", collect(v._h, pol._p, 2, 2, ro(), roll.ptr("set"), roll.ptr("obs0"), 0))
    for missing in ("d_packed", "d_pile_bits", "d_tail", "d_u", "d_logp"):
        refused(-1, "are required", collect(v._h, pol._p, 0, 2, ro(**{missing: None}), roll.ptr("set"), roll.ptr("obs0"), 1))
    refused(-1, "T >= 1", collect(v._h, pol._p, 0, 2, ro(T=0), roll.ptr("set"), roll.ptr("obs0"), 1))
    refused(-1, "inside one day", collect(v._h, pol._p, 0, 2, ro(T=96), roll.ptr("set"), roll.ptr("obs0"), 1))
    refused(-1, "T <= 96", collect(v._h, pol._p, 1, 2, ro(T=97), roll.ptr("set"), roll.ptr("obs0"), 0))
    # advantages
    f = roll.ptr("packed")
    good = dict(T=4, d_packed=f, d_values=f, d_final_values=None, d_mask=None, gamma=0.99, lam=0.95, d_adv=roll.ptr("feat"), d_ret=None, d_stats=None)
    gae = lambda **kw: C.byref(_lib.ChubGae(**dict(good, **kw)))
    refused(-1, "null argument", lib.chub_rollout_gae_device(None, gae(), None))
    refused(-1, "null argument", lib.chub_rollout_gae_device(v._h, None, None))
    for missing in ("d_packed", "d_values", "d_adv"):
        refused(-1, "are required", lib.chub_rollout_gae_device(v._h, gae(**{missing: None}), None))
    refused(-1, "T >= 1", lib.chub_rollout_gae_device(v._h, gae(T=0), None))
    for bad in (dict(gamma=-0.01), dict(gamma=1.01), dict(gamma=float("nan")), dict(lam=-0.5), dict(lam=1.5), dict(lam=float("nan"))):
        refused(-1, "[0, 1]", lib.chub_rollout_gae_device(v._h, gae(**bad), None))
    # nothing ran, nothing was written, and the handle's next step is the twin's
    assert v.next_tick() == tick
    v.sync()
    got = out.read()
    assert all((got[k] == (CANARY64 if k == "bits" else CANARY)).all() for k in NAMES) and (sb.read() == CANARY64).all(), "nothing written"
    h = roll.host()
    assert all((h[k] == (CANARY64 if k in ("bits", "set") else CANARY)).all() for k in h), "nothing written"
    act = rs.uniform(-1, 1, size=(n, A)).astype(F32)
    ra, rb = v.step(act), twin.step(act)
    assert all(np.array_equal(x, y) for x, y in zip(ra[:3], rb[:3]))
    same_state(v, twin, "after the refused calls")
    # COMPAT: collect_set is refused, the set and single set-aware evaluations are not
    c = make("compat", [3, 2], n)
    Driver(c, "compat").reset()
    pc = c.make_policy(gaussian_layers(rs, [c.obs_dim, c.act_dim]))
    pc.set_exploration(3, np.zeros(2, dtype=F32))
    oc, rc_ = SmpSet(c, pc), RollSet(c, pc, 4)
    r4 = _lib.ChubRollout(4, rc_.ptr("packed"), rc_.ptr("bits"), rc_.ptr("tail"), rc_.ptr("u"), rc_.ptr("logp"), None, None)
    refused(-4, "Philox modes", lib.chub_policy_collect_set(c._h, pc._p, 0, 2, C.byref(r4), rc_.ptr("set"), rc_.ptr("obs0"), 0, None))
    got, words = oc.call_set("occupied", np.zeros((n, c.obs_dim), dtype=F32))
    assert np.isfinite(f32(got["logp"])).all() and np.array_equal(words, psl.words(lib_sets(c)["occupied"]))
    # a tape handle: as chub_pile_obs_device
    t = make("philox", [20, 25], n)
    pt = t.make_policy(gaussian_layers(rs, [D, A]))
    pt.set_exploration(3, np.zeros(2, dtype=F32))
    t.tape_register_soc(np.array([50.0], dtype=F32))
    ot, st_ = Smp(t, pt), SetBuf(t)
    refused(-4, "tape handle", lib.chub_pile_set_device(t._h, 1, None, st_.buf.ptr, None))
    o4 = _lib.ChubPolicySampleOut(None, None, None, None, ot.buf["logp"].ptr, None)
    refused(-4, "tape handle", lib.chub_policy_sample_set_device(t._h, pt._p, ot.obs.ptr, D, None, 0, None, C.byref(o4), None))
    close_all(ot, st_, pt, t, oc, rc_, pc, c, out, roll, sb, pol, loads, v, twin, other)


# ---- 7. the torch adapter
TORCH_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["CHUB_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHUB_ROOT"], "tests"))
import torch  # before libchub: both must share one HIP runtime
torch.cuda.set_device(0)
import test_gpu_pile_set
test_gpu_pile_set.torch_adapter_sets_and_advantages()
print("TORCH_PILE_SET_OK")
"""


def test_torch_adapter_collect_with_a_set_advantages_and_sampled_logp():
    """in a child process that imports torch first (as tests/test_gpu_torch_side.py does)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], env=dict(os.environ, CHUB_ROOT=root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TORCH_PILE_SET_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def torch_adapter_sets_and_advantages():
    import torch
    from charginghub_env_amd import wrappers
    n, T = N, 6
    kw = {k: BASE[k] for k in BASE if k != "station_type_list"}
    torch.manual_seed(3)
    for autoreset in ("per_env", True):
        env = wrappers.TorchHubVecEnv(n, [20, 25], ["fast", "slow"], seed=13, autoreset=autoreset, **kw)
        D, A, S, W = env.obs_dim, env.act_dim, env.vec.n_slots, env.vec.bit_words
        net = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, 33), torch.nn.Tanh(), torch.nn.Linear(33, A)).to("cuda")
        critic = torch.nn.Sequential(torch.nn.Linear(D, 32), torch.nn.Tanh(), torch.nn.Linear(32, 1)).to("cuda")
        pol = env.load_policy(net)
        log_std = torch.tensor([-0.5, 0.1], device="cuda")
        pol.set_exploration(21, log_std.cpu().numpy())
        env.reset()
        plain = env.collect(pol, T)
        assert "set_bits" not in plain
        for _ in range(10):
            env.collect(pol, T)  # 66 steps into the day
        with pytest.raises(ValueError, match="unknown pile set"):
            env.collect(pol, T, logp_piles="empty")
        ro = env.collect(pol, T, logp_piles="decidable")
        assert ro is not plain and tuple(ro["set_bits"].shape) == (T, n, W) and ro["set_bits"].dtype == torch.int64
        sets = pl.unpack_bits(ro["set_bits"].cpu().numpy().view(np.uint64).reshape(T * n, W), S)
        assert sets.any() and not sets.all()
        # the recorded logp is the trainer's own forward on the features, over the recorded sets, within the lib's bound
        with torch.no_grad():
            z = net(ro["features"])
        new = wrappers.sampled_logp(z, ro["bits"], ro["u"], log_std, piles=ro["set_bits"])
        layers = [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in net if isinstance(m, torch.nn.Linear)]
        feats = ro["features"].cpu().numpy().reshape(T * n, D)
        z64, err = ps.pre_squash(feats, layers, "tanh")
        on = pl.unpack_bits(ro["bits"].cpu().numpy().view(np.uint64).reshape(T * n, W), S)
        u = ro["u"].cpu().numpy().reshape(T * n, 2).astype(np.float64)
        ref = psl.sampled_logp(z64, on, u, log_std.cpu().numpy(), sets)
        sigma = np.exp(log_std.cpu().numpy().astype(np.float64))
        eps = (u - z64[:, S:]) / sigma
        # (the bound of tests/test_gpu_policy_sample.py's adapter test, the pile part over the set)
        bound = np.where(sets, err[:, :S], 0.0).sum(axis=1) + (np.abs(eps) * (ps.U * np.abs(u) + err[:, S:]) / sigma * 1.01).sum(axis=1) \
            + pl.gamma(S + 2 + 8) * (np.abs(ref) + 50) + (S + 2) * 8 * ps.ULP
        rec = ro["logp"].cpu().numpy().reshape(T * n).astype(np.float64)
        assert (np.abs(rec - ref) <= bound).all(), (np.abs(rec - ref).max(), bound.max())
        ratio = torch.exp(new.reshape(T * n).cpu().double() - torch.tensor(rec))
        assert float((ratio - 1).abs().max()) < 1e-4, "an importance ratio of 1 at unchanged weights"
        full = wrappers.sampled_logp(z, ro["bits"], ro["u"], log_std)
        assert float((full - new).abs().max()) > 1e-2, "the terms of the other piles are not nothing"
        ent = wrappers.sampled_entropy(z, log_std, piles=ro["set_bits"])
        assert tuple(ent.shape) == (T, n) and bool(torch.isfinite(ent).all())
        # advantages: the lib's f32 recurrence, bit for bit
        with torch.no_grad():
            values = torch.cat([critic(ro["obs0"]).reshape(1, n), critic(ro["packed"][:, :, :D]).reshape(T, n)]).contiguous()
            final = critic(env.last_obs).reshape(n).contiguous() if autoreset == "per_env" else None
        adv, ret, st = env.advantages(ro, values, final, gamma=0.99, lam=0.95, stats=True)
        packed = ro["packed"].cpu().numpy()
        want_a, want_r = psl.gae_f32(packed[:, :, D], packed[:, :, D + 1], values.cpu().numpy(), None if final is None else final.cpu().numpy(), 0.99, 0.95)
        assert np.array_equal(adv.cpu().numpy().view(np.uint32), want_a.view(np.uint32)) and np.array_equal(ret.cpu().numpy().view(np.uint32), want_r.view(np.uint32))
        want, bound = psl.stats_of(want_a)
        got = st.cpu().numpy()
        assert got[0] == T * n and abs(got[1] - want[1]) <= bound[1] and abs(got[2] - want[2]) <= bound[2]
        adv2, ret2 = env.advantages(ro, values, final)
        assert adv2 is adv and ret2 is ret
        env.close()
