"""Sampling from the device actor (include/chub.h: chub_policy_set_exploration, chub_policy_sample_device, chub_policy_collect), held to
tests/policy_sample_lib.py's numpy definition: (1) on data whose z is bit-exact; (2) on general data within the bounds; (3) the law of the
draws; (4) what the noise depends on; (5) no trace in the simulation; (6) collect == the same calls one by one; (7) in a replayed graph;
(8) 65 536 envs once; (9) every refusal; (10) the torch adapter.  tests/test_policy_sample_cpu.py holds the definition alone to the same
caps on the same data."""
import ctypes as C

import numpy as np
import pytest

import policy_lib as pl
import policy_sample_lib as ps
from charginghub_env_amd import _lib
from test_gpu_autoreset import Dev, buffers
from test_gpu_parity import hub
from test_gpu_pile_obs import BASE, CANARY, make
from test_gpu_policy import CANARY64, EXTRA, f32, gaussian_layers, same_state

pytestmark = pytest.mark.gpu

F32 = np.float32
NAMES = ("rows", "bits", "tail", "u", "logp", "feat")


class Smp(object):
    """device buffers of one chub_policy_sample_device call on a handle, pattern-filled before every call"""

    def __init__(self, v, pol):
        mg = buffers()
        self.v, self.pol, self.n, self.D = v, pol, v.n_envs, v.obs_dim
        n = self.n
        self.words = dict(rows=n * v.act_dim, bits=n * v.bit_words, tail=n * 2, u=n * pol.n_gaussians, logp=n, feat=n * pol.n_features)
        self.shape = dict(rows=(n, v.act_dim), bits=(n, v.bit_words), tail=(n, 2), u=(n, pol.n_gaussians), logp=(n,), feat=(n, pol.n_features))
        self.buf = {k: mg.DeviceBuffer((w + EXTRA) * (8 if k == "bits" else 4)) for k, w in self.words.items()}
        self.obs, self.mask = mg.DeviceBuffer(n * self.D * 4), mg.DeviceBuffer(n)

    def fill(self):
        for k, w in self.words.items():
            self.buf[k].from_host(np.full(w + EXTRA, CANARY64 if k == "bits" else CANARY, dtype=np.uint64 if k == "bits" else np.uint32))

    def read(self):
        out = {}
        for k, w in self.words.items():
            raw = self.buf[k].to_host(np.uint64 if k == "bits" else np.uint32, (w + EXTRA,))
            assert (raw[w:] == (CANARY64 if k == "bits" else CANARY)).all(), ("the words past the output", k)
            out[k] = raw[:w].reshape(self.shape[k])
        return out

    def call(self, obs=None, mask=None, only=NAMES, stream=0):
        """-> {name: raw words} as the buffers stand after the call"""
        if obs is not None:
            self.obs.from_host(np.ascontiguousarray(obs, dtype=F32))
        self.fill()
        if mask is not None:
            self.mask.from_host(np.ascontiguousarray(mask, dtype=np.uint8))
        self.v.sync()
        p = {k: (self.buf[k].ptr if k in only else 0) for k in NAMES}
        self.pol.sample_device(self.obs.ptr, self.D, d_logp=p["logp"], d_actions=p["rows"], d_pile_bits=p["bits"], d_tail=p["tail"], d_u=p["u"],
                               d_features=p["feat"], d_mask=self.mask.ptr if mask is not None else 0, stream=stream)
        self.v.sync()
        return self.read()

    def free(self):
        for b in list(self.buf.values()) + [self.obs, self.mask]:
            b.free()


def hold_to_the_definition(got, d, head, S, squash, what, rows_are=None):
    """one sampled call's outputs against the definition d (ps.Sample) -> the share of undecided pile decisions as (count, total)"""
    u = f32(got["u"]).astype(np.float64)
    sigma = np.exp(d.log_std)
    err = np.abs(u - d.u)
    print("%s: u max error %.3g of bound %.3g" % (what, err.max(), d.bound_u.max()))
    assert (err <= d.bound_u).all(), (what, "u beyond its bound", err.max(), d.bound_u.max())
    eps = (u - d.zg) / sigma  # recovered
    assert (np.abs(eps - d.eps.astype(np.float64)) <= (d.bound_u + d.ezg) / sigma * 1.001).all(), (what, "eps recovered from u")
    tail, rows = f32(got["tail"]), f32(got["rows"])
    want_tail = ps.squash64(u[:, -2:], squash)
    if squash == "clip":
        assert np.array_equal(tail.astype(np.float64), want_tail), (what, "tail: the clip of the device's own u")
    else:
        assert (np.abs(tail - want_tail) <= pl.TANH_ERR).all(), (what, "tail: tanh of the device's own u")
    undecided = total = 0
    on = d.on
    if head == "piles":
        on = pl.unpack_bits(got["bits"], S)
        assert np.array_equal(on[d.decided], d.on[d.decided]), (what, "a pile decision the bound decides", np.nonzero((on != d.on) & d.decided)[0][:5])
        assert np.array_equal(rows[:, :S], np.where(on, F32(1), F32(-1))), (what, "pile rows are exactly +-1 and agree with the bits")
        assert np.array_equal(got["bits"], pl.pile_bits(rows, S)), (what, "bits from S up are zero")
        assert np.array_equal(got["rows"][:, S:], got["tail"]), (what, "the row's last two entries are the tail")
        undecided, total = int((~d.decided).sum()), d.decided.size
    elif rows_are is not None:
        assert np.array_equal(got["rows"], rows_are[0].view(np.uint32)) and np.array_equal(got["bits"], rows_are[1]), (what, "the dispatch of the loads")
    value, bound = d.logp(on)
    lerr = np.abs(f32(got["logp"]).astype(np.float64) - value)
    print("%s: logp max error %.3g, worst error / bound %.3g" % (what, lerr.max(), (lerr / bound).max()))
    assert (lerr <= bound).all(), (what, "logp beyond its bound", lerr.max(), bound.max())
    return undecided, total


# ---- 1. the definition on exact data
@pytest.mark.parametrize("piles", ps.EXACT_HUBS, ids=lambda p: "%dx%d" % tuple(p))
@pytest.mark.parametrize("head", ["piles", "loads"])
def test_exact_data_is_the_definition(piles, head):
    """relu / clip on dyadic data: z is bit-exact, so u differs from the definition by the roundings of the sample alone.  N = 70: a
    ragged last tile.  [64, 64]: two bit words, five output tiles."""
    n, S = ps.N_SMALL, sum(piles)
    layers, obs, ls = ps.exact_case(piles, head)
    v = make("philox", piles, n)
    pol = v.make_policy(layers, head=head, hidden_act="relu", squash="clip")
    pol.set_exploration(ps.KEY, ls)
    out = Smp(v, pol)
    z, err = ps.pre_squash(obs, layers, "relu")
    undecided = total = 0
    for moment in range(2):
        tick = v.next_tick()
        assert tick == 1 + moment
        d = ps.Sample(z, err, head, S, ps.KEY, tick, np.arange(n), ls)
        got = out.call(obs)
        assert np.array_equal(got["feat"], obs.view(np.uint32)), "the raw feature row, bit for bit"
        rows_are = None
        if head == "loads":  # clip is exact: the loads are the clip of the device's own u, dispatched as fractions
            uq = np.clip(f32(got["u"]), -1, 1)
            rows_are = v.load_dispatch(uq[:, :2], uq[:, 2:], units="fraction")
        a, b = hold_to_the_definition(got, d, head, S, "clip", (piles, head, moment), rows_are)
        undecided, total = undecided + a, total + b
        v.reset()  # (the tick moves: new noise)
    assert undecided <= 0.001 * total
    if piles == [20, 25] and head == "piles":  # the raw feature row of a policy that reads a feature block too
        rs = np.random.RandomState(3)
        wide = v.make_policy(pl.exact_layers(rs, [v.obs_dim + S, 33, S + 2]), inputs=("obs", ("pile_obs", ("car",))), hidden_act="relu", squash="clip",
                             normalize=(np.zeros(v.obs_dim + S, dtype=F32), np.full(v.obs_dim + S, 0.5, dtype=F32), 4.0))
        wide.set_exploration(1, ls)
        ow = Smp(v, wide)
        got = ow.call(obs)
        assert np.array_equal(got["feat"], pl.features([obs, v.pile_obs(("car",))]).view(np.uint32)), "raw blocks, before normalisation"
        ow.free()
        wide.close()
    out.free()
    pol.close()
    v.close()


# ---- 2. general data
@pytest.mark.parametrize("piles,hidden", ps.GENERAL, ids=["13-64-64-47", "13-33-33-4"])
@pytest.mark.parametrize("head", ["piles", "loads"])
def test_general_data_within_the_bounds_and_deterministic(piles, hidden, head):
    n, S = ps.N_SMALL, sum(piles)
    layers, obs, ls = ps.general_case(piles, hidden, head)
    v = make("philox", piles, n)
    pol = v.make_policy(layers, head=head)
    pol.set_exploration(ps.KEY, ls)
    out = Smp(v, pol)
    z, err = ps.pre_squash(obs, layers, "tanh")
    d = ps.Sample(z, err, head, S, ps.KEY, v.next_tick(), np.arange(n), ls)
    got = out.call(obs)
    undecided, total = hold_to_the_definition(got, d, head, S, "tanh", (piles, hidden, head))
    assert undecided <= 0.001 * total
    again = out.call(obs)
    assert all(np.array_equal(got[k], again[k]) for k in NAMES), "two sampled calls with no reset or step between them"
    out.free()
    pol.close()
    v.close()


# ---- 3. the law
def test_the_law_of_the_draws():
    n, S = ps.LAW_N, 45
    v = make("philox", [20, 25], n)
    layers = ps.law_layers(v.obs_dim, S)
    pol = v.make_policy(layers)
    pol.set_exploration(ps.LAW_KEY, np.asarray(ps.LAW_LOG_STD, dtype=F32))
    out = Smp(v, pol)
    assert v.next_tick() == 1
    got = out.call(np.zeros((n, v.obs_dim), dtype=F32))
    z = layers[0][1].astype(np.float64)
    eps = (f32(got["u"]).astype(np.float64) - z[S:]) / np.exp(np.asarray(ps.LAW_LOG_STD, dtype=F32).astype(np.float64))
    ps.check_law(pl.unpack_bits(got["bits"], S), eps, f32(got["logp"]), S)
    out.free()
    pol.close()
    v.close()


# ---- 4. what the noise depends on
def test_what_the_noise_depends_on():
    mg = buffers()
    piles, hidden = ps.GENERAL[0]
    layers, obs, ls = ps.general_case(piles, hidden)
    S = sum(piles)
    handles = [make("philox", piles, 70), make("philox", piles, 33), make("philox", piles, 38, env_id0=32)]
    pols = [h.make_policy(layers) for h in handles]
    for p in pols:
        p.set_exploration(ps.KEY, ls)
    outs = [Smp(h, p) for h, p in zip(handles, pols)]
    assert [h.next_tick() for h in handles] == [1, 1, 1]
    a, b, c = outs[0].call(obs), outs[1].call(obs[:33]), outs[2].call(obs[32:])
    for k in NAMES:
        assert np.array_equal(a[k][:33], b[k]), ("N = 70 and N = 33", k)
        assert np.array_equal(a[k][32:], c[k]), ("env_id0 = 32 over the same global ids", k)
    for name, mask in (("every third", np.arange(70) % 3 == 0), ("none", np.zeros(70, bool))):
        m = outs[0].call(obs, mask=mask)
        for k in NAMES:
            canary = CANARY64 if k == "bits" else CANARY
            assert np.array_equal(m[k][mask], a[k][mask]) and (m[k][~mask] == canary).all(), (name, k)
    # another key; another tick
    pols[1].set_exploration(ps.KEY + 1, ls)
    b2 = outs[1].call(obs[:33])
    assert not np.array_equal(b2["u"], b["u"]) and not np.array_equal(b2["bits"], b["bits"]) and np.array_equal(b2["feat"], b["feat"])
    handles[2].reset()
    handles[2].step(np.zeros((38, handles[2].act_dim), dtype=F32))
    assert handles[2].next_tick() == 3
    c2 = outs[2].call(obs[32:])
    assert not np.array_equal(c2["u"], c["u"]) and not np.array_equal(c2["bits"], c["bits"])
    # a new log_std from device memory: u - z scales by the ratio of the sigmas, the pile decisions do not move
    ls2 = (ls + F32(0.75)).astype(F32)
    dls = mg.DeviceBuffer(8)
    dls.from_host(ls2)
    pols[0].set_log_std_device(dls.ptr)
    a2 = outs[0].call(obs)
    z, err = ps.pre_squash(obs, layers, "tanh")
    d1 = ps.Sample(z, err, "piles", S, ps.KEY, 1, np.arange(70), ls)
    d2 = ps.Sample(z, err, "piles", S, ps.KEY, 1, np.arange(70), ls2)
    assert np.array_equal(a2["bits"], a["bits"])
    e1 = (f32(a["u"]).astype(np.float64) - d1.zg) / np.exp(d1.log_std)
    e2 = (f32(a2["u"]).astype(np.float64) - d2.zg) / np.exp(d2.log_std)
    assert (np.abs(e1 - e2) <= ((d1.bound_u + d1.ezg) / np.exp(d1.log_std) + (d2.bound_u + d2.ezg) / np.exp(d2.log_std)) * 1.001).all()
    assert (np.abs(f32(a2["u"]) - d2.u) <= d2.bound_u).all()
    dls.free()
    for o in outs:
        o.free()
    for p in pols:
        p.close()
    for h in handles:
        h.close()


# ---- 5. no trace
def test_sampling_leaves_no_trace():
    n = 40
    piles, hidden = ps.GENERAL[0]
    layers, obs, ls = ps.general_case(piles, hidden)
    obs = obs[:n]
    va, vb = make("philox", piles, n, seed=4), make("philox", piles, n, seed=4)
    pa, pb = va.make_policy(layers), vb.make_policy(layers)
    from test_gpu_policy import Act
    aa, ab = Act(va), Act(vb)
    before = aa.call(pa, obs)
    pa.set_exploration(9, ls)
    out = Smp(va, pa)
    va.reset()
    vb.reset()
    rs = np.random.RandomState(8)
    for i in range(6):
        out.call(obs)
        assert va.next_tick() == vb.next_tick() == 2 + i, "no tick is consumed"
        act = rs.uniform(-1, 1, size=(n, va.act_dim)).astype(F32)
        ra, rb = va.step(act), vb.step(act)
        assert all(np.array_equal(x, y) for x, y in zip(ra[:3], rb[:3])), ("a following step", i)
    same_state(va, vb, "after sampling between the steps")
    after, twin = aa.call(pa, obs), ab.call(pb, obs)
    assert all(np.array_equal(x, y) and np.array_equal(x, w) for x, y, w in zip(before, after, twin)), "chub_policy_act_device keeps its old bits"
    for x in (out, aa, ab):
        x.free()
    for x in (pa, pb):
        x.close()
    va.close()
    vb.close()


# ---- 6. collect == the same calls one by one
class Roll(object):
    """a rollout's arrays in device memory, pattern-filled"""

    def __init__(self, v, pol, T):
        mg = buffers()
        n, D, W, G, F = v.n_envs, v.obs_dim, v.bit_words, pol.n_gaussians, pol.n_features
        self.v, self.pol, self.T = v, pol, T
        self.shape = dict(packed=(T, n, D + 2), bits=(T, n, W), tail=(T, n, 2), u=(T, n, G), logp=(T, n), feat=(T, n, F), final=(n, D), obs0=(n, D))
        self.buf = {k: mg.DeviceBuffer(int(np.prod(s)) * (8 if k == "bits" else 4)) for k, s in self.shape.items()}
        for k, s in self.shape.items():
            self.buf[k].from_host(np.full(s, CANARY64 if k == "bits" else CANARY, dtype=np.uint64 if k == "bits" else np.uint32))
        self.rows = mg.DeviceBuffer(n * v.act_dim * 4)

    def ptr(self, k, t=0):
        return self.buf[k].ptr + t * int(np.prod(self.shape[k][1:])) * (8 if k == "bits" else 4)

    def collect(self, mode, first=0, T=None, stream=0):
        self.pol.collect(self.T if T is None else T, self.ptr("obs0"), self.ptr("packed"), self.ptr("bits"), self.ptr("tail"), self.ptr("u"),
                         self.ptr("logp"), d_features=self.ptr("feat"), d_final_obs=self.ptr("final") if mode == "autoreset" else 0,
                         first_step=first, mode=mode, stream=stream)

    def by_hand(self, mode, first=0, T=None, stream=0):
        """the calls chub_policy_collect documents, one by one"""
        v, D = self.v, self.v.obs_dim
        if mode == "lockstep" and first % 96 == 0:
            v.reset_device(self.ptr("obs0"), stream=stream)
        for t in range(self.T if T is None else T):
            src, ld = (self.ptr("packed", t - 1), D + 2) if t else (self.ptr("obs0"), D)
            self.pol.sample_device(src, ld, d_logp=self.ptr("logp", t), d_actions=self.rows.ptr if mode == "autoreset" else 0,
                                   d_pile_bits=self.ptr("bits", t), d_tail=self.ptr("tail", t), d_u=self.ptr("u", t), d_features=self.ptr("feat", t),
                                   stream=stream)
            if mode == "lockstep":
                v.step_bits_device_packed(self.ptr("bits", t), self.ptr("tail", t), self.ptr("packed", t), stream=stream)
            else:
                v.step_autoreset_device(self.rows.ptr, self.ptr("packed", t), self.ptr("final"), stream=stream)

    def host(self):
        self.v.sync()
        return {k: self.buf[k].to_host(np.uint64 if k == "bits" else np.uint32, s) for k, s in self.shape.items()}

    def free(self):
        for b in list(self.buf.values()) + [self.rows]:
            b.free()


def same_rollouts(a, b, what, T=None):
    ha, hb = a.host(), b.host()
    for k in ha:
        x, y = (ha[k], hb[k]) if T is None or k in ("final", "obs0") else (ha[k][:T], hb[k][:T])
        assert np.array_equal(x, y), (what, k, np.nonzero(x != y)[0][:4])
    return ha


def twins(rng, head, n, T, seed=6, key=77):
    piles = [20, 25]
    rs = np.random.RandomState(29)
    va, vb = make(rng, piles, n, seed=seed), make(rng, piles, n, seed=seed)
    layers = gaussian_layers(rs, [va.obs_dim, 64, 33, va.act_dim if head == "piles" else 4])
    pa, pb = va.make_policy(layers, head=head), vb.make_policy(layers, head=head)
    ls = np.array([-0.5, 0.0, -0.25, 0.1][:pa.n_gaussians], dtype=F32)
    for p in (pa, pb):
        p.set_exploration(key, ls)
    return va, vb, pa, pb, Roll(va, pa, T), Roll(vb, pb, T)


def close_all(*things):
    for x in things:
        (x.free if hasattr(x, "free") else x.close)()


@pytest.mark.parametrize("mode,head,rng", [("lockstep", "piles", "philox"), ("autoreset", "piles", "philox"), ("lockstep", "loads", "philox"),
                                           ("autoreset", "loads", "philox"), ("lockstep", "piles", "philox_curves")])
def test_collect_equals_the_same_calls_one_by_one(mode, head, rng):
    n, T = 40, 5
    va, vb, pa, pb, ra, rb = twins(rng, head, n, T)
    if mode == "autoreset":
        for v, r in ((va, ra), (vb, rb)):
            v.reset_device(r.ptr("obs0"))
    ra.collect(mode)
    rb.by_hand(mode)
    h = same_rollouts(ra, rb, (mode, head, rng))
    same_state(va, vb, (mode, head, rng))
    assert np.isfinite(f32(h["logp"])).all() and np.isfinite(f32(h["packed"])).all() and not (h["feat"] == CANARY).any()
    assert not np.array_equal(h["u"][0], h["u"][1]), "every step draws under its own tick"
    if mode == "lockstep":
        assert (h["final"] == CANARY).all()
    close_all(ra, rb, pa, pb, va, vb)


def test_collect_lockstep_to_the_end_of_a_day():
    """93 steps from a reset, then first_step = 93: T = 4 is refused with nothing written, T = 3 ends the day"""
    n = 40
    va, vb, pa, pb, ra, rb = twins("philox", "piles", n, 93)
    ra.collect("lockstep")
    rb.by_hand("lockstep")
    same_rollouts(ra, rb, "93 steps")
    last = {k: r.buf["packed"].to_host(np.uint32, r.shape["packed"])[92, :, :va.obs_dim].copy() for k, r in (("a", ra), ("b", rb))}
    for r, o in ((ra, last["a"]), (rb, last["b"])):
        r.buf["obs0"].from_host(o)  # (the observation the next call's first step acts on)
    lib = va._lib
    roll = _lib.ChubRollout(4, ra.ptr("packed"), ra.ptr("bits"), ra.ptr("tail"), ra.ptr("u"), ra.ptr("logp"), None, None)
    tick = va.next_tick()
    assert lib.chub_policy_collect(va._h, pa._p, 0, C.byref(roll), ra.ptr("obs0"), 93, None) == -1 and b"inside one day" in lib.chub_last_error()
    assert va.next_tick() == tick
    ra.collect("lockstep", first=93, T=3)
    rb.by_hand("lockstep", first=93, T=3)
    h = same_rollouts(ra, rb, "the day's last three steps", T=3)
    same_state(va, vb, "the day's end")
    D = va.obs_dim
    assert (f32(h["packed"])[2, :, D + 1] == 1).all() and (f32(h["packed"])[:2, :, D + 1] == 0).all(), "done fires in the 96th step"
    close_all(ra, rb, pa, pb, va, vb)


def test_collect_autoreset_across_the_end_of_an_episode():
    """half of the envs are re-started after 50 hand-issued steps; after 94, T = 4: done fires inside the rollout for the other half, whose
    final_obs rows hold the terminal observation; the rest keep their canaries"""
    n, T = 40, 4
    va, vb, pa, pb, ra, rb = twins("philox", "piles", n, T)
    late = np.arange(n) % 2 == 1
    rs = np.random.RandomState(12)
    for v, r in ((va, ra), (vb, rb)):
        dv = Dev(v)
        v.reset_device(r.ptr("obs0"))
        rs = np.random.RandomState(12)
        for i in range(94):
            if i == 50:
                dv.reset_dmask(late)
            dv.act.from_host(rs.uniform(-1, 1, size=(n, v.act_dim)).astype(F32))
            v.step_autoreset_device(dv.act.ptr, dv.packed.ptr, dv.final.ptr)
        v.sync()
        r.buf["obs0"].from_host(dv.packed.to_host(np.float32, (n, v.obs_dim + 2))[:, :v.obs_dim].copy())
    ra.collect("autoreset")
    rb.by_hand("autoreset")
    h = same_rollouts(ra, rb, "autoreset across an episode's end")
    same_state(va, vb, "autoreset across an episode's end")
    D = va.obs_dim
    done = f32(h["packed"])[:, :, D + 1] == 1
    assert done[1, ~late].all() and done.sum() == (~late).sum(), "the 96th step of the early half"
    assert (h["final"][late] == CANARY).all() and not (h["final"][~late] == CANARY).any()
    assert np.isfinite(f32(h["final"])[~late]).all()
    close_all(ra, rb, pa, pb, va, vb)


# ---- 7. graph
def test_a_captured_rollout_replays_with_new_noise_and_follows_set_log_std_device():
    """two lock-step days of collect recorded once (2 resets + 192 steps: even) and replayed twice: each replay equals an eager twin's run of
    the same ticks, the replays differ, and a set_log_std_device between them is followed"""
    mg = buffers()
    n, T = 40, 96
    va, vb, pa, pb, ra, rb = twins("philox", "piles", n, T)
    ra2, rb2 = Roll(va, pa, T), Roll(vb, pb, T)
    st = mg.Stream(0)
    ra.collect("lockstep", stream=st.ptr)  # (to the clock the capture starts and ends at)
    rb.collect("lockstep")
    st.sync()
    va.graph_begin(st.ptr)
    ra.collect("lockstep", stream=st.ptr)
    ra2.collect("lockstep", stream=st.ptr)
    with pytest.raises(hub().ChubError, match="chub_graph_begin and chub_graph_end"):
        pa.set_exploration(1, np.zeros(2, dtype=F32))
    graph = va.graph_end(st.ptr)
    st.sync()
    dls = mg.DeviceBuffer(8)
    dls.from_host(np.array([0.2, -0.9], dtype=F32))
    seen = []
    for replay in range(2):
        if replay == 1:
            pa.set_log_std_device(dls.ptr, stream=st.ptr)
            pb.set_log_std_device(dls.ptr)
        va.graph_launch(graph, st.ptr)
        rb.collect("lockstep")
        rb2.collect("lockstep")
        st.sync()
        h = same_rollouts(ra, rb, ("replay", replay, "day 1"))
        same_rollouts(ra2, rb2, ("replay", replay, "day 2"))
        same_state(va, vb, ("replay", replay))
        seen.append(h)
    assert not np.array_equal(seen[0]["bits"], seen[1]["bits"]) and not np.array_equal(seen[0]["u"], seen[1]["u"])
    va.graph_destroy(graph)
    close_all(ra, rb, ra2, rb2, dls, pa, pb, va, vb)
    st.destroy()


# ---- 8. 65 536 envs once
def test_65536_envs_once():
    n, S = 65536, 45
    rs = np.random.RandomState(41)
    v = make("philox", [20, 25], n)
    layers = pl.exact_layers(rs, [v.obs_dim, 64, 64, v.act_dim])
    obs = pl.exact_obs(rs, n, v.obs_dim)
    pl.assert_exact(obs, layers)
    ls = np.array([-0.5, 0.0], dtype=F32)
    pol = v.make_policy(layers, hidden_act="relu", squash="clip")
    pol.set_exploration(ps.KEY, ls)
    out = Smp(v, pol)
    got = out.call(obs, only=("bits", "tail", "u", "logp"))
    assert np.isfinite(f32(got["logp"])).all() and (got["rows"] == CANARY).all() and (got["feat"] == CANARY).all()
    sample = np.concatenate([[0, 31, 32, n - 1], rs.choice(n, size=64, replace=False)])
    z, err = ps.pre_squash(obs[sample], layers, "relu")
    d = ps.Sample(z, err, "piles", S, ps.KEY, 1, sample, ls)
    u = f32(got["u"])[sample].astype(np.float64)
    assert (np.abs(u - d.u) <= d.bound_u).all()
    on = pl.unpack_bits(got["bits"][sample], S)
    assert np.array_equal(on[d.decided], d.on[d.decided]) and (~d.decided).sum() <= 0.001 * d.decided.size
    value, bound = d.logp(on)
    assert (np.abs(f32(got["logp"])[sample] - value) <= bound).all()
    assert np.array_equal(f32(got["tail"])[sample].astype(np.float64), np.clip(u, -1, 1))
    out.free()
    pol.close()
    v.close()


# ---- 9. every refusal
def test_every_refusal():
    mg = buffers()
    n = 8
    rs = np.random.RandomState(43)
    v, other = make("philox", [20, 25], n), make("philox", [20, 25], n)
    D, A = v.obs_dim, v.act_dim
    layers = gaussian_layers(rs, [D, 16, A])
    pol = v.make_policy(layers)
    lib = v._lib
    out = Smp(v, pol)
    out.fill()
    roll = Roll(v, pol, 4)
    ls = np.zeros(2, dtype=F32)

    def refused(code, text, rc):
        assert rc == code and text.encode() in lib.chub_last_error(), (rc, lib.chub_last_error())

    so = lambda **kw: _lib.ChubPolicySampleOut(**dict(dict(d_actions=out.buf["rows"].ptr, d_pile_bits=out.buf["bits"].ptr, d_tail=out.buf["tail"].ptr,
                                                             d_u=out.buf["u"].ptr, d_logp=out.buf["logp"].ptr, d_features=out.buf["feat"].ptr), **kw))
    sample = lambda h, p, obs, ld, o: lib.chub_policy_sample_device(h, p, obs, ld, None, C.byref(o) if o is not None else None, None)
    ro = lambda T=4, **kw: _lib.ChubRollout(**dict(dict(T=T, d_packed=roll.ptr("packed"), d_pile_bits=roll.ptr("bits"), d_tail=roll.ptr("tail"),
                                                        d_u=roll.ptr("u"), d_logp=roll.ptr("logp")), **kw))
    collect = lambda h, p, mode, r, obs0, first: lib.chub_policy_collect(h, p, mode, C.byref(r) if r is not None else None, obs0, first, None)
    tick = C.c_uint32()
    refused(-1, "null argument", lib.chub_next_tick(None, C.byref(tick)))
    refused(-1, "null argument", lib.chub_next_tick(v._h, None))
    # before set_exploration
    refused(-1, "chub_policy_set_exploration first", sample(v._h, pol._p, out.obs.ptr, D, so()))
    refused(-1, "chub_policy_set_exploration first", lib.chub_policy_set_log_std_device(pol._p, out.buf["u"].ptr, None))
    refused(-1, "chub_policy_set_exploration first", collect(v._h, pol._p, 0, ro(), roll.ptr("obs0"), 0))
    refused(-1, "null argument", lib.chub_policy_set_exploration(None, 1, ls.ctypes.data))
    refused(-1, "null argument", lib.chub_policy_set_exploration(pol._p, 1, None))
    bad = np.array([0.0, np.nan], dtype=F32)
    refused(-1, "log_std[1] is not finite", lib.chub_policy_set_exploration(pol._p, 1, bad.ctypes.data))
    pol.set_exploration(5, ls)
    refused(-1, "null argument", lib.chub_policy_set_log_std_device(pol._p, None, None))
    refused(-1, "null argument", sample(None, pol._p, out.obs.ptr, D, so()))
    refused(-1, "null argument", sample(v._h, None, out.obs.ptr, D, so()))
    refused(-1, "null argument", sample(v._h, pol._p, out.obs.ptr, D, None))
    refused(-1, "null argument", sample(v._h, pol._p, None, D, so()))
    refused(-1, "ld_obs", sample(v._h, pol._p, out.obs.ptr, D - 1, so()))
    refused(-1, "made for another handle", sample(other._h, pol._p, out.obs.ptr, D, so()))
    refused(-1, "d_logp is required", sample(v._h, pol._p, out.obs.ptr, D, so(d_logp=None)))
    refused(-1, "pile bits need d_tail", sample(v._h, pol._p, out.obs.ptr, D, so(d_tail=None)))
    refused(-1, "null argument", collect(v._h, pol._p, 0, None, roll.ptr("obs0"), 0))
    refused(-1, "null argument", collect(v._h, pol._p, 0, ro(), None, 0))
    refused(-1, "made for another handle", collect(other._h, pol._p, 0, ro(), roll.ptr("obs0"), 0))
    refused(-1, "mode:", collect(v._h, pol._p, 2, ro(), roll.ptr("obs0"), 0))
    for missing in ("d_packed", "d_pile_bits", "d_tail", "d_u", "d_logp"):
        refused(-1, "are required", collect(v._h, pol._p, 0, ro(**{missing: None}), roll.ptr("obs0"), 0))
    refused(-1, "T >= 1", collect(v._h, pol._p, 0, ro(T=0), roll.ptr("obs0"), 0))
    refused(-1, "T >= 1", collect(v._h, pol._p, 0, ro(), roll.ptr("obs0"), -1))
    refused(-1, "inside one day", collect(v._h, pol._p, 0, ro(T=97), roll.ptr("obs0"), 0))
    refused(-1, "inside one day", collect(v._h, pol._p, 0, ro(T=2), roll.ptr("obs0"), 95 + 96))
    refused(-1, "T <= 96", collect(v._h, pol._p, 1, ro(T=97), roll.ptr("obs0"), 0))
    refused(-1, "step() before reset()", collect(v._h, pol._p, 1, ro(), roll.ptr("obs0"), 0))
    assert v.next_tick() == 1 and v.env_clocks(ticks=True)[1].max() == 0, "nothing ran"
    v.sync()
    got = out.read()
    assert all((got[k] == (CANARY64 if k == "bits" else CANARY)).all() for k in NAMES), "nothing written"
    h = roll.host()
    assert all((h[k] == (CANARY64 if k == "bits" else CANARY)).all() for k in h), "nothing written"
    # the sampled launch's LDS rule: images of 416 + 96 rows leave none of the 512 for the log-probability partials
    F = 9 * v.n_slots + 2 * 1 * 5
    full = v.make_policy(gaussian_layers(rs, [F, 96, A]), inputs=(("pile_obs", None), ("station_profile", ("cars",), 5)))
    assert full.n_features == 415
    refused(-4, "rows of LDS", lib.chub_policy_set_exploration(full._p, 1, ls.ctypes.data))
    fits = v.make_policy(gaussian_layers(rs, [F, 64, A]), inputs=(("pile_obs", None), ("station_profile", ("cars",), 5)))
    fits.set_exploration(1, ls)  # 416 + 64 + 4 rows
    # COMPAT: collect is refused, single sampled evaluations are not
    c = make("compat", [3, 2], n)
    pc = c.make_policy(gaussian_layers(rs, [c.obs_dim, c.act_dim]))
    pc.set_exploration(3, ls)
    oc, rc_ = Smp(c, pc), Roll(c, pc, 4)
    r4 = _lib.ChubRollout(4, rc_.ptr("packed"), rc_.ptr("bits"), rc_.ptr("tail"), rc_.ptr("u"), rc_.ptr("logp"), None, None)
    refused(-4, "Philox modes", lib.chub_policy_collect(c._h, pc._p, 0, C.byref(r4), rc_.ptr("obs0"), 0, None))
    assert np.isfinite(f32(oc.call(np.zeros((n, c.obs_dim), dtype=F32))["logp"])).all()
    # a tape handle: the tape rules of chub_policy_act_device
    t = make("philox", [20, 25], n)
    pt = t.make_policy(gaussian_layers(rs, [D, 4]), head="loads")
    pt.set_exploration(3, np.zeros(4, dtype=F32))
    t.tape_register_soc(np.array([50.0], dtype=F32))
    ot = Smp(t, pt)
    o4 = _lib.ChubPolicySampleOut(None, None, None, None, ot.buf["logp"].ptr, None)
    refused(-4, "tape handle", lib.chub_policy_sample_device(t._h, pt._p, ot.obs.ptr, D, None, C.byref(o4), None))
    close_all(ot, pt, t, oc, rc_, pc, c, full, fits, out, roll, pol, v, other)


# ---- 10. the torch adapter
TORCH_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["CHUB_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHUB_ROOT"], "tests"))
import torch  # before libchub: both must share one HIP runtime
torch.cuda.set_device(0)
import test_gpu_policy_sample
test_gpu_policy_sample.torch_adapter_collect()
print("TORCH_COLLECT_OK")
"""


def test_torch_adapter_collect_and_sampled_logp():
    """in a child process that imports torch first (as tests/test_gpu_torch_side.py does)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], env=dict(os.environ, CHUB_ROOT=root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TORCH_COLLECT_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def torch_adapter_collect():
    import torch
    from charginghub_env_amd import wrappers
    n, T = 64, 6
    kw = {k: BASE[k] for k in BASE if k != "station_type_list"}
    torch.manual_seed(3)
    for autoreset in ("per_env", True):
        env = wrappers.TorchHubVecEnv(n, [20, 25], ["fast", "slow"], seed=13, autoreset=autoreset, **kw)
        D, A, S, W = env.obs_dim, env.act_dim, env.vec.n_slots, env.vec.bit_words
        net = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, 33), torch.nn.Tanh(), torch.nn.Linear(33, A)).to("cuda")
        pol = env.load_policy(net)
        log_std = torch.tensor([-0.5, 0.1], device="cuda")
        pol.set_exploration(21, log_std.cpu().numpy())
        env.reset()
        ro = env.collect(pol, T)
        want = dict(obs0=(n, D), packed=(T, n, D + 2), reward=(T, n), done=(T, n), bits=(T, n, W), tail=(T, n, 2), u=(T, n, 2), logp=(T, n),
                    features=(T, n, D))
        assert {k: tuple(v.shape) for k, v in ro.items()} == want
        assert ro["reward"].data_ptr() == ro["packed"][:, :, D].data_ptr() and ro["bits"].dtype == torch.int64
        # the feature rows are the observations the actor read
        assert torch.equal(ro["features"][1:], ro["packed"][:-1, :, :D])
        if autoreset == "per_env":
            assert torch.equal(ro["features"][0], ro["obs0"])
        # an importance ratio of 1 at unchanged weights: sampled_logp of the module's own forward reproduces the recorded logp within the bound
        with torch.no_grad():
            z = net(ro["features"])
        new = wrappers.sampled_logp(z, ro["bits"], ro["u"], log_std)
        layers = [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in net if isinstance(m, torch.nn.Linear)]
        feats = ro["features"].cpu().numpy().reshape(T * n, D)
        z64, err = ps.pre_squash(feats, layers, "tanh")
        on = pl.unpack_bits(ro["bits"].cpu().numpy().view(np.uint64).reshape(T * n, W), S)
        u = ro["u"].cpu().numpy().reshape(T * n, 2).astype(np.float64)
        ref = ps.sampled_logp(z64, on, u, log_std.cpu().numpy())
        # eps is recovered from the rounded u: (u - z) / sigma moves by (ulp(u) / 2 + err_z) / sigma, and logp by |eps| times that
        sigma = np.exp(log_std.cpu().numpy().astype(np.float64))
        eps = (u - z64[:, S:]) / sigma
        bound = err[:, :S].sum(axis=1) + (np.abs(eps) * (ps.U * np.abs(u) + err[:, S:]) / sigma * 1.01).sum(axis=1) \
            + pl.gamma(S + 2 + 8) * (np.abs(ref) + 50) + (S + 2) * 8 * ps.ULP
        rec = ro["logp"].cpu().numpy().reshape(T * n).astype(np.float64)
        assert (np.abs(rec - ref) <= bound).all(), (np.abs(rec - ref).max(), bound.max())
        ratio = torch.exp(new.reshape(T * n).cpu().double() - torch.tensor(rec))
        assert float((ratio - 1).abs().max()) < 1e-4, "an importance ratio of 1 at unchanged weights"
        # a second collect continues from where the first stopped
        last = ro["packed"][T - 1, :, :D].clone()
        assert torch.equal(env._cur_obs, last)
        first_bits = ro["bits"].clone()
        ro2 = env.collect(pol, T)
        assert ro2 is ro and torch.equal(ro2["obs0"], last) and torch.equal(ro2["features"][0], last)
        assert not torch.equal(ro2["bits"], first_bits)
        if autoreset is True:
            assert env._t == 2 * T
            with pytest.raises(ValueError):
                env.collect(pol, 96 - 2 * T + 1)
            env.collect(pol, 96 - 2 * T)  # to the end of the day: the adapter resets as step does
            assert env._t == 0 and env._cur_obs is env._obs0 and env.last_obs is not None  # (reset() starts the adapter's count again)
            ro3 = env.collect(pol, T)  # a day's first rollout begins with the day's reset
            assert bool((ro3["done"] == 0).all()) and env._t == T
        o, r, d, _ = env.rollout(pol, 3)  # the deterministic loop continues from the same bookkeeping
        assert torch.isfinite(o).all()
        env.close()
    off = wrappers.TorchHubVecEnv(8, [20, 25], ["fast", "slow"], seed=1, autoreset=False)
    with pytest.raises(RuntimeError):
        off.collect(None, 4)
    off.close()
