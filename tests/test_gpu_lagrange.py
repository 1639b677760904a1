"""Constrained PPO on the device (include/chub.h, "constrained PPO on the device"), bit for bit against tests/lagrange_lib.py unless said
otherwise: (1) k_cost_gae and its merge on made data over lagrange_lib.GAE_CASES (workgroup edges, look-ahead edges, K, C, columns, done
patterns, kinds, values, masks, carries), a repeated call, two calls against the concatenation, chub_rollout_gae_device on the same data; (2) the step launch against the fold;
(3) the combine launch, and a gradient call fed its output; (4) chub_policy_collect_terms against a twin's attached buffer, step by step;
(5) one recorded iteration replayed three times against three eager ones; (6) the torch adapter's methods in a child process;
(7) refusals and ownership."""
import ctypes as C

import numpy as np
import pytest

import lagrange_lib as ll
from charginghub_env_amd import _lib, vec_env
from test_gpu_adam import Collected, to_host
from test_gpu_autoreset import Dev, buffers
from test_gpu_pile_obs import BASE, CANARY, make
from test_gpu_pile_set import RollSet
from test_gpu_policy import CANARY64, f32, gaussian_layers, same_state
from test_gpu_policy_sample import close_all

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
ST = _lib.ST
CANARY_F64 = np.uint64(0x7FF8BEEF0000BEEF)  # a NaN no kernel writes
STEPS = ll.step_cases()


def to_device(ptr, a):
    a = np.ascontiguousarray(a)
    _lib.check(_lib.load_library().chub_copy_to_device(0, C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, None))


def dbuf(a):
    b = buffers().DeviceBuffer(max(np.ascontiguousarray(a).nbytes, 8))
    b.from_host(a)
    return b


def constraints_of(case):
    return [dict(column=c, kind=k, limit=3.0 + i, lr=0.05 * (i + 1), lambda0=0.5 * i, lambda_max=0.0 if i % 2 else 4.0) for i, (c, k) in enumerate(case["cons"])]


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


class Made(object):
    """a case's arrays in device memory on a handle of its N envs, outputs canary-filled"""

    def __init__(self, case, d, T=None):
        self.case, self.d = case, d
        self.v = v = handle(case["N"])
        self.T = T = d["terms"].shape[0]
        N, K, D = case["N"], len(case["cons"]), v.obs_dim
        rs = np.random.RandomState(5)
        packed = rs.normal(size=(T, N, D + 2)).astype(F32)
        packed[:, :, D + 1] = np.where(d["done"], rs.choice([1.0, 2.5, -1.0], size=(T, N)), 0.0)  # (any non-zero fires)
        self.lag = v.make_lagrange(constraints_of(case))
        self.terms, self.packed = dbuf(d["terms"]), dbuf(packed)
        self.values = [None if x is None else dbuf(x) for x in d["values"]]
        self.finals = [None if x is None else dbuf(x) for x in d["finals"]]
        self.mask = None if d["mask"] is None else dbuf(d["mask"])
        self.adv = [dbuf(np.full((T, N), CANARY, dtype=np.uint32)) for _ in range(K)]
        self.ret = [dbuf(np.full((T, N), CANARY, dtype=np.uint32)) for _ in range(K)] if case.get("ret", True) else None
        self.carry0 = d["carry"]
        if self.carry0 is not None and d["mask"] is not None:  # (a masked-out env's carry keeps its bits: a canary)
            self.carry0 = self.carry0.copy()
            self.carry0.view(np.uint64)[d["mask"] == 0] = CANARY_F64
        self.carry = None if self.carry0 is None else dbuf(self.carry0)

    def run(self, stream=0):
        p = lambda b: 0 if b is None else b.ptr
        self.lag.gae(self.T, self.case["C"], self.terms.ptr, self.packed.ptr, [b.ptr for b in self.adv],
                     d_ret=None if self.ret is None else [b.ptr for b in self.ret], d_values=[p(b) for b in self.values],
                     d_final_values=[p(b) for b in self.finals], gamma=ll.GAMMA, lam=ll.LAM, d_mask=p(self.mask), d_ep_carry=p(self.carry), stream=stream)

    def read(self):
        self.v.sync()
        N, K = self.case["N"], len(self.case["cons"])
        lam, st, w = self.lag.read()
        return dict(adv=[b.to_host(np.uint32, (self.T, N)) for b in self.adv],
                    ret=None if self.ret is None else [b.to_host(np.uint32, (self.T, N)) for b in self.ret],
                    carry=None if self.carry is None else self.carry.to_host(np.uint64, (N, K)), stats=st, lam=lam, words=w)

    def free(self):
        close_all(self.lag, self.terms, self.packed, *[b for b in self.values + self.finals + self.adv + (self.ret or []) + [self.mask, self.carry]
                                                        if b is not None])


def want_of(case, d, carry=None):
    return ll.cost_gae(d["terms"], d["done"], case["cons"], ll.GAMMA, ll.LAM, d["values"], d["finals"], d["mask"], d["carry"] if carry is None else carry)


def check_gae(got, want, case, d, carry0, what):
    live = np.ones(case["N"], dtype=bool) if d["mask"] is None else d["mask"] != 0
    for k in range(len(case["cons"])):
        for name in ("adv", "ret"):
            if got[name] is None:
                continue
            g, w = got[name][k], ll.bits(want[name][k])
            bad = np.nonzero(g[:, live] != w[:, live])
            assert bad[0].size == 0, (what, name, k, "first (t, live env)", [int(x[0]) for x in bad], bad[0].size)
            assert (g[:, ~live] == CANARY).all(), (what, name, k, "a masked-out env's column was written")
    assert np.array_equal(ll.bits(got["stats"]), ll.bits(want["stats"])), (what, "stats", got["stats"], want["stats"])
    if got["carry"] is not None:
        assert np.array_equal(got["carry"][live], ll.bits(want["carry"])[live]), (what, "carry")
        assert np.array_equal(got["carry"][~live], ll.bits(carry0)[~live]), (what, "a masked-out env's carry moved")


# ---- 1. the kernel on made data
@pytest.mark.parametrize("case", ll.GAE_CASES, ids=[c["name"] for c in ll.GAE_CASES])
def test_cost_gae_equals_the_restatement_bit_for_bit(case):
    d = ll.gae_case(case)
    m = Made(case, d)
    want = want_of(case, d)
    m.run()
    got = m.read()
    check_gae(got, want, case, d, m.carry0, case["name"])
    live = (d["mask"] != 0) if d["mask"] is not None else np.ones(case["N"], dtype=bool)
    assert got["stats"][0, 0] == case["T"] * live.sum() and got["stats"][0, 3] == want["stats"][0, 3]
    # the same call again (the carry put back): identical bits
    if m.carry is not None:
        m.carry.from_host(m.carry0)
    m.run()
    again = m.read()
    for k in range(len(case["cons"])):
        assert np.array_equal(got["adv"][k], again["adv"][k]) and (got["ret"] is None or np.array_equal(got["ret"][k], again["ret"][k]))
    assert np.array_equal(ll.bits(got["stats"]), ll.bits(again["stats"])) and (got["carry"] is None or np.array_equal(got["carry"], again["carry"]))
    # the step launch after a real gae call, against the restatement on the same stats
    m.lag.step()
    lam, _, words = m.lag.read()
    for k, c in enumerate(constraints_of(case)):
        wl, ww = ll.lagrange_step(c["lambda0"], [0.0, 0.0, 0.0], want["stats"][k], c["limit"], c["lr"], c["lambda_max"])
        assert ll.bits(F64(lam[k])) == ll.bits(F64(wl)) and np.array_equal(ll.bits(words[k]), ll.bits(ww)), (case["name"], k, lam[k], wl, words[k], ww)
    m.free()


@pytest.mark.parametrize("name", ["n513-t17-k4-c3-edge", "n257-t17-k1-c1-twice", "n513-t9-k2-c3-random-mask"])
def test_two_calls_with_the_carry_equal_one_call_on_the_concatenation(name):
    """costs are integers and halves: the episode sums are exact, so the split changes no bit of them"""
    case = next(c for c in ll.GAE_CASES if c["name"] == name)
    a, b = ll.gae_case(case, seed=1), ll.gae_case(case, seed=2)
    b["mask"] = a["mask"]
    both = dict(a, terms=np.concatenate([a["terms"], b["terms"]]), done=np.concatenate([a["done"], b["done"]]), values=[None] * len(case["cons"]),
                finals=[None] * len(case["cons"]))
    a["values"] = b["values"] = a["finals"] = b["finals"] = both["values"]
    first, second, whole = Made(case, a), Made(case, dict(b, carry=a["carry"])), Made(case, both)
    first.run()
    g1 = first.read()
    w1 = want_of(case, a)
    check_gae(g1, w1, case, a, first.carry0, (name, "first"))
    second.carry.from_host(g1["carry"])
    second.run()
    g2 = second.read()
    check_gae(g2, want_of(case, b, carry=w1["carry"]), case, b, first.carry0, (name, "second"))
    whole.run()
    g = whole.read()
    check_gae(g, want_of(case, both), case, both, whole.carry0, (name, "whole"))
    live = np.ones(case["N"], dtype=bool) if a["mask"] is None else a["mask"] != 0
    assert np.array_equal(g2["carry"][live], g["carry"][live]) and np.array_equal(g1["stats"][:, 3:] + g2["stats"][:, 3:], g["stats"][:, 3:])
    assert g["stats"][:, 3].min() > 0
    for m in (first, second, whole):
        m.free()


def test_the_reward_and_the_cost_entry_points_run_one_recurrence():
    """chub_rollout_gae_device against chub_lagrange_gae_device (K = 1, CHUB_COST_STEP, C = 1) fed the same rewards as its terms: adv, ret
    and the first three stats words bit for bit.  N = 257 is a full workgroup and one lane, T = 9 a full chunk of eight steps and a partial
    one; an episode ends at t = 7 in env 0 and at t = 8 in env 256; every other env is masked out and keeps its canaries"""
    N, T = 257, 9
    v = handle(N)
    D = v.obs_dim
    rs = np.random.RandomState(41)
    done = rs.uniform(size=(T, N)) < 1.0 / 9.0
    done[7, 0] = done[8, 256] = True
    mask = (np.arange(N) % 2 == 0).astype(np.uint8)
    packed = rs.normal(size=(T, N, D + 2)).astype(F32)
    packed[:, :, D + 1] = done
    reward = np.ascontiguousarray(packed[:, :, D])
    lag = v.make_lagrange([dict(column=0, kind="step", limit=1.0, lr=0.1)])
    d_packed, d_terms, d_mask = dbuf(packed), dbuf(reward.reshape(T, N, 1)), dbuf(mask)
    d_values, d_final = dbuf(rs.normal(size=(T + 1, N)).astype(F32)), dbuf(rs.normal(size=N).astype(F32))
    out = [dbuf(np.full((T, N), CANARY, dtype=np.uint32)) for _ in range(4)]
    d_stats = dbuf(np.full(3, CANARY_F64, dtype=np.uint64))
    v.gae_device(T, d_packed.ptr, d_values.ptr, out[0].ptr, d_ret=out[1].ptr, d_final_values=d_final.ptr, gamma=ll.GAMMA, lam=ll.LAM, d_mask=d_mask.ptr,
                 d_stats=d_stats.ptr)
    lag.gae(T, 1, d_terms.ptr, d_packed.ptr, [out[2].ptr], d_ret=[out[3].ptr], d_values=[d_values.ptr], d_final_values=[d_final.ptr], gamma=ll.GAMMA,
            lam=ll.LAM, d_mask=d_mask.ptr)
    v.sync()
    adv, ret, cadv, cret = [b.to_host(np.uint32, (T, N)) for b in out]
    live = mask != 0
    assert np.array_equal(adv, cadv) and np.array_equal(ret, cret)
    assert not (adv[:, live] == CANARY).any() and not (ret[:, live] == CANARY).any()
    for a in (adv, ret, cadv, cret):
        assert (a[:, ~live] == CANARY).all(), "a masked-out env's column was written"
    stats = d_stats.to_host(np.uint64, (3,))
    assert np.array_equal(stats, ll.bits(lag.read()[1])[0, :3]) and stats.view(F64)[0] == T * live.sum()
    close_all(lag, d_packed, d_terms, d_mask, d_values, d_final, d_stats, *out)


# ---- 2. the step on the device against the fold
def set_object(lag, lam, words):
    """lambda and the words through the state calls (and the blob's round trip)"""
    K = lag.K
    blob = np.frombuffer(lag.get_state(), dtype=np.uint8).copy()
    assert blob.size == 8 + 8 * 4 * K and blob[:8].view(np.int64)[0] == K
    body = blob[8:].view(F64)
    body[:K] = lam
    body[K:] = np.asarray(words, dtype=F64).ravel()
    lag.set_state(blob.tobytes())
    assert lag.get_state() == blob.tobytes()


def test_the_step_launch_equals_the_fold_on_made_stats():
    v = handle(255)
    names = list(STEPS)
    for group in (names[:4], names[4:], names[2:3]):  # (K = 4, 4 and 1: lane k takes constraint k)
        cs = [STEPS[n] for n in group]
        lag = v.make_lagrange([dict(column=0, kind="step", limit=c["limit"], lr=c["lr"], lambda0=0.0, lambda_max=c["lambda_max"]) for c in cs])
        lam0, _, w0 = lag.read()
        assert (lam0 == 0).all() and (w0 == 0).all()
        set_object(lag, [c["lam"] for c in cs], [c["words"] for c in cs])
        to_device(lag.stats_address, np.array([c["stats"] for c in cs], dtype=F64))
        lag.step()
        lam, st, w = lag.read()
        for k, (n, c) in enumerate(zip(group, cs)):
            fl, fw = np.array([c["lam"]], dtype=F64), np.array(c["words"], dtype=F64)
            vec_env.lagrange_fold(dict(limit=c["limit"], lr=c["lr"], lambda_max=c["lambda_max"]), fl, fw, c["stats"])
            wl, ww = ll.lagrange_step(c["lam"], c["words"], c["stats"], c["limit"], c["lr"], c["lambda_max"])
            assert ll.bits(F64(lam[k])) == ll.bits(fl)[0] == ll.bits(F64(wl)), (n, lam[k], fl, wl)
            assert np.array_equal(ll.bits(w[k]), ll.bits(fw)) and np.array_equal(ll.bits(fw), ll.bits(ww)), (n, w[k], fw, ww)
        assert np.array_equal(ll.bits(st), ll.bits(np.array([c["stats"] for c in cs], dtype=F64))), "the step reads the stats and leaves them"
        # set_lambda_device: K words from device memory, nothing else moves
        src = dbuf(np.arange(1, len(cs) + 1, dtype=F64) / 8)
        lag.set_lambda_device(src.ptr)
        lam2, _, w2 = lag.read()
        assert np.array_equal(lam2, np.arange(1, len(cs) + 1) / 8) and np.array_equal(ll.bits(w2), ll.bits(w))
        close_all(src, lag)


# ---- 3. combine
STATS3 = np.array([[960.0, 480.0, 7.0, 2.0, 5.0, 13.0], [960.0, -96.0, 7.0, 2.0, 5.0, 13.0], [960.0, 1440.0, 7.0, 2.0, 5.0, 13.0]])


def lagrange3(v, lam):
    lag = v.make_lagrange([dict(column=0, kind="step", limit=1.0, lr=0.1) for _ in range(3)])
    to_device(lag.stats_address, STATS3)
    src = dbuf(np.asarray(lam, dtype=F64))
    lag.set_lambda_device(src.ptr)
    v.sync()
    src.free()
    return lag


@pytest.mark.parametrize("case", ll.COMBINE_CASES, ids=[c["name"] for c in ll.COMBINE_CASES])
def test_combine_equals_the_restatement_bit_for_bit(case):
    v = handle(255)
    adv, adv_stats, costs = ll.combine_case(case)
    n = case["n"]
    lag = lagrange3(v, case["lam"])
    d_adv, d_costs = dbuf(adv), [dbuf(c) for c in costs]
    d_stats = None if adv_stats is None else dbuf(adv_stats)
    d_out = d_adv if case.get("in_place") else dbuf(np.full(n + 1, CANARY, dtype=np.uint32))
    lag.combine(n, d_adv.ptr, [b.ptr for b in d_costs], d_out.ptr, d_adv_stats=0 if d_stats is None else d_stats.ptr)
    v.sync()
    got = d_out.to_host(np.uint32, (n + (0 if case.get("in_place") else 1),))
    want = ll.combine(adv, adv_stats, costs, case["lam"], STATS3)
    bad = np.nonzero(got[:n] != ll.bits(want))[0]
    assert bad.size == 0, (case["name"], "first entry", int(bad[0]), bad.size, f32(got[:n])[bad[:4]], want[bad[:4]])
    if not case.get("in_place"):
        assert got[n] == CANARY, "the entry past n was written"
        assert np.array_equal(d_adv.to_host(np.uint32, (n,)), ll.bits(adv)), "the input moved"
    if not any(case["lam"]):  # every lambda 0: the normalised advantage's own bits
        if adv_stats is None:
            assert np.array_equal(got[:n], ll.bits(adv))
        else:
            m32, s32 = ll.advantage_normaliser(adv_stats)
            assert np.array_equal(got[:n], ll.bits(((adv - m32).astype(F32) * s32).astype(F32)))
    close_all(lag, d_adv, *d_costs, *([d_stats] if d_stats is not None else []), *([] if case.get("in_place") else [d_out]))


def test_a_gradient_call_fed_the_combined_advantage_equals_one_fed_the_statistics():
    """every lambda 0: chub_policy_grad_device on combine's output with no d_adv_stats against the same call on adv with d_adv_stats --
    gradients and stats bit for bit"""
    k = Collected()
    v, n = k.v, k.n_rows
    a64 = k.adv.astype(F64)
    d_stats = dbuf(np.array([float(n), a64.sum(), (a64 * a64).sum()]))
    lag = lagrange3(v, [0.0, 0.0, 0.0])
    costs = [dbuf(np.random.RandomState(i).normal(size=n).astype(F32)) for i in range(3)]
    d_out = dbuf(np.zeros(n, dtype=F32))
    lag.combine(n, k.d_adv.ptr, [b.ptr for b in costs], d_out.ptr, d_adv_stats=d_stats.ptr)
    gW, gb, gls = k.opt_a.grads()
    got = []
    for d_adv, st in ((k.d_adv.ptr, d_stats.ptr), (d_out.ptr, 0)):
        k.pstats.from_host(np.full(6, np.nan))
        k.grad.grad_device(n, n, k.roll.ptr("feat"), k.roll.ptr("u"), d_adv, d_pile_bits=k.roll.ptr("bits"), d_logp_old=k.roll.ptr("logp"), d_adv_stats=st,
                           loss="ppo_clip", clip_eps=0.2, ent_coef=0.01, d_gW=gW, d_gb=gb, d_glog_std=gls, d_stats=k.pstats.ptr)
        v.sync()
        got.append((k.own_gradient(k.opt_a).copy(), k.pstats.to_host(F64, (6,))))
    assert np.array_equal(ll.bits(got[0][0]), ll.bits(got[1][0])) and np.array_equal(ll.bits(got[0][1]), ll.bits(got[1][1]))
    assert np.abs(got[0][0]).max() > 0 and got[0][1][0] == n
    close_all(lag, d_stats, d_out, *costs)
    k.free()


# ---- 4. chub_policy_collect_terms
FIELDS = ("grid_excess", "not_meet", "soc_penalty")


class Terms(RollSet):
    """RollSet with the terms [T][N][C] kept, on a handle with telemetry on"""

    def __init__(self, v, pol, T, fields=FIELDS):
        RollSet.__init__(self, v, pol, T)
        self.fields = fields
        self.C = len(fields)
        self.terms = dbuf(np.full((T, v.n_envs, self.C), CANARY, dtype=np.uint32))

    def collect_terms(self, mode, which="decidable", first=0, stream=0):
        self.pol.collect(self.T, self.ptr("obs0"), self.ptr("packed"), self.ptr("bits"), self.ptr("tail"), self.ptr("u"), self.ptr("logp"),
                         d_features=self.ptr("feat"), d_final_obs=self.ptr("final") if mode == "autoreset" else 0, first_step=first, mode=mode,
                         stream=stream, logp_piles=which, d_set_bits=self.ptr("set"), d_terms=self.terms.ptr, term_fields=self.fields)

    def free(self):
        RollSet.free(self)
        self.terms.free()


def trio(rng, piles, n, T):
    """three equal handles with telemetry on, an actor on each, their rollout arrays"""
    rs = np.random.RandomState(29)
    vs = [make(rng, piles, n, seed=6) for _ in range(3)]
    layers = gaussian_layers(rs, [vs[0].obs_dim, 32, vs[0].act_dim])
    out = []
    for v in vs:
        v.set_telemetry(True)
        pol = v.make_policy(layers)
        pol.set_exploration(77, np.array([-0.5, 0.0], dtype=F32))
        out.append((v, pol, Terms(v, pol, T)))
    return out


def stagger(v, r, seed=3, at=(5, 70)):
    """per-env clocks 85, 85 - at[0] and 85 - at[1] by thirds (85, 80 and 15): a reset, 85 auto-reset steps under random actions, two masked
    resets on the way"""
    dv = Dev(v)
    n = v.n_envs
    rs = np.random.RandomState(seed)
    group = np.arange(n) % 3
    v.reset_device(r.ptr("obs0"))
    for i in range(85):
        if i == at[0]:
            dv.reset_dmask(group == 1)
        if i == at[1]:
            dv.reset_dmask(group == 2)
        dv.act.from_host(rs.uniform(-1, 1, size=(n, v.act_dim)).astype(F32))
        v.step_autoreset_device(dv.act.ptr, dv.packed.ptr, dv.final.ptr)
    v.sync()
    r.buf["obs0"].from_host(dv.packed.to_host(F32, (n, v.obs_dim + 2))[:, :v.obs_dim].copy())
    assert sorted(set(v.env_clocks().tolist())) == sorted([85 - at[1], 85 - at[0], 85])
    return group


@pytest.mark.parametrize("rng", ["philox", "philox_curves"])
@pytest.mark.parametrize("piles", [[3, 2], [20, 25]], ids=["3-2", "20-25"])
@pytest.mark.parametrize("mode", ["lockstep", "autoreset"])
def test_collect_terms_keeps_what_an_attached_buffer_holds_after_every_step(mode, piles, rng):
    n, T = 33, 96 if mode == "lockstep" else 20
    (va, pa, ra), (vb, pb, rb), (vc, pc, rc) = trio(rng, piles, n, T)
    mask = _lib.st_fields_mask(FIELDS)
    # a: an attachment of its own, made before the call, with other fields; b: the twin with the call's fields attached
    own = dbuf(np.full((n, 2), CANARY, dtype=np.uint32))
    attached = dbuf(np.full((n, 3), CANARY, dtype=np.uint32))
    va.attach_step_terms(own.ptr, ("reward", "grid_draw"))
    vb.attach_step_terms(attached.ptr, FIELDS)
    va.set_episode_stats(True)
    if mode == "autoreset":
        for v, r in ((va, ra), (vb, rb), (vc, rc)):
            group = stagger(v, r)
    held = own.to_host(np.uint32, (n, 2))
    ra.collect_terms(mode)
    rc.collect_set(mode, "decidable")
    # the twin: the documented calls one by one, its attached buffer copied out after each step
    D, want = vb.obs_dim, np.zeros((T, n, 3), dtype=np.uint32)
    if mode == "lockstep":
        vb.reset_device(rb.ptr("obs0"))
    for t in range(T):
        src, ld = (rb.ptr("packed", t - 1), D + 2) if t else (rb.ptr("obs0"), D)
        pb.sample_device(src, ld, d_logp=rb.ptr("logp", t), d_actions=rb.rows.ptr if mode == "autoreset" else 0, d_pile_bits=rb.ptr("bits", t),
                         d_tail=rb.ptr("tail", t), d_u=rb.ptr("u", t), d_features=rb.ptr("feat", t), logp_piles="decidable", d_set_bits=rb.ptr("set", t))
        if mode == "lockstep":
            vb.step_bits_device_packed(rb.ptr("bits", t), rb.ptr("tail", t), rb.ptr("packed", t))
        else:
            vb.step_autoreset_device(rb.rows.ptr, rb.ptr("packed", t), rb.ptr("final"))
        vb.sync()
        want[t] = attached.to_host(np.uint32, (n, 3))
    ha, hb, hc = ra.host(), rb.host(), rc.host()
    got = ra.terms.to_host(np.uint32, (T, n, 3))
    bad = np.nonzero(got != want)
    assert bad[0].size == 0, ("first (t, env, column)", [int(x[0]) for x in bad], bad[0].size)
    assert not (got == CANARY).any() and (f32(got)[:, :, 2] > 0).any()
    for k in ha:
        assert np.array_equal(ha[k], hc[k]), (k, "against chub_policy_collect_set")
        assert np.array_equal(ha[k], hb[k]), (k, "against the calls one by one")
    same_state(va, vc, "after the rollout")
    # the handle's own attachment is in force again and its buffer holds what it held
    assert va.step_terms_attached == _lib.st_fields_mask(("reward", "grid_draw")) and vb.step_terms_attached == mask
    assert np.array_equal(own.to_host(np.uint32, (n, 2)), held)
    done = f32(ha["packed"])[:, :, D + 1] != 0
    if mode == "lockstep":
        assert done[T - 1].all() and not done[:T - 1].any()
    else:
        at = done.argmax(axis=0)
        assert (done.sum(axis=0) == (group != 2)).all() and set(at[group == 0]) == {10} and set(at[group == 1]) == {15}
    # AT_DONE on SOC_PENALTY is the episode's test_penalty: the ledger keeps the f64 expression the term narrows once to f32
    ledger = va.episode_stats(finished=True)["test_penalty"]
    ended = np.nonzero(done.any(axis=0))[0]
    cost = ll.costs_of(f32(got), done, 2, ll.AT_DONE)
    assert ended.size > 0
    for e in ended:
        assert ll.bits(F32(ledger[e])) == ll.bits(cost[done[:, e].argmax(), e]), (e, ledger[e], cost[:, e])
    assert (ll.bits(cost[~done]) == 0).all()
    close_all(own, attached, ra, rb, rc, pa, pb, pc, va, vb, vc)


# ---- 5. one recorded iteration
class Iteration(object):
    """collect_terms (auto-reset, T = 20), the reward critic's values and GAE, the cost GAE, the multipliers' step, combine.  The envs' clocks
    are 85, 65 and 45 by thirds: each of three consecutive iterations sees one third of the envs end its day"""
    T, N = 20, 33

    def __init__(self):
        rs = np.random.RandomState(11)
        self.v = v = make("philox", [20, 25], self.N, seed=6)
        v.set_telemetry(True)
        D, T, N = v.obs_dim, self.T, self.N
        self.pol = v.make_policy(gaussian_layers(rs, [D, 32, v.act_dim]))
        self.pol.set_exploration(77, np.array([-0.5, 0.0], dtype=F32))
        self.crit = v.make_critic(gaussian_layers(rs, [D, 16, 1]), max_rows=(T + 1) * N)
        self.r = Terms(v, self.pol, T)
        stagger(v, self.r, at=(20, 40))
        self.lag = v.make_lagrange([dict(column=0, kind="step", limit=0.0, lr=1e-4, lambda0=0.25), dict(column=2, kind="done", limit=0.5, lr=0.01),
                                    dict(column=1, kind="step", limit=1e9, lr=1e-3, lambda0=0.5, lambda_max=2.0)])
        mg = buffers()
        self.values, self.final = mg.DeviceBuffer((T + 1) * N * 4), mg.DeviceBuffer(N * 4)
        self.adv, self.ret, self.stats, self.out = mg.DeviceBuffer(T * N * 4), mg.DeviceBuffer(T * N * 4), mg.DeviceBuffer(24), mg.DeviceBuffer(T * N * 4)
        self.cadv = [mg.DeviceBuffer(T * N * 4) for _ in range(3)]
        self.carry = dbuf(np.zeros((N, 3)))

    def run(self, stream=0):
        v, r, T, N, D = self.v, self.r, self.T, self.N, self.v.obs_dim
        r.collect_terms("autoreset", stream=stream)
        self.crit.values_device(N, N, r.ptr("obs0"), self.values.ptr, ld=D, stream=stream)
        self.crit.values_device(T * N, T * N, r.ptr("packed"), self.values.ptr + 4 * N, ld=D + 2, stream=stream)
        self.crit.values_device(N, N, r.ptr("final"), self.final.ptr, ld=D, stream=stream)
        v.gae_device(T, r.ptr("packed"), self.values.ptr, self.adv.ptr, d_ret=self.ret.ptr, d_final_values=self.final.ptr, d_stats=self.stats.ptr,
                     stream=stream)
        self.lag.gae(T, 3, r.terms.ptr, r.ptr("packed"), [b.ptr for b in self.cadv], d_ep_carry=self.carry.ptr, stream=stream)
        self.lag.step(stream=stream)
        self.lag.combine(T * N, self.adv.ptr, [b.ptr for b in self.cadv], self.out.ptr, d_adv_stats=self.stats.ptr, stream=stream)

    def snapshot(self):
        self.v.sync()
        lam, st, w = self.lag.read()
        return dict(lam=ll.bits(lam), stats=ll.bits(st), words=ll.bits(w), out=self.out.to_host(np.uint32, (self.T * self.N,)),
                    terms=self.r.terms.to_host(np.uint32, (self.T, self.N, 3)), carry=self.carry.to_host(np.uint64, (self.N, 3)),
                    packed=self.r.host()["packed"])

    def free(self):
        close_all(self.lag, self.values, self.final, self.adv, self.ret, self.stats, self.out, self.carry, *self.cadv, self.r, self.crit, self.pol, self.v)


def test_a_recorded_iteration_replays_as_eager_ones():
    """the iteration recorded on a created stream (a recording runs nothing) and replayed three times, against three eager iterations on a
    twin.  Every iteration reads the same obs0 rows, as a replay must; the envs move on, so each rollout -- and each J_last -- is its own"""
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
    for call in (lambda: b.v.make_lagrange([dict(column=0, kind="step")]), b.lag.read, b.lag.get_state, lambda: b.lag.set_state(b"\0" * 104), b.lag.close):
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
    # each iteration's J_last is that rollout's alone: the stats of its own gae, not a running sum
    for it in range(3):
        s, w = eager[it]["stats"].view(F64), eager[it]["words"].view(F64)
        taken = s[:, 3] > 0
        assert (s[:, 3] == Iteration.N // 3).all() and taken.all() and np.array_equal(ll.bits(w[:, 0]), ll.bits(s[:, 4] / s[:, 3]))
    assert not np.array_equal(eager[0]["terms"], eager[1]["terms"]) and not np.array_equal(eager[1]["stats"], eager[2]["stats"])
    assert eager[2]["words"].view(F64)[:, 1:].tolist() == [[3.0, 0.0]] * 3, "three steps taken per constraint"
    b.v.graph_destroy(graph)
    a.free()
    b.free()
    st.destroy()


# ---- 6. the torch adapter, in a child process that imports torch first
TORCH_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["CHUB_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHUB_ROOT"], "tests"))
import torch  # before libchub: both must share one HIP runtime
torch.cuda.set_device(0)
import test_gpu_lagrange
getattr(test_gpu_lagrange, os.environ["CHUB_CHILD"])()
print("TORCH_LAGRANGE_OK")
"""


def test_the_adapters_methods_equal_the_c_calls():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], env=dict(os.environ, CHUB_ROOT=root, CHUB_CHILD="adapter_methods"), capture_output=True,
                       text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "TORCH_LAGRANGE_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def adapter_methods():
    """collect(terms=), make_constraints, cost_advantages, update_multipliers, constrained_advantages and constraint_summary on one adapter
    against the restatement fed the adapter's own rollout (the C calls are held to it above); the default collect is unchanged"""
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
    cons = env.make_constraints([dict(term="soc_penalty", kind="done", limit=0.5, lr=0.01), dict(term="grid_excess", kind="step", limit=0.0, lr=1e-4, lambda0=0.5),
                                 dict(term="soc_penalty", kind="step", limit=1e6, lr=0.5, lambda0=1.0, lambda_max=1.5)])
    assert cons.terms == ("grid_excess", "soc_penalty") and [c["column"] for c in cons.constraints] == [1, 0, 1]
    ro = env.collect(pol, T, logp_piles="decidable", terms=cons.terms)
    plain = env2.collect(pol2, T, logp_piles="decidable")
    torch.cuda.synchronize()
    assert "terms" not in plain and tuple(ro["terms"].shape) == (T, N, 2) and ro["terms_names"] == cons.terms
    for k in plain:
        assert torch.equal(plain[k].cpu(), ro[k].cpu()), (k, "collect(terms=) changes no other array")
    D = env.obs_dim
    values = [torch.randn((T + 1, N), device=env.device), None, torch.randn((T + 1, N), device=env.device)]
    finals = [torch.randn((N,), device=env.device), None, None]
    advs, rets = env.cost_advantages(ro, cons, cost_values=values, final_values=finals, gamma=0.98, lam=0.9)
    adv = torch.randn((T, N), device=env.device)
    a64 = adv.double()
    adv_stats = torch.stack([torch.tensor(float(T * N), dtype=torch.float64, device=env.device), a64.sum(), (a64 * a64).sum()])
    env.update_multipliers(cons)
    out = env.constrained_advantages(adv, adv_stats, advs, cons)
    summary = env.constraint_summary(cons)
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    terms, done = host(ro["terms"]), host(ro["done"]) != 0
    assert done.any() and not done.all()
    want = ll.cost_gae(terms, done, [(1, ll.AT_DONE), (0, ll.STEP), (1, ll.STEP)], 0.98, 0.9, [host(x) for x in values], [host(x) for x in finals],
                       None, np.zeros((N, 3)))
    for k in range(3):
        assert np.array_equal(ll.bits(host(advs[k])), ll.bits(want["adv"][k])) and np.array_equal(ll.bits(host(rets[k])), ll.bits(want["ret"][k])), k
    lam, st, w = cons.read()
    assert np.array_equal(ll.bits(st), ll.bits(want["stats"]))
    assert np.array_equal(ll.bits(host(cons._torch["carry"])), ll.bits(want["carry"]))
    lam_want = []
    for k, c in enumerate(cons.constraints):
        l, ww = ll.lagrange_step(c["lambda0"], [0.0, 0.0, 0.0], want["stats"][k], c["limit"], c["lr"], c["lambda_max"])
        lam_want.append(l)
        assert ll.bits(F64(lam[k])) == ll.bits(F64(l)) and np.array_equal(ll.bits(w[k]), ll.bits(ww)), k
    assert lam_want[2] == 0.0 or lam_want[2] <= 1.5
    got = host(out)
    ref = ll.combine(host(adv), host(adv_stats), [host(a) for a in advs], lam_want, want["stats"])
    assert got.shape == (T, N) and np.array_equal(ll.bits(got.ravel()), ll.bits(ref))
    assert [s["term"] for s in summary] == ["soc_penalty", "grid_excess", "soc_penalty"] and [s["kind"] for s in summary] == ["done", "step", "step"]
    for k, s in enumerate(summary):
        assert s["lambda"] == lam[k] and s["episodes"] == int(st[k, 3]) and s["steps"] == int(w[k, 1]) and s["skipped"] == int(w[k, 2])
        assert s["cost"] == w[k, 0] and (s["episodes"] == 0 or s["episode_cost_mean"] == st[k, 4] / st[k, 3])
    # an object of another handle is refused by every method
    for call in (lambda: env2.cost_advantages(ro, cons), lambda: env2.update_multipliers(cons), lambda: env2.constrained_advantages(adv, None, advs, cons),
                 lambda: env2.constraint_summary(cons)):
        with pytest.raises(ValueError, match="another handle"):
            call()
    with pytest.raises(ValueError, match="terms=constraints.terms"):
        env.cost_advantages(plain, cons)
    with pytest.raises(ValueError):
        env.make_constraints([dict(term="no_such_term")])
    cons.close()
    env.close()
    env2.close()


# ---- 7. refusals and ownership
def test_every_refusal_leaves_the_outputs_untouched():
    case = next(c for c in ll.GAE_CASES if c["name"] == "n255-t7-k2-c3-all")
    d = ll.gae_case(case)
    m = Made(case, d)
    v, lag, lib = m.v, m.lag, _lib.load_library()
    to_device(lag.stats_address, np.full((2, 6), 3.0))
    before = m.read()
    good = dict(column=0, kind="step", limit=1.0, lr=0.1, lambda0=0.0, lambda_max=0.0)
    for text, bad in (("1 .. 4", []), ("1 .. 4", [good] * 5), ("column", [dict(good, column=-1)]), ("kind", [dict(good, kind=2)]),
                      ("finite", [dict(good, lr=-1.0)]), ("finite", [dict(good, limit=float("nan"))]), ("finite", [dict(good, lambda0=float("inf"))]),
                      ("finite", [dict(good, lambda_max=-2.0)]), ("lambda0", [dict(good, lambda0=3.0, lambda_max=2.0)])):
        with pytest.raises(_lib.ChubError, match=text):
            v.make_lagrange(bad)
    with pytest.raises(ValueError):
        v.make_lagrange([dict(good, kind="sometimes")])
    T, C_ = m.T, case["C"]
    args = dict(n_steps=T, n_columns=C_, d_terms=m.terms.ptr, d_packed=m.packed.ptr, d_adv=[b.ptr for b in m.adv])
    for text, kw in (("T >= 1", dict(n_steps=0)), ("C >= 1", dict(n_columns=0)), ("outside 0 .. C - 1", dict(n_columns=2)), ("are required", dict(d_terms=0)),
                     ("are required", dict(d_packed=0)), ("d_adv\\[k\\] is required", dict(d_adv=[m.adv[0].ptr, 0])), ("\\[0, 1\\]", dict(gamma=1.5)),
                     ("\\[0, 1\\]", dict(lam=-0.1)), ("\\[0, 1\\]", dict(gamma=float("nan")))):
        with pytest.raises(_lib.ChubError, match=text):
            lag.gae(**dict(args, **kw))
    out = dbuf(np.full(8, CANARY, dtype=np.uint32))
    for text, call in (("n >= 1", lambda: lag.combine(0, m.adv[0].ptr, [m.adv[0].ptr, m.adv[1].ptr], out.ptr)),
                       ("null argument", lambda: lag.combine(8, 0, [m.adv[0].ptr, m.adv[1].ptr], out.ptr)),
                       ("null argument", lambda: lag.combine(8, m.adv[0].ptr, [m.adv[0].ptr, m.adv[1].ptr], 0)),
                       ("d_adv_cost\\[k\\] is required", lambda: lag.combine(8, m.adv[0].ptr, [m.adv[0].ptr, 0], out.ptr)),
                       ("null argument", lambda: lag.set_lambda_device(0))):
        with pytest.raises(_lib.ChubError, match=text):
            call()
    with pytest.raises(ValueError):
        lag.combine(8, m.adv[0].ptr, [m.adv[0].ptr], out.ptr)
    other = v.make_lagrange([good])
    with pytest.raises(_lib.ChubError, match="another K"):
        lag.set_state(other.get_state())
    # chub_policy_collect_terms: telemetry off, a bad mask, a null d_terms, and chub_policy_collect_set's own refusals
    w = make("philox", [20, 25], 8)
    pol = w.make_policy(gaussian_layers(np.random.RandomState(1), [w.obs_dim, 16, w.act_dim]))
    pol.set_exploration(3, np.array([-0.5, 0.0], dtype=F32))
    r = Terms(w, pol, 4)
    with pytest.raises(_lib.ChubError, match="telemetry is off"):
        r.collect_terms("lockstep")
    w.set_telemetry(True)
    call = lambda which=2, fields=7, d_terms=r.terms.ptr, T=4, first=0: lib.chub_policy_collect_terms(
        w._h, pol._p, 0, which, C.byref(_lib.ChubRollout(T, r.ptr("packed"), r.ptr("bits"), r.ptr("tail"), r.ptr("u"), r.ptr("logp"), None, None)),
        r.ptr("set"), r.ptr("obs0"), first, fields, d_terms, None)
    for text, kw in (("non-empty mask", dict(fields=0)), ("non-empty mask", dict(fields=1 << 27)), ("null argument", dict(d_terms=None)),
                     ("which is negative", dict(which=3)), ("T >= 1", dict(T=0)), ("inside one day", dict(T=4, first=94))):
        assert call(**kw) == -1 and text in lib.chub_last_error().decode(), (text, lib.chub_last_error())
    w.sync()
    assert (r.terms.to_host(np.uint32, (4, 8, 3)) == CANARY).all() and (r.host()["packed"] == CANARY).all()
    assert call() == 0, lib.chub_last_error()
    w.sync()
    assert not (r.terms.to_host(np.uint32, (4, 8, 3)) == CANARY).any() and w.step_terms_attached == 0
    after = m.read()
    for k in ("adv", "ret"):
        assert all(np.array_equal(x, y) and (x == CANARY).all() for x, y in zip(before[k], after[k])), k
    assert np.array_equal(ll.bits(before["stats"]), ll.bits(after["stats"])) and np.array_equal(before["carry"] if before["carry"] is not None else 0,
                                                                                                 after["carry"] if after["carry"] is not None else 0)
    assert np.array_equal(ll.bits(before["lam"]), ll.bits(after["lam"])) and (out.to_host(np.uint32, (8,)) == CANARY).all()
    close_all(out, other, r, pol, w)
    m.free()


def test_destroying_the_handle_takes_a_lagrange_object_and_a_graph_in_its_stride():
    """chub_destroy with a chub_lagrange and a recorded graph alive: CHUB_OK, and a fresh handle works"""
    mg = buffers()
    lib = _lib.load_library()
    it = Iteration()
    st = mg.Stream(0)
    v = it.v
    v.graph_begin(st.ptr)
    it.run(stream=st.ptr)
    graph = v.graph_end(st.ptr)
    st.sync()
    more = v.make_lagrange([dict(column=0, kind="done", limit=1.0, lr=0.1)])
    assert lib.chub_destroy(v._h) == 0, lib.chub_last_error()
    v._h = None  # (what v.close() does; the objects went with the handle, so their close() calls nothing)
    v.graph_destroy(graph)
    more.close()
    it.free()
    st.destroy()
    w = make("philox", (2, 3), 8)
    lag = w.make_lagrange([dict(column=0, kind="step", limit=1.0, lr=0.5, lambda0=0.25)])
    lag.step()
    lam, _, words = lag.read()
    assert lam[0] == 0.25 and words.tolist() == [[0.0, 0.0, 1.0]], "no episode yet: skipped"
    close_all(lag, w)
