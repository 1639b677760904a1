"""Actor gradients on the device (include/chub.h, "actor gradients on the device") against tests/policy_grad_lib.py's f64 restatement:
(1) exact data, bit for bit, for every layer count and every R; (2) every head alignment, hidden width, depth, activation and loss on
made rollouts, within the derived bar; (3) rollouts really collected with decidable sets in both Philox modes and both run modes:
unchanged parameters first, then a step large enough to clip rows both ways; (4) minibatches by d_rows; (5) determinism, a captured
graph, new weights between replays; (6) the forward alone; (7) a normaliser derived from moments; (8) every refusal; (9) the torch adapter
against CUDA autograd, in a child process."""
import ctypes as C

import numpy as np
import pytest

import policy_grad_lib as pgl
import policy_lib as pl
import policy_sample_lib as ps
from charginghub_env_amd import _lib
from test_gpu_autoreset import buffers
from test_gpu_pile_obs import BASE, make
from test_gpu_pile_set import RollSet
from test_gpu_policy import f32
from test_gpu_policy_sample import close_all

pytestmark = pytest.mark.gpu
F32 = np.float32
N_ENVS = 64


def widths_of(c):
    return list(c.hidden) + [c.layers[-1][0].shape[0]]


def tpw_of(c):
    return pgl.tiles_per_workgroup(c.piles, widths_of(c), c.R, c.head, c.act, c.inputs)


def actor(c, max_rows, v=None):
    """a handle of the case's hub, a policy with the case's weights, log_std and normaliser, and its gradient object"""
    v = v or make("philox", c.piles, N_ENVS)
    pol = v.make_policy(c.layers, inputs=c.inputs, head=c.head, hidden_act=c.act, normalize=c.norm)
    pol.set_exploration(ps.KEY, c.log_std)
    return v, pol, v.make_policy_grad(pol, max_rows)


def call(g, c, backward=True):
    piles = c.head == "piles"
    return g.grad(c.features, c.u, c.adv, pile_bits=pgl.pack_bits(c.on, c.S) if piles else None,
                  set_bits=pgl.pack_bits(c.sets, c.S) if (piles and c.sets is not None) else None, logp_old=c.logp_old, rows=c.rows,
                  adv_stats=c.adv_stats, loss=c.loss, clip_eps=c.clip_eps, ent_coef=c.ent_coef, backward=backward)


def within(got, r, what):
    """gradients, log-probabilities, entropies and stats within the restatement's bars; every figure is printed, then all are asserted"""
    bad = check_forward(got, r, what)
    d = np.abs(got["stats"] - r["stats"])
    print(what, "stats", got["stats"], "diff", d, "bar", r["bar_stats"])
    if not (got["stats"][0] == r["stats"][0] and got["stats"][4] == r["stats"][4] and (d <= r["bar_stats"]).all()):
        bad.append(("stats", got["stats"], r["stats"], r["bar_stats"]))
    d = np.abs(got["g_log_std"].astype(np.float64) - r["gls"])
    print(what, "g_log_std diff", d, "bar", r["bar_ls"])
    if not (d <= r["bar_ls"]).all():
        bad.append(("g_log_std", d, r["bar_ls"]))
    for l in range(len(r["gW"]) - 1, -1, -1):
        for name, dev, ref, bar in (("gW", got["grads"][l][0], r["gW"][l], r["bar_W"][l]), ("gb", got["grads"][l][1], r["gb"][l], r["bar_b"][l])):
            d = np.abs(dev.astype(np.float64) - ref)
            print(what, name, l, "max diff %.3e" % d.max(), "bar there %.3e" % bar.ravel()[d.argmax()], "largest |g| %.3e" % np.abs(ref).max())
            if not (d <= bar).all():
                bad.append((name, l, d.max(), bar.ravel()[d.argmax()], int((d > bar).sum()), d.size))
    assert not bad, (what, bad)


def check_forward(got, r, what):
    bad = []
    for name, ref, bar in (("logp_new", r["logp"], r["bar_logp"]), ("entropy", r["ent"], r["bar_ent"])):
        # (the f32 store adds half an ulp of the value)
        d, b = np.abs(got[name].astype(np.float64) - ref), bar + pl.U * np.abs(ref)
        print(what, name, "max diff %.3e" % d.max(), "bar there %.3e" % b[d.argmax()])
        if not (d <= b).all():
            bad.append((name, d.max(), b[d.argmax()], int((d > b).sum()), d.size))
    return bad


# ---- 1. exact data: no tolerance at all
@pytest.mark.parametrize("n_layers,hidden", [(1, (33, 64, 31)), (2, (33, 64, 31)), (3, (33, 64, 31)), (4, (33, 64, 31)), (3, pgl.EXACT_WIDE)],
                         ids=["1", "2", "3", "4", "3-tiles_in_the_partials"])
def test_exact_gradients_bit_for_bit(n_layers, hidden):
    """LOADS, relu, log_std = 0, dyadic data, COEF: gW, gb and g_log_std equal the f64 restatement's f32 rounding for R = 1, 31, 32, 33,
    95 and 300 -- with ceil(R / 32) no multiple of 8 the last workgroups walk no tile and contribute zeros (R = 33: six of eight).
    Hidden (256, 64) has 26 dW tiles: the form that reads and writes them in the workgroup's slice of the partials, and the merge's
    offsets into 26 tiles, with no tolerance either"""
    c0 = pgl.exact_case(n_layers, 300, hidden=hidden)
    assert (pgl.plan(c0.piles, widths_of(c0), 300, "loads", "relu")[1]["in_registers"] == 0) == (hidden == pgl.EXACT_WIDE)
    v, pol, g = actor(c0, 300)
    for R in pgl.R_LIST + (300,):
        c = pgl.exact_case(n_layers, R, hidden=hidden)
        assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(c.layers, c0.layers))
        got = call(g, c)
        gW, gb, gls = pgl.exact_expected(c)
        for l in range(n_layers):
            assert np.array_equal(got["grads"][l][0], gW[l]), (R, "gW", l, np.abs(got["grads"][l][0] - gW[l]).max())
            assert np.array_equal(got["grads"][l][1], gb[l]), (R, "gb", l)
        assert np.array_equal(got["g_log_std"], gls), (R, got["g_log_std"], gls)
        assert got["stats"][0] == R
    close_all(g, pol, v)


# ---- 2. alignments, widths, depths, activations, losses, R: made rollouts
CASES = pgl.gpu_general_cases()


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name + "-" + c.loss)
def test_gradients_within_the_bar(c):
    r = pgl.restate(c, tpw_of(c))
    pgl.check_conditions(c, r)
    v, pol, g = actor(c, c.R)
    got = call(g, c)
    within(got, r, c.name)
    # the forward alone writes the same bits, and twice the same call gives the same bits
    fwd = call(g, c, backward=False)
    assert fwd["grads"] is None and np.array_equal(fwd["logp_new"].view(np.uint32), got["logp_new"].view(np.uint32))
    assert np.array_equal(fwd["entropy"].view(np.uint32), got["entropy"].view(np.uint32))
    again = call(g, c)
    for (a, b), (a2, b2) in zip(got["grads"], again["grads"]):
        assert np.array_equal(a.view(np.uint32), a2.view(np.uint32)) and np.array_equal(b.view(np.uint32), b2.view(np.uint32))
    assert np.array_equal(got["g_log_std"].view(np.uint32), again["g_log_std"].view(np.uint32)) and np.array_equal(got["stats"], again["stats"])
    close_all(g, pol, v)


# ---- 3. rollouts really collected
def collected_case(v, pol, roll, T, layers, ls, norm, rs):
    h = roll.host()
    n, S, D = v.n_envs, v.n_slots, v.obs_dim
    on = pl.unpack_bits(h["bits"][:T].reshape(T * n, -1), S)
    sets = pl.unpack_bits(h["set"][:T].reshape(T * n, -1), S)
    adv = (rs.normal(size=T * n) + 0.3).astype(F32)
    return pgl.Case(layers=layers, log_std=ls, norm=norm, act="tanh", head="piles", S=S, features=f32(h["feat"])[:T].reshape(T * n, D).copy(), on=on,
                    sets=sets, u=f32(h["u"])[:T].reshape(T * n, 2).copy(), logp_old=f32(h["logp"])[:T].reshape(T * n).copy(), adv=adv, loss="ppo_clip",
                    clip_eps=0.2, ent_coef=0.01, piles=[20, 25], hidden=(33,), name="collected")


@pytest.mark.parametrize("mode", ["lockstep", "autoreset"])
@pytest.mark.parametrize("rng", ["philox", "philox_curves"])
def test_collected_rollouts(rng, mode):
    """collect(logp_piles="decidable"), T = 6 at 64 envs, under a normaliser taken from a first rollout's features.  Unchanged parameters:
    |logp_new - logp| within the re-derivation's bound, nothing clipped at eps = 0.2, the mean ratio within that bound of 1.  Then every
    weight moves by a step that clips rows in both directions (asserted on the restatement), and the gradient lies within the bar."""
    T, piles = 6, [20, 25]
    rs = np.random.RandomState(31 + (rng == "philox") + 2 * (mode == "lockstep"))
    v = make(rng, piles, N_ENVS, seed=6)
    D = v.obs_dim
    layers = pgl.general_layers(rs, [D, 33, v.act_dim])
    ls = np.array([-0.2, 0.1], dtype=F32)
    pol = v.make_policy(layers, normalize=(np.zeros(D, dtype=F32), np.ones(D, dtype=F32), 3.0))
    pol.set_exploration(77, ls)
    roll = RollSet(v, pol, T)
    if mode == "autoreset":
        v.reset_device(roll.ptr("obs0"))
    roll.collect_set(mode, "decidable")
    feats = f32(roll.host()["feat"]).reshape(T * N_ENVS, D).astype(np.float64)
    norm = (feats.mean(axis=0).astype(F32), (1.0 / np.sqrt(feats.var(axis=0) + 1e-2)).astype(F32), 3.0)
    pol.set_normalizer(norm[0], norm[1])
    roll.buf["obs0"].from_host(f32(roll.host()["packed"])[T - 1, :, :D].copy())
    roll.collect_set(mode, "decidable", first=T)
    c = collected_case(v, pol, roll, T, layers, ls, norm, rs)
    assert c.sets.any() and not c.sets.all()
    g = v.make_policy_grad(pol, c.R)
    # unchanged parameters
    r0 = pgl.restate(c, tpw_of(c))
    got0 = call(g, c)
    # (the issue's bound: the Gaussian re-derivation's G terms and the re-rounded partial sums; z and the pile terms are the recorded bits)
    d = np.abs(got0["logp_new"].astype(np.float64) - c.logp_old.astype(np.float64))
    bound = pgl.rederivation_bound(r0)
    print("unchanged: max |logp_new - logp| %.3e, bound there %.3e, largest bound %.3e (the forward bar: %.3e)"
          % (d.max(), bound[d.argmax()], bound.max(), r0["bar_logp"].max()))
    assert (d <= bound).all(), (d.max(), bound[d.argmax()])
    assert got0["stats"][0] == c.R and got0["stats"][4] == 0
    assert abs(got0["stats"][5] / c.R - 1.0) <= pgl.ratio_bound(bound.max()), (got0["stats"][5] / c.R, bound.max())
    # a step
    new = pgl.perturbed(rs, layers, 0.35)
    ls_new = (ls + F32(0.05)).astype(F32)
    for l, (W, b) in enumerate(new):
        pol.set_weights(l, W, b)
    pol.set_exploration(77, ls_new)
    c1 = pgl.separate_ratios(c.copy(layers=new, log_std=ls_new))
    r1 = pgl.restate(c1, tpw_of(c1))
    pgl.check_conditions(c1, r1)
    up, down = pgl.clipped_both_ways(c1, r1)
    print("clipped away: %d with A >= 0, %d with A < 0, of %d; ratios %.3f .. %.3f" % (up, down, c1.R, r1["ratio"].min(), r1["ratio"].max()))
    assert up >= 1 and down >= 1
    within(call(g, c1), r1, "collected-%s-%s" % (rng, mode))
    close_all(g, roll, pol, v)


# ---- 4. minibatches
def test_minibatches_by_rows_add_up():
    """a seeded permutation of the 95 rows cut into minibatches of 40, 32 and 23: the sum of R_mb * gradient equals R * the full-batch
    gradient within the bars added; each minibatch within its own bar; a repeated index counts twice"""
    c = [x for x in CASES if x.name == "20x25-33-tanh-piles-95"][0]
    v, pol, g = actor(c, c.R)
    full = call(g, c)
    r = pgl.restate(c, tpw_of(c))
    perm = np.random.RandomState(4).permutation(c.R).astype(np.int64)
    sums = [[np.zeros(W.shape), np.zeros(b.shape)] for W, b in c.layers]
    bars = [[np.zeros(W.shape), np.zeros(b.shape)] for W, b in c.layers]
    for lo, hi in ((0, 40), (40, 72), (72, 95)):
        cm = pgl.separate_ratios(c.copy(rows=perm[lo:hi]))
        assert np.array_equal(cm.logp_old, c.logp_old)
        rm = pgl.restate(cm, tpw_of(cm))
        gm = call(g, cm)
        within(gm, rm, "minibatch %d:%d" % (lo, hi))
        for l in range(len(c.layers)):
            for k, bar in ((0, rm["bar_W"][l]), (1, rm["bar_b"][l])):
                sums[l][k] += (hi - lo) * gm["grads"][l][k].astype(np.float64)
                bars[l][k] += (hi - lo) * bar
    for l in range(len(c.layers)):
        for k, bar in ((0, r["bar_W"][l]), (1, r["bar_b"][l])):
            d = np.abs(sums[l][k] - c.R * full["grads"][l][k].astype(np.float64))
            assert (d <= bars[l][k] + c.R * bar).all(), (l, k, d.max())
    twice = pgl.separate_ratios(c.copy(rows=np.array([7, 7, 20, 3, 7, 94], dtype=np.int64)))
    within(call(g, twice), pgl.restate(twice, 1), "repeated rows")
    close_all(g, pol, v)


# ---- 5. determinism, graphs, new weights between replays
class DevCase(object):
    """a case's arrays in device memory and the outputs of a call.  tail None: the buffers of the determinism test (no d_rows, no
    advantage statistics, no entropy); a number: all of the case's inputs and every output, NaN over the outputs before a call, logp_new
    and entropy `tail` positions longer than R (nothing may write those)"""

    def __init__(self, c, tail=None):
        mg = buffers()
        self.c, self.tail = c, tail
        piles = c.head == "piles"
        ins = dict(features=c.features, u=c.u, adv=c.adv, logp_old=c.logp_old)
        if tail is not None and c.rows is not None:
            ins["rows"] = np.asarray(c.rows, dtype=np.int64)
        if tail is not None and c.adv_stats is not None:
            ins["adv_stats"] = np.asarray(c.adv_stats, dtype=np.float64)
        if piles:
            ins["bits"] = pgl.pack_bits(c.on, c.S)
            if c.sets is not None:
                ins["sets"] = pgl.pack_bits(c.sets, c.S)
        self.shapes = [(W.shape, b.shape) for W, b in c.layers]
        self.buf = {}
        for k, a in ins.items():
            a = np.ascontiguousarray(a)
            self.buf[k] = mg.DeviceBuffer(a.nbytes)
            self.buf[k].from_host(a)
        for l, (ws, bs) in enumerate(self.shapes):
            for k, s in (("gW%d" % l, ws), ("gb%d" % l, bs), ("W%d" % l, ws), ("b%d" % l, bs)):
                self.buf[k] = mg.DeviceBuffer(int(np.prod(s)) * 4)
        self.buf["gls"], self.buf["logp_new"], self.buf["stats"] = mg.DeviceBuffer(16), mg.DeviceBuffer(4 * (c.R + (tail or 0))), mg.DeviceBuffer(48)
        if tail is not None:
            self.buf["entropy"] = mg.DeviceBuffer(4 * (c.R + tail))
            self.clear(np.nan)

    def p(self, k):
        return self.buf[k].ptr if k in self.buf else 0

    def run(self, g, stream=0, backward=True):
        c, L = self.c, len(self.shapes)
        g.grad_device(c.R, len(c.features), self.p("features"), self.p("u"), self.p("adv"), self.p("bits"), self.p("sets"), self.p("logp_old"),
                      d_rows=self.p("rows"), d_adv_stats=self.p("adv_stats"), loss=c.loss, clip_eps=c.clip_eps, ent_coef=c.ent_coef,
                      d_gW=[self.p("gW%d" % l) for l in range(L)] if backward else None, d_gb=[self.p("gb%d" % l) for l in range(L)] if backward else None,
                      d_glog_std=self.p("gls") if backward else 0, d_logp_new=self.p("logp_new"), d_entropy=self.p("entropy"), d_stats=self.p("stats"),
                      stream=stream)

    def put_weights(self, layers):
        for l, (W, b) in enumerate(layers):
            self.buf["W%d" % l].from_host(np.ascontiguousarray(W, dtype=F32))
            self.buf["b%d" % l].from_host(np.ascontiguousarray(b, dtype=F32))

    def clear(self, fill=0.0):
        """zeros (or `fill`) over every output, so that what is read next was written by the call in between"""
        for l, (ws, bs) in enumerate(self.shapes):
            self.buf["gW%d" % l].from_host(np.full(ws, fill, dtype=F32))
            self.buf["gb%d" % l].from_host(np.full(bs, fill, dtype=F32))
        self.buf["gls"].from_host(np.full(4, fill, dtype=F32))
        for k in ("logp_new", "entropy") if "entropy" in self.buf else ("logp_new",):
            self.buf[k].from_host(np.full(self.c.R + (self.tail or 0), fill, dtype=F32))
        self.buf["stats"].from_host(np.full(6, fill, dtype=np.float64))

    def out(self):
        res = []
        for l, (ws, bs) in enumerate(self.shapes):
            res += [self.buf["gW%d" % l].to_host(np.uint32, ws), self.buf["gb%d" % l].to_host(np.uint32, bs)]
        return res + [self.buf["gls"].to_host(np.uint32, (4,))[:2], self.buf["logp_new"].to_host(np.uint32, (self.c.R,)), self.buf["stats"].to_host(np.uint64, (6,))]

    def result(self):
        """(a DevCase with a tail) -> what `call` returns, from these buffers: dict(grads [(gW, gb)], g_log_std, logp_new, entropy [R],
        stats), and past = the positions of logp_new and entropy from R on"""
        R, G = self.c.R, len(self.c.log_std)
        grads = [(f32(self.buf["gW%d" % l].to_host(np.uint32, ws)), f32(self.buf["gb%d" % l].to_host(np.uint32, bs))) for l, (ws, bs) in enumerate(self.shapes)]
        lp, en = (f32(self.buf[k].to_host(np.uint32, (R + self.tail,))) for k in ("logp_new", "entropy"))
        return dict(grads=grads, g_log_std=f32(self.buf["gls"].to_host(np.uint32, (4,)))[:G].copy(), logp_new=lp[:R].copy(), entropy=en[:R].copy(),
                    stats=self.buf["stats"].to_host(np.uint64, (6,)).view(np.float64), past=np.concatenate([lp[R:], en[R:]]))

    def free(self):
        for b in self.buf.values():
            b.free()


def test_two_calls_a_graph_and_new_weights_between_replays():
    mg = buffers()
    c = [x for x in CASES if x.name == "20x25-33-tanh-piles-95"][0]
    v, pol, g = actor(c, c.R)
    d = DevCase(c)
    st = mg.Stream(0)
    d.run(g, st.ptr)
    st.sync()
    eager = d.out()
    d.run(g, st.ptr)
    st.sync()
    assert all(np.array_equal(a, b) for a, b in zip(eager, d.out())), "two calls, the same bits"
    # (a handle's graph covers an even number of resets + steps and ends at the clock it began at: two days, and the gradient call, which
    # takes no tick, in the middle of the second)
    acts, packed, obs0 = mg.DeviceBuffer(N_ENVS * v.act_dim * 4), mg.DeviceBuffer(N_ENVS * (v.obs_dim + 2) * 4), mg.DeviceBuffer(N_ENVS * v.obs_dim * 4)
    v.random_actions_device(acts.ptr, 5, 0, st.ptr)
    st.sync()
    v.graph_begin(st.ptr)
    for i in range(192):
        if i % 96 == 0:
            v.reset_device(obs0.ptr, stream=st.ptr)
        v.step_device_packed(acts.ptr, packed.ptr, stream=st.ptr)
        if i == 130:
            d.run(g, st.ptr)
    graph = v.graph_end(st.ptr)
    st.sync()
    d.clear()
    v.graph_launch(graph, st.ptr)
    st.sync()
    assert all(np.array_equal(a, b) for a, b in zip(eager, d.out())), "a replay equals the eager call"
    # new weights in the trainer's layout, on the stream: the next replay differentiates them (the row-major copies are rebuilt per call)
    rs = np.random.RandomState(12)
    new = pgl.perturbed(rs, c.layers, 0.1)
    d.put_weights(new)
    for l in range(len(new)):
        pol.set_weights_device(l, d.p("W%d" % l), d.p("b%d" % l), stream=st.ptr)
    v.graph_launch(graph, st.ptr)
    st.sync()
    replay = d.out()
    assert not np.array_equal(replay[0], eager[0]) and not np.array_equal(replay[-2], eager[-2])
    c2 = pgl.separate_ratios(c.copy(layers=new))
    assert np.array_equal(c2.logp_old, c.logp_old), "no ratio moved onto a bound"
    r2 = pgl.restate(c2, tpw_of(c2))
    got = dict(grads=[(f32(replay[2 * l]), f32(replay[2 * l + 1])) for l in range(len(new))], g_log_std=f32(replay[-3]))
    for l in range(len(new)):
        assert (np.abs(got["grads"][l][0].astype(np.float64) - r2["gW"][l]) <= r2["bar_W"][l]).all(), l
        assert (np.abs(got["grads"][l][1].astype(np.float64) - r2["gb"][l]) <= r2["bar_b"][l]).all(), l
    assert (np.abs(got["g_log_std"].astype(np.float64) - r2["gls"]) <= r2["bar_ls"]).all()
    v.graph_destroy(graph)
    close_all(d, acts, packed, obs0, g, pol, v)
    st.destroy()


# ---- 7. the normaliser
def test_the_gradient_follows_a_normaliser_from_moments():
    c = [x for x in CASES if x.name == "20x25-33-relu-piles-95"][0]
    assert c.norm is not None
    v, pol, g = actor(c, c.R)
    before = call(g, c)
    mg = buffers()
    D = c.features.shape[1]
    m = v.make_moments(D)
    fb = mg.DeviceBuffer(c.features.nbytes)
    fb.from_host(c.features)
    m.update_device(fb.ptr, len(c.features), ld=D)
    pol.normalizer_from_moments(m, eps=1e-2)
    v.sync()
    mean, inv_std = pol.normalizer()
    assert not np.array_equal(mean, c.norm[0])
    c2 = pgl.separate_ratios(c.copy(norm=(mean, inv_std, c.norm[2])))
    assert np.array_equal(c2.logp_old, c.logp_old)
    after = call(g, c2)
    assert not np.array_equal(after["grads"][0][0], before["grads"][0][0])
    within(after, pgl.restate(c2, tpw_of(c2)), "normaliser from moments")
    fb.free()
    close_all(m, g, pol, v)


# ---- 8. refusals
def test_refusals_come_with_a_message_and_before_any_device_work():
    mg = buffers()
    c = [x for x in CASES if x.name == "20x25-33-tanh-piles-95"][0]
    v = make("philox", c.piles, N_ENVS)
    lib = v._lib
    pol = v.make_policy(c.layers, hidden_act=c.act)

    def refused(code, text, rc):
        msg = lib.chub_last_error().decode()
        assert rc == code and text in msg, (rc, msg)

    h = C.c_void_p()
    refused(-1, "chub_policy_set_exploration first", lib.chub_policy_grad_create(pol._p, 64, C.byref(h)))
    pol.set_exploration(1, c.log_std)
    refused(-1, "max_rows", lib.chub_policy_grad_create(pol._p, 0, C.byref(h)))
    big = v.make_policy(pgl.general_layers(np.random.RandomState(0), [v.obs_dim, 256, 200, 256, v.act_dim]))
    big.set_exploration(1, c.log_std)
    refused(-4, "LDS", lib.chub_policy_grad_create(big._p, 64, C.byref(h)))
    g = v.make_policy_grad(pol, 64)
    st = mg.Stream(0)
    buf = mg.DeviceBuffer(1 << 16)
    p = buf.ptr
    v.graph_begin(st.ptr)
    refused(-4, "chub_graph_begin", lib.chub_policy_grad_create(pol._p, 64, C.byref(h)))
    refused(-4, "chub_graph_begin", lib.chub_policy_grad_destroy(g._g))
    v.reset_device(p, stream=st.ptr)  # (a graph covers an even, non-zero number of resets + steps)
    v.reset_device(p, stream=st.ptr)
    v.graph_destroy(v.graph_end(st.ptr))
    st.sync()

    def args(**kw):
        a = dict(R=64, n_rows=64, d_rows=None, d_features=p, ld_features=v.obs_dim, d_pile_bits=p, d_set_bits=None, d_u=p, d_logp_old=p, d_adv=p,
                 d_adv_stats=None, loss=1, clip_eps=0.2, ent_coef=0.0, pad_=0)
        a.update(kw)
        return _lib.ChubPolicyGradIn(**a)

    out = _lib.ChubPolicyGradOut()
    out.d_logp_new = p
    run = lambda gg, **kw: lib.chub_policy_grad_device(gg._g, C.byref(args(**kw)), C.byref(out), None)
    assert run(g) == 0
    for field in ("d_features", "d_u", "d_adv", "d_pile_bits", "d_logp_old"):
        refused(-1, "null argument", run(g, **{field: None}))
    refused(-1, "null argument", lib.chub_policy_grad_device(g._g, None, C.byref(out), None))
    refused(-1, "null argument", lib.chub_policy_grad_device(g._g, C.byref(args()), None, None))
    assert run(g, loss=0, d_logp_old=None) == 0, "COEF does not read logp_old"
    refused(-1, "max_rows", run(g, R=0))
    refused(-1, "max_rows", run(g, R=65))
    refused(-1, "n_rows", run(g, n_rows=0))
    refused(-1, "n_rows", run(g, n_rows=32))
    refused(-1, "ld_features", run(g, ld_features=v.obs_dim - 1))
    refused(-1, "loss", run(g, loss=2))
    for e in (0.0, 1.0, -0.1, float("nan")):
        refused(-1, "clip_eps", run(g, clip_eps=e))
    for e in (float("inf"), float("nan")):
        refused(-1, "ent_coef", run(g, ent_coef=e))
    loads = v.make_policy(pgl.general_layers(np.random.RandomState(1), [v.obs_dim, 33, 4]), head="loads")
    loads.set_exploration(1, np.zeros(4, dtype=F32))
    gl = v.make_policy_grad(loads, 64)
    refused(-1, "d_set_bits must be NULL", run(gl, d_set_bits=p))
    assert run(gl, d_pile_bits=None) == 0
    v.sync()
    # chub_destroy frees a handle's grad objects with their policies
    buf.free()
    st.destroy()
    gl._g = g._g = None
    close_all(loads, big, pol, v)


# ---- 9. the torch adapter
TORCH_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["CHUB_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHUB_ROOT"], "tests"))
import torch  # before libchub: both must share one HIP runtime
torch.cuda.set_device(0)
import test_gpu_policy_grad
test_gpu_policy_grad.torch_adapter_policy_gradient()
print("TORCH_POLICY_GRAD_OK")
"""


def test_torch_adapter_policy_gradient_against_cuda_autograd():
    """in a child process that imports torch first (as tests/test_gpu_torch_side.py does)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], env=dict(os.environ, CHUB_ROOT=root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TORCH_POLICY_GRAD_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def torch_adapter_policy_gradient():
    import torch
    from charginghub_env_amd import wrappers
    n, T = N_ENVS, 6
    kw = {k: BASE[k] for k in BASE if k != "station_type_list"}
    rs = np.random.RandomState(5)
    env = wrappers.TorchHubVecEnv(n, [20, 25], ["fast", "slow"], seed=13, autoreset="per_env", **kw)
    D, A, S, W = env.obs_dim, env.act_dim, env.vec.n_slots, env.vec.bit_words
    layers = pgl.general_layers(rs, [D, 33, A])
    net = torch.nn.Sequential(torch.nn.Linear(D, 33), torch.nn.Tanh(), torch.nn.Linear(33, A)).to("cuda")
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, (Wl, bl) in zip(lin, layers):
            m.weight.copy_(torch.tensor(Wl))
            m.bias.copy_(torch.tensor(bl))
    pol = env.load_policy(net)
    log_std = torch.tensor([-0.2, 0.1], device="cuda")
    pol.set_exploration(21, log_std.cpu().numpy())
    env.reset()
    ro = env.collect(pol, T, logp_piles="decidable")
    adv = torch.tensor((rs.normal(size=(T, n)) + 1.0).astype(F32), device="cuda")
    # unchanged: evaluate_actions returns the recorded log-probabilities up to the re-derivation
    lp, en = env.evaluate_actions(ro)
    assert tuple(lp.shape) == (T * n,) and bool(torch.isfinite(en).all())
    c0 = pgl.Case(layers=layers, log_std=log_std.cpu().numpy(), act="tanh", head="piles", S=S, features=ro["features"].cpu().numpy().reshape(T * n, D),
                  on=pl.unpack_bits(ro["bits"].cpu().numpy().view(np.uint64).reshape(T * n, W), S),
                  sets=pl.unpack_bits(ro["set_bits"].cpu().numpy().view(np.uint64).reshape(T * n, W), S), u=ro["u"].cpu().numpy().reshape(T * n, 2),
                  logp_old=ro["logp"].cpu().numpy().reshape(T * n), adv=adv.cpu().numpy().reshape(T * n), loss="coef", piles=[20, 25], hidden=(33,))
    same = pgl.rederivation_bound(pgl.restate(c0))
    moved = np.abs(lp.cpu().numpy().astype(np.float64) - c0.logp_old.astype(np.float64))
    assert (moved <= same).all(), (moved.max(), same[moved.argmax()])
    # a step, pushed to the device from the parameters' own memory
    with torch.no_grad():
        for m, (Wl, bl) in zip(lin, pgl.perturbed(rs, layers, 0.25)):
            m.weight.copy_(torch.tensor(Wl))
            m.bias.copy_(torch.tensor(bl))
        log_std += 0.05
    for l, m in enumerate(lin):
        pol.set_weights_device(l, m.weight.data_ptr(), m.bias.data_ptr(), stream=env._stream())
    pol.set_log_std_device(log_std.data_ptr(), stream=env._stream())
    for rows in (None, torch.tensor(rs.permutation(T * n)[:100].astype(np.int64), device="cuda")):
        grads, gls, stats = env.policy_gradient(ro, adv, rows=rows, loss="ppo_clip", clip_eps=0.2, ent_coef=0.01)
        torch.cuda.synchronize()
        new = [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in lin]
        c = pgl.Case(layers=new, log_std=log_std.cpu().numpy(), act="tanh", head="piles", S=S, features=ro["features"].cpu().numpy().reshape(T * n, D),
                     on=pl.unpack_bits(ro["bits"].cpu().numpy().view(np.uint64).reshape(T * n, W), S),
                     sets=pl.unpack_bits(ro["set_bits"].cpu().numpy().view(np.uint64).reshape(T * n, W), S), u=ro["u"].cpu().numpy().reshape(T * n, 2),
                     logp_old=ro["logp"].cpu().numpy().reshape(T * n), adv=adv.cpu().numpy().reshape(T * n), loss="ppo_clip", clip_eps=0.2, ent_coef=0.01,
                     rows=None if rows is None else rows.cpu().numpy(), piles=[20, 25], hidden=(33,))
        # (ties are not defined: a recorded logp whose ratio falls within 2e-3 of a bound is moved by 8e-3, on the device too)
        c = pgl.separate_ratios(c)
        ro["logp"].copy_(torch.tensor(c.logp_old, device="cuda").reshape(T, n))
        grads, gls, stats = env.policy_gradient(ro, adv, rows=rows, loss="ppo_clip", clip_eps=0.2, ent_coef=0.01)
        torch.cuda.synchronize()
        r = pgl.restate(c, tpw_of(c))
        pgl.check_conditions(c, r)
        # CUDA autograd of an f64 copy of the network through the wrappers' own functions
        net64 = torch.nn.Sequential(torch.nn.Linear(D, 33), torch.nn.Tanh(), torch.nn.Linear(33, A)).double().to("cuda")
        lin64 = [m for m in net64 if isinstance(m, torch.nn.Linear)]
        with torch.no_grad():
            for a, b in zip(lin64, lin):
                a.weight.copy_(b.weight.double())
                a.bias.copy_(b.bias.double())
        ls64 = log_std.double().clone().requires_grad_(True)
        idx = slice(None) if rows is None else rows
        flat = lambda t: t.reshape(T * n, *t.shape[2:])[idx]
        z = net64(flat(ro["features"]).double())
        lp64 = wrappers.sampled_logp(z, flat(ro["bits"]), flat(ro["u"]).double(), ls64, piles=flat(ro["set_bits"]))
        en64 = wrappers.sampled_entropy(z, ls64, piles=flat(ro["set_bits"]))
        Aa = flat(adv).double()
        ratio = torch.exp(lp64 - flat(ro["logp"]).double())
        lo, hi = float(F32(1) - F32(0.2)), float(F32(1) + F32(0.2))
        loss = (-torch.minimum(ratio * Aa, torch.clamp(ratio, lo, hi) * Aa) - float(F32(0.01)) * en64).mean()
        loss.backward()
        for l, m in enumerate(lin64):
            assert (np.abs(grads[l][0].cpu().numpy().astype(np.float64) - m.weight.grad.cpu().numpy()) <= r["bar_W"][l]).all(), ("gW", l)
            assert (np.abs(grads[l][1].cpu().numpy().astype(np.float64) - m.bias.grad.cpu().numpy()) <= r["bar_b"][l]).all(), ("gb", l)
        assert (np.abs(gls.cpu().numpy().astype(np.float64) - ls64.grad.cpu().numpy()) <= r["bar_ls"]).all()
        st = stats.cpu().numpy()
        assert st[0] == c.R and st[4] == r["stats"][4] and abs(st[1] / c.R - float(loss)) <= r["bar_stats"][1] / c.R + 1e-12
    env.close()
