"""The critic on the device (include/chub.h, "a critic on the device") against tests/critic_lib.py's f64 restatement: (1) exact data, bit
for bit, for every layer count, every R and both losses; (2) widths, depths, activations, the normaliser, rows and strides within the
derived bar; (3) the actor's chain: a PILES / CLIP actor whose head row S is the critic's head forms the same bits; (4) the values call;
(5) minibatches by d_rows; (6) two calls, a captured graph, new weights and a new normaliser between replays; (7) collected rollouts
through TorchHubVecEnv.values / advantages / value_gradient; (8) every refusal; (9) the torch adapter against CUDA autograd."""
import ctypes as C

import numpy as np
import pytest

import critic_lib as cl
import policy_lib as pl
from charginghub_env_amd import _lib
from test_gpu_autoreset import buffers
from test_gpu_pile_obs import BASE, make
from test_gpu_policy import f32
from test_gpu_policy_sample import close_all

pytestmark = pytest.mark.gpu
F32 = np.float32
N_ENVS = 64


def critic_of(c, max_rows, v=None):
    v = v or make("philox", [3, 2], N_ENVS)
    return v, v.make_critic(c.layers, hidden_act=c.act, normalize=c.norm, max_rows=max_rows)


def padded(c):
    """the case's rows as the device sees them: row stride ld >= F, the padding full of NaN (nothing may read it)"""
    if not c.ld:
        return c.x
    x = np.full((len(c.x), c.ld), np.nan, dtype=F32)
    x[:, :c.F] = c.x
    return x


class DevCase(object):
    """a case's arrays in device memory and the outputs of a call; tail: positions the two values buffers hold past R (nothing may write them)"""

    def __init__(self, c, tail=0):
        mg = buffers()
        self.c, self.tail = c, tail
        self.shapes = [(W.shape, b.shape) for W, b in c.layers]
        self.buf = {}
        ins = dict(x=padded(c), ret=c.ret, v_old=c.v_old)
        if c.rows is not None:
            ins["rows"] = np.asarray(c.rows, dtype=np.int64)
        for k, a in ins.items():
            a = np.ascontiguousarray(a)
            self.buf[k] = mg.DeviceBuffer(a.nbytes)
            self.buf[k].from_host(a)
        for l, (ws, bs) in enumerate(self.shapes):
            for k, s in (("gW%d" % l, ws), ("gb%d" % l, bs), ("W%d" % l, ws), ("b%d" % l, bs)):
                self.buf[k] = mg.DeviceBuffer(int(np.prod(s)) * 4)
        self.buf["values"], self.buf["values2"], self.buf["stats"] = mg.DeviceBuffer(4 * (c.R + tail)), mg.DeviceBuffer(4 * (c.R + tail)), mg.DeviceBuffer(48)
        self.clear()

    def p(self, k):
        return self.buf[k].ptr if k in self.buf else 0

    def run(self, cr, stream=0, backward=True, loss=None):
        c, L = self.c, len(self.shapes)
        cr.grad_device(c.R, len(c.x), self.p("x"), self.p("ret"), self.p("v_old"), self.p("rows"), c.ld, loss or c.loss, c.clip_eps,
                       [self.p("gW%d" % l) for l in range(L)] if backward else None, [self.p("gb%d" % l) for l in range(L)] if backward else None,
                       self.p("values"), self.p("stats"), stream)

    def run_values(self, cr, stream=0):
        c = self.c
        cr.values_device(c.R, len(c.x), self.p("x"), self.p("values2"), self.p("rows"), c.ld, stream)

    def put_weights(self, layers):
        for l, (W, b) in enumerate(layers):
            self.buf["W%d" % l].from_host(np.ascontiguousarray(W, dtype=F32))
            self.buf["b%d" % l].from_host(np.ascontiguousarray(b, dtype=F32))

    def clear(self):
        """a NaN pattern over every output, so that what is read next was written by the call in between"""
        for l, (ws, bs) in enumerate(self.shapes):
            self.buf["gW%d" % l].from_host(np.full(ws, np.nan, dtype=F32))
            self.buf["gb%d" % l].from_host(np.full(bs, np.nan, dtype=F32))
        for k in ("values", "values2"):
            self.buf[k].from_host(np.full(self.c.R + self.tail, np.nan, dtype=F32))
        self.buf["stats"].from_host(np.full(6, np.nan, dtype=np.float64))

    def out(self):
        """-> dict(grads [(gW, gb)], values, values2, stats), f32 / f64; with a tail also past = the two buffers' positions from R on"""
        grads = [(f32(self.buf["gW%d" % l].to_host(np.uint32, ws)), f32(self.buf["gb%d" % l].to_host(np.uint32, bs))) for l, (ws, bs) in enumerate(self.shapes)]
        R = self.c.R
        val, val2 = (f32(self.buf[k].to_host(np.uint32, (R + self.tail,))) for k in ("values", "values2"))
        res = dict(grads=grads, values=val[:R].copy(), values2=val2[:R].copy(), stats=self.buf["stats"].to_host(np.uint64, (6,)).view(np.float64))
        if self.tail:
            res["past"] = np.concatenate([val[R:], val2[R:]])
        return res

    def free(self):
        for b in self.buf.values():
            b.free()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == F32 else np.uint64)


def same_bits(a, b):
    return all(np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(bits(x[1]), bits(y[1])) for x, y in zip(a["grads"], b["grads"])) and \
        np.array_equal(bits(a["values"]), bits(b["values"])) and np.array_equal(bits(a["stats"]), bits(b["stats"]))


def call(cr, c, backward=True, tail=0):
    """one gradient call and the values call on the case, through device buffers of their own"""
    d = DevCase(c, tail)
    d.run(cr, backward=backward)
    d.run_values(cr)
    cr._env.sync()
    got = d.out()
    d.free()
    return got


def within(got, r, what, grads=True):
    """values, stats and gradients within the restatement's bars; every figure is printed, then all are asserted"""
    bad = []
    dv, bv = np.abs(got["values"].astype(np.float64) - r["values"]), r["bar_v"] + pl.U * np.abs(r["values"])  # (the f32 store: half an ulp)
    print(what, "values max diff %.3e" % dv.max(), "bar there %.3e" % bv[dv.argmax()])
    if not (dv <= bv).all() or not (got["values"][~r["ok"]] == 0).all():
        bad.append(("values", dv.max(), bv[dv.argmax()]))
    d = np.abs(got["stats"] - r["stats"])
    print(what, "stats", got["stats"], "diff", d, "bar", r["bar_stats"])
    if not (got["stats"][0] == r["stats"][0] and got["stats"][2] == r["stats"][2] and (d <= r["bar_stats"]).all()):
        bad.append(("stats", got["stats"], r["stats"], r["bar_stats"]))
    for l in range(len(r["gW"]) - 1, -1, -1) if grads else ():
        for name, dev, ref, bar in (("gW", got["grads"][l][0], r["gW"][l], r["bar_W"][l]), ("gb", got["grads"][l][1], r["gb"][l], r["bar_b"][l])):
            d = np.abs(dev.astype(np.float64) - ref)
            print(what, name, l, "max diff %.3e" % d.max(), "bar there %.3e" % bar.ravel()[d.argmax()], "largest |g| %.3e" % np.abs(ref).max())
            if not (d <= bar).all():
                bad.append((name, l, d.max(), bar.ravel()[d.argmax()], int((d > bar).sum()), d.size))
    assert not bad, (what, bad)


# ---- 1. exact data: no tolerance at all
@pytest.mark.parametrize("n_layers,hidden", [(1, cl.EXACT_HIDDEN), (2, cl.EXACT_HIDDEN), (3, cl.EXACT_HIDDEN), (4, cl.EXACT_HIDDEN), (3, cl.EXACT_WIDE)],
                         ids=["1", "2", "3", "4", "3-tiles_in_the_partials"])
def test_exact_gradients_bit_for_bit(n_layers, hidden):
    """relu, dyadic data, MSE and CLIPPED with rows on both sides of the predicate: gW, gb, values and all six stats equal the f64
    restatement's rounding for R = 1, 31, 32, 33, 95 and 300 -- with ceil(R / 32) no multiple of 8 the last workgroups walk no tile and
    contribute zeros.  Hidden (256, 64) has 26 dW tiles: the form that keeps them in the workgroup's slice of the partials"""
    c0 = cl.exact_case(n_layers, 300, hidden=hidden)
    assert (cl.plan(c0.F, c0.sizes[1:], 300, "relu")[1]["in_registers"] == 0) == (hidden == cl.EXACT_WIDE)
    v, cr = critic_of(c0, 300)
    for R in cl.EXACT_R:
        for loss in ("mse", "clipped"):
            c = cl.exact_case(n_layers, R, loss, hidden=hidden)
            assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(c.layers, c0.layers))
            got = call(cr, c)
            gW, gb, val, stats = cl.exact_expected(c)
            for l in range(n_layers):
                assert np.array_equal(got["grads"][l][0], gW[l]), (R, loss, "gW", l, np.abs(got["grads"][l][0] - gW[l]).max())
                assert np.array_equal(got["grads"][l][1], gb[l]), (R, loss, "gb", l)
            assert np.array_equal(got["values"], val) and np.array_equal(got["values2"], val), (R, loss, "values")
            assert np.array_equal(got["stats"], stats), (R, loss, got["stats"], stats)
            if loss == "clipped" and R > 32:
                assert 0 < got["stats"][2] < R
    close_all(cr, v)


# ---- 2. widths, depths, activations, normaliser, rows, strides
CASES = cl.gpu_general_cases()


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_gradients_within_the_bar(c):
    r = cl.restate(c, cl.tiles_per_workgroup(c))
    cl.check_conditions(c, r)
    v, cr = critic_of(c, c.R)
    got = call(cr, c)
    within(got, r, c.name)
    # the values call and the forward-plus-stats call write the same bits, and twice the same call gives the same bits
    assert np.array_equal(bits(got["values"]), bits(got["values2"]))
    fwd = call(cr, c, backward=False)
    assert np.array_equal(bits(fwd["values"]), bits(got["values"])) and np.array_equal(bits(fwd["stats"]), bits(got["stats"]))
    assert all(np.isnan(g[0]).all() and np.isnan(g[1]).all() for g in fwd["grads"]), "no gradient output was asked for"
    assert same_bits(call(cr, c), got)
    close_all(cr, v)


# ---- 3. the actor's chain
@pytest.mark.parametrize("piles", [[3, 2], [20, 25]], ids=["3x2", "20x25"])
@pytest.mark.parametrize("hidden,act", [((33,), "tanh"), ((64, 64), "tanh"), ((33, 31), "relu")], ids=["33", "64x64", "33x31-relu"])
def test_the_critic_runs_the_actors_chain(piles, hidden, act):
    """a PILES-head, CHUB_PSQ_CLIP actor on the same handle whose hidden layers are the critic's and whose head row S is the critic's
    head row (the other rows arbitrary): chub_policy_act_device's d_tail[:, 0] equals chub_critic_values_device on the same observations
    bit for bit.  Row S = 5 sits at place 5 of tile 0, row S = 45 at place 13 of tile 1: another k order or a fused head fails this"""
    mg = buffers()
    v = make("philox", piles, N_ENVS)
    S, D, A = v.n_slots, v.obs_dim, v.act_dim
    rs = np.random.RandomState(500 + S + sum(hidden))
    layers = cl.general_layers(rs, [D] + list(hidden) + [1])
    head_W, head_b = (rs.normal(size=(A, layers[-1][0].shape[1])) * 0.3).astype(F32), (rs.normal(size=A) * 0.3).astype(F32)
    head_W[S], head_b[S] = layers[-1][0][0], layers[-1][1][0]
    obs = (rs.normal(size=(N_ENVS, D)) + 0.3).astype(F32)
    c = cl.Case(layers=layers, act=act, x=obs, ret=np.zeros(N_ENVS, dtype=F32))
    r = cl.restate(c)
    assert (np.abs(r["values"]) + r["bar_v"]).max() < 1.0 and np.abs(r["values"]).min() > 0, "the clip squash is the identity on these values"
    pol = v.make_policy(layers[:-1] + [(head_W, head_b)], hidden_act=act, squash="clip")
    cr = v.make_critic(layers, hidden_act=act, max_rows=N_ENVS)
    d_obs, d_bits, d_tail, d_val = (mg.DeviceBuffer(obs.nbytes), mg.DeviceBuffer(N_ENVS * v.bit_words * 8), mg.DeviceBuffer(N_ENVS * 8),
                                    mg.DeviceBuffer(N_ENVS * 4))
    d_obs.from_host(obs)
    pol.act_device(d_obs.ptr, d_pile_bits=d_bits.ptr, d_tail=d_tail.ptr)
    cr.values_device(N_ENVS, N_ENVS, d_obs.ptr, d_val.ptr)
    v.sync()
    tail = f32(d_tail.to_host(np.uint32, (N_ENVS, 2)))
    val = f32(d_val.to_host(np.uint32, (N_ENVS,)))
    assert (np.abs(val.astype(np.float64) - r["values"]) <= r["bar_v"] + pl.U * np.abs(r["values"])).all()
    assert np.array_equal(bits(tail[:, 0].copy()), bits(val)), (np.abs(tail[:, 0] - val).max(), int((tail[:, 0] != val).sum()))
    close_all(d_obs, d_bits, d_tail, d_val, cr, pol, v)


# ---- 4. the values call
def test_values_over_a_rollout_equal_values_over_its_blocks():
    """one call over [T][N][F] equals T calls over the blocks, and rows in any order and place equal the same rows alone; a packed
    [N, D + 2] block is read with ld = D + 2"""
    mg = buffers()
    T, n, D = 5, 37, 13
    c = cl.synthetic_case(D, (64, 64), "tanh", T * n, "mse", True, None, D + 2, seed=77)
    v, cr = critic_of(c, T * n)
    x = padded(c)
    x[:, D:] = 1e30  # (a packed block's reward and done columns: never read)
    d_x, d_all, d_blk, d_rows, d_pick = (mg.DeviceBuffer(x.nbytes), mg.DeviceBuffer(4 * T * n), mg.DeviceBuffer(4 * T * n), mg.DeviceBuffer(8 * 40),
                                         mg.DeviceBuffer(4 * 40))
    d_x.from_host(x)
    cr.values_device(T * n, T * n, d_x.ptr, d_all.ptr, ld=D + 2)
    for t in range(T):
        cr.values_device(n, n, d_x.ptr + 4 * t * n * (D + 2), d_blk.ptr + 4 * t * n, ld=D + 2)
    rows = np.random.RandomState(3).permutation(T * n)[:40].astype(np.int64)
    d_rows.from_host(rows)
    cr.values_device(40, T * n, d_x.ptr, d_pick.ptr, d_rows.ptr, D + 2)
    v.sync()
    a, b, p = d_all.to_host(np.uint32, (T * n,)), d_blk.to_host(np.uint32, (T * n,)), d_pick.to_host(np.uint32, (40,))
    assert np.array_equal(a, b) and np.array_equal(p, a[rows])
    r = cl.restate(c)
    assert (np.abs(f32(a).astype(np.float64) - r["values"]) <= r["bar_v"] + pl.U * np.abs(r["values"])).all()
    assert np.array_equal(cr.values(c.x), f32(a)), "the host convenience"
    close_all(d_x, d_all, d_blk, d_rows, d_pick, cr, v)


# ---- 5. minibatches
@pytest.mark.parametrize("loss", ["mse", "clipped"])
def test_minibatches_by_rows_add_up(loss):
    """a seeded permutation of the 300 rows cut into minibatches of 140, 96 and 64: the sum of R_mb * gradient equals R * the full-batch
    gradient within the bars added (each call's own f32 chains, f64 merge and final rounding); each minibatch within its own bar; a
    repeated index counts twice"""
    c = [x for x in CASES if x.name == "13-64x64-tanh-%s-300" % loss][0]
    v, cr = critic_of(c, c.R)
    full = call(cr, c)
    r = cl.restate(c, cl.tiles_per_workgroup(c))
    perm = np.random.RandomState(4).permutation(c.R).astype(np.int64)
    sums = [[np.zeros(W.shape), np.zeros(b.shape)] for W, b in c.layers]
    bars = [[np.zeros(W.shape), np.zeros(b.shape)] for W, b in c.layers]
    for lo, hi in ((0, 140), (140, 236), (236, 300)):
        cm = c.copy(rows=perm[lo:hi])
        rm = cl.restate(cm, cl.tiles_per_workgroup(cm))
        gm = call(cr, cm)
        within(gm, rm, "minibatch %d:%d" % (lo, hi))
        for l in range(len(c.layers)):
            for k, bar in ((0, rm["bar_W"][l]), (1, rm["bar_b"][l])):
                sums[l][k] += (hi - lo) * gm["grads"][l][k].astype(np.float64)
                bars[l][k] += (hi - lo) * bar
    for l in range(len(c.layers)):
        for k, bar in ((0, r["bar_W"][l]), (1, r["bar_b"][l])):
            d = np.abs(sums[l][k] - c.R * full["grads"][l][k].astype(np.float64))
            assert (d <= bars[l][k] + c.R * bar).all(), (l, k, d.max())
    twice = c.copy(rows=np.array([7, 7, 20, 3, 7, 299], dtype=np.int64))
    within(call(cr, twice), cl.restate(twice, 1), "repeated rows")
    close_all(cr, v)


# ---- 6. determinism, graphs, new weights and a new normaliser between replays
def test_two_calls_a_graph_and_new_weights_between_replays():
    mg = buffers()
    c = [x for x in CASES if x.name == "13-64x64-tanh-clipped-300-norm"][0]
    v, cr = critic_of(c, c.R, make("philox", [20, 25], N_ENVS))
    d = DevCase(c)
    st = mg.Stream(0)
    d.run(cr, st.ptr)
    d.run_values(cr, st.ptr)
    st.sync()
    eager = d.out()
    assert np.array_equal(bits(eager["values"]), bits(eager["values2"]))
    # (a handle's graph covers an even number of resets + steps and ends at the clock it began at: two days, and the critic's calls, which
    # take no tick, in the middle of the second)
    acts, packed, obs0 = mg.DeviceBuffer(N_ENVS * v.act_dim * 4), mg.DeviceBuffer(N_ENVS * (v.obs_dim + 2) * 4), mg.DeviceBuffer(N_ENVS * v.obs_dim * 4)
    v.random_actions_device(acts.ptr, 5, 0, st.ptr)
    st.sync()
    v.graph_begin(st.ptr)
    for i in range(192):
        if i % 96 == 0:
            v.reset_device(obs0.ptr, stream=st.ptr)
        v.step_device_packed(acts.ptr, packed.ptr, stream=st.ptr)
        if i == 130:
            d.run_values(cr, st.ptr)
            d.run(cr, st.ptr)
    graph = v.graph_end(st.ptr)
    st.sync()
    d.clear()
    v.graph_launch(graph, st.ptr)
    st.sync()
    assert same_bits(eager, d.out()) and np.array_equal(bits(eager["values2"]), bits(d.out()["values2"])), "a replay equals the eager calls"
    # new weights in the trainer's layout and a normaliser from moments, on the stream: the next replay evaluates and differentiates them
    rs = np.random.RandomState(12)
    new = [((W + 0.1 / W.shape[1] * rs.normal(size=W.shape)).astype(F32), (b + 0.01 * rs.normal(size=b.shape)).astype(F32)) for W, b in c.layers]
    d.put_weights(new)
    for l in range(len(new)):
        cr.set_weights_device(l, d.p("W%d" % l), d.p("b%d" % l), stream=st.ptr)
    m = v.make_moments(c.F)
    m.update_device(d.p("x"), len(c.x), ld=c.F, stream=st.ptr)
    cr.normalizer_from_moments(m, eps=1e-2, stream=st.ptr)
    # (ties are not defined: a row the new weights put on the predicate's edge has its v_old or ret moved, in the graph's buffers too)
    x64 = c.x.astype(np.float64)
    norm = (x64.mean(axis=0).astype(F32), (1.0 / np.sqrt(x64.var(axis=0) + 1e-2)).astype(F32), c.norm[2])
    c2 = cl.separate(c.copy(layers=new, norm=norm))
    st.sync()
    d.buf["v_old"].from_host(c2.v_old)
    d.buf["ret"].from_host(c2.ret)
    v.graph_launch(graph, st.ptr)
    st.sync()
    replay = d.out()
    assert not np.array_equal(replay["values"], eager["values"])
    r2 = cl.restate(c2, cl.tiles_per_workgroup(c2))
    cl.check_conditions(c2, r2)
    # (the moments' mean and variance are f64 sums in another order than numpy's: far inside the normaliser's f32 rounding -- the
    # derived normaliser is held to the restatement by the values' and gradients' own bars)
    within(replay, r2, "replay after new weights and a new normaliser")
    assert np.array_equal(bits(replay["values"]), bits(replay["values2"]))
    v.graph_destroy(graph)
    close_all(m, d, acts, packed, obs0, cr, v)
    st.destroy()


# ---- 8. refusals
def test_refusals_come_with_a_message_and_before_any_device_work():
    mg = buffers()
    c = [x for x in CASES if x.name == "13-33-tanh-mse-300"][0]
    v = make("philox", [3, 2], N_ENVS)
    lib = v._lib
    cr = v.make_critic(c.layers, max_rows=64)
    plain = cr

    def refused(code, text, rc):
        msg = lib.chub_last_error().decode()
        assert rc == code and text in msg, (rc, msg)

    # create
    n = len(c.layers)
    Wp = (C.c_void_p * n)(*[W.ctypes.data for W, _ in c.layers])
    bp = (C.c_void_p * n)(*[b.ctypes.data for _, b in c.layers])
    h = C.c_void_p()
    spec = lambda *a: C.byref(_lib.critic_spec(*a))
    create = lambda sp, W=Wp, b=bp, mean=None, inv=None, rows=64, e=v._h: lib.chub_critic_create(e, sp, W, b, mean, inv, rows, C.byref(h))
    refused(-1, "null argument", create(spec(13, [33, 1]), e=None))
    refused(-1, "null argument", create(spec(13, [33, 1]), W=None))
    refused(-1, "F: 1 .. 512", create(spec(0, [33, 1])))
    refused(-1, "must be 1", create(spec(13, [33, 2])))
    refused(-1, "hidden widths", create(spec(13, [257, 1])))
    refused(-1, "hidden_act", create(spec(13, [33, 1], 5)))
    refused(-1, "clip must be > 0", create(spec(13, [33, 1], "tanh", True, -1.0)))
    refused(-1, "normalize needs mean and inv_std", create(spec(13, [33, 1], "tanh", True, 3.0)))
    refused(-1, "max_rows", create(spec(13, [33, 1]), rows=0))
    refused(-4, "LDS", create(spec(13, [256, 256, 161, 1])))
    assert not h.value
    st = mg.Stream(0)
    buf = mg.DeviceBuffer(1 << 16)
    p = buf.ptr
    W0, b0 = c.layers[0]
    v.graph_begin(st.ptr)
    refused(-4, "chub_graph_begin", create(spec(13, [33, 1])))
    refused(-4, "chub_graph_begin", lib.chub_critic_destroy(cr._c))
    refused(-4, "chub_graph_begin", lib.chub_critic_set_weights(cr._c, 0, W0.ctypes.data, b0.ctypes.data))
    v.reset_device(p, stream=st.ptr)  # (a graph covers an even, non-zero number of resets + steps)
    v.reset_device(p, stream=st.ptr)
    v.graph_destroy(v.graph_end(st.ptr))
    st.sync()
    refused(-1, "layer", lib.chub_critic_set_weights(cr._c, 2, W0.ctypes.data, b0.ctypes.data))
    refused(-1, "layer", lib.chub_critic_set_weights_device(cr._c, -1, p, p, None))
    refused(-1, "null argument", lib.chub_critic_set_weights_device(cr._c, 0, None, p, None))
    refused(-1, "normalize = 0", lib.chub_critic_set_normalizer(plain._c, W0.ctypes.data, W0.ctypes.data))
    refused(-1, "normalize = 0", lib.chub_critic_set_normalizer_device(plain._c, p, p, None))
    normed = v.make_critic(c.layers, normalize=(np.zeros(13, dtype=F32), np.ones(13, dtype=F32), 3.0), max_rows=64)
    m7, m13 = v.make_moments(7), v.make_moments(13)
    other = make("philox", [3, 2], N_ENVS)
    m_other = other.make_moments(13)
    refused(-1, "normalize = 0", lib.chub_critic_normalizer_from_moments_device(plain._c, m13._m, 1e-8, None))
    refused(-1, "F = 7", lib.chub_critic_normalizer_from_moments_device(normed._c, m7._m, 1e-8, None))
    refused(-1, "different handles", lib.chub_critic_normalizer_from_moments_device(normed._c, m_other._m, 1e-8, None))
    refused(-1, "eps", lib.chub_critic_normalizer_from_moments_device(normed._c, m13._m, 0.0, None))
    refused(-1, "null argument", lib.chub_critic_set_normalizer_device(normed._c, None, p, None))

    # the calls: every output holds a pattern that a refused call must leave alone
    pattern = np.full(1 << 14, 0x7FC01234, dtype=np.uint32)
    buf.from_host(pattern)
    out_p = p + (1 << 15)  # (inputs from the first half, outputs into the second)

    def args(**kw):
        a = dict(R=64, n_rows=64, d_rows=None, d_x=p, ld=13, d_ret=p, d_v_old=p, loss=1, clip_eps=0.2)
        a.update(kw)
        return _lib.ChubCriticGradIn(**a)

    out = _lib.ChubCriticGradOut()
    out.d_values, out.d_stats, out.d_gW[0], out.d_gb[0] = out_p, out_p + 4096, out_p + 8192, out_p + 12288
    run = lambda **kw: lib.chub_critic_grad_device(cr._c, C.byref(args(**kw)), C.byref(out), None)
    val = lambda **kw: lib.chub_critic_values_device(cr._c, kw.get("d_x", p), kw.get("ld", 13), kw.get("n_rows", 64), kw.get("d_rows", None),
                                                     kw.get("R", 64), kw.get("d_values", out_p), None)
    for field in ("d_x", "d_ret", "d_v_old"):
        refused(-1, "null argument", run(**{field: None}))
    refused(-1, "null argument", lib.chub_critic_grad_device(cr._c, None, C.byref(out), None))
    refused(-1, "null argument", lib.chub_critic_grad_device(cr._c, C.byref(args()), None, None))
    refused(-1, "max_rows", run(R=0))
    refused(-1, "max_rows", run(R=65))
    refused(-1, "n_rows", run(n_rows=0))
    refused(-1, "n_rows", run(n_rows=32))
    refused(-1, "ld", run(ld=12))
    refused(-1, "loss", run(loss=2))
    refused(-1, "loss", run(loss=-1))
    for e in (0.0, -0.1, float("nan"), float("inf")):
        refused(-1, "clip_eps", run(clip_eps=e))
    refused(-1, "null argument", val(d_values=None))
    refused(-1, "null argument", val(d_x=None))
    refused(-1, "max_rows", val(R=0))
    refused(-1, "max_rows", val(R=65))
    refused(-1, "n_rows", val(n_rows=0))
    refused(-1, "n_rows", val(n_rows=63))
    refused(-1, "ld", val(ld=12))
    v.sync()
    assert np.array_equal(buf.to_host(np.uint32, (1 << 14,)), pattern), "a refused call touched an output"
    assert run(loss=0, d_v_old=None) == 0, "MSE does not read v_old"
    assert run(clip_eps=5.0) == 0 and val() == 0
    v.sync()
    assert not np.array_equal(buf.to_host(np.uint32, (1 << 14,))[1 << 13:], pattern[1 << 13:])
    # chub_destroy frees a handle's critics
    buf.free()
    st.destroy()
    normed._c = cr._c = None
    close_all(m7, m13, m_other, other, v)


# ---- 7. collected rollouts and (9) the torch adapter, in child processes that import torch first (as tests/test_gpu_torch_side.py does)
TORCH_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["CHUB_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHUB_ROOT"], "tests"))
import torch  # before libchub: both must share one HIP runtime
torch.cuda.set_device(0)
import test_gpu_critic
getattr(test_gpu_critic, os.environ["CHUB_CHILD"])()
print("TORCH_CRITIC_OK")
"""


def in_a_child(name):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], env=dict(os.environ, CHUB_ROOT=root, CHUB_CHILD=name), capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "TORCH_CRITIC_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_collected_rollouts_values_advantages_value_gradient():
    in_a_child("adapter_collected_rollouts")


def test_torch_adapter_value_gradient_against_cuda_autograd():
    in_a_child("torch_adapter_value_gradient")


def adapter_env(rng, autoreset, n=N_ENVS):
    from charginghub_env_amd import wrappers
    kw = {k: BASE[k] for k in BASE if k != "station_type_list"}
    return wrappers.TorchHubVecEnv(n, [20, 25], ["fast", "slow"], seed=13, autoreset=autoreset, rng=rng, **kw)


def collected_case(env, pol, crit, T, critic_layers, rs):
    """collect, take the critic's normaliser from the rollout's own features, then values -> advantages: the rollout, the tensors and the
    case (v_old: the values as collected; the critic's weights then move, so that rows fall on every side of the clipped predicate)"""
    import torch
    n, D = env.num_envs, crit.n_features
    ro = env.collect(pol, T, logp_piles="decidable")
    torch.cuda.synchronize()
    feats = ro["features"].cpu().numpy().reshape(T * n, D)
    f64 = feats.astype(np.float64)
    norm = (f64.mean(axis=0).astype(F32), (1.0 / np.sqrt(f64.var(axis=0) + 1e-2)).astype(F32), 3.0)
    crit.set_normalizer(norm[0], norm[1])
    vals, final = env.values(crit, ro)
    adv, ret = env.advantages(ro, vals, final)
    torch.cuda.synchronize()
    c = cl.Case(layers=critic_layers, norm=norm, act="tanh", x=feats.copy(), ret=ret.cpu().numpy().reshape(T * n).copy(),
                v_old=vals[:T].cpu().numpy().reshape(T * n).copy(), loss="mse", clip_eps=0.05, name="collected")
    return ro, vals, final, ret, c


def moved_by(c, new):
    """the clip range of a collected case: the median distance the new weights moved the values from the values as collected, so that
    half the rows lie outside the range -- and of those the ones that moved TOWARDS ret are clipped away"""
    return float(F32(np.median(np.abs(cl.forward64(c.copy(layers=new)) - c.v_old.astype(np.float64)))))


def both_ways(c, new):
    """`new` with its head bias shifted so that the median move of the values is 0: a perturbation's head bias alone moves every value
    the same way, and then no row (or every row) outside the range moves towards ret"""
    shift = np.median(cl.forward64(c.copy(layers=new)) - c.v_old.astype(np.float64))
    return new[:-1] + [(new[-1][0], (new[-1][1] - F32(shift)).astype(F32))]


def adapter_collected_rollouts():
    """philox and philox_curves, lockstep and per-env auto-reset, N = 64, T = 8: values -> advantages -> value_gradient end to end; values
    and gradients within the bar of the restatement on the collected features; V[T] is the critic on the state's feature row;
    final_values exactly where specified.  Then an actor with a forecast block: V[T] through the actor's feature launches, no final"""
    import torch
    T, n = 8, N_ENVS
    for rng in ("philox", "philox_curves"):
        for autoreset in (True, "per_env"):
            what = "%s-%s" % (rng, autoreset)
            rs = np.random.RandomState(41 + (rng == "philox") + 2 * (autoreset is True))
            env = adapter_env(rng, autoreset)
            D, A = env.obs_dim, env.act_dim
            pol = env.load_policy(cl.general_layers(rs, [D, 33, A]))
            pol.set_exploration(21, np.array([-0.2, 0.1], dtype=F32))
            layers = cl.general_layers(rs, [D, 33, 31, 1])
            crit = env.load_critic(layers, normalize=(np.zeros(D, dtype=F32), np.ones(D, dtype=F32), 3.0))
            env.reset()
            ro, vals, final, ret, c = collected_case(env, pol, crit, T, layers, rs)
            assert (final is not None) == (autoreset == "per_env"), what
            r = cl.restate(c, cl.tiles_per_workgroup(c))
            v_dev = vals.cpu().numpy()
            dv = np.abs(v_dev[:T].reshape(-1).astype(np.float64) - r["values"])
            print(what, "values max diff %.3e" % dv.max(), "bar there %.3e" % r["bar_v"][dv.argmax()])
            assert (dv <= r["bar_v"] + pl.U * np.abs(r["values"])).all(), what
            # V[T]: the critic on the last block's observation; final_values: on last_obs -- the same launch alone gives the same bits
            x_T = ro["packed"][T - 1, :, :D].cpu().numpy()
            assert np.array_equal(bits(crit.values(x_T)), bits(v_dev[T])), what
            rT = cl.restate(c.copy(x=x_T, ret=np.zeros(n, dtype=F32), v_old=np.zeros(n, dtype=F32)))
            assert (np.abs(v_dev[T].astype(np.float64) - rT["values"]) <= rT["bar_v"] + pl.U * np.abs(rT["values"])).all(), what
            if final is not None:
                assert np.array_equal(bits(crit.values(env.last_obs.cpu().numpy())), bits(final.cpu().numpy())), what
            # the critic moves; the value loss around the values as collected
            new = [((W + 1.0 / W.shape[1] * rs.normal(size=W.shape)).astype(F32), (b + 0.1 * rs.normal(size=b.shape)).astype(F32)) for W, b in layers]
            new = both_ways(c, new)
            for l, (W, b) in enumerate(new):
                crit.set_weights(l, W, b)
            v_old_t = vals[:T].clone()
            eps = moved_by(c, new)
            for loss in ("mse", "clipped"):
                cc = cl.separate(c.copy(layers=new, loss=loss, clip_eps=eps), cl.tiles_per_workgroup(c))
                ret.copy_(torch.tensor(cc.ret, device="cuda").reshape(T, n))
                v_old_t.copy_(torch.tensor(cc.v_old, device="cuda").reshape(T, n))
                rr = cl.restate(cc, cl.tiles_per_workgroup(cc))
                cl.check_conditions(cc, rr)
                grads, stats = env.value_gradient(crit, ro, ret, loss=loss, clip_eps=cc.clip_eps, v_old=v_old_t if loss == "clipped" else None)
                torch.cuda.synchronize()
                got = dict(grads=[(gW.cpu().numpy(), gb.cpu().numpy()) for gW, gb in grads], stats=stats.cpu().numpy(),
                           values=env.values(crit, ro)[0][:T].cpu().numpy().reshape(-1))
                within(got, rr, "%s-%s" % (what, loss))
                if loss == "clipped":
                    print(what, "rows clipped away: %d of %d" % (got["stats"][2], cc.R))
                    assert 0 < got["stats"][2] < cc.R
            env.close()
    # an actor that reads a forecast block beside the observation: its feature row needs the state
    env = adapter_env("philox", "per_env")
    rs = np.random.RandomState(47)
    inputs = ("obs", ("forecast", ("price",), 6))
    F = env.obs_dim + 6
    pol = env.load_policy(cl.general_layers(rs, [F, 33, env.act_dim]), inputs=inputs)
    pol.set_exploration(21, np.array([-0.2, 0.1], dtype=F32))
    crit = env.load_critic(cl.general_layers(rs, [F, 33, 1]))
    env.reset()
    ro = env.collect(pol, T)
    vals, final = env.values(crit, ro)
    assert final is None and tuple(vals.shape) == (T + 1, n)
    feat = torch.zeros((n, F), dtype=torch.float32, device="cuda")
    logp = torch.zeros((n,), dtype=torch.float32, device="cuda")
    pol.sample_device(env._packed.data_ptr(), env.obs_dim + 2, d_logp=logp.data_ptr(), d_features=feat.data_ptr(), stream=env._stream())
    torch.cuda.synchronize()
    assert np.array_equal(feat.cpu().numpy()[:, :env.obs_dim], ro["packed"][T - 1, :, :env.obs_dim].cpu().numpy())
    assert np.array_equal(bits(crit.values(feat.cpu().numpy())), bits(vals[T].cpu().numpy()))
    assert np.array_equal(bits(crit.values(ro["features"].cpu().numpy().reshape(T * n, F))), bits(vals[:T].cpu().numpy().reshape(-1)))
    env.close()


def torch_adapter_value_gradient():
    """load_critic from an nn.Sequential, new weights pushed from the parameters' own memory, value_gradient over all rows and over a
    minibatch under both losses against CUDA f64 autograd of the same loss, held to the derived bar"""
    import torch
    T, n = 6, N_ENVS
    rs = np.random.RandomState(5)
    env = adapter_env("philox", "per_env")
    D, A = env.obs_dim, env.act_dim
    pol = env.load_policy(cl.general_layers(rs, [D, 33, A]))
    pol.set_exploration(21, np.array([-0.2, 0.1], dtype=F32))
    layers = cl.general_layers(rs, [D, 33, 17, 1])
    net = torch.nn.Sequential(torch.nn.Linear(D, 33), torch.nn.Tanh(), torch.nn.Linear(33, 17), torch.nn.Tanh(), torch.nn.Linear(17, 1)).to("cuda")
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, (Wl, bl) in zip(lin, layers):
            m.weight.copy_(torch.tensor(Wl))
            m.bias.copy_(torch.tensor(bl))
    crit = env.load_critic(net, normalize=(np.zeros(D, dtype=F32), np.ones(D, dtype=F32), 3.0))
    with pytest.raises(ValueError):
        env.load_critic(torch.nn.Sequential(torch.nn.Linear(D, 1), torch.nn.Tanh()))
    env.reset()
    ro, vals, final, ret, c = collected_case(env, pol, crit, T, layers, rs)
    with pytest.raises(AssertionError):
        env.value_gradient(crit, ro, ret, loss="clipped")
    with pytest.raises(AssertionError):
        env.value_gradient(crit, ro, ret[:2])
    with pytest.raises(ValueError):
        env.value_gradient(crit, {"features": ro["features"]}, ret)
    # a step, pushed to the device from the parameters' own memory
    with torch.no_grad():
        for m in lin:
            m.weight.add_(torch.tensor((1.0 / m.weight.shape[1] * rs.normal(size=tuple(m.weight.shape))).astype(F32), device="cuda"))
            m.bias.add_(torch.tensor((0.1 * rs.normal(size=tuple(m.bias.shape))).astype(F32), device="cuda"))
    new = both_ways(c, [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in lin])
    with torch.no_grad():
        lin[-1].bias.copy_(torch.tensor(new[-1][1]))
    for l, m in enumerate(lin):
        crit.set_weights_device(l, m.weight.data_ptr(), m.bias.data_ptr(), stream=env._stream())
    v_old_t = vals[:T].clone()
    mean, inv_std, clip = (torch.tensor(a, device="cuda") for a in c.norm)
    eps0 = moved_by(c, new)
    for loss in ("mse", "clipped"):
        for rows in (None, torch.tensor(rs.permutation(T * n)[:100].astype(np.int64), device="cuda")):
            cc = c.copy(layers=new, loss=loss, clip_eps=eps0, rows=None if rows is None else rows.cpu().numpy())
            cc = cl.separate(cc, cl.tiles_per_workgroup(cc))
            ret.copy_(torch.tensor(cc.ret, device="cuda").reshape(T, n))
            v_old_t.copy_(torch.tensor(cc.v_old, device="cuda").reshape(T, n))
            r = cl.restate(cc, cl.tiles_per_workgroup(cc))
            cl.check_conditions(cc, r)
            grads, stats = env.value_gradient(crit, ro, ret, rows=rows, loss=loss, clip_eps=cc.clip_eps, v_old=v_old_t)
            torch.cuda.synchronize()
            # CUDA autograd of an f64 copy of the network on the f32-normalised rows
            net64 = torch.nn.Sequential(torch.nn.Linear(D, 33), torch.nn.Tanh(), torch.nn.Linear(33, 17), torch.nn.Tanh(), torch.nn.Linear(17, 1)).double().to("cuda")
            lin64 = [m for m in net64 if isinstance(m, torch.nn.Linear)]
            with torch.no_grad():
                for a, b in zip(lin64, lin):
                    a.weight.copy_(b.weight.double())
                    a.bias.copy_(b.bias.double())
            idx = slice(None) if rows is None else rows
            flat = lambda t: t.reshape(T * n, *t.shape[2:])[idx]
            x = torch.clamp((flat(ro["features"]) - mean) * inv_std, -float(c.norm[2]), float(c.norm[2]))
            v = net64(x.double())[:, 0]
            rt, vo = flat(ret).double(), flat(v_old_t).double()
            if loss == "mse":
                L = (0.5 * (v - rt) ** 2).mean()
            else:
                eps = float(F32(cc.clip_eps))
                L = (0.5 * torch.maximum((v - rt) ** 2, (vo + torch.clamp(v - vo, -eps, eps) - rt) ** 2)).mean()
            L.backward()
            for l, m in enumerate(lin64):
                dW = np.abs(grads[l][0].cpu().numpy().astype(np.float64) - m.weight.grad.cpu().numpy())
                db = np.abs(grads[l][1].cpu().numpy().astype(np.float64) - m.bias.grad.cpu().numpy())
                print(loss, "rows" if rows is not None else "all", "layer", l, "gW diff %.3e bar %.3e" % (dW.max(), r["bar_W"][l].ravel()[dW.argmax()]))
                assert (dW <= r["bar_W"][l]).all(), ("gW", l, loss)
                assert (db <= r["bar_b"][l]).all(), ("gb", l, loss)
            st = stats.cpu().numpy()
            assert st[0] == cc.R and st[2] == r["stats"][2] and abs(st[1] / cc.R - float(L)) <= r["bar_stats"][1] / cc.R + 1e-12 + 2.0 ** -23 * abs(float(L))
            if loss == "clipped" and rows is None:
                assert 0 < st[2] < cc.R
    env.close()
