"""The optimiser on the device (include/chub.h, "an optimiser on the device") against tests/adam_lib.py's restatement, bit for bit:
(1) the step on every spec and scenario, after 1, 2 and 5 steps; (2) the layout: a fresh policy / critic made from the restatement's
weights acts / values with the same bits, and set_weights_device between steps is honoured; (3) with the gradient calls, over rows of a
collected rollout; (4) a captured minibatch replayed three times against three eager ones; (5) the state's round trip; (6) every
refusal; (7) torch's double-precision AdamW within the derived bar and the torch adapter, in child processes."""
import ctypes as C

import numpy as np
import pytest

import adam_lib as al
import policy_grad_lib as pgl
from charginghub_env_amd import _lib
from test_gpu_autoreset import buffers
from test_gpu_pile_obs import BASE, make
from test_gpu_policy import f32
from test_gpu_policy_sample import Roll, close_all

pytestmark = pytest.mark.gpu
F32 = np.float32
N_ENVS = 64
KEY = 77
INPUTS = {13: ("obs",), 64: pgl.WIDE_INPUTS, 3: (("forecast", ("price",), 3),), 7: (("forecast", ("price",), 7),)}
CHECK_AT = (1, 2, 5)

PLAIN = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0)
SCENARIOS = {
    "plain": (PLAIN, None),
    "clips-decay": (dict(PLAIN, max_grad_norm=0.5, weight_decay=0.01), True),
    "does_not_clip": (dict(PLAIN, max_grad_norm=1e6), False),
    "beta1_0-decay": (dict(PLAIN, betas=(0.0, 0.99), weight_decay=0.01), None),
}


class StepCase(object):
    def __init__(self, net, kind, scenario, explore, seed):
        F, widths = (al.ACTOR_NETS if kind == "policy" else al.CRITIC_NETS)[net]
        self.name = "%s-%s-%s%s" % (kind, net, scenario, "-log_std" if explore else "")
        self.kind, self.F, self.widths, self.explore = kind, F, widths, explore
        self.hyper, self.clips = SCENARIOS[scenario]
        self.shapes = al.shapes_of(F, widths)
        self.G = 2 if explore else 0
        self.n = al.n_params(self.shapes, self.G)
        rs = np.random.RandomState(seed)
        self.layers = pgl.general_layers(rs, [F] + list(widths))
        self.log_std = np.array([-0.5, 0.25], dtype=F32) if explore else None
        # gradients of mixed magnitudes, far above the clip norm of the scenario that clips and far below the other's
        self.grads = [al.stabilised((rs.normal(size=self.n) * 10.0 ** rs.uniform(-2, 0.5, size=self.n)).astype(F32), self.hyper["max_grad_norm"])
                      for _ in range(max(CHECK_AT))]


def all_step_cases():
    cases, seed = [], 100
    for net in al.ACTOR_NETS:
        if net == "13-64-64-47":
            continue
        scen = list(SCENARIOS) if net == "13-33-31-47" else (["clips-decay", "plain"] if net != "64-256-224-47" else ["clips-decay"])
        for i, s in enumerate(scen):
            for explore in ((True, False) if net == "13-33-31-47" and s == "clips-decay" else (i % 2 == 0,)):
                seed += 1
                cases.append(StepCase(net, "policy", s, explore, seed))
    for net in al.CRITIC_NETS:
        for s in ("clips-decay", "does_not_clip", "beta1_0-decay"):
            seed += 1
            cases.append(StepCase(net, "critic", s, False, seed))
    return cases


CASES = all_step_cases()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == F32 else np.uint64)


def to_host(ptr, dtype, shape):
    out = np.empty(shape, dtype=dtype)
    _lib.check(_lib.load_library().chub_copy_to_host(0, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, None))
    return out


def target_of(v, c, layers=None, log_std=None):
    """the case's policy or critic on handle v (with other weights: the fresh twin of the layout test)"""
    layers = c.layers if layers is None else layers
    if c.kind == "critic":
        return v.make_critic(layers, hidden_act="tanh", max_rows=N_ENVS)
    pol = v.make_policy(layers, inputs=INPUTS[c.F], head="piles", hidden_act="tanh")
    if c.explore:
        pol.set_exploration(KEY, c.log_std if log_std is None else log_std)
    return pol


class Dev(object):
    """a target, its optimiser, a flat gradient buffer in the trainer's order and the restatement beside them"""

    def __init__(self, v, c, hyper=None, wrong=None):
        mg = buffers()
        self.v, self.c = v, c
        self.target = target_of(v, c)
        self.opt = v.make_adam(self.target, **(hyper or c.hyper))
        assert self.opt.n_params == c.n and self.opt.has_log_std == c.explore
        self.ref = al.Adam(c.n, al.decay_mask(c.shapes, c.G), wrong=wrong, **(hyper or c.hyper))
        self.theta = al.flatten(c.layers, c.log_std)
        self.g, self.out, self.stats = mg.DeviceBuffer(4 * c.n), mg.DeviceBuffer(4 * c.n), mg.DeviceBuffer(32)
        self.gW, self.gb, p = [], [], self.g.ptr
        for o, i in c.shapes:
            self.gW.append(p)
            self.gb.append(p + 4 * o * i)
            p += 4 * o * (i + 1)
        self.gls = p if c.explore else 0

    def step(self, g, stream=0):
        self.g.from_host(g)
        self.stats.from_host(np.full(4, np.nan))
        self.opt.step_device(self.gW, self.gb, self.gls, self.stats.ptr, stream)
        self.v.sync()
        self.theta, want = self.ref.step(self.theta, g)
        return self.stats.to_host(np.float64, (4,)), want

    def read_theta(self, stream=0):
        """the live weights through get_weights_device / get_log_std_device, flat"""
        self.out.from_host(np.full(self.c.n, np.nan, dtype=F32))
        p = self.out.ptr
        for l, (o, i) in enumerate(self.c.shapes):
            self.target.get_weights_device(l, p, p + 4 * o * i, stream)
            p += 4 * o * (i + 1)
        if self.c.explore:
            self.target.get_log_std(p, stream)
        self.v.sync()
        return self.out.to_host(F32, (self.c.n,))

    def check(self, what):
        got = self.read_theta()
        bad = np.nonzero(bits(got) != bits(self.theta))[0]
        assert bad.size == 0, (what, "theta: %d of %d entries differ, first at %d: %r against %r" % (bad.size, self.c.n, bad[0], got[bad[0]], self.theta[bad[0]]))
        assert self.opt.state() == self.ref.blob(), (what, "t, p1, p2, m or v")

    def free(self):
        close_all(self.g, self.out, self.stats, self.opt, self.target)


def check_stats(got, want, g, what):
    n = len(g)
    print(what, "stats", got, "restated", want)
    assert got[0] == want[0] and bits(np.array(got[2])) == bits(np.array(want[2])) and got[3] == want[3], (what, got, want)
    if np.isfinite(g).all():
        exact = al.fsum_norm(g)
        assert abs(got[1] - exact) <= n * al.U64 * exact, (what, got[1], exact)
    else:
        assert not np.isfinite(got[1])


# ---- 1. and 2. the step and the layout
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_steps_equal_the_restatement_bit_for_bit(c):
    """theta, m, v, t, p1, p2 and scale after 1, 2 and 5 steps; the norm within n 2^-53 of fsum's; then the target's own launch on the
    live buffers against a FRESH target made from the restatement's weights.  64 -> 256 -> 224 -> 47 has 83 chunks on the 64 workgroups
    both launches are capped at: its workgroups 0 .. 18 make a second trip"""
    v = make("philox", al.POLICY_HUB, N_ENVS)
    v.reset()
    d = Dev(v, c)
    for k, g in enumerate(c.grads):
        got, want = d.step(g)
        check_stats(got, want, g, (c.name, k + 1))
        if c.clips is not None:
            assert (got[2] < 1.0) == c.clips
        if k + 1 in CHECK_AT:
            d.check((c.name, k + 1))
    assert d.ref.t == max(CHECK_AT)
    layers, log_std = al.unflatten(d.theta, c.shapes, c.G)
    if c.hyper["weight_decay"]:  # (a decayed bias would have moved further: the restatement leaves it to Adam alone, and so does the device)
        plain = Dev(v, c, dict(c.hyper, weight_decay=0.0))
        for g in c.grads:
            plain.step(g)
        for (_, b), (_, b0) in zip(layers, al.unflatten(plain.theta, c.shapes, c.G)[0]):
            assert np.array_equal(bits(b), bits(b0))
        plain.check((c.name, "no decay"))
        plain.free()
    fresh = target_of(v, c, layers, log_std)
    if c.kind == "critic":
        x = np.random.RandomState(3).normal(size=(N_ENVS, c.F)).astype(F32)
        assert np.array_equal(bits(d.target.values(x)), bits(fresh.values(x)))
    else:
        obs = np.random.RandomState(3).uniform(0, 1, size=(N_ENVS, v.obs_dim)).astype(F32)
        a, b = d.target.act(obs), fresh.act(obs)
        assert np.isfinite(a).all() and np.array_equal(bits(a), bits(b))
    fresh.close()
    d.free()
    v.close()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_gradient_that_is_not_finite_skips_the_step(bad):
    c = [x for x in CASES if x.name == "policy-13-33-31-47-clips-decay-log_std"][0]
    v = make("philox", al.POLICY_HUB, N_ENVS)
    d = Dev(v, c)
    d.step(c.grads[0])
    d.check("before")
    blob = d.opt.state()
    for at in (0, c.n // 2, c.n - 1):  # (a W of layer 0, an entry of the middle, log_std's last)
        g = c.grads[1].copy()
        g[at] = bad
        got, want = d.step(g)
        assert got[0] == 1 and got[2] == 0 and got[3] == 1 and list(want[[0, 2, 3]]) == [1, 0, 1] and not np.isfinite(got[1])
        d.check(("skipped", bad, at))
        assert d.opt.state() == blob
    got, want = d.step(c.grads[1])
    assert got[0] == 2 and got[3] == 0
    d.check("after")
    d.free()
    v.close()


def test_set_weights_device_between_two_steps_is_honoured():
    """the step starts from the new weights and the old moments; reset_device then starts the moments over"""
    mg = buffers()
    cases = [x for x in CASES if x.name in ("policy-13-33-31-47-plain-log_std", "critic-13-64-64-1-clips-decay")]
    assert len(cases) == 2
    for c in cases:
        v = make("philox", al.POLICY_HUB, N_ENVS)
        d = Dev(v, c)
        d.step(c.grads[0])
        d.step(c.grads[1])
        new = pgl.general_layers(np.random.RandomState(8), [c.F] + list(c.widths))
        o, i = c.shapes[1] if len(c.shapes) > 1 else c.shapes[0]
        l = 1 if len(c.shapes) > 1 else 0
        W, b = mg.DeviceBuffer(4 * o * i), mg.DeviceBuffer(4 * o)
        W.from_host(new[l][0])
        b.from_host(new[l][1])
        d.target.set_weights_device(l, W.ptr, b.ptr)
        v.sync()
        layers, log_std = al.unflatten(d.theta, c.shapes, c.G)
        layers[l] = new[l]
        d.theta = al.flatten(layers, log_std)
        d.check("new weights")
        d.step(c.grads[2])
        d.check("a step from the new weights and the old moments")
        d.opt.reset_device()
        d.ref.reset()
        d.step(c.grads[3])
        d.check("after reset_device")
        assert d.ref.t == 1
        close_all(W, b)
        d.free()
        v.close()


# ---- 5. the state's round trip
def test_a_saved_and_restored_state_continues_the_run():
    c = [x for x in CASES if x.name == "policy-7-31-33-64-47-clips-decay-log_std"][0]
    v = make("philox", al.POLICY_HUB, N_ENVS)
    a, b = Dev(v, c), Dev(v, c)
    for g in c.grads[:3]:
        a.step(g)
        b.step(g)
    blob = a.opt.state()
    assert len(blob) == a.opt.state_bytes == 32 + 8 * c.n
    a.opt.reset_device()
    a.step(c.grads[4])  # (something else happens to the state in between)
    a.opt.load_state(blob)
    a.ref.load(blob)
    for l, (Wl, bl) in enumerate(b.target.get_weights()):
        a.target.set_weights(l, Wl, bl)
    a.target.set_exploration(KEY, b.target.get_log_std())
    a.theta = b.theta.copy()
    a.step(c.grads[3])
    b.step(c.grads[3])
    a.check("restored")
    b.check("uninterrupted")
    assert a.opt.state() == b.opt.state() and np.array_equal(bits(a.read_theta()), bits(b.read_theta()))
    a.free()
    b.free()
    v.close()


# ---- 3. with the gradient calls
def discounted(packed, D, gamma=0.97):
    r = packed[:, :, D].astype(np.float64)
    ret = np.zeros_like(r)
    acc = np.zeros(r.shape[1])
    for t in range(len(r) - 1, -1, -1):
        acc = r[t] + gamma * acc
        ret[t] = acc
    return ((ret - ret.mean()) / (ret.std() + 1e-6)).astype(F32)


class Collected(object):
    """a rollout of T = 6 steps on 64 envs of hub [20, 25] collected by an actor 13 -> 64 -> 64 -> 47, a critic 13 -> 64 -> 64 -> 1 beside
    it, returns and advantages in device memory, and both optimisers"""
    T, R = 6, 300

    def __init__(self, lr=3e-3):
        mg = buffers()
        rs = np.random.RandomState(41)
        self.v = v = make("philox", al.POLICY_HUB, N_ENVS, seed=6)
        D = v.obs_dim
        self.n_rows = self.T * N_ENVS
        self.actor_layers = pgl.general_layers(rs, [D, 64, 64, v.act_dim])
        self.critic_layers = pgl.general_layers(rs, [D, 64, 64, 1])
        self.ls = np.array([-0.2, 0.1], dtype=F32)
        self.pol = v.make_policy(self.actor_layers)
        self.pol.set_exploration(KEY, self.ls)
        self.crit = v.make_critic(self.critic_layers, max_rows=self.n_rows)
        self.roll = Roll(v, self.pol, self.T)
        self.roll.collect("lockstep")
        h = self.roll.host()
        self.ret = discounted(f32(h["packed"]), D).reshape(-1)
        self.adv = (rs.normal(size=self.n_rows)).astype(F32)
        self.d_ret, self.d_adv, self.d_rows = mg.DeviceBuffer(4 * self.n_rows), mg.DeviceBuffer(4 * self.n_rows), mg.DeviceBuffer(8 * self.n_rows)
        self.d_ret.from_host(self.ret)
        self.d_adv.from_host(self.adv)
        self.pstats, self.cstats, self.ostats = mg.DeviceBuffer(48), mg.DeviceBuffer(48), mg.DeviceBuffer(64)
        self.grad = v.make_policy_grad(self.pol, self.n_rows)
        hyper = dict(PLAIN, lr=lr, max_grad_norm=0.5, weight_decay=0.01)
        self.opt_a, self.opt_c = v.make_adam(self.pol, **hyper), v.make_adam(self.crit, **hyper)
        self.sa, self.sc = al.shapes_of(D, [64, 64, v.act_dim]), al.shapes_of(D, [64, 64, 1])
        self.ref_a = al.Adam(al.n_params(self.sa, 2), al.decay_mask(self.sa, 2), **hyper)
        self.ref_c = al.Adam(al.n_params(self.sc), al.decay_mask(self.sc), **hyper)
        self.theta_a, self.theta_c = al.flatten(self.actor_layers, self.ls), al.flatten(self.critic_layers)

    def actor_gradient(self, R, d_rows, stream=0, feats=None):
        r = feats or self.roll
        gW, gb, gls = self.opt_a.grads()
        self.grad.grad_device(R, self.n_rows, r.ptr("feat"), r.ptr("u"), self.d_adv.ptr, d_pile_bits=r.ptr("bits"), d_logp_old=r.ptr("logp"),
                              d_rows=d_rows, loss="ppo_clip", clip_eps=0.2, ent_coef=0.0, d_gW=gW, d_gb=gb, d_glog_std=gls, d_stats=self.pstats.ptr,
                              stream=stream)

    def critic_gradient(self, R, d_rows, stream=0, feats=None):
        r = feats or self.roll
        gW, gb, _ = self.opt_c.grads()
        self.crit.grad_device(R, self.n_rows, r.ptr("feat"), self.d_ret.ptr, d_rows=d_rows, loss="mse", d_gW=gW, d_gb=gb, d_stats=self.cstats.ptr,
                              stream=stream)

    def own_gradient(self, opt):
        gW, _, _ = opt.grads()
        return to_host(gW[0], F32, (opt.n_params,))

    def theta_of(self, target, shapes, G):
        flat = al.flatten(target.get_weights(), target.get_log_std() if G else None)
        return flat

    def free(self):
        close_all(self.d_ret, self.d_adv, self.d_rows, self.pstats, self.cstats, self.ostats, self.opt_a, self.opt_c, self.grad, self.roll, self.crit,
                  self.pol, self.v)


@pytest.mark.parametrize("who", ["critic", "actor"])
def test_eight_iterations_with_the_gradient_calls(who):
    """gradient call into the optimiser's own buffers, step, over 300 shuffled rows of the 384 collected: after each iteration the
    gradient is read, the restatement is stepped with it, and the weights are compared bit for bit; the loss of the stats falls"""
    k = Collected()
    v = k.v
    v.shuffle_rows_device(k.d_rows.ptr, k.n_rows, 5)
    losses = []
    for it in range(8):
        if who == "critic":
            k.critic_gradient(k.R, k.d_rows.ptr)
            k.opt_c.step_device(d_stats=k.ostats.ptr)
            v.sync()
            st = k.cstats.to_host(np.float64, (6,))
            k.theta_c, want = k.ref_c.step(k.theta_c, k.own_gradient(k.opt_c))
            got = k.theta_of(k.crit, k.sc, 0)
            assert np.array_equal(bits(got), bits(k.theta_c)), (it, int((bits(got) != bits(k.theta_c)).sum()))
            assert k.opt_c.state() == k.ref_c.blob()
        else:
            k.actor_gradient(k.R, k.d_rows.ptr)
            k.opt_a.step_device(d_stats=k.ostats.ptr)
            v.sync()
            st = k.pstats.to_host(np.float64, (6,))
            k.theta_a, want = k.ref_a.step(k.theta_a, k.own_gradient(k.opt_a))
            got = k.theta_of(k.pol, k.sa, 2)
            assert np.array_equal(bits(got), bits(k.theta_a)), (it, int((bits(got) != bits(k.theta_a)).sum()))
            assert k.opt_a.state() == k.ref_a.blob()
        ost = k.ostats.to_host(np.float64, (4,))
        assert st[0] == k.R and ost[0] == it + 1 == want[0] and ost[3] == 0 and bits(np.array(ost[2])) == bits(np.array(want[2]))
        losses.append(st[1] / st[0])
    print(who, "loss per iteration", losses)
    assert losses[-1] < losses[0] and all(np.isfinite(losses))
    k.free()


# ---- 4. graphs
def minibatch(k, stream, feats=None, mb=128):
    """a shuffle under the actor optimiser's counter, an actor gradient on a slice, a critic gradient on the next, two steps"""
    k.v.shuffle_rows_device(k.d_rows.ptr, k.n_rows, 9, d_counter=k.opt_a.counter_address, offset=0, stream=stream)
    k.actor_gradient(mb, k.d_rows.ptr, stream, feats)
    k.critic_gradient(mb, k.d_rows.ptr + 8 * mb, stream, feats)
    k.opt_a.step_device(d_stats=k.ostats.ptr, stream=stream)
    k.opt_c.step_device(d_stats=k.ostats.ptr + 32, stream=stream)


def test_a_captured_minibatch_replays_as_three_eager_ones():
    """ONE stream, no forked branches.  (A handle's graph covers an even number of resets + steps and ends at the clock it began at: two
    days of steps, and the minibatch, which takes no tick, in the middle of the second.)  Both runs read the rollout the first collected"""
    mg = buffers()
    a, b = Collected(), Collected()
    st = mg.Stream(0)
    lr2 = mg.DeviceBuffer(8)
    lr2.from_host(np.array([1e-3]))
    # eager, on b's targets and optimisers over a's rollout buffers
    rows_eager = []
    for it in range(3):
        if it == 2:
            for o in (b.opt_a, b.opt_c):
                o.set_lr_device(lr2.ptr, st.ptr)
        minibatch(b, st.ptr, a.roll)
        st.sync()
        rows_eager.append(b.d_rows.to_host(np.int64, (b.n_rows,)))
        if it == 1:
            theta2, blob2 = b.theta_of(b.crit, b.sc, 0), b.opt_c.state()
    # set_lr_device was followed: the third step restated from the second's state, the gradient in the buffers and the new lr
    b.ref_c.load(blob2)
    b.ref_c.lr = np.float64(1e-3)
    theta3, _ = b.ref_c.step(theta2, b.own_gradient(b.opt_c))
    assert np.array_equal(bits(theta3), bits(b.theta_of(b.crit, b.sc, 0))) and b.opt_c.state() == b.ref_c.blob()
    # captured on a
    v = a.v
    acts, packed, obs0 = mg.DeviceBuffer(N_ENVS * v.act_dim * 4), mg.DeviceBuffer(N_ENVS * (v.obs_dim + 2) * 4), mg.DeviceBuffer(N_ENVS * v.obs_dim * 4)
    v.random_actions_device(acts.ptr, 5, 0, st.ptr)
    v.reset_device(obs0.ptr, stream=st.ptr)  # (the rollout left the handle six slots into its day: back to the clock a replay ends at)
    st.sync()
    v.graph_begin(st.ptr)
    for i in range(192):
        if i % 96 == 0:
            v.reset_device(obs0.ptr, stream=st.ptr)
        v.step_device_packed(acts.ptr, packed.ptr, stream=st.ptr)
        if i == 130:
            minibatch(a, st.ptr)
    with pytest.raises(_lib.ChubError, match="chub_graph_begin and chub_graph_end"):
        v.make_adam(a.crit)
    with pytest.raises(_lib.ChubError, match="chub_graph_begin and chub_graph_end"):
        a.opt_a.state()
    graph = v.graph_end(st.ptr)
    st.sync()
    assert a.opt_a.state() == al.Adam(a.ref_a.n, a.ref_a.decays).blob(), "a recording runs nothing"
    rows_replay = []
    for it in range(3):
        if it == 2:
            for o in (a.opt_a, a.opt_c):
                o.set_lr_device(lr2.ptr, st.ptr)
        v.graph_launch(graph, st.ptr)
        st.sync()
        rows_replay.append(a.d_rows.to_host(np.int64, (a.n_rows,)))
    for it in range(3):
        assert np.array_equal(rows_replay[it], rows_eager[it]) and np.array_equal(rows_replay[it], al.shuffle_rows(9, it, a.n_rows)), it
        assert np.array_equal(np.sort(rows_replay[it]), np.arange(a.n_rows))
    assert not np.array_equal(rows_replay[0], rows_replay[1]) and not np.array_equal(rows_replay[1], rows_replay[2])
    assert a.opt_a.state() == b.opt_a.state() and a.opt_c.state() == b.opt_c.state()
    assert np.frombuffer(a.opt_a.state()[:8], dtype=np.int64)[0] == 3
    assert np.array_equal(bits(a.theta_of(a.pol, a.sa, 2)), bits(b.theta_of(b.pol, b.sa, 2)))
    assert np.array_equal(bits(a.theta_of(a.crit, a.sc, 0)), bits(b.theta_of(b.crit, b.sc, 0)))
    assert np.array_equal(a.ostats.to_host(np.uint64, (8,)), b.ostats.to_host(np.uint64, (8,)))
    v.graph_destroy(graph)
    close_all(acts, packed, obs0, lr2)
    a.free()
    b.free()
    st.destroy()


def test_set_lr_device_is_followed():
    """the same gradient twice on two optimisers, one of which gets a new lr from device memory in between: the restatement with that lr"""
    mg = buffers()
    c = [x for x in CASES if x.name == "critic-13-1-does_not_clip"][0]
    v = make("philox", al.POLICY_HUB, N_ENVS)
    d = Dev(v, c)
    d.step(c.grads[0])
    lr = mg.DeviceBuffer(8)
    lr.from_host(np.array([0.0625]))
    d.opt.set_lr_device(lr.ptr)
    d.ref.lr = np.float64(0.0625)
    d.step(c.grads[1])
    d.check("new lr")
    d.opt.set_hyper(**dict(c.hyper, lr=0.5, eps=1e-6))
    d.ref.set_hyper(0.5, c.hyper["betas"], 1e-6, c.hyper["weight_decay"], c.hyper["max_grad_norm"])
    d.step(c.grads[2])
    d.check("set_hyper")
    close_all(lr)
    d.free()
    v.close()


# ---- 6. refusals
def test_refusals_leave_the_state_untouched():
    c = [x for x in CASES if x.name == "policy-13-33-31-47-clips-decay-log_std"][0]
    c0 = [x for x in CASES if x.name == "policy-13-33-31-47-clips-decay"][0]
    v = make("philox", al.POLICY_HUB, N_ENVS)
    d, d0 = Dev(v, c), Dev(v, c0)
    d.step(c.grads[0])
    d0.step(c0.grads[0])
    blob, blob0 = d.opt.state(), d0.opt.state()
    bad_hypers = [dict(lr=-1.0), dict(lr=np.nan), dict(eps=-1e-8), dict(eps=np.inf), dict(weight_decay=-0.1), dict(max_grad_norm=-1.0),
                  dict(max_grad_norm=np.inf), dict(betas=(1.0, 0.9)), dict(betas=(0.9, 1.0)), dict(betas=(-0.1, 0.9)), dict(betas=(0.9, np.nan))]
    for h in bad_hypers:
        with pytest.raises(_lib.ChubError, match="libchub error -1"):
            v.make_adam(d.target, **h)
        with pytest.raises(_lib.ChubError, match="libchub error -1"):
            d.opt.set_hyper(**h)
    no_layer = list(d.gW)
    no_layer[1] = 0
    for call in (lambda: d.opt.step_device(no_layer, d.gb, d.gls, d.stats.ptr), lambda: d.opt.step_device(d.gW, no_layer, d.gls, d.stats.ptr),
                 lambda: d.opt.step_device(d.gW, d.gb, 0, d.stats.ptr), lambda: d0.opt.step_device(d0.gW, d0.gb, d.gls, d0.stats.ptr),
                 lambda: d.opt.load_state(blob0), lambda: d.opt.set_lr_device(0)):
        with pytest.raises((_lib.ChubError, ValueError)):
            call()
    # a blob of the right size whose n differs is refused by the library itself
    wrong_n = bytearray(blob)
    wrong_n[24:32] = np.array([c.n - 1], dtype=np.int64).tobytes()
    with pytest.raises(_lib.ChubError, match="parameters"):
        d.opt.load_state(bytes(wrong_n))
    with pytest.raises(_lib.ChubError, match="libchub error -1"):
        d.target.get_weights_device(9, d.out.ptr, d.out.ptr)
    with pytest.raises(_lib.ChubError, match="libchub error -1"):
        v.shuffle_rows_device(d.out.ptr, 0, 1)
    with pytest.raises(_lib.ChubError, match="libchub error -1"):
        v.shuffle_rows_device(0, 8, 1)
    with pytest.raises(_lib.ChubError, match="chub_policy_set_exploration first"):
        d0.target.get_log_std()
    v.sync()
    assert d.opt.state() == blob and d0.opt.state() == blob0
    d.check("after the refusals")
    d0.check("after the refusals")
    # closing the target destroys its optimisers first; closing the optimiser afterwards is harmless
    d.target.close()
    d.opt.close()
    d.g.free(), d.out.free(), d.stats.free()
    d0.free()
    v.close()


def test_destroying_the_handle_takes_the_whole_family_with_it():
    """the ownership path no other test walks: chub_destroy while a policy with a population, a gradient object and an optimiser, and a
    critic with an optimiser, are all alive.  Every call returns CHUB_OK, and a fresh handle works afterwards."""
    lib = _lib.load_library()
    rs = np.random.RandomState(5)
    v = make("philox", (2, 3), N_ENVS)
    pol = v.make_policy(pgl.general_layers(rs, [13, 8, 7]))
    pol.set_exploration(KEY, [-0.5, 0.25])
    family = [pol, v.make_population(pol, 2, KEY), v.make_policy_grad(pol, N_ENVS), v.make_adam(pol, **PLAIN)]
    critic = v.make_critic(pgl.general_layers(rs, [13, 8, 1]), max_rows=N_ENVS)
    family += [critic, v.make_adam(critic, **PLAIN)]
    assert lib.chub_destroy(v._h) == 0, lib.chub_last_error()
    v._h = None  # (what v.close() does; the objects went with the handle, so their close() calls nothing)
    close_all(*family)
    w = make("philox", (2, 3), N_ENVS)
    w.reset()
    fresh = w.make_critic(pgl.general_layers(rs, [13, 8, 1]), max_rows=N_ENVS)
    assert np.isfinite(fresh.values(rs.uniform(0, 1, size=(N_ENVS, 13)).astype(F32))).all()
    close_all(fresh)
    w.close()


# ---- 7. torch: the independent reference and the adapter, in child processes that import torch first (as tests/test_gpu_torch_side.py does)
TORCH_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["CHUB_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHUB_ROOT"], "tests"))
import torch  # before libchub: both must share one HIP runtime
torch.cuda.set_device(0)
import test_gpu_adam
getattr(test_gpu_adam, os.environ["CHUB_CHILD"])()
print("TORCH_ADAM_OK")
"""


def in_a_child(name):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], env=dict(os.environ, CHUB_ROOT=root, CHUB_CHILD=name), capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "TORCH_ADAM_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_against_torch_adamw_in_double_precision():
    in_a_child("against_torch_adamw")


def test_the_torch_adapter_closes_the_loop():
    in_a_child("torch_adapter_loop")


TORCH_HYPER = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
TORCH_STEPS = 20


def torch_case():
    """13 -> 64 -> 64 -> 47 with log_std, 20 gradients, a clip norm at the median of their norms: some steps clip, some do not"""
    c = StepCase("13-64-64-47", "policy", "plain", True, 7)
    rs = np.random.RandomState(70)
    grads = [(rs.normal(size=c.n) * 10.0 ** rs.uniform(-3, -1, size=c.n) * (1 + 0.5 * np.sin(k))).astype(F32) for k in range(TORCH_STEPS)]
    max_norm = float(np.median([al.fsum_norm(g) for g in grads]))
    c.hyper = dict(TORCH_HYPER, max_grad_norm=max_norm)
    c.grads = [al.stabilised(g, max_norm) for g in grads]
    return c


def torch_adamw(c):
    """double-precision AdamW (two parameter groups: only W decays) with clip_grad_norm_ on the same f32 gradients -> theta f64 [n]"""
    import torch
    f64 = torch.float64
    params, p = [], 0
    theta0 = al.flatten(c.layers, c.log_std)
    for o, i in c.shapes:
        params.append((torch.tensor(theta0[p:p + o * i].reshape(o, i), dtype=f64, requires_grad=True), True))
        params.append((torch.tensor(theta0[p + o * i:p + o * (i + 1)], dtype=f64, requires_grad=True), False))
        p += o * (i + 1)
    params.append((torch.tensor(theta0[p:], dtype=f64, requires_grad=True), False))
    h = c.hyper
    opt = torch.optim.AdamW([dict(params=[t for t, w in params if w], weight_decay=h["weight_decay"]),
                             dict(params=[t for t, w in params if not w], weight_decay=0.0)], lr=h["lr"], betas=h["betas"], eps=h["eps"], foreach=False)
    for g in c.grads:
        p = 0
        for t, _ in params:
            t.grad = torch.tensor(g[p:p + t.numel()].reshape(t.shape), dtype=f64)
            p += t.numel()
        torch.nn.utils.clip_grad_norm_([t for t, _ in params], h["max_grad_norm"], foreach=False)
        opt.step()
    return np.concatenate([t.detach().numpy().ravel() for t, _ in params])


def against_torch_adamw():
    c = torch_case()
    want = torch_adamw(c)
    v = make("philox", al.POLICY_HUB, N_ENVS)
    d = Dev(v, c)
    d.ref.track_bar()
    clipped = 0
    for g in c.grads:
        got, _ = d.step(g)
        clipped += got[2] < 1.0
    assert 0 < clipped < TORCH_STEPS
    d.check("20 steps")
    diff, bar = np.abs(d.read_theta().astype(np.float64) - want), d.ref.bar["theta"]
    at = int(np.argmax(diff / bar))
    print("against torch's double AdamW after %d steps (%d clipped): largest |diff| %.3e, largest diff / bar %.3f (diff %.3e, bar %.3e there), "
          "largest bar %.3e, largest |theta| %.3e" % (TORCH_STEPS, clipped, diff.max(), (diff / bar).max(), diff[at], bar[at], bar.max(), np.abs(want).max()))
    assert (diff <= bar).all(), (int((diff > bar).sum()), diff[at], bar[at])
    d.free()
    v.close()


def torch_adapter_loop():
    """TorchHubVecEnv: make_optimizer, policy_gradient / value_gradient into the optimiser's buffers, optimizer_step, shuffle_rows under
    the optimiser's counter, policy_weights / critic_weights -- two minibatches, against the restatement stepped with the views' contents"""
    import torch
    from charginghub_env_amd import wrappers
    kw = {k: BASE[k] for k in BASE if k != "station_type_list"}
    env = wrappers.TorchHubVecEnv(N_ENVS, al.POLICY_HUB, ["fast", "slow"], seed=13, rng="philox", **kw)
    rs = np.random.RandomState(5)
    D, A = env.obs_dim, env.vec.act_dim
    la, lc = pgl.general_layers(rs, [D, 33, A]), pgl.general_layers(rs, [D, 33, 1])
    ls = np.array([-0.3, 0.2], dtype=F32)
    pol = env.load_policy(la)
    pol.set_exploration(KEY, ls)
    crit = env.load_critic(lc)
    hyper = dict(lr=1e-2, max_grad_norm=0.5, weight_decay=0.01)
    oa, oc = env.make_optimizer(pol, **hyper), env.make_optimizer(crit, **hyper)
    sa, sc = al.shapes_of(D, [33, A]), al.shapes_of(D, [33, 1])
    ra, rc = al.Adam(al.n_params(sa, 2), al.decay_mask(sa, 2), **hyper), al.Adam(al.n_params(sc), al.decay_mask(sc), **hyper)
    ta, tc = al.flatten(la, ls), al.flatten(lc)
    env.reset()
    T = 4
    ro = env.collect(pol, T)
    vals, final = env.values(crit, ro)
    adv, ret = env.advantages(ro, vals, final)
    for it in range(2):
        rows = env.shuffle_rows(T * N_ENVS, 3, counter=oa)
        torch.cuda.synchronize()
        assert np.array_equal(rows.cpu().numpy(), al.shuffle_rows(3, it, T * N_ENVS))
        grads, gls, _ = env.policy_gradient(ro, adv, rows=rows[:100], into=oa)
        cgrads, _ = env.value_gradient(crit, ro, ret, rows=rows[100:200], into=oc)
        torch.cuda.synchronize()
        ga = al.flatten([(W.cpu().numpy(), b.cpu().numpy()) for W, b in grads], gls.cpu().numpy())
        gc = al.flatten([(W.cpu().numpy(), b.cpu().numpy()) for W, b in cgrads])
        assert np.abs(ga).max() > 0 and np.abs(gc).max() > 0 and grads[0][0].data_ptr() == oa.grads()[0][0]
        sta, stc = env.optimizer_step(oa), env.optimizer_step(oc)
        torch.cuda.synchronize()
        ta, wa = ra.step(ta, ga)
        tc, wc = rc.step(tc, gc)
        assert sta.cpu().numpy()[0] == it + 1 and np.array_equal(sta.cpu().numpy()[[0, 2, 3]], wa[[0, 2, 3]]) and np.array_equal(stc.cpu().numpy()[[0, 2, 3]], wc[[0, 2, 3]])
        (wl, log_std), cl_ = env.policy_weights(pol), env.critic_weights(crit)
        torch.cuda.synchronize()
        assert np.array_equal(bits(al.flatten([(W.cpu().numpy(), b.cpu().numpy()) for W, b in wl], log_std.cpu().numpy())), bits(ta))
        assert np.array_equal(bits(al.flatten([(W.cpu().numpy(), b.cpu().numpy()) for W, b in cl_])), bits(tc))
    # without the keyword the two calls behave as before: tensors of the adapter's own
    grads2, _, _ = env.policy_gradient(ro, adv, rows=rows[:100])
    assert grads2[0][0].data_ptr() != oa.grads()[0][0]
    env.close()
