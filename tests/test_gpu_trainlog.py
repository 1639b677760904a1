"""The training log and the KL stop on the device (include/chub.h, "a training log and a KL stop on the device"), bit for bit:
(1) the three kernels against tests/trainlog_lib.py's restatement on the CPU test's made sequences; (2) the gate in Adam: a held-back step
keeps every bit, an open or cleared gate leaves the step what tests/adam_lib.py restates; (3) a stop made by construction; (4)
chub_ppo_update against its constituent calls issued one by one; (5) a recorded update replayed against eager ones; (6) the torch
adapter's ppo_update and train_log_summary, in a child process; (7) refusals and ownership.
64 envs x [20, 25], T = 6 (384 rows), an actor 13 -> 33 -> 47 with log_std (2062 parameters: three Adam chunks), a critic 13 -> 33 -> 1."""
import numpy as np
import pytest

import adam_lib as al
import policy_grad_lib as pgl
import trainlog_lib as tl
from charginghub_env_amd import _lib
from test_gpu_adam import KEY, N_ENVS, PLAIN, Dev, bits, discounted, to_host
from test_gpu_autoreset import buffers
from test_gpu_pile_obs import BASE, make
from test_gpu_policy import f32
from test_gpu_policy_sample import Roll, close_all

pytestmark = pytest.mark.gpu
F32 = np.float32
SEQ = tl.sequences()
UPDATE = dict(loss="ppo_clip", value_loss="clipped", clip_eps=0.2, value_clip_eps=0.25, ent_coef=0.01)


# ---- 1. the kernels against the fold
@pytest.mark.parametrize("name", list(SEQ))
def test_the_kernels_equal_the_restatement_bit_for_bit(name):
    mg = buffers()
    seq = SEQ[name]
    v = make("philox", (2, 3), N_ENVS)
    log = v.make_train_log()
    assert np.array_equal(tl.bits(log.read()), tl.bits(tl.Log().w)), "a new log is what begin leaves"
    blocks = [mg.DeviceBuffer(48), mg.DeviceBuffer(48), mg.DeviceBuffer(32), mg.DeviceBuffer(32)]
    # something else in the log first: begin must clear it, the gate included
    stop = np.array([8.0, 0.0, 0.0, np.nan, 0.0, 8.0])
    blocks[0].from_host(stop)
    log.record(blocks[0].ptr, 0, "k1", 1.0)
    v.sync()
    assert to_host(log.gate_address, np.int64, (1,))[0] == 1 and log.read()[tl.STOPPED] == 1
    log.begin()
    want = tl.Log()
    for block in seq["blocks"]:
        for buf, st in zip(blocks, block):
            if st is not None:
                buf.from_host(st)
        p = [buf.ptr if st is not None else 0 for buf, st in zip(blocks, block)]
        log.record(p[0], p[1], seq["kind"], seq["kl_limit"])
        log.steps(p[2], p[3])
        v.sync()  # (the next from_host must not overtake the launches)
        want.record(block[0], block[1], seq["kind"], seq["kl_limit"])
        want.steps(block[2], block[3])
    got = log.read()
    assert np.array_equal(tl.bits(got), tl.bits(want.w)), (name, got, want.w)
    assert to_host(log.gate_address, np.int64, (1,))[0] == want.gate == (seq["stopped_at"] is not None)
    assert (None if got[tl.STOP_INDEX] < 0 else int(got[tl.STOP_INDEX])) == seq["stopped_at"]
    close_all(*blocks)
    log.close()
    v.close()


# ---- 2. the gate in Adam
class Case(object):
    """what test_gpu_adam.Dev asks of a case: an actor with log_std, its weights and four gradients"""

    def __init__(self, F, widths, seed):
        self.name = "policy-%d-%s-log_std" % (F, "-".join(str(w) for w in widths))
        self.kind, self.F, self.widths, self.explore, self.clips = "policy", F, widths, True, True
        self.hyper = dict(PLAIN, max_grad_norm=0.5, weight_decay=0.01)
        self.shapes, self.G = al.shapes_of(F, widths), 2
        self.n = al.n_params(self.shapes, 2)
        rs = np.random.RandomState(seed)
        self.layers = pgl.general_layers(rs, [F] + list(widths))
        self.log_std = np.array([-0.5, 0.25], dtype=F32)
        self.grads = [al.stabilised((rs.normal(size=self.n) * 10.0 ** rs.uniform(-2, 0.5, size=self.n)).astype(F32), 0.5) for _ in range(4)]


def held_back_step(d, g, gate, what):
    """one step with the gate word at 1: every bit stays, the stats say 2"""
    gate.from_host(np.array([1], dtype=np.int64))
    blob, t = d.opt.state(), d.ref.t
    d.g.from_host(g)
    d.stats.from_host(np.full(4, np.nan))
    d.opt.step_device(d.gW, d.gb, d.gls, d.stats.ptr)
    d.v.sync()
    st = d.stats.to_host(np.float64, (4,))
    exact = al.fsum_norm(g)
    assert st[0] == t and st[2] == 0 and st[3] == 2 and abs(st[1] - exact) <= len(g) * al.U64 * exact, (what, st, t, exact)
    d.check(what)  # (theta through get_weights_device, t, p1, p2, m, v through get_state: the restatement has not moved)
    assert d.opt.state() == blob
    return st


def test_a_closed_gate_holds_the_step_back_and_an_open_one_changes_nothing():
    mg = buffers()
    c = Case(13, [33, 47], 61)
    assert c.n == 2062 and al.plan(c.shapes, 2)["step_workgroups"] == 3
    v = make("philox", al.POLICY_HUB, N_ENVS)
    d = Dev(v, c)
    gate = mg.DeviceBuffer(8)
    gate.from_host(np.array([0], dtype=np.int64))
    d.opt.set_gate(gate.ptr)
    d.step(c.grads[0])  # (the gate at 0: the restatement's step)
    d.check("gate at 0")
    held = held_back_step(d, c.grads[1], gate, "gate at 1")
    nan = c.grads[1].copy()
    nan[5] = np.nan  # (the gate comes before the norm: held back, not skipped)
    gate.from_host(np.array([1], dtype=np.int64))
    d.g.from_host(nan)
    d.opt.step_device(d.gW, d.gb, d.gls, d.stats.ptr)
    v.sync()
    st = d.stats.to_host(np.float64, (4,))
    assert st[3] == 2 and np.isnan(st[1]) and st[0] == 1
    d.check("gate at 1, a norm that is not finite")
    gate.from_host(np.array([0], dtype=np.int64))
    got, want = d.step(c.grads[1])
    assert got[0] == 2 == want[0] and got[3] == 0 and tl.bits(got[1:2])[0] == tl.bits(held[1:2])[0], "the norm a held-back step reports is the step's own"
    d.check("gate at 0 again")
    gate.from_host(np.array([-1], dtype=np.int64))  # (any value but 0 closes it)
    held_back_step(d, c.grads[2], gate, "gate at -1")
    d.opt.set_gate(0)  # cleared while the word is not 0: an ungated step
    got, want = d.step(c.grads[2])
    assert got[0] == 3 == want[0] and got[3] == 0
    d.check("gate cleared")
    close_all(gate)
    d.free()
    v.close()


def test_a_closed_gate_holds_every_workgroup_back_on_their_second_trip():
    """64 -> 256 -> 224 -> 47: 83 chunks on 64 workgroups.  A gate that workgroup 0 alone consulted would leave 82 chunks stepped"""
    mg = buffers()
    c = Case(64, [256, 224, 47], 62)
    assert al.plan(c.shapes, 2)["step_workgroups"] == 64 < (c.n + al.CHUNK - 1) // al.CHUNK
    v = make("philox", al.POLICY_HUB, N_ENVS)
    d = Dev(v, c)
    gate = mg.DeviceBuffer(8)
    d.opt.set_gate(gate.ptr)
    gate.from_host(np.array([0], dtype=np.int64))
    d.step(c.grads[0])
    held_back_step(d, c.grads[1], gate, "wide, gate at 1")
    close_all(gate)
    d.free()
    v.close()


# ---- 3. to 5.: a collected rollout, both nets, both optimisers
class Rig(object):
    T = 6

    def __init__(self, lr=3e-3):
        mg = buffers()
        rs = np.random.RandomState(41)
        self.v = v = make("philox", al.POLICY_HUB, N_ENVS, seed=6)
        D = v.obs_dim
        self.n_rows = self.T * N_ENVS
        self.actor_layers = pgl.general_layers(rs, [D, 33, v.act_dim])
        self.critic_layers = pgl.general_layers(rs, [D, 33, 1])
        self.ls = np.array([-0.2, 0.1], dtype=F32)
        self.pol = v.make_policy(self.actor_layers)
        self.pol.set_exploration(KEY, self.ls)
        self.crit = v.make_critic(self.critic_layers, max_rows=self.n_rows)
        self.roll = Roll(v, self.pol, self.T)
        self.roll.collect("lockstep")
        h = self.roll.host()
        self.logp = f32(h["logp"]).reshape(-1)
        ret = discounted(f32(h["packed"]), D).reshape(-1)
        n = self.n_rows
        self.dev = {k: mg.DeviceBuffer(4 * n) for k in ("ret", "adv", "v_old", "logp_old")}
        self.dev["ret"].from_host(ret)
        self.dev["adv"].from_host(rs.normal(size=n).astype(F32))
        self.dev["v_old"].from_host((ret + 0.3 * rs.normal(size=n)).astype(F32))
        self.dev["logp_old"].from_host(self.logp)
        self.d_rows = mg.DeviceBuffer(8 * n)
        self.pstats, self.cstats, self.sa, self.sc = mg.DeviceBuffer(48), mg.DeviceBuffer(48), mg.DeviceBuffer(32), mg.DeviceBuffer(32)
        self.grad = v.make_policy_grad(self.pol, n)
        hyper = dict(PLAIN, lr=lr, max_grad_norm=0.5, weight_decay=0.01)
        self.opt_a, self.opt_c = v.make_adam(self.pol, **hyper), v.make_adam(self.crit, **hyper)
        assert self.opt_a.n_params == 2062
        self.log = v.make_train_log()

    def gradients(self, R, d_rows, stream=0):
        r = self.roll
        gW, gb, gls = self.opt_a.grads()
        self.grad.grad_device(R, self.n_rows, r.ptr("feat"), r.ptr("u"), self.dev["adv"].ptr, d_pile_bits=r.ptr("bits"), d_logp_old=self.dev["logp_old"].ptr,
                              d_rows=d_rows, loss=UPDATE["loss"], clip_eps=UPDATE["clip_eps"], ent_coef=UPDATE["ent_coef"], d_gW=gW, d_gb=gb,
                              d_glog_std=gls, d_stats=self.pstats.ptr, stream=stream)
        gW, gb, _ = self.opt_c.grads()
        self.crit.grad_device(R, self.n_rows, r.ptr("feat"), self.dev["ret"].ptr, d_v_old=self.dev["v_old"].ptr, d_rows=d_rows, loss=UPDATE["value_loss"],
                              clip_eps=UPDATE["value_clip_eps"], d_gW=gW, d_gb=gb, d_stats=self.cstats.ptr, stream=stream)

    def steps(self, stream=0):
        self.opt_a.step_device(d_stats=self.sa.ptr, stream=stream)
        self.opt_c.step_device(d_stats=self.sc.ptr, stream=stream)

    def minibatch(self, R, d_rows, kl, kl_limit, log=True, stream=0, keep=None):
        """the six calls of one minibatch; keep (a list): the four stats blocks are read back into it (that synchronises)"""
        self.gradients(R, d_rows, stream)
        if log:
            self.log.record(self.pstats.ptr, self.cstats.ptr, kl, kl_limit, stream)
        self.steps(stream)
        if log:
            self.log.steps(self.sa.ptr, self.sc.ptr, stream)
        if keep is not None:
            self.v.sync()
            keep.append([b.to_host(np.float64, (k,)) for b, k in ((self.pstats, 6), (self.cstats, 6), (self.sa, 4), (self.sc, 4))])

    def by_hand(self, epochs, mb, key, kl="k3", kl_limit=0.0, log=True, stream=0, keep=None):
        """what chub_ppo_update documents, call by call"""
        M, last = tl.split(self.n_rows, mb)
        if log:
            self.log.begin(stream)
            for o in (self.opt_a, self.opt_c):
                o.set_gate(self.log.gate_address)
        for e in range(epochs):
            self.v.shuffle_rows_device(self.d_rows.ptr, self.n_rows, key, d_counter=self.opt_a.counter_address, offset=e, stream=stream)
            for i in range(M):
                self.minibatch(mb if i + 1 < M else last, self.d_rows.ptr + 8 * i * mb, kl, kl_limit, log, stream, keep)
        for o in (self.opt_a, self.opt_c):
            o.set_gate(0)

    def update(self, n_epochs, mb, seed, kl="k3", kl_limit=0.0, log=True, stream=0, **other):
        r = self.roll
        kw = dict(n_rows=self.n_rows, d_features=r.ptr("feat"), d_u=r.ptr("u"), d_logp_old=self.dev["logp_old"].ptr, d_adv=self.dev["adv"].ptr,
                  d_ret=self.dev["ret"].ptr, d_rows=self.d_rows.ptr, epochs=n_epochs, minibatch_rows=mb, key=seed, d_pile_bits=r.ptr("bits"),
                  d_v_old=self.dev["v_old"].ptr, kl=kl, kl_limit=kl_limit, log=self.log if log is True else (log or None), stream=stream, **UPDATE)
        kw.update(other)
        args = [kw.pop(k) for k in ("grad", "critic", "actor_opt", "critic_opt")] if "grad" in kw else [self.grad, self.crit, self.opt_a, self.opt_c]
        self.v.ppo_update(*args, **kw)

    def snapshot(self, log=True):
        """everything an update may touch, as bits"""
        self.v.sync()
        out = dict(theta_a=bits(al.flatten(self.pol.get_weights(), self.pol.get_log_std())), theta_c=bits(al.flatten(self.crit.get_weights())),
                   state_a=self.opt_a.state(), state_c=self.opt_c.state(), rows=self.d_rows.to_host(np.int64, (self.n_rows,)))
        if log:
            out["log"] = tl.bits(self.log.read())
            out["gate"] = to_host(self.log.gate_address, np.int64, (1,))
        return out

    def free(self):
        close_all(*(list(self.dev.values()) + [self.d_rows, self.pstats, self.cstats, self.sa, self.sc, self.log, self.opt_a, self.opt_c, self.grad, self.roll,
                                               self.crit, self.pol, self.v]))


def same(a, b, what, keys=None):
    for k in keys or a:
        if isinstance(a[k], bytes):
            assert a[k] == b[k], (what, k)
        else:
            assert np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


def test_a_stop_made_by_construction():
    """four minibatches over rows 0 .. 95, 96 .. 191, 192 .. 287, 288 .. 383, lr 1e-4; logp_old is the collected logp, plus 0.5 on the
    third range: K1 of the third minibatch is about 0.5, of the others about 0.  kl_limit = 0.25"""
    LIMIT, R = 0.25, 96
    rigs = [Rig(lr=1e-4) for _ in range(3)]
    free, gated, two = rigs
    for k in rigs:
        logp_old = k.logp.copy()
        logp_old[2 * R:3 * R] += F32(0.5)
        k.dev["logp_old"].from_host(logp_old)
        k.d_rows.from_host(np.arange(k.n_rows, dtype=np.int64))
        k.log.begin()
    # ungated, no limit: the four estimates lie where the construction puts them
    seen = []
    for i in range(4):
        free.minibatch(R, free.d_rows.ptr + 8 * R * i, "k1", 0.0, keep=seen)
    kls = [st[0][3] / st[0][0] for st in seen]
    print("K1 per minibatch, ungated:", kls)
    assert all(st[0][0] == R for st in seen)
    assert abs(kls[0]) < 0.05 and abs(kls[1]) < 0.05 and abs(kls[3]) < 0.05 and 0.45 < kls[2] < 0.55
    assert max(kls[0], kls[1], kls[3]) < LIMIT < kls[2]
    w = free.log.read()
    assert w[tl.STOPPED] == 0 and w[tl.COUNTED] == 4 and w[tl.ACTOR_OPT] == 4 and w[tl.CRITIC_OPT] == 4 and w[tl.KL_MAX] == kls[2]
    # gated
    for o in (gated.opt_a, gated.opt_c):
        o.set_gate(gated.log.gate_address)
    seen = []
    for i in range(4):
        gated.minibatch(R, gated.d_rows.ptr + 8 * R * i, "k1", LIMIT, keep=seen)
    w = gated.log.read()
    assert w[tl.STOP_INDEX] == 2 and w[tl.STOPPED] == 1 and w[tl.COUNTED] == 3 and w[tl.AFTER_STOP] == 1
    assert to_host(gated.log.gate_address, np.int64, (1,))[0] == 1
    assert [st[2][3] for st in seen] == [0, 0, 2, 2] == [st[3][3] for st in seen] and [st[2][0] for st in seen] == [1, 2, 2, 2]
    for base in (tl.ACTOR_OPT, tl.CRITIC_OPT):
        assert list(w[base:base + 3]) == [2, 0, 2], w[base:base + 6]
        assert w[base + 3] == ((seen[0][2 if base == tl.ACTOR_OPT else 3][1] + seen[1][2 if base == tl.ACTOR_OPT else 3][1])
                               + seen[2][2 if base == tl.ACTOR_OPT else 3][1]) + seen[3][2 if base == tl.ACTOR_OPT else 3][1]
    assert w[tl.ACTOR] == 3 * R and w[tl.KL_LAST] == w[tl.KL_MAX] == seen[2][0][3] / seen[2][0][0]
    # the first two minibatches alone
    for i in range(2):
        two.minibatch(R, two.d_rows.ptr + 8 * R * i, "k1", LIMIT)
    same(gated.snapshot(), two.snapshot(), "gated against two minibatches", ("theta_a", "theta_c", "state_a", "state_c"))
    assert not np.array_equal(gated.snapshot()["theta_a"], free.snapshot()["theta_a"])
    for k in rigs:
        k.free()


@pytest.mark.parametrize("kl_limit", [0.0, 1e-9])
def test_ppo_update_equals_its_constituent_calls(kl_limit):
    """2 epochs x 4 minibatches of 100 rows, the last of 84.  kl_limit = 1e-9: the first minibatch's K3 is of the order of 1e-14 (the weights are the
    collecting ones: every ratio is 1 to within f32's rounding of logp), the second's, one step of lr 3e-3 later, of the order of 1e-4"""
    one, hand, nolog = Rig(), Rig(), Rig()
    assert tl.split(one.n_rows, 100) == (4, 84)
    one.update(2, 100, 31, "k3", kl_limit)
    hand.by_hand(2, 100, 31, "k3", kl_limit)
    a, b = one.snapshot(), hand.snapshot()
    same(a, b, "one call against the calls one by one")
    w = one.log.read()
    print("log", w)
    t_then = 4 if kl_limit == 0.0 else 1  # (the actor optimiser's step count when the second epoch's shuffle ran; its offset is 1)
    assert np.array_equal(np.sort(a["rows"]), np.arange(one.n_rows)) and np.array_equal(a["rows"], al.shuffle_rows(31, t_then + 1, one.n_rows))
    if kl_limit == 0.0:
        assert w[tl.COUNTED] == 8 and w[tl.STOPPED] == 0 and w[tl.ACTOR] == 2 * one.n_rows == w[tl.CRITIC] and w[tl.ACTOR_OPT] == 8 == w[tl.CRITIC_OPT]
        assert np.frombuffer(a["state_a"][:8], dtype=np.int64)[0] == 8
        nolog.update(2, 100, 31, log=False)
        same(a, nolog.snapshot(log=False), "without a log", ("theta_a", "theta_c", "state_a", "state_c", "rows"))
    else:
        assert w[tl.STOP_INDEX] == 1 and w[tl.COUNTED] == 2 and w[tl.AFTER_STOP] == 6 and w[tl.ACTOR_OPT] == 1 and w[tl.ACTOR_OPT + 2] == 7
        assert np.frombuffer(a["state_a"][:8], dtype=np.int64)[0] == 1
    # the optimisers have their own gate back (none): a step after the update is taken, stopped log or not
    one.steps()
    one.v.sync()
    assert one.sa.to_host(np.float64, (4,))[3] == 0
    for k in (one, hand, nolog):
        k.free()


def test_a_recorded_update_replays_as_eager_ones():
    """one ppo_update with a log, recorded on a created stream after an eager run, replayed twice, against three eager updates.  (A
    handle's graph covers an even number of resets + steps and ends at the clock it began at: two days of steps, the update in the second.)
    The log after each replay is that update's alone: begin is inside the recording"""
    mg = buffers()
    a, b = Rig(), Rig()
    st = mg.Stream(0)
    run = lambda k: k.update(1, 100, 32, "k3", 0.0, stream=st.ptr)
    eager = []
    for it in range(3):
        run(a)
        st.sync()
        eager.append(a.snapshot())
    run(b)
    st.sync()
    same(eager[0], b.snapshot(), "the eager run before the recording")
    v = b.v
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
            run(b)
    for call in (v.make_train_log, b.log.read, b.log.close):
        with pytest.raises(_lib.ChubError, match="chub_graph_begin and chub_graph_end"):
            call()
    graph = v.graph_end(st.ptr)
    st.sync()
    same(eager[0], b.snapshot(), "a recording runs nothing")
    for it in (1, 2):
        v.graph_launch(graph, st.ptr)
        st.sync()
        same(eager[it], b.snapshot(), ("replay", it))
    assert not np.array_equal(eager[1]["log"], eager[2]["log"]) and eager[2]["log"].view(np.float64)[tl.COUNTED] == 4
    assert np.frombuffer(eager[2]["state_a"][:8], dtype=np.int64)[0] == 12
    v.graph_destroy(graph)
    close_all(acts, packed, obs0)
    a.free()
    b.free()
    st.destroy()


# ---- 7. refusals and ownership
def test_refusals_leave_weights_states_and_log_untouched():
    k = Rig()
    k.update(1, 100, 5)
    before = k.snapshot()
    w2 = make("philox", (2, 3), N_ENVS)
    rs = np.random.RandomState(3)
    other_critic = w2.make_critic(pgl.general_layers(rs, [13, 8, 1]), max_rows=k.n_rows)
    other_opt = w2.make_adam(other_critic, **PLAIN)
    other_log = w2.make_train_log()
    pol2 = k.v.make_policy(k.actor_layers)
    pol2.set_exploration(KEY, k.ls)
    opt2 = k.v.make_adam(pol2, **PLAIN)
    crit2 = k.v.make_critic(k.critic_layers, max_rows=k.n_rows)
    small = k.v.make_critic(k.critic_layers, max_rows=50)
    small_opt = k.v.make_adam(small, **PLAIN)
    own = [k.grad, k.crit, k.opt_a, k.opt_c]
    refused = [
        ("epochs is at least 1", dict(epochs=0)), ("minibatch_rows is at least 1", dict(minibatch_rows=0)),
        ("minibatch_rows is at most", dict(minibatch_rows=k.n_rows + 1)), ("null d_rows", dict(d_rows=0)),
        ("minibatch_rows is at most", dict(grad=k.grad, critic=small, actor_opt=k.opt_a, critic_opt=small_opt)),
        ("one handle", dict(grad=k.grad, critic=other_critic, actor_opt=k.opt_a, critic_opt=other_opt)),
        ("one handle", dict(log=other_log)),
        ("not an optimiser of the gradient object's policy", dict(grad=k.grad, critic=k.crit, actor_opt=opt2, critic_opt=k.opt_c)),
        ("not an optimiser of the critic", dict(grad=k.grad, critic=crit2, actor_opt=k.opt_a, critic_opt=k.opt_c)),
        ("not an optimiser of the gradient object's policy", dict(grad=k.grad, critic=k.crit, actor_opt=k.opt_c, critic_opt=k.opt_c)),
        ("kl_kind", dict(kl=7)), ("kl_limit", dict(kl_limit=-1.0)), ("kl_limit", dict(kl_limit=float("nan"))),
        ("n_rows is at least 1", dict(n_rows=0)),
        ("chub_ppo_update: chub_policy_grad_device: clip_eps", dict(clip_eps=1.5)),
        ("chub_ppo_update: chub_policy_grad_device: null argument", dict(d_u=0)),
        ("chub_ppo_update: chub_policy_grad_device: ent_coef", dict(ent_coef=float("inf"))),
        ("chub_ppo_update: chub_policy_grad_device: loss", dict(loss=9)),
        ("chub_ppo_update: chub_policy_grad_device: ld_features", dict(ld_features=12)),
        ("chub_ppo_update: chub_critic_grad_device: clip_eps", dict(value_clip_eps=-1.0)),
        ("chub_ppo_update: chub_critic_grad_device: null argument", dict(d_ret=0)),
        ("chub_ppo_update: chub_critic_grad_device: null argument", dict(d_v_old=0)),
        ("chub_ppo_update: chub_critic_grad_device: loss", dict(value_loss=9)),
    ]
    for text, kw in refused:
        with pytest.raises(_lib.ChubError, match=text):
            k.update(1, 100, 5, **kw)
    for call in (lambda: k.log.record(k.pstats.ptr, k.cstats.ptr, 2, 0.1), lambda: k.log.record(k.pstats.ptr, k.cstats.ptr, "k1", -0.1),
                 lambda: k.log.record(k.pstats.ptr, k.cstats.ptr, "k1", float("nan"))):
        with pytest.raises(_lib.ChubError, match="libchub error -1"):
            call()
    with pytest.raises(ValueError):
        k.log.record(k.pstats.ptr, k.cstats.ptr, "k2", 0.1)
    same(before, k.snapshot(), "after the refusals")
    # a log destroyed while an optimiser points at its gate: the gate is cleared, the next step is an ungated one
    doomed = k.v.make_train_log()
    k.opt_a.set_gate(doomed.gate_address)
    doomed.close()
    k.steps()
    k.v.sync()
    assert k.sa.to_host(np.float64, (4,))[3] == 0
    assert own == [k.grad, k.crit, k.opt_a, k.opt_c]
    close_all(small_opt, small, crit2, opt2, pol2, other_log, other_opt, other_critic, w2)
    k.free()


def test_destroying_the_handle_takes_logs_gates_and_a_graph_in_its_stride():
    """chub_destroy with a log, two optimisers pointing at its gate and a recorded graph alive: CHUB_OK, and a fresh handle works"""
    mg = buffers()
    lib = _lib.load_library()
    k = Rig()
    st = mg.Stream(0)
    v = k.v
    for o in (k.opt_a, k.opt_c):
        o.set_gate(k.log.gate_address)
    acts, packed, obs0 = mg.DeviceBuffer(N_ENVS * v.act_dim * 4), mg.DeviceBuffer(N_ENVS * (v.obs_dim + 2) * 4), mg.DeviceBuffer(N_ENVS * v.obs_dim * 4)
    v.random_actions_device(acts.ptr, 5, 0, st.ptr)
    v.reset_device(obs0.ptr, stream=st.ptr)
    st.sync()
    v.graph_begin(st.ptr)
    for i in range(2):
        v.step_device_packed(acts.ptr, packed.ptr, stream=st.ptr)
        k.update(1, 192, 3, stream=st.ptr)
    graph = v.graph_end(st.ptr)
    st.sync()
    more = v.make_train_log()
    assert lib.chub_destroy(v._h) == 0, lib.chub_last_error()
    v._h = None  # (what v.close() does; the objects went with the handle, so their close() calls nothing)
    v.graph_destroy(graph)
    close_all(more, acts, packed, obs0)
    k.free()
    st.destroy()
    w = make("philox", (2, 3), N_ENVS)
    log = w.make_train_log()
    log.begin()
    assert log.read()[tl.STOP_INDEX] == -1
    close_all(log, w)


# ---- 6. the torch adapter, in a child process that imports torch first (as tests/test_gpu_adam.py does)
TORCH_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["CHUB_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHUB_ROOT"], "tests"))
import torch  # before libchub: both must share one HIP runtime
torch.cuda.set_device(0)
import test_gpu_trainlog
getattr(test_gpu_trainlog, os.environ["CHUB_CHILD"])()
print("TORCH_TRAINLOG_OK")
"""


def test_the_adapters_update_and_summary():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], env=dict(os.environ, CHUB_ROOT=root, CHUB_CHILD="adapter_update_and_summary"),
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "TORCH_TRAINLOG_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def adapter_update_and_summary():
    """TorchHubVecEnv.ppo_update on one adapter against the adapter's own calls one by one on a twin, the stats of every minibatch read
    back there; train_log_summary against the same quantities formed in torch from those stats: the same f64 sums in the same order"""
    import torch
    from charginghub_env_amd import wrappers
    kw = {k: BASE[k] for k in BASE if k != "station_type_list"}
    T, MB, EPOCHS, KEYS = 6, 100, 2, 19
    hyper = dict(lr=3e-3, max_grad_norm=0.5, weight_decay=0.01)
    rs = np.random.RandomState(5)
    D = 13
    la, lc = pgl.general_layers(rs, [D, 33, 47]), pgl.general_layers(rs, [D, 33, 1])
    made = []
    for _ in range(2):
        env = wrappers.TorchHubVecEnv(N_ENVS, al.POLICY_HUB, ["fast", "slow"], seed=13, rng="philox", **kw)
        pol = env.load_policy(la)
        pol.set_exploration(KEY, np.array([-0.3, 0.2], dtype=F32))
        crit = env.load_critic(lc)
        oa, oc = env.make_optimizer(pol, **hyper), env.make_optimizer(crit, **hyper)
        env.reset()
        ro = env.collect(pol, T, logp_piles="decidable")
        vals, final = env.values(crit, ro)
        adv, ret, adv_stats = env.advantages(ro, vals, final, stats=True)
        v_old = vals[:T].clone()
        made.append((env, pol, crit, oa, oc, ro, adv, ret, adv_stats, v_old))
    # one call, with a target_kl that stops nothing, then the summary
    env, pol, crit, oa, oc, ro, adv, ret, adv_stats, v_old = made[0]
    log = env.make_train_log()
    rows = env.ppo_update(ro, adv, ret, oa, oc, epochs=EPOCHS, minibatch_rows=MB, key=KEYS, clip_eps=0.2, ent_coef=0.01, v_old=v_old, adv_stats=adv_stats,
                          target_kl=1e3, log=log)
    got = env.train_log_summary(log)
    got_k1 = env.train_log_summary(log, kl="k1")
    # the twin, call by call
    env2, pol2, crit2, oa2, oc2, ro2, adv2, ret2, adv_stats2, v_old2 = made[1]
    f64 = torch.float64
    ps, cs = torch.zeros(6, dtype=f64), torch.zeros(6, dtype=f64)
    oa_w, oc_w = torch.zeros(6, dtype=f64), torch.zeros(6, dtype=f64)
    kl_max, n_mb = None, 0
    for e in range(EPOCHS):
        rows2 = env2.shuffle_rows(T * N_ENVS, KEYS, counter=oa2, offset=e)
        for i in range(4):
            r = rows2[i * MB:(i + 1) * MB]
            _, _, st = env2.policy_gradient(ro2, adv2, rows=r, clip_eps=0.2, ent_coef=0.01, adv_stats=adv_stats2, into=oa2)
            _, vst = env2.value_gradient(crit2, ro2, ret2, rows=r, loss="clipped", clip_eps=0.2, v_old=v_old2, into=oc2)
            sa, sc = env2.optimizer_step(oa2), env2.optimizer_step(oc2)
            torch.cuda.synchronize()
            st, vst = st.cpu(), vst.cpu()
            ps, cs = ps + st, cs + vst
            kl = (st[5] / st[0] - 1.0) + st[3] / st[0]
            kl_max = kl if kl_max is None or kl > kl_max else kl_max
            n_mb += 1
            for acc, s in ((oa_w, sa.cpu()), (oc_w, sc.cpu())):
                assert s[3] == 0
                acc[0] += 1
                acc[3] = acc[3] + s[1]
                acc[4] = torch.maximum(acc[4], s[1])
                acc[5] += float(s[2] < 1.0)
    torch.cuda.synchronize()
    assert torch.equal(rows.cpu(), rows2.cpu())
    (w1, l1), (w2, l2) = env.policy_weights(pol), env2.policy_weights(pol2)
    torch.cuda.synchronize()
    assert all(torch.equal(a.cpu(), b.cpu()) and torch.equal(c.cpu(), d.cpu()) for (a, c), (b, d) in zip(w1, w2)) and torch.equal(l1.cpu(), l2.cpu())
    assert oa.state() == oa2.state() and oc.state() == oc2.state()
    var = cs[5] / cs[0] - (cs[4] / cs[0]) ** 2
    want = {"n_minibatches": n_mb, "stopped_at": None, "approx_kl": float((ps[5] / ps[0] - 1.0) + ps[3] / ps[0]), "approx_kl_max": float(kl_max),
            "clip_fraction": float(ps[4] / ps[0]), "entropy": float(ps[2] / ps[0]), "policy_loss": float(ps[1] / ps[0]),
            "value_loss": float(cs[1] / cs[0]), "value_clip_fraction": float(cs[2] / cs[0]),
            "explained_variance": float(1.0 - (cs[3] / cs[0]) / var.clamp_min(1e-12))}
    for name, acc in (("policy_opt", oa_w), ("critic_opt", oc_w)):
        want[name] = {"steps": int(acc[0]), "skipped": 0, "held_back": 0, "grad_norm_mean": float(acc[3] / acc[0]), "grad_norm_max": float(acc[4]),
                      "clipped_steps": int(acc[5])}
    print("summary", got)
    assert got == want, (got, want)
    assert got_k1["approx_kl"] == float(ps[3] / ps[0]) and {k: x for k, x in got_k1.items() if k != "approx_kl"} == {k: x for k, x in want.items() if k != "approx_kl"}
    assert n_mb == 8 and got["policy_opt"]["steps"] == 8 and np.isfinite([got[k] for k in got if isinstance(got[k], float)]).all()
    # target_kl: SB3's rule is 1.5 * target_kl; a target so small that the second minibatch passes it stops the update there
    log2 = env.make_train_log()
    env.ppo_update(ro, adv, ret, oa, oc, epochs=1, minibatch_rows=MB, key=KEYS, clip_eps=0.2, ent_coef=0.01, v_old=v_old, adv_stats=adv_stats,
                   target_kl=1e-12, log=log2)
    s = env.train_log_summary(log2)
    assert s["stopped_at"] is not None and s["policy_opt"]["held_back"] == 4 - s["policy_opt"]["steps"] > 0 and s["n_minibatches"] == s["stopped_at"] + 1
    with pytest.raises(ValueError, match="target_kl needs log"):
        env.ppo_update(ro, adv, ret, oa, oc, epochs=1, minibatch_rows=MB, key=KEYS, clip_eps=0.2, ent_coef=0.01, v_old=v_old, target_kl=0.02)
    env.close()
    env2.close()
