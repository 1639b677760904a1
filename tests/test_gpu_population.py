"""A population of actors on the device (include/chub.h: chub_population_*), held against tests/population_lib.py's numpy definition:
(1) perturb == the definition's members bit for bit, from the trainer's theta and from the centre; (2) the population launch == a plain
policy holding each member's weights, bit for bit, in every output form; (3) set / get / copy of members; (4) the closed loop == the
same calls one by one, == per-member handles of E envs, and in a replayed graph that follows a perturbation between replays; (5) the ES
gradient within the definition's bound, deterministic, exactly zero on equal pairs; (6) no trace in the simulation; (7) refusals;
(8) the torch adapter.  Shapes: F = 13 (k_pad 14), hidden width 33 (one output beyond a tile), S = 2, 45 and 128, members of one and of
two tiles (E = 32, 64)."""
import ctypes as C

import numpy as np
import pytest

import population_lib as popl
from test_gpu_autoreset import Dev, buffers
from test_gpu_parity import hub
from test_gpu_pile_obs import BASE, CANARY, Driver, make
from test_gpu_policy import CANARY64, Act, closed_loop_by_hand, gaussian_layers, packed_pair, same_blocks, upload_layers

pytestmark = pytest.mark.gpu

F32 = np.float32
KEY = 0x0123456789ABCDEF
EXTRA = 64
HUBS = ([20, 25], [1, 1], [64, 64])
NETS = ((), (33,), (64, 33))
SHAPES = ((2, 32), (6, 32), (2, 64))  # (P, E)
ids_hub = lambda p: "%dx%d" % tuple(p)


def same_state(a, b, label):
    """the simulation state of two handles as every reader shows it, with clocks and ticks"""
    ta, tb = a.env_clocks(ticks=True), b.env_clocks(ticks=True)
    assert np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1]), (label, "clocks and ticks")
    for k, (x, y) in enumerate(zip(a.slots() + [a.station_scalars()], b.slots() + [b.station_scalars()])):
        assert np.array_equal(x, y, equal_nan=True), (label, "state array", k)


def u32(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


class LayerBuffers(object):
    """per layer a W and a b buffer in device memory in the trainer's layout, with guard words behind each"""

    def __init__(self, shapes):
        mg = buffers()
        self.shapes = shapes
        self.W = [mg.DeviceBuffer((o * i + EXTRA) * 4) for o, i in shapes]
        self.b = [mg.DeviceBuffer((o + EXTRA) * 4) for o, _ in shapes]

    def fill(self):
        for (o, i), W, b in zip(self.shapes, self.W, self.b):
            W.from_host(np.full(o * i + EXTRA, CANARY, dtype=np.uint32))
            b.from_host(np.full(o + EXTRA, CANARY, dtype=np.uint32))

    def put(self, layers):
        for (W, b), dW, db in zip(layers, self.W, self.b):
            dW.from_host(np.ascontiguousarray(W, dtype=F32))
            db.from_host(np.ascontiguousarray(b, dtype=F32))

    def ptrs(self):
        return [x.ptr for x in self.W], [x.ptr for x in self.b]

    def read(self, l):
        """(W, b) of layer l as u32 words; the guard words are checked"""
        o, i = self.shapes[l]
        W, b = self.W[l].to_host(np.uint32, (o * i + EXTRA,)), self.b[l].to_host(np.uint32, (o + EXTRA,))
        assert (W[o * i:] == CANARY).all() and (b[o:] == CANARY).all(), "the words past an output buffer"
        return W[:o * i].reshape(o, i), b[:o]

    def free(self):
        for x in self.W + self.b:
            x.free()


def member_device(v, pop, out, m):
    """member m through chub_population_get_member_device into guarded buffers -> [(W, b), ..] f32"""
    out.fill()
    v.sync()
    for l in range(len(out.shapes)):
        pop.get_member_device(m, l, out.W[l].ptr, out.b[l].ptr)
    v.sync()
    return [tuple(x.view(F32) for x in out.read(l)) for l in range(len(out.shapes))]


def assert_members(got, want, what):
    for l, ((W, b), (W0, b0)) in enumerate(zip(got, want)):
        bad = np.nonzero(u32(W) != u32(W0))
        assert bad[0].size == 0, (what, "layer", l, "W: first (row, column)", [int(x[0]) for x in bad], bad[0].size)
        assert np.array_equal(u32(b), u32(b0)), (what, "layer", l, "b", np.nonzero(u32(b) != u32(b0))[0][:5])


def sizes_of(v, hidden, head="piles", F=None):
    return [v.obs_dim if F is None else F] + list(hidden) + [v.act_dim if head == "piles" else 4]


# ---- 1. perturb
@pytest.mark.parametrize("piles", HUBS, ids=ids_hub)
def test_perturb_equals_the_definition_bit_for_bit(piles):
    """every member and layer after perturb_device, read back in the trainer's layout, equals population_lib.members: general f32 theta
    in device memory, two sigmas x two generations; theta = NULL (the centre's own weights); generation g and g + 1 differ; the same call
    twice gives the same bits; guard words behind every buffer read into"""
    rs = np.random.RandomState(sum(piles))
    for P, E in SHAPES:
        v = make("philox", piles, P * E)
        for hidden in NETS:
            sizes = sizes_of(v, hidden)
            shapes = list(zip(sizes[1:], sizes[:-1]))
            centre, theta = gaussian_layers(rs, sizes), gaussian_layers(rs, sizes)
            pol = v.make_policy(centre)
            pop = v.make_population(pol, P, KEY)
            assert pop.n_params == popl.param_count(shapes) and pop.envs_per_member == E
            out, src = LayerBuffers(shapes), LayerBuffers(shapes)
            for m in range(P):
                assert_members(member_device(v, pop, out, m), centre, (piles, P, hidden, "at create", m))
            src.put(theta)
            first = None
            for sigma, g in ((0.05, 3), (0.05, 4), (0.75, 3), (0.75, 0xFFFFFFFF)):
                pop.perturb_device(sigma, g, *src.ptrs())
                want = popl.members(theta, sigma, KEY, g, P)
                got = [member_device(v, pop, out, m) for m in range(P)]
                for m in range(P):
                    assert_members(got[m], want[m], (piles, P, hidden, sigma, g, m))
                if first is None:
                    first = got
                elif (sigma, g) == (0.05, 4):
                    assert all((u32(a[0]) != u32(b[0])).mean() > 0.9 for a, b in zip(first[0], got[0])), "generations g and g + 1 differ"
            pop.perturb_device(0.05, 3, *src.ptrs())
            for m in range(P):
                assert_members(member_device(v, pop, out, m), first[m], (piles, P, hidden, "the same call again", m))
            pop.perturb_device(0.25, 9)  # theta = NULL: the centre policy's current weights, read in the kernel's layout
            want = popl.members(centre, 0.25, KEY, 9, P)
            for m in range(P):
                assert_members(member_device(v, pop, out, m), want[m], (piles, P, hidden, "from the centre", m))
            pop.perturb(0.0, 1, theta)  # the host form; sigma = 0: every member is theta
            for m in (0, P - 1):
                assert_members(member_device(v, pop, out, m), theta, (piles, P, hidden, "sigma 0", m))
            for x in (out, src):
                x.free()
            pop.close()
            pol.close()
        v.close()


# ---- 2. act
def act_equals_member_policies(v, pop, P, E, obs, make_member, what, lds, mask=None):
    """the population launch against one plain policy per member, in every output form; -> number of comparisons made.  mask: bool [N],
    the rows the masked form names (None: the rows around the boundary between members 0 and 1, and the last row)"""
    n, D = v.n_envs, v.obs_dim
    if mask is None:
        mask = np.zeros(n, bool)
        mask[E - 5:E + 7] = True  # straddles the boundary between members 0 and 1
        mask[n - 1] = True
    forms = (dict(), dict(bits=False, tail=False), dict(rows=False), dict(mask=mask))
    count = 0
    for ld in lds:
        out = Act(v, ld)
        got = [out.call(pop, obs, **kw) for kw in forms]
        for r, b, t in got[3:]:
            assert (r[~mask] == CANARY).all() and (b[~mask] == CANARY64).all() and (t[~mask] == CANARY).all(), (what, "unnamed rows")
        for m in range(P):
            pm = make_member(pop.get_member(m))
            lo, hi = m * E, (m + 1) * E
            for kw, g in zip(forms, got):
                w = out.call(pm, obs, **kw)
                for name, x, y in zip(("rows", "bits", "tail"), g, w):
                    assert np.array_equal(x[lo:hi], y[lo:hi]), (what, "ld", ld, "member", m, kw.keys(), name)
                    count += 1
            pm.close()
        # the members differ: member 1's rows are not member 0's weights' rows
        assert not np.array_equal(got[0][0][:E], out.call(make_member(pop.get_member(1)), obs)[0][:E]), (what, "members differ")
        out.free()
    return count


@pytest.mark.parametrize("piles", HUBS, ids=ids_hub)
def test_act_equals_a_plain_policy_per_member_bit_for_bit(piles):
    """hidden width 33 leaves 31 padded outputs per tile whose weights must have stayed zero: noise there would reach the next layer"""
    rs = np.random.RandomState(100 + sum(piles))
    for P, E in SHAPES:
        v = make("philox", piles, P * E)
        obs = rs.normal(size=(P * E, v.obs_dim)).astype(F32)
        for hidden in NETS:
            pol = v.make_policy(gaussian_layers(rs, sizes_of(v, hidden)))
            pop = v.make_population(pol, P, KEY)
            pop.perturb_device(0.3, 11)
            v.sync()
            lds = (v.obs_dim, v.obs_dim + 2) if (P, E) != (6, 32) or hidden == (33,) else (v.obs_dim,)
            assert act_equals_member_policies(v, pop, P, E, obs, v.make_policy, (piles, P, E, hidden), lds) > 0
            pop.close()
            pol.close()
        v.close()


@pytest.mark.parametrize("case", ["pile_obs", "loads"])
def test_act_with_a_feature_block_and_with_the_loads_head(case):
    """a PILE_OBS block behind the observation (F = 13 + 2 x 45 = 103: k_pad 104), and the LOADS head with its dispatch launch, on a handle
    that has been stepped; normalised inputs"""
    rs = np.random.RandomState(7)
    P, E = 6, 32
    v = make("philox", [20, 25], P * E)
    d = Driver(v, "philox")
    d.reset()
    for _ in range(3):
        obs = d.step()[0]
    inputs = ("obs", ("pile_obs", ("car", "soc"))) if case == "pile_obs" else ("obs",)
    head = "piles" if case == "pile_obs" else "loads"
    F = v.obs_dim + (2 * v.n_slots if case == "pile_obs" else 0)
    norm = (rs.normal(size=F).astype(F32), rs.uniform(0.05, 1.0, size=F).astype(F32), 4.0)
    mk = lambda layers: v.make_policy(layers, inputs=inputs, head=head, normalize=norm)
    pol = mk(gaussian_layers(rs, sizes_of(v, (33,), head, F)))
    pop = v.make_population(pol, P, KEY)
    pop.perturb_device(0.2, 2)
    v.sync()
    assert act_equals_member_policies(v, pop, P, E, obs, mk, case, (v.obs_dim, v.obs_dim + 2)) > 0
    pop.close()
    pol.close()
    v.close()


# ---- 3. members by hand
def test_set_get_and_copy_members():
    rs = np.random.RandomState(3)
    mg = buffers()
    P, E = 6, 32
    v = make("philox", [20, 25], P * E)
    sizes = sizes_of(v, (33,))
    shapes = list(zip(sizes[1:], sizes[:-1]))
    centre = gaussian_layers(rs, sizes)
    pol = v.make_policy(centre)
    pop = v.make_population(pol, P, KEY)
    pop.perturb(0.1, 1)
    want = popl.members(centre, 0.1, KEY, 1, P)
    out, src = LayerBuffers(shapes), LayerBuffers(shapes)
    # the host forms and the device forms agree, and round-trip general f32 bits (NaN payloads and denormals included)
    new = gaussian_layers(rs, sizes)
    new[0][0].view(np.uint32)[0, :3] = (0x7FC01234, 0x00000001, 0x80000000)
    for l, (W, b) in enumerate(new):
        pop.set_member(2, l, W, b)
    want[2] = new
    new4 = gaussian_layers(rs, sizes)
    src.put(new4)
    for l in range(len(shapes)):
        pop.set_member_device(4, l, src.W[l].ptr, src.b[l].ptr)
    v.sync()
    want[4] = new4
    for m in range(P):
        assert_members(member_device(v, pop, out, m), want[m], ("set", m))
        assert_members(pop.get_member(m), want[m], ("set, host form", m))
    # copy: sources are read before any destination is written -- a swap, a chain and a fan-out in one call
    idx = mg.DeviceBuffer(64)

    def copy(s, t):
        idx.from_host(np.array(list(s) + list(t), dtype=np.int32))
        v.sync()
        pop.copy_members_device(idx.ptr, idx.ptr + 4 * len(s), len(s))
        v.sync()

    copy([0, 1], [1, 0])
    want[0], want[1] = want[1], want[0]
    for m in range(P):
        assert_members(member_device(v, pop, out, m), want[m], ("swap", m))
    copy([2, 3, 5, 5], [3, 4, 2, 0])  # 2 -> 3 -> 4 reads the old 3; 5 goes to two members; 1 and 5 are not named as destinations
    old = list(want)
    want[3], want[4], want[2], want[0] = old[2], old[3], old[5], old[5]
    for m in range(P):
        assert_members(member_device(v, pop, out, m), want[m], ("chain and fan-out", m))
    copy([0, 7, -1, 1], [5, 1, 2, 6])  # a pair with an index outside 0 .. P - 1 is skipped
    want[5] = want[0]
    for m in range(P):
        assert_members(member_device(v, pop, out, m), want[m], ("out of range pairs", m))
    pop.copy_members_device(idx.ptr, idx.ptr + 16, 0)  # count == 0: nothing
    # the centre is untouched by all of it
    fresh = v.make_population(pol, 2, 1)  # (a new population starts as the centre)
    assert_members(fresh.get_member(1), centre, "the centre's weights")
    fresh.close()
    for x in (out, src, idx):
        x.free()
    pop.close()
    pol.close()
    v.close()


# ---- 4. the closed loop
@pytest.mark.parametrize("mode", ["lockstep", "autoreset"])
def test_run_steps_equals_the_same_calls_one_by_one(mode):
    """a day and 9 steps in one call, then 7 more, against a twin that issues act + step from Python with its own population"""
    rs = np.random.RandomState(29)
    P, E = 6, 32
    n = P * E
    va, vb = make("philox", [20, 25], n, seed=6), make("philox", [20, 25], n, seed=6)
    D = va.obs_dim
    layers = gaussian_layers(rs, sizes_of(va, (64, 33)))
    pa, pb = va.make_policy(layers), vb.make_policy(layers)
    qa, qb = va.make_population(pa, P, KEY), vb.make_population(pb, P, KEY)
    for q in (qa, qb):
        q.perturb(0.3, 5)
    da, db, ob = Dev(va), Dev(vb), Act(vb)
    ka, kb = packed_pair(va), packed_pair(vb)
    if mode == "autoreset":
        va.reset_device(da.obs.ptr)
        vb.reset_device(db.obs.ptr)
    for first, count in ((0, 105), (105, 7)):
        reset_obs = da.obs.ptr if (mode == "lockstep" or first == 0) else 0
        qa.run_steps([b.ptr for b in ka], count, first_step=first, mode=mode, d_reset_obs=reset_obs, d_final_obs=da.final.ptr if mode == "autoreset" else 0)
        closed_loop_by_hand(vb, qb, db, ob, mode, first, count, kb, from_obs=first == 0)
        va.sync()
        vb.sync()
        same_blocks(va, ka, kb, (mode, first))
        same_state(va, vb, (mode, first))
        if mode == "autoreset":
            assert np.array_equal(da.final.to_host(np.uint32, (n, D)), db.final.to_host(np.uint32, (n, D)))
    for x in (qa, qb, pa, pb):
        x.close()
    va.close()
    vb.close()


@pytest.mark.parametrize("rng", ["philox", "philox_curves"])
def test_a_members_block_equals_a_handle_of_its_own(rng):
    """8 steps from a reset: for every member m a second handle of E envs with env_id0 = m E, the same seed and a plain policy holding
    member m's weights reproduces member m's block of both packed blocks bit for bit"""
    rs = np.random.RandomState(31)
    P, E = 6, 32
    n = P * E
    v = make(rng, [20, 25], n, seed=21)
    D = v.obs_dim
    pol = v.make_policy(gaussian_layers(rs, sizes_of(v, (33,))))
    pop = v.make_population(pol, P, KEY)
    pop.perturb(0.4, 8)
    dv, k = Dev(v), packed_pair(v)
    pop.run_steps([b.ptr for b in k], 8, mode="lockstep", d_reset_obs=dv.obs.ptr)
    v.sync()
    big = [b.to_host(np.uint32, (n, D + 2)) for b in k]
    obs0 = dv.obs.to_host(np.uint32, (n, D))
    for m in range(P):
        s = make(rng, [20, 25], E, seed=21, env_id0=m * E)
        ps = s.make_policy(pop.get_member(m))
        ds, ks = Dev(s), packed_pair(s)
        ps.run_steps([b.ptr for b in ks], 8, mode="lockstep", d_reset_obs=ds.obs.ptr)
        s.sync()
        assert np.array_equal(ds.obs.to_host(np.uint32, (E, D)), obs0[m * E:(m + 1) * E]), (rng, m, "the reset's observation")
        for j in range(2):
            assert np.array_equal(ks[j].to_host(np.uint32, (E, D + 2)), big[j][m * E:(m + 1) * E]), (rng, "member", m, "packed block", j)
        ps.close()
        s.close()
    pop.close()
    pol.close()
    v.close()


def test_a_captured_day_follows_a_perturbation_between_replays():
    """reset + 95 population steps and a perturbation (generation 9) recorded once; replayed, the run evaluates the weights in place when it
    starts: the eager perturbation of generation 2 between two replays changes the next replay, and the recorded generation 9 the one
    after -- all equal to a twin making the same calls eagerly"""
    mg = buffers()
    rs = np.random.RandomState(37)
    P, E = 2, 32
    n = P * E
    va, vb = make("philox", [20, 25], n, seed=12), make("philox", [20, 25], n, seed=12)
    D = va.obs_dim
    layers = gaussian_layers(rs, sizes_of(va, (64, 33)))
    pa, pb = va.make_policy(layers), vb.make_policy(layers)
    qa, qb = va.make_population(pa, P, KEY), vb.make_population(pb, P, KEY)
    st = mg.Stream(0)
    da, db, ob = Dev(va, st.ptr), Dev(vb), Act(vb)
    ka, kb = packed_pair(va), packed_pair(vb)
    theta_host = gaussian_layers(rs, sizes_of(va, (64, 33)))
    theta = upload_layers(theta_host)
    d_W, d_b = [w.ptr for w, _ in theta], [b.ptr for _, b in theta]
    for q, s in ((qa, st.ptr), (qb, 0)):
        q.perturb_device(0.2, 1, d_W, d_b, stream=s)
    qa.run_steps([b.ptr for b in ka], 95, mode="lockstep", d_reset_obs=da.obs.ptr, stream=st.ptr)
    closed_loop_by_hand(vb, qb, db, ob, "lockstep", 0, 95, kb)
    st.sync()
    va.graph_begin(st.ptr)
    qa.run_steps([b.ptr for b in ka], 95, mode="lockstep", d_reset_obs=da.obs.ptr, stream=st.ptr)
    qa.perturb_device(0.2, 9, d_W, d_b, stream=st.ptr)
    with pytest.raises(hub().ChubError, match="chub_graph_begin and chub_graph_end"):
        va.make_population(pa, P, KEY)
    with pytest.raises(hub().ChubError, match="chub_graph_begin and chub_graph_end"):
        qa.close()
    with pytest.raises(hub().ChubError, match="chub_graph_begin and chub_graph_end"):
        qa.get_member(0, 0)
    with pytest.raises(hub().ChubError, match="chub_graph_begin and chub_graph_end"):
        qa.set_member(0, 0, *layers[0])
    graph = va.graph_end(st.ptr)
    st.sync()
    same_blocks(va, ka, kb, "nothing ran while recording")
    seen = []
    for replay in range(4):
        if replay == 2:
            qa.perturb_device(0.2, 2, d_W, d_b, stream=st.ptr)
            qb.perturb_device(0.2, 2, d_W, d_b)
        va.graph_launch(graph, st.ptr)
        closed_loop_by_hand(vb, qb, db, ob, "lockstep", 0, 95, kb)
        qb.perturb_device(0.2, 9, d_W, d_b)
        st.sync()
        vb.sync()
        same_blocks(va, ka, kb, ("replay", replay))
        same_state(va, vb, ("replay", replay))
        seen.append(qa.get_member(0, 0)[0].copy())
    assert np.array_equal(u32(seen[0]), u32(seen[3])) and np.array_equal(u32(seen[0]), u32(popl.members(theta_host, 0.2, KEY, 9, P)[0][0][0]))
    va.graph_destroy(graph)
    for x in (qa, qb, pa, pb):
        x.close()
    va.close()
    vb.close()


# ---- 5. the ES gradient
@pytest.mark.parametrize("P", [6, 64, 70])
def test_es_gradient_within_the_bound_and_deterministic(P):
    """general utilities: every element of every gW and gb within population_lib's bound 2^-24 |g| + P 2^-52 sum |du eps| of the f64
    definition; two calls give identical bits; utilities equal within every pair give exactly 0.0f everywhere.  P = 64 splits the pairs
    over two workgroups' chunks, P = 70 over three of unequal length"""
    rs = np.random.RandomState(P)
    mg = buffers()
    v = make("philox", [20, 25], P * 32)
    sizes = sizes_of(v, (33,))
    shapes = list(zip(sizes[1:], sizes[:-1]))
    pol = v.make_policy(gaussian_layers(rs, sizes))
    pop = v.make_population(pol, P, KEY)
    out = LayerBuffers(shapes)
    d_util = mg.DeviceBuffer(P * 4)

    def call(util, g):
        out.fill()
        d_util.from_host(np.ascontiguousarray(util, dtype=F32))
        v.sync()
        pop.es_gradient_device(d_util.ptr, g, *out.ptrs())
        v.sync()
        return [out.read(l) for l in range(len(shapes))]

    for g, util in ((5, rs.normal(size=P).astype(F32)), (0xFFFFFFFE, (rs.normal(size=P) * 1e3 + 50).astype(F32))):
        got = call(util, g)
        want, bound = popl.es_gradient(util, KEY, g, P, shapes)
        for l in range(len(shapes)):
            for name, x, w, bd in zip("Wb", got[l], want[l], bound[l]):
                err = np.abs(x.view(F32).astype(np.float64) - w)
                print("es_gradient P=%d layer %d %s: max error / bound %.3g" % (P, l, name, (err / bd).max()))
                assert (err <= bd).all(), (P, l, name, np.nonzero(err > bd)[0][:5], err.max(), bd.max())
                assert np.abs(w).max() > 0
        again = call(util, g)
        assert all(np.array_equal(a, b) for x, y in zip(got, again) for a, b in zip(x, y)), "the same call twice"
        host = pop.es_gradient(util, g)
        assert all(np.array_equal(u32(a), b) for x, y in zip(host, got) for a, b in zip(x, y)), "the host form"
    pairs = np.repeat(rs.normal(size=P // 2).astype(F32), 2)
    for W, b in call(pairs, 5):
        assert (W == 0).all() and (b == 0).all(), "equal utilities within every pair: +0.0f everywhere"
    for x in (out, d_util):
        x.free()
    pop.close()
    pol.close()
    v.close()


# ---- 6. no trace
def test_population_calls_leave_no_trace_in_the_simulation():
    rs = np.random.RandomState(41)
    mg = buffers()
    P, E = 2, 32
    n = P * E
    va, vb = make("philox", [20, 25], n, seed=8), make("philox", [20, 25], n, seed=8)
    size0 = len(va.get_state())
    sizes = sizes_of(va, (33,), F=va.obs_dim + 2 * va.n_slots)
    shapes = list(zip(sizes[1:], sizes[:-1]))
    pol = va.make_policy(gaussian_layers(rs, sizes), inputs=("obs", ("pile_obs", ("car", "soc"))))
    pop = va.make_population(pol, P, KEY)
    assert len(va.get_state()) == size0 == len(vb.get_state()), "chub_state_size"
    out, grads, d_util, idx = Act(va), LayerBuffers(shapes), mg.DeviceBuffer(P * 4), mg.DeviceBuffer(8)
    d_util.from_host(np.array([1.0, -2.0], dtype=F32))
    idx.from_host(np.array([0, 1], dtype=np.int32))
    obs = va.reset()
    vb.reset()
    acts = np.random.RandomState(5)
    for i in range(20):
        out.put_obs(obs)
        pop.perturb_device(0.1, i)
        pop.act_device(out.obs.ptr, d_actions=out.rows.ptr, d_pile_bits=out.bits.ptr, d_tail=out.tail.ptr)
        pop.es_gradient_device(d_util.ptr, i, *grads.ptrs())
        pop.copy_members_device(idx.ptr, idx.ptr + 4, 1)
        pop.get_member_device(1, 0, grads.W[0].ptr, grads.b[0].ptr)
        pop.set_member_device(0, 0, grads.W[0].ptr, grads.b[0].ptr)
        va.sync()
        if i % 7 == 0:
            pop.set_member(1, 1, *pop.get_member(0, 1))
        a = acts.uniform(-1, 1, size=(n, va.act_dim)).astype(F32)
        obs = va.step(a)[0]
        assert np.array_equal(obs, vb.step(a)[0])
    same_state(va, vb, "after 20 steps")
    assert len(va.get_state()) == size0
    for x in (out, grads, d_util, idx):
        x.free()
    pop.close()
    pol.close()
    va.close()
    vb.close()


# ---- 7. refusals
def test_every_refusal_on_a_device():
    chub = hub()
    rs = np.random.RandomState(43)
    v, other = make("philox", [20, 25], 64), make("philox", [20, 25], 64)
    D, A = v.obs_dim, v.act_dim
    layers = gaussian_layers(rs, [D, 33, A])
    pol, pol_other = v.make_policy(layers), other.make_policy(layers)
    lib = v._lib

    def refused(code, text, rc):
        assert rc == code and text.encode() in lib.chub_last_error(), (rc, lib.chub_last_error())

    h = C.c_void_p()
    refused(-1, "P is even and at least 2", lib.chub_population_create(pol._p, 3, 1, C.byref(h)))
    refused(-1, "P is even and at least 2", lib.chub_population_create(pol._p, 0, 1, C.byref(h)))
    refused(-1, "blocks of a multiple of 32", lib.chub_population_create(pol._p, 4, 1, C.byref(h)))  # E = 16
    refused(-1, "blocks of a multiple of 32", lib.chub_population_create(pol._p, 6, 1, C.byref(h)))  # 64 is no multiple of 6
    assert h.value is None
    v48 = make("philox", [20, 25], 96)
    p48 = v48.make_policy(layers)
    with pytest.raises(chub.ChubError, match="blocks of a multiple of 32"):
        v48.make_population(p48, 2, 1)  # E = 48
    p48.close()
    v48.close()
    with pytest.raises(ValueError):
        v.make_population(pol_other, 2, 1)
    pop = v.make_population(pol, 2, KEY)
    out, dv, src = Act(v), Dev(v), LayerBuffers([(33, D), (A, 33)])
    act = lambda hd, q, obs, ld, rows, bits, tail: lib.chub_population_act_device(hd, q, obs, ld, None, rows, bits, tail, None)
    refused(-1, "made for another handle", act(other._h, pop._q, out.obs.ptr, D, out.rows.ptr, None, None))
    refused(-1, "null argument", act(v._h, pop._q, None, D, out.rows.ptr, None, None))
    refused(-1, "ld_obs", act(v._h, pop._q, out.obs.ptr, D - 1, out.rows.ptr, None, None))
    refused(-1, "give d_actions, d_pile_bits or both", act(v._h, pop._q, out.obs.ptr, D, None, None, out.tail.ptr))
    refused(-1, "pile bits need d_tail", act(v._h, pop._q, out.obs.ptr, D, None, out.bits.ptr, None))
    W, b = src.W[0].ptr, src.b[0].ptr
    for m, l, text in ((-1, 0, "m: 0 .. P - 1"), (2, 0, "m: 0 .. P - 1"), (0, 2, "layer: 0 .. n_layers - 1"), (0, -1, "layer: 0 .. n_layers - 1")):
        refused(-1, text, lib.chub_population_set_member_device(pop._q, m, l, W, b, None))
        refused(-1, text, lib.chub_population_get_member_device(pop._q, m, l, W, b, None))
        refused(-1, text, lib.chub_population_get_member(pop._q, m, l, layers[0][0].ctypes.data, layers[0][1].ctypes.data))
        refused(-1, text, lib.chub_population_set_member(pop._q, m, l, layers[0][0].ctypes.data, layers[0][1].ctypes.data))
    refused(-1, "null argument", lib.chub_population_set_member_device(pop._q, 0, 0, None, b, None))
    refused(-1, "count is 0 .. P", lib.chub_population_copy_members_device(pop._q, W, W, 3, None))
    refused(-1, "count is 0 .. P", lib.chub_population_copy_members_device(pop._q, W, W, -1, None))
    refused(-1, "null argument", lib.chub_population_copy_members_device(pop._q, None, W, 1, None))
    Wp, bp = (C.c_void_p * 2)(*src.ptrs()[0]), (C.c_void_p * 2)(*src.ptrs()[1])
    for sigma in (-0.5, float("nan"), float("inf")):
        refused(-1, "sigma is finite and >= 0", lib.chub_population_perturb_device(pop._q, Wp, bp, sigma, 0, None))
    refused(-1, "both given or both NULL", lib.chub_population_perturb_device(pop._q, Wp, None, 0.1, 0, None))
    half = (C.c_void_p * 2)(src.W[0].ptr, None)
    refused(-1, "null argument", lib.chub_population_perturb_device(pop._q, half, bp, 0.1, 0, None))
    refused(-1, "null argument", lib.chub_population_es_gradient_device(pop._q, None, 0, Wp, bp, None))
    refused(-1, "null argument", lib.chub_population_es_gradient_device(pop._q, W, 0, half, bp, None))
    pair = packed_pair(v)
    blocks = (C.c_void_p * 2)(pair[0].ptr, pair[1].ptr)
    run = lambda hd, q, mode, reset_obs, first, count: lib.chub_population_run_steps(hd, q, mode, blocks, reset_obs, None, first, count, None)
    refused(-1, "made for another handle", run(other._h, pop._q, 0, dv.obs.ptr, 0, 4))
    refused(-1, "mode:", run(v._h, pop._q, 2, dv.obs.ptr, 0, 4))
    refused(-1, "bad argument", run(v._h, pop._q, 0, None, 0, 4))
    refused(-1, "step() before reset()", run(v._h, pop._q, 1, dv.obs.ptr, 0, 4))
    assert v.env_clocks(ticks=True)[1].max() == 0, "nothing ran"
    # the centre policy still evaluates its own weights after a perturbation
    obs = rs.normal(size=(64, D)).astype(F32)
    before = out.call(pol, obs)
    pop.perturb_device(0.5, 3)
    after = out.call(pol, obs)
    assert all(np.array_equal(x, y) for x, y in zip(before, after)), "the centre's outputs"
    assert not np.array_equal(out.call(pop, obs)[0], before[0])
    # COMPAT: the closed loop is refused, single evaluations are not
    c = make("compat", [3, 2], 64)
    pc = c.make_policy(gaussian_layers(rs, [c.obs_dim, c.act_dim]))
    qc = c.make_population(pc, 2, 1)
    pairc, dc, oc = packed_pair(c), Dev(c), Act(c)
    blocks = (C.c_void_p * 2)(pairc[0].ptr, pairc[1].ptr)
    refused(-4, "chub_population_run_steps runs the Philox modes", lib.chub_population_run_steps(c._h, qc._q, 0, blocks, dc.obs.ptr, None, 0, 4, None))
    oc.call(qc, np.zeros((64, c.obs_dim), dtype=F32))
    qc.close()
    pc.close()
    c.close()
    # the tape rules of chub_policy_act_device: a LOADS population on a handle that has become a tape handle
    t = make("philox", [20, 25], 64)
    pt = t.make_policy(gaussian_layers(rs, [D, 4]), head="loads")
    qt = t.make_population(pt, 2, 1)
    t.tape_register_soc(np.array([50.0], dtype=F32))
    ot = Act(t)
    refused(-4, "tape handle", lib.chub_population_act_device(t._h, qt._q, ot.obs.ptr, D, None, ot.rows.ptr, None, None, None))
    qt.close()
    pt.close()
    t.close()
    # destroy order: the policy first (it destroys its populations), then the handle; the Python objects outlive both unharmed
    pol.close()
    pop.close()
    v.close()
    q2 = other.make_population(pol_other, 2, 1)
    other.close()
    q2.close()
    pol_other.close()


# ---- 8. the torch adapter
TORCH_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["CHUB_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHUB_ROOT"], "tests"))
import torch  # before libchub: both must share one HIP runtime
torch.cuda.set_device(0)
import test_gpu_population
test_gpu_population.torch_adapter_population()
print("TORCH_POPULATION_OK")
"""


def test_torch_adapter_population():
    """in a child process that imports torch first (as tests/test_gpu_torch_side.py does)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], env=dict(os.environ, CHUB_ROOT=root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TORCH_POPULATION_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def torch_adapter_population():
    """load_population, population_rollout and es_gradient on P = 2, E = 32 against the numpy host (VecChargingHub + DevicePopulation)"""
    import torch
    from charginghub_env_amd import wrappers
    P, n = 2, 64
    kw = {k: BASE[k] for k in BASE if k != "station_type_list"}
    torch.manual_seed(5)
    env = wrappers.TorchHubVecEnv(n, [20, 25], ["fast", "slow"], seed=13, autoreset="per_env", **kw)
    twin = make("philox", [20, 25], n, seed=13)
    D, A = env.obs_dim, env.act_dim
    net = torch.nn.Sequential(torch.nn.Linear(D, 33), torch.nn.Tanh(), torch.nn.Linear(33, A), torch.nn.Tanh()).to("cuda")
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    layers = [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in lin]
    pol = env.load_policy(net)
    pop = env.load_population(pol, P, KEY)
    pop.perturb_device(0.2, 4, [m.weight.data_ptr() for m in lin], [m.bias.data_ptr() for m in lin], stream=env._stream())
    torch.cuda.synchronize()
    want = popl.members(layers, 0.2, KEY, 4, P)
    for m in range(P):
        assert_members(pop.get_member(m), want[m], ("torch perturb", m))
    # the rollout against the numpy host's population on a twin handle
    pt = twin.make_policy(layers)
    qt = twin.make_population(pt, P, KEY)
    qt.perturb(0.2, 4, layers)
    dt, kt = Dev(twin), packed_pair(twin)
    env.reset()
    twin.reset_device(dt.obs.ptr)
    o, r, d, _ = env.population_rollout(pop, 9)
    qt.run_steps([b.ptr for b in kt], 9, mode="autoreset", d_reset_obs=dt.obs.ptr, d_final_obs=dt.final.ptr)
    twin.sync()
    torch.cuda.synchronize()
    last = kt[8 & 1].to_host(F32, (n, D + 2))
    assert np.array_equal(u32(o.cpu().numpy()), u32(last[:, :D])) and np.array_equal(u32(r.cpu().numpy()), u32(last[:, D]))
    # the gradient against the numpy host's
    util = torch.tensor([0.5, -0.25], dtype=torch.float32, device="cuda")
    grads = env.es_gradient(pop, util, 4)
    torch.cuda.synchronize()
    host = qt.es_gradient(util.cpu().numpy(), 4)
    for (gW, gb), (hW, hb), m in zip(grads, host, lin):
        assert gW.shape == m.weight.shape and gb.shape == m.bias.shape
        assert np.array_equal(u32(gW.cpu().numpy()), u32(hW)) and np.array_equal(u32(gb.cpu().numpy()), u32(hb))
    with pytest.raises(AssertionError):
        env.es_gradient(pop, util.double(), 4)
    qt.close()
    pt.close()
    twin.close()
    pop.close()
    pol.close()
    env.close()
