"""An actor on the device (include/chub.h: chub_policy_*): the feature row through a few dense layers on the f32-input MFMA to action
rows / pile bits + tail, and the closed loop issued from C.  Held here against tests/policy_lib.py's numpy definition: (1) on data whose
every partial sum is exact in f32, bit for bit over N x hub shapes x widths x depths, with canaries and masks; (2) on general data within
the definition's rigorous bound, bits wherever the bound decides them, and determinism; (3) the feature row the policy saw, through a
selection matrix, against the feature calls' own outputs; (4) stepping the rows == stepping the bits, and the LOADS head == the dispatch
by hand; (5) no trace in the simulation; (6) chub_policy_run_steps == the same calls one by one, eager and in a replayed graph, with
weights swapped between replays; (7) per-env rows, 65 536 envs, refusals, the torch adapter.  Shapes are chosen for where tiling goes
wrong (N around the 32-env tile, widths around the 32-output tile, S around the 64-bit word), not for the workload."""
import numpy as np
import pytest

import policy_lib as pl
from charginghub_env_amd import _lib
from test_gpu_autoreset import Dev, buffers
from test_gpu_parity import hub
from test_gpu_pile_obs import BASE, CANARY, MODES, Driver, make

pytestmark = pytest.mark.gpu

F32 = np.float32
EXTRA = 64  # words behind each output that must keep the pattern
CANARY64 = np.uint64(0x7FC0BEEF7FC0BEEF)


class Act(object):
    """device buffers of one chub_policy_act_device call on a handle, pattern-filled before every call"""

    def __init__(self, v, ld=None):
        mg = buffers()
        self.v, self.n, self.D, self.A, self.W = v, v.n_envs, v.obs_dim, v.act_dim, v.bit_words
        self.ld = self.D if ld is None else ld
        n = self.n
        self.obs, self.mask = mg.DeviceBuffer(n * self.ld * 4), mg.DeviceBuffer(n)
        self.rows, self.bits = mg.DeviceBuffer((n * self.A + EXTRA) * 4), mg.DeviceBuffer((n * self.W + EXTRA) * 8)
        self.tail = mg.DeviceBuffer((n * 2 + EXTRA) * 4)

    def put_obs(self, obs):
        block = np.full((self.n, self.ld), np.nan, dtype=F32)  # (what lies between the rows is not the policy's to read)
        block[:, :self.D] = obs
        self.obs.from_host(block)

    def call(self, pol, obs=None, mask=None, rows=True, bits=True, tail=True):
        """-> (rows u32 [N, A], bits u64 [N, W], tail u32 [N, 2]) as the buffers stand after the call; the words behind them are checked"""
        n, A, W = self.n, self.A, self.W
        if obs is not None:
            self.put_obs(obs)
        self.rows.from_host(np.full(n * A + EXTRA, CANARY, dtype=np.uint32))
        self.bits.from_host(np.full(n * W + EXTRA, CANARY64, dtype=np.uint64))
        self.tail.from_host(np.full(n * 2 + EXTRA, CANARY, dtype=np.uint32))
        if mask is not None:
            self.mask.from_host(np.ascontiguousarray(mask, dtype=np.uint8))
        self.v.sync()
        pol.act_device(self.obs.ptr, self.ld, d_actions=self.rows.ptr if rows else 0, d_pile_bits=self.bits.ptr if bits else 0,
                       d_tail=self.tail.ptr if tail else 0, d_mask=self.mask.ptr if mask is not None else 0)
        self.v.sync()
        r, b = self.rows.to_host(np.uint32, (n * A + EXTRA,)), self.bits.to_host(np.uint64, (n * W + EXTRA,))
        t = self.tail.to_host(np.uint32, (n * 2 + EXTRA,))
        assert (r[n * A:] == CANARY).all() and (b[n * W:] == CANARY64).all() and (t[n * 2:] == CANARY).all(), "the words past the outputs"
        return r[:n * A].reshape(n, A), b[:n * W].reshape(n, W), t[:n * 2].reshape(n, 2)

    def free(self):
        for b in (self.obs, self.mask, self.rows, self.bits, self.tail):
            b.free()


def same_state(a, b, label):
    """the simulation state of two handles as every reader shows it, with clocks and ticks (snapshots of two handles are not compared:
    a blob also carries arena bytes no call defines)"""
    ta, tb = a.env_clocks(ticks=True), b.env_clocks(ticks=True)
    assert np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1]), (label, "clocks and ticks")
    for k, (x, y) in enumerate(zip(a.slots() + [a.station_scalars()], b.slots() + [b.station_scalars()])):
        assert np.array_equal(x, y, equal_nan=True), (label, "state array", k)


def f32(words):
    return np.ascontiguousarray(words).view(F32)


def check_exact(got, a, S, what):
    """rows, bits and tail against the definition's outputs a [N, A] (f64, exactly representable)"""
    rows, bits, tail = got
    a32 = a.astype(F32)
    assert np.array_equal(a32.astype(np.float64), a), (what, "the expected values are not f32")
    bad = np.nonzero(f32(rows) != a32)
    assert bad[0].size == 0, (what, "rows: first (env, output)", [int(x[0]) for x in bad], bad[0].size, f32(rows)[bad][:4], a32[bad][:4])
    assert np.array_equal(bits, pl.pile_bits(a32, S)), (what, "bits", np.nonzero(bits != pl.pile_bits(a32, S))[0][:5])
    assert np.array_equal(f32(tail), a32[:, S:S + 2]), (what, "tail")


# ---- 1. exact data, bit for bit
HUBS = ([20, 25], [1, 1], [64, 64], [65, 3])
NETS = [(), (1,), (16,), (33,), (64,), (256,), (33, 256), (256, 64), (16, 1, 33), (64, 64), (256, 256, 256), (64, 33, 16)]


@pytest.mark.parametrize("piles", HUBS, ids=lambda p: "%dx%d" % tuple(p))
def test_exact_data_equals_the_definition_bit_for_bit(piles):
    """dyadic observations in the caller's own buffer, sparse asymmetric weights of +-1/8 and +-2/8, relu and clip: every partial sum is
    exact in f32 (policy_lib.assert_exact), so any summation order gives the definition's bits.  N = 1, 33, 257: less than a tile, a tile
    and one env, eight tiles and one; depths 1 .. 4 over widths 1, 16, 33, 64, 256; the observation rows packed (ld = D) and inside a
    [N, D + 2] block."""
    rs = np.random.RandomState(7)
    for n in (1, 33, 257):
        v = make("philox", piles, n)
        D, A, S = v.obs_dim, v.act_dim, v.n_slots
        for ld in (D, D + 2):
            out = Act(v, ld)
            for k, hidden in enumerate(NETS):
                if (k + (ld == D)) % 2 and n != 33:  # (every net at N = 33 in both strides, half of them at each stride otherwise)
                    continue
                layers = pl.exact_layers(rs, [D] + list(hidden) + [A])
                obs = pl.exact_obs(rs, n, D)
                pl.assert_exact(obs, layers)
                a, _ = pl.forward(obs, layers, "relu", "clip")
                pol = v.make_policy(layers, hidden_act="relu", squash="clip")
                check_exact(out.call(pol, obs), a, S, (piles, n, ld, hidden))
                pol.close()
            out.free()
        v.close()


def test_identity_layer_canaries_and_masks():
    """a single layer that copies observation column n % D to output n returns its input rows; only one output kind is written when only
    one is asked for; with a mask -- empty, full, every third env -- the unnamed rows keep the guard pattern"""
    rs = np.random.RandomState(9)
    n = 70
    v = make("philox", [20, 25], n)
    D, A, S = v.obs_dim, v.act_dim, v.n_slots
    W0 = np.zeros((A, D), dtype=F32)
    W0[np.arange(A), np.arange(A) % D] = 1
    pol = v.make_policy([(W0, np.zeros(A, dtype=F32))], squash="clip")
    obs = (pl.exact_obs(rs, n, D) / F32(2)).astype(F32)  # in [-1, 1]: the clip is the identity
    out = Act(v)
    rows, bits, tail = out.call(pol, obs)
    assert np.array_equal(f32(rows), obs[:, np.arange(A) % D]), "an identity layer returns its input rows"
    check_exact((rows, bits, tail), obs[:, np.arange(A) % D].astype(np.float64), S, "identity")
    r, b, t = out.call(pol, obs, bits=False, tail=False)
    assert np.array_equal(r, rows) and (b == CANARY64).all() and (t == CANARY).all(), "rows alone"
    r, b, t = out.call(pol, obs, rows=False)
    assert (r == CANARY).all() and np.array_equal(b, bits) and np.array_equal(t, tail), "bits and tail alone"
    for name, mask in (("empty", np.zeros(n, bool)), ("full", np.ones(n, bool)), ("every third", np.arange(n) % 3 == 0)):
        r, b, t = out.call(pol, obs, mask=mask)
        assert np.array_equal(r[mask], rows[mask]) and np.array_equal(b[mask], bits[mask]) and np.array_equal(t[mask], tail[mask]), name
        assert (r[~mask] == CANARY).all() and (b[~mask] == CANARY64).all() and (t[~mask] == CANARY).all(), (name, "unnamed rows")
    # normalisation on dyadic data: (x - 1/4) * 2 clipped at 1/2 is exact in f32
    mean, inv_std = np.full(D, 0.25, dtype=F32), np.full(D, 2.0, dtype=F32)
    pn = v.make_policy([(W0, np.zeros(A, dtype=F32))], squash="clip", normalize=(mean, inv_std, 0.5))
    x = pl.normalise(obs, mean, inv_std, 0.5)
    assert (np.abs(x) == 0.5).any() and (np.abs(x) < 0.5).any()
    check_exact(out.call(pn, obs), x[:, np.arange(A) % D].astype(np.float64), S, "normalised")
    pn.close()
    pol.close()
    out.free()
    v.close()


# ---- 2. general data
def gaussian_layers(rs, sizes):
    return [((rs.normal(size=(o, i)) / np.sqrt(i)).astype(F32), (rs.normal(size=o) * 0.1).astype(F32)) for i, o in zip(sizes[:-1], sizes[1:])]


@pytest.mark.parametrize("piles,hidden,head", [([20, 25], (64, 64), "piles"), ([1, 1], (33, 33), "piles"), ([64, 64], (64,), "piles")],
                         ids=["13-64-64-47", "13-33-33-4", "13-64-130"])
def test_general_data_within_the_bound_and_deterministic(piles, hidden, head):
    """real observations after a reset and after 5 steps, Gaussian weights scaled by 1 / sqrt(fan-in), tanh / tanh, normalised by the
    observations' own statistics: every output within policy_lib's bound of the f64 definition, every bit equal wherever |a - threshold|
    exceeds the bound, and at most 1 % of the bits left out.  The same call twice gives identical bits; a handle of 257 envs and one of 33
    give identical rows for identical inputs."""
    rs = np.random.RandomState(13)
    big, small = make("philox", piles, 257), make("philox", piles, 33)
    D, A, S = big.obs_dim, big.act_dim, big.n_slots
    layers = gaussian_layers(rs, [D] + list(hidden) + [A])
    d = Driver(big, "philox")
    moments = [d.reset().copy()]
    for _ in range(5):
        obs = d.step()[0]
    moments.append(obs.copy())
    allobs = np.concatenate(moments)
    mean = allobs.mean(axis=0).astype(F32)
    inv_std = (1.0 / (allobs.std(axis=0) + 1e-3)).astype(F32)
    pb = big.make_policy(layers, normalize=(mean, inv_std, 5.0))
    ps = small.make_policy(layers, normalize=(mean, inv_std, 5.0))
    ob, os_ = Act(big), Act(small, D + 2)
    undecided = total = 0
    for obs in moments:
        x = pl.normalise(obs, mean, inv_std, 5.0)
        a, bound = pl.forward(x, layers)
        rows, bits, tail = ob.call(pb, obs)
        got = f32(rows).astype(np.float64)
        err = np.abs(got - a)
        print("policy %s: max error %.3g, max bound %.3g, worst error / bound %.3g" % (hidden, err.max(), bound.max(), (err / bound).max()))
        assert (err <= bound).all(), ("outputs beyond the bound", np.nonzero(err > bound)[0][:5], err.max(), bound.max())
        sure = pl.decided(a[:, :S], bound[:, :S])
        on = pl.unpack_bits(bits, S)
        assert np.array_equal(on[sure], (a[:, :S] >= float(pl.ON_THRESHOLD))[sure]), "a bit the bound decides"
        assert np.array_equal(bits, pl.pile_bits(f32(rows), S)), "bits are the predicate on the squashed f32 rows; bits from S up are zero"
        assert np.array_equal(tail, rows[:, S:]), "the tail is the row's last two entries"
        undecided += (~sure).sum()
        total += sure.size
        again = ob.call(pb, obs)
        assert all(np.array_equal(p, q) for p, q in zip((rows, bits, tail), again)), "the same call twice"
        few = os_.call(ps, obs[:33])
        assert all(np.array_equal(p[:33], q) for p, q in zip((rows, bits, tail), few)), "N = 257 and N = 33, equal inputs"
    print("policy %s: %d of %d bits left out" % (hidden, undecided, total))
    assert undecided <= 0.01 * total
    for x in (pb, ps):
        x.close()
    for x in (ob, os_):
        x.free()
    big.close()
    small.close()


# ---- 3. the feature row the policy saw
PILE_F, SP_F, FC_F = ("car", "soc", "power"), (("cars", "power"), 3), (("slot", "price", "pv"), 4)
BLOCKS = {"obs": "obs", "pile_obs": ("pile_obs", PILE_F), "station_profile": ("station_profile",) + SP_F, "forecast": ("forecast",) + FC_F}
SCALE = F32(2.0 ** -14)  # an exact scaling that brings every feature into the clip's [-1, 1]


def block_rows(v, name, obs):
    if name == "obs":
        return obs
    if name == "pile_obs":
        return v.pile_obs(PILE_F)
    if name == "station_profile":
        return v.station_profile(*SP_F)
    return v.forecast(*FC_F)


def check_feature_row(v, out, names, obs, what):
    """one layer that selects features, normalised by an exact power of two: output n is feature sel[n] * 2^-14, bit for bit; a few
    selections cover the whole row (the later ones through set_weights)"""
    want = pl.features([block_rows(v, name, obs) for name in names])
    n, F = want.shape
    A = v.act_dim
    assert np.abs(want).max() < 2.0 ** 14 and np.isfinite(want).all()
    pol = None
    for start in range(0, F, A):
        sel = (start + np.arange(A)) % F
        W0 = np.zeros((A, F), dtype=F32)
        W0[np.arange(A), sel] = 1
        if pol is None:
            pol = v.make_policy([(W0, np.zeros(A, dtype=F32))], inputs=[BLOCKS[x] for x in names], squash="clip",
                                normalize=(np.zeros(F, dtype=F32), np.full(F, SCALE), 1.0))
            assert pol.n_features == F
        else:
            pol.set_weights(0, W0, np.zeros(A, dtype=F32))
        rows, _, _ = out.call(pol, obs)
        bad = np.nonzero(rows != (want[:, sel] * SCALE).astype(F32).view(np.uint32))
        assert bad[0].size == 0, (what, names, "first (env, output)", [int(x[0]) for x in bad], "feature", sel[bad[1][:1]])
    pol.close()


@pytest.mark.parametrize("rng", MODES)
def test_input_blocks_carry_the_feature_calls_own_outputs(rng):
    n = 33
    v = make(rng, [20, 25], n)
    d = Driver(v, rng)
    out = Act(v)
    obs = d.reset().copy()
    for moment in range(2):
        for names in (("obs",), ("pile_obs",), ("station_profile",), ("forecast",), ("obs", "pile_obs", "station_profile", "forecast"),
                      ("forecast", "obs")):
            check_feature_row(v, out, names, obs, (rng, "moment", moment))
        for _ in range(3):
            obs = d.step()[0].copy()
    out.free()
    v.close()


def test_input_blocks_on_per_env_clocks_across_a_days_end():
    n = 33
    v = make("philox", [20, 25], n)
    dv = Dev(v)
    rs = np.random.RandomState(4)
    act = lambda: rs.uniform(-1, 1, size=(n, v.act_dim)).astype(F32)
    v.reset()
    for _ in range(40):
        v.step(act())
    v.reset_envs(np.arange(n) % 2 == 0)  # half of the envs start a new day: two clocks from here on
    for _ in range(60):
        packed, _ = dv.autoreset(act())
    t = v.env_clocks()
    assert sorted(set(t.tolist())) == [4, 60], t  # the odd envs have crossed their day's end and were reset on the device
    out = Act(v)
    check_feature_row(v, out, ("obs", "pile_obs", "station_profile", "forecast"), packed[:, :v.obs_dim].copy(), "per-env clocks")
    out.free()
    v.close()


# ---- 4. consistency with the step
def test_stepping_the_rows_equals_stepping_the_bits():
    """twins from one seed, one policy each with the same weights: one steps the policy's action rows, the other its bits and tail; 100
    steps (a reset at step 96), state and outputs identical"""
    n = 33
    rs = np.random.RandomState(21)
    va, vb = make("philox", [20, 25], n, seed=5), make("philox", [20, 25], n, seed=5)
    D, A = va.obs_dim, va.act_dim
    layers = gaussian_layers(rs, [D, 64, 64, A])
    pa, pb = va.make_policy(layers), vb.make_policy(layers)
    da, db = Dev(va), Dev(vb)
    oa, ob = Act(va, D + 2), Act(vb, D + 2)
    for dv, v in ((da, va), (db, vb)):
        v.reset_device(dv.obs.ptr)
    src_a, src_b, ld = da.obs.ptr, db.obs.ptr, D
    ons = 0
    for i in range(100):
        if i == 96:
            for dv, v in ((da, va), (db, vb)):
                v.reset_device(dv.obs.ptr)
            src_a, src_b, ld = da.obs.ptr, db.obs.ptr, D
        pa.act_device(src_a, ld, d_actions=oa.rows.ptr)
        pb.act_device(src_b, ld, d_pile_bits=ob.bits.ptr, d_tail=ob.tail.ptr)
        va.step_device_packed(oa.rows.ptr, da.packed.ptr)
        vb.step_bits_device_packed(ob.bits.ptr, ob.tail.ptr, db.packed.ptr)
        src_a, src_b, ld = da.packed.ptr, db.packed.ptr, D + 2
        if i % 25 == 24 or i in (95, 96):
            va.sync()
            vb.sync()
            ka, kb = da.packed.to_host(F32, (n, D + 2)), db.packed.to_host(F32, (n, D + 2))
            assert np.array_equal(ka.view(np.uint32), kb.view(np.uint32)), ("packed outputs at step", i)
            same_state(va, vb, ("step", i))
            ons += pl.unpack_bits(ob.bits.to_host(np.uint64, (n, vb.bit_words)), vb.n_slots).sum()
    assert 0 < ons < 6 * n * vb.n_slots, "the policy switches some piles on and some off"
    for x in (pa, pb):
        x.close()
    for x in (oa, ob):
        x.free()
    va.close()
    vb.close()


@pytest.mark.parametrize("rng", MODES)
def test_loads_head_equals_the_dispatch_by_hand(rng):
    """head LOADS on exact data: the four outputs are the definition's, bit for bit, so chub_load_dispatch_device called by hand on them
    must give the rows and bits the policy call gave; the tail pair comes out as is"""
    n = 33
    rs = np.random.RandomState(17)
    v = make(rng, [20, 25], n)
    d = Driver(v, rng)
    d.reset()
    for _ in range(3):
        d.step()
    D, A, S = v.obs_dim, v.act_dim, v.n_slots
    layers = pl.exact_layers(rs, [D, 33, 4])
    obs = (pl.exact_obs(rs, n, D) / F32(4)).astype(F32)
    pl.assert_exact(obs, layers)
    four, _ = pl.forward(obs, layers, "relu", "clip")
    four = four.astype(F32)
    assert 0 < (np.abs(four[:, :2]) < 1).sum(), "some loads inside the range"
    pol = v.make_policy(layers, head="loads", hidden_act="relu", squash="clip")
    assert pol.n_outputs == 4
    out = Act(v)
    rows, bits, tail = out.call(pol, obs)
    assert np.array_equal(f32(tail), four[:, 2:]), "the tail pair"
    w_rows, w_bits = v.load_dispatch(four[:, :2], four[:, 2:], units="fraction")
    assert np.array_equal(rows, w_rows.view(np.uint32)) and np.array_equal(bits, w_bits)
    assert np.array_equal(bits, pl.pile_bits(f32(rows), S))
    mask = np.arange(n) % 3 == 0
    r, b, t = out.call(pol, obs, mask=mask)
    assert np.array_equal(r[mask], rows[mask]) and (r[~mask] == CANARY).all() and (b[~mask] == CANARY64).all() and (t[~mask] == CANARY).all()
    r, b, t = out.call(pol, obs, rows=False, tail=False)
    assert (r == CANARY).all() and np.array_equal(b, bits) and (t == CANARY).all(), "bits alone: the tail stays in the policy's own buffer"
    pol.close()
    out.free()
    v.close()


# ---- 5. no trace
def test_the_policy_leaves_no_trace_in_the_simulation():
    """a twin that never calls the policy ends 100 steps in the same state at the same ticks, and the handle's own snapshot after the
    run equals its snapshot after the same run from the same start without the calls; chub_state_size is unchanged"""
    n = 33
    va, vb = make("philox", [20, 25], n, seed=8), make("philox", [20, 25], n, seed=8)
    size0 = len(va.get_state())
    F = va.obs_dim + 3 * va.n_slots + 12 + 12
    layers = gaussian_layers(np.random.RandomState(23), [F, 33, va.act_dim])
    pol = va.make_policy(layers, inputs=[BLOCKS[x] for x in ("obs", "pile_obs", "station_profile", "forecast")])
    assert pol.n_features == F and len(va.get_state()) == size0 == len(vb.get_state())
    out = Act(va)
    obs = va.reset()
    vb.reset()
    start = va.get_state()
    va.set_state(start)  # (both of this handle's runs start from the snapshot: the same host-side path into the first step)

    def run(v, calls, obs):
        rs = np.random.RandomState(5)
        for i in range(100):
            if calls:
                out.put_obs(obs)
                pol.act_device(out.obs.ptr, d_actions=out.rows.ptr, d_pile_bits=out.bits.ptr, d_tail=out.tail.ptr)
                v.sync()  # (the host-pointer step below runs on the handle's own stream)
            obs = v.step(rs.uniform(-1, 1, size=(n, v.act_dim)).astype(F32))[0]
        return obs

    oa, ob = run(va, True, obs), run(vb, False, obs)
    assert np.array_equal(oa, ob)
    same_state(va, vb, "after 100 steps")
    blob_with = va.get_state()
    va.set_state(start)
    assert np.array_equal(run(va, False, obs), oa)
    assert np.array_equal(va.get_state(), blob_with), "snapshot blobs"
    pol.close()
    assert len(va.get_state()) == size0
    out.free()
    va.close()
    vb.close()


# ---- 6. the closed loop
def closed_loop_by_hand(v, pol, dv, out, mode, first, count, packed2, stream=0, from_obs=True):
    """the calls chub_policy_run_steps documents, one by one (from_obs: an auto-reset run's first step acts on the dense observation)"""
    D = v.obs_dim
    for i in range(first, first + count):
        src, ld = packed2[(i - 1) & 1].ptr, D + 2
        if mode == "lockstep":
            if i % 96 == 0:
                v.reset_device(dv.obs.ptr, stream=stream)
                src, ld = dv.obs.ptr, D
            pol.act_device(src, ld, d_pile_bits=out.bits.ptr, d_tail=out.tail.ptr, stream=stream)
            v.step_bits_device_packed(out.bits.ptr, out.tail.ptr, packed2[i & 1].ptr, stream=stream)
        else:
            if i == first and from_obs:
                src, ld = dv.obs.ptr, D
            pol.act_device(src, ld, d_actions=out.rows.ptr, stream=stream)
            v.step_autoreset_device(out.rows.ptr, packed2[i & 1].ptr, dv.final.ptr, stream=stream)


def packed_pair(v):
    mg = buffers()
    pair = [mg.DeviceBuffer(v.n_envs * (v.obs_dim + 2) * 4) for _ in range(2)]
    for b in pair:
        b.from_host(np.full((v.n_envs, v.obs_dim + 2), 7, dtype=F32))
    return pair


def same_blocks(v, pa, pb, what):
    shape = (v.n_envs, v.obs_dim + 2)
    for k in range(2):
        assert np.array_equal(pa[k].to_host(np.uint32, shape), pb[k].to_host(np.uint32, shape)), (what, "packed block", k)


@pytest.mark.parametrize("mode,head", [("lockstep", "piles"), ("autoreset", "piles"), ("lockstep", "loads"), ("autoreset", "loads")])
def test_run_steps_equals_the_same_calls_one_by_one(mode, head):
    """two days plus 5 steps in one call, then 7 more from where it stopped, against a twin that issues the documented calls from Python:
    packed blocks, terminal observations and state identical"""
    n = 33
    rs = np.random.RandomState(29)
    va, vb = make("philox", [20, 25], n, seed=6), make("philox", [20, 25], n, seed=6)
    D = va.obs_dim
    layers = gaussian_layers(rs, [D, 64, 64, va.act_dim if head == "piles" else 4])
    pa, pb = va.make_policy(layers, head=head), vb.make_policy(layers, head=head)
    da, db, ob = Dev(va), Dev(vb), Act(vb)
    ka, kb = packed_pair(va), packed_pair(vb)
    if mode == "autoreset":
        va.reset_device(da.obs.ptr)
        vb.reset_device(db.obs.ptr)
    for first, count in ((0, 197), (197, 7)):
        reset_obs = da.obs.ptr if (mode == "lockstep" or first == 0) else 0
        pa.run_steps([b.ptr for b in ka], count, first_step=first, mode=mode, d_reset_obs=reset_obs, d_final_obs=da.final.ptr if mode == "autoreset" else 0)
        closed_loop_by_hand(vb, pb, db, ob, mode, first, count, kb, from_obs=first == 0)  # (the second run continues from the packed block)
        va.sync()
        vb.sync()
        same_blocks(va, ka, kb, (mode, head, first))
        same_state(va, vb, (mode, head, first))
        if mode == "autoreset":
            assert np.array_equal(da.final.to_host(np.uint32, (n, D)), db.final.to_host(np.uint32, (n, D)))
    assert va.env_clocks().tolist() == [(197 + 7) % 96] * n
    for x in (pa, pb):
        x.close()
    va.close()
    vb.close()


def upload_layers(layers):
    mg = buffers()
    out = []
    for W, b in layers:
        dW, db = mg.DeviceBuffer(W.nbytes), mg.DeviceBuffer(b.nbytes)
        dW.from_host(W)
        db.from_host(b)
        out.append((dW, db))
    return out


def test_a_captured_day_replays_and_follows_set_weights_device():
    """reset + 95 closed-loop steps recorded once (an even number of resets + steps) and replayed 3 times equals an eager twin making the
    same calls; chub_policy_set_weights_device between replays changes the next replay, which equals the eager twin with the new weights"""
    mg = buffers()
    n = 33
    rs = np.random.RandomState(31)
    va, vb = make("philox", [20, 25], n, seed=12), make("philox", [20, 25], n, seed=12)
    D, A = va.obs_dim, va.act_dim
    layers, layers2 = gaussian_layers(rs, [D, 64, 33, A]), gaussian_layers(rs, [D, 64, 33, A])
    pa, pb = va.make_policy(layers), vb.make_policy(layers)
    st = mg.Stream(0)
    da, db, ob = Dev(va, st.ptr), Dev(vb), Act(vb)
    ka, kb = packed_pair(va), packed_pair(vb)
    pa.run_steps([b.ptr for b in ka], 95, mode="lockstep", d_reset_obs=da.obs.ptr, stream=st.ptr)  # (to the clock the capture starts and ends at)
    closed_loop_by_hand(vb, pb, db, ob, "lockstep", 0, 95, kb)
    st.sync()
    va.graph_begin(st.ptr)
    pa.run_steps([b.ptr for b in ka], 95, mode="lockstep", d_reset_obs=da.obs.ptr, stream=st.ptr)
    with pytest.raises(hub().ChubError, match="chub_graph_begin and chub_graph_end"):
        pa.set_weights(0, *layers2[0])
    with pytest.raises(hub().ChubError, match="chub_graph_begin and chub_graph_end"):
        va.make_policy(layers)
    with pytest.raises(hub().ChubError, match="chub_graph_begin and chub_graph_end"):
        pa.close()
    graph = va.graph_end(st.ptr)
    st.sync()
    same_blocks(va, ka, kb, "nothing ran while recording")
    dev2 = upload_layers(layers2)
    for replay in range(4):
        if replay == 3:  # new weights in the trainer's layout, on the replay's stream: the buffers the graph's launches read do not move
            for l, (dW, dbias) in enumerate(dev2):
                pa.set_weights_device(l, dW.ptr, dbias.ptr, stream=st.ptr)
                pb.set_weights(l, *layers2[l])
            before = ka[0].to_host(np.uint32, (n, D + 2), st.ptr)
        va.graph_launch(graph, st.ptr)
        closed_loop_by_hand(vb, pb, db, ob, "lockstep", 0, 95, kb)
        st.sync()
        vb.sync()
        same_blocks(va, ka, kb, ("replay", replay))
        same_state(va, vb, ("replay", replay))
    assert not np.array_equal(before, ka[0].to_host(np.uint32, (n, D + 2)))
    va.graph_destroy(graph)
    for x in (pa, pb):
        x.close()
    va.close()
    vb.close()
    st.destroy()


# ---- 7. other
def test_a_handle_with_per_env_rows():
    n = 40
    rs = np.random.RandomState(37)
    rows = dict(hydro_prod_rate=list(rs.uniform(80, 200, n)), init_soc=list(rs.uniform(0.15, 0.6, n)))
    va, vb = make("philox", [20, 25], n, seed=3, **rows), make("philox", [20, 25], n, seed=3, **rows)
    assert va.has_env_params
    D, A, S = va.obs_dim, va.act_dim, va.n_slots
    layers = pl.exact_layers(rs, [D + S, 33, A])
    pa, pb = [v.make_policy(layers, inputs=("obs", ("pile_obs", ("car",))), hidden_act="relu", squash="clip") for v in (va, vb)]
    out = Act(va)
    va.reset()
    vb.reset()  # (the twins stay on one tick)
    obs = pl.exact_obs(rs, n, D)
    x = pl.features([obs, va.pile_obs(("car",))])
    pl.assert_exact(x, layers)
    check_exact(out.call(pa, obs), pl.forward(x, layers, "relu", "clip")[0], S, "per-env rows")
    da, db, ob = Dev(va), Dev(vb), Act(vb)
    ka, kb = packed_pair(va), packed_pair(vb)
    va.reset_device(da.obs.ptr)
    vb.reset_device(db.obs.ptr)
    pa.run_steps([b.ptr for b in ka], 100, mode="autoreset", d_reset_obs=da.obs.ptr, d_final_obs=da.final.ptr)
    closed_loop_by_hand(vb, pb, db, ob, "autoreset", 0, 100, kb)
    va.sync()
    vb.sync()
    same_blocks(va, ka, kb, "per-env rows")
    same_state(va, vb, "per-env rows")
    for x in (pa, pb):
        x.close()
    va.close()
    vb.close()


def test_65536_envs_once():
    """the exact-data check on a 4096-env sample; a checksum of all bits and rows is compared between two calls"""
    n = 65536
    rs = np.random.RandomState(41)
    v = make("philox", [20, 25], n)
    D, A, S = v.obs_dim, v.act_dim, v.n_slots
    layers = pl.exact_layers(rs, [D, 64, 64, A])
    obs = pl.exact_obs(rs, n, D)
    pl.assert_exact(obs, layers)
    pol = v.make_policy(layers, hidden_act="relu", squash="clip")
    out = Act(v)
    rows, bits, tail = out.call(pol, obs)
    sample = np.sort(rs.choice(n, size=4096, replace=False))
    sample[:3], sample[-3:] = (0, 1, 31), (n - 33, n - 32, n - 1)
    a, _ = pl.forward(obs[sample], layers, "relu", "clip")
    check_exact((rows[sample], bits[sample], tail[sample]), a, S, "65 536 envs")
    again = out.call(pol, obs)
    for p, q in zip((rows, bits, tail), again):
        assert int(p.astype(np.uint64).sum()) == int(q.astype(np.uint64).sum()) and np.array_equal(p, q)
    assert np.array_equal(bits, pl.pile_bits(f32(rows), S))
    pol.close()
    out.free()
    v.close()


def test_every_refusal_on_a_device():
    chub = hub()
    n = 8
    rs = np.random.RandomState(43)
    v, other = make("philox", [20, 25], n), make("philox", [20, 25], n)
    D, A = v.obs_dim, v.act_dim
    layers = gaussian_layers(rs, [D, 16, A])
    pol = v.make_policy(layers)
    out, dv = Act(v), Dev(v)
    lib = v._lib

    def refused(code, text, rc):
        assert rc == code and text.encode() in lib.chub_last_error(), (rc, lib.chub_last_error())

    act = lambda h, p, obs, ld, rows, bits, tail: lib.chub_policy_act_device(h, p, obs, ld, None, rows, bits, tail, None)
    refused(-1, "made for another handle", act(other._h, pol._p, out.obs.ptr, D, out.rows.ptr, None, None))
    refused(-1, "null argument", act(v._h, pol._p, None, D, out.rows.ptr, None, None))
    refused(-1, "ld_obs", act(v._h, pol._p, out.obs.ptr, D - 1, out.rows.ptr, None, None))
    refused(-1, "give d_actions, d_pile_bits or both", act(v._h, pol._p, out.obs.ptr, D, None, None, out.tail.ptr))
    refused(-1, "pile bits need d_tail", act(v._h, pol._p, out.obs.ptr, D, None, out.bits.ptr, None))
    refused(-1, "layer: 0 .. n_layers - 1", lib.chub_policy_set_weights_device(pol._p, 2, out.obs.ptr, out.obs.ptr, None))
    refused(-1, "layer: 0 .. n_layers - 1", lib.chub_policy_set_weights(pol._p, -1, layers[0][0].ctypes.data, layers[0][1].ctypes.data))
    pair = packed_pair(v)
    import ctypes as C
    blocks = (C.c_void_p * 2)(pair[0].ptr, pair[1].ptr)
    run = lambda h, p, mode, reset_obs, first, count: lib.chub_policy_run_steps(h, p, mode, blocks, reset_obs, None, first, count, None)
    refused(-1, "made for another handle", run(other._h, pol._p, 0, dv.obs.ptr, 0, 4))
    refused(-1, "mode:", run(v._h, pol._p, 2, dv.obs.ptr, 0, 4))
    refused(-1, "bad argument", run(v._h, pol._p, 0, None, 0, 4))
    refused(-1, "bad argument", run(v._h, pol._p, 0, dv.obs.ptr, -1, 4))
    refused(-1, "step() before reset()", run(v._h, pol._p, 1, dv.obs.ptr, 0, 4))
    assert v.env_clocks(ticks=True)[1].max() == 0, "nothing ran"
    with pytest.raises(ValueError):
        v.make_policy([(layers[0][0][:, :-1], layers[0][1]), layers[1]])  # (a wrong fan-in is caught where the shapes are known)
    with pytest.raises(chub.ChubError, match="the head's output count"):
        v.make_policy(gaussian_layers(rs, [D, 16, A - 1]))
    with pytest.raises(chub.ChubError, match="rows of LDS"):
        v.make_policy(gaussian_layers(rs, [9 * v.n_slots, 256, A]), inputs=(("pile_obs", None),))
    # COMPAT: the closed loop is refused, single evaluations are not
    c = make("compat", [3, 2], n)
    pc = c.make_policy(gaussian_layers(rs, [c.obs_dim, c.act_dim]))
    pairc = packed_pair(c)
    dc = Dev(c)
    blocks = (C.c_void_p * 2)(pairc[0].ptr, pairc[1].ptr)
    refused(-4, "Philox modes", lib.chub_policy_run_steps(c._h, pc._p, 0, blocks, dc.obs.ptr, None, 0, 4, None))
    assert pc.act(np.zeros((n, c.obs_dim), dtype=F32)).shape == (n, c.act_dim)
    pc.close()
    c.close()
    # a tape handle: feature blocks and the LOADS head are refused as the feature calls are; an observation-only actor works
    t = make("philox", [20, 25], n)
    t.tape_register_soc(np.array([50.0], dtype=F32))
    with pytest.raises(chub.ChubError, match="tape handle"):
        t.make_policy(gaussian_layers(rs, [D + t.n_slots, A]), inputs=("obs", ("pile_obs", ("car",))))
    with pytest.raises(chub.ChubError, match="tape handle"):
        t.make_policy(gaussian_layers(rs, [D, 4]), head="loads")
    pt = t.make_policy(layers)
    assert np.abs(pt.act(np.zeros((n, D), dtype=F32))).max() <= 1
    pt.close()
    t.close()
    # the handle destroys its policies; a policy object outliving it does not touch freed memory
    other.close()
    pol.close()
    v.close()


# ---- the torch adapter
TORCH_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["CHUB_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHUB_ROOT"], "tests"))
import torch  # before libchub: both must share one HIP runtime
torch.cuda.set_device(0)
import test_gpu_policy
test_gpu_policy.torch_adapter_policy()
print("TORCH_POLICY_OK")
"""


def test_torch_adapter_load_policy_and_rollout():
    """in a child process that imports torch first (as tests/test_gpu_torch_side.py does)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], env=dict(os.environ, CHUB_ROOT=root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TORCH_POLICY_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def torch_adapter_policy():
    import torch
    from charginghub_env_amd import wrappers
    n = 64
    kw = {k: BASE[k] for k in BASE if k != "station_type_list"}
    torch.manual_seed(3)
    for autoreset in ("per_env", True):
        envs = [wrappers.TorchHubVecEnv(n, [20, 25], ["fast", "slow"], seed=13, autoreset=autoreset, **kw) for _ in range(2)]
        D, A = envs[0].obs_dim, envs[0].act_dim
        net = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, 33), torch.nn.Tanh(), torch.nn.Linear(33, A),
                                  torch.nn.Tanh()).to("cuda")
        pols = [e.load_policy(net) for e in envs]
        assert pols[0].n_features == D and pols[0].n_outputs == A and pols[0].spec.n_layers == 3
        # the device actor against torch's own forward pass: the same f32 network up to summation order and tanh
        obs = envs[0].reset()
        envs[1].reset()
        rows = torch.empty((n, A), dtype=torch.float32, device="cuda")
        pols[0].act_device(obs.data_ptr(), d_actions=rows.data_ptr(), stream=envs[0]._stream())
        with torch.no_grad():
            want = net(obs)
        assert float((rows - want).abs().max()) < 1e-5
        # rollout() == the same closed loop through step(): act_device on the current observation, then the adapter's own step
        for count in (5, 100, 3):
            o, r, d, _ = envs[0].rollout(pols[0], count)
            for _ in range(count):
                cur = envs[1]._cur_obs
                pols[1].act_device(cur.data_ptr(), cur.stride(0), d_actions=rows.data_ptr(), stream=envs[1]._stream())
                o2, r2, d2, _ = envs[1].step(rows)
            assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2), (autoreset, count)
            if autoreset == "per_env":
                assert torch.equal(envs[0].last_obs, envs[1].last_obs)
        # new weights from the trainer's own tensors
        with torch.no_grad():
            for p in net.parameters():
                p.add_(0.05 * torch.randn_like(p))
        lin = [m for m in net if isinstance(m, torch.nn.Linear)]
        for l, m in enumerate(lin):
            pols[0].set_weights_device(l, m.weight.data_ptr(), m.bias.data_ptr(), stream=envs[0]._stream())
        cur = envs[0]._cur_obs
        pols[0].act_device(cur.data_ptr(), cur.stride(0), d_actions=rows.data_ptr(), stream=envs[0]._stream())
        with torch.no_grad():
            want = net(cur)
        assert float((rows - want).abs().max()) < 1e-5
        for e in envs:
            e.close()
    off = wrappers.TorchHubVecEnv(8, [20, 25], ["fast", "slow"], seed=1, autoreset=False)
    with pytest.raises(RuntimeError):
        off.rollout(None, 4)
    with pytest.raises(ValueError):
        off.load_policy(torch.nn.Sequential(torch.nn.Linear(13, 47), torch.nn.ReLU()))
    with pytest.raises(ValueError):
        off.load_policy(torch.nn.Sequential(torch.nn.Linear(13, 8), torch.nn.Sigmoid(), torch.nn.Linear(8, 47)))
    station = wrappers.TorchHubVecEnv(8, [20, 25], ["fast", "slow"], seed=1, control="station")
    assert station.load_policy([(torch.zeros(4, 13), torch.zeros(4))]).n_outputs == 4
    off.close()
    station.close()
