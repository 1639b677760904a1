"""Running feature statistics on the device and the policy's normaliser (include/chub.h: chub_moments_*, chub_policy_*normalizer*), held
against tests/normalizer_lib.py's definition, whose batch sums are exact: (1) a grid of F x ld x R x mask, every update from zeros and a
second one onto the state the first left, within the worst case of f64 summation; (2) constant columns, a column of 10^6 +- 10^-1,
determinism, masked-out NaNs, get / set / reset; (3) from_moments bit for bit; (4) through the policy against tests/policy_lib.py; (5) a
captured graph that follows an in-stream normaliser and holds an update + from_moments itself; (6) the torch adapter; (7) refusals.
Shapes are the smallest at which the launch shape changes: F around the 64-lane wave and the 256-lane workgroup, rows around a workgroup's
pass and beyond one pass of the whole grid."""
import ctypes as C

import numpy as np
import pytest

import normalizer_lib as nl
import policy_lib as pl
from test_gpu_autoreset import Dev, buffers
from test_gpu_parity import hub
from test_gpu_pile_obs import BASE, Driver, make
from test_gpu_policy import Act, closed_loop_by_hand, f32, gaussian_layers, packed_pair, same_blocks, same_state

pytestmark = pytest.mark.gpu

F32 = np.float32
N = 70
PILES = [3, 2]


def bits64(state):
    n, mean, m2 = state
    return np.concatenate([[n], mean, m2]).astype(np.float64).view(np.uint64)


def put(x, ld):
    """x [R, F] -> a device block of rows with stride ld floats; what lies between the rows is NaN (not the kernel's to read)"""
    R, F = x.shape
    block = np.full((R, ld), np.nan, dtype=F32)
    block[:, :F] = x
    buf = buffers().DeviceBuffer(block.nbytes)
    buf.from_host(block)
    return buf


def held(got, ref, R, S2, dmax, what):
    """the device's state against the definition's: the count exact, mean and M2 within the worst case of adding R terms in f64"""
    b_mean, b_m2 = nl.bounds(R, ref, S2, dmax)
    e1, e2 = np.abs(got[1] - ref[1]), np.abs(got[2] - ref[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        w1, w2 = np.nanmax(np.where(b_mean > 0, e1 / b_mean, 0)), np.nanmax(np.where(b_m2 > 0, e2 / b_m2, 0))
    print("moments %s: worst error / bound: mean %.3g, M2 %.3g" % (what, w1, w2))
    assert got[0] == ref[0], (what, "count", got[0], ref[0])
    assert (e1 <= b_mean).all(), (what, "mean", np.nonzero(e1 > b_mean)[0][:5], e1.max(), b_mean.max())
    assert (e2 <= b_m2).all(), (what, "M2", np.nonzero(e2 > b_m2)[0][:5], e2.max(), b_m2.max())


def launch_shape(v, F):
    """(rows per workgroup pass, workgroups at most) the library chooses for F on this device: 256 lanes along min(F, 256) columns, four
    workgroups per compute unit, capped so the partials stay within 4 MiB"""
    info = (C.c_int32 * 4)()
    assert v._lib.chub_device_info(0, info) == 0
    return 256 // min(F, 256), min(4 * info[3], (4 << 20) // (8 * (1 + 2 * F)))


def columns(rs, R, F):
    """features whose scales span 10^5 and whose offsets are of the order of their spread"""
    return ((rs.normal(size=(R, F)) + rs.uniform(-2, 2, size=F)) * np.logspace(-2, 3, F)).astype(F32)


# ---- 1. the shape grid
@pytest.mark.parametrize("F", [1, 13, 23, 63, 64, 65, 512])
def test_every_shape_from_zeros_and_onto_a_state(F):
    """F on both sides of a wave and of the workgroup (two columns per lane at 512, several rows per pass below 129); rows packed and with
    two floats between them; R = 1, 70, 257 and a multiple of N beyond one pass of the whole grid; masks none / random / nobody / everybody
    at R = 70, none / random beyond the grid.  Every case runs two updates on different data: from zeros (pivot = row 0) and onto the state
    the first left (pivot = its mean), each held to the definition applied to the state the device started from."""
    rs = np.random.RandomState(100 + F)
    v = make("philox", PILES, N)
    m = v.make_moments(F)
    rw, grid = launch_shape(v, F)
    big = -(-(grid * rw + 257) // N) * N
    assert big > grid * rw
    mask_buf = buffers().DeviceBuffer(N)
    rand = rs.uniform(size=N) < 0.6
    rand[:2] = (False, True)  # (row 0, the pivot of an empty state, belongs to a masked-out env)
    cases = [(1, None), (257, None), (big, None), (big, rand), (N, None), (N, rand), (N, np.zeros(N, bool)), (N, np.ones(N, bool))]
    for ld in (F, F + 2):
        for R, mask in cases:
            rows = None if mask is None else nl.env_rows(mask, R)
            if mask is not None:
                mask_buf.from_host(mask.astype(np.uint8))
            m.reset_device()
            state = m.get_raw()
            assert state[0] == 0 and not bits64(state).any()
            for k in range(2):
                x = columns(rs, R, F)
                buf = put(x, ld)
                m.update_device(buf.ptr, R, ld=ld, d_mask=mask_buf.ptr if mask is not None else 0)
                got = m.get_raw()
                buf.free()
                ref, _, n_b, S2, dmax = nl.update(state, x, rows)
                what = (F, ld, R, "no mask" if mask is None else int(mask.sum()), k)
                if n_b == 0:
                    assert np.array_equal(bits64(got), bits64(state)), (what, "nobody counted: the state is left alone")
                else:
                    held(got, ref, R, S2, dmax, what)
                state = got
    mask_buf.free()
    m.close()
    v.close()


# ---- 2. accumulation, constants, determinism, masks, checkpoints
def test_accumulation_constant_columns_and_a_large_offset():
    """three updates in a row, the second and third under a mask: a constant column keeps M2 == 0 and its value as the mean EXACTLY, a column
    of 10^6 +- 10^-1 is held like any other (its deviations from the pivot are of the order of 10^-1: no cancellation of a raw sum of
    squares), and an all-zero mask between them changes no bit"""
    rs = np.random.RandomState(7)
    v = make("philox", PILES, N)
    F, R = 6, 4 * N
    m = v.make_moments(F)
    mask_buf = buffers().DeviceBuffer(N)
    state = m.get_raw()
    for k in range(3):
        x = columns(rs, R, F)
        x[:, 1] = F32(1234.5678)
        x[:, 2] = (1e6 + 0.1 * rs.normal(size=R)).astype(F32)
        x[:, 4] = 0
        mask = None if k == 0 else rs.uniform(size=N) < 0.5
        buf = put(x, F)
        if mask is not None:
            mask_buf.from_host(np.zeros(N, dtype=np.uint8))
            m.update_device(buf.ptr, R, d_mask=mask_buf.ptr)
            assert np.array_equal(bits64(m.get_raw()), bits64(state)), "an all-zero mask writes nothing"
            mask_buf.from_host(mask.astype(np.uint8))
        m.update_device(buf.ptr, R, d_mask=mask_buf.ptr if mask is not None else 0)
        got = m.get_raw()
        ref, _, n_b, S2, dmax = nl.update(state, x, None if mask is None else nl.env_rows(mask, R))
        held(got, ref, R, S2, dmax, ("accumulation", k))
        assert got[2][1] == 0.0 and got[2][4] == 0.0 and got[1][1] == np.float64(F32(1234.5678)) and got[1][4] == 0.0, "constant columns"
        assert got[2][2] > 0 and abs(got[1][2] - 1e6) < 0.1 and 0.05 ** 2 < got[2][2] / got[0] < 0.2 ** 2, "the column of 1e6 +- 1e-1"
        n, mean, var = m.get()
        assert n == got[0] and np.array_equal(mean, got[1]) and np.array_equal(var, got[2] / got[0])
        state = got
        buf.free()
    mask_buf.free()
    m.close()
    v.close()


def test_determinism_masked_out_nans_and_the_state_round_trip():
    rs = np.random.RandomState(11)
    v = make("philox", PILES, N)
    mg = buffers()
    for F in (13, 65, 512):
        rw, grid = launch_shape(v, F)
        R = -(-(grid * rw + 99) // N) * N
        m = v.make_moments(F)
        x = columns(rs, R, F)
        mask = rs.uniform(size=N) < 0.5
        mask[0] = True  # (row 0 is the pivot of an empty state whether it counts or not: it stays finite)
        rows = nl.env_rows(mask, R)
        x_nan = x.copy()
        x_nan[~rows] = np.nan
        buf, buf_nan, mask_buf = put(x, F), put(x_nan, F), mg.DeviceBuffer(N)
        mask_buf.from_host(mask.astype(np.uint8))
        start = (5.0, x[:5].astype(np.float64).mean(axis=0), np.abs(rs.normal(size=F)))
        for state in (nl.zero_state(F), start):
            seen = []
            for src in (buf, buf, buf_nan):
                m.set(state[0], state[1], m2=state[2])
                m.update_device(src.ptr, R, d_mask=mask_buf.ptr)
                seen.append(bits64(m.get_raw()))
            assert np.array_equal(seen[0], seen[1]), (F, "two calls from the same state: identical bits")
            assert np.array_equal(seen[0], seen[2]), (F, "masked-out rows filled with NaN change nothing")
            assert np.isfinite(seen[0].view(np.float64)).all() and seen[0].view(np.float64)[0] == state[0] + rows.sum()
        # without the mask the NaNs arrive: a non-finite state, nothing checked on the device
        m.reset_device()
        m.update_device(buf_nan.ptr, R)
        got = m.get_raw()
        assert got[0] == R and np.isnan(got[1]).all() and np.isnan(got[2]).all()
        # get / set: identical bits, odd ones included; the device's own copy of the state is what get reads; reset zeroes it
        odd = (3.0, rs.normal(size=F) * 1e-310, np.abs(rs.normal(size=F)) * 1e300)
        odd[1][0], odd[2][0] = -0.0, np.inf
        m.set(odd[0], odd[1], m2=odd[2])
        assert np.array_equal(bits64(m.get_raw()), bits64(odd))
        raw = np.zeros(1 + 2 * F, dtype=np.float64)
        assert v._lib.chub_copy_to_host(0, raw.ctypes.data_as(C.c_void_p), C.c_void_p(m.state_ptr), raw.nbytes, None) == 0
        assert np.array_equal(raw.view(np.uint64), bits64(odd))
        m.set(4.0, np.arange(F), var=np.full(F, 0.5))
        assert np.array_equal(m.get_raw()[2], np.full(F, 2.0)) and m.get()[2][0] == 0.5
        m.reset_device()
        assert not bits64(m.get_raw()).any() and m.get()[0] == 0 and not m.get()[2].any()
        for b in (buf, buf_nan, mask_buf):
            b.free()
        m.close()
    v.close()


# ---- 3. the normaliser from the moments
def test_from_moments_is_the_definition_bit_for_bit():
    """the library is built without fast-math and the kernel uses the correctly rounded f64 division and square root: mean32 and inv_std32
    are numpy's f64 results narrowed once, bit for bit -- over states the update kernel left (a constant column: inv_std = 1 / sqrt(eps))
    and states set by hand with M2 across 10^-60 .. 10^60 (inv_std stays a normal f32).  Moments that counted nothing leave the normaliser's
    bits alone."""
    rs = np.random.RandomState(13)
    v = make("philox", PILES, N)
    D, A = v.obs_dim, v.act_dim
    layers = gaussian_layers(rs, [D, 32, A])
    canary = (rs.normal(size=D).astype(F32), np.abs(rs.normal(size=D)).astype(F32))
    pol = v.make_policy(layers, normalize=canary + (5.0,))
    m = v.make_moments(D)
    got = pol.normalizer()
    assert np.array_equal(got[0].view(np.uint32), canary[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), canary[1].view(np.uint32))
    pol.normalizer_from_moments(m)  # n == 0
    got = pol.normalizer()
    assert np.array_equal(got[0].view(np.uint32), canary[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), canary[1].view(np.uint32))
    x = columns(rs, 257, D)
    x[:, 3] = F32(0.3)
    buf = put(x, D)
    m.update_device(buf.ptr, 257)
    states = [None, None, (7.0, rs.normal(size=D) * 1e3, 10.0 ** rs.uniform(-60, 60, size=D)), (1.0, rs.normal(size=D), np.zeros(D))]
    for k, (state, eps) in enumerate(zip(states, (1e-8, 1e-2, 1e-8, 0.37))):
        if state is not None:
            m.set(state[0], state[1], m2=state[2])
        state = m.get_raw()
        pol.normalizer_from_moments(m, eps=eps)
        mean32, inv32 = pol.normalizer()
        want = nl.from_moments(state, eps)
        assert np.array_equal(mean32.view(np.uint32), want[0].view(np.uint32)), (k, "mean32")
        assert np.array_equal(inv32.view(np.uint32), want[1].view(np.uint32)), (k, "inv_std32", np.nonzero(inv32 != want[1])[0][:5])
        if k < 2:
            assert inv32[3] == F32(1.0 / np.sqrt(eps)) and mean32[3] == F32(0.3)
    buf.free()
    m.close()
    pol.close()
    v.close()


# ---- 4. through the policy
PILE_F = ("car", "soc", "power")


def test_the_policy_evaluates_the_normaliser_it_was_given():
    """obs + pile_obs through one hidden layer of 32: after from_moments and after set_normalizer_device the action rows are
    tests/policy_lib.py's definition on the features normalised with the normaliser READ BACK, within the definition's bound (the
    comparison tests/test_gpu_policy.py makes on general data); get_normalizer_device returns what was set; the sampled call's features
    stay the raw rows whatever the normaliser is"""
    mg = buffers()
    rs = np.random.RandomState(17)
    v = make("philox", PILES, N)
    D, A, S = v.obs_dim, v.act_dim, v.n_slots
    F = D + len(PILE_F) * S
    layers = gaussian_layers(rs, [F, 32, A])
    clip = 5.0
    pol = v.make_policy(layers, inputs=("obs", ("pile_obs", PILE_F)), normalize=(np.zeros(F, dtype=F32), np.ones(F, dtype=F32), clip))
    assert pol.n_features == F
    pol.set_exploration(5, [-0.5, 0.1])
    d = Driver(v, "philox")
    d.reset()
    for _ in range(7):
        obs = d.step()[0]
    raw = pl.features([obs, v.pile_obs(PILE_F)])
    out, feat, logp = Act(v), mg.DeviceBuffer(N * F * 4), mg.DeviceBuffer(N * 4)
    out.put_obs(obs)
    m = v.make_moments(F)

    def features_now():
        feat.from_host(np.full((N, F), np.nan, dtype=F32))
        pol.sample_device(out.obs.ptr, d_logp=logp.ptr, d_features=feat.ptr)
        v.sync()
        return feat.to_host(F32, (N, F))

    def evaluated(what):
        mean, inv_std = pol.normalizer()
        a, bound = pl.forward(pl.normalise(raw, mean, inv_std, clip), layers)
        rows, bits, tail = out.call(pol, obs)
        err = np.abs(f32(rows).astype(np.float64) - a)
        print("normalised policy, %s: max error %.3g, worst error / bound %.3g" % (what, err.max(), (err / bound).max()))
        assert (err <= bound).all(), (what, err.max(), bound.max())
        assert np.array_equal(bits, pl.pile_bits(f32(rows), S)) and np.array_equal(tail, rows[:, S:])
        return f32(rows).copy()

    assert np.array_equal(features_now().view(np.uint32), raw.view(np.uint32)), "the feature row is obs | pile_obs, raw"
    a0 = evaluated("as created")
    m.update_device(feat.ptr, N)
    pol.normalizer_from_moments(m, eps=1e-4)
    want = nl.from_moments(m.get_raw(), 1e-4)
    got = pol.normalizer()
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    ref = nl.update(nl.zero_state(F), raw)
    held(m.get_raw(), ref[0], N, ref[3], ref[4], "the policy's own feature rows")
    a1 = evaluated("from moments")
    assert not np.array_equal(a0, a1)
    assert np.array_equal(features_now().view(np.uint32), raw.view(np.uint32)), "features stay raw under the new normaliser"
    mean = (raw.mean(axis=0) + rs.normal(size=F)).astype(F32)
    inv_std = (1.0 / (raw.std(axis=0) + 0.1)).astype(F32)
    pair = mg.DeviceBuffer(2 * F * 4)
    pair.from_host(np.stack([mean, inv_std]))
    pol.set_normalizer_device(pair.ptr, pair.ptr + 4 * F)
    back = mg.DeviceBuffer(2 * F * 4)
    pol.get_normalizer_device(back.ptr + 4 * F, back.ptr)  # (the two outputs are separate buffers: swapped here)
    v.sync()
    got = back.to_host(np.uint32, (2, F))
    assert np.array_equal(got[1], mean.view(np.uint32)) and np.array_equal(got[0], inv_std.view(np.uint32)), "get returns what was set"
    a2 = evaluated("set on the device")
    pol.set_normalizer(mean + F32(1), inv_std)
    got = pol.normalizer()
    assert np.array_equal(got[0], mean + F32(1)) and np.array_equal(got[1], inv_std)
    a3 = evaluated("set from the host")
    assert not np.array_equal(a1, a2) and not np.array_equal(a2, a3)
    assert np.array_equal(features_now().view(np.uint32), raw.view(np.uint32))
    for b in (feat, logp, pair, back):
        b.free()
    out.free()
    m.close()
    pol.close()
    v.close()


# ---- 5. graphs
def test_a_captured_day_follows_the_normaliser_and_holds_an_update_itself():
    """test_gpu_policy's captured day (reset + 95 closed-loop steps, an even number of resets + steps, replayed from the clock it was
    recorded at) with a normalised actor: chub_policy_set_normalizer_device on the replay's stream changes the next replay, which equals an
    eager twin whose normaliser was set from the host.  Then a second graph that holds, in front of the day, a moments update over the
    observations of the last packed block (ld = D + 2) and from_moments: every replay equals the twin making the same calls one by one,
    the moments' state included, bit for bit.  What allocates or synchronises is refused while recording."""
    mg = buffers()
    n = 33
    rs = np.random.RandomState(31)
    va, vb = make("philox", [20, 25], n, seed=12), make("philox", [20, 25], n, seed=12)
    D, A = va.obs_dim, va.act_dim
    layers = gaussian_layers(rs, [D, 32, A])
    norm0 = (rs.normal(size=D).astype(F32), (1.0 / (1.0 + 100 * np.abs(rs.normal(size=D)))).astype(F32), 5.0)
    norm1 = (rs.normal(size=D).astype(F32) * 50, (1.0 / (1.0 + 10 * np.abs(rs.normal(size=D)))).astype(F32))
    pa, pb = va.make_policy(layers, normalize=norm0), vb.make_policy(layers, normalize=norm0)
    ma, mb = va.make_moments(D), vb.make_moments(D)
    st = mg.Stream(0)
    da, db, ob = Dev(va, st.ptr), Dev(vb), Act(vb)
    ka, kb = packed_pair(va), packed_pair(vb)
    pa.run_steps([b.ptr for b in ka], 95, mode="lockstep", d_reset_obs=da.obs.ptr, stream=st.ptr)  # (to the clock the captures start and end at)
    closed_loop_by_hand(vb, pb, db, ob, "lockstep", 0, 95, kb)
    st.sync()
    va.graph_begin(st.ptr)
    pa.run_steps([b.ptr for b in ka], 95, mode="lockstep", d_reset_obs=da.obs.ptr, stream=st.ptr)
    for refused in (lambda: pa.set_normalizer(*norm1), lambda: va.make_moments(D), lambda: ma.get_raw(), lambda: ma.set(0.0, np.zeros(D), m2=np.zeros(D)),
                    lambda: ma.close()):
        with pytest.raises(hub().ChubError, match="chub_graph_begin and chub_graph_end"):
            refused()
    graph = va.graph_end(st.ptr)
    st.sync()
    pair = mg.DeviceBuffer(2 * D * 4)
    pair.from_host(np.stack(norm1))
    for replay in range(3):
        if replay == 2:  # a new normaliser on the replay's stream: the buffer the graph's launches read does not move
            pa.set_normalizer_device(pair.ptr, pair.ptr + 4 * D, stream=st.ptr)
            pb.set_normalizer(*norm1)
            before = ka[0].to_host(np.uint32, (n, D + 2), st.ptr)
        va.graph_launch(graph, st.ptr)
        closed_loop_by_hand(vb, pb, db, ob, "lockstep", 0, 95, kb)
        st.sync()
        vb.sync()
        same_blocks(va, ka, kb, ("replay", replay))
        same_state(va, vb, ("replay", replay))
    assert not np.array_equal(before, ka[0].to_host(np.uint32, (n, D + 2))), "the new normaliser acts differently"
    va.graph_destroy(graph)
    # the update and from_moments inside the graph (the run's last step, 94, wrote block 0)
    va.graph_begin(st.ptr)
    ma.update_device(ka[0].ptr, n, ld=D + 2, stream=st.ptr)
    pa.normalizer_from_moments(ma, eps=1e-4, stream=st.ptr)
    pa.run_steps([b.ptr for b in ka], 95, mode="lockstep", d_reset_obs=da.obs.ptr, stream=st.ptr)
    graph = va.graph_end(st.ptr)
    st.sync()
    assert ma.get_raw()[0] == 0, "nothing ran while recording"
    for replay in range(3):
        va.graph_launch(graph, st.ptr)
        mb.update_device(kb[0].ptr, n, ld=D + 2)
        pb.normalizer_from_moments(mb, eps=1e-4)
        closed_loop_by_hand(vb, pb, db, ob, "lockstep", 0, 95, kb)
        st.sync()
        vb.sync()
        same_blocks(va, ka, kb, ("update in the graph", replay))
        same_state(va, vb, ("update in the graph", replay))
        sa, sb = ma.get_raw(), mb.get_raw()
        assert sa[0] == n * (replay + 1) and np.array_equal(bits64(sa), bits64(sb)), ("the moments", replay)
        na, nb = pa.normalizer(), pb.normalizer()
        want = nl.from_moments(sa, 1e-4)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(na + na, nb + want)), ("the normaliser", replay)
    va.graph_destroy(graph)
    pair.free()
    for x in (ma, mb, pa, pb):
        x.close()
    va.close()
    vb.close()
    st.destroy()


# ---- 6. the torch adapter
TORCH_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["CHUB_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHUB_ROOT"], "tests"))
import torch  # before libchub: both must share one HIP runtime
torch.cuda.set_device(0)
import test_gpu_normalizer
test_gpu_normalizer.torch_adapter_update_normalizer()
print("TORCH_NORMALIZER_OK")
"""


def test_torch_adapter_update_normalizer():
    """in a child process that imports torch first (as tests/test_gpu_torch_side.py does)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], env=dict(os.environ, CHUB_ROOT=root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TORCH_NORMALIZER_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def torch_adapter_update_normalizer():
    import torch
    from charginghub_env_amd import wrappers
    T, clip = 4, 5.0
    kw = {k: BASE[k] for k in BASE if k != "station_type_list"}
    torch.manual_seed(3)
    rs = np.random.RandomState(3)
    for autoreset in ("per_env", True):
        env = wrappers.TorchHubVecEnv(N, PILES, ["fast", "slow"], seed=13, autoreset=autoreset, **kw)
        D, A, S = env.obs_dim, env.act_dim, env.vec.n_slots
        F = D + len(PILE_F) * S
        net = torch.nn.Sequential(torch.nn.Linear(F, 32), torch.nn.Tanh(), torch.nn.Linear(32, A)).to("cuda")
        first = (rs.normal(size=F).astype(F32), (1.0 / (1.0 + 30 * np.abs(rs.normal(size=F)))).astype(F32))
        pol = env.load_policy(net, inputs=("obs", ("pile_obs", PILE_F)), normalize=first + (clip,))
        log_std = torch.tensor([-0.5, 0.1], device="cuda")
        pol.set_exploration(21, log_std.cpu().numpy())
        env.reset()
        old = env.policy_normalizer(pol)
        assert all(t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (F,) for t in old)
        assert np.array_equal(old[0].cpu().numpy(), first[0]) and np.array_equal(old[1].cpu().numpy(), first[1])
        ro = env.collect(pol, T)
        m = env.update_normalizer(pol, ro, eps=1e-4)
        # the state is the definition on the rollout's raw features, and the policy's normaliser is derived from it
        feats = ro["features"].cpu().numpy().reshape(T * N, F)
        ref = nl.update(nl.zero_state(F), feats)
        state = m.get_raw()
        held(state, ref[0], T * N, ref[3], ref[4], ("update_normalizer", autoreset))
        new = env.policy_normalizer(pol)
        want = nl.from_moments(state, 1e-4)
        assert np.array_equal(new[0].cpu().numpy().view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(new[1].cpu().numpy().view(np.uint32), want[1].view(np.uint32))
        # the recorded logp belongs to the OLD normaliser: the trainer's forward pass on the features normalised with it reproduces it
        with torch.no_grad():
            z = net(wrappers.normalize_features(ro["features"], old[0], old[1], clip))
            z_new = net(wrappers.normalize_features(ro["features"], new[0], new[1], clip))
        rec = ro["logp"].double()
        ratio = torch.exp(wrappers.sampled_logp(z, ro["bits"], ro["u"], log_std).double() - rec)
        assert float((ratio - 1).abs().max()) < 1e-4, "an importance ratio of 1 under the normaliser the rollout was recorded with"
        off = torch.exp(wrappers.sampled_logp(z_new, ro["bits"], ro["u"], log_std).double() - rec)
        assert float((off - 1).abs().max()) > 1e-2, "the new normaliser is another policy"
        # the next rollout is recorded under the new one; the adapter keeps one moments object per policy, and a mask counts its envs only
        ro = env.collect(pol, T)
        with torch.no_grad():
            z = net(wrappers.normalize_features(ro["features"], new[0], new[1], clip))
        ratio = torch.exp(wrappers.sampled_logp(z, ro["bits"], ro["u"], log_std).double() - ro["logp"].double())
        assert float((ratio - 1).abs().max()) < 1e-4
        mask = torch.zeros(N, dtype=torch.uint8, device="cuda")
        mask[::3] = 1
        assert env.update_normalizer(pol, ro, mask=mask) is m
        rows = nl.env_rows(mask.cpu().numpy(), T * N)
        feats = ro["features"].cpu().numpy().reshape(T * N, F)
        ref = nl.update(state, feats, rows)
        got = m.get_raw()
        assert got[0] == T * N + T * int(mask.sum())
        held(got, ref[0], T * N, ref[3], ref[4], ("update_normalizer, masked", autoreset))
        own = env.vec.make_moments(F)
        assert env.update_normalizer(pol, ro, moments=own) is own and own.get_raw()[0] == T * N and m.get_raw()[0] == got[0]
        with pytest.raises(AssertionError):
            env.update_normalizer(pol, {"features": ro["features"][:, :, :-1]})
        env.close()


# ---- 7. refusals
def test_every_refusal_on_a_device():
    chub = hub()
    rs = np.random.RandomState(43)
    v, other = make("philox", PILES, N), make("philox", PILES, N)
    lib = v._lib
    D, A = v.obs_dim, v.act_dim
    layers = gaussian_layers(rs, [D, 16, A])
    pol = v.make_policy(layers, normalize=(np.zeros(D, dtype=F32), np.ones(D, dtype=F32), 5.0))
    plain = v.make_policy(layers)
    m, wide, far = v.make_moments(D), v.make_moments(D + 1), other.make_moments(D)
    buf, mask = put(np.zeros((2 * N, D), dtype=F32), D), buffers().DeviceBuffer(N)
    mask.from_host(np.ones(N, dtype=np.uint8))
    vec = np.zeros(D, dtype=np.float64)
    dp = vec.ctypes.data_as(C.c_void_p)

    def refused(code, text, rc):
        assert rc == code and text.encode() in lib.chub_last_error(), (rc, lib.chub_last_error())

    h = C.c_void_p()
    refused(-1, "null argument", lib.chub_moments_create(None, D, C.byref(h)))
    refused(-1, "null argument", lib.chub_moments_create(v._h, D, None))
    for F in (0, -3, 513):
        refused(-1, "F is 1 .. 512", lib.chub_moments_create(v._h, F, C.byref(h)))
        assert not h.value
    upd = lambda mm, x, ld, R, msk: lib.chub_moments_update_device(mm, x, ld, R, msk, None)
    refused(-1, "null argument", upd(None, buf.ptr, D, N, None))
    refused(-1, "null argument", upd(m._m, None, D, N, None))
    refused(-1, "ld is at least F", upd(m._m, buf.ptr, D - 1, N, None))
    refused(-1, "R >= 1", upd(m._m, buf.ptr, D, 0, None))
    refused(-1, "R >= 1", upd(m._m, buf.ptr, D, -N, None))
    refused(-1, "multiple of the handle's 70 envs", upd(m._m, buf.ptr, D, N + 1, mask.ptr))
    assert upd(m._m, buf.ptr, D, N + 1, None) == 0, "without a mask any R"
    refused(-1, "null argument", lib.chub_moments_reset_device(None, None))
    n = C.c_double()
    refused(-1, "null argument", lib.chub_moments_get(None, C.byref(n), dp, dp))
    refused(-1, "null argument", lib.chub_moments_get(m._m, None, dp, dp))
    refused(-1, "null argument", lib.chub_moments_get(m._m, C.byref(n), None, dp))
    refused(-1, "null argument", lib.chub_moments_get(m._m, C.byref(n), dp, None))
    refused(-1, "null argument", lib.chub_moments_set(None, 1.0, dp, dp))
    refused(-1, "null argument", lib.chub_moments_set(m._m, 1.0, None, dp))
    refused(-1, "null argument", lib.chub_moments_set(m._m, 1.0, dp, None))
    before = bits64(m.get_raw())
    for count in (-1.0, float("nan"), float("inf"), -float("inf")):
        refused(-1, "count is finite and >= 0", lib.chub_moments_set(m._m, count, dp, dp))
    assert np.array_equal(bits64(m.get_raw()), before) and before.view(np.float64)[0] == N + 1
    refused(-1, "null argument", lib.chub_moments_state_device(None, C.byref(h)))
    refused(-1, "null argument", lib.chub_moments_state_device(m._m, None))
    # the policy's normaliser: a policy made without one has no buffer the kernel reads
    z = buf.ptr
    for rc in (lib.chub_policy_set_normalizer(plain._p, dp, dp), lib.chub_policy_set_normalizer_device(plain._p, z, z, None),
               lib.chub_policy_get_normalizer_device(plain._p, z, z, None), lib.chub_policy_normalizer_from_moments_device(plain._p, m._m, 1e-8, None)):
        refused(-1, "normalize = 0", rc)
    refused(-1, "null argument", lib.chub_policy_set_normalizer(None, dp, dp))
    refused(-1, "null argument", lib.chub_policy_set_normalizer(pol._p, None, dp))
    refused(-1, "null argument", lib.chub_policy_set_normalizer(pol._p, dp, None))
    refused(-1, "null argument", lib.chub_policy_set_normalizer_device(None, z, z, None))
    refused(-1, "null argument", lib.chub_policy_set_normalizer_device(pol._p, None, z, None))
    refused(-1, "null argument", lib.chub_policy_set_normalizer_device(pol._p, z, None, None))
    refused(-1, "null argument", lib.chub_policy_get_normalizer_device(None, z, z, None))
    refused(-1, "null argument", lib.chub_policy_get_normalizer_device(pol._p, None, z, None))
    refused(-1, "null argument", lib.chub_policy_get_normalizer_device(pol._p, z, None, None))
    frm = lib.chub_policy_normalizer_from_moments_device
    refused(-1, "null argument", frm(None, m._m, 1e-8, None))
    refused(-1, "null argument", frm(pol._p, None, 1e-8, None))
    refused(-1, "different handles", frm(pol._p, far._m, 1e-8, None))
    refused(-1, "the moments have F = %d" % (D + 1), frm(pol._p, wide._m, 1e-8, None))
    for eps in (0.0, -1e-8, float("nan"), float("inf")):
        refused(-1, "eps is finite and > 0", frm(pol._p, m._m, eps, None))
    got = pol.normalizer()
    assert not got[0].any() and (got[1] == 1).all(), "nothing ran"
    with pytest.raises(ValueError):
        pol.set_normalizer(np.zeros(D + 1), np.ones(D + 1))
    with pytest.raises(ValueError):
        m.set(1.0, vec)
    # chub_state_size and snapshots do not know the objects
    size = lib.chub_state_size(v._h)
    assert size == lib.chub_state_size(other._h) and v.make_moments(512) is not None and lib.chub_state_size(v._h) == size
    # the handle destroys its moments; an object outliving it does not touch freed memory
    other.close()
    far.close()
    for x in (m, wide, pol, plain):
        x.close()
    buf.free()
    mask.free()
    v.close()
