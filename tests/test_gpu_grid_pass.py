"""The population launch and the moments stream past their first grid pass, on the cases of tests/grid_pass_lib.py (why they are the right
ones: tests/test_grid_pass_cpu.py).  (a) the population's actor launch on 10 to 70 workgroups, where its XCD-aware tile order is no longer
the identity, against one plain policy per member bit for bit, with a mask across an XCD run's and a member's edge, and perturb against
tests/population_lib.py at 11 and 35 pairs; (b) the closed loop on a permuted grid against handles of a member's own; (c) moments streams of
two and three trips of k_moments' loop; (d) a mask over more envs than a grid pass has rows; (e) F at the edges of the lane layout;
(f) the ES gradient and perturb at P = 2100, under the 64-chunk cap.  The expected values are tests/population_lib.py's and
tests/normalizer_lib.py's; every size comes from chub_device_info at run time."""
import ctypes as C

import numpy as np
import pytest

import grid_pass_lib as gpl
import normalizer_lib as nl
import population_lib as popl
from test_gpu_autoreset import Dev, buffers
from test_gpu_normalizer import bits64, columns, held, launch_shape, put
from test_gpu_pile_obs import make
from test_gpu_policy import gaussian_layers, packed_pair
from test_gpu_population import KEY, LayerBuffers, act_equals_member_policies, assert_members, member_device, sizes_of

pytestmark = pytest.mark.gpu

F32 = np.float32


def shape_of(v, F):
    """(RW, grid) through launch_shape, which asks chub_device_info; the case arithmetic's own statement of it has to agree"""
    info = (C.c_int32 * 4)()
    assert v._lib.chub_device_info(0, info) == 0
    rw, grid = launch_shape(v, F)
    assert (rw, grid) == gpl.moments_shape(F, info[3])[1:], (F, info[3])
    return rw, grid


# ---- a. the population's actor launch on permuted grids
@pytest.mark.parametrize("P,E", gpl.POP_CASES, ids=lambda x: str(x))
def test_act_on_a_permuted_grid_equals_a_plain_policy_per_member(P, E):
    """nb = 10, 16, 12, 18, 22, 70 workgroups (nb % 8 = 2, 0, 4, 2, 6, 6; one, two and three tiles a member): a workgroup's tile is not its
    index, so a map that serves a tile twice leaves another tile's canaries, and a member taken from the workgroup's index instead of its
    tile evaluates the wrong weights.  Every form of act_equals_member_policies; the masked one names the rows around the first tile of
    XCD 1's run, a member's first tile, and the last row.  At 11 and 35 pairs perturb is held for every member first"""
    rs = np.random.RandomState(1000 + 7 * P + E)
    v = make("philox", gpl.POP_HUB, P * E)
    assert gpl.pop_grid(P, E)[0] == -(-v.n_envs // 32) > 8
    D = v.obs_dim
    obs = rs.normal(size=(P * E, D)).astype(F32)
    sizes = sizes_of(v, gpl.POP_HIDDEN)
    shapes = list(zip(sizes[1:], sizes[:-1]))
    centre = gaussian_layers(rs, sizes)
    pol = v.make_policy(centre)
    pop = v.make_population(pol, P, KEY)
    pop.perturb_device(0.3, 11)
    v.sync()
    if (P, E) in gpl.POP_PERTURB:
        want = popl.members(centre, 0.3, KEY, 11, P)
        out = LayerBuffers(shapes)
        for m in range(P):
            assert_members(member_device(v, pop, out, m), want[m], (P, E, "perturb", m))
        out.free()
    lds = (D,) if P == 70 else (D, D + 2)
    assert act_equals_member_policies(v, pop, P, E, obs, v.make_policy, ("permuted grid", P, E), lds, mask=gpl.edge_mask(P, E)) == 12 * P * len(lds)
    pop.close()
    pol.close()
    v.close()


# ---- b. the closed loop on a permuted grid
def test_a_members_block_on_a_permuted_grid_equals_a_handle_of_its_own():
    """4 steps from a reset on 10 workgroups: members 0, 1, 4 and 9 against handles of 32 envs with env_id0 = 32 m, the same seed and a plain
    policy holding the member's weights -- not the same kernel call on either side"""
    (P, E), members = gpl.POP_OWN_HANDLE
    rs = np.random.RandomState(53)
    n = P * E
    v = make("philox", gpl.POP_HUB, n, seed=21)
    D = v.obs_dim
    pol = v.make_policy(gaussian_layers(rs, sizes_of(v, gpl.POP_HIDDEN)))
    pop = v.make_population(pol, P, KEY)
    pop.perturb(0.4, 8)
    dv, k = Dev(v), packed_pair(v)
    pop.run_steps([b.ptr for b in k], 4, mode="lockstep", d_reset_obs=dv.obs.ptr)
    v.sync()
    big = [b.to_host(np.uint32, (n, D + 2)) for b in k]
    obs0 = dv.obs.to_host(np.uint32, (n, D))
    for m in members:
        s = make("philox", gpl.POP_HUB, E, seed=21, env_id0=m * E)
        ps = s.make_policy(pop.get_member(m))
        ds, ks = Dev(s), packed_pair(s)
        ps.run_steps([b.ptr for b in ks], 4, mode="lockstep", d_reset_obs=ds.obs.ptr)
        s.sync()
        assert np.array_equal(ds.obs.to_host(np.uint32, (E, D)), obs0[m * E:(m + 1) * E]), (m, "the reset's observation")
        for j in range(2):
            assert np.array_equal(ks[j].to_host(np.uint32, (E, D + 2)), big[j][m * E:(m + 1) * E]), ("member", m, "packed block", j)
        ps.close()
        s.close()
    assert not np.array_equal(big[1][:E], big[1][E:2 * E]), "the members' blocks differ"
    pop.close()
    pol.close()
    v.close()


# ---- c .. e. the moments stream
def two_updates(v, m, F, R, ld, mask, mask_buf, what, own_last=False):
    """from zeros and onto the state the first update left, each held to the definition applied to the state the device started from, as
    test_gpu_normalizer.py's shape grid does"""
    N = v.n_envs
    rows = None if mask is None else nl.env_rows(mask, R)
    if mask is not None:
        mask_buf.from_host(mask.astype(np.uint8))
    m.reset_device()
    state = m.get_raw()
    assert state[0] == 0 and not bits64(state).any()
    for k in range(2):
        x = gpl.moments_batch(columns, F, R, k, own_last=own_last)
        buf = put(x, ld)
        m.update_device(buf.ptr, R, ld=ld, d_mask=mask_buf.ptr if mask is not None else 0)
        got = m.get_raw()
        buf.free()
        ref, _, n_b, S2, dmax = nl.update(state, x, rows)
        assert n_b == (R if rows is None else int(rows.sum())) > 0
        held(got, ref, R, S2, dmax, what + (R, ld, "no mask" if mask is None else "%d of %d envs" % (mask.sum(), N), k))
        state = got


@pytest.mark.parametrize("F", gpl.LONG_F)
def test_a_stream_of_two_trips(F):
    """R = the smallest multiple of 70 above 8 grid RW + 257: every workgroup makes one whole trip of its loop and the first ones a second,
    whose k = 0 is live and whose last k is past R -- the row and offset carried across the trip, and under the mask the env.  One F also
    with two floats between the rows"""
    v = make("philox", gpl.MOMENTS_PILES, gpl.MOMENTS_N)
    rw, grid = shape_of(v, F)
    R = gpl.long_rows(rw, grid)
    assert gpl.trips_of(R, rw, grid) == 2
    m, mask_buf = v.make_moments(F), buffers().DeviceBuffer(gpl.MOMENTS_N)
    for ld in (F, F + 2) if F == gpl.LONG_LD_F else (F,):
        for mask in (None, gpl.random_mask(gpl.MOMENTS_N, F)):
            two_updates(v, m, F, R, ld, mask, mask_buf, ("two trips", F))
    mask_buf.free()
    m.close()
    v.close()


def test_a_stream_of_three_trips_with_a_ragged_end():
    """F = 64 at R above 16 grid RW + 3 RW + 1: two whole trips, and a third that only the first workgroups make, with k = 0 alone live"""
    F = gpl.RAGGED_F
    v = make("philox", gpl.MOMENTS_PILES, gpl.MOMENTS_N)
    rw, grid = shape_of(v, F)
    R = gpl.ragged_rows(rw, grid)
    assert gpl.trips_of(R, rw, grid) == 3 and gpl.live_of(R, rw, grid, 0, 2) == [True] + [False] * 7
    m, mask_buf = v.make_moments(F), buffers().DeviceBuffer(gpl.MOMENTS_N)
    for mask in (None, gpl.random_mask(gpl.MOMENTS_N, F + 1)):
        two_updates(v, m, F, R, F, mask, mask_buf, ("three trips", F))
    mask_buf.free()
    m.close()
    v.close()


def test_a_long_masked_stream_twice_and_with_masked_out_nans():
    """two trips under a mask: the same call from the same state gives the same bits, and so does one whose masked-out rows are NaN (a row
    that does not count is not read into the sums in the second trip either)"""
    F, N = gpl.DETERMINISM_F, gpl.MOMENTS_N
    rs = np.random.RandomState(19)
    v = make("philox", gpl.MOMENTS_PILES, N)
    rw, grid = shape_of(v, F)
    R = gpl.long_rows(rw, grid)
    m = v.make_moments(F)
    x = gpl.moments_batch(columns, F, R, 0)
    mask = gpl.random_mask(N, 3)
    mask[0] = True  # (row 0 is the pivot of an empty state whether it counts or not: it stays finite)
    rows = nl.env_rows(mask, R)
    x_nan = x.copy()
    x_nan[~rows] = np.nan
    buf, buf_nan, mask_buf = put(x, F), put(x_nan, F), buffers().DeviceBuffer(N)
    mask_buf.from_host(mask.astype(np.uint8))
    start = (5.0, x[:5].astype(np.float64).mean(axis=0), np.abs(rs.normal(size=F)))
    for state in (nl.zero_state(F), start):
        seen = []
        for src in (buf, buf, buf_nan):
            m.set(state[0], state[1], m2=state[2])
            m.update_device(src.ptr, R, d_mask=mask_buf.ptr)
            seen.append(bits64(m.get_raw()))
        assert np.array_equal(seen[0], seen[1]), "two calls from the same state: identical bits"
        assert np.array_equal(seen[0], seen[2]), "masked-out rows filled with NaN change nothing"
        assert np.isfinite(seen[0].view(np.float64)).all() and seen[0].view(np.float64)[0] == state[0] + rows.sum()
    for b in (buf, buf_nan, mask_buf):
        b.free()
    m.close()
    v.close()


@pytest.mark.parametrize("F", gpl.WIDE_F)
def test_a_mask_over_more_envs_than_a_grid_pass_has_rows(F):
    """a handle of N > grid RW envs (about 5000 at F = 64 and 1400 at F = 512 on 256 compute units): the env of a lane's next row is
    e + grid RW with ONE subtraction of N, on a step that no remainder has reduced.  R = 3 N: with a mask R is a multiple of N
    (include/chub.h; chub_moments_update_device refuses 3 N + 17, which is held here too)"""
    probe = make("philox", gpl.WIDE_PILES, 32)
    rw, grid = shape_of(probe, F)
    probe.close()
    N, R = gpl.wide_envs(rw, grid), gpl.wide_rows(rw, grid)
    assert N > grid * rw and min(-(-R // rw), grid) * rw < N
    v = make("philox", gpl.WIDE_PILES, N)
    m, mask_buf = v.make_moments(F), buffers().DeviceBuffer(N)
    for mask in (gpl.random_mask(N, F), None):
        two_updates(v, m, F, R, F, mask, mask_buf, ("wide mask", F))
    before = bits64(m.get_raw())
    buf = put(np.zeros((1, F), dtype=F32), F)  # (refused before any device work)
    assert v._lib.chub_moments_update_device(m._m, buf.ptr, F, R + 17, mask_buf.ptr, None) == -1
    assert b"multiple of the handle's %d envs" % N in v._lib.chub_last_error() and np.array_equal(bits64(m.get_raw()), before)
    buf.free()
    mask_buf.free()
    m.close()
    v.close()


@pytest.mark.parametrize("F", gpl.EDGE_F)
def test_the_lane_layouts_edges(F):
    """F = 128 | 129: two rows a pass with the LDS tree, then one row and no tree; 255 | 256: the last shapes with one column a lane;
    257: two columns a lane, for lane 0 alone -- column 256 has a scale and an offset of its own, so that column 0 read in its place
    cannot pass.  R = 1, 257 and beyond one pass of the grid; the mask where R is a multiple of N"""
    v = make("philox", gpl.MOMENTS_PILES, gpl.MOMENTS_N)
    rw, grid = shape_of(v, F)
    assert rw == (2 if F == 128 else 1)
    m, mask_buf = v.make_moments(F), buffers().DeviceBuffer(gpl.MOMENTS_N)
    for R in gpl.edge_rows(rw, grid):
        for mask in (None, gpl.random_mask(gpl.MOMENTS_N, F)) if R % gpl.MOMENTS_N == 0 else (None,):
            two_updates(v, m, F, R, F, mask, mask_buf, ("lane layout", F), own_last=F == 257)
    if F == 257:
        x = gpl.moments_batch(columns, F, 257, 0, own_last=True).astype(np.float64)
        assert abs(x[:, 256].mean() - x[:, 0].mean()) > 30 and x[:, 256].std() > 50 * x[:, 0].std()
    mask_buf.free()
    m.close()
    v.close()


# ---- f. the ES gradient and perturb under the chunk cap
def test_es_gradient_and_perturb_under_the_chunk_cap():
    """P = 2100 members of 32 envs on hub [1, 1]: 1050 pairs are 62 chunks of 17 pairs, the last of 13 (chub_population_create's cap of 64
    chunks binds above P = 2048).  The gradient within population_lib's bound on general utilities, the same bits on a second call,
    +0.0f everywhere on utilities equal within pairs; perturb bit for bit for the first and the last pair and one of a middle chunk"""
    P, E = gpl.ES_P, gpl.ES_E
    rs = np.random.RandomState(P)
    mg = buffers()
    v = make("philox", gpl.ES_HUB, P * E)
    sizes = sizes_of(v, gpl.ES_HIDDEN)
    shapes = list(zip(sizes[1:], sizes[:-1]))
    centre, theta = gaussian_layers(rs, sizes), gaussian_layers(rs, sizes)
    pol = v.make_policy(centre)
    pop = v.make_population(pol, P, KEY)
    cp, chunks = gpl.es_chunks(P, gpl.es_items(shapes))
    assert cp > gpl.CHUNK_PAIRS and (chunks - 1) * cp < P // 2 < chunks * cp
    out, src = LayerBuffers(shapes), LayerBuffers(shapes)
    d_util = mg.DeviceBuffer(P * 4)

    def call(util, g):
        out.fill()
        d_util.from_host(np.ascontiguousarray(util, dtype=F32))
        v.sync()
        pop.es_gradient_device(d_util.ptr, g, *out.ptrs())
        v.sync()
        return [out.read(l) for l in range(len(shapes))]

    g, util = 5, (rs.normal(size=P) * 10 + 3).astype(F32)
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
    pairs = np.repeat(rs.normal(size=P // 2).astype(F32), 2)
    for W, b in call(pairs, g):
        assert (W == 0).all() and (b == 0).all(), "equal utilities within every pair: +0.0f everywhere"
    # perturb: the pair index j = q / tiles up to 1049
    src.put(theta)
    pop.perturb_device(0.05, 3, *src.ptrs())
    v.sync()
    want = popl.members(theta, 0.05, KEY, 3, P)
    j_mid = (chunks // 2) * cp + cp // 2
    for mbr in (0, 1, 2 * j_mid, 2 * j_mid + 1, P - 2, P - 1):
        assert_members(member_device(v, pop, out, mbr), want[mbr], (P, "perturb", mbr))
    for x in (out, src, d_util):
        x.free()
    pop.close()
    pol.close()
    v.close()
