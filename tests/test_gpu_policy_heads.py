"""The device actor (chub_policy.hip: k_policy in its three instantiations, k_policy_relayout, chub_policy_run_steps,
chub_policy_collect[_set]) and k_gae at the shapes tests/test_gpu_policy.py, test_gpu_policy_sample.py and test_gpu_pile_set.py do not
reach: the tail means on every alignment against runs of four rows, half-waves, tiles and bit words; three to 65 bit words and up to 130
head tiles for four waves; a head the re-layout kernel covers only in a second pass of its grid; a feature row of 316 floats; the closed
loop on a hub whose stations take the step kernels' chunked forms; GAE around the edges of its chunks of eight steps.  The cases are made
in tests/policy_heads_lib.py, the expected values by policy_lib, policy_sample_lib and pile_set_lib, and tests/test_policy_heads_cpu.py
holds those definitions alone to the caps used here.  Nothing measured is asserted: every tolerance is a bound those libraries compute
from the data."""
import numpy as np
import pytest

import pile_set_lib as psl
import policy_heads_lib as hl
import policy_lib as pl
import policy_sample_lib as ps
from test_gpu_autoreset import Dev
from test_gpu_pile_obs import CANARY, Driver, make
from test_gpu_pile_set import Gae, RollSet, SmpSet
from test_gpu_policy import CANARY64, Act, check_exact, closed_loop_by_hand, f32, gaussian_layers, packed_pair, same_blocks, same_state, upload_layers
from test_gpu_policy_sample import NAMES, Smp, close_all, hold_to_the_definition

pytestmark = pytest.mark.gpu

F32 = np.float32


# ---- 1. the deterministic actor, exact data, bit for bit
@pytest.mark.parametrize("piles", hl.ALL_HUBS, ids=hl.hub_id)
def test_exact_data_equals_the_definition_on_every_head_alignment(piles):
    """the scheme of test_gpu_policy.test_exact_data_equals_the_definition_bit_for_bit: rows, every bit word (bits from S up zero), the
    tail and the words past every output, for nets (), (33,) and (256, 64).  [31, 32], [64, 63] and [255, 0] have rows S + 1 in tile
    2 W: without the head's t < 2 W guard that tile's word lands on the next env's first word, or for the last env (and at N = 1) on
    the canary.  [30, 0], [3, 0] and [4, 3] have one tile of outputs and two of bits: without the bump in chub_policy_create the upper
    half of the word keeps the canary.  The big hubs give one wave up to 33 head tiles and 65 words per env."""
    S = sum(piles)
    sizes = (hl.big_n(piles),) if hl.big_n(piles) else (33, 1)
    for n in sizes:
        v = make("philox", piles, n)
        assert (v.n_slots, v.act_dim, v.bit_words) == (S, S + 2, hl.head_geometry(S)["W"])
        out = Act(v)
        for hidden in hl.NETS:
            layers, obs, a = hl.exact_actor_case(piles, hidden, n)
            pol = v.make_policy(layers, hidden_act="relu", squash="clip")
            got = out.call(pol, obs)
            check_exact(got, a, S, (piles, n, hidden))
            assert n == 1 or (pl.unpack_bits(got[1], S).any() and not pl.unpack_bits(got[1], S).all())
            pol.close()
        out.free()
        v.close()


# ---- 2. the re-layout beyond one pass of its grid
def test_relayout_of_a_head_beyond_one_grid_pass():
    """[4096, 3] behind 256 hidden units: 130 x 256 x 32 head elements for a grid of 1024 x 256 threads, so outputs 1024 and above are
    written by the grid-stride loop's later rounds alone.  The policy as built, then a new head through set_weights, then another
    through set_weights_device: each time the definition's outputs, bit for bit.  A single-pass re-layout leaves zeros (at creation) or
    the previous head (afterwards) there, and policy_heads_lib.relayout_case asserts that the expected outputs from 1024 up are neither."""
    layers, heads, obs, outs = hl.relayout_case()
    piles, n = hl.RELAYOUT_HUB, hl.RELAYOUT_N
    S = sum(piles)
    v = make("philox", piles, n)
    out = Act(v)
    pol = v.make_policy(layers, hidden_act="relu", squash="clip")
    check_exact(out.call(pol, obs), outs[0], S, "as built")
    pol.set_weights(1, *heads[0])
    check_exact(out.call(pol, obs), outs[1], S, "after set_weights")
    (dW, db), = upload_layers([heads[1]])
    pol.set_weights_device(1, dW.ptr, db.ptr)
    v.sync()
    check_exact(out.call(pol, obs), outs[2], S, "after set_weights_device")
    close_all(dW, db, pol, out, v)


# ---- 3. the sampled actor, exact data
@pytest.mark.parametrize("piles,head", [(p, "piles") for p in hl.ALL_HUBS] + [(p, "loads") for p in hl.LOADS_HUBS],
                         ids=lambda c: hl.hub_id(c) if isinstance(c, list) else c)
def test_sampled_exact_data_is_the_definition_on_every_head_alignment(piles, head):
    """the scheme of test_gpu_policy_sample.test_exact_data_is_the_definition over two ticks.  [3, 0]: rows S, S + 1 lie in two runs of
    four, so Gaussian 1 is word 1 of a block its run generates anew -- gb.v[0] in its place fails u's bound.  [4, 3]: the two Gaussian
    terms of logp sit in the two half-waves and meet only in the __shfl_xor; [20, 11]: in two tiles, hence two waves, and meet only in
    the LDS rows (test_logp_cannot_hide_a_term makes a term lost there certain to show).  [30, 0]: the second head tile is all padding
    and must add nothing.  The big hubs: a wave's terms run over up to 33 tiles.  LOADS: the rows are load_dispatch of the device's
    own clipped u, on [300, 20] and [4096, 3] through its big-station path."""
    n, S = hl.sampled_n(piles), sum(piles)
    layers, obs, ls, z, err = hl.sampled_case(piles, head)
    v = make("philox", piles, n)
    pol = v.make_policy(layers, head=head, hidden_act="relu", squash="clip")
    pol.set_exploration(hl.KEY, ls)
    out = Smp(v, pol)
    undecided = total = 0
    for moment in range(2):
        tick = v.next_tick()
        assert tick == 1 + moment
        d = hl.sampled_definition(piles, head, tick, z, err, ls)
        got = out.call(obs)
        assert np.array_equal(got["feat"], obs.view(np.uint32)), "the raw feature row, bit for bit"
        rows_are = None
        if head == "loads":
            uq = np.clip(f32(got["u"]), -1, 1)
            rows_are = v.load_dispatch(uq[:, :2], uq[:, 2:], units="fraction")
        a, b = hold_to_the_definition(got, d, head, S, "clip", (piles, head, moment), rows_are)
        undecided, total = undecided + a, total + b
        v.reset()  # (the tick moves: new noise)
    print("%s %s: %d of %d pile decisions undecided" % (piles, head, undecided, total))
    assert undecided <= hl.UNDECIDED_CAP * total
    close_all(out, pol, v)


# ---- 4. a log-probability that cannot hide a term
@pytest.mark.parametrize("piles", hl.ALL_HUBS, ids=hl.hub_id)
def test_logp_cannot_hide_a_term(piles):
    """zero weights, so z is the bias exactly and err_z = 0; saturated piles whose term is below 2e-28 and about 25 live ones whose term
    is at least 0.127, at piles 0 and 1, around the first tile and word boundaries, at the end of the row and at seeded places.  The
    definition's bound is at most a quarter of the smallest live term (asserted here for the decisions taken and, on the same data, in
    tests/test_policy_heads_cpu.py), so a term lost in the half-waves' shuffle ([4, 3]), in the waves' LDS rows ([20, 11] and up) or in a
    wave's walk over its tiles (the big hubs) is outside the bound, as is a term the set launch counts or skips wrongly: the sets are
    asserted to split the live piles."""
    n, S = hl.sampled_n(piles), sum(piles)
    layers, obs, ls, live = hl.live_case(piles)
    v = make("philox", piles, n)
    drv = Driver(v, "philox")
    pol = v.make_policy(layers)
    pol.set_exploration(hl.KEY, ls)
    out = SmpSet(v, pol)
    split = {which: [0, 0] for which in ("occupied", "decidable")}
    for moment, steps in enumerate((0, 8)):
        drv.reset()
        for _ in range(steps):
            drv.step()
        assert v.next_tick() == hl.LIVE_TICKS[moment]
        d = hl.live_definition(piles, layers, obs, ls, hl.LIVE_TICKS[moment])
        assert d.decided.all(), "with err_z = 0 the bound decides every pile"
        plain = out.call(obs)
        hold_to_the_definition(plain, d, "piles", S, "tanh", (piles, "plain", moment))
        on = pl.unpack_bits(plain["bits"], S)
        hl.assert_live_condition(d, layers, live, on)
        for which in psl.PSET_NAMES:
            got, words = out.call_set(which, obs)
            in_set = v.pile_set(which)
            assert np.array_equal(words, psl.words(in_set)), (which, "d_set_bits")
            for k in NAMES:
                if k != "logp" or which == "all":
                    assert np.array_equal(got[k], plain[k]), (piles, which, k, "bit for bit the plain sampled call's")
            value, bound = psl.masked_logp(d, on, in_set)
            hl.assert_live_condition(d, layers, live, on, in_set)
            lerr = np.abs(f32(got["logp"]).astype(np.float64) - value)
            print("%s %s after %d steps: logp max error %.3g of bound %.3g, live piles in the set %d of %d" %
                  (piles, which, steps, lerr.max(), bound.max(), in_set[:, live].sum(), in_set[:, live].size))
            assert (lerr <= bound).all(), (piles, which, "logp beyond its bound", lerr.max(), bound.max())
            if which != "all":
                split[which][0] += int(in_set[:, live].sum())
                split[which][1] += int((~in_set[:, live]).sum())
    for which, (inside, outside) in split.items():
        assert inside > 0 and outside > 0, (piles, which, "the set does not split the live piles", inside, outside)
    close_all(out, pol, v)


# ---- 5. feature rows wider than 256
def check_wide_feature_row(v, out, obs, what):
    """test_gpu_policy.check_feature_row for hl.WIDE_INPUTS: one layer that selects features, normalised by an exact power of two; output
    n is feature sel[n] * 2^-14, bit for bit; two selections cover the 316 features (the second through set_weights)"""
    want = pl.features([obs, v.pile_obs(("car",))])
    n, F = want.shape
    A = v.act_dim
    scale = F32(2.0 ** -14)
    assert F == 316 and np.abs(want).max() < 2.0 ** 14 and np.isfinite(want).all()
    pol = None
    for start in range(0, F, A):
        sel = (start + np.arange(A)) % F
        W0 = np.zeros((A, F), dtype=F32)
        W0[np.arange(A), sel] = 1
        if pol is None:
            pol = v.make_policy([(W0, np.zeros(A, dtype=F32))], inputs=hl.WIDE_INPUTS, squash="clip",
                                normalize=(np.zeros(F, dtype=F32), np.full(F, scale), 1.0))
            assert pol.n_features == F
        else:
            pol.set_weights(0, W0, np.zeros(A, dtype=F32))
        rows, _, _ = out.call(pol, obs)
        bad = np.nonzero(rows != (want[:, sel] * scale).astype(F32).view(np.uint32))
        assert bad[0].size == 0, (what, "first (env, output)", [int(x[0]) for x in bad], "feature", sel[bad[1][:1]])
    pol.close()
    return want


def test_feature_rows_wider_than_256():
    """[300, 3] with the observation and the car column: F = 316, P image rows 0 .. 315, f_pad = 316.  After a reset and after 3 steps:
    every feature is found at its place (a wrong stride or an index that wraps in the gather puts another feature there); then an exact
    network [316, 64, A] behind a dyadic normalisation with a clip, deterministic and sampled, the sampled call's `features` being the raw
    blocks before normalisation"""
    piles, n = hl.WIDE_HUB, hl.WIDE_N
    S = sum(piles)
    F, layers, obs, norm = hl.wide_case()
    v = make("philox", piles, n)
    drv = Driver(v, "philox")
    out = Act(v)
    pol = v.make_policy(layers, inputs=hl.WIDE_INPUTS, hidden_act="relu", squash="clip", normalize=norm)
    assert pol.n_features == F
    ls = np.array([-1.0, -0.5], dtype=F32)
    pol.set_exploration(hl.KEY, ls)
    smp = Smp(v, pol)
    real = drv.reset().copy()
    cars = []
    for moment in range(2):
        raw = check_wide_feature_row(v, out, real, ("real observations, moment", moment))
        car = raw[:, v.obs_dim:]
        cars.append(car)
        x = hl.wide_normalised(obs, car, norm)
        pl.assert_exact(x, layers)
        check_exact(out.call(pol, obs), pl.forward(x, layers, "relu", "clip")[0], S, ("F = 316", moment))
        z, err = ps.pre_squash(x, layers, "relu")
        d = ps.Sample(z, err, "piles", S, hl.KEY, v.next_tick(), np.arange(n), ls)
        got = smp.call(obs)
        assert np.array_equal(got["feat"], pl.features([obs, car]).view(np.uint32)), "raw blocks, before normalisation"
        a, b = hold_to_the_definition(got, d, "piles", S, "clip", ("F = 316 sampled", moment))
        assert a <= hl.UNDECIDED_CAP * b
        for _ in range(3):
            real = drv.step()[0].copy()
    assert cars[1].any() and not np.array_equal(cars[0], cars[1]), "the car column moves with the state"
    close_all(smp, out, pol, v)


# ---- 6. the closed loop on a chunked hub
@pytest.mark.parametrize("mode,head", [("lockstep", "piles"), ("autoreset", "piles"), ("lockstep", "loads"), ("autoreset", "loads")])
def test_run_steps_on_a_chunked_hub_equals_the_same_calls_one_by_one(mode, head):
    """the scheme of test_gpu_policy.test_run_steps_equals_the_same_calls_one_by_one on [300, 20]: the actor's five bit words feed the
    chunked step kernels, its loads head load_dispatch's big-station path, inside the loop.  A day plus 5 steps in one call, then 7 more"""
    piles, n = hl.LOOP_HUB, hl.LOOP_N
    rs = np.random.RandomState(29)
    va, vb = make("philox", piles, n, seed=6), make("philox", piles, n, seed=6)
    D = va.obs_dim
    layers = gaussian_layers(rs, [D, 64, va.act_dim] if head == "piles" else [D, 33, 4])
    pa, pb = va.make_policy(layers, head=head), vb.make_policy(layers, head=head)
    da, db, ob = Dev(va), Dev(vb), Act(vb)
    ka, kb = packed_pair(va), packed_pair(vb)
    if mode == "autoreset":
        va.reset_device(da.obs.ptr)
        vb.reset_device(db.obs.ptr)
    for first, count in ((0, 101), (101, 7)):
        reset_obs = da.obs.ptr if (mode == "lockstep" or first == 0) else 0
        pa.run_steps([b.ptr for b in ka], count, first_step=first, mode=mode, d_reset_obs=reset_obs, d_final_obs=da.final.ptr if mode == "autoreset" else 0)
        closed_loop_by_hand(vb, pb, db, ob, mode, first, count, kb, from_obs=first == 0)
        va.sync()
        vb.sync()
        same_blocks(va, ka, kb, (mode, head, first))
        same_state(va, vb, (mode, head, first))
        if mode == "autoreset":
            assert np.array_equal(da.final.to_host(np.uint32, (n, D)), db.final.to_host(np.uint32, (n, D)))
    assert va.env_clocks().tolist() == [(101 + 7) % 96] * n
    close_all(pa, pb, ob, *(ka + kb))
    va.close()
    vb.close()


def test_collect_set_on_a_chunked_hub_across_a_days_end():
    """100 auto-reset steps of collect_set("decidable") on [300, 20] against single sample_set_device + step calls on a twin.  A rollout
    holds at most 96 steps in this mode, so the 100 are two calls of 60 and 40: the day ends at the 36th step of the second, and the
    actor's next step reads the re-started envs' observation from the packed block.  Every kept array, the set words included"""
    piles, n, T = hl.LOOP_HUB, hl.LOOP_N, 60
    rs = np.random.RandomState(29)
    va, vb = make("philox", piles, n, seed=6), make("philox", piles, n, seed=6)
    D, S = va.obs_dim, sum(piles)
    layers = gaussian_layers(rs, [D, 64, va.act_dim])
    pols = [v.make_policy(layers) for v in (va, vb)]
    for p in pols:
        p.set_exploration(77, np.array([-0.5, 0.0], dtype=F32))
    ra, rb = RollSet(va, pols[0], T), RollSet(vb, pols[1], T)
    for v, r in ((va, ra), (vb, rb)):
        v.reset_device(r.ptr("obs0"))
    dones = 0
    for first, count in ((0, 60), (60, 40)):
        ra.collect_set("autoreset", "decidable", first=first, T=count)
        rb.by_hand_set("autoreset", "decidable", first=first, T=count)
        ha, hb = ra.host(), rb.host()
        for k in ha:
            x, y = (ha[k], hb[k]) if k in ("final", "obs0") else (ha[k][:count], hb[k][:count])
            assert np.array_equal(x, y), (first, k, np.nonzero(x != y)[0][:4])
        same_state(va, vb, ("collect_set", first))
        sets = pl.unpack_bits(ha["set"][:count].reshape(count * n, -1), S)
        assert sets.any() and not sets.all()
        done = f32(ha["packed"])[:count, :, D + 1] == 1
        dones += int(done.sum())
        if first:
            assert done[35].all() and done.sum() == n, "the day's 96th step"
            assert not (ha["final"] == CANARY).any() and np.isfinite(f32(ha["packed"])[:count]).all()
        for r, h in ((ra, ha), (rb, hb)):
            r.buf["obs0"].from_host(h["packed"][count - 1, :, :D].copy())
    assert dones == n and va.env_clocks().tolist() == [4] * n
    close_all(ra, rb, *pols)
    va.close()
    vb.close()


def test_stepping_the_rows_equals_stepping_the_bits_on_a_chunked_hub():
    """the scheme of test_gpu_policy.test_stepping_the_rows_equals_stepping_the_bits on [300, 20]: twins from one seed, one steps the
    policy's action rows, the other its five bit words and tail; 100 steps (a reset at step 96), packed outputs and state identical"""
    piles, n = hl.LOOP_HUB, hl.LOOP_N
    rs = np.random.RandomState(21)
    va, vb = make("philox", piles, n, seed=5), make("philox", piles, n, seed=5)
    D, A = va.obs_dim, va.act_dim
    assert vb.bit_words == 5
    layers = gaussian_layers(rs, [D, 64, A])
    pa, pb = va.make_policy(layers), vb.make_policy(layers)
    da, db = Dev(va), Dev(vb)
    oa, ob = Act(va, D + 2), Act(vb, D + 2)
    ons = 0
    for i in range(100):
        if i in (0, 96):
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
    close_all(pa, pb, oa, ob)
    va.close()
    vb.close()


# ---- 7. GAE at its chunk edges
@pytest.fixture(scope="module")
def gae_handle():
    v = make("philox", [20, 25], hl.GAE_N)
    yield v
    v.close()


@pytest.mark.parametrize("T", hl.GAE_T)
def test_gae_at_the_edges_of_its_chunks_bit_for_bit(gae_handle, T):
    """k_gae sweeps backwards in chunks of eight prefetched steps: T = 7 is one partial chunk, 8 one full, 9 and 13 a partial chunk after
    a full one, 17 two full and one step.  done on the last element of a chunk, on the first of the next, on both (consecutive), at every
    step and nowhere, per env from a seed; with and without final_values and ret, under a mask; 300 envs are a full workgroup and a
    ragged one.  A carry of adv or v_next lost or kept across a chunk's edge changes adv there, and psl.gae_f32 is bit for bit"""
    v = gae_handle
    g = Gae(v, T)
    D, N = v.obs_dim, hl.GAE_N
    assert D == 13
    for dones in hl.GAE_DONES:
        for with_final in (False, True):
            packed, values, final = hl.gae_edge_case(T, dones, with_final, D=D)
            r, dn = packed[:, :, D], packed[:, :, D + 1]
            for gamma, lam in psl.GAE_FACTORS:
                want_a, want_r = psl.gae_f32(r, dn, values, final, gamma, lam)
                adv, ret, st = g.call(packed, values, final, gamma, lam)
                what = (T, dones, with_final, gamma, lam)
                assert np.array_equal(adv, want_a.view(np.uint32)), (what, "adv", np.nonzero(adv != want_a.view(np.uint32))[0][:4])
                assert np.array_equal(ret, want_r.view(np.uint32)), (what, "ret")
                assert (st == CANARY64).all(), (what, "no statistics asked for")
            want_a, _ = psl.gae_f32(r, dn, values, final, 0.99, 0.95)
            adv, ret, _ = g.call(packed, values, final, 0.99, 0.95, ret=False)
            assert np.array_equal(adv, want_a.view(np.uint32)) and (ret == CANARY).all(), (T, dones, with_final, "d_ret = NULL")
            mask = np.where(np.arange(N) % 4 == 1, 7, 0).astype(np.uint8)
            on = mask != 0
            adv_m, ret_m, _ = g.call(packed, values, final, 0.99, 0.95, mask=mask)
            assert np.array_equal(adv_m[:, on], adv[:, on]) and (adv_m[:, ~on] == CANARY).all() and (ret_m[:, ~on] == CANARY).all(), "a device mask"
            assert not (ret_m[:, on] == CANARY).any()
    # the statistics once: the pair pattern, under the mask
    packed, values, final = hl.gae_edge_case(T, "pair", True, D=D)
    adv, _, st = g.call(packed, values, final, 0.99, 0.95, mask=mask, stats=True)
    want, bound = psl.stats_of(f32(adv)[:, on])
    got = st.view(np.float64)
    assert got[0] == want[0] == T * on.sum(), "the count is exact"
    assert abs(got[1] - want[1]) <= bound[1] and abs(got[2] - want[2]) <= bound[2], (got, want, bound)
    g.free()
