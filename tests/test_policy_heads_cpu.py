"""The cases of tests/test_gpu_policy_heads.py without a device (tests/policy_heads_lib.py makes them for both files): the hubs show the
alignments they are listed for; the definition ALONE stays within the caps the GPU test uses on that test's own data -- at most 0.1 % of a
hub's pile decisions undecided, and on the live / saturated biases a log-probability bound of at most a quarter of the smallest live term;
the Philox block and the tabulated normal behind those expected values are the ones tests/test_policy_sample_cpu.py holds to the oracle;
and the GAE blocks fire where their names say, with the f32 recurrence inside its derived bound of the textbook sum."""
import numpy as np
import pytest

import pile_set_lib as psl
import policy_heads_lib as hl
import policy_lib as pl
import policy_sample_lib as ps
import test_policy_sample_cpu

F32 = np.float32


def test_the_hubs_show_the_alignments_they_are_listed_for():
    """arithmetic on S alone, from the kernel's layout as policy_heads_lib.head_geometry states it"""
    geo = {hl.hub_id(p): hl.head_geometry(sum(p)) for p in hl.ALL_HUBS}
    S = {hl.hub_id(p): sum(p) for p in hl.ALL_HUBS}
    assert [S[hl.hub_id(p)] for p in hl.ALIGN_HUBS] == [3, 7, 31, 63, 127, 30, 62]
    assert [S[hl.hub_id(p)] for p, _ in hl.BIG_HUBS] == [170, 255, 320, 4099]
    # the Gaussian pair in two runs of four; in two half-waves; in two tiles, hence two waves
    assert all(S[k] % 4 == 3 and geo[k]["run"][0] != geo[k]["run"][1] for k in ("3x0", "4x3", "20x11", "31x32", "64x63", "255x0", "4096x3"))
    assert geo["3x0"]["half"][0] == geo["3x0"]["half"][1] and all(geo[k]["half"][0] != geo[k]["half"][1] for k in ("4x3", "20x11", "31x32"))
    assert geo["4x3"]["tile"][0] == geo["4x3"]["tile"][1] and all(geo[k]["tile"][0] != geo[k]["tile"][1] for k in ("20x11", "31x32", "64x63", "255x0"))
    # Gaussian 1 in a tile past the env's last bit word: only the t < 2 W guards keep that word from being read or written
    for k in ("31x32", "64x63", "255x0"):
        assert geo[k]["tile"][1] == 2 * geo[k]["W"] == geo[k]["tiles"] - 1, k
    assert geo["20x11"]["tile"][1] == 1 < 2 * geo["20x11"]["W"]
    # the bump: one tile of outputs, two tiles of bits -- the second tile is all padding; A = 64 fills two tiles to the last row
    assert (geo["30x0"]["plain"], geo["30x0"]["tiles"]) == (1, 2) and S["30x0"] + 2 == 32
    assert (geo["0x62"]["plain"], geo["0x62"]["tiles"]) == (2, 2) and S["0x62"] + 2 == 64
    assert [geo[k]["plain"] == geo[k]["tiles"] for k in ("3x0", "4x3", "20x11")] == [False, False, True]
    # three and more bit words; more head tiles than a workgroup has waves (4), so that a wave's logp terms run over several tiles
    assert [geo[hl.hub_id(p)]["W"] for p, _ in hl.BIG_HUBS] == [3, 4, 5, 65]
    assert [geo[hl.hub_id(p)]["plain"] for p, _ in hl.BIG_HUBS] == [6, 9, 11, 129]
    assert [geo[hl.hub_id(p)]["tiles"] for p, _ in hl.BIG_HUBS] == [6, 9, 11, 130]  # (S = 4099: 129 tiles of outputs, 65 words of bits)


def test_philox_and_the_normal_are_the_ones_held_to_the_oracle():
    """the cases' expected values come from policy_sample_lib's own Sample, noise_words, philox and normal_from_word (imported, not
    restated), and that module's functions are what tests/test_policy_sample_cpu.py compares with the oracle -- run here once more"""
    assert hl.ps is ps and hl.psl is psl and hl.pl is pl and psl.ps is ps
    for name in ("philox", "noise_words", "normal_from_word", "normal_tables", "Sample"):
        assert not hasattr(hl, name), ("restated in policy_heads_lib", name)
    assert test_policy_sample_cpu.ps is ps
    test_policy_sample_cpu.test_philox_and_the_tabulated_normal_are_the_oracles()
    # the words of the runs the alignment hubs are about: pile S - 1 is word 2 of block S >> 2, the Gaussians words 0 and 1 of one block
    for piles in hl.ALIGN_HUBS[:5]:
        S = sum(piles)
        pw, gw = ps.noise_words(hl.KEY, 2, [0, 69], S, 2)
        k0, k1 = hl.KEY & 0xFFFFFFFF, hl.KEY >> 32
        assert pw[1, S - 1] == ps.philox(S >> 2, 15 << 16, 2, 69, k0, k1)[2]
        assert np.array_equal(gw[1], ps.philox(0, (15 << 16) | 1, 2, 69, k0, k1)[:2]) and gw[1, 0] != gw[1, 1]


def sampled_cases():
    for piles in hl.ALL_HUBS:
        yield piles, "piles"
    for piles in hl.LOADS_HUBS:
        yield piles, "loads"


@pytest.mark.parametrize("piles,head", list(sampled_cases()), ids=lambda c: hl.hub_id(c) if isinstance(c, list) else c)
def test_the_exact_sampled_cases_stay_within_the_undecided_cap(piles, head):
    """the two ticks the GPU test takes per hub (and six more): at most 0.1 % of the hub's pile decisions lie within the bound of their
    threshold, z carries no error beyond the chain's own bound, and the bounds are finite"""
    layers, obs, ls, z, err = hl.sampled_case(piles, head)
    S = sum(piles)
    assert len(obs) == hl.sampled_n(piles) and z.shape == (len(obs), S + 2 if head == "piles" else 4)
    for ticks in ((1, 2), range(3, 9)):
        undecided = total = 0
        for tick in ticks:
            d = hl.sampled_definition(piles, head, tick, z, err, ls)
            undecided += int((~d.decided).sum())
            total += d.decided.size
            value, bound = d.logp()
            assert np.isfinite(value).all() and np.isfinite(bound).all() and np.isfinite(d.bound_u).all() and d.bound_u.max() < 1e-3
            if head == "piles":
                assert d.on.any() and not d.on.all(), "both decisions are taken"
        print("%s %s ticks %s: %d of %d pile decisions undecided" % (piles, head, list(ticks), undecided, total))
        assert undecided <= hl.UNDECIDED_CAP * total, (piles, head, undecided, total)


@pytest.mark.parametrize("piles", hl.ALL_HUBS, ids=hl.hub_id)
def test_the_live_case_cannot_hide_a_term(piles):
    """a condition on the DATA, not a measurement: with z the bias exactly, the definition's log-probability bound -- for the full sum and
    for any subset of the piles -- is at most a quarter of the smallest live term, on the ticks the GPU test samples at
    (policy_heads_lib.LIVE_TICKS).  The saturated piles take the certain decision, and with err_z = 0 every pile is decided"""
    S = sum(piles)
    layers, obs, ls, live = hl.live_case(piles)
    assert 3 <= len(live) <= 27 and (np.diff(live) > 0).all() and live[-1] == S - 1 and live[0] == 0
    rs = np.random.RandomState(S)
    for tick in hl.LIVE_TICKS:
        d = hl.live_definition(piles, layers, obs, ls, tick)
        saturated = np.ones(S, dtype=bool)
        saturated[live] = False
        assert np.array_equal(d.on[:, saturated], np.broadcast_to(np.arange(S)[saturated] % 2 == 0, d.on[:, saturated].shape))
        assert d.decided.all(), "with err_z = 0 no decision is within the bound of its threshold"
        bound, term = hl.assert_live_condition(d, layers, live)
        print("%s tick %d: %d live piles, bound %.3g against a smallest term of %.3g" % (piles, tick, len(live), bound, term))
        for share in (0.0, 0.5):
            hl.assert_live_condition(d, layers, live, in_set=rs.rand(len(obs), S) < share)
        # dropping any one live term moves the value by more than the bound
        value, b = d.logp()
        terms = ps.softplus(np.where(d.on, -d.zp, d.zp))[:, live]
        assert (terms.min(axis=1) > 4 * b * (1 - 1e-12)).all()


def test_the_relayout_case_needs_a_second_pass_and_shows_it():
    layers, heads, obs, outs = hl.relayout_case()  # (asserts what it promises)
    assert [W.shape for W, _ in heads] == [(4101, 256)] * 2 and len(outs) == 3 and outs[0].shape == (3, 4101)
    assert not np.array_equal(heads[0][0], heads[1][0])


def test_the_wide_case_is_wider_than_256_and_exact():
    F, layers, obs, norm = hl.wide_case()
    assert F == 316 > 256 and F + hl.WIDE_HIDDEN + 4 <= 512, "it fits the two LDS images with the sampled launch's four rows"
    rs = np.random.RandomState(1)
    car = (rs.rand(hl.WIDE_N, sum(hl.WIDE_HUB)) < 0.5).astype(F32)
    x = hl.wide_normalised(obs, car, norm)
    pl.assert_exact(x, layers)
    a, bound = pl.forward(x, layers, "relu", "clip")
    assert np.array_equal(a.astype(F32).astype(np.float64), a) and len(np.unique(a)) > 8


@pytest.mark.parametrize("T", hl.GAE_T)
@pytest.mark.parametrize("dones", hl.GAE_DONES)
def test_the_gae_blocks_fire_where_their_names_say(T, dones):
    """and the f32 recurrence stays within pile_set_lib's derived bound of the f64 textbook sum on them"""
    for with_final in (False, True):
        packed, values, final = hl.gae_edge_case(T, dones, with_final)
        D = packed.shape[2] - 2
        r, d = packed[:, :, D], packed[:, :, D + 1]
        fired = d != 0
        assert fired.shape == (T, hl.GAE_N) and hl.GAE_N > 256 and hl.GAE_N % 256
        rows = hl.gae_done_rows(T, dones)
        assert not fired[~rows].any()
        k = T - 1 - np.arange(T)
        if dones == "chunk_last":
            assert all(fired[t].any() and not fired[t].all() for t in range(T) if rows[t]) and rows[0]
            assert all(rows[t] for t in range(T) if k[t] % 8 == 7) and rows.sum() == (T // 8 if T % 8 == 0 else T // 8 + 1)
        elif dones == "chunk_first":
            assert all(fired[t].any() and not fired[t].all() for t in range(T) if rows[t]) and rows[T - 1] and rows.sum() == (T + 7) // 8
        elif dones == "pair":
            assert (fired.sum(axis=0) == 2).all() and (np.diff(np.nonzero(fired.T)[1].reshape(-1, 2), axis=1) == 1).all()
            if T > 8:
                assert fired[T - 9, ::2].all() and fired[T - 8, ::2].all(), "the pair straddles the first chunk edge"
        elif dones == "every":
            assert fired.all()
        else:
            assert not fired.any()
        for gamma, lam in psl.GAE_FACTORS:
            a32, r32 = psl.gae_f32(r, d, values, final, gamma, lam)
            a64, r64 = psl.gae_f64(r, d, values, final, gamma, lam)
            ba, br = psl.gae_bound(r, d, values, final, gamma, lam, a32, r32)
            assert (np.abs(a32 - a64) <= ba).all() and (np.abs(r32 - r64) <= br).all(), (T, dones, with_final, gamma, lam)
    assert 7 in hl.GAE_T and 8 in hl.GAE_T and any(t > 8 and t % 8 for t in hl.GAE_T) and any(t > 16 for t in hl.GAE_T)
