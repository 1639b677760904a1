"""The cases of tests/test_gpu_grad_trips.py are the right ones, by arithmetic and through the host-only plans: at R2 and R3 every net used
gets 512 workgroups (one, the byte-capped actor, 488) whose trips through k_policy_grad's and k_critic's walk are two and three, unequal,
with a partial last tile; every exact case meets its exactness condition per workgroup; every general case's data meet the conditions
under which the derived bar means something; a restatement that loses whole tiles leaves that bar; and the byte cap on the workgroups is
out of a critic's reach and within a PILES actor's.  No GPU needed."""
import itertools

import numpy as np

import critic_lib as cl
import grid_pass_lib as gpl
import policy_grad_lib as pgl

R2, R3 = gpl.GRAD_R2, gpl.GRAD_R3
EXACT_NETS = ((1, cl.EXACT_HIDDEN), (2, cl.EXACT_HIDDEN), (3, cl.EXACT_HIDDEN), (4, cl.EXACT_HIDDEN), (3, cl.EXACT_WIDE))


def critic_plan_of(c):
    rc, p, msg = cl.plan(c.F, c.sizes[1:], c.R, c.act)
    assert rc == 0, msg
    return p


def test_the_walk_restated():
    assert (R2, R3) == (16455, 32871) and (gpl.grad_tiles(R2), gpl.grad_tiles(R3)) == (515, 1028)
    assert gpl.grad_blocks(R2) == gpl.grad_blocks(R3) == 512 and gpl.grad_blocks(300) == 16 and gpl.grad_blocks(16384) == 512
    assert gpl.grad_trips(300, 16).tolist() == [1] * 10 + [0] * 6, "what every earlier test launched: no second trip"
    assert gpl.grad_trips(16384, 512).max() == 1 and gpl.grad_trips(16385, 512).tolist() == [2] + [1] * 511
    assert gpl.grad_trips(R2, 512).tolist() == [2] * 3 + [1] * 509
    assert gpl.grad_trips(R3, 512).tolist() == [3] * 4 + [2] * 508
    # the values call: up to 1024 workgroups
    assert gpl.value_blocks(R2) == 520 and gpl.grad_trips(R2, 520).tolist() == [1] * 515 + [0] * 5
    assert gpl.value_blocks(R3) == 1024 and gpl.grad_trips(R3, 1024).tolist() == [2] * 4 + [1] * 1020
    for R in (R2, R3):
        assert R % 32 == 7, "a partial last tile of 7 rows"
        trip, wg = gpl.grad_trip_of(R, 512)
        assert np.array_equal(np.bincount(wg * 4 + trip, minlength=2048).reshape(512, 4).astype(bool).sum(axis=1), gpl.grad_trips(R, 512))
        parts = [gpl.grad_trip_positions(R, 512, t) for t in range(trip.max() + 1)]
        assert np.array_equal(np.sort(np.concatenate(parts)), np.arange(R)) and [len(p) for p in parts][:2] == [16384, min(R - 16384, 16384)]
        last = gpl.grad_last_trip(R, 512)
        assert last[-1] and not last[0] and last.sum() == R - 32 * (gpl.grad_tiles(R) - 512)
        by = gpl.grad_by_workgroup(np.arange(1, R + 1, dtype=np.float64)[:, None], 512)
        assert by.shape == (512, 32 * (trip.max() + 1), 1) and by[2, 32, 0] == (512 + 2) * 32 + 1 and by.sum() == R * (R + 1) / 2


def test_every_net_gets_512_workgroups_and_the_stated_trips():
    seen = set()
    for c, tpw in cl.trip_general_cases():
        p = critic_plan_of(c)
        rows, pairs, part = gpl.grad_shape(c.sizes)
        assert p["workgroups"] == 512 == gpl.grad_blocks(c.R, part) and p["lds_rows"] == rows and p["in_registers"] == (pairs <= gpl.GRAD_REG_PAIRS)
        assert tpw == gpl.grad_trips(c.R, 512).max() == {R2: 2, R3: 3}[c.R]
        seen.add((c.R, p["in_registers"]))
    assert (R2, 0) in seen and (R2, 1) in seen and (R3, 1) in seen
    for n_layers, hidden in EXACT_NETS:
        for R in (R2, R3):
            sizes = [cl.EXACT_F] + list(hidden[:n_layers - 1]) + [1]
            rc, p, msg = cl.plan(sizes[0], sizes[1:], R, "relu")
            assert rc == 0 and p["workgroups"] == 512 and (p["in_registers"] == 0) == (hidden == cl.EXACT_WIDE), msg
            rc, p, msg = pgl.plan([20, 25], list(hidden[:n_layers - 1]) + [4], R, "loads", "relu")
            assert rc == 0 and p["workgroups"] == 512 and (p["in_registers"] == 0) == (hidden == pgl.EXACT_WIDE), msg
    capped = 0
    for c, tpw in pgl.trip_general_cases():
        blocks = pgl.blocks_of(c)
        sizes = [c.features.shape[1]] + [W.shape[0] for W, _ in c.layers]
        assert blocks == gpl.grad_blocks(c.R, gpl.grad_shape(sizes)[2]) and tpw == gpl.grad_trips(c.R, blocks).max() == {R2: 2, R3: 3}[c.R]
        if blocks != 512:
            capped += 1
            assert blocks == pgl.CAPPED_BLOCKS and c.R == R2 and gpl.grad_trips(R2, blocks).tolist() == [2] * 27 + [1] * 461
        # every stored row is met in every trip
        trip = gpl.grad_trip_of(c.R, blocks)[0]
        assert all(len(np.unique(c.rows[trip == t])) == 95 for t in range(tpw - 1))
    assert capped == 1


def test_the_exact_cases_are_exact_per_workgroup():
    """the critic's cases meet the condition over all rows, as at R = 300; the actor's deeper cases at R3 pass 2^23 quanta over all rows
    and stay far below it over a workgroup's own rows, which is all an f32 chain covers"""
    over_all = []
    for n_layers, hidden in EXACT_NETS:
        for R in (R2, R3):
            for loss in ("mse", "clipped"):
                c = cl.exact_case(n_layers, R, loss, hidden=hidden)  # (asserts)
                assert c.R == R and c.rows is None
            c = pgl.exact_case(n_layers, R, hidden=hidden, blocks=512)  # (asserts, per workgroup)
            r = pgl.restate(c)
            lp, en, stats = pgl.exact_forward(c, r)
            assert np.abs(lp - r["logp"]).max() <= r["bar_logp"].max() and np.abs(en - r["ent"]).max() <= r["bar_ent"].max()
            assert stats[0] == R and np.all(np.abs(stats - r["stats"]) <= r["bar_stats"] + 1e-9 * np.abs(r["stats"]))
            try:
                pgl.assert_exact(c)
            except AssertionError:
                over_all.append((n_layers, R))
    assert over_all and all(R == R3 for _, R in over_all), over_all


def test_the_general_cases_meet_their_conditions_and_see_whole_tiles_missing():
    for lib in (cl, pgl):
        for c, tpw in lib.trip_general_cases():
            blocks = pgl.blocks_of(c) if lib is pgl else critic_plan_of(c)["workgroups"]
            r = lib.restate(c, tpw)
            lib.check_conditions(c, r)
            for mistake in lib.TRIP_MISTAKES:
                assert lib.outside_bar(r, lib.restate(c, tpw, mistake, blocks=blocks)), (c.name, mistake)
    # the "mixed" lists carry indices outside the arrays and repeats into the later trips and the partial last tile
    mixed = [c for c, _ in cl.trip_general_cases() if c.rows is not None]
    assert len(mixed) == 4
    for c in mixed:
        trip = gpl.grad_trip_of(c.R, 512)[0]
        bad = (c.rows < 0) | (c.rows >= len(c.x))
        assert all(bad[trip == t].sum() >= 2 for t in range(trip.max() + 1)) and bad[c.R - 7:].any() and not bad[c.R - 7:].all()
        assert all(len(np.unique(c.rows[trip == t])) < (trip == t).sum() for t in range(trip.max() + 1))


def test_the_parts_of_a_call_by_trip():
    for loss in ("coef", "ppo_clip"):
        c, tpw = pgl.trip_parts_case(loss)
        pgl.check_conditions(c, pgl.restate(c, tpw))
        assert c.loss == loss and c.R == R3 and pgl.blocks_of(c) == 512
        for cm in pgl.trip_parts(c, 512):
            assert np.array_equal(pgl.separate_ratios(cm).logp_old, c.logp_old), "no part puts a ratio on a bound"
    for lib in (cl, pgl):
        c = [c for c, _ in lib.trip_general_cases() if c.R == R3][0]
        parts = lib.trip_parts(c, 512)
        assert [p.R for p in parts] == [16384, 16384, 103]
        base = np.arange(c.R) if c.rows is None else c.rows
        assert np.array_equal(np.sort(np.concatenate([p.rows for p in parts])), np.sort(base))
        assert np.array_equal(parts[1].rows[:32], base[512 * 32:513 * 32]) and np.array_equal(parts[2].rows[-7:], base[-7:])


def test_the_byte_cap_is_out_of_a_critics_reach_and_within_a_piles_actors():
    """grad_blocks also caps the workgroups so that the f32 partials stay within 256 MiB: fewer than 512 from 128 dW tiles on.  Only tile
    counts matter, so the widths 32 k are every case.  A critic (and a LOADS actor: one head tile) that the LDS rule accepts has at most
    126 dW tiles; a PILES head of many piles has as many output tiles as its widest input and passes 128"""
    most, accepted = 0, 0
    for f in range(1, 17):
        for hid in itertools.chain.from_iterable(itertools.product(range(1, 9), repeat=n) for n in range(4)):
            sizes = [32 * f] + [32 * h for h in hid] + [1]
            rows, pairs, part = gpl.grad_shape(sizes)
            rc, p, msg = cl.plan(sizes[0], sizes[1:], R3)
            assert (rc == 0) == (rows <= gpl.GRAD_LDS_ROWS), (sizes, rc, msg)
            if rc == 0:
                accepted += 1
                most = max(most, pairs)
                assert p["workgroups"] == 512 == gpl.grad_blocks(R3, part), sizes
                rc, p, msg = pgl.plan([20, 25], sizes[1:-1] + [4], R3, "loads")  # (F = 13: fewer tiles still)
                assert rc == 0 and p["workgroups"] == 512, msg
    assert accepted > 6000 and most == 126
    assert gpl.grad_blocks(R3, 126 * 1024 + 32 * 25) == 512 and gpl.grad_blocks(R3, 128 * 1024 + 32) == 504
    # PILES: S piles, one column per pile beside the observation, no hidden layer
    reached = {}
    for S in range(32, 640, 32):
        sizes = [13 + S, S + 2]
        rows, pairs, part = gpl.grad_shape(sizes)
        rc, p, msg = pgl.plan([S // 2, S - S // 2], sizes[1:], R3, "piles", "tanh", pgl.CAPPED_INPUTS)
        if rc == 0:
            assert rows <= gpl.GRAD_LDS_ROWS and p["workgroups"] == gpl.grad_blocks(R3, part), (S, p)
            reached[S] = p["workgroups"]
    assert reached[320] == 512 and min(reached.values()) < 512
    rc, p, msg = pgl.plan(pgl.TRIP_CAPPED[0], [352], R3, "piles", "tanh", pgl.CAPPED_INPUTS)
    assert rc == 0 and p["workgroups"] == pgl.CAPPED_BLOCKS == gpl.grad_blocks(R3, gpl.grad_shape([pgl.CAPPED_F, 352])[2]) and p["in_registers"] == 0
