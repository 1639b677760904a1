"""The cases of tests/test_gpu_grid_pass.py are the right ones, by arithmetic (tests/grid_pass_lib.py), for devices of 64, 256 and 304
compute units: the population's tile order is a permutation whose XCD runs are contiguous and every population case permutes; every long
moments case makes a second loop trip and one a third, partial one; the wide mask outnumbers a grid pass; P = 2100 is under the chunk
cap; and at every R used the definition's bound on the mean is small enough to see one row missing.  No GPU needed."""
import numpy as np

import grid_pass_lib as gpl
from test_gpu_normalizer import columns  # (a function of numpy alone)


def test_the_tile_order_is_a_permutation_of_contiguous_runs():
    for nb in range(2, 4097, 2):
        tiles = [int(t) for t in gpl.tile_of(np.arange(nb), nb)]
        assert sorted(tiles) == list(range(nb)), nb
        at = 0
        for x, run in enumerate(gpl.xcd_runs(nb)):
            assert run == list(range(at, at + len(run))), (nb, x, "one contiguous run, in the order of x")
            assert len(run) == nb // 8 + (x < nb % 8)
            at += len(run)
        if nb <= 8:
            assert tiles == list(range(nb)), "the identity up to 8 workgroups: what every earlier test launched"


def test_every_population_case_permutes():
    seen_r, straddles = set(), 0
    for P, E in gpl.POP_CASES:
        nb, tpm = gpl.pop_grid(P, E)
        assert P % 2 == 0 and nb % 2 == 0 and nb > 8
        tiles = [int(gpl.tile_of(b, nb)) for b in range(nb)]
        assert tiles != list(range(nb)) and sum(t != b for b, t in enumerate(tiles)) >= nb // 2, (P, E, "a non-identity map")
        seen_r.add(nb % 8)
        # the member of a permuted tile: some workgroup serves another member than the identity map would give it
        assert any(t // tpm != b // tpm for b, t in enumerate(tiles)), (P, E)
        runs = gpl.xcd_runs(nb)
        for m in range(P):
            owners = set(x for x, run in enumerate(runs) for t in run if t // tpm == m)
            straddles += len(owners) > 1
        # the mask: around the first tile of XCD 1's run, a member's first tile, inside the batch; both sides of the edge are named
        t = gpl.edge_tile(P, E)
        assert t == runs[1][0] and t % tpm == 0 and t >= 1 and 32 * t + 7 <= P * E
        mask = gpl.edge_mask(P, E)
        assert mask.sum() == 13 and mask[32 * t - 5] and mask[32 * t + 6] and not mask[32 * t - 6] and not mask[32 * t + 7] and mask[-1]
        assert (32 * t - 1) // E != (32 * t) // E, "a member's edge"
    assert [gpl.pop_grid(P, E)[0] for P, E in gpl.POP_CASES] == [10, 16, 12, 18, 22, 70]
    assert [gpl.pop_grid(P, E)[1] for P, E in gpl.POP_CASES] == [1, 1, 2, 3, 1, 1]
    assert seen_r == {0, 2, 4, 6}
    assert straddles >= 1, "a member whose tiles lie in two XCD runs"
    assert set(gpl.POP_PERTURB) <= set(gpl.POP_CASES) and gpl.POP_OWN_HANDLE[0] in gpl.POP_CASES
    assert max(gpl.POP_OWN_HANDLE[1]) == gpl.POP_OWN_HANDLE[0][0] - 1


def test_the_moments_shape_is_the_librarys():
    """against the figures of DESIGN.md 6.21 and the lane layout's edges"""
    assert gpl.moments_shape(1, 256) == (1, 256, 1024) and gpl.moments_shape(64, 256) == (64, 4, 1024)
    assert gpl.moments_shape(128, 256)[:2] == (128, 2) and gpl.moments_shape(129, 256)[:2] == (129, 1)
    assert gpl.moments_shape(255, 256)[:2] == (255, 1) and gpl.moments_shape(256, 256)[:2] == (256, 1) and gpl.moments_shape(257, 256)[:2] == (256, 1)
    # the 4 MiB of partials cap the grid at F = 257 (above 254 compute units) and at F = 512 (above 127)
    assert gpl.moments_shape(257, 256)[2] == 1018 == gpl.moments_shape(257, 304)[2] and gpl.moments_shape(257, 64)[2] == 256
    assert gpl.moments_shape(512, 256)[2] == 511 == gpl.moments_shape(512, 304)[2] and gpl.moments_shape(512, 64)[2] == 256
    assert gpl.moments_shape(256, 304)[2] == 1022 and gpl.moments_shape(255, 304)[2] == 1026 and gpl.moments_shape(64, 304)[2] == 1216


def test_every_long_case_makes_a_second_trip_and_one_a_third_partial_one():
    for cus in gpl.CUS:
        for F in gpl.LONG_F:
            _, rw, grid = gpl.moments_shape(F, cus)
            R = gpl.long_rows(rw, grid)
            assert R % gpl.MOMENTS_N == 0 and R > gpl.AHEAD * grid * rw + 257
            assert gpl.trips(R, F, cus) == 2 == gpl.trips_of(R, rw, grid), (cus, F, R)
            assert gpl.launch_of(R, rw, grid)[1] == grid
            # trip 0 is whole for everybody; workgroup 0's trip 1 starts inside R and ends past it; nobody makes a third
            assert all(all(gpl.live_of(R, rw, grid, b, 0)) for b in (0, grid // 2, grid - 1))
            second = gpl.live_of(R, rw, grid, 0, 1)
            assert second[0] and not second[-1] and gpl.live_of(R, rw, grid, 0, 2) is None
        _, rw, grid = gpl.moments_shape(gpl.RAGGED_F, cus)
        R = gpl.ragged_rows(rw, grid)
        assert R % gpl.MOMENTS_N == 0 and gpl.trips(R, gpl.RAGGED_F, cus) == 3
        assert all(gpl.live_of(R, rw, grid, grid - 1, 1)), "the second trip is whole"
        last = gpl.live_of(R, rw, grid, 0, 2)
        assert last == [True] + [False] * 7, (cus, "the last trip: some k live and some not", last)
        assert gpl.live_of(R, rw, grid, grid - 1, 2) is None, "and only the first workgroups make it"


def test_the_wide_mask_outnumbers_a_grid_pass_and_the_edge_rows_pass_the_grid():
    for cus in gpl.CUS:
        for F in gpl.WIDE_F:
            _, rw, grid = gpl.moments_shape(F, cus)
            N, R = gpl.wide_envs(rw, grid), gpl.wide_rows(rw, grid)
            blocks = gpl.launch_of(R, rw, grid)[1]
            assert N > grid * rw and N % 10 == 0 and R % N == 0
            assert blocks * rw < N, "e_step = blocks RW is not reduced: the walk's one subtraction has to be enough"
            assert gpl.AHEAD * blocks * rw > N, "and the walk does wrap within a trip"
        for F in gpl.EDGE_F:
            _, rw, grid = gpl.moments_shape(F, cus)
            rows = gpl.edge_rows(rw, grid)
            assert rows[:2] == (1, 257) and rows[2] % gpl.MOMENTS_N == 0 and grid * rw + 257 <= rows[2] < grid * rw + 257 + gpl.MOMENTS_N
    for N in (gpl.MOMENTS_N, 1420, 5000):
        mask = gpl.random_mask(N, 5)
        assert not mask[0] and mask[1] and 0.4 * N < mask.sum() < 0.8 * N


def test_the_chunk_cap_binds_at_p_2100():
    D, A = 2 + 4 * 2 + 3, sum(gpl.ES_HUB) + 2
    shapes = [(33, D), (A, 33)]
    items = gpl.es_items(shapes)
    assert items == 33 * 4
    cp, chunks = gpl.es_chunks(gpl.ES_P, items)
    pairs = gpl.ES_P // 2
    assert (cp, chunks) == (17, 62), "1050 pairs: 66 chunks of 16 are capped at 64, which makes 17 pairs a chunk and so 62 chunks"
    assert cp > gpl.CHUNK_PAIRS and 0 < pairs - (chunks - 1) * cp < cp, "a shorter last chunk"
    # what the earlier tests launched: one chunk size never above 16, the cap never reached
    assert [gpl.es_chunks(P, 33 * 4) for P in (6, 64, 70)] == [(3, 1), (16, 2), (12, 3)]
    assert gpl.es_chunks(2048, items) == (16, 64) and gpl.es_chunks(2050, items)[0] == 17


def test_the_mean_bound_sees_one_row_missing_at_every_r():
    """at the largest device size, where R and so the bound are largest: leaving out any one of at least 98 % of the counted rows moves the
    mean of some column by more than twice the bound on it (twice: a second update onto a state of the same size halves the move)"""
    cus = max(gpl.CUS)
    cases = [(F, gpl.long_rows(*gpl.moments_shape(F, cus)[1:]), gpl.MOMENTS_N) for F in gpl.LONG_F]
    cases.append((gpl.RAGGED_F, gpl.ragged_rows(*gpl.moments_shape(gpl.RAGGED_F, cus)[1:]), gpl.MOMENTS_N))
    cases += [(F, gpl.wide_rows(*gpl.moments_shape(F, cus)[1:]), gpl.wide_envs(*gpl.moments_shape(F, cus)[1:])) for F in gpl.WIDE_F]
    cases += [(F, R, gpl.MOMENTS_N) for F in gpl.EDGE_F for R in gpl.edge_rows(*gpl.moments_shape(F, cus)[1:])[1:]]
    for F, R, N in cases:
        x = gpl.moments_batch(columns, F, R, 0, own_last=F == 257)
        masks = [None] if R % N else [None, gpl.random_mask(N, F)]
        for mask in masks:
            rows = None if mask is None else mask[np.arange(R) % N]
            ratio = gpl.drop_one_row(x, rows)
            seen = (ratio > 2).mean()
            print("F %d R %d %s: one row missing moves a mean by more than twice its bound for %.4f of the rows (median %.3g bounds)" %
                  (F, R, "masked" if mask is not None else "all", seen, np.median(ratio)))
            assert seen >= 0.98, (F, R, seen)
