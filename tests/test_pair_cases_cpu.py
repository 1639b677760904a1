"""The coverage conditions of the populations for the paired tail launch (tests/pair_cases_lib.py), on the CPU oracle alone, and the pair rule
the GPU tests rely on.  This is what keeps tests/test_gpu_pair_cases.py from passing while comparing nothing: every branch, forecourt state and
lane order it claims to hold to the oracle is reached at the steps that occupy BOTH positions of a pair."""
import ctypes as C

import numpy as np
import pytest

import pair_cases_lib as pc
import tail_cases_lib as tc

HANDLE, CALL, STEPS = 0, 1, 2  # CHUB_PAIR_* (include/chub.h)


def test_population_and_script():
    assert pc.N == 96 and pc.K == 6 and pc.BLOCK == 16 and pc.PERIOD == 8 and pc.PLAN == (96, 40) and pc.MIN_HITS == 4
    assert pc.HUB is tc.HUB and pc.classify is tc.classify and pc.flags_of is tc.flags_of  # imported, not copied
    for name, kw in pc.configs():
        assert kw["station_list"] == [64, 64] and kw["station_type_list"] == ["fast", "fast"] and kw["constant_charging"] is False
    b = pc.action_batches()
    assert b.shape == (8, 96, 130) and b.dtype == np.float32 and np.abs(b).max() <= 1.0
    el, fc, piles = b[:, :, 128], b[:, :, 129], b[:, :, :128]
    blk = lambda k: slice(16 * k, 16 * k + 16)
    assert (el[:, blk(0)] == 1).all() and (fc[:, blk(1)] == 1).all() and (fc[:, blk(2)] == 1).all() and (el[:, blk(3)] == 0.5).all()
    assert [int(v) for v in el[:, 16]] == [1, -1, -1, 1, -1, -1, -1, 1]                      # h2_limited: the tank leaves its floor and returns
    assert [int(v) for v in piles[:, blk(3)].max(axis=(1, 2))] == [-1, 1, -1, -1, -1, -1, 1, 1]  # grid_wrap: piles all off / all on
    assert [int(v) for v in piles[:, blk(3)].min(axis=(1, 2))] == [-1, 1, -1, -1, -1, -1, 1, 1]
    for k in (0, 2, 4, 5):
        assert len(np.unique(piles[:, blk(k)])) > 8 * 16 * 100  # free


def test_both_positions_and_calls():
    """the steps that are a pair's first step in one alignment and its second in the other, worked out from the calls themselves"""
    first, second = {"even": set(), "odd": set()}, {"even": set(), "odd": set()}
    for align in ("even", "odd"):
        calls = pc.alignment_calls(align)
        assert [c for c in calls if c[1] not in (1, 2)] == []
        assert sorted(i for f, c in calls for i in range(f, f + c)) == list(range(136))
        for f, c in calls:
            if c == 2:
                first[align].add(f)
                second[align].add(f + 1)
                assert f // 96 == (f + 1) // 96  # a pair never straddles the day's end
    assert pc.alignment_calls("even")[:2] == [(0, 2), (2, 2)] and pc.alignment_calls("even")[47:49] == [(94, 2), (96, 2)]
    assert pc.alignment_calls("odd")[:3] == [(0, 1), (1, 2), (3, 2)] and pc.alignment_calls("odd")[47:51] == [(93, 2), (95, 1), (96, 1), (97, 2)]
    assert pc.alignment_calls("odd")[-2:] == [(133, 2), (135, 1)]
    both = (first["even"] & second["odd"]) | (first["odd"] & second["even"])
    assert sorted(both) == list(np.nonzero(pc.both_positions())[0]) == list(range(1, 95)) + list(range(97, 135))
    assert sorted(first["even"] | first["odd"]) == list(pc.pair_firsts())
    assert pc.chain_calls("even", 8)[:2] == [(0, 8), (8, 8)] and pc.chain_calls("even", 14)[6:8] == [(84, 12), (96, 14)]
    assert pc.chain_calls("odd", 8)[:3] == [(0, 1), (1, 8), (9, 8)] and pc.chain_calls("odd", 8)[12:15] == [(89, 7), (96, 1), (97, 8)]
    # every chain call ends where a call of the same alignment's calls of two ends: that is where their states are compared
    for align in ("even", "odd"):
        ends = {f + c - 1 for f, c in pc.alignment_calls(align)}
        for length in (8, 14):
            assert {f + c - 1 for f, c in pc.chain_calls(align, length)} <= ends


def pair_plan(kw, n, t, left, **options):
    import charginghub_env_amd as m
    from charginghub_env_amd import _lib
    cfg = m.make_config(kw["station_list"], kw["station_type_list"], **{f: v for f, v in kw.items() if f not in ("station_list", "station_type_list")})
    opt = _lib.ChubOptions()
    for f, v in options.items():
        setattr(opt, f, v)
    out = (C.c_int64 * 3)()
    assert m.load_library().chub_pair_plan(C.byref(cfg), n, _lib.RNG_PHILOX, C.byref(opt), 0, 0, t, left, out) == 0
    return list(out)


def test_paired_steps_is_the_librarys_rule():
    """pc.paired_steps (what the GPU tests intend) against chub_pair_plan on the handles they make, for every call they issue"""
    kw = pc.configs()[0][1]
    calls = {(f % 96 if f < 96 else f - 96, c) for align in ("even", "odd") for length in (2, 8, 14) for f, c in pc.chain_calls(align, length)}
    calls |= {(1, 2), (3, 6), (10, 4), (0, 1)}
    for t, c in sorted(calls):
        assert pair_plan(kw, 16, t, c, fused_step=1, span_steps=2) == [1, 1, pc.paired_steps(t, c)], (t, c)
    assert [pc.paired_steps(*a) for a in ((0, 1), (0, 2), (1, 2), (95, 1), (89, 7), (3, 6), (94, 8))] == [0, 2, 2, 0, 6, 6, 2]
    assert pair_plan(kw, 16, 1, 2, fused_step=1, span_steps=1)[HANDLE] == 0  # the pairs-off side
    for name in pc.XCD_HUBS:
        for n in pc.XCD_SIZES:
            assert pair_plan(pc.XCD_HUBS[name], n, 3, 6, fused_step=1, span_steps=2) == [1, 1, 6]


def test_every_config_reaches_its_branches_at_both_positions(capsys):
    tr = pc.oracle_trajectory()
    counts, flips = pc.branch_counts(tr), pc.flip_counts(tr)
    with capsys.disabled():
        print("\nbranch hits on the oracle at the %d steps that occupy both positions of a pair, env-steps of %d per config:" % (
            pc.both_positions().sum(), pc.both_positions().sum() * pc.BLOCK))
        for name in pc.NAMES:
            print("  %-16s %s" % (name, "  ".join("%s %d" % (f, counts[name][f]) for f in pc.FLAGS)))
        print("  pairs (on, off) / (off, on): %s" % "  ".join("%s.%s %d / %d" % (n, f, a, b) for (n, f), (a, b) in flips.items()))
    assert tr.q_overflow == 0
    assert tr.done[95].all() and not tr.done[:95].any() and not tr.done[96:].any()
    assert set(pc.MUST_REACH) == set(pc.NAMES)
    for name, flags in pc.MUST_REACH.items():
        for flag in flags:
            least = pc.GRID_WRAP_MIN if flag == "grid_wrap" else pc.MIN_HITS
            assert least == 4 and counts[name][flag] >= least, (name, flag, counts[name][flag])
    assert {f for flags in pc.MUST_REACH.values() for f in flags} == {"brim", "floor", "h2_limited", "fc_at_max", "fc_takes_all", "fc_on", "not_meet", "no_gen",
                                                                     "clamp", "grid_wrap", "renew_covers", "grid_pays"}
    assert {f for _, f in pc.MUST_FLIP} == {"brim", "floor", "clamp"}
    for key, (on_off, off_on) in flips.items():
        assert on_off >= pc.MIN_HITS and off_on >= pc.MIN_HITS, (key, on_off, off_on)
    # no_gen on every step of the hub without an electrolyser
    k = pc.NAMES.index("no_electrolyser")
    assert tr.flags["no_gen"][:, k * 16:(k + 1) * 16].all()


def test_the_forecourt_builds_a_line_a_list_and_double_arrivals(capsys):
    tr = pc.forecourt_trajectory()
    c = pc.forecourt_counts(tr)
    with capsys.disabled():
        print("\nforecourt (fcev_stuck, 16 envs, seed 31, 96 + 12 steps), env-steps at both positions: %s" % c)
    assert tr.q_overflow == 0
    assert c["line"] >= pc.MIN_HITS and c["queue"] >= pc.MIN_HITS and c["arrivals2"] >= pc.MIN_HITS
    assert c["max_line"] >= 2 and c["max_queue"] > c["max_line"]  # a list beyond the line: the folded tail is state


@pytest.mark.parametrize("n", pc.XCD_SIZES)
@pytest.mark.parametrize("name", list(pc.XCD_HUBS))
def test_envs_of_an_eighth_differ_from_one_another(name, n):
    """a lane sent to another env of its own eighth -- or of any other -- cannot leave what the right env leaves"""
    tr = pc.xcd_trajectory(name, n)
    assert tr.q_overflow == 0 and n % 2048 == 0
    assert pc.distinct_in_every_eighth(tr, n, step=2) == [0] * 8
    rows = np.concatenate([tr.slots[k][2].reshape(n, -1) for k in (0, 1)], axis=1)
    assert len(np.unique(np.ascontiguousarray(rows).view(np.uint32), axis=0)) == n  # ... nor across eighths
