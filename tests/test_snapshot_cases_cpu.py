"""The coverage condition of the snapshot tests, on the CPU oracle alone (tests/snapshot_cases_lib.py).

tests/test_gpu_snapshots.py restores snapshots at five moments and compares the continuation.  A continuation can only differ where the
snapshot holds state that matters: with empty queues and nobody to admit, a restore that dropped a flag passes.  So at every named moment
the designed population must hold, on the oracle:

  at least MIN_HITS station units with cars waiting (line > 0): the next step's draws are decoded against a queue;
  at least MIN_HITS envs with a non-empty FCEV waiting list, and on the fcev_stuck case at least MIN_HITS envs whose list is longer than
      the device keeps entry by entry (its folded tail q_fold / q_fold_cnt is state) -- at every moment but right after a reset, which
      empties the list (hy_reset, HYD:197-208): there the counts are asserted to be 0, which is what a restore must bring back;
  at least one car admitted by the step after the moment (the draws made ahead are consumed);
  no overflow of the oracle's own arrays.

The counts are over the whole population of one RNG mode: the tables' traffic is a daytime one, so at the day's end only the hub of 3 + 2
piles still has cars waiting while only the larger hubs admit cars.  At the two moments that are free to choose (mid_day, second_day) the two
[20, 25] cases must hold cars waiting AND admit cars in the same step, each by itself.  These are conditions, not measurements: if a moment
misses one, the moment moves, not the bar.  The counts are printed (pytest -s) and copied into DESIGN 6.15."""
import pytest

import snapshot_cases_lib as sc

MODES = ("philox", "philox_curves")


def population(rng):
    return [name for name, r in sc.CASE_MODES if r == rng]


@pytest.mark.parametrize("rng", MODES)
def test_every_moment_holds_state_that_a_restore_can_get_wrong(rng):
    for moment, p in sc.MOMENTS.items():
        total = {}
        for name in population(rng):
            c = sc.coverage(name, rng, p)
            print("%-14s %-12s p = %3d  %-11s %s" % (rng, moment, p, name, "  ".join("%s %3d" % kv for kv in c.items())))
            for k, v in c.items():
                total[k] = total.get(k, 0) + v
        stuck = sc.coverage(sc.STUCK, rng, p)
        where = (rng, moment, p, total)
        assert total["units_with_line"] >= sc.MIN_HITS, where
        assert total["admitted_next_step"] >= 1, where
        if p == 0:  # a reset leaves no forecourt list: nothing to hold, and a restore must bring exactly that back
            assert total["envs_with_fcev_list"] == 0 and total["envs_with_folded_list"] == 0, where
        else:
            assert total["envs_with_fcev_list"] >= sc.MIN_HITS, where
            assert stuck["envs_with_folded_list"] >= sc.MIN_HITS, (where, stuck)


@pytest.mark.parametrize("rng", MODES)
@pytest.mark.parametrize("name", ["c3", sc.STUCK])
@pytest.mark.parametrize("moment", ["mid_day", "second_day"])
def test_the_free_moments_hold_a_queue_and_admissions_in_one_case(moment, name, rng):
    c = sc.coverage(name, rng, sc.MOMENTS[moment])
    assert c["units_with_line"] >= sc.MIN_HITS and c["admitted_next_step"] >= 1, (name, rng, moment, c)


@pytest.mark.parametrize("name,rng", sc.CASE_MODES)
def test_the_oracle_arrays_do_not_overflow(name, rng):
    assert sc.oracle_trajectory(name, rng).overflow == 0  # (orc_vec_overflow after every step: q_overflow | stay_overflow of any env)


def test_the_script_and_the_moments_are_what_the_gpu_tests_assume():
    assert sc.MOMENTS["after_reset"] == 0 and sc.MOMENTS["at_done"] == 96 and sc.MOMENTS["past_done"] == 97
    assert 0 < sc.MOMENTS["mid_day"] < 96 and sc.PLAN[0] < sc.MOMENTS["second_day"] < sc.TOTAL - 5
    for name, (kw, n, modes) in sc.CASES.items():
        assert 64 <= n <= 130, name
        tr = sc.oracle_trajectory(name, modes[0])
        assert tr.done[95].all() and not tr.done[:95].any(), name  # `done` is the 96th step's, and nothing before it
        acts = sc.action_script(name)
        assert acts.shape == (sc.TOTAL,) + (n, sum(kw["station_list"]) + 2) and (acts[0, :, :-2] == 1).all() and (acts[7, :, :-2] == 1).all()
