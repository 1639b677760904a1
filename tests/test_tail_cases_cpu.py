"""The coverage condition of the designed tail population (tests/tail_cases_lib.py), on the CPU oracle alone: every config reaches the
branches of the tail it was built for.  This is what keeps tests/test_gpu_tail_cases.py from passing while comparing nothing: a GPU
comparison on these env-steps is a comparison on the brim, the hydrogen-limited fuel cell, the wrap of the grid clamp, ..."""
import os
import re

import numpy as np

import orclib
import tail_cases_lib as tc


def test_telemetry_columns_are_the_headers_list():
    hdr = open(os.path.join(orclib.ROOT, "include", "chub.h")).read()
    body = re.search(r"enum \{\s*CHUB_T_HY_ACT = 0,(.*?)\};", hdr, flags=re.S).group(0)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\bCHUB_T_(\w+)", body) == tc.T_NAMES + ["COUNT"]


def test_population_and_script():
    """env i takes config i // 16; the batches have period 8; scripted entries are the script's, free ones differ from env to env"""
    assert tc.N == 96 and len(tc.CONFIGS) == 6 and tc.NAMES == ["brim", "h2_limited", "no_electrolyser", "grid_wrap", "renew_covers", "loss_permeate"]
    rows = tc.rows()
    assert sorted(rows) == sorted(tc.FIELDS) and all(len(v) == tc.N for v in rows.values())
    for k, (name, kw) in enumerate(tc.configs()):
        assert kw["station_list"] == [64, 64] and kw["station_type_list"] == ["fast", "fast"] and kw["constant_charging"] is False
        for f in tc.FIELDS:
            assert rows[f][16 * k:16 * k + 16] == [kw[f]] * 16, (name, f)
    b = tc.action_batches()
    assert b.shape == (8, 96, 130) and b.dtype == np.float32 and np.abs(b).max() <= 1.0
    for t in (0, 7, 8, 95, 96, 135):
        assert tc.actions(t) is not None and np.array_equal(tc.actions(t), b[t % 8])
    el, fc, piles = b[:, :, 128], b[:, :, 129], b[:, :, :128]
    blk = lambda k: slice(16 * k, 16 * k + 16)
    assert (el[:, blk(0)] == 1).all() and (el[:, blk(1)] == -1).all() and (fc[:, blk(1)] == 1).all()
    assert (el[:, blk(3)] == 0.5).all() and (el[:, blk(4)] == np.float32(-0.9)).all() and (fc[:, blk(4)] == -1).all()
    assert (piles[:, blk(1)] == 1).all() and (piles[:, blk(3)] == 1).all()
    for k in (0, 2, 4, 5):
        assert len(np.unique(piles[:, blk(k)])) > 8 * 16 * 100  # free
    for k in (2, 5):
        assert len(np.unique(el[:, blk(k)])) == 128 and len(np.unique(fc[:, blk(k)])) == 128


def test_classifier_on_hand_made_rows():
    """the flags on telemetry rows written by hand from their definitions"""
    z = np.zeros(38)

    def row(**kw):
        r = z.copy()
        for name, v in kw.items():
            r[tc.T[name]] = v
        return r

    on = lambda f: {k for k in tc.FLAGS if f[k]}
    # electrolyser action 0.5 -> 0.75 requested and run: not clamped; the grid pays; the electrolyser runs (no fuel cell)
    assert on(tc.classify(row(HY_ACT=0.75, HY_FLOW_SPEED=2.0, ALL_POWER_SECOND=300.0, HYDROGEN_POWER=120.0, STORE_SOC=0.5), 0.5, 0.0, 100.0)) == {"grid_pays"}
    # ... clamped to index 0 of the table, which wraps to full power
    assert on(tc.classify(row(HY_ACT=1.0, HY_FLOW_SPEED=2.0, ALL_POWER_SECOND=300.0, HYDROGEN_POWER=120.0, STORE_SOC=0.5), 0.5, 0.0, 100.0)) == {"clamp", "grid_wrap", "grid_pays"}
    assert on(tc.classify(row(HY_ACT=0.31, HY_FLOW_SPEED=2.0, ALL_POWER_SECOND=300.0, HYDROGEN_POWER=120.0, STORE_SOC=0.5), 0.5, 0.0, 100.0)) == {"clamp", "grid_pays"}
    # full power asked for and run is no clamp
    assert on(tc.classify(row(HY_ACT=1.0, HY_FLOW_SPEED=0.0, STORE_SOC=1.0), 1.0, 0.0, 100.0)) == {"brim", "no_gen"}
    # the brim: only the compressor's trickle, renewables cover it, the fuel cell takes what the chargers still draw
    assert on(tc.classify(row(HY_ACT=1.0, HY_FLOW_SPEED=0.001, ALL_POWER_SECOND=0.01, STORE_SOC=1.0, FC_POWER=40.0, HY_TO_USE=40.0 * 1500 / 119.6),
                          1.0, 0.3, 100.0)) == {"brim", "no_gen", "renew_covers", "fc_on", "fc_takes_all"}
    # the fuel cell at its maximum, then short of hydrogen, the tank at its floor with demand unmet
    assert on(tc.classify(row(STORE_SOC=0.1, FC_POWER=1000.0, HY_TO_USE=100.0, NOT_MEET=3.0, EV_SUM_NET=50.0), -1.0, 1.0, 1000.0)) == {
        "floor", "not_meet", "no_gen", "fc_on", "fc_at_max", "h2_limited"}
    # vectorised: leading shape kept
    f = tc.classify(np.stack([row(STORE_SOC=1.0), row(STORE_SOC=0.1)]), np.float32([-1, -1]), np.float32([0, 0]), np.array([100.0, 100.0]))
    assert f["brim"].tolist() == [True, False] and f["floor"].tolist() == [False, True]


def test_every_config_reaches_its_branches_on_the_oracle(capsys):
    tr = tc.oracle_trajectory()
    counts, steps = tc.branch_counts(tr)
    assert steps == 136 * 16
    with capsys.disabled():
        print("\nbranch hits on the oracle, env-steps of %d per config (PHILOX, seed %#x, env_id0 %d, action seed %d):" % (steps, tc.SEED, tc.ENV_ID0, tc.ACTION_SEED))
        for name in tc.NAMES:
            print("  %-16s %s" % (name, "  ".join("%s %d" % (f, counts[name][f]) for f in tc.FLAGS)))
    assert tr.q_overflow == 0
    assert tr.done[95].all() and not tr.done[:95].any() and not tr.done[96:].any()
    for name, need in tc.MUST_REACH.items():
        for flag, least in need.items():
            got = counts[name][flag]
            if least == "every":
                assert got == steps, (name, flag, got)
            elif least == "half":
                assert 2 * got > steps, (name, flag, got)
            else:
                assert least == 4 and got >= least, (name, flag, got)
    assert set(tc.MUST_REACH) == set(tc.NAMES)
    # the flags the table names, no fewer
    assert {f for need in tc.MUST_REACH.values() for f in need} == {"brim", "renew_covers", "fc_takes_all", "h2_limited", "fc_at_max", "floor", "no_gen",
                                                                  "not_meet", "fc_on", "clamp", "grid_wrap", "grid_pays"}
