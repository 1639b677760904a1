"""Constrained PPO's host-only parts (include/chub.h, "constrained PPO on the device") and its numpy restatement tests/lagrange_lib.py,
without a device: the symbols, enums and structs; the restated cost GAE against chub_rollout_gae_device's restatement and the f64 textbook
sum; the episode sums against a plain forward loop in exact rationals; the carry across calls; chub_lagrange_fold bit for bit on made stats;
the refusals that need no device; and the failure experiment: every wrong= variant differs on a named case of the GPU test's lists."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import lagrange_lib as ll
import pile_set_lib as psl

ERR_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["chub_policy_collect_terms", "chub_lagrange_create", "chub_lagrange_destroy", "chub_lagrange_gae_device", "chub_lagrange_step_device",
       "chub_lagrange_combine_device", "chub_lagrange_device", "chub_lagrange_read", "chub_lagrange_set_lambda_device", "chub_lagrange_state_size",
       "chub_lagrange_get_state", "chub_lagrange_set_state", "chub_lagrange_fold"]
STEPS = ll.step_cases()
BY_NAME = {c["name"]: c for c in ll.GAE_CASES}


def lib():
    from charginghub_env_amd import _lib
    return _lib.load_library()


def last_error():
    return lib().chub_last_error().decode()


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def struct_fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?=,|$)", decl.strip())]


def test_header_device_header_and_binding_agree():
    from charginghub_env_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "chub.h")).read()
    dev = open(os.path.join(ROOT, "charginghub-env_amd", "csrc", "chub_lagrange.h")).read()
    L = lib()
    for fn in NEW:
        assert fn in _lib.EXPORTED and re.search(r"\bint %s\(" % fn, hdr), fn
        assert getattr(L, fn).argtypes is not None, fn
    assert re.search(r"enum \{ CHUB_COST_STEP = 0, CHUB_COST_AT_DONE, CHUB_COST_KIND_COUNT \}", hdr)
    assert re.search(r"enum CostKind \{ COST_STEP = 0, COST_AT_DONE, COST_KIND_COUNT \}", dev)
    assert _lib.COST_KIND == {"step": ll.STEP, "done": ll.AT_DONE} and (ll.STEP, ll.AT_DONE) == (0, 1)
    sizes = dict(re.findall(r"CHUB_LAG_(\w+) = (\d+)", hdr))
    assert (int(sizes["MAX_K"]), int(sizes["STATS"]), int(sizes["WORDS"])) == (_lib.LAG_MAX_K, _lib.LAG_STATS, _lib.LAG_WORDS) == (4, 6, 3)
    for name, want in (("kLagMaxK", 4), ("kLagStats", 6), ("kLagWords", 3), ("kLagLanes", ll.LANES), ("kLagCombineBlocks", ll.COMBINE_BLOCKS)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, dev).group(1)) == want, name
    # the look-ahead is k_gae's own constant, defined once in chub_gae.h, and the workgroup equals k_gae's
    gae = open(os.path.join(ROOT, "charginghub-env_amd", "csrc", "chub_gae.h")).read()
    for name, want in (("kGaeLanes", ll.LANES), ("kGaeAhead", ll.AHEAD)):
        assert [int(x) for x in re.findall(r"constexpr int %s = (\d+);" % name, gae)] == [want], name
    kern = open(os.path.join(ROOT, "charginghub-env_amd", "csrc", "chub_lagrange.hip")).read()
    assert "t1 -= kGaeAhead" in kern and "kLagAhead" not in kern + dev
    names = [n for n, _ in _lib.ChubConstraint._fields_]
    assert struct_fields(hdr, "chub_constraint") == names and C.sizeof(_lib.ChubConstraint) == 40
    names = ["lambda" if n == "lam" else n for n, _ in _lib.ChubCostGae._fields_]
    assert struct_fields(hdr, "chub_cost_gae") == names, (struct_fields(hdr, "chub_cost_gae"), names)
    assert C.sizeof(_lib.ChubCostGae) == 8 + 8 + 8 * (2 + 4 + 4 + 1) + 8 + 8 * (4 + 4 + 1)


# ---- the restated cost GAE
@pytest.mark.parametrize("name", ["n255-t7-k2-c3-all", "n513-t17-k4-c3-edge", "n257-t17-k1-c1-twice", "n256-t17-k2-c3-random-noret"])
def test_cost_gae_is_the_reward_recurrence_and_close_to_the_f64_sum(name):
    """operation for operation chub_rollout_gae_device's recurrence (pile_set_lib.gae_f32 restates it) with the cost as the reward; and
    within pile_set_lib.gae_bound -- derived from the f32 values held: three roundings per delta, two per product, one per sum -- of the
    textbook sum in f64"""
    case = BY_NAME[name]
    d = ll.gae_case(case)
    got = ll.cost_gae(d["terms"], d["done"], case["cons"], ll.GAMMA, ll.LAM, d["values"], d["finals"], None, d["carry"])
    T, N = case["T"], case["N"]
    for k, (column, kind) in enumerate(case["cons"]):
        cost = ll.costs_of(d["terms"], d["done"], column, kind)
        if kind == ll.AT_DONE:
            assert (ll.bits(cost[~d["done"]]) == 0).all() and np.array_equal(cost[d["done"]], d["terms"][:, :, column][d["done"]])
        V = np.zeros((T + 1, N), dtype=np.float32) if d["values"][k] is None else d["values"][k]
        a32, r32 = psl.gae_f32(cost, d["done"], V, d["finals"][k], ll.GAMMA, ll.LAM)
        assert np.array_equal(ll.bits(got["adv"][k]), ll.bits(a32)) and np.array_equal(ll.bits(got["ret"][k]), ll.bits(r32)), (name, k)
        a64, r64 = psl.gae_f64(cost, d["done"], V, d["finals"][k], ll.GAMMA, ll.LAM)
        ba, br = psl.gae_bound(cost, d["done"], V, d["finals"][k], ll.GAMMA, ll.LAM, a32, r32)
        assert (np.abs(a32 - a64) <= ba).all() and (np.abs(r32 - r64) <= br).all(), (name, k, np.abs(a32 - a64).max(), ba.max())
        assert np.abs(a32 - a64).max() > 0, "the bound is not met by identity"
        # the first three stats are the advantages' count, sum and squares within the reduction's own error
        a = got["adv"][k].astype(np.float64)
        st = got["stats"][k]
        assert st[0] == T * N and abs(st[1] - a.sum()) <= T * N * 2.0 ** -52 * np.abs(a).sum() and abs(st[2] - (a * a).sum()) <= T * N * 2.0 ** -52 * (a * a).sum()


@pytest.mark.parametrize("case", ll.GAE_CASES, ids=[c["name"] for c in ll.GAE_CASES])
def test_episode_sums_equal_a_forward_loop_in_exact_rationals(case):
    """costs are integers and halves and the carries integers: every sum and square is exact in f64, so the descending pass, the trees and
    a plain forward loop over Fractions agree exactly"""
    d = ll.gae_case(case)
    got = ll.cost_gae(d["terms"], d["done"], case["cons"], ll.GAMMA, ll.LAM, d["values"], d["finals"], d["mask"], d["carry"])
    live = np.ones(case["N"], dtype=bool) if d["mask"] is None else d["mask"] != 0
    for k, (column, kind) in enumerate(case["cons"]):
        cost = ll.costs_of(d["terms"], d["done"], column, kind)
        fin, rest = ll.episode_costs_forward(cost, d["done"], None if d["carry"] is None else d["carry"][:, k])
        eps = [x for e in np.nonzero(live)[0] for x in fin[e]]
        st = got["stats"][k]
        assert Fraction(st[3]) == len(eps) and Fraction(st[4]) == sum(eps, Fraction(0)) and Fraction(st[5]) == sum((x * x for x in eps), Fraction(0)), (case["name"], k)
        for e in range(case["N"]):
            want = rest[e] if live[e] else Fraction(0 if d["carry"] is None else float(d["carry"][e, k]))
            assert Fraction(got["carry"][e, k]) == want, (case["name"], k, e)
        if d["mask"] is not None:
            assert np.isnan(got["adv"][k][:, ~live]).all() and not np.isnan(got["adv"][k][:, live]).any()


@pytest.mark.parametrize("name", ["n513-t17-k4-c3-edge", "n257-t17-k1-c1-twice", "n255-t8-k1-c3-none-carry", "n513-t9-k2-c3-random-mask"])
def test_two_calls_with_the_carry_equal_one_call_on_the_concatenation(name):
    case = BY_NAME[name]
    a, b = ll.gae_case(case, seed=1), ll.gae_case(case, seed=2)
    first = ll.cost_gae(a["terms"], a["done"], case["cons"], ll.GAMMA, ll.LAM, mask=a["mask"], carry=a["carry"])
    second = ll.cost_gae(b["terms"], b["done"], case["cons"], ll.GAMMA, ll.LAM, mask=a["mask"], carry=first["carry"])
    both = ll.cost_gae(np.concatenate([a["terms"], b["terms"]]), np.concatenate([a["done"], b["done"]]), case["cons"], ll.GAMMA, ll.LAM,
                       mask=a["mask"], carry=a["carry"])
    assert np.array_equal(second["carry"], both["carry"])
    assert np.array_equal(first["stats"][:, 3:] + second["stats"][:, 3:], both["stats"][:, 3:]), name
    assert both["stats"][:, 3].sum() > 0 or case["done"] == "none"


# ---- the step rule against the library's host form
def fold(c):
    from charginghub_env_amd import _lib
    lam, w = np.array([c["lam"]], dtype=np.float64), np.array(c["words"], dtype=np.float64)
    con = _lib.ChubConstraint(0, 0, c["limit"], c["lr"], 0.0, c["lambda_max"])
    assert lib().chub_lagrange_fold(C.byref(con), ptr(lam), ptr(w), ptr(np.asarray(c["stats"], dtype=np.float64))) == 0, last_error()
    return lam[0], w


@pytest.mark.parametrize("name", list(STEPS))
def test_the_fold_equals_the_restatement_bit_for_bit(name):
    c = STEPS[name]
    lam, w = fold(c)
    want_lam, want_w = ll.lagrange_step(c["lam"], c["words"], c["stats"], c["limit"], c["lr"], c["lambda_max"])
    assert ll.bits(np.float64(lam)) == ll.bits(np.float64(want_lam)) and np.array_equal(ll.bits(w), ll.bits(want_w)), (name, lam, w, want_lam, want_w)


def test_the_step_rule_case_by_case():
    lam, w = fold(STEPS["no_episode"])
    assert lam == 0.25 and list(w) == [1.5, 3.0, 2.0], "n == 0: lambda and J_last keep their bits, one more skipped"
    lam, w = fold(STEPS["floor"])
    assert lam == 0.0 and list(w) == [0.5, 1.0, 0.0], "0.1 + 0.1 (0.5 - 5.5) is floored at 0; the step counts as taken"
    lam, w = fold(STEPS["ceiling"])
    assert lam == 10.0 and list(w) == [25.0, 8.0, 0.0]
    lam, w = fold(STEPS["no_ceiling"])
    assert lam == 9.9 + 0.5 * 24.0 and list(w) == [25.0, 8.0, 0.0], "lambda_max == 0: no ceiling"
    for name in ("nan_cost", "infinite_cost"):
        lam, w = fold(STEPS[name])
        assert lam == 0.25 and list(w) == [2.0, 3.0, 2.0], name
    lam, w = fold(STEPS["at_the_limit"])
    assert lam == 0.75 and list(w) == [4.0, 2.0, 0.0], "J == limit: taken, lambda where it was"
    # a multiplier that is NaN stays and the step is skipped
    lam, w = fold(dict(STEPS["ordinary"], lam=np.nan))
    assert np.isnan(lam) and list(w) == [0.0, 3.0, 2.0]


def test_refusals_without_a_device():
    from charginghub_env_amd import _lib
    L = lib()
    lam, w, st = np.zeros(1), np.zeros(3), np.zeros(6)
    good = dict(column=0, kind=0, limit=1.0, lr=0.1, lambda0=0.0, lambda_max=0.0)
    con = lambda **kw: C.byref(_lib.ChubConstraint(**dict(good, **kw)))
    h, h2, n = C.c_void_p(), C.c_void_p(), C.c_int64()
    stand_in = C.c_void_p(8)  # (never read: a call refused for its arguments returns before it touches the handle)
    cases = [
        ("fold: null constraint", lambda: L.chub_lagrange_fold(None, ptr(lam), ptr(w), ptr(st)), "null"),
        ("fold: null lambda", lambda: L.chub_lagrange_fold(con(), None, ptr(w), ptr(st)), "null"),
        ("fold: null words", lambda: L.chub_lagrange_fold(con(), ptr(lam), None, ptr(st)), "null"),
        ("fold: null stats", lambda: L.chub_lagrange_fold(con(), ptr(lam), ptr(w), None), "null"),
        ("fold: unknown kind", lambda: L.chub_lagrange_fold(con(kind=2), ptr(lam), ptr(w), ptr(st)), "kind"),
        ("fold: negative kind", lambda: L.chub_lagrange_fold(con(kind=-1), ptr(lam), ptr(w), ptr(st)), "kind"),
        ("fold: negative column", lambda: L.chub_lagrange_fold(con(column=-1), ptr(lam), ptr(w), ptr(st)), "column"),
        ("fold: negative lr", lambda: L.chub_lagrange_fold(con(lr=-0.1), ptr(lam), ptr(w), ptr(st)), "finite"),
        ("fold: NaN limit", lambda: L.chub_lagrange_fold(con(limit=float("nan")), ptr(lam), ptr(w), ptr(st)), "finite"),
        ("fold: infinite lambda_max", lambda: L.chub_lagrange_fold(con(lambda_max=float("inf")), ptr(lam), ptr(w), ptr(st)), "finite"),
        ("fold: negative lambda0", lambda: L.chub_lagrange_fold(con(lambda0=-1.0), ptr(lam), ptr(w), ptr(st)), "finite"),
        ("fold: lambda0 above the ceiling", lambda: L.chub_lagrange_fold(con(lambda0=2.0, lambda_max=1.0), ptr(lam), ptr(w), ptr(st)), "lambda0"),
        ("create: null handle", lambda: L.chub_lagrange_create(None, 1, con(), C.byref(h)), "null"),
        ("create: null constraints", lambda: L.chub_lagrange_create(stand_in, 1, None, C.byref(h)), "null"),
        ("create: null out", lambda: L.chub_lagrange_create(stand_in, 1, con(), None), "null"),
        ("create: K = 0", lambda: L.chub_lagrange_create(stand_in, 0, con(), C.byref(h)), "1 .. 4"),
        ("create: K = 5", lambda: L.chub_lagrange_create(stand_in, 5, con(), C.byref(h)), "1 .. 4"),
        ("create: unknown kind", lambda: L.chub_lagrange_create(stand_in, 1, con(kind=7), C.byref(h)), "kind"),
        ("gae: null", lambda: L.chub_lagrange_gae_device(None, C.byref(_lib.ChubCostGae()), None), "null"),
        ("step: null", lambda: L.chub_lagrange_step_device(None, None), "null"),
        ("combine: null", lambda: L.chub_lagrange_combine_device(None, 1, ptr(st), None, (C.c_void_p * 4)(), ptr(st), None), "null"),
        ("device: null", lambda: L.chub_lagrange_device(None, C.byref(h), C.byref(h2)), "null"),
        ("read: null", lambda: L.chub_lagrange_read(None, ptr(lam), ptr(st), ptr(w)), "null"),
        ("set_lambda: null", lambda: L.chub_lagrange_set_lambda_device(None, ptr(lam), None), "null"),
        ("state_size: null", lambda: L.chub_lagrange_state_size(None, C.byref(n)), "null"),
        ("get_state: null", lambda: L.chub_lagrange_get_state(None, ptr(st)), "null"),
        ("set_state: null", lambda: L.chub_lagrange_set_state(None, ptr(st)), "null"),
        ("collect_terms: null handle", lambda: L.chub_policy_collect_terms(None, None, 0, -1, None, None, None, 0, 1, ptr(st), None), "null"),
    ]
    for what, call, text in cases:
        before = (lam.copy(), w.copy())
        assert call() == ERR_ARG, what
        assert text in last_error(), (what, last_error())
        assert np.array_equal(lam, before[0]) and np.array_equal(w, before[1]), what
    assert L.chub_lagrange_destroy(None) == 0, "destroying nothing is not an error"


# ---- the failure experiment: each wrong variant differs from the definition on a named case of the GPU test's lists
def gae_differs(name, wrong, what):
    case = BY_NAME[name]
    d = ll.gae_case(case)
    run = lambda w: ll.cost_gae(d["terms"], d["done"], case["cons"], ll.GAMMA, ll.LAM, d["values"], d["finals"], d["mask"], d["carry"], wrong=w)
    good, bad = run(None), run(wrong)
    return {"adv": not np.array_equal(ll.bits(good["adv"][0]), ll.bits(bad["adv"][0])) or
            any(not np.array_equal(ll.bits(g), ll.bits(b)) for g, b in zip(good["adv"], bad["adv"])),
            "episodes": not np.array_equal(good["stats"][:, 3:], bad["stats"][:, 3:]),
            "carry": not np.array_equal(good["carry"], bad["carry"])}[what]


def test_every_wrong_variant_is_told_apart():
    seen = set()
    # (a) an AT_DONE cost taken at every step: the advantages and the episode costs of a case whose done is rare
    assert gae_differs("n257-t9-k2-c27-last", "at_done_every_step", "adv") and gae_differs("n257-t17-k1-c1-twice", "at_done_every_step", "episodes")
    seen.add("at_done_every_step")
    # (b) the carry dropped: the episode that ends inside the rollout misses what it cost before, and an open one forgets it
    assert gae_differs("n1-t9-k2-c3-last-carry", "carry_dropped", "episodes") and gae_differs("n255-t8-k1-c3-none-carry", "carry_dropped", "carry")
    seen.add("carry_dropped")
    # (c) the segment behind the last done is an open episode, not a finished one
    assert gae_differs("n255-t7-k2-c3-all", "open_segment_counted", "episodes") and gae_differs("n257-t17-k1-c1-twice", "open_segment_counted", "episodes")
    assert not gae_differs("n255-t8-k1-c3-none-carry", "open_segment_counted", "episodes"), "without a done nothing closes either way"
    seen.add("open_segment_counted")
    # (d) lambda clamped before the increment: the floor is missed
    c = STEPS["floor"]
    good, bad = (ll.lagrange_step(c["lam"], c["words"], c["stats"], c["limit"], c["lr"], c["lambda_max"], wrong=w)[0] for w in (None, "clamp_before_increment"))
    assert good == 0.0 and bad < 0.0
    c = STEPS["ceiling"]
    assert ll.lagrange_step(c["lam"], c["words"], c["stats"], c["limit"], c["lr"], c["lambda_max"], wrong="clamp_before_increment")[0] > c["lambda_max"]
    seen.add("clamp_before_increment")
    # (e), (f) on the combine cases
    stats = np.array([[960.0, 480.0, 0.0, 0.0, 0.0, 0.0], [960.0, -96.0, 0.0, 0.0, 0.0, 0.0], [960.0, 1440.0, 0.0, 0.0, 0.0, 0.0]])
    by = {c["name"]: c for c in ll.COMBINE_CASES}
    adv, st, costs = ll.combine_case(by["n255-mixed"])
    good, bad = (ll.combine(adv, st, costs, by["n255-mixed"]["lam"], stats, wrong=w) for w in (None, "not_centred"))
    assert not np.array_equal(ll.bits(good), ll.bits(bad)) and np.abs(good - bad).max() > 0.1
    seen.add("not_centred")
    # (f) differs only in the sign of zeros: a = -0.0 minus 0 * (a negative number) = -0.0 - (-0.0) = +0.0
    case = by["n257-zeros-no-stats-signed-zeros"]
    adv, st, costs = ll.combine_case(case)
    good, bad = (ll.combine(adv, st, costs, case["lam"], stats, wrong=w) for w in (None, "zero_lambda_not_skipped"))
    assert np.array_equal(good, bad), "equal as numbers"
    assert np.array_equal(ll.bits(good), ll.bits(adv)), "every lambda 0 and no stats: the advantage's own bits"
    differ = ll.bits(good) != ll.bits(bad)
    assert differ.any() and (good[differ] == 0).all() and (ll.bits(good[differ]) == 0x80000000).all() and (ll.bits(bad[differ]) == 0).all()
    seen.add("zero_lambda_not_skipped")
    assert seen == set(ll.WRONG)


def test_all_multipliers_zero_leave_the_normalised_advantage():
    by = {c["name"]: c for c in ll.COMBINE_CASES}
    adv, st, costs = ll.combine_case(by["n255-zeros-stats"])
    m32, s32 = ll.advantage_normaliser(st)
    want = ((adv - m32).astype(np.float32) * s32).astype(np.float32)
    got = ll.combine(adv, st, costs, [0.0, 0.0, 0.0], np.ones((3, 6)))
    assert np.array_equal(ll.bits(got), ll.bits(want))
