"""Reward scaling's host-only parts (include/chub.h, "reward scaling on the device") and its numpy restatement tests/return_norm_lib.py,
without a device.  Three tests load the library and fail without the feature: the symbols, structs and constants; chub_return_norm_fold
bit for bit on made partials; the refusals that need no device.  The rest hold return_norm_lib to independent statements -- exact
rationals, a forward Python loop, numpy's two-pass variance, pile_set_lib's recurrence -- and run the failure experiment: every wrong=
variant differs on a named case of the GPU test's list."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import pile_set_lib as psl
import return_norm_lib as rl

ERR_ARG = -1
F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["chub_return_norm_create", "chub_return_norm_destroy", "chub_return_norm_update_device", "chub_return_norm_gae_device",
       "chub_return_norm_reset_carry_device", "chub_return_norm_reset_device", "chub_return_norm_device", "chub_return_norm_state_size",
       "chub_return_norm_get_state", "chub_return_norm_set_state", "chub_return_norm_fold"]
VARIANTS = [(c, carry) for c in rl.CASES for carry in (False, True)]
IDS = ["%s-%s" % (c["name"], "carry" if k else "plain") for c, k in VARIANTS]


def masked(case, carry):
    """the GPU test's rule: masks alternate over the list, so that both carry states meet both mask states"""
    return (rl.CASES.index(case) + int(carry)) % 2 == 1


def lib():
    from charginghub_env_amd import _lib
    return _lib.load_library()


def last_error():
    return lib().chub_last_error().decode()


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the tests that load the library
def test_header_device_header_and_binding_agree():
    from charginghub_env_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "chub.h")).read()
    dev = open(os.path.join(ROOT, "charginghub-env_amd", "csrc", "chub_retnorm.h")).read()
    L = lib()
    for fn in NEW:
        assert fn in _lib.EXPORTED and re.search(r"\bint %s\(" % fn, hdr), fn
        assert getattr(L, fn).argtypes is not None, fn
    body = re.search(r"typedef struct chub_return_norm_spec \{(.*?)\} chub_return_norm_spec;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(float|double) (\w+);", body) == [("float", "gamma"), ("float", "clip"), ("double", "eps")]
    assert [n for n, _ in _lib.ChubReturnNormSpec._fields_] == ["gamma", "clip", "eps"] and C.sizeof(_lib.ChubReturnNormSpec) == 16
    assert int(re.search(r"#define CHUB_RETURN_NORM_MAGIC (0x[0-9a-f]+)ull", hdr).group(1), 16) == _lib.RETURN_NORM_MAGIC == rl.MAGIC
    assert rl.MAGIC.to_bytes(8, "little") == b"CHBRNRM1" and _lib.RETURN_NORM_BLOB_HEAD == rl.BLOB_HEAD
    for name, want in (("kRetLanes", rl.LANES), ("kRetAhead", rl.AHEAD)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, dev).group(1)) == want, name
    # the scaled GAE is k_gae itself: its look-ahead and workgroup are defined once, in chub_gae.h
    gae = open(os.path.join(ROOT, "charginghub-env_amd", "csrc", "chub_gae.h")).read()
    for name, want in (("kGaeLanes", rl.LANES), ("kGaeAhead", rl.AHEAD)):
        assert [int(x) for x in re.findall(r"constexpr int %s = (\d+);" % name, gae)] == [want], name
    # the scaled call shares chub_gae unchanged
    assert re.search(r"int chub_return_norm_gae_device\(chub_return_norm \*rn, const chub_gae \*g, void \*stream\);", hdr)


FOLDS = {
    "empty-state": dict(state=[0.0, 0.0, 0.0], n_b=24.0, K=1.5, S1=-6.0, S2=40.5),
    "running": dict(state=[96.0, 2.25, 310.0], n_b=24.0, K=2.25, S1=-6.0, S2=40.5),
    "running-thirds": dict(state=[7.0, 1.0 / 3.0, 0.1], n_b=3.0, K=1.0 / 3.0, S1=0.7, S2=0.9),
    "nothing-counted": dict(state=[96.0, 2.25, 310.0], n_b=0.0, K=2.25, S1=0.0, S2=0.0),
    "nothing-counted-empty": dict(state=[0.0, 0.0, 0.0], n_b=0.0, K=7.0, S1=0.0, S2=0.0),
    "constant": dict(state=[0.0, 0.0, 0.0], n_b=12.0, K=3.0, S1=0.0, S2=0.0),
    "cancels-below-zero": dict(state=[0.0, 0.0, 0.0], n_b=3.0, K=0.0, S1=0.3, S2=0.03 - 1e-17),
    "nan": dict(state=[0.0, 0.0, 0.0], n_b=8.0, K=1.0, S1=np.nan, S2=np.nan),
    "nan-pivot": dict(state=[0.0, 0.0, 0.0], n_b=8.0, K=np.nan, S1=np.nan, S2=np.nan),
    "huge": dict(state=[1e6, -4e5, 3e17], n_b=6291456.0, K=-4e5, S1=1.25e9, S2=7.5e14),
}


@pytest.mark.parametrize("name", list(FOLDS))
@pytest.mark.parametrize("eps", [1e-8, 1e-4])
def test_the_fold_equals_the_restatement_bit_for_bit(name, eps):
    from charginghub_env_amd import vec_env
    f = FOLDS[name]
    st = np.array(f["state"], dtype=F64)
    sc = vec_env.return_norm_fold(st, f["n_b"], f["K"], f["S1"], f["S2"], eps)
    want, wsc = rl.fold(f["state"], f["n_b"], f["K"], f["S1"], f["S2"], eps)
    assert np.array_equal(rl.bits(st), rl.bits(want)), (name, st, want)
    assert (sc is None and wsc is None) or rl.bits(F32(sc)) == rl.bits(F32(wsc)), (name, sc, wsc)
    if name == "constant":
        assert st[2] == 0.0 and st[1] == 3.0 and rl.bits(F32(sc)) == rl.bits(F32(F64(1.0) / np.sqrt(F64(eps))))
    if name == "cancels-below-zero":
        assert st[2] == 0.0, "S2 - S1 S1 / n_b below 0 is 0"
    if name.startswith("nan"):
        assert np.isnan(st[1]) and np.isnan(st[2]) and np.isnan(sc) and st[0] == 8.0
    if name.startswith("nothing"):
        assert sc is None and np.array_equal(st, np.array(f["state"]))


def test_refusals_without_a_device():
    from charginghub_env_amd import _lib
    L = lib()
    st, sc = np.array([1.0, 2.0, 3.0]), np.array([0.5], dtype=F32)
    spec = lambda **kw: C.byref(_lib.ChubReturnNormSpec(**dict(dict(gamma=0.99, clip=10.0, eps=1e-8), **kw)))
    h, h2, h3, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
    stand_in = C.c_void_p(8)  # (never read: a call refused for its arguments returns before it touches the handle)
    nan, inf = float("nan"), float("inf")
    fold = lambda s, c, eps: L.chub_return_norm_fold(s, c, 4.0, 1.0, 2.0, 3.0, eps)
    cases = [
        ("fold: null state", lambda: fold(None, ptr(sc), 1e-8), "null"),
        ("fold: null scale", lambda: fold(ptr(st), None, 1e-8), "null"),
        ("fold: eps 0", lambda: fold(ptr(st), ptr(sc), 0.0), "eps"),
        ("fold: eps negative", lambda: fold(ptr(st), ptr(sc), -1e-8), "eps"),
        ("fold: eps NaN", lambda: fold(ptr(st), ptr(sc), nan), "eps"),
        ("fold: eps infinite", lambda: fold(ptr(st), ptr(sc), inf), "eps"),
        ("create: null handle", lambda: L.chub_return_norm_create(None, spec(), C.byref(h)), "null"),
        ("create: null spec", lambda: L.chub_return_norm_create(stand_in, None, C.byref(h)), "null"),
        ("create: null out", lambda: L.chub_return_norm_create(stand_in, spec(), None), "null"),
        ("create: gamma above 1", lambda: L.chub_return_norm_create(stand_in, spec(gamma=1.5), C.byref(h)), "gamma"),
        ("create: gamma negative", lambda: L.chub_return_norm_create(stand_in, spec(gamma=-0.1), C.byref(h)), "gamma"),
        ("create: gamma NaN", lambda: L.chub_return_norm_create(stand_in, spec(gamma=nan), C.byref(h)), "gamma"),
        ("create: eps 0", lambda: L.chub_return_norm_create(stand_in, spec(eps=0.0), C.byref(h)), "eps"),
        ("create: eps infinite", lambda: L.chub_return_norm_create(stand_in, spec(eps=inf), C.byref(h)), "eps"),
        ("create: eps NaN", lambda: L.chub_return_norm_create(stand_in, spec(eps=nan), C.byref(h)), "eps"),
        ("create: clip negative", lambda: L.chub_return_norm_create(stand_in, spec(clip=-1.0), C.byref(h)), "clip"),
        ("create: clip NaN", lambda: L.chub_return_norm_create(stand_in, spec(clip=nan), C.byref(h)), "clip"),
        ("update: null", lambda: L.chub_return_norm_update_device(None, ptr(st), 4, None, None), "null"),
        ("gae: null", lambda: L.chub_return_norm_gae_device(None, C.byref(_lib.ChubGae()), None), "null"),
        ("reset_carry: null", lambda: L.chub_return_norm_reset_carry_device(None, None, None), "null"),
        ("reset: null", lambda: L.chub_return_norm_reset_device(None, None), "null"),
        ("device: null", lambda: L.chub_return_norm_device(None, C.byref(h), C.byref(h2), C.byref(h3)), "null"),
        ("state_size: null", lambda: L.chub_return_norm_state_size(None, C.byref(n)), "null"),
        ("get_state: null", lambda: L.chub_return_norm_get_state(None, ptr(st)), "null"),
        ("set_state: null", lambda: L.chub_return_norm_set_state(None, ptr(st)), "null"),
    ]
    for what, call, text in cases:
        assert call() == ERR_ARG, what
        assert text in last_error(), (what, last_error())
        assert st.tolist() == [1.0, 2.0, 3.0] and sc[0] == 0.5 and h.value is None, what
    assert L.chub_return_norm_destroy(None) == 0, "destroying nothing is not an error"


# ---- the restatement against independent statements (these pass on return_norm_lib alone: no coverage of the kernels)
@pytest.mark.parametrize("case,carry", VARIANTS, ids=IDS)
def test_every_made_case_is_exact_from_an_empty_state(case, carry):
    """the proof the GPU test's bit-for-bit comparison rests on: g in f32 and every partial sum of d and d d in f64 are exact, so the
    restated order, the device's order and exact rationals give one answer; the restatement is held to the rationals here"""
    a = rl.case_arrays(case, carry=carry, mask=masked(case, carry))
    g, rest, n_b, S1, S2 = rl.prove_exact(case, a)
    got = rl.update([0.0, 0.0, 0.0], 1.0, a["carry"], a["reward"], a["done"], case["gamma"], rl.EPS, a["mask"])
    live = got["live"]
    T, N = a["reward"].shape
    for t in range(T):
        for e in np.nonzero(live)[0]:
            assert Fraction(float(got["g"][t, e])) == g[t][e], (case["name"], t, e)
    assert np.isnan(got["g"][:, ~live]).all()
    for e in range(N):
        want = rest[e] if live[e] else (Fraction(0) if a["carry"] is None else Fraction(float(a["carry"][e])))
        assert Fraction(float(got["carry"][e])) == want, (case["name"], "carry", e)
    assert (Fraction(got["sums"][0]), Fraction(got["sums"][1]), Fraction(got["sums"][2])) == (n_b, S1, S2), case["name"]
    assert n_b == T * int(live.sum()) and got["state"][0] == n_b
    # mean and M2 against numpy's two-pass statistics of the counted values, to the precision of f64 on numbers of this size
    x = got["g"][:, live].astype(F64).ravel()
    assert abs(got["state"][1] - x.mean()) <= 1e-12 * (1.0 + np.abs(x).max())
    assert abs(got["state"][2] - x.var() * x.size) <= 1e-9 * (1.0 + x.var() * x.size)
    assert rl.bits(got["scale"]) == rl.bits(F32(F64(1.0) / np.sqrt(got["state"][2] / got["state"][0] + F64(rl.EPS))))


def test_the_forward_recurrence_is_a_plain_python_loop():
    case = rl.case_named("n257-t17-twice-g1")
    a = rl.case_arrays(case, carry=True, mask=True)
    got, carry, live = rl.returns_forward(a["reward"], a["done"], 0.99, a["carry"], a["mask"])
    gm = F32(0.99)
    for e in range(case["N"]):
        g = F32(a["carry"][e])
        for t in range(case["T"]):
            g = F32(F32(gm * g) + a["reward"][t, e])
            if live[e]:
                assert rl.bits(got[t, e]) == rl.bits(g)
            if a["done"][t, e]:
                g = F32(0.0)
        assert rl.bits(carry[e]) == rl.bits(g if live[e] else a["carry"][e])


def test_two_updates_are_one_update_within_the_derived_bounds():
    """floats, three successive updates: each lies within 6.21's bounds of the definition in exact rationals applied to the state it started
    from, and the final state is close to numpy's statistics of everything counted"""
    rs = np.random.RandomState(3)
    N, T = 513, 17
    state, scale, carry = np.zeros(3), F32(1.0), None
    seen = []
    for it in range(3):
        reward = (rs.normal(size=(T, N)) * 30.0 + 5.0).astype(F32)
        done = rs.rand(T, N) < 0.1
        out = rl.update(state, scale, carry, reward, done, 0.99, rl.EPS)
        want, b_mean, b_m2 = rl.merge_bounds(state, out["g"], out["live"])
        assert out["state"][0] == want[0] and abs(out["state"][1] - want[1]) <= b_mean and abs(out["state"][2] - want[2]) <= b_m2, it
        state, scale, carry = out["state"], out["scale"], out["carry"]
        seen.append(out["g"].astype(F64).ravel())
    x = np.concatenate(seen)
    assert abs(state[1] - x.mean()) <= 1e-11 * np.abs(x).max() and abs(state[2] / state[0] - x.var()) <= 1e-10 * x.var()


def test_scale_one_without_a_clip_is_the_plain_recurrence_and_the_clip_selects():
    packed, values, final = psl.gae_case(5, "last", True)
    D = packed.shape[2] - 2
    r, d = packed[:, :, D], packed[:, :, D + 1]
    a0, r0 = psl.gae_f32(r, d, values, final, 0.99, 0.95)
    a1, r1, st = rl.scaled_gae(r, d, values, final, 0.99, 0.95, 1.0, 0.0)
    assert np.array_equal(rl.bits(a0), rl.bits(a1)) and np.array_equal(rl.bits(r0), rl.bits(r1)) and st[0] == a0.size
    x = rl.scaled_reward(np.array([4.0, -4.0, 6.0, -6.0, 3.0, np.nan, -0.0], dtype=F32), 0.5, 2.0)
    assert x[:5].tolist() == [2.0, -2.0, 2.0, -2.0, 1.5] and np.isnan(x[5]) and rl.bits(x[6:])[0] == 0x80000000
    assert rl.scaled_reward(np.array([1e6], dtype=F32), 3.0, 0.0)[0] == F32(3e6), "clip 0: none"


def test_the_blob_round_trips():
    carry = np.arange(5, dtype=F32) - 2
    blob = rl.blob_of(5, [10.0, -1.5, 7.25], F32(0.25), carry)
    magic, N, state, scale, c = rl.blob_parts(blob)
    assert len(blob) == 48 + 20 and (magic, N, state.tolist(), scale) == (rl.MAGIC, 5, [10.0, -1.5, 7.25], 0.25) and np.array_equal(c, carry)


# ---- the failure experiment: each wrong variant differs from the definition on a named case of the GPU test's list
def shows(case, carry, wrong, scale=0.5, clip=2.0):
    """the outputs (of an update from an empty state, and of the scaled GAE at `scale` and `clip`) on which the variant's bits differ"""
    a = rl.case_arrays(case, carry=carry, mask=masked(case, carry))
    run = lambda w: rl.update([0.0, 0.0, 0.0], 1.0, a["carry"], a["reward"], a["done"], case["gamma"], rl.EPS, a["mask"], wrong=w)
    good, bad = run(None), run(wrong)
    out = set()
    for k in ("state", "carry"):
        if not np.array_equal(rl.bits(good[k]), rl.bits(bad[k])):
            out.add(k)
    if rl.bits(good["scale"]) != rl.bits(bad["scale"]):
        out.add("scale")
    V = np.zeros((case["T"] + 1, case["N"]), dtype=F32)
    adv = lambda w: rl.scaled_gae(a["reward"], a["done"], V, None, 0.5, 1.0, scale, clip, a["mask"], wrong=w)[0]
    if not np.array_equal(rl.bits(adv(None)), rl.bits(adv(wrong))):
        out.add("adv")
    return out


TABLE = {
    # variant: (case, with a carry, the outputs that must differ)
    "carry_not_zeroed": ("n257-t9-last-g1", False, {"carry"}),
    "zeroed_before_counting": ("n255-t7-all-g05", False, {"state", "scale"}),
    "sample_variance": ("n1-t7-all-g05", False, {"scale"}),
    "clip_before_scale": ("n256-t8-first-g1", False, {"adv"}),
    "masked_carry_advanced": ("n256-t8-first-g1", False, {"carry"}),
    "pivot_dropped": (rl.OFFSET_CASE, False, {"state", "scale"}),
}


@pytest.mark.parametrize("wrong", rl.WRONG)
def test_every_wrong_variant_shows_on_its_named_case(wrong):
    name, carry, must = TABLE[wrong]
    case = rl.case_named(name)
    if wrong == "masked_carry_advanced":
        assert masked(case, carry), "the named case runs with a mask"
    got = shows(case, carry, wrong)
    assert must <= got, (wrong, name, got)
    everywhere = [c["name"] for c, k in VARIANTS if shows(c, k, wrong)]
    assert name in everywhere
    if wrong == "pivot_dropped":
        # the raw sum of squares is near 2^55, where an f64 steps by 8: the pivoted M2 is the exact one to 2^-40, the raw one is off by more
        # than 2^-20 of it, a million times that
        a = rl.case_arrays(case, carry=carry, mask=masked(case, carry))
        g, rest, n_b, S1, S2 = rl.prove_exact(case, a)
        exact = S2 - S1 * S1 / n_b
        right = rl.update([0.0, 0.0, 0.0], 1.0, a["carry"], a["reward"], a["done"], case["gamma"], rl.EPS, a["mask"])["state"][2]
        raw = rl.update([0.0, 0.0, 0.0], 1.0, a["carry"], a["reward"], a["done"], case["gamma"], rl.EPS, a["mask"], wrong=wrong)["state"][2]
        assert abs(right - float(exact)) <= 2.0 ** -40 * float(exact) and abs(raw - float(exact)) > 2.0 ** -20 * float(exact), (right, raw, float(exact))
        plain = [c["name"] for c, k in VARIANTS if "offset" not in c and {"state", "scale"} & shows(c, k, wrong)]
        print("pivot_dropped also moves bits on", plain)


def test_print_the_failure_table(capsys):
    """the table DESIGN 6.29 carries: per variant, the cases of the list on which any output differs"""
    with capsys.disabled():
        for wrong in rl.WRONG:
            hits = ["%s%s:%s" % (c["name"], "+carry" if k else "", ",".join(sorted(s))) for c, k in VARIANTS for s in [shows(c, k, wrong)] if s]
            print("\n%s: %d of %d: %s" % (wrong, len(hits), len(VARIANTS), "; ".join(hits[:4])))
            assert hits, wrong
