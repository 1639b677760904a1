"""Reward scaling on the device (include/chub.h, "reward scaling on the device") restated in numpy, operation for operation: the forward
recurrence of the discounted return with its carry, the pivoted sums in the kernels' reduction order, the merge into the running state,
the scale, and the scaled, clipped reward fed to pile_set_lib's GAE recurrence.  f32 arithmetic is numpy float32 arithmetic (every
operation rounded once), the sums are f64 in the order the header states.  `wrong=` switches one deliberate mistake on, for the failure
experiment of tests/test_return_norm_cpu.py; the case list below is what the GPU test runs."""
from fractions import Fraction

import numpy as np

import pile_set_lib as psl

F32, F64 = np.float32, np.float64
LANES, AHEAD = 256, 8
MAGIC, BLOB_HEAD = 0x314D524E52424843, 48
WRONG = ("carry_not_zeroed", "zeroed_before_counting", "sample_variance", "clip_before_scale", "masked_carry_advanced", "pivot_dropped")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == F32 else np.uint64)


# ---- the reduction order (chub_rollout_gae_device's)
def tree(lanes):
    """[blocks, 256, W] -> [blocks, W]: lane l takes lane l + h, h = 128 .. 1"""
    a = np.array(lanes, dtype=F64)
    h = LANES // 2
    while h > 0:
        a[:, :h] = a[:, :h] + a[:, h:2 * h]
        h //= 2
    return a[:, 0]


def reduce_lanes(w):
    """per-env words [N, W] f64 -> [W]: the workgroups' trees, then lane l of the merge takes partials l, l + 256, .. ascending from 0, then
    the same tree"""
    N, W = w.shape
    blocks = (N + LANES - 1) // LANES
    lanes = np.zeros((blocks * LANES, W), dtype=F64)
    lanes[:N] = w
    partials = tree(lanes.reshape(blocks, LANES, W))
    acc = np.zeros((LANES, W), dtype=F64)
    for b in range(blocks):
        acc[b % LANES] = acc[b % LANES] + partials[b]
    return tree(acc[None])[0]


# ---- the discounted return, forward in t
def returns_forward(reward, done, gamma, carry=None, mask=None, wrong=None):
    """reward, done [T, N] (done: non-zero fires), carry [N] f32 or None (zeros) -> (g [T, N] f32 as counted, carry_out [N] f32, live [N]);
    a masked-out env's column of g is NaN (not counted) and its carry keeps its bits"""
    r = np.asarray(reward, dtype=F32)
    d = np.asarray(done) != 0
    T, N = r.shape
    live = np.ones(N, dtype=bool) if mask is None else np.asarray(mask) != 0
    c0 = np.zeros(N, dtype=F32) if carry is None else np.array(carry, dtype=F32)
    g, gm = c0.copy(), F32(gamma)
    out = np.full((T, N), np.nan, dtype=F32)
    with np.errstate(all="ignore"):
        for t in range(T):
            if wrong == "zeroed_before_counting":
                g = (F32(gm * g) + r[t]).astype(F32)
                g = np.where(d[t], F32(0), g).astype(F32)
                out[t] = g
                continue
            g = (F32(gm * g) + r[t]).astype(F32)
            out[t] = g
            if wrong != "carry_not_zeroed":
                g = np.where(d[t], F32(0), g).astype(F32)
    out[:, ~live] = np.nan
    keep = ~live if wrong != "masked_carry_advanced" else np.zeros(N, dtype=bool)
    return out, np.where(keep, c0, g).astype(F32), live


def scale_of(n, m2, eps, wrong=None):
    with np.errstate(all="ignore"):
        if n == 0.0:
            return F32(1.0)
        den = F64(n) - F64(1.0) if wrong == "sample_variance" else F64(n)
        return F32(F64(1.0) / np.sqrt(F64(m2) / den + F64(eps)))


def fold(state, n_b, K, S1, S2, eps, wrong=None):
    """(n, mean, M2), the sums of n_b values around K -> ((n', mean', M2'), scale32), every f64 operation rounded once; n_b == 0: (state, None)"""
    n, mean, m2 = (F64(x) for x in state)
    n_b, K, S1, S2 = F64(n_b), F64(K), F64(S1), F64(S2)
    if not n_b > 0.0:
        return np.array([n, mean, m2], dtype=F64), None
    with np.errstate(all="ignore"):
        t = S2 - (S1 * S1) / n_b
        m2b = F64(0.0) if t < 0.0 else t
        n1 = n + n_b
        if n > 0.0:
            db = S1 / n_b
            mean1 = K + S1 / n1
            m21 = (m2 + m2b) + (db * db) * ((n * n_b) / n1)
        else:
            mean1 = K + S1 / n_b
            m21 = m2b
    return np.array([n1, mean1, m21], dtype=F64), scale_of(n1, m21, eps, wrong)


def sums(g, live, K):
    """the counted values' (n_b, S1, S2) around K in the kernels' order: a lane t ascending, then reduce_lanes"""
    T, N = g.shape
    w = np.zeros((N, 3), dtype=F64)
    with np.errstate(all="ignore"):
        for t in range(T):
            dd = g[t].astype(F64) - F64(K)
            w[:, 1] = w[:, 1] + dd
            w[:, 2] = w[:, 2] + dd * dd
    w[:, 0] = float(T)
    w[~live] = 0.0
    return reduce_lanes(w)


def update(state, scale, carry, reward, done, gamma, eps, mask=None, wrong=None):
    """chub_return_norm_update_device: -> dict(state [3] f64, scale f32, carry [N] f32, g, K, sums)"""
    state = np.asarray(state, dtype=F64)
    r = np.asarray(reward, dtype=F32)
    g, carry_out, live = returns_forward(r, done, gamma, carry, mask, wrong)
    K = F64(0.0) if wrong == "pivot_dropped" else (state[1] if state[0] > 0.0 else F64(r[0, 0]))
    n_b, S1, S2 = sums(g, live, K)
    new, sc = fold(state, n_b, K, S1, S2, eps, wrong)
    return dict(state=new, scale=F32(scale) if sc is None else sc, carry=carry_out, g=g, K=K, sums=(n_b, S1, S2), live=live)


# ---- the scaled GAE
def scaled_reward(reward, scale, clip, wrong=None):
    r, s, c = np.asarray(reward, dtype=F32), F32(scale), F32(clip)
    with np.errstate(all="ignore"):
        if wrong == "clip_before_scale":
            if c != 0.0:
                r = np.where(r > c, c, np.where(r < -c, -c, r)).astype(F32)
            return (r * s).astype(F32)
        x = (r * s).astype(F32)
        if c != 0.0:
            x = np.where(x > c, c, np.where(x < -c, -c, x)).astype(F32)
    return x


def gae_stats(adv, live):
    """count, sum and sum of squares of the advantages in chub_rollout_gae_device's order: a lane t descending, then reduce_lanes"""
    T, N = adv.shape
    w = np.zeros((N, 3), dtype=F64)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            a = adv[t].astype(F64)
            w[:, 1] = w[:, 1] + a
            w[:, 2] = w[:, 2] + a * a
    w[:, 0] = float(T)
    w[~live] = 0.0
    return reduce_lanes(w)


def scaled_gae(reward, done, values, final_values, gamma, lam, scale, clip, mask=None, wrong=None):
    """-> (adv, ret [T, N] f32, stats [3] f64); masked-out envs' columns are NaN (not written)"""
    N = np.asarray(reward).shape[1]
    live = np.ones(N, dtype=bool) if mask is None else np.asarray(mask) != 0
    with np.errstate(all="ignore"):
        adv, ret = psl.gae_f32(scaled_reward(reward, scale, clip, wrong), done, values, final_values, gamma, lam)
    st = gae_stats(adv, live)
    adv[:, ~live] = np.nan
    ret[:, ~live] = np.nan
    return adv, ret, st


# ---- the state blob
def blob_of(N, state, scale, carry):
    b = np.zeros(BLOB_HEAD + 4 * N, dtype=np.uint8)
    b[:8].view(np.uint64)[0] = MAGIC
    b[8:16].view(np.int64)[0] = N
    b[16:40].view(F64)[:] = state
    b[40:44].view(F32)[0] = scale
    b[BLOB_HEAD:].view(F32)[:] = carry
    return b.tobytes()


def blob_parts(blob):
    b = np.frombuffer(bytes(blob), dtype=np.uint8)
    return (int(b[:8].view(np.uint64)[0]), int(b[8:16].view(np.int64)[0]), b[16:40].view(F64).copy(), b[40:44].view(F32)[0],
            b[BLOB_HEAD:].view(F32).copy())


# ---- the cases the GPU test runs (and on which the CPU test shows that each wrong= variant differs)
def done_pattern(kind, T, N, rs):
    d = np.zeros((T, N), dtype=bool)
    if kind == "all":
        d[:] = True
    elif kind == "first":
        d[0] = True
    elif kind == "last":
        d[T - 1] = True
    elif kind == "edge":  # either side of the first chunk's edge, forward in t: t = 7 closes chunk 0, t = 8 opens chunk 1
        d[min(AHEAD - 1, T - 1), 0::2] = True
        d[min(AHEAD, T - 1), 1::2] = True
    elif kind == "twice":
        for e in range(N):
            d[rs.choice(T, size=min(2, T), replace=False), e] = True
    elif kind == "random":
        d = rs.rand(T, N) < 0.2
    elif kind == "random9":  # random, and one within every nine steps: with gamma = 0.5 no value is halved more than nine times
        d = rs.rand(T, N) < 0.2
        for e in range(N):
            gap = 0
            for t in range(T):
                gap = 0 if d[t, e] else gap + 1
                if gap == AHEAD:
                    d[t, e], gap = True, 0
    else:
        assert kind == "none", kind
    return d


CASES = [
    dict(name="n1-t1-none-g1", N=1, T=1, done="none", gamma=1.0),
    dict(name="n1-t7-all-g05", N=1, T=7, done="all", gamma=0.5),
    dict(name="n255-t7-all-g05", N=255, T=7, done="all", gamma=0.5),
    dict(name="n256-t8-first-g1", N=256, T=8, done="first", gamma=1.0),
    dict(name="n257-t9-last-g1", N=257, T=9, done="last", gamma=1.0),
    dict(name="n513-t17-edge-g1", N=513, T=17, done="edge", gamma=1.0),
    dict(name="n256-t9-edge-g05", N=256, T=9, done="edge", gamma=0.5),
    dict(name="n257-t17-twice-g1", N=257, T=17, done="twice", gamma=1.0),
    dict(name="n513-t9-random-g05", N=513, T=9, done="random", gamma=0.5),
    dict(name="n256-t17-random9-g05", N=256, T=17, done="random9", gamma=0.5),
    dict(name="n255-t8-none-g05", N=255, T=8, done="none", gamma=0.5),
    dict(name="n513-t1-random-g1", N=513, T=1, done="random", gamma=1.0),
    dict(name="n257-t7-twice-g05", N=257, T=7, done="twice", gamma=0.5),
    dict(name="n513-t17-none-g1", N=513, T=17, done="none", gamma=1.0),
    # rewards 2^22 + halves, g = r exactly: the raw sum of squares needs 58 bits, the pivoted one 15 -- variant (f)'s case
    dict(name="n255-t7-all-g05-offset", N=255, T=7, done="all", gamma=0.5, offset=4194304.0),
]
EPS = 1e-8
OFFSET_CASE = "n255-t7-all-g05-offset"


def case_named(name):
    return next(c for c in CASES if c["name"] == name)


def case_arrays(case, carry=False, mask=False, seed=0):
    """reward [T, N] f32 (small integers and halves around the case's offset), done [T, N] bool, carry [N] f32 (integers) or None,
    mask [N] u8 or None (env 0 masked out: the pivot row serves all the same)"""
    rs = np.random.RandomState(9000 + CASES.index(case) + 100 * seed)
    T, N = case["T"], case["N"]
    reward = (rs.randint(-8, 9, size=(T, N)) / 2.0 + case.get("offset", 0.0)).astype(F32)
    done = done_pattern(case["done"], T, N, rs)
    c = rs.randint(-6, 7, size=N).astype(F32) if carry else None
    m = None
    if mask:
        m = (rs.rand(N) < 0.6).astype(np.uint8)
        m[0] = 0
        if N == 1:
            m[0] = 1
    return dict(reward=reward, done=done, carry=c, mask=m)


def packed_of(reward, done, D, seed=5):
    """blocks [T, N, D + 2] f32: observations of noise, the reward at column D, any non-zero where done fires at D + 1"""
    rs = np.random.RandomState(seed)
    T, N = reward.shape
    packed = rs.normal(size=(T, N, D + 2)).astype(F32)
    packed[:, :, D] = reward
    packed[:, :, D + 1] = np.where(done, rs.choice([1.0, 2.5, -1.0], size=(T, N)), 0.0)
    return packed


# ---- exactness: what makes "bit for bit from an empty state" independent of the order of the sums
def exact_returns(reward, done, gamma, carry=None):
    """the recurrence over exact rationals: g [T][N] Fractions and the carry out"""
    T, N = reward.shape
    gm = Fraction(float(F32(gamma)))
    out = [[None] * N for _ in range(T)]
    rest = []
    for e in range(N):
        g = Fraction(0) if carry is None else Fraction(float(carry[e]))
        for t in range(T):
            g = gm * g + Fraction(float(reward[t, e]))
            out[t][e] = g
            if done[t, e]:
                g = Fraction(0)
        rest.append(g)
    return out, rest


def prove_exact(case, arrays):
    """On the case's arrays from an EMPTY state: every g is an f32; with d = g - K all d and d d are multiples of one power of two, q, and
    sum |d| / q and sum d d / q^2 stay below 2^53, so EVERY partial sum of either, in any order, is an f64 held exactly.  Returns
    (g, carry, n_b, S1, S2) as Fractions / lists of them; raises AssertionError where the case is not exact."""
    r, d, carry, mask = arrays["reward"], arrays["done"], arrays["carry"], arrays["mask"]
    T, N = r.shape
    g, rest = exact_returns(r, d, case["gamma"], carry)
    live = np.ones(N, dtype=bool) if mask is None else mask != 0
    K = Fraction(float(r[0, 0]))
    dd = []
    for t in range(T):
        for e in range(N):
            assert Fraction(float(F32(float(g[t][e])))) == g[t][e], (case["name"], "g is no f32", t, e)
            if live[e]:
                dd.append(g[t][e] - K)
    for e in range(N):
        assert Fraction(float(F32(float(rest[e])))) == rest[e]
    den = max([x.denominator for x in dd] + [1])
    assert den & (den - 1) == 0
    assert sum(abs(x) for x in dd) * den < 2 ** 53, (case["name"], "S1 may round")
    assert sum(x * x for x in dd) * den * den < 2 ** 53, (case["name"], "S2 may round")
    return g, rest, len(dd), sum(dd), sum(x * x for x in dd)


# ---- 6.21's derived bounds, for an update that starts from a state that is not empty
def merge_bounds(state0, g, live):
    """(definition's (n, mean, M2) in exact rationals applied to the f64 state the call started from, bound on mean, bound on M2):
    mean: (R + 8) 2^-53 (max |d| + |mean|), M2: 4 (R + 8) 2^-53 (sum d d + M2), R the counted values of the call"""
    n0, mean0, m20 = (Fraction(float(x)) for x in state0)
    vals = [Fraction(float(x)) for x in g[:, live].ravel()]
    R = len(vals)
    K = mean0 if n0 > 0 else vals[0]
    d = [x - K for x in vals]
    S1, S2 = sum(d), sum(x * x for x in d)
    m2b = S2 - S1 * S1 / R
    n1 = n0 + R
    if n0 > 0:
        mean1 = K + S1 / n1
        m21 = m20 + m2b + (S1 / R) ** 2 * (n0 * R / n1)
    else:
        mean1, m21 = K + S1 / R, m2b
    u = (R + 8) * 2.0 ** -53
    return (float(n1), float(mean1), float(m21)), u * (float(max(abs(x) for x in d)) + abs(float(mean1))), 4 * u * (float(S2) + float(m21))
