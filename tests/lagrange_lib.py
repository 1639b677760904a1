"""Constrained PPO on the device (include/chub.h, "constrained PPO on the device") restated in numpy, operation for operation: the cost
GAE and the episode costs of chub_lagrange_gae_device with its reduction order, the multiplier's step rule and the combined advantage.
f32 arithmetic is numpy float32 arithmetic (every operation rounded once), the sums are f64 in the order the header states.  `wrong=` switches
one deliberate mistake on, for the failure experiment of tests/test_lagrange_cpu.py; the case lists below are what the GPU test runs."""
import numpy as np

F32, F64 = np.float32, np.float64
LANES, AHEAD, COMBINE_BLOCKS = 256, 8, 2048
STEP, AT_DONE = 0, 1
WRONG = ("at_done_every_step", "carry_dropped", "open_segment_counted", "clamp_before_increment", "not_centred", "zero_lambda_not_skipped")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == F32 else np.uint64)


# ---- the cost GAE
def costs_of(terms, done, column, kind, wrong=None):
    """c_t [T, N] f32: the column's value; under AT_DONE exactly +0.0f where done does not fire"""
    c = np.ascontiguousarray(terms[:, :, column], dtype=F32)
    if kind == AT_DONE and wrong != "at_done_every_step":
        c = np.where(done, c, F32(0.0)).astype(F32)
    return c


def tree(lanes):
    """[blocks, 256, W] -> [blocks, W]: lane l takes lane l + h, h = 128 .. 1"""
    a = np.array(lanes, dtype=F64)
    h = LANES // 2
    while h > 0:
        a[:, :h] = a[:, :h] + a[:, h:2 * h]
        h //= 2
    return a[:, 0]


def reduce_lanes(w):
    """per-env words [N, W] f64 -> (stats [W], partials [blocks, W]) in the kernel's order: the workgroups' trees, then lane l of the merge
    takes partials l, l + 256, .. ascending from 0, then the same tree"""
    N, W = w.shape
    blocks = (N + LANES - 1) // LANES
    lanes = np.zeros((blocks * LANES, W), dtype=F64)
    lanes[:N] = w
    partials = tree(lanes.reshape(blocks, LANES, W))
    acc = np.zeros((LANES, W), dtype=F64)
    for b in range(blocks):
        acc[b % LANES] = acc[b % LANES] + partials[b]
    return tree(acc[None])[0], partials


def cost_gae(terms, done, constraints, gamma, lam, values=None, finals=None, mask=None, carry=None, wrong=None):
    """terms [T, N, C] f32, done [T, N] (non-zero fires), constraints [(column, kind)], values / finals: per constraint [T + 1, N] / [N] f32 or
    None, mask [N] or None, carry [N, K] f64 or None -> dict(adv, ret: lists of [T, N] f32 (rows of masked-out envs are NaN: not written),
    carry [N, K] f64, stats [K, 6] f64, lanes [K][N, 6] the per-env words)"""
    terms = np.asarray(terms, dtype=F32)
    d = np.asarray(done) != 0
    T, N, _ = terms.shape
    K = len(constraints)
    live = np.ones(N, dtype=bool) if mask is None else np.asarray(mask) != 0
    g = F32(gamma)
    gl = F32(g * F32(lam))
    out = dict(adv=[], ret=[], carry=np.zeros((N, K)) if carry is None else np.array(carry, dtype=F64), stats=np.zeros((K, 6)), lanes=[])
    for k, (column, kind) in enumerate(constraints):
        c = costs_of(terms, d, column, kind, wrong)
        V = np.zeros((T + 1, N), dtype=F32) if values is None or values[k] is None else np.asarray(values[k], dtype=F32)
        fin = np.zeros(N, dtype=F32) if finals is None or finals[k] is None else np.asarray(finals[k], dtype=F32)
        adv, ret = np.full((T, N), np.nan, dtype=F32), np.full((T, N), np.nan, dtype=F32)
        a, v_next = np.zeros(N, dtype=F32), V[T]
        seg, is_open, carry_out = np.zeros(N), np.ones(N, dtype=bool), np.zeros(N)
        w = np.zeros((N, 6))
        with np.errstate(all="ignore"):
            for t in range(T - 1, -1, -1):
                vn = np.where(d[t], fin, v_next).astype(F32)
                delta = (F32(c[t] + F32(g * vn)) - V[t]).astype(F32)
                a = (delta + F32(gl * np.where(d[t], F32(0), a).astype(F32))).astype(F32)
                adv[t], ret[t] = a, (a + V[t]).astype(F32)
                a64 = a.astype(F64)
                w[:, 1] = w[:, 1] + a64
                w[:, 2] = w[:, 2] + a64 * a64
                v_next = V[t]
                closes = d[t] if wrong == "open_segment_counted" else d[t] & ~is_open
                carry_out = np.where(d[t] & is_open, seg, carry_out)
                w[:, 3] = np.where(closes, w[:, 3] + 1.0, w[:, 3])
                w[:, 4] = np.where(closes, w[:, 4] + seg, w[:, 4])
                w[:, 5] = np.where(closes, w[:, 5] + seg * seg, w[:, 5])
                seg = np.where(d[t], c[t].astype(F64), seg + c[t].astype(F64))
                is_open = is_open & ~d[t]
            carry_in = np.zeros(N) if carry is None or wrong == "carry_dropped" else np.asarray(carry, dtype=F64)[:, k]
            x = carry_in + seg
            carry_out = np.where(is_open, x, carry_out)
            w[:, 3] = np.where(is_open, w[:, 3], w[:, 3] + 1.0)
            w[:, 4] = np.where(is_open, w[:, 4], w[:, 4] + x)
            w[:, 5] = np.where(is_open, w[:, 5], w[:, 5] + x * x)
        w[:, 0] = float(T)
        w[~live] = 0.0
        adv[:, ~live] = np.nan
        ret[:, ~live] = np.nan
        out["carry"][live, k] = carry_out[live]
        out["adv"].append(adv)
        out["ret"].append(ret)
        out["lanes"].append(w)
        out["stats"][k] = reduce_lanes(w)[0]
    return out


def episode_costs_forward(cost, done, carry_in=None):
    """a plain forward loop over one constraint's costs [T, N]: (the finished episodes' costs per env as lists of Fractions, the open
    remainder per env) -- exact rationals, for data whose sums are exact"""
    from fractions import Fraction
    T, N = cost.shape
    finished, rest = [[] for _ in range(N)], []
    for e in range(N):
        acc = Fraction(0) if carry_in is None else Fraction(float(carry_in[e]))
        for t in range(T):
            acc += Fraction(float(cost[t, e]))
            if done[t, e]:
                finished[e].append(acc)
                acc = Fraction(0)
        rest.append(acc)
    return finished, rest


# ---- the multiplier's step
def lagrange_step(lam, words, stats, limit, lr, lambda_max, wrong=None):
    """one constraint: lam float, words [J_last, taken, skipped], stats [6] -> (lam, words), f64, every operation rounded once"""
    lam, w, st = F64(lam), np.array(words, dtype=F64), np.asarray(stats, dtype=F64)
    with np.errstate(all="ignore"):
        n = st[3]
        J = st[4] / n
        if n == 0.0 or not np.isfinite(J):
            w[2] = w[2] + 1.0
            return lam, w
        if wrong == "clamp_before_increment":
            l = F64(0.0) if lam < 0.0 else lam
            if lambda_max != 0.0 and l > lambda_max:
                l = F64(lambda_max)
            l = l + F64(lr) * (J - F64(limit))
        else:
            l = lam + F64(lr) * (J - F64(limit))
            l = F64(0.0) if l < 0.0 else l
            if lambda_max != 0.0:
                l = F64(lambda_max) if l > lambda_max else l
    if l != l:
        w[2] = w[2] + 1.0
        return lam, w
    w[1] = w[1] + 1.0
    w[0] = J
    return l, w


# ---- the combined advantage
def advantage_normaliser(adv_stats):
    """(m32, s32) of chub_policy_grad_device's "Advantage" paragraph"""
    cnt, s, q = (F64(x) for x in adv_stats)
    with np.errstate(all="ignore"):
        m = s / cnt
        var = q / cnt - m * m
        var = var if var > 0.0 else F64(0.0)
        return F32(m), F32(F64(1.0) / np.sqrt(var + F64(1e-8)))


def combine(adv, adv_stats, cost_advs, lam, stats, wrong=None):
    """adv [n] f32, adv_stats [3] f64 or None, cost_advs [K][n] f32, lam [K] f64, stats [K, 6] f64 -> out [n] f32"""
    a = np.array(adv, dtype=F32).ravel()
    with np.errstate(all="ignore"):
        if adv_stats is not None:
            m32, s32 = advantage_normaliser(adv_stats)
            a = ((a - m32).astype(F32) * s32).astype(F32)
        total = F64(0.0)
        for k, c in enumerate(cost_advs):
            l32 = F32(F64(lam[k]))
            total = total + F64(l32)
            if l32 == 0.0 and wrong != "zero_lambda_not_skipped":
                continue
            mc32 = F32(F64(stats[k][1]) / F64(stats[k][0]))
            centred = np.asarray(c, dtype=F32).ravel() if wrong == "not_centred" else (np.asarray(c, dtype=F32).ravel() - mc32).astype(F32)
            a = (a - (l32 * centred).astype(F32)).astype(F32)
        inv32 = F32(F64(1.0) / (F64(1.0) + total))
        return (a * inv32).astype(F32)


# ---- the cases the GPU test runs (and on which the CPU test shows that each wrong= variant differs)
def done_pattern(kind, T, N, rs):
    d = np.zeros((T, N), dtype=bool)
    if kind == "all":
        d[:] = True
    elif kind == "first":
        d[0] = True
    elif kind == "last":
        d[T - 1] = True
    elif kind == "edge":  # either side of the first look-ahead chunk's edge: the chunk from the top holds t = T - 1 .. T - AHEAD
        lo = max(T - AHEAD, 0)
        d[lo, 0::2] = True
        d[max(lo - 1, 0), 1::2] = True
    elif kind == "twice":
        for e in range(N):
            d[rs.choice(T, size=min(2, T), replace=False), e] = True
    elif kind == "random":
        d = rs.rand(T, N) < 0.2
    else:
        assert kind == "none", kind
    return d


S, A = STEP, AT_DONE
GAE_CASES = [
    dict(name="n1-t1-k1-c1-none", N=1, T=1, C=1, cons=[(0, S)], done="none", values=[False], finals=[False]),
    dict(name="n1-t9-k2-c3-last-carry", N=1, T=9, C=3, cons=[(2, A), (0, S)], done="last", values=[True, False], finals=[True, False], carry=True),
    dict(name="n255-t7-k2-c3-all", N=255, T=7, C=3, cons=[(0, S), (2, A)], done="all", values=[True, True], finals=[True, True]),
    dict(name="n256-t8-k4-c27-first", N=256, T=8, C=27, cons=[(0, S), (26, A), (12, S), (12, A)], done="first", values=[True, False, True, False],
         finals=[False] * 4, carry=True),
    dict(name="n257-t9-k2-c27-last", N=257, T=9, C=27, cons=[(26, A), (0, S)], done="last", values=[False, True], finals=[False, True]),
    dict(name="n513-t17-k4-c3-edge", N=513, T=17, C=3, cons=[(0, S), (1, A), (2, S), (1, S)], done="edge", values=[True] * 4,
         finals=[True, False, True, False], carry=True),
    dict(name="n257-t17-k1-c1-twice", N=257, T=17, C=1, cons=[(0, A)], done="twice", values=[True], finals=[True], carry=True),
    dict(name="n513-t9-k2-c3-random-mask", N=513, T=9, C=3, cons=[(1, S), (2, A)], done="random", values=[True, True], finals=[False, True],
         carry=True, mask=True),
    dict(name="n256-t17-k2-c3-random-noret", N=256, T=17, C=3, cons=[(2, S), (0, A)], done="random", values=[True, False], finals=[True, False],
         ret=False),
    dict(name="n255-t8-k1-c3-none-carry", N=255, T=8, C=3, cons=[(1, S)], done="none", values=[False], finals=[False], carry=True),
    dict(name="n513-t1-k4-c27-random", N=513, T=1, C=27, cons=[(0, A), (26, S), (13, A), (0, S)], done="random", values=[True, False, False, True],
         finals=[True] * 4, carry=True),
    dict(name="n257-t7-k3-c3-twice-mask", N=257, T=7, C=3, cons=[(0, S), (1, A), (2, A)], done="twice", values=[True] * 3, finals=[True] * 3,
         carry=True, mask=True),
]
GAMMA, LAM = 0.99, 0.95


def gae_case(case, seed=0):
    """the case's arrays: terms (small integers and halves), done, values, finals, mask, carry (integers)"""
    rs = np.random.RandomState(4000 + GAE_CASES.index(case) + 100 * seed)
    T, N, C, K = case["T"], case["N"], case["C"], len(case["cons"])
    terms = (rs.randint(0, 9, size=(T, N, C)) / 2.0).astype(F32)
    done = done_pattern(case["done"], T, N, rs)
    values = [(rs.normal(size=(T + 1, N)) * 3.0).astype(F32) if g else None for g in case["values"]]
    finals = [(rs.normal(size=N) * 3.0).astype(F32) if g else None for g in case["finals"]]
    mask = (rs.rand(N) < 0.6).astype(np.uint8) if case.get("mask") else None
    carry = rs.randint(1, 20, size=(N, K)).astype(F64) if case.get("carry") else None
    return dict(terms=terms, done=done, values=values, finals=finals, mask=mask, carry=carry)


def step_cases():
    """name -> dict(lam, words, stats, limit, lr, lambda_max): made stats for the step rule"""
    st = lambda n, s: np.array([960.0, 12.5, 99.0, n, s, s * s], dtype=F64)
    return {
        "ordinary": dict(lam=0.25, words=[0.0, 3.0, 1.0], stats=st(8.0, 36.0), limit=4.0, lr=0.05, lambda_max=10.0),
        "no_episode": dict(lam=0.25, words=[1.5, 3.0, 1.0], stats=st(0.0, 0.0), limit=4.0, lr=0.05, lambda_max=10.0),
        "floor": dict(lam=0.1, words=[0.0, 0.0, 0.0], stats=st(4.0, 2.0), limit=5.5, lr=0.1, lambda_max=10.0),
        "ceiling": dict(lam=9.9, words=[0.0, 7.0, 0.0], stats=st(2.0, 50.0), limit=1.0, lr=0.5, lambda_max=10.0),
        "nan_cost": dict(lam=0.25, words=[2.0, 3.0, 1.0], stats=st(3.0, np.nan), limit=4.0, lr=0.05, lambda_max=10.0),
        "infinite_cost": dict(lam=0.25, words=[2.0, 3.0, 1.0], stats=st(3.0, np.inf), limit=4.0, lr=0.05, lambda_max=10.0),
        "no_ceiling": dict(lam=9.9, words=[0.0, 7.0, 0.0], stats=st(2.0, 50.0), limit=1.0, lr=0.5, lambda_max=0.0),
        "at_the_limit": dict(lam=0.75, words=[0.0, 1.0, 0.0], stats=st(5.0, 20.0), limit=4.0, lr=0.3, lambda_max=0.0),
    }


COMBINE_CASES = [
    dict(name="n1-zeros", n=1, lam=[0.0, 0.0, 0.0], stats=True),
    dict(name="n255-mixed", n=255, lam=[0.5, 0.0, 2.0], stats=True),
    dict(name="n257-mixed-in-place", n=257, lam=[0.5, 0.0, 2.0], stats=True, in_place=True),
    dict(name="n257-zeros-no-stats-signed-zeros", n=257, lam=[0.0, 0.0, 0.0], stats=False, signed_zeros=True),
    dict(name="past-a-grid-pass-mixed", n=COMBINE_BLOCKS * LANES + 1, lam=[0.5, 0.0, 2.0], stats=True),
    dict(name="n255-zeros-stats", n=255, lam=[0.0, 0.0, 0.0], stats=True),
]


def combine_case(case):
    """adv [n], adv_stats [3] or None (the true count, sum and sum of squares in f64), cost_advs [3][n]"""
    rs = np.random.RandomState(7000 + COMBINE_CASES.index(case))
    n = case["n"]
    adv = (rs.normal(size=n) * 2.0 + 0.3).astype(F32)
    if case.get("signed_zeros"):
        adv[::3] = F32(-0.0)
        adv[1::3] = F32(0.0)
    costs = [(rs.normal(size=n) * (k + 1.0) + 1.5).astype(F32) for k in range(len(case["lam"]))]
    a64 = adv.astype(F64)
    adv_stats = np.array([float(n), a64.sum(), (a64 * a64).sum()]) if case["stats"] else None
    return adv, adv_stats, costs
