"""The numpy definitions of include/chub.h's section "pile sets and advantages", and nothing else defines the expected values of
tests/test_pile_set_cpu.py and tests/test_gpu_pile_set.py: the three pile sets from the car / emergency columns, the log-probability over
a set (policy_sample_lib's terms and bounds with the skipped terms left out), the f32 GAE operation by operation, and an f64 textbook GAE
with a derived bound on what the f32 one may differ by.  The cases of both tests (hubs, seeds, GAE blocks) are made HERE."""
import numpy as np

import policy_lib as pl
import policy_sample_lib as ps

F32 = np.float32
U = pl.U
PSET_NAMES = ("all", "occupied", "decidable")
FORCED_ON = F32(1.01)  # judge_feasibility's threshold on a pile's emergency (CHS:1404-1413)

# the hubs of both tests: a small one, the flagship, two words / three output tiles, a full word with a station of 0 piles, the other station of 0
HUBS = ([3, 2], [20, 25], [40, 30], [64, 0], [0, 33])
N_ENVS = 70  # two full env tiles of the actor and one of 6


# ---- the sets
def sets_from_columns(car, emergency):
    """car, emergency [N, S] f32 (chub_pile_obs_device's columns, or the oracle's) -> {name: bool [N, S]}"""
    car, em = np.asarray(car, dtype=F32), np.asarray(emergency, dtype=F32)
    occupied = car != 0
    return {"all": np.ones(car.shape, dtype=bool), "occupied": occupied, "decidable": occupied & (em < FORCED_ON)}


def words(on):
    """bool [N, S] -> uint64 [N, ceil(S / 64)] in chub_step_bits' layout, bits from S up zero"""
    on = np.asarray(on, dtype=bool)
    n, S = on.shape
    W = (S + 63) // 64
    padded = np.zeros((n, W * 64), dtype=bool)
    padded[:, :S] = on
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(n, W).astype(np.uint64)


def sets_differ(sets, need_forced_on=False):
    """what every test asserts of its reference side: the three sets are not all equal over its envs (and a forced-on pile exists)"""
    assert not np.array_equal(sets["all"], sets["occupied"]), "every pile is occupied: the sets are all equal"
    if need_forced_on:
        assert (sets["occupied"] & ~sets["decidable"]).any(), "no forced-on pile in this state"


# ---- the log-probability over a set
def masked_logp(d, on, in_set):
    """d: policy_sample_lib.Sample; on bool [N, S]: the decisions taken; in_set bool [N, S] -> (value [N] f64, bound [N]).  Sample.logp's terms
    and error model with the piles outside the set left out: a left-out term contributes neither value nor rounding, and the chain is no
    longer than the full one"""
    on, m = np.asarray(on, dtype=bool), np.asarray(in_set, dtype=bool)
    eps, ls = d.eps.astype(np.float64), d.log_std
    x = np.where(on, -d.zp, d.zp)
    T = np.where(m, ps.softplus(x), 0.0)
    e = np.exp(-np.abs(x))
    err_pile = np.where(m, d.ezp + e * ps.EXP_ULP * ps.ULP + np.log1p(e) * ps.LOG1P_ULP * ps.ULP + 1.001 * U * (ps.softplus(x) + d.ezp), 0.0)
    g = -0.5 * eps * eps - ls - ps.HALF_LN_2PI
    err_g = 4.004 * U * (0.5 * eps * eps + np.abs(ls) + ps.HALF_LN_2PI)
    value = -T.sum(axis=1) + g.sum(axis=1)
    mag = T.sum(axis=1) + np.abs(g).sum(axis=1) + err_pile.sum(axis=1) + err_g.sum(axis=1)
    bound = err_pile.sum(axis=1) + err_g.sum(axis=1) + pl.gamma(d.S + d.G + 8) * mag
    return value, bound


def sampled_logp(z, on, u, log_std, in_set=None):
    """policy_sample_lib.sampled_logp over a set (None: every pile), f64"""
    z, u, ls = np.asarray(z, dtype=np.float64), np.asarray(u, dtype=np.float64), np.asarray(log_std, dtype=np.float64)
    S = np.shape(on)[1]
    eps = (u - z[:, S:]) / np.exp(ls)
    t = ps.softplus(np.where(on, -z[:, :S], z[:, :S]))
    if in_set is not None:
        t = np.where(in_set, t, 0.0)
    return -t.sum(axis=1) + (-0.5 * eps * eps - ls - ps.HALF_LN_2PI).sum(axis=1)


def sampled_entropy(z, log_std, in_set=None):
    """the Bernoulli entropy of the pile logits over a set (None: every pile) plus the Gaussian entropy, f64"""
    z, ls = np.asarray(z, dtype=np.float64), np.asarray(log_std, dtype=np.float64)
    S = z.shape[1] - ls.shape[0]
    zp = z[:, :S]
    h = ps.softplus(zp) - zp / (1.0 + np.exp(-zp))
    if in_set is not None:
        h = np.where(in_set, h, 0.0)
    return h.sum(axis=1) + (0.5 + ls + ps.HALF_LN_2PI).sum()


# ---- generalised advantage estimation
def gae_f32(reward, done, values, final_values, gamma, lam):
    """the header's recurrence, every operation a rounded f32 operation.  reward, done [T, N] f32 (done: non-zero fires), values [T + 1, N] f32,
    final_values [N] f32 or None -> (adv, ret) f32 [T, N]"""
    r, V = np.asarray(reward, dtype=F32), np.asarray(values, dtype=F32)
    d = np.asarray(done) != 0
    T, N = r.shape
    g = F32(gamma)
    gl = F32(g * F32(lam))
    fin = np.zeros(N, dtype=F32) if final_values is None else np.asarray(final_values, dtype=F32)
    adv, ret = np.zeros((T, N), dtype=F32), np.zeros((T, N), dtype=F32)
    nxt = np.zeros(N, dtype=F32)
    for t in range(T - 1, -1, -1):
        vn = np.where(d[t], fin, V[t + 1]).astype(F32)
        delta = (F32(r[t] + F32(g * vn)) - V[t]).astype(F32)
        nxt = (delta + F32(gl * np.where(d[t], F32(0), nxt).astype(F32))).astype(F32)
        adv[t] = nxt
        ret[t] = (nxt + V[t]).astype(F32)
    return adv, ret


def gae_f64(reward, done, values, final_values, gamma, lam):
    """the textbook form in f64: adv[t] = sum_k (gamma lam)^k delta[t + k] over k = 0 .. up to and including the first step at which done fires
    (or T - 1), delta[t] = r[t] + gamma vn[t] - V[t].  gamma and lam are the f32 values the device is given; their product is exact in f64."""
    r, V = np.asarray(reward, dtype=np.float64), np.asarray(values, dtype=np.float64)
    d = np.asarray(done) != 0
    T, N = r.shape
    g, gl = float(F32(gamma)), float(F32(gamma)) * float(F32(lam))
    fin = np.zeros(N) if final_values is None else np.asarray(final_values, dtype=np.float64)
    delta = r + g * np.where(d, fin[None, :], V[1:]) - V[:-1]
    adv = np.zeros((T, N))
    for t in range(T):
        alive = np.ones(N, dtype=bool)
        for k in range(T - t):
            adv[t] += np.where(alive, gl ** k * delta[t + k], 0.0)
            alive &= ~d[t + k]
    return adv, adv + V[:-1]


def gae_bound(reward, done, values, final_values, gamma, lam, adv32, ret32):
    """|gae_f32 - gae_f64| <= (bound_adv, bound_ret), from the f32 values held.  With u = 2^-24 and every f32 result fl(x) = x (1 + e), |e| <= u:
      delta: three roundings over r, gamma vn and V                     -> D[t] = gamma_3 (|r| + gamma |vn| + |V[t]|)
      gl32 = fl(gamma lam) = gl (1 + e0); p = fl(gl32 a') = gl a' (1 + e0)(1 + e1); a = fl(delta32 + p):
      E[t] <= D[t] + gl E[t + 1] + 2.001 u gl |a32[t + 1]| + 1.001 u |a32[t]|, E[T] = 0 and a done step cuts the chain
      ret = fl(a + V): E[t] + 1.001 u |ret32[t]|
    plus one subnormal step per operation, and the f64 side's own rounding (T terms of relative 2^-52 each, far below)"""
    r, V = np.abs(np.asarray(reward, dtype=np.float64)), np.abs(np.asarray(values, dtype=np.float64))
    d = np.asarray(done) != 0
    T, N = r.shape
    g, gl = float(F32(gamma)), float(F32(gamma)) * float(F32(lam))
    fin = np.zeros(N) if final_values is None else np.abs(np.asarray(final_values, dtype=np.float64))
    a32, r32 = np.abs(np.asarray(adv32, dtype=np.float64)), np.abs(np.asarray(ret32, dtype=np.float64))
    D = pl.gamma(3) * (r + g * np.where(d, fin[None, :], V[1:]) + V[:-1])
    E = np.zeros((T + 1, N))
    a_next = np.zeros(N)
    for t in range(T - 1, -1, -1):
        carry = np.where(d[t], 0.0, gl * E[t + 1] + 2.001 * U * gl * a_next)
        E[t] = D[t] + carry + 1.001 * U * a32[t] + 5 * pl.TINY
        a_next = a32[t]
    scale = (r + V[:-1] + V[1:] + fin[None, :]).max() * T + 1.0
    E = E[:T] * (1 + 1e-9) + 2.0 ** -45 * scale
    return E, E + 1.001 * U * r32 + pl.TINY


GAE_T = (1, 5, 96)
GAE_DONES = ("first", "last", "nowhere")
GAE_FACTORS = ((0.99, 0.95), (1.0, 1.0), (0.0, 0.0))


def gae_case(T, dones, with_final, N=N_ENVS, D=13, seed=0):
    """synthetic blocks: packed [T, N, D + 2] f32 with rewards of the hub's size and done at t = 0 / t = T - 1 for a third of the envs each way
    (`dones`: "first", "last", "nowhere"), values [T + 1, N], final_values [N] or None"""
    rs = np.random.RandomState(1000 * T + 10 * GAE_DONES.index(dones) + int(with_final) + seed)
    packed = rs.normal(size=(T, N, D + 2)).astype(F32)
    packed[:, :, D] = (rs.normal(size=(T, N)) * 3.0 - 1.0).astype(F32)
    packed[:, :, D + 1] = 0
    if dones == "first":
        packed[0, rs.rand(N) < 0.4, D + 1] = 1
    elif dones == "last":
        packed[T - 1, rs.rand(N) < 0.4, D + 1] = 1
    values = (rs.normal(size=(T + 1, N)) * 5.0).astype(F32)
    final = (rs.normal(size=N) * 5.0).astype(F32) if with_final else None
    return packed, values, final


def stats_of(adv):
    """count, sum and sum of squares of the advantages as math.fsum gives them, and the header's bound n 2^-53 sum |x| for sum and squares"""
    import math
    x = np.asarray(adv, dtype=np.float64).ravel()
    n = x.size
    return (float(n), math.fsum(x), math.fsum(x * x)), (0.0, n * 2.0 ** -53 * float(np.abs(x).sum()), n * 2.0 ** -53 * float((x * x).sum()))
