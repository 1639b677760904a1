"""The numpy definition of SAMPLING from the device actor (include/chub.h, "sampling from the device actor"), and nothing else defines the
expected values of tests/test_policy_sample_cpu.py and tests/test_gpu_policy_sample.py: the Philox block (a vectorised restatement, held
to the oracle's orc_philox4x32_10 by the CPU test), the tabulated normal restated in f32 operation by operation, the pile draw, the
Gaussian sample and the log-probability in f64, and rigorous bounds on what a conforming device may differ by, in the style of
policy_lib.forward.  The cases of the GPU tests (seeds, keys, shapes) are made HERE, so that the CPU test can hold the definition alone to
the same caps on the same data."""
import os

import numpy as np

import orclib
import policy_lib as pl

F32 = np.float32
U = pl.U                  # unit roundoff of f32
ULP = 2.0 ** -23          # the relative size of one ulp of an f32 result, at most
# Errors of the device library's functions, in ulp.  No table of them is installed with the device library; these are the OpenCL
# full-profile limits its functions are written to meet (expf 3, log1pf 2; the HIP programming guide's own table lists less).
# tanhf is policy_lib.TANH_ERR.  The division is __fdiv_rn: correctly rounded, 1/2 ulp.
EXP_ULP = 3
LOG1P_ULP = 2
SITE_POLICY = 15
HALF_LN_2PI = 0.5 * np.log(2.0 * np.pi)


# ---- Philox4x32-10
def philox(c0, c1, c2, c3, k0, k1):
    """counter words (arrays or scalars, broadcast together) under key (k0, k1) -> uint32 [..., 4]"""
    c = [np.asarray(x, dtype=np.uint64) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    M32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        c = [h1 ^ c[1] ^ k0, l1, h0 ^ c[3] ^ k1, l0]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, axis=-1).astype(np.uint32)


def noise_words(key, tick, gids, S, G):
    """the policy's noise for global env ids `gids` at Philox tick `tick`: (pile words uint32 [N, S], Gaussian words uint32 [N, G]).
    Pile b: word b & 3 of block b >> 2, kind 0.  Gaussian i: word i of block 0, kind 1.  Counter (block, 15 << 16 | kind, tick, gid)."""
    gids = np.asarray(gids, dtype=np.uint64)
    k0, k1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    nblk = (S + 3) // 4
    if nblk:
        blocks = philox(np.arange(nblk, dtype=np.uint64)[None, :], SITE_POLICY << 16, int(tick) & 0xFFFFFFFF, gids[:, None], k0, k1)
        piles = blocks.reshape(len(gids), nblk * 4)[:, :S]
    else:
        piles = np.zeros((len(gids), 0), dtype=np.uint32)
    gauss = philox(0, (SITE_POLICY << 16) | 1, int(tick) & 0xFFFFFFFF, gids, k0, k1)[:, :G]
    return np.ascontiguousarray(piles), np.ascontiguousarray(gauss)


# ---- the tabulated normal, every operation a rounded f32 operation
_TABLES = []


def normal_tables():
    if not _TABLES:
        for name in ("normal_icdf_4097.f32", "normal_tail_4097.f32"):
            t = np.fromfile(os.path.join(orclib.DATA_DIR, name), dtype="<f4")
            assert t.shape == (4097,)
            _TABLES.append(t.astype(F32))
    return _TABLES


def normal_from_word(w):
    """uint32 words -> f32 N(0,1): 4096 cells of the inverse CDF, linear inside a cell; the outer 16 cells on either side through the
    second table with cells of 2^-20 (the upper ones by symmetry)"""
    tz, tl = normal_tables()
    w = np.asarray(w, dtype=np.uint32)
    cell = w >> np.uint32(20)
    hi, lo = cell >= 4096 - 16, cell < 16
    m = np.where(hi, ~w, w)
    tail = hi | lo
    idx = np.where(tail, m >> np.uint32(12), cell).astype(np.int64)
    frac = np.where(tail, (m & np.uint32(0xFFF)).astype(F32) * F32(1.0 / 4096.0), (w & np.uint32(0xFFFFF)).astype(F32) * F32(1.0 / 1048576.0)).astype(F32)
    a, b = np.where(tail, tl[idx], tz[idx]).astype(F32), np.where(tail, tl[idx + 1], tz[idx + 1]).astype(F32)
    z = (a + ((b - a).astype(F32) * frac).astype(F32)).astype(F32)
    return np.where(hi, -z, z).astype(F32)


# ---- the pre-squash outputs z and their bound
def pre_squash(x, layers, hidden_act="tanh"):
    """x [N, F] f32 (normalised) -> (z, err_z), f64 [N, outputs]: the last layer's PRE-squash outputs and policy_lib.forward's bound for them
    (the chain's gamma term over the values held, the incoming error through |W|)"""
    if len(layers) > 1:
        h, err = pl.forward(x, layers[:-1], hidden_act, hidden_act)
    else:
        h, err = np.asarray(x, dtype=np.float64), np.zeros(np.shape(x))
    W, b = np.asarray(layers[-1][0], dtype=np.float64), np.asarray(layers[-1][1], dtype=np.float64)
    K = W.shape[1]
    z = h @ W.T + b
    err_z = pl.gamma(K + 2) * (np.abs(b) + (np.abs(h) + err) @ np.abs(W).T) + err @ np.abs(W).T + K * pl.TINY
    return z, err_z


def squash64(u, squash):
    return np.tanh(u) if squash == "tanh" else np.minimum(np.maximum(u, -1.0), 1.0)


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


class Sample(object):
    """the definition on one batch.  z, err_z [N, A_out] f64 from pre_squash; head "piles" (S logits, then the two tail means) or "loads"
    (four means); gids the global env ids; log_std [G].
      U [N, S] f64 (exact), p [N, S] f64, bound_p, on = U < p, decided = |U - p| > bound_p
      eps [N, G] f32 (the device's bits), u [N, G] f64, bound_u
      logp(on) -> (value [N] f64, bound [N]) for the pile decisions `on` actually taken"""

    def __init__(self, z, err_z, head, S, key, tick, gids, log_std):
        z, err_z = np.asarray(z, dtype=np.float64), np.asarray(err_z, dtype=np.float64)
        self.S = S = S if head == "piles" else 0
        self.G = G = 2 if head == "piles" else 4
        self.log_std = ls = np.asarray(log_std, dtype=F32).astype(np.float64)
        assert ls.shape == (G,) and z.shape[1] == S + G
        pw, gw = noise_words(key, tick, gids, S, G)
        self.zp, self.ezp, self.zg, self.ezg = z[:, :S], err_z[:, :S], z[:, S:], err_z[:, S:]
        # piles
        self.U = (pw >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        with np.errstate(over="ignore"):
            self.p = p = 1.0 / (1.0 + np.exp(-self.zp))
        # |dp/dz| <= 1/4; expf's relative error reaches p through p (1 - p); the sum 1 + e and the quotient are each rounded once
        self.bound_p = self.ezp / 4 + p * (1 - p) * EXP_ULP * ULP * 1.01 + p * 2.01 * U + pl.TINY
        self.on = self.U < p
        self.decided = np.abs(self.U - p) > self.bound_p
        # Gaussians
        self.eps = normal_from_word(gw)
        eps = self.eps.astype(np.float64)
        sigma = np.exp(ls)
        self.u = self.zg + sigma * eps
        # sigma = expf(log_std) within EXP_ULP ulp, the product and the sum each rounded once (the sum over the values the device holds)
        self.bound_u = self.ezg + np.abs(sigma * eps) * (EXP_ULP * ULP + 2 * U) + 1.001 * U * (np.abs(self.zg) + self.ezg + np.abs(sigma * eps)) + pl.TINY

    def logp(self, on=None):
        on = self.on if on is None else np.asarray(on, dtype=bool)
        eps, ls = self.eps.astype(np.float64), self.log_std
        x = np.where(on, -self.zp, self.zp)
        T = softplus(x)                                     # a pile's term is -T
        e = np.exp(-np.abs(x))
        # softplus is 1-Lipschitz; expf's error reaches log1p's argument, d log1p(e) <= de; log1pf's own ulps; the sum max(x, 0) + l rounded
        err_pile = self.ezp + e * EXP_ULP * ULP + np.log1p(e) * LOG1P_ULP * ULP + 1.001 * U * (T + self.ezp)
        g = -0.5 * eps * eps - ls - HALF_LN_2PI
        # eps is the device's own bits; eps^2, the two differences and the constant are each rounded once
        err_g = 4.004 * U * (0.5 * eps * eps + np.abs(ls) + HALF_LN_2PI)
        value = -T.sum(axis=1) + g.sum(axis=1)
        mag = T.sum(axis=1) + np.abs(g).sum(axis=1) + err_pile.sum(axis=1) + err_g.sum(axis=1)
        # the chain: one addition per term, the half-waves' shuffle and the waves' partials -- fewer than S + G + 8 additions in any order
        bound = err_pile.sum(axis=1) + err_g.sum(axis=1) + pl.gamma(self.S + self.G + 8) * mag
        return value, bound


def sampled_logp(z, on, u, log_std):
    """the log-probability as a trainer evaluates it from recorded data, in f64: z [N, S + G] pre-squash outputs, on bool [N, S], u [N, G] the
    recorded pre-squash samples, eps = (u - z_gauss) / exp(log_std)"""
    z, u, ls = np.asarray(z, dtype=np.float64), np.asarray(u, dtype=np.float64), np.asarray(log_std, dtype=np.float64)
    S = np.shape(on)[1]
    eps = (u - z[:, S:]) / np.exp(ls)
    x = np.where(on, -z[:, :S], z[:, :S])
    return -softplus(x).sum(axis=1) + (-0.5 * eps * eps - ls - HALF_LN_2PI).sum(axis=1)


# ---- the law: what the statistical checks of the GPU test assert, on whatever made the draws
LAW_N, LAW_LOGITS, LAW_KEY, LAW_LOG_STD = 4096, (-2.0, 0.0, 1.5), 0x5EED0000C0FFEE, (-0.5, 0.25)


def law_layers(D, S):
    """zero weights, biases giving pile b the logit LAW_LOGITS[b % 3] and the tail means 0.25, -0.5"""
    b = np.array([LAW_LOGITS[k % 3] for k in range(S)] + [0.25, -0.5], dtype=F32)
    return [(np.zeros((S + 2, D), dtype=F32), b)]


def check_law(on, eps, logp, S):
    """on bool [N, S], eps [N, 2] (recovered (u - z) / sigma), logp [N]: every assertion within 5 standard errors"""
    n = len(on)
    logits = np.array([LAW_LOGITS[k % 3] for k in range(S)])
    p = 1.0 / (1.0 + np.exp(-logits))
    for v in LAW_LOGITS:
        cols = logits == v
        cnt, pv = n * int(cols.sum()), 1.0 / (1.0 + np.exp(-v))
        rate = on[:, cols].mean()
        assert abs(rate - pv) <= 5 * np.sqrt(pv * (1 - pv) / cnt), ("on-rate of logit", v, rate, pv)
    e = np.asarray(eps, dtype=np.float64).ravel()
    assert abs(e.mean()) <= 5 / np.sqrt(e.size), ("mean of eps", e.mean())
    # Var(eps^2) = E eps^4 - 1 = 2 for a normal: the sample variance's standard error is sqrt(2 / n)
    assert abs(e.var() - 1.0) <= 5 * np.sqrt(2.0 / e.size), ("variance of eps", e.var())
    ls = np.asarray(LAW_LOG_STD, dtype=np.float64)
    entropy = -(p * np.log(p) + (1 - p) * np.log(1 - p)).sum() + (0.5 + ls + HALF_LN_2PI).sum()
    # Var(logp) = sum_b p (1 - p) z_b^2 (a Bernoulli's log-odds) + 1/2 per Gaussian (Var(eps^2 / 2))
    var = (p * (1 - p) * logits ** 2).sum() + 0.5 * len(ls)
    m = np.asarray(logp, dtype=np.float64).mean()
    assert abs(m + entropy) <= 5 * np.sqrt(var / n), ("mean of logp against minus the entropy", m, -entropy)


# ---- the GPU test's cases, made here so that the CPU test sees the same data
EXACT_HUBS = ([20, 25], [1, 1], [64, 64])
GENERAL = (([20, 25], (64, 64)), ([1, 1], (33, 33)))
N_SMALL = 70
KEY = 0x0123456789ABCDEF


def obs_dim(piles):
    return 2 + 4 * sum(1 for p in piles if p > 0) + 3


def exact_case(piles, head="piles"):
    """relu / clip on dyadic data: z is bit-exact.  -> (layers, obs [70, D], log_std)"""
    rs = np.random.RandomState(101 + sum(piles))
    D, S = obs_dim(piles), sum(piles)
    layers = pl.exact_layers(rs, [D, 33, S + 2 if head == "piles" else 4])
    obs = pl.exact_obs(rs, N_SMALL, D)
    pl.assert_exact(obs, layers)
    return layers, obs, np.array([-1.0, -0.5, 0.0, 0.25][:2 if head == "piles" else 4], dtype=F32)


def general_case(piles, hidden, head="piles"):
    """Gaussian weights scaled by 1 / sqrt(fan-in), Gaussian observations -> (layers, obs [70, D], log_std)"""
    rs = np.random.RandomState(202 + sum(piles))
    D, S = obs_dim(piles), sum(piles)
    sizes = [D] + list(hidden) + [S + 2 if head == "piles" else 4]
    layers = [((rs.normal(size=(o, i)) / np.sqrt(i)).astype(F32), (rs.normal(size=o) * 0.1).astype(F32)) for i, o in zip(sizes[:-1], sizes[1:])]
    obs = rs.normal(size=(N_SMALL, D)).astype(F32)
    return layers, obs, np.array([-0.7, 0.1, -0.2, 0.3][:2 if head == "piles" else 4], dtype=F32)
