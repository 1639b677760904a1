"""The optimiser on the device (include/chub.h, "an optimiser on the device") restated in numpy: the Adam step operation by operation in
f64 / f32 (the sum of squares in the kernel's own order), the state blob, the plan's arithmetic, the row shuffle (its Philox is
policy_sample_lib's, which tests/test_policy_sample_cpu.py holds to the oracle's), the condition on the test data, and the bar of the
comparison with torch's double-precision AdamW, carried along the recurrence."""
import math
import struct

import numpy as np

import policy_sample_lib as ps

F32, F64 = np.float32, np.float64
U32 = 2.0 ** -24   # unit roundoff of f32
U64 = 2.0 ** -53   # .. of f64
LANES, PER_LANE, CHUNK, MAX_BLOCKS, N_SCALARS = 256, 4, 1024, 64, 12
BLOB_HEADER = 32

# the specs of the issue: (F on the hub it names or a row width, widths)
POLICY_HUB = [20, 25]   # S = 45 piles: D = 13 observation floats, A = 47 outputs
ACTOR_NETS = {"3-47": (3, [47]), "13-33-31-47": (13, [33, 31, 47]), "7-31-33-64-47": (7, [31, 33, 64, 47]), "64-256-224-47": (64, [256, 224, 47]),
              "13-64-64-47": (13, [64, 64, 47])}
CRITIC_NETS = {"13-1": (13, [1]), "13-64-64-1": (13, [64, 64, 1])}


def shapes_of(F, widths):
    return [(o, i) for o, i in zip(widths, [F] + list(widths[:-1]))]


def n_params(shapes, G=0):
    return sum(o * (i + 1) for o, i in shapes) + G


def plan(shapes, G=0):
    """chub_adam_plan's arithmetic"""
    n = n_params(shapes, G)
    chunks = (n + CHUNK - 1) // CHUNK
    blocks = min(chunks, MAX_BLOCKS)
    return dict(n=n, state_bytes=BLOB_HEADER + 8 * n, workspace_bytes=12 * n + 8 * chunks + 8 * N_SCALARS, norm_workgroups=blocks, step_workgroups=blocks)


def flatten(layers, log_std=None):
    """[(W, b), ..] (+ log_std) -> the flat f32 vector in the trainer's order"""
    parts = []
    for W, b in layers:
        parts += [np.asarray(W, dtype=F32).ravel(), np.asarray(b, dtype=F32).ravel()]
    if log_std is not None:
        parts.append(np.asarray(log_std, dtype=F32).ravel())
    return np.concatenate(parts)


def unflatten(flat, shapes, G=0):
    """-> ([(W, b), ..], log_std or None)"""
    out, p = [], 0
    for o, i in shapes:
        out.append((flat[p:p + o * i].reshape(o, i).copy(), flat[p + o * i:p + o * (i + 1)].copy()))
        p += o * (i + 1)
    return out, (flat[p:p + G].copy() if G else None)


def decay_mask(shapes, G=0):
    """True at the entries of a W"""
    parts = []
    for o, i in shapes:
        parts += [np.ones(o * i, dtype=bool), np.zeros(o, dtype=bool)]
    parts.append(np.zeros(G, dtype=bool))
    return np.concatenate(parts)


def sum_of_squares(g):
    """sum g^2 in the kernel's order: per chunk of 1024 lane j of 256 adds entries j, j + 256, j + 512, j + 768 from 0, the lanes meet in a
    tree (j += j + 128, + 64, .. + 1), the chunks are added in ascending order from 0"""
    g = np.asarray(g, dtype=F32).astype(F64)
    chunks = (len(g) + CHUNK - 1) // CHUNK
    sq = np.zeros(chunks * CHUNK, dtype=F64)
    with np.errstate(all="ignore"):
        sq[:len(g)] = g * g
        sq = sq.reshape(chunks, PER_LANE, LANES)
        red = np.zeros((chunks, LANES), dtype=F64)
        for j in range(PER_LANE):
            red = red + sq[:, j, :]
        stride = LANES // 2
        while stride:
            red = red[:, :stride] + red[:, stride:2 * stride]
            stride //= 2
        total = F64(0.0)
        for c in range(chunks):
            total = total + red[c, 0]
    return total


def clip_scale(norm, max_grad_norm):
    """the f32 scale of a finite norm"""
    if max_grad_norm == 0.0:
        return F32(1.0)
    r = F64(max_grad_norm) / (F64(norm) + F64(1e-6))
    return F32(r if r < 1.0 else 1.0)


def scale_is_stable(g, max_grad_norm):
    """the condition on the data: the f32 rounding of `scale` does not change under a relative perturbation of the norm by n 2^-53"""
    norm = np.sqrt(sum_of_squares(g))
    if not np.isfinite(norm):
        return True
    d = norm * len(g) * U64
    return clip_scale(norm - d, max_grad_norm) == clip_scale(norm, max_grad_norm) == clip_scale(norm + d, max_grad_norm)


def stabilised(g, max_grad_norm):
    """g, rescaled by factors near 1 until the condition holds (a case is not dropped)"""
    g = np.asarray(g, dtype=F32)
    k = 0
    while not scale_is_stable(g, max_grad_norm):
        k += 1
        assert k < 64
        g = (g * F32(1.0 + k / 64.0)).astype(F32)
    return g


class Adam(object):
    """the optimiser's state and one step on a flat f32 parameter vector; `wrong` names a deliberately wrong variant of the failure experiment"""

    def __init__(self, n, decays, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0, wrong=None):
        self.n, self.decays, self.wrong = int(n), np.asarray(decays, dtype=bool), wrong
        self.set_hyper(lr, betas, eps, weight_decay, max_grad_norm)
        self.reset()
        self.bar = None

    def set_hyper(self, lr, betas, eps, weight_decay, max_grad_norm):
        self.lr, self.beta1, self.beta2, self.eps, self.wd, self.max_norm = (F64(x) for x in (lr, betas[0], betas[1], eps, weight_decay, max_grad_norm))

    def reset(self):
        self.t, self.p1, self.p2 = 0, F64(1.0), F64(1.0)
        self.m, self.v = np.zeros(self.n, dtype=F32), np.zeros(self.n, dtype=F32)

    def blob(self):
        return struct.pack("<qddq", self.t, float(self.p1), float(self.p2), self.n) + self.m.tobytes() + self.v.tobytes()

    def load(self, blob):
        self.t, p1, p2, n = struct.unpack("<qddq", blob[:BLOB_HEADER])
        assert n == self.n and len(blob) == BLOB_HEADER + 8 * n
        self.p1, self.p2 = F64(p1), F64(p2)
        self.m = np.frombuffer(blob, dtype=F32, count=n, offset=BLOB_HEADER).copy()
        self.v = np.frombuffer(blob, dtype=F32, count=n, offset=BLOB_HEADER + 4 * n).copy()

    def step(self, theta, g):
        """-> (theta_new f32 [n], stats f64 [4]); the state moves on unless the step is skipped"""
        theta, g = np.asarray(theta, dtype=F32), np.asarray(g, dtype=F32)
        assert theta.shape == g.shape == (self.n,)
        with np.errstate(all="ignore"):
            norm = np.sqrt(sum_of_squares(g))
        if not np.isfinite(norm):
            return theta.copy(), np.array([self.t, norm, 0.0, 1.0], dtype=F64)
        scale = clip_scale(norm, self.max_norm)
        p1_old, p2_old = self.p1, self.p2
        self.t += 1
        self.p1, self.p2 = self.p1 * self.beta1, self.p2 * self.beta2
        p1, p2 = (p1_old, p2_old) if self.wrong == "correction_before_increment" else (self.p1, self.p2)
        omb1, omb2 = F64(1.0) - self.beta1, F64(1.0) - self.beta2
        with np.errstate(all="ignore"):
            gp = g.astype(F64) * F64(scale)
            m32 = (self.beta1 * self.m.astype(F64) + omb1 * gp).astype(F32)
            v32 = (self.beta2 * self.v.astype(F64) + omb2 * (gp * gp)).astype(F32)
            denom = np.sqrt(v32.astype(F64)) / np.sqrt(F64(1.0) - p2) + self.eps
            th = theta.astype(F64)
            if self.wd != 0.0:
                decays = np.ones(self.n, dtype=bool) if self.wrong == "decay_on_biases" else self.decays
                th = np.where(decays, th * (F64(1.0) - self.lr * self.wd), th)
            upd = (self.lr / (F64(1.0) - p1)) * (m32.astype(F64) / denom)
            new = (th - upd).astype(F32)
        if self.bar is not None:
            self._carry_bar(g, gp, scale, m32, v32, denom, upd, new)
        self.m, self.v = m32, v32
        return new, np.array([self.t, norm, F64(scale), 0.0], dtype=F64)

    # ---- the bar of the comparison with double-precision AdamW + clip_grad_norm_ on the same f32 gradients.  The device differs by the
    # rounding of theta, m, v to f32 after each step, the f32 scale, the running products against pow, and f64 roundings (a few U64)
    def track_bar(self):
        self.bar = dict(m=np.zeros(self.n), v=np.zeros(self.n), theta=np.zeros(self.n))

    def _carry_bar(self, g, gp, scale, m32, v32, denom, upd, new):
        b, t = self.bar, self.t
        b1, b2 = float(self.beta1), float(self.beta2)
        slack = 8 * U64
        # the clipped gradient: the f32 rounding of the scale, the norm's order (n U64 relative), the product
        eg = np.abs(gp) * (0.0 if self.max_norm == 0.0 else U32 * (1 + U32) + self.n * 2 * U64 + slack)
        m64, v64 = m32.astype(F64), v32.astype(F64)
        em = b1 * b["m"] + (1 - b1) * eg + U32 * np.abs(m64) + slack * (np.abs(m64) + b["m"])
        ev = b2 * b["v"] + (1 - b2) * (2 * np.abs(gp) * eg + eg * eg) + U32 * v64 + slack * (v64 + b["v"])
        root2 = math.sqrt(1.0 - float(self.p2))
        # |sqrt(v) - sqrt(v*)| <= sqrt(v) - sqrt(max(v - ev, 0)) for |v - v*| <= ev (concavity)
        ed = (np.sqrt(v64) - np.sqrt(np.maximum(v64 - ev, 0.0))) / root2
        d_lo = np.maximum(denom - ed, float(self.eps))
        step = float(self.lr) / (1.0 - float(self.p1))
        # running products against pow: |p - beta^t| <= t U64 p, relative to 1 - p
        rp = (t + 1) * U64 * (float(self.p1) / (1.0 - float(self.p1)) + float(self.p2) / (1.0 - float(self.p2)))
        u_big = step * (np.abs(m64) + em) / d_lo
        du = step * (em / d_lo + np.abs(m64) * ed / (denom * d_lo)) + u_big * (rp + slack)
        b["theta"] = b["theta"] + du + U32 * np.abs(new.astype(F64)) + slack * (np.abs(new.astype(F64)) + np.abs(upd) + b["theta"])
        b["m"], b["v"] = em, ev


def fsum_norm(g):
    g = np.asarray(g, dtype=F32).astype(F64)
    return math.sqrt(math.fsum((g * g).tolist()))


# ---- the row shuffle
SITE_SHUFFLE = 17
ROUNDS, WALK_CAP = 6, 64
SHUFFLE_R = (1, 2, 3, 5, 8, 9, 31, 32, 33, 300, 1023, 1024, 1025, 16455, 65537)
SHUFFLE_BIG = 6291456  # 1.5 * 2^22: six trips of the launch's 2^20 lanes, a quarter of E's domain outside 0 .. R - 1
SHUFFLE_KEYS = ((5, 0), (0x9E3779B97F4A7C15, 3), (77, (1 << 32) + 9), (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFE))  # (key, counter)


def bit_length(R):
    return int(R - 1).bit_length()


def encrypt(x, nb, key, c):
    """E on an array of values below 2^nb"""
    x = np.asarray(x, dtype=np.uint64)
    lo = nb >> 1
    hi = nb - lo
    mask_lo, mask_hi = np.uint64((1 << lo) - 1), np.uint64((1 << hi) - 1)
    k0, k1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    c2, c3 = int(c) & 0xFFFFFFFF, (int(c) >> 32) & 0xFFFFFFFF
    left, right = x >> np.uint64(lo), x & mask_lo
    for i in range(ROUNDS):
        if i & 1:
            right = right ^ (ps.philox(left, (SITE_SHUFFLE << 16) | i, c2, c3, k0, k1)[..., 0].astype(np.uint64) & mask_lo)
        else:
            left = left ^ (ps.philox(right, (SITE_SHUFFLE << 16) | i, c2, c3, k0, k1)[..., 0].astype(np.uint64) & mask_hi)
    return (left << np.uint64(lo)) | right


def shuffle_rows(key, c, R, walk=None, at=None):
    """-> int64 [R]; walk (a list): the largest number of applications of E any entry took is appended.  at: entries r to compute alone
    (an entry is a function of its own r: -> int64 [len(at)])"""
    R = int(R)
    nb = bit_length(R)
    if nb == 0:
        if walk is not None:
            walk.append(0)
        return np.zeros(1 if at is None else len(at), dtype=np.int64)
    c = int(c) & 0xFFFFFFFFFFFFFFFF
    y = encrypt(np.arange(R, dtype=np.uint64) if at is None else np.asarray(at, dtype=np.uint64), nb, key, c)
    steps = 1
    while steps < WALK_CAP:
        out = y >= np.uint64(R)
        if not out.any():
            break
        y[out] = encrypt(y[out], nb, key, c)
        steps += 1
    if walk is not None:
        walk.append(steps)
    y = y.astype(np.int64)
    y[y >= R] = -1
    return y
