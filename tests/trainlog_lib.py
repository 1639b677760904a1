"""The training log (include/chub.h, "a training log and a KL stop on the device") restated in numpy f64 from the table of its words:
begin, record and steps, one rounded operation each, plus the made sequences of stats blocks the CPU and the GPU tests share.  `wrong`
names a deliberately wrong variant of the failure experiment."""
import numpy as np

F64 = np.float64
WORDS = 30
COUNTED, AFTER_STOP, STOPPED, STOP_INDEX, ACTOR, KL_MAX, KL_LAST, CRITIC, ACTOR_OPT, CRITIC_OPT = 0, 1, 2, 3, 4, 10, 11, 12, 18, 24
K1, K3 = 0, 1
WRONG = ("stop_not_counted", "stop_not_sticky", "gt_limit")


class Log(object):
    def __init__(self, wrong=None):
        assert wrong is None or wrong in WRONG
        self.wrong = wrong
        self.begin()

    def begin(self):
        self.w = np.zeros(WORDS, dtype=F64)
        self.w[STOP_INDEX] = -1.0
        self.gate = 0
        self.calls = 0  # record calls since begin

    def kl(self, ps, kind):
        if ps is None:
            return F64(0.0)
        ps = np.asarray(ps, dtype=F64)
        n = ps[0]
        if n == 0.0:
            return F64(0.0)
        with np.errstate(all="ignore"):
            k1 = ps[3] / n
            if kind == K1:
                return k1
            return (ps[5] / n - F64(1.0)) + k1

    def record(self, ps, cs, kind=K3, kl_limit=0.0):
        w = self.w
        index, self.calls = self.calls, self.calls + 1
        if w[STOPPED] != 0.0 and self.wrong != "stop_not_sticky":
            w[AFTER_STOP] += 1.0
            return
        kl = self.kl(ps, kind)
        with np.errstate(all="ignore"):
            stops = kl_limit > 0.0 and ((kl > kl_limit) if self.wrong == "gt_limit" else not (kl <= kl_limit))
        if stops:
            w[STOPPED], w[STOP_INDEX], self.gate = 1.0, F64(index), 1
            if self.wrong == "stop_not_counted":
                return
        elif self.wrong == "stop_not_sticky":
            w[STOPPED], self.gate = 0.0, 0
        with np.errstate(all="ignore"):
            if ps is not None:
                w[ACTOR:ACTOR + 6] = w[ACTOR:ACTOR + 6] + np.asarray(ps, dtype=F64)
            if cs is not None:
                w[CRITIC:CRITIC + 6] = w[CRITIC:CRITIC + 6] + np.asarray(cs, dtype=F64)
            if w[COUNTED] == 0.0 or kl > w[KL_MAX]:
                w[KL_MAX] = kl
        w[KL_LAST] = kl
        w[COUNTED] += 1.0

    def steps(self, sa, sc):
        for base, st in ((ACTOR_OPT, sa), (CRITIC_OPT, sc)):
            if st is None:
                continue
            t, norm, scale, how = (F64(x) for x in st)
            w = self.w
            if how == 0.0:
                w[base] += 1.0
                if scale < 1.0:
                    w[base + 5] += 1.0
            elif how == 1.0:
                w[base + 1] += 1.0
            else:
                w[base + 2] += 1.0
            if np.isfinite(norm):
                w[base + 3] = w[base + 3] + norm
                if norm > w[base + 4]:
                    w[base + 4] = norm


def bits(a):
    return np.ascontiguousarray(a, dtype=F64).view(np.uint64)


def actor_stats(rs, n, k1, k3_extra=0.0):
    """a stats block of n rows whose K1 estimate is about k1 and whose K3 estimate is about k3_extra + ... : the sums are made, not
    derived from rows, so the two estimators can be put on either side of a limit independently"""
    n = F64(n)
    sum_dlogp = F64(k1) * n
    sum_ratio = n * (F64(1.0) + F64(k3_extra) - F64(k1))  # K3 = (sum_ratio / n - 1) + k1 ~ k3_extra
    return np.array([n, rs.normal() * n, rs.uniform(1, 3) * n, sum_dlogp, np.floor(rs.uniform(0, 0.3) * n), sum_ratio], dtype=F64)


def critic_stats(rs, n):
    n = F64(n)
    ret = rs.normal(size=int(n)) if n else np.zeros(0)
    return np.array([n, rs.uniform(0, 2) * n, np.floor(rs.uniform(0, 0.2) * n), rs.uniform(0, 1) * n, ret.sum(), (ret * ret).sum()], dtype=F64)


def step_stats(rs, t, how, norm=None, scale=None):
    norm = rs.uniform(0.1, 3.0) if norm is None else norm
    scale = (1.0 if rs.uniform() < 0.5 else np.float32(0.5 / norm)) if scale is None else scale
    return np.array([t, norm, scale if how == 0 else 0.0, how], dtype=F64)


def sequences():
    """name -> dict(kind, kl_limit, blocks [(pstats or None, cstats or None, astats_actor or None, astats_critic or None)], and what the
    log must say: stopped_at, counted, after_stop)"""
    rs = np.random.RandomState(20)
    out = {}

    def mb(n, k1, k3=0.0, t=1, how=0, **kw):
        return (actor_stats(rs, n, k1, k3), critic_stats(rs, n), step_stats(rs, t, how, **kw), step_stats(rs, t, how))

    # KL below, below, above, below the limit: the stop is at index 2, the 4th goes to AFTER_STOP, the sums hold the first three only
    out["below-below-above-below"] = dict(kind=K1, kl_limit=0.03, stopped_at=2, counted=3, after_stop=1,
                                          blocks=[mb(100, 0.01, t=1), mb(100, 0.02, t=2), mb(100, 0.05, t=2, how=2), mb(84, 0.001, t=2, how=2)])
    # a limit of 0 never stops, whatever the KL
    out["limit-0"] = dict(kind=K3, kl_limit=0.0, stopped_at=None, counted=4, after_stop=0,
                          blocks=[mb(128, 0.5, 0.4, t=1), mb(128, 5.0, 7.0, t=2), mb(128, -1.0, 0.0, t=3, how=1, norm=np.inf), mb(1, 0.3, 0.3, t=3)])
    # a NaN in stats[3] stops
    nan = mb(64, 0.001, 0.001, t=2, how=2)
    nan[0][3] = np.nan
    out["nan"] = dict(kind=K3, kl_limit=0.02, stopped_at=1, counted=2, after_stop=1, blocks=[mb(64, 0.001, 0.001, t=1), nan, mb(64, 0.0, 0.0, t=1, how=2)])
    # rows == 0: the estimate is 0, the minibatch is counted
    out["rows-0"] = dict(kind=K1, kl_limit=0.02, stopped_at=None, counted=3, after_stop=0,
                         blocks=[mb(0, 0.0, t=1), mb(32, 0.01, t=2), mb(0, 0.0, t=3)])
    # blocks where only one of the estimators passes the limit: K1 small and K3 large, then the other way round
    pair = [mb(100, 0.001, 0.001, t=1), mb(100, 0.01, 0.04, t=2), mb(100, 0.04, 0.01, t=3), mb(100, 0.001, 0.001, t=4)]
    out["k1-of-the-pair"] = dict(kind=K1, kl_limit=0.03, stopped_at=2, counted=3, after_stop=1, blocks=pair)
    out["k3-of-the-pair"] = dict(kind=K3, kl_limit=0.03, stopped_at=1, counted=2, after_stop=2, blocks=pair)
    # missing blocks: no actor stats (the estimate is 0), no critic stats, one optimiser only
    a, b = mb(50, 9.0, 9.0, t=1), mb(50, 0.01, 0.01, t=2)
    out["null-blocks"] = dict(kind=K3, kl_limit=0.02, stopped_at=None, counted=3, after_stop=0,
                              blocks=[(None, a[1], a[2], None), (b[0], None, None, b[3]), (None, None, None, None)])
    # a KL exactly at the limit does not stop (kl <= limit); the next one above it does.  Powers of two: the estimate is exact
    out["at-the-limit"] = dict(kind=K1, kl_limit=0.25, stopped_at=1, counted=2, after_stop=0,
                               blocks=[(np.array([64.0, 1.0, 2.0, 16.0, 0.0, 64.0]), None, None, None),
                                       (np.array([64.0, 1.0, 2.0, 16.0 + 2.0 ** -48, 0.0, 64.0]), None, None, None)])
    return out


def restate(seq, wrong=None):
    log = Log(wrong)
    for ps, cs, sa, sc in seq["blocks"]:
        log.record(ps, cs, seq["kind"], seq["kl_limit"])
        log.steps(sa, sc)
    return log


def split(n_rows, minibatch_rows):
    """chub_ppo_update's split: (minibatches per epoch, rows of the last)"""
    m = -(-n_rows // minibatch_rows)
    return m, n_rows - (m - 1) * minibatch_rows


def gated_step(adam, theta, g, gate, wrong=None):
    """adam_lib.Adam.step behind the gate: a closed gate (gate != 0) keeps theta and the state and says stats = [t, norm, 0, 2].
    wrong="gate_workgroup_0": only workgroup 0 of the step launch consults the word -- it returns (no scalars, no stats[3] = 0, its chunks
    0, blocks, 2 blocks, .. untouched) while the other workgroups step their chunks from the scalars' copy"""
    import adam_lib as al
    if not gate:
        return adam.step(theta, g)
    with np.errstate(all="ignore"):
        norm = np.sqrt(al.sum_of_squares(g))
    held = np.array([adam.t, norm, 0.0, 2.0], dtype=F64)
    if wrong != "gate_workgroup_0":
        return np.asarray(theta, dtype=np.float32).copy(), held
    t, p1, p2, m, v = adam.t, adam.p1, adam.p2, adam.m.copy(), adam.v.copy()
    new, _ = adam.step(theta, g)
    chunks = (adam.n + al.CHUNK - 1) // al.CHUNK
    blocks = min(chunks, al.MAX_BLOCKS)
    of_wg0 = (np.arange(adam.n) // al.CHUNK) % blocks == 0
    new[of_wg0], adam.m[of_wg0], adam.v[of_wg0] = np.asarray(theta, dtype=np.float32)[of_wg0], m[of_wg0], v[of_wg0]
    adam.t, adam.p1, adam.p2 = t, p1, p2
    return new, held
