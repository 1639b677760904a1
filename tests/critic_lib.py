"""The numpy f64 restatement of include/chub.h's "a critic on the device", and nothing else defines the expected values of
tests/test_critic_cpu.py and tests/test_gpu_critic.py.  It is evaluated AT the f32 inputs: the normalisation, and under the clipped loss
d, v_c, e1, e2 and the activity predicate, are formed in f32 as the header says (from the f64 value rounded once), everything else in f64.

The bar is derived, not chosen (DESIGN.md 6.23 "The bar", 6.24).  policy_lib's forward bound gives err_h per hidden image and err_v;
c = v - ret carries err_v plus one rounding; steps (4) and (5) of 6.23 carry it back through the layers (delta_in = (W^T delta) act'(h): a
chain of `out` products, the incoming error through |W|, tanh's factor off by 2 |h| err_h + err_h^2, relu's mask undecided where
|z| <= err_z) and into a parameter (the operands' errors, one rounding per product, 32 rows per MFMA chain and tpw = ceil(tiles /
workgroups) tiles per workgroup in f32, one rounding after the f64 merge).  All of it over R."""
import ctypes as C
import functools

import numpy as np

import grid_pass_lib as gpl
import policy_lib as pl

F32 = np.float32
U, TINY = pl.U, pl.TINY
U64 = 2.0 ** -53


class Case(object):
    """everything one call reads.  layers [(W, b)] f32 (the last has one output), norm None or (mean, inv_std, clip), act "tanh" / "relu";
    per-row arrays over n_rows rows: x [., F] f32 (ld: the row stride the device copy is given, >= F), ret, v_old f32; rows int64 [R] or
    None (indices outside 0 .. n_rows - 1 are skipped); loss "mse" / "clipped"; clip_eps"""

    def __init__(self, **kw):
        self.norm = self.rows = self.v_old = None
        self.loss, self.clip_eps, self.name, self.ld = "mse", 0.2, "", None
        self.__dict__.update(kw)

    def copy(self, **kw):
        c = Case(**self.__dict__)
        c.__dict__.update(kw)
        return c

    @property
    def R(self):
        return len(self.x) if self.rows is None else len(self.rows)

    @property
    def F(self):
        return self.x.shape[1]

    @property
    def sizes(self):
        return [self.F] + [W.shape[0] for W, _ in self.layers]


def clipped_parts(v32, v_old, ret, eps):
    """the header's f32 chain -> d, v_c, e1, e2 (f32) and the predicate, every operation rounded once"""
    v32, v_old, ret, eps = (np.asarray(a, dtype=F32) for a in (v32, v_old, ret, F32(eps)))
    d = (v32 - v_old).astype(F32)
    vc = (v_old + np.minimum(np.maximum(d, -eps), eps)).astype(F32)
    t1, t2 = (v32 - ret).astype(F32), (vc - ret).astype(F32)
    e1, e2 = (t1 * t1).astype(F32), (t2 * t2).astype(F32)
    active = ((d > -eps) & (d < eps)) | (e1 >= e2)
    return d, vc, e1, e2, active


MISTAKES_MSE = ("row_dropped", "ret_shifted", "no_1_over_R")
MISTAKES = MISTAKES_MSE + ("clip_ignored", "v_old_ignored")  # (the last two change nothing under MSE: they are asked of the clipped cases)
TRIP_MISTAKES = ("later_trips_dropped", "last_trip_only")  # whole tiles lost in a workgroup's walk: asked of the cases of more than one trip


def mistakes_of(c):
    return MISTAKES if c.loss == "clipped" else MISTAKES_MSE


def restate(c, tpw=1, mistake=None, blocks=None):
    """-> dict: gW, gb (lists, f64), values [R] f64 (0 at skipped positions), stats [6], coef, active, d, e1, e2 (over the valid rows) and
    the bars bar_W, bar_b, bar_v [R], bar_stats, err_e (the derived error of e1 - e2 per valid row).  tpw: tiles of 32 rows a workgroup
    walks at most.  mistake: one of MISTAKES or TRIP_MISTAKES (a deliberately wrong restatement; the bars are the right one's); blocks: the
    call's workgroups, which the TRIP_MISTAKES need"""
    n_rows = len(c.x)
    idx_all = np.arange(n_rows) if c.rows is None else np.asarray(c.rows, dtype=np.int64)
    R = len(idx_all)
    ok = (idx_all >= 0) & (idx_all < n_rows)
    idx = idx_all[ok]
    x = c.x[idx]
    if c.norm is not None:
        x = pl.normalise(x, *c.norm)
    ret32 = np.asarray(c.ret, dtype=F32)
    if mistake == "ret_shifted":
        ret32 = np.roll(ret32, -1)
    ret = ret32[idx].astype(np.float64)

    # ---- forward, with policy_lib.forward's bound per image
    hs, errs, zs, ezs = [np.asarray(x, dtype=np.float64)], [np.zeros(x.shape)], [], []
    L = len(c.layers)
    for l, (W, b) in enumerate(c.layers):
        W, b = np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64)
        K = W.shape[1]
        h, err = hs[-1], errs[-1]
        z = h @ W.T + b
        ez = pl.gamma(K + 2) * (np.abs(b) + (np.abs(h) + err) @ np.abs(W).T) + err @ np.abs(W).T + K * TINY
        zs.append(z)
        ezs.append(ez)
        if l < L - 1:
            if c.act == "tanh":
                hs.append(np.tanh(z))
                errs.append(ez + pl.TANH_ERR)
            else:
                hs.append(np.maximum(z, 0.0))
                errs.append(ez)
    v, ev = zs[-1][:, 0], ezs[-1][:, 0]

    # ---- c = R dL/dv, the loss terms
    coef = v - ret
    ed = ev + 2 * U * (np.abs(coef) + ev) + TINY  # the device's f32 difference against the f64 one
    n = len(idx)
    if c.loss == "mse":
        active = np.ones(n, dtype=bool)
        term = 0.5 * coef * coef
        bar_term = np.abs(coef) * ed + 0.5 * ed * ed
        d = e1 = e2 = np.zeros(n)
        err_e = np.zeros(n)
    else:
        v_old = np.zeros(n_rows, dtype=F32) if mistake == "v_old_ignored" else np.asarray(c.v_old, dtype=F32)
        d, vc, e1, e2, active = clipped_parts(v.astype(F32), v_old[idx], ret32[idx], c.clip_eps)
        if mistake == "clip_ignored":
            active = np.ones(n, dtype=bool)
        d, e1, e2 = d.astype(np.float64), e1.astype(np.float64), e2.astype(np.float64)
        # outside the range v_c = v_old +- eps does not depend on v: e2 is the device's bits; e1 carries the forward error
        err_e = 2 * np.abs(coef) * ed + ed * ed + 2 * U * e1 + TINY
        term = 0.5 * np.maximum(e1, e2)
        # inside the range v_c = v_old + fl(v - v_old) moves with v: two more roundings on the way, then e2 as e1
        evc = ev * (1 + 4 * U) + 2 * U * (2 * np.abs(d) + np.abs(v_old[idx].astype(np.float64))) + TINY
        t2 = np.abs(vc.astype(np.float64) - ret)
        err_e2 = np.where(np.abs(d) < float(F32(c.clip_eps)), 2 * t2 * evc + evc * evc + 2 * U * e2 + TINY, 0.0)
        bar_term = 0.5 * np.maximum(err_e, err_e2) + U * np.maximum(e1, e2)  # (|max(a, b) - max(a', b')| <= max(|a - a'|, |b - b'|))
    delta_v = np.where(active, coef, 0.0)
    err_dv = np.where(active, ed, 0.0)
    dr = ret - v
    stats = np.array([float(n), term.sum(), float((~active).sum()), (dr * dr).sum(), ret.sum(), (ret * ret).sum()])
    acc64 = (n + 600) * U64  # f64 sums in the device's order against numpy's
    bar_stats = np.array([0.0, bar_term.sum() + acc64 * np.abs(term).sum(), 0.0, (2 * np.abs(dr) * ev + ev * ev).sum() + acc64 * (dr * dr).sum(),
                          acc64 * np.abs(ret).sum(), acc64 * (ret * ret).sum()]) * 1.001 + TINY
    values, bar_v = np.zeros(R), np.zeros(R)
    values[ok], bar_v[ok] = v, ev * 1.001 + TINY

    # ---- backward
    delta = delta_v[:, None].copy()
    err_delta = err_dv[:, None] * 1.001 + TINY
    if mistake == "row_dropped":  # (the first row from the middle on that has a gradient to lose)
        live = np.flatnonzero(np.roll(delta[:, 0] != 0.0, -(n // 2)))
        delta[(live[0] + n // 2) % n if len(live) else 0] = 0.0
    if mistake in TRIP_MISTAKES:  # (a workgroup walks the tiles b, b + blocks, ..: only its first tile counts / only its last one)
        at = np.arange(R)[ok]
        kept = at // 32 < blocks if mistake == "later_trips_dropped" else gpl.grad_last_trip(R, blocks)[at]
        delta[~kept] = 0.0
    div = 1.0 if mistake == "no_1_over_R" else float(R)  # (the sum divided by R, as the merge does)
    gam = pl.gamma(32 * int(tpw) + 3)
    gW, gb, bar_W, bar_b = [None] * L, [None] * L, [None] * L, [None] * L
    dl, edl = delta, err_delta
    for l in range(L - 1, -1, -1):
        W = np.asarray(c.layers[l][0], dtype=np.float64)
        h, eh = hs[l], errs[l]
        gW[l] = dl.T @ h / div
        gb[l] = dl.sum(axis=0) / div
        ad = np.abs(dl)
        bar_W[l] = ((edl.T @ (np.abs(h) + eh) + ad.T @ eh) + gam * ((ad + edl).T @ (np.abs(h) + eh))) / R * 1.001 + TINY
        bar_b[l] = (edl.sum(axis=0) + pl.gamma(32 * int(tpw) + 34) * (ad + edl).sum(axis=0)) / R * 1.001 + TINY
        if l > 0:
            pre = dl @ W
            e_pre = edl @ np.abs(W) + pl.gamma(W.shape[0] + 2) * ((ad + edl) @ np.abs(W)) + W.shape[0] * TINY
            if c.act == "tanh":
                fac = 1.0 - h * h
                e_fac = 2 * np.abs(h) * eh + eh * eh + 2.002 * U
                nd = pre * fac
                edl = e_pre * (np.abs(fac) + e_fac) + np.abs(pre) * e_fac + U * np.abs(nd)
            else:
                zl, ezl = zs[l - 1], ezs[l - 1]
                nd = np.where(zl > 0, pre, 0.0)
                edl = np.where(np.abs(zl) <= ezl, np.abs(pre) + e_pre, np.where(zl > 0, e_pre, 0.0))
            dl = nd
    return dict(gW=gW, gb=gb, values=values, stats=stats, coef=coef, active=active, d=d, e1=e1, e2=e2, err_e=err_e, ev=ev, bar_W=bar_W, bar_b=bar_b,
                bar_v=bar_v, bar_stats=bar_stats, delta=delta, hs=hs, ok=ok, v=v)


def outside_bar(right, wrong):
    """whether a wrong restatement leaves the right one's bar somewhere in gW or gb"""
    out = any((np.abs(a - b) > bar).any() for a, b, bar in zip(right["gW"], wrong["gW"], right["bar_W"]))
    return bool(out | any((np.abs(a - b) > bar).any() for a, b, bar in zip(right["gb"], wrong["gb"], right["bar_b"])))


def undecided(c, r):
    """(near, tied): rows whose |d| lies within 1e-3 of eps; inactive-candidate rows (|d| >= eps) whose |e1 - e2| lies inside its own
    derived error -- there no conforming device can be held to the predicate"""
    if c.loss != "clipped":
        z = np.zeros(len(r["coef"]), dtype=bool)
        return z, z
    eps = float(F32(c.clip_eps))
    near = np.abs(np.abs(r["d"]) - eps) <= 1e-3
    tied = (np.abs(r["d"]) >= eps) & (np.abs(r["e1"] - r["e2"]) <= r["err_e"])
    return near, tied


def check_conditions(c, r):
    """the conditions on a case's DATA under which the GPU comparison means something: the bar below 2^-8 of every layer's largest
    gradient; under the clipped loss no |d| within 1e-3 of eps and no candidate row whose e1 - e2 lies inside its own derived error"""
    for l in range(len(c.layers)):
        assert r["bar_W"][l].max() < 2.0 ** -8 * np.abs(r["gW"][l]).max(), ("bar of gW", c.name, l, r["bar_W"][l].max(), np.abs(r["gW"][l]).max())
        assert r["bar_b"][l].max() < 2.0 ** -8 * np.abs(r["gb"][l]).max(), ("bar of gb", c.name, l, r["bar_b"][l].max(), np.abs(r["gb"][l]).max())
    near, tied = undecided(c, r)
    assert not near.any() and not tied.any(), ("a row on the predicate's edge", c.name, int(near.sum()), int(tied.sum()))
    assert r["ev"].max() < 1e-3, ("the forward bound reaches the margin around eps", c.name, r["ev"].max())


def separate(c, tpw=1):
    """move what the definition leaves open out of the way, as policy_grad_lib.separate_ratios moves a logp: a row with |d| within 2e-3 of
    eps gets its v_old moved by 8e-3, a candidate row with |e1 - e2| within 4 times its derived error gets its ret moved by 0.05"""
    if c.loss != "clipped":
        return c
    for _ in range(4):
        r = restate(c, tpw)
        idx = (np.arange(len(c.x)) if c.rows is None else np.asarray(c.rows))[r["ok"]]
        eps = float(F32(c.clip_eps))
        near = np.abs(np.abs(r["d"]) - eps) <= 2e-3
        tied = (np.abs(r["d"]) >= eps) & (np.abs(r["e1"] - r["e2"]) <= 4 * r["err_e"])
        if not near.any() and not tied.any():
            break
        v_old, ret = c.v_old.copy(), c.ret.copy()
        v_old[idx[near]] += F32(8e-3)
        ret[idx[tied & ~near]] += F32(0.05)
        c = c.copy(v_old=v_old, ret=ret)
    return c


# ---- the plan, through the C ABI (host-only: it needs no device)
def plan(F, widths, R, act="tanh", normalize=False, clip=0.0):
    """chub_critic_plan -> (rc, dict of the out struct, message)"""
    import charginghub_env_amd as chub
    from charginghub_env_amd import _lib

    lib = chub.load_library()
    spec = _lib.critic_spec(F, widths, act, normalize, clip)
    out = _lib.ChubCriticPlanOut()
    rc = lib.chub_critic_plan(C.byref(spec), int(R), C.byref(out))
    return rc, {name: int(getattr(out, name)) for name, _ in out._fields_}, lib.chub_last_error().decode()


def tiles_per_workgroup(c):
    rc, p, msg = plan(c.F, c.sizes[1:], c.R, c.act)
    assert rc == 0, msg
    tiles = (c.R + 31) // 32
    return (tiles + p["workgroups"] - 1) // p["workgroups"]


# ---- cases.  Made HERE so that the CPU test holds the conditions on the GPU test's own data
def general_layers(rs, sizes):
    """weights at scale 1 / fan-in (a row's sum of |w| stays near 0.8, the forward bound does not grow with depth)"""
    return [((rs.normal(size=(o, i)) / i).astype(F32), (rs.normal(size=o) * 0.1).astype(F32)) for i, o in zip(sizes[:-1], sizes[1:])]


def forward64(c, x=None):
    x = c.x if x is None else x
    h = np.asarray(x if c.norm is None else pl.normalise(x, *c.norm), dtype=np.float64)
    for l, (W, b) in enumerate(c.layers):
        h = h @ np.asarray(W, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
        if l < len(c.layers) - 1:
            h = np.tanh(h) if c.act == "tanh" else np.maximum(h, 0.0)
    return h[:, 0]


def synthetic_case(F, hidden, act="tanh", n_rows=300, loss="mse", norm=False, rows=None, ld=None, seed=0, clip_eps=0.2):
    """rows drawn in numpy; ret and v_old around the net's own value, so that under the clipped loss rows fall on both sides of the
    predicate (|d| < eps for about half of them, e1 >= e2 for about half of the others)"""
    rs = np.random.RandomState(12000 + 131 * F + 17 * len(hidden) + sum(hidden) + 3 * n_rows + seed)
    layers = general_layers(rs, [F] + list(hidden) + [1])
    x = (rs.normal(size=(n_rows, F)) + 0.3).astype(F32)
    nrm = ((rs.normal(size=F) * 0.2).astype(F32), ((1.0 + rs.rand(F)) * 0.5).astype(F32), 3.0) if norm else None
    c = Case(layers=layers, norm=nrm, act=act, x=x, ret=np.zeros(n_rows, dtype=F32), v_old=np.zeros(n_rows, dtype=F32), loss=loss, clip_eps=clip_eps,
             ld=ld)
    v = forward64(c)
    ret = (v + 0.5 * rs.normal(size=n_rows) + 0.1).astype(F32)
    v_old = (v + 0.25 * rs.normal(size=n_rows)).astype(F32)
    if rows == "mixed":  # repeats, indices outside the arrays on both sides, an order that is not ascending
        rows = rs.randint(0, n_rows, size=n_rows + 17).astype(np.int64)
        rows[[3, 40, 41, n_rows]] = [-1, n_rows, 2 ** 40, -(2 ** 33)]
        rows[5] = rows[6]
    c = c.copy(ret=ret, v_old=v_old, rows=rows,
               name="%d-%s-%s-%s-%d%s%s%s" % (F, "x".join(map(str, hidden)) or "linear", act, loss, n_rows, "-norm" if norm else "",
                                               "-rows" if rows is not None else "", "-ld%d" % ld if ld else ""))
    return separate(c, tiles_per_workgroup(c))


GENERAL_SHAPES = (
    # F, hidden, act, norm, rows, ld
    (13, (33,), "tanh", False, None, None),
    (13, (64, 64), "tanh", False, None, None),
    (13, (33, 31), "relu", False, None, None),
    (7, (31, 33, 64), "tanh", False, None, None),
    (13, (256, 33), "tanh", False, None, None),
    (64, (256, 224), "tanh", False, None, None),   # 64 + 256 + 224 + 512 + 16 = 1072 LDS rows, 141 KB: beyond 64 KiB, dW tiles in the partials
    (13, (64, 64), "tanh", True, None, None),
    (13, (33,), "relu", False, "mixed", None),
    (45, (33, 17), "tanh", True, "mixed", 47),     # F no multiple of 2 or 32, ld > F (a packed block's D + 2)
    (13, (), "tanh", False, None, 15),             # one layer: the head alone
)
GENERAL_ROWS = 300  # ten tiles of 32, the last one partial: sixteen workgroups, six of them walk no tile


def gpu_general_cases():
    out = []
    for k, (F, hidden, act, norm, rows, ld) in enumerate(GENERAL_SHAPES):
        for loss in ("mse", "clipped"):
            out.append(synthetic_case(F, hidden, act, GENERAL_ROWS, loss, norm, rows, ld, seed=k))
    return out


# ---- the cases of more than one trip of k_critic's walk (tests/test_gpu_grad_trips.py): tests/grid_pass_lib.py's R2 and R3
TRIP_R = (gpl.GRAD_R2, gpl.GRAD_R3)
TRIP_SHAPES = (
    (13, (64, 64), "tanh", False, None, None),
    (13, (33, 31), "relu", False, None, None),
    (13, (), "tanh", False, None, 15),
    (45, (33, 17), "tanh", True, "mixed", 47),
)
TRIP_WIDE = (64, (256, 224), "tanh", False, None, None)  # dW tiles in the partials; its f64 restatement is the slowest: R2 and MSE only


def later_trips_mixed(c):
    """a "mixed" case's row list with more of the same in the later trips: indices outside the arrays and a repeat in the first tiles of
    the second (and third) trip and in the partial last tile.  Rows leave or count twice; none is new, so no row comes onto an edge"""
    rows, n_rows = c.rows.copy(), len(c.x)
    for t in range(1, (gpl.grad_tiles(c.R) - 1) // gpl.GRAD_MAX_BLOCKS + 1):
        at = t * gpl.GRAD_MAX_BLOCKS * 32
        rows[[at + 5, at + 32 + 31]] = [-7, n_rows + 1]
        rows[at + 9] = rows[at + 8]
    rows[c.R - 2] = 2 ** 35
    return c.copy(rows=rows)


@functools.lru_cache(maxsize=None)
def trip_general_cases():
    """-> [(case, tpw)]: TRIP_SHAPES under both losses at R2 and R3, TRIP_WIDE under MSE at R2; tpw: 2 and 3, from the plan"""
    out = []
    for R in TRIP_R:
        for k, (F, hidden, act, norm, rows, ld) in enumerate(TRIP_SHAPES):
            for loss in ("mse", "clipped"):
                c = synthetic_case(F, hidden, act, R - 17 if rows == "mixed" else R, loss, norm, rows, ld, seed=60 + k)
                out.append(later_trips_mixed(c) if rows == "mixed" else c)
    F, hidden, act, norm, rows, ld = TRIP_WIDE
    out.append(synthetic_case(F, hidden, act, gpl.GRAD_R2, "mse", norm, rows, ld, seed=70))
    assert all(c.R in TRIP_R for c in out)
    return [(c, tiles_per_workgroup(c)) for c in out]


def trip_parts(c, blocks):
    """the call over R rows cut by trip: -> [case], part t holding, through d_rows, the positions the workgroups meet in their trip t"""
    base = np.arange(c.R, dtype=np.int64) if c.rows is None else np.asarray(c.rows, dtype=np.int64)
    trips = -(-gpl.grad_tiles(c.R) // blocks)
    return [c.copy(rows=base[gpl.grad_trip_positions(c.R, blocks, t)], name="%s-trip%d" % (c.name, t)) for t in range(trips)]


# ---- the exact cases: every product and every partial sum exact in f32, so values, gradients and stats equal the restatement BIT FOR BIT
EXACT_F, EXACT_HIDDEN = 13, (33, 64, 31)
EXACT_WIDE = (256, 64)  # 8 + 16 + 2 = 26 dW tiles of 32 x 32: more than the 16 a workgroup keeps in registers
EXACT_R = (1, 31, 32, 33, 95, 300)
EXACT_EPS = 0.75


def exact_case(n_layers, n_rows, loss="mse", hidden=EXACT_HIDDEN, F=EXACT_F, blocks=None):
    """relu, features multiples of 1/2, weights in {-1, 0, 1} (three per output), integer biases; ret = v + k / 2 and v_old = v + j / 2 with
    small integers k, j, eps = 3/4: d, v_c, e1 and e2 are multiples of 1/16, |v_c - ret| is an odd and |v - ret| an even multiple of 1/4
    outside the range (never e1 == e2), |d| is never eps"""
    hidden = tuple(hidden[:n_layers - 1])
    rs = np.random.RandomState(87000 + n_layers + 7 * sum(hidden))  # (the net does not depend on R or the loss: one critic serves them all)
    sizes = [F] + list(hidden) + [1]
    layers = []
    for fan_in, out in zip(sizes[:-1], sizes[1:]):
        W = np.zeros((out, fan_in), dtype=F32)
        for n in range(out):
            cols = rs.choice(fan_in, size=min(3, fan_in), replace=False)
            W[n, cols] = rs.choice([-1, 1], size=len(cols))
        layers.append((W, rs.randint(-1, 2, size=out).astype(F32)))
    rs = np.random.RandomState(88000 + 100 * n_layers + n_rows + 7 * sum(hidden))
    x = (rs.randint(-4, 5, size=(n_rows, F)) / 2.0).astype(F32)
    c = Case(layers=layers, act="relu", x=x, ret=np.zeros(n_rows, dtype=F32), v_old=np.zeros(n_rows, dtype=F32), loss=loss, clip_eps=EXACT_EPS,
             name="exact-%d-%d-%s" % (n_layers, n_rows, loss))
    v = forward64(c)
    c = c.copy(ret=(v + rs.randint(-3, 5, size=n_rows) / 2.0).astype(F32), v_old=(v + rs.randint(-3, 4, size=n_rows) / 2.0).astype(F32))
    assert_exact(c, blocks)
    return c


def exact_sums(dl, h, blocks, q):
    """the sums of a dW tile and of a bias: without `blocks` over all rows below 2^23 quanta; with it over each workgroup's own rows
    (tiles b, b + blocks, ..: the only f32 chain there is) below 2^23 and over all rows below 2^53, which the f64 merge holds exactly"""
    ad, ah = np.abs(dl), np.abs(h)
    total = max((ad.T @ ah).max(), ad.sum(axis=0).max()) / q
    if blocks is None:
        return total < 2.0 ** 23
    A, H = gpl.grad_by_workgroup(ad, blocks), gpl.grad_by_workgroup(ah, blocks)
    own = max(np.matmul(A.transpose(0, 2, 1), H).max(), A.sum(axis=1).max()) / q
    return own < 2.0 ** 23 and total < 2.0 ** 53


def assert_exact(c, blocks=None):
    """every value and every product is a multiple of 2^-4 and every sum of absolute values stays below 2^23 quanta: any partial sum in
    any order is exact in f32.  blocks: the call's workgroups -- then the sums over rows are held per workgroup (exact_sums)"""
    q = 2.0 ** -4
    r = restate(c)
    assert blocks is None or c.rows is None
    h = np.asarray(c.x, dtype=np.float64)
    for l, (W, b) in enumerate(c.layers):
        W, b = np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64)
        assert ((np.abs(h) @ np.abs(W).T + np.abs(b)).max()) / q < 2.0 ** 23
        h = h @ W.T + b
        if l < len(c.layers) - 1:
            h = np.maximum(h, 0.0)
        assert np.array_equal(h / q, np.round(h / q))
    for a in (c.ret, c.v_old, r["e1"], r["e2"]):
        a = np.asarray(a, dtype=np.float64)
        assert np.array_equal(a / q, np.round(a / q)) and np.abs(a).max(initial=0.0) / q < 2.0 ** 23
    if c.loss == "clipped":
        assert (np.abs(np.abs(r["d"]) - EXACT_EPS) >= 0.25).all() and (r["e1"] != r["e2"])[np.abs(r["d"]) > EXACT_EPS].all()
    dl = r["delta"]
    for l in range(len(c.layers) - 1, -1, -1):
        W = np.asarray(c.layers[l][0], dtype=np.float64)
        assert np.array_equal(dl / q, np.round(dl / q))
        assert exact_sums(dl, r["hs"][l], blocks, q)
        if l > 0:
            assert (np.abs(dl) @ np.abs(W)).max() / q < 2.0 ** 23
            dl = np.where(r["hs"][l] > 0, dl @ W, 0.0)
    return r


def exact_expected(c, r=None):
    """the bits the device must give: the exact sums in f64, divided by R, rounded once -> (gW, gb, values f32; stats f64)"""
    r = r or restate(c)
    return [g.astype(F32) for g in r["gW"]], [g.astype(F32) for g in r["gb"]], r["values"].astype(F32), r["stats"]
