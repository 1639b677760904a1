"""The per-episode ledger on the device (include/chub.h: chub_set_episode_stats): the reference's cumulated_income / cumulated_draw_ele /
acumulate_reward / deviation / test_penalty (evcssp_manager.py:259-297), kept per env by the step's tail kernel.  Held here against (a) the
reference's own recordings in COMPAT, nine fixtures side by side on their own clocks; (b) the same handle's telemetry added up on the host,
bit for bit, in the one-launch and the two-launch step, in PHILOX and PHILOX_CURVES; (c) a host shadow through staggered clocks, device masks
and 200 auto-reset calls; (d) a captured graph against a twin that issues the same calls one by one; (e) the summary kernel's definition;
(f) copies and snapshots; (g) a handle that never asked."""
import ctypes as C
import math

import numpy as np
import pytest

import orclib
from charginghub_env_amd import _lib
from test_gpu_autoreset import Dev, buffers
from test_gpu_env_clocks import KW
from test_gpu_env_params_compat import FIELDS, FIXTURES, program
from test_gpu_parity import TIGHT, hub, kwargs_of

pytestmark = pytest.mark.gpu

T, EP, NAMES = _lib.T, _lib.EP, _lib.EPISODE_NAMES
NEP = len(NAMES)


def cap_mass_of(vlt):
    return (0.089 * (200 / 1)) * (np.asarray(vlt, dtype=np.float64) * 1000)  # env.py: _capacity_mass


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def block(v, finished):
    d = v.episode_stats(finished=finished)
    return np.stack([d[name] for name in NAMES], axis=1)  # [N, NEP]


class Shadow(object):
    """the ledger as the host computes it from the telemetry columns and reward_f64 of a step, in the order of the header's table"""

    def __init__(self, n, init_soc, cap_mass):
        self.n = n
        self.init_soc = np.broadcast_to(np.asarray(init_soc, dtype=np.float64), (n,)).copy()
        self.cap_mass = np.broadcast_to(np.asarray(cap_mass, dtype=np.float64), (n,)).copy()
        self.live, self.fin = np.zeros((n, NEP)), np.zeros((n, NEP))
        self.episodes, self.pending = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=bool)

    def reset(self, mask=None):
        m = np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        self.live[m] = 0.0
        self.live[m, EP["end_soc"]] = self.init_soc[m]

    def step(self, tel, r64, done, mask=None):
        m = np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        L = self.live
        soc = tel[:, T["Store_SOC"]]
        ret = L[:, EP["return"]] + r64
        inc = L[:, EP["income"]] + tel[:, T["income"]]
        drw = L[:, EP["draw_ele"]] + ((tel[:, T["ev_power_0_net"]] + tel[:, T["ev_power_1_net"]]) + tel[:, T["re_hydrogen_power"]])
        ln = L[:, EP["length"]] + 1.0
        dev = np.abs(soc - self.init_soc)
        pen = np.abs(np.abs(soc - self.init_soc) * self.cap_mass / 1000 / 0.2)  # env.py:391-393
        new = np.stack([ret, inc, drw, ln, dev, pen, soc], axis=1)
        L[m] = new[m]
        d = m & np.asarray(done, dtype=bool)
        self.fin[d] = L[d]
        self.episodes[d] += 1
        self.pending[d] = True

    def check(self, v, label):
        assert np.array_equal(bits(block(v, False)), bits(self.live)), (label, "live")
        assert np.array_equal(bits(block(v, True)), bits(self.fin)), (label, "finished")
        assert np.array_equal(v.episode_counts(), self.episodes), (label, "episodes")


# ---- (a) the reference's recordings, COMPAT, nine fixtures in one handle on their own clocks
@pytest.mark.parametrize("repeat", [1, 40])
def test_reference_fixtures_ledger_in_one_compat_handle(repeat):
    chub = hub()
    gs = [orclib.load_golden(name) for name in FIXTURES]
    kws = [kwargs_of(g) for g in gs]
    gs = [{key: g[key] for key in g.files} for g in gs]  # (an .npz member is read from the archive on every access)
    n = len(FIXTURES) * repeat
    fx = np.arange(n) % len(FIXTURES)
    rows = {f: [kws[k][f] for k in fx] for f in FIELDS}
    v = chub.VecChargingHub(n, rng="compat", station_list=[20, 25], station_type_list=["fast", "slow"], **rows)
    scratch = chub.VecChargingHub(1, rng="compat", **kws[0])
    v.set_telemetry(True)
    v.set_episode_stats(True)
    assert v.has_episode_stats and v.has_env_params
    A = v.act_dim
    v.set_compat_seeds(np.stack([gs[k]["ctor_seeds"] for k in fx]))
    v.compat_replay_constructor()
    progs = [program(g) for g in gs]
    seeds = [{int(ep): (int(a), int(b)) for ep, a, b in g["seeds"]} for g in gs]
    an = [list(g["attr_names"]) for g in gs]
    longest = max(len(p) for p, _ in progs)
    k_ep = np.zeros(n, dtype=np.int64)        # steps into the episode
    ret = np.zeros(n)                         # sequential f64 sum of the fixture's rewards since the env's reset
    episodes = np.zeros(n, dtype=np.uint32)
    done_steps = np.zeros(n, dtype=np.int64)
    for tau in range(longest):
        ops = {e: progs[fx[e]][0][tau] for e in range(n) if tau < len(progs[fx[e]][0])}
        resets = [e for e, op in ops.items() if op[0] == "reset"]
        movers = [e for e, op in ops.items() if op[0] == "step"]
        if resets:
            mask = np.zeros(n, dtype=bool)
            days, z = np.zeros((n, 2), dtype=np.int32), np.zeros((n, 3))
            st = None
            for e in resets:
                _, d_, z_, ep = ops[e]
                if ep is not None and ep in seeds[fx[e]]:
                    scratch.set_compat_seeds([seeds[fx[e]][ep]])
                    st = v.compat_state() if st is None else st
                    st[e] = scratch.compat_state()[0]
                mask[e], days[e], z[e] = True, d_, z_
            if st is not None:
                v.set_compat_state(st)
            before = block(v, True)
            v.reset_envs(mask, days, z)
            live = block(v, False)
            for e in resets:
                want = np.zeros(NEP)
                want[EP["end_soc"]] = kws[fx[e]]["init_soc"]
                assert np.array_equal(bits(live[e]), bits(want)), (FIXTURES[fx[e]], e, "reset")
                k_ep[e], ret[e] = 0, 0.0
            assert np.array_equal(bits(block(v, True)), bits(before)) and np.array_equal(v.episode_counts(), episodes)  # no reset touches them
        if movers:
            mask = np.zeros(n, dtype=bool)
            act, z = np.zeros((n, A), dtype=np.float32), np.zeros((n, 3))
            for e in movers:
                k, g = ops[e][1], gs[fx[e]]
                mask[e], act[e], z[e] = True, g["action"][k], g["exo_z"][k]
            before_live, before_fin = block(v, False), block(v, True)
            obs, rew, done, _ = v.step_envs(mask, act, z)
            live, fin, counts = block(v, False), block(v, True), v.episode_counts()
            still = ~mask
            assert np.array_equal(bits(live[still]), bits(before_live[still]))  # a masked call updates only the envs it serves
            for e in movers:
                k, g, name, a = ops[e][1], gs[fx[e]], FIXTURES[fx[e]], an[fx[e]]
                k_ep[e] += 1
                ret[e] += g["reward"][k]
                ke, at = k_ep[e], g["attrs"][k]
                for col, attr in (("income", "cumulated_income"), ("draw_ele", "cumulated_draw_ele")):
                    want = at[a.index(attr)]
                    assert abs(live[e, EP[col]] - want) <= ke * 1e-7 + 1e-9 * abs(want), (name, e, k, col, live[e, EP[col]], want)
                assert abs(live[e, EP["deviation"]] - at[a.index("deviation")]) <= TIGHT, (name, e, k, "deviation")
                assert live[e, EP["length"]] == ke, (name, e, k, "length")
                assert abs(live[e, EP["return"]] - ret[e]) <= ke * TIGHT, (name, e, k, "return", live[e, EP["return"]], ret[e])
                assert bool(done[e]) == bool(g["done"][k])
                if g["done"][k]:
                    want = at[a.index("test_penalty")]
                    assert abs(fin[e, EP["test_penalty"]] - want) <= TIGHT * abs(want), (name, e, k, "test_penalty", fin[e, EP["test_penalty"]], want)
                    episodes[e] += 1
                    done_steps[e] += 1
                    assert np.array_equal(bits(fin[e]), bits(live[e])), (name, e, k, "finished == live of that step")
                else:
                    assert np.array_equal(bits(fin[e]), bits(before_fin[e])), (name, e, k)
            assert np.array_equal(counts, episodes)
    past = FIXTURES.index("env_past_done")
    assert (done_steps[fx == past] == 2).all() and (k_ep[fx == past] == 250).all()  # two ends of day without a reset: the ledger kept running
    v.close()
    scratch.close()


# ---- (b) exact against the handle's own telemetry
def run_day_and_a_bit(rng, piles, n, seed=21, **opt):
    chub = hub()
    kw = dict(KW, station_list=list(piles))
    v = chub.VecChargingHub(n, seed=seed, rng=rng, env_id0=40, **dict(kw, **opt))
    v.set_telemetry(True)
    v.set_episode_stats(True)
    sh = Shadow(n, kw["init_soc"], cap_mass_of(kw["hydro_store_vlt"]))
    rs = np.random.RandomState(3)
    v.reset()
    sh.reset()
    sh.check(v, "reset")
    for t in range(96 + 1 + 10):
        if t == 96:
            v.reset()
            sh.reset()
        else:
            _, _, done, _ = v.step(rs.uniform(-1, 1, size=(n, v.act_dim)).astype(np.float32))
            assert done.all() == (t == 95) and done.any() == (t == 95)
            sh.step(v.telemetry(), v.reward_f64(), done)
        if t in (0, 1, 50, 95, 96, 106):
            sh.check(v, (rng, piles, n, opt, t))
    assert (sh.episodes == 1).all() and (sh.fin[:, EP["length"]] == 96).all() and (sh.live[:, EP["length"]] == 10).all()
    return v, sh


@pytest.mark.parametrize("rng,piles,n,opt,one_launch", [("philox", [20, 25], 130, {}, True), ("philox", [20, 25], 1000, {"fused_step": "off"}, False),
                                                        ("philox", [3, 2], 70, {}, None), ("philox_curves", [20, 25], 70, {}, None)],
                         ids=["one-launch-130", "two-launch-1000", "hub-3-2", "curves-70"])
def test_ledger_equals_the_sum_of_the_handles_own_telemetry(rng, piles, n, opt, one_launch):
    v, sh = run_day_and_a_bit(rng, piles, n, **opt)
    if one_launch is not None:
        assert v.uses_fused_step == one_launch
    if n == 130:  # ... and the two launch forms keep the same books
        w, _ = run_day_and_a_bit(rng, piles, n, fused_step="off")
        assert not w.uses_fused_step
        for fin in (False, True):
            assert np.array_equal(bits(block(v, fin)), bits(block(w, fin)))
        w.close()
    v.close()


# ---- (c) clocks, masks, auto-reset; (e) the summary
N_C = 300


@pytest.fixture(scope="module")
def staggered_run():
    """v: ledger on, driven by auto-reset calls; twin: the same seed, ledger off, driven by the calls the auto-reset call is defined as (a step
    of everybody, then a device-mask reset of those done) -- its telemetry between the two feeds the host shadow"""
    chub = hub()
    v, twin = (chub.VecChargingHub(N_C, seed=5, rng="philox", env_id0=7, **KW) for _ in range(2))
    twin.set_telemetry(True)
    v.set_episode_stats(True)
    sh = Shadow(N_C, KW["init_soc"], cap_mass_of(KW["hydro_store_vlt"]))
    rs = np.random.RandomState(9)
    group = np.arange(N_C) % 4
    for h in (v, twin):
        h.reset()
    sh.reset()
    for j in (1, 2, 3):
        for _ in range(17 + j):
            a = rs.uniform(-1, 1, size=(N_C, v.act_dim)).astype(np.float32)
            v.step(a)
            _, _, done, _ = twin.step(a)
            sh.step(twin.telemetry(), twin.reward_f64(), done)
        for h in (v, twin):
            h.reset_envs(group == j)
        sh.reset(group == j)
    assert v.clock_groups == 4
    sh.check(v, "staggered")
    dv, dt = Dev(v), Dev(twin)
    fired = np.zeros(N_C, dtype=np.int64)
    ones = np.ones(N_C, dtype=np.uint8)
    for s in range(200):
        a = rs.uniform(-1, 1, size=(N_C, v.act_dim)).astype(np.float32)
        packed, _ = dv.autoreset(a)
        _, _, done = dt.step_dmask(ones, a)
        sh.step(twin.telemetry(), twin.reward_f64(), done)
        dt.reset_dmask(done)
        sh.reset(done != 0)
        assert np.array_equal(packed[:, -1] > 0.5, done != 0), s
        fired += done != 0
        if s % 50 == 49:
            sh.check(v, ("auto-reset", s))
    yield v, sh, fired, dv
    v.close()
    twin.close()


def test_ledger_through_staggered_clocks_masks_and_autoreset(staggered_run):
    v, sh, fired, dv = staggered_run
    assert np.array_equal(v.episode_counts(), fired) and fired.min() >= 2
    fin, live = block(v, True), block(v, False)
    assert (fin[:, EP["length"]] == 96).all()
    assert np.array_equal(bits(fin), bits(sh.fin)) and np.array_equal(bits(live), bits(sh.live))
    # a device-mask step that names nobody changes no ledger entry
    dv.step_dmask(np.zeros(N_C, dtype=np.uint8), np.zeros((N_C, v.act_dim), dtype=np.float32))
    sh.check(v, "all-zero device mask")


def check_summary(raw, fin, pending, label):
    x = fin[pending]
    n = len(x)
    assert raw.shape == (1 + 4 * NEP,) and raw[0] == n, (label, raw[0], n)
    for c in range(NEP):
        s, ss, lo, hi = raw[1 + 4 * c:5 + 4 * c]
        col = [float(f) for f in x[:, c]]
        sq = [f * f for f in col]
        if n == 0:
            assert s == 0.0 and ss == 0.0 and lo == np.inf and hi == -np.inf, (label, c)
            continue
        assert lo == min(col) and hi == max(col), (label, c, "min / max are exact")
        # the error bound of ANY summation order of n f64 terms
        assert abs(s - math.fsum(col)) <= n * 2.0 ** -53 * math.fsum(abs(f) for f in col), (label, c, "sum", s, math.fsum(col))
        assert abs(ss - math.fsum(sq)) <= n * 2.0 ** -53 * math.fsum(sq), (label, c, "sumsq", ss, math.fsum(sq))


def test_summary_after_the_staggered_run(staggered_run):
    v, sh, fired, dv = staggered_run
    a, b = v.episode_summary_raw(drain=False), v.episode_summary_raw(drain=False)
    assert np.array_equal(bits(a), bits(b))  # no atomics, every order fixed
    assert sh.pending.all()
    check_summary(a, sh.fin, sh.pending, "staggered")
    # the device form into the caller's buffer: the same bits
    mg = buffers()
    out = mg.DeviceBuffer(8 * (1 + 4 * NEP))
    v.episode_summary_device(out.ptr, drain=False)
    v.sync()
    assert np.array_equal(bits(out.to_host(np.float64, (1 + 4 * NEP,))), bits(a))
    d = v.episode_summary(drain=True)
    assert d["count"] == N_C and d["length"] == {"mean": 96.0, "std": 0.0, "min": 96.0, "max": 96.0}
    assert abs(d["return"]["mean"] - sh.fin[:, EP["return"]].mean()) <= 1e-12 * abs(sh.fin[:, EP["return"]]).max()
    check_summary(v.episode_summary_raw(drain=True), sh.fin, np.zeros(N_C, dtype=bool), "drained")
    assert np.array_equal(bits(block(v, True)), bits(sh.fin))  # draining clears flags, not records


@pytest.mark.parametrize("n", [1, 257])  # one lane; one workgroup and one lane
def test_summary_small_batches(n):
    chub = hub()
    v = chub.VecChargingHub(n, seed=2, rng="philox", **KW)
    v.set_episode_stats(True)
    check_summary(v.episode_summary_raw(drain=True), np.zeros((n, NEP)), np.zeros(n, dtype=bool), "nothing finished yet")
    v.reset()
    rs = np.random.RandomState(n)
    half = np.arange(n) % 2 == 0
    for t in range(96):
        a = rs.uniform(-1, 1, size=(n, v.act_dim)).astype(np.float32)
        if t == 95 and n > 1:
            v.step_envs(half, a)  # only every other env ends its day
        else:
            v.step(a)
    pending = half if n > 1 else np.ones(1, dtype=bool)
    fin = block(v, True)
    assert np.array_equal(v.episode_counts(), pending.astype(np.uint32))
    a, b = v.episode_summary_raw(drain=False), v.episode_summary_raw(drain=True)
    assert np.array_equal(bits(a), bits(b))
    check_summary(a, fin, pending, n)
    check_summary(v.episode_summary_raw(drain=True), fin, np.zeros(n, dtype=bool), "drained")
    v.close()


# ---- (d) a captured graph of auto-reset calls with the summary and the block copy inside
def test_graph_with_summary_and_block_copy_equals_eager():
    chub = hub()
    mg = buffers()
    n = 52
    kw = dict(seed=77, rng="philox", env_id0=0, **KW)

    def start():
        v = chub.VecChargingHub(n, **kw)
        v.set_episode_stats(True)
        v.reset()
        rs_head = np.random.RandomState(1)
        head = rs_head.uniform(-1, 1, size=(n, v.act_dim)).astype(np.float32)
        for k in range(1, 79):
            v.step_envs(np.arange(n) * 7 // n * 13 >= k, head)
        return v

    g, e = start(), start()
    st = mg.Stream(0)
    dg, de = Dev(g, st.ptr), Dev(e)
    words = 1 + 4 * NEP
    bufs = [(mg.DeviceBuffer(8 * words), mg.DeviceBuffer(8 * NEP * n), mg.DeviceBuffer(4 * n)) for _ in range(2)]
    dg.act.from_host(np.zeros((n, g.act_dim), dtype=np.float32), st.ptr)
    st.sync()
    g.graph_begin(st.ptr)
    with pytest.raises(chub.ChubError, match="chub_graph_begin and chub_graph_end"):
        g.set_episode_stats(False)
    for k in range(8):
        g.step_autoreset_device(dg.act.ptr, dg.packed.ptr, dg.final.ptr, stream=st.ptr)
    g.episode_summary_device(bufs[0][0].ptr, drain=True, stream=st.ptr)
    g.episode_stats_device(bufs[0][1].ptr, bufs[0][2].ptr, finished=True, stream=st.ptr)
    graph = g.graph_end(st.ptr)
    rs = np.random.RandomState(8)
    ended = 0
    for r in range(3):
        act = rs.uniform(-1, 1, size=(n, g.act_dim)).astype(np.float32)
        dg.act.from_host(act, st.ptr)
        g.graph_launch(graph, st.ptr)
        for k in range(8):
            de.autoreset(act)
        e.episode_summary_device(bufs[1][0].ptr, drain=True)
        e.episode_stats_device(bufs[1][1].ptr, bufs[1][2].ptr, finished=True)
        st.sync()
        e.sync()
        got = [bufs[0][0].to_host(np.float64, (words,), st.ptr), bufs[0][1].to_host(np.float64, (NEP, n), st.ptr), bufs[0][2].to_host(np.uint32, (n,), st.ptr)]
        want = [bufs[1][0].to_host(np.float64, (words,)), bufs[1][1].to_host(np.float64, (NEP, n)), bufs[1][2].to_host(np.uint32, (n,))]
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(got[2], want[2]), r
        assert np.array_equal(bits(got[1].T), bits(block(g, True))) and np.array_equal(got[2], g.episode_counts())
        assert np.array_equal(bits(block(g, False)), bits(block(e, False))), r
        assert got[0][0] == got[2].sum() - ended  # the episodes that ended in this replay (each drained once)
        ended = int(got[2].sum())
    assert ended > 0
    g.graph_destroy(graph)
    g.close()
    e.close()
    st.destroy()


# ---- (f) copies and snapshots
def four_arrays(v):
    return [bits(block(v, False)), bits(block(v, True)), v.episode_counts()]


def test_copy_envs_carries_the_ledger():
    chub = hub()
    n, m = 40, 12
    src = chub.VecChargingHub(n, seed=3, rng="philox", **KW)
    dst = chub.VecChargingHub(m, seed=4, rng="philox", env_id0=500, **KW)
    off = chub.VecChargingHub(m, seed=4, rng="philox", env_id0=900, **KW)
    for v in (src, dst):
        v.set_episode_stats(True)
    rs = np.random.RandomState(0)
    for v in (src, dst, off):
        v.reset()
    for t in range(96 + 30):  # mid-episode, one finished episode behind it
        if t == 96:
            src.reset()
        src.step(rs.uniform(-1, 1, size=(n, src.act_dim)).astype(np.float32))
    for t in range(7):
        dst.step(rs.uniform(-1, 1, size=(m, dst.act_dim)).astype(np.float32))
    s_idx, d_idx = [3, 9, 17, 30, 39], [0, 2, 5, 6, 11]
    before = four_arrays(dst)
    s_pending = src.episode_summary_raw(drain=False)[0]
    assert s_pending == n and dst.episode_summary_raw(drain=False)[0] == 0
    dst.copy_envs(s_idx, d_idx, source=src)
    want, got = four_arrays(src), four_arrays(dst)
    others = np.setdiff1d(np.arange(m), d_idx)
    for a, b, w in zip(got, before, want):
        assert np.array_equal(a[d_idx], w[s_idx]) and np.array_equal(a[others], b[others])
    assert dst.episode_summary_raw(drain=False)[0] == 5  # the pending flags came along
    assert (block(dst, False)[d_idx, EP["length"]] == 30).all()
    for t in range(4):  # ... and they go on from there
        dst.step_envs(np.ones(m, dtype=bool), rs.uniform(-1, 1, size=(m, dst.act_dim)).astype(np.float32))
    assert (block(dst, False)[d_idx, EP["length"]] == 34).all() and (block(dst, False)[others, EP["length"]] == 11).all()
    for a, b in ((off, src), (src, off)):
        with pytest.raises(chub.ChubError, match="episode ledger"):
            a.copy_envs([0], [1], source=b)
    for v in (src, dst, off):
        v.close()


def test_snapshots_carry_the_ledger():
    chub = hub()
    n = 33
    v = chub.VecChargingHub(n, seed=8, rng="philox", **KW)
    off = chub.VecChargingHub(n, seed=8, rng="philox", **KW)
    v.set_episode_stats(True)
    rs = np.random.RandomState(1)
    acts = [rs.uniform(-1, 1, size=(n, v.act_dim)).astype(np.float32) for _ in range(20)]
    for h in (v, off):
        h.reset()
    for t in range(90):
        a = rs.uniform(-1, 1, size=(n, v.act_dim)).astype(np.float32)
        v.step(a)
        off.step(a)
    blob = v.get_state()
    blob_off = off.get_state()
    assert blob.size == blob_off.size + n * (2 * NEP * 8 + 4 + 1)  # larger by exactly the four arrays
    for a in acts:
        v.step(a)
    first = four_arrays(v) + [bits(v.episode_summary_raw(drain=False))]
    assert v.episode_counts().min() == 1
    v.set_state(blob)
    assert v.episode_counts().max() == 0 and (block(v, False)[:, EP["length"]] == 90).all()
    for a in acts:
        v.step(a)
    for a, b in zip(first, four_arrays(v) + [bits(v.episode_summary_raw(drain=False))]):
        assert np.array_equal(a, b)
    # one taken with the ledger on is refused by a handle with it off, and the other way round, with nothing written
    keep_v, keep_off = four_arrays(v), off.get_state()
    with pytest.raises(chub.ChubError, match="episode ledger"):
        off.set_state(blob)
    with pytest.raises(chub.ChubError, match="episode ledger"):
        v.set_state(blob_off)
    assert np.array_equal(off.get_state(), keep_off)
    for a, b in zip(keep_v, four_arrays(v)):
        assert np.array_equal(a, b)
    v.close()
    off.close()


def test_a_ledger_handle_does_not_become_a_tape_handle():
    chub = hub()
    v = chub.VecChargingHub(8, seed=1, rng="philox", **KW)
    v.set_episode_stats(True)
    with pytest.raises(chub.ChubError, match="keeps the episode ledger"):
        v.tape_register_soc([50.0])
    v.set_episode_stats(False)
    v.tape_register_soc([50.0])
    with pytest.raises(chub.ChubError, match="tape handle"):
        v.set_episode_stats(True)
    assert not v.has_episode_stats
    v.close()


# ---- (g) off means off
def test_off_means_off():
    chub = hub()
    n = 90
    a_, b_ = (chub.VecChargingHub(n, seed=6, rng="philox", **KW) for _ in range(2))
    lib = a_._lib
    out = np.zeros((n, NEP))
    cnt = np.zeros(n, dtype=np.uint32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    assert not a_.has_episode_stats
    for rc in (lib.chub_get_episode_stats(a_._h, 0, p(out)), lib.chub_get_episode_counts(a_._h, p(cnt)),
               lib.chub_episode_stats_device(a_._h, 1, p(out), None, None), lib.chub_episode_summary_device(a_._h, p(out), 1, None),
               lib.chub_episode_summary(a_._h, p(out), 1)):
        assert rc == -1 and b"episode ledger is off" in lib.chub_last_error()
    size_off = lib.chub_state_size(a_._h)
    b_.set_episode_stats(True)
    assert lib.chub_state_size(b_._h) == size_off + n * (2 * NEP * 8 + 4 + 1)
    rs = np.random.RandomState(4)
    for h in (a_, b_):
        h.reset()
    for t in range(30):
        if t == 12:
            b_.set_episode_stats(False)
            assert lib.chub_state_size(b_._h) == size_off
        act = rs.uniform(-1, 1, size=(n, a_.act_dim)).astype(np.float32)
        ra, rb = a_.step(act), b_.step(act)
        for j in range(3):
            assert np.array_equal(np.asarray(ra[j]).view(np.uint8), np.asarray(rb[j]).view(np.uint8)), (t, j)
    for x, y in zip(a_.slots() + [a_.station_scalars()] + list(a_.env_clocks(ticks=True)), b_.slots() + [b_.station_scalars()] + list(b_.env_clocks(ticks=True))):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    a_.close()
    b_.close()
