"""Per-env hub parameters (chub_create_params / chub_set_env_params, include/chub.h): one handle whose envs have different electrolysers,
tanks, fuel cells, FCEV traffic and fluctuations, as a vector of differently built reference envs (MGR:25-27).

What is pinned here: every env of a handle with rows computes bit for bit what a homogeneous handle built from its row computes (same
seed, same global env id) -- in PHILOX and PHILOX_CURVES, below and above the one-launch threshold of the homogeneous handles, eager, in
chub_run_steps and in graph replays; rows rewritten in place (set on a mask, then reset on it; a captured graph replayed after the
change); snapshots; and what such a handle refuses."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HUB = dict(station_list=[20, 25], station_type_list=["fast", "slow"])
FIELDS = ("hydro_prod_rate", "hydro_store_vlt", "init_soc", "fc_max_power", "fcev_permeate", "renew_fluctuate", "price_fluctuate", "hydro_loss")
# the configs of the issue: defaults, no electrolyser, 5 m^3 tanks at init_soc 0.1 and 1.0, the permeate > 1 quirk, a stuck forecourt,
# fluctuations with tank losses
CONFIGS = [
    dict(),
    dict(hydro_prod_rate=0.0),
    dict(hydro_store_vlt=5.0, init_soc=0.1),
    dict(hydro_store_vlt=5.0, init_soc=1.0),
    dict(fcev_permeate=1.5),
    dict(fcev_permeate=0.1, hydro_store_vlt=400.0),
    dict(renew_fluctuate=0.3, price_fluctuate=0.3, hydro_loss=0.02),
]
DEFAULTS = dict(hydro_prod_rate=430.0, hydro_store_vlt=5000.0, init_soc=0.5, fc_max_power=100.0, fcev_permeate=0.01, renew_fluctuate=0.0,
                price_fluctuate=0.0, hydro_loss=0.0)


def hub():
    import charginghub_env_amd as chub
    return chub


def row_kwargs(n, pick):
    """the eight kwargs as sequences: env i takes CONFIGS[pick(i)]"""
    return {f: [CONFIGS[pick(i)].get(f, DEFAULTS[f]) for i in range(n)] for f in FIELDS}


def _acts(n, A, seed, t):
    return np.random.RandomState(seed * 1000 + t).uniform(-1, 1, (n, A)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _snap(v):
    """everything a step leaves that introspection shows: slots, station scalars, telemetry"""
    return [s.copy() for s in v.slots()], v.station_scalars().copy(), v.telemetry().copy()


def _rows_of(snap, sel):
    slots, sc, tel = snap
    return [s[sel] for s in slots], sc[sel], tel[sel]


def _same(a, b, what):
    for k in (0, 1):
        assert np.array_equal(_bits(a[0][k]), _bits(b[0][k])), (what, "slots", k)
    assert np.array_equal(_bits(a[1]), _bits(b[1])), (what, "station scalars")
    assert np.array_equal(_bits(a[2]), _bits(b[2])), (what, "telemetry")


# ---------------------------------------------------------------------------------------------- 2. rows against homogeneous handles
@pytest.mark.parametrize("rng,n", [("philox", 1000), ("philox", 65536), ("philox_curves", 1000), ("philox_curves", 65536)])
def test_rows_equal_homogeneous_handles_bit_for_bit(rng, n):
    """N envs, env i on config i % K, against K homogeneous handles of N envs on the same seed: row i against handle i % K.  Two days and
    a cut-short episode of random actions.  At 1000 envs the homogeneous handles run the one-launch step, the handle with rows the
    two-launch step: the forms agree too."""
    chub = hub()
    K = len(CONFIGS)
    seed = 77
    rows = chub.VecChargingHub(n, seed=seed, rng=rng, **HUB, **row_kwargs(n, lambda i: i % K))
    homs = [chub.VecChargingHub(n, seed=seed, rng=rng, **HUB, **CONFIGS[k]) for k in range(K)]
    assert rows.has_env_params and not any(h.has_env_params for h in homs)
    assert not rows.uses_fused_step
    sel = [np.arange(n) % K == k for k in range(K)]
    every = 1 if n <= 1000 else 64  # (introspection of every env: each checkpoint copies the whole state of eight handles)
    for v in [rows] + homs:
        v.set_telemetry(True)
    steps = [("reset", 0)] + [("step", t) for t in range(96)] + [("reset", 0)] + [("step", t) for t in range(96)]
    steps += [("reset", 0)] + [("step", t) for t in range(17)]  # the cut-short episode
    for i, (kind, t) in enumerate(steps):
        if kind == "reset":
            outs = [v.reset() for v in [rows] + homs]
            for k in range(K):
                assert np.array_equal(_bits(outs[0][sel[k]]), _bits(outs[1 + k][sel[k]])), ("reset obs", i, k)
            continue
        a = _acts(n, rows.act_dim, seed, i)
        outs = [v.step(a) for v in [rows] + homs]
        for k in range(K):
            for j, what in enumerate(("obs", "reward", "done")):
                assert np.array_equal(_bits(outs[0][j][sel[k]]), _bits(outs[1 + k][j][sel[k]])), (what, i, k)
        if i % every == 0 or i == len(steps) - 1:
            s0 = _snap(rows)
            for k in range(K):
                _same(_rows_of(s0, sel[k]), _rows_of(_snap(homs[k]), sel[k]), ("step", i, "config", k))
    # the forecourt (the queue and line are telemetry columns, compared above): fcev_stuck_count of the handle = the sum over the configs'
    # own envs in their homogeneous handles
    assert rows.fcev_stuck_count() == sum(_stuck_among(homs[k], sel[k]) for k in range(K))
    for v in [rows] + homs:
        v.close()


def _stuck_among(v, sel):
    """envs of `sel` whose FCEV list is stuck (there is no per-env accessor): reset the others -- a reset empties their list -- count,
    and restore the handle from a snapshot"""
    blob = v.get_state()
    v.reset_envs(~sel)
    c = v.fcev_stuck_count()
    v.set_state(blob)
    return c


# ---------------------------------------------------------------------------------------------- 4. rows equal to cfg: every launch form
@pytest.mark.parametrize("rng", ["philox", "philox_curves"])
@pytest.mark.parametrize("form", ["eager", "graph", "run_steps"])
def test_rows_equal_to_cfg_are_the_homogeneous_handle(rng, form):
    chub = hub()
    from charginghub_env_amd import multi_gpu
    n = 1000
    cfg = CONFIGS[6]
    res = []
    for with_rows in (False, True):
        kw = {f: [cfg.get(f, DEFAULTS[f])] * n for f in FIELDS} if with_rows else dict(cfg)
        v = chub.VecChargingHub(n, seed=2024, rng=rng, **HUB, **kw)
        assert v.has_env_params == with_rows
        st = multi_gpu.Stream(0)
        acts = [multi_gpu.DeviceBuffer(n * v.act_dim * 4) for _ in range(4)]
        for bt, a in enumerate(acts):
            v.random_actions_device(a.ptr, 5, bt, st.ptr)
        packed = [multi_gpu.DeviceBuffer(n * (v.obs_dim + 2) * 4) for _ in range(2)]
        obs0 = multi_gpu.DeviceBuffer(n * v.obs_dim * 4)

        def day():
            for i in range(96):
                if i == 0:
                    v.reset_device(obs0.ptr, stream=st.ptr)
                v.step_device_packed(acts[i % 4].ptr, packed[i & 1].ptr, stream=st.ptr)

        if form == "eager":
            day()
            day()
        elif form == "graph":  # (a capture covers an even number of calls: two days of a reset and 96 steps)
            st.sync()
            v.graph_begin(st.ptr)
            day()
            day()
            g = v.graph_end(st.ptr)
            v.graph_launch(g, st.ptr)
            v.graph_destroy(g)
        else:
            c_acts = (C.c_void_p * 4)(*[a.ptr for a in acts])
            c_packed = (C.c_void_p * 2)(*[p.ptr for p in packed])
            chub._lib.check(v._lib.chub_run_steps(v._h, None, c_acts, 4, c_packed, None, obs0.ptr, 0, 192, st.ptr))
        st.sync()
        res.append((packed[1].to_host(np.float32, (n, v.obs_dim + 2), st.ptr), [s.copy() for s in v.slots()], v.station_scalars().copy()))
        for b in acts + packed + [obs0]:
            b.free()
        v.close()
    assert np.array_equal(_bits(res[0][0]), _bits(res[1][0]))
    for k in (0, 1):
        assert np.array_equal(_bits(res[0][1][k]), _bits(res[1][1][k]))
    assert np.array_equal(_bits(res[0][2]), _bits(res[1][2]))


# ---------------------------------------------------------------------------------------------- 5. set on a mask, reset on it
def test_set_env_params_then_reset_envs_on_half_the_envs():
    """A: rows R0, then R1 on half the envs + reset_envs of that half.  B: control, R0 throughout, the same calls.  C: created with R1 on
    that half.  After the reset A equals C everywhere (what survives a reset -- the OU states -- does not depend on the rows) and B on
    the untouched half."""
    chub = hub()
    n = 2048
    K = len(CONFIGS)
    r0 = row_kwargs(n, lambda i: i % K)
    half = (np.arange(n) // 7) % 2 == 0
    r1 = row_kwargs(n, lambda i: (i * 3 + 1) % K if half[i] else i % K)
    A = chub.VecChargingHub(n, seed=5, **HUB, **r0)
    B = chub.VecChargingHub(n, seed=5, **HUB, **r0)
    Cc = chub.VecChargingHub(n, seed=5, **HUB, **r1)
    hs = (A, B, Cc)
    for v in hs:
        v.set_telemetry(True)
        v.reset()
    for t in range(40):
        a = _acts(n, A.act_dim, 9, t)
        for v in hs:
            v.step(a)
    A.set_env_params(mask=half, **r1)  # (rows [N]: only those of the masked envs are read)
    got = A.env_params()
    for f in FIELDS:
        assert np.array_equal(got[f], np.asarray(r1[f], dtype=np.float64)), f
    outs = [v.reset_envs(half) for v in hs]
    assert np.array_equal(_bits(outs[0]), _bits(outs[2]))
    assert np.array_equal(_bits(outs[0][~half]), _bits(outs[1][~half]))
    for t in range(60):
        a = _acts(n, A.act_dim, 10, t)
        o = [v.step(a) for v in hs]
        for j in range(3):
            assert np.array_equal(_bits(o[0][j]), _bits(o[2][j])), (t, j)
            assert np.array_equal(_bits(o[0][j][~half]), _bits(o[1][j][~half])), (t, j)
    _same(_snap(A), _snap(Cc), "after the reset")
    _same(_rows_of(_snap(A), ~half), _rows_of(_snap(B), ~half), "untouched half")
    for v in hs:
        v.close()


# ---------------------------------------------------------------------------------------------- 6. a graph replayed after set_env_params
def test_graph_replay_after_set_env_params_equals_the_new_rows():
    """A captures two days, replays them with rows R0, gets R1, replays again.  D has R1 from the start and runs the same four days eagerly:
    every day starts with a reset of every env, so A's last day is D's, bit for bit."""
    chub = hub()
    from charginghub_env_amd import multi_gpu
    n = 4096
    K = len(CONFIGS)
    r0 = row_kwargs(n, lambda i: i % K)
    r1 = row_kwargs(n, lambda i: (i + 3) % K)
    out = []
    for which in ("graph", "eager"):
        v = chub.VecChargingHub(n, seed=11, **HUB, **(r0 if which == "graph" else r1))
        st = multi_gpu.Stream(0)
        acts = [multi_gpu.DeviceBuffer(n * v.act_dim * 4) for _ in range(2)]
        for bt, a in enumerate(acts):
            v.random_actions_device(a.ptr, 3, bt, st.ptr)
        packed = [multi_gpu.DeviceBuffer(n * (v.obs_dim + 2) * 4) for _ in range(2)]
        obs0 = multi_gpu.DeviceBuffer(n * v.obs_dim * 4)

        def day():
            v.reset_device(obs0.ptr, stream=st.ptr)
            for i in range(96):
                v.step_device_packed(acts[i % 2].ptr, packed[i & 1].ptr, stream=st.ptr)

        if which == "graph":  # (a capture covers an even number of calls and ends at the clock it began at: two days)
            st.sync()
            v.graph_begin(st.ptr)
            day()
            day()
            g = v.graph_end(st.ptr)
            v.graph_launch(g, st.ptr)
            st.sync()
            v.set_env_params(**r1)
            v.graph_launch(g, st.ptr)
            st.sync()
            v.graph_destroy(g)
        else:
            for _ in range(4):
                day()
            st.sync()
        out.append((np.stack([p.to_host(np.float32, (n, v.obs_dim + 2), st.ptr) for p in packed]), obs0.to_host(np.float32, (n, v.obs_dim), st.ptr),
                    [s.copy() for s in v.slots()], v.station_scalars().copy()))
        for b in acts + packed + [obs0]:
            b.free()
        v.close()
    (p0, o0, s0, c0), (p1, o1, s1, c1) = out
    assert np.array_equal(_bits(o0), _bits(o1))
    assert np.array_equal(_bits(p0), _bits(p1))  # (the last two steps' packed blocks)
    for k in (0, 1):
        assert np.array_equal(_bits(s0[k]), _bits(s1[k]))
    assert np.array_equal(_bits(c0), _bits(c1))


def test_graph_that_starts_with_a_step_sees_new_rows_on_its_next_replay():
    """A graph whose first call is a step (no reset in front of the change): its first step draws its own state-independent variates at
    every replay (a graph's first step never consumes draws the previous launch left), so the FCEV count of the first step after
    chub_set_env_params is already the new row's.  A replays a captured span of two days that starts and ends at slot 5; E makes the same
    calls one by one; both change their rows between the two passes.  Everything stays bit for bit equal."""
    chub = hub()
    from charginghub_env_amd import multi_gpu
    n = 2048
    K = len(CONFIGS)
    r0 = row_kwargs(n, lambda i: (i % 2) * 5)        # configs 0 and 5 (permeate 0.01 / 0.1: the create-time bound covers both)
    r1 = row_kwargs(n, lambda i: ((i + 1) % 2) * 5)  # ... swapped: every env's FCEV rate changes
    del K
    out = []
    for which in ("graph", "eager"):
        v = chub.VecChargingHub(n, seed=21, **HUB, **r0)
        v.set_telemetry(True)
        st = multi_gpu.Stream(0)
        acts = [multi_gpu.DeviceBuffer(n * v.act_dim * 4) for _ in range(2)]
        for bt, a in enumerate(acts):
            v.random_actions_device(a.ptr, 8, bt, st.ptr)
        packed = [multi_gpu.DeviceBuffer(n * (v.obs_dim + 2) * 4) for _ in range(2)]
        obs0 = multi_gpu.DeviceBuffer(n * v.obs_dim * 4)
        i = [0]

        def step():
            v.step_device_packed(acts[i[0] % 2].ptr, packed[i[0] & 1].ptr, stream=st.ptr)
            i[0] += 1

        def span():  # slot 5 -> slot 5 two days on: 91 steps, reset, 96 steps, reset, 5 steps (194 calls)
            for _ in range(91):
                step()
            for k in (96, 5):
                v.reset_device(obs0.ptr, stream=st.ptr)
                for _ in range(k):
                    step()

        v.reset_device(obs0.ptr, stream=st.ptr)
        for _ in range(5):
            step()
        if which == "graph":
            st.sync()
            v.graph_begin(st.ptr)
            span()
            g = v.graph_end(st.ptr)
            v.graph_launch(g, st.ptr)
            st.sync()
            v.set_env_params(**r1)
            v.graph_launch(g, st.ptr)
            st.sync()
            v.graph_destroy(g)
        else:
            span()
            st.sync()
            v.set_env_params(**r1)
            span()
            st.sync()
        out.append((np.stack([p.to_host(np.float32, (n, v.obs_dim + 2), st.ptr) for p in packed]), _snap(v)))
        for b in acts + packed + [obs0]:
            b.free()
        v.close()
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0]))
    _same(out[0][1], out[1][1], "graph vs eager after the change")


# ---------------------------------------------------------------------------------------------- 7. snapshots
def test_snapshot_round_trip_carries_the_rows_and_kinds_do_not_mix():
    chub = hub()
    n = 1024
    K = len(CONFIGS)
    r0 = row_kwargs(n, lambda i: i % K)
    v = chub.VecChargingHub(n, seed=3, **HUB, **r0)
    h = chub.VecChargingHub(n, seed=3, **HUB)
    v.reset()
    h.reset()
    for t in range(10):
        v.step(_acts(n, v.act_dim, 1, t))
    blob = v.get_state()
    ref = [v.step(_acts(n, v.act_dim, 2, t)) for t in range(20)]
    v.set_env_params(init_soc=0.9, hydro_loss=0.05)
    v.set_state(blob)
    for f in FIELDS:
        assert np.array_equal(v.env_params()[f], np.asarray(r0[f], dtype=np.float64)), f
    again = [v.step(_acts(n, v.act_dim, 2, t)) for t in range(20)]
    for a, b in zip(ref, again):
        for j in range(3):
            assert np.array_equal(_bits(a[j]), _bits(b[j]))
    hblob = h.get_state()
    with pytest.raises(chub.ChubError, match="per-env hub parameters"):
        h.set_state(blob)
    with pytest.raises(chub.ChubError, match="without per-env hub parameters"):
        v.set_state(hblob)
    v.close()
    h.close()


# ---------------------------------------------------------------------------------------------- 8. error paths
def test_errors_and_refusals():
    chub = hub()
    n = 64
    bad = {f: [DEFAULTS[f]] * n for f in FIELDS}
    bad["init_soc"][3] = 0.05
    with pytest.raises(chub.ChubError, match=r"-1: init_soc must be in \[0.1, 1\] \(env 3\)"):
        chub.VecChargingHub(n, **HUB, **bad)
    bad = {f: [DEFAULTS[f]] * n for f in FIELDS}
    bad["hydro_store_vlt"][5] = 0.0
    with pytest.raises(chub.ChubError, match=r"-1: hydrogen system sizes must be non-negative \(env 5\)"):
        chub.VecChargingHub(n, **HUB, **bad)
    with pytest.raises(ValueError, match="n_envs = 64"):
        chub.VecChargingHub(n, **HUB, init_soc=[0.5] * (n - 1))

    v = chub.VecChargingHub(n, **HUB, init_soc=[0.5] * n)  # fcev_permeate 0.01 everywhere: 1 arrival per step at most
    v.reset()
    with pytest.raises(chub.ChubError, match=r"-1: fcev_permeate gives up to \d+ FCEV arrivals per step, more than the 1 .*\(env 0\)"):
        v.set_env_params(fcev_permeate=0.1)
    bad = np.full(n, 0.5)
    bad[7] = 2.0
    with pytest.raises(chub.ChubError, match=r"-1: init_soc must be in \[0.1, 1\] \(env 7\)"):
        v.set_env_params(init_soc=bad)
    v.set_env_params(mask=np.arange(n) != 7, init_soc=bad)  # (env 7 not named: its row is not read)
    with pytest.raises(chub.ChubError, match="-4: the scalar-load control"):
        v.step_load(np.zeros((n, 2)), np.zeros((n, 2)))
    with pytest.raises(chub.ChubError, match="-4: tape mode"):
        v.tape_register_soc([50.0])
    A = v.act_dim
    with pytest.raises(chub.ChubError, match="-4: tape mode"):
        v.step_tape(np.zeros((n, A), np.float32), np.zeros((2, n), np.uint64), np.zeros((n, A - 2, 2), np.uint32))
    with pytest.raises(chub.ChubError, match="-4: tape mode"):
        v.reset_tape(np.zeros((2, n), np.uint32), np.zeros((n, A - 2, 2), np.uint32))
    with pytest.raises(chub.ChubError, match="-4: chub_get_hy_table"):
        v.hy_table()
    with pytest.raises(chub.ChubError, match="-4: chub_set_hy_table"):
        v.set_hy_table(np.zeros(102))
    v.close()


def test_hy_table_of_each_env_is_the_homogeneous_handles_table():
    chub = hub()
    K = len(CONFIGS)
    n = 2 * K
    v = chub.VecChargingHub(n, **HUB, **row_kwargs(n, lambda i: i % K))
    for k in range(K):
        h = chub.VecChargingHub(1, **HUB, **CONFIGS[k])
        want = h.hy_table()
        h.close()
        for e in (k, k + K):
            assert np.array_equal(_bits(v.hy_table(env=e)), _bits(want)), (k, e)
    v.close()
