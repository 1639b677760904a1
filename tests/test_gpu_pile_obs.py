"""Per-pile observations on the device (include/chub.h: chub_pile_obs_device): Station::situation (CHS.hpp:204-231) and the two stay counters
(CHS.hpp:245-246) of every pile as columns [N][C][S], written by one launch.  Held here against (1) chub_get_slots, bit for bit, in the three
RNG modes and hub shapes from one pile to 300; (2) the oracle directly in the Philox modes and the reference's own recording in COMPAT;
(3) field subsets; (4) device masks; (5) every way the state gets where it is -- device-mask steps, the auto-reset step, copies, snapshots,
per-env parameter rows; (6) a range of many workgroups; (7) a captured graph; (8) a twin that never calls it; (9) refusals; (10) the torch
adapter."""
import numpy as np
import pytest

import orclib
from orclib import orc, ptr
from charginghub_env_amd import _lib
from test_gpu_autoreset import Dev, buffers
from test_gpu_parity import _oracle_vec, hub, kwargs_of

pytestmark = pytest.mark.gpu

ALL = (1 << _lib.PILE_COUNT) - 1
BASE = dict(station_type_list=["fast", "slow"], hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2, fc_max_power=100.0, fcev_permeate=0.01)
MODES = ("philox", "philox_curves", "compat")
CANARY = np.uint32(0x7FC0BEEF)  # a NaN no kernel writes


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def host_form(v):
    """chub_get_slots' per-station blocks re-ordered into [N][9][S], station 0's piles first"""
    return np.concatenate(v.slots(), axis=2)


def same(got, want, what):
    bad = np.nonzero(bits(got) != bits(want))
    assert bad[0].size == 0, (what, "first (env, column, slot)", [int(x[0]) for x in bad], bad[0].size, got[bad][:5], want[bad][:5])


def variates(rs, n):
    return np.stack([rs.randint(0, 100, n), rs.randint(0, 150, n)], axis=1).astype(np.int32), rs.normal(size=(n, 3))


def make(rng, piles, n, seed=11, **extra):
    chub = hub()
    v = chub.VecChargingHub(n, seed=seed, rng=rng, station_list=list(piles), **dict(BASE, **extra))
    if rng == "compat":
        rs = np.random.RandomState(3)
        v.set_compat_seeds(np.stack([rs.randint(1, 2**31 - 1, n), rs.randint(1, 2**31 - 1, n)], axis=1).astype(np.uint32))
        v.compat_replay_constructor()
    return v


class Driver(object):
    """reset and random-action steps on a fixed key; COMPAT takes its exogenous variates from a seeded generator"""

    def __init__(self, v, rng, key=5):
        self.v, self.compat, self.rs = v, rng == "compat", np.random.RandomState(key)

    def reset(self):
        d, z = variates(self.rs, self.v.n_envs) if self.compat else (None, None)
        return self.v.reset(d, z)

    def action(self):
        a = self.rs.uniform(-1, 1, size=(self.v.n_envs, self.v.act_dim)).astype(np.float32)
        return a, (self.rs.normal(size=(self.v.n_envs, 3)) if self.compat else None)

    def step(self):
        return self.v.step(*self.action())


# ---- 1. against chub_get_slots, bit for bit
SHAPES = [(rng, piles, False) for rng in MODES for piles in ([20, 25], [1, 1], [0, 7], [64, 64])] + \
         [(rng, piles, False) for rng in ("philox", "compat") for piles in ([65, 3], [300, 3])] + [(rng, [20, 25], True) for rng in MODES]


@pytest.mark.parametrize("rng,piles,cc", SHAPES, ids=lambda c: str(c).replace(" ", ""))
def test_columns_equal_get_slots(rng, piles, cc):
    """chub_get_slots is k_pile_obs with all nine fields, fetched and re-ordered on the host into per-station blocks: both sides of this bit
    comparison come from the one device decode.  What it holds is that host re-ordering, in every mode and shape, and (with the field-subset
    and mask tests below, which compare to the same form) the kernel's column subset / offset logic against the all-fields launch.  The
    decode itself is held to the oracle and the reference's recordings: test_columns_equal_the_oracle, the COMPAT test behind it, and the
    slots() comparisons of test_gpu_parity.py, test_gpu_big_stations.py, test_gpu_soc_curves_oracle.py and test_gpu_tape.py."""
    n = 67 if piles == [20, 25] else 5
    v = make(rng, piles, n, constant_charging=cc)
    S = piles[0] + piles[1]
    d = Driver(v, rng)
    d.reset()
    got = v.pile_obs()
    assert got.shape == (n, 9, S) and got.dtype == np.float32
    same(got, host_form(v), (rng, piles, "after the reset"))
    left = np.zeros((n, S), dtype=bool)  # piles a car has left
    refilled = False
    had = host_form(v)[:, 0] == 1
    for t in range(1, 41):
        d.step()
        want = host_form(v)
        if t <= 12 or t == 40:
            same(v.pile_obs(), want, (rng, piles, "step", t))
            empty = want[:, 0] == 0
            assert (want[:, 7][empty] == -1).all() and (want[:, 8][empty] == -1).all() and (want[:, 2:7].transpose(0, 2, 1)[empty] == 0).all()
        car = want[:, 0] == 1
        left |= had & ~car
        refilled |= bool((left & car).any())
        had = car
    if S >= 45:
        assert left.any() and refilled  # by step 40 cars have left and their piles have been taken again
    v.close()


# ---- 2. against the oracle (Philox modes) and the reference's recording (COMPAT): the decode itself
# (a PHILOX_CURVES handle takes stations of at most 64 piles: [65, 3] exists in PHILOX alone, as in SHAPES above)
ORACLE_SHAPES = [(rng, piles) for rng in ("philox", "philox_curves") for piles in ([20, 25], [1, 1], [0, 7], [64, 64])] + [("philox", [65, 3])]


@pytest.mark.parametrize("rng,piles", ORACLE_SHAPES, ids=lambda c: c if isinstance(c, str) else "%d,%d" % tuple(c))
def test_columns_equal_the_oracle(rng, piles):
    """all nine columns bit for bit, from chub_pile_obs_device and from chub_get_slots: tests/test_gpu_parity.py and
    tests/test_gpu_soc_curves_oracle.py hold chub_get_slots' power and emergency to the oracle's by uint32 equality like the other seven, so
    the same holds here.  The shapes are test_columns_equal_get_slots' within the plain oracle's 256 piles per station: one pile, a station
    of none, a full wave per station and one pile more."""
    chub = hub()
    kw = dict(BASE, station_list=piles, constant_charging=False, renew_fluctuate=0.0, price_fluctuate=0.0, hydro_loss=0.0)
    n, steps = (8, 30) if piles == [20, 25] else (5, 12)
    seed, env_id0, S = 0xC0FFEE12345, 1000, sum(piles)
    v = chub.VecChargingHub(n, seed=seed, rng=rng, env_id0=env_id0, **kw)
    cfg, h = _oracle_vec(kw, n, env_id0, seed, rng=rng)
    o_obs, o_rew, o_done = np.zeros((n, v.obs_dim)), np.zeros(n), np.zeros(n, dtype=np.uint8)

    def oracle_form():
        out = []
        for k, nk in enumerate(piles):
            w = np.zeros((n, 9, nk), dtype=np.float32)
            orc.orc_vec_slots(h, k, ptr(w))
            out.append(w)
        return np.concatenate(out, axis=2)

    def check(what):
        want = oracle_form()
        assert want.shape == (n, 9, S)
        same(v.pile_obs(), want, (rng, piles, "pile_obs") + what)
        same(host_form(v), want, (rng, piles, "slots") + what)

    rs = np.random.RandomState(7)
    v.reset()
    orc.orc_vec_reset(h, None, None, ptr(o_obs))
    check(("reset",))
    cars = 0
    for t in range(steps):
        act = rs.uniform(-1, 1, size=(n, v.act_dim)).astype(np.float32)
        if t % 7 == 0:
            act[:, :S] = 1.0
        v.step(act)
        orc.orc_vec_step(h, ptr(act), None, ptr(o_obs), ptr(o_rew), ptr(o_done), 4)
        check(("step", t))
        cars += int(oracle_form()[:, 0].sum())
    assert cars > 0  # (the comparison was not one of empty piles)
    orc.orc_vec_destroy(h)
    v.close()


def test_columns_equal_the_reference_recording_in_compat():
    """env_c3_random, replayed as test_gpu_parity.py::test_compat_matches_reference_golden replays it: the device columns against the rows
    the unmodified reference recorded (slots0 / slots1)"""
    chub = hub()
    name, n = "env_c3_random", 3
    g = orclib.load_golden(name)
    kw = kwargs_of(g)
    g = {key: g[key] for key in g.files}
    v = chub.VecChargingHub(n, rng="compat", **kw)
    rep = lambda a: np.repeat(np.asarray(a)[None, :], n, axis=0)
    v.set_compat_seeds(rep(g["ctor_seeds"]))
    v.compat_replay_constructor()
    v.reset(rep(g["ctor_days"]), rep(g["ctor_z"]))
    seeds = {int(ep): (int(a), int(b)) for ep, a, b in g["seeds"]}
    steps = int(g["steps_per_episode"])
    i = 0
    for ep in range(int(g["episodes"])):
        if ep in seeds:
            v.set_compat_seeds(rep(seeds[ep]))
        v.reset(rep(g["reset_days"][ep]), rep(g["reset_z"][ep]))
        for t in range(steps):
            v.step(rep(g["action"][i]), rep(g["exo_z"][i]))
            want = np.concatenate([g["slots0"][i], g["slots1"][i]], axis=1).astype(np.float32)
            same(v.pile_obs(), rep3(want, n), (name, ep, t))
            i += 1
    assert i > 0
    v.close()


def rep3(a, n):
    return np.repeat(a[None], n, axis=0)


# ---- 3. field subsets
@pytest.mark.parametrize("rng", MODES)
def test_field_subsets_are_the_matching_columns(rng):
    mg = buffers()
    n, S = 9, 45
    v = make(rng, [20, 25], n)
    d = Driver(v, rng)
    d.reset()
    for _ in range(9):
        d.step()
    full = v.pile_obs()
    same(full, host_form(v), (rng, "all fields"))
    extra = 64
    for mask in (0b000000001, 0b000010101, 0b110000000):
        cols = [f for f in range(9) if mask >> f & 1]
        assert v._lib.chub_pile_obs_columns(mask) == len(cols)
        count = n * len(cols) * S
        buf = mg.DeviceBuffer((count + extra) * 4)
        buf.from_host(np.full(count + extra, CANARY, dtype=np.uint32))
        v.pile_obs_device(buf.ptr, mask)
        raw = buf.to_host(np.uint32, (count + extra,))
        assert (raw[count:] == CANARY).all(), (rng, mask, "the words past N * C * S")
        same(raw[:count].view(np.float32).reshape(n, len(cols), S), full[:, cols], (rng, mask))
        same(v.pile_obs(mask), full[:, cols], (rng, mask, "host form"))
        same(v.pile_obs([_lib.PILE_NAMES[f] for f in reversed(cols)]), full[:, cols], (rng, mask, "by name"))
        buf.free()
    v.close()


# ---- 4. masks
@pytest.mark.parametrize("rng", MODES)
def test_a_device_mask_writes_only_the_rows_it_names(rng):
    mg = buffers()
    n, S = 67, 45
    v = make(rng, [20, 25], n)
    d = Driver(v, rng)
    d.reset()
    for _ in range(6):
        d.step()
    full = v.pile_obs()
    same(full, host_form(v), rng)
    named = [0, 3, 64, 66]
    m = np.zeros(n, dtype=np.uint8)
    m[named] = 1
    m[3] = 255  # (any non-zero byte names an env)
    d_mask, buf = mg.DeviceBuffer(n), mg.DeviceBuffer(n * 9 * S * 4)
    pattern = np.full((n, 9, S), CANARY, dtype=np.uint32)
    for mask_rows, fields, cols in ((m, ALL, list(range(9))), (m, 0b000010101, [0, 2, 4]), (np.zeros(n, dtype=np.uint8), ALL, list(range(9)))):
        C_ = len(cols)
        buf.from_host(pattern)
        d_mask.from_host(mask_rows)
        v.pile_obs_device(buf.ptr, fields, d_mask=d_mask.ptr)
        raw = buf.to_host(np.uint32, (n * 9 * S,))
        got = raw[:n * C_ * S].reshape(n, C_, S)
        on = mask_rows != 0
        assert np.array_equal(got[on], bits(full[:, cols])[on]), (rng, fields, "named rows")
        assert (got[~on] == CANARY).all() and (raw[n * C_ * S:] == CANARY).all(), (rng, fields, "every other row keeps the pattern")
    v.close()


# ---- 5. every way the state gets where it is
@pytest.mark.parametrize("rng", MODES)
def test_after_device_mask_steps(rng):
    n = 37
    v = make(rng, [20, 25], n)
    drv = Driver(v, rng)
    drv.reset()
    d = Dev(v)
    rs = np.random.RandomState(2)
    for t in range(14):
        mask = rs.uniform(size=n) < 0.5
        mask[t % n] = True
        a, z = drv.action()
        d.step_dmask(mask, a, z)
        same(v.pile_obs(), host_form(v), (rng, "device-mask step", t))
    assert v.clock_groups > 1
    v.close()


def test_after_the_autoreset_step_across_a_days_end():
    """16 envs, 4 of them cloned in at another time of day: 97 auto-reset steps from the reset, so that 12 envs end their day at step 96
    (and show their new episode's piles) and the clones at step 66"""
    n = 16
    v, src = make("philox", [20, 25], n, seed=5), make("philox", [20, 25], n, seed=6)
    rs = np.random.RandomState(9)
    act = lambda: rs.uniform(-1, 1, size=(n, v.act_dim)).astype(np.float32)
    src.reset()
    for _ in range(30):
        src.step(act())
    v.reset()
    v.copy_envs([0, 1, 2, 3], [12, 13, 14, 15], source=src)
    same(v.pile_obs()[12:], src.pile_obs()[:4], "clones show their sources' piles")
    d = Dev(v)
    ended = np.zeros(n, dtype=int)
    for t in range(1, 98):
        packed, _ = d.autoreset(act())
        done = packed[:, -1] > 0.5
        ended += done
        if done.any() or t % 8 == 0 or t == 97:
            same(v.pile_obs(), host_form(v), ("auto-reset step", t))
        if t == 66:
            assert done[12:].all() and not done[:12].any()
        if t == 96:
            assert done[:12].all() and not done[12:].any()
    assert (ended == 1).all()
    v.close()
    src.close()


@pytest.mark.parametrize("rng", MODES)
def test_after_copies_snapshots_and_with_parameter_rows(rng):
    n = 12
    rs = np.random.RandomState(4)
    v = make(rng, [20, 25], n, init_soc=list(rs.uniform(0.15, 0.6, n)), hydro_store_vlt=list(rs.uniform(20, 60, n)))
    assert v.has_env_params
    d = Driver(v, rng)
    d.reset()
    for t in range(10):
        d.step()
        same(v.pile_obs(), host_form(v), (rng, "parameter rows", t))
    at_snapshot, snap = v.pile_obs(), v.get_state()
    for t in range(7):
        d.step()
    later = v.pile_obs()
    assert not np.array_equal(bits(later), bits(at_snapshot))
    v.copy_envs([0, 1, 2], [9, 10, 11])
    got = v.pile_obs()
    same(got[9:], later[:3], (rng, "copies: the destination rows are the source rows"))
    same(got[:9], later[:9], (rng, "copies: the others are where they were"))
    same(got, host_form(v), (rng, "after the copy"))
    v.set_state(snap)
    same(v.pile_obs(), at_snapshot, (rng, "after set_state"))
    same(v.pile_obs(), host_form(v), (rng, "after set_state, host form"))
    v.close()


# ---- 6. many workgroups
def test_a_range_of_many_workgroups():
    """4099 envs x 45 piles = 184 455 lanes: 720 full workgroups and one of 135 lanes"""
    n = 4099
    v = make("philox", [20, 25], n)
    d = Driver(v, "philox")
    d.reset()
    for _ in range(10):
        d.step()
    same(v.pile_obs(), host_form(v), "4099 envs")
    v.close()


# ---- 7. a captured graph
def test_recorded_into_a_graph_it_takes_no_tick():
    """two days (a reset and 96 steps each: a graph covers an even number of resets + steps, and a lock-step replay starts at the clock it was
    captured at), every step followed by the call into ONE buffer; the twin records the same graph without the calls"""
    mg = buffers()
    n, S = 64, 16
    ticks = []
    for with_calls in (True, False):
        v = make("philox", [8, 8], n, seed=77)
        st = mg.Stream(0)
        acts = [mg.DeviceBuffer(n * v.act_dim * 4) for _ in range(4)]
        for b, a in enumerate(acts):
            v.random_actions_device(a.ptr, 5, b, st.ptr)
        packed, obs0 = mg.DeviceBuffer(n * (v.obs_dim + 2) * 4), mg.DeviceBuffer(n * v.obs_dim * 4)
        out = mg.DeviceBuffer(n * 9 * S * 4)
        out.from_host(np.full(n * 9 * S, CANARY, dtype=np.uint32))
        st.sync()
        v.graph_begin(st.ptr)
        for i in range(192):
            if i % 96 == 0:
                v.reset_device(obs0.ptr, stream=st.ptr)
            v.step_device_packed(acts[i % 4].ptr, packed.ptr, stream=st.ptr)
            if with_calls:
                v.pile_obs_device(out.ptr, stream=st.ptr)
        g = v.graph_end(st.ptr)
        if with_calls:
            assert (out.to_host(np.uint32, (n * 9 * S,), st.ptr) == CANARY).all()  # nothing ran while recording
        for replay in range(2):
            v.graph_launch(g, st.ptr)
            st.sync()
            if with_calls:
                same(out.to_host(np.float32, (n, 9, S), st.ptr), host_form(v), ("replay", replay))
        ticks.append(v.env_clocks(ticks=True))
        v.graph_destroy(g)
        if with_calls:
            o_with = v.step(np.zeros((n, v.act_dim), dtype=np.float32))[0]
        else:
            assert np.array_equal(v.step(np.zeros((n, v.act_dim), dtype=np.float32))[0], o_with)  # the two runs are one simulation
        v.close()
        st.destroy()
    assert np.array_equal(ticks[0][0], ticks[1][0]) and np.array_equal(ticks[0][1], ticks[1][1])
    assert ticks[0][1].min() > 0  # (the replays did move it)


# ---- 8. no side effects
@pytest.mark.parametrize("rng", MODES)
def test_a_twin_that_never_calls_computes_the_same(rng):
    """Two handles on one seed, one calls after every step.  Their outputs are compared step by step and their state through every
    getter; the snapshot BLOBS of two handles cannot be compared byte for byte (the arena a blob copies holds the handle's device context,
    i.e. its own device addresses), so the blob comparison is made on the calling handle itself: the run with the calls against the same
    run from the same snapshot without them."""
    mg = buffers()
    n = 21
    a_, b_ = make(rng, [20, 25], n, seed=3), make(rng, [20, 25], n, seed=3)
    da, db = Driver(a_, rng), Driver(b_, rng)
    buf = mg.DeviceBuffer(n * 9 * 45 * 4)

    def run(v, d, calls):
        outs = []
        for t in range(20):
            outs.append(d.step()[:3])
            if calls:
                v.sync()
                v.pile_obs_device(buf.ptr)
                v.pile_obs_device(buf.ptr, ("car", "emergency", "soc"))
        v.sync()
        return outs

    oa, ob = da.reset(), db.reset()
    assert np.array_equal(oa, ob)
    start = a_.get_state()
    a_.set_state(start)  # (both of this handle's runs start from the snapshot: the same host-side path into the first step)
    rs_state = da.rs.get_state()
    ra, rb = run(a_, da, True), run(b_, db, False)
    for t, (x, y) in enumerate(zip(ra, rb)):
        assert all(np.array_equal(p, q) for p, q in zip(x, y)), (rng, "packed outputs", t)
    assert a_.get_state().size == b_.get_state().size
    same(host_form(a_), host_form(b_), (rng, "slots"))
    assert np.array_equal(a_.station_scalars(), b_.station_scalars())
    assert all(np.array_equal(p, q) for p, q in zip(a_.env_clocks(ticks=True), b_.env_clocks(ticks=True)))
    if rng == "compat":
        assert np.array_equal(a_.compat_state(), b_.compat_state())
    blob_with = a_.get_state()
    a_.set_state(start)
    da.rs.set_state(rs_state)
    again = run(a_, da, False)
    for t, (x, y) in enumerate(zip(ra, again)):
        assert all(np.array_equal(p, q) for p, q in zip(x, y)), (rng, "the same run without the calls", t)
    assert np.array_equal(a_.get_state(), blob_with), (rng, "snapshot blobs")
    a_.close()
    b_.close()


# ---- 9. refusals
def test_refusals():
    chub = hub()
    mg = buffers()
    v = make("philox", [20, 25], 8)
    v.reset()
    buf = mg.DeviceBuffer(8 * 9 * 45 * 4)
    lib = v._lib
    assert lib.chub_pile_obs_device(v._h, 0, None, buf.ptr, None) == -1
    assert lib.chub_pile_obs_device(v._h, 1 << 9, None, buf.ptr, None) == -1
    assert lib.chub_pile_obs_device(v._h, ALL, None, None, None) == -1
    with pytest.raises(ValueError):
        v.pile_obs(("car", "speed"))
    size = v.get_state().size
    v.pile_obs_device(buf.ptr)
    assert v.get_state().size == size  # the SoC table is no snapshot state
    v.tape_register_soc(np.array([50.0], dtype=np.float32))  # a tape handle from here on
    assert lib.chub_pile_obs_device(v._h, ALL, None, buf.ptr, None) == -4
    assert "tape handle" in lib.chub_last_error().decode()
    with pytest.raises(chub.ChubError, match="tape handle"):
        v.pile_obs()
    v.close()


# ---- 10. the torch adapter
TORCH_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["CHUB_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHUB_ROOT"], "tests"))
import torch  # before libchub: both must share one HIP runtime
torch.cuda.set_device(0)
import test_gpu_pile_obs
test_gpu_pile_obs.torch_adapter_pile_obs()
print("TORCH_PILE_OBS_OK")
"""


def test_torch_adapter():
    """in a child process that imports torch first (as tests/test_gpu_torch_side.py does)"""
    import os
    import subprocess
    import sys
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch without a device")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], env=dict(os.environ, CHUB_ROOT=root), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "TORCH_PILE_OBS_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def torch_adapter_pile_obs():
    import inspect

    import torch
    from charginghub_env_amd import wrappers
    n = 64
    names = ("car", "emergency", "soc")
    for autoreset in ("per_env", True, False):
        env = wrappers.TorchHubVecEnv(n, [20, 25], ["fast", "slow"], seed=13, autoreset=autoreset, pile_obs=names,
                                      **{k: BASE[k] for k in BASE if k != "station_type_list"})
        assert env.pile_names == names
        cols = [_lib.PILE[x] for x in names]
        env.reset()
        p = env.pile_obs()
        assert tuple(p.shape) == (n, 3, 45) and p.dtype == torch.float32 and p.is_cuda
        same(p.cpu().numpy(), host_form(env.vec)[:, cols], (autoreset, "after reset()"))
        g = torch.Generator(device="cuda").manual_seed(1)
        for t in range(100 if autoreset == "per_env" else 20):
            env.step(torch.rand((n, env.act_dim), device="cuda", generator=g) * 2 - 1)
            q = env.pile_obs()
            assert q.data_ptr() == p.data_ptr()  # one buffer the adapter owns
            if t % 10 == 9 or t in (95, 96):
                same(q.cpu().numpy(), host_form(env.vec)[:, cols], (autoreset, "step", t))
        env.close()
    # the call path issues no host synchronisation: the adapter's method and the two below it are an enqueue and nothing else
    from charginghub_env_amd import vec_env
    for fn in (wrappers.TorchHubVecEnv.pile_obs, vec_env.VecChargingHub.pile_obs_device):
        src = inspect.getsource(fn)
        assert "sync" not in src.split('"""')[-1] and "cpu()" not in src and "to_host" not in src, fn
    off = wrappers.TorchHubVecEnv(8, [20, 25], ["fast", "slow"], seed=1)
    with pytest.raises(RuntimeError):
        off.pile_obs()
    off.close()
