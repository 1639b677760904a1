"""Step terms on the device (include/chub.h: chub_get_step_terms_device, chub_set_step_terms): what a step's reward is made of, the hydrogen
side and the constraint costs, [N][C], one read-only launch over the telemetry block.  The expected values are always
tests/step_terms_lib.py's numpy definition (held to the reference's recorded attributes by tests/test_step_terms_cpu.py) on the block
chub_get_telemetry reports; the comparison is bit for bit and every output buffer is pre-filled with a NaN no kernel writes, with a
guard row behind it.  Held here: (1) kernel == definition in the three RNG modes, four hub shapes and both homes of the block, field
subsets and device masks; (2) per-env rows; (3) the identities that tie the terms to the tail's own reward and to the ledger; (4) the
reference's recorded attributes through the drop-in class; (5) the attached output in every step form, the auto-reset ordering, a
captured graph, refusals; (6) the torch adapter."""
import numpy as np
import pytest

import orclib
import step_terms_lib as stl
from charginghub_env_amd import _lib
from test_gpu_autoreset import Dev, buffers, random_mask
from test_gpu_parity import PY_SEEDS, TIGHT, close, hub, kwargs_of
from test_gpu_pile_obs import BASE, CANARY, MODES, Driver, make

pytestmark = pytest.mark.gpu

ST, T, EP = _lib.ST, _lib.T, _lib.EP
ALL = stl.ALL
NC = _lib.ST_COUNT
GUARD = 256  # words behind the output that must keep the canary
EVERY_THIRD = sum(1 << f for f in range(0, NC, 3))


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want, what, view=bits32):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(view(got) != view(want))
    assert bad[0].size == 0, (what, "first (env, column)", [int(x[0]) for x in bad], bad[0].size, got[bad][:5], want[bad][:5])


def expected(v, init_soc=None, vlt=None):
    """the definition on the handle's telemetry block: float64 [N, 27]"""
    init_soc = BASE["init_soc"] if init_soc is None else init_soc
    vlt = BASE["hydro_store_vlt"] if vlt is None else vlt
    return stl.terms(v.telemetry(), init_soc, stl.cap_mass_of(vlt))


class Out(object):
    """a device buffer for [N, 27] floats, canary-filled on demand, with a guard row behind it"""

    def __init__(self, n):
        self.n, self.floats = n, n * NC
        self.buf = buffers().DeviceBuffer((self.floats + GUARD) * 4)
        self.ptr = self.buf.ptr

    def fill(self):
        self.buf.from_host(np.full(self.floats + GUARD, CANARY, dtype=np.uint32))

    def words(self, fields=ALL):
        """the N * C words a call with `fields` may write, uint32 [N, C]; everything behind them is intact"""
        C_ = len(stl.cols_of(fields))
        w = self.buf.to_host(np.uint32, (self.floats + GUARD,))
        assert (w[self.n * C_:] == CANARY).all(), (fields, "the words past N * C")
        return w[:self.n * C_].reshape(self.n, C_)

    def call(self, v, fields=ALL, d_mask=0, stream=0):
        self.fill()
        v.sync()
        v.step_terms_device(self.ptr, fields, d_mask=d_mask, stream=stream)
        v.sync()
        return self.words(fields)

    def free(self):
        self.buf.free()


def made(rng, piles, n, **extra):
    v = make(rng, piles, n, **extra)
    v.set_telemetry(True)
    return v


# ---- 1. kernel == definition, bit for bit
@pytest.mark.parametrize("n", [1, 67, 600])
@pytest.mark.parametrize("piles", [[3, 2], [0, 5], [5, 0], [20, 25]], ids=lambda p: "%d_%d" % tuple(p))
@pytest.mark.parametrize("rng", MODES)
def test_kernel_equals_the_definition(rng, piles, n):
    """reset, then 8 steps on chub_random_actions_device rows, two of them with the tail actions forced to +-1 (electrolyser full on: the
    grid clamp and gen_hy; electrolyser off, fuel cell full on).  At [3, 2] 600 envs keep the telemetry block in device memory, 1 and 67
    in pinned host memory (the rule is 16 KB of action rows); 67 and 600 are not multiples of the workgroup's 256 rows."""
    v = made(rng, piles, n)
    in_hbm = n * v.act_dim * 4 > 16384
    if piles == [3, 2]:
        assert in_hbm == (n == 600)
    compat = rng == "compat"
    d, out = Dev(v), Out(n)
    drv = Driver(v, rng)
    drv.reset()
    A = v.act_dim
    rs = np.random.RandomState(n)
    seen_gen, fc_on = set(), False
    for t in range(8):
        v.random_actions_device(d.act.ptr, 123, t)
        if t in (2, 5):
            act = d.act.to_host(np.float32, (n, A))
            act[:, A - 2:] = (1.0, -1.0) if t == 2 else (-1.0, 1.0)
            d.act.from_host(act)
        if compat:
            d.z.from_host(rs.normal(size=(n, 3)))
        v.step_device(d.act.ptr, d.obs.ptr, d.rew.ptr, d.done.ptr, d_exo_z=d.z.ptr if compat else 0)
        want = expected(v)
        what = (rng, piles, n, "step", t)
        got64 = v.step_terms()
        assert got64.shape == (n, NC) and got64.dtype == np.float64
        same(got64, want, what + ("the host form, f64",), bits64)
        w32 = want.astype(np.float32)
        got = out.call(v)
        assert not (got == CANARY).any(), what
        same(got.view(np.float32), w32, what + ("all fields",))
        for fields in (1 << (3 * t + 1) % NC, EVERY_THIRD):  # a single field, every third: columns in ascending field order
            same(out.call(v, fields).view(np.float32), w32[:, stl.cols_of(fields)], what + ("fields", fields))
        same(v.step_terms(EVERY_THIRD), want[:, stl.cols_of(EVERY_THIRD)], what + ("the host form, every third",), bits64)
        mask = rs.uniform(size=n) < 0.5
        d.mask.from_host(mask.astype(np.uint8))
        got = out.call(v, ALL, d_mask=d.mask.ptr)
        assert (got[~mask] == CANARY).all(), what + ("rows of unmasked envs",)
        same(got[mask].view(np.float32), w32[mask], what + ("masked rows",))
        seen_gen |= set(want[:, ST["gen_hy"]].tolist())
        fc_on |= bool((want[:, ST["fc_power"]] > 0).any())
    assert seen_gen == {0.0, 1.0}, (rng, piles, n, "gen_hy takes both values over the run")
    if piles == [20, 25] and n >= 67:
        assert fc_on, "the fuel cell ran somewhere"
    d.mask.from_host(np.zeros(n, dtype=np.uint8))
    assert (out.call(v, ALL, d_mask=d.mask.ptr) == CANARY).all()  # an all-zero mask writes nothing
    out.free()
    v.close()


# ---- 2. per-env rows
def test_per_env_rows_take_their_own_init_soc_and_capacity():
    n = 70
    rs = np.random.RandomState(4)
    init_soc, vlt = rs.uniform(0.15, 0.6, n), rs.uniform(20, 60, n)
    v = made("philox", [3, 2], n, init_soc=list(init_soc), hydro_store_vlt=list(vlt))
    assert v.has_env_params
    out = Out(n)
    drv = Driver(v, "philox")
    drv.reset()
    for t in range(3):
        drv.step()
        want = expected(v, init_soc, vlt)
        same(v.step_terms(), want, ("rows", t, "f64"), bits64)
        same(out.call(v).view(np.float32), want.astype(np.float32), ("rows", t))
        two = ("soc_deviation", "soc_penalty")
        same(out.call(v, two).view(np.float32), want[:, [25, 26]].astype(np.float32), ("rows", t, two))
        # the homogeneous constants would give other numbers for (almost) every env
        other = expected(v)
        assert (bits64(other[:, 25]) != bits64(want[:, 25])).sum() > n // 2 and (bits64(other[:, 26]) != bits64(want[:, 26])).sum() > n // 2
    out.free()
    v.close()


# ---- 3. identities
def test_identities_with_the_reward_and_the_ledger():
    n = 67
    v = made("philox", [20, 25], n)
    v.set_episode_stats(True)
    drv = Driver(v, "philox")
    drv.reset()
    for t in range(6):
        _, rew, _, _ = drv.step()
        x = v.step_terms()
        c = [x[:, f] for f in range(NC)]
        # the tail's own expression for the income (income_hys + income_evs + income_evs_serve + hy_cost), left to right
        income = (c[7] + ((c[2] + c[4]) + (c[3] + c[5]))) + c[6] + c[8]
        same(income, c[1], ("income", t), bits64)
        # ... and for the reward: that sum + hy_loss + not_meet_loss over 50, by div_c: within 1 ulp of the division
        recomposed = (income + c[9] + c[10]) / 50
        assert (np.abs(recomposed - c[0]) <= np.spacing(np.abs(c[0]))).all(), ("reward within 1 ulp", t)
        same(c[0].astype(np.float32), rew, ("(float) REWARD is the step's reward output", t))
        live = v.episode_stats(finished=False)
        same(c[25], live["deviation"], ("SOC_DEVIATION == live DEVIATION", t), bits64)
        same(c[26], live["test_penalty"], ("SOC_PENALTY == live TEST_PENALTY", t), bits64)
        if t == 0:
            same(c[11], live["draw_ele"], ("GRID_DRAW == live DRAW_ELE after an episode's first step",), bits64)
    assert (c[26] > 0).any() and (c[1] != 0).any()
    v.close()


# ---- 4. against the reference through the drop-in class
def _attrs_close(x, at, what):
    close([x[ST["income_evs0"]], x[ST["income_evs1"]], x[ST["cost_evs0"]], x[ST["cost_evs1"]], x[ST["income_serve"]], x[ST["income_hys"]],
           x[ST["hy_cost"]], x[ST["hy_gen"]], x[ST["gen_hy"]], x[ST["hy_for_fc"]], x[ST["soc_deviation"]], x[ST["cost_evs0"]] + x[ST["cost_evs1"]]],
          [at["re_income_evs_list_0"], at["re_income_evs_list_1"], at["re_income_evs_cost_list_0"], at["re_income_evs_cost_list_1"],
           at["re_income_evs_serve"], at["re_income_hys"], at["re_hy_cost"], at["re_hy_gen"], at["gen_hy"], at["re_hy_for_fc"], at["deviation"],
           at["re_income_evs_cost"]], what, rtol=TIGHT, atol=TIGHT)


@pytest.mark.parametrize("name", ["env_c1_envtest", "env_clamp", "env_fcev_queue", "env_past_done"])
def test_dropin_class_terms_match_the_reference_attributes(name):
    """EvcsspManagerEnv_v6 driven as tests/test_gpu_parity.py drives it (one COMPAT env: the telemetry block in pinned host memory, reset and
    step as one launch); after each step step_terms() of its handle against what the reference class carried after that step.
    test_penalty is assigned by the reference only where `done` fires and kept until it fires again (MGR:275-290): compared there."""
    import random
    chub = hub()
    g = orclib.load_golden(name)
    names = [str(x) for x in g["attr_names"]]
    if name == "env_c1_envtest":  # test/env_test.py: nothing injected, action=None
        random.seed(0)
        np.random.seed(0)
        env = chub.EvcsspManagerEnv_v6(station_list=[20, 25], station_type_list=["fast", "slow"], constant_charging=False, seed_rand=False,
                                       hydro_prod_rate=100, hydro_store_vlt=500 / 20, init_soc=0.2, fc_max_power=100, fcev_permeate=0.01,
                                       use_lagrange=False, renew_fluctuate=0.0, price_fluctuate=0.0, hydro_loss=0.0)
        action = lambda i: None
    else:
        random.seed(PY_SEEDS[name])
        np.random.seed(PY_SEEDS[name])
        kw = kwargs_of(g)
        if "ctor_kwargs_names" in g.files:
            given = set(str(x) for x in g["ctor_kwargs_names"])
            kw = {k: val for k, val in kw.items() if k in given}
        env = chub.EvcsspManagerEnv_v6(seed_rand=False, use_lagrange=False, compat_seeds=[int(x) for x in g["ctor_seeds"]], **kw)
        action = lambda i: g["action"][i]
    steps, i, fresh = int(g["steps_per_episode"]), 0, 0
    seeds = {int(r[0]): (int(r[1]), int(r[2])) for r in g["seeds"]} if g["seeds"].size else {}
    for ep in range(int(g["episodes"])):
        if ep in seeds:
            env.set_compat_seeds(*seeds[ep])
        env.reset()
        draw = 0.0
        for t in range(steps):
            _, r, done, _ = env.step(action(i))
            x = env._vec.step_terms()
            assert x.shape == (1, NC)
            x = x[0]
            at = dict(zip(names, g["attrs"][i]))
            what = (name, ep, t)
            _attrs_close(x, at, what)
            draw += x[ST["grid_draw"]]
            close(draw, at["cumulated_draw_ele"], what + ("cumulated_draw_ele",), rtol=TIGHT, atol=TIGHT)
            close(x[ST["reward"]], g["reward"][i], what + ("reward",), rtol=TIGHT, atol=TIGHT)
            assert x[ST["reward"]] == r
            if done and not np.isnan(at["test_penalty"]):
                close(x[ST["soc_penalty"]], at["test_penalty"], what + ("test_penalty",), rtol=TIGHT, atol=TIGHT)
                close(x[ST["soc_penalty"]], env.test_penalty, what + ("the class's own test_penalty",), rtol=0, atol=0)
                fresh += 1
            i += 1
    assert fresh == int(g["done"].sum())  # (env_fcev_queue's one episode is cut short at 45 steps: its `done` never fires)
    env.close()


# ---- 5. the attached output
@pytest.mark.parametrize("rng", ["philox", "compat"])
def test_attached_buffer_follows_every_step_form(rng):
    """lock-step, host-masked and device-masked steps: the attached rows of the envs a call served equal an explicit call made right
    after it, the other rows stay; resets write nothing; after a detach nothing is written"""
    n = 67
    v = made(rng, [3, 2], n)
    compat = rng == "compat"
    d, att, out = Dev(v), Out(n), Out(n)
    fields = ("reward", "income_evs0", "not_meet_loss", "grid_excess", "fcev_queue", "soc_deviation", "soc_penalty")
    cols = stl.cols_of(fields)
    drv = Driver(v, rng)
    drv.reset()
    assert v.step_terms_attached == 0
    att.fill()
    v.attach_step_terms(att.ptr, fields)
    assert v.step_terms_attached == _lib.st_fields_mask(fields)
    rs = np.random.RandomState(6)

    def variates():
        return (np.stack([rs.randint(0, 100, n), rs.randint(0, 150, n)], axis=1).astype(np.int32), rs.normal(size=(n, 3))) if compat else (None, None)

    for t in range(3):  # lock-step
        drv.step()
        v.sync()
        got = att.words(fields)
        same(got.view(np.float32), expected(v)[:, cols].astype(np.float32), (rng, "lock-step", t))
        assert np.array_equal(got, out.call(v, fields)), (rng, "lock-step", t, "an explicit call right after")
    for t in range(4):  # host-masked and device-masked steps: served rows only
        before = att.words(fields)
        mask = random_mask(rs, n)
        act = rs.uniform(-1, 1, size=(n, v.act_dim)).astype(np.float32)
        _, z = variates()
        if t % 2 == 0:
            v.step_envs(mask, act, z)
        else:
            d.step_dmask(mask, act, z)
        v.sync()
        got = att.words(fields)
        assert np.array_equal(got[~mask], before[~mask]), (rng, "masked", t, "rows of envs the call did not serve")
        assert np.array_equal(got, out.call(v, fields)), (rng, "masked", t)  # (the block of an env not served has not moved either)
        same(got.view(np.float32), expected(v)[:, cols].astype(np.float32), (rng, "masked", t))
        assert (got[mask] != before[mask]).any()
    before = att.words(fields)
    mask = random_mask(rs, n)
    days, z = variates()
    v.reset_envs(mask, days, z)  # a masked reset, a device-mask reset and a reset of everybody: nothing is written
    days, z = variates()
    d.reset_dmask(mask, days, z)
    v.sync()
    assert np.array_equal(att.words(fields), before), (rng, "masked resets")
    assert not np.array_equal(out.call(v, fields), before)  # (an explicit call now shows the new episodes' station columns and SOC)
    drv.reset()
    v.sync()
    assert np.array_equal(att.words(fields), before), (rng, "reset of everybody")
    drv.step()
    v.sync()
    assert not np.array_equal(att.words(fields), before)
    v.detach_step_terms()
    assert v.step_terms_attached == 0
    att.fill()
    drv.step()
    v.sync()
    assert (att.words(fields) == CANARY).all(), (rng, "after a detach")
    att.free()
    out.free()
    v.close()


def staggered_twins(n, seed=21):
    """twin PHILOX handles of n envs x [3, 2] on one seed: 94 lock-step steps, then a masked reset of the odd envs"""
    chub = hub()
    rs = np.random.RandomState(2)
    acts = [rs.uniform(-1, 1, size=(n, 7)).astype(np.float32) for _ in range(94)]
    odd = np.arange(n) % 2 == 1
    out = []
    for _ in range(2):
        v = chub.VecChargingHub(n, seed=seed, rng="philox", station_list=[3, 2], **BASE)
        v.set_telemetry(True)
        v.reset()
        for a in acts:
            v.step(a)
        v.reset_envs(odd)
        out.append(v)
    return out[0], out[1], odd


def test_autoreset_leaves_the_terminal_terms():
    """A: chub_autoreset_step_device with the buffer attached.  B: chub_step_device_packed, the terms, then the device-mask reset of that
    step's done.  A's rows equal B's in every call -- in the call where the even envs' done fires their SOC_* and INCOME_EVS* are the
    terminal step's, which an explicit call after A's call (the reset has rewritten those telemetry columns) no longer shows."""
    n = 64
    va, vb, odd = staggered_twins(n)
    da, db, att, out = Dev(va), Dev(vb), Out(n), Out(n)
    D = va.obs_dim
    att.fill()
    va.attach_step_terms(att.ptr)
    rs = np.random.RandomState(5)
    fired = []
    for k in range(4):
        act = rs.uniform(-1, 1, size=(n, va.act_dim)).astype(np.float32)
        packed, _ = da.autoreset(act)
        va.sync()
        got = att.words()
        db.act.from_host(act)
        vb.step_device_packed(db.act.ptr, db.packed.ptr)
        want = vb.step_terms().astype(np.float32)
        same(want, expected(vb).astype(np.float32), ("B's terms are the definition", k))
        done = db.packed.to_host(np.float32, (n, D + 2))[:, D + 1] > 0.5
        db.reset_dmask(done)
        same(got.view(np.float32), want, ("call", k))
        assert np.array_equal(done, packed[:, D + 1] > 0.5)
        fired.append(done.copy())
        if done.any():
            after = out.call(va).view(np.float32)  # the block as it stands once A's call is over
            assert (after[done][:, ST["soc_deviation"]] == 0).all() and (got.view(np.float32)[done][:, ST["soc_deviation"]] > 0).any()
            same(after[~done], got.view(np.float32)[~done], ("envs that were not restarted", k))
    assert [bool(f.any()) for f in fired] == [False, True, False, False] and np.array_equal(fired[1], ~odd)
    for b in (att, out):
        b.free()
    va.close()
    vb.close()


def test_graph_of_autoreset_calls_fills_the_attached_buffer():
    """two auto-reset calls captured on per-env clocks with the buffer attached (each: step, terms, reset -- the terms launch is one more
    node and does not count towards the even number of resets + steps), replayed twice: the buffer equals the twin's after the same four
    calls issued one by one.  Attaching and detaching inside the capture are refused and leave it unharmed."""
    chub = hub()
    mg = buffers()
    n = 64
    vg, ve, odd = staggered_twins(n, seed=22)
    st = mg.Stream(0)
    dg, de, attg, atte = Dev(vg, st.ptr), Dev(ve), Out(n), Out(n)
    attg.fill()
    atte.fill()
    vg.attach_step_terms(attg.ptr)
    ve.attach_step_terms(atte.ptr)
    act = np.random.RandomState(9).uniform(-1, 1, size=(n, vg.act_dim)).astype(np.float32)
    dg.act.from_host(act, st.ptr)
    st.sync()
    vg.graph_begin(st.ptr)
    for call in (vg.detach_step_terms, lambda: vg.attach_step_terms(atte.ptr)):
        with pytest.raises(chub.ChubError, match="libchub error -4"):
            call()
    for k in range(2):
        vg.step_autoreset_device(dg.act.ptr, dg.packed.ptr, dg.final.ptr, stream=st.ptr)
    graph = vg.graph_end(st.ptr)
    assert (attg.words() == CANARY).all()  # a capture runs nothing
    for r in range(2):
        vg.graph_launch(graph, st.ptr)
        st.sync()
        for k in range(2):
            pe, _ = de.autoreset(act)
        ve.sync()
        assert np.array_equal(attg.words(), atte.words()), ("replay", r)
        assert np.array_equal(dg.packed.to_host(np.float32, (n, vg.obs_dim + 2), st.ptr), pe), ("replay", r)
    same(atte.words().view(np.float32)[odd], expected(ve).astype(np.float32)[odd], "the odd envs were not restarted in the last call")
    (tg, ticks_g), (te, ticks_e) = vg.env_clocks(ticks=True), ve.env_clocks(ticks=True)
    assert np.array_equal(tg, te) and np.array_equal(ticks_g, ticks_e)  # two ticks per auto-reset call: the terms launch takes none
    assert ticks_g.max() <= 1 + 94 + 1 + 2 * 4
    vg.graph_destroy(graph)
    for b in (attg, atte):
        b.free()
    vg.close()
    ve.close()
    st.destroy()


def test_refusals():
    chub = hub()
    v = make("philox", [3, 2], 8)
    out = Out(8)
    v.reset()
    for call in (lambda: v.attach_step_terms(out.ptr), lambda: v.step_terms_device(out.ptr), v.step_terms):
        with pytest.raises(chub.ChubError, match="libchub error -1: telemetry is off"):
            call()
    v.set_telemetry(True)
    for bad in (0, 1 << 27):
        assert v._lib.chub_get_step_terms_device(v._h, bad, None, out.ptr, None) == -1
        assert v._lib.chub_set_step_terms(v._h, 1 << 27, out.ptr) == -1
    assert v._lib.chub_get_step_terms_device(v._h, 1, None, None, None) == -1 and v._lib.chub_get_step_terms(v._h, 1, None) == -1
    v.attach_step_terms(out.ptr, ("reward",))
    with pytest.raises(chub.ChubError, match="libchub error -1: .*detach first"):
        v.set_telemetry(False)
    v.set_telemetry(True)  # (switching it on again is no offence)
    assert v.step_terms_attached == 1
    v.detach_step_terms()
    v.set_telemetry(False)
    with pytest.raises(chub.ChubError, match="telemetry is off"):
        v.step_terms()
    out.free()
    v.close()


# ---- 6. the torch adapter
TORCH_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["CHUB_ROOT"])
sys.path.insert(0, os.path.join(os.environ["CHUB_ROOT"], "tests"))
import torch  # before libchub: both must share one HIP runtime
torch.cuda.set_device(0)
import test_gpu_step_terms
test_gpu_step_terms.torch_adapter_step_terms()
print("TORCH_STEP_TERMS_OK")
"""


def test_torch_adapter():
    """in a child process that imports torch first (as tests/test_gpu_torch_side.py does; nothing of torch is touched in this one)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD], env=dict(os.environ, CHUB_ROOT=root), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "TORCH_STEP_TERMS_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def torch_adapter_step_terms():
    import inspect

    import torch
    from charginghub_env_amd import wrappers
    n = 64
    kw = {k: BASE[k] for k in BASE if k != "station_type_list"}
    asked = ("soc_penalty", "reward", "grid_excess", "not_meet_loss")
    names = ("reward", "not_meet_loss", "grid_excess", "soc_penalty")
    for autoreset, control in ((True, "pile"), ("per_env", "pile"), ("per_env", "station"), (False, "pile")):
        env = wrappers.TorchHubVecEnv(n, [3, 2], ["fast", "slow"], seed=13, autoreset=autoreset, control=control, step_terms=asked, **kw)
        assert env.terms_names == names
        env.reset()
        p = env.step_terms()
        assert tuple(p.shape) == (n, 4) and p.dtype == torch.float32 and p.is_cuda and not p.any()  # zeros before the first step
        g = torch.Generator(device="cuda").manual_seed(1)
        dones = 0
        for t in range(100 if autoreset else 20):
            obs, reward, done, _ = env.step(torch.rand((n, env.act_dim), device="cuda", generator=g) * 2 - 1)
            q = env.step_terms()
            assert q.data_ptr() == p.data_ptr()  # one buffer the adapter owns
            assert torch.equal(q[:, 0].view(torch.int32), reward.contiguous().view(torch.int32)), (autoreset, control, "reward column", t)
            if bool(done.any()):  # the step re-started these envs: their rows are the terminal step's
                dones += 1
                assert t == 95 and bool(done.all())
                assert bool((q[:, 3] > 0).any()), "the end-of-day penalty of the finished episodes"
                now = torch.from_numpy(env.vec.step_terms(names)).to(torch.float32)  # the block as it stands: the new episodes' SOC
                assert bool((now[:, 3] == 0).all()) and torch.equal(now[:, 0], q[:, 0].cpu())
            elif t % 10 == 9:
                same(q.cpu().numpy(), env.vec.step_terms(names).astype(np.float32), (autoreset, control, "step", t))
        assert dones == (1 if autoreset else 0)
        env.close()
    src = inspect.getsource(wrappers.TorchHubVecEnv.step_terms)  # it launches nothing: the step already filled the buffer
    assert "self.vec" not in src.split('"""')[-1] and "sync" not in src.split('"""')[-1]
    off = wrappers.TorchHubVecEnv(8, [3, 2], ["fast", "slow"], seed=1, **kw)
    assert off.terms_names == ()
    with pytest.raises(RuntimeError):
        off.step_terms()
    off.close()
