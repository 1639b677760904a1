"""k_policy_grad and k_critic past a workgroup's first tile of rows.  At most 512 workgroups walk the tiles b, b + 512, ..; every other test
stays below 16 tiles, so that no workgroup ever took a second trip.  Here R2 = 16455 (workgroups 0 .. 2 walk two tiles, the rest one) and
R3 = 32871 (workgroups 0 .. 3 walk three, the rest two; the values call's 1024 workgroups one or two), both with a last tile of 7 rows
(tests/grid_pass_lib.py; tests/test_grad_trips_cpu.py holds the arithmetic and the conditions on every case's data):
(1) exact data, bit for bit -- what a workgroup carries from tile to tile (dW tiles in registers or in its partials, bias sums, f64 stats,
log_std sums) with no tolerance; (2) general nets within the derived bar with tpw = 2 and 3, determinism, the forward alone, the values
call, and nothing written past R; (3) one call equals the calls on its first, second and third trips' rows."""
import numpy as np
import pytest

import critic_lib as cl
import grid_pass_lib as gpl
import policy_grad_lib as pgl
import test_gpu_critic as tc
import test_gpu_policy_grad as tp
from test_gpu_policy_sample import close_all

pytestmark = pytest.mark.gpu
F32 = np.float32
TAIL = 32                      # positions every per-row output buffer holds past R
NAN_BITS = np.uint32(0x7FC00000)  # the pattern the buffers hold before a call
EXACT_NETS = [(1, cl.EXACT_HIDDEN), (2, cl.EXACT_HIDDEN), (3, cl.EXACT_HIDDEN), (4, cl.EXACT_HIDDEN), (3, cl.EXACT_WIDE)]
EXACT_IDS = ["1", "2", "3", "4", "3-tiles_in_the_partials"]


def untouched(a):
    return bool((np.ascontiguousarray(a, dtype=F32).view(np.uint32) == NAN_BITS).all())


def bits_equal(a, b):
    return np.array_equal(tc.bits(a), tc.bits(b))


# ---- 1. exact data: no tolerance at all
@pytest.mark.parametrize("R", cl.TRIP_R)
@pytest.mark.parametrize("n_layers,hidden", EXACT_NETS, ids=EXACT_IDS)
def test_critic_exact_bit_for_bit(n_layers, hidden, R):
    """gW, gb, the values of both calls and all six stats equal the f64 restatement's rounding when workgroups walk two and three tiles"""
    c0 = cl.exact_case(n_layers, R, hidden=hidden)
    p = cl.plan(c0.F, c0.sizes[1:], R, "relu")[1]
    assert p["workgroups"] == 512 and (p["in_registers"] == 0) == (hidden == cl.EXACT_WIDE)
    v, cr = tc.critic_of(c0, R)
    for loss in ("mse", "clipped"):
        c = c0 if loss == "mse" else cl.exact_case(n_layers, R, loss, hidden=hidden)
        got = tc.call(cr, c, tail=TAIL)
        gW, gb, val, stats = cl.exact_expected(c)
        for l in range(n_layers):
            assert np.array_equal(got["grads"][l][0], gW[l]), (R, loss, "gW", l, np.abs(got["grads"][l][0] - gW[l]).max(), int((got["grads"][l][0] != gW[l]).sum()))
            assert np.array_equal(got["grads"][l][1], gb[l]), (R, loss, "gb", l, np.abs(got["grads"][l][1] - gb[l]).max())
        bad = np.flatnonzero(got["values"] != val)
        assert not len(bad), (R, loss, "values of the gradient call", len(bad), bad[:8])
        bad = np.flatnonzero(got["values2"] != val)
        assert not len(bad), (R, loss, "values of the values call", len(bad), bad[:8])
        assert np.array_equal(got["stats"], stats), (R, loss, got["stats"], stats)
        assert untouched(got["past"]), (R, loss, "written past R")
        if loss == "clipped":
            assert 0 < got["stats"][2] < R
    close_all(cr, v)


def actor_call(g, c, backward=True):
    """one call through device buffers of its own, a NaN pattern over every output before it"""
    d = tp.DevCase(c, tail=TAIL)
    d.run(g, backward=backward)
    g._env.sync()
    got = d.result()
    d.free()
    return got


@pytest.mark.parametrize("R", pgl.TRIP_R)
@pytest.mark.parametrize("n_layers,hidden", EXACT_NETS, ids=EXACT_IDS)
def test_actor_exact_bit_for_bit(n_layers, hidden, R):
    """LOADS, relu, COEF: gW, gb, g_log_std, logp_new, entropy and the stats.  Over all R3 rows the deeper nets' sums of absolute values
    pass 2^23 quanta; over a workgroup's own three tiles, which is all an f32 chain covers, they stay below 2^16 (exact_case asserts it)"""
    c = pgl.exact_case(n_layers, R, hidden=hidden, blocks=512)
    v, pol, g = tp.actor(c, R)
    p = g.plan(R)
    assert p["workgroups"] == 512 and (p["in_registers"] == 0) == (hidden == pgl.EXACT_WIDE)
    got = actor_call(g, c)
    r = pgl.restate(c)
    gW, gb, gls = pgl.exact_expected(c, r)
    lp, en, stats = pgl.exact_forward(c, r)
    for l in range(n_layers):
        assert np.array_equal(got["grads"][l][0], gW[l]), (R, "gW", l, np.abs(got["grads"][l][0] - gW[l]).max(), int((got["grads"][l][0] != gW[l]).sum()))
        assert np.array_equal(got["grads"][l][1], gb[l]), (R, "gb", l, np.abs(got["grads"][l][1] - gb[l]).max())
    assert np.array_equal(got["g_log_std"], gls), (R, got["g_log_std"], gls)
    for name, want in (("logp_new", lp), ("entropy", en)):
        bad = np.flatnonzero(got[name] != want)
        assert not len(bad), (R, name, len(bad), bad[:8], got[name][bad[:4]], want[bad[:4]])
    assert np.array_equal(got["stats"], stats), (R, got["stats"], stats)
    assert untouched(got["past"]), (R, "written past R")
    close_all(g, pol, v)


# ---- 2. general nets within the derived bar, tpw from the plan
CRITIC_CASES = cl.trip_general_cases()
ACTOR_CASES = pgl.trip_general_cases()


@pytest.mark.parametrize("c,tpw", CRITIC_CASES, ids=[c.name for c, _ in CRITIC_CASES])
def test_critic_within_the_bar(c, tpw):
    r = cl.restate(c, tpw)
    cl.check_conditions(c, r)
    v, cr = tc.critic_of(c, c.R)
    assert cr.plan(c.R)["workgroups"] == 512 and tpw == gpl.grad_trips(c.R, 512).max() >= 2
    got = tc.call(cr, c, tail=TAIL)
    tc.within(got, r, c.name)
    assert bits_equal(got["values"], got["values2"]), "chub_critic_values_device forms the gradient call's bits"
    fwd = tc.call(cr, c, backward=False, tail=TAIL)
    assert bits_equal(fwd["values"], got["values"]) and bits_equal(fwd["values2"], got["values"]) and bits_equal(fwd["stats"], got["stats"])
    assert all(untouched(gW) and untouched(gb) for gW, gb in fwd["grads"]), "no gradient output was asked for"
    again = tc.call(cr, c, tail=TAIL)
    assert tc.same_bits(again, got) and bits_equal(again["values2"], got["values2"])
    assert untouched(got["past"]) and untouched(fwd["past"]) and untouched(again["past"]), "written past R"
    close_all(cr, v)


@pytest.mark.parametrize("c,tpw", ACTOR_CASES, ids=[c.name for c, _ in ACTOR_CASES])
def test_actor_within_the_bar(c, tpw):
    r = pgl.restate(c, tpw)
    pgl.check_conditions(c, r)
    v, pol, g = tp.actor(c, c.R)
    blocks = g.plan(c.R)["workgroups"]
    assert blocks == pgl.blocks_of(c) and tpw == gpl.grad_trips(c.R, blocks).max() >= 2
    got = actor_call(g, c)
    tp.within(got, r, c.name)
    fwd = actor_call(g, c, backward=False)
    assert all(bits_equal(fwd[k], got[k]) for k in ("logp_new", "entropy", "stats"))
    assert all(untouched(gW) and untouched(gb) for gW, gb in fwd["grads"]) and untouched(fwd["g_log_std"]), "no gradient output was asked for"
    again = actor_call(g, c)
    assert all(bits_equal(a, b) and bits_equal(a2, b2) for (a, a2), (b, b2) in zip(again["grads"], got["grads"]))
    assert all(bits_equal(again[k], got[k]) for k in ("g_log_std", "logp_new", "entropy", "stats"))
    assert untouched(got["past"]) and untouched(fwd["past"]) and untouched(again["past"]), "written past R"
    close_all(g, pol, v)


# ---- 3. one call equals its parts
def adds_up(c, full, r, parts, what):
    """parts [(R, got, restatement)]: the sum of R_part * gradient equals R * the whole call's gradient within the bars added"""
    bad = []
    for l in range(len(c.layers)):
        for k, name in ((0, "bar_W"), (1, "bar_b")):
            total = sum(R * got["grads"][l][k].astype(np.float64) for R, got, _ in parts)
            bar = sum(R * rp[name][l] for R, _, rp in parts) + c.R * r[name][l]
            d = np.abs(total - c.R * full["grads"][l][k].astype(np.float64))
            print(what, "layer", l, name, "largest difference %.3e, bar there %.3e" % (d.max(), bar.ravel()[d.argmax()]))
            if not (d <= bar).all():
                bad.append((l, name, d.max(), bar.ravel()[d.argmax()]))
    assert not bad, (what, bad)


@pytest.mark.parametrize("loss", ["mse", "clipped"])
def test_critic_one_call_equals_its_trips(loss):
    """d_rows lists that hold the rows of R3's first, second and third trips (16384, 16384 and 103 rows): three calls of one trip each,
    weighted by their R, add up to the one call of three trips; each within its own bar.  A failure here names the trip"""
    c, tpw = [(c, t) for c, t in CRITIC_CASES if c.name == "13-64x64-tanh-%s-%d" % (loss, gpl.GRAD_R3)][0]
    v, cr = tc.critic_of(c, c.R)
    full, r = tc.call(cr, c), cl.restate(c, tpw)
    tc.within(full, r, c.name)
    parts = []
    for cm in cl.trip_parts(c, 512):
        tm = cl.tiles_per_workgroup(cm)
        assert tm == 1
        rm, gm = cl.restate(cm, tm), tc.call(cr, cm)
        tc.within(gm, rm, cm.name)
        parts.append((cm.R, gm, rm))
    assert [R for R, _, _ in parts] == [16384, 16384, 103]
    adds_up(c, full, r, parts, c.name)
    close_all(cr, v)


@pytest.mark.parametrize("loss", ["coef", "ppo_clip"])
def test_actor_one_call_equals_its_trips(loss):
    c, tpw = pgl.trip_parts_case(loss)
    v, pol, g = tp.actor(c, c.R)
    full, r = actor_call(g, c), pgl.restate(c, tpw)
    tp.within(full, r, c.name)
    parts = []
    for cm in pgl.trip_parts(c, 512):
        assert tp.tpw_of(cm) == 1
        rm, gm = pgl.restate(cm, 1), actor_call(g, cm)
        tp.within(gm, rm, cm.name)
        parts.append((cm.R, gm, rm))
    assert [R for R, _, _ in parts] == [16384, 16384, 103]
    adds_up(c, full, r, parts, c.name)
    d = np.abs(sum(R * gm["g_log_std"].astype(np.float64) for R, gm, _ in parts) - c.R * full["g_log_std"].astype(np.float64))
    assert (d <= sum(R * rm["bar_ls"] for R, _, rm in parts) + c.R * r["bar_ls"]).all(), ("g_log_std", d)
    close_all(g, pol, v)
