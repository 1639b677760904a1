"""Pile sets and advantages (include/chub.h: chub_pile_set_device, chub_policy_sample_set_device, chub_policy_collect_set,
chub_rollout_gae_device) without a device: the new entry points declared, exported and bound; tests/pile_set_lib.py's f32 GAE against the
f64 textbook sum within the derived bound; the set definitions against the CPU oracle (its step ignores every action bit outside
DECIDABLE); the torch helpers sampled_logp / sampled_entropy against numpy; the refusals that need no device."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import orclib
import pile_set_lib as psl
import policy_sample_lib as ps
from orclib import orc, ptr
from charginghub_env_amd import _lib, vec_env, wrappers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
BASE = dict(hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2, fc_max_power=100.0, fcev_permeate=0.01)


def test_symbols_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chub.h")).read(), flags=re.S)
    assert re.search(r"enum \{ CHUB_PSET_ALL = 0, CHUB_PSET_OCCUPIED, CHUB_PSET_DECIDABLE, CHUB_PSET_COUNT \};", header)
    assert _lib.PSET_NAMES == psl.PSET_NAMES and [_lib.PSET[n] for n in _lib.PSET_NAMES] == [0, 1, 2]
    lib = _lib.load_library()
    for name, n_args in (("chub_pile_set_device", 5), ("chub_policy_sample_set_device", 9), ("chub_policy_collect_set", 9),
                         ("chub_rollout_gae_device", 3)):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args
    gae = header[header.index("typedef struct chub_gae {"):header.index("} chub_gae;")]
    fields = re.findall(r"(\w+)(?:,\s*\*?(\w+))?;", gae)
    names = [n for pair in fields for n in pair if n]
    assert names == ["T", "d_packed", "d_values", "d_final_values", "d_mask", "gamma", "lambda", "d_adv", "d_ret", "d_stats"]
    assert [n for n, _ in _lib.ChubGae._fields_] == [n if n != "lambda" else "lam" for n in names]
    assert C.sizeof(_lib.ChubGae) == 8 * 5 + 8 + 8 * 3
    for method in ("pile_set_device", "pile_set", "gae_device"):
        assert callable(getattr(vec_env.VecChargingHub, method))
    for fn in (vec_env.DevicePolicy.sample_device, vec_env.DevicePolicy.collect):
        p = inspect.signature(fn).parameters
        assert p["logp_piles"].default is None and p["d_set_bits"].default == 0
    assert inspect.signature(wrappers.TorchHubVecEnv.collect).parameters["logp_piles"].default is None
    p = inspect.signature(wrappers.TorchHubVecEnv.advantages).parameters
    assert (p["gamma"].default, p["lam"].default, p["stats"].default, p["final_values"].default) == (0.99, 0.95, False, None)
    assert _lib.pile_set("decidable") == 2 and _lib.pile_set(1) == 1
    with pytest.raises(ValueError, match="unknown pile set"):
        _lib.pile_set("empty")


def test_bad_arguments_are_refused_without_a_device():
    lib = _lib.load_library()
    f = C.c_void_p(8)  # never dereferenced: the checks come first
    msg = lambda: lib.chub_last_error().decode()
    assert lib.chub_pile_set_device(None, 0, None, f, None) == -1 and msg() == "null argument"
    assert lib.chub_pile_set_device(f, 0, None, None, None) == -1 and msg() == "null argument"
    out = _lib.ChubPolicySampleOut()
    assert lib.chub_policy_sample_set_device(None, f, f, 13, None, 0, None, C.byref(out), None) == -1 and msg() == "null argument"
    roll = _lib.ChubRollout()
    assert lib.chub_policy_collect_set(f, f, 0, 3, C.byref(roll), f, f, 0, None) == -1 and "CHUB_PSET" in msg()
    assert lib.chub_policy_collect_set(f, f, 0, -1, C.byref(roll), f, f, 0, None) == -1 and "CHUB_PSET" in msg()
    assert lib.chub_policy_collect_set(None, f, 0, 2, C.byref(roll), f, f, 0, None) == -1 and msg() == "null argument"
    good = dict(T=4, d_packed=8, d_values=8, d_final_values=None, d_mask=None, gamma=0.99, lam=0.95, d_adv=8, d_ret=None, d_stats=None)
    gae = lambda **kw: C.byref(_lib.ChubGae(**dict(good, **kw)))
    assert lib.chub_rollout_gae_device(None, gae(), None) == -1 and msg() == "null argument"
    assert lib.chub_rollout_gae_device(f, None, None) == -1 and msg() == "null argument"
    for missing in ("d_packed", "d_values", "d_adv"):
        assert lib.chub_rollout_gae_device(f, gae(**{missing: None}), None) == -1 and "are required" in msg()
    for T in (0, -3):
        assert lib.chub_rollout_gae_device(f, gae(T=T), None) == -1 and "T >= 1" in msg()
    for bad in (dict(gamma=-0.01), dict(gamma=1.01), dict(gamma=float("nan")), dict(lam=-0.5), dict(lam=1.5), dict(lam=float("nan"))):
        assert lib.chub_rollout_gae_device(f, gae(**bad), None) == -1 and "[0, 1]" in msg(), bad


# ---- the f32 GAE against the f64 textbook sum
@pytest.mark.parametrize("T", psl.GAE_T)
@pytest.mark.parametrize("dones", psl.GAE_DONES)
@pytest.mark.parametrize("with_final", [False, True])
def test_f32_gae_within_the_bound_of_the_textbook_sum(T, dones, with_final):
    packed, values, final = psl.gae_case(T, dones, with_final)
    D = packed.shape[2] - 2
    r, d = packed[:, :, D], packed[:, :, D + 1]
    if dones != "nowhere":
        assert (d != 0).any() and not (d != 0).all()
    for gamma, lam in psl.GAE_FACTORS:
        a32, r32 = psl.gae_f32(r, d, values, final, gamma, lam)
        a64, r64 = psl.gae_f64(r, d, values, final, gamma, lam)
        ba, br = psl.gae_bound(r, d, values, final, gamma, lam, a32, r32)
        ea, er = np.abs(a32.astype(np.float64) - a64), np.abs(r32.astype(np.float64) - r64)
        print("T %d %s final %s gamma %g lam %g: adv error %.3g of bound %.3g (|adv| up to %.3g)" % (T, dones, with_final, gamma, lam, ea.max(), ba.max(), np.abs(a64).max()))
        assert (ea <= ba).all() and (er <= br).all(), (gamma, lam, (ea / ba).max(), (er / br).max())
        assert (ba <= 1e-3 * (1 + np.abs(a64).max())).all(), "the bound says something"
        fired = d != 0
        if gamma == 0.0:  # nothing but the step's own reward and value
            assert np.array_equal(a32, (r - values[:-1]).astype(F32) + F32(0))
        if fired.any() and final is None and gamma == 1.0:  # an episode's end is worth 0: delta = r - V there, and the chain is cut
            assert np.array_equal(a32[fired], (r[fired] - values[:-1][fired]).astype(F32))


def test_gae_bootstraps_through_the_final_values_only_where_done_fires():
    packed, values, final = psl.gae_case(5, "last", True)
    D = packed.shape[2] - 2
    r, d = packed[:, :, D], packed[:, :, D + 1]
    a, _ = psl.gae_f32(r, d, values, final, 0.99, 0.95)
    other = final + F32(1)
    b, _ = psl.gae_f32(r, d, values, other, 0.99, 0.95)
    fired = d[4] != 0
    assert np.array_equal(a[:, ~fired], b[:, ~fired]) and (a[:, fired] != b[:, fired]).all()
    moved = values.copy()
    moved[5, fired] += F32(7)  # V of the NEXT episode's first observation: not read where done fires
    c, _ = psl.gae_f32(r, d, moved, final, 0.99, 0.95)
    assert np.array_equal(a, c)


# ---- the sets against the oracle: its step ignores every action bit outside DECIDABLE
def oracle_vec(piles, n, seed):
    cfg = orclib.make_config(piles=piles, types=("fast", "slow"), **BASE)
    return cfg, orc.orc_vec_create(C.byref(cfg), orclib.tables(), n, 0, orclib.PHILOX, seed)


def oracle_columns(h, piles, n):
    out = []
    for k, nk in enumerate(piles):
        w = np.zeros((n, 9, nk), dtype=F32)
        orc.orc_vec_slots(h, k, ptr(w))
        out.append(w)
    return np.concatenate(out, axis=2)


@pytest.mark.parametrize("piles", psl.HUBS, ids=lambda p: "%dx%d" % tuple(p))
def test_the_oracles_step_ignores_the_complement_of_decidable(piles):
    """two oracles on the same seeds, 66 steps into a day (forced-on cars exist), then 8 steps with bits B and with B XOR (random bits outside
    DECIDABLE), the set recomputed from the car / emergency columns each step: observations, rewards and all nine pile columns stay
    identical, bit for bit.  A flip INSIDE the set does change the state: the sets are not vacuous."""
    n, S = 12, sum(piles)
    D = 2 + 4 * sum(1 for p in piles if p > 0) + 3
    (_, a), (_, b), (_, c) = (oracle_vec(piles, n, 0xFEED5) for _ in range(3))
    obs = [np.zeros((n, D)) for _ in range(3)]
    rew, done = [np.zeros(n) for _ in range(3)], [np.zeros(n, dtype=np.uint8) for _ in range(3)]
    rs = np.random.RandomState(17)
    for h, o in zip((a, b, c), obs):
        orc.orc_vec_reset(h, None, None, ptr(o))
    seen = {k: np.zeros((0, S), dtype=bool) for k in psl.PSET_NAMES}

    def step(acts):
        for h, act, o, r, dn in zip((a, b, c), acts, obs, rew, done):
            orc.orc_vec_step(h, ptr(np.ascontiguousarray(act)), None, ptr(o), ptr(r), ptr(dn), 4)

    for t in range(66):
        act = rs.uniform(-1, 1, size=(n, S + 2)).astype(F32)
        if t == 0:
            cols = oracle_columns(a, piles, n)
            for k, v in psl.sets_from_columns(cols[:, 0], cols[:, 2]).items():
                seen[k] = np.concatenate([seen[k], v])
        step((act, act, act))
    parted = False
    for t in range(8):
        cols = oracle_columns(a, piles, n)
        sets = psl.sets_from_columns(cols[:, 0], cols[:, 2])
        for k, v in sets.items():
            seen[k] = np.concatenate([seen[k], v])
        act = np.where(rs.rand(n, S + 2) < 0.5, F32(1), F32(-1)).astype(F32)
        act[:, S:] = rs.uniform(-1, 1, size=(n, 2))
        other = act.copy()
        flip = (rs.rand(n, S) < 0.5) & ~sets["decidable"]
        other[:, :S][flip] *= -1
        inside = act.copy()
        inside[:, :S][sets["decidable"]] *= -1
        step((act, other, inside if not parted else act))
        assert np.array_equal(obs[0], obs[1]) and np.array_equal(rew[0], rew[1]), ("outputs", t)
        assert np.array_equal(oracle_columns(a, piles, n).view(np.uint32), oracle_columns(b, piles, n).view(np.uint32)), ("pile columns", t)
        if not parted and sets["decidable"].any():
            parted = True
            assert not np.array_equal(oracle_columns(a, piles, n), oracle_columns(c, piles, n)), "a flip inside the set changes the state"
    assert parted
    psl.sets_differ(seen, need_forced_on=True)
    assert np.array_equal(psl.words(seen["all"])[:, -1], np.full(len(seen["all"]), (1 << ((S - 1) % 64 + 1)) - 1, dtype=np.uint64))
    for h in (a, b, c):
        orc.orc_vec_destroy(h)


def test_words_are_step_bits_layout():
    import policy_lib as pl
    rs = np.random.RandomState(2)
    for S in (1, 5, 63, 64, 65, 70, 128):
        on = rs.rand(9, S) < 0.5
        w = psl.words(on)
        assert w.shape == (9, (S + 63) // 64) and w.dtype == np.uint64
        assert np.array_equal(pl.unpack_bits(w, S), on)
        assert np.array_equal(w, pl.pile_bits(np.where(on, F32(1), F32(-1)), S))


# ---- the torch helpers
def old_sampled_logp(z, bits_or_on, u, log_std):
    """wrappers.sampled_logp as it stood before it took `piles`"""
    import torch
    G = log_std.shape[-1]
    S = z.shape[-1] - G
    on = bits_or_on
    if on.dtype != torch.bool:
        sh = torch.arange(64, device=on.device, dtype=torch.int64)
        on = (((on.unsqueeze(-1) >> sh) & 1) != 0).flatten(-2)[..., :S]
    zp, zg = z[..., :S], z[..., S:]
    piles = -torch.nn.functional.softplus(torch.where(on, -zp, zp)).sum(dim=-1)
    eps = (u - zg) / torch.exp(log_std)
    return piles + (-0.5 * eps * eps - log_std - 0.5 * math.log(2.0 * math.pi)).sum(dim=-1)


@pytest.mark.parametrize("S", [5, 45, 70])
def test_sampled_logp_and_entropy_against_numpy(S):
    torch = pytest.importorskip("torch")
    rs = np.random.RandomState(S)
    T, n, G = 3, 7, 2
    z = (rs.normal(size=(T, n, S + G)) * 2).astype(F32)
    on, in_set = rs.rand(T, n, S) < 0.5, rs.rand(T, n, S) < 0.4
    u = rs.normal(size=(T, n, G)).astype(F32)
    ls = np.array([-0.5, 0.2], dtype=F32)
    flat = lambda x: x.reshape(T * n, -1)
    as_words = lambda m: torch.from_numpy(psl.words(flat(m)).view(np.int64).reshape(T, n, -1))
    zt, ut, lt = torch.from_numpy(z), torch.from_numpy(u), torch.from_numpy(ls)
    for bits in (torch.from_numpy(on), as_words(on)):
        new, old = wrappers.sampled_logp(zt, bits, ut, lt), old_sampled_logp(zt, bits, ut, lt)
        assert torch.equal(new, old) and torch.equal(new, wrappers.sampled_logp(zt, bits, ut, lt, piles=None)), "piles=None keeps the result exactly"
        for piles in (torch.from_numpy(in_set), as_words(in_set)):
            got = wrappers.sampled_logp(zt, bits, ut, lt, piles=piles).numpy().reshape(T * n)
            want = psl.sampled_logp(flat(z), flat(on), flat(u), ls, flat(in_set))
            assert np.abs(got - want).max() <= 64 * (S + G) * ps.ULP * (1 + np.abs(want).max())
    full = wrappers.sampled_logp(zt, torch.from_numpy(on), ut, lt, piles=torch.ones(T, n, S, dtype=torch.bool))
    assert torch.equal(full, wrappers.sampled_logp(zt, torch.from_numpy(on), ut, lt))
    for piles, m in ((None, None), (torch.from_numpy(in_set), flat(in_set)), (as_words(in_set), flat(in_set))):
        got = wrappers.sampled_entropy(zt, lt, piles=piles).numpy().reshape(T * n)
        want = psl.sampled_entropy(flat(z), ls, m)
        assert np.abs(got - want).max() <= 64 * (S + G) * ps.ULP * (1 + np.abs(want).max())
    # the entropy is minus the mean log-probability: at logit 0 a pile contributes ln 2, a left-out pile nothing
    z0 = torch.zeros(1, S + G)
    some = torch.zeros(1, S, dtype=torch.bool)
    some[0, :3] = True
    h = wrappers.sampled_entropy(z0, lt, piles=some)
    assert abs(float(h) - (3 * math.log(2.0) + float((0.5 + ls + ps.HALF_LN_2PI).sum()))) < 1e-5
    # differentiable in z and log_std; no gradient reaches a left-out logit
    zg, lg = zt.clone().requires_grad_(True), lt.clone().requires_grad_(True)
    (wrappers.sampled_logp(zg, torch.from_numpy(on), ut, lg, piles=torch.from_numpy(in_set)).sum() + wrappers.sampled_entropy(zg, lg, piles=torch.from_numpy(in_set)).sum()).backward()
    assert bool((zg.grad[..., :S][~torch.from_numpy(in_set)] == 0).all()) and bool((zg.grad[..., :S][torch.from_numpy(in_set)] != 0).any())
    assert bool(torch.isfinite(lg.grad).all()) and bool((lg.grad != 0).all())


class StubVec(object):
    """what TorchHubVecEnv.advantages touches of a VecChargingHub"""

    def __init__(self):
        self.calls = []

    def gae_device(self, n_steps, d_packed, d_values, d_adv, d_ret=0, d_final_values=0, gamma=0.99, lam=0.95, d_mask=0, d_stats=0, stream=0):
        self.calls.append((n_steps, d_packed, d_values, d_adv, d_ret, d_final_values, gamma, lam, d_mask, d_stats, stream))


def test_torch_adapter_advantages_checks_its_arguments_and_passes_them_on():
    torch = pytest.importorskip("torch")
    env = object.__new__(wrappers.TorchHubVecEnv)  # (the constructor creates a handle on a device)
    env.torch, env.device, env.vec, env.num_envs = torch, torch.device("cpu"), StubVec(), 6
    env._stream = lambda: 77
    T, D = 4, 13
    ro = {"packed": torch.zeros(T, 6, D + 2)}
    values, final = torch.zeros(T + 1, 6), torch.zeros(6)
    for bad in (torch.zeros(T, 6), torch.zeros(T + 1, 6, dtype=torch.float64), torch.zeros(6, T + 1).t()):
        with pytest.raises(AssertionError, match="values must be"):
            env.advantages(ro, bad)
    with pytest.raises(AssertionError, match="final_values must be"):
        env.advantages(ro, values, torch.zeros(5))
    assert env.vec.calls == []
    adv, ret = env.advantages(ro, values)
    assert tuple(adv.shape) == tuple(ret.shape) == (T, 6) and adv.dtype == torch.float32
    adv2, ret2, st = env.advantages(ro, values, final, gamma=0.9, lam=0.8, stats=True)
    assert adv2 is adv and ret2 is ret and tuple(st.shape) == (3,) and st.dtype == torch.float64
    assert env.vec.calls == [(T, ro["packed"].data_ptr(), values.data_ptr(), adv.data_ptr(), ret.data_ptr(), 0, 0.99, 0.95, 0, 0, 77),
                             (T, ro["packed"].data_ptr(), values.data_ptr(), adv.data_ptr(), ret.data_ptr(), final.data_ptr(), 0.9, 0.8, 0, st.data_ptr(), 77)]
