"""Station-level control (include/chub.h: chub_load_dispatch_device) without a device: the numpy definition (tests/load_dispatch_lib.py)
on a case checked by hand, the definition held to the CPU oracle -- OrcStation.step_load(load) against OrcStation.step(rows built by the
definition), bit for bit at every step -- the names and enum values on every side, the refusals that need no device, and the torch
adapter's option."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import charginghub_env_amd as chub
import load_dispatch_lib as ldl
from charginghub_env_amd import _lib, wrappers
from orclib import COMPAT, PHILOX, OrcStation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_the_definition_on_a_case_checked_by_hand():
    """One fast station of 8 piles.  Order by emergency descending, ties by slot: 0 (10), 3 (10), 6 (.5), 4 (.25), then the zeros 1 (no car), 2,
    5, 7 (no car).  Running sum over the cars: 5, 7, 7.5, 11.5, 14.5, 15.5; the stray power on the empty pile 1 must not count."""
    car = np.array([[1, 0, 1, 1, 1, 1, 1, 0]], dtype=F32)
    em = np.array([[10, 0, 0, 10, 0.25, 0, 0.5, 0]], dtype=F32)
    pw = np.array([[5, 9, 3, 2, 4, 1, 0.5, 0]], dtype=F32)

    def on(load, mn=7.0, mx=15.5, cc=False, units=ldl.KW, details=False):
        return ldl.station_dispatch(car, em, pw, [mn], [mx], [load], 0, cc, units, details)

    def piles(*idx):
        want = np.zeros((1, 8), dtype=bool)
        want[0, list(idx)] = True
        return want

    assert np.array_equal(on(11.5), piles(0, 3, 6, 4))     # a load equal to a running sum: that car is on
    assert np.array_equal(on(11.25), piles(0, 3, 6))
    assert np.array_equal(on(14.5), piles(0, 3, 6, 4, 2))  # the tie among emergency 0: slot 2 before slot 5
    assert np.array_equal(on(15.0), piles(0, 3, 6, 4, 2))
    assert np.array_equal(on(3.0), piles(0, 3))            # below min_power: clamped to 7 = the two must-charge cars
    assert np.array_equal(on(100.0), piles(0, 3, 6, 4, 2, 5))  # above max_power: every car, never an empty pile
    # the must-charge clause: with a record that does not cover them (mn = 0) a load of 5 reaches slot 0 alone; slot 3 is on all the same
    got, beyond = on(5.0, mn=0.0, details=True)
    assert np.array_equal(got, piles(0, 3)) and beyond.tolist() == [1]
    assert on(11.5, details=True)[1].tolist() == [0]
    # fraction units: a = -1 is mn, a = +1 is mx, a = 0 the middle (11.25), and beyond [-1, 1] it saturates
    assert np.array_equal(on(-1.0, units=ldl.FRACTION), piles(0, 3)) and np.array_equal(on(-7.0, units=ldl.FRACTION), piles(0, 3))
    assert np.array_equal(on(0.0, units=ldl.FRACTION), piles(0, 3, 6))
    assert np.array_equal(on(1.0, units=ldl.FRACTION), piles(0, 3, 6, 4, 2, 5)) and np.array_equal(on(9.0, units=ldl.FRACTION), piles(0, 3, 6, 4, 2, 5))
    assert ldl.target([0.0], [7.0], [15.5], ldl.FRACTION).tolist() == [11.25]
    # constant charging: the first roundf(load / constant_power) cars of the order; roundf sends .5 away from zero (2.5 -> 3, 0.5 -> 1)
    cp = ldl.CONSTANT_POWER[0]
    for q, n_on in ((2.5, 3), (0.5, 1), (2.25, 2), (0.0, 0)):
        load = F32(q) * cp
        assert F32(load / cp) == F32(q)
        assert ldl.roundf(load / cp) == n_on
        got = on(load, mn=0.0, mx=1000.0, cc=True)
        assert np.array_equal(got, piles(*([0, 3, 6, 4, 2, 5][:n_on] + [0, 3]))), (q, got)  # (the two must-charge cars whatever the count)
    assert ldl.roundf([-0.5, 1.5, 0.49999997, 3.0]).tolist() == [-1.0, 2.0, 0.0, 3.0]
    # rows and bits of a hub [3, 5] read from the same columns: station 0 = piles 0-2, station 1 = piles 3-7
    cols = np.stack([car, em, pw], axis=1)
    scal = np.zeros((1, 2, 8))
    scal[0, 0, [0, 2]] = 0.0, 8.0
    scal[0, 1, [0, 2]] = 2.0, 7.5
    rows, bits, beyond = ldl.hub_dispatch(cols, scal, [3, 5], [0, 1], False, [[5.0, 6.5]], [[0.25, -0.5]], details=True)
    assert rows.dtype == F32 and rows.tolist() == [[1, -1, -1, 1, 1, -1, 1, -1, 0.25, -0.5]]  # station 1: 3 (2), 6 (2.5), 4 (6.5), 5 (7.5)
    assert bits.dtype == np.uint64 and bits.tolist() == [[0b01011001]] and beyond.tolist() == [[0, 0]]
    rows, bits = ldl.hub_dispatch(cols, scal, [0, 8], [0, 1], False, [[99.0, 3.0]], [[0, 0]])  # station 0 has no piles: its load is not read
    assert bits.tolist() == [[0b00001001]]
    assert ldl.pack_bits(np.ones((2, 65), bool)).tolist() == [[2 ** 64 - 1, 1]] * 2


@pytest.mark.parametrize("cc", [False, True], ids=["curve", "constant"])
@pytest.mark.parametrize("typ", [0, 1], ids=["fast", "slow"])
@pytest.mark.parametrize("mode", [COMPAT, PHILOX], ids=["compat", "philox"])
def test_the_definition_is_the_oracles_scalar_load_step(mode, typ, cc):
    """step_load(load) == step(rows from the definition) on stations of 1, 5, 25 and 64 piles, 8 seeds x 288 steps each, with loads inside,
    below, above and exactly at min_power, and exactly at a car's running sum: slots and scalars bit-identical at every step, and no
    must-charge car ever beyond the load (the clause of the definition that a scalar-load step does not have stays idle)."""
    seeds, steps = 8, 288
    rs = np.random.RandomState(1000 * mode + 10 * typ + int(cc))
    for piles in (1, 5, 25, 64):
        a = [OrcStation(typ, piles, constant_charging=cc) for _ in range(seeds)]
        b = [OrcStation(typ, piles, constant_charging=cc) for _ in range(seeds)]
        for s in range(seeds):
            for st in (a[s], b[s]):
                if mode == COMPAT:
                    st.seed_compat(100 + s, 7000 + 3 * s)
                else:
                    st.seed_philox(77, s)
                    st.set_tick(1)
                st.reset()
        for t in range(steps + 1):
            sl_a, sl_b = np.stack([st.slots() for st in a]), np.stack([st.slots() for st in b])
            sc_a, sc_b = np.stack([st.scalars() for st in a]), np.stack([st.scalars() for st in b])
            assert np.array_equal(sl_a.view(np.uint32), sl_b.view(np.uint32)), (piles, t)
            assert np.array_equal(sc_a, sc_b), (piles, t)
            if t == steps:
                break
            mn, mx = sc_b[:, 0].astype(F32), sc_b[:, 2].astype(F32)
            u = rs.uniform(size=seeds).astype(F32)
            kind = (t + np.arange(seeds)) % 5
            car, pw = sl_b[:, 0] > 0.5, sl_b[:, 3]
            order = np.argsort(-sl_b[:, 2], axis=1, kind="stable")
            cum = np.cumsum(np.take_along_axis(np.where(car, pw, F32(0)).astype(F32), order, axis=1), axis=1, dtype=F32)
            loads = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                              [mn + u * (mx - mn), mn - F32(1) - u, mx + F32(1) + u, mn], cum[np.arange(seeds), (t // 5) % piles]).astype(F32)
            on, beyond = ldl.station_dispatch(sl_b[:, 0], sl_b[:, 2], sl_b[:, 3], mn, mx, loads, typ, cc, details=True)
            assert beyond.sum() == 0, (piles, t, beyond)
            for s in range(seeds):
                if mode == PHILOX:
                    a[s].set_tick(t + 2)
                    b[s].set_tick(t + 2)
                a[s].step_load(loads[s])
                b[s].step(on[s].astype(F32))


def test_names_and_values_agree_in_header_and_binding():
    hdr = open(os.path.join(ROOT, "include", "chub.h")).read()
    assert re.search(r"enum \{ CHUB_LOAD_KW = 0, CHUB_LOAD_FRACTION = 1 \};", hdr)
    assert (_lib.LOAD_KW, _lib.LOAD_FRACTION) == (0, 1) == (ldl.KW, ldl.FRACTION) and _lib.LOAD_UNITS == {"kw": 0, "fraction": 1}
    header = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"^int chub_load_dispatch_device\(chub_env \*env, int units, const float \*d_loads\s*, const float \*d_tail\s*,\s*"
                     r"const uint8_t \*d_mask\s*, float \*d_actions\s*,\s*uint64_t \*d_pile_bits\s*, void \*stream\);", header, re.M)
    assert re.search(r"^int chub_load_dispatch\(chub_env \*env, int units, const float \*loads, const float \*tail, float \*actions, "
                     r"uint64_t \*pile_bits\);", header, re.M)
    lib = _lib.load_library()
    for name, n_args in (("chub_load_dispatch_device", 8), ("chub_load_dispatch", 6)):
        assert name in _lib.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args
    for method in ("load_dispatch", "load_dispatch_device", "step_load_device"):
        assert callable(getattr(chub.VecChargingHub, method))
    assert _lib.load_units("kw") == 0 and _lib.load_units("fraction") == 1 and _lib.load_units(1) == 1 and _lib.load_units(0) == 0
    for bad in ("KW", "percent", 2, -1, None):
        with pytest.raises(ValueError, match="load units"):
            _lib.load_units(bad)
    # the constant powers of the definition are the kernels' (chub_curves.h)
    curves = open(os.path.join(ROOT, "charginghub-env_amd", "csrc", "chub_curves.h")).read()
    for typ, name in ((0, "kFastConstantPower"), (1, "kSlowConstantPower")):
        assert F32(float(re.search(name + r" = \(float\) ([0-9.]+);", curves).group(1))) == ldl.CONSTANT_POWER[typ]


def test_bad_arguments_are_refused_without_a_device():
    lib = _lib.load_library()
    f = C.c_void_p(8)  # never dereferenced: the checks come first
    dev = lib.chub_load_dispatch_device
    assert dev(None, 0, f, f, None, f, f, None) == -1 and lib.chub_last_error().decode() == "null argument"
    assert dev(f, 0, None, f, None, f, f, None) == -1 and lib.chub_last_error().decode() == "null argument"
    assert dev(f, 0, f, f, None, None, None, None) == -1 and "d_actions, d_pile_bits or both" in lib.chub_last_error().decode()
    assert dev(f, 0, f, None, None, f, None, None) == -1 and "need d_tail" in lib.chub_last_error().decode()
    assert dev(f, 0, f, None, None, f, f, None) == -1 and "need d_tail" in lib.chub_last_error().decode()
    for units in (2, -1, 1 << 20):
        assert dev(f, units, f, f, None, f, f, None) == -1 and "CHUB_LOAD_KW or CHUB_LOAD_FRACTION" in lib.chub_last_error().decode()
    host = lib.chub_load_dispatch
    assert host(None, 0, f, f, f, f) == -1 and host(f, 0, None, f, f, f) == -1
    assert host(f, 0, f, f, None, None) == -1 and host(f, 0, f, None, f, None) == -1
    assert host(f, 5, f, f, f, f) == -1 and "CHUB_LOAD_KW or CHUB_LOAD_FRACTION" in lib.chub_last_error().decode()


def test_torch_adapter_rejects_a_bad_option_before_it_builds_anything():
    pytest.importorskip("torch")
    with pytest.raises(ValueError, match="control must be 'pile' or 'station'"):
        wrappers.TorchHubVecEnv(4, [20, 25], ["fast", "slow"], control="load")
    with pytest.raises(ValueError, match="load units"):
        wrappers.TorchHubVecEnv(4, [20, 25], ["fast", "slow"], control="station", load_units="percent")
    with pytest.raises(ValueError, match="load units"):
        wrappers.TorchHubVecEnv(4, [20, 25], ["fast", "slow"], load_units=3)


class StubVec(object):
    """what TorchHubVecEnv.step touches of a VecChargingHub"""
    bit_words = 1

    def __init__(self):
        self.calls = []

    def load_dispatch_device(self, d_loads, d_tail, d_actions=0, d_pile_bits=0, units="kw", d_mask=0, stream=0):
        self.calls.append(("dispatch", d_loads, d_tail, d_actions, d_pile_bits, units, d_mask, stream))

    def step_device_packed(self, d_actions, d_packed, d_exo_z=0, stream=0):
        self.calls.append(("step", d_actions, d_packed, stream))

    def step_autoreset_device(self, d_actions, d_packed, d_final_obs=0, **kw):
        self.calls.append(("autoreset", d_actions, d_packed, d_final_obs, kw.get("stream")))


@pytest.mark.parametrize("per_env", [False, True])
def test_torch_adapter_dispatches_into_its_own_rows_then_takes_the_step_path(per_env):
    torch = pytest.importorskip("torch")
    n, D, A = 3, 13, 47
    env = object.__new__(wrappers.TorchHubVecEnv)  # (the constructor creates a handle on a device)
    env.torch, env.device, env.vec = torch, torch.device("cpu"), StubVec()
    env.num_envs, env.obs_dim, env.act_dim, env.per_env, env.autoreset, env._t = n, D, 4, per_env, False, 0
    env._packed, env.last_obs = torch.zeros((n, D + 2)), torch.zeros((n, D))
    env._rows, env._loads, env._tail, env._load_units = torch.zeros((n, A)), torch.zeros((n, 2)), torch.zeros((n, 2)), _lib.LOAD_FRACTION
    with pytest.raises(AssertionError, match=r"shape \(3, 4\)"):
        env.step(torch.zeros((n, A)))
    act = torch.tensor([[0.5, -0.5, 0.1, 0.2], [1, -1, 0.3, 0.4], [0, 0, 0.5, 0.6]], dtype=torch.float32)
    env.step(act)
    rows = env._rows.data_ptr()
    want_step = ("autoreset", rows, env._packed.data_ptr(), env.last_obs.data_ptr(), 0) if per_env else ("step", rows, env._packed.data_ptr(), 0)
    assert env.vec.calls == [("dispatch", env._loads.data_ptr(), env._tail.data_ptr(), rows, 0, _lib.LOAD_FRACTION, 0, 0), want_step]
    assert torch.equal(env._loads, act[:, :2]) and torch.equal(env._tail, act[:, 2:])
    with pytest.raises(RuntimeError, match="control='station'"):
        env.step_bits(torch.zeros((n, 1), dtype=torch.int64), torch.zeros((n, 2)))
