"""Per-station deadline profiles (include/chub.h: chub_station_profile_device) without a device: one field list on every side, the two
entry points declared, exported and bound, the size of a (fields, buckets) pair, the refusals that need no device, the name -> mask
translation, the numpy definition (tests/station_profile_lib.py) on a case small enough to check by hand, and the torch adapter's option."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import charginghub_env_amd as chub
import station_profile_lib as spl
from charginghub_env_amd import _lib, wrappers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = (1 << 7) - 1


def test_fields_are_one_list():
    """the CHUB_SP_* enum of the header, _lib.SP_NAMES, the kernel's field bits and the test oracle's names"""
    hdr = open(os.path.join(ROOT, "include", "chub.h")).read()
    body = hdr[hdr.index("CHUB_SP_CARS = 0"):hdr.index("CHUB_SP_COUNT\n")]
    cols = [c.lower() for c in re.findall(r"\bCHUB_SP_([A-Z0-9_]+)", body)]
    assert isinstance(_lib.SP_NAMES, tuple) and len(set(_lib.SP_NAMES)) == _lib.SP_COUNT == 7
    assert tuple(cols) == _lib.SP_NAMES == spl.SP_NAMES == ("cars", "charging", "must_charge", "power", "power_charging", "emergency", "soc_gap")
    assert [_lib.SP[n] for n in _lib.SP_NAMES] == list(range(7))
    kern = open(os.path.join(ROOT, "charginghub-env_amd", "csrc", "chub_kernels.hip")).read()
    bits = re.findall(r"\bSPF_([A-Z_]+) = (\d+)u", re.search(r"enum ProfileField : uint32_t \{([^}]*)\}", kern).group(1))
    assert [b[0].lower() for b in bits] == cols and [int(b[1]) for b in bits] == [1 << i for i in range(7)]


def test_symbols_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chub.h")).read(), flags=re.S)
    assert re.search(r"^int chub_station_profile_size\(uint32_t fields, int32_t buckets\);", header, re.M)
    assert re.search(r"^int chub_station_profile_device\(chub_env \*env, uint32_t fields, int32_t buckets, const uint8_t \*d_mask, "
                     r"float \*d_out, void \*stream\);", header, re.M)
    lib = _lib.load_library()
    for name, n_args in (("chub_station_profile_size", 2), ("chub_station_profile_device", 6)):
        assert name in _lib.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args
    for method in ("station_profile", "station_profile_device"):
        assert callable(getattr(chub.VecChargingHub, method))
    assert callable(wrappers.TorchHubVecEnv.station_profile)


def test_size_of_fields_and_buckets():
    lib = _lib.load_library()
    for mask in range(1, 1 << 7):
        for B in (1, 2, 8, 31, 32):
            assert lib.chub_station_profile_size(mask, B) == 2 * bin(mask).count("1") * B == 2 * len(_lib.sp_fields_names(mask)) * B
    assert lib.chub_station_profile_size(ALL, 32) == 448
    assert lib.chub_station_profile_size(0, 8) == -1 and "CHUB_SP" in lib.chub_last_error().decode()
    for mask in (1 << 7, ALL | 1 << 7, 1 << 31):
        assert lib.chub_station_profile_size(mask, 8) == -1
    for B in (0, -1, 33, 1 << 20):
        assert lib.chub_station_profile_size(ALL, B) == -1 and "buckets" in lib.chub_last_error().decode()


def test_bad_arguments_are_refused_without_a_device():
    lib = _lib.load_library()
    f = C.c_void_p(8)  # never dereferenced: the checks come first
    assert lib.chub_station_profile_device(None, ALL, 8, None, f, None) == -1 and lib.chub_last_error().decode() == "null argument"
    assert lib.chub_station_profile_device(f, ALL, 8, None, None, None) == -1 and lib.chub_last_error().decode() == "null argument"
    for mask, B in ((0, 8), (1 << 7, 8), (ALL, 0), (ALL, 33)):
        assert lib.chub_station_profile_device(f, mask, B, None, f, None) == -1


def test_names_translate_to_masks():
    m = _lib.sp_fields_mask
    assert m(None) == ALL and m(_lib.SP_NAMES) == ALL
    assert m(("cars", "must_charge", "power")) == 0b1101 == m(["power", "cars", "must_charge", "cars"])  # a set: order and repeats do not matter
    assert m("soc_gap") == 64 and m(("power_charging",)) == 16
    assert m(0b1100000) == 0b1100000 and m(np.uint32(5)) == 5
    assert _lib.sp_fields_names(0b1101) == ("cars", "must_charge", "power") and _lib.sp_fields_names(ALL) == _lib.SP_NAMES
    for bad in (("cars", "speed"), "POWER", ["soc"], ("",)):
        with pytest.raises(ValueError, match="unknown station-profile field"):
            m(bad)
    for bad in (0, 1 << 7, -1, ()):
        with pytest.raises(ValueError):
            m(bad)


def test_the_definition_on_a_case_checked_by_hand():
    """2 envs of hub [3, 2], B = 4.  Columns: car, charge, emergency, power, soc, init_soc, target_soc, stay_time, already_stay_time.
    Ties at exactly half a quantum go to the even neighbour: 0.5 -> 0 and 1.5 -> 2 quanta (power 2^-20 and 3 * 2^-20 kW, emergency
    3 * 2^-21, soc_gap 3 * 2^-17 %); a car with 7 and one with 38 slots left sit in the last bucket, one with exactly 4 too; env 0's
    station 1 is empty, with stray values on a pile without a car that must not count; read as hub [5, 0] station 1 has no piles."""
    h, none = 2.0 ** -20, [0, 0, 0, 0, 0, 0, 0, -1, -1]
    piles = np.array([
        [[1, 1, 10, 7.5, 50, 20, 90, 5, 4], [1, 0, 0.25, h, 60.5, 30, 80.25, 10, 3], [1, 1, 10, 3 * h, 70, 40, 95, 9, 8],
         none, [0, 1, 0, 5.0, 0, 0, 0, -1, -1]],
        [[1, 0, 1.5, 11.25, 30, 30, 100, 6, 4], none, [1, 1, h / 2, 4.0, 99.5, 50, 99.25, 3, 1],
         [1, 1, 10, 22.0, 10, 10, 85, 4, 0], [1, 0, 3 * h / 2, 0.0, 81, 81, 81 + 3 * 2.0 ** -17, 40, 2]]], dtype=np.float32)
    cols = np.ascontiguousarray(piles.transpose(0, 2, 1))  # [N][9][S]
    assert cols.shape == (2, 9, 5) and cols[1, 6, 4] == np.float32(81 + 3 * 2.0 ** -17) != 81
    got = spl.profile_from_columns(cols, [3, 2], None, 4)
    assert got.shape == (2, 2, 7, 4) and got.dtype == np.float32
    p0 = 7.5 + 2.0 ** -18  # (7.5 * 2^19 + 2 quanta) * 2^-19: the half quantum of the pile in bucket 3 went to 0, the 1.5 to 2
    want = np.array([
        [[[2, 0, 0, 1], [2, 0, 0, 0], [2, 0, 0, 0], [p0, 0, 0, 0], [p0, 0, 0, 0], [20, 0, 0, 0.25], [65, 0, 0, 19.75]],
         np.zeros((7, 4))],
        [[[0, 2, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0], [0, 15.25, 0, 0], [0, 4, 0, 0], [0, 1.5, 0, 0], [0, 69.75, 0, 0]],
         [[0, 0, 0, 2], [0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 22], [0, 0, 0, 22], [0, 0, 0, 10 + 2.0 ** -19], [0, 0, 0, 75 + 2.0 ** -15]]]])
    assert np.array_equal(got, want.astype(np.float32)), (got, want)
    assert np.float32(p0) != 7.5 and np.float32(10 + 2.0 ** -19) != 10 and np.float32(75 + 2.0 ** -15) != 75  # (the quanta show in f32)
    # a field subset is the matching columns; B = 1 is the station totals; a 0-pile station is a block of zeros
    assert np.array_equal(spl.profile_from_columns(cols, [3, 2], ("soc_gap", "cars"), 4), got[:, :, [0, 6]])
    assert np.array_equal(spl.profile_from_columns(cols, [3, 2], 0b0001001, 1)[..., 0], np.array([[[3, p0], [0, 0]], [[2, 15.25], [2, 22]]], dtype=np.float32))
    assert np.array_equal(spl.profile_from_columns(cols, [5, 0], ("cars", "power"), 1)[..., 0], np.array([[[3, p0], [0, 0]], [[4, 37.25], [0, 0]]], dtype=np.float32))
    assert np.array_equal(spl.profile_from_columns(cols, [0, 5], ("cars", "power"), 1)[..., 0], np.array([[[0, 0], [3, p0]], [[0, 0], [4, 37.25]]], dtype=np.float32))
    # the last bucket moves with B: at B = 32 the car with 38 slots left is alone in bucket 31, the one with 7 in bucket 6
    wide = spl.profile_from_columns(cols, [3, 2], "cars", 32)[:, :, 0]
    assert wide[1, 1, 31] == 1 and wide[1, 1, 3] == 1 and wide[0, 0, 6] == 1 and wide.sum() == 7


class StubVec(object):
    """what TorchHubVecEnv.station_profile touches of a VecChargingHub"""

    def __init__(self):
        self.calls = []

    def station_profile_device(self, d_out, fields=None, buckets=8, d_mask=0, stream=0):
        self.calls.append((d_out, fields, buckets, d_mask, stream))


def bare_adapter(buf, mask, buckets):
    env = object.__new__(wrappers.TorchHubVecEnv)  # (the constructor creates a handle on a device)
    env.vec, env._sp_buf, env._sp_mask, env._sp_buckets = StubVec(), buf, mask, buckets
    env._stream = lambda: 77
    return env


def test_torch_adapter_refuses_without_the_option_and_passes_its_buffer_with_it():
    env = bare_adapter(None, None, None)
    with pytest.raises(RuntimeError, match="construct with station_profile="):
        env.station_profile()
    assert env.vec.calls == []

    class Buf(object):
        def data_ptr(self):
            return 4096

    buf = Buf()
    env = bare_adapter(buf, 0b1101, 8)
    assert env.station_profile() is buf and env.station_profile() is buf  # one buffer, overwritten by the next call
    assert env.vec.calls == [(4096, 0b1101, 8, 0, 77)] * 2  # ... filled on the adapter's stream, every env


def test_torch_adapter_rejects_a_bad_option_before_it_builds_anything():
    pytest.importorskip("torch")
    with pytest.raises(ValueError, match="unknown station-profile field"):
        wrappers.TorchHubVecEnv(4, [20, 25], ["fast", "slow"], station_profile=dict(fields=("cars", "speed"), buckets=8))
    with pytest.raises(ValueError, match="buckets"):
        wrappers.TorchHubVecEnv(4, [20, 25], ["fast", "slow"], station_profile=dict(fields=("cars",), buckets=33))
    with pytest.raises(ValueError, match="station_profile"):
        wrappers.TorchHubVecEnv(4, [20, 25], ["fast", "slow"], station_profile=dict(field=("cars",)))
