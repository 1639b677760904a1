"""rng_mode PHILOX_CURVES at the interface, without a GPU: the header's enum, the Python constant and the validation of the mode come
before any device call (tests/test_gpu_soc_curves.py runs the mode itself)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_python_and_library_agree_on_the_third_mode():
    from charginghub_env_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "chub.h")).read()
    modes = dict((n, int(v)) for n, v in re.findall(r"\bCHUB_RNG_(\w+) = (\d+)", hdr))
    assert modes == {"COMPAT": _lib.RNG_COMPAT, "PHILOX": _lib.RNG_PHILOX, "PHILOX_CURVES": _lib.RNG_PHILOX_CURVES} == {"COMPAT": 0, "PHILOX": 1, "PHILOX_CURVES": 2}
    assert _lib.RNG_MODES == {"compat": 0, "philox": 1, "philox_curves": 2}


def test_create_accepts_the_mode_and_refuses_what_it_does_not_cover():
    import charginghub_env_amd as m
    from charginghub_env_amd import _lib
    lib = m.load_library()
    h = C.c_void_p()
    data = _lib.DATA_DIR.encode()
    big = m.make_config([65, 20], ["fast", "slow"])  # a station's unit must fit one wave of k_slot_curves
    assert lib.chub_create(C.byref(big), data, 4, 0, 0, 1, _lib.RNG_PHILOX_CURVES, C.byref(h)) == -4
    assert b"PHILOX_CURVES covers stations of at most 64 piles" in lib.chub_last_error()
    assert lib.chub_create(C.byref(big), data, 4, 0, 0, 1, 3, C.byref(h)) == -1  # (one past the last mode)
    assert b"unknown rng_mode" in lib.chub_last_error()
    if lib.chub_device_count() == 0:  # the mode itself passes the argument checks: what stops it here is the missing device
        good = m.make_config([20, 25], ["fast", "slow"])
        assert lib.chub_create(C.byref(good), data, 4, 0, 0, 1, _lib.RNG_PHILOX_CURVES, C.byref(h)) == -3
        assert b"no HIP device" in lib.chub_last_error()
    assert not h.value


def test_python_constructors_validate_the_name():
    import charginghub_env_amd as m
    with pytest.raises(ValueError, match="philox_curves"):
        m.VecChargingHub(4, [20, 25], ["fast", "slow"], rng="curves")
    with pytest.raises(ValueError, match="philox_curves"):
        m.EvcsspManagerEnv_v6([20, 25], ["fast", "slow"], rng="curves")
