"""Per-pile observations (include/chub.h: chub_pile_obs_device) without a device: one field list on every side, the two entry points
declared, exported and bound, the column count of a field mask, the name -> mask translation, and the torch adapter's refusal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import charginghub_env_amd as chub
from charginghub_env_amd import _lib, wrappers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fields_are_one_list():
    """the CHUB_PILE_* enum of the header, _lib.PILE_NAMES, the kernel's field bits and the order chub_get_slots documents"""
    hdr = open(os.path.join(ROOT, "include", "chub.h")).read()
    body = hdr[hdr.index("CHUB_PILE_CAR = 0"):hdr.index("CHUB_PILE_COUNT\n")]
    cols = [c.lower() for c in re.findall(r"\bCHUB_PILE_([A-Z0-9_]+)", body)]
    assert len(cols) == _lib.PILE_COUNT == len(_lib.PILE_NAMES) == len(set(_lib.PILE_NAMES)) == 9
    assert isinstance(_lib.PILE_NAMES, tuple)
    assert _lib.PILE_NAMES == ("car", "charge", "emergency", "power", "soc", "init_soc", "target_soc", "stay_time", "already_stay_time")
    for enum_name, name in zip(cols, _lib.PILE_NAMES):
        assert name.startswith(enum_name), (enum_name, name)  # (CHUB_PILE_ALREADY_STAY: already_stay_time)
    assert [_lib.PILE[n] for n in _lib.PILE_NAMES] == list(range(9))
    kern = open(os.path.join(ROOT, "charginghub-env_amd", "csrc", "chub_kernels.hip")).read()
    bits = re.findall(r"\bPF_([A-Z_]+) = (\d+)u", re.search(r"enum PileField : uint32_t \{([^}]*)\}", kern).group(1))
    assert [b[0].lower() for b in bits] == cols and [int(b[1]) for b in bits] == [1 << i for i in range(9)]
    doc = re.search(r"chub_get_slots: per env, per station k, field-major \[9\]\[piles\[k\]\]: (.*?)\(CHS\.hpp:245-246\)", hdr, re.S).group(1)
    listed = re.findall(r"\b(car|charge|emergency|power|soc|init_soc|target_soc|stay_time|already_stay_time)\b", doc)
    assert tuple(listed) == _lib.PILE_NAMES


def test_symbols_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chub.h")).read(), flags=re.S)
    assert re.search(r"^int chub_pile_obs_columns\(uint32_t fields\);", header, re.M)
    assert re.search(r"^int chub_pile_obs_device\(chub_env \*env, uint32_t fields, const uint8_t \*d_mask, float \*d_out, void \*stream\);", header, re.M)
    lib = _lib.load_library()
    for name, n_args in (("chub_pile_obs_columns", 1), ("chub_pile_obs_device", 5)):
        assert name in _lib.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args
    for method in ("pile_obs", "pile_obs_device"):
        assert callable(getattr(chub.VecChargingHub, method))
    assert callable(wrappers.TorchHubVecEnv.pile_obs)


def test_columns_of_a_field_mask():
    lib = _lib.load_library()
    assert lib.chub_pile_obs_columns(0) == -1 and "CHUB_PILE" in lib.chub_last_error().decode()
    assert lib.chub_pile_obs_columns(1 << 9) == -1
    assert lib.chub_pile_obs_columns(0x1FF | 1 << 9) == -1 and lib.chub_pile_obs_columns(1 << 31) == -1
    assert lib.chub_pile_obs_columns(0x1FF) == 9
    assert lib.chub_pile_obs_columns(0b10101) == 3
    for f in range(9):
        assert lib.chub_pile_obs_columns(1 << f) == 1
    for mask in range(1, 1 << 9):
        assert lib.chub_pile_obs_columns(mask) == bin(mask).count("1") == len(_lib.pile_fields_names(mask))


def test_bad_arguments_are_refused_without_a_device():
    lib = _lib.load_library()
    f = C.c_void_p(8)  # never dereferenced: the checks come first
    assert lib.chub_pile_obs_device(None, 0x1FF, None, f, None) == -1 and lib.chub_last_error().decode() == "null argument"
    assert lib.chub_pile_obs_device(f, 0x1FF, None, None, None) == -1 and lib.chub_last_error().decode() == "null argument"


def test_names_translate_to_masks():
    m = _lib.pile_fields_mask
    assert m(None) == 0x1FF and m(_lib.PILE_NAMES) == 0x1FF
    assert m(("car", "emergency", "soc")) == 0b10101 == m(["soc", "car", "emergency", "car"])  # a set: order and repeats do not matter
    assert m("power") == 8 and m(("already_stay_time",)) == 256
    assert m(0b110000000) == 0b110000000 and m(np.uint32(5)) == 5
    assert _lib.pile_fields_names(0b10101) == ("car", "emergency", "soc") and _lib.pile_fields_names(0x1FF) == _lib.PILE_NAMES
    for bad in (("car", "speed"), "SOC", ["stay"], ("",)):
        with pytest.raises(ValueError, match="unknown per-pile field"):
            m(bad)
    for bad in (0, 1 << 9, -1, ()):
        with pytest.raises(ValueError):
            m(bad)


class StubVec(object):
    """what TorchHubVecEnv.pile_obs touches of a VecChargingHub"""

    def __init__(self):
        self.calls = []

    def pile_obs_device(self, d_out, fields=None, d_mask=0, stream=0):
        self.calls.append((d_out, fields, d_mask, stream))


def bare_adapter(pile_buf, mask):
    env = object.__new__(wrappers.TorchHubVecEnv)  # (the constructor creates a handle on a device)
    env.vec, env._pile_buf, env._pile_mask = StubVec(), pile_buf, mask
    env._stream = lambda: 77
    return env


def test_torch_adapter_refuses_without_the_option_and_passes_its_buffer_with_it():
    env = bare_adapter(None, None)
    with pytest.raises(RuntimeError, match="construct with pile_obs="):
        env.pile_obs()
    assert env.vec.calls == []

    class Buf(object):
        def data_ptr(self):
            return 4096

    buf = Buf()
    env = bare_adapter(buf, 0b10101)
    assert env.pile_obs() is buf and env.pile_obs() is buf  # one buffer, overwritten by the next call
    assert env.vec.calls == [(4096, 0b10101, 0, 77)] * 2  # ... filled on the adapter's stream, every env


def test_torch_adapter_rejects_an_unknown_name_before_it_builds_anything():
    pytest.importorskip("torch")
    with pytest.raises(ValueError, match="unknown per-pile field"):
        wrappers.TorchHubVecEnv(4, [20, 25], ["fast", "slow"], pile_obs=("car", "speed"))
