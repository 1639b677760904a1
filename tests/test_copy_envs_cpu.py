"""chub_copy_envs / chub_copy_envs_device without a device: the two symbols are declared in include/chub.h, exported by the library and
bound by the ctypes layer, the Python methods exist, and null arguments are refused before anything touches the GPU."""
import ctypes as C
import os
import re

import numpy as np

import charginghub_env_amd as chub
from charginghub_env_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("chub_copy_envs", "chub_copy_envs_device")


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "chub.h")).read()
    lib = _lib.load_library()
    for name in NAMES:
        assert re.search(r"^int %s\(chub_env \*dst, chub_env \*src, " % name, header, re.M), name
        assert name in _lib.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == (5 if name == "chub_copy_envs" else 6)
        assert not name.startswith(("chub_reset", "chub_step", "chub_run_steps"))
    assert callable(chub.VecChargingHub.copy_envs) and callable(chub.VecChargingHub.copy_envs_device)
    assert callable(chub.wrappers.TorchHubVecEnv.copy_envs)
    assert not hasattr(chub.wrappers.StaggeredHub, "copy_envs")


def test_null_arguments_are_refused_without_a_device():
    lib = _lib.load_library()
    idx = np.zeros(2, dtype=np.int64)
    p = idx.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(8)  # never dereferenced: the null checks come first
    for args in ((None, None, p, p, 2), (None, fake, p, p, 2), (fake, None, p, p, 2), (fake, fake, None, p, 2), (fake, fake, p, None, 2)):
        assert lib.chub_copy_envs(*args) == -1
        assert lib.chub_last_error().decode() == "null argument"
        assert lib.chub_copy_envs_device(*args, None) == -1
        assert lib.chub_last_error().decode() == "null argument"
