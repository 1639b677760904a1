"""The per-episode ledger (include/chub.h: chub_set_episode_stats) without a device: one column list on every side, the entry points declared,
exported and bound, the stable-baselines adapter's ``infos[i]["episode"]`` against a stand-in hub, and the two facts about the reference's
recordings that tests/test_gpu_episode_stats.py builds its bars on."""
import ctypes as C
import glob
import os
import re

import numpy as np

import charginghub_env_amd as chub
from charginghub_env_amd import _lib, vec_env, wrappers

import orclib
from test_wrappers_cpu import FakeHub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"chub_set_episode_stats": 2, "chub_has_episode_stats": 1, "chub_get_episode_stats": 3, "chub_get_episode_counts": 2,
         "chub_episode_stats_device": 5, "chub_episode_summary_device": 4, "chub_episode_summary": 3}


def test_columns_are_one_list():
    """the CHUB_EP_* enum of the header, the device-side column count and enum, and _lib.EPISODE_NAMES"""
    hdr = open(os.path.join(ROOT, "include", "chub.h")).read()
    body = hdr[hdr.index("CHUB_EP_RETURN = 0"):hdr.index("CHUB_EP_COUNT\n")]
    cols = re.findall(r"\bCHUB_EP_([A-Z0-9_]+)", body)
    assert [c.lower() for c in cols] == _lib.EPISODE_NAMES
    assert len(cols) == _lib.EP_COUNT == len(set(_lib.EPISODE_NAMES)) == 7
    dev = open(os.path.join(ROOT, "charginghub-env_amd", "csrc", "chub_device.h")).read()
    assert int(re.search(r"kEpCount = (\d+);", dev).group(1)) == _lib.EP_COUNT
    dev_cols = re.findall(r"\bEPC_([A-Z0-9_]+)", re.search(r"enum EpCol \{([^}]*)\}", dev).group(1))
    assert dev_cols == cols
    assert [_lib.EP[n] for n in _lib.EPISODE_NAMES] == list(range(7))
    # the existing enums and the option struct are where they were
    assert _lib.T_COUNT == 38 and int(re.search(r"kTelemCount = (\d+);", dev).group(1)) == 38 and C.sizeof(_lib.ChubOptions) == 32


def test_symbols_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chub.h")).read(), flags=re.S)
    lib = _lib.load_library()
    for name, n_args in NAMES.items():
        m = re.search(r"^int %s\(((?:const )?chub_env \*env[^;]*)\);" % name, header, re.M | re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name
        assert name in _lib.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args
    for method in ("set_episode_stats", "episode_stats", "episode_counts", "episode_stats_device", "episode_summary", "episode_summary_device"):
        assert callable(getattr(chub.VecChargingHub, method))
    assert isinstance(chub.VecChargingHub.has_episode_stats, property)
    for method in ("episode_stats", "episode_summary"):
        assert callable(getattr(wrappers.TorchHubVecEnv, method))


def test_null_arguments_are_refused_without_a_device():
    lib = _lib.load_library()
    f = C.c_void_p(8)  # never dereferenced: the null checks come first
    assert lib.chub_set_episode_stats(None, 1) == -1 and lib.chub_last_error().decode() == "null handle"
    assert lib.chub_has_episode_stats(None) == -1
    for fn, calls in ((lib.chub_get_episode_stats, ((None, 0, f), (f, 0, None))), (lib.chub_get_episode_counts, ((None, f), (f, None))),
                      (lib.chub_episode_stats_device, ((None, 1, f, None, None), (f, 1, None, None, None))),
                      (lib.chub_episode_summary_device, ((None, f, 1, None), (f, None, 1, None))),
                      (lib.chub_episode_summary, ((None, f, 1), (f, None, 1)))):
        for args in calls:
            assert fn(*args) == -1
            assert lib.chub_last_error().decode() == "null argument"


def test_summary_dict_means_and_deviations():
    x = np.array([[1.0, 2.0, 4.0], [3.0, 3.0, 3.0]])
    raw = [3.0]
    for i in range(_lib.EP_COUNT):
        col = x[i % 2]
        raw += [col.sum(), (col * col).sum(), col.min(), col.max()]
    d = vec_env.summary_dict(raw)
    assert d["count"] == 3 and set(d) == {"count"} | set(_lib.EPISODE_NAMES)
    assert d["return"]["mean"] == 7.0 / 3 and abs(d["return"]["std"] - np.std(x[0])) < 1e-15 and d["return"]["min"] == 1.0 and d["return"]["max"] == 4.0
    assert d["income"]["std"] == 0.0
    empty = vec_env.summary_dict([0.0] + [0.0, 0.0, np.inf, -np.inf] * _lib.EP_COUNT)
    assert empty["count"] == 0 and np.isnan(empty["length"]["mean"]) and empty["length"]["min"] == np.inf and empty["length"]["max"] == -np.inf


class LedgerHub(FakeHub):
    """FakeHub with the ledger surface of VecChargingHub: reward 1 per step, income 2, draw_ele 3"""

    def __init__(self, *a, **kw):
        FakeHub.__init__(self, *a, **kw)
        self.ledger_on, self.length = False, 0

    def set_episode_stats(self, on=True):
        self.ledger_on = on

    def reset(self):
        self.length = 0
        return FakeHub.reset(self)

    def step(self, actions):
        self.length += 1
        return FakeHub.step(self, actions)

    def episode_stats(self, finished=False):
        assert self.ledger_on and not finished  # (the adapter reads the running episode, before its reset)
        full = lambda v: np.full(self.n_envs, v, dtype=np.float64)
        return {"return": full(self.length) + np.arange(self.n_envs), "income": full(2.0 * self.length), "draw_ele": full(3.0 * self.length),
                "length": full(self.length), "deviation": full(0.25), "test_penalty": full(0.5), "end_soc": full(0.75)}


def test_sb3_adapter_reports_the_episode_where_it_ended():
    hub = LedgerHub()
    env = wrappers.HubVecEnv(vec=hub, episode_stats=True)
    assert hub.ledger_on and env.episode_stats
    env.reset()
    a = np.zeros((4, 7), dtype=np.float32)
    for t in range(95):
        _, _, dones, infos = env.step(a)
        assert not dones.any() and all(info == {} for info in infos)
    _, _, dones, infos = env.step(a)
    assert dones.all()
    for i, info in enumerate(infos):
        assert set(info) == {"terminal_observation", "TimeLimit.truncated", "episode"}
        assert info["episode"] == {"r": 96.0 + i, "l": 96, "income": 192.0, "draw_ele": 288.0, "test_penalty": 0.5, "end_soc": 0.75}
        assert isinstance(info["episode"]["l"], int) and isinstance(info["episode"]["r"], float)
    _, _, dones, infos = env.step(a)  # the next episode has started over
    assert not dones.any() and all(info == {} for info in infos) and hub.length == 1
    # an episode the time limit cuts short reports what it had
    hub = LedgerHub()
    env = wrappers.HubVecEnv(vec=hub, max_episode_steps=10, episode_stats=True)
    env.reset()
    for t in range(9):
        assert all("episode" not in info for info in env.step(a)[3])
    infos = env.step(a)[3]
    assert infos[1]["TimeLimit.truncated"] is True and infos[1]["episode"]["l"] == 10 and infos[1]["episode"]["r"] == 11.0


def test_sb3_adapter_default_infos_are_unchanged():
    hub = LedgerHub()
    env = wrappers.HubVecEnv(vec=hub)
    assert not hub.ledger_on and not env.episode_stats
    env.reset()
    a = np.zeros((4, 7), dtype=np.float32)
    for t in range(95):
        assert all(info == {} for info in env.step(a)[3])
    infos = env.step(a)[3]
    assert all(set(info) == {"terminal_observation", "TimeLimit.truncated"} for info in infos)


def test_recorded_ledgers_are_sequential_sums_and_the_penalty_comes_with_done():
    """in every env fixture the recorded cumulated_income IS the sequential f64 sum of the recorded per-step income since the reset (zero
    error: the GPU test may hold the device's sum to k addend bars), and test_penalty is first set at step 95, where done first fires"""
    files = sorted(glob.glob(os.path.join(orclib.GOLDEN_DIR, "env_*.npz")))
    assert len(files) == 24
    reached = 0
    for f in files:
        g = np.load(f)
        tn, an = list(g["telem_names"]), list(g["attr_names"])
        inc, cum, pen = g["telem"][:, tn.index("income")], g["attrs"][:, an.index("cumulated_income")], g["attrs"][:, an.index("test_penalty")]
        spe = int(g["steps_per_episode"])
        s = 0.0
        for k in range(len(inc)):
            s = (0.0 if k % spe == 0 else s) + inc[k]
            assert s == cum[k], (f, k)
        have = np.nonzero(~np.isnan(pen))[0]
        if len(have):
            reached += 1
            assert have[0] == 95 and bool(g["done"][95]) and not g["done"][:95].any(), f
        else:
            assert not g["done"].any(), f
    assert reached == 16
