"""CPU tests of per-env hub parameters (chub_create_params, include/chub.h): how VecChargingHub's kwargs become rows, the ctypes layout of
chub_env_params against the header, per-rank slicing of the sharded hosts, and the launch plan of a handle with rows (chub_launch_plan_params)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("hydro_prod_rate", "hydro_store_vlt", "init_soc", "fc_max_power", "fcev_permeate", "renew_fluctuate", "price_fluctuate", "hydro_loss")


def test_scalars_keep_the_homogeneous_path_and_any_sequence_selects_rows():
    from charginghub_env_amd import vec_env
    kw = dict(init_soc=0.3, hydro_loss=0.01, constant_charging=1)
    scalar, rows = vec_env.split_env_params(4, kw)
    assert rows is None and scalar == kw
    scalar, rows = vec_env.split_env_params(3, dict(init_soc=[0.2, 0.3, None], hydro_loss=0.01, hydro_prod_rate=None, constant_charging=1))
    assert scalar == dict(constant_charging=1)
    assert rows.shape == (3,) and rows.dtype.names == FIELDS
    assert rows["init_soc"].tolist() == [0.2, 0.3, 0.5]       # None -> the default
    assert rows["hydro_loss"].tolist() == [0.01] * 3           # a scalar broadcasts
    assert rows["hydro_prod_rate"].tolist() == [430.0] * 3     # None -> 430 (HYD:140-143), as make_config
    assert rows["hydro_store_vlt"].tolist() == [5000.0] * 3
    assert rows["fc_max_power"].tolist() == [100.0] * 3
    assert rows["fcev_permeate"].tolist() == [0.01] * 3
    # numpy arrays count as sequences, 0-d arrays as scalars
    _, rows = vec_env.split_env_params(2, dict(fcev_permeate=np.array([0.01, 1.5])))
    assert rows["fcev_permeate"].tolist() == [0.01, 1.5]
    assert vec_env.split_env_params(2, dict(fcev_permeate=np.float64(0.02)))[1] is None


@pytest.mark.parametrize("bad", [[0.5] * 3, [0.5] * 5, [[0.5, 0.5], [0.5, 0.5]], []])
def test_sequences_of_the_wrong_length_are_refused(bad):
    from charginghub_env_amd import vec_env
    with pytest.raises(ValueError, match="init_soc: expected a scalar or a sequence of n_envs = 4"):
        vec_env.split_env_params(4, dict(init_soc=bad))
    with pytest.raises(ValueError, match="init_soc: expected a scalar or a sequence of total_envs = 4"):
        vec_env.slice_env_kwargs(dict(init_soc=bad), 4, 0, 2)


def test_env_params_struct_matches_the_header():
    from charginghub_env_amd import _lib, vec_env
    hdr = open(os.path.join(ROOT, "include", "chub.h")).read()
    body = hdr[hdr.index("typedef struct chub_env_params"):hdr.index("} chub_env_params;")]
    assert tuple(re.findall(r"double\s+(\w+);", body)) == FIELDS == _lib.ENV_PARAM_FIELDS
    assert C.sizeof(_lib.ChubEnvParams) == 8 * len(FIELDS)
    assert vec_env.ENV_PARAMS_DTYPE.itemsize == C.sizeof(_lib.ChubEnvParams)
    for f in FIELDS:
        assert getattr(_lib.ChubEnvParams, f).offset == vec_env.ENV_PARAMS_DTYPE.fields[f][1], f
    # the same names and meanings as chub_config's eight scalars
    cfg = [n for n, _ in _lib.ChubConfig._fields_]
    assert cfg[-len(FIELDS):] == list(FIELDS)


def test_native_sharded_hub_slices_per_env_kwargs_by_rank():
    from charginghub_env_amd import multi_gpu

    class FakeComm(object):
        def __init__(self, rank, world):
            self.rank, self.world = rank, world

    class FakeShard(object):
        obs_dim, act_dim = 17, 47

    total, world = 12, 3
    kw = dict(station_list=[20, 25], station_type_list=["fast", "slow"], init_soc=[0.1 * (i % 9) + 0.1 for i in range(total)],
              hydro_loss=0.02, fcev_permeate=np.arange(total) * 0.01)
    seen = []
    for rank in range(world):
        h = multi_gpu.NativeShardedHub(total, kw, comm=FakeComm(rank, world), shard=lambda n, lo, tot, root: FakeShard())
        seen.append((h.env_id0, h.n_local))
        lo, n = h.env_id0, h.n_local
        assert h.hub_kwargs["init_soc"] == kw["init_soc"][lo:lo + n]
        assert list(h.hub_kwargs["fcev_permeate"]) == list(kw["fcev_permeate"][lo:lo + n])
        assert h.hub_kwargs["hydro_loss"] == 0.02 and h.hub_kwargs["station_list"] == [20, 25]
    assert sum(n for _, n in seen) == total and [lo for lo, _ in seen] == sorted(lo for lo, _ in seen)
    with pytest.raises(ValueError, match="total_envs = 12"):
        multi_gpu.NativeShardedHub(total, dict(init_soc=[0.5] * 10), comm=FakeComm(0, 2), shard=lambda n, lo, tot, root: FakeShard())


def test_torch_sharded_hub_slices_per_env_kwargs():
    pytest.importorskip("torch")
    from charginghub_env_amd import sharded

    class FakeEngine(object):
        obs_dim, act_dim = 17, 47

    kw = dict(init_soc=[0.2, 0.3, 0.4], price_fluctuate=0.1)
    h = sharded.ShardedChargingHub(3, kw, engine=lambda n, lo: FakeEngine())  # (no process group: one rank holds everything)
    assert (h.env_id0, h.n_local) == (0, 3)
    assert h.hub_kwargs == dict(init_soc=[0.2, 0.3, 0.4], price_fluctuate=0.1)
    with pytest.raises(ValueError, match="total_envs = 3"):
        sharded.ShardedChargingHub(3, dict(init_soc=[0.2]), engine=lambda n, lo: FakeEngine())


def _plan(fn, cfg, n, rng, opt=None):
    from charginghub_env_amd import _lib
    out = (C.c_int32 * 16)()
    rc = fn(C.byref(cfg), n, rng, C.byref(opt) if opt is not None else None, out)
    return rc, list(out)


def test_launch_plan_params_runs_the_two_launch_step():
    """chub_launch_plan_params: the plan chub_launch_plan reports, without the one-launch step and chub_run_steps's spans, for PHILOX and
    PHILOX_CURVES at every size; COMPAT: one kernel per station at every size"""
    import charginghub_env_amd as chub
    from charginghub_env_amd import _lib
    lib = _lib.load_library()
    cfg = chub.make_config([20, 25], ["fast", "slow"])
    ONE, SPAN_OK, PIPED = 6, 7, 8
    for rng in (_lib.RNG_PHILOX, _lib.RNG_PHILOX_CURVES):
        for n in (1, 64, 1000, 20000, 65536, 262144):
            for fused in (0, 1, 2):
                opt = _lib.ChubOptions()
                opt.fused_step = fused
                rc0, base = _plan(lib.chub_launch_plan, cfg, n, rng, opt)
                rc1, got = _plan(lib.chub_launch_plan_params, cfg, n, rng, opt)
                assert rc1 == rc0, (rng, n, fused, lib.chub_last_error())
                if rc0 != 0:
                    continue
                assert got[ONE] == 0 and got[SPAN_OK] == 0 and got[PIPED] == 0, (rng, n, fused)
                keep = [i for i in range(16) if i not in (ONE, SPAN_OK, PIPED)]
                assert [got[i] for i in keep] == [base[i] for i in keep], (rng, n, fused)
    COMPAT_SMALL, COMPAT, SPLIT2, WALK_AHEAD = 10, 11, 12, 13
    for n in (1, 8, 64, 1000, 40000, 65536):
        for slot_kernel in (0, 1):
            opt = _lib.ChubOptions()
            opt.slot_kernel = slot_kernel
            rc0, base = _plan(lib.chub_launch_plan, cfg, n, _lib.RNG_COMPAT, opt)
            rc1, got = _plan(lib.chub_launch_plan_params, cfg, n, _lib.RNG_COMPAT, opt)
            assert rc0 == rc1 == 0
            assert got[COMPAT] == 1 and got[COMPAT_SMALL] == 0 and got[SPLIT2] == 0 and got[WALK_AHEAD] == 0 and got[ONE] == 0, (n, got)
            assert got[14:16] == base[14:16]  # (the station kernels of that form)
    assert _plan(lib.chub_launch_plan, cfg, 1000, _lib.RNG_COMPAT)[1][COMPAT] != 1  # (homogeneous: the split step)
    # the homogeneous plan is untouched: small PHILOX batches still take the one-launch step there
    assert _plan(lib.chub_launch_plan, cfg, 1000, _lib.RNG_PHILOX)[1][ONE] != 0


def test_create_params_validates_rows_before_any_device_call():
    """a bad row is refused with chub_create's code and message plus the env index, GPU or not (the rows are checked before the data files
    and the device are opened)"""
    import charginghub_env_amd as chub
    from charginghub_env_amd import _lib
    lib = _lib.load_library()
    cfg = chub.make_config([20, 25], ["fast", "slow"])
    n = 8
    rows = (_lib.ChubEnvParams * n)()
    for r in rows:
        r.hydro_prod_rate, r.hydro_store_vlt, r.init_soc, r.fc_max_power, r.fcev_permeate = 430.0, 5000.0, 0.5, 100.0, 0.01
    rows[5].init_soc = 1.5
    h = C.c_void_p()
    rc = lib.chub_create_params(C.byref(cfg), b"/nonexistent", n, 0, 0, 0, _lib.RNG_PHILOX, None, rows, C.byref(h))
    assert rc == -1 and lib.chub_last_error() == b"init_soc must be in [0.1, 1] (env 5)"
    rows[5].init_soc = 0.5
    rows[2].fc_max_power = -1.0
    rc = lib.chub_create_params(C.byref(cfg), b"/nonexistent", n, 0, 0, 0, _lib.RNG_PHILOX, None, rows, C.byref(h))
    assert rc == -1 and lib.chub_last_error() == b"hydrogen system sizes must be non-negative (env 2)"
    rows[2].fc_max_power = 100.0
    rc = lib.chub_create_params(C.byref(cfg), b"/nonexistent", n, 0, 0, 0, _lib.RNG_COMPAT, None, rows, C.byref(h))
    assert rc == -2 and not h.value  # (COMPAT takes rows too: the data files come next)
    # cfg's own scalars are ignored: an invalid one does not matter once rows are given
    cfg.init_soc = 0.0
    rc = lib.chub_create_params(C.byref(cfg), b"/nonexistent", n, 0, 0, 0, _lib.RNG_PHILOX, None, rows, C.byref(h))
    assert rc == -2 and not h.value  # (the data files come next)
    assert lib.chub_create_params(C.byref(cfg), b"/nonexistent", n, 0, 0, 0, _lib.RNG_PHILOX, None, None, C.byref(h)) == -1
