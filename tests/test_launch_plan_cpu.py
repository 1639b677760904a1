"""CPU tests of the launch plan (chub_launch_plan, csrc/chub_plan.h): which launch forms a handle of a given hub shape, batch, RNG
mode and chub_options runs -- the decisions chub_create_ex makes through the same code, without a device.  Every size threshold is
checked on both sides of its boundary; the expected values are worked out by hand from the thresholds, not recomputed from them."""
import ctypes as C
import os
import re

import pytest

import orclib

ROOT = orclib.ROOT

# the CHUB_PLAN_* indices of include/chub.h, in order
FIELDS = ["packed", "big_tile", "pblock", "pslots", "epb", "xcd", "one_launch", "span_size_ok", "span_piped", "span_steps",
          "compat_small", "compat", "split2", "walk_ahead", "station0", "station1"]
# values: packed 0 none, 1 small tile, 2 small tile + stations > 64 piles, 3 large tile, 4 large tile + stations > 64 piles;
# one_launch 0 none, 1 k_step_fused, 2 k_step_tailwave; compat 0 PHILOX, 1 per station, 2 split, 3 split + k_slot_walk2<.., 32>, 4 ... 64;
# station 0 k_slot, 1 k_slot_unit, 2 k_slot_unit_any, 3 k_slot_curves


def lib_and_mod():
    import charginghub_env_amd as m
    from charginghub_env_amd import _lib
    return m.load_library(), m, _lib


def plan_rc(stations, n_envs, rng="philox", **options):
    lib, m, _lib = lib_and_mod()
    cfg = m.make_config(list(stations), ["fast", "slow"])
    opt = _lib.ChubOptions()
    for k, v in options.items():
        setattr(opt, k, v)
    out = (C.c_int32 * len(FIELDS))()
    rc = lib.chub_launch_plan(C.byref(cfg), n_envs, _lib.RNG_MODES[rng], C.byref(opt), out)
    return rc, dict(zip(FIELDS, out)), lib.chub_last_error()


def plan(stations, n_envs, rng="philox", **options):
    rc, p, err = plan_rc(stations, n_envs, rng, **options)
    assert rc == 0, err
    return p


def test_plan_fields_are_the_headers_list():
    hdr = open(os.path.join(ROOT, "include", "chub.h")).read()
    body = re.search(r"enum \{\s*CHUB_PLAN_PACKED = 0,(.*?)\};", hdr, flags=re.S).group(0)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\bCHUB_PLAN_(\w+)", body)
    assert names == [f.upper() for f in FIELDS] + ["COUNT"]


def test_default_hub_small_batch():
    # [20, 25]: 45 piles, 512 // 45 = 11 envs per workgroup of the small tile
    assert plan([20, 25], 1024) == dict(packed=1, big_tile=0, pblock=256, pslots=2, epb=11, xcd=1, one_launch=2, span_size_ok=1, span_piped=1,
                                        span_steps=0, compat_small=0, compat=0, split2=0, walk_ahead=0, station0=0, station1=0)


@pytest.mark.parametrize("n_envs, one_launch", [(8448, 2), (8449, 0)])  # 768 workgroups of 11 envs for k_step_tailwave
def test_one_launch_step_threshold(n_envs, one_launch):
    assert plan([20, 25], n_envs)["one_launch"] == one_launch


@pytest.mark.parametrize("n_envs, ok", [(4224, 1), (4225, 0)])  # 384 workgroups
def test_span_size_threshold(n_envs, ok):
    assert plan([20, 25], n_envs)["span_size_ok"] == ok


@pytest.mark.parametrize("n_envs, piped", [(2816, 1), (2817, 0)])  # 256 workgroups
def test_piped_span_threshold(n_envs, piped):
    assert plan([20, 25], n_envs)["span_piped"] == piped


@pytest.mark.parametrize("n_envs, xcd", [(139810, 1), (139811, 0)])  # 6 Mi charger slots: 139 810 x 45 = 6 291 450, 139 811 x 45 = 6 291 495
def test_xcd_order_threshold(n_envs, xcd):
    assert plan([20, 25], n_envs)["xcd"] == xcd


@pytest.mark.parametrize("n_envs, tile", [(233016, (1, 0, 256, 2, 11)), (233017, (3, 1, 512, 4, 45))])  # 10 Mi slots: 10 485 720 / 10 485 765
def test_large_tile_threshold(n_envs, tile):
    p = plan([20, 25], n_envs)
    assert (p["packed"], p["big_tile"], p["pblock"], p["pslots"], p["epb"]) == tile
    assert p["one_launch"] == 0 and p["xcd"] == 0


@pytest.mark.parametrize("n_envs, one_launch, span_ok", [(28032, 1, 1), (28033, 0, 0)])
def test_hub_of_fewer_than_8_piles_takes_k_step_fused(n_envs, one_launch, span_ok):
    # [3, 4]: 7 piles, 512 // 7 = 73 envs per workgroup (more than the tail wave's 64 lanes): k_step_fused up to 384 workgroups = 28 032 envs
    p = plan([3, 4], n_envs)
    assert (p["epb"], p["one_launch"], p["span_size_ok"], p["span_piped"]) == (73, one_launch, span_ok, 0)


def test_hub_of_more_than_512_piles_takes_the_large_tile_at_any_batch():
    p = plan([300, 270], 1)
    assert (p["packed"], p["big_tile"], p["epb"], p["one_launch"], p["station0"], p["station1"]) == (4, 1, 3, 0, 2, 2)
    assert plan([300, 270], 1024)["packed"] == 4
    assert plan([300, 270], 1024, tile=1)["packed"] == 0  # 570 piles do not fit the small tile's 512 lanes


@pytest.mark.parametrize("stations, packed", [([300, 314], 4), ([300, 315], 0), ([300, 326], 0), ([300, 329], 0), ([300, 330], 4)])
def test_lanes_the_reciprocal_cannot_divide_are_not_packed(stations, packed):
    # the packed kernel divides lane numbers by S0 + S1 with a 20-bit reciprocal: on the 2048 lanes of the large tile it fails for 615, 626, 629 ...
    assert plan(stations, 64)["packed"] == packed


@pytest.mark.parametrize("n_envs, packed", [(5711392, 3), (5711393, 0)])  # (45 + 2) x 16 bytes per env below 2^32: 5 711 392 x 752 = 4 294 966 784
def test_32_bit_offset_limit(n_envs, packed):
    assert plan([20, 25], n_envs)["packed"] == packed


@pytest.mark.parametrize("stations, kernels, packed", [([64, 64], (0, 0), 1), ([64, 65], (0, 1), 2), ([256, 257], (1, 2), 4), ([257, 1], (2, 0), 2)])
def test_station_kernels(stations, kernels, packed):
    p = plan(stations, 16)
    assert (p["station0"], p["station1"], p["packed"]) == kernels + (packed,)
    p = plan(stations, 16, slot_kernel=1)
    assert (p["station0"], p["station1"], p["packed"], p["one_launch"]) == kernels + (0, 0)


@pytest.mark.parametrize("n_envs, small, compat", [(8, 1, 2), (9, 0, 3)])
def test_compat_small_fit(n_envs, small, compat):
    # [20, 25]: units of 20 and 25 lanes -> min(64, 3 x (64 // 20), 4 x (64 // 25)) = min(64, 9, 8) = 8 envs in k_compat_small's workgroup
    p = plan([20, 25], n_envs, "compat")
    assert (p["compat_small"], p["compat"], p["split2"], p["walk_ahead"], p["packed"], p["one_launch"]) == (small, compat, 1, 1, 0, 0)


def test_compat_small_fit_of_small_units():
    # [2, 3]: min(64, 3 x 32, 4 x 21) = 64
    assert plan([2, 3], 64, "compat")["compat_small"] == 1
    assert plan([2, 3], 65, "compat")["compat_small"] == 0


@pytest.mark.parametrize("stations, split2, compat", [([7, 20], 0, 2), ([8, 20], 1, 3), ([20, 7], 0, 2), ([64, 8], 1, 3)])
def test_split2_needs_units_of_8_lanes(stations, split2, compat):
    p = plan(stations, 1024, "compat")
    assert (p["split2"], p["compat"]) == (split2, compat)


@pytest.mark.parametrize("n_envs, compat", [(40000, 3), (40001, 4)])
def test_walk2_envs_per_walk_workgroup(n_envs, compat):
    assert plan([20, 25], n_envs, "compat")["compat"] == compat


def test_compat_options():
    p = plan([20, 25], 1024, "compat", walk_ahead=1)
    assert (p["compat"], p["split2"], p["walk_ahead"]) == (2, 1, 0)
    p = plan([20, 25], 1024, "compat", slot_kernel=1)
    assert (p["compat"], p["split2"], p["walk_ahead"]) == (1, 0, 0)
    p = plan([20, 25], 1, "compat", slot_kernel=1)  # the drop-in class keeps its one launch; its other calls go per station
    assert (p["compat_small"], p["compat"]) == (1, 1)
    assert plan([20, 25], 1, "compat", fused_step=1)["compat_small"] == 0
    p = plan([65, 20], 1, "compat")  # a unit of more than one wave: neither k_compat_small nor the split form
    assert (p["compat_small"], p["compat"], p["station0"], p["station1"]) == (0, 1, 1, 0)


def test_philox_curves():
    p = plan([20, 25], 1024, "philox_curves")
    assert (p["packed"], p["one_launch"], p["compat"], p["station0"], p["station1"]) == (0, 0, 0, 3, 3)
    rc, _, err = plan_rc([65, 20], 4, "philox_curves")
    assert rc == -4 and b"PHILOX_CURVES covers stations of at most 64 piles" in err


def test_every_option_value():
    base = plan([20, 25], 1024)
    for field, values in (("slot_kernel", (0, 2)), ("work_order", (0,)), ("walk_ahead", (0, 1)), ("span_tails", (0,)), ("tile", (0,)), ("fused_step", (0,))):
        for v in values:
            assert plan([20, 25], 1024, **{field: v}) == base, (field, v)
    assert plan([20, 25], 1024, slot_kernel=1)["packed"] == 0
    assert plan([20, 25], 1024, work_order=1)["xcd"] == 0
    assert plan([20, 25], 1024, span_tails=1)["span_piped"] == 0
    assert plan([20, 25], 1024, fused_step=1)["one_launch"] == 0
    assert plan([20, 25], 1024, fused_step=1)["span_size_ok"] == 1
    p = plan([20, 25], 100000, fused_step=2)  # forced: 9091 workgroups
    assert (p["one_launch"], p["span_size_ok"], p["span_piped"]) == (2, 1, 0)
    assert plan([20, 25], 1024, span_tails=2, span_steps=5)["span_piped"] == 1
    for v in (0, 1, 96):
        assert plan([20, 25], 1024, span_steps=v)["span_steps"] == v
    p = plan([20, 25], 1024, tile=1)
    assert (p["packed"], p["big_tile"], p["xcd"], p["one_launch"]) == (1, 0, 1, 2)
    p = plan([20, 25], 1024, tile=2)
    assert (p["packed"], p["big_tile"], p["epb"], p["xcd"], p["one_launch"], p["span_piped"]) == (3, 1, 45, 0, 0, 0)
    assert plan([20, 25], 233017, tile=1)["packed"] == 1


def test_refusals():
    rc, _, err = plan_rc([20, 25], 8, tile=2, fused_step=2)  # the single-launch step runs on the small tile
    assert rc == -4 and b"fused_step = 2: the single-launch step covers" in err
    rc, _, err = plan_rc([20, 25], 8, "compat", fused_step=2)
    assert rc == -4 and b"fused_step = 2" in err
    rc, _, err = plan_rc([20, 25], 8449, span_tails=2)  # no one-launch step at this size
    assert rc == -4 and b"span_tails = 2" in err
    rc, _, err = plan_rc([3, 4], 8, span_tails=2)  # 73 envs per workgroup: more than the tail wave's lanes
    assert rc == -4 and b"span_tails = 2: the tail wave of a span covers" in err
    for field, bad in (("slot_kernel", 3), ("fused_step", -1), ("tile", 3), ("walk_ahead", 2), ("work_order", 2), ("span_steps", 97), ("span_tails", 3)):
        rc, _, err = plan_rc([20, 25], 8, **{field: bad})
        assert rc == -1 and ("chub_options." + field).encode() in err, (field, err)
    rc, _, err = plan_rc([20, 25], 0)
    assert rc == -1 and b"n_envs must be positive" in err
    rc, _, err = plan_rc([0, 0], 8)
    assert rc == -1 and b"must have fast pile or slow pile" in err
    rc, _, err = plan_rc([4097, 1], 8)
    assert rc == -4 and b"4096 piles" in err
    lib, m, _lib = lib_and_mod()
    out = (C.c_int32 * len(FIELDS))()
    assert lib.chub_launch_plan(C.byref(m.make_config([20, 25], ["fast", "slow"])), 8, 3, None, out) == -1
    assert lib.chub_launch_plan(None, 8, 1, None, out) == -1
