"""The step terms (include/chub.h: chub_get_step_terms_device) without a device: the five entry points declared, exported and bound,
chub_get_step_terms_size and the name -> mask helpers, null handles -- and tests/step_terms_lib.py's numpy definition held to the
reference: every golden fixture replayed through the CPU oracle, the definition applied to the oracle's telemetry after each step and
compared with the attributes the unmodified reference class carried after that step."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import charginghub_env_amd as chub
import orclib
import step_terms_lib as stl
from charginghub_env_amd import _lib, wrappers
from orclib import OrcEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = stl.ALL
ST = _lib.ST
RTOL, ATOL = 1e-11, 1e-9  # what tests/test_oracle_golden.py holds the oracle's telemetry to on the same fixtures


# ---- 1. the ABI without a device
def test_fields_are_one_list():
    hdr = open(os.path.join(ROOT, "include", "chub.h")).read()
    body = hdr[hdr.index("CHUB_ST_REWARD = 0"):hdr.index("CHUB_ST_COUNT\n")]
    cols = tuple(c.lower() for c in re.findall(r"\bCHUB_ST_([A-Z0-9_]+)", body))
    assert cols == _lib.ST_NAMES and len(cols) == _lib.ST_COUNT == 27
    assert [ST[n] for n in _lib.ST_NAMES] == list(range(27))
    assert (ST["reward"], ST["grid_draw"], ST["gen_hy"], ST["soc_deviation"], ST["soc_penalty"]) == (0, 11, 16, 25, 26)


def test_symbols_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chub.h")).read(), flags=re.S)
    assert re.search(r"^int chub_get_step_terms_size\(uint32_t fields\);", header, re.M)
    assert re.search(r"^int chub_get_step_terms_device\(chub_env \*env, uint32_t fields, const uint8_t \*d_mask, float \*d_out, void \*stream\);",
                     header, re.M)
    assert re.search(r"^int chub_get_step_terms\(chub_env \*env, uint32_t fields, double \*out\);", header, re.M)
    assert re.search(r"^int chub_set_step_terms\(chub_env \*env, uint32_t fields, float \*d_out\);", header, re.M)
    assert re.search(r"^int chub_get_step_terms_attached\(const chub_env \*env\);", header, re.M)
    lib = _lib.load_library()
    for name, n_args in (("chub_get_step_terms_size", 1), ("chub_get_step_terms_device", 5), ("chub_get_step_terms", 3), ("chub_set_step_terms", 3),
                         ("chub_get_step_terms_attached", 1)):
        assert name in _lib.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args
    for method in ("step_terms", "step_terms_device", "attach_step_terms", "detach_step_terms"):
        assert callable(getattr(chub.VecChargingHub, method))
    assert callable(wrappers.TorchHubVecEnv.step_terms)


def test_size_values_and_error_codes():
    lib = _lib.load_library()
    assert lib.chub_get_step_terms_size(0) == -1 and "CHUB_ST" in lib.chub_last_error().decode()
    for bad in (1 << 27, ALL | 1 << 27, 1 << 31, 0xFFFFFFFF):
        assert lib.chub_get_step_terms_size(bad) == -1
    assert lib.chub_get_step_terms_size(ALL) == 27 and lib.chub_get_step_terms_size(1) == 1 and lib.chub_get_step_terms_size(1 << 26) == 1
    for mask in list(range(1, 1 << 27, 999983)) + [1 << f for f in range(27)]:
        assert lib.chub_get_step_terms_size(mask) == bin(mask).count("1") == len(_lib.st_fields_names(mask))


def test_null_handles_and_outputs_are_refused():
    lib = _lib.load_library()
    f = C.c_void_p(8)  # never dereferenced: the checks come first
    for call in (lambda: lib.chub_get_step_terms_device(None, ALL, None, f, None), lambda: lib.chub_get_step_terms_device(f, ALL, None, None, None),
                 lambda: lib.chub_get_step_terms(None, ALL, f), lambda: lib.chub_get_step_terms(f, ALL, None)):
        assert call() == -1 and lib.chub_last_error().decode() == "null argument"
    for call in (lambda: lib.chub_set_step_terms(None, ALL, f), lambda: lib.chub_set_step_terms(None, 0, None),
                 lambda: lib.chub_get_step_terms_attached(None)):
        assert call() == -1 and lib.chub_last_error().decode() == "null handle"


def test_names_translate_to_masks():
    m = _lib.st_fields_mask
    assert m(None) == ALL and m(_lib.ST_NAMES) == ALL
    three = 1 << 10 | 1 << 12 | 1 << 26
    assert m(("not_meet_loss", "grid_excess", "soc_penalty")) == three == m(["soc_penalty", "grid_excess", "not_meet_loss", "grid_excess"])
    assert m("reward") == 1 and m(three) == three and m(np.uint32(5)) == 5
    assert _lib.st_fields_names(three) == ("not_meet_loss", "grid_excess", "soc_penalty") and _lib.st_fields_names(ALL) == _lib.ST_NAMES
    for bad in (("reward", "profit"), "REWARD", ["income_evs"], ("",)):
        with pytest.raises(ValueError, match="unknown step term"):
            m(bad)
    for bad in (0, 1 << 27, -1, ()):
        with pytest.raises(ValueError):
            m(bad)
    assert stl.cols_of(three) == [10, 12, 26]


def test_torch_adapter_rejects_unknown_names_before_it_builds_anything():
    pytest.importorskip("torch")
    with pytest.raises(ValueError, match="unknown step term"):
        wrappers.TorchHubVecEnv(4, [20, 25], ["fast", "slow"], step_terms=("reward", "profit"))


# ---- 2. the definition
def test_definition_on_a_made_row():
    """one env, every column a different number: each term is the table's expression, evaluated here a second time in plain Python"""
    tel = np.arange(1, 39, dtype=np.float64)[None, :] * 1.25
    tel[0, _lib.T["Store_SOC"]] = 0.35
    init_soc, vlt = 0.2, 25.0
    cap_mass = float(stl.cap_mass_of(vlt))
    assert cap_mass == (0.089 * 200) * 25000.0
    got = stl.terms(tel, init_soc, cap_mass)[0]
    t = {name: float(tel[0, i]) for name, i in _lib.T.items()}
    p = t["price_now"] / 4
    draw = (t["ev_power_0_net"] + t["ev_power_1_net"]) + t["re_hydrogen_power"]
    dev = abs(t["Store_SOC"] - init_soc)
    want = [t["reward"], t["income"], 0.42 / 4 * t["charge_power_0"], 0.21 / 4 * t["charge_power_1"], -p * t["ev_power_0_net"],
            -p * t["ev_power_1_net"], 0.8 * (t["flow_in_0"] + t["flow_in_1"]), 6 / 1000 * t["hy_use"], -p * t["re_hydrogen_power"],
            -6 / 1000 * t["hy_to_use"], -10 / 1000 * t["not_meet"], draw, max(draw - 2000, 0), t["re_used_renew"], t["fc_power"], t["hy_act"],
            1.0 if t["hy_flow_speed"] > 0.5 else 0.0, 15 * 60 * t["hy_flow_speed"], t["hy_use"], t["not_meet"], t["hy_to_use"],
            t["total_mass_need"], t["fcev_arrive_number"], t["fcev_line"], t["fcev_queue_len"], dev, abs(dev * cap_mass / 1000 / 0.2)]
    assert got.tolist() == want
    # the grid excess is positive only beyond the 2000 kW limit, GEN_HY switches above 0.5 exactly, per-env arrays broadcast
    tel2 = np.repeat(tel, 3, axis=0)
    tel2[:, _lib.T["ev_power_0_net"]] = [100.0, 1990.0, 3000.0]
    tel2[:, _lib.T["hy_flow_speed"]] = [0.5, 0.5000001, 0.0]
    g2 = stl.terms(tel2, np.array([0.2, 0.35, 0.5]), stl.cap_mass_of([25.0, 50.0, 5000.0]))
    assert g2[0, ST["grid_excess"]] == 0 and g2[2, ST["grid_excess"]] == g2[2, ST["grid_draw"]] - 2000 > 0
    assert g2[:, ST["gen_hy"]].tolist() == [0.0, 1.0, 0.0]
    assert g2[1, ST["soc_deviation"]] == 0 and g2[1, ST["soc_penalty"]] == 0
    assert g2[2, ST["soc_penalty"]] == abs(abs(0.35 - 0.5) * float(stl.cap_mass_of(5000.0)) / 1000 / 0.2)


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.allclose(a, b, rtol=RTOL, atol=ATOL), (what, a, b, np.abs(a - b).max())


def _check_fixture(name):
    g = orclib.load_golden(name)
    cfg = orclib.golden_config(g)
    steps = int(g["steps_per_episode"])
    seeds = {int(ep): (int(a), int(b)) for ep, a, b in g["seeds"]} if g["seeds"].size else {}
    env = OrcEnv(cfg, ctor_seeds=tuple(int(x) for x in g["ctor_seeds"]))
    env.reset(g["ctor_days"], g["ctor_z"])
    init_soc, cap_mass = float(g["kw_init_soc"]), float(stl.cap_mass_of(float(g["kw_hydro_store_vlt"])))
    names = [str(x) for x in g["attr_names"]]
    i, seen_penalty, last_penalty = 0, 0, None
    for ep in range(int(g["episodes"])):
        if ep in seeds:
            env.seed_compat(*seeds[ep])
        env.reset(g["reset_days"][ep], g["reset_z"][ep])
        draw = 0.0
        for t in range(steps):
            _, r, done = env.step(g["action"][i], g["exo_z"][i])
            x = stl.terms(env.telemetry()[None, :], init_soc, cap_mass)[0]
            at = dict(zip(names, g["attrs"][i]))
            what = (name, ep, t)
            _close([x[ST["income_evs0"]], x[ST["income_evs1"]], x[ST["cost_evs0"]], x[ST["cost_evs1"]], x[ST["income_serve"]],
                    x[ST["income_hys"]], x[ST["hy_cost"]], x[ST["hy_gen"]], x[ST["gen_hy"]], x[ST["hy_for_fc"]], x[ST["soc_deviation"]],
                    x[ST["cost_evs0"]] + x[ST["cost_evs1"]]],
                   [at["re_income_evs_list_0"], at["re_income_evs_list_1"], at["re_income_evs_cost_list_0"], at["re_income_evs_cost_list_1"],
                    at["re_income_evs_serve"], at["re_income_hys"], at["re_hy_cost"], at["re_hy_gen"], at["gen_hy"], at["re_hy_for_fc"],
                    at["deviation"], at["re_income_evs_cost"]], what)
            draw += x[ST["grid_draw"]]  # (the running sum since the reset: MGR:262, zeroed by reset() alone)
            _close(draw, at["cumulated_draw_ele"], what + ("cumulated_draw_ele",))
            _close(x[ST["reward"]], g["reward"][i], what + ("reward",))
            # test_penalty is an attribute the reference assigns only in the step whose `done` fires (MGR:275-290) and keeps until the next
            # such step: NaN before the first, fresh where done, stale in between (the fixtures that step on past `done`).  SOC_PENALTY is
            # the same expression "as if the day ended now", so it is compared where the attribute is fresh; in between the attribute
            # still holds the last fresh value
            if not np.isnan(at["test_penalty"]):
                if done:
                    _close(x[ST["soc_penalty"]], at["test_penalty"], what + ("test_penalty",))
                    last_penalty = at["test_penalty"]
                    seen_penalty += 1
                else:
                    assert at["test_penalty"] == last_penalty, what
            else:
                assert not done and last_penalty is None, what
            assert x[ST["grid_excess"]] == max(x[ST["grid_draw"]] - 2000, 0) and x[ST["soc_penalty"]] >= 0
            i += 1
    assert i == g["attrs"].shape[0]
    if steps >= 96:
        assert seen_penalty >= 1, name


@pytest.mark.parametrize("name", orclib.GOLDEN_ENV)
def test_definition_matches_the_reference_attributes(name):
    _check_fixture(name)


@pytest.mark.parametrize("name", orclib.GOLDEN_ENV_BIG)
def test_definition_matches_the_reference_attributes_on_stations_of_more_than_256_piles(name):
    with orclib.big_oracle():
        _check_fixture(name)
