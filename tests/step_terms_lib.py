"""The step terms (include/chub.h: chub_get_step_terms_device) as a numpy definition (TEST INFRASTRUCTURE): the table of the header over a
telemetry block [N, 38], in f64 in the order written there.  tests/test_step_terms_cpu.py holds it to the reference's recorded
attributes; tests/test_gpu_step_terms.py holds the kernel to it bit for bit."""
import numpy as np

from charginghub_env_amd import _lib

T, ST = _lib.T, _lib.ST
ALL = (1 << _lib.ST_COUNT) - 1


def cap_mass_of(vlt):
    return (0.089 * (200 / 1)) * (np.asarray(vlt, dtype=np.float64) * 1000)  # env.py: _capacity_mass (HYD:92-100)


def terms(tel, init_soc, cap_mass):
    """tel [N, 38] f64 (chub_get_telemetry's layout) -> [N, 27] f64 in the order of _lib.ST_NAMES; init_soc and cap_mass scalars or [N]"""
    tel = np.asarray(tel, dtype=np.float64)
    c = lambda name: tel[:, T[name]]
    p = c("price_now") / 4
    out = np.zeros((tel.shape[0], _lib.ST_COUNT))
    out[:, ST["reward"]] = c("reward")
    out[:, ST["income"]] = c("income")
    out[:, ST["income_evs0"]] = 0.42 / 4 * c("charge_power_0")
    out[:, ST["income_evs1"]] = 0.21 / 4 * c("charge_power_1")
    out[:, ST["cost_evs0"]] = -p * c("ev_power_0_net")
    out[:, ST["cost_evs1"]] = -p * c("ev_power_1_net")
    out[:, ST["income_serve"]] = 0.8 * (c("flow_in_0") + c("flow_in_1"))
    out[:, ST["income_hys"]] = 6 / 1000 * c("hy_use")
    out[:, ST["hy_cost"]] = -p * c("re_hydrogen_power")
    out[:, ST["hy_loss"]] = -6 / 1000 * c("hy_to_use")
    out[:, ST["not_meet_loss"]] = -10 / 1000 * c("not_meet")
    draw = (c("ev_power_0_net") + c("ev_power_1_net")) + c("re_hydrogen_power")
    out[:, ST["grid_draw"]] = draw
    out[:, ST["grid_excess"]] = np.maximum(draw - 2000, 0)
    out[:, ST["used_renew"]] = c("re_used_renew")
    out[:, ST["fc_power"]] = c("fc_power")
    out[:, ST["hy_act"]] = c("hy_act")
    out[:, ST["gen_hy"]] = np.where(c("hy_flow_speed") > 0.5, 1.0, 0.0)
    out[:, ST["hy_gen"]] = 15 * 60 * c("hy_flow_speed")
    out[:, ST["hy_use"]] = c("hy_use")
    out[:, ST["not_meet"]] = c("not_meet")
    out[:, ST["hy_for_fc"]] = c("hy_to_use")
    out[:, ST["mass_need"]] = c("total_mass_need")
    out[:, ST["fcev_arrive"]] = c("fcev_arrive_number")
    out[:, ST["fcev_line"]] = c("fcev_line")
    out[:, ST["fcev_queue"]] = c("fcev_queue_len")
    dev = np.abs(c("Store_SOC") - init_soc)
    out[:, ST["soc_deviation"]] = dev
    out[:, ST["soc_penalty"]] = np.abs(dev * cap_mass / 1000 / 0.2)
    return out


def cols_of(fields):
    mask = _lib.st_fields_mask(fields)
    return [f for f in range(_lib.ST_COUNT) if mask >> f & 1]
