"""ctypes binding of include/chub.h.  Fails loudly when libchub.so is missing -- there is no fallback."""
import ctypes as C
import os

# kernel arguments in device memory (read by every wave's first scalar loads); only effective when set before the
# HIP runtime initialises, harmless otherwise
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

_HERE = os.path.dirname(os.path.abspath(__file__))
DATA_DIR = os.path.join(_HERE, "data")

CHUB_FAST, CHUB_SLOW = 0, 1
RNG_COMPAT, RNG_PHILOX, RNG_PHILOX_CURVES = 0, 1, 2
RNG_MODES = {"compat": RNG_COMPAT, "philox": RNG_PHILOX, "philox_curves": RNG_PHILOX_CURVES}
T_COUNT = 38
TELEMETRY_NAMES = ["hy_act", "hy_flow_speed", "all_power_second", "Store_SOC", "capacity", "total_mass_need", "hy_use",
                   "not_meet", "fc_power", "hy_to_use", "re_used_renew", "re_ev_power_0", "re_ev_power_1",
                   "re_hydrogen_power", "income", "reward", "re_pv_power", "re_wd_power", "price_next",
                   "fcev_arrive_number", "fcev_line", "fcev_queue_len", "pv_day", "wd_day",
                   "ev_power_0_net", "ev_power_1_net", "ev_power_sum_net", "price_now",
                   "min_power_0", "charge_power_0", "max_power_0", "line_0", "flow_in_0",
                   "min_power_1", "charge_power_1", "max_power_1", "line_1", "flow_in_1"]
T = {name: i for i, name in enumerate(TELEMETRY_NAMES)}
# the columns of the per-episode ledger (the CHUB_EP_* enum of include/chub.h, in order)
EPISODE_NAMES = ["return", "income", "draw_ele", "length", "deviation", "test_penalty", "end_soc"]
EP_COUNT = len(EPISODE_NAMES)
EP = {name: i for i, name in enumerate(EPISODE_NAMES)}
# the per-pile columns of chub_pile_obs_device (the CHUB_PILE_* enum of include/chub.h, in order: chub_get_slots' nine fields)
PILE_NAMES = ("car", "charge", "emergency", "power", "soc", "init_soc", "target_soc", "stay_time", "already_stay_time")
PILE_COUNT = len(PILE_NAMES)
PILE = {name: i for i, name in enumerate(PILE_NAMES)}


def pile_fields_mask(fields=None):
    """a field set of chub_pile_obs_device as its bit mask: None = all nine, an int = the mask itself, else a sequence of PILE_NAMES"""
    if fields is None:
        return (1 << PILE_COUNT) - 1
    if hasattr(fields, "__index__"):  # (an int of any kind)
        fields = fields.__index__()
        if fields <= 0 or fields >> PILE_COUNT:
            raise ValueError("fields: a non-empty mask over the %d per-pile fields, got %#x" % (PILE_COUNT, fields))
        return fields
    if isinstance(fields, str):
        fields = (fields,)
    mask = 0
    for name in fields:
        if name not in PILE:
            raise ValueError("unknown per-pile field %r (one of %s)" % (name, ", ".join(PILE_NAMES)))
        mask |= 1 << PILE[name]
    if not mask:
        raise ValueError("fields: at least one per-pile field")
    return mask


def pile_fields_names(mask):
    """the columns a mask selects, in the order they come out (ascending field order)"""
    return tuple(name for i, name in enumerate(PILE_NAMES) if mask >> i & 1)



# the columns of chub_station_profile_device (the CHUB_SP_* enum of include/chub.h, in order)
SP_NAMES = ("cars", "charging", "must_charge", "power", "power_charging", "emergency", "soc_gap")
SP_COUNT = len(SP_NAMES)
SP = {name: i for i, name in enumerate(SP_NAMES)}


def sp_fields_mask(fields=None):
    """a field set of chub_station_profile_device as its bit mask: None = all seven, an int = the mask itself, else a sequence of SP_NAMES"""
    if fields is None:
        return (1 << SP_COUNT) - 1
    if hasattr(fields, "__index__"):  # (an int of any kind)
        fields = fields.__index__()
        if fields <= 0 or fields >> SP_COUNT:
            raise ValueError("fields: a non-empty mask over the %d station-profile fields, got %#x" % (SP_COUNT, fields))
        return fields
    if isinstance(fields, str):
        fields = (fields,)
    mask = 0
    for name in fields:
        if name not in SP:
            raise ValueError("unknown station-profile field %r (one of %s)" % (name, ", ".join(SP_NAMES)))
        mask |= 1 << SP[name]
    if not mask:
        raise ValueError("fields: at least one station-profile field")
    return mask


def sp_fields_names(mask):
    """the columns a mask selects, in the order they come out (ascending field order)"""
    return tuple(name for i, name in enumerate(SP_NAMES) if mask >> i & 1)


# the columns of chub_forecast_device (the CHUB_FC_* enum of include/chub.h, in order)
FC_NAMES = ("slot", "valid", "sin", "cos", "price", "pv", "wind", "arrivals0", "arrivals1", "fcev")
FC_COUNT = len(FC_NAMES)
FC = {name: i for i, name in enumerate(FC_NAMES)}


def fc_fields_mask(fields=None):
    """a field set of chub_forecast_device as its bit mask: None = all ten, an int = the mask itself, else a sequence of FC_NAMES"""
    if fields is None:
        return (1 << FC_COUNT) - 1
    if hasattr(fields, "__index__"):  # (an int of any kind)
        fields = fields.__index__()
        if fields <= 0 or fields >> FC_COUNT:
            raise ValueError("fields: a non-empty mask over the %d look-ahead fields, got %#x" % (FC_COUNT, fields))
        return fields
    if isinstance(fields, str):
        fields = (fields,)
    mask = 0
    for name in fields:
        if name not in FC:
            raise ValueError("unknown look-ahead field %r (one of %s)" % (name, ", ".join(FC_NAMES)))
        mask |= 1 << FC[name]
    if not mask:
        raise ValueError("fields: at least one look-ahead field")
    return mask


def fc_fields_names(mask):
    """the columns a mask selects, in the order they come out (ascending field order)"""
    return tuple(name for i, name in enumerate(FC_NAMES) if mask >> i & 1)


# the columns of chub_get_step_terms_device (the CHUB_ST_* enum of include/chub.h, in order)
ST_NAMES = ("reward", "income", "income_evs0", "income_evs1", "cost_evs0", "cost_evs1", "income_serve", "income_hys", "hy_cost", "hy_loss",
            "not_meet_loss", "grid_draw", "grid_excess", "used_renew", "fc_power", "hy_act", "gen_hy", "hy_gen", "hy_use", "not_meet",
            "hy_for_fc", "mass_need", "fcev_arrive", "fcev_line", "fcev_queue", "soc_deviation", "soc_penalty")
ST_COUNT = len(ST_NAMES)
ST = {name: i for i, name in enumerate(ST_NAMES)}


def st_fields_mask(fields=None):
    """a field set of chub_get_step_terms_device as its bit mask: None = all 27, an int = the mask itself, else a sequence of ST_NAMES"""
    if fields is None:
        return (1 << ST_COUNT) - 1
    if hasattr(fields, "__index__"):  # (an int of any kind)
        fields = fields.__index__()
        if fields <= 0 or fields >> ST_COUNT:
            raise ValueError("fields: a non-empty mask over the %d step terms, got %#x" % (ST_COUNT, fields))
        return fields
    if isinstance(fields, str):
        fields = (fields,)
    mask = 0
    for name in fields:
        if name not in ST:
            raise ValueError("unknown step term %r (one of %s)" % (name, ", ".join(ST_NAMES)))
        mask |= 1 << ST[name]
    if not mask:
        raise ValueError("fields: at least one step term")
    return mask


def st_fields_names(mask):
    """the columns a mask selects, in the order they come out (ascending field order)"""
    return tuple(name for i, name in enumerate(ST_NAMES) if mask >> i & 1)


# the units of chub_load_dispatch's station targets (CHUB_LOAD_KW / CHUB_LOAD_FRACTION of include/chub.h)
LOAD_KW, LOAD_FRACTION = 0, 1
LOAD_UNITS = {"kw": LOAD_KW, "fraction": LOAD_FRACTION}


def load_units(units):
    """the units of a station target as chub_load_dispatch's enum value: "kw", "fraction" or the value itself"""
    if isinstance(units, str):
        if units not in LOAD_UNITS:
            raise ValueError("unknown load units %r (one of %s)" % (units, ", ".join(sorted(LOAD_UNITS))))
        return LOAD_UNITS[units]
    if units not in (LOAD_KW, LOAD_FRACTION):
        raise ValueError("load units: 'kw' (%d) or 'fraction' (%d), got %r" % (LOAD_KW, LOAD_FRACTION, units))
    return int(units)


# an actor on the device (chub_policy_*): the CHUB_PIN_* / CHUB_PACT_* / CHUB_PHEAD_* / CHUB_PSQ_* / CHUB_PRUN_* enums of include/chub.h, in order
PIN_NAMES = ("obs", "pile_obs", "station_profile", "forecast")
PACT_NAMES = ("tanh", "relu")
PHEAD_NAMES = ("piles", "loads")
PSQ_NAMES = ("tanh", "clip")
PRUN_NAMES = ("lockstep", "autoreset")
PIN = {name: i for i, name in enumerate(PIN_NAMES)}
PACT = {name: i for i, name in enumerate(PACT_NAMES)}
PHEAD = {name: i for i, name in enumerate(PHEAD_NAMES)}
PSQ = {name: i for i, name in enumerate(PSQ_NAMES)}
PRUN = {name: i for i, name in enumerate(PRUN_NAMES)}
POLICY_MAX_INPUTS = POLICY_MAX_LAYERS = 4


class ChubPolicyInput(C.Structure):
    _fields_ = [("kind", C.c_int32), ("fields", C.c_int32), ("param", C.c_int32)]


class ChubPolicySpec(C.Structure):
    """chub_policy_spec of include/chub.h"""
    _fields_ = [("n_inputs", C.c_int32), ("inputs", ChubPolicyInput * 4), ("n_layers", C.c_int32), ("width", C.c_int32 * 4),
                ("hidden_act", C.c_int32), ("head", C.c_int32), ("squash", C.c_int32), ("normalize", C.c_int32), ("clip", C.c_float)]


class ChubPolicySampleOut(C.Structure):
    """chub_policy_sample_out of include/chub.h: device addresses, 0 / None = not asked for"""
    _fields_ = [("d_actions", C.c_void_p), ("d_pile_bits", C.c_void_p), ("d_tail", C.c_void_p), ("d_u", C.c_void_p), ("d_logp", C.c_void_p),
                ("d_features", C.c_void_p)]


class ChubRollout(C.Structure):
    """chub_rollout of include/chub.h: T and the device addresses of the [T][N][...] arrays"""
    _fields_ = [("T", C.c_int64), ("d_packed", C.c_void_p), ("d_pile_bits", C.c_void_p), ("d_tail", C.c_void_p), ("d_u", C.c_void_p),
                ("d_logp", C.c_void_p), ("d_features", C.c_void_p), ("d_final_obs", C.c_void_p)]


class ChubGae(C.Structure):
    """chub_gae of include/chub.h: T, the device addresses of a rollout's blocks and the values, the two factors, the outputs"""
    _fields_ = [("T", C.c_int64), ("d_packed", C.c_void_p), ("d_values", C.c_void_p), ("d_final_values", C.c_void_p), ("d_mask", C.c_void_p),
                ("gamma", C.c_float), ("lam", C.c_float), ("d_adv", C.c_void_p), ("d_ret", C.c_void_p), ("d_stats", C.c_void_p)]


# actor gradients (chub_policy_grad_*): the CHUB_PLOSS_* enum of include/chub.h, in order
PLOSS_NAMES = ("coef", "ppo_clip")
PLOSS = {name: i for i, name in enumerate(PLOSS_NAMES)}


def policy_loss(loss):
    """a surrogate loss as its CHUB_PLOSS_* value: a name of PLOSS_NAMES, or the value itself (the library refuses an unknown one)"""
    return _enum_value(PLOSS, loss, "policy loss")


class ChubPolicyGradPlanOut(C.Structure):
    """chub_policy_grad_plan_out of include/chub.h"""
    _fields_ = [("n_params", C.c_int64), ("workspace_bytes", C.c_int64), ("workgroups", C.c_int32), ("lds_rows", C.c_int32),
                ("lds_bytes", C.c_int32), ("in_registers", C.c_int32)]


class ChubPolicyGradIn(C.Structure):
    """chub_policy_grad_in of include/chub.h: device addresses, 0 / None = not given"""
    _fields_ = [("R", C.c_int64), ("n_rows", C.c_int64), ("d_rows", C.c_void_p), ("d_features", C.c_void_p), ("ld_features", C.c_int64),
                ("d_pile_bits", C.c_void_p), ("d_set_bits", C.c_void_p), ("d_u", C.c_void_p), ("d_logp_old", C.c_void_p), ("d_adv", C.c_void_p),
                ("d_adv_stats", C.c_void_p), ("loss", C.c_int32), ("clip_eps", C.c_float), ("ent_coef", C.c_float), ("pad_", C.c_int32)]


class ChubPolicyGradOut(C.Structure):
    """chub_policy_grad_out of include/chub.h: device addresses, 0 / None = not asked for"""
    _fields_ = [("d_gW", C.c_void_p * 4), ("d_gb", C.c_void_p * 4), ("d_glog_std", C.c_void_p), ("d_logp_new", C.c_void_p),
                ("d_entropy", C.c_void_p), ("d_stats", C.c_void_p)]


# a critic on the device (chub_critic_*): the CHUB_VLOSS_* enum of include/chub.h, in order
VLOSS_NAMES = ("mse", "clipped")
VLOSS = {name: i for i, name in enumerate(VLOSS_NAMES)}


def value_loss(loss):
    """a value loss as its CHUB_VLOSS_* value: a name of VLOSS_NAMES, or the value itself (the library refuses an unknown one)"""
    return _enum_value(VLOSS, loss, "value loss")


class ChubCriticSpec(C.Structure):
    """chub_critic_spec of include/chub.h"""
    _fields_ = [("F", C.c_int32), ("n_layers", C.c_int32), ("width", C.c_int32 * 4), ("hidden_act", C.c_int32), ("normalize", C.c_int32),
                ("clip", C.c_float)]


def critic_spec(F, widths, hidden_act="tanh", normalize=False, clip=0.0):
    """chub_critic_spec for rows of F floats and layers of these widths (the last is 1); nothing is checked here: the library refuses"""
    spec = ChubCriticSpec()
    spec.F = int(F)
    spec.n_layers = len(widths)
    for l, w in enumerate(list(widths)[:4]):
        spec.width[l] = int(w)
    spec.hidden_act = _enum_value(PACT, hidden_act, "hidden activation")
    spec.normalize = 1 if normalize else 0
    spec.clip = float(clip)
    return spec


class ChubCriticPlanOut(C.Structure):
    """chub_critic_plan_out of include/chub.h"""
    _fields_ = [("n_params", C.c_int64), ("workspace_bytes", C.c_int64), ("workgroups", C.c_int32), ("lds_rows", C.c_int32),
                ("lds_bytes", C.c_int32), ("in_registers", C.c_int32)]


class ChubCriticGradIn(C.Structure):
    """chub_critic_grad_in of include/chub.h: device addresses, 0 / None = not given"""
    _fields_ = [("R", C.c_int64), ("n_rows", C.c_int64), ("d_rows", C.c_void_p), ("d_x", C.c_void_p), ("ld", C.c_int64), ("d_ret", C.c_void_p),
                ("d_v_old", C.c_void_p), ("loss", C.c_int32), ("clip_eps", C.c_float)]


class ChubCriticGradOut(C.Structure):
    """chub_critic_grad_out of include/chub.h: device addresses, 0 / None = not asked for"""
    _fields_ = [("d_gW", C.c_void_p * 4), ("d_gb", C.c_void_p * 4), ("d_values", C.c_void_p), ("d_stats", C.c_void_p)]


class ChubAdamHyper(C.Structure):
    """chub_adam_hyper of include/chub.h"""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
                ("max_grad_norm", C.c_double)]


def adam_hyper(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0):
    """chub_adam_hyper from Python values; nothing is checked here: the library refuses"""
    return ChubAdamHyper(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(max_grad_norm))


class ChubAdamPlanOut(C.Structure):
    """chub_adam_plan_out of include/chub.h"""
    _fields_ = [("n", C.c_int64), ("state_bytes", C.c_int64), ("workspace_bytes", C.c_int64), ("norm_workgroups", C.c_int32),
                ("step_workgroups", C.c_int32)]


# a training log and a KL stop on the device (chub_train_log_*): the CHUB_KL_* and CHUB_TLOG_* enums of include/chub.h
KL_NAMES = ("k1", "k3")
KL = {name: i for i, name in enumerate(KL_NAMES)}
TLOG = {"counted": 0, "after_stop": 1, "stopped": 2, "stop_index": 3, "actor": 4, "kl_max": 10, "kl_last": 11, "critic": 12, "actor_opt": 18,
        "critic_opt": 24}
TLOG_WORDS = 30


def kl_kind(kl):
    """a KL estimator as its CHUB_KL_* value: a name of KL_NAMES, or the value itself (the library refuses an unknown one)"""
    return _enum_value(KL, kl, "KL estimator")


class ChubPpoUpdateArgs(C.Structure):
    """chub_ppo_update_args of include/chub.h: handles and device addresses, 0 / None = not given"""
    _fields_ = [("grad", C.c_void_p), ("critic", C.c_void_p), ("actor_opt", C.c_void_p), ("critic_opt", C.c_void_p), ("log", C.c_void_p),
                ("n_rows", C.c_int64), ("d_features", C.c_void_p), ("ld_features", C.c_int64), ("d_pile_bits", C.c_void_p),
                ("d_set_bits", C.c_void_p), ("d_u", C.c_void_p), ("d_logp_old", C.c_void_p), ("d_adv", C.c_void_p), ("d_adv_stats", C.c_void_p),
                ("d_ret", C.c_void_p), ("d_v_old", C.c_void_p), ("policy_loss", C.c_int32), ("value_loss", C.c_int32),
                ("policy_clip_eps", C.c_float), ("value_clip_eps", C.c_float), ("ent_coef", C.c_float), ("epochs", C.c_int32),
                ("minibatch_rows", C.c_int64), ("key", C.c_uint64), ("d_rows", C.c_void_p), ("kl_kind", C.c_int32), ("pad_", C.c_int32),
                ("kl_limit", C.c_double)]


# constrained PPO on the device (chub_lagrange_*): the CHUB_COST_* and CHUB_LAG_* enums of include/chub.h
COST_KIND_NAMES = ("step", "done")
COST_KIND = {name: i for i, name in enumerate(COST_KIND_NAMES)}
LAG_MAX_K, LAG_STATS, LAG_WORDS = 4, 6, 3


def cost_kind(kind):
    """a cost kind as its CHUB_COST_* value: a name of COST_KIND_NAMES, or the value itself (the library refuses an unknown one)"""
    return _enum_value(COST_KIND, kind, "cost kind")


class ChubConstraint(C.Structure):
    """chub_constraint of include/chub.h"""
    _fields_ = [("column", C.c_int32), ("kind", C.c_int32), ("limit", C.c_double), ("lr", C.c_double), ("lambda0", C.c_double),
                ("lambda_max", C.c_double)]


class ChubCostGae(C.Structure):
    """chub_cost_gae of include/chub.h: device addresses, 0 / None = not given"""
    _fields_ = [("T", C.c_int64), ("C", C.c_int32), ("pad_", C.c_int32), ("d_terms", C.c_void_p), ("d_packed", C.c_void_p),
                ("d_values", C.c_void_p * 4), ("d_final_values", C.c_void_p * 4), ("d_mask", C.c_void_p), ("gamma", C.c_float),
                ("lam", C.c_float), ("d_adv", C.c_void_p * 4), ("d_ret", C.c_void_p * 4), ("d_ep_carry", C.c_void_p)]


# reward scaling on the device (chub_return_norm_*)
RETURN_NORM_MAGIC = 0x314d524e52424843  # CHUB_RETURN_NORM_MAGIC of include/chub.h: the first word of a state blob
RETURN_NORM_BLOB_HEAD = 48              # magic, N, the state [3], scale32 and its padding; the carry [N] f32 follows


class ChubReturnNormSpec(C.Structure):
    """chub_return_norm_spec of include/chub.h"""
    _fields_ = [("gamma", C.c_float), ("clip", C.c_float), ("eps", C.c_double)]


# pile sets (chub_pile_set_device): the CHUB_PSET_* enum of include/chub.h, in order
PSET_NAMES = ("all", "occupied", "decidable")
PSET = {name: i for i, name in enumerate(PSET_NAMES)}


def pile_set(which):
    """a pile set as its CHUB_PSET_* value: a name of PSET_NAMES, or the value itself (the library refuses an unknown one)"""
    return _enum_value(PSET, which, "pile set")


def _enum_value(table, value, what):
    if isinstance(value, str):
        if value not in table:
            raise ValueError("unknown %s %r (one of %s)" % (what, value, ", ".join(table)))
        return table[value]
    return int(value)


def policy_inputs(inputs):
    """the input blocks of a policy as (kind, fields mask, param) triples.  An entry is a kind name ("obs"; the feature blocks with every
    field and 8 buckets / slots of look-ahead), or a tuple (kind, fields[, param]) with fields as the feature call takes them"""
    if isinstance(inputs, str):
        inputs = (inputs,)
    out = []
    for entry in inputs:
        kind, fields, param = (entry, None, None) if isinstance(entry, (str, int)) else (tuple(entry) + (None, None))[:3]
        kind = _enum_value(PIN, kind, "policy input")
        if kind == PIN["obs"]:
            out.append((kind, 0, 0))
        elif kind == PIN["pile_obs"]:
            out.append((kind, pile_fields_mask(fields), 0))
        elif kind == PIN["station_profile"]:
            out.append((kind, sp_fields_mask(fields), 8 if param is None else int(param)))
        elif kind == PIN["forecast"]:
            out.append((kind, fc_fields_mask(fields), 8 if param is None else int(param)))
        else:
            out.append((kind, int(fields or 0), int(param or 0)))  # (the library refuses it with its own message)
    return out


def policy_spec(widths, inputs=("obs",), head="piles", hidden_act="tanh", squash="tanh", normalize=False, clip=0.0):
    """a chub_policy_spec from Python values: widths = the outputs of every layer (the last one the head's), inputs as policy_inputs takes
    them.  Counts beyond the struct's four slots are passed on as they are: the library refuses them"""
    spec = ChubPolicySpec()
    blocks = policy_inputs(inputs)
    spec.n_inputs = len(blocks)
    for i, (kind, fields, param) in enumerate(blocks[:POLICY_MAX_INPUTS]):
        spec.inputs[i].kind, spec.inputs[i].fields, spec.inputs[i].param = kind, fields, param
    widths = [int(w) for w in widths]
    spec.n_layers = len(widths)
    for l, w in enumerate(widths[:POLICY_MAX_LAYERS]):
        spec.width[l] = w
    spec.hidden_act = _enum_value(PACT, hidden_act, "hidden activation")
    spec.head = _enum_value(PHEAD, head, "policy head")
    spec.squash = _enum_value(PSQ, squash, "squash")
    spec.normalize = int(bool(normalize))
    spec.clip = float(clip)
    return spec


class ChubOptions(C.Structure):
    """chub_options of include/chub.h (all zero = defaults; the library reads no environment variables)"""
    _fields_ = [("slot_kernel", C.c_int32), ("no_arena", C.c_int32), ("fused_step", C.c_int32), ("tile", C.c_int32), ("walk_ahead", C.c_int32), ("work_order", C.c_int32), ("span_steps", C.c_int32), ("span_tails", C.c_int32)]


SLOT_KERNELS = {"auto": 0, "wave": 1, "packed": 2}
FUSED_STEP = {"auto": 0, "off": 1, "on": 2}
TILES = {"auto": 0, "small": 1, "large": 2}
WALK_AHEAD = {"auto": 0, "off": 1}
WORK_ORDER = {"auto": 0, "dispatch": 1}


class ChubError(RuntimeError):
    pass


class ChubConfig(C.Structure):
    _fields_ = [("station_list", C.c_int32 * 2), ("station_type_list", C.c_int32 * 2),
                ("constant_charging", C.c_int32), ("reserved0", C.c_int32),
                ("hydro_prod_rate", C.c_double), ("hydro_store_vlt", C.c_double), ("init_soc", C.c_double),
                ("fc_max_power", C.c_double), ("fcev_permeate", C.c_double), ("renew_fluctuate", C.c_double),
                ("price_fluctuate", C.c_double), ("hydro_loss", C.c_double)]


# the eight scalar constructor kwargs that may differ from env to env (chub_env_params, chub_create_params)
ENV_PARAM_FIELDS = ("hydro_prod_rate", "hydro_store_vlt", "init_soc", "fc_max_power", "fcev_permeate", "renew_fluctuate", "price_fluctuate",
                    "hydro_loss")


class ChubEnvParams(C.Structure):
    _fields_ = [(name, C.c_double) for name in ENV_PARAM_FIELDS]


def lib_path():
    """libchub.so next to this file; CHUB_LIB names another build of it (compiler-flag experiments)"""
    return os.environ.get("CHUB_LIB") or os.path.join(_HERE, "libchub.so")


def source_hash():
    """the hash the Makefile compiles into chub_build_id(): sha256 over the sources, first 16 hex digits"""
    import hashlib

    h = hashlib.sha256()
    csrc = os.path.join(_HERE, "csrc")
    for name in ("chub_kernels.hip", "chub_policy.hip", "chub_gae.hip", "chub_critic.hip", "chub_adam.hip", "chub_trainlog.hip", "chub_lagrange.hip", "chub_retnorm.hip", "chub_runtime.cpp", "chub_comm.cpp", "chub_device.h", "chub_curves.h",
                 "chub_plan.h", "chub_policy.h", "chub_gae.h", "chub_critic.h", "chub_adam.h", "chub_trainlog.h", "chub_lagrange.h", "chub_retnorm.h"):
        h.update(open(os.path.join(csrc, name), "rb").read())
    h.update(open(os.path.join(os.path.dirname(_HERE), "include", "chub.h"), "rb").read())
    return h.hexdigest()[:16]


_lib = None


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise ChubError("libchub.so is not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "or `make -C charginghub-env_amd/csrc`; there is no CPU fallback" % path)
    lib = C.CDLL(path)
    if not os.environ.get("CHUB_LIB"):
        # a prebuilt library must match the sources next to it: no silent reuse of a stale build
        lib.chub_build_id.restype = C.c_char_p
        have, want = lib.chub_build_id().decode(), source_hash()
        if have != want:
            raise ChubError("libchub.so (build id %s) is older than its sources (%s): rebuild with "
                            "`make -C charginghub-env_amd/csrc`" % (have, want))
    P, I, L = C.c_void_p, C.c_int, C.c_int64
    sig = {
        "chub_create": (I, [C.POINTER(ChubConfig), C.c_char_p, L, L, I, C.c_uint64, I, C.POINTER(P)]),
        "chub_create_ex": (I, [C.POINTER(ChubConfig), C.c_char_p, L, L, I, C.c_uint64, I, C.POINTER(ChubOptions), C.POINTER(P)]),
        "chub_destroy": (I, [P]),
        "chub_obs_dim": (I, [P]), "chub_act_dim": (I, [P]), "chub_num_envs": (L, [P]), "chub_clock": (I, [P]), "chub_uses_packed_kernel": (I, [P]), "chub_uses_fused_step": (I, [P]), "chub_uses_xcd_order": (I, [P]),
        "chub_launch_plan": (I, [C.POINTER(ChubConfig), L, I, C.POINTER(ChubOptions), P]),
        "chub_launch_plan_params": (I, [C.POINTER(ChubConfig), L, I, C.POINTER(ChubOptions), P]),
        "chub_pair_plan": (I, [C.POINTER(ChubConfig), L, I, C.POINTER(ChubOptions), I, C.c_uint32, I, L, P]), "chub_uses_pair_tails": (I, [P]),
        "chub_create_params": (I, [C.POINTER(ChubConfig), C.c_char_p, L, L, I, C.c_uint64, I, C.POINTER(ChubOptions), P, C.POINTER(P)]),
        "chub_set_env_params": (I, [P, P, P]), "chub_get_env_params": (I, [P, P]), "chub_has_env_params": (I, [P]),
        "chub_reset": (I, [P, P, P, P]),
        "chub_step": (I, [P, P, P, P, P, P]), "chub_host_actions": (I, [P, C.POINTER(P)]),
        "chub_step_bits": (I, [P, P, P, P, P, P, P]), "chub_host_bits": (I, [P, C.POINTER(P), C.POINTER(P)]),
        "chub_step_bits_device": (I, [P, P, P, P, P, P, P, P]), "chub_step_bits_device_packed": (I, [P, P, P, P, P, P]),
        "chub_reset_device": (I, [P, P, P, P, P]),
        "chub_step_device": (I, [P, P, P, P, P, P, P]),
        "chub_step_device_packed": (I, [P, P, P, P, P]),
        "chub_reset_envs": (I, [P, P, P, P, P]), "chub_step_envs": (I, [P, P, P, P, P, P, P]), "chub_reset_envs_device": (I, [P, P, P, P, P, P]),
        "chub_step_envs_device": (I, [P, P, P, P, P, P, P, P]), "chub_env_clocks": (I, [P, P, P]), "chub_clock_groups": (I, [P]),
        "chub_dmask_reset_envs_device": (I, [P, P, P, P, P, P]), "chub_dmask_step_envs_device": (I, [P, P, P, P, P, P, P, P]),
        "chub_autoreset_step_device": (I, [P, P, P, P, P, P, P, P]),
        "chub_call_plan": (I, [C.POINTER(ChubConfig), L, I, C.POINTER(ChubOptions), I, C.c_uint32, P]),
        "chub_step_load": (I, [P, P, P, P, P, P]), "chub_step_load_device": (I, [P, P, P, P, P, P, P]),
        "chub_step_load_envs": (I, [P, P, P, P, P, P, P]), "chub_step_load_envs_device": (I, [P, P, P, P, P, P, P, P]),
        "chub_random_actions_device": (I, [P, C.c_uint64, C.c_uint32, P, P]),
        "chub_sync": (I, [P]),
        "chub_profile_begin": (I, [P, I, I]), "chub_profile_end": (I, [P, P, P, P]),
        "chub_get_slots": (I, [P, P]), "chub_get_station_scalars": (I, [P, P]), "chub_get_telemetry": (I, [P, P]),
        "chub_get_obs_f64": (I, [P, P]), "chub_get_reward_f64": (I, [P, P]), "chub_set_telemetry": (I, [P, I]), "chub_fcev_stuck_count": (I, [P, P]),
        "chub_telemetry_host": (I, [P, C.POINTER(P), C.POINTER(P), C.POINTER(P)]),
        "chub_set_episode_stats": (I, [P, I]), "chub_has_episode_stats": (I, [P]), "chub_get_episode_stats": (I, [P, I, P]),
        "chub_get_episode_counts": (I, [P, P]), "chub_episode_stats_device": (I, [P, I, P, P, P]),
        "chub_episode_summary_device": (I, [P, P, I, P]), "chub_episode_summary": (I, [P, P, I]),
        "chub_pile_obs_columns": (I, [C.c_uint32]), "chub_pile_obs_device": (I, [P, C.c_uint32, P, P, P]),
        "chub_station_profile_size": (I, [C.c_uint32, C.c_int32]), "chub_station_profile_device": (I, [P, C.c_uint32, C.c_int32, P, P, P]),
        "chub_load_dispatch_device": (I, [P, I, P, P, P, P, P, P]), "chub_load_dispatch": (I, [P, I, P, P, P, P]),
        "chub_forecast_size": (I, [C.c_uint32, C.c_int32]), "chub_forecast_device": (I, [P, C.c_uint32, C.c_int32, P, P, P]),
        "chub_forecast": (I, [P, C.c_uint32, C.c_int32, P]),
        "chub_get_step_terms_size": (I, [C.c_uint32]), "chub_get_step_terms_device": (I, [P, C.c_uint32, P, P, P]),
        "chub_get_step_terms": (I, [P, C.c_uint32, P]), "chub_set_step_terms": (I, [P, C.c_uint32, P]), "chub_get_step_terms_attached": (I, [P]),
        "chub_set_rng_compat_seeds": (I, [P, P]), "chub_set_rng_compat_state": (I, [P, P]),
        "chub_get_rng_compat_state": (I, [P, P]), "chub_compat_replay_constructor": (I, [P]), "chub_set_ou_state": (I, [P, P]),
        "chub_copy_envs": (I, [P, P, P, P, L]), "chub_copy_envs_device": (I, [P, P, P, P, L, P]),
        "chub_state_size": (L, [P]), "chub_get_state": (I, [P, P, L]), "chub_set_state": (I, [P, P, L]),
        "chub_get_hy_table": (I, [P, P]), "chub_get_hy_table_env": (I, [P, L, P]), "chub_set_hy_table": (I, [P, P]),
        "chub_last_error": (C.c_char_p, []), "chub_device_count": (I, []), "chub_build_id": (C.c_char_p, []),
        "chub_comm_unique_id": (I, [P]), "chub_comm_create": (I, [P, I, I, I, C.POINTER(P)]), "chub_comm_destroy": (I, [P]),
        "chub_comm_world": (I, [P]), "chub_comm_rank": (I, [P]), "chub_comm_gather": (I, [P, P, P, L, P]),
        "chub_comm_gather_timed": (I, [P, P, P, L, P, I, C.POINTER(C.c_double)]),
        "chub_comm_max_f64": (I, [P, C.POINTER(C.c_double), P]), "chub_comm_barrier": (I, [P, P]),
        "chub_comm_ranks_seen": (I, [P, C.POINTER(C.c_int), P]),
        "chub_comm_set_overlap": (I, [P, I]), "chub_comm_gather_begin": (I, [P, P, P]), "chub_comm_join": (I, [P, P]), "chub_device_info": (I, [I, P]),
        "chub_step_gather": (I, [P, P, P, P, P, P]), "chub_run_steps": (I, [P, P, P, I, P, P, P, L, L, P]),
        "chub_tape_register_soc": (I, [P, P, C.c_int32, P]), "chub_set_slots": (I, [P, P]), "chub_set_station_queue": (I, [P, P]),
        "chub_step_tape": (I, [P, P, P, P, P, P, P]), "chub_reset_tape": (I, [P, P, P, P]), "chub_tape_clear_soc": (I, [P]),
        "chub_step_tape_env": (I, [P, P, P, P, P, P, C.c_int32, P, P, P]), "chub_reset_tape_env": (I, [P, P, P, P, P, P]),
        "chub_graph_begin": (I, [P, P]), "chub_graph_end": (I, [P, P, C.POINTER(P)]), "chub_graph_launch": (I, [P, P]),
        "chub_graph_destroy": (I, [P]),
        "chub_malloc_device": (I, [I, L, C.POINTER(P)]), "chub_free_device": (I, [I, P]), "chub_copy_to_host": (I, [I, P, P, L, P]),
        "chub_copy_to_device": (I, [I, P, P, L, P]), "chub_alloc_host": (I, [I, L, C.POINTER(P)]), "chub_free_host": (I, [I, P]), "chub_stream_create": (I, [I, C.POINTER(P)]), "chub_stream_destroy": (I, [I, P]),
        "chub_stream_sync": (I, [I, P]),
        "chub_policy_input_width": (I, [C.POINTER(ChubConfig), C.POINTER(ChubPolicySpec), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "chub_policy_create": (I, [P, C.POINTER(ChubPolicySpec), P, P, P, P, C.POINTER(P)]), "chub_policy_destroy": (I, [P]),
        "chub_policy_set_weights": (I, [P, C.c_int32, P, P]), "chub_policy_set_weights_device": (I, [P, C.c_int32, P, P, P]),
        "chub_policy_act_device": (I, [P, P, P, L, P, P, P, P, P]), "chub_policy_act": (I, [P, P, P, P]),
        "chub_policy_run_steps": (I, [P, P, I, P, P, P, L, L, P]),
        "chub_next_tick": (I, [P, C.POINTER(C.c_uint32)]), "chub_policy_set_exploration": (I, [P, C.c_uint64, P]),
        "chub_policy_set_log_std_device": (I, [P, P, P]),
        "chub_policy_sample_device": (I, [P, P, P, L, P, C.POINTER(ChubPolicySampleOut), P]),
        "chub_policy_collect": (I, [P, P, I, C.POINTER(ChubRollout), P, L, P]),
        "chub_pile_set_device": (I, [P, I, P, P, P]),
        "chub_policy_sample_set_device": (I, [P, P, P, L, P, I, P, C.POINTER(ChubPolicySampleOut), P]),
        "chub_policy_collect_set": (I, [P, P, I, I, C.POINTER(ChubRollout), P, P, L, P]),
        "chub_rollout_gae_device": (I, [P, C.POINTER(ChubGae), P]),
        "chub_moments_create": (I, [P, C.c_int32, C.POINTER(P)]), "chub_moments_destroy": (I, [P]),
        "chub_moments_update_device": (I, [P, P, L, L, P, P]), "chub_moments_reset_device": (I, [P, P]),
        "chub_moments_get": (I, [P, C.POINTER(C.c_double), P, P]), "chub_moments_set": (I, [P, C.c_double, P, P]),
        "chub_moments_state_device": (I, [P, C.POINTER(P)]),
        "chub_policy_set_normalizer": (I, [P, P, P]), "chub_policy_set_normalizer_device": (I, [P, P, P, P]),
        "chub_policy_get_normalizer_device": (I, [P, P, P, P]), "chub_policy_normalizer_from_moments_device": (I, [P, P, C.c_double, P]),
        "chub_population_param_count": (I, [C.POINTER(ChubConfig), C.POINTER(ChubPolicySpec), C.POINTER(L)]),
        "chub_population_create": (I, [P, C.c_int32, C.c_uint64, C.POINTER(P)]), "chub_population_destroy": (I, [P]),
        "chub_population_perturb_device": (I, [P, P, P, C.c_float, C.c_uint32, P]),
        "chub_population_set_member_device": (I, [P, C.c_int32, C.c_int32, P, P, P]),
        "chub_population_get_member_device": (I, [P, C.c_int32, C.c_int32, P, P, P]),
        "chub_population_set_member": (I, [P, C.c_int32, C.c_int32, P, P]), "chub_population_get_member": (I, [P, C.c_int32, C.c_int32, P, P]),
        "chub_population_copy_members_device": (I, [P, P, P, C.c_int32, P]),
        "chub_population_act_device": (I, [P, P, P, L, P, P, P, P, P]), "chub_population_run_steps": (I, [P, P, I, P, P, P, L, L, P]),
        "chub_population_es_gradient_device": (I, [P, P, C.c_uint32, P, P, P]),
        "chub_policy_grad_plan": (I, [C.POINTER(ChubConfig), C.POINTER(ChubPolicySpec), L, C.POINTER(ChubPolicyGradPlanOut)]),
        "chub_policy_grad_create": (I, [P, L, C.POINTER(P)]), "chub_policy_grad_destroy": (I, [P]),
        "chub_policy_grad_device": (I, [P, C.POINTER(ChubPolicyGradIn), C.POINTER(ChubPolicyGradOut), P]),
        "chub_critic_plan": (I, [C.POINTER(ChubCriticSpec), L, C.POINTER(ChubCriticPlanOut)]),
        "chub_critic_create": (I, [P, C.POINTER(ChubCriticSpec), P, P, P, P, L, C.POINTER(P)]), "chub_critic_destroy": (I, [P]),
        "chub_critic_set_weights": (I, [P, C.c_int32, P, P]), "chub_critic_set_weights_device": (I, [P, C.c_int32, P, P, P]),
        "chub_critic_set_normalizer": (I, [P, P, P]), "chub_critic_set_normalizer_device": (I, [P, P, P, P]),
        "chub_critic_normalizer_from_moments_device": (I, [P, P, C.c_double, P]),
        "chub_critic_values_device": (I, [P, P, L, L, P, L, P, P]),
        "chub_critic_grad_device": (I, [P, C.POINTER(ChubCriticGradIn), C.POINTER(ChubCriticGradOut), P]),
        "chub_adam_plan": (I, [P, P, C.c_int32, C.c_int32, C.POINTER(ChubAdamPlanOut)]),
        "chub_adam_create_policy": (I, [P, C.POINTER(ChubAdamHyper), C.POINTER(P)]),
        "chub_adam_create_critic": (I, [P, C.POINTER(ChubAdamHyper), C.POINTER(P)]), "chub_adam_destroy": (I, [P]),
        "chub_adam_set_hyper": (I, [P, C.POINTER(ChubAdamHyper)]), "chub_adam_set_lr_device": (I, [P, P, P]),
        "chub_adam_grads": (I, [P, P, P, C.POINTER(P)]), "chub_adam_counter_device": (I, [P, C.POINTER(P)]),
        "chub_adam_step_device": (I, [P, P, P, P, P, P]), "chub_adam_reset_device": (I, [P, P]),
        "chub_adam_state_size": (I, [P, C.POINTER(L)]), "chub_adam_get_state": (I, [P, P]), "chub_adam_set_state": (I, [P, P]),
        "chub_policy_get_weights_device": (I, [P, C.c_int32, P, P, P]), "chub_policy_get_weights": (I, [P, C.c_int32, P, P]),
        "chub_policy_get_log_std_device": (I, [P, P, P]), "chub_policy_get_log_std": (I, [P, P]),
        "chub_critic_get_weights_device": (I, [P, C.c_int32, P, P, P]), "chub_critic_get_weights": (I, [P, C.c_int32, P, P]),
        "chub_shuffle_rows_device": (I, [P, C.c_uint64, P, L, L, P, P]), "chub_shuffle_rows": (I, [C.c_uint64, C.c_uint64, L, P]),
        "chub_train_log_create": (I, [P, C.POINTER(P)]), "chub_train_log_destroy": (I, [P]), "chub_train_log_begin_device": (I, [P, P]),
        "chub_train_log_record_device": (I, [P, P, P, C.c_int32, C.c_double, P]), "chub_train_log_steps_device": (I, [P, P, P, P]),
        "chub_train_log_device": (I, [P, C.POINTER(P), C.POINTER(P)]), "chub_train_log_read": (I, [P, P]),
        "chub_train_log_fold": (I, [P, P, P, P, C.c_int32, C.c_double]), "chub_adam_set_gate": (I, [P, P]),
        "chub_ppo_update_plan": (I, [L, L, C.POINTER(L), C.POINTER(L)]), "chub_ppo_update": (I, [C.POINTER(ChubPpoUpdateArgs), P]),
        "chub_policy_collect_terms": (I, [P, P, I, I, C.POINTER(ChubRollout), P, P, L, C.c_uint32, P, P]),
        "chub_lagrange_create": (I, [P, C.c_int32, C.POINTER(ChubConstraint), C.POINTER(P)]), "chub_lagrange_destroy": (I, [P]),
        "chub_lagrange_gae_device": (I, [P, C.POINTER(ChubCostGae), P]), "chub_lagrange_step_device": (I, [P, P]),
        "chub_lagrange_combine_device": (I, [P, L, P, P, C.POINTER(P), P, P]),
        "chub_lagrange_device": (I, [P, C.POINTER(P), C.POINTER(P)]), "chub_lagrange_read": (I, [P, P, P, P]),
        "chub_lagrange_set_lambda_device": (I, [P, P, P]), "chub_lagrange_state_size": (I, [P, C.POINTER(L)]),
        "chub_lagrange_get_state": (I, [P, P]), "chub_lagrange_set_state": (I, [P, P]),
        "chub_lagrange_fold": (I, [C.POINTER(ChubConstraint), P, P, P]),
        "chub_return_norm_create": (I, [P, C.POINTER(ChubReturnNormSpec), C.POINTER(P)]), "chub_return_norm_destroy": (I, [P]),
        "chub_return_norm_update_device": (I, [P, P, L, P, P]), "chub_return_norm_gae_device": (I, [P, C.POINTER(ChubGae), P]),
        "chub_return_norm_reset_carry_device": (I, [P, P, P]), "chub_return_norm_reset_device": (I, [P, P]),
        "chub_return_norm_device": (I, [P, C.POINTER(P), C.POINTER(P), C.POINTER(P)]), "chub_return_norm_state_size": (I, [P, C.POINTER(L)]),
        "chub_return_norm_get_state": (I, [P, P]), "chub_return_norm_set_state": (I, [P, P]),
        "chub_return_norm_fold": (I, [P, P, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]),
    }
    for name, (res, args) in sig.items():
        try:
            fn = getattr(lib, name)  # AttributeError here == ABI drift between chub.h and the library
        except AttributeError:
            if os.environ.get("CHUB_LIB"):  # an older build loaded on purpose (A/B timing): it lacks the newer entry points --
                def missing(*_a, _name=name, _path=path):  # ... and says so where one of them is first used
                    raise ChubError("%s is not exported by the library CHUB_LIB names (%s): an older build" % (_name, _path))
                setattr(lib, name, missing)
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


EXPORTED = ["chub_create", "chub_create_ex", "chub_destroy", "chub_obs_dim", "chub_act_dim", "chub_num_envs", "chub_clock", "chub_uses_packed_kernel", "chub_uses_fused_step", "chub_uses_xcd_order", "chub_launch_plan", "chub_launch_plan_params", "chub_pair_plan", "chub_uses_pair_tails",
            "chub_create_params", "chub_set_env_params", "chub_get_env_params", "chub_has_env_params", "chub_reset",
            "chub_step", "chub_host_actions", "chub_step_bits", "chub_host_bits", "chub_step_bits_device", "chub_step_bits_device_packed", "chub_reset_device", "chub_step_device", "chub_step_device_packed", "chub_step_load", "chub_step_load_device", "chub_step_load_envs", "chub_step_load_envs_device", "chub_reset_envs", "chub_step_envs", "chub_reset_envs_device", "chub_step_envs_device",
            "chub_env_clocks", "chub_clock_groups", "chub_dmask_reset_envs_device", "chub_dmask_step_envs_device", "chub_autoreset_step_device", "chub_call_plan", "chub_random_actions_device", "chub_sync", "chub_profile_begin", "chub_profile_end",
            "chub_get_slots", "chub_get_station_scalars", "chub_get_telemetry", "chub_get_obs_f64",
            "chub_get_reward_f64", "chub_set_telemetry", "chub_fcev_stuck_count", "chub_set_rng_compat_seeds", "chub_set_rng_compat_state", "chub_get_rng_compat_state", "chub_compat_replay_constructor", "chub_set_ou_state",
            "chub_copy_envs", "chub_copy_envs_device", "chub_state_size", "chub_get_state", "chub_set_state", "chub_get_hy_table", "chub_get_hy_table_env", "chub_set_hy_table", "chub_last_error", "chub_device_count", "chub_build_id",
            "chub_comm_unique_id", "chub_comm_create", "chub_comm_destroy", "chub_comm_world", "chub_comm_rank", "chub_comm_gather", "chub_comm_gather_timed",
            "chub_comm_max_f64", "chub_comm_barrier", "chub_comm_ranks_seen", "chub_comm_set_overlap", "chub_comm_gather_begin", "chub_comm_join", "chub_device_info", "chub_step_gather", "chub_run_steps", "chub_tape_register_soc", "chub_set_slots",
            "chub_set_station_queue", "chub_step_tape", "chub_reset_tape", "chub_tape_clear_soc", "chub_step_tape_env", "chub_reset_tape_env", "chub_telemetry_host", "chub_graph_begin", "chub_graph_end", "chub_graph_launch", "chub_graph_destroy",
            "chub_malloc_device", "chub_free_device", "chub_copy_to_host", "chub_copy_to_device", "chub_alloc_host", "chub_free_host", "chub_stream_create",
            "chub_stream_destroy", "chub_stream_sync",
            "chub_set_episode_stats", "chub_has_episode_stats", "chub_get_episode_stats", "chub_get_episode_counts", "chub_episode_stats_device",
            "chub_episode_summary_device", "chub_episode_summary", "chub_pile_obs_columns", "chub_pile_obs_device",
            "chub_station_profile_size", "chub_station_profile_device", "chub_load_dispatch_device", "chub_load_dispatch",
            "chub_forecast_size", "chub_forecast_device", "chub_forecast",
            "chub_get_step_terms_size", "chub_get_step_terms_device", "chub_get_step_terms", "chub_set_step_terms", "chub_get_step_terms_attached",
            "chub_policy_input_width", "chub_policy_create", "chub_policy_destroy", "chub_policy_set_weights", "chub_policy_set_weights_device",
            "chub_policy_act_device", "chub_policy_act", "chub_policy_run_steps",
            "chub_next_tick", "chub_policy_set_exploration", "chub_policy_set_log_std_device", "chub_policy_sample_device", "chub_policy_collect",
            "chub_pile_set_device", "chub_policy_sample_set_device", "chub_policy_collect_set", "chub_rollout_gae_device",
            "chub_moments_create", "chub_moments_destroy", "chub_moments_update_device", "chub_moments_reset_device", "chub_moments_get", "chub_moments_set",
            "chub_moments_state_device", "chub_policy_set_normalizer", "chub_policy_set_normalizer_device", "chub_policy_get_normalizer_device",
            "chub_policy_normalizer_from_moments_device",
            "chub_population_param_count", "chub_population_create", "chub_population_destroy", "chub_population_perturb_device",
            "chub_population_set_member_device", "chub_population_get_member_device", "chub_population_set_member", "chub_population_get_member",
            "chub_population_copy_members_device", "chub_population_act_device", "chub_population_run_steps", "chub_population_es_gradient_device",
            "chub_policy_grad_plan", "chub_policy_grad_create", "chub_policy_grad_destroy", "chub_policy_grad_device",
            "chub_critic_plan", "chub_critic_create", "chub_critic_destroy", "chub_critic_set_weights", "chub_critic_set_weights_device",
            "chub_critic_set_normalizer", "chub_critic_set_normalizer_device", "chub_critic_normalizer_from_moments_device",
            "chub_critic_values_device", "chub_critic_grad_device",
            "chub_adam_plan", "chub_adam_create_policy", "chub_adam_create_critic", "chub_adam_destroy", "chub_adam_set_hyper", "chub_adam_set_lr_device",
            "chub_adam_grads", "chub_adam_counter_device", "chub_adam_step_device", "chub_adam_reset_device", "chub_adam_state_size",
            "chub_adam_get_state", "chub_adam_set_state", "chub_policy_get_weights_device", "chub_policy_get_weights",
            "chub_policy_get_log_std_device", "chub_policy_get_log_std", "chub_critic_get_weights_device", "chub_critic_get_weights",
            "chub_shuffle_rows_device", "chub_shuffle_rows",
            "chub_train_log_create", "chub_train_log_destroy", "chub_train_log_begin_device", "chub_train_log_record_device",
            "chub_train_log_steps_device", "chub_train_log_device", "chub_train_log_read", "chub_train_log_fold", "chub_adam_set_gate",
            "chub_ppo_update_plan", "chub_ppo_update",
            "chub_policy_collect_terms", "chub_lagrange_create", "chub_lagrange_destroy", "chub_lagrange_gae_device", "chub_lagrange_step_device",
            "chub_lagrange_combine_device", "chub_lagrange_device", "chub_lagrange_read", "chub_lagrange_set_lambda_device",
            "chub_lagrange_state_size", "chub_lagrange_get_state", "chub_lagrange_set_state", "chub_lagrange_fold",
            "chub_return_norm_create", "chub_return_norm_destroy", "chub_return_norm_update_device", "chub_return_norm_gae_device",
            "chub_return_norm_reset_carry_device", "chub_return_norm_reset_device", "chub_return_norm_device", "chub_return_norm_state_size",
            "chub_return_norm_get_state", "chub_return_norm_set_state", "chub_return_norm_fold"]


def check(rc):
    if rc != 0:
        msg = load_library().chub_last_error()
        raise ChubError("libchub error %d: %s" % (rc, msg.decode() if msg else "?"))
