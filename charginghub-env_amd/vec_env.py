"""VecChargingHub -- N lock-step charging-hub environments on one MI355X.

Batched counterpart of ``EvcsspManagerEnv_v6`` (evcssp_manager.py:19-414): same constructor kwargs, same
observation / action layout per env, arrays of shape ``[N, ...]``.  All simulation runs in libchub's HIP
kernels; this class only marshals numpy arrays across the C ABI.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ChubConfig, ChubError, ChubOptions, check, load_library


def make_config(station_list, station_type_list, constant_charging=False, hydro_prod_rate=None, hydro_store_vlt=None,
                init_soc=0.5, fc_max_power=None, fcev_permeate=0.01, renew_fluctuate=0, price_fluctuate=0,
                hydro_loss=0):
    """Constructor kwargs of the reference (MGR:25-27) -> chub_config, with the reference's defaults
    (hydro_prod_rate None -> 430 HYD:140-143, hydro_store_vlt None -> 5000 HYD:96, fc_max_power None -> 100 HYD:401-404)."""
    if not (len(station_list) == len(station_type_list) == 2):  # MGR:37
        raise AssertionError("station_list and station_type_list must both have 2 entries")
    cfg = ChubConfig()
    for k in range(2):
        cfg.station_list[k] = int(station_list[k])
        if station_type_list[k] == "fast":
            cfg.station_type_list[k] = _lib.CHUB_FAST
        elif station_type_list[k] == "slow":
            cfg.station_type_list[k] = _lib.CHUB_SLOW
        else:
            raise ValueError("EVS type must be fast or slow")  # AGG:196
    cfg.constant_charging = int(bool(constant_charging))
    cfg.hydro_prod_rate = 430.0 if hydro_prod_rate is None else float(hydro_prod_rate)
    cfg.hydro_store_vlt = 5000.0 if hydro_store_vlt is None else float(hydro_store_vlt)
    cfg.init_soc = float(init_soc)
    cfg.fc_max_power = 100.0 if fc_max_power is None else float(fc_max_power)
    cfg.fcev_permeate = float(fcev_permeate)
    cfg.renew_fluctuate = float(renew_fluctuate)
    cfg.price_fluctuate = float(price_fluctuate)
    cfg.hydro_loss = float(hydro_loss)
    return cfg


_ENV_PARAM_DEFAULTS = {"hydro_prod_rate": 430.0, "hydro_store_vlt": 5000.0, "init_soc": 0.5, "fc_max_power": 100.0, "fcev_permeate": 0.01,
                       "renew_fluctuate": 0.0, "price_fluctuate": 0.0, "hydro_loss": 0.0}  # make_config's defaults (None -> the reference's)


def _is_sequence(v):
    return v is not None and not isinstance(v, (str, bytes)) and np.ndim(v) > 0


def _field_values(name, value, n_envs):
    """one per-env kwarg -> float64 [n_envs]: a scalar broadcasts, a sequence must have one entry per env (None entries take the default)"""
    if _is_sequence(value):
        seq = list(np.asarray(value, dtype=object).ravel()) if np.ndim(value) == 1 else None
        if seq is None or len(seq) != n_envs:
            raise ValueError("%s: expected a scalar or a sequence of n_envs = %d values, got shape %s" % (name, n_envs, np.shape(value)))
        return np.array([_ENV_PARAM_DEFAULTS[name] if v is None else float(v) for v in seq], dtype=np.float64)
    return np.full(n_envs, _ENV_PARAM_DEFAULTS[name] if value is None else float(value), dtype=np.float64)


def split_env_params(n_envs, kwargs):
    """The hub kwargs with per-env sequences taken out: (scalar kwargs for make_config, rows) -- rows is None when every one of the
    eight per-env kwargs (_lib.ENV_PARAM_FIELDS) is a scalar, else a [n_envs] array of chub_env_params (scalars broadcast)."""
    if not any(_is_sequence(kwargs.get(f)) for f in _lib.ENV_PARAM_FIELDS):
        return dict(kwargs), None
    scalar = {k: v for k, v in kwargs.items() if k not in _lib.ENV_PARAM_FIELDS}
    rows = np.zeros(n_envs, dtype=ENV_PARAMS_DTYPE)
    for f in _lib.ENV_PARAM_FIELDS:
        rows[f] = _field_values(f, kwargs.get(f), n_envs)
    return scalar, rows


def slice_env_kwargs(kwargs, total_envs, lo, n):
    """the hub kwargs of a shard that holds envs lo .. lo + n - 1 of total_envs: per-env sequences (one value per env of the whole
    batch) sliced, everything else as it is"""
    out = {}
    for k, v in kwargs.items():
        if k in _lib.ENV_PARAM_FIELDS and _is_sequence(v):
            seq = np.asarray(v, dtype=object).ravel()
            if np.ndim(v) != 1 or seq.size != total_envs:
                raise ValueError("%s: expected a scalar or a sequence of total_envs = %d values, got shape %s" % (k, total_envs, np.shape(v)))
            v = list(seq[lo:lo + n])
        out[k] = v
    return out


ENV_PARAMS_DTYPE = np.dtype([(f, np.float64) for f in _lib.ENV_PARAM_FIELDS])  # the layout of chub_env_params


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def summary_dict(raw):
    """chub_episode_summary's [1 + 4 * EP_COUNT] doubles -> {"count": n, name: {"mean", "std", "min", "max"}}"""
    raw = np.asarray(raw, dtype=np.float64)
    n = int(raw[0])
    out = {"count": n}
    for i, name in enumerate(_lib.EPISODE_NAMES):
        s, ss, lo, hi = (float(v) for v in raw[1 + 4 * i:5 + 4 * i])
        mean = s / n if n else float("nan")
        var = max(ss / n - mean * mean, 0.0) if n else float("nan")
        out[name] = {"mean": mean, "std": var ** 0.5, "min": lo, "max": hi}
    return out


class _DeviceNet(object):
    """What DevicePolicy and DeviceCritic share, as chub_policy and chub_critic share MlpNet in csrc/chub_runtime.cpp: one net's weight and
    normaliser calls.  A subclass names the C prefix (`_c_name`: the calls are chub_<_c_name>_*), the attribute that holds its handle
    (`_h_name`) and what its messages call a row (`_row`)."""
    _c_name = _h_name = _row = None

    def _net(self, call, *args):
        check(getattr(self._lib, "chub_%s_%s" % (self._c_name, call))(getattr(self, self._h_name), *args))

    def set_weights(self, layer, W, b):
        """new weights of one layer from host arrays, W [out, in] (the nn.Linear layout) and b [out]; synchronises"""
        W = np.ascontiguousarray(W, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32).ravel()
        if not 0 <= int(layer) < len(self.layer_shapes) or W.shape != self.layer_shapes[layer] or b.shape != (W.shape[0],):
            raise ValueError("set_weights: layer %r takes W %s and b (%d,)" % (layer, self.layer_shapes[layer] if 0 <= int(layer) < len(self.layer_shapes) else "?", W.shape[0]))
        self._net("set_weights", int(layer), _ptr(W), _ptr(b))

    def set_weights_device(self, layer, d_W, d_b, stream=0):
        """the same from device memory in the trainer's layout (e.g. a parameter's data_ptr()), as one re-layout launch on `stream`: a
        captured graph's next replay evaluates the new weights"""
        self._net("set_weights_device", int(layer), d_W or None, d_b or None, stream or None)

    def get_weights(self, layer=None):
        """the LIVE weights as float32 numpy arrays in the nn.Linear layout: (W, b) of one layer, or with layer=None the list over all
        layers; synchronises"""
        if layer is None:
            return [self.get_weights(l) for l in range(len(self.layer_shapes))]
        if not 0 <= int(layer) < len(self.layer_shapes):
            raise ValueError("get_weights: layer is 0 .. %d" % (len(self.layer_shapes) - 1))
        W = np.zeros(self.layer_shapes[layer], dtype=np.float32)
        b = np.zeros((W.shape[0],), dtype=np.float32)
        self._net("get_weights", int(layer), _ptr(W), _ptr(b))
        return W, b

    def get_weights_device(self, layer, d_W, d_b, stream=0):
        """one layer into device memory in the trainer's layout (e.g. a parameter's data_ptr()), one launch on `stream`"""
        self._net("get_weights_device", int(layer), d_W or None, d_b or None, stream or None)

    def set_normalizer(self, mean, inv_std):
        """new mean / inv_std [F] from host arrays; synchronises"""
        mean = np.ascontiguousarray(mean, dtype=np.float32).ravel()
        inv_std = np.ascontiguousarray(inv_std, dtype=np.float32).ravel()
        if mean.shape != (self.n_features,) or inv_std.shape != (self.n_features,):
            raise ValueError("mean and inv_std must have %d entries (the %s)" % (self.n_features, self._row))
        self._net("set_normalizer", _ptr(mean), _ptr(inv_std))

    def set_normalizer_device(self, d_mean, d_inv_std, stream=0):
        """the same from device memory, [F] f32 each, as copies on `stream`: a captured graph's next replay evaluates the new normaliser"""
        self._net("set_normalizer_device", d_mean or None, d_inv_std or None, stream or None)

    def normalizer_from_moments(self, m, eps=1e-8, stream=0):
        """mean = (float) the moments' mean, inv_std = (float) (1 / sqrt(M2 / n + eps)) (the population variance), one launch on `stream`;
        moments that have counted nothing leave the normaliser alone.  Recordable into a graph."""
        self._net("normalizer_from_moments_device", m._m, float(eps), stream or None)

    def close(self):
        if getattr(self, self._h_name, None) and getattr(self._env, "_h", None):
            self._net("destroy")
        setattr(self, self._h_name, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DevicePolicy(_DeviceNet):
    """An MLP actor on the device (chub_policy_*, include/chub.h "an actor on the device"): made by VecChargingHub.make_policy.  The
    feature row (the observation and / or the feature calls' blocks) goes through the dense layers in ONE launch and comes out as action
    rows or pile bits + tail, which every step form takes; run_steps is the closed loop issued from C.  Exact f32: every product rounded
    once, f32 accumulation (an fmaf chain), the trainer's network up to summation order."""
    _c_name, _h_name, _row = "policy", "_p", "feature row"

    def __init__(self, env, layers, inputs=("obs",), head="piles", hidden_act="tanh", squash="tanh", normalize=None):
        self._env = env
        self._lib = env._lib
        layers = [(np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32).ravel()) for W, b in layers]
        mean = inv_std = None
        clip = 0.0
        if normalize is not None:
            mean, inv_std, clip = normalize
            mean = np.ascontiguousarray(mean, dtype=np.float32).ravel()
            inv_std = np.ascontiguousarray(inv_std, dtype=np.float32).ravel()
        self.spec = _lib.policy_spec([W.shape[0] if W.ndim == 2 else -1 for W, _ in layers], inputs, head, hidden_act, squash,
                                     normalize is not None, clip)
        F, A = C.c_int32(), C.c_int32()
        check(self._lib.chub_policy_input_width(C.byref(env.cfg), C.byref(self.spec), C.byref(F), C.byref(A)))
        self.n_features, self.n_outputs = F.value, A.value
        fan_in = self.n_features
        for l, (W, b) in enumerate(layers):  # (the library sees pointers only: the shapes are checked here)
            if W.shape != (self.spec.width[l], fan_in) or b.shape != (W.shape[0],):
                raise ValueError("layer %d: W must have shape (%d, %d) and b (%d,), got %s and %s"
                                 % (l, self.spec.width[l], fan_in, self.spec.width[l], W.shape, b.shape))
            fan_in = W.shape[0]
        if normalize is not None and (mean.shape != (self.n_features,) or inv_std.shape != (self.n_features,)):
            raise ValueError("normalize: mean and inv_std must have %d entries (the feature row)" % self.n_features)
        self.layer_shapes = [W.shape for W, _ in layers]
        n = len(layers)
        Wp = (C.c_void_p * n)(*[W.ctypes.data for W, _ in layers])
        bp = (C.c_void_p * n)(*[b.ctypes.data for _, b in layers])
        h = C.c_void_p()
        check(self._lib.chub_policy_create(env._h, C.byref(self.spec), Wp, bp, _ptr(mean), _ptr(inv_std), C.byref(h)))
        self._p = h

    def act_device(self, d_obs=0, ld_obs=None, d_actions=0, d_pile_bits=0, d_tail=0, d_mask=0, stream=0):
        """one evaluation on `stream`: d_obs [N] rows of obs_dim floats with row stride ld_obs floats (default obs_dim; a packed
        [N, D + 2] block: D + 2) -> d_actions [N, A] f32 and / or d_pile_bits [N, bit_words] u64 with d_tail [N, 2] f32.  d_mask [N] u8 in
        device memory: only the rows of the envs it names are written.  No synchronisation, nothing of the simulation changes,
        recordable into a graph."""
        ld = self._env.obs_dim if ld_obs is None else int(ld_obs)
        check(self._lib.chub_policy_act_device(self._env._h, self._p, d_obs or None, ld, d_mask or None, d_actions or None, d_pile_bits or None,
                                               d_tail or None, stream or None))

    def act(self, obs=None):
        """act_device through host memory: obs [N, D] -> float32 action rows [N, A] (the convenience form: it allocates, synchronises and
        copies)"""
        e = self._env
        o = None if obs is None else np.ascontiguousarray(obs, dtype=np.float32)
        if o is not None and o.shape != (e.n_envs, e.obs_dim):
            raise AssertionError("obs must have shape (%d, %d)" % (e.n_envs, e.obs_dim))
        actions = np.zeros((e.n_envs, e.act_dim), dtype=np.float32)
        check(self._lib.chub_sync(e._h))  # (calls in flight on any stream write the state the feature blocks read)
        check(self._lib.chub_policy_act(e._h, self._p, _ptr(o), _ptr(actions)))
        return actions

    def get_log_std(self, d_log_std=0, stream=0):
        """log_std [G]: as a float32 numpy array (synchronises), or with d_log_std a copy into device memory on `stream`"""
        if d_log_std:
            check(self._lib.chub_policy_get_log_std_device(self._p, d_log_std, stream or None))
            return None
        ls = np.zeros((self.n_gaussians,), dtype=np.float32)
        check(self._lib.chub_policy_get_log_std(self._p, _ptr(ls)))
        return ls

    def run_steps(self, d_packed2, n_steps, first_step=0, mode="lockstep", d_reset_obs=0, d_final_obs=0, stream=0):
        """the closed loop issued from C (chub_policy_run_steps): d_packed2 = the addresses of two [N, D + 2] f32 blocks, step i writes block
        i & 1.  mode "lockstep": a reset into d_reset_obs [N, D] before every step whose index is a multiple of 96, bits-form steps;
        "autoreset": chub_autoreset_step_device per step, the first one acting on d_reset_obs (the observation the caller holds) if given.
        Returns after enqueueing."""
        blocks = (C.c_void_p * 2)(int(d_packed2[0]), int(d_packed2[1]))
        check(self._lib.chub_policy_run_steps(self._env._h, self._p, _lib._enum_value(_lib.PRUN, mode, "run mode"), blocks, d_reset_obs or None,
                                              d_final_obs or None, int(first_step), int(n_steps), stream or None))

    # ---- sampling (include/chub.h, "sampling from the device actor")
    @property
    def n_gaussians(self):
        """G: the Gaussian outputs, 2 (the tail pair of the piles head) or 4 (the loads head)"""
        return 2 if self.spec.head == _lib.PHEAD["piles"] else 4

    def set_exploration(self, key, log_std):
        """the key of the policy's noise (a uint64) and log_std [G] of its Gaussian outputs, from host values; synchronises.  Needed once
        before sample_device / collect"""
        ls = np.ascontiguousarray(np.broadcast_to(np.asarray(log_std, dtype=np.float32), (self.n_gaussians,)))
        check(self._lib.chub_policy_set_exploration(self._p, int(key) & (2 ** 64 - 1), _ptr(ls)))
        self._explores = True

    @property
    def has_exploration(self):
        """whether set_exploration has made the policy's log_std (what get_log_std reads and an optimiser made from now on trains)"""
        return getattr(self, "_explores", False)

    def set_log_std_device(self, d_log_std, stream=0):
        """log_std [G] f32 from device memory (e.g. a parameter's data_ptr()) as a copy on `stream`: a captured graph's next replay
        samples with it"""
        check(self._lib.chub_policy_set_log_std_device(self._p, d_log_std, stream or None))

    def sample_device(self, d_obs=0, ld_obs=None, d_logp=0, d_actions=0, d_pile_bits=0, d_tail=0, d_u=0, d_features=0, d_mask=0, stream=0,
                      logp_piles=None, d_set_bits=0):
        """one SAMPLED evaluation on `stream` (chub_policy_sample_device): as act_device, with the action drawn from the actor's
        distribution under the tick of the handle's next launch (VecChargingHub.next_tick), its log-probability in d_logp [N] f32 (required),
        the pre-squash Gaussian samples in d_u [N, G] and the raw feature row in d_features [N, F].  No tick is consumed.
        logp_piles="all" | "occupied" | "decidable" (chub_policy_sample_set_device): the same draws and outputs, with d_logp counting a
        pile's term only where the pile is in that set of the current state (VecChargingHub.pile_set_device), which is also written to
        d_set_bits [N, bit_words] u64 if given."""
        ld = self._env.obs_dim if ld_obs is None else int(ld_obs)
        out = _lib.ChubPolicySampleOut(d_actions or None, d_pile_bits or None, d_tail or None, d_u or None, d_logp or None, d_features or None)
        if logp_piles is None:
            if d_set_bits:
                raise ValueError("d_set_bits needs logp_piles (the set to write)")
            check(self._lib.chub_policy_sample_device(self._env._h, self._p, d_obs or None, ld, d_mask or None, C.byref(out), stream or None))
        else:
            check(self._lib.chub_policy_sample_set_device(self._env._h, self._p, d_obs or None, ld, d_mask or None, _lib.pile_set(logp_piles),
                                                          d_set_bits or None, C.byref(out), stream or None))

    def collect(self, n_steps, d_obs0, d_packed, d_pile_bits, d_tail, d_u, d_logp, d_features=0, d_final_obs=0, first_step=0, mode="lockstep",
                stream=0, logp_piles=None, d_set_bits=0, d_terms=0, term_fields=None):
        """the closed loop that keeps the trajectory (chub_policy_collect): n_steps sampled steps into [T][N][...] arrays in device memory,
        the actor reading d_obs0 [N, D] at the first step and the packed block before it afterwards.  Returns after enqueueing.
        logp_piles="all" | "occupied" | "decidable" with d_set_bits [T, N, bit_words] u64 (chub_policy_collect_set): d_logp[t] counts the
        piles of that set in the state step t acts on, and d_set_bits[t] keeps the set.  d_terms [T, N, C] f32 with term_fields (names
        or a mask, as set_step_terms takes them): block t keeps step t's terms (chub_policy_collect_terms; telemetry must be on)."""
        r = _lib.ChubRollout(int(n_steps), d_packed or None, d_pile_bits or None, d_tail or None, d_u or None, d_logp or None, d_features or None,
                             d_final_obs or None)
        run = _lib._enum_value(_lib.PRUN, mode, "run mode")
        if d_terms or term_fields is not None:
            if logp_piles is None and d_set_bits:
                raise ValueError("d_set_bits needs logp_piles (the set to keep)")
            which = -1 if logp_piles is None else _lib.pile_set(logp_piles)
            check(self._lib.chub_policy_collect_terms(self._env._h, self._p, run, which, C.byref(r), d_set_bits or None, d_obs0 or None,
                                                      int(first_step), _lib.st_fields_mask(term_fields), d_terms or None, stream or None))
        elif logp_piles is None:
            if d_set_bits:
                raise ValueError("d_set_bits needs logp_piles (the set to keep)")
            check(self._lib.chub_policy_collect(self._env._h, self._p, run, C.byref(r), d_obs0 or None, int(first_step), stream or None))
        else:
            check(self._lib.chub_policy_collect_set(self._env._h, self._p, run, _lib.pile_set(logp_piles), C.byref(r), d_set_bits or None,
                                                    d_obs0 or None, int(first_step), stream or None))

    # ---- the normaliser read back (include/chub.h, "running feature statistics"; written and derived: _DeviceNet): policies made with normalize=
    def get_normalizer_device(self, d_mean, d_inv_std, stream=0):
        """the normaliser the policy evaluates with, copied on `stream` into d_mean / d_inv_std [F] f32 in device memory"""
        check(self._lib.chub_policy_get_normalizer_device(self._p, d_mean or None, d_inv_std or None, stream or None))

    def normalizer(self):
        """(mean, inv_std) as float32 numpy arrays (the convenience form: it allocates, synchronises and copies)"""
        e = self._env
        out = np.zeros((2, self.n_features), dtype=np.float32)
        d = C.c_void_p()
        check(self._lib.chub_malloc_device(e._device, out.nbytes, C.byref(d)))
        try:
            check(self._lib.chub_sync(e._h))  # (calls in flight on any stream may write the normaliser)
            check(self._lib.chub_policy_get_normalizer_device(self._p, d, C.c_void_p(d.value + out.nbytes // 2), None))
            check(self._lib.chub_copy_to_host(e._device, _ptr(out), d, out.nbytes, None))
        finally:
            self._lib.chub_free_device(e._device, d)
        return out[0].copy(), out[1].copy()


class DevicePopulation(object):
    """P actors on one handle (chub_population_*, include/chub.h "a population of actors"): made by VecChargingHub.make_population from a
    DevicePolicy, the centre, whose spec, normaliser and buffers it shares.  Member m serves envs [m E, (m + 1) E), E = N / P a multiple
    of 32, inside the same single actor launch per step.  perturb_device draws members 2j / 2j + 1 = theta +- sigma eps from counter-based
    noise that is never stored; es_gradient_device regenerates it: g = sum_j (util[2j] - util[2j + 1]) eps_j."""

    def __init__(self, env, policy, P, key):
        self._env = env
        self._lib = env._lib
        self.policy = policy
        self.n_members = int(P)
        self.key = int(key) & (2 ** 64 - 1)
        self.layer_shapes = list(policy.layer_shapes)
        h = C.c_void_p()
        check(self._lib.chub_population_create(policy._p, self.n_members, self.key, C.byref(h)))
        self._q = h
        self.envs_per_member = env.n_envs // self.n_members

    @property
    def n_params(self):
        """parameters per member: the sum over layers of out * (in + 1) (chub_population_param_count)"""
        n = C.c_int64()
        check(self._lib.chub_population_param_count(C.byref(self._env.cfg), C.byref(self.policy.spec), C.byref(n)))
        return n.value

    def _ptr_arrays(self, d_W, d_b):
        n = len(self.layer_shapes)
        if len(d_W) != n or len(d_b) != n:
            raise ValueError("one device address per layer: %d layers" % n)
        return (C.c_void_p * n)(*[int(p) for p in d_W]), (C.c_void_p * n)(*[int(p) for p in d_b])

    def perturb_device(self, sigma, generation, d_W=None, d_b=None, stream=0):
        """every member from theta on `stream`: members 2j / 2j + 1 = theta + / - sigma eps(generation, j).  d_W / d_b: per layer the device
        address of W [out, in] and b [out] float32 (the nn.Linear layout, e.g. data_ptr()); None: the centre policy's current weights.
        sigma and generation are host values: a captured graph replays the same ones."""
        if (d_W is None) != (d_b is None):
            raise ValueError("perturb_device: d_W and d_b are both given or both None")
        Wp, bp = (None, None) if d_W is None else self._ptr_arrays(d_W, d_b)
        check(self._lib.chub_population_perturb_device(self._q, Wp, bp, float(sigma), int(generation) & 0xFFFFFFFF, stream or None))

    def _host_layers(self, layers):
        out = [(np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32).ravel()) for W, b in layers]
        if [W.shape for W, _ in out] != self.layer_shapes or any(b.shape != (W.shape[0],) for W, b in out):
            raise ValueError("layers must be (W, b) pairs of shapes %s" % (self.layer_shapes,))
        return out

    def perturb(self, sigma, generation, layers=None):
        """perturb_device from host arrays, layers = [(W, b), ..] (None: the centre policy's weights); it allocates, copies and synchronises"""
        e = self._env
        if layers is None:
            self.perturb_device(sigma, generation)
            check(self._lib.chub_sync(e._h))
            return
        layers = self._host_layers(layers)
        flat = np.concatenate([a.ravel() for W, b in layers for a in (W, b)])
        d = C.c_void_p()
        check(self._lib.chub_malloc_device(e._device, flat.nbytes, C.byref(d)))
        try:
            check(self._lib.chub_copy_to_device(e._device, d, _ptr(flat), flat.nbytes, None))
            d_W, d_b, at = [], [], d.value
            for W, b in layers:
                d_W.append(at)
                d_b.append(at + W.nbytes)
                at += W.nbytes + b.nbytes
            self.perturb_device(sigma, generation, d_W, d_b)
            check(self._lib.chub_sync(e._h))
        finally:
            self._lib.chub_free_device(e._device, d)

    def set_member(self, m, layer, W, b):
        """member m's layer from host arrays, W [out, in] and b [out]; synchronises"""
        W = np.ascontiguousarray(W, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32).ravel()
        if not 0 <= int(layer) < len(self.layer_shapes) or W.shape != self.layer_shapes[layer] or b.shape != (W.shape[0],):
            raise ValueError("set_member: layer %r takes W %s and b of its rows" % (layer, self.layer_shapes[layer] if 0 <= int(layer) < len(self.layer_shapes) else "?"))
        check(self._lib.chub_population_set_member(self._q, int(m), int(layer), _ptr(W), _ptr(b)))

    def get_member(self, m, layer=None):
        """member m's weights as float32 numpy arrays: (W, b) of one layer, or with layer=None the list over all layers; synchronises"""
        if layer is None:
            return [self.get_member(m, l) for l in range(len(self.layer_shapes))]
        if not 0 <= int(layer) < len(self.layer_shapes):
            raise ValueError("get_member: layer is 0 .. %d" % (len(self.layer_shapes) - 1))
        W = np.zeros(self.layer_shapes[layer], dtype=np.float32)
        b = np.zeros((W.shape[0],), dtype=np.float32)
        check(self._lib.chub_population_get_member(self._q, int(m), int(layer), _ptr(W), _ptr(b)))
        return W, b

    def set_member_device(self, m, layer, d_W, d_b, stream=0):
        """member m's layer from device memory in the trainer's layout, one launch on `stream`"""
        check(self._lib.chub_population_set_member_device(self._q, int(m), int(layer), d_W or None, d_b or None, stream or None))

    def get_member_device(self, m, layer, d_W, d_b, stream=0):
        """member m's layer into device memory in the trainer's layout, one launch on `stream`"""
        check(self._lib.chub_population_get_member_device(self._q, int(m), int(layer), d_W or None, d_b or None, stream or None))

    def copy_members_device(self, d_src, d_dst, count, stream=0):
        """member dst[i] becomes a copy of member src[i] (int32 indices in device memory, count <= P) in one launch on `stream`; every source
        is read before any destination is written, so src = [0, 1], dst = [1, 0] swaps"""
        check(self._lib.chub_population_copy_members_device(self._q, d_src or None, d_dst or None, int(count), stream or None))

    def act_device(self, d_obs=0, ld_obs=None, d_actions=0, d_pile_bits=0, d_tail=0, d_mask=0, stream=0):
        """DevicePolicy.act_device with member m's weights for envs [m E, (m + 1) E): bit for bit what a policy holding them writes"""
        ld = self._env.obs_dim if ld_obs is None else int(ld_obs)
        check(self._lib.chub_population_act_device(self._env._h, self._q, d_obs or None, ld, d_mask or None, d_actions or None, d_pile_bits or None,
                                                   d_tail or None, stream or None))

    def run_steps(self, d_packed2, n_steps, first_step=0, mode="lockstep", d_reset_obs=0, d_final_obs=0, stream=0):
        """DevicePolicy.run_steps with the population's actor (chub_population_run_steps)"""
        blocks = (C.c_void_p * 2)(int(d_packed2[0]), int(d_packed2[1]))
        check(self._lib.chub_population_run_steps(self._env._h, self._q, _lib._enum_value(_lib.PRUN, mode, "run mode"), blocks, d_reset_obs or None,
                                                  d_final_obs or None, int(first_step), int(n_steps), stream or None))

    def es_gradient_device(self, d_util, generation, d_gW, d_gb, stream=0):
        """g = sum over pairs j of (util[2j] - util[2j + 1]) eps(generation, j) in f64, rounded once to float32, into d_gW[l] [out, in] and
        d_gb[l] [out] (device addresses per layer); d_util [P] float32 in device memory.  The same bits every call."""
        Wp, bp = self._ptr_arrays(d_gW, d_gb)
        check(self._lib.chub_population_es_gradient_device(self._q, d_util or None, int(generation) & 0xFFFFFFFF, Wp, bp, stream or None))

    def es_gradient(self, util, generation):
        """es_gradient_device through host memory: util [P] -> [(gW, gb), ..] float32 numpy arrays; it allocates, copies and synchronises"""
        e = self._env
        util = np.ascontiguousarray(util, dtype=np.float32).ravel()
        if util.shape != (self.n_members,):
            raise ValueError("util must have %d entries (one per member)" % self.n_members)
        out = np.zeros((self.n_params,), dtype=np.float32)
        d = C.c_void_p()
        check(self._lib.chub_malloc_device(e._device, out.nbytes + util.nbytes, C.byref(d)))
        try:
            check(self._lib.chub_copy_to_device(e._device, C.c_void_p(d.value + out.nbytes), _ptr(util), util.nbytes, None))
            d_gW, d_gb, at = [], [], d.value
            for o, i in self.layer_shapes:
                d_gW.append(at)
                d_gb.append(at + 4 * o * i)
                at += 4 * o * (i + 1)
            self.es_gradient_device(d.value + out.nbytes, generation, d_gW, d_gb)
            check(self._lib.chub_sync(e._h))
            check(self._lib.chub_copy_to_host(e._device, _ptr(out), d, out.nbytes, None))
        finally:
            self._lib.chub_free_device(e._device, d)
        res, at = [], 0
        for o, i in self.layer_shapes:
            res.append((out[at:at + o * i].reshape(o, i).copy(), out[at + o * i:at + o * (i + 1)].copy()))
            at += o * (i + 1)
        return res

    def close(self):
        if getattr(self, "_q", None) and getattr(self.policy, "_p", None) and getattr(self._env, "_h", None):
            check(self._lib.chub_population_destroy(self._q))
        self._q = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DevicePolicyGrad(object):
    """Actor gradients on the device (chub_policy_grad_*, include/chub.h "actor gradients on the device"): made by
    VecChargingHub.make_policy_grad from a DevicePolicy that has set_exploration.  grad_device differentiates a surrogate loss over rows of
    a collected rollout through the policy's LIVE weights, normaliser and log_std and writes the gradient in the trainer's layout;
    evaluate_device is the forward alone.  A handful of launches on the caller's stream, the same bits every call, no autograd."""

    def __init__(self, env, policy, max_rows):
        self._env = env
        self._lib = env._lib
        self.policy = policy
        self.max_rows = int(max_rows)
        self.layer_shapes = list(policy.layer_shapes)
        self.n_params = sum(o * (i + 1) for o, i in self.layer_shapes)
        h = C.c_void_p()
        check(self._lib.chub_policy_grad_create(policy._p, self.max_rows, C.byref(h)))
        self._g = h

    def plan(self, R=None):
        """chub_policy_grad_plan for a call of R rows (default max_rows) -> dict(n_params, workspace_bytes, workgroups, lds_rows, lds_bytes,
        in_registers); host arithmetic only"""
        out = _lib.ChubPolicyGradPlanOut()
        check(self._lib.chub_policy_grad_plan(C.byref(self._env.cfg), C.byref(self.policy.spec), int(self.max_rows if R is None else R), C.byref(out)))
        return {name: int(getattr(out, name)) for name, _ in out._fields_}

    def grad_device(self, R, n_rows, d_features, d_u, d_adv, d_pile_bits=0, d_set_bits=0, d_logp_old=0, d_rows=0, d_adv_stats=0, ld_features=None,
                    loss="ppo_clip", clip_eps=0.2, ent_coef=0.0, d_gW=None, d_gb=None, d_glog_std=0, d_logp_new=0, d_entropy=0, d_stats=0, stream=0):
        """one call on `stream` (chub_policy_grad_device).  The per-row arrays hold n_rows rows: d_features [n_rows, F] raw (row stride
        ld_features floats, default F), d_pile_bits / d_set_bits [n_rows, bit_words] u64, d_u [n_rows, G], d_logp_old, d_adv [n_rows];
        d_rows [R] int64 picks the rows (0: rows 0 .. R - 1); d_adv_stats [3] f64 normalises the advantage.  Outputs, each optional:
        d_gW[l] [out, in] / d_gb[l] [out] (device addresses per layer, the trainer's layout), d_glog_std [G], d_logp_new / d_entropy [R],
        d_stats [6] f64.  With no gradient output the call is the forward alone.  No synchronisation; recordable into a graph."""
        a = _lib.ChubPolicyGradIn(int(R), int(n_rows), d_rows or None, d_features or None,
                                  self.policy.n_features if ld_features is None else int(ld_features), d_pile_bits or None, d_set_bits or None,
                                  d_u or None, d_logp_old or None, d_adv or None, d_adv_stats or None, _lib.policy_loss(loss), float(clip_eps),
                                  float(ent_coef), 0)
        o = _lib.ChubPolicyGradOut()
        for l in range(len(self.layer_shapes)):
            o.d_gW[l] = (d_gW[l] or None) if d_gW else None
            o.d_gb[l] = (d_gb[l] or None) if d_gb else None
        o.d_glog_std, o.d_logp_new, o.d_entropy, o.d_stats = d_glog_std or None, d_logp_new or None, d_entropy or None, d_stats or None
        check(self._lib.chub_policy_grad_device(self._g, C.byref(a), C.byref(o), stream or None))

    def evaluate_device(self, R, n_rows, d_features, d_u, d_logp_new, d_entropy=0, d_pile_bits=0, d_set_bits=0, d_rows=0, ld_features=None, stream=0):
        """the forward alone ("evaluate actions"): the current policy's log-probability of the recorded actions into d_logp_new [R] and the
        entropy into d_entropy [R].  The advantage plays no part: d_u stands in for it"""
        self.grad_device(R, n_rows, d_features, d_u, d_u, d_pile_bits, d_set_bits, 0, d_rows, 0, ld_features, "coef", 0.0, 0.0, None, None, 0,
                         d_logp_new, d_entropy, 0, stream)

    def grad(self, features, u, adv, pile_bits=None, set_bits=None, logp_old=None, rows=None, adv_stats=None, loss="ppo_clip", clip_eps=0.2,
             ent_coef=0.0, backward=True):
        """grad_device through host memory (the convenience form: it allocates, copies and synchronises): numpy arrays in, ->
        dict(grads=[(gW, gb), ..], g_log_std [G], logp_new [R], entropy [R], stats [6]); backward=False: the forward alone, grads and
        g_log_std are None"""
        e, pol = self._env, self.policy
        F, G = pol.n_features, pol.n_gaussians
        features = np.ascontiguousarray(features, dtype=np.float32).reshape(-1, F)
        n_rows = len(features)
        ins = [("features", features), ("u", np.ascontiguousarray(u, dtype=np.float32).reshape(n_rows, G)),
               ("adv", np.ascontiguousarray(adv, dtype=np.float32).reshape(n_rows))]
        if pile_bits is not None:
            ins.append(("pile_bits", np.ascontiguousarray(pile_bits, dtype=np.uint64).reshape(n_rows, -1)))
        if set_bits is not None:
            ins.append(("set_bits", np.ascontiguousarray(set_bits, dtype=np.uint64).reshape(n_rows, -1)))
        if logp_old is not None:
            ins.append(("logp_old", np.ascontiguousarray(logp_old, dtype=np.float32).reshape(n_rows)))
        if rows is not None:
            ins.append(("rows", np.ascontiguousarray(rows, dtype=np.int64).ravel()))
        if adv_stats is not None:
            ins.append(("adv_stats", np.ascontiguousarray(adv_stats, dtype=np.float64).reshape(3)))
        R = n_rows if rows is None else len(dict(ins)["rows"])
        outs = [("grads", np.zeros(self.n_params + G, dtype=np.float32)), ("logp_new", np.zeros(R, dtype=np.float32)),
                ("entropy", np.zeros(R, dtype=np.float32)), ("stats", np.zeros(6, dtype=np.float64))]
        at, off = 0, {}
        for name, arr in ins + outs:
            off[name] = at
            at += (arr.nbytes + 15) & ~15
        d = C.c_void_p()
        check(self._lib.chub_malloc_device(e._device, max(at, 16), C.byref(d)))
        try:
            for name, arr in ins:
                if arr.nbytes:
                    check(self._lib.chub_copy_to_device(e._device, C.c_void_p(d.value + off[name]), _ptr(arr), arr.nbytes, None))
            d_gW, d_gb, p = [], [], d.value + off["grads"]
            for o, i in self.layer_shapes:
                d_gW.append(p)
                d_gb.append(p + 4 * o * i)
                p += 4 * o * (i + 1)
            addr = lambda name: d.value + off[name] if name in off else 0
            check(self._lib.chub_sync(e._h))
            self.grad_device(R, n_rows, addr("features"), addr("u"), addr("adv"), addr("pile_bits"), addr("set_bits"), addr("logp_old"), addr("rows"),
                             addr("adv_stats"), None, loss, clip_eps, ent_coef, d_gW if backward else None, d_gb if backward else None,
                             p if backward else 0, addr("logp_new"), addr("entropy"), addr("stats"))
            check(self._lib.chub_sync(e._h))
            for name, arr in outs:
                check(self._lib.chub_copy_to_host(e._device, _ptr(arr), C.c_void_p(d.value + off[name]), arr.nbytes, None))
        finally:
            self._lib.chub_free_device(e._device, d)
        res = dict(outs)
        flat, grads, p = res.pop("grads"), [], 0
        for o, i in self.layer_shapes:
            grads.append((flat[p:p + o * i].reshape(o, i).copy(), flat[p + o * i:p + o * (i + 1)].copy()))
            p += o * (i + 1)
        res["grads"] = grads if backward else None
        res["g_log_std"] = flat[p:p + G].copy() if backward else None
        return res

    def evaluate(self, features, u, pile_bits=None, set_bits=None, rows=None):
        """evaluate_device through host memory -> (logp_new [R], entropy [R])"""
        r = self.grad(features, u, np.zeros(len(np.asarray(u).reshape(-1, self.policy.n_gaussians)), dtype=np.float32), pile_bits, set_bits, None, rows,
                      None, "coef", 0.0, 0.0, backward=False)
        return r["logp_new"], r["entropy"]

    def close(self):
        if getattr(self, "_g", None) and getattr(self.policy, "_p", None) and getattr(self._env, "_h", None):
            check(self._lib.chub_policy_grad_destroy(self._g))
        self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceCritic(_DeviceNet):
    """A value network on the device (chub_critic_*, include/chub.h "a critic on the device"): made by VecChargingHub.make_critic.  It
    reads rows of F floats the caller points at (a rollout's features, observation blocks); values_device is the forward alone,
    grad_device the value loss and its gradient through the critic's LIVE weights and normaliser in the trainer's layout.  The actor's
    numerics, the same bits every call, no autograd."""
    _c_name, _h_name, _row = "critic", "_c", "row"

    def __init__(self, env, layers, hidden_act="tanh", normalize=None, max_rows=None):
        self._env = env
        self._lib = env._lib
        layers = [(np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32).ravel()) for W, b in layers]
        if not layers or any(W.ndim != 2 for W, _ in layers):
            raise ValueError("layers: a list of (W [out, in], b [out])")
        mean = inv_std = None
        clip = 0.0
        if normalize is not None:
            mean, inv_std, clip = normalize
            mean = np.ascontiguousarray(mean, dtype=np.float32).ravel()
            inv_std = np.ascontiguousarray(inv_std, dtype=np.float32).ravel()
        self.n_features = int(layers[0][0].shape[1])
        self.max_rows = int(env.n_envs if max_rows is None else max_rows)
        self.spec = _lib.critic_spec(self.n_features, [W.shape[0] for W, _ in layers], hidden_act, normalize is not None, clip)
        fan_in = self.n_features
        for l, (W, b) in enumerate(layers):  # (the library sees pointers only: the shapes are checked here)
            if W.shape[1] != fan_in or b.shape != (W.shape[0],):
                raise ValueError("layer %d: W must have %d columns and b %d entries, got %s and %s" % (l, fan_in, W.shape[0], W.shape, b.shape))
            fan_in = W.shape[0]
        if normalize is not None and (mean.shape != (self.n_features,) or inv_std.shape != (self.n_features,)):
            raise ValueError("normalize: mean and inv_std must have %d entries (the row)" % self.n_features)
        self.layer_shapes = [W.shape for W, _ in layers]
        self.n_params = sum(o * (i + 1) for o, i in self.layer_shapes)
        n = len(layers)
        Wp = (C.c_void_p * n)(*[W.ctypes.data for W, _ in layers])
        bp = (C.c_void_p * n)(*[b.ctypes.data for _, b in layers])
        h = C.c_void_p()
        check(self._lib.chub_critic_create(env._h, C.byref(self.spec), Wp, bp, _ptr(mean), _ptr(inv_std), self.max_rows, C.byref(h)))
        self._c = h

    def plan(self, R=None):
        """chub_critic_plan for a call of R rows (default max_rows) -> dict(n_params, workspace_bytes, workgroups, lds_rows, lds_bytes,
        in_registers); host arithmetic only"""
        out = _lib.ChubCriticPlanOut()
        check(self._lib.chub_critic_plan(C.byref(self.spec), int(self.max_rows if R is None else R), C.byref(out)))
        return {name: int(getattr(out, name)) for name, _ in out._fields_}

    def values_device(self, R, n_rows, d_x, d_values, d_rows=0, ld=None, stream=0):
        """the forward alone on `stream` (chub_critic_values_device): d_x holds n_rows rows of F floats with row stride ld floats (default
        F), d_rows [R] int64 picks them (0: rows 0 .. R - 1), V goes to d_values [R] f32 at position r.  One launch, no synchronisation;
        recordable into a graph."""
        check(self._lib.chub_critic_values_device(self._c, d_x or None, self.n_features if ld is None else int(ld), int(n_rows), d_rows or None, int(R),
                                                  d_values or None, stream or None))

    def grad_device(self, R, n_rows, d_x, d_ret, d_v_old=0, d_rows=0, ld=None, loss="mse", clip_eps=0.2, d_gW=None, d_gb=None, d_values=0, d_stats=0,
                    stream=0):
        """one call on `stream` (chub_critic_grad_device): the value loss over rows of d_x against d_ret [n_rows] (and d_v_old [n_rows] under
        loss="clipped").  Outputs, each optional: d_gW[l] [out, in] / d_gb[l] [out] (device addresses per layer, the trainer's layout),
        d_values [R], d_stats [6] f64 (rows, loss terms, clipped rows, sum (ret - v)^2, sum ret, sum ret^2).  With no gradient output the
        call is the forward plus stats.  No synchronisation; recordable into a graph."""
        a = _lib.ChubCriticGradIn(int(R), int(n_rows), d_rows or None, d_x or None, self.n_features if ld is None else int(ld), d_ret or None,
                                  d_v_old or None, _lib.value_loss(loss), float(clip_eps))
        o = _lib.ChubCriticGradOut()
        for l in range(len(self.layer_shapes)):
            o.d_gW[l] = (d_gW[l] or None) if d_gW else None
            o.d_gb[l] = (d_gb[l] or None) if d_gb else None
        o.d_values, o.d_stats = d_values or None, d_stats or None
        check(self._lib.chub_critic_grad_device(self._c, C.byref(a), C.byref(o), stream or None))

    def _through_host(self, ins, outs, call):
        """device memory for named numpy arrays, the inputs copied in, call(addr), the outputs copied back"""
        e = self._env
        at, off = 0, {}
        for name, arr in ins + outs:
            off[name] = at
            at += (arr.nbytes + 15) & ~15
        d = C.c_void_p()
        check(self._lib.chub_malloc_device(e._device, max(at, 16), C.byref(d)))
        try:
            for name, arr in ins:
                if arr.nbytes:
                    check(self._lib.chub_copy_to_device(e._device, C.c_void_p(d.value + off[name]), _ptr(arr), arr.nbytes, None))
            check(self._lib.chub_sync(e._h))
            call(lambda name: d.value + off[name] if name in off else 0)
            check(self._lib.chub_sync(e._h))
            for name, arr in outs:
                check(self._lib.chub_copy_to_host(e._device, _ptr(arr), C.c_void_p(d.value + off[name]), arr.nbytes, None))
        finally:
            self._lib.chub_free_device(e._device, d)

    def values(self, x, rows=None):
        """values_device through host memory (the convenience form: it allocates, copies and synchronises): x [n_rows, F] -> V [R] f32"""
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, self.n_features)
        ins = [("x", x)]
        if rows is not None:
            ins.append(("rows", np.ascontiguousarray(rows, dtype=np.int64).ravel()))
        R = len(x) if rows is None else len(ins[1][1])
        v = np.zeros(R, dtype=np.float32)
        self._through_host(ins, [("values", v)], lambda addr: self.values_device(R, len(x), addr("x"), addr("values"), addr("rows")))
        return v

    def grad(self, x, ret, v_old=None, rows=None, loss="mse", clip_eps=0.2, backward=True):
        """grad_device through host memory -> dict(grads=[(gW, gb), ..] or None, values [R], stats [6])"""
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, self.n_features)
        n_rows = len(x)
        ins = [("x", x), ("ret", np.ascontiguousarray(ret, dtype=np.float32).reshape(n_rows))]
        if v_old is not None:
            ins.append(("v_old", np.ascontiguousarray(v_old, dtype=np.float32).reshape(n_rows)))
        if rows is not None:
            ins.append(("rows", np.ascontiguousarray(rows, dtype=np.int64).ravel()))
        R = n_rows if rows is None else len(dict(ins)["rows"])
        flat, v, stats = np.zeros(self.n_params, dtype=np.float32), np.zeros(R, dtype=np.float32), np.zeros(6, dtype=np.float64)

        def call(addr):
            d_gW, d_gb, p = [], [], addr("grads")
            for o, i in self.layer_shapes:
                d_gW.append(p)
                d_gb.append(p + 4 * o * i)
                p += 4 * o * (i + 1)
            self.grad_device(R, n_rows, addr("x"), addr("ret"), addr("v_old"), addr("rows"), None, loss, clip_eps, d_gW if backward else None,
                             d_gb if backward else None, addr("values"), addr("stats"))

        self._through_host(ins, [("grads", flat), ("values", v), ("stats", stats)], call)
        grads, p = [], 0
        for o, i in self.layer_shapes:
            grads.append((flat[p:p + o * i].reshape(o, i).copy(), flat[p + o * i:p + o * (i + 1)].copy()))
            p += o * (i + 1)
        return {"grads": grads if backward else None, "values": v, "stats": stats}

    def set_normalizer_device(self, d_mean, d_inv_std, stream=0):
        """the same from device memory, [F] f32 each, as copies on `stream`"""
        _DeviceNet.set_normalizer_device(self, d_mean, d_inv_std, stream)

    def normalizer_from_moments(self, m, eps=1e-8, stream=0):
        """mean = (float) the moments' mean, inv_std = (float) (1 / sqrt(M2 / n + eps)), one launch on `stream`, as the policy's; recordable"""
        _DeviceNet.normalizer_from_moments(self, m, eps, stream)


class DeviceAdam(object):
    """Adam with gradient clipping on the device (chub_adam_*, include/chub.h "an optimiser on the device"): made by
    VecChargingHub.make_adam for a DevicePolicy or a DeviceCritic.  The parameters are the target's LIVE device weights: a step reads
    gradients in the trainer's layout and writes the new weights straight into the kernels' layout, two launches, the same bits every
    time.  The flat parameter vector (and m, v) is W[0], b[0], W[1], b[1], .., then the policy's log_std."""

    def __init__(self, env, target, hyper):
        self._env = env
        self._lib = env._lib
        self.target = target
        h = C.c_void_p()
        if isinstance(target, DevicePolicy):
            check(self._lib.chub_adam_create_policy(target._p, C.byref(hyper), C.byref(h)))
        elif isinstance(target, DeviceCritic):
            check(self._lib.chub_adam_create_critic(target._c, C.byref(hyper), C.byref(h)))
        else:
            raise TypeError("make_adam: a DevicePolicy or a DeviceCritic")
        self._a = h
        self.layer_shapes = list(target.layer_shapes)
        size = C.c_int64()
        check(self._lib.chub_adam_state_size(self._a, C.byref(size)))
        self.state_bytes = size.value
        self.n_params = (size.value - 32) // 8
        gW, gb, gl = (C.c_void_p * 4)(), (C.c_void_p * 4)(), C.c_void_p()
        check(self._lib.chub_adam_grads(self._a, gW, gb, C.byref(gl)))
        n = len(self.layer_shapes)
        self._grads = ([gW[l] or 0 for l in range(n)], [gb[l] or 0 for l in range(n)], gl.value or 0)
        t = C.c_void_p()
        check(self._lib.chub_adam_counter_device(self._a, C.byref(t)))
        self.counter_address = t.value

    @property
    def has_log_std(self):
        return self._grads[2] != 0

    def grads(self):
        """(d_gW [layers], d_gb [layers], d_glog_std or 0): device addresses into the optimiser's own gradient buffer, the trainer's
        layout in the flat order -- what a gradient call writes there needs no allocation by the caller"""
        return list(self._grads[0]), list(self._grads[1]), self._grads[2]

    def step_device(self, d_gW=None, d_gb=None, d_glog_std=None, d_stats=0, stream=0):
        """one step on `stream` (chub_adam_step_device) from gradients at these device addresses (default: the optimiser's own buffers);
        d_stats [4] f64: t, the gradient's norm, the clip scale, 1 where the step was skipped (a norm that is not finite).  Two launches,
        no synchronisation; recordable into a graph, whose replays advance t, the bias corrections and the moments by themselves."""
        n = len(self.layer_shapes)
        gW = self._grads[0] if d_gW is None else d_gW
        gb = self._grads[1] if d_gb is None else d_gb
        gl = self._grads[2] if d_glog_std is None else d_glog_std
        Wp = (C.c_void_p * 4)(*[(gW[l] or None) for l in range(n)])
        bp = (C.c_void_p * 4)(*[(gb[l] or None) for l in range(n)])
        check(self._lib.chub_adam_step_device(self._a, Wp, bp, gl or None, d_stats or None, stream or None))

    def set_gate(self, d_gate):
        """point the optimiser at an int64 word in device memory (a DeviceTrainLog's gate_address), or 0 / None for none
        (chub_adam_set_gate): where the word is not 0 a step keeps every bit of weights and state and writes stats [t, norm, 0, 2]"""
        check(self._lib.chub_adam_set_gate(self._a, d_gate or None))

    def set_hyper(self, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0):
        """new hyper-parameters from host values; synchronises"""
        check(self._lib.chub_adam_set_hyper(self._a, C.byref(_lib.adam_hyper(lr, betas, eps, weight_decay, max_grad_norm))))

    def set_lr_device(self, d_lr, stream=0):
        """lr from one f64 in device memory, as a copy on `stream`: a schedule inside a graph"""
        check(self._lib.chub_adam_set_lr_device(self._a, d_lr or None, stream or None))

    def reset_device(self, stream=0):
        """m = v = 0, t = 0, the bias corrections' products back to 1, on `stream`"""
        check(self._lib.chub_adam_reset_device(self._a, stream or None))

    def state(self):
        """the state blob as bytes: int64 t, f64 p1, f64 p2, int64 n, m [n] f32, v [n] f32; synchronises"""
        blob = np.zeros(self.state_bytes, dtype=np.uint8)
        check(self._lib.chub_adam_get_state(self._a, _ptr(blob)))
        return blob.tobytes()

    def load_state(self, blob):
        """a state() blob back (of an optimiser with as many parameters); synchronises"""
        buf = np.frombuffer(bytes(blob), dtype=np.uint8)
        if buf.size != self.state_bytes:
            raise ValueError("load_state: a blob of %d bytes, this optimiser's has %d" % (buf.size, self.state_bytes))
        check(self._lib.chub_adam_set_state(self._a, _ptr(buf)))

    def close(self):
        if getattr(self, "_a", None) and getattr(self._env, "_h", None) and (getattr(self.target, "_p", None) or getattr(self.target, "_c", None)):
            check(self._lib.chub_adam_destroy(self._a))  # (a closed target has destroyed its optimisers already)
        self._a = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceTrainLog(object):
    """The numbers of a PPO update and its KL stop, kept on the device (chub_train_log_*, include/chub.h "a training log and a KL stop on
    the device"): made by VecChargingHub.make_train_log.  begin, record and steps are one small launch each on the caller's stream,
    recordable into a graph; read is the one synchronising copy.  gate_address is the word DeviceAdam.set_gate takes."""

    def __init__(self, env):
        self._env = env
        self._lib = env._lib
        h = C.c_void_p()
        check(self._lib.chub_train_log_create(env._h, C.byref(h)))
        self._t = h
        w, g = C.c_void_p(), C.c_void_p()
        check(self._lib.chub_train_log_device(self._t, C.byref(w), C.byref(g)))
        self.words_address, self.gate_address = w.value, g.value

    def begin(self, stream=0):
        """every word 0, the stop index -1, the gate 0 (chub_train_log_begin_device)"""
        check(self._lib.chub_train_log_begin_device(self._t, stream or None))

    def record(self, d_pstats=0, d_cstats=0, kl="k3", kl_limit=0.0, stream=0):
        """one minibatch, after its two gradient calls and before its steps (chub_train_log_record_device): d_pstats / d_cstats are the
        stats blocks [6] f64 of DevicePolicyGrad.grad_device / DeviceCritic.grad_device (0: none).  kl_limit > 0 stops the update at the
        first minibatch whose estimate is not <= kl_limit."""
        check(self._lib.chub_train_log_record_device(self._t, d_pstats or None, d_cstats or None, _lib.kl_kind(kl), float(kl_limit), stream or None))

    def steps(self, d_astats_actor=0, d_astats_critic=0, stream=0):
        """after the minibatch's optimiser steps (chub_train_log_steps_device), on their stats blocks [4] f64 (0: none)"""
        check(self._lib.chub_train_log_steps_device(self._t, d_astats_actor or None, d_astats_critic or None, stream or None))

    def read(self):
        """the words -> float64 [TLOG_WORDS] (the layout: _lib.TLOG); synchronises"""
        words = np.zeros(_lib.TLOG_WORDS, dtype=np.float64)
        check(self._lib.chub_train_log_read(self._t, _ptr(words)))
        return words

    def close(self):
        if getattr(self, "_t", None) and getattr(self._env, "_h", None):
            check(self._lib.chub_train_log_destroy(self._t))
        self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def train_log_fold(words, gate, pstats=None, cstats=None, kl="k3", kl_limit=0.0):
    """the record step on host memory (chub_train_log_fold; no device): words float64 [TLOG_WORDS] and gate int64 [1] are updated in place"""
    assert words.dtype == np.float64 and words.size == _lib.TLOG_WORDS and gate.dtype == np.int64 and gate.size == 1
    ps = None if pstats is None else np.ascontiguousarray(pstats, dtype=np.float64)
    cs = None if cstats is None else np.ascontiguousarray(cstats, dtype=np.float64)
    check(_lib.load_library().chub_train_log_fold(_ptr(words), _ptr(gate), None if ps is None else _ptr(ps), None if cs is None else _ptr(cs),
                                                  _lib.kl_kind(kl), float(kl_limit)))


class DeviceLagrange(object):
    """K = 1 .. 4 constraints with their Lagrange multipliers on the device (chub_lagrange_*, include/chub.h "constrained PPO on the
    device"): made by VecChargingHub.make_lagrange.  gae, step and combine enqueue on the caller's stream and are recordable into a
    graph; read is the one synchronising copy.  constraints: dicts or tuples (column, kind, limit, lr, lambda0, lambda_max) with column
    the index within the rows of the terms array gae is given and kind "step" | "done"."""

    def __init__(self, env, constraints):
        self._env = env
        self._lib = env._lib
        rows = [c if isinstance(c, dict) else dict(zip(("column", "kind", "limit", "lr", "lambda0", "lambda_max"), c)) for c in constraints]
        self.K = len(rows)
        arr = (_lib.ChubConstraint * max(self.K, 1))()
        for k, c in enumerate(rows):
            arr[k] = _lib.ChubConstraint(int(c["column"]), _lib.cost_kind(c.get("kind", "step")), float(c.get("limit", 0.0)), float(c.get("lr", 0.0)),
                                         float(c.get("lambda0", 0.0)), float(c.get("lambda_max", 0.0)))
        self.constraints = [dict(column=a.column, kind=a.kind, limit=a.limit, lr=a.lr, lambda0=a.lambda0, lambda_max=a.lambda_max) for a in arr[:self.K]]
        h = C.c_void_p()
        check(self._lib.chub_lagrange_create(env._h, self.K, arr, C.byref(h)))
        self._g = h
        lam, st = C.c_void_p(), C.c_void_p()
        check(self._lib.chub_lagrange_device(self._g, C.byref(lam), C.byref(st)))
        self.lambda_address, self.stats_address = lam.value, st.value

    @staticmethod
    def _four(addresses, K):
        a = list(addresses) if addresses else []
        if len(a) > K:
            raise ValueError("%d addresses for %d constraints" % (len(a), K))
        return (C.c_void_p * 4)(*[x or None for x in a + [0] * (4 - len(a))])

    def gae(self, n_steps, n_columns, d_terms, d_packed, d_adv, d_ret=None, d_values=None, d_final_values=None, gamma=0.99, lam=0.95, d_mask=0,
            d_ep_carry=0, stream=0):
        """cost advantages, cost returns and episode costs of a collected rollout (chub_lagrange_gae_device): d_terms [T, N, n_columns]
        f32, d_packed [T, N, D + 2] (only done is read); per constraint d_adv[k] [T, N] (required), d_ret[k] [T, N], d_values[k]
        [T + 1, N] (none: V = 0) and d_final_values[k] [N] as sequences of device addresses; d_ep_carry [N, K] f64 carries the cost of
        the episodes still open from call to call.  The stats block is written by the second of the two launches."""
        g = _lib.ChubCostGae()
        g.T, g.C, g.d_terms, g.d_packed, g.d_mask = int(n_steps), int(n_columns), d_terms or None, d_packed or None, d_mask or None
        g.d_values, g.d_final_values = self._four(d_values, self.K), self._four(d_final_values, self.K)
        g.d_adv, g.d_ret = self._four(d_adv, self.K), self._four(d_ret, self.K)
        g.gamma, g.lam, g.d_ep_carry = float(gamma), float(lam), d_ep_carry or None
        check(self._lib.chub_lagrange_gae_device(self._g, C.byref(g), stream or None))

    def step(self, stream=0):
        """projected dual ascent on every multiplier from the stats the last gae left (chub_lagrange_step_device): one launch"""
        check(self._lib.chub_lagrange_step_device(self._g, stream or None))

    def combine(self, n, d_adv, d_adv_cost, d_out, d_adv_stats=0, stream=0):
        """d_out [n] = (normalised advantage - sum_k lambda_k (cost advantage_k - its mean)) / (1 + sum_k lambda_k)
        (chub_lagrange_combine_device): what grad_device / ppo_update take as d_adv with no d_adv_stats.  d_out may be d_adv."""
        if len(d_adv_cost) != self.K:
            raise ValueError("%d cost advantages for %d constraints" % (len(d_adv_cost), self.K))
        arr = (C.c_void_p * 4)(*[x or None for x in list(d_adv_cost) + [0] * (4 - self.K)])
        check(self._lib.chub_lagrange_combine_device(self._g, int(n), d_adv or None, d_adv_stats or None, arr, d_out or None, stream or None))

    def set_lambda_device(self, d_lambda, stream=0):
        """the multipliers from K f64 words in device memory (chub_lagrange_set_lambda_device): one launch"""
        check(self._lib.chub_lagrange_set_lambda_device(self._g, d_lambda or None, stream or None))

    def read(self):
        """(lambda [K], stats [K, 6], words [K, 3] = J_last, steps taken, steps skipped) as float64; synchronises"""
        lam, st, w = np.zeros(self.K), np.zeros((self.K, _lib.LAG_STATS)), np.zeros((self.K, _lib.LAG_WORDS))
        check(self._lib.chub_lagrange_read(self._g, _ptr(lam), _ptr(st), _ptr(w)))
        return lam, st, w

    def get_state(self):
        """lambda and the counters as bytes, for a checkpoint (chub_lagrange_get_state); synchronises"""
        n = C.c_int64()
        check(self._lib.chub_lagrange_state_size(self._g, C.byref(n)))
        blob = np.zeros(n.value, dtype=np.uint8)
        check(self._lib.chub_lagrange_get_state(self._g, _ptr(blob)))
        return blob.tobytes()

    def set_state(self, blob):
        """get_state's bytes back (chub_lagrange_set_state): a blob of another K is refused"""
        n = C.c_int64()
        check(self._lib.chub_lagrange_state_size(self._g, C.byref(n)))
        b = np.frombuffer(bytes(blob), dtype=np.uint8).copy()
        if b.size < 8:
            raise ValueError("set_state: not a state blob (%d bytes)" % b.size)
        if int(b[:8].view(np.int64)[0]) == self.K and b.size != n.value:  # (another K: the library refuses it, from the first word alone)
            raise ValueError("set_state: %d bytes, this object's state has %d" % (b.size, n.value))
        check(self._lib.chub_lagrange_set_state(self._g, _ptr(b)))

    def close(self):
        if getattr(self, "_g", None) and getattr(self._env, "_h", None):
            check(self._lib.chub_lagrange_destroy(self._g))
        self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lagrange_fold(constraint, lam, words, stats):
    """the multiplier's step on host memory for one constraint (chub_lagrange_fold; no device): lam float64 [1] and words float64 [3]
    (J_last, taken, skipped) are updated in place from stats float64 [6]"""
    assert lam.dtype == np.float64 and lam.size == 1 and words.dtype == np.float64 and words.size == 3
    st = np.ascontiguousarray(stats, dtype=np.float64)
    assert st.size == _lib.LAG_STATS
    c = _lib.ChubConstraint(int(constraint.get("column", 0)), _lib.cost_kind(constraint.get("kind", "step")), float(constraint.get("limit", 0.0)),
                            float(constraint.get("lr", 0.0)), float(constraint.get("lambda0", 0.0)), float(constraint.get("lambda_max", 0.0)))
    check(_lib.load_library().chub_lagrange_fold(C.byref(c), _ptr(lam), _ptr(words), _ptr(st)))


class DeviceReturnNorm(object):
    """Reward scaling by the running spread of the discounted return (chub_return_norm_*, include/chub.h "reward scaling on the device";
    stable-baselines' VecNormalize with norm_reward): made by VecChargingHub.make_return_norm.  update_device, gae_device and the two
    resets enqueue on the caller's stream and are recordable into a graph; state, scale and get_state / set_state synchronise."""

    def __init__(self, env, gamma=0.99, eps=1e-8, clip=10.0):
        self._env = env
        self._lib = env._lib
        self.gamma, self.eps, self.clip = float(gamma), float(eps), float(clip)
        spec = _lib.ChubReturnNormSpec(self.gamma, self.clip, self.eps)
        h = C.c_void_p()
        check(self._lib.chub_return_norm_create(env._h, C.byref(spec), C.byref(h)))
        self._g = h
        st, sc, ca = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(self._lib.chub_return_norm_device(self._g, C.byref(st), C.byref(sc), C.byref(ca)))
        self.state_address, self.scale_address, self.carry_address = st.value, sc.value, ca.value

    def update_device(self, n_steps, d_packed, d_mask=0, stream=0):
        """a rollout's blocks d_packed [T, N, D + 2] into the running state, then the scale (chub_return_norm_update_device): two launches"""
        check(self._lib.chub_return_norm_update_device(self._g, d_packed or None, int(n_steps), d_mask or None, stream or None))

    def gae_device(self, n_steps, d_packed, d_values, d_adv, d_ret=0, d_final_values=0, gamma=0.99, lam=0.95, d_mask=0, d_stats=0, stream=0):
        """VecChargingHub.rollout_gae with every reward multiplied by the object's scale word and clipped (chub_return_norm_gae_device)"""
        g = _lib.ChubGae(int(n_steps), d_packed or None, d_values or None, d_final_values or None, d_mask or None, float(gamma), float(lam),
                         d_adv or None, d_ret or None, d_stats or None)
        check(self._lib.chub_return_norm_gae_device(self._g, C.byref(g), stream or None))

    def reset_carry_device(self, d_mask=0, stream=0):
        """the carried return of the named envs (none: all) back to 0 (chub_return_norm_reset_carry_device)"""
        check(self._lib.chub_return_norm_reset_carry_device(self._g, d_mask or None, stream or None))

    def reset_device(self, stream=0):
        """state, scale and carry to empty (chub_return_norm_reset_device)"""
        check(self._lib.chub_return_norm_reset_device(self._g, stream or None))

    def get_state(self):
        """the state, the scale and the carry as bytes, for a checkpoint (chub_return_norm_get_state); synchronises"""
        n = C.c_int64()
        check(self._lib.chub_return_norm_state_size(self._g, C.byref(n)))
        blob = np.zeros(n.value, dtype=np.uint8)
        check(self._lib.chub_return_norm_get_state(self._g, _ptr(blob)))
        return blob.tobytes()

    def set_state(self, blob):
        """get_state's bytes back (chub_return_norm_set_state): a blob of another N is refused"""
        n = C.c_int64()
        check(self._lib.chub_return_norm_state_size(self._g, C.byref(n)))
        b = np.frombuffer(bytes(blob), dtype=np.uint8).copy()
        if b.size < _lib.RETURN_NORM_BLOB_HEAD:
            raise ValueError("set_state: not a state blob (%d bytes)" % b.size)
        N = int(b[8:16].view(np.int64)[0])
        if int(b[:8].view(np.uint64)[0]) == _lib.RETURN_NORM_MAGIC and b.size != _lib.RETURN_NORM_BLOB_HEAD + 4 * max(N, 0):
            raise ValueError("set_state: %d bytes, a blob of N = %d has %d" % (b.size, N, _lib.RETURN_NORM_BLOB_HEAD + 4 * max(N, 0)))
        check(self._lib.chub_return_norm_set_state(self._g, _ptr(b)))  # (another magic or another N: the library refuses it, from the head alone)

    def _head(self):
        b = np.frombuffer(self.get_state(), dtype=np.uint8)
        return b[16:40].view(np.float64).copy(), b[40:44].view(np.float32)[0], b[_lib.RETURN_NORM_BLOB_HEAD:].view(np.float32).copy()

    def state(self):
        """(n, mean, M2) as float64 [3]; synchronises"""
        return self._head()[0]

    def scale(self):
        """scale32 as numpy float32; synchronises"""
        return self._head()[1]

    def carry(self):
        """the carried return per env, float32 [N]; synchronises"""
        return self._head()[2]

    def close(self):
        if getattr(self, "_g", None) and getattr(self._env, "_h", None):
            check(self._lib.chub_return_norm_destroy(self._g))
        self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def return_norm_fold(state, n_b, K, S1, S2, eps=1e-8):
    """the merge of a call's sums into the running state and the scale that follows, on host memory (chub_return_norm_fold; no device):
    state float64 [3] = (n, mean, M2) is updated in place; returns scale32, or None where n_b == 0 wrote nothing"""
    assert state.dtype == np.float64 and state.size == 3 and state.flags.c_contiguous
    sc = np.full(1, np.nan, dtype=np.float32)
    check(_lib.load_library().chub_return_norm_fold(_ptr(state), _ptr(sc), float(n_b), float(K), float(S1), float(S2), float(eps)))
    return None if not n_b > 0 else sc[0]


def ppo_update_plan(n_rows, minibatch_rows):
    """(minibatches per epoch, rows of the last one) of ppo_update's split (chub_ppo_update_plan; host arithmetic only)"""
    m, last = C.c_int64(), C.c_int64()
    check(_lib.load_library().chub_ppo_update_plan(int(n_rows), int(minibatch_rows), C.byref(m), C.byref(last)))
    return m.value, last.value


class DeviceMoments(object):
    """Running count, mean and M2 per feature on the device (chub_moments_*, include/chub.h "running feature statistics"): made by
    VecChargingHub.make_moments.  The state is [1 + 2 F] float64 in device memory (n | mean | M2); update_device adds a batch of rows in
    two launches with every sum's order fixed (the same bits every call), pivoted so that a constant column has M2 == 0 exactly."""

    def __init__(self, env, F):
        self._env = env
        self._lib = env._lib
        self.n_features = int(F)
        h = C.c_void_p()
        check(self._lib.chub_moments_create(env._h, self.n_features, C.byref(h)))
        self._m = h

    def update_device(self, d_x, rows, ld=None, d_mask=0, stream=0):
        """add `rows` rows of F float32 with row stride ld floats (default F) in device memory.  d_mask [N] u8 in device memory: row r
        belongs to env r % N and only the rows of the envs it names count.  No synchronisation, recordable into a graph."""
        ld = self.n_features if ld is None else int(ld)
        check(self._lib.chub_moments_update_device(self._m, d_x or None, ld, int(rows), d_mask or None, stream or None))

    def reset_device(self, stream=0):
        """the state back to zeros, on `stream`"""
        check(self._lib.chub_moments_reset_device(self._m, stream or None))

    def get_raw(self):
        """(count, mean [F], M2 [F]) as the state holds them, float64; synchronises"""
        n = C.c_double()
        mean = np.zeros((self.n_features,), dtype=np.float64)
        m2 = np.zeros((self.n_features,), dtype=np.float64)
        check(self._lib.chub_moments_get(self._m, C.byref(n), _ptr(mean), _ptr(m2)))
        return n.value, mean, m2

    def get(self):
        """(count, mean [F], var [F]) with var = M2 / count, the population variance (zeros while nothing is counted); synchronises"""
        n, mean, m2 = self.get_raw()
        return n, mean, (m2 / n if n > 0 else np.zeros_like(m2))

    def set(self, count, mean, var=None, m2=None):
        """the state from host values (a checkpoint): count, mean [F] and either var [F] (M2 = var * count) or m2 [F] itself, which
        get_raw() round-trips bit for bit; synchronises"""
        if (var is None) == (m2 is None):
            raise ValueError("set: exactly one of var and m2")
        mean = np.ascontiguousarray(mean, dtype=np.float64).ravel()
        m2 = np.ascontiguousarray(np.asarray(var, dtype=np.float64) * float(count) if m2 is None else m2, dtype=np.float64).ravel()
        if mean.shape != (self.n_features,) or m2.shape != (self.n_features,):
            raise ValueError("set: mean and var / m2 must have %d entries" % self.n_features)
        check(self._lib.chub_moments_set(self._m, float(count), _ptr(mean), _ptr(m2)))

    @property
    def state_ptr(self):
        """the device address of the state, [1 + 2 F] float64: n | mean | M2 (it never moves)"""
        p = C.c_void_p()
        check(self._lib.chub_moments_state_device(self._m, C.byref(p)))
        return p.value

    def close(self):
        if getattr(self, "_m", None) and getattr(self._env, "_h", None):
            check(self._lib.chub_moments_destroy(self._m))
        self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VecChargingHub(object):
    def __init__(self, n_envs, station_list, station_type_list, seed=0, rng="philox", device=0, env_id0=0,
                 data_dir=None, slot_kernel="auto", no_arena=False, copy_outputs=True, fused_step="auto", tile="auto", walk_ahead="auto",
                 work_order="auto", span_steps="auto", span_tails="auto", **kwargs):
        """slot_kernel: PHILOX handles: "auto" (the packed slot kernel wherever the hub shape allows), "wave" (the wave-local one for
        every step) or "packed"; COMPAT handles: "auto" / "packed" the split step (stream walks one env per lane, one slot pass over both
        stations), "wave" one kernel per station (bit-identical); no_arena: one device allocation per array (no snapshots) -- chub_options.
        copy_outputs=False: reset() / step() return the handle's own pinned arrays (valid until the next call) instead of
        fresh copies -- at 65 536 envs the copies are a third of a host-pointer step."""
        kwargs.pop("seed_rand", None)
        kwargs.pop("use_lagrange", None)  # ignored by the reference too (MGR:126)
        self._lib = load_library()
        self.n_envs = int(n_envs)
        # any of the eight hydrogen / FCEV / fluctuation kwargs may be a sequence of one value per env (chub_create_params)
        scalar_kwargs, rows = split_env_params(self.n_envs, kwargs)
        self.cfg = make_config(station_list, station_type_list, **scalar_kwargs)
        if rng not in _lib.RNG_MODES:
            raise ValueError("rng must be 'philox', 'compat' or 'philox_curves'")
        self.rng_mode = _lib.RNG_MODES[rng]
        h = C.c_void_p()
        opt = ChubOptions()
        opt.slot_kernel = _lib.SLOT_KERNELS[slot_kernel]
        opt.no_arena = int(bool(no_arena))
        opt.fused_step = _lib.FUSED_STEP[fused_step]  # "auto": one launch per step for small batches; "off" / "on" (parity cross-check)
        opt.tile = _lib.TILES[tile]  # packed slot kernel: "auto" (by working-set size), "small" (256 x 2) or "large" (512 x 4)
        opt.walk_ahead = _lib.WALK_AHEAD[walk_ahead]  # COMPAT batches: "auto" (step i + 1's stream walks beside step i's tails) or "off"
        opt.span_steps = 0 if span_steps == "auto" else (1 if span_steps == "off" else int(span_steps))  # chub_run_steps: steps per launch (one-launch handles); two-launch handles: pairs of steps with ONE tail launch ("auto": large batches, "off", 2: always)
        opt.span_tails = {"auto": 0, "same_wave": 1, "own_wave": 2}[span_tails]  # ... and the wave a span's tails run on (own_wave: a step behind the slots)
        opt.work_order = _lib.WORK_ORDER[work_order]  # PHILOX packed kernels: "auto" (XCD-aware while the streams are cache-resident) or "dispatch"
        self._copy_outputs = bool(copy_outputs)
        if rows is None:
            check(self._lib.chub_create_ex(C.byref(self.cfg), (data_dir or _lib.DATA_DIR).encode(), self.n_envs, int(env_id0),
                                           int(device), int(seed) & 0xFFFFFFFFFFFFFFFF, self.rng_mode, C.byref(opt), C.byref(h)))
        else:
            check(self._lib.chub_create_params(C.byref(self.cfg), (data_dir or _lib.DATA_DIR).encode(), self.n_envs, int(env_id0),
                                               int(device), int(seed) & 0xFFFFFFFFFFFFFFFF, self.rng_mode, C.byref(opt), _ptr(rows),
                                               C.byref(h)))
        self._h = h
        self.obs_dim = self._lib.chub_obs_dim(h)
        self.act_dim = self._lib.chub_act_dim(h)
        self.n_slots = self.act_dim - 2
        self.piles = (int(station_list[0]), int(station_list[1]))
        self._device = int(device)
        self._host_allocs = []
        # the arrays the host-pointer entry points write into: pinned, so that the copies back are plain DMA
        self._obs = self._pinned_array((self.n_envs, self.obs_dim), np.float32)
        self._reward = self._pinned_array((self.n_envs,), np.float32)
        self._done = self._pinned_array((self.n_envs,), np.uint8)

    def _pinned_array(self, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        check(self._lib.chub_alloc_host(self._device, max(n, 1), C.byref(p)))
        self._host_allocs.append(p.value)
        buf = (C.c_char * max(n, 1)).from_address(p.value)
        a = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        a[...] = 0
        return a

    def _out(self):
        if self._copy_outputs:
            return self._obs.copy(), self._reward.copy(), self._done.astype(bool), {}
        return self._obs, self._reward, self._done.view(np.bool_), {}

    # ---- hot path
    def reset(self, exo_days=None, exo_z=None):
        d = None if exo_days is None else np.ascontiguousarray(exo_days, dtype=np.int32).reshape(self.n_envs, 2)
        z = None if exo_z is None else np.nan_to_num(np.ascontiguousarray(exo_z, dtype=np.float64)).reshape(self.n_envs, 3)
        check(self._lib.chub_reset(self._h, _ptr(d), _ptr(z), _ptr(self._obs)))
        return self._obs.copy() if self._copy_outputs else self._obs

    def step(self, actions, exo_z=None):
        a = np.ascontiguousarray(actions, dtype=np.float32)
        if a.shape != (self.n_envs, self.act_dim):  # MGR:148
            raise AssertionError("actions must have shape (%d, %d)" % (self.n_envs, self.act_dim))
        z = None if exo_z is None else np.nan_to_num(np.ascontiguousarray(exo_z, dtype=np.float64)).reshape(self.n_envs, 3)
        check(self._lib.chub_step(self._h, _ptr(a), _ptr(z), _ptr(self._obs), _ptr(self._reward), _ptr(self._done)))
        return self._out()

    def pinned_actions(self):
        """the handle's pinned [N, A] f32 action buffer as a numpy array: fill it in place and pass it to step() to save the
        CPU copy into pinned memory (chub_host_actions)"""
        if getattr(self, "_pinned", None) is None:
            p = C.c_void_p()
            check(self._lib.chub_host_actions(self._h, C.byref(p)))
            buf = (C.c_float * (self.n_envs * self.act_dim)).from_address(p.value)
            self._pinned = np.frombuffer(buf, dtype=np.float32).reshape(self.n_envs, self.act_dim)
        return self._pinned

    # ---- packed actions (chub_step_bits): one bit per pile + the two tail floats, 16 bytes per env up to 64 piles
    @property
    def bit_words(self):
        return (self.n_slots + 63) // 64

    def pack_actions(self, actions, out=None):
        """[N, A] f32 action rows -> (pile_bits [N, ceil(S / 64)] u64, tail [N, 2] f32): exactly what action_to_real
        (evcssp_manager.py:384-393) keeps of them -- pile on iff f32((a + 1) / 2) >= 0.5, i.e. a >= -2^-25.  out: the arrays to
        fill (e.g. pinned_bits())"""
        a = np.asarray(actions, dtype=np.float32)
        if a.shape != (self.n_envs, self.act_dim):
            raise AssertionError("actions must have shape (%d, %d)" % (self.n_envs, self.act_dim))
        bits, tail = out if out is not None else (np.zeros((self.n_envs, self.bit_words), dtype=np.uint64),
                                                  np.zeros((self.n_envs, 2), dtype=np.float32))
        on = a[:, :self.n_slots] >= np.float32(-2.0 ** -25)
        packed = np.packbits(on, axis=1, bitorder="little")
        pad = self.bit_words * 8 - packed.shape[1]
        if pad:
            packed = np.concatenate([packed, np.zeros((self.n_envs, pad), dtype=np.uint8)], axis=1)
        bits[...] = np.ascontiguousarray(packed).view("<u8")
        tail[...] = a[:, self.n_slots:]
        return bits, tail

    def pinned_bits(self):
        """the handle's pinned (pile_bits, tail) staging arrays (chub_host_bits): fill them in place and pass them to step_bits()"""
        if getattr(self, "_pinned_bits", None) is None:
            pb, pt = C.c_void_p(), C.c_void_p()
            check(self._lib.chub_host_bits(self._h, C.byref(pb), C.byref(pt)))
            b = np.frombuffer((C.c_uint64 * (self.n_envs * self.bit_words)).from_address(pb.value), dtype=np.uint64)
            t = np.frombuffer((C.c_float * (self.n_envs * 2)).from_address(pt.value), dtype=np.float32)
            self._pinned_bits = (b.reshape(self.n_envs, self.bit_words), t.reshape(self.n_envs, 2))
        return self._pinned_bits

    def step_bits(self, pile_bits, tail, exo_z=None):
        """step() with the actions already reduced to what the env uses of them: 16 bytes per env over PCIe instead of 4 (S + 2)"""
        b = np.ascontiguousarray(pile_bits, dtype=np.uint64)
        t = np.ascontiguousarray(tail, dtype=np.float32)
        if b.shape != (self.n_envs, self.bit_words) or t.shape != (self.n_envs, 2):
            raise AssertionError("pile_bits must have shape (%d, %d) and tail (%d, 2)" % (self.n_envs, self.bit_words, self.n_envs))
        z = None if exo_z is None else np.nan_to_num(np.ascontiguousarray(exo_z, dtype=np.float64)).reshape(self.n_envs, 3)
        check(self._lib.chub_step_bits(self._h, _ptr(b), _ptr(t), _ptr(z), _ptr(self._obs), _ptr(self._reward), _ptr(self._done)))
        return self._out()

    def load_actions(self, loads, tail):
        """[N, A] action array of the scalar-load mode: loads [N, 2] in kW (one per station), tail [N, 2] as in step()."""
        a = np.zeros((self.n_envs, self.act_dim), dtype=np.float32)
        loads = np.asarray(loads, dtype=np.float32).reshape(self.n_envs, 2)
        if self.piles[0] > 0:
            a[:, 0] = loads[:, 0]
        if self.piles[1] > 0:
            a[:, self.piles[0]] = loads[:, 1]
        a[:, self.n_slots:] = np.asarray(tail, dtype=np.float32).reshape(self.n_envs, 2)
        return a

    def step_load(self, loads, tail, exo_z=None):
        """Scalar-load control (the reference's evs_step(float), CHS.hpp:1169-1186 / 1480-1497): one kW target per station."""
        a = self.load_actions(loads, tail)
        z = None if exo_z is None else np.nan_to_num(np.ascontiguousarray(exo_z, dtype=np.float64)).reshape(self.n_envs, 3)
        check(self._lib.chub_step_load(self._h, _ptr(a), _ptr(z), _ptr(self._obs), _ptr(self._reward), _ptr(self._done)))
        return self._out()

    # ---- tape mode (parity instrument, see include/chub.h): recorded decisions through the production kernels
    def tape_register_soc(self, soc):
        s = np.ascontiguousarray(soc, dtype=np.float32).ravel()
        ids = np.zeros(s.size, dtype=np.uint32)
        check(self._lib.chub_tape_register_soc(self._h, _ptr(s), int(s.size), _ptr(ids)))
        return ids

    def tape_clear_soc(self):
        check(self._lib.chub_tape_clear_soc(self._h))

    def set_slots(self, rows):
        r = np.ascontiguousarray(rows, dtype=np.int32).reshape(self.n_envs, self.n_slots, 6)
        check(self._lib.chub_set_slots(self._h, _ptr(r)))

    def set_station_queue(self, line):
        q = np.ascontiguousarray(line, dtype=np.int32).reshape(self.n_envs, 2)
        check(self._lib.chub_set_station_queue(self._h, _ptr(q)))

    def reset_tape(self, occ_tape, car_tape, exo_days=None, exo_z=None):
        """evs_reset fed the reference's draws (chub_reset_tape): occ_tape [2, N] u32, car_tape [N, S, 2] u32; with exo_days [N, 2] and
        exo_z [N, 3] the tail takes renew_reset's days and make_state's normals from the caller too (chub_reset_tape_env)"""
        oc = np.ascontiguousarray(occ_tape, dtype=np.uint32).reshape(2, self.n_envs)
        ct = np.ascontiguousarray(car_tape, dtype=np.uint32).reshape(self.n_envs, self.n_slots, 2)
        if exo_days is None and exo_z is None:
            check(self._lib.chub_reset_tape(self._h, _ptr(oc), _ptr(ct), _ptr(self._obs)))
        else:
            if exo_days is None or exo_z is None:  # (the C API's own refusal, before numpy sees a None)
                raise ChubError("chub_reset_tape_env needs exo_days AND exo_z (the tail's side of the tape), or neither")
            d = np.ascontiguousarray(exo_days, dtype=np.int32).reshape(self.n_envs, 2)
            z = self._tape_normals(exo_z)
            check(self._lib.chub_reset_tape_env(self._h, _ptr(oc), _ptr(ct), _ptr(d), _ptr(z), _ptr(self._obs)))
        return self._obs.copy() if self._copy_outputs else self._obs

    def _tape_normals(self, exo_z):
        """[N, 3] f64 normals of a tape.  The wind process samples on every call (REN:66-69): its column must be finite.  The PV process samples only
        while the panel's table value is non-zero (REN:56-63: nothing is drawn at night) and the price noise on every fourth step (MGR:354):
        where the reference drew nothing its fixtures hold NaN, which becomes 0 here -- the tail does not look at a normal its process does not
        draw"""
        z = np.ascontiguousarray(exo_z, dtype=np.float64).reshape(self.n_envs, 3)
        if not np.isfinite(z[:, 1]).all():
            raise ChubError("tape normals: the wind column is drawn on every call and must be finite")
        return np.nan_to_num(z)

    def step_tape(self, actions, pk_tape, car_tape, exo_z=None, hv_tape=None):
        """one step from the tape (chub_step_tape); with exo_z [N, 3] f64 and hv_tape [N, W] u32 (word 0 = FCEV arrivals, word 1 + j =
        arrival j's SoC as f32 bits) the per-env tail replays the reference's draws as well (chub_step_tape_env)"""
        a = np.ascontiguousarray(actions, dtype=np.float32).reshape(self.n_envs, self.act_dim)
        pk = np.ascontiguousarray(pk_tape, dtype=np.uint64).reshape(2, self.n_envs)
        ct = np.ascontiguousarray(car_tape, dtype=np.uint32).reshape(self.n_envs, self.n_slots, 2)
        if exo_z is None and hv_tape is None:
            check(self._lib.chub_step_tape(self._h, _ptr(a), _ptr(pk), _ptr(ct), _ptr(self._obs), _ptr(self._reward), _ptr(self._done)))
        else:
            if exo_z is None or hv_tape is None:
                raise ChubError("chub_step_tape_env needs exo_z AND hv_tape (the tail's side of the tape), or neither")
            z = self._tape_normals(exo_z)
            hv = np.ascontiguousarray(hv_tape, dtype=np.uint32)
            hv = hv.reshape(self.n_envs, hv.size // self.n_envs)
            check(self._lib.chub_step_tape_env(self._h, _ptr(a), _ptr(pk), _ptr(ct), _ptr(z), _ptr(hv), int(hv.shape[1]), _ptr(self._obs),
                                               _ptr(self._reward), _ptr(self._done)))
        return self._out()

    # ---- per-env clocks (every reference env owns its clock, MGR:137-140, 304-316): reset / step a subset of the envs
    def _mask(self, mask):
        m = np.ascontiguousarray(np.asarray(mask).astype(bool), dtype=np.uint8)
        if m.shape != (self.n_envs,):
            raise AssertionError("mask must have shape (%d,)" % self.n_envs)
        return m

    def reset_envs(self, mask, exo_days=None, exo_z=None):
        """reset the envs of `mask`; returns the current observation of every env ([N, D]: fresh rows for the envs of the
        mask, the others as their last call left them).  exo_days / exo_z: as for reset() (COMPAT handles)"""
        m = self._mask(mask)
        d = np.ascontiguousarray(exo_days, dtype=np.int32) if exo_days is not None else None
        z = np.nan_to_num(np.ascontiguousarray(exo_z, dtype=np.float64)) if exo_z is not None else None
        check(self._lib.chub_reset_envs(self._h, _ptr(m), _ptr(d), _ptr(z), _ptr(self._obs)))
        return self._obs.copy()

    def step_envs(self, mask, actions, exo_z=None):
        """step the envs of `mask` only ([N, A] actions, the other rows are ignored); returns full-size obs, reward, done with
        the rows of the other envs as their last call left them"""
        m = self._mask(mask)
        a = np.ascontiguousarray(actions, dtype=np.float32)
        if a.shape != (self.n_envs, self.act_dim):  # MGR:148
            raise AssertionError("actions must have shape (%d, %d)" % (self.n_envs, self.act_dim))
        z = np.nan_to_num(np.ascontiguousarray(exo_z, dtype=np.float64)) if exo_z is not None else None
        check(self._lib.chub_step_envs(self._h, _ptr(m), _ptr(a), _ptr(z), _ptr(self._obs), _ptr(self._reward), _ptr(self._done)))
        return self._out()

    def step_load_envs(self, mask, loads, tail, exo_z=None):
        """step_load() for the envs of `mask` only"""
        m = self._mask(mask)
        a = self.load_actions(loads, tail)
        z = np.nan_to_num(np.ascontiguousarray(exo_z, dtype=np.float64)) if exo_z is not None else None
        check(self._lib.chub_step_load_envs(self._h, _ptr(m), _ptr(a), _ptr(z), _ptr(self._obs), _ptr(self._reward), _ptr(self._done)))
        return self._out()

    def env_clocks(self, ticks=False):
        """slot of day of every env (and, with ticks=True, the Philox tick of every env's last launch)"""
        t = np.zeros(self.n_envs, dtype=np.int32)
        tk = np.zeros(self.n_envs, dtype=np.uint32)
        check(self._lib.chub_env_clocks(self._h, _ptr(t), _ptr(tk)))
        return (t, tk) if ticks else t

    @property
    def clock_groups(self):
        """number of distinct env clocks right now (1 = lock-step)"""
        return self._lib.chub_clock_groups(self._h)

    # ---- copying envs on the device (chub_copy_envs): env dst_idx[i] becomes a clone of env src_idx[i] of `source` (default: this handle)
    def copy_envs(self, src_idx, dst_idx, source=None):
        """Clone envs by index without leaving the device: population-based training (the worst k become copies of the best k), planners
        (fan real envs out into a scratch handle), restarts from archived states.  The whole simulation state of the env is copied; in
        the Philox modes the clone keeps drawing from its OWN counters (this handle's seed and tick, its own env id), so it parts from
        its source at the next step.  Destinations must be distinct and, within one handle, no env both source and destination.  This
        handle's cached observation rows follow (the clone's current observation is its source's)."""
        src = self if source is None else source
        s = np.ascontiguousarray(np.asarray(src_idx).ravel(), dtype=np.int64)
        d = np.ascontiguousarray(np.asarray(dst_idx).ravel(), dtype=np.int64)
        if s.shape != d.shape:
            raise AssertionError("src_idx and dst_idx must have the same length")
        check(self._lib.chub_copy_envs(self._h, src._h, _ptr(s), _ptr(d), int(s.size)))
        if s.size and src.obs_dim == self.obs_dim:
            self._obs[d] = src._obs[s]

    def copy_envs_device(self, d_src_idx, d_dst_idx, count, source=None, stream=0):
        """copy_envs with the index arrays (int64) in device memory, enqueued on `stream`: no host synchronisation and no validation of
        the indices (see chub_copy_envs_device for the caller's obligations); this handle runs on per-env clocks afterwards"""
        src = self if source is None else source
        check(self._lib.chub_copy_envs_device(self._h, src._h, d_src_idx, d_dst_idx, int(count), stream or None))

    # ---- device-pointer path (ints are raw device addresses, e.g. torch.Tensor.data_ptr())
    def reset_device(self, d_obs, d_exo_days=0, d_exo_z=0, stream=0):
        check(self._lib.chub_reset_device(self._h, d_exo_days or None, d_exo_z or None, d_obs, stream or None))

    def step_device(self, d_actions, d_obs, d_reward, d_done, d_exo_z=0, stream=0):
        check(self._lib.chub_step_device(self._h, d_actions, d_exo_z or None, d_obs, d_reward, d_done, stream or None))

    def step_device_packed(self, d_actions, d_packed, d_exo_z=0, stream=0):
        """One [N, D+2] f32 output buffer: obs, reward, done -- what a shard sends in the per-step RCCL gather."""
        check(self._lib.chub_step_device_packed(self._h, d_actions, d_exo_z or None, d_packed, stream or None))

    def step_bits_device(self, d_pile_bits, d_tail, d_obs, d_reward, d_done, d_exo_z=0, stream=0):
        """the device-pointer step fed one bit per pile ([N, bit_words] u64) + the two tail floats ([N, 2] f32) instead of action rows:
        on the packed slot kernel the step reads the bits themselves (chub_step_bits_device)"""
        check(self._lib.chub_step_bits_device(self._h, d_pile_bits, d_tail, d_exo_z or None, d_obs, d_reward, d_done, stream or None))

    def step_bits_device_packed(self, d_pile_bits, d_tail, d_packed, d_exo_z=0, stream=0):
        check(self._lib.chub_step_bits_device_packed(self._h, d_pile_bits, d_tail, d_exo_z or None, d_packed, stream or None))

    # ---- masks in device memory and the step that resets whoever finished: the host never looks at a mask (include/chub.h)
    def reset_envs_dmask_device(self, d_mask, d_obs, d_exo_days=0, d_exo_z=0, stream=0):
        """reset_envs with the mask ([N] uint8) in device memory, enqueued on `stream`: one launch, one tick, no host wait; the
        handle runs on per-env clocks afterwards and stays there whatever the mask holds"""
        check(self._lib.chub_dmask_reset_envs_device(self._h, d_mask, d_exo_days or None, d_exo_z or None, d_obs, stream or None))

    def step_envs_dmask_device(self, d_mask, d_actions, d_obs, d_reward, d_done, d_exo_z=0, stream=0):
        """step_envs with the mask ([N] uint8) in device memory (as reset_envs_dmask_device); only the named envs' rows are written"""
        check(self._lib.chub_dmask_step_envs_device(self._h, d_mask, d_actions, d_exo_z or None, d_obs, d_reward, d_done, stream or None))

    def step_autoreset_device(self, d_actions, d_packed, d_final_obs=0, d_exo_z=0, d_reset_exo_days=0, d_reset_exo_z=0, stream=0):
        """every env takes one step on its own clock and every env whose done fired is reset in the same call (always two ticks):
        d_packed [N, D + 2] carries, for a reset env, the step's reward, done = 1 and the first observation of the new episode;
        d_final_obs [N, D] (optional) receives the terminal observation rows of the reset envs"""
        check(self._lib.chub_autoreset_step_device(self._h, d_actions, d_exo_z or None, d_reset_exo_days or None, d_reset_exo_z or None,
                                                   d_packed, d_final_obs or None, stream or None))

    def random_actions_device(self, d_actions, key, batch, stream=0):
        check(self._lib.chub_random_actions_device(self._h, int(key), int(batch), d_actions, stream or None))

    def graph_begin(self, stream):
        """record the device-pointer calls issued on `stream` from here on instead of running them (chub_graph_begin)"""
        check(self._lib.chub_graph_begin(self._h, stream))

    def graph_end(self, stream):
        g = C.c_void_p()
        check(self._lib.chub_graph_end(self._h, stream, C.byref(g)))
        return g

    def graph_launch(self, graph, stream):
        check(self._lib.chub_graph_launch(graph, stream))

    def graph_destroy(self, graph):
        self._lib.chub_graph_destroy(graph)

    def profile_begin(self, max_steps, every=1):
        check(self._lib.chub_profile_begin(self._h, int(max_steps), int(every)))

    def profile_end(self):
        """-> (slot kernel ms summed, env kernel ms summed, steps covered)"""
        a, b, n = C.c_double(), C.c_double(), C.c_int()
        check(self._lib.chub_profile_end(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def sync(self):
        check(self._lib.chub_sync(self._h))

    @property
    def uses_packed_kernel(self):
        return bool(self._lib.chub_uses_packed_kernel(self._h))

    @property
    def uses_fused_step(self):
        return bool(self._lib.chub_uses_fused_step(self._h))

    @property
    def uses_pair_tails(self):
        """chub_run_steps sends pairs of lock-step steps out with one tail launch (chub_options.span_steps on the two-launch step)"""
        return bool(self._lib.chub_uses_pair_tails(self._h))

    @property
    def uses_xcd_order(self):
        return bool(self._lib.chub_uses_xcd_order(self._h))

    @property
    def clock(self):
        return self._lib.chub_clock(self._h)

    # ---- introspection
    def set_telemetry(self, on=True):
        check(self._lib.chub_set_telemetry(self._h, int(bool(on))))
        self._tel_views = None

    def telemetry_views(self):
        """the handle's telemetry block as live numpy views, no copy and no device read (chub_telemetry_host): telem [T_COUNT, N]
        (one row per _lib.TELEMETRY_NAMES entry), obs64 [N, D], reward64 [N].  Current once the call that produced them has
        completed: reset() / step() return completed; after a device-pointer call, sync() first.  Handles of a few envs only (action rows
        of at most 16 KB in all: the drop-in class's one env): a batch keeps its block in device memory -- libchub returns
        CHUB_ERR_UNSUPPORTED here (ChubError) and telemetry() / obs_f64() / reward_f64() copy."""
        if getattr(self, "_tel_views", None) is None:
            pt, po, pr = C.c_void_p(), C.c_void_p(), C.c_void_p()
            check(self._lib.chub_telemetry_host(self._h, C.byref(pt), C.byref(po), C.byref(pr)))
            N, D, T = self.n_envs, self.obs_dim, _lib.T_COUNT
            view = lambda p, n, shape: np.frombuffer((C.c_double * n).from_address(p.value), dtype=np.float64).reshape(shape)
            self._tel_views = (view(pt, T * N, (T, N)), view(po, N * D, (N, D)), view(pr, N, (N,)))
        return self._tel_views

    def slots(self):
        """list over stations of arrays [N, 9, piles_k]: car, charge, emergency, power, soc, init_soc, target_soc,
        stay_time, already_stay_time."""
        out = np.zeros((self.n_envs, 9 * self.n_slots), dtype=np.float32)
        check(self._lib.chub_get_slots(self._h, _ptr(out)))
        s0 = self.piles[0]
        a = out[:, :9 * s0].reshape(self.n_envs, 9, s0)
        b = out[:, 9 * s0:].reshape(self.n_envs, 9, self.piles[1])
        return [a, b]

    # ---- per-pile observations on the device (chub_pile_obs_device): Station::situation and the stay counters as columns
    def pile_obs_device(self, d_out, fields=None, d_mask=0, stream=0):
        """the per-pile columns into device memory, d_out [N, C, n_slots] f32: env, then the C fields asked for in the order of
        _lib.PILE_NAMES, then hub slot (station 0's piles first, as in an action row) -- every value the bits slots() reports, in another
        layout.  fields: names, a bit mask, or None for all nine; d_mask [N] u8 in device memory: only the rows of the envs it names are
        written.  One launch on `stream`: no synchronisation, nothing of the simulation changes, recordable into a graph."""
        check(self._lib.chub_pile_obs_device(self._h, _lib.pile_fields_mask(fields), d_mask or None, d_out, stream or None))

    def pile_obs(self, fields=None):
        """pile_obs_device into host memory: float32 [N, C, n_slots] (the convenience form: it allocates, synchronises and copies)"""
        mask = _lib.pile_fields_mask(fields)
        out = np.zeros((self.n_envs, len(_lib.pile_fields_names(mask)), self.n_slots), dtype=np.float32)
        if out.size == 0:
            return out
        d = C.c_void_p()
        check(self._lib.chub_malloc_device(self._device, out.nbytes, C.byref(d)))
        try:
            check(self._lib.chub_sync(self._h))  # (calls in flight on any stream write the state)
            check(self._lib.chub_pile_obs_device(self._h, mask, None, d, None))
            check(self._lib.chub_copy_to_host(self._device, _ptr(out), d, out.nbytes, None))
        finally:
            self._lib.chub_free_device(self._device, d)
        return out

    # ---- pile sets on the device (chub_pile_set_device): the piles whose action bit the next step can see
    def pile_set_device(self, d_bits, which="decidable", d_mask=0, stream=0):
        """a pile set of every env into device memory, d_bits [N, bit_words] u64 in step_bits' layout (bits from n_slots up zero): "all",
        "occupied" (the pile holds a car) or "decidable" (it holds a car whose emergency is below 1.01: the step reads the pile's action bit).
        d_mask [N] u8 in device memory: only the rows of the envs it names are written.  One launch on `stream`: no synchronisation, nothing
        of the simulation changes, recordable into a graph."""
        check(self._lib.chub_pile_set_device(self._h, _lib.pile_set(which), d_mask or None, d_bits, stream or None))

    def pile_set(self, which="decidable"):
        """pile_set_device into host memory, unpacked: bool [N, n_slots] (the convenience form: it allocates, synchronises and copies)"""
        words = np.zeros((self.n_envs, self.bit_words), dtype=np.uint64)
        d = C.c_void_p()
        check(self._lib.chub_malloc_device(self._device, words.nbytes, C.byref(d)))
        try:
            check(self._lib.chub_sync(self._h))  # (calls in flight on any stream write the state)
            check(self._lib.chub_pile_set_device(self._h, _lib.pile_set(which), None, d, None))
            check(self._lib.chub_copy_to_host(self._device, _ptr(words), d, words.nbytes, None))
        finally:
            self._lib.chub_free_device(self._device, d)
        return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :self.n_slots].astype(bool)

    # ---- advantages on the device (chub_rollout_gae_device): GAE over a collected rollout's blocks
    def gae_device(self, n_steps, d_packed, d_values, d_adv, d_ret=0, d_final_values=0, gamma=0.99, lam=0.95, d_mask=0, d_stats=0, stream=0):
        """generalised advantage estimation over n_steps blocks: d_packed [T, N, D + 2] (a rollout's), d_values [T + 1, N] f32 (V of obs0,
        then V of every block's observation), d_final_values [N] (V of the terminal observations; 0: an episode's end is worth 0) ->
        d_adv, d_ret [T, N] f32 and d_stats [3] f64 (count, sum, sum of squares of the advantages).  Exact f32, every operation rounded
        once; the statistics have the same bits every call.  One launch on `stream` (two with d_stats): no synchronisation, no simulation
        state read, recordable into a graph."""
        g = _lib.ChubGae(int(n_steps), d_packed or None, d_values or None, d_final_values or None, d_mask or None, float(gamma), float(lam),
                         d_adv or None, d_ret or None, d_stats or None)
        check(self._lib.chub_rollout_gae_device(self._h, C.byref(g), stream or None))

    # ---- per-station deadline profiles on the device (chub_station_profile_device): who is due by when
    def station_profile_device(self, d_out, fields=None, buckets=8, d_mask=0, stream=0):
        """the stations' cars binned by the time they have left, into device memory: d_out [N, 2, C, B] f32 -- env, station, the C fields
        asked for in the order of _lib.SP_NAMES, then bucket min(left, B) - 1.  fields: names, a bit mask, or None for all seven; d_mask
        [N] u8 in device memory: only the blocks of the envs it names are written.  The shape does not depend on the hub.  One launch on
        `stream`: no synchronisation, nothing of the simulation changes, recordable into a graph."""
        check(self._lib.chub_station_profile_device(self._h, _lib.sp_fields_mask(fields), int(buckets), d_mask or None, d_out, stream or None))

    def station_profile(self, fields=None, buckets=8):
        """station_profile_device into host memory: float32 [N, 2, C, B] (the convenience form: it allocates, synchronises and copies)"""
        mask = _lib.sp_fields_mask(fields)
        check(min(self._lib.chub_station_profile_size(mask, int(buckets)), 0))
        out = np.zeros((self.n_envs, 2, len(_lib.sp_fields_names(mask)), int(buckets)), dtype=np.float32)
        d = C.c_void_p()
        check(self._lib.chub_malloc_device(self._device, out.nbytes, C.byref(d)))
        try:
            check(self._lib.chub_sync(self._h))  # (calls in flight on any stream write the state)
            check(self._lib.chub_station_profile_device(self._h, mask, int(buckets), None, d, None))
            check(self._lib.chub_copy_to_host(self._device, _ptr(out), d, out.nbytes, None))
        finally:
            self._lib.chub_free_device(self._device, d)
        return out

    # ---- exogenous look-ahead on the device (chub_forecast_device): slot of day, tariff, renewables, mean arrivals
    def forecast_device(self, d_out, fields=None, horizon=8, d_mask=0, stream=0):
        """what is deterministic about the next `horizon` slots of every env's day, into device memory: d_out [N, C, H] f32 -- env, the C
        fields asked for in the order of _lib.FC_NAMES, then look-ahead h (h = 0: the slot the env's next step simulates).  fields: names,
        a bit mask, or None for all ten; d_mask [N] u8 in device memory: only the blocks of the envs it names are written.  The noise on
        PV, wind and price is not forecast.  One launch on `stream`: no synchronisation, nothing of the simulation changes, recordable
        into a graph."""
        check(self._lib.chub_forecast_device(self._h, _lib.fc_fields_mask(fields), int(horizon), d_mask or None, d_out, stream or None))

    def forecast(self, fields=None, horizon=8):
        """forecast_device into host memory: float32 [N, C, H] (the convenience form: it allocates, synchronises and copies)"""
        mask = _lib.fc_fields_mask(fields)
        check(min(self._lib.chub_forecast_size(mask, int(horizon)), 0))
        out = np.zeros((self.n_envs, len(_lib.fc_fields_names(mask)), int(horizon)), dtype=np.float32)
        check(self._lib.chub_forecast(self._h, mask, int(horizon), _ptr(out)))
        return out

    # ---- step terms on the device (chub_get_step_terms_device): what the last step's reward is made of, the hydrogen side, constraint costs
    def step_terms_device(self, d_out, fields=None, d_mask=0, stream=0):
        """the terms of every env's last step into device memory, d_out [N, C] f32: env, then the C fields asked for in the order of
        _lib.ST_NAMES -- each the f64 expression of include/chub.h over the telemetry block, narrowed once.  Needs set_telemetry(True).
        fields: names, a bit mask, or None for all 27; d_mask [N] u8 in device memory: only the rows of the envs it names are written.
        It reports the block as it stands (an env reset since its last step shows that step's hydrogen and money columns beside the new
        episode's station columns).  One launch on `stream`: no synchronisation, nothing of the simulation changes, recordable into a
        graph."""
        check(self._lib.chub_get_step_terms_device(self._h, _lib.st_fields_mask(fields), d_mask or None, d_out, stream or None))

    def step_terms(self, fields=None):
        """the same for every env into host memory: float64 [N, C], the expressions before narrowing (the convenience form: it
        allocates, synchronises and copies)"""
        mask = _lib.st_fields_mask(fields)
        out = np.zeros((self.n_envs, len(_lib.st_fields_names(mask))), dtype=np.float64)
        check(self._lib.chub_get_step_terms(self._h, mask, _ptr(out)))
        return out

    def attach_step_terms(self, d_out, fields=None):
        """from now on every step call of every form fills d_out [N, C] f32 (device memory that outlives the attachment) right behind its
        kernels, on its own stream and with its own mask: only the rows of the envs a call served change, resets write nothing, and an
        auto-reset step writes a restarted env's TERMINAL terms (chub_set_step_terms).  Needs set_telemetry(True); not between
        graph_begin and graph_end."""
        check(self._lib.chub_set_step_terms(self._h, _lib.st_fields_mask(fields), d_out))

    def detach_step_terms(self):
        check(self._lib.chub_set_step_terms(self._h, 0, None))

    @property
    def step_terms_attached(self):
        """the attached field mask, or 0"""
        return self._lib.chub_get_step_terms_attached(self._h)

    # ---- station-level control on the device (chub_load_dispatch_device): one target per station -> action rows / one bit per pile
    def load_dispatch_device(self, d_loads, d_tail, d_actions=0, d_pile_bits=0, units="kw", d_mask=0, stream=0):
        """the reference's evs_step(float) dispatch as one read-only launch on `stream`: d_loads [N, 2] f32 (one target per station: kW, or
        with units="fraction" an action in [-1, 1] over the station's [min_power, max_power]) -> d_actions [N, A] f32 (pile entries +1 / -1,
        then d_tail's [N, 2] entries) and / or d_pile_bits [N, bit_words] u64 (step_bits' layout), for ANY step form to take.  d_mask [N] u8
        in device memory: only the rows of the envs it names are written.  No synchronisation, nothing of the simulation changes,
        recordable into a graph."""
        check(self._lib.chub_load_dispatch_device(self._h, _lib.load_units(units), d_loads, d_tail or None, d_mask or None, d_actions or None,
                                                  d_pile_bits or None, stream or None))

    def load_dispatch(self, loads, tail, units="kw"):
        """load_dispatch_device through host memory: loads [N, 2], tail [N, 2] -> (actions float32 [N, A], pile_bits uint64 [N, bit_words])
        (the convenience form: it allocates, synchronises and copies)"""
        u = _lib.load_units(units)
        ld = np.ascontiguousarray(loads, dtype=np.float32)
        t = np.ascontiguousarray(tail, dtype=np.float32)
        if ld.shape != (self.n_envs, 2) or t.shape != (self.n_envs, 2):
            raise AssertionError("loads and tail must have shape (%d, 2)" % self.n_envs)
        actions = np.zeros((self.n_envs, self.act_dim), dtype=np.float32)
        bits = np.zeros((self.n_envs, self.bit_words), dtype=np.uint64)
        check(self._lib.chub_sync(self._h))  # (calls in flight on any stream write the state)
        check(self._lib.chub_load_dispatch(self._h, u, _ptr(ld), _ptr(t), _ptr(actions), _ptr(bits)))
        return actions, bits

    # ---- an actor on the device (chub_policy_*): closed-loop rollouts with no host between the steps
    def make_policy(self, layers, inputs=("obs",), head="piles", hidden_act="tanh", squash="tanh", normalize=None):
        """an MLP actor bound to this handle -> DevicePolicy.  layers: [(W, b), ...] with W [out, in] (the nn.Linear layout), 1 .. 4 of them,
        hidden widths 1 .. 256, the last one the head's: "piles" act_dim outputs (an action row), "loads" 4 (load0, load1, tail0, tail1;
        the loads go through load_dispatch as fractions).  inputs: the blocks of the feature row in order -- "obs", or (kind, fields[,
        param]) with kind "pile_obs" / "station_profile" / "forecast" and fields / param as those calls take them.  normalize: None or
        (mean [F], inv_std [F], clip)."""
        return DevicePolicy(self, layers, inputs, head, hidden_act, squash, normalize)

    def make_moments(self, F):
        """running count / mean / M2 of F features on the device, bound to this handle -> DeviceMoments (chub_moments_create, 1 <= F <= 512):
        what DevicePolicy.normalizer_from_moments turns into the policy's normaliser"""
        return DeviceMoments(self, F)

    def make_population(self, policy, P, key):
        """P members around `policy` (a DevicePolicy of this handle, the centre) -> DevicePopulation (chub_population_create): P even, the
        handle's envs P blocks of a multiple of 32; key: the uint64 key of the perturbation noise.  Every member starts as the centre."""
        if policy._env is not self:
            raise ValueError("make_population: the policy was made for another handle")
        return DevicePopulation(self, policy, P, key)

    def make_policy_grad(self, policy, max_rows):
        """actor gradients for `policy` (a DevicePolicy of this handle with set_exploration) over calls of up to max_rows rows ->
        DevicePolicyGrad (chub_policy_grad_create); refused where the policy's images do not fit the gradient launch's LDS"""
        if policy._env is not self:
            raise ValueError("make_policy_grad: the policy was made for another handle")
        return DevicePolicyGrad(self, policy, max_rows)

    def make_critic(self, layers, hidden_act="tanh", normalize=None, max_rows=None):
        """a value network bound to this handle -> DeviceCritic (chub_critic_create).  layers: [(W [out, in], b [out]), ...] float32 in the
        nn.Linear layout, the last with one output; the rows it reads have layers[0][0].shape[1] floats.  normalize: None or (mean [F],
        inv_std [F], clip), the critic's own.  max_rows: the most rows one call works on (default n_envs; T * n_envs for a rollout)."""
        return DeviceCritic(self, layers, hidden_act, normalize, max_rows)

    def make_adam(self, target, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0):
        """Adam on the LIVE weights of `target`, a DevicePolicy or a DeviceCritic of this handle -> DeviceAdam (chub_adam_create_*).
        A policy that has set_exploration by now trains its log_std too.  weight_decay is decoupled (AdamW's) and touches W only;
        max_grad_norm > 0 clips the gradient's global norm (0: no clipping)."""
        if getattr(target, "_env", None) is not self:
            raise ValueError("make_adam: the target was made for another handle")
        return DeviceAdam(self, target, _lib.adam_hyper(lr, betas, eps, weight_decay, max_grad_norm))

    def make_train_log(self):
        """a training log with its gate word for this handle -> DeviceTrainLog (chub_train_log_create)"""
        return DeviceTrainLog(self)

    def make_lagrange(self, constraints):
        """K = 1 .. 4 constraints with their multipliers for this handle -> DeviceLagrange (chub_lagrange_create).  constraints: dicts
        with column (within the terms rows its gae will be given), kind "step" | "done", limit, lr, lambda0, lambda_max (0: no ceiling)"""
        return DeviceLagrange(self, constraints)

    def make_return_norm(self, gamma=0.99, eps=1e-8, clip=10.0):
        """running statistics of the discounted return and the reward scale they give, for this handle -> DeviceReturnNorm
        (chub_return_norm_create): VecNormalize's norm_reward with its defaults; clip 0 = none"""
        return DeviceReturnNorm(self, gamma=gamma, eps=eps, clip=clip)

    def ppo_update(self, grad, critic, actor_opt, critic_opt, n_rows, d_features, d_u, d_logp_old, d_adv, d_ret, d_rows, epochs, minibatch_rows, key,
                   d_pile_bits=0, d_set_bits=0, d_adv_stats=0, d_v_old=0, ld_features=None, loss="ppo_clip", value_loss="mse", clip_eps=0.2,
                   value_clip_eps=0.2, ent_coef=0.0, kl="k3", kl_limit=0.0, log=None, stream=0):
        """a whole PPO update enqueued on `stream` by one call (chub_ppo_update): per epoch a shuffle of the n_rows rows into d_rows
        [n_rows] int64 under the actor optimiser's step count, per minibatch the actor gradient, the critic gradient, log.record, the two
        steps, log.steps.  grad: a DevicePolicyGrad; critic: a DeviceCritic; the optimisers are theirs.  With log (a DeviceTrainLog)
        the update begins the log and both optimisers honour its gate: kl_limit > 0 stops stepping at the first minibatch whose KL
        estimate (kl: "k1" or "k3") is not <= kl_limit.  No synchronisation; recordable into a graph."""
        a = _lib.ChubPpoUpdateArgs()
        a.grad, a.critic, a.actor_opt, a.critic_opt, a.log = grad._g, critic._c, actor_opt._a, critic_opt._a, (log._t if log is not None else None)
        a.n_rows, a.d_features = int(n_rows), d_features or None
        a.ld_features = grad.policy.n_features if ld_features is None else int(ld_features)
        a.d_pile_bits, a.d_set_bits, a.d_u, a.d_logp_old, a.d_adv = d_pile_bits or None, d_set_bits or None, d_u or None, d_logp_old or None, d_adv or None
        a.d_adv_stats, a.d_ret, a.d_v_old = d_adv_stats or None, d_ret or None, d_v_old or None
        a.policy_loss, a.value_loss = _lib.policy_loss(loss), _lib.value_loss(value_loss)
        a.policy_clip_eps, a.value_clip_eps, a.ent_coef = float(clip_eps), float(value_clip_eps), float(ent_coef)
        a.epochs, a.minibatch_rows, a.key, a.d_rows = int(epochs), int(minibatch_rows), int(key) & (2 ** 64 - 1), d_rows or None
        a.kl_kind, a.kl_limit = _lib.kl_kind(kl), float(kl_limit)
        check(self._lib.chub_ppo_update(C.byref(a), stream or None))

    def shuffle_rows_device(self, d_rows, R, key, d_counter=0, offset=0, stream=0):
        """a permutation of 0 .. R - 1 into d_rows [R] int64 on `stream` (chub_shuffle_rows_device): a pure function of (key, counter, R)
        with counter = the int64 at d_counter (0: zero; a DeviceAdam's counter_address: its step count, so that every replay of a
        captured epoch shuffles anew) + offset.  Slices of d_rows are the d_rows of the gradient calls.  One launch; recordable."""
        check(self._lib.chub_shuffle_rows_device(self._h, int(key) & (2 ** 64 - 1), d_counter or None, int(offset), int(R), d_rows or None,
                                                 stream or None))

    def shuffle_rows(self, R, key, counter=0):
        """the same permutation computed on the host (chub_shuffle_rows) -> int64 [R]; no device"""
        rows = np.zeros(int(R), dtype=np.int64)
        check(self._lib.chub_shuffle_rows(int(key) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1), int(R), _ptr(rows)))
        return rows

    def next_tick(self):
        """the Philox tick of this handle's next reset or step (chub_next_tick): the tick a sampled policy call made now draws its noise
        under.  Host arithmetic only."""
        t = C.c_uint32()
        check(self._lib.chub_next_tick(self._h, C.byref(t)))
        return t.value

    def step_load_device(self, d_actions, d_obs, d_reward, d_done, d_exo_z=0, stream=0):
        """the device-pointer form of step_load (chub_step_load_device): d_actions [N, A] f32 in load_actions' layout"""
        check(self._lib.chub_step_load_device(self._h, d_actions, d_exo_z or None, d_obs, d_reward, d_done, stream or None))

    def station_scalars(self):
        out = np.zeros((self.n_envs, 2, 8), dtype=np.float64)
        check(self._lib.chub_get_station_scalars(self._h, _ptr(out)))
        return out

    def telemetry(self):
        out = np.zeros((self.n_envs, _lib.T_COUNT), dtype=np.float64)
        check(self._lib.chub_get_telemetry(self._h, _ptr(out)))
        return out

    def obs_f64(self):
        out = np.zeros((self.n_envs, self.obs_dim), dtype=np.float64)
        check(self._lib.chub_get_obs_f64(self._h, _ptr(out)))
        return out

    def reward_f64(self):
        out = np.zeros(self.n_envs, dtype=np.float64)
        check(self._lib.chub_get_reward_f64(self._h, _ptr(out)))
        return out

    # ---- per-episode accounting on the device (chub_set_episode_stats): the reference's end-of-day ledger (MGR:259-297), one per env
    def set_episode_stats(self, on=True):
        """keep the per-episode ledger: return, income, electricity drawn, length, and the tank's deviation / test_penalty / SOC as of the
        env's last step (_lib.EPISODE_NAMES).  Off by default; switching on zeroes everything and counting starts with the next call."""
        check(self._lib.chub_set_episode_stats(self._h, int(bool(on))))

    @property
    def has_episode_stats(self):
        return self._lib.chub_has_episode_stats(self._h) == 1

    def episode_stats(self, finished=False):
        """{name: float64 [n_envs]} over _lib.EPISODE_NAMES: the running episode of every env ("as if it ended now"), or with finished=True
        the record of the env's last finished episode (zeros until it has finished one: see episode_counts()).  Synchronises."""
        out = np.zeros((self.n_envs, _lib.EP_COUNT), dtype=np.float64)
        check(self._lib.chub_get_episode_stats(self._h, int(bool(finished)), _ptr(out)))
        return {name: out[:, i].copy() for i, name in enumerate(_lib.EPISODE_NAMES)}

    def episode_counts(self):
        """uint32 [n_envs]: the episodes every env has finished since the ledger was switched on"""
        out = np.zeros(self.n_envs, dtype=np.uint32)
        check(self._lib.chub_get_episode_counts(self._h, _ptr(out)))
        return out

    def episode_stats_device(self, d_out, d_counts=0, finished=True, stream=0):
        """the live / finished block into device memory, d_out [EP_COUNT, N] f64 (column-major, as stored) and optionally d_counts [N] u32:
        device-to-device copies on `stream`, no synchronisation, recordable into a graph"""
        check(self._lib.chub_episode_stats_device(self._h, int(bool(finished)), d_out, d_counts or None, stream or None))

    def episode_summary_device(self, d_out, drain=True, stream=0):
        """the finished episodes nobody has looked at yet (the envs whose pending flag is set), reduced on the device into d_out
        [1 + 4 * EP_COUNT] f64: count, then per column sum, sum of squares, min, max; drain clears the flags.  No synchronisation."""
        check(self._lib.chub_episode_summary_device(self._h, d_out, int(bool(drain)), stream or None))

    def episode_summary_raw(self, drain=True):
        """episode_summary_device into host memory: float64 [1 + 4 * EP_COUNT].  Synchronises."""
        out = np.zeros(1 + 4 * _lib.EP_COUNT, dtype=np.float64)
        check(self._lib.chub_episode_summary(self._h, _ptr(out), int(bool(drain))))
        return out

    def episode_summary(self, drain=True):
        """{"count": n, name: {"mean", "std", "min", "max"}} over the episodes that ended since the last draining call (what a trainer logs):
        29 doubles cross the bus instead of a [N, EP_COUNT] block.  mean and std (population) are computed here from sum and sum of squares;
        with count 0 they are NaN, min +inf and max -inf."""
        return summary_dict(self.episode_summary_raw(drain))

    def fcev_stuck_count(self):
        """envs whose FCEV forecourt is stuck: no prefix of its waiting list fits into 15 minutes any more, so -- as in the
        reference (HYD:270-276) -- nobody is served again until reset and the list only grows"""
        n = C.c_int64()
        check(self._lib.chub_fcev_stuck_count(self._h, C.byref(n)))
        return n.value

    def set_compat_seeds(self, seeds):
        s = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(self.n_envs, 2)
        check(self._lib.chub_set_rng_compat_seeds(self._h, _ptr(s)))

    def set_compat_state(self, state):
        s = np.ascontiguousarray(state, dtype=np.uint32).reshape(self.n_envs, 33)
        check(self._lib.chub_set_rng_compat_state(self._h, _ptr(s)))

    def compat_state(self):
        out = np.zeros((self.n_envs, 33), dtype=np.uint32)
        check(self._lib.chub_get_rng_compat_state(self._h, _ptr(out)))
        return out

    def compat_replay_constructor(self):
        check(self._lib.chub_compat_replay_constructor(self._h))

    def set_ou_state(self, ou):
        o = np.ascontiguousarray(ou, dtype=np.float64).reshape(self.n_envs, 3)
        check(self._lib.chub_set_ou_state(self._h, _ptr(o)))

    def get_state(self):
        """Snapshot of the whole simulation state as bytes (see chub_get_state)."""
        n = self._lib.chub_state_size(self._h)
        if n < 0:
            check(int(n))
        buf = np.empty(n, dtype=np.uint8)
        check(self._lib.chub_get_state(self._h, _ptr(buf), n))
        return buf

    def set_state(self, blob):
        b = np.ascontiguousarray(blob, dtype=np.uint8)
        check(self._lib.chub_set_state(self._h, _ptr(b), b.size))

    # ---- per-env hub parameters (chub_create_params)
    @property
    def has_env_params(self):
        return self._lib.chub_has_env_params(self._h) == 1

    def env_params(self):
        """the eight per-env kwargs as {name: float64 [n_envs]} (a homogeneous handle: its config, broadcast)"""
        if not self.has_env_params:
            return {f: np.full(self.n_envs, getattr(self.cfg, f), dtype=np.float64) for f in _lib.ENV_PARAM_FIELDS}
        rows = np.zeros(self.n_envs, dtype=ENV_PARAMS_DTYPE)
        check(self._lib.chub_get_env_params(self._h, _ptr(rows)))
        return {f: rows[f].copy() for f in _lib.ENV_PARAM_FIELDS}

    def set_env_params(self, mask=None, **fields):
        """overwrite the given fields (scalar or one value per env) of the envs `mask` names (None = all); the others keep theirs.  They
        apply from the next call on; follow with reset_envs(mask) to start those envs afresh (domain randomisation)."""
        unknown = set(fields) - set(_lib.ENV_PARAM_FIELDS)
        if unknown:
            raise TypeError("unknown per-env parameters: %s" % ", ".join(sorted(unknown)))
        cur = self.env_params()
        rows = np.zeros(self.n_envs, dtype=ENV_PARAMS_DTYPE)
        for f in _lib.ENV_PARAM_FIELDS:
            rows[f] = _field_values(f, fields[f], self.n_envs) if f in fields else cur[f]
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask, dtype=bool).reshape(self.n_envs), dtype=np.uint8)
        check(self._lib.chub_set_env_params(self._h, _ptr(m), _ptr(rows)))

    def hy_table(self, env=None):
        """hy_power_speed_list (HYD:154-157): the handle's table, or env i's own (COMPAT after compat_replay_constructor)"""
        out = np.zeros(102, dtype=np.float64)
        if env is None:
            check(self._lib.chub_get_hy_table(self._h, _ptr(out)))
        else:
            check(self._lib.chub_get_hy_table_env(self._h, int(env), _ptr(out)))
        return out

    def set_hy_table(self, table):
        t = np.ascontiguousarray(table, dtype=np.float64)
        if t.shape != (102,):
            raise ValueError("table must have 102 entries")
        check(self._lib.chub_set_hy_table(self._h, _ptr(t)))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.chub_destroy(self._h)
            self._h = None
            self._obs = self._reward = self._done = self._pinned = self._pinned_bits = self._tel_views = None
            for p in self._host_allocs:
                self._lib.chub_free_host(self._device, p)
            self._host_allocs = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


__all__ = ["VecChargingHub", "DevicePolicy", "DeviceMoments", "make_config", "ChubError", "split_env_params", "slice_env_kwargs"]
