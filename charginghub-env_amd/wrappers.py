"""What RL trainers put around the hub: registration, time limit, vector-env adapters, telemetry in ``info``.

The reference registers one id with gym (``evcssp_env_cpp/__init__.py:3-8``: ``charging-hub-v6``,
``max_episode_steps=999``) and returns an empty ``info`` (``MGR:302``) while keeping the step's accounting on
attributes (``re_used_renew``, ``re_ev_power_list``, ``income`` ... ``MGR:183-297``).  Neither gym nor Gymnasium is a
dependency here: the adapters are duck-typed to the three calling conventions in use --

* ``make()``            -- ``gym.make('evcssp_env_cpp:charging-hub-v6', **kwargs)`` of the reference: the single drop-in
                           env inside a ``TimeLimit(999)``;
* ``HubVecEnv``         -- the stable-baselines ``VecEnv`` convention (``reset() -> obs``, ``step_async / step_wait``,
                           ``dones`` with automatic reset and ``terminal_observation`` in the per-env ``infos``);
* ``HubVectorEnv``      -- the Gymnasium ``VectorEnv`` convention (``reset(seed=, options=) -> (obs, info)``,
                           ``step -> (obs, reward, terminated, truncated, info)`` with dict-of-arrays ``info``).

All N envs of a ``VecChargingHub`` run in lock-step (one clock), so an episode end is an all-env event and automatic
reset is one ``chub_reset``.
"""
import numpy as np

from . import _lib
from .env import Box, EvcsspManagerEnv_v6, _space
from .vec_env import VecChargingHub

ENV_ID = "charging-hub-v6"
MAX_EPISODE_STEPS = 999   # evcssp_env_cpp/__init__.py:6
REWARD_THRESHOLD = 99     # evcssp_env_cpp/__init__.py:7

# reference attribute name (MGR:175-297) -> telemetry column of chub_get_telemetry
_T = {n: i for i, n in enumerate(_lib.TELEMETRY_NAMES)}
INFO_COLUMNS = {
    "hy_act": _T["hy_act"], "re_hydrogen_power_init": _T["all_power_second"], "Store_SOC": _T["Store_SOC"],
    "fc_power": _T["fc_power"], "re_hy_for_fc": _T["hy_to_use"], "re_used_renew": _T["re_used_renew"],
    "re_hydrogen_power": _T["re_hydrogen_power"], "income": _T["income"], "re_pv_power": _T["re_pv_power"],
    "re_wd_power": _T["re_wd_power"], "hy_use": _T["hy_use"], "not_meet": _T["not_meet"],
    "price_next": _T["price_next"], "fcev_arrive_number": _T["fcev_arrive_number"],
}


def telemetry_info(tel):
    """[N, T_COUNT] telemetry block -> dict of [N] arrays under the reference's attribute names"""
    info = {name: tel[:, col].copy() for name, col in INFO_COLUMNS.items()}
    info["re_hy_gen"] = 900.0 * tel[:, _T["hy_flow_speed"]]                                    # MGR:183
    info["re_ev_power_list"] = tel[:, [_T["re_ev_power_0"], _T["re_ev_power_1"]]].copy()       # MGR:212
    return info


class TimeLimit(object):
    """``gym.wrappers.TimeLimit`` as the reference's registration applies it (old 4-tuple step API): after
    ``max_episode_steps`` steps without a reset, ``done`` is forced and ``info['TimeLimit.truncated']`` says whether the
    env itself had not ended.  The hub's own ``done`` fires every 96 steps (MGR:271-273); it may be stepped on without a
    reset (infinite horizon), which is when this limit matters."""

    def __init__(self, env, max_episode_steps=MAX_EPISODE_STEPS):
        self.env = env
        self._max_episode_steps = int(max_episode_steps)
        self._elapsed_steps = None

    def __getattr__(self, name):
        return getattr(self.env, name)

    @property
    def unwrapped(self):
        return self.env

    def reset(self, **kwargs):
        self._elapsed_steps = 0
        return self.env.reset(**kwargs)

    def step(self, action=None):
        assert self._elapsed_steps is not None, "Cannot call env.step() before calling reset()"
        obs, reward, done, info = self.env.step(action)
        self._elapsed_steps += 1
        if self._elapsed_steps >= self._max_episode_steps:
            info = dict(info)
            info["TimeLimit.truncated"] = not done
            done = True
        return obs, reward, done, info


def make(id=ENV_ID, **kwargs):
    """The reference's ``gym.make('evcssp_env_cpp:charging-hub-v6', **env_kwargs)`` (test/env_test.py:36)."""
    if id.split(":")[-1] != ENV_ID:
        raise ValueError("unknown environment id %r (have %r)" % (id, ENV_ID))
    return TimeLimit(EvcsspManagerEnv_v6(**kwargs), MAX_EPISODE_STEPS)


def register():
    """Register ``charging-hub-v6`` with whichever of gym / gymnasium is importable; returns the module names done."""
    done = []
    for modname in ("gym", "gymnasium"):
        try:
            mod = __import__(modname + ".envs.registration", fromlist=["register"])
        except Exception:
            continue
        mod.register(id=ENV_ID, entry_point="charginghub_env_amd:EvcsspManagerEnv_v6",
                     max_episode_steps=MAX_EPISODE_STEPS, reward_threshold=REWARD_THRESHOLD)
        done.append(modname)
    return done


def _spaces(vec, data_dir=None):
    price = np.fromfile((data_dir or _lib.DATA_DIR) + "/price_96.f64", dtype="<f8")
    obs_price = (price - np.mean(price)) / np.std(price)
    lo, hi = [-1.0, min(obs_price)], [1.0, max(obs_price)]           # MGR:51-104
    for k in range(2):
        if vec.piles[k] > 0:
            lo += [-1.0, -1.0, -1.0, 0]
            hi += [1.0, 1.0, 1.0, 2]
    lo += [0, 0, 0]
    hi += [1, 1, 1]
    return (_space(np.array(lo, dtype=np.float32), np.array(hi, dtype=np.float32)),
            _space(-1.0, 1.0, (vec.act_dim,)))


class _HubBatch(object):
    """shared by the two vector conventions: owns (or borrows) a VecChargingHub, counts steps, applies the limit"""

    def __init__(self, vec=None, n_envs=None, max_episode_steps=None, telemetry=False, data_dir=None, episode_stats=False, **hub_kwargs):
        if vec is None:
            if n_envs is None:
                raise ValueError("give either vec= or n_envs= and the hub kwargs")
            vec = VecChargingHub(n_envs, data_dir=data_dir, **hub_kwargs)
        self.vec = vec
        self.num_envs = vec.n_envs
        self.single_observation_space, self.single_action_space = _spaces(vec, data_dir)
        self.observation_space, self.action_space = self.single_observation_space, self.single_action_space
        self.max_episode_steps = None if max_episode_steps is None else int(max_episode_steps)
        self.telemetry = bool(telemetry)
        if self.telemetry:
            vec.set_telemetry(True)
        self.episode_stats = bool(episode_stats)
        if self.episode_stats:  # the per-episode ledger on the device (chub_set_episode_stats)
            vec.set_episode_stats(True)
        self._elapsed = 0
        self.metadata = EvcsspManagerEnv_v6.metadata
        self.reward_range = (-float("inf"), float("inf"))
        self.spec = None

    def _step(self, actions):
        obs, reward, done, _ = self.vec.step(actions)
        self._elapsed += 1
        truncated = np.zeros(self.num_envs, dtype=bool)
        if self.max_episode_steps is not None and self._elapsed >= self.max_episode_steps:
            truncated = ~done
        tel = telemetry_info(self.vec.telemetry()) if self.telemetry else {}
        return obs, reward, done, truncated, tel

    def _reset(self):
        self._elapsed = 0
        return self.vec.reset()

    def close(self):
        self.vec.close()

    def render(self, mode="human"):
        return None


class HubVecEnv(_HubBatch):
    """stable-baselines ``VecEnv`` convention over one VecChargingHub.

    ``step_wait`` returns ``(obs, rewards, dones, infos)``; when the episode ends (all envs at once) the envs are reset,
    the returned ``obs`` is the first observation of the next episode and ``infos[i]['terminal_observation']`` holds the
    last one of the finished episode; ``infos[i]['TimeLimit.truncated']`` marks an end forced by ``max_episode_steps``.
    ``episode_stats=True`` (off by default: the infos are then exactly the above) switches the hub's per-episode ledger on, and the
    ``infos[i]`` of an env whose episode ended carries ``episode = {"r": return, "l": length, "income", "draw_ele", "test_penalty",
    "end_soc"}`` (``r`` and ``l`` as stable-baselines' ``Monitor`` writes them; the others the reference's end-of-day ledger,
    MGR:275-297) -- read from the hub's live block before the reset, so an episode the time limit cut short reports what it had.
    """

    def __init__(self, vec=None, n_envs=None, max_episode_steps=None, telemetry=False, episode_stats=False, **hub_kwargs):
        _HubBatch.__init__(self, vec, n_envs, max_episode_steps, telemetry, episode_stats=episode_stats, **hub_kwargs)
        self._pending = None

    def reset(self):
        return self._reset()

    def step_async(self, actions):
        self._pending = np.asarray(actions, dtype=np.float32)

    def step_wait(self):
        obs, reward, done, truncated, tel = self._step(self._pending)
        self._pending = None
        dones = done | truncated
        infos = [dict() for _ in range(self.num_envs)]
        if tel:
            for name, col in tel.items():
                for i in range(self.num_envs):
                    infos[i][name] = col[i]
        if dones.any():
            # lock-step clock: the episode ends for every env in the same step
            ep = self.vec.episode_stats(finished=False) if self.episode_stats else None
            for i in range(self.num_envs):
                infos[i]["terminal_observation"] = obs[i]
                infos[i]["TimeLimit.truncated"] = bool(truncated[i])
                if ep is not None:
                    infos[i]["episode"] = {"r": float(ep["return"][i]), "l": int(ep["length"][i]), "income": float(ep["income"][i]),
                                           "draw_ele": float(ep["draw_ele"][i]), "test_penalty": float(ep["test_penalty"][i]),
                                           "end_soc": float(ep["end_soc"][i])}
            obs = self._reset()
            dones = np.ones(self.num_envs, dtype=bool)
        return obs, reward, dones, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def seed(self, seed=None):
        return [None] * self.num_envs  # streams are fixed by the hub's constructor seed (Philox key)

    def get_attr(self, attr_name, indices=None):
        n = self.num_envs if indices is None else len(np.atleast_1d(indices))
        return [getattr(self, attr_name)] * n

    def env_is_wrapped(self, wrapper_class, indices=None):
        n = self.num_envs if indices is None else len(np.atleast_1d(indices))
        return [False] * n


class HubVectorEnv(_HubBatch):
    """Gymnasium ``VectorEnv`` convention over one VecChargingHub (autoreset mode "next step": the step after an
    episode end ignores its actions, resets and returns the first observation with zero reward)."""

    def __init__(self, vec=None, n_envs=None, max_episode_steps=None, telemetry=False, autoreset=True, **hub_kwargs):
        _HubBatch.__init__(self, vec, n_envs, max_episode_steps, telemetry, **hub_kwargs)
        self.autoreset = bool(autoreset)
        self._needs_reset = True
        self.closed = False

    def reset(self, seed=None, options=None):
        self._needs_reset = False
        return self._reset(), {}

    def step(self, actions):
        if self._needs_reset:
            if not self.autoreset:
                raise RuntimeError("episode has ended: call reset()")
            obs, info = self.reset()
            z = np.zeros(self.num_envs, dtype=bool)
            return obs, np.zeros(self.num_envs, dtype=np.float32), z, z.copy(), info
        obs, reward, done, truncated, info = self._step(actions)
        if (done | truncated).any():
            self._needs_reset = True
        return obs, reward, done, truncated, info

    def close(self, **kwargs):
        if not self.closed:
            self.closed = True
            _HubBatch.close(self)


def _unpack_words(words, S):
    """recorded bit words int64 [..., W] -> bool [..., S] (a bool tensor passes through)"""
    import torch

    if words.dtype == torch.bool:
        return words
    sh = torch.arange(64, device=words.device, dtype=torch.int64)
    return (((words.unsqueeze(-1) >> sh) & 1) != 0).flatten(-2)[..., :S]


def sampled_logp(z, bits_or_on, u, log_std, piles=None):
    """The log-probability of recorded actions under a network's outputs, in torch and differentiable in `z` and `log_std`: what a trainer
    uses for the NEW policy's term of an importance ratio (include/chub.h, "sampling from the device actor"; the old policy's term is the
    recorded ``logp``).  z [..., S + G]: the last layer's PRE-squash outputs (S pile logits, then the G Gaussian means; G = log_std's
    length, S may be 0); bits_or_on: the pile decisions as a bool tensor [..., S] or as recorded bit words int64 [..., W]; u [..., G]: the
    recorded pre-squash samples.  eps = (u - z_gauss) / exp(log_std);
        logp = sum_b (on_b ? -softplus(-z_b) : -softplus(z_b)) + sum_i (-0.5 eps_i^2 - log_std_i - 0.5 ln 2 pi)
    The Gaussian part is the density of the pre-squash sample: no tanh Jacobian, which cancels in every ratio.
    piles: a bool tensor [..., S] or recorded set words int64 [..., W] (a rollout's ``set_bits``): only the piles of the set count, as in
    a ``logp`` recorded with ``logp_piles=``; None: every pile counts."""
    import math

    import torch

    G = log_std.shape[-1]
    S = z.shape[-1] - G
    on = _unpack_words(bits_or_on, S)
    zp, zg = z[..., :S], z[..., S:]
    terms = torch.nn.functional.softplus(torch.where(on, -zp, zp))
    if piles is not None:
        terms = torch.where(_unpack_words(piles, S), terms, torch.zeros_like(terms))
    eps = (u - zg) / torch.exp(log_std)
    return -terms.sum(dim=-1) + (-0.5 * eps * eps - log_std - 0.5 * math.log(2.0 * math.pi)).sum(dim=-1)


def sampled_entropy(z, log_std, piles=None):
    """The entropy of the actor's distribution at outputs z [..., S + G], in torch and differentiable in `z` and `log_std` (an entropy
    bonus): the Bernoulli entropy of the pile logits, H(p) = softplus(z) - z sigmoid(z), summed over the piles of `piles` (a bool tensor
    [..., S] or recorded set words int64 [..., W]; None: all of them), plus the Gaussian entropy sum_i (0.5 + log_std_i + 0.5 ln 2 pi) of
    the pre-squash samples."""
    import math

    import torch

    G = log_std.shape[-1]
    S = z.shape[-1] - G
    zp = z[..., :S]
    h = torch.nn.functional.softplus(zp) - zp * torch.sigmoid(zp)
    if piles is not None:
        h = torch.where(_unpack_words(piles, S), h, torch.zeros_like(h))
    return h.sum(dim=-1) + (0.5 + log_std + 0.5 * math.log(2.0 * math.pi)).sum(dim=-1)


def normalize_features(features, mean, inv_std, clip):
    """The device actor's input normalisation restated in torch (include/chub.h, "an actor on the device"): features [..., F] raw feature
    rows (a rollout's ``features``), mean / inv_std [F] (``TorchHubVecEnv.policy_normalizer``), clip the policy's.  The subtraction, the
    product and the clamp are three f32 operations, each rounded once, as in the kernel: for finite inputs the result is bit for bit what
    the actor's first layer saw, so the trainer's own network on it reproduces z.  (A NaN feature stays NaN here; the kernel clamps it.)"""
    import torch

    return torch.clamp((features - mean) * inv_std, min=-float(clip), max=float(clip))


def train_log_summary(words, kl="k3"):
    """The words of a training log (DeviceTrainLog.read) -> a dict under stable-baselines3's names; the sums are the log's f64 sums, every
    quotient is one f64 division.  A log that counted no minibatch gives NaN means."""
    w = np.asarray(words, dtype=np.float64)
    T = _lib.TLOG
    a, c = w[T["actor"]:T["actor"] + 6], w[T["critic"]:T["critic"] + 6]
    with np.errstate(all="ignore"):
        k1 = a[3] / a[0]
        out = {"n_minibatches": int(w[T["counted"]]), "stopped_at": None if w[T["stop_index"]] < 0 else int(w[T["stop_index"]]),
               "approx_kl": float(k1 if _lib.kl_kind(kl) == _lib.KL["k1"] else (a[5] / a[0] - 1.0) + k1), "approx_kl_max": float(w[T["kl_max"]]),
               "clip_fraction": float(a[4] / a[0]), "entropy": float(a[2] / a[0]), "policy_loss": float(a[1] / a[0]),
               "value_loss": float(c[1] / c[0]), "value_clip_fraction": float(c[2] / c[0]),
               "explained_variance": float(1.0 - (c[3] / c[0]) / max(c[5] / c[0] - (c[4] / c[0]) ** 2, 1e-12))}
        for name, base in (("policy_opt", T["actor_opt"]), ("critic_opt", T["critic_opt"])):
            o = w[base:base + 6]
            out[name] = {"steps": int(o[0]), "skipped": int(o[1]), "held_back": int(o[2]), "grad_norm_mean": float(o[3] / (o[0] + o[2])),  # (a skipped step's norm is not finite and not in the sum)
                         "grad_norm_max": float(o[4]), "clipped_steps": int(o[5])}
    return out


class TorchHubVecEnv(object):
    """The hub for an on-device learner: actions in and observations / rewards / dones out are torch CUDA tensors, the
    step runs through the device-pointer entry points on torch's current stream, and nothing is copied through the host
    (the host-pointer ``VecChargingHub.step`` moves 47 + 15 floats per env over PCIe, about 3x the device time at 65 536
    envs).  ``step`` returns views of ONE packed [N, D + 2] output buffer (what ``chub_step_device_packed`` writes);
    with ``autoreset`` the envs are reset in the step that ends the episode and the returned observation is the first
    of the next one (``last_obs`` keeps the terminal one).  torch is imported here, not by the package.

    ``autoreset=True`` counts ONE clock for the whole batch on the host (every env ends its day in the same step).
    ``autoreset="per_env"`` keeps no clock at all: every ``step`` is one ``chub_autoreset_step_device`` -- each env steps on its
    own clock and whoever finishes is reset on the device, in the same call -- so ``done`` is the per-env flag, ``last_obs`` is a
    fixed [N, D] buffer whose rows are valid where ``done`` (the terminal observations), and envs cloned in from an adapter at
    another time of day (``copy_envs``) simply keep their own days.  Nothing in that path reads the device or waits for it.
    ``step_bits`` is refused in this mode (the auto-reset call takes action rows).  ``device`` is a CUDA ordinal or a ``torch.device``.

    ``episode_stats=True`` switches the hub's per-episode ledger on (chub_set_episode_stats): ``episode_stats()`` and
    ``episode_summary()`` then give every env's finished-episode record, or its reduction over the episodes that ended since the last
    look, as CUDA tensors filled on torch's stream -- no device read, no wait, whatever the envs' clocks are.

    ``pile_obs=("car", "emergency", "soc")`` (any of _lib.PILE_NAMES; None: off) makes ``pile_obs()`` available: the per-pile columns
    the reference keeps in Station::situation, as one [N, C, S] CUDA tensor (chub_pile_obs_device); ``pile_names`` is the column order.

    ``station_profile=dict(fields=("cars", "must_charge", "power"), buckets=8)`` (fields: any of _lib.SP_NAMES, None for all; None: off)
    makes ``station_profile()`` available: each station's cars binned by the time they have left, as one [N, 2, C, B] CUDA tensor whose
    shape does not depend on the hub (chub_station_profile_device); ``profile_names`` is the column order.

    ``forecast=dict(fields=("valid", "cos", "price", "pv", "wind"), horizon=8)`` (fields: any of _lib.FC_NAMES, None for all; None: off)
    makes ``forecast()`` available: what is deterministic about the next H slots of every env's day -- slot of day, tariff, the env's PV
    and wind profiles, mean arrivals -- as one [N, C, H] CUDA tensor (chub_forecast_device); ``forecast_names`` is the column order.

    ``step_terms=("not_meet_loss", "grid_excess", "soc_penalty")`` (any of _lib.ST_NAMES; None: off) makes ``step_terms()`` available: what the
    last step's reward is made of, the hydrogen side and the constraint costs a Lagrangian method penalises, as one float32 [N, C] CUDA
    tensor; ``terms_names`` is the column order.  It switches the hub's telemetry on and attaches the buffer (chub_set_step_terms): every
    step fills it behind its own kernels, so ``step_terms()`` launches nothing, and an env the step has just re-started (either autoreset
    mode) shows the terms of its TERMINAL step -- the end-of-day ``soc_penalty`` included -- beside the new episode's first observation.

    ``control="station"`` makes the policy set one load per station instead of one action per pile (the reference's evs_step(float)):
    ``act_dim`` is 4 whatever the hub -- load of station 0, load of station 1, the two tail actions -- and every ``step`` first turns the
    loads into an action row the adapter owns (chub_load_dispatch_device, one read-only launch on torch's stream), then takes the step
    path of its ``autoreset`` mode, ``"per_env"`` included.  ``load_units="fraction"`` (the default) reads a load as an action in [-1, 1]
    over the station's [min_power, max_power]; ``"kw"`` as kW.  ``step_bits`` is refused in this mode.  The default ``control="pile"``
    is the adapter described above."""

    def __init__(self, n_envs, station_list, station_type_list, seed=0, device=0, autoreset=True, episode_stats=False, pile_obs=None,
                 station_profile=None, control="pile", load_units="fraction", forecast=None, step_terms=None, **hub_kwargs):
        import torch  # before libchub is loaded by VecChargingHub: both must share one HIP runtime

        if not (autoreset is True or autoreset is False or autoreset == "per_env"):
            raise ValueError("autoreset must be True, False or 'per_env', not %r" % (autoreset,))
        if control not in ("pile", "station"):  # (ValueError before anything is built)
            raise ValueError("control must be 'pile' or 'station', not %r" % (control,))
        self.control = control
        self._load_units = _lib.load_units(load_units)
        self._pile_mask = None if pile_obs is None else _lib.pile_fields_mask(pile_obs)  # (ValueError for an unknown name, before anything is built)
        self.pile_names = () if pile_obs is None else _lib.pile_fields_names(self._pile_mask)
        self._sp_mask = self._sp_buckets = None
        if station_profile is not None:  # (ValueError for an unknown name or key, before anything is built)
            unknown = set(station_profile) - {"fields", "buckets"}
            if unknown:
                raise ValueError("station_profile: a dict of fields and buckets, not %s" % sorted(unknown))
            self._sp_mask, self._sp_buckets = _lib.sp_fields_mask(station_profile.get("fields")), int(station_profile.get("buckets", 8))
            if not 1 <= self._sp_buckets <= 32:
                raise ValueError("station_profile: buckets 1 .. 32, not %d" % self._sp_buckets)
        self.profile_names = () if self._sp_mask is None else _lib.sp_fields_names(self._sp_mask)
        self._fc_mask = self._fc_horizon = None
        if forecast is not None:  # (ValueError for an unknown name or key, before anything is built)
            unknown = set(forecast) - {"fields", "horizon"}
            if unknown:
                raise ValueError("forecast: a dict of fields and horizon, not %s" % sorted(unknown))
            self._fc_mask, self._fc_horizon = _lib.fc_fields_mask(forecast.get("fields")), int(forecast.get("horizon", 8))
            if not 1 <= self._fc_horizon <= 96:
                raise ValueError("forecast: horizon 1 .. 96, not %d" % self._fc_horizon)
        self.forecast_names = () if self._fc_mask is None else _lib.fc_fields_names(self._fc_mask)
        self._st_mask = None if step_terms is None else _lib.st_fields_mask(step_terms)  # (ValueError for an unknown name, before anything is built)
        self.terms_names = () if step_terms is None else _lib.st_fields_names(self._st_mask)
        self.torch = torch
        self.device = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
        if self.device.type == "cuda":
            torch.cuda.set_device(self.device)
        rng = hub_kwargs.pop("rng", "philox")  # ("philox_curves": PHILOX's draws with the charge curves evaluated on the device)
        self.vec = VecChargingHub(n_envs, station_list, station_type_list, seed=seed, rng=rng, device=int(self.device.index or 0),
                                  **hub_kwargs)
        self.num_envs, self.obs_dim, self.act_dim = self.vec.n_envs, self.vec.obs_dim, self.vec.act_dim
        self._rows = None
        if control == "station":  # the policy's row is (load 0, load 1, tail 0, tail 1); the dispatch fills the hub's own [N, A] rows
            self._rows = torch.zeros((self.num_envs, self.vec.act_dim), dtype=torch.float32, device=self.device)
            self._loads = torch.zeros((self.num_envs, 2), dtype=torch.float32, device=self.device)
            self._tail = torch.zeros((self.num_envs, 2), dtype=torch.float32, device=self.device)
            self.act_dim = 4
        self.per_env = autoreset == "per_env"
        self.autoreset = bool(autoreset)
        self._packed = torch.empty((self.num_envs, self.obs_dim + 2), dtype=torch.float32, device=self.device)
        self._obs0 = torch.empty((self.num_envs, self.obs_dim), dtype=torch.float32, device=self.device)
        self.last_obs = None
        if self.per_env:  # the terminal rows land here on the device: rows valid where the step's done is set
            self.last_obs = torch.zeros((self.num_envs, self.obs_dim), dtype=torch.float32, device=self.device)
        self._cur_obs = None  # the observation rows the last reset / step returned
        self._t = 0
        self._ep_block = self._ep_counts = self._ep_summary = None
        if episode_stats:
            self.vec.set_episode_stats(True)
            self._ep_block = torch.zeros((_lib.EP_COUNT, self.num_envs), dtype=torch.float64, device=self.device)
            self._ep_counts = torch.zeros((self.num_envs,), dtype=torch.int32, device=self.device)  # (the handle's u32 words)
            self._ep_summary = torch.zeros((1 + 4 * _lib.EP_COUNT,), dtype=torch.float64, device=self.device)
        self._pile_buf = None
        if self._pile_mask is not None:
            self._pile_buf = torch.zeros((self.num_envs, len(self.pile_names), self.vec.n_slots), dtype=torch.float32, device=self.device)

        self._sp_buf = None
        if self._sp_mask is not None:
            self._sp_buf = torch.zeros((self.num_envs, 2, len(self.profile_names), self._sp_buckets), dtype=torch.float32, device=self.device)

        self._fc_buf = None
        if self._fc_mask is not None:
            self._fc_buf = torch.zeros((self.num_envs, len(self.forecast_names), self._fc_horizon), dtype=torch.float32, device=self.device)

        self._st_buf = None
        if self._st_mask is not None:  # every step fills the buffer behind its own kernels, from the telemetry block its tail writes
            self._st_buf = torch.zeros((self.num_envs, len(self.terms_names)), dtype=torch.float32, device=self.device)
            self.vec.set_telemetry(True)
            self.vec.attach_step_terms(self._st_buf.data_ptr(), self._st_mask)

    def step_terms(self):
        """float32 [N, C] CUDA tensor: for every env the columns of ``terms_names`` of its last step (zeros before the first).  Nothing is
        launched here: the step itself filled the buffer, on the stream it ran on.  An env the step re-started keeps its terminal step's
        terms; a reset writes nothing.  It is ONE buffer, overwritten by the next step."""
        if self._st_buf is None:
            raise RuntimeError("step terms are off: construct with step_terms=(names of _lib.ST_NAMES)")
        return self._st_buf

    def forecast(self):
        """float32 [N, C, H] CUDA tensor: for every env the columns of ``forecast_names`` over the next H slots of its day, h = 0 being the
        slot its next step simulates -- an env the step has just re-started shows slot 0 and its new days.  Filled by one launch on torch's
        current stream, without a wait; it is ONE buffer, overwritten by the next call."""
        if self._fc_buf is None:
            raise RuntimeError("the look-ahead is off: construct with forecast=dict(fields=(names of _lib.FC_NAMES), horizon=H)")
        self.vec.forecast_device(self._fc_buf.data_ptr(), self._fc_mask, self._fc_horizon, stream=self._stream())
        return self._fc_buf

    def station_profile(self):
        """float32 [N, 2, C, B] CUDA tensor: for every env and station the columns of ``profile_names`` over the B buckets of time left, as
        the piles stand after the last reset / step.  Filled by one launch on torch's current stream, without a wait; it is ONE buffer,
        overwritten by the next call."""
        if self._sp_buf is None:
            raise RuntimeError("station profiles are off: construct with station_profile=dict(fields=(names of _lib.SP_NAMES), buckets=B)")
        self.vec.station_profile_device(self._sp_buf.data_ptr(), self._sp_mask, self._sp_buckets, stream=self._stream())
        return self._sp_buf

    def pile_obs(self):
        """float32 [N, C, S] CUDA tensor: for every env the columns of ``pile_names`` over its S piles in hub-slot order (station 0's
        first, as in an action row), as the piles stand after the last reset / step -- an env the step has just re-started shows its new
        episode's piles.  Filled by one launch on torch's current stream, without a wait; it is ONE buffer, overwritten by the next call."""
        if self._pile_buf is None:
            raise RuntimeError("per-pile observations are off: construct with pile_obs=(names of _lib.PILE_NAMES)")
        self.vec.pile_obs_device(self._pile_buf.data_ptr(), self._pile_mask, stream=self._stream())
        return self._pile_buf

    def _need_episode_stats(self):
        if self._ep_block is None:
            raise RuntimeError("the episode ledger is off: construct with episode_stats=True")

    def episode_stats(self, finished=True):
        """{name: float64 [N] CUDA tensor} over _lib.EPISODE_NAMES plus "episodes" (int32 [N]: finished episodes per env): the record of
        every env's last finished episode (finished=False: its running one), copied on the device on torch's current stream.  The tensors
        are views of one buffer the next call overwrites."""
        self._need_episode_stats()
        self.vec.episode_stats_device(self._ep_block.data_ptr(), self._ep_counts.data_ptr(), finished=finished, stream=self._stream())
        out = {name: self._ep_block[i] for i, name in enumerate(_lib.EPISODE_NAMES)}
        out["episodes"] = self._ep_counts
        return out

    def episode_summary(self, drain=True):
        """float64 [1 + 4 * EP_COUNT] CUDA tensor over the episodes that ended since the last draining call: their count, then per column
        of _lib.EPISODE_NAMES sum, sum of squares, min, max -- reduced on the device on torch's current stream, without waiting
        (charginghub_env_amd.vec_env.summary_dict turns its host copy into means and deviations).  The next call overwrites it."""
        self._need_episode_stats()
        self.vec.episode_summary_device(self._ep_summary.data_ptr(), drain=drain, stream=self._stream())
        return self._ep_summary

    def _stream(self):
        if self.device.type != "cuda":
            return 0
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def _on_device(self, t):
        return t.device.type == self.device.type

    def reset(self):
        self.vec.reset_device(self._obs0.data_ptr(), stream=self._stream())
        self._t = 0
        self._cur_obs = self._obs0
        return self._obs0

    def step(self, actions):
        a = actions
        if not (self._on_device(a) and a.dtype == self.torch.float32 and a.is_contiguous()
                and tuple(a.shape) == (self.num_envs, self.act_dim)):
            raise AssertionError("actions must be a contiguous float32 tensor on %s of shape (%d, %d)"
                                 % (self.device, self.num_envs, self.act_dim))
        if self._rows is not None:  # station-level control: the loads become the hub's action rows, on the device
            self._loads.copy_(a[:, :2])
            self._tail.copy_(a[:, 2:])
            self.vec.load_dispatch_device(self._loads.data_ptr(), self._tail.data_ptr(), d_actions=self._rows.data_ptr(), units=self._load_units,
                                          stream=self._stream())
            a = self._rows
        if self.per_env:  # step + reset of whoever is done, on the device: no clock here, nothing read back
            self.vec.step_autoreset_device(a.data_ptr(), self._packed.data_ptr(), self.last_obs.data_ptr(), stream=self._stream())
            D = self.obs_dim
            self._cur_obs = self._packed[:, :D]
            return self._cur_obs, self._packed[:, D], self._packed[:, D + 1] > 0.5, {}
        self.vec.step_device_packed(a.data_ptr(), self._packed.data_ptr(), stream=self._stream())
        return self._after_step()

    def _after_step(self):
        D = self.obs_dim
        obs, reward, done = self._packed[:, :D], self._packed[:, D], self._packed[:, D + 1] > 0.5
        self._cur_obs = obs
        self._t += 1
        if self.autoreset and self._t % 96 == 0:  # lock-step clock: done fires for every env in this step (MGR:271-273)
            self.last_obs = obs.clone()
            reward, done = reward.clone(), done.clone()
            obs = self.reset()
        return obs, reward, done, {}

    def pack_bits(self, actions):
        """[N, A] float32 CUDA action rows -> (pile_bits [N, W] int64, tail [N, 2] float32), on the device: what action_to_real
        (evcssp_manager.py:384-393) keeps of them (pile on iff a >= -2^-25).  A policy that samples on / off decisions can build
        the bits itself and never materialise the rows."""
        torch = self.torch
        S, W = self.vec.n_slots, self.vec.bit_words
        on = (actions[:, :S] >= -2.0 ** -25).to(torch.int64)
        if S < 64 * W:
            on = torch.nn.functional.pad(on, (0, 64 * W - S))
        sh = torch.arange(64, device=actions.device, dtype=torch.int64)
        bits = (on.view(-1, W, 64) << sh).sum(dim=2)  # bit 63 lands in the sign bit: the same 64 bits as the unsigned word
        return bits.contiguous(), actions[:, S:].contiguous()

    def step_bits(self, pile_bits, tail):
        """step() fed one bit per pile + the two tail floats (pack_bits' layout) instead of action rows: 8 W + 8 bytes of action input
        per env instead of 4 (S + 2); on the packed slot kernel the step reads the bits themselves"""
        torch, N, W = self.torch, self.num_envs, self.vec.bit_words
        if self._rows is not None:
            raise RuntimeError("step_bits is not available with control='station' (the adapter dispatches the loads into action rows)")
        if self.per_env:
            raise RuntimeError("step_bits is not available with autoreset='per_env' (chub_autoreset_step_device takes action rows)")
        if not (self._on_device(pile_bits) and pile_bits.dtype == torch.int64 and pile_bits.is_contiguous() and tuple(pile_bits.shape) == (N, W)
                and self._on_device(tail) and tail.dtype == torch.float32 and tail.is_contiguous() and tuple(tail.shape) == (N, 2)):
            raise AssertionError("pile_bits must be a contiguous int64 tensor on %s of shape (%d, %d), tail float32 (%d, 2)" % (self.device, N, W, N))
        self.vec.step_bits_device_packed(pile_bits.data_ptr(), tail.data_ptr(), self._packed.data_ptr(), stream=self._stream())
        return self._after_step()

    # ---- an actor on the device (chub_policy_*): the trained network evaluated by the hub itself, closed-loop rollouts issued from C
    def load_policy(self, module_or_layers, inputs=("obs",), head=None, squash=None, normalize=None):
        """A feed-forward actor -> DevicePolicy (VecChargingHub.make_policy).  module_or_layers: an ``nn.Sequential`` of ``Linear`` /
        ``Tanh`` / ``ReLU`` (the activation between the Linears is the hidden one and must be the same throughout; a Tanh behind the last
        Linear is the squash), or a list of ``(W, b)`` tensors / arrays in the nn.Linear layout.  head: "piles" or "loads" (default: what
        ``control`` says); squash: "tanh" or "clip" (default: "tanh").  The weights are copied; after an optimiser step
        ``policy.set_weights_device(l, linear.weight.data_ptr(), linear.bias.data_ptr(), stream)`` brings layer l up to date on the
        device."""
        torch = self.torch
        hidden = None
        if isinstance(module_or_layers, torch.nn.Module):
            layers, acts = [], []
            for m in module_or_layers.children():
                if isinstance(m, torch.nn.Linear):
                    if m.bias is None:
                        raise ValueError("load_policy: every Linear needs a bias")
                    layers.append((m.weight.detach().to("cpu", torch.float32).numpy(), m.bias.detach().to("cpu", torch.float32).numpy()))
                    acts.append(None)
                elif isinstance(m, (torch.nn.Tanh, torch.nn.ReLU)) and layers and acts[-1] is None:
                    acts[-1] = "tanh" if isinstance(m, torch.nn.Tanh) else "relu"
                else:
                    raise ValueError("load_policy: an nn.Sequential of Linear / Tanh / ReLU, not %s here" % type(m).__name__)
            if not layers:
                raise ValueError("load_policy: no Linear layer")
            if len(set(acts[:-1])) > 1 or None in acts[:-1]:
                raise ValueError("load_policy: one activation, Tanh or ReLU, behind every hidden Linear")
            hidden = acts[0] if len(acts) > 1 else None
            if acts[-1] == "relu" or (acts[-1] == "tanh" and squash not in (None, "tanh")):
                raise ValueError("load_policy: behind the last Linear only a Tanh (the squash) may follow")
            squash = "tanh" if acts[-1] == "tanh" else squash
        else:
            layers = [(W.detach().to("cpu", torch.float32).numpy() if hasattr(W, "detach") else W,
                       b.detach().to("cpu", torch.float32).numpy() if hasattr(b, "detach") else b) for W, b in module_or_layers]
        if head is None:
            head = "loads" if self.control == "station" else "piles"
        return self.vec.make_policy(layers, inputs=inputs, head=head, hidden_act=hidden or "tanh", squash=squash or "tanh", normalize=normalize)

    def rollout(self, policy, n_steps):
        """n_steps closed-loop steps of `policy` from the current observation, issued from C on torch's current stream with nothing on the
        host between them (chub_policy_run_steps), in the adapter's auto-reset mode: ``autoreset="per_env"`` every step is the auto-reset
        step and ``last_obs`` keeps the terminal rows; ``autoreset=True`` the batch is reset where ``step`` would reset it, after the 96th
        step of its day (``last_obs`` is set only for a day that ends with the rollout).  Returns (obs, reward, done, {}) of the LAST step as
        views of its packed block, as ``step`` does."""
        if not self.autoreset:
            raise RuntimeError("rollout needs an auto-reset mode: construct with autoreset=True or 'per_env'")
        if self._cur_obs is None:
            raise RuntimeError("rollout() before reset()")
        n_steps = int(n_steps)
        if n_steps <= 0:
            raise ValueError("n_steps must be positive")
        if getattr(self, "_packed_alt", None) is None:
            self._packed_alt = self.torch.empty_like(self._packed)
        first = 0 if self.per_env else self._t
        blocks = [None, None]  # step i writes block i & 1 and reads block (i - 1) & 1: the block that holds the current observation
        blocks[(first - 1) & 1], blocks[first & 1] = self._packed, self._packed_alt
        fresh = self._cur_obs is self._obs0  # the current observation is a reset's dense [N, D] block, not a packed one
        if self.per_env:
            policy.run_steps([b.data_ptr() for b in blocks], n_steps, first_step=first, mode="autoreset", d_reset_obs=self._obs0.data_ptr() if fresh else 0,
                             d_final_obs=self.last_obs.data_ptr(), stream=self._stream())
        else:
            start, count = first, n_steps
            if first % 96 == 0:  # the adapter has just reset (the observation is in _obs0): the run must not begin with a reset of its own
                if getattr(self, "_pol_bits", None) is None:
                    self._pol_bits = self.torch.zeros((self.num_envs, self.vec.bit_words), dtype=self.torch.int64, device=self.device)
                    self._pol_tail = self.torch.zeros((self.num_envs, 2), dtype=self.torch.float32, device=self.device)
                policy.act_device(self._obs0.data_ptr(), self.obs_dim, d_pile_bits=self._pol_bits.data_ptr(), d_tail=self._pol_tail.data_ptr(),
                                  stream=self._stream())
                self.vec.step_bits_device_packed(self._pol_bits.data_ptr(), self._pol_tail.data_ptr(), blocks[first & 1].data_ptr(),
                                                 stream=self._stream())
                start, count = first + 1, n_steps - 1
            if count:
                policy.run_steps([b.data_ptr() for b in blocks], count, first_step=start, mode="lockstep", d_reset_obs=self._obs0.data_ptr(),
                                 stream=self._stream())
            self._t += n_steps - 1  # (_after_step counts the last one)
        last = blocks[(first + n_steps - 1) & 1]
        if last is not self._packed:
            self._packed, self._packed_alt = last, self._packed
        if self.per_env:
            D = self.obs_dim
            self._cur_obs = self._packed[:, :D]
            return self._cur_obs, self._packed[:, D], self._packed[:, D + 1] > 0.5, {}
        return self._after_step()

    # ---- a population of actors (chub_population_*): the gradient-free route -- perturb, one closed-loop day, fitness, ES gradient
    def load_population(self, policy, P, key):
        """P members around `policy` (a DevicePolicy from ``load_policy``, the centre) -> DevicePopulation (VecChargingHub.make_population):
        member m acts for envs [m E, (m + 1) E), E = num_envs / P a multiple of 32.  ``pop.perturb_device(sigma, generation, d_W, d_b,
        stream)`` with the data_ptr()s of the centre's Linear layers draws the members on the device."""
        return self.vec.make_population(policy, P, key)

    def population_rollout(self, pop, n_steps):
        """``rollout`` with the population's actor (chub_population_run_steps): n_steps closed-loop steps of all P members at once, member
        m's weights for its block of envs; the same auto-reset modes, the same return value"""
        return self.rollout(pop, n_steps)

    def es_gradient(self, pop, utilities, generation):
        """The ES gradient estimate of `pop`'s generation on torch's current stream (chub_population_es_gradient_device): utilities [P]
        float32 CUDA (e.g. centred ranks of the members' fitness) -> a list of (gW, gb) float32 CUDA tensors in the nn.Linear shapes,
        g = sum over pairs j of (u[2j] - u[2j + 1]) eps_j with the noise regenerated, not stored, accumulated in f64 in a fixed order.
        sigma and 1 / (P sigma) are the caller's to apply.  The next call with the same population overwrites the tensors."""
        torch = self.torch
        u = utilities
        if not (self._on_device(u) and u.dtype == torch.float32 and u.is_contiguous() and tuple(u.shape) == (pop.n_members,)):
            raise AssertionError("utilities must be a contiguous float32 tensor on %s of shape (%d,)" % (self.device, pop.n_members))
        cache = getattr(self, "_es_grads", None)
        if cache is None:
            cache = self._es_grads = {}
        grads = cache.get(id(pop))
        if grads is None:
            grads = cache[id(pop)] = [(torch.zeros((o, i), dtype=torch.float32, device=self.device),
                                       torch.zeros((o,), dtype=torch.float32, device=self.device)) for o, i in pop.layer_shapes]
        pop.es_gradient_device(u.data_ptr(), generation, [gW.data_ptr() for gW, _ in grads], [gb.data_ptr() for _, gb in grads],
                               stream=self._stream())
        return grads

    def collect(self, policy, n_steps, logp_piles=None, terms=None):
        """n_steps SAMPLED closed-loop steps of `policy` (after ``policy.set_exploration``) from the current observation, issued from C on
        torch's current stream (chub_policy_collect), keeping the trajectory: a dict of CUDA tensors the next call with the same policy and
        n_steps overwrites --
            obs0 [N, D]: the observation the first step acted on; packed [T, N, D + 2]: step t's output block, whose observation the actor
            of step t + 1 read; reward [T, N] and done [T, N] (1.0 / 0.0): views of packed; bits [T, N, W] int64 and tail [T, N, 2]: the
            actions taken; u [T, N, G]: the pre-squash Gaussian samples; logp [T, N]; features [T, N, F]: the raw feature rows the actor saw.
        ``sampled_logp`` of the trainer's own forward pass on ``features`` gives the new policy's term of the importance ratio.
        ``logp_piles="all" | "occupied" | "decidable"`` (chub_policy_collect_set): ``logp`` counts a pile's term only where the pile is in
        that set of the state the step acted on, and the dict also holds set_bits [T, N, W] int64, the sets -- what
        ``sampled_logp(..., piles=ro["set_bits"])`` and ``sampled_entropy`` take.  "decidable" are the piles whose bit the step reads.
        ``terms=(names of _lib.ST_NAMES)`` (chub_policy_collect_terms): the dict gains terms [T, N, C], step t's terms in block t in the
        order of ``rollout["terms_names"]`` (ascending field order) -- a finished env's row holds its terminal step's terms -- what
        ``cost_advantages`` reads.  Telemetry is switched on by the first such call; a ``step_terms=`` buffer stays attached and unwritten.
        ``autoreset="per_env"``: every step is the auto-reset step, ``last_obs`` keeps the terminal rows, n_steps <= 96.
        ``autoreset=True``: the rollout stays inside the batch's day (n_steps <= 96 - steps taken today); one that begins a day begins with
        the day's reset, made by the call itself (it replaces the one the adapter made), and one that ends a day is followed by the
        adapter's reset as in ``step``."""
        torch = self.torch
        if not self.autoreset:
            raise RuntimeError("collect needs an auto-reset mode: construct with autoreset=True or 'per_env'")
        if self._cur_obs is None:
            raise RuntimeError("collect() before reset()")
        T = int(n_steps)
        today = 0 if self.per_env else self._t % 96
        if not 0 < T <= 96 - today:
            raise ValueError("n_steps must be 1 .. %d here (a rollout stays inside one day)" % (96 - today))
        N, D, W = self.num_envs, self.obs_dim, self.vec.bit_words
        cache = getattr(self, "_rollouts", None)
        if cache is None:
            cache = self._rollouts = {}
        if logp_piles is not None:
            _lib.pile_set(logp_piles)  # (ValueError for an unknown name, before anything is allocated)
        st_mask = None if terms is None else _lib.st_fields_mask(terms)  # (ValueError for an unknown name, before anything is allocated)
        key = (id(policy), T, logp_piles is not None) + (() if st_mask is None else (st_mask,))
        ro = cache.get(key)
        if ro is None:
            f32 = dict(dtype=torch.float32, device=self.device)
            ro = cache[key] = {
                "obs0": torch.zeros((N, D), **f32), "packed": torch.zeros((T, N, D + 2), **f32),
                "bits": torch.zeros((T, N, W), dtype=torch.int64, device=self.device), "tail": torch.zeros((T, N, 2), **f32),
                "u": torch.zeros((T, N, policy.n_gaussians), **f32), "logp": torch.zeros((T, N), **f32),
                "features": torch.zeros((T, N, policy.n_features), **f32)}
            ro["reward"], ro["done"] = ro["packed"][:, :, D], ro["packed"][:, :, D + 1]
            if logp_piles is not None:
                ro["set_bits"] = torch.zeros((T, N, W), dtype=torch.int64, device=self.device)
            if st_mask is not None:
                ro["terms_names"] = _lib.st_fields_names(st_mask)
                ro["terms"] = torch.zeros((T, N, len(ro["terms_names"])), **f32)
                self.vec.set_telemetry(True)
        self._rollout_policy = getattr(self, "_rollout_policy", {})
        self._rollout_policy[id(ro)] = policy  # (policy_gradient / evaluate_actions find the rollout's actor here)
        ro["obs0"].copy_(self._cur_obs)
        extra = {} if logp_piles is None else dict(logp_piles=logp_piles, d_set_bits=ro["set_bits"].data_ptr())
        if st_mask is not None:
            extra.update(d_terms=ro["terms"].data_ptr(), term_fields=st_mask)
        policy.collect(T, ro["obs0"].data_ptr(), ro["packed"].data_ptr(), ro["bits"].data_ptr(), ro["tail"].data_ptr(), ro["u"].data_ptr(),
                       ro["logp"].data_ptr(), d_features=ro["features"].data_ptr(), d_final_obs=self.last_obs.data_ptr() if self.per_env else 0,
                       first_step=today, mode="autoreset" if self.per_env else "lockstep", stream=self._stream(), **extra)
        self._packed.copy_(ro["packed"][T - 1])  # (the block `step` and `rollout` continue from)
        self._cur_obs = self._packed[:, :D]
        if not self.per_env:
            self._t += T
            if self._t % 96 == 0:
                self.last_obs = self._cur_obs.clone()
                self.reset()
        return ro

    def advantages(self, rollout, values, final_values=None, gamma=0.99, lam=0.95, stats=False, reward_norm=None):
        """Generalised advantage estimation over a ``collect`` rollout, on torch's current stream in one launch (chub_rollout_gae_device):
        values [T + 1, N] float32 CUDA = the critic on ``rollout["obs0"]`` and then on every block's observation
        (``rollout["packed"][:, :, :D]``); final_values [N] = the critic on ``last_obs`` (the terminal rows of ``autoreset="per_env"``),
        read only where done fires; None: an episode's end is worth 0.  Returns (adv, ret), float32 [T, N] CUDA tensors the next call with
        the same T overwrites; with stats=True (adv, ret, stats), stats a float64 [3] CUDA tensor: count, sum and sum of squares of the
        advantages (mean and variance for normalisation with nothing read back).  Exact f32: delta = (r + gamma vn) - V,
        adv = delta + (gamma lam) adv', every operation rounded once.  reward_norm: a ``make_reward_normalizer`` object
        (chub_return_norm_gae_device) -- r is the rollout's reward times the object's scale word, clipped to its clip; the critic then
        learns returns in scaled units.  None: the raw reward."""
        torch = self.torch
        packed = rollout["packed"]
        T, N = int(packed.shape[0]), self.num_envs
        ok = lambda t, shape: self._on_device(t) and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
        if not ok(values, (T + 1, N)):
            raise AssertionError("values must be a contiguous float32 tensor on %s of shape (%d, %d)" % (self.device, T + 1, N))
        if final_values is not None and not ok(final_values, (N,)):
            raise AssertionError("final_values must be a contiguous float32 tensor on %s of shape (%d,)" % (self.device, N))
        cache = getattr(self, "_gae", None)
        if cache is None:
            cache = self._gae = {}
        out = cache.get(T)
        if out is None:
            out = cache[T] = (torch.zeros((T, N), dtype=torch.float32, device=self.device), torch.zeros((T, N), dtype=torch.float32, device=self.device),
                              torch.zeros((3,), dtype=torch.float64, device=self.device))
        adv, ret, st = out
        if reward_norm is not None:
            self._own_reward_norm(reward_norm, "advantages")
        gae = self.vec.gae_device if reward_norm is None else reward_norm.gae_device
        gae(T, packed.data_ptr(), values.data_ptr(), adv.data_ptr(), d_ret=ret.data_ptr(),
            d_final_values=0 if final_values is None else final_values.data_ptr(), gamma=gamma, lam=lam,
            d_stats=st.data_ptr() if stats else 0, stream=self._stream())
        return (adv, ret, st) if stats else (adv, ret)

    # ---- actor gradients on the device (chub_policy_grad_*): the policy-gradient step with no autograd for the actor
    def _policy_grad_entry(self, policy, R, n_rows):
        """the policy's gradient object for calls of R rows over arrays of n_rows, with the tensors its calls fill (made on first use)"""
        torch = self.torch
        cache = getattr(self, "_pgrad", None)
        if cache is None:
            cache = self._pgrad = {}
        ent = cache.get(id(policy))
        if ent is None or ent["grad"].max_rows < R:
            if ent is not None:
                ent["grad"].close()
            g = self.vec.make_policy_grad(policy, max(R, n_rows))
            f32 = dict(dtype=torch.float32, device=self.device)
            ent = cache[id(policy)] = {"grad": g, "grads": [(torch.zeros((o, i), **f32), torch.zeros((o,), **f32)) for o, i in g.layer_shapes],
                                       "g_log_std": torch.zeros((policy.n_gaussians,), **f32),
                                       "stats": torch.zeros((6,), dtype=torch.float64, device=self.device), "rows": {}}
        return ent

    def _policy_grad_call(self, rollout, adv, rows, loss, clip_eps, ent_coef, adv_stats, backward, into=None):
        torch = self.torch
        policy = getattr(self, "_rollout_policy", {}).get(id(rollout))
        if policy is None:
            raise ValueError("rollout: a dict returned by this adapter's collect()")
        feats = rollout["features"]
        n_rows = int(feats.shape[0]) * int(feats.shape[1])
        if rows is not None and not (self._on_device(rows) and rows.dtype == torch.int64 and rows.dim() == 1 and rows.is_contiguous()):
            raise AssertionError("rows must be a contiguous 1-d int64 tensor on %s" % (self.device,))
        R = n_rows if rows is None else int(rows.numel())
        if adv is not None and not (self._on_device(adv) and adv.dtype == torch.float32 and adv.is_contiguous() and adv.numel() == n_rows):
            raise AssertionError("adv must be a contiguous float32 tensor on %s with one entry per (step, env)" % (self.device,))
        if adv_stats is not None and not (self._on_device(adv_stats) and adv_stats.dtype == torch.float64 and adv_stats.is_contiguous()
                                          and adv_stats.numel() == 3):
            raise AssertionError("adv_stats must be a contiguous float64 tensor on %s of 3 entries (advantages(..., stats=True))" % (self.device,))
        ent = self._policy_grad_entry(policy, R, n_rows)
        out = ent["rows"].get(R)
        if out is None:
            out = ent["rows"][R] = (torch.zeros((R,), dtype=torch.float32, device=self.device), torch.zeros((R,), dtype=torch.float32, device=self.device))
        piles = policy.spec.head == _lib.PHEAD["piles"]
        sets = rollout.get("set_bits") if piles else None
        dst = ent if into is None else self._into(into, policy, "policy_gradient")
        ent["grad"].grad_device(R, n_rows, feats.data_ptr(), rollout["u"].data_ptr(), (adv if adv is not None else rollout["logp"]).data_ptr(),
                                d_pile_bits=rollout["bits"].data_ptr() if piles else 0, d_set_bits=0 if sets is None else sets.data_ptr(),
                                d_logp_old=rollout["logp"].data_ptr(), d_rows=0 if rows is None else rows.data_ptr(),
                                d_adv_stats=0 if adv_stats is None else adv_stats.data_ptr(), loss=loss, clip_eps=clip_eps, ent_coef=ent_coef,
                                d_gW=[gW.data_ptr() for gW, _ in dst["grads"]] if backward else None,
                                d_gb=[gb.data_ptr() for _, gb in dst["grads"]] if backward else None,
                                d_glog_std=dst["g_log_std"].data_ptr() if backward else 0, d_logp_new=out[0].data_ptr(), d_entropy=out[1].data_ptr(),
                                d_stats=ent["stats"].data_ptr() if backward else 0, stream=self._stream())
        return (ent if into is None else dict(ent, grads=dst["grads"], g_log_std=dst["g_log_std"])), out

    def policy_gradient(self, rollout, adv, rows=None, loss="ppo_clip", clip_eps=0.2, ent_coef=0.0, adv_stats=None, into=None):
        """The actor's gradient of a surrogate loss over a ``collect`` rollout, on torch's current stream with no autograd
        (chub_policy_grad_device): the CURRENT weights, normaliser and log_std of the rollout's policy, the recorded actions, ``logp`` and
        sets of `rollout`, adv [T, N] float32 CUDA (``advantages``), rows: an int64 CUDA tensor of flat (step, env) indices t * N + n (a
        minibatch; None: every row), loss "ppo_clip" or "coef", adv_stats: the float64 [3] tensor of ``advantages(..., stats=True)`` to
        normalise the advantage with.  Returns (grads, g_log_std, stats): grads a list of (gW, gb) in ``load_policy``'s layout, g_log_std
        [G], stats float64 [6] (rows, sum of loss terms, sum of entropies, sum of logp_old - logp_new, rows clipped away, sum of ratios) --
        CUDA tensors the next call with the same policy overwrites.  An optimiser step on them and ``policy.set_weights_device`` /
        ``set_log_std_device`` close the loop.  into: an optimiser ``make_optimizer`` made for the rollout's policy -- the gradient is
        written into ITS buffers, the returned grads and g_log_std are views of them, and ``optimizer_step`` closes the loop."""
        ent, _ = self._policy_grad_call(rollout, adv, rows, loss, clip_eps, ent_coef, adv_stats, True, into)
        return ent["grads"], ent["g_log_std"], ent["stats"]

    def evaluate_actions(self, rollout, rows=None):
        """(logp_new, entropy) float32 [R] CUDA: the rollout's policy as it is NOW on the recorded actions of `rows` (None: every row, flat
        [T * N]), the forward alone; the next call with the same R overwrites them"""
        _, out = self._policy_grad_call(rollout, None, rows, "coef", 0.0, 0.0, None, False)
        return out

    # ---- a critic on the device (chub_critic_*): values for ``advantages`` and the value loss's gradient with no autograd
    def load_critic(self, module_or_layers, normalize=None):
        """A feed-forward value network -> DeviceCritic (VecChargingHub.make_critic), for calls of up to 96 * num_envs rows (a rollout).
        module_or_layers: what ``load_policy`` accepts -- an ``nn.Sequential`` of ``Linear`` / ``Tanh`` / ``ReLU`` (one activation behind
        every hidden Linear, nothing behind the last, which has one output), or a list of ``(W, b)`` tensors / arrays in the nn.Linear
        layout (hidden activation tanh).  Its rows are the feature rows of the actor it is trained beside: ``Linear(F, ..)``.  normalize:
        None or (mean [F], inv_std [F], clip), the critic's own.  The weights are copied; after an optimiser step
        ``critic.set_weights_device(l, linear.weight.data_ptr(), linear.bias.data_ptr(), stream)`` brings layer l up to date."""
        torch = self.torch
        hidden = None
        if isinstance(module_or_layers, torch.nn.Module):
            layers, acts = [], []
            for m in module_or_layers.children():
                if isinstance(m, torch.nn.Linear):
                    if m.bias is None:
                        raise ValueError("load_critic: every Linear needs a bias")
                    layers.append((m.weight.detach().to("cpu", torch.float32).numpy(), m.bias.detach().to("cpu", torch.float32).numpy()))
                    acts.append(None)
                elif isinstance(m, (torch.nn.Tanh, torch.nn.ReLU)) and layers and acts[-1] is None:
                    acts[-1] = "tanh" if isinstance(m, torch.nn.Tanh) else "relu"
                else:
                    raise ValueError("load_critic: an nn.Sequential of Linear / Tanh / ReLU, not %s here" % type(m).__name__)
            if not layers:
                raise ValueError("load_critic: no Linear layer")
            if len(set(acts[:-1])) > 1 or None in acts[:-1]:
                raise ValueError("load_critic: one activation, Tanh or ReLU, behind every hidden Linear")
            if acts[-1] is not None:
                raise ValueError("load_critic: nothing may follow the last Linear (the value is a linear output)")
            hidden = acts[0] if len(acts) > 1 else None
        else:
            layers = [(W.detach().to("cpu", torch.float32).numpy() if hasattr(W, "detach") else W,
                       b.detach().to("cpu", torch.float32).numpy() if hasattr(b, "detach") else b) for W, b in module_or_layers]
        return self.vec.make_critic(layers, hidden_act=hidden or "tanh", normalize=normalize, max_rows=96 * self.num_envs)

    def _critic_rollout(self, critic, rollout, who):
        policy = getattr(self, "_rollout_policy", {}).get(id(rollout))
        if policy is None:
            raise ValueError("rollout: a dict returned by this adapter's collect()")
        feats = rollout["features"]
        if critic.n_features != int(feats.shape[2]):
            raise ValueError("%s: the critic reads rows of %d floats, the rollout's feature rows have %d" % (who, critic.n_features, int(feats.shape[2])))
        cache = getattr(self, "_critics", None)
        if cache is None:
            cache = self._critics = {}
        ent = cache.get(id(critic))
        if ent is None:
            f32 = dict(dtype=self.torch.float32, device=self.device)
            ent = cache[id(critic)] = {"grads": [(self.torch.zeros((o, i), **f32), self.torch.zeros((o,), **f32)) for o, i in critic.layer_shapes],
                                       "stats": self.torch.zeros((6,), dtype=self.torch.float64, device=self.device), "values": {}}
        return policy, feats, ent

    def values(self, critic, rollout):
        """The critic over a ``collect`` rollout, on torch's current stream (chub_critic_values_device) -> (values [T + 1, N],
        final_values [N] or None), float32 CUDA tensors ready for ``advantages`` that the next call with the same critic and T
        overwrites.  values[t], t < T: the critic on ``rollout["features"][t]``, the rows the actor saw, in ONE launch over T * N rows.
        values[T]: the critic on the feature row of the state NOW -- the last packed block for an actor that reads the observation alone;
        otherwise the actor's feature launches fill a scratch row first (``sample_device(d_features=...)``, which consumes no tick).
        final_values: the critic on ``last_obs`` under ``autoreset="per_env"`` with an observation-only actor; otherwise None: an
        episode's end is worth 0 (the state behind a terminal feature row is gone)."""
        torch = self.torch
        policy, feats, ent = self._critic_rollout(critic, rollout, "values")
        T, N, F, D = int(feats.shape[0]), self.num_envs, critic.n_features, self.obs_dim
        out = ent["values"].get(T)
        if out is None:
            f32 = dict(dtype=torch.float32, device=self.device)
            out = ent["values"][T] = (torch.zeros((T + 1, N), **f32), torch.zeros((N,), **f32), torch.zeros((N, F), **f32), torch.zeros((N,), **f32))
        vals, final, scratch, logp = out
        st = self._stream()
        critic.values_device(T * N, T * N, feats.data_ptr(), vals.data_ptr(), stream=st)
        obs_only = all(policy.spec.inputs[i].kind == _lib.PIN["obs"] for i in range(policy.spec.n_inputs))
        if obs_only:
            critic.values_device(N, N, rollout["packed"][T - 1].data_ptr(), vals[T].data_ptr(), ld=D + 2, stream=st)
        else:
            fresh = self._cur_obs is self._obs0  # (a reset's dense [N, D] block, or the observation columns of the packed block)
            policy.sample_device(self._obs0.data_ptr() if fresh else self._packed.data_ptr(), D if fresh else D + 2, d_logp=logp.data_ptr(),
                                 d_features=scratch.data_ptr(), stream=st)
            critic.values_device(N, N, scratch.data_ptr(), vals[T].data_ptr(), stream=st)
        if not (self.per_env and obs_only):
            return vals, None
        critic.values_device(N, N, self.last_obs.data_ptr(), final.data_ptr(), ld=int(self.last_obs.stride(0)), stream=st)
        return vals, final

    def value_gradient(self, critic, rollout, ret, rows=None, loss="mse", clip_eps=0.2, v_old=None, into=None):
        """The critic's gradient of the value loss over a ``collect`` rollout, on torch's current stream with no autograd
        (chub_critic_grad_device): the critic's CURRENT weights and normaliser on ``rollout["features"]``, ret [T, N] float32 CUDA
        (``advantages``), rows: an int64 CUDA tensor of flat (step, env) indices t * N + n (a minibatch; None: every row), loss "mse" or
        "clipped" (PPO2's clipped value loss around v_old [T, N], e.g. ``values(...)[0][:T]`` as collected, within clip_eps).  Returns
        (grads, stats): grads a list of (gW, gb) in ``load_critic``'s layout, stats float64 [6] (rows, sum of loss terms, rows clipped
        away, sum of (ret - v)^2, sum of ret, sum of ret^2) -- CUDA tensors the next call with the same critic overwrites.  into: an
        optimiser ``make_optimizer`` made for `critic` -- the gradient is written into ITS buffers and the returned grads are views of them."""
        torch = self.torch
        policy, feats, ent = self._critic_rollout(critic, rollout, "value_gradient")
        n_rows = int(feats.shape[0]) * int(feats.shape[1])
        if rows is not None and not (self._on_device(rows) and rows.dtype == torch.int64 and rows.dim() == 1 and rows.is_contiguous()):
            raise AssertionError("rows must be a contiguous 1-d int64 tensor on %s" % (self.device,))
        R = n_rows if rows is None else int(rows.numel())
        per_row = lambda t: self._on_device(t) and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n_rows
        if not per_row(ret):
            raise AssertionError("ret must be a contiguous float32 tensor on %s with one entry per (step, env)" % (self.device,))
        clipped = _lib.value_loss(loss) == _lib.VLOSS["clipped"]
        if clipped and (v_old is None or not per_row(v_old)):
            raise AssertionError("v_old must be a contiguous float32 tensor on %s with one entry per (step, env) under loss='clipped'" % (self.device,))
        grads = ent["grads"] if into is None else self._into(into, critic, "value_gradient")["grads"]
        critic.grad_device(R, n_rows, feats.data_ptr(), ret.data_ptr(), d_v_old=v_old.data_ptr() if clipped else 0,
                           d_rows=0 if rows is None else rows.data_ptr(), loss=loss, clip_eps=clip_eps, d_gW=[gW.data_ptr() for gW, _ in grads],
                           d_gb=[gb.data_ptr() for _, gb in grads], d_stats=ent["stats"].data_ptr(), stream=self._stream())
        return grads, ent["stats"]

    # ---- an optimiser on the device (chub_adam_*, chub_shuffle_rows_device): the update with no torch optimiser and no re-layout
    def _device_view(self, ptr, shape, typestr="<f4"):
        """a tensor over device memory the library owns (only the address and the shape are used)"""
        iface = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2)
        return self.torch.as_tensor(type("DeviceArray", (), {"__cuda_array_interface__": iface})(), device=self.device)

    def make_optimizer(self, policy_or_critic, **hyper):
        """Adam with gradient clipping on the LIVE weights of a ``load_policy`` actor or a ``load_critic`` critic -> DeviceAdam
        (VecChargingHub.make_adam; hyper: lr, betas, eps, weight_decay, max_grad_norm).  ``policy_gradient(..., into=opt)`` /
        ``value_gradient(..., into=opt)`` write the gradient into its own buffers and ``optimizer_step(opt)`` steps from there: the
        next act, sample, values or gradient call sees the new weights with no ``set_weights_device``."""
        opt = self.vec.make_adam(policy_or_critic, **hyper)
        gW, gb, gl = opt.grads()
        opt._views = {"grads": [(self._device_view(gW[l], (o, i)), self._device_view(gb[l], (o,))) for l, (o, i) in enumerate(opt.layer_shapes)],
                      "g_log_std": self._device_view(gl, (opt.target.n_gaussians,)) if gl else None,
                      "stats": self.torch.zeros((4,), dtype=self.torch.float64, device=self.device)}
        return opt

    def _into(self, opt, target, who):
        if opt.target is not target or getattr(opt, "_views", None) is None:
            raise ValueError("%s: into= takes an optimiser this adapter's make_optimizer made for the same policy / critic" % who)
        return opt._views

    def optimizer_step(self, opt):
        """One step of `opt` from the gradients in its own buffers, on torch's current stream (chub_adam_step_device) -> the float64 [4]
        CUDA stats tensor (t, the gradient's norm, the clip scale, 1 where a norm that was not finite skipped the step) the next step of
        `opt` overwrites."""
        views = self._into(opt, opt.target, "optimizer_step")
        opt.step_device(d_stats=views["stats"].data_ptr(), stream=self._stream())
        return views["stats"]

    def optimizer_stats(self, opt):
        """the float64 [4] CUDA stats tensor the last ``optimizer_step(opt)`` wrote (zeros before the first)"""
        return self._into(opt, opt.target, "optimizer_stats")["stats"]

    # ---- a training log and a KL stop on the device (chub_train_log_*, chub_ppo_update): the update as one call, its numbers in one read
    def make_train_log(self):
        """The numbers of a PPO update and its KL stop, kept on the device -> DeviceTrainLog (VecChargingHub.make_train_log): what
        ``ppo_update(..., log=log)`` fills and ``train_log_summary(log)`` reads."""
        return self.vec.make_train_log()

    def ppo_update(self, rollout, adv, ret, policy_opt, critic_opt, *, epochs, minibatch_rows, key, clip_eps, ent_coef, v_old=None,
                   loss="ppo_clip", value_loss="clipped", adv_stats=None, target_kl=None, kl="k3", log=None):
        """A whole PPO update over a ``collect`` rollout, enqueued on torch's current stream by ONE call (chub_ppo_update): `epochs` times a
        shuffle of the rollout's T * N rows under `key` and policy_opt's step count, and per minibatch of minibatch_rows rows (the last of
        an epoch takes the remainder) the actor gradient, the critic gradient, the two optimiser steps.  adv, ret [T, N] float32 CUDA
        (``advantages``), v_old [T, N] under value_loss="clipped"; policy_opt / critic_opt: ``make_optimizer`` of the rollout's policy and of
        the critic; clip_eps serves both losses.  log: a ``make_train_log`` log -- the update begins it, every minibatch is recorded into
        it, and with target_kl the update stops stepping at the first minibatch whose approximate KL (kl: "k3", the mean of
        (ratio - 1) - log ratio, or "k1", the mean of -log ratio) is not <= 1.5 * target_kl: stable-baselines3's rule, factor included.
        target_kl needs a log.  Nothing is read back; the call may be recorded into a graph, whose replays each begin the log anew.  After
        a stop the remaining gradient launches still run; their steps are held back."""
        torch = self.torch
        policy = getattr(self, "_rollout_policy", {}).get(id(rollout))
        if policy is None:
            raise ValueError("rollout: a dict returned by this adapter's collect()")
        if policy_opt.target is not policy:
            raise ValueError("ppo_update: policy_opt is not an optimiser of the rollout's policy")
        critic = critic_opt.target
        if target_kl is not None and log is None:
            raise ValueError("ppo_update: target_kl needs log= (the stop is a word of the log)")
        feats = rollout["features"]
        n_rows = int(feats.shape[0]) * int(feats.shape[1])
        per_row = lambda t: t is not None and self._on_device(t) and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n_rows
        clipped = _lib.value_loss(value_loss) == _lib.VLOSS["clipped"]
        if not per_row(adv) or not per_row(ret) or (clipped and not per_row(v_old)):
            raise AssertionError("adv, ret (and v_old under value_loss='clipped') must be contiguous float32 tensors on %s with one entry per "
                                 "(step, env)" % (self.device,))
        if adv_stats is not None and not (self._on_device(adv_stats) and adv_stats.dtype == torch.float64 and adv_stats.is_contiguous()
                                          and adv_stats.numel() == 3):
            raise AssertionError("adv_stats must be a contiguous float64 tensor on %s of 3 entries (advantages(..., stats=True))" % (self.device,))
        mb = min(int(minibatch_rows), n_rows)  # (one minibatch per epoch either way)
        ent = self._policy_grad_entry(policy, n_rows, n_rows)
        rows_cache = getattr(self, "_ppo_rows", None)
        if rows_cache is None:
            rows_cache = self._ppo_rows = {}
        rows = rows_cache.get(n_rows)
        if rows is None:
            rows = rows_cache[n_rows] = torch.zeros((n_rows,), dtype=torch.int64, device=self.device)
        piles = policy.spec.head == _lib.PHEAD["piles"]
        sets = rollout.get("set_bits") if piles else None
        self.vec.ppo_update(ent["grad"], critic, policy_opt, critic_opt, n_rows, feats.data_ptr(), rollout["u"].data_ptr(), rollout["logp"].data_ptr(),
                            adv.data_ptr(), ret.data_ptr(), rows.data_ptr(), epochs, mb, key, d_pile_bits=rollout["bits"].data_ptr() if piles else 0,
                            d_set_bits=0 if sets is None else sets.data_ptr(), d_adv_stats=0 if adv_stats is None else adv_stats.data_ptr(),
                            d_v_old=v_old.data_ptr() if clipped else 0, loss=loss, value_loss=value_loss, clip_eps=clip_eps, value_clip_eps=clip_eps,
                            ent_coef=ent_coef, kl=kl, kl_limit=0.0 if target_kl is None else 1.5 * float(target_kl), log=log, stream=self._stream())
        return rows

    # ---- constrained PPO on the device (chub_lagrange_*): cost advantages, multipliers, the combined advantage
    def make_constraints(self, constraints):
        """Constraints with their Lagrange multipliers on the device -> DeviceLagrange (VecChargingHub.make_lagrange).  constraints: up to
        four dicts ``dict(term="grid_excess", kind="step", limit=.., lr=.., lambda0=0, lambda_max=0)``: term a name of _lib.ST_NAMES,
        kind "step" (the term's value at every step) or "done" (its value where the episode ends, 0 elsewhere; on "soc_penalty" the
        reference's test_penalty), limit the bound on an episode's mean cost, lr the multiplier's step, lambda_max 0 = no ceiling.  The
        object's ``terms`` is the ``terms=`` tuple ``collect`` must be given: the distinct terms, so that a terms row holds nothing else."""
        names = _lib.st_fields_names(_lib.st_fields_mask([c["term"] for c in constraints]))
        rows = [dict(column=names.index(c["term"]), kind=c.get("kind", "step"), limit=c.get("limit", 0.0), lr=c.get("lr", 0.0),
                     lambda0=c.get("lambda0", 0.0), lambda_max=c.get("lambda_max", 0.0)) for c in constraints]
        lag = self.vec.make_lagrange(rows)
        lag.terms = names
        lag.term_of = tuple(c["term"] for c in constraints)
        return lag

    def _own_constraints(self, constraints, who):
        if getattr(constraints, "_env", None) is not self.vec:
            raise ValueError("%s: the constraints were made for another handle" % who)

    def cost_advantages(self, rollout, constraints, cost_values=None, final_values=None, gamma=0.99, lam=0.95):
        """Cost GAE over a ``collect(..., terms=constraints.terms)`` rollout for every constraint in one pass, on torch's current stream
        (chub_lagrange_gae_device): cost_values, a sequence with per constraint a [T + 1, N] float32 CUDA tensor (the cost critic as
        ``advantages`` takes the reward critic's values) or None (V = 0); final_values likewise [N].  Returns (advs, rets): per constraint
        a float32 [T, N] CUDA tensor, overwritten by the next call with the same T.  The cost of episodes still running at the rollout's
        end is carried to the next call in a [N, K] float64 tensor of the object's; the stats ``update_multipliers`` reads are left
        in the object."""
        torch = self.torch
        self._own_constraints(constraints, "cost_advantages")
        if "terms" not in rollout or tuple(rollout["terms_names"]) != tuple(constraints.terms):
            raise ValueError("cost_advantages: the rollout must be collected with terms=constraints.terms %r" % (constraints.terms,))
        T, N, K = int(rollout["packed"].shape[0]), self.num_envs, constraints.K
        ok = lambda t, shape: self._on_device(t) and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
        vals = list(cost_values) if cost_values is not None else [None] * K
        fins = list(final_values) if final_values is not None else [None] * K
        if len(vals) != K or len(fins) != K:
            raise ValueError("cost_advantages: one entry per constraint (%d)" % K)
        for v in vals:
            if v is not None and not ok(v, (T + 1, N)):
                raise AssertionError("cost_values[k] must be a contiguous float32 tensor on %s of shape (%d, %d)" % (self.device, T + 1, N))
        for v in fins:
            if v is not None and not ok(v, (N,)):
                raise AssertionError("final_values[k] must be a contiguous float32 tensor on %s of shape (%d,)" % (self.device, N))
        cache = constraints.__dict__.setdefault("_torch", {})
        if "carry" not in cache:
            cache["carry"] = torch.zeros((N, K), dtype=torch.float64, device=self.device)
        out = cache.get(("gae", T))
        if out is None:
            out = cache[("gae", T)] = ([torch.zeros((T, N), dtype=torch.float32, device=self.device) for _ in range(K)],
                                       [torch.zeros((T, N), dtype=torch.float32, device=self.device) for _ in range(K)])
        advs, rets = out
        constraints.gae(T, len(constraints.terms), rollout["terms"].data_ptr(), rollout["packed"].data_ptr(), [a.data_ptr() for a in advs],
                        d_ret=[r.data_ptr() for r in rets], d_values=[0 if v is None else v.data_ptr() for v in vals],
                        d_final_values=[0 if v is None else v.data_ptr() for v in fins], gamma=gamma, lam=lam,
                        d_ep_carry=cache["carry"].data_ptr(), stream=self._stream())
        return advs, rets

    def update_multipliers(self, constraints):
        """One step of projected dual ascent on every multiplier, from the episodes the last ``cost_advantages`` saw finish, on torch's
        current stream (chub_lagrange_step_device).  A rollout in which no episode finished moves nothing and counts as skipped."""
        self._own_constraints(constraints, "update_multipliers")
        constraints.step(stream=self._stream())

    def constrained_advantages(self, adv, adv_stats, cost_advs, constraints):
        """The advantage a PPO-Lagrangian update ascends, in one streaming launch on torch's current stream (chub_lagrange_combine_device):
        (A - sum_k lambda_k (A_k - mean A_k)) / (1 + sum_k lambda_k) with A the reward advantage, normalised by adv_stats where given
        (``advantages(..., stats=True)``), and A_k the cost advantages of the last ``cost_advantages``.  Returns a float32 tensor of adv's
        shape (overwritten by the next call of the same size): hand it to ``policy_gradient`` / ``ppo_update`` as adv with adv_stats=None."""
        torch = self.torch
        self._own_constraints(constraints, "constrained_advantages")
        n = adv.numel()
        flat = lambda t: self._on_device(t) and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n
        if not flat(adv) or len(cost_advs) != constraints.K or not all(flat(c) for c in cost_advs):
            raise AssertionError("adv and one cost advantage per constraint must be contiguous float32 tensors on %s of one size" % (self.device,))
        if adv_stats is not None and not (self._on_device(adv_stats) and adv_stats.dtype == torch.float64 and adv_stats.is_contiguous()
                                          and adv_stats.numel() == 3):
            raise AssertionError("adv_stats must be a contiguous float64 tensor on %s of 3 entries (advantages(..., stats=True))" % (self.device,))
        cache = constraints.__dict__.setdefault("_torch", {})
        out = cache.get(("combined", tuple(adv.shape)))
        if out is None:
            out = cache[("combined", tuple(adv.shape))] = torch.zeros(tuple(adv.shape), dtype=torch.float32, device=self.device)
        constraints.combine(n, adv.data_ptr(), [c.data_ptr() for c in cost_advs], out.data_ptr(),
                            d_adv_stats=0 if adv_stats is None else adv_stats.data_ptr(), stream=self._stream())
        return out

    def constraint_summary(self, constraints):
        """One synchronising read of the constraints -> a list with per constraint a dict: term, kind, limit, lambda, cost (J_last: the
        mean episode cost the last taken step saw), episodes and episode_cost_mean of the last ``cost_advantages``, steps, skipped."""
        self._own_constraints(constraints, "constraint_summary")
        lam, st, w = constraints.read()
        out = []
        for k, c in enumerate(constraints.constraints):
            out.append(dict(term=constraints.term_of[k] if hasattr(constraints, "term_of") else c["column"], kind=_lib.COST_KIND_NAMES[c["kind"]],
                            limit=c["limit"], **{"lambda": float(lam[k])}, cost=float(w[k, 0]), episodes=int(st[k, 3]),
                            episode_cost_mean=float(st[k, 4] / st[k, 3]) if st[k, 3] else float("nan"), steps=int(w[k, 1]), skipped=int(w[k, 2])))
        return out

    def train_log_summary(self, log, kl="k3"):
        """One synchronising read of `log` -> a dict under stable-baselines3's names.  Over the counted minibatches, weighted by rows:
        approx_kl (kl: "k3" or "k1"), clip_fraction, entropy, policy_loss, value_loss, value_clip_fraction, explained_variance
        (1 - E(ret - v)^2 / Var ret from the critic's sums); approx_kl_max, the largest single minibatch's estimate as recorded;
        n_minibatches; stopped_at (None, or the index of the minibatch that set the stop); and per optimiser, under "policy_opt" and
        "critic_opt": steps, skipped, held_back, grad_norm_mean, grad_norm_max, clipped_steps."""
        return train_log_summary(log.read(), kl)

    def shuffle_rows(self, R, key, counter=None, offset=0):
        """A permutation of 0 .. R - 1 as an int64 CUDA tensor, on torch's current stream (chub_shuffle_rows_device): a pure function
        of (key, counter + offset, R).  counter: None (0), an optimiser (its step count, read on the device when the launch runs), or an
        int64 CUDA tensor of one entry.  Slices of it are the ``rows`` of ``policy_gradient`` / ``value_gradient``."""
        torch = self.torch
        rows = torch.empty((int(R),), dtype=torch.int64, device=self.device)
        d_counter = 0 if counter is None else counter.counter_address if hasattr(counter, "counter_address") else counter.data_ptr()
        self.vec.shuffle_rows_device(rows.data_ptr(), R, key, d_counter=d_counter, offset=offset, stream=self._stream())
        return rows

    def _weights(self, target):
        torch = self.torch
        f32 = dict(dtype=torch.float32, device=self.device)
        out = [(torch.empty((o, i), **f32), torch.empty((o,), **f32)) for o, i in target.layer_shapes]
        for l, (W, b) in enumerate(out):
            target.get_weights_device(l, W.data_ptr(), b.data_ptr(), stream=self._stream())
        return out

    def policy_weights(self, policy):
        """The actor's LIVE weights -> ([(W, b), ..] in nn.Linear's layout, log_std [G] or None), new float32 CUDA tensors filled on
        torch's current stream (chub_policy_get_weights_device)"""
        log_std = None
        if policy.has_exploration:
            log_std = self.torch.empty((policy.n_gaussians,), dtype=self.torch.float32, device=self.device)
            policy.get_log_std(log_std.data_ptr(), stream=self._stream())
        return self._weights(policy), log_std

    def critic_weights(self, critic):
        """The critic's LIVE weights -> [(W, b), ..] in nn.Linear's layout, new float32 CUDA tensors filled on torch's current stream"""
        return self._weights(critic)

    # ---- reward scaling by running return statistics (chub_return_norm_*): VecNormalize's norm_reward with nothing read back
    def make_reward_normalizer(self, gamma=0.99, eps=1e-8, clip=10.0):
        """Running statistics of the discounted return, per env across rollouts, and the reward scale 1 / sqrt(var + eps) they give ->
        DeviceReturnNorm (VecChargingHub.make_return_norm).  gamma is the discount of the tracked return (the trainer's), clip bounds
        the scaled reward (0: none).  ``update_reward_normalizer`` then ``advantages(..., reward_norm=rn)`` per rollout, as VecNormalize
        updates before it normalises.  Episode accounting (``episode_stats``) stays in raw units."""
        return self.vec.make_return_norm(gamma=gamma, eps=eps, clip=clip)

    def _own_reward_norm(self, rn, who):
        if getattr(rn, "_env", None) is not self.vec:
            raise ValueError("%s: the reward normaliser was made for another handle" % who)

    def update_reward_normalizer(self, rollout, rn, mask=None):
        """Add the discounted returns of a ``collect`` rollout to `rn` and set its scale from them, two launches on torch's current
        stream (chub_return_norm_update_device).  The return of an env's running episode is carried to the next call.  mask: a uint8 /
        bool CUDA tensor [N]; only the envs it names count or move their carry.  Returns rn."""
        torch = self.torch
        self._own_reward_norm(rn, "update_reward_normalizer")
        packed = rollout["packed"]
        if not (self._on_device(packed) and packed.dtype == torch.float32 and packed.is_contiguous() and packed.dim() == 3
                and tuple(packed.shape[1:]) == (self.num_envs, self.obs_dim + 2)):
            raise AssertionError("rollout['packed'] must be a contiguous float32 tensor on %s of shape (T, %d, %d)"
                                 % (self.device, self.num_envs, self.obs_dim + 2))
        d_mask = 0
        if mask is not None:
            if not (self._on_device(mask) and mask.dtype in (torch.uint8, torch.bool) and mask.is_contiguous() and tuple(mask.shape) == (self.num_envs,)):
                raise AssertionError("mask must be a contiguous uint8 or bool tensor on %s of shape (%d,)" % (self.device, self.num_envs))
            d_mask = mask.data_ptr()
        rn.update_device(int(packed.shape[0]), packed.data_ptr(), d_mask=d_mask, stream=self._stream())
        return rn

    def reward_scale(self, rn):
        """The scale `rn` multiplies rewards by, as a float32 [1] CUDA tensor over the object's own word: nothing is read or copied, and a
        later update shows in it (clone it to keep a value)."""
        self._own_reward_norm(rn, "reward_scale")
        return self._device_view(rn.scale_address, (1,))

    # ---- a normaliser that follows the rollouts (chub_moments_*, chub_policy_normalizer_from_moments_device)
    def update_normalizer(self, policy, rollout, moments=None, eps=1e-8, mask=None):
        """Running observation statistics, VecNormalize-style, with nothing read back: add the raw feature rows of a ``collect`` rollout
        (``rollout["features"]`` [T, N, F]) to `moments` (a DeviceMoments; None: one the adapter makes and keeps per policy), then set the
        policy's normaliser from them, mean and 1 / sqrt(var + eps) -- three launches on torch's current stream.  mask: a uint8 / bool CUDA
        tensor [N]; only the rows of the envs it names count.  The rollout's ``logp`` was recorded under the normaliser in force BEFORE this
        call: take ``policy_normalizer(policy)`` first if the trainer is to reproduce z from ``features`` (``normalize_features``).  Returns
        the moments object."""
        torch = self.torch
        feats = rollout["features"]
        F = policy.n_features
        if not (self._on_device(feats) and feats.dtype == torch.float32 and feats.is_contiguous() and feats.dim() == 3
                and tuple(feats.shape[1:]) == (self.num_envs, F)):
            raise AssertionError("rollout['features'] must be a contiguous float32 tensor on %s of shape (T, %d, %d)" % (self.device, self.num_envs, F))
        if moments is None:
            cache = getattr(self, "_moments", None)
            if cache is None:
                cache = self._moments = {}
            moments = cache.get(id(policy))
            if moments is None:
                moments = cache[id(policy)] = self.vec.make_moments(F)
        d_mask = 0
        if mask is not None:
            if not (self._on_device(mask) and mask.dtype in (torch.uint8, torch.bool) and mask.is_contiguous() and tuple(mask.shape) == (self.num_envs,)):
                raise AssertionError("mask must be a contiguous uint8 or bool tensor on %s of shape (%d,)" % (self.device, self.num_envs))
            d_mask = mask.data_ptr()
        moments.update_device(feats.data_ptr(), int(feats.shape[0]) * self.num_envs, ld=F, d_mask=d_mask, stream=self._stream())
        policy.normalizer_from_moments(moments, eps=eps, stream=self._stream())
        return moments

    def policy_normalizer(self, policy):
        """(mean, inv_std): the normaliser `policy` evaluates with, as two new float32 [F] CUDA tensors filled on torch's current stream
        (chub_policy_get_normalizer_device): no synchronisation"""
        torch = self.torch
        mean = torch.empty((policy.n_features,), dtype=torch.float32, device=self.device)
        inv_std = torch.empty_like(mean)
        policy.get_normalizer_device(mean.data_ptr(), inv_std.data_ptr(), stream=self._stream())
        return mean, inv_std

    def copy_envs(self, src_idx, dst_idx, source=None):
        """env dst_idx[i] becomes a clone of env src_idx[i] of `source` (another TorchHubVecEnv; default: this one), on torch's current
        stream and without a host read: the indices are int64 CUDA tensors as torch.topk returns them (chub_copy_envs_device: distinct
        destinations, within one adapter no env both source and destination -- e.g. the top k and the bottom k of one ranking, 2 k <= N).
        The cached observation rows are copied along, so the rows the last reset / step returned stay the envs' current observations.
        With ``autoreset=True`` copy between adapters that are at the same step of the day (that mode counts one clock for the whole
        batch); with ``autoreset="per_env"`` the adapters may be at any times of day: a clone keeps its source's clock and ends its
        day when that clock does."""
        torch = self.torch
        src = self if source is None else source
        for name, t in (("src_idx", src_idx), ("dst_idx", dst_idx)):
            if not (self._on_device(t) and t.dtype == torch.int64 and t.dim() == 1):
                raise AssertionError("%s must be a 1-d int64 tensor on %s" % (name, self.device))
        if src_idx.numel() != dst_idx.numel():
            raise AssertionError("src_idx and dst_idx must have the same length")
        s, d = src_idx.contiguous(), dst_idx.contiguous()
        self.vec.copy_envs_device(s.data_ptr(), d.data_ptr(), s.numel(), source=src.vec, stream=self._stream())
        if self._cur_obs is not None and src._cur_obs is not None:
            self._cur_obs.index_copy_(0, d, src._cur_obs.index_select(0, s))
        return self._cur_obs

    def close(self):
        self.vec.close()


class StaggeredHub(object):
    """Non-lock-step episodes: G groups of envs whose days are offset against each other by 96/G slots.

    The N envs of a VecChargingHub that is only ever reset and stepped as a whole share one clock, so all N episodes end
    in the same step -- convenient for the kernels, but a learner then sees every env at the same time of day.  This front
    splits the env range into G contiguous groups (global env ids unchanged: group g covers ``[g*N/G, (g+1)*N/G)``) and keeps
    group g ``g * 96 // G`` slots ahead: ``reset()`` resets all groups and then walks group g through its head start with
    the all-on action (the reference's ``step(None)``, MGR:146-147).  ``step()`` steps every group, and a group whose day
    has ended (its own ``done``) is reset on the spot (``autoreset=True``): the returned observation rows of that group are
    the first of its next episode, ``info['terminal_observation']`` keeps the last ones and ``info['reset_groups']`` lists
    the groups reset in this step.

    Two forms.  The default keeps one hub per group: every group is bit-identical to a plain hub over the same global env
    range given the same head start.  ``one_handle=True`` runs all N envs in ONE hub with per-env clocks
    (``reset_envs`` / ``step_envs``, include/chub.h): one allocation, one launch per call whatever the number of groups
    (65 536 envs in 8 groups: 1.9 G env-steps/s on the device-pointer path); its Philox ticks count the handle's calls, so
    its random streams differ from the per-group form's (same distribution).
    """

    def __init__(self, n_envs, groups, station_list, station_type_list, seed=0, env_id0=0, autoreset=True,
                 hub_factory=None, one_handle=False, **hub_kwargs):
        groups = int(groups)
        if groups < 1 or n_envs % groups:
            raise ValueError("n_envs must split evenly over the groups")
        if groups > 96:
            raise ValueError("at most 96 groups (one per slot of the day)")
        make = hub_factory or VecChargingHub
        self.n_envs, self.groups, self.per = int(n_envs), groups, int(n_envs) // groups
        self.offsets = [g * 96 // groups for g in range(groups)]
        self.hub = None
        if one_handle:
            self.hub = make(self.n_envs, station_list, station_type_list, seed=seed, env_id0=env_id0, **hub_kwargs)
            self.hubs = [self.hub]
        else:
            self.hubs = [make(self.per, station_list, station_type_list, seed=seed, env_id0=env_id0 + g * self.per,
                              **hub_kwargs) for g in range(groups)]
        self.obs_dim, self.act_dim = self.hubs[0].obs_dim, self.hubs[0].act_dim
        self.piles, self.n_slots = self.hubs[0].piles, self.act_dim - 2
        self.autoreset = bool(autoreset)

    def _rows(self, g):
        return slice(g * self.per, (g + 1) * self.per)

    def _mask(self, gs):
        m = np.zeros(self.n_envs, dtype=bool)
        for g in gs:
            m[self._rows(g)] = True
        return m

    @property
    def clocks(self):
        """slot of day of every group"""
        if self.hub is not None:
            return [int(t) for t in self.hub.env_clocks()[::self.per]]
        return [h.clock for h in self.hubs]

    def reset(self):
        if self.hub is not None:
            head = np.zeros((self.n_envs, self.act_dim), dtype=np.float32)
            head[:, :self.n_slots] = 1.0  # step(None): every pile on, fuel cell and electrolyser at 0 (MGR:146-147, 384-404)
            obs = self.hub.reset()
            for k in range(1, max(self.offsets) + 1):  # the k-th head-start step: every group that is at least k slots ahead
                obs = self.hub.step_envs(self._mask([g for g in range(self.groups) if self.offsets[g] >= k]), head)[0]
            return obs
        obs = np.zeros((self.n_envs, self.obs_dim), dtype=np.float32)
        head = np.zeros((self.per, self.act_dim), dtype=np.float32)
        head[:, :self.n_slots] = 1.0  # step(None): every pile on, fuel cell and electrolyser at 0 (MGR:146-147, 384-404)
        for g, h in enumerate(self.hubs):
            o = h.reset()
            for _ in range(self.offsets[g]):
                o = h.step(head)[0]
            obs[self._rows(g)] = o
        return obs

    def step(self, actions):
        a = np.ascontiguousarray(actions, dtype=np.float32)
        if a.shape != (self.n_envs, self.act_dim):  # MGR:148
            raise AssertionError("actions must have shape (%d, %d)" % (self.n_envs, self.act_dim))
        info = {}
        if self.hub is not None:
            obs, reward, done, _ = self.hub.step(a)
            ended = [g for g in range(self.groups) if done[self._rows(g)].all()]
            if ended and self.autoreset:
                info["terminal_observation"] = np.zeros_like(obs)
                m = self._mask(ended)
                info["terminal_observation"][m] = obs[m]
                info["reset_groups"] = ended
                obs = self.hub.reset_envs(m)
            return obs, reward, done, info
        obs = np.zeros((self.n_envs, self.obs_dim), dtype=np.float32)
        reward = np.zeros(self.n_envs, dtype=np.float32)
        done = np.zeros(self.n_envs, dtype=bool)
        for g, h in enumerate(self.hubs):
            rows = self._rows(g)
            o, r, d, _ = h.step(a[rows])
            reward[rows], done[rows] = r, d
            if d.all() and self.autoreset:
                info.setdefault("terminal_observation", np.zeros_like(obs))[rows] = o
                info.setdefault("reset_groups", []).append(g)
                o = h.reset()
            obs[rows] = o
        return obs, reward, done, info

    def set_telemetry(self, on=True):
        for h in self.hubs:
            h.set_telemetry(on)

    def telemetry(self):
        return np.concatenate([h.telemetry() for h in self.hubs], axis=0)

    def close(self):
        for h in self.hubs:
            h.close()


__all__ = ["ENV_ID", "StaggeredHub", "TorchHubVecEnv", "MAX_EPISODE_STEPS", "TimeLimit", "make", "register", "HubVecEnv", "HubVectorEnv",
           "telemetry_info", "Box"]
