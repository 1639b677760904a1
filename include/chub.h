/* chub.h -- C ABI of the MI355X-native vectorised charging-hub environment runtime (libchub.so).
 *
 * Drop-in boundary.  In the reference the Python host (evcssp_env_cpp/envs/evcssp_manager.py:19,
 * class EvcsspManagerEnv_v6) reaches its native core through the Boost.Python module `pyevstation`
 * (evcssp_env_cpp/envs/lion_cpp20/main.cpp:19-290).  This header is what replaces that module for
 * the reset()/step() hot path: plain pointers and sizes, no Python / torch / Boost types.  Each entry
 * point names the reference interface it stands in for.  Everything behind it runs on the GPU; there
 * is no CPU fallback -- every call fails with CHUB_ERR_HIP when no device is usable.
 *
 * Conventions
 *   - N = n_envs, S = piles[0] + piles[1], D = chub_obs_dim(), A = S + 2.
 *   - all arrays are dense row-major; "host" pointers are ordinary CPU memory owned by the caller,
 *     "device" pointers are HIP device memory on the handle's device, owned by the caller.
 *   - every function returns 0 on success or a negative CHUB_ERR_* code; chub_last_error() gives the
 *     message of the calling thread's last failure.  Nothing is printed (the reference prints and
 *     carries on, CHS.hpp:103,292,825).
 *   - a handle is not thread-safe; use one host thread per handle (the reference is single-threaded
 *     with process-global state, CHS.hpp:23-25).
 */
#ifndef CHUB_H
#define CHUB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHUB_VERSION 1

enum {
    CHUB_OK = 0,
    CHUB_ERR_ARG = -1,      /* bad argument (the reference: AssertionError / ValueError, MGR:37,148; AGG:196) */
    CHUB_ERR_DATA = -2,     /* data files missing or malformed (the reference: silent UB, CHS.hpp:102-105,733) */
    CHUB_ERR_HIP = -3,      /* HIP runtime failure / no GPU */
    CHUB_ERR_UNSUPPORTED = -4,
    CHUB_ERR_COMM = -5      /* RCCL failure (multi-GPU gather) */
};

enum { CHUB_FAST = 0, CHUB_SLOW = 1 };

/* RNG modes.  COMPAT reproduces the reference's two process-global streams per environment (glibc
 * rand() TYPE_3 + std::minstd_rand0, CHS.hpp:23-45) in the reference's consumption order; exogenous
 * normals / day indices come from the caller (the reference draws them from numpy / random, REN:25,74).
 * PHILOX is the production mode: counter-based Philox4x32-10, key = seed, counter = (block,
 * site<<16|index, tick, global env id); results do not depend on how envs are sharded over GPUs.  Its EV
 * arrival SoC takes one of 2048 equiprobable classes and car_step is read from per-class tables.
 * PHILOX_CURVES: PHILOX's draws, keyed exactly as in PHILOX, with the reference's CONTINUOUS arrival SoC
 * (CHS.hpp:803-814) and car_step evaluated on the device along the reference's curves (CHS.hpp:467-726, the
 * arithmetic COMPAT is pinned with); station sums as in PHILOX (integers of 2^-19 kW, independent of order).
 *   The draw contract: a car admitted into hub slot j of global env g at the launch's tick uses the SAME Philox
 *   block as PHILOX, block(SITE_SOC = 5, j, 0) -- counter (0, 5 << 16 | j, tick, g), key = seed: word 1 % 1000 is
 *   the target level and word 2 the extra stay, as in PHILOX; word 0 gives the arrival SoC by linear
 *   interpolation of the 4097-node inverse CDF of clip(N(7,3),1,10) (12 bits pick the cell, 20 interpolate;
 *   soc = 75 - 5 d), where PHILOX takes the class word 0 >> 21.  So on one seed the cars, targets and extra
 *   stays at reset are those of PHILOX, each car's SoC lies inside its PHILOX class's cell of the table (nodes
 *   2c .. 2c + 2), and trajectories part after the reset because a stay depends on the SoC.  Everything else
 *   (arrival counts, renege / balk, evs_reset's occupancy, the forecourt, OU) draws PHILOX's counters.
 *   Not in this mode (CHUB_ERR_UNSUPPORTED with a message): stations of more than 64 piles, the scalar-load
 *   control (chub_step_load*), chub_tape_register_soc (the car tape's .x carries the f32 bits of each
 *   recorded arrival SoC instead of a class id), chub_set_slots.  The chub_options that pick the packed /
 *   one-launch / span kernels are accepted and have no effect: chub_uses_packed_kernel returns 0 and
 *   chub_run_steps issues its steps one by one.  Snapshots of one mode are refused by a handle of another.
 *   Stays: a stay is ceil(needed slots) + the extra stay, as in PHILOX, and is kept in five bits; chub_create refuses curves on which
 *   one could exceed 31, so no stay of this mode is ever clamped (the oracle's back-end of this mode does not clamp either: it raises
 *   orc_station.stay_overflow, which the tests assert stays 0). */
enum { CHUB_RNG_COMPAT = 0, CHUB_RNG_PHILOX = 1, CHUB_RNG_PHILOX_CURVES = 2 };

/* Constructor kwargs of EvcsspManagerEnv_v6 (MGR:25-27), same names and meaning.  use_lagrange is
 * ignored by the reference (MGR:126) and has no field.  seed_rand maps to the seeds given at create. */
typedef struct chub_config {
    int32_t station_list[2];      /* piles per station; 0 = station absent from obs but still simulated.  At most 4096 per station (the reference's
                                     constructors take any count, CHS.hpp:1148, 1458): CHUB_ERR_UNSUPPORTED beyond -- see INTEGRATION.md */
    int32_t station_type_list[2]; /* CHUB_FAST / CHUB_SLOW */
    int32_t constant_charging;
    int32_t reserved0;
    double hydro_prod_rate;       /* m^3/h  (None -> 430, HYD:140-143) */
    double hydro_store_vlt;       /* m^3    (None -> 5000, HYD:96) */
    double init_soc;              /* 0.1 .. 1 (HYD:137) */
    double fc_max_power;          /* kW     (None -> 100, HYD:401-404) */
    double fcev_permeate;
    double renew_fluctuate;
    double price_fluctuate;
    double hydro_loss;
} chub_config;

typedef struct chub_env chub_env;

/* Build options that are not constructor kwargs of the reference (all zero = defaults; the library reads no
 * environment variables). */
typedef struct chub_options {
    int32_t slot_kernel;  /* PHILOX steps: 0 = the packed slot kernel wherever the hub shape allows (default),
                             1 = the wave-local slot kernel for every step, 2 = same as 0 (kept for tests that name it).
                             COMPAT resets / steps of handles beyond a handful of envs: 0 / 2 = the split form (the stream walks one ENV per
                             lane, then the slots of both stations in one launch, which also leaves the next step's count of empty slots),
                             1 = one kernel per station with the unit's first lane walking (bit-identical; the parity cross-check) */
    int32_t no_arena;     /* 1: one hipMalloc per array instead of one arena (disables chub_get_state / chub_set_state) */
    int32_t fused_step;   /* PHILOX lock-step steps as ONE launch (slot work + per-env tail + next step's draws per workgroup):
                             0 = for small batches, where the two step kernels are launch-bound (default: up to 768 slot workgroups; hubs of fewer than 8 piles
                             up to 384), 1 = never, 2 = always
                             (hub shapes the packed slot kernel covers, stations of at most 64 piles).  Results are bit-identical.
                             COMPAT handles whose envs all fit one workgroup (the drop-in class: one env) run reset and step as one
                             launch too -- station 0, station 1, tail back to back -- unless this is 1. */
    int32_t tile;         /* workgroup tile of the packed slot kernel: 0 = by working-set size (default; a hub of more than 512 piles takes the
                             second tile whatever its batch), 1 = 256 lanes x 2 slots (state and action rows live in the caches), 2 = 512 lanes
                             x 4 slots (they stream from HBM).  Results are bit-identical. */
    int32_t walk_ahead;   /* COMPAT split step: 0 = lock-step steps of every env walk the streams ahead of their step (default): stations of 8 to 64
                             piles run the slot pass of step i and the stream walks of step i + 1 in ONE launch (the walk two steps ahead of the
                             slots it draws for: it takes the slots that will be empty from the stays alone), other shapes the tails of step i
                             and those walks; the walk writes a shadow of the streams that the slot pass of step i + 1 commits, so a reset that
                             comes instead never sees it.  1 = never (every step walks its own streams first: the parity cross-check).
                             Results are bit-identical. */
    int32_t work_order;   /* PHILOX packed kernels, cache-resident sizes (the small tile, at most 6 M charger slots): 0 = tiles, tail and level workgroups
                             take their work in contiguous eighths per XCD (the dispatcher hands workgroup b to XCD b % 8) (default),
                             1 = the dispatcher's order (workgroup b takes tile b: the A/B and the parity cross-check).  Results are bit-identical. */
    int32_t span_steps;   /* chub_run_steps on a PHILOX handle that runs the one-launch step (fused_step): spans of lock-step steps as ONE launch
                             (k_steps_fused: each workgroup goes from step to step by itself, one workgroup barrier between steps; a span ends
                             at the day's end at the latest): 0 = as many steps as the call and the day allow (default), 1 = never (every step
                             a launch: the parity cross-check), n = at most n steps per launch.  Results are bit-identical.  Of a span's packed
                             outputs the last two blocks remain (the policy is open loop over the span: the call's own action batches).
                             On a PHILOX handle that runs the TWO-launch step on the small tile of the packed slot kernel (stations of at most 64 piles)
                             the same option bounds the steps per TAIL launch: chub_run_steps sends PAIRS of lock-step steps out as three launches --
                             slot(i), slot(i + 1), then the per-env tails of both steps in one launch (k_env_pair) -- instead of four: 0 = from 8192
                             envs on (default), 1 = never, 2 and more = at any size.  Pairs never straddle a day's end or the call's; an odd step out
                             goes by the per-step path.  Not with a communicator, on per-env clocks, on a tape handle, on a handle with per-env hub
                             parameters, under the profiler or with step terms, episode statistics or telemetry attached.  Bit-identical as well. */
    int32_t span_tails;   /* ... and where a span's per-env tails run: 0 = by size (default: up to 256 workgroups -- one per CU -- as 2, beyond as 1), 1 = on the
                             workgroup's last slot wave, behind its slot phases (k_steps_fused), 2 = on a fifth wave of the workgroup, ONE STEP BEHIND
                             the slot waves (k_steps_piped: the slot phases of step s + 1 read nothing the tails of step s write, so the two chains of a
                             step run side by side; hubs of 8 piles and more).  Results are bit-identical. */
} chub_options;

/* telemetry column indices of chub_get_telemetry (names of the reference attributes, MGR:183-297) */
enum {
    CHUB_T_HY_ACT = 0, CHUB_T_HY_FLOW_SPEED, CHUB_T_ALL_POWER_SECOND, CHUB_T_STORE_SOC, CHUB_T_CAPACITY,
    CHUB_T_TOTAL_MASS_NEED, CHUB_T_HY_USE, CHUB_T_NOT_MEET, CHUB_T_FC_POWER, CHUB_T_HY_TO_USE,
    CHUB_T_USED_RENEW, CHUB_T_EV0, CHUB_T_EV1, CHUB_T_HYDROGEN_POWER, CHUB_T_INCOME, CHUB_T_REWARD,
    CHUB_T_RE_PV, CHUB_T_RE_WD, CHUB_T_PRICE_NEXT, CHUB_T_HV_ARRIVE, CHUB_T_HV_LINE, CHUB_T_QUEUE_LEN,
    CHUB_T_PV_DAY, CHUB_T_WD_DAY,
    /* ev_power_list / ev_power_sum after the fuel-cell rescale -- what the incomes and cumulated_draw_ele use (MGR:219-224, 262) --
     * and real_state[1] as the step found it (MGR:234) */
    CHUB_T_EV0_NET, CHUB_T_EV1_NET, CHUB_T_EV_SUM_NET, CHUB_T_PRICE_NOW,
    /* per station what make_state puts into real_state (MGR:364-368) + flow_in_number[-1] (MGR:246); valid after reset too */
    CHUB_T_MIN0, CHUB_T_CHG0, CHUB_T_MAX0, CHUB_T_LINE0, CHUB_T_FLOW0, CHUB_T_MIN1, CHUB_T_CHG1, CHUB_T_MAX1, CHUB_T_LINE1, CHUB_T_FLOW1,
    CHUB_T_COUNT
};

/* ---- lifetime ------------------------------------------------------------------------------
 * Replaces: EvcsspManagerEnv_v6.__init__ (MGR:25-130) = Change_Use_Seed (main.cpp:21) + 2x
 * Fast/SlowChargeStation(int,bool,bool) (main.cpp:188,240; AGG:188-196) + HySystem/HFC/ReNew setup.
 * data_dir holds car_flow_possibility_list_save.csv (parsed with the reference's own float parser,
 * CHS.hpp:138-155) and price_96.f64 / pv_100x96.f64 / wd_150x96.f64.  env_id0 = global index of this
 * handle's first env (shard offset); device = HIP device ordinal.  No reset is performed. */
int chub_create(const chub_config *cfg, const char *data_dir, int64_t n_envs, int64_t env_id0, int device,
                uint64_t seed, int rng_mode, chub_env **out);
int chub_create_ex(const chub_config *cfg, const char *data_dir, int64_t n_envs, int64_t env_id0, int device,
                   uint64_t seed, int rng_mode, const chub_options *opt /* NULL = defaults */, chub_env **out);
int chub_destroy(chub_env *env);

/* ---- per-env hub parameters ----------------------------------------------------------------------------------------------
 * In the reference every EvcsspManagerEnv_v6 is its own object built from its own kwargs (MGR:25-27): a vector of them may mix
 * electrolysers, tanks, fuel cells, FCEV traffic and fluctuations (domain randomisation).  A handle made by chub_create_params
 * holds such a mix: station_list, station_type_list and constant_charging stay per handle (they set the slot layout), the eight
 * scalars below are per env.  Each row has the chub_config field of the same name and meaning; an env computes exactly what a
 * homogeneous handle built from a chub_config with its row computes (same seed, same global env id: bit for bit).
 *   chub_create_params: as chub_create_ex; cfg's eight scalars are ignored in favour of rows [N].  Every row is validated as
 *       chub_create validates its config (same codes and messages, with " (env i)" appended).  fcev_permeate > 1 counts as 0.01 per
 *       env, as in the reference.  The FCEV waiting list is sized for the largest arrival bound of any row.
 *   chub_set_env_params: overwrite the rows of the envs a host mask names (NULL = all; rows is [N], only the named rows are read).
 *       The new rows apply from the next launch on, including to a captured graph's next replay (the arrays do not move; a graph's
 *       first step draws its own state-independent variates, so no FCEV count drawn with the old rate is consumed).  The state
 *       of an env is not touched -- its tank keeps its content until a reset starts it at the new init_soc -- so the domain-
 *       randomisation pattern is chub_set_env_params(mask, rows) then chub_reset_envs(mask).  What survives that reset is what
 *       survives any reset (the OU states, MGR:304-316) and does not depend on the rows.  A row whose FCEV arrival bound exceeds the
 *       one the handle was created with is refused (CHUB_ERR_ARG): create with the largest fcev_permeate you will use.  COMPAT: the
 *       named envs' hy_power_speed_list becomes the zero-demand sweep of their new row; chub_compat_replay_constructor rebuilds it.
 *   chub_get_env_params: the rows, [N].  chub_has_env_params: 1 for a handle made by chub_create_params, else 0.
 *   chub_launch_plan_params: chub_launch_plan for such a handle (CHUB_PLAN_* values).
 * Modes and forms: all three RNG modes.  Steps run as two launches -- the slot kernel, then the tail k_env<.., ENV_PARAMS> -- lock-step
 * or masked: the options that pick the one-launch step and chub_run_steps's spans are accepted and have no effect (chub_uses_fused_step
 * returns 0, chub_run_steps issues its steps one by one).  COMPAT: the reference's sequence for N differently built envs is
 * chub_create_params -> chub_set_rng_compat_seeds -> chub_compat_replay_constructor (each env the constructor with its own kwargs and
 * streams; until then each env's table is the zero-demand sweep of its row) -> chub_reset.  Such a handle runs one COMPAT form at every
 * batch size: one kernel per station with the unit's first lane walking the streams, the tail drawing the forecourt (the split step's
 * walks and k_compat_small are not built for rows; chub_options.slot_kernel / walk_ahead have no effect).  Entry points not built for
 * per-env rows return CHUB_ERR_UNSUPPORTED with a message: the scalar-load control (chub_step_load*), tape mode
 * (chub_tape_register_soc, chub_step_tape*, chub_reset_tape*), chub_get_hy_table and chub_set_hy_table (one table for every env;
 * chub_get_hy_table_env gives env i's).  Snapshots carry the rows; one taken from a handle with rows is refused by a handle without
 * and the other way round. */
typedef struct chub_env_params {
    double hydro_prod_rate;
    double hydro_store_vlt;
    double init_soc;
    double fc_max_power;
    double fcev_permeate;
    double renew_fluctuate;
    double price_fluctuate;
    double hydro_loss;
} chub_env_params;
int chub_create_params(const chub_config *cfg, const char *data_dir, int64_t n_envs, int64_t env_id0, int device, uint64_t seed, int rng_mode,
                       const chub_options *opt /* NULL = defaults */, const chub_env_params *rows /* [N] */, chub_env **out);
int chub_set_env_params(chub_env *env, const uint8_t *mask /* host, NULL = all */, const chub_env_params *rows /* [N] */);
int chub_get_env_params(chub_env *env, chub_env_params *rows /* [N] */);
int chub_has_env_params(const chub_env *env);
int chub_launch_plan_params(const chub_config *cfg, int64_t n_envs, int rng_mode, const chub_options *opt /* NULL = defaults */, int32_t *out);
/* The pair rule of chub_run_steps (chub_options.span_steps on a handle on the two-launch step) for this hub shape, batch, RNG mode and options, without a device:
 * out[CHUB_PAIR_HANDLE] = 1 if a handle made this way runs pairs of steps with one tail launch at all, out[CHUB_PAIR_CALL] = 1 if a call in the
 * state `flags` describes does, out[CHUB_PAIR_STEPS] = how many of the next `left` steps then go out as pairs when the clock shows slot t of the day. */
enum { CHUB_PAIR_HANDLE = 0, CHUB_PAIR_CALL, CHUB_PAIR_STEPS, CHUB_PAIR_COUNT };
enum { CHUB_PAIRF_COMM = 1, CHUB_PAIRF_PER_ENV = 2, CHUB_PAIRF_TAPE = 4, CHUB_PAIRF_OUTPUTS = 8, CHUB_PAIRF_PROFILING = 16 };
int chub_pair_plan(const chub_config *cfg, int64_t n_envs, int rng_mode, const chub_options *opt /* NULL = defaults */, int env_params, uint32_t flags,
                   int t, int64_t left, int64_t *out);
int chub_uses_pair_tails(const chub_env *env); /* 1: chub_run_steps sends pairs of steps out with one tail launch (where the call allows) */

int chub_obs_dim(const chub_env *env);  /* 2 + 4*(#stations with piles>0) + 3 (MGR:74-104) */
int chub_act_dim(const chub_env *env);  /* S + 2 (MGR:108-113) */
int64_t chub_num_envs(const chub_env *env);
int chub_clock(const chub_env *env);    /* 0..95: the slot of day, shared by all envs while they run in lock-step (env 0's otherwise) */
int chub_uses_packed_kernel(const chub_env *env); /* 1: PHILOX steps of this handle run k_slot_packed (the production kernel) */
int chub_uses_fused_step(const chub_env *env);    /* 1: its lock-step steps run as one launch (k_step_tailwave / k_step_fused / k_compat_small, small batches) */
int chub_uses_xcd_order(const chub_env *env);     /* 1: its packed kernels' workgroups take their work in XCD-aware order (chub_options.work_order) */

/* The launch forms chub_create_ex would choose for this hub shape, batch, RNG mode and options, without a device: out[CHUB_PLAN_COUNT], one
 * value per CHUB_PLAN_* index.  Returns what chub_create_ex returns for arguments and combinations it refuses (same code, same message). */
int chub_launch_plan(const chub_config *cfg, int64_t n_envs, int rng_mode, const chub_options *opt /* NULL = defaults */, int32_t *out);
enum {
    CHUB_PLAN_PACKED = 0,     /* PHILOX steps on k_slot_packed: 0 no, 1 small tile, 2 small tile with stations of more than 64 piles, 3 large tile, 4 large tile
                                 with stations of more than 64 piles */
    CHUB_PLAN_BIG_TILE,       /* 1: the packed kernel's large tile */
    CHUB_PLAN_PBLOCK,         /* ... its workgroup size */
    CHUB_PLAN_PSLOTS,         /* ... and slots per lane */
    CHUB_PLAN_EPB,            /* whole envs per packed workgroup */
    CHUB_PLAN_XCD,            /* 1: XCD-aware work order (what the kernels read; chub_uses_xcd_order: not where the step is one launch) */
    CHUB_PLAN_ONE_LAUNCH,     /* lock-step steps as one launch: 0 no, 1 k_step_fused, 2 k_step_tailwave */
    CHUB_PLAN_SPAN_SIZE_OK,   /* 1: chub_run_steps's spans of steps in one launch are allowed by size */
    CHUB_PLAN_SPAN_PIPED,     /* ... as k_steps_piped (1) or k_steps_fused (0) */
    CHUB_PLAN_SPAN_STEPS,     /* chub_options.span_steps */
    CHUB_PLAN_COMPAT_SMALL,   /* 1: COMPAT lock-step resets and steps as one launch (k_compat_small) */
    CHUB_PLAN_COMPAT,         /* COMPAT's other resets and steps: 0 (PHILOX), 1 one kernel per station, 2 the split form, 3 the split form walking two steps
                                 ahead (k_slot_walk2, 32 envs per walk workgroup), 4 the same with 64 */
    CHUB_PLAN_SPLIT2,         /* 1: the split form's steps take two slots per lane (k_slot_split2) */
    CHUB_PLAN_WALK_AHEAD,     /* 1: lock-step split steps walk the next step's streams ahead (chub_options.walk_ahead) */
    CHUB_PLAN_STATION0,       /* station 0's slot kernel where the packed one is not used: 0 k_slot, 1 k_slot_unit, 2 k_slot_unit_any, 3 k_slot_curves */
    CHUB_PLAN_STATION1,
    CHUB_PLAN_COUNT
};

/* ---- hot path ------------------------------------------------------------------------------
 * chub_reset replaces EvcsspManagerEnv_v6.reset (MGR:304-316 -> AGG:157-175 evs_reset main.cpp:199,251,
 * HYD:197-208, REN:51-53).  chub_step replaces EvcsspManagerEnv_v6.step (MGR:136-302 -> AGG:116-155
 * evs_step(Vector_float) main.cpp:198,250; hv_car_number_wrt_poisson / mk_soc main.cpp:151,163).
 *   actions  [N,A] f32 in [-1,1]; pile bit = ((a+1)/2 >= 0.5) in f32; tail is swapped as in MGR:395-403.  Tail actions outside
 *            [-1,1] (NaN and infinities included) are the caller's error: the electrolyser's table index is clamped for memory safety only
 *   exo_days [N,2] i32 (pv_day, wd_day) -- required in COMPAT mode, ignored (may be NULL) in PHILOX
 *   exo_z    [N,3] f64 standard normals for the (pv, wd, price) OU updates (REN:71-76) -- COMPAT only
 *   obs      [N,D] f32, reward [N] f32, done [N] u8
 * Host-pointer forms copy in/out around the device-pointer forms. */
int chub_reset(chub_env *env, const int32_t *exo_days, const double *exo_z, float *obs);
int chub_step(chub_env *env, const float *actions, const double *exo_z, float *obs, float *reward, uint8_t *done);
/* The handle's pinned action buffer [N,A] f32: a host that writes its actions there and passes this pointer to chub_step
 * saves the CPU copy into pinned memory (any other host pointer works too). */
int chub_host_actions(chub_env *env, float **out);

/* Packed-action form of chub_step for hosts that sit behind PCIe: all that action_to_real (MGR:384-393) keeps of an action row is
 * one bit per pile ((a + 1) / 2 >= 0.5) and the two tail floats, so that is what travels: pile_bits [N, ceil(S / 64)] u64 (bit b of
 * word w = hub slot 64 w + b: station 0's piles first, as in an action row; 1 = on) and tail [N, 2] f32 = the last two entries
 * of the action row, unchanged.  16 bytes per env for hubs of up to 64 piles instead of 4 (S + 2).  Results are bit for bit those of
 * chub_step on any action rows with the same bits and tail.  chub_host_bits: the handle's pinned staging for both arrays (fill in
 * place and pass these pointers to save a staging copy).  The _device form takes device pointers on `stream`: on the packed slot
 * kernel (PHILOX handles; both launch forms, per-env clocks, recordable into graphs) the step reads the bits themselves -- 8 bytes
 * per env and word of action input instead of a row of floats, and the tail kernel takes the two tail actions from d_tail; on the
 * other kernels the bits are first expanded into action rows on the device. */
int chub_step_bits(chub_env *env, const uint64_t *pile_bits, const float *tail, const double *exo_z, float *obs, float *reward,
                   uint8_t *done);
int chub_host_bits(chub_env *env, uint64_t **pile_bits_out, float **tail_out);
int chub_step_bits_device(chub_env *env, const uint64_t *d_pile_bits, const float *d_tail, const double *d_exo_z, float *d_obs,
                          float *d_reward, uint8_t *d_done, void *stream);
/* ... with the outputs of chub_step_device_packed: one [N, D + 2] f32 block (obs, reward, done as 0 / 1) */
int chub_step_bits_device_packed(chub_env *env, const uint64_t *d_pile_bits, const float *d_tail, const double *d_exo_z, float *d_packed,
                                 void *stream);

/* Same, all pointers device memory, enqueued on `stream` (a hipStream_t, NULL = default stream);
 * returns after enqueueing.  This is the form the multi-GPU host and bench.py use. */
int chub_reset_device(chub_env *env, const int32_t *d_exo_days, const double *d_exo_z, float *d_obs, void *stream);
int chub_step_device(chub_env *env, const float *d_actions, const double *d_exo_z, float *d_obs, float *d_reward,
                     uint8_t *d_done, void *stream);

/* Per-env clocks.  Every reference env is its own object with its own clock: any one of them can be reset, or stepped,
 * while the others are not (MGR:137-140, 271-273, 299, 304-316).  These entry points take a host array mask[n_envs]
 * (non-zero = the env takes part) next to full-size [n_envs, ...] arrays of which only the rows of the named envs are
 * read and written (exo_days / exo_z as for chub_reset / chub_step: COMPAT handles only).  The first such call makes the clock two bytes of per-env device state; a call is
 * still ONE launch (one Philox tick) in which every env it names runs on its own clock, and lock-step use -- chub_reset /
 * chub_step on everybody -- costs what it did.  chub_reset of everybody brings all envs back onto one clock.
 * chub_env_clocks: slot of day of every env and (tick_out may be NULL) the Philox tick of its last launch;
 * chub_clock_groups: number of distinct clocks right now.  (Both read the device: they synchronise.) */
int chub_reset_envs(chub_env *env, const uint8_t *mask, const int32_t *exo_days, const double *exo_z, float *obs);
int chub_step_envs(chub_env *env, const uint8_t *mask, const float *actions, const double *exo_z, float *obs, float *reward,
                   uint8_t *done);
int chub_reset_envs_device(chub_env *env, const uint8_t *mask /* host */, const int32_t *d_exo_days, const double *d_exo_z, float *d_obs,
                           void *stream);
int chub_step_envs_device(chub_env *env, const uint8_t *mask /* host */, const float *d_actions, const double *d_exo_z, float *d_obs,
                          float *d_reward, uint8_t *d_done, void *stream);
int chub_env_clocks(chub_env *env, int32_t *t_out, uint32_t *tick_out);
int chub_clock_groups(chub_env *env);

/* Masks in device memory, and the step that resets whoever finished.  Which envs finished a step is known on the device only; a trainer
 * whose episodes are staggered (clones from an archive or another handle, chub_copy_envs_device) would otherwise read `done` back,
 * synchronise, build a host mask and call chub_reset_envs_device -- a device read and a stream wait per step.  On these entry points the
 * host never looks at a mask.
 *   chub_dmask_reset_envs_device / chub_dmask_step_envs_device: chub_reset_envs_device / chub_step_envs_device with d_mask [N] u8 in DEVICE
 *       memory (the caller's buffer, read by the launch in stream order).  The call returns after enqueueing: no synchronisation, no staging
 *       copy, no allocation.  It always takes exactly one Philox tick and always launches, over the whole range of envs; the handle goes onto
 *       per-env clocks as after a host-mask call and STAYS there -- a device mask that happens to name everybody cannot return it to lock-step
 *       (chub_reset of everybody still does) -- and the next launch makes its own state-independent draws, as after any call on a subset.
 *       For a mask that is neither empty nor full: state, outputs and ticks are bit for bit those of the host-mask call with the same mask.
 *       An all-zero mask changes no env state and writes no output row; it still consumes its tick.  All three RNG modes, with and without
 *       per-env parameter rows.  CHUB_ERR_UNSUPPORTED with a message: tape handles.  (Scalar-load and bits forms take host masks only.)
 *   chub_autoreset_step_device: every env takes one step on its own clock, and every env whose `done` fired in that step is then reset, in
 *       the same call on the same stream.  ALWAYS two ticks: T for the step, T + 1 for the reset launch, whether or not anybody was done (the
 *       streams then depend on nothing the host cannot know, and results stay independent of sharding).  Results: those of
 *       chub_step_device_packed of everybody followed by a masked reset with mask = that step's done.  d_packed [N, D + 2]: for a reset env
 *       the step's reward, done = 1 and the FIRST OBSERVATION OF THE NEW EPISODE; d_final_obs [N, D] (may be NULL) receives the terminal
 *       observation rows of the reset envs, rows of other envs are left alone.  Valid on a lock-step handle (it moves to per-env clocks
 *       first).  COMPAT: the step reads d_exo_z as chub_step_device does; the reset reads the rows of the reset envs of d_reset_exo_days
 *       [N, 2] / d_reset_exo_z [N, 3] (ignored, may be NULL, in the Philox modes).  While nobody is done the reset launch's workgroups
 *       return at entry: the handle counts the done envs on the device.
 *   Ticks: chub_env_clocks(.., tick_out) stays truthful -- the launches note on the device whom they served, and chub_env_clocks /
 *       chub_get_state (which synchronise anyway) fold that into the host's record; snapshots taken after such calls restore and continue
 *       bit-identically.
 *   Graphs: all three are recordable between chub_graph_begin and chub_graph_end under the rule that such a capture starts on per-env
 *       clocks.  A device mask is the caller's buffer and is re-read on every replay (no per-call copy); a captured auto-reset call is two
 *       launches (k calls: 2k, always even).  Such a graph may be replayed indefinitely whatever the envs' clocks are. */
int chub_dmask_reset_envs_device(chub_env *env, const uint8_t *d_mask, const int32_t *d_exo_days, const double *d_exo_z, float *d_obs,
                                 void *stream);
int chub_dmask_step_envs_device(chub_env *env, const uint8_t *d_mask, const float *d_actions, const double *d_exo_z, float *d_obs,
                                float *d_reward, uint8_t *d_done, void *stream);
int chub_autoreset_step_device(chub_env *env, const float *d_actions, const double *d_exo_z, const int32_t *d_reset_exo_days,
                               const double *d_reset_exo_z, float *d_packed /* [N, D + 2] */, float *d_final_obs /* [N, D], may be NULL */,
                               void *stream);

/* The launch forms ONE reset / step takes on a handle of this shape (chub_launch_plan's per-call half), without a device: flags describe the
 * call and the handle's state, out[CHUB_CALLPLAN_COUNT] receives the forms (values in the order of the enums of csrc/chub_plan.h: CallForm,
 * OneLaunch, SlotForm, LevelsForm, EnvForm).  env_params != 0: a handle made by chub_create_params. */
enum {
    CHUB_CALL_RESET = 1,       /* a reset (else a step) */
    CHUB_CALL_PER_ENV = 2,     /* the handle is on per-env clocks */
    CHUB_CALL_ALL_SERVED = 4,  /* the call serves every env (no mask) */
    CHUB_CALL_DEV_MASK = 8,    /* the mask is in device memory: the masked forms and per-env clocks whatever else is set */
    CHUB_CALL_FRESH = 16,      /* the launch makes its own state-independent draws */
    CHUB_CALL_BITS = 32,       /* one bit per pile (chub_step_bits*) */
    CHUB_CALL_LOAD = 64,       /* the scalar-load control */
    CHUB_CALL_CAPTURING = 128  /* between chub_graph_begin and chub_graph_end */
};
enum { CHUB_CALLPLAN_CALL = 0, CHUB_CALLPLAN_ONE, CHUB_CALLPLAN_SLOT, CHUB_CALLPLAN_LEVELS, CHUB_CALLPLAN_ENV, CHUB_CALLPLAN_COUNT };
int chub_call_plan(const chub_config *cfg, int64_t n_envs, int rng_mode, const chub_options *opt /* NULL = defaults */, int env_params,
                   uint32_t flags, int32_t *out);

/* Scalar-load control mode: replaces EvcsspManagerEnv-level use of Fast/SlowChargeStation.evs_step(float)
 * (CHS.hpp:1169-1186 / 1480-1497, bound at main.cpp:196-197,248-249): one kW target per station instead of one bit per
 * pile; the piles are switched on in urgency order until the (clamped) target is met.  Same array layout as chub_step,
 * with actions[i][0] = load of station 0 and actions[i][station_list[0]] = load of station 1 (kW, not normalised; the
 * other pile entries are ignored; a station without piles has no load entry); the two tail entries keep their meaning. */
int chub_step_load(chub_env *env, const float *actions, const double *exo_z, float *obs, float *reward, uint8_t *done);
int chub_step_load_device(chub_env *env, const float *d_actions, const double *d_exo_z, float *d_obs, float *d_reward,
                          uint8_t *d_done, void *stream);
/* ... and on a subset of the envs (mask as for chub_step_envs: every reference station takes evs_step(float) on its own) */
int chub_step_load_envs(chub_env *env, const uint8_t *mask, const float *actions, const double *exo_z, float *obs, float *reward,
                        uint8_t *done);
int chub_step_load_envs_device(chub_env *env, const uint8_t *mask /* host */, const float *d_actions, const double *d_exo_z, float *d_obs,
                               float *d_reward, uint8_t *d_done, void *stream);

/* Packed form for the multi-GPU gather: one [N, D+2] f32 buffer, row = obs[D], reward, done (0.0 / 1.0), so that
 * a shard's whole step output travels in a single RCCL gather. */
int chub_step_device_packed(chub_env *env, const float *d_actions, const double *d_exo_z, float *d_packed, void *stream);

/* Random policy on device: fills d_actions [N,A] with i.i.d. uniform(-1,1) f32 from Philox key
 * `key`, counter (j, 0, batch, global env id).  (test/env_test.py drives the reference with a fixed
 * policy; RL trainers supply their own.) */
int chub_random_actions_device(chub_env *env, uint64_t key, uint32_t batch, float *d_actions, void *stream);

int chub_sync(chub_env *env);

/* ---- multi-GPU: the one collective of the path -----------------------------------------------------------------
 * No counterpart in the reference (it has nothing distributed): environments are independent, so the
 * path shards by contiguous ranges of the global env index -- one process per GPU, handle i created with
 * env_id0 = i * n_local (the Philox streams are keyed by the GLOBAL env id, so results do not depend on the sharding) --
 * and per step each shard's packed output [n_local, D+2] f32 (chub_step_device_packed) travels to rank 0 in ONE grouped
 * ncclSend / ncclRecv over the direct xGMI links, enqueued on the same HIP stream as the step kernels: no host wait,
 * capturable in a hipGraph.  RCCL is loaded on first use (dlopen); a process that never makes a communicator never maps it.
 *   chub_comm_unique_id: rank 0 makes the 128-byte RCCL id; the host passes it to the other ranks (file, pipe, socket).
 *   chub_comm_create:    every rank, same id (ncclCommInitRank on `device`).
 *   chub_comm_gather:    every rank: `bytes` from d_send to rank 0's d_recv + rank * bytes (d_recv ignored elsewhere).  IN PLACE on rank 0:
 *                        with d_send == d_recv its own block already lies where it belongs and rank 0 neither sends to nor receives from
 *                        itself (on a world of one nothing is enqueued at all).
 *   chub_step_gather:    the multi-GPU step: chub_step_device_packed + chub_comm_gather of the packed block on one stream.  Rank 0's step
 *                        kernels write its block STRAIGHT INTO d_gathered (rows 0 .. n_local - 1: the in-place form above -- no copy of
 *                        the root's own block); d_packed is not touched on rank 0 and may be NULL there.  Every other rank steps into
 *                        d_packed and sends it; d_gathered is ignored there.
 *   chub_comm_max_f64 / chub_comm_barrier: max over ranks of one host double / rendezvous (both synchronise `stream`);
 *                        what bench.py brackets its timed region with.
 *   chub_comm_gather_timed: the same gather `reps` times back to back between two HIP events on `stream`: microseconds per gather
 *                        (the per-phase split bench.py prints at N > 1; every rank calls it; synchronises).
 *   chub_comm_world:     the communicator's size as RCCL reports it (ncclCommCount).
 *   chub_comm_ranks_seen: all-reduce sum of one 1 per rank: the number of processes RCCL actually moved data between.
 *   chub_device_info:    out[4] = PCI domain, bus, device of HIP device `device` and its compute-unit count (which physical GPU a
 *                        rank sits on; bench.py lists it per rank). */
typedef struct chub_comm chub_comm;
int chub_comm_unique_id(void *id128);
int chub_comm_create(const void *id128, int world, int rank, int device, chub_comm **out);
int chub_comm_destroy(chub_comm *comm);
int chub_comm_world(const chub_comm *comm);
int chub_comm_rank(const chub_comm *comm);
int chub_comm_gather(chub_comm *comm, const void *d_send, void *d_recv, int64_t bytes, void *stream);
int chub_comm_gather_timed(chub_comm *comm, const void *d_send, void *d_recv, int64_t bytes, void *stream, int reps, double *us_per_gather);
int chub_comm_max_f64(chub_comm *comm, double *value, void *stream);
int chub_comm_barrier(chub_comm *comm, void *stream);
int chub_comm_ranks_seen(chub_comm *comm, int *out, void *stream);
/* Overlapped gathers (off by default).  chub_comm_set_overlap(comm, 1): chub_comm_gather / chub_step_gather put the collective on a
 * stream of the communicator's own, behind an event of the caller's stream, and the caller's stream goes on at once: the gather of step
 * k runs beside the kernels of step k + 1.  Inside a hipGraph capture (chub_graph_begin .. chub_graph_end) the events are graph edges --
 * no host cost per replay; call by call they cost the host two event calls per step (measured slower than the serial form).
 *   chub_comm_gather_begin: before enqueueing work that overwrites a send buffer: `stream` waits for the gather that last read it.
 *                           Announcing a buffer here is what makes its gathers overlapped ones (two gathers may be out at a time: the packed
 *                           step output is double-buffered; chub_step_gather announces its block -- a third buffer waits, on `stream`, for
 *                           the older of the two; a buffer whose gather has been joined gives its slot up); chub_comm_gather of a buffer
 *                           nobody announced goes out on the caller's stream behind every gather still out
 *                           Join (chub_comm_join) BEFORE chub_graph_begin: a capture must not wait on an event recorded outside it.  The
 *                           overlapped form has run on a world of one only; it stays off by default (bench.py --overlap-gather) until a
 *                           run with more than one rank has verified it
 *   chub_comm_join:         `stream` waits for every gather still out: before the gathered blocks are consumed, before a host
 *                           synchronisation that is meant to cover them (chub_graph_end, chub_comm_max_f64 / barrier / ranks_seen /
 *                           gather_timed call it themselves) */
int chub_comm_set_overlap(chub_comm *comm, int enabled);
int chub_comm_gather_begin(chub_comm *comm, const void *d_send, void *stream);
int chub_comm_join(chub_comm *comm, void *stream);
int chub_device_info(int device, int32_t *out4);
int chub_step_gather(chub_env *env, chub_comm *comm, const float *d_actions, float *d_packed, float *d_gathered, void *stream);

/* A run of n_steps steps issued from C, starting at step index first_step: before every step whose index is a multiple of 96 a
 * chub_reset_device (into d_reset_obs), then chub_step_gather (comm != NULL; d_gathered2 may be NULL off rank 0) or
 * chub_step_device_packed, with actions d_action_batches[i % n_batches] and outputs d_packed2[i & 1] / d_gathered2[i & 1].  Exactly
 * the RESULTS of the calls a host loop would make (PHILOX handles); returns after enqueueing.  Without a communicator, on a handle that
 * runs the one-launch step (chub_uses_fused_step: small batches) and with at most 8 action batches, consecutive lock-step steps go out as
 * ONE launch per span (k_steps_piped / k_steps_fused; chub_options.span_steps, span_tails) -- a span ends where the call does, at a reset and where the handle's clock
 * wraps; only the span's last two packed blocks exist afterwards, as after the same steps issued one by one.  Not under the per-kernel
 * profiler, with telemetry on, with the episode ledger on (chub_set_episode_stats), with a tape loaded or on per-env clocks: every step is
 * then a launch of its own. */
int chub_run_steps(chub_env *env, chub_comm *comm, const float *const *d_action_batches, int n_batches, float *const *d_packed2,
                   float *const *d_gathered2, float *d_reset_obs, int64_t first_step, int64_t n_steps, void *stream);

/* Per-kernel timing of the step: between chub_profile_begin and chub_profile_end every `every`-th step (up to
 * max_steps samples) records HIP events on the launch stream around the slot kernel and the env kernel; _end
 * synchronises and returns the summed durations in milliseconds and the number of steps sampled. */
int chub_profile_begin(chub_env *env, int max_steps, int every);
int chub_profile_end(chub_env *env, double *slot_ms_sum, double *env_ms_sum, int *n_steps);

/* ---- introspection (parity tests, `re_*` telemetry, show_situation MGR:412-414) ---------------
 * chub_get_slots: per env, per station k, field-major [9][piles[k]]: car, charge, emergency, power, soc,
 *   init_soc, target_soc (Station::situation, CHS.hpp:204-231), stay_time, already_stay_time
 *   (CHS.hpp:245-246); out is [N][9*S] f32 with station 0's block first.  Empty slots report the pile
 *   defaults of the reference (-1 for the two counters).
 * chub_get_station_scalars: [N][2][8] f64 = min_power, charge_power, max_power, car_number, line,
 *   flow_in_number[-1], station_time_hole, transformer_limit (AGG:198-218, MGR:368).
 * chub_get_telemetry: [N][CHUB_T_COUNT] f64 of the last step.
 * chub_get_obs_f64 / chub_get_reward_f64: last observation / reward before the f32 narrowing. */
int chub_get_slots(chub_env *env, float *out);
int chub_get_station_scalars(chub_env *env, double *out);
int chub_get_telemetry(chub_env *env, double *out);
int chub_get_obs_f64(chub_env *env, double *out);
int chub_get_reward_f64(chub_env *env, double *out);
int chub_set_telemetry(chub_env *env, int enabled); /* off by default: the hot path then skips those stores */
/* Handles of a few envs (action rows of at most 16 KB in all: the drop-in class runs ONE env) keep the telemetry block in pinned host
 * memory that the device writes directly (no copy back): *telem [CHUB_T_COUNT][N] (column-
 * major: one row per CHUB_T_* index), *obs64 [N][D], *reward64 [N], all f64, owned by the handle, valid while telemetry stays on.
 * Larger handles keep the block in device memory (posted PCIe writes of 27 MB per step at 65 536 envs would stall the tail kernel):
 * CHUB_ERR_UNSUPPORTED here, chub_get_telemetry / chub_get_obs_f64 / chub_get_reward_f64 copy.
 * Contents are current once the call that produced them has completed (any host-pointer entry point returns completed; after a
 * device-pointer call: chub_sync / a stream synchronise).  This is how EvcsspManagerEnv_v6.step() reads everything the reference
 * class exposes after a step (MGR:183-297, 364-372) without one device read. */
int chub_telemetry_host(chub_env *env, double **telem, double **obs64, double **reward64);

/* ---- per-episode accounting on the device ---------------------------------------------------------------------------------------
 * The reference keeps a ledger per episode: cumulated_income and cumulated_draw_ele are zeroed in reset() (MGR:305-306) and added to in
 * every step() (MGR:259-262), acumulate_reward runs over the steps (MGR:269), deviation is the tank's distance from init_soc after every
 * step (MGR:297), and the step that ends the day derives test_penalty from it (MGR:275-290).  With the ledger on, the step's per-env tail
 * keeps the same columns per env in device memory -- in every launch form, in all three RNG modes, lock-step, masked or auto-reset:
 *   CHUB_EP_RETURN        += the step's reward in f64, before the f32 narrowing (CHUB_T_REWARD)                     0 at reset
 *   CHUB_EP_INCOME        += CHUB_T_INCOME                                                                         0 at reset
 *   CHUB_EP_DRAW_ELE      += (CHUB_T_EV0_NET + CHUB_T_EV1_NET) + CHUB_T_HYDROGEN_POWER (MGR:262)                   0 at reset
 *   CHUB_EP_LENGTH        += 1                                                                                     0 at reset
 *   CHUB_EP_DEVIATION     abs(Store_SOC - init_soc) of the last step (CHUB_T_STORE_SOC: stale after the fuel cell) 0 at reset
 *   CHUB_EP_TEST_PENALTY  abs(abs(Store_SOC - init_soc) * capacity_mass / 1000 / 0.2) of the last step             0 at reset
 *   CHUB_EP_END_SOC       Store_SOC of the last step                                                               the reset's SOC
 * (init_soc and capacity_mass are the env's own on a handle made by chub_create_params).  Two blocks and two per-env words:
 *   live      the columns above, "as if the episode ended now"; zeroed by whatever resets the env (chub_reset*, masked and device-mask
 *             resets, the reset half of chub_autoreset_step_device).  An env stepped on past `done` without a reset keeps accumulating, as
 *             the reference object does.  A masked call updates only the envs it serves.
 *   finished  a copy of the env's live columns taken in the step whose `done` fired; no reset touches it
 *   episodes  u32: how many such steps the env has seen
 *   pending   u8: set with the finished block, cleared only by a draining summary call
 * The additions are IEEE f64 in step order: the sums equal, bit for bit, what a host gets by adding the same handle's telemetry columns.
 *   chub_set_episode_stats: off by default -- a handle that never asks pays one uniform branch per tail.  Switching on allocates (outside the
 *       arena) and zeroes everything; counting starts with the next call.  CHUB_ERR_UNSUPPORTED on tape handles and between chub_graph_begin
 *       and chub_graph_end; it takes effect for a captured graph's next replay, as chub_set_telemetry does.  With the ledger on chub_run_steps
 *       issues its steps one by one (as with telemetry on); single one-launch steps keep their form.  While the ledger is on
 *       chub_tape_register_soc is CHUB_ERR_UNSUPPORTED too (switch it off first): no handle is a tape handle and keeps the ledger.
 *   chub_get_episode_stats: host memory, out [N][CHUB_EP_COUNT]; finished = 0 selects the live block, 1 the finished one.  Synchronises.
 *   chub_get_episode_counts: host memory, out [N].  Synchronises.
 *   chub_episode_stats_device: d_out [CHUB_EP_COUNT][N] (column-major, as stored), d_counts [N] or NULL: device-to-device copies enqueued on
 *       `stream`.  Recordable into a graph; no synchronisation.
 *   chub_episode_summary_device: over the envs whose pending flag is set, d_out [1 + 4 * CHUB_EP_COUNT] f64 in the caller's device memory:
 *       their count, then per column of the finished block sum, sum of squares, min, max (count 0: sums 0, min +inf, max -inf).  drain != 0
 *       clears the flags it read.  Two launches on `stream` (per-workgroup partials, then their sum in workgroup order): no atomics, every
 *       order fixed, so two calls on one state give identical bits.  Recordable into a graph; no synchronisation.  The partials live in ONE
 *       buffer owned by the handle (the host form uses it too): summary calls on one handle must be ordered against each other -- the same
 *       stream, or an event between them -- as they must be against the steps that write the ledger.  Two of them in flight on different
 *       streams race on that buffer.
 *   chub_episode_summary: the same into host memory.  Synchronises.
 * All of them but the first two return CHUB_ERR_ARG with a message while the ledger is off.  Snapshots carry the four arrays when the ledger
 * is on (chub_state_size grows by exactly their bytes); one taken with the ledger on is refused by a handle with it off and the other way
 * round, with nothing written.  chub_copy_envs* copies an env's live block, finished block, count and flag with the rest of its state; a copy
 * between a handle with the ledger on and one with it off is CHUB_ERR_ARG. */
enum {
    CHUB_EP_RETURN = 0, CHUB_EP_INCOME, CHUB_EP_DRAW_ELE, CHUB_EP_LENGTH, CHUB_EP_DEVIATION, CHUB_EP_TEST_PENALTY, CHUB_EP_END_SOC,
    CHUB_EP_COUNT
};
int chub_set_episode_stats(chub_env *env, int enabled);
int chub_has_episode_stats(const chub_env *env);
int chub_get_episode_stats(chub_env *env, int finished, double *out);
int chub_get_episode_counts(chub_env *env, uint32_t *out);
int chub_episode_stats_device(chub_env *env, int finished, double *d_out, uint32_t *d_counts, void *stream);
int chub_episode_summary_device(chub_env *env, double *d_out, int drain, void *stream);
int chub_episode_summary(chub_env *env, double *out, int drain);

/* ---- per-pile observations on the device -----------------------------------------------------------------------------------------
 * A policy sets one bit per pile, and the reference shows it every pile: Station::situation (CHS.hpp:204-231) holds car, charge, emergency,
 * power, soc, init_soc and target_soc per pile, the two stay counters sit beside it (CHS.hpp:245-246).  chub_get_slots reports these nine
 * fields through the host (it synchronises, allocates, runs this launch with every field and re-orders in a host loop: a parity
 * instrument); chub_pile_obs_device writes them as columns into the caller's device memory in ONE launch on `stream`, for a policy or a
 * heuristic that never leaves the device:
 *   fields  a bit mask over the CHUB_PILE_* enum (bit f = field f; the enum has chub_get_slots' nine fields in its order); C = its popcount
 *           columns come out, in ascending field order.  chub_pile_obs_columns gives C for a valid mask (it needs no device).
 *   d_out   [N][C][S] f32, S = piles[0] + piles[1]: env-major, then column, then HUB SLOT -- station 0's piles first, as in an action row
 *           (a station of 0 piles contributes no slots), so that a wave stores runs of consecutive floats.  NOT chub_get_slots' layout: that
 *           one is [N][station][9][piles[k]], per-station blocks.  Every value is, bit for bit, what chub_get_slots reports for that pile
 *           and field at the same moment, the defaults of an empty pile included (0, and -1 for the two counters).
 *   d_mask  [N] u8 in device memory or NULL: with a mask only the rows of the envs whose byte is non-zero are written, every other row of
 *           d_out is left alone (an all-zero mask writes nothing).
 * It reads simulation state and writes d_out, nothing else: no tick, no clock, no draw -- the handle computes what it would have computed
 * without the call.  It returns after enqueueing: no synchronisation, no allocation, no staging copy; order it against the calls that
 * write the state as any other call on the handle (the same stream, or an event).  Valid at any point after the first reset: after resets
 * and steps of every form (masked, device-mask, auto-reset: a re-started env shows its new episode's piles), chub_copy_envs* and
 * chub_set_state; on lock-step and per-env clocks, with or without per-env parameter rows, telemetry or the ledger; in all three RNG
 * modes and for every hub shape the handle can be created with.  Recordable between chub_graph_begin and chub_graph_end, where it does
 * not count towards the even number of resets + steps a graph must cover.
 * Cost follows the field set: the state word alone gives car and charge; power, emergency and init_soc add the pile's record (PHILOX: its
 * class row), the counters one byte, and the SoC -- which no mode stores -- is a read of a per-class table in PHILOX (derived data built on
 * the device when the handle is created: not snapshot state, chub_state_size is unchanged) and a replay of the car's steps along the
 * curve in COMPAT and PHILOX_CURVES, as in chub_get_slots.  A field that is not asked for costs none of this.
 * CHUB_ERR_ARG: null handle, null d_out, fields 0 or with bits from CHUB_PILE_COUNT up.  CHUB_ERR_UNSUPPORTED with a message: tape handles
 * (chub_tape_register_soc rewrites the class tables the columns are read from). */
enum {
    CHUB_PILE_CAR = 0, CHUB_PILE_CHARGE, CHUB_PILE_EMERGENCY, CHUB_PILE_POWER, CHUB_PILE_SOC, CHUB_PILE_INIT_SOC, CHUB_PILE_TARGET_SOC,
    CHUB_PILE_STAY_TIME, CHUB_PILE_ALREADY_STAY, CHUB_PILE_COUNT
};
int chub_pile_obs_columns(uint32_t fields);
int chub_pile_obs_device(chub_env *env, uint32_t fields, const uint8_t *d_mask, float *d_out, void *stream);

/* ---- per-station deadline profiles on the device -------------------------------------------------------------------------------------
 * A policy that sets a station's load (chub_step_load*) must know how much charging falls due by when: the station's cars binned by the
 * time they have left, with what they still need.  chub_station_profile_device writes that histogram for every env and both stations into
 * the caller's device memory in ONE launch on `stream`; its shape depends on (fields, buckets) alone, never on the hub, so one policy
 * serves hubs of 2 piles and of 8192.
 *   fields   a bit mask over the CHUB_SP_* enum (bit f = field f); C = its popcount columns come out, in ascending field order
 *   buckets  B, 1 .. 32.  With left = stay_time - already_stay_time as chub_get_slots reports it, a pile with a car falls into bucket
 *            min(left, B) - 1: B = 1 gives plain station totals, the last bucket collects every longer stay (a COMPAT stay may exceed 31)
 *   d_out    [N][2][C][B] f32: env, station, column, bucket.  chub_station_profile_size gives the floats per env, 2 * C * B, for valid
 *            arguments (it needs no device).  A station of 0 piles gives a block of zeros.
 *   d_mask   [N] u8 in device memory or NULL: with a mask only the blocks of the envs whose byte is non-zero are written.
 * Every value is defined on what chub_get_slots / chub_pile_obs_device report for the station's piles with car == 1 at the same moment,
 * over the cars of the bucket:
 *   CARS            number of cars                      CHARGING        cars with charge == 1
 *   MUST_CHARGE     cars with emergency == 10 (the step's must_charge predicate: judge_feasibility forces these on)
 *   POWER           sum of power, in units of 2^-19 kW  POWER_CHARGING  the same over the cars with charge == 1
 *   EMERGENCY       sum of emergency, units of 2^-20    SOC_GAP         sum of f32(target_soc - soc), units of 2^-16 %
 * The four sums are integer sums (the convention of the PHILOX station sums): each term is llrint((double) x * 2^q), round-half-even, the
 * terms are added as signed 64-bit integers and the result is (float) sum * 2^-q -- independent of lane order, workgroup shape and launch
 * form, so two calls on one state give identical bits.  Counts are exact.
 * Manners are chub_pile_obs_device's: it reads simulation state and writes d_out, nothing else (no tick, no clock, no draw); it returns
 * after enqueueing (no synchronisation, no allocation, no staging copy); valid at any point after the first reset, after resets and steps
 * of every form, chub_copy_envs* and chub_set_state, on lock-step and per-env clocks, with or without per-env parameter rows, telemetry
 * or the ledger, in all three RNG modes and for every hub shape; recordable between chub_graph_begin and chub_graph_end, where it does
 * not count towards the even number of resets + steps.  Cost follows the field set: CARS and CHARGING need the state word alone,
 * MUST_CHARGE, POWER* and EMERGENCY add the class row or hot record, SOC_GAP alone the SoC (a table read in PHILOX, a replay of the
 * car's steps in COMPAT and PHILOX_CURVES).
 * CHUB_ERR_ARG: null handle, null d_out, fields 0 or with bits from CHUB_SP_COUNT up, buckets outside 1 .. 32 (chub_station_profile_size
 * returns the same code).  CHUB_ERR_UNSUPPORTED with a message: tape handles, as for chub_pile_obs_device. */
enum {
    CHUB_SP_CARS = 0, CHUB_SP_CHARGING, CHUB_SP_MUST_CHARGE, CHUB_SP_POWER, CHUB_SP_POWER_CHARGING, CHUB_SP_EMERGENCY, CHUB_SP_SOC_GAP,
    CHUB_SP_COUNT
};
int chub_station_profile_size(uint32_t fields, int32_t buckets);
int chub_station_profile_device(chub_env *env, uint32_t fields, int32_t buckets, const uint8_t *d_mask, float *d_out, void *stream);

/* ---- exogenous look-ahead on the device: tariff, renewables, arrivals ------------------------------------------------------------------
 * The reference's observation carries the time of day only as sin(2 pi t / 96) (MGR:319-320: slots t and 48 - t look alike), and the
 * tariff, the PV / wind day profiles and the arrival law an energy-management policy plans against live inside the handle; on per-env
 * clocks the slot of day itself is device state.  chub_forecast_device writes, per env, the next H slots of what is DETERMINISTIC about the
 * exogenous world into the caller's device memory in ONE launch on `stream`:
 *   fields   a bit mask over the CHUB_FC_* enum (bit f = field f); C = its popcount columns come out, in ascending field order
 *   horizon  H, 1 .. 96
 *   d_out    [N][C][H] f32: env, column, look-ahead h.  chub_forecast_size gives the floats per env, C * H, for valid arguments (it needs
 *            no device).
 *   d_mask   [N] u8 in device memory or NULL: with a mask only the blocks of the envs whose byte is non-zero are written, every other block
 *            of d_out is left alone (an all-zero mask writes nothing).
 * Per env let t be its slot of day, 0 .. 95: the slot its next step simulates, what chub_env_clocks reports (lock-step: the handle's
 * clock); for h = 0 .. H - 1 let s = (t + h) % 96.  Every f64 expression is evaluated in f64 and narrowed once:
 *   SLOT       (float) s
 *   VALID      1 if t + h <= 95 (the slot lies inside the env's current day), else 0.  Beyond the day's end the other columns wrap with the
 *              env's CURRENT PV / wind days: the next reset draws new ones, which nobody knows yet
 *   SIN        (float) sin(2 pi s / 96) of the handle's table: at h = 0 the bits of observation column 0
 *   COS        the same table at (s + 24) % 96
 *   PRICE      (float) price[(s + 95) % 96]: the tariff part of real_state[1] as the step that simulates slot s finds it (make_state adds
 *              price[-1], the tariff of the slot before, MGR:354-359; after a reset that is price[95], AGG:171)
 *   PV         (float) (max(x, 0) * 5), x = the PV profile of the env's day at slot s: the noise-free part of re_pv_power (REN:38-43, MGR:349)
 *   WIND       (float) (max(x, 0) * 1), x = the wind profile of the env's day at slot s
 *   ARRIVALS0  (float) sum / 1000.0f, sum = the integer sum over the 1000 levels of uniform_rand of station 0's arrival count at slot s:
 *   ARRIVALS1  the mean of what the station's draw of slot s can come to, before balking -- reported whatever the station's pile count
 *   FCEV       the same over the FCEV arrival count the tail would read for THIS env: the handle's table, or with per-env rows
 *              clamp(roundf(rate of the env * arrival index), 0, 255); it follows chub_set_env_params from the next call on
 * The Ornstein-Uhlenbeck noise on PV, wind and price is deliberately NOT forecast (nor the env's price noise in PRICE): the observation
 * already shows the current slot's noisy values, so a policy has the noise as observation minus column h = 0.
 * Manners are chub_pile_obs_device's: it reads state and writes d_out, nothing else (no tick, no clock, no draw: the handle computes what
 * it would have computed without the call); it returns after enqueueing (no synchronisation, no allocation, no staging copy); valid at
 * any point after the first reset, after resets and steps of every form (masked, device-mask, auto-reset: a re-started env shows slot 0
 * and its new days), chub_copy_envs* and chub_set_state; on lock-step and per-env clocks, with or without per-env parameter rows,
 * telemetry or the ledger, in all three RNG modes (COMPAT's days are the caller's exo_days) and for every hub shape.  Recordable between
 * chub_graph_begin and chub_graph_end, where it does not count towards the even number of resets + steps: a lock-step handle's clock is
 * recorded by value (a graph replays only from the clock it started at), per-env clocks are read when the graph runs.
 * The mean counts are derived tables built on the host when the handle is created (per-env rows: a histogram of the arrival index per
 * slot, so that an env's FCEV mean is a sum of at most 301 terms): not snapshot state, chub_state_size is unchanged.
 * chub_forecast: the same through host memory, every env (it allocates, copies and synchronises: the convenience form).
 * CHUB_ERR_ARG: null handle, null d_out / out, fields 0 or with bits from CHUB_FC_COUNT up, horizon outside 1 .. 96 (chub_forecast_size
 * returns the same code).  CHUB_ERR_UNSUPPORTED with a message: tape handles (their arrivals are the caller's). */
enum {
    CHUB_FC_SLOT = 0, CHUB_FC_VALID, CHUB_FC_SIN, CHUB_FC_COS, CHUB_FC_PRICE, CHUB_FC_PV, CHUB_FC_WIND, CHUB_FC_ARRIVALS0, CHUB_FC_ARRIVALS1,
    CHUB_FC_FCEV, CHUB_FC_COUNT
};
int chub_forecast_size(uint32_t fields, int32_t horizon);
int chub_forecast_device(chub_env *env, uint32_t fields, int32_t horizon, const uint8_t *d_mask, float *d_out, void *stream);
int chub_forecast(chub_env *env, uint32_t fields, int32_t horizon, float *out);

/* ---- step terms on the device: reward parts, hydrogen side, constraint costs ----------------------------------------------------------
 * What the reward of a step is made of, and what a constrained learner penalises: the reference keeps them as attributes after every step
 * (re_income_*, re_hy_cost, hy_loss, not_meet_loss, cumulated_draw_ele's increment, the forecourt, the tank's distance from init_soc; its
 * own use_lagrangian / test_penalty block is MGR:275-297).  Every one of them is a function of the telemetry block the step's tail writes
 * in every launch form and RNG mode (CHUB_T_*), of init_soc and of capacity_mass; chub_get_step_terms_device evaluates that function for every
 * env in ONE read-only launch on `stream` and writes the columns asked for into the caller's device memory.
 * With T[x] = telemetry column CHUB_T_x of the env and p = T[PRICE_NOW] / 4, every expression evaluated in f64 in the order written
 * (no contraction; constants folded as the reference's Python folds them):
 *    0 REWARD         T[REWARD]                           (MGR:267)      14 FC_POWER       T[FC_POWER]
 *    1 INCOME         T[INCOME]                           (MGR:259)      15 HY_ACT         T[HY_ACT]
 *    2 INCOME_EVS0    0.42 / 4 * T[CHG0]      re_income_evs_list[0]      16 GEN_HY         T[HY_FLOW_SPEED] > 0.5 ? 1 : 0   (MGR:173-179)
 *    3 INCOME_EVS1    0.21 / 4 * T[CHG1]      re_income_evs_list[1]      17 HY_GEN         15 * 60 * T[HY_FLOW_SPEED]           re_hy_gen
 *    4 COST_EVS0      -p * T[EV0_NET]    re_income_evs_cost_list[0]      18 HY_USE         T[HY_USE]
 *    5 COST_EVS1      -p * T[EV1_NET]    re_income_evs_cost_list[1]      19 NOT_MEET       T[NOT_MEET]
 *    6 INCOME_SERVE   0.8 * (T[FLOW0] + T[FLOW1]) re_income_evs_serve    20 HY_FOR_FC      T[HY_TO_USE]                      re_hy_for_fc
 *    7 INCOME_HYS     6 / 1000 * T[HY_USE]            re_income_hys      21 MASS_NEED      T[TOTAL_MASS_NEED]
 *    8 HY_COST        -p * T[HYDROGEN_POWER]             re_hy_cost      22 FCEV_ARRIVE    T[HV_ARRIVE]
 *    9 HY_LOSS        -6 / 1000 * T[HY_TO_USE]            (MGR:225)      23 FCEV_LINE      T[HV_LINE]
 *   10 NOT_MEET_LOSS  -10 / 1000 * T[NOT_MEET]            (MGR:255)      24 FCEV_QUEUE     T[QUEUE_LEN]
 *   11 GRID_DRAW      (T[EV0_NET] + T[EV1_NET]) + T[HYDROGEN_POWER]      25 SOC_DEVIATION  fabs(T[STORE_SOC] - init_soc)        (MGR:297)
 *                     (MGR:262: the ledger's DRAW_ELE increment)         26 SOC_PENALTY    fabs(SOC_DEVIATION * capacity_mass / 1000 / 0.2)
 *   12 GRID_EXCESS    max(GRID_DRAW - 2000, 0)  (the 2000 kW of MGR:160)                   (MGR:277-290, "as if the day ended now")
 *   13 USED_RENEW     T[USED_RENEW]
 * init_soc and capacity_mass are the handle's; on a handle made by chub_create_params the env's own row, exactly as the ledger takes them.
 * So INCOME = (INCOME_HYS + ((INCOME_EVS0 + COST_EVS0) + (INCOME_EVS1 + COST_EVS1))) + INCOME_SERVE + HY_COST bit for bit (the tail's own
 * expression), that sum + HY_LOSS + NOT_MEET_LOSS over 50 is REWARD within 1 ulp, and (float) REWARD is the step's reward output.
 *   fields  a bit mask over the CHUB_ST_* enum (bit f = field f); C = its popcount columns come out, in ascending field order.
 *           chub_get_step_terms_size gives C for a valid mask (it needs no device), CHUB_ERR_ARG for 0 or bits from CHUB_ST_COUNT up.
 *   d_out   [N][C] f32, env-major; each value is the f64 expression narrowed once.
 *   d_mask  [N] u8 in device memory or NULL: with a mask only the rows of the envs whose byte is non-zero are written, every other row of
 *           d_out is left alone (an all-zero mask writes nothing).
 * Manners are chub_pile_obs_device's: it reads the telemetry block and writes d_out, nothing else (no tick, no clock, no draw); it returns
 * after enqueueing (no synchronisation, no allocation, no staging copy); recordable between chub_graph_begin and chub_graph_end, where it
 * does not count towards the even number of resets + steps.  It works wherever telemetry works: all three RNG modes, every hub shape,
 * per-env rows, tape handles, and both homes of the block (pinned host memory on handles of a few envs, device memory otherwise).
 * It reports the block AS IT STANDS.  A reset rewrites the station columns, STORE_SOC, the exogenous columns and the days of the envs it
 * restarts and leaves the rest: an env reset since its last step shows that step's hydrogen and money columns (REWARD, INCOME, COST_*,
 * HY_*, GRID_*, FCEV_*, ...) beside the NEW episode's INCOME_EVS0/1, INCOME_SERVE and SOC_*.  Before the first step the block is zero.
 *   chub_get_step_terms: the convenience form, every env, out [N][C] F64 in host memory: the expressions before narrowing, by the same kernel
 *       with an f64 store.  It allocates, copies and synchronises.
 *   chub_set_step_terms: attaches d_out [N][C] f32 (the caller's device memory, which must outlive the attachment).  From then on every STEP
 *       call of every form -- lock-step, host-masked, device-masked, bits, load, packed, gather, tape, chub_run_steps and the step half of
 *       chub_autoreset_step_device -- enqueues the launch on its own stream right behind the step's kernels, with that call's mask: only the
 *       rows of the envs the call served change.  Resets never write d_out.  In chub_autoreset_step_device the launch goes BETWEEN the step
 *       and the reset, so a restarted env's row holds its TERMINAL step's terms -- the end-of-day SOC_DEVIATION / SOC_PENALTY and station
 *       incomes the reset is about to overwrite in the block -- beside the new episode's first observation in d_packed.  Inside a capture
 *       the launch is one more node of the graph (not counted towards the even number of resets + steps).  fields == 0 or d_out == NULL
 *       detaches.  CHUB_ERR_ARG when telemetry is off or the mask is bad; CHUB_ERR_UNSUPPORTED between chub_graph_begin and chub_graph_end
 *       (a recorded step keeps the launch it was recorded with: a graph recorded while attached fills the buffer on every replay).  While
 *       an output is attached chub_set_telemetry(env, 0) is CHUB_ERR_ARG: detach first.  With nothing attached a step costs one null
 *       test on the host more than before.
 *   chub_get_step_terms_attached: the attached mask, or 0.
 * All of them: CHUB_ERR_ARG with a message for a null handle or null output, a bad mask, telemetry off. */
enum {
    CHUB_ST_REWARD = 0, CHUB_ST_INCOME, CHUB_ST_INCOME_EVS0, CHUB_ST_INCOME_EVS1, CHUB_ST_COST_EVS0, CHUB_ST_COST_EVS1, CHUB_ST_INCOME_SERVE,
    CHUB_ST_INCOME_HYS, CHUB_ST_HY_COST, CHUB_ST_HY_LOSS, CHUB_ST_NOT_MEET_LOSS, CHUB_ST_GRID_DRAW, CHUB_ST_GRID_EXCESS, CHUB_ST_USED_RENEW,
    CHUB_ST_FC_POWER, CHUB_ST_HY_ACT, CHUB_ST_GEN_HY, CHUB_ST_HY_GEN, CHUB_ST_HY_USE, CHUB_ST_NOT_MEET, CHUB_ST_HY_FOR_FC, CHUB_ST_MASS_NEED,
    CHUB_ST_FCEV_ARRIVE, CHUB_ST_FCEV_LINE, CHUB_ST_FCEV_QUEUE, CHUB_ST_SOC_DEVIATION, CHUB_ST_SOC_PENALTY, CHUB_ST_COUNT
};
int chub_get_step_terms_size(uint32_t fields);
int chub_get_step_terms_device(chub_env *env, uint32_t fields, const uint8_t *d_mask, float *d_out, void *stream);
int chub_get_step_terms(chub_env *env, uint32_t fields, double *out);
int chub_set_step_terms(chub_env *env, uint32_t fields, float *d_out);
int chub_get_step_terms_attached(const chub_env *env);

/* ---- station-level control on the device: kW targets to pile actions ------------------------------------------------------------------
 * The reference's station-level control, evs_step(float) (CHS.hpp:1169-1186 / 1480-1497: catch_load, assign_on_off, rank_power_add), takes
 * one kW target per station and switches the piles on in urgency order until the target is met.  chub_step_load* runs it inside the
 * wave-local step kernels (COMPAT and PHILOX, homogeneous handles, host masks).  chub_load_dispatch_device is the same dispatch as ONE
 * read-only launch on `stream` that turns the targets into what EVERY step form takes -- an action row, or one bit per pile -- so that a
 * policy which sets a station's load (its observations: chub_station_profile_device) runs in all three RNG modes, with per-env rows, under
 * device masks, through chub_autoreset_step_device, chub_step_bits_device* and the packed kernels, and inside graphs.
 *   units       CHUB_LOAD_KW: d_loads are kW.  CHUB_LOAD_FRACTION: d_loads are a in [-1, 1] like every other action; f = min(max((a + 1) / 2,
 *               0), 1) and the target is min_power + f * (max_power - min_power), every operation rounded to f32 (no FMA).
 *   d_loads     [N][2] f32: the target of station 0 and of station 1 (the entry of a station without piles is not read)
 *   d_tail      [N][2] f32: the two tail actions, copied into the rows (required with d_actions; not read otherwise)
 *   d_mask      [N] u8 in device memory or NULL: with a mask only the rows of the envs whose byte is non-zero are written
 *   d_actions   [N][A] f32 or NULL: pile entries exactly +1.0f (on) or -1.0f (off), then the two tail entries
 *   d_pile_bits [N][ceil(S / 64)] u64 or NULL: chub_step_bits' layout; bits from S up are zero.  Both outputs, if both are given, agree.
 * Definition, per env and station k with piles: car, emergency and power of every pile are what chub_pile_obs_device reports; mn and mx are
 * the f32 min_power and max_power of the unit's record (what chub_get_station_scalars shows).  The target is clamped as catch_load clamps
 * it (if load > mx: mx, else if load < mn: mn).  The piles are ordered by emergency descending, ties by slot index (the reference's
 * multimap keyed by -emergency); along that order the power of every pile with a car is added to ONE f32 running sum, sequentially
 * (rank_power_add).  A car is on iff (double) load + 0.0001 >= (double) the sum up to and including itself; with constant charging iff
 * fewer than roundf(load / constant_power) cars precede it.  In addition a car with emergency == 10 is on: judge_feasibility forces it on
 * when the row is stepped, and the outputs say what the step will do.  Stepping the row (chub_step_device*) or the bits
 * (chub_step_bits_device*) then computes, bit for bit, what chub_step_load_device computes from the same targets wherever no must-charge
 * car lies beyond the target (the scalar-load step leaves such a car off; a stepped row cannot).
 * Manners are chub_pile_obs_device's: it reads simulation state and writes its outputs, nothing else (no tick, no clock, no draw); it
 * returns after enqueueing (no synchronisation, no allocation, no staging copy); valid at any point after the first reset, after resets
 * and steps of every form, on lock-step and per-env clocks, with or without per-env parameter rows, telemetry or the ledger, in all three
 * RNG modes and for every hub shape (stations of 0 to 4096 piles); recordable between chub_graph_begin and chub_graph_end, where it does
 * not count towards the even number of resets + steps.
 * chub_load_dispatch: the same through host memory, every env (it allocates, copies and synchronises: the convenience form).
 * CHUB_ERR_ARG: null handle, null loads, both outputs null, d_actions without d_tail, unknown units.  CHUB_ERR_UNSUPPORTED with a message:
 * tape handles, as for chub_pile_obs_device. */
enum { CHUB_LOAD_KW = 0, CHUB_LOAD_FRACTION = 1 };
int chub_load_dispatch_device(chub_env *env, int units, const float *d_loads /* [N,2] */, const float *d_tail /* [N,2] */,
                              const uint8_t *d_mask /* [N] or NULL */, float *d_actions /* [N,A] or NULL */,
                              uint64_t *d_pile_bits /* [N,W] or NULL */, void *stream);
int chub_load_dispatch(chub_env *env, int units, const float *loads, const float *tail, float *actions, uint64_t *pile_bits);

/* ---- an actor on the device: closed-loop rollouts with no host ------------------------------------------------------------------------
 * Everything that surrounds a policy runs on the device (the step in every form, observations, profiles, forecasts, the dispatch); this
 * section adds the policy itself, for the common case of a feed-forward actor: the env's feature row, through 1 .. 4 dense layers, to the
 * action row or the pile bits the step already takes, as ONE launch on the caller's stream -- and chub_policy_run_steps, the closed loop
 * issued from C, which a captured graph can hold.
 *   Feature row: the spec's 1 .. 4 input blocks, concatenated in the order given into F floats per env:
 *       CHUB_PIN_OBS             D floats: the env's observation row, supplied by the caller (d_obs) or by the run loop
 *       CHUB_PIN_PILE_OBS        fields = a CHUB_PILE_* mask: C * S floats, chub_pile_obs_device's row of the env
 *       CHUB_PIN_STATION_PROFILE fields = a CHUB_SP_* mask, param = buckets: chub_station_profile_size floats
 *       CHUB_PIN_FORECAST        fields = a CHUB_FC_* mask, param = horizon: chub_forecast_size floats
 *     With normalize = 1 every feature becomes x <- min(max((x - mean[f]) * inv_std[f], -clip), clip), the subtraction and the product each
 *     rounded to f32 (no FMA).
 *   Layers: h <- act(W[l] h + b[l]), W[l] [width[l]][inputs of layer l] row-major (the nn.Linear layout), hidden widths 1 .. 256, hidden_act
 *     CHUB_PACT_TANH or CHUB_PACT_RELU on every layer but the last.  The last layer's width is fixed by the head, its outputs z are squashed to
 *     a = tanhf(z) (CHUB_PSQ_TANH) or a = min(max(z, -1), 1) (CHUB_PSQ_CLIP):
 *       CHUB_PHEAD_PILES  A = S + 2 outputs: an action row.  Outputs: d_actions [N, A] f32 and / or d_pile_bits [N, ceil(S / 64)] u64 with
 *                         d_tail [N, 2] f32 -- chub_step_bits_device's layout, bits from S up zero.  Pile bit b is a[b] >= -2^-25 on the squashed
 *                         f32 value: the step kernels' own predicate ((a + 1) / 2 >= 0.5 in f32), not the sign of z.  Stepping the bits and
 *                         stepping the row therefore give the same state bit for bit.
 *       CHUB_PHEAD_LOADS  4 outputs (load0, load1, tail0, tail1): the two loads go through chub_load_dispatch_device as CHUB_LOAD_FRACTION,
 *                         which writes d_actions and / or d_pile_bits; d_tail (if given) receives the tail pair.
 *   Numerics contract.  Every product is rounded once and accumulated in f32, as an fmaf chain (gfx950's v_mfma_f32_32x32x2_f32: f32 in, f32
 *     accumulate); no wider and no narrower arithmetic is used.  The bias is the chain's initial value.  The order of a layer's terms is
 *     unspecified but fixed: two calls on the same inputs give identical bits, whatever N, the mask or an env's place in the batch.  tanh is the
 *     device library's tanhf.  So an evaluated policy is the trainer's f32 network up to summation order.
 *   chub_policy_input_width: F and the head's output count for a hub shape and a spec, or the code and message chub_policy_create would give
 *       for them.  It needs no device.
 *   chub_policy_create: W[l] / b[l] host f32 as above (n_layers of each), mean / inv_std [F] host f32 (read when normalize = 1, else may be
 *       NULL).  Everything is validated before any allocation.  The weights are copied to the device in the kernel's own layout; scratch for the
 *       non-OBS blocks, the load / tail buffers and the run loop's action buffers are allocated here, all OUTSIDE the arena:
 *       chub_state_size and snapshots are unchanged.  A policy is bound to its handle; chub_destroy destroys the handle's policies first.
 *   chub_policy_set_weights: new W / b of one layer from host memory (it synchronises).  chub_policy_set_weights_device: the same from device
 *       memory in the trainer's layout, as a re-layout launch on `stream` (no synchronisation; recordable).  The buffers the policy kernel reads
 *       never move, so a captured graph's next replay evaluates the new weights.
 *   chub_policy_act_device: d_obs [N] rows of at least D floats with row stride ld_obs floats (a packed [N, D + 2] block: ld_obs = D + 2; not
 *       read, may be NULL, without a CHUB_PIN_OBS block).  The call enqueues the feature launches of the spec's non-OBS blocks into the policy's
 *       scratch, with the same mask, then ONE policy launch, then (CHUB_PHEAD_LOADS) chub_load_dispatch_device.  With d_mask [N] u8 (device
 *       memory) only the rows of the named envs are written.  Manners are chub_pile_obs_device's: no tick, no clock, no draw; no
 *       synchronisation, allocation or staging copy; recordable between chub_graph_begin and chub_graph_end without counting towards the even
 *       number of resets + steps; valid in all three RNG modes, on lock-step and per-env clocks, with per-env rows.  A policy's scratch is one
 *       buffer: calls on one policy must be ordered against each other (the same stream, or an event).
 *   chub_policy_act: the convenience form through host memory, every env: obs [N, D] -> actions [N, A].  Allocates, copies, synchronises.
 *   chub_policy_run_steps: the closed loop issued from C, steps first_step .. first_step + n_steps - 1; returns after enqueueing.  Results are
 *       exactly those of the same calls made one by one; inside a capture the whole run is recorded, under the step calls' own rules.
 *       CHUB_PRUN_LOCKSTEP: before every step whose index is a multiple of 96 a chub_reset_device into d_reset_obs [N, D]; then per step i
 *           chub_policy_act_device on the newest observation -- d_reset_obs right after a reset, else d_packed2[(i - 1) & 1] (so a run that
 *           starts mid-day continues from the block its predecessor left) -- into the policy's own bits and tail, and
 *           chub_step_bits_device_packed into d_packed2[i & 1] [N, D + 2].  16 bytes of action per env and word instead of a float row.
 *       CHUB_PRUN_AUTORESET: per step chub_policy_act_device into the policy's own action rows and chub_autoreset_step_device into
 *           d_packed2[i & 1] (d_final_obs [N, D] may be NULL).  The handle must have been reset.  The call's first step reads d_reset_obs [N, D]
 *           (the observation the caller holds) if it is given, else d_packed2[(first_step - 1) & 1]; every later step the packed block before it.
 *       Philox modes only: COMPAT needs the caller's normals per step (CHUB_ERR_UNSUPPORTED).
 * Refusals, all with a message and before any device work.  CHUB_ERR_ARG: null arguments; n_inputs or n_layers outside 1 .. 4; an unknown
 * kind, activation, head or squash; a feature block's own bad arguments (that call's message); widths outside
 * 1 .. 256; a last width that is not the head's; clip <= 0 (or NaN) with normalize; a policy used with a handle it was not made for; no
 * output asked for, or d_pile_bits without d_tail.  CHUB_ERR_UNSUPPORTED: chub_policy_create, chub_policy_destroy and the host form of
 * set_weights between chub_graph_begin and chub_graph_end; a non-OBS block or the LOADS head on a tape handle (as the feature calls); a
 * feature row and hidden layers that do not fit the kernel's 64 KiB of LDS (F rounded up to 2 and the widest odd hidden layer, plus the
 * widest even hidden layer, each rounded up to 32: at most 512 rows together -- F <= 256 always fits).
 * Out of scope: a critic IN the loop (values of all recorded observations are one batched call afterwards: "a critic on the device",
 * below), bf16 / f16 weights, recurrent or convolutional actors, the multi-GPU hosts, COMPAT in chub_policy_run_steps. */
enum { CHUB_PIN_OBS = 0, CHUB_PIN_PILE_OBS, CHUB_PIN_STATION_PROFILE, CHUB_PIN_FORECAST, CHUB_PIN_COUNT };
enum { CHUB_PACT_TANH = 0, CHUB_PACT_RELU, CHUB_PACT_COUNT };
enum { CHUB_PHEAD_PILES = 0, CHUB_PHEAD_LOADS, CHUB_PHEAD_COUNT };
enum { CHUB_PSQ_TANH = 0, CHUB_PSQ_CLIP, CHUB_PSQ_COUNT };
enum { CHUB_PRUN_LOCKSTEP = 0, CHUB_PRUN_AUTORESET, CHUB_PRUN_COUNT };
typedef struct chub_policy chub_policy;
typedef struct chub_policy_input { int32_t kind, fields, param; } chub_policy_input;
typedef struct chub_policy_spec {
    int32_t n_inputs;             /* 1 .. 4 blocks, concatenated in this order into one feature row of F floats */
    chub_policy_input inputs[4];
    int32_t n_layers;             /* 1 .. 4 dense layers, the last one the output layer */
    int32_t width[4];             /* width[l] = outputs of layer l, hidden widths 1 .. 256; width[n_layers - 1] is fixed by head */
    int32_t hidden_act;           /* CHUB_PACT_* */
    int32_t head;                 /* CHUB_PHEAD_* */
    int32_t squash;               /* CHUB_PSQ_* */
    int32_t normalize;            /* 0 / 1 */
    float clip;
} chub_policy_spec;
int chub_policy_input_width(const chub_config *cfg, const chub_policy_spec *spec, int32_t *F_out, int32_t *A_out);
int chub_policy_create(chub_env *env, const chub_policy_spec *spec, const float *const *W, const float *const *b, const float *mean,
                       const float *inv_std, chub_policy **out);
int chub_policy_destroy(chub_policy *pol);
int chub_policy_set_weights(chub_policy *pol, int32_t layer, const float *W, const float *b);
int chub_policy_set_weights_device(chub_policy *pol, int32_t layer, const float *d_W, const float *d_b, void *stream);
int chub_policy_act_device(chub_env *env, chub_policy *pol, const float *d_obs, int64_t ld_obs, const uint8_t *d_mask, float *d_actions,
                           uint64_t *d_pile_bits, float *d_tail, void *stream);
int chub_policy_act(chub_env *env, chub_policy *pol, const float *obs, float *actions);
int chub_policy_run_steps(chub_env *env, chub_policy *pol, int mode, float *const *d_packed2, float *d_reset_obs, float *d_final_obs,
                          int64_t first_step, int64_t n_steps, void *stream);

/* ---- sampling from the device actor: exploration noise, log-probabilities, rollouts that keep the trajectory --------------------------
 * The actor above is deterministic and chub_policy_run_steps keeps nothing.  This section makes on-policy training data in the same
 * launches: the action is DRAWN from the actor's distribution inside the actor launch, its log-probability is written beside it, and
 * chub_policy_collect keeps every step's block, action and log-probability where the trainer reads them.  Nothing of a policy's spec
 * changes: a policy made by chub_policy_create samples once chub_policy_set_exploration has given it a key and a scale.
 *   The distribution.  z = the last layer's pre-squash outputs, computed exactly as the deterministic actor computes them (same chain, same
 *     bits).  G = the number of Gaussian outputs:
 *       CHUB_PHEAD_PILES  outputs 0 .. S-1 are pile LOGITS, outputs S, S+1 the means of the two tail actions: G = 2
 *       CHUB_PHEAD_LOADS  all four outputs (load0, load1, tail0, tail1) are Gaussian means: G = 4
 *     Noise is Philox4x32-10 under the POLICY's key (a uint64 split as the env's seed is), counter (block, 15 << 16 | kind, tick, global env
 *     id): site 15 is no step's.  tick is the Philox tick of the handle's NEXT launch (chub_next_tick: host arithmetic, no device read),
 *     formed in the kernel as the steps form theirs, so a captured graph's next replay draws new noise as its steps do.  The noise does not
 *     depend on N, the mask, an env's place in the batch or sharding (env_id0).  Sampling consumes no tick: two sampled calls with no reset
 *     or step between them give IDENTICAL bits.
 *       pile b (kind 0): w = word b & 3 of block b >> 2; U = (float) (w >> 8) * 2^-24 (exact); p = 1 / (1 + expf(-z_b)) in f32; on iff U < p
 *       Gaussian i (kind 1): eps_i = the handle's tabulated normal (the OU draws' function and tables) of word i of block 0;
 *           u_i = z_i + sigma_i * eps_i, sigma_i = expf(log_std_i), the product and the sum each rounded to f32 (no FMA); action = squash(u_i)
 *     Log-probability, one f32 per env:
 *       logp = sum_b (on_b ? -softplus(-z_b) : -softplus(z_b)) + sum_i (-0.5 eps_i^2 - log_std_i - 0.5 ln 2 pi)
 *     with softplus(x) = max(x, 0) + log1pf(expf(-|x|)).  The Gaussian part is the density of the PRE-squash u: no tanh Jacobian is applied,
 *     since it is a function of u alone and cancels in every importance ratio.  The order of the sum is unspecified but fixed for a policy (no
 *     atomics).  Every pile counts, whether it holds a car or not (counting only occupied piles: not done).
 *     Outputs: action rows get pile entries exactly +1.0f / -1.0f (what the dispatch writes) and the squashed tail; pile bits are zero from bit
 *     S up; CHUB_PHEAD_LOADS sends the squashed loads through chub_load_dispatch_device as fractions, as the deterministic call does.
 *   chub_next_tick: the Philox tick of the handle's next reset or step, i.e. the tick a sampled call made now draws under.
 *   chub_policy_set_exploration: key and log_std [G] from host memory (it copies and synchronises).  The buffer is the policy's, allocated once
 *       outside the arena: snapshots are unchanged.  chub_policy_set_log_std_device: a copy on `stream` into that buffer: recordable, and a
 *       captured graph's next replay samples with the new scale, as with chub_policy_set_weights_device.
 *       The sampled launch needs 4 rows of LDS behind the deterministic launch's two images: a policy whose images leave fewer than 4 of the 512
 *       rows is refused HERE with CHUB_ERR_UNSUPPORTED (the deterministic fit rule is unchanged, and such a policy still evaluates).
 *   chub_policy_sample_device: the manners of chub_policy_act_device -- the same feature launches, the same mask semantics (only the named envs'
 *       rows of EVERY output are written), no tick consumed, no clock, no synchronisation, no allocation; recordable without counting towards a
 *       graph's even number of resets + steps.  d_logp is required, every other output optional (d_tail is required with d_pile_bits under
 *       CHUB_PHEAD_PILES).  d_u [N, G] are the pre-squash samples, d_features [N, F] the RAW feature row (before normalisation): what the
 *       trainer feeds its own network to reproduce z.
 *   chub_policy_collect: a host loop of the calls below, like chub_policy_run_steps; returns after enqueueing; Philox modes only.  The actor
 *       at step t reads d_obs0 [N, D] (ld = D) for t = 0 and block t - 1 of d_packed (ld = D + 2) afterwards: no copy.
 *       CHUB_PRUN_LOCKSTEP: first_step % 96 + T <= 96.  If first_step % 96 == 0 it begins with chub_reset_device into d_obs0.  Per step
 *           chub_policy_sample_device straight into the rollout's d_pile_bits[t], d_tail[t], d_u[t], d_logp[t], d_features[t], then
 *           chub_step_bits_device_packed from those into d_packed[t].
 *       CHUB_PRUN_AUTORESET: T <= 96 (an env finishes at most once, so each row of d_final_obs is written at most once); the handle must have
 *           been reset.  Per step the sample goes into the policy's own action rows AND the rollout's bits, tail, u, logp and features, then
 *           chub_autoreset_step_device into d_packed[t] with d_final_obs.
 * Refusals, with a message and before any device work.  CHUB_ERR_ARG: null env, policy, out, d_logp, d_obs0 or required rollout arrays; T <= 0;
 * the day and T rules above; a policy of another handle; sampling before chub_policy_set_exploration; a log_std that is not finite; the
 * observation rules of chub_policy_act_device.  CHUB_ERR_UNSUPPORTED: chub_policy_set_exploration between chub_graph_begin and
 * chub_graph_end; the LDS rule above; COMPAT in chub_policy_collect; the tape rules of chub_policy_act_device. */
int chub_next_tick(const chub_env *env, uint32_t *out);
int chub_policy_set_exploration(chub_policy *pol, uint64_t key, const float *log_std /* host [G] */);
int chub_policy_set_log_std_device(chub_policy *pol, const float *d_log_std /* [G] */, void *stream);
typedef struct chub_policy_sample_out {
    float *d_actions;       /* [N][A] or NULL */
    uint64_t *d_pile_bits;  /* [N][W] or NULL */
    float *d_tail;          /* [N][2]: squashed tail pair; required with d_pile_bits */
    float *d_u;             /* [N][G] or NULL: the pre-squash Gaussian samples */
    float *d_logp;          /* [N], required */
    float *d_features;      /* [N][F] or NULL: the RAW feature row, before normalisation */
} chub_policy_sample_out;
int chub_policy_sample_device(chub_env *env, chub_policy *pol, const float *d_obs, int64_t ld_obs, const uint8_t *d_mask,
                              const chub_policy_sample_out *out, void *stream);
typedef struct chub_rollout {
    int64_t T;
    float *d_packed;        /* [T][N][D + 2]: block t = the packed output of step t */
    uint64_t *d_pile_bits;  /* [T][N][W] */
    float *d_tail;          /* [T][N][2] */
    float *d_u;             /* [T][N][G] */
    float *d_logp;          /* [T][N] */
    float *d_features;      /* [T][N][F] or NULL */
    float *d_final_obs;     /* [N][D] or NULL (AUTORESET only) */
} chub_rollout;
int chub_policy_collect(chub_env *env, chub_policy *pol, int mode, const chub_rollout *r, float *d_obs0 /* [N][D] */,
                        int64_t first_step, void *stream);

/* ---- pile sets and advantages: log-probabilities over the piles a step can see, GAE over a collected rollout ---------------------------
 * The step ignores a pile's action bit wherever the reference's judge_feasibility overrides it (CHS:1404-1413): a pile with no car at the
 * start of the step is forced off, a pile whose car has emergency >= 1.01 is forced on, and a car that arrives during the step is not
 * touched by that step's action.  The sampled actor above nevertheless counts all S Bernoulli terms.  This section names the piles that
 * matter, lets the sampled launch count only those, and turns a collected rollout into advantages without leaving the device.
 *   chub_pile_set_device: d_bits [N][W] u64 in chub_step_bits' layout, W = ceil(S / 64), bits from S up zero.  Bit b of env e:
 *       CHUB_PSET_ALL        b < S
 *       CHUB_PSET_OCCUPIED   chub_pile_obs_device's car column of the pile is non-zero
 *       CHUB_PSET_DECIDABLE  occupied, and its emergency column is < 1.01f: the reference's predicate, on the values the columns hold
 *     Manners are chub_pile_obs_device's: ONE launch on `stream`, read-only on simulation state (no tick, no clock, no draw), no
 *     synchronisation, no allocation; with d_mask [N] u8 only the rows of the named envs are written; all three RNG modes and slot layouts,
 *     every hub shape (a station of 0 piles, stations of 4096); valid wherever chub_pile_obs_device is; recordable between chub_graph_begin
 *     and chub_graph_end without counting towards the even number of resets + steps.  OCCUPIED reads the state word alone, DECIDABLE adds
 *     the pile's record (PHILOX: its class row).  A step whose bits differ only outside DECIDABLE computes the same state and outputs.
 *   chub_policy_sample_set_device: chub_policy_sample_device with a set.  It enqueues chub_pile_set_device in front, with the same mask, into
 *     d_set_bits [N][W] (NULL: a buffer of the policy's own), then the sampled actor launch with the set as one more input.  Every draw and
 *     d_pile_bits, d_actions, d_tail, d_u and d_features are bit for bit what chub_policy_sample_device writes; only d_logp differs: a
 *     pile's Bernoulli term is added iff its bit is in the set, in the same fixed order with the other terms left out.  The Gaussian terms
 *     always count.  With CHUB_PSET_ALL d_logp too is chub_policy_sample_device's.  Under CHUB_PHEAD_LOADS the log-probability has no pile
 *     terms: only CHUB_PSET_ALL is accepted.
 *   chub_policy_collect_set: chub_policy_collect with the set launch and the set-aware sample per step; d_set_bits [T][N][W] (required),
 *     block t = the set in the state step t acts on.  The same day, T and mode rules; Philox modes only.
 *   chub_rollout_gae_device: generalised advantage estimation over a rollout's blocks, one launch (two with d_stats) on `stream`.  Per env,
 *     for t = T-1 .. 0, in f32 with every operation rounded once and no contraction, gl = gamma * lambda formed once in f32:
 *       d      = packed[t][D + 1] != 0
 *       vn     = d ? (d_final_values ? d_final_values[e] : 0) : V[t + 1]
 *       delta  = (packed[t][D] + gamma * vn) - V[t]
 *       adv[t] = delta + gl * (d ? 0 : adv[t + 1]),  adv[T] = 0
 *       ret[t] = adv[t] + V[t]
 *     V[0] = V(d_obs0) and V[t + 1] = V(the observation in block t): on an auto-reset rollout the observation in block t of a finished env is
 *     already the next episode's (the right V[t + 1] for step t + 1), and the terminal one is in d_final_obs, whose value d_final_values
 *     carries (NULL: an episode's end is worth 0).  With d_mask only the named envs' columns of d_adv / d_ret are written and counted.
 *     d_stats [3] f64: count, sum and sum of squares of the advantages written, reduced without atomics in an order fixed for (N, T): two
 *     calls give identical bits.  The partials live in one buffer of the handle's: calls that ask for d_stats must be ordered against
 *     each other.  `env` supplies N and D only: no simulation state is read, no tick, no synchronisation, no allocation; recordable.
 * Refusals, with a message and before any device work.  CHUB_ERR_ARG: null env, d_bits, g, d_packed, d_values or d_adv; null d_set_bits in
 * chub_policy_collect_set; an unknown `which`; which != CHUB_PSET_ALL under CHUB_PHEAD_LOADS; T <= 0; gamma or lambda outside [0, 1] or
 * NaN; everything chub_policy_sample_device and chub_policy_collect refuse.  CHUB_ERR_UNSUPPORTED: tape handles, as for
 * chub_pile_obs_device.  Out of scope: a critic inside these calls (d_values comes from "a critic on the device", below, or from the trainer). */
enum { CHUB_PSET_ALL = 0, CHUB_PSET_OCCUPIED, CHUB_PSET_DECIDABLE, CHUB_PSET_COUNT };
int chub_pile_set_device(chub_env *env, int which, const uint8_t *d_mask, uint64_t *d_bits /* [N][W] */, void *stream);
int chub_policy_sample_set_device(chub_env *env, chub_policy *pol, const float *d_obs, int64_t ld_obs, const uint8_t *d_mask, int which,
                                  uint64_t *d_set_bits /* [N][W] out, or NULL: the policy's own scratch */,
                                  const chub_policy_sample_out *out, void *stream);
int chub_policy_collect_set(chub_env *env, chub_policy *pol, int mode, int which, const chub_rollout *r,
                            uint64_t *d_set_bits /* [T][N][W], required */, float *d_obs0, int64_t first_step, void *stream);
typedef struct chub_gae {
    int64_t T;
    const float *d_packed;        /* [T][N][D + 2]: reward at column D, done at D + 1 (a rollout's d_packed) */
    const float *d_values;        /* [T + 1][N]: V[0] = V(d_obs0), V[t + 1] = V(the observation in block t) */
    const float *d_final_values;  /* [N] or NULL: V(d_final_obs), read only where done fires (bootstrap through the day's end) */
    const uint8_t *d_mask;        /* [N] or NULL */
    float gamma, lambda;
    float *d_adv, *d_ret;         /* [T][N] each; d_ret may be NULL */
    double *d_stats;              /* [3] or NULL: count, sum and sum of squares of the advantages written */
} chub_gae;
int chub_rollout_gae_device(chub_env *env, const chub_gae *g, void *stream);

/* ---- running feature statistics: a normaliser that follows the rollouts ----------------------------------------------------------------
 * The actor's input normalisation x <- clip((x - mean[f]) * inv_std[f]) is given at chub_policy_create.  A trainer that keeps running
 * observation statistics (stable-baselines' VecNormalize / RunningMeanStd) needs them computed where the rollout lies, and needs to hand them
 * to the policy without destroying it.  This section adds both: a moments object that accumulates count, mean and M2 per feature on the
 * device, and setters / a getter of a policy's normaliser, one of which derives it from the moments -- all in-stream and recordable.
 *   The state.  [1 + 2F] f64 in device memory: n | mean[F] | M2[F] (M2 = the sum of squared deviations from the mean: the population
 *     variance is M2 / n).  Zeros after create; it never moves.  State and partials are allocated at create, OUTSIDE the arena: chub_state_size
 *     and snapshots are unchanged; chub_moments_get / chub_moments_set are how a checkpoint carries the state.  The object is bound to its
 *     handle; chub_destroy destroys a handle's moments objects first, as it does its policies.
 *   chub_moments_update_device: R rows of F floats with row stride ld >= F floats -- a rollout's d_features (R = T N, ld = F), or the
 *     observations inside d_packed (F = D, ld = D + 2).  With d_mask [N] u8 in device memory row r belongs to env r % N (R a multiple of N) and
 *     only the rows of envs with a non-zero byte count; the rows of other envs are not read.  Manners are chub_rollout_gae_device's: no
 *     simulation state read, no tick, no synchronisation, no allocation; recordable between chub_graph_begin and chub_graph_end without
 *     counting towards the even number of resets + steps.  The partials are one buffer of the object's: calls on one object must be ordered
 *     against each other (the same stream, or an event).
 *   Definition, per feature f, all in f64, every operation rounded once:
 *       K     = n > 0 ? mean[f] : (double) x[0][f]       the pivot; row 0 serves whether it is masked or not
 *       d     = (double) x - K
 *       n_b   = the counted rows,  S1 = sum d,  S2 = sum d d  over them
 *       M2_b  = max(S2 - S1 S1 / n_b, 0)
 *       n'    = n + n_b
 *       n > 0:   mean' = K + S1 / n',   M2' = (M2 + M2_b) + (S1 / n_b)^2 (n n_b / n')          (Chan et al.)
 *       n == 0:  mean' = K + S1 / n_b,  M2' = M2_b
 *     n_b == 0 leaves the state untouched: an all-zero mask writes nothing.  Non-finite inputs give a non-finite state; nothing is checked on
 *     the device.  The pivot makes a constant column come out with M2 == 0 exactly and removes the cancellation of a raw sum of squares.  The
 *     order of the sums is unspecified but fixed for (R, F, ld, N) on one device: two calls on the same data and state give identical bits.  No
 *     atomics.  Two launches: the rows' sums per workgroup (the grid is chosen once at create from F and the device's compute units, so the
 *     rows a workgroup takes depend on (R, F) only), then the partials' sum and the merge.
 *   chub_moments_reset_device: the state back to zeros, as a memset on `stream`; recordable.
 *   chub_moments_get / chub_moments_set: the state to / from host memory (count, mean [F], m2 [F]); both synchronise; identical bits round trip.
 *   chub_moments_state_device: the address of the state, for a trainer that reads it in its own kernels.
 *   The policy's normaliser.  All four calls need a policy created with normalize = 1 (a normalize = 0 policy keeps its null pointers, and the
 *     kernel's argument block does not change).  chub_policy_set_normalizer: mean / inv_std [F] from host memory (it synchronises).  The device
 *     forms are copies, or one tiny launch, on `stream` into / out of the policy's own buffer: recordable, no synchronisation.  The buffers
 *     the policy kernel reads never move, so a captured graph's next replay evaluates the new normaliser.  chub_policy_get_normalizer_device
 *     copies out, [F] each: what the trainer needs to reproduce z from a rollout's raw d_features.
 *     chub_policy_normalizer_from_moments_device: in one launch mean32[f] = (float) mean[f] and
 *     inv_std32[f] = (float) (1.0 / sqrt(M2[f] / n + eps)): the population variance, as RunningMeanStd uses; IEEE f64 division and square root,
 *     every operation rounded once.  n == 0 leaves the normaliser as it is, decided on the device with no host read.
 * Refusals, all with a message and before any device work.  CHUB_ERR_ARG: null arguments; F outside 1 .. 512; ld < F; R <= 0; a mask with
 * R % N != 0; chub_moments_set with count < 0 or not finite; a normaliser call on a normalize = 0 policy; from_moments with objects of
 * different F or different handles, or eps not finite and > 0.  CHUB_ERR_UNSUPPORTED: chub_moments_create / destroy / get / set and
 * chub_policy_set_normalizer between chub_graph_begin and chub_graph_end.
 * Out of scope: accumulating inside the sampled actor launch, reward / return scaling, the multi-GPU hosts (an all-reduce of [1 + 2F]
 * doubles is the trainer's), anything in the snapshot. */
typedef struct chub_moments chub_moments;
int chub_moments_create(chub_env *env, int32_t F, chub_moments **out);   /* 1 <= F <= 512 */
int chub_moments_destroy(chub_moments *m);
int chub_moments_update_device(chub_moments *m, const float *d_x, int64_t ld, int64_t R, const uint8_t *d_mask /* [N] or NULL */, void *stream);
int chub_moments_reset_device(chub_moments *m, void *stream);
int chub_moments_get(chub_moments *m, double *count, double *mean /* [F] */, double *m2 /* [F] */);  /* synchronises */
int chub_moments_set(chub_moments *m, double count, const double *mean, const double *m2);           /* synchronises */
int chub_moments_state_device(chub_moments *m, const double **d_state);  /* [1 + 2F] f64: n | mean[F] | M2[F] */
int chub_policy_set_normalizer(chub_policy *pol, const float *mean, const float *inv_std);               /* host; synchronises */
int chub_policy_set_normalizer_device(chub_policy *pol, const float *d_mean, const float *d_inv_std, void *stream);
int chub_policy_get_normalizer_device(chub_policy *pol, float *d_mean, float *d_inv_std, void *stream);  /* copies out, [F] each */
int chub_policy_normalizer_from_moments_device(chub_policy *pol, chub_moments *m, double eps, void *stream);

/* ---- a population of actors: perturb, act, run, ES gradient ---------------------------------------------------------------------------
 * Evolution strategies, population-based training and plain evaluation of many candidate policies need no backward pass: they need P sets
 * of weights evaluated on P blocks of envs.  A chub_population holds P members, each with its own weights, and evaluates all of them in the
 * same single actor launch per step; its members are perturbed on the device from a centre with counter-based noise that is never stored,
 * and utilities per member are turned into the ES gradient estimate by regenerating that noise.
 *   Objects.  A population is bound to a chub_policy, "the centre": the policy's spec, normaliser, scratch, bits / tail / rows buffers and
 *     handle are the population's.  The policy's own weights are never touched by a population call.  chub_population_create: P even,
 *     2 <= P; N = P E with E a multiple of 32, so that a workgroup's tile of 32 envs belongs to exactly one member.  Member m serves envs
 *     [m E, (m + 1) E).  At create every member equals the centre's current weights.  The members' weights live in the kernel's own device
 *     layout, allocated once OUTSIDE the arena together with a staging block of the same size (chub_population_copy_members_device) and the
 *     partial sums of the gradient; they never move.  chub_state_size and snapshots are unchanged.  chub_policy_destroy / chub_destroy
 *     destroy a policy's populations first.  chub_population_param_count: host-only, no device: the sum over layers of out * (in + 1).
 *   The noise, a pure function of (key, generation, pair, layer, row, column).  Layer l is the augmented matrix [W | b] with columns
 *     k = 0 .. in (column `in` is the bias).  eps(g, j, l, row, k) is the handle's tabulated normal (normal_from_word: the OU draws'
 *     function and tables) applied to word k & 3 of the Philox4x32-10 block with counter
 *         (row << 8 | (k >> 2), 16 << 16 | l, g, j)
 *     under the population's key, a uint64 split as the policy's key is (low word first).  in <= 512 and row <= 8193 keep the fields apart.
 *     Nothing of P, N or the hub enters the noise.
 *   The pairing.  Members 2j and 2j + 1 are an antithetic pair: with d = sigma * eps rounded once to f32, member 2j gets theta + d and
 *     member 2j + 1 gets theta - d, each rounded once, no FMA.
 *   Manners of the device calls: on the caller's stream, no synchronisation, no allocation, no tick; recordable between chub_graph_begin
 *     and chub_graph_end without counting towards the even number of resets + steps.
 *   chub_population_perturb_device: theta in the trainer's layout (d_W[l] [out][in] row-major, d_b[l] [out], device memory); both arrays
 *     NULL: the centre policy's current weights.  One launch per layer writes every member's layer straight into the device layout (the
 *     re-layout fused with the draw); everything beyond `in` and `out` in the padded layout stays zero.  sigma and generation are HOST
 *     arguments: a captured graph replays the SAME generation and sigma -- record one graph per generation, or perturb between replays.
 *   chub_population_set_member_device / get_member_device: one member's layer from / to the trainer's [out][in] / [out] layout, one launch.
 *     chub_population_set_member / get_member: the same through host memory; they copy and synchronise.
 *   chub_population_copy_members_device: member dst[i] becomes a copy of member src[i], i = 0 .. count - 1 with count <= P, in ONE launch: the
 *     weight-side companion of chub_copy_envs_device.  ALL sources are read before any destination is written, so overlapping sets are
 *     welcome: src = {0, 1}, dst = {1, 0} swaps the two.  The indices are device memory and cannot be checked by the host: a pair with an
 *     index outside 0 .. P - 1 is skipped; of two pairs that name one destination the later wins.  Members not named are untouched.
 *   chub_population_act_device: arguments, feature launches, mask semantics, refusals and the LOADS dispatch are chub_policy_act_device's.
 *     CONTRACT: the outputs of member m's envs are bit for bit what chub_policy_act_device writes for a policy holding member m's
 *     weights: the chain, the order and the squash are the same.
 *   chub_population_run_steps: chub_policy_run_steps with the population's actor: both modes, Philox modes only, the same rules.
 *   chub_population_es_gradient_device: per parameter
 *         g[l][row][k] = sum over pairs j of ((double) util[2j] - (double) util[2j + 1]) * (double) eps(generation, j, l, row, k)
 *     accumulated in f64 (product and sum each rounded once) in an order fixed for (P, spec), rounded once to f32 and written in the
 *     trainer's layout (d_gW[l] [out][in], d_gb[l] [out]).  No atomics: two calls give identical bits.  The noise is regenerated, not read;
 *     sigma and 1 / (P sigma) are the trainer's to apply.  Two launches per layer; the pairs' partial sums live in one buffer of the
 *     population's: calls on one population must be ordered against each other.  d_util [P] f32 in device memory.
 * Refusals, all with a message and before any device work.  CHUB_ERR_ARG: null arguments; P odd or < 2; N != P E or E no multiple of 32;
 *     a population of another handle or policy; m or layer out of range; count < 0 or > P; sigma not finite or < 0; only one of d_W / d_b
 *     NULL; everything chub_policy_act_device / chub_policy_run_steps refuse.  CHUB_ERR_UNSUPPORTED: create, destroy and the host forms
 *     between chub_graph_begin and chub_graph_end; COMPAT in run_steps; the tape rules of chub_policy_act_device.
 * Out of scope: sampling from a population (the sampled launches stay single-policy), per-member normalisers, non-antithetic noise, rank
 *     shaping (fitness is chub_episode_stats_device's return column viewed as [P][E]; its reduction and ranking are the trainer's), the
 *     multi-GPU hosts. */
typedef struct chub_population chub_population;
int chub_population_param_count(const chub_config *cfg, const chub_policy_spec *spec, int64_t *n_out);
int chub_population_create(chub_policy *pol, int32_t P, uint64_t key, chub_population **out);
int chub_population_destroy(chub_population *pop);
int chub_population_perturb_device(chub_population *pop, const float *const *d_W, const float *const *d_b, float sigma, uint32_t generation,
                                   void *stream);
int chub_population_set_member_device(chub_population *pop, int32_t m, int32_t layer, const float *d_W, const float *d_b, void *stream);
int chub_population_get_member_device(chub_population *pop, int32_t m, int32_t layer, float *d_W, float *d_b, void *stream);
int chub_population_set_member(chub_population *pop, int32_t m, int32_t layer, const float *W, const float *b);  /* host; synchronises */
int chub_population_get_member(chub_population *pop, int32_t m, int32_t layer, float *W, float *b);              /* host; synchronises */
int chub_population_copy_members_device(chub_population *pop, const int32_t *d_src, const int32_t *d_dst, int32_t count, void *stream);
int chub_population_act_device(chub_env *env, chub_population *pop, const float *d_obs, int64_t ld_obs, const uint8_t *d_mask, float *d_actions,
                               uint64_t *d_pile_bits, float *d_tail, void *stream);
int chub_population_run_steps(chub_env *env, chub_population *pop, int mode, float *const *d_packed2, float *d_reset_obs, float *d_final_obs,
                              int64_t first_step, int64_t n_steps, void *stream);
int chub_population_es_gradient_device(chub_population *pop, const float *d_util /* [P] */, uint32_t generation, float *const *d_gW,
                                       float *const *d_gb, void *stream);

/* ---- actor gradients on the device: log-probabilities, PPO-clip loss, backward pass ----------------------------------------------------
 * The step of a policy-gradient update that used to leave the library: the CURRENT policy's log-probability of recorded actions and the
 * gradient of a surrogate loss with respect to the actor's weights and log_std, through the actor's own chain.  A chub_policy_grad is
 * bound to a chub_policy (its spec, live weights, normaliser and log_std); chub_policy_collect_set + chub_rollout_gae_device leave
 * everything a call reads in device memory.
 *   Rows.  A call works on R rows; a row is one (step, env) pair: R = T N over a rollout's [T][N][...] arrays taken flat.  d_rows [R]
 *     int64 (NULL: rows 0 .. R - 1) indexes EVERY per-row array; the arrays hold n_rows rows, and an index outside 0 .. n_rows - 1 (device
 *     memory: the host cannot check it) is skipped: it adds to nothing, stats[0] does not count it, its logp_new / entropy are 0.  A
 *     repeated index counts as often as it is named.  Per row: d_features [.][F] the RAW feature row with row stride ld_features >= F;
 *     d_pile_bits [.][W] (PILES); d_set_bits [.][W] or NULL for every pile (NULL under LOADS); d_u [.][G]; d_logp_old [.]; d_adv [.].
 *   Forward.  x = clamp((feature - mean) * inv_std) with the policy's CURRENT normaliser exactly as the actor does (f32 subtraction, f32
 *     product, clamp); the layers under the actor's numerics contract (every product rounded once, f32 accumulation from the bias in
 *     ascending input order, the device library's tanhf): the pre-squash outputs z are the bits the actor's own launch forms.
 *   logp_r: over the piles b of the set  -softplus(on_b ? -z_b : z_b)  with on_b the recorded bit, plus over the Gaussian outputs
 *     -0.5 eps_i^2 - log_std_i - 0.5 ln 2 pi  with eps_i = (u_i - z_i) / expf(log_std_i) in f32.
 *   H_r: over the same piles  softplus(z_b) - z_b sigmoid(z_b),  plus over the Gaussian outputs  0.5 + log_std_i + 0.5 ln 2 pi.
 *   Advantage.  A_r = adv_r; with d_adv_stats [3] f64 (count, sum, sum of squares: chub_rollout_gae_device's d_stats)
 *     A_r = (adv_r - m32) * s32, m = sum / count, s = 1 / sqrt(max(sumsq / count - m m, 0) + 1e-8), every f64 operation rounded once, m and
 *     s each rounded once to f32, the subtraction and the product each rounded once.
 *   Loss.  CHUB_PLOSS_COEF:      L = (1 / R) sum_r (-A_r logp_r - ent_coef H_r); d_logp_old is not read (it may be NULL).
 *          CHUB_PLOSS_PPO_CLIP:  ratio_r = expf(logp_r - logp_old_r),
 *                                L = (1 / R) sum_r (-min(ratio A, clamp(ratio, 1 - eps, 1 + eps) A) - ent_coef H_r);
 *              the row's policy term has a gradient iff (A >= 0 and ratio < 1 + eps) or (A < 0 and ratio > 1 - eps) (1 -+ eps rounded to
 *              f32), and there R dL/dlogp_r = -A ratio; elsewhere 0.  A ratio exactly on a bound is not defined beyond this predicate.
 *   Gradients.  dlogp/dz_b = on_b - sigmoid(z_b) and dH/dz_b = -z_b sigmoid(z_b) (1 - sigmoid(z_b)) for piles of the set, 0 for the others;
 *     dlogp/dz_i = eps_i / expf(log_std_i); dlogp/dlog_std_i = eps_i^2 - 1; dH/dlog_std_i = 1.  Hidden layers: tanh passes delta (1 - h^2),
 *     relu delta [h > 0].  The normaliser is a constant.  The factor 1 / R is applied ONCE, to the summed gradient, in f64 (below).
 *   Outputs, each optional: d_gW[l] [out][in] and d_gb[l] [out] in the TRAINER's layout (chub_policy_set_weights_device's), d_glog_std [G];
 *     d_logp_new [R] and d_entropy [R], written at position r of the call (not at d_rows[r]); d_stats [6] f64: rows counted, sum of the
 *     rows' loss terms, sum of entropies, sum of (logp_old - logp_new), rows whose policy term was clipped away, sum of ratios (the last
 *     three are 0 under COEF).  With every gradient output NULL the call is the forward alone ("evaluate actions"): no backward launch.
 *   Numerics of the gradient.  Products are rounded once and accumulated in f32 on the f32-input MFMA over the rows a workgroup walks
 *     (32 rows per chain link, a workgroup's tiles in ascending order); the workgroups' partial sums are added in f64 in workgroup order,
 *     divided by R in f64 and rounded once to f32.  The log_std sums and the stats are f64 from the row up.  No atomics: two calls on
 *     the same inputs give identical bits, and the order is a function of (R, spec) alone.
 *   Launches of one call, on the caller's stream: a small launch that rebuilds zero-padded row-major copies of layers 1.. from the
 *     policy's LIVE device weights (they cannot go stale after chub_policy_set_weights_device, or inside a graph), the gradient launch,
 *     the merge.  No allocation, no synchronisation, no tick; recordable.  The copies and the partials belong to the object: calls on
 *     one object must be ordered against each other.
 *   chub_policy_grad_plan: host-only, no device: the parameter count (sum of out * (in + 1)), the workgroups of a call of R rows
 *     (ceil(R / 32) rounded up to 8, at most 512, fewer where the partials would pass 256 MiB), the LDS rows and bytes, whether the
 *     dW tiles stay in registers (at most 16 tiles of 32 x 32 over all layers) and the workspace create allocates for max_rows = R --
 *     or the refusal create would give.  The fit rule: LDS rows = F rounded up to 32 + every hidden width rounded up to 32 + twice the
 *     widest layer output rounded up to 32 + 16, each row 33 floats (one of padding), at most 160 KiB.  13 -> 64 -> 64 -> 47 takes 304
 *     rows, 64 -> 256 -> 256 -> 47 takes 1104 -- by THIS rule; a gradient object also needs chub_policy_set_exploration, whose own rule
 *     (the policy's two images and 4 more rows within 512) refuses 64 -> 256 -> 256: for that actor the plan succeeds and no object
 *     can be made.  64 -> 256 -> 224 -> 47 (1072 rows) is the widest of that shape that samples.  A policy that does not fit still acts
 *     and samples.
 *   chub_policy_grad_create allocates outside the arena: chub_state_size and snapshots are unchanged.  chub_policy_destroy / chub_destroy
 *     destroy a policy's grad objects first.
 * Refusals, all with a message and before any device work.  CHUB_ERR_ARG: null g / in / out, null d_features, d_u, d_adv, d_pile_bits
 *     (PILES) or d_logp_old (PPO_CLIP); R <= 0, R > max_rows, n_rows < 1, ld_features < F; an unknown loss; eps outside (0, 1) under
 *     PPO_CLIP; ent_coef not finite; d_set_bits under LOADS; a policy without chub_policy_set_exploration (no log_std); max_rows < 1.
 *     CHUB_ERR_UNSUPPORTED: the fit rule; create / destroy between chub_graph_begin and chub_graph_end.
 * Out of scope: the value loss (the critic trains on `ret` through "a critic on the device", below: chub_critic_grad_device), an
 *     optimiser (see "an optimiser on the device", below: chub_adam_step_device), gradients with respect to the normaliser or through the tanh squash, bf16 weights,
 *     populations, the multi-GPU hosts (an all-reduce of the returned gradients is the trainer's), COMPAT rollouts. */
enum { CHUB_PLOSS_COEF = 0, CHUB_PLOSS_PPO_CLIP, CHUB_PLOSS_COUNT };
typedef struct chub_policy_grad chub_policy_grad;
typedef struct chub_policy_grad_plan_out {
    int64_t n_params;             /* sum over layers of out * (in + 1); log_std's G come on top */
    int64_t workspace_bytes;      /* what chub_policy_grad_create(max_rows = R) allocates */
    int32_t workgroups, lds_rows, lds_bytes, in_registers;
} chub_policy_grad_plan_out;
typedef struct chub_policy_grad_in {
    int64_t R, n_rows;            /* rows of this call; rows the per-row arrays hold */
    const int64_t *d_rows;        /* [R] or NULL */
    const float *d_features;      /* [n_rows][F], row stride ld_features */
    int64_t ld_features;
    const uint64_t *d_pile_bits, *d_set_bits;  /* [n_rows][W] */
    const float *d_u, *d_logp_old, *d_adv;     /* [n_rows][G], [n_rows], [n_rows] */
    const double *d_adv_stats;    /* [3] or NULL */
    int32_t loss;                 /* CHUB_PLOSS_* */
    float clip_eps, ent_coef;
    int32_t pad_;
} chub_policy_grad_in;
typedef struct chub_policy_grad_out {
    float *d_gW[4], *d_gb[4];
    float *d_glog_std, *d_logp_new, *d_entropy;
    double *d_stats;
} chub_policy_grad_out;
int chub_policy_grad_plan(const chub_config *cfg, const chub_policy_spec *spec, int64_t R, chub_policy_grad_plan_out *out);
int chub_policy_grad_create(chub_policy *pol, int64_t max_rows, chub_policy_grad **out);
int chub_policy_grad_destroy(chub_policy_grad *g);
int chub_policy_grad_device(chub_policy_grad *g, const chub_policy_grad_in *in, const chub_policy_grad_out *out, void *stream);

/* ---- a critic on the device: values, value loss and its gradient -----------------------------------------------------------------------
 * The value function of a policy-gradient update: V over rows of a collected rollout (what chub_rollout_gae_device takes as d_values) and
 * the gradient of a regression on `ret` with respect to the critic's weights.  A chub_critic is a feed-forward network over rows of F
 * floats with ONE linear output; it is bound to a handle as a policy is, destroyed by chub_destroy before the handle, and allocated
 * outside the arena: chub_state_size and snapshots are unchanged.
 *   Spec.  1 .. 4 layers, hidden widths 1 .. 256, width[n_layers - 1] = 1, F = 1 .. 512 (the limit of chub_moments), hidden_act one of
 *     CHUB_PACT_*.  The critic has no input blocks of its own: it reads rows the caller points at -- d_x with row stride ld >= F floats,
 *     n_rows rows, and optionally d_rows [R] int64 picking them, exactly as chub_policy_grad_in does (an index outside 0 .. n_rows - 1 is
 *     skipped: it adds to nothing, is not counted, and its value is written as 0; a repeated index counts as often as it is named).  The
 *     rows it is meant for are a rollout's d_features [T][N][F], the raw rows the actor saw at each step; for an OBS-only actor they are
 *     also d_obs0, the packed blocks (ld = D + 2) and d_final_obs.
 *   Normaliser.  With normalize the critic has its own mean / inv_std [F], applied exactly as the actor applies its own:
 *     x = clamp((row - mean) * inv_std, -clip, clip), f32 subtraction, f32 product, clamp.  chub_critic_set_normalizer (host memory; it
 *     synchronises), chub_critic_set_normalizer_device (device memory, on `stream`) and chub_critic_normalizer_from_moments_device (from
 *     a chub_moments of the same handle and F, as chub_policy_normalizer_from_moments_device) mirror the policy's three calls.
 *   Forward.  The actor's numerics contract: every product is rounded once, accumulation is in f32 from the bias in ascending input
 *     order on v_mfma_f32_32x32x2_f32, tanh is the device library's tanhf, relu is exact.  The head is a linear output v with no squash.
 *     Two calls on the same inputs give identical bits whatever R, d_rows or a row's place in the call, and the value the forward-only
 *     call writes and the v inside a gradient call are the same bits.  A PILES / CHUB_PSQ_CLIP actor whose hidden layers are the critic's
 *     and whose head row S is the critic's head row forms the same bits in d_tail[.][0] wherever |v| < 1.
 *   Weights.  chub_critic_set_weights is the host form (it copies and synchronises); chub_critic_set_weights_device takes W [out][in] and
 *     b [out] in device memory in the trainer's layout and runs a re-layout launch on `stream` (recordable).  The buffers the kernel
 *     reads never move.
 *   chub_critic_values_device is the forward alone: V of rows d_rows[0 .. R - 1] (NULL: rows 0 .. R - 1) into d_values [R], at position r
 *     of the call.  One launch; no backward, no allocation, no synchronisation, no tick; recordable.
 *   chub_critic_grad_device.  in: R, n_rows, d_rows, d_x, ld, d_ret [n_rows], d_v_old [n_rows] (read under CLIPPED only), loss, clip_eps.
 *     CHUB_VLOSS_MSE:      L = (1 / R) sum_r 0.5 (v - ret)^2; per row R dL/dv = v - ret, ONE f32 subtraction; the row's loss term in the
 *                          stats is 0.5 times the f64 square of that f32 difference.
 *     CHUB_VLOSS_CLIPPED:  PPO2's clipped value loss: d = v - v_old, v_c = v_old + clamp(d, -eps, eps), e1 = (v - ret)^2,
 *                          e2 = (v_c - ret)^2, each operation rounded once in f32; L = (1 / R) sum_r 0.5 max(e1, e2) (the row's loss term
 *                          is 0.5 times the f64 value of the f32 maximum).  A row is ACTIVE iff (d > -eps and d < eps) or e1 >= e2; there
 *                          R dL/dv = v - ret, elsewhere 0.  A d exactly on a bound, or e1 == e2 outside the range, is not defined beyond
 *                          this predicate.
 *     Hidden layers pass delta as the actor's gradient does: tanh delta (1 - h^2), relu delta [h > 0].  The normaliser is a constant.
 *     Products are rounded once and accumulated in f32 on the f32-input MFMA over the rows a workgroup walks (32 rows per chain link, a
 *     workgroup's tiles in ascending order); 1 / R is applied ONCE, to the f64 sum of the workgroups' f32 partials in workgroup order,
 *     and the result is rounded once to f32.  No atomics: two calls on the same inputs give identical bits, and the order is a function
 *     of (R, spec) alone.
 *     out, each optional: d_gW[l] [out][in] and d_gb[l] [out] in the TRAINER's layout; d_values [R], written at position r; d_stats [6]
 *     f64: rows counted, sum of the rows' loss terms, rows whose gradient was clipped away (0 under MSE), sum of (ret - v)^2, sum of ret,
 *     sum of ret^2 (the last three are the ingredients of explained variance), all f64 from the row up.  With every gradient output NULL
 *     the call is the forward plus stats: no backward.  Launches of one call with a backward, on the caller's stream: a small launch
 *     that rebuilds zero-padded row-major copies of layers 1.. from the critic's LIVE device weights, the forward/backward launch, the
 *     merge.  No allocation, no synchronisation, no tick; recordable.  The copies and the partials belong to the critic: its gradient
 *     calls must be ordered against each other.
 *   chub_critic_plan: host-only, no device: the parameter count (sum of out * (in + 1)), the workgroups of a call of R rows, the LDS rows
 *     and bytes, whether the dW tiles stay in registers, and the workspace chub_critic_create allocates for max_rows = R -- or the refusal
 *     create would give.  The fit rule and the workgroup rule are chub_policy_grad_plan's with the head's single output rounded up to
 *     one tile of 32: LDS rows = F rounded up to 32 + every hidden width rounded up to 32 + twice the widest layer output rounded up
 *     to 32 + 16, each row 33 floats, at most 160 KiB; workgroups = ceil(R / 32) rounded up to 8, at most 512, fewer where the partials
 *     would pass 256 MiB; in registers with at most 16 dW tiles of 32 x 32 over all layers.  13 -> 64 -> 64 -> 1 takes 304 rows.
 * Refusals, all with a message and before any device work.  CHUB_ERR_ARG: null arguments; F, n_layers or widths out of range; last
 *     width != 1; an unknown activation or loss; clip <= 0 or NaN with normalize; normalize without mean / inv_std; a normaliser call on a
 *     critic made with normalize = 0; R <= 0, R > max_rows, n_rows < 1, R > n_rows without d_rows, ld < F; null d_x, or null d_ret in a
 *     gradient call; null d_v_old or eps <= 0 or not finite under CLIPPED; null d_values in the values call; moments of another handle or
 *     another F; max_rows < 1.  CHUB_ERR_UNSUPPORTED: the fit rule; create, destroy or a host set_* between chub_graph_begin and
 *     chub_graph_end.
 * Out of scope: a trunk shared with the actor, return normalisation, an optimiser (see "an optimiser on the device", below), bf16, the multi-GPU hosts, and terminal values for
 *     feature rows with non-OBS blocks: the state is gone by then, so d_final_values is NULL and an episode's end is worth 0 for such
 *     critics. */
enum { CHUB_VLOSS_MSE = 0, CHUB_VLOSS_CLIPPED, CHUB_VLOSS_COUNT };
typedef struct chub_critic chub_critic;
typedef struct chub_critic_spec {
    int32_t F;
    int32_t n_layers;
    int32_t width[4];             /* outputs of layer l; width[n_layers - 1] = 1 */
    int32_t hidden_act;           /* CHUB_PACT_* */
    int32_t normalize;
    float clip;
} chub_critic_spec;
typedef struct chub_critic_plan_out {
    int64_t n_params;             /* sum over layers of out * (in + 1) */
    int64_t workspace_bytes;      /* what chub_critic_create(max_rows = R) allocates beside the weights */
    int32_t workgroups, lds_rows, lds_bytes, in_registers;
} chub_critic_plan_out;
typedef struct chub_critic_grad_in {
    int64_t R, n_rows;            /* rows of this call; rows the per-row arrays hold */
    const int64_t *d_rows;        /* [R] or NULL */
    const float *d_x;             /* [n_rows][F], row stride ld */
    int64_t ld;
    const float *d_ret, *d_v_old; /* [n_rows] each; d_v_old is read under CHUB_VLOSS_CLIPPED only */
    int32_t loss;                 /* CHUB_VLOSS_* */
    float clip_eps;
} chub_critic_grad_in;
typedef struct chub_critic_grad_out {
    float *d_gW[4], *d_gb[4];
    float *d_values;              /* [R] */
    double *d_stats;              /* [6] */
} chub_critic_grad_out;
int chub_critic_plan(const chub_critic_spec *spec, int64_t R, chub_critic_plan_out *out);
int chub_critic_create(chub_env *env, const chub_critic_spec *spec, const float *const *W, const float *const *b, const float *mean,
                       const float *inv_std, int64_t max_rows, chub_critic **out);
int chub_critic_destroy(chub_critic *c);
int chub_critic_set_weights(chub_critic *c, int32_t layer, const float *W, const float *b);
int chub_critic_set_weights_device(chub_critic *c, int32_t layer, const float *d_W, const float *d_b, void *stream);
int chub_critic_set_normalizer(chub_critic *c, const float *mean, const float *inv_std);
int chub_critic_set_normalizer_device(chub_critic *c, const float *d_mean, const float *d_inv_std, void *stream);
int chub_critic_normalizer_from_moments_device(chub_critic *c, chub_moments *m, double eps, void *stream);
int chub_critic_values_device(chub_critic *c, const float *d_x, int64_t ld, int64_t n_rows, const int64_t *d_rows /* [R] or NULL */, int64_t R,
                              float *d_values /* [R] */, void *stream);
int chub_critic_grad_device(chub_critic *c, const chub_critic_grad_in *in, const chub_critic_grad_out *out, void *stream);

/* ---- an optimiser on the device: Adam, gradient clipping, minibatch shuffles, weights read back ------------------------------------------
 * What closes a PPO epoch inside the library: an Adam step that reads gradients where chub_policy_grad_device / chub_critic_grad_device
 * leave them and writes the new weights straight into the kernels' own layout, a counter-based row shuffle whose slices are the d_rows
 * of the two gradient calls, and the calls that hand the trained weights back.  After them M minibatches of (shuffle slice, actor
 * gradient, critic gradient, two steps) are a chain of launches with nothing on the host between them, capturable as one graph whose
 * every replay continues from the weights, moments and counter the last one left.
 *   The parameter vector.  Flat, in the trainer's (torch's state_dict) order: for each layer W[l] row-major [out][in], then b[l]; for a
 *     policy that had chub_policy_set_exploration at create, log_std [G] last.  n is its length.  m and v are f32 [n] in that order.
 *     chub_adam_grads gives pointers into a gradient buffer of the object's own in the same order (d_gW / d_gb of layers the target has
 *     not: NULL; d_glog_std: NULL without log_std): what chub_policy_grad_out / chub_critic_grad_out is filled with there needs no
 *     allocation by the caller.  chub_adam_step_device takes any device pointers, these included.
 *   There is no master copy.  The parameters are the target's LIVE device weights (per tile of 32 outputs [k_pad][32], biases
 *     [tiles * 32]) and the policy's log_std buffer.  A lane owns one real parameter: it finds that parameter's place in the layout,
 *     reads it, writes it; the zero padding beyond `in` and `out` is never touched.  chub_*_set_weights* on the target between steps
 *     cannot make anything stale (the next step starts from the new weights and the old moments), and the next act, sample, values or
 *     gradient call in the stream sees the new weights without a re-layout launch.
 *   One step.  Every operation is an f64 operation rounded once unless said otherwise; t (int64), p1, p2 (f64) and the hyper-parameters
 *     live in device memory.
 *       1. norm = sqrt(sum g^2) over all n entries.  The squares are exact in f64.  The order of the sum: chunk c is entries 1024 c ..;
 *          lane j of 256 adds entries j, j + 256, j + 512, j + 768 of the chunk in that order from 0 (an entry past n adds +0); the
 *          lanes meet in a tree, lane j += lane j + 128, then + 64, .. + 1; the chunks' sums are added in ascending order from 0.
 *       2. norm not finite: the step is SKIPPED.  Weights, m, v, t, p1, p2 keep their bits; stats = {t, norm, 0, 1}.
 *       3. scale = (float) min(1, max_grad_norm / (norm + 1e-6)); with max_grad_norm == 0 scale is exactly 1.
 *       4. t += 1; p1 *= beta1; p2 *= beta2 (running products, not pow).
 *       5. Per parameter: g' = (double) g * (double) scale (exact); m32 = (float) (beta1 * m + (1 - beta1) * g');
 *          v32 = (float) (beta2 * v + (1 - beta2) * (g' * g')); from the STORED f32 values denom = sqrt(v32) / sqrt(1 - p2) + eps;
 *          th = (double) theta; for entries of a W only, where weight_decay != 0: th = th * (1 - lr * weight_decay) (biases and log_std
 *          are never decayed); th = th - (lr / (1 - p1)) * (m32 / denom); theta = (float) th.  1 - beta1 and 1 - beta2 are f64
 *          differences formed once.
 *       6. stats = {t, norm, scale, 0}.
 *       An optimiser with a gate (chub_adam_set_gate: "a training log and a KL stop on the device", below) whose word is not 0 is HELD
 *       BACK after 1. exactly as 2. skips it, with stats = {t, norm, 0, 2}.
 *   Launches.  A step is TWO launches, whatever the layer count, on the caller's stream: the first writes the chunks' sums and copies
 *     t, p1, p2 into a "previous" block; in the second every workgroup adds the sums, reads "previous", and lane 0 of workgroup 0 alone
 *     writes the new scalars: a launch never reads what another of its workgroups writes.  Both launches run min(chunks, 64) workgroups
 *     that take chunks b, b + 64, ..  No allocation, no synchronisation, no tick, no atomics: two objects fed the same gradients hold
 *     identical bits.  Recordable between chub_graph_begin and chub_graph_end (it is no reset or step of the handle: the count of those
 *     is not touched); a replayed graph advances t, p1, p2 by itself.  chub_adam_set_lr_device copies one f64 from device memory into
 *     the object's lr on the stream: a schedule inside a graph.  chub_adam_counter_device gives the address of t.
 *   chub_adam_plan: host-only, no device: n, the state blob's bytes, the device memory create allocates (m, v, the gradient buffer,
 *     the chunks' sums, the scalars) and the workgroups of the two launches, for layers out_dims[l] x in_dims[l] and G log_std entries.
 *   Ownership.  Allocated outside the arena: chub_state_size and snapshots are unchanged.  chub_policy_destroy, chub_critic_destroy and
 *     chub_destroy destroy a target's optimisers first.  The state blob is {int64 t, double p1, double p2, int64 n}, m[n], v[n]:
 *     32 + 8 n bytes; chub_adam_set_state refuses a blob whose n differs.  chub_adam_reset_device: m = v = 0, t = 0, p1 = p2 = 1.
 *   Reading weights back.  chub_policy_get_weights_device / chub_critic_get_weights_device write W [out][in] and b [out] of one layer
 *     in the trainer's layout (one launch on `stream`), chub_policy_get_log_std_device [G] (one copy); the forms without _device take
 *     host memory and synchronise.
 *   chub_shuffle_rows_device: d_rows[r], r = 0 .. R - 1, is a permutation of 0 .. R - 1, a pure function of (key, c, R) with
 *     c = *d_counter + offset as uint64 (d_counter NULL: 0), read on the device.  nb is the bit length of R - 1, lo = nb >> 1,
 *     hi = nb - lo; left = x >> lo has hi bits, right is the low lo bits.  E(x) is six rounds i = 0 .. 5: even i
 *     left ^= F_i(right) & mask_hi, odd i right ^= F_i(left) & mask_lo, with F_i(val) word 0 of Philox4x32-10 at counter
 *     (val, 17 << 16 | i, low word of c, high word of c) under key (low word first).  d_rows[r] is cycle-walked: y = E(r), and while
 *     y >= R, y = E(y), at most 64 applications of E; an entry that has not landed by then is written as -1, which the gradient calls
 *     skip.  R = 1 writes 0.  One launch, one lane per r (a lane takes r, r + 2^20, .. beyond 2^20 rows), no tick; recordable.  Pointing
 *     d_counter at chub_adam_counter_device's t gives every replay of a captured epoch a new shuffle; `offset` tells several shuffles
 *     apart within one graph.  chub_shuffle_rows is the same definition in host C, no device.
 * Refusals, all with a message and before any device work.  CHUB_ERR_ARG: a null argument; lr, eps, weight_decay or max_grad_norm
 *     negative or not finite; a beta outside [0, 1); a null d_gW[l] or d_gb[l] for a layer the target has; a null d_glog_std where the
 *     vector has log_std, a non-null one where it has not; a blob of another n; a layer outside 0 .. n_layers - 1; log_std calls on a
 *     policy without chub_policy_set_exploration; R < 1 or R > 2^40.  CHUB_ERR_UNSUPPORTED: create, destroy and the host forms between
 *     chub_graph_begin and chub_graph_end.
 * Out of scope: other optimisers, per-layer learning rates, a clamp on log_std, AMSGrad, populations, the multi-GPU hosts. */
typedef struct chub_adam chub_adam;
typedef struct chub_adam_hyper { double lr, beta1, beta2, eps, weight_decay, max_grad_norm; } chub_adam_hyper;
typedef struct chub_adam_plan_out { int64_t n; int64_t state_bytes; int64_t workspace_bytes; int32_t norm_workgroups, step_workgroups; } chub_adam_plan_out;
int chub_adam_plan(const int32_t *out_dims, const int32_t *in_dims, int32_t n_layers, int32_t G, chub_adam_plan_out *out);
int chub_adam_create_policy(chub_policy *pol, const chub_adam_hyper *h, chub_adam **out);
int chub_adam_create_critic(chub_critic *c, const chub_adam_hyper *h, chub_adam **out);
int chub_adam_destroy(chub_adam *a);
int chub_adam_set_hyper(chub_adam *a, const chub_adam_hyper *h);                       /* host; synchronises */
int chub_adam_set_lr_device(chub_adam *a, const double *d_lr, void *stream);
int chub_adam_grads(chub_adam *a, float **d_gW /* [4] */, float **d_gb /* [4] */, float **d_glog_std);
int chub_adam_counter_device(chub_adam *a, const int64_t **d_t);
int chub_adam_step_device(chub_adam *a, const float *const *d_gW, const float *const *d_gb, const float *d_glog_std, double *d_stats /* [4] or NULL */,
                          void *stream);
int chub_adam_reset_device(chub_adam *a, void *stream);
int chub_adam_state_size(chub_adam *a, int64_t *bytes);
int chub_adam_get_state(chub_adam *a, void *blob);                                     /* host; synchronises */
int chub_adam_set_state(chub_adam *a, const void *blob);                               /* host; synchronises */
int chub_policy_get_weights_device(chub_policy *pol, int32_t layer, float *d_W, float *d_b, void *stream);
int chub_policy_get_weights(chub_policy *pol, int32_t layer, float *W, float *b);      /* host; synchronises */
int chub_policy_get_log_std_device(chub_policy *pol, float *d_log_std /* [G] */, void *stream);
int chub_policy_get_log_std(chub_policy *pol, float *log_std /* [G] */);               /* host; synchronises */
int chub_critic_get_weights_device(chub_critic *c, int32_t layer, float *d_W, float *d_b, void *stream);
int chub_critic_get_weights(chub_critic *c, int32_t layer, float *W, float *b);        /* host; synchronises */
int chub_shuffle_rows_device(chub_env *env, uint64_t key, const int64_t *d_counter /* or NULL: 0 */, int64_t offset, int64_t R, int64_t *d_rows /* [R] */,
                             void *stream);
int chub_shuffle_rows(uint64_t key, uint64_t counter, int64_t R, int64_t *rows);       /* host-only restatement in C, no device */

/* ---- a training log and a KL stop on the device: the numbers of a recorded PPO update, target_kl, the update as one call ------------------
 * A recorded epoch overwrites the stats blocks of its gradient calls and steps minibatch by minibatch, and nobody is on the host to break
 * its loop.  A chub_train_log is one block of CHUB_TLOG_WORDS f64 words plus one int64 GATE word in device memory that three small
 * launches keep: the sums a trainer prints after an update, and the stop that an approximate KL past its limit sets and that the
 * optimiser steps honour.  It is bound to a handle, destroyed by chub_destroy before the handle, and allocated outside the arena:
 * chub_state_size and snapshots are unchanged.
 *   The words (CHUB_TLOG_*): COUNTED minibatches counted; AFTER_STOP minibatches recorded after the stop (they are not counted);
 *     STOPPED 0 / 1; STOP_INDEX the record call that set the stop, counting the record calls since begin from 0, -1 if none;
 *     ACTOR + 0 .. 5 the sums of chub_policy_grad_device's stats[0 .. 5] (rows, loss terms, entropies, logp_old - logp_new, rows clipped
 *     away, ratios); KL_MAX, KL_LAST the largest and the last KL estimate over the counted minibatches (the first counted minibatch sets
 *     KL_MAX whatever its sign; a NaN never replaces it); CRITIC + 0 .. 5 the sums of chub_critic_grad_device's stats[0 .. 5] (rows, loss
 *     terms, rows clipped away, (ret - v)^2, ret, ret^2); ACTOR_OPT + 0 .. 5 and CRITIC_OPT + 0 .. 5 per optimiser: steps taken, steps
 *     skipped by a norm that is not finite, steps held back by the gate, the sum of the norms, the largest norm, steps with scale < 1.
 *   chub_train_log_begin_device: every word 0, STOP_INDEX -1, the gate 0.
 *   chub_train_log_record_device runs after the two gradient calls of a minibatch and before its steps, on their stats blocks d_pstats [6]
 *     and d_cstats [6] (either may be NULL).  With STOPPED set it adds 1 to AFTER_STOP and nothing else.  Otherwise, with n = pstats[0],
 *     every f64 operation rounded once: CHUB_KL_K1 kl = pstats[3] / n; CHUB_KL_K3 kl = (pstats[5] / n - 1) + pstats[3] / n, the mean of
 *     (ratio - 1) - log ratio; n == 0 or no d_pstats: kl = 0.  Both blocks are added into ACTOR.. and CRITIC.., one addition per word in
 *     the order of the record calls; KL_MAX, KL_LAST and COUNTED follow.  With kl_limit > 0 and !(kl <= kl_limit) -- a NaN estimate
 *     stops -- STOPPED and the gate become 1 and STOP_INDEX the call's index.  The minibatch that sets the stop IS counted and is not
 *     stepped.  chub_train_log_fold is the same source run on host memory, no device.
 *   chub_train_log_steps_device runs after the minibatch's steps, on the two stats blocks [4] of chub_adam_step_device (either may be
 *     NULL).  By stats[3]: 0 taken, 1 skipped, 2 held back.  The norm's sum and maximum take every FINITE norm, whatever became of the
 *     step; scale < 1 counts taken steps only.  It counts after the stop as before it.
 *   The gate.  chub_adam_set_gate points an optimiser at an int64 in device memory (NULL clears).  Where that word is not 0 a step
 *     returns as it does for a norm that is not finite: weights, m, v, t, p1, p2 keep their bits, and stats = {t, norm, 0, 2}; the norm
 *     launch still runs.  Every workgroup of the step launch reads the word, which only an earlier launch writes.  Without a gate a step
 *     is what it was.  chub_train_log_destroy clears the gate of every optimiser of the handle that points at the log's.
 *   Launches.  begin, record and steps are ONE launch of one workgroup each; lane 0 folds (the fold is a chain through thirty words).
 *     No launch reads a word another of its workgroups writes; no atomics; no allocation, no synchronisation, no tick.  Recordable
 *     between chub_graph_begin and chub_graph_end (no reset or step of the handle: the count of those is not touched).
 *     chub_train_log_device gives the addresses of the words and of the gate; chub_train_log_read copies the words to host memory and
 *     synchronises.
 *   chub_ppo_update is a host loop over existing calls, as chub_policy_collect is for the rollout; it returns after enqueueing.  With
 *     M = ceil(n_rows / minibatch_rows) minibatches per epoch, the last of the remainder (chub_ppo_update_plan: host arithmetic only),
 *     it issues: with a log, begin; per epoch e = 0 .. epochs - 1 chub_shuffle_rows_device(key, the ACTOR optimiser's t, offset e, n_rows)
 *     into d_rows; per minibatch i on d_rows + i * minibatch_rows: the actor gradient into the actor optimiser's own buffers
 *     (chub_adam_grads), the critic gradient likewise, record, the actor step, the critic step, steps.  With a log both optimisers have
 *     the log's gate for the duration of the call (whatever gate they had is theirs again afterwards); without one record, steps and
 *     begin are left out and the optimisers keep the gate they have.  The four stats blocks are the log's own; without a log each
 *     optimiser owns a gradient block [6] and a step block [4] (80 bytes beside what chub_adam_plan counts).  d_rows [n_rows] int64 is
 *     the caller's.  The critic reads the feature rows (d_features, ld_features).
 * Refusals, all with a message and before any device work.  CHUB_ERR_ARG: a null argument; an unknown kl_kind; kl_limit negative or
 *     NaN; for chub_ppo_update: epochs < 1; minibatch_rows < 1 or above the gradient object's or the critic's max_rows; a null d_rows;
 *     objects of different handles; an optimiser whose target is not the given policy / critic; and whatever a constituent call
 *     refuses, under that call's name.  CHUB_ERR_UNSUPPORTED: create, destroy and read between chub_graph_begin and chub_graph_end.
 * Out of scope: after a stop the gradient launches of the remaining minibatches still run and are wasted (gating them would need the
 *     word inside the gradient kernels; the host cannot know of the stop without a read); a log per epoch; the multi-GPU hosts. */
enum {
    CHUB_TLOG_COUNTED = 0, CHUB_TLOG_AFTER_STOP = 1, CHUB_TLOG_STOPPED = 2, CHUB_TLOG_STOP_INDEX = 3, CHUB_TLOG_ACTOR = 4,
    CHUB_TLOG_KL_MAX = 10, CHUB_TLOG_KL_LAST = 11, CHUB_TLOG_CRITIC = 12, CHUB_TLOG_ACTOR_OPT = 18, CHUB_TLOG_CRITIC_OPT = 24,
    CHUB_TLOG_WORDS = 30
};
enum { CHUB_KL_K1 = 0, CHUB_KL_K3, CHUB_KL_COUNT };
typedef struct chub_train_log chub_train_log;
typedef struct chub_ppo_update_args {
    chub_policy_grad *grad;       /* the actor's gradient object (and through it the policy) */
    chub_critic *critic;
    chub_adam *actor_opt, *critic_opt;
    chub_train_log *log;          /* or NULL */
    int64_t n_rows;               /* rows the per-row arrays hold: all of them are shuffled */
    const float *d_features;      /* [n_rows][F], row stride ld_features: the actor's and the critic's rows */
    int64_t ld_features;
    const uint64_t *d_pile_bits, *d_set_bits;
    const float *d_u, *d_logp_old, *d_adv;
    const double *d_adv_stats;    /* [3] or NULL */
    const float *d_ret, *d_v_old;
    int32_t policy_loss, value_loss;   /* CHUB_PLOSS_*, CHUB_VLOSS_* */
    float policy_clip_eps, value_clip_eps, ent_coef;
    int32_t epochs;
    int64_t minibatch_rows;
    uint64_t key;
    int64_t *d_rows;              /* [n_rows], the caller's */
    int32_t kl_kind;              /* CHUB_KL_* */
    int32_t pad_;
    double kl_limit;              /* 0: never stops */
} chub_ppo_update_args;
int chub_train_log_create(chub_env *env, chub_train_log **out);
int chub_train_log_destroy(chub_train_log *log);
int chub_train_log_begin_device(chub_train_log *log, void *stream);
int chub_train_log_record_device(chub_train_log *log, const double *d_pstats /* [6] or NULL */, const double *d_cstats /* [6] or NULL */, int32_t kl_kind,
                                 double kl_limit, void *stream);
int chub_train_log_steps_device(chub_train_log *log, const double *d_astats_actor /* [4] or NULL */, const double *d_astats_critic /* [4] or NULL */,
                                void *stream);
int chub_train_log_device(chub_train_log *log, const double **d_words, const int64_t **d_gate);
int chub_train_log_read(chub_train_log *log, double *words /* [CHUB_TLOG_WORDS] */);   /* host; synchronises */
int chub_train_log_fold(double *words, int64_t *gate, const double *pstats, const double *cstats, int32_t kl_kind,
                        double kl_limit);                                              /* host-only: the record step, no device */
int chub_adam_set_gate(chub_adam *a, const int64_t *d_gate /* or NULL: none */);
int chub_ppo_update_plan(int64_t n_rows, int64_t minibatch_rows, int64_t *minibatches, int64_t *last_rows);  /* host-only */
int chub_ppo_update(const chub_ppo_update_args *args, void *stream);

/* ---- constrained PPO on the device: step terms kept per step, cost advantages, Lagrange multipliers, the combined advantage ---------------
 * PPO-Lagrangian on what the step terms expose (CHUB_ST_GRID_EXCESS, CHUB_ST_NOT_MEET, CHUB_ST_SOC_PENALTY, ..): the reference's constructor
 * takes use_lagrange and its step() keeps the block commented out (MGR:275-297).  A chub_lagrange holds K = 1 .. CHUB_LAG_MAX_K constraints,
 * their multipliers lambda [K] f64, a stats block [K][CHUB_LAG_STATS] f64, per constraint the words {J_last, steps taken, steps skipped}
 * (f64) and the partials of the reduction, sized at create from N -- all in device memory outside the arena: chub_state_size and snapshots
 * are unchanged.  It is bound to a handle and destroyed by chub_destroy before the handle.  Cost critics are chub_critic objects trained on
 * d_ret[k] by the existing calls.
 *   chub_policy_collect_terms: chub_policy_collect (which < 0) or chub_policy_collect_set (which >= 0; the same rules and refusals) that
 *     also keeps every step's terms: block t of d_terms [T][N][C] f32, C = chub_get_step_terms_size(fields), is bit for bit what a buffer
 *     attached with chub_set_step_terms(env, fields, ..) holds right after step t of the same loop; under CHUB_PRUN_AUTORESET a finished
 *     env's row therefore holds its terminal step's terms.  Whatever attachment the handle had is in force again when the call returns,
 *     and its buffer is not written by the call.  Recordable as chub_policy_collect is: the per-step destination is a launch argument.
 *   A constraint: `column` is a column of the d_terms rows the object is given, `kind` how a step's cost c_t is read from it:
 *     CHUB_COST_STEP the column's value; CHUB_COST_AT_DONE the column's value where packed[t][D + 1] != 0 and exactly +0.0f elsewhere
 *     (on CHUB_ST_SOC_PENALTY: the reference's test_penalty as an end-of-day constraint).  J, the constrained quantity, is the mean cost
 *     of a finished episode; `limit` is its bound, `lr` the multiplier's step, `lambda0` its start, `lambda_max` its ceiling (0: none).
 *   chub_lagrange_gae_device: kernel k_cost_gae plus a one-workgroup merge on `stream`.  Per env, for every constraint, in one pass
 *     t = T-1 .. 0:
 *       Advantage: chub_rollout_gae_device's recurrence operation for operation with c_t in place of packed[t][D] (f32, every operation
 *         rounded once, no contraction, gl formed once); d_values[k] NULL: V = 0 everywhere; d_final_values[k] NULL: an end is worth 0.
 *       Episode cost, f64, with seg = 0 and open = true: at a step with done -- if open, carry_out = seg, else the segment is a finished
 *         episode of cost seg; then seg = (double) c_t, open = false.  At a step without done seg = seg + (double) c_t.  After t = 0 with
 *         carry_in = d_ep_carry[e][k] (0 without d_ep_carry): x = carry_in + seg; if open carry_out = x, else x is a finished episode.
 *         d_ep_carry[e][k] = carry_out.  A finished episode of cost x adds (1, x, x x) to the env's three episode sums.
 *       Stats [k][0 .. 5]: count, sum and sum of squares of the advantages written; episodes finished, the sum of their costs, the sum
 *         of the costs' squares.
 *       Reduction order (chub_rollout_gae_device's): a lane takes its env's sums in the order it writes (t descending; per step the
 *         advantage, then an episode that step closes; the episode closed after t = 0 last); lanes are envs 256 b .. 256 b + 255 of
 *         workgroup b and meet in the tree h = 128, 64, .. 1 (lane l += lane l + h); lane l of the merge workgroup takes partials l,
 *         l + 256, .. ascending from 0, then the same tree.  No atomics: two calls give identical bits.
 *       With d_mask the other envs are not read, not written and not counted, and their carry keeps its bits.
 *     A cost load is 4 bytes at a stride of C floats: collect only the columns you constrain (C = K is the fast case).
 *   chub_lagrange_step_device: one launch of one wave, lane k per constraint, f64, every operation rounded once: n = stats[k][3],
 *     J = stats[k][4] / n.  n == 0 or J not finite: lambda keeps its bits, skipped += 1.  Else l = lambda + lr (J - limit);
 *     l = l < 0 ? 0 : l; with lambda_max != 0, l = l > lambda_max ? lambda_max : l; a NaN l leaves lambda, taken and J_last as they are
 *     and adds 1 to skipped; else lambda = l, taken += 1, J_last = J.  It reads only what an earlier launch wrote.
 *     chub_lagrange_fold is the same source on host memory for one constraint, no device.
 *   chub_lagrange_combine_device: one streaming launch over n = T N entries.  a = d_adv_stats ? (adv - m32) * s32 : adv with m32, s32
 *     chub_policy_grad_device's "Advantage" paragraph; for k ascending with l32 = (float) lambda[k]: l32 == 0 performs NO operation (with
 *     every lambda 0 the output has the normalised advantage's bits), else a = a - l32 * (advc_k - mc32_k), three operations each rounded
 *     once, mc32_k = (float) (stats[k][1] / stats[k][0]) -- cost advantages are centred, not scaled; out = a * inv32,
 *     inv32 = (float) (1 / (1 + sum_k (double) l32_k)), the sum ascending in f64 from 0.  d_out may be d_adv; it must not overlap a
 *     d_adv_cost[k].  Hand d_out to chub_policy_grad_device / chub_ppo_update as d_adv with d_adv_stats = NULL.  The call presupposes a
 *     chub_lagrange_gae_device call that counted at least one entry: with stats[k][0] == 0 (no gae yet, or every env masked out) and
 *     lambda[k] != 0, mc32_k is 0 / 0 and the whole output is NaN.
 *   chub_lagrange_device gives the addresses of lambda and the stats; chub_lagrange_read copies lambda [K], the stats [K][6] and the
 *     words [K][3] to host memory (each may be NULL) and synchronises; chub_lagrange_set_lambda_device copies K f64 words from device
 *     memory in one launch; chub_lagrange_get_state / _set_state move a blob of chub_lagrange_state_size bytes (K, lambda, the words)
 *     for checkpoints: a blob of another K is refused.
 *   Manners of the device calls: no tick, no simulation state read, no allocation, no synchronisation; recordable between
 *     chub_graph_begin and chub_graph_end, not counted among its resets and steps.  Calls on one object must be ordered against each other.
 * Refusals, all with a message and before any device work.  CHUB_ERR_ARG: a null argument; K outside 1 .. 4; a column below 0 (create) or
 *     above C - 1 (gae); an unknown kind; lr, limit, lambda0 or lambda_max negative or not finite; lambda0 above a non-zero lambda_max;
 *     T <= 0; gamma or lambda outside [0, 1] or NaN; a null d_terms, d_packed or d_adv[k]; n < 1; for chub_policy_collect_terms telemetry
 *     off, a bad mask or a null d_terms, and whatever chub_policy_collect(_set) refuses.  No C call takes both a handle and an object:
 *     the Python adapter refuses an object made for another handle.  CHUB_ERR_UNSUPPORTED: create, destroy, read and the state calls
 *     between chub_graph_begin and chub_graph_end; a step's block of d_packed or d_terms beyond 4 GiB (the kernel's offsets are 32 bits).
 * Out of scope: a multi-output critic (one chub_critic per constraint); PID or Adam on lambda; gating the policy update on feasibility;
 *     populations; the multi-GPU hosts; COMPAT rollouts. */
enum { CHUB_COST_STEP = 0, CHUB_COST_AT_DONE, CHUB_COST_KIND_COUNT };
enum { CHUB_LAG_MAX_K = 4, CHUB_LAG_STATS = 6, CHUB_LAG_WORDS = 3 };
typedef struct chub_lagrange chub_lagrange;
typedef struct chub_constraint {
    int32_t column;               /* within a d_terms row */
    int32_t kind;                 /* CHUB_COST_* */
    double limit, lr, lambda0, lambda_max;
} chub_constraint;
typedef struct chub_cost_gae {
    int64_t T;
    int32_t C;                    /* floats of a d_terms row */
    int32_t pad_;
    const float *d_terms;         /* [T][N][C] */
    const float *d_packed;        /* [T][N][D + 2]: only done, at column D + 1, is read */
    const float *d_values[4];     /* per constraint [T + 1][N], or NULL: V = 0 */
    const float *d_final_values[4]; /* per constraint [N], or NULL: an end is worth 0 */
    const uint8_t *d_mask;        /* [N] or NULL */
    float gamma, lambda;
    float *d_adv[4];              /* per constraint [T][N], required for k < K */
    float *d_ret[4];              /* per constraint [T][N] or NULL */
    double *d_ep_carry;           /* [N][K] f64, in and out, or NULL */
} chub_cost_gae;
int chub_policy_collect_terms(chub_env *env, chub_policy *pol, int mode, int which /* < 0: chub_policy_collect */, const chub_rollout *r,
                              uint64_t *d_set_bits /* [T][N][W] where which >= 0 */, float *d_obs0, int64_t first_step, uint32_t fields,
                              float *d_terms /* [T][N][C] */, void *stream);
int chub_lagrange_create(chub_env *env, int32_t K, const chub_constraint *c /* [K] */, chub_lagrange **out);
int chub_lagrange_destroy(chub_lagrange *lag);
int chub_lagrange_gae_device(chub_lagrange *lag, const chub_cost_gae *g, void *stream);
int chub_lagrange_step_device(chub_lagrange *lag, void *stream);
int chub_lagrange_combine_device(chub_lagrange *lag, int64_t n, const float *d_adv, const double *d_adv_stats /* [3] or NULL */,
                                 const float *const *d_adv_cost /* host array [K] of device addresses */, float *d_out, void *stream);
int chub_lagrange_device(chub_lagrange *lag, const double **d_lambda, const double **d_stats);
int chub_lagrange_read(chub_lagrange *lag, double *lambda /* [K] */, double *stats /* [K][6] */, double *words /* [K][3] */); /* host; synchronises */
int chub_lagrange_set_lambda_device(chub_lagrange *lag, const double *d_lambda /* [K], device */, void *stream);
int chub_lagrange_state_size(chub_lagrange *lag, int64_t *bytes);
int chub_lagrange_get_state(chub_lagrange *lag, void *blob);
int chub_lagrange_set_state(chub_lagrange *lag, const void *blob);
int chub_lagrange_fold(const chub_constraint *c, double *lambda, double *words /* [3] */, const double *stats /* [6] */); /* host-only */

/* ---- reward scaling on the device: running statistics of the discounted return, a GAE that divides by their spread -----------------------
 * The reward side of stable-baselines' VecNormalize (norm_reward): rewards are divided by the running standard deviation of the
 * discounted return and clipped; no mean is subtracted.  The reward here is money and its scale moves with the hub's shape; everything
 * from chub_rollout_gae_device on reads it raw.  A chub_return_norm is bound to a handle and holds gamma (f32), eps (f64) and clip (f32,
 * 0 = none); in device memory, outside the arena, the state [n, mean, M2] f64, the word scale32 (f32), a carry g[N] f32 and the partials
 * of the reduction.  chub_state_size and snapshots are unchanged, no simulation state is read and no tick is consumed; chub_destroy frees
 * a handle's objects first, as it does its moments objects.  After create: state zeros, scale32 = 1.0f, carry zeros.
 *   chub_return_norm_update_device: the rollout's blocks d_packed [T][N][D + 2] into the state, two launches on `stream`.  Per counted env
 *     e, forward in t, in f32 with every operation rounded once and no contraction, g starting at carry[e]:
 *       g = gamma * g + packed[t][e][D]              (two operations)
 *       g is counted
 *       if packed[t][e][D + 1] != 0:  g = 0          (after counting: stable-baselines' order)
 *     and carry[e] = g after t = T - 1.  With d_mask [N] u8 an env not named is not read, not counted and its carry keeps its bits.  The
 *     n_b = T (counted envs) values join the state by the pivoted form of "running feature statistics", all in f64, every operation
 *     rounded once:
 *       K     = n > 0 ? mean : (double) packed[0][0][D]       (row 0 serves whether env 0 is masked or not)
 *       d     = (double) g - K,   S1 = sum d,   S2 = sum d d
 *       M2_b  = t < 0 ? 0 : t  with  t = S2 - S1 S1 / n_b     (a NaN stays a NaN)
 *       n'    = n + n_b
 *       n > 0:   mean' = K + S1 / n',   M2' = (M2 + M2_b) + (S1 / n_b)^2 (n n_b / n')
 *       n == 0:  mean' = K + S1 / n_b,  M2' = M2_b
 *       scale32 = n' == 0 ? 1.0f : (float) (1 / sqrt(M2' / n' + eps))      (the population variance; IEEE f64 division and square root)
 *     n_b == 0 writes nothing: state and scale32 keep their bits.  Order of the sums: a lane takes its env's values t ascending; lanes are
 *     envs 256 b .. 256 b + 255 of workgroup b and meet in the tree h = 128, 64, .. 1 (lane l += lane l + h); lane l of the one merge
 *     workgroup takes partials l, l + 256, .. ascending from 0, then the same tree.  No atomics: two calls give identical bits.
 *     chub_return_norm_fold is the merge and the scale as host code, compiled from the function the merge kernel runs: state [3] and
 *     *scale are updated from (n_b, K, S1, S2); it needs no device.
 *   chub_return_norm_gae_device: chub_rollout_gae_device's recurrence, operation for operation, reduction and d_stats included, with
 *     packed[t][D] replaced by
 *       r' = packed[t][D] * scale32                             (one f32 operation)
 *       if clip != 0:  r' = r' > clip ? clip : (r' < -clip ? -clip : r')     (selects: a NaN stays a NaN)
 *     scale32 is loaded from the object's device word inside the kernel: a replayed graph uses the scale its own update launch left.
 *     chub_gae is shared unchanged.  With scale32 == 1 and clip == 0 every output has chub_rollout_gae_device's bits.  The statistics'
 *     partials are the handle's one buffer: calls that ask for d_stats are ordered as chub_rollout_gae_device's are.
 *   chub_return_norm_reset_carry_device: carry[e] = 0 for the named envs (d_mask NULL: all), for lock-step trainers that reset between
 *     rollouts; chub_return_norm_reset_device: state zeros, scale32 = 1.0f, carry zeros.  One launch each.
 *   chub_return_norm_device gives the addresses of the state [3], scale32 and the carry [N] (each may be NULL); they never move.
 *   chub_return_norm_get_state / _set_state move a blob of chub_return_norm_state_size bytes for checkpoints; both synchronise.  The blob:
 *     a magic (u64), N (i64), the state [3] f64, scale32 with four bytes of padding, the carry [N] f32.  set_state installs scale32 as
 *     the blob gives it.  A blob with another magic or of another N is refused.
 *   Manners of the device calls: no synchronisation, no allocation, no atomics, the same bits on every call; recordable between
 *     chub_graph_begin and chub_graph_end, not counted among its resets and steps.  Calls on one object must be ordered against each other.
 * Refusals, all with a message and before any device work.  CHUB_ERR_ARG: a null argument (rn, spec, out, d_packed, g, its d_packed,
 *     d_values or d_adv, a blob); T <= 0; gamma (the spec's, the call's) or lambda outside [0, 1] or NaN; eps <= 0 or not finite; clip < 0
 *     or NaN; a blob of another N.  No C call takes both a handle and an object: the Python adapter refuses an object made for another
 *     handle.  The kernels address with 64 bits: no block size is refused.  CHUB_ERR_UNSUPPORTED: tape handles; create, destroy and the
 *     state calls between chub_graph_begin and chub_graph_end.
 * Out of scope: scaling cost returns (chub_lagrange limits stay in raw units); statistics per step inside a rollout (one scale per
 *     rollout: the critic's targets share a scale within a batch); writing the scaled rewards out; subtracting a mean (VecNormalize does
 *     not either); episode accounting, which stays in raw units as Monitor under VecNormalize does. */
typedef struct chub_return_norm chub_return_norm;
typedef struct chub_return_norm_spec {
    float gamma;                  /* [0, 1]: the discount of the return whose spread is tracked */
    float clip;                   /* >= 0; 0: none */
    double eps;                   /* > 0, finite */
} chub_return_norm_spec;
#define CHUB_RETURN_NORM_MAGIC 0x314d524e52424843ull   /* "CHBRNRM1" */
int chub_return_norm_create(chub_env *env, const chub_return_norm_spec *spec, chub_return_norm **out);
int chub_return_norm_destroy(chub_return_norm *rn);
int chub_return_norm_update_device(chub_return_norm *rn, const float *d_packed /* [T][N][D + 2] */, int64_t T,
                                   const uint8_t *d_mask /* [N] or NULL */, void *stream);
int chub_return_norm_gae_device(chub_return_norm *rn, const chub_gae *g, void *stream);
int chub_return_norm_reset_carry_device(chub_return_norm *rn, const uint8_t *d_mask /* [N] or NULL */, void *stream);
int chub_return_norm_reset_device(chub_return_norm *rn, void *stream);
int chub_return_norm_device(chub_return_norm *rn, const double **d_state /* [3] */, const float **d_scale /* [1] */, const float **d_carry /* [N] */);
int chub_return_norm_state_size(chub_return_norm *rn, int64_t *bytes);
int chub_return_norm_get_state(chub_return_norm *rn, void *blob);        /* host; synchronises */
int chub_return_norm_set_state(chub_return_norm *rn, const void *blob);  /* host; synchronises */
int chub_return_norm_fold(double state[3], float *scale, double n_b, double K, double S1, double S2, double eps);  /* host-only */

/* The FCEV waiting list is unbounded as in the reference (HYD:264-265): the entries a list that still gets served can
 * hold are kept one by one, and once no prefix of it fits into 15 minutes any more (HYD:270-276: nobody is served again
 * until reset and the list only grows) its entries are folded into their count and running sums, which is all the
 * reference ever reads of them again.  chub_fcev_stuck_count: number of envs whose forecourt is currently in that state. */
int chub_fcev_stuck_count(chub_env *env, int64_t *out);

/* COMPAT streams: seeds [N][2] u32 = (srand seed, e.seed()) per env, i.e. what Change_Use_Seed /
 * srand / e.seed would install (CHS.hpp:25-44). */
int chub_set_rng_compat_seeds(chub_env *env, const uint32_t *seeds);
/* Raw COMPAT stream state per env, [N][33] u32: the 31 words of glibc's TYPE_3 ring, the index of its
 * front pointer (rear = front - 3 mod 31), and the minstd_rand0 word -- to continue streams mid-sequence. */
int chub_set_rng_compat_state(chub_env *env, const uint32_t *state);
int chub_get_rng_compat_state(chub_env *env, uint32_t *state);
/* COMPAT: what the reference's constructor does with the two streams before its first reset() (MGR:25-119): one
 * evs_reset per station constructor (CHS.hpp:1152,1462) and the 101-step electrolyser sweep with live FCEV arrivals
 * (HYD:154-157), which also yields each env's hy_power_speed_list.  Call once after chub_create /
 * chub_set_rng_compat_seeds, then chub_reset (= MGR:120). */
int chub_compat_replay_constructor(chub_env *env);
/* Persistent OU states (never reset by the reference, MGR:304-316): [N][3] f64 pv, wd, price. */
int chub_set_ou_state(chub_env *env, const double *ou);

/* ---- hipGraph capture: a launch-bound loop as one submission ---------------------------------------------------------------
 * Between chub_graph_begin and chub_graph_end the device-pointer entry points (chub_reset_device, chub_step_device*,
 * chub_step_gather, chub_random_actions_device) called with `stream` are recorded, not run; chub_graph_launch replays the
 * recording.  What a replay repeats verbatim: clocks, buffers and the order of calls -- so record whole episodes (reset + 96
 * steps), an even number of calls (the state-independent draws are double-buffered), and replay only when the handle is back at
 * the clock the capture started from (slot of day, steps since the last reset mod 4: chub_graph_launch refuses otherwise).
 * What it does not repeat: the random streams -- every replay (and every call issued one by one between replays) moves the
 * Philox tick on, so a replayed episode is a new episode.  PHILOX handles only.
 * `stream` is a created stream (chub_stream_create or the caller's own), not the default stream. */
typedef struct chub_graph chub_graph;
int chub_graph_begin(chub_env *env, void *stream);
int chub_graph_end(chub_env *env, void *stream, chub_graph **out);
int chub_graph_launch(chub_graph *graph, void *stream);
int chub_graph_destroy(chub_graph *graph);

/* ---- device buffers and streams for hosts without a GPU array library (the reference-shaped Python host is ctypes + numpy):
 * plain hipMalloc / hipFree / hipMemcpy (synchronising) / hipStream* on `device`. */
int chub_malloc_device(int device, int64_t bytes, void **out);
int chub_free_device(int device, void *d_ptr);
int chub_copy_to_host(int device, void *dst, const void *d_src, int64_t bytes, void *stream);
int chub_copy_to_device(int device, void *d_dst, const void *src, int64_t bytes, void *stream);
int chub_alloc_host(int device, int64_t bytes, void **out);  /* pinned host memory: the DMA engines reach it directly */
int chub_free_host(int device, void *ptr);
int chub_stream_create(int device, void **out);
int chub_stream_destroy(int device, void *stream);
int chub_stream_sync(int device, void *stream);

/* ---- tape mode: a parity instrument for the production (PHILOX) kernels ------------------------------------------------
 * The production streams are this build's own definition, so the kernels that run them cannot be compared with the
 * reference's recorded trajectories seed for seed.  Tape mode closes that gap: the caller supplies what the streams
 * would have drawn -- per (station, env) unit the step's packed station-level decisions (64 bits: bits 0-9 one renege-pass bit per
 * queue position, 10-13 arrivals n <= 9, 14 + 4 l (l = 0..10) how many of the n arrivals stay if the queue holds l cars after the
 * renege pass; k_draw_levels decodes the word against the unit's live queue, dk_make in chub_kernels.hip) and per admitted car its
 * arrival SoC, target level and extra stay -- and the SAME packed slot kernel replays them.  Arbitrary arrival SoCs are registered as
 * classes of the class table first.  tests/test_gpu_tape.py replays every reference fixture this way, evs_reset included.
 *   chub_tape_register_soc: soc[count] -> class_ids[count].  The caller's arrival SoCs take the place of the handle's own 2048
 *                          classes, first come first row (the slot state has 11 bits for the class), so a handle that registers
 *                          any is a tape handle from then on: chub_reset / chub_step and their device / masked / bits forms return
 *                          CHUB_ERR_ARG on it (cars admitted by the build's own draws would be given the caller's SoCs).  An SoC outside
 *                          0 .. 100, or one whose stay could exceed the state word's 31 slots, is refused.  chub_tape_clear_soc starts
 *                          over at class 0 (between episodes): the next call must be the chub_reset_tape that wipes every slot --
 *                          chub_step_tape returns CHUB_ERR_ARG until then.
 *   chub_set_slots:        rows [N][S][6] i32 in hub order (station 0's slots first): class (-1 = empty), target level,
 *                          stay_time (<= 31), already_stay_time, car_steps taken, charging flag.
 *   chub_set_station_queue: line [N][2] i32 (Station::line).
 *   chub_step_tape:        one step; pk_tape [2][N] u64, car_tape [N][S][2] u32 in hub order = class, level | late << 16
 *                          (read only for slots that admit a car this step).  Host pointers. */
int chub_tape_register_soc(chub_env *env, const float *soc, int32_t count, uint32_t *class_ids);
int chub_tape_clear_soc(chub_env *env);
int chub_set_slots(chub_env *env, const int32_t *rows);
int chub_set_station_queue(chub_env *env, const int32_t *line);
int chub_step_tape(chub_env *env, const float *actions, const uint64_t *pk_tape, const uint32_t *car_tape, float *obs,
                   float *reward, uint8_t *done);
/*   chub_reset_tape:       one reset of every env, evs_reset (CHS.hpp:1209-1231 / 1520-1542) fed the reference's draws: occ_tape [2][N] u32
 *                          = what init_station_car_number and the balk pass of the empty queue came to per unit (arrivals as signed 16
 *                          bits | arrivals that stay << 16: the word k_reset_levels leaves), car_tape as above for the cars admitted. */
int chub_reset_tape(chub_env *env, const uint32_t *occ_tape, const uint32_t *car_tape, float *obs);
/* The WHOLE step / reset from the tape (round 5): the per-env tail of the production step -- k_env<.., PHILOX>, or the tail half of the
 * one-launch step k_step_fused -- takes its variates from the caller as well, where the reference draws them:
 *   exo_z    [N][3] f64  the normals of the PV, wind and price OU processes (np.random.normal inside OU_Noise.sample, renewable.py:71-76,
 *                        evcssp_manager.py:344-361), as the reference's numpy drew them; entries of processes that do not draw are not read
 *   hv_tape  [N][hv_w] u32  the forecourt: word 0 = FCEV arrivals of this step (PoissonNumber.hv_car_number_wrt_poisson, hydro_sys.py:251),
 *                        word 1 + j = arrival j's SoC, f32 bits (CarArriveRandom.mk_soc, hydro_sys.py:259)
 *   exo_days [N][2] i32  a reset's PV / wind days (random.randint inside ReNew.renew_reset, renewable.py:25,51-53)
 * With chub_set_hy_table (hy_power_speed_list as the reference's constructor built it) the observation, reward and every telemetry
 * column of the PRODUCTION kernels can be held to the reference's recorded values directly: tests/test_gpu_tape.py does, on every
 * fixture, in both launch forms (k_slot_packed + k_env, and k_step_fused).  exo_z / hv_tape (exo_days / exo_z) both null: the tail
 * keeps this build's own Philox draws, as chub_step_tape / chub_reset_tape. */
int chub_step_tape_env(chub_env *env, const float *actions, const uint64_t *pk_tape, const uint32_t *car_tape, const double *exo_z,
                       const uint32_t *hv_tape, int32_t hv_w, float *obs, float *reward, uint8_t *done);
int chub_reset_tape_env(chub_env *env, const uint32_t *occ_tape, const uint32_t *car_tape, const int32_t *exo_days, const double *exo_z,
                        float *obs);

/* Snapshot / restore of the whole simulation state (clock, streams, every slot and env variable): checkpoint /
 * resume, planners that branch from a state.  The reference cannot do this (pickling disabled, main.cpp:234; raw
 * back-pointers, CHS.hpp:238).
 *   The blob is a header, the handle's device arena, every env's last tick and, with the ledger on, its block.  The arena holds the
 *       simulation state and, riding along, what the last launch made ahead of the next step: the station draws of the next tick (pk,
 *       drw) and, in COMPAT, the shadow streams and counts of a walk that ran ahead.  The header says which of that is good: the draws are
 *       reused by the first step after chub_set_state exactly when the snapshot's last launch served every env (they are a function of
 *       the key, the tick, the env id and the queues the blob itself restores, not of the launch form that made them; redrawn, they come
 *       out the same); a COMPAT walk that ran ahead and the counts of empty slots are void after every restore, and the next step makes
 *       its own.  The continuation is bit-identical to the source handle's own, whichever launch forms the two handles run.
 *   Target: the handle the blob was taken from, or one created with the same chub_config, n_envs, env_id0, RNG mode and data directory,
 *       both with or both without per-env rows (then with the same waiting-list capacity: the largest fcev_permeate of the rows at
 *       create) and both with the ledger on or off.  chub_options may differ (tile, slot_kernel, fused_step, walk_ahead, work_order,
 *       span_*: the arena's layout does not depend on them; no_arena handles take no part).  The target need never have been reset and
 *       may be anywhere in a day, on one clock or on per-env clocks: clocks, ticks and the graph tick base come from the blob.
 *   Seed: the Philox key is the handle's, not state (as for chub_copy_envs).  A PHILOX / PHILOX_CURVES blob restored into a handle of
 *       another seed gives the source's state exactly -- every reader returns the source's values -- and from the next launch on the
 *       target draws with its OWN key: another future, the same for every such restore.  The draws that rode along were made with the
 *       source's key (the header names it), so they are void there and the first step makes its own.
 *   CHUB_ERR_ARG, with a message and nothing written (every check comes before the first write): null arguments, a buffer smaller than
 *       chub_state_size / a truncated blob, not a snapshot, another n_envs, env_id0, chub_config, RNG mode, rows against no rows, another
 *       waiting-list capacity of the rows, ledger against no ledger, a corrupt header.  CHUB_ERR_UNSUPPORTED, before any HIP call: a
 *       no_arena handle; a handle between chub_graph_begin and chub_graph_end (a snapshot synchronises and copies: take and restore it
 *       between replays; the capture goes on unharmed). */
int64_t chub_state_size(const chub_env *env);
int chub_get_state(chub_env *env, void *buf, int64_t size);
int chub_set_state(chub_env *env, const void *buf, int64_t size);

/* ---- copying envs on the device: branch, clone and seed envs by index -------------------------------------------------------------
 * Env dst_idx[i] of `dst` becomes a clone of env src_idx[i] of `src`, i = 0 .. count - 1, without leaving the device: what a deep copy of
 * the reference object gives (population-based training: the worst k envs become copies of the best k; planners: N real envs fanned out
 * into K branches each in a scratch handle; restarts from archived states).  `src` may be `dst`; one source may be named many times.
 *   Copied: everything chub_get_state counts as simulation state of that env -- every slot of both stations, the station records and
 *       queues, tank, capacity, OU states, price noise, PV / wind day, the forecourt list (its folded form included), the env's slot of day
 *       (and price-noise phase), in COMPAT the committed streams and the env's hy_power_speed_list; on handles made by chub_create_params the
 *       env's parameter row and its table: the destination becomes the same hub as the source.
 *   Not copied: the stream identity in PHILOX / PHILOX_CURVES -- the destination keeps drawing from its own counters (dst's seed, dst's
 *       tick, its own global env id), so a clone parts from its source at the next launch, and a scratch handle with another seed samples
 *       other futures.  (In COMPAT the streams ARE state: a clone given its source's actions and exo_z stays bit-identical to it.)  Draws
 *       made one launch ahead of the next step are neither copied nor reused: the destination handle's next launch makes its own, as after
 *       a call on a subset of the envs.  Telemetry, obs64 and reward64 of the last step are left alone, and the call writes no observation:
 *       the destination's current observation is the source's last observation row (it is a function of the copied state only).
 *   Clocks: a copy may give the destination another slot of day than its neighbours, so `dst` goes onto per-env clocks as after a masked
 *       call (chub_clock_groups / chub_env_clocks report the truth; chub_reset of everybody returns to one clock).  chub_copy_envs keeps
 *       `dst` in lock-step when both handles are in lock-step on the same slot of day and price phase.
 *   Handle pairs: same device, same RNG mode, same station_list / station_type_list / constant_charging, both with or both without per-env
 *       rows; without rows equal chub_config scalars; n_envs, env_id0, seed and chub_options may differ.  A scratch handle must have been
 *       reset once before it is stepped.
 *   chub_copy_envs (host index arrays) validates, uploads the indices, runs the device form and synchronises.  CHUB_ERR_ARG, with a message
 *       naming the offending position and nothing written: null arguments, count < 0, an index out of range, a destination named twice,
 *       within one handle an env that is both source and destination, incompatible handles, a source row whose FCEV arrival bound exceeds
 *       the one `dst` was created with (as chub_set_env_params).  CHUB_ERR_UNSUPPORTED: tape handles, a handle between chub_graph_begin and
 *       chub_graph_end.  count == 0 succeeds and does nothing.
 *   chub_copy_envs_device (index arrays in device memory, e.g. what a top-k on the device left) returns after enqueueing ONE gather /
 *       scatter launch on `stream`: no host synchronisation, no device read.  It checks the handles but cannot check the indices: the caller
 *       guarantees distinct destinations, within one handle no env both source and destination, and rows that fit `dst`.  A pair with an
 *       index out of range (or a source whose waiting list is longer than `dst` can hold) is skipped; destinations named twice or envs
 *       that are both end with unspecified contents, and no other env is affected.  `dst` is on per-env clocks afterwards. */
int chub_copy_envs(chub_env *dst, chub_env *src, const int64_t *src_idx, const int64_t *dst_idx, int64_t count);
int chub_copy_envs_device(chub_env *dst, chub_env *src, const int64_t *d_src_idx, const int64_t *d_dst_idx, int64_t count, void *stream);

/* electrolyser action->power table hy_power_speed_list[102] (HYD:154-157).  The reference builds it at construction
 * with 101 real hy_step()s, i.e. with live random FCEV demand, which matters whenever a tank clamp binds during that
 * sweep.  COMPAT: chub_compat_replay_constructor computes exactly that table per env from the env's streams (until
 * then, and in PHILOX mode, the table is the zero-demand sweep, one per handle: the production mode's definition).
 * chub_get_hy_table_env returns env i's table (PHILOX: the handle's; a handle with per-env parameters: the zero-demand sweep of env
 * i's row); chub_set_hy_table installs one for every env. */
int chub_get_hy_table(const chub_env *env, double *out102);
int chub_get_hy_table_env(chub_env *env, int64_t env_index, double *out102);
int chub_set_hy_table(chub_env *env, const double *in102);

const char *chub_last_error(void);
int chub_device_count(void);
/* hash of the sources this library was built from (the Python host refuses a library that is older than its sources) */
const char *chub_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* CHUB_H */
