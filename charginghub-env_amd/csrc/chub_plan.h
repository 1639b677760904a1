// chub_plan.h -- which launch forms a handle runs.  Decided once per handle from the hub shape, the batch, the RNG mode and
// chub_options (plan_handle: what chub_create_ex keeps and chub_launch_plan reports), then per reset / step from the call's
// state (plan_call).  Host-only C++, no HIP calls: chub_runtime.cpp decides with it, the launchers in chub_kernels.hip launch
// the forms it names and decide nothing themselves.
#pragma once

#include <stdint.h>

#include <algorithm>

#include "../../include/chub.h"
#include "chub_device.h"

namespace chub {

// ---- the size thresholds and the compile-time knobs behind them
#ifndef CHUB_XCD_ANY_TILE
#define CHUB_XCD_ANY_TILE 0  // (tile experiments: 1 = the second tile also takes the XCD-aware order while the streams are cache-resident)
#endif
#ifndef CHUB_SPLIT2
#define CHUB_SPLIT2 1  // the split step's slot pass with two slots per lane (slot_body_split2); 0: slot_body_compat<.., SPLIT> for every step
#endif
#ifndef CHUB_PAIR_MIN_ENVS
#define CHUB_PAIR_MIN_ENVS 8192
#endif
constexpr int64_t kBigTileSlots = (int64_t) 10 << 20;  // handles of at least this many charger slots take the second tile (chub_options.tile overrides)
constexpr int64_t kXcdOrderSlots = (int64_t) 6 << 20;  // handles of at most this many charger slots (their streams live in the caches) run their
                                                       // step kernels in XCD-aware work order
constexpr int kPipedMaxBlocks = 256;   // chub_run_steps's spans with the tails on a wave of their own, a step behind (k_steps_piped), up to this many workgroups --
                                       // one per CU: the slot waves then have nobody else's tails to overlap with.  us per step, tails on their own wave vs on
                                       // the last slot wave: 128 workgroups 4.93 vs 6.13; 192: 4.99 vs 6.12; 256: 5.00 vs 6.18 / 4.85 vs 6.40; 373: 9.40 vs 7.47;
                                       // 384: 9.73 vs 7.25 (two workgroups per CU already run one's tails beside the other's slot phases)
constexpr int kFusedMaxBlocksTailWave = 768;  // ... as k_step_tailwave (hubs of 8 piles and more: the tails on a wave of their own).  us per step as graph replays,
                                              // one launch vs two: 373 workgroups 8.15 vs 9.6; 559: 9.32 vs 10.08; 745: 9.57 vs 10.18; 1118: 14.99 vs 11.41 (up to
                                              // four workgroups of five waves are resident per CU: 1024 in all)
constexpr int kSpanMaxBlocks = 384;           // chub_run_steps's spans of steps in one launch, up to this many workgroups (745: 12.9 us per step against 11.0)
constexpr int kFusedMaxBlocks = 384;   // PHILOX lock-step steps of at most this many slot workgroups run as ONE launch (k_step_fused).  Measured, us per step
                                       // as graph replays, one launch vs two: 8.08 vs 8.82 at 128 workgroups (C2), 8.50 vs 9.30 at 256, 9.42 vs 9.79 at 373,
                                       // 10.79 vs 10.61 at 745, 11.71 vs 11.38 at 1024, 17.9 vs 13.1 at 1490
// chub_run_steps on the two-launch PHILOX step: pairs of steps whose tails share ONE launch (k_env_pair: slot(i), slot(i + 1), tails(i and i + 1)) from
// this many envs on (chub_options.span_steps overrides: 1 = never, 2 and more = at any size).  The tail launch's fixed costs -- kernel boundary, the cold start of its load burst,
// the drain of its rows -- are then paid once per two steps.  Measured, us per step as graph replays of two days, every step two launches vs pairs
// ([20, 25] hub): 8704 envs 10.35 vs 9.65; 16 384: 11.74 vs 11.40; 24 576: 14.42 vs 13.84; 32 768: 16.53 vs 15.95; 65 536: 24.62 vs 23.86 -- a gain
// at every size at which that hub's step is two launches; smaller handles on the two-launch step were not measured and keep the per-step path.
constexpr int64_t kPairMinEnvs = CHUB_PAIR_MIN_ENVS;
// Envs per walk workgroup of k_slot_walk2 (one wave walks them): 64, or -- batches of at most kWalk2HalfMaxEnvs envs -- 32: twice the walking
// waves, each with half the cars to evaluate (all 64 lanes still evaluate).  A small batch's launch lasts as long as its longest walk
// (4096 envs: 27.0 -> 22.3 us, 16 384: 31.1 -> 26.8, 32 768: 37.7 -> 33.2, 40 000: 40.4 -> 39.7); a large one is bound by instruction issue,
// where the second set of serial phases costs more than the shorter chain gives (65 536 envs: 54.6 -> 59.1 us).
constexpr int64_t kWalk2HalfMaxEnvs = 40000;

// ---- per handle (the values chub_launch_plan reports: include/chub.h, CHUB_PLAN_*)
enum PackedForm : int32_t {  // k_slot_packed: its tile, and whether a unit may span several waves (a station of more than 64 piles)
    PACKED_NONE = 0, PACKED_SMALL = 1, PACKED_SMALL_WIDE = 2, PACKED_LARGE = 3, PACKED_LARGE_WIDE = 4
};
enum OneLaunch : int32_t {  // a lock-step step as one launch; the last three are what a call with action bits or a complete tape makes of it
    ONE_NONE = 0, ONE_FUSED = 1, ONE_TAILWAVE = 2, ONE_FUSED_BITS = 3, ONE_TAILWAVE_BITS = 4, ONE_FUSED_TAPE = 5
};
enum CompatForm : int32_t {  // COMPAT resets / steps that are not k_compat_small's
    COMPAT_NONE = 0,       // (a PHILOX handle)
    COMPAT_STATIONS = 1,   // one kernel per station, the unit's first lane walking the streams
    COMPAT_SPLIT = 2,      // the split form: stream walks one env per lane, then the slots of both stations in one launch
    COMPAT_WALK2_32 = 3,   // ... whose lock-step steps run the slot pass beside the next step's walks (k_slot_walk2<.., 32>)
    COMPAT_WALK2_64 = 4    // ... with 64 envs per walk workgroup
};
enum StationKernel : int32_t {  // a station's slot kernel wherever the packed one is not used
    STATION_WAVE = 0,      // k_slot: units of at most 64 piles inside a wave
    STATION_UNIT = 1,      // k_slot_unit: a workgroup of 256 lanes per unit
    STATION_UNIT_ANY = 2,  // k_slot_unit_any: a unit of more than 256 piles walked in chunks
    STATION_CURVES = 3     // k_slot_curves (PHILOX_CURVES)
};

struct LaunchPlan {  // one int32 per CHUB_PLAN_* index, in that order
    int32_t packed;        // PackedForm: PHILOX steps run k_slot_packed
    int32_t big_tile;      // the packed kernel's tile: (kBigBlock, kBigSlotsPerLane) instead of (kPackedBlock, kSlotsPerLane)
    int32_t pblock, pslots;
    int32_t epb;           // whole envs per packed workgroup
    int32_t xcd;           // HubParams::xcd: tiles, tail and level workgroups in XCD-aware order
    int32_t one_launch;    // OneLaunch (ONE_NONE, ONE_FUSED or ONE_TAILWAVE)
    int32_t span_size_ok;  // chub_run_steps's spans of steps in one launch: few enough workgroups (or the one-launch step forced)
    int32_t span_piped;    // ... with the tails on a wave of their own, a step behind (k_steps_piped; else k_steps_fused)
    int32_t span_steps;    // chub_options.span_steps
    int32_t compat_small;  // COMPAT lock-step resets and steps as ONE launch (k_compat_small): every env fits one workgroup
    int32_t compat;        // CompatForm
    int32_t split2;        // the split form's steps take two slots per lane (k_slot_split2; stations of 8 to 64 piles)
    int32_t walk_ahead;    // lock-step split steps walk the next step's streams ahead (k_env_walk, or k_slot_walk2 by CompatForm)
    int32_t station[2];    // StationKernel of each station
};
static_assert(sizeof(LaunchPlan) == CHUB_PLAN_COUNT * sizeof(int32_t), "LaunchPlan mirrors the CHUB_PLAN_* list");

// The plan of a handle, or (CHUB_ERR_*, *msg) for the arguments and combinations chub_create_ex refuses, in the order it checks them.
inline int plan_handle(const chub_config *cfg, int64_t n_envs, int rng_mode, const chub_options &opt, LaunchPlan &p, const char **msg) {
    auto refuse = [&](int code, const char *m) {
        *msg = m;
        return code;
    };
    if (opt.slot_kernel < 0 || opt.slot_kernel > 2) return refuse(CHUB_ERR_ARG, "chub_options.slot_kernel must be 0, 1 or 2");
    if (opt.fused_step < 0 || opt.fused_step > 2) return refuse(CHUB_ERR_ARG, "chub_options.fused_step must be 0, 1 or 2");
    if (opt.tile < 0 || opt.tile > 2) return refuse(CHUB_ERR_ARG, "chub_options.tile must be 0, 1 or 2");
    if (opt.walk_ahead < 0 || opt.walk_ahead > 1) return refuse(CHUB_ERR_ARG, "chub_options.walk_ahead must be 0 or 1");
    if (opt.work_order < 0 || opt.work_order > 1) return refuse(CHUB_ERR_ARG, "chub_options.work_order must be 0 or 1");
    if (opt.span_steps < 0 || opt.span_steps > 96) return refuse(CHUB_ERR_ARG, "chub_options.span_steps must be 0 .. 96");
    if (opt.span_tails < 0 || opt.span_tails > 2)
        return refuse(CHUB_ERR_ARG, "chub_options.span_tails must be 0 (by size), 1 (on the last slot wave) or 2 (on a wave of their own)");
    if (n_envs <= 0) return refuse(CHUB_ERR_ARG, "n_envs must be positive");
    const int S0 = cfg->station_list[0], S1 = cfg->station_list[1], St = S0 + S1;
    if (n_envs * (int64_t) (St + 2) >= (int64_t) 1 << 31)
        return refuse(CHUB_ERR_UNSUPPORTED, "n_envs * (piles + 2) must stay below 2^31 per handle (32-bit slot indices)");
    if (rng_mode != CHUB_RNG_COMPAT && rng_mode != CHUB_RNG_PHILOX && rng_mode != CHUB_RNG_PHILOX_CURVES) return refuse(CHUB_ERR_ARG, "unknown rng_mode");
    // PHILOX_CURVES: PHILOX's draws and tail, the slots on k_slot_curves (chub_kernels.hip); a unit is one wave's lanes there
    const bool curves = rng_mode == CHUB_RNG_PHILOX_CURVES, compat = rng_mode == CHUB_RNG_COMPAT;
    if (curves && (S0 > 64 || S1 > 64))
        return refuse(CHUB_ERR_UNSUPPORTED, "rng_mode PHILOX_CURVES covers stations of at most 64 piles (its slot kernel keeps a station's unit inside one wave)");
    for (int k = 0; k < 2; k++) {
        if (cfg->station_list[k] < 0) return refuse(CHUB_ERR_ARG, "station_list entries must be >= 0");
        // the production (PHILOX) kernel lays whole envs over a workgroup's 512 (2048) virtual lanes; the wave-local kernels keep a unit
        // of up to 64 piles inside a wave, give a larger one a workgroup of 256 lanes (k_slot_unit) and walk a unit of more than 256
        // piles in chunks (k_slot_unit_any, whose scalar-load control ranks the whole unit in LDS: kMaxPiles)
        if (cfg->station_list[k] > kMaxPiles) return refuse(CHUB_ERR_UNSUPPORTED, "more than 4096 piles per station is not supported");
        if (cfg->station_type_list[k] != CHUB_FAST && cfg->station_type_list[k] != CHUB_SLOW)
            return refuse(CHUB_ERR_ARG, "EVS type must be fast or slow");  // AGG:196
    }
    if (St < 1) return refuse(CHUB_ERR_ARG, "A station must have fast pile or slow pile!");  // MGR:336
    const bool small_units = S0 <= 64 && S1 <= 64;
    for (int k = 0; k < 2; k++) {
        const int S = cfg->station_list[k];
        p.station[k] = curves ? STATION_CURVES : S > 256 ? STATION_UNIT_ANY : S > 64 ? STATION_UNIT : STATION_WAVE;
    }

    // packed slot kernel (k_slot_packed): the workgroup's virtual lanes laid over whole envs end to end.  The workgroup tile: the small one
    // while state and action rows live in the caches, the large one once they stream from HBM (a hub too large for the small tile's 512
    // virtual lanes -- stations of several hundred piles -- still fits the large one's 2048)
    const int64_t slots = n_envs * (int64_t) St;
    p.big_tile = (opt.tile == 2 || (opt.tile == 0 && (slots >= kBigTileSlots || St > kPackedBlock * kSlotsPerLane))) ? 1 : 0;
    p.pblock = p.big_tile ? kBigBlock : kPackedBlock;
    p.pslots = p.big_tile ? kBigSlotsPerLane : kSlotsPerLane;
    // ... and the work order: XCD-aware while the streams are cache-resident (measured: 4-6 % of the step; HBM-resident sizes lose 1 %)
    p.xcd = (opt.work_order == 0 && (!p.big_tile || CHUB_XCD_ANY_TILE) && slots <= kXcdOrderSlots) ? 1 : 0;
    const int pb = p.pblock * p.pslots;
    p.epb = pb / St > 0 ? pb / St : 1;
    if (p.epb > pb / 4) p.epb = pb / 4;  // the workgroup's per-unit LDS areas hold 2 * pb / 4 units: hubs of 1-3 piles leave lanes idle
    bool magic_ok = true;  // the kernel divides lane numbers by S0 + S1 with a 20-bit reciprocal
    for (int l = 0; l < pb && magic_ok; l++)
        if ((((uint32_t) l * ((1u << 20) / (uint32_t) St + 1u)) >> 20) != (uint32_t) (l / St)) magic_ok = false;
    const bool packed = rng_mode == CHUB_RNG_PHILOX && St <= pb && magic_ok &&
                        (uint64_t) n_envs * (uint64_t) (St + 2) * 16u < ((uint64_t) 1 << 32) &&  // 32-bit byte offsets
                        opt.slot_kernel != 1;  // (PHILOX_CURVES: k_slot_curves whatever the options say)
    // (the kernel instance goes by the block size: the two tiles may share one under KFLAGS)
    const bool large = p.pblock == kBigBlock;
    p.packed = !packed ? PACKED_NONE : large ? (small_units ? PACKED_LARGE : PACKED_LARGE_WIDE) : (small_units ? PACKED_SMALL : PACKED_SMALL_WIDE);

    // the whole step as one launch: where the two kernels are launch- and latency-bound and every workgroup finds room at once
    const int64_t nb = (n_envs + p.epb - 1) / p.epb;
    const bool can = packed && small_units && p.pblock == kPackedBlock;
    const bool fused = can && (opt.fused_step == 2 || (opt.fused_step == 0 && nb <= (p.epb <= 64 ? kFusedMaxBlocksTailWave : kFusedMaxBlocks)));
    p.one_launch = !fused ? ONE_NONE : p.epb <= 64 ? ONE_TAILWAVE : ONE_FUSED;  // (the tail wave's lanes are the workgroup's envs)
    p.span_size_ok = (nb <= kSpanMaxBlocks || opt.fused_step == 2) ? 1 : 0;
    // chub_run_steps's spans: the tails on a wave of their own, a step behind the slot waves (k_steps_piped) -- its 64 lanes are the workgroup's envs
    const bool can_pipe = p.one_launch == ONE_TAILWAVE;
    p.span_piped = (can_pipe && (opt.span_tails == 2 || (opt.span_tails == 0 && nb <= kPipedMaxBlocks))) ? 1 : 0;
    p.span_steps = opt.span_steps;

    // the reference-exact mode at a handful of envs (the drop-in class: one): both station passes and the tail in one launch
    const int U0 = S0 > 0 ? (S0 < 64 ? S0 : 64) : 1, U1 = S1 > 0 ? (S1 < 64 ? S1 : 64) : 1;  // HubParams::U
    const int64_t fit = std::min<int64_t>(64, std::min<int64_t>(kCompatSmallWaves0 * (64 / U0), kCompatSmallWaves1 * (64 / U1)));
    p.compat_small = (compat && opt.fused_step != 1 && small_units && n_envs <= fit) ? 1 : 0;
    // ... and everything else as the split step (stream walks, one env per lane -> slots of both stations in one launch) unless
    // slot_kernel = 1 asks for one kernel per station with the unit's first lane walking (the parity cross-check).  Measured, us per
    // step, split vs per station: 47.1 vs 51.1 at 1024 envs, 49.7 vs 50.9 at 4096, 54 vs 70 at 8192, 100 vs 279 at 65 536 ([20, 25] hub)
    const bool split = compat && small_units && opt.slot_kernel != 1;
    p.split2 = (split && CHUB_SPLIT2 && U0 >= 8 && U1 >= 8) ? 1 : 0;  // (at most 8 units per virtual wave of 128 lanes)
    p.walk_ahead = (split && opt.walk_ahead == 0) ? 1 : 0;
    const bool walk2 = p.walk_ahead && p.split2 && !p.compat_small;
    p.compat = !compat ? COMPAT_NONE : !split ? COMPAT_STATIONS : !walk2 ? COMPAT_SPLIT : n_envs <= kWalk2HalfMaxEnvs ? COMPAT_WALK2_32 : COMPAT_WALK2_64;

    if (opt.fused_step == 2 && !can)
        return refuse(CHUB_ERR_UNSUPPORTED, "fused_step = 2: the single-launch step covers PHILOX handles on the packed slot kernel with "
                                            "stations of at most 64 piles");
    if (opt.span_tails == 2 && !can_pipe)
        return refuse(CHUB_ERR_UNSUPPORTED, "span_tails = 2: the tail wave of a span covers handles on the one-launch step (fused_step) with at most 64 envs "
                                            "per workgroup (hubs of 8 piles and more)");
    return CHUB_OK;
}

// ... and what becomes of that plan on a handle with per-env hub parameters (chub_create_params).  The tail k_env<.., ENV_PARAMS> reads each
// env's constants: the forms that carry a tail of their own (k_step_fused / k_step_tailwave, the spans of chub_run_steps, k_compat_small) are not
// built for that, so such a handle runs the two-launch step whatever the options say.  COMPAT: one kernel per station, the unit's first lane
// walking the streams and the tail drawing the forecourt, at every batch size (the split step's walks read the per-handle FCEV counts).
inline int plan_params(LaunchPlan &p, int rng_mode, const char **msg) {
    (void) msg;
    if (rng_mode == CHUB_RNG_COMPAT) {
        p.compat = COMPAT_STATIONS;
        p.compat_small = 0;
        p.split2 = 0;
        p.walk_ahead = 0;
    }
    p.one_launch = ONE_NONE;
    p.span_size_ok = 0;
    p.span_piped = 0;
    return CHUB_OK;
}

// ---- pairs of steps whose tails share one launch (chub_run_steps; k_env_pair in chub_kernels.hip)
// per handle: the form exists for it -- its slot launch decodes the second step's raw draws in the unit pass of the lock-step small tile, its tail
// is the homogeneous PHILOX tail, its step is two launches (a handle on the one-launch step sends whole spans out as one launch) -- and is wanted:
// chub_options.span_steps, which bounds the steps per tail launch here as it bounds the steps per launch there, is 0 (by size) or at least 2
inline bool plan_pair_handle(const LaunchPlan &p, int64_t n_envs, const chub_options &opt, bool env_params) {
    if (p.packed != PACKED_SMALL || p.one_launch != ONE_NONE || env_params || opt.span_steps == 1) return false;
    return opt.span_steps >= 2 || n_envs >= kPairMinEnvs;
}
// per call of chub_run_steps: lock-step steps of every env into the packed blocks and nothing else that reads a step's tail before the next
// step's slot launch, or between the two
struct PairState {
    bool comm;         // a communicator gathers every step's block
    bool per_env;      // the handle runs on per-env clocks
    bool tape;         // a tape handle
    bool outputs;      // step terms, the episode ledger or telemetry are attached
    bool profiling;    // the per-kernel profiler samples step launches
};
inline bool plan_pair_call(bool handle_pairs, const PairState &c) {
    return handle_pairs && !c.comm && !c.per_env && !c.tape && !c.outputs && !c.profiling;
}
// how many of the next `left` steps of a call go out as pairs when the handle's clock shows slot t of the day: pairs never straddle the day's
// end or the call's; an odd step out goes by the per-step path
inline int64_t pair_steps(int t, int64_t left) {
    const int64_t day = 96 - t;
    const int64_t k = left < day ? left : day;
    return k > 0 ? k & ~(int64_t) 1 : 0;
}

// ---- per call
enum CallForm : int32_t {  // the kernel sequence of one reset / step
    CALL_COMPAT_SMALL,     // k_compat_small: both station passes and the tail
    CALL_ONE_LAUNCH,       // k_step_fused / k_step_tailwave (CallPlan::one)
    CALL_SLOT_WALK2,       // k_slot_walk2: the slot pass beside the next step's stream walks, then the tails
    CALL_SLOT_ENV_WALK,    // the slot pass (CallPlan::slot), then the tails beside the next step's stream walks (k_env_walk)
    CALL_SLOT_ENV          // the slot pass (CallPlan::slot), then the tails (CallPlan::env)
};
enum SlotForm : int32_t {  // what launch_slot runs
    SLOT_PACKED, SLOT_PACKED_MASKED, SLOT_PACKED_TAPE, SLOT_PACKED_BITS,  // k_slot_packed
    SLOT_CURVES,           // k_slot_curves, both stations in one launch
    SLOT_WAVE,             // PHILOX k_slot, both stations in one launch
    SLOT_STATIONS,         // PHILOX, one launch per station (LaunchPlan::station)
    SLOT_SPLIT,            // COMPAT split form: k_compat_walk -> k_slot_split
    SLOT_SPLIT2,           // ... -> k_slot_split2
    SLOT_COMPAT_STATIONS   // COMPAT, one launch per station
};
enum LevelsForm : int32_t { LEVELS_NONE, LEVELS_DRAW, LEVELS_RESET };  // PHILOX station draws in front: k_draw_levels / k_reset_levels
enum EnvForm : int32_t { ENV_PHILOX, ENV_PHILOX_CLOCKS, ENV_PHILOX_TAPE, ENV_COMPAT, ENV_COMPAT_CLOCKS,  // k_env: mode, per-env clocks, tail tape,
                         ENV_PHILOX_PARAMS, ENV_PHILOX_PARAMS_CLOCKS, ENV_COMPAT_PARAMS, ENV_COMPAT_PARAMS_CLOCKS };  // per-env hub parameters

struct CallState {
    bool reset, load_mode;
    bool per_env;      // the handle runs on per-env clocks
    bool all_served;   // the call serves every env (no mask)
    bool capturing;
    bool car_tape, pk_tape, tail_tape;
    bool bits;         // one bit per pile (chub_step_bits*)
    bool fresh;        // the call makes its own state-independent draws (StepArgs::fresh)
    bool env_params;   // the handle has per-env hub parameters (plan_params)
    bool dev_mask;     // the call's mask lives in device memory and the host never sees it (chub_dmask_*_device, the reset of
                       // chub_autoreset_step_device): per-env clocks and the masked forms whatever the mask holds, over the whole env range
};
struct CallPlan {
    CallForm call;
    OneLaunch one;
    SlotForm slot;
    LevelsForm levels;
    EnvForm env;
};

inline bool slot_form_split(SlotForm f) { return f == SLOT_SPLIT || f == SLOT_SPLIT2; }

// the slot pass of a reset or step that runs one (the COMPAT constructor's reset of every env included)
inline SlotForm slot_form(const LaunchPlan &p, const CallState &c) {
    if (p.station[0] == STATION_CURVES) return SLOT_CURVES;
    if (p.packed != PACKED_NONE && !c.load_mode)
        return c.car_tape ? SLOT_PACKED_TAPE : c.bits && !c.reset ? SLOT_PACKED_BITS : !c.all_served ? SLOT_PACKED_MASKED : SLOT_PACKED;
    switch ((CompatForm) p.compat) {
    case COMPAT_NONE: return (p.station[0] == STATION_WAVE && p.station[1] == STATION_WAVE) ? SLOT_WAVE : SLOT_STATIONS;
    case COMPAT_STATIONS: return SLOT_COMPAT_STATIONS;
    default: return (p.split2 && !c.reset && !c.load_mode) ? SLOT_SPLIT2 : SLOT_SPLIT;
    }
}

// CallPlan::slot, levels and env are those of the CALL_SLOT_* forms
inline CallPlan plan_call(const LaunchPlan &p, const CallState &c_in) {
    CallState c = c_in;
    if (c.dev_mask) {  // nobody knows whether the mask names everybody: it never does, as far as the forms go
        c.per_env = true;
        c.all_served = false;
    }
    CallPlan r = {CALL_SLOT_ENV, ONE_NONE, SLOT_WAVE, LEVELS_NONE, ENV_PHILOX};
    const bool compat = p.compat != COMPAT_NONE, lock_step = !c.load_mode && !c.per_env;
    if (p.compat_small && !c.per_env && (c.reset || !c.load_mode)) {
        r.call = CALL_COMPAT_SMALL;
        return r;
    }
    // (tape mode: the one-launch form replays only a complete tape -- station draws, car variates and the tail's variates)
    if (!c.reset && p.one_launch != ONE_NONE && lock_step && ((!c.car_tape && !c.pk_tape) || (c.car_tape && c.pk_tape && c.tail_tape))) {
        r.call = CALL_ONE_LAUNCH;
        r.one = c.tail_tape ? ONE_FUSED_TAPE : !c.bits ? (OneLaunch) p.one_launch : p.one_launch == ONE_TAILWAVE ? ONE_TAILWAVE_BITS : ONE_FUSED_BITS;
        r.levels = (c.fresh || c.pk_tape) ? LEVELS_DRAW : LEVELS_NONE;
        return r;
    }
    r.slot = slot_form(p, c);
    r.env = compat ? (c.env_params ? (c.per_env ? ENV_COMPAT_PARAMS_CLOCKS : ENV_COMPAT_PARAMS) : c.per_env ? ENV_COMPAT_CLOCKS : ENV_COMPAT)
          : c.tail_tape ? ENV_PHILOX_TAPE
          : c.env_params ? (c.per_env ? ENV_PHILOX_PARAMS_CLOCKS : ENV_PHILOX_PARAMS) : c.per_env ? ENV_PHILOX_CLOCKS : ENV_PHILOX;
    // lock-step split steps of every env walk the next step's streams ahead: beside this step's slot pass (k_slot_walk2), or its tails
    const bool ahead = !c.reset && slot_form_split(r.slot) && c.all_served && !c.per_env;
    if (ahead && !c.load_mode && !c.capturing && (p.compat == COMPAT_WALK2_32 || p.compat == COMPAT_WALK2_64)) {
        r.call = CALL_SLOT_WALK2;
        r.slot = SLOT_SPLIT2;
    } else if (ahead && p.walk_ahead) {
        r.call = CALL_SLOT_ENV_WALK;
    }
    if (!compat) {  // PHILOX: the station draws in front of the slot pass (tape: the caller's occupancy draws are in pk already)
        if (!c.reset) r.levels = (c.fresh || c.pk_tape) ? LEVELS_DRAW : LEVELS_NONE;
        else r.levels = (r.slot == SLOT_WAVE || r.slot == SLOT_STATIONS || !c.car_tape) ? LEVELS_RESET : LEVELS_NONE;
    }
    return r;
}

}  // namespace chub
