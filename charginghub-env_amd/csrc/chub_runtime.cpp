// chub_runtime.cpp -- host side of libchub.so: the C ABI of include/chub.h, table construction at
// create time, HBM state ownership and kernel launches.  No simulation arithmetic of the step runs on
// the host; what does run here is init-time table building (arrival CDF parsing with the reference's
// own parser, level thresholds, the electrolyser action->power sweep, price statistics).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/chub.h"
#include "chub_device.h"
#include "chub_plan.h"
#include "chub_policy.h"
#include "chub_gae.h"
#include "chub_critic.h"
#include "chub_adam.h"
#include "chub_trainlog.h"
#include "chub_lagrange.h"
#include "chub_retnorm.h"

namespace chub {
template <bool RESET>
void launch_slot(const CallPlan &cp, const HubParams &hp, const LaunchPlan &lp, const DevCtx *ctx, const StepArgs &sa, hipStream_t stream,
                 const PackedPtrs &pp, hipEvent_t ev0, hipEvent_t ev1);
void launch_check_ttab(const DevCtx *ctx, uint32_t *d_mismatch, hipStream_t stream);
void launch_build_cls_soc(const DevCtx *ctx, float *d_out, hipStream_t stream);
void launch_pile_obs(const HubParams &hp, const DevCtx *ctx, uint32_t fields, const uint8_t *d_mask, const float *d_cls_soc, float *d_out,
                     hipStream_t stream);
void launch_pile_set(const HubParams &hp, const DevCtx *ctx, int which, const uint8_t *d_mask, uint64_t *d_bits, hipStream_t stream);
void launch_station_profile(const HubParams &hp, const DevCtx *ctx, uint32_t fields, int buckets, const uint8_t *d_mask, const float *d_cls_soc,
                            float *d_out, hipStream_t stream);
void launch_load_dispatch(const HubParams &hp, const DevCtx *ctx, int units, const uint8_t *d_mask, const float *d_cls_soc, const float *d_loads,
                          const float *d_tail, float *d_actions, uint64_t *d_bits, hipStream_t stream);
void launch_forecast(const HubParams &hp, const DevCtx *ctx, const ForecastTabs &ft, uint32_t fields, int horizon, int t, const uint16_t *d_clk,
                     const uint8_t *d_mask, float *d_out, hipStream_t stream);
template <typename OUT>
void launch_step_terms(const HubParams &hp, const DevCtx *ctx, uint32_t fields, const uint8_t *d_mask, OUT *d_out, hipStream_t stream);
template <bool RESET>
void launch_env(EnvForm f, const HubParams &hp, const DevCtx *ctx, const StepArgs &sa, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1,
                const PackedPtrs &pp);
void launch_random_actions(const HubParams &hp, uint64_t key, uint32_t batch, float *d_actions, hipStream_t stream);
void launch_compat_ctor_sweep(const HubParams &hp, const DevCtx *ctx, int rng_cur, hipStream_t stream, bool env_params);
void launch_tick_advance(uint32_t *tick_base, uint32_t by, hipStream_t stream);
void launch_fill_clocks(uint16_t *dst, int64_t n, uint16_t value, hipStream_t stream);
void launch_keep_clocks(uint16_t *dst, const uint16_t *src, int64_t n, hipStream_t stream);
void launch_expand_bits(const HubParams &hp, const uint64_t *d_bits, const float *d_tail, float *d_actions, hipStream_t stream);
void launch_copy_envs(int layout, const CopyArgs &a, hipStream_t stream);
void launch_episode_summary(const HubParams &hp, const DevCtx *ctx, double *d_partials, double *d_out, int drain, hipStream_t stream);
void launch_step_fused(const CallPlan &cp, const HubParams &hp, const DevCtx *ctx, const StepArgs &sa, hipStream_t stream, const PackedPtrs &pp,
                       hipEvent_t ev0, hipEvent_t ev1);
template <bool RESET>
void launch_compat_small(const HubParams &hp, const DevCtx *ctx, const StepArgs &sa, hipStream_t stream, const PackedPtrs &pp);
void launch_steps_fused(const HubParams &hp, const LaunchPlan &lp, const DevCtx *ctx, const StepArgs &sa, hipStream_t stream, const PackedPtrs &pp,
                        int n_steps, int pc0, int64_t first, const float *const *batches, int n_batches, float *const *packed2);
void launch_slot_walk2(const LaunchPlan &lp, const HubParams &hp, const DevCtx *ctx, const StepArgs &sa, const StepArgs &sw, hipStream_t stream,
                       hipEvent_t ev0, hipEvent_t ev1);
void launch_env_walk(const HubParams &hp, const DevCtx *ctx, const StepArgs &sa, const StepArgs &sw, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1,
                     const PackedPtrs &pp);
void launch_pair(const HubParams &hp, const DevCtx *ctx, const StepArgs &sa, const StepArgs &sb, hipStream_t stream, const PackedPtrs &pp,
                 const PairBufs &pb, int sel, bool chain_start, bool more);
}  // namespace chub

using namespace chub;

static thread_local std::string g_err;

static int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
// an entry point that is not built for handles with per-env hub parameters (include/chub.h: chub_create_params)
static int refuse_params(const char *what) {
    return fail(CHUB_ERR_UNSUPPORTED, std::string(what) + " is not supported on a handle with per-env hub parameters (chub_create_params)");
}
// for the other translation units of the library (chub_comm.cpp); not part of the ABI
extern "C" __attribute__((visibility("hidden"))) int chub_set_last_error_(int code, const char *msg) { return fail(code, msg); }

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(CHUB_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));               \
    } while (0)

// The handle holds what outlives a call: configuration, device state, clocks, staging.  What ONE reset or step was asked to do -- its mask,
// actions or bits, variates, tapes, outputs -- travels as a StepCall (below), never as a field here.
struct chub_env {
    chub_config cfg;
    HubParams hp;
    SlotArrays sl;
    StationArrays st;
    EnvArrays ev;
    CompatRng cr;
    Tables tb;
    int device;
    LaunchPlan plan;           // the launch forms of this handle (chub_plan.h)
    // chub_run_steps sends pairs of steps out with one tail launch (plan_pair_handle): what a pair keeps apart from the handle's arrays, ONE block
    // outside the arena -- scratch: every chain of pairs fills what it reads, no snapshot carries it, no copy moves it
    bool pair_tails = false;
    PairBufs pair = {};
    char *d_pair = nullptr;
    int rng_cur = 0;           // COMPAT: which of CompatRng's three buffers holds the committed streams (moved on by every commit: chub_device.h)
    uint32_t walked_tick = 0;  // COMPAT split step: the tick whose stream walk has run already, beside the previous step's tails (0: none)
    uint32_t e2_tick = ~0u;    // ... and the tick of the pass after which StationArrays::empt2 holds every unit's count (what a walk two steps ahead needs)
    bool empt_valid;    // COMPAT, split step: StationArrays::empt holds every unit's empty-slot count for the next step (left by the last split pass)
    DevCtx *d_ctx;      // device copy of {hp, sl, st, ev, cr, tb}
    bool ctx_dirty;
    // lock-step clock (MGR:137-140,299; CHS.hpp:1204; AGG:150-151; HYD:192-193 are three copies of it)
    int t;
    int price_count;
    uint32_t tick;             // Philox tick: +1 per launched reset / step (one per clock group and call)
    // per-env clocks (chub_reset_envs / chub_step_envs): once a call names a subset of the envs, the clock is per-env device
    // state (StepArgs::env_clk) and the lock-step clock above is unused -- until everybody is reset again
    bool per_env;
    uint16_t *d_env_clk;            // [2][N], in the arena
    uint8_t *d_mask;                // [2][N], in the arena: the masks of the last two masked calls (the launches in flight read them)
    uint8_t *h_mask;                // [2][N] pinned staging for them
    hipEvent_t mask_done[2];        // recorded behind the launches that read d_mask[i]
    uint32_t mask_seq;
    // device masks and auto-reset (chub_dmask_*_device, chub_autoreset_step_device): the host never sees such a mask, so the launches note on
    // the device whom they served; chub_env_clocks and chub_get_state (which synchronise anyway) fold that into h_tick
    uint32_t *d_tick_note = nullptr;   // [N], in the arena: the true tick of the last device-mask launch that served the env (0: none)
    uint8_t *d_done_mask = nullptr;    // [2][N], in the arena: the done masks of the last two auto-reset calls (the reset launches read them)
    uint32_t *d_done_count = nullptr;  // [2][16]: how many envs each of them names
    uint32_t done_seq = 0;
    // a capture on per-env clocks: every masked call gets a device mask of its own (owned by the graph: a replay reads no host
    // memory), and the capture notes which launch of it served each env last (chub_env_clocks after a replay)
    std::vector<void *> cap_masks;
    std::vector<uint32_t> cap_rel;  // [N] launch number (1-based) within the capture of the env's last masked launch, 0 = none
    uint32_t cap_full_rel;          // launch number of the capture's last launch that served every env, 0 = none
    bool graph_per_env0;
    uint32_t graph_full_tick0;
    std::vector<uint32_t> graph_h_tick0;
    std::vector<uint32_t> h_tick;   // [N] tick of the last launch that served the env through a mask (chub_env_clocks)
    uint32_t full_tick;             // tick of the last launch that served every env
    bool predrawn;                  // the last launch served every env: its level blocks left the next step's state-independent draws
    double price[96];
    double hy_table[102];
    std::vector<void *> allocs;
    // all state and tables live in ONE device allocation (carved 256-B aligned): a few large pages instead of ~60
    // scattered small buffers, so the latency-bound kernels do not start with a TLB miss per array
    char *arena;
    size_t arena_size, arena_used;
    // staging for the host-pointer entry points
    float *d_actions, *d_obs, *d_reward;
    uint8_t *d_done;
    double *d_exo_z;
    int32_t *d_exo_days;
    hipStream_t stream;
    // host-pointer entry points: pinned staging + a private stream (lazily made by host_path_init)
    hipStream_t host_stream;
    hipStream_t upload_stream;    // uploads that must stay outside a capture in progress (masks of captured calls)
    float *h_actions, *h_packed;  // pinned: [N][A], [N][D+2]
    uint64_t *h_bits, *d_bits;    // chub_step_bits: [N][ceil(S / 64)] pinned staging and its device copy
    float *h_tail, *d_tail;       //                 [N][2]
    float *d_packed;              // [N][D+2]
    double *h_telem;    // telemetry block in pinned host memory, written by the tail kernel directly: telem [T][N], obs64 [N][D], reward64 [N]
                        // (handles of a few envs: the drop-in class); larger handles keep the block in device memory:
    double *d_telem = nullptr;
    int tape_classes;   // PHILOX tape mode: caller-registered arrival-SoC classes so far
    bool tape_stale = false;  // chub_tape_clear_soc since the last reset: the slots may hold cars of classes that are gone
    // per-env hub parameters (chub_create_params): DevCtx::ep, EnvArrays::hy_env and the raw rows live in the arena (snapshots carry them)
    bool env_params = false;
    chub_env_params *d_rows = nullptr;  // [N] the rows as the caller gave them (chub_get_env_params)
    int hv_max_arrive = 0;              // FCEV arrivals per step at most, over the rows at create: sizes qcap / hv_w (chub_set_env_params keeps below it)
    int hv_top[96];                     // the largest arrival index of each slot of the day (what that bound is computed from)
    EnvParamArrays ep = {nullptr, nullptr, nullptr};
    // the per-episode ledger (chub_set_episode_stats): DevCtx::es points into ONE block outside the arena, allocated when the ledger is first
    // switched on -- live [kEpCount][N] f64, finished [kEpCount][N] f64, episodes [N] u32, pending [N] u8 -- which snapshots carry behind the arena
    EpisodeArrays es = {0, 0, nullptr, nullptr, nullptr, nullptr};
    char *d_ledger = nullptr;
    // chub_pile_obs_device, PHILOX: [2][kSocLevels][kClsRow] f32, a class's SoC after n car_steps (k_build_cls_soc, at create and when a tape
    // registers classes).  Derived data outside the arena: no snapshot carries it, no copy moves it
    float *d_cls_soc = nullptr;
    // chub_forecast_device: the mean arrival counts per slot of day and, with per-env rows, the histogram of the FCEV arrival index (one block, built
    // on the host at create beside cnt / cnt_hv / hv_idx).  Derived data outside the arena, as d_cls_soc
    ForecastTabs fc = {nullptr, nullptr, nullptr};
    // chub_set_step_terms: the caller's [N][C] f32 buffer every step call fills behind its kernels (run_call), and its field mask; null / 0: none
    float *st_out = nullptr;
    uint32_t st_fields = 0;
    // the actors made for this handle (chub_policy_create): destroyed before it.  Everything they own lies outside the arena
    std::vector<chub_policy *> policies;
    // the running feature statistics made for this handle (chub_moments_create): destroyed before it, state and partials outside the arena
    std::vector<chub_moments *> moments;
    // the critics made for this handle (chub_critic_create): destroyed before it, weights and workspace outside the arena
    std::vector<chub_critic *> critics;
    // the training logs made for this handle (chub_train_log_create): destroyed before it, words, gate and stats blocks outside the arena
    std::vector<chub_train_log *> train_logs;
    // the constraint objects made for this handle (chub_lagrange_create): destroyed before it, multipliers, stats and partials outside the arena
    std::vector<chub_lagrange *> lagranges;
    // the reward scalers made for this handle (chub_return_norm_create): destroyed before it, state, scale, carry and partials outside the arena
    std::vector<chub_return_norm *> return_norms;
    // chub_rollout_gae_device's statistics: the workgroups' partials [ceil(N / 256)][3] f64, allocated at create outside the arena (derived
    // scratch: no snapshot carries it).  One buffer: calls that ask for d_stats must be ordered against each other
    double *d_gae_part = nullptr;
    double *d_ep_sum = nullptr;  // k_episode_summary's partials [kEpSumMaxBlocks][kEpSumWords], then the host form's result [kEpSumWords]
    int public_mode = 0;     // the rng_mode the handle was created with: CHUB_RNG_PHILOX_CURVES is hp.rng_mode = PHILOX + hp.soc_curves
    bool tape_only = false;  // ... and once there are any, the handle's class rows are the caller's: only tape resets / steps may admit cars
    uint32_t h_late8[8];
    double h_sin96[96];
    std::vector<float> h_ttab[2];  // host copy of Tables::ttab (chub_tape_register_soc: the longest target time)
    uint32_t *d_tick_base;     // see HubParams::tick_base
    uint32_t graph_base;       // host mirror of *d_tick_base: ticks covered by the graph replays so far
    uint32_t graph_tick0;      // host state at chub_graph_begin (restored at chub_graph_end: a capture runs nothing)
    int graph_t0, graph_pc0;
    bool graph_predrawn0;
    bool capturing;
    chub_comm *cap_comm = nullptr;  // the communicator whose gathers the capture in progress holds (chub_step_gather)
    // optional per-kernel timing with HIP events on the launch stream (chub_profile_*)
    std::vector<hipEvent_t> prof_events;
    size_t prof_used, prof_cap;
    int prof_every, prof_phase;
    bool prof_on;
};

// ------------------------------------------------------------------------------- data loading
// Read2Vector::string_to_float (CHS.hpp:138-155): f32 accumulator, `d *= 0.1` is an f64 product narrowed
// to f32.  Not correctly rounded -- and that changes 79 of the 96 000 arrival-table cells, so it is kept.
static float parse_cell(const char *s, int len) {
    int i = 0;
    float sum = 0;
    while (i < len && s[i] != '.') {
        sum = sum * 10.0f + (float) s[i] - 48.0f;
        ++i;
    }
    ++i;
    float d = 1;
    while (i < len) {
        d = (float) ((double) d * 0.1);
        float t = (float) (s[i] - '0');
        sum = sum + t * d;
        ++i;
    }
    return sum;
}

// Read2Vector::read + file_to_string (CHS.hpp:96-136): keep digits and '.', split on ','
static int load_cdf(const std::string &path, std::vector<float> &cdf) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return fail(CHUB_ERR_DATA, "cannot open " + path);
    std::string cur;
    std::vector<float> row;
    cdf.clear();
    int rows = 0;
    int c;
    auto flush_cell = [&]() {
        if (!cur.empty()) {
            row.push_back(parse_cell(cur.data(), (int) cur.size()));
            cur.clear();
        }
    };
    bool bad = false;
    auto flush_row = [&]() {
        flush_cell();
        if (!row.empty()) {
            if (row.size() != 301) bad = true;
            cdf.insert(cdf.end(), row.begin(), row.end());
            row.clear();
            rows++;
        }
    };
    while ((c = fgetc(f)) != EOF) {
        if ((c >= '0' && c <= '9') || c == '.') cur.push_back((char) c);
        else if (c == ',') flush_cell();
        else if (c == '\n') flush_row();
    }
    flush_row();
    fclose(f);
    if (bad || rows != 96) return fail(CHUB_ERR_DATA, path + ": expected 96 rows x 301 columns");
    return 0;
}

static int load_f64(const std::string &path, double *dst, size_t count) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return fail(CHUB_ERR_DATA, "cannot open " + path);
    size_t got = fread(dst, sizeof(double), count, f);
    int extra = fgetc(f);
    fclose(f);
    if (got != count || extra != EOF) return fail(CHUB_ERR_DATA, path + ": wrong size");
    return 0;
}

// RandomUtil::uniform_rand(0,1) at level k (CHS.hpp:35-44)
static float level_value(int k) {
    float tr = (float) k / 999.0f;
    tr = tr * (1.0f - 0.0f) + 0.0f;
    return tr;
}

// numpy pairwise sum of 96 values (np.mean / np.std, MGR:45-46)
static double np_sum96(const double *a) {
    double r[8];
    for (int j = 0; j < 8; j++) r[j] = a[j];
    for (int i = 8; i < 96; i += 8)
        for (int j = 0; j < 8; j++) r[j] += a[i + j];
    return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
}

template <typename T>
static int dev_alloc(chub_env *e, T **p, size_t count, bool zero = true) {
    const size_t bytes = ((count ? count : 1) * sizeof(T) + 255) & ~(size_t) 255;
    void *q = nullptr;
    if (e->arena && e->arena_used + bytes <= e->arena_size) {
        q = e->arena + e->arena_used;
        e->arena_used += bytes;
    } else {
        HIP_TRY(hipMalloc(&q, bytes));
        e->allocs.push_back(q);
    }
    if (zero) HIP_TRY(hipMemset(q, 0, bytes));
    *p = (T *) q;
    return 0;
}

template <typename T>
static int dev_upload(chub_env *e, const T **p, const std::vector<T> &v) {
    T *q = nullptr;
    int rc = dev_alloc(e, &q, v.size(), false);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(q, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *p = q;
    return 0;
}

static int pow2_ge(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// The hub constants that follow from the eight scalar constructor kwargs (hydrogen system HYD:94-98, 144, 10-24, 57-72; fluctuations
// REN:38-49, MGR:354-357): chub_create_ex derives the handle's with it, chub_create_params / chub_set_env_params each env's
struct EnvConsts {
    double v_h_max, cells, rc_cells, cap_mass, rc_cap_mass, init_soc, hydro_loss, fc_max_power, renew_fluct1, price_fluct1;
    float hv_rate;  // f32(f32(0.3) * f32(permeate)), permeate > 1 -> 0.01 (the reference's quirk)
};
static double hub_v_M() { return 0.082 * (273 + 25) / 1; }
static EnvConsts derive_env_consts(double hydro_prod_rate, double hydro_store_vlt, double init_soc, double fc_max_power, double fcev_permeate,
                                   double renew_fluctuate, double price_fluctuate, double hydro_loss) {
    EnvConsts k;
    k.cap_mass = (0.089 * (200 / 1)) * (hydro_store_vlt * 1000);
    k.v_h_max = 0.089 * hydro_prod_rate * 1000 / 3600;
    k.init_soc = init_soc;
    k.hydro_loss = hydro_loss;
    k.fc_max_power = fc_max_power;
    {
        double v_H_L = (10.0 / 1000) / 60;
        double v_H_mol = v_H_L / hub_v_M();
        double v_H_mass = v_H_mol * 2.02;
        k.cells = ceil(k.v_h_max / v_H_mass);
    }
    k.rc_cells = k.cells != 0.0 ? 1.0 / k.cells : 0.0;
    k.rc_cap_mass = 1.0 / k.cap_mass;
    k.renew_fluct1 = 1 + renew_fluctuate;
    k.price_fluct1 = 1 + price_fluctuate;
    float hv_pin = (float) 0.3, hv_perm = (float) fcev_permeate;
    if (hv_perm > 1) hv_perm = (float) 0.01;
    k.hv_rate = hv_pin * hv_perm;
    return k;
}
static EnvConsts derive_env_consts(const chub_config &c) {
    return derive_env_consts(c.hydro_prod_rate, c.hydro_store_vlt, c.init_soc, c.fc_max_power, c.fcev_permeate, c.renew_fluctuate, c.price_fluctuate,
                             c.hydro_loss);
}
static EnvConsts derive_env_consts(const chub_env_params &r) {
    return derive_env_consts(r.hydro_prod_rate, r.hydro_store_vlt, r.init_soc, r.fc_max_power, r.fcev_permeate, r.renew_fluctuate, r.price_fluctuate,
                             r.hydro_loss);
}
// what chub_create_ex refuses of its eight scalars (HYD:137); `where` names the env of a per-env row
static int check_scalars(double init_soc, double hydro_prod_rate, double hydro_store_vlt, double fc_max_power, const std::string &where) {
    if (!(init_soc >= 0.1 && init_soc <= 1)) return fail(CHUB_ERR_ARG, "init_soc must be in [0.1, 1]" + where);
    if (!(hydro_prod_rate >= 0) || !(hydro_store_vlt > 0) || !(fc_max_power >= 0))
        return fail(CHUB_ERR_ARG, "hydrogen system sizes must be non-negative" + where);
    return CHUB_OK;
}
// FCEV arrivals per step at most for a rate: the largest count the arrival table can give (the table is built from the same expression)
static int hv_bound(const int *hv_top, float hv_rate) {
    int m = 0;
    for (int t = 0; t < 96; t++) {
        int c = (int) roundf(hv_rate * (float) hv_top[t]);
        c = c < 0 ? 0 : (c > 255 ? 255 : c);
        m = c > m ? c : m;
    }
    return m;
}

// HySystem.__init__ sweep (HYD:154-158) with zero FCEV demand: electrolyser + compressor power of the
// flow each request level yields while the tank integrates it (see chub_set_hy_table in chub.h).
static void build_hy_table(const HubParams &hp, double *table) {
    double cap = hp.init_soc * hp.cap_mass;
    for (int i = 0; i < 101; i++) {
        double gen_speed = 0.01 * i;
        double must_charge = hp.cap_mass * 0.1 - cap;
        must_charge = must_charge > 0 ? must_charge : 0.0;
        double upper_charge = hp.cap_mass - cap;
        upper_charge = upper_charge > 0 ? upper_charge : 0.0;
        double charge_temp = gen_speed * hp.v_h_max * (15 * 60);
        charge_temp = charge_temp < upper_charge ? charge_temp : upper_charge;
        charge_temp = charge_temp > must_charge ? charge_temp : must_charge;
        double flow = charge_temp / (15 * 60);
        flow = flow < hp.v_h_max ? flow : hp.v_h_max;
        double ele = 0.0;
        if (hp.cells != 0.0) {
            double v_H_mass = flow / hp.cells;
            double v_H_mol = v_H_mass / 2.02;
            double v_H_L = v_H_mol * hp.v_M;
            double v_H = v_H_L * 1000 * 60;
            double temp = v_H * 2 * 96487 / (hp.v_M * 1000 * 60);
            double power = pow(temp, 2) * 0.326 + temp * 1.476;
            ele = hp.cells * power / 1000;
        }
        double cpr = ((flow / 2.02) * hp.cpr_w12 / 0.8) / 1000;
        cap += flow * 15 * 60;
        cap -= cap * hp.hydro_loss;
        table[i] = ele + cpr;
    }
    table[101] = table[100];
}

// PHILOX: one class row = (power, t_soc) of a car that arrived with `soc` after n = 0 .. kClsRow-1 car_steps
// (add_car CHS.hpp:864-877 / 1029-1042 for entry 0, car_step CHS.hpp:900-905 / 1065-1070 from entry to entry), evaluated with
// the curve functions of chub_curves.h on the host
static void build_class_row(bool fast, bool cp, const CurveConsts &cc, float soc, float *row /* [kClsRow][2] */) {
    float t_soc = fast ? fast_soc_to_time(soc, cp) : slow_soc_to_time(soc, cp);
    float power = fast ? fast_time_to_power(t_soc, cp) : slow_time_to_power(t_soc, cp);
    for (int n = 0; n < kClsRow; n++) {
        row[2 * n] = power;
        row[2 * n + 1] = t_soc;
        const float tt = t_soc + 1.0f;
        const float soc_n = fast ? fast_time_to_soc(tt, cp, cc) : slow_time_to_soc(tt, cp, cc);
        power = fast ? fast_time_to_power(tt, cp) : slow_time_to_power(tt, cp);
        t_soc = fast ? fast_soc_to_time(soc_n, cp) : slow_soc_to_time(soc_n, cp);
    }
}

template <typename T>
static int fetch(std::vector<T> &dst, const T *src, size_t count) {
    dst.resize(count);
    HIP_TRY(hipMemcpy(dst.data(), src, count * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}

// upload {hp, arrays, tables} when something in them changed (create, telemetry toggle)
static PackedPtrs packed_ptrs(const chub_env *e) {
    PackedPtrs p;
    p.ev = &e->ev;
    p.st = &e->st;
    p.hot = (uint32_t *) e->sl.hot;
    p.stay8 = (uint8_t *) e->sl.stay8;
    p.rec = (uint32_t *) e->st.rec;
    p.cls[0] = e->tb.cls[0];
    p.cls[1] = e->tb.cls[1];
    p.ttab[0] = e->tb.ttab[0];
    p.ttab[1] = e->tb.ttab[1];
    p.ttab2 = e->tb.ttab2;
    memcpy(p.late8, e->h_late8, sizeof p.late8);
    p.tb = &e->tb;
    p.sin96 = e->h_sin96;
    p.pk[0] = (uint32_t *) e->st.pk[0];
    p.pk[1] = (uint32_t *) e->st.pk[1];
    return p;
}

static int sync_ctx(chub_env *e, hipStream_t s) {
    if (!e->ctx_dirty) return 0;
    DevCtx h;
    h.hp = e->hp; h.sl = e->sl; h.st = e->st; h.ev = e->ev; h.cr = e->cr; h.tb = e->tb; h.ep = e->ep; h.es = e->es;
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(e->d_ctx, &h, sizeof h, hipMemcpyHostToDevice));
    e->ctx_dirty = false;
    return 0;
}

#if CHUB_TRACE
static void *g_stamps_slot = nullptr, *g_stamps_env = nullptr;
extern "C" void chub_debug_stamps(void *slot, void *env) { g_stamps_slot = slot; g_stamps_env = env; }  // measurement builds only
#endif
extern "C" {

const char *chub_last_error(void) { return g_err.c_str(); }

int chub_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int chub_device_info(int device, int32_t *out4) {
    if (!out4) return fail(CHUB_ERR_ARG, "null argument");
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, device));
    out4[0] = p.pciDomainID;
    out4[1] = p.pciBusID;
    out4[2] = p.pciDeviceID;
    out4[3] = p.multiProcessorCount;
    return CHUB_OK;
}

static int write_env_params(chub_env *e, const uint8_t *mask, const chub_env_params *rows);
static int create_impl(const chub_config *cfg_in, const char *data_dir, int64_t n_envs, int64_t env_id0, int device, uint64_t seed, int rng_mode,
                       const chub_options *opt_in, const chub_env_params *rows, chub_env **out);

int chub_create(const chub_config *cfg, const char *data_dir, int64_t n_envs, int64_t env_id0, int device,
                uint64_t seed, int rng_mode, chub_env **out) {
    return chub_create_ex(cfg, data_dir, n_envs, env_id0, device, seed, rng_mode, nullptr, out);
}
int chub_create_ex(const chub_config *cfg, const char *data_dir, int64_t n_envs, int64_t env_id0, int device,
                   uint64_t seed, int rng_mode, const chub_options *opt, chub_env **out) {
    return create_impl(cfg, data_dir, n_envs, env_id0, device, seed, rng_mode, opt, nullptr, out);
}
int chub_create_params(const chub_config *cfg, const char *data_dir, int64_t n_envs, int64_t env_id0, int device, uint64_t seed, int rng_mode,
                       const chub_options *opt, const chub_env_params *rows, chub_env **out) {
    if (!rows) return fail(CHUB_ERR_ARG, "null argument");
    return create_impl(cfg, data_dir, n_envs, env_id0, device, seed, rng_mode, opt, rows, out);
}


// chub_create_ex, and (rows != null) chub_create_params: the handle's scalar kwargs are then each env's row; cfg_in's are ignored
static int create_impl(const chub_config *cfg_in, const char *data_dir, int64_t n_envs, int64_t env_id0, int device, uint64_t seed, int rng_mode,
                       const chub_options *opt_in, const chub_env_params *rows, chub_env **out) {
    if (!cfg_in || !data_dir || !out) return fail(CHUB_ERR_ARG, "null argument");
    chub_options opt;
    memset(&opt, 0, sizeof opt);
    if (opt_in) opt = *opt_in;
    *out = nullptr;
    LaunchPlan plan;
    const char *msg = nullptr;
    if (const int rc = plan_handle(cfg_in, n_envs, rng_mode, opt, plan, &msg)) return fail(rc, msg);
    if (rows)
        if (const int rc = plan_params(plan, rng_mode, &msg)) return fail(rc, msg);
    // PHILOX_CURVES: PHILOX's draws and tail, the slots on k_slot_curves (chub_kernels.hip)
    const bool soc_curves = rng_mode == CHUB_RNG_PHILOX_CURVES;
    const int public_mode = rng_mode;
    if (soc_curves) rng_mode = CHUB_RNG_PHILOX;
    // a handle with rows takes the handle-wide constants (tables it keeps but its tails do not read) from env 0's row
    chub_config cfg_eff = *cfg_in;
    if (rows) {
        for (int64_t i = 0; i < n_envs; i++) {
            const chub_env_params &r = rows[i];
            if (const int rc = check_scalars(r.init_soc, r.hydro_prod_rate, r.hydro_store_vlt, r.fc_max_power, " (env " + std::to_string(i) + ")")) return rc;
        }
        const chub_env_params &r = rows[0];
        cfg_eff.hydro_prod_rate = r.hydro_prod_rate; cfg_eff.hydro_store_vlt = r.hydro_store_vlt; cfg_eff.init_soc = r.init_soc;
        cfg_eff.fc_max_power = r.fc_max_power; cfg_eff.fcev_permeate = r.fcev_permeate; cfg_eff.renew_fluctuate = r.renew_fluctuate;
        cfg_eff.price_fluctuate = r.price_fluctuate; cfg_eff.hydro_loss = r.hydro_loss;
    } else if (const int rc = check_scalars(cfg_in->init_soc, cfg_in->hydro_prod_rate, cfg_in->hydro_store_vlt, cfg_in->fc_max_power, "")) {
        return rc;  // HYD:137
    }
    const chub_config *cfg = &cfg_eff;

    chub_env *e = new chub_env();
    e->cfg = *cfg_in;
    e->env_params = rows != nullptr;
    e->plan = plan;
    e->pair_tails = plan_pair_handle(plan, n_envs, opt, rows != nullptr);
    e->public_mode = public_mode;
    e->device = device;
    e->t = 0;
    e->price_count = 0;
    e->tick = 0;
    e->per_env = false;
    e->d_env_clk = nullptr;
    e->d_mask = nullptr;
    e->h_mask = nullptr;
    e->mask_done[0] = e->mask_done[1] = nullptr;
    e->mask_seq = 0;
    e->cap_full_rel = 0;
    e->graph_per_env0 = false;
    e->graph_full_tick0 = 0;
    e->full_tick = 0;
    e->predrawn = false;
    e->stream = nullptr;
    e->host_stream = nullptr;
    e->upload_stream = nullptr;
    e->h_actions = e->h_packed = e->d_packed = nullptr;
    e->h_bits = e->d_bits = nullptr;
    e->h_tail = e->d_tail = nullptr;
    e->h_telem = nullptr;
    e->empt_valid = false;
    e->prof_used = e->prof_cap = 0;
    e->prof_on = false;
    e->arena = nullptr;
    e->arena_size = e->arena_used = 0;
    auto bail = [&](int rc) {
        chub_destroy(e);
        return rc;
    };

    // ---- tables from the data files
    std::string dir(data_dir);
    std::vector<float> cdf;
    int rc;
    if ((rc = load_cdf(dir + "/car_flow_possibility_list_save.csv", cdf))) return bail(rc);
    std::vector<double> pv(100 * 96), wd(150 * 96);
    if ((rc = load_f64(dir + "/price_96.f64", e->price, 96))) return bail(rc);
    if ((rc = load_f64(dir + "/pv_100x96.f64", pv.data(), pv.size()))) return bail(rc);
    if ((rc = load_f64(dir + "/wd_150x96.f64", wd.data(), wd.size()))) return bail(rc);

    {   // data files are validated before the device is touched (so bad data reports CHUB_ERR_DATA everywhere)
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            return bail(fail(CHUB_ERR_HIP, "no HIP device available: libchub has no CPU path"));
        if (device < 0 || device >= ndev) return bail(fail(CHUB_ERR_ARG, "device ordinal out of range"));
        hipError_t he = hipSetDevice(device);
        if (he != hipSuccess) return bail(fail(CHUB_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(he)));
    }

    // FCEV arrivals per step at most (the count table below is built from the same expression): sizes the explicit part
    // of the waiting list
    int hv_max_arrive = 0;
    {
        float hv_pin = (float) 0.3, hv_perm = (float) cfg->fcev_permeate;
        if (hv_perm > 1) hv_perm = (float) 0.01;
        for (int t = 0; t < 96; t++) {
            // the largest arrival index of row t: level 999 (u = 1), or 300 when the row's CDF never reaches it (CHS.hpp:731-743)
            int n = 300;
            for (int j = 0; j < 301; j++)
                if ((double) cdf[t * 301 + j] >= (double) level_value(kLevels - 1)) {
                    n = j;
                    break;
                }
            e->hv_top[t] = n;
            int c = (int) roundf(hv_pin * hv_perm * (float) n);
            c = c < 0 ? 0 : (c > 255 ? 255 : c);
            hv_max_arrive = c > hv_max_arrive ? c : hv_max_arrive;
        }
    }
    if (hv_max_arrive > 127) return bail(fail(CHUB_ERR_UNSUPPORTED, "more than 127 FCEV arrivals per step"));
    for (int64_t i = 0; rows && i < n_envs; i++) {  // (rows: the largest bound of any env sizes the waiting list)
        const int m = hv_bound(e->hv_top, derive_env_consts(rows[i]).hv_rate);
        if (m > 127) return bail(fail(CHUB_ERR_UNSUPPORTED, "more than 127 FCEV arrivals per step (env " + std::to_string(i) + ")"));
        hv_max_arrive = m > hv_max_arrive ? m : hv_max_arrive;
    }
    e->hv_max_arrive = hv_max_arrive;
    const int qcap = hv_max_arrive > 0 ? 2 * hv_max_arrive - 1 : 1;

    {   // arena: generous upper bound of everything allocated below (telemetry buffers come later, separately)
        const size_t S_tot = (size_t) (cfg->station_list[0] + cfg->station_list[1]);
        const size_t per_env = S_tot * (rng_mode == CHUB_RNG_COMPAT ? 88 : 40) + 1024 + (size_t) qcap * 16 +  // (COMPAT: 16 + 4 + 2 * 32 bytes per slot)
                               (rng_mode == CHUB_RNG_COMPAT ? 102 * 8 + 3 * 33 * 4 + 2 * 4 * (size_t) (1 + hv_max_arrive) + 1024 + 64 : 0);
        const size_t per_env_rows = rows ? (size_t) PRM_COUNT * 8 + 4 + sizeof(chub_env_params) + (rng_mode == CHUB_RNG_COMPAT ? 0 : 102 * 8) : 0;  // + 256-B rounding: the 8 MB below
        const size_t want = (size_t) n_envs * (per_env + per_env_rows) + ((size_t) 8 << 20) + (rows ? (size_t) 96 * kLevels * 2 : 0) +
                            (rng_mode == CHUB_RNG_PHILOX ? 2 * ((size_t) kSocLevels + 2) * (kClsRow * 8 + 4) : 0);
        void *q = nullptr;
        if (!opt.no_arena && hipMalloc(&q, want) == hipSuccess) {
            e->arena = (char *) q;
            e->arena_size = want;
            e->allocs.push_back(q);
        }
    }

    HubParams &hp = e->hp;
    memset(&hp, 0, sizeof hp);
    hp.n_envs = n_envs;
    hp.env_id0 = env_id0;
    int active = 0;
    for (int k = 0; k < 2; k++) {
        hp.S[k] = cfg->station_list[k];
        hp.type[k] = cfg->station_type_list[k];
        hp.H[k] = pow2_ge(hp.S[k] > 0 ? (hp.S[k] < 64 ? hp.S[k] : 64) : 1);  // wave-local kernels: units of at most one wave
        hp.logH[k] = 0;
        while ((1 << hp.logH[k]) < hp.H[k]) hp.logH[k]++;
        hp.U[k] = hp.S[k] > 0 ? (hp.S[k] < 64 ? hp.S[k] : 64) : 1;  // COMPAT wave-local kernels: units of exactly S lanes
        active += hp.S[k] > 0;
        // transformer_limit = constant_power * charge_number in f32 (CHS.hpp:1133-1134, 1443-1444)
        float constant_power = hp.type[k] == CHUB_FAST ? kFastConstantPower : kSlowConstantPower;
        hp.transformer_limit[k] = constant_power * (float) hp.S[k];
    }
    hp.base[0] = 0;
    hp.base[1] = n_envs * hp.S[0];
    hp.obs_dim = 2 + 4 * active + 3;
    hp.act_dim = hp.S[0] + hp.S[1] + 2;
    hp.constant_charging = cfg->constant_charging ? 1 : 0;
    hp.rng_mode = rng_mode;
    hp.soc_curves = soc_curves ? 1 : 0;
    hp.telemetry = 0;
    hp.qcap = qcap;
    hp.hv_w = 1 + hv_max_arrive;
    hp.key[0] = (uint32_t) seed;
    hp.key[1] = (uint32_t) (seed >> 32);
    hp.cc = make_curve_consts();
    // hydrogen system (HYD:94-98, 144, 10-24, 57-72)
    const EnvConsts k0 = derive_env_consts(*cfg);
    hp.cap_mass = k0.cap_mass;
    hp.v_h_max = k0.v_h_max;
    hp.init_soc = k0.init_soc;
    hp.hydro_loss = k0.hydro_loss;
    hp.fc_max_power = k0.fc_max_power;
    hp.v_M = hub_v_M();
    hp.cells = k0.cells;
    {
        double alpha = 1.4, R = 0.082, T = 273 + 25, P_in = 1, P_out = 200;
        double P_a = sqrt(P_in * P_out);
        double part1 = alpha / (alpha - 1);
        double part2 = part1 * R * T;
        double part3 = (alpha - 1) / alpha;
        double W_1 = part2 * (-1 + pow(P_a / P_in, part3));
        double W_2 = part2 * (-1 + pow(P_out / P_a, part3));
        hp.cpr_w12 = W_1 + W_2;
    }
    hp.rc_cells = k0.rc_cells;
    hp.rc_cap_mass = k0.rc_cap_mass;
    hp.rc_vm60k = 1.0 / (hp.v_M * 1000 * 60);
    for (int k = 0; k < 2; k++) {
        const double half_range = (double) hp.transformer_limit[k] / 2;
        hp.rc_half_range[k] = half_range != 0.0 ? 1.0 / half_range : 0.0;
    }
    hp.renew_fluct1 = k0.renew_fluct1;
    hp.price_fluct1 = k0.price_fluct1;
    {
        double mean = np_sum96(e->price) / 96;
        double dev[96];
        for (int i = 0; i < 96; i++) {
            double d = fabs(e->price[i] - mean);
            dev[i] = d * d;
        }
        hp.price_mean = mean;
        hp.price_std = sqrt(np_sum96(dev) / 96);
        hp.rc_price_std = 1.0 / hp.price_std;
    }

    // arrival index per (slot of day, level): first j with CDF[t][j] >= u_k, else 300 (CHS.hpp:731-743),
    // then the per-station-type scaling + std::round (CHS.hpp:751-780, HYD:247-251)
    std::vector<uint8_t> cnt[2], cnt_hv(96 * kLevels);
    std::vector<uint16_t> hv_idx(96 * kLevels);  // (per-env parameters: the index itself, each env scales it by its own rate on the device)
    cnt[0].resize(96 * kLevels);
    cnt[1].resize(96 * kLevels);
    float hv_pin = (float) 0.3, hv_perm = (float) cfg->fcev_permeate;
    if (hv_perm > 1) hv_perm = (float) 0.01;
    for (int t = 0; t < 96; t++) {
        for (int k = 0; k < kLevels; k++) {
            float u = level_value(k);
            int n = 300;
            for (int j = 0; j < 301; j++) {
                if ((double) cdf[t * 301 + j] >= (double) u) {
                    n = j;
                    break;
                }
            }
            for (int s = 0; s < 2; s++) {
                float possible_in = hp.type[s] == CHUB_FAST ? (float) 0.15 : (float) 0.1;
                float permeability = (float) 0.2;
                float po = possible_in * permeability * (float) n;
                int c = (int) roundf(po);
                cnt[s][t * kLevels + k] = (uint8_t) (c < 0 ? 0 : (c > 255 ? 255 : c));
            }
            int c = (int) roundf(hv_pin * hv_perm * (float) n);
            cnt_hv[t * kLevels + k] = (uint8_t) (c < 0 ? 0 : (c > 255 ? 255 : c));
            hv_idx[t * kLevels + k] = (uint16_t) n;
        }
    }
    // chub_forecast_device: the mean of each table over a slot's 1000 levels (an integer sum, narrowed and divided once), and for handles with
    // per-env rows how often each arrival index occurs among them -- the device then sums at most kFcHist terms per (env, slot)
    std::vector<float> fc_mean(3 * 96);
    std::vector<uint32_t> fc_hist(rows ? 96 * kFcHist : 0, 0u);
    std::vector<uint16_t> fc_hist_len(rows ? 96 : 0, (uint16_t) 0);
    for (int t = 0; t < 96; t++) {
        const uint8_t *tab[3] = {&cnt[0][t * kLevels], &cnt[1][t * kLevels], &cnt_hv[t * kLevels]};
        for (int j = 0; j < 3; j++) {
            uint32_t sum = 0;
            for (int k = 0; k < kLevels; k++) sum += tab[j][k];
            fc_mean[j * 96 + t] = (float) sum / 1000.0f;
        }
        if (rows) {
            uint32_t levels[kFcHist] = {0u};
            for (int k = 0; k < kLevels; k++) levels[hv_idx[t * kLevels + k]]++;
            for (uint32_t v = 0; v < (uint32_t) kFcHist; v++)
                if (levels[v]) fc_hist[t * kFcHist + fc_hist_len[t]++] = v | (levels[v] << 16);
        }
    }
    if (rng_mode == CHUB_RNG_PHILOX) {
        // the packed per-step station draws (draw_station_levels) hold up to 9 arrivals per station and step
        int top = 0;
        for (int sidx = 0; sidx < 2; sidx++)
            for (uint8_t c : cnt[sidx]) top = c > top ? c : top;
        if (top > 9)
            return bail(fail(CHUB_ERR_UNSUPPORTED, "arrival table yields more than 9 EV arrivals per station and step"));
    }
    // level thresholds of the renege / balk tests (CHS.hpp:1286-1303): u > 0.1*logf(w+1), u <= expf(-0.01*m)
    std::vector<uint16_t> thr_renege(kMaxLine);
    for (int w = 0; w < kMaxLine; w++) {
        float leave_possibility = (float) (0.1 * (double) logf((float) (w + 1)));
        int thr = kLevels;
        for (int k = 0; k < kLevels; k++)
            if (level_value(k) > leave_possibility) {
                thr = k;
                break;
            }
        thr_renege[w] = (uint16_t) thr;
    }
    std::vector<int16_t> thr_balk(kBalkTab);
    for (int m = 0; m < kBalkTab; m++) {
        float stay = expf((float) (-(0.01 * m)));
        int thr = -1;
        for (int k = 0; k < kLevels; k++)
            if (level_value(k) <= stay) thr = k;
        thr_balk[m] = (int16_t) thr;
    }
    std::vector<int16_t> inv_balk(kLevels);
    for (int v = 0; v < kLevels; v++) {
        int best = -1;
        for (int m = 0; m < kBalkTab; m++)
            if ((int) thr_balk[m] >= v) best = m;
        inv_balk[v] = (int16_t) best;
    }
    std::vector<double> price_v(e->price, e->price + 96), pvT(96 * 100), wdT(96 * 150);
    for (int d = 0; d < 100; d++)
        for (int t = 0; t < 96; t++) pvT[t * 100 + d] = pv[d * 96 + t];
    for (int d = 0; d < 150; d++)
        for (int t = 0; t < 96; t++) wdT[t * 150 + d] = wd[d * 96 + t];
    // PHILOX-mode sampling tables + the 1000 possible target SoCs already mapped through each station's curve
    std::vector<float> icdf(4097);
    std::vector<uint32_t> late_thr(16);
    {
        FILE *f = fopen((dir + "/soc_d_icdf_4097.f32").c_str(), "rb");
        if (!f || fread(icdf.data(), 4, 4097, f) != 4097) {
            if (f) fclose(f);
            return bail(fail(CHUB_ERR_DATA, "cannot read soc_d_icdf_4097.f32"));
        }
        fclose(f);
        f = fopen((dir + "/late_thr_16.u32").c_str(), "rb");
        if (!f || fread(late_thr.data(), 4, 16, f) != 16) {
            if (f) fclose(f);
            return bail(fail(CHUB_ERR_DATA, "cannot read late_thr_16.u32"));
        }
        fclose(f);
    }
    std::vector<float> nicdf(4097), ntail(4097);
    {
        FILE *f = fopen((dir + "/normal_icdf_4097.f32").c_str(), "rb");
        if (!f || fread(nicdf.data(), 4, 4097, f) != 4097) {
            if (f) fclose(f);
            return bail(fail(CHUB_ERR_DATA, "cannot read normal_icdf_4097.f32"));
        }
        fclose(f);
        f = fopen((dir + "/normal_tail_4097.f32").c_str(), "rb");
        if (!f || fread(ntail.data(), 4, 4097, f) != 4097) {
            if (f) fclose(f);
            return bail(fail(CHUB_ERR_DATA, "cannot read normal_tail_4097.f32"));
        }
        fclose(f);
    }
    std::vector<double> sin96(96);
    for (int t = 0; t < 96; t++) sin96[t] = sin((2 * M_PI / 96) * (double) t);  // np.sin(k * time), MGR:319-320
    std::vector<float> ttab[2], cls[2], cls_soc0[2];
    const size_t n_classes = (size_t) kSocLevels;
    for (int s = 0; s < 2; s++) {
        const bool fast = hp.type[s] == CHUB_FAST, cpw = hp.constant_charging != 0;
        ttab[s].resize(kLevels);
        float tt_max = 0.0f;
        for (int k = 0; k < kLevels; k++) {
            float tr = (float) k / 999.0f;
            float target = tr * (100.0f - 80.0f) + 80.0f;  // uniform_rand(80, 100), CHS.hpp:35-44
            ttab[s][k] = fast ? fast_soc_to_time(target, cpw) : slow_soc_to_time(target, cpw);
            tt_max = ttab[s][k] > tt_max ? ttab[s][k] : tt_max;
        }
        if (rng_mode != CHUB_RNG_PHILOX) continue;
        // PHILOX: the arrival SoC takes one of kSocLevels = 2048 equiprobable classes: class l sits at probability (l + 0.5) /
        // 2048 of the tabulated inverse CDF of clip(N(7,3),1,10), i.e. exactly at its node 2 l + 1 (mk_soc,
        // CHS.hpp:804-814); its row holds where the car is on its curve after every number of car_steps it can take
        cls[s].assign((n_classes + 1) * (size_t) kClsRow * 2, 0.0f);  // + one row of padding: entry n + 1 is read with entry n
        cls_soc0[s].assign(n_classes, 0.0f);
        float ts_min = 1e30f;
        for (int l = 0; l < kSocLevels; l++) {
            float d = icdf[2 * l + 1];
            if ((double) d < 1.0) d = 1.0f;
            else if ((double) d > 10.0) d = 10.0f;
            const float soc = (float) (75.0 - 5.0 * (double) d);
            cls_soc0[s][l] = soc;
            float *row = &cls[s][(size_t) l * kClsRow * 2];
            build_class_row(fast, cpw, hp.cc, soc, row);
            ts_min = row[1] < ts_min ? row[1] : ts_min;
        }
        // stay_time = ceil(soc_to_time(target) - soc_to_time(soc)) + late (late <= 15): the state word has 5 bits for what is left
        // of it and for the car_steps taken (a car takes at most stay_time - 1), a class row kClsRow = 32 entries
        const int max_stay = (int) ceilf(tt_max - ts_min) + 15;
        if (max_stay > 31) return bail(fail(CHUB_ERR_UNSUPPORTED, "charge curves yield stays longer than 31 slots (the 5-bit fields of the slot state)"));
    }
    e->tape_classes = 0;
    e->capturing = false;
    e->graph_base = 0;
    hp.packed = plan.packed != PACKED_NONE ? 1 : 0;
    hp.pblock = plan.pblock;
    hp.pslots = plan.pslots;
    hp.epb = plan.epb;
    hp.xcd = plan.xcd;
    hp.compat_split = (plan.compat == COMPAT_SPLIT || plan.compat == COMPAT_WALK2_32 || plan.compat == COMPAT_WALK2_64) ? 1 : 0;
    build_hy_table(hp, e->hy_table);
    std::vector<double> hy_v(e->hy_table, e->hy_table + 102);

    if ((rc = dev_upload(e, &e->tb.cnt[0], cnt[0]))) return bail(rc);
    if ((rc = dev_upload(e, &e->tb.cnt[1], cnt[1]))) return bail(rc);
    if ((rc = dev_upload(e, &e->tb.cnt_hv, cnt_hv))) return bail(rc);
    if ((rc = dev_upload(e, &e->tb.thr_renege, thr_renege))) return bail(rc);
    if ((rc = dev_upload(e, &e->tb.thr_balk, thr_balk))) return bail(rc);
    if ((rc = dev_upload(e, &e->tb.inv_balk, inv_balk))) return bail(rc);
    if ((rc = dev_upload(e, &e->tb.price, price_v))) return bail(rc);
    if ((rc = dev_upload(e, &e->tb.pvT, pvT))) return bail(rc);
    if ((rc = dev_upload(e, &e->tb.wdT, wdT))) return bail(rc);
    if ((rc = dev_upload(e, &e->tb.hy_table, hy_v))) return bail(rc);
    if ((rc = dev_upload(e, &e->tb.soc_d_icdf, icdf))) return bail(rc);
    if ((rc = dev_upload(e, &e->tb.late_thr, late_thr))) return bail(rc);
    memcpy(e->h_late8, late_thr.data(), sizeof e->h_late8);
    if ((rc = dev_upload(e, &e->tb.normal_icdf, nicdf))) return bail(rc);
    if ((rc = dev_upload(e, &e->tb.normal_tail, ntail))) return bail(rc);
    if ((rc = dev_upload(e, &e->tb.sin96, sin96))) return bail(rc);
    memcpy(e->h_sin96, sin96.data(), sizeof e->h_sin96);
    if ((rc = dev_upload(e, &e->tb.ttab[0], ttab[0]))) return bail(rc);
    if ((rc = dev_upload(e, &e->tb.ttab[1], ttab[1]))) return bail(rc);
    {
        std::vector<float> t2(2048, 0.0f);
        for (int s = 0; s < 2; s++) memcpy(&t2[(size_t) s * 1024], ttab[s].data(), kLevels * sizeof(float));
        if ((rc = dev_upload(e, &e->tb.ttab2, t2))) return bail(rc);
    }
    e->tb.cls[0] = e->tb.cls[1] = e->tb.cls_soc0[0] = e->tb.cls_soc0[1] = nullptr;
    if (rng_mode == CHUB_RNG_PHILOX) {
        // both stations' class tables in one buffer (the packed kernel addresses station 1's as station 0's + a byte distance)
        std::vector<float> both(cls[0]);
        both.insert(both.end(), cls[1].begin(), cls[1].end());
        if ((rc = dev_upload(e, &e->tb.cls[0], both))) return bail(rc);
        e->tb.cls[1] = e->tb.cls[0] + cls[0].size();
        for (int s = 0; s < 2; s++)
            if ((rc = dev_upload(e, &e->tb.cls_soc0[s], cls_soc0[s]))) return bail(rc);
    }
    for (int s = 0; s < 2; s++) e->h_ttab[s] = ttab[s];

    // ---- state in HBM
    const size_t N = (size_t) n_envs, NS = N * (size_t) (hp.S[0] + hp.S[1]);
#define ALLOC(ptr, count)                                        \
    if ((rc = dev_alloc(e, &(ptr), (count)))) return bail(rc)
    e->sl.stay8 = nullptr;
    e->sl.wrd = nullptr;
    e->sl.soc0 = nullptr;
    e->sl.var[0] = e->sl.var[1] = nullptr;
    e->st.empt = nullptr;
    e->st.fa[0] = e->st.fa[1] = nullptr;
    e->st.empt2[0] = e->st.empt2[1] = e->st.shrt[0] = e->st.shrt[1] = nullptr;
    if (soc_curves) {
        ALLOC(e->sl.hot, 2 * NS);  // power, t_soc
        ALLOC(e->sl.wrd, NS);      // the state word
        ALLOC(e->sl.soc0, NS);     // arrival SoC (cold)
        ALLOC(e->sl.stay8, NS);
    } else if (rng_mode == CHUB_RNG_PHILOX) {
        ALLOC(e->sl.hot, NS);  // 4-byte slot state
        ALLOC(e->sl.stay8, NS);
    } else {
        ALLOC(e->sl.hot, 4 * NS);  // the 16-byte hot record: power, arrival SoC, t_soc, word
        ALLOC(e->sl.var[0], 8 * NS); ALLOC(e->sl.var[1], 8 * NS);  // the split step's new cars as the walk made them: 32 bytes per admission rank
        ALLOC(e->st.empt, 2 * N); ALLOC(e->st.fa[0], 2 * N); ALLOC(e->st.fa[1], 2 * N);
        ALLOC(e->st.empt2[0], 2 * N); ALLOC(e->st.empt2[1], 2 * N); ALLOC(e->st.shrt[0], 2 * N); ALLOC(e->st.shrt[1], 2 * N);
    }
    ALLOC(e->st.rec, 8 * N); ALLOC(e->st.pk[0], 2 * N); ALLOC(e->st.pk[1], 2 * N); ALLOC(e->st.tail_act, 2 * N);
    ALLOC(e->ev.cap, N); ALLOC(e->ev.store_soc, N); ALLOC(e->ev.ou, 3 * N); ALLOC(e->ev.price_noise, N);
    ALLOC(e->ev.pv_day, N); ALLOC(e->ev.wd_day, N); ALLOC(e->ev.q_len, N); ALLOC(e->ev.hv_line, N);
    ALLOC(e->ev.q_fold, 2 * N); ALLOC(e->ev.q_fold_cnt, N); ALLOC(e->ev.q_time, N * (size_t) qcap); ALLOC(e->ev.q_mass, N * (size_t) qcap);
    e->ev.hy_env = nullptr;
    ALLOC(e->ev.drw[0], 4 * N); ALLOC(e->ev.drw[1], 4 * N); ALLOC(e->ev.drw_cnt[0], N); ALLOC(e->ev.drw_cnt[1], N);
    e->ev.obs64 = nullptr; e->ev.reward64 = nullptr; e->ev.telem = nullptr;
    for (int p = 0; p < 3; p++) e->cr.g3[p] = e->cr.minstd3[p] = nullptr;
    e->rng_cur = 0;
    e->ev.hv_pre[0] = e->ev.hv_pre[1] = nullptr;
    if (rng_mode == CHUB_RNG_COMPAT) {
        ALLOC(e->ev.hy_env, N * 102);
        for (int p = 0; p < 3; p++) {  // the streams' three buffers in rotation: committed (rng_cur), the walk's shadow, the far walk's (CompatRng)
            ALLOC(e->cr.g3[p], N * 32); ALLOC(e->cr.minstd3[p], N);
        }
        ALLOC(e->ev.hv_pre[0], N * (size_t) hp.hv_w); ALLOC(e->ev.hv_pre[1], N * (size_t) hp.hv_w);
        std::vector<double> rep(N * 102);  // until chub_compat_replay_constructor: every env the zero-demand table
        for (size_t i = 0; i < N; i++) memcpy(&rep[i * 102], e->hy_table, sizeof e->hy_table);
        HIP_TRY(hipMemcpy(e->ev.hy_env, rep.data(), rep.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    ALLOC(e->d_env_clk, 2 * N); ALLOC(e->d_mask, 2 * N);
    ALLOC(e->d_tick_note, N); ALLOC(e->d_done_mask, 2 * N); ALLOC(e->d_done_count, 32);
    ALLOC(e->d_tick_base, 64);
    e->hp.tick_base = e->d_tick_base;
    ALLOC(e->d_ctx, 1);
    e->ctx_dirty = true;
    ALLOC(e->d_actions, N * (size_t) hp.act_dim); ALLOC(e->d_obs, N * (size_t) hp.obs_dim); ALLOC(e->d_reward, N);
    ALLOC(e->d_done, N); ALLOC(e->d_exo_z, N * 3); ALLOC(e->d_exo_days, N * 2);
    if (rows) {
        double *prm = nullptr;
        float *hv_rate = nullptr;
        ALLOC(prm, (size_t) PRM_COUNT * N); ALLOC(hv_rate, N); ALLOC(e->d_rows, N);
        if (!e->ev.hy_env) ALLOC(e->ev.hy_env, N * 102);  // (COMPAT has one already)
        e->ep.prm = prm;
        e->ep.hv_rate = hv_rate;
        if ((rc = dev_upload(e, &e->ep.hv_idx, hv_idx))) return bail(rc);
    }
#undef ALLOC
    if (rows && (rc = write_env_params(e, nullptr, rows))) return bail(rc);
    {   // tank starts at init_soc (HyStore.__init__, HYD:99-100)
        std::vector<double> cap(N, hp.init_soc * hp.cap_mass), soc(N, hp.init_soc);
        for (size_t i = 0; rows && i < N; i++) {
            const EnvConsts k = derive_env_consts(rows[i]);
            cap[i] = k.init_soc * k.cap_mass;
            soc[i] = k.init_soc;
        }
        HIP_TRY(hipMemcpy(e->ev.cap, cap.data(), N * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->ev.store_soc, soc.data(), N * sizeof(double), hipMemcpyHostToDevice));
    }
    if (rng_mode == CHUB_RNG_COMPAT) {
        // default seeds: env i gets srand(seed + 2*id + 1), e.seed(seed + 2*id + 2)
        std::vector<uint32_t> seeds(2 * N);
        for (size_t i = 0; i < N; i++) {
            uint32_t id = (uint32_t) (env_id0 + (int64_t) i);
            seeds[2 * i] = (uint32_t) seed + 2u * id + 1u;
            seeds[2 * i + 1] = (uint32_t) seed + 2u * id + 2u;
        }
        *out = e;
        rc = chub_set_rng_compat_seeds(e, seeds.data());
        if (rc) {
            *out = nullptr;
            return bail(rc);
        }
        // the COMPAT hot record keeps a car's target as its LEVEL and reads soc_to_time(target) from Tables::ttab: once per handle the device
        // evaluates all 2 x 1000 entries itself (the functions the stream walk's add_car uses) and the table must hold exactly those bits
        uint32_t *d_bad = nullptr, bad = 0u;
        if ((rc = sync_ctx(e, nullptr))) {
            *out = nullptr;
            return bail(rc);
        }
        if (hipMalloc((void **) &d_bad, sizeof(uint32_t)) != hipSuccess || hipMemset(d_bad, 0, sizeof(uint32_t)) != hipSuccess) {
            if (d_bad) (void) hipFree(d_bad);
            *out = nullptr;
            return bail(fail(CHUB_ERR_HIP, "hipMalloc failed"));
        }
        launch_check_ttab(e->d_ctx, d_bad, nullptr);
        const hipError_t he = hipMemcpy(&bad, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost);
        (void) hipFree(d_bad);
        if (he != hipSuccess || bad != 0u) {
            *out = nullptr;
            return bail(fail(he != hipSuccess ? CHUB_ERR_HIP : CHUB_ERR_UNSUPPORTED,
                             he != hipSuccess ? "the target-time table could not be checked on the device"
                                              : "the device's soc_to_time differs from the host-built table of target times"));
        }
    }
    {
        const size_t b_mean = fc_mean.size() * sizeof(float), b_hist = fc_hist.size() * sizeof(uint32_t), b_len = fc_hist_len.size() * sizeof(uint16_t);
        char *d = nullptr;
        if (hipMalloc((void **) &d, b_mean + b_hist + b_len) != hipSuccess) return bail(fail(CHUB_ERR_HIP, "hipMalloc failed"));
        e->fc.mean = (const float *) d;
        if (b_hist) {
            e->fc.hist = (const uint32_t *) (d + b_mean);
            e->fc.hist_len = (const uint16_t *) (d + b_mean + b_hist);
        }
        if (hipMemcpy(d, fc_mean.data(), b_mean, hipMemcpyHostToDevice) != hipSuccess ||
            (b_hist && (hipMemcpy(d + b_mean, fc_hist.data(), b_hist, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(d + b_mean + b_hist, fc_hist_len.data(), b_len, hipMemcpyHostToDevice) != hipSuccess)))
            return bail(fail(CHUB_ERR_HIP, "the look-ahead tables could not be uploaded"));
    }
    if (rng_mode == CHUB_RNG_PHILOX && !soc_curves) {
        // the SoC column of k_pile_obs / k_station_profile: the class rows' SoC, by the device's own replay of the curve (replay_soc_steps, the
        // chain the other two layouts run per pile), so that the table's entries are that replay's bits whatever the host's libm makes of it
        if (hipMalloc((void **) &e->d_cls_soc, (size_t) 2 * kSocLevels * kClsRow * sizeof(float)) != hipSuccess) {
            e->d_cls_soc = nullptr;
            return bail(fail(CHUB_ERR_HIP, "hipMalloc failed"));
        }
        if ((rc = sync_ctx(e, nullptr))) return bail(rc);
        launch_build_cls_soc(e->d_ctx, e->d_cls_soc, nullptr);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess)
            return bail(fail(CHUB_ERR_HIP, "the SoC table of the arrival classes could not be built on the device"));
    }
    if (hipMalloc((void **) &e->d_gae_part, (size_t) ((n_envs + kGaeLanes - 1) / kGaeLanes) * 3 * sizeof(double)) != hipSuccess) {
        e->d_gae_part = nullptr;
        return bail(fail(CHUB_ERR_HIP, "hipMalloc failed"));
    }
    if (e->pair_tails) {  // records 32 N, tail actions 8 N, raw draws 16 N, env draws 4 x (16 N + N) bytes, each part 256-byte aligned
        const size_t Np = (size_t) n_envs;
        auto up = [](size_t b) { return (b + 255) & ~(size_t) 255; };
        const size_t b_rec = up(32 * Np), b_act = up(8 * Np), b_raw = up(16 * Np), b_drw = up(16 * Np), b_cnt = up(Np);
        const size_t total = b_rec + b_act + b_raw + 4 * (b_drw + b_cnt);
        if (hipMalloc((void **) &e->d_pair, total) != hipSuccess) {
            e->d_pair = nullptr;
            return bail(fail(CHUB_ERR_HIP, "hipMalloc failed"));
        }
        if (hipMemset(e->d_pair, 0, total) != hipSuccess) return bail(fail(CHUB_ERR_HIP, "hipMemset failed"));
        char *q = e->d_pair;
        e->pair.rec_a = (uint32_t *) q; q += b_rec;
        e->pair.tail_act_a = (float *) q; q += b_act;
        e->pair.pkraw = (uint64_t *) q; q += b_raw;
        for (int a = 0; a < 2; a++)
            for (int b = 0; b < 2; b++) {
                e->pair.drw[a][b] = (uint32_t *) q; q += b_drw;
                e->pair.cnt[a][b] = (uint8_t *) q; q += b_cnt;
            }
    }
    *out = e;
    return CHUB_OK;
}

static void policy_free(chub_policy *pol);
static void moments_free(chub_moments *m);
static void critic_free(chub_critic *c);
static void train_log_free(chub_train_log *log);
static void lagrange_free(chub_lagrange *lag);
static void return_norm_free(chub_return_norm *rn);

int chub_destroy(chub_env *e) {
    if (!e) return CHUB_OK;
    while (!e->return_norms.empty()) return_norm_free(e->return_norms.back());
    while (!e->lagranges.empty()) lagrange_free(e->lagranges.back());
    while (!e->train_logs.empty()) train_log_free(e->train_logs.back());  // (first: it clears the gates of optimisers that still live)
    while (!e->moments.empty()) moments_free(e->moments.back());  // (each takes itself off the list)
    while (!e->policies.empty()) policy_free(e->policies.back());
    while (!e->critics.empty()) critic_free(e->critics.back());
    if (!e->allocs.empty() || !e->prof_events.empty()) {  // a handle that never reached the device owns nothing there
        (void) hipSetDevice(e->device);
        (void) hipDeviceSynchronize();
        for (void *p : e->allocs) (void) hipFree(p);
        for (hipEvent_t ev : e->prof_events) (void) hipEventDestroy(ev);
        if (e->h_actions) (void) hipHostFree(e->h_actions);
        if (e->h_mask) (void) hipHostFree(e->h_mask);
        for (hipEvent_t ev : e->mask_done)
            if (ev) (void) hipEventDestroy(ev);
        if (e->h_packed) (void) hipHostFree(e->h_packed);
        if (e->h_telem) (void) hipHostFree(e->h_telem);
        if (e->d_telem) (void) hipFree(e->d_telem);
        if (e->d_ledger) (void) hipFree(e->d_ledger);
        if (e->d_cls_soc) (void) hipFree(e->d_cls_soc);
        if (e->fc.mean) (void) hipFree((void *) e->fc.mean);
        if (e->d_ep_sum) (void) hipFree(e->d_ep_sum);
        if (e->d_gae_part) (void) hipFree(e->d_gae_part);
        if (e->d_pair) (void) hipFree(e->d_pair);
        if (e->h_bits) (void) hipHostFree(e->h_bits);  // h_tail / d_tail are the ends of the same blocks
        if (e->d_bits) (void) hipFree(e->d_bits);
        if (e->d_packed) (void) hipFree(e->d_packed);
        if (e->host_stream) (void) hipStreamDestroy(e->host_stream);
        if (e->upload_stream) (void) hipStreamDestroy(e->upload_stream);
    }
    (void) hipGetLastError();  // HIP's last-error slot is per thread and sticky: do not leave ours for the next handle's checks
    delete e;
    return CHUB_OK;
}

int chub_obs_dim(const chub_env *e) { return e ? e->hp.obs_dim : CHUB_ERR_ARG; }
int chub_act_dim(const chub_env *e) { return e ? e->hp.act_dim : CHUB_ERR_ARG; }
int64_t chub_num_envs(const chub_env *e) { return e ? e->hp.n_envs : CHUB_ERR_ARG; }
int chub_clock(const chub_env *e) {  // lock-step: the clock; per-env clocks: env 0's (chub_env_clocks has them all)
    if (!e) return CHUB_ERR_ARG;
    if (!e->per_env) return e->t;
    uint16_t c = 0;
    if (hipSetDevice(e->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(&c, e->d_env_clk + (size_t) ((e->tick + 1u - e->graph_base) & 1u) * (size_t) e->hp.n_envs, sizeof c, hipMemcpyDeviceToHost) != hipSuccess)
        return CHUB_ERR_HIP;
    return (int) (c & 127u);
}
int chub_uses_packed_kernel(const chub_env *e) { return e ? e->hp.packed : CHUB_ERR_ARG; }
int chub_uses_xcd_order(const chub_env *e) {  // (the single-launch step has one order only)
    return e ? ((e->hp.packed && e->hp.xcd && e->plan.one_launch == ONE_NONE) ? 1 : 0) : CHUB_ERR_ARG;
}
int chub_uses_fused_step(const chub_env *e) { return e ? ((e->plan.one_launch != ONE_NONE || e->plan.compat_small) ? 1 : 0) : CHUB_ERR_ARG; }

int chub_uses_pair_tails(const chub_env *e) { return e ? (e->pair_tails ? 1 : 0) : CHUB_ERR_ARG; }

int chub_pair_plan(const chub_config *cfg, int64_t n_envs, int rng_mode, const chub_options *opt_in, int env_params, uint32_t flags, int t, int64_t left,
                   int64_t *out) {
    if (!cfg || !out) return fail(CHUB_ERR_ARG, "null argument");
    if (t < 0 || t > 95 || left < 0) return fail(CHUB_ERR_ARG, "t must be 0 .. 95 and left >= 0");
    chub_options opt;
    memset(&opt, 0, sizeof opt);
    if (opt_in) opt = *opt_in;
    LaunchPlan p;
    const char *msg = nullptr;
    if (const int rc = plan_handle(cfg, n_envs, rng_mode, opt, p, &msg)) return fail(rc, msg);
    if (env_params)
        if (const int rc = plan_params(p, rng_mode, &msg)) return fail(rc, msg);
    const bool handle = plan_pair_handle(p, n_envs, opt, env_params != 0);
    PairState c;
    c.comm = (flags & CHUB_PAIRF_COMM) != 0;
    c.per_env = (flags & CHUB_PAIRF_PER_ENV) != 0;
    c.tape = (flags & CHUB_PAIRF_TAPE) != 0;
    c.outputs = (flags & CHUB_PAIRF_OUTPUTS) != 0;
    c.profiling = (flags & CHUB_PAIRF_PROFILING) != 0;
    const bool call = plan_pair_call(handle, c);
    out[CHUB_PAIR_HANDLE] = handle ? 1 : 0;
    out[CHUB_PAIR_CALL] = call ? 1 : 0;
    out[CHUB_PAIR_STEPS] = call ? pair_steps(t, left) : 0;
    return CHUB_OK;
}

int chub_launch_plan(const chub_config *cfg, int64_t n_envs, int rng_mode, const chub_options *opt_in, int32_t *out) {
    if (!cfg || !out) return fail(CHUB_ERR_ARG, "null argument");
    chub_options opt;
    memset(&opt, 0, sizeof opt);
    if (opt_in) opt = *opt_in;
    LaunchPlan p;
    const char *msg = nullptr;
    if (const int rc = plan_handle(cfg, n_envs, rng_mode, opt, p, &msg)) return fail(rc, msg);
    memcpy(out, &p, sizeof p);  // (LaunchPlan is the CHUB_PLAN_* list: chub_plan.h)
    return CHUB_OK;
}

int chub_launch_plan_params(const chub_config *cfg, int64_t n_envs, int rng_mode, const chub_options *opt_in, int32_t *out) {
    if (!cfg || !out) return fail(CHUB_ERR_ARG, "null argument");
    chub_options opt;
    memset(&opt, 0, sizeof opt);
    if (opt_in) opt = *opt_in;
    LaunchPlan p;
    const char *msg = nullptr;
    if (const int rc = plan_handle(cfg, n_envs, rng_mode, opt, p, &msg)) return fail(rc, msg);
    if (const int rc = plan_params(p, rng_mode, &msg)) return fail(rc, msg);
    memcpy(out, &p, sizeof p);
    return CHUB_OK;
}

int chub_sync(chub_env *e) {
    if (!e) return fail(CHUB_ERR_ARG, "null handle");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    return CHUB_OK;
}

// ---- one call ---------------------------------------------------------------------------------------------------------------
// What ONE reset or step was asked to do, as a value.  Every entry point of the C ABI fills one in and hands it to run_call (a span of
// chub_run_steps: to run_span); nothing of a call is kept on the handle, so nothing of it can be left behind for the next one.

// where a call's outputs go (StepArgs has the fields' meaning)
struct OutSink {
    float *obs, *reward;
    int obs_stride, reward_stride;
    uint8_t *done;
    float *done_f32;
};
// three arrays: obs [N][D], reward [N], done [N] u8 (a reset: obs alone)
static OutSink dense_out(const chub_env *e, float *obs, float *reward, uint8_t *done) { return {obs, reward, e->hp.obs_dim, 1, done, nullptr}; }
// one block [N][D + 2] f32: obs, reward, done as 0 / 1
static OutSink packed_out(const chub_env *e, float *packed) {
    const int D = e->hp.obs_dim;
    return {packed, packed + D, D + 2, D + 2, nullptr, packed + D + 1};
}

struct StepCall {
    bool reset;
    int load_mode;            // step: the scalar-load control (chub_step_load*)
    const uint8_t *mask;      // HOST [N], non-zero = the call serves this env; null: every env.  Everything below is device memory
    const uint8_t *dmask;     // or the mask in DEVICE memory, read by the launch alone (chub_dmask_*_device, the reset of an auto-reset call)
    // auto-reset (chub_autoreset_step_device): its step leaves the done mask and its count, its reset reads them and saves the terminal rows
    uint8_t *done_mask;
    uint32_t *done_count;
    const uint32_t *skip_count;
    float *final_obs;
    const float *actions;     // step: the action rows [N][A], or
    const uint64_t *bits;     //   one decision bit per pile [N][ceil(S / 64)] and
    const float *tail;        //   the two tail actions [N][2] (chub_step_bits*)
    const int32_t *exo_days;  // reset: [N][2] or null
    const double *exo_z;      // [N][3] or null
    // tape mode (chub_step_tape* / chub_reset_tape*): the station draws of a step, the cars' variates, and (tail_tape: exo_z, exo_days and
    // the FCEV arrivals hv_tape [N][hv_w]) the tail's variates come from the caller
    const uint64_t *pk_tape;
    const uint32_t *car_tape, *hv_tape;
    int hv_w;
    bool tail_tape;
    OutSink out;
};
static StepCall reset_call(const chub_env *e, const uint8_t *mask, const int32_t *d_exo_days, const double *d_exo_z, float *d_obs) {
    StepCall c = {};
    c.reset = true;
    c.mask = mask;
    c.exo_days = d_exo_days;
    c.exo_z = d_exo_z;
    c.out = dense_out(e, d_obs, nullptr, nullptr);
    return c;
}
static StepCall step_call(const uint8_t *mask, const float *d_actions, const double *d_exo_z, const OutSink &out, int load_mode) {
    StepCall c = {};
    c.load_mode = load_mode;
    c.mask = mask;
    c.actions = d_actions;
    c.exo_z = d_exo_z;
    c.out = out;
    return c;
}

// ---- clocks -----------------------------------------------------------------------------------------------------------------
// Every reference env owns its clock (MGR:137-140, 271-273, 299).  Lock-step (the usual case: everybody reset and stepped
// together) is ONE clock on the host, passed to the kernels as an argument.  The first call that names a subset of the envs
// (chub_reset_envs / chub_step_envs) makes the clock per-env device state: [2][N] u16, read at [tick & 1] and written at
// [(tick + 1) & 1] by the tail kernel for every env (served envs: one step on, or back to 0; the others: unchanged), so
// any call is still ONE launch with one Philox tick, however many different clocks the envs show.  A reset of everybody
// returns to the host clock.

// the mask of one call as its launch sees it: the device copy (null: every env) and the first / last env it names
struct MaskView {
    const uint8_t *d_mask;
    int64_t lo, hi;
};

// onto per-env clocks: every env starts from the lock-step clock, in the buffer the next launch reads
static void enter_per_env(chub_env *e, hipStream_t s) {
    const size_t N = (size_t) e->hp.n_envs;
    const uint16_t c = (uint16_t) ((uint32_t) e->t | (((uint32_t) e->price_count & 3u) << 8));
    launch_fill_clocks(e->d_env_clk + (size_t) ((e->tick + 1u - e->graph_base) & 1u) * N, (int64_t) N, c, s);
    e->per_env = true;
    if (e->h_tick.size() != N) e->h_tick.assign(N, 0u);
}
static const char *const kCaptureNeedsClocks = "a capture that names subsets of the envs must start on per-env clocks: make the first call "
                                               "on a subset before chub_graph_begin (it fills the per-env clocks from the handle's clock)";

// A mask in device memory: the host does not know whom it names, so the call is a masked one over the whole range of envs whatever it
// holds -- no count, no staging, no copy, no wait; a captured call re-reads the caller's buffer on every replay.
static int serve_dmask(chub_env *e, const uint8_t *d_mask, hipStream_t s, int &served, MaskView &mv) {
    if (!e->per_env) {
        if (e->capturing) return fail(CHUB_ERR_ARG, kCaptureNeedsClocks);
        enter_per_env(e, s);
    }
    mv = {d_mask, 0, e->hp.n_envs - 1};
    served = 1;
    return CHUB_OK;
}

// What one call serves: 0 nobody, 1 a subset (mask uploaded, per-env clocks on), 2 every env.
static int serve_mask(chub_env *e, const uint8_t *mask, hipStream_t s, int &served, MaskView &mv) {
    const size_t N = (size_t) e->hp.n_envs;
    size_t n_masked = N;
    mv = {nullptr, 0, (int64_t) N - 1};
    if (mask) {
        n_masked = 0;
        int64_t lo = -1, hi = -1;
        for (size_t i = 0; i < N; i++)
            if (mask[i]) {
                n_masked++;
                if (lo < 0) lo = (int64_t) i;
                hi = (int64_t) i;
            }
        if (n_masked) {
            mv.lo = lo;
            mv.hi = hi;
        }
    }
    served = n_masked == 0 ? 0 : (n_masked == N ? 2 : 1);
    if (served != 1) return CHUB_OK;
    if (e->capturing) {
        // a replay must not read the caller's (or the handle's staging) memory: the mask of a captured call lives in a device
        // buffer of its own, filled now and freed with the graph.  The clocks are device state, so nothing of them is baked in.
        if (!e->per_env) return fail(CHUB_ERR_ARG, kCaptureNeedsClocks);
        uint8_t *d = nullptr;
        HIP_TRY(hipMalloc((void **) &d, N));
        e->cap_masks.push_back(d);
        // filled now, outside the capture: on a stream of its own (the null stream may not be touched while another stream captures)
        if (!e->upload_stream) HIP_TRY(hipStreamCreateWithFlags(&e->upload_stream, hipStreamNonBlocking));
        HIP_TRY(hipMemcpyAsync(d, mask, N, hipMemcpyHostToDevice, e->upload_stream));
        HIP_TRY(hipStreamSynchronize(e->upload_stream));
        mv.d_mask = d;
        return CHUB_OK;
    }
    if (!e->per_env) enter_per_env(e, s);
    // the mask of this call: the caller's array is only borrowed for the duration of the call, so it goes through one of two
    // pinned staging buffers; a buffer is reused once the launches that read its device copy are done (two masked calls ago)
    if (!e->h_mask) {
        HIP_TRY(hipHostMalloc((void **) &e->h_mask, 2 * N, hipHostMallocDefault));
        for (hipEvent_t &ev : e->mask_done) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    const uint32_t b = e->mask_seq & 1u;
    if (e->mask_seq >= 2) HIP_TRY(hipEventSynchronize(e->mask_done[b]));
    memcpy(e->h_mask + (size_t) b * N, mask, N);
    HIP_TRY(hipMemcpyAsync(e->d_mask + (size_t) b * N, e->h_mask + (size_t) b * N, N, hipMemcpyHostToDevice, s));
    mv.d_mask = e->d_mask + (size_t) b * N;
    return CHUB_OK;
}

static int note_served(chub_env *e, const uint8_t *mask, int served, hipStream_t s) {
    const size_t N = (size_t) e->hp.n_envs;
    if (e->capturing) {  // nothing ran: only note which launch of the capture this was (applied by every replay)
        const uint32_t rel = e->tick - e->graph_tick0;
        if (served == 2) e->cap_full_rel = rel;
        else {
            if (e->cap_rel.size() != N) e->cap_rel.assign(N, 0u);
            for (size_t i = 0; i < N; i++)
                if (mask[i]) e->cap_rel[i] = rel;
        }
        return CHUB_OK;
    }
    if (served == 2) {
        e->full_tick = e->tick;
        return CHUB_OK;
    }
    HIP_TRY(hipEventRecord(e->mask_done[e->mask_seq & 1u], s));
    e->mask_seq += 1;
    for (size_t i = 0; i < N; i++)
        if (mask[i]) e->h_tick[i] = e->tick;
    return CHUB_OK;
}

// COMPAT: the handle's lock-step steps of every env run the slot pass beside the NEXT step's stream walks (k_slot_walk2)
static bool walks_two_ahead(const chub_env *e) { return e->plan.compat == COMPAT_WALK2_32 || e->plan.compat == COMPAT_WALK2_64; }

// the launch forms of a reset / step (chub_plan.h)
static CallPlan plan_this_call(const chub_env *e, const StepCall &call, int served, bool fresh) {
    CallState c;
    c.reset = call.reset;
    c.load_mode = call.load_mode != 0;
    c.per_env = e->per_env;
    c.all_served = served == 2;
    c.capturing = e->capturing;
    c.car_tape = call.car_tape != nullptr;
    c.pk_tape = !call.reset && call.pk_tape;
    c.tail_tape = call.tail_tape;
    c.bits = !call.reset && call.bits;
    c.fresh = fresh;
    c.env_params = e->env_params;
    c.dev_mask = call.dmask != nullptr;
    return plan_call(e->plan, c);
}

// The part of StepArgs that every launch of a call fills the same way, for the launch with Philox tick `tick`: the clock and the tariff, the
// call's inputs, tapes and outputs, the envs it serves; then the device's copy of the handle's context is brought up to date
static int fill_args(chub_env *e, const StepCall &c, int served, const MaskView &mv, uint32_t tick, hipStream_t s, StepArgs &sa) {
    memset(&sa, 0, sizeof sa);
    sa.t = c.reset ? 0 : e->t;
    sa.tick = tick - e->graph_base;
    sa.draw_price = (e->price_count % 4 == 0) ? 1 : 0;
    sa.station_filter = -1;
    if (c.reset) {
        sa.price_last = e->price[95];  // AGG:171: price = [] + mean_for_MAD; price[-1]
    } else {
        sa.price_last = e->price[e->t];  // AGG:147
        sa.price_prev = e->price[(e->t + 95) % 96];  // what the make_state before this step saw there (the reset: price[95], AGG:171)
    }
    sa.actions = c.actions;
    sa.act_bits = c.bits;
    sa.act_tail = c.tail;
    sa.exo_days = c.exo_days;
    sa.exo_z = c.exo_z;
    sa.obs = c.out.obs;
    sa.obs_stride = c.out.obs_stride;
    sa.reward = c.out.reward;
    sa.reward_stride = c.out.reward_stride;
    sa.done = c.out.done;
    sa.done_f32 = c.out.done_f32;
    sa.load_mode = c.load_mode;
    sa.pk_tape = c.pk_tape;
    sa.car_tape = c.car_tape;  // (a tape reset: the units' occupancy draws are in pk already, the cars' variates come from the tape)
    sa.hv_tape = c.hv_tape;
    sa.hv_w = c.hv_w;
    sa.tail_tape = c.tail_tape ? 1 : 0;
    // the state-independent draws of a step: left by the previous launch's level blocks if that launch served every env
    // (for the tick that is now this launch's), otherwise made by this launch itself (a graph's first step always makes its
    // own: a replay must not depend on what ran before it)
    sa.fresh = (!c.reset && (!e->predrawn || (e->capturing && tick == e->graph_tick0 + 1u))) ? 1 : 0;
    sa.rng_cur = e->rng_cur;
    sa.env_lo = 0;
    sa.env_hi = (int32_t) (e->hp.n_envs - 1);
    if (e->per_env) {
        sa.env_clk = e->d_env_clk;
        if (served == 1) {
            sa.env_mask = mv.d_mask;
            sa.env_lo = (int32_t) mv.lo;
            sa.env_hi = (int32_t) mv.hi;
        }
    }
    if (c.dmask) sa.tick_note = e->d_tick_note;  // (whom the launch served: only the device knows)
    sa.done_mask = c.done_mask;
    sa.done_count = c.done_count;
    sa.skip_count = c.skip_count;
    sa.final_obs = c.final_obs;
    return sync_ctx(e, s);
}

// the handle's clocks behind a launch that went out: a reset, or k steps
static void advance_clocks(chub_env *e, const StepCall &c, int served, int k) {
    e->predrawn = served == 2;  // the launch's level blocks left the next step's draws of every env it served
    if (c.reset) {
        if (served == 2) {  // everybody starts a new day: one clock again (the launch itself still ran on the envs' own clocks)
            e->per_env = false;
            e->t = 0;
            e->price_count = 0;  // MGR:313 (after make_state)
        }
    } else if (!e->per_env) {
        e->price_count += k;
        e->t = (e->t + k) % 96;
    }
}

// ONE launched reset: of every env (served = 2) or of the envs of the uploaded mask (served = 1)
static int run_reset(chub_env *e, const StepCall &c, int served, const MaskView &mv, hipStream_t s) {
    e->tick += 1;
    e->walked_tick = 0;  // (a walk that ran ahead for a step that now does not come: its shadow is simply overwritten)
    StepArgs sa;
    if (const int rc = fill_args(e, c, served, mv, e->tick, s, sa)) return rc;
    const CallPlan cp = plan_this_call(e, c, served, false);
    // COMPAT split reset: the walk's draws are committed by the slot pass (k_compat_small walks the streams in place: nothing to commit)
    sa.commit_rng = (cp.call != CALL_COMPAT_SMALL && slot_form_split(cp.slot)) ? 1 : 0;
    sa.walk_short = walks_two_ahead(e) ? 1 : 0;  // (the reset's walk leaves its short stays for a walk two steps ahead, as every walk of such a handle)
    if (cp.call == CALL_COMPAT_SMALL) {
        launch_compat_small<true>(e->hp, e->d_ctx, sa, s, packed_ptrs(e));
        e->empt_valid = true;  // (k_compat_small is the split step in one launch: its slot waves leave the counts)
    } else {
        launch_slot<true>(cp, e->hp, e->plan, e->d_ctx, sa, s, packed_ptrs(e), nullptr, nullptr);
        if (sa.commit_rng) sa.rng_cur = e->rng_cur = (e->rng_cur + 1) % 3;  // the commit: the walk's shadow is the streams' buffer from here on
        launch_env<true>(cp.env, e->hp, e->d_ctx, sa, s, nullptr, nullptr, packed_ptrs(e));
        // (a split reset leaves the counts of the units it served; those of the others are as good as they were)
        e->empt_valid = e->hp.compat_split != 0 && (served == 2 || e->empt_valid) && !e->capturing;
        if (e->hp.compat_split != 0 && served == 2 && !e->capturing) e->e2_tick = e->tick;  // (... and every unit's empt2, at this tick's parity)
    }
    HIP_TRY(hipGetLastError());
    advance_clocks(e, c, served, 1);
    return CHUB_OK;
}

// ONE launched step: of every env (served = 2) or of the envs of the uploaded mask (served = 1)
static int run_step(chub_env *e, const StepCall &c, int served, const MaskView &mv, hipStream_t s) {
    e->tick += 1;
    const uint32_t walked_tick = e->walked_tick;
    e->walked_tick = 0;
    StepArgs sa;
    if (const int rc = fill_args(e, c, served, mv, e->tick, s, sa)) return rc;
#if CHUB_TRACE
    sa.stamps_slot = (unsigned long long *) g_stamps_slot;
    sa.stamps_env = (unsigned long long *) g_stamps_env;
#endif
    const CallPlan cp = plan_this_call(e, c, served, sa.fresh != 0);
    const bool split_step = cp.call != CALL_COMPAT_SMALL && slot_form_split(cp.slot);
    if (split_step) {  // COMPAT split step: the slot pass commits the walk's draws, the tail reads the forecourt's from where the walk left them
        sa.commit_rng = 1;
        sa.hv_tape = (const uint32_t *) e->ev.hv_pre[sa.tick & 1u];
        sa.hv_w = e->hp.hv_w;
        sa.walked = (walked_tick == e->tick && served == 2 && !e->per_env) ? 1 : 0;
        sa.walk_short = walks_two_ahead(e) ? 1 : 0;
    }
    bool prof = e->prof_on && e->prof_used < e->prof_cap;
    if (prof) {
        prof = (e->prof_phase % e->prof_every) == 0;  // sample: the event records are not free
        e->prof_phase++;
    }
    // four events per profiled step: start / stop of the slot kernel, start / stop of the tail kernel
    hipEvent_t *pe = prof ? &e->prof_events[4 * e->prof_used] : nullptr;
    sa.empt_fresh = ((cp.call == CALL_COMPAT_SMALL || e->hp.compat_split) && (!e->empt_valid || e->capturing)) ? 1 : 0;
    if (cp.call == CALL_COMPAT_SMALL) {
        launch_compat_small<false>(e->hp, e->d_ctx, sa, s, packed_ptrs(e));
        e->empt_valid = true;
        if (prof) {  // one kernel, no dispatch timestamps: the sample spans nothing
            for (int i = 0; i < 4; i++) HIP_TRY(hipEventRecord(pe[i], s));
        }
    } else if (cp.call == CALL_ONE_LAUNCH) {
        launch_step_fused(cp, e->hp, e->d_ctx, sa, s, packed_ptrs(e), prof ? pe[0] : nullptr, prof ? pe[1] : nullptr);
        if (prof) {  // one kernel: the whole step is on the first pair of timestamps, the second pair spans nothing
            HIP_TRY(hipEventRecord(pe[2], s));
            HIP_TRY(hipEventRecord(pe[3], s));
        }
    } else if (cp.call == CALL_SLOT_WALK2) {
        // lock-step COMPAT steps of every env, stations of 8 to 64 piles: the slot pass of this step beside the stream walks of the NEXT one
        // (k_slot_walk2: the walk two steps ahead of the slots it draws for), then the tails alone -- if the next call is that step, its walk
        // has run; if it is anything else, the walk's shadow is never committed
        if (e->e2_tick != e->tick - 1u) sa.empt_fresh = 1;  // (empt2 is not the previous pass's for every unit: counted in front)
        StepArgs sw = sa;
        sw.t = (e->t + 1) % 96;
        sw.tick = sa.tick + 1u;
        sw.walk_far = 1;  // (reads the buffer behind the committed one -- this step's shadow -- and writes the one behind that)
        launch_slot_walk2(e->plan, e->hp, e->d_ctx, sa, sw, s, prof ? pe[0] : nullptr, prof ? pe[1] : nullptr);
        sa.rng_cur = e->rng_cur = (e->rng_cur + 1) % 3;  // the commit of this step's draws: its walk's shadow is the streams' buffer now
        launch_env<false>(cp.env, e->hp, e->d_ctx, sa, s, prof ? pe[2] : nullptr, prof ? pe[3] : nullptr, packed_ptrs(e));
        e->walked_tick = e->tick + 1u;
        e->empt_valid = true;
        e->e2_tick = e->tick;
    } else {
        launch_slot<false>(cp, e->hp, e->plan, e->d_ctx, sa, s, packed_ptrs(e), prof ? pe[0] : nullptr, prof ? pe[1] : nullptr);
        if (sa.commit_rng) sa.rng_cur = e->rng_cur = (e->rng_cur + 1) % 3;  // the commit (as above)
        if (split_step && served == 2 && !e->per_env && !e->capturing) e->e2_tick = e->tick;  // (every unit's empt2, whichever pass it was)
        if (cp.call == CALL_SLOT_ENV_WALK) {
            // lock-step COMPAT steps of every env: the tails of this step and the stream walks of the NEXT one in one launch (k_env_walk) --
            // if the next call is that step, its walk has run; if it is anything else, the walk's shadow is never committed
            StepArgs sw = sa;  // (rng_cur: the buffer this step's slot pass has just made the committed one)
            sw.t = (e->t + 1) % 96;
            sw.tick = sa.tick + 1u;
            launch_env_walk(e->hp, e->d_ctx, sa, sw, s, prof ? pe[2] : nullptr, prof ? pe[3] : nullptr, packed_ptrs(e));
            e->walked_tick = e->tick + 1u;
        } else {
            launch_env<false>(cp.env, e->hp, e->d_ctx, sa, s, prof ? pe[2] : nullptr, prof ? pe[3] : nullptr, packed_ptrs(e));
        }
        e->empt_valid = e->hp.compat_split != 0 && !e->capturing;  // (counted for every unit in front of the walk, or good already; the pass left the served units')
    }
    if (prof) e->prof_used++;
    HIP_TRY(hipGetLastError());
    advance_clocks(e, c, served, 1);
    return CHUB_OK;
}

// the precondition of a COMPAT handle's calls: the caller brings the variates the reference's numpy would have drawn
static int check_compat_variates(const chub_env *e, bool reset, const int32_t *exo_days, const double *exo_z) {
    if (e->hp.rng_mode != CHUB_RNG_COMPAT) return CHUB_OK;
    if (reset && (!exo_days || !exo_z)) return fail(CHUB_ERR_ARG, "COMPAT mode needs exo_days and exo_z");
    if (!reset && !exo_z) return fail(CHUB_ERR_ARG, "COMPAT mode needs exo_z");
    return CHUB_OK;
}

// ONE reset or step, from the checks that depend on the call to the handle's bookkeeping behind the launch
static int run_call(chub_env *e, const StepCall &call, hipStream_t s) {
    if (call.reset) {
        if (const int rc = check_compat_variates(e, true, call.exo_days, call.exo_z)) return rc;
        if (e->tape_only && !call.car_tape)
            return fail(CHUB_ERR_ARG, "a handle with registered tape classes resets through chub_reset_tape / chub_reset_tape_env only");
    } else {
        if (e->tick == 0) return fail(CHUB_ERR_ARG, "step() before reset()");
        if (e->tape_only && !call.pk_tape)
            return fail(CHUB_ERR_ARG, "a handle with registered tape classes steps through chub_step_tape / chub_step_tape_env only (its class "
                                      "rows hold the caller's arrival SoCs: cars admitted by this build's own draws would be given them)");
        if (const int rc = check_compat_variates(e, false, nullptr, call.exo_z)) return rc;
        if (call.load_mode && e->hp.soc_curves)
            return fail(CHUB_ERR_UNSUPPORTED, "the scalar-load control (chub_step_load*) is not supported in rng_mode PHILOX_CURVES");
        if (call.load_mode && e->env_params) return refuse_params("the scalar-load control (chub_step_load*)");
    }
    HIP_TRY(hipSetDevice(e->device));
    StepCall c = call;
    if (c.bits && !(e->hp.packed && e->hp.rng_mode == CHUB_RNG_PHILOX)) {
        // only the packed PHILOX slot kernel reads the bits themselves (8 bytes per env and word instead of a row of floats); for every other
        // kernel they are expanded on the device into the action rows it reads
        launch_expand_bits(e->hp, c.bits, c.tail, e->d_actions, s);
        HIP_TRY(hipGetLastError());
        c.actions = e->d_actions;
        c.bits = nullptr;
        c.tail = nullptr;
    }
    (void) hipGetLastError();  // a stale error of an earlier, unrelated call must not be reported as this call's
    int served = 0;
    MaskView mv;
    const bool was_per_env = e->per_env;
    int rc = c.dmask ? serve_dmask(e, c.dmask, s, served, mv) : serve_mask(e, c.mask, s, served, mv);
    if (rc || served == 0) return rc;
    rc = c.reset ? run_reset(e, c, served, mv, s) : run_step(e, c, served, mv, s);
    if (rc) {
        e->per_env = was_per_env;  // nothing was launched: the handle stays on the clock(s) it was on
        return rc;
    }
    // the attached step terms (chub_set_step_terms): the rows of the envs this step served, from the telemetry block its tail has just written --
    // behind the step's kernels and, in an auto-reset call, in front of the reset that overwrites part of that block
    hipError_t st_err = hipSuccess;
    if (e->st_out && !c.reset) {
        launch_step_terms<float>(e->hp, e->d_ctx, e->st_fields, mv.d_mask, e->st_out, s);
        st_err = hipGetLastError();
    }
    if (!c.dmask) rc = note_served(e, c.mask, served, s);  // (a device mask: the launch itself notes whom it served, StepArgs::tick_note)
    if (st_err != hipSuccess) return fail(CHUB_ERR_HIP, std::string("the step ran, its step terms could not be launched: ") + hipGetErrorString(st_err));
    return rc;
}

int chub_reset_device(chub_env *e, const int32_t *d_exo_days, const double *d_exo_z, float *d_obs, void *stream) {
    if (!e || !d_obs) return fail(CHUB_ERR_ARG, "null argument");
    return run_call(e, reset_call(e, nullptr, d_exo_days, d_exo_z, d_obs), (hipStream_t) stream);
}

int chub_reset_envs_device(chub_env *e, const uint8_t *mask, const int32_t *d_exo_days, const double *d_exo_z, float *d_obs, void *stream) {
    if (!e || !mask || !d_obs) return fail(CHUB_ERR_ARG, "null argument");
    return run_call(e, reset_call(e, mask, d_exo_days, d_exo_z, d_obs), (hipStream_t) stream);
}

int chub_step_device(chub_env *e, const float *d_actions, const double *d_exo_z, float *d_obs, float *d_reward,
                     uint8_t *d_done, void *stream) {
    if (!e || !d_actions || !d_obs || !d_reward || !d_done) return fail(CHUB_ERR_ARG, "null argument");
    return run_call(e, step_call(nullptr, d_actions, d_exo_z, dense_out(e, d_obs, d_reward, d_done), 0), (hipStream_t) stream);
}

int chub_step_device_packed(chub_env *e, const float *d_actions, const double *d_exo_z, float *d_packed, void *stream) {
    if (!e || !d_actions || !d_packed) return fail(CHUB_ERR_ARG, "null argument");
    return run_call(e, step_call(nullptr, d_actions, d_exo_z, packed_out(e, d_packed), 0), (hipStream_t) stream);
}

int chub_step_load_device(chub_env *e, const float *d_actions, const double *d_exo_z, float *d_obs, float *d_reward,
                          uint8_t *d_done, void *stream) {
    if (!e || !d_actions || !d_obs || !d_reward || !d_done) return fail(CHUB_ERR_ARG, "null argument");
    return run_call(e, step_call(nullptr, d_actions, d_exo_z, dense_out(e, d_obs, d_reward, d_done), 1), (hipStream_t) stream);
}

int chub_step_envs_device(chub_env *e, const uint8_t *mask, const float *d_actions, const double *d_exo_z, float *d_obs, float *d_reward,
                          uint8_t *d_done, void *stream) {
    if (!e || !mask || !d_actions || !d_obs || !d_reward || !d_done) return fail(CHUB_ERR_ARG, "null argument");
    return run_call(e, step_call(mask, d_actions, d_exo_z, dense_out(e, d_obs, d_reward, d_done), 0), (hipStream_t) stream);
}

// ---- masks in device memory, and the step that resets whoever finished (include/chub.h) ---------------------------------------------------
static int refuse_tape_dmask(const chub_env *e, const char *what) {
    if (!e->tape_only) return CHUB_OK;
    return fail(CHUB_ERR_UNSUPPORTED, std::string(what) + " is not supported on a tape handle (chub_tape_register_soc)");
}

int chub_dmask_reset_envs_device(chub_env *e, const uint8_t *d_mask, const int32_t *d_exo_days, const double *d_exo_z, float *d_obs, void *stream) {
    if (!e || !d_mask || !d_obs) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = refuse_tape_dmask(e, "chub_dmask_reset_envs_device")) return rc;
    StepCall c = reset_call(e, nullptr, d_exo_days, d_exo_z, d_obs);
    c.dmask = d_mask;
    return run_call(e, c, (hipStream_t) stream);
}

int chub_dmask_step_envs_device(chub_env *e, const uint8_t *d_mask, const float *d_actions, const double *d_exo_z, float *d_obs, float *d_reward,
                                uint8_t *d_done, void *stream) {
    if (!e || !d_mask || !d_actions || !d_obs || !d_reward || !d_done) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = refuse_tape_dmask(e, "chub_dmask_step_envs_device")) return rc;
    StepCall c = step_call(nullptr, d_actions, d_exo_z, dense_out(e, d_obs, d_reward, d_done), 0);
    c.dmask = d_mask;
    return run_call(e, c, (hipStream_t) stream);
}

// Two launches, two ticks, whoever is done: the step of every env on its own clock (tick T), which leaves each env's done byte and their
// count in the handle's buffers, then the masked reset of exactly those envs (tick T + 1), whose workgroups return at entry while the count
// is 0.  Both go into the packed block: a reset env's row keeps the step's reward and done = 1 and takes the new episode's first observation.
int chub_autoreset_step_device(chub_env *e, const float *d_actions, const double *d_exo_z, const int32_t *d_reset_exo_days,
                               const double *d_reset_exo_z, float *d_packed, float *d_final_obs, void *stream) {
    if (!e || !d_actions || !d_packed) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = refuse_tape_dmask(e, "chub_autoreset_step_device")) return rc;
    if (e->tick == 0) return fail(CHUB_ERR_ARG, "step() before reset()");
    if (const int rc = check_compat_variates(e, false, nullptr, d_exo_z)) return rc;
    if (e->hp.rng_mode == CHUB_RNG_COMPAT && (!d_reset_exo_days || !d_reset_exo_z))
        return fail(CHUB_ERR_ARG, "COMPAT mode needs d_reset_exo_days and d_reset_exo_z (the rows of the envs that finish are read)");
    hipStream_t s = (hipStream_t) stream;
    HIP_TRY(hipSetDevice(e->device));
    // Everything a caller can get wrong has been refused above: from here on only the HIP runtime can fail.  If it does before the step is
    // launched the handle is left as it was found (clocks, draws, mask buffer); if it does between the two launches the step HAS run -- one
    // tick is consumed, the done mask is on the device and nobody has been reset -- and the error is returned as it is: the caller's stream
    // is in a state only it can judge (the same holds for any call whose second kernel fails to launch).
    const bool was_per_env = e->per_env, was_predrawn = e->predrawn;
    if (!e->per_env) {
        if (e->capturing) return fail(CHUB_ERR_ARG, kCaptureNeedsClocks);
        enter_per_env(e, s);
        e->predrawn = false;  // (the step below makes its own draws, as after any call that changed how the envs are served)
    }
    const size_t N = (size_t) e->hp.n_envs;
    const uint32_t b = e->done_seq & 1u;
    uint8_t *mask = e->d_done_mask + (size_t) b * N;
    uint32_t *count = e->d_done_count + (size_t) b * 16;
    StepCall st = step_call(nullptr, d_actions, d_exo_z, packed_out(e, d_packed), 0);
    st.done_mask = mask;
    st.done_count = count;
    int rc = hipMemsetAsync(count, 0, sizeof(uint32_t), s) == hipSuccess ? CHUB_OK : fail(CHUB_ERR_HIP, "hipMemsetAsync of the done count failed");
    if (!rc) rc = run_call(e, st, s);
    if (rc) {  // nothing was launched
        e->per_env = was_per_env;
        e->predrawn = was_predrawn;
        return rc;
    }
    e->done_seq += 1;
    StepCall rs = reset_call(e, nullptr, d_reset_exo_days, d_reset_exo_z, d_packed);
    rs.out = packed_out(e, d_packed);
    rs.dmask = mask;
    rs.skip_count = count;
    rs.final_obs = d_final_obs;
    return run_call(e, rs, s);
}

// the launch forms of one reset / step (plan_call of chub_plan.h) for a handle of this shape, without a device
int chub_call_plan(const chub_config *cfg, int64_t n_envs, int rng_mode, const chub_options *opt_in, int env_params, uint32_t flags, int32_t *out) {
    if (!cfg || !out) return fail(CHUB_ERR_ARG, "null argument");
    chub_options opt;
    memset(&opt, 0, sizeof opt);
    if (opt_in) opt = *opt_in;
    LaunchPlan p;
    const char *msg = nullptr;
    if (const int rc = plan_handle(cfg, n_envs, rng_mode, opt, p, &msg)) return fail(rc, msg);
    if (env_params)
        if (const int rc = plan_params(p, rng_mode, &msg)) return fail(rc, msg);
    CallState c = {};
    c.reset = (flags & CHUB_CALL_RESET) != 0;
    c.per_env = (flags & CHUB_CALL_PER_ENV) != 0;
    c.all_served = (flags & CHUB_CALL_ALL_SERVED) != 0;
    c.dev_mask = (flags & CHUB_CALL_DEV_MASK) != 0;
    c.fresh = (flags & CHUB_CALL_FRESH) != 0;
    c.bits = (flags & CHUB_CALL_BITS) != 0;
    c.load_mode = (flags & CHUB_CALL_LOAD) != 0;
    c.capturing = (flags & CHUB_CALL_CAPTURING) != 0;
    c.env_params = env_params != 0;
    const CallPlan r = plan_call(p, c);
    out[CHUB_CALLPLAN_CALL] = r.call;
    out[CHUB_CALLPLAN_ONE] = r.one;
    out[CHUB_CALLPLAN_SLOT] = r.slot;
    out[CHUB_CALLPLAN_LEVELS] = r.levels;
    out[CHUB_CALLPLAN_ENV] = r.env;
    return CHUB_OK;
}

// the scalar-load step on a subset of the envs (every reference env can take evs_step(float) on its own, CHS.hpp:1169-1186 / 1480-1497)
int chub_step_load_envs_device(chub_env *e, const uint8_t *mask, const float *d_actions, const double *d_exo_z, float *d_obs, float *d_reward,
                               uint8_t *d_done, void *stream) {
    if (!e || !mask || !d_actions || !d_obs || !d_reward || !d_done) return fail(CHUB_ERR_ARG, "null argument");
    return run_call(e, step_call(mask, d_actions, d_exo_z, dense_out(e, d_obs, d_reward, d_done), 1), (hipStream_t) stream);
}

int chub_step_gather(chub_env *e, chub_comm *comm, const float *d_actions, float *d_packed, float *d_gathered, void *stream) {
    if (!e || !comm || !d_actions) return fail(CHUB_ERR_ARG, "null argument");
    // (overlapped gathers, chub_comm_set_overlap: the gather that last sent this block must have left before the kernels overwrite it;
    // a capture remembers the communicator so that chub_graph_end can join its stream)
    // the ROOT's kernels write its packed block straight into the gathered buffer (its first n_envs rows): no copy of the root's own block, neither
    // by a send to itself nor otherwise; d_packed is not touched there (may be null).  Every other rank steps into d_packed and sends it.
    const bool root = chub_comm_rank(comm) == 0;
    if (root && !d_gathered) return fail(CHUB_ERR_ARG, "rank 0 needs the gathered buffer");
    if (!root && !d_packed) return fail(CHUB_ERR_ARG, "null argument");
    float *out = root ? d_gathered : d_packed;
    int rc = chub_comm_gather_begin(comm, out, stream);
    if (rc) return rc;
    if (e->capturing) e->cap_comm = comm;
    rc = chub_step_device_packed(e, d_actions, nullptr, out, stream);
    if (rc) return rc;
    return chub_comm_gather(comm, out, d_gathered, e->hp.n_envs * (int64_t) (e->hp.obs_dim + 2) * (int64_t) sizeof(float), stream);
}

// chub_run_steps on a PHILOX handle that runs the one-launch step (k_step_fused): a span of lock-step steps goes out as ONE launch
// (k_steps_fused: the workgroup that owns an env's slots, records and tail goes from step to step by itself).  Not on a tape handle,
// on per-env clocks, under the per-kernel profiler or with chub_options.span_steps = 1.  (The steps of chub_run_steps are row steps
// into the packed block: no tape and no decision bits to look for.)
static bool span_ok(const chub_env *e, int n_batches) {
    return e->plan.one_launch != ONE_NONE && e->plan.span_size_ok && e->plan.span_steps != 1 && !e->per_env && !e->prof_on && !e->tape_only &&
           n_batches <= 8 && e->tick != 0 && !e->hp.telemetry && !e->es.on;
}

static int run_span(chub_env *e, const float *const *batches, int n_batches, float *const *packed2, int64_t first, int k, hipStream_t s) {
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    if (e->t + k > 96) return fail(CHUB_ERR_ARG, "a span of steps ends at the day's end at the latest");
    // the span's first step, as chub_step_device_packed would be asked for it; the kernel moves on through the batches and the two blocks
    const StepCall c = step_call(nullptr, batches[first % n_batches], nullptr, packed_out(e, packed2[first & 1]), 0);
    const MaskView all = {nullptr, 0, e->hp.n_envs - 1};
    StepArgs sa;
    if (const int rc = fill_args(e, c, 2, all, e->tick + 1u, s, sa)) return rc;
    launch_steps_fused(e->hp, e->plan, e->d_ctx, sa, s, packed_ptrs(e), k, e->price_count, first, batches, n_batches, packed2);
    HIP_TRY(hipGetLastError());
    e->tick += (uint32_t) k;
    advance_clocks(e, c, 2, k);
    return note_served(e, nullptr, 2, s);
}

// chub_run_steps on a handle whose pairs of steps share one tail launch (plan_pair_handle / plan_pair_call): n_pairs pairs from step `first`, all
// within the handle's day.  Every pair is slot(i), slot(i + 1), tails(i and i + 1); the first is preceded by the draws no earlier launch has
// left, the last leaves the handle as single steps would (launch_pair).
static bool pairs_ok(const chub_env *e, const chub_comm *comm) {
    PairState c;
    c.comm = comm != nullptr;
    c.per_env = e->per_env;
    c.tape = e->tape_only;
    c.outputs = e->st_out != nullptr || e->es.on != 0 || e->hp.telemetry != 0;
    c.profiling = e->prof_on;
    return plan_pair_call(e->pair_tails, c) && e->tick != 0;
}

static int run_pairs(chub_env *e, const float *const *batches, int n_batches, float *const *packed2, int64_t first, int64_t n_pairs, hipStream_t s) {
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    const MaskView all = {nullptr, 0, e->hp.n_envs - 1};
    int sel = 0;
    for (int64_t p = 0; p < n_pairs; p++) {
        const int64_t i = first + 2 * p;
        const StepCall c1 = step_call(nullptr, batches[i % n_batches], nullptr, packed_out(e, packed2[i & 1]), 0);
        const StepCall c2 = step_call(nullptr, batches[(i + 1) % n_batches], nullptr, packed_out(e, packed2[(i + 1) & 1]), 0);
        StepArgs sa, sb;
        if (const int rc = fill_args(e, c1, 2, all, e->tick + 1u, s, sa)) return rc;
        {   // the second step's arguments: as the handle will stand behind the first
            const int t0 = e->t, pc0 = e->price_count;
            const bool pd0 = e->predrawn;
            e->t = t0 + 1;
            e->price_count = pc0 + 1;
            e->predrawn = true;
            const int rc = fill_args(e, c2, 2, all, e->tick + 2u, s, sb);
            e->t = t0;
            e->price_count = pc0;
            e->predrawn = pd0;
            if (rc) return rc;
        }
        launch_pair(e->hp, e->d_ctx, sa, sb, s, packed_ptrs(e), e->pair, sel, p == 0, p + 1 < n_pairs);
        if (hipGetLastError() != hipSuccess) {
            e->predrawn = false;
            return fail(CHUB_ERR_HIP, "a pair of steps could not be launched");
        }
        e->tick += 2u;
        advance_clocks(e, c1, 2, 2);
        sel ^= 1;
    }
    return note_served(e, nullptr, 2, s);
}

// A run of steps issued from C: what a host loop of chub_reset_device / chub_step_device_packed / chub_step_gather calls does, without
// a trip through the host language per step (multi-GPU shards of a few thousand envs are otherwise bound by the host's issue rate)
int chub_run_steps(chub_env *e, chub_comm *comm, const float *const *d_action_batches, int n_batches, float *const *d_packed2,
                   float *const *d_gathered2, float *d_reset_obs, int64_t first_step, int64_t n_steps, void *stream) {
    if (!e || !d_action_batches || n_batches <= 0 || !d_packed2 || !d_packed2[0] || !d_packed2[1] || !d_reset_obs || first_step < 0 ||
        n_steps < 0)
        return fail(CHUB_ERR_ARG, "bad argument");
    for (int64_t i = first_step; i < first_step + n_steps; i++) {
        int rc;
        if (i % 96 == 0 && (rc = chub_reset_device(e, nullptr, nullptr, d_reset_obs, stream))) return rc;
        // PAIRS of steps with one tail launch (k_env_pair) where the plan says so: up to the day's end or the call's, an odd step out by the paths below
        if (pairs_ok(e, comm)) {
            const int64_t k2 = pair_steps(e->t, std::min<int64_t>(first_step + n_steps - i, 96 - i % 96));
            if (k2 >= 2) {
                if ((rc = run_pairs(e, d_action_batches, n_batches, d_packed2, i, k2 / 2, (hipStream_t) stream))) return rc;
                i += k2 - 1;
                continue;
            }
        }
        // a SPAN of steps in ONE launch (k_steps_fused) where the handle runs the one-launch step anyway: up to the day's end or the call's
        if (!comm) {
            int64_t k = first_step + n_steps - i;
            k = k < 96 - i % 96 ? k : 96 - i % 96;
            k = k < 96 - e->t ? k : 96 - e->t;  // (the handle's own clock need not be i % 96: a caller may step on past `done` -- the span ends where the clock wraps)
            if (e->plan.span_steps > 1 && k > e->plan.span_steps) k = e->plan.span_steps;
            if (k >= 2 && span_ok(e, n_batches)) {
                if ((rc = run_span(e, d_action_batches, n_batches, d_packed2, i, (int) k, (hipStream_t) stream))) return rc;
                i += k - 1;
                continue;
            }
        }
        const float *act = d_action_batches[i % n_batches];
        float *packed = d_packed2[i & 1];
        if (comm) rc = chub_step_gather(e, comm, act, packed, d_gathered2 ? d_gathered2[i & 1] : nullptr, stream);
        else rc = chub_step_device_packed(e, act, nullptr, packed, stream);
        if (rc) return rc;
    }
    return CHUB_OK;
}

// slot of day (and, if asked, the Philox tick of the last launch) of every env
static int fetch_clocks(chub_env *e, std::vector<uint16_t> &c) {
    const size_t N = (size_t) e->hp.n_envs;
    c.assign(N, (uint16_t) ((uint32_t) e->t | (((uint32_t) e->price_count & 3u) << 8)));
    if (!e->per_env) return CHUB_OK;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    // the buffer the next launch reads
    HIP_TRY(hipMemcpy(c.data(), e->d_env_clk + (size_t) ((e->tick + 1u - e->graph_base) & 1u) * N, N * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return CHUB_OK;
}

int chub_env_clocks(chub_env *e, int32_t *t_out, uint32_t *tick_out) {
    if (!e || !t_out) return fail(CHUB_ERR_ARG, "null argument");
    const size_t N = (size_t) e->hp.n_envs;
    std::vector<uint16_t> c;
    int rc = fetch_clocks(e, c);
    if (rc) return rc;
    if (e->per_env && tick_out) {  // what the device-mask launches noted of whom they served (the device is idle: fetch_clocks synchronised)
        std::vector<uint32_t> note(N);
        HIP_TRY(hipMemcpy(note.data(), e->d_tick_note, N * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (e->h_tick.size() != N) e->h_tick.assign(N, 0u);
        for (size_t i = 0; i < N; i++)
            if (note[i] > e->h_tick[i]) e->h_tick[i] = note[i];
    }
    for (size_t i = 0; i < N; i++) {
        t_out[i] = (int32_t) (c[i] & 127u);
        if (tick_out) tick_out[i] = (e->h_tick.size() == N && e->h_tick[i] > e->full_tick) ? e->h_tick[i] : e->full_tick;
    }
    return CHUB_OK;
}

int chub_clock_groups(chub_env *e) {  // number of distinct clocks among the envs
    if (!e) return CHUB_ERR_ARG;
    std::vector<uint16_t> c;
    int rc = fetch_clocks(e, c);
    if (rc) return rc;
    std::sort(c.begin(), c.end());
    return (int) (std::unique(c.begin(), c.end()) - c.begin());
}

// ---- chub_copy_envs: env dst_idx[i] of `dst` becomes a clone of env src_idx[i] of `src`, on the device (k_copy_envs) ------------------------
// The kernel moves the state; what the handle keeps on the host ABOUT that state is settled here, exactly as after a masked call or a
// restored snapshot: the draws a launch made ahead for the next step (pk; the COMPAT walk's shadow, var, fa, hv_pre) and the counts a pass
// left (empt, empt2, shrt) belong to the destination's old state, so the next launch makes and counts its own (StepArgs::fresh,
// empt_fresh; a walk that ran ahead is void).  Nothing of them is reused and nothing is copied approximately.

static const char *copy_refuse_handle(const chub_env *e) {
    if (e->tape_only) return "chub_copy_envs is not supported on a tape handle (chub_tape_register_soc)";
    if (e->capturing) return "chub_copy_envs between chub_graph_begin and chub_graph_end (a copy cannot be recorded: call it between replays)";
    return nullptr;
}

static int copy_check_handles(const chub_env *dst, const chub_env *src) {
    for (const chub_env *e : {dst, src})
        if (const char *why = copy_refuse_handle(e)) return fail(CHUB_ERR_UNSUPPORTED, why);
    if (src == dst) return CHUB_OK;
    if (src->device != dst->device) return fail(CHUB_ERR_ARG, "chub_copy_envs: the two handles live on different devices");
    if (src->public_mode != dst->public_mode) return fail(CHUB_ERR_ARG, "chub_copy_envs: the two handles have different RNG modes");
    const chub_config &a = src->cfg, &b = dst->cfg;
    if (a.station_list[0] != b.station_list[0] || a.station_list[1] != b.station_list[1] || a.station_type_list[0] != b.station_type_list[0] ||
        a.station_type_list[1] != b.station_type_list[1] || (a.constant_charging != 0) != (b.constant_charging != 0))
        return fail(CHUB_ERR_ARG, "chub_copy_envs: the two handles differ in station_list, station_type_list or constant_charging");
    if (src->env_params != dst->env_params)
        return fail(CHUB_ERR_ARG, "chub_copy_envs: one handle has per-env hub parameters (chub_create_params) and the other has none");
    if ((src->es.on != 0) != (dst->es.on != 0))
        return fail(CHUB_ERR_ARG, "chub_copy_envs: one handle keeps the episode ledger (chub_set_episode_stats) and the other does not");
    if (!src->env_params &&
        (a.hydro_prod_rate != b.hydro_prod_rate || a.hydro_store_vlt != b.hydro_store_vlt || a.init_soc != b.init_soc || a.fc_max_power != b.fc_max_power ||
         a.fcev_permeate != b.fcev_permeate || a.renew_fluctuate != b.renew_fluctuate || a.price_fluctuate != b.price_fluctuate || a.hydro_loss != b.hydro_loss))
        return fail(CHUB_ERR_ARG, "chub_copy_envs: the two handles were created with different chub_config scalars (a clone must be the same hub)");
    return CHUB_OK;
}

static uint16_t lock_step_clock(const chub_env *e) { return (uint16_t) ((uint32_t) e->t | (((uint32_t) e->price_count & 3u) << 8)); }

// the launch and the handle's bookkeeping behind it.  keep_clocks: the caller has shown that no destination's clock changes (both handles
// in lock-step on equal clocks): the destination stays in lock-step; otherwise it goes onto per-env clocks as a masked call does
static int copy_launch(chub_env *dst, chub_env *src, const int64_t *d_src_idx, const int64_t *d_dst_idx, int64_t count, hipStream_t s, bool keep_clocks) {
    HIP_TRY(hipSetDevice(dst->device));
    (void) hipGetLastError();
    if (const int rc = sync_ctx(src, s)) return rc;
    if (const int rc = sync_ctx(dst, s)) return rc;
    const size_t Nd = (size_t) dst->hp.n_envs, Ns = (size_t) src->hp.n_envs;
    if (!keep_clocks && !dst->per_env) {  // (as serve_mask: every env starts from the lock-step clock, in the buffer the next launch reads)
        launch_fill_clocks(dst->d_env_clk + (size_t) ((dst->tick + 1u - dst->graph_base) & 1u) * Nd, (int64_t) Nd, lock_step_clock(dst), s);
        dst->per_env = true;
        if (dst->h_tick.size() != Nd) dst->h_tick.assign(Nd, 0u);
    }
    CopyArgs a;
    memset(&a, 0, sizeof a);
    a.src = src->d_ctx;
    a.dst = dst->d_ctx;
    a.src_idx = d_src_idx;
    a.dst_idx = d_dst_idx;
    a.count = count;
    a.src_clk = src->per_env ? src->d_env_clk + (size_t) ((src->tick + 1u - src->graph_base) & 1u) * Ns : nullptr;
    a.dst_clk = keep_clocks ? nullptr : dst->d_env_clk + (size_t) ((dst->tick + 1u - dst->graph_base) & 1u) * Nd;
    a.src_clk_value = lock_step_clock(src);
    a.src_rng = src->rng_cur;
    a.dst_rng = dst->rng_cur;
    a.src_rows = (const double *) src->d_rows;
    a.dst_rows = (double *) dst->d_rows;
    launch_copy_envs(slot_layout(dst->hp), a, s);
    HIP_TRY(hipGetLastError());
    dst->predrawn = false;   // pk was decoded against the old queues (and a row may have come along): the next launch draws its own
    dst->walked_tick = 0;    // COMPAT: a walk that ran ahead of its step walked the old state
    dst->empt_valid = false; // ... and the counts the last pass left are the old slots'
    dst->e2_tick = ~0u;
    return CHUB_OK;
}

int chub_copy_envs_device(chub_env *dst, chub_env *src, const int64_t *d_src_idx, const int64_t *d_dst_idx, int64_t count, void *stream) {
    if (!dst || !src || !d_src_idx || !d_dst_idx) return fail(CHUB_ERR_ARG, "null argument");
    if (count < 0) return fail(CHUB_ERR_ARG, "count < 0");
    if (const int rc = copy_check_handles(dst, src)) return rc;
    if (count == 0) return CHUB_OK;
    return copy_launch(dst, src, d_src_idx, d_dst_idx, count, (hipStream_t) stream, false);
}

int chub_copy_envs(chub_env *dst, chub_env *src, const int64_t *src_idx, const int64_t *dst_idx, int64_t count) {
    if (!dst || !src || !src_idx || !dst_idx) return fail(CHUB_ERR_ARG, "null argument");
    if (count < 0) return fail(CHUB_ERR_ARG, "count < 0");
    if (const int rc = copy_check_handles(dst, src)) return rc;
    if (count == 0) return CHUB_OK;
    const int64_t Ns = src->hp.n_envs, Nd = dst->hp.n_envs;
    std::vector<uint8_t> is_dst((size_t) Nd, 0);
    for (int64_t i = 0; i < count; i++) {
        const std::string at = "[" + std::to_string(i) + "] = ";
        if (src_idx[i] < 0 || src_idx[i] >= Ns)
            return fail(CHUB_ERR_ARG, "src_idx" + at + std::to_string(src_idx[i]) + " is out of range (the source handle has " + std::to_string(Ns) + " envs)");
        if (dst_idx[i] < 0 || dst_idx[i] >= Nd)
            return fail(CHUB_ERR_ARG, "dst_idx" + at + std::to_string(dst_idx[i]) + " is out of range (the destination handle has " + std::to_string(Nd) + " envs)");
        if (is_dst[(size_t) dst_idx[i]])
            return fail(CHUB_ERR_ARG, "dst_idx" + at + std::to_string(dst_idx[i]) + " names a destination a second time");
        is_dst[(size_t) dst_idx[i]] = 1;
    }
    for (int64_t i = 0; src == dst && i < count; i++)
        if (is_dst[(size_t) src_idx[i]])
            return fail(CHUB_ERR_ARG, "src_idx[" + std::to_string(i) + "] = " + std::to_string(src_idx[i]) +
                                          " is also a destination (within one handle no env may be both)");
    HIP_TRY(hipSetDevice(dst->device));
    HIP_TRY(hipDeviceSynchronize());  // (launches in flight on any stream read or write these arrays: as the other host-form mutators)
    if (src != dst && src->env_params) {  // the rows come along: each must fit the waiting list `dst` was created with (as chub_set_env_params)
        std::vector<chub_env_params> rows;
        if (const int rc = fetch(rows, (const chub_env_params *) src->d_rows, (size_t) Ns)) return rc;
        for (int64_t i = 0; i < count; i++) {
            const int m = hv_bound(dst->hv_top, derive_env_consts(rows[(size_t) src_idx[i]]).hv_rate);
            if (m > dst->hv_max_arrive)
                return fail(CHUB_ERR_ARG, "src_idx[" + std::to_string(i) + "] = " + std::to_string(src_idx[i]) + ": its fcev_permeate gives up to " +
                                              std::to_string(m) + " FCEV arrivals per step, more than the " + std::to_string(dst->hv_max_arrive) +
                                              " the destination handle's waiting list was sized for at create");
        }
    }
    // both handles in lock-step on equal clocks: no clock changes, the destination stays in lock-step
    const bool keep_clocks = !dst->per_env && !src->per_env && lock_step_clock(src) == lock_step_clock(dst);
    int64_t *d_idx = nullptr;
    HIP_TRY(hipMalloc((void **) &d_idx, 2 * (size_t) count * sizeof(int64_t)));
    int rc = CHUB_OK;
    if (hipMemcpy(d_idx, src_idx, (size_t) count * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_idx + count, dst_idx, (size_t) count * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(CHUB_ERR_HIP, "chub_copy_envs: the indices could not be uploaded");
    if (!rc) rc = copy_launch(dst, src, d_idx, d_idx + count, count, nullptr, keep_clocks);
    const hipError_t he = hipDeviceSynchronize();
    (void) hipFree(d_idx);
    if (!rc && he != hipSuccess) rc = fail(CHUB_ERR_HIP, std::string("chub_copy_envs: ") + hipGetErrorString(he));
    return rc;
}

// The output arrays of a host-pointer step, as the device sees them: pinned host memory (hipHostMalloc: chub_alloc_host, what
// VecChargingHub hands in) is mapped into the device's address space, so the tail kernel can store its rows straight into the
// caller's arrays -- they cross PCIe as posted writes while the kernel runs instead of in a copy phase of their own behind it.
// Any other host memory gets the handle's device staging and a copy back.
static bool device_view(void *host, void **dev) {
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, host, 0) != hipSuccess || !d) {
        (void) hipGetLastError();
        return false;
    }
    *dev = d;
    return true;
}

// ---- host-pointer entry points: the reference-shaped API (numpy in / numpy out), bounded by PCIe: (A + D + 2) * 4 bytes per env and
// step.  Each stages its arrays with the helpers below and goes through run_call.  chub_step and chub_step_bits work on a private
// stream with async copies; every other one on the null stream with blocking copies.

static int host_path_init(chub_env *e) {
    if (e->host_stream) return CHUB_OK;
    const size_t N = (size_t) e->hp.n_envs, A = (size_t) e->hp.act_dim;
    HIP_TRY(hipStreamCreateWithFlags(&e->host_stream, hipStreamNonBlocking));
    HIP_TRY(hipHostMalloc((void **) &e->h_actions, N * A * sizeof(float), hipHostMallocDefault));
    return CHUB_OK;
}

int chub_host_actions(chub_env *e, float **out) {
    if (!e || !out) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    int rc = host_path_init(e);
    if (rc) return rc;
    *out = e->h_actions;
    return CHUB_OK;
}

// One input array on its way to the device.  s null: a blocking copy into the handle's staging `d_stage`; otherwise an async copy on s --
// from the handle's pinned buffers (chub_host_actions, chub_host_bits) one DMA, any other host pointer is staged by the HIP runtime.
// in_place: pinned host memory is not copied at all, the kernels READ it where it is.  d_in: what the kernels are given
static int upload(void *d_stage, const void *host, size_t bytes, hipStream_t s, bool in_place, const void **d_in) {
    void *v = nullptr;
    if (in_place && device_view((void *) host, &v)) {
        *d_in = v;
        return CHUB_OK;
    }
    if (s) HIP_TRY(hipMemcpyAsync(d_stage, host, bytes, hipMemcpyHostToDevice, s));
    else HIP_TRY(hipMemcpy(d_stage, host, bytes, hipMemcpyHostToDevice));
    *d_in = d_stage;
    return CHUB_OK;
}

// Where a host-pointer step stores: pinned output arrays (try_direct, see device_view) are written by the tail kernel itself;
// any other host memory gets the handle's device staging and fetch_out behind the launch
static OutSink host_out(const chub_env *e, float *obs, float *reward, uint8_t *done, bool try_direct, bool &direct) {
    void *v_obs = nullptr, *v_rew = nullptr, *v_done = nullptr;
    direct = try_direct && device_view(obs, &v_obs) && device_view(reward, &v_rew) && device_view(done, &v_done);
    return direct ? dense_out(e, (float *) v_obs, (float *) v_rew, (uint8_t *) v_done) : dense_out(e, e->d_obs, e->d_reward, e->d_done);
}

// ... the copy back from that staging (on s, or blocking: as upload).  mask: only the rows of the envs it names are written;
// reward and done null: a reset's obs alone
static int fetch_out(chub_env *e, const uint8_t *mask, float *obs, float *reward, uint8_t *done, hipStream_t s) {
    const size_t N = (size_t) e->hp.n_envs, D = (size_t) e->hp.obs_dim;
    auto back = [s](void *dst, const void *src, size_t bytes) {
        return s ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    };
    if (!mask) {
        HIP_TRY(back(obs, e->d_obs, N * D * sizeof(float)));
        if (reward) HIP_TRY(back(reward, e->d_reward, N * sizeof(float)));
        if (done) HIP_TRY(back(done, e->d_done, N));
        return CHUB_OK;
    }
    std::vector<float> o(N * D), r(N);
    std::vector<uint8_t> d(N);
    HIP_TRY(hipMemcpy(o.data(), e->d_obs, N * D * sizeof(float), hipMemcpyDeviceToHost));
    if (reward) HIP_TRY(hipMemcpy(r.data(), e->d_reward, N * sizeof(float), hipMemcpyDeviceToHost));
    if (done) HIP_TRY(hipMemcpy(d.data(), e->d_done, N, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; i++)
        if (mask[i]) {
            memcpy(obs + i * D, &o[i * D], D * sizeof(float));
            if (reward) reward[i] = r[i];
            if (done) done[i] = d[i];
        }
    return CHUB_OK;
}

// a reset's PV / wind days (REN:51-53) index the 100 x 96 and 150 x 96 tables; mask: the values of the envs outside it are not looked at
static int check_exo_days(const chub_env *e, const uint8_t *mask, const int32_t *exo_days) {
    for (size_t i = 0; i < (size_t) e->hp.n_envs; i++)
        if ((!mask || mask[i]) && (exo_days[2 * i] < 0 || exo_days[2 * i] >= 100 || exo_days[2 * i + 1] < 0 || exo_days[2 * i + 1] >= 150))
            return fail(CHUB_ERR_ARG, "exo_days out of range");
    return CHUB_OK;
}

// chub_reset (mask null) and chub_reset_envs: full-size arrays, only the rows of the named envs are read and written
static int reset_host(chub_env *e, const uint8_t *mask, const int32_t *exo_days, const double *exo_z, float *obs) {
    HIP_TRY(hipSetDevice(e->device));
    const size_t N = (size_t) e->hp.n_envs;
    int rc = check_compat_variates(e, true, exo_days, exo_z);
    if (rc) return rc;
    const void *d_days = e->d_exo_days, *d_z = e->d_exo_z;
    if (e->hp.rng_mode == CHUB_RNG_COMPAT) {
        if ((rc = check_exo_days(e, mask, exo_days))) return rc;
        if ((rc = upload(e->d_exo_days, exo_days, N * 2 * sizeof(int32_t), nullptr, false, &d_days))) return rc;
        if ((rc = upload(e->d_exo_z, exo_z, N * 3 * sizeof(double), nullptr, false, &d_z))) return rc;
    }
    if ((rc = run_call(e, reset_call(e, mask, (const int32_t *) d_days, (const double *) d_z, e->d_obs), nullptr))) return rc;
    return fetch_out(e, mask, obs, nullptr, nullptr, nullptr);
}

int chub_reset(chub_env *e, const int32_t *exo_days, const double *exo_z, float *obs) {
    if (!e || !obs) return fail(CHUB_ERR_ARG, "null argument");
    return reset_host(e, nullptr, exo_days, exo_z, obs);
}

int chub_reset_envs(chub_env *e, const uint8_t *mask, const int32_t *exo_days, const double *exo_z, float *obs) {
    if (!e || !mask || !obs) return fail(CHUB_ERR_ARG, "null argument");
    return reset_host(e, mask, exo_days, exo_z, obs);
}

// The host-pointer step on rows of actions.  s: the handle's private stream (chub_step: async copies, pinned arrays used where they are, one
// stream synchronisation at the end) or null (blocking copies through the staging)
static int step_host(chub_env *e, const uint8_t *mask, const float *actions, const double *exo_z, float *obs, float *reward, uint8_t *done,
                     int load_mode, hipStream_t s) {
    int rc = check_compat_variates(e, false, nullptr, exo_z);
    if (rc) return rc;
    const size_t N = (size_t) e->hp.n_envs, A = (size_t) e->hp.act_dim;
    // A handful of envs (the drop-in class: one): inputs that sit in pinned host memory are READ BY THE KERNELS where they are -- a
    // few hundred bytes over PCIe -- instead of going through a copy engine first: the step is then one launch set and one
    // stream synchronisation, no copy in either direction.  Larger batches and pageable memory take the DMA as before.
    const bool tiny = s && N * A * sizeof(float) <= 16384;
    const void *d_z = e->d_exo_z, *d_act = nullptr;
    if (e->hp.rng_mode == CHUB_RNG_COMPAT && (rc = upload(e->d_exo_z, exo_z, N * 3 * sizeof(double), s, tiny, &d_z))) return rc;
    if ((rc = upload(e->d_actions, actions, N * A * sizeof(float), s, tiny, &d_act))) return rc;
    bool direct = false;
    const OutSink out = host_out(e, obs, reward, done, s != nullptr, direct);
    if ((rc = run_call(e, step_call(mask, (const float *) d_act, (const double *) d_z, out, load_mode), s))) return rc;
    if (!direct && (rc = fetch_out(e, mask, obs, reward, done, s))) return rc;
    if (s) HIP_TRY(hipStreamSynchronize(s));
    return CHUB_OK;
}

int chub_step(chub_env *e, const float *actions, const double *exo_z, float *obs, float *reward, uint8_t *done) {
    if (!e || !actions || !obs || !reward || !done) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    if (const int rc = host_path_init(e)) return rc;
    return step_host(e, nullptr, actions, exo_z, obs, reward, done, 0, e->host_stream);
}

int chub_step_load(chub_env *e, const float *actions, const double *exo_z, float *obs, float *reward, uint8_t *done) {
    if (!e || !actions || !obs || !reward || !done) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    return step_host(e, nullptr, actions, exo_z, obs, reward, done, 1, nullptr);
}

int chub_step_envs(chub_env *e, const uint8_t *mask, const float *actions, const double *exo_z, float *obs, float *reward, uint8_t *done) {
    if (!e || !mask || !actions || !obs || !reward || !done) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    return step_host(e, mask, actions, exo_z, obs, reward, done, 0, nullptr);
}

int chub_step_load_envs(chub_env *e, const uint8_t *mask, const float *actions, const double *exo_z, float *obs, float *reward, uint8_t *done) {
    if (!e || !mask || !actions || !obs || !reward || !done) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    return step_host(e, mask, actions, exo_z, obs, reward, done, 1, nullptr);
}

// ---- packed-action form of the host-pointer step: one bit per pile + the two tail floats (16 bytes per env for hubs of up to
// 64 piles instead of 4 * (S + 2)): what action_to_real (MGR:384-393) keeps of an action row.  The packed slot kernel reads
// the bits themselves (k_slot_packed<.., BITS>: the same step with another action load, bit for bit chub_step's results); for the
// other kernels they are expanded on the device into the action rows those read.
static int bits_path_init(chub_env *e) {
    int rc = host_path_init(e);
    if (rc || e->h_bits) return rc;
    const size_t N = (size_t) e->hp.n_envs, W = (size_t) ((e->hp.S[0] + e->hp.S[1] + 63) / 64);
    // bits and tail in ONE pinned block and one device block: a caller that fills the handle's staging goes up in a single DMA
    HIP_TRY(hipHostMalloc((void **) &e->h_bits, N * W * sizeof(uint64_t) + N * 2 * sizeof(float), hipHostMallocDefault));
    e->h_tail = (float *) (e->h_bits + N * W);
    HIP_TRY(hipMalloc((void **) &e->d_bits, N * W * sizeof(uint64_t) + N * 2 * sizeof(float)));
    e->d_tail = (float *) (e->d_bits + N * W);
    return CHUB_OK;
}

int chub_host_bits(chub_env *e, uint64_t **bits_out, float **tail_out) {
    if (!e || !bits_out || !tail_out) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    int rc = bits_path_init(e);
    if (rc) return rc;
    *bits_out = e->h_bits;
    *tail_out = e->h_tail;
    return CHUB_OK;
}

static StepCall bits_call(const uint64_t *d_pile_bits, const float *d_tail, const double *d_exo_z, const OutSink &out) {
    StepCall c = step_call(nullptr, nullptr, d_exo_z, out, 0);
    c.bits = d_pile_bits;
    c.tail = d_tail;
    return c;
}

int chub_step_bits_device(chub_env *e, const uint64_t *d_pile_bits, const float *d_tail, const double *d_exo_z, float *d_obs,
                          float *d_reward, uint8_t *d_done, void *stream) {
    if (!e || !d_pile_bits || !d_tail || !d_obs || !d_reward || !d_done) return fail(CHUB_ERR_ARG, "null argument");
    return run_call(e, bits_call(d_pile_bits, d_tail, d_exo_z, dense_out(e, d_obs, d_reward, d_done)), (hipStream_t) stream);
}

int chub_step_bits_device_packed(chub_env *e, const uint64_t *d_pile_bits, const float *d_tail, const double *d_exo_z, float *d_packed,
                                 void *stream) {
    if (!e || !d_pile_bits || !d_tail || !d_packed) return fail(CHUB_ERR_ARG, "null argument");
    return run_call(e, bits_call(d_pile_bits, d_tail, d_exo_z, packed_out(e, d_packed)), (hipStream_t) stream);
}

int chub_step_bits(chub_env *e, const uint64_t *pile_bits, const float *tail, const double *exo_z, float *obs, float *reward,
                   uint8_t *done) {
    if (!e || !pile_bits || !tail || !obs || !reward || !done) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    int rc = bits_path_init(e);
    if (rc) return rc;
    if ((rc = check_compat_variates(e, false, nullptr, exo_z))) return rc;
    const size_t N = (size_t) e->hp.n_envs, W = (size_t) ((e->hp.S[0] + e->hp.S[1] + 63) / 64);
    const size_t n_bits = N * W * sizeof(uint64_t), n_tail = N * 2 * sizeof(float);
    hipStream_t s = e->host_stream;
    const void *d_z = e->d_exo_z, *d_bits = nullptr, *d_tail = e->d_tail;
    if (e->hp.rng_mode == CHUB_RNG_COMPAT && (rc = upload(e->d_exo_z, exo_z, N * 3 * sizeof(double), s, false, &d_z))) return rc;
    // from the handle's pinned block (chub_host_bits) bits and tail go up in ONE DMA
    const bool one_block = pile_bits == e->h_bits && tail == e->h_tail;
    if ((rc = upload(e->d_bits, pile_bits, one_block ? n_bits + n_tail : n_bits, s, false, &d_bits))) return rc;
    if (!one_block && (rc = upload(e->d_tail, tail, n_tail, s, false, &d_tail))) return rc;
    bool direct = false;
    const OutSink out = host_out(e, obs, reward, done, true, direct);
    if ((rc = run_call(e, bits_call((const uint64_t *) d_bits, (const float *) d_tail, (const double *) d_z, out), s))) return rc;
    if (!direct && (rc = fetch_out(e, nullptr, obs, reward, done, s))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return CHUB_OK;
}

// ---- hipGraph capture of whole episodes (launch-bound loops: small shards, multi-GPU strong scaling) -----------------------
struct chub_graph {
    hipGraph_t graph;
    hipGraphExec_t exec;
    int device;
    chub_env *env;
    uint32_t ticks;       // resets + steps one replay covers
    uint32_t arg0;        // host tick - tick base at chub_graph_begin: the captured launches carry arg0 + 1 .. arg0 + ticks
    int t_begin, pc_begin;  // the handle's clocks at chub_graph_begin: what a replay starts from (baked into the launches)
    bool per_env_begin, per_env_end, predrawn_end;  // captured on per-env clocks (device state: nothing of them is baked in)
    std::vector<void *> masks;        // device masks of the captured calls on subsets of the envs
    std::vector<uint32_t> rel;        // [N] or empty: launch number within the graph of every env's last masked launch
    uint32_t full_rel;                // launch number of the graph's last launch on every env
    int t_end, pc_end;    // the handle's clocks after a replay
};

int chub_graph_begin(chub_env *e, void *stream) {
    if (!e || !stream) return fail(CHUB_ERR_ARG, "chub_graph_begin needs a handle and a created (non-default) stream");
    if (e->capturing) return fail(CHUB_ERR_ARG, "a capture is already in progress on this handle");
    if (e->hp.rng_mode != CHUB_RNG_PHILOX) return fail(CHUB_ERR_ARG, "graphs replay PHILOX steps (COMPAT takes host draws every step)");
    if (e->prof_on) return fail(CHUB_ERR_ARG, "per-kernel profiling is on");
    HIP_TRY(hipSetDevice(e->device));
    int rc = sync_ctx(e, (hipStream_t) stream);
    if (rc) return rc;
    HIP_TRY(hipStreamBeginCapture((hipStream_t) stream, hipStreamCaptureModeRelaxed));
    e->capturing = true;
    e->graph_tick0 = e->tick;
    e->graph_t0 = e->t;
    e->graph_pc0 = e->price_count;
    e->graph_predrawn0 = e->predrawn;
    e->graph_per_env0 = e->per_env;
    e->graph_full_tick0 = e->full_tick;
    e->graph_h_tick0 = e->h_tick;
    e->cap_masks.clear();
    e->cap_rel.clear();
    e->cap_full_rel = 0;
    e->cap_comm = nullptr;
    return CHUB_OK;
}

int chub_graph_end(chub_env *e, void *stream, chub_graph **out) {
    if (!e || !stream || !out) return fail(CHUB_ERR_ARG, "null argument");
    if (!e->capturing) return fail(CHUB_ERR_ARG, "no capture in progress");
    *out = nullptr;
    e->capturing = false;
    const uint32_t ticks = e->tick - e->graph_tick0;
    const int t_end = e->t, pc_end = e->price_count;
    const bool per_env_end = e->per_env, predrawn_end = e->predrawn;
    std::vector<void *> masks;
    masks.swap(e->cap_masks);
    auto drop_masks = [&]() {
        for (void *m : masks) (void) hipFree(m);
    };
    // nothing ran: the handle is where it was at chub_graph_begin; every chub_graph_launch moves it on by one replay
    e->tick = e->graph_tick0;
    e->t = e->graph_t0;
    e->price_count = e->graph_pc0;
    e->predrawn = e->graph_predrawn0;
    e->per_env = e->graph_per_env0;
    e->full_tick = e->graph_full_tick0;
    e->h_tick = e->graph_h_tick0;
    // overlapped gathers ran on the communicator's stream: it joins the capture's stream here (a capture ends on one stream; and the
    // next replay's first kernels overwrite the blocks the last gathers send)
    if (e->cap_comm) (void) chub_comm_join(e->cap_comm, stream);
    e->cap_comm = nullptr;
    // every replay moves the Philox tick base on by the ticks the graph covers (its last node)
    launch_tick_advance(e->d_tick_base, ticks, (hipStream_t) stream);
    hipGraph_t g = nullptr;
    hipError_t he = hipStreamEndCapture((hipStream_t) stream, &g);
    if (he != hipSuccess || !g) {
        drop_masks();
        return fail(CHUB_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(he));
    }
    if (ticks == 0 || (ticks & 1u)) {
        (void) hipGraphDestroy(g);
        drop_masks();
        return fail(CHUB_ERR_ARG, "a graph must cover an even, non-zero number of resets + steps (double-buffered draws)");
    }
    hipGraphExec_t x = nullptr;
    he = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
    if (he != hipSuccess) {
        (void) hipGraphDestroy(g);
        drop_masks();
        return fail(CHUB_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(he));
    }
    chub_graph *cg = new chub_graph();
    cg->graph = g;
    cg->exec = x;
    cg->device = e->device;
    cg->env = e;
    cg->ticks = ticks;
    cg->arg0 = e->graph_tick0 - e->graph_base;
    cg->t_begin = e->graph_t0;
    cg->pc_begin = e->graph_pc0;
    cg->per_env_begin = e->graph_per_env0;
    cg->per_env_end = per_env_end;
    cg->predrawn_end = predrawn_end;
    cg->masks.swap(masks);
    cg->rel.swap(e->cap_rel);
    cg->full_rel = e->cap_full_rel;
    cg->t_end = t_end;
    cg->pc_end = pc_end;
    *out = cg;
    return CHUB_OK;
}

int chub_graph_launch(chub_graph *g, void *stream) {
    if (!g) return fail(CHUB_ERR_ARG, "null graph");
    HIP_TRY(hipSetDevice(g->device));
    chub_env *e = g->env;
    if (e->capturing) return fail(CHUB_ERR_ARG, "a capture is in progress on this handle");
    if (g->per_env_begin != e->per_env)
        return fail(CHUB_ERR_ARG, g->per_env_begin ? "this graph was captured on per-env clocks: the handle is in lock-step (make a call on a subset of the envs first)"
                                                   : "this graph replays lock-step calls: the envs of this handle run on their own clocks (reset all of them first)");
    // a lock-step replay repeats the clocks of its launches verbatim (slot of day, price-noise phase: kernel arguments): it
    // continues the handle's run only from where the capture started.  On per-env clocks the clocks are device state and a replay
    // continues from wherever every env is.
    if (!g->per_env_begin && (e->t != g->t_begin || ((e->price_count ^ g->pc_begin) & 3) != 0))
        return fail(CHUB_ERR_ARG, "the handle is not at the clock this graph was captured at (slot of day " + std::to_string(g->t_begin) +
                                      ", steps since reset mod 4 = " + std::to_string(g->pc_begin & 3) + "): a replay bakes the clocks in");
    // The captured launches carry the arguments arg0 + 1 .. arg0 + ticks, and a launch's effective Philox tick is its argument
    // + the device-side tick base.  Calls issued one by one since the capture (or since the last replay) have moved the host
    // tick on without moving the base: bring the base to where argument arg0 + k means tick + k again, so that a replay never
    // runs on a tick an eager call has already used (nor the other way round).
    const uint32_t delta = (e->tick - e->graph_base) - g->arg0;
    if (delta != 0u) {
        // The per-env clocks are double-buffered by the parity of that same argument: the graph's first launch reads buffer
        // (arg0 + 1) & 1, while the live clocks -- after an odd number of eager calls -- sit in buffer (arg0 + delta + 1) & 1,
        // the other one.  Bring them over before the base moves (every env would otherwise replay from a stale slot
        // of day and price phase).
        if (g->per_env_begin && (delta & 1u)) {
            const size_t N = (size_t) e->hp.n_envs;
            launch_keep_clocks(e->d_env_clk + (size_t) ((g->arg0 + 1u) & 1u) * N, e->d_env_clk + (size_t) (g->arg0 & 1u) * N, (int64_t) N,
                               (hipStream_t) stream);
        }
        launch_tick_advance(e->d_tick_base, delta, (hipStream_t) stream);
        HIP_TRY(hipGetLastError());
        e->graph_base += delta;
    }
    HIP_TRY(hipGraphLaunch(g->exec, (hipStream_t) stream));
    // the replay covers g->ticks resets + steps: its last node moves the device-side tick base on, the host mirrors it, so that
    // calls issued one by one afterwards continue the same tick sequence (their argument is the tick minus the base)
    const uint32_t tick0 = e->tick;
    e->tick += g->ticks;
    e->graph_base += g->ticks;
    e->per_env = g->per_env_end;
    if (!g->per_env_begin || !g->per_env_end) {  // the replay ran on, or ended on, the one clock of the handle
        e->t = g->t_end;
        e->price_count = g->pc_end;
    }
    e->predrawn = g->predrawn_end;
    if (g->full_rel) e->full_tick = tick0 + g->full_rel;
    if (!g->rel.empty()) {
        const size_t N = (size_t) e->hp.n_envs;
        if (e->h_tick.size() != N) e->h_tick.assign(N, 0u);
        for (size_t i = 0; i < N; i++)
            if (g->rel[i]) e->h_tick[i] = tick0 + g->rel[i];
    }
    return CHUB_OK;
}

int chub_graph_destroy(chub_graph *g) {
    if (!g) return CHUB_OK;
    (void) hipSetDevice(g->device);
    (void) hipGraphExecDestroy(g->exec);
    (void) hipGraphDestroy(g->graph);
    (void) hipDeviceSynchronize();  // a replay still in flight reads the masks
    for (void *m : g->masks) (void) hipFree(m);
    delete g;
    return CHUB_OK;
}

// ---- device memory and streams for hosts without a GPU array library (the Python host is ctypes + numpy) ----------------
int chub_malloc_device(int device, int64_t bytes, void **out) {
    if (!out || bytes <= 0) return fail(CHUB_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMalloc(out, (size_t) bytes));
    return CHUB_OK;
}
int chub_free_device(int device, void *p) {
    if (!p) return CHUB_OK;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipFree(p));
    return CHUB_OK;
}
int chub_copy_to_host(int device, void *dst, const void *d_src, int64_t bytes, void *stream) {
    if (!dst || !d_src || bytes < 0) return fail(CHUB_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpyAsync(dst, d_src, (size_t) bytes, hipMemcpyDeviceToHost, (hipStream_t) stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t) stream));
    return CHUB_OK;
}
int chub_copy_to_device(int device, void *d_dst, const void *src, int64_t bytes, void *stream) {
    if (!d_dst || !src || bytes < 0) return fail(CHUB_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpyAsync(d_dst, src, (size_t) bytes, hipMemcpyHostToDevice, (hipStream_t) stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t) stream));
    return CHUB_OK;
}
int chub_alloc_host(int device, int64_t bytes, void **out) {
    if (!out || bytes <= 0) return fail(CHUB_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipHostMalloc(out, (size_t) bytes, hipHostMallocDefault));
    return CHUB_OK;
}
int chub_free_host(int device, void *p) {
    if (!p) return CHUB_OK;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipHostFree(p));
    return CHUB_OK;
}
int chub_stream_create(int device, void **out) {
    if (!out) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(device));
    hipStream_t s;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out = (void *) s;
    return CHUB_OK;
}
int chub_stream_destroy(int device, void *stream) {
    if (!stream) return CHUB_OK;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamDestroy((hipStream_t) stream));
    return CHUB_OK;
}
int chub_stream_sync(int device, void *stream) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamSynchronize((hipStream_t) stream));
    return CHUB_OK;
}

// ---- tape mode (parity instrument, PHILOX handles): recorded decisions replayed through the production kernels -------
int chub_tape_register_soc(chub_env *e, const float *soc, int32_t count, uint32_t *class_ids) {
    if (!e || !soc || !class_ids || count < 0) return fail(CHUB_ERR_ARG, "bad argument");
    if (e->env_params) return refuse_params("tape mode (chub_tape_register_soc)");
    if (e->es.on)  // (chub_set_episode_stats refuses a tape handle; a handle that keeps the ledger does not become one either)
        return fail(CHUB_ERR_UNSUPPORTED, "tape mode on a handle that keeps the episode ledger: call chub_set_episode_stats(env, 0) first");
    if (e->hp.rng_mode != CHUB_RNG_PHILOX) return fail(CHUB_ERR_ARG, "tape mode needs a PHILOX handle");
    if (e->hp.soc_curves)
        return fail(CHUB_ERR_UNSUPPORTED, "rng_mode PHILOX_CURVES has no classes: its car tape carries each arrival SoC itself (f32 bits in .x)");
    if (e->tape_classes + count > kSocLevels) return fail(CHUB_ERR_UNSUPPORTED, "too many tape classes (chub_tape_clear_soc starts over)");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    // The state word has room for kSocLevels classes and the production kernel is the one to be replayed, so the caller's arrival
    // SoCs take the PLACE of this build's own classes, first come first row: from here on the handle is a tape handle (cars that a
    // Philox step or reset admits would be given the caller's SoCs)
    const bool cp = e->hp.constant_charging != 0;
    std::vector<float> rows((size_t) count * kClsRow * 2);
    const size_t first = (size_t) e->tape_classes;
    for (int k = 0; k < 2; k++) {  // (checked for the whole batch before anything is overwritten)
        const bool fast = e->hp.type[k] == CHUB_FAST;
        float tt_max = 0.0f;
        for (float t : e->h_ttab[k]) tt_max = t > tt_max ? t : tt_max;
        for (int i = 0; i < count; i++) {
            // stay_time = ceil(soc_to_time(target) - soc_to_time(soc)) + late (late <= 15) must fit the state word's 5-bit fields, as
            // chub_create checks for the build's own classes: an arrival SoC whose stay could not is refused, not clamped
            float row[kClsRow * 2];
            build_class_row(fast, cp, e->hp.cc, soc[i], row);
            if (!(soc[i] >= 0.0f && soc[i] <= 100.0f) || (int) ceilf(tt_max - row[1]) + 15 > kMaxStay)
                return fail(CHUB_ERR_ARG, "chub_tape_register_soc: an arrival SoC whose stay could exceed 31 slots (or outside 0 .. 100)");
        }
    }
    e->tape_only = e->tape_only || count > 0;
    for (int k = 0; k < 2; k++) {
        const bool fast = e->hp.type[k] == CHUB_FAST;
        for (int i = 0; i < count; i++) build_class_row(fast, cp, e->hp.cc, soc[i], &rows[(size_t) i * kClsRow * 2]);
        if (count) {
            HIP_TRY(hipMemcpy((void *) (e->tb.cls[k] + first * kClsRow * 2), rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy((void *) (e->tb.cls_soc0[k] + first), soc, (size_t) count * sizeof(float), hipMemcpyHostToDevice));
        }
    }
    if (count) {  // the SoC table follows the rows it is derived from (chub_get_slots reads it on this handle too)
        if (const int rc = sync_ctx(e, nullptr)) return rc;
        launch_build_cls_soc(e->d_ctx, e->d_cls_soc, nullptr);
        HIP_TRY(hipGetLastError());
    }
    for (int i = 0; i < count; i++) class_ids[i] = (uint32_t) (first + (size_t) i);
    e->tape_classes += count;
    return CHUB_OK;
}

int chub_tape_clear_soc(chub_env *e) {
    if (!e) return fail(CHUB_ERR_ARG, "null handle");
    // the next chub_tape_register_soc starts at class 0 again.  Cars of the old classes still in their slots would be re-read against the
    // new rows: the caller clears between episodes, right in front of the chub_reset_tape that wipes every slot (evs_reset, CHS.hpp:1209-1231),
    // and chub_step_tape refuses to run until that reset has happened
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    e->tape_classes = 0;
    e->tape_stale = true;
    return CHUB_OK;
}

int chub_set_slots(chub_env *e, const int32_t *rows) {
    if (!e || !rows) return fail(CHUB_ERR_ARG, "null argument");
    if (e->hp.rng_mode != CHUB_RNG_PHILOX) return fail(CHUB_ERR_ARG, "chub_set_slots needs a PHILOX handle");
    if (e->hp.soc_curves) return fail(CHUB_ERR_UNSUPPORTED, "chub_set_slots writes class-table slot states: not supported in rng_mode PHILOX_CURVES");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    const HubParams &hp = e->hp;
    const size_t N = (size_t) hp.n_envs, S = (size_t) (hp.S[0] + hp.S[1]);
    std::vector<uint32_t> st(N * S, 0u);
    std::vector<uint8_t> stay(N * S, 0);
    for (size_t env = 0; env < N; env++)
        for (int k = 0; k < 2; k++)
            for (size_t i = 0; i < (size_t) hp.S[k]; i++) {
                const int32_t *r = rows + (env * S + (k ? (size_t) hp.S[0] : 0) + i) * 6;
                if (r[0] < 0) continue;  // empty slot
                const int left = r[2] - r[3];
                if ((uint32_t) r[0] >= (uint32_t) kSocLevels || r[1] < 0 || r[1] >= kLevels || r[2] < 1 || r[2] > kMaxStay || left < 1 || r[4] < 0 ||
                    r[4] >= kClsRow)
                    return fail(CHUB_ERR_ARG, "chub_set_slots: field out of range");
                const size_t idx = env * S + (k ? (size_t) hp.S[0] : 0) + i;  // PHILOX state is hub-major
                // the state word (chub_device.h): a car of that class and level with `left` to go, r[4] car_steps on, charging or not
                st[idx] = ps_make(left, (uint32_t) r[0], (uint32_t) r[1]) | (uint32_t) r[4] * kPsStep | (r[5] ? kPsChg : 0u);
                stay[idx] = (uint8_t) r[2];
            }
    HIP_TRY(hipMemcpy(e->sl.hot, st.data(), st.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->sl.stay8, stay.data(), stay.size(), hipMemcpyHostToDevice));
    return CHUB_OK;
}

int chub_set_station_queue(chub_env *e, const int32_t *line) {
    if (!e || !line) return fail(CHUB_ERR_ARG, "null argument");
    e->walked_tick = 0;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t N = (size_t) e->hp.n_envs;
    std::vector<uint32_t> rec;
    int rc = fetch(rec, (const uint32_t *) e->st.rec, 8 * N);
    if (rc) return rc;
    for (size_t env = 0; env < N; env++)
        for (int k = 0; k < 2; k++) {
            if (line[env * 2 + k] < 0 || line[env * 2 + k] > kMaxLine) return fail(CHUB_ERR_ARG, "queue length out of range");
            uint32_t &w = rec[4 * ((size_t) k * N + env) + 3];
            w = (w & ~15u) | (uint32_t) line[env * 2 + k];
        }
    HIP_TRY(hipMemcpy(e->st.rec, rec.data(), rec.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    // the next step's station draws were decoded one launch ahead against the queue lengths just overwritten: the next launch
    // draws and decodes its own (k_draw_levels; same Philox counters)
    e->predrawn = false;
    return CHUB_OK;
}

// the temporary device buffers of one tape call: freed when the call returns, once everything that may still read them has run
namespace {
struct TapeBuffers {
    std::vector<void *> held;
    ~TapeBuffers() {
        if (held.empty()) return;
        (void) hipDeviceSynchronize();
        for (void *p : held) (void) hipFree(p);
    }
    // a device copy of `bytes` of host memory
    int put(const void *host, size_t bytes, const void **d_out) {
        void *d = nullptr;
        HIP_TRY(hipMalloc(&d, bytes));
        held.push_back(d);
        HIP_TRY(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
        *d_out = d;
        return CHUB_OK;
    }
};
}  // namespace

int chub_step_tape(chub_env *e, const float *actions, const uint64_t *pk_tape, const uint32_t *car_tape, float *obs, float *reward,
                   uint8_t *done) {
    return chub_step_tape_env(e, actions, pk_tape, car_tape, nullptr, nullptr, 0, obs, reward, done);
}

// ... the whole step from the tape: the per-env tail (k_env<.., TAPE> / the tail half of k_step_fused<.., TAPE>) takes the step's exogenous
// normals and the forecourt's arrivals from the caller as well
int chub_step_tape_env(chub_env *e, const float *actions, const uint64_t *pk_tape, const uint32_t *car_tape, const double *exo_z,
                       const uint32_t *hv_tape, int32_t hv_w, float *obs, float *reward, uint8_t *done) {
    if (!e || !actions || !pk_tape || !car_tape || !obs || !reward || !done) return fail(CHUB_ERR_ARG, "null argument");
    if (e->env_params) return refuse_params("tape mode (chub_step_tape / chub_step_tape_env)");
    if (e->hp.rng_mode != CHUB_RNG_PHILOX || !(e->hp.packed || e->hp.soc_curves))
        return fail(CHUB_ERR_ARG, "tape mode drives the packed PHILOX slot kernel: the hub shape must be one it covers");
    if ((exo_z != nullptr) != (hv_tape != nullptr) || (hv_tape && hv_w < 1)) return fail(CHUB_ERR_ARG, "the tail's tape is exo_z [N][3] AND hv_tape [N][hv_w >= 1]");
    if (e->tape_stale) return fail(CHUB_ERR_ARG, "chub_tape_clear_soc was called: reset (chub_reset_tape) before the next tape step");
    HIP_TRY(hipSetDevice(e->device));
    const size_t N = (size_t) e->hp.n_envs, S = (size_t) (e->hp.S[0] + e->hp.S[1]);
    TapeBuffers tb;
    int rc;
    const void *d_hv = nullptr, *d_z = nullptr, *d_pk = nullptr, *d_ct = nullptr, *d_act = nullptr;
    if (hv_tape) {
        // at most as many arrivals per step as the handle's forecourt can see from its own tables (the waiting list's explicit entries
        // are sized for that, chub_create), each with its SoC on the tape
        const uint32_t most = (uint32_t) ((e->hp.qcap + 1) / 2);
        for (size_t i = 0; i < N; i++)
            if (hv_tape[i * (size_t) hv_w] > most || hv_tape[i * (size_t) hv_w] > (uint32_t) (hv_w - 1))
                return fail(CHUB_ERR_ARG, "hv_tape: more FCEV arrivals in one step than the handle's forecourt (or the tape's width) takes");
        if ((rc = tb.put(hv_tape, N * (size_t) hv_w * sizeof(uint32_t), &d_hv))) return rc;
        if ((rc = upload(e->d_exo_z, exo_z, N * 3 * sizeof(double), nullptr, false, &d_z))) return rc;
    }
    // the car tape is in hub order [N][S][2] (station 0's slots first), which is the kernel's own slot order
    if ((rc = tb.put(pk_tape, 2 * N * sizeof(uint64_t), &d_pk))) return rc;
    if ((rc = tb.put(car_tape, 2 * N * S * sizeof(uint32_t), &d_ct))) return rc;
    if ((rc = upload(e->d_actions, actions, N * (size_t) e->hp.act_dim * sizeof(float), nullptr, false, &d_act))) return rc;
    StepCall c = step_call(nullptr, (const float *) d_act, (const double *) d_z, dense_out(e, e->d_obs, e->d_reward, e->d_done), 0);
    c.pk_tape = (const uint64_t *) d_pk;
    c.car_tape = (const uint32_t *) d_ct;
    c.hv_tape = (const uint32_t *) d_hv;
    c.hv_w = hv_w;
    c.tail_tape = d_hv != nullptr;
    if ((rc = run_call(e, c, nullptr))) return rc;
    return fetch_out(e, nullptr, obs, reward, done, nullptr);
}

int chub_reset_tape(chub_env *e, const uint32_t *occ_tape, const uint32_t *car_tape, float *obs) {
    return chub_reset_tape_env(e, occ_tape, car_tape, nullptr, nullptr, obs);
}

// ... the whole reset from the tape: the tail (k_env<RESET, .., TAPE>) takes renew_reset's days (REN:51-53) and make_state's normals
// (MGR:344-361) from the caller
int chub_reset_tape_env(chub_env *e, const uint32_t *occ_tape, const uint32_t *car_tape, const int32_t *exo_days, const double *exo_z, float *obs) {
    if (!e || !occ_tape || !car_tape || !obs) return fail(CHUB_ERR_ARG, "null argument");
    if (e->env_params) return refuse_params("tape mode (chub_reset_tape / chub_reset_tape_env)");
    if ((exo_days != nullptr) != (exo_z != nullptr)) return fail(CHUB_ERR_ARG, "the tail's tape of a reset is exo_days [N][2] AND exo_z [N][3]");
    int rc;
    if (exo_days && (rc = check_exo_days(e, nullptr, exo_days))) return rc;
    if (e->hp.rng_mode != CHUB_RNG_PHILOX || !(e->hp.packed || e->hp.soc_curves))
        return fail(CHUB_ERR_ARG, "tape mode drives the packed PHILOX slot kernel: the hub shape must be one it covers");
    if (e->capturing) return fail(CHUB_ERR_ARG, "tape mode cannot be captured");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t N = (size_t) e->hp.n_envs, S = (size_t) (e->hp.S[0] + e->hp.S[1]);
    TapeBuffers tb;
    const void *d_ct = nullptr, *d_days = nullptr, *d_z = nullptr;
    if ((rc = tb.put(car_tape, 2 * N * S * sizeof(uint32_t), &d_ct))) return rc;
    // the reset is the launch with argument tick + 1 - base: its slot kernel reads the units' occupancy draws from pk[that & 1],
    // where k_reset_levels would have left this build's own
    const uint32_t arg = e->tick + 1u - e->graph_base;
    HIP_TRY(hipMemcpy((void *) e->st.pk[arg & 1u], occ_tape, 2 * N * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (exo_days) {
        if ((rc = upload(e->d_exo_days, exo_days, 2 * N * sizeof(int32_t), nullptr, false, &d_days))) return rc;
        if ((rc = upload(e->d_exo_z, exo_z, 3 * N * sizeof(double), nullptr, false, &d_z))) return rc;
    }
    StepCall c = reset_call(e, nullptr, (const int32_t *) d_days, (const double *) d_z, e->d_obs);
    c.car_tape = (const uint32_t *) d_ct;
    c.tail_tape = exo_days != nullptr;
    if ((rc = run_call(e, c, nullptr))) return rc;
    e->tape_stale = false;  // evs_reset has wiped every slot
    return fetch_out(e, nullptr, obs, nullptr, nullptr, nullptr);
}

int chub_random_actions_device(chub_env *e, uint64_t key, uint32_t batch, float *d_actions, void *stream) {
    if (!e || !d_actions) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    launch_random_actions(e->hp, key, batch, d_actions, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

// ------------------------------------------------------------------------------- introspection
int chub_get_slots(chub_env *e, float *out) {
    if (!e || !out) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    const HubParams &hp = e->hp;
    const size_t N = (size_t) hp.n_envs, S = (size_t) (hp.S[0] + hp.S[1]), F = (size_t) CHUB_PILE_COUNT;
    int rc;
    if ((rc = sync_ctx(e, nullptr))) return rc;
    // every pile's nine values by the device's one decode: k_pile_obs with all fields, [N][9][S]
    std::vector<float> cols;
    float *d_cols = nullptr;
    HIP_TRY(hipMalloc((void **) &d_cols, N * F * S * sizeof(float)));
    launch_pile_obs(hp, e->d_ctx, (1u << CHUB_PILE_COUNT) - 1u, nullptr, e->d_cls_soc, d_cols, nullptr);
    rc = hipGetLastError() != hipSuccess ? fail(CHUB_ERR_HIP, "the pile decode could not be launched") : fetch(cols, (const float *) d_cols, N * F * S);
    (void) hipFree(d_cols);
    if (rc) return rc;
    // ... re-ordered into the per-station blocks: station k's piles are the hub slots from off_k on
    for (size_t env = 0; env < N; env++) {
        const float *c = cols.data() + env * F * S;
        float *o = out + env * F * S;
        for (int k = 0; k < 2; k++) {
            const size_t n = (size_t) hp.S[k], off = k ? (size_t) hp.S[0] : 0;
            for (size_t f = 0; f < F; f++, o += n) memcpy(o, c + f * S + off, n * sizeof(float));
        }
    }
    return CHUB_OK;
}

int chub_pile_obs_columns(uint32_t fields) {
    if (fields == 0u || (fields >> CHUB_PILE_COUNT) != 0u) return fail(CHUB_ERR_ARG, "fields: a non-empty mask over the CHUB_PILE_* fields");
    return __builtin_popcount(fields);
}

int chub_pile_obs_device(chub_env *e, uint32_t fields, const uint8_t *d_mask, float *d_out, void *stream) {
    if (!e || !d_out) return fail(CHUB_ERR_ARG, "null argument");
    if (chub_pile_obs_columns(fields) < 0) return CHUB_ERR_ARG;
    if (e->tape_only)
        return fail(CHUB_ERR_UNSUPPORTED, "chub_pile_obs_device is not supported on a tape handle (chub_tape_register_soc rewrites the class tables)");
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    if (const int rc = sync_ctx(e, (hipStream_t) stream)) return rc;  // (nothing to do inside a capture: chub_graph_begin has done it)
    launch_pile_obs(e->hp, e->d_ctx, fields, d_mask, e->d_cls_soc, d_out, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

// ---- pile sets (include/chub.h): which piles' action bits the next step can see, as chub_step_bits' words
static int pile_set_check(const chub_env *e, int which, const char *who) {
    if (which < 0 || which >= CHUB_PSET_COUNT)
        return fail(CHUB_ERR_ARG, std::string(who) + ": which is CHUB_PSET_ALL, CHUB_PSET_OCCUPIED or CHUB_PSET_DECIDABLE");
    if (e->tape_only)
        return fail(CHUB_ERR_UNSUPPORTED, std::string(who) + " is not supported on a tape handle (chub_tape_register_soc rewrites the class tables)");
    return CHUB_OK;
}

int chub_pile_set_device(chub_env *e, int which, const uint8_t *d_mask, uint64_t *d_bits, void *stream) {
    if (!e || !d_bits) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = pile_set_check(e, which, "chub_pile_set_device")) return rc;
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    if (const int rc = sync_ctx(e, (hipStream_t) stream)) return rc;  // (nothing to do inside a capture: chub_graph_begin has done it)
    launch_pile_set(e->hp, e->d_ctx, which, d_mask, d_bits, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_station_profile_size(uint32_t fields, int32_t buckets) {
    if (fields == 0u || (fields >> CHUB_SP_COUNT) != 0u) return fail(CHUB_ERR_ARG, "fields: a non-empty mask over the CHUB_SP_* fields");
    if (buckets < 1 || buckets > 32) return fail(CHUB_ERR_ARG, "buckets: 1 .. 32");
    return 2 * __builtin_popcount(fields) * buckets;
}

int chub_station_profile_device(chub_env *e, uint32_t fields, int32_t buckets, const uint8_t *d_mask, float *d_out, void *stream) {
    if (!e || !d_out) return fail(CHUB_ERR_ARG, "null argument");
    if (chub_station_profile_size(fields, buckets) < 0) return CHUB_ERR_ARG;
    if (e->tape_only)
        return fail(CHUB_ERR_UNSUPPORTED,
                    "chub_station_profile_device is not supported on a tape handle (chub_tape_register_soc rewrites the class tables)");
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    if (const int rc = sync_ctx(e, (hipStream_t) stream)) return rc;  // (nothing to do inside a capture: chub_graph_begin has done it)
    launch_station_profile(e->hp, e->d_ctx, fields, buckets, d_mask, e->d_cls_soc, d_out, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

// The exogenous look-ahead: what is deterministic about the next `horizon` slots of every env's day, as a read-only launch (k_forecast)
static_assert((int) CHUB_FC_COUNT == kFcCount && (int) CHUB_FC_FCEV == (int) FC_FCEV, "FcField (chub_device.h) restates the CHUB_FC_* enum");
int chub_forecast_size(uint32_t fields, int32_t horizon) {
    if (fields == 0u || (fields >> CHUB_FC_COUNT) != 0u) return fail(CHUB_ERR_ARG, "fields: a non-empty mask over the CHUB_FC_* fields");
    if (horizon < 1 || horizon > 96) return fail(CHUB_ERR_ARG, "horizon: 1 .. 96");
    return __builtin_popcount(fields) * horizon;
}

int chub_forecast_device(chub_env *e, uint32_t fields, int32_t horizon, const uint8_t *d_mask, float *d_out, void *stream) {
    if (!e || !d_out) return fail(CHUB_ERR_ARG, "null argument");
    if (chub_forecast_size(fields, horizon) < 0) return CHUB_ERR_ARG;
    if (e->tape_only) return fail(CHUB_ERR_UNSUPPORTED, "chub_forecast_device is not supported on a tape handle (its arrivals are the caller's)");
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    if (const int rc = sync_ctx(e, (hipStream_t) stream)) return rc;  // (nothing to do inside a capture: chub_graph_begin has done it)
    // lock-step: the clock by value (a capture records it: a graph replays only from the clock it started at); per-env clocks: the buffer
    // the handle's next launch reads (as copy_launch)
    const uint16_t *d_clk = e->per_env ? e->d_env_clk + (size_t) ((e->tick + 1u - e->graph_base) & 1u) * (size_t) e->hp.n_envs : nullptr;
    launch_forecast(e->hp, e->d_ctx, e->fc, fields, horizon, e->t, d_clk, d_mask, d_out, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_forecast(chub_env *e, uint32_t fields, int32_t horizon, float *out) {
    if (!e || !out) return fail(CHUB_ERR_ARG, "null argument");
    const int per_env = chub_forecast_size(fields, horizon);
    if (per_env < 0) return CHUB_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t bytes = (size_t) e->hp.n_envs * (size_t) per_env * sizeof(float);
    float *d = nullptr;
    HIP_TRY(hipMalloc((void **) &d, bytes));
    int rc = chub_forecast_device(e, fields, horizon, nullptr, d, nullptr);
    if (!rc && hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(CHUB_ERR_HIP, "the forecast could not be copied to the host");
    (void) hipFree(d);
    return rc;
}

// Step terms: what the last step's reward is made of and what a constrained learner penalises, as a read-only launch over the telemetry
// block (k_step_terms); attached (chub_set_step_terms), run_call enqueues it behind every step
static_assert((int) CHUB_ST_COUNT == 27 && (int) CHUB_ST_SOC_PENALTY == 26 && (int) CHUB_T_COUNT == kTelemCount, "k_step_terms reads CHUB_T_* columns into CHUB_ST_* fields");
int chub_get_step_terms_size(uint32_t fields) {
    if (fields == 0u || (fields >> CHUB_ST_COUNT) != 0u) return fail(CHUB_ERR_ARG, "fields: a non-empty mask over the CHUB_ST_* fields");
    return __builtin_popcount(fields);
}

// what every step-terms entry point asks of its handle and mask
static int check_step_terms(const chub_env *e, uint32_t fields, const void *out) {
    if (!e || !out) return fail(CHUB_ERR_ARG, "null argument");
    if (chub_get_step_terms_size(fields) < 0) return CHUB_ERR_ARG;
    if (!(e->hp.telemetry & 1)) return fail(CHUB_ERR_ARG, "telemetry is off: the step terms are read from its block, call chub_set_telemetry(env, 1) first");
    return CHUB_OK;
}

int chub_get_step_terms_device(chub_env *e, uint32_t fields, const uint8_t *d_mask, float *d_out, void *stream) {
    if (const int rc = check_step_terms(e, fields, d_out)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    if (const int rc = sync_ctx(e, (hipStream_t) stream)) return rc;  // (nothing to do inside a capture: chub_graph_begin has done it)
    launch_step_terms<float>(e->hp, e->d_ctx, fields, d_mask, d_out, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_get_step_terms(chub_env *e, uint32_t fields, double *out) {
    if (const int rc = check_step_terms(e, fields, out)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t bytes = (size_t) e->hp.n_envs * (size_t) __builtin_popcount(fields) * sizeof(double);
    double *d = nullptr;
    HIP_TRY(hipMalloc((void **) &d, bytes));
    int rc = sync_ctx(e, nullptr);
    if (!rc) {
        launch_step_terms<double>(e->hp, e->d_ctx, fields, nullptr, d, nullptr);
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(CHUB_ERR_HIP, "the step terms could not be launched or copied to the host");
    }
    (void) hipFree(d);
    return rc;
}

int chub_set_step_terms(chub_env *e, uint32_t fields, float *d_out) {
    if (!e) return fail(CHUB_ERR_ARG, "null handle");
    if (e->capturing)
        return fail(CHUB_ERR_UNSUPPORTED, "chub_set_step_terms between chub_graph_begin and chub_graph_end (attach or detach between captures: "
                                          "a recorded step keeps the launch it was recorded with)");
    if (fields == 0u || !d_out) {  // detach
        e->st_out = nullptr;
        e->st_fields = 0u;
        return CHUB_OK;
    }
    if (const int rc = check_step_terms(e, fields, d_out)) return rc;
    e->st_out = d_out;
    e->st_fields = fields;
    return CHUB_OK;
}

int chub_get_step_terms_attached(const chub_env *e) { return e ? (int) e->st_fields : fail(CHUB_ERR_ARG, "null handle"); }

// Station-level control: the dispatch of evs_step(float) as a read-only launch (k_load_dispatch) in front of any step form
int chub_load_dispatch_device(chub_env *e, int units, const float *d_loads, const float *d_tail, const uint8_t *d_mask, float *d_actions,
                              uint64_t *d_pile_bits, void *stream) {
    if (!e || !d_loads) return fail(CHUB_ERR_ARG, "null argument");
    if (!d_actions && !d_pile_bits) return fail(CHUB_ERR_ARG, "chub_load_dispatch: give d_actions, d_pile_bits or both");
    if (d_actions && !d_tail) return fail(CHUB_ERR_ARG, "chub_load_dispatch: action rows need d_tail (their last two entries)");
    if (units != CHUB_LOAD_KW && units != CHUB_LOAD_FRACTION) return fail(CHUB_ERR_ARG, "units: CHUB_LOAD_KW or CHUB_LOAD_FRACTION");
    if (e->tape_only)
        return fail(CHUB_ERR_UNSUPPORTED, "chub_load_dispatch is not supported on a tape handle (chub_tape_register_soc rewrites the class tables)");
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    if (const int rc = sync_ctx(e, (hipStream_t) stream)) return rc;  // (nothing to do inside a capture: chub_graph_begin has done it)
    launch_load_dispatch(e->hp, e->d_ctx, units, d_mask, e->d_cls_soc, d_loads, d_tail, d_actions, d_pile_bits, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_load_dispatch(chub_env *e, int units, const float *loads, const float *tail, float *actions, uint64_t *pile_bits) {
    if (!e || !loads) return fail(CHUB_ERR_ARG, "null argument");
    if (!actions && !pile_bits) return fail(CHUB_ERR_ARG, "chub_load_dispatch: give actions, pile_bits or both");
    if (actions && !tail) return fail(CHUB_ERR_ARG, "chub_load_dispatch: action rows need tail (their last two entries)");
    if (units != CHUB_LOAD_KW && units != CHUB_LOAD_FRACTION) return fail(CHUB_ERR_ARG, "units: CHUB_LOAD_KW or CHUB_LOAD_FRACTION");
    HIP_TRY(hipSetDevice(e->device));
    const size_t N = (size_t) e->hp.n_envs, S = (size_t) (e->hp.S[0] + e->hp.S[1]), W = (S + 63) / 64;
    const size_t b_in = 2 * N * sizeof(float), b_act = actions ? N * (S + 2) * sizeof(float) : 0, b_bits = pile_bits ? N * W * sizeof(uint64_t) : 0;
    char *d = nullptr;  // loads | tail | bits | rows, one allocation
    HIP_TRY(hipMalloc((void **) &d, 2 * b_in + b_bits + b_act));
    float *d_loads = (float *) d, *d_tail = tail ? (float *) (d + b_in) : nullptr;
    uint64_t *d_bits = pile_bits ? (uint64_t *) (d + 2 * b_in) : nullptr;
    float *d_act = actions ? (float *) (d + 2 * b_in + b_bits) : nullptr;
    int rc = CHUB_OK;
    if (hipMemcpy(d_loads, loads, b_in, hipMemcpyHostToDevice) != hipSuccess || (tail && hipMemcpy(d_tail, tail, b_in, hipMemcpyHostToDevice) != hipSuccess))
        rc = fail(CHUB_ERR_HIP, "chub_load_dispatch: the inputs could not be copied to the device");
    if (!rc) rc = chub_load_dispatch_device(e, units, d_loads, d_tail, nullptr, d_act, d_bits, nullptr);
    if (!rc && (hipDeviceSynchronize() != hipSuccess || (actions && hipMemcpy(actions, d_act, b_act, hipMemcpyDeviceToHost) != hipSuccess) ||
                (pile_bits && hipMemcpy(pile_bits, d_bits, b_bits, hipMemcpyDeviceToHost) != hipSuccess)))
        rc = fail(CHUB_ERR_HIP, "chub_load_dispatch: the launch failed or its outputs could not be copied back");
    (void) hipFree(d);
    return rc;
}

int chub_get_station_scalars(chub_env *e, double *out) {
    if (!e || !out) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t N = (size_t) e->hp.n_envs;
    std::vector<uint32_t> rec;
    std::vector<uint16_t> clk;  // station_time_hole (CHS.hpp:1204) is the env's own slot of day
    int rc;
    if ((rc = fetch(rec, (const uint32_t *) e->st.rec, 8 * N)) || (rc = fetch_clocks(e, clk))) return rc;
    for (size_t env = 0; env < N; env++)
        for (int k = 0; k < 2; k++) {
            double *o = out + (env * 2 + k) * 8;
            const uint32_t *r = &rec[4 * ((size_t) k * N + env)];
            float mn, ch, mx;
            memcpy(&mn, &r[0], 4); memcpy(&ch, &r[1], 4); memcpy(&mx, &r[2], 4);
            o[0] = mn; o[1] = ch; o[2] = mx;
            o[3] = (double) pkd_cars(r[3]);  // car_number
            o[4] = (double) pkd_line(r[3]);  // line
            o[5] = (double) pkd_flow(r[3]);  // flow_in_number[-1] (can be negative right after reset)
            o[6] = (double) (clk[env] & 127u); o[7] = e->hp.transformer_limit[k];
        }
    return CHUB_OK;
}

int chub_set_telemetry(chub_env *e, int enabled) {
    if (!e) return fail(CHUB_ERR_ARG, "null handle");
    if (!enabled && e->st_out)
        return fail(CHUB_ERR_ARG, "step terms are attached and read the telemetry block: detach first (chub_set_step_terms(env, 0, NULL))");
    HIP_TRY(hipSetDevice(e->device));
    if (enabled && !e->h_telem && !e->d_telem) {
        const size_t N = (size_t) e->hp.n_envs, D = (size_t) e->hp.obs_dim;
        const size_t count = N * (size_t) kTelemCount + N * D + N;
        double *base = nullptr;
        if (N * (size_t) e->hp.act_dim * sizeof(float) <= 16384) {
            // handles of a few envs (the bound chub_step uses for reading the caller's arrays in place: the drop-in class): one block of
            // pinned host memory, mapped into the device's address space -- the tail kernel's telemetry stores cross PCIe as posted
            // writes while it runs, and reading them back is a host read: no device read per step
            HIP_TRY(hipHostMalloc((void **) &e->h_telem, count * sizeof(double), hipHostMallocDefault));
            memset(e->h_telem, 0, count * sizeof(double));
            void *dv = nullptr;
            if (!device_view(e->h_telem, &dv)) {
                (void) hipHostFree(e->h_telem);
                e->h_telem = nullptr;
                return fail(CHUB_ERR_HIP, "pinned telemetry block is not visible to the device");
            }
            base = (double *) dv;
        } else {
            // a batch: 27 MB per step at 65 536 envs would stall the tail on posted PCIe writes -- the block stays in HBM (outside the
            // arena: a snapshot does not carry it) and the getters copy
            HIP_TRY(hipMalloc((void **) &e->d_telem, count * sizeof(double)));
            hipError_t he = hipMemset(e->d_telem, 0, count * sizeof(double));
            if (he != hipSuccess) {
                (void) hipFree(e->d_telem);
                e->d_telem = nullptr;
                return fail(CHUB_ERR_HIP, std::string("hipMemset: ") + hipGetErrorString(he));
            }
            base = e->d_telem;
        }
        e->ev.telem = base;
        e->ev.obs64 = e->ev.telem + N * (size_t) kTelemCount;
        e->ev.reward64 = e->ev.obs64 + N * D;
    }
    e->hp.telemetry = (e->hp.telemetry & ~1) | (enabled ? 1 : 0);  // (bit 1 is the episode ledger's)
    e->ctx_dirty = true;
    return CHUB_OK;
}

static int need_telemetry(chub_env *e) {
    if (!e->h_telem && !e->d_telem) return fail(CHUB_ERR_ARG, "telemetry is off: call chub_set_telemetry(env, 1) first");
    return 0;
}

int chub_telemetry_host(chub_env *e, double **telem, double **obs64, double **reward64) {
    if (!e || !telem || !obs64 || !reward64) return fail(CHUB_ERR_ARG, "null argument");
    int rc = need_telemetry(e);
    if (rc) return rc;
    if (!e->h_telem)
        return fail(CHUB_ERR_UNSUPPORTED, "the telemetry block of a handle of this size lives in device memory: read it with chub_get_telemetry / "
                                          "chub_get_obs_f64 / chub_get_reward_f64");
    const size_t N = (size_t) e->hp.n_envs, D = (size_t) e->hp.obs_dim;
    *telem = e->h_telem;
    *obs64 = e->h_telem + N * (size_t) kTelemCount;
    *reward64 = *obs64 + N * D;
    return CHUB_OK;
}

// `count` doubles of the telemetry block from `offset` on, wherever the block lives (the work in flight is waited for)
static int telem_fetch(chub_env *e, size_t offset, size_t count, double *dst) {
    int rc = need_telemetry(e);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    if (e->h_telem) memcpy(dst, e->h_telem + offset, count * sizeof(double));
    else HIP_TRY(hipMemcpy(dst, e->d_telem + offset, count * sizeof(double), hipMemcpyDeviceToHost));
    return CHUB_OK;
}

int chub_get_telemetry(chub_env *e, double *out) {
    if (!e || !out) return fail(CHUB_ERR_ARG, "null argument");
    const size_t N = (size_t) e->hp.n_envs;
    std::vector<double> t(N * (size_t) kTelemCount);
    int rc = telem_fetch(e, 0, t.size(), t.data());
    if (rc) return rc;
    for (size_t env = 0; env < N; env++)
        for (int i = 0; i < kTelemCount; i++) out[env * kTelemCount + i] = t[(size_t) i * N + env];
    return CHUB_OK;
}

int chub_get_obs_f64(chub_env *e, double *out) {
    if (!e || !out) return fail(CHUB_ERR_ARG, "null argument");
    const size_t N = (size_t) e->hp.n_envs;
    return telem_fetch(e, N * (size_t) kTelemCount, N * (size_t) e->hp.obs_dim, out);
}

int chub_get_reward_f64(chub_env *e, double *out) {
    if (!e || !out) return fail(CHUB_ERR_ARG, "null argument");
    const size_t N = (size_t) e->hp.n_envs;
    return telem_fetch(e, N * (size_t) kTelemCount + N * (size_t) e->hp.obs_dim, N, out);
}

// ---- the per-episode ledger (include/chub.h: chub_set_episode_stats) ---------------------------------------------------------------------
static size_t ledger_bytes(const chub_env *e) {
    return (size_t) e->hp.n_envs * (2 * (size_t) kEpCount * sizeof(double) + sizeof(uint32_t) + sizeof(uint8_t));
}
int chub_set_episode_stats(chub_env *e, int enabled) {
    if (!e) return fail(CHUB_ERR_ARG, "null handle");
    if (e->tape_only) return fail(CHUB_ERR_UNSUPPORTED, "chub_set_episode_stats is not supported on a tape handle (chub_tape_register_soc)");
    if (e->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_set_episode_stats between chub_graph_begin and chub_graph_end (call it between replays)");
    HIP_TRY(hipSetDevice(e->device));
    if (enabled && !e->es.on) {
        const size_t N = (size_t) e->hp.n_envs;
        if (!e->d_ep_sum) HIP_TRY(hipMalloc((void **) &e->d_ep_sum, ((size_t) kEpSumMaxBlocks + 1) * kEpSumWords * sizeof(double)));
        if (!e->d_ledger) HIP_TRY(hipMalloc((void **) &e->d_ledger, ledger_bytes(e)));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemset(e->d_ledger, 0, ledger_bytes(e)));  // counting starts with the next call
        e->es.live = (double *) e->d_ledger;
        e->es.fin = e->es.live + (size_t) kEpCount * N;
        e->es.episodes = (uint32_t *) (e->es.fin + (size_t) kEpCount * N);
        e->es.pending = (uint8_t *) (e->es.episodes + N);
    }
    e->es.on = enabled ? 1 : 0;
    e->hp.telemetry = (e->hp.telemetry & ~2) | (enabled ? 2 : 0);  // what the tail reads: one word for both flags
    e->ctx_dirty = true;
    return CHUB_OK;
}

int chub_has_episode_stats(const chub_env *e) { return e ? e->es.on : CHUB_ERR_ARG; }

static int need_ledger(const chub_env *e) {
    if (!e->es.on) return fail(CHUB_ERR_ARG, "the episode ledger is off: call chub_set_episode_stats(env, 1) first");
    return 0;
}

int chub_get_episode_stats(chub_env *e, int finished, double *out) {
    if (!e || !out) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = need_ledger(e)) return rc;
    const size_t N = (size_t) e->hp.n_envs;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<double> t;
    if (const int rc = fetch(t, (const double *) (finished ? e->es.fin : e->es.live), (size_t) kEpCount * N)) return rc;
    for (size_t env = 0; env < N; env++)
        for (int c = 0; c < kEpCount; c++) out[env * kEpCount + c] = t[(size_t) c * N + env];
    return CHUB_OK;
}

int chub_get_episode_counts(chub_env *e, uint32_t *out) {
    if (!e || !out) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = need_ledger(e)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, e->es.episodes, (size_t) e->hp.n_envs * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CHUB_OK;
}

int chub_episode_stats_device(chub_env *e, int finished, double *d_out, uint32_t *d_counts, void *stream) {
    if (!e || !d_out) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = need_ledger(e)) return rc;
    const size_t N = (size_t) e->hp.n_envs;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpyAsync(d_out, finished ? e->es.fin : e->es.live, (size_t) kEpCount * N * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t) stream));
    if (d_counts) HIP_TRY(hipMemcpyAsync(d_counts, e->es.episodes, N * sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t) stream));
    return CHUB_OK;
}

int chub_episode_summary_device(chub_env *e, double *d_out, int drain, void *stream) {
    if (!e || !d_out) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = need_ledger(e)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    if (const int rc = sync_ctx(e, (hipStream_t) stream)) return rc;
    launch_episode_summary(e->hp, e->d_ctx, e->d_ep_sum, d_out, drain, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_episode_summary(chub_env *e, double *out, int drain) {
    if (!e || !out) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = need_ledger(e)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());  // (steps in flight on any stream write the ledger)
    double *d_res = e->d_ep_sum + (size_t) kEpSumMaxBlocks * kEpSumWords;
    if (const int rc = chub_episode_summary_device(e, d_res, drain, nullptr)) return rc;
    HIP_TRY(hipMemcpy(out, d_res, kEpSumWords * sizeof(double), hipMemcpyDeviceToHost));
    return CHUB_OK;
}

int chub_set_rng_compat_seeds(chub_env *e, const uint32_t *seeds) {
    if (!e || !seeds) return fail(CHUB_ERR_ARG, "null argument");
    e->walked_tick = 0;  // (a walk that ran ahead drew from the streams as they were)
    if (e->hp.rng_mode != CHUB_RNG_COMPAT) return fail(CHUB_ERR_ARG, "handle is not in COMPAT mode");
    HIP_TRY(hipSetDevice(e->device));
    const size_t N = (size_t) e->hp.n_envs;
    std::vector<uint32_t> g(N * 32), m(N);
    for (size_t i = 0; i < N; i++) {
        // glibc srandom_r, TYPE_3: LCG fill of 31 words, front = 3, rear = 0, 310 warm-up draws
        uint32_t *r = &g[i * 32];
        uint32_t sd = seeds[2 * i] ? seeds[2 * i] : 1u;
        int32_t word = (int32_t) sd;
        r[0] = (uint32_t) word;
        for (int j = 1; j < 31; j++) {
            long hi = word / 127773, lo = word % 127773;
            word = (int32_t) (16807 * lo - 2836 * hi);
            if (word < 0) word += 2147483647;
            r[j] = (uint32_t) word;
        }
        uint32_t f = 3, b = 0;
        for (int j = 0; j < 310; j++) {
            r[f] += r[b];
            f = (f + 1 == 31) ? 0 : f + 1;
            b = (b + 1 == 31) ? 0 : b + 1;
        }
        r[31] = f;
        uint32_t x = seeds[2 * i + 1] % 2147483647u;  // minstd_rand0::seed
        m[i] = x ? x : 1u;
    }
    HIP_TRY(hipMemcpy(e->cr.g3[e->rng_cur], g.data(), g.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->cr.minstd3[e->rng_cur], m.data(), m.size() * 4, hipMemcpyHostToDevice));
    return CHUB_OK;
}

int chub_set_rng_compat_state(chub_env *e, const uint32_t *state) {
    if (!e || !state) return fail(CHUB_ERR_ARG, "null argument");
    e->walked_tick = 0;  // (a walk that ran ahead of its step is void)
    if (e->hp.rng_mode != CHUB_RNG_COMPAT) return fail(CHUB_ERR_ARG, "handle is not in COMPAT mode");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t N = (size_t) e->hp.n_envs;
    std::vector<uint32_t> g(N * 32), m(N);
    for (size_t i = 0; i < N; i++) {
        if (state[i * 33 + 31] >= 31u) return fail(CHUB_ERR_ARG, "front index must be < 31");
        memcpy(&g[i * 32], &state[i * 33], 32 * 4);
        m[i] = state[i * 33 + 32];
    }
    HIP_TRY(hipMemcpy(e->cr.g3[e->rng_cur], g.data(), g.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->cr.minstd3[e->rng_cur], m.data(), m.size() * 4, hipMemcpyHostToDevice));
    return CHUB_OK;
}

int chub_get_rng_compat_state(chub_env *e, uint32_t *state) {
    if (!e || !state) return fail(CHUB_ERR_ARG, "null argument");
    if (e->hp.rng_mode != CHUB_RNG_COMPAT) return fail(CHUB_ERR_ARG, "handle is not in COMPAT mode");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t N = (size_t) e->hp.n_envs;
    std::vector<uint32_t> g, m;
    int rc;
    if ((rc = fetch(g, (const uint32_t *) e->cr.g3[e->rng_cur], N * 32)) || (rc = fetch(m, (const uint32_t *) e->cr.minstd3[e->rng_cur], N))) return rc;
    for (size_t i = 0; i < N; i++) {
        memcpy(&state[i * 33], &g[i * 32], 32 * 4);
        state[i * 33 + 32] = m[i];
    }
    return CHUB_OK;
}

int chub_profile_begin(chub_env *e, int max_steps, int every) {
    if (!e || max_steps <= 0 || every <= 0) return fail(CHUB_ERR_ARG, "bad argument");
    e->prof_every = every;
    e->prof_phase = 0;
    HIP_TRY(hipSetDevice(e->device));
    while (e->prof_events.size() < (size_t) max_steps * 4) {
        hipEvent_t ev;
        HIP_TRY(hipEventCreate(&ev));
        e->prof_events.push_back(ev);
    }
    e->prof_cap = (size_t) max_steps;
    e->prof_used = 0;
    e->prof_on = true;
    return CHUB_OK;
}

int chub_profile_end(chub_env *e, double *slot_ms_sum, double *env_ms_sum, int *n_steps) {
    if (!e || !slot_ms_sum || !env_ms_sum || !n_steps) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    double a = 0, b = 0;
    for (size_t i = 0; i < e->prof_used; i++) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, e->prof_events[4 * i], e->prof_events[4 * i + 1]));
        a += ms;
        HIP_TRY(hipEventElapsedTime(&ms, e->prof_events[4 * i + 2], e->prof_events[4 * i + 3]));
        b += ms;
    }
    *slot_ms_sum = a;
    *env_ms_sum = b;
    *n_steps = (int) e->prof_used;
    e->prof_on = false;
    return CHUB_OK;
}

int chub_compat_replay_constructor(chub_env *e) {
    if (!e) return fail(CHUB_ERR_ARG, "null handle");
    e->walked_tick = 0;  // (a walk that ran ahead of its step is void)
    if (e->hp.rng_mode != CHUB_RNG_COMPAT) return fail(CHUB_ERR_ARG, "handle is not in COMPAT mode");
    HIP_TRY(hipSetDevice(e->device));
    int rc = sync_ctx(e, nullptr);
    if (rc) return rc;
    // (1) the two station constructors each run evs_reset (CHS.hpp:1152, 1462; AGG:188-196)
    StepArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.station_filter = -1;
    sa.env_hi = (int32_t) (e->hp.n_envs - 1);
    sa.commit_rng = e->hp.compat_split;  // (the split form's walk leaves the streams' state in the shadow buffer: the commit moves rng_cur on)
    sa.rng_cur = e->rng_cur;
    CallState c = {};
    c.reset = c.all_served = true;
    const CallPlan cp = {CALL_SLOT_ENV, ONE_NONE, slot_form(e->plan, c), LEVELS_NONE, ENV_COMPAT};
    launch_slot<true>(cp, e->hp, e->plan, e->d_ctx, sa, nullptr, packed_ptrs(e), nullptr, nullptr);
    if (sa.commit_rng) e->rng_cur = (e->rng_cur + 1) % 3;
    e->empt_valid = e->hp.compat_split != 0;
    e->e2_tick = ~0u;  // (no pass has left empt2 for a walk two steps ahead: the first step counts for itself)
    // (2) HySystem.__init__: 101 hy_step()s with live FCEV arrivals (HYD:154-157,168,250-259) -> the streams advance and
    //     every env gets the hy_power_speed_list the reference would have built from its draws
    launch_compat_ctor_sweep(e->hp, e->d_ctx, e->rng_cur, nullptr, e->env_params);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return CHUB_OK;
}

// ---- snapshot / restore (the reference cannot be pickled or deep-copied, MAIN:234) -----------
// Blob = header + the device arena (all state arrays; the tables in it are constant and simply ride along).
struct SnapshotHeader {
    uint64_t magic;
    int64_t n_envs, env_id0;
    chub_config cfg;
    int32_t rng_mode, t, price_count;
    uint32_t tick, graph_base;
    uint64_t arena_used;
    double hy_table[102];
    // per-env clocks (the clocks themselves are in the arena); the blob ends with every env's last tick
    int32_t predrawn, per_env;
    int32_t rng_cur;  // COMPAT: which of the arena's three stream buffers holds the committed streams
    int32_t pad_;     // bit 0: taken from a handle with per-env hub parameters, bit 1: with the episode ledger on -- its block then ends the blob
                      // (0 otherwise: the blob of a homogeneous handle without the ledger is unchanged); bits 8 .. 15, with bit 0: the rows'
                      // FCEV arrivals per step at most (hv_max_arrive <= 127), which sizes q_time / q_mass / hv_pre inside the arena -- two
                      // capacities can round to one arena_used (every array is padded to 256 bytes), so the size alone does not tell them apart
    uint32_t key[2];  // the source's Philox key (its seed): not state -- the target keeps its own -- but the draws made ahead carry it
};
static const char *const kSnapshotInCapture = "chub_get_state / chub_set_state between chub_graph_begin and chub_graph_end (a snapshot synchronises and "
                                              "copies: call it between replays)";
static const uint64_t kSnapMagic = 0x43485542534e4150ull;  // "CHUBSNAP"

int64_t chub_state_size(const chub_env *e) {
    if (!e) return fail(CHUB_ERR_ARG, "null handle");
    if (!e->arena) return fail(CHUB_ERR_UNSUPPORTED, "snapshot needs the single-arena allocation (CHUB_NO_ARENA is set)");
    return (int64_t) (sizeof(SnapshotHeader) + e->arena_used + (size_t) e->hp.n_envs * sizeof(uint32_t) + (e->es.on ? ledger_bytes(e) : 0));
}

int chub_get_state(chub_env *e, void *buf, int64_t size) {
    if (!e || !buf) return fail(CHUB_ERR_ARG, "null argument");
    if (e->capturing) return fail(CHUB_ERR_UNSUPPORTED, kSnapshotInCapture);
    const int64_t need = chub_state_size(e);
    if (need < 0) return (int) need;
    if (size < need) return fail(CHUB_ERR_ARG, "buffer too small for the snapshot");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    SnapshotHeader h;
    memset(&h, 0, sizeof h);
    h.magic = kSnapMagic;
    h.n_envs = e->hp.n_envs;
    h.env_id0 = e->hp.env_id0;
    h.cfg = e->cfg;
    h.rng_mode = e->public_mode;
    h.t = e->t;
    h.price_count = e->price_count;
    h.tick = e->tick;
    h.graph_base = e->graph_base;
    h.arena_used = e->arena_used;
    memcpy(h.hy_table, e->hy_table, sizeof h.hy_table);
    h.predrawn = e->predrawn ? 1 : 0;
    h.per_env = e->per_env ? 1 : 0;
    h.rng_cur = e->rng_cur;
    h.key[0] = e->hp.key[0];
    h.key[1] = e->hp.key[1];
    h.pad_ = (e->env_params ? 1 | (e->hv_max_arrive << 8) : 0) | (e->es.on ? 2 : 0);  // (the rows themselves are in the arena)
    memcpy(buf, &h, sizeof h);
    HIP_TRY(hipMemcpy((char *) buf + sizeof h, e->arena, e->arena_used, hipMemcpyDeviceToHost));
    {
        const size_t N = (size_t) e->hp.n_envs;
        std::vector<int32_t> t(N);
        std::vector<uint32_t> tk(N);
        int rc = chub_env_clocks(e, t.data(), tk.data());
        if (rc) return rc;
        memcpy((char *) buf + sizeof h + e->arena_used, tk.data(), N * sizeof(uint32_t));
        if (e->es.on)
            HIP_TRY(hipMemcpy((char *) buf + sizeof h + e->arena_used + N * sizeof(uint32_t), e->d_ledger, ledger_bytes(e), hipMemcpyDeviceToHost));
    }
    return CHUB_OK;
}

int chub_set_state(chub_env *e, const void *buf, int64_t size) {
    if (!e || !buf) return fail(CHUB_ERR_ARG, "null argument");
    if (e->capturing) return fail(CHUB_ERR_UNSUPPORTED, kSnapshotInCapture);
    const int64_t need = chub_state_size(e);
    if (need < 0) return (int) need;
    SnapshotHeader h;
    if (size < (int64_t) sizeof h) return fail(CHUB_ERR_ARG, "snapshot truncated");
    memcpy(&h, buf, sizeof h);
    if (h.magic != kSnapMagic) return fail(CHUB_ERR_ARG, "not a chub snapshot");
    if (((h.pad_ & 1) != 0) != e->env_params)
        return fail(CHUB_ERR_ARG, e->env_params ? "snapshot was taken from a handle without per-env hub parameters"
                                                : "snapshot was taken from a handle with per-env hub parameters (chub_create_params)");
    if (((h.pad_ & 2) != 0) != (e->es.on != 0))
        return fail(CHUB_ERR_ARG, e->es.on ? "snapshot was taken from a handle without the episode ledger (chub_set_episode_stats)"
                                           : "snapshot was taken from a handle with the episode ledger on (chub_set_episode_stats)");
    if (h.n_envs != e->hp.n_envs || h.env_id0 != e->hp.env_id0 || h.rng_mode != e->public_mode ||
        memcmp(&h.cfg, &e->cfg, sizeof h.cfg) != 0 || h.arena_used != e->arena_used || size < need)
        return fail(CHUB_ERR_ARG, "snapshot was taken from a handle with a different configuration");
    if (e->env_params && ((h.pad_ >> 8) & 0xff) != e->hv_max_arrive)
        return fail(CHUB_ERR_ARG, "snapshot was taken from a handle whose FCEV waiting list was sized for " + std::to_string((h.pad_ >> 8) & 0xff) +
                                      " arrivals per step, this handle's for " + std::to_string(e->hv_max_arrive) + " (the largest fcev_permeate at create)");
    if (h.rng_cur < 0 || h.rng_cur > 2) return fail(CHUB_ERR_ARG, "snapshot header is corrupt");  // (every header check comes before the first write)
    e->walked_tick = 0;  // (a walk that ran ahead of its step is void)
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    // device pointers inside the arena are position-dependent: restore only into the handle's own layout, which the
    // checks above guarantee is the same; the DevCtx block (pointers, flags) is rewritten from the host copy
    HIP_TRY(hipMemcpy(e->arena, (const char *) buf + sizeof h, e->arena_used, hipMemcpyHostToDevice));
    e->empt_valid = false;  // (the restored slot state has not been counted)
    e->e2_tick = ~0u;       // (... nor has any pass left empt2 for a walk two steps ahead)
    e->rng_cur = h.rng_cur;
    e->t = h.t;
    e->price_count = h.price_count;
    e->tick = h.tick;
    e->graph_base = h.graph_base;
    memcpy(e->hy_table, h.hy_table, sizeof h.hy_table);
    e->ctx_dirty = true;
    {
        const size_t N = (size_t) e->hp.n_envs;
        // (the draws made ahead are a function of key, tick, env id and the queues this blob restores: good in a handle of any launch form,
        // void under another key)
        e->predrawn = h.predrawn != 0 && h.key[0] == e->hp.key[0] && h.key[1] == e->hp.key[1];
        e->per_env = h.per_env != 0;
        e->h_tick.resize(N);
        memcpy(e->h_tick.data(), (const char *) buf + sizeof h + e->arena_used, N * sizeof(uint32_t));
        if (e->es.on)
            HIP_TRY(hipMemcpy(e->d_ledger, (const char *) buf + sizeof h + e->arena_used + N * sizeof(uint32_t), ledger_bytes(e), hipMemcpyHostToDevice));
        e->full_tick = 0;  // per env, from the blob
    }
    return CHUB_OK;
}

int chub_fcev_stuck_count(chub_env *e, int64_t *out) {
    if (!e || !out) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint8_t> f;
    int rc = fetch(f, (const uint8_t *) e->ev.hv_line, (size_t) e->hp.n_envs);
    if (rc) return rc;
    int64_t n = 0;
    for (uint8_t b : f) n += (b & 128u) ? 1 : 0;
    *out = n;
    return CHUB_OK;
}

int chub_set_ou_state(chub_env *e, const double *ou) {
    if (!e || !ou) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    const size_t N = (size_t) e->hp.n_envs;
    std::vector<double> t(3 * N);
    for (size_t i = 0; i < N; i++)
        for (int c = 0; c < 3; c++) t[(size_t) c * N + i] = ou[i * 3 + c];
    HIP_TRY(hipMemcpy(e->ev.ou, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    return CHUB_OK;
}

int chub_get_hy_table(const chub_env *e, double *out102) {
    if (!e || !out102) return fail(CHUB_ERR_ARG, "null argument");
    if (e->env_params) return refuse_params("chub_get_hy_table (one table for every env; chub_get_hy_table_env gives env i's)");
    memcpy(out102, e->hy_table, sizeof e->hy_table);
    return CHUB_OK;
}

int chub_get_hy_table_env(chub_env *e, int64_t env_index, double *out102) {
    if (!e || !out102) return fail(CHUB_ERR_ARG, "null argument");
    if (env_index < 0 || env_index >= e->hp.n_envs) return fail(CHUB_ERR_ARG, "env index out of range");
    if (!e->ev.hy_env) return chub_get_hy_table(e, out102);  // PHILOX: one table for the whole handle
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out102, (const double *) e->ev.hy_env + (size_t) env_index * 102, 102 * sizeof(double), hipMemcpyDeviceToHost));
    return CHUB_OK;
}

int chub_set_hy_table(chub_env *e, const double *in102) {
    if (!e || !in102) return fail(CHUB_ERR_ARG, "null argument");
    if (e->env_params) return refuse_params("chub_set_hy_table (one table for every env)");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    memcpy(e->hy_table, in102, sizeof e->hy_table);
    HIP_TRY(hipMemcpy((void *) e->tb.hy_table, in102, sizeof e->hy_table, hipMemcpyHostToDevice));
    if (e->ev.hy_env) {
        const size_t N = (size_t) e->hp.n_envs;
        std::vector<double> rep(N * 102);
        for (size_t i = 0; i < N; i++) memcpy(&rep[i * 102], in102, sizeof e->hy_table);
        HIP_TRY(hipMemcpy(e->ev.hy_env, rep.data(), rep.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    return CHUB_OK;
}

// ---- per-env hub parameters (include/chub.h) ----------------------------------------------------------------------------------
// Rows -> DevCtx::ep (the derived constants, field-major, and the FCEV rate), EnvArrays::hy_env (each env's zero-demand electrolyser table,
// built on the host by build_hy_table: glibc's pow(temp, 2) is not always temp * temp, so a device copy of the sweep would not be the
// homogeneous handle's table) and the raw rows.  Only the envs the mask names are written; a table is built once per distinct tank /
// electrolyser setting among them.
static int write_env_params(chub_env *e, const uint8_t *mask, const chub_env_params *rows) {
    const size_t N = (size_t) e->hp.n_envs;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());  // (launches in flight read these arrays)
    std::vector<double> prm((size_t) PRM_COUNT * N), hy(N * 102);
    std::vector<float> rate(N);
    std::vector<chub_env_params> raw(N);
    if (mask) {  // the envs the mask does not name keep what they have
        int rc;
        if ((rc = fetch(prm, (const double *) e->ep.prm, prm.size())) || (rc = fetch(rate, (const float *) e->ep.hv_rate, N)) ||
            (rc = fetch(hy, (const double *) e->ev.hy_env, hy.size())) || (rc = fetch(raw, (const chub_env_params *) e->d_rows, N)))
            return rc;
    }
    std::map<std::string, size_t> built;  // (init_soc, hydro_store_vlt, hydro_prod_rate, hydro_loss) -> an env whose table holds that sweep
    HubParams hq = e->hp;
    for (size_t i = 0; i < N; i++) {
        if (mask && !mask[i]) continue;
        const chub_env_params &r = rows[i];
        raw[i] = r;
        const EnvConsts k = derive_env_consts(r);
        const double v[PRM_COUNT] = {k.v_h_max, k.cells, k.rc_cells, k.cap_mass, k.rc_cap_mass, k.init_soc, k.hydro_loss, k.fc_max_power,
                                     k.renew_fluct1, k.price_fluct1};
        for (int f = 0; f < PRM_COUNT; f++) prm[(size_t) f * N + i] = v[f];
        rate[i] = k.hv_rate;
        const double key[4] = {r.init_soc, r.hydro_store_vlt, r.hydro_prod_rate, r.hydro_loss};
        const std::string ks((const char *) key, sizeof key);
        const auto it = built.find(ks);
        if (it != built.end()) {
            memcpy(&hy[i * 102], &hy[it->second * 102], 102 * sizeof(double));
        } else {
            hq.init_soc = k.init_soc; hq.cap_mass = k.cap_mass; hq.v_h_max = k.v_h_max; hq.cells = k.cells; hq.hydro_loss = k.hydro_loss;
            build_hy_table(hq, &hy[i * 102]);
            built.emplace(ks, i);
        }
    }
    HIP_TRY(hipMemcpy((void *) e->ep.prm, prm.data(), prm.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((void *) e->ep.hv_rate, rate.data(), N * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->ev.hy_env, hy.data(), hy.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_rows, raw.data(), N * sizeof(chub_env_params), hipMemcpyHostToDevice));
    // the next step's FCEV counts were drawn one launch ahead with the old rates: the next launch draws its own
    e->predrawn = false;
    return CHUB_OK;
}

int chub_set_env_params(chub_env *e, const uint8_t *mask, const chub_env_params *rows) {
    if (!e || !rows) return fail(CHUB_ERR_ARG, "null argument");
    if (!e->env_params) return fail(CHUB_ERR_ARG, "the handle has no per-env hub parameters: create it with chub_create_params");
    if (e->capturing) return fail(CHUB_ERR_ARG, "chub_set_env_params inside a capture (call it between replays)");
    for (int64_t i = 0; i < e->hp.n_envs; i++) {
        if (mask && !mask[i]) continue;
        const chub_env_params &r = rows[i];
        const std::string where = " (env " + std::to_string(i) + ")";
        if (const int rc = check_scalars(r.init_soc, r.hydro_prod_rate, r.hydro_store_vlt, r.fc_max_power, where)) return rc;
        const int m = hv_bound(e->hv_top, derive_env_consts(r).hv_rate);
        if (m > 127) return fail(CHUB_ERR_UNSUPPORTED, "more than 127 FCEV arrivals per step" + where);
        if (m > e->hv_max_arrive)
            return fail(CHUB_ERR_ARG, "fcev_permeate gives up to " + std::to_string(m) + " FCEV arrivals per step, more than the " +
                                      std::to_string(e->hv_max_arrive) + " the handle's waiting list was sized for at create" + where);
    }
    return write_env_params(e, mask, rows);
}

int chub_get_env_params(chub_env *e, chub_env_params *rows) {
    if (!e || !rows) return fail(CHUB_ERR_ARG, "null argument");
    if (!e->env_params) return fail(CHUB_ERR_ARG, "the handle has no per-env hub parameters: create it with chub_create_params");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(rows, e->d_rows, (size_t) e->hp.n_envs * sizeof(chub_env_params), hipMemcpyDeviceToHost));
    return CHUB_OK;
}

int chub_has_env_params(const chub_env *e) { return e ? (e->env_params ? 1 : 0) : CHUB_ERR_ARG; }

// ---- an actor on the device (include/chub.h): an MLP from the feature row to the action row / pile bits, and the closed loop issued from C.
// The kernel and the device weight layout are chub_policy.hip / chub_policy.h; here: validation, ownership, and the calls' order.
static_assert((int) CHUB_PIN_COUNT == PIN_COUNT && (int) CHUB_PIN_FORECAST == PIN_FORECAST && (int) CHUB_PACT_COUNT == PACT_COUNT &&
                  (int) CHUB_PACT_RELU == PACT_RELU && (int) CHUB_PHEAD_COUNT == PHEAD_COUNT && (int) CHUB_PHEAD_LOADS == PHEAD_LOADS &&
                  (int) CHUB_PSQ_COUNT == PSQ_COUNT && (int) CHUB_PSQ_CLIP == PSQ_CLIP && (int) CHUB_PRUN_COUNT == PRUN_COUNT &&
                  (int) CHUB_PRUN_AUTORESET == PRUN_AUTORESET,
              "chub_policy.h restates the CHUB_PIN_* / PACT / PHEAD / PSQ / PRUN enums");
}  // extern "C"

// ---- device memory that an object owns: allocate zeroed and remember, free all
struct DeviceAllocs {
    std::vector<void *> ptrs;
    // *p = count zeroed elements (at least 4 bytes).  Returns nullptr, or what failed, for the owner's own error text
    template <class T>
    const char *zeroed(T **p, size_t count) {
        size_t bytes = count * sizeof(T);
        void *d = nullptr;
        if (!bytes) bytes = 4;
        if (hipMalloc(&d, bytes) != hipSuccess) return "out of device memory";
        ptrs.push_back(d);
        if (hipMemset(d, 0, bytes) != hipSuccess) return "hipMemset failed";
        *p = (T *) d;
        return nullptr;
    }
    void free_all() {
        for (void *p : ptrs) (void) hipFree(p);
        ptrs.clear();
    }
};

// ---- one net's layers in the kernels' layout (chub_policy.h): what an actor and a critic both are on the host, and what a population, a
// gradient call and an optimiser read of their target.  The entry points of chub_policy_* and chub_critic_* that write, read or normalise
// weights are their own refusals and one net_* call with the caller's name.
struct MlpNet {
    chub_env *env;
    const char *noun, *row_noun, *alloc_who;  // the error texts' "policy" / "critic", "feature row" / "rows", "chub_policy" / "chub_critic_create"
    int32_t n_layers, F;
    int32_t out[kPolicyMaxLayers], in[kPolicyMaxLayers], k_pad[kPolicyMaxLayers];
    int32_t tiles[kPolicyMaxLayers];        // output tiles of 32 a layer's buffers hold: the owner's rule
    float *d_w[kPolicyMaxLayers], *d_b[kPolicyMaxLayers];  // the layers in the kernel's layout (never move)
    float *d_norm;                          // mean [F] | inv_std [F]
    float *d_stage;                         // the host form of set_weights: W | b of the largest layer, in the trainer's layout
    bool normalize;
    DeviceAllocs allocs;
    std::vector<chub_adam *> adams;         // made for this net (chub_adam_create_policy / _critic): destroyed before it
};

static void adam_free(chub_adam *a);

template <class T>
static int net_alloc(MlpNet &n, T **p, size_t count) {
    if (const char *what = n.allocs.zeroed(p, count)) return fail(CHUB_ERR_HIP, std::string(n.alloc_who) + ": " + what);
    return CHUB_OK;
}

// the layers, the staging buffer and the normaliser, zeroed, for the out / in / tiles that stand in the net
static int net_alloc_layers(MlpNet &n) {
    size_t stage = 0;
    for (int l = 0; l < n.n_layers; l++) {
        n.k_pad[l] = (n.in[l] + 1) & ~1;
        stage = std::max(stage, (size_t) n.out[l] * (size_t) n.in[l] + (size_t) n.out[l]);
        if (const int rc = net_alloc(n, &n.d_w[l], (size_t) n.tiles[l] * (size_t) n.k_pad[l] * kPolicyOutTile)) return rc;
        if (const int rc = net_alloc(n, &n.d_b[l], (size_t) n.tiles[l] * kPolicyOutTile)) return rc;
    }
    if (const int rc = net_alloc(n, &n.d_stage, stage)) return rc;
    return net_alloc(n, &n.d_norm, 2 * (size_t) n.F);
}

// the optimisers first; then nothing in flight may still read what goes
static void net_free(MlpNet &n) {
    while (!n.adams.empty()) adam_free(n.adams.back());
    (void) hipSetDevice(n.env->device);
    (void) hipDeviceSynchronize();
    n.allocs.free_all();
}

// what a call that enqueues starts with; and what a host form (it copies and synchronises) starts with
static int net_begin(const MlpNet &n) {
    HIP_TRY(hipSetDevice(n.env->device));
    (void) hipGetLastError();
    return CHUB_OK;
}

static int net_begin_host(const MlpNet &n, const char *who) {
    if (n.env->capturing)
        return fail(CHUB_ERR_UNSUPPORTED, std::string(who) + " between chub_graph_begin and chub_graph_end (it copies and synchronises: use " + who +
                                              "_device)");
    return net_begin(n);
}

static int net_check_layer(const MlpNet &n, int32_t layer) {
    if (layer < 0 || layer >= n.n_layers) return fail(CHUB_ERR_ARG, "layer: 0 .. n_layers - 1");
    return CHUB_OK;
}

// W [out][in], b [out] in device memory -> layer l's blocks at d_w / d_b (the net's own, or a population member's); and back
static void net_relayout(const MlpNet &n, int l, const float *d_W, const float *d_b, float *d_w, float *d_bias, void *stream) {
    launch_policy_relayout(d_W, d_b, d_w, d_bias, n.out[l], n.in[l], n.k_pad[l], n.tiles[l], (hipStream_t) stream);
}

static void net_unlayout(const MlpNet &n, int l, const float *d_w, const float *d_bias, float *d_W, float *d_b, void *stream) {
    launch_policy_unlayout(d_w, d_bias, d_W, d_b, n.out[l], n.in[l], n.k_pad[l], (hipStream_t) stream);
}

// the staging buffer holds layer l as W | b: where b stands
static float *net_stage_b(const MlpNet &n, int l) { return n.d_stage + (size_t) n.out[l] * (size_t) n.in[l]; }

// host W | b of layer l into the staging buffer, and out of it
static int net_stage_in(MlpNet &n, int l, const float *W, const float *b) {
    const size_t nw = (size_t) n.out[l] * (size_t) n.in[l], nb = (size_t) n.out[l];
    HIP_TRY(hipDeviceSynchronize());  // (the staging buffer is one; nothing may still be reading the layer either)
    HIP_TRY(hipMemcpy(n.d_stage, W, nw * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(n.d_stage + nw, b, nb * sizeof(float), hipMemcpyHostToDevice));
    return CHUB_OK;
}

static int net_stage_out(MlpNet &n, int l, float *W, float *b) {
    const size_t nw = (size_t) n.out[l] * (size_t) n.in[l], nb = (size_t) n.out[l];
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(W, n.d_stage, nw * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(b, n.d_stage + nw, nb * sizeof(float), hipMemcpyDeviceToHost));
    return CHUB_OK;
}

static int net_upload(MlpNet &n, int l, const float *W, const float *b) {
    if (const int rc = net_stage_in(n, l, W, b)) return rc;
    net_relayout(n, l, n.d_stage, net_stage_b(n, l), n.d_w[l], n.d_b[l], nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return CHUB_OK;
}

static int net_set_weights(MlpNet &n, const char *who, int32_t layer, const float *W, const float *b) {
    if (const int rc = net_check_layer(n, layer)) return rc;
    if (const int rc = net_begin_host(n, who)) return rc;
    return net_upload(n, layer, W, b);
}

static int net_set_weights_device(MlpNet &n, int32_t layer, const float *d_W, const float *d_b, void *stream) {
    if (const int rc = net_check_layer(n, layer)) return rc;
    if (const int rc = net_begin(n)) return rc;
    net_relayout(n, layer, d_W, d_b, n.d_w[layer], n.d_b[layer], stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

// reading weights back: the kernels' layout -> the trainer's, the way a population's members go
static int net_get_weights_device(MlpNet &n, int32_t layer, float *d_W, float *d_b, void *stream) {
    if (const int rc = net_check_layer(n, layer)) return rc;
    if (const int rc = net_begin(n)) return rc;
    net_unlayout(n, layer, n.d_w[layer], n.d_b[layer], d_W, d_b, stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

static int net_get_weights(MlpNet &n, const char *who, int32_t layer, float *W, float *b) {
    if (const int rc = net_check_layer(n, layer)) return rc;
    if (const int rc = net_begin_host(n, who)) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (the staging buffer is one)
    if (const int rc = net_get_weights_device(n, layer, n.d_stage, net_stage_b(n, layer), nullptr)) return rc;
    return net_stage_out(n, layer, W, b);
}

// the normaliser, written, read and derived: all into / out of the net's own d_norm, which never moves
static int net_needs_normalizer(const MlpNet &n, const char *who) {
    if (!n.normalize)
        return fail(CHUB_ERR_ARG, std::string(who) + ": the " + n.noun + " was created with normalize = 0 (its kernel reads no normaliser)");
    return CHUB_OK;
}

static hipError_t net_copy_normalizer(MlpNet &n, const float *mean, const float *inv_std) {
    const hipError_t rc = hipMemcpy(n.d_norm, mean, (size_t) n.F * sizeof(float), hipMemcpyHostToDevice);
    return rc != hipSuccess ? rc : hipMemcpy(n.d_norm + n.F, inv_std, (size_t) n.F * sizeof(float), hipMemcpyHostToDevice);
}

static int net_set_normalizer(MlpNet &n, const char *who, const float *mean, const float *inv_std) {
    if (const int rc = net_needs_normalizer(n, who)) return rc;
    if (const int rc = net_begin_host(n, who)) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (a launch in flight reads the buffer)
    HIP_TRY(net_copy_normalizer(n, mean, inv_std));
    return CHUB_OK;
}

static int net_set_normalizer_device(MlpNet &n, const char *who, const float *d_mean, const float *d_inv_std, void *stream) {
    if (const int rc = net_needs_normalizer(n, who)) return rc;
    if (const int rc = net_begin(n)) return rc;
    HIP_TRY(hipMemcpyAsync(n.d_norm, d_mean, (size_t) n.F * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t) stream));
    HIP_TRY(hipMemcpyAsync(n.d_norm + n.F, d_inv_std, (size_t) n.F * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t) stream));
    return CHUB_OK;
}

static int net_get_normalizer_device(MlpNet &n, const char *who, float *d_mean, float *d_inv_std, void *stream) {
    if (const int rc = net_needs_normalizer(n, who)) return rc;
    if (const int rc = net_begin(n)) return rc;
    HIP_TRY(hipMemcpyAsync(d_mean, n.d_norm, (size_t) n.F * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t) stream));
    HIP_TRY(hipMemcpyAsync(d_inv_std, n.d_norm + n.F, (size_t) n.F * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t) stream));
    return CHUB_OK;
}

// the weights and the normaliser a create call was given, into a net whose buffers stand
static int net_load(MlpNet &n, const char *who, const float *const *W, const float *const *b, const float *mean, const float *inv_std) {
    if (n.normalize && net_copy_normalizer(n, mean, inv_std) != hipSuccess)
        return fail(CHUB_ERR_HIP, std::string(who) + ": mean / inv_std could not be copied to the device");
    for (int l = 0; l < n.n_layers; l++)
        if (const int rc = net_upload(n, l, W[l], b[l])) return rc;
    return CHUB_OK;
}

struct chub_policy {
    MlpNet net;
    chub_policy_spec spec;
    int32_t A_out, waves;
    PolicyArgs pa;                          // everything that does not change from call to call
    float *d_scratch[kPolicyMaxInputs];     // [N][width] of every non-OBS block
    float *d_loads, *d_tail;                // [N][2] each: the LOADS head's outputs; the run loop's tail pair
    uint64_t *d_bits;                       // [N][W]: the run loop's pile bits
    float *d_rows;                          // [N][S + 2]: the run loop's action rows (CHUB_PRUN_AUTORESET)
    uint64_t *d_set;                        // [N][W]: the pile set of a set-aware sampled call that names no buffer of its own
    // sampling (chub_policy_set_exploration): the key of the policy's noise and the Gaussian outputs' log_std [G] (allocated once, never moves)
    int32_t lds_rows, G;                    // rows of the two LDS images; Gaussian outputs (2 PILES, 4 LOADS)
    bool explore;
    uint32_t key[2];
    float *d_log_std;
    std::vector<chub_population *> populations;  // made for this policy (chub_population_create): destroyed before it
    std::vector<chub_policy_grad *> grads;       // made for this policy (chub_policy_grad_create): destroyed before it
};

extern "C" {

// what a spec comes to on a hub of this shape: the feature row's blocks, F, the head's output count and the LDS rows the kernel needs
struct PolicyShape {
    int32_t width[kPolicyMaxInputs];
    int32_t F, A_out, p_rows, q_rows;
};

static int policy_shape(const int32_t piles[2], const chub_policy_spec *sp, PolicyShape &ps) {
    if (piles[0] < 0 || piles[1] < 0 || piles[0] + piles[1] <= 0 || piles[0] > 4096 || piles[1] > 4096)
        return fail(CHUB_ERR_ARG, "station_list: 0 .. 4096 piles per station, at least one pile");
    const int S = piles[0] + piles[1], D = 2 + 4 * ((piles[0] > 0) + (piles[1] > 0)) + 3;
    if (sp->n_inputs < 1 || sp->n_inputs > kPolicyMaxInputs) return fail(CHUB_ERR_ARG, "n_inputs: 1 .. 4");
    if (sp->n_layers < 1 || sp->n_layers > kPolicyMaxLayers) return fail(CHUB_ERR_ARG, "n_layers: 1 .. 4");
    int64_t F = 0;
    for (int i = 0; i < sp->n_inputs; i++) {
        const chub_policy_input &in = sp->inputs[i];
        int w;
        switch (in.kind) {
        case CHUB_PIN_OBS: w = D; break;
        case CHUB_PIN_PILE_OBS:
            if ((w = chub_pile_obs_columns((uint32_t) in.fields)) < 0) return CHUB_ERR_ARG;  // (that call's message)
            w *= S;
            break;
        case CHUB_PIN_STATION_PROFILE:
            if ((w = chub_station_profile_size((uint32_t) in.fields, in.param)) < 0) return CHUB_ERR_ARG;
            break;
        case CHUB_PIN_FORECAST:
            if ((w = chub_forecast_size((uint32_t) in.fields, in.param)) < 0) return CHUB_ERR_ARG;
            break;
        default: return fail(CHUB_ERR_ARG, "inputs[" + std::to_string(i) + "].kind: one of the CHUB_PIN_* kinds");
        }
        ps.width[i] = w;
        F += w;
    }
    if (sp->hidden_act < 0 || sp->hidden_act >= CHUB_PACT_COUNT) return fail(CHUB_ERR_ARG, "hidden_act: CHUB_PACT_TANH or CHUB_PACT_RELU");
    if (sp->head < 0 || sp->head >= CHUB_PHEAD_COUNT) return fail(CHUB_ERR_ARG, "head: CHUB_PHEAD_PILES or CHUB_PHEAD_LOADS");
    if (sp->squash < 0 || sp->squash >= CHUB_PSQ_COUNT) return fail(CHUB_ERR_ARG, "squash: CHUB_PSQ_TANH or CHUB_PSQ_CLIP");
    if (sp->normalize != 0 && sp->normalize != 1) return fail(CHUB_ERR_ARG, "normalize: 0 or 1");
    const int A_out = sp->head == CHUB_PHEAD_PILES ? S + 2 : 4;
    for (int l = 0; l + 1 < sp->n_layers; l++)
        if (sp->width[l] < 1 || sp->width[l] > kPolicyMaxHidden)
            return fail(CHUB_ERR_ARG, "width[" + std::to_string(l) + "]: hidden widths are 1 .. 256");
    if (sp->width[sp->n_layers - 1] != A_out)
        return fail(CHUB_ERR_ARG, "width[n_layers - 1] must be the head's output count, " + std::to_string(A_out));
    if (sp->normalize && !(sp->clip > 0.0f)) return fail(CHUB_ERR_ARG, "clip must be > 0 with normalize");
    // the two LDS images: P the feature row and the outputs of the odd layers, Q the outputs of the even layers (hidden layers only)
    int64_t p_rows = (F + 1) & ~(int64_t) 1, q_rows = 0;
    for (int l = 0; l + 1 < sp->n_layers; l++) {
        const int64_t rows = (int64_t) ((sp->width[l] + kPolicyOutTile - 1) / kPolicyOutTile) * kPolicyOutTile;
        if (l & 1) p_rows = rows > p_rows ? rows : p_rows;
        else q_rows = rows > q_rows ? rows : q_rows;
    }
    if (p_rows + q_rows > kPolicyLdsRows)
        return fail(CHUB_ERR_UNSUPPORTED, "a feature row of " + std::to_string(F) + " floats and these hidden widths need " + std::to_string(p_rows + q_rows) +
                                              " rows of LDS: at most " + std::to_string(kPolicyLdsRows) + " (F <= 256 always fits)");
    ps.F = (int32_t) F;
    ps.A_out = A_out;
    ps.p_rows = (int32_t) p_rows;
    ps.q_rows = (int32_t) q_rows;
    return CHUB_OK;
}

int chub_policy_input_width(const chub_config *cfg, const chub_policy_spec *spec, int32_t *F_out, int32_t *A_out) {
    if (!cfg || !spec || !F_out || !A_out) return fail(CHUB_ERR_ARG, "null argument");
    PolicyShape ps;
    if (const int rc = policy_shape(cfg->station_list, spec, ps)) return rc;
    *F_out = ps.F;
    *A_out = ps.A_out;
    return CHUB_OK;
}

static void population_free(chub_population *pop);
static void policy_grad_free(chub_policy_grad *g);

static void policy_free(chub_policy *pol) {
    chub_env *e = pol->net.env;
    while (!pol->populations.empty()) population_free(pol->populations.back());
    while (!pol->grads.empty()) policy_grad_free(pol->grads.back());
    net_free(pol->net);  // (its synchronise also covers the scratch a launch in flight reads)
    e->policies.erase(std::remove(e->policies.begin(), e->policies.end(), pol), e->policies.end());
    delete pol;
}

int chub_policy_create(chub_env *e, const chub_policy_spec *spec, const float *const *W, const float *const *b, const float *mean,
                       const float *inv_std, chub_policy **out) {
    if (!e || !spec || !W || !b || !out) return fail(CHUB_ERR_ARG, "null argument");
    *out = nullptr;
    PolicyShape ps;
    if (const int rc = policy_shape(e->hp.S, spec, ps)) return rc;
    for (int l = 0; l < spec->n_layers; l++)
        if (!W[l] || !b[l]) return fail(CHUB_ERR_ARG, "null argument");
    if (spec->normalize && (!mean || !inv_std)) return fail(CHUB_ERR_ARG, "normalize needs mean and inv_std");
    if (e->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_policy_create between chub_graph_begin and chub_graph_end (it allocates and synchronises)");
    bool feature_block = false;
    for (int i = 0; i < spec->n_inputs; i++) feature_block |= spec->inputs[i].kind != CHUB_PIN_OBS;
    if (e->tape_only && (feature_block || spec->head == CHUB_PHEAD_LOADS))
        return fail(CHUB_ERR_UNSUPPORTED, "a policy that reads feature blocks or sets station loads is not supported on a tape handle "
                                          "(chub_tape_register_soc rewrites the class tables)");
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();

    chub_policy *pol = new chub_policy();
    MlpNet &net = pol->net;
    net.env = e;
    net.noun = "policy";
    net.row_noun = "feature row";
    net.alloc_who = "chub_policy";
    net.n_layers = spec->n_layers;
    net.F = ps.F;
    net.normalize = spec->normalize != 0;
    pol->spec = *spec;
    pol->A_out = ps.A_out;
    pol->lds_rows = ps.p_rows + ps.q_rows;
    pol->G = spec->head == CHUB_PHEAD_PILES ? 2 : 4;
    e->policies.push_back(pol);
    const size_t N = (size_t) e->hp.n_envs;
    const int S = e->hp.S[0] + e->hp.S[1], Wd = (S + 63) / 64;
    PolicyArgs &pa = pol->pa;
    memset(&pa, 0, sizeof pa);
    pa.n_envs = e->hp.n_envs;
    pa.n_inputs = spec->n_inputs;
    pa.n_layers = spec->n_layers;
    pa.F = ps.F;
    pa.f_pad = (ps.F + 1) & ~1;
    pa.q_row0 = ps.p_rows;
    pa.hidden_act = spec->hidden_act;
    pa.squash = spec->squash;
    pa.normalize = spec->normalize;
    pa.head = spec->head;
    pa.clip = spec->clip;
    pa.S = S;
    pa.A = S + 2;
    pa.W = Wd;
    int max_tiles = 1;
    for (int l = 0; l < spec->n_layers; l++) {
        net.in[l] = l ? spec->width[l - 1] : ps.F;
        net.out[l] = spec->width[l];
        net.tiles[l] = (spec->width[l] + kPolicyOutTile - 1) / kPolicyOutTile;
        // the head's tiles cover every bit word in full: bits from S up are written as zeros, not left alone
        if (l == spec->n_layers - 1 && spec->head == CHUB_PHEAD_PILES && net.tiles[l] < 2 * Wd) net.tiles[l] = 2 * Wd;
        max_tiles = std::max(max_tiles, net.tiles[l]);
    }
    pol->waves = max_tiles < kPolicyMaxWaves ? max_tiles : kPolicyMaxWaves;
    int rc = net_alloc_layers(net);
    for (int l = 0; l < spec->n_layers; l++) pa.layer[l] = {net.d_w[l], net.d_b[l], net.k_pad[l], net.tiles[l]};
    for (int i = 0; i < spec->n_inputs && !rc; i++) {
        pa.in[i].width = ps.width[i];
        pa.in[i].ld = ps.width[i];
        if (spec->inputs[i].kind != CHUB_PIN_OBS) {
            rc = net_alloc(net, &pol->d_scratch[i], N * (size_t) ps.width[i]);
            pa.in[i].p = pol->d_scratch[i];
        }
    }
    if (!rc) rc = net_alloc(net, &pol->d_loads, 2 * N);
    if (!rc) rc = net_alloc(net, &pol->d_tail, 2 * N);
    if (!rc) rc = net_alloc(net, &pol->d_bits, N * (size_t) Wd);
    if (!rc) rc = net_alloc(net, &pol->d_rows, N * (size_t) (S + 2));
    if (!rc) rc = net_alloc(net, &pol->d_set, N * (size_t) Wd);
    if (spec->normalize) {
        pa.mean = net.d_norm;
        pa.inv_std = net.d_norm + ps.F;
    }
    pa.loads = pol->d_loads;
    if (!rc) rc = net_load(net, "chub_policy_create", W, b, mean, inv_std);
    if (rc) {
        const std::string msg = g_err;
        policy_free(pol);
        return fail(rc, msg);
    }
    *out = pol;
    return CHUB_OK;
}

int chub_policy_destroy(chub_policy *pol) {
    if (!pol) return CHUB_OK;
    if (pol->net.env->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_policy_destroy between chub_graph_begin and chub_graph_end (it synchronises and frees)");
    policy_free(pol);
    (void) hipGetLastError();
    return CHUB_OK;
}

int chub_policy_set_weights(chub_policy *pol, int32_t layer, const float *W, const float *b) {
    if (!pol || !W || !b) return fail(CHUB_ERR_ARG, "null argument");
    return net_set_weights(pol->net, "chub_policy_set_weights", layer, W, b);
}

int chub_policy_set_weights_device(chub_policy *pol, int32_t layer, const float *d_W, const float *d_b, void *stream) {
    if (!pol || !d_W || !d_b) return fail(CHUB_ERR_ARG, "null argument");
    return net_set_weights_device(pol->net, layer, d_W, d_b, stream);
}

int chub_policy_get_weights(chub_policy *pol, int32_t layer, float *W, float *b) {
    if (!pol || !W || !b) return fail(CHUB_ERR_ARG, "null argument");
    return net_get_weights(pol->net, "chub_policy_get_weights", layer, W, b);
}

int chub_policy_get_weights_device(chub_policy *pol, int32_t layer, float *d_W, float *d_b, void *stream) {
    if (!pol || !d_W || !d_b) return fail(CHUB_ERR_ARG, "null argument");
    return net_get_weights_device(pol->net, layer, d_W, d_b, stream);
}

// what an evaluation asks of its observation argument, and of the handle (the tape rules of the feature calls)
static int policy_check_obs(const chub_env *e, const chub_policy *pol, const float *d_obs, int64_t ld_obs) {
    bool obs_block = false;
    for (int i = 0; i < pol->spec.n_inputs; i++) obs_block |= pol->spec.inputs[i].kind == CHUB_PIN_OBS;
    if (obs_block && !d_obs) return fail(CHUB_ERR_ARG, "null argument");
    if (obs_block && ld_obs < e->hp.obs_dim) return fail(CHUB_ERR_ARG, "ld_obs: at least the observation's " + std::to_string(e->hp.obs_dim) + " floats");
    return CHUB_OK;
}

static int policy_check_tape(const chub_env *e, const chub_policy *pol) {
    bool feature_block = false;
    for (int i = 0; i < pol->spec.n_inputs; i++) feature_block |= pol->spec.inputs[i].kind != CHUB_PIN_OBS;
    if (e->tape_only && (feature_block || pol->spec.head == CHUB_PHEAD_LOADS))
        return fail(CHUB_ERR_UNSUPPORTED, "a policy that reads feature blocks or sets station loads is not supported on a tape handle "
                                          "(chub_tape_register_soc rewrites the class tables)");
    return CHUB_OK;
}

// the feature launches of the spec's non-OBS blocks into the policy's scratch; the OBS blocks point at the caller's rows
static int policy_feature_blocks(chub_env *e, chub_policy *pol, const float *d_obs, int64_t ld_obs, const uint8_t *d_mask, PolicyArgs &pa, void *stream) {
    const chub_policy_spec &sp = pol->spec;
    for (int i = 0; i < sp.n_inputs; i++) {
        const chub_policy_input &in = sp.inputs[i];
        int rc = CHUB_OK;
        switch (in.kind) {
        case CHUB_PIN_OBS:
            pa.in[i].p = d_obs;
            pa.in[i].ld = ld_obs;
            break;
        case CHUB_PIN_PILE_OBS: rc = chub_pile_obs_device(e, (uint32_t) in.fields, d_mask, pol->d_scratch[i], stream); break;
        case CHUB_PIN_STATION_PROFILE: rc = chub_station_profile_device(e, (uint32_t) in.fields, in.param, d_mask, pol->d_scratch[i], stream); break;
        default: rc = chub_forecast_device(e, (uint32_t) in.fields, in.param, d_mask, pol->d_scratch[i], stream); break;
        }
        if (rc) return rc;
    }
    return CHUB_OK;
}

// everything a deterministic evaluation refuses for, with nothing enqueued yet
static int policy_act_check(const chub_env *e, const chub_policy *pol, const float *d_obs, int64_t ld_obs, const float *d_actions,
                            const uint64_t *d_pile_bits, const float *d_tail) {
    if (pol->net.env != e) return fail(CHUB_ERR_ARG, "this policy was made for another handle");
    if (const int rc = policy_check_obs(e, pol, d_obs, ld_obs)) return rc;
    if (!d_actions && !d_pile_bits) return fail(CHUB_ERR_ARG, "chub_policy_act: give d_actions, d_pile_bits or both");
    if (pol->spec.head == CHUB_PHEAD_PILES && d_pile_bits && !d_tail) return fail(CHUB_ERR_ARG, "chub_policy_act: pile bits need d_tail (the two tail actions)");
    return policy_check_tape(e, pol);
}

// one deterministic evaluation, checked by the caller.  pop == nullptr: the policy's own weights (chub_policy_act_device); else the members
// of a population of this policy, member m for envs [m E, (m + 1) E) (chub_population_act_device)
static void population_args(const chub_population *pop, const PolicyArgs &pa, PolicyPopArgs &out);
static int policy_act_enqueue(chub_env *e, chub_policy *pol, const chub_population *pop, const float *d_obs, int64_t ld_obs, const uint8_t *d_mask,
                              float *d_actions, uint64_t *d_pile_bits, float *d_tail, void *stream) {
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    PolicyArgs pa = pol->pa;
    if (const int rc = policy_feature_blocks(e, pol, d_obs, ld_obs, d_mask, pa, stream)) return rc;
    const bool loads = pol->spec.head == CHUB_PHEAD_LOADS;
    pa.mask = d_mask;
    pa.actions = loads ? nullptr : d_actions;
    pa.bits = loads ? nullptr : (uint32_t *) d_pile_bits;
    pa.tail = d_tail ? d_tail : (loads ? pol->d_tail : nullptr);
    if (pop) {
        PolicyPopArgs pp;
        population_args(pop, pa, pp);
        launch_policy_pop(pp, pol->waves, (hipStream_t) stream);
    } else {
        launch_policy(pa, pol->waves, (hipStream_t) stream);
    }
    HIP_TRY(hipGetLastError());
    if (loads) return chub_load_dispatch_device(e, CHUB_LOAD_FRACTION, pol->d_loads, pa.tail, d_mask, d_actions, d_pile_bits, stream);
    return CHUB_OK;
}

int chub_policy_act_device(chub_env *e, chub_policy *pol, const float *d_obs, int64_t ld_obs, const uint8_t *d_mask, float *d_actions,
                           uint64_t *d_pile_bits, float *d_tail, void *stream) {
    if (!e || !pol) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = policy_act_check(e, pol, d_obs, ld_obs, d_actions, d_pile_bits, d_tail)) return rc;
    return policy_act_enqueue(e, pol, nullptr, d_obs, ld_obs, d_mask, d_actions, d_pile_bits, d_tail, stream);
}

int chub_policy_act(chub_env *e, chub_policy *pol, const float *obs, float *actions) {
    if (!e || !pol || !actions) return fail(CHUB_ERR_ARG, "null argument");
    if (pol->net.env != e) return fail(CHUB_ERR_ARG, "this policy was made for another handle");
    if (e->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_policy_act between chub_graph_begin and chub_graph_end (it allocates and synchronises)");
    bool obs_block = false;
    for (int i = 0; i < pol->spec.n_inputs; i++) obs_block |= pol->spec.inputs[i].kind == CHUB_PIN_OBS;
    if (obs_block && !obs) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t N = (size_t) e->hp.n_envs, D = (size_t) e->hp.obs_dim, A = (size_t) e->hp.act_dim;
    const size_t b_obs = N * D * sizeof(float), b_act = N * A * sizeof(float);
    char *d = nullptr;  // obs | rows, one allocation
    HIP_TRY(hipMalloc((void **) &d, b_obs + b_act));
    float *d_obs = (float *) d, *d_act = (float *) (d + b_obs);
    int rc = CHUB_OK;
    if (obs_block && hipMemcpy(d_obs, obs, b_obs, hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(CHUB_ERR_HIP, "chub_policy_act: the observations could not be copied to the device");
    if (!rc) rc = chub_policy_act_device(e, pol, d_obs, (int64_t) D, nullptr, d_act, nullptr, pol->d_tail, nullptr);
    if (!rc && (hipDeviceSynchronize() != hipSuccess || hipMemcpy(actions, d_act, b_act, hipMemcpyDeviceToHost) != hipSuccess))
        rc = fail(CHUB_ERR_HIP, "chub_policy_act: the launch failed or its output could not be copied back");
    (void) hipFree(d);
    return rc;
}

// The closed loop: what a host loop of chub_reset_device / chub_policy_act_device / chub_step_bits_device_packed (or
// chub_autoreset_step_device) calls does, with nothing on the host between the steps.  pop == nullptr: chub_policy_run_steps; else the
// population's actor in the policy's place (chub_population_run_steps)
static int policy_run(chub_env *e, chub_policy *pol, const chub_population *pop, int mode, float *const *d_packed2, float *d_reset_obs, float *d_final_obs,
                      int64_t first_step, int64_t n_steps, void *stream) {
    const char *who = pop ? "chub_population_run_steps" : "chub_policy_run_steps";
    if (!e || !pol || !d_packed2 || !d_packed2[0] || !d_packed2[1] || first_step < 0 || n_steps < 0) return fail(CHUB_ERR_ARG, "bad argument");
    if (pol->net.env != e) return fail(CHUB_ERR_ARG, "this policy was made for another handle");
    if (mode != CHUB_PRUN_LOCKSTEP && mode != CHUB_PRUN_AUTORESET) return fail(CHUB_ERR_ARG, "mode: CHUB_PRUN_LOCKSTEP or CHUB_PRUN_AUTORESET");
    if (mode == CHUB_PRUN_LOCKSTEP && !d_reset_obs) return fail(CHUB_ERR_ARG, "bad argument");
    if (e->hp.rng_mode == CHUB_RNG_COMPAT)
        return fail(CHUB_ERR_UNSUPPORTED, std::string(who) + " runs the Philox modes: COMPAT steps take the caller's normals one by one");
    if (mode == CHUB_PRUN_AUTORESET && e->tick == 0) return fail(CHUB_ERR_ARG, "step() before reset()");
    const int D = e->hp.obs_dim;
    for (int64_t i = first_step; i < first_step + n_steps; i++) {
        int rc;
        const float *obs = d_packed2[(i - 1) & 1];
        int64_t ld = D + 2;
        const bool lock = mode == CHUB_PRUN_LOCKSTEP;
        if (lock && i % 96 == 0) {
            if ((rc = chub_reset_device(e, nullptr, nullptr, d_reset_obs, stream))) return rc;
            obs = d_reset_obs;
            ld = D;
        } else if (!lock && i == first_step && d_reset_obs) {
            obs = d_reset_obs;
            ld = D;
        }
        float *rows = lock ? nullptr : pol->d_rows;
        uint64_t *bits = lock ? pol->d_bits : nullptr;
        float *tail = lock ? pol->d_tail : nullptr;
        if ((rc = policy_act_check(e, pol, obs, ld, rows, bits, tail))) return rc;
        if ((rc = policy_act_enqueue(e, pol, pop, obs, ld, nullptr, rows, bits, tail, stream))) return rc;
        if (lock) rc = chub_step_bits_device_packed(e, pol->d_bits, pol->d_tail, nullptr, d_packed2[i & 1], stream);
        else rc = chub_autoreset_step_device(e, pol->d_rows, nullptr, nullptr, nullptr, d_packed2[i & 1], d_final_obs, stream);
        if (rc) return rc;
    }
    return CHUB_OK;
}

int chub_policy_run_steps(chub_env *e, chub_policy *pol, int mode, float *const *d_packed2, float *d_reset_obs, float *d_final_obs,
                          int64_t first_step, int64_t n_steps, void *stream) {
    return policy_run(e, pol, nullptr, mode, d_packed2, d_reset_obs, d_final_obs, first_step, n_steps, stream);
}

// ---- sampling from the device actor (include/chub.h): exploration noise, log-probabilities, rollouts that keep the trajectory
static_assert((uint32_t) SITE_POLICY == kPolicySite, "chub_policy.h restates SITE_POLICY of chub_device.h");

int chub_next_tick(const chub_env *e, uint32_t *out) {
    if (!e || !out) return fail(CHUB_ERR_ARG, "null argument");
    *out = e->tick + 1u;
    return CHUB_OK;
}

int chub_policy_set_exploration(chub_policy *pol, uint64_t key, const float *log_std) {
    if (!pol || !log_std) return fail(CHUB_ERR_ARG, "null argument");
    chub_env *e = pol->net.env;
    for (int i = 0; i < pol->G; i++)
        if (!std::isfinite(log_std[i])) return fail(CHUB_ERR_ARG, "log_std[" + std::to_string(i) + "] is not finite");
    if (e->capturing)
        return fail(CHUB_ERR_UNSUPPORTED, "chub_policy_set_exploration between chub_graph_begin and chub_graph_end (it copies and synchronises: use "
                                          "chub_policy_set_log_std_device)");
    if (pol->lds_rows + kPolicyLogpRows > kPolicyLdsRows)
        return fail(CHUB_ERR_UNSUPPORTED, "the sampled launch needs " + std::to_string(kPolicyLogpRows) + " rows of LDS behind this policy's " +
                                              std::to_string(pol->lds_rows) + ": at most " + std::to_string(kPolicyLdsRows) + " together");
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    HIP_TRY(hipDeviceSynchronize());  // (a sampled launch in flight reads the buffer)
    if (!pol->d_log_std)
        if (const int rc = net_alloc(pol->net, &pol->d_log_std, 4)) return rc;
    HIP_TRY(hipMemcpy(pol->d_log_std, log_std, (size_t) pol->G * sizeof(float), hipMemcpyHostToDevice));
    pol->key[0] = (uint32_t) key;  // (split as the env's seed is)
    pol->key[1] = (uint32_t) (key >> 32);
    pol->explore = true;
    return CHUB_OK;
}

int chub_policy_set_log_std_device(chub_policy *pol, const float *d_log_std, void *stream) {
    if (!pol || !d_log_std) return fail(CHUB_ERR_ARG, "null argument");
    if (!pol->explore) return fail(CHUB_ERR_ARG, "chub_policy_set_exploration first (it makes the policy's log_std buffer)");
    HIP_TRY(hipSetDevice(pol->net.env->device));
    (void) hipGetLastError();
    HIP_TRY(hipMemcpyAsync(pol->d_log_std, d_log_std, (size_t) pol->G * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t) stream));
    return CHUB_OK;
}

// everything chub_policy_sample_device refuses for, with nothing enqueued yet
static int policy_sample_check(chub_env *e, chub_policy *pol, const float *d_obs, int64_t ld_obs, const chub_policy_sample_out *out) {
    if (!e || !pol || !out) return fail(CHUB_ERR_ARG, "null argument");
    if (pol->net.env != e) return fail(CHUB_ERR_ARG, "this policy was made for another handle");
    if (!pol->explore) return fail(CHUB_ERR_ARG, "chub_policy_sample: chub_policy_set_exploration first (the key and log_std)");
    if (const int rc = policy_check_obs(e, pol, d_obs, ld_obs)) return rc;
    if (!out->d_logp) return fail(CHUB_ERR_ARG, "chub_policy_sample: d_logp is required");
    if (pol->spec.head == CHUB_PHEAD_PILES && out->d_pile_bits && !out->d_tail)
        return fail(CHUB_ERR_ARG, "chub_policy_sample: pile bits need d_tail (the two tail actions)");
    return policy_check_tape(e, pol);
}

// what the set-aware calls refuse on top, with nothing enqueued yet (after policy_sample_check: pol and e are good)
static int policy_set_check(const chub_env *e, const chub_policy *pol, int which, const char *who) {
    if (const int rc = pile_set_check(e, which, who)) return rc;
    if (which != CHUB_PSET_ALL && pol->spec.head == CHUB_PHEAD_LOADS)
        return fail(CHUB_ERR_ARG, std::string(who) + ": under CHUB_PHEAD_LOADS the log-probability has no pile terms: which must be CHUB_PSET_ALL");
    return CHUB_OK;
}

// one sampled evaluation, checked by the caller.  which < 0: chub_policy_sample_device's launches; else the pile set launch in front, with the
// same mask, and the set-aware actor launch
static int policy_sample_enqueue(chub_env *e, chub_policy *pol, const float *d_obs, int64_t ld_obs, const uint8_t *d_mask, int which,
                                 uint64_t *d_set_bits, const chub_policy_sample_out *out, void *stream) {
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    PolicySampleSetArgs sa;
    static_cast<PolicyArgs &>(sa) = pol->pa;
    sa.set = nullptr;
    if (which >= 0) {
        uint64_t *set = d_set_bits ? d_set_bits : pol->d_set;
        if (const int rc = chub_pile_set_device(e, which, d_mask, set, stream)) return rc;
        sa.set = (const uint32_t *) set;
    }
    if (const int rc = policy_feature_blocks(e, pol, d_obs, ld_obs, d_mask, sa, stream)) return rc;
    const bool loads = pol->spec.head == CHUB_PHEAD_LOADS;
    sa.mask = d_mask;
    sa.actions = loads ? nullptr : out->d_actions;
    sa.bits = loads ? nullptr : (uint32_t *) out->d_pile_bits;
    sa.tail = out->d_tail ? out->d_tail : (loads ? pol->d_tail : nullptr);
    sa.tick_base = e->d_tick_base;
    sa.log_std = pol->d_log_std;
    sa.normal_icdf = (const float *) e->tb.normal_icdf;
    sa.normal_tail = (const float *) e->tb.normal_tail;
    sa.u = out->d_u;
    sa.logp = out->d_logp;
    sa.features = out->d_features;
    sa.key[0] = pol->key[0];
    sa.key[1] = pol->key[1];
    sa.tick = e->tick + 1u - e->graph_base;  // the argument the handle's next launch carries: + *tick_base on the device (CHUB_TICK)
    sa.gid0 = (uint32_t) e->hp.env_id0;
    sa.G = pol->G;
    sa.r_row0 = 0;
    if (which >= 0) launch_policy_sample_set(sa, pol->waves, (hipStream_t) stream);
    else launch_policy_sample(sa, pol->waves, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    if (loads && (out->d_actions || out->d_pile_bits))
        return chub_load_dispatch_device(e, CHUB_LOAD_FRACTION, pol->d_loads, sa.tail, d_mask, out->d_actions, out->d_pile_bits, stream);
    return CHUB_OK;
}

int chub_policy_sample_device(chub_env *e, chub_policy *pol, const float *d_obs, int64_t ld_obs, const uint8_t *d_mask,
                              const chub_policy_sample_out *out, void *stream) {
    if (const int rc = policy_sample_check(e, pol, d_obs, ld_obs, out)) return rc;
    return policy_sample_enqueue(e, pol, d_obs, ld_obs, d_mask, -1, nullptr, out, stream);
}

int chub_policy_sample_set_device(chub_env *e, chub_policy *pol, const float *d_obs, int64_t ld_obs, const uint8_t *d_mask, int which,
                                  uint64_t *d_set_bits, const chub_policy_sample_out *out, void *stream) {
    if (const int rc = policy_sample_check(e, pol, d_obs, ld_obs, out)) return rc;
    if (const int rc = policy_set_check(e, pol, which, "chub_policy_sample_set_device")) return rc;
    return policy_sample_enqueue(e, pol, d_obs, ld_obs, d_mask, which, d_set_bits, out, stream);
}

// The closed loop that keeps what a trainer needs: a host loop of the calls the header lists, like chub_policy_run_steps.  which < 0:
// chub_policy_collect; else chub_policy_collect_set, whose step t also leaves its pile set in d_set_bits[t]
static int policy_collect(chub_env *e, chub_policy *pol, int mode, int which, const chub_rollout *r, uint64_t *d_set_bits, float *d_obs0,
                          int64_t first_step, void *stream, uint32_t fields = 0u, float *d_terms = nullptr) {
    if (!e || !pol || !r || !d_obs0 || (which >= 0 && !d_set_bits)) return fail(CHUB_ERR_ARG, "null argument");
    if (pol->net.env != e) return fail(CHUB_ERR_ARG, "this policy was made for another handle");
    if (mode != CHUB_PRUN_LOCKSTEP && mode != CHUB_PRUN_AUTORESET) return fail(CHUB_ERR_ARG, "mode: CHUB_PRUN_LOCKSTEP or CHUB_PRUN_AUTORESET");
    if (!r->d_packed || !r->d_pile_bits || !r->d_tail || !r->d_u || !r->d_logp)
        return fail(CHUB_ERR_ARG, "chub_policy_collect: d_packed, d_pile_bits, d_tail, d_u and d_logp are required");
    if (r->T <= 0 || first_step < 0) return fail(CHUB_ERR_ARG, "chub_policy_collect: T >= 1 steps from first_step >= 0");
    if (mode == CHUB_PRUN_LOCKSTEP && first_step % 96 + r->T > 96)
        return fail(CHUB_ERR_ARG, "chub_policy_collect: a lock-step rollout stays inside one day (first_step % 96 + T <= 96)");
    if (mode == CHUB_PRUN_AUTORESET && r->T > 96)
        return fail(CHUB_ERR_ARG, "chub_policy_collect: T <= 96 (an env finishes at most once, so a row of d_final_obs is written at most once)");
    if (e->hp.rng_mode == CHUB_RNG_COMPAT)
        return fail(CHUB_ERR_UNSUPPORTED, "chub_policy_collect runs the Philox modes: COMPAT steps take the caller's normals one by one");
    if (mode == CHUB_PRUN_AUTORESET && e->tick == 0) return fail(CHUB_ERR_ARG, "step() before reset()");
    chub_policy_sample_out probe = {};
    probe.d_logp = r->d_logp;
    probe.d_pile_bits = r->d_pile_bits;
    probe.d_tail = r->d_tail;
    if (const int rc = policy_sample_check(e, pol, d_obs0, e->hp.obs_dim, &probe)) return rc;
    if (which >= 0)
        if (const int rc = policy_set_check(e, pol, which, "chub_policy_collect_set")) return rc;
    const size_t N = (size_t) e->hp.n_envs, D = (size_t) e->hp.obs_dim, Wd = (size_t) ((e->hp.S[0] + e->hp.S[1] + 63) / 64);
    int rc;
    if (mode == CHUB_PRUN_LOCKSTEP && first_step % 96 == 0 && (rc = chub_reset_device(e, nullptr, nullptr, d_obs0, stream))) return rc;
    // chub_policy_collect_terms: step t's terms go to block t of d_terms; the handle's own attachment is in force again on every way out
    struct TermsGuard {
        chub_env *e;
        float *out;
        uint32_t fields;
        ~TermsGuard() {
            e->st_out = out;
            e->st_fields = fields;
        }
    } guard = {e, e->st_out, e->st_fields};
    const size_t Ct = d_terms ? (size_t) __builtin_popcount(fields) : 0;
    for (int64_t t = 0; t < r->T; t++) {
        const size_t k = (size_t) t;
        if (d_terms) {
            e->st_out = d_terms + k * N * Ct;
            e->st_fields = fields;
        }
        const float *obs = t ? r->d_packed + (k - 1) * N * (D + 2) : d_obs0;
        const int64_t ld = t ? (int64_t) D + 2 : (int64_t) D;
        float *packed = r->d_packed + k * N * (D + 2);
        chub_policy_sample_out o;
        o.d_actions = mode == CHUB_PRUN_AUTORESET ? pol->d_rows : nullptr;
        o.d_pile_bits = r->d_pile_bits + k * N * Wd;
        o.d_tail = r->d_tail + k * N * 2;
        o.d_u = r->d_u + k * N * (size_t) pol->G;
        o.d_logp = r->d_logp + k * N;
        o.d_features = r->d_features ? r->d_features + k * N * (size_t) pol->net.F : nullptr;
        if ((rc = policy_sample_enqueue(e, pol, obs, ld, nullptr, which, which >= 0 ? d_set_bits + k * N * Wd : nullptr, &o, stream))) return rc;
        if (mode == CHUB_PRUN_LOCKSTEP) rc = chub_step_bits_device_packed(e, o.d_pile_bits, o.d_tail, nullptr, packed, stream);
        else rc = chub_autoreset_step_device(e, pol->d_rows, nullptr, nullptr, nullptr, packed, r->d_final_obs, stream);
        if (rc) return rc;
    }
    return CHUB_OK;
}

int chub_policy_collect(chub_env *e, chub_policy *pol, int mode, const chub_rollout *r, float *d_obs0, int64_t first_step, void *stream) {
    return policy_collect(e, pol, mode, -1, r, nullptr, d_obs0, first_step, stream);
}

int chub_policy_collect_set(chub_env *e, chub_policy *pol, int mode, int which, const chub_rollout *r, uint64_t *d_set_bits, float *d_obs0,
                            int64_t first_step, void *stream) {
    if (which < 0 || which >= CHUB_PSET_COUNT)
        return fail(CHUB_ERR_ARG, "chub_policy_collect_set: which is CHUB_PSET_ALL, CHUB_PSET_OCCUPIED or CHUB_PSET_DECIDABLE");
    return policy_collect(e, pol, mode, which, r, d_set_bits, d_obs0, first_step, stream);
}

// chub_policy_collect(_set) that keeps every step's terms (include/chub.h, "constrained PPO on the device"): policy_collect is the loop; the
// step forms read e->st_out / e->st_fields when they enqueue, so the per-step destination is a launch argument and nothing is attached
int chub_policy_collect_terms(chub_env *e, chub_policy *pol, int mode, int which, const chub_rollout *r, uint64_t *d_set_bits, float *d_obs0,
                              int64_t first_step, uint32_t fields, float *d_terms, void *stream) {
    if (const int rc = check_step_terms(e, fields, d_terms)) return rc;
    if (which >= CHUB_PSET_COUNT)
        return fail(CHUB_ERR_ARG, "chub_policy_collect_terms: which is negative (chub_policy_collect), CHUB_PSET_ALL, CHUB_PSET_OCCUPIED or CHUB_PSET_DECIDABLE");
    return policy_collect(e, pol, mode, which < 0 ? -1 : which, r, d_set_bits, d_obs0, first_step, stream, fields, d_terms);
}

// ---- advantages (include/chub.h, chub_rollout_gae_device): the env supplies N and D and the partials of the statistics, nothing else.
// The horizon and the discounts of every GAE call, refused in the caller's name
static int gae_check_T(const char *who, int64_t T) {
    return T <= 0 ? fail(CHUB_ERR_ARG, std::string(who) + ": T >= 1") : CHUB_OK;
}

static int gae_check_discounts(const char *who, float gamma, float lambda) {
    if (!(gamma >= 0.0f && gamma <= 1.0f) || !(lambda >= 0.0f && lambda <= 1.0f))
        return fail(CHUB_ERR_ARG, std::string(who) + ": gamma and lambda lie in [0, 1]");
    return CHUB_OK;
}

// a chub_gae checked and, on the env's device, stated as the unscaled launch's arguments
static int gae_args(GaeArgs *a, const char *who, chub_env *e, const chub_gae *g) {
    if (!g->d_packed || !g->d_values || !g->d_adv) return fail(CHUB_ERR_ARG, std::string(who) + ": d_packed, d_values and d_adv are required");
    if (const int rc = gae_check_T(who, g->T)) return rc;
    if (const int rc = gae_check_discounts(who, g->gamma, g->lambda)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    a->n_envs = e->hp.n_envs;
    a->T = g->T;
    a->D = e->hp.obs_dim;
    a->gamma = g->gamma;
    a->gl = g->gamma * g->lambda;
    a->clip = 0.0f;
    a->scale = nullptr;
    a->packed = g->d_packed;
    a->values = g->d_values;
    a->final_values = g->d_final_values;
    a->mask = g->d_mask;
    a->adv = g->d_adv;
    a->ret = g->d_ret;
    a->partials = g->d_stats ? e->d_gae_part : nullptr;
    a->stats = g->d_stats;
    return CHUB_OK;
}

int chub_rollout_gae_device(chub_env *e, const chub_gae *g, void *stream) {
    if (!e || !g) return fail(CHUB_ERR_ARG, "null argument");
    GaeArgs a;
    if (const int rc = gae_args(&a, "chub_rollout_gae_device", e, g)) return rc;
    launch_gae(a, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

}  // extern "C"

// ---- running feature statistics (include/chub.h): the state [1 + 2F] f64 and the partials of the two launches, owned by the object, outside
// the arena.  The kernels are chub_policy.hip's k_moments / k_moments_merge; here: validation, ownership and the launch shape.
struct chub_moments {
    chub_env *env;
    int32_t F, L, RW;    // columns; lanes along a row and rows per workgroup pass (chub_policy.h, MomentsArgs)
    int32_t grid;        // workgroups of launch 1 at most, chosen once at create from F and the device's CU count
    double *d_state;     // [1 + 2F]: n | mean[F] | M2[F] (never moves)
    double *d_part;      // [grid][1 + 2F], then the pivots [1 + F]
};

extern "C" {

constexpr int kMomentsMaxF = 512;
constexpr int kMomentsBlocksPerCu = 4;               // 4 workgroups x 256 lanes x kMomentsAhead loads: 32 KiB in flight per CU
constexpr size_t kMomentsPartialBytes = 4u << 20;    // the partials stay at most this large

static void moments_free(chub_moments *m) {
    chub_env *e = m->env;
    (void) hipSetDevice(e->device);
    (void) hipDeviceSynchronize();  // (a launch still in flight reads and writes the buffers)
    if (m->d_state) (void) hipFree(m->d_state);
    if (m->d_part) (void) hipFree(m->d_part);
    e->moments.erase(std::remove(e->moments.begin(), e->moments.end(), m), e->moments.end());
    delete m;
}

int chub_moments_create(chub_env *e, int32_t F, chub_moments **out) {
    if (!e || !out) return fail(CHUB_ERR_ARG, "null argument");
    *out = nullptr;
    if (F < 1 || F > kMomentsMaxF) return fail(CHUB_ERR_ARG, "chub_moments_create: F is 1 .. " + std::to_string(kMomentsMaxF));
    if (e->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_moments_create between chub_graph_begin and chub_graph_end (it allocates and synchronises)");
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device));
    const size_t row = (size_t) (1 + 2 * F) * sizeof(double);
    int64_t grid = (int64_t) kMomentsBlocksPerCu * (cus > 0 ? cus : 1);
    if ((size_t) grid * row > kMomentsPartialBytes) grid = (int64_t) (kMomentsPartialBytes / row);
    chub_moments *m = new chub_moments();
    m->env = e;
    m->F = F;
    m->L = F < kMomentsLanes ? F : kMomentsLanes;
    m->RW = kMomentsLanes / m->L;
    m->grid = (int32_t) grid;
    e->moments.push_back(m);
    const size_t part = (size_t) grid * row + (size_t) (1 + F) * sizeof(double);
    if (hipMalloc((void **) &m->d_state, row) != hipSuccess || hipMalloc((void **) &m->d_part, part) != hipSuccess ||
        hipMemset(m->d_state, 0, row) != hipSuccess || hipMemset(m->d_part, 0, part) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        moments_free(m);
        (void) hipGetLastError();
        return fail(CHUB_ERR_HIP, "chub_moments_create: out of device memory");
    }
    *out = m;
    return CHUB_OK;
}

int chub_moments_destroy(chub_moments *m) {
    if (!m) return CHUB_OK;
    if (m->env->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_moments_destroy between chub_graph_begin and chub_graph_end (it synchronises and frees)");
    moments_free(m);
    (void) hipGetLastError();
    return CHUB_OK;
}

int chub_moments_update_device(chub_moments *m, const float *d_x, int64_t ld, int64_t R, const uint8_t *d_mask, void *stream) {
    if (!m || !d_x) return fail(CHUB_ERR_ARG, "null argument");
    if (ld < m->F) return fail(CHUB_ERR_ARG, "chub_moments_update_device: ld is at least F = " + std::to_string(m->F) + " floats");
    if (R <= 0) return fail(CHUB_ERR_ARG, "chub_moments_update_device: R >= 1");
    const int64_t N = m->env->hp.n_envs;
    if (d_mask && R % N != 0)
        return fail(CHUB_ERR_ARG, "chub_moments_update_device: with a mask R is a multiple of the handle's " + std::to_string(N) + " envs (row r belongs to env r % N)");
    HIP_TRY(hipSetDevice(m->env->device));
    (void) hipGetLastError();
    MomentsArgs a;
    a.x = d_x;
    a.ld = ld;
    a.R = R;
    a.passes = (R + m->RW - 1) / m->RW;
    a.F = m->F;
    a.L = m->L;
    a.RW = m->RW;
    a.blocks = (int32_t) (a.passes < m->grid ? a.passes : m->grid);
    a.n_envs = N;
    a.e_step = ((int64_t) a.blocks * m->RW) % N;
    a.mask = d_mask;
    a.state = m->d_state;
    a.partials = m->d_part;
    a.pivot = m->d_part + (size_t) m->grid * (size_t) (1 + 2 * m->F);
    launch_moments(a, m->d_state, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_moments_reset_device(chub_moments *m, void *stream) {
    if (!m) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(m->env->device));
    (void) hipGetLastError();
    HIP_TRY(hipMemsetAsync(m->d_state, 0, (size_t) (1 + 2 * m->F) * sizeof(double), (hipStream_t) stream));
    return CHUB_OK;
}

int chub_moments_get(chub_moments *m, double *count, double *mean, double *m2) {
    if (!m || !count || !mean || !m2) return fail(CHUB_ERR_ARG, "null argument");
    if (m->env->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_moments_get between chub_graph_begin and chub_graph_end (it synchronises)");
    HIP_TRY(hipSetDevice(m->env->device));
    (void) hipGetLastError();
    HIP_TRY(hipDeviceSynchronize());
    std::vector<double> h((size_t) (1 + 2 * m->F));
    HIP_TRY(hipMemcpy(h.data(), m->d_state, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    *count = h[0];
    memcpy(mean, h.data() + 1, (size_t) m->F * sizeof(double));
    memcpy(m2, h.data() + 1 + m->F, (size_t) m->F * sizeof(double));
    return CHUB_OK;
}

int chub_moments_set(chub_moments *m, double count, const double *mean, const double *m2) {
    if (!m || !mean || !m2) return fail(CHUB_ERR_ARG, "null argument");
    if (!std::isfinite(count) || count < 0.0) return fail(CHUB_ERR_ARG, "chub_moments_set: count is finite and >= 0");
    if (m->env->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_moments_set between chub_graph_begin and chub_graph_end (it copies and synchronises)");
    HIP_TRY(hipSetDevice(m->env->device));
    (void) hipGetLastError();
    HIP_TRY(hipDeviceSynchronize());  // (an update in flight reads and writes the state)
    std::vector<double> h((size_t) (1 + 2 * m->F));
    h[0] = count;
    memcpy(h.data() + 1, mean, (size_t) m->F * sizeof(double));
    memcpy(h.data() + 1 + m->F, m2, (size_t) m->F * sizeof(double));
    HIP_TRY(hipMemcpy(m->d_state, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    return CHUB_OK;
}

int chub_moments_state_device(chub_moments *m, const double **d_state) {
    if (!m || !d_state) return fail(CHUB_ERR_ARG, "null argument");
    *d_state = m->d_state;
    return CHUB_OK;
}

// ---- a net's normaliser derived from the moments; the policy's normaliser calls (include/chub.h)
static int net_normalizer_from_moments(MlpNet &n, const char *who, chub_moments *m, double eps, void *stream) {
    if (const int rc = net_needs_normalizer(n, who)) return rc;
    if (m->env != n.env) return fail(CHUB_ERR_ARG, std::string(who) + ": the " + n.noun + " and the moments were made for different handles");
    if (m->F != n.F)
        return fail(CHUB_ERR_ARG, std::string(who) + ": the moments have F = " + std::to_string(m->F) + ", the " + n.noun + "'s " + n.row_noun + " " +
                                      std::to_string(n.F));
    if (!(eps > 0.0) || !std::isfinite(eps)) return fail(CHUB_ERR_ARG, std::string(who) + ": eps is finite and > 0");
    if (const int rc = net_begin(n)) return rc;
    launch_normalizer_from_moments(m->d_state, n.F, eps, n.d_norm, n.d_norm + n.F, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_policy_set_normalizer(chub_policy *pol, const float *mean, const float *inv_std) {
    if (!pol || !mean || !inv_std) return fail(CHUB_ERR_ARG, "null argument");
    return net_set_normalizer(pol->net, "chub_policy_set_normalizer", mean, inv_std);
}

int chub_policy_set_normalizer_device(chub_policy *pol, const float *d_mean, const float *d_inv_std, void *stream) {
    if (!pol || !d_mean || !d_inv_std) return fail(CHUB_ERR_ARG, "null argument");
    return net_set_normalizer_device(pol->net, "chub_policy_set_normalizer_device", d_mean, d_inv_std, stream);
}

int chub_policy_get_normalizer_device(chub_policy *pol, float *d_mean, float *d_inv_std, void *stream) {
    if (!pol || !d_mean || !d_inv_std) return fail(CHUB_ERR_ARG, "null argument");
    return net_get_normalizer_device(pol->net, "chub_policy_get_normalizer_device", d_mean, d_inv_std, stream);
}

int chub_policy_normalizer_from_moments_device(chub_policy *pol, chub_moments *m, double eps, void *stream) {
    if (!pol || !m) return fail(CHUB_ERR_ARG, "null argument");
    return net_normalizer_from_moments(pol->net, "chub_policy_normalizer_from_moments_device", m, eps, stream);
}

}  // extern "C"

// ---- a population of actors (include/chub.h): P members' weights in the kernel's layout, perturbed, evaluated and differentiated (ES) on the
// device.  The kernels are chub_policy.hip's; here: validation, ownership and the calls' order.
static_assert((uint32_t) SITE_POPULATION == kPopulationSite, "chub_policy.h restates SITE_POPULATION of chub_device.h");
// the noise counter's first word is row << 8 | k >> 2: column k <= in <= 512 gives a group <= 128 < 2^8, row <= 8193 < 2^24
static_assert(kPolicyLdsRows <= 512 && kPolicyMaxHidden <= 512, "a layer's inputs (the feature row or a hidden width) are at most 512");
static_assert((512 >> 2) < (1 << 8) && (uint64_t) (2 * 4096 + 2 - 1) == 8193u && (8193ull << 8 | 0xFFull) <= 0xFFFFFFFFull,
              "the fields of the population noise counter stay apart");

struct chub_population {
    chub_policy *pol;
    int32_t P, E;
    uint32_t key[2];
    float *d_params;                         // [P][member_floats]: per member every layer's [tiles][k_pad][32] and [tiles * 32] (never moves)
    float *d_stage;                          // [P][member_floats]: chub_population_copy_members_device reads every source into it first
    int64_t member_floats;
    int64_t off_w[kPolicyMaxLayers], off_b[kPolicyMaxLayers];  // a layer's blocks inside a member's
    double *d_part;                          // [chunks][items of the largest layer][4]: the ES gradient's partial sums
    int32_t chunk_pairs, chunks;             // pairs per chunk and chunks, fixed at create for (P, spec)
    DeviceAllocs allocs;
};

extern "C" {

constexpr int kPopChunkPairs = 16;                  // pairs a lane of the gradient's first launch takes at least
constexpr int kPopMaxChunks = 64;
constexpr size_t kPopPartialBytes = 64u << 20;      // the partial sums stay at most this large (or one chunk)

static void population_free(chub_population *pop) {
    chub_policy *pol = pop->pol;
    (void) hipSetDevice(pol->net.env->device);
    (void) hipDeviceSynchronize();  // (a launch still in flight reads the weights)
    pop->allocs.free_all();
    pol->populations.erase(std::remove(pol->populations.begin(), pol->populations.end(), pop), pol->populations.end());
    delete pop;
}

static void population_args(const chub_population *pop, const PolicyArgs &pa, PolicyPopArgs &out) {
    static_cast<PolicyArgs &>(out) = pa;
    out.tiles_per_member = pop->E / kPolicyEnvTile;
    out.pad_ = 0;
    for (int l = 0; l < kPolicyMaxLayers; l++) {
        out.w_stride[l] = out.b_stride[l] = pop->member_floats;
        if (l < pa.n_layers) {
            out.layer[l].w = pop->d_params + pop->off_w[l];
            out.layer[l].b = pop->d_params + pop->off_b[l];
        }
    }
}

int chub_population_param_count(const chub_config *cfg, const chub_policy_spec *spec, int64_t *n_out) {
    if (!cfg || !spec || !n_out) return fail(CHUB_ERR_ARG, "null argument");
    PolicyShape ps;
    if (const int rc = policy_shape(cfg->station_list, spec, ps)) return rc;
    int64_t n = 0;
    for (int l = 0; l < spec->n_layers; l++) n += (int64_t) spec->width[l] * ((l ? spec->width[l - 1] : ps.F) + 1);
    *n_out = n;
    return CHUB_OK;
}

// one layer of the population as the weight kernels take it
static PopLayerArgs population_layer(const chub_population *pop, int l, uint32_t generation) {
    const MlpNet &net = pop->pol->net;
    PopLayerArgs a;
    a.w = pop->d_params + pop->off_w[l];
    a.bias = pop->d_params + pop->off_b[l];
    a.stride = pop->member_floats;
    a.out = net.out[l];
    a.in = net.in[l];
    a.k_pad = net.k_pad[l];
    a.tiles = net.tiles[l];
    a.layer = l;
    a.pairs = pop->P / 2;
    a.key[0] = pop->key[0];
    a.key[1] = pop->key[1];
    a.generation = generation;
    a.normal_icdf = (const float *) net.env->tb.normal_icdf;
    a.normal_tail = (const float *) net.env->tb.normal_tail;
    return a;
}

int chub_population_create(chub_policy *pol, int32_t P, uint64_t key, chub_population **out) {
    if (!pol || !out) return fail(CHUB_ERR_ARG, "null argument");
    *out = nullptr;
    chub_env *e = pol->net.env;
    const int64_t N = e->hp.n_envs;
    if (P < 2 || (P & 1)) return fail(CHUB_ERR_ARG, "chub_population_create: P is even and at least 2 (members 2j and 2j + 1 are an antithetic pair)");
    if (N % P != 0 || (N / P) % kPolicyEnvTile != 0)
        return fail(CHUB_ERR_ARG, "chub_population_create: the handle's " + std::to_string(N) + " envs are not P = " + std::to_string(P) +
                                      " blocks of a multiple of " + std::to_string(kPolicyEnvTile) + " envs (a workgroup's tile belongs to one member)");
    if (e->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_population_create between chub_graph_begin and chub_graph_end (it allocates and synchronises)");
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    chub_population *pop = new chub_population();
    pop->pol = pol;
    pop->P = P;
    pop->E = (int32_t) (N / P);
    pop->key[0] = (uint32_t) key;  // (split as the policy's key is)
    pop->key[1] = (uint32_t) (key >> 32);
    const MlpNet &net = pol->net;
    int64_t at = 0, items = 0;
    for (int l = 0; l < net.n_layers; l++) {
        pop->off_w[l] = at;
        at += (int64_t) net.tiles[l] * net.k_pad[l] * kPolicyOutTile;
        pop->off_b[l] = at;
        at += (int64_t) net.tiles[l] * kPolicyOutTile;
        items = std::max(items, (int64_t) net.out[l] * (net.in[l] / 4 + 1));
    }
    pop->member_floats = at;
    // the gradient's chunks of pairs: at least kPopChunkPairs pairs each, at most kPopMaxChunks chunks, the partials within kPopPartialBytes
    const int pairs = P / 2;
    const size_t chunk_bytes = (size_t) items * 4 * sizeof(double);
    int64_t chunks = std::min<int64_t>((pairs + kPopChunkPairs - 1) / kPopChunkPairs, kPopMaxChunks);
    chunks = std::max<int64_t>(1, std::min<int64_t>(chunks, (int64_t) (kPopPartialBytes / chunk_bytes)));
    pop->chunk_pairs = (int32_t) ((pairs + chunks - 1) / chunks);
    pop->chunks = (pairs + pop->chunk_pairs - 1) / pop->chunk_pairs;
    pol->populations.push_back(pop);
    const size_t floats = (size_t) P * (size_t) at;
    bool ok = !pop->allocs.zeroed(&pop->d_params, floats) && !pop->allocs.zeroed(&pop->d_stage, floats) &&
              !pop->allocs.zeroed(&pop->d_part, (size_t) pop->chunks * (size_t) items * 4);
    // every member = the centre's current weights: its blocks are the member's layout already
    for (int m = 0; m < P && ok; m++)
        for (int l = 0; l < net.n_layers && ok; l++) {
            float *base = pop->d_params + (int64_t) m * at;
            ok = hipMemcpyAsync(base + pop->off_w[l], net.d_w[l], (size_t) net.tiles[l] * net.k_pad[l] * kPolicyOutTile * sizeof(float),
                                hipMemcpyDeviceToDevice, nullptr) == hipSuccess &&
                 hipMemcpyAsync(base + pop->off_b[l], net.d_b[l], (size_t) net.tiles[l] * kPolicyOutTile * sizeof(float), hipMemcpyDeviceToDevice, nullptr) ==
                     hipSuccess;
        }
    if (!ok || hipDeviceSynchronize() != hipSuccess) {
        population_free(pop);
        (void) hipGetLastError();
        return fail(CHUB_ERR_HIP, "chub_population_create: out of device memory");
    }
    *out = pop;
    return CHUB_OK;
}

int chub_population_destroy(chub_population *pop) {
    if (!pop) return CHUB_OK;
    if (pop->pol->net.env->capturing)
        return fail(CHUB_ERR_UNSUPPORTED, "chub_population_destroy between chub_graph_begin and chub_graph_end (it synchronises and frees)");
    population_free(pop);
    (void) hipGetLastError();
    return CHUB_OK;
}

int chub_population_perturb_device(chub_population *pop, const float *const *d_W, const float *const *d_b, float sigma, uint32_t generation,
                                   void *stream) {
    if (!pop) return fail(CHUB_ERR_ARG, "null argument");
    const chub_policy *pol = pop->pol;
    if ((d_W == nullptr) != (d_b == nullptr)) return fail(CHUB_ERR_ARG, "chub_population_perturb_device: d_W and d_b are both given or both NULL (the centre's weights)");
    if (d_W)
        for (int l = 0; l < pol->spec.n_layers; l++)
            if (!d_W[l] || !d_b[l]) return fail(CHUB_ERR_ARG, "null argument");
    if (!std::isfinite(sigma) || sigma < 0.0f) return fail(CHUB_ERR_ARG, "chub_population_perturb_device: sigma is finite and >= 0");
    HIP_TRY(hipSetDevice(pol->net.env->device));
    (void) hipGetLastError();
    for (int l = 0; l < pol->spec.n_layers; l++) {
        const PopLayerArgs a = population_layer(pop, l, generation);
        if (d_W) launch_population_perturb(a, d_W[l], d_b[l], 0, sigma, (hipStream_t) stream);
        else launch_population_perturb(a, pol->net.d_w[l], pol->net.d_b[l], 1, sigma, (hipStream_t) stream);
    }
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

static int population_check_member(const chub_population *pop, int32_t m, int32_t layer) {
    if (m < 0 || m >= pop->P) return fail(CHUB_ERR_ARG, "m: 0 .. P - 1");
    if (layer < 0 || layer >= pop->pol->spec.n_layers) return fail(CHUB_ERR_ARG, "layer: 0 .. n_layers - 1");
    return CHUB_OK;
}

int chub_population_set_member_device(chub_population *pop, int32_t m, int32_t layer, const float *d_W, const float *d_b, void *stream) {
    if (!pop || !d_W || !d_b) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = population_check_member(pop, m, layer)) return rc;
    HIP_TRY(hipSetDevice(pop->pol->net.env->device));
    (void) hipGetLastError();
    float *base = pop->d_params + (int64_t) m * pop->member_floats;
    net_relayout(pop->pol->net, layer, d_W, d_b, base + pop->off_w[layer], base + pop->off_b[layer], stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_population_get_member_device(chub_population *pop, int32_t m, int32_t layer, float *d_W, float *d_b, void *stream) {
    if (!pop || !d_W || !d_b) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = population_check_member(pop, m, layer)) return rc;
    HIP_TRY(hipSetDevice(pop->pol->net.env->device));
    (void) hipGetLastError();
    const float *base = pop->d_params + (int64_t) m * pop->member_floats;
    net_unlayout(pop->pol->net, layer, base + pop->off_w[layer], base + pop->off_b[layer], d_W, d_b, stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

// the host forms go through the policy's staging buffer (W | b of the largest layer, the trainer's layout), as chub_policy_set_weights does
int chub_population_set_member(chub_population *pop, int32_t m, int32_t layer, const float *W, const float *b) {
    if (!pop || !W || !b) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = population_check_member(pop, m, layer)) return rc;
    MlpNet &net = pop->pol->net;
    if (const int rc = net_begin_host(net, "chub_population_set_member")) return rc;
    if (const int rc = net_stage_in(net, layer, W, b)) return rc;
    if (const int rc = chub_population_set_member_device(pop, m, layer, net.d_stage, net_stage_b(net, layer), nullptr)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return CHUB_OK;
}

int chub_population_get_member(chub_population *pop, int32_t m, int32_t layer, float *W, float *b) {
    if (!pop || !W || !b) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = population_check_member(pop, m, layer)) return rc;
    MlpNet &net = pop->pol->net;
    if (const int rc = net_begin_host(net, "chub_population_get_member")) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (const int rc = chub_population_get_member_device(pop, m, layer, net.d_stage, net_stage_b(net, layer), nullptr)) return rc;
    return net_stage_out(net, layer, W, b);
}

int chub_population_copy_members_device(chub_population *pop, const int32_t *d_src, const int32_t *d_dst, int32_t count, void *stream) {
    if (!pop || !d_src || !d_dst) return fail(CHUB_ERR_ARG, "null argument");
    if (count < 0 || count > pop->P)
        return fail(CHUB_ERR_ARG, "chub_population_copy_members_device: count is 0 .. P (every source is staged before any destination is written)");
    HIP_TRY(hipSetDevice(pop->pol->net.env->device));
    (void) hipGetLastError();
    launch_population_copy(pop->d_params, pop->d_stage, pop->member_floats, pop->P, d_src, d_dst, count, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_population_act_device(chub_env *e, chub_population *pop, const float *d_obs, int64_t ld_obs, const uint8_t *d_mask, float *d_actions,
                               uint64_t *d_pile_bits, float *d_tail, void *stream) {
    if (!e || !pop) return fail(CHUB_ERR_ARG, "null argument");
    if (pop->pol->net.env != e) return fail(CHUB_ERR_ARG, "this population was made for another handle");
    if (const int rc = policy_act_check(e, pop->pol, d_obs, ld_obs, d_actions, d_pile_bits, d_tail)) return rc;
    return policy_act_enqueue(e, pop->pol, pop, d_obs, ld_obs, d_mask, d_actions, d_pile_bits, d_tail, stream);
}

int chub_population_run_steps(chub_env *e, chub_population *pop, int mode, float *const *d_packed2, float *d_reset_obs, float *d_final_obs,
                              int64_t first_step, int64_t n_steps, void *stream) {
    if (!e || !pop) return fail(CHUB_ERR_ARG, "null argument");
    if (pop->pol->net.env != e) return fail(CHUB_ERR_ARG, "this population was made for another handle");
    return policy_run(e, pop->pol, pop, mode, d_packed2, d_reset_obs, d_final_obs, first_step, n_steps, stream);
}

int chub_population_es_gradient_device(chub_population *pop, const float *d_util, uint32_t generation, float *const *d_gW, float *const *d_gb,
                                       void *stream) {
    if (!pop || !d_util || !d_gW || !d_gb) return fail(CHUB_ERR_ARG, "null argument");
    const chub_policy *pol = pop->pol;
    for (int l = 0; l < pol->spec.n_layers; l++)
        if (!d_gW[l] || !d_gb[l]) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(pol->net.env->device));
    (void) hipGetLastError();
    for (int l = 0; l < pol->spec.n_layers; l++)  // (one buffer of partials: the stream orders a layer's merge before the next layer's sums)
        launch_population_es_gradient(population_layer(pop, l, generation), d_util, pop->chunk_pairs, pop->chunks, pop->d_part, d_gW[l], d_gb[l],
                                      (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

// ---- actor gradients on the device (include/chub.h): the plan, the object, the call.  The kernels are chub_policy.hip's
static_assert((int) CHUB_PLOSS_COUNT == PLOSS_COUNT && (int) CHUB_PLOSS_PPO_CLIP == PLOSS_PPO_CLIP, "chub_policy.h restates the CHUB_PLOSS_* enum");
}  // extern "C"

// what a spec comes to for the gradient launches: tiles, LDS rows, the partials' layout and the workgroups of a call of R rows
struct GradPlan {
    int64_t n_params, wrm_floats, wrm_off[kPolicyMaxLayers], param0[kPolicyMaxLayers + 1];
    int32_t in[kPolicyMaxLayers], ot[kPolicyMaxLayers], it[kPolicyMaxLayers], h_row0[kPolicyMaxLayers], pair0[kPolicyMaxLayers], bias0[kPolicyMaxLayers];
    int32_t x_rows, d_row0[2], s_row0, lds_rows, n_pairs, bias_floats, part_floats, in_registers;
};

static int grad_blocks(const GradPlan &gp, int64_t R) {
    const int64_t tiles = (R + 31) / 32;
    int64_t nb = std::min<int64_t>((tiles + 7) & ~(int64_t) 7, kGradMaxBlocks);
    const int64_t by_bytes = std::max<int64_t>(8, (int64_t) (kGradPartialBytes / ((size_t) gp.part_floats * sizeof(float))) & ~(int64_t) 7);
    return (int) std::min(nb, by_bytes);
}

// (stats: the f64 a workgroup leaves beside its f32 partials, kGradPart64 or kCriticStats)
static size_t grad_workspace(const GradPlan &gp, int blocks, int stats) {
    return (size_t) gp.wrm_floats * sizeof(float) + (size_t) blocks * ((size_t) gp.part_floats * sizeof(float) + (size_t) stats * sizeof(double));
}

static int grad_plan(int nl, const int32_t *width, int F, GradPlan &gp) {
    memset(&gp, 0, sizeof gp);
    int rows = (F + 31) / 32 * 32, dmax = 0;
    gp.x_rows = rows;
    for (int l = 0; l < nl; l++) {
        gp.in[l] = l ? width[l - 1] : F;
        gp.ot[l] = (width[l] + 31) / 32;
        gp.it[l] = (gp.in[l] + 31) / 32;
        gp.pair0[l] = gp.n_pairs;
        gp.n_pairs += gp.ot[l] * gp.it[l];
        gp.bias0[l] = gp.bias_floats;
        gp.bias_floats += gp.ot[l] * 32;
        gp.param0[l] = gp.n_params;
        gp.n_params += (int64_t) width[l] * (gp.in[l] + 1);
        if (l) {
            gp.wrm_off[l] = gp.wrm_floats;
            gp.wrm_floats += (int64_t) gp.ot[l] * 32 * gp.it[l] * 32;
        }
        if (l + 1 < nl) {
            gp.h_row0[l] = rows;
            rows += gp.ot[l] * 32;
        }
        dmax = std::max(dmax, gp.ot[l] * 32);
    }
    gp.param0[nl] = gp.n_params;
    gp.d_row0[0] = rows;
    gp.d_row0[1] = rows + dmax;
    gp.s_row0 = rows + 2 * dmax;
    gp.lds_rows = gp.s_row0 + kGradScratchRows;
    gp.part_floats = gp.n_pairs * 1024 + gp.bias_floats;
    gp.in_registers = gp.n_pairs <= kGradRegSlots * kGradWaves ? 1 : 0;
    if ((int64_t) gp.lds_rows * kGradRowStride * (int64_t) sizeof(float) > kGradLdsBytes)
        return fail(CHUB_ERR_UNSUPPORTED, "the gradient launch keeps the feature rows, every hidden layer and two delta images in LDS: " +
                                              std::to_string(gp.lds_rows) + " rows of " + std::to_string(kGradRowStride) + " floats, at most " +
                                              std::to_string(kGradLdsBytes / (kGradRowStride * (int) sizeof(float))) + " (160 KiB); the policy still acts and samples");
    return CHUB_OK;
}

// the *_plan_out block of chub_policy_grad_plan and chub_critic_plan
template <class PlanOut>
static void grad_plan_out(const GradPlan &gp, int64_t R, int stats, PlanOut *out) {
    out->n_params = gp.n_params;
    out->workgroups = grad_blocks(gp, R);
    out->lds_rows = gp.lds_rows;
    out->lds_bytes = gp.lds_rows * kGradRowStride * (int32_t) sizeof(float);
    out->in_registers = gp.in_registers;
    out->workspace_bytes = (int64_t) grad_workspace(gp, out->workgroups, stats);
}

// what the gradient launches of one net keep between calls: the plan, the row-major copies of layers 1.., the workgroups' f32 and f64 partials
struct GradWorkspace {
    GradPlan gp;
    int32_t max_blocks;
    float *d_wrm, *d_part;
    double *d_part64;
    DeviceAllocs allocs;
};

// nullptr, or what failed (DeviceAllocs::zeroed); the owner frees ws.allocs
static const char *grad_workspace_create(GradWorkspace &ws, const GradPlan &gp, int64_t max_rows, int stats) {
    ws.gp = gp;
    ws.max_blocks = grad_blocks(gp, max_rows);
    if (const char *what = ws.allocs.zeroed(&ws.d_wrm, (size_t) gp.wrm_floats)) return what;
    if (const char *what = ws.allocs.zeroed(&ws.d_part, (size_t) ws.max_blocks * (size_t) gp.part_floats)) return what;
    return ws.allocs.zeroed(&ws.d_part64, (size_t) ws.max_blocks * (size_t) stats);
}

// what a gradient call asks of its rows; ld_text names the stride and the row in the caller's words
static int grad_check_rows(const char *who, int64_t max_rows, int64_t R, int64_t n_rows, const int64_t *d_rows, int64_t ld, int F, const char *ld_text) {
    if (R <= 0 || R > max_rows) return fail(CHUB_ERR_ARG, std::string(who) + ": R is 1 .. max_rows = " + std::to_string(max_rows));
    if (n_rows < 1) return fail(CHUB_ERR_ARG, std::string(who) + ": n_rows, the rows the arrays hold, is at least 1");
    if (!d_rows && R > n_rows) return fail(CHUB_ERR_ARG, std::string(who) + ": without d_rows the call reads rows 0 .. R - 1: R <= n_rows");
    if (ld < F) return fail(CHUB_ERR_ARG, std::string(ld_text) + std::to_string(F) + " floats");
    return CHUB_OK;
}

static void grad_layers(const MlpNet &n, const GradWorkspace &ws, GradLayer *layer) {
    const GradPlan &gp = ws.gp;
    for (int l = 0; l < n.n_layers; l++) {
        GradLayer &L = layer[l];
        L.w = n.d_w[l];
        L.b = n.d_b[l];
        L.wrm = l ? ws.d_wrm + gp.wrm_off[l] : nullptr;
        L.k_pad = n.k_pad[l];
        L.in = gp.in[l];
        L.out = n.out[l];
        L.ot = gp.ot[l];
        L.it = gp.it[l];
        L.h_row0 = gp.h_row0[l];
        L.pair0 = gp.pair0[l];
        L.bias0 = gp.bias0[l];
    }
}

// what PolicyGradArgs and CriticArgs share: the layers, the partials and the plan's numbers (a is zeroed first)
template <class Args>
static void grad_args(const MlpNet &n, const GradWorkspace &ws, Args &a) {
    const GradPlan &gp = ws.gp;
    memset(&a, 0, sizeof a);
    grad_layers(n, ws, a.layer);
    a.part = ws.d_part;
    a.part64 = ws.d_part64;
    a.n_layers = n.n_layers;
    a.F = n.F;
    a.x_rows = gp.x_rows;
    a.d_row0[0] = gp.d_row0[0];
    a.d_row0[1] = gp.d_row0[1];
    a.s_row0 = gp.s_row0;
    a.n_pairs = gp.n_pairs;
    a.part_floats = gp.part_floats;
    a.bias_floats = gp.bias_floats;
}

// what GradMergeArgs and CriticMergeArgs share (m is zeroed first); backward: some layer's gradient is asked for
template <class Merge, class Out>
static void grad_merge_args(const MlpNet &n, const GradWorkspace &ws, int64_t R, const Out *out, Merge &m) {
    const GradPlan &gp = ws.gp;
    memset(&m, 0, sizeof m);
    for (int l = 0; l < n.n_layers; l++) {
        m.gW[l] = out->d_gW[l];
        m.gb[l] = out->d_gb[l];
        m.in[l] = gp.in[l];
        m.it[l] = gp.it[l];
        m.pair0[l] = gp.pair0[l];
        m.bias0[l] = gp.bias0[l];
        m.param0[l] = gp.param0[l];
        m.backward |= out->d_gW[l] != nullptr || out->d_gb[l] != nullptr;
    }
    m.param0[n.n_layers] = gp.param0[n.n_layers];
    m.part = ws.d_part;
    m.part64 = ws.d_part64;
    m.stats = out->d_stats;
    m.R = R;
    m.n_layers = n.n_layers;
    m.blocks = grad_blocks(gp, R);
    m.part_floats = gp.part_floats;
    m.bias_base = gp.n_pairs * 1024;
}

struct chub_policy_grad {
    chub_policy *pol;
    int64_t max_rows;
    GradWorkspace ws;
};

extern "C" {

static void policy_grad_free(chub_policy_grad *g) {
    chub_policy *pol = g->pol;
    (void) hipSetDevice(pol->net.env->device);
    (void) hipDeviceSynchronize();  // (a launch still in flight reads the copies and writes the partials)
    g->ws.allocs.free_all();
    pol->grads.erase(std::remove(pol->grads.begin(), pol->grads.end(), g), pol->grads.end());
    delete g;
}

int chub_policy_grad_plan(const chub_config *cfg, const chub_policy_spec *spec, int64_t R, chub_policy_grad_plan_out *out) {
    if (!cfg || !spec || !out) return fail(CHUB_ERR_ARG, "null argument");
    if (R < 1) return fail(CHUB_ERR_ARG, "chub_policy_grad_plan: R is at least 1");
    PolicyShape ps;
    if (const int rc = policy_shape(cfg->station_list, spec, ps)) return rc;
    GradPlan gp;
    if (const int rc = grad_plan(spec->n_layers, spec->width, ps.F, gp)) return rc;
    grad_plan_out(gp, R, kGradPart64, out);
    return CHUB_OK;
}

int chub_policy_grad_create(chub_policy *pol, int64_t max_rows, chub_policy_grad **out) {
    if (!pol || !out) return fail(CHUB_ERR_ARG, "null argument");
    *out = nullptr;
    if (max_rows < 1) return fail(CHUB_ERR_ARG, "chub_policy_grad_create: max_rows is at least 1");
    chub_env *e = pol->net.env;
    if (!pol->explore) return fail(CHUB_ERR_ARG, "chub_policy_grad_create: chub_policy_set_exploration first (the log-probability needs log_std)");
    PolicyShape ps;
    if (const int rc = policy_shape(e->hp.S, &pol->spec, ps)) return rc;
    GradPlan gp;
    if (const int rc = grad_plan(pol->spec.n_layers, pol->spec.width, ps.F, gp)) return rc;
    if (e->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_policy_grad_create between chub_graph_begin and chub_graph_end (it allocates and synchronises)");
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    if (policy_grad_prepare() != 0) {
        (void) hipGetLastError();
        return fail(CHUB_ERR_HIP, "chub_policy_grad_create: the gradient kernel's LDS limit could not be raised");
    }
    chub_policy_grad *g = new chub_policy_grad();
    g->pol = pol;
    g->max_rows = max_rows;
    pol->grads.push_back(g);
    if (grad_workspace_create(g->ws, gp, max_rows, kGradPart64) || hipDeviceSynchronize() != hipSuccess) {
        policy_grad_free(g);
        (void) hipGetLastError();
        return fail(CHUB_ERR_HIP, "chub_policy_grad_create: out of device memory");
    }
    *out = g;
    return CHUB_OK;
}

int chub_policy_grad_destroy(chub_policy_grad *g) {
    if (!g) return CHUB_OK;
    if (g->pol->net.env->capturing)
        return fail(CHUB_ERR_UNSUPPORTED, "chub_policy_grad_destroy between chub_graph_begin and chub_graph_end (it synchronises and frees)");
    policy_grad_free(g);
    (void) hipGetLastError();
    return CHUB_OK;
}

// what chub_policy_grad_device refuses of its input (chub_ppo_update asks the same before it enqueues anything)
static int policy_grad_check(const chub_policy_grad *g, const chub_policy_grad_in *in) {
    const chub_policy *pol = g->pol;
    const bool piles = pol->spec.head == CHUB_PHEAD_PILES;
    if (!in->d_features || !in->d_u || !in->d_adv || (piles && !in->d_pile_bits)) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = grad_check_rows("chub_policy_grad_device", g->max_rows, in->R, in->n_rows, in->d_rows, in->ld_features, pol->net.F,
                                       "ld_features: at least the feature row's "))
        return rc;
    if (in->loss != CHUB_PLOSS_COEF && in->loss != CHUB_PLOSS_PPO_CLIP) return fail(CHUB_ERR_ARG, "loss: CHUB_PLOSS_COEF or CHUB_PLOSS_PPO_CLIP");
    if (in->loss == CHUB_PLOSS_PPO_CLIP) {
        if (!(in->clip_eps > 0.0f && in->clip_eps < 1.0f)) return fail(CHUB_ERR_ARG, "clip_eps: inside (0, 1) under CHUB_PLOSS_PPO_CLIP");
        if (!in->d_logp_old) return fail(CHUB_ERR_ARG, "null argument");
    }
    if (!std::isfinite(in->ent_coef)) return fail(CHUB_ERR_ARG, "ent_coef is not finite");
    if (!piles && in->d_set_bits) return fail(CHUB_ERR_ARG, "chub_policy_grad_device: under CHUB_PHEAD_LOADS the log-probability has no pile terms: d_set_bits must be NULL");
    if (!pol->explore) return fail(CHUB_ERR_ARG, "chub_policy_grad_device: chub_policy_set_exploration first (the log-probability needs log_std)");
    return CHUB_OK;
}

int chub_policy_grad_device(chub_policy_grad *g, const chub_policy_grad_in *in, const chub_policy_grad_out *out, void *stream) {
    if (!g || !in || !out) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = policy_grad_check(g, in)) return rc;
    const chub_policy *pol = g->pol;
    HIP_TRY(hipSetDevice(pol->net.env->device));
    (void) hipGetLastError();
    const GradPlan &gp = g->ws.gp;
    PolicyGradArgs a;
    grad_args(pol->net, g->ws, a);
    GradMergeArgs m;
    grad_merge_args(pol->net, g->ws, in->R, out, m);
    for (int l = 0; l < pol->net.n_layers; l++) m.out[l] = pol->net.out[l];
    m.glog_std = out->d_glog_std;
    m.G = pol->G;
    m.backward |= out->d_glog_std != nullptr;
    a.R = in->R;
    a.rows_total = in->n_rows;
    a.rows = in->d_rows;
    a.features = in->d_features;
    a.ld = in->ld_features;
    a.pile_bits = (const uint32_t *) in->d_pile_bits;
    a.set_bits = (const uint32_t *) in->d_set_bits;
    a.u = in->d_u;
    a.logp_old = in->d_logp_old;
    a.adv = in->d_adv;
    a.adv_stats = in->d_adv_stats;
    a.mean = pol->pa.mean;
    a.inv_std = pol->pa.inv_std;
    a.log_std = pol->d_log_std;
    a.logp_new = out->d_logp_new;
    a.entropy = out->d_entropy;
    a.clip = pol->spec.clip;
    a.clip_eps = in->clip_eps;
    a.ent_coef = in->ent_coef;
    a.hidden_act = pol->spec.hidden_act;
    a.normalize = pol->spec.normalize;
    a.head = pol->spec.head;
    a.S = pol->pa.S;
    a.A = pol->A_out;
    a.W = pol->pa.W;
    a.G = pol->G;
    a.loss = in->loss;
    a.backward = m.backward;
    launch_policy_grad(a, m, m.blocks, gp.lds_rows, gp.in_registers != 0, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

// ---- a critic on the device (include/chub.h): the plan, the object, the calls.  The kernels are chub_critic.hip's; the weight layout, the
// re-layout launch, the fit rule and the workgroup rule are the actor's and its gradient's (GradPlan above, the head one tile of 32)
static_assert((int) CHUB_VLOSS_COUNT == VLOSS_COUNT && (int) CHUB_VLOSS_CLIPPED == VLOSS_CLIPPED, "chub_critic.h restates the CHUB_VLOSS_* enum");
}  // extern "C"

constexpr int kCriticMaxF = 512;  // the limit of chub_moments

struct chub_critic {
    MlpNet net;
    chub_critic_spec spec;
    int64_t max_rows;
    GradWorkspace ws;
};

static int critic_check_spec(const chub_critic_spec *sp) {
    if (sp->F < 1 || sp->F > kCriticMaxF) return fail(CHUB_ERR_ARG, "F: 1 .. " + std::to_string(kCriticMaxF) + " floats per row");
    if (sp->n_layers < 1 || sp->n_layers > kPolicyMaxLayers) return fail(CHUB_ERR_ARG, "n_layers: 1 .. 4");
    for (int l = 0; l + 1 < sp->n_layers; l++)
        if (sp->width[l] < 1 || sp->width[l] > kPolicyMaxHidden) return fail(CHUB_ERR_ARG, "width[" + std::to_string(l) + "]: hidden widths are 1 .. 256");
    if (sp->width[sp->n_layers - 1] != 1) return fail(CHUB_ERR_ARG, "width[n_layers - 1] must be 1: the critic's head is one linear output");
    if (sp->hidden_act < 0 || sp->hidden_act >= CHUB_PACT_COUNT) return fail(CHUB_ERR_ARG, "hidden_act: CHUB_PACT_TANH or CHUB_PACT_RELU");
    if (sp->normalize != 0 && sp->normalize != 1) return fail(CHUB_ERR_ARG, "normalize: 0 or 1");
    if (sp->normalize && !(sp->clip > 0.0f)) return fail(CHUB_ERR_ARG, "clip must be > 0 with normalize");
    return CHUB_OK;
}

// the gradient's plan for the critic's layers
static int critic_plan(const chub_critic_spec *sp, GradPlan &gp) {
    if (const int rc = critic_check_spec(sp)) return rc;
    if (grad_plan(sp->n_layers, sp->width, sp->F, gp) != CHUB_OK)  // (its only refusal is the fit rule; said here in the critic's words)
        return fail(CHUB_ERR_UNSUPPORTED, "the critic keeps its rows, every hidden layer and two delta images in LDS: " + std::to_string(gp.lds_rows) +
                                              " rows of " + std::to_string(kGradRowStride) + " floats, at most " +
                                              std::to_string(kGradLdsBytes / (kGradRowStride * (int) sizeof(float))) + " (160 KiB)");
    return CHUB_OK;
}

extern "C" {

static void critic_free(chub_critic *c) {
    chub_env *e = c->net.env;
    net_free(c->net);  // (its synchronise also covers the partials a launch in flight writes)
    c->ws.allocs.free_all();
    e->critics.erase(std::remove(e->critics.begin(), e->critics.end(), c), e->critics.end());
    delete c;
}

int chub_critic_plan(const chub_critic_spec *spec, int64_t R, chub_critic_plan_out *out) {
    if (!spec || !out) return fail(CHUB_ERR_ARG, "null argument");
    if (R < 1) return fail(CHUB_ERR_ARG, "chub_critic_plan: R is at least 1");
    GradPlan gp;
    if (const int rc = critic_plan(spec, gp)) return rc;
    grad_plan_out(gp, R, kCriticStats, out);
    return CHUB_OK;
}

int chub_critic_create(chub_env *e, const chub_critic_spec *spec, const float *const *W, const float *const *b, const float *mean,
                       const float *inv_std, int64_t max_rows, chub_critic **out) {
    if (!e || !spec || !W || !b || !out) return fail(CHUB_ERR_ARG, "null argument");
    *out = nullptr;
    GradPlan gp;
    if (const int rc = critic_plan(spec, gp)) return rc;
    for (int l = 0; l < spec->n_layers; l++)
        if (!W[l] || !b[l]) return fail(CHUB_ERR_ARG, "null argument");
    if (spec->normalize && (!mean || !inv_std)) return fail(CHUB_ERR_ARG, "normalize needs mean and inv_std");
    if (max_rows < 1) return fail(CHUB_ERR_ARG, "chub_critic_create: max_rows is at least 1");
    if (e->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_critic_create between chub_graph_begin and chub_graph_end (it allocates and synchronises)");
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    if (critic_prepare() != 0) {
        (void) hipGetLastError();
        return fail(CHUB_ERR_HIP, "chub_critic_create: the critic kernel's LDS limit could not be raised");
    }
    chub_critic *c = new chub_critic();
    MlpNet &net = c->net;
    net.env = e;
    net.noun = "critic";
    net.row_noun = "rows";
    net.alloc_who = "chub_critic_create";
    net.n_layers = spec->n_layers;
    net.F = spec->F;
    net.normalize = spec->normalize != 0;
    for (int l = 0; l < spec->n_layers; l++) {
        net.in[l] = gp.in[l];
        net.out[l] = spec->width[l];
        net.tiles[l] = gp.ot[l];
    }
    c->spec = *spec;
    c->max_rows = max_rows;
    e->critics.push_back(c);
    int rc = net_alloc_layers(net);
    if (!rc)
        if (const char *what = grad_workspace_create(c->ws, gp, max_rows, kCriticStats)) rc = fail(CHUB_ERR_HIP, std::string(net.alloc_who) + ": " + what);
    if (!rc) rc = net_load(net, "chub_critic_create", W, b, mean, inv_std);
    if (rc) {
        const std::string msg = g_err;
        critic_free(c);
        (void) hipGetLastError();
        return fail(rc, msg);
    }
    *out = c;
    return CHUB_OK;
}

int chub_critic_destroy(chub_critic *c) {
    if (!c) return CHUB_OK;
    if (c->net.env->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_critic_destroy between chub_graph_begin and chub_graph_end (it synchronises and frees)");
    critic_free(c);
    (void) hipGetLastError();
    return CHUB_OK;
}

int chub_critic_set_weights(chub_critic *c, int32_t layer, const float *W, const float *b) {
    if (!c || !W || !b) return fail(CHUB_ERR_ARG, "null argument");
    return net_set_weights(c->net, "chub_critic_set_weights", layer, W, b);
}

int chub_critic_set_weights_device(chub_critic *c, int32_t layer, const float *d_W, const float *d_b, void *stream) {
    if (!c || !d_W || !d_b) return fail(CHUB_ERR_ARG, "null argument");
    return net_set_weights_device(c->net, layer, d_W, d_b, stream);
}

int chub_critic_get_weights(chub_critic *c, int32_t layer, float *W, float *b) {
    if (!c || !W || !b) return fail(CHUB_ERR_ARG, "null argument");
    return net_get_weights(c->net, "chub_critic_get_weights", layer, W, b);
}

int chub_critic_get_weights_device(chub_critic *c, int32_t layer, float *d_W, float *d_b, void *stream) {
    if (!c || !d_W || !d_b) return fail(CHUB_ERR_ARG, "null argument");
    return net_get_weights_device(c->net, layer, d_W, d_b, stream);
}

int chub_critic_set_normalizer(chub_critic *c, const float *mean, const float *inv_std) {
    if (!c || !mean || !inv_std) return fail(CHUB_ERR_ARG, "null argument");
    return net_set_normalizer(c->net, "chub_critic_set_normalizer", mean, inv_std);
}

int chub_critic_set_normalizer_device(chub_critic *c, const float *d_mean, const float *d_inv_std, void *stream) {
    if (!c || !d_mean || !d_inv_std) return fail(CHUB_ERR_ARG, "null argument");
    return net_set_normalizer_device(c->net, "chub_critic_set_normalizer_device", d_mean, d_inv_std, stream);
}

int chub_critic_normalizer_from_moments_device(chub_critic *c, chub_moments *m, double eps, void *stream) {
    if (!c || !m) return fail(CHUB_ERR_ARG, "null argument");
    return net_normalizer_from_moments(c->net, "chub_critic_normalizer_from_moments_device", m, eps, stream);
}

// what every critic call asks of its rows
static int critic_check_rows(const chub_critic *c, const char *who, const float *d_x, int64_t ld, int64_t n_rows, const int64_t *d_rows, int64_t R) {
    if (!d_x) return fail(CHUB_ERR_ARG, "null argument");
    return grad_check_rows(who, c->max_rows, R, n_rows, d_rows, ld, c->spec.F, "ld: at least the row's ");
}

static void critic_args(const chub_critic *c, CriticArgs &a) {
    grad_args(c->net, c->ws, a);
    a.mean = c->net.d_norm;
    a.inv_std = c->net.d_norm + c->spec.F;
    a.clip = c->spec.clip;
    a.hidden_act = c->spec.hidden_act;
    a.normalize = c->spec.normalize;
}

int chub_critic_values_device(chub_critic *c, const float *d_x, int64_t ld, int64_t n_rows, const int64_t *d_rows, int64_t R, float *d_values,
                              void *stream) {
    if (!c || !d_values) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = critic_check_rows(c, "chub_critic_values_device", d_x, ld, n_rows, d_rows, R)) return rc;
    HIP_TRY(hipSetDevice(c->net.env->device));
    (void) hipGetLastError();
    CriticArgs a;
    critic_args(c, a);
    a.R = R;
    a.rows_total = n_rows;
    a.rows = d_rows;
    a.x = d_x;
    a.ld = ld;
    a.values = d_values;
    // (no partials to merge: as many workgroups as the tiles give, up to what 256 CUs hold of the 13-64-64-1 form, four each)
    const int64_t tiles = (R + 31) / 32;
    launch_critic_values(a, (int) std::min<int64_t>((tiles + 7) & ~(int64_t) 7, kCriticValueBlocks), c->ws.gp.lds_rows, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

// what chub_critic_grad_device refuses of its input (chub_ppo_update asks the same before it enqueues anything)
static int critic_grad_check(const chub_critic *c, const chub_critic_grad_in *in) {
    if (const int rc = critic_check_rows(c, "chub_critic_grad_device", in->d_x, in->ld, in->n_rows, in->d_rows, in->R)) return rc;
    if (!in->d_ret) return fail(CHUB_ERR_ARG, "null argument");
    if (in->loss != CHUB_VLOSS_MSE && in->loss != CHUB_VLOSS_CLIPPED) return fail(CHUB_ERR_ARG, "loss: CHUB_VLOSS_MSE or CHUB_VLOSS_CLIPPED");
    if (in->loss == CHUB_VLOSS_CLIPPED) {
        if (!(in->clip_eps > 0.0f) || !std::isfinite(in->clip_eps)) return fail(CHUB_ERR_ARG, "clip_eps: finite and > 0 under CHUB_VLOSS_CLIPPED");
        if (!in->d_v_old) return fail(CHUB_ERR_ARG, "null argument");
    }
    return CHUB_OK;
}

int chub_critic_grad_device(chub_critic *c, const chub_critic_grad_in *in, const chub_critic_grad_out *out, void *stream) {
    if (!c || !in || !out) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = critic_grad_check(c, in)) return rc;
    HIP_TRY(hipSetDevice(c->net.env->device));
    (void) hipGetLastError();
    const GradPlan &gp = c->ws.gp;
    CriticArgs a;
    critic_args(c, a);
    CriticMergeArgs m;
    grad_merge_args(c->net, c->ws, in->R, out, m);
    a.R = in->R;
    a.rows_total = in->n_rows;
    a.rows = in->d_rows;
    a.x = in->d_x;
    a.ld = in->ld;
    a.ret = in->d_ret;
    a.v_old = in->d_v_old;
    a.values = out->d_values;
    a.clip_eps = in->clip_eps;
    a.loss = in->loss;
    a.stats = 1;
    a.backward = m.backward;
    launch_critic_grad(a, m, m.blocks, gp.lds_rows, gp.in_registers != 0, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

// ---- reading log_std back (include/chub.h)
int chub_policy_get_log_std_device(chub_policy *pol, float *d_log_std, void *stream) {
    if (!pol || !d_log_std) return fail(CHUB_ERR_ARG, "null argument");
    if (!pol->explore) return fail(CHUB_ERR_ARG, "chub_policy_set_exploration first (it makes the policy's log_std buffer)");
    HIP_TRY(hipSetDevice(pol->net.env->device));
    (void) hipGetLastError();
    HIP_TRY(hipMemcpyAsync(d_log_std, pol->d_log_std, (size_t) pol->G * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t) stream));
    return CHUB_OK;
}

int chub_policy_get_log_std(chub_policy *pol, float *log_std) {
    if (!pol || !log_std) return fail(CHUB_ERR_ARG, "null argument");
    if (!pol->explore) return fail(CHUB_ERR_ARG, "chub_policy_set_exploration first (it makes the policy's log_std buffer)");
    if (pol->net.env->capturing)
        return fail(CHUB_ERR_UNSUPPORTED, "chub_policy_get_log_std between chub_graph_begin and chub_graph_end (it copies and synchronises: use "
                                          "chub_policy_get_log_std_device)");
    HIP_TRY(hipSetDevice(pol->net.env->device));
    (void) hipGetLastError();
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(log_std, pol->d_log_std, (size_t) pol->G * sizeof(float), hipMemcpyDeviceToHost));
    return CHUB_OK;
}

}  // extern "C"

// ---- an optimiser on the device (include/chub.h): the plan, the object, the calls.  The kernels are chub_adam.hip's; the parameters are
// the target's live weights, so the object owns the moments, the scalars, a gradient buffer and the chunks' partials, and nothing else
struct AdamPlan {
    int64_t n, param0[kPolicyMaxLayers + 1];
    int32_t chunks, blocks;
};

static void adam_plan(const int32_t *out_dims, const int32_t *in_dims, int n_layers, int G, AdamPlan &ap) {
    int64_t n = 0;
    for (int l = 0; l < n_layers; l++) {
        ap.param0[l] = n;
        n += (int64_t) out_dims[l] * ((int64_t) in_dims[l] + 1);
    }
    ap.param0[n_layers] = n;
    ap.n = n + G;
    ap.chunks = (int32_t) ((ap.n + kAdamChunk - 1) / kAdamChunk);
    ap.blocks = ap.chunks < kAdamMaxBlocks ? ap.chunks : kAdamMaxBlocks;
}

constexpr size_t kAdamBlobHeader = 32;  // int64 t, double p1, double p2, int64 n

struct chub_adam {
    MlpNet *net;        // the target's: a policy's or a critic's
    AdamPlan ap;
    AdamArgs args;      // everything but the gradient pointers and the stats
    int32_t n_layers, G;
    float *d_m, *d_v, *d_g;
    double *d_scalars, *d_partials;
    double *d_own_stats;  // chub_ppo_update without a log: the target's gradient stats [6], then the step's [4]
    DeviceAllocs allocs;
};

static void adam_free(chub_adam *a) {
    (void) hipSetDevice(a->net->env->device);
    (void) hipDeviceSynchronize();  // (a launch still in flight reads and writes all of these)
    a->allocs.free_all();
    std::vector<chub_adam *> &list = a->net->adams;
    list.erase(std::remove(list.begin(), list.end(), a), list.end());
    delete a;
}

static int adam_check_hyper(const chub_adam_hyper *h) {
    const double nonneg[4] = {h->lr, h->eps, h->weight_decay, h->max_grad_norm};
    static const char *const names[4] = {"lr", "eps", "weight_decay", "max_grad_norm"};
    for (int i = 0; i < 4; i++)
        if (!(nonneg[i] >= 0.0) || !std::isfinite(nonneg[i])) return fail(CHUB_ERR_ARG, std::string(names[i]) + ": finite and >= 0");
    if (!(h->beta1 >= 0.0 && h->beta1 < 1.0) || !(h->beta2 >= 0.0 && h->beta2 < 1.0)) return fail(CHUB_ERR_ARG, "beta1, beta2: in [0, 1)");
    return CHUB_OK;
}

extern "C" {

int chub_adam_plan(const int32_t *out_dims, const int32_t *in_dims, int32_t n_layers, int32_t G, chub_adam_plan_out *out) {
    if (!out_dims || !in_dims || !out) return fail(CHUB_ERR_ARG, "null argument");
    if (n_layers < 1 || n_layers > kPolicyMaxLayers) return fail(CHUB_ERR_ARG, "n_layers: 1 .. 4");
    if (G < 0 || G > 4) return fail(CHUB_ERR_ARG, "G: 0 (no log_std) .. 4");
    for (int l = 0; l < n_layers; l++)
        if (out_dims[l] < 1 || in_dims[l] < 1 || out_dims[l] > 65536 || in_dims[l] > 65536) return fail(CHUB_ERR_ARG, "out_dims, in_dims: 1 .. 65536 each");
    AdamPlan ap;
    adam_plan(out_dims, in_dims, n_layers, G, ap);
    out->n = ap.n;
    out->state_bytes = (int64_t) kAdamBlobHeader + 8 * ap.n;
    out->workspace_bytes = 12 * ap.n + 8 * (int64_t) ap.chunks + 8 * (int64_t) ADAM_SCALARS;  // m, v, the gradient buffer; the partials; the scalars
    out->norm_workgroups = ap.blocks;
    out->step_workgroups = ap.blocks;
    return CHUB_OK;
}

// the object for a net's live layers and, with G > 0, the policy's log_std [G]
static int adam_create_for(MlpNet &net, const char *who, int G, float *d_log_std, const chub_adam_hyper *h, chub_adam **out) {
    if (const int rc = adam_check_hyper(h)) return rc;
    if (net.env->capturing)
        return fail(CHUB_ERR_UNSUPPORTED, std::string(who) + " between chub_graph_begin and chub_graph_end (it allocates and synchronises)");
    HIP_TRY(hipSetDevice(net.env->device));
    (void) hipGetLastError();
    chub_adam *a = new chub_adam();
    a->net = &net;
    a->n_layers = net.n_layers;
    a->G = G;
    AdamArgs &g = a->args;
    for (int l = 0; l < net.n_layers; l++) {
        g.w[l] = net.d_w[l];
        g.b[l] = net.d_b[l];
        g.in[l] = net.in[l];
        g.out[l] = net.out[l];
        g.k_pad[l] = net.k_pad[l];
    }
    g.log_std = d_log_std;
    adam_plan(g.out, g.in, a->n_layers, a->G, a->ap);
    const AdamPlan &ap = a->ap;
    for (int l = 0; l <= a->n_layers; l++) g.param0[l] = ap.param0[l];
    g.n = ap.n;
    g.n_layers = a->n_layers;
    g.chunks = ap.chunks;
    net.adams.push_back(a);
    const size_t n = (size_t) ap.n;
    double sc[ADAM_SCALARS] = {h->lr, h->beta1, h->beta2, h->eps, h->weight_decay, h->max_grad_norm, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0};  // (t = 0 is all zero bits)
    const bool ok = !a->allocs.zeroed(&a->d_m, n) && !a->allocs.zeroed(&a->d_v, n) && !a->allocs.zeroed(&a->d_g, n) &&
                    !a->allocs.zeroed(&a->d_scalars, (size_t) ADAM_SCALARS) && !a->allocs.zeroed(&a->d_partials, (size_t) ap.chunks) &&
                    !a->allocs.zeroed(&a->d_own_stats, (size_t) (kTrainLogGradStats + kTrainLogStepStats)) &&
                    hipMemcpy(a->d_scalars, sc, sizeof sc, hipMemcpyHostToDevice) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        adam_free(a);
        (void) hipGetLastError();
        return fail(CHUB_ERR_HIP, "chub_adam_create: out of device memory");
    }
    g.m = a->d_m;
    g.v = a->d_v;
    g.scalars = a->d_scalars;
    g.partials = a->d_partials;
    *out = a;
    return CHUB_OK;
}

int chub_adam_create_policy(chub_policy *pol, const chub_adam_hyper *h, chub_adam **out) {
    if (!pol || !h || !out) return fail(CHUB_ERR_ARG, "null argument");
    *out = nullptr;
    return adam_create_for(pol->net, "chub_adam_create_policy", pol->explore ? pol->G : 0, pol->explore ? pol->d_log_std : nullptr, h, out);
}

int chub_adam_create_critic(chub_critic *c, const chub_adam_hyper *h, chub_adam **out) {
    if (!c || !h || !out) return fail(CHUB_ERR_ARG, "null argument");
    *out = nullptr;
    return adam_create_for(c->net, "chub_adam_create_critic", 0, nullptr, h, out);
}

int chub_adam_destroy(chub_adam *a) {
    if (!a) return CHUB_OK;
    if (a->net->env->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_adam_destroy between chub_graph_begin and chub_graph_end (it synchronises and frees)");
    adam_free(a);
    (void) hipGetLastError();
    return CHUB_OK;
}

int chub_adam_set_hyper(chub_adam *a, const chub_adam_hyper *h) {
    if (!a || !h) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = adam_check_hyper(h)) return rc;
    if (a->net->env->capturing)
        return fail(CHUB_ERR_UNSUPPORTED, "chub_adam_set_hyper between chub_graph_begin and chub_graph_end (it copies and synchronises: use chub_adam_set_lr_device)");
    HIP_TRY(hipSetDevice(a->net->env->device));
    (void) hipGetLastError();
    HIP_TRY(hipDeviceSynchronize());
    const double sc[6] = {h->lr, h->beta1, h->beta2, h->eps, h->weight_decay, h->max_grad_norm};
    HIP_TRY(hipMemcpy(a->d_scalars, sc, sizeof sc, hipMemcpyHostToDevice));
    return CHUB_OK;
}

int chub_adam_set_lr_device(chub_adam *a, const double *d_lr, void *stream) {
    if (!a || !d_lr) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(a->net->env->device));
    (void) hipGetLastError();
    HIP_TRY(hipMemcpyAsync(a->d_scalars + ADAM_LR, d_lr, sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t) stream));
    return CHUB_OK;
}

int chub_adam_grads(chub_adam *a, float **d_gW, float **d_gb, float **d_glog_std) {
    if (!a || !d_gW || !d_gb || !d_glog_std) return fail(CHUB_ERR_ARG, "null argument");
    for (int l = 0; l < kPolicyMaxLayers; l++) {
        const bool has = l < a->n_layers;
        d_gW[l] = has ? a->d_g + a->ap.param0[l] : nullptr;
        d_gb[l] = has ? a->d_g + a->ap.param0[l] + (int64_t) a->args.out[l] * a->args.in[l] : nullptr;
    }
    *d_glog_std = a->G ? a->d_g + a->ap.param0[a->n_layers] : nullptr;
    return CHUB_OK;
}

int chub_adam_counter_device(chub_adam *a, const int64_t **d_t) {
    if (!a || !d_t) return fail(CHUB_ERR_ARG, "null argument");
    *d_t = reinterpret_cast<const int64_t *>(a->d_scalars) + ADAM_T;
    return CHUB_OK;
}

int chub_adam_step_device(chub_adam *a, const float *const *d_gW, const float *const *d_gb, const float *d_glog_std, double *d_stats, void *stream) {
    if (!a || !d_gW || !d_gb) return fail(CHUB_ERR_ARG, "null argument");
    for (int l = 0; l < a->n_layers; l++)
        if (!d_gW[l] || !d_gb[l]) return fail(CHUB_ERR_ARG, "null argument: d_gW[" + std::to_string(l) + "] / d_gb[" + std::to_string(l) + "]");
    if (a->G && !d_glog_std) return fail(CHUB_ERR_ARG, "null argument: d_glog_std (the parameter vector ends with the policy's log_std)");
    if (!a->G && d_glog_std) return fail(CHUB_ERR_ARG, "d_glog_std: the parameter vector has no log_std (a critic, or a policy without chub_policy_set_exploration at create)");
    HIP_TRY(hipSetDevice(a->net->env->device));
    (void) hipGetLastError();
    AdamArgs g = a->args;
    for (int l = 0; l < a->n_layers; l++) {
        g.gW[l] = d_gW[l];
        g.gb[l] = d_gb[l];
    }
    g.glog_std = d_glog_std;
    g.stats = d_stats;
    launch_adam_step(g, a->ap.blocks, a->ap.blocks, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_adam_reset_device(chub_adam *a, void *stream) {
    if (!a) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(a->net->env->device));
    (void) hipGetLastError();
    launch_adam_reset(a->d_m, a->d_v, a->ap.n, a->d_scalars, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_adam_state_size(chub_adam *a, int64_t *bytes) {
    if (!a || !bytes) return fail(CHUB_ERR_ARG, "null argument");
    *bytes = (int64_t) kAdamBlobHeader + 8 * a->ap.n;
    return CHUB_OK;
}

int chub_adam_get_state(chub_adam *a, void *blob) {
    if (!a || !blob) return fail(CHUB_ERR_ARG, "null argument");
    if (a->net->env->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_adam_get_state between chub_graph_begin and chub_graph_end (it copies and synchronises)");
    HIP_TRY(hipSetDevice(a->net->env->device));
    (void) hipGetLastError();
    HIP_TRY(hipDeviceSynchronize());
    char *p = static_cast<char *>(blob);
    const size_t nf = (size_t) a->ap.n * sizeof(float);
    HIP_TRY(hipMemcpy(p, a->d_scalars + ADAM_T, 24, hipMemcpyDeviceToHost));
    const int64_t n = a->ap.n;
    memcpy(p + 24, &n, 8);
    HIP_TRY(hipMemcpy(p + kAdamBlobHeader, a->d_m, nf, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(p + kAdamBlobHeader + nf, a->d_v, nf, hipMemcpyDeviceToHost));
    return CHUB_OK;
}

int chub_adam_set_state(chub_adam *a, const void *blob) {
    if (!a || !blob) return fail(CHUB_ERR_ARG, "null argument");
    const char *p = static_cast<const char *>(blob);
    int64_t n;
    memcpy(&n, p + 24, 8);
    if (n != a->ap.n)
        return fail(CHUB_ERR_ARG, "chub_adam_set_state: the blob holds " + std::to_string(n) + " parameters, this optimiser " + std::to_string(a->ap.n));
    if (a->net->env->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_adam_set_state between chub_graph_begin and chub_graph_end (it copies and synchronises)");
    HIP_TRY(hipSetDevice(a->net->env->device));
    (void) hipGetLastError();
    HIP_TRY(hipDeviceSynchronize());
    const size_t nf = (size_t) a->ap.n * sizeof(float);
    HIP_TRY(hipMemcpy(a->d_scalars + ADAM_T, p, 24, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(a->d_m, p + kAdamBlobHeader, nf, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(a->d_v, p + kAdamBlobHeader + nf, nf, hipMemcpyHostToDevice));
    return CHUB_OK;
}

// ---- minibatch indices (include/chub.h): the shuffle's definition is chub_adam.h's, shared by the kernel and the host form
int chub_shuffle_rows_device(chub_env *e, uint64_t key, const int64_t *d_counter, int64_t offset, int64_t R, int64_t *d_rows, void *stream) {
    if (!e || !d_rows) return fail(CHUB_ERR_ARG, "null argument");
    if (R < 1 || R > ((int64_t) 1 << 40)) return fail(CHUB_ERR_ARG, "chub_shuffle_rows_device: R is 1 .. 2^40");
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    launch_shuffle_rows(key, d_counter, offset, R, d_rows, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_shuffle_rows(uint64_t key, uint64_t counter, int64_t R, int64_t *rows) {
    if (!rows) return fail(CHUB_ERR_ARG, "null argument");
    if (R < 1 || R > ((int64_t) 1 << 40)) return fail(CHUB_ERR_ARG, "chub_shuffle_rows: R is 1 .. 2^40");
    const int nb = shuffle_bits(R);
    for (int64_t r = 0; r < R; r++) rows[r] = shuffle_row(r, R, nb, key, counter);
    return CHUB_OK;
}

}  // extern "C"

// ---- a training log and a KL stop on the device (include/chub.h): the object, the three launches, the host fold, the gate, the update as
// one call.  The kernels are chub_trainlog.hip's, the fold's arithmetic chub_trainlog.h's
static_assert((int) CHUB_TLOG_WORDS == TLOG_WORDS && (int) CHUB_TLOG_COUNTED == TLOG_COUNTED && (int) CHUB_TLOG_AFTER_STOP == TLOG_AFTER_STOP &&
                  (int) CHUB_TLOG_STOPPED == TLOG_STOPPED && (int) CHUB_TLOG_STOP_INDEX == TLOG_STOP_INDEX && (int) CHUB_TLOG_ACTOR == TLOG_ACTOR &&
                  (int) CHUB_TLOG_KL_MAX == TLOG_KL_MAX && (int) CHUB_TLOG_KL_LAST == TLOG_KL_LAST && (int) CHUB_TLOG_CRITIC == TLOG_CRITIC &&
                  (int) CHUB_TLOG_ACTOR_OPT == TLOG_ACTOR_OPT && (int) CHUB_TLOG_CRITIC_OPT == TLOG_CRITIC_OPT && (int) CHUB_KL_K1 == KL_K1 &&
                  (int) CHUB_KL_K3 == KL_K3 && (int) CHUB_KL_COUNT == KL_COUNT,
              "chub_trainlog.h restates the CHUB_TLOG_* / CHUB_KL_* enums");
static_assert(kTrainLogStepStats == kAdamStats, "the log reads the optimiser's stats block");

struct chub_train_log {
    chub_env *env;
    double *d_block;   // the words [TLOG_WORDS], the gate (one int64 word), then chub_ppo_update's four stats blocks
    double *d_words;
    int64_t *d_gate;
    double *d_pstats, *d_cstats, *d_astats_actor, *d_astats_critic;
    DeviceAllocs allocs;
};

template <class F>
static void for_each_adam(chub_env *e, F f) {
    for (chub_policy *pol : e->policies)
        for (chub_adam *a : pol->net.adams) f(a);
    for (chub_critic *c : e->critics)
        for (chub_adam *a : c->net.adams) f(a);
}

static void train_log_free(chub_train_log *log) {
    chub_env *e = log->env;
    (void) hipSetDevice(e->device);
    (void) hipDeviceSynchronize();  // (a launch still in flight reads the gate and writes the words)
    for_each_adam(e, [log](chub_adam *a) {
        if (a->args.gate == log->d_gate) a->args.gate = nullptr;
    });
    log->allocs.free_all();
    e->train_logs.erase(std::remove(e->train_logs.begin(), e->train_logs.end(), log), e->train_logs.end());
    delete log;
}

static int train_log_check_kl(const char *who, int32_t kl_kind, double kl_limit) {
    if (kl_kind != CHUB_KL_K1 && kl_kind != CHUB_KL_K3) return fail(CHUB_ERR_ARG, std::string(who) + ": kl_kind: CHUB_KL_K1 or CHUB_KL_K3");
    if (!(kl_limit >= 0.0)) return fail(CHUB_ERR_ARG, std::string(who) + ": kl_limit: >= 0 (0: never stops)");
    return CHUB_OK;
}

static int ppo_split(int64_t n_rows, int64_t minibatch_rows, int64_t *minibatches, int64_t *last_rows) {
    if (n_rows < 1) return fail(CHUB_ERR_ARG, "chub_ppo_update: n_rows is at least 1");
    if (minibatch_rows < 1) return fail(CHUB_ERR_ARG, "chub_ppo_update: minibatch_rows is at least 1");
    const int64_t M = (n_rows + minibatch_rows - 1) / minibatch_rows;  // (n_rows <= 2^40 wherever it matters: no overflow below 2^62)
    *minibatches = M;
    *last_rows = n_rows - (M - 1) * minibatch_rows;
    return CHUB_OK;
}

extern "C" {

int chub_train_log_create(chub_env *e, chub_train_log **out) {
    if (!e || !out) return fail(CHUB_ERR_ARG, "null argument");
    *out = nullptr;
    if (e->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_train_log_create between chub_graph_begin and chub_graph_end (it allocates and synchronises)");
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    chub_train_log *log = new chub_train_log();
    log->env = e;
    e->train_logs.push_back(log);
    constexpr size_t kWords = (size_t) TLOG_WORDS + 1 + 2 * kTrainLogGradStats + 2 * kTrainLogStepStats;
    double h[kWords] = {0.0};
    h[TLOG_STOP_INDEX] = -1.0;  // (what begin leaves)
    if (log->allocs.zeroed(&log->d_block, kWords) || hipMemcpy(log->d_block, h, sizeof h, hipMemcpyHostToDevice) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        train_log_free(log);
        (void) hipGetLastError();
        return fail(CHUB_ERR_HIP, "chub_train_log_create: out of device memory");
    }
    log->d_words = log->d_block;
    log->d_gate = reinterpret_cast<int64_t *>(log->d_block + TLOG_WORDS);
    log->d_pstats = log->d_block + TLOG_WORDS + 1;
    log->d_cstats = log->d_pstats + kTrainLogGradStats;
    log->d_astats_actor = log->d_cstats + kTrainLogGradStats;
    log->d_astats_critic = log->d_astats_actor + kTrainLogStepStats;
    *out = log;
    return CHUB_OK;
}

int chub_train_log_destroy(chub_train_log *log) {
    if (!log) return CHUB_OK;
    if (log->env->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_train_log_destroy between chub_graph_begin and chub_graph_end (it synchronises and frees)");
    train_log_free(log);
    (void) hipGetLastError();
    return CHUB_OK;
}

int chub_train_log_begin_device(chub_train_log *log, void *stream) {
    if (!log) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(log->env->device));
    (void) hipGetLastError();
    launch_trainlog_begin(log->d_words, log->d_gate, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_train_log_record_device(chub_train_log *log, const double *d_pstats, const double *d_cstats, int32_t kl_kind, double kl_limit, void *stream) {
    if (!log) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = train_log_check_kl("chub_train_log_record_device", kl_kind, kl_limit)) return rc;
    HIP_TRY(hipSetDevice(log->env->device));
    (void) hipGetLastError();
    launch_trainlog_record(log->d_words, log->d_gate, d_pstats, d_cstats, kl_kind, kl_limit, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_train_log_steps_device(chub_train_log *log, const double *d_astats_actor, const double *d_astats_critic, void *stream) {
    if (!log) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(log->env->device));
    (void) hipGetLastError();
    launch_trainlog_steps(log->d_words, d_astats_actor, d_astats_critic, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_train_log_device(chub_train_log *log, const double **d_words, const int64_t **d_gate) {
    if (!log || !d_words || !d_gate) return fail(CHUB_ERR_ARG, "null argument");
    *d_words = log->d_words;
    *d_gate = log->d_gate;
    return CHUB_OK;
}

int chub_train_log_read(chub_train_log *log, double *words) {
    if (!log || !words) return fail(CHUB_ERR_ARG, "null argument");
    if (log->env->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_train_log_read between chub_graph_begin and chub_graph_end (it copies and synchronises)");
    HIP_TRY(hipSetDevice(log->env->device));
    (void) hipGetLastError();
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(words, log->d_words, (size_t) TLOG_WORDS * sizeof(double), hipMemcpyDeviceToHost));
    return CHUB_OK;
}

int chub_train_log_fold(double *words, int64_t *gate, const double *pstats, const double *cstats, int32_t kl_kind, double kl_limit) {
    if (!words || !gate) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = train_log_check_kl("chub_train_log_fold", kl_kind, kl_limit)) return rc;
    trainlog_record(words, gate, pstats, cstats, kl_kind, kl_limit);
    return CHUB_OK;
}

int chub_adam_set_gate(chub_adam *a, const int64_t *d_gate) {
    if (!a) return fail(CHUB_ERR_ARG, "null argument");
    a->args.gate = d_gate;
    return CHUB_OK;
}

int chub_ppo_update_plan(int64_t n_rows, int64_t minibatch_rows, int64_t *minibatches, int64_t *last_rows) {
    if (!minibatches || !last_rows) return fail(CHUB_ERR_ARG, "null argument");
    return ppo_split(n_rows, minibatch_rows, minibatches, last_rows);
}

int chub_ppo_update(const chub_ppo_update_args *u, void *stream) {
    if (!u) return fail(CHUB_ERR_ARG, "null argument");
    if (!u->grad || !u->critic || !u->actor_opt || !u->critic_opt) return fail(CHUB_ERR_ARG, "chub_ppo_update: null grad, critic, actor_opt or critic_opt");
    chub_policy *pol = u->grad->pol;
    chub_env *e = pol->net.env;
    if (u->critic->net.env != e || u->actor_opt->net->env != e || u->critic_opt->net->env != e || (u->log && u->log->env != e))
        return fail(CHUB_ERR_ARG, "chub_ppo_update: the gradient object, the critic, the optimisers and the log belong to one handle");
    if (u->actor_opt->net != &pol->net) return fail(CHUB_ERR_ARG, "chub_ppo_update: actor_opt is not an optimiser of the gradient object's policy");
    if (u->critic_opt->net != &u->critic->net) return fail(CHUB_ERR_ARG, "chub_ppo_update: critic_opt is not an optimiser of the critic");
    if (u->epochs < 1) return fail(CHUB_ERR_ARG, "chub_ppo_update: epochs is at least 1");
    int64_t M, last;
    if (const int rc = ppo_split(u->n_rows, u->minibatch_rows, &M, &last)) return rc;
    if (u->minibatch_rows > u->grad->max_rows || u->minibatch_rows > u->critic->max_rows)
        return fail(CHUB_ERR_ARG, "chub_ppo_update: minibatch_rows is at most the gradient object's max_rows = " + std::to_string(u->grad->max_rows) +
                                      " and the critic's = " + std::to_string(u->critic->max_rows));
    if (!u->d_rows) return fail(CHUB_ERR_ARG, "chub_ppo_update: null d_rows (the caller's [n_rows] int64 the shuffles are written to)");
    if (const int rc = train_log_check_kl("chub_ppo_update", u->kl_kind, u->kl_limit)) return rc;
    if (u->n_rows > ((int64_t) 1 << 40)) return fail(CHUB_ERR_ARG, "chub_ppo_update: chub_shuffle_rows_device: R is 1 .. 2^40");
    // the constituents' own refusals, for both sizes of a minibatch, before anything is enqueued
    chub_policy_grad_in pin = {};
    pin.n_rows = u->n_rows;
    pin.d_features = u->d_features;
    pin.ld_features = u->ld_features;
    pin.d_pile_bits = u->d_pile_bits;
    pin.d_set_bits = u->d_set_bits;
    pin.d_u = u->d_u;
    pin.d_logp_old = u->d_logp_old;
    pin.d_adv = u->d_adv;
    pin.d_adv_stats = u->d_adv_stats;
    pin.loss = u->policy_loss;
    pin.clip_eps = u->policy_clip_eps;
    pin.ent_coef = u->ent_coef;
    chub_critic_grad_in cin = {};
    cin.n_rows = u->n_rows;
    cin.d_x = u->d_features;
    cin.ld = u->ld_features;
    cin.d_ret = u->d_ret;
    cin.d_v_old = u->d_v_old;
    cin.loss = u->value_loss;
    cin.clip_eps = u->value_clip_eps;
    const int64_t sizes[2] = {M > 1 ? u->minibatch_rows : last, last};
    for (int k = 0; k < 2; k++) {
        pin.R = cin.R = sizes[k];
        pin.d_rows = cin.d_rows = u->d_rows;
        if (const int rc = policy_grad_check(u->grad, &pin)) return fail(rc, "chub_ppo_update: chub_policy_grad_device: " + std::string(g_err));
        if (const int rc = critic_grad_check(u->critic, &cin)) return fail(rc, "chub_ppo_update: chub_critic_grad_device: " + std::string(g_err));
    }
    chub_policy_grad_out pout = {};
    chub_critic_grad_out cout_ = {};
    float *unused = nullptr;
    if (const int rc = chub_adam_grads(u->actor_opt, pout.d_gW, pout.d_gb, &pout.d_glog_std)) return rc;
    if (const int rc = chub_adam_grads(u->critic_opt, cout_.d_gW, cout_.d_gb, &unused)) return rc;
    chub_train_log *log = u->log;
    double *astats_actor = log ? log->d_astats_actor : u->actor_opt->d_own_stats + kTrainLogGradStats;
    double *astats_critic = log ? log->d_astats_critic : u->critic_opt->d_own_stats + kTrainLogGradStats;
    pout.d_stats = log ? log->d_pstats : u->actor_opt->d_own_stats;
    cout_.d_stats = log ? log->d_cstats : u->critic_opt->d_own_stats;
    const int64_t *gate_a = u->actor_opt->args.gate, *gate_c = u->critic_opt->args.gate;
    if (log) u->actor_opt->args.gate = u->critic_opt->args.gate = log->d_gate;
    const int64_t *d_t = reinterpret_cast<const int64_t *>(u->actor_opt->d_scalars) + ADAM_T;
    int rc = log ? chub_train_log_begin_device(log, stream) : CHUB_OK;
    for (int32_t ep = 0; ep < u->epochs && !rc; ep++) {
        rc = chub_shuffle_rows_device(e, u->key, d_t, ep, u->n_rows, u->d_rows, stream);
        for (int64_t i = 0; i < M && !rc; i++) {
            pin.R = cin.R = i + 1 < M ? u->minibatch_rows : last;
            pin.d_rows = cin.d_rows = u->d_rows + i * u->minibatch_rows;
            rc = chub_policy_grad_device(u->grad, &pin, &pout, stream);
            if (!rc) rc = chub_critic_grad_device(u->critic, &cin, &cout_, stream);
            if (!rc && log) rc = chub_train_log_record_device(log, pout.d_stats, cout_.d_stats, u->kl_kind, u->kl_limit, stream);
            if (!rc) rc = chub_adam_step_device(u->actor_opt, pout.d_gW, pout.d_gb, pout.d_glog_std, astats_actor, stream);
            if (!rc) rc = chub_adam_step_device(u->critic_opt, cout_.d_gW, cout_.d_gb, nullptr, astats_critic, stream);
            if (!rc && log) rc = chub_train_log_steps_device(log, astats_actor, astats_critic, stream);
        }
    }
    u->actor_opt->args.gate = gate_a;
    u->critic_opt->args.gate = gate_c;
    return rc;
}

}  // extern "C"

// ---- constrained PPO on the device (include/chub.h): the object, the three device calls, the state calls, the host fold.  The kernels are
// chub_lagrange.hip's, the step rule's arithmetic chub_lagrange.h's
static_assert((int) CHUB_COST_STEP == COST_STEP && (int) CHUB_COST_AT_DONE == COST_AT_DONE && (int) CHUB_COST_KIND_COUNT == COST_KIND_COUNT &&
                  (int) CHUB_LAG_MAX_K == kLagMaxK && (int) CHUB_LAG_STATS == kLagStats && (int) CHUB_LAG_WORDS == kLagWords,
              "chub_lagrange.h restates the CHUB_COST_* / CHUB_LAG_* enums");

struct chub_lagrange {
    chub_env *env;
    int32_t K;
    chub_constraint c[kLagMaxK];
    double *d_block;     // lambda [K], the stats [K][6], the words [K][3]
    double *d_lambda, *d_stats, *d_words;
    double *d_partials;  // [ceil(N / 256)][K][6]
    DeviceAllocs allocs;
};

static void lagrange_free(chub_lagrange *lag) {
    chub_env *e = lag->env;
    (void) hipSetDevice(e->device);
    (void) hipDeviceSynchronize();  // (a launch still in flight reads and writes the block)
    lag->allocs.free_all();
    e->lagranges.erase(std::remove(e->lagranges.begin(), e->lagranges.end(), lag), e->lagranges.end());
    delete lag;
}

static int lagrange_check_constraint(const char *who, const chub_constraint &c) {
    const std::string w(who);
    if (c.column < 0) return fail(CHUB_ERR_ARG, w + ": a constraint's column is at least 0");
    if (c.kind != CHUB_COST_STEP && c.kind != CHUB_COST_AT_DONE) return fail(CHUB_ERR_ARG, w + ": kind: CHUB_COST_STEP or CHUB_COST_AT_DONE");
    const double v[4] = {c.limit, c.lr, c.lambda0, c.lambda_max};
    for (double x : v)
        if (!(x >= 0.0) || !__builtin_isfinite(x)) return fail(CHUB_ERR_ARG, w + ": limit, lr, lambda0 and lambda_max are finite and not negative");
    if (c.lambda_max != 0.0 && c.lambda0 > c.lambda_max) return fail(CHUB_ERR_ARG, w + ": lambda0 lies at or below a non-zero lambda_max");
    return CHUB_OK;
}

extern "C" {

int chub_lagrange_create(chub_env *e, int32_t K, const chub_constraint *c, chub_lagrange **out) {
    if (!e || !c || !out) return fail(CHUB_ERR_ARG, "null argument");
    *out = nullptr;
    if (K < 1 || K > kLagMaxK) return fail(CHUB_ERR_ARG, "chub_lagrange_create: K is 1 .. 4 constraints");
    for (int32_t k = 0; k < K; k++)
        if (const int rc = lagrange_check_constraint("chub_lagrange_create", c[k])) return rc;
    if (e->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_lagrange_create between chub_graph_begin and chub_graph_end (it allocates and synchronises)");
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    chub_lagrange *lag = new chub_lagrange();
    lag->env = e;
    lag->K = K;
    for (int32_t k = 0; k < K; k++) lag->c[k] = c[k];
    e->lagranges.push_back(lag);
    const size_t words = (size_t) K * (1 + kLagStats + kLagWords);
    const size_t blocks = ((size_t) e->hp.n_envs + kLagLanes - 1) / kLagLanes;
    double h[kLagMaxK] = {0.0};
    for (int32_t k = 0; k < K; k++) h[k] = c[k].lambda0;
    if (lag->allocs.zeroed(&lag->d_block, words) || lag->allocs.zeroed(&lag->d_partials, blocks * (size_t) K * kLagStats) ||
        hipMemcpy(lag->d_block, h, (size_t) K * sizeof(double), hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        lagrange_free(lag);
        (void) hipGetLastError();
        return fail(CHUB_ERR_HIP, "chub_lagrange_create: out of device memory");
    }
    lag->d_lambda = lag->d_block;
    lag->d_stats = lag->d_lambda + K;
    lag->d_words = lag->d_stats + (size_t) K * kLagStats;
    *out = lag;
    return CHUB_OK;
}

int chub_lagrange_destroy(chub_lagrange *lag) {
    if (!lag) return CHUB_OK;
    if (lag->env->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_lagrange_destroy between chub_graph_begin and chub_graph_end (it synchronises and frees)");
    lagrange_free(lag);
    (void) hipGetLastError();
    return CHUB_OK;
}

int chub_lagrange_gae_device(chub_lagrange *lag, const chub_cost_gae *g, void *stream) {
    if (!lag || !g) return fail(CHUB_ERR_ARG, "null argument");
    if (!g->d_terms || !g->d_packed) return fail(CHUB_ERR_ARG, "chub_lagrange_gae_device: d_terms and d_packed are required");
    if (const int rc = gae_check_T("chub_lagrange_gae_device", g->T)) return rc;
    if (g->C < 1) return fail(CHUB_ERR_ARG, "chub_lagrange_gae_device: C >= 1 floats in a d_terms row");
    if (const int rc = gae_check_discounts("chub_lagrange_gae_device", g->gamma, g->lambda)) return rc;
    for (int32_t k = 0; k < lag->K; k++) {
        if (lag->c[k].column >= g->C) return fail(CHUB_ERR_ARG, "chub_lagrange_gae_device: a constraint's column lies outside 0 .. C - 1");
        if (!g->d_adv[k]) return fail(CHUB_ERR_ARG, "chub_lagrange_gae_device: d_adv[k] is required for every constraint");
    }
    const chub_env *e = lag->env;
    if ((uint64_t) e->hp.n_envs * (uint64_t) std::max(e->hp.obs_dim + 2, g->C) * sizeof(float) > 0xffffffffull)
        return fail(CHUB_ERR_UNSUPPORTED, "chub_lagrange_gae_device: one step's block of d_packed or d_terms is at most 4 GiB (the kernel's offsets are 32 bits)");
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    CostGaeArgs a = {};
    a.n_envs = e->hp.n_envs;
    a.T = g->T;
    a.D = e->hp.obs_dim;
    a.C = g->C;
    a.K = lag->K;
    a.gamma = g->gamma;
    a.gl = g->gamma * g->lambda;
    a.terms = g->d_terms;
    a.packed = g->d_packed;
    a.mask = g->d_mask;
    a.carry = g->d_ep_carry;
    a.partials = lag->d_partials;
    a.stats = lag->d_stats;
    for (int32_t k = 0; k < lag->K; k++) {
        a.values[k] = g->d_values[k];
        a.final_values[k] = g->d_final_values[k];
        a.adv[k] = g->d_adv[k];
        a.ret[k] = g->d_ret[k];
        a.column[k] = lag->c[k].column;
        a.kind[k] = lag->c[k].kind;
    }
    launch_cost_gae(a, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_lagrange_step_device(chub_lagrange *lag, void *stream) {
    if (!lag) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(lag->env->device));
    (void) hipGetLastError();
    LagrangeStepArgs a = {};
    a.K = lag->K;
    a.lambda = lag->d_lambda;
    a.words = lag->d_words;
    a.stats = lag->d_stats;
    for (int32_t k = 0; k < lag->K; k++) {
        a.limit[k] = lag->c[k].limit;
        a.lr[k] = lag->c[k].lr;
        a.lambda_max[k] = lag->c[k].lambda_max;
    }
    launch_lagrange_step(a, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_lagrange_combine_device(chub_lagrange *lag, int64_t n, const float *d_adv, const double *d_adv_stats, const float *const *d_adv_cost,
                                 float *d_out, void *stream) {
    if (!lag || !d_adv || !d_adv_cost || !d_out) return fail(CHUB_ERR_ARG, "null argument");
    if (n < 1) return fail(CHUB_ERR_ARG, "chub_lagrange_combine_device: n >= 1 entries");
    for (int32_t k = 0; k < lag->K; k++)
        if (!d_adv_cost[k]) return fail(CHUB_ERR_ARG, "chub_lagrange_combine_device: d_adv_cost[k] is required for every constraint");
    HIP_TRY(hipSetDevice(lag->env->device));
    (void) hipGetLastError();
    LagrangeCombineArgs a = {};
    a.n = n;
    a.K = lag->K;
    a.adv = d_adv;
    a.adv_stats = d_adv_stats;
    a.lambda = lag->d_lambda;
    a.stats = lag->d_stats;
    for (int32_t k = 0; k < lag->K; k++) a.advc[k] = d_adv_cost[k];
    a.out = d_out;
    launch_lagrange_combine(a, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_lagrange_device(chub_lagrange *lag, const double **d_lambda, const double **d_stats) {
    if (!lag || !d_lambda || !d_stats) return fail(CHUB_ERR_ARG, "null argument");
    *d_lambda = lag->d_lambda;
    *d_stats = lag->d_stats;
    return CHUB_OK;
}

int chub_lagrange_read(chub_lagrange *lag, double *lambda, double *stats, double *words) {
    if (!lag) return fail(CHUB_ERR_ARG, "null argument");
    if (lag->env->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_lagrange_read between chub_graph_begin and chub_graph_end (it copies and synchronises)");
    HIP_TRY(hipSetDevice(lag->env->device));
    (void) hipGetLastError();
    HIP_TRY(hipDeviceSynchronize());
    const size_t K = (size_t) lag->K;
    if (lambda) HIP_TRY(hipMemcpy(lambda, lag->d_lambda, K * sizeof(double), hipMemcpyDeviceToHost));
    if (stats) HIP_TRY(hipMemcpy(stats, lag->d_stats, K * kLagStats * sizeof(double), hipMemcpyDeviceToHost));
    if (words) HIP_TRY(hipMemcpy(words, lag->d_words, K * kLagWords * sizeof(double), hipMemcpyDeviceToHost));
    return CHUB_OK;
}

int chub_lagrange_set_lambda_device(chub_lagrange *lag, const double *d_lambda, void *stream) {
    if (!lag || !d_lambda) return fail(CHUB_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(lag->env->device));
    (void) hipGetLastError();
    launch_lagrange_set_lambda(lag->d_lambda, d_lambda, lag->K, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

// the checkpoint blob: K as an int64, lambda [K], the words [K][3]
int chub_lagrange_state_size(chub_lagrange *lag, int64_t *bytes) {
    if (!lag || !bytes) return fail(CHUB_ERR_ARG, "null argument");
    *bytes = (int64_t) (sizeof(int64_t) + (size_t) lag->K * (1 + kLagWords) * sizeof(double));
    return CHUB_OK;
}

int chub_lagrange_get_state(chub_lagrange *lag, void *blob) {
    if (!lag || !blob) return fail(CHUB_ERR_ARG, "null argument");
    if (lag->env->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_lagrange_get_state between chub_graph_begin and chub_graph_end (it copies and synchronises)");
    const int64_t K = lag->K;
    memcpy(blob, &K, sizeof K);
    double *w = reinterpret_cast<double *>(static_cast<char *>(blob) + sizeof K);
    return chub_lagrange_read(lag, w, nullptr, w + K);
}

int chub_lagrange_set_state(chub_lagrange *lag, const void *blob) {
    if (!lag || !blob) return fail(CHUB_ERR_ARG, "null argument");
    if (lag->env->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_lagrange_set_state between chub_graph_begin and chub_graph_end (it copies and synchronises)");
    int64_t K;
    memcpy(&K, blob, sizeof K);
    if (K != lag->K) return fail(CHUB_ERR_ARG, "chub_lagrange_set_state: the blob was taken from an object of another K");
    const double *w = reinterpret_cast<const double *>(static_cast<const char *>(blob) + sizeof K);
    HIP_TRY(hipSetDevice(lag->env->device));
    (void) hipGetLastError();
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(lag->d_lambda, w, (size_t) K * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(lag->d_words, w + K, (size_t) K * kLagWords * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    return CHUB_OK;
}

int chub_lagrange_fold(const chub_constraint *c, double *lambda, double *words, const double *stats) {
    if (!c || !lambda || !words || !stats) return fail(CHUB_ERR_ARG, "null argument");
    if (const int rc = lagrange_check_constraint("chub_lagrange_fold", *c)) return rc;
    lagrange_step(lambda, words, stats, c->limit, c->lr, c->lambda_max);
    return CHUB_OK;
}

}  // extern "C"

// ---- reward scaling on the device (include/chub.h): the object, the four device calls, the state calls, the host fold.  The kernels are
// chub_retnorm.hip's, the merge's arithmetic chub_retnorm.h's
struct chub_return_norm {
    chub_env *env;
    chub_return_norm_spec spec;
    double *d_words;     // the state [3], then the pivot copy [2] (never move)
    double *d_state, *d_pivot;
    float *d_scale;      // [1]
    float *d_carry;      // [N]
    double *d_partials;  // [ceil(N / 256)][3]
    DeviceAllocs allocs;
};

static void return_norm_free(chub_return_norm *rn) {
    chub_env *e = rn->env;
    (void) hipSetDevice(e->device);
    (void) hipDeviceSynchronize();  // (a launch still in flight reads and writes the buffers)
    rn->allocs.free_all();
    e->return_norms.erase(std::remove(e->return_norms.begin(), e->return_norms.end(), rn), e->return_norms.end());
    delete rn;
}

// what every call on an object checks first: the object, and that its handle has not become a tape handle
static int return_norm_check(const chub_return_norm *rn, const char *who) {
    if (!rn) return fail(CHUB_ERR_ARG, "null argument");
    if (rn->env->tape_only) return fail(CHUB_ERR_UNSUPPORTED, std::string(who) + " is not supported on a tape handle (chub_tape_register_soc)");
    return CHUB_OK;
}

struct ReturnNormBlobHead {
    uint64_t magic;
    int64_t n_envs;
    double state[3];
    float scale, pad_;
};
static_assert(sizeof(ReturnNormBlobHead) == 48, "the blob's head is 48 bytes");

extern "C" {

int chub_return_norm_create(chub_env *e, const chub_return_norm_spec *spec, chub_return_norm **out) {
    if (!e || !spec || !out) return fail(CHUB_ERR_ARG, "null argument");
    *out = nullptr;
    if (!(spec->gamma >= 0.0f && spec->gamma <= 1.0f)) return fail(CHUB_ERR_ARG, "chub_return_norm_create: gamma lies in [0, 1]");
    if (!(spec->eps > 0.0) || !__builtin_isfinite(spec->eps)) return fail(CHUB_ERR_ARG, "chub_return_norm_create: eps is finite and above 0");
    if (!(spec->clip >= 0.0f)) return fail(CHUB_ERR_ARG, "chub_return_norm_create: clip is at least 0 (0: none)");
    if (e->tape_only) return fail(CHUB_ERR_UNSUPPORTED, "chub_return_norm_create is not supported on a tape handle (chub_tape_register_soc)");
    if (e->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_return_norm_create between chub_graph_begin and chub_graph_end (it allocates and synchronises)");
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    chub_return_norm *rn = new chub_return_norm();
    rn->env = e;
    rn->spec = *spec;
    e->return_norms.push_back(rn);
    const size_t N = (size_t) e->hp.n_envs, blocks = (N + kRetLanes - 1) / kRetLanes;
    const float one = 1.0f;
    if (rn->allocs.zeroed(&rn->d_words, 5) || rn->allocs.zeroed(&rn->d_scale, 1) || rn->allocs.zeroed(&rn->d_carry, N) ||
        rn->allocs.zeroed(&rn->d_partials, blocks * 3) || hipMemcpy(rn->d_scale, &one, sizeof one, hipMemcpyHostToDevice) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        return_norm_free(rn);
        (void) hipGetLastError();
        return fail(CHUB_ERR_HIP, "chub_return_norm_create: out of device memory");
    }
    rn->d_state = rn->d_words;
    rn->d_pivot = rn->d_words + 3;
    *out = rn;
    return CHUB_OK;
}

int chub_return_norm_destroy(chub_return_norm *rn) {
    if (!rn) return CHUB_OK;
    if (rn->env->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_return_norm_destroy between chub_graph_begin and chub_graph_end (it synchronises and frees)");
    return_norm_free(rn);
    (void) hipGetLastError();
    return CHUB_OK;
}

int chub_return_norm_update_device(chub_return_norm *rn, const float *d_packed, int64_t T, const uint8_t *d_mask, void *stream) {
    if (const int rc = return_norm_check(rn, "chub_return_norm_update_device")) return rc;
    if (!d_packed) return fail(CHUB_ERR_ARG, "null argument");
    if (T <= 0) return fail(CHUB_ERR_ARG, "chub_return_norm_update_device: T >= 1");
    const chub_env *e = rn->env;
    HIP_TRY(hipSetDevice(e->device));
    (void) hipGetLastError();
    ReturnMomentsArgs a = {};
    a.n_envs = e->hp.n_envs;
    a.T = T;
    a.D = e->hp.obs_dim;
    a.gamma = rn->spec.gamma;
    a.eps = rn->spec.eps;
    a.packed = d_packed;
    a.mask = d_mask;
    a.carry = rn->d_carry;
    a.partials = rn->d_partials;
    a.pivot = rn->d_pivot;
    a.state = rn->d_state;
    a.scale = rn->d_scale;
    launch_return_moments(a, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_return_norm_gae_device(chub_return_norm *rn, const chub_gae *g, void *stream) {
    if (const int rc = return_norm_check(rn, "chub_return_norm_gae_device")) return rc;
    if (!g) return fail(CHUB_ERR_ARG, "null argument");
    GaeArgs a;
    if (const int rc = gae_args(&a, "chub_return_norm_gae_device", rn->env, g)) return rc;
    a.clip = rn->spec.clip;
    a.scale = rn->d_scale;
    launch_gae(a, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_return_norm_reset_carry_device(chub_return_norm *rn, const uint8_t *d_mask, void *stream) {
    if (const int rc = return_norm_check(rn, "chub_return_norm_reset_carry_device")) return rc;
    HIP_TRY(hipSetDevice(rn->env->device));
    (void) hipGetLastError();
    launch_return_reset_carry(rn->d_carry, d_mask, rn->env->hp.n_envs, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_return_norm_reset_device(chub_return_norm *rn, void *stream) {
    if (const int rc = return_norm_check(rn, "chub_return_norm_reset_device")) return rc;
    HIP_TRY(hipSetDevice(rn->env->device));
    (void) hipGetLastError();
    launch_return_reset(rn->d_state, rn->d_scale, rn->d_carry, rn->env->hp.n_envs, (hipStream_t) stream);
    HIP_TRY(hipGetLastError());
    return CHUB_OK;
}

int chub_return_norm_device(chub_return_norm *rn, const double **d_state, const float **d_scale, const float **d_carry) {
    if (!rn) return fail(CHUB_ERR_ARG, "null argument");
    if (d_state) *d_state = rn->d_state;
    if (d_scale) *d_scale = rn->d_scale;
    if (d_carry) *d_carry = rn->d_carry;
    return CHUB_OK;
}

int chub_return_norm_state_size(chub_return_norm *rn, int64_t *bytes) {
    if (!rn || !bytes) return fail(CHUB_ERR_ARG, "null argument");
    *bytes = (int64_t) (sizeof(ReturnNormBlobHead) + (size_t) rn->env->hp.n_envs * sizeof(float));
    return CHUB_OK;
}

int chub_return_norm_get_state(chub_return_norm *rn, void *blob) {
    if (const int rc = return_norm_check(rn, "chub_return_norm_get_state")) return rc;
    if (!blob) return fail(CHUB_ERR_ARG, "null argument");
    if (rn->env->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_return_norm_get_state between chub_graph_begin and chub_graph_end (it copies and synchronises)");
    HIP_TRY(hipSetDevice(rn->env->device));
    (void) hipGetLastError();
    HIP_TRY(hipDeviceSynchronize());
    ReturnNormBlobHead h = {};
    h.magic = CHUB_RETURN_NORM_MAGIC;
    h.n_envs = rn->env->hp.n_envs;
    HIP_TRY(hipMemcpy(h.state, rn->d_state, sizeof h.state, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&h.scale, rn->d_scale, sizeof h.scale, hipMemcpyDeviceToHost));
    memcpy(blob, &h, sizeof h);
    HIP_TRY(hipMemcpy(static_cast<char *>(blob) + sizeof h, rn->d_carry, (size_t) h.n_envs * sizeof(float), hipMemcpyDeviceToHost));
    return CHUB_OK;
}

int chub_return_norm_set_state(chub_return_norm *rn, const void *blob) {
    if (const int rc = return_norm_check(rn, "chub_return_norm_set_state")) return rc;
    if (!blob) return fail(CHUB_ERR_ARG, "null argument");
    if (rn->env->capturing) return fail(CHUB_ERR_UNSUPPORTED, "chub_return_norm_set_state between chub_graph_begin and chub_graph_end (it copies and synchronises)");
    ReturnNormBlobHead h;
    memcpy(&h, blob, sizeof h);
    if (h.magic != CHUB_RETURN_NORM_MAGIC) return fail(CHUB_ERR_ARG, "chub_return_norm_set_state: not a return-norm state blob (the magic differs)");
    if (h.n_envs != rn->env->hp.n_envs) return fail(CHUB_ERR_ARG, "chub_return_norm_set_state: the blob was taken from an object of another N");
    HIP_TRY(hipSetDevice(rn->env->device));
    (void) hipGetLastError();
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(rn->d_state, h.state, sizeof h.state, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(rn->d_scale, &h.scale, sizeof h.scale, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(rn->d_carry, static_cast<const char *>(blob) + sizeof h, (size_t) h.n_envs * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    return CHUB_OK;
}

int chub_return_norm_fold(double state[3], float *scale, double n_b, double K, double S1, double S2, double eps) {
    if (!state || !scale) return fail(CHUB_ERR_ARG, "null argument");
    if (!(eps > 0.0) || !__builtin_isfinite(eps)) return fail(CHUB_ERR_ARG, "chub_return_norm_fold: eps is finite and above 0");
    return_norm_fold(state, scale, n_b, K, S1, S2, eps);
    return CHUB_OK;
}

}  // extern "C"
