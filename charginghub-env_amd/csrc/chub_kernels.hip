// chub_kernels.hip -- the per-step hot path of the charging-hub environment as CDNA4 (gfx950) kernels.
//
//   k_slot_packed   2 charger slots per lane, every PHILOX step and reset (production).  The workgroup's 512 virtual lanes are
//           laid over whole envs end to end (hub-major 4-byte slot state, like the action rows); phases in the reference's
//           order (CHS.hpp:1188-1207 / 1499-1518): departures -> arrivals (pre-drawn levels, renege, balk) -> admission by
//           ballot + prefix rank (across waves through LDS) in the shadow of the class-row reads -> on/off, car_step = the
//           next row entry -> station sums (integer LDS atomics) -> last wave: add_car for the new cars, one 16-byte
//           station record per unit.
//   k_slot  the same phases with wave-local units (H = pow2 >= S_k lanes each): COMPAT streams (16-byte hot record, curves
//           evaluated), PHILOX scalar-load control.
//   k_env   lane = environment.  The scalar tail of step(): electrolyser clamp against the grid limit, FCEV arrivals +
//           SAE-J2601 fueling + the waiting list, electrolyser / compressor / tank, renewable netting, fuel cell, incomes and
//           reward, done, exogenous update (PV / wind / price OU) and the normalised observation.  The J2601 breakpoints
//           are immediates; the PV and wind rows of the current slot and the electrolyser action->power table are staged
//           in LDS; its last workgroups draw the next step's state-independent variates.  MULTI: per-env clocks.
//   k_reset_levels, k_draw_levels, k_compat_ctor_sweep, k_random_actions, k_tick_advance, k_fill_clocks: small
//           helpers (reset draws, a step's own station draws, COMPAT constructor replay, bench policy,
//           graph replays, per-env clocks).
//   k_pile_obs, k_station_profile: every pile's Station::situation values by ONE decode (pile_decode), as columns and as
//           per-station bins; chub_get_slots is k_pile_obs with every field.
//   k_forecast: the next H slots of what is deterministic about an env's day (time, tariff, PV / wind profiles, mean arrivals).
//
// No MFMA: there is no dense contraction anywhere in this path.  By bytes it is HBM-bound; measured VALU
// issue, the vector L1's access rate and HBM streaming are each more than half used.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "chub_device.h"
#include "chub_plan.h"

namespace chub {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// Per-env clocks: the envs a launch serves (StepArgs::env_mask) and the clock each env is on (StepArgs::env_clk, double-
// buffered by tick parity; lock-step: every env, the clock in StepArgs itself)
__device__ __forceinline__ bool in_group(const StepArgs &sa, int64_t env) { return !sa.env_mask || sa.env_mask[env] != 0; }
__device__ __forceinline__ uint32_t env_clk(const StepArgs &sa, int64_t n_envs, int64_t env) {
    return sa.env_clk[(int64_t) (sa.tick & 1u) * n_envs + env];
}
// A call on a subset of the envs only launches work for the range of envs it names (StepArgs::env_lo .. env_hi: the first and the
// last served env; every env in a lock-step call): lane i of a grid over `segments` copies of that range -> segment, env
__device__ __forceinline__ int64_t range_len(const StepArgs &sa) { return (int64_t) sa.env_hi - sa.env_lo + 1; }
__device__ __forceinline__ bool range_unit(const StepArgs &sa, int64_t i, int segments, int &seg, int64_t &env) {
    const int64_t R = range_len(sa);
    if (i >= (int64_t) segments * R) return false;
    seg = (i >= R ? 1 : 0) + (i >= 2 * R ? 1 : 0);
    env = sa.env_lo + (i - (int64_t) seg * R);
    return true;
}

__device__ __forceinline__ int clk_t(uint32_t c) { return (int) (c & 127u); }
__device__ __forceinline__ uint32_t clk_next(uint32_t c) {  // one step later: slot of day + 1 (mod 96), price_count + 1 (mod 4)
    return (uint32_t) ((clk_t(c) + 1) % 96) | ((((c >> 8) + 1u) & 3u) << 8);
}

// ------------------------------------------------------------------------------------------ Philox
struct U4 {
    uint32_t v[4];
};

__device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                            uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; i++) {
        // (one 32 x 32 -> 64 multiply per product -- v_mad_u64_u32 -- instead of a v_mul_hi_u32 / v_mul_lo_u32 pair: all three run at a quarter of the
        // 32-bit rate, and a block is 20 products)
        const uint64_t p0 = (uint64_t) 0xD2511F53u * c0, p1 = (uint64_t) 0xCD9E8D57u * c2;
        const uint32_t h0 = (uint32_t) (p0 >> 32), l0 = (uint32_t) p0, h1 = (uint32_t) (p1 >> 32), l1 = (uint32_t) p1;
        uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    U4 r;
    r.v[0] = c0; r.v[1] = c1; r.v[2] = c2; r.v[3] = c3;
    return r;
}

__device__ __forceinline__ uint32_t pick(const U4 &b, int i) {
    uint32_t r = b.v[0];
    r = (i == 1) ? b.v[1] : r;
    r = (i == 2) ? b.v[2] : r;
    r = (i == 3) ? b.v[3] : r;
    return r;
}

// Philox tick of a launch = the host's tick (a kernel argument) + a base kept in device memory: a captured graph of steps bakes
// the host ticks in, and every replay moves the base on (k_tick_advance, the graph's last node), so no counter ever repeats
#define CHUB_TICK(hp, host_tick) ((host_tick) + *(hp).tick_base)
struct PhiloxCtx {
    uint32_t k0, k1, tick, gid;
    __device__ __forceinline__ U4 block(uint32_t site, uint32_t index, uint32_t blk) const {
        return philox4x32_10(blk, (site << 16) | index, tick, gid, k0, k1);
    }
};

// ------------------------------------------------------------- reference streams (COMPAT), one lane
// The ring lives in global memory (RingGlobal: every kernel but the split step's walk) or, for the walk of the split step, parked in LDS
// (RingLds: word w of the workgroup's lane l at s[w * 256 + l] -- a draw is then two LDS reads instead of two dependent global round trips)
struct RingGlobal {
    uint32_t *g;
    __device__ __forceinline__ uint32_t get(uint32_t i) const { return g[i]; }
    __device__ __forceinline__ void set(uint32_t i, uint32_t v) const { g[i] = v; }
};
template <int NW>
struct RingLdsT {  // NW: the lanes (envs) whose rings share the area
    uint32_t *s;
    __device__ __forceinline__ uint32_t get(uint32_t i) const { return s[i * (uint32_t) NW]; }
    __device__ __forceinline__ void set(uint32_t i, uint32_t v) const { s[i * (uint32_t) NW] = v; }
};
typedef RingLdsT<256> RingLds;
template <typename Ring>
struct CompatStreamT {
    Ring r;  // 32 words: ring[31] + front index
    uint32_t gf, gr, x;
    // (cur: which of the handle's three stream buffers holds the committed streams, StepArgs::rng_cur)
    __device__ void load(const CompatRng &cr, int cur, int64_t env) {  // (RingGlobal)
        r.g = cr.g3[cur] + env * 32;
        gf = r.get(31);
        gr = (gf + 28u) % 31u;
        x = cr.minstd3[cur][env];
    }
    __device__ void store(const CompatRng &cr, int cur, int64_t env) {
        r.set(31, gf);
        cr.minstd3[cur][env] = x;
    }
    // glibc random_r TYPE_3: *f += *r; result = *f >> 1  (rand(), CHS.hpp:41)
    __device__ uint32_t rand31() {
        uint32_t v = r.get(gf) + r.get(gr);
        r.set(gf, v);
        gf = (gf + 1u == 31u) ? 0u : gf + 1u;
        gr = (gr + 1u == 31u) ? 0u : gr + 1u;
        return v >> 1;
    }
    __device__ int level() { return (int) (rand31() % 1000u); }
    // std::minstd_rand0 (CHS.hpp:25): x * 16807 mod (2^31 - 1).  2^31 = 1 (mod 2^31 - 1), so the 46-bit product folds as low 31 bits +
    // the rest, minus the modulus once if need be: the same residue as the 64-bit modulo (x is never 0: the modulus is prime)
    __device__ uint32_t minstd() {
        const uint64_t p = (uint64_t) x * 16807ull;
        uint32_t v = (uint32_t) (p & 0x7FFFFFFFull) + (uint32_t) (p >> 31);
        x = v >= 2147483647u ? v - 2147483647u : v;
        return x;
    }
    // libstdc++ generate_canonical<double,53>: two draws.  The division by the constant R * R is q = sum * RN(1 / (R * R)), one exact
    // residual, one correction (chub_curves.h, CHUB_DIV_K64): with the correctly rounded reciprocal and q within an ulp of the quotient that is the
    // correctly rounded quotient (Markstein 1990) -- 3 instructions instead of the ~35 of the f64 division sequence, twice per polar trial
    // on the walk's serial chain (tests/test_host_cpu.py checks the identity on 4e8 dividends of this shape on the CPU)
    __device__ double canon_d() {
        const double R = 2147483646.0;
        double sum = (double) (minstd() - 1u);
        sum += (double) (minstd() - 1u) * R;
        double ret = CHUB_DIV_K64(sum, R * R);
        if (ret >= 1.0) ret = 0.99999999999999988898;
        return ret;
    }
    // generate_canonical<float,24>: one draw (the division by 2^31 is the multiplication by 2^-31: exact scaling, nothing underflows)
    __device__ float canon_f() {
        float ret = __fmul_rn((float) (minstd() - 1u), 4.656612873077392578125e-10f);
        if (ret >= 1.0f) ret = 0.99999994f;
        return ret;
    }
    // std::normal_distribution<double>, fresh per call: polar, y*mult (CHS.hpp:805).  In two halves: polar_d is all that touches the stream
    // (the rejection loop: cheap, serial per env); normal_of_polar_d is the transform (f64 log, division, sqrt: a hundred-odd instructions that
    // depend on nothing but the accepted point) -- the dense stream walk (compat_walk_wave) runs the first half one env per lane and the
    // second one CAR per lane.  normal_d = both, back to back: the same operations in the same order, the same bits.
    __device__ void polar_d(double &y_, double &r2) {
        double x_;
        do {
            x_ = 2.0 * canon_d() - 1.0;
            y_ = 2.0 * canon_d() - 1.0;
            r2 = x_ * x_ + y_ * y_;
        } while (r2 > 1.0 || r2 == 0.0);
    }
    static __device__ __forceinline__ double normal_of_polar_d(double y_, double r2, double mean, double sd) {
        double mult = __dsqrt_rn(-2.0 * log(r2) / r2);
        return (y_ * mult) * sd + mean;
    }
    __device__ double normal_d(double mean, double sd) {
        double y_, r2;
        polar_d(y_, r2);
        return normal_of_polar_d(y_, r2, mean, sd);
    }
    // std::normal_distribution<float> (CHS.hpp:819,833).  logf is evaluated as the f32 rounding of the f64 log.
    __device__ void polar_f(float &y_, float &r2) {
        float x_;
        do {
            x_ = __fsub_rn(__fmul_rn(2.0f, canon_f()), 1.0f);
            y_ = __fsub_rn(__fmul_rn(2.0f, canon_f()), 1.0f);
            r2 = __fadd_rn(__fmul_rn(x_, x_), __fmul_rn(y_, y_));
        } while (r2 > 1.0f || r2 == 0.0f);
    }
    static __device__ __forceinline__ float normal_of_polar_f(float y_, float r2, float mean, float sd) {
        float lg = (float) log((double) r2);
        float mult = __fsqrt_rn(__fdiv_rn(__fmul_rn(-2.0f, lg), r2));
        return __fadd_rn(__fmul_rn(__fmul_rn(y_, mult), sd), mean);
    }
    __device__ float normal_f(float mean, float sd) {
        float y_, r2;
        polar_f(y_, r2);
        return normal_of_polar_f(y_, r2, mean, sd);
    }
};
typedef CompatStreamT<RingGlobal> CompatStream;

// ------------------------------------------------------------------------------- small arithmetic
// RandomUtil::uniform_rand(a, b) at level k (CHS.hpp:35-44): two f32 roundings after the division
__device__ __forceinline__ float uniform_level(int k, float a, float b) {
    float tr = __fdiv_rn((float) k, 999.0f);
    return __fadd_rn(__fmul_rn(tr, __fsub_rn(b, a)), a);
}

// calculate_needed (CHS.hpp:879-898 / 1044-1063) from the cached curve times
__device__ __forceinline__ float emergency_of(float t_target, float t_soc, int tl) {
    float need = __fsub_rn(t_target, t_soc);
    if (need > 0.0f) {
        if ((float) tl <= ceilf(need)) return 10.0f;
        float q = __fdiv_rn(need, (float) tl);
        return (float) ((double) q * (double) q);
    }
    return 0.0f;
}

// Both uses the step makes of the emergency -- force-on when emergency >= 1.01 (CHS.hpp:1406) and min_power when
// emergency > 8 (CHS.hpp:1248) -- reduce to the "must charge" branch: otherwise emergency = (need/left)^2 with
// left > ceil(need) >= need, i.e. < 1.  So the hot path only needs this predicate, no division.
__device__ __forceinline__ bool must_charge(float t_target, float t_soc, int tl) {
    // need > 0 && tl <= ceil(need) (CHS.hpp:883-890): for an integer tl >= 1, ceil(need) >= tl exactly when need > tl - 1 (both
    // sides are exact in f32), and that implies need > 0.  tl <= 0 does not occur: an empty slot is never asked.
    const float need = __fsub_rn(t_target, t_soc);
    return need > (float) (tl - 1);
}

__device__ __forceinline__ float arrive_soc_from(double normal73) {  // mk_soc, CHS.hpp:804-814
    float d = (float) normal73;
    if ((double) d < 1.0) d = 1.0f;
    else if ((double) d > 10.0) d = 10.0f;
    return (float) (75.0 - 5.0 * (double) d);
}

// popcount of the bits of m below this lane: two mbcnt instructions (no lane mask to build, no 64-bit and)
__device__ __forceinline__ int prefix_count(uint64_t m) {
    return (int) __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0u));
}

// XCD-aware work order.  The dispatcher hands workgroup b of a launch to XCD b % 8 (each XCD has its own L2); with this mapping XCD x works
// on ONE contiguous eighth of the launch's tiles (its b / 8-th) instead of on every eighth tile, so that neighbouring tiles -- which share
// cache lines at their borders -- share an L2 (slot kernel: L2 misses - 14 %, fabric writes - 11.5 %) and a CU touches one eighth of every
// array (vector-TLB misses 954 -> 0 per launch); nothing stays in L2 across kernel boundaries (profiles/round5_work_order_pmc.txt).  Measured (round 5, A/B inside one call,
// bit-identical; tiles, tail workgroups and level workgroups all in this order): cache-resident sizes gain 4-6 % of the step (C4 27.1 ->
// 25.95 us, 32 768 envs 18.3 -> 17.1, 8192 envs 10.8 -> 10.3, 131 072 envs 44.8 -> 43.8); the HBM-resident C5 LOSES 1 % (contiguous eighths
// concentrate each XCD's streams on fewer memory channels at a time), so handles beyond cache-resident sizes (chub_plan.h) keep the dispatcher's
// order (HubParams::xcd -> PackedArgs::xcd / TailArgs::xcd).
__device__ __forceinline__ uint32_t xcd_order(uint32_t b, uint32_t nb, uint32_t on) {
    if (!on) return b;
    const uint32_t q = nb >> 3, r = nb & 7u, x = b & 7u, i = b >> 3;
    return x * q + (x < r ? x : r) + i;
}

// Phase timestamps of measurement builds (KFLAGS=-DCHUB_TRACE=1; nothing in a product build): the shader clock when the wave gets here
// -- a stamp waits for scalar results only, so a phase's share shows where the wave stood, not what it overlapped
#if CHUB_TRACE
#define CHUB_STAMP_DECL(n) unsigned long long stamp_[n] = {}
#define CHUB_STAMP(i) do { unsigned long long t_; asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); stamp_[i] = t_; } while (0)
// ... and the constant 100 MHz clock all XCDs share (every XCD has a shader-clock counter of its own): calibrates the stamps' rate
#define CHUB_STAMP_REAL(i) do { unsigned long long t_; asm volatile("s_memrealtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); stamp_[i] = t_; } while (0)
#else
#define CHUB_STAMP_REAL(i) do {} while (0)
#define CHUB_STAMP_DECL(n) do {} while (0)
#define CHUB_STAMP(i) do {} while (0)
#endif
// action_to_real (MGR:384-393) switches a pile on iff (a + 1) / 2 >= 0.5 on the f32 array.  In round-to-nearest-even f32
// that is exactly a >= -2^-25 (a + 1 rounds to 1 from -2^-25 upwards, the tie going to the even 1.0; checked against the
// two-step form on every f32 around the threshold and a stride over all others), so one compare replaces add, mul, compare.
constexpr float kActOnThreshold = -2.98023223876953125e-8f;

// What k_slot hands to the per-env tail for one (station, env) unit: one 16-byte record.
struct StationRec {
    float mn, chg, mx;  // min_power, charge_power, max_power (CHS.hpp:1257-1259)
    uint32_t pkd;       // pkd_make(line, flow_in, car_number), chub_device.h
};
__device__ __forceinline__ void rec_store(CHUB_G(uint32_t) rec, uint32_t u, float mn, float chg, float mx, uint32_t pkd) {
    u32x4 v = {__float_as_uint(mn), __float_as_uint(chg), __float_as_uint(mx), pkd};
    *((CHUB_G(u32x4)) (rec + 4u * u)) = v;
}
__device__ __forceinline__ StationRec rec_load(CHUB_G(uint32_t) rec, uint32_t u) {
    const u32x4 v = *((CHUB_G(u32x4)) (rec + 4u * u));
    StationRec r;
    r.mn = __uint_as_float(v.x); r.chg = __uint_as_float(v.y); r.mx = __uint_as_float(v.z); r.pkd = v.w;
    return r;
}

// DPP lane exchanges for the (integer) butterfly sums of the wave-local kernel.  After the xor-1 and xor-2 steps every lane of a quad holds the quad's
// sum, so the mirror patterns (lane i <-> 7-i, i <-> 15-i) pair the same partial sums as xor 4 / xor 8 would.
__device__ __forceinline__ int dppi_xor1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true); }      // quad_perm [1,0,3,2]
__device__ __forceinline__ int dppi_xor2(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true); }      // quad_perm [2,3,0,1]
__device__ __forceinline__ int dppi_mirror8(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true); }  // row_half_mirror
__device__ __forceinline__ int dppi_mirror16(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true); } // row_mirror
// PHILOX-mode station sums are integer sums of slot powers in units of 2^-19 kW (see slot_body); back to kW in f32
__device__ __forceinline__ float fixed_to_kw(int v) { return (float) v * (1.0f / 524288.0f); }
// ... a slot power as that integer: the product with 2^19 is exact in f32, rounded to the nearest integer (ties to even), so a
// car's contribution is within 2^-20 kW of its f32 power and the error of a sum has no sign (round 3 truncated: up to 1.9e-6 kW
// per car, always downwards)
__device__ __forceinline__ int kw_to_fixed(float p) { return (int) rintf(p * 524288.0f); }

// PHILOX mode: mk_soc (CHS.hpp:804-814) from one 32-bit uniform by linear interpolation of the tabulated
// inverse CDF of clip(N(7,3),1,10): 12 bits pick the cell, 20 bits interpolate (three f32 roundings)
__device__ __forceinline__ float soc_from_word(const float *icdf, uint32_t w) {
    const uint32_t idx = w >> 20;
    const float frac = (float) (w & 0xFFFFFu) * (1.0f / 1048576.0f);
    const float a = icdf[idx], b = icdf[idx + 1];
    const float d = __fadd_rn(a, __fmul_rn(__fsub_rn(b, a), frac));
    return arrive_soc_from((double) d);
}
// PHILOX mode: mk_late_time (CHS.hpp:816-830) = #{j : w >= LT[j]} on the tabulated CDF of max(0, round(N(2,2)))
__device__ __forceinline__ int late_from_word(const uint32_t *thr, uint32_t w) {
    int late = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) late += (w >= thr[j]) ? 1 : 0;
    if (__any(w >= thr[7])) {  // the thresholds increase: beyond the 8th only with probability 0.3 %
#pragma unroll
        for (int j = 8; j < 16; j++) late += (w >= thr[j]) ? 1 : 0;
    }
    return late;
}

// PHILOX mode: N(0,1) from one 32-bit uniform by two-level tabulated inverse CDF (tools/gen_tables.py): 4096 cells,
// linear interpolation inside a cell; the lowest 16 cells (p < 2^-8: where the quantile function bends most) are refined by a
// second table with cells of 2^-20, the highest 16 are their mirror.
__device__ __forceinline__ float normal_from_word(const float *tz, const float *tl, uint32_t w) {
    const uint32_t cell = w >> 20;
    const bool hi = cell >= 4096u - 16u, lo = cell < 16u;
    const uint32_t m = hi ? ~w : w;  // tail: < 2^24
    const bool tail = hi || lo;
    const float *tab = tail ? tl : tz;
    const uint32_t idx = tail ? (m >> 12) : cell;
    const float frac = tail ? (float) (m & 0xFFFu) * (1.0f / 4096.0f) : (float) (w & 0xFFFFFu) * (1.0f / 1048576.0f);
    const float a = tab[idx], b = tab[idx + 1];
    const float z = __fadd_rn(a, __fmul_rn(__fsub_rn(b, a), frac));
    return hi ? -z : z;
}

// PHILOX: the station-level draws of receive_car (CHS.hpp:1272-1303 / 1583-1614) do not depend on state, only their
// use does: arrival count = table[slot of day][level]; queued car w stays iff level_w >= thr_renege[w]; arrival j stays
// iff level_j <= thr_balk[line + j], i.e. iff line <= inv_balk[level_j] - j (thr_balk is non-increasing).  So one lane
// per (station, env) unit draws them for the NEXT step, in extra blocks of the k_env launch.  Packed into 64 bits (the form
// chub_step_tape takes them in from the caller, pk_tape):
//   bits 0-9 renege pass bit per queue position, 10-13 arrivals n (<= 9), 14+4l (l = 0..10): how many of the n
//   arrivals stay (balk pass, incl. the j <= S guard) if the queue holds l cars after the renege pass.
// What those draws come to for a unit whose queue holds `line` cars (Station::line as the previous step left it): the renege
// pass over the queue (CHS.hpp:1286-1293), the arrivals, and -- slow station -- those of them that stay given the queue just
// thinned (CHS.hpp:1297-1306; the fast station records the un-thinned count, CHS.hpp:1617).  Decoded ONCE per unit, where the draws
// are made (one launch ahead), instead of by every lane of the unit in the slot kernel, which then only needs
//   assign = min(want, empties), line = min(want - assign, max_line)     (assign_car, CHS.hpp:417-430)
__device__ __forceinline__ uint32_t dk_make(uint64_t pk, int line, bool fast) {
    line = __popc((uint32_t) pk & ((1u << line) - 1u));
    const int n_in = (int) (pk >> 10) & 15;
    const int flow = fast ? n_in : (int) ((pk >> (14 + 4 * line)) & 15);
    return (uint32_t) (line + flow) | ((uint32_t) flow << 8);
}
// The same, drawn and decoded in one go where the queue length is known at draw time (the level blocks of k_env, k_draw_levels):
// only what this queue length needs -- `line` renege tests instead of all ten, the balk tests at ONE queue length instead of the
// whole table of eleven; the words: SITE_ARRIVE word 0 = arrival level, word 1 + j = balk level of arrival j; SITE_RENEGE word w = queue position w
__device__ __forceinline__ uint32_t draw_decoded_levels(const HubParams &hp, const Tables &tb, uint32_t tick, int t, int k, int64_t env,
                                                        int line, bool fast) {
    PhiloxCtx px{hp.key[0], hp.key[1], tick, (uint32_t) (hp.env_id0 + env)};
    const U4 a0 = px.block(SITE_ARRIVE, (uint32_t) k, 0);
    const U4 r0 = px.block(SITE_RENEGE, (uint32_t) k, 0);
    int n_in = (int) tb.cnt[k][t * kLevels + (int) (a0.v[0] % 1000u)];
    n_in = n_in > 9 ? 9 : n_in;
    uint32_t rw[10] = {r0.v[0], r0.v[1], r0.v[2], r0.v[3], 0u, 0u, 0u, 0u, 0u, 0u};
    if (__any(line > 4)) {  // the words of queue positions 4-9 only where some unit of the wave has such a queue
        const U4 r1 = px.block(SITE_RENEGE, (uint32_t) k, 1), r2 = px.block(SITE_RENEGE, (uint32_t) k, 2);
        rw[4] = r1.v[0]; rw[5] = r1.v[1]; rw[6] = r1.v[2]; rw[7] = r1.v[3]; rw[8] = r2.v[0]; rw[9] = r2.v[1];
    }
    int stay_q = 0;
#pragma unroll
    for (int w = 0; w < kMaxLine; w++) stay_q += (w < line && (int) (rw[w] % 1000u) >= (int) tb.thr_renege[w]) ? 1 : 0;
    int flow = n_in;
    if (!fast && __any(n_in > 0)) {  // the slow station records what survives the balk pass at the queue length just computed
        uint32_t bw[9] = {a0.v[1], a0.v[2], a0.v[3], 0u, 0u, 0u, 0u, 0u, 0u};
        if (__any(n_in > 3)) {
            const U4 a1 = px.block(SITE_ARRIVE, (uint32_t) k, 1), a2 = px.block(SITE_ARRIVE, (uint32_t) k, 2);
            bw[3] = a1.v[0]; bw[4] = a1.v[1]; bw[5] = a1.v[2]; bw[6] = a1.v[3]; bw[7] = a2.v[0]; bw[8] = a2.v[1];
        }
        const int S = hp.S[k];
        flow = 0;
#pragma unroll
        for (int j = 0; j < 9; j++) {
            if (j >= 3 && !__any(n_in > j)) break;
            const int top = (int) tb.inv_balk[bw[j] % 1000u] - j;  // arrival j stays iff line <= top (thr_balk is non-increasing)
            flow += (j < n_in && j <= S && stay_q <= top) ? 1 : 0;
        }
    }
    return (uint32_t) (stay_q + flow) | ((uint32_t) flow << 8);
}
// The same draws left RAW -- the 64-bit form above -- for a step whose queue length is not known yet at draw time: the second step of a pair whose
// tails share one launch (k_env_pair) is decoded by its own slot launch (dk_make in slot_body_packed's unit pass).  Same Philox sites and
// counters, same tables, same comparisons as draw_decoded_levels, so dk_make of this word gives that function's word bit for bit.  Lazy in
// the same way: the queue in front of that step holds at most qmax cars (the `want` of the step before it: line = min(want - assign,
// max_line)), and dk_make looks at renege bits below the queue length and at the balk entry of the thinned queue only, so the words of
// queue positions 4-9 are drawn only where some unit of the wave may queue that far, and the balk table is filled up to qmax.
__device__ __forceinline__ uint64_t draw_raw_levels(const HubParams &hp, const Tables &tb, uint32_t tick, int t, int k, int64_t env, int qmax,
                                                    bool fast) {
    PhiloxCtx px{hp.key[0], hp.key[1], tick, (uint32_t) (hp.env_id0 + env)};
    const U4 a0 = px.block(SITE_ARRIVE, (uint32_t) k, 0);
    const U4 r0 = px.block(SITE_RENEGE, (uint32_t) k, 0);
    int n_in = (int) tb.cnt[k][t * kLevels + (int) (a0.v[0] % 1000u)];
    n_in = n_in > 9 ? 9 : n_in;
    uint32_t rw[10] = {r0.v[0], r0.v[1], r0.v[2], r0.v[3], 0u, 0u, 0u, 0u, 0u, 0u};
    if (__any(qmax > 4)) {
        const U4 r1 = px.block(SITE_RENEGE, (uint32_t) k, 1), r2 = px.block(SITE_RENEGE, (uint32_t) k, 2);
        rw[4] = r1.v[0]; rw[5] = r1.v[1]; rw[6] = r1.v[2]; rw[7] = r1.v[3]; rw[8] = r2.v[0]; rw[9] = r2.v[1];
    }
    uint32_t ren = 0u;
#pragma unroll
    for (int w = 0; w < kMaxLine; w++) ren |= ((int) (rw[w] % 1000u) >= (int) tb.thr_renege[w]) ? (1u << w) : 0u;
    uint64_t pk = (uint64_t) (ren | ((uint32_t) n_in << 10));
    if (!fast && __any(n_in > 0)) {
        uint32_t bw[9] = {a0.v[1], a0.v[2], a0.v[3], 0u, 0u, 0u, 0u, 0u, 0u};
        if (__any(n_in > 3)) {
            const U4 a1 = px.block(SITE_ARRIVE, (uint32_t) k, 1), a2 = px.block(SITE_ARRIVE, (uint32_t) k, 2);
            bw[3] = a1.v[0]; bw[4] = a1.v[1]; bw[5] = a1.v[2]; bw[6] = a1.v[3]; bw[7] = a2.v[0]; bw[8] = a2.v[1];
        }
        const int S = hp.S[k];
        int top[9];  // arrival j stays iff the thinned queue holds at most top[j] cars (-1: never)
#pragma unroll
        for (int j = 0; j < 9; j++) top[j] = -1;
#pragma unroll
        for (int j = 0; j < 9; j++) {
            if (j >= 3 && !__any(n_in > j)) break;
            top[j] = (j < n_in && j <= S) ? (int) tb.inv_balk[bw[j] % 1000u] - j : -1;
        }
        const bool more3 = __any(n_in > 3);
#pragma unroll
        for (int l = 0; l <= kMaxLine; l++) {
            if (l > 0 && !__any(qmax >= l)) break;
            int c = (l <= top[0] ? 1 : 0) + (l <= top[1] ? 1 : 0) + (l <= top[2] ? 1 : 0);
            if (more3) {
#pragma unroll
                for (int j = 3; j < 9; j++) c += l <= top[j] ? 1 : 0;
            }
            pk |= (uint64_t) c << (14 + 4 * l);
        }
    }
    return pk;
}
__device__ __forceinline__ int dk_want(uint32_t dk) { return (int) (dk & 255u); }
__device__ __forceinline__ int dk_flow(uint32_t dk) { return (int) ((dk >> 8) & 255u); }

// ---------------------------------------------------------------------------------------- slot state
// The PHILOX state word (ps_*) and the COMPAT hot record's fourth word (hot_*) are laid out in chub_device.h.

// car_step (CHS.hpp:900-905 / 1065-1070): soc and power one slot further along the curve, evaluated together.  Same
// expressions as time_to_soc / time_to_power (chub_curves.h), but the powers of x are shared between the two
// polynomials and each transcendental branch is skipped when no lane of the wave is in its regime.
template <int TYPE>
__device__ __forceinline__ void car_step_curves(float tt, bool cp, const CurveConsts &cc, float &soc, float &power) {
    if (cp) {
        soc = time_to_soc<TYPE>(tt, cp, cc);
        power = time_to_power<TYPE>(tt, cp);
        return;
    }
    if (TYPE == 0) {
        const float xf = tt * 15.0f;
        const double x = xf, t = tt;
        const bool p1 = tt >= 0 && t < (28.7 / 15), p2 = tt >= 0 && t < (51.2 / 15);  // fast_time_to_power
        const bool s0 = tt <= 0, s1 = t <= 28.7 / 15, s2 = t <= 51.2 / 15;            // fast_time_to_soc
        float pw = 0.0f, sc = 100.0f;
        if (__any(p1 || (!s0 && s1))) {
            const double e = exp(0.053 * x);
            if (p1) pw = (float) (0.7194 * e + 47.78);
            if (!s0 && s1) sc = (float) ((0.7194 / 0.053) * e + 50.15 * x - (double) cc.fast_aa1_c) * cc.fast_soc_scale;
        }
        if (__any((!p1 && p2) || (!s0 && !s1 && s2))) {
            const double x2 = x * x, x3 = x2 * x, x4 = x2 * x2, x5 = x4 * x;
            if (!p1 && p2) pw = (float) (0.0002253 * x4 - 0.03572 * x3 + 2.016 * x2 - 48.76 * x + 457.7);
            if (!s0 && !s1 && s2)
                sc = (float) ((0.0002253 / 5) * x5 - (0.03572 / 4) * x4 + (2.016 / 3) * x3 - (48.76 / 2) * x2 + 457.7 * x +
                              (double) cc.fast_aa2_c) * cc.fast_soc_scale;
        }
        if (s0) sc = 0.0f;
        soc = sc;
        power = pw;
    } else {
        const float xf = tt / 4.0f;
        const double x = xf, t = tt;
        const bool p1 = t < 2.33 * 4, p2 = t < 3.67 * 4;                 // slow_time_to_power
        const bool c0 = tt <= 0, c1 = t <= 2.33 * 4, c2 = t <= 3.67 * 4; // slow_c_hole
        float pw = 0.0f, ch = cc.slow_c2_end;
        if (__any(p1 || (!c0 && c1))) {
            const double x2 = x * x, x3 = x2 * x, x4 = x2 * x2, x5 = x4 * x;
            if (p1) pw = (float) (-0.002056 * x4 + 0.00921 * x3 + 0.03562 * x2 + 0.02379 * x + 6.007);
            if (!c0 && c1)
                ch = (float) (-0.0004112 * x5 + 0.0023025 * x4 + (0.03562 / 3) * x3 + 0.011895 * x2 + 6.007 * x);
        }
        if (__any((!p1 && p2) || (!c0 && !c1 && c2))) {
            if (!p1 && p2) pw = (float) ((-4.041 * x + 21.1) / (x - 0.485));
            if (!c0 && !c1 && c2) ch = (float) (-4.041 * x + 19.140115 * log(fabs(x - 0.485)) + 11.943306312699628);
        }
        if (c0) ch = 0.0f;
        soc = (float) CHUB_DIV_K64((double) (100.0f * ch), 19.285746346634653);
        power = pw;
    }
}

// The COMPAT hot record as a whole (its words and the fourth word's bits: chub_device.h)
struct CompatSlot {
    float power, arr_soc, t_soc;
    int tl;       // stay left
    bool charge;  // charging this step
    int meta;
    static __device__ __forceinline__ CompatSlot unpack(const u32x4 h) {
        CompatSlot s;
        s.power = __uint_as_float(h.x); s.arr_soc = __uint_as_float(h.y); s.t_soc = __uint_as_float(h.z);
        s.tl = hot_tl(h.w);
        s.charge = (h.w & 128u) != 0u;
        s.meta = (int) (h.w >> 8);
        return s;
    }
    __device__ __forceinline__ u32x4 pack() const {
        return u32x4{__float_as_uint(power), __float_as_uint(arr_soc), __float_as_uint(t_soc),
                     (uint32_t) tl | (charge ? 128u : 0u) | ((uint32_t) meta << 8)};
    }
};

// What add_car (CHS.hpp:864-877 / 1029-1042) produces for one admitted slot.
struct NewCar {
    float soc, t_target, t_soc, power;
    int stay, lev;  // lev: target-SoC level, target = 80 + 20 * lev / 999 (CHS.hpp:35-44)
};

template <int TYPE>
__device__ __forceinline__ NewCar make_car(float arrive_soc, int lev, float t_target, int late, bool cp) {
    NewCar c;
    c.soc = arrive_soc;
    c.lev = lev;
    c.t_target = t_target;
    c.t_soc = soc_to_time<TYPE>(arrive_soc, cp);
    const float need = __fsub_rn(c.t_target, c.t_soc);
    int stay = (int) ceilf(need) + late;  // calculate_min_charging_time + mk_late_time
    c.stay = stay > 127 ? 127 : stay;
    c.power = time_to_power<TYPE>(c.t_soc, cp);
    return c;
}

// ------------------------------------------------------------------------------- the phases of the station step
// The reference's station step (CHS.hpp:1188-1207 / 1499-1518), one definition per phase.  The kernel forms below (wave-local units, a
// workgroup per unit, a unit in chunks, the split step and its walks) differ in how lanes map onto slots and in where a unit's state lives;
// the arithmetic of a phase is what stands here, and "the same draws in the same order, the same arithmetic: the same bits" holds
// between the forms because they call the same function.  (The packed production body, slot_body_packed, is a form of its own.)

// receive_car (CHS.hpp:1272-1316 / 1583-1627) ends in assign_car (CHS.hpp:417-430): of the `want` cars at the door (the queue that stayed +
// the arrivals recorded) as many as there are empty slots are admitted, the others queue up to max_line.  flow and assign may be negative
// right after the reset of a small fast station (CHS.hpp:1617): nobody is admitted then; a caller that stores assign clamps it itself.
struct Received {
    int flow, assign, line;  // flow_in_number.back(), cars admitted, Station::line
};
__device__ __forceinline__ Received assign_car(const int want, const int flow, const int empties) {
    Received r;
    r.flow = flow;
    r.assign = want < empties ? want : empties;
    const int line = want - r.assign;
    r.line = line < kMaxLine ? line : kMaxLine;
    return r;
}
// ... on the COMPAT streams, in the reference's consumption order: the initial occupancy (RESET: init_station_car_number, CHS.hpp:832-842) or
// the arrival count of the env's own slot of day, the renege pass over the queue, the balk pass over the arrivals.  line: the queue coming in
template <bool RESET, typename Stream>
__device__ __forceinline__ Received receive_car_streams(Stream &rs, const HubParams &hp, const StepArgs &sa, const Tables &tb, const int k,
                                                        const int env, const bool fast, const int line, const int empties) {
    const int S = hp.S[k], mu = S / 2;  // round(charge_number / 2) on ints, CHS.hpp:1276
    int n_in;
    if (RESET) {
        const int temp = (int) roundf(rs.normal_f((float) mu, 1.0f));
        n_in = temp > mu + 3 ? mu + 3 : (temp < mu - 3 ? mu - 3 : temp);
    } else {
        const int t_env = sa.env_clk ? clk_t(env_clk(sa, hp.n_envs, env)) : sa.t;  // per-env clocks: the env's own slot of day
        n_in = (int) tb.cnt[k][t_env * kLevels + rs.level()];
    }
    int stay_q = 0;
    for (int w = 0; w < line; w++) stay_q += (rs.level() >= (int) tb.thr_renege[w]) ? 1 : 0;
    int true_in = 0;
    for (int j = 0; j < n_in; j++) {
        const int m = stay_q + j;
        const int thr = (int) tb.thr_balk[m < kBalkTab ? m : kBalkTab - 1];
        true_in += (rs.level() <= thr && j <= S) ? 1 : 0;
    }
    const int flow = fast ? n_in : true_in;  // the fast station records the un-thinned count, CHS.hpp:1617 / 1306
    return assign_car(stay_q + flow, flow, empties);
}
// ... from PHILOX's station word: the unit's draws were made and decoded one launch ahead (draw_decoded_levels; RESET: the raw
// initial-occupancy draws of k_reset_levels, arrivals | arrivals that stay << 16)
template <bool RESET>
__device__ __forceinline__ Received receive_car_word(const uint32_t pk, const bool fast, const int empties) {
    if (RESET) {
        const int flow = fast ? (int) (int16_t) (pk & 0xFFFFu) : (int) ((pk >> 16) & 0xFFFFu);
        return assign_car(flow, flow, empties);
    }
    return assign_car(dk_want(pk), dk_flow(pk), empties);
}

// A new car's three variates from the COMPAT streams, in the reference's consumption order: mk_soc (CHS.hpp:804-814), the target level
// (CHS.hpp:35-44), mk_late_time("slow") (CHS.hpp:816-830)
struct CarDraw {
    float soc;
    int lev, late;
};
template <typename Stream>
__device__ __forceinline__ CarDraw draw_car_streams(Stream &rs) {
    CarDraw d;
    d.soc = arrive_soc_from(rs.normal_d(7.0, 3.0));
    d.lev = rs.level();
    const int late = (int) roundf(rs.normal_f(2.0f, 2.0f));
    d.late = late < 0 ? 0 : late;
    return d;
}
// ... and add_car (CHS.hpp:864-877 / 1029-1042) on the curves from them
__device__ __forceinline__ NewCar add_car_compat(const bool fast, const float soc, const int lev, const int late, const bool cp) {
    const float target = uniform_level(lev, 80.0f, 100.0f);
    NewCar nc;
    if (fast) nc = make_car<0>(soc, lev, soc_to_time<0>(target, cp), late, cp);
    else nc = make_car<1>(soc, lev, soc_to_time<1>(target, cp), late, cp);
    return nc;
}
__device__ __forceinline__ CompatSlot compat_slot_of(const NewCar &nc) {  // the hot record of a car that has just arrived
    CompatSlot s;
    s.power = nc.power; s.arr_soc = nc.soc; s.t_soc = nc.t_soc;
    s.tl = nc.stay;
    s.charge = false;
    s.meta = nc.stay | (nc.lev << 7);
    return s;
}

// PHILOX add_car (CHS.hpp:864-877 / 1029-1042): one Philox block per new car, keyed by (env, hub slot, tick) -- word 0 the SoC, word 1 the
// target level, word 2 the extra stay
__device__ __forceinline__ U4 car_block(const HubParams &hp, const StepArgs &sa, const int env, const int hub_slot) {
    PhiloxCtx px{hp.key[0], hp.key[1], CHUB_TICK(hp, sa.tick), (uint32_t) (hp.env_id0 + env)};
    return px.block(SITE_SOC, (uint32_t) hub_slot, 0);
}
struct PhiloxCar {
    float power, t_soc, t_target;
    int stay;
    uint32_t word;  // the slot's new state word (0: the car does not stay)
};
__device__ __forceinline__ PhiloxCar add_car_philox(const HubParams &hp, const StepArgs &sa, const Tables &tb, const int k, const int env,
                                                    const int hub_slot) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const U4 o = car_block(hp, sa, env, hub_slot);
    const uint32_t c = o.v[0] >> kSocLevelShift, lev = o.v[1] % 1000u;
    const f32x2 e0 = *(CHUB_G(const f32x2)) ((CHUB_G(const char)) tb.cls[k] + (size_t) c * (kClsRow * 8u));  // the class row's first entry
    PhiloxCar n;
    n.t_target = tb.ttab[k][lev];
    const int late = late_from_word(tb.late_thr, o.v[2]);
    const int stay = (int) ceilf(__fsub_rn(n.t_target, e0.y)) + late;  // calculate_min_charging_time + mk_late_time
    n.stay = stay > kMaxStay ? kMaxStay : stay;
    n.power = e0.x;
    n.t_soc = e0.y;
    n.word = n.stay > 0 ? ps_make(n.stay, c, lev) : 0u;
    return n;
}

// car_step (CHS.hpp:900-905 / 1065-1070) of a COMPAT slot that is on: one slot further along the curves
__device__ __forceinline__ void car_step_compat(CompatSlot &s, const bool fast, const bool cp, const CurveConsts &cc) {
    s.meta += kMetaStep;
    float soc_new;
    const float tt = __fadd_rn(s.t_soc, 1.0f);
    if (fast) {
        car_step_curves<0>(tt, cp, cc, soc_new, s.power);
        s.t_soc = soc_to_time<0>(soc_new, cp);
    } else {
        car_step_curves<1>(tt, cp, cc, soc_new, s.power);
        s.t_soc = soc_to_time<1>(soc_new, cp);
    }
}
// remove_car (CHS.hpp:912-923 / 1077-1088) of a COMPAT slot: one slot of stay less; a car whose stay is over leaves (returns true) and the
// record is wiped.  The charging flag is that of a car that is on AND stays.
__device__ __forceinline__ bool remove_car_compat(CompatSlot &s, const bool on) {
    bool leave = false;
    if (s.tl > 0) {
        s.tl -= 1;
        if (s.tl <= 0) {
            leave = true;
            s.tl = 0;
            s.power = s.t_soc = s.arr_soc = 0.0f;
            s.meta = 0;
        }
    }
    s.charge = on && s.tl > 0;
    return leave;
}
// car_step + remove_car on the PHILOX state word.  A car_step is one more entry along the class row, taken only by a car that stays: one
// that leaves this step is wiped right after its car_step (CHS.hpp:1196-1201).  The word's part alone (returns whether the car took the
// step) is all k_slot_unit_any's first pass needs; car_step_philox moves the slot's power and t_soc along with it and returns whether
// the car left, like remove_car_compat.
struct PhiloxWord {
    uint32_t w;
    int tl;       // stay left
    bool charge;  // charging this step
};
struct PhiloxSlot : PhiloxWord {
    float power, t_soc;
};
__device__ __forceinline__ bool car_step_word(PhiloxWord &s, const bool on) {
    const bool step = on && s.tl > 1;
    if (step) s.w += kPsStep;
    s.w &= ~kPsChg;
    if (s.tl > 0) {  // remove_car
        s.tl -= 1;
        s.w -= 1u;
        if (s.tl <= 0) {
            s.tl = 0;
            s.w = 0u;
        }
    }
    s.charge = on && s.tl > 0;
    if (s.charge) s.w |= kPsChg;
    return step;
}
__device__ __forceinline__ bool car_step_philox(PhiloxSlot &s, const bool on, const float next_power, const float next_t_soc) {
    const bool car = s.tl > 0;
    if (car_step_word(s, on)) {
        s.power = next_power;
        s.t_soc = next_t_soc;
    }
    const bool leave = car && s.tl == 0;
    if (leave) s.power = s.t_soc = 0.0f;
    return leave;
}
__device__ __forceinline__ PhiloxSlot philox_slot_of(const PhiloxCar &nc) {  // the slot of a car that has just arrived
    PhiloxSlot s;
    s.w = nc.word; s.tl = nc.stay; s.charge = false;
    s.power = nc.power; s.t_soc = nc.t_soc;
    return s;
}
// the slot value of a kernel that serves either state layout (both have power, t_soc, tl, charge)
template <int MODE> struct SlotOf { typedef CompatSlot type; };
template <> struct SlotOf<MODE_PHILOX> { typedef PhiloxSlot type; };

// Scalar-load control, evs_step(float) (CHS.hpp:1169-1186 / 1480-1497).  catch_load (CHS.hpp:358-366): the station's kW target, clamped to
// [min_power, max_power] of the previous calculate_output
__device__ __forceinline__ float catch_load(const HubParams &hp, const StepArgs &sa, const StationArrays &st, const int k, const int env,
                                            const uint32_t sidx) {
    const StationRec pr = rec_load(st.rec, sidx);
    float load = sa.actions[(uint32_t) env * (uint32_t) hp.act_dim + (uint32_t) (k ? hp.S[0] : 0)];
    if (load > pr.mx) load = pr.mx;
    else if (load < pr.mn) load = pr.mn;
    return load;
}
// ... and whether it switches on a car (assign_on_off, CHS.hpp:1318-1362 / 1629-1674) that has `mine_before` cars in front of it in urgency
// order and the cumulative power `mine` up to and including itself (rank_power_add, CHS.hpp:1375-1402): a constant-power fleet takes the
// first round(load / constant_power) cars, the others as many as the target covers
__device__ __forceinline__ bool load_says_on(const bool cp, const bool fast, const float load, const float mine, const int mine_before) {
    if (cp) {
        const int n_on = (int) roundf(__fdiv_rn(load, fast ? kFastConstantPower : kSlowConstantPower));
        return mine_before < n_on;
    }
    return (double) load + 0.0001 >= (double) mine;
}

// calculate_output (CHS.hpp:1233-1261 / 1544-1572), PHILOX: integer butterfly over a wave-local unit's H lanes (order-independent sums of
// slot powers in units of 2^-19 kW: kw_to_fixed)
__device__ __forceinline__ void unit_sums_dpp(const int H, int &i_min, int &i_max, int &i_chg) {
    if (H > 1) { i_min += dppi_xor1(i_min); i_max += dppi_xor1(i_max); i_chg += dppi_xor1(i_chg); }
    if (H > 2) { i_min += dppi_xor2(i_min); i_max += dppi_xor2(i_max); i_chg += dppi_xor2(i_chg); }
    if (H > 4) { i_min += dppi_mirror8(i_min); i_max += dppi_mirror8(i_max); i_chg += dppi_mirror8(i_chg); }
    if (H > 8) { i_min += dppi_mirror16(i_min); i_max += dppi_mirror16(i_max); i_chg += dppi_mirror16(i_chg); }
    if (H > 16) { i_min += __shfl_xor(i_min, 16); i_max += __shfl_xor(i_max, 16); i_chg += __shfl_xor(i_chg, 16); }
    if (H > 32) { i_min += __shfl_xor(i_min, 32); i_max += __shfl_xor(i_max, 32); i_chg += __shfl_xor(i_chg, 32); }
}
// ... one lane adding n slots' terms in LDS to its running sums, in slot order.  COMPAT: the reference's sequential f32 sums
// (CHS.hpp:1244-1255), same order, same roundings; PHILOX: 64-bit integers, one rounding to f32 at the end (fixed64_to_kw)
struct SumsF32 {
    float mn, chg, mx;
    __device__ __forceinline__ void add(const float *t_min, const float *t_chg, const float *t_max, const int n) {
        for (int i = 0; i < n; i++) {
            mx = __fadd_rn(mx, t_max[i]);
            mn = __fadd_rn(mn, t_min[i]);
            chg = __fadd_rn(chg, t_chg[i]);
        }
    }
};
struct SumsI64 {
    long long mn, chg, mx;
    __device__ __forceinline__ void add(const uint32_t *t_min, const uint32_t *t_chg, const uint32_t *t_max, const int n) {
        for (int i = 0; i < n; i++) {
            mn += (long long) (int) t_min[i];
            chg += (long long) (int) t_chg[i];
            mx += (long long) (int) t_max[i];
        }
    }
};
__device__ __forceinline__ float fixed64_to_kw(long long v) { return (float) v * (1.0f / 524288.0f); }

// ---- scalar-load control mode, evs_step(float) (CHS.hpp:1169-1186 / 1480-1497): one kW target per station; the piles are
// switched on in urgency order until the target is met (assign_on_off, CHS.hpp:1318-1362 / 1629-1674).  Wave-local units
// (H = pow2 >= S lanes).  Returns this lane's on / off decision.
template <int BLOCK>
__device__ __forceinline__ bool load_mode_on(const HubParams &hp, const StepArgs &sa, const StationArrays &st, const int k,
                                             const int env, const bool unit_ok, const bool valid, const int slot, const bool car0,
                                             const float pw0, const float em0, float *lds_f, uint32_t *lds_u, const int ubase) {
    const int wave = threadIdx.x >> 6;
    const int S = hp.S[k];
    const uint32_t sidx = (uint32_t) k * (uint32_t) hp.n_envs + (uint32_t) env;
    const bool cp = hp.constant_charging != 0;
    const float load = unit_ok ? catch_load(hp, sa, st, k, env, sidx) : 0.0f;
    // std::multimap keyed by -emergency (CHS.hpp:1324-1336): emergency descending, ties by slot index (ubase: the unit's first lane)
    int rk = 0;
    for (int j = 0; j < S; j++) {
        const float ej = __shfl(em0, ubase + j);
        rk += (ej > em0 || (ej == em0 && j < slot)) ? 1 : 0;
    }
    // rank_power_add (CHS.hpp:1375-1402): cumulative power of the cars in that order, added sequentially in f32
    float *by_rank = lds_f + wave * 64 + ubase;          // this unit's H floats
    uint32_t *car_by_rank = lds_u + wave * 64 + ubase;
    if (valid) {
        by_rank[rk] = car0 ? pw0 : 0.0f;
        car_by_rank[rk] = car0 ? 1u : 0u;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float cum = 0.0f, mine = 0.0f;
    int cars_before = 0, mine_before = 0;
    for (int q = 0; q < S; q++) {
        if (q == rk) mine_before = cars_before;
        cum = __fadd_rn(cum, valid ? by_rank[q] : 0.0f);
        cars_before += valid ? (int) car_by_rank[q] : 0;
        if (q == rk) mine = cum;
    }
    const bool chg = car0 && load_says_on(cp, hp.type[k] == 0, load, mine, mine_before);
    __builtin_amdgcn_wave_barrier();
    __syncthreads();  // the scratch areas are reused below
    return chg;
}

// ---------------------------------------------------------------------------------------- k_slot, COMPAT streams
// lane = charger slot; one (env, station) unit = H = pow2 >= S_k lanes, 64 / H units per wave.  Phases in the reference's order
// (CHS.hpp:1188-1207 / 1499-1518).  The unit's first lane walks the env's two reference streams in the reference's
// consumption order; station sums in the reference's sequential f32 order.  Pinned against the recorded reference
// trajectories (tests/golden).
// SPLIT (the split step of large batches): the walk was done by k_compat_walk, one ENV per lane (here one lane per UNIT walks while
// the other lanes of the wave idle); this body then only fetches what it came to -- flow, cars admitted, queue -- and the admitted
// lanes their car's variates (the phases: receive_car_streams, draw_car_streams, add_car_compat above).
// wave0 / mid (k_compat_small): the station's units start at workgroup wave `wave0`, and mid() is called by every lane in front of the
// first look at what the walk came to (there: the workgroup barrier behind which the walker wave's results are in).
struct NoSlotMid {
    __device__ __forceinline__ void operator()() {}
};
template <int TYPE, bool RESET, int BLOCK, bool SPLIT = false, typename SlotMid = NoSlotMid>
__device__ __forceinline__ void slot_body_compat(const HubParams &hp, const StepArgs &sa, const SlotArrays &sl, const StationArrays &st,
                                 const CompatRng &cr, const Tables &tb, const int k, const int64_t block_local,
                                 float *lds_f, uint32_t *lds_u, const int wave0 = 0, SlotMid mid = SlotMid()) {
    constexpr int WAVES = BLOCK / 64;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave_abs = tid >> 6, wave = wave_abs - wave0;  // wave: among the station's waves (env mapping); wave_abs: the LDS areas
    // a unit takes U = S lanes (1 for a station without piles), floor(64 / U) units per wave, the rest of the wave idle: 3 units of 20
    // piles or 2 of 25 per wave (units of the next power of two left 38 % / 22 % of the lanes idle)
    const int U = hp.U[k], S = hp.S[k];
    const int upw = 64 / U;
    const int uiw = lane / U;
    const int slot = lane - uiw * U;
    const int64_t N = hp.n_envs;
    // 32-bit indices: n_envs * (piles + 2) < 2^31 is checked at create
    const int env_first = (int) block_local * (WAVES * upw);
    const int env = env_first + wave * upw + uiw;
    const bool unit_ok = uiw < upw && env < (int) N && in_group(sa, env);
    const bool valid = unit_ok && slot < S;
    const int leader = uiw < upw ? uiw * U : 63;  // the unit's first lane
    const uint64_t unit_mask = (U == 64) ? ~0ull : (uiw < upw ? (((1ull << U) - 1ull) << leader) : 0ull);
    const uint32_t idx = (uint32_t) hp.base[k] + (uint32_t) env * (uint32_t) S + (uint32_t) slot;
    const uint32_t sidx = (uint32_t) k * (uint32_t) N + (uint32_t) env;
    const int hub_slot = (k ? hp.S[0] : 0) + slot;
    const bool cp = hp.constant_charging != 0;

    // the unit's queue length, the slot's hot record and its action go out together (one memory round trip)
    uint32_t line_in = 0;
    u32x4 hot = {0u, 0u, 0u, 0u};
    float a = 0.0f;
    if (!RESET && unit_ok) line_in = st.rec[4u * sidx + 3u];
    if (!RESET && valid) {
        hot = ((CHUB_G(u32x4)) sl.hot)[idx];
        a = sa.actions[(uint32_t) env * (uint32_t) hp.act_dim + (uint32_t) hub_slot];
    }
    CompatSlot s = CompatSlot::unpack(hot);
    bool car = s.tl > 0;
    float t_target = car ? tb.ttab[k][hot_level(hot.w)] : 0.0f;  // soc_to_time(target) of the car's level
    int on_override = -1;
    if (!RESET && sa.load_mode)
        on_override = load_mode_on<BLOCK>(hp, sa, st, k, env, unit_ok, valid, slot, car, s.power,
                                          car ? emergency_of(t_target, s.t_soc, s.tl) : 0.0f, lds_f, lds_u, leader) ? 1 : 0;
    // judge_feasibility + assign_on_off_piece (CHS.hpp:1404-1413, 1364-1373); action_to_real (MGR:384-393)
    const bool on = on_override >= 0 ? (car && on_override != 0) : (car && (a >= kActOnThreshold || must_charge(t_target, s.t_soc, s.tl)));
    if (on) car_step_compat(s, TYPE == 0, cp, hp.cc);
    const bool leave = remove_car_compat(s, on);
    if (leave) t_target = 0.0f;
    car = s.tl > 0;

    // ---- receive_car: arrivals, renege, balk, admission
    const bool empty = valid && !car;
    const uint64_t be = __ballot(empty) & unit_mask;
    const int empties = __popcll(be);
    const int rank = prefix_count(be);
    int line = pkd_line(line_in);
    // the unit's first lane walks the two reference streams in the reference's order and parks the per-admission
    // variates in LDS, indexed by admission rank
    float *lds_soc = lds_f;
    uint32_t *lds_lev = lds_u, *lds_late = lds_u + BLOCK;
    const int lbase = wave_abs * 64 + leader;
    int2 fa = make_int2(0, 0);
    int new_line = line;
    if (SPLIT) {
        mid();
        if (unit_ok && slot == 0) {
            const uint32_t w = st.fa[sa.tick & 1u][sidx];
            fa = make_int2((int) (int16_t) (w & 0xFFFFu), (int) ((w >> 16) & 255u));
            new_line = (int) (w >> 24);
        }
    } else if (unit_ok && slot == 0) {
        CompatStream rs;
        rs.load(cr, sa.rng_cur, env);
        const Received rc = receive_car_streams<RESET>(rs, hp, sa, tb, k, env, TYPE == 0, line, empties);
        new_line = rc.line;
        for (int rr = 0; rr < rc.assign; rr++) {  // ascending slot order == ascending rank
            const CarDraw d = draw_car_streams(rs);
            lds_soc[lbase + rr] = d.soc;
            lds_lev[lbase + rr] = (uint32_t) d.lev;
            lds_late[lbase + rr] = (uint32_t) d.late;
        }
        rs.store(cr, sa.rng_cur, env);
        fa = make_int2(rc.flow, rc.assign);
    }
    const int flow = __shfl(fa.x, leader);
    const int assign = __shfl(fa.y, leader);
    line = __shfl(new_line, leader);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const bool adm = empty && rank < assign;
    if (adm && SPLIT) {  // the car as the walk made it (compat_walk_env: add_car there, one record per admission rank)
        const uint32_t vi = (uint32_t) env * (uint32_t) (hp.S[0] + hp.S[1]) + (uint32_t) (k ? hp.S[0] : 0) + (uint32_t) rank;
        const u32x4 vv = ((CHUB_G(const u32x4)) sl.var[sa.tick & 1u])[2u * vi];
        s.arr_soc = __uint_as_float(sl.var[sa.tick & 1u][8u * vi + 4u]);
        s.power = __uint_as_float(vv.x);
        t_target = __uint_as_float(vv.y);
        s.t_soc = __uint_as_float(vv.z);
        s.tl = (int) (vv.w & 127u);
        s.meta = (int) vv.w;
    } else if (adm) {
        const NewCar nc = add_car_compat(TYPE == 0, lds_soc[lbase + rank], (int) lds_lev[lbase + rank], (int) lds_late[lbase + rank], cp);
        t_target = nc.t_target;
        s = compat_slot_of(nc);
    } else if (leave || RESET) {
        s.meta = 0;
    }
    car = s.tl > 0;

    // ---- calculate_output (CHS.hpp:1233-1261 / 1544-1572): SumsF32
    const bool urgent = car && must_charge(t_target, s.t_soc, s.tl);
    const float v_min = urgent ? s.power : 0.0f, v_max = car ? s.power : 0.0f, v_chg = s.charge ? s.power : 0.0f;
    // every lane parks its three terms in the wave's own scratch area and the unit's first lane -- the only one that needs the sums --
    // adds them up in slot order (each lane fetching its S neighbours' terms by cross-lane reads cost 3 S of those per wave)
    SumsF32 r = {0.0f, 0.0f, 0.0f};
    {
        __builtin_amdgcn_wave_barrier();  // (the admitted lanes' reads of the walk's variates above are done)
        float *t_max = lds_f + wave_abs * 64, *t_min = (float *) lds_u + wave_abs * 64, *t_chg = (float *) lds_u + BLOCK + wave_abs * 64;
        t_max[lane] = v_max;
        t_min[lane] = v_min;
        t_chg[lane] = v_chg;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (unit_ok && slot == 0) r.add(t_min + leader, t_chg + leader, t_max + leader, S);
    }
    const int cars = __popcll(__ballot(car) & unit_mask);

    if (valid) ((CHUB_G(u32x4)) sl.hot)[idx] = s.pack();
    if (unit_ok && slot == 0) {
        rec_store(st.rec, sidx, r.mn, r.chg, r.mx, pkd_make(line, flow, cars));
    }
    if (SPLIT) {  // what the next step's walk needs of the slots: a slot is empty after remove_car iff it has at most one slot of stay left
        const int n_empty = __popcll(__ballot(valid && s.tl <= 1) & unit_mask), n_empty2 = __popcll(__ballot(valid && s.tl <= 2) & unit_mask);
        if (unit_ok && slot == 0) {
            st.empt[sidx] = (uint8_t) n_empty;
            st.empt2[sa.tick & 1u][sidx] = (uint8_t) n_empty2;
        }
        // (the step's draws are now taken: the buffer the walk left the streams' state in becomes the committed one -- on the host, by
        // moving StepArgs::rng_cur on: no copy)
    }
}

// ---------------------------------------------------------------------------------------- the split step's slot pass, two units' worth per lane
// slot_body_compat<.., SPLIT> spends its instructions on lanes that sit idle: the f64 curve work of car_step is needed by the third of
// the lanes whose car charges, add_car's by one lane in fifteen, and the sequential f32 sums by one lane per unit -- but a wave pays
// for each in full.  Here a lane carries TWO slots (virtual waves 2w and 2w + 1 of the same station), and those three pieces are done
// ONCE per wave for both: the charging lanes' inputs of both virtual waves are packed into the wave's own LDS area by ballot ranks (42 of
// 128 on average: one pass), evaluated by lanes 0 .. n - 1 with the same device functions -- the same bits -- and picked up again;
// likewise the new cars; and lane 2 * unit + v adds up the terms of unit `unit` of virtual wave v, so one loop serves both.  No
// workgroup barrier anywhere (the gathering across a WORKGROUP's waves lost to its barriers).  Lock-step and
// masked steps without the scalar-load mode; everything else keeps slot_body_compat.
template <int TYPE, int BLOCK>
__device__ __forceinline__ void slot_body_split2(const HubParams &hp, const StepArgs &sa, const SlotArrays &sl, const StationArrays &st,
                                                 const CompatRng &cr, const Tables &tb, const int k, const int64_t block_local, float *lds) {
    constexpr int WAVES = BLOCK / 64;
    constexpr int kArea = 3 * 128 + 16;  // per wave: three arrays of 128 terms (aliased by the gathering areas) + the units' words
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    // Units are laid end to end over the wave's 128 VIRTUAL lanes v = 64 j + lane (j = the lane's first / second slot): floor(128 / U) units per
    // wave -- 5 stations of 25 piles instead of the 2 x 2 that fit when a unit had to stay inside one virtual wave (round 6: a fifth of the
    // slow station's waves gone), 6 of 20 as before.  At most one unit straddles the two virtual waves; its ranks and counts take both ballots.
    const int U = hp.U[k], S = hp.S[k];
    const int upp = 128 / U;  // units per wave (U >= 8 here: at most 16)
    const uint32_t umagic = 65536u / (uint32_t) U + 1u;  // v / U = (v * umagic) >> 16, exact for v < 128 (the error term v / 65536 < 1 / U)
    const int N = (int) hp.n_envs;
    const int env_first = (int) block_local * (WAVES * upp);
    const uint32_t St = (uint32_t) (hp.S[0] + hp.S[1]);
    const bool cp = hp.constant_charging != 0;
    float *wl = lds + wave * kArea;
    uint32_t *wu = (uint32_t *) wl;

    int env[2], uiw[2], slot[2];
    bool unit_ok[2], valid[2];
    uint32_t idx[2], sidx[2], fa_w[2];
    uint64_t m_same[2], m_other[2];  // the unit's lanes in the lane's own virtual wave / in the other one
    int lead_lane[2], lead_j[2];     // where the unit's first virtual lane sits
    u32x4 hot[2];
    float a[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int v = 64 * j + lane;
        uiw[j] = (int) (((uint32_t) v * umagic) >> 16);
        slot[j] = v - uiw[j] * U;
        const int ua = uiw[j] * U, ub = ua + U;  // the unit's virtual lanes [ua, ub)
        const bool has = uiw[j] < upp;
        lead_lane[j] = has ? (ua & 63) : 63;
        lead_j[j] = ua >> 6;
        if (j == 0) {  // (ua < 64)
            const int hi = ub < 64 ? ub : 64;
            m_same[j] = has ? ((hi == 64 ? ~0ull : ((1ull << hi) - 1ull)) & ~((1ull << ua) - 1ull)) : 0ull;
            m_other[j] = (has && ub > 64) ? ((1ull << (ub - 64)) - 1ull) : 0ull;
        } else {       // (ub > 64)
            const int lo = ua > 64 ? ua - 64 : 0, hi = ub - 64 < 64 ? ub - 64 : 64;
            m_same[j] = has ? ((hi == 64 ? ~0ull : ((1ull << hi) - 1ull)) & ~((1ull << lo) - 1ull)) : 0ull;
            m_other[j] = (has && ua < 64) ? (~0ull << ua) : 0ull;
        }
        env[j] = env_first + wave * upp + uiw[j];
        unit_ok[j] = has && env[j] < N && in_group(sa, env[j]);
        valid[j] = unit_ok[j] && slot[j] < S;
        idx[j] = (uint32_t) hp.base[k] + (uint32_t) env[j] * (uint32_t) S + (uint32_t) slot[j];
        sidx[j] = (uint32_t) k * (uint32_t) N + (uint32_t) env[j];
        hot[j] = u32x4{0u, 0u, 0u, 0u};
        a[j] = 0.0f;
        fa_w[j] = 0u;
        if (unit_ok[j] && slot[j] == 0) fa_w[j] = st.fa[sa.tick & 1u][sidx[j]];  // what the walk came to (flow_in, cars admitted, queue): with the first loads
        if (valid[j]) {
            hot[j] = ((CHUB_G(u32x4)) sl.hot)[idx[j]];
            a[j] = sa.actions[(uint32_t) env[j] * (uint32_t) hp.act_dim + (uint32_t) ((k ? hp.S[0] : 0) + slot[j])];
        }
    }
    float power[2], t_target[2], t_soc[2], arr_soc[2];
    int tl[2], meta[2];
    bool car[2], leave[2], on[2], charge[2];
    CHUB_G(const float) ttab_k = tb.ttab[k];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        power[j] = __uint_as_float(hot[j].x);
        arr_soc[j] = __uint_as_float(hot[j].y);
        t_soc[j] = __uint_as_float(hot[j].z);
        tl[j] = hot_tl(hot[j].w);
        meta[j] = (int) (hot[j].w >> 8);
        car[j] = tl[j] > 0;
        t_target[j] = car[j] ? ttab_k[hot_level(hot[j].w)] : 0.0f;  // soc_to_time(target) of the car's level (hot_level)
        leave[j] = false;
        // judge_feasibility + assign_on_off_piece (CHS.hpp:1404-1413, 1364-1373); action_to_real (MGR:384-393)
        on[j] = car[j] && (a[j] >= kActOnThreshold || must_charge(t_target[j], t_soc[j], tl[j]));
    }
    // ---- receive_car (CHS.hpp:1272-1316 / 1583-1627), ahead of car_step: who leaves depends on the stay alone (remove_car, CHS.hpp:912-923 /
    // 1077-1088), so the empties, the ranks and who is admitted are known here, and the new cars' variates (the walk's) are requested
    // BEFORE the curve work instead of behind it
    bool empty[2], adm[2];
    int rank[2], line[2], flow[2], assign[2];
    u32x4 vv[2];
    float nc_soc[2];
    uint64_t be[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        empty[j] = valid[j] && !(car[j] && tl[j] > 1);
        be[j] = __ballot(empty[j]);
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
        // rank = the unit's empties in front of this lane: those of its own virtual wave below it, + (second virtual wave of a straddling
        // unit) all of the unit's empties in the first
        rank[j] = prefix_count(be[j] & m_same[j]) + (j == 1 ? __popcll(be[0] & m_other[1]) : 0);
        // the walk's word of the unit (flow_in, cars admitted, queue), from the unit's first virtual lane -- which for a lane's first slot is
        // in the first virtual wave, for its second slot in either
        const uint32_t w0 = (uint32_t) __shfl((int) fa_w[0], lead_lane[j]);
        uint32_t w = w0;
        if (j == 1) {
            const uint32_t w1 = (uint32_t) __shfl((int) fa_w[1], lead_lane[j]);
            w = lead_j[j] ? w1 : w0;
        }
        flow[j] = (int) (int16_t) (w & 0xFFFFu);
        assign[j] = (int) ((w >> 16) & 255u);
        line[j] = (int) (w >> 24);
        adm[j] = empty[j] && rank[j] < assign[j];
        vv[j] = u32x4{0u, 0u, 0u, 0u};
        nc_soc[j] = 0.0f;
        if (adm[j]) {  // the new car as the walk made it (add_car in compat_walk_env): requested here, picked up behind the curve work
            const uint32_t vi = (uint32_t) env[j] * St + (uint32_t) (k ? hp.S[0] : 0) + (uint32_t) rank[j];
            vv[j] = ((CHUB_G(const u32x4)) sl.var[sa.tick & 1u])[2u * vi];  // (the record's two 16-byte halves share a 32-byte sector)
            nc_soc[j] = __uint_as_float(sl.var[sa.tick & 1u][8u * vi + 4u]);
        }
    }
    // ---- car_step (CHS.hpp:900-905 / 1065-1070) of both virtual waves' charging cars, packed
    {
        const uint64_t b0 = __ballot(on[0]), b1 = __ballot(on[1]);
        const int n0 = __popcll(b0), n1 = __popcll(b1);
        if (n0 + n1 <= 64) {
            float *g_in = wl, *g_pw = wl + 64, *g_ts = wl + 128;
            const int p0 = prefix_count(b0), p1 = n0 + prefix_count(b1);
            if (on[0]) g_in[p0] = __fadd_rn(t_soc[0], 1.0f);
            if (on[1]) g_in[p1] = __fadd_rn(t_soc[1], 1.0f);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (lane < n0 + n1) {
                float soc_new, pw;
                car_step_curves<TYPE>(g_in[lane], cp, hp.cc, soc_new, pw);
                g_pw[lane] = pw;
                g_ts[lane] = soc_to_time<TYPE>(soc_new, cp);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (on[0]) { power[0] = g_pw[p0]; t_soc[0] = g_ts[p0]; }
            if (on[1]) { power[1] = g_pw[p1]; t_soc[1] = g_ts[p1]; }
            __builtin_amdgcn_wave_barrier();
        } else {  // (more than half of the slots charge: each virtual wave for itself)
#pragma unroll
            for (int j = 0; j < 2; j++)
                if (on[j]) {
                    float soc_new;
                    car_step_curves<TYPE>(__fadd_rn(t_soc[j], 1.0f), cp, hp.cc, soc_new, power[j]);
                    t_soc[j] = soc_to_time<TYPE>(soc_new, cp);
                }
        }
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
        if (on[j]) meta[j] += kMetaStep;  // one more car_step on this car's account (its SoC is replayed from it on demand)
        if (car[j]) {  // remove_car (CHS.hpp:912-923 / 1077-1088)
            tl[j] -= 1;
            if (tl[j] <= 0) {
                car[j] = false;
                leave[j] = true;
                tl[j] = 0;
                power[j] = t_target[j] = t_soc[j] = arr_soc[j] = 0.0f;
                meta[j] = 0;
            }
        }
        charge[j] = on[j] && car[j];
    }
    // ---- add_car (CHS.hpp:864-877 / 1029-1042): the walk evaluated it (one record per admission rank); the admitted lanes take theirs
#pragma unroll
    for (int j = 0; j < 2; j++) {
        if (adm[j]) {
            power[j] = __uint_as_float(vv[j].x);
            t_target[j] = __uint_as_float(vv[j].y);
            t_soc[j] = __uint_as_float(vv[j].z);
            tl[j] = (int) (vv[j].w & 127u);
            car[j] = tl[j] > 0;
            meta[j] = (int) vv[j].w;
        } else if (leave[j]) {
            meta[j] = 0;
        }
    }
    // ---- calculate_output (CHS.hpp:1233-1261 / 1544-1572): the reference adds slot powers sequentially in f32 (CHS.hpp:1244-1255):
    // same order, same roundings -- one lane per unit and term adds up the unit's S terms, which lie side by side in the 128 virtual lanes
    float *t_max = wl, *t_min = wl + 128, *t_chg = wl + 256;
    uint32_t *u_word = wu + 384;  // [unit]: line | flow | cars of the unit (pkd_make)
    {
        const uint64_t bc0 = __ballot(car[0]), bc1 = __ballot(car[1]);
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const bool urgent = car[j] && must_charge(t_target[j], t_soc[j], tl[j]);
            t_max[j * 64 + lane] = car[j] ? power[j] : 0.0f;
            t_min[j * 64 + lane] = urgent ? power[j] : 0.0f;
            t_chg[j * 64 + lane] = charge[j] ? power[j] : 0.0f;
            const int cars = __popcll((j ? bc1 : bc0) & m_same[j]) + __popcll((j ? bc0 : bc1) & m_other[j]);
            if (unit_ok[j] && slot[j] == 0) u_word[uiw[j]] = pkd_make(line[j], flow[j], cars);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // (one lane per unit AND term: lane 16 * term + unit -- a loop of S additions instead of 3 S; each lane stores its own word of the unit's
    // record: min, charge, max power in that order, the first of them the packed word behind)
    if (lane < 48 && (lane & 15) < upp) {
        const int term = lane >> 4, un = lane & 15;
        const int e = env_first + wave * upp + un;
        if (e < N && in_group(sa, e)) {
            const float *t = (term == 0 ? t_min : (term == 1 ? t_chg : t_max)) + un * U;
            float r = 0.0f;
            for (int i = 0; i < S; i++) r = __fadd_rn(r, t[i]);
            const uint32_t u = (uint32_t) k * (uint32_t) N + (uint32_t) e;
            st.rec[4u * u + (uint32_t) term] = __float_as_uint(r);
            if (term == 0) st.rec[4u * u + 3u] = u_word[un];
        }
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
        if (valid[j]) {
            u32x4 h2;
            h2.x = __float_as_uint(power[j]);
            h2.y = __float_as_uint(adm[j] ? nc_soc[j] : arr_soc[j]);  // the arrival SoC
            h2.z = __float_as_uint(t_soc[j]);
            h2.w = (uint32_t) tl[j] | (charge[j] ? 128u : 0u) | ((uint32_t) meta[j] << 8);
            // (the record goes back whole: storing only the words that changed -- 4 bytes for a car that neither charged, left nor arrived, nothing for
            // an empty slot -- was measured in round 6: the launch 49.6 -> 59 us, WRITE_SIZE 80 -> 100 MiB, FETCH_SIZE 54 -> 69 MiB: a partly
            // written sector costs a read-modify-write)
            ((CHUB_G(u32x4)) sl.hot)[idx[j]] = h2;
        }
    }
    {   // what the next step's walk needs of the slots: a slot is empty after remove_car iff it has at most one slot of stay left
        const uint64_t e1[2] = {__ballot(valid[0] && tl[0] <= 1), __ballot(valid[1] && tl[1] <= 1)};
        const uint64_t e2[2] = {__ballot(valid[0] && tl[0] <= 2), __ballot(valid[1] && tl[1] <= 2)};
#pragma unroll
        for (int j = 0; j < 2; j++) {
            if (unit_ok[j] && slot[j] == 0) {  // (the unit's first virtual lane: its own virtual wave's part + the other's)
                st.empt[sidx[j]] = (uint8_t) (__popcll(e1[j] & m_same[j]) + __popcll(e1[1 - j] & m_other[j]));
                st.empt2[sa.tick & 1u][sidx[j]] = (uint8_t) (__popcll(e2[j] & m_same[j]) + __popcll(e2[1 - j] & m_other[j]));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------- k_slot, PHILOX, wave-local units
// The same phases on the 4-byte PHILOX slot state for what the packed kernel below does not cover: the scalar-load control mode
// (and every step of a handle created with chub_options.slot_kernel = 1: the parity cross-check).  One unit = H = pow2 >= S_k lanes of one wave: ballot + prefix rank inside the wave,
// integer DPP butterfly for the station sums.  Bit for bit the packed kernel's results (test_philox_other_slot_kernel runs
// every step through this one).
template <bool RESET, int BLOCK>
__device__ void slot_body_wave(const HubParams &hp, const StepArgs &sa, const SlotArrays &sl, const StationArrays &st,
                               const Tables &tb, const int k, const int64_t block_local, float *lds_f, uint32_t *lds_u) {
    constexpr int WAVES = BLOCK / 64;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int H = hp.H[k], S = hp.S[k], logH = hp.logH[k];
    const int upw = 64 >> logH;
    const int uiw = lane >> logH;
    const int slot = lane & (H - 1);
    const int64_t N = hp.n_envs;
    const int env_first = (int) block_local * (WAVES * upw);
    const int env = env_first + wave * upw + uiw;
    const bool unit_ok = env < (int) N && in_group(sa, env);
    const bool valid = unit_ok && slot < S;
    const uint64_t unit_mask = (H == 64) ? ~0ull : (((1ull << H) - 1ull) << (uiw << logH));
    const int hub_slot = (k ? hp.S[0] : 0) + slot;
    const uint32_t idx = (uint32_t) env * (uint32_t) (hp.S[0] + hp.S[1]) + (uint32_t) hub_slot;  // PHILOX state is hub-major
    const uint32_t sidx = (uint32_t) k * (uint32_t) N + (uint32_t) env;
    const bool fast = hp.type[k] == 0;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    CHUB_G(const float) cls = tb.cls[k];

    uint32_t pk_in = 0;
    uint32_t w0 = 0u;
    float a = 0.0f;
    if (unit_ok) pk_in = st.pk[sa.tick & 1u][sidx];
    if (!RESET && valid) {
        w0 = sl.hot[idx];
        a = sa.actions[(uint32_t) env * (uint32_t) hp.act_dim + (uint32_t) hub_slot];
    }
    PhiloxSlot s = {{w0, ps_tl(w0), false}, 0.0f, 0.0f};
    bool car = s.tl > 0;
    f32x4 row = {0.0f, 0.0f, 0.0f, 0.0f};
    float t_target = 0.0f;
    if (car) {
        row = *(CHUB_G(const f32x4)) ((CHUB_G(const char)) cls + ((size_t) ps_cls(w0) * (kClsRow * 8u) + ps_n(w0) * 8u));
        t_target = tb.ttab[k][ps_lev(w0)];
    }
    s.power = row.x;
    s.t_soc = row.y;
    int on_override = -1;
    if (!RESET && sa.load_mode)
        on_override = load_mode_on<BLOCK>(hp, sa, st, k, env, unit_ok, valid, slot, car, s.power,
                                          car ? emergency_of(t_target, s.t_soc, s.tl) : 0.0f, lds_f, lds_u, uiw << logH) ? 1 : 0;
    const bool on = on_override >= 0 ? (car && on_override != 0) : (car && (a >= kActOnThreshold || must_charge(t_target, s.t_soc, s.tl)));
    if (car_step_philox(s, on, row.z, row.w)) t_target = 0.0f;
    if (RESET) s.w = 0u;
    car = s.tl > 0;

    // ---- receive_car: arrivals, renege, balk, admission
    const bool empty = valid && !car;
    const uint64_t be = __ballot(empty) & unit_mask;
    const int empties = __popcll(be);
    const int rank = prefix_count(be);
    Received rc = {0, 0, 0};
    if (unit_ok) rc = receive_car_word<RESET>(pk_in, fast, empties);
    if (empty && rank < rc.assign) {
        const PhiloxCar nc = add_car_philox(hp, sa, tb, k, env, hub_slot);
        t_target = nc.t_target;
        s = philox_slot_of(nc);
        car = s.tl > 0;
        sl.stay8[idx] = (uint8_t) nc.stay;
    }

    // ---- calculate_output (CHS.hpp:1233-1261 / 1544-1572): order-independent sums -- every slot power rounded to the nearest
    // multiple of 2^-19 kW, integer butterfly over the unit's H lanes, one rounding to f32
    const bool urgent = car && must_charge(t_target, s.t_soc, s.tl);
    const int q = kw_to_fixed(s.power);
    int i_min = urgent ? q : 0, i_max = car ? q : 0, i_chg = s.charge ? q : 0;
    unit_sums_dpp(H, i_min, i_max, i_chg);
    const int cars = __popcll(__ballot(car) & unit_mask);

    if (valid) sl.hot[idx] = s.w;
    if (unit_ok && slot == 0) {
        rec_store(st.rec, sidx, fixed_to_kw(i_min), fixed_to_kw(i_chg), fixed_to_kw(i_max), pkd_make(rc.line, rc.flow, cars));
    }
}

// ---------------------------------------------------------------------------------------- k_slot_unit: one workgroup per unit
// Stations of more than 64 piles (the reference takes any size, CHS.hpp:1148, 1458) outside the packed production kernel: COMPAT
// streams, the scalar-load control mode, PHILOX handles forced onto the wave-local kernels.  One (env, station) unit = ONE
// workgroup of 256 lanes (S_k <= 256), lane = charger slot; the same phases as slot_body_compat / slot_body_wave with the
// wave-local steps made workgroup-wide through LDS: ballots of empty slots per wave, the stream walk / the decode of the
// pre-drawn levels on lane 0, the reference's sequential f32 sums (COMPAT) or 64-bit integer sums (PHILOX: what the packed
// kernel's BIG path adds up) by lane 0 over the slots in order.  A parity instrument, not a fast path.
template <bool RESET, int MODE>
__global__ __launch_bounds__(256) void k_slot_unit(const DevCtx *__restrict__ ctx, StepArgs sa, int k) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const HubParams &hp = ctx->hp;
    const SlotArrays &sl = ctx->sl;
    const StationArrays &st = ctx->st;
    const Tables &tb = ctx->tb;
    __shared__ float s_a[256], s_b[256], s_c[256];  // load mode: emergency, power, power by rank; sums: min, charge, max power per slot
    __shared__ uint32_t s_u[256], s_v[256], s_w[256];
    __shared__ float s_soc[256];                    // COMPAT: per-admission variates, by admission rank
    __shared__ uint64_t s_ball[8];
    __shared__ int s_hdr[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int env = (int) blockIdx.x;
    const int64_t N = hp.n_envs;
    if (!in_group(sa, env)) return;  // the whole workgroup: nothing of an env that is not served is touched
    const int S = hp.S[k], slot = tid;
    const bool valid = slot < S;
    const bool fast = hp.type[k] == 0, cp = hp.constant_charging != 0;
    const int hub_slot = (k ? hp.S[0] : 0) + slot;
    const uint32_t idx = MODE == MODE_PHILOX ? (uint32_t) env * (uint32_t) (hp.S[0] + hp.S[1]) + (uint32_t) hub_slot
                                             : (uint32_t) hp.base[k] + (uint32_t) env * (uint32_t) S + (uint32_t) slot;
    const uint32_t sidx = (uint32_t) k * (uint32_t) N + (uint32_t) env;
    CHUB_G(const float) cls = tb.cls[k];

    // ---- the slot as the previous step left it
    typename SlotOf<MODE>::type s = {};  // the mode's slot value, empty
    float t_target = 0.0f, a = 0.0f, next_power = 0.0f, next_t_soc = 0.0f;
    if (!RESET && valid) {
        a = sa.actions[(uint32_t) env * (uint32_t) hp.act_dim + (uint32_t) hub_slot];
        if constexpr (MODE == MODE_COMPAT) {
            const u32x4 hot = ((CHUB_G(u32x4)) sl.hot)[idx];
            s = CompatSlot::unpack(hot);
            if (s.tl > 0) t_target = tb.ttab[k][hot_level(hot.w)];  // (the record keeps the arrival SoC, the target's time is a table entry)
        } else {
            s.w = sl.hot[idx];
            s.tl = ps_tl(s.w);
            if (s.tl > 0) {
                const f32x4 row = *(CHUB_G(const f32x4)) ((CHUB_G(const char)) cls + ((size_t) ps_cls(s.w) * (kClsRow * 8u) + ps_n(s.w) * 8u));
                s.power = row.x; s.t_soc = row.y; next_power = row.z; next_t_soc = row.w;
                t_target = tb.ttab[k][ps_lev(s.w)];
            }
        }
    }
    bool car = s.tl > 0, leave;

    // ---- on / off: judge_feasibility + assign_on_off_piece (CHS.hpp:1404-1413, 1364-1373), or the scalar-load control
    // (assign_on_off, CHS.hpp:1318-1362 / 1629-1674: the piles in urgency order, std::multimap keyed by -emergency)
    bool on;
    if (!RESET && sa.load_mode) {
        const float em0 = car ? emergency_of(t_target, s.t_soc, s.tl) : 0.0f;
        s_a[tid] = em0;
        __syncthreads();
        int rk = 0;
        for (int j = 0; j < S; j++) {
            const float ej = s_a[j];
            rk += (ej > em0 || (ej == em0 && j < slot)) ? 1 : 0;
        }
        if (valid) {
            s_c[rk] = car ? s.power : 0.0f;
            s_u[rk] = car ? 1u : 0u;
        }
        __syncthreads();
        // catch_load against the previous calculate_output; rank_power_add (CHS.hpp:1375-1402): sequential f32
        const float load = catch_load(hp, sa, st, k, env, sidx);
        float cum = 0.0f, mine = 0.0f;
        int cars_before = 0, mine_before = 0;
        for (int q = 0; q < S; q++) {
            if (q == rk) mine_before = cars_before;
            cum = __fadd_rn(cum, s_c[q]);
            cars_before += (int) s_u[q];
            if (q == rk) mine = cum;
        }
        on = car && load_says_on(cp, fast, load, mine, mine_before);
        __syncthreads();
    } else {
        on = car && (a >= kActOnThreshold || must_charge(t_target, s.t_soc, s.tl));
    }

    // ---- car_step, remove_car
    if constexpr (MODE == MODE_COMPAT) {
        if (on) car_step_compat(s, fast, cp, hp.cc);
        leave = remove_car_compat(s, on);
    } else {
        leave = car_step_philox(s, on, next_power, next_t_soc);
        if (RESET) s.w = 0u;
    }
    if (leave) t_target = 0.0f;
    car = s.tl > 0;

    // ---- receive_car: empties over the whole unit, admission rank = empties below the slot
    const bool empty = valid && !car;
    const uint64_t be = __ballot(empty);
    if (lane == 0) s_ball[wave] = be;
    __syncthreads();
    int empties = 0, rank = prefix_count(be);
    for (int w = 0; w < 4; w++) {
        const int c = __popcll(s_ball[w]);
        empties += c;
        rank += w < wave ? c : 0;
    }
    if (tid == 0) {
        Received rc;
        if (MODE == MODE_COMPAT) {
            const CompatRng &cr = ctx->cr;
            CompatStream rs;
            rs.load(cr, sa.rng_cur, env);
            rc = receive_car_streams<RESET>(rs, hp, sa, tb, k, env, fast, RESET ? 0 : pkd_line(st.rec[4u * sidx + 3u]), empties);
            for (int rr = 0; rr < rc.assign; rr++) {  // ascending slot order == ascending rank
                const CarDraw d = draw_car_streams(rs);
                s_soc[rr] = d.soc;
                s_v[rr] = (uint32_t) d.lev;
                s_w[rr] = (uint32_t) d.late;
            }
            rs.store(cr, sa.rng_cur, env);
        } else {
            rc = receive_car_word<RESET>(st.pk[sa.tick & 1u][sidx], fast, empties);
        }
        s_hdr[0] = rc.assign; s_hdr[1] = rc.flow; s_hdr[2] = rc.line;
    }
    __syncthreads();
    const int assign = s_hdr[0];
    if (empty && rank < assign) {
        if constexpr (MODE == MODE_COMPAT) {
            const NewCar nc = add_car_compat(fast, s_soc[rank], (int) s_v[rank], (int) s_w[rank], cp);
            t_target = nc.t_target;
            s = compat_slot_of(nc);
        } else {
            const PhiloxCar nc = add_car_philox(hp, sa, tb, k, env, hub_slot);
            t_target = nc.t_target;
            s = philox_slot_of(nc);
            sl.stay8[idx] = (uint8_t) nc.stay;
        }
        car = s.tl > 0;
    } else if (leave || RESET) {
        if constexpr (MODE == MODE_COMPAT) s.meta = 0;
    }

    // ---- calculate_output (CHS.hpp:1233-1261 / 1544-1572)
    const bool urgent = car && must_charge(t_target, s.t_soc, s.tl);
    const uint64_t bc = __ballot(car);
    if (lane == 0) s_ball[4 + wave] = bc;
    if (MODE == MODE_COMPAT) {
        s_a[tid] = urgent ? s.power : 0.0f;
        s_b[tid] = s.charge ? s.power : 0.0f;
        s_c[tid] = car ? s.power : 0.0f;
    } else {
        const int q = kw_to_fixed(s.power);
        s_u[tid] = (uint32_t) (urgent ? q : 0);
        s_v[tid] = (uint32_t) (s.charge ? q : 0);
        s_w[tid] = (uint32_t) (car ? q : 0);
    }
    if (valid) {
        if constexpr (MODE == MODE_COMPAT) ((CHUB_G(u32x4)) sl.hot)[idx] = s.pack();
        else sl.hot[idx] = s.w;
    }
    __syncthreads();
    if (tid == 0) {
        const int cars = __popcll(s_ball[4]) + __popcll(s_ball[5]) + __popcll(s_ball[6]) + __popcll(s_ball[7]);
        float r_min, r_chg, r_max;
        if (MODE == MODE_COMPAT) {
            SumsF32 r = {0.0f, 0.0f, 0.0f};
            r.add(s_a, s_b, s_c, S);
            r_min = r.mn; r_chg = r.chg; r_max = r.mx;
        } else {
            SumsI64 r = {0, 0, 0};
            r.add(s_u, s_v, s_w, S);
            r_min = fixed64_to_kw(r.mn); r_chg = fixed64_to_kw(r.chg); r_max = fixed64_to_kw(r.mx);
        }
        rec_store(st.rec, sidx, r_min, r_chg, r_max, pkd_make(s_hdr[2], s_hdr[1], cars));
    }
}

// ---------------------------------------------------------------------------------------- k_slot_unit_any: a unit of any size
// Stations of more than 256 piles (the reference's constructors take any count, CHS.hpp:1148, 1458).  One (env, station) unit = ONE
// workgroup of 256 lanes that goes over the unit's piles in chunks of 256, in slot order, in two passes with the slot records
// themselves (global memory; every lane re-reads only what it wrote) as the state between them:
//   pass 1  per chunk: on / off, car_step, departures, the record written back; the unit's empty slots counted
//   lane 0  arrivals / renege / balk / how many are admitted (receive_car; COMPAT: the env's streams in the reference's order)
//   pass 2  per chunk: admission by rank (COMPAT: lane 0 draws the chunk's new cars' variates, in rank order, as it gets there),
//           add_car, then calculate_output: lane 0 adds the chunk's slot powers to the running sums IN SLOT ORDER (COMPAT: the
//           reference's sequential f32 sums; PHILOX: 64-bit integers)
// The scalar-load control (evs_step(float)) ranks every pile of the unit by urgency first: three arrays over the whole unit in
// LDS, hence kMaxPiles.  A parity instrument like k_slot_unit (same phases, same arithmetic), not a fast path.
template <bool RESET, int MODE>
__global__ __launch_bounds__(256) void k_slot_unit_any(const DevCtx *__restrict__ ctx, StepArgs sa, int k) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const HubParams &hp = ctx->hp;
    const SlotArrays &sl = ctx->sl;
    const StationArrays &st = ctx->st;
    const Tables &tb = ctx->tb;
    __shared__ float s_a[256], s_b[256], s_c[256];  // the chunk's min / charge / max power per slot (COMPAT)
    __shared__ uint32_t s_u[256], s_v[256], s_w[256];  // ... as integers (PHILOX); COMPAT: s_v / s_w = level, late time by admission rank
    __shared__ float s_soc[256];                    // COMPAT: arrival SoC by admission rank within the chunk
    __shared__ uint64_t s_ball[8];
    __shared__ int s_hdr[4];
    __shared__ int s_cnt;
    __shared__ float s_em[kMaxPiles], s_pw[kMaxPiles];    // load mode: emergency by slot; power by urgency rank -> running sum
    __shared__ uint16_t s_cb[kMaxPiles], s_rk[kMaxPiles]; // ... cars by urgency rank -> cars before the rank; urgency rank by slot
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int env = (int) blockIdx.x;
    const int64_t N = hp.n_envs;
    if (!in_group(sa, env)) return;  // the whole workgroup: nothing of an env that is not served is touched
    const int S = hp.S[k], chunks = (S + 255) >> 8;
    const bool fast = hp.type[k] == 0, cp = hp.constant_charging != 0;
    const int hub0 = k ? hp.S[0] : 0;
    const uint32_t idx0 = MODE == MODE_PHILOX ? (uint32_t) env * (uint32_t) (hp.S[0] + hp.S[1]) + (uint32_t) hub0
                                              : (uint32_t) hp.base[k] + (uint32_t) env * (uint32_t) S;
    const uint32_t sidx = (uint32_t) k * (uint32_t) N + (uint32_t) env;
    CHUB_G(const float) cls = tb.cls[k];
    if (tid == 0) s_cnt = 0;
    __syncthreads();

    // ---- scalar-load control (assign_on_off, CHS.hpp:1318-1362 / 1629-1674): the piles in urgency order (std::multimap keyed by
    // -emergency: ties in slot order), switched on until the target is met
    float load = 0.0f;
    if (!RESET && sa.load_mode) {
        for (int slot = tid; slot < S; slot += 256) {
            const uint32_t idx = idx0 + (uint32_t) slot;
            float t_target = 0.0f, t_soc = 0.0f;
            int tl;
            if (MODE == MODE_COMPAT) {
                const u32x4 hot = ((CHUB_G(u32x4)) sl.hot)[idx];
                t_soc = __uint_as_float(hot.z);
                tl = hot_tl(hot.w);
                if (tl > 0) t_target = tb.ttab[k][hot_level(hot.w)];
            } else {
                const uint32_t w0 = sl.hot[idx];
                tl = ps_tl(w0);
                if (tl > 0) {
                    t_soc = (*(CHUB_G(const f32x2)) ((CHUB_G(const char)) cls + ((size_t) ps_cls(w0) * (kClsRow * 8u) + ps_n(w0) * 8u))).y;
                    t_target = tb.ttab[k][ps_lev(w0)];
                }
            }
            s_em[slot] = tl > 0 ? emergency_of(t_target, t_soc, tl) : 0.0f;
        }
        __syncthreads();
        for (int slot = tid; slot < S; slot += 256) {
            const uint32_t idx = idx0 + (uint32_t) slot;
            float power = 0.0f;
            bool car;
            if (MODE == MODE_COMPAT) {
                const u32x4 hot = ((CHUB_G(u32x4)) sl.hot)[idx];
                car = hot_tl(hot.w) != 0;
                power = __uint_as_float(hot.x);
            } else {
                const uint32_t w0 = sl.hot[idx];
                car = ps_tl(w0) > 0;
                if (car) power = (*(CHUB_G(const f32x2)) ((CHUB_G(const char)) cls + ((size_t) ps_cls(w0) * (kClsRow * 8u) + ps_n(w0) * 8u))).x;
            }
            const float em0 = s_em[slot];
            int rk = 0;
            for (int j = 0; j < S; j++) {
                const float ej = s_em[j];
                rk += (ej > em0 || (ej == em0 && j < slot)) ? 1 : 0;
            }
            s_rk[slot] = (uint16_t) rk;
            s_pw[rk] = car ? power : 0.0f;
            s_cb[rk] = car ? 1 : 0;
        }
        __syncthreads();
        // catch_load against the previous calculate_output; rank_power_add (CHS.hpp:1375-1402): sequential f32
        load = catch_load(hp, sa, st, k, env, sidx);
        if (tid == 0) {
            float cum = 0.0f;
            int cars_before = 0;
            for (int q = 0; q < S; q++) {
                const int c = (int) s_cb[q];
                cum = __fadd_rn(cum, s_pw[q]);
                s_pw[q] = cum;                        // the running sum up to and including rank q
                s_cb[q] = (uint16_t) cars_before;     // cars of a higher urgency
                cars_before += c;
            }
        }
        __syncthreads();
    }

    // ---- pass 1: the slots as the previous step left them -> on / off, car_step, departures
    for (int c = 0; c < chunks; c++) {
        const int slot = (c << 8) + tid;
        const bool valid = slot < S;
        const uint32_t idx = idx0 + (uint32_t) slot;
        float a = 0.0f;
        if (!RESET && valid) a = sa.actions[(uint32_t) env * (uint32_t) hp.act_dim + (uint32_t) (hub0 + slot)];
        // on / off of a slot with a car: the scalar-load control by the car's urgency rank, else the pile's action or its urgency
        auto switched_on = [&](const float t_target, const float t_soc, const int tl) {
            if (!RESET && sa.load_mode) {
                const int rk = (int) s_rk[slot];
                return load_says_on(cp, fast, load, s_pw[rk], (int) s_cb[rk]);
            }
            return a >= kActOnThreshold || must_charge(t_target, t_soc, tl);
        };
        bool car;
        if constexpr (MODE == MODE_COMPAT) {
            CompatSlot s = {};
            float t_target = 0.0f;
            if (!RESET && valid) {
                const u32x4 hot = ((CHUB_G(u32x4)) sl.hot)[idx];
                s = CompatSlot::unpack(hot);
                if (s.tl > 0) t_target = tb.ttab[k][hot_level(hot.w)];
            }
            const bool on = s.tl > 0 && switched_on(t_target, s.t_soc, s.tl);
            if (on) car_step_compat(s, fast, cp, hp.cc);
            remove_car_compat(s, on);
            if (RESET) s.meta = 0;
            if (valid) ((CHUB_G(u32x4)) sl.hot)[idx] = s.pack();
            car = s.tl > 0;
        } else {  // (the state word alone: pass 2 reads the car's row entry again)
            PhiloxWord s = {};
            float t_target = 0.0f, t_soc = 0.0f;
            if (!RESET && valid) {
                s.w = sl.hot[idx];
                s.tl = ps_tl(s.w);
                if (s.tl > 0) {
                    t_soc = (*(CHUB_G(const f32x2)) ((CHUB_G(const char)) cls + ((size_t) ps_cls(s.w) * (kClsRow * 8u) + ps_n(s.w) * 8u))).y;
                    t_target = tb.ttab[k][ps_lev(s.w)];
                }
            }
            const bool on = s.tl > 0 && switched_on(t_target, t_soc, s.tl);
            car_step_word(s, on);
            if (RESET) s.w = 0u;
            if (valid) sl.hot[idx] = s.w;
            car = s.tl > 0;
        }
        const uint64_t be = __ballot(valid && !car);
        if (lane == 0 && be) atomicAdd(&s_cnt, __popcll(be));
    }
    __syncthreads();
    const int empties = s_cnt;

    // ---- receive_car (CHS.hpp:1272-1316 / 1583-1627): lane 0 decides how many cars the unit admits
    CompatStream rs;
    if (tid == 0) {
        Received rc;
        if (MODE == MODE_COMPAT) {
            rs.load(ctx->cr, sa.rng_cur, env);
            rc = receive_car_streams<RESET>(rs, hp, sa, tb, k, env, fast, RESET ? 0 : pkd_line(st.rec[4u * sidx + 3u]), empties);
        } else {
            rc = receive_car_word<RESET>(st.pk[sa.tick & 1u][sidx], fast, empties);
        }
        s_hdr[0] = rc.assign; s_hdr[1] = rc.flow; s_hdr[2] = rc.line;
    }
    __syncthreads();
    const int assign = s_hdr[0];

    // ---- pass 2: admission by rank, add_car, calculate_output (CHS.hpp:1233-1261 / 1544-1572)
    int base = 0, cars = 0;                     // empties / cars of the chunks in front (the same number in every lane)
    SumsF32 rf = {0.0f, 0.0f, 0.0f};            // lane 0: the running sums
    SumsI64 ri = {0, 0, 0};
    for (int c = 0; c < chunks; c++) {
        const int slot = (c << 8) + tid;
        const bool valid = slot < S;
        const uint32_t idx = idx0 + (uint32_t) slot;
        float power = 0.0f, t_target = 0.0f, t_soc = 0.0f;
        int tl = 0;
        bool charge = false;
        if (valid) {  // what pass 1 left (this lane's own stores)
            if (MODE == MODE_COMPAT) {
                const u32x4 hot = ((CHUB_G(u32x4)) sl.hot)[idx];
                const CompatSlot cs = CompatSlot::unpack(hot);
                power = cs.power; t_soc = cs.t_soc; tl = cs.tl; charge = cs.charge;
                if (tl > 0) t_target = tb.ttab[k][hot_level(hot.w)];
            } else {
                const uint32_t w0 = sl.hot[idx];
                tl = ps_tl(w0);
                charge = (w0 & kPsChg) != 0u;
                if (tl > 0) {
                    const f32x2 row = *(CHUB_G(const f32x2)) ((CHUB_G(const char)) cls + ((size_t) ps_cls(w0) * (kClsRow * 8u) + ps_n(w0) * 8u));
                    power = row.x; t_soc = row.y;
                    t_target = tb.ttab[k][ps_lev(w0)];
                }
            }
        }
        bool car = tl > 0;
        const bool empty = valid && !car;
        const uint64_t be = __ballot(empty);
        if (lane == 0) s_ball[wave] = be;
        __syncthreads();
        int chunk_empties = 0, rank = base + prefix_count(be);
        for (int w = 0; w < 4; w++) {
            const int n = __popcll(s_ball[w]);
            chunk_empties += n;
            rank += w < wave ? n : 0;
        }
        if (MODE == MODE_COMPAT) {
            if (tid == 0) {  // the chunk's new cars, ascending slot order == ascending rank
                int n_new = assign - base;
                n_new = n_new < 0 ? 0 : (n_new > chunk_empties ? chunk_empties : n_new);
                for (int rr = 0; rr < n_new; rr++) {
                    const CarDraw d = draw_car_streams(rs);
                    s_soc[rr] = d.soc;
                    s_v[rr] = (uint32_t) d.lev;
                    s_w[rr] = (uint32_t) d.late;
                }
            }
            __syncthreads();
        }
        if (empty && rank < assign) {
            if (MODE == MODE_COMPAT) {
                const int r = rank - base;
                const NewCar nc = add_car_compat(fast, s_soc[r], (int) s_v[r], (int) s_w[r], cp);
                t_target = nc.t_target; t_soc = nc.t_soc; tl = nc.stay; power = nc.power;
                ((CHUB_G(u32x4)) sl.hot)[idx] = compat_slot_of(nc).pack();
            } else {
                const PhiloxCar nc = add_car_philox(hp, sa, tb, k, env, hub0 + slot);
                t_target = nc.t_target; t_soc = nc.t_soc; tl = nc.stay; power = nc.power;
                sl.hot[idx] = nc.word;
                sl.stay8[idx] = (uint8_t) nc.stay;
            }
            car = tl > 0;
        }
        const bool urgent = car && must_charge(t_target, t_soc, tl);
        const uint64_t bc = __ballot(car);
        if (lane == 0) s_ball[4 + wave] = bc;
        if (MODE == MODE_COMPAT) {
            s_a[tid] = urgent ? power : 0.0f;
            s_b[tid] = charge ? power : 0.0f;
            s_c[tid] = car ? power : 0.0f;
        } else {
            const int q = kw_to_fixed(power);
            s_u[tid] = (uint32_t) (urgent ? q : 0);
            s_v[tid] = (uint32_t) (charge ? q : 0);
            s_w[tid] = (uint32_t) (car ? q : 0);
        }
        __syncthreads();
        cars += __popcll(s_ball[4]) + __popcll(s_ball[5]) + __popcll(s_ball[6]) + __popcll(s_ball[7]);
        if (tid == 0) {
            const int n = S - (c << 8) < 256 ? S - (c << 8) : 256;
            if (MODE == MODE_COMPAT) rf.add(s_a, s_b, s_c, n);
            else ri.add(s_u, s_v, s_w, n);
        }
        base += chunk_empties;
        __syncthreads();  // the chunk's LDS areas are free again
    }
    if (tid == 0) {
        if (MODE == MODE_COMPAT) {
            rs.store(ctx->cr, sa.rng_cur, env);
            rec_store(st.rec, sidx, rf.mn, rf.chg, rf.mx, pkd_make(s_hdr[2], s_hdr[1], cars));
        } else {
            rec_store(st.rec, sidx, fixed64_to_kw(ri.mn), fixed64_to_kw(ri.chg), fixed64_to_kw(ri.mx), pkd_make(s_hdr[2], s_hdr[1], cars));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_slot_packed: the PHILOX step (production).  PHILOX slot state is laid out hub-major, [env][hub slot] (station 0's piles,
// then station 1's), like the action rows: the workgroup's BLOCK * T virtual lanes map onto epb = BLOCK * T / (S0 + S1) whole
// envs laid end to end, so its state loads, action loads and state stores are each ONE contiguous run of memory, read or
// written once.  A unit = one (env, station) = S_k consecutive virtual lanes; units may straddle a wave boundary, so every
// (virtual) wave publishes its ballot of empty slots in LDS (admission rank = empties of the unit in the previous wave +
// empties below the lane in its own wave), and the station sums are integer LDS atomics (order-independent by definition).
// A slot is empty after this step iff its stay is over, which the state word says by itself: the ballots, the barrier,
// the renege / balk / admission arithmetic and the queueing of the admitted lanes all run while the class-row reads are
// still in flight.  The new cars of the workgroup (a handful) and the station records are the last wave's business, one
// lane per car / per unit; the other waves are done after the second barrier.
//
// PackedArgs: everything a wave needs up front, by value in the kernel arguments and requested in one scalar batch.
struct PackedArgs {
    uint32_t S[2], type[2];
    uint32_t n_envs, epb, magic, cls_delta;  // envs per workgroup; 2^20 / (S0 + S1) + 1; byte distance cls[1] - cls[0]
    CHUB_G(uint32_t) state;          // [N][S0 + S1]: one word per slot
    CHUB_G(uint32_t) rec;
    CHUB_G(const uint32_t) pk;       // this step's station draws per unit, decoded (dk_make); RESET: the raw initial-occupancy draws
    CHUB_G(const float) actions;
    CHUB_G(const float) cls0;        // station 0's class table; station 1's is cls_delta bytes further
    CHUB_G(const float) ttab2;       // [2][1024] soc_to_time(target level) of both stations' curves (1000 used)
    CHUB_G(const uint32_t) car_tape; // TAPE: [N][S0 + S1][2] per slot, used if the slot admits a car this step: class, level | late << 16
    // add_car's Philox block (the new cars come last in the workgroup, behind two barriers: nothing of theirs should wait
    // for a load that could have been issued at the start of the wave)
    uint32_t key[2], gid0, tick;     // Philox key, global id of env 0, host tick
    const uint32_t *tick_base;       // device-side tick offset (graph replays), added to tick
    uint32_t late[8];                // the first 8 thresholds of mk_late_time's table (late_from_word); beyond them with probability 0.3 %
    CHUB_G(const uint8_t) env_mask;  // per-env clocks: non-zero = the launch serves this env (null: every env)
    uint32_t blk0;                   // ... and the first workgroup of the range of envs it names (the grid covers that range only)
    uint32_t xcd;                    // non-zero: tiles in XCD-aware order (xcd_order; handles whose streams are cache-resident: the small tile) -- the
                                     // launch's number of workgroups, here so that it arrives with the first batch of arguments (gridDim.x is a load of its own)
    CHUB_G(float) tail_act;          // [N][2] out: the env's two tail actions, for the tail kernel (StationArrays::tail_act)
    CHUB_G(uint8_t) stay8;           // [N][S0 + S1] out, per admitted car: its stay_time (introspection only)
    CHUB_G(const uint32_t) rec_prev; // RAW (the second slot launch of a pair, k_env_pair): the records the pair's first slot launch left -- pk is then
                                     // the units' raw 64-bit draws (the pk_tape layout at dk_make), decoded against the queue length kept there
};

typedef const uint32_t __attribute__((address_space(4))) *chub_sptr;  // constant address space: scalar loads
__device__ __forceinline__ uint32_t sload_u32(const void *p, int i) { return ((chub_sptr) (uintptr_t) p)[i]; }
// A masked reset behind a step that counted its done envs on the device (StepArgs::skip_count, chub_autoreset_step_device): the count is 0
// on most calls and the mask then names nobody.  The count was written by an earlier launch of the stream, so a uniform load reads it.
__device__ __forceinline__ bool mask_is_empty(const StepArgs &sa) { return sa.skip_count != nullptr && sload_u32(sa.skip_count, 0) == 0u; }

// RESET: evs_reset (CHS.hpp:1209-1231 / 1520-1542) on the same layout: no state comes in, the unit's initial occupancy was drawn
// by k_reset_levels, every wave helps with the (many) new cars.  BIG: a station with more than 64 piles -- a unit then spans
// several waves (its empties are counted over all of them) and its power sums need 64 bits.
// The action rows are read exactly once: CHUB_ACT_NT = 1 loads them with the non-temporal hint, so that they do not push the slot state --
// which the next step reads again -- out of the Infinity Cache (C5: 69 MB of rows per step next to 134 MB of state)
#ifndef CHUB_ACT_NT
#define CHUB_ACT_NT 0
#endif
#if CHUB_ACT_NT
#define CHUB_ACT_LOAD(p) __builtin_nontemporal_load(p)
#else
#define CHUB_ACT_LOAD(p) (*(p))
#endif
#ifndef CHUB_ACC_COPIES
#define CHUB_ACC_COPIES 2  // copies of a unit's LDS accumulators (lanes spread over them by lane number: fewer same-address atomics; 1 / 2 / 4: 21.28 / 20.95 / 21.12 us)
#endif
constexpr int kAccCopies = CHUB_ACC_COPIES;
#ifndef CHUB_TAIL_PRE
#define CHUB_TAIL_PRE 1  // 1: the tail actions packed_records hands over are requested with the workgroup's first loads; 0: where it stores them (A/B)
#endif
#ifndef CHUB_UNIT_DRAWS
#define CHUB_UNIT_DRAWS 1  // 1: steps on the small tile take a unit's decoded draws and its admission count once, in the unit pass; 0: every lane of the unit (A/B)
#endif
#ifndef CHUB_EPI_ALL
#define CHUB_EPI_ALL 1  // 1: every wave of the workgroup takes its share of the new cars (a third barrier: -0.2 us at C4); 0: the last wave alone
#endif
// The station records of a workgroup of the packed kernel, one lane of ONE wave per unit (the caller has passed the workgroup's last
// barrier: every car's LDS atomics are in).  FUSED: also into s_rec, for the tails that follow in the same workgroup.
#define CHUB_AT(T_, base, byte_off) (*(CHUB_G(T_)) ((CHUB_G(char)) (base) + (uint32_t) (byte_off)))
template <int BLOCK, int T, bool RESET, bool BIG, bool MASKED, bool FUSED, bool BITS, bool RAW = false>
__device__ __forceinline__ void packed_records(const PackedArgs &pa, const uint32_t block_local, int *s_acc, const uint32_t *s_unit, u32x4 *s_rec,
                                               const float *tail_pre = nullptr) {
    const int lane = threadIdx.x & 63;
    const int S0 = (int) pa.S[0], S1 = (int) pa.S[1], St = S0 + S1;
    const int epb = (int) pa.epb, N = (int) pa.n_envs;
    const int env_first = (int) block_local * epb;
    const long long *s_acc64 = (const long long *) s_acc;
    // the wave's own LDS atomics above are in program order with the reads below; nothing else touches s_acc any more
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int i = lane; i < 2 * epb; i += 64) {  // one station record per unit
        const int e = i >> 1, k = i & 1;
        const int env = env_first + e;
        if (env >= N) continue;
        if (MASKED && pa.env_mask[env] == 0) continue;
        const uint32_t su = (uint32_t) (k ? N : 0) + (uint32_t) env;
        if (!RESET && !FUSED && !BITS && k == 0) {  // the env's tail actions sit in the lines this workgroup has just read: hand them to the tail kernel packed
            typedef float f32x2_ __attribute__((ext_vector_type(2)));
            // The first pass (unit i = lane: all there is for hubs of 16 piles and more, 32 envs per workgroup at most) has them in registers,
            // requested with the workgroup's first loads (slot_body_packed); the passes behind it read them here.
            const uint32_t ai = ((uint32_t) env * (uint32_t) (St + 2) + (uint32_t) St) << 2;
            f32x2_ tv;
            if (CHUB_TAIL_PRE && i < 64) tv = f32x2_{tail_pre[0], tail_pre[1]};
            else tv = f32x2_{CHUB_AT(const float, pa.actions, ai), CHUB_AT(const float, pa.actions, ai + 4u)};
            CHUB_AT(f32x2_, pa.tail_act, (uint32_t) env << 3) = tv;
        }
        uint32_t lf = s_unit[i];
        if (!RAW && (k ? S1 : S0) == 0) {  // (RAW: the unit pass has decoded the raw draws and left exactly this word in s_unit)
            // a station without piles still queues, reneges and balks (receive_car runs on it as on any other, CHS.hpp:1272-1316 /
            // 1583-1627; nobody is ever admitted): its queue length and arrival count move on here, power sums and cars stay 0
            const uint32_t pk = CHUB_AT(const uint32_t, pa.pk, su << 2);
            const bool fast = (k ? pa.type[1] : pa.type[0]) == 0;
            int want, fl;
            if (RESET) {  // evs_reset of a station without piles: init_station_car_number(0, 3) arrivals, nobody queues
                fl = fast ? (int) (int16_t) (pk & 0xFFFFu) : (int) ((pk >> 16) & 0xFFFFu);
                want = fl;
            } else {
                want = dk_want(pk);
                fl = dk_flow(pk);
            }
            // assign_car (CHS.hpp:417-430) with no empty slot: min(line + flow, 0) cars are assigned, the rest queue
            const int as = want < 0 ? want : 0;
            int ln = want - as;
            ln = ln < kMaxLine ? ln : kMaxLine;
            lf = pkd_make(ln, fl, 0);
        }
        u32x4 rv;
        if (!BIG) {
            int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
            for (int c = 0; c < kAccCopies; c++) {
                const int *acc = s_acc + 4 * i + c * 8 * epb;
                a0 += acc[0]; a1 += acc[1]; a2 += acc[2]; a3 += acc[3];
            }
            rv = u32x4{__float_as_uint(fixed_to_kw(a0)), __float_as_uint(fixed_to_kw(a1)), __float_as_uint(fixed_to_kw(a2)),
                       lf | ((uint32_t) a3 << 16)};
        } else {
            const long long *a64 = s_acc64 + 4 * i;
            rv = u32x4{__float_as_uint((float) a64[0] * (1.0f / 524288.0f)), __float_as_uint((float) a64[1] * (1.0f / 524288.0f)),
                       __float_as_uint((float) a64[2] * (1.0f / 524288.0f)), lf | ((uint32_t) a64[3] << 16)};
        }
        CHUB_AT(u32x4, pa.rec, su << 4) = rv;
        if (FUSED) s_rec[i] = rv;
    }
}
#undef CHUB_AT

// MASKED: per-env clocks (the launch serves the envs of a mask); the lock-step instantiation carries none of it.
// FUSED (k_step_fused, small batches): the workgroup goes on by itself -- the body then returns IN FRONT of its third barrier with what
// this wave does next (w + 1: wave w < last; WAVES: the last wave, which will write the records, also into s_rec, between the two
// halves of its tails), does not hand the tail actions over through memory, and calls hook.prefetch() behind its first loads /
// hook.park() in front of its first barrier (the tail's table rows travel with the slot loads).
struct NoHook {
    __device__ __forceinline__ void prefetch() {}
    __device__ __forceinline__ void park() {}
};
// BITS: the pile decisions arrive as one bit per pile ([N][ceil(S / 64)] u64 behind pa.actions) instead of a row of floats:
// 8 bytes per env and word instead of 4 per pile (chub_step_bits; the tail kernel reads the two tail actions from their own array).
// PIPED (k_steps_piped): the new cars are the business of the upper half of the workgroup's slot waves -- the lower half returns right behind the
// third barrier and makes the next step's draws meanwhile.
// RAW (the second slot launch of a pair of steps whose tails share one launch, k_env_pair): no tail launch has run since the step before, so
// the unit's draws wait in their raw 64-bit form and the unit pass decodes them (dk_make) against the queue the step before left in its record.
template <int BLOCK, int T, bool TAPE, bool RESET, bool BIG, bool MASKED, bool FUSED, typename Hook, bool BITS = false, bool PIPED = false, bool RAW = false>
__device__ __forceinline__ int slot_body_packed(const HubParams &hp, const StepArgs &sa, PackedArgs &pa, const Tables &tb,
                                                const uint32_t block_local, uint32_t *q_cnt, uint32_t *q_new,
                                                uint64_t *s_ball, int *s_acc, uint32_t *s_unit, Hook &hook, u32x4 *s_rec, uint32_t *s_uinfo) {
    // T slots per lane: virtual lane v = tid + j * BLOCK (j < T), virtual wave = wave + j * (BLOCK / 64).  All T slots' loads
    // are in flight together and the barriers are shared.
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    constexpr int WAVES = BLOCK / 64;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int S0 = (int) pa.S[0], S1 = (int) pa.S[1], St = S0 + S1;
    const int epb = (int) pa.epb, N = (int) pa.n_envs;
    const int env_first = (int) block_local * epb;
    const uint32_t idx0 = (uint32_t) env_first * (uint32_t) St;
    CHUB_STAMP_DECL(16);
    CHUB_STAMP_REAL(12);
    CHUB_STAMP(0);
    // every array reached from here is < 4 GiB (checked at create), so addresses are a uniform base + a 32-bit byte offset
    // per lane: the loads and stores take the base from SGPRs and need no 64-bit address arithmetic
#define CHUB_AT(T_, base, byte_off) (*(CHUB_G(T_)) ((CHUB_G(char)) (base) + (uint32_t) (byte_off)))

    // phase A loads: slot state, action, the unit's packed draws.  Steps on the small tile request the state words of all T slots FIRST and everything
    // else behind them (the per-env clock byte, the draws, the action rows or bit words, the last wave's tail actions): vector loads
    // return in order, and the class-row requests below wait for the state words alone -- the draws are not looked at before the
    // admission, the actions not before the rows are in.  All of a step's requests sit in one basic block and are issued by every lane:
    // a lane without a slot asks for the workgroup's first slot / env (env_first < N in every launch), and what it gets is never used
    // (its occupancy is forced to 0 below).  One block, because behind exec-predicated blocks the wait in front of the class rows
    // comes out as vmcnt(0).  Two forms keep the slot-by-slot order: the large tile, whose streams come from HBM (state words first cost it
    // 1.4 % of the C5 step), and the one-launch kernels (FUSED: 0.4-1 % of the C2 step; they compile to what they were) -- docs/LAB_NOTEBOOK.md, Part I.
    constexpr bool STATE_FIRST = !RESET && !FUSED && BLOCK <= 256;
    // The same forms take a unit's decoded draws ONCE: all S_k lanes of a unit used to ask for the same word and work the same
    // assign / line out of it.  The lane that runs unit u in the unit pass behind barrier 1 (thread u; T <= 2 and epb <= BLOCK * T / 4: 2 epb <= BLOCK
    // units, one pass) requests the word behind its wave's action rows, as the last wave requests its tail actions, and leaves the unit's
    // admission count in s_uinfo -- where its empties were, which only that count needed -- and its record word in s_unit.  (A wait counts
    // from the youngest request: a wave that makes such an extra request waits for one of its action rows with the state words, the others
    // for the state words alone.  In front of the state words, where every wave's wait is exact, and on the last wave were measured and
    // lost 0.1 % each -- docs/LAB_NOTEBOOK.md, Part I.)  A step's `want` is an unsigned byte of the decoded
    // word (dk_make), so the count is 0 ... 64; the raw draws of a reset, which are negative on small fast stations, keep the per-lane form,
    // as do the large tile, the one-launch kernels and stations of more than 64 piles.
    constexpr bool UNIT_DRAWS = CHUB_UNIT_DRAWS && STATE_FIRST && !BIG && T <= 2;
    static_assert(!RAW || (UNIT_DRAWS && !MASKED && !BITS && !TAPE), "the raw draws are decoded in the unit pass of the lock-step small tile");
    int e_[T], k_[T], slot[T];
    bool valid[T];
    uint32_t sidx[T];
    uint32_t s2[T];
    float act[T];
    u32x2 actw[T];  // BITS: the word of the env's decision bits this slot's bit sits in
    int hs_[T];
    uint32_t pk_in[T];
    uint32_t served[T];  // per-env clocks: is the env served by this launch?  Requested right behind the state, looked at with it
    // The env's two tail actions sit in the lines this workgroup reads anyway: the lane of the last wave that will write env lane / 2's
    // records (packed_records, its first pass) asks for them here and hands them to the tail kernel from registers, not behind a
    // round trip of its own at the end of the workgroup's life.
    constexpr bool HOIST_TAIL = CHUB_TAIL_PRE && !RESET && !FUSED && !BITS;
    float tail_pre[2];
#pragma unroll
    for (int j = 0; j < T; j++) {
        const int v = tid + j * BLOCK;
        // v / (S0 + S1) (magic = 2^20 / St + 1, checked on the host); 24-bit multiplies (full rate; v < 2^11, magic <= 2^20 + 1, the
        // product below 2^32): the 32-bit v_mul_lo_u32 is a quarter-rate instruction
        e_[j] = (int) (__umul24((uint32_t) v, pa.magic) >> 20);
        const int hs = v - (int) __umul24((uint32_t) e_[j], (uint32_t) St);  // hub slot
        k_[j] = hs >= S0 ? 1 : 0;
        hs_[j] = hs;
        slot[j] = hs - (k_[j] ? S0 : 0);
        const int env = env_first + e_[j];
        valid[j] = e_[j] < epb && env < N;
        served[j] = 1u;
        sidx[j] = (uint32_t) (k_[j] ? N : 0) + (uint32_t) env;
        asm volatile("" : "=v"(s2[j]), "=v"(act[j]), "=v"(pk_in[j]), "=v"(actw[j]));
        if (!STATE_FIRST) {  // slot by slot, the lanes that have one: clock byte, state, action, draws
            if (RESET) {
                s2[j] = 0u;
                act[j] = 0.0f;
            }
            if (MASKED && valid[j]) served[j] = pa.env_mask[env];
            if (valid[j]) {
                if (!RESET) {
                    s2[j] = CHUB_AT(uint32_t, pa.state, (idx0 + (uint32_t) v) << 2);
                    if (BITS) actw[j] = CHUB_AT(const u32x2, pa.actions, ((uint32_t) env * (((uint32_t) St + 63u) >> 6) + ((uint32_t) hs >> 6)) << 3);
                    else act[j] = CHUB_ACT_LOAD((CHUB_G(const float)) ((CHUB_G(const char)) pa.actions + (uint32_t) ((idx0 + (uint32_t) v + 2u * (uint32_t) env) << 2)));  // row stride S0 + S1 + 2
                }
                pk_in[j] = CHUB_AT(const uint32_t, pa.pk, sidx[j] << 2);
            }
        }
    }
    if (STATE_FIRST) {
        uint32_t vc[T], envc[T];  // the lane's slot and env, or the workgroup's first
#pragma unroll
        for (int j = 0; j < T; j++) {
            vc[j] = valid[j] ? (uint32_t) (tid + j * BLOCK) : 0u;
            envc[j] = valid[j] ? (uint32_t) (env_first + e_[j]) : (uint32_t) env_first;
        }
#pragma unroll
        for (int j = 0; j < T; j++) s2[j] = CHUB_AT(uint32_t, pa.state, (idx0 + vc[j]) << 2);
        asm volatile("" ::: "memory");  // (the compiler keeps the requests of one block in this order)
        if (MASKED) {
#pragma unroll
            for (int j = 0; j < T; j++) served[j] = CHUB_AT(const uint8_t, pa.env_mask, envc[j]);
            asm volatile("" ::: "memory");
        }
        if (!UNIT_DRAWS) {
#pragma unroll
            for (int j = 0; j < T; j++) pk_in[j] = CHUB_AT(const uint32_t, pa.pk, (valid[j] ? sidx[j] : (uint32_t) env_first) << 2);
            asm volatile("" ::: "memory");
        }
#pragma unroll
        for (int j = 0; j < T; j++) {
            if (BITS) actw[j] = CHUB_AT(const u32x2, pa.actions, (envc[j] * (((uint32_t) St + 63u) >> 6) + (valid[j] ? (uint32_t) hs_[j] >> 6 : 0u)) << 3);
            else act[j] = CHUB_ACT_LOAD((CHUB_G(const float)) ((CHUB_G(const char)) pa.actions + (uint32_t) ((idx0 + vc[j] + 2u * envc[j]) << 2)));  // row stride S0 + S1 + 2
        }
    }
    uint32_t upk = 0u;  // UNIT_DRAWS: unit tid's decoded draws
    u32x2 uraw = {0u, 0u};  // RAW: its raw draws, and
    uint32_t uprev = 0u;    //      the fourth word of its record of the step before
    if (UNIT_DRAWS) asm volatile("" : "=v"(upk));
    if (RAW) asm volatile("" : "=v"(uraw), "=v"(uprev));
    if (UNIT_DRAWS && (tid & ~63) < 2 * epb) {  // (wave-uniform: the 22 units of a workgroup of the 20 + 25 hub are the first wave's alone)
        asm volatile("" ::: "memory");
        const int ue = tid >> 1, uenv = env_first + ue;
        const uint32_t ui = ue < epb && uenv < N ? (uint32_t) ((tid & 1) ? N : 0) + (uint32_t) uenv : (uint32_t) env_first;
        if (RAW) {
            uraw = CHUB_AT(const u32x2, pa.pk, ui << 3);
            uprev = CHUB_AT(const uint32_t, pa.rec_prev, (ui << 4) + 12u);
        } else {
            upk = CHUB_AT(const uint32_t, pa.pk, ui << 2);
        }
    }
    if (HOIST_TAIL) asm volatile("" : "=v"(tail_pre[0]), "=v"(tail_pre[1]));
    if (HOIST_TAIL && wave == WAVES - 1) {  // behind everything else: the other waves' wait for the state words then leaves them in flight as well
        asm volatile("" ::: "memory");
        const int te = env_first + (lane >> 1);
        const uint32_t tenv = (uint32_t) ((lane >> 1) < epb && te < N ? te : env_first);
        const uint32_t ai = (tenv * (uint32_t) (St + 2) + (uint32_t) St) << 2;
        tail_pre[0] = CHUB_AT(const float, pa.actions, ai);
        tail_pre[1] = CHUB_AT(const float, pa.actions, ai + 4u);
    }
    if (!TAPE) {  // the new cars' Philox inputs: scalar registers from here on, requested behind the first loads
        pa.tick += sload_u32(pa.tick_base, 0);  // CHUB_TICK
        asm volatile("" : "+s"(pa.key[0]), "+s"(pa.key[1]), "+s"(pa.gid0), "+s"(pa.tick), "+s"(pa.late[0]), "+s"(pa.late[1]), "+s"(pa.late[2]),
                          "+s"(pa.late[3]), "+s"(pa.late[4]), "+s"(pa.late[5]), "+s"(pa.late[6]), "+s"(pa.late[7]));
    }
    CHUB_STAMP(1);  // first loads issued
    if (FUSED) hook.prefetch();
    if (tid == 0) q_cnt[0] = 0;
    for (int i = tid; i < (BIG ? 16 : 8 * kAccCopies) * epb; i += BLOCK) s_acc[i] = 0;
    long long *s_acc64 = (long long *) s_acc;  // BIG: {min, charge, max power, cars} as four 64-bit sums per unit

    // ---- second round trip, only for the slots whose car stays: where it is on its curve (entries n, n + 1 of its class
    // row) and the time its target SoC stands for (4 bytes of a table that sits in the vector L1), both in flight together.  A
    // car that leaves this step is wiped right after its car_step (CHS.hpp:1196-1201): nothing of it is needed, and a slot is
    // empty after remove_car (CHS.hpp:912-923 / 1077-1088) iff it had at most one slot of stay left
    uint32_t w0[T];
    int tl[T];
    bool stays[T];
    f32x4 row[T];
    float ttg[T];
    // (every state word waited for in front of the first request: a wait behind slot 0's requests could not leave them in flight
    // without leaving the draws and actions, which are older, behind)
    if (!FUSED) {
#pragma unroll
        for (int j = 0; j < T; j++) asm volatile("" : "+v"(s2[j]));
    }
    if (MASKED) {  // ... and the clock bytes, which were requested right behind them: an env the launch does not serve has no slots here
#pragma unroll
        for (int j = 0; j < T; j++) {
            asm volatile("" : "+v"(served[j]));
            valid[j] = valid[j] && served[j] != 0u;
        }
    }
#pragma unroll
    for (int j = 0; j < T; j++) {
        if (FUSED) asm volatile("" : "+v"(s2[j]));  // (the one-launch kernels: slot by slot, as their loads)
        w0[j] = valid[j] ? s2[j] : 0u;
        tl[j] = ps_tl(w0[j]);
        stays[j] = tl[j] > 1;
        asm volatile("" : "=v"(row[j]), "=v"(ttg[j]));
        if (stays[j]) {
            row[j] = CHUB_AT(const f32x4, pa.cls0, (k_[j] ? pa.cls_delta : 0u) + (ps_cls(w0[j]) << 8) + (ps_n(w0[j]) << 3));
            ttg[j] = CHUB_AT(const float, pa.ttab2, (k_[j] ? 4096u : 0u) + (ps_lev(w0[j]) << 2));
        }
    }

    CHUB_STAMP(2);  // state words here, class-row / target-time reads issued
    // ---- receive_car (CHS.hpp:1272-1316 / 1583-1627) while those are in flight
    bool empty[T];
    uint64_t be[T];
#pragma unroll
    for (int j = 0; j < T; j++) {
        empty[j] = valid[j] && !stays[j];
        be[j] = __ballot(empty[j]);
        if (lane == 0) s_ball[wave + j * WAVES] = be[j];
    }
    if (FUSED) hook.park();
    CHUB_STAMP(3);
    __syncthreads();
    CHUB_STAMP(4);  // barrier 1 passed
    // ---- every unit's empties, ONCE per unit: a lane per unit reads the ballots of the (at most two) virtual waves the unit lies in
    // and leaves, in one word, the empties in front of the unit inside its first wave, the unit's empties in that wave, its empties in
    // all -- UNIT_DRAWS: how many of them take a car, with the unit's record word in s_unit -- and which wave that is.  (Rounds 2-3 had every LANE work its unit's 64-bit masks out for itself, two popcounts and an LDS
    // read each: a third of the kernel's vector instructions.)  Stations of more than 64 piles keep that form below.
    if (!BIG) {
        for (int u = tid; u < 2 * epb; u += BLOCK) {
            const int e = u >> 1, k = u & 1;
            const int Sk = k ? S1 : S0;
            const int U0 = e * St + (k ? S0 : 0), U1 = U0 + Sk;  // the unit's virtual lanes [U0, U1) of the workgroup
            const int wv = U0 >> 6, lo = U0 & 63;
            const int hi0 = (U1 - (wv << 6)) < 64 ? (U1 - (wv << 6)) : 64;
            uint32_t info = (uint32_t) wv << 24;
            int all = 0;  // the unit's empties
            if (Sk > 0) {
                const uint64_t b0 = s_ball[wv];
                const uint64_t below_lo = lo ? (~0ull >> (64 - lo)) : 0ull, below_hi = ~0ull >> (64 - hi0);
                const int start_e = __popcll(b0 & below_lo), cnt0 = __popcll(b0 & below_hi & ~below_lo);
                const int over = U1 - ((wv + 1) << 6);  // lanes of the unit in the next virtual wave
                const int cnt1 = over > 0 ? __popcll(s_ball[wv + 1] & (~0ull >> (64 - over))) : 0;
                all = cnt0 + cnt1;
                info |= (uint32_t) start_e | ((uint32_t) cnt0 << 8) | (UNIT_DRAWS ? 0u : (uint32_t) (cnt0 + cnt1) << 16);
            }
            if (UNIT_DRAWS) {
                // assign_car (CHS.hpp:417-430), once per unit: the queue after the renege pass + the arrivals that stay, and flow_in, were decoded
                // one launch ahead (dk_make).  The third byte carries how many of the unit's empties take a car instead of how many there are.
                // (A unit past the batch's end or of an env the launch does not serve has no empties -- its lanes balloted none -- and so admits nobody.)
                if (RAW) {
                    asm volatile("" : "+v"(uraw), "+v"(uprev));
                    upk = dk_make((uint64_t) uraw.x | ((uint64_t) uraw.y << 32), pkd_line(uprev), (k ? pa.type[1] : pa.type[0]) == 0);
                } else {
                    asm volatile("" : "+v"(upk));
                }
                const int want = dk_want(upk);
                const int assign = want < all ? want : all;
                const int ln = want - assign;
                s_unit[u] = pkd_make(ln < kMaxLine ? ln : kMaxLine, dk_flow(upk), 0);
                info |= (uint32_t) assign << 16;
            }
            s_uinfo[u] = info;
        }
    }

    // ---- the occupied slots' step: urgency, feasibility / on-off, car_step, departure (CHS.hpp:1188-1202 / 1499-1513) and
    // their share of calculate_output (CHS.hpp:1233-1261 / 1544-1572) -- nothing here waits for the admission
    uint32_t w0n[T];
#pragma unroll
    for (int j = 0; j < T; j++) {
        if (BITS) asm volatile("" : "+v"(row[j]), "+v"(ttg[j]), "+v"(actw[j]));
        else asm volatile("" : "+v"(row[j]), "+v"(ttg[j]), "+v"(act[j]));
        const int u = 2 * e_[j] + k_[j];
        int *acc = s_acc + 4 * u + (BIG ? 0 : (lane & (kAccCopies - 1)) * 8 * epb);  // the unit's {min, charge power | max power, cars}: two 64-bit LDS atomics per car
        w0n[j] = 0u;
        if (stays[j]) {
            const float t_target = ttg[j];
            // action_to_real (MGR:384-393), judge_feasibility (CHS.hpp:1404-1413)
            const bool bit_on = BITS && ((((hs_[j] & 32) ? actw[j].y : actw[j].x) >> (hs_[j] & 31)) & 1u) != 0u;
            const bool on = (BITS ? bit_on : act[j] >= kActOnThreshold) || must_charge(t_target, row[j].y, tl[j]);
            const float power = on ? row[j].z : row[j].x, t_soc = on ? row[j].w : row[j].y;  // car_step = the next entry of the class row
            const int q = kw_to_fixed(power);
            const bool urgent = must_charge(t_target, t_soc, tl[j] - 1);
            w0n[j] = (w0[j] & ~kPsChg) - 1u + (on ? (kPsStep | kPsChg) : 0u);
            if (!BIG) {
                atomicAdd((unsigned long long *) (acc + 2), (unsigned long long) (uint32_t) q | (1ull << 32));
                if (on || urgent)
                    atomicAdd((unsigned long long *) acc,
                              (unsigned long long) (urgent ? (uint32_t) q : 0u) | ((unsigned long long) (on ? (uint32_t) q : 0u) << 32));
            } else {
                unsigned long long *a64 = (unsigned long long *) (s_acc64 + 4 * u);
                atomicAdd(a64 + 2, (unsigned long long) q);
                atomicAdd(a64 + 3, 1ull);
                if (urgent) atomicAdd(a64 + 0, (unsigned long long) q);
                if (on) atomicAdd(a64 + 1, (unsigned long long) q);
            }
        }
    }
    CHUB_STAMP(5);  // rows consumed, sums added
    if (!BIG) __syncthreads();  // the units' words are in
    CHUB_STAMP(6);  // barrier 2 passed

    // ---- receive_car (CHS.hpp:1272-1316 / 1583-1627): admission
    int line[T], flow[T];
    bool adm[T];
    uint64_t ba[T];
    uint32_t n_push = 0;
#pragma unroll
    for (int j = 0; j < T; j++) {
        const int vw = wave + j * WAVES;
        int empties, rank;
        if (!BIG) {
            // rank = the unit's empties in front of this lane: inside the unit's first wave, empties of the wave below the lane minus
            // those in front of the unit; in its second wave, the unit's empties of the first wave + those below the lane
            const uint32_t info = valid[j] ? s_uinfo[2 * e_[j] + k_[j]] : 0u;  // (lanes past the workgroup's last env hold no unit)
            const int m = prefix_count(be[j]);
            empties = (int) ((info >> 16) & 255u);
            rank = (int) (info >> 24) == vw ? m - (int) (info & 255u) : m + (int) ((info >> 8) & 255u);
        } else {
            const int Sk = k_[j] ? S1 : S0;
            const int ub = e_[j] * St + (k_[j] ? S0 : 0) - vw * 64, ue = ub + Sk;  // relative to this wave's lane 0
            // a unit of up to 256 lanes: its empties in every virtual wave it touches; those in earlier waves come before this lane
            empties = 0;
            rank = 0;
#pragma unroll
            for (int w = 0; w < WAVES * T; w++) {
                int lo = ub + (vw - w) * 64, hi = ue + (vw - w) * 64;  // the unit's lanes relative to wave w's lane 0
                lo = lo < 0 ? 0 : lo;
                hi = hi > 64 ? 64 : hi;
                if (hi > lo) {
                    const uint64_t m = (~0ull >> (64 - hi)) & (~0ull << lo);
                    const uint64_t b = (w == vw ? be[j] : s_ball[w]) & m;
                    empties += __popcll(b);
                    if (w < vw) rank += __popcll(b);
                    else if (w == vw) rank += prefix_count(b);
                }
            }
        }
        line[j] = 0;
        flow[j] = 0;
        int assign = 0;
        if (UNIT_DRAWS) {
            assign = empties;  // (the unit pass left min(want, empties) in that byte)
        } else if (valid[j]) {
            const uint32_t pk = pk_in[j];
            int want;
            if (RESET) {
                // the unit's initial occupancy, drawn by k_reset_levels just before.  The fast station records the raw draw, which is
                // negative for small stations (mu - 3 < 0, CHS.hpp:1617, 832-842): assign_car then admits nobody, the queue stays empty
                const bool fast = (k_[j] ? pa.type[1] : pa.type[0]) == 0;
                flow[j] = fast ? (int) (int16_t) (pk & 0xFFFFu) : (int) ((pk >> 16) & 0xFFFFu);
                want = flow[j];
            } else {
                // queue after the renege pass + the arrivals that stay, and flow_in: decoded one launch ahead, once per unit (dk_make)
                want = dk_want(pk);
                flow[j] = dk_flow(pk);
            }
            assign = want < empties ? want : empties;  // assign_car, CHS.hpp:417-430
            line[j] = want - assign;
            line[j] = line[j] < kMaxLine ? line[j] : kMaxLine;
        }
        adm[j] = empty[j] && rank < assign;
        ba[j] = __ballot(adm[j]);
        n_push += (uint32_t) __popcll(ba[j]);
    }
    if (n_push) {  // wave-uniform
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&q_cnt[0], n_push);
        base = __shfl(base, 0);
#pragma unroll
        for (int j = 0; j < T; j++) {
            if (adm[j]) q_new[base + prefix_count(ba[j])] = (uint32_t) (tid + j * BLOCK);
            base += (uint32_t) __popcll(ba[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < T; j++) {
        if (valid[j] && !adm[j]) CHUB_AT(uint32_t, pa.state, (idx0 + (uint32_t) (tid + j * BLOCK)) << 2) = w0n[j];
        if (!UNIT_DRAWS && valid[j] && slot[j] == 0) s_unit[2 * e_[j] + k_[j]] = pkd_make(line[j], flow[j], 0);
    }
    CHUB_STAMP(7);  // admission done, state stores issued
    __syncthreads();
    CHUB_STAMP(8);  // barrier 3 passed
    // Everything left -- the workgroup's new cars and, after them, the station records -- is the last wave's business: the
    // other waves are done (their wave slots go to the next workgroup instead of idling at a third barrier through the
    // Philox block and the dependent table read of the new cars).  RESET: about half of all slots get a car, so every wave
    // serves its share and the workgroup meets again in front of the records.
    constexpr bool ALL = RESET || CHUB_EPI_ALL || FUSED;  // every wave takes new cars
    if (!ALL && wave != WAVES - 1) return 0;
    if (PIPED && wave < WAVES / 2) return wave + 1;
    // ---- add_car (CHS.hpp:864-877 / 1029-1042) for the workgroup's new cars, one lane per car
    const uint32_t n_adm = q_cnt[0];
    for (uint32_t i = (uint32_t) (PIPED ? tid - (WAVES / 2) * 64 : (ALL ? tid : lane)); i < n_adm; i += (PIPED ? BLOCK - (WAVES / 2) * 64 : (ALL ? BLOCK : 64))) {
        const int src = (int) q_new[i];
        const int s_e = (int) (__umul24((uint32_t) src, pa.magic) >> 20);
        const int s_hs = src - (int) __umul24((uint32_t) s_e, (uint32_t) St);
        const int s_k = s_hs >= S0 ? 1 : 0;
        uint32_t c, lev;
        int late;
        if (TAPE) {
            const u32x2 tp = CHUB_AT(const u32x2, pa.car_tape, (idx0 + (uint32_t) src) << 3);
            c = tp.x;
            lev = tp.y & 0xFFFFu;
            late = (int) (tp.y >> 16);
        } else {
            PhiloxCtx p2{pa.key[0], pa.key[1], pa.tick, pa.gid0 + (uint32_t) (env_first + s_e)};
            const U4 o = p2.block(SITE_SOC, (uint32_t) s_hs, 0);  // word 0 SoC class, 1 target level, 2 extra stay
            c = o.v[0] >> kSocLevelShift;
            lev = o.v[1] % 1000u;
            late = 0;  // late_from_word, the first 8 thresholds from registers
#pragma unroll
            for (int j = 0; j < 8; j++) late += (o.v[2] >= pa.late[j]) ? 1 : 0;
            if (__any(o.v[2] >= pa.late[7])) {
#pragma unroll
                for (int j = 8; j < 16; j++) late += (o.v[2] >= tb.late_thr[j]) ? 1 : 0;
            }
        }
        f32x2 e0 = CHUB_AT(const f32x2, pa.cls0, (s_k ? pa.cls_delta : 0u) + (c << 8));
        float tt_ = CHUB_AT(const float, pa.ttab2, (s_k ? 4096u : 0u) + (lev << 2));  // soc_to_time(target), CHS.hpp:867 / 1032
        asm volatile("" : "+v"(e0), "+v"(tt_));  // both lookups in flight together
        int st_ = (int) ceilf(__fsub_rn(tt_, e0.y)) + late;  // calculate_min_charging_time + mk_late_time
        st_ = st_ > kMaxStay ? kMaxStay : st_;
        CHUB_AT(uint32_t, pa.state, (idx0 + (uint32_t) src) << 2) = st_ > 0 ? ps_make(st_, c, lev) : 0u;
        CHUB_AT(uint8_t, pa.stay8, idx0 + (uint32_t) src) = (uint8_t) st_;
        if (st_ > 0) {
            const int q = kw_to_fixed(e0.x);
            if (!BIG) {
                int *ac = s_acc + 4 * (2 * s_e + s_k) + (lane & (kAccCopies - 1)) * 8 * epb;
                atomicAdd((unsigned long long *) (ac + 2), (unsigned long long) (uint32_t) q | (1ull << 32));
                if (must_charge(tt_, e0.y, st_)) atomicAdd(ac, q);
            } else {
                unsigned long long *a64 = (unsigned long long *) (s_acc64 + 4 * (2 * s_e + s_k));
                atomicAdd(a64 + 2, (unsigned long long) q);
                atomicAdd(a64 + 3, 1ull);
                if (must_charge(tt_, e0.y, st_)) atomicAdd(a64 + 0, (unsigned long long) q);
            }
        }
    }
    CHUB_STAMP(9);  // new cars done
    // FUSED (k_step_fused): the workgroup's third barrier and the station records are the caller's business from here (its last wave
    // runs the first half of its envs' tails in front of them): every wave returns its role, the last wave WAVES
    if (FUSED) return wave == WAVES - 1 ? WAVES : wave + 1;
    if (ALL) {
        __syncthreads();
        CHUB_STAMP(10);  // barrier 4 passed
        CHUB_STAMP_REAL(13);
#if CHUB_TRACE
        if (sa.stamps_slot && tid == 0) {
            for (int i = 0; i <= 10; i++) sa.stamps_slot[(size_t) block_local * 16 + i] = stamp_[i];
            sa.stamps_slot[(size_t) block_local * 16 + 12] = stamp_[12];
            sa.stamps_slot[(size_t) block_local * 16 + 13] = stamp_[13];
        }
#endif
        if (wave != WAVES - 1) return 0;
    }
    packed_records<BLOCK, T, RESET, BIG, MASKED, false, BITS, RAW>(pa, block_local, s_acc, s_unit, nullptr, tail_pre);
#if CHUB_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    CHUB_STAMP(11);  // records stored: the workgroup is done
    if (sa.stamps_slot && lane == 0) sa.stamps_slot[(size_t) block_local * 16 + 11] = stamp_[11];
#endif
    return 0;
#undef CHUB_AT
}

template <int BLOCK, int T, bool TAPE, bool RESET, bool BIG, bool MASKED, bool BITS = false, bool RAW = false>
__global__ __launch_bounds__(BLOCK, (BLOCK <= 256 ? 8 : 2048 / BLOCK)) void k_slot_packed(const DevCtx *__restrict__ ctx, StepArgs sa, PackedArgs pa_in) {
    __shared__ uint32_t q_new[BLOCK * T];
    __shared__ uint32_t q_cnt[2];
    __shared__ uint64_t s_ball[BLOCK * T / 64 + 2];                   // [1 + virtual wave]: a unit's neighbouring wave may be "wave -1" or "wave WAVES"
    __shared__ __attribute__((aligned(16))) int s_acc[2 * BLOCK * T * kAccCopies];  // 2 epb <= BLOCK * T / 2 units x {min, charge, max power, cars} (BIG: as 64-bit sums, few units)
    __shared__ uint32_t s_unit[BLOCK * T / 2];                        // per unit: line | flow << 8
    __shared__ uint32_t s_uinfo[BLOCK * T / 2];                       // per unit: where its empties are and how many of them take a car (the admission's unit pass)
    if (RESET && MASKED && mask_is_empty(sa)) return;  // (a masked reset of nobody: chub_autoreset_step_device on most calls)
    // all kernel arguments this wave needs, requested in ONE batch of scalar loads at its very start (the single asm
    // statement makes every one of them live here), instead of in a chain of dependent loads in front of the first
    // vector load
    PackedArgs pa = pa_in;
    asm volatile("" : "+s"(pa.S[0]), "+s"(pa.S[1]), "+s"(pa.type[0]), "+s"(pa.type[1]), "+s"(pa.n_envs), "+s"(pa.epb), "+s"(pa.magic),
                      "+s"(pa.cls_delta), "+s"(pa.state), "+s"(pa.rec), "+s"(pa.pk), "+s"(pa.actions), "+s"(pa.cls0), "+s"(pa.ttab2));
    NoHook hook;
    (void) slot_body_packed<BLOCK, T, TAPE, RESET, BIG, MASKED, false, NoHook, BITS, false, RAW>(ctx->hp, sa, pa, ctx->tb, xcd_order(blockIdx.x, pa.xcd, MASKED ? 0u : pa.xcd) + (MASKED ? pa.blk0 : 0u), q_cnt, q_new,
                                                                                     s_ball + 1, s_acc, s_unit, hook, nullptr, s_uinfo);
}

// What the tail's first loads need, by value in the kernel arguments: one scalar load at the start of the wave instead
// of a dozen dependent hops through the context pointer in front of the load burst of this latency-bound kernel.
struct TailArgs {
    CHUB_G(const double) ou;
    CHUB_G(const double) price_noise;
    CHUB_G(const double) cap;
    CHUB_G(const int16_t) pv_day;
    CHUB_G(const int16_t) wd_day;
    CHUB_G(const uint8_t) q_len;
    CHUB_G(const uint8_t) hv_line;
    CHUB_G(const uint32_t) drw;   // this step's pre-drawn env variates
    CHUB_G(const uint8_t) drw_cnt;
    CHUB_G(uint32_t) rec;
    CHUB_G(const float) actions;
    uint32_t n_envs, act_dim, s_tot, xcd;  // xcd: the tail workgroups in XCD-aware order (xcd_order), as the slot kernel's tiles
    // the rows of this slot of the day and what the tail's Philox context needs: nothing in front of the load burst goes
    // through the context pointer (each hop there is a dependent scalar round trip of this latency-bound kernel)
    CHUB_G(const float) tail_act;  // [N][2] the tail actions as the packed slot kernel left them, or null: read the action rows
    CHUB_G(const double) pv_row;   // pvT + t_next * 100
    CHUB_G(const double) wd_row;   // wdT + t_next * 150
    CHUB_G(const double) pv_row_now;  // ... and the rows of the slot being simulated: what the previous make_state looked up
    CHUB_G(const double) wd_row_now;
    CHUB_G(const double) hy_table;
    const uint32_t *tick_base;
    double sin_t;                  // sin96[t_next] (lock-step; per-env clocks read the table)
    uint32_t key[2], gid0, pad2;
};
inline TailArgs make_tail_args(const EnvArrays &ev, const StationArrays &st, const HubParams &hp, const StepArgs &sa, const PackedPtrs &pp,
                               bool reset) {
    TailArgs ta;
    const int t_next = reset ? 0 : (sa.t + 1) % 96;
    ta.tail_act = (hp.rng_mode == MODE_PHILOX && hp.packed && !sa.load_mode && !reset) ? (CHUB_G(const float)) st.tail_act : nullptr;
    if (sa.act_bits && !reset) ta.tail_act = (CHUB_G(const float)) sa.act_tail;  // packed actions: the caller's [N][2] array is that already
    ta.pv_row = (CHUB_G(const double)) (pp.tb->pvT + t_next * 100);
    ta.wd_row = (CHUB_G(const double)) (pp.tb->wdT + t_next * 150);
    ta.pv_row_now = (CHUB_G(const double)) (pp.tb->pvT + (reset ? 0 : sa.t) * 100);
    ta.wd_row_now = (CHUB_G(const double)) (pp.tb->wdT + (reset ? 0 : sa.t) * 150);
    ta.hy_table = (CHUB_G(const double)) pp.tb->hy_table;
    ta.tick_base = hp.tick_base;
    ta.sin_t = pp.sin96[t_next];
    ta.key[0] = hp.key[0];
    ta.key[1] = hp.key[1];
    ta.gid0 = (uint32_t) hp.env_id0;
    ta.pad2 = 0;
    ta.ou = (CHUB_G(const double)) ev.ou;
    ta.price_noise = (CHUB_G(const double)) ev.price_noise;
    ta.cap = (CHUB_G(const double)) ev.cap;
    ta.pv_day = (CHUB_G(const int16_t)) ev.pv_day;
    ta.wd_day = (CHUB_G(const int16_t)) ev.wd_day;
    ta.q_len = (CHUB_G(const uint8_t)) ev.q_len;
    ta.hv_line = (CHUB_G(const uint8_t)) ev.hv_line;
    ta.drw = (CHUB_G(const uint32_t)) ev.drw[sa.tick & 1u];
    ta.drw_cnt = (CHUB_G(const uint8_t)) ev.drw_cnt[sa.tick & 1u];
    ta.rec = (CHUB_G(uint32_t)) st.rec;
    ta.actions = (CHUB_G(const float)) sa.actions;
    ta.n_envs = (uint32_t) hp.n_envs;
    ta.act_dim = (uint32_t) hp.act_dim;
    ta.s_tot = (uint32_t) (hp.S[0] + hp.S[1]);
    ta.xcd = (hp.rng_mode == MODE_PHILOX && hp.packed && hp.xcd) ? 1u : 0u;  // (COMPAT tails in this order: measured, no gain)
    return ta;
}

template <bool RESET, int MODE, int BLOCK>
__global__ __launch_bounds__(BLOCK, 7) void k_slot(const DevCtx *__restrict__ ctx, StepArgs sa, int64_t nb0) {
    const HubParams &hp = ctx->hp;
    __shared__ float lds_f[BLOCK];
    __shared__ uint32_t lds_u[2 * BLOCK];
    int k;
    int64_t bl;
    const int64_t bid = blockIdx.x;
    if (sa.station_filter >= 0) {
        k = sa.station_filter;
        bl = bid;
    } else {
        k = (bid >= nb0) ? 1 : 0;
        bl = k ? bid - nb0 : bid;
    }
    if (MODE == MODE_PHILOX) slot_body_wave<RESET, BLOCK>(hp, sa, ctx->sl, ctx->st, ctx->tb, k, bl, lds_f, lds_u);
    else if (hp.type[k] == 0) slot_body_compat<0, RESET, BLOCK>(hp, sa, ctx->sl, ctx->st, ctx->cr, ctx->tb, k, bl, lds_f, lds_u);
    else slot_body_compat<1, RESET, BLOCK>(hp, sa, ctx->sl, ctx->st, ctx->cr, ctx->tb, k, bl, lds_f, lds_u);
}

// ---------------------------------------------------------------------------------------- k_slot_curves, PHILOX_CURVES
// The third RNG mode (CHUB_RNG_PHILOX_CURVES): PHILOX's draws, keyed exactly as PHILOX keys them, with the reference's continuous arrival SoC
// and car_step evaluated on the device along the curves (car_step_curves + soc_to_time, the arithmetic COMPAT is pinned with).  Internally the
// handle is a PHILOX handle (hp.rng_mode = MODE_PHILOX: the station draws of k_draw_levels / k_reset_levels and the tail k_env<.., MODE_PHILOX>
// are reused as they are) with hp.soc_curves = 1, which sends its slot launches here instead of to k_slot_packed / k_slot.
//   slot state, hub-major [env][S0 + S1] like PHILOX's:
//     SlotArrays::hot   [NS][2] f32: power, t_soc = soc_to_time(current SoC)   (8 B read + 8 B written per slot and step)
//     SlotArrays::wrd   [NS]    u32: PHILOX's state word with the class bits zero: bits 0-4 stay left, bit 5 charging, bits 6-10 car_steps taken,
//                                    bits 22-31 target level                     (4 B read + 4 B written)
//     SlotArrays::soc0  [NS]    f32: the arrival SoC, written once at admission (introspection: init_soc, the SoC's replay), as stay8
//   a new car: the PHILOX block px.block(SITE_SOC, hub slot, 0) -- word 0 -> soc_from_word (the continuous SoC; PHILOX's class is word 0 >> 21),
//   word 1 % 1000 the target level, word 2 late_from_word.  Tape mode: car_tape's .x carries the f32 bits of the recorded arrival SoC.
// Lane = slot, wave-local units of H = pow2 >= S_k lanes (slot_body_wave's shape), one station per workgroup and the station type a template
// parameter, so the f64 branches of the curves are uniform per wave; sums as PHILOX's (integers of 2^-19 kW, DPP butterflies).
template <int TYPE, bool RESET, int BLOCK>
__device__ __forceinline__ void slot_body_curves(const HubParams &hp, const StepArgs &sa, const SlotArrays &sl, const StationArrays &st,
                                                 const Tables &tb, const int k, const int64_t block_local) {
    constexpr int WAVES = BLOCK / 64;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int H = hp.H[k], S = hp.S[k], logH = hp.logH[k];
    const int upw = 64 >> logH;
    const int uiw = lane >> logH;
    const int slot = lane & (H - 1);
    const int64_t N = hp.n_envs;
    const int env = (int) block_local * (WAVES * upw) + wave * upw + uiw;
    const bool unit_ok = env < (int) N && in_group(sa, env);
    const bool valid = unit_ok && slot < S;
    const uint64_t unit_mask = (H == 64) ? ~0ull : (((1ull << H) - 1ull) << (uiw << logH));
    const int hub_slot = (k ? hp.S[0] : 0) + slot;
    const uint32_t idx = (uint32_t) env * (uint32_t) (hp.S[0] + hp.S[1]) + (uint32_t) hub_slot;
    const uint32_t sidx = (uint32_t) k * (uint32_t) N + (uint32_t) env;
    const bool cp = hp.constant_charging != 0;

    uint32_t pk_in = 0, w0 = 0u;
    float a = 0.0f;
    f32x2 hv = {0.0f, 0.0f};
    if (unit_ok) pk_in = st.pk[sa.tick & 1u][sidx];
    if (!RESET && valid) {
        w0 = sl.wrd[idx];
        hv = *(CHUB_G(const f32x2)) ((CHUB_G(const float)) sl.hot + 2u * idx);
        a = sa.actions[(uint32_t) env * (uint32_t) hp.act_dim + (uint32_t) hub_slot];
    }
    int tl = ps_tl(w0);
    bool car = tl > 0;
    float power = hv.x, t_soc = hv.y;
    const float t_target = car ? tb.ttab[k][ps_lev(w0)] : 0.0f;
    // ---- judge_feasibility + assign_on_off_piece (CHS.hpp:1404-1413, 1364-1373)
    const bool on = car && (a >= kActOnThreshold || must_charge(t_target, t_soc, tl));
    // ---- car_step along the curves (CHS.hpp:900-905 / 1065-1070); a car that leaves this step is wiped right after it (CHS.hpp:1196-1201)
    if (on && tl > 1) {
        float soc_new;
        car_step_curves<TYPE>(__fadd_rn(t_soc, 1.0f), cp, hp.cc, soc_new, power);
        t_soc = soc_to_time<TYPE>(soc_new, cp);
        w0 += kPsStep;
    }
    w0 &= ~kPsChg;
    if (car) {  // remove_car (CHS.hpp:912-923 / 1077-1088)
        tl -= 1;
        w0 -= 1u;
        if (tl <= 0) {
            car = false;
            w0 = 0u;
            power = t_soc = 0.0f;
        }
    }
    const bool charge = on && car;
    if (charge) w0 |= kPsChg;

    // ---- receive_car (CHS.hpp:1272-1316 / 1583-1627): the unit's draws as PHILOX decodes them (draw_decoded_levels / k_reset_levels)
    const bool empty = valid && !car;
    const uint64_t be = __ballot(empty) & unit_mask;
    const int empties = __popcll(be);
    const int rank = prefix_count(be);
    Received rc = {0, 0, 0};
    if (unit_ok) rc = receive_car_word<RESET>(pk_in, TYPE == 0, empties);
    float tgt = t_target;
    if (empty && rank < rc.assign) {  // add_car (CHS.hpp:864-877 / 1029-1042)
        float soc;
        uint32_t lev;
        int late;
        if (sa.car_tape) {
            const uint32_t *tp = sa.car_tape + 2u * idx;
            soc = __uint_as_float(tp[0]);
            lev = tp[1] & 0xFFFFu;
            late = (int) (tp[1] >> 16);
        } else {
            const U4 o = car_block(hp, sa, env, hub_slot);
            soc = soc_from_word(tb.soc_d_icdf, o.v[0]);
            lev = o.v[1] % 1000u;
            late = late_from_word(tb.late_thr, o.v[2]);
        }
        tgt = tb.ttab[k][lev];
        t_soc = soc_to_time<TYPE>(soc, cp);
        power = time_to_power<TYPE>(t_soc, cp);
        int stay = (int) ceilf(__fsub_rn(tgt, t_soc)) + late;  // calculate_min_charging_time + mk_late_time
        stay = stay > kMaxStay ? kMaxStay : stay;  // (never binds on the mode's own draws: chub_create refuses curves whose stays could pass kMaxStay, chub.h; a car tape may carry any extra stay)
        tl = stay;
        car = tl > 0;
        w0 = car ? ps_make(stay, 0u, lev) : 0u;
        sl.stay8[idx] = (uint8_t) stay;
        sl.soc0[idx] = soc;
    }

    // ---- calculate_output (CHS.hpp:1233-1261 / 1544-1572): PHILOX's order-independent integer sums
    const bool urgent = car && must_charge(tgt, t_soc, tl);
    const int q = kw_to_fixed(power);
    int i_min = urgent ? q : 0, i_max = car ? q : 0, i_chg = charge ? q : 0;
    unit_sums_dpp(H, i_min, i_max, i_chg);
    const int cars = __popcll(__ballot(car) & unit_mask);

    if (valid) {
        sl.wrd[idx] = w0;
        const f32x2 out = {car ? power : 0.0f, car ? t_soc : 0.0f};
        *(CHUB_G(f32x2)) ((CHUB_G(float)) sl.hot + 2u * idx) = out;
    }
    if (unit_ok && slot == 0) rec_store(st.rec, sidx, fixed_to_kw(i_min), fixed_to_kw(i_chg), fixed_to_kw(i_max), pkd_make(rc.line, rc.flow, cars));
}

template <bool RESET, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_slot_curves(const DevCtx *__restrict__ ctx, StepArgs sa, int64_t nb0) {
    const HubParams &hp = ctx->hp;
    const int64_t bid = blockIdx.x;
    const int k = (bid >= nb0) ? 1 : 0;  // one station per workgroup: the type below is uniform over it
    const int64_t bl = k ? bid - nb0 : bid;
    if (hp.type[k] == 0) slot_body_curves<0, RESET, BLOCK>(hp, sa, ctx->sl, ctx->st, ctx->tb, k, bl);
    else slot_body_curves<1, RESET, BLOCK>(hp, sa, ctx->sl, ctx->st, ctx->tb, k, bl);
}

// ---------------------------------------------------------------------------------------- COMPAT, the split step
// One kernel per station with the unit's first lane walking the env's streams keeps 2 of a wave's 64 lanes busy through the longest
// part of the step (every polar normal of the reference's std::normal_distribution costs a lane about a microsecond): 250 of the
// 279 us of a step at 65 536 envs.  Large batches therefore run
//   (k_compat_empties lane = slot: how many slots of each unit are empty once this step's departures are out -- a slot is empty after
//                     remove_car iff it had at most one slot of stay left, CHS.hpp:912-923 / 1077-1088 -- all the walk needs of the slots;
//                     only where the previous pass was not a split one: k_slot_split leaves the counts for the next step itself)
//   k_compat_walk     lane = ENV, 64 walks per wave: station 0's draws, then station 1's, in the reference's consumption order
//                     (receive_car, CHS.hpp:1272-1316 / 1583-1627; the forecourt's follow in the tail kernel as before), leaving per
//                     unit flow / cars admitted / queue and per admitted car its three variates
//   k_slot_split      lane = slot, both stations in ONE launch: everything else (slot_body_compat<.., SPLIT>)
// Same streams, same order, same arithmetic as the one-kernel-per-station form (chub_options.slot_kernel = 1 keeps that one:
// the parity cross-check; handles of a few envs run k_compat_small).
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_compat_empties(const DevCtx *__restrict__ ctx, StepArgs sa, int64_t nb0) {
    const HubParams &hp = ctx->hp;
    const int64_t bid = blockIdx.x;
    const int k = (bid >= nb0) ? 1 : 0;
    const int64_t bl = k ? bid - nb0 : bid;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int U = hp.U[k], S = hp.S[k];  // (the unit layout of slot_body_compat)
    const int upw = 64 / U, uiw = lane / U, slot = lane - uiw * U;
    const int env = (int) bl * ((BLOCK / 64) * upw) + wave * upw + uiw;
    const bool unit_ok = uiw < upw && env < (int) hp.n_envs && in_group(sa, env);
    const bool valid = unit_ok && slot < S;
    const uint64_t unit_mask = (U == 64) ? ~0ull : (uiw < upw ? (((1ull << U) - 1ull) << (uiw * U)) : 0ull);
    uint32_t w = 0u;
    if (valid) w = ctx->sl.hot[4 * ((size_t) hp.base[k] + (size_t) env * (size_t) S + (size_t) slot) + 3];  // (slot indices go up to 2^31: 64-bit word index)
    const bool empty = valid && (int) (w & 127u) <= 1;  // (hot_tl spelt out: through the function this kernel comes out with another schedule)
    const uint64_t be = __ballot(empty) & unit_mask, be2 = __ballot(valid && (int) (w & 127u) <= 2) & unit_mask;
    if (unit_ok && slot == 0) {
        ctx->st.empt[(uint32_t) k * (uint32_t) hp.n_envs + (uint32_t) env] = (uint8_t) __popcll(be);
        // ... and what the slot pass of the step before this one would have left for the walk of the step behind this one (empt2)
        ctx->st.empt2[(sa.tick + 1u) & 1u][(uint32_t) k * (uint32_t) hp.n_envs + (uint32_t) env] = (uint8_t) __popcll(be2);
    }
}

// The walk of ONE env: station 0's draws, then station 1's, in the reference's consumption order (receive_car, CHS.hpp:1272-1316 /
// 1583-1627), leaving per unit flow / cars admitted / queue (StationArrays::fa) and per admitted car its three variates (SlotArrays::var)
// FORECOURT (k_compat_walk / k_env_walk): the env's forecourt draws of the step follow the stations' in the streams (hvs_step inside hy_step,
// HYD:250-260, behind both evs_step calls, MGR:149-180): the arrival level, then one mk_soc per arrival -- made here as well and left in
// EnvArrays::hv_pre for the tail, which then does not touch the streams at all
template <bool RESET, typename Stream, bool FORECOURT = false>
__device__ __forceinline__ void compat_walk_env(const DevCtx *__restrict__ ctx, const StepArgs &sa, const int env, Stream &rs) {
    const HubParams &hp = ctx->hp;
    const Tables &tb = ctx->tb;
    const StationArrays &st = ctx->st;
    const int64_t N = hp.n_envs;
    const uint32_t St = (uint32_t) (hp.S[0] + hp.S[1]);
    const uint32_t par = sa.tick & 1u;  // the step the draws belong to: its buffers
    const bool far = !RESET && sa.walk_far != 0;
    const bool cp = hp.constant_charging != 0;
    for (int k = 0; k < 2; k++) {
        const int S = hp.S[k];
        const bool fast = hp.type[k] == 0;
        const uint32_t sidx = (uint32_t) k * (uint32_t) N + (uint32_t) env;
        int line = 0, empties = S;
        if (far) {
            // two steps ahead of the slots (StepArgs::walk_far): the queue as the previous step's walk left it, and the slots that will be
            // empty = those with at most two slots of stay left when the step before that one ended, minus the cars the previous step's
            // walk admits, plus those of them that stay one slot at most
            const uint32_t wp = st.fa[par ^ 1u][sidx];
            line = (int) (wp >> 24);
            empties = (int) st.empt2[par][sidx] - (int) ((wp >> 16) & 255u) + (int) st.shrt[par ^ 1u][sidx];
        } else if (!RESET) {
            line = pkd_line(st.rec[4u * sidx + 3u]);
            empties = (int) st.empt[sidx];
        }
        const Received rc = receive_car_streams<RESET>(rs, hp, sa, tb, k, env, fast, line, empties);
        CHUB_G(u32x4) var = (CHUB_G(u32x4)) ctx->sl.var[par] + 2u * ((uint32_t) env * St + (uint32_t) (k ? hp.S[0] : 0));
        int n_short = 0;
        for (int rr = 0; rr < rc.assign; rr++) {  // ascending slot order == ascending rank
            const CarDraw d = draw_car_streams(rs);
            // add_car HERE, where the car's variates are in registers: every lane of the walk that still has a car to draw evaluates it, while
            // in the slot pass the one lane in fifteen that admits a car made its whole wave pay for the f64 curve work (round 6: 250 of a slot
            // wave's 813 vector instructions)
            const NewCar nc = add_car_compat(fast, d.soc, d.lev, d.late, cp);
            var[2 * rr] = u32x4{__float_as_uint(nc.power), __float_as_uint(nc.t_target), __float_as_uint(nc.t_soc), (uint32_t) nc.stay | ((uint32_t) d.lev << 7)};
            var[2 * rr + 1] = u32x4{__float_as_uint(d.soc), 0u, 0u, 0u};
            // (what a walk two steps ahead needs of this step's admissions: how many of them stay one slot at most)
            n_short += (nc.stay <= 1) ? 1 : 0;
        }
        st.fa[par][sidx] = ((uint32_t) rc.flow & 0xFFFFu) | ((uint32_t) (rc.assign > 0 ? rc.assign : 0) << 16) | ((uint32_t) rc.line << 24);
        if (sa.walk_short) st.shrt[par][sidx] = (uint8_t) n_short;
    }
    if (FORECOURT && !RESET) {
        const int t_env = sa.env_clk ? clk_t(env_clk(sa, N, env)) : sa.t;
        CHUB_G(uint32_t) hv = ctx->ev.hv_pre[sa.tick & 1u] + (uint32_t) env * (uint32_t) hp.hv_w;
        const int arrive = (int) tb.cnt_hv[(uint32_t) t_env * (uint32_t) kLevels + (uint32_t) rs.level()];
        hv[0] = (uint32_t) arrive;
        for (int j = 0; j < arrive; j++) hv[1 + j] = __float_as_uint(arrive_soc_from(rs.normal_d(7.0, 3.0)));  // (arrive < hv_w: chub_create)
    }
}

// ---- the dense walk (round 6): the walk of 64 envs by ONE WAVE, in two kinds of phase.
// What is serial in a walk is the streams, and the streams are touched by cheap integer work only: the level draws, and the rejection loops of
// the polar normals (CompatStreamT::polar_d / polar_f).  What is expensive -- per new car two f64 logs, two divisions, two square roots and
// add_car's curve work, some 400 vector instructions -- depends on nothing but the accepted points.  With one env per lane all the way
// (compat_walk_env) a wave pays those 400 instructions once per car of its BUSIEST env (8 + 5 passes on an average step of the bench hub for
// 3 + 1.5 cars per env) on a chain that is the split step's long pole.  Here: phase A, lane = env, draws the raw points of up to kWalkCap cars
// into the wave's staging area in LDS (compacted: car j of the lanes that still have one, lane order); phase B, lane = CAR, evaluates them
// densely packed (3 + 2 passes) and writes the new cars where the slot pass looks for them.  Rounds repeat while any env has cars left.
// Same streams, same order of draws per env, the same phase functions as compat_walk_env, which k_compat_small (a handful of envs on one
// wave's lanes) keeps.  walk_rounds is the one form that does not call draw_car_streams: it takes a car's variates in two halves (the accepted
// points here, the transforms by another lane), which normal_d / normal_f are defined as (CompatStreamT).
constexpr int kWalkCap = 256;
constexpr int kWalkStageWords = kWalkCap * 7 + 64;  // per staged car: y, r2 of the SoC normal (f64), y, r2 of the extra-stay normal (f32), a word; + one counter per lane
struct WalkStage {
    double *yd, *r2d;
    float *yf, *r2f;
    uint32_t *meta;  // target level (10 bits) | owner lane << 10 | the car's admission rank << 16
    uint32_t *cnt;   // [64] per owner lane: cars of the round's station that stay one slot at most
};
__device__ __forceinline__ WalkStage walk_stage(uint32_t *base) {  // base: 8-byte aligned, kWalkStageWords words
    WalkStage g;
    g.yd = (double *) base;
    g.r2d = g.yd + kWalkCap;
    g.yf = (float *) (g.r2d + kWalkCap);
    g.r2f = g.yf + kWalkCap;
    g.meta = (uint32_t *) (g.r2f + kWalkCap);
    g.cnt = g.meta + kWalkCap;
    return g;
}
__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// KIND 0: a station's new cars (variates + add_car, written to SlotArrays::var / var_soc of env0 + owner lane); KIND 1: the forecourt's
// arrivals (one SoC normal each, written to EnvArrays::hv_pre).  `want`: how many the lane's env has to draw (0: none / no env).  All 64 lanes call.
template <int KIND, typename Stream>
__device__ __forceinline__ void walk_rounds(const DevCtx *__restrict__ ctx, const StepArgs &sa, Stream &rs, const WalkStage &sg, const int lane, const uint32_t env0,
                                            const int want, const int k, const bool fast) {
    const HubParams &hp = ctx->hp;
    const uint32_t St = (uint32_t) (hp.S[0] + hp.S[1]);
    const uint32_t par = sa.tick & 1u;
    const bool cp = hp.constant_charging != 0;
    int rr = 0;
    while (__any(want - rr > 0)) {
        const int rem = want - rr;
        // ---- phase A, lane = env: the raw points of the env's next cars -- as many per env as the staging area holds for all (the largest
        // quota Q with sum over envs of min(cars left, Q) <= kWalkCap), filed ENV BY ENV: lane l's cars at base_l .. base_l + q_l - 1, so
        // that phase B's neighbouring lanes hold one env's consecutive admission ranks and their records leave as one run of memory
        int Q = 0;
        {
            int total = 0;
            for (int j = 0;; j++) {
                const int c = __popcll(__ballot(rem > j));
                if (c == 0 || total + c > kWalkCap) break;  // (j = 0 always fits: c <= 64)
                total += c;
                Q = j + 1;
            }
        }
        const int mine = rem < Q ? (rem > 0 ? rem : 0) : Q;
        int base_l = mine;  // exclusive prefix sum of `mine` over the lanes (Hillis-Steele over the wave)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(base_l, d);
            if (lane >= d) base_l += up;
        }
        const int base = __shfl(base_l, 63);  // cars staged this round
        base_l -= mine;
        for (int j = 0; j < Q; j++) {
            if (j < mine) {
                const int i = base_l + j;
                double yd, r2d;
                rs.polar_d(yd, r2d);  // the SoC normal's accepted point (mk_soc, CHS.hpp:804-814 / HYD:259)
                sg.yd[i] = yd;
                sg.r2d[i] = r2d;
                uint32_t lev = 0u;
                if (KIND == 0) {
                    lev = (uint32_t) rs.level();  // target level (CHS.hpp:35-44)
                    float yf, r2f;
                    rs.polar_f(yf, r2f);          // mk_late_time's accepted point (CHS.hpp:816-830)
                    sg.yf[i] = yf;
                    sg.r2f[i] = r2f;
                }
                sg.meta[i] = lev | ((uint32_t) lane << 10) | ((uint32_t) (rr + j) << 16);
            }
        }
        wave_sync_lds();
        // ---- phase B, lane = car
        for (int i = lane; i < base; i += 64) {
            const uint32_t w = sg.meta[i];
            const uint32_t owner = (w >> 10) & 63u, rank = w >> 16;
            const float soc = arrive_soc_from(Stream::normal_of_polar_d(sg.yd[i], sg.r2d[i], 7.0, 3.0));
            if (KIND == 0) {
                const int lev = (int) (w & 1023u);
                int late = (int) roundf(Stream::normal_of_polar_f(sg.yf[i], sg.r2f[i], 2.0f, 2.0f));  // mk_late_time("slow")
                late = late < 0 ? 0 : late;
                const NewCar nc = add_car_compat(fast, soc, lev, late, cp);
                const uint32_t vi = (env0 + owner) * St + (uint32_t) (k ? hp.S[0] : 0) + rank;
                // ONE 32-byte record per new car (the hot record's four words + the arrival SoC): a sector written whole; neighbouring lanes hold
                // the same env's next admission ranks (the staging area is filled env by env), so a unit's records leave as one run
                ((CHUB_G(u32x4)) ctx->sl.var[par])[2u * vi] =
                    u32x4{__float_as_uint(nc.power), __float_as_uint(nc.t_target), __float_as_uint(nc.t_soc), (uint32_t) nc.stay | ((uint32_t) lev << 7)};
                ((CHUB_G(u32x4)) ctx->sl.var[par])[2u * vi + 1u] = u32x4{__float_as_uint(soc), 0u, 0u, 0u};
                // (what a walk two steps ahead needs of this step's admissions: how many of them stay one slot at most)
                if (nc.stay <= 1) atomicAdd(&sg.cnt[owner], 1u);
            } else {
                ctx->ev.hv_pre[par][(env0 + owner) * (uint32_t) hp.hv_w + 1u + rank] = __float_as_uint(soc);  // (rank < arrivals < hv_w: chub_create)
            }
        }
        wave_sync_lds();
        rr += mine;
    }
}

// The walk of 64 envs by one wave (lane = env in the serial phases): station 0's draws, then station 1's, then the forecourt's, in the
// reference's consumption order -- what compat_walk_env<.., FORECOURT = true> does for one env, with the new cars evaluated densely (above).
// live: the lane has an env to walk (inside the batch and named by the call).  All 64 lanes call.
template <bool RESET, typename Stream>
__device__ __forceinline__ void compat_walk_wave(const DevCtx *__restrict__ ctx, const StepArgs &sa, const uint32_t env0, const int lane, const bool live,
                                                 Stream &rs, uint32_t *stage_words) {
    const HubParams &hp = ctx->hp;
    const Tables &tb = ctx->tb;
    const StationArrays &st = ctx->st;
    const int64_t N = hp.n_envs;
    const uint32_t par = sa.tick & 1u;  // the step the draws belong to: its buffers
    const bool far = !RESET && sa.walk_far != 0;
    const int env = (int) env0 + lane;
    const WalkStage sg = walk_stage(stage_words);
    sg.cnt[lane] = 0u;
    wave_sync_lds();
    for (int k = 0; k < 2; k++) {
        const int S = hp.S[k];
        const bool fast = hp.type[k] == 0;
        const uint32_t sidx = (uint32_t) k * (uint32_t) N + (uint32_t) env;
        int as = 0, fl = 0, new_line = 0;
        if (live) {
            int line = 0, empties = S;
            if (far) {  // (two steps ahead of the slots: see compat_walk_env)
                const uint32_t wp = st.fa[par ^ 1u][sidx];
                line = (int) (wp >> 24);
                empties = (int) st.empt2[par][sidx] - (int) ((wp >> 16) & 255u) + (int) st.shrt[par ^ 1u][sidx];
            } else if (!RESET) {
                line = pkd_line(st.rec[4u * sidx + 3u]);
                empties = (int) st.empt[sidx];
            }
            const Received rc = receive_car_streams<RESET>(rs, hp, sa, tb, k, env, fast, line, empties);
            fl = rc.flow;
            new_line = rc.line;
            as = rc.assign > 0 ? rc.assign : 0;
        }
        walk_rounds<0>(ctx, sa, rs, sg, lane, env0, as, k, fast);
        if (live) {
            st.fa[par][sidx] = ((uint32_t) fl & 0xFFFFu) | ((uint32_t) as << 16) | ((uint32_t) new_line << 24);
            if (sa.walk_short) st.shrt[par][sidx] = (uint8_t) sg.cnt[lane];
        }
        sg.cnt[lane] = 0u;  // (read and cleared by its own lane; the next station's phase B comes behind a wave barrier)
    }
    if (!RESET) {
        int arrive = 0;
        if (live) {
            const int t_env = sa.env_clk ? clk_t(env_clk(sa, N, env)) : sa.t;
            arrive = (int) tb.cnt_hv[(uint32_t) t_env * (uint32_t) kLevels + (uint32_t) rs.level()];
            ctx->ev.hv_pre[par][(uint32_t) env * (uint32_t) hp.hv_w] = (uint32_t) arrive;
        }
        walk_rounds<1>(ctx, sa, rs, sg, lane, env0, arrive, 0, false);
    }
}

// One workgroup's NW walks (256; k_slot_walk2: 64, one wave): the rings parked in LDS, walked, and the streams' state behind the draws
// written to the SHADOW of the step the draws belong to -- the stream buffer behind the committed one (CompatRng::g3 / minstd3: three buffers in
// rotation, StepArgs::rng_cur names the committed one): when the slot pass of that step has been launched the host moves rng_cur on, which IS
// the commit -- nothing is copied.  A walk two steps ahead (StepArgs::walk_far) starts from the previous step's shadow, rng_cur + 1, instead of the
// committed streams and writes rng_cur + 2.
template <bool RESET, int NW = 256, int LANES = NW>  // NW envs walked by LANES threads (LANES = 64 > NW = 32: half a wave's lanes walk, all of them evaluate the new cars)
__device__ __forceinline__ void compat_walk_block(const DevCtx *__restrict__ ctx, const StepArgs &sa, const uint32_t blk, uint32_t *s_ring, uint32_t *s_stage,
                                                  const uint32_t tid = threadIdx.x) {  // tid: the thread's number among the block's LANES; s_stage: LANES / 64 staging areas of kWalkStageWords
    static_assert(LANES >= NW && LANES % 64 == 0 && (NW % 64 == 0 || LANES == 64), "whole waves; a block of fewer than 64 envs is one wave");
    const int64_t N = ctx->hp.n_envs;
    const bool far = !RESET && sa.walk_far != 0;
    const uint32_t b_src = ((uint32_t) sa.rng_cur + (far ? 1u : 0u)) % 3u, b_dst = (b_src + 1u) % 3u;
    const uint32_t *g_src = (const uint32_t *) ctx->cr.g3[b_src];
    const uint32_t *m_src = (const uint32_t *) ctx->cr.minstd3[b_src];
    uint32_t *m_dst = (uint32_t *) ctx->cr.minstd3[b_dst];
    // the glibc rings of the workgroup's envs (128 bytes each, one contiguous run of memory) are parked in LDS for the walk: transposed, so
    // that the lanes of a wave hit different banks when each reads a word of its own ring
    const uint32_t env0 = blk * (uint32_t) NW;
    const uint32_t n_here = (uint32_t) N - env0 < (uint32_t) NW ? (uint32_t) N - env0 : (uint32_t) NW;
    {
        const u32x4 *src = (const u32x4 *) (g_src + (size_t) env0 * 32u);
        for (uint32_t j = tid; j < n_here * 8u; j += (uint32_t) LANES) {
            const u32x4 q = src[j];
            const uint32_t l = j >> 3, w = (j & 7u) << 2;
            s_ring[(w + 0u) * (uint32_t) NW + l] = q.x;
            s_ring[(w + 1u) * (uint32_t) NW + l] = q.y;
            s_ring[(w + 2u) * (uint32_t) NW + l] = q.z;
            s_ring[(w + 3u) * (uint32_t) NW + l] = q.w;
        }
    }
    __syncthreads();
    // (64 walks per wave: fewer -- 32 or 16 envs per wave, more waves -- measured slower: 115 / 129 vs 110 us per step at 65 536 envs)
    const int env = (int) (env0 + tid);
    const bool has_env = tid < (uint32_t) NW && env < (int) N;
    const bool live = has_env && in_group(sa, env);
    {
        CompatStreamT<RingLdsT<NW>> rs;
        rs.r.s = s_ring + (tid < (uint32_t) NW ? tid : 0u);
        rs.gf = rs.gr = 0u;
        rs.x = 1u;
        if (has_env) {
            rs.gf = rs.r.get(31);
            rs.gr = (rs.gf + 28u) % 31u;
            rs.x = m_src[env];  // (an env the call does not name: its streams as they are, in the shadow too)
        }
        compat_walk_wave<RESET>(ctx, sa, env0 + (tid & ~63u), (int) (tid & 63u), live, rs, s_stage + (tid >> 6) * (uint32_t) kWalkStageWords);
        if (has_env) {
            rs.r.set(31, rs.gf);
            m_dst[env] = rs.x;
        }
    }
    __syncthreads();
    {
        u32x4 *dst = (u32x4 *) (ctx->cr.g3[b_dst] + (size_t) env0 * 32u);
        for (uint32_t j = tid; j < n_here * 8u; j += (uint32_t) LANES) {
            const uint32_t l = j >> 3, w = (j & 7u) << 2;
            dst[j] = u32x4{s_ring[(w + 0u) * (uint32_t) NW + l], s_ring[(w + 1u) * (uint32_t) NW + l], s_ring[(w + 2u) * (uint32_t) NW + l],
                           s_ring[(w + 3u) * (uint32_t) NW + l]};
        }
    }
}

template <bool RESET>
__global__ __launch_bounds__(256) void k_compat_walk(const DevCtx *__restrict__ ctx, StepArgs sa) {
    __shared__ __attribute__((aligned(16))) uint32_t s_ring[32 * 256];
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[4 * kWalkStageWords];
    compat_walk_block<RESET>(ctx, sa, blockIdx.x, s_ring, s_stage);
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK, 7) void k_slot_split2(const DevCtx *__restrict__ ctx, StepArgs sa, int64_t nb0) {
    const HubParams &hp = ctx->hp;
    const int64_t bid = blockIdx.x;
    const int k = (bid >= nb0) ? 1 : 0;
    const int64_t bl = k ? bid - nb0 : bid;
    __shared__ float lds[(BLOCK / 64) * (3 * 128 + 16)];
    if (hp.type[k] == 0) slot_body_split2<0, BLOCK>(hp, sa, ctx->sl, ctx->st, ctx->cr, ctx->tb, k, bl, lds);
    else slot_body_split2<1, BLOCK>(hp, sa, ctx->sl, ctx->st, ctx->cr, ctx->tb, k, bl, lds);
}

// The slot pass of step i and the stream walks of step i + 1 in ONE launch: the walk -- one serial chain per env, a wave per SIMD for 20 to
// 40 us -- no longer stands between two slot passes but runs in the shadow of one.  It cannot look at what the slot pass beside it leaves,
// and does not need to: who leaves depends on the stays alone, so the slots that will be empty for step i + 1 are those with at most two
// slots of stay left after step i - 1 (StationArrays::empt2, left by that step's pass) minus the cars step i admits (its walk's word) plus
// those of them that stay one slot at most (StationArrays::shrt, from that walk: make_car's arithmetic); the queue is in that word too,
// and the streams continue from step i's shadow, which the slot pass beside it is committing (StepArgs::walk_far).  Workgroups
// [0, nwalk): 64 (or 32) walks each, on one wave (8 KB of rings + 7 KB of staging in LDS: a larger area would cost the slot workgroups their occupancy),
// at raised priority; the others: slot_body_split2.
#ifndef CHUB_WALK2_OCC
#define CHUB_WALK2_OCC 7  // workgroups per CU of k_slot_walk2 (sets its register budget: 72 VGPRs at 7, 80 at 6, 96 at 5)
#endif
template <int BLOCK, int kWalk2Envs>
__global__ __launch_bounds__(BLOCK, CHUB_WALK2_OCC) void k_slot_walk2(const DevCtx *__restrict__ ctx, StepArgs sa, StepArgs sw, int64_t nb0, int nwalk) {
    constexpr int kWords = (BLOCK / 64) * (3 * 128 + 16) > 32 * kWalk2Envs + kWalkStageWords ? (BLOCK / 64) * (3 * 128 + 16) : 32 * kWalk2Envs + kWalkStageWords;
    __shared__ __attribute__((aligned(16))) float lds[kWords];  // a walk workgroup: 8 KB of rings + the walking wave's staging area
    if ((int) blockIdx.x < nwalk) {
        // one wave of the workgroup walks, the others end at once (ended waves do not count at its barriers) -- the wave whose number is
        // the workgroup's modulo 4, so that the walks of the workgroups a CU receives do not all sit on the same SIMD
        if ((threadIdx.x >> 6) != (blockIdx.x & 3u)) return;
        __builtin_amdgcn_s_setprio(3);
        compat_walk_block<false, kWalk2Envs, 64>(ctx, sw, blockIdx.x, (uint32_t *) lds, (uint32_t *) lds + 32 * kWalk2Envs, threadIdx.x & 63u);
        return;
    }
    const HubParams &hp = ctx->hp;
    const int64_t bid = (int64_t) blockIdx.x - nwalk;
    const int k = (bid >= nb0) ? 1 : 0;
    const int64_t bl = k ? bid - nb0 : bid;
    if (hp.type[k] == 0) slot_body_split2<0, BLOCK>(hp, sa, ctx->sl, ctx->st, ctx->cr, ctx->tb, k, bl, lds);
    else slot_body_split2<1, BLOCK>(hp, sa, ctx->sl, ctx->st, ctx->cr, ctx->tb, k, bl, lds);
}

template <bool RESET, int BLOCK>
__global__ __launch_bounds__(BLOCK, 7) void k_slot_split(const DevCtx *__restrict__ ctx, StepArgs sa, int64_t nb0) {
    const HubParams &hp = ctx->hp;
    const int64_t bid = blockIdx.x;
    const int k = (bid >= nb0) ? 1 : 0;
    const int64_t bl = k ? bid - nb0 : bid;
    __shared__ float lds_f[BLOCK];  // (the scalar-load mode's rank pass: the only user of the scratch areas here)
    __shared__ uint32_t lds_u[2 * BLOCK];
    if (hp.type[k] == 0) slot_body_compat<0, RESET, BLOCK, true>(hp, sa, ctx->sl, ctx->st, ctx->cr, ctx->tb, k, bl, lds_f, lds_u);
    else slot_body_compat<1, RESET, BLOCK, true>(hp, sa, ctx->sl, ctx->st, ctx->cr, ctx->tb, k, bl, lds_f, lds_u);
}

// ----------------------------------------------------------------------------------------- k_env
// SAE J2601 target pressure (HYD:338-388 on the table HYD:232-233)
__device__ __forceinline__ double j2601_target(double p) {
    const double X[10] = {0.50, 5.00, 10.0, 15.0, 20.0, 30.0, 40.0, 50.0, 60.0, 70.0};
    const double Y[10] = {87.4, 81.0, 86.8, 86.1, 85.4, 83.8, 82.2, 80.4, 78.5, 76.1};
    if (p < X[1]) return Y[0];
    double r = p;
    bool hit = false;
#pragma unroll
    for (int a = 0; a < 8; a++) {
        const bool in = (a < 7) ? (X[1 + a] <= p && p < X[2 + a]) : (X[1 + a] <= p && p <= X[2 + a]);
        if (in && !hit) {
            r = (Y[2 + a] - Y[1 + a]) / (X[2 + a] - X[1 + a]) * (p - X[1 + a]) + Y[1 + a];
            hit = true;
        }
    }
    return r;
}
// x / c for a divisor known ahead of time, without the ~35-instruction division sequence on the tail's dependent chain:
// q = x * RN(1/c), one exact residual, one correction (Markstein; Brisebarre, Muller, Raina 2004).  The result is the
// correctly rounded quotient except for isolated (divisor-specific) x where it is one ulp off -- 1e-16 relative on f64
// values whose parity bar is 1e-5.
__device__ __forceinline__ double div_c(double x, double c, double rc) {
    const double q = x * rc;
    const double r = __fma_rn(-q, c, x);
    return __fma_rn(r, rc, q);
}
#define DIV_K(x, c) div_c((x), (double) (c), 1.0 / (double) (c))  // literal divisor: reciprocal folded at compile time

__device__ __forceinline__ double pressure_to_mass(double p) { return (6.3 * 1000) * DIV_K(p, 70); }  // HYD:390-391
// HYD:308-321
__device__ __forceinline__ void j2601_time_mass(double p0, double &time_need, double &mass_need) {
    const double target = j2601_target(p0);
    if (p0 < 5) time_need = DIV_K(69 - p0, 18.5) + (87.4 - 69) / 7.2;
    else time_need = (5 <= p0 && p0 < 70) ? DIV_K(target - p0, 18.5) : (target - p0) / 0.0;
    mass_need = pressure_to_mass(target) - pressure_to_mass(p0);
}

__device__ __forceinline__ void fcev_time_mass(float socf, double &tn, double &mn) {
    double soc = (double) socf;
    if (soc < 0.5) soc = 0.5;
    const double p0 = (soc * 0.01) * 70;  // _soc_to_pressure HYD:302-306
    j2601_time_mass(p0, tn, mn);
}

__device__ __forceinline__ double ou_sample(double &state, double theta, double sigma, double z) {  // REN:71-76
    const double dx = theta * (0.0 - state) + sigma * z;
    state += dx;
    return state;
}

#define CHUB_TEL(i, v)                                        \
    do {                                                      \
        if (tel_on) ev.telem[(size_t) (i) * (size_t) N + (size_t) env] = (v); \
    } while (0)

// The per-env tail of step() / reset(), lane = env.
constexpr int kEnvBlock = 256;  // compile-time (reading blockDim.x fetches the AQL packet)

// ---- the per-env tail of step() / reset() for one env per lane: the body of k_env (tables staged in LDS between the
// load burst and the arithmetic).
// What the tail of one env reads of its own state (PHILOX step).  k_step_fused requests it for the last wave's envs together with
// the wave's first slot loads, a whole slot pass ahead of its use.
struct TailIn {
    double ou_pv, ou_wd, ou_price, price_noise, cap;
    float a_el, a_fc;
    int pv_day, wd_day, q_len, hv_line;
    u32x4 drw;
    uint32_t drw_n;
};
__device__ __forceinline__ void tail_prefetch(TailIn &in, const TailArgs &ta, const uint32_t e32, const bool predrawn) {
    const uint32_t n32 = ta.n_envs;
    in.ou_pv = ta.ou[e32];
    in.ou_wd = ta.ou[n32 + e32];
    in.ou_price = ta.ou[2u * n32 + e32];
    in.price_noise = ta.price_noise[e32];
    if (ta.tail_act) {  // packed actions: the two tail actions have an array of their own
        typedef float f32x2_ __attribute__((ext_vector_type(2)));
        const f32x2_ tv = ((CHUB_G(const f32x2_)) ta.tail_act)[e32];
        in.a_el = tv.x;
        in.a_fc = tv.y;
    } else {
        const uint32_t ai = e32 * ta.act_dim + ta.s_tot;
        in.a_el = ta.actions[ai];
        in.a_fc = ta.actions[ai + 1u];
    }
    in.cap = ta.cap[e32];
    in.pv_day = ta.pv_day[e32];
    in.wd_day = ta.wd_day[e32];
    in.q_len = ta.q_len[e32];
    in.hv_line = ta.hv_line[e32];
    if (predrawn) {
        in.drw = ((CHUB_G(const u32x4)) ta.drw)[e32];
        in.drw_n = ta.drw_cnt[e32];
    }
}

// A pair of steps in one lane (k_env_pair): what the first step's tail hands to the second -- the env's carried state in registers, and the second
// step's other inputs (its station records, tail actions, pre-drawn variates, its element of the next slot's table rows), requested with the
// first step's load burst so that the launch pays one cold round trip
struct TailNext {
    TailIn in;
    u32x4 r0, r1;
    double st_pv, st_wd;
};

// FUSED (k_step_fused): one WAVE runs the tails of up to 64 envs of its workgroup right behind their station records: the table rows
// are already in LDS (the caller's), the two records come from LDS (s_rec, [2 * local env + station]), `row` = the lane's place
// among the wave's output rows, env0 = the env of row 0, and the only synchronisation is the wave's own.
// The tail has two halves: what does not look at the station records (the slot's exogenous values, the FCEV forecourt, the exogenous
// update for the next slot) and what does (clamp, hydrogen step, netting, fuel cell, money, observation).  mid() is called between
// them by every lane: nothing in k_env; in k_step_fused the workgroup's third barrier and the record pass, so that the last wave's
// first half runs while the workgroup's first wave is still busy with the new cars.
struct NoMid {
    __device__ __forceinline__ void operator()() {}
    __device__ __forceinline__ void at1() {}  // (more places every lane with an env passes: k_steps_piped's tail wave meets the slot waves at some of them)
    __device__ __forceinline__ void at2() {}
    __device__ __forceinline__ void at3() {}
};
// EB: lanes of the workgroup that calls it (k_env: kEnvBlock; k_compat_small: its 512)
// TAPE (the parity instrument of include/chub.h, PHILOX handles): the tail's variates come from the caller -- the exogenous normals
// (sa.exo_z, f64 as the reference's numpy drew them), a reset's days (sa.exo_days), the forecourt's arrivals and their SoCs (sa.hv_tape) --
// and everything else is the production tail, instruction for instruction.
// FCEV arrivals of env e at slot of day t and level `lev` on a handle with per-env hub parameters: the host's expression behind Tables::cnt_hv
// (chub_create_ex) with the env's own rate -- the same f32 product and rounding, so the count is bit for bit the per-handle table's
__device__ __forceinline__ uint32_t hv_count_rate(float rate, uint32_t n) {  // ... of arrival index n at that rate (k_forecast sums over the indices)
    const int c = (int) roundf(rate * (float) n);
    return (uint32_t) (c < 0 ? 0 : (c > 255 ? 255 : c));
}
__device__ __forceinline__ uint32_t hv_count_env(const EnvParamArrays &ep, uint32_t e, int t, uint32_t lev) {
    return hv_count_rate(ep.hv_rate[e], (uint32_t) ep.hv_idx[(uint32_t) t * (uint32_t) kLevels + lev]);
}

// EP (ENV_PARAMS, handles made by chub_create_params): the hydrogen, fuel-cell, fluctuation and FCEV constants are the env's own (DevCtx::ep, read
// in the first load burst) and the electrolyser table is the env's row of EnvArrays::hy_env instead of the block's LDS copy
// PAIR (k_env_pair): 1 = the first step of a pair: it also requests the second step's inputs (ta2: that step's arguments) and leaves them, with the
// env's state as it stands behind this step, in nx; 2 = the second step: everything comes from nx (`pre` = nx->in), its table rows of "now" are the
// first step's rows of "next" (the caller passes those LDS arrays) and only the next slot's rows are parked
template <bool RESET, int MODE, bool MULTI, bool FUSED = false, typename Mid = NoMid, int EB = kEnvBlock, bool TAPE = false, bool EP = false, int PAIR = 0>
__device__ __forceinline__ void env_tail(const DevCtx *__restrict__ ctx, const StepArgs &sa, const int env, const bool live,
                                         const double *s_pv, const double *s_wd, const double *s_pv_now, const double *s_wd_now,
                                         const double *s_hy, const uint8_t *s_hv, float *s_out, const int env_block, const TailArgs &ta,
                                         const u32x4 *s_rec, const int local_env, const int env0_fused, const int rows_fused,
                                         const TailIn &pre, const bool use_pre, Mid &mid, TailNext *nx = nullptr, const TailArgs *ta2 = nullptr) {
    static_assert(PAIR == 0 || (!RESET && MODE == MODE_PHILOX && !MULTI && !FUSED && !TAPE && !EP), "pairs: the lock-step PHILOX step of the stand-alone tail");
    const HubParams &hp = ctx->hp;
    const EnvArrays &ev = ctx->ev;
    const CompatRng &cr = ctx->cr;
    const Tables &tb = ctx->tb;
    const int64_t N = hp.n_envs;  // (through the context pointer on purpose: round 5 measured the step 0.1 us SLOWER with this and hp.telemetry taken from
                                  // the kernel arguments -- the first touch of the context then comes later, in the middle of the dependent chain)
    // the clock of this lane's env: the launch's (lock-step), or its group's (per-env clocks: table rows then come straight
    // from global memory instead of the LDS copy of "the" slot of the day)
    constexpr bool multi = MULTI;  // its own instantiation: the lock-step kernel carries none of this
    const uint32_t my_clk = (multi && env < (int) N) ? env_clk(sa, N, env) : 0u;
    if (multi && env < (int) N)  // every env's clock moves to the other buffer: one step on, back to 0, or as it is
        sa.env_clk[(int64_t) ((sa.tick + 1u) & 1u) * N + env] = (uint16_t) (!live ? my_clk : (RESET ? 0u : clk_next(my_clk)));
    const int t_now = multi ? clk_t(my_clk) : sa.t;
    const int t_next = RESET ? 0 : (t_now + 1) % 96;
    const bool draw_price = multi ? ((my_clk >> 8) & 3u) == 0u : sa.draw_price != 0;
    const double price_last = multi ? tb.price[RESET ? 95 : t_now] : sa.price_last;
    const double price_prev = multi ? tb.price[(t_now + 95) % 96] : sa.price_prev;  // what the previous make_state saw as price[-1]
#define TAB_PV(d) (multi ? tb.pvT[t_next * 100 + (d)] : s_pv[d])
#define TAB_WD(d) (multi ? tb.wdT[t_next * 150 + (d)] : s_wd[d])
#define TAB_PV_NOW(d) (multi ? tb.pvT[t_now * 100 + (d)] : s_pv_now[d])
#define TAB_WD_NOW(d) (multi ? tb.wdT[t_now * 150 + (d)] : s_wd_now[d])
#define TAB_HY(i) ((MODE == MODE_COMPAT || EP) ? hy_env[i] : s_hy[i])
#define HP_E(field, own) (EP ? (own) : hp.field)  // a hub constant: the handle's, or (EP) the env's
#define TAB_HV(l) (EP ? hv_count_env(ctx->ep, e32, t_now, (uint32_t) (l)) : multi ? tb.cnt_hv[(uint32_t) t_now * (uint32_t) kLevels + (uint32_t) (l)] : s_hv[l])
    // ---- prefetch: every per-env input is requested before the table staging and its barrier, and the PHILOX
    // words that do not depend on state (FCEV arrival level, the three OU normals) are drawn here too, so the
    // memory latencies of this latency-bound kernel overlap instead of queueing behind one another.
    const uint32_t e32 = (uint32_t) env, n32 = ta.n_envs;
    CHUB_STAMP_DECL(16);
    CHUB_STAMP_REAL(8);
    CHUB_STAMP(0);
#if CHUB_TRACE
    {
        uint32_t n_ = n32;
        asm volatile("" : "+s"(n_));
        CHUB_STAMP(1);  // kernel arguments here
    }
#endif
    // the table rows of this slot of the day (PV, wind, hy_table; COMPAT: FCEV counts) go out first, one element per lane, in
    // the same burst as the state loads: one memory round trip for everything (they are parked in LDS further down)
    double st_pv = 0.0, st_wd = 0.0, st_hy = 0.0, st_pv_now = 0.0, st_wd_now = 0.0;
    uint32_t st_hv = 0;
    const double sin_t = multi ? tb.sin96[t_next] : ta.sin_t;  // the observation's time feature
    // bit 0: telemetry; bit 1: the per-episode ledger (chub_set_episode_stats) -- EpisodeArrays::on, mirrored into this word so that the tail
    // learns both from ONE scalar load in a cache line it reads anyway, not from a load of its own at the far end of the context in front
    // of the per-env burst (the two compared: DESIGN 6.9)
    const int32_t tel_word = hp.telemetry;
    const bool tel_on = (tel_word & 1) != 0;
    const bool ep_on = (tel_word & 2) != 0;
    if (!FUSED) {
        const int i = threadIdx.x;
        if (PAIR == 2) {  // requested by the pair's first step
            st_pv = nx->st_pv;
            st_wd = nx->st_wd;
        } else if (!multi) {  // lock-step: the rows of the launch's slot of the day
            if (i < 100) st_pv = ta.pv_row[i];
            if (i < 150) st_wd = ta.wd_row[i];
            if (!RESET) {
                if (i < 100) st_pv_now = ta.pv_row_now[i];
                if (i < 150) st_wd_now = ta.wd_row_now[i];
            }
            if (PAIR == 1) {
                nx->st_pv = nx->st_wd = 0.0;
                if (i < 100) nx->st_pv = ta2->pv_row[i];
                if (i < 150) nx->st_wd = ta2->wd_row[i];
            }
        }
        if (!RESET && PAIR != 2) {
            if (!EP && i < 102) st_hy = ta.hy_table[i];
            // (the split step's tail does not look the forecourt's arrivals up -- the walk did: no table row, and no hop through the context
            // pointer for its address in front of the per-env loads)
            if (MODE == MODE_COMPAT && !EP && !multi && !sa.hv_tape && i < kLevels / 4) st_hv = ((CHUB_G(const uint32_t)) tb.cnt_hv)[sa.t * (kLevels / 4) + i];
        }
    }
    // The device-side tick offset of graph replays is a scalar load from DEVICE memory (a miss in the scalar cache of every CU at the start of a
    // launch), and a wave cannot wait for its scalar loads one by one: issued here it sat in front of the per-env loads below, which wait for
    // kernel arguments (round 5: the compiler's s_waitcnt lgkmcnt(0) in front of the burst waited for it -- two round trips in a row).  The
    // steady-state PHILOX step needs the tick only for the forecourt's later arrivals, so it asks for the offset BEHIND the burst.
    constexpr bool tick_late = MODE == MODE_PHILOX && !RESET && !TAPE;
    const bool tick_now = MODE == MODE_PHILOX && (!tick_late || sa.fresh != 0);
    PhiloxCtx px{ta.key[0], ta.key[1], tick_now ? sa.tick + sload_u32(ta.tick_base, 0) : sa.tick, ta.gid0 + (uint32_t) env};
    double cap = 0.0, in_price_noise = 0.0;
    double ou_pv = 0.0, ou_wd = 0.0, ou_price = 0.0, z_pv = 0.0, z_wd = 0.0, z_pr = 0.0;
    float a_el_f = 0.0f, a_fc_f = 0.0f, P0f = 0.0f, P1f = 0.0f, mn0 = 0.0f, mx0 = 0.0f, mn1 = 0.0f, mx1 = 0.0f;
    int pv_day = 0, wd_day = 0, q_len = 0, hv_line = 0, F0i = 0, F1i = 0, ln0 = 0, ln1 = 0, hv_lev = 0, hv_arrive = 0;
    u32x4 drw_raw = {0u, 0u, 0u, 0u};
    uint32_t drw_n = 0u, hvw0 = 0u, hvw1 = 0u;
    const bool have_pre = (FUSED || PAIR == 2) && use_pre;  // the env's own state came in ahead of time (tail_prefetch; PAIR: from the step before)
    double p_v_h_max = 0.0, p_cells = 0.0, p_rc_cells = 0.0, p_cap_mass = 0.0, p_rc_cap_mass = 0.0, p_init_soc = 0.0, p_hydro_loss = 0.0;
    double p_fc_max_power = 0.0, p_renew_fluct1 = 0.0, p_price_fluct1 = 0.0;
    if (live) {
        if (EP) {  // the env's own constants, with its state
            CHUB_G(const double) pr = ctx->ep.prm;
            p_cap_mass = pr[PRM_CAP_MASS * n32 + e32];
            p_renew_fluct1 = pr[PRM_RENEW_FLUCT1 * n32 + e32];
            p_price_fluct1 = pr[PRM_PRICE_FLUCT1 * n32 + e32];
            if (RESET) {
                p_init_soc = pr[PRM_INIT_SOC * n32 + e32];
            } else {
                p_v_h_max = pr[PRM_V_H_MAX * n32 + e32];
                p_cells = pr[PRM_CELLS * n32 + e32];
                p_rc_cells = pr[PRM_RC_CELLS * n32 + e32];
                p_rc_cap_mass = pr[PRM_RC_CAP_MASS * n32 + e32];
                p_hydro_loss = pr[PRM_HYDRO_LOSS * n32 + e32];
                p_fc_max_power = pr[PRM_FC_MAX_POWER * n32 + e32];
            }
        }
        if (have_pre) {
            ou_pv = pre.ou_pv; ou_wd = pre.ou_wd; ou_price = pre.ou_price; in_price_noise = pre.price_noise;
        } else {
            ou_pv = ta.ou[e32];
            ou_wd = ta.ou[n32 + e32];
            ou_price = ta.ou[2u * n32 + e32];
            in_price_noise = ta.price_noise[e32];
        }
        if (PAIR == 2) {
            const u32x4 v0 = nx->r0, v1 = nx->r1;
            mn0 = __uint_as_float(v0.x); P0f = __uint_as_float(v0.y); mx0 = __uint_as_float(v0.z); ln0 = pkd_line(v0.w); F0i = pkd_flow(v0.w);
            mn1 = __uint_as_float(v1.x); P1f = __uint_as_float(v1.y); mx1 = __uint_as_float(v1.z); ln1 = pkd_line(v1.w); F1i = pkd_flow(v1.w);
        } else if (!FUSED) {  // (FUSED: the records are read from LDS behind mid(), where this workgroup writes them)
            const StationRec r0 = rec_load(ta.rec, e32), r1 = rec_load(ta.rec, n32 + e32);
            mn0 = r0.mn; P0f = r0.chg; mx0 = r0.mx; ln0 = pkd_line(r0.pkd); F0i = pkd_flow(r0.pkd);
            mn1 = r1.mn; P1f = r1.chg; mx1 = r1.mx; ln1 = pkd_line(r1.pkd); F1i = pkd_flow(r1.pkd);
        }
        if (!RESET && have_pre) {
            a_el_f = pre.a_el; a_fc_f = pre.a_fc; cap = pre.cap;
            pv_day = pre.pv_day; wd_day = pre.wd_day; q_len = pre.q_len; hv_line = pre.hv_line;
        } else if (!RESET) {
            if (ta.tail_act) {
                typedef float f32x2_ __attribute__((ext_vector_type(2)));
                const f32x2_ tv = ((CHUB_G(const f32x2_)) ta.tail_act)[e32];
                a_el_f = tv.x;
                a_fc_f = tv.y;
            } else {
                const uint32_t ai = e32 * ta.act_dim + ta.s_tot;
                a_el_f = ta.actions[ai];
                a_fc_f = ta.actions[ai + 1u];
            }
            cap = ta.cap[e32];
            pv_day = ta.pv_day[e32];
            wd_day = ta.wd_day[e32];
            q_len = ta.q_len[e32];
            hv_line = ta.hv_line[e32];
        }
        if (MODE == MODE_COMPAT && !RESET && sa.hv_tape) {  // the split step: the forecourt's draws wait where the walk left them -- the count and
            hvw0 = sa.hv_tape[e32 * (uint32_t) sa.hv_w];    // the first arrival's SoC with the burst, not as two round trips of their own behind it
            if (sa.hv_w > 1) hvw1 = sa.hv_tape[e32 * (uint32_t) sa.hv_w + 1u];
        }
        if (TAPE) {
            z_pv = sa.exo_z[e32 * 3u + 0u];
            z_wd = sa.exo_z[e32 * 3u + 1u];
            z_pr = sa.exo_z[e32 * 3u + 2u];
            if (!RESET) hv_arrive = (int) sa.hv_tape[e32 * (uint32_t) sa.hv_w];
        } else if (MODE == MODE_PHILOX && !RESET && !sa.fresh) {
            // this step's state-independent env draws (three OU normals, FCEV arrival count) were made one launch ahead by
            // the level blocks of k_env (draw_env_levels): 350 dependent instructions less on this latency-bound chain
            if (have_pre) {
                drw_raw = pre.drw;
                drw_n = pre.drw_n;
            } else {
                drw_raw = ((CHUB_G(const u32x4)) ta.drw)[e32];  // unpacked behind the table staging: no wait for it here
                drw_n = ta.drw_cnt[e32];
            }
        } else if (MODE == MODE_PHILOX) {
            const U4 ow = px.block(SITE_OU, 0, 0);  // word 0 pv, 1 wind, 2 price
            z_pv = (double) normal_from_word(tb.normal_icdf, tb.normal_tail, ow.v[0]);
            z_wd = (double) normal_from_word(tb.normal_icdf, tb.normal_tail, ow.v[1]);
            z_pr = (double) normal_from_word(tb.normal_icdf, tb.normal_tail, ow.v[2]);
            if (!RESET) {
                // the FCEV arrival level is state-independent: look its count up now, one byte straight from the table
                hv_lev = (int) (px.block(SITE_HV, 0, 0).v[0] % 1000u);
                hv_arrive = EP ? (int) hv_count_env(ctx->ep, e32, t_now, (uint32_t) hv_lev)
                               : (int) tb.cnt_hv[(uint32_t) t_now * (uint32_t) kLevels + (uint32_t) hv_lev];
            }
        } else {
            z_pv = sa.exo_z[e32 * 3u + 0u];
            z_wd = sa.exo_z[e32 * 3u + 1u];
            z_pr = sa.exo_z[e32 * 3u + 2u];
        }
        if (PAIR == 1) {  // the second step's inputs, behind this step's own requests: its waits leave them in flight
            typedef float f32x2_ __attribute__((ext_vector_type(2)));
            nx->r0 = ((CHUB_G(const u32x4)) ta2->rec)[e32];
            nx->r1 = ((CHUB_G(const u32x4)) ta2->rec)[n32 + e32];
            const f32x2_ tv = ((CHUB_G(const f32x2_)) ta2->tail_act)[e32];
            nx->in.a_el = tv.x;
            nx->in.a_fc = tv.y;
            nx->in.drw = ((CHUB_G(const u32x4)) ta2->drw)[e32];
            nx->in.drw_n = ta2->drw_cnt[e32];
        }
    }


    if (tick_late && !tick_now) {
        const uint32_t *tbp = ta.tick_base;
        asm volatile("" : "+s"(tbp) : : "memory");  // (not to be hoisted above the loads issued so far)
        px.tick += sload_u32(tbp, 0);
    }
    if (!FUSED) {
        // the table rows requested at the top arrive with the state loads; park them in LDS
        static_assert(EB >= 150, "one table element per lane");
        CHUB_STAMP(2);  // load burst issued
        const int i = threadIdx.x;
        if (i < 100) ((double *) s_pv)[i] = st_pv;
        if (i < 150) ((double *) s_wd)[i] = st_wd;
        if (!RESET && PAIR != 2) {
            if (i < 100) ((double *) s_pv_now)[i] = st_pv_now;
            if (i < 150) ((double *) s_wd_now)[i] = st_wd_now;
            if (!EP && i < 102) ((double *) s_hy)[i] = st_hy;
            if (MODE == MODE_COMPAT && !EP && i < kLevels / 4) ((uint32_t *) s_hv)[i] = st_hv;
        }
        __syncthreads();
    }
    CHUB_STAMP(3);  // rows parked, barrier passed: the loads have landed
    if (!TAPE && MODE == MODE_PHILOX && !RESET && !sa.fresh) {
        z_pv = (double) __uint_as_float(drw_raw.x);
        z_wd = (double) __uint_as_float(drw_raw.y);
        z_pr = (double) __uint_as_float(drw_raw.z);
        hv_arrive = (int) drw_n;
    }
    // stand-alone kernel: output rows go through LDS so that the workgroup writes its kEnvBlock consecutive rows (one
    // contiguous run of memory) with coalesced stores instead of 15 scattered 4-byte stores per lane
    const int row_w = sa.obs_stride;  // D (dense) or D + 2 (packed: obs, reward, done)
    auto flush_rows = [&]() {
        if (FUSED) {  // the wave's own rows: wave-level synchronisation only
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            float *dst = sa.obs + (size_t) env0_fused * (size_t) row_w;
            const int total = rows_fused * row_w;
            if ((((uintptr_t) dst) & 15u) == 0) {  // 16 bytes per lane and store: the wave's last dependent LDS round trips, a quarter as many
                typedef float f32x4 __attribute__((ext_vector_type(4)));
                const int quads = total >> 2;
                for (int i = (int) (threadIdx.x & 63u); i < quads; i += 64) ((f32x4 *) dst)[i] = ((const f32x4 *) s_out)[i];
                for (int i = (quads << 2) + (int) (threadIdx.x & 63u); i < total; i += 64) dst[i] = s_out[i];
            } else {
                for (int i = (int) (threadIdx.x & 63u); i < total; i += 64) dst[i] = s_out[i];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();  // s_out is reused by the wave's next group of envs
            return;
        }
        __syncthreads();
        const int env0 = env_block * EB;
        const int rows = (int) N - env0 < EB ? (int) N - env0 : EB;
        float *dst = sa.obs + (size_t) env0 * (size_t) row_w;
        const int total = rows * row_w;
        // per-env clocks: only the rows of the envs this launch serves (whole block served: the plain path)
        if (MULTI && sa.env_mask && !__syncthreads_and((live || env >= (int) N) ? 1 : 0)) {
            for (int i = threadIdx.x; i < total; i += EB)
                if (in_group(sa, env0 + i / row_w)) dst[i] = s_out[i];
        } else if ((((uintptr_t) dst) & 15u) == 0) {  // 16 bytes per lane and store: a quarter of the store instructions
            typedef float f32x4 __attribute__((ext_vector_type(4)));
            const int quads = total >> 2;
            for (int i = threadIdx.x; i < quads; i += EB) ((f32x4 *) dst)[i] = ((const f32x4 *) s_out)[i];
            for (int i = (quads << 2) + threadIdx.x; i < total; i += EB) dst[i] = s_out[i];
        } else {
            for (int i = threadIdx.x; i < total; i += EB) dst[i] = s_out[i];
        }
    };
    // what the first half hands to the second
    const double *hy_env = (MODE == MODE_COMPAT || EP) ? (const double *) ev.hy_env + (size_t) e32 * 102u : nullptr;
    (void) hy_env;
    // COMPAT: the env's own hy_power_speed_list entry the electrolyser clamp looks at first (MGR:160-180; its index follows from the action
    // alone) is requested HERE, in front of the first half, instead of as a round trip of its own in the second
    double hy_req_pre = 0.0;
    if ((MODE == MODE_COMPAT || EP) && !RESET && live) {
        int rq = (int) ceil((((double) a_el_f + 1) / 2) * 100);
        rq = rq < 0 ? 0 : (rq > 101 ? 101 : rq);
        hy_req_pre = hy_env[rq];
    }
    const double cap_mass = HP_E(cap_mass, p_cap_mass);
    double store_soc = 0.0, reward = 0.0, in_re_pv = 0.0, in_re_wd = 0.0, in_price_next = 0.0, total_mass_need = 0.0;
    double re_pv = 0.0, re_wd = 0.0, price_next = 0.0;
    int arrive = 0;
    uint32_t fold_n = 0;
    // ---- first half.  One pass of a do/while (here and below) so that lanes without an env skip the work but still reach mid()
    // and the workgroup barrier of flush_rows() at the same program point as everybody else
    do {
    if (!live) break;

    // COMPAT: the forecourt's draws either continue the env's streams here (one kernel per station, k_compat_small), or -- the split step --
    // were made by the walk behind the stations' and wait in sa.hv_tape (the tail then does not touch the streams)
    const bool hv_walked = MODE == MODE_COMPAT && sa.hv_tape != nullptr;
    CompatStream rs;
    if (MODE == MODE_COMPAT && !RESET && !hv_walked) rs.load(cr, sa.rng_cur, env);

    if (RESET) {
        // renew_reset (REN:51-53) + hy_reset (HYD:197-208)
        if (MODE == MODE_COMPAT || TAPE) {
            pv_day = sa.exo_days[e32 * 2u + 0u];
            wd_day = sa.exo_days[e32 * 2u + 1u];
        } else {
            const U4 o = px.block(SITE_DAY, 0, 0);
            pv_day = (int) (o.v[0] % 100u);
            wd_day = (int) (o.v[1] % 150u);
        }
        ev.pv_day[e32] = (int16_t) pv_day;
        ev.wd_day[e32] = (int16_t) wd_day;
        ev.q_len[e32] = 0;
        ev.hv_line[e32] = 0;
        cap = HP_E(init_soc, p_init_soc) * cap_mass;
        store_soc = HP_E(init_soc, p_init_soc);
        CHUB_TEL(4, cap);
        if (ep_on) {  // a new episode: the live block starts over (MGR:305-306); the finished block, the counter and the flag stay
            CHUB_G(double) lv = ctx->es.live;
#pragma unroll
            for (int c = 0; c < kEpCount; c++) lv[(size_t) c * n32 + e32] = c == EPC_END_SOC ? store_soc : 0.0;
        }
    } else {
        // What the previous make_state (MGR:344-361: the end of the previous step, or reset) produced for THIS slot is not kept as
        // state but re-derived, operation for operation, from what it was computed from: the table rows of this slot of the day,
        // the OU states as that make_state left them (the values loaded above), the price noise and the tariff it saw last.
        {
            double tp = TAB_PV_NOW(pv_day);
            if (tp > 0 && (pv_day % 2) == 0) tp += ou_pv * HP_E(renew_fluct1, p_renew_fluct1);  // REN:38-43
            in_re_pv = (tp > 0 ? tp : 0.0) * 5;
            double tw = TAB_WD_NOW(wd_day);
            tw += ou_wd * HP_E(renew_fluct1, p_renew_fluct1);                 // REN:45-49
            in_re_wd = (tw > 0 ? tw : 0.0) * 1;
        }
        in_price_next = price_prev + in_price_noise;            // MGR:354-359
        // ---- hvs_step (HYD:253-285): FCEV arrivals -> J2601 -> 15-minute FIFO.  The reference's waiting list is unbounded.
        // Here: up to hp.qcap explicit entries, which is all a list that still gets served can hold (after a partial serve
        // it keeps at most arrive - 1 of the step's arrivals, HYD:270-279), plus -- once no prefix fits any more (nobody is
        // served again until reset) -- a folded tail: entry count and the running sums of time and mass in
        // the reference's left-to-right order, so that sum(needed_time_list) / sum(needed_hy_list) stay bit-identical.
        const int qcap = hp.qcap;
        double *qt = (double *) ev.q_time + (size_t) e32 * (size_t) qcap, *qm = (double *) ev.q_mass + (size_t) e32 * (size_t) qcap;
        if (MODE == MODE_COMPAT && !hv_walked) hv_lev = rs.level();
        arrive = MODE == MODE_COMPAT ? (hv_walked ? (int) hvw0 : (int) TAB_HV(hv_lev)) : hv_arrive;
        double total_mass = 0.0;
        const bool fcev_pre = !TAPE && MODE == MODE_PHILOX && !RESET && !sa.fresh;
        // the first arrival's SoC was drawn one launch ahead with the other env draws (level_block: same Philox counter); its
        // fueling time and mass follow from it alone
        double pre_tn = 0.0, pre_mn = 0.0;
        if (fcev_pre && arrive > 0) fcev_time_mass(__uint_as_float(drw_raw.w), pre_tn, pre_mn);
        bool stuck = (hv_line & 128) != 0;
        hv_line &= 127;
        if (fcev_pre && q_len == 0 && !stuck && arrive == 1 && pre_tn <= 15.0) {
            // the common case by far: an empty FIFO, one arrival, served within the slot (hvs_step leaves the FIFO empty and
            // the line at 0, HYD:281-283) -- nothing to read from or write to the queue arrays
            total_mass = pre_mn;
            if (hv_line != 0) {
                ev.hv_line[e32] = 0;
                hv_line = 0;
            }
        } else if (q_len > 0 || stuck || arrive > 0) {
            double total_time = 0.0;
            if (stuck) {  // q_len == 0: everything is folded
                total_time = ev.q_fold[2u * e32];
                total_mass = ev.q_fold[2u * e32 + 1u];
                fold_n = ev.q_fold_cnt[e32];
            }
            for (int i = 0; i < q_len; i++) {
                total_time += qt[i];
                total_mass += qm[i];
            }
            for (int j = 0; j < arrive; j++) {
                double tn, mn;
                if (fcev_pre && j == 0) {
                    tn = pre_tn;
                    mn = pre_mn;
                } else {
                    float socf;
                    if (hv_walked && j == 0) socf = __uint_as_float(hvw1);
                    else if (TAPE || hv_walked) socf = __uint_as_float(sa.hv_tape[e32 * (uint32_t) sa.hv_w + 1u + (uint32_t) j]);
                    else if (MODE == MODE_COMPAT) socf = arrive_soc_from(rs.normal_d(7.0, 3.0));
                    else socf = soc_from_word(tb.soc_d_icdf, px.block(SITE_HVSOC, (uint32_t) j, 0).v[0]);
                    fcev_time_mass(socf, tn, mn);
                }
                if (stuck) {
                    fold_n++;
                } else if (q_len < qcap) {  // always (qcap = 2 * max arrivals per step - 1, chub_create)
                    qt[q_len] = tn;
                    qm[q_len] = mn;
                    q_len++;
                }
                total_time += tn;
                total_mass += mn;
            }
            int hv_num = 0;
            if (total_time > 15.0) {
                bool found = false;
                if (!stuck) {
                    for (int i = 1; i <= arrive - 1; i++) {
                        int keep = q_len - i;
                        keep = keep < 0 ? 0 : keep;
                        double part = 0.0;
                        for (int j = 0; j < keep; j++) part += qt[j];
                        if (part <= 15.0) {
                            hv_line = i;
                            hv_num = keep;
                            found = true;
                            break;
                        }
                    }
                }
                if (found) {
                    for (int j = hv_num; j < q_len; j++) {
                        qt[j - hv_num] = qt[j];
                        qm[j - hv_num] = qm[j];
                    }
                    q_len -= hv_num;
                } else {
                    // no prefix fits: the list only grows from here on (every later prefix contains this one), so its entries
                    // are never looked at one by one again -- fold them
                    fold_n += (uint32_t) q_len;
                    q_len = 0;
                    stuck = true;
                    ev.q_fold[2u * e32] = total_time;
                    ev.q_fold[2u * e32 + 1u] = total_mass;
                    ev.q_fold_cnt[e32] = fold_n;
                }
            } else {
                hv_line = 0;
                q_len = 0;
            }
            ev.q_len[e32] = (uint8_t) q_len;
            ev.hv_line[e32] = (uint8_t) (hv_line | (stuck ? 128 : 0));
        } else if (hv_line != 0) {
            ev.hv_line[e32] = 0;  // empty FIFO, no arrivals: total time 0 <= 15 -> line = 0 (HYD:281-283)
            hv_line = 0;
        }
        total_mass_need = total_mass;
        if (PAIR == 1) {
            nx->in.q_len = q_len;
            nx->in.hv_line = hv_line | (stuck ? 128 : 0);  // (the byte in memory: the line, and whether the list is stuck)
        }
    }
    mid.at1();

    // ---- make_state (MGR:344-361), the exogenous update for the NEXT slot: it looks at neither records nor actions, so it sits in
    // the first half (same operations in the same order as when it followed the reward: every chain is its own)
    {
        double temp = TAB_PV(pv_day);
        if (temp > 0 && (pv_day % 2) == 0) {  // REN:38-43
            temp += ou_sample(ou_pv, .01, 1., z_pv) * HP_E(renew_fluct1, p_renew_fluct1);
            ev.ou[e32] = ou_pv;
        }
        re_pv = (temp > 0 ? temp : 0.0) * 5;
        temp = TAB_WD(wd_day);
        temp += ou_sample(ou_wd, .01, 1.5, z_wd) * HP_E(renew_fluct1, p_renew_fluct1);  // REN:45-49
        ev.ou[n32 + e32] = ou_wd;
        re_wd = (temp > 0 ? temp : 0.0) * 1;
        if (draw_price) {  // MGR:354-357
            price_next = ou_sample(ou_price, .1, 0.005, z_pr) * HP_E(price_fluct1, p_price_fluct1);
            ev.ou[2u * n32 + e32] = ou_price;
            ev.price_noise[e32] = price_next;
            if (PAIR == 1) nx->in.price_noise = price_next;
            price_next += price_last;
        } else {
            price_next = price_last + in_price_noise;
            if (PAIR == 1) nx->in.price_noise = in_price_noise;
        }
    }
    if (MODE == MODE_COMPAT && !RESET && !hv_walked) rs.store(cr, sa.rng_cur, env);
    } while (0);

    CHUB_STAMP(4);  // first half (exogenous values, forecourt, next slot's exogenous update) done
    mid();  // k_step_fused: the workgroup's third barrier + the station records (by this wave); nothing elsewhere
    if (FUSED && live) {  // the records this workgroup has just written, from LDS
        const u32x4 v0 = s_rec[2 * local_env], v1 = s_rec[2 * local_env + 1];
        mn0 = __uint_as_float(v0.x); P0f = __uint_as_float(v0.y); mx0 = __uint_as_float(v0.z); ln0 = pkd_line(v0.w); F0i = pkd_flow(v0.w);
        mn1 = __uint_as_float(v1.x); P1f = __uint_as_float(v1.y); mx1 = __uint_as_float(v1.z); ln1 = pkd_line(v1.w); F1i = pkd_flow(v1.w);
    }

    // ---- second half
    do {
    if (!live) break;
    if (!RESET) {
        const double a_el = ((double) a_el_f + 1) / 2;  // action_real[-1] <- action[-2]  (MGR:400-403)
        const double a_fc = ((double) a_fc_f + 1) / 2;  // action_real[-2] <- action[-1]  (MGR:395-398)
        const double P0 = (double) P0f, P1 = (double) P1f;
        const double F0 = (double) F0i, F1 = (double) F1i;
        double re_new_power = in_re_wd + in_re_pv;    // MGR:143
        const double charging_power = 0.0 + P0 + P1;  // MGR:157
        // ---- electrolyser request clamp against the grid limit (MGR:160-180)
        double hy_power_limit = 2000 + re_new_power - charging_power;
        hy_power_limit = hy_power_limit > 0 ? hy_power_limit : 0.0;
        double act_el = a_el;
        int req = (int) ceil(a_el * 100);
        req = req < 0 ? 0 : (req > 101 ? 101 : req);  // actions outside [-1,1] would index out of the table
        if (((MODE == MODE_COMPAT || EP) ? hy_req_pre : TAB_HY(req)) > hy_power_limit) {
            int ind = 0;
            while (ind < 102 && !(TAB_HY(ind) >= hy_power_limit)) ind++;
            // hy_power_speed_list_input[ind - 1]; python index -1 wraps to the last entry (1.0)
            act_el = (ind >= 102 || ind == 0) ? 0.01 * 100 : 0.01 * (ind - 1);
        }
        {
        // ---- hy_step (HYD:160-195): production clamp, electrolyser + compressor power, tank
        double must_chg = cap_mass * 0.1 - cap;
        must_chg = must_chg > 0 ? must_chg : 0.0;
        double upper_charge = cap_mass - cap;
        upper_charge = upper_charge > 0 ? upper_charge : 0.0;
        const double v_h_max = HP_E(v_h_max, p_v_h_max), cells = HP_E(cells, p_cells);
        double charge_temp = act_el * v_h_max * (15 * 60);
        charge_temp = charge_temp < upper_charge ? charge_temp : upper_charge;
        charge_temp = charge_temp > must_chg ? charge_temp : must_chg;
        double flow = DIV_K(charge_temp, 15 * 60);
        flow = flow < v_h_max ? flow : v_h_max;
        double ele_power = 0.0;
        if (cells != 0.0) {  // Electrolyser.get_power, HYD:38-48
            const double v_H_mass = div_c(flow, cells, HP_E(rc_cells, p_rc_cells));
            const double v_H_mol = DIV_K(v_H_mass, 2.02);
            const double v_H_L = v_H_mol * hp.v_M;
            const double v_H = v_H_L * 1000 * 60;
            const double temp = div_c(v_H * 2 * 96487, hp.v_M * 1000 * 60, hp.rc_vm60k);
            double power = temp * temp * 0.326 + temp * 1.476;
            ele_power = DIV_K(cells * power, 1000);
        }
        const double cpr_power = DIV_K(DIV_K(DIV_K(flow, 2.02) * hp.cpr_w12, 0.8), 1000);  // Compressor.generate_W, HYD:74-82
        // sty_step (HYD:104-126)
        cap += flow * 15 * 60;
        double lower_change = cap - 0.1 * cap_mass;
        lower_change = lower_change > 0 ? lower_change : 0.0;
        const double hy_use = total_mass_need < lower_change ? total_mass_need : lower_change;
        const double not_meet = total_mass_need - hy_use;
        cap -= hy_use;
        cap -= cap * HP_E(hydro_loss, p_hydro_loss);
        store_soc = div_c(cap, cap_mass, HP_E(rc_cap_mass, p_rc_cap_mass));
        const double all_power_second = ele_power + cpr_power;
        const bool gen_hy = flow > 0.5;  // MGR:161,173-179
        mid.at2();
        // ---- renewable netting (MGR:183-213)
        double hydrogen_power = all_power_second;
        double ev_power_sum = charging_power;
        double e0 = P0, e1 = P1;
        // fc_rate = charging_power / (0 + P0 + P1) (MGR:187-191) divides a positive finite number by itself: exactly 1
        double used_renew = 0.0;
        if (re_new_power >= hydrogen_power) {
            re_new_power -= hydrogen_power;
            used_renew += hydrogen_power;
            hydrogen_power = 0.0;
            const double tmp = ev_power_sum;
            ev_power_sum = ev_power_sum - re_new_power;
            ev_power_sum = ev_power_sum > 0 ? ev_power_sum : 0.0;
            used_renew += tmp - ev_power_sum;
            const double sl_ = 0.0 + e0 + e1;
            if (sl_ > 0) {
                const double rate = ev_power_sum / sl_;
                e0 = rate * e0;
                e1 = rate * e1;
            }
        } else {
            hydrogen_power -= re_new_power;
            used_renew = re_new_power;
        }
        CHUB_TEL(11, e0);  // self.re_ev_power_list is taken before the fuel-cell rescale (MGR:212)
        CHUB_TEL(12, e1);
        // ---- fuel cell (MGR:215-227, HFC.use_cell HYD:409-430)
        const double fc_max_power = HP_E(fc_max_power, p_fc_max_power);
        double fc_power = gen_hy ? 0.0 : fc_max_power * a_fc;
        if (fc_power > fc_max_power) fc_power = fc_max_power;
        else if (fc_power < 0) fc_power = 0.0;
        else if (fc_power > ev_power_sum) fc_power = ev_power_sum;
        double hy_to_use = DIV_K(fc_power * 1500, 119.6);
        hy_to_use = cap < hy_to_use ? cap : hy_to_use;
        fc_power = fc_power > 0 ? fc_power : 0.0;  // HYD:426 (not H2-limited)
        cap -= hy_to_use;                          // Store_SOC is not refreshed (HYD:428)
        ev_power_sum -= fc_power;
        {
            const double sl_ = 0.0 + e0 + e1;
            if (sl_ > 0) {
                const double rate_ = ev_power_sum / sl_;
                e0 = rate_ * e0;
                e1 = rate_ * e1;
            }
        }
        const double hy_loss = -6 / 1000.0 * hy_to_use;
        // ---- incomes and reward (MGR:233-269)
        const double real_price_dollar = in_price_next / 4;
        const double income_evs_fast = 0.42 / 4 * P0 - real_price_dollar * e0;
        const double income_evs_slow = 0.21 / 4 * P1 - real_price_dollar * e1;
        const double income_evs = income_evs_fast + income_evs_slow;
        const double income_evs_serve = 0.8 * (0.0 + F0 + F1);
        const double income_hys = 6 / 1000.0 * hy_use;
        const double not_meet_loss = -10 / 1000.0 * not_meet;
        const double hy_cost = -real_price_dollar * hydrogen_power;
        reward = DIV_K(income_hys + income_evs + income_evs_serve + hy_cost + 1 * hy_loss + not_meet_loss, 50);
        if (tel_on) {
            CHUB_TEL(0, act_el); CHUB_TEL(1, flow); CHUB_TEL(2, all_power_second); CHUB_TEL(4, cap);
            CHUB_TEL(5, total_mass_need); CHUB_TEL(6, hy_use); CHUB_TEL(7, not_meet); CHUB_TEL(8, fc_power);
            CHUB_TEL(9, hy_to_use); CHUB_TEL(10, used_renew); CHUB_TEL(13, hydrogen_power);
            CHUB_TEL(14, income_hys + income_evs + income_evs_serve + hy_cost); CHUB_TEL(15, reward);
            CHUB_TEL(19, (double) arrive); CHUB_TEL(20, (double) hv_line); CHUB_TEL(21, (double) q_len + (double) fold_n);
            // ev_power_list / ev_power_sum as the incomes and cumulated_draw_ele see them, after the fuel-cell rescale (MGR:219-224, 262)
            CHUB_TEL(24, e0); CHUB_TEL(25, e1); CHUB_TEL(26, ev_power_sum);
            CHUB_TEL(27, in_price_next);  // real_state[1] as this step found it: what real_price_dollar is a quarter of (MGR:234)
        }
        if (ep_on) {
            // the episode ledger: cumulated_income / cumulated_draw_ele (MGR:259-262), acumulate_reward (MGR:269), deviation (MGR:297) and what
            // the end-of-day block derives from it (MGR:275-290) "as if the episode ended now".  Plain divisions: the sums are held bit for bit
            // to the same additions made on the host.  Where `done` fires (the expression further down) the step's live columns are the record
            // of the finished episode.  An env stepped on past `done` keeps adding, as the reference object does.
            CHUB_G(double) lv = ctx->es.live;
            const size_t nn = n32, ee = e32;
            const double init_soc = EP ? ctx->ep.prm[PRM_INIT_SOC * n32 + e32] : hp.init_soc;
            double col[kEpCount];
            col[EPC_RETURN] = lv[EPC_RETURN * nn + ee] + reward;
            col[EPC_INCOME] = lv[EPC_INCOME * nn + ee] + (income_hys + income_evs + income_evs_serve + hy_cost);
            col[EPC_DRAW_ELE] = lv[EPC_DRAW_ELE * nn + ee] + ((e0 + e1) + hydrogen_power);
            col[EPC_LENGTH] = lv[EPC_LENGTH * nn + ee] + 1.0;
            col[EPC_DEVIATION] = fabs(store_soc - init_soc);
            col[EPC_TEST_PENALTY] = fabs(col[EPC_DEVIATION] * cap_mass / 1000 / 0.2);
            col[EPC_END_SOC] = store_soc;
#pragma unroll
            for (int c = 0; c < kEpCount; c++) lv[c * nn + ee] = col[c];
            if ((t_now + 1) >= 96) {
                CHUB_G(double) fin = ctx->es.fin;
#pragma unroll
                for (int c = 0; c < kEpCount; c++) fin[c * nn + ee] = col[c];
                ctx->es.episodes[ee] += 1u;
                ctx->es.pending[ee] = 1;
            }
        }
        }
    }

    ev.cap[e32] = cap;
    if (PAIR == 1) {  // the env's state behind this step, for the pair's second step in this lane
        nx->in.ou_pv = ou_pv;
        nx->in.ou_wd = ou_wd;
        nx->in.ou_price = ou_price;
        nx->in.cap = cap;
        nx->in.pv_day = pv_day;
        nx->in.wd_day = wd_day;
    }

    // state_norm (MGR:318-342) of what make_state (MGR:362-373) collects, written straight to the output row
    float *obs = s_out + (FUSED ? (int) (threadIdx.x & 63u) : (int) threadIdx.x) * row_w;
    double *o64 = tel_on ? (double *) ev.obs64 + (size_t) e32 * hp.obs_dim : nullptr;
    int n = 0;
#define CHUB_OBS(v)                    \
    do {                               \
        const double v_ = (v);         \
        obs[n] = (float) v_;           \
        if (o64) o64[n] = v_;          \
        n++;                           \
    } while (0)
    CHUB_OBS(sin_t);
    CHUB_OBS(div_c(price_next - hp.price_mean, hp.price_std, hp.rc_price_std));
    if (hp.S[0] > 0) {
        const double half_range = (double) hp.transformer_limit[0] / 2, rc_hr = hp.rc_half_range[0];
        CHUB_OBS(div_c((double) mn0 - half_range, half_range, rc_hr));
        CHUB_OBS(div_c((double) P0f - half_range, half_range, rc_hr));
        CHUB_OBS(div_c((double) mx0 - half_range, half_range, rc_hr));
        CHUB_OBS(DIV_K((double) ln0, 5));
    }
    if (hp.S[1] > 0) {
        const double half_range = (double) hp.transformer_limit[1] / 2, rc_hr = hp.rc_half_range[1];
        CHUB_OBS(div_c((double) mn1 - half_range, half_range, rc_hr));
        CHUB_OBS(div_c((double) P1f - half_range, half_range, rc_hr));
        CHUB_OBS(div_c((double) mx1 - half_range, half_range, rc_hr));
        CHUB_OBS(DIV_K((double) ln1, 5));
    }
    CHUB_OBS(store_soc);
    CHUB_OBS(DIV_K(re_pv, 42 * 5));
    CHUB_OBS(DIV_K(re_wd, 92 * 1));
#undef CHUB_OBS
    if (!RESET) {
        const bool dn = (t_now + 1) >= 96;  // MGR:271-273
        if (sa.done_f32) {  // packed row: reward and done ride in the same LDS row
            obs[n] = (float) reward;
            obs[n + 1] = dn ? 1.0f : 0.0f;
        } else {
            sa.reward[(size_t) e32 * sa.reward_stride] = (float) reward;
            if (sa.done) sa.done[e32] = (uint8_t) (dn ? 1 : 0);
            if (sa.done_f32) sa.done_f32[(size_t) e32 * sa.reward_stride] = dn ? 1.0f : 0.0f;
        }
    } else if (MULTI && sa.done_f32) {  // a masked reset into packed rows (auto-reset): the step's reward and done stay in the env's row
        obs[n] = sa.reward[(size_t) e32 * sa.reward_stride];
        obs[n + 1] = sa.done_f32[(size_t) e32 * sa.reward_stride];
    }
    if (tel_on) {
        ev.reward64[e32] = reward;
        CHUB_TEL(3, store_soc); CHUB_TEL(16, re_pv); CHUB_TEL(17, re_wd); CHUB_TEL(18, price_next);
        CHUB_TEL(22, (double) pv_day); CHUB_TEL(23, (double) wd_day);
        // the station scalars make_state puts into real_state (MGR:364-368) and the arrivals income_evs_serve counts (MGR:246)
        CHUB_TEL(28, (double) mn0); CHUB_TEL(29, (double) P0f); CHUB_TEL(30, (double) mx0); CHUB_TEL(31, (double) ln0); CHUB_TEL(32, (double) F0i);
        CHUB_TEL(33, (double) mn1); CHUB_TEL(34, (double) P1f); CHUB_TEL(35, (double) mx1); CHUB_TEL(36, (double) ln1); CHUB_TEL(37, (double) F1i);
    }
    } while (0);
    CHUB_STAMP(5);  // second half (clamp, hydrogen step, netting, fuel cell, money, observation) done
    mid.at3();
    if (MULTI) {  // device masks and auto-reset (every lane is here: the do / while above)
        if (RESET && sa.final_obs && live) {  // the row the reset is about to replace: the terminal observation
            const float *row = sa.obs + (size_t) e32 * (size_t) row_w;
            float *fin = sa.final_obs + (size_t) e32 * (size_t) hp.obs_dim;
            for (int j = 0; j < hp.obs_dim; j++) fin[j] = row[j];
        }
        if (sa.tick_note && live) sa.tick_note[e32] = CHUB_TICK(hp, sa.tick);
        if (!RESET && sa.done_mask) {
            const bool dn = live && (t_now + 1) >= 96;
            if (env < (int) N) sa.done_mask[e32] = (uint8_t) (dn ? 1 : 0);
            const unsigned long long fired = __ballot(dn);
            if ((threadIdx.x & 63u) == 0u && fired != 0ull) atomicAdd(sa.done_count, (uint32_t) __popcll(fired));
        }
    }
    flush_rows();
#if CHUB_TRACE
    CHUB_STAMP(6);  // rows flushed
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    CHUB_STAMP(7);  // stores drained
    CHUB_STAMP_REAL(9);
    if (!FUSED && sa.stamps_env && threadIdx.x == 0) for (int i = 0; i < 10; i++) sa.stamps_env[(size_t) env_block * 16 + i] = stamp_[i];
#endif
#undef TAB_PV
#undef TAB_WD
#undef TAB_PV_NOW
#undef TAB_WD_NOW
#undef TAB_HY
#undef TAB_HV
#undef HP_E
}

// Next step's state-independent draws, lane u: [0, 2N) the station-level variates of unit u, [2N, 3N) the per-env draws
template <bool RESET, bool MULTI, bool EP = false>
__device__ __forceinline__ void level_block(const DevCtx *__restrict__ ctx, const StepArgs &sa, const int64_t u, const int line_known = -1) {
    const HubParams &hp = ctx->hp;
    const int64_t N = hp.n_envs;
    if (u >= 3 * N) return;
    const int64_t env_ = u < N ? u : (u < 2 * N ? u - N : u - 2 * N);
    if (MULTI && !in_group(sa, env_)) return;
    // the slot of day the draws are for: the one after this launch's, on the env's own clock
    const int t_next = RESET ? 0 : ((MULTI ? clk_t(env_clk(sa, N, env_)) : sa.t) + 1) % 96;
    if (u < 2 * N) {
        const int kk = u >= N ? 1 : 0;
        // drawn AND decoded here, against the queue the slot kernel of this launch has just left in the unit's record
        const int line_now = line_known >= 0 ? line_known : pkd_line(ctx->st.rec[4u * (uint32_t) u + 3u]);
        ctx->st.pk[(sa.tick + 1u) & 1u][u] = draw_decoded_levels(hp, ctx->tb, CHUB_TICK(hp, sa.tick + 1u), t_next, kk, u - (int64_t) kk * N,
                                                                 line_now, hp.type[kk] == 0);
    } else {
        // the per-env draws (same Philox sites and counters the tail would use itself)
        const uint32_t e = (uint32_t) (u - 2 * N);
        const Tables &tb = ctx->tb;
        PhiloxCtx px{hp.key[0], hp.key[1], CHUB_TICK(hp, sa.tick + 1u), (uint32_t) (hp.env_id0 + e)};
        const U4 ow = px.block(SITE_OU, 0, 0);  // word 0 pv, 1 wind, 2 price
        const uint32_t hv_lev = px.block(SITE_HV, 0, 0).v[0] % 1000u;
        u32x4 d;
        d.x = __float_as_uint(normal_from_word(tb.normal_icdf, tb.normal_tail, ow.v[0]));
        d.y = __float_as_uint(normal_from_word(tb.normal_icdf, tb.normal_tail, ow.v[1]));
        d.z = __float_as_uint(normal_from_word(tb.normal_icdf, tb.normal_tail, ow.v[2]));
        const uint32_t cnt = EP ? hv_count_env(ctx->ep, e, t_next, hv_lev) : (uint32_t) tb.cnt_hv[(uint32_t) t_next * (uint32_t) kLevels + hv_lev];
        d.w = cnt != 0u ? __float_as_uint(soc_from_word(tb.soc_d_icdf, px.block(SITE_HVSOC, 0, 0).v[0])) : 0u;  // the first arrival's SoC
        ((CHUB_G(u32x4)) ctx->ev.drw[(sa.tick + 1u) & 1u])[e] = d;
        ctx->ev.drw_cnt[(sa.tick + 1u) & 1u][e] = (uint8_t) cnt;
    }
}

template <bool RESET, int MODE, bool MULTI, bool TAPE = false, bool EP = false>
__global__ __launch_bounds__(kEnvBlock) void k_env(const DevCtx *__restrict__ ctx, StepArgs sa, TailArgs ta, int nb_env) {
    __shared__ double s_pv[100], s_wd[150], s_pv_now[100], s_wd_now[150], s_hy[102];
    __shared__ __attribute__((aligned(16))) uint8_t s_hv[kLevels];
    __shared__ __attribute__((aligned(16))) float s_out[kEnvBlock * 16];  // output rows: obs_dim + 2 <= 15 floats
    // a masked reset whose mask was counted on the device (auto-reset: the envs the step in front found done) and names nobody: nothing to
    // do, tails and level workgroups alike -- one uniform load.  (Every env's clock has been carried to the other buffer by k_keep_clocks.)
    if (RESET && MULTI && mask_is_empty(sa)) return;
    if (MODE == MODE_PHILOX && (int) blockIdx.x >= nb_env) {
        // the last blocks of the grid: next step's station-level draws, one lane per (station, env).
        // They are pure VALU work and fill the issue slots the latency-bound tail waves leave empty.
        int seg = 0;
        int64_t env_ = 0;
#if CHUB_TRACE
        CHUB_STAMP_DECL(16);
        CHUB_STAMP_REAL(8);
#endif
        // XCD-aware order here too where the launch divides evenly (every XCD's eighth of the envs a whole number of workgroups, the tail
        // workgroups a multiple of 8): level workgroup j runs on XCD j % 8 and takes that XCD's envs -- station 0's units, station 1's,
        // then the env draws -- so that its CUs touch the same eighth of every array as the tail workgroups beside them
        const uint32_t jb = blockIdx.x - (uint32_t) nb_env, n32 = (uint32_t) ctx->hp.n_envs, per = n32 >> 3;  // envs per XCD
        bool have;
        if (!MULTI && ta.xcd && (n32 & 2047u) == 0u && ((uint32_t) nb_env & 7u) == 0u) {
            const uint32_t x = jb & 7u, i = jb >> 3, wpx = per / kEnvBlock;  // i-th of the 3 * wpx workgroups of XCD x
            seg = (int) (i / wpx);
            env_ = (int64_t) (x * per + (i - (uint32_t) seg * wpx) * kEnvBlock + threadIdx.x);
            have = seg < 3;
        } else {
            have = range_unit(sa, (int64_t) jb * kEnvBlock + threadIdx.x, 3, seg, env_);
        }
        if (have) level_block<RESET, MULTI, EP>(ctx, sa, (int64_t) seg * ctx->hp.n_envs + env_);
#if CHUB_TRACE
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        CHUB_STAMP_REAL(9);
        if (sa.stamps_env && threadIdx.x == 0) {  // (the level workgroups' rows follow the tail workgroups': entry and exit on the shared clock)
            sa.stamps_env[(size_t) blockIdx.x * 16 + 8] = stamp_[8];
            sa.stamps_env[(size_t) blockIdx.x * 16 + 9] = stamp_[9];
        }
#endif
        return;
    }
    const int blk = (int) xcd_order(blockIdx.x, (uint32_t) nb_env, MULTI ? 0u : ta.xcd) + (MULTI ? sa.env_lo / kEnvBlock : 0);  // a call on a subset: the blocks of its range of envs only
    const int env = blk * kEnvBlock + (int) threadIdx.x;
    TailIn none;  // (the stand-alone tail loads its inputs itself)
    NoMid nomid;
    env_tail<RESET, MODE, MULTI, false, NoMid, kEnvBlock, TAPE, EP>(ctx, sa, env, env < (int) ta.n_envs && (!MULTI || in_group(sa, env)), s_pv, s_wd, s_pv_now,
                                                                s_wd_now, s_hy, s_hv, s_out, blk, ta, nullptr, 0, 0, 0, none, false, nomid);
}

// ---------------------------------------------------------------------------------------- k_env_pair: the tails of TWO steps in one launch
// Large PHILOX batches inside chub_run_steps (the plan's pair rule, chub_plan.h): the launches of a pair of lock-step steps go slot(i), slot(i + 1),
// tails(i and i + 1) -- nothing in a step's slot phases reads what the previous step's tail writes -- so the tail launch's fixed costs (kernel
// boundary, the cold start of its load burst, the drain of its rows) are paid once per two steps.  What a pair keeps apart:
//   * records and tail actions: the pair's first slot launch writes PairArgs::rec_a / tail_act_a, its second the handle's own arrays
//     (StationArrays::rec / tail_act), so behind a pair the handle holds what a single step would have left;
//   * station draws: the first step's are decoded ahead as ever (StationArrays::pk, against the records of the step before the pair); the
//     second step's wait raw in PairArgs::pkraw and are decoded by its own slot launch (slot_body_packed<.., RAW>);
//   * env draws: a pair reads PairArgs::drw_in[0 / 1] and (MORE) writes the next pair's into drw_out[0 / 1], the other block of two.
// MORE: another pair follows at once (same day, same call).  Otherwise the launch leaves the handle where any other entry point can go on: the
// next step's draws where a single step's tail launch leaves them (level_block), and in the other parity what it would have found there.
struct PairArgs {
    CHUB_G(const uint32_t) rec_a;     // [2N][4] the records of the pair's first step
    CHUB_G(uint64_t) pkraw;           // [2N] raw station draws: in, the pair's second step's (not MORE: decoded into pk for whoever looks); out, the next pair's
    CHUB_G(const uint32_t) drw_in[2]; // [N][4] the env draws of the pair's two steps, and
    CHUB_G(const uint8_t) cnt_in[2];  // [N]   their FCEV arrival counts
    CHUB_G(uint32_t) drw_out[2];      // MORE: the next pair's
    CHUB_G(uint8_t) cnt_out[2];
};

// a step's state-independent env draws (level_block's, same Philox sites and counters): three OU normals and the first FCEV arrival, for slot t of the day
__device__ __forceinline__ void draw_env_pre(const DevCtx *__restrict__ ctx, const uint32_t tick, const int t, const uint32_t e, CHUB_G(uint32_t) drw,
                                             CHUB_G(uint8_t) cnt_out) {
    const HubParams &hp = ctx->hp;
    const Tables &tb = ctx->tb;
    PhiloxCtx px{hp.key[0], hp.key[1], tick, (uint32_t) (hp.env_id0 + e)};
    const U4 ow = px.block(SITE_OU, 0, 0);  // word 0 pv, 1 wind, 2 price
    const uint32_t hv_lev = px.block(SITE_HV, 0, 0).v[0] % 1000u;
    u32x4 d;
    d.x = __float_as_uint(normal_from_word(tb.normal_icdf, tb.normal_tail, ow.v[0]));
    d.y = __float_as_uint(normal_from_word(tb.normal_icdf, tb.normal_tail, ow.v[1]));
    d.z = __float_as_uint(normal_from_word(tb.normal_icdf, tb.normal_tail, ow.v[2]));
    const uint32_t cnt = (uint32_t) tb.cnt_hv[(uint32_t) t * (uint32_t) kLevels + hv_lev];
    d.w = cnt != 0u ? __float_as_uint(soc_from_word(tb.soc_d_icdf, px.block(SITE_HVSOC, 0, 0).v[0])) : 0u;  // the first arrival's SoC
    ((CHUB_G(u32x4)) drw)[e] = d;
    cnt_out[e] = (uint8_t) cnt;
}

// lane u of the level workgroups of a launch ([0, 2N) units, [2N, 3N) envs) -> its place, in XCD-aware order where the launch divides evenly (k_env)
__device__ __forceinline__ bool level_lane(const uint32_t jb, const uint32_t n32, const int nb_env, const uint32_t xcd, int64_t &u) {
    const uint32_t per = n32 >> 3;
    if (xcd && (n32 & 2047u) == 0u && ((uint32_t) nb_env & 7u) == 0u) {
        const uint32_t x = jb & 7u, i = jb >> 3, wpx = per / kEnvBlock;
        const uint32_t seg = i / wpx;
        u = (int64_t) seg * n32 + (int64_t) (x * per + (i - seg * wpx) * kEnvBlock + threadIdx.x);
        return seg < 3u;
    }
    u = (int64_t) jb * kEnvBlock + threadIdx.x;
    return u < 3 * (int64_t) n32;
}

// In front of a chain of pairs: what no earlier launch has left -- the raw station draws of the first pair's second step and the env draws of
// both its steps (sa: the pair's first step; its decoded station draws are in pk[tick & 1] already)
__global__ __launch_bounds__(kEnvBlock) void k_pair_draws(const DevCtx *__restrict__ ctx, StepArgs sa, PairArgs pr, uint32_t xcd) {
    const HubParams &hp = ctx->hp;
    const uint32_t n32 = (uint32_t) hp.n_envs;
    int64_t u;
    if (!level_lane(blockIdx.x, n32, 8, xcd, u)) return;
    const uint32_t tick1 = CHUB_TICK(hp, sa.tick + 1u);
    if (u < 2 * (int64_t) n32) {
        const int kk = u >= (int64_t) n32 ? 1 : 0;
        const int want = dk_want(ctx->st.pk[sa.tick & 1u][u]);
        pr.pkraw[u] = draw_raw_levels(hp, ctx->tb, tick1, sa.t + 1, kk, u - (int64_t) kk * n32, want, hp.type[kk] == 0);
    } else {
        const uint32_t e = (uint32_t) (u - 2 * (int64_t) n32);
        draw_env_pre(ctx, tick1 - 1u, sa.t, e, pr.drw_out[0], pr.cnt_out[0]);
        draw_env_pre(ctx, tick1, sa.t + 1, e, pr.drw_out[1], pr.cnt_out[1]);
    }
}

template <bool MORE>
__global__ __launch_bounds__(kEnvBlock) void k_env_pair(const DevCtx *__restrict__ ctx, StepArgs sa, StepArgs sb, TailArgs ta, TailArgs tb2, PairArgs pr,
                                                        int nb_env) {
    __shared__ double s_pv[100], s_wd[150], s_pv_now[100], s_wd_now[150], s_hy[102], s_pv2[100], s_wd2[150];
    __shared__ __attribute__((aligned(16))) float s_out[2][kEnvBlock * 16];  // each step's output rows
    if ((int) blockIdx.x >= nb_env) {
        const HubParams &hp = ctx->hp;
        const uint32_t n32 = (uint32_t) hp.n_envs;
        int64_t u;
        if (!level_lane(blockIdx.x - (uint32_t) nb_env, n32, nb_env, ta.xcd, u)) return;
        if (!MORE) {
            // what the tail launch of the pair's second step alone would leave for the step behind it ...
            level_block<false, false>(ctx, sb, u);
            // ... and what it would have found: that step's own draws, in the other parity
            if (u < 2 * (int64_t) n32) {
                const int kk = u >= (int64_t) n32 ? 1 : 0;
                ctx->st.pk[sb.tick & 1u][u] = dk_make(pr.pkraw[u], pkd_line(pr.rec_a[4u * (uint32_t) u + 3u]), hp.type[kk] == 0);
            } else {
                const uint32_t e = (uint32_t) (u - 2 * (int64_t) n32);
                ((CHUB_G(u32x4)) ctx->ev.drw[sb.tick & 1u])[e] = ((CHUB_G(const u32x4)) pr.drw_in[1])[e];
                ctx->ev.drw_cnt[sb.tick & 1u][e] = pr.cnt_in[1][e];
            }
            return;
        }
        const uint32_t tick2 = CHUB_TICK(hp, sb.tick + 1u);  // the next pair's first step
        if (u < 2 * (int64_t) n32) {
            const int kk = u >= (int64_t) n32 ? 1 : 0;
            const bool fast = hp.type[kk] == 0;
            const int64_t env_ = u - (int64_t) kk * n32;
            // its first step: drawn and decoded against the queue the pair's second slot launch has left, as ever
            const int line_now = pkd_line(ctx->st.rec[4u * (uint32_t) u + 3u]);
            const uint32_t dk = draw_decoded_levels(hp, ctx->tb, tick2, sb.t + 1, kk, env_, line_now, fast);
            ctx->st.pk[(sb.tick + 1u) & 1u][u] = dk;
            // its second step: raw, in the same lane -- the queue in front of it cannot exceed the first step's `want`
            pr.pkraw[u] = draw_raw_levels(hp, ctx->tb, tick2 + 1u, sb.t + 2, kk, env_, dk_want(dk), fast);
        } else {
            const uint32_t e = (uint32_t) (u - 2 * (int64_t) n32);
            draw_env_pre(ctx, tick2, sb.t + 1, e, pr.drw_out[0], pr.cnt_out[0]);
            draw_env_pre(ctx, tick2 + 1u, sb.t + 2, e, pr.drw_out[1], pr.cnt_out[1]);
        }
        return;
    }
    const int blk = (int) xcd_order(blockIdx.x, (uint32_t) nb_env, ta.xcd);
    const int env = blk * kEnvBlock + (int) threadIdx.x;
    const bool live = env < (int) ta.n_envs;
    TailIn none;
    TailNext nx;
    NoMid nomid;
    env_tail<false, MODE_PHILOX, false, false, NoMid, kEnvBlock, false, false, 1>(ctx, sa, env, live, s_pv, s_wd, s_pv_now, s_wd_now, s_hy, nullptr, s_out[0], blk, ta,
                                                                                  nullptr, 0, 0, 0, none, false, nomid, &nx, &tb2);
    // the second step, same lane: the env's state from registers, its other inputs as the first step's burst brought them; its rows of "now" are
    // the first step's rows of "next"
    env_tail<false, MODE_PHILOX, false, false, NoMid, kEnvBlock, false, false, 2>(ctx, sb, env, live, s_pv2, s_wd2, s_pv, s_wd, s_hy, nullptr, s_out[1], blk, tb2,
                                                                                  nullptr, 0, 0, 0, nx.in, true, nomid, &nx, nullptr);
}

// ---------------------------------------------------------------------------------------- k_env_walk: COMPAT, the split step's second launch
// The tails of step i and the stream walks of step i + 1 in ONE launch (lock-step steps of every env): both are one wave per SIMD --
// the tail a latency chain that waits two thirds of its time, the walk bound by instruction issue -- and they do not depend on each other:
// the walk needs the queue lengths and empty-slot counts the slot pass of step i has just left, and reads the streams as that slot pass
// committed them (the tail does not touch them: its forecourt draws were made by step i's walk); it writes the streams' state behind its
// draws to the shadow, so if a reset comes instead of step i + 1 nothing has happened.  Workgroups [0, nb_env): env_tail; the others: walks.
__global__ __launch_bounds__(256) void k_env_walk(const DevCtx *__restrict__ ctx, StepArgs sa, TailArgs ta, StepArgs sw, int nb_env) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[32 * 256 + 4 * kWalkStageWords];  // the walk's rings (32 KB) + its waves' staging areas / the tail's table rows and output rows (22 KB)
    if ((int) blockIdx.x >= nb_env) {
        __builtin_amdgcn_s_setprio(3);  // the walks are the launch's long pole: the tail wave on the same SIMD takes the issue slots they leave
        compat_walk_block<false>(ctx, sw, blockIdx.x - (uint32_t) nb_env, lds, lds + 32 * 256);
        return;
    }
    double *s_pv = (double *) lds, *s_wd = s_pv + 100, *s_pv_now = s_wd + 150, *s_wd_now = s_pv_now + 100, *s_hy = s_wd_now + 150;  // 602 doubles
    uint8_t *s_hv = (uint8_t *) (s_hy + 102 + 2);                                                                                   // kLevels bytes, 16-byte aligned
    float *s_out = (float *) (s_hv + 1008);                                                                                          // kEnvBlock * 16 floats
    static_assert((602 + 2) * 8 + 1008 + kEnvBlock * 16 * 4 <= 32 * 256 * 4 && kLevels <= 1008, "the tail's LDS inside the walk's");
    const int env = (int) blockIdx.x * kEnvBlock + (int) threadIdx.x;
    TailIn none;
    NoMid nomid;
    env_tail<false, MODE_COMPAT, false>(ctx, sa, env, env < (int) ta.n_envs, s_pv, s_wd, s_pv_now, s_wd_now, s_hy, s_hv, s_out, (int) blockIdx.x, ta, nullptr, 0, 0,
                                        0, none, false, nomid);
}

// ---------------------------------------------------------------------------------------- k_compat_small: COMPAT, a handful of envs, ONE launch
// The reference-exact mode is what the drop-in class runs, one env at a time (EvcsspManagerEnv_v6: test/env_test.py's loop), and there
// a step is nothing but launch latency and the serial walk of the env's two reference streams.  When every env of the handle fits ONE
// workgroup, the split step (k_compat_walk -> k_slot_split -> k_env) runs inside one launch of kCompatSmallBlock lanes, its parts as
// ROLES of the workgroup's waves:
//   wave 0             lane = env: the walk (compat_walk_env: station 0's draws, then station 1's), later the tail
//   waves 1 .. 3       station 0's units, waves 4 .. 7 station 1's (slot_body_compat<.., SPLIT>): loads, on / off, car_step along the
//                      curves and the departures run WHILE wave 0 walks; the bodies stop at the workgroup barrier in front of their
//                      first look at what the walk came to
// then the admissions, sums and records, another barrier, and env_tail (its forecourt draws continue the env's streams where the walk
// left them).  What crosses waves goes through memory as between the three launches (release / acquire at agent scope around the
// workgroup barriers).  Same functions, same order of draws: the results are those of the three launches.
static_assert(64 * (1 + kCompatSmallWaves0 + kCompatSmallWaves1) == kCompatSmallBlock, "wave roles of k_compat_small");
struct SmallMid {
    __device__ __forceinline__ void operator()() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
};
template <bool RESET>
__global__ __launch_bounds__(kCompatSmallBlock) void k_compat_small(const DevCtx *__restrict__ ctx, StepArgs sa, TailArgs ta) {
    constexpr int BLOCK = kCompatSmallBlock;
    __shared__ float lds_f[BLOCK];
    __shared__ uint32_t lds_u[2 * BLOCK];
    __shared__ double s_pv[100], s_wd[150], s_pv_now[100], s_wd_now[150], s_hy[102];
    __shared__ __attribute__((aligned(16))) uint8_t s_hv[kLevels];
    __shared__ __attribute__((aligned(16))) float s_out[kEnvBlock * 16];
    const HubParams &hp = ctx->hp;
    const int wave = (int) (threadIdx.x >> 6);
    const int k = wave <= kCompatSmallWaves0 ? 0 : 1, wave0 = k ? 1 + kCompatSmallWaves0 : 1;
    SmallMid mid;
    if (!RESET && sa.empt_fresh) {
        // the units' empty-slot counts are not the previous pass's (the first step after create / chub_set_state): counted here
        if (wave >= 1) {
            const int lane = (int) (threadIdx.x & 63u), U = hp.U[k], S = hp.S[k];
            const int upw = 64 / U, uiw = lane / U, slot = lane - uiw * U;
            const int env = (wave - wave0) * upw + uiw;
            const bool unit_ok = uiw < upw && env < (int) hp.n_envs;
            const bool valid = unit_ok && slot < S;
            const uint64_t unit_mask = (U == 64) ? ~0ull : (uiw < upw ? (((1ull << U) - 1ull) << (uiw * U)) : 0ull);
            uint32_t w = 0u;
            if (valid) w = ctx->sl.hot[4 * ((size_t) hp.base[k] + (size_t) env * (size_t) S + (size_t) slot) + 3];
            const uint64_t be = __ballot(valid && hot_tl(w) <= 1) & unit_mask;
            if (unit_ok && slot == 0) ctx->st.empt[(uint32_t) k * (uint32_t) hp.n_envs + (uint32_t) env] = (uint8_t) __popcll(be);
        }
        mid();
    }
    if (wave == 0) {
        const int env = (int) threadIdx.x;
        if (env < (int) hp.n_envs) {
            CompatStream rs;
            rs.load(ctx->cr, sa.rng_cur, env);
            compat_walk_env<RESET>(ctx, sa, env, rs);
            rs.store(ctx->cr, sa.rng_cur, env);
        }
        mid();  // (the barrier the slot waves reach inside their bodies)
    } else if (hp.type[k] == 0) {
        slot_body_compat<0, RESET, BLOCK, true, SmallMid>(hp, sa, ctx->sl, ctx->st, ctx->cr, ctx->tb, k, 0, lds_f, lds_u, wave0, mid);
    } else {
        slot_body_compat<1, RESET, BLOCK, true, SmallMid>(hp, sa, ctx->sl, ctx->st, ctx->cr, ctx->tb, k, 0, lds_f, lds_u, wave0, mid);
    }
    mid();  // the station records are in
    const int env = (int) threadIdx.x;
    TailIn none;
    NoMid nomid;
    env_tail<RESET, MODE_COMPAT, false, false, NoMid, BLOCK>(ctx, sa, env, env < (int) ta.n_envs, s_pv, s_wd, s_pv_now, s_wd_now, s_hy, s_hv, s_out, 0, ta,
                                                                    nullptr, 0, 0, 0, none, false, nomid);
}

// ---------------------------------------------------------------------------------------- k_step_fused: the whole step in ONE launch
// Small batches (C2: 4096 envs; every shard of an 8-GPU strong-scaling run): both step kernels are launch- and latency-bound
// there -- a handful of waves per CU, 4-5 us each of which 1.7 us is the kernel boundary -- and the chip has room for every
// workgroup at once, which is what made the fused form lose at 65 536 envs (lingering tail waves taking wave slots from the
// memory-bound slot work).  So: the packed slot body as it is, and behind the station records the workgroup goes on by itself --
//   last wave:  the per-env tails of the workgroup's envs (env_tail, records from LDS, table rows prefetched with the slot loads)
//   wave 0:     next step's station-level draws of the workgroup's units, decoded against the queue lengths just computed
//   wave 1:     next step's per-env draws
// Same functions, same Philox counters, same operations as k_slot_packed + k_env: bit-identical results
// (tests: chub_options.fused_step forced on / off).  PHILOX, lock-step, stations of up to 64 piles.
// The next step's draws of a one-launch workgroup (k_step_fused / k_step_tailwave / k_steps_fused / k_steps_piped): role 1 = the station-level draws of
// its units, decoded against the queue lengths the admission pass left in s_unit; role 2 = its envs' draws; any other role: nothing.
__device__ __forceinline__ void draw_next_step(const int role, const DevCtx *__restrict__ ctx, const StepArgs &sa, const PackedArgs &pa, const uint32_t *s_unit) {
    const int lane = threadIdx.x & 63;
    const int epb = (int) pa.epb, N = (int) pa.n_envs, env_first = (int) blockIdx.x * epb;
    if (role == 1) {
        for (int i = lane; i < 2 * epb; i += 64) {
            const int e = i >> 1, k = i & 1, env = env_first + e;
            if (env >= N) continue;
            int line;
            if ((k ? pa.S[1] : pa.S[0]) == 0u) {  // a station without piles: its queue moves on as in the body's record pass
                const int want = dk_want(pa.pk[(uint32_t) (k ? N : 0) + (uint32_t) env]);
                line = want < kMaxLine ? want : kMaxLine;
            } else {
                line = pkd_line(s_unit[i]);
            }
            level_block<false, false>(ctx, sa, (int64_t) k * N + env, line);
        }
    } else if (role == 2) {
        for (int i = lane; i < epb; i += 64)
            if (env_first + i < N) level_block<false, false>(ctx, sa, 2 * (int64_t) N + env_first + i);
    }
}
// The table rows a tail WAVE (k_step_tailwave, k_steps_piped) keeps in LDS for its envs: requested with the per-env state, parked behind the
// wave's first barrier (one wave: two or three elements per lane)
struct TailWaveRows {
    double r_pv[2], r_pvn[2], r_wd[3], r_wdn[3], r_hy[2];
    __device__ __forceinline__ void request(const TailArgs &ta, const bool with_hy) {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int i = lane + 64 * q;
            r_pv[q] = r_pvn[q] = r_hy[q] = 0.0;
            if (i < 100) {
                r_pv[q] = ta.pv_row[i];
                r_pvn[q] = ta.pv_row_now[i];
            }
            if (i < 102 && with_hy) r_hy[q] = ta.hy_table[i];
        }
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const int i = lane + 64 * q;
            r_wd[q] = r_wdn[q] = 0.0;
            if (i < 150) {
                r_wd[q] = ta.wd_row[i];
                r_wdn[q] = ta.wd_row_now[i];
            }
        }
    }
    __device__ __forceinline__ void park(double *s_pv, double *s_wd, double *s_pv_now, double *s_wd_now, double *s_hy, const bool with_hy) const {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int i = lane + 64 * q;
            if (i < 100) {
                s_pv[i] = r_pv[q];
                s_pv_now[i] = r_pvn[q];
            }
            if (i < 102 && with_hy) s_hy[i] = r_hy[q];
        }
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const int i = lane + 64 * q;
            if (i < 150) {
                s_wd[i] = r_wd[q];
                s_wd_now[i] = r_wdn[q];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the wave's own LDS rows, read back by other lanes of it)
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
};
struct TailPrefetch {
    const TailArgs &ta;
    double *s_pv, *s_wd, *s_pv_now, *s_wd_now, *s_hy;
    double r_pv, r_wd, r_pv_now, r_wd_now, r_hy;
    TailIn tin;          // the last wave: the state of its first 64 envs
    int tail_env;        // ... of this env (-1: none)
    bool predrawn;
    __device__ __forceinline__ void prefetch() {
        const int i = threadIdx.x;
        if (tail_env >= 0) tail_prefetch(tin, ta, (uint32_t) tail_env, predrawn);
        r_pv = r_wd = r_pv_now = r_wd_now = r_hy = 0.0;
        if (i < 100) {
            r_pv = ta.pv_row[i];
            r_pv_now = ta.pv_row_now[i];
        }
        if (i < 150) {
            r_wd = ta.wd_row[i];
            r_wd_now = ta.wd_row_now[i];
        }
        if (i < 102) r_hy = ta.hy_table[i];
    }
    __device__ __forceinline__ void park() {
        const int i = threadIdx.x;
        if (i < 100) {
            s_pv[i] = r_pv;
            s_pv_now[i] = r_pv_now;
        }
        if (i < 150) {
            s_wd[i] = r_wd;
            s_wd_now[i] = r_wd_now;
        }
        if (i < 102) s_hy[i] = r_hy;
    }
};

template <int BLOCK, int T, bool BITS, bool TAPE>
__device__ __forceinline__ void step_fused_body(const DevCtx *__restrict__ ctx, const StepArgs &sa, const PackedArgs &pa_in, const TailArgs &ta) {
    static_assert(BLOCK >= 150 && BLOCK / 64 >= 3, "one table element per lane; three waves with work of their own");
    __shared__ uint32_t q_new[BLOCK * T];
    __shared__ uint32_t q_cnt[2];
    __shared__ uint64_t s_ball[BLOCK * T / 64 + 2];
    __shared__ __attribute__((aligned(16))) int s_acc[2 * BLOCK * T * kAccCopies];
    __shared__ uint32_t s_unit[BLOCK * T / 2];
    __shared__ uint32_t s_uinfo[BLOCK * T / 2];
    __shared__ __attribute__((aligned(16))) u32x4 s_rec[BLOCK * T / 2];
    __shared__ double s_pv[100], s_wd[150], s_pv_now[100], s_wd_now[150], s_hy[102];
    __shared__ __attribute__((aligned(16))) float s_out[64 * 16];
    PackedArgs pa = pa_in;
    asm volatile("" : "+s"(pa.S[0]), "+s"(pa.S[1]), "+s"(pa.type[0]), "+s"(pa.type[1]), "+s"(pa.n_envs), "+s"(pa.epb), "+s"(pa.magic),
                      "+s"(pa.cls_delta), "+s"(pa.state), "+s"(pa.rec), "+s"(pa.pk), "+s"(pa.actions), "+s"(pa.cls0), "+s"(pa.ttab2));
    TailPrefetch hook{ta, s_pv, s_wd, s_pv_now, s_wd_now, s_hy, 0.0, 0.0, 0.0, 0.0, 0.0, TailIn(), -1, sa.fresh == 0 && !TAPE};
    {   // the lanes of the last wave that will run a tail: which env's state to request up front
        const int le = (int) (threadIdx.x & 63u), env = (int) blockIdx.x * (int) pa_in.epb + le;
        if ((int) (threadIdx.x >> 6) == BLOCK / 64 - 1 && le < (int) pa_in.epb && env < (int) pa_in.n_envs) hook.tail_env = env;
    }
    const int role = slot_body_packed<BLOCK, T, TAPE, false, false, false, true, TailPrefetch, BITS>(ctx->hp, sa, pa, ctx->tb, blockIdx.x, q_cnt, q_new,
                                                                                                      s_ball + 1, s_acc, s_unit, hook, s_rec, s_uinfo);
    constexpr int WAVES = BLOCK / 64;
    const int lane = threadIdx.x & 63;
    const int epb = (int) pa.epb, N = (int) pa.n_envs, env_first = (int) blockIdx.x * epb;
    // The body has returned in front of the workgroup's third barrier (behind it every new car is in its slot and in the LDS sums).
    // The last wave runs the first half of its first 64 envs' tails before it goes there -- the half that needs no station record --
    // while the first wave is still busy with the new cars' Philox blocks; then the barrier, the records (by the last wave), the
    // second half.  The other waves pass the barrier and go on to next step's draws.
    struct RecordsMid {
        const PackedArgs &pa;
        int *s_acc;
        const uint32_t *s_unit;
        u32x4 *s_rec;
        bool first;  // the first group of envs: the barrier and the records are still ahead
        __device__ __forceinline__ void at1() {}
        __device__ __forceinline__ void at2() {}
        __device__ __forceinline__ void at3() {}
        __device__ __forceinline__ void operator()() {
            if (!first) return;
            __syncthreads();
            packed_records<BLOCK, T, false, false, false, true, BITS>(pa, blockIdx.x, s_acc, s_unit, s_rec);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // s_rec was written by other lanes of this wave
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    };
    if (role != WAVES) __syncthreads();
    if (role == 1 || role == 2) {
        draw_next_step(role, ctx, sa, pa, s_unit);
    } else if (role == WAVES) {
        for (int c = 0; c < epb; c += 64) {  // the workgroup's envs, 64 at a time (the wave's own LDS traffic: wave-level synchronisation)
            const int le = c + lane, env = env_first + le;
            const bool live = le < epb && env < N;
            int rows = epb - c < 64 ? epb - c : 64;
            rows = N - (env_first + c) < rows ? N - (env_first + c) : rows;
            RecordsMid mid{pa, s_acc, s_unit, s_rec, c == 0};
            env_tail<false, MODE_PHILOX, false, true, RecordsMid, kEnvBlock, TAPE>(ctx, sa, env, live, s_pv, s_wd, s_pv_now, s_wd_now, s_hy, nullptr, s_out, 0, ta,
                                                                                   s_rec, live ? le : 0, env_first + c, rows > 0 ? rows : 0, hook.tin, c == 0, mid);
        }
    }
}

template <int BLOCK, int T, bool BITS = false, bool TAPE = false>
__global__ __launch_bounds__(BLOCK, 4) void k_step_fused(const DevCtx *__restrict__ ctx, StepArgs sa, PackedArgs pa_in, TailArgs ta) {
    step_fused_body<BLOCK, T, BITS, TAPE>(ctx, sa, pa_in, ta);
}

// ---- The one-launch step with the tails on a wave of their own (k_step_tailwave; hubs of 8 piles and more: at most 64 envs per workgroup).
// What k_steps_piped's stamps showed holds inside ONE step too: the tail's first half (the slot's exogenous values, the forecourt, the next
// slot's exogenous update: ~1 us) looks at nothing the slot phases produce, the next step's draws (~2 us of Philox blocks and dependent table
// reads on two waves) wait for the admission's queue lengths only, and only the second half of the tail needs the station records.  So a fifth
// wave starts the tails with the kernel, beside the slot phases; slot waves 0 / 1 pass the fourth barrier right behind the third and make
// the next step's draws beside everything that follows; slot waves 2 / 3 serve the new cars and end; the tail wave turns the LDS sums into the
// station records behind the fourth barrier and runs the second half.  Chain: slot phases + new cars + records + second half, instead of slot
// phases + new cars + draws | first half + records + second half.  Same functions, same Philox counters: bit-identical (tests: every test of
// the one-launch step runs through it; chub_options.fused_step forced on / off).
template <int BLOCK, int T, bool BITS>
struct TailWaveMid {
    const PackedArgs &pa;
    int *s_acc;
    const uint32_t *s_unit;
    u32x4 *s_rec;
    __device__ __forceinline__ void at1() { __syncthreads(); }  // #2
    __device__ __forceinline__ void at2() {}
    __device__ __forceinline__ void at3() {}
    __device__ __forceinline__ void operator()() {
        __syncthreads();  // #3
        __syncthreads();  // #4: every new car is in its slot and in the LDS sums
        packed_records<BLOCK, T, false, false, false, true, BITS>(pa, blockIdx.x, s_acc, s_unit, s_rec);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // s_rec was written by other lanes of this wave
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
};
template <int BLOCK, int T, bool BITS = false>
__global__ __launch_bounds__(BLOCK + 64, 2) void k_step_tailwave(const DevCtx *__restrict__ ctx, StepArgs sa, PackedArgs pa_in, TailArgs ta) {
    constexpr int WAVES = BLOCK / 64;
    static_assert(WAVES == 4, "two waves draw while two serve the new cars");
    __shared__ uint32_t q_new[BLOCK * T];
    __shared__ uint32_t q_cnt[2];
    __shared__ uint64_t s_ball[BLOCK * T / 64 + 2];
    __shared__ __attribute__((aligned(16))) int s_acc[2 * BLOCK * T * kAccCopies];
    __shared__ uint32_t s_unit[BLOCK * T / 2];
    __shared__ uint32_t s_uinfo[BLOCK * T / 2];
    __shared__ __attribute__((aligned(16))) u32x4 s_rec[BLOCK * T / 2];
    __shared__ double s_pv[100], s_wd[150], s_pv_now[100], s_wd_now[150], s_hy[102];
    __shared__ __attribute__((aligned(16))) float s_out[64 * 16];
    PackedArgs pa = pa_in;
    asm volatile("" : "+s"(pa.S[0]), "+s"(pa.S[1]), "+s"(pa.type[0]), "+s"(pa.type[1]), "+s"(pa.n_envs), "+s"(pa.epb), "+s"(pa.magic),
                      "+s"(pa.cls_delta), "+s"(pa.state), "+s"(pa.rec), "+s"(pa.pk), "+s"(pa.actions), "+s"(pa.cls0), "+s"(pa.ttab2));
    const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int epb = (int) pa.epb, N = (int) pa.n_envs, env_first = (int) blockIdx.x * epb;
    if (wave < WAVES) {
        NoHook hook;
        const int role = slot_body_packed<BLOCK, T, false, false, false, false, true, NoHook, BITS, true>(ctx->hp, sa, pa, ctx->tb, blockIdx.x, q_cnt, q_new,
                                                                                                            s_ball + 1, s_acc, s_unit, hook, nullptr, s_uinfo);
        __syncthreads();  // #4 (waves 0 / 1: right behind the third; waves 2 / 3: behind their new cars)
        draw_next_step(role, ctx, sa, pa, s_unit);
        return;
    }
    // ---- the tail wave
    const int env = env_first + lane;
    const bool live = lane < epb && env < N;
    TailIn tin = TailIn();
    if (live) tail_prefetch(tin, ta, (uint32_t) env, sa.fresh == 0);
    TailWaveRows tr;
    tr.request(ta, true);
    __syncthreads();  // #1
    tr.park(s_pv, s_wd, s_pv_now, s_wd_now, s_hy, true);
    int rows = epb < 64 ? epb : 64;
    rows = N - env_first < rows ? N - env_first : rows;
    TailWaveMid<BLOCK, T, BITS> mid{pa, s_acc, s_unit, s_rec};  // #2 (at1: behind the forecourt), #3 and #4 + the records (between the halves)
    env_tail<false, MODE_PHILOX, false, true, TailWaveMid<BLOCK, T, BITS>, kEnvBlock, false>(ctx, sa, env, live, s_pv, s_wd, s_pv_now, s_wd_now, s_hy, nullptr, s_out, 0, ta,
                                                                                       s_rec, live ? lane : 0, env_first, rows > 0 ? rows : 0, tin, true, mid);
}

// ---- A SPAN of lock-step steps in ONE launch ("multi-step persistent kernel for the random-policy bench").
// k_step_fused gives every workgroup whole envs -- their slots, their station records, their tails, the next step's draws -- and nothing
// crosses workgroups (MGR:136-302: the reference's envs are separate objects), so a workgroup can go from one step to the next BY ITSELF:
// no grid-wide synchronisation, one workgroup barrier between steps (every store of a step is then out and visible to the workgroup's own
// waves, which share the CU's vector cache).  What a step needs beyond the previous step's state arrives as today: the step's action rows
// (chub_run_steps's batches, step i reads batch i % n_batches) and its packed output block (step i writes block i & 1) -- so the policy is
// open loop over the span (the random-policy bench, replayed action tapes), and of the span's outputs the last two blocks remain.  Every
// per-step kernel argument is a function of the step number (clock, Philox tick, tariff, table rows, buffer parities): same functions,
// same Philox counters, bit-identical to the steps issued one by one.  What it saves is the kernel boundary between two steps of a
// launch-bound batch (the one-launch step is boundary + five dependent round trips + an f64 chain).
struct SpanArgs {
    int32_t n_steps, pc0;         // steps in the span (it ends at a day boundary at the latest); price_count before its first step (MGR:354)
    uint32_t first;               // index of its first step
    int32_t n_batches, D;
    const float *actions[8];      // chub_run_steps's action batches (n_batches <= 8)
    float *packed[2];             // ... and its two packed output blocks
    CHUB_G(const uint32_t) pk[2];     // StationArrays::pk, EnvArrays::drw / drw_cnt by tick parity
    CHUB_G(const uint32_t) drw[2];
    CHUB_G(const uint8_t) drw_cnt[2];
    CHUB_G(const double) price;   // Tables::price, pvT, wdT, sin96
    CHUB_G(const double) pvT;
    CHUB_G(const double) wdT;
    CHUB_G(const double) sin96;
};
template <int BLOCK, int T>
__global__ __launch_bounds__(BLOCK, 2) void k_steps_fused(const DevCtx *__restrict__ ctx, StepArgs sa0, PackedArgs pa0, TailArgs ta0, SpanArgs sp) {
    for (int s = 0; s < sp.n_steps; s++) {
        if (s) __syncthreads();
        StepArgs sa = sa0;
        PackedArgs pa = pa0;
        TailArgs ta = ta0;
        const uint32_t i = sp.first + (uint32_t) s;
        const int t = sa0.t + s, t_next = (t + 1) % 96;
        sa.t = t;
        sa.tick = sa0.tick + (uint32_t) s;
        sa.draw_price = ((sp.pc0 + s) % 4 == 0) ? 1 : 0;
        sa.price_last = sp.price[t];               // AGG:147
        sa.price_prev = sp.price[(t + 95) % 96];
        const uint32_t b = i % (uint32_t) sp.n_batches;
        const float *act = sp.actions[0];
#pragma unroll
        for (int j = 1; j < 8; j++) act = b == (uint32_t) j ? sp.actions[j] : act;
        float *out = (i & 1u) ? sp.packed[1] : sp.packed[0];
        sa.actions = act;
        sa.obs = out;
        sa.reward = out + sp.D;
        sa.done_f32 = out + sp.D + 1;
        if (s) sa.fresh = 0;  // (the previous step of this launch left this step's draws)
        const bool odd = (sa.tick & 1u) != 0u;
        pa.pk = odd ? sp.pk[1] : sp.pk[0];
        pa.actions = (CHUB_G(const float)) act;
        pa.tick = sa.tick;
        ta.drw = odd ? sp.drw[1] : sp.drw[0];
        ta.drw_cnt = odd ? sp.drw_cnt[1] : sp.drw_cnt[0];
        ta.actions = (CHUB_G(const float)) act;
        ta.pv_row = sp.pvT + t_next * 100;
        ta.wd_row = sp.wdT + t_next * 150;
        ta.pv_row_now = sp.pvT + t * 100;
        ta.wd_row_now = sp.wdT + t * 150;
        ta.sin_t = sp.sin96[t_next];
        step_fused_body<BLOCK, T, false, false>(ctx, sa, pa, ta);
    }
}

// ---- The same span with the TAILS A STEP BEHIND, on a wave of their own (k_steps_piped; hubs of 8 piles and more: at most 64 envs per
// workgroup).  In k_steps_fused a step is three chains end to end -- the slot phases up to the new cars (three dependent round trips, three
// barriers: ~2.4 us), the next step's draws (Philox blocks and dependent table reads on two waves: ~1.7 us) and, on the last wave alone, the
// station records and the tails (~600 dependent f64 operations, a wave64 f64 operation every 8 cycles: ~3.5 us) -- and none of them waits for
// the next one's RESULT: the slot phases of step s + 1 read slot words, decoded draws and action rows, none of which the tails of step s write
// (level_block takes the queue length from the admission pass, not from the tail), and the draws need the queue lengths the admission left,
// not the new cars.  So:
//   slot waves 0, 1:  behind the third barrier the next step's draws (units / envs) WHILE
//   slot waves 2, 3:  serve the new cars;  fourth barrier, next step
//   a fifth wave:     the station records and the tails of step s - 1 while the slot waves run step s: the LDS sums and queue words of a step
//                     live in two buffers by step parity, the table rows and output rows in areas nobody else touches; after the slot waves'
//                     last step it runs the last tails alone (a wave that has ended no longer counts at the barrier).
// gfx950 has ONE barrier per workgroup, so the tail wave takes part in the slot waves' four barriers per step: behind its load requests, behind
// the records, behind the forecourt (Mid::at1) and in front of its output flush (Mid::at3) -- four pieces of the tail against the four phases of
// the slot step, placed by the stamps of tools/experiments/piped_stamps.py so that neither side waits long for the other.
// Same functions, same Philox counters, same operations per env: bit-identical to steps issued one by one (tests).
#ifdef CHUB_PIPED_STAMPS  // (measurement build: when the tail wave of workgroup 0 reaches and leaves each of a step's four barriers)
__device__ unsigned long long g_piped_stamps[16];
#define PIPED_STAMP(k) do { if (stamp_on) g_piped_stamps[k] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define PIPED_STAMP(k) do { } while (0)
#endif
struct PipedMid {
    bool stamp_on;
    __device__ __forceinline__ void at1() { PIPED_STAMP(4); __syncthreads(); PIPED_STAMP(5); }
    __device__ __forceinline__ void at2() {}
    __device__ __forceinline__ void at3() { PIPED_STAMP(6); __syncthreads(); PIPED_STAMP(7); }
    __device__ __forceinline__ void operator()() {}
};
__device__ __forceinline__ void span_args(const StepArgs &sa0, const PackedArgs &pa0, const TailArgs &ta0, const SpanArgs &sp, const int s,
                                          StepArgs &sa, PackedArgs &pa, TailArgs &ta) {
    sa = sa0;
    pa = pa0;
    ta = ta0;
    const uint32_t i = sp.first + (uint32_t) s;
    const int t = sa0.t + s, t_next = (t + 1) % 96;
    sa.t = t;
    sa.tick = sa0.tick + (uint32_t) s;
    sa.draw_price = ((sp.pc0 + s) % 4 == 0) ? 1 : 0;
    sa.price_last = sp.price[t];               // AGG:147
    sa.price_prev = sp.price[(t + 95) % 96];
    const uint32_t b = i % (uint32_t) sp.n_batches;
    const float *act = sp.actions[0];
#pragma unroll
    for (int j = 1; j < 8; j++) act = b == (uint32_t) j ? sp.actions[j] : act;
    float *out = (i & 1u) ? sp.packed[1] : sp.packed[0];
    sa.actions = act;
    sa.obs = out;
    sa.reward = out + sp.D;
    sa.done_f32 = out + sp.D + 1;
    if (s) sa.fresh = 0;  // (the previous step of this launch left this step's draws)
    const bool odd = (sa.tick & 1u) != 0u;
    pa.pk = odd ? sp.pk[1] : sp.pk[0];
    pa.actions = (CHUB_G(const float)) act;
    pa.tick = sa.tick;
    ta.drw = odd ? sp.drw[1] : sp.drw[0];
    ta.drw_cnt = odd ? sp.drw_cnt[1] : sp.drw_cnt[0];
    ta.actions = (CHUB_G(const float)) act;
    ta.pv_row = sp.pvT + t_next * 100;
    ta.wd_row = sp.wdT + t_next * 150;
    ta.pv_row_now = sp.pvT + t * 100;
    ta.wd_row_now = sp.wdT + t * 150;
    ta.sin_t = sp.sin96[t_next];
}
template <int BLOCK, int T>
__global__ __launch_bounds__(BLOCK + 64, 2) void k_steps_piped(const DevCtx *__restrict__ ctx, StepArgs sa0, PackedArgs pa0, TailArgs ta0, SpanArgs sp) {
    constexpr int WAVES = BLOCK / 64;
    static_assert(WAVES == 4, "two waves draw while two serve the new cars");
    __shared__ uint32_t q_new[BLOCK * T];
    __shared__ uint32_t q_cnt[2];
    __shared__ uint64_t s_ball[BLOCK * T / 64 + 2];
    __shared__ __attribute__((aligned(16))) int s_acc2[2][2 * BLOCK * T * kAccCopies];  // a step's LDS sums and queue words, by step parity: the tail wave
    __shared__ uint32_t s_unit2[2][BLOCK * T / 2];                                      // turns them into station records while the next step is under way
    __shared__ uint32_t s_uinfo[BLOCK * T / 2];
    __shared__ __attribute__((aligned(16))) u32x4 s_rec[BLOCK * T / 2];                 // the tail wave's: the records ...
    __shared__ double s_pv[100], s_wd[150], s_pv_now[100], s_wd_now[150], s_hy[102];    // ... the table rows
    __shared__ __attribute__((aligned(16))) float s_out[64 * 16];                       // ... and its output rows
    const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int n = sp.n_steps;
    if (wave < WAVES) {
        // ---- the slot waves: step s = the packed slot body up to its third barrier (#1 #2 #3); then waves 0 / 1 the next step's draws, waves 2 / 3
        // the new cars; the fourth barrier (#4); the next step
        for (int s = 0; s < n; s++) {
            StepArgs sa;
            PackedArgs pa;
            TailArgs ta;
            span_args(sa0, pa0, ta0, sp, s, sa, pa, ta);
            asm volatile("" : "+s"(pa.S[0]), "+s"(pa.S[1]), "+s"(pa.type[0]), "+s"(pa.type[1]), "+s"(pa.n_envs), "+s"(pa.epb), "+s"(pa.magic),
                              "+s"(pa.cls_delta), "+s"(pa.state), "+s"(pa.rec), "+s"(pa.pk), "+s"(pa.actions), "+s"(pa.cls0), "+s"(pa.ttab2));
            NoHook hook;
            int *const s_acc = s_acc2[s & 1];
            uint32_t *const s_unit = s_unit2[s & 1];
            const int role = slot_body_packed<BLOCK, T, false, false, false, false, true, NoHook, false, true>(ctx->hp, sa, pa, ctx->tb, blockIdx.x, q_cnt, q_new,
                                                                                                                s_ball + 1, s_acc, s_unit, hook, nullptr, s_uinfo);
            draw_next_step(role, ctx, sa, pa, s_unit);  // (waves 0 / 1; the queue lengths are the admission's: in s_unit since the third barrier)
            __syncthreads();  // #4
        }
        return;  // (a wave that has ended no longer counts at the workgroup's barrier: the tail wave runs the last step's records and tails by itself)
    }
    // ---- the tail wave: during step s the station records and the tails of step s - 1
    for (int s = 0; s <= n; s++) {
        if (s == 0) {  // nothing to do during the first step: its four barriers
            __syncthreads();
            __syncthreads();
            __syncthreads();
            __syncthreads();
            continue;
        }
        StepArgs sa;
        PackedArgs pa;
        TailArgs ta;
        span_args(sa0, pa0, ta0, sp, s - 1, sa, pa, ta);
        const int lane = threadIdx.x & 63;
        const int epb = (int) pa.epb, N = (int) pa.n_envs, env_first = (int) blockIdx.x * epb;
        const int env = env_first + lane;
        const bool live = lane < epb && env < N;
        TailIn tin = TailIn();
        if (live) tail_prefetch(tin, ta, (uint32_t) env, sa.fresh == 0);
        TailWaveRows tr;
        tr.request(ta, s == 1);  // (the hydrogen table does not change: parked once)
        const bool stamp_on = blockIdx.x == 0 && (threadIdx.x & 63) == 0 && s == n - 2;
        (void) stamp_on;
        PIPED_STAMP(0);
        __syncthreads();  // #1
        PIPED_STAMP(1);
        // the station records of step s - 1 (every car's sums are in since that step's fourth barrier), into the record array and into s_rec
        packed_records<BLOCK, T, false, false, false, true, false>(pa, blockIdx.x, s_acc2[(s - 1) & 1], s_unit2[(s - 1) & 1], s_rec);
        PIPED_STAMP(2);
        __syncthreads();  // #2
        PIPED_STAMP(3);
        tr.park(s_pv, s_wd, s_pv_now, s_wd_now, s_hy, s == 1);  // (its wave-level fence also covers the records above: read back by other lanes of this wave)
        int rows = epb < 64 ? epb : 64;
        rows = N - env_first < rows ? N - env_first : rows;
        PipedMid mid{stamp_on};  // #3 (at1: behind the forecourt), #4 (at3: in front of the flush)
        env_tail<false, MODE_PHILOX, false, true, PipedMid, kEnvBlock, false>(ctx, sa, env, live, s_pv, s_wd, s_pv_now, s_wd_now, s_hy, nullptr, s_out, 0, ta,
                                                                              s_rec, live ? lane : 0, env_first, rows > 0 ? rows : 0, tin, true, mid);
        PIPED_STAMP(8);  // (flushed)
    }
}
#ifdef CHUB_PIPED_STAMPS
extern "C" int chub_debug_piped_stamps(unsigned long long *out) {
    return (int) hipMemcpyFromSymbol(out, HIP_SYMBOL(g_piped_stamps), sizeof(unsigned long long) * 16);
}
#endif

// COMPAT only: HySystem.__init__ (HYD:154-158) builds hy_power_speed_list with 101 REAL hy_step()s from the initial tank:
// each draws the FCEV arrival level and one mk_soc per arrival from the env's two streams (HYD:250-259), serves the
// 15-minute FIFO, clamps the production against the tank and moves the tank; entry i is the electrolyser + compressor
// power at request 0.01 * i.  Then hy_reset().  One lane per env replays exactly that: the streams advance by what the
// reference's constructor consumes and the table comes out as the reference's (it depends on the draws whenever a tank
// clamp binds).  Same operations as the step's tail (env_tail), plain f64 divisions.
// EP (handles with per-env hub parameters): the env's own constants and FCEV rate -- the reference's constructor with that env's kwargs.
template <bool EP>
__global__ void k_compat_ctor_sweep(const DevCtx *__restrict__ ctx, int rng_cur) {
    const HubParams &hp = ctx->hp;
    const EnvArrays &ev = ctx->ev;
    const Tables &tb = ctx->tb;
    const int64_t env = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= hp.n_envs) return;
    const uint32_t e32 = (uint32_t) env, n32 = (uint32_t) hp.n_envs;
    (void) e32;
    (void) n32;
#define HP_E(field, f) (EP ? ctx->ep.prm[(f) * n32 + e32] : hp.field)
    CompatStream rs;
    rs.load(ctx->cr, rng_cur, env);
    const int qcap = hp.qcap;
    double *qt = (double *) ev.q_time + (size_t) env * (size_t) qcap, *qm = (double *) ev.q_mass + (size_t) env * (size_t) qcap;
    double *table = (double *) ev.hy_env + (size_t) env * 102u;
    const double cap_mass = HP_E(cap_mass, PRM_CAP_MASS);
    double cap = HP_E(init_soc, PRM_INIT_SOC) * cap_mass;  // HyStore.__init__ (HYD:99-100)
    const double v_h_max = HP_E(v_h_max, PRM_V_H_MAX), cells = HP_E(cells, PRM_CELLS), hydro_loss = HP_E(hydro_loss, PRM_HYDRO_LOSS);
    int q_len = 0;
    bool stuck = false;
    double fold_t = 0.0, fold_m = 0.0;
    for (int i = 0; i < 101; i++) {
        const int t = i % 96;  // sys_time (HYD:192-193)
        // hvs_step (HYD:253-285)
        const int arrive = EP ? (int) hv_count_env(ctx->ep, e32, t, (uint32_t) rs.level()) : (int) tb.cnt_hv[t * kLevels + rs.level()];
        double total_time = stuck ? fold_t : 0.0, total_mass = stuck ? fold_m : 0.0;
        for (int q = 0; q < q_len; q++) {
            total_time += qt[q];
            total_mass += qm[q];
        }
        for (int j = 0; j < arrive; j++) {
            double tn, mn;
            fcev_time_mass(arrive_soc_from(rs.normal_d(7.0, 3.0)), tn, mn);
            if (!stuck && q_len < qcap) {
                qt[q_len] = tn;
                qm[q_len] = mn;
                q_len++;
            }
            total_time += tn;
            total_mass += mn;
        }
        if (total_time > 15.0) {
            int hv_num = 0;
            bool found = false;
            if (!stuck) {
                for (int a = 1; a <= arrive - 1 && !found; a++) {
                    int keep = q_len - a;
                    keep = keep < 0 ? 0 : keep;
                    double part = 0.0;
                    for (int j = 0; j < keep; j++) part += qt[j];
                    if (part <= 15.0) {
                        hv_num = keep;
                        found = true;
                    }
                }
            }
            if (found) {
                for (int j = hv_num; j < q_len; j++) {
                    qt[j - hv_num] = qt[j];
                    qm[j - hv_num] = qm[j];
                }
                q_len -= hv_num;
            } else {
                stuck = true;
                q_len = 0;
                fold_t = total_time;
                fold_m = total_mass;
            }
        } else {
            q_len = 0;
        }
        // hy_step (HYD:160-195) at gen_speed = 0.01 * i
        const double gen_speed = 0.01 * i;
        double must_chg = cap_mass * 0.1 - cap;
        must_chg = must_chg > 0 ? must_chg : 0.0;
        double upper_charge = cap_mass - cap;
        upper_charge = upper_charge > 0 ? upper_charge : 0.0;
        double charge_temp = gen_speed * v_h_max * (15 * 60);
        charge_temp = charge_temp < upper_charge ? charge_temp : upper_charge;
        charge_temp = charge_temp > must_chg ? charge_temp : must_chg;
        double flow = charge_temp / (15 * 60);
        flow = flow < v_h_max ? flow : v_h_max;
        double ele_power = 0.0;
        if (cells != 0.0) {  // Electrolyser.get_power, HYD:38-48
            const double v_H_mass = flow / cells;
            const double v_H_mol = v_H_mass / 2.02;
            const double v_H_L = v_H_mol * hp.v_M;
            const double v_H = v_H_L * 1000 * 60;
            const double temp = v_H * 2 * 96487 / (hp.v_M * 1000 * 60);
            const double power = temp * temp * 0.326 + temp * 1.476;
            ele_power = cells * power / 1000;
        }
        const double cpr_power = ((flow / 2.02) * hp.cpr_w12 / 0.8) / 1000;  // Compressor.generate_W, HYD:74-82
        // sty_step (HYD:104-126)
        cap += flow * 15 * 60;
        double lower_change = cap - 0.1 * cap_mass;
        lower_change = lower_change > 0 ? lower_change : 0.0;
        const double hy_use = total_mass < lower_change ? total_mass : lower_change;
        cap -= hy_use;
        cap -= cap * hydro_loss;
        table[i] = ele_power + cpr_power;
    }
    table[101] = table[100];
    rs.store(ctx->cr, rng_cur, env);
    // hy_reset (HYD:197-208): the step state is re-initialised by chub_reset; the FIFO arrays were scratch here
#undef HP_E
}

void launch_compat_ctor_sweep(const HubParams &hp, const DevCtx *ctx, int rng_cur, hipStream_t stream, bool env_params) {
    if (env_params) hipLaunchKernelGGL(k_compat_ctor_sweep<true>, dim3((unsigned) ((hp.n_envs + 63) / 64)), dim3(64), 0, stream, ctx, rng_cur);
    else hipLaunchKernelGGL(k_compat_ctor_sweep<false>, dim3((unsigned) ((hp.n_envs + 63) / 64)), dim3(64), 0, stream, ctx, rng_cur);
}

// -------------------------------------------------------------------- random policy (bench / tests)
__global__ void k_random_actions(int64_t n_envs, int64_t env_id0, int act_dim, uint32_t k0, uint32_t k1, uint32_t batch,
                                 float *actions) {
    const int64_t total = n_envs * (int64_t) ((act_dim + 3) / 4);
    const int per = (act_dim + 3) / 4;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t) gridDim.x * blockDim.x) {
        const int64_t env = i / per;
        const int j4 = (int) (i % per);
        U4 o = philox4x32_10((uint32_t) j4, 0u, batch, (uint32_t) (env_id0 + env), k0, k1);
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int j = j4 * 4 + c;
            if (j < act_dim) actions[env * act_dim + j] = (float) (o.v[c] >> 8) * (2.0f / 16777216.0f) - 1.0f;
        }
    }
}

// -------------------------------------------------------------------- introspection: current SoC on demand
// The step kernels keep, per occupied slot, the arrival SoC (COMPAT: the hot record's second word; PHILOX: the class) and the number of car_steps taken since
// (hot.w bits 25-31) instead of storing the SoC every step: the SoC after n steps is the same deterministic chain
// soc -> soc_to_time -> +1 slot -> time_to_soc the step evaluated (CHS.hpp:900-905 / 1065-1070), replayed here with the
// same device functions, so the value is bit for bit the one the step produced.
__device__ __forceinline__ float replay_soc_steps(const HubParams &hp, int k, float soc, int n) {
    const bool cp = hp.constant_charging != 0;
    for (int i = 0; i < n; i++) {
        float pw;
        if (hp.type[k] == 0) car_step_curves<0>(__fadd_rn(soc_to_time<0>(soc, cp), 1.0f), cp, hp.cc, soc, pw);
        else car_step_curves<1>(__fadd_rn(soc_to_time<1>(soc, cp), 1.0f), cp, hp.cc, soc, pw);
    }
    return soc;
}

// -------------------------------------------------------------------- per-pile observations (chub_pile_obs_device)
// Tables of the PHILOX SoC column, [2][kSocLevels][kClsRow] f32: the class's arrival SoC after n = 0 .. kClsRow-1 car_steps, i.e. what
// replay_soc_steps gives a slot of that class and count, written BY THE SAME CHAIN ON THE DEVICE (entry n is the chain's value after n
// steps, so every prefix is the replay's own result) when the handle is created and whenever a tape rewrites class rows.  One lane per
// (station, class).
__global__ void k_build_cls_soc(const DevCtx *__restrict__ ctx, float *out) {
    const HubParams &hp = ctx->hp;
    const int i = (int) (blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= 2 * kSocLevels) return;
    const int k = i / kSocLevels, c = i - k * kSocLevels;
    float soc = ctx->tb.cls_soc0[k][c];
    float *row = out + (size_t) i * kClsRow;
    row[0] = soc;
    for (int n = 1; n < kClsRow; n++) {
        soc = replay_soc_steps(hp, k, soc, 1);
        row[n] = soc;
    }
}
void launch_build_cls_soc(const DevCtx *ctx, float *d_out, hipStream_t stream) {
    hipLaunchKernelGGL(k_build_cls_soc, dim3((2 * kSocLevels + 255) / 256), dim3(256), 0, stream, ctx, d_out);
}

// Station::situation (CHS.hpp:204-231) and the two stay counters (CHS.hpp:245-246) of every pile as columns: out[env][column][hub slot],
// the columns of the field mask in ascending order, every value the f32 Station::situation holds for that pile.  Lane = (env, hub
// slot) of a flat range, so a wave's stores of one column are runs of consecutive floats; no lane talks to another (a unit is not a wave
// here), so stations of any size take the same path.  LAYOUT: the handle's slot arrays (SlotArrays) -- the output is the same for all three.
// What a field set does not ask for is not loaded: the state word alone gives car, charge and already_stay_time's `left`; the class row /
// hot record only power, emergency (with Tables::ttab) and init_soc; stay8 only the two counters; the SoC only the SoC column -- PHILOX reads
// it from k_build_cls_soc's table, the other two replay the car's steps (replay_soc_steps).
struct PileObsArgs {
    const DevCtx *ctx;
    const uint8_t *mask;   // [N] or null: rows of envs whose byte is 0 are not written
    const float *cls_soc;  // PHILOX: k_build_cls_soc's tables
    float *out;            // [N][columns][S0 + S1]
    uint32_t fields;       // bits of the CHUB_PILE_* enum
};
enum PileField : uint32_t { PF_CAR = 1u, PF_CHARGE = 2u, PF_EMERGENCY = 4u, PF_POWER = 8u, PF_SOC = 16u, PF_INIT_SOC = 32u, PF_TARGET_SOC = 64u,
                            PF_STAY_TIME = 128u, PF_ALREADY_STAY = 256u };
// One pile's decode, THE reader of all three slot layouts: k_pile_obs (and through it chub_get_slots) and k_station_profile (whose bins are
// sums over exactly these values).  What `fields` (PF_* bits) does not ask for is not loaded and stays 0.  i = env * S + slot, the pile's
// index in the slot-major PHILOX arrays.  cls_soc (PHILOX): k_build_cls_soc's tables, rebuilt whenever the class rows change.
struct PileVals {
    int left, stay, lev;
    bool chg;
    float power, t_soc, arrive, soc;
};
template <int LAYOUT>
__device__ __forceinline__ PileVals pile_decode(const DevCtx *__restrict__ ctx, const float *cls_soc, uint32_t fields, int64_t env, int slot,
                                                int64_t i) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const HubParams &hp = ctx->hp;
    const Tables &tb = ctx->tb;
    const int S0 = hp.S[0];
    const bool want_row = (fields & (PF_EMERGENCY | PF_POWER)) != 0u;  // (power, t_soc) of the car's point on its curve
    const int k = slot >= S0 ? 1 : 0;
    int left, stay = 0, lev, n;
    bool chg;
    float power = 0.0f, t_soc = 0.0f, arrive = 0.0f, soc = 0.0f;
    if (LAYOUT == LAYOUT_COMPAT) {  // station-major 16-byte records; the fourth word alone when nothing else is asked for
        const int64_t idx = hp.base[k] + env * hp.S[k] + (slot - (k ? S0 : 0));
        u32x4 h = {0u, 0u, 0u, 0u};
        if (want_row || (fields & (PF_SOC | PF_INIT_SOC))) h = *(CHUB_G(const u32x4)) (ctx->sl.hot + 4 * idx);
        else h.w = ctx->sl.hot[4 * idx + 3];
        const CompatSlot s = CompatSlot::unpack(h);
        left = s.tl; chg = s.charge; stay = s.meta & 127; lev = hot_level(h.w); n = (int) (h.w >> 25);
        power = s.power; t_soc = s.t_soc; arrive = s.arr_soc;
        if (left > 0 && (fields & PF_SOC)) soc = replay_soc_steps(hp, k, arrive, n);
    } else {
        const uint32_t w0 = LAYOUT == LAYOUT_CURVES ? ctx->sl.wrd[i] : ctx->sl.hot[i];
        left = ps_tl(w0); chg = (w0 & kPsChg) != 0u; lev = (int) ps_lev(w0); n = (int) ps_n(w0);
        if (left > 0) {
            if (LAYOUT == LAYOUT_CURVES) {
                if (want_row) {
                    const f32x2 hv = *(CHUB_G(const f32x2)) ((CHUB_G(const float)) ctx->sl.hot + 2 * i);
                    power = hv.x; t_soc = hv.y;
                }
                if (fields & (PF_SOC | PF_INIT_SOC)) arrive = ctx->sl.soc0[i];
                if (fields & PF_SOC) soc = replay_soc_steps(hp, k, arrive, n);
            } else {
                const uint32_t c = ps_cls(w0);
                if (want_row) {
                    const f32x2 row = *(CHUB_G(const f32x2)) ((CHUB_G(const char)) tb.cls[k] + ((size_t) c * (kClsRow * 8u) + (uint32_t) n * 8u));
                    power = row.x; t_soc = row.y;
                }
                if (fields & PF_INIT_SOC) arrive = tb.cls_soc0[k][c];
                if (fields & PF_SOC) soc = cls_soc[((size_t) k * kSocLevels + c) * kClsRow + (uint32_t) n];
            }
        }
        if (fields & (PF_STAY_TIME | PF_ALREADY_STAY)) stay = (int) ctx->sl.stay8[i];
    }
    return {left, stay, lev, chg, power, t_soc, arrive, soc};
}
template <int LAYOUT>
__global__ __launch_bounds__(256) void k_pile_obs(const PileObsArgs a) {
    const DevCtx *__restrict__ ctx = a.ctx;
    const HubParams &hp = ctx->hp;
    const Tables &tb = ctx->tb;
    const uint32_t fields = a.fields;
    const int S0 = hp.S[0], S = S0 + hp.S[1], C = __popc(fields);
    const int64_t NS = hp.n_envs * (int64_t) S;
    const bool small = NS <= 0xFFFFFFFFll;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < NS; i += (int64_t) gridDim.x * blockDim.x) {
        const int64_t env = small ? (int64_t) ((uint32_t) i / (uint32_t) S) : i / S;  // (a 64-bit division costs more than the rest of a lane's work)
        if (a.mask && !a.mask[env]) continue;
        const int slot = (int) (i - env * S);
        const int k = slot >= S0 ? 1 : 0;
        const PileVals p = pile_decode<LAYOUT>(ctx, a.cls_soc, fields, env, slot, i);
        const bool car = p.left > 0;
        float *o = a.out + ((int64_t) env * C * S + slot);  // column c of this pile: o[c * S]
        if (fields & PF_CAR) { *o = car ? 1.0f : 0.0f; o += S; }
        if (fields & PF_CHARGE) { *o = p.chg ? 1.0f : 0.0f; o += S; }
        if (fields & PF_EMERGENCY) { *o = car ? emergency_of(tb.ttab[k][p.lev], p.t_soc, p.left) : 0.0f; o += S; }
        if (fields & PF_POWER) { *o = car ? p.power : 0.0f; o += S; }
        if (fields & PF_SOC) { *o = car ? p.soc : 0.0f; o += S; }
        if (fields & PF_INIT_SOC) { *o = car ? p.arrive : 0.0f; o += S; }
        if (fields & PF_TARGET_SOC) { *o = car ? uniform_level(p.lev, 80.0f, 100.0f) : 0.0f; o += S; }
        if (fields & PF_STAY_TIME) { *o = car ? (float) p.stay : -1.0f; o += S; }
        if (fields & PF_ALREADY_STAY) { *o = car ? (float) (p.stay - p.left) : -1.0f; }
    }
}
void launch_pile_obs(const HubParams &hp, const DevCtx *ctx, uint32_t fields, const uint8_t *d_mask, const float *d_cls_soc, float *d_out,
                     hipStream_t stream) {
    const int64_t NS = hp.n_envs * (int64_t) (hp.S[0] + hp.S[1]);
    if (NS <= 0) return;
    int64_t nb = (NS + 255) / 256;
    if (nb > (1 << 20)) nb = 1 << 20;  // (beyond 2^28 piles the lanes stride)
    const PileObsArgs a = {ctx, d_mask, d_cls_soc, d_out, fields};
    switch (slot_layout(hp)) {
    case LAYOUT_COMPAT: hipLaunchKernelGGL(k_pile_obs<LAYOUT_COMPAT>, dim3((unsigned) nb), dim3(256), 0, stream, a); break;
    case LAYOUT_CURVES: hipLaunchKernelGGL(k_pile_obs<LAYOUT_CURVES>, dim3((unsigned) nb), dim3(256), 0, stream, a); break;
    default: hipLaunchKernelGGL(k_pile_obs<LAYOUT_PHILOX>, dim3((unsigned) nb), dim3(256), 0, stream, a); break;
    }
}

// -------------------------------------------------------------------- pile sets (chub_pile_set_device)
// Which piles' action bits can matter to the next step, as chub_step_bits' words: out[env][W] u64, bit b = hub slot b, bits from S up zero.
// The values are pile_decode's, i.e. k_pile_obs' car and emergency columns: PSET_OCCUPIED asks it for the car alone (the state word),
// PSET_DECIDABLE for the emergency too (judge_feasibility's own predicate, CHS:1404-1413: no car -> forced off, emergency >= 1.01 -> forced
// on), PSET_ALL loads nothing.  A workgroup takes E = max(1, 256 / S) whole envs, one lane per pile (a station of more than 256 piles: the
// lanes stride); the envs' words are assembled in LDS by atomicOr and stored whole, consecutive lanes on consecutive words: no global atomics.
enum PileSet : int { PSET_ALL = 0, PSET_OCCUPIED, PSET_DECIDABLE, PSET_COUNT };
constexpr int kPileSetLanes = 256;
constexpr int kPileSetLdsWords = 2 * (kPileSetLanes + 4);  // u32 words of E envs: E * 2 W <= 2 (256 / S) (S / 64 + 1) <= 8 + 512 / S for S <= 256, 2 W <= 256 beyond
struct PileSetArgs {
    const DevCtx *ctx;
    const uint8_t *mask;   // [N] or null: rows of envs whose byte is 0 are not written
    uint32_t *out;         // [N][2 W] u32 = [N][W] u64, little-endian halves
    int which;             // PileSet
    int envs;              // E: envs per workgroup
};
template <int LAYOUT>
__global__ __launch_bounds__(kPileSetLanes) void k_pile_set(const PileSetArgs a) {
    __shared__ uint32_t words[kPileSetLdsWords];
    const DevCtx *__restrict__ ctx = a.ctx;
    const HubParams &hp = ctx->hp;
    const Tables &tb = ctx->tb;
    const int S0 = hp.S[0], S = S0 + hp.S[1], W2 = 2 * ((S + 63) >> 6), E = a.envs;
    const int tid = (int) threadIdx.x;
    const int64_t env0 = (int64_t) blockIdx.x * E;
    const uint32_t fields = a.which == PSET_DECIDABLE ? (PF_CAR | PF_EMERGENCY) : PF_CAR;
    for (int w = tid; w < E * W2; w += kPileSetLanes) words[w] = 0u;
    __syncthreads();
    for (int idx = tid; idx < E * S; idx += kPileSetLanes) {
        const int j = idx / S, slot = idx - j * S;
        const int64_t env = env0 + j;
        if (env >= hp.n_envs || (a.mask && !a.mask[env])) continue;
        bool in = true;
        if (a.which != PSET_ALL) {
            const PileVals p = pile_decode<LAYOUT>(ctx, nullptr, fields, env, slot, env * S + slot);
            in = p.left > 0;
            if (in && a.which == PSET_DECIDABLE) in = emergency_of(tb.ttab[slot >= S0 ? 1 : 0][p.lev], p.t_soc, p.left) < 1.01f;
        }
        if (in) atomicOr(&words[j * W2 + (slot >> 5)], 1u << (slot & 31));
    }
    __syncthreads();
    for (int w = tid; w < E * W2; w += kPileSetLanes) {
        const int64_t env = env0 + w / W2;
        if (env < hp.n_envs && (!a.mask || a.mask[env])) a.out[env0 * W2 + w] = words[w];
    }
}
void launch_pile_set(const HubParams &hp, const DevCtx *ctx, int which, const uint8_t *d_mask, uint64_t *d_bits, hipStream_t stream) {
    const int S = hp.S[0] + hp.S[1];
    if (hp.n_envs <= 0 || S <= 0) return;
    const int E = S >= kPileSetLanes ? 1 : kPileSetLanes / S;
    const int64_t nb = (hp.n_envs + E - 1) / E;
    const PileSetArgs a = {ctx, d_mask, (uint32_t *) d_bits, which, E};
    switch (slot_layout(hp)) {
    case LAYOUT_COMPAT: hipLaunchKernelGGL(k_pile_set<LAYOUT_COMPAT>, dim3((unsigned) nb), dim3(kPileSetLanes), 0, stream, a); break;
    case LAYOUT_CURVES: hipLaunchKernelGGL(k_pile_set<LAYOUT_CURVES>, dim3((unsigned) nb), dim3(kPileSetLanes), 0, stream, a); break;
    default: hipLaunchKernelGGL(k_pile_set<LAYOUT_PHILOX>, dim3((unsigned) nb), dim3(kPileSetLanes), 0, stream, a); break;
    }
}

// -------------------------------------------------------------------- exogenous look-ahead (chub_forecast_device)
// What is deterministic about the next H slots of an env's day, as columns: out[env][column][h], the columns of the field mask in ascending
// order (FcField), h = 0 the slot the env's next step simulates.  Lane = one float of the flat [N][C][H] range, so a wave stores runs of
// consecutive floats (k_pile_obs' pattern); no lane talks to another, no LDS.  The env's clock and days are the same address for every lane
// of its block.  MULTI: the clock is the env's own (the buffer the handle's next launch reads); otherwise it is an argument and the slot,
// time, tariff and arrival columns are wave-uniform.  EP (per-env rows): the FCEV mean is the sum over the arrival indices v of
// hist[s][v] * hv_count_rate(rate of the env, v) over the slot's non-empty bins -- at most kFcHist terms (about 60 with the packaged
// arrival table) instead of 1000 levels, with the tail's own rounding and clamp;
// the homogeneous means are the host's (chub_create, beside cnt / cnt_hv).  The OU noise is not forecast: see include/chub.h.
struct ForecastArgs {
    const DevCtx *ctx;
    const uint8_t *mask;   // [N] or null: blocks of envs whose byte is 0 are not written
    const uint16_t *clk;   // MULTI: [N] the envs' clocks (StepArgs::env_clk's layout)
    ForecastTabs ft;
    float *out;            // [N][columns][horizon]
    uint64_t colmap;       // 4 bits per column: its field
    int32_t columns, horizon;
    int32_t t;             // lock-step: the handle's clock
};
template <bool EP, bool MULTI>
__global__ __launch_bounds__(256) void k_forecast(const ForecastArgs a) {
    const DevCtx *__restrict__ ctx = a.ctx;
    const Tables &tb = ctx->tb;
    const uint32_t H = (uint32_t) a.horizon, CH = (uint32_t) a.columns * H;
    const int64_t total = ctx->hp.n_envs * (int64_t) CH;
    const bool small = total <= 0xFFFFFFFFll;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t) gridDim.x * blockDim.x) {
        const int64_t env = small ? (int64_t) ((uint32_t) i / CH) : i / CH;
        if (a.mask && !a.mask[env]) continue;
        const uint32_t r = (uint32_t) (i - env * CH), c = r / H, h = r - c * H;
        const uint32_t f = (uint32_t) (a.colmap >> (4u * c)) & 15u;
        uint32_t t = MULTI ? (uint32_t) clk_t(a.clk[env]) : (uint32_t) a.t;
        t = t > 95u ? 95u : t;  // (a clock is 0 .. 95; no table index below depends on that being so)
        const uint32_t th = t + h, s = th >= 96u ? th - 96u : th;
        float v;
        switch (f) {
        case FC_SLOT: v = (float) s; break;
        case FC_VALID: v = th <= 95u ? 1.0f : 0.0f; break;
        case FC_SIN: v = (float) tb.sin96[s]; break;
        case FC_COS: v = (float) tb.sin96[s >= 72u ? s - 72u : s + 24u]; break;
        case FC_PRICE: v = (float) tb.price[s == 0u ? 95u : s - 1u]; break;  // the tariff of the slot before: what the step of slot s finds in price[-1]
        case FC_PV: {
            const uint32_t d = (uint32_t) ctx->ev.pv_day[env];
            const double x = tb.pvT[s * 100u + (d < 100u ? d : 99u)];
            v = (float) ((x > 0 ? x : 0.0) * 5);  // REN:38-43, MGR:349 without the noise factor
            break;
        }
        case FC_WIND: {
            const uint32_t d = (uint32_t) ctx->ev.wd_day[env];
            const double x = tb.wdT[s * 150u + (d < 150u ? d : 149u)];
            v = (float) ((x > 0 ? x : 0.0) * 1);
            break;
        }
        case FC_ARRIVALS0: v = a.ft.mean[s]; break;
        case FC_ARRIVALS1: v = a.ft.mean[96u + s]; break;
        default:  // FC_FCEV
            if (EP) {
                const float rate = ctx->ep.hv_rate[env];
                const uint32_t *hist = a.ft.hist + s * (uint32_t) kFcHist;
                const uint32_t bins = min((uint32_t) a.ft.hist_len[s], (uint32_t) kFcHist);
                uint32_t sum = 0u;
                for (uint32_t j = 0u; j < bins; j++) {
                    const uint32_t b = hist[j];
                    sum += (b >> 16) * hv_count_rate(rate, b & 0xFFFFu);
                }
                v = (float) sum / 1000.0f;
            } else {
                v = a.ft.mean[192u + s];
            }
            break;
        }
        a.out[i] = v;
    }
}
void launch_forecast(const HubParams &hp, const DevCtx *ctx, const ForecastTabs &ft, uint32_t fields, int horizon, int t, const uint16_t *d_clk,
                     const uint8_t *d_mask, float *d_out, hipStream_t stream) {
    ForecastArgs a = {ctx, d_mask, d_clk, ft, d_out, 0ull, 0, horizon, t};
    for (uint32_t f = 0; f < (uint32_t) kFcCount; f++)
        if (fields >> f & 1u) a.colmap |= (uint64_t) f << (4 * a.columns++);
    const int64_t total = hp.n_envs * (int64_t) a.columns * horizon;
    if (total <= 0) return;
    int64_t nb = (total + 255) / 256;
    if (nb > (1 << 20)) nb = 1 << 20;  // (beyond 2^28 floats the lanes stride)
    const bool ep = ft.hist != nullptr, multi = d_clk != nullptr;
    if (ep && multi) hipLaunchKernelGGL((k_forecast<true, true>), dim3((unsigned) nb), dim3(256), 0, stream, a);
    else if (ep) hipLaunchKernelGGL((k_forecast<true, false>), dim3((unsigned) nb), dim3(256), 0, stream, a);
    else if (multi) hipLaunchKernelGGL((k_forecast<false, true>), dim3((unsigned) nb), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((k_forecast<false, false>), dim3((unsigned) nb), dim3(256), 0, stream, a);
}

// -------------------------------------------------------------------- step terms (chub_get_step_terms_device)
// What the reward of an env's last step is made of and what a constrained learner penalises, as columns: out[env][column], the columns of the
// field mask in ascending order of the CHUB_ST_* enum.  A pure function of the telemetry block [kTelemCount][N] the tail has written (in
// whichever launch form and RNG mode) and of the hub's init_soc and capacity_mass -- the env's own with per-env rows, as the ledger takes
// them; the expressions are include/chub.h's table, in f64 in the order written there, narrowed once by the store type.  Lane = env, so a
// wave's load of one telemetry column is a run of consecutive doubles; of the 38 columns only those the field set reads are loaded (need:
// the host's union over the fields, wave-uniform branches).  The rows go through LDS, as the tail's output rows do: the workgroup's
// kStBlock rows are one contiguous run of out, stored with consecutive lanes on consecutive words.  With a mask only the rows of the envs it
// names are written.  Reads telemetry (and ep.prm), writes out: nothing else.
constexpr int kStBlock = 256;
struct StepTermsArgs {
    const DevCtx *ctx;
    const uint8_t *mask;  // [N] or null: rows of envs whose byte is 0 are not written
    void *out;            // [N][columns] f32 or f64
    uint64_t need;        // bit c: some field asked for reads telemetry column c
    uint32_t fields;      // bits of the CHUB_ST_* enum
};
// the telemetry columns field f reads
static uint64_t step_term_reads(int f) {
    auto b = [](int c) { return 1ull << c; };
    const uint64_t price = b(CHUB_T_PRICE_NOW), draw = b(CHUB_T_EV0_NET) | b(CHUB_T_EV1_NET) | b(CHUB_T_HYDROGEN_POWER);
    switch (f) {
    case CHUB_ST_REWARD: return b(CHUB_T_REWARD);
    case CHUB_ST_INCOME: return b(CHUB_T_INCOME);
    case CHUB_ST_INCOME_EVS0: return b(CHUB_T_CHG0);
    case CHUB_ST_INCOME_EVS1: return b(CHUB_T_CHG1);
    case CHUB_ST_COST_EVS0: return price | b(CHUB_T_EV0_NET);
    case CHUB_ST_COST_EVS1: return price | b(CHUB_T_EV1_NET);
    case CHUB_ST_INCOME_SERVE: return b(CHUB_T_FLOW0) | b(CHUB_T_FLOW1);
    case CHUB_ST_INCOME_HYS: case CHUB_ST_HY_USE: return b(CHUB_T_HY_USE);
    case CHUB_ST_HY_COST: return price | b(CHUB_T_HYDROGEN_POWER);
    case CHUB_ST_HY_LOSS: case CHUB_ST_HY_FOR_FC: return b(CHUB_T_HY_TO_USE);
    case CHUB_ST_NOT_MEET_LOSS: case CHUB_ST_NOT_MEET: return b(CHUB_T_NOT_MEET);
    case CHUB_ST_GRID_DRAW: case CHUB_ST_GRID_EXCESS: return draw;
    case CHUB_ST_USED_RENEW: return b(CHUB_T_USED_RENEW);
    case CHUB_ST_FC_POWER: return b(CHUB_T_FC_POWER);
    case CHUB_ST_HY_ACT: return b(CHUB_T_HY_ACT);
    case CHUB_ST_GEN_HY: case CHUB_ST_HY_GEN: return b(CHUB_T_HY_FLOW_SPEED);
    case CHUB_ST_MASS_NEED: return b(CHUB_T_TOTAL_MASS_NEED);
    case CHUB_ST_FCEV_ARRIVE: return b(CHUB_T_HV_ARRIVE);
    case CHUB_ST_FCEV_LINE: return b(CHUB_T_HV_LINE);
    case CHUB_ST_FCEV_QUEUE: return b(CHUB_T_QUEUE_LEN);
    default: return b(CHUB_T_STORE_SOC);  // SOC_DEVIATION, SOC_PENALTY
    }
}
template <typename OUT>
__global__ __launch_bounds__(kStBlock) void k_step_terms(const StepTermsArgs a) {
    __shared__ __attribute__((aligned(16))) OUT s_rows[kStBlock * CHUB_ST_COUNT];
    const DevCtx *__restrict__ ctx = a.ctx;
    const HubParams &hp = ctx->hp;
    const int64_t N = hp.n_envs;
    const uint32_t fields = a.fields;
    const int C = __popc(fields);
    const int64_t env0 = (int64_t) blockIdx.x * kStBlock, env = env0 + (int64_t) threadIdx.x;
    const bool live = env < N && (!a.mask || a.mask[env] != 0);
    if (live) {
        CHUB_G(const double) tel = ctx->ev.telem;
        // column c of this env, if any field asked for reads it
#define ST_T(c) ((a.need >> (c) & 1ull) ? tel[(int64_t) (c) * N + env] : 0.0)
        const double t_reward = ST_T(CHUB_T_REWARD), t_income = ST_T(CHUB_T_INCOME), chg0 = ST_T(CHUB_T_CHG0), chg1 = ST_T(CHUB_T_CHG1);
        const double e0 = ST_T(CHUB_T_EV0_NET), e1 = ST_T(CHUB_T_EV1_NET), hydrogen_power = ST_T(CHUB_T_HYDROGEN_POWER);
        const double flow0 = ST_T(CHUB_T_FLOW0), flow1 = ST_T(CHUB_T_FLOW1), hy_use = ST_T(CHUB_T_HY_USE), hy_to_use = ST_T(CHUB_T_HY_TO_USE);
        const double not_meet = ST_T(CHUB_T_NOT_MEET), used_renew = ST_T(CHUB_T_USED_RENEW), fc_power = ST_T(CHUB_T_FC_POWER);
        const double hy_act = ST_T(CHUB_T_HY_ACT), speed = ST_T(CHUB_T_HY_FLOW_SPEED), mass_need = ST_T(CHUB_T_TOTAL_MASS_NEED);
        const double hv_arrive = ST_T(CHUB_T_HV_ARRIVE), hv_line = ST_T(CHUB_T_HV_LINE), queue = ST_T(CHUB_T_QUEUE_LEN);
        const double store_soc = ST_T(CHUB_T_STORE_SOC);
        const double p = ST_T(CHUB_T_PRICE_NOW) / 4;
#undef ST_T
        double init_soc = hp.init_soc, cap_mass = hp.cap_mass;
        if (ctx->ep.prm && (fields & (1u << CHUB_ST_SOC_DEVIATION | 1u << CHUB_ST_SOC_PENALTY))) {  // per-env rows: the env's own, as the ledger's tail
            init_soc = ctx->ep.prm[(int64_t) PRM_INIT_SOC * N + env];
            cap_mass = ctx->ep.prm[(int64_t) PRM_CAP_MASS * N + env];
        }
        const double draw = (e0 + e1) + hydrogen_power;  // MGR:262
        const double excess = draw - 2000;
        const double deviation = fabs(store_soc - init_soc);  // MGR:297
        OUT *row = s_rows + (int) threadIdx.x * C;
        int n = 0;
#define ST_OUT(f, v)                                    \
    if (fields & (1u << (f))) row[n++] = (OUT) (v)
        ST_OUT(CHUB_ST_REWARD, t_reward);
        ST_OUT(CHUB_ST_INCOME, t_income);
        ST_OUT(CHUB_ST_INCOME_EVS0, 0.42 / 4 * chg0);
        ST_OUT(CHUB_ST_INCOME_EVS1, 0.21 / 4 * chg1);
        ST_OUT(CHUB_ST_COST_EVS0, -p * e0);
        ST_OUT(CHUB_ST_COST_EVS1, -p * e1);
        ST_OUT(CHUB_ST_INCOME_SERVE, 0.8 * (flow0 + flow1));
        ST_OUT(CHUB_ST_INCOME_HYS, 6 / 1000.0 * hy_use);
        ST_OUT(CHUB_ST_HY_COST, -p * hydrogen_power);
        ST_OUT(CHUB_ST_HY_LOSS, -6 / 1000.0 * hy_to_use);
        ST_OUT(CHUB_ST_NOT_MEET_LOSS, -10 / 1000.0 * not_meet);
        ST_OUT(CHUB_ST_GRID_DRAW, draw);
        ST_OUT(CHUB_ST_GRID_EXCESS, excess > 0 ? excess : 0.0);  // beyond the 2000 kW of MGR:160
        ST_OUT(CHUB_ST_USED_RENEW, used_renew);
        ST_OUT(CHUB_ST_FC_POWER, fc_power);
        ST_OUT(CHUB_ST_HY_ACT, hy_act);
        ST_OUT(CHUB_ST_GEN_HY, speed > 0.5 ? 1.0 : 0.0);  // MGR:173-179
        ST_OUT(CHUB_ST_HY_GEN, 15 * 60 * speed);
        ST_OUT(CHUB_ST_HY_USE, hy_use);
        ST_OUT(CHUB_ST_NOT_MEET, not_meet);
        ST_OUT(CHUB_ST_HY_FOR_FC, hy_to_use);
        ST_OUT(CHUB_ST_MASS_NEED, mass_need);
        ST_OUT(CHUB_ST_FCEV_ARRIVE, hv_arrive);
        ST_OUT(CHUB_ST_FCEV_LINE, hv_line);
        ST_OUT(CHUB_ST_FCEV_QUEUE, queue);
        ST_OUT(CHUB_ST_SOC_DEVIATION, deviation);
        ST_OUT(CHUB_ST_SOC_PENALTY, fabs(deviation * cap_mass / 1000 / 0.2));  // MGR:277-290, as if the day ended now
#undef ST_OUT
    }
    // the workgroup's rows as one run of out; under a mask that names only some of them, element by element
    const bool whole = __syncthreads_and((live || env >= N) ? 1 : 0) != 0;
    const int64_t left = N - env0;
    const int total = (int) (left < kStBlock ? left : kStBlock) * C;
    OUT *dst = (OUT *) a.out + env0 * C;
    if (whole) {
        for (int i = (int) threadIdx.x; i < total; i += kStBlock) dst[i] = s_rows[i];
    } else {
        for (int i = (int) threadIdx.x; i < total; i += kStBlock)
            if (a.mask[env0 + i / C]) dst[i] = s_rows[i];
    }
}
template <typename OUT>
void launch_step_terms(const HubParams &hp, const DevCtx *ctx, uint32_t fields, const uint8_t *d_mask, OUT *d_out, hipStream_t stream) {
    if (hp.n_envs <= 0) return;
    StepTermsArgs a = {ctx, d_mask, d_out, 0ull, fields};
    for (int f = 0; f < (int) CHUB_ST_COUNT; f++)
        if (fields >> f & 1u) a.need |= step_term_reads(f);
    hipLaunchKernelGGL(k_step_terms<OUT>, dim3((unsigned) ((hp.n_envs + kStBlock - 1) / kStBlock)), dim3(kStBlock), 0, stream, a);
}
template void launch_step_terms<float>(const HubParams &, const DevCtx *, uint32_t, const uint8_t *, float *, hipStream_t);
template void launch_step_terms<double>(const HubParams &, const DevCtx *, uint32_t, const uint8_t *, double *, hipStream_t);

// -------------------------------------------------------------------- per-station deadline profiles (chub_station_profile_device)
// A station's cars binned by the time they have left: out[env][station][column][bucket], the columns of the field mask in ascending order,
// a car with `left` slots to go in bucket min(left, B) - 1.  The per-pile values are pile_decode's, i.e. k_pile_obs' columns; new here is the
// reduction of a station's 1 .. 4096 piles into C x B bins.  A workgroup owns whole envs: `group` of them at a time (the host picks it so that
// the group's piles fill the 256 lanes and its bins fit kSpBins), an env of more piles than lanes is walked in chunks of 256.  Every bin is
// one 8-byte word of LDS: a count takes 32-bit adds on its low half, a sum 64-bit adds of llrint(x * 2^q) -- integer adds commute, so the
// result does not depend on lane order, group size or grid -- and the group's blocks leave as one run of consecutive floats.  Three
// barriers per group, each reached by every lane (the mask and the empty piles skip inside the lane loops, never around a barrier).
// What a field set does not ask for is not loaded: cars and charging need the state word alone, must_charge / power* / emergency the
// class row or hot record, soc_gap alone the SoC (PHILOX: k_build_cls_soc's table; the other two replay the car's steps).
struct StationProfileArgs {
    const DevCtx *ctx;
    const uint8_t *mask;   // [N] or null: blocks of envs whose byte is 0 are not written
    const float *cls_soc;  // PHILOX: k_build_cls_soc's tables
    float *out;            // [N][2][columns][buckets]
    uint32_t fields;       // bits of the CHUB_SP_* enum
    int buckets;           // 1 .. 32
    int group;             // envs a workgroup takes at a time: group * 2 * columns * buckets <= kSpBins
};
enum ProfileField : uint32_t { SPF_CARS = 1u, SPF_CHARGING = 2u, SPF_MUST_CHARGE = 4u, SPF_POWER = 8u, SPF_POWER_CHARGING = 16u, SPF_EMERGENCY = 32u,
                               SPF_SOC_GAP = 64u };
constexpr int kSpBins = 2048;  // 16 KB of LDS; one env of all seven fields and 32 buckets takes 448
__device__ __forceinline__ unsigned long long sp_term(float x, double scale) { return (unsigned long long) __double2ll_rn((double) x * scale); }
template <int LAYOUT>
__global__ __launch_bounds__(256) void k_station_profile(const StationProfileArgs a) {
    __shared__ unsigned long long bins[kSpBins];
    const DevCtx *__restrict__ ctx = a.ctx;
    const HubParams &hp = ctx->hp;
    const Tables &tb = ctx->tb;
    const uint32_t fields = a.fields;
    const int B = a.buckets, CB = __popc(fields) * B, per_env = 2 * CB, G = a.group;
    const int S0 = hp.S[0], S = S0 + hp.S[1];
    const int64_t N = hp.n_envs;
    const int tid = (int) threadIdx.x;
    uint32_t pf = 0u;  // the pile fields behind the profile's
    if (fields & (SPF_MUST_CHARGE | SPF_EMERGENCY)) pf |= PF_EMERGENCY;
    if (fields & (SPF_POWER | SPF_POWER_CHARGING)) pf |= PF_POWER;
    if (fields & SPF_SOC_GAP) pf |= PF_SOC;
    for (int64_t env0 = (int64_t) blockIdx.x * G; env0 < N; env0 += (int64_t) gridDim.x * G) {
        const int ng = (int) (N - env0 < (int64_t) G ? N - env0 : (int64_t) G);
        const int n_bins = ng * per_env, n_piles = ng * S;
        for (int j = tid; j < n_bins; j += 256) bins[j] = 0ull;
        __syncthreads();
        for (int j = tid; j < n_piles; j += 256) {
            const int e = j / S, slot = j - e * S;
            const int64_t env = env0 + e;
            if (a.mask && !a.mask[env]) continue;
            const PileVals p = pile_decode<LAYOUT>(ctx, a.cls_soc, pf, env, slot, env * S + slot);
            if (p.left <= 0) continue;
            const int k = slot >= S0 ? 1 : 0;
            unsigned long long *col = bins + ((e * 2 + k) * CB + (p.left < B ? p.left : B) - 1);
            const float em = (pf & PF_EMERGENCY) ? emergency_of(tb.ttab[k][p.lev], p.t_soc, p.left) : 0.0f;
            if (fields & SPF_CARS) { atomicAdd((unsigned int *) col, 1u); col += B; }
            if (fields & SPF_CHARGING) { if (p.chg) atomicAdd((unsigned int *) col, 1u); col += B; }
            if (fields & SPF_MUST_CHARGE) { if (em == 10.0f) atomicAdd((unsigned int *) col, 1u); col += B; }
            if (fields & SPF_POWER) { atomicAdd(col, sp_term(p.power, 524288.0)); col += B; }
            if (fields & SPF_POWER_CHARGING) { if (p.chg) atomicAdd(col, sp_term(p.power, 524288.0)); col += B; }
            if (fields & SPF_EMERGENCY) { atomicAdd(col, sp_term(em, 1048576.0)); col += B; }
            if (fields & SPF_SOC_GAP) atomicAdd(col, sp_term(__fsub_rn(uniform_level(p.lev, 80.0f, 100.0f), p.soc), 65536.0));
        }
        __syncthreads();
        for (int j = tid; j < n_bins; j += 256) {
            const int e = j / per_env;
            if (a.mask && !a.mask[env0 + e]) continue;
            int c = (j - e * per_env) % CB / B, f = 0;  // column c is the c-th set bit of the mask
            for (uint32_t m = fields; c > 0 || !(m & 1u); m >>= 1, f++) c -= (int) (m & 1u);
            const uint32_t bit = 1u << f;
            const float unit = (bit & (SPF_POWER | SPF_POWER_CHARGING)) ? 0x1p-19f : bit == SPF_EMERGENCY ? 0x1p-20f : bit == SPF_SOC_GAP ? 0x1p-16f : 1.0f;
            a.out[env0 * per_env + j] = __fmul_rn((float) (long long) bins[j], unit);
        }
        __syncthreads();  // (the next group zeroes the bins)
    }
}
void launch_station_profile(const HubParams &hp, const DevCtx *ctx, uint32_t fields, int buckets, const uint8_t *d_mask, const float *d_cls_soc,
                            float *d_out, hipStream_t stream) {
    const int S = hp.S[0] + hp.S[1];
    if (hp.n_envs <= 0) return;
    int group = S > 0 ? 256 / S : 256;  // envs whose piles fill the workgroup's lanes ...
    const int fit = kSpBins / (2 * __builtin_popcount(fields) * buckets);  // ... as far as their bins fit (>= 4)
    group = group < 1 ? 1 : (group > fit ? fit : group);
    int64_t nb = (hp.n_envs + group - 1) / group;
    if (nb > (1 << 20)) nb = 1 << 20;  // (beyond that the workgroups stride)
    const StationProfileArgs a = {ctx, d_mask, d_cls_soc, d_out, fields, buckets, group};
    switch (slot_layout(hp)) {
    case LAYOUT_COMPAT: hipLaunchKernelGGL(k_station_profile<LAYOUT_COMPAT>, dim3((unsigned) nb), dim3(256), 0, stream, a); break;
    case LAYOUT_CURVES: hipLaunchKernelGGL(k_station_profile<LAYOUT_CURVES>, dim3((unsigned) nb), dim3(256), 0, stream, a); break;
    default: hipLaunchKernelGGL(k_station_profile<LAYOUT_PHILOX>, dim3((unsigned) nb), dim3(256), 0, stream, a); break;
    }
}

// -------------------------------------------------------------------- station-level control (chub_load_dispatch_device)
// evs_step(float)'s dispatch (catch_load, assign_on_off, rank_power_add: CHS.hpp:1169-1186 / 1480-1497) as a read-only launch in front of ANY
// step form: one kW target (or a fraction of [min_power, max_power]) per station in, the pile decisions out -- as an action row (+1 / -1 and
// the caller's two tail entries) and / or as chub_step_bits' words.  The per-pile values are pile_decode's, i.e. k_pile_obs' columns; the
// target is clamped against the unit's record as catch_load does; the decision is load_says_on, the step's own, plus what judge_feasibility
// forces on anyway (emergency == 10).  A workgroup owns whole envs, `group` at a time; a group's piles sit in LDS under their group-local
// index j = e * Sp + slot.  The urgency order (emergency descending, ties by slot: the reference's multimap keyed by -emergency):
//   BIG = false (stations of at most 64 piles): every pile counts the piles of its unit in front of it (O(S_k) LDS reads) and puts itself
//       at that rank of its unit's range of s_ord;
//   BIG = true: one bitonic sort of 64-bit keys over the whole group -- unit | inverted emergency bits (emergency is never negative, so its
//       bits order as it does) | j | flags -- after which unit (e, k)'s piles are the run from e * Sp + (k ? S0 : 0) on.  A hub of more than
//       kLdBig piles (group = 1) goes station by station: two passes.
// Then ONE lane per unit walks its run, adding the cars' powers to the f32 running sum in that order (the sum is sequential in the
// reference: rank_power_add), all units of the group side by side, and leaves +1 / -1 per pile where the pile's power was.  Every barrier
// is reached by every lane: the mask, the empty piles and the absent stations skip inside the lane loops.  Rows leave as runs of
// consecutive floats (lane = hub slot), bits as ballot words (a wave = one word).
struct LoadDispatchArgs {
    const DevCtx *ctx;
    const uint8_t *mask;   // [N] or null: rows of envs whose byte is 0 are not written
    const float *cls_soc;  // (pile_decode's argument; the SoC is not asked for)
    const float *loads;    // [N][2] one target per station
    const float *tail;     // [N][2] the two tail actions, copied into the rows (null without rows)
    float *actions;        // [N][S + 2] or null
    uint64_t *bits;        // [N][ceil(S / 64)] or null
    int units;             // 0 kW, 1 fraction of [min_power, max_power]
    int group;             // envs a workgroup takes at a time
};
constexpr int kLdSmall = 1024, kLdBig = 4096;  // piles a group holds in LDS: 12 KB / 48 KB
constexpr int kLdWords = 128;                  // bit words of a group (a hub of 8192 piles has 128)
template <int LAYOUT, bool BIG>
__global__ __launch_bounds__(256) void k_load_dispatch(const LoadDispatchArgs a) {
    __shared__ float s_pw[BIG ? kLdBig : kLdSmall];          // by j: the pile's power (0 without a car), then its decision (+1 / -1)
    __shared__ unsigned long long s_key[BIG ? kLdBig : 1];   // BIG: the sort keys
    __shared__ float s_em[BIG ? 1 : kLdSmall];               // small: by j, the pile's emergency
    __shared__ uint32_t s_ord[BIG ? 1 : kLdSmall];           // small: by position in the urgency order, j << 2 | must charge << 1 | car
    __shared__ unsigned long long s_bits[kLdWords];          // the group's bit words (a pass ORs its station in)
    const DevCtx *__restrict__ ctx = a.ctx;
    const HubParams &hp = ctx->hp;
    const Tables &tb = ctx->tb;
    const int S0 = hp.S[0], S = S0 + hp.S[1], A = S + 2, W = (S + 63) >> 6, G = a.group;
    const int64_t N = hp.n_envs;
    const int tid = (int) threadIdx.x;
    const bool cp = hp.constant_charging != 0;
    const int n_pass = (BIG && S > kLdBig) ? 2 : 1;  // (two passes: group is 1)
    for (int64_t env0 = (int64_t) blockIdx.x * G; env0 < N; env0 += (int64_t) gridDim.x * G) {
        const int ng = (int) (N - env0 < (int64_t) G ? N - env0 : (int64_t) G);
        for (int pass = 0; pass < n_pass; pass++) {
            const int lo = (n_pass == 2 && pass == 1) ? S0 : 0, hi = (n_pass == 2 && pass == 0) ? S0 : S;  // the pass's hub slots
            const int Sp = hi - lo, n = ng * Sp;
            int n_pad = 1;
            if (BIG) while (n_pad < n) n_pad <<= 1;
            // ---- every pile's car, emergency and power, as k_pile_obs reports them
            for (int j = tid; j < (BIG ? n_pad : n); j += 256) {
                float em = 0.0f, pw = 0.0f;
                bool car = false;
                int k = 0, e = 0;
                if (j < n) {
                    e = j / Sp;
                    const int slot = lo + (j - e * Sp);
                    const int64_t env = env0 + e;
                    k = slot >= S0 ? 1 : 0;
                    if (!(a.mask && !a.mask[env])) {
                        const PileVals p = pile_decode<LAYOUT>(ctx, a.cls_soc, PF_EMERGENCY | PF_POWER, env, slot, env * S + slot);
                        car = p.left > 0;
                        if (car) { em = emergency_of(tb.ttab[k][p.lev], p.t_soc, p.left); pw = p.power; }
                    }
                }
                if (j < n) s_pw[j] = pw;
                const uint32_t flags = (car && em == 10.0f ? 2u : 0u) | (car ? 1u : 0u);
                if (BIG) {
                    const unsigned long long key = ((unsigned long long) (uint32_t) (e * 2 + k) << 46) |
                                                   ((unsigned long long) (0x7FFFFFFFu - __float_as_uint(em)) << 15) |
                                                   (unsigned long long) (((uint32_t) j << 2) | flags);
                    s_key[j] = j < n ? key : ~0ull;
                } else {
                    s_em[j] = em;
                    s_ord[j] = flags;  // (by j until the ranks are known)
                }
            }
            __syncthreads();
            // ---- the urgency order
            if (BIG) {
                for (int k2 = 2; k2 <= n_pad; k2 <<= 1)
                    for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
                        for (int t = tid; t < (n_pad >> 1); t += 256) {
                            const int i = ((t & ~(j2 - 1)) << 1) | (t & (j2 - 1)), p = i | j2;
                            const unsigned long long x = s_key[i], y = s_key[p];
                            if ((x > y) == ((i & k2) == 0)) { s_key[i] = y; s_key[p] = x; }
                        }
                        __syncthreads();
                    }
            } else {
                uint32_t mine[(kLdSmall + 255) / 256];  // this lane's piles: position << 2 | flags
#pragma unroll
                for (int r = 0; r < (kLdSmall + 255) / 256; r++) {
                    const int j = tid + 256 * r;
                    mine[r] = 0u;
                    if (j < n) {
                        const int e = j / Sp, slot = j - e * Sp;
                        const int k = slot >= S0 ? 1 : 0;
                        const int ub = e * Sp + (k ? S0 : 0), Sk = hp.S[k];
                        const float em0 = s_em[j];
                        int rk = 0;
                        for (int i = ub; i < ub + Sk; i++) {
                            const float ei = s_em[i];
                            rk += (ei > em0 || (ei == em0 && i < j)) ? 1 : 0;
                        }
                        mine[r] = ((uint32_t) (ub + rk) << 2) | s_ord[j];
                    }
                }
                __syncthreads();
#pragma unroll
                for (int r = 0; r < (kLdSmall + 255) / 256; r++) {
                    const int j = tid + 256 * r;
                    if (j < n) s_ord[mine[r] >> 2] = ((uint32_t) j << 2) | (mine[r] & 3u);
                }
                __syncthreads();
            }
            // ---- one lane per unit: the target, then the running sum along the order
            if (tid < 2 * ng) {
                const int e = tid >> 1, k = tid & 1;
                const int64_t env = env0 + e;
                const int Sk = hp.S[k], off = k ? S0 : 0;
                if (Sk > 0 && off >= lo && off + Sk <= hi && !(a.mask && !a.mask[env])) {
                    const StationRec pr = rec_load(ctx->st.rec, (uint32_t) k * (uint32_t) N + (uint32_t) env);
                    float load = a.loads[env * 2 + k];
                    if (a.units == 1) {
                        float f = __fmul_rn(__fadd_rn(load, 1.0f), 0.5f);
                        f = f < 0.0f ? 0.0f : (f > 1.0f ? 1.0f : f);
                        load = __fadd_rn(pr.mn, __fmul_rn(f, __fsub_rn(pr.mx, pr.mn)));
                    }
                    if (load > pr.mx) load = pr.mx;  // catch_load's clamp (CHS.hpp:358-366)
                    else if (load < pr.mn) load = pr.mn;
                    const bool fast = hp.type[k] == 0;
                    const int base = e * Sp + (off - lo);
                    float cum = 0.0f;
                    int cars = 0;
                    for (int q = 0; q < Sk; q++) {
                        const uint32_t o = BIG ? ((uint32_t) s_key[base + q] & 0x7FFFu) : s_ord[base + q];
                        const int j = (int) (o >> 2);
                        bool on = false;
                        if (o & 1u) {
                            cum = __fadd_rn(cum, s_pw[j]);
                            on = load_says_on(cp, fast, load, cum, cars) || (o & 2u) != 0u;
                            cars++;
                        }
                        s_pw[j] = on ? 1.0f : -1.0f;
                    }
                }
            }
            __syncthreads();
            // ---- rows: the pass's pile entries, lane = hub slot; the tail with the last pass
            if (a.actions) {
                for (int j = tid; j < n; j += 256) {
                    const int e = j / Sp;
                    const int64_t env = env0 + e;
                    if (a.mask && !a.mask[env]) continue;
                    a.actions[env * A + (lo + (j - e * Sp))] = s_pw[j];
                }
                if (pass == n_pass - 1)
                    for (int j = tid; j < 2 * ng; j += 256) {
                        const int64_t env = env0 + (j >> 1);
                        if (a.mask && !a.mask[env]) continue;
                        a.actions[env * A + S + (j & 1)] = a.tail[env * 2 + (j & 1)];
                    }
            }
            // ---- bits: lane = bit of the group's words, a wave = one word (ng * W * 64 positions: whole waves)
            if (a.bits) {
                for (int b = tid; b < ng * W * 64; b += 256) {
                    const int e = b / (W * 64), slot = b - e * (W * 64);
                    const bool on = slot >= lo && slot < hi && s_pw[e * Sp + (slot - lo)] > 0.0f;
                    const unsigned long long word = __ballot(on);
                    if ((tid & 63) == 0) {
                        const unsigned long long all = (pass ? s_bits[b >> 6] : 0ull) | word;
                        s_bits[b >> 6] = all;
                        const int64_t env = env0 + e;
                        if (pass == n_pass - 1 && !(a.mask && !a.mask[env])) a.bits[env * W + (slot >> 6)] = all;
                    }
                }
            }
            __syncthreads();  // (the next pass / group overwrites the LDS arrays)
        }
    }
}
int load_dispatch_group(const HubParams &hp, bool big) {
    const int S = hp.S[0] + hp.S[1];
    const int cap = big ? kLdBig : kLdSmall;
    int group = S > cap ? 1 : cap / S;
    return group > 128 ? 128 : group;  // (two units per env, one lane each)
}
void launch_load_dispatch(const HubParams &hp, const DevCtx *ctx, int units, const uint8_t *d_mask, const float *d_cls_soc, const float *d_loads,
                          const float *d_tail, float *d_actions, uint64_t *d_bits, hipStream_t stream) {
    const int S = hp.S[0] + hp.S[1];
    if (hp.n_envs <= 0 || S <= 0) return;
    const bool big = hp.S[0] > 64 || hp.S[1] > 64;
    const int group = load_dispatch_group(hp, big);
    int64_t nb = (hp.n_envs + group - 1) / group;
    if (nb > (1 << 20)) nb = 1 << 20;  // (beyond that the workgroups stride)
    const LoadDispatchArgs a = {ctx, d_mask, d_cls_soc, d_loads, d_tail, d_actions, d_bits, units, group};
    const dim3 grid((unsigned) nb), block(256);
    switch (slot_layout(hp)) {
    case LAYOUT_COMPAT:
        if (big) hipLaunchKernelGGL((k_load_dispatch<LAYOUT_COMPAT, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((k_load_dispatch<LAYOUT_COMPAT, false>), grid, block, 0, stream, a);
        break;
    case LAYOUT_CURVES:  // (at most 64 piles per station in this mode)
        hipLaunchKernelGGL((k_load_dispatch<LAYOUT_CURVES, false>), grid, block, 0, stream, a);
        break;
    default:
        if (big) hipLaunchKernelGGL((k_load_dispatch<LAYOUT_PHILOX, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((k_load_dispatch<LAYOUT_PHILOX, false>), grid, block, 0, stream, a);
        break;
    }
}

// PHILOX reset: evs_reset's initial occupancy per (station, env) unit -- init_station_car_number(mu, 3) (CHS.hpp:832-842)
// thinned by the balk test of an empty queue -- drawn once per unit here (every lane of the unit used to redo it),
// handed to k_slot<RESET> through this tick's pk word: arrivals | arrivals that stay << 8.
__device__ __forceinline__ void reset_levels_body(const DevCtx *__restrict__ ctx, const StepArgs &sa) {
    // four lanes per unit: lane q takes the Philox blocks q, q + 4, ... of the unit's arrival words (four arrivals each), the
    // quad adds up.  (One lane per unit walking all its arrivals was a 15-iteration dependent chain at two waves per SIMD:
    // 20 us per reset.)
    const uint32_t tick = sa.tick;
    const HubParams &hp = ctx->hp;
    const Tables &tb = ctx->tb;
    const int64_t N = hp.n_envs;
    const int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int q = (int) (t & 3);
    int k = 0;
    int64_t env = 0;
    const bool live = range_unit(sa, t >> 2, 2, k, env);  // the units of the envs the call names: both stations of env_lo .. env_hi
    const int64_t u = (int64_t) k * N + env;
    const bool served = live && in_group(sa, env);
    const int S = hp.S[k], mu = S / 2;  // round(charge_number / 2) on ints, CHS.hpp:1276
    PhiloxCtx px{hp.key[0], hp.key[1], CHUB_TICK(hp, tick), (uint32_t) (hp.env_id0 + env)};
    const float cn = __fadd_rn(normal_from_word(tb.normal_icdf, tb.normal_tail, px.block(SITE_INIT, (uint32_t) k, 0).v[0]), (float) mu);
    int n_in = (int) roundf(cn);
    n_in = n_in > mu + 3 ? mu + 3 : (n_in < mu - 3 ? mu - 3 : n_in);
    int true_in = 0;
    // arrival j (word 1 + j of the unit's SITE_ARRIVE stream) stays iff u <= expf(-0.01*(line+j)) and j <= S
    for (int blk = q; served && 4 * blk <= n_in; blk += 4) {
        const U4 b = px.block(SITE_ARRIVE, (uint32_t) k, (uint32_t) blk);
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const int j = 4 * blk + w - 1;
            if (j < 0 || j >= n_in) continue;
            const int thr = (int) tb.thr_balk[j < kBalkTab ? j : kBalkTab - 1];
            true_in += ((int) (b.v[w] % 1000u) <= thr && j <= S) ? 1 : 0;
        }
    }
    true_in += __shfl_xor(true_in, 1);
    true_in += __shfl_xor(true_in, 2);
    if (served && q == 0)
        ctx->st.pk[tick & 1u][u] = ((uint32_t) n_in & 0xFFFFu) | ((uint32_t) true_in << 16);  // n_in: signed 16 bits
}
__global__ void k_reset_levels(const DevCtx *__restrict__ ctx, StepArgs sa) { reset_levels_body(ctx, sa); }
// ... in front of the masked reset of an auto-reset call, whose mask may name nobody (every workgroup then returns at entry)
__global__ void k_reset_levels_gated(const DevCtx *__restrict__ ctx, StepArgs sa) {
    if (mask_is_empty(sa)) return;
    reset_levels_body(ctx, sa);
}

// fresh launches (StepArgs::fresh): this step's station-level draws, made right in front of the slot kernel -- what the
// previous launch's level blocks would have left in pk[tick & 1]
__global__ void k_draw_levels(const DevCtx *__restrict__ ctx, StepArgs sa) {
    const HubParams &hp = ctx->hp;
    const int64_t N = hp.n_envs;
    int kk = 0;
    int64_t env = 0;
    if (!range_unit(sa, (int64_t) blockIdx.x * blockDim.x + threadIdx.x, 2, kk, env)) return;
    const int64_t u = (int64_t) kk * N + env;
    if (!in_group(sa, env)) return;
    const int t = sa.env_clk ? clk_t(env_clk(sa, N, env)) : sa.t;
    // tape mode: the caller's recorded draws instead of this build's (the 64-bit layout above), decoded the same way
    const int line_now = pkd_line(ctx->st.rec[4u * (uint32_t) u + 3u]);
    ctx->st.pk[sa.tick & 1u][u] = sa.pk_tape ? dk_make(sa.pk_tape[u], line_now, hp.type[kk] == 0)
                                             : draw_decoded_levels(hp, ctx->tb, CHUB_TICK(hp, sa.tick), t, kk, env, line_now, hp.type[kk] == 0);
}

// per-env clocks, a call on a subset of the envs: the clocks of the envs outside the launched range move to the other buffer as they are
__global__ void k_keep_clocks(uint16_t *dst, const uint16_t *src, int64_t n) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// ------------------------------------------------------------------------------------- launchers
// kernel launch with the dispatch's own start / stop timestamps when asked for (chub_profile_*), a plain launch otherwise
#define CHUB_LAUNCH(kernel, grid, block, stream, ev0, ev1, ...)                                         \
    do {                                                                                                \
        if ((ev0) || (ev1)) hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, ev0, ev1, 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__);                           \
    } while (0)
static inline int64_t blocks_for(int64_t n_envs, int H, int block) {
    const int64_t upb = (int64_t) (block / 64) * (64 / H);
    return (n_envs + upb - 1) / upb;
}
// slot_body_split2: a wave's units lie end to end over its 128 virtual lanes
static inline int64_t blocks_for_split2(int64_t n_envs, int U, int block) {
    const int64_t upb = (int64_t) (block / 64) * (128 / U);
    return (n_envs + upb - 1) / upb;
}

// The launchers launch the forms chub_plan.h names (LaunchPlan per handle, CallPlan per call) and decide nothing themselves.
// ev0 / ev1 (may be null): kernel start / stop timestamps of the dispatch itself (hipExtLaunchKernelGGL), what
// chub_profile_* reports -- plain hipEventRecord pairs around a launch also count the gap in front of it
static void launch_levels(LevelsForm lv, const DevCtx *ctx, const StepArgs &sa, hipStream_t stream) {
    const int64_t n = (int64_t) sa.env_hi - sa.env_lo + 1;
    switch (lv) {
    case LEVELS_NONE: break;
    case LEVELS_DRAW: hipLaunchKernelGGL(k_draw_levels, dim3((unsigned) ((2 * n + 255) / 256)), dim3(256), 0, stream, ctx, sa); break;
    case LEVELS_RESET:
        if (sa.skip_count) hipLaunchKernelGGL(k_reset_levels_gated, dim3((unsigned) ((8 * n + 255) / 256)), dim3(256), 0, stream, ctx, sa);
        else hipLaunchKernelGGL(k_reset_levels, dim3((unsigned) ((8 * n + 255) / 256)), dim3(256), 0, stream, ctx, sa);
        break;
    }
}

static PackedArgs make_packed_args(const HubParams &hp, const StepArgs &sa, const PackedPtrs &pp);

template <bool TAPE, bool RESET, bool MASKED, bool BITS>
static void launch_packed(const HubParams &hp, const LaunchPlan &lp, const DevCtx *ctx, const StepArgs &sa, hipStream_t stream, const PackedPtrs &pp,
                          hipEvent_t ev0, hipEvent_t ev1) {
    const PackedArgs pa = make_packed_args(hp, sa, pp);
    // every workgroup of the batch, or (a call on a subset of the envs) those of the range of envs it names
    const uint32_t nb = MASKED ? (uint32_t) (sa.env_hi / hp.epb - sa.env_lo / hp.epb + 1) : (uint32_t) ((hp.n_envs + hp.epb - 1) / hp.epb);
    switch ((PackedForm) lp.packed) {
    case PACKED_SMALL:
        CHUB_LAUNCH((k_slot_packed<kPackedBlock, kSlotsPerLane, TAPE, RESET, false, MASKED, BITS>), dim3(nb), dim3(kPackedBlock), stream, ev0, ev1, ctx, sa, pa);
        break;
    case PACKED_SMALL_WIDE:
        CHUB_LAUNCH((k_slot_packed<kPackedBlock, kSlotsPerLane, TAPE, RESET, true, MASKED, BITS>), dim3(nb), dim3(kPackedBlock), stream, ev0, ev1, ctx, sa, pa);
        break;
    case PACKED_LARGE:
        CHUB_LAUNCH((k_slot_packed<kBigBlock, kBigSlotsPerLane, TAPE, RESET, false, MASKED, BITS>), dim3(nb), dim3(kBigBlock), stream, ev0, ev1, ctx, sa, pa);
        break;
    case PACKED_LARGE_WIDE:
        CHUB_LAUNCH((k_slot_packed<kBigBlock, kBigSlotsPerLane, TAPE, RESET, true, MASKED, BITS>), dim3(nb), dim3(kBigBlock), stream, ev0, ev1, ctx, sa, pa);
        break;
    case PACKED_NONE: break;
    }
}

// one launch per station: the reference streams are consumed station 0 first, then station 1
template <bool RESET, int MODE>
static void launch_stations(const HubParams &hp, const LaunchPlan &lp, const DevCtx *ctx, const StepArgs &sa, hipStream_t stream, hipEvent_t ev0,
                            hipEvent_t ev1) {
    constexpr int BLOCK = 256;
    // (COMPAT units take exactly S lanes, the PHILOX wave-local kernel's the next power of two: its sums are DPP butterflies)
    const int64_t nb0 = blocks_for(hp.n_envs, MODE == MODE_COMPAT ? hp.U[0] : hp.H[0], BLOCK), nb1 = blocks_for(hp.n_envs, MODE == MODE_COMPAT ? hp.U[1] : hp.H[1], BLOCK);
    for (int k = 0; k < 2; k++) {
        StepArgs s2 = sa;
        s2.station_filter = k;
        hipEvent_t e0 = k == 0 ? ev0 : nullptr, e1 = k == 1 ? ev1 : nullptr;
        switch ((StationKernel) lp.station[k]) {
        case STATION_UNIT_ANY: CHUB_LAUNCH((k_slot_unit_any<RESET, MODE>), dim3((unsigned) hp.n_envs), dim3(256), stream, e0, e1, ctx, s2, k); break;
        case STATION_UNIT: CHUB_LAUNCH((k_slot_unit<RESET, MODE>), dim3((unsigned) hp.n_envs), dim3(256), stream, e0, e1, ctx, s2, k); break;
        case STATION_WAVE:
        case STATION_CURVES: CHUB_LAUNCH((k_slot<RESET, MODE, BLOCK>), dim3((unsigned) (k ? nb1 : nb0)), dim3(BLOCK), stream, e0, e1, ctx, s2, nb0); break;
        }
    }
}

// COMPAT split step, in front of its slot pass: the empty-slot counts of every unit, whatever envs the call names, where they are not
// the previous pass's (they are then good for whoever is stepped next), and the step's own stream walks, one env per lane, where they
// have not run beside the previous step's tails (k_env_walk).  Returns the start event the slot pass still has to take.
static hipEvent_t launch_split_front(const HubParams &hp, const DevCtx *ctx, const StepArgs &sa, hipStream_t stream, hipEvent_t ev0) {
    constexpr int BLOCK = 256;
    if (sa.empt_fresh && !sa.walked) {
        const int64_t nb0 = blocks_for(hp.n_envs, hp.U[0], BLOCK), nb1 = blocks_for(hp.n_envs, hp.U[1], BLOCK);
        StepArgs all = sa;
        all.env_mask = nullptr;
        CHUB_LAUNCH((k_compat_empties<BLOCK>), dim3((unsigned) (nb0 + nb1)), dim3(BLOCK), stream, ev0, (hipEvent_t) nullptr, ctx, all, nb0);
        ev0 = nullptr;
    }
    if (!sa.walked) {
        CHUB_LAUNCH((k_compat_walk<false>), dim3((unsigned) ((hp.n_envs + 255) / 256)), dim3(256), stream, ev0, (hipEvent_t) nullptr, ctx, sa);
        ev0 = nullptr;
    }
    return ev0;
}

template <bool RESET>
void launch_slot(const CallPlan &cp, const HubParams &hp, const LaunchPlan &lp, const DevCtx *ctx, const StepArgs &sa, hipStream_t stream,
                 const PackedPtrs &pp, hipEvent_t ev0, hipEvent_t ev1) {
    constexpr int BLOCK = 256;
    const int64_t nbh0 = blocks_for(hp.n_envs, hp.H[0], BLOCK), nbh1 = blocks_for(hp.n_envs, hp.H[1], BLOCK);
    const int64_t nbu0 = blocks_for(hp.n_envs, hp.U[0], BLOCK), nbu1 = blocks_for(hp.n_envs, hp.U[1], BLOCK);
    launch_levels(cp.levels, ctx, sa, stream);
    switch (cp.slot) {
    case SLOT_PACKED: launch_packed<false, RESET, false, false>(hp, lp, ctx, sa, stream, pp, ev0, ev1); break;
    case SLOT_PACKED_MASKED: launch_packed<false, RESET, true, false>(hp, lp, ctx, sa, stream, pp, ev0, ev1); break;
    case SLOT_PACKED_TAPE: launch_packed<true, RESET, false, false>(hp, lp, ctx, sa, stream, pp, ev0, ev1); break;  // (tape mode runs in lock-step)
    case SLOT_PACKED_BITS:  // one bit per pile (lock-step steps only)
        if constexpr (!RESET) launch_packed<false, false, false, true>(hp, lp, ctx, sa, stream, pp, ev0, ev1);
        break;
    case SLOT_CURVES: CHUB_LAUNCH((k_slot_curves<RESET, BLOCK>), dim3((unsigned) (nbh0 + nbh1)), dim3(BLOCK), stream, ev0, ev1, ctx, sa, nbh0); break;
    case SLOT_WAVE: CHUB_LAUNCH((k_slot<RESET, MODE_PHILOX, BLOCK>), dim3((unsigned) (nbh0 + nbh1)), dim3(BLOCK), stream, ev0, ev1, ctx, sa, nbh0); break;
    case SLOT_STATIONS: launch_stations<RESET, MODE_PHILOX>(hp, lp, ctx, sa, stream, ev0, ev1); break;
    case SLOT_SPLIT:  // the split step: (empties ->) the stream walks, one env per lane -> the slots of both stations in one launch
        if constexpr (RESET) {
            CHUB_LAUNCH((k_compat_walk<true>), dim3((unsigned) ((hp.n_envs + 255) / 256)), dim3(256), stream, ev0, (hipEvent_t) nullptr, ctx, sa);
            ev0 = nullptr;
        } else {
            ev0 = launch_split_front(hp, ctx, sa, stream, ev0);
        }
        CHUB_LAUNCH((k_slot_split<RESET, BLOCK>), dim3((unsigned) (nbu0 + nbu1)), dim3(BLOCK), stream, ev0, ev1, ctx, sa, nbu0);
        break;
    case SLOT_SPLIT2: {  // ... with two slots per lane (stations of 8 to 64 piles: at most 8 units per virtual wave)
        ev0 = launch_split_front(hp, ctx, sa, stream, ev0);
        const int64_t sb0 = blocks_for_split2(hp.n_envs, hp.U[0], BLOCK), sb1 = blocks_for_split2(hp.n_envs, hp.U[1], BLOCK);
        CHUB_LAUNCH((k_slot_split2<BLOCK>), dim3((unsigned) (sb0 + sb1)), dim3(BLOCK), stream, ev0, ev1, ctx, sa, sb0);
        break;
    }
    case SLOT_COMPAT_STATIONS: launch_stations<RESET, MODE_COMPAT>(hp, lp, ctx, sa, stream, ev0, ev1); break;
    }
}
template void launch_slot<true>(const CallPlan &, const HubParams &, const LaunchPlan &, const DevCtx *, const StepArgs &, hipStream_t, const PackedPtrs &,
                                hipEvent_t, hipEvent_t);
template void launch_slot<false>(const CallPlan &, const HubParams &, const LaunchPlan &, const DevCtx *, const StepArgs &, hipStream_t, const PackedPtrs &,
                                 hipEvent_t, hipEvent_t);

// COMPAT split step, lock-step steps of every env of a handle whose stations take the two-slots-per-lane pass: the slot pass of step i
// (sa) beside the stream walks of step i + 1 (sw: walk_far), k_slot_walk2.  Step i's own walk first where it has not run (the first step
// after a reset or anything else that voided it: near, from the committed streams), the empty-slot counts in front of it where they are
// not the previous pass's.
void launch_slot_walk2(const LaunchPlan &lp, const HubParams &hp, const DevCtx *ctx, const StepArgs &sa, const StepArgs &sw, hipStream_t stream,
                       hipEvent_t ev0, hipEvent_t ev1) {
    constexpr int BLOCK = 256;
    ev0 = launch_split_front(hp, ctx, sa, stream, ev0);
    const int64_t sb0 = blocks_for_split2(hp.n_envs, hp.U[0], BLOCK), sb1 = blocks_for_split2(hp.n_envs, hp.U[1], BLOCK);
    switch ((CompatForm) lp.compat) {
    case COMPAT_WALK2_32: {
        const int nwalk = (int) ((hp.n_envs + 31) / 32);
        CHUB_LAUNCH((k_slot_walk2<BLOCK, 32>), dim3((unsigned) (nwalk + sb0 + sb1)), dim3(BLOCK), stream, ev0, ev1, ctx, sa, sw, sb0, nwalk);
        break;
    }
    case COMPAT_WALK2_64: {
        const int nwalk = (int) ((hp.n_envs + 63) / 64);
        CHUB_LAUNCH((k_slot_walk2<BLOCK, 64>), dim3((unsigned) (nwalk + sb0 + sb1)), dim3(BLOCK), stream, ev0, ev1, ctx, sa, sw, sb0, nwalk);
        break;
    }
    default: break;
    }
}

static PackedArgs make_packed_args(const HubParams &hp, const StepArgs &sa, const PackedPtrs &pp) {
    PackedArgs pa;
    for (int k = 0; k < 2; k++) {
        pa.S[k] = (uint32_t) hp.S[k];
        pa.type[k] = (uint32_t) hp.type[k];
    }
    pa.n_envs = (uint32_t) hp.n_envs;
    pa.epb = (uint32_t) hp.epb;
    pa.magic = (1u << 20) / (uint32_t) (hp.S[0] + hp.S[1]) + 1u;
    pa.cls_delta = (uint32_t) ((const char *) pp.cls[1] - (const char *) pp.cls[0]);
    pa.state = (CHUB_G(uint32_t)) pp.hot;
    pa.rec = (CHUB_G(uint32_t)) pp.rec;
    pa.pk = (CHUB_G(const uint32_t)) pp.pk[sa.tick & 1u];
    pa.actions = sa.act_bits ? (CHUB_G(const float)) (const void *) sa.act_bits : (CHUB_G(const float)) sa.actions;
    pa.cls0 = (CHUB_G(const float)) pp.cls[0];
    pa.ttab2 = (CHUB_G(const float)) pp.ttab2;
    pa.car_tape = (CHUB_G(const uint32_t)) sa.car_tape;
    pa.key[0] = hp.key[0];
    pa.key[1] = hp.key[1];
    pa.gid0 = (uint32_t) hp.env_id0;
    pa.tick = sa.tick;
    pa.tick_base = hp.tick_base;
    for (int j = 0; j < 8; j++) pa.late[j] = pp.late8[j];
    pa.env_mask = (CHUB_G(const uint8_t)) sa.env_mask;
    pa.blk0 = sa.env_mask ? (uint32_t) (sa.env_lo / hp.epb) : 0u;
    pa.xcd = hp.xcd ? (uint32_t) ((hp.n_envs + hp.epb - 1) / hp.epb) : 0u;  // (the grid of an unmasked launch: launch_slot)
    pa.tail_act = (CHUB_G(float)) pp.st->tail_act;
    pa.stay8 = (CHUB_G(uint8_t)) pp.stay8;
    pa.rec_prev = nullptr;
    return pa;
}

// the whole PHILOX lock-step step as ONE launch (k_step_fused / k_step_tailwave)
void launch_step_fused(const CallPlan &cp, const HubParams &hp, const DevCtx *ctx, const StepArgs &sa, hipStream_t stream, const PackedPtrs &pp,
                       hipEvent_t ev0, hipEvent_t ev1) {
    launch_levels(cp.levels, ctx, sa, stream);
    const PackedArgs pa = make_packed_args(hp, sa, pp);
    TailArgs ta = make_tail_args(*pp.ev, *pp.st, hp, sa, pp, false);
    // the tails read their two actions from the action rows (the workgroup has just had them in cache), or with one bit per pile from
    // the caller's [N][2] array
    ta.tail_act = (cp.one == ONE_FUSED_BITS || cp.one == ONE_TAILWAVE_BITS) ? (CHUB_G(const float)) sa.act_tail : nullptr;
    const uint32_t nb = (uint32_t) ((hp.n_envs + hp.epb - 1) / hp.epb);
    switch (cp.one) {  // (the tail wave's lanes are the workgroup's envs)
    case ONE_FUSED: CHUB_LAUNCH((k_step_fused<kPackedBlock, kSlotsPerLane>), dim3(nb), dim3(kPackedBlock), stream, ev0, ev1, ctx, sa, pa, ta); break;
    case ONE_TAILWAVE: CHUB_LAUNCH((k_step_tailwave<kPackedBlock, kSlotsPerLane>), dim3(nb), dim3(kPackedBlock + 64), stream, ev0, ev1, ctx, sa, pa, ta); break;
    case ONE_FUSED_BITS: CHUB_LAUNCH((k_step_fused<kPackedBlock, kSlotsPerLane, true>), dim3(nb), dim3(kPackedBlock), stream, ev0, ev1, ctx, sa, pa, ta); break;
    case ONE_TAILWAVE_BITS:
        CHUB_LAUNCH((k_step_tailwave<kPackedBlock, kSlotsPerLane, true>), dim3(nb), dim3(kPackedBlock + 64), stream, ev0, ev1, ctx, sa, pa, ta);
        break;
    case ONE_FUSED_TAPE:  // station draws, car variates and the tail's variates all come from the tape
        CHUB_LAUNCH((k_step_fused<kPackedBlock, kSlotsPerLane, false, true>), dim3(nb), dim3(kPackedBlock), stream, ev0, ev1, ctx, sa, pa, ta);
        break;
    case ONE_NONE: break;
    }
}

// a span of n_steps lock-step steps from `sa` (the span's first step) in one launch: chub_run_steps, PHILOX handles on the one-launch step
void launch_steps_fused(const HubParams &hp, const LaunchPlan &lp, const DevCtx *ctx, const StepArgs &sa, hipStream_t stream, const PackedPtrs &pp,
                        int n_steps, int pc0, int64_t first, const float *const *batches, int n_batches, float *const *packed2) {
    launch_levels(sa.fresh ? LEVELS_DRAW : LEVELS_NONE, ctx, sa, stream);
    const PackedArgs pa = make_packed_args(hp, sa, pp);
    TailArgs ta = make_tail_args(*pp.ev, *pp.st, hp, sa, pp, false);
    ta.tail_act = nullptr;  // (the tails read their two actions from the action rows, as in k_step_fused)
    SpanArgs sp = {};
    sp.n_steps = n_steps;
    sp.pc0 = pc0;
    sp.first = (uint32_t) (first % (2 * n_batches));  // (only first mod n_batches and first mod 2 matter: 2 * n_batches is a multiple of both)
    sp.n_batches = n_batches;
    sp.D = hp.obs_dim;
    for (int j = 0; j < 8; j++) sp.actions[j] = batches[j < n_batches ? j : 0];
    sp.packed[0] = packed2[0];
    sp.packed[1] = packed2[1];
    for (int q = 0; q < 2; q++) {
        sp.pk[q] = (CHUB_G(const uint32_t)) pp.pk[q];
        sp.drw[q] = (CHUB_G(const uint32_t)) pp.ev->drw[q];
        sp.drw_cnt[q] = (CHUB_G(const uint8_t)) pp.ev->drw_cnt[q];
    }
    sp.price = (CHUB_G(const double)) pp.tb->price;
    sp.pvT = (CHUB_G(const double)) pp.tb->pvT;
    sp.wdT = (CHUB_G(const double)) pp.tb->wdT;
    sp.sin96 = (CHUB_G(const double)) pp.tb->sin96;
    const uint32_t nb = (uint32_t) ((hp.n_envs + hp.epb - 1) / hp.epb);
    if (lp.span_piped)  // (the tail wave's lanes are the workgroup's envs)
        hipLaunchKernelGGL((k_steps_piped<kPackedBlock, kSlotsPerLane>), dim3(nb), dim3(kPackedBlock + 64), 0, stream, ctx, sa, pa, ta, sp);
    else
        hipLaunchKernelGGL((k_steps_fused<kPackedBlock, kSlotsPerLane>), dim3(nb), dim3(kPackedBlock), 0, stream, ctx, sa, pa, ta, sp);
}

// COMPAT lock-step reset / step of a handle whose envs all fit one workgroup: one launch
template <bool RESET>
void launch_compat_small(const HubParams &hp, const DevCtx *ctx, const StepArgs &sa, hipStream_t stream, const PackedPtrs &pp) {
    const TailArgs ta = make_tail_args(*pp.ev, *pp.st, hp, sa, pp, RESET);
    hipLaunchKernelGGL(k_compat_small<RESET>, dim3(1), dim3(kCompatSmallBlock), 0, stream, ctx, sa, ta);
}
template void launch_compat_small<true>(const HubParams &, const DevCtx *, const StepArgs &, hipStream_t, const PackedPtrs &);
template void launch_compat_small<false>(const HubParams &, const DevCtx *, const StepArgs &, hipStream_t, const PackedPtrs &);

template <bool RESET>
void launch_env(EnvForm f, const HubParams &hp, const DevCtx *ctx, const StepArgs &sa, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1,
                const PackedPtrs &pp) {
    const TailArgs ta = make_tail_args(*pp.ev, *pp.st, hp, sa, pp, RESET);
    // the tail blocks of every env, or (per-env clocks) of the range of envs the call names
    const int nb_env = sa.env_clk ? sa.env_hi / kEnvBlock - sa.env_lo / kEnvBlock + 1 : (int) ((hp.n_envs + kEnvBlock - 1) / kEnvBlock);
    if (sa.env_clk && sa.env_mask) {
        // the clocks are double-buffered by launch parity and the tail moves those of the envs of its blocks to the other buffer; the
        // envs outside the range keep theirs: copied here
        const int64_t N = hp.n_envs;
        hipLaunchKernelGGL(k_keep_clocks, dim3((unsigned) ((N + 255) / 256)), dim3(256), 0, stream, sa.env_clk + (int64_t) ((sa.tick + 1u) & 1u) * N,
                           (const uint16_t *) sa.env_clk + (int64_t) (sa.tick & 1u) * N, N);
    }
    // PHILOX: + the level-draw workgroups: next step's state-independent variates (3 lanes per env: two stations, one env)
    const unsigned nb = (unsigned) nb_env + (unsigned) ((3 * ((int64_t) sa.env_hi - sa.env_lo + 1) + kEnvBlock - 1) / kEnvBlock);
    switch (f) {
    case ENV_PHILOX: CHUB_LAUNCH((k_env<RESET, MODE_PHILOX, false>), dim3(nb), dim3(kEnvBlock), stream, ev0, ev1, ctx, sa, ta, nb_env); break;
    case ENV_PHILOX_CLOCKS: CHUB_LAUNCH((k_env<RESET, MODE_PHILOX, true>), dim3(nb), dim3(kEnvBlock), stream, ev0, ev1, ctx, sa, ta, nb_env); break;
    case ENV_PHILOX_TAPE:  // tape mode (lock-step): the tail's variates from the caller
        CHUB_LAUNCH((k_env<RESET, MODE_PHILOX, false, true>), dim3(nb), dim3(kEnvBlock), stream, ev0, ev1, ctx, sa, ta, nb_env);
        break;
    case ENV_COMPAT: CHUB_LAUNCH((k_env<RESET, MODE_COMPAT, false>), dim3((unsigned) nb_env), dim3(kEnvBlock), stream, ev0, ev1, ctx, sa, ta, nb_env); break;
    case ENV_COMPAT_CLOCKS: CHUB_LAUNCH((k_env<RESET, MODE_COMPAT, true>), dim3((unsigned) nb_env), dim3(kEnvBlock), stream, ev0, ev1, ctx, sa, ta, nb_env); break;
    case ENV_PHILOX_PARAMS:  // per-env hub parameters (chub_create_params)
        CHUB_LAUNCH((k_env<RESET, MODE_PHILOX, false, false, true>), dim3(nb), dim3(kEnvBlock), stream, ev0, ev1, ctx, sa, ta, nb_env);
        break;
    case ENV_PHILOX_PARAMS_CLOCKS:
        CHUB_LAUNCH((k_env<RESET, MODE_PHILOX, true, false, true>), dim3(nb), dim3(kEnvBlock), stream, ev0, ev1, ctx, sa, ta, nb_env);
        break;
    case ENV_COMPAT_PARAMS:
        CHUB_LAUNCH((k_env<RESET, MODE_COMPAT, false, false, true>), dim3((unsigned) nb_env), dim3(kEnvBlock), stream, ev0, ev1, ctx, sa, ta, nb_env);
        break;
    case ENV_COMPAT_PARAMS_CLOCKS:
        CHUB_LAUNCH((k_env<RESET, MODE_COMPAT, true, false, true>), dim3((unsigned) nb_env), dim3(kEnvBlock), stream, ev0, ev1, ctx, sa, ta, nb_env);
        break;
    }
}
template void launch_env<true>(EnvForm, const HubParams &, const DevCtx *, const StepArgs &, hipStream_t, hipEvent_t, hipEvent_t, const PackedPtrs &);
template void launch_env<false>(EnvForm, const HubParams &, const DevCtx *, const StepArgs &, hipStream_t, hipEvent_t, hipEvent_t, const PackedPtrs &);

// COMPAT split step, lock-step: the tails of step `sa` + the walks of the step after it (`sw`: its clock and tick)
void launch_env_walk(const HubParams &hp, const DevCtx *ctx, const StepArgs &sa, const StepArgs &sw, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1,
                     const PackedPtrs &pp) {
    const TailArgs ta = make_tail_args(*pp.ev, *pp.st, hp, sa, pp, false);
    const int nb_env = (int) ((hp.n_envs + kEnvBlock - 1) / kEnvBlock);
    const unsigned nb = (unsigned) nb_env + (unsigned) ((hp.n_envs + 255) / 256);
    CHUB_LAUNCH(k_env_walk, dim3(nb), dim3(kEnvBlock), stream, ev0, ev1, ctx, sa, ta, sw, nb_env);
}

// A pair of lock-step steps of every env whose tails share one launch (k_env_pair; PHILOX handles on the small tile of the packed slot kernel):
// sa / sb: the pair's first and second step; chain_start: no pair ran right before this one (k_pair_draws first, behind the first step's own
// station draws if that step is a fresh one); more: another pair follows at once; sel: which of the two blocks of env draws this pair reads
void launch_pair(const HubParams &hp, const DevCtx *ctx, const StepArgs &sa_in, const StepArgs &sb_in, hipStream_t stream, const PackedPtrs &pp,
                 const PairBufs &pb, int sel, bool chain_start, bool more) {
    StepArgs sa = sa_in, sb = sb_in;
    const int64_t N = hp.n_envs;
    const int nb_env = (int) ((N + kEnvBlock - 1) / kEnvBlock);
    const unsigned nb_lev = (unsigned) ((3 * N + kEnvBlock - 1) / kEnvBlock);
    PairArgs pr;
    pr.rec_a = (CHUB_G(const uint32_t)) pb.rec_a;
    pr.pkraw = (CHUB_G(uint64_t)) pb.pkraw;
    for (int q = 0; q < 2; q++) {
        pr.drw_in[q] = (CHUB_G(const uint32_t)) pb.drw[sel][q];
        pr.cnt_in[q] = (CHUB_G(const uint8_t)) pb.cnt[sel][q];
        pr.drw_out[q] = (CHUB_G(uint32_t)) pb.drw[sel ^ 1][q];
        pr.cnt_out[q] = (CHUB_G(uint8_t)) pb.cnt[sel ^ 1][q];
    }
    const uint32_t xcd = hp.xcd ? 1u : 0u;
    if (chain_start) {
        launch_levels(sa.fresh ? LEVELS_DRAW : LEVELS_NONE, ctx, sa, stream);
        PairArgs p0 = pr;  // (the prologue fills the blocks this pair reads)
        for (int q = 0; q < 2; q++) {
            p0.drw_out[q] = (CHUB_G(uint32_t)) pb.drw[sel][q];
            p0.cnt_out[q] = (CHUB_G(uint8_t)) pb.cnt[sel][q];
        }
        hipLaunchKernelGGL(k_pair_draws, dim3(nb_lev), dim3(kEnvBlock), 0, stream, ctx, sa, p0, xcd);
    }
    sa.fresh = 0;  // (every draw of both steps has been made ahead)
    sb.fresh = 0;
    const uint32_t nb = (uint32_t) ((N + hp.epb - 1) / hp.epb);
    PackedArgs pa = make_packed_args(hp, sa, pp);
    pa.rec = (CHUB_G(uint32_t)) pb.rec_a;
    pa.tail_act = (CHUB_G(float)) pb.tail_act_a;
    hipLaunchKernelGGL((k_slot_packed<kPackedBlock, kSlotsPerLane, false, false, false, false>), dim3(nb), dim3(kPackedBlock), 0, stream, ctx, sa, pa);
    PackedArgs pa2 = make_packed_args(hp, sb, pp);
    pa2.pk = (CHUB_G(const uint32_t)) (const void *) pb.pkraw;
    pa2.rec_prev = (CHUB_G(const uint32_t)) pb.rec_a;
    hipLaunchKernelGGL((k_slot_packed<kPackedBlock, kSlotsPerLane, false, false, false, false, false, true>), dim3(nb), dim3(kPackedBlock), 0, stream, ctx,
                       sb, pa2);
    TailArgs ta = make_tail_args(*pp.ev, *pp.st, hp, sa, pp, false), tb2 = make_tail_args(*pp.ev, *pp.st, hp, sb, pp, false);
    ta.rec = (CHUB_G(uint32_t)) pb.rec_a;
    ta.tail_act = (CHUB_G(const float)) pb.tail_act_a;
    ta.drw = pr.drw_in[0];
    ta.drw_cnt = pr.cnt_in[0];
    tb2.drw = pr.drw_in[1];
    tb2.drw_cnt = pr.cnt_in[1];
    if (more) hipLaunchKernelGGL(k_env_pair<true>, dim3((unsigned) nb_env + nb_lev), dim3(kEnvBlock), 0, stream, ctx, sa, sb, ta, tb2, pr, nb_env);
    else hipLaunchKernelGGL(k_env_pair<false>, dim3((unsigned) nb_env + nb_lev), dim3(kEnvBlock), 0, stream, ctx, sa, sb, ta, tb2, pr, nb_env);
}

__global__ void k_tick_advance(uint32_t *tick_base, uint32_t by) { *tick_base += by; }


// chub_step_bits: the pile decisions arrive as one bit per pile (what action_to_real makes of the action row, MGR:384-393) and
// the two tail actions as floats; this writes the [N, S + 2] f32 action rows the step kernels read: +1 / -1 for the piles (any
// value on the same side of the threshold gives the same step), the tail as it is
__global__ void k_expand_bits(int64_t n_envs, int S, int W, const uint64_t *__restrict__ bits, const float *__restrict__ tail,
                              float *__restrict__ actions) {
    const uint32_t A = (uint32_t) S + 2u;
    const uint32_t total = (uint32_t) n_envs * A;  // n_envs * (piles + 2) < 2^31 (checked at create)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const uint32_t env = i / A;
        const uint32_t j = i - env * A;
        float v;
        if (j < (uint32_t) S) v = ((bits[(size_t) env * (size_t) W + (j >> 6)] >> (j & 63u)) & 1ull) ? 1.0f : -1.0f;
        else v = tail[env * 2u + (j - (uint32_t) S)];
        actions[i] = v;
    }
}
void launch_expand_bits(const HubParams &hp, const uint64_t *d_bits, const float *d_tail, float *d_actions, hipStream_t stream) {
    const int S = hp.S[0] + hp.S[1];
    const int64_t total = hp.n_envs * (int64_t) (S + 2);
    int64_t nb = (total + 255) / 256;
    if (nb > 16384) nb = 16384;
    hipLaunchKernelGGL(k_expand_bits, dim3((unsigned) nb), dim3(256), 0, stream, hp.n_envs, S, (S + 63) / 64, d_bits, d_tail, d_actions);
}

// entering per-env clocks: every env starts from the handle's lock-step clock
__global__ void k_fill_clocks(uint16_t *dst, int64_t n, uint16_t value) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = value;
}
void launch_fill_clocks(uint16_t *dst, int64_t n, uint16_t value, hipStream_t stream) {
    hipLaunchKernelGGL(k_fill_clocks, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, stream, dst, n, value);
}
void launch_keep_clocks(uint16_t *dst, const uint16_t *src, int64_t n, hipStream_t stream) {
    hipLaunchKernelGGL(k_keep_clocks, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, stream, dst, src, n);
}
void launch_tick_advance(uint32_t *tick_base, uint32_t by, hipStream_t stream) {
    hipLaunchKernelGGL(k_tick_advance, dim3(1), dim3(1), 0, stream, tick_base, by);
}

// ---- chub_copy_envs: env d of one handle becomes a clone of env s of another (or the same) handle, by index, on the device
// One wave per (s, d) pair, four pairs per workgroup.  What moves is the env's simulation state and nothing else: its slot rows, both
// station records, the tank, OU and forecourt words, its days and clock, the committed COMPAT streams, its electrolyser table and (handles
// with per-env hub parameters) its row.  What a launch made AHEAD of the next step from the old state -- pk, and the COMPAT walk's shadow
// streams, var, fa, empt*, shrt, hv_pre -- is not touched: the host marks it void (chub_runtime.cpp: copy_launch) and the next launch
// makes its own, as after a masked call.  drw / drw_cnt (state-independent, keyed by the destination's own counters) stay as they are.
//
// The bulk is the slot rows (4 .. 16 bytes per slot): a row is contiguous per env (hub-major layouts) or per env and station (COMPAT),
// so the wave's lanes take consecutive 16-byte pieces of it where both ends are 16-byte aligned (COMPAT's records always are, hub-major
// rows whenever 4 S is a multiple of 16), consecutive words otherwise: one fully coalesced request per 1 KiB / 256 bytes either way.
// The ~30 scalars go one per lane.
__device__ __forceinline__ void copy_span(CHUB_G(uint8_t) d, CHUB_G(const uint8_t) s, uint32_t n, uint32_t lane) {
    const uint32_t al = (uint32_t) (uintptr_t) d | (uint32_t) (uintptr_t) s;
    uint32_t done = 0u;
    if ((al & 15u) == 0u) {
        const uint32_t nv = n >> 4;
        for (uint32_t i = lane; i < nv; i += 64u) ((CHUB_G(u32x4)) d)[i] = ((CHUB_G(const u32x4)) s)[i];
        done = nv << 4;
    }
    if ((al & 3u) == 0u) {
        const uint32_t nw = (n - done) >> 2;
        for (uint32_t i = lane; i < nw; i += 64u) ((CHUB_G(uint32_t)) (d + done))[i] = ((CHUB_G(const uint32_t)) (s + done))[i];
        done += nw << 2;
    }
    for (uint32_t i = done + lane; i < n; i += 64u) d[i] = s[i];
}
template <typename T>
__device__ __forceinline__ void copy_rows(CHUB_G(T) d, int64_t d_off, CHUB_G(const T) s, int64_t s_off, uint32_t count, uint32_t lane) {
    copy_span((CHUB_G(uint8_t)) (d + d_off), (CHUB_G(const uint8_t)) (s + s_off), count * (uint32_t) sizeof(T), lane);
}

template <int LAYOUT>
__global__ __launch_bounds__(256) void k_copy_envs(CopyArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t pair = (int64_t) blockIdx.x * 4 + (int64_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    if (pair >= a.count) return;
    const int64_t s = a.src_idx[pair], d = a.dst_idx[pair];
    const HubParams &hs = a.src->hp;
    const HubParams &hd = a.dst->hp;
    const int64_t Ns = hs.n_envs, Nd = hd.n_envs;
    if (s < 0 || s >= Ns || d < 0 || d >= Nd) return;
    const EnvArrays &es = a.src->ev;
    const EnvArrays &ed = a.dst->ev;
    // (the device form cannot refuse: a waiting list longer than the destination handle's rows can hold leaves the pair alone)
    const uint32_t qcap = (uint32_t) (hs.qcap < hd.qcap ? hs.qcap : hd.qcap);
    if ((uint32_t) es.q_len[s] > qcap) return;
    const uint32_t S0 = (uint32_t) hd.S[0], S1 = (uint32_t) hd.S[1], S = S0 + S1;  // (the same in both handles)

    // ---- slot rows
    if (LAYOUT == LAYOUT_COMPAT) {
        copy_rows<uint32_t>(a.dst->sl.hot, 4 * (hd.base[0] + d * (int64_t) S0), a.src->sl.hot, 4 * (hs.base[0] + s * (int64_t) S0), 4u * S0, lane);
        copy_rows<uint32_t>(a.dst->sl.hot, 4 * (hd.base[1] + d * (int64_t) S1), a.src->sl.hot, 4 * (hs.base[1] + s * (int64_t) S1), 4u * S1, lane);
    } else if (LAYOUT == LAYOUT_CURVES) {
        copy_rows<uint32_t>(a.dst->sl.hot, 2 * d * (int64_t) S, a.src->sl.hot, 2 * s * (int64_t) S, 2u * S, lane);
        copy_rows<uint32_t>(a.dst->sl.wrd, d * (int64_t) S, a.src->sl.wrd, s * (int64_t) S, S, lane);
        copy_rows<float>(a.dst->sl.soc0, d * (int64_t) S, a.src->sl.soc0, s * (int64_t) S, S, lane);
        copy_rows<uint8_t>(a.dst->sl.stay8, d * (int64_t) S, a.src->sl.stay8, s * (int64_t) S, S, lane);
    } else {
        copy_rows<uint32_t>(a.dst->sl.hot, d * (int64_t) S, a.src->sl.hot, s * (int64_t) S, S, lane);
        copy_rows<uint8_t>(a.dst->sl.stay8, d * (int64_t) S, a.src->sl.stay8, s * (int64_t) S, S, lane);
    }

    // ---- the forecourt list, the electrolyser table, the committed streams
    copy_rows<double>(ed.q_time, d * (int64_t) hd.qcap, es.q_time, s * (int64_t) hs.qcap, qcap, lane);
    copy_rows<double>(ed.q_mass, d * (int64_t) hd.qcap, es.q_mass, s * (int64_t) hs.qcap, qcap, lane);
    if (es.hy_env && ed.hy_env) copy_rows<double>(ed.hy_env, d * 102, es.hy_env, s * 102, 102u, lane);
    if (LAYOUT == LAYOUT_COMPAT) copy_rows<uint32_t>(a.dst->cr.g3[a.dst_rng], d * 32, a.src->cr.g3[a.src_rng], s * 32, 32u, lane);

    // ---- the scalars, one per lane
    const bool rows = a.src->ep.prm && a.dst->ep.prm && a.src_rows && a.dst_rows;
    const bool ledger = a.src->es.on && a.dst->es.on;
    static_assert(kEpCount == 7 && PRM_COUNT <= 10, "k_copy_envs: lanes 18-24 / 25-31 take the ledger's columns, 32-41 the parameter row");
    switch (lane) {
    case 0: ed.cap[d] = es.cap[s]; break;
    case 1: ed.store_soc[d] = es.store_soc[s]; break;
    case 2: case 3: case 4: ed.ou[(int64_t) (lane - 2u) * Nd + d] = es.ou[(int64_t) (lane - 2u) * Ns + s]; break;
    case 5: ed.price_noise[d] = es.price_noise[s]; break;
    case 6: ed.pv_day[d] = es.pv_day[s]; break;
    case 7: ed.wd_day[d] = es.wd_day[s]; break;
    case 8: ed.q_len[d] = es.q_len[s]; break;
    case 9: ed.hv_line[d] = es.hv_line[s]; break;
    case 10: case 11: ed.q_fold[2 * d + (int64_t) (lane - 10u)] = es.q_fold[2 * s + (int64_t) (lane - 10u)]; break;
    case 12: ed.q_fold_cnt[d] = es.q_fold_cnt[s]; break;
    case 13: if (a.dst_clk) a.dst_clk[d] = a.src_clk ? a.src_clk[s] : (uint16_t) a.src_clk_value; break;
    case 14: case 15: {  // the station records, 16 bytes each (unit u = k N + env)
        const int64_t k = (int64_t) (lane - 14u);
        ((CHUB_G(u32x4)) a.dst->st.rec)[k * Nd + d] = ((CHUB_G(const u32x4)) a.src->st.rec)[k * Ns + s];
        break;
    }
    case 16: if (LAYOUT == LAYOUT_COMPAT) a.dst->cr.minstd3[a.dst_rng][d] = a.src->cr.minstd3[a.src_rng][s]; break;
    case 17: if (rows) ((CHUB_G(float)) a.dst->ep.hv_rate)[d] = a.src->ep.hv_rate[s]; break;
    case 18: case 19: case 20: case 21: case 22: case 23: case 24:  // the episode ledger (the host has checked: on in both handles or in neither)
        if (ledger) a.dst->es.live[(int64_t) (lane - 18u) * Nd + d] = a.src->es.live[(int64_t) (lane - 18u) * Ns + s];
        break;
    case 25: case 26: case 27: case 28: case 29: case 30: case 31:
        if (ledger) a.dst->es.fin[(int64_t) (lane - 25u) * Nd + d] = a.src->es.fin[(int64_t) (lane - 25u) * Ns + s];
        break;
    case 42: if (ledger) a.dst->es.episodes[d] = a.src->es.episodes[s]; break;
    case 43: if (ledger) a.dst->es.pending[d] = a.src->es.pending[s]; break;
    default:
        if (rows && lane >= 32u && lane < 32u + (uint32_t) PRM_COUNT)
            ((CHUB_G(double)) a.dst->ep.prm)[(int64_t) (lane - 32u) * Nd + d] = a.src->ep.prm[(int64_t) (lane - 32u) * Ns + s];
        else if (rows && lane >= 48u && lane < 56u)
            a.dst_rows[8 * d + (int64_t) (lane - 48u)] = a.src_rows[8 * s + (int64_t) (lane - 48u)];
        break;
    }
}

void launch_copy_envs(int layout, const CopyArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned) ((a.count + 3) / 4)), block(256);
    switch (layout) {
    case LAYOUT_COMPAT: hipLaunchKernelGGL(k_copy_envs<LAYOUT_COMPAT>, grid, block, 0, stream, a); break;
    case LAYOUT_CURVES: hipLaunchKernelGGL(k_copy_envs<LAYOUT_CURVES>, grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL(k_copy_envs<LAYOUT_PHILOX>, grid, block, 0, stream, a); break;
    }
}

// ---- chub_episode_summary: the finished episodes nobody has looked at yet, reduced on the device
// k_episode_summary walks the envs (lane i of the grid takes envs i, i + lanes, ...: a fixed assignment), and for the envs whose pending flag is
// set adds up the count and per column of the finished block the sum, the sum of squares, min and max; a wave combines its lanes with __shfl_down,
// the workgroup its waves through LDS in wave order, and the workgroup's kEpSumWords partials go to the handle's buffer.
// k_episode_summary_combine (one wave, a launch of its own behind it: a kernel boundary is the one hand-off between workgroups that needs no
// fence) takes one partial per lane and combines them with the same tree.  No atomics anywhere and every order fixed: two calls on one state give the same bits.
__device__ __forceinline__ void ep_sum_merge(double &cnt, double *v, double o_cnt, const double *o) {
    cnt += o_cnt;
#pragma unroll
    for (int c = 0; c < kEpCount; c++) {
        v[4 * c] += o[4 * c];
        v[4 * c + 1] += o[4 * c + 1];
        v[4 * c + 2] = o[4 * c + 2] < v[4 * c + 2] ? o[4 * c + 2] : v[4 * c + 2];
        v[4 * c + 3] = o[4 * c + 3] > v[4 * c + 3] ? o[4 * c + 3] : v[4 * c + 3];
    }
}
// lane l takes lane l + off, off = 32 .. 1: a fixed tree, after which lane 0 holds the wave's values
__device__ __forceinline__ void ep_sum_wave(double &cnt, double *v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        double o[4 * kEpCount];
        const double o_cnt = __shfl_down(cnt, off);
#pragma unroll
        for (int j = 0; j < 4 * kEpCount; j++) o[j] = __shfl_down(v[j], off);
        ep_sum_merge(cnt, v, o_cnt, o);
    }
}
__global__ __launch_bounds__(kEpSumBlock) void k_episode_summary(const DevCtx *__restrict__ ctx, double *__restrict__ partials, int drain) {
    __shared__ double s_part[kEpSumBlock / 64][kEpSumWords];
    const EpisodeArrays &es = ctx->es;
    const int64_t N = ctx->hp.n_envs;
    double cnt = 0.0, v[4 * kEpCount];
#pragma unroll
    for (int c = 0; c < kEpCount; c++) {
        v[4 * c] = 0.0;
        v[4 * c + 1] = 0.0;
        v[4 * c + 2] = __builtin_huge_val();
        v[4 * c + 3] = -__builtin_huge_val();
    }
    for (int64_t i = (int64_t) blockIdx.x * kEpSumBlock + threadIdx.x; i < N; i += (int64_t) gridDim.x * kEpSumBlock) {
        if (!es.pending[i]) continue;
        if (drain) es.pending[i] = 0;  // (the flag this lane has just read: nobody else looks at env i)
        double x[4 * kEpCount];
#pragma unroll
        for (int c = 0; c < kEpCount; c++) {
            const double f = es.fin[(int64_t) c * N + i];
            x[4 * c] = f;
            x[4 * c + 1] = f * f;
            x[4 * c + 2] = f;
            x[4 * c + 3] = f;
        }
        ep_sum_merge(cnt, v, 1.0, x);
    }
    ep_sum_wave(cnt, v);
    const int wave = (int) (threadIdx.x >> 6);
    if ((threadIdx.x & 63u) == 0u) {
        s_part[wave][0] = cnt;
#pragma unroll
        for (int j = 0; j < 4 * kEpCount; j++) s_part[wave][1 + j] = v[j];
    }
    __syncthreads();
    const int j = (int) threadIdx.x;
    if (j < kEpSumWords) {  // word j of the workgroup's partial: the waves in order
        const int kind = j == 0 ? 0 : (j - 1) & 3;
        double r = s_part[0][j];
        for (int w = 1; w < kEpSumBlock / 64; w++) {
            const double o = s_part[w][j];
            r = kind < 2 ? r + o : (kind == 2 ? (o < r ? o : r) : (o > r ? o : r));
        }
        partials[(size_t) blockIdx.x * kEpSumWords + j] = r;
    }
}
// one wave: lane b holds workgroup b's partial (the identity beyond the grid), all its words requested at once, then the same fixed tree
__global__ __launch_bounds__(64) void k_episode_summary_combine(const double *__restrict__ partials, int n_blocks, double *__restrict__ out) {
    static_assert(kEpSumMaxBlocks <= 64, "k_episode_summary_combine: one lane per partial");
    const int b = (int) threadIdx.x;
    double cnt = 0.0, v[4 * kEpCount];
#pragma unroll
    for (int c = 0; c < kEpCount; c++) {
        v[4 * c] = 0.0;
        v[4 * c + 1] = 0.0;
        v[4 * c + 2] = __builtin_huge_val();
        v[4 * c + 3] = -__builtin_huge_val();
    }
    if (b < n_blocks) {
        const double *p = partials + (size_t) b * kEpSumWords;
        cnt = p[0];
#pragma unroll
        for (int j = 0; j < 4 * kEpCount; j++) v[j] = p[1 + j];
    }
    ep_sum_wave(cnt, v);
    if (b == 0) {
        out[0] = cnt;
#pragma unroll
        for (int j = 0; j < 4 * kEpCount; j++) out[1 + j] = v[j];
    }
}
int episode_summary_blocks(int64_t n_envs) {
    const int64_t nb = (n_envs + kEpSumBlock - 1) / kEpSumBlock;
    return (int) (nb < 1 ? 1 : (nb > kEpSumMaxBlocks ? kEpSumMaxBlocks : nb));
}
void launch_episode_summary(const HubParams &hp, const DevCtx *ctx, double *d_partials, double *d_out, int drain, hipStream_t stream) {
    const int nb = episode_summary_blocks(hp.n_envs);
    hipLaunchKernelGGL(k_episode_summary, dim3((unsigned) nb), dim3(kEpSumBlock), 0, stream, ctx, d_partials, drain);
    hipLaunchKernelGGL(k_episode_summary_combine, dim3(1), dim3(64), 0, stream, (const double *) d_partials, nb, d_out);
}

// chub_create, COMPAT handles: every entry of Tables::ttab against the device's own soc_to_time(uniform_level(l, 80, 100)) -- the expression
// add_car evaluates (make_car's callers) -- bit for bit; *mismatch counts the entries that differ
__global__ void k_check_ttab(const DevCtx *__restrict__ ctx, uint32_t *mismatch) {
    const int i = (int) (blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= 2 * kLevels) return;
    const int k = i / kLevels, lev = i - k * kLevels;
    const bool cp = ctx->hp.constant_charging != 0;
    const float target = uniform_level(lev, 80.0f, 100.0f);
    const float t = ctx->hp.type[k] == 0 ? soc_to_time<0>(target, cp) : soc_to_time<1>(target, cp);
    if (__float_as_uint(t) != __float_as_uint(ctx->tb.ttab[k][lev])) atomicAdd(mismatch, 1u);
}
void launch_check_ttab(const DevCtx *ctx, uint32_t *d_mismatch, hipStream_t stream) {
    hipLaunchKernelGGL(k_check_ttab, dim3((2 * kLevels + 255) / 256), dim3(256), 0, stream, ctx, d_mismatch);
}

void launch_random_actions(const HubParams &hp, uint64_t key, uint32_t batch, float *d_actions, hipStream_t stream) {
    const int per = (hp.act_dim + 3) / 4;
    int64_t total = hp.n_envs * per;
    int64_t nb = (total + 255) / 256;
    if (nb > 8192) nb = 8192;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(k_random_actions, dim3((unsigned) nb), dim3(256), 0, stream, hp.n_envs, hp.env_id0, hp.act_dim,
                       (uint32_t) key, (uint32_t) (key >> 32), batch, d_actions);
}

}  // namespace chub
