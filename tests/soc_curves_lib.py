"""Shared pieces of the PHILOX_CURVES tests (tests/test_gpu_soc_curves.py): the reference fixtures replayed through the new slot kernel
in tape mode, and the host's f32 curve chain (chub_curves.h / the oracle) that a car's power and SoC must follow on the device."""
import numpy as np

import orclib
from orclib import orc

FAST, SLOW = 0, 1


def curve(typ, which, x, cp):
    """the oracle's f32 curves: which = 0 time_to_power, 1 time_to_soc, 2 soc_to_time"""
    f = orc.orc_curve_fast if typ == FAST else orc.orc_curve_slow
    return np.float32(f(which, float(x), int(cp)))


def arrive(typ, soc, cp):
    """add_car (CHS.hpp:864-877 / 1029-1042): (power, soc) of a car that has just arrived with this SoC"""
    return curve(typ, 0, curve(typ, 2, soc, cp), cp), np.float32(soc)


def car_step(typ, soc, cp):
    """car_step (CHS.hpp:900-905 / 1065-1070): soc -> soc_to_time -> + 1 slot -> time_to_soc / time_to_power, as build_class_row chains it"""
    tt = np.float32(curve(typ, 2, soc, cp) + np.float32(1.0))
    return curve(typ, 0, tt, cp), curve(typ, 1, tt, cp)


def philox_word(seed, tick, gid, site, index, block=0):
    """Philox4x32-10 block (block, site << 16 | index, tick, global env id) under key = seed: the counter layout of include/chub.h"""
    ctr = np.array([block, (site << 16) | index, tick, gid], dtype=np.uint32)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    out = np.zeros(4, dtype=np.uint32)
    orc.orc_philox4x32_10(orclib.ptr(ctr), orclib.ptr(key), orclib.ptr(out))
    return out


def replay_fixture(chub, name, n_envs=2):
    """every episode of a reference fixture through rng_mode PHILOX_CURVES in tape mode (resets included): the recorded arrival SoC of each
    new car goes straight into the car tape (.x = its f32 bits), no class is registered.  Per-slot state bit-exact, station counts exact,
    the power sums and everything downstream of them within test_gpu_tape's slack-derived bars, the other columns within 1e-9."""
    import test_gpu_tape as tt
    g = orclib.load_golden(name)
    piles = [int(x) for x in g["kw_station_list"]]
    types = [int(x) for x in g["kw_station_type"]]
    cp = bool(g["kw_constant_charging"])
    kw = dict(station_list=piles, station_type_list=["fast" if t == 0 else "slow" for t in types], constant_charging=cp,
              hydro_prod_rate=float(g["kw_hydro_prod_rate"]), hydro_store_vlt=float(g["kw_hydro_store_vlt"]),
              init_soc=float(g["kw_init_soc"]), fc_max_power=float(g["kw_fc_max_power"]),
              fcev_permeate=float(g["kw_fcev_permeate"]), renew_fluctuate=float(g["kw_renew_fluctuate"]),
              price_fluctuate=float(g["kw_price_fluctuate"]), hydro_loss=float(g["kw_hydro_loss"]))
    v = chub.VecChargingHub(n_envs, seed=1, rng="philox_curves", **kw)
    assert not v.uses_packed_kernel
    v.set_telemetry(True)
    v.set_hy_table(g["hy_table"])
    hv_w = 1 + g["hv_soc"].shape[1]
    S0, S1 = piles
    S = S0 + S1
    levels = tt._levels()
    rep = lambda a: np.repeat(np.asarray(a)[None], n_envs, axis=0)
    steps = int(g["steps_per_episode"])
    v.reset_tape(np.zeros((2, n_envs), dtype=np.uint32), np.zeros((n_envs, S, 2), dtype=np.uint32), rep(g["ctor_days"]), rep(g["ctor_z"]))

    def compare(cur, st, what):
        sl = v.slots()
        sc = v.station_scalars()
        for e in range(n_envs):
            for k in (0, 1):
                got, want = sl[k][e], cur[k]
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, what, k, got, want)
                ref = st[6 * k:6 * k + 6]
                assert np.array_equal(sc[e, k, 3:6], ref[3:6]), (name, what, k, sc[e, k], ref)
                tt._hold("station_sums", [3 * k, 3 * k + 1, 3 * k + 2], sc[e, k, :3], ref[:3], tt._slack(st, piles)[k], (name, what, e))

    def tape_car(typ, slots, s):
        lev, late = tt._new_car(typ, cp, slots[5, s], slots[6, s], slots[7, s], levels)
        return [np.float32(slots[5, s]).view(np.uint32), lev | (late << 16)]

    i = n_new = 0
    for ep in range(int(g["episodes"])):
        prev = [g["reset_slots0"][ep], g["reset_slots1"][ep]]
        rst = g["reset_stations"][ep]
        occ = np.zeros((2, n_envs), dtype=np.uint32)
        car = np.zeros((S, 2), dtype=np.uint32)
        for k, off in ((0, 0), (1, S0)):
            flow = int(rst[6 * k + 5])
            occ[k, :] = (flow & 0xFFFF) | (max(flow, 0) << 16)
            for s in np.nonzero(prev[k][0] > 0.5)[0]:
                car[off + s] = tape_car(types[k], prev[k], s)
                n_new += 1
        v.reset_tape(occ, rep(car), rep(g["reset_days"][ep]), rep(g["reset_z"][ep]))
        compare(prev, rst, ("reset", ep))
        o64 = v.obs_f64()
        D_ = o64.shape[1]
        cols = [0, 1, D_ - 3, D_ - 2, D_ - 1] + [c for c in range(2, D_ - 3) if (c - 2) % 4 == 3]
        for e in range(n_envs):
            assert np.allclose(o64[e, cols], g["reset_obs"][ep][cols], rtol=tt.TIGHT, atol=tt.TIGHT), (name, "reset obs", ep)
            sl_ = tt._slack(rst, piles)
            sc_ = v.station_scalars()
            for j, k in enumerate([k for k in (0, 1) if piles[k] > 0]):
                cs = [2 + 4 * j, 3 + 4 * j, 4 + 4 * j]
                tt._hold("reset_obs_station", cs, o64[e, cs], g["reset_obs"][ep][cs], sl_[k] / (float(sc_[e, k, 7]) / 2), (name, "reset obs", ep))
        line = [int(rst[4]), int(rst[10])]
        for t in range(steps):
            cur = [g["slots0"][i], g["slots1"][i]]
            st = g["stations"][i]
            pk = np.zeros((2, n_envs), dtype=np.uint64)
            car = np.zeros((S, 2), dtype=np.uint32)
            for k, off, n in ((0, 0, S0), (1, S0, S1)):
                line_after, flow = int(st[6 * k + 4]), int(st[6 * k + 5])
                word, new = tt._pk_word(n, prev[k], cur[k], line[k], line_after, flow)
                pk[k, :] = word
                for s in np.nonzero(new)[0]:
                    car[off + s] = tape_car(types[k], cur[k], s)
                    n_new += 1
                line[k] = line_after
            hv = np.zeros(hv_w, dtype=np.uint32)
            hv[0] = int(g["telem"][i][19])
            hv[1:1 + hv[0]] = g["hv_soc"][i][:hv[0]].view(np.uint32)
            _, _, done = v.step_tape(rep(g["action"][i]), pk, rep(car), rep(g["exo_z"][i]), rep(hv))[:3]
            compare(cur, st, (ep, t))
            assert all(bool(d) == bool(g["done"][i]) for d in done)
            tt._check_tail(v, g, i, name, n_envs, (ep, t), piles)
            prev = cur
            i += 1
    v.close()
    return n_new
