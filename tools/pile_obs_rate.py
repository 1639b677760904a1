#!/usr/bin/env python3
"""chub_pile_obs_device on a device-resident handle: us per call for the three RNG modes and three field sets, beside the HBM floor of the
call's algorithmic bytes (state bytes read per pile in that mode and field set + 4 C bytes written, at the 6.3 TB/s a streaming kernel
reaches on an MI355X).  Each handle is reset and stepped 30 times first (piles occupied as in a run); every (mode, field set) is warmed up,
then they alternate, CALLS calls between two stream synchronisations each, ROUNDS times; the best round is reported.
    python tools/pile_obs_rate.py [--shapes 65536x20,25 262144x32,32] [--rounds 5] [--calls 50] [--out profiles/pile_obs_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import charginghub_env_amd as chub
from charginghub_env_amd import _lib, multi_gpu

FIELD_SETS = {"all": _lib.PILE_NAMES, "car_emergency_soc": ("car", "emergency", "soc"), "car_emergency": ("car", "emergency")}
HBM_BYTES_PER_US = 6.3e6  # 6.3 TB/s: what a streaming kernel reaches (8 TB/s is the part's specification)


def state_bytes(mode, names):
    """slot-state bytes a call reads per pile (the class rows, the target times and the SoC table are tables of a few hundred KB that stay
    in the caches: not counted)"""
    names = set(names)
    row = bool(names & {"emergency", "power"})
    counters = bool(names & {"stay_time", "already_stay_time"})
    if mode == "compat":  # the 16-byte record, or its fourth word alone
        return 16 if row or names & {"soc", "init_soc"} else 4
    b = 4 + (1 if counters else 0)  # the state word, stay8
    if mode == "philox_curves":
        b += (8 if row else 0) + (4 if names & {"soc", "init_soc"} else 0)  # (power, t_soc), the arrival SoC
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["65536x20,25", "262144x32,32"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--modes", nargs="+", default=["philox", "philox_curves", "compat"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    for shape in args.shapes:
        n_s, piles_s = shape.split("x")
        n, piles = int(n_s), [int(x) for x in piles_s.split(",")]
        S = sum(piles)
        kw = dict(station_list=piles, station_type_list=["fast", "slow"], hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2,
                  fc_max_power=100.0, fcev_permeate=0.01)
        st = multi_gpu.Stream(0)
        out = multi_gpu.DeviceBuffer(n * _lib.PILE_COUNT * S * 4)
        runs = {}
        rs = np.random.RandomState(1)
        for mode in args.modes:
            v = chub.VecChargingHub(n, seed=1, rng=mode, **kw)
            D, A = v.obs_dim, v.act_dim
            acts = [multi_gpu.DeviceBuffer(n * A * 4) for _ in range(2)]
            for b, a in enumerate(acts):
                v.random_actions_device(a.ptr, 123, b, st.ptr)
            obs, rew, done = multi_gpu.DeviceBuffer(n * D * 4), multi_gpu.DeviceBuffer(n * 4), multi_gpu.DeviceBuffer(n)
            compat = mode == "compat"  # (its exogenous variates come from the caller)
            z, days = multi_gpu.DeviceBuffer(n * 3 * 8), multi_gpu.DeviceBuffer(n * 2 * 4)
            z.from_host(rs.normal(size=(n, 3)), st.ptr)
            days.from_host(np.stack([rs.randint(0, 100, n), rs.randint(0, 150, n)], axis=1).astype(np.int32), st.ptr)
            v.reset_device(obs.ptr, days.ptr if compat else 0, z.ptr if compat else 0, stream=st.ptr)
            for t in range(30):
                v.step_device(acts[t & 1].ptr, obs.ptr, rew.ptr, done.ptr, d_exo_z=z.ptr if compat else 0, stream=st.ptr)
            st.sync()
            for b in acts + [obs, rew, done, z, days]:
                b.free()
            runs[mode] = v
        best = {}

        def batch(mode, fs):
            mask = _lib.pile_fields_mask(FIELD_SETS[fs])
            st.sync()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                runs[mode].pile_obs_device(out.ptr, mask, stream=st.ptr)
            st.sync()
            return (time.perf_counter() - t0) / args.calls * 1e6

        cases = [(mode, fs) for mode in args.modes for fs in FIELD_SETS]
        for c in cases:  # warm-up
            batch(*c)
        for _ in range(args.rounds):
            for c in cases:
                us = batch(*c)
                best[c] = min(best.get(c, us), us)
        for mode, fs in cases:
            names = FIELD_SETS[fs]
            per_pile = state_bytes(mode, names) + 4 * len(names)
            floor = n * S * per_pile / HBM_BYTES_PER_US
            row = dict(shape=shape, n_envs=n, piles=piles, mode=mode, fields=fs, columns=len(names), us_per_call=round(best[(mode, fs)], 2),
                       bytes_per_pile=per_pile, hbm_floor_us=round(floor, 2), build_id=chub.load_library().chub_build_id().decode())
            rows.append(row)
            print(json.dumps(row), flush=True)
        for v in runs.values():
            v.close()
        out.free()
        st.destroy()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
