#!/usr/bin/env python3
"""The three RNG modes side by side in one process, on the same device-resident step path (chub_reset_device / chub_step_device, call by call):
env-steps/s, us per step and the slot state's bytes per slot and step.  Each shape is warmed up (one whole day per mode), then the modes
alternate, one timed day each, ROUNDS times; the best day of each mode is reported.
    python tools/soc_modes_rate.py [--shapes 65536x20,25 262144x32,32] [--rounds 3] [--out profiles/soc_modes_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import charginghub_env_amd as chub
from charginghub_env_amd import multi_gpu

# slot state read + written per slot and step: PHILOX the 4-byte word; PHILOX_CURVES 8-byte (power, t_soc) + the 4-byte word;
# COMPAT the 16-byte hot record
STATE_BYTES = {"philox": 8, "philox_curves": 24, "compat": 32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["65536x20,25", "262144x32,32"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", nargs="+", default=["philox", "philox_curves", "compat"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    for shape in args.shapes:
        n_s, piles_s = shape.split("x")
        n, piles = int(n_s), [int(x) for x in piles_s.split(",")]
        kw = dict(station_list=piles, station_type_list=["fast", "slow"], hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2,
                  fc_max_power=100.0, fcev_permeate=0.01)
        st = multi_gpu.Stream(0)
        rs = np.random.RandomState(1)
        runs = {}
        for mode in args.modes:
            v = chub.VecChargingHub(n, seed=1, rng=mode, **kw)
            D, A = v.obs_dim, v.act_dim
            acts = [multi_gpu.DeviceBuffer(n * A * 4) for _ in range(2)]
            for b, a in enumerate(acts):
                v.random_actions_device(a.ptr, 123, b, st.ptr)
            z = multi_gpu.DeviceBuffer(n * 3 * 8)
            z.from_host(rs.normal(size=(n, 3)), st.ptr)
            days = multi_gpu.DeviceBuffer(n * 2 * 4)
            days.from_host(np.stack([rs.randint(0, 100, n), rs.randint(0, 150, n)], axis=1).astype(np.int32), st.ptr)
            obs, rew, done = multi_gpu.DeviceBuffer(n * D * 4), multi_gpu.DeviceBuffer(n * 4), multi_gpu.DeviceBuffer(n)
            compat = mode == "compat"
            runs[mode] = dict(v=v, bufs=(acts, z, days, obs, rew, done), best=None, compat=compat)

        def day(r):
            v = r["v"]
            acts, z, days, obs, rew, done = r["bufs"]
            zp = z.ptr if r["compat"] else 0
            v.reset_device(obs.ptr, days.ptr if r["compat"] else 0, zp, stream=st.ptr)
            st.sync()
            t0 = time.perf_counter()
            for t in range(96):
                v.step_device(acts[t & 1].ptr, obs.ptr, rew.ptr, done.ptr, d_exo_z=zp, stream=st.ptr)
            st.sync()
            return time.perf_counter() - t0

        for mode in args.modes:  # warm-up: one whole day each
            day(runs[mode])
        for _ in range(args.rounds):
            for mode in args.modes:
                dt = day(runs[mode])
                r = runs[mode]
                r["best"] = dt if r["best"] is None else min(r["best"], dt)
        for mode in args.modes:
            r = runs[mode]
            us = r["best"] / 96 * 1e6
            row = dict(shape=shape, n_envs=n, piles=piles, mode=mode, us_per_step=round(us, 2), env_steps_per_s=round(n / us * 1e6),
                       state_bytes_per_slot_step=STATE_BYTES[mode], build_id=chub.load_library().chub_build_id().decode())
            rows.append(row)
            print(json.dumps(row), flush=True)
            r["v"].close()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
