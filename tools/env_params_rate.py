#!/usr/bin/env python3
"""Homogeneous handles against handles with per-env hub parameters (chub_create_params) in one process, on the same device-resident step path
(chub_reset_device / chub_step_device, call by call): env-steps/s and us per step.  Per mode three handles: homogeneous; rows that all equal
the homogeneous config ("rows_same": the cost of the ENV_PARAMS tail alone, same work); rows cycling through seven different configs
("rows_mixed": the issue's domain-randomisation set, which also changes the work -- a stuck forecourt, empty tanks).  Each handle is warmed up
(one whole day), then the handles alternate, one timed day each, ROUNDS times; the best day of each is reported.
    python tools/env_params_rate.py [--shapes 65536x20,25] [--modes philox philox_curves compat] [--rounds 3] [--out profiles/env_params_rate.json]
COMPAT handles with rows run one kernel per station (include/chub.h), so COMPAT also reports the homogeneous handle on that form
("homogeneous_stations", chub_options.slot_kernel = 1) beside its default (the split step with the walks ahead)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import charginghub_env_amd as chub
from charginghub_env_amd import multi_gpu

BASE = dict(hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2, fc_max_power=100.0, fcev_permeate=0.01, renew_fluctuate=0.0,
            price_fluctuate=0.0, hydro_loss=0.0)
MIXED = [dict(), dict(hydro_prod_rate=0.0), dict(hydro_store_vlt=5.0, init_soc=0.1), dict(hydro_store_vlt=5.0, init_soc=1.0),
         dict(fcev_permeate=1.5), dict(fcev_permeate=0.1, hydro_store_vlt=400.0), dict(renew_fluctuate=0.3, price_fluctuate=0.3, hydro_loss=0.02)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["65536x20,25"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", nargs="+", default=["philox", "philox_curves", "compat"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    for shape in args.shapes:
        n_s, piles_s = shape.split("x")
        n, piles = int(n_s), [int(x) for x in piles_s.split(",")]
        hub = dict(station_list=piles, station_type_list=["fast", "slow"])
        st = multi_gpu.Stream(0)
        for mode in args.modes:
            runs = {}
            compat = mode == "compat"
            kinds = ("homogeneous", "homogeneous_stations", "rows_same", "rows_mixed") if compat else ("homogeneous", "rows_same", "rows_mixed")
            rs = np.random.RandomState(1)
            z = multi_gpu.DeviceBuffer(n * 3 * 8)
            z.from_host(rs.normal(size=(n, 3)), st.ptr)
            days = multi_gpu.DeviceBuffer(n * 2 * 4)
            days.from_host(np.stack([rs.randint(0, 100, n), rs.randint(0, 150, n)], axis=1).astype(np.int32), st.ptr)
            for kind in kinds:
                if kind.startswith("homogeneous"):
                    kw = dict(BASE, slot_kernel="wave") if kind == "homogeneous_stations" else dict(BASE)
                elif kind == "rows_same":
                    kw = {f: [v] * n for f, v in BASE.items()}
                else:
                    kw = {f: [MIXED[i % len(MIXED)].get(f, BASE[f]) for i in range(n)] for f in BASE}
                t0 = time.perf_counter()
                v = chub.VecChargingHub(n, seed=1, rng=mode, **hub, **kw)
                create_s = time.perf_counter() - t0
                D, A = v.obs_dim, v.act_dim
                acts = [multi_gpu.DeviceBuffer(n * A * 4) for _ in range(2)]
                for b, a in enumerate(acts):
                    v.random_actions_device(a.ptr, 123, b, st.ptr)
                obs, rew, done = multi_gpu.DeviceBuffer(n * D * 4), multi_gpu.DeviceBuffer(n * 4), multi_gpu.DeviceBuffer(n)
                runs[kind] = dict(v=v, bufs=(acts, obs, rew, done), best=None, create_s=create_s)

            def day(r):
                v = r["v"]
                acts, obs, rew, done = r["bufs"]
                v.reset_device(obs.ptr, days.ptr if compat else 0, z.ptr if compat else 0, stream=st.ptr)
                st.sync()
                t0 = time.perf_counter()
                for t in range(96):
                    v.step_device(acts[t & 1].ptr, obs.ptr, rew.ptr, done.ptr, d_exo_z=z.ptr if compat else 0, stream=st.ptr)
                st.sync()
                return time.perf_counter() - t0

            for r in runs.values():  # warm-up: one whole day each
                day(r)
            for _ in range(args.rounds):
                for r in runs.values():
                    dt = day(r)
                    r["best"] = dt if r["best"] is None else min(r["best"], dt)
            # host cost of rows that are all different: chub_set_env_params builds one electrolyser table per distinct row
            r = runs["rows_mixed"]
            t0 = time.perf_counter()
            r["v"].set_env_params(init_soc=np.linspace(0.1, 1.0, n))
            r["set_distinct_s"] = time.perf_counter() - t0
            base_us = runs["homogeneous"]["best"] / 96 * 1e6
            for kind, r in runs.items():
                us = r["best"] / 96 * 1e6
                row = dict(shape=shape, n_envs=n, piles=piles, mode=mode, handle=kind, us_per_step=round(us, 2), env_steps_per_s=round(n / us * 1e6),
                           vs_homogeneous=round(us / base_us, 4), create_s=round(r["create_s"], 3),
                           set_distinct_rows_s=round(r["set_distinct_s"], 3) if "set_distinct_s" in r else None,
                           fused_step=r["v"].uses_fused_step, build_id=chub.load_library().chub_build_id().decode())
                rows.append(row)
                print(json.dumps(row), flush=True)
                r["v"].close()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
