#!/usr/bin/env python3
"""chub_forecast_device on a device-resident PHILOX handle: us per call for a few (fields, horizon) cases, each beside a hipMemsetAsync of
the same output size on the same stream -- the write-only yardstick -- and the per-env-row form of the handle.  Each
handle is reset and stepped 30 times first; every case is warmed up, then the cases alternate, CALLS calls between two device
synchronisations each, ROUNDS times; median, best and worst round are reported.
    python tools/forecast_rate.py [--shapes 65536x20,25] [--rounds 11] [--calls 1000] [--out profiles/forecast_rate.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # before libchub: both must share one HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import charginghub_env_amd as chub
from charginghub_env_amd import _lib, multi_gpu

CASES = [("all", None, 8, False), ("all", None, 96, False), ("price_pv_wind", ("price", "pv", "wind"), 8, False), ("all", None, 8, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["65536x20,25"])
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream().cuda_stream
    hip = ctypes.CDLL("libamdhip64.so")  # (the runtime torch and libchub have loaded)
    hip.hipMemsetAsync.restype = ctypes.c_int
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]

    def memset(t):
        rc = hip.hipMemsetAsync(t.data_ptr(), 0, t.numel() * 4, stream or None)
        assert rc == 0, rc
    rows = []
    for shape in args.shapes:
        n_s, piles_s = shape.split("x")
        n, piles = int(n_s), [int(x) for x in piles_s.split(",")]
        handles = {}
        for per_env_rows in (False, True):
            perm = list(np.linspace(0.01, 0.5, n)) if per_env_rows else 0.01
            v = chub.VecChargingHub(n, seed=1, rng="philox", station_list=piles, station_type_list=["fast", "slow"], hydro_prod_rate=100.0,
                                    hydro_store_vlt=25.0, init_soc=0.2, fc_max_power=100.0, fcev_permeate=perm)
            acts = [multi_gpu.DeviceBuffer(n * v.act_dim * 4) for _ in range(2)]
            for b, a in enumerate(acts):
                v.random_actions_device(a.ptr, 123, b, stream)
            packed = multi_gpu.DeviceBuffer(n * (v.obs_dim + 2) * 4)
            v.reset_device(packed.ptr, stream=stream)
            for t in range(30):
                v.step_device_packed(acts[t & 1].ptr, packed.ptr, stream=stream)
            torch.cuda.synchronize()
            handles[per_env_rows] = (v, acts + [packed])
        cases = {}
        for name, fields, H, per_env_rows in CASES:
            v = handles[per_env_rows][0]
            mask = _lib.fc_fields_mask(fields)
            out = torch.zeros((n, len(_lib.fc_fields_names(mask)), H), dtype=torch.float32, device="cuda")
            key = (name, H, per_env_rows)
            cases[key + ("forecast",)] = lambda v=v, out=out, mask=mask, H=H: v.forecast_device(out.data_ptr(), mask, H, stream=stream)
            cases[key + ("memset",)] = lambda out=out: memset(out)

        def batch(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.calls * 1e6

        for fn in cases.values():  # warm-up
            batch(fn)
        times = {c: [] for c in cases}
        for _ in range(args.rounds):
            for c, fn in cases.items():
                times[c].append(batch(fn))
        for (name, H, per_env_rows, route), ts in times.items():
            mask = _lib.fc_fields_mask(dict((c[0], c[1]) for c in CASES)[name])
            row = dict(shape=shape, n_envs=n, piles=piles, mode="philox", fields=name, horizon=H, per_env_rows=per_env_rows, route=route,
                       out_bytes=4 * n * len(_lib.fc_fields_names(mask)) * H, rounds=len(ts), calls_per_round=args.calls,
                       us_per_call_median=round(statistics.median(ts), 2), us_per_call_min=round(min(ts), 2), us_per_call_max=round(max(ts), 2),
                       build_id=chub.load_library().chub_build_id().decode())
            rows.append(row)
            print(json.dumps(row), flush=True)
        for v, bufs in handles.values():
            for b in bufs:
                b.free()
            v.close()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
