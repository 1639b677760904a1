#!/usr/bin/env python3
"""chub_station_profile_device on a device-resident PHILOX handle: us per call beside the only other route to the same numbers --
chub_pile_obs_device of the pile columns the fields need, alone and followed by a torch reduction of those columns into the same
[N, 2, C, B] histogram (float sums: the same quantities, not the same bits).  Each handle is reset and stepped 30 times first; every case is
warmed up, then the cases alternate, CALLS calls between two device synchronisations each, ROUNDS times; best and median round are reported.
    python tools/station_profile_rate.py [--shapes 65536x20,25 1024x300,270] [--rounds 7] [--calls 50] [--out profiles/station_profile_rate.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch  # before libchub: both must share one HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import charginghub_env_amd as chub
from charginghub_env_amd import _lib, multi_gpu

FIELD_SETS = {"counts": ("cars", "charging", "must_charge"), "all": _lib.SP_NAMES}
LEFT = ("stay_time", "already_stay_time")
NEEDS = {"cars": ("car",), "charging": ("car", "charge"), "must_charge": ("car", "emergency"), "power": ("car", "power"),
         "power_charging": ("car", "charge", "power"), "emergency": ("car", "emergency"), "soc_gap": ("car", "soc", "target_soc")}


def pile_columns(names):
    need = set(LEFT)
    for f in names:
        need |= set(NEEDS[f])
    return tuple(p for p in _lib.PILE_NAMES if p in need)


def torch_reduce(cols, pile_names, names, S0, B, out):
    """the [N, C', S] pile columns -> out [N, 2, C, B] by one scatter_add per call"""
    col = {p: cols[:, i] for i, p in enumerate(pile_names)}
    car = col["car"] == 1
    left = (col["stay_time"] - col["already_stay_time"]).clamp(max=B).long() - 1
    station = (torch.arange(cols.shape[2], device=cols.device) >= S0).long() * (B + 1)
    idx = torch.where(car, left, torch.full_like(left, B)) + station  # (piles without a car go to a spare bin per station)
    chg = car & (col["charge"] == 1) if "charge" in col else None
    vals = []
    for f in names:
        if f == "cars":
            vals.append(car.float())
        elif f == "charging":
            vals.append(chg.float())
        elif f == "must_charge":
            vals.append((car & (col["emergency"] == 10)).float())
        elif f == "power":
            vals.append(col["power"])
        elif f == "power_charging":
            vals.append(col["power"] * chg)
        elif f == "emergency":
            vals.append(col["emergency"])
        else:
            vals.append((col["target_soc"] - col["soc"]) * car)
    vals = torch.stack(vals, dim=1)
    bins = torch.zeros((cols.shape[0], len(names), 2 * (B + 1)), dtype=torch.float32, device=cols.device)
    bins.scatter_add_(2, idx[:, None, :].expand(-1, len(names), -1), vals)
    out.copy_(bins.view(cols.shape[0], len(names), 2, B + 1)[..., :B].transpose(1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["65536x20,25", "1024x300,270"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--buckets", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream().cuda_stream
    B = args.buckets
    rows = []
    for shape in args.shapes:
        n_s, piles_s = shape.split("x")
        n, piles = int(n_s), [int(x) for x in piles_s.split(",")]
        S = sum(piles)
        v = chub.VecChargingHub(n, seed=1, rng="philox", station_list=piles, station_type_list=["fast", "slow"], hydro_prod_rate=100.0,
                                hydro_store_vlt=25.0, init_soc=0.2, fc_max_power=100.0, fcev_permeate=0.01)
        acts = [multi_gpu.DeviceBuffer(n * v.act_dim * 4) for _ in range(2)]
        for b, a in enumerate(acts):
            v.random_actions_device(a.ptr, 123, b, stream)
        packed = multi_gpu.DeviceBuffer(n * (v.obs_dim + 2) * 4)
        v.reset_device(packed.ptr, stream=stream)
        for t in range(30):
            v.step_device_packed(acts[t & 1].ptr, packed.ptr, stream=stream)
        torch.cuda.synchronize()
        cases, bufs = {}, {}
        for fs, names in FIELD_SETS.items():
            pnames = pile_columns(names)
            prof = torch.zeros((n, 2, len(names), B), dtype=torch.float32, device="cuda")
            cols = torch.zeros((n, len(pnames), S), dtype=torch.float32, device="cuda")
            red = torch.zeros_like(prof)
            bufs[fs] = (prof, cols, red)
            smask, pmask = _lib.sp_fields_mask(names), _lib.pile_fields_mask(pnames)
            cases[(fs, "station_profile")] = lambda prof=prof, smask=smask: v.station_profile_device(prof.data_ptr(), smask, B, stream=stream)
            cases[(fs, "pile_obs")] = lambda cols=cols, pmask=pmask: v.pile_obs_device(cols.data_ptr(), pmask, stream=stream)

            def both(cols=cols, pmask=pmask, pnames=pnames, names=names, red=red):
                v.pile_obs_device(cols.data_ptr(), pmask, stream=stream)
                torch_reduce(cols, pnames, names, piles[0], B, red)
            cases[(fs, "pile_obs_and_torch_reduction")] = both

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
        for fs, names in FIELD_SETS.items():  # the two routes give the same numbers (the torch sums are float sums: a loose check)
            prof, cols, red = bufs[fs]
            torch.cuda.synchronize()
            worst = float((prof - red).abs().max())
            assert worst <= 1e-2 * max(1.0, float(prof.abs().max())), (fs, worst)
        for (fs, route), ts in times.items():
            row = dict(shape=shape, n_envs=n, piles=piles, mode="philox", fields=fs, buckets=B, route=route, pile_columns=len(pile_columns(FIELD_SETS[fs])),
                       us_per_call_best=round(min(ts), 2), us_per_call_median=round(statistics.median(ts), 2),
                       build_id=chub.load_library().chub_build_id().decode())
            rows.append(row)
            print(json.dumps(row), flush=True)
        for b in acts + [packed]:
            b.free()
        v.close()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
