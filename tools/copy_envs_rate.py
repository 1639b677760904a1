#!/usr/bin/env python3
"""chub_copy_envs_device against the route the snapshot API offers for the same job, in one process.  Per mode one handle is reset and stepped
into the day; then a device-form copy of 1 %, 10 % and 100 % of the envs (the sources come from a twin handle of the same size, so a 100 %
copy has distinct destinations) is timed by HIP events on the launch stream (torch.cuda.Event), with warm-up, best of ROUNDS; reported with
the state bytes it moves (read + written) and the bandwidth that implies, beside one lock-step step of that handle (same events) and
chub_get_state + chub_set_state of the whole handle (host clock: it is a host round trip).  The step that follows a copy makes its own
station draws (k_draw_levels in front): its time is reported too ("step_after_copy_us"), and so is a later step of the handle, which the
device form has left on per-env clocks ("step_per_env_clocks_us", against "step_us" in lock-step).
    python tools/copy_envs_rate.py [--shape 65536x20,25] [--modes philox compat] [--rounds 3] [--out profiles/copy_envs_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import charginghub_env_amd as chub

HUB = dict(hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2, fc_max_power=100.0, fcev_permeate=0.01)


def state_bytes(v, compat):
    """bytes of one env's state as k_copy_envs moves it (chub_device.h), read once and written once"""
    S = v.n_slots
    slots = 16 * S if compat else (17 * S if v.rng_mode == 2 else 5 * S)
    scalars = 8 * 6 + 2 * 2 + 2 + 16 + 4 + 2 + 2 * 16  # tank, OU, noise; days; list head; folded list; clock; station records
    qcap = 1  # fcev_permeate 0.01: at most one arrival per step
    return 2 * (slots + scalars + 16 * qcap + (102 * 8 + 33 * 4 if compat else 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="65536x20,25")
    ap.add_argument("--modes", nargs="+", default=["philox", "compat"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n_s, piles_s = args.shape.split("x")
    n, piles = int(n_s), [int(x) for x in piles_s.split(",")]
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for mode in args.modes:
        compat = mode == "compat"
        vs = [chub.VecChargingHub(n, piles, ["fast", "slow"], seed=s, rng=mode, **HUB) for s in (1, 2)]
        v, twin = vs
        D, A = v.obs_dim, v.act_dim
        gen = torch.Generator(device="cuda").manual_seed(1)
        act = torch.rand((n, A), device="cuda", generator=gen) * 2 - 1
        z = torch.randn((n, 3), device="cuda", dtype=torch.float64, generator=gen)
        days = torch.stack([torch.randint(0, 100, (n,), device="cuda"), torch.randint(0, 150, (n,), device="cuda")], dim=1).to(torch.int32).contiguous()
        obs, rew, done = (torch.empty((n, D), device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, device="cuda", dtype=torch.uint8))
        zp, dp = (z.data_ptr(), days.data_ptr()) if compat else (0, 0)

        def step(h):
            h.step_device(act.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(), d_exo_z=zp, stream=stream)

        def timed(fn, reps=1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3 / reps  # us

        for h in vs:
            h.reset_device(obs.data_ptr(), dp, zp, stream=stream)
            for _ in range(20):
                step(h)
        torch.cuda.synchronize()
        step_us = min(timed(lambda: step(v), reps=10) for _ in range(args.rounds))
        per_env = state_bytes(v, compat)
        res = dict(shape=args.shape, n_envs=n, piles=piles, mode=mode, step_us=round(step_us, 2), state_bytes_per_env_rw=per_env,
                   build_id=chub.load_library().chub_build_id().decode())
        perm = torch.randperm(n, device="cuda", generator=gen)
        for pct in (1, 10, 100):
            k = max(1, n * pct // 100)
            src = torch.randint(0, n, (k,), device="cuda", generator=gen).to(torch.int64)
            dst = perm[:k].to(torch.int64).contiguous()
            copy = lambda: v.copy_envs_device(src.data_ptr(), dst.data_ptr(), k, source=twin, stream=stream)
            copy()  # warm-up (the first copy also moves the handle onto per-env clocks)
            torch.cuda.synchronize()
            us = min(timed(copy) for _ in range(args.rounds))
            res["copy_%d_pct" % pct] = dict(envs=k, us=round(us, 2), bytes=k * per_env, gb_per_s=round(k * per_env / us / 1e3, 1),
                                            vs_step=round(us / step_us, 3))
        # the device form leaves the handle on per-env clocks until everybody is reset: what a step costs there, and the first step behind
        # a copy (which also makes its own station draws, k_draw_levels in front)
        res["step_after_copy_us"] = round(min(timed(lambda: (copy(), step(v))) for _ in range(args.rounds)) - res["copy_100_pct"]["us"], 2)
        step(v)
        res["step_per_env_clocks_us"] = round(min(timed(lambda: step(v), reps=10) for _ in range(args.rounds)), 2)
        res["clock_groups_after"] = v.clock_groups
        torch.cuda.synchronize()
        best = None
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            blob = v.get_state()
            v.set_state(blob)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        res["get_state_set_state_us"] = round(best * 1e6, 1)
        res["snapshot_bytes"] = int(blob.size)
        rows.append(res)
        print(json.dumps(res), flush=True)
        for h in vs:
            h.close()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
