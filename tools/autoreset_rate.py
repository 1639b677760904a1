#!/usr/bin/env python3
"""chub_autoreset_step_device against the route a trainer with staggered episodes had before it, in one process.  Per mode (--modes: PHILOX, PHILOX_CURVES)
one handle per leg, per-env clocks in GROUPS groups (masked head-start steps), timed by HIP events on the launch stream (torch.cuda.Event)
over one day (96 calls) per leg, after one warm-up day, the legs alternating, best of ROUNDS:
  (a) autoreset        chub_autoreset_step_device per call (two launches, the reset's workgroups returning at entry while nobody is done);
                       also split into the calls of the day in which a group finishes and those in which nobody does -- by call index:
                       group g starts its day g * (96 // GROUPS) slots ahead, so it finishes in call 95 - g * (96 // GROUPS) of every day
  (b) host_route       chub_step_device_packed + a device-to-host copy of `done` + a stream wait + chub_reset_envs_device with the host
                       mask on the steps where somebody finished (host clock around the day: it is a host round trip per step)
  (c) step_per_env     the step of everybody on per-env clocks alone (no reset: the clocks simply wrap)
  (d) step_lock_step   the lock-step step of a twin handle
    python tools/autoreset_rate.py [--shape 65536x20,25] [--groups 8] [--rounds 3] [--modes philox philox_curves] [--out profiles/autoreset_rate.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="65536x20,25")
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", nargs="+", default=["philox"], choices=["philox", "philox_curves"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n_s, piles_s = args.shape.split("x")
    n, piles, G = int(n_s), [int(x) for x in piles_s.split(",")], args.groups
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream().cuda_stream
    lib = chub.load_library()

    rows = []
    for mode in args.modes:
        def handle(seed):
            return chub.VecChargingHub(n, piles, ["fast", "slow"], seed=seed, rng=mode, **HUB)

        va, vb, vc, vd = handle(1), handle(1), handle(1), handle(1)
        D, A = va.obs_dim, va.act_dim
        gen = torch.Generator(device="cuda").manual_seed(1)
        act = torch.rand((n, A), device="cuda", generator=gen) * 2 - 1
        packed = torch.empty((n, D + 2), device="cuda")
        final = torch.empty((n, D), device="cuda")
        obs = torch.empty((n, D), device="cuda")
        rew, done = torch.empty(n, device="cuda"), torch.empty(n, device="cuda", dtype=torch.uint8)
        grp = (torch.arange(n, device="cuda") * G // n)
        apart = 96 // G
        mask = torch.empty(n, device="cuda", dtype=torch.uint8)
        host_done = torch.empty(n, dtype=torch.float32).pin_memory()

        for v in (va, vb, vc):  # the same staggered start for the three per-env-clock legs
            v.reset_device(obs.data_ptr(), stream=stream)
            for k in range(1, (G - 1) * apart + 1):
                mask.copy_((grp * apart >= k).to(torch.uint8))
                v.step_envs_dmask_device(mask.data_ptr(), act.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(), stream=stream)
        vd.reset_device(obs.data_ptr(), stream=stream)
        torch.cuda.synchronize()

        def call_a():
            va.step_autoreset_device(act.data_ptr(), packed.data_ptr(), final.data_ptr(), stream=stream)

        def call_b():
            vb.step_device_packed(act.data_ptr(), packed.data_ptr(), stream=stream)
            host_done.copy_(packed[:, D + 1], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            m = (host_done.numpy() > 0.5).astype(np.uint8)
            if m.any():
                chub._lib.check(lib.chub_reset_envs_device(vb._h, m.ctypes.data, None, None, obs.data_ptr(), stream))

        def call_c():
            vc.step_device_packed(act.data_ptr(), packed.data_ptr(), stream=stream)

        def call_d():
            vd.step_device_packed(act.data_ptr(), packed.data_ptr(), stream=stream)

        def day_events(fn):
            """one day, an event pair per call -> us per call, [96]"""
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(97)]
            ev[0].record()
            for i in range(96):
                fn()
                ev[i + 1].record()
            ev[96].synchronize()
            return np.array([ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(96)])

        def day_host(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(96):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / 96

        legs = dict(autoreset=call_a, host_route=call_b, step_per_env=call_c, step_lock_step=call_d)
        for fn in legs.values():  # one warm-up day each
            for i in range(96):
                fn()
        torch.cuda.synchronize()
        best = {}
        split = None
        for r in range(args.rounds):  # alternating legs
            for name, fn in legs.items():
                if name == "host_route":
                    us = day_host(fn)
                else:
                    per_call = day_events(fn)
                    us = float(per_call.mean())
                    if name == "autoreset":
                        busy = np.zeros(96, dtype=bool)
                        busy[[95 - g * apart for g in range(G)]] = True  # the calls in which a group's clock reaches the day's end
                        cur = dict(nobody_done_us=float(per_call[~busy].mean()), somebody_done_us=float(per_call[busy].mean()))
                        if split is None or cur["nobody_done_us"] < split["nobody_done_us"]:
                            split = cur
                best[name] = us if name not in best else min(best[name], us)
        res = dict(mode=mode, shape=args.shape, n_envs=n, piles=piles, groups=G, build_id=lib.chub_build_id().decode(),
                   autoreset_us=round(best["autoreset"], 2), host_route_us=round(best["host_route"], 2),
                   step_per_env_us=round(best["step_per_env"], 2), step_lock_step_us=round(best["step_lock_step"], 2),
                   autoreset_nobody_done_us=round(split["nobody_done_us"], 2), autoreset_somebody_done_us=round(split["somebody_done_us"], 2),
                   autoreset_minus_step_nobody_done_us=round(split["nobody_done_us"] - best["step_per_env"], 2),
                   clock_groups=va.clock_groups)
        print(json.dumps(res), flush=True)
        rows.append(res)
        for v in (va, vb, vc, vd):
            v.close()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
