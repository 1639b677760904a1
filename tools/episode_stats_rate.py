#!/usr/bin/env python3
"""What the per-episode ledger (chub_set_episode_stats) costs, and what its summary call saves, in one process.  PHILOX, one handle per leg,
timed by HIP events on the launch stream (torch.cuda.Event) over one day (96 calls) per leg, after one warm-up day, the legs alternating,
best of ROUNDS:
  (a) lock_step_off / lock_step_on    chub_step_device_packed of everybody, ledger off / on
  (b) autoreset_off / autoreset_on    chub_autoreset_step_device on per-env clocks in GROUPS groups, ledger off / on
  (c) summary                         one chub_episode_summary_device(drain = 0) over the finished block (every env pending)
  (d) block_d2h                       the device-to-host copy of a whole finished block [EP_COUNT, N] f64 into pinned memory, which the
                                      summary call replaces (29 doubles instead)
    python tools/episode_stats_rate.py [--shape 65536x20,25] [--groups 8] [--rounds 3] [--out profiles/episode_stats_rate.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import charginghub_env_amd as chub
from charginghub_env_amd import _lib

HUB = dict(hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2, fc_max_power=100.0, fcev_permeate=0.01)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="65536x20,25")
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n_s, piles_s = args.shape.split("x")
    n, piles, G = int(n_s), [int(x) for x in piles_s.split(",")], args.groups
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream().cuda_stream
    lib = chub.load_library()

    def handle(ledger):
        v = chub.VecChargingHub(n, piles, ["fast", "slow"], seed=1, rng="philox", **HUB)
        if ledger:
            v.set_episode_stats(True)
        return v

    lock = {False: handle(False), True: handle(True)}
    auto = {False: handle(False), True: handle(True)}
    D, A = lock[True].obs_dim, lock[True].act_dim
    gen = torch.Generator(device="cuda").manual_seed(1)
    act = torch.rand((n, A), device="cuda", generator=gen) * 2 - 1
    packed = torch.empty((n, D + 2), device="cuda")
    final = torch.empty((n, D), device="cuda")
    obs = torch.empty((n, D), device="cuda")
    rew, done = torch.empty(n, device="cuda"), torch.empty(n, device="cuda", dtype=torch.uint8)
    grp = (torch.arange(n, device="cuda") * G // n)
    apart = 96 // G
    mask = torch.empty(n, device="cuda", dtype=torch.uint8)
    for v in auto.values():  # the same staggered start for both auto-reset legs
        v.reset_device(obs.data_ptr(), stream=stream)
        for k in range(1, (G - 1) * apart + 1):
            mask.copy_((grp * apart >= k).to(torch.uint8))
            v.step_envs_dmask_device(mask.data_ptr(), act.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(), stream=stream)
    for v in lock.values():
        v.reset_device(obs.data_ptr(), stream=stream)
    torch.cuda.synchronize()

    legs = {}
    for on in (False, True):
        legs["lock_step_" + ("on" if on else "off")] = lambda v=lock[on]: v.step_device_packed(act.data_ptr(), packed.data_ptr(), stream=stream)
        legs["autoreset_" + ("on" if on else "off")] = lambda v=auto[on]: v.step_autoreset_device(act.data_ptr(), packed.data_ptr(), final.data_ptr(),
                                                                                                  stream=stream)

    def day_events(fn, calls=96):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for i in range(calls):
            fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / calls

    for fn in legs.values():  # one warm-up day each: afterwards every env of the ledger-on handles has a finished episode pending
        for i in range(96):
            fn()
    torch.cuda.synchronize()
    best = {}
    for r in range(args.rounds):  # alternating legs
        for name, fn in legs.items():
            us = day_events(fn)
            best[name] = us if name not in best else min(best[name], us)

    v = auto[True]
    words = 1 + 4 * _lib.EP_COUNT
    d_sum = torch.zeros(words, dtype=torch.float64, device="cuda")
    d_block = torch.zeros((_lib.EP_COUNT, n), dtype=torch.float64, device="cuda")
    h_block = torch.zeros((_lib.EP_COUNT, n), dtype=torch.float64).pin_memory()
    v.episode_stats_device(d_block.data_ptr(), finished=True, stream=stream)

    def call_summary():
        v.episode_summary_device(d_sum.data_ptr(), drain=False, stream=stream)

    def call_d2h():
        h_block.copy_(d_block, non_blocking=True)

    for fn in (call_summary, call_d2h):
        for i in range(8):
            fn()
    torch.cuda.synchronize()
    summary_us = min(day_events(call_summary, 32) for _ in range(args.rounds))
    d2h_us = min(day_events(call_d2h, 32) for _ in range(args.rounds))
    torch.cuda.synchronize()
    res = dict(mode="philox", shape=args.shape, n_envs=n, piles=piles, groups=G, rounds=args.rounds, build_id=lib.chub_build_id().decode(),
               lock_step_off_us=round(best["lock_step_off"], 2), lock_step_on_us=round(best["lock_step_on"], 2),
               autoreset_off_us=round(best["autoreset_off"], 2), autoreset_on_us=round(best["autoreset_on"], 2),
               summary_us=round(summary_us, 2), summary_pending=int(d_sum[0].item()), block_d2h_us=round(d2h_us, 2),
               block_bytes=int(h_block.numel() * 8), summary_bytes=8 * words, uses_fused_step=bool(lock[True].uses_fused_step))
    print(json.dumps(res), flush=True)
    for h in list(lock.values()) + list(auto.values()):
        h.close()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump([res], open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
