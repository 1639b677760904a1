#!/usr/bin/env python3
"""Handles on the two-launch step: microseconds per step of chub_run_steps as hipGraph replays of two days (what bench.py times) with every step
a slot launch and a tail launch (span_steps = 1) against pairs of steps with ONE tail launch (span_steps = 2: k_env_pair), by batch size, the two
forms alternating, + a checksum of the last block -- where the pair rule's size threshold (kPairMinEnvs, csrc/chub_plan.h) belongs:
    python3 tools/pair_rate.py --envs 8704 16384 24576 32768 65536"""
import argparse, ctypes as C, sys, time
sys.path.insert(0, ".")
ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, nargs="+", default=[8704, 16384, 24576, 32768, 65536])
ap.add_argument("--days", type=int, default=40)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()
import numpy as np
import charginghub_env_amd as chub
from charginghub_env_amd import multi_gpu
from charginghub_env_amd._lib import check
kw = dict(station_list=[20, 25], station_type_list=["fast", "slow"], hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2, fc_max_power=100.0, fcev_permeate=0.01)


def rate(n, span):
    v = chub.VecChargingHub(n, seed=1, span_steps=span, fused_step="off", **kw)
    D, A = v.obs_dim, v.act_dim
    st = multi_gpu.Stream(0)
    acts = [multi_gpu.DeviceBuffer(n * A * 4) for _ in range(4)]
    for b, a in enumerate(acts):
        v.random_actions_device(a.ptr, 123, b, st.ptr)
    packed = [multi_gpu.DeviceBuffer(n * (D + 2) * 4) for _ in range(2)]
    obs0 = multi_gpu.DeviceBuffer(n * D * 4)
    c_acts = (C.c_void_p * 4)(*[a.ptr for a in acts])
    c_packed = (C.c_void_p * 2)(packed[0].ptr, packed[1].ptr)
    st.sync()
    v.graph_begin(st.ptr)
    check(v._lib.chub_run_steps(v._h, None, c_acts, 4, c_packed, None, obs0.ptr, 0, 192, st.ptr))
    g = v.graph_end(st.ptr)
    for _ in range(3):
        v.graph_launch(g, st.ptr)
    st.sync()
    reps = max(1, args.days // 2)
    t0 = time.perf_counter()
    for _ in range(reps):
        v.graph_launch(g, st.ptr)
    st.sync()
    us = (time.perf_counter() - t0) / (reps * 192) * 1e6
    v.graph_destroy(g)
    chk = float(packed[1].to_host(np.float32, (n, D + 2), st.ptr).astype(np.float64).sum())
    pairs = v.uses_pair_tails
    v.close()
    st.destroy()
    return us, chk, pairs


for n in args.envs:
    single, paired = [], []
    for _ in range(args.repeats):
        a, chk_a, pa = rate(n, "off")
        b, chk_b, pb = rate(n, 2)
        assert not pa and pb and chk_a == chk_b, (n, pa, pb, chk_a, chk_b)
        single.append(a)
        paired.append(b)
    ms, mp = sorted(single)[len(single) // 2], sorted(paired)[len(paired) // 2]
    print("n %6d  every step two launches %s  median %.2f us/step   pairs %s  median %.2f   gain %.2f %%   checksum %.6f" % (
        n, " ".join("%.2f" % x for x in single), ms, " ".join("%.2f" % x for x in paired), mp, (ms / mp - 1) * 100, chk_a))
