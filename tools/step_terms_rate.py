#!/usr/bin/env python3
"""The step terms on a device-resident PHILOX handle (chub_get_step_terms_device, chub_set_step_terms), two measurements:
  launch  us per explicit call for all 27 columns and for three constraint columns, each beside a hipMemsetAsync of the same output on
          the same stream (the write-only yardstick);
  step    us per lock-step chub_step_device_packed on three handles of one seed: telemetry off, telemetry on, telemetry on with all 27
          columns attached (the launch then rides behind every step).
Each handle is reset and stepped 30 times first; every case is warmed up, then the cases alternate, CALLS calls between two stream
synchronisations each, ROUNDS times; median, best and worst round are reported.
    python tools/step_terms_rate.py [--shape 65536x20,25] [--rounds 11] [--calls 500] [--out profiles/step_terms_rate.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import charginghub_env_amd as chub
from charginghub_env_amd import _lib, multi_gpu

FIELD_SETS = [("all", None), ("constraints", ("not_meet_loss", "grid_excess", "soc_penalty"))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="65536x20,25")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n_s, piles_s = args.shape.split("x")
    n, piles = int(n_s), [int(x) for x in piles_s.split(",")]
    st = multi_gpu.Stream(0)
    stream = st.ptr
    lib = chub.load_library()
    hip = ctypes.CDLL("libamdhip64.so")  # (the runtime libchub has loaded)
    hip.hipMemsetAsync.restype = ctypes.c_int
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    build_id = lib.chub_build_id().decode()

    handles, bufs = {}, []
    for name, telemetry, attached in (("telemetry_off", False, False), ("telemetry_on", True, False), ("terms_attached", True, True)):
        v = chub.VecChargingHub(n, seed=1, rng="philox", station_list=piles, station_type_list=["fast", "slow"], hydro_prod_rate=100.0,
                                hydro_store_vlt=25.0, init_soc=0.2, fc_max_power=100.0, fcev_permeate=0.01)
        if telemetry:
            v.set_telemetry(True)
        acts = [multi_gpu.DeviceBuffer(n * v.act_dim * 4) for _ in range(2)]
        for b, a in enumerate(acts):
            v.random_actions_device(a.ptr, 123, b, stream)
        packed = multi_gpu.DeviceBuffer(n * (v.obs_dim + 2) * 4)
        terms = multi_gpu.DeviceBuffer(n * _lib.ST_COUNT * 4)
        if attached:
            v.attach_step_terms(terms.ptr)
        v.reset_device(packed.ptr, stream=stream)
        for t in range(30):
            v.step_device_packed(acts[t & 1].ptr, packed.ptr, stream=stream)
        st.sync()
        handles[name] = (v, acts, packed, terms)
        bufs += acts + [packed, terms]

    cases = {}
    v, _, _, terms = handles["telemetry_on"]
    for fname, fields in FIELD_SETS:
        mask = _lib.st_fields_mask(fields)
        nbytes = 4 * n * len(_lib.st_fields_names(mask))
        cases[("launch", fname, "step_terms", nbytes)] = lambda v=v, mask=mask, p=terms.ptr: v.step_terms_device(p, mask, stream=stream)

        def memset(p=terms.ptr, nbytes=nbytes):
            rc = hip.hipMemsetAsync(p, 0, nbytes, stream)
            assert rc == 0, rc
        cases[("launch", fname, "memset", nbytes)] = memset
    for name, (v, acts, packed, _) in handles.items():
        def step(v=v, acts=acts, packed=packed, k=[0]):
            v.step_device_packed(acts[k[0] & 1].ptr, packed.ptr, stream=stream)
            k[0] += 1
        cases[("step", name, "step_device_packed", 0)] = step

    def batch(fn):
        st.sync()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        st.sync()
        return (time.perf_counter() - t0) / args.calls * 1e6

    for fn in cases.values():  # warm-up
        batch(fn)
    times = {c: [] for c in cases}
    for _ in range(args.rounds):
        for c, fn in cases.items():
            times[c].append(batch(fn))
    rows = []
    for (kind, name, route, nbytes), ts in times.items():
        med = statistics.median(ts)
        row = dict(shape=args.shape, n_envs=n, piles=piles, mode="philox", kind=kind, case=name, route=route, out_bytes=nbytes, rounds=len(ts),
                   calls_per_round=args.calls, us_per_call_median=round(med, 2), us_per_call_min=round(min(ts), 2), us_per_call_max=round(max(ts), 2),
                   build_id=build_id)
        if kind == "step":
            row["env_steps_per_s_median"] = round(n / med * 1e6)
        rows.append(row)
        print(json.dumps(row), flush=True)
    for v, _, _, _ in handles.values():
        v.close()
    for b in bufs:
        b.free()
    st.destroy()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
