#!/usr/bin/env python3
"""The device actor (chub_policy_*) on a device-resident PHILOX handle, measurements on ONE build in one process:
  launch          us per chub_policy_act_device (bits + tail out), CALLS launches between two HIP events;
  closed_loop     env-steps/s of chub_policy_run_steps (lock-step mode: reset, then per step the actor and the bits-form step) over ten days;
  open_loop       the same for chub_run_steps with its open-loop random action batches;
  sampled_launch  us per chub_policy_sample_device (bits + tail + u + logp out), as `launch`;
  collect         env-steps/s of chub_policy_collect in lock-step mode, ten calls of one day each, every step's block and action kept;
  pile_set_*      us per chub_pile_set_device, one case per set (all, occupied, decidable), as `launch`;
  sampled_set_launch  us per chub_policy_sample_set_device with the decidable set (the set launch and the set-aware actor launch), as `launch`;
  collect_set     env-steps/s of chub_policy_collect_set with the decidable set, as `collect`;
  gae             us per chub_rollout_gae_device over the collected day (T = 96, with d_ret, d_final_values and d_stats), with the bytes it
                  asks for and the bytes of the lines it touches; with --torch-gae also gae_torch, the same recurrence as a torch loop over
                  the same device memory in the same process (torch is then imported first, so that both share one HIP runtime).
  --population    adds, around the same policy as the centre: pop_launch_P<P> us per chub_population_act_device at P = 2, 256 and 2048 members
                  (as `launch`; at P = 2048 every workgroup reads its own member's weights), pop_closed_loop env-steps/s of
                  chub_population_run_steps at P = 256 (as `closed_loop`), perturb_P<P> and es_gradient_P<P> us per
                  chub_population_perturb_device / chub_population_es_gradient_device at P = 256 and 2048, with the Philox blocks a call
                  computes; the sampled and set cases are left out.
  --policy-grad   adds, after one collected day with decidable sets and raw feature rows: policy_grad us per chub_policy_grad_device over the
                  whole day (R = 96 N rows, PPO_CLIP with the sets, every gradient output) and policy_eval us per forward-only call, with
                  the algorithmic FLOP of each; with --torch-grad also policy_grad_torch, the same update as torch autograd over the same
                  device memory in the same process (f32 network, wrappers.sampled_logp / sampled_entropy; torch is then imported first).
                  The other sampled and set cases are left out.
  --critic        the --policy-grad cases and, over the same collected day's feature rows, a 13-64-64-1 critic (the actor's hidden widths):
                  critic_values us per chub_critic_values_device over the R rows, critic_grad us per chub_critic_grad_device under CLIPPED
                  with every output, critic_grad_mb4096 the same call over a minibatch of 4096 rows picked by d_rows, and critic_grad_large /
                  critic_values_large for a 13-256-224-1 critic (dW tiles in the partials, 137 KB of LDS); with --torch-critic also
                  critic_values_torch and critic_grad_torch, the same two as torch autograd over the same device memory.
  --adam          a case of its own (torch first, one process, TorchHubVecEnv; T = 96, actor 13-64-64-47 and critic 13-64-64-1): the UPDATE
                  PART of one minibatch, everything between the two gradient calls and the next -- update_torch: torch Adam.step() on both
                  networks plus the set_weights_device / set_log_std_device calls of quickstart part 9; update_device: two
                  chub_adam_step_device -- and the whole epoch at minibatches of 4096 and of 65 536 rows: epoch_torch_mb<R> issued eagerly
                  the parent's way (torch.randperm outside), epoch_device_mb<R> eagerly with the device shuffle and steps,
                  epoch_graph_mb<R> the same chain recorded once and replayed; shuffle / shuffle_torch: chub_shuffle_rows_device against
                  torch.randperm over the rollout's rows.  us per update, ms per epoch, us per shuffle, between two events.
  --trainlog      a case of its own beside --adam's (the same rollout, nets and optimisers): the whole epoch at minibatches of 4096 and of
                  65 536 rows as ONE chub_ppo_update -- epoch_update_mb<R> without a log, epoch_update_log_mb<R> with one (two more launches per
                  minibatch, one more per update) -- each eagerly and as one captured graph replayed (.._graph_..), and beside them
                  --adam's epoch_device_mb<R> / epoch_graph_mb<R>, the same chain issued call by call from Python.  ms per epoch.
  --lagrange      a case of its own (torch first, TorchHubVecEnv; T = 96): on one collected rollout with all 27 step terms kept,
                  gae_reward: chub_rollout_gae_device (with ret and stats) as the parent commit has it; cost_gae_k<K>_c<C>:
                  chub_lagrange_gae_device (values, returns and the episode carry for every constraint) at K = 1, 2, 4 with C = K terms
                  columns and at K = 2 reading two columns of the 27; combine_k2 / combine_k2_torch: chub_lagrange_combine_device against
                  the same arithmetic as one torch expression, combine_k2_rotating: the launch over four rotating sets of its arrays, more
                  than the 256 MiB cache holds; lagrange_step: the multipliers' launch.  us per call between two events,
                  with the bytes each call must move (bytes_useful) and the bytes its strided reads touch at 64-byte granularity (bytes_lines).
  --return-norm   a case of its own (torch first, TorchHubVecEnv; T = 96): on one collected rollout, gae_reward: chub_rollout_gae_device
                  (with ret and stats) as the parent commit has it; gae_scaled: chub_return_norm_gae_device on the same arrays;
                  return_norm_update: chub_return_norm_update_device (two launches); return_norm_torch: the same arithmetic as eager
                  torch (a forward loop for g, var, the scaled and clipped reward).  us per call between two events, with bytes_useful
                  and bytes_lines as --lagrange counts them.  With CHUB_LIB=<the parent's libchub.so> only gae_reward runs: the
                  unscaled call on the parent's library, for the process-to-process spread.
Every case is warmed up, then the cases alternate, ROUNDS times; median, best and worst round are reported with the build id.
--open-loop-only measures the open loop alone, --launch-only the open loop and the deterministic launch, --no-sets the first five cases:
with CHUB_LIB=<another build's libchub.so> those are the rates of a build without the newer entry points (the parent commit), on the same
device; run in alternating processes with this build's they show what the run-to-run spread is.
    python tools/policy_rate.py [--shape 65536x20,25] [--hidden 64,64] [--rounds 7] [--calls 200] [--days 10] [--out profiles/policy_rate.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

if "--torch-gae" in sys.argv or "--torch-grad" in sys.argv or "--torch-critic" in sys.argv or "--adam" in sys.argv or "--trainlog" in sys.argv or "--lagrange" in sys.argv or "--return-norm" in sys.argv:
    import torch  # before libchub is loaded: both must share one HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import charginghub_env_amd as chub
from charginghub_env_amd import multi_gpu
from charginghub_env_amd._lib import check


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="65536x20,25")
    ap.add_argument("--hidden", default="64,64")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--days", type=int, default=10)
    ap.add_argument("--open-loop-only", action="store_true")
    ap.add_argument("--launch-only", action="store_true")
    ap.add_argument("--torch-gae", action="store_true")
    ap.add_argument("--no-sets", action="store_true", help="the first five cases only: what a build without the pile set entry points can run")
    ap.add_argument("--population", action="store_true", help="the open loop, the launch, the closed loop and the population cases")
    ap.add_argument("--policy-grad", action="store_true", help="the open loop, the launch and the actor-gradient cases")
    ap.add_argument("--torch-grad", action="store_true")
    ap.add_argument("--critic", action="store_true", help="the actor-gradient cases and the critic's, in one process")
    ap.add_argument("--torch-critic", action="store_true")
    ap.add_argument("--adam", action="store_true", help="the optimiser's cases alone (see the module's text)")
    ap.add_argument("--trainlog", action="store_true", help="one chub_ppo_update per epoch, with and without a training log (see the module's text)")
    ap.add_argument("--lagrange", action="store_true", help="the cost GAE, the combine and the step launches beside the reward GAE (see the module's text)")
    ap.add_argument("--return-norm", action="store_true", help="the return statistics' update and the scaled GAE beside the reward GAE (see the module's text)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.lagrange:
        return lagrange_cases(args)
    if args.return_norm:
        return return_norm_cases(args)
    if args.adam:
        return adam_cases(args)
    if args.trainlog:
        return trainlog_cases(args)
    n_s, piles_s = args.shape.split("x")
    n, piles = int(n_s), [int(x) for x in piles_s.split(",")]
    hidden = [int(x) for x in args.hidden.split(",") if x]
    st = multi_gpu.Stream(0)
    stream = st.ptr
    lib = chub.load_library()
    hip = ctypes.CDLL("libamdhip64.so")  # (the runtime libchub has loaded)
    for name, argtypes in (("hipEventCreate", [ctypes.POINTER(ctypes.c_void_p)]), ("hipEventRecord", [ctypes.c_void_p, ctypes.c_void_p]),
                           ("hipEventSynchronize", [ctypes.c_void_p]),
                           ("hipEventElapsedTime", [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p])):
        getattr(hip, name).restype = ctypes.c_int
        getattr(hip, name).argtypes = argtypes
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(ctypes.byref(e)) == 0
    build_id = lib.chub_build_id().decode()

    v = chub.VecChargingHub(n, seed=1, rng="philox", station_list=piles, station_type_list=["fast", "slow"], hydro_prod_rate=100.0,
                            hydro_store_vlt=25.0, init_soc=0.2, fc_max_power=100.0, fcev_permeate=0.01)
    D, A = v.obs_dim, v.act_dim
    acts = [multi_gpu.DeviceBuffer(n * A * 4) for _ in range(4)]
    for b, a in enumerate(acts):
        v.random_actions_device(a.ptr, 123, b, stream)
    packed = [multi_gpu.DeviceBuffer(n * (D + 2) * 4) for _ in range(2)]
    obs0 = multi_gpu.DeviceBuffer(n * D * 4)
    bits, tail = multi_gpu.DeviceBuffer(n * v.bit_words * 8), multi_gpu.DeviceBuffer(n * 2 * 4)
    c_acts = (ctypes.c_void_p * 4)(*[a.ptr for a in acts])
    c_packed = (ctypes.c_void_p * 2)(packed[0].ptr, packed[1].ptr)
    steps = 96 * args.days

    def between_events(fn):
        assert hip.hipEventRecord(ev[0], stream) == 0
        fn()
        assert hip.hipEventRecord(ev[1], stream) == 0
        assert hip.hipEventSynchronize(ev[1]) == 0
        ms = ctypes.c_float()
        assert hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[1]) == 0
        return ms.value

    def open_loop():
        st.sync()
        t0 = time.perf_counter()
        check(lib.chub_run_steps(v._h, None, c_acts, 4, c_packed, None, obs0.ptr, 0, steps, stream))
        st.sync()
        return n * steps / (time.perf_counter() - t0)

    cases = {("open_loop", "chub_run_steps", "env_steps_per_s"): open_loop}
    notes = {}  # kind -> what a row of that case says on top
    if not args.open_loop_only:
        rs = np.random.RandomState(0)
        sizes = [D] + hidden + [A]
        layers = [((rs.normal(size=(o, i)) / np.sqrt(i)).astype(np.float32), (0.1 * rs.normal(size=o)).astype(np.float32))
                  for i, o in zip(sizes[:-1], sizes[1:])]
        pol = v.make_policy(layers)

        def launch():
            def many():
                for _ in range(args.calls):
                    pol.act_device(packed[1].ptr, D + 2, d_pile_bits=bits.ptr, d_tail=tail.ptr, stream=stream)
            return between_events(many) * 1e3 / args.calls

        def closed_loop():
            st.sync()
            t0 = time.perf_counter()
            pol.run_steps([p.ptr for p in packed], steps, mode="lockstep", d_reset_obs=obs0.ptr, stream=stream)
            st.sync()
            return n * steps / (time.perf_counter() - t0)

        cases[("launch", "chub_policy_act_device", "us_per_launch")] = launch
        if args.population:
            cases[("closed_loop", "chub_policy_run_steps", "env_steps_per_s")] = closed_loop
            population_cases(cases, notes, v, pol, sizes, packed, obs0, bits, tail, st, steps, args.calls, between_events)
            args.launch_only = True  # (the sampled and set cases are not part of this run)
        if args.policy_grad or args.critic:
            roll = policy_grad_cases(cases, notes, v, pol, layers, obs0, st, max(1, args.calls // 20), between_events, args.torch_grad)
            if args.critic:
                critic_cases(cases, notes, v, roll, hidden, st, max(1, args.calls // 20), between_events, args.torch_critic)
            args.launch_only = True
        if not args.launch_only:
            cases[("closed_loop", "chub_policy_run_steps", "env_steps_per_s")] = closed_loop
            # the SAMPLED actor: one launch with bits + tail + u + logp out, and chub_policy_collect in lock-step mode, a day per call
            pol.set_exploration(2024, np.array([-0.5, -0.5], dtype=np.float32))
            W = v.bit_words
            roll = dict(packed=multi_gpu.DeviceBuffer(96 * n * (D + 2) * 4), bits=multi_gpu.DeviceBuffer(96 * n * W * 8),
                        tail=multi_gpu.DeviceBuffer(96 * n * 2 * 4), u=multi_gpu.DeviceBuffer(96 * n * 2 * 4), logp=multi_gpu.DeviceBuffer(96 * n * 4))

            def sampled_launch():
                def many():
                    for _ in range(args.calls):
                        pol.sample_device(packed[1].ptr, D + 2, d_logp=roll["logp"].ptr, d_pile_bits=bits.ptr, d_tail=tail.ptr, d_u=roll["u"].ptr,
                                          stream=stream)
                return between_events(many) * 1e3 / args.calls

            def collect():
                st.sync()
                t0 = time.perf_counter()
                for _ in range(args.days):
                    pol.collect(96, obs0.ptr, roll["packed"].ptr, roll["bits"].ptr, roll["tail"].ptr, roll["u"].ptr, roll["logp"].ptr,
                                mode="lockstep", stream=stream)
                st.sync()
                return n * steps / (time.perf_counter() - t0)

            cases[("sampled_launch", "chub_policy_sample_device", "us_per_launch")] = sampled_launch
            cases[("collect", "chub_policy_collect", "env_steps_per_s")] = collect

        if not args.launch_only and not args.no_sets:
            # pile sets, the set-aware sampled launch and collect, and GAE over the collected day
            roll["set"] = multi_gpu.DeviceBuffer(96 * n * W * 8)
            T = 96
            gae = dict(values=multi_gpu.DeviceBuffer((T + 1) * n * 4), final=multi_gpu.DeviceBuffer(n * 4), adv=multi_gpu.DeviceBuffer(T * n * 4),
                       ret=multi_gpu.DeviceBuffer(T * n * 4), stats=multi_gpu.DeviceBuffer(24))
            gae["values"].from_host(rs.normal(size=((T + 1) * n,)).astype(np.float32))
            gae["final"].from_host(rs.normal(size=(n,)).astype(np.float32))

            def pile_set(which):
                def run():
                    def many():
                        for _ in range(args.calls):
                            v.pile_set_device(roll["set"].ptr, which, stream=stream)
                    return between_events(many) * 1e3 / args.calls
                return run

            def sampled_set_launch():
                def many():
                    for _ in range(args.calls):
                        pol.sample_device(packed[1].ptr, D + 2, d_logp=roll["logp"].ptr, d_pile_bits=bits.ptr, d_tail=tail.ptr, d_u=roll["u"].ptr,
                                          stream=stream, logp_piles="decidable", d_set_bits=roll["set"].ptr)
                return between_events(many) * 1e3 / args.calls

            def collect_set():
                st.sync()
                t0 = time.perf_counter()
                for _ in range(args.days):
                    pol.collect(96, obs0.ptr, roll["packed"].ptr, roll["bits"].ptr, roll["tail"].ptr, roll["u"].ptr, roll["logp"].ptr,
                                mode="lockstep", stream=stream, logp_piles="decidable", d_set_bits=roll["set"].ptr)
                st.sync()
                return n * steps / (time.perf_counter() - t0)

            gae_calls = max(1, args.calls // 10)

            def gae_device():
                def many():
                    for _ in range(gae_calls):
                        v.gae_device(T, roll["packed"].ptr, gae["values"].ptr, gae["adv"].ptr, d_ret=gae["ret"].ptr, d_final_values=gae["final"].ptr,
                                     gamma=0.99, lam=0.95, d_stats=gae["stats"].ptr, stream=stream)
                return between_events(many) * 1e3 / gae_calls

            for which in ("all", "occupied", "decidable"):
                cases[("pile_set_" + which, "chub_pile_set_device", "us_per_launch")] = pile_set(which)
            cases[("sampled_set_launch", "chub_policy_sample_set_device", "us_per_launch")] = sampled_set_launch
            cases[("collect_set", "chub_policy_collect_set", "env_steps_per_s")] = collect_set
            cases[("gae", "chub_rollout_gae_device", "us_per_call")] = gae_device
            if args.torch_gae:
                cases[("gae_torch", "a torch loop over the same memory", "us_per_call")] = torch_gae_case(roll["packed"].ptr, gae, n, T, D, max(1, gae_calls // 4))

    for fn in cases.values():  # warm-up (the open loop first: it leaves real observations in the packed blocks)
        fn()
    values = {c: [] for c in cases}
    for _ in range(args.rounds):
        for c, fn in cases.items():
            values[c].append(fn())
    rows = []
    for (kind, route, unit), xs in values.items():
        row = dict(shape=args.shape, n_envs=n, piles=piles, mode="philox", net=[D] + hidden + [A], kind=kind, route=route, unit=unit, rounds=len(xs),
                   median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3), steps_per_round=steps,
                   launches_per_round=args.calls, build_id=build_id, lib=os.environ.get("CHUB_LIB", ""))
        row.update(notes.get(kind, {}))
        if kind in ("gae", "gae_torch"):  # what the recurrence asks for (V, reward + done in; adv, ret out), and the lines that holds at a
            useful = 96 * n * (4 + 8 + 4 + 4) + n * 8           # (D + 2) * 4-byte row stride: every line of the packed blocks
            lines = 96 * n * ((D + 2) * 4 + 4 + 4 + 4) + n * 8
            row.update(bytes_asked_for=useful, bytes_of_lines_touched=lines, gb_per_s_of_lines=round(lines / (row["median"] * 1e-6) / 1e9, 1))
        rows.append(row)
        print(json.dumps(row), flush=True)
    v.close()
    st.destroy()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


def population_cases(cases, notes, v, pol, sizes, packed, obs0, bits, tail, st, steps, calls, between_events):
    """the --population cases: populations of 2, 256 and 2048 members around `pol`, all perturbed from it once"""
    n, D, stream = v.n_envs, v.obs_dim, st.ptr
    shapes = list(zip(sizes[1:], sizes[:-1]))
    pops = {P: v.make_population(pol, P, 77) for P in (2, 256, 2048)}
    for q in pops.values():
        q.perturb_device(0.05, 1, stream=stream)
    util = multi_gpu.DeviceBuffer(2048 * 4)
    util.from_host(np.random.RandomState(1).normal(size=2048).astype(np.float32))
    gW, gb = [multi_gpu.DeviceBuffer(o * i * 4) for o, i in shapes], [multi_gpu.DeviceBuffer(o * 4) for o, _ in shapes]
    few = max(1, calls // 10)

    def pop_launch(q):
        def run():
            def many():
                for _ in range(calls):
                    q.act_device(packed[1].ptr, D + 2, d_pile_bits=bits.ptr, d_tail=tail.ptr, stream=stream)
            return between_events(many) * 1e3 / calls
        return run

    def pop_closed_loop():
        st.sync()
        t0 = time.perf_counter()
        pops[256].run_steps([p.ptr for p in packed], steps, mode="lockstep", d_reset_obs=obs0.ptr, stream=stream)
        st.sync()
        return n * steps / (time.perf_counter() - t0)

    def perturb(q):
        def run():
            def many():
                for g in range(few):
                    q.perturb_device(0.05, g, stream=stream)
            return between_events(many) * 1e3 / few
        return run

    def es_gradient(q):
        def run():
            def many():
                for g in range(few):
                    q.es_gradient_device(util.ptr, g, [x.ptr for x in gW], [x.ptr for x in gb], stream=stream)
            return between_events(many) * 1e3 / few
        return run

    for P, q in pops.items():
        cases[("pop_launch_P%d" % P, "chub_population_act_device", "us_per_launch")] = pop_launch(q)
        notes["pop_launch_P%d" % P] = dict(members=P, weight_bytes_per_launch=(n // 32) * 4 * sum(
            ((o + 31) // 32 * 32) * (((i + 1) & ~1) + 1) for o, i in shapes))
    cases[("pop_closed_loop", "chub_population_run_steps", "env_steps_per_s")] = pop_closed_loop
    notes["pop_closed_loop"] = dict(members=256)
    for P in (256, 2048):
        blocks = (P // 2) * sum(o * (i // 4 + 1) for o, i in shapes)  # one block per (pair, output row, group of four columns of [W | b])
        cases[("perturb_P%d" % P, "chub_population_perturb_device", "us_per_call")] = perturb(pops[P])
        cases[("es_gradient_P%d" % P, "chub_population_es_gradient_device", "us_per_call")] = es_gradient(pops[P])
        notes["perturb_P%d" % P] = notes["es_gradient_P%d" % P] = dict(members=P, philox_blocks=blocks, launches_per_round=few)


def device_view(ptr, shape, typestr="<f4"):
    """a torch tensor over device memory this process owns (never read on the host: only the address and the shape are used)"""
    iface = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2)
    return torch.as_tensor(type("DeviceArray", (), {"__cuda_array_interface__": iface})(), device="cuda")


def policy_grad_cases(cases, notes, v, pol, layers, obs0, st, calls, between_events, with_torch):
    """the --policy-grad cases: one collected day (lock-step, decidable sets, raw feature rows), then the whole day as ONE batch"""
    n, D, W, T, stream = v.n_envs, v.obs_dim, v.bit_words, 96, st.ptr
    R, F = T * n, pol.n_features
    pol.set_exploration(2024, np.array([-0.5, -0.5], dtype=np.float32))
    B = multi_gpu.DeviceBuffer
    roll = dict(packed=B(R * (D + 2) * 4), bits=B(R * W * 8), tail=B(R * 8), u=B(R * 8), logp=B(R * 4), feat=B(R * F * 4), set=B(R * W * 8),
                adv=B(R * 4), logp_new=B(R * 4), ent=B(R * 4), stats=B(48), gls=B(16))
    pol.collect(T, obs0.ptr, roll["packed"].ptr, roll["bits"].ptr, roll["tail"].ptr, roll["u"].ptr, roll["logp"].ptr, d_features=roll["feat"].ptr,
                mode="lockstep", stream=stream, logp_piles="decidable", d_set_bits=roll["set"].ptr)
    roll["adv"].from_host(np.random.RandomState(2).normal(size=R).astype(np.float32))
    shapes = [W_.shape for W_, _ in layers]
    gW, gb = [B(o * i * 4) for o, i in shapes], [B(o * 4) for o, _ in shapes]
    g = v.make_policy_grad(pol, R)
    plan = g.plan()
    # the update moves the weights a little, so that ratios are not all 1 (the work does not depend on it)
    rs = np.random.RandomState(3)
    moved = [((W_ + 0.02 * rs.normal(size=W_.shape) / np.sqrt(W_.shape[1])).astype(np.float32), b_) for W_, b_ in layers]
    for l, (W_, b_) in enumerate(moved):
        pol.set_weights(l, W_, b_)

    def grad(backward):
        def run():
            def many():
                for _ in range(calls):
                    g.grad_device(R, R, roll["feat"].ptr, roll["u"].ptr, roll["adv"].ptr, roll["bits"].ptr, roll["set"].ptr, roll["logp"].ptr,
                                  loss="ppo_clip", clip_eps=0.2, ent_coef=0.01, d_gW=[x.ptr for x in gW] if backward else None,
                                  d_gb=[x.ptr for x in gb] if backward else None, d_glog_std=roll["gls"].ptr if backward else 0,
                                  d_logp_new=roll["logp_new"].ptr, d_entropy=roll["ent"].ptr, d_stats=roll["stats"].ptr, stream=stream)
            return between_events(many) * 1e3 / calls
        return run

    mac = sum(o * i for o, i in shapes)  # multiply-adds of one row's forward
    cases[("policy_grad", "chub_policy_grad_device", "us_per_call")] = grad(True)
    cases[("policy_eval", "chub_policy_grad_device, no gradient outputs", "us_per_call")] = grad(False)
    notes["policy_grad"] = dict(rows=R, launches_per_round=calls, flop_per_row=3 * 2 * mac, gflop_per_call=round(3 * 2 * mac * R / 1e9, 1),
                                workgroups=plan["workgroups"], lds_bytes=plan["lds_bytes"], in_registers=plan["in_registers"])
    notes["policy_eval"] = dict(rows=R, launches_per_round=calls, flop_per_row=2 * mac, gflop_per_call=round(2 * mac * R / 1e9, 1))
    if with_torch:
        from charginghub_env_amd import wrappers
        few = max(1, calls // 2)
        S = v.n_slots
        net = torch.nn.Sequential(*[m for k, (o, i) in enumerate(shapes) for m in ([torch.nn.Linear(i, o)] + ([torch.nn.Tanh()] if k < len(shapes) - 1 else []))]).to("cuda")
        lin = [m for m in net if isinstance(m, torch.nn.Linear)]
        with torch.no_grad():
            for m, (W_, b_) in zip(lin, moved):
                m.weight.copy_(torch.tensor(W_))
                m.bias.copy_(torch.tensor(b_))
        log_std = torch.tensor([-0.5, -0.5], device="cuda", requires_grad=True)
        feat, u, lp_old, adv = device_view(roll["feat"].ptr, (R, F)), device_view(roll["u"].ptr, (R, 2)), device_view(roll["logp"].ptr, (R,)), device_view(roll["adv"].ptr, (R,))
        bits, sets = device_view(roll["bits"].ptr, (R, W), "<i8"), device_view(roll["set"].ptr, (R, W), "<i8")

        def torch_grad():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(few):
                for prm in list(net.parameters()) + [log_std]:
                    prm.grad = None
                z = net(feat)
                lp = wrappers.sampled_logp(z, bits, u, log_std, piles=sets)
                en = wrappers.sampled_entropy(z, log_std, piles=sets)
                ratio = torch.exp(lp - lp_old)
                loss = (-torch.minimum(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv) - 0.01 * en).mean()
                loss.backward()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / few
        cases[("policy_grad_torch", "torch autograd over the same memory", "us_per_call")] = torch_grad
        notes["policy_grad_torch"] = dict(rows=R, launches_per_round=few)
    return roll


def critic_cases(cases, notes, v, roll, hidden, st, calls, between_events, with_torch):
    """the --critic cases: the collected day's raw feature rows as ONE batch, `ret` and `v_old` around the critic's own values"""
    n, T, stream = v.n_envs, 96, st.ptr
    R = T * n
    F = roll["feat"].nbytes // (4 * R)  # (the actor's feature row: the critic reads the same rows)
    B = multi_gpu.DeviceBuffer
    buf = dict(values=B(R * 4), ret=B(R * 4), v_old=B(R * 4), stats=B(48), rows=B(4096 * 8))
    buf["rows"].from_host(np.random.RandomState(5).permutation(R)[:4096].astype(np.int64))

    def make(widths, seed):
        rs = np.random.RandomState(seed)
        sizes = [F] + list(widths) + [1]
        layers = [((rs.normal(size=(o, i)) / np.sqrt(i)).astype(np.float32), (0.1 * rs.normal(size=o)).astype(np.float32)) for i, o in zip(sizes[:-1], sizes[1:])]
        cr = v.make_critic(layers, max_rows=R)
        shapes = [W_.shape for W_, _ in layers]
        return cr, layers, shapes, [B(o * i * 4) for o, i in shapes], [B(o * 4) for o, _ in shapes]

    cr, layers, shapes, gW, gb = make(hidden, 7)
    # v_old: the critic's values; ret: beside them; then the weights move a little, so that rows fall on both sides of the predicate
    cr.values_device(R, R, roll["feat"].ptr, buf["v_old"].ptr, stream=stream)
    st.sync()
    v0 = buf["v_old"].to_host(np.float32, (R,))
    buf["ret"].from_host((v0 + 0.5 * np.random.RandomState(8).normal(size=R)).astype(np.float32))
    rs = np.random.RandomState(9)
    moved = [((W_ + 0.1 * rs.normal(size=W_.shape) / np.sqrt(W_.shape[1])).astype(np.float32), b_) for W_, b_ in layers]
    for l, (W_, b_) in enumerate(moved):
        cr.set_weights(l, W_, b_)

    def values(c, k):
        def run():
            def many():
                for _ in range(k):
                    c.values_device(R, R, roll["feat"].ptr, buf["values"].ptr, stream=stream)
            return between_events(many) * 1e3 / k
        return run

    def grad(c, w, b, k, rows=0, Rc=R):
        def run():
            def many():
                for _ in range(k):
                    c.grad_device(Rc, R, roll["feat"].ptr, buf["ret"].ptr, buf["v_old"].ptr, rows, None, "clipped", 0.2, [x.ptr for x in w],
                                  [x.ptr for x in b], buf["values"].ptr, buf["stats"].ptr, stream)
            return between_events(many) * 1e3 / k
        return run

    mac = sum(o * i for o, i in shapes)
    plan = cr.plan()
    cases[("critic_values", "chub_critic_values_device", "us_per_call")] = values(cr, calls)
    cases[("critic_grad", "chub_critic_grad_device, CLIPPED, every output", "us_per_call")] = grad(cr, gW, gb, calls)
    cases[("critic_grad_mb4096", "chub_critic_grad_device, 4096 rows by d_rows", "us_per_call")] = grad(cr, gW, gb, 10 * calls, buf["rows"].ptr, 4096)
    notes["critic_values"] = dict(rows=R, launches_per_round=calls, flop_per_row=2 * mac, gflop_per_call=round(2 * mac * R / 1e9, 1),
                                  workgroups=plan["workgroups"], lds_bytes=plan["lds_bytes"])
    notes["critic_grad"] = dict(rows=R, launches_per_round=calls, flop_per_row=3 * 2 * mac, gflop_per_call=round(3 * 2 * mac * R / 1e9, 1),
                                workgroups=plan["workgroups"], lds_bytes=plan["lds_bytes"], in_registers=plan["in_registers"])
    notes["critic_grad_mb4096"] = dict(rows=4096, launches_per_round=10 * calls, workgroups=cr.plan(4096)["workgroups"])
    big, _, bshapes, bW, bb = make((256, 224), 11)
    bplan, bmac = big.plan(), sum(o * i for o, i in bshapes)
    cases[("critic_values_large", "chub_critic_values_device, %d-256-224-1" % F, "us_per_call")] = values(big, 2)
    cases[("critic_grad_large", "chub_critic_grad_device, %d-256-224-1" % F, "us_per_call")] = grad(big, bW, bb, 2)
    notes["critic_grad_large"] = dict(rows=R, launches_per_round=2, flop_per_row=3 * 2 * bmac, gflop_per_call=round(3 * 2 * bmac * R / 1e9, 1),
                                      workgroups=bplan["workgroups"], lds_bytes=bplan["lds_bytes"], in_registers=bplan["in_registers"])
    notes["critic_values_large"] = dict(rows=R, launches_per_round=2, flop_per_row=2 * bmac, gflop_per_call=round(2 * bmac * R / 1e9, 1))
    if with_torch:
        few = max(1, calls // 2)
        net = torch.nn.Sequential(*[m for k, (o, i) in enumerate(shapes) for m in ([torch.nn.Linear(i, o)] + ([torch.nn.Tanh()] if k < len(shapes) - 1 else []))]).to("cuda")
        lin = [m for m in net if isinstance(m, torch.nn.Linear)]
        with torch.no_grad():
            for m, (W_, b_) in zip(lin, moved):
                m.weight.copy_(torch.tensor(W_))
                m.bias.copy_(torch.tensor(b_))
        feat, ret, v_old = device_view(roll["feat"].ptr, (R, F)), device_view(buf["ret"].ptr, (R,)), device_view(buf["v_old"].ptr, (R,))

        def timed(fn):
            def run():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(few):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) * 1e3 / few
            return run

        def torch_values():
            with torch.no_grad():
                return net(feat)[:, 0]

        def torch_grad():
            for prm in net.parameters():
                prm.grad = None
            val = net(feat)[:, 0]
            v_c = v_old + torch.clamp(val - v_old, -0.2, 0.2)
            (0.5 * torch.maximum((val - ret) ** 2, (v_c - ret) ** 2)).mean().backward()

        cases[("critic_values_torch", "torch forward over the same memory", "us_per_call")] = timed(torch_values)
        cases[("critic_grad_torch", "torch autograd over the same memory", "us_per_call")] = timed(torch_grad)
        notes["critic_values_torch"] = dict(rows=R, launches_per_round=few)
        notes["critic_grad_torch"] = dict(rows=R, launches_per_round=few)


def torch_gae_case(packed_ptr, gae, n, T, D, calls):
    """the same recurrence written the usual way, as a reverse torch loop of elementwise launches over the same device memory (torch's
    current stream); timed with torch's own events"""
    def view(ptr, shape):
        count = int(np.prod(shape))
        buf = (ctypes.c_float * count).from_address(0)  # (never read on the host: only the address and the shape are used)
        iface = dict(shape=tuple(shape), typestr="<f4", data=(int(ptr), False), version=2)
        holder = type("DeviceArray", (), {"__cuda_array_interface__": iface})()
        del buf
        return torch.as_tensor(holder, device="cuda")

    packed, values, final = view(packed_ptr, (T, n, D + 2)), view(gae["values"].ptr, (T + 1, n)), view(gae["final"].ptr, (n,))
    adv, ret = torch.empty((T, n), device="cuda"), torch.empty((T, n), device="cuda")

    def once():
        nxt = torch.zeros(n, device="cuda")
        for t in range(T - 1, -1, -1):
            r, d = packed[t, :, D], packed[t, :, D + 1] != 0
            vn = torch.where(d, final, values[t + 1])
            delta = r + 0.99 * vn - values[t]
            nxt = delta + (0.99 * 0.95) * torch.where(d, torch.zeros_like(nxt), nxt)
            adv[t] = nxt
            ret[t] = nxt + values[t]
        return adv.double().sum(), (adv.double() ** 2).sum()

    def run():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            once()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls
    return run




def adam_cases(args):
    """--adam: the update part of a minibatch and the whole epoch, the parent's way and this build's, alternating in one process"""
    n_s, piles_s = args.shape.split("x")
    n, piles = int(n_s), [int(x) for x in piles_s.split(",")]
    hidden = [int(x) for x in args.hidden.split(",") if x]
    T = 96
    env = chub.TorchHubVecEnv(n, piles, ["fast", "slow"], seed=1, rng="philox", autoreset="per_env", hydro_prod_rate=100.0, hydro_store_vlt=25.0,
                              init_soc=0.2, fc_max_power=100.0, fcev_permeate=0.01)
    build_id = chub.load_library().chub_build_id().decode()
    D, A = env.obs_dim, env.act_dim
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)  # (a created stream: a recording needs one)

    def mlp(sizes):
        mods = []
        for i, o in zip(sizes[:-1], sizes[1:]):
            mods += [torch.nn.Linear(i, o), torch.nn.Tanh()]
        return torch.nn.Sequential(*mods[:-1]).to("cuda")

    def twin():
        """a policy and a critic with their nn.Sequentials (the same initial weights every time)"""
        torch.manual_seed(0)
        net, vnet = mlp([D] + hidden + [A]), mlp([D] + hidden + [1])
        pol = env.load_policy(net)
        pol.set_exploration(7, [-0.5, -0.5])
        return net, vnet, pol, env.load_critic(vnet)

    net, vnet, pol_t, crit_t = twin()        # the parent's way: torch optimisers, weights pushed back after every step
    _, _, pol_d, crit_d = twin()             # this build's way
    a_lin, c_lin = [m for m in net if isinstance(m, torch.nn.Linear)], [m for m in vnet if isinstance(m, torch.nn.Linear)]
    log_std = torch.full((2,), -0.5, device="cuda")
    a_opt_t = torch.optim.Adam([p for m in a_lin for p in (m.weight, m.bias)] + [log_std], lr=3e-4)
    c_opt_t = torch.optim.Adam([p for m in c_lin for p in (m.weight, m.bias)], lr=1e-3)
    a_opt_d, c_opt_d = env.make_optimizer(pol_d, lr=3e-4), env.make_optimizer(crit_d, lr=1e-3)
    env.reset()
    ro = env.collect(pol_t, T, logp_piles="decidable")
    env._rollout_policy[id(ro)] = pol_t
    values, final = env.values(crit_t, ro)
    adv, ret, adv_stats = env.advantages(ro, values, final, stats=True)
    v_old = values[:T].clone()
    R = T * n

    def grads_torch(rows):
        grads, gls, _ = env.policy_gradient(ro, adv, rows=rows, adv_stats=adv_stats)
        vg, _ = env.value_gradient(crit_t, ro, ret, rows=rows, loss="clipped", v_old=v_old)
        for m, (gW, gb) in zip(a_lin, grads):
            m.weight.grad, m.bias.grad = gW, gb
        log_std.grad = gls
        for m, (gW, gb) in zip(c_lin, vg):
            m.weight.grad, m.bias.grad = gW, gb

    def update_torch():
        st = torch.cuda.current_stream().cuda_stream
        a_opt_t.step()
        c_opt_t.step()
        for l, m in enumerate(a_lin):
            pol_t.set_weights_device(l, m.weight.data_ptr(), m.bias.data_ptr(), st)
        pol_t.set_log_std_device(log_std.data_ptr(), st)
        for l, m in enumerate(c_lin):
            crit_t.set_weights_device(l, m.weight.data_ptr(), m.bias.data_ptr(), st)

    def update_device():
        env.optimizer_step(a_opt_d)
        env.optimizer_step(c_opt_d)

    ro_d = dict(ro)  # the same rollout, differentiated through the second policy
    env._rollout_policy[id(ro_d)] = pol_d

    def grads_device(rows):
        env.policy_gradient(ro_d, adv, rows=rows, adv_stats=adv_stats, into=a_opt_d)
        env.value_gradient(crit_d, ro_d, ret, rows=rows, loss="clipped", v_old=v_old, into=c_opt_d)

    def epoch_torch(mb):
        perm = torch.randperm(R, device="cuda")
        for i in range(R // mb):
            grads_torch(perm[i * mb:(i + 1) * mb])
            update_torch()

    def epoch_device(mb):
        rows = env.shuffle_rows(R, 11, counter=a_opt_d)
        for i in range(R // mb):
            grads_device(rows[i * mb:(i + 1) * mb])
            update_device()

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps  # ms

    few = max(1, args.calls // 4)
    cases, failed = {}, {}
    grads_torch(None)
    grads_device(None)
    cases[("update_torch", "torch Adam.step() x 2 + 6 set_weights_device + set_log_std_device", "us_per_update")] = lambda: timed(update_torch, few) * 1e3
    cases[("update_device", "chub_adam_step_device x 2", "us_per_update")] = lambda: timed(update_device, few) * 1e3
    cases[("shuffle", "chub_shuffle_rows_device", "us_per_call")] = lambda: timed(lambda: env.shuffle_rows(R, 11, counter=a_opt_d), 20) * 1e3
    cases[("shuffle_torch", "torch.randperm", "us_per_call")] = lambda: timed(lambda: torch.randperm(R, device="cuda"), 20) * 1e3
    for mb in (4096, 65536):
        if R % mb:
            continue
        cases[("epoch_torch_mb%d" % mb, "eager, the parent's way", "ms_per_epoch")] = lambda mb=mb: timed(lambda: epoch_torch(mb), 1)
        cases[("epoch_device_mb%d" % mb, "eager, chub_adam_step_device and chub_shuffle_rows_device", "ms_per_epoch")] = lambda mb=mb: timed(lambda: epoch_device(mb), 1)
        epoch_device(mb)  # (every tensor the calls cache exists before the recording)
        torch.cuda.synchronize()
        try:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                epoch_device(mb)
            cases[("epoch_graph_mb%d" % mb, "one captured graph replayed", "ms_per_epoch")] = lambda graph=graph: timed(graph.replay, 1)
        except Exception as e:  # the row then says so: NOT MEASURED
            failed["epoch_graph_mb%d" % mb] = repr(e)[:300]
    for fn in cases.values():
        fn()
    vals = {c: [] for c in cases}
    for _ in range(args.rounds):
        for c, fn in cases.items():
            vals[c].append(fn())
    rows = []
    for (kind, route, unit), xs in vals.items():
        rows.append(dict(shape=args.shape, n_envs=n, piles=piles, T=T, rows=R, actor=[D] + hidden + [A], critic=[D] + hidden + [1], kind=kind, route=route,
                         unit=unit, rounds=len(xs), median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3), build_id=build_id))
    for kind, why in failed.items():
        rows.append(dict(shape=args.shape, kind=kind, unit="NOT MEASURED", error=why, build_id=build_id))
    for row in rows:
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)
    torch.cuda.synchronize()
    env.close()


def trainlog_cases(args):
    """--trainlog: the epoch as one chub_ppo_update, with and without a log, eager and replayed, beside --adam's call-by-call epoch"""
    n_s, piles_s = args.shape.split("x")
    n, piles = int(n_s), [int(x) for x in piles_s.split(",")]
    hidden = [int(x) for x in args.hidden.split(",") if x]
    T = 96
    env = chub.TorchHubVecEnv(n, piles, ["fast", "slow"], seed=1, rng="philox", autoreset="per_env", hydro_prod_rate=100.0, hydro_store_vlt=25.0,
                              init_soc=0.2, fc_max_power=100.0, fcev_permeate=0.01)
    build_id = chub.load_library().chub_build_id().decode()
    D, A = env.obs_dim, env.act_dim
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)  # (a created stream: a recording needs one)

    def mlp(sizes):
        mods = []
        for i, o in zip(sizes[:-1], sizes[1:]):
            mods += [torch.nn.Linear(i, o), torch.nn.Tanh()]
        return torch.nn.Sequential(*mods[:-1]).to("cuda")

    torch.manual_seed(0)
    pol = env.load_policy(mlp([D] + hidden + [A]))
    pol.set_exploration(7, [-0.5, -0.5])
    crit = env.load_critic(mlp([D] + hidden + [1]))
    a_opt, c_opt = env.make_optimizer(pol, lr=3e-4), env.make_optimizer(crit, lr=1e-3)
    log = env.make_train_log()
    env.reset()
    ro = env.collect(pol, T, logp_piles="decidable")
    values, final = env.values(crit, ro)
    adv, ret, adv_stats = env.advantages(ro, values, final, stats=True)
    v_old = values[:T].clone()
    R = T * n

    def epoch_calls(mb):  # (--adam's epoch_device: the chain issued call by call)
        rows = env.shuffle_rows(R, 11, counter=a_opt)
        for i in range(R // mb):
            r = rows[i * mb:(i + 1) * mb]
            env.policy_gradient(ro, adv, rows=r, adv_stats=adv_stats, into=a_opt)
            env.value_gradient(crit, ro, ret, rows=r, loss="clipped", v_old=v_old, into=c_opt)
            env.optimizer_step(a_opt)
            env.optimizer_step(c_opt)

    def epoch_update(mb, with_log):
        env.ppo_update(ro, adv, ret, a_opt, c_opt, epochs=1, minibatch_rows=mb, key=11, clip_eps=0.2, ent_coef=0.0, v_old=v_old, adv_stats=adv_stats,
                       log=log if with_log else None)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps  # ms

    cases, failed = {}, {}
    for mb in (4096, 65536):
        if R % mb:
            continue
        routes = {"epoch_device": ("the calls one by one from Python", lambda mb=mb: epoch_calls(mb)),
                  "epoch_update": ("one chub_ppo_update, no log", lambda mb=mb: epoch_update(mb, False)),
                  "epoch_update_log": ("one chub_ppo_update with a log", lambda mb=mb: epoch_update(mb, True))}
        for name, (route, fn) in routes.items():
            cases[("%s_mb%d" % (name, mb), "eager, " + route, "ms_per_epoch")] = lambda fn=fn: timed(fn, 1)
            fn()  # (every tensor the calls cache exists before the recording)
            torch.cuda.synchronize()
            kind = "%s_mb%d" % (name.replace("epoch_device", "epoch_graph").replace("epoch_update", "epoch_update_graph"), mb)
            try:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    fn()
                cases[(kind, "one captured graph replayed, " + route, "ms_per_epoch")] = lambda graph=graph: timed(graph.replay, 1)
            except Exception as e:  # the row then says so: NOT MEASURED
                failed[kind] = repr(e)[:300]
    for fn in cases.values():
        fn()
    vals = {c: [] for c in cases}
    for _ in range(args.rounds):
        for c, fn in cases.items():
            vals[c].append(fn())
    summary = env.train_log_summary(log)
    rows = []
    for (kind, route, unit), xs in vals.items():
        rows.append(dict(shape=args.shape, n_envs=n, piles=piles, T=T, rows=R, actor=[D] + hidden + [A], critic=[D] + hidden + [1], kind=kind, route=route,
                         unit=unit, rounds=len(xs), median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3), build_id=build_id))
    for kind, why in failed.items():
        rows.append(dict(shape=args.shape, kind=kind, unit="NOT MEASURED", error=why, build_id=build_id))
    rows.append(dict(shape=args.shape, kind="last_log", summary=summary, build_id=build_id))
    for row in rows:
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)
    torch.cuda.synchronize()
    env.close()


def lagrange_cases(args):
    """--lagrange: the constrained learner's launches beside the parent's reward GAE, on one collected rollout"""
    n_s, piles_s = args.shape.split("x")
    n, piles = int(n_s), [int(x) for x in piles_s.split(",")]
    T = 96
    env = chub.TorchHubVecEnv(n, piles, ["fast", "slow"], seed=1, rng="philox", autoreset="per_env", hydro_prod_rate=100.0, hydro_store_vlt=25.0,
                              init_soc=0.2, fc_max_power=100.0, fcev_permeate=0.01)
    build_id = chub.load_library().chub_build_id().decode()
    D, A = env.obs_dim, env.act_dim
    torch.manual_seed(0)
    lin = lambda i, o: torch.nn.Sequential(torch.nn.Linear(i, 64), torch.nn.Tanh(), torch.nn.Linear(64, o)).to("cuda")
    pol = env.load_policy(lin(D, A))
    pol.set_exploration(7, [-0.5, -0.5])
    crit = env.load_critic(lin(D, 1))
    env.reset()
    ro = env.collect(pol, T, logp_piles="decidable", terms=chub._lib.ST_NAMES)
    values, final = env.values(crit, ro)
    adv, ret, adv_stats = env.advantages(ro, values, final, stats=True)
    R = T * n
    f32 = dict(dtype=torch.float32, device=env.device)
    stream = torch.cuda.current_stream().cuda_stream
    row = (D + 2) * 4
    lines = lambda stride, used: min(stride, 64 * ((used + 63) // 64 + (1 if stride % 64 else 0)))  # bytes of a strided row its reads touch, at most

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3  # us

    cases, meta, keep = {}, {}, []
    cases["gae_reward"] = lambda: env.advantages(ro, values, final, stats=True)
    meta["gae_reward"] = dict(route="chub_rollout_gae_device with d_ret and d_stats", bytes_useful=R * (8 + 4 + 4 + 4), bytes_lines=R * (lines(row, 8) + 12))
    names = ("grid_excess", "not_meet", "soc_penalty", "soc_deviation")
    for K, C in ((1, 1), (2, 2), (4, 4), (2, 27)):
        cols = [chub._lib.ST[x] for x in names[:K]] if C == 27 else list(range(K))
        terms = ro["terms"] if C == 27 else ro["terms"][:, :, [chub._lib.ST[x] for x in names[:K]]].contiguous()
        lag = env.vec.make_lagrange([dict(column=c, kind="done" if names[k] == "soc_penalty" else "step", limit=1.0, lr=1e-3) for k, c in enumerate(cols)])
        advs, rets = [torch.zeros((T, n), **f32) for _ in range(K)], [torch.zeros((T, n), **f32) for _ in range(K)]
        carry = torch.zeros((n, K), dtype=torch.float64, device=env.device)
        keep.append((lag, terms, advs, rets, carry))
        kind = "cost_gae_k%d_c%d" % (K, C)
        cases[kind] = lambda lag=lag, terms=terms, advs=advs, rets=rets, carry=carry, K=K, C=C: lag.gae(
            T, C, terms.data_ptr(), ro["packed"].data_ptr(), [a.data_ptr() for a in advs], d_ret=[r.data_ptr() for r in rets],
            d_values=[values.data_ptr()] * K, d_final_values=[final.data_ptr()] * K, d_ep_carry=carry.data_ptr(), stream=stream)
        meta[kind] = dict(route="chub_lagrange_gae_device: values, returns and carry for every constraint",
                          bytes_useful=R * (4 + K * 16) + n * K * 16, bytes_lines=R * (lines(row, 4) + lines(4 * C, 4 * K) + K * 12) + n * K * 16)
    lag2 = keep[1][0]
    cadv = keep[1][2]
    out = torch.zeros((T, n), **f32)
    lam = torch.tensor([0.5, 2.0], dtype=torch.float64, device=env.device)
    cases["cost_gae_k2_c2"]()
    lag2.set_lambda_device(lam.data_ptr(), stream=stream)
    cases["combine_k2"] = lambda: lag2.combine(R, adv.data_ptr(), [c.data_ptr() for c in cadv], out.data_ptr(), d_adv_stats=adv_stats.data_ptr(), stream=stream)
    meta["combine_k2"] = dict(route="chub_lagrange_combine_device, two multipliers not 0", bytes_useful=R * 16, bytes_lines=R * 16)
    torch.cuda.synchronize()
    m = (adv_stats[1] / adv_stats[0]).float()
    sdev = (1.0 / torch.sqrt((adv_stats[2] / adv_stats[0] - (adv_stats[1] / adv_stats[0]) ** 2).clamp_min(0.0) + 1e-8)).float()
    mc = [c.mean() for c in cadv]
    inv = float(1.0 / (1.0 + 0.5 + 2.0))

    def combine_torch():
        torch.mul(((adv - m) * sdev) - 0.5 * (cadv[0] - mc[0]) - 2.0 * (cadv[1] - mc[1]), inv, out=out)

    cases["combine_k2_torch"] = combine_torch
    meta["combine_k2_torch"] = dict(route="the same arithmetic as one eager torch expression (its temporaries included)", bytes_useful=R * 16, bytes_lines=R * 16)
    # the same launch over four rotating sets of its arrays (4 x 101 MB, past the 256 MiB cache): the rate from HBM
    sets = [(adv.clone(), [c.clone() for c in cadv], torch.zeros((T, n), **f32)) for _ in range(4)]
    turn = [0]

    def combine_rotating():
        a, cs, o = sets[turn[0] % len(sets)]
        turn[0] += 1
        lag2.combine(R, a.data_ptr(), [c.data_ptr() for c in cs], o.data_ptr(), d_adv_stats=adv_stats.data_ptr(), stream=stream)

    cases["combine_k2_rotating"] = combine_rotating
    meta["combine_k2_rotating"] = dict(route="chub_lagrange_combine_device over four rotating sets of arrays (403 MB in all)", bytes_useful=R * 16, bytes_lines=R * 16)
    cases["lagrange_step"] = lambda: lag2.step(stream=stream)
    meta["lagrange_step"] = dict(route="chub_lagrange_step_device, K = 2", bytes_useful=2 * 11 * 8, bytes_lines=2 * 11 * 8)
    reps = {"lagrange_step": max(args.calls, 1)}
    for fn in cases.values():
        fn()
    torch.cuda.synchronize()
    vals = {c: [] for c in cases}
    for _ in range(args.rounds):
        for c, fn in cases.items():
            vals[c].append(timed(fn, reps.get(c, 10)))
    rows = []
    for kind, xs in vals.items():
        med = statistics.median(xs)
        rows.append(dict(shape=args.shape, n_envs=n, piles=piles, T=T, rows=R, kind=kind, unit="us_per_call", rounds=len(xs), median=round(med, 2),
                         min=round(min(xs), 2), max=round(max(xs), 2), gb_per_s_useful=round(meta[kind]["bytes_useful"] / med / 1e3, 1),
                         gb_per_s_lines=round(meta[kind]["bytes_lines"] / med / 1e3, 1), build_id=build_id, **meta[kind]))
    for row_ in rows:
        print(json.dumps(row_), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)
    torch.cuda.synchronize()
    for lag, *_ in keep:
        lag.close()
    env.close()


def return_norm_cases(args):
    """--return-norm: the reward scaling's launches beside the parent's reward GAE, on one collected rollout"""
    n_s, piles_s = args.shape.split("x")
    n, piles = int(n_s), [int(x) for x in piles_s.split(",")]
    T = 96
    env = chub.TorchHubVecEnv(n, piles, ["fast", "slow"], seed=1, rng="philox", autoreset="per_env", hydro_prod_rate=100.0, hydro_store_vlt=25.0,
                              init_soc=0.2, fc_max_power=100.0, fcev_permeate=0.01)
    build_id = chub.load_library().chub_build_id().decode()
    D, A = env.obs_dim, env.act_dim
    torch.manual_seed(0)
    lin = lambda i, o: torch.nn.Sequential(torch.nn.Linear(i, 64), torch.nn.Tanh(), torch.nn.Linear(64, o)).to("cuda")
    pol = env.load_policy(lin(D, A))
    pol.set_exploration(7, [-0.5, -0.5])
    crit = env.load_critic(lin(D, 1))
    env.reset()
    ro = env.collect(pol, T, logp_piles="decidable")
    values, final = env.values(crit, ro)
    R = T * n
    row = (D + 2) * 4
    lines = lambda stride, used: min(stride, 64 * ((used + 63) // 64 + (1 if stride % 64 else 0)))  # bytes of a strided row its reads touch, at most

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3  # us

    cases, meta = {}, {}
    gae_bytes = dict(bytes_useful=R * (8 + 4 + 4 + 4), bytes_lines=R * (lines(row, 8) + 12))
    cases["gae_reward"] = lambda: env.advantages(ro, values, final, stats=True)
    meta["gae_reward"] = dict(route="chub_rollout_gae_device with d_ret and d_stats", **gae_bytes)
    rn = None
    if os.environ.get("CHUB_LIB"):
        try:
            rn = env.make_reward_normalizer()
        except chub._lib.ChubError:  # (the parent's library: the unscaled call alone)
            rn = None
    else:
        rn = env.make_reward_normalizer()
    if rn is not None:
        cases["gae_scaled"] = lambda: env.advantages(ro, values, final, stats=True, reward_norm=rn)
        meta["gae_scaled"] = dict(route="chub_return_norm_gae_device with d_ret and d_stats", **gae_bytes)
        cases["return_norm_update"] = lambda: env.update_reward_normalizer(ro, rn)
        meta["return_norm_update"] = dict(route="chub_return_norm_update_device: the moments launch and its merge", bytes_useful=R * 8 + n * 8,
                                          bytes_lines=R * lines(row, 8) + n * 8)
        reward, done = ro["reward"], ro["done"]
        carry = torch.zeros((n,), dtype=torch.float32, device=env.device)
        gs = torch.zeros((T, n), dtype=torch.float32, device=env.device)
        zero = torch.zeros((), dtype=torch.float32, device=env.device)

        def same_in_torch():
            g = carry
            for t in range(T):
                g = 0.99 * g + reward[t]
                gs[t] = g
                g = torch.where(done[t] != 0, zero, g)
            carry.copy_(g)
            var = gs.double().var(unbiased=False)
            return torch.clamp(reward * (1.0 / torch.sqrt(var + 1e-8)).float(), -10.0, 10.0)

        cases["return_norm_torch"] = same_in_torch
        meta["return_norm_torch"] = dict(route="the update's arithmetic and the scaled, clipped reward as eager torch (its temporaries included)",
                                         bytes_useful=R * 8 + n * 8 + R * 4, bytes_lines=R * lines(row, 8) + n * 8 + R * 4)
    for fn in cases.values():
        fn()
    torch.cuda.synchronize()
    vals = {c: [] for c in cases}
    for _ in range(args.rounds):
        for c, fn in cases.items():
            vals[c].append(timed(fn, 2 if c == "return_norm_torch" else 10))
    rows = []
    for kind, xs in vals.items():
        med = statistics.median(xs)
        rows.append(dict(shape=args.shape, n_envs=n, piles=piles, T=T, rows=R, kind=kind, unit="us_per_call", rounds=len(xs), median=round(med, 2),
                         min=round(min(xs), 2), max=round(max(xs), 2), gb_per_s_useful=round(meta[kind]["bytes_useful"] / med / 1e3, 1),
                         gb_per_s_lines=round(meta[kind]["bytes_lines"] / med / 1e3, 1), build_id=build_id, lib=os.environ.get("CHUB_LIB", ""),
                         **meta[kind]))
    for row_ in rows:
        print(json.dumps(row_), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)
    torch.cuda.synchronize()
    if rn is not None:
        rn.close()
    env.close()


if __name__ == "__main__":
    main()
