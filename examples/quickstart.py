#!/usr/bin/env python3
"""Seven ways to drive the hub, smallest first (run from the repo root on a machine with an MI355X):

    python examples/quickstart.py

1. the drop-in single env (the reference's class and call pattern, test/env_test.py);
2. the batched host-pointer API (numpy in / numpy out);
3. the device-resident API (torch CUDA tensors in / out, no host copies) -- what an on-device learner should use;
4. a closed-loop day with an actor evaluated by the hub itself (numpy and ctypes only: no torch, no host between the steps);
5. on-policy training data: the hub samples from the actor, and keeps actions, log-probabilities and every step's block on the device;
6. one PPO-shaped iteration on that data: log-probabilities over the piles the step can see, a torch critic, advantages on the device;
7. one evolution-strategies generation, no backward pass: a population of perturbed actors on one handle, a closed-loop day for all of
   them at once, member fitness from the episode ledger, the ES gradient from regenerated noise, an SGD step on the centre;
8. one PPO epoch with the actor's gradient from the device (a torch critic beside it);
9. one complete PPO iteration in which torch does nothing but the two optimiser steps: collect -> values -> advantages -> minibatches of
   the actor's and the critic's gradients from the device -> the stepped weights of both networks straight back;
10. PPO epochs with no torch optimiser: Adam and the minibatch shuffle on the device, the epoch recorded once and replayed;
11. three PPO iterations whose update is ONE call with target_kl, and the numbers stable-baselines3 prints read once per iteration;
12. three PPO-Lagrangian iterations: the grid draw over the limit and the tank's end-of-day penalty as constraints, their multipliers,
    cost advantages and the combined advantage on the device, one cost critic per constraint;
13. part 11's three iterations with the reward scaled by the running spread of the discounted return (VecNormalize's norm_reward): the
    statistics, the scale and the scaled advantages stay on the device.
"""
import os
import sys
import time

import numpy as np

try:
    import torch  # before libchub is loaded (part 3 shares torch's HIP runtime); parts 1 and 2 do not need it
except ImportError:
    torch = None

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HUB = dict(station_list=[20, 25], station_type_list=["fast", "slow"], hydro_prod_rate=100, hydro_store_vlt=25,
           init_soc=0.2, fc_max_power=100, fcev_permeate=0.01)


def single_env():
    import charginghub_env_amd as chub

    env = chub.make("evcssp_env_cpp:charging-hub-v6", constant_charging=False, seed_rand=False, **HUB)
    env.reset()
    done, ret = False, 0.0
    while not done:
        obs, reward, done, info = env.step(action=None)      # None = every pile on, as in the reference's smoke test
        ret += reward
    print("1. drop-in env: one episode, return %.4f, observation %s" % (ret, np.round(obs, 3)))
    env.close()


def batched_host(n=4096):
    import charginghub_env_amd as chub

    hub = chub.VecChargingHub(n, seed=0, **HUB)
    obs = hub.reset()
    rs = np.random.RandomState(0)
    batches = [rs.uniform(-1, 1, (n, hub.act_dim)).astype(np.float32) for _ in range(8)]   # a policy would produce these
    t0 = time.perf_counter()
    for t in range(96):
        obs, reward, done, _ = hub.step(batches[t % 8])
    dt = time.perf_counter() - t0
    print("2. %d envs through numpy: %.1f M env-steps/s, mean reward %.4f, all done: %s"
          % (n, n * 96 / dt / 1e6, reward.mean(), bool(done.all())))
    # every reference env owns its clock: any subset can start a new day (or move) on its own
    obs = hub.reset()
    for t in range(30):
        obs, reward, done, _ = hub.step(rs.uniform(-1, 1, (n, hub.act_dim)).astype(np.float32))
    obs = hub.reset_envs(np.arange(n) % 2 == 0)              # half of the envs abandon their day
    obs, reward, done, _ = hub.step(rs.uniform(-1, 1, (n, hub.act_dim)).astype(np.float32))
    print("   per-env clocks: slots of day now %s (%d clocks)" % (sorted(set(hub.env_clocks().tolist())), hub.clock_groups))
    hub.close()
    # differently built hubs in one handle: any of the eight hydrogen / FCEV / fluctuation kwargs may be one value per env
    kw = dict(HUB, hydro_store_vlt=rs.uniform(5, 400, n), init_soc=rs.uniform(0.1, 1, n))
    hub = chub.VecChargingHub(n, seed=0, **kw)
    hub.reset()
    for t in range(48):
        obs, reward, done, _ = hub.step(batches[t % 8])
    redo = rs.uniform(size=n) < 0.25                          # domain randomisation: new tanks for a quarter of the envs ...
    hub.set_env_params(mask=redo, hydro_store_vlt=rs.uniform(5, 400, n), renew_fluctuate=0.3)
    obs = hub.reset_envs(redo)                                # ... which start a new day with them
    print("   per-env parameters: tank sizes %.0f .. %.0f m^3, mean reward %.4f"
          % (hub.env_params()["hydro_store_vlt"].min(), hub.env_params()["hydro_store_vlt"].max(), reward.mean()))
    hub.close()


def device_resident(n=65536):
    import charginghub_env_amd as chub

    if torch is None:
        print("3. skipped: torch is not installed")
        return

    env = chub.TorchHubVecEnv(n, seed=0, pile_obs=("car", "emergency"), station_profile=dict(fields=("cars", "power"), buckets=8), **HUB)
    obs = env.reset()
    actions = torch.rand((n, env.act_dim), device="cuda") * 2 - 1
    for _ in range(96):
        env.step(actions)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps = 960
    for _ in range(steps):
        obs, reward, done, _ = env.step(actions)             # a policy would map obs -> actions here, on the device
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("3. %d envs on the device: %.0f M env-steps/s, mean reward %.4f" % (n, n * steps / dt / 1e6, float(reward.mean())))
    # a policy that emits on / off decisions hands over one bit per pile (+ the two tail floats) instead of a row of floats
    bits, tail = env.pack_bits(actions)
    t0 = time.perf_counter()
    for _ in range(steps):
        obs, reward, done, _ = env.step_bits(bits, tail)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("   the same decisions as bits: %.0f M env-steps/s" % (n * steps / dt / 1e6))
    # a per-pile policy sees every pile (Station::situation): [n, columns, piles] on the device, here "charge whoever is urgent"
    piles = env.pile_obs()
    car, emergency = piles[:, 0], piles[:, 1]
    urgent = actions.clone()
    urgent[:, :env.act_dim - 2] = torch.where((car > 0) & (emergency >= 0.25), 1.0, -1.0)
    obs, reward, done, _ = env.step(urgent)
    print("   per-pile columns %s: %.1f cars per env, %.1f of them urgent" % (env.pile_names, float(car.sum(1).mean()),
                                                                             float(((car > 0) & (emergency >= 0.25)).sum(1).float().mean())))
    # a station-level policy sees who is due by when, [n, 2, columns, buckets] whatever the hub's size; here the kW of the cars due within
    # two slots, per station: an action row of the scalar-load control (VecChargingHub.step_load*)
    load = env.station_profile()[:, :, 1, :2].sum(-1)
    print("   station profiles %s: %.1f kW per station due within two slots" % (env.profile_names, float(load.mean())))
    # population-based selection without leaving the device: the worst tenth becomes a copy of the best tenth (each clone keeps its own
    # random streams, so it parts from its source at the next step)
    k = max(1, n // 10)
    best, worst = torch.topk(reward, k).indices, torch.topk(reward, k, largest=False).indices
    env.copy_envs(best, worst)
    obs, reward, done, _ = env.step(actions)
    print("   best %d copied over worst %d: mean reward of the next step %.4f" % (k, k, float(reward.mean())))
    env.close()


def closed_loop(n=4096):
    import charginghub_env_amd as chub
    from charginghub_env_amd import multi_gpu

    hub = chub.VecChargingHub(n, seed=0, **HUB)
    D, A = hub.obs_dim, hub.act_dim
    rs = np.random.RandomState(0)
    sizes = [D, 64, 64, A]                                   # a small random actor; a trained one hands over its nn.Linear weights
    layers = [((rs.normal(size=(o, i)) / np.sqrt(i)).astype(np.float32), np.zeros(o, dtype=np.float32)) for i, o in zip(sizes[:-1], sizes[1:])]
    policy = hub.make_policy(layers)                         # exact f32 on the matrix cores: the trainer's network up to summation order
    packed = [multi_gpu.DeviceBuffer(n * (D + 2) * 4) for _ in range(2)]
    reset_obs = multi_gpu.DeviceBuffer(n * D * 4)
    t0 = time.perf_counter()
    policy.run_steps([b.ptr for b in packed], 96, d_reset_obs=reset_obs.ptr)   # reset + 96 x (actor, step), issued from C
    hub.sync()
    dt = time.perf_counter() - t0
    last = packed[95 & 1].to_host(np.float32, (n, D + 2))    # obs, reward, done of the day's last step
    print("4. %d envs, a 13-64-64-47 actor on the device, one closed-loop day: %.1f M env-steps/s, mean reward %.4f, all done: %s"
          % (n, n * 96 / dt / 1e6, last[:, D].mean(), bool((last[:, D + 1] > 0.5).all())))
    policy.close()
    hub.close()


def on_policy_data(n=4096, steps=32):
    import charginghub_env_amd as chub

    if torch is None:
        print("5. skipped: torch is not installed")
        return
    env = chub.TorchHubVecEnv(n, seed=0, autoreset="per_env", **HUB)
    D, A = env.obs_dim, env.act_dim
    net = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, A)).to("cuda")
    log_std = torch.full((2,), -0.5, device="cuda")
    policy = env.load_policy(net)
    policy.set_exploration(key=7, log_std=log_std.cpu().numpy())   # the noise's key and the scale of the two tail actions
    env.reset()
    ro = env.collect(policy, steps)                           # sampled actions, their log-probabilities and every step's block, kept
    new = chub.wrappers.sampled_logp(net(ro["features"]), ro["bits"], ro["u"], log_std)   # the new policy's term, differentiable
    ratio = torch.exp(new - ro["logp"]).detach()              # (a loss would keep the graph: PPO's clipped surrogate is built on this)
    print("5. %d envs x %d sampled steps kept on the device: mean reward %.4f, mean log-probability %.2f, importance ratio %.5f .. %.5f"
          % (n, steps, float(ro["reward"].mean()), float(ro["logp"].mean()), float(ratio.min()), float(ratio.max())))
    env.close()


def ppo_iteration(n=4096, steps=64):
    import charginghub_env_amd as chub

    if torch is None:
        print("6. skipped: torch is not installed")
        return
    env = chub.TorchHubVecEnv(n, seed=0, autoreset="per_env", **HUB)
    D, A = env.obs_dim, env.act_dim
    net = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, A)).to("cuda")
    critic = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1)).to("cuda")
    log_std = torch.full((2,), -0.5, device="cuda", requires_grad=True)
    opt = torch.optim.Adam(list(net.parameters()) + list(critic.parameters()) + [log_std], lr=3e-4)
    policy = env.load_policy(net)
    policy.set_exploration(key=7, log_std=log_std.detach().cpu().numpy())
    env.reset()
    # the step ignores a pile's bit where the pile is empty or its car is forced on: only the decidable piles' terms enter logp
    ro = env.collect(policy, steps, logp_piles="decidable")
    with torch.no_grad():                                    # the critic on obs0 and on every block's observation: one batched call each
        values = torch.cat([critic(ro["obs0"]).reshape(1, n), critic(ro["packed"][:, :, :D]).reshape(steps, n)]).contiguous()
        final = critic(env.last_obs).reshape(n).contiguous()  # the terminal observations of the envs whose day ended in the rollout
    adv, ret, stats = env.advantages(ro, values, final, gamma=0.99, lam=0.95, stats=True)   # one launch; count, sum, sum of squares beside
    mean = stats[1] / stats[0]
    std = (stats[2] / stats[0] - mean * mean).clamp_min(1e-12).sqrt()
    a = ((adv - mean) / std).float()
    z = net(ro["features"])
    new = chub.wrappers.sampled_logp(z, ro["bits"], ro["u"], log_std, piles=ro["set_bits"])
    ratio = torch.exp(new - ro["logp"])
    surrogate = torch.min(ratio * a, ratio.clamp(0.8, 1.2) * a).mean()
    entropy = chub.wrappers.sampled_entropy(z, log_std, piles=ro["set_bits"]).mean()
    value_loss = (critic(ro["features"]).reshape(steps, n) - ret).pow(2).mean()
    loss = -surrogate + 0.5 * value_loss - 0.01 * entropy
    opt.zero_grad()
    loss.backward()
    opt.step()
    sets = ro["set_bits"]
    decidable = sum(((sets >> b) & 1).sum() for b in range(env.vec.n_slots)) / float(sets.shape[0] * n) if sets.shape[-1] == 1 else float("nan")
    print("6. %d envs x %d steps, one PPO iteration: %.1f of %d piles decidable per step, importance ratio %.5f .. %.5f, advantage std %.3f, loss %.4f"
          % (n, steps, float(decidable), env.vec.n_slots, float(ratio.min()), float(ratio.max()), float(std), float(loss.detach())))
    for l, m in enumerate(x for x in net if isinstance(x, torch.nn.Linear)):   # the stepped weights, on the device, for the next collect
        policy.set_weights_device(l, m.weight.data_ptr(), m.bias.data_ptr(), torch.cuda.current_stream().cuda_stream)
    policy.set_log_std_device(log_std.data_ptr(), torch.cuda.current_stream().cuda_stream)
    env.close()


def es_generation(n=4096, members=64, sigma=0.05, lr=0.02, generation=0):
    import charginghub_env_amd as chub

    if torch is None:
        print("7. skipped: torch is not installed")
        return
    env = chub.TorchHubVecEnv(n, seed=0, autoreset="per_env", episode_stats=True, **HUB)
    D, A = env.obs_dim, env.act_dim
    net = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, A), torch.nn.Tanh()).to("cuda")   # the centre
    linears = [m for m in net if isinstance(m, torch.nn.Linear)]
    policy = env.load_policy(net)
    pop = env.load_population(policy, members, key=7)         # member m acts for envs [m E, (m + 1) E), E = n / members
    stream = torch.cuda.current_stream().cuda_stream
    # members 2j / 2j + 1 = theta + / - sigma eps_j, drawn on the device from the centre's own tensors; the noise is never stored
    pop.perturb_device(sigma, generation, [m.weight.data_ptr() for m in linears], [m.bias.data_ptr() for m in linears], stream=stream)
    env.reset()
    env.population_rollout(pop, 96)                           # one closed-loop day, every member at once: one actor launch per step
    fitness = env.episode_stats()["return"].view(members, -1).mean(dim=1)   # the day's return per env, viewed as [P][E]
    ranks = fitness.argsort().argsort().float()
    util = (ranks / (members - 1) - 0.5).contiguous()         # centred ranks: the trainer's choice of fitness shaping
    grads = env.es_gradient(pop, util, generation)            # sum_j (u[2j] - u[2j + 1]) eps_j, the noise regenerated: nn.Linear shapes
    with torch.no_grad():                                     # plain SGD ascent on the centre; 1 / (P sigma) is the estimator's scale
        for m, (gW, gb) in zip(linears, grads):
            m.weight.add_(lr / (members * sigma) * gW)
            m.bias.add_(lr / (members * sigma) * gb)
    for l, m in enumerate(linears):                           # the centre policy follows, for evaluation and the next generation
        policy.set_weights_device(l, m.weight.data_ptr(), m.bias.data_ptr(), stream)
    print("7. %d envs, %d members x %d envs, one ES generation of %d parameters: fitness %.3f .. %.3f, gradient norm %.3f"
          % (n, members, n // members, pop.n_params, float(fitness.min()), float(fitness.max()),
             float(torch.sqrt(sum((gW ** 2).sum() + (gb ** 2).sum() for gW, gb in grads)))))
    env.close()


def ppo_on_device_gradients(n=4096, steps=64, minibatches=4):
    import charginghub_env_amd as chub

    if torch is None:
        print("8. skipped: torch is not installed")
        return
    env = chub.TorchHubVecEnv(n, seed=0, autoreset="per_env", **HUB)
    D, A = env.obs_dim, env.act_dim
    net = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, A)).to("cuda")   # holds the weights; never run
    linears = [m for m in net if isinstance(m, torch.nn.Linear)]
    critic = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1)).to("cuda")
    log_std = torch.full((2,), -0.5, device="cuda")
    params = [p for m in linears for p in (m.weight, m.bias)] + [log_std]
    opt = torch.optim.Adam(params, lr=3e-4)                    # the optimiser stays with the trainer; the actor needs no autograd
    policy = env.load_policy(net)
    policy.set_exploration(key=7, log_std=log_std.cpu().numpy())
    stream = torch.cuda.current_stream().cuda_stream
    env.reset()
    ro = env.collect(policy, steps, logp_piles="decidable")
    with torch.no_grad():
        values = torch.cat([critic(ro["obs0"]).reshape(1, n), critic(ro["packed"][:, :, :D]).reshape(steps, n)]).contiguous()
        final = critic(env.last_obs).reshape(n).contiguous()
    adv, ret, adv_stats = env.advantages(ro, values, final, gamma=0.99, lam=0.95, stats=True)
    perm = torch.randperm(steps * n, device="cuda")
    clipped = 0.0
    for rows in perm.chunk(minibatches):                     # a minibatch is a list of flat (step, env) indices into the rollout
        # the CURRENT weights' log-probabilities of the recorded actions, the clipped surrogate and its gradient: a handful of launches
        grads, g_log_std, stats = env.policy_gradient(ro, adv, rows=rows.contiguous(), loss="ppo_clip", clip_eps=0.2, ent_coef=0.01,
                                                      adv_stats=adv_stats)
        for m, (gW, gb) in zip(linears, grads):                # the returned tensors ARE the gradients, in nn.Linear's layout
            m.weight.grad, m.bias.grad = gW, gb
        log_std.grad = g_log_std
        opt.step()
        for l, m in enumerate(linears):                        # the stepped weights go straight back: the next minibatch differentiates them
            policy.set_weights_device(l, m.weight.data_ptr(), m.bias.data_ptr(), stream)
        policy.set_log_std_device(log_std.data_ptr(), stream)
        clipped = clipped + stats[4] / stats[0]
    logp_new, entropy = env.evaluate_actions(ro)              # the forward alone, under the weights as they are now
    kl = float((ro["logp"].reshape(-1) - logp_new).mean())
    print("8. %d envs x %d steps, one PPO epoch in %d minibatches with the actor's gradient from the device: clipped away %.3f of the rows, "
          "approximate KL %.5f, mean entropy %.2f" % (n, steps, minibatches, float(clipped) / minibatches, kl, float(entropy.mean())))
    env.close()


def ppo_all_on_device(n=4096, steps=64, minibatches=4):
    import charginghub_env_amd as chub

    if torch is None:
        print("9. skipped: torch is not installed")
        return
    env = chub.TorchHubVecEnv(n, seed=0, autoreset="per_env", **HUB)
    D, A = env.obs_dim, env.act_dim
    net = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, A)).to("cuda")      # hold the weights; never run
    vnet = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1)).to("cuda")
    a_lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    c_lin = [m for m in vnet if isinstance(m, torch.nn.Linear)]
    log_std = torch.full((2,), -0.5, device="cuda")
    a_opt = torch.optim.Adam([p for m in a_lin for p in (m.weight, m.bias)] + [log_std], lr=3e-4)
    c_opt = torch.optim.Adam([p for m in c_lin for p in (m.weight, m.bias)], lr=1e-3)
    policy = env.load_policy(net)
    policy.set_exploration(key=7, log_std=log_std.cpu().numpy())
    critic = env.load_critic(vnet)                             # the same nn.Sequential forms; its rows are the actor's feature rows
    stream = torch.cuda.current_stream().cuda_stream
    env.reset()
    ro = env.collect(policy, steps, logp_piles="decidable")
    values, final = env.values(critic, ro)                     # V over the whole rollout in one launch, V of the state now, V of last_obs
    adv, ret, adv_stats = env.advantages(ro, values, final, gamma=0.99, lam=0.95, stats=True)
    v_old = values[:steps].clone()                             # the values as collected: the centre of the clipped value loss
    clipped = v_clipped = 0.0
    for rows in torch.randperm(steps * n, device="cuda").chunk(minibatches):
        rows = rows.contiguous()
        grads, g_log_std, stats = env.policy_gradient(ro, adv, rows=rows, loss="ppo_clip", clip_eps=0.2, ent_coef=0.01, adv_stats=adv_stats)
        v_grads, v_stats = env.value_gradient(critic, ro, ret, rows=rows, loss="clipped", clip_eps=0.2, v_old=v_old)
        for m, (gW, gb) in zip(a_lin, grads):                  # the returned tensors ARE the gradients, in nn.Linear's layout
            m.weight.grad, m.bias.grad = gW, gb
        log_std.grad = g_log_std
        for m, (gW, gb) in zip(c_lin, v_grads):
            m.weight.grad, m.bias.grad = gW, gb
        a_opt.step()                                           # torch's whole part of the iteration: these two lines
        c_opt.step()
        for l, m in enumerate(a_lin):                          # the stepped weights go straight back, for both networks
            policy.set_weights_device(l, m.weight.data_ptr(), m.bias.data_ptr(), stream)
        policy.set_log_std_device(log_std.data_ptr(), stream)
        for l, m in enumerate(c_lin):
            critic.set_weights_device(l, m.weight.data_ptr(), m.bias.data_ptr(), stream)
        clipped, v_clipped = clipped + stats[4] / stats[0], v_clipped + v_stats[2] / v_stats[0]
    _, st = env.value_gradient(critic, ro, ret)                # explained variance from the call's own sums: 1 - E(ret - v)^2 / Var ret
    ev = 1.0 - (st[3] / st[0]) / (st[5] / st[0] - (st[4] / st[0]) ** 2).clamp_min(1e-12)
    print("9. %d envs x %d steps, one PPO iteration with both gradients from the device: clipped away %.3f of the actor's rows and %.3f of "
          "the critic's, value loss %.4f, explained variance %.3f" % (n, steps, float(clipped) / minibatches, float(v_clipped) / minibatches,
                                                                     float(st[1] / st[0]), float(ev)))
    env.close()


def ppo_epochs_on_device(n=4096, steps=64, minibatches=4, epochs=4):
    import charginghub_env_amd as chub

    if torch is None:
        print("10. skipped: torch is not installed")
        return
    env = chub.TorchHubVecEnv(n, seed=0, autoreset="per_env", **HUB)
    D, A = env.obs_dim, env.act_dim
    net = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, A)).to("cuda")      # receive the weights at the end
    vnet = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1)).to("cuda")
    policy = env.load_policy(net)
    policy.set_exploration(key=7, log_std=[-0.5, -0.5])
    critic = env.load_critic(vnet)
    a_opt = env.make_optimizer(policy, lr=3e-4, max_grad_norm=0.5)    # Adam on the LIVE device weights (and log_std): no torch optimiser,
    c_opt = env.make_optimizer(critic, lr=1e-3, max_grad_norm=0.5)    # no set_weights_device after a step
    env.reset()
    ro = env.collect(policy, steps, logp_piles="decidable")
    values, final = env.values(critic, ro)
    adv, ret, adv_stats = env.advantages(ro, values, final, gamma=0.99, lam=0.95, stats=True)
    v_old = values[:steps].clone()
    R = steps * n
    mb = R // minibatches

    def epoch():
        # a permutation of the rollout's rows that is never stored apart from its output; its counter is the actor optimiser's step
        # count, read on the device when the launch runs, so that every epoch -- every replay -- shuffles anew
        rows = env.shuffle_rows(R, key=11, counter=a_opt)
        for i in range(minibatches):
            r = rows[i * mb:(i + 1) * mb]
            env.policy_gradient(ro, adv, rows=r, loss="ppo_clip", clip_eps=0.2, ent_coef=0.01, adv_stats=adv_stats, into=a_opt)
            env.value_gradient(critic, ro, ret, rows=r, loss="clipped", clip_eps=0.2, v_old=v_old, into=c_opt)
            env.optimizer_step(a_opt)                          # the gradients lie in the optimisers' own buffers: two launches each
            env.optimizer_step(c_opt)

    epoch()                                                    # once eagerly: every tensor the calls cache exists before the recording
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                              # the M-minibatch epoch as one chain of launches, recorded once
        epoch()
    for _ in range(epochs - 1):                                # each replay continues from the weights, moments and counter of the last
        graph.replay()
    a_stats = env.optimizer_stats(a_opt)                       # of the last step: t, the gradient's norm, the clip scale, skipped
    (layers, log_std), v_layers = env.policy_weights(policy), env.critic_weights(critic)
    with torch.no_grad():                                      # the trained weights back into the nn.Sequentials, in nn.Linear's layout
        for m, (W, b) in zip([m for m in net if isinstance(m, torch.nn.Linear)], layers):
            m.weight.copy_(W), m.bias.copy_(b)
        for m, (W, b) in zip([m for m in vnet if isinstance(m, torch.nn.Linear)], v_layers):
            m.weight.copy_(W), m.bias.copy_(b)
    logp_new, entropy = env.evaluate_actions(ro)
    kl = float((ro["logp"].reshape(-1) - logp_new).mean())
    print("10. %d envs x %d steps, %d PPO epochs of %d minibatches with no torch optimiser, the epoch recorded once and replayed: %d Adam steps, "
          "last gradient norm %.3f (clip scale %.3f), approximate KL %.5f, log_std %s"
          % (n, steps, epochs, minibatches, int(a_stats[0]), float(a_stats[1]), float(a_stats[2]), kl, [round(float(x), 4) for x in log_std]))
    env.close()


def ppo_with_log_and_target_kl(n=4096, steps=64, minibatches=4, epochs=4, iterations=3):
    import charginghub_env_amd as chub

    if torch is None:
        print("11. skipped: torch is not installed")
        return
    env = chub.TorchHubVecEnv(n, seed=0, autoreset="per_env", **HUB)
    D, A = env.obs_dim, env.act_dim
    net = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, A)).to("cuda")
    vnet = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1)).to("cuda")
    policy = env.load_policy(net)
    policy.set_exploration(key=7, log_std=[-0.5, -0.5])
    critic = env.load_critic(vnet)
    a_opt = env.make_optimizer(policy, lr=3e-4, max_grad_norm=0.5)
    c_opt = env.make_optimizer(critic, lr=1e-3, max_grad_norm=0.5)
    log = env.make_train_log()                                 # thirty f64 words and a gate word on the device
    env.reset()
    for it in range(iterations):
        ro = env.collect(policy, steps, logp_piles="decidable")
        values, final = env.values(critic, ro)
        adv, ret, adv_stats = env.advantages(ro, values, final, gamma=0.99, lam=0.95, stats=True)
        v_old = values[:steps].clone()
        # the whole update in one call: per epoch a shuffle, per minibatch two gradients, the log's record, two steps, the log's steps.
        # The first minibatch whose approximate KL passes 1.5 * target_kl (stable-baselines3's rule) closes the gate: no later step is taken
        env.ppo_update(ro, adv, ret, a_opt, c_opt, epochs=epochs, minibatch_rows=steps * n // minibatches, key=11 + it, clip_eps=0.2,
                       ent_coef=0.01, v_old=v_old, adv_stats=adv_stats, target_kl=0.02, log=log)
        s = env.train_log_summary(log)                         # the iteration's one read-back
        print("11. iteration %d: %d minibatches counted%s, approx_kl %.5f (max %.5f), clip_fraction %.3f, entropy %.3f, policy_loss %.4f, "
              "value_loss %.4f, explained_variance %.3f, actor steps %d (held back %d, clipped %d), grad norm %.3f"
              % (it, s["n_minibatches"], "" if s["stopped_at"] is None else ", stopped at %d" % s["stopped_at"], s["approx_kl"], s["approx_kl_max"],
                 s["clip_fraction"], s["entropy"], s["policy_loss"], s["value_loss"], s["explained_variance"], s["policy_opt"]["steps"],
                 s["policy_opt"]["held_back"], s["policy_opt"]["clipped_steps"], s["policy_opt"]["grad_norm_mean"]))
    env.close()


def ppo_lagrangian(n=4096, steps=64, minibatches=4, epochs=2, iterations=3):
    import charginghub_env_amd as chub

    if torch is None:
        print("12. skipped: torch is not installed")
        return
    env = chub.TorchHubVecEnv(n, seed=0, autoreset="per_env", **HUB)
    D, A = env.obs_dim, env.act_dim
    mlp = lambda out: torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, out)).to("cuda")
    policy = env.load_policy(mlp(A))
    policy.set_exploration(key=7, log_std=[-0.5, -0.5])
    critic = env.load_critic(mlp(1))
    a_opt = env.make_optimizer(policy, lr=3e-4, max_grad_norm=0.5)
    c_opt = env.make_optimizer(critic, lr=1e-3, max_grad_norm=0.5)
    # two constraints on an episode's cost: the energy drawn over the grid limit, summed over the day, and the tank's end-of-day
    # penalty (the reference's test_penalty).  Each has a multiplier on the device and a cost critic of its own
    cons = env.make_constraints([dict(term="grid_excess", kind="step", limit=50.0, lr=1e-3),
                                 dict(term="soc_penalty", kind="done", limit=0.5, lr=0.05, lambda_max=10.0)])
    cost_critics = [env.load_critic(mlp(1)) for _ in range(cons.K)]
    cost_opts = [env.make_optimizer(c, lr=1e-3, max_grad_norm=0.5) for c in cost_critics]
    log = env.make_train_log()
    env.reset()
    for it in range(iterations):
        ro = env.collect(policy, steps, logp_piles="decidable", terms=cons.terms)   # the rollout keeps the constrained step terms
        values, final = env.values(critic, ro)
        adv, ret, adv_stats = env.advantages(ro, values, final, gamma=0.99, lam=0.95, stats=True)
        cost_vf = [tuple(t.clone() for t in env.values(c, ro)) for c in cost_critics]
        cost_advs, cost_rets = env.cost_advantages(ro, cons, cost_values=[v for v, _ in cost_vf], final_values=[f for _, f in cost_vf],
                                                   gamma=0.99, lam=0.95)          # every constraint in one pass, episode costs counted
        env.update_multipliers(cons)                                              # lambda += lr (J - limit), kept in [0, lambda_max]
        combined = env.constrained_advantages(adv, adv_stats, cost_advs, cons)    # (A - sum lambda_k A_k) / (1 + sum lambda_k)
        for c, opt, c_ret in zip(cost_critics, cost_opts, cost_rets):             # the cost critics: existing calls on the cost returns
            env.value_gradient(c, ro, c_ret, into=opt)
            env.optimizer_step(opt)
        env.ppo_update(ro, combined, ret, a_opt, c_opt, epochs=epochs, minibatch_rows=steps * n // minibatches, key=23 + it, clip_eps=0.2,
                       ent_coef=0.01, v_old=values[:steps].clone(), adv_stats=None, log=log)
        s = env.train_log_summary(log)
        print("12. iteration %d: policy_loss %.4f, approx_kl %.5f; %s" % (it, s["policy_loss"], s["approx_kl"], "; ".join(
            "%s (%s) lambda %.4f, episode cost %.3f over %d episodes against %.2f, steps %d, skipped %d"
            % (c["term"], c["kind"], c["lambda"], c["episode_cost_mean"], c["episodes"], c["limit"], c["steps"], c["skipped"])
            for c in env.constraint_summary(cons))))
    env.close()


def ppo_with_reward_scaling(n=4096, steps=64, minibatches=4, epochs=4, iterations=3):
    import charginghub_env_amd as chub

    if torch is None:
        print("13. skipped: torch is not installed")
        return
    env = chub.TorchHubVecEnv(n, seed=0, autoreset="per_env", **HUB)
    D, A = env.obs_dim, env.act_dim
    net = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, A)).to("cuda")
    vnet = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1)).to("cuda")
    policy = env.load_policy(net)
    policy.set_exploration(key=7, log_std=[-0.5, -0.5])
    critic = env.load_critic(vnet)
    a_opt = env.make_optimizer(policy, lr=3e-4, max_grad_norm=0.5)
    c_opt = env.make_optimizer(critic, lr=1e-3, max_grad_norm=0.5)
    log = env.make_train_log()
    rn = env.make_reward_normalizer(gamma=0.99, eps=1e-8, clip=10.0)   # the state [n, mean, M2], the scale and a carry per env, on the device
    scale = env.reward_scale(rn)                                        # a tensor over the object's own word: no read until it is printed
    env.reset()
    for it in range(iterations):
        ro = env.collect(policy, steps, logp_piles="decidable")
        values, final = env.values(critic, ro)
        env.update_reward_normalizer(ro, rn)                            # update first, then normalise, as VecNormalize does
        adv, ret, adv_stats = env.advantages(ro, values, final, gamma=0.99, lam=0.95, stats=True, reward_norm=rn)
        v_old = values[:steps].clone()
        env.ppo_update(ro, adv, ret, a_opt, c_opt, epochs=epochs, minibatch_rows=steps * n // minibatches, key=11 + it, clip_eps=0.2,
                       ent_coef=0.01, v_old=v_old, adv_stats=adv_stats, target_kl=0.02, log=log)
        s = env.train_log_summary(log)
        print("13. iteration %d: reward scale %.6g, value_loss %.4f, explained_variance %.3f, approx_kl %.5f, policy_loss %.4f"
              % (it, float(scale[0]), s["value_loss"], s["explained_variance"], s["approx_kl"], s["policy_loss"]))
    env.close()


if __name__ == "__main__":
    single_env()
    batched_host()
    device_resident()
    closed_loop()
    on_policy_data()
    ppo_iteration()
    es_generation()
    ppo_on_device_gradients()
    ppo_all_on_device()
    ppo_epochs_on_device()
    ppo_with_log_and_target_kl()
    ppo_lagrangian()
    ppo_with_reward_scaling()
