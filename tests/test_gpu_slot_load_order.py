"""The packed slot kernel's first loads (slot_body_packed, packed_records): a step requests the state words of all its slots first and
everything else behind them, from every lane -- a lane without a slot asks for the workgroup's first slot / env -- and the last wave's
lanes request the tail actions of the envs whose records they will write with those first loads (the first pass of packed_records:
unit i = lane, i.e. the workgroup's first 32 envs; the passes behind it read them in place).

Held to the CPU oracle call by call (slots and station records bit for bit, observation and reward to the f64 tail's 1e-9) over one day
plus a cut-short one, at the smallest shapes where either change can go wrong:
  * lanes without a slot and clamped addresses: hub [20, 25] (11 envs on the small tile's 512 virtual lanes, 17 lanes idle) with 1, 12
    (a second workgroup of one env) and 23 envs, on both tiles;
  * the first pass's bound from both sides: 16 piles (32 envs per workgroup: one pass exactly) and 15 piles (34 envs: two units in a second
    pass), and one pile (128 envs per workgroup: four passes), each with a partly filled last workgroup;
  * a station without piles ([16, 0]) and a hub whose action rows end unaligned ([3, 7]);
  * every kernel that compiles the same body: calls on a subset of the envs, one bit per pile, the one-launch step on a tail wave
    (hubs of 8 piles and more) and on the last slot wave (smaller hubs), spans of steps in one launch, a captured graph.
The actions are uniform random per env and step, the two tail floats included: another env's pair handed to the tail kernel shows in
the reward."""
import ctypes as C

import numpy as np
import pytest

from orclib import orc, ptr
from test_gpu_env_clocks import Pair
from test_gpu_parity import TIGHT, _oracle_vec, check_slots, close, hub

pytestmark = pytest.mark.gpu

HUB = dict(station_type_list=["fast", "slow"], hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2, fc_max_power=100.0,
           fcev_permeate=0.01, constant_charging=False, renew_fluctuate=0.3, price_fluctuate=0.3, hydro_loss=0.001)
SEED, ENV_ID0 = 0xFEED5EED, 4000
PLAN = (96, 10)  # one day, and one cut short by the next reset


class Run(Pair):
    """test_gpu_env_clocks.Pair (the handle and the oracle's envs, driven with the same calls and compared after each) with the
    constructor options that choose the launch form"""

    def __init__(self, piles, n, **options):
        chub = hub()
        kw = dict(HUB, station_list=list(piles))
        self.n, self.kw, self.slot_kernel, self.rng = n, kw, "auto", "philox"
        self.v = chub.VecChargingHub(n, seed=SEED, rng="philox", env_id0=ENV_ID0, **options, **kw)
        assert self.v.uses_packed_kernel
        self.v.set_telemetry(True)
        self.cfg, self.h = _oracle_vec(kw, n, ENV_ID0, SEED)
        self.D, self.A = self.v.obs_dim, self.v.act_dim
        self.o_obs = np.zeros((n, self.D))
        self.o_rew = np.zeros(n)
        self.o_done = np.zeros(n, dtype=np.int32)
        self.t = np.zeros(n, dtype=np.int64)
        self.rs = np.random.RandomState(11)

    def step_bits(self, label=""):
        """a lock-step chub_step_bits on thresholded pile actions (which the bits carry whole) and random tail floats"""
        S = sum(self.kw["station_list"])
        act = self.rs.uniform(-1, 1, size=(self.n, self.A)).astype(np.float32)
        act[:, :S] = np.where(act[:, :S] >= 0, np.float32(1), np.float32(-1))
        bits, tail = self.v.pack_actions(act)
        obs, rew, done, _ = self.v.step_bits(bits, tail)
        orc.orc_vec_step(self.h, ptr(act), None, ptr(self.o_obs), ptr(self.o_rew), ptr(self.o_done8), 1)
        assert np.array_equal(done, self.o_done8.astype(bool)), (label, "done")
        self._compare(np.arange(self.n), ("step_bits", label), True)
        close(obs, self.o_obs, (label, "obs f32"), atol=1e-6)


def lock_step_days(p):
    for ep, steps in enumerate(PLAN):
        p.reset(label=ep)
        for t in range(steps):
            p.step(label=(ep, t))
    assert orc.orc_vec_overflow(p.h) == 0
    p.close()


@pytest.mark.parametrize("tile", ["small", "large"])
@pytest.mark.parametrize("n", [1, 12, 23])
def test_lanes_without_a_slot(n, tile):
    """hub [20, 25]: 11 envs per 512 virtual lanes (45 envs per 2048), the other lanes -- and, in the last workgroup, the lanes of the envs
    past the batch's end -- request the workgroup's first slot and use nothing of it"""
    p = Run([20, 25], n, fused_step="off", tile=tile)
    assert not p.v.uses_fused_step
    lock_step_days(p)


@pytest.mark.parametrize("piles,n", [([9, 7], 70), ([8, 7], 70), ([1, 0], 130), ([16, 0], 70), ([3, 7], 77)],
                         ids=["16_piles_one_pass", "15_piles_two_passes", "one_pile_four_passes", "station_without_piles", "rows_end_unaligned"])
def test_tail_actions_from_registers_and_in_place(piles, n):
    """packed_records' first pass hands over the tail actions requested with the workgroup's first loads, the passes behind it read them
    where they did: 32 envs per workgroup (one pass), 34 (a second pass of two units), 128 (four passes) -- the last workgroup partly
    filled in each"""
    p = Run(piles, n, fused_step="off", tile="small")
    assert not p.v.uses_fused_step
    lock_step_days(p)


def test_calls_on_a_subset_of_the_envs():
    """chub_step_envs on a strict subset, then on everybody (the masked instantiation: the clock byte is requested right behind the state words)"""
    n = 23
    p = Run([20, 25], n, fused_step="off", tile="small")
    idx = np.arange(n)
    p.reset(label="all")
    for i in range(3):
        p.step(label=("lock-step", i))
    for i in range(12):
        p.step(idx % 3 == i % 3, ("a third", i))
        p.step(np.ones(n, dtype=bool), ("everybody, masked", i))
    p.step(idx >= 11, "the second workgroup and its neighbour alone")
    p.reset(idx % 2 == 0, "every other env")
    for i in range(6):
        p.step(label=("two clocks", i))
    assert orc.orc_vec_overflow(p.h) == 0
    p.close()


def test_one_bit_per_pile():
    """chub_step_bits: the bit words take the action rows' place among the first loads; the tail kernel reads the caller's own tail array"""
    p = Run([20, 25], 23, fused_step="off", tile="small")
    p.o_done8 = np.zeros(p.n, dtype=np.uint8)
    for ep, steps in enumerate(PLAN):
        p.reset(label=ep)
        for t in range(steps):
            p.step_bits(label=(ep, t))
    p.close()


@pytest.mark.parametrize("piles,n,fused", [([20, 25], 23, "on"), ([20, 25], 23, "off"), ([3, 2], 230, "on")],
                         ids=["tail_wave", "two_launches", "last_slot_wave"])
def test_one_launch_step(piles, n, fused):
    """fused_step on: the body inside k_step_tailwave (the tails on a wave of their own) and, for hubs of fewer than 8 piles, inside
    k_step_fused (102 envs per workgroup here); off: the same handle arguments on k_slot_packed + k_env"""
    p = Run(piles, n, fused_step=fused)
    assert p.v.uses_fused_step == (fused == "on")
    lock_step_days(p)


@pytest.mark.parametrize("piles,n", [([20, 25], 23), ([3, 2], 230)], ids=["tails_on_their_own_wave", "tails_on_the_last_slot_wave"])
def test_a_span_of_steps_in_one_launch(piles, n):
    """chub_run_steps with spans of 24 steps (k_steps_piped / k_steps_fused): a day, a reset and 10 steps more, the end state against the
    oracle stepped with the same action batches"""
    chub = hub()
    from charginghub_env_amd import multi_gpu
    from charginghub_env_amd._lib import check
    kw = dict(HUB, station_list=list(piles))
    v = chub.VecChargingHub(n, seed=SEED, rng="philox", env_id0=ENV_ID0, fused_step="on", span_steps=24, **kw)
    assert v.uses_packed_kernel and v.uses_fused_step
    cfg, h = _oracle_vec(kw, n, ENV_ID0, SEED)
    D, A = v.obs_dim, v.act_dim
    rs = np.random.RandomState(3)
    host = [rs.uniform(-1, 1, size=(n, A)).astype(np.float32) for _ in range(5)]
    acts = [multi_gpu.DeviceBuffer(n * A * 4) for _ in host]
    for a, x in zip(acts, host):
        a.from_host(x)
    packed = [multi_gpu.DeviceBuffer(n * (D + 2) * 4) for _ in range(2)]
    obs0 = multi_gpu.DeviceBuffer(n * D * 4)
    c_acts = (C.c_void_p * len(acts))(*[a.ptr for a in acts])
    c_packed = (C.c_void_p * 2)(packed[0].ptr, packed[1].ptr)
    total = sum(PLAN)
    check(v._lib.chub_run_steps(v._h, None, c_acts, len(acts), c_packed, None, obs0.ptr, 0, total, None))
    v.sync()
    o_obs, o_rew, o_done = np.zeros((n, D)), np.zeros(n), np.zeros(n, dtype=np.uint8)
    for i in range(total):
        if i % 96 == 0:
            orc.orc_vec_reset(h, None, None, ptr(o_obs))
        orc.orc_vec_step(h, ptr(host[i % len(host)]), None, ptr(o_obs), ptr(o_rew), ptr(o_done), 1)
    out = packed[(total - 1) & 1].to_host(np.float32, (n, D + 2))
    S0, S1 = piles
    sl, sc = v.slots(), v.station_scalars()
    for e in range(n):
        env = orc.orc_vec_env(h, e)
        for k, nk in ((0, S0), (1, S1)):
            want = np.zeros((9, nk), dtype=np.float32)
            orc.orc_station_slots(orc.orc_env_station(env, k), ptr(want))
            check_slots(sl[k][e], want, ("span", e, k))
            ws = np.zeros(8)
            orc.orc_station_scalars(orc.orc_env_station(env, k), ptr(ws))
            assert np.array_equal(sc[e, k, :6], ws[:6]), ("span", e, k, sc[e, k], ws)
    close(out[:, :D], o_obs, "span obs f32", atol=1e-6)
    close(out[:, D], o_rew, "span reward f32", rtol=1e-6, atol=1e-6)
    assert np.array_equal(out[:, D + 1] != 0, o_done.astype(bool))
    assert orc.orc_vec_overflow(h) == 0
    orc.orc_vec_destroy(h)
    v.close()


def test_a_captured_graph_replayed_twice_equals_eager_calls():
    """a reset and five steps of k_slot_packed + k_env captured once and replayed twice against the same calls made one by one: outputs,
    slot state and station records bit for bit.  (A replay bakes the clocks in: the capture starts with the reset, at the clock it
    ends at, and makes an even number of calls, as the other captures of this suite do.)"""
    chub = hub()
    from charginghub_env_amd import multi_gpu
    kw = dict(HUB, station_list=[20, 25])
    n, K = 23, 5
    res = []
    for form in ("eager", "graph"):
        v = chub.VecChargingHub(n, seed=SEED, rng="philox", env_id0=ENV_ID0, fused_step="off", tile="small", **kw)
        assert v.uses_packed_kernel and not v.uses_fused_step
        st = multi_gpu.Stream(0)
        D, A = v.obs_dim, v.act_dim
        acts = [multi_gpu.DeviceBuffer(n * A * 4) for _ in range(3)]
        for b, a in enumerate(acts):
            v.random_actions_device(a.ptr, 5, b, st.ptr)
        packed = [multi_gpu.DeviceBuffer(n * (D + 2) * 4) for _ in range(2)]
        obs0 = multi_gpu.DeviceBuffer(n * D * 4)

        def steps():
            v.reset_device(obs0.ptr, stream=st.ptr)
            for i in range(K):
                v.step_device_packed(acts[i % 3].ptr, packed[i & 1].ptr, stream=st.ptr)

        steps()
        st.sync()
        if form == "graph":
            v.graph_begin(st.ptr)
            steps()
            g = v.graph_end(st.ptr)
            v.graph_launch(g, st.ptr)
            mid = packed[(K - 1) & 1].to_host(np.float32, (n, D + 2), st.ptr)
            v.graph_launch(g, st.ptr)
            st.sync()
            v.graph_destroy(g)
        else:
            steps()
            mid = packed[(K - 1) & 1].to_host(np.float32, (n, D + 2), st.ptr)
            steps()
        end = packed[(K - 1) & 1].to_host(np.float32, (n, D + 2), st.ptr)
        res.append([mid, end, np.concatenate([x.reshape(n, -1) for x in v.slots()], axis=1), v.station_scalars().reshape(n, -1), np.array([v.clock])])
        v.close()
        st.destroy()
    assert res[0][-1][0] == K
    assert not np.array_equal(res[0][0], res[0][1])  # (the ticks go on: another episode)
    for k in range(len(res[0])):
        assert np.array_equal(res[0][k].view(np.uint32) if res[0][k].dtype == np.float32 else res[0][k],
                              res[1][k].view(np.uint32) if res[1][k].dtype == np.float32 else res[1][k]), ("eager vs graph", k)
