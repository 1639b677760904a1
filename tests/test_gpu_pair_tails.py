"""chub_run_steps's pairs of steps whose tails share ONE launch (chub_options.span_steps on the two-launch step; k_env_pair, k_slot_packed<.., RAW>, k_pair_draws).

Every test runs one program of calls on two handles with the same seed -- pairs forced on (span_steps = 2) and pairs off (span_steps = 1: every
step a slot launch and a tail launch), both on the two-launch step -- and compares, bit for bit: both packed output blocks wherever the program
notes them, the decoded slots (chub_get_slots), the station scalars, and the WHOLE device arena as chub_get_state returns it: slot state words,
stay8, both stations' records, the tail actions, every env state array and both parities of the draw buffers (StationArrays::pk, EnvArrays::drw /
drw_cnt).  The arena also holds the handle's own device addresses (DevCtx): the bytes in which the two handles' blobs differ right after
their first reset -- when nothing but their addresses can differ -- are left out of the later comparisons.

The hub [2, 2] is there for the lazy raw draws: the words of queue positions 4 .. 9 are drawn only where a unit may queue that far.  Seed 31,
global env 0: the queues in front of step 5 of the first day -- the second step of the pair (4, 5) where the span starts the day, as in the
graph test -- hold 8 and 5 cars, those in front of steps 7, 9, 11 and 13 -- second steps of pairs in the program of spans -- (8, 4), (8, 4),
(7, 5) and (5, 5) (tests/test_pair_tails_cpu.py asserts it on the CPU oracle)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HUBS = {
    "c4_hub": dict(station_list=[20, 25], station_type_list=["fast", "slow"], fcev_permeate=0.02, renew_fluctuate=0.2, price_fluctuate=0.1),
    "no_slow_piles": dict(station_list=[16, 0], station_type_list=["fast", "slow"], fcev_permeate=0.0),
    "tiny": dict(station_list=[3, 5], station_type_list=["slow", "fast"], fcev_permeate=0.05, renew_fluctuate=0.3, price_fluctuate=0.3, hydro_loss=0.001),
    "full_waves": dict(station_list=[64, 64], station_type_list=["fast", "slow"], fcev_permeate=0.02, renew_fluctuate=0.1, price_fluctuate=0.2),
    "long_queues": dict(station_list=[2, 2], station_type_list=["fast", "slow"], fcev_permeate=0.02, renew_fluctuate=0.2, price_fluctuate=0.1),
}
SEED = 31


def hub():
    import charginghub_env_amd as chub
    return chub


class Side:
    """one handle, its buffers and the trace of what the program noted"""

    def __init__(self, n, kw, pairs):
        chub = hub()
        from charginghub_env_amd import multi_gpu
        self.v = v = chub.VecChargingHub(n, seed=SEED, rng="philox", fused_step="off", span_steps=2 if pairs else "off", **kw)
        assert v.uses_pair_tails == pairs and not v.uses_fused_step and v.uses_packed_kernel
        self.n, self.D, self.A = n, v.obs_dim, v.act_dim
        self.st = multi_gpu.Stream(0)
        self.acts = [multi_gpu.DeviceBuffer(n * self.A * 4) for _ in range(3)]
        for b, a in enumerate(self.acts):
            v.random_actions_device(a.ptr, 9, b, self.st.ptr)
        self.packed = [multi_gpu.DeviceBuffer(n * (self.D + 2) * 4) for _ in range(2)]
        for p in self.packed:  # (a block is compared before its first step has written it)
            p.from_host(np.zeros((n, self.D + 2), dtype=np.float32), self.st.ptr)
        self.obs0 = multi_gpu.DeviceBuffer(n * self.D * 4)
        self.c_acts = (C.c_void_p * 3)(*[a.ptr for a in self.acts])
        self.c_packed = (C.c_void_p * 2)(self.packed[0].ptr, self.packed[1].ptr)
        self.trace = []
        self.addr = None

    def run(self, first, count):
        from charginghub_env_amd._lib import check
        check(self.v._lib.chub_run_steps(self.v._h, None, self.c_acts, 3, self.c_packed, None, self.obs0.ptr, first, count, self.st.ptr))

    def step(self, i):
        self.v.step_device_packed(self.acts[i % 3].ptr, self.packed[i & 1].ptr, stream=self.st.ptr)

    def blocks(self):
        return [p.to_host(np.float32, (self.n, self.D + 2), self.st.ptr) for p in self.packed]

    def note(self, arena=False, blob=True):
        self.trace += self.blocks()
        if arena:
            self.st.sync()
            self.trace += [np.concatenate([x.reshape(self.n, -1) for x in self.v.slots()], axis=1), self.v.station_scalars().reshape(self.n, -1)]
            if blob:
                self.trace.append(self.v.get_state())

    def close(self):
        self.v.close()
        self.st.destroy()


def compare(on, off, label):
    """the traces of the two sides; blobs (uint8) without the bytes that are the handles' own addresses"""
    assert len(on.trace) == len(off.trace)
    addr = None
    for k, (a, b) in enumerate(zip(on.trace, off.trace)):
        assert a.shape == b.shape and a.dtype == b.dtype, (label, k)
        if a.dtype == np.uint8 and a.ndim == 1:
            if addr is None:  # the first blob of a program is taken right behind the first reset
                addr = a != b
                assert addr.sum() <= 4096, (label, "the two handles differ in more than their addresses right after the reset", int(addr.sum()))
                continue
            bad = np.nonzero((a != b) & ~addr)[0]
            assert bad.size == 0, (label, "arena: array %d differs in %d bytes, first at offset %d of %d" % (k, bad.size, bad[0], a.size))
        else:
            u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
            bad = np.argwhere(np.ascontiguousarray(a).view(u) != np.ascontiguousarray(b).view(u))
            assert bad.size == 0, (label, "array %d differs in %d places, first at %s" % (k, len(bad), bad[0]))


def both(n, kw, program, label):
    sides = [Side(n, kw, True), Side(n, kw, False)]
    try:
        for s in sides:
            program(s)
        compare(sides[0], sides[1], label)
    finally:
        for s in sides:
            s.close()


def spans_program(s):
    s.run(0, 1)           # the reset and a span of ONE step: no pair
    s.note(arena=True)    # (the first blob: where the two handles' addresses sit)
    s.run(1, 2)           # a span of two from an odd step: one pair
    s.note(arena=True)
    s.run(3, 3)           # three from an odd step: a pair and an odd step out
    s.note(arena=True)
    s.run(6, 4)           # two spans back to back, each a chain of its own
    s.run(10, 6)
    s.note(arena=True)
    s.step(16)            # single calls behind a span ...
    s.step(17)
    s.step(18)
    s.note(arena=True)
    s.run(19, 2)          # ... and a span behind single calls
    s.note(arena=True)
    s.run(21, 96 - 21 + 5)  # across the day boundary: pairs to the day's end, the reset, pairs and an odd step out in the new day
    s.note(arena=True)
    first = 96 + 5
    s.st.sync()
    blob = s.v.get_state()  # a span, a snapshot, further steps, the snapshot back, the same steps again
    s.run(first, 7)
    s.note(arena=True)
    s.st.sync()
    s.v.set_state(blob)
    s.run(first, 7)
    s.note(arena=True)
    s.run(first + 7, 96)  # 96 steps: to the day's end (84: pairs all the way), the reset, 12 more
    s.note(arena=True)


@pytest.mark.parametrize("n", [300, 2304])
@pytest.mark.parametrize("name", ["c4_hub", "no_slow_piles", "tiny", "full_waves", "long_queues"])
def test_pairs_against_every_step_two_launches(name, n):
    """spans of 1, 2, 3 and 96 steps, from odd steps, across a day boundary, back to back, mixed with single calls both ways and around a
    snapshot; 300 envs: a partial tail workgroup and a partial last slot tile, 2304: several tail workgroups"""
    both(n, HUBS[name], spans_program, (name, n))


def test_snapshot_replays_the_same_steps():
    """the steps run again from the restored snapshot give what they gave the first time (within the paired handle itself)"""
    s = Side(300, HUBS["c4_hub"], True)
    try:
        s.run(0, 9)
        s.st.sync()
        blob = s.v.get_state()
        s.run(9, 8)
        first = s.blocks()
        s.st.sync()
        s.v.set_state(blob)
        s.run(9, 8)
        again = s.blocks()
        for a, b in zip(first, again):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        s.close()


@pytest.mark.parametrize("name", ["c4_hub", "long_queues"])
def test_pairs_in_a_graph_of_two_days_replayed(name):
    """the paired form captured in a graph of two whole days (194 ticks) and replayed three times, against the same six days call by call:
    both packed blocks after every replay, slots and station scalars at the end"""
    n = 300
    on, off = Side(n, HUBS[name], True), Side(n, HUBS[name], False)
    try:
        on.st.sync()
        on.v.graph_begin(on.st.ptr)
        on.run(0, 192)
        g = on.v.graph_end(on.st.ptr)
        for r in range(3):
            on.v.graph_launch(g, on.st.ptr)
            on.note()
            off.run(0, 192)
            off.note()
        # (no blobs: a snapshot's header carries the ticks the replays covered, which the handle stepped call by call does not have)
        on.note(arena=True, blob=False)
        off.note(arena=True, blob=False)
        on.v.graph_destroy(g)
        compare(on, off, (name, "graph"))
    finally:
        on.close()
        off.close()
