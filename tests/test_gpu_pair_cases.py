"""The paired tail launch (chub_run_steps on a handle with span_steps >= 2 on the two-launch step: k_pair_draws, k_slot_packed<.., RAW>,
k_env_pair<MORE>) against the CPU oracle, on the populations of tests/pair_cases_lib.py:

  Part 1  the tail's rare branches (six homogeneous handles of 16 envs of [64, 64] fast), every step of the script at BOTH positions of a pair:
          the "even" alignment runs calls of two from a day's step 0, the "odd" one from its step 1; chains of 8 and of 14 steps
          (k_env_pair<true>, whose blocks are overwritten before anyone can read them) are checked at their ends;
  Part 2  the forecourt with a line, a waiting list of hundreds and several arrivals per step (fcev_stuck, 16 envs): further arrivals are
          drawn inside the tail, draw_env_pre leaves only the count and the first arrival's SoC;
  Part 3  2048 and 4096 envs: level_lane's XCD-aware branch in k_pair_draws and in the level blocks of k_env_pair<true / false>, and the plain
          branch at the same sizes (work_order = "dispatch").
tests/test_pair_cases_cpu.py asserts on the oracle alone that the branches, the forecourt states and distinct envs are there.

After every call, for the two steps whose packed blocks remain: against the oracle -- f32 observation within 1e-6 absolute, f32 reward at 1e-6,
done equal, and at the call's end slots and station scalars [:6] bit for bit (the bars of test_gpu_tail_cases.against_oracle_step); against a
pairs-off handle (span_steps = "off", same seed and env_id0) bit for bit -- both blocks, slots, scalars and the arena with the address bytes
left out (as compare of test_gpu_pair_tails does it).  obs_f64() and reward_f64() are NOT compared: the tail writes EnvArrays::obs64 /
reward64 only with telemetry on (env_tail: `tel_on ? ev.obs64 : nullptr`), and telemetry sends chub_run_steps down the per-step path.

That pairs ran is asserted, not assumed: no telemetry, outputs, ledger, clocks, tape, profiler or communicator on the paired side;
uses_pair_tails, not uses_fused_step, uses_packed_kernel; and for every call chub_pair_plan's CHUB_PAIR_CALL and CHUB_PAIR_STEPS for the
handle's clock and the call's length are the number of steps the test means to go out as pairs.

A failing comparison names the config, the step, the env, the step's position in its pair and the branches the oracle took there."""
import ctypes as C
import functools

import numpy as np
import pytest

import pair_cases_lib as pc

pytestmark = pytest.mark.gpu


def hub():
    import charginghub_env_amd as chub
    return chub


class Case(object):
    """a population: its oracle trajectory, one handle per block of `block` envs (kws[k]), the batches and the plan of episodes"""

    def __init__(self, label, trajectory, names, kws, block, batches, plan, seed, env_id0):
        self.label, self.trajectory, self.names, self.kws, self.block = label, trajectory, names, kws, block
        self.batches, self.plan, self.seed, self.env_id0 = batches, plan, seed, env_id0

    @property
    def tr(self):
        return self.trajectory()

    def envs(self, k):
        return np.arange(k * self.block, (k + 1) * self.block)

    def slot_of_day(self, i):
        """(episode, step of the episode) of step i of the run"""
        ep = 0
        while i >= self.plan[ep]:
            i -= self.plan[ep]
            ep += 1
        return ep, i

    def where(self, i, env, pos):
        ep, t = self.slot_of_day(i)
        return "%s, config %s, step %d (episode %d, step %d: %s), env %d (local %d), branches %s" % (
            self.label, self.names[env // self.block], i, ep, t, pos, env, env % self.block, pc.flags_of(self.tr.flags, (i, env)))


PART1 = Case("part 1", pc.oracle_trajectory, pc.NAMES, [kw for _, kw in pc.configs()], pc.BLOCK, pc.action_batches(), pc.PLAN, pc.SEED, pc.ENV_ID0)
PART2 = Case("part 2", pc.forecourt_trajectory, ["fcev_stuck"], [pc.FORECOURT], pc.FORECOURT_N, pc.forecourt_batches(), pc.FORECOURT_PLAN,
             pc.FORECOURT_SEED, 0)


def xcd_case(name, n):
    return Case("part 3 (%d envs)" % n, functools.partial(pc.xcd_trajectory, name, n), [name], [pc.XCD_HUBS[name]], n, pc.xcd_batches(name, n),
                (pc.XCD_STEPS,), pc.XCD_SEED, 0)


# ---- comparisons that name the env-step
def no_bad(bad, case, i, envs, pos, what, got=None, want=None):
    bad = np.asarray(bad).reshape(len(envs), -1)
    rows = np.nonzero(bad.any(axis=1))[0]
    if rows.size:
        j = rows[0]
        detail = "" if got is None else "; got %s, want %s" % (np.asarray(got)[j].reshape(-1)[bad[j]][:6], np.asarray(want)[j].reshape(-1)[bad[j]][:6])
        raise AssertionError("%s differs at %s (%d envs of this call differ)%s" % (what, case.where(i, int(envs[j]), pos), rows.size, detail))


def same_bits(got, want, case, i, envs, pos, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    no_bad(got.view(u) != want.view(u), case, i, envs, pos, what, got, want)


def near(got, want, case, i, envs, pos, what, rtol, atol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    no_bad(~np.isclose(got, want, rtol=rtol, atol=atol), case, i, envs, pos, what, got, want)


# ---- a handle, its buffers and its calls
class Handle(object):
    def __init__(self, case, k, pairs, **options):
        from charginghub_env_amd import _lib, multi_gpu
        chub = hub()
        self.case, self.k, self.pairs, self.kw, self.envs = case, k, pairs, case.kws[k], case.envs(k)
        n = self.n = case.block
        self.v = v = chub.VecChargingHub(n, seed=case.seed, rng="philox", env_id0=case.env_id0 + n * k, fused_step="off",
                                         span_steps=2 if pairs else "off", **self.kw, **options)
        assert v.uses_pair_tails == pairs and not v.uses_fused_step and v.uses_packed_kernel, (case.label, case.names[k])
        self.D, self.A = v.obs_dim, v.act_dim
        assert case.batches.shape == (pc.PERIOD, n * len(case.kws), self.A)
        self.acts = [multi_gpu.DeviceBuffer(n * self.A * 4) for _ in range(pc.PERIOD)]
        for b, a in enumerate(self.acts):
            a.from_host(case.batches[b][self.envs])
        self.packed = [multi_gpu.DeviceBuffer(n * (self.D + 2) * 4) for _ in range(2)]
        for p in self.packed:
            p.from_host(np.zeros((n, self.D + 2), dtype=np.float32))
        self.obs0 = multi_gpu.DeviceBuffer(n * self.D * 4)
        self.c_acts = (C.c_void_p * pc.PERIOD)(*[a.ptr for a in self.acts])
        self.c_packed = (C.c_void_p * 2)(self.packed[0].ptr, self.packed[1].ptr)
        self.opt = _lib.ChubOptions()
        self.opt.fused_step, self.opt.span_steps = 1, 2
        self.opt.work_order = _lib.WORK_ORDER[options.get("work_order", "auto")]
        self.cfg = chub.make_config(self.kw["station_list"], self.kw["station_type_list"],
                                    **{f: x for f, x in self.kw.items() if f not in ("station_list", "station_type_list")})
        self.positions = {}  # step -> its position in the call that ran it

    def pair_plan(self, t, left):
        from charginghub_env_amd import _lib
        out = (C.c_int64 * 3)()
        assert self.v._lib.chub_pair_plan(C.byref(self.cfg), self.n, _lib.RNG_PHILOX, C.byref(self.opt), 0, 0, t, left, out) == 0
        return list(out)

    def run(self, first, count):
        """chub_run_steps; on the paired side: as many of the call's steps go out as pairs as the test intends"""
        from charginghub_env_amd._lib import check
        ep, t = self.case.slot_of_day(first)
        assert t == 0 or self.v.clock == t, (first, t, self.v.clock)
        intended = pc.paired_steps(t, count)
        for j in range(count):
            self.positions[first + j] = ("a pair's %s step" % ("first", "second")[j & 1]) if j < intended else "a single step"
        if self.pairs:
            assert self.pair_plan(t, count) == [1, 1, intended], (first, count, self.pair_plan(t, count))
        check(self.v._lib.chub_run_steps(self.v._h, None, self.c_acts, pc.PERIOD, self.c_packed, None, self.obs0.ptr, first, count, None))

    def step(self, i):
        self.positions[i] = "a single call"
        self.v.step_device_packed(self.acts[i % pc.PERIOD].ptr, self.packed[i & 1].ptr)

    def do(self, op):
        """("run", first, count) or ("step", i) -> the last step it ran"""
        if op[0] == "run":
            self.run(op[1], op[2])
            return op[1] + op[2] - 1
        self.step(op[1])
        return op[1]

    def block(self, i):
        return self.packed[i & 1].to_host(np.float32, (self.n, self.D + 2))

    def state(self):
        sl = self.v.slots()
        return {"slots of station 0": sl[0], "slots of station 1": sl[1], "station scalars": self.v.station_scalars()}

    def close(self):
        self.v.close()


def block_against_oracle(h, i, blk):
    case, tr, envs, pos, D = h.case, h.case.tr, h.envs, h.positions[i], h.D
    same_bits(blk[:, D + 1] != 0, tr.done[i, envs], case, i, envs, pos, "done")
    near(blk[:, :D], tr.obs[i, envs], case, i, envs, pos, "f32 obs", 0.0, 1e-6)
    near(blk[:, D], tr.reward[i, envs], case, i, envs, pos, "f32 reward", 1e-6, 1e-6)


def state_against_oracle(h, i, state):
    case, tr, envs, pos = h.case, h.case.tr, h.envs, h.positions[i]
    for k in (0, 1):
        same_bits(state["slots of station %d" % k], tr.slots[k][i, envs], case, i, envs, pos, "slots of station %d" % k)
    same_bits(state["station scalars"][:, :, :6], tr.scalars[i, envs][:, :, :6], case, i, envs, pos, "station scalars")


def address_bytes(on, off, label):
    """where the two handles' arenas may differ: their own device addresses (DevCtx) -- the bytes in which their blobs differ when nothing else can"""
    addr = on.v.get_state() != off.v.get_state()
    assert addr.sum() <= 4096, (label, "the two handles differ in more than their addresses", int(addr.sum()))
    return addr


def drive(case, k, program, record=None, **options):
    """Block k of the case: the paired handle and the pairs-off handle through the program.  After every call both remaining blocks and the
    state against the oracle and against the pairs-off handle.  record: {"blocks": {step: block}, "states": {last step of a call: state}}
    of the paired handle, filled in."""
    on, off = Handle(case, k, True, **options), Handle(case, k, False, **options)
    label = (case.label, case.names[k])
    try:
        addr = None
        if program[0] != ("run", 0, 1):
            # the first call holds a pair already: find the address bytes behind a reset and a single step, then go back to the fresh handle
            fresh = [h.v.get_state() for h in (on, off)]
            for h in (on, off):
                h.run(0, 1)
            addr = address_bytes(on, off, label)
            for h, blob in zip((on, off), fresh):
                h.v.set_state(blob)
                h.positions.clear()
        for op in program:
            last = on.do(op)
            assert off.do(op) == last
            if addr is None:  # behind ("run", 0, 1): a reset and one step, no pair
                addr = address_bytes(on, off, label)
            for i in (last - 1, last):
                if i < 0:
                    continue
                b_on, b_off = on.block(i), off.block(i)
                block_against_oracle(on, i, b_on)
                same_bits(b_on, b_off, case, i, on.envs, on.positions[i], "pairs on vs off: packed block")
                if record is not None:
                    record["blocks"][(k, i)] = b_on
            s_on, s_off = on.state(), off.state()
            state_against_oracle(on, last, s_on)
            for name in s_on:
                same_bits(s_on[name], s_off[name], case, last, on.envs, on.positions[last], "pairs on vs off: " + name)
            a, b = on.v.get_state(), off.v.get_state()
            bad = np.nonzero((a != b) & ~addr)[0]
            assert bad.size == 0, (label, "pairs on vs off: the arena after step %d (%s) differs in %d bytes, first at offset %d of %d" % (
                last, on.positions[last], bad.size, bad[0], a.size))
            if record is not None:
                record["states"][(k, last)] = s_on
        return on.positions
    finally:
        on.close()
        off.close()


def program_of(calls):
    return [("run", f, c) for f, c in calls]


@functools.lru_cache(maxsize=None)
def alignment_run(part, align):
    """the whole script in calls of two on every block of the case; what the paired handles left, for the chains to be compared with"""
    case = {1: PART1, 2: PART2}[part]
    calls = pc.alignment_calls(align, case.plan)
    assert all(c == 2 or (c == 1 and align == "odd") for _, c in calls)
    record = {"blocks": {}, "states": {}}
    for k in range(len(case.kws)):
        positions = drive(case, k, program_of(calls), record)
        # every step from an episode's second to its last but one held the position this alignment gives it
        for i in np.nonzero(pc.both_positions(case.plan))[0]:
            ep, t = case.slot_of_day(int(i))
            want = ("first", "second")[(t & 1) ^ (align == "odd")]
            assert positions[int(i)] == "a pair's %s step" % want, (align, i, positions[int(i)])
    return record


def chains(part, align, length):
    """the paired handles alone through calls of `length` steps: at every call's end the two remaining blocks and the state against the oracle
    and, bit for bit, against what the calls of two of the same alignment left at the same step"""
    case = {1: PART1, 2: PART2}[part]
    record = alignment_run(part, align)
    calls = pc.chain_calls(align, length, case.plan)
    assert max(pc.paired_steps(case.slot_of_day(f)[1], c) for f, c in calls) >= 6  # chains: k_env_pair<true> runs
    for k in range(len(case.kws)):
        h = Handle(case, k, True)
        try:
            for f, c in calls:
                h.run(f, c)
                last = f + c - 1
                for i in (last - 1, last):
                    if i < 0:
                        continue
                    blk = h.block(i)
                    block_against_oracle(h, i, blk)
                    same_bits(blk, record["blocks"][(k, i)], case, i, h.envs, h.positions[i], "calls of %d vs calls of two: packed block" % length)
                st = h.state()
                state_against_oracle(h, last, st)
                for name in st:
                    same_bits(st[name], record["states"][(k, last)][name], case, last, h.envs, h.positions[last], "calls of %d vs calls of two: %s" % (length, name))
        finally:
            h.close()


# ---- Part 1
@pytest.mark.parametrize("align", ["even", "odd"])
def test_rare_branches_in_calls_of_two(align):
    """every step of the designed script as a pair's first step (one alignment) and as its second (the other)"""
    alignment_run(1, align)


@pytest.mark.parametrize("length", [8, 14])
@pytest.mark.parametrize("align", ["even", "odd"])
def test_rare_branches_in_chains(align, length):
    chains(1, align, length)


# ---- Part 2
@pytest.mark.parametrize("align", ["even", "odd"])
def test_forecourt_in_calls_of_two(align):
    """a line, a waiting list of hundreds (q_time, q_mass and the folded tail are arena state: pairs on vs off) and several arrivals per step"""
    alignment_run(2, align)


@pytest.mark.parametrize("align", ["even", "odd"])
def test_forecourt_in_chains(align):
    chains(2, align, 8)


# ---- Part 3
@pytest.mark.parametrize("order", ["auto", "dispatch"])
@pytest.mark.parametrize("n", pc.XCD_SIZES)
@pytest.mark.parametrize("name", list(pc.XCD_HUBS))
def test_level_lanes_at_sizes_that_divide_evenly(name, n, order):
    """2048 envs: one level workgroup per XCD and segment (wpx = 1), 4096: two.  k_pair_draws and a <false> pair, two <true> pairs and a
    <false> one, a single step that reads what the last pair's level blocks left, a chain again -- every env against the oracle"""
    case = xcd_case(name, n)
    probe = Handle(case, 0, True, work_order=order)
    try:
        assert probe.v.uses_xcd_order == (order == "auto"), (name, n, order)
    finally:
        probe.close()
    program = list(pc.XCD_PROGRAM)
    assert program[0] == ("run", 0, 1) and [pc.paired_steps(op[1], op[2]) for op in program if op[0] == "run"] == [0, 2, 6, 4]
    drive(case, 0, program, work_order=order)
