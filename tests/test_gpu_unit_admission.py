"""The packed slot kernel's admission, once per unit (slot_body_packed): on the small tile a step's unit pass -- one lane per (env, station)
behind the workgroup's first barrier -- loads the unit's decoded draws itself, works out assign = min(want, empties) and the capped queue,
leaves the admission count in the unit's word (s_uinfo) and writes the unit's record word (s_unit); the S_k lanes of the unit only compare
their rank with that count.  Resets, the large tile, the one-launch kernels and stations of more than 64 piles keep the per-lane form.

Held to the CPU oracle bit for bit -- slot words, station scalars (the three power sums, car_number, line, flow_in), the f64 observation
and reward, done -- after EVERY call, every env of the batch, served by the call or not, over a reset plus one whole day under a seeded
random policy, at the shapes where the unit lane's work can go wrong:

  [20, 25] x 23   two full workgroups (11 envs, 22 units on the first wave) and one holding a single env; units straddle waves
  [64, 64] x 9    a unit is exactly a wave
  [5, 3]   x 130  64 envs per workgroup: 128 unit lanes over two waves
  [1, 1]   x 300  envs per workgroup at their cap (128): 256 unit lanes, all four waves; the fast station's reset draw is negative
                  (nobody admitted, empty queue) and its queue stands at max_line through the peak
  [16, 0], [0, 7] x 70   a station without piles: its unit has no lanes, its record is packed_records' own

Every shape in the lock-step form, as a masked call on every third env followed by one on the rest, and fed one bit per pile; one shape
restored mid-day into a fresh handle (chub_set_state: the restored launch consumes the pre-drawn words), one fixture through tape mode
(the unit lane reads the words decoded from the caller's tape).  What each day must contain is counted on the oracle's side and asserted, so
that no case passes for want of the situation: a unit without a single empty, more cars wanting in than empties, fewer, a queue at
max_line, and for [1, 1] the negative reset draw.  (A step's own `want` is a count, never negative: only a reset's raw draw is, and
resets keep the per-lane form.)  The large tile did not take the change and is held bit-identical to the small one by test_gpu_parity."""
import ctypes as C

import numpy as np
import pytest

from orclib import orc, ptr
from test_gpu_parity import _oracle_vec, hub

pytestmark = pytest.mark.gpu

HUB = dict(station_type_list=["fast", "slow"], hydro_prod_rate=100.0, hydro_store_vlt=25.0, init_soc=0.2, fc_max_power=100.0,
           fcev_permeate=0.01, constant_charging=False, renew_fluctuate=0.3, price_fluctuate=0.3, hydro_loss=0.001)
SEED, ENV_ID0 = 0xAD1155, 7000
MAX_LINE = 10
SHAPES = [([20, 25], 23), ([64, 64], 9), ([5, 3], 130), ([1, 1], 300), ([16, 0], 70), ([0, 7], 70)]
IDS = ["20_25", "64_64", "5_3", "1_1", "16_0", "0_7"]
# what the day of each shape must show on the oracle's side, in every form (counted on the oracle alone before the shapes were relied on)
COMMON = ("want_over_empties", "want_under_empties", "no_empties", "line_at_max")
MUST = {"20_25": COMMON, "5_3": COMMON, "16_0": COMMON + ("no_piles",), "0_7": COMMON + ("no_piles",),
        "64_64": ("want_under_empties",),  # (no seed fills 64 piles: the arrival rates do not grow with the station)
        "1_1": ("want_over_empties", "no_empties", "line_at_max", "negative_reset_draw")}  # (a single pile is never left idle with nobody waiting)


class Day(object):
    """the handle (device=True) and the oracle's envs, driven with the same calls and compared, whole batch, after each"""

    def __init__(self, piles, n, device=True):
        self.piles, self.n, self.device = list(piles), n, device
        self.kw = dict(HUB, station_list=self.piles)
        self.cfg, self.h = _oracle_vec(self.kw, n, ENV_ID0, SEED)
        self.v = None
        if device:
            self.open()
        self.D = orc.orc_env_obs_dim(C.byref(self.cfg))
        self.A = sum(self.piles) + 2
        self.o_obs, self.o_rew, self.o_done = np.zeros((n, self.D)), np.zeros(n), np.zeros(n, dtype=bool)
        self.calls = 0
        self.rs = np.random.RandomState(11)
        self.seen = dict.fromkeys(("want_over_empties", "want_under_empties", "no_empties", "line_at_max", "negative_reset_draw", "no_piles"), 0)

    def open(self):
        self.v = hub().VecChargingHub(self.n, seed=SEED, rng="philox", env_id0=ENV_ID0, fused_step="off", tile="small", **self.kw)
        assert self.v.uses_packed_kernel and not self.v.uses_fused_step
        self.v.set_telemetry(True)

    def restore_into_a_fresh_handle(self):
        snap = self.v.get_state()
        self.v.close()
        self.open()
        self.v.set_state(snap)

    # ---- the oracle's side
    def _oracle_slots(self):
        out = []
        for k in (0, 1):
            a = np.zeros((self.n, 9, self.piles[k]), dtype=np.float32)
            if self.piles[k]:
                orc.orc_vec_slots(self.h, k, ptr(a))
            out.append(a)
        return out

    def _oracle_scalars(self):
        sc = np.zeros((self.n, 2, 8))
        orc.orc_vec_station_scalars(self.h, ptr(sc))
        return sc

    def _ticks(self, rows):
        """the Philox tick of the call for the envs it serves: the device's own report; without a device, one per call"""
        self.calls += 1
        if self.device:
            return self.v.env_clocks(ticks=True)[1]
        return np.full(self.n, self.calls, dtype=np.uint32)

    def _oracle_call(self, rows, ticks, act):
        before = self._oracle_slots() if act is not None else None
        for e in rows:
            env = orc.orc_vec_env(self.h, int(e))
            orc.orc_rng_set_tick(orc.orc_env_rng(env), int(ticks[e]) - 1)  # (the oracle counts up at the start of a call)
            if act is None:
                orc.orc_env_reset(env, None, None, ptr(self.o_obs[e]))
            else:
                r, d = C.c_double(0.0), C.c_int(0)
                orc.orc_env_step(env, ptr(act[e]), None, ptr(self.o_obs[e]), C.byref(r), C.byref(d))
                self.o_rew[e], self.o_done[e] = r.value, bool(d.value)
        sc = self._oracle_scalars()
        if act is None:
            self.seen["negative_reset_draw"] += int((sc[rows, :, 5] < 0).sum())
            return
        # receive_car as the oracle ran it, per unit: empties after the departures, the cars admitted, the queue left
        after = self._oracle_slots()
        for k in (0, 1):
            b, a = before[k][rows], after[k][rows]
            empties = self.piles[k] - ((b[:, 0] > 0.5) & (b[:, 7] - b[:, 8] > 1)).sum(axis=1)
            admitted = ((a[:, 0] > 0.5) & (a[:, 8] == 0)).sum(axis=1)
            line = sc[rows, k, 4]
            assert (admitted <= empties).all()
            self.seen["want_over_empties"] += int((line > 0).sum())
            self.seen["want_under_empties"] += int(((line == 0) & (admitted < empties)).sum())
            self.seen["line_at_max"] += int((line == MAX_LINE).sum())
            if self.piles[k]:
                self.seen["no_empties"] += int(((empties == 0) & (line > 0)).sum())
            else:
                self.seen["no_piles"] += int((line > 0).sum())

    # ---- both sides
    def _compare(self, label, with_reward):
        if not self.device:
            return
        sl, want_sl = self.v.slots(), self._oracle_slots()
        for k in (0, 1):
            assert np.array_equal(sl[k].view(np.uint32), want_sl[k].view(np.uint32)), (label, "slots of station", k)
        sc, want_sc = self.v.station_scalars(), self._oracle_scalars()
        assert np.array_equal(sc[:, :, :6], want_sc[:, :, :6]), (label, "station scalars", np.argwhere(sc[:, :, :6] != want_sc[:, :, :6])[:5])
        obs = self.v.obs_f64()
        assert np.array_equal(obs, self.o_obs), (label, "obs", np.argwhere(obs != self.o_obs)[:5])
        if with_reward:
            rew = self.v.reward_f64()
            assert np.array_equal(rew, self.o_rew), (label, "reward", np.argwhere(rew != self.o_rew)[:5])

    def reset(self, label="reset"):
        if self.device:
            self.v.reset()
        rows = np.arange(self.n)
        self._oracle_call(rows, self._ticks(rows), None)
        self._compare(label, False)

    def actions(self):
        act = self.rs.uniform(-1, 1, size=(self.n, self.A)).astype(np.float32)
        if self.rs.randint(5) == 0:
            act[:, :self.A - 2] = 1.0
        return act

    def step(self, mask=None, bits=False, label=""):
        rows = np.arange(self.n) if mask is None else np.nonzero(mask)[0]
        act = self.actions()
        if bits:  # thresholded pile actions, which the bits carry whole
            act[:, :self.A - 2] = np.where(act[:, :self.A - 2] >= 0, np.float32(1), np.float32(-1))
        if self.device:
            if bits:
                done = self.v.step_bits(*self.v.pack_actions(act))[2]
            else:
                done = (self.v.step(act) if mask is None else self.v.step_envs(mask, act))[2]
        self._oracle_call(rows, self._ticks(rows), act)
        if self.device:
            assert np.array_equal(np.asarray(done, dtype=bool)[rows], self.o_done[rows]), (label, "done")
        self._compare(label, True)

    def close(self, must):
        assert orc.orc_vec_overflow(self.h) == 0
        orc.orc_vec_destroy(self.h)
        if self.device:
            self.v.close()
        missing = [c for c in must if self.seen[c] == 0]
        assert not missing, ("the day never showed", missing, self.seen)
        return self.seen


def one_day(form, piles, n, must, device=True):
    p = Day(piles, n, device)
    third = np.arange(n) % 3 == 0
    p.reset()
    for t in range(96):
        if form == "masked":
            p.step(third, label=(t, "every third env"))
            p.step(~third, label=(t, "the rest"))
        elif form == "restored":
            if t == 41:
                p.restore_into_a_fresh_handle()
            p.step(label=t)
        else:
            p.step(bits=form == "bits", label=t)
    return p.close(must)


@pytest.mark.parametrize("form", ["lock_step", "masked", "bits"])
@pytest.mark.parametrize("piles,n", SHAPES, ids=IDS)
def test_a_day_matches_the_oracle(piles, n, form):
    one_day(form, piles, n, MUST["%d_%d" % tuple(piles)])


def test_a_day_restored_mid_day_into_a_fresh_handle():
    """chub_get_state after step 41, the handle destroyed, a fresh one restored: its first launch consumes the words the old handle drew a
    launch ahead, and the unit lanes read them from the restored arena"""
    one_day("restored", [20, 25], 23, MUST["20_25"])


def test_tape_mode_reads_the_callers_words():
    """tape mode on the small tile and two launches per step: the unit lane reads the words decoded from the caller's pk tape -- the
    reference's own recorded day of the 20 + 25 hub (test_gpu_tape's replay of that fixture)"""
    from test_gpu_tape import test_packed_kernel_replays_reference_fixture as replay
    replay("env_c3_random", tile="small", fused="off")
