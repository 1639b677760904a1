"""Running feature statistics without a device (include/chub.h, "running feature statistics"): the new entry points are one list in the
header and the binding; wrappers.normalize_features is the kernel's f32 normalisation bit for bit, values on +-clip included; and
tests/normalizer_lib.py's definition is consistent with itself -- two batches merged equal one batch over their concatenation within the
bound the GPU test holds the device to, and a constant column has M2 == 0 exactly."""
import os
import re

import numpy as np
import pytest

import normalizer_lib as nl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

NEW = ("chub_moments_create", "chub_moments_destroy", "chub_moments_update_device", "chub_moments_reset_device", "chub_moments_get",
       "chub_moments_set", "chub_moments_state_device", "chub_policy_set_normalizer", "chub_policy_set_normalizer_device",
       "chub_policy_get_normalizer_device", "chub_policy_normalizer_from_moments_device")


def test_the_new_entry_points_are_in_the_header_and_the_binding():
    from charginghub_env_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "chub.h")).read()
    for fn in NEW:
        assert fn in _lib.EXPORTED and re.search(r"\bint %s\(" % fn, hdr), fn
    # the new section stands behind "pile sets and advantages", and the two paragraphs that keep a critic out of scope are still there
    assert hdr.index("---- pile sets and advantages") < hdr.index("---- running feature statistics") < hdr.index("int chub_moments_create(")
    assert hdr.count("Out of scope: a critic") == 2
    from charginghub_env_amd import vec_env, wrappers
    for name in ("set_normalizer", "set_normalizer_device", "get_normalizer_device", "normalizer", "normalizer_from_moments"):
        assert callable(getattr(vec_env.DevicePolicy, name)), name
    for name in ("update_device", "reset_device", "get", "set", "close"):
        assert callable(getattr(vec_env.DeviceMoments, name)), name
    assert isinstance(vec_env.DeviceMoments.state_ptr, property) and callable(vec_env.VecChargingHub.make_moments)
    assert callable(wrappers.TorchHubVecEnv.update_normalizer) and callable(wrappers.TorchHubVecEnv.policy_normalizer)


def test_normalize_features_in_torch_is_the_kernels_f32_arithmetic_bit_for_bit():
    torch = pytest.importorskip("torch")
    from charginghub_env_amd import wrappers
    rs = np.random.RandomState(3)
    T, n, F, clip = 3, 37, 29, 2.5
    x = (rs.normal(size=(T, n, F)) * np.logspace(-2, 3, F)).astype(F32)  # columns whose scales differ by 10^5
    mean = (rs.normal(size=F) * np.logspace(-2, 3, F)).astype(F32)
    inv_std = (1.0 / np.logspace(-2, 3, F)).astype(F32)
    # dyadic entries that land on +-clip exactly, beside entries far beyond it
    x[0, :, 0], mean[0], inv_std[0] = rs.choice([-1.0, 1.5, 0.25, 4.0, -3.0], size=n), 0.25, 2.0
    want = nl.normalise(x, mean, inv_std, clip)
    assert (want == F32(clip)).any() and (want == -F32(clip)).any() and (np.abs(want) < clip).any()
    assert (want[0, :, 0] == F32(clip)).any() and (want[0, :, 0] == -F32(clip)).any(), "values that land on the clip themselves"
    got = wrappers.normalize_features(torch.tensor(x), torch.tensor(mean), torch.tensor(inv_std), clip)
    assert got.dtype == torch.float32 and tuple(got.shape) == x.shape
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    # a clip that is no f32 is the policy's f32 clip
    got = wrappers.normalize_features(torch.tensor(x), torch.tensor(mean), torch.tensor(inv_std), 0.1)
    assert np.array_equal(got.numpy().view(np.uint32), nl.normalise(x, mean, inv_std, 0.1).view(np.uint32))


@pytest.mark.parametrize("F,R1,R2", [(1, 1, 1), (13, 70, 187), (64, 257, 3), (5, 1000, 1000)])
def test_two_batches_merged_equal_one_batch_over_their_concatenation(F, R1, R2):
    """Columns whose scales span 10^6, each with an offset of the order of its own spread.  (The state keeps the mean rounded to f64 AT THE
    MEAN'S MAGNITUDE, and the next merge reads that rounding error e <= 2^-53 |mean| as part of the distance between the batch means: M2
    moves by 2 e |S1 / n_b| n n_b / n'.  That is the running algorithm's own, not a summation error, and the bound below -- which knows the
    deviations only -- covers it while |mean| is of the order of R spreads; a column of 10^6 +- 10^-1 is held to the definition on the
    state it actually starts from, in the GPU test.)"""
    rs = np.random.RandomState(F + R1)
    x = ((rs.normal(size=(R1 + R2, F)) + rs.uniform(-2, 2, size=F)) * np.logspace(-3, 3, F)).astype(F32)
    one, _, n_b, S2, dmax = nl.update(nl.zero_state(F), x)
    two = nl.update(nl.update(nl.zero_state(F), x[:R1])[0], x[R1:])[0]
    assert one[0] == two[0] == n_b == R1 + R2
    b_mean, b_m2 = nl.bounds(R1 + R2, one, S2, dmax)
    assert (np.abs(two[1] - one[1]) <= b_mean).all(), (np.abs(two[1] - one[1]).max(), b_mean.min())
    assert (np.abs(two[2] - one[2]) <= b_m2).all(), (np.abs(two[2] - one[2]).max(), b_m2.min())
    # against numpy's own two-pass moments in f64, far inside the same bound's scale
    x64 = x.astype(np.float64)
    assert (np.abs(one[1] - x64.mean(axis=0)) <= 1e-12 * np.abs(x64).max(axis=0)).all()
    assert np.allclose(one[2], x64.var(axis=0) * (R1 + R2), rtol=1e-9, atol=1e-300)
    # a mask that counts nobody leaves the state as it is, one that counts everybody is no mask
    assert all(np.array_equal(a, b) for a, b in zip(nl.update(one, x, np.zeros(len(x), bool))[0], one))
    assert all(np.array_equal(a, b) for a, b in zip(nl.update(nl.zero_state(F), x, np.ones(len(x), bool))[0], one))


def test_a_constant_column_has_m2_zero_exactly():
    rs = np.random.RandomState(5)
    x = rs.normal(size=(300, 4)).astype(F32)
    x[:, 1] = F32(1234.5678)   # no short binary fraction: a raw sum of squares would not cancel
    x[:, 3] = F32(-1e6) + F32(0.1)
    st = nl.update(nl.zero_state(4), x[:100])[0]
    assert st[2][1] == 0.0 and st[2][3] == 0.0 and st[1][1] == np.float64(x[0, 1]) and st[2][0] > 0
    st = nl.update(st, x[100:], rs.uniform(size=200) < 0.5)[0]
    assert st[2][1] == 0.0 and st[2][3] == 0.0 and st[1][1] == np.float64(x[0, 1]) and st[1][3] == np.float64(x[0, 3])
    mean32, inv32 = nl.from_moments(st, 1e-8)
    assert mean32[1] == x[0, 1] and inv32[1] == F32(1.0 / np.sqrt(1e-8)) and nl.from_moments(nl.zero_state(4), 1e-8) is None
    # non-finite inputs give a non-finite state
    x[7, 0] = np.nan
    bad = nl.update(nl.zero_state(4), x)[0]
    assert np.isnan(bad[1][0]) and np.isnan(bad[2][0]) and np.isfinite(bad[1][2])
