"""chub_shuffle_rows_device (include/chub.h, "an optimiser on the device") against tests/adam_lib.py's numpy definition: every R of the
CPU test's list, and 6 291 456 rows -- six trips of the launch's 2^20 lanes, a quarter of E's domain outside 0 .. R - 1."""
import numpy as np
import pytest

import adam_lib as al
from test_gpu_autoreset import buffers
from test_gpu_pile_obs import make
from test_gpu_policy_sample import close_all

pytestmark = pytest.mark.gpu
CANARY = -7


def test_every_size_equals_the_definition_and_is_a_permutation():
    mg = buffers()
    v = make("philox", [3, 2], 64)
    biggest = max(al.SHUFFLE_R)
    rows, counter = mg.DeviceBuffer(8 * (biggest + 1)), mg.DeviceBuffer(8)
    key, c = al.SHUFFLE_KEYS[2]  # (a counter above 2^32)
    counter.from_host(np.array([c - 5], dtype=np.int64))
    for R in al.SHUFFLE_R:
        want = al.shuffle_rows(key, c, R)
        rows.from_host(np.full(biggest + 1, CANARY, dtype=np.int64))
        v.shuffle_rows_device(rows.ptr, R, key, d_counter=counter.ptr, offset=5)  # (counter + offset, read on the device)
        v.sync()
        got = rows.to_host(np.int64, (biggest + 1,))
        assert np.array_equal(got[:R], want), (R, np.nonzero(got[:R] != want)[0][:5])
        assert (got[R:] == CANARY).all(), (R, "nothing is written past R")
        assert (got[:R] >= 0).all() and np.array_equal(np.sort(got[:R]), np.arange(R)), R
        assert np.array_equal(v.shuffle_rows(R, key, c), want)
    # no counter: 0; another key, a 64-bit one
    for key, c in (al.SHUFFLE_KEYS[0], al.SHUFFLE_KEYS[1]):
        v.shuffle_rows_device(rows.ptr, 1025, key, offset=c)
        v.sync()
        assert np.array_equal(rows.to_host(np.int64, (1025,)), al.shuffle_rows(key, c, 1025))
    close_all(rows, counter, v)


def test_six_million_rows():
    """every entry against chub_shuffle_rows, the definition in host C (which tests/test_adam_cpu.py holds to the numpy definition at this
    size too), every 97th entry against the numpy definition itself (an entry is a function of its own r; all of them in numpy take a
    quarter of a minute), and a permutation with no -1"""
    mg = buffers()
    R = al.SHUFFLE_BIG
    v = make("philox", [3, 2], 64)
    key, c = al.SHUFFLE_KEYS[2]
    rows = mg.DeviceBuffer(8 * (R + 1024))
    rows.from_host(np.full(R + 1024, CANARY, dtype=np.int64))
    v.shuffle_rows_device(rows.ptr, R, key, offset=c)
    v.sync()
    got = rows.to_host(np.int64, (R + 1024,))
    assert (got[R:] == CANARY).all()
    got = got[:R]
    assert np.array_equal(got, v.shuffle_rows(R, key, c))
    at = np.arange(0, R, 97)
    assert np.array_equal(got[at], al.shuffle_rows(key, c, R, at=at))
    seen = np.zeros(R, dtype=bool)
    assert got.min() == 0 and got.max() == R - 1
    seen[got] = True
    assert seen.all()
    close_all(rows, v)
