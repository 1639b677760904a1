"""The optimiser's host-only parts (include/chub.h, "an optimiser on the device") against tests/adam_lib.py, without a device:
chub_adam_plan's arithmetic, chub_shuffle_rows bit for bit against the numpy definition, E as a bijection, the refusals that need no
device, and the conditions on the data of tests/test_gpu_adam.py, checked here on the same data."""
import ctypes as C
import math

import numpy as np
import pytest

import adam_lib as al

ERR_ARG = -1


def lib():
    from charginghub_env_amd import _lib
    return _lib.load_library()


def last_error():
    return lib().chub_last_error().decode()


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


ALL_NETS = [(name, al.shapes_of(F, w), G) for name, (F, w) in al.ACTOR_NETS.items() for G in (0, 2)] + \
           [(name, al.shapes_of(F, w), 0) for name, (F, w) in al.CRITIC_NETS.items()]


@pytest.mark.parametrize("name,shapes,G", ALL_NETS, ids=lambda x: str(x) if not isinstance(x, list) else "")
def test_plan_equals_the_arithmetic(name, shapes, G):
    from charginghub_env_amd import _lib
    out_dims = np.array([o for o, _ in shapes], dtype=np.int32)
    in_dims = np.array([i for _, i in shapes], dtype=np.int32)
    out = _lib.ChubAdamPlanOut()
    assert lib().chub_adam_plan(ptr(out_dims), ptr(in_dims), len(shapes), G, C.byref(out)) == 0, last_error()
    got = {k: int(getattr(out, k)) for k, _ in out._fields_}
    assert got == al.plan(shapes, G), (name, got, al.plan(shapes, G))


def test_the_wide_net_takes_a_second_trip():
    """64 -> 256 -> 224 -> 47 with log_std: 83 chunks of 1024 on 64 workgroups -- workgroups 0 .. 18 of both launches walk a second chunk"""
    p = al.plan(al.shapes_of(*al.ACTOR_NETS["64-256-224-47"]), 2)
    assert p["n"] == 84785 and p["norm_workgroups"] == p["step_workgroups"] == al.MAX_BLOCKS < (p["n"] + al.CHUNK - 1) // al.CHUNK == 83
    small = al.plan(al.shapes_of(*al.ACTOR_NETS["13-33-31-47"]), 2)
    assert small["norm_workgroups"] == (small["n"] + al.CHUNK - 1) // al.CHUNK < al.MAX_BLOCKS


def c_shuffle(key, counter, R):
    rows = np.full(R, -7, dtype=np.int64)
    assert lib().chub_shuffle_rows(C.c_uint64(key), C.c_uint64(counter), R, ptr(rows)) == 0, last_error()
    return rows


@pytest.mark.parametrize("R", al.SHUFFLE_R)
def test_shuffle_rows_equals_the_definition_and_is_a_permutation(R):
    walk = []
    for key, counter in al.SHUFFLE_KEYS:
        want = al.shuffle_rows(key, counter, R, walk)
        got = c_shuffle(key, counter, R)
        assert np.array_equal(got, want), (R, key, counter, np.nonzero(got != want)[0][:5])
        assert (got >= 0).all() and np.array_equal(np.sort(got), np.arange(R)), (R, key, counter)
    print("R = %d: the longest walk took %d applications of E (cap %d)" % (R, max(walk), al.WALK_CAP))
    assert max(walk) <= al.WALK_CAP // 2, "far below the cap"


@pytest.mark.parametrize("nb", range(1, 13))
def test_E_is_a_bijection_of_its_whole_domain(nb):
    """exhaustively; with R = 2^nb the walk never leaves the domain, so chub_shuffle_rows is E itself"""
    for key, counter in al.SHUFFLE_KEYS[:2]:
        y = al.encrypt(np.arange(1 << nb, dtype=np.uint64), nb, key, counter)
        assert np.array_equal(np.sort(y), np.arange(1 << nb, dtype=np.uint64)), (nb, key, counter)
        assert np.array_equal(c_shuffle(key, counter, 1 << nb), y.astype(np.int64))


def test_six_million_rows_on_the_host():
    """the size of the GPU test: chub_shuffle_rows is a permutation with no -1, and equals the numpy definition at every 97th entry"""
    R = al.SHUFFLE_BIG
    key, c = al.SHUFFLE_KEYS[2]
    got = c_shuffle(key, c, R)
    at = np.arange(0, R, 97)
    assert np.array_equal(got[at], al.shuffle_rows(key, c, R, at=at))
    seen = np.zeros(R, dtype=bool)
    assert got.min() == 0 and got.max() == R - 1
    seen[got] = True
    assert seen.all()


def test_counters_and_keys_give_different_permutations():
    R = 4096
    base = c_shuffle(5, 0, R)
    for other in (c_shuffle(5, 1, R), c_shuffle(6, 0, R), c_shuffle(5, 1 << 32, R), c_shuffle(5 + (1 << 32), 0, R)):
        same = int((other == base).sum())
        assert same < R // 64, same
    moved = np.abs(base - np.arange(R)).mean()
    assert R / 4 < moved < R / 2.4, moved  # (a uniform permutation: R / 3)


def test_refusals_that_need_no_device():
    from charginghub_env_amd import _lib
    L = lib()
    one = np.ones(4, dtype=np.int32)
    out = _lib.ChubAdamPlanOut()
    rows = np.zeros(8, dtype=np.int64)
    hyper = _lib.adam_hyper()
    h = C.c_void_p()
    size = C.c_int64()
    four = (C.c_void_p * 4)()
    calls = [
        ("plan: null out", lambda: L.chub_adam_plan(ptr(one), ptr(one), 1, 0, None)),
        ("plan: null dims", lambda: L.chub_adam_plan(None, ptr(one), 1, 0, C.byref(out))),
        ("plan: no layers", lambda: L.chub_adam_plan(ptr(one), ptr(one), 0, 0, C.byref(out))),
        ("plan: five layers", lambda: L.chub_adam_plan(ptr(one), ptr(one), 5, 0, C.byref(out))),
        ("plan: negative G", lambda: L.chub_adam_plan(ptr(one), ptr(one), 1, -1, C.byref(out))),
        ("plan: a zero dim", lambda: L.chub_adam_plan(ptr(np.zeros(4, dtype=np.int32)), ptr(one), 1, 0, C.byref(out))),
        ("shuffle: null rows", lambda: L.chub_shuffle_rows(1, 0, 8, None)),
        ("shuffle: R = 0", lambda: L.chub_shuffle_rows(1, 0, 0, ptr(rows))),
        ("shuffle: R > 2^40", lambda: L.chub_shuffle_rows(1, 0, (1 << 40) + 1, ptr(rows))),
        ("shuffle_device: null env", lambda: L.chub_shuffle_rows_device(None, 1, None, 0, 8, ptr(rows), None)),
        ("create_policy: null", lambda: L.chub_adam_create_policy(None, C.byref(hyper), C.byref(h))),
        ("create_critic: null", lambda: L.chub_adam_create_critic(None, C.byref(hyper), C.byref(h))),
        ("set_hyper: null", lambda: L.chub_adam_set_hyper(None, C.byref(hyper))),
        ("set_lr_device: null", lambda: L.chub_adam_set_lr_device(None, ptr(rows), None)),
        ("grads: null", lambda: L.chub_adam_grads(None, four, four, C.byref(h))),
        ("counter: null", lambda: L.chub_adam_counter_device(None, C.byref(h))),
        ("step: null", lambda: L.chub_adam_step_device(None, four, four, None, None, None)),
        ("reset: null", lambda: L.chub_adam_reset_device(None, None)),
        ("state_size: null", lambda: L.chub_adam_state_size(None, C.byref(size))),
        ("get_state: null", lambda: L.chub_adam_get_state(None, ptr(rows))),
        ("set_state: null", lambda: L.chub_adam_set_state(None, ptr(rows))),
        ("policy_get_weights_device: null", lambda: L.chub_policy_get_weights_device(None, 0, ptr(rows), ptr(rows), None)),
        ("policy_get_log_std_device: null", lambda: L.chub_policy_get_log_std_device(None, ptr(rows), None)),
        ("critic_get_weights_device: null", lambda: L.chub_critic_get_weights_device(None, 0, ptr(rows), ptr(rows), None)),
    ]
    for what, call in calls:
        assert call() == ERR_ARG, what
        assert last_error(), what
    assert L.chub_adam_destroy(None) == 0
    assert (rows == 0).all()


# ---- the restatement itself, and the conditions on the GPU cases' data
def test_the_sum_of_squares_lies_within_its_bound_of_fsum():
    rs = np.random.RandomState(2)
    for n in (1, 188, 1024, 1025, 84785):
        g = (rs.normal(size=n) * 10.0 ** rs.uniform(-3, 1, size=n)).astype(np.float32)
        a, b = math.sqrt(al.sum_of_squares(g)), al.fsum_norm(g)
        assert abs(a - b) <= n * al.U64 * b, (n, a, b)


def test_a_step_by_hand():
    """one parameter, two steps, every number written out"""
    a = al.Adam(1, [True], lr=0.5, betas=(0.5, 0.75), eps=0.0, weight_decay=0.0, max_grad_norm=0.0)
    th, st = a.step(np.array([1.0], dtype=np.float32), np.array([2.0], dtype=np.float32))
    # m = 1, v = 1, p1 = 0.5, p2 = 0.75: denom = 1 / 0.5 = 2, step = 0.5 / 0.5 = 1: theta = 1 - 1 * (1 / 2)
    assert th[0] == 0.5 and a.m[0] == 1.0 and a.v[0] == 1.0 and list(st) == [1.0, 2.0, 1.0, 0.0]
    th, st = a.step(th, np.array([np.inf], dtype=np.float32))
    assert th[0] == 0.5 and a.t == 1 and list(st) == [1.0, np.inf, 0.0, 1.0]
    blob = a.blob()
    b = al.Adam(1, [True])
    b.load(blob)
    assert (b.t, b.p1, b.p2, b.m[0], b.v[0]) == (1, 0.5, 0.75, 1.0, 1.0) and len(blob) == 40


def test_the_wrong_variants_show_on_the_gpu_cases_data():
    """the failure experiment on the CPU twin: a device that formed the bias correction from t before the increment, or decayed the
    biases, would differ from the restatement tests/test_gpu_adam.py compares it with -- the first on every case at the first step, the
    second on every case with weight_decay != 0"""
    import test_gpu_adam as tg
    for case in tg.all_step_cases():
        theta = al.flatten(case.layers, case.log_std)
        mask = al.decay_mask(case.shapes, case.G)
        right, _ = al.Adam(case.n, mask, **case.hyper).step(theta, case.grads[0])
        early, _ = al.Adam(case.n, mask, wrong="correction_before_increment", **case.hyper).step(theta, case.grads[0])
        biases, _ = al.Adam(case.n, mask, wrong="decay_on_biases", **case.hyper).step(theta, case.grads[0])
        assert not np.array_equal(right.view(np.uint32), early.view(np.uint32)), case.name
        differs = not np.array_equal(right.view(np.uint32), biases.view(np.uint32))
        assert differs == (case.hyper["weight_decay"] != 0.0), case.name
        assert np.array_equal(right[mask].view(np.uint32), biases[mask].view(np.uint32))


def test_the_gpu_cases_meet_the_condition_on_their_data():
    import test_gpu_adam as tg
    n = 0
    for case in tg.all_step_cases():
        for g in case.grads:
            if np.isfinite(g).all():
                assert al.scale_is_stable(g, case.hyper["max_grad_norm"]), case.name
                n += 1
        clipped = [al.clip_scale(np.sqrt(al.sum_of_squares(g)), case.hyper["max_grad_norm"]) < 1 for g in case.grads if np.isfinite(g).all()]
        if case.clips is not None:
            assert all(c == case.clips for c in clipped), (case.name, clipped)
    assert n >= 20
