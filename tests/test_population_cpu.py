"""A population of device actors without a device (include/chub.h, "a population of actors"): the law and the uniqueness of the
perturbation noise as tests/population_lib.py defines it, the antithetic pairs on exact data, the ES estimator on a quadratic, the header /
binding / device-code agreement, and chub_population_param_count with its refusals."""
import ctypes as C
import os
import re

import numpy as np

import orclib
import policy_lib as pl
import population_lib as popl

ROOT = orclib.ROOT
F32 = np.float32
KEY = 0x0123456789ABCDEF


def chub():
    import charginghub_env_amd as m
    return m


def test_the_noise_is_standard_normal():
    """over the parameters of 13 -> 33 -> 47 and 8 pairs: the mean within 5 / sqrt(n) of 0, the variance within 5 sqrt(2 / n) of 1"""
    e = np.concatenate([popl.eps(KEY, 3, j, l, o, i + 1).astype(np.float64).ravel() for j in range(8) for l, (o, i) in enumerate([(33, 13), (47, 33)])])
    n = e.size
    assert n == 8 * (33 * 14 + 47 * 34)
    assert abs(e.mean()) <= 5 / np.sqrt(n), e.mean()
    assert abs(e.var() - 1.0) <= 5 * np.sqrt(2.0 / n), e.var()
    # generation, pair, layer and key each change the draw
    base = popl.eps(KEY, 3, 0, 0, 33, 14)
    for other in (popl.eps(KEY, 4, 0, 0, 33, 14), popl.eps(KEY, 3, 1, 0, 33, 14), popl.eps(KEY, 3, 0, 1, 33, 14), popl.eps(KEY ^ (1 << 40), 3, 0, 0, 33, 14)):
        assert (other != base).mean() > 0.99
    assert np.array_equal(base, popl.eps(KEY, 3, 0, 0, 33, 14))


def test_no_two_parameters_of_a_layer_share_a_counter_and_word():
    """the (counter word 0, word index) pairs of a layer, enumerated: all distinct, at the field widths' ends too (in = 512, row = 8193)"""
    for l, rows, cols in ((0, 33, 14), (1, 47, 34), (3, 8194, 257), (2, 256, 513), (0, 1, 1)):
        c0, c1, w = popl.counters(l, rows, cols)
        assert (c1 == ((16 << 16) | l)).all()
        ids = (c0.astype(np.uint64) << np.uint64(2)) | w.astype(np.uint64)
        assert np.unique(ids).size == rows * cols, (l, rows, cols)
        assert int(c0.max()) < 2 ** 32
    # the fields stay apart: the column group of in = 512 needs 8 bits, row 8193 sits above them
    c0, _, w = popl.counters(0, 8194, 513)
    assert int(c0[0, 512]) == 128 and int(w[0, 512]) == 0 and int(c0[8193, 0]) == 8193 << 8 and int(c0[8193, 512]) == (8193 << 8) | 128
    assert int(c0[1, 0]) > int(c0[0, 512])
    # layers differ in counter word 1, never in word 0
    assert not np.array_equal(popl.eps(KEY, 0, 0, 0, 4, 5), popl.eps(KEY, 0, 0, 1, 4, 5))


def test_members_are_antithetic_pairs():
    """dyadic theta (policy_lib.exact_layers: zeros and multiples of 1/8) and sigma = 2^-6, so d = sigma eps is exact: wherever theta + d and
    theta - d are both exact in f32 -- every zero of theta (more than 1000 parameters per pair) and the others whose d has no bit below
    theta's last place -- member 2j - theta == -(member 2j + 1 - theta) with no tolerance; and everywhere the two members are the
    roundings the definition spells out"""
    rs = np.random.RandomState(1)
    theta = pl.exact_layers(rs, [13, 33, 47])
    P, sigma = 6, F32(2.0 ** -6)
    mem = popl.members(theta, sigma, KEY, 5, P)
    checked = 0
    for j in range(P // 2):
        for l, (W, b) in enumerate(theta):
            aug = np.concatenate([W, b[:, None]], axis=1).astype(np.float64)
            d = (sigma * popl.eps(KEY, 5, j, l, *aug.shape)).astype(F32).astype(np.float64)
            plus = np.concatenate([mem[2 * j][l][0], mem[2 * j][l][1][:, None]], axis=1).astype(np.float64)
            minus = np.concatenate([mem[2 * j + 1][l][0], mem[2 * j + 1][l][1][:, None]], axis=1).astype(np.float64)
            exact = (plus == aug + d) & (minus == aug - d)
            assert exact[aug == 0].all(), "where theta is zero both members are d itself"
            assert np.array_equal((plus - aug)[exact], -(minus - aug)[exact])
            assert np.array_equal(plus.astype(F32), (aug + d).astype(F32)) and np.array_equal(minus.astype(F32), (aug - d).astype(F32))
            checked += int(exact.sum())
    assert checked > 1000
    # sigma = 0: every member is theta
    for m in popl.members(theta, 0.0, KEY, 5, 2):
        for (W, b), (W0, b0) in zip(m, theta):
            assert np.array_equal(W, W0) and np.array_equal(b, b0)


def test_the_estimator_points_along_the_gradient_of_a_quadratic():
    """f(theta) = -|theta - theta*|^2 over a 3 -> 2 layer (d = 8 parameters), K = 512 pairs: the cosine between es_gradient(f(members)) and
    the true gradient -2 (theta - theta*) is at least 0.9 (its expectation is about sqrt(K / (K + d)) = 0.99)"""
    rs = np.random.RandomState(4)
    P, key, g, sigma = 1024, 0xC0FFEE0000000017, 7, 0.05
    theta = [(rs.normal(size=(2, 3)).astype(F32), rs.normal(size=2).astype(F32))]
    star = rs.normal(size=8)
    mem = popl.members(theta, sigma, key, g, P)
    f = np.array([-np.sum((popl.flat(m) - star) ** 2) for m in mem])
    grads, bounds = popl.es_gradient(f.astype(F32), key, g, P, [(2, 3)])
    est = popl.flat(grads)
    true = -2.0 * (popl.flat(theta) - star)
    cos = est @ true / np.linalg.norm(est) / np.linalg.norm(true)
    print("cosine of the ES estimate and the true gradient: %.4f" % cos)
    assert cos >= 0.9, cos
    assert all(np.isfinite(bw).all() and np.isfinite(bb).all() for bw, bb in bounds)
    # utilities equal within every pair: exactly zero
    zero, _ = popl.es_gradient(np.repeat(rs.normal(size=P // 2), 2).astype(F32), key, g, P, [(2, 3)])
    assert not popl.flat(zero).any()


def test_header_binding_and_device_code_agree():
    from charginghub_env_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "chub.h")).read()
    csrc = os.path.join(ROOT, "charginghub-env_amd", "csrc")
    names = ["chub_population_param_count", "chub_population_create", "chub_population_destroy", "chub_population_perturb_device",
             "chub_population_set_member_device", "chub_population_get_member_device", "chub_population_set_member", "chub_population_get_member",
             "chub_population_copy_members_device", "chub_population_act_device", "chub_population_run_steps", "chub_population_es_gradient_device"]
    for fn in names:
        assert fn in _lib.EXPORTED and re.search(r"\bint %s\(" % fn, hdr), fn
    assert "(row << 8 | (k >> 2), 16 << 16 | l, g, j)" in hdr, "the header carries the noise counter verbatim"
    dev, pol = open(os.path.join(csrc, "chub_device.h")).read(), open(os.path.join(csrc, "chub_policy.h")).read()
    assert re.search(r"SITE_POPULATION = 16\b", dev) and re.search(r"kPopulationSite = 16u", pol)
    assert popl.SITE_POPULATION == 16
    assert "static_assert((uint32_t) SITE_POPULATION == kPopulationSite" in open(os.path.join(csrc, "chub_runtime.cpp")).read()


def test_param_count_is_the_formula_and_refuses_without_a_device():
    m = chub()
    from charginghub_env_amd import _lib
    lib = m.load_library()
    for piles in ([20, 25], [1, 1], [64, 64]):
        cfg = m.make_config(piles, ["fast", "slow"])
        S, D = sum(piles), 2 + 4 * sum(1 for p in piles if p > 0) + 3
        for hidden in ((), (33,), (64, 33)):
            for head, A in (("piles", S + 2), ("loads", 4)):
                sizes = [D] + list(hidden) + [A]
                spec = _lib.policy_spec(sizes[1:], ("obs",), head)
                n = C.c_int64(-7)
                assert lib.chub_population_param_count(C.byref(cfg), C.byref(spec), C.byref(n)) == 0, lib.chub_last_error()
                assert n.value == sum(o * (i + 1) for i, o in zip(sizes[:-1], sizes[1:])) == popl.param_count(list(zip(sizes[1:], sizes[:-1])))
    cfg = m.make_config([20, 25], ["fast", "slow"])
    spec = _lib.policy_spec([64, 47], (("pile_obs", ("car", "soc")), "obs"))  # F = 90 + 13
    n = C.c_int64(-7)
    assert lib.chub_population_param_count(C.byref(cfg), C.byref(spec), C.byref(n)) == 0 and n.value == 64 * 104 + 47 * 65
    n = C.c_int64(-7)
    for args in ((None, C.byref(spec), C.byref(n)), (C.byref(cfg), None, C.byref(n)), (C.byref(cfg), C.byref(spec), None)):
        assert lib.chub_population_param_count(*args) == -1 and lib.chub_last_error() == b"null argument"
    bad = _lib.policy_spec([64, 46])
    assert lib.chub_population_param_count(C.byref(cfg), C.byref(bad), C.byref(n)) == -1 and b"the head's output count, 47" in lib.chub_last_error()
    bad = _lib.policy_spec([257, 47])
    assert lib.chub_population_param_count(C.byref(cfg), C.byref(bad), C.byref(n)) == -1 and b"hidden widths are 1 .. 256" in lib.chub_last_error()
    assert n.value == -7, "nothing is written on a refusal"
    # the device calls refuse null arguments before anything else
    block = C.create_string_buffer(64)
    live = C.addressof(block)
    h = C.c_void_p()
    assert lib.chub_population_create(None, 2, 1, C.byref(h)) == -1 and lib.chub_last_error() == b"null argument"
    assert lib.chub_population_destroy(None) == 0
    for call in (lambda: lib.chub_population_perturb_device(None, None, None, 0.1, 0, None),
                 lambda: lib.chub_population_set_member_device(None, 0, 0, live, live, None),
                 lambda: lib.chub_population_get_member(None, 0, 0, live, live),
                 lambda: lib.chub_population_copy_members_device(None, live, live, 1, None),
                 lambda: lib.chub_population_act_device(None, None, live, 13, None, live, None, None, None),
                 lambda: lib.chub_population_run_steps(None, None, 0, live, live, None, 0, 4, None),
                 lambda: lib.chub_population_es_gradient_device(None, live, 0, live, live, None)):
        assert call() == -1 and lib.chub_last_error() == b"null argument"
