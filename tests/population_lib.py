"""The numpy definition of a POPULATION of device actors (include/chub.h, "a population of actors"), and nothing else defines the expected
values of tests/test_population_cpu.py and tests/test_gpu_population.py: the perturbation noise as a pure function of (key, generation,
pair, layer, row, column), the antithetic members with their f32 roundings spelled out, the ES gradient estimate in f64 and the bound on
what a conforming device may differ from it by."""
import numpy as np

import policy_sample_lib as psl

F32 = np.float32
SITE_POPULATION = 16


def counters(l, rows, cols):
    """the noise's (counter word 0, counter word 1, word index) of every element of the augmented matrix [W | b] of layer l with `rows`
    outputs and `cols` = in + 1 columns: uint64 [rows, cols] x 2 and int [rows, cols]"""
    r, k = np.meshgrid(np.arange(rows, dtype=np.uint64), np.arange(cols, dtype=np.uint64), indexing="ij")
    c0 = (r << np.uint64(8)) | (k >> np.uint64(2))
    c1 = np.full_like(c0, (SITE_POPULATION << 16) | int(l))
    return c0, c1, (k & np.uint64(3)).astype(np.int64)


def eps(key, g, j, l, rows, cols):
    """eps(g, j, l, row, k) for row < rows, k < cols (cols = in + 1: column `in` is the bias) -> f32 [rows, cols]: the tabulated normal of
    word k & 3 of the Philox4x32-10 block with counter (row << 8 | k >> 2, 16 << 16 | l, g, j) under the key (low word, high word)"""
    k0, k1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    c0, c1, w = counters(l, rows, cols)
    blocks = psl.philox(c0, c1, int(g) & 0xFFFFFFFF, int(j) & 0xFFFFFFFF, k0, k1)
    words = np.take_along_axis(blocks, w[..., None], axis=-1)[..., 0]
    return psl.normal_from_word(words)


def shapes_of(layers):
    return [tuple(np.shape(W)) for W, _ in layers]


def members(theta_layers, sigma, key, g, P):
    """theta_layers [(W [out, in], b [out]), ..] f32 -> the P members, each a list of (W, b) f32: with d = f32(sigma * eps) member 2j is
    f32(theta + d) and member 2j + 1 is f32(theta - d)"""
    assert P >= 2 and P % 2 == 0
    sigma = F32(sigma)
    out = [[] for _ in range(P)]
    for j in range(P // 2):
        for l, (W, b) in enumerate(theta_layers):
            W, b = np.asarray(W, dtype=F32), np.asarray(b, dtype=F32)
            aug = np.concatenate([W, b[:, None]], axis=1)
            d = (sigma * eps(key, g, j, l, aug.shape[0], aug.shape[1])).astype(F32)
            plus, minus = (aug + d).astype(F32), (aug - d).astype(F32)
            out[2 * j].append((np.ascontiguousarray(plus[:, :-1]), np.ascontiguousarray(plus[:, -1])))
            out[2 * j + 1].append((np.ascontiguousarray(minus[:, :-1]), np.ascontiguousarray(minus[:, -1])))
    return out


def es_gradient(util, key, g, P, shapes):
    """util [P] f32, shapes [(out, in), ..] -> ([(gW, gb), ..] f64, [(bound W, bound b), ..]): per parameter
    g = sum_j ((double) util[2j] - (double) util[2j + 1]) * (double) eps(g, j, l, row, k), and the per-element bound
    2^-24 |g| + P 2^-52 sum_j |du_j eps_j| on what a device that accumulates in f64 in any order and rounds once to f32 may differ by"""
    util = np.asarray(util, dtype=F32).astype(np.float64)
    assert util.shape == (P,)
    du = util[0::2] - util[1::2]
    grads, bounds = [], []
    for l, (o, i) in enumerate(shapes):
        acc, mag = np.zeros((o, i + 1)), np.zeros((o, i + 1))
        for j in range(P // 2):
            t = du[j] * eps(key, g, j, l, o, i + 1).astype(np.float64)
            acc += t
            mag += np.abs(t)
        bound = 2.0 ** -24 * np.abs(acc) + P * 2.0 ** -52 * mag
        grads.append((acc[:, :-1], acc[:, -1]))
        bounds.append((bound[:, :-1], bound[:, -1]))
    return grads, bounds


def flat(layers):
    """[(W, b), ..] -> one vector, W row-major then b, layer after layer"""
    return np.concatenate([np.asarray(a, dtype=np.float64).ravel() for W, b in layers for a in (W, b)])


def param_count(shapes):
    return sum(o * (i + 1) for o, i in shapes)
