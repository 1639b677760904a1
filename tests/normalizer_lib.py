"""Running feature statistics and the normaliser derived from them, in numpy: the definition of include/chub.h's section "running feature
statistics".  A batch's sums are EXACT here (math.fsum per column over the f64 deviations from the pivot), so what a device may differ by is
its own summation error alone; `bounds` is the worst case of f64 summation for it.  No GPU needed."""
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -53  # unit roundoff of f64


def zero_state(F):
    return 0.0, np.zeros(F, dtype=np.float64), np.zeros(F, dtype=np.float64)


def pivot(state, x):
    """K: the state's mean once anything is counted, else row 0 of the batch -- whether row 0 itself counts or not"""
    n, mean, _ = state
    return np.array(mean, dtype=np.float64) if n > 0 else np.asarray(x, dtype=F32)[0].astype(np.float64)


def batch_sums(x, K, rows=None):
    """-> (n_b, S1 [F], S2 [F], max|d| [F]): d = (double) x - K over the counted rows (rows: bool [R] or None = all), each d and each
    d * d rounded once in f64, their sums exact and rounded once"""
    x = np.asarray(x, dtype=F32)
    d = x.astype(np.float64) - K[None, :]
    if rows is not None:
        d = d[np.asarray(rows, dtype=bool)]
    F = x.shape[1]
    if len(d) == 0:
        return 0, np.zeros(F), np.zeros(F), np.zeros(F)
    q = d * d
    S1 = np.array([math.fsum(d[:, f]) for f in range(F)], dtype=np.float64)
    S2 = np.array([math.fsum(q[:, f]) for f in range(F)], dtype=np.float64)
    return len(d), S1, S2, np.abs(d).max(axis=0)


def merge(state, K, n_b, S1, S2):
    """the batch's sums about K into the state (Chan et al.); n_b == 0 returns the state as it is"""
    n, mean, m2 = state
    if n_b == 0:
        return n, np.array(mean, dtype=np.float64), np.array(m2, dtype=np.float64)
    nb = float(n_b)
    with np.errstate(invalid="ignore", over="ignore"):
        t = S2 - (S1 * S1) / nb
        m2b = np.where(t < 0.0, 0.0, t)  # (a NaN stays one)
        n1 = n + nb
        if n > 0:
            db = S1 / nb
            return n1, K + S1 / n1, (m2 + m2b) + (db * db) * ((n * nb) / n1)
        return n1, K + S1 / nb, m2b


def update(state, x, rows=None):
    """one chub_moments_update_device by the definition -> (state', K, n_b, sum d d [F], max|d| [F])"""
    K = pivot(state, x)
    n_b, S1, S2, dmax = batch_sums(x, K, rows)
    return merge(state, K, n_b, S1, S2), K, n_b, S2, dmax


def bounds(R, ref_state, S2, dmax):
    """what a device that adds R terms in f64 in some order may differ by: (bound on |mean - ref|, bound on |M2 - ref|), per feature"""
    _, mean, m2 = ref_state
    return (R + 8) * U * (dmax + np.abs(mean)), 4 * (R + 8) * U * (S2 + m2)


def env_rows(mask, R):
    """bool [R]: row r belongs to env r % N and counts where the mask's byte of that env is non-zero"""
    mask = np.asarray(mask)
    return mask[np.arange(R) % len(mask)] != 0


def from_moments(state, eps):
    """-> (mean32, inv_std32): (float) mean and (float) (1 / sqrt(M2 / n + eps)), every f64 operation rounded once (numpy's f64 division and
    square root are IEEE); None while nothing is counted (the normaliser is left alone)"""
    n, mean, m2 = state
    if not n > 0:
        return None
    return np.asarray(mean, dtype=np.float64).astype(F32), (1.0 / np.sqrt(np.asarray(m2, dtype=np.float64) / n + eps)).astype(F32)


def normalise(x, mean, inv_std, clip):
    """the kernel's normalisation in f32: subtract, multiply, clamp, each rounded once"""
    x, mean, inv_std, clip = np.asarray(x, dtype=F32), np.asarray(mean, dtype=F32), np.asarray(inv_std, dtype=F32), F32(clip)
    y = ((x - mean).astype(F32) * inv_std).astype(F32)
    return np.minimum(np.maximum(y, -clip), clip).astype(F32)
