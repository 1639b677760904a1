"""The numpy definition of the device actor (include/chub.h, "an actor on the device"), and nothing else defines the expected values of
tests/test_policy_cpu.py and tests/test_gpu_policy.py: feature concatenation, normalisation in f32, the forward pass in f64, the squash,
the pile-bit predicate with the step kernels' threshold, and a rigorous per-output bound on what an f32 fmaf chain in ANY order may differ
from the f64 value by."""
import numpy as np

F32 = np.float32
# a pile is on iff its squashed f32 action a >= this: f32((a + 1) / 2) >= 0.5, the step kernels' predicate (kActOnThreshold, chub_kernels.hip)
ON_THRESHOLD = F32(-2.0 ** -25)
U = 2.0 ** -24          # unit roundoff of f32
TANH_ERR = 4 * 2.0 ** -24   # 4 ulp of a result in [0.5, 1), the largest tanh takes: a few ulp for the device library's tanhf
TINY = 2.0 ** -149      # one underflow per term at most


def features(blocks):
    """the feature row: the blocks' rows side by side, [N, F] f32 (a block of any shape [N, ...] is flattened per env)"""
    return np.concatenate([np.ascontiguousarray(b, dtype=F32).reshape(len(b), -1) for b in blocks], axis=1)


def normalise(x, mean, inv_std, clip):
    """x <- min(max((x - mean) * inv_std, -clip), clip), every operation rounded to f32"""
    x, mean, inv_std, clip = np.asarray(x, dtype=F32), np.asarray(mean, dtype=F32), np.asarray(inv_std, dtype=F32), F32(clip)
    y = ((x - mean).astype(F32) * inv_std).astype(F32)
    return np.minimum(np.maximum(y, -clip), clip).astype(F32)


def gamma(k):
    return k * U / (1.0 - k * U)


def forward(x, layers, hidden_act="tanh", squash="tanh"):
    """x [N, F] f32 (already normalised), layers [(W [out, in], b [out]), ...] f32 -> (a, bound), both f64 [N, out of the last layer]:
    the squashed outputs evaluated in f64, and per output a bound on |device value - a| for a device that rounds every product once and
    accumulates in f32 from the bias in some order.  Per layer of fan-in K the chain's own error is gamma * (|b| + sum |w| |h|) with
    gamma = (K + 2) u / (1 - (K + 2) u) over the values the device actually holds (|h| + the incoming error), the incoming error goes
    through |W|, both activations are 1-Lipschitz, relu and clip are exact, tanhf is within a few ulp."""
    h = np.asarray(x, dtype=np.float64)
    err = np.zeros_like(h)
    for l, (W, b) in enumerate(layers):
        W, b = np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64)
        K = W.shape[1]
        z = h @ W.T + b
        held = np.abs(h) + err
        err = gamma(K + 2) * (np.abs(b) + held @ np.abs(W).T) + err @ np.abs(W).T + K * TINY
        last = l == len(layers) - 1
        kind = squash if last else hidden_act
        if kind == "tanh":
            h, err = np.tanh(z), err + TANH_ERR
        elif kind == "relu":
            h = np.maximum(z, 0.0)
        elif kind == "clip":
            h = np.minimum(np.maximum(z, -1.0), 1.0)
        else:
            raise ValueError(kind)
    return h, err


def pile_bits(a, S):
    """squashed f32 actions [N, >= S] -> uint64 [N, ceil(S / 64)]: bit b of word w = (a[64 w + b] >= ON_THRESHOLD), bits from S up zero"""
    a = np.asarray(a, dtype=F32)
    on = a[:, :S] >= ON_THRESHOLD
    W = (S + 63) // 64
    packed = np.packbits(on, axis=1, bitorder="little")
    pad = W * 8 - packed.shape[1]
    if pad:
        packed = np.concatenate([packed, np.zeros((len(a), pad), dtype=np.uint8)], axis=1)
    return np.ascontiguousarray(packed).view("<u8").reshape(len(a), W)


def unpack_bits(bits, S):
    """uint64 [N, W] -> bool [N, S]"""
    b = np.ascontiguousarray(bits, dtype="<u8").view(np.uint8).reshape(len(bits), -1)
    return np.unpackbits(b, axis=1, bitorder="little")[:, :S].astype(bool)


def decided(a, bound):
    """where the f64 value is further from the threshold than the bound: there every conforming device sets the same bit"""
    return np.abs(np.asarray(a, dtype=np.float64) - float(ON_THRESHOLD)) > bound


# ---- data on which every partial sum is exact in f32, so that any summation order gives the same bits
def exact_layers(rs, sizes, nonzeros=8):
    """layers for sizes = [F, w0, w1, ..]: per output at most `nonzeros` weights of +-1/8 or +-2/8 at random inputs, the rest zero; biases
    multiples of 1/8 in [-1/2, 1/2].  ASYMMETRIC: no row equals another's transpose image."""
    layers = []
    for fan_in, out in zip(sizes[:-1], sizes[1:]):
        W = np.zeros((out, fan_in), dtype=F32)
        for n in range(out):
            cols = rs.choice(fan_in, size=min(nonzeros, fan_in), replace=False)
            W[n, cols] = rs.choice([-2, -1, 1, 2], size=len(cols)).astype(F32) / F32(8)
        b = rs.randint(-4, 5, size=out).astype(F32) / F32(8)
        layers.append((W, b))
    return layers


def exact_obs(rs, n, width):
    """multiples of 2^-4 in [-2, 2]"""
    return (rs.randint(-32, 33, size=(n, width)).astype(F32) / F32(16)).astype(F32)


def assert_exact(x, layers):
    """every partial sum of relu layers on this data is a multiple of 2^-q below 2^(24 - q): exact in f32 whatever the order"""
    mag = np.abs(np.asarray(x, dtype=np.float64)).max(initial=0.0)
    q = 4
    for W, b in layers:
        mag = float(np.abs(W).sum(axis=1).max()) * mag + float(np.abs(b).max())
        q += 3
        assert mag * 2.0 ** q < 2.0 ** 24, ("not exact in f32", mag, q)
