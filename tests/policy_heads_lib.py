"""The cases of tests/test_policy_heads_cpu.py and tests/test_gpu_policy_heads.py: hubs, seeds, weights and keys, made HERE so that the CPU
test holds the definition alone to the GPU test's caps on the GPU test's own data.  Nothing is defined here: the expected values are
policy_lib's forward pass, policy_sample_lib's Sample (its Philox block and tabulated normal, which tests/test_policy_sample_cpu.py holds
to the oracle) and pile_set_lib's masked log-probability and f32 GAE.

The hubs are chosen by where the head's rows fall in k_policy's accumulator layout (chub_policy.hip): output row n lies in tile n >> 5, in
the half-wave (n >> 2) & 1 and in the run of four rows n >> 2; a bit word holds two tiles; the head has max(ceil((S + 2) / 32),
2 ceil(S / 64)) tiles and a workgroup at most four waves.  head_geometry() states that arithmetic once."""
import numpy as np

import pile_set_lib as psl
import policy_lib as pl
import policy_sample_lib as ps

F32 = np.float32

# one hub per alignment of the tail means (rows S, S + 1) against runs of 4, half-waves of 8, tiles of 32 and words of 64, each the smallest
ALIGN_HUBS = ([3, 0], [4, 3], [20, 11], [31, 32], [64, 63], [30, 0], [0, 62])
# (hub, n): three and five bit words, more head tiles than waves, the step kernels' chunked forms, and the largest station
BIG_HUBS = (([100, 70], 33), ([255, 0], 33), ([300, 20], 33), ([4096, 3], 3))
NETS = ((), (33,), (256, 64))
LOADS_HUBS = ([20, 11], [300, 20], [4096, 3])
UNDECIDED_CAP = 0.001  # the cap of tests/test_gpu_policy_sample.py
KEY = ps.KEY


def hub_id(p):
    return "%dx%d" % tuple(p)


def big_n(piles):
    for p, n in BIG_HUBS:
        if list(p) == list(piles):
            return n
    return None


def sampled_n(piles):
    """envs of a sampled case: 70 (two env tiles and a ragged one) on the alignment hubs, the table's n on the big ones"""
    n = big_n(piles)
    return ps.N_SMALL if n is None else n


ALL_HUBS = tuple(ALIGN_HUBS) + tuple(p for p, _ in BIG_HUBS)


def head_geometry(S):
    """-> dict of where the PILES head's rows fall: W u64 words, plain = ceil((S + 2) / 32) tiles, tiles after the bump to 2 W, and for the
    two tail rows S, S + 1 their run, half-wave-of-a-tile index and tile"""
    W = (S + 63) // 64
    plain = (S + 2 + 31) // 32
    return dict(W=W, plain=plain, tiles=max(plain, 2 * W), run=(S >> 2, (S + 1) >> 2), half=(S >> 3, (S + 1) >> 3), tile=(S >> 5, (S + 1) >> 5))


# ---- 1. the deterministic actor on exact data
def exact_actor_case(piles, hidden, n):
    """-> (layers, obs [n, D], a [n, A] f64): relu / clip on dyadic data, every partial sum exact in f32"""
    S, D = sum(piles), ps.obs_dim(piles)
    rs = np.random.RandomState(7000 + 31 * S + 7 * len(hidden) + sum(hidden) + n)
    layers = pl.exact_layers(rs, [D] + list(hidden) + [S + 2])
    obs = pl.exact_obs(rs, n, D)
    pl.assert_exact(obs, layers)
    return layers, obs, pl.forward(obs, layers, "relu", "clip")[0]


# ---- 2. a head whose device layout k_policy_relayout's grid (1024 x 256 threads) covers only in a second pass
RELAYOUT_HUB, RELAYOUT_N, RELAYOUT_HIDDEN = [4096, 3], 3, 256
RELAYOUT_GRID = 1024 * 256


def relayout_case():
    """-> (layers, [head1, head2], obs, [a0, a1, a2]): the policy as built, two replacement heads, and the definition's outputs with each.
    Outputs 1024 and above lie in tiles 32 and above, whose elements k_policy_relayout reaches only when it goes round its loop again:
    they are asserted to vary within a stage and to differ between stages, so that neither zeros nor the previous head can pass."""
    piles = RELAYOUT_HUB
    S, D = sum(piles), ps.obs_dim(piles)
    geo = head_geometry(S)
    first_pass_rows = RELAYOUT_GRID // (32 * RELAYOUT_HIDDEN) * 32
    assert geo["tiles"] * RELAYOUT_HIDDEN * 32 > RELAYOUT_GRID and first_pass_rows == 1024 < S
    rs = np.random.RandomState(8128)
    layers = pl.exact_layers(rs, [D, RELAYOUT_HIDDEN, S + 2])
    heads = [pl.exact_layers(rs, [RELAYOUT_HIDDEN, S + 2])[0] for _ in range(2)]
    obs = pl.exact_obs(rs, RELAYOUT_N, D)
    outs = []
    for head in [layers[1]] + heads:
        net = [layers[0], head]
        pl.assert_exact(obs, net)
        outs.append(pl.forward(obs, net, "relu", "clip")[0])
    for k, a in enumerate(outs):
        late = a[:, first_pass_rows:]
        assert len(np.unique(late)) > 4 and (late != 0).mean() > 0.25, ("the outputs of the later passes say nothing", k)
        if k:
            assert (late != outs[k - 1][:, first_pass_rows:]).mean() > 0.25, ("the previous head would pass", k)
    return layers, heads, obs, outs


# ---- 3. the sampled actor on exact data: policy_sample_lib.exact_case, cut to the hub's n
def sampled_case(piles, head="piles"):
    """-> (layers, obs [n, D], log_std, z, err_z)"""
    layers, obs, ls = ps.exact_case(piles, head)
    obs = np.ascontiguousarray(obs[:sampled_n(piles)])
    z, err = ps.pre_squash(obs, layers, "relu")
    return layers, obs, ls, z, err


def sampled_definition(piles, head, tick, z, err, ls):
    return ps.Sample(z, err, head, sum(piles), KEY, tick, np.arange(len(z)), ls)


# ---- 4. a log-probability that cannot hide a term
LIVE_LOG_STD = (-0.5, 0.25)
LIVE_TAIL = (0.25, -0.5)
SATURATED = 64.0
LIVE_TICKS = (2, 11)  # the handle's next tick after a reset, and after another reset and 8 steps


def live_piles(S, rs):
    """piles 0 and 1, both sides of the first tile and word boundaries, the last nine, four seeded places"""
    fixed = [0, 1] + list(range(30, 34)) + list(range(62, 66)) + list(range(S - 9, S))
    fixed += [int(b) for b in rs.choice(S, size=min(4, S), replace=False)]
    return np.array(sorted(set(b for b in fixed if 0 <= b < S)), dtype=np.int64)


def live_case(piles):
    """zero weights: z is the bias exactly.  Saturated piles (+64 on even, -64 on odd piles: the decision is certain, the term below
    2e-28) and about 25 live ones (+-k/8, k = 4 .. 16: each term at least softplus(-2) = 0.127).
    -> (layers, obs [n, D], log_std, live pile indices)"""
    S, D, n = sum(piles), ps.obs_dim(piles), sampled_n(piles)
    rs = np.random.RandomState(404 + S)
    live = live_piles(S, rs)
    b = np.where(np.arange(S) % 2 == 0, SATURATED, -SATURATED)
    b[live] = rs.choice([-1.0, 1.0], size=len(live)) * rs.randint(4, 17, size=len(live)) / 8.0
    b = np.concatenate([b, LIVE_TAIL]).astype(F32)
    layers = [(np.zeros((S + 2, D), dtype=F32), b)]
    return layers, pl.exact_obs(rs, n, D), np.asarray(LIVE_LOG_STD, dtype=F32), live


def live_definition(piles, layers, obs, ls, tick):
    """the definition with err_z = 0, after asserting that z IS the bias"""
    z, _ = ps.pre_squash(obs, layers)
    assert np.array_equal(z, np.broadcast_to(layers[0][1].astype(np.float64), z.shape)), "z is the bias exactly"
    return ps.Sample(z, np.zeros_like(z), "piles", sum(piles), KEY, tick, np.arange(len(z)), ls)


def smallest_live_term(layers, live):
    """whatever the decision, a live pile's term is at least softplus(-|z|)"""
    return float(ps.softplus(-np.abs(layers[0][1][live].astype(np.float64))).min())


def assert_live_condition(d, layers, live, on=None, in_set=None):
    """the condition on the DATA under which the log-probability check sees every live term: the definition's bound is at most a quarter
    of the smallest live term -> (largest bound, smallest term)"""
    on = d.on if on is None else on
    _, bound = d.logp(on) if in_set is None else psl.masked_logp(d, on, in_set)
    term = smallest_live_term(layers, live)
    assert bound.max() <= term / 4, ("a live term could hide inside the bound", bound.max(), term)
    return float(bound.max()), term


# ---- 5. feature rows wider than 256
WIDE_HUB, WIDE_N, WIDE_INPUTS, WIDE_HIDDEN = [300, 3], 33, ("obs", ("pile_obs", ("car",))), 64


def wide_case():
    """F = 13 + 303 = 316.  -> (F, layers [F, 64, A], obs [n, D], (mean, inv_std, clip)): dyadic mean and inv_std, so that the normalised
    row stays on policy_lib.assert_exact's grid of 2^-4 for observation entries AND for a car column of whole numbers"""
    S, D = sum(WIDE_HUB), ps.obs_dim(WIDE_HUB)
    F = D + S
    rs = np.random.RandomState(316)
    layers = pl.exact_layers(rs, [F, WIDE_HIDDEN, S + 2])
    obs = pl.exact_obs(rs, WIDE_N, D)
    mean = (rs.randint(-4, 5, size=F) / 4.0).astype(F32)
    inv_std = rs.choice([1.0, 2.0], size=F).astype(F32)
    return F, layers, obs, (mean, inv_std, 2.0)


def wide_normalised(obs, car, norm):
    """the normalised feature row of wide_case on the car column the handle shows, checked to be exact data"""
    x = pl.normalise(pl.features([obs, car]), *norm)
    assert np.array_equal(x * 16, np.round(x * 16)) and (np.abs(x) == norm[2]).any() and (np.abs(x) < norm[2]).any()
    return x


# ---- 6. the closed loop on a hub whose stations take the step kernels' chunked forms
LOOP_HUB, LOOP_N = [300, 20], 9

# ---- 7. GAE at the edges of k_gae's chunks of eight steps, counted from the END of the rollout
GAE_CHUNK = 8
GAE_T = (7, 8, 9, 13, 17)
GAE_DONES = ("chunk_last", "chunk_first", "pair", "every", "none")
GAE_N = 300  # two workgroups of 256 lanes, the second ragged


def gae_done_rows(T, dones):
    """the steps at which `dones` may fire, as bool [T].  Step t is element k = T - 1 - t of the backward sweep: the last element of a
    chunk has k % 8 == 7 (and t = 0 ends the partial chunk), the first has k % 8 == 0"""
    k = T - 1 - np.arange(T)
    if dones == "chunk_last":
        return (k % GAE_CHUNK == GAE_CHUNK - 1) | (np.arange(T) == 0)
    if dones == "chunk_first":
        return k % GAE_CHUNK == 0
    return np.full(T, dones in ("pair", "every"))


def gae_edge_case(T, dones, with_final, N=GAE_N, D=13):
    """pile_set_lib.gae_case's blocks with done placed per env from a seed: at a chunk's last or first element for half of the envs each,
    at two consecutive steps (for the even envs the pair straddles the first chunk edge where there is one), at every step, nowhere.
    -> (packed [T, N, D + 2], values [T + 1, N], final [N] or None)"""
    rs = np.random.RandomState(5000 + 100 * T + 10 * GAE_DONES.index(dones) + int(with_final))
    packed = rs.normal(size=(T, N, D + 2)).astype(F32)
    packed[:, :, D] = (rs.normal(size=(T, N)) * 3.0 - 1.0).astype(F32)
    done = np.zeros((T, N), dtype=bool)
    rows = gae_done_rows(T, dones)
    if dones in ("chunk_last", "chunk_first"):
        done[rows] = rs.rand(int(rows.sum()), N) < 0.5
    elif dones == "pair":
        t0 = rs.randint(0, T - 1, size=N)
        if T > GAE_CHUNK:
            t0[::2] = T - GAE_CHUNK - 1
        done[t0, np.arange(N)] = True
        done[t0 + 1, np.arange(N)] = True
    elif dones == "every":
        done[:] = True
    packed[:, :, D + 1] = done
    values = (rs.normal(size=(T + 1, N)) * 5.0).astype(F32)
    final = (rs.normal(size=N) * 5.0).astype(F32) if with_final else None
    return packed, values, final
