"""The cases of tests/test_gpu_grid_pass.py and the arithmetic that says they are the right ones (tests/test_grid_pass_cpu.py): plain Python
restatements of three pieces of index arithmetic -- the population launch's tile order (k_policy<PolicyPopArgs>), the moments stream's
launch shape and loop trips (chub_moments_create, chub_moments_update_device, k_moments) and the ES gradient's chunks of pairs
(chub_population_create) -- and, for tests/test_gpu_grad_trips.py and tests/test_grad_trips_cpu.py, of a fourth: the gradient kernels'
workgroups and the tiles each of them walks (grad_blocks, k_policy_grad, k_critic).  They choose and check cases; they are never the expected value of a kernel's output: those stay
tests/population_lib.py's and tests/normalizer_lib.py's.  No GPU needed."""
import numpy as np

import normalizer_lib as nl

ENV_TILE = 32     # kPolicyEnvTile: the envs of one workgroup of the actor launch
XCDS = 8          # the dispatcher hands workgroup b to XCD b % 8
LANES = 256       # kMomentsLanes
AHEAD = 8         # kMomentsAhead: passes a lane has in flight = grid passes per trip of k_moments' loop
BLOCKS_PER_CU = 4             # kMomentsBlocksPerCu
PARTIAL_BYTES = 4 << 20       # kMomentsPartialBytes
CHUNK_PAIRS = 16              # kPopChunkPairs
MAX_CHUNKS = 64               # kPopMaxChunks
POP_PARTIAL_BYTES = 64 << 20  # kPopPartialBytes
CUS = (64, 256, 304)          # the device sizes the case arithmetic is checked at (the GPU tests take theirs from chub_device_info)


# ---- the population launch's tile order
def tile_of(b, nb):
    """the tile of 32 envs workgroup b of nb takes: XCD x = b % 8 serves one contiguous run of tiles, the first nb % 8 runs one tile longer"""
    q, r, x = nb >> 3, nb & 7, b & 7
    return x * q + np.minimum(x, r) + (b >> 3)  # (b: an int or an array of them)


def xcd_runs(nb):
    """per XCD x the sorted tiles of the workgroups b = x (mod 8)"""
    tiles = tile_of(np.arange(nb), nb)
    return [sorted(int(t) for t in tiles[x::XCDS]) for x in range(XCDS)]


POP_HUB, POP_HIDDEN = [20, 25], (33,)
POP_CASES = ((10, 32), (16, 32), (6, 64), (6, 96), (22, 32), (70, 32))  # (P, E)
POP_PERTURB = ((22, 32), (70, 32))  # perturb held for every member here: 11 and 35 pairs
POP_OWN_HANDLE = ((10, 32), (0, 1, 4, 9))  # (P, E) and the members held against a handle of their own


def pop_grid(P, E):
    """-> (workgroups, tiles per member) of the population's actor launch"""
    assert E % ENV_TILE == 0
    return P * E // ENV_TILE, E // ENV_TILE


def edge_tile(P, E):
    """the first tile of XCD 1's run"""
    return int(tile_of(1, pop_grid(P, E)[0]))


def edge_mask(P, E):
    """bool [P E]: the rows 32 t - 5 .. 32 t + 6 around the first tile t of XCD 1's run -- the edge of an XCD's run and of a member at once
    (tests/test_grid_pass_cpu.py) -- and the last row"""
    t = edge_tile(P, E)
    mask = np.zeros(P * E, bool)
    mask[ENV_TILE * t - 5:ENV_TILE * t + 7] = True
    mask[-1] = True
    return mask


# ---- the moments stream
def moments_shape(F, cus):
    """-> (L, RW, grid): lanes along a row, rows per workgroup pass, workgroups at most (four per compute unit, the partials within 4 MiB)"""
    L = min(F, LANES)
    return L, LANES // L, min(BLOCKS_PER_CU * max(cus, 1), PARTIAL_BYTES // (8 * (1 + 2 * F)))


def launch_of(R, rw, grid):
    """-> (passes, workgroups launched) of one update of R rows"""
    passes = -(-R // rw)
    return passes, min(passes, grid)


def trips_of(R, rw, grid):
    """the largest number of trips of k_moments' loop any workgroup makes (workgroup 0's): a trip covers AHEAD passes of the whole grid"""
    passes, blocks = launch_of(R, rw, grid)
    return -(-passes // (blocks * AHEAD))


def trips(R, F, cus):
    _, rw, grid = moments_shape(F, cus)
    return trips_of(R, rw, grid)


def live_of(R, rw, grid, b, t, r_in=0):
    """ok[k] before the mask, k = 0 .. AHEAD - 1, of row r_in of workgroup b's pass in trip t; None where the workgroup makes no trip t"""
    passes, blocks = launch_of(R, rw, grid)
    if b >= blocks or b + t * AHEAD * blocks >= passes:
        return None
    return [(b + (t * AHEAD + k) * blocks) * rw + r_in < R for k in range(AHEAD)]


def above(x, n):
    """the smallest multiple of n above x"""
    return (x // n + 1) * n


MOMENTS_N, MOMENTS_PILES = 70, [3, 2]
LONG_F = (1, 23, 64, 65, 257, 512)
LONG_LD_F = 65     # the F that also runs with two floats between the rows
RAGGED_F = 64
DETERMINISM_F = 65
WIDE_F, WIDE_PILES = (64, 512), [1, 1]
EDGE_F = (128, 129, 255, 256, 257)


def long_rows(rw, grid):
    """two trips: one whole trip of the grid, 257 rows and the rest of an env block into the second"""
    return above(AHEAD * grid * rw + 257, MOMENTS_N)


def ragged_rows(rw, grid):
    """three trips: two whole ones, three passes and a row into the third, whose k = 1 .. 7 are past R"""
    return above(2 * AHEAD * grid * rw + 3 * rw + 1, MOMENTS_N)


def wide_envs(rw, grid):
    """a handle whose envs outnumber a grid pass's rows: the env walk's step is the unreduced grid RW"""
    return above(grid * rw + 900, 10)


def wide_rows(rw, grid):
    """3 N: with a mask R is a multiple of N (include/chub.h; 3 N + 17 is refused)"""
    return 3 * wide_envs(rw, grid)


def edge_rows(rw, grid):
    return (1, 257, above(grid * rw + 256, MOMENTS_N))


def random_mask(N, seed):
    """60 % of the envs, env 0 (row 0: the pivot of an empty state) masked out and env 1 counted"""
    mask = np.random.RandomState(seed).uniform(size=N) < 0.6
    mask[:2] = (False, True)
    return mask


def moments_batch(columns, F, R, k, own_last=False):
    """the k-th batch [R, F] of a moments case, through tests/test_gpu_normalizer.py's `columns` (passed in: this file needs no GPU module);
    own_last: the last column gets a scale and an offset that no other column has"""
    x = columns(np.random.RandomState(7919 * F + 2 * (R % 100003) + k), R, F)
    if own_last:
        x[:, -1] = (x[:, -1] * np.float32(3e-3) + np.float32(41.0)).astype(np.float32)
    return x


def drop_one_row(x, rows=None):
    """per counted row, how far leaving that one row out moves the mean, over tests/normalizer_lib.py's bound on the mean for a batch of
    these R rows from zeros, at the best column: max_f |mean_f - x[r, f]| / (n - 1) / bound_f.  Above 1 the bound sees that row missing."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    R = len(x)
    d = x - x[0][None, :]
    if rows is not None:
        x, d = x[rows], d[rows]
    n, mean = len(x), x.mean(axis=0)
    b_mean, _ = nl.bounds(R, (n, mean, np.zeros_like(mean)), np.zeros_like(mean), np.abs(d).max(axis=0))
    return (np.abs(x - mean[None, :]) / (n - 1) / b_mean[None, :]).max(axis=1)


# ---- the ES gradient's chunks
ES_P, ES_E, ES_HUB, ES_HIDDEN = 2100, 32, [1, 1], (33,)


def es_items(shapes):
    """lanes of the gradient's first launch for the largest layer: out x (in / 4 + 1) column groups"""
    return max(o * (i // 4 + 1) for o, i in shapes)


def es_chunks(P, items):
    """-> (chunk_pairs, chunks): at least 16 pairs a chunk, at most 64 chunks, the partials [chunks][items][4] f64 within 64 MiB"""
    pairs = P // 2
    chunks = min(-(-pairs // CHUNK_PAIRS), MAX_CHUNKS)
    chunks = max(1, min(chunks, POP_PARTIAL_BYTES // (items * 32)))
    chunk_pairs = -(-pairs // chunks)
    return chunk_pairs, -(-pairs // chunk_pairs)


# ---- the gradient kernels' walk (k_policy_grad, k_critic: chub_runtime.cpp's grad_blocks, the loop `tile = b; tile < n_tiles; tile += blocks`)
GRAD_TILE = 32                  # rows of one tile of the walk
GRAD_MAX_BLOCKS = 512           # kGradMaxBlocks
GRAD_PARTIAL_BYTES = 256 << 20  # kGradPartialBytes
GRAD_REG_PAIRS = 16             # kGradRegSlots * kGradWaves: dW tiles a workgroup keeps in registers
GRAD_LDS_ROWS = 160 * 1024 // (33 * 4)  # kGradLdsBytes / (kGradRowStride floats): 1241
GRAD_SCRATCH_ROWS = 16          # kGradScratchRows
VALUE_BLOCKS = 1024             # kCriticValueBlocks: workgroups of chub_critic_values_device at most
GRAD_R2 = 512 * 32 + 2 * 32 + 7      # 16455: 515 tiles, workgroups 0 .. 2 walk two and the rest one; tile 514 has 7 rows
GRAD_R3 = 2 * 512 * 32 + 3 * 32 + 7  # 32871: 1028 tiles, workgroups 0 .. 3 walk three and the rest two; tile 1027 has 7 rows


def grad_tiles(R):
    return -(-R // GRAD_TILE)


def grad_shape(sizes):
    """grad_plan for layer sizes [F, width 0, ..]: -> (lds_rows, n_pairs, part_floats) -- the feature image, every hidden image, two
    delta images of the widest layer and the scratch rows; one dW tile per (output tile, input tile); the dW tiles and the bias sums"""
    up = lambda n: -(-n // 32)
    ot, it = [up(o) for o in sizes[1:]], [up(i) for i in sizes[:-1]]
    rows = 32 * it[0] + 32 * sum(ot[:-1]) + 2 * 32 * max(ot) + GRAD_SCRATCH_ROWS
    pairs = sum(o * i for o, i in zip(ot, it))
    return rows, pairs, pairs * 1024 + 32 * sum(ot)


def grad_blocks(R, part_floats=1):
    """workgroups of a gradient call of R rows: the tiles rounded up to 8, at most 512, and no more than keep the f32 partials
    (part_floats a workgroup) within 256 MiB"""
    nb = min((grad_tiles(R) + 7) & ~7, GRAD_MAX_BLOCKS)
    return min(nb, max(8, (GRAD_PARTIAL_BYTES // (4 * part_floats)) & ~7))


def value_blocks(R):
    return min((grad_tiles(R) + 7) & ~7, VALUE_BLOCKS)


def grad_trips(R, blocks):
    """int [blocks]: the tiles workgroup b walks (b, b + blocks, ..)"""
    tiles = grad_tiles(R)
    return np.array([len(range(b, tiles, blocks)) for b in range(blocks)])


def grad_trip_of(R, blocks):
    """-> (trip [R], workgroup [R]) of every position of the call's row list"""
    tile = np.arange(R) // GRAD_TILE
    return tile // blocks, tile % blocks


def grad_last_trip(R, blocks):
    """bool [R]: the positions in the last tile their workgroup walks"""
    tile = np.arange(R) // GRAD_TILE
    return tile + blocks >= grad_tiles(R)


def grad_trip_positions(R, blocks, trip):
    """the positions 0 .. R - 1 that the workgroups meet in their trip `trip`, ascending"""
    return np.flatnonzero(grad_trip_of(R, blocks)[0] == trip).astype(np.int64)


def grad_by_workgroup(a, blocks):
    """a [R, n] over the call's positions -> [blocks, 32 trips, n]: the rows workgroup b meets in its walk, zeros where it walks no tile
    or the tile ends early"""
    a = np.asarray(a)
    trips = -(-grad_tiles(len(a)) // blocks)
    full = np.zeros((trips * blocks * GRAD_TILE, a.shape[1]), dtype=a.dtype)
    full[:len(a)] = a
    return full.reshape(trips, blocks, GRAD_TILE, a.shape[1]).transpose(1, 0, 2, 3).reshape(blocks, trips * GRAD_TILE, a.shape[1])
