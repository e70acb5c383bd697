"""Adversarial inputs for the marching-cubes kernels (sparse blocks and dense lattices), importable without a GPU.

A sparse case is `(keys sorted, tsdf [n,512], weight [n,512], colour [n,512,3], voxel_size)`, the layout
tsdf_ref.extract_mesh takes.  All of them are seeded numpy; the voxel size is 0.1 unless stated, and apart from
far_keys every vertex coordinate stays below 4 in magnitude.  tests/test_mc_cases_cpu.py checks on the numpy
restatement alone that each case really contains what it is meant to contain.
"""
import itertools

import numpy as np

import tsdf_ref

f32 = np.float32
V = 0.1
LIM = 1 << 20          # block coordinates lie in -LIM .. LIM - 1 (21-bit key fields)
FAR = 999_999          # the farthest block integration can allocate (TSDF_COORD_LIMIT)
SUBNORMAL = 1e-40      # a float32 subnormal (the smallest normal is 1.18e-38)


def _sorted(coords):
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    keys = tsdf_ref.pack_keys(coords)
    assert len(np.unique(keys)) == len(keys)
    order = np.argsort(keys)
    return keys[order], coords[order]


def _noise_case(coords, seed, voxel_size=V):
    """i.i.d. uniform(-1, 1) tsdf, weight 1 and uniform(0, 255) colours on the blocks `coords`; also the sorted coords."""
    keys, coords = _sorted(coords)
    rng = np.random.default_rng(seed)
    n = len(keys)
    tsdf = rng.uniform(-1, 1, (n, 512)).astype(f32)
    color = rng.uniform(0, 255, (n, 512, 3)).astype(f32)
    return [keys, tsdf, np.ones((n, 512), f32), color, voxel_size], coords, rng


def _cube(lo, hi):
    return list(itertools.product(range(lo, hi + 1), repeat=3))


def noise(seed=11):
    """2x2x2 blocks at -1..0 on each axis: 15^3 cubes of i.i.d. noise, negative block coordinates in the keys."""
    case, _c, _r = _noise_case(_cube(-1, 0), seed)
    return tuple(case)


def noise_holes(seed=12, zero_block=None):
    """3x3x3 blocks at -1..1, about 10 % of the voxels with weight 0 and tsdf NaN.  zero_block = block coordinates:
    that block's weights are all 0 as well (its tsdf stays as it is: only the weight test keeps it out)."""
    case, coords, rng = _noise_case(_cube(-1, 1), seed)
    hole = rng.random((len(coords), 512)) < 0.10
    case[1][hole] = np.nan
    case[2][hole] = 0.0
    if zero_block is not None:
        (b,) = np.nonzero((coords == np.asarray(zero_block)).all(1))[0]
        case[2][b] = 0.0
    return tuple(case)


# the block set of gaps(), by group; groups lie at least two blocks apart, so they do not interact
GAP_GROUPS = {
    "face": [(-4, -4, -4), (-3, -4, -4)],
    "edge": [(-4, -1, -4), (-3, 0, -4)],
    "corner": [(-4, 2, -4), (-3, 3, -3)],
    "L": [(0, -4, -4), (1, -4, -4), (0, -3, -4)],
    "isolated": [(3, -4, -4)],
    "minus_star": [(2, 2, 2), (1, 2, 2), (2, 1, 2), (2, 2, 1)],       # the first block has only its -x/-y/-z neighbours
    "plus_star": [(-3, -3, 1), (-2, -3, 1), (-3, -2, 1), (-3, -3, 2)],  # the mirror: only +x/+y/+z
}


def gaps(seed=13):
    """Noise on a sparse block set with every adjacency class of the 27-neighbourhood (GAP_GROUPS)."""
    case, _c, _r = _noise_case([b for grp in GAP_GROUPS.values() for b in grp], seed)
    return tuple(case)


def exact_zeros(seed=14):
    """The noise blocks with about 5 % of the voxels 0.0 and about 5 % -0.0: neither is negative, e becomes 0 or -0."""
    case, _c, rng = _noise_case(_cube(-1, 0), seed)
    r = rng.random(case[1].shape)
    case[1][r < 0.05] = f32(0.0)
    case[1][(r >= 0.05) & (r < 0.10)] = f32(-0.0)
    return tuple(case)


def subnormals(seed=15):
    """The noise blocks with about 5 % float32 subnormals of both signs (+-1e-40): -1e-40 is negative, +1e-40 is not."""
    case, _c, rng = _noise_case(_cube(-1, 0), seed)
    r = rng.random(case[1].shape)
    case[1][r < 0.025] = f32(SUBNORMAL)
    case[1][(r >= 0.025) & (r < 0.05)] = f32(-SUBNORMAL)
    assert (np.abs(case[1][r < 0.05]) > 0).all() and (np.abs(case[1][r < 0.05]) < np.finfo(f32).tiny).all()
    return tuple(case)


def single(seed=16, holes=False):
    """One block: only its 7^3 interior cubes are valid, no edge across the block's faces carries a vertex.  With every
    weight positive each crossing inside it lies in a valid cube; holes = True gives about 10 % of the voxels weight 0
    (tsdf NaN), which leaves crossings that no valid cube uses."""
    case, _c, rng = _noise_case([(0, -1, 0)], seed)
    if holes:
        hole = rng.random((1, 512)) < 0.10
        case[1][hole] = np.nan
        case[2][hole] = 0.0
    return tuple(case)


# the clusters of far_keys(), each contiguous in key order and listed in key order
FAR_CLUSTERS = [
    [(-LIM, -LIM, -LIM)],                       # the lower end of every key field
    [(-FAR, 0, 0), (-FAR, 0, 1)],               # the farthest allocatable block, both signs
    [(0, 0, LIM - 1)],                          # its +z neighbour would alias (0, 1, -LIM) ...
    [(0, 1, -LIM)],                             # ... which exists
    [(0, LIM - 1, 0)],                          # its +y neighbour would alias (1, -LIM, 0) ...
    [(1, -LIM, 0)],                             # ... which exists
    [(FAR - 1, 0, 0), (FAR, 0, 0)],
    [(LIM - 1, LIM - 1, LIM - 1)],              # the upper end of every key field
]


def far_keys(seed=17):
    """Noise clusters of one or two blocks at the ends of the key fields (FAR_CLUSTERS).  Vertex coordinates reach
    2^20 * 8 * 0.1 = 8.4e5, where a float32 ulp is 1/16."""
    case, coords, _r = _noise_case([b for c in FAR_CLUSTERS for b in c], seed)
    assert [tuple(c) for c in coords] == [b for c in FAR_CLUSTERS for b in c]  # clusters contiguous, in key order
    return tuple(case)


MANY_SHAPE = (11, 11, 9)
MANY_NOISE = (0, 1022, 1023, 1024)  # table positions of the noise blocks: both sides of the scan's chunk of 1024
MANY_V = 0.05                       # 11 blocks of 8 voxels: a voxel of 0.05 keeps |vertex| < 4


def many_blocks(n_blocks=1025, seed=18):
    """The first n_blocks (<= 1025, in key order) of an 11x11x9 slab of blocks around the origin: tsdf +1 and weight 1
    everywhere except i.i.d. noise in the blocks at table positions MANY_NOISE.  Voxel size 0.05."""
    sx, sy, sz = MANY_SHAPE
    coords = [(x - sx // 2, y - sy // 2, z - sz // 2) for x in range(sx) for y in range(sy) for z in range(sz)]
    keys, coords = _sorted(coords)
    case, _c, _r = _noise_case(coords[:1025], seed, MANY_V)
    quiet = np.ones(1025, bool)
    quiet[list(MANY_NOISE)] = False
    case[1][quiet] = f32(1.0)
    assert 0 < n_blocks <= 1025
    return tuple(a[:n_blocks] if isinstance(a, np.ndarray) else a for a in case)


SPARSE = {
    "noise": noise,
    "noise_holes": noise_holes,
    "gaps": gaps,
    "exact_zeros": exact_zeros,
    "subnormals": subnormals,
    "single": single,
    "single_holes": lambda: single(holes=True),
    "far_keys": far_keys,
    "many_1023": lambda: many_blocks(1023),
    "many_1024": lambda: many_blocks(1024),
    "many_1025": lambda: many_blocks(1025),
    "holes_zero_block": lambda: noise_holes(zero_block=(0, 0, 0)),
}


# ---- dense lattices: tsdf [N^3], stored x fastest ---------------------------------------------------------------------
DENSE_R = 0.5           # with centre 0 and radius 1 every lattice point has norm < 1: the un-contraction is the identity
DENSE_SIZES = (2, 3, 5, 16, 17, 33)
DENSE_GROUP = 256       # lattice points per workgroup of the dense kernels
SCAN_CHUNK = 1024       # values per chunk of the scan over the per-workgroup counts


def dense_noise(N, seed=20):
    return np.random.default_rng(seed + N).uniform(-1, 1, N ** 3).astype(f32)


def dense_zeros(N=17, seed=21):
    """Noise with about 5 % 0.0, 5 % -0.0 and 5 % subnormals of both signs."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1, 1, N ** 3).astype(f32)
    r = rng.random(N ** 3)
    t[r < 0.05] = f32(0.0)
    t[(r >= 0.05) & (r < 0.10)] = f32(-0.0)
    t[(r >= 0.10) & (r < 0.125)] = f32(SUBNORMAL)
    t[(r >= 0.125) & (r < 0.15)] = f32(-SUBNORMAL)
    return t


def dense_scan_crossing(N=65, seed=22):
    """+1 everywhere except noise in the planes k = 0 and k = N - 2 and in the storage range of workgroups 1022..1025:
    65^3 points are 1073 workgroups, so the scan over their counts crosses its chunk of 1024 between non-zero counts."""
    assert (N ** 3 + DENSE_GROUP - 1) // DENSE_GROUP > SCAN_CHUNK + 1
    rng = np.random.default_rng(seed)
    t = np.ones((N, N, N), f32)  # [k, j, i]
    t[0] = rng.uniform(-1, 1, (N, N))
    t[N - 2] = rng.uniform(-1, 1, (N, N))
    t = t.reshape(-1)
    lo, hi = (SCAN_CHUNK - 2) * DENSE_GROUP, (SCAN_CHUNK + 2) * DENSE_GROUP
    t[lo:hi] = rng.uniform(-1, 1, hi - lo)
    return t


DENSE = {f"noise_{N}": (lambda N=N: (dense_noise(N), N)) for N in DENSE_SIZES}
DENSE["zeros_17"] = lambda: (dense_zeros(17), 17)
DENSE["scan_65"] = lambda: (dense_scan_crossing(65), 65)
