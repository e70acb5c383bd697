"""Point clouds for the distCUDA2 tests (tests/test_knn_cpu.py pins the oracle's brute force on them, tests/test_gpu_knn.py
the HIP search against that brute force): the degenerate inputs the header of g4splat_amd/csrc/knn.hip claims to handle
exactly, and a float32 numpy restatement of the definition."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)

DEGENERATE = ["coincident", "duplicates200", "line", "lattice", "offset1e4", "thin", "nonfinite"]


def degenerate_cloud(name, P, seed=0):
    """float32 [P', 3]; P' = P except for the lattice, whose side is the largest with side^3 <= P."""
    rng = np.random.default_rng(seed)
    if name == "coincident":  # every distance is zero
        return np.tile(np.array([[0.3, -1.2, 2.5]], np.float32), (P, 1))
    if name == "duplicates200":  # 200 coincident points inside a normal cloud
        pts = rng.normal(size=(P, 3)).astype(np.float32)
        rows = rng.choice(P, 200, replace=False)
        pts[rows] = pts[rows[0]]
        return pts
    if name == "line":  # equally spaced on a line that is parallel to no axis
        t = np.arange(P, dtype=np.float32)[:, None]
        return (np.array([[1.0, -2.0, 0.5]], np.float32) + t * np.array([[0.015625, 0.03125, -0.0078125]], np.float32)).astype(np.float32)
    if name == "lattice":  # integer lattice: every distance is tied many times over
        side = int(round(P ** (1.0 / 3.0)))
        while side ** 3 > P:
            side -= 1
        g = np.arange(side, dtype=np.float32)
        pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
        return np.ascontiguousarray(pts[rng.permutation(pts.shape[0])])
    if name == "offset1e4":  # far from the origin: the coordinates keep few fraction bits
        return (np.float32(1e4) + np.float32(1e-2) * rng.normal(size=(P, 3)).astype(np.float32)).astype(np.float32)
    if name == "thin":  # the cubic lattice of the curve puts every point into one y / z cell
        pts = rng.normal(size=(P, 3)).astype(np.float32) * np.float32(1e-3)
        pts[:, 0] = (rng.random(P) * 1e6).astype(np.float32)
        return pts
    if name == "nonfinite":  # rows with NaN / +inf / -inf coordinates: they find nothing and nobody finds them
        pts = rng.normal(size=(P, 3)).astype(np.float32)
        rows = nonfinite_rows(P)
        bad = [(np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf), (np.nan, np.nan, np.nan), (np.inf, np.inf, np.inf),
               (-np.inf, 1.0, np.inf), (np.nan, -np.inf, 2.0), (np.inf, 0.5, 0.5)]
        for i, r in enumerate(rows):
            for a in range(3):
                if bad[i % len(bad)][a] != 0.0:
                    pts[r, a] = bad[i % len(bad)][a]
        return pts
    raise ValueError(name)


def nonfinite_rows(P):
    """Rows of the "nonfinite" cloud that hold a non-finite coordinate: the first, the last, leaf ends, and a few more."""
    return sorted({r for r in (0, 1, 63, 64, P // 3, P // 2, P // 2 + 1, P - 2, P - 1) if 0 <= r < P})


def knn_mean3_numpy(pts):
    """The definition, in float32 numpy (O(P^2) memory: small P only): differences candidate - query, three squares,
    (dx^2 + dy^2) + dz^2; the own index excluded; a distance is taken only where `best > dist` holds, so NaN, inf and
    FLT_MAX never are; the three smallest summed smallest first and divided by 3."""
    p = np.ascontiguousarray(pts, np.float32)
    P = p.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        d = p[None, :, :] - p[:, None, :]  # [query, candidate, axis]
        sq = d * d
        dist = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
        assert dist.dtype == np.float32
        dist = np.where(dist < FLT_MAX, dist, FLT_MAX)  # (NaN compares false)
        dist[np.arange(P), np.arange(P)] = FLT_MAX
        dist = np.concatenate([dist, np.full((P, 3), FLT_MAX, np.float32)], axis=1)  # fewer than three others
        best = np.sort(dist, axis=1)[:, :3]
        out = ((best[:, 0] + best[:, 1]) + best[:, 2]) / np.float32(3.0)
    assert out.dtype == np.float32
    return out
