"""The numpy restatement of the mesh rasteriser's contract (tests/mesh_render_ref.py) against independent truth: a float64
ray cast, the fill rule's watertightness on hand-made quads, and the dilated depth on maps whose answer is known.  No GPU."""
import numpy as np
import pytest

import mesh_render_ref as mr

f32, f64 = np.float32, np.float64
W, H, FOCAL = 67, 45, 60.0


# ---- float64 ray cast ----------------------------------------------------------------------------------------------------
def ray_cast(vertices, faces, Pm, off):
    """Möller-Trumbore per sample in float64: (nearest face or -1, its depth, the second nearest depth) as [H,W]."""
    v = np.asarray(vertices, f64)[np.asarray(faces)]
    jj, ii = np.meshgrid(np.arange(W, dtype=f64), np.arange(H, dtype=f64))
    d = np.stack([(2 * (jj + off) / W - 1) / f64(Pm[0, 0]), (2 * (ii + off) / H - 1) / f64(Pm[1, 1]), np.ones_like(jj)], -1)
    best, second, face = np.full((H, W), np.inf), np.full((H, W), np.inf), np.full((H, W), -1)
    for f, (a, b, c) in enumerate(v):
        e1, e2 = b - a, c - a
        p = np.cross(d, e2)
        det = p @ e1
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            u = (p @ (-a)) * inv
            q = np.cross(-a, e1)
            w = (d @ q) * inv
            t = (e2 @ q) * inv
        hit = (det != 0) & (u > 0) & (w > 0) & (u + w < 1) & (t > 0)
        t = np.where(hit, t, np.inf)
        nearer = t < best
        second = np.where(nearer, best, np.minimum(second, t))
        face = np.where(nearer, f, face)
        best = np.where(nearer, t, best)
    return face, best, second


def near_an_edge(fc, distance):
    """[H,W]: the samples within `distance` pixels of a projected edge of any face, in float64 from the float32 coordinates."""
    jj, ii = np.meshgrid(np.arange(W, dtype=f64), np.arange(H, dtype=f64))
    near = np.zeros((H, W), bool)
    sx, sy = fc.sx.astype(f64), fc.sy.astype(f64)
    for f in range(len(sx)):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            ex, ey = sx[f, b] - sx[f, a], sy[f, b] - sy[f, a]
            t = np.clip(((jj - sx[f, a]) * ex + (ii - sy[f, a]) * ey) / max(ex * ex + ey * ey, 1e-30), 0, 1)
            near |= np.hypot(jj - (sx[f, a] + t * ex), ii - (sy[f, a] + t * ey)) < distance
    return near


# The relative error of zbuf against the float64 depth that the restatement itself reaches on the agreed samples of these
# six inputs is at most 9.8e-7 (measured once, off 0.5 / 0.0: 40 faces 3.4e-7 / 2.2e-7, 300 faces seed 1 5.7e-7 / 9.8e-7, seed 2 4.4e-7 / 2.6e-7; the
# float32 roundings of the projection and of a quotient chain).  Four times that for headroom across seeds.
ZBUF_BOUND = 4 * 9.8e-7


@pytest.mark.parametrize("off", [0.5, 0.0])
@pytest.mark.parametrize("seed,n_faces,spread", [(0, 40, 0.5), (1, 300, 0.25), (2, 300, 0.25)])
def test_the_restatement_agrees_with_a_float64_ray_cast(seed, n_faces, spread, off):
    vertices, faces = mr.soup(seed, n_faces, spread, W, H, FOCAL)
    Wv, Pm = mr.pinhole(W, H, FOCAL, FOCAL)
    got = mr.render(vertices, faces, Wv, Pm, W, H, off=off)
    assert (got.fc.status == mr.OK).all() and (got.stats == 0).all()
    face, depth, second = ray_cast(vertices, faces, Pm, off)
    with np.errstate(invalid="ignore"):
        tie = np.isfinite(second) & ((second - depth) < 1e-5 * depth)
    excluded = near_an_edge(got.fc, 1 / 128) | tie
    share = excluded.mean()
    agreed = ~excluded
    hit = agreed & (face >= 0)
    err = np.abs(got.zbuf[hit].astype(f64) - depth[hit]) / depth[hit]
    print(f"seed {seed} faces {n_faces} off {off}: covered {(face >= 0).mean():.3f}, excluded {share:.4f}, "
          f"disagree outside the band {(got.pix_to_face != face)[agreed].sum()}, zbuf relative error {err.max():.3e}")
    assert share <= 0.03
    assert hit.sum() > 200
    assert (got.pix_to_face[agreed] == face[agreed]).all()
    assert err.max() <= ZBUF_BOUND
    # the weights are a partition of one, and reproduce the depth: 1 / zpix = sum of w_k-free terms, so sum w_k = 1 up to rounding
    assert np.abs(got.bary[hit].sum(-1) - 1).max() < 1e-6 and (got.bary >= 0).all()


# ---- watertightness ------------------------------------------------------------------------------------------------------
def _quad(diagonal, winding, x0=3, y0=2, x1=11, y1=9, z=2.0):
    """A quad with its corners on the samples (x0, y0) .. (x1, y1) at depth z, in front of pinhole(16, 12, 8, 8) with off = 0,
    split along either diagonal, every face in either winding."""
    Wq, Hq, fq = 16, 12, 8.0
    corners = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]  # clockwise on the screen, from the top left
    vertices = np.array([[((2 * x / Wq - 1) / (2 * fq / Wq)) * z, ((2 * y / Hq - 1) / (2 * fq / Hq)) * z, z] for x, y in corners], f32)
    faces = [[0, 1, 2], [0, 2, 3]] if diagonal == 0 else [[0, 1, 3], [1, 2, 3]]
    if winding:
        faces = [f[::-1] for f in faces]
    return vertices, np.array(faces, np.int32), Wq, Hq, fq


@pytest.mark.parametrize("diagonal", [0, 1])
@pytest.mark.parametrize("winding", [0, 1])
def test_a_split_quad_is_watertight(diagonal, winding):
    vertices, faces, Wq, Hq, fq = _quad(diagonal, winding)
    Wv, Pm = mr.pinhole(Wq, Hq, fq, fq)
    fc = mr.setup(*mr.face_positions(vertices, faces), Wv, Pm, Wq, Hq, 0.0, 1e-6)
    assert (fc.status == mr.OK).all()
    assert sorted(set(fc.X.reshape(-1)) | set(fc.Y.reshape(-1))) == [256 * c for c in (2, 3, 9, 11)]  # corners on samples
    ii, jj = np.meshgrid(np.arange(Hq), np.arange(Wq), indexing="ij")
    owners = sum(mr.sample(fc, f, ii, jj)[0].astype(int) for f in range(2))
    want = np.zeros((Hq, Wq), int)
    want[2:9, 3:11] = 1  # rows 2..8, columns 3..10: the top and left borders are owned, the bottom and right are not
    assert np.array_equal(owners, want)  # (the diagonal of an 8 x 7 quad meets no interior sample: the square below does)


def test_the_shared_diagonal_of_a_square_is_owned_once():
    """A 6 x 6 square, so that the diagonal passes through five interior samples, with both diagonals and windings."""
    for diagonal in (0, 1):
        for winding in (0, 1):
            vertices, faces, Wq, Hq, fq = _quad(diagonal, winding, 3, 2, 9, 8)
            Wv, Pm = mr.pinhole(Wq, Hq, fq, fq)
            fc = mr.setup(*mr.face_positions(vertices, faces), Wv, Pm, Wq, Hq, 0.0, 1e-6)
            ii, jj = np.meshgrid(np.arange(Hq), np.arange(Wq), indexing="ij")
            cover = [mr.sample(fc, f, ii, jj)[0] for f in range(2)]
            owners = cover[0].astype(int) + cover[1]
            want = np.zeros((Hq, Wq), int)
            want[2:8, 3:9] = 1
            assert np.array_equal(owners, want), (diagonal, winding)
            line = [(2 + k, 3 + k) for k in range(1, 6)] if diagonal == 0 else [(2 + k, 9 - k) for k in range(1, 6)]
            assert all(owners[i, j] == 1 for i, j in line)
            assert cover[0].sum() > 10 and cover[1].sum() > 10  # both faces own part of the square


def test_of_two_coincident_faces_the_smaller_index_wins():
    vertices, faces, Wq, Hq, fq = _quad(0, 0)
    Wv, Pm = mr.pinhole(Wq, Hq, fq, fq)
    doubled = np.concatenate([faces[:1], faces[:1], faces[1:], faces[1:]])
    got = mr.render(vertices, doubled, Wv, Pm, Wq, Hq, off=0.0)
    assert set(np.unique(got.pix_to_face)) == {-1, 0, 2}
    swapped = mr.render(vertices, doubled[[2, 3, 0, 1]], Wv, Pm, Wq, Hq, off=0.0)
    assert set(np.unique(swapped.pix_to_face)) == {-1, 0, 2}
    assert np.array_equal(swapped.pix_to_face >= 0, got.pix_to_face >= 0)


# ---- dilated depth -------------------------------------------------------------------------------------------------------
DW, DH, DF = 33, 29, 40.0


def _dilate_pm():
    return mr.pinhole(DW, DH, DF, DF)[1]


# |out - expected| on the interior of the constant map is at most 3.1e-7 (measured once: 2.9e-7 without a limit, 3.1e-7 with
# max_dilation = 0.05; one float32 ulp of 2 is 2.4e-7, and the chain back-project, move, project, interpolate ends near one);
# four times that.
CONSTANT_BOUND = 4 * 3.1e-7


@pytest.mark.parametrize("max_dilation", [1e8, 0.05])
def test_a_constant_map_moves_by_the_dilation(max_dilation):
    depth = np.full((DH, DW), 2.0, f32)
    out, _c, pix = mr.dilate(depth, _dilate_pm(), 1.5, max_dilation)
    expected = 2.0 - min(1.5 / DF * 2.0, max_dilation)
    inner = out[2:-2, 2:-2]
    print("constant map, max_dilation", max_dilation, "largest error", np.abs(inner.astype(f64) - expected).max())
    assert (pix[2:-2, 2:-2] >= 0).all()
    assert np.abs(inner.astype(f64) - expected).max() <= CONSTANT_BOUND


def _smooth_map():
    ii, jj = np.meshgrid(np.arange(DH), np.arange(DW), indexing="ij")
    return (2.5 + 0.4 * np.sin(jj / 7.0) + 0.3 * np.cos(ii / 5.0)).astype(f32)


# |out - in| with dilation_pixels = 0 on the smooth map is at most 2.4e-7 (measured once; one float32 ulp of the map's values:
# the map goes through a back-projection, a projection, a snap to 1/256 pixel that lands on the vertex, and one
# interpolation); four times that.
IDENTITY_BOUND = 4 * 2.4e-7


def test_no_dilation_returns_the_map():
    depth = _smooth_map()
    rgb = np.random.default_rng(3).uniform(-0.2, 1.2, (3, DH, DW)).astype(f32)
    out, col, pix = mr.dilate(depth, _dilate_pm(), 0.0, 1e8, rgb=rgb)
    err = np.abs(out.astype(f64) - depth).max()
    print("dilation 0: largest |out - in|", err, "drawn", (pix >= 0).mean())
    assert err <= IDENTITY_BOUND
    assert (pix[:-1, :-1] >= 0).all()
    # the last row and column lie on edges the fill rule leaves out: the fallback serves them, bit for bit
    assert (pix[-1] == -1).all() and (pix[:, -1] == -1).all()
    assert np.array_equal(out[-1], depth[-1]) and np.array_equal(out[:, -1], depth[:, -1])
    assert np.array_equal(col[:, -1], rgb[:, -1])  # rgb restored, unclamped
    drawn = pix >= 0
    assert np.abs(col[:, drawn] - np.clip(rgb, 0, 1)[:, drawn]).max() < 1e-5


def test_a_depth_step_grows_the_near_surface():
    depth = np.full((DH, DW), 3.0, f32)
    depth[:, :16] = 1.0
    out, _c, _pix = mr.dilate(depth, _dilate_pm(), 1.5, 1e8)
    assert (out.astype(f64) <= depth.astype(f64) + IDENTITY_BOUND).all()
    # far-side pixels next to the step take a near-surface depth
    assert (out[2:-2, 16] < 1.5).all()
    assert (out[2:-2, 20:-2] > 2.5).all() and (out[2:-2, 2:14] < 1.0).all()


def test_holes_stay_holes_and_rgb_is_restored():
    depth = _smooth_map()
    depth[10:14, 12:17] = 0.0
    depth[20, 5] = np.inf
    rgb = np.random.default_rng(4).uniform(0, 1, (3, DH, DW)).astype(f32)
    out, col, pix = mr.dilate(depth, _dilate_pm(), 0.0, 1e8, rgb=rgb)
    hole = np.zeros((DH, DW), bool)
    hole[10:14, 12:17] = True
    assert (out[hole] == 0).all() and (pix[hole] == -1).all()
    assert out[20, 5] == np.inf and pix[20, 5] == -1
    undrawn = pix < 0
    assert undrawn.sum() > hole.sum() and np.array_equal(col[:, undrawn], rgb[:, undrawn])
    assert np.isfinite(out[~hole & (depth < np.inf)]).all()
    # with a dilation the hole's inner pixels still see nothing: no face exists over an invalid vertex
    out2, _c, pix2 = mr.dilate(depth, _dilate_pm(), 0.5, 1e8)
    assert (out2[11:13, 14:15] == 0).all() and (pix2[11:13, 14:15] == -1).all()


def test_a_large_dilation_across_a_step_draws_large_faces():
    """Ten pixels of dilation across a step from 1 to 3: the faces over the step cover boxes of more than 64 samples (the
    device's list path), the near surface grows over the far side, and nothing moves away from the camera."""
    depth = mr.step_map(DW, DH, 16, True)
    fc = mr.dilated_faces(depth, _dilate_pm(), 10.0, 1e8)
    samples = mr.box_samples(fc)
    assert (samples > 64).sum() >= 5 and samples.max() < DW * DH
    out, _c, pix = mr.dilate(depth, _dilate_pm(), 10.0, 1e8)
    assert (out.astype(f64) <= depth.astype(f64) + IDENTITY_BOUND).all()
    assert (out[4:-4, 16:20] < 1.5).all()  # the four columns behind the step take a near-surface depth
    assert (pix[4:-4, 4:-4] >= 0).all()
