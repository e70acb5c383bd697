"""TSDF fusion without a GPU: the numpy restatement (tests/tsdf_ref.py) against float64 statements of what fusion means --
(a) the fused values against an analytic field, (b) the block walk against a slab test of the exact segment -- and (c) the
conditions under which each case of tests/tsdf_cases.py reaches the code it is named for.  tests/test_gpu_tsdf_fusion.py
then holds the kernels to the restatement bit for bit on the same cases."""
import itertools

import numpy as np
import pytest

import tsdf_cases as tc
import tsdf_ref
from tsdf_ref import BEHIND, INTEGRATED, INVALID, OUTSIDE, TRUNCATED

f32 = np.float32


def _fates(c, v, touched):
    return tsdf_ref.voxel_fates(touched, v.depth, v.mask, v.intr, v.E, c.voxel, c.T, c.depth_trunc)


def _walks(c, v):
    return tsdf_ref.pixel_walks(v.depth, v.mask, v.intr, v.E, c.voxel, c.T, c.depth_trunc)


def _first_view(name):
    c = tc.case(name)
    steps, _ref = tc.reference(name)
    touched = steps[0].keys  # a fresh volume: the table after the first view is what it touched
    return c, c.views[0], _walks(c, c.views[0]), _fates(c, c.views[0], touched)


# ---- (a) values against an analytic field -------------------------------------------------------------------------------
RADIUS = 1.5
_A = {}


def _eye_sphere(voxel, T):
    """A sphere of RADIUS centred on the eye: depth = R / sqrt(1 + a^2 + b^2) at every pixel.  Returns the view, the
    volume after one integration and after three, and per voxel of the table q (float64 camera-space centre)."""
    if (voxel, T) not in _A:
        rng = np.random.default_rng(7)
        cam, intr, E = tc.camera(64, 48, *tc.OFF_CENTRE, tc.rotation((0.7, -0.4, 0.6), 0.9), (0.137, -0.219, 0.083))
        a, b = tc.rays(64, 48, intr)
        depth = (RADIUS / np.sqrt(1 + a * a + b * b)).astype(f32)
        rgb = rng.uniform(-0.1, 1.1, (3, 48, 64)).astype(f32)
        vols = []
        for k in (1, 3):
            ref = tsdf_ref.RefVolume(voxel, T, 10.0)
            counts = [ref.integrate(depth, rgb, intr, E) for _ in range(k)]
            assert counts[0][0] == counts[0][1] > 50 and all(c == (counts[0][0], 0) for c in counts[1:])
            vols.append(ref)
        lane = np.arange(512)
        loc = np.stack([lane & 7, (lane >> 3) & 7, lane >> 6], 1)
        g = tsdf_ref.unpack_keys(vols[0].keys)[:, None, :] * 8 + loc[None]
        p = (g + 0.5) * float(f32(voxel))
        E64 = np.asarray(E, np.float64).reshape(4, 4)
        q = p @ E64[:3, :3].T + E64[:3, 3]
        _A[(voxel, T)] = (intr, depth, rgb, vols, q)
    return _A[(voxel, T)]


@pytest.mark.parametrize("voxel,T", [(0.04, 0.16), (0.02, 0.24)])
def test_fused_values_are_the_analytic_distance(voxel, T):
    """Every voxel with weight > 0 and |tsdf| < 1 holds tsdf * T = R - |q| up to z * (0.5/fx + 0.5/fy) + 16 ulp(R).

    Derivation.  The contract measures along the ray through the centre of the pixel the voxel projects to: with
    s(a, b) = sqrt(1 + a^2 + b^2) it stores (d - z) * s(a_p, b_p), and here d * s(a_p, b_p) = R exactly, so the value is
    R - z * s(a_p, b_p).  The truth is R - |q| = R - z * s(a_q, b_q) with the voxel's own ray (a_q, b_q) = (x/z, y/z).
    The voxel projects into the pixel, so |a_q - a_p| <= 0.5/fx and |b_q - b_p| <= 0.5/fy, and s is 1-Lipschitz in each
    argument (|ds/da| = |a|/s < 1): the two differ by at most z * (0.5/fx + 0.5/fy).  The float32 evaluation -- the
    depth map's rounding, E p, the square root, the product, the division by T and the multiplication back -- stays
    within a few ulps of its largest intermediate, which R bounds: 16 ulp(R)."""
    intr, _depth, _rgb, (one, _three), q = _eye_sphere(voxel, T)
    fx, fy = float(intr[0]), float(intr[1])
    tsdf, weight, _ = one.voxels()
    sel = (weight > 0) & (np.abs(tsdf) < 1)
    assert sel.sum() > 5000 and (tsdf[sel] < 0).sum() > 1000 and (tsdf[sel] > 0).sum() > 1000
    z = q[..., 2][sel]
    err = np.abs(tsdf[sel].astype(np.float64) * float(f32(T)) - (RADIUS - np.linalg.norm(q[sel], axis=1)))
    first = z * (0.5 / fx + 0.5 / fy)
    print(f"\nvoxel {voxel} T {T}: {sel.sum()} voxels, largest error / first term = {(err / first).max():.3f}")
    assert (err <= first + 16 * np.spacing(f32(RADIUS))).all(), (err / first).max()


@pytest.mark.parametrize("voxel,T", [(0.04, 0.16), (0.02, 0.24)])
def test_a_repeated_view_counts_three_times_and_changes_nothing_else(voxel, T):
    """The same view three times: weight exactly 3 where it was 1, tsdf within 3 ulps of the single view's (each
    running mean (t*w + t)/(w + 1) rounds twice, the first one, (0 + t)/1, is exact), colour exactly
    floor(255 * clamp(rgb)) of the pixel the voxel projects to (q, 2q and 3q are integers below 2^24 and divide exactly).
    The pixel comes from the float64 projection; voxels within 1e-4 pixels of a pixel's edge are left out."""
    intr, _depth, rgb, (one, three), q = _eye_sphere(voxel, T)
    fx, fy, cx, cy = (float(x) for x in intr)
    t1, w1, _ = one.voxels()
    t3, w3, c3 = three.voxels()
    assert np.array_equal(one.keys, three.keys) and set(np.unique(w1)) == {0.0, 1.0}
    assert np.array_equal(w3, 3 * w1)
    on = w1 > 0
    assert (np.abs(t3[on] - t1[on]) <= 3 * np.spacing(np.abs(t1[on]))).all()
    assert (t3[~on] == 0).all() and (c3[~on] == 0).all()
    pu, pv = fx * q[..., 0] / q[..., 2] + cx + 0.5, fy * q[..., 1] / q[..., 2] + cy + 0.5
    clear = on & (np.abs(pu - np.round(pu)) > 1e-4) & (np.abs(pv - np.round(pv)) > 1e-4)
    assert clear.sum() > 0.999 * on.sum()
    u, v = np.floor(pu[clear]).astype(int), np.floor(pv[clear]).astype(int)
    want = np.floor(255.0 * np.clip(rgb[:, v, u].astype(np.float64), 0.0, 1.0)).T
    assert np.array_equal(c3[clear].astype(np.float64), want)
    assert len(np.unique(want)) == 256


# ---- (b) the block walk against a float64 slab test -------------------------------------------------------------------
def _segment64(v, pixel, T, voxel):
    """The segment ends of pixels [n,2] in block units: the header's expressions on the float32 camera, in float64."""
    fx, fy, cx, cy = (float(x) for x in v.intr)
    C = tsdf_ref.camera_to_world(v.E).astype(np.float64)
    d = v.depth[pixel[:, 1], pixel[:, 0]].astype(np.float64)
    rx, ry = (pixel[:, 0] - cx) / fx, (pixel[:, 1] - cy) / fy
    bs = 8.0 * float(f32(voxel))
    ends = []
    for z in (d - float(f32(T)), d + float(f32(T))):
        cam = np.stack([rx * z, ry * z, z, np.ones_like(z)], 1)
        ends.append(cam @ C.T / bs)
    return ends


def _chord(a, b, lo, hi):
    """Length of the part of segment a -> b inside the boxes [lo, hi] ([k,3] each; negative: no common point)."""
    d = b - a
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - a) / d, (hi - a) / d
    flat = d == 0
    inside = (lo <= a) & (a <= hi)
    tmin = np.where(flat, np.where(inside, -np.inf, np.inf), np.minimum(t1, t2)).max(1)
    tmax = np.where(flat, np.where(inside, np.inf, -np.inf), np.maximum(t1, t2)).min(1)
    return (np.minimum(tmax, 1.0) - np.maximum(tmin, 0.0)) * np.linalg.norm(d)


@pytest.mark.parametrize("name", ["oblique_long", "near_camera", "far_patches"])
def test_block_walk_covers_the_exact_segment(name):
    """For every valid pixel: the list runs from floor(a) to floor(b) in unit steps of one axis, is as long as
    1 + the Manhattan distance and shorter than the cap; every listed block lies within eps of the float64 segment; every
    block whose interior the float64 segment crosses over a length above eps is listed.

    eps = 8 float32 ulps of the largest block-unit coordinate of the segment.  a and b each come from eleven float32
    roundings ((u - cx)/fx: two, d -+ T: one, the products with z: one each, C's row: three products and three sums, the
    division by B: one) of at most half an ulp of an intermediate no larger than that coordinate's scale, under 6 ulps
    together; the walk's own t = (boundary - a_i)/dir_i adds a rounding of a difference of such numbers, which can swap
    two steps only where the segment passes within an ulp of a block edge.  So the float32 walk is an exact walk of a
    segment displaced by less than eps: it cannot list a block farther than eps from the true segment.  It can miss a
    block the true segment crosses only if the displaced segment avoids its interior.  Over a chord longer than eps whose
    direction has every component at least a quarter of its length, the chord's midpoint is eps/8 or more inside the
    block along every axis, beyond the displacement; far_patches, the one case whose ulp is not negligible against a
    block (1/32 of one), keeps its rays that oblique, which is asserted here.  At the other cases' ulp of 1e-6 blocks a
    chord that long through a block's outermost 1e-6 does not occur in these seeded inputs."""
    c = tc.case(name)
    checked = 0
    for v in c.views:
        w = _walks(c, v)
        sel = np.nonzero(w["inside"])[0]
        if len(sel) == 0:
            continue
        a32, b32 = w["a"][sel], w["b"][sel]
        a64, b64 = (e[sel] for e in _segment64(v, w["pixel"], c.T, c.voxel))
        assert not w["cut"].any()
        for i, s in enumerate(sel):
            n = w["length"][s]
            path = w["path"][s, :n]
            first, last = np.floor(a32[i]).astype(np.int64), np.floor(b32[i]).astype(np.int64)
            assert np.array_equal(path[0], first) and np.array_equal(path[-1], last)
            assert (np.abs(np.diff(path, axis=0)).sum(1) == 1).all()
            assert n == 1 + np.abs(last - first).sum() and n < w["cap"]
            a, b = a64[i], b64[i]
            eps = 8.0 * float(np.spacing(f32(max(np.abs(a).max(), np.abs(b).max()))))
            assert np.abs(a32[i] - a).max() < eps and np.abs(b32[i] - b).max() < eps
            assert (_chord(a, b, path - eps, path + 1.0 + eps) >= 0).all(), (name, w["pixel"][s])
            lo, hi = np.floor(np.minimum(a, b)).astype(np.int64), np.floor(np.maximum(a, b)).astype(np.int64)
            box = np.array(list(itertools.product(*[range(l, h + 1) for l, h in zip(lo, hi)])), np.int64)
            crossed = box[_chord(a, b, box.astype(np.float64), box + 1.0) > eps]
            listed = {tuple(p) for p in path}
            assert all(tuple(p) in listed for p in crossed), (name, w["pixel"][s])
            if name == "far_patches":
                assert (np.abs(b - a) >= 0.25 * np.linalg.norm(b - a)).all()
            checked += 1
    assert checked >= 1000


# ---- (c) the conditions of the cases ----------------------------------------------------------------------------------
def test_oblique_long_conditions():
    c, v, w, f = _first_view("oblique_long")
    H, W = v.depth.shape
    assert w["cap"] == 16 and tsdf_ref.valid_pixels(v.depth, v.mask, c.depth_trunc).all() and w["inside"].all()
    assert w["length"].max() >= 6 and not w["cut"].any()
    assert tuple(np.round(v.intr, 1)) == (70.0, 65.0, 20.3, 30.7)
    done = f["fate"] == INTEGRATED
    borders = [(f["u"][done] == 0).sum(), (f["u"][done] == W - 1).sum(), (f["v"][done] == 0).sum(), (f["v"][done] == H - 1).sum()]
    outside = (f["fate"] == OUTSIDE).sum()
    print(f"\noblique_long: longest walk {w['length'].max()} cells, voxels integrated at u=0, u=W-1, v=0, v=H-1: {borders}, "
          f"outside the frame {outside}, truncated {(f['fate'] == TRUNCATED).sum()}, blocks {len(f['fate'])}")
    assert min(borders) > 0 and outside > 0 and (f["fate"] == TRUNCATED).sum() > 0


def test_near_camera_conditions():
    c, v, w, f = _first_view("near_camera")
    z0 = v.depth[w["pixel"][:, 1], w["pixel"][:, 0]] - f32(c.T)
    behind = (f["fate"] == BEHIND).sum()
    print(f"\nnear_camera: {(z0 < 0).sum()} of {len(z0)} segments start behind the camera, {behind} voxels with z <= 0, "
          f"{(f['fate'] == INTEGRATED).sum()} integrated")
    assert (z0 < 0).sum() > 100 and (z0 > 0).sum() > 100 and behind > 0 and (f["z"] == 0).sum() == 0
    assert (f["fate"] == INTEGRATED).sum() > 100


def test_ties_conditions():
    c, v, w, f = _first_view("ties")
    assert tuple(v.intr) == (16.0, 16.0, 16.0, 16.0)
    assert np.array_equal(tsdf_ref.camera_to_world(v.E)[:, 3] / f32(0.5), [3.0, -2.0, 1.0])  # the eye, in blocks
    zero_dir = ((w["b"] - w["a"]) == 0).any(1).sum()
    u, vv = w["pixel"][:, 0], w["pixel"][:, 1]
    diag = (np.abs(u - 16) == np.abs(vv - 16)) | (u == 16) | (vv == 16)
    on_bound = ((f["fate"] == TRUNCATED) & (f["sdf"] == -f32(c.T))).sum()
    print(f"\nties: {w['ties'].sum()} steps chose between equal t, on {(w['ties'] > 0).sum()} pixels "
          f"({(w['ties'][diag] > 0).sum()} of them on the diagonals and axes); {zero_dir} segments with a zero direction "
          f"component; {on_bound} voxels with sdf == -sdf_trunc")
    assert w["ties"].sum() >= 20 and zero_dir >= 33 and not w["cut"].any()
    assert (w["ties"][diag] > 0).sum() >= 20
    assert on_bound >= 1


def test_validity_conditions():
    c, v, w, f = _first_view("validity")
    seen = f["u"] >= 0  # voxels of touched blocks that project into the frame
    d, m = v.depth[f["v"][seen], f["u"][seen]], v.mask[f["v"][seen], f["u"][seen]]
    bits = lambda x: np.asarray(x, f32).view(np.uint32)
    for val in tc.VALIDITY_DEPTHS:
        assert (bits(d) == bits(val)).any(), val
    for val in tc.VALIDITY_MASKS:
        assert (bits(m) == bits(val)).any(), val
    done = f["fate"] == INTEGRATED
    dd, dm = v.depth[f["v"][done], f["u"][done]], v.mask[f["v"][done], f["u"][done]]
    assert (dd == tc.VALIDITY_TRUNC).any() and (dm == f32(0.5)).any()  # the two edge values that are valid
    assert not (dd > tc.VALIDITY_TRUNC).any() and not (dm < f32(0.5)).any()
    got = np.unique(bits(v.rgb[:, f["v"][done], f["u"][done]]))
    missing = np.setdiff1d(bits(tc.validity_colours()), got)
    print(f"\nvalidity: {done.sum()} voxels integrated, {(f['fate'] == INVALID).sum()} at invalid pixels, "
          f"{len(np.unique(bits(tc.validity_colours())))} colour values all seen by integrated voxels: {len(missing) == 0}")
    assert len(missing) == 0
    q = tsdf_ref.quantise(tc.validity_colours())
    assert q[0] == 0 and q[1] == 0 and q[2] == 255  # NaN, -0.1, 1.1
    # float32 k/255 * 255 lands on k or just below it; truncation and rounding to nearest then differ
    exact = (tc.validity_colours() * f32(255))[3:]
    assert (exact != np.rint(exact)).sum() >= 100 and (q[3:] != np.rint(exact)).sum() >= 100


def _key_bytes(keys):
    k = np.asarray(keys, np.int64)
    return [len(np.unique((k >> (8 * i)) & 0xFF)) for i in range(8)]


def test_far_patches_conditions():
    c = tc.case("far_patches")
    steps, ref = tc.reference("far_patches")
    assert len(c.views) == 8
    touched = np.concatenate([ref.keys[np.isin(ref.slots, s.touched_slots)] for s in steps[:6]])
    per_byte = _key_bytes(touched)
    coords = tsdf_ref.unpack_keys(ref.keys)
    print(f"\nfar_patches: distinct values per key byte (low to high) {per_byte}; block coordinates from {coords.min()} "
          f"to {coords.max()}; counts {[s.counts for s in steps]}")
    assert min(per_byte) >= 3
    assert (coords[:, :].min() < -100_000) and (coords.max() > 100_000)
    for s in steps[:6]:
        assert s.counts[0] == s.counts[1] > 0 and (s.weight > 0).sum() > 0
    w7, w8 = _walks(c, c.views[6]), _walks(c, c.views[7])
    assert len(w7["inside"]) == 192 and not w7["inside"].any() and steps[6].counts == (0, 0)
    assert (np.abs(w7["a"]) >= 1e6).any(1).all() and (np.abs(w7["b"]) >= 1e6).any(1).all()
    assert 20 < w8["inside"].sum() < 172 and steps[7].counts[0] > 0
    assert tsdf_ref.unpack_keys(steps[7].keys).max() == 999_999


def test_merge_sequence_conditions():
    c = tc.case("merge_sequence")
    steps, ref = tc.reference("merge_sequence")
    assert len(c.views) == 20
    n = [len(s.keys) for s in steps]
    cnt = [s.counts for s in steps]
    # 1, 2: a first view, and again
    assert cnt[0][0] == cnt[0][1] > 256 and cnt[1] == (cnt[0][0], 0)
    assert set(np.unique(steps[1].weight)) == {0.0, 2.0}
    # 3: no valid pixel
    assert cnt[2] == (0, 0) and np.array_equal(steps[2].keys, steps[1].keys) and len(steps[2].touched_slots) == 0
    # 4, 5: all new keys below / above the table
    for i, below in ((3, True), (4, False)):
        new = np.setdiff1d(steps[i].keys, steps[i - 1].keys)
        assert cnt[i][0] == cnt[i][1] == len(new) > 0
        assert new.max() < steps[i - 1].keys.min() if below else new.min() > steps[i - 1].keys.max()
    # 6: interleaved
    is_new = ~np.isin(steps[5].keys, steps[4].keys)
    runs = 1 + int((is_new[1:] != is_new[:-1]).sum())
    assert cnt[5][1] == is_new.sum() > 0 and runs >= 8
    # 7: old table and touched list above 256, some touched blocks old and some new
    assert n[5] > 256 and cnt[6][0] > 256 and 0 < cnt[6][1] < cnt[6][0]
    # 8: one pixel
    assert c.views[7].depth.shape == (1, 1) and cnt[7][0] >= 1
    # 9 .. 20: the ring
    assert all(cnt[i][0] > 0 for i in range(8, 20)) and cnt[8][1] > 0
    ring = np.unique(np.concatenate([s.touched_slots for s in steps[8:]]))
    assert ref.weight[ring].max() == 12 and ref.weight.max() == 12
    print(f"\nmerge_sequence: counts {cnt}; table sizes {n}; view 6 merges {runs} alternating runs; largest weight "
          f"{ref.weight.max():.0f}")


@pytest.mark.parametrize("shape", tc.SMALL_SHAPES)
def test_small_image_conditions(shape):
    W, H = shape
    name = f"small_{W}x{H}"
    c = tc.case(name)
    steps, ref = tc.reference(name)
    w = _walks(c, c.views[0])
    assert w["cap"] == tc.SMALL_CAP and not w["cut"].any()
    assert steps[0].counts[0] >= 1 and ref.weight.max() == 1


def test_small_images_sit_on_both_sides_of_a_scan_chunk_and_a_sort_tile():
    n = sorted(W * H * tc.SMALL_CAP for W, H in tc.SMALL_SHAPES)
    assert n == [7, 1022, 1029, 1792, 1799, 2100, 2100, 4095, 4102]


def test_reference_counts_are_the_table_growth():
    for name in tc.CASES:
        steps, _ref = tc.reference(name)
        size = 0
        for s in steps:
            assert len(s.keys) == size + s.counts[1] and len(s.touched_slots) == s.counts[0]
            assert (np.diff(s.keys) > 0).all() and sorted(s.slots) == list(range(len(s.keys)))
            size = len(s.keys)
