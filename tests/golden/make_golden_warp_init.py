"""Golden vectors of the warp initialiser, produced by RUNNING THE REFERENCE'S OWN CODE on the CPU of the build container:

    warp_init.npz   scene/gaussian_model.py `get_gaussian_parameters_by_warp_from_depths`, imported and called for real, in
                    float32 and in float64, twice: recording A (grid -1, min_scale 0.035, max_scale 0.05) and recording B
                    (grid 3, min_scale 0.035, max_scale 0.16).

Stand-ins, and what they mean for the golden.
  * `tqdm` is the identity on its iterable.
  * For the float64 run `Tensor.float` returns the double tensor and every torch factory maps an explicit
    dtype=torch.float32 to float64: the reference hard-codes both (utils/point_utils.py depths_to_points,
    _camera_intrinsics_from_view).  Everything else follows the dtype of the cameras, depths and images it is handed, which
    are the float32 inputs widened.
  * `_warp_coverage_mask`, `_project_world_points_to_view`, `_points_to_distance_map` and `depths_to_points` of the imported
    module are wrapped to RECORD what they return per (view, earlier view) or per view; they compute nothing themselves.
The reference returns rows, not masks.  Its per-pixel keep mask is rebuilt from the records exactly as its own lines
combine them -- not covered by any earlier view, on the lattice, depth > 0, and distance / 2 (times the grid) below
max_scale --, and main() asserts that this mask selects the rows the reference returned (same number, same means).

Scene (tests/warp_init_ref.py): four views of (W, H) = (24,18), (20,20), (24,18), (17,23), 60 degrees horizontal FoV, poses
(tx, ty, tz, yaw) = POSES, depths ray-cast in float64 from the height field z = 2.1 + 0.3 sin(2.6 x) cos(2.2 y) with a
nearer patch z = 1.3 over |x - 0.25| < 0.22, |y| < 0.25, +-1.2 % uniform relative depth noise and a zero-depth block
[:3, :4] in every view.

Yardstick, per recording.  Per continuous output the largest |float32 run - float64 run| of the reference over the rows both
runs keep (rotations as matrices rebuilt from the quaternions); for the projections the same over the recorded (u, v, z)
of the pixels both runs place in the image; for the relative depth error the same over the pixels that tap the same texel.
A pixel is NEAR a threshold when, for some earlier view, its float64 u or v lies within 4 x the projection yardstick of a
half-integer or of a closed border (0, W - 1 or H - 1), or its relative depth error lies within 4 x its yardstick of
depth_error_thresh.  main() asserts: near pixels are at most 1 % of each view's pixels; away from them the two runs' keep
masks are equal; every later view has at least 10 % covered and 10 % uncovered valid pixels (recording A).

Nothing of the reference is copied: the npz holds inputs and recorded results only.
Run in the build container only (needs the reference checkout):  python tests/golden/make_golden_warp_init.py"""
import contextlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # g4splat_amd.synthetic: the scene's cameras
from _ref_import import _FACTORIES, reference_modules  # noqa: E402
import warp_init_ref as wr  # noqa: E402


@contextlib.contextmanager
def float_is_double():
    saved_float, saved = torch.Tensor.float, {n: getattr(torch, n) for n in _FACTORIES}

    def widen(fn):
        def wrapped(*a, **k):
            if k.get("dtype") is torch.float32:
                k["dtype"] = torch.float64
            return fn(*a, **k)
        return wrapped

    try:
        torch.Tensor.float = lambda self, *a, **k: self.double()
        for n, f in saved.items():
            setattr(torch, n, widen(f))
        yield
    finally:
        torch.Tensor.float = saved_float
        for n, f in saved.items():
            setattr(torch, n, f)


def run_reference(cams, depths, images, dtype, g, min_scale, max_scale):
    """The reference's function on the CPU in `dtype`: its rows, and per view the rebuilt keep mask with what it was built of."""
    tqdm = types.ModuleType("tqdm")
    tqdm.tqdm = lambda it, **k: it
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    views = [types.SimpleNamespace(world_view_transform=t(c.world_view_transform), full_proj_transform=t(c.full_proj_transform),
                                   image_width=c.image_width, image_height=c.image_height, original_image=t(im))
             for c, im in zip(cams, images)]
    rec = {"cover": [], "proj": [], "dist": [], "points": []}
    with reference_modules({"tqdm": tqdm}), (float_is_double() if dtype == torch.float64 else contextlib.nullcontext()):
        import scene.gaussian_model as gm

        def recording(name, key):
            fn = getattr(gm, name)

            def wrapped(*a, **k):
                out = fn(*a, **k)
                rec[key].append(out)
                return out
            setattr(gm, name, wrapped)

        recording("_warp_coverage_mask", "cover")
        recording("_project_world_points_to_view", "proj")
        recording("_points_to_distance_map", "dist")
        recording("depths_to_points", "points")
        out = gm.get_gaussian_parameters_by_warp_from_depths([t(d)[None] for d in depths], views, depth_error_thresh=wr.DEPTH_ERROR_THRESH,
                                                             min_scale=min_scale, max_scale=max_scale, downsample_pixel_grid_size=g)
    means, scales, quats, colors = (o.numpy() for o in out)
    want = np.float32 if dtype == torch.float32 else np.float64
    assert all(o.dtype == want for o in (means, scales, quats, colors)), [o.dtype for o in (means, scales, quats, colors)]
    V = len(views)
    assert len(rec["cover"]) == len(rec["proj"]) == V * (V - 1) // 2 and len(rec["dist"]) == len(rec["points"]) == V
    res = types.SimpleNamespace(means=means, scales=scales, quaternions=quats, colors=colors, keep=[], covered=[], pairs={}, s=[])
    step, k, row = (g if g > 0 else 1), 0, 0
    for i, d in enumerate(depths):
        H, W = d.shape
        covered = np.zeros((H, W), bool)
        for j in range(i):
            covered |= rec["cover"][k].numpy()
            xy, z = rec["proj"][k]
            res.pairs[(i, j)] = (xy[..., 0].numpy().reshape(-1), xy[..., 1].numpy().reshape(-1), z.numpy().reshape(-1))
            k += 1
        lattice = np.zeros((H, W), bool)
        lattice[::step, ::step] = True
        s = rec["dist"][i].numpy() / 2.0
        if g > 0:
            s = s * g
        assert s.dtype == want
        keep = ~covered & lattice & (d > 0) & (s < max_scale)
        n = int(keep.sum())
        assert np.array_equal(means[row:row + n], rec["points"][i].numpy().reshape(H, W, 3)[keep]), i  # the reference's rows
        row += n
        res.keep.append(keep), res.covered.append(covered & (d > 0)), res.s.append(s)
    assert row == len(means), (row, len(means))
    return res


def relative_errors(pairs, depths, dtype):
    """Per (i, j): the tapped texel's flat index (-1 outside the image) and the relative depth error, in `dtype`."""
    out = {}
    for (i, j), (u, v, z) in pairs.items():
        d = depths[j].astype(dtype)
        H, W = d.shape
        with np.errstate(invalid="ignore"):
            inside = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1) & (z > 0)
        ui, vi = np.clip(np.rint(u), 0, W - 1).astype(np.int64), np.clip(np.rint(v), 0, H - 1).astype(np.int64)
        tap = np.where(inside, vi * W + ui, -1)
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.abs(z - d[vi, ui]) / (np.abs(z) + dtype(1e-6))
        out[(i, j)] = (tap, rel)
    return out


def record(cams, depths, images, g, min_scale, max_scale, coverage_shares):
    r32 = run_reference(cams, depths, images, torch.float32, g, min_scale, max_scale)
    r64 = run_reference(cams, depths, images, torch.float64, g, min_scale, max_scale)
    # yardsticks of the rows
    i32, i64 = [], []
    o32 = o64 = 0
    for k32, k64 in zip(r32.keep, r64.keep):
        both = (k32 & k64).reshape(-1)
        i32.append(o32 + (np.cumsum(k32.reshape(-1)) - 1)[both])
        i64.append(o64 + (np.cumsum(k64.reshape(-1)) - 1)[both])
        o32, o64 = o32 + int(k32.sum()), o64 + int(k64.sum())
    i32, i64 = np.concatenate(i32), np.concatenate(i64)
    yard = {k: float(np.abs(getattr(r32, k)[i32].astype(np.float64) - getattr(r64, k)[i64]).max()) for k in ("means", "scales", "colors")}
    yard["rotations"] = float(np.abs(wr.quaternion_to_matrix(r32.quaternions[i32]) - wr.quaternion_to_matrix(r64.quaternions[i64])).max())
    # yardsticks of the projections and of the relative depth error
    e32, e64 = relative_errors(r32.pairs, depths, np.float32), relative_errors(r64.pairs, depths, np.float64)
    yp = yr = 0.0
    for key in r64.pairs:
        same = (e32[key][0] == e64[key][0]) & (e64[key][0] >= 0)
        for a, b in zip(r32.pairs[key], r64.pairs[key]):
            yp = max(yp, float(np.abs(a[same].astype(np.float64) - b[same]).max(initial=0.0)))
        yr = max(yr, float(np.abs(e32[key][1][same].astype(np.float64) - e64[key][1][same]).max(initial=0.0)))
    yard["projection"], yard["relative_error"] = yp, yr
    # near pixels
    near = [np.zeros(d.shape, bool) for d in depths]
    for (i, j), (u, v, z) in r64.pairs.items():
        H, W = depths[j].shape
        half = lambda t: np.abs(t - np.floor(t) - 0.5)
        n = (half(u) <= 4 * yp) | (half(v) <= 4 * yp)
        n |= (np.abs(u) <= 4 * yp) | (np.abs(u - (W - 1)) <= 4 * yp) | (np.abs(v) <= 4 * yp) | (np.abs(v - (H - 1)) <= 4 * yp)
        tap, rel = e64[(i, j)]
        n |= (tap >= 0) & (np.abs(rel - wr.DEPTH_ERROR_THRESH) <= 4 * yr)
        near[i] |= n.reshape(near[i].shape)
    for v, (n, k32, k64, d) in enumerate(zip(near, r32.keep, r64.keep, depths)):
        assert n.sum() <= 0.01 * n.size, (v, int(n.sum()), n.size)
        assert np.array_equal(k32[~n], k64[~n]), v
        valid, cov = d > 0, r64.covered[v]
        print(f"  view {v}: near {int(n.sum())} of {n.size}, covered / uncovered valid {int(cov.sum())} / {int((valid & ~cov).sum())}, kept {int(k64.sum())}")
        if coverage_shares and v > 0:
            assert cov.sum() >= 0.1 * valid.sum() and (valid & ~cov).sum() >= 0.1 * valid.sum(), v
        assert np.array_equal(r32.covered[v][~n], cov[~n]), v
    print(f"  rows {len(r64.means)}, scales at the clamp {int((r64.scales[:, 0] == min_scale).sum())}, "
          f"cut {int(sum(((s >= max_scale) & ~c & (d > 0)).sum() for s, c, d in zip(r64.s, r64.covered, depths)))}")
    print("  yardstick", yard)
    flat = lambda maps: np.concatenate([m.reshape(-1) for m in maps])
    return dict(keep=flat(r64.keep), keep32=flat(r32.keep), near=flat(near), means=r64.means, scales=r64.scales,
                quaternions=r64.quaternions, colors=r64.colors, yardstick=json.dumps(yard))


def main():
    cams, depths, images = wr.scene(wr.GOLDEN_SIZES)
    out = dict(wvt=np.stack([c.world_view_transform for c in cams]), full=np.stack([c.full_proj_transform for c in cams]),
               fov=np.array([[c.FoVx, c.FoVy] for c in cams], np.float64), sizes=np.array(wr.GOLDEN_SIZES, np.int32),
               depths=np.concatenate([d.reshape(-1) for d in depths]), images=np.concatenate([i.reshape(-1) for i in images]),
               depth_error_thresh=np.float32(wr.DEPTH_ERROR_THRESH))
    for name, args in wr.RECORDINGS.items():
        print("recording", name, args)
        for k, v in record(cams, depths, images, coverage_shares=name == "A", **args).items():
            out[f"{name}_{k}"] = v
    np.savez_compressed(os.path.join(HERE, "warp_init.npz"), **out)


if __name__ == "__main__":
    main()
