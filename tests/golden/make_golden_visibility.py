"""Golden vectors of the visibility grid, produced by RUNNING THE REFERENCE'S OWN CODE on the CPU of the build container:

    visibility_grid.npz   guidance/vis_grid.py `VisibilityGrid` (its grid, `check_valid_camera_center`,
                          `render_visibility_map`), guidance/cam_utils.py `check_valid_camera_center_by_depth` and
                          `build_visibility_masks`, planes/get_global_3Dpnts.py `get_visible_mask_for_input_views` and
                          matcha/dm_scene/charts.py `depths_to_points_parallel`, imported and called for real.  The packages
                          this image lacks (pytorch3d, pytransform3d, the matcha modules charts.py imports without using
                          them here, the dataset readers) are empty stand-ins; cam_utils.to_tensor_safe, which hard-codes
                          device='cuda' and float32, is replaced after import by one for the CPU and the default dtype.

Scene.  The five look-at cameras of make_golden_unbounded.py at 64 x 48, the analytic depth of the unit sphere with a
background depth of 5, the box [-2.03, -1.97, -2.11] .. [2.07, 2.01, 1.93].  The grid is built from the first four views at
R = 32 and R = 48 and marched from all five.

Decisions.  Every recorded output but the point clouds is a decision.  torch orders its matmuls differently from the
contract, so a decision at an edge may differ; everything is therefore run a second time in float64
(torch.set_default_dtype, float64 cameras and maps, Tensor.float made .to(float64)), and so is the restatement
(tests/visibility_ref.py).  The agreed set of an output = the elements on which ref32 == ref64 and
restatement32 == restatement64; its complement may hold at most 0.1 % of the output (asserted here, counts stored).  The
test demands equality on the agreed set.  Point clouds: tol = 4 * max |ref32 - ref64|, the factor of the other goldens.

Nothing of the reference is copied: the npz holds inputs and recorded results only.
Run in the build container only (needs /root/reference):  python tests/golden/make_golden_visibility.py"""
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from _ref_import import reference_modules  # noqa: E402

W, H = 64, 48
EYES = [(3.2, 0.3, 0.2), (-0.4, 3.0, 0.5), (-3.0, -0.6, 0.9), (0.5, -0.7, -3.1), (1.9, 1.8, 1.7)]
BACKGROUND = 5.0
BBOX_MIN = np.array([-2.03, -1.97, -2.11], np.float32)
BBOX_MAX = np.array([2.07, 2.01, 1.93], np.float32)
RESOLUTIONS = (32, 48)
N_INPUT = 4
THRESHOLD = 0.1


def make_inputs():
    import visibility_ref as vr
    from g4splat_amd import synthetic
    rng = np.random.default_rng(2025)
    cams = [synthetic.look_at_camera(e, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), math.radians(55), W, H) for e in EYES]
    depths = [vr.sphere_depth(c, W, H, 1.0, BACKGROUND) for c in cams]
    # explicit points: in and around the box, many near the sphere's surface, the camera centres, the box's corners
    n = 4000
    pts = rng.uniform(-2.6, 2.6, (n, 3))
    s = rng.normal(size=(n // 2, 3))
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    pts[: n // 2] = s * rng.uniform(0.9, 1.1, (n // 2, 1))
    special = np.concatenate([np.asarray(EYES), [BBOX_MIN, BBOX_MAX, (BBOX_MIN + BBOX_MAX) / 2]])
    pts[-len(special):] = special
    return cams, depths, pts.astype(np.float32)


def _stubs():
    def module(name, **names):
        m = types.ModuleType(name)
        for k, v in names.items():
            setattr(m, k, v)
        return m

    class GSCamera:
        pass

    pytransform3d = module("pytransform3d")
    pytransform3d.visualizer = module("pytransform3d.visualizer")
    pytorch3d = module("pytorch3d")
    pytorch3d.transforms = module("pytorch3d.transforms", quaternion_apply=None)
    return {
        "pytransform3d": pytransform3d, "pytransform3d.visualizer": pytransform3d.visualizer,
        "pytorch3d": pytorch3d, "pytorch3d.transforms": pytorch3d.transforms,
        "matcha.dm_scene.meshes": module("matcha.dm_scene.meshes", get_manifold_meshes_from_pointmaps=None,
                                         remove_faces_from_single_mesh=None),
        "matcha.dm_scene.gaussians": module("matcha.dm_scene.gaussians", get_gaussian_surfel_parameters_from_mesh=None),
        "matcha.dm_utils.rendering": module("matcha.dm_utils.rendering", depth2normal_parallel=None,
                                            normal2curv_parallel=None),
        "matcha.dm_scene.cameras": module("matcha.dm_scene.cameras", GSCamera=GSCamera),
        "scene.dataset_readers": module("scene.dataset_readers", load_see3d_cameras=None, load_cameras=None),
    }


def run_reference(cams, depths, points, double):
    """Every recorded output of the reference, as numpy arrays."""
    dt = torch.float64 if double else torch.float32
    npdt = np.float64 if double else np.float32
    out = {}
    saved_float, saved_default = torch.Tensor.float, torch.get_default_dtype()
    try:
        if double:
            torch.set_default_dtype(torch.float64)
            torch.Tensor.float = lambda self, *a, **k: self.to(torch.float64)
        with reference_modules(_stubs()):
            sys.path.insert(0, "/root/reference")
            import guidance.cam_utils as cam_utils
            cam_utils.to_tensor_safe = lambda data, dtype=None, device=None: torch.as_tensor(np.asarray(data)).to(dt)
            import guidance.vis_grid as vis_grid
            import planes.get_global_3Dpnts as g3d
            from matcha.dm_scene.charts import depths_to_points_parallel
            ref_cams = []
            for i, c in enumerate(cams):
                wvt = np.asarray(c.world_view_transform, npdt)
                ref_cams.append(types.SimpleNamespace(
                    R=wvt[:3, :3].copy(), T=wvt[3, :3].copy(), FoVx=c.FoVx, FoVy=c.FoVy, image_width=W, image_height=H,
                    world_view_transform=torch.tensor(wvt, dtype=dt),
                    full_proj_transform=torch.tensor(np.asarray(c.full_proj_transform, npdt), dtype=dt), image_name=f"v{i}"))
            maps = [torch.tensor(d, dtype=dt) for d in depths]
            pts = torch.tensor(points, dtype=dt)
            for R in RESOLUTIONS:
                grid = vis_grid.VisibilityGrid(torch.tensor(BBOX_MIN, dtype=dt), torch.tensor(BBOX_MAX, dtype=dt), R,
                                               ref_cams[:N_INPUT], maps[:N_INPUT], device="cpu")
                out[f"grid{R}"] = (grid.visibility_grid.numpy() > 0.5).reshape(-1)
                out[f"maps{R}"] = np.stack([m.numpy() > 0.5 for m in
                                            grid.render_visibility_map(ref_cams, [m.clone() for m in maps])])
                out[f"centres{R}"] = grid.check_valid_camera_center(pts).numpy()
            out["free"] = cam_utils.check_valid_camera_center_by_depth(ref_cams, maps, pts).numpy()
            out["surface"] = g3d.get_visible_mask_for_input_views(ref_cams, maps, pts, THRESHOLD).numpy()
            clouds = [depths_to_points_parallel(m[None], [c])[0] for m, c in zip(maps, ref_cams)]
            out["clouds"] = np.stack([c.numpy() for c in clouds])
            maps3 = [m[None] for m in maps]
            out["times"] = np.stack([m.numpy() for m in cam_utils.build_visibility_masks(
                ref_cams, maps3, clouds, depth_threshold=THRESHOLD, return_origin_masks=True)])
            for k in (1, 2):
                out[f"masks{k}"] = np.stack([m.numpy() > 0.5 for m in cam_utils.build_visibility_masks(
                    ref_cams, maps3, clouds, depth_threshold=THRESHOLD, least_num_views=k)])
    finally:
        torch.Tensor.float = saved_float
        torch.set_default_dtype(saved_default)
    return out


def run_restatement(cams, depths, points, clouds, dtype):
    """The same outputs from tests/visibility_ref.py; the masks use the reference's point clouds, as the test will."""
    import visibility_ref as vr
    out = {}
    views = list(zip(cams, depths))
    for R in RESOLUTIONS:
        bits = vr.build(BBOX_MIN, BBOX_MAX, R, views[:N_INPUT], dtype)
        out[f"grid{R}"] = bits
        out[f"maps{R}"] = np.stack([vr.march(bits, BBOX_MIN, BBOX_MAX, R, d, c, dtype=dtype) > 0.5 for c, d in views])
        out[f"centres{R}"] = vr.sample(bits, points, BBOX_MIN, BBOX_MAX, R, dtype)
    out["free"] = vr.check_valid_camera_center_by_depth(cams, depths, points, dtype)
    out["surface"] = vr.get_visible_mask_for_input_views(cams, depths, points, THRESHOLD, dtype)
    out["times"] = np.stack(vr.build_visibility_masks(cams, depths, clouds, THRESHOLD, return_origin_masks=True, dtype=dtype))
    for k in (1, 2):
        out[f"masks{k}"] = np.stack(vr.build_visibility_masks(cams, depths, clouds, THRESHOLD, k, dtype=dtype)) > 0.5
    return out


def main():
    cams, depths, points = make_inputs()
    r32 = run_reference(cams, depths, points, False)
    r64 = run_reference(cams, depths, points, True)
    assert r32["clouds"].dtype == np.float32 and r64["clouds"].dtype == np.float64
    s32 = run_restatement(cams, depths, points, r32["clouds"], np.float32)
    s64 = run_restatement(cams, depths, points, r64["clouds"], np.float64)
    out = {"bbox_min": BBOX_MIN, "bbox_max": BBOX_MAX, "resolutions": np.array(RESOLUTIONS), "n_input": np.int64(N_INPUT),
           "threshold": np.float64(THRESHOLD), "points": points, "depths": np.stack(depths),
           "wvt": np.stack([c.world_view_transform for c in cams]), "full": np.stack([c.full_proj_transform for c in cams]),
           "fov": np.array([[c.FoVx, c.FoVy] for c in cams], np.float64)}
    report = []
    for key in sorted(s32):
        a32, a64 = np.asarray(r32[key]), np.asarray(r64[key])
        ref_differ = a32.astype(np.float64) != a64.astype(np.float64)
        agreed = ~ref_differ & (np.asarray(s32[key]).astype(np.float64) == np.asarray(s64[key]).astype(np.float64))
        excluded = int((~agreed).sum())
        assert excluded <= 0.001 * agreed.size, (key, excluded, agreed.size)
        out[key] = np.packbits(a32.reshape(-1)) if a32.dtype == bool else a32
        out[key + "_ref64"] = np.packbits(a64.reshape(-1)) if a64.dtype == bool else a64.astype(np.float32)
        out[key + "_agreed"] = np.packbits(agreed.reshape(-1))
        out[key + "_shape"] = np.array(a32.shape)
        out[key + "_excluded"] = np.array([excluded, agreed.size, int(ref_differ.sum())])
        report.append(f"{key}: ref32 != ref64 on {int(ref_differ.sum())}, excluded {excluded} of {agreed.size}, "
                      f"true on {float(np.mean(a32 > 0)):.3f}")
    err = float(np.abs(r32["clouds"].astype(np.float64) - r64["clouds"]).max())
    out["clouds"] = r32["clouds"]
    out["tol"] = np.float64(4.0 * err)
    path = os.path.join(HERE, "visibility_grid.npz")
    np.savez_compressed(path, **out)
    print(f"wrote visibility_grid.npz {os.path.getsize(path)} bytes; cloud tol = {4.0 * err:.3e}")
    print("\n".join(report))


if __name__ == "__main__":
    main()
