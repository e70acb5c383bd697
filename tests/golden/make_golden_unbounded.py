"""Golden vectors of the unbounded TSDF, produced by RUNNING THE REFERENCE'S OWN CODE on the CPU of the build container:

    unbounded_tsdf.npz   2d-gaussian-splatting/utils/mesh_utils.py:184-279 `GaussianExtractor.extract_mesh_unbounded`,
                         called for real, with utils.mcube_utils.marching_cubes_with_contraction replaced by a stand-in
                         that captures the `sdf` closure, evaluates it on chosen contracted sample points and returns an
                         object whose `as_open3d.vertices` are chosen world points, and o3d.utility.Vector3dVector
                         replaced by one that captures the colours.  So the reference's own compute_unbounded_tsdf /
                         compute_sdf_perframe (contraction, adaptive truncation, grid_sample, running mean) produce both
                         the recorded tsdf of the contracted samples and the recorded colours of the world points.

Tolerance.  torch's grid_sample and matmul order their arithmetic differently from the contract, so agreement is to a
tolerance.  The same closure is run a second time in float64 (torch.set_default_dtype, float64 maps and cameras, and
Tensor.float made the identity for that run because the reference casts the vertices with .float()).
tol = 4 * max |ref32 - ref64| over the samples whose per-view decisions agree between float32 and float64; the factor 4
covers the different operation order.  The closure does not expose its decisions, so they are taken from the restatement
(tests/unbounded_ref.py) evaluated in float32 and in float64 on the same inputs; at most 0.1 % of the samples may
disagree.  tol and that count are stored in the npz.

Nothing of the reference is copied: the npz holds inputs and recorded results only.
Run in the build container only (needs /root/reference):  python tests/golden/make_golden_unbounded.py"""
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
RESOLUTION = 64      # voxel_size = 2 radius / 64 = 0.0625: exact in float32
CENTER = np.array([0.0625, -0.03125, 0.046875], np.float32)
RADIUS = 2.0
BACKGROUND = 8.0     # finite depth where the rays miss the sphere: the contracted zone is observed too
EYES = [(3.2, 0.3, 0.2), (-0.4, 3.0, 0.5), (-3.0, -0.6, 0.9), (0.5, -0.7, -3.1), (1.9, 1.8, 1.7)]


def make_inputs():
    import tsdf_ref
    from g4splat_amd import mesh as mesh_mod
    from g4splat_amd import synthetic
    rng = np.random.default_rng(2024)
    views = []
    for e in EYES:
        cam = synthetic.look_at_camera(e, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), math.radians(55), W, H)
        intr, E = mesh_mod.camera_intrinsics(cam), mesh_mod.camera_extrinsic(cam)
        depth = tsdf_ref.sphere_depth(E, intr, W, H, (0, 0, 0), 1.0)
        depth[depth <= 0] = BACKGROUND
        rgb = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
        views.append((np.ascontiguousarray(cam.full_proj_transform, np.float32), depth.astype(np.float32), rgb))
    # contracted samples: random directions, norms spread over [0, 3.3], plus the special norms
    n = 20000
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    norms = rng.uniform(0, 3.3, n)
    norms[: n // 4] = rng.uniform(0.1, 0.6, n // 4)  # many near the unit sphere of the world (|y| = 0.5 at radius 2)
    samples = (d * norms[:, None]).astype(np.float32)
    special = np.array([[0, 0, 0], [1, 0, 0], [0, -1, 0], [0, 0, 1], [0.6, 0.8, 0], [2, 0, 0], [0, 2, 0], [0, -1.2, 1.6],
                        [1.9, 1.9, 1.9], [-1.9, 1.9, -1.9], [0, 0, 3.3], [2.5, 0, 0], [0, -1.999, 0], [1.5, 0, 0]], np.float32)
    samples[: len(special)] = special
    # world points: in a box around the scene (some behind some cameras) and near the sphere's surface
    m = 2000
    world = rng.uniform(-3.5, 3.5, (m, 3))
    s = rng.normal(size=(m // 2, 3))
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    world[: m // 2] = s * rng.uniform(0.8, 1.3, (m // 2, 1))
    return views, samples, world.astype(np.float32)


def run_reference(views, samples, world, double):
    """(tsdf of the contracted samples, colours of the world points) from the reference's extract_mesh_unbounded."""
    dt = torch.float64 if double else torch.float32
    got = {}

    def fake_mc(sdf, bounding_box_min, bounding_box_max, level, resolution, inv_contraction):
        got["R"] = float(bounding_box_max[0])
        got["tsdf"] = sdf(torch.tensor(samples, dtype=dt)).numpy().copy()
        return types.SimpleNamespace(as_open3d=types.SimpleNamespace(vertices=world.astype(np.float64 if double else np.float32),
                                                                     vertex_colors=None))

    def vector3d(a):
        got["rgb"] = np.array(a)
        return got["rgb"]

    mcube = types.ModuleType("utils.mcube_utils")
    mcube.marching_cubes_with_contraction = fake_mc
    o3d = types.ModuleType("open3d")
    o3d.utility = types.SimpleNamespace(Vector3dVector=vector3d)
    tqdm = types.ModuleType("tqdm")
    tqdm.tqdm = lambda it, **k: it
    render_utils = types.ModuleType("utils.render_utils")
    render_utils.save_img_f32 = render_utils.save_img_u8 = None
    saved_float, saved_default = torch.Tensor.float, torch.get_default_dtype()
    try:
        if double:
            torch.set_default_dtype(torch.float64)
            torch.Tensor.float = lambda self, *a, **k: self
        with reference_modules({"utils.mcube_utils": mcube, "open3d": o3d, "tqdm": tqdm, "utils.render_utils": render_utils}):
            import utils.mesh_utils as ref_mesh
            ex = object.__new__(ref_mesh.GaussianExtractor)
            ex.viewpoint_stack = [types.SimpleNamespace(full_proj_transform=torch.tensor(M, dtype=dt)) for M, _d, _c in views]
            ex.depthmaps = [torch.tensor(d, dtype=dt)[None] for _M, d, _c in views]
            ex.rgbmaps = [torch.tensor(c, dtype=dt) for _M, _d, c in views]
            ex.center = torch.tensor(CENTER, dtype=dt)
            ex.radius = RADIUS
            ex.gaussians = types.SimpleNamespace(get_xyz=torch.tensor(samples[:500] * 2.0, dtype=dt))
            ex.extract_mesh_unbounded(resolution=RESOLUTION)
    finally:
        torch.Tensor.float = saved_float
        torch.set_default_dtype(saved_default)
    return got["tsdf"], got["rgb"], got["R"]


def main():
    import unbounded_ref as ur
    views, samples, world = make_inputs()
    voxel_size = RADIUS * 2 / RESOLUTION
    t32, c32, R = run_reference(views, samples, world, False)
    t64, c64, _ = run_reference(views, samples, world, True)
    assert t32.dtype == np.float32 and c32.dtype == np.float32 and t64.dtype == np.float64 and c64.dtype == np.float64
    # decisions in float32 and in float64, from the restatement
    agree = []
    for pts, contracted in ((samples, True), (world, False)):
        u32 = ur.sample(pts, views, CENTER, RADIUS, voxel_size, contracted)[3]
        u64 = ur.sample(pts, views, CENTER, RADIUS, voxel_size, contracted, dtype=np.float64)[3]
        agree.append((u32 == u64).all(1))
    n_disagree = int((~agree[0]).sum() + (~agree[1]).sum())
    assert n_disagree <= 0.001 * (len(samples) + len(world)), n_disagree
    err_t = np.abs(t32.astype(np.float64) - t64)[agree[0]].max()
    err_c = np.abs(c32.astype(np.float64) - c64)[agree[1]].max()
    tol = 4.0 * max(err_t, err_c)
    out = {"center": CENTER, "radius": np.float64(RADIUS), "voxel_size": np.float64(voxel_size), "R": np.float64(R),
           "samples": samples, "world": world, "tsdf": t32, "world_rgb": c32, "tol": np.float64(tol),
           "n_disagree": np.int64(n_disagree), "max_err32_64": np.array([err_t, err_c])}
    for i, (M, d, c) in enumerate(views):
        out[f"v{i}_fpt"], out[f"v{i}_depth"], out[f"v{i}_rgb"] = M, d, c
    path = os.path.join(HERE, "unbounded_tsdf.npz")
    np.savez_compressed(path, **out)
    print(f"wrote unbounded_tsdf.npz {os.path.getsize(path)} bytes; tol = {tol:.3e} (tsdf {err_t:.3e}, rgb {err_c:.3e} "
          f"between float32 and float64), decisions differ on {n_disagree} of {len(samples) + len(world)} samples; R = {R:.4f}")


if __name__ == "__main__":
    main()
