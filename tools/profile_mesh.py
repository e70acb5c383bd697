"""Time the TSDF fusion and marching cubes on the S3 scene (1.5 M surfels, 1600x1200, 8 views) with HIP events.

    python tools/profile_mesh.py [--out profiles/mesh_s3.json] [--depth-trunc X]

Renders the eight room views through render(), fuses them with g4splat_amd.mesh.TSDFVolume and extracts the mesh.
Every library call of the volume is bracketed by HIP events on the launch stream (per entry point: alloc_count =
emit + sort + unique + lookup + the count read-back; merge; integrate; extract_count; extract_emit).  depth_trunc
defaults to render.py's rule (2 x the radius of GaussianExtractor.estimate_bounding_sphere), voxel_size =
depth_trunc / 1024 and sdf_trunc = 5 voxel_size as in render.py.  Writes one JSON document.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g4splat_amd import _lib, mesh, synthetic  # noqa: E402
from g4splat_amd.gaussian_model import GaussianModel  # noqa: E402
from g4splat_amd.gaussian_renderer import render  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mesh_s3.json")
    ap.add_argument("--surfels", type=int, default=1_500_000)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--depth-trunc", type=float, default=-1.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sc = synthetic.scene_room(args.surfels, seed=0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    model = GaussianModel(sh_degree=3)
    model.create_from_parameters(t(sc.means3D), t(sc.scales), t(sc.rotations), t(synthetic.SH_C0 * sc.shs[:, 0] + 0.5))
    with torch.no_grad():
        p = np.clip(sc.opacities, 1e-4, 1 - 1e-4)
        model._opacity.copy_(t(np.log(p / (1 - p))))
    model.active_sh_degree = 0
    cams = [SimpleNamespace(image_width=c.image_width, image_height=c.image_height, FoVx=c.FoVx, FoVy=c.FoVy,
                            world_view_transform=t(c.world_view_transform), full_proj_transform=t(c.full_proj_transform),
                            camera_center=t(c.camera_center), znear=c.znear, zfar=c.zfar)
            for c in synthetic.room_cameras(args.views, args.width, args.height)]
    pipe = SimpleNamespace(depth_ratio=1.0, compute_cov3D_python=False, convert_SHs_python=False)
    ex = mesh.GaussianExtractor(model, render, pipe)
    ex.reconstruction(cams)
    torch.cuda.synchronize()
    depth_trunc = args.depth_trunc if args.depth_trunc > 0 else 2.0 * ex.radius
    voxel = depth_trunc / 1024
    sdf_trunc = 5 * voxel

    times = {}
    plain_call = _lib.call
    stream = torch.cuda.current_stream(dev)

    def timed_call(name, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        plain_call(name, *a)
        e1.record(stream)
        e1.synchronize()
        times.setdefault(name, []).append(e0.elapsed_time(e1))

    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    _lib.call = timed_call
    try:
        vol = mesh.TSDFVolume(voxel, sdf_trunc, depth_trunc, dev, initial_blocks=65536)
        per_view = []
        t0 = time.perf_counter()
        for cam, d, rgb in zip(cams, ex.depthmaps, ex.rgbmaps):
            m, n_new = vol.integrate(d, rgb, cam)
            per_view.append({"touched_blocks": m, "new_blocks": n_new})
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        m_out = vol.extract_triangle_mesh()
        t2 = time.perf_counter()
    finally:
        _lib.call = plain_call
    for i, pv in enumerate(per_view):
        for k in ("g4s_tsdf_alloc_count", "g4s_tsdf_merge", "g4s_tsdf_integrate"):
            if i < len(times.get(k, [])):
                pv[k.replace("g4s_tsdf_", "") + "_ms"] = times[k][i]
    res = {
        "scene": f"scene_room({args.surfels}), room_cameras({args.views}, {args.width}, {args.height}), depth_ratio 1",
        "radius": ex.radius, "depth_trunc": depth_trunc, "voxel_size": voxel, "sdf_trunc": sdf_trunc,
        "blocks": vol.num_blocks, "pool_blocks": vol.pool_blocks, "pool_grows": vol.grows,
        "vertices": int(len(m_out.vertices)), "triangles": int(len(m_out.triangles)),
        "per_view": per_view,
        "extract_count_ms": times.get("g4s_tsdf_extract_count", [None])[0],
        "extract_emit_ms": times.get("g4s_tsdf_extract_emit", [None])[0],
        "fusion_wall_s": t1 - t0, "extraction_wall_s_incl_host_copy": t2 - t1,
        "peak_bytes_above_maps": torch.cuda.max_memory_allocated(dev) - base,
        "build": _lib.load().g4s_version().decode(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "per_view"}))


if __name__ == "__main__":
    main()
