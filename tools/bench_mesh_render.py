"""Time the mesh rasteriser and the dilated depth against the byte floor of each path at the copy bandwidth measured in the
same process.  No earlier implementation exists to race (pytorch3d is not available on this platform), so the yardstick
is what the path has to move.

    python tools/bench_mesh_render.py [--rounds 5] [--out profiles/mesh_render_summary.txt]

(a) render_mesh at 1600 x 1200 of a mesh of about 2 x 10^6 faces: dense_marching_cubes of the analytic field
    cos(k x) + cos(k y) + cos(k z) over a 320^3 lattice.
(b) dilated_depths over the stage stack -- 50 views of 800 x 600 plus 30 of 512 x 512 -- and beside it adaptive_tsdf over
    the same stack at 10^6 points: the overhead of use_dilated_depth as a ratio to the step it feeds.

Byte floors.  Dilate, per pixel: depth and rgb in (16 B), the vertex out and back in (24 B), the key initialised, updated
and read once (24 B), depth and rgb out (16 B) = 80 B.  Raster: 12 B per face for its indices plus 12 B per vertex
gathered, the same 24 B of key traffic per pixel, and the resolve's outputs (pix_to_face 4, depth 4, bary 12, rgb 12,
normal 12 = 44 B per pixel).  What is timed is the public call (workspace and outputs allocated, the view table staged),
between HIP events, after one warm-up; median and range of --rounds rounds."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from g4splat_amd import _lib, mesh, mesh_render, synthetic  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def timed(fn, rounds):
    fn()
    torch.cuda.synchronize()
    return [event_ms(fn)[1] for _ in range(rounds)]


def copy_bandwidth(dev, rounds):
    """GB/s of a device-to-device copy of 1 GiB (read + write counted)."""
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    ms = timed(lambda: dst.copy_(src), rounds)
    return 2 * src.numel() * 4 / (statistics.median(ms) * 1e-3) / 1e9


def pinhole(W, H, f, t=(0.0, 0.0, 0.0)):
    Pm = np.zeros((4, 4), np.float32)
    Pm[0, 0], Pm[1, 1], Pm[2, 2], Pm[2, 3], Pm[3, 2] = 2.0 * f / W, 2.0 * f / H, 1.0, 1.0, -0.01
    Wv = np.eye(4, dtype=np.float32)
    Wv[3, :3] = t
    return Wv, Pm


def stage_stack(dev, seed=0):
    """50 views of 800 x 600 and 30 of 512 x 512: a wavy wall at depth about 3, random colours."""
    rng = np.random.default_rng(seed)
    views = []
    for k in range(80):
        W, H = (800, 600) if k < 50 else (512, 512)
        ii, jj = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
        depth = (3.0 + 0.5 * torch.sin(jj / 37.0 + k) + 0.4 * torch.cos(ii / 23.0 - k)).float()
        rgb = torch.rand((3, H, W), device=dev)
        views.append((pinhole(W, H, 0.8 * W, (rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.5, 0.5))), depth, rgb))
    return views


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lattice", type=int, default=320)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--out", default="profiles/mesh_render_summary.txt")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    fmt = lambda v: f"{statistics.median(v):9.3f} ({min(v):.3f}-{max(v):.3f})"
    bw = copy_bandwidth(dev, args.rounds)
    floor_ms = lambda nbytes: nbytes / (bw * 1e9) * 1e3

    # (a) the rasteriser
    N = args.lattice
    x = torch.linspace(-0.9, 0.9, N, device=dev)
    k = 2 * math.pi * 4 / 1.8  # four periods across the lattice
    c = torch.cos(k * x)
    field = (c[:, None, None] + c[None, :, None] + c[None, None, :]).contiguous()
    verts, tris = mesh.dense_marching_cubes(field, 0.9, (0.0, 0.0, 0.0), 1.0, to_host=False)
    del field
    dm = mesh.DeviceMesh(verts, torch.rand_like(verts), tris)
    W, H = 1600, 1200
    cam = synthetic.look_at_camera((1.6, -2.1, 1.2), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), math.radians(50), W, H)
    cam = (torch.as_tensor(cam.world_view_transform), mesh._projection_matrix(cam))
    render = lambda: mesh_render.render_mesh(dm, cam, image_size=(H, W))
    maps = render()
    covered = float((maps["pix_to_face"] >= 0).float().mean())
    seen = int(mesh_render.visible_face_mask(dm, [cam], [(H, W)]).sum())
    raster_ms = timed(render, args.rounds)
    F, V = tris.size(0), verts.size(0)
    raster_bytes = 12 * F + 12 * V + (24 + 44) * W * H

    # (b) the dilated depth beside the step it feeds
    views = stage_stack(dev)
    pixels = sum(d.numel() for _c, d, _r in views)
    dilate = lambda: mesh_render.dilated_depths(views, 1.5, 0.01)
    dilate_ms = timed(dilate, args.rounds)
    no_rgb = [(cam_, d, None) for cam_, d, _r in views]
    dilate_depth_ms = timed(lambda: mesh_render.dilated_depths(no_rgb, 1.5, 0.01), args.rounds)
    points = (torch.rand((args.points, 3), device=dev) - 0.5) * torch.tensor([4.0, 4.0, 2.0], device=dev) + torch.tensor([0.0, 0.0, 3.0], device=dev)
    tsdf_ms = timed(lambda: mesh.adaptive_tsdf(points, no_rgb, 0.05), args.rounds)
    dilate_bytes, dilate_depth_bytes = 80 * pixels, (80 - 24) * pixels

    med = statistics.median
    lines = [f"mesh rasteriser and dilated depth; {torch.cuda.get_device_name(0)}; {_lib.load().g4s_version().decode()}",
             f"copy bandwidth measured in this process (1 GiB device-to-device, read + write): {bw:.0f} GB/s",
             f"HIP-event times of the public calls in ms: median (min-max) of {args.rounds} rounds after one warm-up", "",
             f"(a) render_mesh at {W} x {H}: {F} faces, {V} vertices (dense_marching_cubes of a {N}^3 lattice); "
             f"{100 * covered:.1f} % of the pixels covered, {seen} faces win a pixel",
             f"    render_mesh                         {fmt(raster_ms)}",
             f"    byte floor {raster_bytes / 1e6:.1f} MB                 {floor_ms(raster_bytes):9.3f}   time / floor = {med(raster_ms) / floor_ms(raster_bytes):.1f}", "",
             f"(b) dilated_depths over 50 views of 800 x 600 + 30 of 512 x 512 = {pixels} pixels",
             f"    depth and rgb                       {fmt(dilate_ms)}",
             f"    byte floor {dilate_bytes / 1e6:.1f} MB               {floor_ms(dilate_bytes):9.3f}   time / floor = {med(dilate_ms) / floor_ms(dilate_bytes):.1f}",
             f"    depth only (the sdf pass)           {fmt(dilate_depth_ms)}",
             f"    byte floor {dilate_depth_bytes / 1e6:.1f} MB               {floor_ms(dilate_depth_bytes):9.3f}   time / floor = {med(dilate_depth_ms) / floor_ms(dilate_depth_bytes):.1f}",
             f"    adaptive_tsdf, {args.points} points, same stack   {fmt(tsdf_ms)}",
             f"    use_dilated_depth adds {med(dilate_depth_ms) / med(tsdf_ms):.2f} x the sample it feeds", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
