"""Time the unbounded mesh extraction on the synthetic room (the S3 room of tools/bench_mesh_export.py, its rendered
views): the fused lattice kernel, the dense marching cubes and the vertex colouring, each between HIP events, beside a
plain torch formulation of the contract's per-view update on the same GPU.

    python tools/bench_mesh_unbounded.py [--resolutions 512 1024] [--rounds 5] [--out profiles/mesh_unbounded_summary.txt]

The torch formulation is written from include/g4s_render_maps.h ("Unbounded TSDF and dense marching cubes"), one
element-wise torch call per operation of the contract, and evaluates the lattice in chunks of 256^3 points as the
reference's marching_cubes_with_contraction does.  It is checked against the fused kernel's lattice to the tolerance of
tests/golden/unbounded_tsdf.npz before anything is timed.  Timing: one warm-up of each, then --rounds rounds that
alternate fused kernel / torch formulation, so that clock and thermal drift hit both alike; median and range are
reported.  Peak device memory is torch's max_memory_allocated over one whole extract_mesh_unbounded call (the views and
the model are resident too; their share is reported)."""
import argparse
import os
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from g4splat_amd import _lib, mesh, synthetic  # noqa: E402
from g4splat_amd.gaussian_model import GaussianModel  # noqa: E402
from g4splat_amd.gaussian_renderer import render  # noqa: E402

CHUNK = 256 ** 3


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def torch_lattice_chunk(first, count, N, R, views, center, radius, voxel_size):
    """tsdf of lattice points [first, first + count) in storage order: the contract, one torch call per operation."""
    dev = center.device
    one = torch.tensor(1.0, device=dev)
    h = (2.0 * torch.tensor(R, dtype=torch.float32, device=dev)) / float(N - 1)
    idx = torch.arange(first, first + count, device=dev, dtype=torch.int64)
    ijk = (idx % N, (idx // N) % N, idx // (N * N))
    y = [-R + c.to(torch.float32) * h for c in ijk]
    m = torch.sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2])
    s = 1.0 / (2.0 - m)
    inner = m < 1
    p = [torch.where(inner, y[c], s * (y[c] / m)) * radius + center[c] for c in range(3)]
    T = torch.full_like(m, 5.0) * voxel_size
    T = torch.where(m > 1, T * (1.0 / (2.0 - torch.clamp(m, max=1.9))), T)
    tsdf, w = torch.ones_like(m), torch.ones_like(m)
    for M, depth in views:
        W, H = depth.shape[1], depth.shape[0]
        hc = [((p[0] * M[0, c] + p[1] * M[1, c]) + p[2] * M[2, c]) + M[3, c] for c in (0, 1, 3)]
        z = hc[2]
        px, py = hc[0] / z, hc[1] / z
        inside = (px > -1) & (px < 1) & (py > -1) & (py < 1) & (z > 0)
        ix, iy = ((px + 1) / 2) * float(W - 1), ((py + 1) / 2) * float(H - 1)
        ix, iy = torch.where(inside, ix, torch.zeros_like(ix)), torch.where(inside, iy, torch.zeros_like(iy))
        fx0, fy0 = torch.floor(ix), torch.floor(iy)
        x0, y0 = fx0.to(torch.int64), fy0.to(torch.int64)
        x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
        fx, fy = ix - fx0, iy - fy0
        flat = depth.reshape(-1)
        d = ((flat[y0 * W + x0] * ((1 - fx) * (1 - fy)) + flat[y0 * W + x1] * (fx * (1 - fy))) + flat[y1 * W + x0] * ((1 - fx) * fy)) \
            + flat[y1 * W + x1] * (fx * fy)
        sdf = d - z
        use = inside & (sdf > -T)
        t = torch.minimum(one, torch.maximum(-one, sdf / T))
        tsdf = torch.where(use, (tsdf * w + t) / (w + 1), tsdf)
        w = torch.where(use, w + 1, w)
    return tsdf


def torch_lattice(N, R, views, center, radius, voxel_size, out):
    for first in range(0, N ** 3, CHUNK):
        count = min(CHUNK, N ** 3 - first)
        out[first:first + count] = torch_lattice_chunk(first, count, N, R, views, center, radius, voxel_size)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--surfels", type=int, default=400_000)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/mesh_unbounded_summary.txt")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sc = synthetic.scene_room(args.surfels, seed=4, scale_mean=0.03, scale_sigma=0.2)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    model = GaussianModel(sh_degree=3)
    model.create_from_parameters(t(sc.means3D), t(sc.scales), t(sc.rotations), t(np.full((len(sc.means3D), 3), 0.5, np.float32)))
    with torch.no_grad():
        model._opacity.fill_(float(np.log(0.97 / 0.03)))
    model.active_sh_degree = 0
    cams = [SimpleNamespace(image_width=c.image_width, image_height=c.image_height, FoVx=c.FoVx, FoVy=c.FoVy,
                            world_view_transform=t(c.world_view_transform), full_proj_transform=t(c.full_proj_transform),
                            camera_center=t(c.camera_center), znear=c.znear, zfar=c.zfar)
            for c in synthetic.room_cameras(args.views, args.width, args.height)]
    pipe = SimpleNamespace(depth_ratio=1.0, compute_cov3D_python=False, convert_SHs_python=False)
    ex = mesh.GaussianExtractor(model, render, pipe)
    ex.reconstruction(cams)
    tol = float(np.load(os.path.join(ROOT, "tests", "golden", "unbounded_tsdf.npz"))["tol"])
    tviews = [(c.full_proj_transform.float(), d[0].float().contiguous()) for c, d in zip(cams, ex.depthmaps)]
    lines = [f"unbounded mesh extraction: scene_room({args.surfels}) rendered from room_cameras({args.views}, {args.width}, "
             f"{args.height}); radius {ex.radius:.4f}; {torch.cuda.get_device_name(0)}; {_lib.load().g4s_version().decode()}",
             f"HIP-event times in ms: median (min-max) of {args.rounds} rounds after one warm-up, fused kernel and torch "
             f"formulation alternating; torch formulation in chunks of 256^3 points; agreement tolerance {tol:.3e}", ""]
    resident = torch.cuda.memory_allocated()
    for N in args.resolutions:
        voxel = ex.radius * 2 / N
        torch.cuda.reset_peak_memory_stats()
        dm = ex.extract_mesh_unbounded(resolution=N, to_host=False, keep_grid=True)  # warm-up of all three passes
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        R, views = ex.unbounded_R, ex._unbounded_views()
        fused = ex.unbounded_tsdf
        other = torch_lattice(N, R, tviews, ex.center, ex.radius, voxel, torch.empty_like(fused))  # warm-up + check
        diff = (other - fused).abs()
        beyond = int((~(diff <= tol)).sum())
        agree = f"max |torch - fused| {float(diff.max()):.3e}, {beyond} of {N ** 3} points beyond the tolerance"
        assert beyond <= 1e-4 * N ** 3, agree
        del diff
        ms = {"grid": [], "torch": [], "cubes": [], "colour": []}
        for _ in range(args.rounds):
            ms["grid"].append(event_ms(lambda: mesh.unbounded_tsdf_grid(N, R, views, ex.center, ex.radius, voxel, dev))[1])
            ms["torch"].append(event_ms(lambda: torch_lattice(N, R, tviews, ex.center, ex.radius, voxel, other))[1])
            (verts, tris), c = event_ms(lambda: mesh.dense_marching_cubes(fused, R, ex.center, ex.radius, 32.0, to_host=False))
            ms["cubes"].append(c)
            ms["colour"].append(event_ms(lambda: mesh.unbounded_tsdf(verts, views, ex.center, ex.radius, voxel, contracted=False,
                                                                      return_rgb=True))[1])
        fmt = lambda v: f"{statistics.median(v):10.2f} ({min(v):.2f}-{max(v):.2f})"
        lines += [f"resolution {N}: R {R:.4f}, voxel_size {voxel:.6f}, {dm.vertices.size(0)} vertices, {dm.triangles.size(0)} triangles",
                  f"  fused lattice kernel (g4s_utsdf_grid, {args.views} views) {fmt(ms['grid'])}",
                  f"  torch formulation, {-(-N ** 3 // CHUNK)} chunks               {fmt(ms['torch'])}"
                  f"   = {statistics.median(ms['torch']) / statistics.median(ms['grid']):.1f} x the fused kernel",
                  f"  dense marching cubes (count + emit)               {fmt(ms['cubes'])}",
                  f"  vertex colours (g4s_utsdf_sample, world mode)     {fmt(ms['colour'])}",
                  f"  {agree}",
                  f"  peak device memory of extract_mesh_unbounded {peak / 2 ** 20:.0f} MiB, of which {resident / 2 ** 20:.0f} MiB "
                  f"model and views", ""]
        ex.unbounded_tsdf = None
        del fused, other, dm, verts, tris
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
