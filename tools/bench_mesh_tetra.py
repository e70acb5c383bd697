"""Time the tetrahedral mesh extraction on the synthetic room (the S3 room of tools/bench_mesh_export.py, its rendered
views): the point TSDF, the marching tetrahedra and the fused bisection, each between HIP events, beside a plain torch
formulation of the same contract on the same GPU.  What is timed is the public call of g4splat_amd.mesh (view table built
and staged, workspace allocated, counts read by the host), which is what a caller pays, not the bare launches.

    python tools/bench_mesh_tetra.py [--downsample 0.5] [--rounds 5] [--out profiles/mesh_tetra_summary.txt]

The torch formulation is written from include/g4s_render_maps.h ("Adaptive TSDF at points and marching tetrahedra"), one
element-wise torch call per operation of the contract: the field per view as the reference integrates it, the marching
tetrahedra through torch.unique over the edge keys, and the bisection as eight passes of the field over the view stack.
Each is checked EQUAL to the kernels' output before anything is timed (tsdf and vertices bit for bit, edges and faces as
integers).  The tetrahedralisation itself is the host's (scipy) and is timed apart.  Timing: one warm-up of each, then
--rounds rounds that alternate kernel / torch formulation; median and range are reported."""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_mtet_table  # noqa: E402
from g4splat_amd import _lib, mesh, synthetic  # noqa: E402
from g4splat_amd.gaussian_model import GaussianModel  # noqa: E402
from g4splat_amd.gaussian_renderer import render  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def torch_tsdf(p, views, trunc, znear=1e-6, zfar=1e6):
    """The contract's field at points p [n,3], one torch call per operation; views: (Wv [4,4], Pm [4,4], depth [H,W])."""
    # 0-dim float32 tensors: a Python scalar divisor would be turned into a multiplication by its reciprocal
    trunc, znear, zfar = (torch.tensor(float(a), dtype=torch.float32, device=p.device) for a in (trunc, znear, zfar))
    x, y, z3 = p[:, 0], p[:, 1], p[:, 2]
    tsdf, w = torch.full_like(x, -1.0), torch.zeros_like(x)
    for Wv, Pm, depth in views:
        H, W = depth.shape
        v = [((x * Wv[0, c] + y * Wv[1, c]) + z3 * Wv[2, c]) + Wv[3, c] for c in range(3)]
        q = {c: ((v[0] * Pm[0, c] + v[1] * Pm[1, c]) + v[2] * Pm[2, c]) + Pm[3, c] for c in (0, 1, 3)}
        qw = torch.where(q[3] > znear, q[3], znear.expand_as(q[3]))
        ix, iy = ((1.0 + q[0] / qw) * float(W)) / 2.0, ((1.0 + q[1] / qw) * float(H)) / 2.0
        z = v[2]
        used = (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1) & (z > znear) & (z < zfar)
        ix, iy = torch.where(used, ix, torch.zeros_like(ix)), torch.where(used, iy, torch.zeros_like(iy))
        fx0, fy0 = torch.floor(ix), torch.floor(iy)
        x0, y0 = fx0.to(torch.int64), fy0.to(torch.int64)
        x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
        fx, fy = ix - fx0, iy - fy0
        flat = depth.reshape(-1)
        d = ((flat[y0 * W + x0] * ((1 - fx) * (1 - fy)) + flat[y0 * W + x1] * (fx * (1 - fy))) + flat[y1 * W + x0] * ((1 - fx) * fy)) \
            + flat[y1 * W + x1] * (fx * fy)
        diff = d - z
        used = used & (d > 0) & (diff >= -trunc)
        dist = torch.clamp(diff / trunc, max=1.0)
        tsdf = torch.where(used, (tsdf * w + dist) / (w + 1), tsdf)
        w = torch.where(used, w + 1, w)
    return tsdf


_EDGES = torch.tensor(gen_mtet_table.EDGES)
_TRIS = torch.tensor([[e for tri in t for e in tri] + [0] * (6 - 3 * len(t)) for t in gen_mtet_table.table()])
_NTRI = torch.tensor([len(t) for t in gen_mtet_table.table()])


def torch_mtet(tets, sdf):
    """(edges, faces) of the contract through torch.unique, faces in tet order."""
    dev = tets.device
    t = tets.long()
    occ = sdf > 0
    case = (occ[t].long() << torch.arange(4, device=dev)).sum(1)
    ntri = _NTRI.to(dev)[case]
    sel = ntri > 0
    t, case, ntri = t[sel], case[sel], ntri[sel]
    pairs = t[:, _EDGES.to(dev)]  # [m,6,2]
    keys = (pairs.min(-1).values << 32) | pairs.max(-1).values  # [m,6]
    crossing = occ[pairs[..., 0]] != occ[pairs[..., 1]]
    uniq = torch.unique(keys[crossing])
    edges = torch.stack([uniq >> 32, uniq & 0xFFFFFFFF], 1).to(torch.int32)
    vid = torch.searchsorted(uniq, torch.gather(keys, 1, _TRIS.to(dev)[case]))  # [m,6]
    keep = (torch.arange(2, device=dev)[None] < ntri[:, None]).reshape(-1)
    return edges, vid.reshape(-1, 3)[keep].to(torch.int32)


def torch_bisect(p, edges, sdf, views, trunc, steps=8):
    e = edges.long()
    l, r, ls = p[e[:, 0]].clone(), p[e[:, 1]].clone(), sdf[e[:, 0]].clone()
    for _ in range(steps):
        m = (l + r) / 2
        ms = torch_tsdf(m, views, trunc)
        low = ((ms < 0) & (ls < 0)) | ((ms > 0) & (ls > 0))
        l, r, ls = torch.where(low[:, None], m, l), torch.where(low[:, None], r, m), torch.where(low, ms, ls)
    return (l + r) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--downsample", type=float, default=0.5)
    ap.add_argument("--surfels", type=int, default=400_000)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/mesh_tetra_summary.txt")
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
    extent = mesh.cameras_spatial_extent(cams)
    trunc = 5e-3 * extent
    points, _scale = mesh.tetra_points(model, args.downsample, 2e-4 * extent, generator=torch.Generator().manual_seed(0))
    t0 = time.perf_counter()
    cells = mesh.triangulate(points)
    host_s = time.perf_counter() - t0
    views = [(c, d, None) for c, d in zip(cams, ex.depthmaps)]
    tviews = [(c.world_view_transform.float(), t(mesh._projection_matrix(c)), d[0].float().contiguous())
              for c, d in zip(cams, ex.depthmaps)]
    # warm-up and the equality checks
    sdf = mesh.adaptive_tsdf(points, views, trunc)
    edges, faces = mesh.marching_tetrahedra(points, cells, sdf)
    verts = mesh.bisect_surface(points, edges, sdf, views, trunc, steps=8)
    assert torch.equal(torch_tsdf(points, tviews, trunc).view(torch.int32), sdf.view(torch.int32)), "torch field differs"
    te, tf = torch_mtet(cells, sdf)
    assert torch.equal(te, edges) and torch.equal(tf, faces), "torch marching tetrahedra differ"
    assert torch.equal(torch_bisect(points, edges, sdf, tviews, trunc).view(torch.int32), verts.view(torch.int32)), \
        "torch bisection differs"
    names = ["tsdf", "tsdf_torch", "mtet", "mtet_torch", "bisect", "bisect_torch"]
    ms = {k: [] for k in names}
    for _ in range(args.rounds):
        ms["tsdf"].append(event_ms(lambda: mesh.adaptive_tsdf(points, views, trunc))[1])
        ms["tsdf_torch"].append(event_ms(lambda: torch_tsdf(points, tviews, trunc))[1])
        ms["mtet"].append(event_ms(lambda: mesh.marching_tetrahedra(points, cells, sdf))[1])
        ms["mtet_torch"].append(event_ms(lambda: torch_mtet(cells, sdf))[1])
        ms["bisect"].append(event_ms(lambda: mesh.bisect_surface(points, edges, sdf, views, trunc, steps=8))[1])
        ms["bisect_torch"].append(event_ms(lambda: torch_bisect(points, edges, sdf, tviews, trunc))[1])
    fmt = lambda v: f"{statistics.median(v):10.2f} ({min(v):.2f}-{max(v):.2f})"
    ratio = lambda a, b: f"   = {statistics.median(ms[b]) / statistics.median(ms[a]):.1f} x the kernel"
    lines = [f"tetrahedral mesh extraction: scene_room({args.surfels}) rendered from room_cameras({args.views}, {args.width}, "
             f"{args.height}); spatial extent {extent:.4f}, trunc {trunc:.5f}; {torch.cuda.get_device_name(0)}; "
             f"{_lib.load().g4s_version().decode()}",
             f"{points.size(0)} tetra points (downsample {args.downsample}), {cells.size(0)} tets (scipy Delaunay on the host: "
             f"{host_s:.1f} s), {edges.size(0)} crossing edges, {faces.size(0)} triangles",
             f"HIP-event times in ms: median (min-max) of {args.rounds} rounds after one warm-up, kernel and torch formulation "
             "alternating; each torch formulation equals its kernel's output exactly (checked first)",
             "the kernel rows time the public calls of g4splat_amd.mesh, not the launches alone: each includes building the "
             "view table on the host, its staging copy and stream synchronisation, the workspace and output allocations, and "
             "for the marching tetrahedra the min/max index check and the host's two reads of the counts", "",
             f"  point TSDF (g4s_atsdf_sample, {args.views} views)          {fmt(ms['tsdf'])}",
             f"  torch formulation                                 {fmt(ms['tsdf_torch'])}{ratio('tsdf', 'tsdf_torch')}",
             f"  marching tetrahedra (g4s_mtet_count + emit)       {fmt(ms['mtet'])}",
             f"  torch formulation (torch.unique)                  {fmt(ms['mtet_torch'])}{ratio('mtet', 'mtet_torch')}",
             f"  fused bisection, 8 steps (g4s_atsdf_bisect)       {fmt(ms['bisect'])}",
             f"  torch formulation, eight passes                   {fmt(ms['bisect_torch'])}{ratio('bisect', 'bisect_torch')}", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
