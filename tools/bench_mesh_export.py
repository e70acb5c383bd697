"""Time every stage of the multi-resolution mesh export on the synthetic room, on the GPU and -- the same stage on the same
arrays -- in numpy / scipy on the host.

    python tools/bench_mesh_export.py [--mesh-res 768] [--repeat 5] [--out profiles/mesh_export.json]

The room is 6 x 4 x 3 m and the cameras stand 0.72 m from its centre, so the reference's factors (2, 8, 16) would give an
empty first level and a third one that is culled entirely; the default factors (3, 5, 20) truncate at 2.2, 3.6 and 14.4 m,
inside the room, so that every level contributes and the cull removes a part of the second and third.

Stages (render_multires.py:129-206 of the reference): one bounded TSDF extraction per factor, the observed-face cull of
every level after the first, the join, the clustering, post_process_mesh (clustering + two compactions) and filter_mesh.
GPU figures: one warm-up call, then the median of --repeat calls, each bracketed by torch.cuda.synchronize().  Host
figures: one call (they take seconds): the cull in numpy (one camera at a time, so no [C,V] array), the clustering with
scipy.sparse.csgraph.connected_components over the edge-sharing graph, compaction and the edge filter in numpy.  The
host results are compared with the GPU's before the table is printed (clusters as a partition).  The reference's own
path (pytorch3d + open3d) is not measured: neither runs on this stack.
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_ops_ref as ref  # noqa: E402
from g4splat_amd import _lib, mesh, synthetic  # noqa: E402
from g4splat_amd.gaussian_model import GaussianModel  # noqa: E402
from g4splat_amd.gaussian_renderer import render  # noqa: E402


def gpu_time(fn, repeat):
    fn()  # warm-up: allocator, code objects
    out, ms = None, []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return out, statistics.median(ms), min(ms), max(ms)


def host_time(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t0)


def scipy_clusters(tris):
    """(labels, sizes) of the header's definition through scipy: triangles that use the same undirected edge are chained."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    F = len(tris)
    a = np.concatenate([tris[:, 0], tris[:, 1], tris[:, 2]]).astype(np.int64)
    b = np.concatenate([tris[:, 1], tris[:, 2], tris[:, 0]]).astype(np.int64)
    owner = np.tile(np.arange(F, dtype=np.int64), 3)
    ok = a != b
    key = (np.minimum(a, b)[ok] << 32) | np.maximum(a, b)[ok]
    owner = owner[ok]
    order = np.argsort(key, kind="stable")
    key, owner = key[order], owner[order]
    same = key[1:] == key[:-1]
    g = coo_matrix((np.ones(int(same.sum()), np.int8), (owner[:-1][same], owner[1:][same])), shape=(F, F))
    _n, comp = connected_components(g, directed=False)
    first = np.full(comp.max() + 1, F, np.int64)
    np.minimum.at(first, comp, np.arange(F))
    labels = first[comp].astype(np.int32)
    return labels, np.bincount(labels, minlength=F)[labels].astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-res", type=int, default=768)
    ap.add_argument("--factors", type=float, nargs="+", default=[3.0, 5.0, 20.0])
    ap.add_argument("--surfels", type=int, default=400_000)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default="profiles/mesh_export.json")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sc = synthetic.scene_room(args.surfels, seed=4, scale_mean=0.03, scale_sigma=0.2)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    model = GaussianModel(sh_degree=3)
    model.create_from_parameters(t(sc.means3D), t(sc.scales), t(sc.rotations), t(np.full((len(sc.means3D), 3), 0.5, np.float32)))
    with torch.no_grad():
        model._opacity.fill_(float(np.log(0.97 / 0.03)))
    model.active_sh_degree = 0
    host_cams = synthetic.room_cameras(args.views, args.width, args.height)
    cams = [SimpleNamespace(image_width=c.image_width, image_height=c.image_height, FoVx=c.FoVx, FoVy=c.FoVy,
                            world_view_transform=t(c.world_view_transform), full_proj_transform=t(c.full_proj_transform),
                            camera_center=t(c.camera_center), znear=c.znear, zfar=c.zfar) for c in host_cams]
    pipe = SimpleNamespace(depth_ratio=1.0, compute_cov3D_python=False, convert_SHs_python=False)
    ex = mesh.GaussianExtractor(model, render, pipe)
    ex.reconstruction(cams)
    rows = []

    def row(stage, size, gpu, host_ms):
        rows.append({"stage": stage, "size": size, "gpu_ms_median": gpu[1], "gpu_ms_min": gpu[2], "gpu_ms_max": gpu[3],
                     "host_ms": host_ms})

    levels, truncs = [], []
    for f in args.factors:
        trunc = ex.radius * f
        voxel = trunc / args.mesh_res
        g = gpu_time(lambda: ex.extract_mesh_bounded(voxel_size=voxel, sdf_trunc=5 * voxel, depth_trunc=trunc, to_host=False),
                     args.repeat)
        ex.volume = None
        levels.append(g[0])
        truncs.append(trunc)
        row(f"extract factor {f:g} (fusion of {args.views} views + marching cubes)", f"{g[0].triangles.size(0)} triangles", g, None)
    culled = [levels[0]]
    for i in range(1, len(levels)):
        m = levels[i]
        g = gpu_time(lambda: mesh.observed_face_mask(m, cams, truncs[i - 1]), args.repeat)
        hm = None
        if not args.skip_host:
            hv, ht = m.vertices.cpu().numpy(), m.triangles.cpu().numpy()
            keep, hm = host_time(lambda: ref.keep_unobserved(ht, ref.observed_vertices(hv, host_cams, truncs[i - 1])))
            assert np.array_equal(g[0].cpu().numpy().astype(bool), keep)
        row(f"cull mask level {i} ({args.views} cameras)", f"{m.vertices.size(0)} vertices, {m.triangles.size(0)} triangles", g, hm)
        keep_dev = g[0]
        g = gpu_time(lambda: mesh.compact_mesh(m, keep_dev), args.repeat)
        hm = None
        if not args.skip_host:
            want, hm = host_time(lambda: ref.compact(tuple(a.cpu().numpy() for a in m), keep))
            assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(g[0], want))
        row(f"compact level {i}", f"{m.triangles.size(0)} -> {g[0].triangles.size(0)} triangles", g, hm)
        if g[0].triangles.size(0) > 0:
            culled.append(g[0])
    g = gpu_time(lambda: mesh.join_meshes(culled), args.repeat)
    joined = g[0]
    F = joined.triangles.size(0)
    hj = tuple(a.cpu().numpy() for a in joined)
    hm = None if args.skip_host else host_time(lambda: ref.join_meshes([tuple(a.cpu().numpy() for a in m) for m in culled]))[1]
    row("join (torch.cat)", f"{F} triangles", g, hm)
    g = gpu_time(lambda: mesh.cluster_connected_triangles(joined), args.repeat)
    hm = None
    if not args.skip_host:
        (hl, hs), hm = host_time(lambda: scipy_clusters(hj[2]))
        assert np.array_equal(g[0][0].cpu().numpy(), hl) and np.array_equal(g[0][1].cpu().numpy(), hs)
    n_clusters = int((g[0][0] == torch.arange(F, dtype=torch.int32, device=dev)).sum())
    row("cluster_connected_triangles", f"{F} triangles, {n_clusters} clusters", g, hm)
    g = gpu_time(lambda: mesh.post_process_mesh(joined, cluster_to_keep=1000), args.repeat)
    hm = None
    if not args.skip_host:
        def host_post():
            labels, sizes = scipy_clusters(hj[2])
            kept = ref.compact(hj, sizes >= ref.cluster_threshold(labels, sizes, 1000))
            tt = kept[2]
            return ref.compact(kept, (tt[:, 0] != tt[:, 1]) & (tt[:, 1] != tt[:, 2]) & (tt[:, 0] != tt[:, 2]), compact_vertices=False)
        want, hm = host_time(host_post)
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(g[0], want))
    row("post_process_mesh (cluster + 2 compactions)", f"{F} -> {g[0].triangles.size(0)} triangles", g, hm)
    thr = 3.0 * truncs[0] / args.mesh_res
    g = gpu_time(lambda: mesh.filter_mesh(joined, thr), args.repeat)
    hm = None
    if not args.skip_host:
        want, hm = host_time(lambda: ref.filter_mesh(hj, thr))
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(g[0], want))
    row("filter_mesh (edge filter + compaction)", f"{F} -> {g[0].triangles.size(0)} triangles", g, hm)

    res = {"scene": f"scene_room({args.surfels}), room_cameras({args.views}, {args.width}, {args.height})",
           "radius": ex.radius, "mesh_res": args.mesh_res, "factors": args.factors, "repeat": args.repeat,
           "device": torch.cuda.get_device_name(0), "build": _lib.load().g4s_version().decode(), "stages": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("| stage | size | GPU ms (median, min-max) | host numpy/scipy ms |")
    print("|---|---|---|---|")
    for r in rows:
        host = "-" if r["host_ms"] is None else f"{r['host_ms']:.0f}"
        print(f"| {r['stage']} | {r['size']} | {r['gpu_ms_median']:.2f} ({r['gpu_ms_min']:.2f}-{r['gpu_ms_max']:.2f}) | {host} |")


if __name__ == "__main__":
    main()
