"""Times the visibility grid (g4splat_amd/visibility.py, csrc/tsdf/visibility.hip) beside the same contract written in plain
torch on the same GPU, in the reference's formulation:

    build   R = 256 over an 8 m box, 8 and 32 views of 512 x 512: the kernel (one thread per voxel, early exit, ballot)
            against guidance/cam_utils.py check_valid_camera_center_by_depth's shape -- all 16.7 M voxel centres in
            memory, one pass per view with nonzero, two gathers and a scatter, a float grid at the end;
    march   one 512 x 512 map: the kernel over the 2 MiB bit grid, the same kernel over a 16 MiB byte grid
            (g4s_visgrid_march_bytes: does the packing buy anything?), against guidance/vis_grid.py
            render_visibility_map's shape -- every sample of every ray materialised ([H W, S - 10, 3], in row chunks of at
            most --chunk-mb), looked up in the float grid, reduced with any().

Every figure is the median of --runs runs after --warmup warm-ups, the device synchronised before each clock reading;
peak memory is torch's allocator's (the library allocates through it).  The torch results are compared with the
kernels' first and the number of differing elements is printed: torch contracts multiply-adds, so single edge decisions
may differ.  DESIGN.md ("Visibility grid") holds the numbers with the library's build id.

    python tools/bench_visibility.py [--runs 20] [--warmup 5] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g4splat_amd import _lib, synthetic, visibility  # noqa: E402
from g4splat_amd._device import host_f32  # noqa: E402

DEV = torch.device("cuda:0")
R, SIZE = 256, 512
LO, HI = (-4.0, -4.0, -4.0), (4.0, 4.0, 4.0)


def sphere_depth(cam, W, H, radius, background):
    """Depth map of the sphere of `radius` about the origin along the rays of the contract's ray record."""
    rec = torch.as_tensor(visibility.ray_record(cam, W, H), dtype=torch.float64)
    o, D = rec[:3], rec[3:].reshape(3, 3)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    dirs = torch.stack([x.reshape(-1), y.reshape(-1), torch.ones(H * W, dtype=torch.float64)], 1) @ D.T
    a, b, c = (dirs * dirs).sum(1), 2.0 * (dirs @ o), float(o @ o) - radius * radius
    disc = b * b - 4.0 * a * c
    t = (-b - disc.clamp_min(0).sqrt()) / (2.0 * a)
    return torch.where((disc > 0) & (t > 0), t, torch.full_like(t, background)).float().reshape(H, W).to(DEV)


def make_views(n):
    cams = []
    for i in range(n):
        a, z = 2.0 * math.pi * i * 0.381966, -2.0 + 4.0 * (i + 0.5) / n
        cams.append(synthetic.look_at_camera((3.2 * math.cos(a), 3.2 * math.sin(a), z), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0),
                                             math.radians(70.0), SIZE, SIZE))
    return cams, [sphere_depth(c, SIZE, SIZE, 1.0, 9.0) for c in cams]


# ---- the contract in plain torch, the reference's formulation ------------------------------------------------------------
def torch_project(cam, W, H, pts):
    M = torch.as_tensor(np.asarray(cam.world_view_transform, np.float32), device=DEV)
    fx = W / (2.0 * math.tan(cam.FoVx / 2.0))
    fy = H / (2.0 * math.tan(cam.FoVy / 2.0))
    c = [((pts[:, 0] * M[0, j] + pts[:, 1] * M[1, j]) + pts[:, 2] * M[2, j]) + M[3, j] for j in range(3)]
    u = c[0] / c[2] * fx + W / 2
    v = c[1] / c[2] * fy + H / 2
    return c[2], u, v, (u >= 0) & (u < W) & (v >= 0) & (v < H)


def torch_grid_centers(lo, hi):
    cell = (hi - lo) / R
    i = torch.arange(R, device=DEV)
    X, Y, Z = torch.meshgrid(i, i, i, indexing="ij")
    return torch.stack([lo[0] + (X + 0.5) * cell[0], lo[1] + (Y + 0.5) * cell[1], lo[2] + (Z + 0.5) * cell[2]], -1).reshape(-1, 3)


def torch_build(lo, hi, cams, depths):
    pts = torch_grid_centers(lo, hi)
    valid = torch.zeros(pts.shape[0], dtype=torch.bool, device=DEV)
    for cam, depth in zip(cams, depths):
        H, W = depth.shape
        z, u, v, inside = torch_project(cam, W, H, pts)
        if not torch.any(inside):
            continue
        ui = torch.clamp(u[inside].long(), 0, W - 1)
        vi = torch.clamp(v[inside].long(), 0, H - 1)
        zi = z[inside]
        ok = (zi < depth[vi, ui]) & (zi > 0)
        valid[torch.nonzero(inside).squeeze(-1)[ok]] = True
    grid = torch.zeros((R, R, R), dtype=torch.float32, device=DEV)
    grid[valid.reshape(R, R, R)] = 1.0
    return grid


def torch_march(lo, hi, grid, cam, depth, S, chunk_mb):
    H, W = depth.shape
    rec = torch.as_tensor(visibility.ray_record(cam, W, H), device=DEV)
    o, D = rec[:3], rec[3:].reshape(3, 3)
    invalid = depth <= 1e-6
    d = torch.where(invalid, torch.full_like(depth, 1e-3), depth)
    t = torch.linspace(0, 1, S, device=DEV)[: max(S - 10, 0)]
    rows = max(1, min(H, int(chunk_mb * 2 ** 20 / (W * max(len(t), 1) * 12))))
    out = torch.empty((H, W), dtype=torch.float32, device=DEV)
    x = torch.arange(W, device=DEV).float()
    for r0 in range(0, H, rows):
        r1 = min(H, r0 + rows)
        yy, xx = torch.meshgrid(torch.arange(r0, r1, device=DEV).float(), x, indexing="ij")
        xx, yy = xx.reshape(-1), yy.reshape(-1)
        dirs = torch.stack([(D[r, 0] * xx + D[r, 1] * yy) + D[r, 2] for r in range(3)], 1)      # [n,3]
        tv = t.reshape(1, -1, 1) * d[r0:r1].reshape(-1, 1, 1)                                   # [n,S-10,1]
        pts = (o.reshape(1, 1, 3) + tv * dirs[:, None, :]).reshape(-1, 3)
        idx = torch.clamp((pts - lo) / (hi - lo) * R, 0, R - 1).int()
        vals = grid[idx[:, 0], idx[:, 1], idx[:, 2]].reshape(-1, len(t))
        out[r0:r1] = (1 - (vals < 0.5).any(-1).float()).reshape(r1 - r0, W)
    out[invalid] = 0.0
    return out


# ---- timing --------------------------------------------------------------------------------------------------------------
def measure(fn, runs, warmup):
    """(median ms, peak MiB above what was allocated before, last result)."""
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize(DEV)
    base = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    times = []
    for _ in range(runs):
        torch.cuda.synchronize(DEV)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(DEV)
        times.append((time.perf_counter() - t0) * 1e3)
    peak = (torch.cuda.max_memory_allocated(DEV) - base) / 2 ** 20
    return statistics.median(times), peak, out


def march_raw(entry, grid, storage, cam, depth, S):
    """One march call on the given storage of the grid (the packed words or one byte per voxel), S given."""
    H, W = depth.shape
    out = torch.empty((H, W), dtype=torch.float32, device=DEV)
    _lib.call(entry, R, grid._lo, grid._hi, _lib.ptr(storage), W, H, _lib.ptr(depth), host_f32(visibility.ray_record(cam, W, H)),
              S, _lib.ptr(out), None, 0, _lib.stream(DEV))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chunk-mb", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lo, hi = torch.tensor(LO, device=DEV), torch.tensor(HI, device=DEV)
    rows, result = [], {"build_id": _lib.load().g4s_version().decode(), "device": torch.cuda.get_device_name(DEV),
                        "runs": a.runs, "warmup": a.warmup}
    grid32 = None
    for n in (8, 32):
        cams, depths = make_views(n)
        ms, mib, grid = measure(lambda: visibility.VisibilityGrid(lo, hi, R, cams, depths), a.runs, a.warmup)
        tms, tmib, tgrid = measure(lambda: torch_build(lo, hi, cams, depths), a.runs, a.warmup)
        differ = int((grid.visibility_grid != tgrid).sum())
        visible = float(grid.visibility_grid.mean())
        rows.append(f"build R={R} {n:2d} views {SIZE}x{SIZE}: kernel {ms:8.3f} ms {mib:8.1f} MiB | torch {tms:9.3f} ms {tmib:8.1f} MiB"
                    f" | x{tms / ms:.1f} | visible {visible:.3f}, {differ} voxels differ")
        result[f"build_{n}"] = {"kernel_ms": ms, "kernel_mib": mib, "torch_ms": tms, "torch_mib": tmib, "differ": differ}
        grid32 = grid
        del tgrid
    # one march from a novel camera between the inputs
    cam = synthetic.look_at_camera((2.5, 0.6, 0.4), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), math.radians(60.0), SIZE, SIZE)
    depth = sphere_depth(cam, SIZE, SIZE, 1.0, 7.0)
    S = grid32.n_samples(depth)
    dense = grid32.visibility_grid
    bytes_grid = (dense > 0.5).to(torch.uint8).contiguous()
    ms, mib, vmap = measure(lambda: grid32.render_visibility_map([cam], [depth])[0], a.runs, a.warmup)
    bms, bmib, bmap = measure(lambda: march_raw("g4s_visgrid_march_bytes", grid32, bytes_grid, cam, depth, S), a.runs, a.warmup)
    tms, tmib, tmap = measure(lambda: torch_march(lo, hi, dense, cam, depth, S, a.chunk_mb), a.runs, a.warmup)
    assert torch.equal(vmap, bmap), "the byte grid must give the bit grid's map"
    differ = int((vmap != tmap).sum())
    rows.append(f"march {SIZE}x{SIZE}, S = {S}: bit grid {ms:8.3f} ms {mib:8.1f} MiB (incl. the sample count's read-back) | byte grid "
                f"{bms:8.3f} ms | torch {tms:9.3f} ms {tmib:8.1f} MiB | x{tms / ms:.1f} | ones {float(vmap.mean()):.3f}, "
                f"{differ} pixels differ")
    # the kernel alone, without the .max().item() of the sample count
    kms, _m, _o = measure(lambda: march_raw("g4s_visgrid_march", grid32, grid32.words, cam, depth, S), a.runs, a.warmup)
    rows.append(f"march kernel alone: bit grid {kms:8.3f} ms | byte grid {bms:8.3f} ms")
    result["march"] = {"S": S, "bit_ms": ms, "bit_kernel_ms": kms, "byte_kernel_ms": bms, "bit_mib": mib, "torch_ms": tms,
                       "torch_mib": tmib, "differ": differ}
    text = "\n".join([f"{result['build_id']} on {result['device']}; median of {a.runs} after {a.warmup} warm-ups"] + rows)
    print(text)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
