"""Times the warp initialiser (g4splat_amd/warp_init.py, csrc/tsdf/warp_init.hip) beside the same contract written in plain
torch on the same GPU, at the stage's usual size: --views input views (50) of 800 x 600 plus --extra inpainted views (30) of
512 x 512, all in one ordered stack, for the grids -1 and 2.

Scene: synthetic overlapping views, a height field z = 2.1 + 0.3 sin(2.6 x) cos(2.2 y) seen from nearby poses (the depth of
every pixel by a fixed-point iteration on the device), with --noise (0.6 %) uniform relative depth noise so that a later view
is explained in part only, and random images.

The torch side is written here from the contract (include/g4s_render_maps.h, "Warp surfels"): the double loop over (view,
earlier view), every turn with whole-image temporaries -- the projection, the closed-border mask, the rounded gather, the
depth test --, then the distance map, the normal map, the quaternion and the boolean gathers.  It is neither the code under
test nor the reference's files.  Its floats follow torch's kernels, so a pixel within rounding of a threshold may fall the other
way: before anything is timed the two sides' numbers of rows are compared to --decisions (1e-3) of all lattice pixels, and
both are reported.  Timing: --warmup warm-up rounds, then --rounds rounds that alternate the two sides, the device synchronised
before each clock reading; medians; peak memory is torch's allocator's above what the inputs hold.

    python tools/bench_warp_init.py [--rounds 5] [--warmup 2] [--out FILE]
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
from g4splat_amd import _lib, synthetic, warp_init  # noqa: E402
from g4splat_amd.visibility import ray_record  # noqa: E402

DEV = torch.device("cuda:0")


def height(x, y):
    return 2.1 + 0.3 * torch.sin(2.6 * x) * torch.cos(2.2 * y)


def make_views(n, W, H, seed, noise):
    """n cameras within 0.3 of the origin looking down +z with a small yaw, their depths of the height field, random images."""
    rng = np.random.default_rng(seed)
    g = torch.Generator(device="cpu").manual_seed(seed)
    cams, depths, images = [], [], []
    for _ in range(n):
        eye, yaw = rng.uniform(-0.3, 0.3, 3) * (1.0, 1.0, 0.3), rng.uniform(-0.08, 0.08)
        c, s = math.cos(yaw), math.sin(yaw)
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        fovx = math.radians(60.0)
        cam = synthetic.make_camera(R, -R.T @ eye, fovx, 2.0 * math.atan(math.tan(fovx / 2) * H / W), W, H)
        ray = torch.as_tensor(ray_record(cam, W, H), dtype=torch.float64, device=DEV)
        o, D = ray[:3], ray[3:].reshape(3, 3)
        y, x = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float64), torch.arange(W, device=DEV, dtype=torch.float64), indexing="ij")
        dirs = torch.stack([D[r, 0] * x + D[r, 1] * y + D[r, 2] for r in range(3)], -1)
        d = torch.full((H, W), 2.1, dtype=torch.float64, device=DEV)
        for _it in range(40):  # a contraction: |grad height| tan(FoV / 2) < 1
            d = (height(o[0] + d * dirs[..., 0], o[1] + d * dirs[..., 1]) - o[2]) / dirs[..., 2]
        d = d * (1.0 + noise * (2.0 * torch.rand((H, W), generator=g, dtype=torch.float64).to(DEV) - 1.0))
        cams.append(cam), depths.append(d.float().contiguous()), images.append(torch.rand((3, H, W), generator=g).to(DEV).contiguous())
    return cams, depths, images


# ---- the contract in plain torch -------------------------------------------------------------------------------------------
def _unit(a):
    return a / a.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def torch_points(ray, depth):
    H, W = depth.shape
    o, D = ray[:3], ray[3:].reshape(3, 3)
    y, x = torch.meshgrid(torch.arange(H, device=DEV).float(), torch.arange(W, device=DEV).float(), indexing="ij")
    return torch.stack([o[r] + depth * ((D[r, 0] * x + D[r, 1] * y) + D[r, 2]) for r in range(3)], -1)


def torch_covered(P, wvt, fx, fy, depth, thresh):
    H, W = depth.shape
    c = [((P[..., 0] * wvt[0, j] + P[..., 1] * wvt[1, j]) + P[..., 2] * wvt[2, j]) + wvt[3, j] for j in range(3)]
    z = c[2]
    u, v = (c[0] / z) * fx + W * 0.5, (c[1] / z) * fy + H * 0.5
    inside = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1) & (z > 0)
    ui, vi = torch.round(u).nan_to_num(0).long().clamp(0, W - 1), torch.round(v).nan_to_num(0).long().clamp(0, H - 1)
    d = depth[vi, ui]
    return inside & (d > 0) & ((z - d).abs() / (z + 1e-6) < thresh)


def torch_quaternions(n):
    z = _unit(n)
    ref = torch.zeros_like(z)
    par = z[:, 0].abs() > 0.9
    ref[:, 0], ref[:, 1] = (~par).float(), par.float()
    x = _unit(torch.linalg.cross(ref, z))
    y = torch.linalg.cross(z, x)
    m00, m11, m22 = x[:, 0], y[:, 1], z[:, 2]
    q = torch.stack([(1 + m00 + m11 + m22).clamp_min(0).sqrt() / 2,
                     (1 + m00 - m11 - m22).clamp_min(0).sqrt() / 2 * torch.sign(y[:, 2] - z[:, 1] + 1e-12),
                     (1 - m00 + m11 - m22).clamp_min(0).sqrt() / 2 * torch.sign(z[:, 0] - x[:, 2] + 1e-12),
                     (1 - m00 - m11 + m22).clamp_min(0).sqrt() / 2 * torch.sign(x[:, 1] - y[:, 0] + 1e-12)], -1)
    return _unit(q)


def torch_surfels(cams, depths, images, thresh=0.01, min_scale=0.0005, max_scale=0.05, g=-1):
    rays = [torch.as_tensor(ray_record(c, d.shape[1], d.shape[0]), device=DEV) for c, d in zip(cams, depths)]
    wvts = [torch.as_tensor(np.asarray(c.world_view_transform, np.float32), device=DEV) for c in cams]
    focal = [(d.shape[1] / (2.0 * math.tan(c.FoVx / 2.0)), d.shape[0] / (2.0 * math.tan(c.FoVy / 2.0))) for c, d in zip(cams, depths)]
    out = [[], [], [], []]
    for i, depth in enumerate(depths):
        H, W = depth.shape
        P = torch_points(rays[i], depth)
        keep = depth > 0
        if g > 0:
            lattice = torch.zeros_like(keep)
            lattice[::g, ::g] = True
            keep &= lattice
        for j in range(i):
            keep &= ~torch_covered(P, wvts[j], focal[j][0], focal[j][1], depths[j], thresh)
        dh, dv = (P[:, 1:] - P[:, :-1]).norm(dim=-1), (P[1:] - P[:-1]).norm(dim=-1)
        s = torch.stack([torch.cat([dh, dh[:, -1:]], 1), torch.cat([dh[:, :1], dh], 1), torch.cat([dv, dv[-1:]], 0),
                         torch.cat([dv[:1], dv], 0)]).min(dim=0).values * 0.5
        if g > 0:
            s = s * float(g)
        keep &= s < max_scale
        n = torch.zeros_like(P)
        n[1:-1, 1:-1] = _unit(torch.linalg.cross(P[2:, 1:-1] - P[:-2, 1:-1], P[1:-1, 2:] - P[1:-1, :-2]))
        n[0, 1:-1], n[-1, 1:-1] = n[1, 1:-1], n[-2, 1:-1]
        n[:, 0], n[:, -1] = n[:, 1], n[:, -2]
        out[0].append(P[keep])
        out[1].append(s[keep].clamp_min(min_scale)[:, None].repeat(1, 2))
        out[2].append(torch_quaternions(n[keep]))
        out[3].append(images[i].permute(1, 2, 0)[keep])
    return tuple(torch.cat(o) for o in out)


def alternate(sides, rounds, warmup):
    times, peaks = {n: [] for n in sides}, {n: 0.0 for n in sides}
    for r in range(warmup + rounds):
        for name, fn in sides.items():
            torch.cuda.synchronize(DEV)
            base = torch.cuda.memory_allocated(DEV)
            torch.cuda.reset_peak_memory_stats(DEV)
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize(DEV)
            ms = (time.perf_counter() - t0) * 1e3
            del out
            if r >= warmup:
                times[name].append(ms)
                peaks[name] = max(peaks[name], (torch.cuda.max_memory_allocated(DEV) - base) / 2 ** 20)
    return {n: (statistics.median(times[n]), min(times[n]), max(times[n]), peaks[n]) for n in sides}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--extra", type=int, default=30)
    ap.add_argument("--noise", type=float, default=0.006)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--decisions", type=float, default=1e-3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    groups = [make_views(a.views, 800, 600, 17, a.noise), make_views(a.extra, 512, 512, 18, a.noise)]
    cams, depths, images = (groups[0][k] + groups[1][k] for k in range(3))
    result = {"build_id": _lib.load().g4s_version().decode(), "device": torch.cuda.get_device_name(DEV), "rounds": a.rounds,
              "warmup": a.warmup, "views": a.views, "extra_views": a.extra}
    rows = []
    for g in (-1, 2):
        step = max(g, 1)
        cells = sum(-(-d.shape[0] // step) * -(-d.shape[1] // step) for d in depths)
        hip = lambda: warp_init.warp_surfels(depths, cams, images, downsample_pixel_grid_size=g)  # noqa: E731
        plain = lambda: torch_surfels(cams, depths, images, g=g)  # noqa: E731
        kept, kept_torch = hip()[0].shape[0], plain()[0].shape[0]
        assert abs(kept - kept_torch) <= a.decisions * cells, (g, kept, kept_torch, cells)
        t = alternate({"hip": hip, "torch": plain}, a.rounds, a.warmup)
        rows.append(f"grid {g:2d}: {len(depths)} views, {cells} lattice pixels, {kept} rows: HIP {t['hip'][0]:9.3f} ms ({t['hip'][1]:.3f} .. "
                    f"{t['hip'][2]:.3f}) {t['hip'][3]:8.1f} MiB | torch {t['torch'][0]:9.3f} ms ({t['torch'][1]:.3f} .. {t['torch'][2]:.3f}) "
                    f"{t['torch'][3]:8.1f} MiB | x{t['torch'][0] / t['hip'][0]:.1f} | torch keeps {kept_torch}")
        result[f"grid_{g}"] = {"hip_ms": t["hip"][0], "hip_mib": t["hip"][3], "torch_ms": t["torch"][0], "torch_mib": t["torch"][3],
                               "lattice_pixels": cells, "rows": kept, "rows_torch": kept_torch}
    text = "\n".join([f"{result['build_id']} on {result['device']}; medians (min .. max) of {a.rounds} alternating rounds after "
                      f"{a.warmup} warm-ups"] + rows)
    print(text)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
