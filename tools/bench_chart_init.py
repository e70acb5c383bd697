"""Times the Gaussian initialisation from depth charts (g4splat_amd/chart_init.py, csrc/tsdf/chart_init.hip) beside the same
contract written in plain torch on the same GPU, at the stage's own size: the trainer's cap of
--views input views (50) of 800 x 600 plus --extra inpainted views (30) of 512 x 512.

    surfels  initial_gaussians without the cap: per group of views two launches and a scan, the points formed in the kernels;
             against the same contract in whole-tensor torch: the back-projection as a matmul, the gathered vertices of all
             faces, the sides, altitudes and their ratio, the boolean gather of the kept faces, the two axes, the
             orthogonalisation and the quaternion table, every step a tensor of n_faces rows;
    pick     voxel_downsample_gaussians over the result at --voxel (0.01): the voxel sort and one launch; it has no torch side
             (the reference goes through open3d on the host), so it is timed alone.

The torch version is written here; it is neither the code under test nor the reference's files.  Its sums are torch's and
its rays come out of matmuls, so its floats are not the contract's bit for bit: what is checked before anything is timed is
that the two sides keep the same number of faces up to --decisions (1e-5) of all faces and that, over the first three views of
each group taken singly and fed the library's own back-projected points, wherever the numbers are equal, every output agrees
to --rtol (1e-4) of the output's largest magnitude (rotations as matrices; scales and rotations over the rows whose two
axis lengths differ by more than 1e-3 of the longer, since which axis comes first is a decision as well).  Timing: --warmup warm-up rounds, then --rounds rounds that alternate the two sides, the device synchronised before each clock reading; medians; peak
memory is torch's allocator's above what the inputs hold (the library allocates through it).

    python tools/bench_chart_init.py [--rounds 5] [--warmup 2] [--out FILE]
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
from g4splat_amd import _lib, chart_init, synthetic, visibility  # noqa: E402

DEV = torch.device("cuda:0")


def make_group(n, W, H, seed):
    """n cameras around the origin, smooth depths of 2 .. 4.5 with a few depth steps (elongated faces), random images."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    cams, depths, images = [], [], []
    for v in range(n):
        a, z = 2.0 * math.pi * v * 0.381966, -1.0 + 2.0 * (v + 0.5) / max(n, 1)
        cams.append(synthetic.look_at_camera((3.5 * math.cos(a), 3.5 * math.sin(a), z), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0),
                                             math.radians(55.0), W, H))
        coarse = torch.rand((1, 1, 7, 9), generator=g)
        d = 2.0 + 2.5 * torch.nn.functional.interpolate(coarse, (H, W), mode="bicubic", align_corners=True)[0, 0].clamp(0, 1)
        steps = torch.nn.functional.interpolate(torch.rand((1, 1, 5, 6), generator=g), (H, W), mode="nearest")[0, 0]
        depths.append((d + 0.6 * (steps > 0.5)).to(DEV).contiguous())
        images.append(torch.rand((H, W, 3), generator=g).to(DEV).contiguous())
    return cams, depths, images


# ---- the contract in plain torch -------------------------------------------------------------------------------------------
def torch_points(cam, depth):
    H, W = depth.shape
    wvt = torch.as_tensor(np.asarray(cam.world_view_transform, np.float32), device=DEV)
    full = torch.as_tensor(np.asarray(cam.full_proj_transform, np.float32), device=DEV)
    c2w = wvt.T.inverse()
    ndc2pix = torch.tensor([[W / 2, 0, 0, W / 2], [0, H / 2, 0, H / 2], [0, 0, 0, 1]], device=DEV).float().T
    intr = ((c2w.T @ full) @ ndc2pix)[:3, :3].T
    gx, gy = torch.meshgrid(torch.arange(W, device=DEV).float(), torch.arange(H, device=DEV).float(), indexing="xy")
    pix = torch.stack([gx, gy, torch.ones_like(gx)], dim=-1).reshape(-1, 3)
    rays = pix @ intr.inverse().T @ c2w[:3, :3].T
    return depth.reshape(-1, 1) * rays + c2w[:3, 3]


def _dot(a, b):
    return (a * b).sum(dim=-1, keepdim=True)


def _unit(a):
    return a / a.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def torch_quaternions(x0, x1, n):
    """The contract's table on the columns (x0, x1, n) of the rotation."""
    m00, m10, m20 = x0.unbind(-1)
    m01, m11, m21 = x1.unbind(-1)
    m02, m12, m22 = n.unbind(-1)
    t = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], dim=-1)
    q_abs = torch.sqrt(t.clamp_min(0.0))
    a, b, c, d, e, f = m21 - m12, m02 - m20, m10 - m01, m10 + m01, m02 + m20, m12 + m21
    sq = q_abs ** 2
    rows = torch.stack([torch.stack([sq[:, 0], a, b, c], dim=-1), torch.stack([a, sq[:, 1], d, e], dim=-1),
                        torch.stack([b, d, sq[:, 2], f], dim=-1), torch.stack([c, e, f, sq[:, 3]], dim=-1)], dim=1)
    best = q_abs.argmax(dim=-1)
    q = rows[torch.arange(len(best), device=DEV), best] / (2.0 * q_abs.gather(1, best[:, None]).clamp_min(0.1))
    return torch.where(q[:, :1] < 0, -q, q)


def torch_surfels(cams, depths, images, ratio_th=5.0, normalized_scales=0.5, normal_scale=1e-10, points=None):
    """The contract in whole-tensor torch: every step materialises its [n_faces,3] (or [n_faces,3,3]) result.  points: the
    vertices [H*W,3] per view, in place of this side's own back-projection (the row-by-row check)."""
    H, W = depths[0].shape
    verts = torch.cat([torch_points(c, d) for c, d in zip(cams, depths)] if points is None else points)
    cols = torch.cat([i.reshape(-1, 3).clamp(0, 1) for i in images])
    cell = torch.arange(H * W, device=DEV).reshape(H, W)[:-1, :-1].reshape(-1)
    view = torch.cat([torch.stack([cell, cell + W, cell + 1], dim=1), torch.stack([cell + W + 1, cell + 1, cell + W], dim=1)])
    faces = torch.cat([view + v * H * W for v in range(len(cams))])
    A, B, C = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    s = (C - A, A - B, B - C)
    n = [_unit(x) for x in s]
    lengths = torch.cat([(s[i] - _dot(s[i], n[(i + 1) % 3]) * n[i]).norm(dim=-1, keepdim=True) for i in range(3)], dim=1)
    keep = lengths.max(dim=1).values / lengths.min(dim=1).values < ratio_th
    del A, B, C, s, n, lengths
    faces = faces[keep]
    A, B, C = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    third = 1.0 / 3.0
    means = (third * A + third * B) + third * C
    colors = (third * cols[faces[:, 0]] + third * cols[faces[:, 1]]) + third * cols[faces[:, 2]]
    r2, r6 = math.sqrt(2.0) / 2.0, 1.0 / math.sqrt(6.0)
    t0, t1 = r2 * (B - A), (2.0 * r6) * C - r6 * (A + B)
    l0, l1 = t0.norm(dim=-1, keepdim=True), t1.norm(dim=-1, keepdim=True)
    first0 = l0 >= l1
    u, w = torch.where(first0, t0, t1), torch.where(first0, t1, t0)
    w = w - _dot(w, u) * u / _dot(u, u)
    o0, o1 = torch.where(first0, u, w), torch.where(first0, w, u)
    scales = torch.cat([(o0 * normalized_scales).norm(dim=-1, keepdim=True), (o1 * normalized_scales).norm(dim=-1, keepdim=True),
                        torch.full_like(o0[:, :1], normal_scale)], dim=1)
    x0, x1 = _unit(o0), _unit(o1)
    return {"means": means, "scales": scales, "quaternions": torch_quaternions(x0, x1, torch.linalg.cross(x0, x1)), "colors": colors,
            "axis_margin": ((l0 - l1).abs() / torch.maximum(l0, l1))[:, 0]}


def torch_initial(groups):
    parts = [torch_surfels(*g) for g in groups if g[0]]
    p = {k: torch.cat([x[k] for x in parts]) for k in ("means", "scales", "quaternions", "colors")}
    return p["means"], p["scales"][:, :2] * 1.0, p["quaternions"], p["colors"]


def rotations(q):
    r, i, j, k = q.double().unbind(-1)
    s = 2.0 / (q.double() ** 2).sum(-1)
    return torch.stack([1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r), s * (i * j + k * r), 1 - s * (i * i + k * k),
                        s * (j * k - i * r), s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)], dim=-1)


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
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rtol", type=float, default=1e-4)
    ap.add_argument("--decisions", type=float, default=1e-5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    inputs, extra = make_group(a.views, 800, 600, 17), make_group(a.extra, 512, 512, 18)
    n_faces = 2 * (a.views * 799 * 599 + a.extra * 511 * 511)
    result = {"build_id": _lib.load().g4s_version().decode(), "device": torch.cuda.get_device_name(DEV), "rounds": a.rounds,
              "warmup": a.warmup, "views": a.views, "extra_views": a.extra, "faces": n_faces}

    hip = lambda: chart_init.initial_gaussians(inputs[1], inputs[0], inputs[2], extra[1] or None, extra[0], extra[2])  # noqa: E731
    plain = lambda: torch_initial([inputs, extra])  # noqa: E731
    got, want = hip(), plain()
    kept, kept_torch = got[0].shape[0], want[0].shape[0]
    assert abs(kept - kept_torch) <= a.decisions * n_faces, (kept, kept_torch)
    # Row by row over single views, both sides on the SAME vertices (the library's back-projection): the sides of a face are
    # differences of points a pixel apart, so the last bits of a matmul back-projection move a ratio by 1e-4 of its value and
    # thousands of the 6 x 10^7 faces fall the other way, each shifting every later row.  On shared vertices only torch's own
    # association of its sums is left, and rows are compared on the views where both sides keep the same number of faces.
    # Which axis opens the orthogonalisation is a decision too (|t0| >= |t1|).  The axes are differences of coordinates of a
    # few units a pixel (a few thousandths) apart, known to a few 1e-5 of their length: rows where the two lengths are within
    # 1e-3 of each other are left out of the scale and rotation comparison, and counted.
    diffs, compared, ties, rows_compared = {}, 0, 0, 0
    singles = [(g[0][v:v + 1], g[1][v:v + 1], g[2][v:v + 1]) for g in (inputs, extra) for v in range(min(3, len(g[0])))]
    for cams, depths, images in singles:
        one = chart_init.initial_gaussians(depths, cams, images)
        shared = torch_surfels(cams, depths, images, points=[visibility.depths_to_points(d, c) for d, c in zip(depths, cams)])
        ref = (shared["means"], shared["scales"][:, :2], shared["quaternions"], shared["colors"])
        if one[0].shape[0] != ref[0].shape[0]:
            continue
        compared += 1
        clear = shared["axis_margin"] > 1e-3
        ties += int((~clear).sum())
        rows_compared += len(clear)
        for name, g, w in zip(("means", "scales", "rotations", "colors"), one, ref):
            if name == "rotations":
                g, w = rotations(g), rotations(w)
            if name in ("scales", "rotations"):
                g, w = g[clear], w[clear]
            err = (g - w).abs().reshape(len(g), -1).max(dim=1).values / w.abs().max()
            if float(err.max()) > a.rtol:  # say which row before the assertion below fails
                r = int(err.argmax())
                print(f"{name}: row {r} of {len(g)} differs by {float(err.max()):.3e}; {int((err > a.rtol).sum())} rows beyond rtol; axis margin "
                      f"{float(shared['axis_margin'][clear][r] if name in ('scales', 'rotations') else shared['axis_margin'][r]):.3e}; "
                      f"got {g[r].tolist()} want {w[r].tolist()}")
            diffs[name] = max(diffs.get(name, 0.0), float(err.max()))
    assert ties <= 1e-2 * max(rows_compared, 1), (ties, rows_compared)
    assert compared == 0 or max(diffs.values()) <= a.rtol, (compared, diffs)
    del want
    t = alternate({"hip": hip, "torch": plain}, a.rounds, a.warmup)
    rows = [f"surfels {a.views} + {a.extra} views, {n_faces} faces, {kept} kept: HIP {t['hip'][0]:9.3f} ms ({t['hip'][1]:.3f} .. "
            f"{t['hip'][2]:.3f}) {t['hip'][3]:8.1f} MiB | torch {t['torch'][0]:9.3f} ms ({t['torch'][1]:.3f} .. {t['torch'][2]:.3f}) "
            f"{t['torch'][3]:8.1f} MiB | x{t['torch'][0] / t['hip'][0]:.1f} | torch keeps {kept_torch}; "
            f"largest relative difference over {compared} of {len(singles)} single views ({rows_compared} rows, {ties} with tied axes left "
            f"out of scales and rotations): " + ", ".join(f"{k} {v:.1e}" for k, v in diffs.items())]
    result["surfels"] = {"hip_ms": t["hip"][0], "hip_mib": t["hip"][3], "torch_ms": t["torch"][0], "torch_mib": t["torch"][3],
                         "kept": kept, "kept_torch": kept_torch, "views_compared": compared, "rows_compared": rows_compared, "tied_axes": ties, "differences": diffs}

    params = {"means": got[0]}
    idx, factor = chart_init.voxel_downsample_gaussians(params, a.voxel)
    t = alternate({"hip": lambda: chart_init.voxel_downsample_gaussians(params, a.voxel)}, a.rounds, a.warmup)
    rows.append(f"pick    {kept} surfels at voxel {a.voxel:g}: HIP {t['hip'][0]:9.3f} ms ({t['hip'][1]:.3f} .. {t['hip'][2]:.3f}) "
                f"{t['hip'][3]:8.1f} MiB | {len(idx)} voxels, factor {factor:.3f}")
    result["pick"] = {"hip_ms": t["hip"][0], "hip_mib": t["hip"][3], "voxels": len(idx), "factor": factor}
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
