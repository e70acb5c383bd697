"""Times the depth-cue stage (g4splat_amd/depth_cues.py, csrc/tsdf/depth_cues.hip) beside the same stage written in plain
torch on the same GPU, in the reference's formulation, at the stage's own size: --views input views (24) of 800 x 600 plus
--inpainted inpainted views (12) of 512 x 512, --planes fitted global planes (36), eight local planes per view (288
(plane, view) pairs):

    cues     view_geometry_cues over all views: 3 launches, against the loop body of guidance/see3d_dn_util.py per view
             (masked selects, five float32 sums and two .item() read-backs, the back-projection as a matmul, torch.cross,
             F.normalize, a masked assignment);
    refine   refine_depths_with_planes with return_points: 4 launches and one back-projection per view, against a
             full-image ray/plane intersection per (plane, view) pair with its two 4 x 4 inverses, the paste, the second
             alignment and the refill per inpainted view, and a matmul back-projection per view.

The torch version is written here; it is neither the code under test nor the reference's files.  Its sums are float32 in
torch's order and its rays come out of matmuls, so its floats are not the contract's bit for bit: what is checked before
anything is timed is that every decision is the same (visibility exactly; the validity of a plane intersection on all but
--decisions of the masked pixels, 0.1 %) and that every float output agrees to --rtol (1e-4) of the output's largest
magnitude, over the pixels whose decision is the same and whose plane depth is below 100 on both sides (a ray along its
plane).  The normals are differences of float32 points a pixel apart -- a few thousandths of a unit at a depth of a few
units, known to a few 1e-7 --, so the two sides' normals agree to --normal-tol (1e-3) only.  The differences found are printed.  Timing: --warmup warm-up rounds,
then --rounds rounds that alternate the two sides, the device synchronised before each clock reading; medians; peak memory
is torch's allocator's above what the inputs hold (the library allocates through it).

    python tools/bench_depth_cues.py [--rounds 7] [--warmup 2] [--out FILE]
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
from g4splat_amd import _lib, depth_cues, synthetic  # noqa: E402

DEV = torch.device("cuda:0")
IDS_PER_VIEW = 8


def make_scene(n_input, n_inpainted, n_planes):
    g = torch.Generator(device="cpu").manual_seed(17)
    cams, sizes = [], []
    V = n_input + n_inpainted
    for v in range(V):
        W, H = (800, 600) if v < n_input else (512, 512)
        a, z = 2.0 * math.pi * v * 0.381966, -1.0 + 2.0 * (v + 0.5) / V
        cams.append(synthetic.look_at_camera((3.5 * math.cos(a), 3.5 * math.sin(a), z), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0),
                                             math.radians(55.0), W, H))
        sizes.append((H, W))

    def smooth(H, W, lo, hi):
        coarse = torch.rand((1, 1, 7, 9), generator=g)
        return (lo + (hi - lo) * torch.nn.functional.interpolate(coarse, (H, W), mode="bicubic", align_corners=True)[0, 0]).clamp(lo, hi)
    depths = [smooth(H, W, 2.0, 4.5) for H, W in sizes]
    disps = [(1.6 / d + 0.05 + 0.03 * smooth(*d.shape, -1.0, 1.0)) for d in depths]
    alphas = [torch.where(smooth(*d.shape, 0.0, 1.0) > 0.35, 0.97, 0.4) for d in depths]
    confs = [smooth(*d.shape, 0.0, 1.0) > 0.4 for d in depths]
    # plane masks: a grid of blocks, every block one of the view's ids (arbitrary positive integers) or 0
    masks, gdict = [], {k: [] for k in range(n_planes + 1)}
    for v, (H, W) in enumerate(sizes):
        ids = [0] + [3 * (v * IDS_PER_VIEW + i) + 2 for i in range(IDS_PER_VIEW)]
        blocks = torch.randint(0, len(ids), (H // 50 + 1, W // 50 + 1), generator=g)
        m = torch.tensor(ids, dtype=torch.int32)[blocks].repeat_interleave(50, 0).repeat_interleave(50, 1)[:H, :W]
        masks.append(m.contiguous())
        for i, pid in enumerate(ids[1:]):
            gdict[(v * 5 + i * 7) % (n_planes + 1)].append((v, pid))  # key n_planes is never fitted
    planes = {}
    for k in range(n_planes):
        n = torch.randn(3, generator=g)
        planes[k] = ((n / n.norm()).numpy(), (0.4 * torch.randn(3, generator=g)).numpy())
    dev = lambda maps: [m.to(DEV).contiguous() for m in maps]  # noqa: E731
    monos = [1.0 / d for d in disps]
    return cams, dev(depths), dev(disps), dev(alphas), dev(confs), dev(masks), dev(monos), gdict, planes


# ---- the stage in plain torch, the reference's formulation --------------------------------------------------------------
class TorchCamera:
    def __init__(self, cam, H, W):
        self.wvt = torch.as_tensor(np.asarray(cam.world_view_transform, np.float32), device=DEV)
        self.full = torch.as_tensor(np.asarray(cam.full_proj_transform, np.float32), device=DEV)
        self.W, self.H = W, H
        self.fx = W / (2.0 * math.tan(cam.FoVx / 2.0))
        self.fy = H / (2.0 * math.tan(cam.FoVy / 2.0))


def torch_align(disp, depth, mask):
    t, d = 1.0 / depth[mask], disp[mask]
    w = torch.ones_like(t)
    num = torch.sum(w * t * d) - torch.sum(w * t) * torch.sum(w * d) / torch.sum(w)
    den = torch.sum(w * d ** 2) - torch.sum(w * d) ** 2 / torch.sum(w)
    beta = (num / den).item()
    alpha = (torch.sum(w * (t - beta * d)) / torch.sum(w)).item()
    return 1.0 / (alpha + beta * disp), alpha, beta


def torch_points(cam, depth):
    c2w = cam.wvt.T.inverse()
    ndc2pix = torch.tensor([[cam.W / 2, 0, 0, cam.W / 2], [0, cam.H / 2, 0, cam.H / 2], [0, 0, 0, 1]], device=DEV).float().T
    intr = ((c2w.T @ cam.full) @ ndc2pix)[:3, :3].T
    gx, gy = torch.meshgrid(torch.arange(cam.W, device=DEV).float(), torch.arange(cam.H, device=DEV).float(), indexing="xy")
    pix = torch.stack([gx, gy, torch.ones_like(gx)], dim=-1).reshape(-1, 3)
    rays = pix @ intr.inverse().T @ c2w[:3, :3].T
    return depth.reshape(-1, 1) * rays + c2w[:3, 3]


def torch_cues(tcams, disps, warps, alphas, threshold):
    out = []
    for cam, disp, warp, alpha_map in zip(tcams, disps, warps, alphas):
        visible = alpha_map > threshold
        aligned, alpha, beta = torch_align(disp, warp, visible)
        P = torch_points(cam, aligned).reshape(cam.H, cam.W, 3)
        normal = torch.zeros_like(P)
        dx = P[2:, 1:-1] - P[:-2, 1:-1]
        dy = P[1:-1, 2:] - P[1:-1, :-2]
        normal[1:-1, 1:-1] = torch.nn.functional.normalize(torch.cross(dx, dy, dim=-1), dim=-1)
        merged = aligned.clone()
        merged[visible] = warp[visible]
        out.append(dict(visibility=visible, mono_depth=1.0 / disp, aligned_depth=aligned, depth=merged, normal_world=normal,
                        normal_cam=normal @ cam.wvt[:3, :3], coeffs=(alpha, beta)))
    return out


def torch_plane_depth(normal, centre, cam):
    K = torch.tensor([[cam.fx, 0, cam.W / 2], [0, cam.fy, cam.H / 2], [0, 0, 1]], device=DEV).float()
    c2w = cam.wvt.inverse().T
    o = c2w[:3, 3]
    y, x = torch.meshgrid(torch.arange(cam.H, device=DEV), torch.arange(cam.W, device=DEV), indexing="ij")
    pix = torch.stack([x, y, torch.ones_like(x)], dim=-1).float()
    rays = torch.nn.functional.normalize(torch.matmul(torch.matmul(pix, torch.inverse(K).T), c2w[:3, :3].T), dim=-1)
    nd = torch.sum(normal.view(1, 1, 3) * rays, dim=-1)
    num = torch.sum(normal * (centre - o))
    nd = torch.clamp(torch.abs(nd), min=1e-8) * torch.sign(nd)
    t = num / nd
    hit = o.view(1, 1, 3) + t.unsqueeze(-1) * rays
    cam_pts = torch.matmul(torch.cat([hit, torch.ones_like(hit[..., :1])], dim=-1), torch.inverse(c2w).T)
    depth = cam_pts[..., 2]
    depth[~((t > 0) & (depth > 0))] = 0
    return depth


def torch_refine(tcams, depths, masks, confs, monos, gdict, planes_dev, n_input):
    depth_list = [d.clone() for d in depths]
    for key, pairs in gdict.items():
        if key not in planes_dev:
            continue
        normal, centre = planes_dev[key]
        for v, pid in pairs:
            aligned = torch_plane_depth(normal, centre, tcams[v])
            region = masks[v] == pid
            depth_list[v][region] = aligned[region]
    for v in range(n_input, len(tcams)):
        fitted, _a, _b = torch_align(1.0 / monos[v], depth_list[v], confs[v])
        replace = ~(masks[v] > 0.5) & ~confs[v]
        depth_list[v][replace] = fitted[replace]
    return depth_list, [torch_points(c, d) for c, d in zip(tcams, depth_list)]


# ---- comparison and timing ---------------------------------------------------------------------------------------------
def worst_relative(got, want, keep=None):
    """The largest |got - want| over all views, as a fraction of the output's largest magnitude."""
    worst, scale = 0.0, 0.0
    for v, (a, b) in enumerate(zip(got, want)):
        k = torch.ones_like(a, dtype=torch.bool) if keep is None else keep[v]
        if k.any():
            diff = (a - b).abs()[k]
            worst = math.inf if bool(diff.isnan().any()) else max(worst, float(diff.max()))
            scale = max(scale, float(b.abs()[k].max()))
    return worst / max(scale, 1e-30)


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
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--inpainted", type=int, default=12)
    ap.add_argument("--planes", type=int, default=36)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rtol", type=float, default=1e-4)
    ap.add_argument("--decisions", type=float, default=1e-3)
    ap.add_argument("--normal-tol", type=float, default=1e-3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cams, depths, disps, alphas, confs, masks, monos, gdict, planes = make_scene(a.views, a.inpainted, a.planes)
    V, n_input = len(cams), a.views
    tcams = [TorchCamera(c, *d.shape) for c, d in zip(cams, depths)]
    planes_dev = {k: (torch.as_tensor(n, device=DEV), torch.as_tensor(c, device=DEV)) for k, (n, c) in planes.items()}
    n_pairs = sum(len(p) for k, p in gdict.items() if k in planes)
    result = {"build_id": _lib.load().g4s_version().decode(), "device": torch.cuda.get_device_name(DEV), "rounds": a.rounds,
              "warmup": a.warmup, "views": V, "input_views": n_input, "pairs": n_pairs, "planes": a.planes,
              "pixels": sum(d.numel() for d in depths)}
    rows = []

    # ---- cues
    hip_cues = lambda: depth_cues.view_geometry_cues(cams, disps, depths, alphas, 0.9)  # noqa: E731
    plain_cues = lambda: torch_cues(tcams, disps, depths, alphas, 0.9)  # noqa: E731
    got, want = hip_cues(), plain_cues()
    assert all(torch.equal(g, w["visibility"]) for g, w in zip(got.visibility, want)), "visibility differs"
    diffs = {"coeffs": worst_relative([got.coeffs.cpu()], [torch.tensor([w["coeffs"] for w in want])])}
    for name in ("mono_depth", "aligned_depth", "depth", "normal_world", "normal_cam"):
        diffs[name] = worst_relative(getattr(got, name), [w[name] for w in want])
    assert all(v <= (a.normal_tol if k.startswith("normal") else a.rtol) for k, v in diffs.items()), diffs
    del got, want
    t = alternate({"hip": hip_cues, "torch": plain_cues}, a.rounds, a.warmup)
    rows.append(f"cues   {V} views, {result['pixels']} pixels: HIP {t['hip'][0]:8.3f} ms ({t['hip'][1]:.3f} .. {t['hip'][2]:.3f}) "
                f"{t['hip'][3]:7.1f} MiB, 3 launches | torch {t['torch'][0]:8.3f} ms ({t['torch'][1]:.3f} .. {t['torch'][2]:.3f}) "
                f"{t['torch'][3]:7.1f} MiB | x{t['torch'][0] / t['hip'][0]:.1f} | visibility equal, largest relative difference "
                + ", ".join(f"{k} {v:.1e}" for k, v in diffs.items()))
    result["cues"] = {"hip_ms": t["hip"][0], "hip_mib": t["hip"][3], "torch_ms": t["torch"][0], "torch_mib": t["torch"][3],
                      "launches": 3, "differences": diffs}

    # ---- refine.  A ray that runs along its plane meets it hundreds of units away or behind the camera, and there float32
    # formulations disagree by much of the value: the confident maps leave such pixels out (the alignment would divide by
    # their 0), and the comparison below leaves out what lies beyond FAR on either side.
    FAR = 100.0
    planed, _r, _z = depth_cues.apply_global_planes(cams, depths, masks, gdict, planes)
    planed_torch, _p = torch_refine(tcams, depths, masks, confs, monos, gdict, planes_dev, V)
    confs = [c & (x > 0) & (x < FAR) & (y > 0) & (y < FAR) for c, x, y in zip(confs, planed, planed_torch)]
    del planed, planed_torch, _p
    hip_refine = lambda: depth_cues.refine_depths_with_planes(cams, depths, masks, confs, monos, gdict, planes, n_input,  # noqa: E731
                                                              return_points=True)
    plain_refine = lambda: torch_refine(tcams, depths, masks, confs, monos, gdict, planes_dev, n_input)  # noqa: E731
    (got_d, got_p), (want_d, want_p) = hip_refine(), plain_refine()
    same = [(g > 0) == (w > 0) for g, w in zip(got_d, want_d)]
    flipped = sum(int((~k).sum()) for k in same)
    keep = [k & (g < FAR) & (w < FAR) for k, g, w in zip(same, got_d, want_d)]
    beyond = sum(int((k & ~q).sum()) for k, q in zip(same, keep))
    masked = sum(int((m > 0).sum()) for m in masks)
    assert flipped <= a.decisions * masked, (flipped, masked)
    diffs = {"depth": worst_relative(got_d, want_d, keep),
             "points": worst_relative(got_p, want_p, [k.reshape(-1, 1).expand(-1, 3) for k in keep])}
    assert max(diffs.values()) <= a.rtol, diffs
    _o, replaced, zeroed = depth_cues.apply_global_planes(cams, depths, masks, gdict, planes)
    del got_d, got_p, want_d, want_p
    t = alternate({"hip": hip_refine, "torch": plain_refine}, a.rounds, a.warmup)
    rows.append(f"refine {V} views ({V - n_input} inpainted), {n_pairs} (plane, view) pairs of {a.planes} planes: HIP {t['hip'][0]:8.3f} ms "
                f"({t['hip'][1]:.3f} .. {t['hip'][2]:.3f}) {t['hip'][3]:7.1f} MiB, 4 launches + {V} back-projections | torch "
                f"{t['torch'][0]:8.3f} ms ({t['torch'][1]:.3f} .. {t['torch'][2]:.3f}) {t['torch'][3]:7.1f} MiB | "
                f"x{t['torch'][0] / t['hip'][0]:.1f} | {int(replaced.sum())} pixels replaced, {int(zeroed.sum())} zeroed, {flipped} of "
                f"{masked} validity decisions differ, {beyond} pixels beyond {FAR:g} left out, largest relative difference " + ", ".join(f"{k} {v:.1e}" for k, v in diffs.items()))
    result["refine"] = {"hip_ms": t["hip"][0], "hip_mib": t["hip"][3], "torch_ms": t["torch"][0], "torch_mib": t["torch"][3],
                        "launches": 4 + V, "replaced": int(replaced.sum()), "zeroed": int(zeroed.sum()), "decisions_differ": flipped,
                        "masked_pixels": masked, "beyond_far": beyond, "differences": diffs}
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
