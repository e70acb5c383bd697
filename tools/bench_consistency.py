"""Times the two cross-view consistency solvers (g4splat_amd/consistency.py, csrc/tsdf/consistency.hip) against a
plain-torch version of the same contract on the same GPU.

Scene, by the recipe of tests/golden/make_golden_consistency.py at a user's size: --views cameras of --width x --height on
a sphere around the unit sphere, every depth map the camera-space depth of the pixel centre's ray (5.0 where it misses),
every cloud its view's depth back-projected at the pixel centres (so N = views * width * height), random images, masks
3 * face + 20 * view + 2 with the cube face of the pixel's point, six global planes listing every view that shows the
face, every fourth view an anchor, the first --input views input views.

Per solver it prints the median time of the whole call (HIP events around it, after --warmup warm-ups, over --runs runs: the
host plumbing and its synchronisations are inside), the kernel launches the call makes (counted from the code: fill, points,
paint; one memset, counts, source, resolve), the peak device memory the call adds (torch's allocator: outputs, state and
workspace), and the same for the baseline.

The baseline is written from include/g4s_render_maps.h ("Cross-view consistency"), not taken from the reference: the
projection element-wise in float32 in the contract's order, the point solver over [n,V] tables of visibility and taps for
chunks of --table-points points (the tables the reference keeps for all N), per-pixel winners by scatter_reduce(amax); the
plane solver with one projection per (pair, anchor) and a sequential in-place repaint per step, as the reference runs
it.  Both must give the library's outputs; the number of differing pixels is printed.  DESIGN.md ("Cross-view consistency")
holds the numbers.

    python tools/bench_consistency.py [--views 24] [--width 800] [--height 600] [--input 4] [--runs 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g4splat_amd import _lib, consistency, synthetic  # noqa: E402

BACKGROUND = 5.0
THRESHOLD = 0.1


def cube_face(p):
    axis = np.abs(p).argmax(-1)
    comp = np.take_along_axis(p, axis[..., None], -1)[..., 0]
    return 2 * axis + (comp < 0) + 1


def make_scene(V, W, H, seed=0):
    """(cams, depths [V][H,W] f32, clouds [V][H*W,3] f32, images [V][H,W,3] u8, masks [V][H,W] i32, dict, anchors), numpy."""
    rng = np.random.default_rng(seed)
    cams, depths, clouds, masks = [], [], [], []
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for v in range(V):
        a, h = 2.0 * math.pi * v * 0.381966, -0.8 + 1.6 * (v + 0.5) / V
        r = math.sqrt(1.0 - h * h)
        eye = (3.2 * r * math.cos(a), 3.2 * r * math.sin(a), 3.2 * h)
        cam = synthetic.look_at_camera(eye, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), math.radians(55), W, H)
        wvt = np.asarray(cam.world_view_transform, np.float64).reshape(4, 4)
        fx, fy = W / (2.0 * math.tan(cam.FoVx / 2.0)), H / (2.0 * math.tan(cam.FoVy / 2.0))
        d = np.stack([(x + 0.5 - W / 2.0) / fx, (y + 0.5 - H / 2.0) / fy, np.ones_like(x)], -1).reshape(-1, 3)
        Rinv = np.linalg.inv(wvt[:3, :3])
        o, dirs = -wvt[3, :3] @ Rinv, d @ Rinv  # world point = o + t * dirs, t the camera-space depth
        qa, qb, qc = (dirs * dirs).sum(1), 2.0 * (dirs @ o), float(o @ o) - 1.0
        disc = qb * qb - 4.0 * qa * qc
        t = (-qb - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * qa)
        depth = np.where((disc > 0) & (t > 0), t, BACKGROUND).astype(np.float32)
        p = o[None] + depth.astype(np.float64)[:, None] * dirs
        cams.append(cam)
        depths.append(depth.reshape(H, W))
        clouds.append(p.astype(np.float32))
        masks.append(np.where(depth < 4.9, 3 * cube_face(p) + 20 * v + 2, 0).astype(np.int32).reshape(H, W))
    images = [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(V)]
    gdict = {}
    for k, face in enumerate([4, 1, 6, 2, 5, 3]):
        gdict[k] = [(v, 3 * face + 20 * v + 2) for v in range(V) if (masks[v] == 3 * face + 20 * v + 2).any()]
    return cams, depths, clouds, images, masks, gdict, list(range(0, V, 4))


# ---- the plain-torch baseline -------------------------------------------------------------------------------------------------
class TorchView:
    def __init__(self, cam, depth):
        self.H, self.W = depth.shape
        self.M = torch.as_tensor(np.asarray(cam.world_view_transform, np.float32).reshape(4, 4)).tolist()
        self.fx = float(np.float32(self.W / (2.0 * math.tan(float(cam.FoVx) / 2.0))))
        self.fy = float(np.float32(self.H / (2.0 * math.tan(float(cam.FoVy) / 2.0))))
        self.depth = depth.reshape(-1)


def torch_surface(P, view, threshold):
    """(vis bool [n], pix int64 [n]) of points [n,3]: the header's projection, tap and SURFACE, one torch op per operation."""
    M, W, H = view.M, view.W, view.H
    c = [((P[:, 0] * M[0][j] + P[:, 1] * M[1][j]) + P[:, 2] * M[2][j]) + M[3][j] for j in range(3)]
    z = c[2]
    u = (c[0] / z) * view.fx + W * 0.5
    v = (c[1] / z) * view.fy + H * 0.5
    inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    col = torch.where(inside, u, torch.zeros_like(u)).long().clamp_(max=W - 1)
    row = torch.where(inside, v, torch.zeros_like(v)).long().clamp_(max=H - 1)
    pix = row * W + col
    d = view.depth[pix]
    vis = inside & (z > 0) & ((z - d).abs() / (z + 1e-6) < threshold)
    return vis, pix


def torch_point_solver(views, images, points, n_input, threshold, table_points):
    """images: float32 [H,W,3] per view.  Returns (images_out, confident maps)."""
    dev, N, V = points.device, points.size(0), len(views)
    conf = [torch.ones(v.H * v.W, dtype=torch.uint8, device=dev) for v in views]
    winner = [torch.zeros(v.H * v.W, dtype=torch.int64, device=dev) for v in views]
    colours = torch.zeros((N, 3), dtype=torch.uint8, device=dev)
    for lo in range(0, N, table_points):
        P = points[lo: lo + table_points]
        n = P.size(0)
        vis = torch.zeros((n, V), dtype=torch.bool, device=dev)
        pix = torch.zeros((n, V), dtype=torch.int64, device=dev)
        for v, view in enumerate(views):
            vis[:, v], pix[:, v] = torch_surface(P, view, threshold)
        seen = vis[:, :n_input].any(1) if n_input else torch.zeros(n, dtype=torch.bool, device=dev)
        unseen = torch.nonzero(~seen & vis.any(1)).squeeze(-1)
        first = vis[unseen].float().argmax(1)
        first_pix = pix[unseen, first]
        for v in range(V):
            sel = first == v
            if sel.any():
                colours[lo + unseen[sel]] = (images[v].reshape(-1, 3)[first_pix[sel]] * 255.0).to(torch.uint8)
        for v in range(n_input, V):
            conf[v][pix[vis[:, v] & seen, v]] = 0
            idx = torch.nonzero(vis[:, v] & ~seen).squeeze(-1)
            winner[v].scatter_reduce_(0, pix[idx, v], idx + (lo + 1), "amax")
    outs = []
    for v, view in enumerate(views):
        out = images[v].reshape(-1, 3).clone()
        hit = torch.nonzero(winner[v]).squeeze(-1)
        # a tensor divisor: torch divides by a Python scalar on the device as a multiplication by its reciprocal, which
        # is not the contract's correctly rounded division
        out[hit] = colours[winner[v][hit] - 1].float() / torch.tensor(255.0, device=dev)
        outs.append(out.reshape(view.H, view.W, 3))
    return outs, [c.reshape(v.H, v.W) for c, v in zip(conf, views)]


def torch_plane_solver(views, images, masks, clouds, gdict, anchors, threshold):
    """images: uint8 [H,W,3] per view.  Returns (images_out, anchor per plane, counts [K][A])."""
    sets = {(w, p): torch.nonzero(masks[w].reshape(-1) == p).squeeze(-1) for pairs in gdict.values() for w, p in pairs}
    counts = []
    for pairs in gdict.values():
        row = [0] * len(anchors)
        for w, p in pairs:
            P = clouds[w][sets[(w, p)]]
            for j, a in enumerate(anchors):
                row[j] += int(torch_surface(P, views[a], threshold)[0].sum().item())
        counts.append(row)
    anchor = consistency.choose_anchor_views(counts, anchors)
    out = [im.reshape(-1, 3).clone() for im in images]
    for k, pairs in zip(range(len(gdict)), gdict.values()):
        if anchor[k] == -1:
            continue
        for w, p in pairs:
            q = sets[(w, p)]
            vis, pix = torch_surface(clouds[w][q], views[anchor[k]], threshold)
            out[w][q[vis]] = out[anchor[k]][pix[vis]]  # the right-hand side is gathered before the assignment
    return [o.reshape(im.shape) for o, im in zip(out, images)], anchor, counts


# ---- measurement ----------------------------------------------------------------------------------------------------------------
def measure(fn, dev, runs, warmup):
    """((median, least, largest) ms between HIP events around fn(), peak bytes the call adds, fn()'s last result)."""
    for _ in range(warmup):
        out = fn()
    del out
    times, peak = [], 0
    for _ in range(runs):
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize(dev)
        times.append(a.elapsed_time(b))
        peak = max(peak, torch.cuda.max_memory_allocated(dev) - base)
    return (statistics.median(times), min(times), max(times)), peak, out


def differing_pixels(got, want):
    return sum(int((a.reshape(-1, a.shape[-1] if a.dim() == 3 else 1) != b.reshape(-1, b.shape[-1] if b.dim() == 3 else 1))
                   .any(-1).sum()) for a, b in zip(got, want))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--input", type=int, default=4)
    ap.add_argument("--table-points", type=int, default=1 << 30, help="points per [n,V] table of the baseline")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_consistency needs a HIP device: there is no CPU measurement")
    dev = torch.device("cuda:0")
    V, W, H, I = args.views, args.width, args.height, args.input
    cams, depths, clouds, images, masks, gdict, anchors = make_scene(V, W, H)

    def to(arrays):
        return [torch.as_tensor(a, device=dev) for a in arrays]

    depths, clouds, images, masks = to(depths), to(clouds), to(images), to(masks)
    float_images = [im.float() / torch.tensor(255.0, device=dev) for im in images]  # u8 / 255, correctly rounded
    points = torch.cat(clouds)
    N = points.size(0)
    views = [TorchView(c, d) for c, d in zip(cams, depths)]
    result = {"views": V, "width": W, "height": H, "input_views": I, "points": N, "anchors": len(anchors),
              "device": torch.cuda.get_device_name(dev), "library": _lib.load().g4s_version().decode(),
              "runs": args.runs, "warmup": args.warmup}

    def report(name, ms, peak, launches=None):
        result[name] = {"ms": ms[0], "min_ms": ms[1], "max_ms": ms[2], "peak_MiB": peak / 2 ** 20, "launches": launches}
        print(f"{name:22s} {ms[0]:10.2f} ms ({ms[1]:.2f} .. {ms[2]:.2f})  peak {peak / 2 ** 20:10.1f} MiB" +
              (f"  {launches} launches" if launches else ""))

    ms, peak, got = measure(lambda: consistency.solve_point_inconsistency(cams, depths, float_images, points, I, THRESHOLD), dev,
                            args.runs, args.warmup)
    report("point solver", ms, peak, 3)
    ms, peak, want = measure(lambda: torch_point_solver(views, float_images, points, I, THRESHOLD, args.table_points), dev,
                             args.runs, args.warmup)
    report("point solver (torch)", ms, peak)
    result["point_image_pixels_differing"] = differing_pixels(got[0], want[0])
    result["point_conf_pixels_differing"] = differing_pixels(got[1], want[1])
    result["point_pixels_differing"] = result["point_image_pixels_differing"] + result["point_conf_pixels_differing"]
    result["point_pixels_repainted"] = differing_pixels(got[0], float_images)
    result["point_conf_zeros"] = sum(int((c == 0).sum()) for c in got[1])
    result["point_storage_bytes"] = {"library_per_point": 4, "reference_per_point": 17 * V,
                                     "library_MiB": (4 * N + 4 * (V - I) * W * H) / 2 ** 20, "reference_MiB": 17 * V * N / 2 ** 20}
    del got, want

    ms, peak, got = measure(lambda: consistency.solve_plane_inconsistency(cams, depths, images, masks, clouds, gdict, anchors,
                                                                          THRESHOLD), dev, args.runs, args.warmup)
    report("plane solver", ms, peak, 4)
    ms, peak, want = measure(lambda: torch_plane_solver(views, images, masks, clouds, gdict, anchors, THRESHOLD), dev, args.runs,
                             args.warmup)
    report("plane solver (torch)", ms, peak)
    result["plane_pixels_differing"] = differing_pixels(got[0], want[0])
    result["plane_pixels_repainted"] = differing_pixels(got[0], images)
    result["plane_anchors_equal"] = [got[1][k] for k in gdict] == want[1] and got[2].tolist() == want[2]
    result["plane_triples"] = sum(len(p) for p in gdict.values()) * (len(anchors) + 1)
    print(f"pixels differing from the baseline: point solver {result['point_pixels_differing']}, plane solver "
          f"{result['plane_pixels_differing']}; anchors and counts equal: {result['plane_anchors_equal']}")
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
