"""What the mip filter costs on the MI355X at the metric's size (S3: 1.5 M surfels, 1600x1200, SH degree 3), filter ON
as G4Splat trains (configs/free_gaussians_refinement/default.yaml: use_mip_filter).

    python tools/bench_mip.py [--rounds 5] [--iters 24] [--P 1500000] [--width 1600] [--height 1200]

1. The training iteration of tools/train_iter_bench.py (render -> fused L1+SSIM + regularisers -> backward -> statistics
   -> FusedAdam) with `get_activated` as the fused pair g4s_activations_mip_forward / _backward and as the three torch
   getters, IN THE SAME PROCESS: the tool swaps the model class's property between rounds (no switch in the library),
   rounds alternate fused / torch after a warm-up of both, and the figure is the median of the rounds' means with the
   smallest and largest round beside it (the round-to-round spread any difference has to beat).  With --filter-off the
   same iteration with the filter off is timed too (the path bench.py measures).
2. compute_mip_filter at P points for V = 24 and V = 100 views: g4s_mip_filter (camera table + two launches) against
   the reference's torch loop over the cameras on the same device; median time of --filter-runs calls each (host clock
   around a synchronise: the torch loop's cost is its launches), and the peak device memory each adds.  Their results are
   compared first: the largest relative difference, and for rows further apart than 1e-5 (another decision taken: the
   loop's GEMM sums in its own order) how close they sit to a decision threshold.

One JSON line."""
import argparse
import json
import math
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g4splat_amd import _lib, synthetic  # noqa: E402
from g4splat_amd.gaussian_model import GaussianModel  # noqa: E402
from g4splat_amd.gaussian_renderer import render  # noqa: E402
from g4splat_amd.losses import geometry_regularizers, photometric_loss  # noqa: E402

FUSED = GaussianModel.get_activated
TORCH = property(lambda self: (self.get_scaling, self.get_rotation, self.get_opacity))


def mip_cameras(cams, width, height):
    """R, T, focal lengths as the reference's cameras hold them, from world_view_transform = W2C^T."""
    out = []
    for c in cams:
        wvt = np.asarray(c.world_view_transform, np.float32)
        out.append(SimpleNamespace(R=wvt[:3, :3].copy(), T=wvt[3, :3].copy(), focal_x=width / (2 * c.tanfovx),
                                   focal_y=height / (2 * c.tanfovy), image_width=width, image_height=height))
    return out


def threshold_margin(xyz, views, znear=0.2):
    """Rows on which the two computations differ by more than rounding took another decision somewhere (the torch loop's
    xyz @ R is a GEMM with its own summation order): for each such row the smallest relative distance, in float64, of any
    view's depth to znear or of its projection to a border -- and of those the largest.  A value of the order of float32's
    resolution says every such row sits on a threshold."""
    if xyz.shape[0] == 0:
        return 0.0
    x = xyz.detach().double().cpu().numpy()
    margin = np.full(x.shape[0], np.inf)
    for c in views:
        pc = x @ c.R.astype(np.float64) + c.T.astype(np.float64)
        z = pc[:, 2]
        margin = np.minimum(margin, np.abs(z - znear) / znear)
        zc = np.maximum(z, 0.001)
        for val, size in ((pc[:, 0] / zc * c.focal_x + c.image_width / 2.0, c.image_width),
                          (pc[:, 1] / zc * c.focal_y + c.image_height / 2.0, c.image_height)):
            for thr in (-0.15 * size, 1.15 * size):
                margin = np.minimum(margin, np.where(z > 0.5 * znear, np.abs(val - thr) / abs(thr), np.inf))
    return float(margin.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds per variant")
    ap.add_argument("--iters", type=int, default=24, help="iterations per round")
    ap.add_argument("--P", type=int, default=1_500_000)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--filter-runs", type=int, default=7)
    ap.add_argument("--filter-off", action="store_true", help="also time the iteration with the filter off")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    _lib.load()
    scene = synthetic.scene_room(a.P, seed=0)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    model = GaussianModel(sh_degree=3, use_mip_filter=True)
    model.create_from_parameters(t(scene.means3D), t(scene.scales), t(scene.rotations), torch.rand((a.P, 3), device=dev))
    with torch.no_grad():
        model._opacity.copy_(torch.logit(t(scene.opacities).clamp(1e-4, 1 - 1e-4)))
        model._features_rest.copy_(t(scene.shs[:, 1:, :]))
    model.active_sh_degree = 3
    model.training_setup()
    room = synthetic.room_cameras(8, a.width, a.height, fovx_deg=90.0)
    cams = [SimpleNamespace(image_width=a.width, image_height=a.height, FoVx=2 * math.atan(c.tanfovx),
                            FoVy=2 * math.atan(c.tanfovy), world_view_transform=t(c.world_view_transform),
                            full_proj_transform=t(c.full_proj_transform), camera_center=t(c.camera_center),
                            znear=0.01, zfar=100.0) for c in room]
    model.compute_mip_filter(mip_cameras(room, a.width, a.height))
    gts = [torch.rand((3, a.height, a.width), device=dev) for _ in cams]
    pipe = SimpleNamespace(depth_ratio=0.0, compute_cov3D_python=False)
    bg = torch.zeros(3, device=dev)

    def iteration(i):
        out = render(cams[i % 8], model, pipe, bg)
        loss, _l1, _s = photometric_loss(out["render"], gts[i % 8], 0.2)
        normal_mean, dist_mean = geometry_regularizers(out["rend_normal"], out["surf_normal"], out["rend_dist"])
        (loss + 0.05 * normal_mean + 100.0 * dist_mean).backward()
        with torch.no_grad():
            model.add_densification_stats(out["viewspace_points"], out["visibility_filter"], out["radii"])
            model.optimizer.step()
            model.optimizer.zero_grad(set_to_none=True)

    def one_round(prop, filter_on=True):
        GaussianModel.get_activated = prop
        model.set_mip_filter(filter_on)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.iters):
            iteration(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.iters * 1e3

    variants = [("fused", FUSED, True), ("torch_getters", TORCH, True)]
    if a.filter_off:
        variants.append(("filter_off", FUSED, False))
    try:
        for _name, prop, on in variants:  # warm-up of every variant: code objects, allocator pools, Adam state
            one_round(prop, on)
        times = {name: [] for name, _p, _o in variants}
        for _ in range(a.rounds):
            for name, prop, on in variants:
                times[name].append(one_round(prop, on))
    finally:
        GaussianModel.get_activated = FUSED
        model.set_mip_filter(True)
    iteration_ms = {name: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                           "rounds": [round(x, 3) for x in v]} for name, v in times.items()}

    # ---- compute_mip_filter ------------------------------------------------------------------------------------------
    def timed(fn):
        fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        ms = []
        for _ in range(a.filter_runs):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                "peak_extra_MiB": round((torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20, 2)}

    filter_rows = {}
    for V in (24, 100):
        views = mip_cameras(synthetic.room_cameras(V, a.width, a.height, fovx_deg=90.0), a.width, a.height)
        model.compute_mip_filter(views)
        hip = model.mip_filter.clone()
        ref = model._mip_filter_torch(views)
        rel = ((hip - ref).abs() / ref)[:, 0]
        apart = torch.nonzero(rel > 1e-5)[:, 0]
        filter_rows[f"V={V}"] = {"hip": timed(lambda: model.compute_mip_filter(views)),
                                 "torch_loop": timed(lambda: model._mip_filter_torch(views)),
                                 "largest_relative_difference_of_the_other_rows": float(rel[rel <= 1e-5].max()),
                                 "rows_apart_by_more_than_1e-5": int(apart.numel()),
                                 "their_largest_margin_to_a_decision": threshold_margin(model._xyz[apart], views)}
    print(json.dumps({"P": a.P, "resolution": [a.width, a.height], "iters_per_round": a.iters, "rounds": a.rounds,
                      "iteration_ms_filter_on": iteration_ms, "compute_mip_filter": filter_rows}))


if __name__ == "__main__":
    main()
