"""Times the two consumers of the chart points (g4splat_amd/chart_points.py) at n = 5, 20 and 50 charts of 384 x 512 (--sizes) with
one point per pixel -- what the shipped configurations produce (max_sfm_points: null, sfm_confidence_threshold: -1):

  fit    all charts from packed points and mono disparities to fitted depths: ChartPoints (project), fit_disparities (sample,
         float64 moments, coefficients on the device) and aligned_depths
  loss   one forward + backward of the point-reference term with a confidence (the inverted index is built once, before
         timing; its one-off cost is reported beside it)

against the torch composition, the feature's "before" (there is no parent-commit time: the parent has neither):

  fit    the reference's loop: per chart a homogeneous product with full_proj_transform, grid_sample, five sums, two .item()
         calls and 1 / (alpha + beta disp)
  loss   per chart grid_sample of the depths and of the confidence under the points, cat, the confidence term, mean, autograd
         backward (grid_sample's backward scatters with float atomics)

Scene: tools/bench_chart_match.py's (views on an arc at a slanted plane) without its depth noise; the points are each chart's own
back-projected pixels (half a pixel off grid_sample's centres, so every point blends four pixels) and land in their image.  Before timing, coefficients, the loss and both gradients of the two sides are
compared (1e-4 relative; the depths lie 1 % off the points, so that no sign hangs on rounding).
Timing: medians (min .. max) of --rounds rounds that alternate the sides after --warmup warm-up rounds, each between two device
synchronisations; the allocator peak is torch's above what is held before the round.  --launches counts the device kernels of
one call of each side with torch.profiler.

Nothing here has been measured until this tool has run on an MI355X; DESIGN.md ("Chart points") holds the table it prints.

    python tools/bench_chart_points.py [--sizes 5,20,50] [--rounds 5] [--warmup 2] [--launches] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g4splat_amd import _lib, chart_match, chart_points  # noqa: E402
from tools.bench_chart_aligner import count_kernels  # noqa: E402
from tools.bench_chart_match import DEV, alternate, make_scene  # noqa: E402


def pixel_points(cams, depths):
    """[n, H W, 3]: every chart's pixels back-projected at its depths (o + d dir, the matcher's ray record)."""
    n, H, W = depths.shape
    rec = torch.as_tensor(chart_match.camera_records(cams, W, H), device=DEV)
    y, x = torch.meshgrid(torch.arange(H, device=DEV).float(), torch.arange(W, device=DEV).float(), indexing="ij")
    pix = torch.stack([x, y, torch.ones_like(x)], -1).reshape(1, H * W, 3)
    dirs = pix @ rec[:, 3:12].reshape(n, 3, 3).transpose(1, 2)
    return (rec[:, None, 0:3] + depths.reshape(n, H * W, 1) * dirs).contiguous()


def torch_project(points, wvt, full, H, W):
    h = torch.cat([points, torch.ones_like(points[..., :1])], dim=-1)
    q = h @ full
    return (h @ wvt)[..., 2], (q[..., :2] / q[..., 3:4]).view(1, -1, 1, 2)


def torch_sample(m, grid):
    return torch.nn.functional.grid_sample(m[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0, 0, :, 0]


def torch_fit(points, wvts, fulls, disp):
    """The reference's loop: (coeffs as Python floats, fitted depths)"""
    n, H, W = disp.shape
    coeffs, out = [], []
    for c in range(n):
        z, grid = torch_project(points[c], wvts[c], fulls[c], H, W)
        d = torch_sample(disp[c], grid)
        t = 1.0 / z
        ones = torch.ones_like(t)
        beta = ((torch.sum(t * d) - torch.sum(t) * torch.sum(d) / torch.sum(ones)) / (torch.sum(d ** 2) - torch.sum(d) ** 2 / torch.sum(ones))).item()
        alpha = (torch.sum(t - beta * d) / torch.sum(ones)).item()
        coeffs.append((alpha, beta))
        out.append(1.0 / (alpha + beta * disp[c]))
    return coeffs, torch.stack(out)


def torch_loss(grids, zs, depths, conf, cw):
    s = torch.cat([torch_sample(depths[c], g) for c, g in enumerate(grids)])
    k = torch.cat([torch_sample(conf[c], g) for c, g in enumerate(grids)])
    return (k * (s - zs).abs() - cw * torch.log(k)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5,20,50")
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H, W = a.height, a.width
    result = {"build_id": _lib.load().g4s_version().decode(), "device": torch.cuda.get_device_name(DEV), "rounds": a.rounds,
              "warmup": a.warmup, "height": H, "width": W}
    rows = []
    for n in (int(s) for s in a.sizes.split(",")):
        cams, ref, cur = make_scene(n, H, W, noise=0.0)
        points = pixel_points(cams, ref)
        disp = (0.8 / ref + 0.05).contiguous()
        conf = (1.0 + torch.exp(0.3 * torch.sin(0.01 * torch.arange(n * H * W, device=DEV).float()))).reshape(n, H, W)
        wvts = torch.as_tensor(np.stack([c.world_view_transform for c in cams]), device=DEV)
        fulls = torch.as_tensor(np.stack([c.full_proj_transform for c in cams]), device=DEV)

        def hip_fit():
            cp = chart_points.ChartPoints(cams, points, H, W)
            coeffs = chart_points.fit_disparities(disp, cp)
            return coeffs, chart_points.aligned_depths(disp, coeffs)

        cp = chart_points.ChartPoints(cams, points, H, W)
        torch.cuda.synchronize(DEV)
        t0 = time.perf_counter()
        cp.build_index()
        torch.cuda.synchronize(DEV)
        index_ms = (time.perf_counter() - t0) * 1e3
        projected = [torch_project(points[c], wvts[c], fulls[c], H, W) for c in range(n)]
        grids, zs = [g for _z, g in projected], torch.cat([z for z, _g in projected])
        # 1 % behind the points in even charts and 1 % in front in odd ones: no point within rounding of the kink s = z, where the
        # two sides' signs would be rounding noise
        side = torch.where(torch.arange(n, device=DEV) % 2 == 0, 1.01, 0.99).reshape(n, 1, 1)
        d_hip, k_hip = (cur * side).requires_grad_(), conf.clone().requires_grad_()
        d_t, k_t = (cur * side).requires_grad_(), conf.clone().requires_grad_()

        def hip_loss():
            d_hip.grad = k_hip.grad = None
            loss = chart_points.point_reference_loss(d_hip, cp, k_hip, 0.2)
            loss.backward()
            return loss.detach()

        def t_loss():
            d_t.grad = k_t.grad = None
            loss = torch_loss(grids, zs, d_t, k_t, 0.2)
            loss.backward()
            return loss.detach()

        ch, ct = hip_fit()[0].cpu().numpy(), np.array(torch_fit(points, wvts, fulls, disp)[0])
        assert np.abs(ch - ct).max() <= 1e-4 * np.abs(ct).max(), (ch, ct)
        lh, lt = float(hip_loss()), float(t_loss())
        assert abs(lh - lt) <= 1e-4 * abs(lt), (lh, lt)
        gerr = max(float((g - t).abs().max() / t.abs().max()) for g, t in ((d_hip.grad, d_t.grad), (k_hip.grad, k_t.grad)))
        assert gerr <= 1e-4, gerr
        launches = None
        if a.launches:
            launches = {"fit": count_kernels(hip_fit), "fit_torch": count_kernels(lambda: torch_fit(points, wvts, fulls, disp)),
                        "loss": count_kernels(hip_loss), "loss_torch": count_kernels(t_loss)}
        t = alternate({"fit": hip_fit, "fit_torch": lambda: torch_fit(points, wvts, fulls, disp), "loss": hip_loss, "loss_torch": t_loss},
                      a.rounds, a.warmup)
        row = f"n = {n:2d}: " + " | ".join(f"{k} {v[0]:8.3f} ms ({v[1]:.3f} .. {v[2]:.3f}) {v[3]:7.1f} MiB" for k, v in t.items())
        row += f" | torch / hip: fit x{t['fit_torch'][0] / t['fit'][0]:.2f}, loss x{t['loss_torch'][0] / t['loss'][0]:.2f}"
        row += f" | index build (once) {index_ms:.3f} ms | gradients off torch's by {gerr:.2e} of their largest entry"
        if launches:
            row += " | kernels: " + ", ".join(f"{k} {v}" for k, v in launches.items())
        rows.append(row)
        print(row, flush=True)
        result[f"n_{n}"] = {k: {"ms": v[0], "min": v[1], "max": v[2], "mib": v[3]} for k, v in t.items()}
        result[f"n_{n}"].update(index_ms=index_ms, first_loss=(lh, lt), gradient_error=gerr)
        if launches:
            result[f"n_{n}"]["kernels"] = launches
        del cp, points, grids, zs, projected
        torch.cuda.empty_cache()
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
