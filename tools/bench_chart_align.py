"""Times the chart alignment losses (g4splat_amd/chart_align.py, csrc/chart_align.hip), forward plus backward, beside the same
terms written in plain torch on the same GPU, at n = 5, 20 and 50 charts of 384 x 512 (--sizes), and reports both sides' peak
memory.

Scene: n views on an arc looking at a slanted plane; the initial and the reference depths carry 3 % of white noise, the
current depths 2 % more; confidence in [1.2, 4], masks and gradient masks of 0 / 1.  All four terms are on, with the weights
of align_charts_in_parallel (gradient 10, normal 4, curvature 1).

The torch side is written here from the contract (include/g4s_losses.h, "Chart alignment losses") the way the stage it
replaces is shaped: all n charts back-projected to [n,H,W,3] points, sliced, crossed and normalised, padded and differenced
four ways, the depth term with the confidence and its log, autograd for the backward.  It is neither the code under test
nor the reference's files.  Its floats follow torch's kernels, so a Laplacian or a difference within rounding of zero may
take the other sign there: before anything is timed the two sides' four means are compared to 1e-4 relative, and at most
--kinks (1e-3) of the depth gradient's elements may differ by more than 1e-3 of the largest entry (a pixel's gradient
gathers some 30 such signs, torch's point differences carry a relative error of about 4e-6, and the quantities are of
order one: a few in 10^4); both figures are reported.  Timing:
--warmup warm-up rounds, then --rounds rounds that alternate the two sides, the device synchronised before each clock
reading; medians; peak memory is torch's allocator's above what the inputs hold (the library allocates nothing itself: its
workspace comes from that allocator too).  Bytes: the fused pair moves 68 B per pixel forward and 128 B backward, counted
from the kernels' loads and stores (bytes_per_pixel(); a neighbour's value is counted once: it comes from cache), and the
rate reported is those bytes over the measured time.

    python tools/bench_chart_align.py [--sizes 5,20,50] [--rounds 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g4splat_amd import _lib, chart_align  # noqa: E402
from tools.bench_chart_match import DEV, alternate, make_scene  # noqa: E402

WEIGHTS = (1.0, 10.0, 4.0, 1.0)
LAMBDA = 0.2


def bytes_per_pixel():
    """HBM bytes per pixel of the fused calls, every map counted once per kernel that reads or writes it.
    forward:  normals kernel reads d (4), writes nu (12); terms kernel reads d, r, c, m, d0, gm (24), nu0 (12), kappa0 (4),
              nu (12);
    backward: normals kernel 16; A/B kernel reads d (4), nu (12), kappa0 (4), nu0 (12), writes A, B (24); gather reads d, r,
              c, m, d0, gm (24), A, B (24), writes two gradients (8)."""
    fwd = (4 + 12) + (24 + 12 + 4 + 12)
    bwd = (4 + 12) + (4 + 12 + 4 + 12 + 24) + (24 + 24 + 8)
    return fwd, bwd


def make_inputs(n, H, W, seed=7):
    cams, plane, _cur = make_scene(n, H, W, noise=0.0)
    g = torch.Generator(device=DEV).manual_seed(seed)

    def noise(scale, shape=plane.shape):
        return 1.0 + scale * (2.0 * torch.rand(shape, generator=g, device=DEV) - 1.0)

    d0, ref = plane * noise(0.03), plane * noise(0.03)
    cur = d0 * noise(0.02)
    conf = 1.2 + 2.8 * torch.rand(plane.shape, generator=g, device=DEV)
    masks = (torch.rand(plane.shape, generator=g, device=DEV) < 0.8).float()
    gmasks = (torch.rand((n, H - 1, W - 1), generator=g, device=DEV) < 0.75).float()
    return cams, d0.contiguous(), ref.contiguous(), cur.contiguous(), conf, masks, gmasks


# ---- the contract in plain torch -------------------------------------------------------------------------------------------
def torch_normals(rec, D):
    n, H, W = D.shape
    y, x = torch.meshgrid(torch.arange(H, device=DEV).float(), torch.arange(W, device=DEV).float(), indexing="ij")
    pix = torch.stack([x, y, torch.ones_like(x)], -1).reshape(1, H * W, 3)
    dirs = pix @ rec[:, 3:12].reshape(n, 3, 3).transpose(1, 2)
    pts = (D.reshape(n, H * W, 1) * dirs + rec[:, None, 0:3]).reshape(n, H, W, 3)
    out = torch.zeros_like(pts)
    dx = pts[:, 2:, 1:-1] - pts[:, :-2, 1:-1]
    dy = pts[:, 1:-1, 2:] - pts[:, 1:-1, :-2]
    out[:, 1:-1, 1:-1] = torch.nn.functional.normalize(torch.cross(dx, dy, dim=-1), dim=-1)
    return out


def torch_curv(nu):
    p = torch.nn.functional.pad(nu[:, None], [0, 0, 1, 1, 1, 1], mode="replicate")[:, 0]
    c = p[:, 1:-1, 1:-1]
    lap = (p[:, :-2, 1:-1] - c) + (p[:, 1:-1, :-2] - c) + (p[:, 2:, 1:-1] - c) + (p[:, 1:-1, 2:] - c)
    return lap.norm(p=1, dim=-1)


def torch_img_grad(d):
    return torch.stack([d[:, 1:, :-1] - d[:, :-1, :-1], d[:, :-1, 1:] - d[:, :-1, :-1]], 1)


def torch_terms(rec, d, ref, conf, masks, d0, gmasks, nu0, kappa0):
    diff = (d - ref).abs()
    diff = masks * (conf * diff - LAMBDA * torch.log(conf))
    grad = (gmasks[:, None] * (torch_img_grad(d) - torch_img_grad(d0))).abs().mean()
    nu = torch_normals(rec, d)
    return torch.stack([diff.mean(), grad, (1.0 - (nu0 * nu).sum(-1)).mean(), (kappa0 - torch_curv(nu)).abs().mean()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5,20,50")
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kinks", type=float, default=1e-3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H, W = a.height, a.width
    fwd_b, bwd_b = bytes_per_pixel()
    result = {"build_id": _lib.load().g4s_version().decode(), "device": torch.cuda.get_device_name(DEV), "rounds": a.rounds,
              "warmup": a.warmup, "height": H, "width": W, "bytes_per_pixel_forward": fwd_b, "bytes_per_pixel_backward": bwd_b}
    weights = torch.tensor(WEIGHTS, device=DEV)
    rows = []
    for n in (int(s) for s in a.sizes.split(",")):
        cams, d0, ref, cur, conf, masks, gmasks = make_inputs(n, H, W)
        losses = chart_align.AlignmentLosses(cams, d0, confidence_weighting=LAMBDA)
        rec, nu0, kappa0 = losses._cams, losses.initial_normals, losses._initial_curv

        def hip():
            d, c = cur.clone().requires_grad_(True), conf.clone().requires_grad_(True)
            t = losses.terms(d, ref, c, masks, gmasks, use_gradient_loss=True)
            (t * weights).sum().backward()
            return t.detach(), d.grad, c.grad

        def plain():
            d, c = cur.clone().requires_grad_(True), conf.clone().requires_grad_(True)
            t = torch_terms(rec, d, ref, c, masks, d0, gmasks, nu0, kappa0)
            (t * weights).sum().backward()
            return t.detach(), d.grad, c.grad

        sides, skipped, agree = {"hip": hip}, None, None
        th, gh, _ch = hip()
        try:
            tt, gt, _ct = plain()
            agree = (float(((th - tt).abs() / tt.abs()).max()), float(((gh - gt).abs() > 1e-3 * gt.abs().max()).float().mean()))
            assert agree[0] <= 1e-4 and agree[1] <= a.kinks, (n, agree)
            sides["torch"] = plain
            del tt, gt, _ct
        except torch.cuda.OutOfMemoryError as e:
            skipped = str(e).splitlines()[0]
        del gh, _ch
        torch.cuda.empty_cache()
        t = alternate(sides, a.rounds, a.warmup)
        px = n * H * W
        row = (f"n = {n:2d} at {H}x{W}: means {[round(float(v), 6) for v in th]} | HIP fwd+bwd {t['hip'][0]:9.3f} ms "
               f"({t['hip'][1]:.3f} .. {t['hip'][2]:.3f}) {t['hip'][3]:9.1f} MiB, {px * (fwd_b + bwd_b) / t['hip'][0] / 1e6:.0f} GB/s of its "
               f"{fwd_b + bwd_b} B per pixel | ")
        entry = {"means_hip": [float(v) for v in th], "hip_ms": t["hip"][0], "hip_mib": t["hip"][3]}
        if skipped is None:
            row += (f"torch {t['torch'][0]:9.3f} ms ({t['torch'][1]:.3f} .. {t['torch'][2]:.3f}) {t['torch'][3]:9.1f} MiB | "
                    f"x{t['torch'][0] / t['hip'][0]:.1f} | means agree to {agree[0]:.1e}, {agree[1]:.1e} of the depth gradient's elements differ")
            entry.update({"torch_ms": t["torch"][0], "torch_mib": t["torch"][3], "means_rel": agree[0], "grad_elements_off": agree[1]})
        else:
            row += f"torch SKIPPED, could not allocate: {skipped}"
            entry["torch_skipped"] = skipped
        rows.append(row)
        result[f"n_{n}"] = entry
        del losses
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
