"""Times the chart deformation (g4splat_amd/chart_deform.py, csrc/chart_deform.hip), forward plus backward, beside the same
contract written in plain torch on the same GPU, at n = 5, 20 and 50 charts of 384 x 512 (--sizes), and reports both sides'
peak memory.

Scene: n views on an arc looking at a slanted plane with 3 % of white noise on the depths (tools/bench_chart_match.py); the
configuration charts_alignment.py runs (four encoding levels of 8 channels, a depth encoding of 30 bins, 32 -> 64 -> 64 -> 1).
Parameters are trained-like: encodings uniform in +- scene_radius, Xavier-sized weights, biases in +- 0.5, so every ReLU goes
both ways.  The cotangent is a fixed random map.

The torch side is written here from the contract (include/g4s_losses.h, "Chart deformation") the way the stage it replaces is
shaped: four grid_sample calls over the levels at the transposed lattice, one over the depth encoding, a cat, a permute and
an add, three bmm with ReLU and the two rescales, the ray factor, autograd for the backward (its grid_sample backward scatters
with float atomics).  It is neither the code under test nor the reference's files.  Before anything is timed the two sides'
depths are compared to 1e-5 of the largest; and at a size of at most --check-pixels pixels (the 5-chart size) both sides'
depths and parameter gradients are compared with the torch side run in float64: the library may be off by at most four times
what float32 torch is off (the parameters are not settled away from the ReLU kinks and the cotangent has random signs, so a
gradient is a sum with cancellation and the float32 sides differ from each other by 1e-3 of the largest entry; against
float64 each is judged by itself); the figures are printed per parameter.  Timing: --warmup warm-up rounds, then --rounds rounds that alternate the two sides, the device synchronised before
each clock reading; medians; peak memory is torch's allocator's above what the inputs hold (the library allocates nothing
itself: its workspace comes from that allocator too) and is printed beside the workspace the library states.

FLOP: the matrix products only, 2 (E S + (layers - 2) S S) per pixel forward on the MFMA and three times that backward
(recompute, W^T dz, dz a^T); the rate is those over the measured time against the 157.3 TFLOPS f32 MFMA peak.  Bytes per
pixel, counted from the kernels' loads and stores (the weights and the encoding grids are small and come from cache):
forward reads d0 and depth_coords and writes the depth, 12 B; backward reads d0, depth_coords and the cotangent (12 B),
writes dL/dx (4 E), and the gathers read dL/dx once per level (4 C each, each pixel by up to four texels' threads, from cache)
and once for the depth encoding (4 E) with depth_coords (4): 12 + 12 + 4 E + 4 E + 4 E + 4 = 412 B at E = 32.

    python tools/bench_chart_deform.py [--sizes 5,20,50] [--rounds 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g4splat_amd import _lib, chart_deform  # noqa: E402
from tools.bench_chart_match import DEV, alternate, make_scene  # noqa: E402

MFMA_F32_PEAK = 157.3e12


def trained_like(m, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    with torch.no_grad():
        for k, p in m.named_parameters():
            u = torch.rand(p.shape, generator=g, device=DEV) * 2.0 - 1.0
            if k.endswith("encodings"):
                p.copy_(m.scene_radius * u)
            elif k.endswith("weight"):
                p.copy_(torch.randn(p.shape, generator=g, device=DEV) * float(np.sqrt(2.0 / p.shape[2])))
            else:
                p.copy_(0.5 * u)


def torch_depths(m, params, T=torch.float32):
    """The contract in plain torch: deformed depths [n,H,W] from the parameters (a dict by name), in the float type T."""
    n, H, W = m.n, m.height, m.width
    lin = lambda K: torch.linspace(-1.0, 1.0, K, device=DEV, dtype=T)  # noqa: E731
    uv = torch.stack(torch.meshgrid(lin(H), lin(W), indexing="ij"), dim=-1).repeat(n, 1, 1, 1)
    levels = [p for k, p in params.items() if k.startswith("charts_encoding")]
    enc = torch.cat([torch.nn.functional.grid_sample(v, uv, mode="bilinear", padding_mode="border", align_corners=False).permute(0, 2, 3, 1)
                     for v in levels], dim=-1).reshape(n, H * W, -1)
    grid = torch.cat([torch.zeros(n, H * W, 1, 1, device=DEV, dtype=T), -1 + 2 * m.depth_coords.to(T).view(n, H * W, 1, 1)], dim=-1)
    denc = torch.nn.functional.grid_sample(params["depth_encoding.encodings"][..., None], grid, mode="bilinear", padding_mode="border",
                                           align_corners=False)[..., 0].permute(0, 2, 1)
    x = (enc + denc) / m.scene_radius
    layers = m._NL
    for j in range(layers):
        x = torch.bmm(x, params[f"deformation.mlp.{2 * j}.weight"].transpose(1, 2)) + params[f"deformation.mlp.{2 * j}.bias"][:, None, :]
        if j < layers - 1:
            x = torch.relu(x)
    delta = (x[..., 0] * m.deformation_radius).reshape(n, H, W)
    y, xx = torch.meshgrid(torch.arange(H, device=DEV).to(T), torch.arange(W, device=DEV).to(T), indexing="ij")
    pix = torch.stack([xx, y, torch.ones_like(xx)], -1).reshape(1, H * W, 3)
    dirs = pix @ m._cams[:, 3:12].to(T).reshape(n, 3, 3).transpose(1, 2)
    d0 = m._d0.to(T)
    return d0 + delta * (torch.sign(d0) / dirs.norm(dim=-1).reshape(n, H, W))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5,20,50")
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check-pixels", type=int, default=1000000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H, W = a.height, a.width
    result = {"build_id": _lib.load().g4s_version().decode(), "device": torch.cuda.get_device_name(DEV), "rounds": a.rounds,
              "warmup": a.warmup, "height": H, "width": W}
    rows = []
    for n in (int(s) for s in a.sizes.split(",")):
        cams, d0, _cur = make_scene(n, H, W, noise=0.03)
        m = chart_deform.ChartDeformation(cams, d0)
        trained_like(m)
        by_id = {id(p): k for k, p in m.named_parameters()}
        names = [by_id[id(p)] for p in m._params()]  # the order of the library call
        cot = torch.rand((n, H, W), generator=torch.Generator(device=DEV).manual_seed(4), device=DEV) * 2.0 - 1.0
        E, S, NL = m._E, m._S, m._NL
        flop = 2.0 * (E * S + (NL - 2) * S * S) * n * H * W * 4.0  # forward, and three such products backward
        bytes_px = 12 + (12 + 4 * E + 4 * E + 4 * E + 4)

        def hip():
            params = [p.detach().clone().requires_grad_(True) for p in m._params()]
            d = chart_deform._Deform.apply(m, False, *params)
            (d * cot).sum().backward()
            return d.detach(), [p.grad for p in params]

        def plain(T=torch.float32):
            params = {k: p.detach().to(T).requires_grad_(True) if T != torch.float32 else p.detach().clone().requires_grad_(True)
                      for k, p in m.named_parameters()}
            d = torch_depths(m, params, T)
            (d * cot.to(T)).sum().backward()
            return d.detach(), [params[k].grad for k in names]

        def errors(got, want):
            """largest difference / largest entry of the float64 run: depths, then per parameter"""
            return [float((x.double() - y).abs().max() / y.abs().max()) for x, y in zip([got[0]] + got[1], [want[0]] + want[1])]

        sides, skipped, agree = {"hip": hip}, None, None
        dh, gh = hip()
        try:
            dt, gt = plain()
            agree = [float((dh - dt).abs().max() / dt.abs().max())]
            assert agree[0] <= 1e-5, (n, agree)
            if n * H * W <= a.check_pixels:  # both sides against the same contract in float64
                truth = plain(torch.float64)
                eh, et = errors((dh, gh), truth), errors((dt, gt), truth)
                del truth
                print(f"n = {n}: largest difference / largest entry against the float64 run, HIP then torch: depths {eh[0]:.1e} {et[0]:.1e}; "
                      + "; ".join(f"{k} {x:.1e} {y:.1e}" for k, x, y in zip(names, eh[1:], et[1:])), flush=True)
                agree += [max(eh[1:]), max(et[1:])]
                assert all(x <= max(4.0 * y, 1e-6) for x, y in zip(eh, et)), (n, eh, et)
            sides["torch"] = plain
            del dt, gt
        except torch.cuda.OutOfMemoryError as e:
            skipped = str(e).splitlines()[0]
        del dh, gh
        torch.cuda.empty_cache()
        t = alternate(sides, a.rounds, a.warmup)
        param_mib = sum(p.numel() for p in m.parameters()) * 4 / 2 ** 20
        ws_mib = m.workspace_bytes / 2 ** 20
        row = (f"n = {n:2d} at {H}x{W}: HIP fwd+bwd {t['hip'][0]:9.3f} ms ({t['hip'][1]:.3f} .. {t['hip'][2]:.3f}) {t['hip'][3]:9.1f} MiB "
               f"(workspace {ws_mib:.1f} MiB; the rest is the output, the cotangent product and the parameters' copies and gradients, "
               f"2 x {param_mib:.1f} MiB), {flop / t['hip'][0] / 1e9:.2f} TFLOPS = {100 * flop / (t['hip'][0] * 1e-3) / MFMA_F32_PEAK:.1f} % of the "
               f"f32 MFMA peak, {n * H * W * bytes_px / t['hip'][0] / 1e6:.0f} GB/s of its {bytes_px} B per pixel | ")
        entry = {"hip_ms": t["hip"][0], "hip_mib": t["hip"][3], "workspace_mib": ws_mib, "tflops": flop / t["hip"][0] / 1e9}
        if skipped is None:
            row += (f"torch {t['torch'][0]:9.3f} ms ({t['torch'][1]:.3f} .. {t['torch'][2]:.3f}) {t['torch'][3]:9.1f} MiB | "
                    f"x{t['torch'][0] / t['hip'][0]:.2f} | depths agree to {agree[0]:.1e}"
                    + (f", gradients off the float64 run by at most {agree[1]:.1e} (HIP), {agree[2]:.1e} (torch)" if len(agree) > 1 else ""))
            entry.update({"torch_ms": t["torch"][0], "torch_mib": t["torch"][3], "agreement": agree})
        else:
            row += f"torch SKIPPED, could not allocate: {skipped}"
            entry["torch_skipped"] = skipped
        rows.append(row)
        result[f"n_{n}"] = entry
        del m
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
