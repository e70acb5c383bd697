"""Times the chart matcher's loss (g4splat_amd/chart_match.py, csrc/chart_match.hip), forward plus backward, beside the same
contract written in plain torch on the same GPU, at n = 5, 20 and 50 charts of 384 x 512 (--sizes), and reports both sides'
peak memory.

Scene: n views on an arc looking at a slanted plane, 1 % of relative depth noise; most views see most of every other, and
about 85 % of all pairs match under spatial_extent / 20 (the count is printed); the current depths are the reference depths
times a smooth 0.5 % bump.

The torch side is written here from the contract (include/g4s_losses.h, "Chart matcher") the way the stage it replaces is
shaped: the n H W points repeated for the n cameras, two batched matrix products, grid_sample on every depth map, [n,n,H W]
errors, fov masks and products, autograd for the backward.  It is neither the code under test nor the reference's files.
Its floats follow torch's kernels, so a pair within rounding of an edge may fall the other way: before anything is timed the
two sides' match counts are compared to --decisions (1e-3) of all pairs and the two losses to 1e-4 relative, and both are
reported.  A size the torch side cannot allocate is skipped on that side and reported as such.  Timing: --warmup warm-up
rounds, then --rounds rounds that alternate the two sides, the device synchronised before each clock reading; medians; peak
memory is torch's allocator's above what the inputs hold (the library allocates nothing itself: its workspace comes from
that allocator too).

    python tools/bench_chart_match.py [--sizes 5,20,50] [--rounds 5] [--warmup 2] [--out FILE]
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g4splat_amd import _lib, chart_match  # noqa: E402

DEV = torch.device("cuda:0")


def make_scene(n, H, W, seed=5, noise=0.01):
    rng = np.random.default_rng(seed)
    cams = []
    for v in range(n):
        t = v / max(n - 1, 1) - 0.5
        yaw, pitch, centre = -0.45 * t, 0.08 * np.sin(3.0 * v), np.array([2.2 * t, 0.3 * np.cos(2.0 * v), 0.2 * np.sin(v)])
        cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
        R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
        wvt = np.eye(4)
        wvt[:3, :3], wvt[3, :3] = R, -centre @ R
        P = np.zeros((4, 4))
        P[0, 0], P[1, 1] = 1.6, 1.6 * W / H
        P[2, 2], P[2, 3], P[3, 2] = 100.0 / 99.99, 1.0, -100.0 * 0.01 / 99.99
        wvt32, P32 = wvt.astype(np.float32), P.astype(np.float32)
        cams.append(SimpleNamespace(world_view_transform=wvt32, projection_matrix=P32,
                                    full_proj_transform=(wvt32.astype(np.float64) @ P32.astype(np.float64)).astype(np.float32)))
    rec = chart_match.camera_records(cams, W, H).astype(np.float64)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    normal, depths = np.array([0.3, 0.2, 1.0]), []
    for v in range(n):
        o, D = rec[v, 0:3], rec[v, 3:12].reshape(3, 3)
        dirs = np.stack([D[k, 0] * xx + D[k, 1] * yy + D[k, 2] for k in range(3)], -1)
        depths.append((4.0 - normal @ o) / (dirs @ normal) * (1.0 + noise * rng.uniform(-1.0, 1.0, (H, W))))
    ref = torch.as_tensor(np.stack(depths), dtype=torch.float32, device=DEV)
    bump = 1.0 + 0.005 * torch.sin(0.05 * torch.arange(W, device=DEV))[None, None, :] * torch.cos(0.04 * torch.arange(H, device=DEV))[None, :, None]
    return cams, ref, (ref * bump).contiguous()


# ---- the contract in plain torch -------------------------------------------------------------------------------------------
def torch_pairs(rec, D):
    """(e, fov) [n, n H W] of every (target, source pixel) pair at the depths D [n,H,W]."""
    n, H, W = D.shape
    N, m = H * W, min(H, W)
    y, x = torch.meshgrid(torch.arange(H, device=DEV).float(), torch.arange(W, device=DEV).float(), indexing="ij")
    x, y = x.reshape(1, N), y.reshape(1, N)
    o, R = rec[:, 0:3], rec[:, 3:12].reshape(n, 3, 3)
    dirs = torch.stack([(R[:, k, 0:1] * x + R[:, k, 1:2] * y) + R[:, k, 2:3] for k in range(3)], -1)
    q = D.reshape(n, N, 1) * dirs + o[:, None, :]
    pts = q.reshape(1, n * N, 3).repeat(n, 1, 1)
    V, P = rec[:, 12:28].reshape(n, 4, 4), rec[:, 28:44].reshape(n, 4, 4)
    h = torch.cat([pts, torch.ones_like(pts[..., :1])], -1) @ V
    z = h[..., 2]
    a = h[..., :3] * torch.tensor([-1.0, -1.0, 1.0], device=DEV)
    r = torch.cat([a, torch.ones_like(a[..., :1])], -1) @ P
    u = r[..., :2] / r[..., 3:4].clamp_min(1e-6)
    fin = u.isfinite().all(dim=-1)
    g = u.nan_to_num(nan=0.0, posinf=0.0, neginf=0.0) * torch.tensor([W / m, H / m], device=DEV) * torch.tensor([-m / W, -m / H], device=DEV)
    s = torch.nn.functional.grid_sample(D.reshape(n, 1, H, W), g.view(n, -1, 1, 2), mode="bilinear", padding_mode="zeros",
                                        align_corners=False)[:, 0, :, 0]
    fov = (z > 0) & fin & (s > 0)
    return (z - s * fov).abs(), fov


@torch.no_grad()
def torch_match(rec, D, thr):
    e, fov = torch_pairs(rec, D)
    e[~fov] = 1e8
    return e < thr


def torch_loss(rec, D, matches):
    e, fov = torch_pairs(rec, D)
    return (e.nan_to_num() * fov * matches).mean()


def count_bits(words):
    """The number of set bits of the packed matches (int32 words), without expanding them."""
    v = words.to(torch.int64) & 0xFFFFFFFF
    v = v - ((v >> 1) & 0x55555555)
    v = (v & 0x33333333) + ((v >> 2) & 0x33333333)
    v = (v + (v >> 4)) & 0x0F0F0F0F
    return int((((v * 0x01010101) & 0xFFFFFFFF) >> 24).sum())


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
    ap.add_argument("--sizes", default="5,20,50")
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--decisions", type=float, default=1e-3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H, W = a.height, a.width
    result = {"build_id": _lib.load().g4s_version().decode(), "device": torch.cuda.get_device_name(DEV), "rounds": a.rounds,
              "warmup": a.warmup, "height": H, "width": W}
    rows = []
    for n in (int(s) for s in a.sizes.split(",")):
        cams, ref, cur = make_scene(n, H, W)
        matcher = chart_match.ChartMatcher(cams, reference_depths=ref)
        torch.cuda.synchronize(DEV)
        t0 = time.perf_counter()
        matcher.match(None)
        match_ms = (time.perf_counter() - t0) * 1e3
        rec = matcher._cams

        def hip():
            d = cur.clone().requires_grad_(True)
            v = matcher.loss(d)
            v.backward()
            return v.detach(), d.grad

        def plain():
            d = cur.clone().requires_grad_(True)
            v = torch_loss(rec, d, matches)
            v.backward()
            return v.detach(), d.grad

        sides, skipped = {"hip": hip}, None
        try:
            matches = torch_match(rec, ref, matcher.matching_thr)
            pairs, count, count_torch = n * n * H * W, count_bits(matcher.words), int(matches.sum())
            assert abs(count - count_torch) <= a.decisions * pairs, (n, count, count_torch)
            lh, lt = float(hip()[0]), float(plain()[0])
            assert abs(lh - lt) <= 1e-4 * abs(lt), (n, lh, lt)
            sides["torch"] = plain
        except torch.cuda.OutOfMemoryError as e:
            skipped, matches, count = str(e).splitlines()[0], None, count_bits(matcher.words)
            count_torch, lh, lt = None, float(hip()[0]), None
        torch.cuda.empty_cache()
        t = alternate(sides, a.rounds, a.warmup)
        row = (f"n = {n:2d} at {H}x{W}: {count} matches of {n * n * H * W} pairs, thr {matcher.matching_thr:.4f}, match() {match_ms:.2f} ms | "
               f"HIP fwd+bwd {t['hip'][0]:9.3f} ms ({t['hip'][1]:.3f} .. {t['hip'][2]:.3f}) {t['hip'][3]:9.1f} MiB | ")
        entry = {"matches": count, "matches_torch": count_torch, "loss_hip": lh, "loss_torch": lt, "match_ms": match_ms,
                 "hip_ms": t["hip"][0], "hip_mib": t["hip"][3]}
        if skipped is None:
            row += (f"torch {t['torch'][0]:9.3f} ms ({t['torch'][1]:.3f} .. {t['torch'][2]:.3f}) {t['torch'][3]:9.1f} MiB | "
                    f"x{t['torch'][0] / t['hip'][0]:.1f} | torch matches {count_torch}")
            entry.update({"torch_ms": t["torch"][0], "torch_mib": t["torch"][3]})
        else:
            row += f"torch SKIPPED, could not allocate: {skipped}"
            entry["torch_skipped"] = skipped
        rows.append(row)
        result[f"n_{n}"] = entry
        del matches, matcher
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
