"""Times view selection (g4splat_amd/view_selection.py, csrc/tsdf/view_select.hip) beside the same contract written in plain
torch on the same GPU, in the reference's formulation, at the novel-view stage's own sizes:

    select   select_need_inpaint_views over --points points (1.5 M) and --cameras candidate cameras (120) of 512 x 512,
             select_num = 10: one bits launch and one counts launch for the whole table, then host decisions, against a
             projection of ALL points into both cameras for every pair the decisions ask about (a [3,3] x [3,P] matmul, the
             in-image test, two boolean masks, four .item() read-backs per pair);
    lookat   get_novel_cams_lookat_points for --views input views (24) of 800 x 600 points each, fps_num = 10: k launches
             for all clouds together, against fps_num - 1 sequential rounds of torch kernels per view over [N,3] and [N]
             temporaries, and torch.cdist for the nearest centre.

The torch versions are written here; they are neither the code under test nor the reference's files.  Both sides run under
the same seeds (random for the selection, torch's device generator for the draws), so their outputs must be EQUAL, which is
checked before anything is timed.  Timing: --warmup warm-up rounds, then --rounds rounds that alternate the two sides,
the device synchronised before each clock reading; medians; peak memory is torch's allocator's above what the inputs hold
(the library allocates through it).

    python tools/bench_view_selection.py [--rounds 7] [--warmup 2] [--out FILE]
"""
import argparse
import json
import math
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g4splat_amd import _lib, synthetic, view_selection as vs  # noqa: E402

DEV = torch.device("cuda:0")
SIZE = 512


def make_selection_scene(n_points, n_cameras):
    cams = []
    for i in range(n_cameras):
        a, z = 2.0 * math.pi * i * 0.381966, -2.0 + 4.0 * (i + 0.5) / n_cameras
        cams.append(synthetic.look_at_camera((3.2 * math.cos(a), 3.2 * math.sin(a), z), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0),
                                             math.radians(60.0), SIZE, SIZE))
    g = torch.Generator(device="cpu").manual_seed(7)
    pts = torch.rand((n_points, 3), generator=g) * 8.0 - 4.0
    s = torch.randn((n_points // 4, 3), generator=g)
    pts[: n_points // 4] = s / s.norm(dim=1, keepdim=True) * (0.9 + 0.2 * torch.rand((n_points // 4, 1), generator=g))
    rates = (torch.rand(n_cameras, generator=g) * 0.7).tolist()
    return cams, pts.to(DEV), rates


# ---- the contract in plain torch, the reference's formulation ------------------------------------------------------------
class TorchCamera:
    def __init__(self, cam):
        M = torch.as_tensor(np.asarray(cam.world_view_transform, np.float32), device=DEV)
        self.R_w2c, self.T = M[:3, :3].T.contiguous(), M[3, :3].contiguous()
        self.W, self.H = cam.image_width, cam.image_height
        self.fx = self.W / (2.0 * math.tan(cam.FoVx / 2.0))
        self.fy = self.H / (2.0 * math.tan(cam.FoVy / 2.0))


def torch_visible_mask(cam, pts):
    pc = torch.matmul(cam.R_w2c, pts.T).T + cam.T
    depth = pc[:, 2]
    p2 = pc[:, :2] / pc[:, 2:3]
    p2[:, 0] = p2[:, 0] * cam.fx + cam.W / 2
    p2[:, 1] = p2[:, 1] * cam.fy + cam.H / 2
    inside = (p2[:, 0] >= 0) & (p2[:, 0] < cam.W) & (p2[:, 1] >= 0) & (p2[:, 1] < cam.H)
    return (depth > 0) & inside


def torch_ratio(cam1, cam2, pts):
    m1, m2 = torch_visible_mask(cam1, pts), torch_visible_mask(cam2, pts)
    common = torch.logical_and(m1, m2).sum().item()
    r1 = common / m1.sum().item() if m1.sum().item() > 0 else 0
    r2 = common / m2.sum().item() if m2.sum().item() > 0 else 0
    return max(r1, r2)


def torch_select(tcams, rates, pts, select_num, low=0.05, high=0.5, bound=0.8):
    """The five steps with a pair check per question; returns (ids, pair checks made)."""
    checks = [0]

    def covisible(view, chosen):
        for s in chosen:
            checks[0] += 1
            if torch_ratio(tcams[s], tcams[view], pts) > bound:
                return True
        return False
    order = list(enumerate(rates))
    random.shuffle(order)
    inside = [i for i, r in order if low <= r <= high]
    chosen = inside[:1]
    for view in inside[1:]:
        if not covisible(view, chosen):
            chosen.append(view)
        if len(chosen) >= select_num:
            break
    if len(chosen) < select_num:
        for view in [i for i, r in order if r < low and i not in chosen]:
            if not covisible(view, chosen):
                chosen.append(view)
            if len(chosen) >= select_num:
                break
    if len(chosen) < select_num:
        rest = [i for i in range(len(rates)) if i not in chosen and rates[i] <= high]
        random.shuffle(rest)
        chosen.extend(rest[: select_num - len(chosen)])
    return chosen, checks[0]


def torch_fps(points, k):
    n = points.shape[0]
    chosen = torch.zeros(k, dtype=torch.int, device=points.device)
    dist = torch.ones(n, device=points.device) * 1e10
    chosen[0] = torch.randint(0, n, (1,), device=points.device)
    for i in range(1, k):
        d = torch.sum((points - points[chosen[i - 1]].unsqueeze(0)) ** 2, dim=1)
        dist = torch.min(dist, d)
        chosen[i] = torch.argmax(dist)
    return points[chosen]


def torch_lookat(train, clouds, novel, k):
    closest = torch.argmin(torch.cdist(novel, train), dim=1)
    samples = torch.stack([torch_fps(clouds[i], k) for i in range(train.shape[0])], dim=0)
    ids = torch.randint(0, k, (novel.shape[0],), device=novel.device)
    return samples[closest, ids]


# ---- timing --------------------------------------------------------------------------------------------------------------
def alternate(sides, rounds, warmup):
    """{name: (median ms, peak MiB above what was allocated before)} of callables run in alternating rounds."""
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
    return {n: (statistics.median(times[n]), peaks[n]) for n in sides}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_500_000)
    ap.add_argument("--cameras", type=int, default=120)
    ap.add_argument("--select-num", type=int, default=10)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--cloud", type=int, default=800 * 600)
    ap.add_argument("--novel", type=int, default=200)
    ap.add_argument("--fps-num", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = {"build_id": _lib.load().g4s_version().decode(), "device": torch.cuda.get_device_name(DEV), "rounds": a.rounds,
              "warmup": a.warmup}
    rows = []

    # ---- selection
    cams, pts, rates = make_selection_scene(a.points, a.cameras)
    tcams = [TorchCamera(c) for c in cams]

    def hip_select():
        random.seed(3)
        return vs.select_need_inpaint_views(cams, rates, pts, a.select_num)

    def plain_select():
        random.seed(3)
        return torch_select(tcams, rates, pts, a.select_num)[0]
    ids = hip_select()
    random.seed(3)
    tids, checks = torch_select(tcams, rates, pts, a.select_num)
    assert ids == tids, f"selection differs: {ids} vs {tids}"
    table = vs.Covisibility(pts, cams)
    differ = sum(int((table.mask(c) != torch_visible_mask(tcams[c], pts)).sum()) for c in range(0, a.cameras, 16))
    t = alternate({"hip": hip_select, "torch": plain_select}, a.rounds, a.warmup)
    rows.append(f"select {a.points} points, {a.cameras} cameras {SIZE}x{SIZE}, select_num {a.select_num}: HIP {t['hip'][0]:9.3f} ms "
                f"{t['hip'][1]:7.1f} MiB (table of {a.cameras * (a.cameras + 1) // 2} pairs) | torch {t['torch'][0]:9.3f} ms "
                f"{t['torch'][1]:7.1f} MiB ({checks} pair checks) | x{t['torch'][0] / t['hip'][0]:.1f} | ids equal, "
                f"{differ} mask bits differ in every 16th camera")
    result["select"] = {"hip_ms": t["hip"][0], "hip_mib": t["hip"][1], "torch_ms": t["torch"][0], "torch_mib": t["torch"][1],
                        "pair_checks": checks, "ids": ids, "mask_bits_differ": differ}
    del table, pts

    # ---- look-at points
    g = torch.Generator(device="cpu").manual_seed(11)
    train = (torch.randn((a.views, 3), generator=g) * 2.0).to(DEV)
    clouds = (torch.randn((a.views, a.cloud, 3), generator=g) * 1.5).to(DEV) + train[:, None, :]
    novel = (torch.randn((a.novel, 3), generator=g) * 2.5).to(DEV)

    def hip_lookat():
        torch.manual_seed(5)
        return vs.get_novel_cams_lookat_points(train, clouds, novel, a.fps_num)

    def plain_lookat():
        torch.manual_seed(5)
        return torch_lookat(train, clouds, novel, a.fps_num)
    got, want = hip_lookat(), plain_lookat()
    assert torch.equal(got, want), f"look-at points differ in {int((got != want).any(1).sum())} of {a.novel} rows"
    t = alternate({"hip": hip_lookat, "torch": plain_lookat}, a.rounds, a.warmup)
    rows.append(f"lookat {a.views} views of {a.cloud} points, fps_num {a.fps_num}, {a.novel} novel cameras: HIP {t['hip'][0]:9.3f} ms "
                f"{t['hip'][1]:7.1f} MiB | torch {t['torch'][0]:9.3f} ms {t['torch'][1]:7.1f} MiB | x{t['torch'][0] / t['hip'][0]:.1f} | "
                f"points equal")
    result["lookat"] = {"hip_ms": t["hip"][0], "hip_mib": t["hip"][1], "torch_ms": t["torch"][0], "torch_mib": t["torch"][1]}
    text = "\n".join([f"{result['build_id']} on {result['device']}; medians of {a.rounds} alternating rounds after {a.warmup} "
                      f"warm-ups"] + rows)
    print(text)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
