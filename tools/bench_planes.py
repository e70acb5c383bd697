"""Times the global-planes stage (g4splat_amd/planes.py, csrc/tsdf/planes.hip) on a synthetic room of planes: the six
walls of a box seen from --views cameras inside it, --points chart points sampled on the walls (in runs along each wall, the
order a back-projected chart cloud has), every view's mask the wall index of its pixel.

Per kernel pass it prints the median time between HIP events over --runs runs after --warmup warm-ups, the number of
launches the pass takes, and the bytes per second achieved against the pass's byte model (what a pass must move at least):

    labels       per point 12 B read; per (point, view) one 4 B label written, one 4 B mask tap and two 4 B zmin accesses
                 (the atomic min and the read-back): 12 N + 16 N V
    overlap      per point the 4 B label and 8 B of membership per 64 global planes: N (4 + 8 ceil(G / 64))
    assign       per point the label and one membership word read and written: N (4 + 16)
    row overlap  per point one membership word, and the others for the points of the row (counted as all): 8 N ceil(G / 64)
    row merge    one word read per point, one written for the points of the row (counted as all): 16 N
    row mask     one word read and one byte written per point: 9 N

and then the wall time of the whole of get_global_3Dplane.  DESIGN.md ("Global planes") holds the numbers.

    python tools/bench_planes.py [--points 2000000] [--views 30] [--size 512] [--runs 10] [--warmup 3] [--out FILE]
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
from g4splat_amd import _lib, planes, synthetic  # noqa: E402

DEV = torch.device("cuda:0")
HALF = 2.0  # the room is the box [-2, 2]^3


def room_points(n, rng):
    """[n,3] float32 on the six walls, wall after wall, each wall in raster order with a small jitter."""
    per = [n // 6 + (1 if k < n % 6 else 0) for k in range(6)]
    out = []
    for k, m in enumerate(per):
        side = max(int(math.ceil(math.sqrt(m))), 1)
        idx = np.arange(m)
        a = ((idx // side + 0.5) / side * 2.0 - 1.0) * HALF + rng.uniform(-1e-3, 1e-3, m)
        b = ((idx % side + 0.5) / side * 2.0 - 1.0) * HALF + rng.uniform(-1e-3, 1e-3, m)
        c = np.full(m, HALF if k % 2 == 0 else -HALF)
        axis = k // 2
        out.append(np.stack([c, a, b] if axis == 0 else ([a, c, b] if axis == 1 else [a, b, c]), 1))
    return np.concatenate(out).astype(np.float32)


def wall_mask(cam, size):
    """int32 [size,size]: 10 (wall + 1) for the wall each pixel's ray leaves the room through (ids 10 .. 60)."""
    wvt = np.asarray(cam.world_view_transform, np.float64)
    c2w = np.linalg.inv(wvt.T)
    f = size / (2.0 * math.tan(cam.FoVx / 2.0))
    y, x = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    d = np.stack([(x - size / 2) / f, (y - size / 2) / f, np.ones_like(x, np.float64)], -1) @ c2w[:3, :3].T
    o = c2w[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (HALF - o) / d, np.where(d < 0, (-HALF - o) / d, np.inf))
    axis = t.argmin(-1)
    sign = np.take_along_axis(d, axis[..., None], -1)[..., 0] < 0
    return (10 * (2 * axis + sign + 1)).astype(np.int32)


def make_views(n, size):
    cams = []
    for i in range(n):
        a, z = 2.0 * math.pi * i * 0.381966, -1.0 + 2.0 * (i + 0.5) / n
        eye = (0.8 * math.cos(a), 0.8 * math.sin(a), 0.5 * z)
        target = (eye[0] + math.cos(a + 1.0), eye[1] + math.sin(a + 1.0), eye[2] - 0.3 * z)
        cams.append(synthetic.look_at_camera(eye, target, (0.0, 0.0, 1.0), math.radians(70.0), size, size))
    return cams, [torch.as_tensor(wall_mask(c, size), device=DEV) for c in cams]


def timed(fn, runs, warmup):
    """Median milliseconds between HIP events around fn()."""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(DEV)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(DEV)
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--views", type=int, default=30)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    N, V = args.points, args.views
    pts = torch.as_tensor(room_points(N, np.random.default_rng(0)), device=DEV)
    cams, masks = make_views(V, args.size)
    lib = _lib.load()
    result = {"points": N, "views": V, "size": args.size, "device": torch.cuda.get_device_name(DEV),
              "library": lib.g4s_version().decode(), "passes": {}}

    def report(name, ms, launches, model_bytes):
        result["passes"][name] = {"ms": ms, "launches": launches, "model_bytes": model_bytes,
                                  "GB_per_s": model_bytes / (ms * 1e-3) / 1e9}
        print(f"{name:12s} {ms:9.3f} ms  {launches} launch(es)  {model_bytes / 2 ** 20:9.1f} MiB model  "
              f"{model_bytes / (ms * 1e-3) / 1e9:8.1f} GB/s")

    views = planes._LabelledViews(cams, pts, masks, 0.01)
    chunk = views.chunk
    ms = timed(lambda: views._launch(0, min(chunk, V)), args.runs, args.warmup)
    vc = min(chunk, V)
    report("labels", ms, 2, 12 * N + 16 * N * vc)
    result["passes"]["labels"]["views_per_launch"] = vc

    # the state the merge is in after all views: every view's planes assigned
    provider = planes._DeviceProvider(views)
    member = provider.member
    for v in range(V):
        ids, sizes, _c = provider.view_counts(v)
        provider.assign(v, [member.G + k for k in range(len(ids))])  # every plane of every view a row of its own
    G, words = member.G, (member.G + 63) // 64
    labels, P = views.labels(V - 1), len(views.id_lists[V - 1])
    out = torch.empty(P * (G + 1), dtype=torch.int32, device=DEV)
    report("overlap", timed(lambda: _lib.call("g4s_plane_overlap", N, _lib.ptr(labels), P, *member._args(), _lib.ptr(out),
                                              _lib.ptr(out[P * G:]), None, 0, _lib.stream(DEV)), args.runs, args.warmup),
           1, N * (4 + 8 * words))
    ws = torch.empty(lib.g4s_plane_assign_workspace(P), dtype=torch.uint8, device=DEV)
    target = _lib.array(_lib.c_i, list(range(P)))
    report("assign", timed(lambda: _lib.call("g4s_plane_assign", N, _lib.ptr(labels), P, target, *member._args(), _lib.ptr(ws),
                                             ws.numel(), _lib.stream(DEV)), args.runs, args.warmup), 1, N * 20)
    row = torch.empty(G, dtype=torch.int32, device=DEV)
    report("row overlap", timed(lambda: _lib.call("g4s_plane_row_overlap", N, *member._args(), 0, _lib.ptr(row), None, 0,
                                                  _lib.stream(DEV)), args.runs, args.warmup), 1, 8 * N * words)
    report("row merge", timed(lambda: _lib.call("g4s_plane_row_merge", N, *member._args(), 0, 0 if G < 2 else 1, None, 0,
                                                _lib.stream(DEV)), args.runs, args.warmup), 1, 16 * N)
    mask = torch.empty(N, dtype=torch.uint8, device=DEV)
    report("row mask", timed(lambda: _lib.call("g4s_plane_row_mask", N, *member._args(), 0, _lib.ptr(mask), None, 0,
                                               _lib.stream(DEV)), args.runs, args.warmup), 1, 9 * N)

    torch.cuda.synchronize(DEV)
    t0 = time.perf_counter()
    idx, ids = planes.get_global_3Dplane(cams, pts, masks)
    torch.cuda.synchronize(DEV)
    result["end_to_end"] = {"s": time.perf_counter() - t0, "global_planes": len(ids), "rows_before_sweep": G,
                            "membership_MiB": member.words.numel() * 8 / 2 ** 20,
                            "labels_MiB_per_launch": 4 * N * vc / 2 ** 20}
    print(f"get_global_3Dplane: {result['end_to_end']['s']:.3f} s, {len(ids)} global planes "
          f"({G} rows when every plane of every view is kept apart)")
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
