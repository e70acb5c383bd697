"""Mesh evaluation timing: python tools/bench_mesh_eval.py [--vertices 2000000] [--samples 200000]   (run on the GPU box)

Two synthetic meshes of the size the reference scores (eval/mesh_eval.py: vertex clouds of a few million, 200 000 surface
samples a side): a bumpy height field of --vertices vertices and a displaced copy.  Timed between HIP events, median of 5
after 2 warm-ups: the two voxel down-samples, the four nearest-neighbour searches, the two surface samplings and evaluate
as a whole.  Beside them, on the same box, scikit-learn's KDTree doing the same four queries on the same clouds (build +
query, wall clock, once), after its indices and distances have been compared with the library's.  Prints one line per
piece; no test depends on a figure from here."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from g4splat_amd import mesh as mesh_mod  # noqa: E402
from g4splat_amd import mesh_eval as me  # noqa: E402


def height_field(n_vertices, seed, lift):
    """A side x side grid over a 6 x 4 m floor with smooth bumps, two triangles a cell, as a DeviceMesh."""
    side = int(np.sqrt(n_vertices))
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.linspace(0, 6, side, dtype=np.float32), np.linspace(0, 4, side, dtype=np.float32), indexing="xy")
    z = lift + 0.2 * np.sin(3 * x + rng.uniform(0, 6)) * np.cos(2 * y) + rng.normal(0, 0.002, x.shape)
    v = np.stack([x.ravel(), y.ravel(), z.ravel().astype(np.float32)], 1).astype(np.float32)
    i = (np.arange(side - 1)[:, None] * side + np.arange(side - 1)[None, :]).ravel()
    t = np.concatenate([np.stack([i, i + 1, i + side + 1], 1), np.stack([i, i + side + 1, i + side], 1)]).astype(np.int32)
    dev = torch.device("cuda", torch.cuda.current_device())
    return mesh_mod.DeviceMesh(torch.as_tensor(v, device=dev), torch.full((len(v), 3), 0.5, device=dev), torch.as_tensor(t, device=dev))


def timed(fn, rounds=5, warmup=2):
    times, out = [], None
    for it in range(warmup + rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            times.append(e0.elapsed_time(e1))
    return float(np.median(times)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=2_000_000)
    ap.add_argument("--samples", type=int, default=200_000)
    ap.add_argument("--down_sample", type=float, default=0.02)
    ap.add_argument("--no_kdtree", action="store_true")
    args = ap.parse_args()
    pred, trgt = height_field(args.vertices, 0, 0.0), height_field(args.vertices, 1, 0.02)
    print(f"meshes: {len(pred.vertices)} vertices, {len(pred.triangles)} triangles each; {args.samples} samples a side", flush=True)

    ms, vp = timed(lambda: me.voxel_down_sample(pred.vertices, args.down_sample))
    ms2, vt = timed(lambda: me.voxel_down_sample(trgt.vertices, args.down_sample))
    print(f"voxel_down_sample x2      {ms + ms2:9.3f} ms   -> {len(vp)} and {len(vt)} points", flush=True)
    ms, (pp, _n, _f) = timed(lambda: me.sample_surface(pred, args.samples))
    ms2, (pt, _n, _f) = timed(lambda: me.sample_surface(trgt, args.samples))
    print(f"sample_surface x2         {ms + ms2:9.3f} ms   (cumulative areas included)", flush=True)
    pairs = [("vertices pred <- trgt", vp, vt), ("vertices trgt <- pred", vt, vp), ("samples pred <- trgt", pp, pt), ("samples trgt <- pred", pt, pp)]
    total, results = 0.0, []
    for name, cloud, query in pairs:
        ms, (dist, idx) = timed(lambda: me.nearest_neighbors(cloud, query))
        total += ms
        results.append((dist.cpu().numpy(), idx.cpu().numpy()))
        print(f"nearest_neighbors {name:22s} {ms:9.3f} ms   {len(cloud)} references, {len(query)} queries", flush=True)
    print(f"nearest_neighbors x4      {total:9.3f} ms", flush=True)
    ms, metrics = timed(lambda: me.evaluate(pred, trgt, down_sample=args.down_sample, n_samples=args.samples), rounds=3, warmup=1)
    print(f"evaluate                  {ms:9.3f} ms   " + ", ".join(f"{k} {v:.4f}" for k, v in metrics.items()), flush=True)

    if args.no_kdtree:
        return
    from sklearn.neighbors import KDTree
    total = 0.0
    for (name, cloud, query), (dist, idx) in zip(pairs, results):
        c, q = cloud.cpu().numpy().astype(np.float64), query.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        kd, ki = KDTree(c).query(q)
        s = time.perf_counter() - t0
        total += s
        same = float(np.mean(ki[:, 0] == idx))
        worst = float(np.max(np.abs(kd[:, 0] - dist) / np.maximum(kd[:, 0], 1e-30)))
        print(f"KDTree (host) {name:22s} {s * 1e3:9.1f} ms   same index on {100 * same:.4f} % of the queries, "
              f"largest relative distance difference {worst:.2e}", flush=True)
    print(f"KDTree (host) x4          {total * 1e3:9.1f} ms   ({os.cpu_count()} CPUs on the box; scikit-learn's query is one thread)", flush=True)


if __name__ == "__main__":
    main()
