"""Times the plane-mask stage (g4splat_amd/plane_masks.py, csrc/tsdf/plane_masks.hip) beside the host formulation of the
reference's planes/plane_excavator.py on the same machine, at the stage's own size: --views input views (24) of 800 x 600
plus --inpainted inpainted views (12) of 512 x 512, --masks SAM-like masks (256) per view.

    hip    excavate_planes over all views in one call: k-means from given seeds, pick and merge, opening, components, pair
           counts, paint, relabel -- the launches of all views shared, the masks read where they lie on the device.
    host   per view, as the reference runs it: sklearn KMeans(n_clusters=8, init=the same seeds, n_init=1) over the normals,
           the pick and merge, per kept cluster a 9x9 opening and an 8-connected labelling with scipy.ndimage (in place of
           OpenCV, which this build does not have), the size filter, and the reference-shaped numpy double loop over masks
           and components with its repaint and np.mean per plane.  Its inputs are host arrays already: no copy is timed.

The host code is written here; it is neither the code under test nor the reference's files.  What is checked before anything
is timed, per view: sklearn stops after the same number of iterations, its centres agree to 1e-5 and its labels on all but
0.1 % of the pixels (near-ties of float32 distances); from the library's labels the scipy components equal the library's
exactly; from those the double loop's seg_mask and areas equal the library's exactly and its mean normals to 1e-5.
Timing: after that pass (the warm-up of both sides), --rounds rounds that alternate the two sides, the device synchronised
before each clock reading; medians with their range.  The host side can be limited to the first --host-views views of each
size (its time is then reported for those views, next to the library's time for the same views).

    python tools/bench_plane_masks.py [--rounds 3] [--host-views N] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g4splat_amd import _lib, plane_masks  # noqa: E402

DEV = torch.device("cuda:0")
RATIO = 0.004
DIRECTIONS = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0.6, 0, 0.8], [0, -0.6, 0.8], [-0.8, 0.6, 0], [0.577, 0.577, 0.577]])


def make_view(rng, H, W, n_masks):
    sites = rng.uniform(0, 1, (12, 2)) * [H, W]
    direction = np.concatenate([np.arange(7), rng.integers(0, 7, 5)])
    noise = rng.uniform(0.05, 0.15, 12)
    yy, xx = np.mgrid[0:H, 0:W]
    site = np.argmin((yy[..., None] - sites[:, 0]) ** 2 + (xx[..., None] - sites[:, 1]) ** 2, axis=2)
    n = DIRECTIONS[direction[site]] + rng.normal(size=(H, W, 3)) * noise[site][..., None]
    normals = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(np.float32)
    masks = np.zeros((n_masks, H, W), bool)
    for m in range(n_masks):  # ellipses of up to 4.5 % of the image, about half of them above the size bar
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        ry, rx = H * rng.uniform(0.02, 0.12), W * rng.uniform(0.02, 0.12)
        y0, y1, x0, x1 = int(max(cy - ry, 0)), int(min(cy + ry + 1, H)), int(max(cx - rx, 0)), int(min(cx + rx + 1, W))
        masks[m, y0:y1, x0:x1] = ((yy[y0:y1, x0:x1] - cy) / ry) ** 2 + ((xx[y0:y1, x0:x1] - cx) / rx) ** 2 <= 1.0
    return normals, masks


# ---- the stage on the host, the reference's formulation -------------------------------------------------------------------
def host_kmeans(normals, seeds):
    from sklearn.cluster import KMeans
    km = KMeans(n_clusters=len(seeds), init=seeds, n_init=1).fit(normals.reshape(-1, 3))
    return km.labels_, km.cluster_centers_, km.n_iter_


def host_components(pred, centres, shape, n_clusters=6):
    """normals_cluster after the KMeans: the list of component masks."""
    from scipy import ndimage
    lut = plane_masks.select_normal_clusters(np.bincount(pred, minlength=len(centres)), centres, n_clusters)
    bar = shape[0] * shape[1] * RATIO
    box, eight = np.ones((9, 9), bool), np.ones((3, 3), bool)
    out = []
    for r in range(int(lut.max()) + 1):
        mask = np.isin(pred, np.flatnonzero(lut == r)).reshape(shape)
        opened = ndimage.binary_dilation(ndimage.binary_erosion(mask, box, border_value=1), box)
        lab, n = ndimage.label(opened, structure=eight)
        sizes = np.bincount(lab.reshape(-1), minlength=n + 1)
        clean = np.isin(lab, [i for i in range(1, n + 1) if sizes[i] >= bar])
        lab, n = ndimage.label(mask & clean, structure=eight)
        out.extend(lab == i for i in range(1, n + 1))
    return out


def host_join(normals, masks, clusters, max_planes=100):
    """PlaneExcavator.__call__ after the network, with an int32 seg_mask."""
    H, W = normals.shape[:2]
    bar = H * W * RATIO
    seg = np.zeros((H, W), np.int32)
    count = 0
    for mask in sorted(masks, key=lambda x: np.sum(x)):
        for normal_mask in clusters:
            intersect = mask & normal_mask
            if np.sum(intersect) < bar:
                continue
            count += 1
            seg[intersect] = count
    new = np.zeros_like(seg)
    avg, areas = [], []
    for i in range(min(max_planes, count)):
        mask = seg == i + 1
        area = mask.sum()
        if area < bar:
            continue
        areas.append(area)
        new[mask] = len(areas)
        a = np.mean(normals[mask], axis=0)
        avg.append(a / np.sqrt((a ** 2).sum()))
    return new, (np.stack(avg) if avg else None), (np.array(areas) if areas else None)


def host_view(normals, masks, seeds):
    pred, centres, _ = host_kmeans(normals, seeds)
    return host_join(normals, masks, host_components(pred, centres, normals.shape[:2]))


# ---- checks and timing ---------------------------------------------------------------------------------------------------
def check_view(v, normals, masks, seeds, dev_normals):
    labels, centres, counts, n_iter = plane_masks.kmeans_normals(dev_normals, seeds)
    pred, host_centres, host_iter = host_kmeans(normals, seeds)
    differ = int((labels.cpu().numpy().reshape(-1) != pred).sum())
    assert n_iter == host_iter, (v, n_iter, host_iter)
    assert np.abs(centres.cpu().numpy() - host_centres).max() <= 1e-5, v
    assert differ <= 1e-3 * pred.size, (v, differ)
    lut = plane_masks.select_normal_clusters(counts, centres)
    comps, sizes, n = plane_masks.normal_components(labels, lut, normals.shape[0] * normals.shape[1] * RATIO)
    clusters = host_components(labels.cpu().numpy().reshape(-1).astype(np.int64), centres.cpu().numpy(), normals.shape[:2])
    comps_h = comps.cpu().numpy()
    assert len(clusters) == n and all((c == (comps_h == i)).all() for i, c in enumerate(clusters)), v
    got = plane_masks.join_planes(dev_normals, torch.from_numpy(masks).to(DEV), comps, n, normals.shape[0] * normals.shape[1] * RATIO)
    seg, avg, areas = host_join(normals, masks, clusters)
    assert (got.seg_mask.cpu().numpy() == seg).all(), v
    assert (areas is None) == (got.areas is None) and (areas is None or got.areas.tolist() == areas.tolist()), v
    assert avg is None or np.abs(got.normal - avg).max() <= 1e-5, v
    return differ, n, 0 if areas is None else len(areas)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--inpainted", type=int, default=12)
    ap.add_argument("--masks", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-views", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(23)
    shapes = [(600, 800)] * a.views + [(512, 512)] * a.inpainted
    views = [make_view(rng, H, W, a.masks) for H, W in shapes]
    seeds = [plane_masks.kmeanspp_seeds(n, 8, torch.Generator().manual_seed(v)) for v, (n, _m) in enumerate(views)]
    dev_normals = [torch.from_numpy(n).to(DEV) for n, _m in views]
    dev_masks = [torch.from_numpy(m).to(DEV) for _n, m in views]
    k = a.host_views
    subset = list(range(len(views))) if k is None else list(range(min(k, a.views))) + list(range(a.views, a.views + min(k, a.inpainted)))
    print(f"{len(views)} views, {sum(h * w for h, w in shapes)} pixels, {a.masks} masks each; host side on {len(subset)} views", flush=True)

    differ = comps = planes = 0
    for v in subset:
        d, n, p = check_view(v, *views[v], seeds[v], dev_normals[v])
        differ, comps, planes = differ + d, comps + n, planes + p
        print(f"  view {v}: equal ({d} labels differ from sklearn's, {n} components, {p} planes)", flush=True)

    def hip(idx):
        out = plane_masks.excavate_planes([dev_normals[v] for v in idx], [dev_masks[v] for v in idx], min_size_ratio=RATIO,
                                          init=[seeds[v] for v in idx])
        torch.cuda.synchronize(DEV)
        return out
    whole = hip(range(len(views)))
    again = hip(range(len(views)))
    assert all(torch.equal(x.seg_mask, y.seg_mask) for x, y in zip(whole, again)), "two runs differ"
    sides = {"hip_all": lambda: hip(range(len(views))), "hip_subset": lambda: hip(subset),
             "host_subset": lambda: [host_view(*views[v], seeds[v]) for v in subset]}
    times = {n: [] for n in sides}
    for r in range(a.rounds):
        for name, fn in sides.items():
            torch.cuda.synchronize(DEV)
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
        print(f"  round {r}: " + ", ".join(f"{n} {t[-1]:.1f} ms" for n, t in times.items()), flush=True)
    stat = {n: (statistics.median(t), min(t), max(t)) for n, t in times.items()}
    result = {"build_id": _lib.load().g4s_version().decode(), "device": torch.cuda.get_device_name(DEV), "rounds": a.rounds,
              "views": len(views), "host_views": len(subset), "masks": a.masks, "pixels": sum(h * w for h, w in shapes),
              "labels_differ_from_sklearn": differ, "components": comps, "planes": planes,
              **{f"{n}_ms": s[0] for n, s in stat.items()}, **{f"{n}_range_ms": s[1:] for n, s in stat.items()}}
    text = (f"{result['build_id']} on {result['device']}; medians (min .. max) of {a.rounds} alternating rounds\n"
            f"all {len(views)} views: HIP {stat['hip_all'][0]:.1f} ms ({stat['hip_all'][1]:.1f} .. {stat['hip_all'][2]:.1f})\n"
            f"{len(subset)} views: HIP {stat['hip_subset'][0]:.1f} ms ({stat['hip_subset'][1]:.1f} .. {stat['hip_subset'][2]:.1f}) | host "
            f"{stat['host_subset'][0]:.1f} ms ({stat['host_subset'][1]:.1f} .. {stat['host_subset'][2]:.1f}) | "
            f"x{stat['host_subset'][0] / stat['hip_subset'][0]:.0f} | outputs equal on these views: {differ} labels differ from sklearn's, "
            f"{comps} components, {planes} planes")
    print(text)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
