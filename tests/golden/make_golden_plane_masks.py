"""Golden vectors of the plane-mask stage (tests/golden/plane_masks.npz), made on the CPU of the build container.

Normal maps.  Two synthetic maps, 45 x 67 and 120 x 160 (H x W): seven unit directions dealt over a Voronoi layout of twelve
    sites, plus Gaussian noise whose standard deviation varies per site between 0.05 and 0.15, renormalised.  float32.
k-means.  Per map the seeds of sklearn.cluster.kmeans_plusplus(X, 8, random_state=0) and the labels, centres and n_iter_ of
    KMeans(n_clusters=8, init=seeds, n_init=1).fit(X): the reference's call (planes/plane_excavator.py normals_cluster) with
    the seeding made explicit.
Merge cases.  The reference's OWN planes/tools.py merge_normal_clusters, imported from the reference tree with an empty
    stand-in for cv2 (the function uses numpy only) and called on (pred, sorted_topk, centers) cases: no merge, one merge, a
    chain (a ~ b and b ~ c but not a ~ c, and a cluster that absorbs two), and a merge whose second pick admits a label that
    was not in sorted_topk.  The last needs a tie of counts (a label outside the pick never has more members than one inside
    it); the case is one where numpy's argpartition and the library's smaller-label-first rule decide the tie alike.
    Recorded per case: counts [8], sorted_topk, centers [8,3] and the table label -> rank (or -1) read off the function's
    results.

Nothing of the reference is copied: the npz holds inputs and recorded results only.
Run in the build container only (needs the reference tree that _ref_import.py names, and sklearn):
    python tests/golden/make_golden_plane_masks.py"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import REF  # noqa: E402

REF_PLANES = os.path.join(REF, "planes")
SHAPES = {"small": (45, 67), "large": (120, 160)}
DIRECTIONS = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0.6, 0, 0.8], [0, -0.6, 0.8], [-0.8, 0.6, 0], [0.577, 0.577, 0.577]],
                      np.float64)


def normal_map(H, W, seed):
    rng = np.random.default_rng(seed)
    sites = rng.uniform(0, 1, (12, 2)) * [H, W]
    direction = np.concatenate([np.arange(7), rng.integers(0, 7, 5)])
    noise = rng.uniform(0.05, 0.15, 12)
    yy, xx = np.mgrid[0:H, 0:W]
    d2 = (yy[..., None] - sites[:, 0]) ** 2 + (xx[..., None] - sites[:, 1]) ** 2
    site = np.argmin(d2, axis=2)
    n = DIRECTIONS[direction[site]] + rng.normal(size=(H, W, 3)) * noise[site][..., None]
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    return n.astype(np.float32)


def kmeans_record(normals):
    from sklearn.cluster import KMeans, kmeans_plusplus
    X = normals.reshape(-1, 3)
    seeds, _ = kmeans_plusplus(X, 8, random_state=0)
    km = KMeans(n_clusters=8, init=seeds, n_init=1).fit(X)
    return seeds.astype(np.float32), km.labels_.astype(np.int8).reshape(normals.shape[:2]), km.cluster_centers_, km.n_iter_


def merge_cases():
    axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 1, 1], [-1, -1, -1]], np.float64)
    near = lambda v, w, t: np.asarray(v, np.float64) * (1 - t) + np.asarray(w, np.float64) * t  # noqa: E731
    cases = {}
    cases["no_merge"] = ([100, 90, 80, 70, 60, 50, 40, 5], [0, 1, 2, 3, 4, 5], axes * 0.9)
    c = axes.copy()
    c[3] = near(axes[1], axes[0], 0.1)  # rank 3 joins rank 1
    cases["one_merge"] = ([100, 90, 80, 70, 60, 50, 40, 5], [0, 1, 2, 3, 4, 5], c)
    c = axes.copy()
    c[0], c[1], c[2] = [1, 0, 0], [0.97, 0.243, 0], [0.88, 0.475, 0]  # 0 ~ 1, 1 ~ 2, 0 !~ 2
    c[5] = near(axes[3], axes[4], 0.08)
    c[4] = near(axes[3], axes[2], 0.08)  # 3 absorbs 4 and 5
    cases["chain"] = ([100, 90, 80, 70, 60, 50, 40, 5], [0, 1, 2, 3, 4, 5], c)
    c = axes.copy()
    c[1] = near(axes[0], axes[2], 0.06)  # label 1 joins label 0; labels 4, 6, 7 tie at 5 members and 6 was picked
    cases["admits_seventh"] = ([50, 20, 50, 60, 5, 100, 5, 5], [5, 3, 2, 0, 1, 6], c)
    return cases


def run_merge(counts, topk, centers):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, REF_PLANES)
    try:
        import tools
    finally:
        sys.path.remove(REF_PLANES)
    pred = np.repeat(np.arange(len(counts)), counts)
    new_pred, new_topk, n = tools.merge_normal_clusters(pred, np.array(topk), np.array(centers, np.float64))
    assert n == len(new_topk)
    rank = {int(label): r for r, label in enumerate(new_topk)}
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return np.array([rank.get(int(new_pred[first[j]]), -1) for j in range(len(counts))], np.int32), [int(t) for t in new_topk]


def main():
    out = {}
    for i, (name, (H, W)) in enumerate(SHAPES.items()):
        normals = normal_map(H, W, 20 + i)
        seeds, labels, centres, n_iter = kmeans_record(normals)
        assert len(np.unique(labels)) == 8
        out.update({f"{name}_normals": normals, f"{name}_seeds": seeds, f"{name}_labels": labels,
                    f"{name}_centres": centres.astype(np.float64), f"{name}_n_iter": np.int32(n_iter)})
        print(name, normals.shape, "n_iter", n_iter, "counts", np.bincount(labels.reshape(-1)))
    names = []
    for name, (counts, topk, centers) in merge_cases().items():
        lut, new_topk = run_merge(counts, topk, centers)
        names.append(name)
        out.update({f"merge_{name}_counts": np.array(counts, np.int64), f"merge_{name}_topk": np.array(topk, np.int32),
                    f"merge_{name}_centres": np.array(centers, np.float64), f"merge_{name}_lut": lut})
        print(name, "topk", topk, "->", new_topk, "lut", lut.tolist())
        if name == "no_merge":
            assert new_topk == topk
        if name == "admits_seventh":
            assert set(new_topk) - set(topk), "the second pick must admit a label outside the first"
    assert len(set(out["merge_chain_lut"].tolist()) - {-1}) == 3
    out["merge_cases"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "plane_masks.npz"), **out)


if __name__ == "__main__":
    main()
