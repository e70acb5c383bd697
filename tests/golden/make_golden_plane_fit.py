"""Golden vectors of the global plane fit, produced by RUNNING THE REFERENCE'S OWN CODE on the CPU of the build container:

    plane_fit.npz   planes/refine_depth_with_planes.py `normals_cluster_1d` and `fit_plane_ransac`, imported and called for real
                    (sklearn's KMeans and RANSACRegressor, scipy's SLSQP underneath), glued in the order of the script's fit
                    loop (lines 547-597).  The import stand-ins are make_golden_depth_cues._stubs().

Scene.  A room corner, the planes x = 0, y = 0 and z = 0 of the positive octant, seen by four 64 x 48 cameras inside the room.
Depth is the ray's hit plus Gaussian noise (sigma 0.005); the rendered normals are the plane's normal plus noise (sigma
0.03).  View 0 holds two blobs inside the wall x = 0: one 0.12 nearer with tilted normals (k-means removes it), one 0.05 nearer
with the wall's normals (RANSAC removes it).  The confident map of view 1 leaves out six columns.  Nineteen pixels of view 3
carry id 99: the pair (3, 99) is listed under plane 12 and alone under plane 13, and is too small to be used.  Plane keys 10,
11, 12 list the three planes' local ids in all four views.

For each plane the reference runs eight times: run 0 on the pairs' valid pixels in raster order, runs 1 .. 7 on seeded
permutations of each pair's pixels.  The order changes which seeds KMeans(random_state=0) picks and which samples
RANSACRegressor(random_state=42) draws, so the spread of the eight results is the reference's own sensitivity to the two
random streams the library replaces.  The yardstick per plane is the largest pairwise difference of the normals' angle and of
the planes' offsets along the normal at a common point (the mean of the eight inlier centroids).

Nothing of the reference is copied: the npz holds inputs and recorded results only.
Run in the build container only (needs /root/reference):  python tests/golden/make_golden_plane_fit.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_depth_cues as mgd  # noqa: E402
import visibility_ref as VR  # noqa: E402
from _ref_import import reference_modules  # noqa: E402
from g4splat_amd.synthetic import look_at_camera  # noqa: E402

W, H = 64, 48
ORDERS = 8
SMALL_ID = 99
EYES = [(2.0, 1.6, 1.2), (1.5, 2.2, 1.0), (2.4, 1.0, 1.5), (1.2, 1.4, 2.2)]
KEYS = (10, 11, 12)


def local_id(view, axis):
    return 1 + (axis + view) % 3 + 3 * view


def make_inputs():
    rng = np.random.default_rng(20260)
    cams = [look_at_camera(e, (0.3, 0.3, 0.3), (0.0, 0.0, 1.0), 1.0, W, H) for e in EYES]
    depths, normals, masks, confs = [], [], [], []
    for v, cam in enumerate(cams):
        o, _D = VR.ray_record(cam, W, H, np.float64)
        dirs = VR.ray_dirs(cam, W, H, np.float64)
        best_t = np.full(H * W, np.inf)
        axis_of = np.full(H * W, -1)
        for a in range(3):
            with np.errstate(divide="ignore", invalid="ignore"):
                t = -o[a] / dirs[:, a]
            hit = o[None] + t[:, None] * dirs
            others = [b for b in range(3) if b != a]
            ok = (t > 0) & np.isfinite(t) & (hit[:, others] >= 0).all(axis=1) & (hit[:, others] <= 3.0).all(axis=1) & (t < best_t)
            best_t[ok], axis_of[ok] = t[ok], a
        depth = np.where(axis_of >= 0, best_t + 0.005 * rng.normal(size=H * W), 5.0)
        nrm = np.zeros((H * W, 3))
        nrm[np.arange(H * W), np.maximum(axis_of, 0)] = 1.0
        nrm = nrm + 0.03 * rng.normal(size=(H * W, 3))
        mask = np.where(axis_of >= 0, 1 + (axis_of + v) % 3 + 3 * v, 0).astype(np.int32)
        conf = np.ones(H * W, bool)
        if v == 0:
            ys, xs = np.divmod(np.arange(H * W), W)
            wall = np.nonzero(axis_of == 0)[0]
            c0, c1 = wall[len(wall) // 3], wall[2 * len(wall) // 3]
            for centre, shift, tilt in ((c0, 0.12, True), (c1, 0.05, False)):
                blob = (axis_of == 0) & ((ys - ys[centre]) ** 2 + (xs - xs[centre]) ** 2 <= 25)
                depth[blob] -= shift
                if tilt:
                    nrm[blob] = np.array([0.6, 0.5, 0.62]) + 0.03 * rng.normal(size=(int(blob.sum()), 3))
        if v == 1:
            conf.reshape(H, W)[:, :6] = False
        if v == 3:
            mask[:19] = SMALL_ID
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        depths.append(depth.reshape(H, W).astype(np.float32))
        normals.append(nrm.reshape(H, W, 3).astype(np.float32))
        masks.append(mask.reshape(H, W))
        confs.append(conf.reshape(H, W))
    gdict = {KEYS[a]: [(v, local_id(v, a)) for v in range(len(cams))] for a in range(3)}
    gdict[12].append((3, SMALL_ID))
    gdict[13] = [(3, SMALL_ID)]
    return cams, depths, normals, masks, confs, gdict


def run_reference(inputs):
    cams, depths, normals, masks, confs, gdict = inputs
    points = [VR.depths_to_points(d, c) for d, c in zip(depths, cams)]
    out = {}
    with reference_modules(mgd._stubs()):
        sys.path.insert(0, "/root/reference")
        from planes.refine_depth_with_planes import fit_plane_ransac, normals_cluster_1d
        for key, pairs in gdict.items():
            runs = []
            for order in range(ORDERS):
                rng = np.random.default_rng(1000 * key + order)
                pnts, priors = [], []
                for view_id, plane_id in pairs:  # lines 554-585
                    valid = ((masks[view_id] == plane_id) & confs[view_id]).reshape(-1)
                    valid_points = points[view_id][valid]
                    if valid_points.shape[0] < 20:
                        continue
                    valid_normals = normals[view_id].reshape(-1, 3)[valid]
                    if order:
                        perm = rng.permutation(len(valid_points))
                        valid_points, valid_normals = valid_points[perm], valid_normals[perm]
                    cluster_masks, cluster_centers = normals_cluster_1d(valid_normals)
                    pnts.append(valid_points[cluster_masks[0]])
                    priors.append(cluster_centers[0])
                if not pnts:
                    break
                prior = np.stack(priors, axis=0).mean(axis=0)
                prior = prior / np.linalg.norm(prior)
                pnts = np.concatenate(pnts, axis=0)
                normal, centre, inliers = fit_plane_ransac(pnts, prior_normal=prior)
                runs.append({"normal": np.asarray(normal, np.float64), "centre": np.asarray(centre, np.float64), "prior": prior,
                             "points": pnts, "inliers": np.asarray(inliers, bool),
                             "centroid": pnts[np.asarray(inliers, bool)].astype(np.float64).mean(axis=0)})
            if runs:
                out[key] = runs
    return out


def yardstick(runs):
    """(largest pairwise angle in radians, largest pairwise offset difference at the common point)."""
    common = np.mean([r["centroid"] for r in runs], axis=0)
    normals = [r["normal"] * (1.0 if np.dot(r["normal"], runs[0]["normal"]) >= 0 else -1.0) for r in runs]
    offs = [float(np.dot(n, common - r["centre"])) for n, r in zip(normals, runs)]
    angle = max(float(np.arccos(min(1.0, np.dot(a, b)))) for a in normals for b in normals)
    return angle, max(abs(a - b) for a in offs for b in offs), common


def main():
    inputs = make_inputs()
    cams, depths, normals, masks, confs, gdict = inputs
    ref = run_reference(inputs)
    assert sorted(ref) == list(KEYS), sorted(ref)
    small = int(((masks[3] == SMALL_ID) & confs[3]).sum())
    assert small == 19, small
    out = {"wvt": np.stack([c.world_view_transform for c in cams]), "full": np.stack([c.full_proj_transform for c in cams]),
           "fov": np.array([[c.FoVx, c.FoVy] for c in cams], np.float64), "depths": np.stack(depths), "normals": np.stack(normals),
           "masks": np.stack(masks), "confs": np.stack(confs),
           "gdict": np.array(json.dumps({str(k): [[int(v), int(p)] for v, p in pairs] for k, pairs in gdict.items()})),
           "keys": np.array(KEYS, np.int64)}
    for key in KEYS:
        runs = ref[key]
        angle, offset, common = yardstick(runs)
        assert angle > 0 and offset > 0
        share = [float(r["inliers"].mean()) for r in runs]
        assert min(share) < 0.995 and min(share) > 0.5, share  # the blob and the noise tail are outside
        out[f"ref_normal_{key}"] = np.stack([r["normal"] for r in runs])
        out[f"ref_centre_{key}"] = np.stack([r["centre"] for r in runs])
        out[f"ref_centroid_{key}"] = np.stack([r["centroid"] for r in runs])
        out[f"ref_inliers_{key}"] = np.array([int(r["inliers"].sum()) for r in runs], np.int64)
        out[f"ref_count_{key}"] = np.array([len(r["points"]) for r in runs], np.int64)
        out[f"ref_points_{key}"] = runs[0]["points"].astype(np.float32)  # run 0: the raster order
        out[f"ref_prior_{key}"] = runs[0]["prior"]
        out[f"ref_mask_{key}"] = runs[0]["inliers"]
        out[f"common_{key}"] = common
        out[f"yardstick_{key}"] = np.array([angle, offset], np.float64)
        print(key, "points", [len(r["points"]) for r in runs], "inlier share", np.round(share, 3), "yardstick", angle, offset)
    path = os.path.join(HERE, "plane_fit.npz")
    np.savez_compressed(path, **out)
    print(f"wrote plane_fit.npz {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
