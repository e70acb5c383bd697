"""Times the global plane fit (g4splat_amd/plane_fit.py, csrc/tsdf/plane_fit.hip) beside the same loop in the reference's
shape on the same machine -- per (plane, view) pair a copy of the pair's points and normals to the host and sklearn's
KMeans(8), per plane sklearn's RANSACRegressor(max_trials=1000) over an estimator that solves the constrained fit with
scipy's SLSQP from the prior -- at the stage's own size: --views input views (24) of 800 x 600 plus --inpainted inpainted
views (12) of 512 x 512, --planes global planes (36), eight local planes per view less one in 36 (280 pairs).

Scene: every local plane region of a view shows one of the global planes (depth = the ray's hit, noise of sigma 0.004, a
tenth of the pixels off by up to 0.2; normals = the plane's plus noise); where the hit is nearer than 0.5 or beyond 12 the
confident map is off.  The host side is written here; it is neither the code under test nor the reference's files.  The two
sides draw different k-means seeds and samples, so their planes differ as two runs of the reference differ: the largest
angle between the two sides' normals and the largest offset difference at the inliers' centroid are printed, not asserted;
what is asserted is that both sides fit the same planes.  Timing: --warmup warm-up rounds, then --rounds rounds that
alternate the two sides, the device synchronised before each clock reading; medians.  No target is set in advance.

    python tools/bench_plane_fit.py [--rounds 3] [--warmup 1] [--out FILE]
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
from g4splat_amd import _lib, plane_fit, synthetic, visibility  # noqa: E402

DEV = torch.device("cuda:0")
IDS_PER_VIEW = 8


def make_scene(n_input, n_inpainted, n_planes):
    g = torch.Generator(device="cpu").manual_seed(23)
    V = n_input + n_inpainted
    planes = []
    for _ in range(n_planes):
        n = torch.randn(3, generator=g, dtype=torch.float64)
        planes.append((n / n.norm(), 0.5 * torch.randn(3, generator=g, dtype=torch.float64)))
    cams, depths, normals, masks, confs = [], [], [], [], []
    gdict = {k: [] for k in range(n_planes)}
    for v in range(V):
        W, H = (800, 600) if v < n_input else (512, 512)
        a, z = 2.0 * math.pi * v * 0.381966, -1.0 + 2.0 * (v + 0.5) / V
        cam = synthetic.look_at_camera((3.5 * math.cos(a), 3.5 * math.sin(a), z), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), math.radians(55.0), W, H)
        rec = torch.from_numpy(visibility.ray_record(cam, W, H).astype(np.float64))
        o, D = rec[:3], rec[3:].reshape(3, 3)
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        dirs = torch.stack([xs, ys, torch.ones_like(xs)], dim=-1) @ D.T
        ids = [0] + [3 * (v * IDS_PER_VIEW + i) + 2 for i in range(IDS_PER_VIEW)]
        blocks = torch.randint(0, len(ids), (H // 50 + 1, W // 50 + 1), generator=g)
        slot = blocks.repeat_interleave(50, 0).repeat_interleave(50, 1)[:H, :W]
        mask = torch.tensor(ids, dtype=torch.int32)[slot].contiguous()
        depth = torch.full((H, W), 5.0, dtype=torch.float64)
        normal = torch.zeros((H, W, 3), dtype=torch.float64)
        normal[..., 2] = 1.0
        conf = torch.rand((H, W), generator=g) > 0.1
        for i in range(IDS_PER_VIEW):
            if (v * IDS_PER_VIEW + i) % n_planes == 0:
                continue  # listed under no plane
            k = (v * 5 + i * 7) % n_planes
            gdict[k].append((v, ids[i + 1]))
            n, c = planes[k]
            t = torch.dot(n, c - o) / (dirs @ n)
            region = slot == i + 1
            ok = (t > 0.5) & (t < 12.0)
            depth[region] = torch.where(ok, t, torch.full_like(t, 5.0))[region]
            conf &= ~(region & ~ok)
            normal[region] = n  # one side for every view: a wall is seen from one side, and the prior is a mean of normals
        depth += 0.004 * torch.randn((H, W), generator=g, dtype=torch.float64)
        off = torch.rand((H, W), generator=g) < 0.1
        depth[off] += 0.4 * (torch.rand(int(off.sum()), generator=g, dtype=torch.float64) - 0.5)
        normal += 0.05 * torch.randn((H, W, 3), generator=g, dtype=torch.float64)
        normal /= normal.norm(dim=-1, keepdim=True)
        cams.append(cam)
        depths.append(depth.float().to(DEV))
        normals.append(normal.float().to(DEV).contiguous())
        masks.append(mask.to(DEV))
        confs.append(conf.to(DEV))
    return cams, depths, normals, masks, confs, gdict


# ---- the loop in the reference's shape: sklearn and scipy on the host ----------------------------------------------------------
def _estimator_class():
    from scipy.optimize import minimize
    from sklearn.base import BaseEstimator, RegressorMixin

    class SlsqpPlane(RegressorMixin, BaseEstimator):
        def __init__(self, alpha=1.0, prior=None):
            self.alpha, self.prior = alpha, prior

        def fit(self, X, y=None):
            X = np.asarray(X, np.float64)
            prior = np.asarray(self.prior, np.float64)

            def objective(q):
                norm = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
                if norm < 1e-8:
                    return 1e10
                n = q[:3] / norm
                return np.mean((X @ n + q[3] / norm) ** 2) + self.alpha * (1.0 - abs(float(np.dot(prior, n)))) ** 2
            x0 = np.concatenate([prior, [-float(np.dot(prior, X.mean(axis=0)))]])
            res = minimize(objective, x0, method="SLSQP",
                           constraints={"type": "eq", "fun": lambda q: q[0] * q[0] + q[1] * q[1] + q[2] * q[2] - 1.0})
            self.coef_ = res.x if res.success else x0
            return self

        def predict(self, X):
            q = self.coef_ / np.linalg.norm(self.coef_[:3])
            return X[:, 0] * q[0] + X[:, 1] * q[1] + X[:, 2] * q[2] + q[3]

    return SlsqpPlane


def host_fit(cams, depths, normals, masks, confs, gdict):
    from sklearn.cluster import KMeans
    from sklearn.linear_model import RANSACRegressor
    Estimator = _estimator_class()
    points = [visibility.depths_to_points(d, c) for d, c in zip(depths, cams)]
    out = {}
    for key, pairs in gdict.items():
        pnts, priors = [], []
        for v, pid in pairs:
            valid = ((masks[v] == pid) & confs[v]).reshape(-1)
            valid_points = points[v][valid]
            if valid_points.shape[0] < 20:
                continue
            rows = normals[v].reshape(-1, 3)[valid].cpu().numpy()
            km = KMeans(n_clusters=8, random_state=0, n_init=1).fit(rows)
            top = int(np.argmax(np.bincount(km.labels_)))
            pnts.append(valid_points[torch.from_numpy(km.labels_ == top).to(DEV)])
            priors.append(km.cluster_centers_[top] / np.linalg.norm(km.cluster_centers_[top]))
        if not pnts:
            continue
        prior = np.mean(priors, axis=0)
        prior /= np.linalg.norm(prior)
        X = torch.cat(pnts).cpu().numpy()
        ransac = RANSACRegressor(estimator=Estimator(1.0, prior), residual_threshold=0.01, min_samples=3, max_trials=1000,
                                 random_state=42).fit(X, np.zeros(len(X)))
        q = ransac.estimator_.coef_ / np.linalg.norm(ransac.estimator_.coef_[:3])
        out[key] = (q, X[ransac.inlier_mask_].astype(np.float64).mean(axis=0), ransac.n_trials_, len(X))
    return out


def alternate(sides, rounds, warmup):
    times = {n: [] for n in sides}
    for r in range(warmup + rounds):
        for name, fn in sides.items():
            torch.cuda.synchronize(DEV)
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize(DEV)
            ms = (time.perf_counter() - t0) * 1e3
            del out
            print(f"round {r - warmup}: {name} {ms:.1f} ms", flush=True)
            if r >= warmup:
                times[name].append(ms)
    return {n: (statistics.median(times[n]), min(times[n]), max(times[n])) for n in sides}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--inpainted", type=int, default=12)
    ap.add_argument("--planes", type=int, default=36)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    scene = make_scene(a.views, a.inpainted, a.planes)
    cams, depths, normals, masks, confs, gdict = scene
    hip = lambda: plane_fit.fit_global_planes(*scene)  # noqa: E731
    host = lambda: host_fit(*scene)  # noqa: E731
    (planes, info), want = hip(), host()
    assert sorted(planes) == sorted(want), (sorted(planes), sorted(want))
    angle = offset = angle_all = offset_all = 0.0
    settled = 0
    for k, (q, centroid, trials, _n) in want.items():
        n, d = np.asarray(planes[k][0], np.float64), info[k]["d"]
        s = 1.0 if np.dot(n, q[:3]) >= 0 else -1.0
        da = math.degrees(math.acos(min(1.0, s * float(np.dot(n, q[:3])))))
        do = abs(s * (float(np.dot(n, centroid)) + d) - (float(np.dot(q[:3], centroid)) + q[3]))
        angle_all, offset_all = max(angle_all, da), max(offset_all, do)
        if trials < 1000 and info[k]["trials"] < 1000:  # both sides stopped by sklearn's rule: a consensus was found
            settled += 1
            angle, offset = max(angle, da), max(offset, do)
    # the stages of the HIP side, once
    stages = {}
    keys, plane_pair, pair_view, pair_id = plane_fit.pair_table(gdict, len(depths))
    torch.cuda.synchronize(DEV)
    t0 = time.perf_counter()
    pts, nrm, offs, _n = plane_fit._gather(DEV, cams, depths, normals, masks, confs, pair_view, pair_id)
    torch.cuda.synchronize(DEV)
    stages["gather_ms"] = (time.perf_counter() - t0) * 1e3
    N = sum(v["points"] for v in info.values())
    po = [0] + list(np.cumsum([info[k]["points"] for k in sorted(info)]))
    cloud = pts[:N].contiguous()  # any N rows: the kernels' times depend on the sizes alone
    samples = plane_fit.draw_sample_triples([b - c for c, b in zip(po, po[1:])], 1000)
    priors = [info[k]["prior"] for k in sorted(info)]
    for name, fn in (("hypotheses_ms", lambda: plane_fit.plane_hypotheses(cloud, po, samples.to(DEV), priors)),
                     ("score_ms", lambda: plane_fit.score_hypotheses(cloud, po, hyp, 0.01)),
                     ("refit_ms", lambda: plane_fit.refit_planes(cloud, po, hyp, [0] * (len(po) - 1), 0.01, priors))):
        best = math.inf
        for _ in range(3):
            torch.cuda.synchronize(DEV)
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize(DEV)
            best = min(best, (time.perf_counter() - t0) * 1e3)
        if name == "hypotheses_ms":
            hyp = res
        stages[name] = best
    t = alternate({"hip": hip, "host": host}, a.rounds, a.warmup)
    n_pairs = sum(len(p) for p in gdict.values())
    result = {"build_id": _lib.load().g4s_version().decode(), "device": torch.cuda.get_device_name(DEV), "rounds": a.rounds,
              "warmup": a.warmup, "views": len(cams), "pairs": n_pairs, "planes_fitted": len(planes), "gathered_rows": int(pts.shape[0]),
              "plane_points": int(N), "evaluations": int(N) * 1000, "hip_ms": t["hip"][0], "host_ms": t["host"][0],
              "settled_planes": settled, "largest_angle_deg": angle, "largest_offset": offset, "largest_angle_deg_all": angle_all,
              "largest_offset_all": offset_all, "host_trials": [int(w[2]) for w in want.values()],
              "hip_trials": [info[k]["trials"] for k in sorted(info)], **stages}
    text = (f"{result['build_id']} on {result['device']}; medians (min .. max) of {a.rounds} alternating rounds after {a.warmup} warm-ups\n"
            f"plane fit {len(cams)} views, {n_pairs} pairs, {len(planes)} planes, {int(pts.shape[0])} gathered rows, {int(N)} plane points: "
            f"HIP {t['hip'][0]:.1f} ms ({t['hip'][1]:.1f} .. {t['hip'][2]:.1f}) | host (sklearn, scipy) {t['host'][0]:.1f} ms "
            f"({t['host'][1]:.1f} .. {t['host'][2]:.1f}) | x{t['host'][0] / t['hip'][0]:.1f} | over the {settled} planes on which both sides "
            f"stopped before 1000 trials the largest angle between the sides' normals is {angle:.3f} deg and the largest offset "
            f"difference {offset:.2e} (over all planes {angle_all:.3f} deg, {offset_all:.2e})\n"
            f"HIP stages, best of 3: gather {stages['gather_ms']:.2f} ms (first call), hypotheses {stages['hypotheses_ms']:.2f} ms, "
            f"scoring of {int(N) * 1000:.3g} evaluations {stages['score_ms']:.2f} ms, refit {stages['refit_ms']:.2f} ms (each with its "
            f"host checks, upload and synchronisation)")
    print(text)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
