"""Golden vectors of the global-planes stage, produced by RUNNING THE REFERENCE'S OWN CODE on the CPU of the build container:

    global_planes.npz   guidance/cam_utils.py `get_pixel_to_points_tensor` and planes/merge_global_3Dplane.py
                        `get_plane_pnts_idx_from_mask`, `get_global_3Dplane`, `update_global_3Dplane` and
                        `final_merge_global_3Dplane`, imported and called for real, in float32 and in float64.  The import
                        stand-ins are make_golden_visibility._stubs() plus empty `arguments` and `PIL` modules.

Scene.  The five 64 x 48 cameras and unit-sphere depth maps of the visibility golden.  Points: the back-projected clouds of
views 0 .. 3 (12 288 points; the sphere does not occlude a cloud, so far-side and background points share pixels with
near-side ones and the depth test has work to do).  View 4's own cloud is left out.  Masks: the cube-face index (1 .. 6) of
the pixel's surface point, permuted and offset per view so that ids are non-contiguous, 0 on the background; view 4 also
gets a one-pixel plane on a pixel no point projects to (an empty local plane in a later view).

Decisions.  Labels are decisions; torch orders its matmul differently from the contract, so everything is run a second
time in float64, and so is the restatement (tests/planes_ref.py).  The agreed set = the (view, point) pairs on which
ref32 == ref64 and restatement32 == restatement64; it may leave out at most 0.1 % (asserted).  The dicts of the two runs
must be equal (asserted), as must the further properties main() asserts: the depth test rejects at least 5 % somewhere,
merges happen in the update loop and in the final sweep, a later view founds a plane and has an empty one, view 0 has none.

Also recorded: the reference's resume path (dict from views 0 .. 2, then all views) and its update / final merge on
hand-made index sets (a chain, a rate of exactly 0.5, two candidates).

Nothing of the reference is copied: the npz holds inputs and recorded results only.
Run in the build container only (needs /root/reference):  python tests/golden/make_golden_planes.py"""
import copy
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_visibility as mgv  # noqa: E402
from _ref_import import reference_modules  # noqa: E402

W, H = mgv.W, mgv.H
N_CLOUDS = 4
DEPTH_THRESH = 0.01
PERMS = [(0, 1, 2, 3, 4, 5), (3, 0, 5, 1, 4, 2), (5, 4, 3, 2, 1, 0), (1, 2, 0, 4, 5, 3), (2, 5, 1, 0, 3, 4)]
ONE_PIXEL_ID = 977


def cube_face(p):
    """1 .. 6: the face of the cube about the origin that the direction p [..., 3] leaves through."""
    axis = np.abs(p).argmax(-1)
    comp = np.take_along_axis(p, axis[..., None], -1)[..., 0]
    return 2 * axis + (comp < 0) + 1


def make_inputs():
    g = np.load(os.path.join(HERE, "visibility_grid.npz"))
    cams = [types.SimpleNamespace(world_view_transform=g["wvt"][i], full_proj_transform=g["full"][i], FoVx=float(g["fov"][i, 0]),
                                  FoVy=float(g["fov"][i, 1]), image_width=W, image_height=H) for i in range(len(g["wvt"]))]
    depths, clouds = g["depths"], g["clouds"]
    points = np.ascontiguousarray(clouds[:N_CLOUDS].reshape(-1, 3)).astype(np.float32)
    masks = []
    for v in range(len(cams)):
        face = cube_face(clouds[v].reshape(H, W, 3).astype(np.float64))
        ids = 3 * np.asarray(PERMS[v])[face - 1] + 20 * v + 2  # 2, 5, .. 17 in view 0, 22 .. 37 in view 1, ...
        masks.append(np.where(depths[v] < mgv.BACKGROUND, ids, 0).astype(np.int32))
    return cams, points, masks


def paint_empty_plane(cams, points, masks):
    """A one-pixel plane in the last view on a pixel that no candidate point falls into, in float32 and in float64."""
    import planes_ref as pr
    v = len(cams) - 1
    used = np.zeros(H * W, bool)
    for dt in (np.float32, np.float64):
        cand, pix, _z = pr.candidates(points, cams[v], W, H, dt)
        used[pix[cand]] = True
    free = np.nonzero(~used & (masks[v].reshape(-1) == 0))[0]
    assert len(free) > 0
    masks[v].reshape(-1)[free[len(free) // 2]] = ONE_PIXEL_ID


def _stubs():
    stubs = mgv._stubs()
    stubs["arguments"] = types.ModuleType("arguments")
    stubs["arguments"].ModelParams = None
    stubs["PIL"] = types.ModuleType("PIL")
    stubs["PIL"].Image = None
    return stubs


def _plain(d):
    return {int(k): [(int(v), int(p)) for v, p in pairs] for k, pairs in d.items()}


def _sets_as_map(sets):
    """A pixel-to-points tensor [1, n, K] and mask [1, n] from which get_plane_pnts_idx_from_mask reads the given index sets
    (none holds 0) as planes 1 .. n."""
    K = max(len(s) for s in sets)
    m = torch.zeros((1, len(sets), K), dtype=torch.int)
    for k, s in enumerate(sets):
        m[0, k, : len(s)] = torch.tensor(sorted(s), dtype=torch.int)
    return m, torch.arange(1, len(sets) + 1, dtype=torch.int).reshape(1, -1)


HAND_CASES = {
    # C passes only against A ∪ B: the sweep compares with the grown set
    "chain": {"final": [list(range(1, 11)), [6, 7, 8, 9, 10, 11, 12, 13], [1, 11, 12, 13, 14, 15, 16]]},
    # the same sets with C ahead of B: C is compared with A alone and is never looked at again
    "chain_reordered": {"final": [list(range(1, 11)), [1, 11, 12, 13, 14, 15, 16], [6, 7, 8, 9, 10, 11, 12, 13]]},
    # 2 / 4 = 0.5 is not above the threshold
    "exactly_half": {"init": [[1, 2, 3, 4]], "update": [[3, 4, 5, 6]]},
    # both global planes pass; the first one takes the plane
    "first_wins": {"init": [[1, 2, 3, 4], [3, 4, 5, 6, 7, 8]], "update": [[3, 4, 5]]},
}


def run_hand_cases(mg):
    out = {}
    for name, case in HAND_CASES.items():
        if "final" in case:
            sets = [torch.tensor(s, dtype=torch.int64) for s in case["final"]]
            ids = {k: [(k, 1)] for k in range(len(sets))}
        else:
            sets = [torch.tensor(s, dtype=torch.int64) for s in case["init"]]
            ids = {k: [(0, k + 1)] for k in range(len(sets))}
            pmap, mask = _sets_as_map(case["update"])
            sets, ids = mg.update_global_3Dplane(sets, ids, pmap, mask, 1)
        sets, ids = mg.final_merge_global_3Dplane(sets, ids)
        out[name] = {"sets": [sorted(int(i) for i in s) for s in sets],
                     "ids": {str(k): [[int(v), int(p)] for v, p in pairs] for k, pairs in ids.items()}}
    return out


def run_reference(cams, points, masks, double):
    dt = torch.float64 if double else torch.float32
    npdt = np.float64 if double else np.float32
    out = {}
    saved_float, saved_default = torch.Tensor.float, torch.get_default_dtype()
    try:
        if double:
            torch.set_default_dtype(torch.float64)
            torch.Tensor.float = lambda self, *a, **k: self.to(torch.float64)
        with reference_modules(_stubs()):
            sys.path.insert(0, "/root/reference")
            import guidance.cam_utils as cam_utils
            cam_utils.to_tensor_safe = lambda data, dtype=None, device=None: torch.as_tensor(np.asarray(data)).to(dt)
            import planes.merge_global_3Dplane as mg
            ref_cams = []
            for c in cams:
                wvt = np.asarray(c.world_view_transform, npdt)
                ref_cams.append(types.SimpleNamespace(R=wvt[:3, :3].copy(), T=wvt[3, :3].copy(), FoVx=c.FoVx, FoVy=c.FoVy,
                                                      image_width=W, image_height=H))
            pts = torch.tensor(points, dtype=dt)
            tmasks = [torch.tensor(m, dtype=torch.int) for m in masks]
            labels = np.zeros((len(cams), len(points)), np.int32)
            per_pixel = 0
            for v, (cam, mask) in enumerate(zip(ref_cams, tmasks)):
                pmap = cam_utils.get_pixel_to_points_tensor(cam, pts, depth_thresh=DEPTH_THRESH)
                full = cam_utils.get_pixel_to_points_tensor(cam, pts, use_depth_threshold=False)
                per_pixel = max(per_pixel, int(full.shape[-1]))
                for pid in torch.unique(mask):
                    if pid == 0:
                        continue
                    idx = mg.get_plane_pnts_idx_from_mask(pmap, mask, pid).numpy()
                    assert (labels[v, idx] == 0).all()
                    labels[v, idx] = int(pid)
            out["labels"] = labels
            out["per_pixel"] = per_pixel
            idx, ids = mg.get_global_3Dplane(ref_cams, pts, tmasks, None)
            out["idx"], out["ids"] = [i.numpy().astype(np.int64) for i in idx], _plain(ids)
            _i3, ids3 = mg.get_global_3Dplane(ref_cams[:3], pts, tmasks[:3], None)
            out["ids3"] = _plain(ids3)
            idx, ids = mg.get_global_3Dplane(ref_cams, pts, tmasks, copy.deepcopy(out["ids3"]))
            out["resume_idx"], out["resume_ids"] = [i.numpy().astype(np.int64) for i in idx], _plain(ids)
            out["hand"] = run_hand_cases(mg)
    finally:
        torch.Tensor.float = saved_float
        torch.set_default_dtype(saved_default)
    return out


def _json(d):
    return np.array(json.dumps({str(k): [[int(v), int(p)] for v, p in pairs] for k, pairs in d.items()}))


def _ragged(arrays):
    return (np.concatenate(arrays).astype(np.int32) if arrays else np.zeros(0, np.int32),
            np.cumsum([0] + [len(a) for a in arrays]).astype(np.int64))


def main():
    import planes_ref as pr
    cams, points, masks = make_inputs()
    paint_empty_plane(cams, points, masks)
    r32 = run_reference(cams, points, masks, False)
    r64 = run_reference(cams, points, masks, True)
    s32 = np.stack([pr.front_labels(points, c, m, DEPTH_THRESH, np.float32) for c, m in zip(cams, masks)])
    s64 = np.stack([pr.front_labels(points, c, m, DEPTH_THRESH, np.float64) for c, m in zip(cams, masks)])
    ref_differ = r32["labels"] != r64["labels"]
    agreed = ~ref_differ & (s32 == s64)
    excluded = int((~agreed).sum())
    assert excluded <= 0.001 * agreed.size, (excluded, agreed.size)
    assert r32["ids"] == r64["ids"] and r32["resume_ids"] == r64["resume_ids"] and r32["hand"] == r64["hand"]
    assert all(np.array_equal(a, b) for a, b in zip(r32["idx"], r64["idx"]))
    rejected = [pr.depth_rejected(points, c, m, DEPTH_THRESH) for c, m in zip(cams, masks)]
    assert max(r / max(n, 1) for r, n in rejected) >= 0.05, rejected
    stats = {}
    _idx, ids = pr.get_global_3Dplane(points, cams, masks, None, 0.5, DEPTH_THRESH, np.float32, stats)
    assert stats["update_merges"] >= 1 and stats["new_planes"] >= 1 and stats["final_merges"] >= 1, stats
    assert stats["empty_planes"] >= 1, stats
    view0 = pr.all_planes(points, cams[:1], masks[:1], DEPTH_THRESH)[0]
    assert all(len(S) > 0 for _pid, S in view0)  # the reference would raise on an empty global plane
    assert ids == r32["ids"], (ids, r32["ids"])
    flat, offs = _ragged(r32["idx"])
    rflat, roffs = _ragged(r32["resume_idx"])
    out = {"points": points, "masks": np.stack(masks), "depth_thresh": np.float64(DEPTH_THRESH),
           "wvt": np.stack([c.world_view_transform for c in cams]), "full": np.stack([c.full_proj_transform for c in cams]),
           "fov": np.array([[c.FoVx, c.FoVy] for c in cams], np.float64),
           "labels": r32["labels"], "labels_ref64": r64["labels"], "labels_agreed": np.packbits(agreed.reshape(-1)),
           "labels_excluded": np.array([excluded, agreed.size, int(ref_differ.sum())]),
           "ids": _json(r32["ids"]), "idx": flat, "idx_offsets": offs, "ids3": _json(r32["ids3"]),
           "resume_ids": _json(r32["resume_ids"]), "resume_idx": rflat, "resume_idx_offsets": roffs,
           "hand_cases": np.array(json.dumps(HAND_CASES)), "hand_results": np.array(json.dumps(r32["hand"])),
           "stats": np.array(json.dumps(dict(stats, per_pixel=r32["per_pixel"], rejected=rejected)))}
    path = os.path.join(HERE, "global_planes.npz")
    np.savez_compressed(path, **out)
    print(f"wrote global_planes.npz {os.path.getsize(path)} bytes")
    print(f"labels: ref32 != ref64 on {int(ref_differ.sum())}, excluded {excluded} of {agreed.size}; "
          f"restatement32 != ref32 on {int((s32 != r32['labels']).sum())}")
    print(f"{len(r32['ids'])} global planes, {len(r32['ids3'])} after three views; {stats}; at most {r32['per_pixel']} points per "
          f"pixel; depth test rejects {rejected}")
    print(json.dumps(r32["hand"]))


if __name__ == "__main__":
    main()
