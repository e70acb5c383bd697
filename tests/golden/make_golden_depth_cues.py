"""Golden vectors of the depth-cue stage, produced by RUNNING THE REFERENCE'S OWN CODE on the CPU of the build container:

    depth_cues.npz   matcha/pointmap/depthanythingv2.py `depth_linear_align` and `depth_linear_align_2`, utils/point_utils.py
                     `depth_to_normal` (over `depths_to_points`) and planes/refine_depth_with_planes.py
                     `compute_plane_aligned_depth`, imported and called for real, in float32 and in float64, glued in the
                     order of guidance/see3d_dn_util.py's loop body and of the paste and refill loops of
                     refine_depth_with_planes.py.  The import stand-ins are make_golden_planes._stubs() plus empty modules
                     for what depthanythingv2.py and the planes script import without using on these paths (pytorch3d,
                     depth_anything_v2, mast3r, the point-map base classes, render_utils, charts).

Scene.  The five 64 x 48 cameras and unit-sphere depth maps of the visibility golden, the last two views treated as
inpainted (n_input_views = 3).  The mono disparity is an affine map of the true disparity plus a smooth perturbation
(about 0.3 .. 0.9); the alpha maps keep 1e-3 away from 0.9; the plane masks are the cube-face ids of
make_golden_planes.py plus a 3 x 3 patch of id 977 in view 4.  Fitted planes: the six cube faces, slightly tilted, under
keys 0 .. 5, each listed by the views that do not look along it; key 6, a plane through view 1's x axis whose horizon runs
between two pixel rows, lists a pair of view 1 that a face key lists as well (the later key wins); key 7 lists (4, 977) and has no fitted plane.  The confident maps of the inpainted views leave out
every pixel whose plane intersection is invalid (the reference divides by such a depth and returns NaN coefficients).

main() asserts its own coverage: at least 1 % of some view's masked pixels get the 0 of an invalid intersection, the refill
region of both inpainted views is non-empty, the duplicate pair resolves to the later plane, and the float32 and float64
runs take the same validity decision on all but at most 0.1 % of the masked pixels (those are recorded as left out).
Per float output it records the largest |float32 run - float64 run| over the compared pixels: the reference's own
rounding noise, the yardstick of tests/test_depth_cues_cpu.py and tests/test_gpu_depth_cues.py.

Nothing of the reference is copied: the npz holds inputs and recorded results only.
Run in the build container only (needs /root/reference):  python tests/golden/make_golden_depth_cues.py"""
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
import make_golden_planes as mgp  # noqa: E402
import make_golden_visibility as mgv  # noqa: E402
from _ref_import import reference_modules  # noqa: E402

W, H = mgv.W, mgv.H
N_INPUT = 3
THRESHOLD = 0.9
PATCH_ID = 977
HORIZON_VIEW = 1


def _smooth(v, fx, fy, phase):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.sin(fx * x / W * 2 * np.pi + phase + v) * np.cos(fy * y / H * 2 * np.pi - 0.5 * v)


def make_inputs():
    import depth_cues_ref as dr
    cams, _points, masks = mgp.make_inputs()
    g = np.load(os.path.join(HERE, "visibility_grid.npz"))
    depths = g["depths"].astype(np.float32)
    V = len(cams)
    surface = depths < mgv.BACKGROUND
    masks = [m.copy() for m in masks]
    ys, xs = np.nonzero(~surface[4])
    y0, x0 = int(ys[0]), int(xs[0])
    assert not surface[4][y0:y0 + 3, x0:x0 + 3].any()
    masks[4][y0:y0 + 3, x0:x0 + 3] = PATCH_ID
    disps, alphas = [], []
    for v in range(V):
        true_disp = 1.0 / depths[v].astype(np.float64)
        disps.append((1.6 * true_disp + 0.05 + 0.03 * _smooth(v, 2, 1, 0.3)).astype(np.float32))
        seen = _smooth(v, 1, 1, 1.0) > -0.2
        alphas.append(np.where(seen, 0.95 + 0.04 * _smooth(v, 3, 2, 0.0), 0.45 + 0.4 * _smooth(v, 2, 3, 2.0)).astype(np.float32))
        assert np.abs(alphas[-1] - 0.9).min() > 1e-3
    # the face id of view v for cube face f (1 .. 6), as make_golden_planes numbers them
    face_id = lambda v, f: 3 * mgp.PERMS[v][f - 1] + 20 * v + 2  # noqa: E731
    planes, gdict = {}, {}
    tilt = [(0.03, -0.02), (-0.02, 0.04), (0.05, 0.01), (0.01, -0.03), (-0.04, 0.02), (0.02, 0.03)]
    for f in range(1, 7):
        axis, sign = (f - 1) // 2, 1.0 - 2.0 * ((f - 1) % 2)
        n = np.zeros(3)
        n[axis] = sign
        n[(axis + 1) % 3], n[(axis + 2) % 3] = tilt[f - 1]
        n /= np.linalg.norm(n)
        c = np.zeros(3)
        c[axis] = 0.8 * sign
        planes[f - 1] = (n.astype(np.float32), c.astype(np.float32))
        # a view lists the face unless it looks along the plane: there the intersections run to hundreds of units or behind
        # the camera, and the reference's float32 noise at such a pixel would be the yardstick of every other pixel
        gdict[f - 1] = []
        for v in range(V):
            region = masks[v] == face_id(v, f)
            z, valid = dr.plane_depth_image(planes[f - 1][0], planes[f - 1][1], cams[v], H, W, np.float64)
            if region.any() and valid[region].all() and z[region].max() < 20.0:
                gdict[f - 1].append((v, int(face_id(v, f))))
    # the plane that crosses view 1's horizon, pasted over the face of view 1 with the most pixels
    c2w = np.linalg.inv(np.asarray(cams[HORIZON_VIEW].world_view_transform, np.float64)).T
    o, R = c2w[:3, 3], c2w[:3, :3]
    counts = {int(p): int((masks[HORIZON_VIEW] == p).sum()) for p in np.unique(masks[HORIZON_VIEW]) if p}
    dup_id = max(counts, key=counts.get)
    # it holds the camera's x axis and lies 0.3 below the camera; its horizon runs half-way between rows H/2 and H/2 + 1
    phi = -np.arctan(0.5 / (H / (2.0 * np.tan(cams[HORIZON_VIEW].FoVy / 2.0))))
    planes[6] = ((R @ np.array([0.0, np.cos(phi), np.sin(phi)])).astype(np.float32), (o + R @ np.array([0.0, 0.3, 0.0])).astype(np.float32))
    gdict[6] = [(HORIZON_VIEW, dup_id)]
    gdict[7] = [(4, PATCH_ID)]  # never fitted
    monos = [(np.float32(1) / d).astype(np.float32) for d in disps]
    # confident maps: true on the input views; on the inpainted ones a part of the image, minus invalid intersections
    confs = []
    for v in range(V):
        if v < N_INPUT:
            confs.append(np.ones((H, W), bool))
            continue
        conf = _smooth(v, 1, 2, 0.7) > -0.3  # surface and background: both ends of the disparity range anchor the fit
        for dt in (np.float32, np.float64):
            _o, _r, _z, touched, valid = dr.apply_global_planes(cams, list(depths), masks, gdict, planes, dt)
            conf &= ~(touched[v] & ~valid[v])
        confs.append(conf)
    return cams, depths, masks, disps, alphas, monos, confs, gdict, planes, dup_id


def _stubs():
    def module(name, **names):
        m = types.ModuleType(name)
        for k, v in names.items():
            setattr(m, k, v)
        return m

    stubs = mgp._stubs()
    p3d = stubs["pytorch3d"]
    p3d.structures = module("pytorch3d.structures", Pointclouds=None)
    p3d.renderer = module("pytorch3d.renderer", PointsRasterizationSettings=None, PointsRasterizer=None)
    da = module("depth_anything_v2")
    da.dpt = module("depth_anything_v2.dpt", DepthAnythingV2=None)
    stubs.update({
        "pytorch3d.structures": p3d.structures, "pytorch3d.renderer": p3d.renderer,
        "depth_anything_v2": da, "depth_anything_v2.dpt": da.dpt,
        "matcha.pointmap.base": module("matcha.pointmap.base", PointMap=object),
        "matcha.pointmap.utils": module("matcha.pointmap.utils", load_colmap_scene=None),
        "matcha.pointmap.dust3r": module("matcha.pointmap.dust3r", compute_dust3r_scene=None),
        "matcha.pointmap.mast3r": module("matcha.pointmap.mast3r", compute_mast3r_scene=None),
        "matcha.dm_scene.cameras": module("matcha.dm_scene.cameras", GSCamera=object, CamerasWrapper=object, P3DCameras=object),
        "matcha.dm_utils.rendering": module("matcha.dm_utils.rendering", fov2focal=None, depth2normal_parallel=None,
                                            normal2curv_parallel=None),
        "matcha.dm_scene.charts": module("matcha.dm_scene.charts", depths_to_points_parallel=None),
        "utils.render_utils": module("utils.render_utils", save_img_f32=None, save_img_u8=None),
    })
    return stubs


def run_reference(inputs, double):
    cams, depths, masks, disps, alphas, monos, confs, gdict, planes, _dup = inputs
    dt = torch.float64 if double else torch.float32
    out = {}
    saved_float, saved_default = torch.Tensor.float, torch.get_default_dtype()
    try:
        if double:
            torch.set_default_dtype(torch.float64)
            torch.Tensor.float = lambda self, *a, **k: self.to(torch.float64)
        with reference_modules(_stubs()):
            sys.path.insert(0, "/root/reference")
            from matcha.pointmap.depthanythingv2 import depth_linear_align, depth_linear_align_2
            from utils.point_utils import depth_to_normal
            from planes.refine_depth_with_planes import compute_plane_aligned_depth
            V = len(cams)
            ref_cams = []
            for c in cams:
                fx = W / (2.0 * np.tan(c.FoVx / 2.0))
                fy = H / (2.0 * np.tan(c.FoVy / 2.0))
                ref_cams.append(types.SimpleNamespace(
                    world_view_transform=torch.tensor(np.asarray(c.world_view_transform, np.float64), dtype=dt),
                    full_proj_transform=torch.tensor(np.asarray(c.full_proj_transform, np.float64), dtype=dt),
                    image_width=W, image_height=H, focal_x=fx, focal_y=fy))
            T = lambda a: torch.tensor(np.asarray(a), dtype=dt)  # noqa: E731
            # ---- the loop body of guidance/see3d_dn_util.py, every view
            cue = {k: [] for k in ("aligned_depth", "normal_world", "normal_cam", "depth", "coeffs", "align2", "coeffs2")}
            for v in range(V):
                disp, warp = T(disps[v]), T(depths[v])
                visible = torch.tensor(alphas[v]) > THRESHOLD
                aligned, alpha, beta = depth_linear_align(disp=disp, render_depth=warp, visible_mask=visible, return_alpha_beta=True)
                normal = depth_to_normal(ref_cams[v], aligned.unsqueeze(0))
                normal_cam = normal @ ref_cams[v].world_view_transform[:3, :3]
                merged = aligned.clone()
                merged[visible] = warp[visible]
                a2, alpha2, beta2 = depth_linear_align_2(depth=T(monos[v]), render_depth=warp, visible_mask=visible,
                                                          return_alpha_beta=True)
                for k, x in (("aligned_depth", aligned), ("normal_world", normal), ("normal_cam", normal_cam), ("depth", merged),
                             ("align2", a2)):
                    cue[k].append(x.numpy().astype(np.float64))
                cue["coeffs"].append([alpha, beta])
                cue["coeffs2"].append([alpha2, beta2])
            out.update({k: np.array(x, np.float64) for k, x in cue.items()})
            # ---- one whole image against one plane
            full, ok = [], []
            for key, v in ((0, 0), (6, HORIZON_VIEW), (3, 4)):
                d, _pts = compute_plane_aligned_depth(T(planes[key][0]), T(planes[key][1]), ref_cams[v], (H, W))
                full.append(d.numpy().astype(np.float64))
                ok.append(d.numpy() > 0)
            out["plane_full"], out["plane_full_valid"] = np.array(full), np.array(ok)
            # ---- the paste loop of planes/refine_depth_with_planes.py, in dict order, then its refill loop
            depth_list = [T(d).clone() for d in depths]
            touched = [np.zeros((H, W), bool) for _ in range(V)]
            valid = [np.zeros((H, W), bool) for _ in range(V)]
            winner = [np.full((H, W), -1, np.int32) for _ in range(V)]
            for key, pairs in gdict.items():
                if key not in planes:
                    continue
                for view_id, plane_id in pairs:
                    mask = masks[view_id] == plane_id
                    d, _pts = compute_plane_aligned_depth(T(planes[key][0]), T(planes[key][1]), ref_cams[view_id], (H, W))
                    tmask = torch.from_numpy(mask)
                    depth_list[view_id][tmask] = d[tmask]
                    touched[view_id] |= mask
                    valid[view_id][mask] = (d.numpy() > 0)[mask]
                    winner[view_id][mask] = key
            out["planed"] = np.array([d.numpy().astype(np.float64) for d in depth_list])
            coeffs = np.zeros((V, 2))
            for v in range(N_INPUT, V):
                conf = torch.from_numpy(confs[v])
                mono_disp = 1. / T(monos[v])
                fitted, alpha, beta = depth_linear_align(disp=mono_disp, render_depth=depth_list[v], visible_mask=conf,
                                                         return_alpha_beta=True)
                replace = ~torch.from_numpy(masks[v] > 0.5) & ~conf
                depth_list[v][replace] = fitted[replace]
                coeffs[v] = [alpha, beta]
            out["refined"] = np.array([d.numpy().astype(np.float64) for d in depth_list])
            out["refill_coeffs"] = coeffs
            out["touched"], out["valid"], out["winner"] = np.array(touched), np.array(valid), np.array(winner)
    finally:
        torch.Tensor.float = saved_float
        torch.set_default_dtype(saved_default)
    return out


FLOAT_OUTPUTS = ("aligned_depth", "normal_world", "normal_cam", "depth", "coeffs", "align2", "coeffs2", "plane_full", "planed",
                 "refined", "refill_coeffs")


def main():
    inputs = make_inputs()
    cams, depths, masks, disps, alphas, monos, confs, gdict, planes, dup_id = inputs
    V = len(cams)
    r32, r64 = run_reference(inputs, False), run_reference(inputs, True)
    assert np.isfinite(r32["coeffs"]).all() and np.isfinite(r32["refill_coeffs"]).all() and np.isfinite(r64["refill_coeffs"]).all()
    assert np.array_equal(r32["touched"], r64["touched"]) and np.array_equal(r32["winner"], r64["winner"])
    # coverage
    zero_share = [float((r64["touched"][v] & ~r64["valid"][v]).sum()) / max(int(r64["touched"][v].sum()), 1) for v in range(V)]
    assert max(zero_share) >= 0.01, zero_share
    refill_region = [int(((masks[v] == 0) & ~confs[v]).sum()) for v in range(N_INPUT, V)]
    assert min(refill_region) > 0, refill_region
    dup = masks[HORIZON_VIEW] == dup_id
    assert sum((HORIZON_VIEW, dup_id) in [tuple(p) for p in pairs] for pairs in gdict.values()) == 2
    assert dup.any() and (r64["winner"][HORIZON_VIEW][dup] == 6).all()
    assert (r64["winner"][4][masks[4] == PATCH_ID] == -1).all() and not r64["touched"][4][masks[4] == PATCH_ID].any()
    # the compared set: the masked pixels on which both runs take the same validity decision
    agreed = r32["valid"] == r64["valid"]
    excluded = int((r64["touched"] & ~agreed).sum())
    assert excluded <= 0.001 * int(r64["touched"].sum()), (excluded, int(r64["touched"].sum()))
    full_agreed = r32["plane_full_valid"] == r64["plane_full_valid"]
    assert int((~full_agreed).sum()) <= 0.001 * full_agreed.size
    yard = {}
    for k in FLOAT_OUTPUTS:
        a, b = r32[k], r64[k]
        keep = np.ones(a.shape, bool)
        if k in ("planed", "refined"):
            keep = agreed
        if k == "plane_full":
            keep = full_agreed
        yard[k] = float(np.abs(a - b)[keep].max())
    out = {"wvt": np.stack([c.world_view_transform for c in cams]), "full": np.stack([c.full_proj_transform for c in cams]),
           "fov": np.array([[c.FoVx, c.FoVy] for c in cams], np.float64), "n_input": np.int64(N_INPUT),
           "threshold": np.float64(THRESHOLD), "depths": depths, "masks": np.stack(masks), "disps": np.stack(disps),
           "alphas": np.stack(alphas), "confs": np.stack(confs),
           "gdict": np.array(json.dumps({str(k): [[int(v), int(p)] for v, p in pairs] for k, pairs in gdict.items()})),
           "plane_keys": np.array(sorted(planes), np.int64),
           "plane_rows": np.stack([np.concatenate(planes[k]) for k in sorted(planes)]).astype(np.float32),
           "plane_full_pairs": np.array([[0, 0], [6, HORIZON_VIEW], [3, 4]], np.int64),
           "dup_pair": np.array([HORIZON_VIEW, dup_id], np.int64), "agreed": agreed, "full_agreed": full_agreed,
           "excluded": np.array([excluded, int(r64["touched"].sum())], np.int64),
           "touched": r64["touched"], "valid": r64["valid"], "winner": r64["winner"],
           "plane_full_valid": r64["plane_full_valid"],
           "yardstick": np.array(json.dumps(yard))}
    # the normals and the depth-domain alignment are kept for the inpainted views (the views the reference's loop runs on);
    # the merged depth is the rendered depth where visible and aligned_depth elsewhere, exactly, and is not stored
    for k in FLOAT_OUTPUTS:
        if k != "depth":
            out["ref64_" + k] = r64[k][N_INPUT:] if k in ("normal_world", "normal_cam", "align2") else r64[k]
    path = os.path.join(HERE, "depth_cues.npz")
    np.savez_compressed(path, **out)
    print(f"wrote depth_cues.npz {os.path.getsize(path)} bytes")
    print(f"zero share per view {zero_share}; refill region {refill_region}; excluded {excluded}")
    print(json.dumps(yard, indent=1))


if __name__ == "__main__":
    main()
