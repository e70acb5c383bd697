"""Golden vectors for the mip filter, produced by RUNNING THE REFERENCE'S OWN `GaussianModel`
(2d-gaussian-splatting/scene/gaussian_model.py) on the CPU of the build container:

    mip_filter.npz   (a) compute_mip_filter (:388-434) for 300 points and 5 cameras of differing focal lengths and image
                         sizes: a cluster every camera sees, a wide box (points behind cameras, outside the 15 %
                         border, seen by one view only, seen by nobody) and far points;
                     (b) get_scaling / get_opacity (:157-192) with that filter on, and the gradients of
                         sum(get_scaling * c_s) + sum(get_opacity * c_o) with respect to _scaling and _opacity under fixed
                         random cotangents.

The script refuses to write a fixture in which any (point, view) pair lies within a relative 1e-4 of a decision
threshold (z against znear, u and v against the four borders): then no case has to be left out of a comparison, and a
one-ulp difference between the reference's GEMM and a spelled-out sum cannot flip a decision.
Run where the reference checkout that _ref_import.py points at exists:  python tests/golden/make_golden_mip.py"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import reference_modules  # noqa: E402

ZNEAR, VARIANCE = 0.2, 0.2
# (focal_x, focal_y, width, height, eye)
VIEWS = [(420.0, 415.0, 640, 480, (0.3, -0.2, -3.6)), (310.5, 322.25, 400, 300, (3.1, 0.4, -1.2)),
         (800.0, 790.0, 1200, 680, (-2.4, 1.1, 2.9)), (151.0, 149.5, 160, 120, (0.2, 3.3, 0.6)),
         (505.0, 512.0, 512, 512, (-3.0, -0.8, -1.5))]


def look_at(eye, target=(0.0, 0.0, 0.0)):
    """(R, T) as the reference's cameras hold them: camera space = xyz @ R + T."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(np.array([0.0, 1.0, 0.1]), fwd)
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    w2c = np.stack([right, up, fwd])  # rows: the camera's axes
    return w2c.T.astype(np.float32), (-w2c @ eye).astype(np.float32)


def make_inputs():
    rng = np.random.default_rng(20251019)
    xyz = np.concatenate([rng.normal(0, 0.7, (180, 3)), rng.uniform(-6, 6, (90, 3)),
                          rng.normal(0, 1, (30, 3)) * 40.0]).astype(np.float32)
    P = xyz.shape[0]
    cams = []
    for fx, fy, w, h, eye in VIEWS:
        R, T = look_at(eye)
        cams.append(types.SimpleNamespace(R=R, T=T, focal_x=fx, focal_y=fy, image_width=w, image_height=h))
    return dict(xyz=xyz, cams=cams,
                scaling=rng.uniform(np.log(3e-4), np.log(0.05), (P, 2)).astype(np.float32),
                opacity=rng.normal(0, 2.0, (P, 1)).astype(np.float32),
                cot_scaling=rng.uniform(0.5, 1.5, (P, 2)).astype(np.float32),
                cot_opacity=rng.uniform(0.5, 1.5, (P, 1)).astype(np.float32))


def check_margins(xyz, cams):
    """No decision within a relative 1e-4 of its threshold (float64).  Returns per-view (valid depth, in screen)."""
    x = xyz.astype(np.float64)
    depth_ok, screen_ok = [], []
    for c in cams:
        pc = x @ c.R.astype(np.float64) + c.T.astype(np.float64)
        z = pc[:, 2]
        assert (np.abs(z - ZNEAR) > 1e-4 * ZNEAR).all(), "a depth too close to znear"
        zc = np.maximum(z, 0.001)
        u = pc[:, 0] / zc * c.focal_x + c.image_width / 2.0
        v = pc[:, 1] / zc * c.focal_y + c.image_height / 2.0
        live = z > ZNEAR  # (the borders decide nothing for a point the depth test already drops)
        for val, size in ((u, c.image_width), (v, c.image_height)):
            for thr in (-0.15 * size, 1.15 * size):
                assert (np.abs(val - thr)[live] > 1e-4 * abs(thr)).all(), "a projection too close to a border"
        depth_ok.append(live)
        screen_ok.append((u >= -0.15 * c.image_width) & (u <= 1.15 * c.image_width) &
                         (v >= -0.15 * c.image_height) & (v <= 1.15 * c.image_height))
    return np.stack(depth_ok), np.stack(screen_ok)


def main():
    inp = make_inputs()
    depth_ok, screen_ok = check_margins(inp["xyz"], inp["cams"])
    seen_by = (depth_ok & screen_ok).sum(axis=0)
    cover = dict(behind=int((~depth_ok).any(axis=0).sum()), outside=int((depth_ok & ~screen_ok).any(axis=0).sum()),
                 nobody=int((seen_by == 0).sum()), one_view=int((seen_by == 1).sum()), all_views=int((seen_by == 5).sum()))
    assert min(cover.values()) >= 5, cover
    out = {}
    with reference_modules():
        from scene.gaussian_model import GaussianModel
        gm = GaussianModel(3)
        gm._xyz = torch.nn.Parameter(torch.tensor(inp["xyz"]))
        gm._scaling = torch.nn.Parameter(torch.tensor(inp["scaling"]))
        gm._opacity = torch.nn.Parameter(torch.tensor(inp["opacity"]))
        gm.set_mip_filter(True)
        gm.compute_mip_filter(inp["cams"], znear=ZNEAR, filter_variance=VARIANCE)
        out["mip_filter"] = gm.mip_filter.detach().numpy().copy()
        scales, opac = gm.get_scaling, gm.get_opacity
        ((scales * torch.tensor(inp["cot_scaling"])).sum() + (opac * torch.tensor(inp["cot_opacity"])).sum()).backward()
        out["scales"], out["opacities"] = scales.detach().numpy().copy(), opac.detach().numpy().copy()
        out["grad_scaling"], out["grad_opacity"] = gm._scaling.grad.numpy().copy(), gm._opacity.grad.numpy().copy()
    assert out["mip_filter"].shape == (inp["xyz"].shape[0], 1) and out["mip_filter"].dtype == np.float32
    for k in ("xyz", "scaling", "opacity", "cot_scaling", "cot_opacity"):
        out["in_" + k] = inp[k]
    out["in_R"] = np.stack([c.R for c in inp["cams"]])
    out["in_T"] = np.stack([c.T for c in inp["cams"]])
    out["in_intrinsics"] = np.array([[c.focal_x, c.focal_y, c.image_width, c.image_height] for c in inp["cams"]], np.float64)
    out["in_znear"], out["in_filter_variance"] = np.float64(ZNEAR), np.float64(VARIANCE)
    out["seen_by"] = seen_by.astype(np.int32)
    path = os.path.join(HERE, "mip_filter.npz")
    np.savez_compressed(path, **out)
    print("wrote mip_filter.npz", os.path.getsize(path), cover)


if __name__ == "__main__":
    main()
