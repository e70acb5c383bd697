"""The small scenes that more than one test file renders: the cameras, models, loss and map inputs of the render(), training,
mip-filter and render-maps tests.  A plain module like tests/knn_clouds.py; nothing here touches a GPU unless asked to."""
from types import SimpleNamespace

import numpy as np
import torch

from g4splat_amd import synthetic
from g4splat_amd.gaussian_model import GaussianModel

RENDER_KEYS = {"render", "viewspace_points", "visibility_filter", "radii", "rend_alpha", "rend_normal", "rend_normal_cam",
        "rend_dist", "surf_depth", "surf_normal", "surf_normal_cam", "rend_depth"}
MAP_NAMES = ("rend_alpha", "rend_normal", "rend_normal_cam", "rend_depth", "rend_dist", "surf_depth", "surf_normal",
         "surf_normal_cam")
TRAIN_W, TRAIN_H, TRAIN_P = 96, 64, 400


def render_camera(W=80, H=56):
    cam = synthetic.look_at_camera((0.3, -0.2, -3.0), (0, 0, 0), (0, 1, 0), 1.0, W, H)
    return SimpleNamespace(image_width=W, image_height=H, FoVx=cam.FoVx, FoVy=cam.FoVy,
                           world_view_transform=torch.tensor(cam.world_view_transform),
                           full_proj_transform=torch.tensor(cam.full_proj_transform),
                           camera_center=torch.tensor(cam.camera_center), znear=0.01, zfar=100.0)


def render_model(P=300, seed=0):
    rng = np.random.default_rng(seed)
    m = GaussianModel(sh_degree=3)
    pts = torch.tensor(rng.uniform(-1, 1, (P, 3)).astype(np.float32))
    m.create_from_parameters(pts, torch.tensor(rng.uniform(0.05, 0.2, (P, 2)).astype(np.float32)),
                             torch.tensor(rng.normal(size=(P, 4)).astype(np.float32)),
                             torch.tensor(rng.uniform(0, 1, (P, 3)).astype(np.float32)))
    with torch.no_grad():
        m._opacity += 2.0
    m.active_sh_degree = 1
    return m


def render_loss(out):
    return (out["render"] ** 2).mean() + out["rend_dist"].mean() + (1 - (out["rend_normal"] * out["surf_normal"]).sum(0)).mean() \
        + 0.1 * out["surf_depth"].mean()


def train_cams(dev):
    out = []
    for i in range(4):
        a = 0.6 * i - 0.9
        cam = synthetic.look_at_camera((2.6 * np.sin(a), 0.3 * (i - 1.5), -2.6 * np.cos(a)), (0, 0, 0), (0, 1, 0), 1.0, TRAIN_W, TRAIN_H)
        out.append(SimpleNamespace(image_width=TRAIN_W, image_height=TRAIN_H, FoVx=cam.FoVx, FoVy=cam.FoVy,
                                   world_view_transform=torch.tensor(cam.world_view_transform, device=dev),
                                   full_proj_transform=torch.tensor(cam.full_proj_transform, device=dev),
                                   camera_center=torch.tensor(cam.camera_center, device=dev), znear=0.01, zfar=100.0))
    return out


def train_model(seed, dev, jitter):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-0.9, 0.9, (TRAIN_P, 3)).astype(np.float32)
    cols = rng.uniform(0, 1, (TRAIN_P, 3)).astype(np.float32)
    sc = rng.uniform(0.06, 0.2, (TRAIN_P, 2)).astype(np.float32)
    rot = rng.normal(size=(TRAIN_P, 4)).astype(np.float32)
    if jitter:  # the trainee starts away from the scene that produced the targets
        j = np.random.default_rng(seed + 1)
        pts = pts + j.normal(0, 0.03, pts.shape).astype(np.float32)
        cols = np.clip(cols + j.normal(0, 0.2, cols.shape), 0, 1).astype(np.float32)
        sc = sc * j.uniform(0.7, 1.3, sc.shape).astype(np.float32)
    m = GaussianModel(sh_degree=3)
    t = lambda a: torch.tensor(a, device=dev)
    m.create_from_parameters(t(pts), t(sc), t(rot), t(cols))
    with torch.no_grad():
        m._opacity += 2.5
    m.active_sh_degree = 1
    return m


def maps_camera(W, H, eye=(0.3, -0.2, -3.0), dev="cpu"):
    cam = synthetic.look_at_camera(eye, (0, 0, 0), (0, 1, 0), 1.0, W, H)
    return SimpleNamespace(image_width=W, image_height=H,
                           world_view_transform=torch.tensor(cam.world_view_transform, device=dev),
                           full_proj_transform=torch.tensor(cam.full_proj_transform, device=dev))


def allmap(W, H, seed, holes=True):
    """A plausible allmap: smooth depth field with steps, alpha in (0,1], unnormalised normals."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    alpha = np.clip(rng.uniform(0.2, 1.0, (H, W)) + 0.1 * np.sin(xx / 7), 0.05, 1.0).astype(np.float32)
    depth = (2.5 + 0.4 * np.sin(xx / 9.0) * np.cos(yy / 5.0) + 0.05 * rng.normal(size=(H, W))).astype(np.float32)
    depth[yy > 0.7 * H] += 1.0  # a depth discontinuity
    n = rng.normal(size=(3, H, W)).astype(np.float32) * alpha
    med = (depth + 0.02 * rng.normal(size=(H, W))).astype(np.float32)
    dist = rng.uniform(0, 0.1, (H, W)).astype(np.float32)
    am = np.stack([depth * alpha, alpha, n[0], n[1], n[2], med, dist]).astype(np.float32)
    if holes and H > 4 and W > 4:
        am[1, 2, 3] = 0.0; am[0, 2, 3] = 0.0          # 0/0 -> nan -> 0
        am[1, 3, 1] = 0.0; am[0, 3, 1] = 0.5          # x/0 -> +inf -> 0
        am[5, 1, 2] = np.nan                           # nan median
        am[5, 4, 4] = np.inf
    return am
