"""View selection (include/g4s_render_maps.h, "View selection"; csrc/tsdf/view_select.hip).

The two pieces of the reference's novel-view stage (render_novel_views.py over guidance/cam_utils.py) that sit between
the visibility maps of g4splat_amd.visibility and the camera file the stage writes: which candidate cameras go to the
inpainter (select_need_inpaint_views over covisibility_check_by_gs) and where the look-around cameras aim
(get_novel_cams_lookat_points over farthest_point_sample).

The library computes, for all cameras at once, one bit per (camera, point) and the integer table of shared points, and
samples all clouds in one batch; there is no torch path.  The sequential decisions are made on the host in Python
integers and floats, exactly as the reference writes them, by ONE function, `select_views`, over a ratio(i, j) callable:
the device table here, the numpy restatement in tests/view_selection_ref.py.  The random draws are the reference's calls
in the reference's order.

A camera is anything with world_view_transform, FoVx, FoVy, image_width and image_height.  Points and clouds are device
tensors.  INTEGRATION.md section O lists the differences from the reference.
"""
import ctypes
import random

import numpy as np
import torch

from . import _lib
from ._device import focal_lengths, hip_device, host_f32, launch, to_np
from .planes import covisibility_rate

MAX_POINTS = 2 ** 31 - 64


# ---- host-side checks (nothing here touches the library) --------------------------------------------------------------
def _camera_arrays(cameras):
    """(n, world_view [n*16], focal [n*2], sizes [n*2]) as the library's host arrays."""
    cameras = list(cameras)
    if not cameras:
        raise ValueError("at least one camera is needed")
    world_view, focal, sizes = [], [], []
    for i, cam in enumerate(cameras):
        M = np.asarray(to_np(cam.world_view_transform), np.float32)
        if M.size != 16:
            raise ValueError(f"camera {i}: world_view_transform must be 4 x 4")
        W, H = int(cam.image_width), int(cam.image_height)
        if W <= 0 or H <= 0:
            raise ValueError(f"camera {i}: image_width and image_height must be positive")
        world_view.extend(M.reshape(16).tolist())
        focal += focal_lengths(cam, W, H)
        sizes += [W, H]
    return len(cameras), host_f32(world_view), host_f32(focal), (ctypes.c_int * len(sizes))(*sizes)


def _check_points(points):
    if not isinstance(points, torch.Tensor):
        raise ValueError("points must be a tensor [P,3] on a HIP device")
    if points.dim() != 2 or points.size(1) != 3:
        raise ValueError(f"points must be [P,3] (got {tuple(points.shape)})")
    if points.size(0) > MAX_POINTS:
        raise ValueError("at most 2^31 - 64 points")


def _xyz(gaussians_or_points):
    return gaussians_or_points.get_xyz if hasattr(gaussians_or_points, "get_xyz") else gaussians_or_points


# ---- A. visible bits and the covisibility table --------------------------------------------------------------------------
class Covisibility:
    """Which of P points each of C cameras sees (in the image and in front of the camera), as bits, and how many points
    every pair shares.  `words` int64 [C, ceil(P / 64)]: bit (p & 63) of words[c, p >> 6]; `counts` int32 [C,C], computed
    on first use; `visible_counts` int32 [C] its diagonal.  Two launches for any number of pairs."""

    def __init__(self, points, cameras):
        _check_points(points)
        self.n_cameras, world_view, focal, sizes = _camera_arrays(cameras)
        dev, pts = hip_device(points.device), points.detach().float().contiguous()
        self.device, self.n_points = dev, pts.size(0)
        C, P = self.n_cameras, self.n_points
        self.n_words = (P + 63) // 64
        self.words = torch.empty((C, self.n_words), dtype=torch.int64, device=dev)
        self._counts = self._table = None
        launch(dev, "g4s_view_bits", P, _lib.ptr(pts), C, world_view, focal, sizes, _lib.ptr(self.words),
               workspace=_lib.load().g4s_view_bits_workspace(C), sync=True)

    @property
    def counts(self):
        if self._counts is None:
            C, dev = self.n_cameras, self.device
            counts = torch.empty((C, C), dtype=torch.int32, device=dev)
            launch(dev, "g4s_view_overlap", C, self.n_words, _lib.ptr(self.words), _lib.ptr(counts))
            self._counts = counts
        return self._counts

    @property
    def visible_counts(self):
        return self.counts.diagonal()

    def mask(self, c):
        """bool [P]: the points camera c sees."""
        shifts = torch.arange(64, dtype=torch.int64, device=self.device)
        bits = (self.words[int(c)].unsqueeze(1) >> shifts.unsqueeze(0)) & 1
        return bits.reshape(-1)[: self.n_points].bool()

    def ratio(self, i, j):
        """The reference's covisibility ratio of cameras i and j: max(common / |V_i|, common / |V_j|) in Python numbers, a
        camera that sees nothing contributing 0.  The table is read back once."""
        if self._table is None:
            self._table = self.counts.cpu().tolist()
        t = self._table
        return covisibility_rate(t[i][j], t[i][i], t[j][j])  # a camera that sees nothing shares nothing: 0 either way


def get_visible_points_mask(camera, points):
    """guidance/cam_utils.py: bool [P], the points in the camera's image and in front of it."""
    return Covisibility(points, [camera]).mask(0)


def get_covisible_points(camera1, camera2, points):
    """guidance/cam_utils.py: the points [n,3] that both cameras see."""
    table = Covisibility(points, [camera1, camera2])
    return points[table.mask(0) & table.mask(1)]


def covisibility_check_by_gs(camera1, camera2, gaussians_or_points):
    """guidance/cam_utils.py: the covisibility ratio of two cameras over a Gaussian model's centres (or points [P,3])."""
    return Covisibility(_xyz(gaussians_or_points), [camera1, camera2]).ratio(0, 1)


# ---- the decisions (host, no device code: tests/test_view_selection_cpu.py runs them over the restatement) ---------------
def select_views(rates, ratio, select_num=10, none_visible_rate_low_bound=0.05, none_visible_rate_high_bound=0.5,
                 covisible_rate_high_bound=0.8, rng=random):
    """The reference's select_need_inpaint_views as decisions over ratio(i, j).  rates[i] is view i's share of pixels no
    input view sees.  The views are shuffled once; those with a rate inside the bounds are taken greedily, each only if its
    ratio against every view taken so far stays at or below covisible_rate_high_bound; if that leaves fewer than
    select_num, the views below the lower bound are tried the same way; if there are still too few, the rest with a rate at
    or below the upper bound is shuffled and fills up.  `rng` is consumed exactly as the reference consumes `random`."""
    rates = list(rates)
    order = [(i, rate) for i, rate in enumerate(rates)]
    rng.shuffle(order)
    selected = []

    def take_greedily(candidates):
        for view, _rate in candidates:
            if view in selected:
                continue  # as in the reference, this also skips the stop test below
            if not any(ratio(s, view) > covisible_rate_high_bound for s in selected):
                selected.append(view)
            if len(selected) >= select_num:
                break

    in_range = [(i, r) for i, r in order if none_visible_rate_low_bound <= r <= none_visible_rate_high_bound]
    if in_range:
        selected.append(in_range[0][0])
    take_greedily(in_range)
    if len(selected) < select_num:
        take_greedily([(i, r) for i, r in order if r < none_visible_rate_low_bound and i not in selected])
    if len(selected) < select_num:
        rest = [i for i in range(len(rates)) if i not in selected and rates[i] <= none_visible_rate_high_bound]
        rng.shuffle(rest)
        selected.extend(rest[: select_num - len(selected)])
    return selected


def select_need_inpaint_views(novel_cams, gs_none_visible_rate, gaussians_or_points, select_num=10,
                              none_visible_rate_low_bound=0.05, none_visible_rate_high_bound=0.5,
                              covisible_rate_high_bound=0.8):
    """guidance/cam_utils.py: the ids of the candidate cameras to inpaint.  One covisibility table over all candidates
    replaces the reference's projection of every point for every pair it asks about."""
    novel_cams, rates = list(novel_cams), list(gs_none_visible_rate)
    if len(novel_cams) != len(rates):
        raise ValueError(f"{len(novel_cams)} cameras but {len(rates)} rates")
    table = Covisibility(_xyz(gaussians_or_points), novel_cams)
    return select_views(rates, table.ratio, select_num, none_visible_rate_low_bound, none_visible_rate_high_bound,
                        covisible_rate_high_bound, random)


# ---- B. farthest-point sampling ----------------------------------------------------------------------------------------------
def _check_sampling(clouds, num_samples, first_indices):
    if not isinstance(clouds, torch.Tensor) or clouds.dim() != 3 or clouds.size(2) != 3:
        raise ValueError("clouds must be a tensor [M,N,3] on a HIP device")
    M, N = clouds.size(0), clouds.size(1)
    k = int(num_samples)
    if M < 1:
        raise ValueError("at least one cloud is needed")
    if not 2 <= k < N:
        raise ValueError(f"num_samples must be at least 2 and below the {N} points of a cloud (got {k})")
    first = first_indices.reshape(-1).tolist() if isinstance(first_indices, torch.Tensor) else [int(i) for i in first_indices]
    if len(first) != M:
        raise ValueError(f"{M} clouds but {len(first)} first indices")
    for m, i in enumerate(first):
        if not 0 <= int(i) < N:
            raise ValueError(f"first index {i} of cloud {m} is outside 0 .. {N - 1}")
    return M, N, k, [int(i) for i in first]


def farthest_point_indices(clouds, num_samples, first_indices, return_dist=False):
    """Farthest-point sampling of M clouds [M,N,3] at once: (indices int32 [M,k], points [M,k,3]), and with return_dist the
    final squared distance of every point to its cloud's nearest sample, float32 [M,N], capped at 1e10 as in the
    reference.  Sample 0 of cloud m is first_indices[m]; every further one is the point farthest from the samples so far,
    the smallest index among equals.  k launches for all clouds together."""
    M, N, k, first = _check_sampling(clouds, num_samples, first_indices)
    dev = hip_device(clouds.device)
    pts = clouds.detach().float().contiguous()
    indices = torch.empty((M, k), dtype=torch.int32, device=dev)
    samples = torch.empty((M, k, 3), dtype=torch.float32, device=dev)
    dist = torch.empty((M, N), dtype=torch.float32, device=dev)
    launch(dev, "g4s_fps", M, N, _lib.ptr(pts), _lib.array(ctypes.c_int, first), k, _lib.ptr(indices), _lib.ptr(samples),
           _lib.ptr(dist), workspace=_lib.load().g4s_fps_workspace(M, k), sync=True)
    return (indices, samples, dist) if return_dist else (indices, samples)


def farthest_point_sample(points, num_samples, first_index=None):
    """guidance/cam_utils.py: num_samples points of points [N,3], farthest first.  As in the reference, a cloud of at most
    num_samples points comes back unchanged, and without first_index the first sample is drawn with torch.randint on the
    points' device."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.size(1) != 3:
        raise ValueError("points must be a tensor [N,3] on a HIP device")
    N = points.size(0)
    if N <= num_samples:
        return points
    if first_index is None:
        first_index = torch.randint(0, N, (1,), device=points.device)
    return farthest_point_indices(points.unsqueeze(0), num_samples, first_index if isinstance(first_index, torch.Tensor)
                                  else [first_index])[1][0]


def draw_lookat_indices(n_views, n_points, n_novel, fps_num, device):
    """The random draws of get_novel_cams_lookat_points, the reference's calls in the reference's order: per input view the
    first sample of its cloud (none when the cloud has at most fps_num points), then one look-at sample id per novel
    camera.  (first [n_views] or None, ids [n_novel]), int64 on `device`."""
    first = None
    if n_points > fps_num:
        first = torch.cat([torch.randint(0, n_points, (1,), device=device) for _ in range(n_views)])
    return first, torch.randint(0, fps_num, (n_novel,), device=device)


def nearest_train_indices(train_cam_centers, novel_cam_centers):
    """int64 [K]: for every novel centre the training centre at the smallest squared distance ((dx*dx + dy*dy) + dz*dz in
    float32, d = train - novel), the smallest index among equals."""
    t, c = train_cam_centers.float(), novel_cam_centers.float()
    dx, dy, dz = (t[None, :, a] - c[:, None, a] for a in range(3))
    d = (dx * dx + dy * dy) + dz * dz
    ids = torch.arange(t.size(0), device=d.device).expand_as(d)
    return torch.where(d == d.min(1, keepdim=True).values, ids, t.size(0)).min(1).values


def get_novel_cams_lookat_points(train_cam_centers, gs_train_view_points, novel_cam_centers, fps_num=10):
    """guidance/cam_utils.py: [K,3], for every novel camera one of the fps_num farthest-point samples of the cloud of its
    nearest training camera.  One batched sampling for all training views."""
    clouds = gs_train_view_points
    if not isinstance(clouds, torch.Tensor) or clouds.dim() != 3 or clouds.size(2) != 3:
        raise ValueError("gs_train_view_points must be a tensor [M,N,3] on a HIP device")
    M, N, K = clouds.size(0), clouds.size(1), novel_cam_centers.size(0)
    if tuple(train_cam_centers.shape) != (M, 3) or tuple(novel_cam_centers.shape) != (K, 3):
        raise ValueError("train_cam_centers must be [M,3] and novel_cam_centers [K,3]")
    device = novel_cam_centers.device
    closest = nearest_train_indices(train_cam_centers, novel_cam_centers)
    first, ids = draw_lookat_indices(M, N, K, int(fps_num), device)
    samples = clouds if first is None else farthest_point_indices(clouds, fps_num, first)[1]
    return samples[closest, ids]
