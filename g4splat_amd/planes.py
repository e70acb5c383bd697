"""Global 3D planes (include/g4s_render_maps.h, "Global planes"; csrc/tsdf/planes.hip).

The stage the reference runs between view selection and plane-aware depth refinement (planes/merge_global_3Dplane.py over
guidance/cam_utils.py get_pixel_to_points_tensor): which points of the chart cloud each view's plane mask claims -- the
front points of every pixel -- and which local planes of which views are one scene plane.  The result is the reference's
`global_3Dplane_ID_dict` (the file global_3Dplane_ID_dict.json three later stages read) and the point indices per plane.

Labels, membership and every count are computed on the device by the library; there is no torch path and no sort, unique,
isin or cat over points.  The sequential merge decisions are made on the host in Python integers and floats, exactly as
the reference writes them, by ONE function, `merge_global_planes`, over a counts provider: the device state here, Python
sets in tests/planes_ref.py.  Only the small count matrices and the masks' id lists cross to the host: one read-back per
view and one per sweep step.

A camera is anything with world_view_transform, FoVx and FoVy; a plane mask is an integer device tensor [H,W] whose size
stands in for the camera's; ids are any non-zero int32, 0 is "no plane".  INTEGRATION.md section M lists the differences
from the reference.
"""
import ctypes
import json

import torch

from . import _lib
from ._device import camera_views, device_points, launch


# ---- the decisions (host, no device code: tests/test_planes_cpu.py runs them over sets) ------------------------------------
def covisibility_rate(c, a, b):
    """max(c / a, c / b) in Python floats for |G ∩ S| = c, |G| = a, |S| = b; an empty set has rate 0 against everything
    (the reference divides by zero there)."""
    if a == 0 or b == 0:
        return 0.0
    return max(c / a, c / b)


def _as_id_dict(d):
    """{int: [(view, plane), ...]} from a dict as returned here or loaded from JSON; keys must be 0 .. K-1 in order."""
    out = {int(k): [(int(v), int(p)) for v, p in pairs] for k, pairs in d.items()}
    if list(out) != list(range(len(out))):
        raise ValueError("previous_global_3Dplane_ID_dict must have the keys 0 .. K-1 in order")
    return out


def merge_global_planes(provider, n_views, previous_global_3Dplane_ID_dict=None, covisible_ratio_thresh=0.5):
    """The reference's get_init_global_3Dplane / update_global_3Dplane / final_merge_global_3Dplane as decisions over integer
    counts.  Returns (list of ascending index arrays, {global id: [(view id, plane id), ...]}).

    provider:
      view_counts(v)   -> (plane ids of view v ascending without 0, sizes [P], counts [P][G]) against the G rows so far
      assign(v, target)   target[k] = row that local plane k joins (rows at and above G are new), or -1
      row_counts(g)    -> [G] |row g ∩ row h|, [g] being the row's size
      merge_rows(dst, src);  row_indices(g) -> ascending indices of row g

    The local planes of a view are disjoint, so the counts read before a view's decisions stay valid while its planes
    are absorbed one after the other; only the sizes move, by |G ∪ S| = |G| + |S| - |G ∩ S|."""
    thresh = covisible_ratio_thresh
    sizes, ids = [], {}
    if n_views == 0:
        return [], {}
    if previous_global_3Dplane_ID_dict is None:
        plane_ids, s, _ = provider.view_counts(0)
        for k, pid in enumerate(plane_ids):  # empty planes included, as in the reference
            sizes.append(int(s[k]))
            ids[k] = [(0, pid)]
        provider.assign(0, list(range(len(plane_ids))))
        next_view = 1
    else:
        ids = _as_id_dict(previous_global_3Dplane_ID_dict)
        sizes = [0] * len(ids)
        last = max([v for pairs in ids.values() for v, _p in pairs], default=0)
        if last >= n_views:
            raise ValueError(f"the previous dict names view {last} but there are {n_views} views")
        where = {}
        for g, pairs in ids.items():
            for pair in pairs:
                if pair in where:
                    raise ValueError(f"the previous dict lists (view, plane) {pair} twice")
                where[pair] = g
        for v in range(last + 1):
            plane_ids, s, counts = provider.view_counts(v)
            target = [where.get((v, pid), -1) for pid in plane_ids]
            for k, g in enumerate(target):
                if g >= 0:  # a row the provider has not made yet is empty
                    sizes[g] += int(s[k]) - (int(counts[k][g]) if g < len(counts[k]) else 0)
            provider.assign(v, target)
        next_view = last + 1
    for v in range(next_view, n_views):
        plane_ids, s, counts = provider.view_counts(v)
        n_before = len(sizes)
        target = []
        for k, pid in enumerate(plane_ids):
            b = int(s[k])
            if b == 0:
                target.append(-1)
                continue
            for g in range(len(sizes)):
                c = int(counts[k][g]) if g < n_before else 0  # a row made by this view is disjoint from this plane
                if covisibility_rate(c, sizes[g], b) > thresh:
                    sizes[g] += b - c
                    ids[g].append((v, pid))
                    target.append(g)
                    break
            else:
                target.append(len(sizes))
                ids[len(sizes)] = [(v, pid)]
                sizes.append(b)
        provider.assign(v, target)
    # the final sweep: counts against the grown row are read again after every merge
    n = len(sizes)
    merged = [False] * n
    new_idx, new_ids = [], {}
    for i in range(n):
        if merged[i]:
            continue
        cur_ids = list(ids[i])
        counts = provider.row_counts(i) if i + 1 < n else None
        for j in range(i + 1, n):
            if merged[j]:
                continue
            if covisibility_rate(int(counts[j]), int(counts[i]), sizes[j]) > thresh:
                provider.merge_rows(i, j)
                cur_ids.extend(ids[j])
                merged[j] = True
                counts = provider.row_counts(i)
        new_ids[len(new_idx)] = cur_ids
        new_idx.append(provider.row_indices(i))
        merged[i] = True
    return new_idx, new_ids


# ---- JSON, in the reference's shape: string keys, lists of pairs ------------------------------------------------------------
def save_global_3Dplane_ID_dict(path, global_3Dplane_ID_dict):
    with open(path, "w") as f:
        json.dump({str(k): [[int(v), int(p)] for v, p in pairs] for k, pairs in global_3Dplane_ID_dict.items()}, f)


def load_global_3Dplane_ID_dict(path):
    with open(path) as f:
        return {int(k): [(int(v), int(p)) for v, p in pairs] for k, pairs in json.load(f).items()}


# ---- device path ---------------------------------------------------------------------------------------------------------------
def slot_mask(mask, dev):
    """(slot mask int32 [H,W] with values 0 .. P, the P plane ids ascending as a device tensor): torch.unique and
    bucketize over the mask's pixels."""
    if not isinstance(mask, torch.Tensor) or mask.device != dev:
        raise RuntimeError(f"plane masks must be tensors on {dev}")
    if mask.dim() != 2 or mask.dtype.is_floating_point:
        raise RuntimeError(f"a plane mask must be an integer tensor [H,W] (got {tuple(mask.shape)}, {mask.dtype})")
    m = mask.detach().to(torch.int32)
    ids = torch.unique(m)
    ids = ids[ids != 0]
    slots = torch.where(m != 0, torch.bucketize(m, ids) + 1, torch.zeros_like(m)) if ids.numel() else torch.zeros_like(m)
    return slots.to(torch.int32).contiguous(), ids


class _LabelledViews:
    """Slot labels of a list of views, computed a chunk of views per launch and kept one chunk at a time."""

    MAX_LABEL_BYTES = 1 << 28

    def __init__(self, cameras, points, plane_masks, depth_thresh):
        self.dev, self.points = device_points(points)
        self.n = self.points.size(0)
        self.cameras, masks = list(cameras), list(plane_masks)
        if len(self.cameras) != len(masks):
            raise ValueError(f"{len(self.cameras)} cameras but {len(masks)} plane masks")
        self.slots, self.ids = [], []
        for m in masks:
            s, ids = slot_mask(m, self.dev)
            self.slots.append(s)
            self.ids.append(ids)
        self.id_lists = [ids.tolist() for ids in self.ids]
        self.depth_thresh = float(depth_thresh)
        self.chunk = max(1, min(len(masks), self.MAX_LABEL_BYTES // max(4 * self.n, 1)))
        self._first, self._labels = 0, None

    def labels(self, v):
        """int32 [N] slot labels of view v (a view into the current chunk)."""
        if self._labels is None or not self._first <= v < self._first + self._labels.size(0):
            self._first = v - v % self.chunk
            self._labels = self._launch(self._first, min(self._first + self.chunk, len(self.slots)))
        return self._labels[v - self._first]

    def _launch(self, lo, hi):
        dev, n = self.dev, self.n
        # the view plumbing of the Visibility section; a float view of the int32 mask only carries its address and shape
        views = camera_views(self.cameras[lo:hi], [s.view(torch.float32) for s in self.slots[lo:hi]], dev)
        labels = torch.empty((hi - lo, max(n, 1)), dtype=torch.int32, device=dev)[:, :n].contiguous()
        launch(dev, "g4s_plane_labels", n, _lib.ptr(self.points), self.depth_thresh, *views.head, _lib.ptr(labels),
               workspace=_lib.load().g4s_plane_labels_workspace(views.n, views.sizes), sync=True)
        return labels


class PlaneMembership:
    """Membership of N points in G global planes as bits: `words` int64 [n_words, N], bit (g & 63) of words[g >> 6, i].
    Grows by whole blocks of N words; the bits at and above G stay zero."""

    def __init__(self, n_points, device):
        self.n, self.dev, self.G = int(n_points), device, 0
        self.words = torch.zeros((1, max(self.n, 1)), dtype=torch.int64, device=device)
        self.launches = 0

    @property
    def n_words(self):
        return self.words.size(0)

    def _args(self):
        return [self.G, self.n_words, _lib.ptr(self.words)]

    def _grow(self, G):
        need = (G + 63) // 64
        if need > self.n_words:
            words = torch.zeros((max(need, 2 * self.n_words), self.words.size(1)), dtype=torch.int64, device=self.dev)
            words[: self.n_words] = self.words
            self.words = words
        self.G = max(self.G, G)

    def _read(self, t):
        return t.cpu().tolist()  # the one read-back (and host synchronisation) of a step

    def overlap(self, labels, n_planes):
        """(sizes [P], counts [P][G]) as Python ints for the slot labels of one view."""
        P, G = int(n_planes), self.G
        out = torch.empty(max(P * (G + 1), 1), dtype=torch.int32, device=self.dev)
        launch(self.dev, "g4s_plane_overlap", self.n, _lib.ptr(labels), P, *self._args(), _lib.ptr(out),
               ctypes.c_void_p(out.data_ptr() + 4 * P * G))
        self.launches += 1
        flat = self._read(out)
        return flat[P * G: P * G + P], [flat[k * G: (k + 1) * G] for k in range(P)]

    def assign(self, labels, target):
        """Sets bit target[p - 1] of every point labelled p (target -1: none); rows beyond G are created."""
        if not target:
            return
        self._grow(max(max(target) + 1, self.G))
        launch(self.dev, "g4s_plane_assign", self.n, _lib.ptr(labels), len(target), _lib.array(ctypes.c_int, target),
               *self._args(), workspace=_lib.load().g4s_plane_assign_workspace(len(target)), sync=True)
        self.launches += 1

    def row_counts(self, row):
        out = torch.empty(max(self.G, 1), dtype=torch.int32, device=self.dev)
        launch(self.dev, "g4s_plane_row_overlap", self.n, *self._args(), int(row), _lib.ptr(out))
        self.launches += 1
        return self._read(out)[: self.G]

    def merge_rows(self, dst, src):
        launch(self.dev, "g4s_plane_row_merge", self.n, *self._args(), int(src), int(dst))
        self.launches += 1

    def row_mask(self, row):
        mask = torch.empty(max(self.n, 1), dtype=torch.uint8, device=self.dev)
        launch(self.dev, "g4s_plane_row_mask", self.n, *self._args(), int(row), _lib.ptr(mask))
        self.launches += 1
        return mask[: self.n]

    def row_indices(self, row):
        """int64 [k]: the ascending point indices of a row (the non-zero positions of its mask)."""
        return torch.nonzero(self.row_mask(row)).squeeze(-1)


class _DeviceProvider:
    """merge_global_planes' counts provider over the library."""

    def __init__(self, views):
        self.views = views
        self.member = PlaneMembership(views.n, views.dev)

    def view_counts(self, v):
        ids = self.views.id_lists[v]
        sizes, counts = self.member.overlap(self.views.labels(v), len(ids))
        return ids, sizes, counts

    def assign(self, v, target):
        self.member.assign(self.views.labels(v), target)

    def row_counts(self, g):
        return self.member.row_counts(g)

    def merge_rows(self, dst, src):
        self.member.merge_rows(dst, src)

    def row_indices(self, g):
        return self.member.row_indices(g)


def front_point_labels(cameras, points, plane_masks, depth_thresh=0.01):
    """int32 [V,N]: for every view the plane id (the mask's own value) of every point that is a front point of its pixel --
    not point 0, in the image, in front of the camera, within depth_thresh of the nearest such point of the pixel -- and 0
    for every other point.  A negative depth_thresh turns the depth test off."""
    views = _LabelledViews(cameras, points, plane_masks, depth_thresh)
    out = torch.empty((len(views.slots), views.n), dtype=torch.int32, device=views.dev)
    for v, ids in enumerate(views.ids):
        lut = torch.cat([torch.zeros(1, dtype=torch.int32, device=views.dev), ids])  # slot -> plane id, P + 1 entries
        out[v] = lut[views.labels(v).long()]
    return out


def plane_point_indices(labels_v, plane_id):
    """What the reference's get_plane_pnts_idx_from_mask returns: the ascending indices of the points of one view's local
    plane (index 0 never carries a label)."""
    if int(plane_id) == 0:
        return torch.empty(0, dtype=torch.int64, device=labels_v.device)
    return torch.nonzero(labels_v == int(plane_id)).squeeze(-1)


def get_global_3Dplane(cameras, points, plane_masks, previous_global_3Dplane_ID_dict=None, covisible_ratio_thresh=0.5,
                       depth_thresh=0.01):
    """planes/merge_global_3Dplane.py get_global_3Dplane on the device: (global_3Dplane_pnts_idx -- a list of ascending
    int64 index tensors --, global_3Dplane_ID_dict {global id: [(view id, plane id), ...]}).  With a previous dict the sets
    are rebuilt from its (view, plane) pairs and the update continues from the view after its last."""
    views = _LabelledViews(cameras, points, plane_masks, depth_thresh)
    return merge_global_planes(_DeviceProvider(views), len(views.slots), previous_global_3Dplane_ID_dict,
                               covisible_ratio_thresh)
