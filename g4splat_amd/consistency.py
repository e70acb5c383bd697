"""Cross-view consistency (include/g4s_render_maps.h, "Cross-view consistency"; csrc/tsdf/consistency.hip).

The third stage the reference runs between view selection and training (scripts/plane_refine_depth.py): one of two
"inconsistency solvers" writes the confident maps that train_with_refine_depth.py loads as pa_confident_maps_list and
repaints the inpainted images so that views agree on colour.

  solve_point_inconsistency   guidance/inconsistence_solver.py: a point of the refined clouds that an input view sees
                              marks its pixel of every inpainted view as not confident; a point that only inpainted views
                              see carries the colour of the first of them into the others.
  solve_plane_inconsistency   guidance/plane_inconsistency_solver.py: every global plane picks the anchor view that sees
                              most of its points, and the pixels of the plane in every view take the anchor's colours.

Everything per point and per pixel runs in the library; there is no torch path, no table per (point, view) pair and no
launch per (plane, view, anchor) triple.  The small decisions -- which anchor, which order -- are made on the host in
Python integers by `choose_anchor_views` and `plane_steps`, which run without a device.

A camera is anything with world_view_transform, FoVx and FoVy; a view's size is its depth map's, and every image, mask
and point grid of the view must match it.  There is no file I/O: the callers keep writing PNGs (images_to_uint8 is the
reference's save step).  INTEGRATION.md section N lists the differences from the reference.
"""
import numpy as np
import torch

from . import _lib, planes
from ._device import camera_views, device_points, hip_device, host_array, launch, on_device

MAX_VIEWS_PER_CALL = 4096  # a longer view list of the point solver is passed in chunks


# ---- the decisions (host, no device code: tests/test_consistency_cpu.py runs them) -------------------------------------
def choose_anchor_views(counts, anchor_view_ids):
    """The anchor view of every plane from counts [K][A] (anything that iterates as rows of integers): the view of the
    first j with the largest count if that count is > 0, otherwise -1 -- the reference's strict `>` scan."""
    anchor_view_ids = [int(a) for a in anchor_view_ids]
    out = []
    for row in counts:
        best, view = 0, -1
        for j, c in enumerate(row):
            if int(c) > best:
                best, view = int(c), anchor_view_ids[j]
        out.append(view)
    return out


def _as_pairs(global_3Dplane_ID_dict):
    """{key: [(view, plane id), ...]} in the dict's order, as planes.py returns or loads it; a pair listed twice raises."""
    out, seen = {}, set()
    for k, pairs in global_3Dplane_ID_dict.items():
        out[int(k)] = [(int(v), int(p)) for v, p in pairs]
        for pair in out[int(k)]:
            if pair in seen:
                raise ValueError(f"global_3Dplane_ID_dict lists (view, plane) {pair} twice")
            seen.add(pair)
    return out


def plane_steps(global_3Dplane_ID_dict, anchor_of_plane):
    """The repaint order: [(view, plane id, anchor view), ...], the pairs of every plane whose anchor is not -1, in dict
    order then list order.  Step t is entry t.  A (view, plane) pair listed twice raises ValueError."""
    steps = []
    for k, pairs in _as_pairs(global_3Dplane_ID_dict).items():
        a = int(anchor_of_plane[k])
        if a != -1:
            steps.extend((v, p, a) for v, p in pairs)
    return steps


def images_to_uint8(x):
    """uint8 of trunc(x * 255.0f): the reference's save step (`(rgb * 255).astype(np.uint8)`), for tensors and arrays."""
    if isinstance(x, torch.Tensor):
        return (x.float() * 255.0).to(torch.uint8)
    return (np.asarray(x, np.float32) * np.float32(255.0)).astype(np.uint8)


# ---- argument plumbing -------------------------------------------------------------------------------------------------------
def _check_tensor(t, name, v, dev, dtype, shapes):
    if not isinstance(t, torch.Tensor) or t.device != dev:
        raise RuntimeError(f"{name}[{v}] must be a tensor on {dev}")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}[{v}] must be {dtype} (got {t.dtype})")
    if tuple(t.shape) not in shapes:
        raise ValueError(f"{name}[{v}] must have shape {' or '.join(str(s) for s in shapes)} (got {tuple(t.shape)})")
    return t.detach().contiguous()


def _same_length(n, **lists):
    for name, l in lists.items():
        if len(l) != n:
            raise ValueError(f"{n} cameras but {len(l)} {name}")


# ---- A. point solver -------------------------------------------------------------------------------------------------------
def _view_chunks(n_views, n_input):
    """(lo, hi, input views of the chunk): the whole list if it fits one call, otherwise the input views in chunks and then
    the inpainted views in chunks -- the order the library's `resume` asks for."""
    if n_views <= MAX_VIEWS_PER_CALL:
        return [(0, n_views, n_input)] if n_views else []
    step = MAX_VIEWS_PER_CALL
    chunks = [(lo, min(lo + step, n_input), min(lo + step, n_input) - lo) for lo in range(0, n_input, step)]
    return chunks + [(lo, min(lo + step, n_views), 0) for lo in range(n_input, n_views, step)]


def _solve_points(cameras, depths, images, points, n_input_views, depth_threshold, outputs):
    cameras, depths, images = list(cameras), list(depths), list(images)
    V, I = len(cameras), int(n_input_views)
    _same_length(V, depths=depths, images=images)
    if not 0 <= I <= V:
        raise ValueError(f"n_input_views must be in 0 .. {V} (got {I})")
    if not isinstance(points, torch.Tensor) or not points.dtype.is_floating_point:
        raise RuntimeError("points must be a floating-point tensor on a HIP device")
    dev, pts = device_points(points)
    n = pts.size(0)
    lib = _lib.load()
    need_state = n > 0 and (not outputs or I < V)
    state = torch.zeros(max(n, 1), dtype=torch.int32, device=dev) if need_state else None
    for v, d in enumerate(depths):  # every view is checked before the first chunk is launched
        if on_device(d, dev, "depth").dim() < 2:
            raise RuntimeError(f"depth must be [H,W] or [1,H,W] (got {tuple(d.shape)})")
        H, W = d.shape[-2:]
        images[v] = _check_tensor(images[v], "images", v, dev, torch.float32, ((H, W, 3), (3, H, W)))
    images_out, conf = [], []
    first = True
    for lo, hi, n_in in _view_chunks(V, I):
        views = camera_views(cameras[lo:hi], depths[lo:hi], dev)
        imgs, chw, outs, confs = images[lo:hi], [], [], []
        for v in range(lo, hi):
            H, W = views.size(v - lo)
            chw.append(0 if tuple(images[v].shape) == (H, W, 3) else 1)
            if outputs:
                outs.append(torch.empty((H, W, 3), dtype=torch.float32, device=dev))
                confs.append(torch.empty((H, W), dtype=torch.uint8, device=dev))
        launch(dev, "g4s_consistency_points", n, _lib.ptr(pts), float(depth_threshold), views.n, n_in, *views.head[1:],
               _lib.ptrs(imgs), _lib.array(_lib.c_i, chw), _lib.ptrs(outs) if outputs else None,
               _lib.ptrs(confs) if outputs else None, 0 if first else 1, _lib.ptr(state),
               workspace=lib.g4s_consistency_points_workspace(views.n, n_in, views.sizes), sync=True)
        first = False
        images_out += outs
        conf += confs
    return images_out, conf, state, n, dev


def solve_point_inconsistency(cameras, depths, images, points, n_input_views, depth_threshold=0.1):
    """guidance/inconsistence_solver.py on the device: (images_out -- float32 [H,W,3] per view --, confident_maps -- uint8
    [H,W] per view) for all V views, the first n_input_views of them input views.  images are float32 [H,W,3] or [3,H,W]
    (a camera's original_image) in 0 .. 1 and are only read; points [N,3] are the refined clouds of all views.  A pixel
    that several unseen points hit takes the colour of the largest point index."""
    images_out, conf, _state, _n, _dev = _solve_points(cameras, depths, images, points, n_input_views, depth_threshold, True)
    return images_out, conf


def point_states(cameras, depths, images, points, n_input_views, depth_threshold=0.1):
    """(seen bool [N], visible bool [N], colours uint8 [N,3]): some input view sees the point, some view sees it, and the
    colour of a point that is visible and not seen (0 for every other point)."""
    _o, _c, state, n, dev = _solve_points(cameras, depths, images, points, n_input_views, depth_threshold, False)
    if state is None:
        state = torch.zeros(0, dtype=torch.int32, device=dev)
    s = state[:n]
    colours = torch.stack([(s >> (8 * c)) & 255 for c in range(3)], dim=1).to(torch.uint8)
    return ((s >> 24) & 1).bool(), ((s >> 25) & 1).bool(), colours


# ---- B. plane solver -------------------------------------------------------------------------------------------------------
def solve_plane_inconsistency(cameras, depths, images, plane_masks, points, global_3Dplane_ID_dict, anchor_view_ids,
                              depth_threshold=0.1):
    """guidance/plane_inconsistency_solver.py on the device: (images_out -- uint8 [H,W,3] per view --, anchor_of_plane
    {k: view or -1}, counts int64 [K,A]).  Per view: a uint8 image [H,W,3], an integer plane mask [H,W] (any ids, 0 = no
    plane) and pixel-aligned float32 points [H*W,3] (the refine_points_frame clouds); the dict is planes.py's, and
    anchor_view_ids are indices into the view list.  The inputs are only read."""
    cameras, depths, images = list(cameras), list(depths), list(images)
    plane_masks, points = list(plane_masks), list(points)
    V = len(cameras)
    _same_length(V, depths=depths, images=images, plane_masks=plane_masks, points=points)
    pairs = _as_pairs(global_3Dplane_ID_dict)
    anchor_view_ids = [int(a) for a in anchor_view_ids]
    K, A = len(pairs), len(anchor_view_ids)
    if V == 0:
        return [], {k: -1 for k in pairs}, torch.zeros((K, A), dtype=torch.int64)
    if not isinstance(depths[0], torch.Tensor):
        raise RuntimeError("depth must be a tensor on a HIP device")
    dev = hip_device(depths[0].device)
    views = camera_views(cameras, depths, dev)
    imgs, slots, clouds, outs, slot_of = [], [], [], [], []
    for v in range(V):
        H, W = views.size(v)
        imgs.append(_check_tensor(images[v], "images", v, dev, torch.uint8, ((H, W, 3),)))
        s, ids = planes.slot_mask(plane_masks[v], dev)
        if tuple(s.shape) != (H, W):
            raise ValueError(f"plane_masks[{v}] must have shape {(H, W)} (got {tuple(s.shape)})")
        slots.append(s)
        slot_of.append({pid: k + 1 for k, pid in enumerate(ids.tolist())})
        clouds.append(_check_tensor(points[v], "points", v, dev, torch.float32, ((H * W, 3), (H, W, 3))))
        outs.append(torch.empty((H, W, 3), dtype=torch.uint8, device=dev))
    slot_offset = [0]
    for s in slot_of:
        slot_offset.append(slot_offset[-1] + len(s) + 1)
    n_slots = slot_offset[-1]
    slot_plane = [-1] * n_slots
    for n, plist in enumerate(pairs.values()):
        for v, p in plist:
            if not 0 <= v < V:
                raise ValueError(f"global_3Dplane_ID_dict names view {v} but there are {V} views")
            if p in slot_of[v]:  # a plane id the mask does not hold is an empty set
                slot_plane[slot_offset[v] + slot_of[v][p]] = n
    lib = _lib.load()
    head = [float(depth_threshold), *views.head, _lib.ptrs(slots), _lib.ptrs(clouds)]
    offsets = _lib.array(_lib.c_i, slot_offset)
    counts = torch.zeros(max(K * A, 1), dtype=torch.int32, device=dev)
    launch(dev, "g4s_consistency_plane_counts", *head, offsets, _lib.array(_lib.c_i, slot_plane), K, A,
           host_array(_lib.c_i, anchor_view_ids), _lib.ptr(counts),
           workspace=lib.g4s_consistency_plane_counts_workspace(V, n_slots, A))
    counts = counts[: K * A].cpu().to(torch.int64).reshape(K, A)  # the one read-back
    anchors = choose_anchor_views(counts.tolist(), anchor_view_ids)
    anchor_of_plane = dict(zip(pairs, anchors))
    slot_step, slot_anchor = [-1] * n_slots, [0] * n_slots
    for t, (v, p, a) in enumerate(plane_steps(pairs, anchor_of_plane)):
        if p in slot_of[v]:
            e = slot_offset[v] + slot_of[v][p]
            slot_step[e], slot_anchor[e] = t, a
    launch(dev, "g4s_consistency_plane_repaint", *head, _lib.ptrs(imgs), _lib.ptrs(outs), offsets,
           _lib.array(_lib.c_i, slot_step), _lib.array(_lib.c_i, slot_anchor),
           workspace=lib.g4s_consistency_plane_repaint_workspace(V, views.sizes, n_slots), sync=True)
    return outs, anchor_of_plane, counts
