"""Per-view plane masks (include/g4s_render_maps.h, "Plane masks"; csrc/tsdf/plane_masks.hip).

What the reference's planes/plane_excavator.py does per view once the SAM network has produced its masks, and writes as
plane_mask_frame*.npy for planes.get_global_3Dplane, consistency.solve_plane_inconsistency and
depth_cues.apply_global_planes:

  kmeans_normals, kmeanspp_seeds     sklearn's KMeans(n_clusters=8, n_init=1) over the view's normals (Lloyd's algorithm).
  select_normal_clusters,            the top-n pick by size and planes/tools.py merge_normal_clusters (host, K numbers).
  merge_normal_clusters
  normal_components                  remove_small_isolated_areas (9x9 open, 8-connected components, size filter) for all kept
                                     clusters at once.
  normals_cluster                    the reference-named wrapper over the three.
  join_planes, excavate_planes       PlaneExcavator.__call__ after the network: the mask x component double loop, the
                                     repaint, the mean normal per plane.
  save_plane_mask, load_plane_mask   the .npy file the later stages read.

Everything per pixel runs in the library, all views in a number of launches that does not depend on the number of views,
masks or components; there is no torch path.  The SAM network stays with the caller: sam_masks is an input, [M,H,W] bool or
uint8 on the device, as infer_masks returns it.

Every call takes one view ([H,W,3] normals) and returns one result, or a list of views / a stacked [V,H,W,3] tensor and
returns lists; views may differ in size and in mask count.  The inputs are never written.  Two runs give the same bits.
INTEGRATION.md section R lists the differences from the reference.
"""
import collections
import math

import numpy as np
import torch

from . import _lib
from ._device import check_dtype, check_view_count, host_array, launch, mask_bytes, same_device, to_np, view_list

MAX_K = 16          # G4S_KMEANS_MAX_K
KMEANS_SPAN = 4096  # G4S_KMEANS_SPAN: pixels one workgroup of the k-means kernels labels and reduces
SEED_SAMPLE = 4096  # kmeanspp_seeds looks at no more valid normals than this

PlaneMasks = collections.namedtuple("PlaneMasks", "seg_mask normal areas")


# ---- host side: argument checks (no device code: tests/test_plane_masks_cpu.py runs them) -------------------------------
def _views(maps, name, tail, single_dim):
    """(single, list): one [H,W`tail`] tensor is a single view; otherwise a list of views or a stacked tensor."""
    if isinstance(maps, torch.Tensor) and maps.dim() == single_dim:
        return True, [maps]
    return False, view_list(maps, name, tail)


def _check_maps(maps, name, dev, dtypes, trailing=(), shapes=None, n=None):
    """The maps as contiguous tensors [H,W,*trailing] on one HIP device; ValueError for anything else."""
    check_view_count(maps, name, n)
    out = []
    for v, t in enumerate(maps):
        label = f"{name}[{v}]"
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{label} must be a tensor on a HIP device")
        check_dtype(t, dtypes, label)
        dev = same_device(t, dev, label)
        if t.dim() != 2 + len(trailing) or tuple(t.shape[2:]) != tuple(trailing) or t.numel() == 0:
            raise ValueError(f"{label} must be a non-empty [H,W{''.join(',%d' % s for s in trailing)}] map (got {tuple(t.shape)})")
        if shapes is not None and tuple(t.shape[:2]) != shapes[v]:
            raise ValueError(f"{label} must have shape {shapes[v]} (got {tuple(t.shape[:2])})")
        out.append(t.detach().contiguous())
    return dev, out


def _check_masks(sam_masks, dev, shapes):
    """Per view a contiguous uint8 view of the [M,H,W] bool / uint8 masks; M may be 0."""
    check_view_count(sam_masks, "sam_masks", len(shapes))
    out = []
    for v, t in enumerate(sam_masks):
        label = f"sam_masks[{v}]"
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{label} must be a tensor on a HIP device")
        check_dtype(t, (torch.bool, torch.uint8), label)
        dev = same_device(t, dev, label)
        if t.dim() != 3 or tuple(t.shape[1:]) != shapes[v]:
            raise ValueError(f"{label} must be [M,{shapes[v][0]},{shapes[v][1]}] (got {tuple(t.shape)})")
        out.append(mask_bytes(t.detach().contiguous()))
    return out


def _shapes(maps):
    return [tuple(t.shape[:2]) for t in maps]


def _sizes(maps):
    return host_array(_lib.c_i, [s for t in maps for s in (t.shape[1], t.shape[0])])


def _per_view(value, n, name):
    """A scalar for all views, or one value per view."""
    values = [value] * n if np.ndim(value) == 0 else list(value)
    if len(values) != n:
        raise ValueError(f"{n} views but {len(values)} {name}")
    return values


def _unwrap(single, *lists):
    return tuple(l[0] for l in lists) if single else lists


def min_plane_size(shape, min_size_ratio):
    """H * W * min_size_ratio, the reference's bar for a component, a pair and a plane (a float, compared with >=)."""
    return shape[0] * shape[1] * min_size_ratio


# ---- 1. k-means -------------------------------------------------------------------------------------------------------------
def kmeanspp_seeds(normals, k, generator=None):
    """Greedy k-means++ seeds of one view, float32 [k,3], on the host in numpy: over the valid normals (no NaN component)
    taken at a fixed stride so that at most 4096 are looked at, with 2 + floor(ln k) trials per centre as sklearn's
    kmeans_plusplus, drawing from `generator` (a CPU torch.Generator; None: one seeded with 0).  These are not sklearn's
    random_state=0 seeds: the clusters agree with the reference's statistically, not label for label."""
    if generator is None:
        generator = torch.Generator().manual_seed(0)
    X = np.asarray(to_np(normals), np.float32).reshape(-1, 3)
    X = X[~np.isnan(X).any(axis=1)]
    if len(X) == 0:
        raise ValueError("kmeanspp_seeds: the view has no valid normal")
    X = X[::max(1, -(-len(X) // SEED_SAMPLE))].astype(np.float64)
    trials = 2 + int(math.log(k))
    centres = [X[int(torch.randint(len(X), (1,), generator=generator))]]
    closest = ((X - centres[0]) ** 2).sum(axis=1)
    for _ in range(1, k):
        cum = np.cumsum(closest)
        draws = torch.rand(trials, generator=generator, dtype=torch.float64).numpy() * cum[-1]
        cand = np.minimum(np.searchsorted(cum, draws), len(X) - 1)
        dist = np.minimum(closest[None, :], ((X[None, :, :] - X[cand][:, None, :]) ** 2).sum(axis=2))
        best = int(np.argmin(dist.sum(axis=1)))
        centres.append(X[cand[best]])
        closest = dist[best]
    return np.stack(centres).astype(np.float32)


def _check_init(init, k, n_views, single):
    """None for "k-means++", else float32 [V,K,3]; K <= 16 is checked here, before anything touches a device."""
    if isinstance(init, str):
        if init != "k-means++":
            raise ValueError(f"init must be a [K,3] array or 'k-means++' (got {init!r})")
        if not 1 <= int(k) <= MAX_K:
            raise ValueError(f"k must be in 1 .. {MAX_K} (got {k})")
        return None
    a = np.asarray([to_np(i) for i in init] if isinstance(init, (list, tuple)) else to_np(init), np.float32)
    if a.ndim == 2:
        a = np.broadcast_to(a, (n_views,) + a.shape) if n_views is not None else a[None]
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[1] < 1:
        raise ValueError(f"init must be [K,3] or [V,K,3] (got {a.shape})")
    if a.shape[1] > MAX_K:
        raise ValueError(f"k must be in 1 .. {MAX_K} (got {a.shape[1]})")
    if not np.isfinite(a).all():
        raise ValueError("init must be finite")
    return a


def kmeans_normals(normals, init="k-means++", max_iter=300, tol=1e-4, k=8, generator=None):
    """Lloyd's algorithm as sklearn runs it for KMeans(n_clusters=k, n_init=1): (labels int8 [H,W], centres float32 [K,3],
    counts int32 [K], n_iter).  init: [K,3] ([V,K,3] or a list for several views), or "k-means++" for kmeanspp_seeds(view, k,
    generator).  A pixel with a NaN component gets label -1; an empty cluster keeps its centre (sklearn relocates it).  The
    host waits once per eight iterations and once at the end."""
    single, maps = _views(normals, "normals", ",3", 3)
    seeds = _check_init(init, k, None if isinstance(init, str) else len(maps), single)
    if int(max_iter) < 1:
        raise ValueError(f"max_iter must be at least 1 (got {max_iter})")
    if not float(tol) >= 0.0:
        raise ValueError(f"tol must not be negative (got {tol})")
    if seeds is not None and len(seeds) != len(maps):
        raise ValueError(f"{len(maps)} views but {len(seeds)} init arrays")
    dev, maps = _check_maps(maps, "normals", None, (torch.float32,), (3,))
    V = len(maps)
    if V == 0:
        return [], [], [], []
    if seeds is None:
        seeds = np.stack([kmeanspp_seeds(m, int(k), generator) for m in maps])
    K = seeds.shape[1]
    labels = [torch.empty(m.shape[:2], dtype=torch.int8, device=dev) for m in maps]
    centres = torch.empty((V, K, 3), dtype=torch.float32, device=dev)
    counts = torch.empty((V, K), dtype=torch.int32, device=dev)
    n_iter = host_array(_lib.c_i, [0] * V)
    sizes = _sizes(maps)
    launch(dev, "g4s_kmeans_normals", V, sizes, _lib.ptrs(maps), K, host_array(_lib.c_f, seeds.reshape(-1).tolist()),
           int(max_iter), float(tol), _lib.ptrs(labels), _lib.ptr(centres), _lib.ptr(counts), n_iter,
           workspace=_lib.load().g4s_kmeans_normals_workspace(V, sizes), sync=True)
    return _unwrap(single, labels, list(centres.unbind(0)), list(counts.unbind(0)), [n_iter[v] for v in range(V)])


# ---- 2. the pick and merge of clusters (host) ---------------------------------------------------------------------------
def _top(counts, n):
    return sorted(range(len(counts)), key=lambda j: (-int(counts[j]), j))[:n]


def merge_normal_clusters(counts, sorted_topk, centres):
    """planes/tools.py merge_normal_clusters over the cluster sizes instead of the label image: the table label -> rank
    (int32 [K], -1 = dropped; merged labels share a rank).  sorted_topk: the picked labels, largest first.  Pairs of picked
    clusters in that order whose normalised centres have a dot product above 0.95 merge into the earlier one; when anything
    merged, the pick is taken again over the merged counts of ALL K labels.  A label outside sorted_topk has no more members
    than any picked one, so the second pick admits it only at a tie of counts: it does when it is the smaller label."""
    counts = np.asarray(to_np(counts), np.int64).reshape(-1)
    c = np.asarray(to_np(centres), np.float64).reshape(-1, 3)
    K = len(counts)
    top = [int(t) for t in sorted_topk]
    if len(c) != K or not 1 <= K <= MAX_K or len(set(top)) != len(top) or any(not 0 <= t < K for t in top):
        raise ValueError(f"counts [K], centres [K,3], K in 1 .. {MAX_K}, and distinct picked labels below K")
    with np.errstate(invalid="ignore", divide="ignore"):
        c = c / np.linalg.norm(c, axis=1, keepdims=True)
    target, merged, kept = list(range(K)), [False] * len(top), len(top)
    for i in range(len(top)):
        if merged[i]:
            continue
        for j in range(i + 1, len(top)):
            if not merged[j] and np.dot(c[top[i]], c[top[j]]) > 0.95:
                target[top[j]] = top[i]
                merged[j] = True
                kept -= 1
    if kept != len(top):
        new_counts = np.zeros(K, np.int64)
        np.add.at(new_counts, target, counts)
        top = _top(new_counts, kept)
    rank = {label: r for r, label in enumerate(top)}
    return np.array([rank.get(target[j], -1) for j in range(K)], np.int32)


def select_normal_clusters(counts, centres, n_clusters=6):
    """The reference's pick of the n_clusters largest clusters followed by merge_normal_clusters: label -> rank, int32 [K].
    Where counts tie the smaller label ranks first; numpy's argpartition, which the reference uses, leaves that order
    unspecified."""
    counts = np.asarray(to_np(counts), np.int64).reshape(-1)
    return merge_normal_clusters(counts, _top(counts, min(int(n_clusters), len(counts))), centres)


# ---- 3. opening and components ----------------------------------------------------------------------------------------------
def _components(dev, labels, luts, min_sizes, do_open, want_opened):
    """Lists in, lists out: (components, sizes, n, opened or None)."""
    V = len(labels)
    lut_rows = []
    for v, lut in enumerate(luts):
        lut = np.asarray(to_np(lut), np.int64).reshape(-1)
        if len(lut) > MAX_K or ((lut < -1) | (lut >= MAX_K)).any():
            raise ValueError(f"lut[{v}]: at most {MAX_K} labels with ranks in -1 .. {MAX_K - 1}")
        lut_rows.extend(lut.tolist() + [-1] * (MAX_K - len(lut)))
    floors = [max(1, int(math.ceil(m))) for m in min_sizes]  # size >= m for an integer size
    comps = [torch.empty(l.shape, dtype=torch.int32, device=dev) for l in labels]
    opened = [torch.empty(l.shape, dtype=torch.int8, device=dev) for l in labels] if want_opened else None
    n = host_array(_lib.c_i, [0] * V)
    sizes = _sizes(labels)
    ws = launch(dev, "g4s_normal_components_count", V, sizes, _lib.ptrs(labels), host_array(_lib.c_i, lut_rows), 1 if do_open else 0,
                host_array(_lib.c_i, floors), _lib.ptrs(opened) if want_opened else None, _lib.ptrs(comps), n,
                workspace=_lib.load().g4s_normal_components_workspace(V, sizes))
    counts = [n[v] for v in range(V)]
    comp_sizes = [torch.empty(c, dtype=torch.int32, device=dev) for c in counts]
    launch(dev, "g4s_normal_components_sizes", V, sizes, n, _lib.ptrs([s if s.numel() else None for s in comp_sizes]),
           workspace=ws, sync=True)
    return comps, comp_sizes, counts, opened


def normal_components(labels, lut, min_size, open=True, return_opened=False):
    """(components int32 [H,W] with -1 for none, sizes int32 [n], n): the 9x9 opening of every rank's mask (OpenCV's borders:
    the erode takes pixels outside the image as members, the dilate as non-members) and its 8-connected components of at
    least min_size pixels, numbered by (rank, first pixel in raster order).  labels int8 [H,W]; lut: label -> rank or -1
    (select_normal_clusters).  open=False labels the ranks as they are.  return_opened adds the opened ranks, int8 [H,W].
    This is remove_small_isolated_areas and the second cv2.connectedComponents of normals_cluster; the equality is the
    library's stated rule (the blur's result is discarded there, Otsu of a {0, 255} image is the identity), not a
    measured one."""
    single, maps = _views(labels, "labels", "", 2)
    luts = [lut] if single else list(lut)
    check_view_count(luts, "lut", len(maps))
    min_sizes = _per_view(min_size, len(maps), "min_size")
    dev, maps = _check_maps(maps, "labels", None, (torch.int8,))
    if not maps:
        return ([], [], []) + (([],) if return_opened else ())
    comps, sizes, n, opened = _components(dev, maps, luts, min_sizes, open, return_opened)
    return _unwrap(single, comps, sizes, n, *([opened] if return_opened else []))


def _cluster(dev, normals, n_init_clusters, n_clusters, min_size_ratio, init, generator):
    """Steps 1-3 over checked views: (components, n) lists."""
    labels, centres, counts, _n_iter = kmeans_normals(normals, init, k=n_init_clusters, generator=generator)
    counts_h, centres_h = to_np(torch.stack(counts)), to_np(torch.stack(centres))  # one read-back for all views
    luts = [select_normal_clusters(counts_h[v], centres_h[v], n_clusters) for v in range(len(normals))]
    bars = [min_plane_size(m.shape, min_size_ratio) for m in normals]
    comps, _sizes_, n, _opened = _components(dev, labels, luts, bars, True, False)
    return comps, n


def normals_cluster(normals, img_shape=None, n_init_clusters=8, n_clusters=6, min_size_ratio=0.004, init="k-means++",
                    generator=None):
    """planes/plane_excavator.py normals_cluster: the list of boolean [H,W] masks of the normal components of one view
    ([H,W,3], or [H*W,3] with img_shape), or a list of such lists for several views."""
    if isinstance(normals, torch.Tensor) and normals.dim() == 2 and img_shape is not None:
        normals = normals.reshape(int(img_shape[0]), int(img_shape[1]), 3)
    single, maps = _views(normals, "normals", ",3", 3)
    _check_init(init, n_init_clusters, len(maps), single)
    dev, maps = _check_maps(maps, "normals", None, (torch.float32,), (3,))
    if not maps:
        return []
    comps, n = _cluster(dev, maps, n_init_clusters, n_clusters, min_size_ratio, init, generator)
    out = [[c == i for i in range(k)] for c, k in zip(comps, n)]
    return out[0] if single else out


# ---- 4. the join with the masks ---------------------------------------------------------------------------------------------
def assign_pair_ids(pair_counts, order, bar):
    """The reference's first double loop over the counts C [M,n]: masks in `order`, components in id order, a pair with C >=
    bar takes the next id (from 1).  Returns (pair_ids int32 [M,n], 0 = none; count)."""
    C = np.asarray(pair_counts)
    if C.ndim != 2 or C.shape[0] != len(order):
        raise ValueError(f"pair_counts must be [M,n] with one row per mask of the order (got {C.shape})")
    ids = np.zeros(C.shape, np.int32)
    count = 0
    for m in order:
        for c in range(C.shape[1]):
            if C[m, c] < bar:
                continue
            count += 1
            ids[m, c] = count
    return ids, count


def renumber_planes(id_areas, count, max_planes, bar):
    """The reference's second loop: ids 1 .. min(max_planes, count) whose painted area is at least `bar` are renumbered from
    1 in order; every other id becomes 0.  Returns (relabel int32 [count + 1], areas int64 [n_planes])."""
    relabel = np.zeros(count + 1, np.int32)
    areas = []
    for i in range(min(int(max_planes), count)):
        if id_areas[i + 1] < bar:
            continue
        areas.append(int(id_areas[i + 1]))
        relabel[i + 1] = len(areas)
    return relabel, np.array(areas, np.int64)


def mean_normals(sums, areas):
    """float64 [n,3]: the fixed-point sums [n,3] int64 / 2^32 / area, normalised."""
    avg = np.asarray(sums, np.int64).astype(np.float64) / 4294967296.0 / np.asarray(areas, np.float64)[:, None]
    return avg / np.sqrt((avg ** 2).sum(axis=1, keepdims=True))


def _join(dev, normals, masks, comps, n_comps, bars, max_planes):
    """Lists in, list of PlaneMasks out.  Three launches and three read-backs for all views."""
    V = len(normals)
    lib = _lib.load()
    sizes = _sizes(normals)
    M = [int(m.shape[0]) for m in masks]
    n_masks, n_components = host_array(_lib.c_i, M), host_array(_lib.c_i, n_comps)
    mask_ptrs = _lib.ptrs([m if m.numel() else None for m in masks])
    comp_ptrs = _lib.ptrs(comps)
    total_masks, total_pairs = sum(M), sum(m * n for m, n in zip(M, n_comps))
    areas = torch.empty(max(total_masks, 1), dtype=torch.int32, device=dev)
    pairs = torch.empty(max(total_pairs, 1), dtype=torch.int32, device=dev)
    launch(dev, "g4s_plane_pair_counts", V, sizes, comp_ptrs, mask_ptrs, n_masks, n_components, _lib.ptr(areas), _lib.ptr(pairs),
           workspace=lib.g4s_plane_pair_counts_workspace(V), sync=True)
    areas_h, pairs_h = to_np(areas), to_np(pairs)
    order, pair_ids, counts = [], [], []
    mb = pb = 0
    for v in range(V):
        o = np.argsort(areas_h[mb:mb + M[v]], kind="stable")  # sorted(masks, key=np.sum): stable, ascending
        ids, count = assign_pair_ids(pairs_h[pb:pb + M[v] * n_comps[v]].reshape(M[v], n_comps[v]), o, bars[v])
        order.extend(o.tolist())
        pair_ids.extend(ids.reshape(-1).tolist())
        counts.append(count)
        mb += M[v]
        pb += M[v] * n_comps[v]
    seg = [torch.empty(m.shape[:2], dtype=torch.int32, device=dev) for m in normals]
    seg_ptrs = _lib.ptrs(seg)
    n_ids = host_array(_lib.c_i, counts)
    total_ids = sum(counts) + V
    id_areas = torch.empty(total_ids, dtype=torch.int32, device=dev)
    launch(dev, "g4s_plane_paint", V, sizes, comp_ptrs, mask_ptrs, n_masks, n_components, host_array(_lib.c_i, order),
           host_array(_lib.c_i, pair_ids), n_ids, seg_ptrs, _lib.ptr(id_areas),
           workspace=lib.g4s_plane_paint_workspace(V, total_masks, total_pairs), sync=True)
    id_areas_h = to_np(id_areas)
    relabel, plane_areas = [], []
    ib = 0
    for v in range(V):
        r, a = renumber_planes(id_areas_h[ib:ib + counts[v] + 1], counts[v], max_planes, bars[v])
        relabel.extend(r.tolist())
        plane_areas.append(a)
        ib += counts[v] + 1
    n_planes = [len(a) for a in plane_areas]
    sums = torch.empty((sum(n_planes) + V, 3), dtype=torch.int64, device=dev)
    launch(dev, "g4s_plane_relabel", V, sizes, seg_ptrs, _lib.ptrs(normals), n_ids, host_array(_lib.c_i, relabel),
           host_array(_lib.c_i, n_planes), _lib.ptr(sums), workspace=lib.g4s_plane_relabel_workspace(V, total_ids), sync=True)
    sums_h = to_np(sums)
    out = []
    sb = 0
    for v in range(V):
        p = n_planes[v]
        if p == 0:
            out.append(PlaneMasks(seg[v], None, None))
        else:
            out.append(PlaneMasks(seg[v], mean_normals(sums_h[sb + 1:sb + 1 + p], plane_areas[v]), plane_areas[v]))
        sb += p + 1
    return out


def join_planes(normals, sam_masks, components, n_components, min_size, max_planes=100):
    """PlaneExcavator.__call__ after the clustering and the network, from given normal components (int32 [H,W], -1 = none,
    n_components of them): PlaneMasks(seg_mask int32 [H,W], normal float64 [n,3] or None, areas int64 [n] or None).  Masks
    ascending by area (stable), components in id order; a pair with at least min_size common pixels takes the next id and
    paints its pixels over earlier ids; of the first max_planes ids those that still cover min_size pixels are renumbered
    from 1; `normal` is their normalised mean normal."""
    single, maps = _views(normals, "normals", ",3", 3)
    masks = [sam_masks] if single else list(sam_masks)
    comps = [components] if single else list(components)
    n_comps = [int(n) for n in _per_view(n_components, len(maps), "n_components")]
    bars = _per_view(min_size, len(maps), "min_size")
    dev, maps = _check_maps(maps, "normals", None, (torch.float32,), (3,))
    _d, comps = _check_maps(comps, "components", dev, (torch.int32,), (), _shapes(maps), len(maps))
    masks = _check_masks(masks, dev, _shapes(maps))
    if any(n < 0 for n in n_comps):
        raise ValueError("n_components must not be negative")
    if not maps:
        return []
    out = _join(dev, maps, masks, comps, n_comps, bars, max_planes)
    return out[0] if single else out


def excavate_planes(normals, sam_masks, min_size_ratio=0.004, n_init_normal_clusters=8, n_normal_clusters=6,
                    num_sam_prompts=256, max_planes=100, init="k-means++", generator=None):
    """PlaneExcavator.__call__ with given normals and the masks of the caller's SAM run: PlaneMasks(seg_mask, normal, areas),
    the keys of the reference's outputs, per view.  The keywords are the fields of PlaneExcavatorConfig (num_sam_prompts
    is the caller's: the network is not run here) and the reference's constant of 100 planes.  init: the k-means seeds,
    see kmeans_normals."""
    single, maps = _views(normals, "normals", ",3", 3)
    masks = [sam_masks] if single else list(sam_masks)
    check_view_count(masks, "sam_masks", len(maps))
    _check_init(init, n_init_normal_clusters, len(maps), single)
    dev, maps = _check_maps(maps, "normals", None, (torch.float32,), (3,))
    masks = _check_masks(masks, dev, _shapes(maps))
    if not maps:
        return []
    comps, n = _cluster(dev, maps, n_init_normal_clusters, n_normal_clusters, min_size_ratio, init, generator)
    out = _join(dev, maps, masks, comps, n, [min_plane_size(m.shape, min_size_ratio) for m in maps], max_planes)
    return out[0] if single else out


# ---- the file the later stages read ----------------------------------------------------------------------------------------
def save_plane_mask(path, seg_mask):
    """np.save of the int32 [H,W] ids: plane_mask_frame*.npy."""
    np.save(path, np.asarray(to_np(seg_mask), np.int32))


def load_plane_mask(path, device=None):
    """The int32 [H,W] tensor of a plane_mask_frame*.npy (the reference's are uint8), on `device` if given."""
    seg = torch.from_numpy(np.load(path).astype(np.int32))
    return seg if device is None else seg.to(device)
