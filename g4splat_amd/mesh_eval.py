"""Mesh evaluation on the GPU: accuracy, completeness, Chamfer-L1, precision, recall, F-score, normal consistency.

The counterpart of 2d-gaussian-splatting/eval/mesh_eval.py (there: open3d's voxel_down_sample, trimesh's sample and
face_normals, four scikit-learn KDTree queries on the host), over the "mesh evaluation" section of
include/g4s_render_maps.h, which states the semantics (csrc/tsdf/mesh_eval.hip; tests/mesh_eval_ref.py restates them).

    dist, index = nearest_neighbors(ref, query)        # exact, smallest index on ties
    points = voxel_down_sample(points, voxel_size)     # voxels in ascending (cz, cy, cx)
    points, normals, face = sample_surface(mesh, count, generator)
    metrics = evaluate(mesh_pred, mesh_trgt)           # the reference's nine keys
    python -m g4splat_amd.mesh_eval --input_mesh a.ply --gt_mesh b.ply --output_txt metrics.txt

Meshes are mesh.TriangleMesh (numpy; uploaded) or mesh.DeviceMesh (tensors), clouds [n,3] arrays or tensors; results are
device tensors, and nothing returns to the host before evaluate's final dictionary.

Differences from the reference: points are float32 (open3d and trimesh work in float64); the down-sample has an order
(open3d's is a hash map's); sampling draws from torch's generator, not numpy's global state, so the normal figures agree
with the reference statistically and not sample for sample; the sampler's face search uses side='right', so a face of
zero area is never chosen; an empty cloud raises ValueError (the reference returns NaN).
"""
import argparse

import numpy as np
import torch

from . import _lib
from ._device import default_device, launch, voxel_downsample_count
from .mesh import TriangleMesh, as_device_mesh

METRIC_KEYS = ("Acc", "Comp", "Chamfer-L1", "Prec", "Recal", "F-score", "Normal-Acc", "Normal-Comp", "Normal-Consistency")


def _cloud(points, device=None, what="points"):
    """[n,3] float32 contiguous tensor on a HIP device (an array is uploaded to `device` or the current one)."""
    if isinstance(points, torch.Tensor):
        if points.device.type != "cuda":
            raise RuntimeError(f"{what} must be a HIP tensor or a numpy array (there is no CPU path)")
        t = points
    else:
        dev = torch.device(device) if device is not None else default_device()
        t = torch.as_tensor(np.ascontiguousarray(points, np.float32), device=dev)
    if t.dim() != 2 or t.size(1) != 3:
        raise ValueError(f"{what} must be [n,3], got {tuple(t.shape)}")
    return t.float().contiguous()


def nearest_neighbors(ref, query):
    """(dist [n_query] float32 = sqrt of the library's squared distance, index [n_query] int32) of every query's nearest
    reference point; ties go to the smallest index, and a query with no finite candidate gets (sqrt(FLT_MAX), -1)."""
    lib = _lib.load()
    dev = next((t.device for t in (ref, query) if isinstance(t, torch.Tensor)), None)
    ref = _cloud(ref, dev, "ref")
    query = _cloud(query, ref.device, "query")
    if ref.device != query.device:
        raise RuntimeError("ref and query live on different devices")
    n_ref, n_query = ref.size(0), query.size(0)
    if n_ref == 0:
        raise ValueError("nearest_neighbors: the reference cloud is empty")
    dev = ref.device
    d2 = torch.empty(n_query, dtype=torch.float32, device=dev)
    idx = torch.empty(n_query, dtype=torch.int32, device=dev)
    launch(dev, "g4s_nn_search", n_ref, _lib.ptr(ref), n_query, _lib.ptr(query), _lib.ptr(d2), _lib.ptr(idx),
           workspace=lib.g4s_nn_workspace(n_ref, n_query))
    return torch.sqrt(d2), idx


def voxel_down_sample(points, voxel_size):
    """One point per occupied voxel of edge `voxel_size`: the float64 mean of the voxel's points, as float32."""
    pts = _cloud(points)
    n, dev = pts.size(0), pts.device
    if n == 0:
        raise ValueError("voxel_down_sample: the cloud is empty")
    ws, count = voxel_downsample_count(pts, voxel_size, "voxel_down_sample")
    out = torch.empty((count, 3), dtype=torch.float32, device=dev)
    launch(dev, "g4s_voxel_downsample_emit", n, _lib.ptr(pts), count, _lib.ptr(out), workspace=ws)
    return out


def cumulative_areas(mesh):
    """[F] float64 on the device: the inclusive running sum of the face areas (float64 from the float32 vertices).  A face
    that names a vertex outside the mesh has no area, so it is never drawn."""
    v = mesh.vertices.double()
    t = mesh.triangles.long()
    ok = ((t >= 0) & (t < v.size(0))).all(dim=1)
    t = t.clamp(0, v.size(0) - 1)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    area = 0.5 * torch.linalg.cross(b - a, c - a).norm(dim=1)
    return torch.cumsum(torch.where(ok, area, torch.zeros_like(area)), 0)


def sample_surface(mesh, count, generator=None, u=None, cum_area=None):
    """`count` points uniform over the mesh's area: (points [count,3], normals [count,3] = their faces' unit normals,
    face_index [count] int32), device tensors.  The three random numbers of a sample come from torch.rand under
    `generator` (a generator of the mesh's device), or from `u` [count,3]; `cum_area` defaults to cumulative_areas."""
    dm, _host = as_device_mesh(mesh)
    dev = dm.vertices.device
    n_tri, n_vert = dm.triangles.size(0), dm.vertices.size(0)
    if n_tri == 0 or n_vert == 0:
        raise ValueError("sample_surface: the mesh has no triangles")
    count = int(count)
    with torch.cuda.device(dev):
        if u is None:
            u = torch.rand((count, 3), dtype=torch.float32, device=dev, generator=generator)
        u = _cloud(u, dev, "u")
        if u.size(0) != count:
            raise ValueError(f"u must be [{count},3], got {tuple(u.shape)}")
        if cum_area is None:
            cum_area = cumulative_areas(dm)
        cum_area = cum_area.to(device=dev, dtype=torch.float64).contiguous()
        points = torch.empty((count, 3), dtype=torch.float32, device=dev)
        normals = torch.empty_like(points)
        face = torch.empty(count, dtype=torch.int32, device=dev)
        _lib.call("g4s_mesh_sample_surface", count, _lib.ptr(u), _lib.ptr(cum_area), n_tri, _lib.ptr(dm.triangles), n_vert,
                  _lib.ptr(dm.vertices), _lib.ptr(points), _lib.ptr(normals), _lib.ptr(face), _lib.stream(dev))
    return points, normals, face


def metrics_from_parts(dist_acc, dist_comp, normal_acc, normal_comp, threshold):
    """The reference's nine figures from: dist_acc = every predicted point's distance to the target cloud, dist_comp =
    every target point's distance to the predicted cloud, normal_acc / normal_comp = |n . n'| of every predicted / target
    sample with its nearest sample of the other mesh.  Means and the threshold test in float64; one host read."""
    f64 = torch.float64
    parts = torch.stack([dist_acc.to(f64).mean(), dist_comp.to(f64).mean(), (dist_acc.to(f64) < threshold).to(f64).mean(),
                         (dist_comp.to(f64) < threshold).to(f64).mean(), normal_acc.to(f64).mean(), normal_comp.to(f64).mean()])
    acc, comp, prec, recal, n_acc, n_comp = parts.tolist()
    fscore = 2.0 * prec * recal / (prec + recal) if prec + recal > 0.0 else float("nan")
    return {"Acc": acc * 100, "Comp": comp * 100, "Chamfer-L1": (acc + comp) / 2 * 100, "Prec": prec * 100, "Recal": recal * 100,
            "F-score": fscore * 100, "Normal-Acc": n_acc * 100, "Normal-Comp": n_comp * 100,
            "Normal-Consistency": (n_acc + n_comp) * 0.5 * 100}


def _abs_dot(a, b):
    """|a . b| per row in float64: the products of float32 values are exact there, summed (x + y) + z."""
    p = a.double() * b.double()
    return ((p[:, 0] + p[:, 1]) + p[:, 2]).abs()


def evaluate(mesh_pred, mesh_trgt, threshold=0.05, down_sample=0.02, n_samples=200000, generator=None):
    """The reference's metrics of a predicted mesh against the target (eval/mesh_eval.py evaluate): distances between the
    voxel-down-sampled vertex clouds (down_sample = 0 or None: the vertices as they are), and the agreement of the face
    normals at `n_samples` surface samples a mesh, each paired with the nearest sample of the other mesh."""
    pred, _ = as_device_mesh(mesh_pred)
    trgt, _ = as_device_mesh(mesh_trgt, pred.vertices.device)
    if pred.vertices.size(0) == 0 or trgt.vertices.size(0) == 0:
        raise ValueError("evaluate: a mesh has no vertices")
    verts_pred, verts_trgt = pred.vertices, trgt.vertices
    if down_sample:
        verts_pred, verts_trgt = voxel_down_sample(verts_pred, down_sample), voxel_down_sample(verts_trgt, down_sample)
    dist_comp, _ = nearest_neighbors(verts_pred, verts_trgt)
    dist_acc, _ = nearest_neighbors(verts_trgt, verts_pred)
    pts_pred, nrm_pred, _ = sample_surface(pred, n_samples, generator)
    pts_trgt, nrm_trgt, _ = sample_surface(trgt, n_samples, generator)
    _, near_pred = nearest_neighbors(pts_pred, pts_trgt)  # per target sample
    _, near_trgt = nearest_neighbors(pts_trgt, pts_pred)  # per predicted sample
    normal_acc = _abs_dot(nrm_pred, nrm_trgt[near_trgt.long()])
    normal_comp = _abs_dot(nrm_trgt, nrm_pred[near_pred.long()])
    return metrics_from_parts(dist_acc, dist_comp, normal_acc, normal_comp, threshold)


def eval_mesh(input_mesh_path, gt_mesh_path):
    from . import ply_io
    return evaluate(TriangleMesh(*ply_io.read_triangle_mesh(input_mesh_path)), TriangleMesh(*ply_io.read_triangle_mesh(gt_mesh_path)))


def main(argv=None):
    parser = argparse.ArgumentParser(description="Scores a reconstructed mesh against the ground truth on the GPU.")
    parser.add_argument("--input_mesh", type=str, required=True, help="PLY of the mesh to score")
    parser.add_argument("--gt_mesh", type=str, required=True, help="PLY of the ground-truth mesh")
    parser.add_argument("--output_txt", type=str, required=True, help="text file the metrics are appended to")
    args = parser.parse_args(argv)
    lines = [f"{k}: {v}" for k, v in eval_mesh(args.input_mesh, args.gt_mesh).items()]
    print("\n".join(lines))
    with open(args.output_txt, "a") as f:
        f.write("".join(line + "\n" for line in lines))


if __name__ == "__main__":
    main()
