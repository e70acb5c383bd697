"""Golden vectors of the chart-surfel stage, produced by RUNNING THE REFERENCE'S OWN CODE on the CPU of the build container:

    chart_init.npz   matcha/dm_scene/charts.py `get_gaussian_parameters_from_pa_data`, imported and called for real, in
                     float32 and in float64.  That one call runs the reference's face construction
                     (matcha/dm_scene/meshes.py `get_manifold_meshes_from_pointmaps`), its elongated-face expression, its
                     face removal and matcha/dm_scene/gaussians.py `get_gaussian_surfel_parameters_from_mesh`.

Stand-ins, and what they mean for the golden.  pytorch3d is absent, so `pytorch3d` and its sub-modules are replaced in
sys.modules:
  * `Meshes`, `TexturesVertex` and `join_meshes_as_scene` are the few lines below: containers of the vertex, face and
    feature tensors the reference hands them.  `submeshes` keeps the chosen faces and does NOT renumber vertices (the
    reference only ever gathers vertices through faces, so the values are the same) and records the chosen face indices:
    that record is the reference's keep mask.
  * `matrix_to_quaternion` is tests/chart_init_ref.py's restatement.  THE GOLDEN'S QUATERNIONS THEREFORE PIN NOTHING BEYOND
    THE RESTATEMENT.  The matrices the reference passes to it are recorded: keep mask, means, scales, colours and the
    pre-quaternion rotation are the reference's.
  * every other pytorch3d name is an empty class that is never touched on this path.
The elongation ratios are internal to the reference's function; `ratio_th` is passed as an object that compares like the
number 5 and keeps the tensor it was compared with, so the recorded ratios are the reference's too.

Scene.  Seed 20, 2 views of 9 x 7 points.  View 0: a unit grid with mild noise (ratios well below 5).  View 1: columns
stretched by 1 .. 9 so that ratios fall on both sides of 5, and one vertex repeated (degenerate faces: a zero altitude,
the ratio is not finite, dropped).  Colours reach outside [0, 1].

main() asserts its own coverage: kept and dropped faces both exist in view 1, the degenerate faces are dropped, and at most
1 % of the faces are near the threshold (the float32 and float64 runs' relative ratio difference, see below).
Yardstick.  Per continuous output the largest |float32 run - float64 run| of the reference over the faces both runs keep;
for the rotation, of the matrices rebuilt from the two runs' quaternions; for the ratio, the largest RELATIVE difference over
the faces whose float64 ratio is finite and below 4 ratio_th (far above the threshold the ratio is ill-conditioned and
irrelevant).  A face is "near the threshold" when |ratio64 - ratio_th| <= yard_ratio * ratio_th.

Nothing of the reference is copied: the npz holds inputs and recorded results only.
Run in the build container only (needs /root/reference):  python tests/golden/make_golden_chart_init.py"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _ref_import import reference_modules  # noqa: E402
import chart_init_ref as cr  # noqa: E402

SEED, V, H, W = 20, 2, 9, 7
RATIO_TH = 5.0
NORMALIZED_SCALES, NORMAL_SCALE = 0.5, 1e-10
REPEATED = (1, 4, 3)  # view, row, column of the vertex that repeats its right neighbour


def make_inputs():
    rng = np.random.default_rng(SEED)
    r, c = np.mgrid[0:H, 0:W].astype(np.float64)
    pts = np.zeros((V, H, W, 3))
    pts[0] = np.stack([c, r, 4.0 + 0.15 * rng.standard_normal((H, W))], axis=-1) + 0.05 * rng.standard_normal((H, W, 3))
    stretch = np.cumsum(rng.uniform(1.0, 9.0, W))
    pts[1] = np.stack([np.broadcast_to(stretch, (H, W)), r, 6.0 + 0.3 * rng.standard_normal((H, W))], axis=-1)
    pts[1] += 0.05 * rng.standard_normal((H, W, 3))
    v, y, x = REPEATED
    pts[v, y, x] = pts[v, y, x + 1]
    images = rng.uniform(-0.2, 1.2, (V, H, W, 3))
    return pts.astype(np.float32), images.astype(np.float32)


# ---- the stand-ins ----------------------------------------------------------------------------------------------------------
class TexturesVertex:
    def __init__(self, verts_features):
        self.features = [f for f in verts_features]

    def verts_features_packed(self):
        return torch.cat(self.features, dim=0)


class Meshes:
    chosen = []  # the face indices of every submeshes call, in call order

    def __init__(self, verts, faces, textures=None):
        self.verts, self.faces, self.textures = list(verts), list(faces), textures

    def __len__(self):
        return len(self.verts)

    def to(self, device):
        return self

    def verts_packed(self):
        return torch.cat(self.verts, dim=0)

    def faces_packed(self):
        out, base = [], 0
        for v, f in zip(self.verts, self.faces):
            out.append(f + base)
            base += len(v)
        return torch.cat(out, dim=0)

    def submeshes(self, face_indices):
        idx = face_indices[0][0]
        Meshes.chosen.append(idx.clone())
        return Meshes([self.verts_packed()], [self.faces_packed()[idx]], TexturesVertex([self.textures.verts_features_packed()]))


def join_meshes_as_scene(meshes):
    return Meshes([torch.cat([m.verts_packed() for m in meshes])],
                  [torch.cat([m.faces_packed() + sum(len(p.verts_packed()) for p in meshes[:i]) for i, m in enumerate(meshes)])],
                  TexturesVertex([torch.cat([m.textures.verts_features_packed() for m in meshes])]))


class _Anything(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


class _Threshold:
    """Compares like `value` and keeps what it was compared with."""

    def __init__(self, value):
        self.value, self.seen = value, None

    def __gt__(self, other):
        self.seen = other
        return other < self.value


def _stubs(rotations):
    names = ["pytorch3d", "pytorch3d.structures", "pytorch3d.renderer", "pytorch3d.renderer.blending", "pytorch3d.renderer.mesh",
             "pytorch3d.renderer.mesh.shader", "pytorch3d.transforms", "pytorch3d.transforms.transform3d", "pytorch3d.ops",
             "pytorch3d.io", "pytorch3d.utils", "pytorch3d.renderer.cameras", "pytorch3d.loss"]
    mods = {n: _Anything(n) for n in names}
    mods["pytorch3d.structures"].Meshes = Meshes
    mods["pytorch3d.structures"].join_meshes_as_scene = join_meshes_as_scene
    mods["pytorch3d.renderer"].TexturesVertex = TexturesVertex

    def matrix_to_quaternion(R):
        rotations.append(R.clone())
        return torch.from_numpy(cr.matrix_to_quaternion(R.numpy()))

    mods["pytorch3d.transforms"].matrix_to_quaternion = matrix_to_quaternion
    return mods


def run_reference(points, images, dtype):
    """The reference's function on the CPU in `dtype`: its results, the keep mask, the ratios and the rotations."""
    rotations = []
    Meshes.chosen = []
    with reference_modules(_stubs(rotations)):
        sys.path.insert(0, "/root/reference")
        from matcha.dm_scene.charts import get_gaussian_parameters_from_pa_data
        th = _Threshold(RATIO_TH)
        out = get_gaussian_parameters_from_pa_data(torch.from_numpy(points).to(dtype), [torch.from_numpy(i).to(dtype) for i in images],
                                                   ratio_th=th, normal_scale=NORMAL_SCALE, normalized_scales=NORMALIZED_SCALES)
    n_faces = 2 * V * (H - 1) * (W - 1)
    keep = np.zeros(n_faces, bool)
    assert len(Meshes.chosen) == 1 and len(rotations) == 1 and th.seen is not None and len(th.seen) == n_faces
    keep[Meshes.chosen[0].numpy()] = True
    res = {k: out[k].numpy() for k in ("means", "scales", "quaternions", "colors")}
    res.update(keep=keep, ratio=th.seen.numpy(), rotations=rotations[0].numpy())
    assert all(res[k].dtype == (np.float32 if dtype == torch.float32 else np.float64) for k in ("means", "scales", "colors", "ratio"))
    return res


def main():
    points, images = make_inputs()
    # the constants of the contract are the reference's
    with reference_modules(_stubs([])):
        sys.path.insert(0, "/root/reference")
        from matcha.dm_scene.gaussians import get_regular_triangle_bary_coords
        bary = get_regular_triangle_bary_coords(1).numpy()
    assert bary.dtype == np.float32 and tuple(int(b) for b in bary.reshape(3).view(np.uint32)) == cr.BARY_BITS
    axes = np.array([[-np.sqrt(2) / 2, np.sqrt(2) / 2, 0.0], [-1 / np.sqrt(6), -1 / np.sqrt(6), 2 / np.sqrt(6)]]).astype(np.float32)
    assert tuple(int(b) for b in axes[0].view(np.uint32)) == cr.AXIS0_BITS and tuple(int(b) for b in axes[1].view(np.uint32)) == cr.AXIS1_BITS

    r32, r64 = run_reference(points, images, torch.float32), run_reference(points, images, torch.float64)
    both = r32["keep"] & r64["keep"]
    row32, row64 = np.cumsum(r32["keep"]) - 1, np.cumsum(r64["keep"]) - 1
    i32, i64 = row32[both], row64[both]
    yard = {k: float(np.abs(r32[k][i32].astype(np.float64) - r64[k][i64]).max()) for k in ("means", "scales", "colors")}
    yard["rotations"] = float(np.abs(cr.quaternion_to_matrix(r32["quaternions"][i32]) - cr.quaternion_to_matrix(r64["quaternions"][i64])).max())
    yard["pre_rotations"] = float(np.abs(r32["rotations"][i32].astype(np.float64) - r64["rotations"][i64]).max())
    ratio64 = r64["ratio"]
    with np.errstate(invalid="ignore"):
        relevant = np.isfinite(ratio64) & (ratio64 < 4 * RATIO_TH)
        yard["ratio"] = float((np.abs(r32["ratio"][relevant].astype(np.float64) - ratio64[relevant]) / ratio64[relevant]).max())
        near = np.abs(ratio64 - RATIO_TH) <= yard["ratio"] * RATIO_TH
    # coverage
    per_view = 2 * (H - 1) * (W - 1)
    k1 = r64["keep"][per_view:]
    assert k1.any() and (~k1).any() and r64["keep"][:per_view].all()
    assert (~np.isfinite(ratio64)).sum() >= 1 and not r64["keep"][~np.isfinite(ratio64)].any()
    assert near.sum() <= 0.01 * len(near), (int(near.sum()), len(near))
    assert np.array_equal(r32["keep"][~near], r64["keep"][~near])
    print(f"faces {len(near)}, kept {int(r64['keep'].sum())}, near the threshold {int(near.sum())}, non-finite ratios {int((~np.isfinite(ratio64)).sum())}")
    print("yardstick", yard)
    np.savez_compressed(os.path.join(HERE, "chart_init.npz"), points=points, images=images, ratio_th=np.float32(RATIO_TH),
                        normalized_scales=np.float32(NORMALIZED_SCALES), normal_scale=np.float32(NORMAL_SCALE),
                        ref64_keep=r64["keep"], ref32_keep=r32["keep"], ref64_ratio=ratio64, near=near,
                        ref64_means=r64["means"], ref64_scales=r64["scales"], ref64_colors=r64["colors"],
                        ref64_rotations=r64["rotations"], ref64_quaternions=r64["quaternions"], yardstick=json.dumps(yard))


if __name__ == "__main__":
    main()
