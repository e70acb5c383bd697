"""Golden vectors of the tetrahedral mesh extraction, produced by RUNNING THE REFERENCE'S OWN CODE on the CPU of the build
container:

    tetra_tsdf.npz   matcha/dm_extractors/adaptive_tsdf.py `AdaptiveTSDF` (integrate with its default flags, one call per
                     view, as extract_mesh_adaptive_tsdf.py:146-204 drives it) at sample points and at the points of a
                     Kuhn lattice, and 2d-gaussian-splatting/utils/tetmesh.py `marching_tetrahedra` over that lattice with
                     the field the reference computed on it.  Both files are imported by path, with an empty stand-in for
                     matcha.dm_scene.cameras (only a type annotation uses it) and SimpleNamespace cameras.

Samples.  The contract (include/g4s_render_maps.h) and the reference decide "is this view used" from float32 values that
they compute in different operation orders, so a point that lies on a decision boundary may be decided differently.  Every
sample within 1e-3 px of a frustum bound (ix = 0, W - 1; iy = 0, H - 1) or within 1e-4 trunc of the -trunc bound in any
view is dropped HERE; the test excludes nothing.  The lattice field is recorded as an input of the marching tetrahedra
(which only reads its signs), not compared.

Tolerance.  The one intended difference is grid_sample's float32 round trip (pixel -> [-1, 1] -> pixel) and torch's own
operation order; the largest |reference - restatement| over the kept samples is measured here (tests/tetra_ref.py in
float32) and tol = 4 x that is stored with it.

Nothing of the reference is copied: the npz holds inputs and recorded results only.
Run in the build container only (needs /root/reference):  python tests/golden/make_golden_tetra.py"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

REF = "/root/reference"
TRUNC = 0.1
LATTICE_N, LATTICE_HALF = 9, 1.4  # 9^3 points over [-1.4, 1.4]^3: 3072 tets around the unit sphere


def _load(name, path, stubs=()):
    saved = {k: sys.modules.get(k) for k in stubs}
    for k in stubs:
        sys.modules[k] = types.ModuleType(k)
    if "matcha.dm_scene.cameras" in stubs:
        sys.modules["matcha.dm_scene.cameras"].GSCamera = object
    try:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                del sys.modules[k]
            else:
                sys.modules[k] = v
    return mod


def run_reference_tsdf(ref, points, views):
    field = ref.AdaptiveTSDF(points=torch.tensor(points), trunc_margin=TRUNC)
    for _cam, Wv, Pm, depth, rgb in views:
        H, W = depth.shape
        cam = types.SimpleNamespace(world_view_transform=torch.tensor(Wv), projection_matrix=torch.tensor(Pm),
                                    full_proj_transform=torch.tensor(Wv) @ torch.tensor(Pm), image_height=H, image_width=W)
        field.integrate(img=torch.tensor(rgb), depth=torch.tensor(depth), camera=cam)
    out = field.return_field_values()
    return out["tsdf"].reshape(-1).numpy().copy(), out["colors"].reshape(-1, 3).numpy().copy()


def decision_margins(points, views):
    """(distance in px to the nearest frustum bound, |diff + trunc| / trunc where the point is inside) over all views."""
    import tetra_ref as tr
    px = np.full(len(points), np.inf)
    tm = np.full(len(points), np.inf)
    for _cam, Wv, Pm, depth, _rgb in views:
        H, W = depth.shape
        ix, iy, z = (a.astype(np.float64) for a in tr.pixel_coordinates(points, (Wv, Pm, depth)))
        px = np.minimum(px, np.min([np.abs(ix), np.abs(ix - (W - 1)), np.abs(iy), np.abs(iy - (H - 1))], 0))
        inside = (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1) & (z > 1e-6)
        idx = np.nonzero(inside)[0]
        x0, y0 = np.floor(ix[idx]).astype(int), np.floor(iy[idx]).astype(int)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        fx, fy = ix[idx] - x0, iy[idx] - y0
        D = depth.astype(np.float64)
        d = D[y0, x0] * (1 - fx) * (1 - fy) + D[y0, x1] * fx * (1 - fy) + D[y1, x0] * (1 - fx) * fy + D[y1, x1] * fx * fy
        tm[idx] = np.minimum(tm[idx], np.abs(d - z[idx] + TRUNC) / TRUNC)
    return px, tm


def main():
    import tetra_ref as tr
    ref_tsdf = _load("ref_adaptive_tsdf", os.path.join(REF, "matcha", "dm_extractors", "adaptive_tsdf.py"),
                     stubs=("matcha", "matcha.dm_scene", "matcha.dm_scene.cameras"))
    ref_tet = _load("ref_tetmesh", os.path.join(REF, "2d-gaussian-splatting", "utils", "tetmesh.py"))
    views = tr.sphere_views(64, 48, background=0.0, seed=7)
    rng = np.random.default_rng(2025)
    n = 6000
    pts = rng.uniform(-1.8, 1.8, (n, 3))
    s = rng.normal(size=(n // 2, 3))
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    pts[: n // 2] = s * rng.uniform(0.85, 1.15, (n // 2, 1))  # half of them in the band around the surface
    pts = pts.astype(np.float32)
    px, tm = decision_margins(pts, views)
    keep = (px >= 1e-3) & (tm >= 1e-4)
    pts = np.ascontiguousarray(pts[keep])
    tsdf, cols = run_reference_tsdf(ref_tsdf, pts, views)
    assert tsdf.dtype == np.float32 and cols.dtype == np.float32
    my_t, my_c, used = tr.adaptive_tsdf(pts, [v[1:] for v in views], TRUNC)
    err_t, err_c = float(np.abs(my_t.astype(np.float64) - tsdf).max()), float(np.abs(my_c.astype(np.float64) - cols).max())
    tol = 4.0 * max(err_t, err_c)

    lat, tets = tr.kuhn_lattice(LATTICE_N)
    lat = ((lat / np.float32(LATTICE_N - 1)) * np.float32(2 * LATTICE_HALF) - np.float32(LATTICE_HALF)).astype(np.float32)
    lat_sdf, _c = run_reference_tsdf(ref_tsdf, lat, views)
    verts, _scales, faces, interp_v = ref_tet.marching_tetrahedra(torch.tensor(lat)[None], torch.tensor(tets).long(),
                                                                  torch.tensor(lat_sdf)[None], torch.ones(1, len(lat), 1))
    edges, faces = interp_v[0].numpy().astype(np.int32), faces[0].numpy().astype(np.int32)

    out = {"trunc": np.float64(TRUNC), "points": pts, "tsdf": tsdf, "colors": cols, "tol": np.float64(tol),
           "max_err": np.array([err_t, err_c]), "n_dropped": np.int64((~keep).sum()), "lattice": lat, "tets": tets,
           "lattice_sdf": lat_sdf, "edges": edges, "faces": faces}
    for i, (_cam, Wv, Pm, depth, rgb) in enumerate(views):
        out[f"v{i}_wv"], out[f"v{i}_pm"], out[f"v{i}_depth"], out[f"v{i}_rgb"] = Wv, Pm, depth, rgb
    path = os.path.join(HERE, "tetra_tsdf.npz")
    np.savez_compressed(path, **out)
    print(f"wrote tetra_tsdf.npz {os.path.getsize(path)} bytes; {len(pts)} samples ({int((~keep).sum())} dropped), "
          f"{int(used.any(1).sum())} seen, {int((tsdf > 0).sum())} positive; max |ref - restatement| tsdf {err_t:.3e}, "
          f"colour {err_c:.3e}, tol = {tol:.3e}; lattice: {len(tets)} tets, {len(edges)} crossing edges, {len(faces)} faces")


if __name__ == "__main__":
    main()
