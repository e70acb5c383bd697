"""Golden vectors of the cross-view consistency stage, produced by RUNNING THE REFERENCE'S OWN SCRIPTS on the CPU of the
build container:

    consistency.npz   guidance/inconsistence_solver.py and guidance/plane_inconsistency_solver.py, run for real through
                      runpy as `__main__` over a temporary directory of the files they read (refine_depth_frame*.tiff,
                      rgb_frame*.png, plane_mask_frame*.npy, refine_points_frame*.ply, global_3Dplane_ID_dict.json, the
                      anchor json, an empty inpainted_images/), with torch on one thread.  Recorded: the inputs, and what
                      the scripts wrote -- the confident maps and repainted PNGs of the point solver, the repainted PNGs
                      of the plane solver.

The import stand-ins are make_golden_visibility._stubs() plus: scene.dataset_readers.load_cameras / load_see3d_cameras
returning camera namespaces (R, T, FoVx, FoVy, image_width, image_height, original_image = u8 / 255 as [3,H,W]), an
`arguments.ModelParams` with `extract`, no-op utils.general_utils.safe_state / seed_everything, a `trimesh.load` whose
`.vertices` are read from the file, and a CPU float32 cam_utils.to_tensor_safe.

Scene.  The five 64 x 48 cameras and unit-sphere depth maps of the visibility golden, reordered [2, 0, 1, 3, 4]: ONE input
view and four inpainted views.  Clouds: each view's depth back-projected at PIXEL CENTRES (x + 0.5, y + 0.5) in float64
through the inverse of world_view_transform, rounded to float32 (the visibility golden's own clouds sit at integer
pixels, where a view's own points land on truncation boundaries and float32 and float64 disagree on 9 % of the
decisions).  Images: default_rng(0) uint8.  Masks: 3 * face + 20 * view + 2, face 1 .. 6 the cube face of the pixel's point,
0 on the background.  Dict: six planes in face order [4, 1, 6, 2, 5, 3], their pairs in view order range(V) for even k and
[3, 0, 4, 1, 2] for odd k, views without a pixel of the face left out.  Anchors [3, 0, 1].

Decisions.  torch orders its matmul differently from the contract, so the restatement (tests/consistency_ref.py) is run
in float32 and the pixels on which it differs from what the scripts wrote are recorded as excluded; the agreed set may
leave out at most 0.1 % per solver and per output (asserted).  main() also asserts that the scene keeps the properties the
tests lean on: order-sensitive duplicates, changed pixels, confident-map zeros, chains of length two, own-view anchors,
more than one anchor.

Nothing of the reference is copied: the npz holds inputs and recorded results only.
Run in the build container only (needs /root/reference):  python tests/golden/make_golden_consistency.py"""
import json
import math
import os
import runpy
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_visibility as mgv  # noqa: E402
from _ref_import import REF, reference_modules  # noqa: E402
from make_golden_planes import cube_face  # noqa: E402

W, H = mgv.W, mgv.H
VIEW_ORDER = [2, 0, 1, 3, 4]
N_INPUT = 1
FACE_ORDER = [4, 1, 6, 2, 5, 3]
ODD_VIEW_ORDER = [3, 0, 4, 1, 2]
ANCHORS = [3, 0, 1]
THRESHOLD = 0.1  # both scripts hard-code it
CAP = 0.001


def make_inputs():
    g = np.load(os.path.join(HERE, "visibility_grid.npz"))
    V = len(VIEW_ORDER)
    cams, depths, clouds, masks = [], [], [], []
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for v, src in enumerate(VIEW_ORDER):
        cam = types.SimpleNamespace(world_view_transform=g["wvt"][src], full_proj_transform=g["full"][src],
                                    FoVx=float(g["fov"][src, 0]), FoVy=float(g["fov"][src, 1]), image_width=W, image_height=H)
        depth = g["depths"][src].astype(np.float32)
        fx, fy = W / (2.0 * math.tan(cam.FoVx / 2.0)), H / (2.0 * math.tan(cam.FoVy / 2.0))
        d = depth.astype(np.float64)
        c = np.stack([(x + 0.5 - W / 2.0) / fx * d, (y + 0.5 - H / 2.0) / fy * d, d], -1).reshape(-1, 3)
        wvt = np.asarray(cam.world_view_transform, np.float64).reshape(4, 4)
        p = (c - wvt[3, :3]) @ np.linalg.inv(wvt[:3, :3])  # c = p @ wvt[:3,:3] + wvt[3,:3]
        face = cube_face(p.reshape(H, W, 3))
        cams.append(cam)
        depths.append(depth)
        clouds.append(p.astype(np.float32))
        masks.append(np.where(depth < 4.9, 3 * face + 20 * v + 2, 0).astype(np.int32))
    images = np.random.default_rng(0).integers(0, 256, (V, H, W, 3)).astype(np.uint8)
    gdict = {}
    for k, face in enumerate(FACE_ORDER):
        order = range(V) if k % 2 == 0 else ODD_VIEW_ORDER
        gdict[k] = [(v, 3 * face + 20 * v + 2) for v in order if (masks[v] == 3 * face + 20 * v + 2).any()]
    return cams, depths, clouds, masks, images, gdict


def _stubs(cams, images):
    from g4splat_amd import ply_io

    def module(name, **names):
        m = types.ModuleType(name)
        for k, v in names.items():
            setattr(m, k, v)
        return m

    def ref_camera(v):
        wvt = np.asarray(cams[v].world_view_transform, np.float32).reshape(4, 4)
        return types.SimpleNamespace(R=wvt[:3, :3].copy(), T=wvt[3, :3].copy(), FoVx=cams[v].FoVx, FoVy=cams[v].FoVy,
                                     image_width=W, image_height=H,
                                     original_image=torch.tensor(images[v]).permute(2, 0, 1).float() / 255)

    class ModelParams:
        def __init__(self, parser, sentinel=False):
            pass

        def extract(self, args):
            return args

    def load(path):
        d = ply_io.read_ply_vertices(path)
        return types.SimpleNamespace(vertices=np.stack([d["x"], d["y"], d["z"]], 1).astype(np.float64))

    stubs = mgv._stubs()
    stubs["scene.dataset_readers"] = module(
        "scene.dataset_readers", load_cameras=lambda args: ([ref_camera(v) for v in range(N_INPUT)], None),
        load_see3d_cameras=lambda path, root: ([ref_camera(v) for v in range(N_INPUT, len(cams))], None))
    stubs["arguments"] = module("arguments", ModelParams=ModelParams)
    stubs["utils.general_utils"] = module("utils.general_utils", safe_state=lambda *a, **k: None,
                                          seed_everything=lambda *a, **k: None)
    stubs["trimesh"] = module("trimesh", load=load)
    return stubs


def write_scene(root, depths, clouds, masks, images, gdict):
    from PIL import Image
    from g4splat_amd import ply_io
    plane_root, see3d_root = os.path.join(root, "planes"), os.path.join(root, "see3d")
    os.makedirs(plane_root)
    os.makedirs(os.path.join(see3d_root, "inpainted_images"))
    for v in range(len(depths)):
        Image.fromarray(depths[v], mode="F").save(os.path.join(plane_root, f"refine_depth_frame{v:06d}.tiff"))
        Image.fromarray(images[v]).save(os.path.join(plane_root, f"rgb_frame{v:06d}.png"))
        np.save(os.path.join(plane_root, f"plane_mask_frame{v:06d}.npy"), masks[v])
        ply_io.write_point_cloud(os.path.join(plane_root, f"refine_points_frame{v:06d}.ply"), clouds[v])
    with open(os.path.join(plane_root, "global_3Dplane_ID_dict.json"), "w") as f:
        json.dump({str(k): [[v, p] for v, p in pairs] for k, pairs in gdict.items()}, f)
    anchor_json = os.path.join(root, "anchors.json")
    with open(anchor_json, "w") as f:
        json.dump(ANCHORS, f)
    return plane_root, see3d_root, anchor_json


def run_script(name, cams, depths, clouds, masks, images, gdict):
    """Runs guidance/<name> as __main__ over a fresh directory; returns (confident maps uint8 [V,H,W] in 0 / 255, repainted
    PNGs uint8 [V - N_INPUT,H,W,3])."""
    from PIL import Image
    V = len(cams)
    saved_argv, saved_threads, saved_cwd = list(sys.argv), torch.get_num_threads(), os.getcwd()
    with tempfile.TemporaryDirectory() as root:
        plane_root, see3d_root, anchor_json = write_scene(root, depths, clouds, masks, images, gdict)
        for v in range(V):  # the files hold what was put in
            assert np.array_equal(np.array(Image.open(os.path.join(plane_root, f"refine_depth_frame{v:06d}.tiff"))), depths[v])
        try:
            torch.set_num_threads(1)
            os.chdir(root)
            with reference_modules(_stubs(cams, images)):
                sys.path.insert(0, "/root/reference")
                import guidance.cam_utils as cam_utils
                cam_utils.to_tensor_safe = lambda data, dtype=None, device=None: torch.as_tensor(np.asarray(data)).to(torch.float32)
                sys.argv = [name, "--plane_root_path", plane_root, "--see3d_root_path", see3d_root]
                if "plane" in name:
                    sys.argv += ["--anchor_view_id_json_path", anchor_json]
                runpy.run_path(os.path.join(REF, "guidance", name), run_name="__main__")
        finally:
            sys.argv = saved_argv
            os.chdir(saved_cwd)
            torch.set_num_threads(saved_threads)
        conf = np.stack([np.array(Image.open(os.path.join(plane_root, f"confident_map_frame{v:06d}.png"))) for v in range(V)])
        pngs = np.stack([np.array(Image.open(os.path.join(see3d_root, "inpainted_images", f"predict_warp_frame{v:06d}.png")))
                         for v in range(V - N_INPUT)])
    return conf, pngs


def main():
    import consistency_ref as cr
    cams, depths, clouds, masks, images, gdict = make_inputs()
    V = len(cams)
    points = np.concatenate(clouds)
    conf_a, png_a = run_script("inconsistence_solver.py", cams, depths, clouds, masks, images, gdict)
    conf_b, png_b = run_script("plane_inconsistency_solver.py", cams, depths, clouds, masks, images, gdict)
    assert (conf_b == 255).all()  # the plane solver's pseudo confident maps

    # the restatement, float32
    f_images = [images[v].astype(np.float32) / np.float32(255) for v in range(V)]  # original_image
    stats = {}
    outs, confs = cr.point_solver(cams, depths, f_images, points, N_INPUT, THRESHOLD, np.float32, stats)
    s_conf = np.stack(confs) * 255
    s_png_a = np.stack([cr.images_to_uint8(o) for o in outs[N_INPUT:]])
    lengths = [np.zeros(H * W, np.int64) for _ in range(V)]
    b_outs, anchor_of_plane, counts = cr.plane_solver(cams, depths, list(images), masks, clouds, gdict, ANCHORS, THRESHOLD,
                                                      np.float32, lengths)
    s_png_b = np.stack(b_outs[N_INPUT:])
    agreed_conf = s_conf == conf_a
    agreed_a = (s_png_a == png_a).all(-1)
    agreed_b = (s_png_b == png_b).all(-1)
    for name, agreed in (("conf", agreed_conf[N_INPUT:]), ("point images", agreed_a), ("plane images", agreed_b)):
        excluded = int((~agreed).sum())
        print(f"{name}: {excluded} of {agreed.size} pixels differ from the restatement")
        assert excluded <= CAP * agreed.size, (name, excluded, agreed.size)
    assert (conf_a[:N_INPUT] == 255).all()

    # the scene must keep the properties the tests lean on
    steps = cr.plane_steps(gdict, anchor_of_plane)
    src = cr.plane_sources(cams, depths, masks, clouds, steps, THRESHOLD)
    own = sum(int(((src[w][0] != cr.NO_STEP) & (src[w][1] == w)).sum()) for w in range(V))
    chain = np.bincount(np.concatenate(lengths[N_INPUT:]), minlength=3)
    stats.update(anchors=[anchor_of_plane[k] for k in gdict], steps=len(steps), own_view_anchor_pixels=own,
                 chain_lengths=chain.tolist(), counts=counts.tolist(),
                 plane_changed=[int((b_outs[v] != images[v]).any(-1).sum()) for v in range(N_INPUT, V)])
    print(json.dumps(stats))
    assert stats["duplicate_pixels_differing"] > 1000, stats
    assert stats["changed_pixels"] > 1000, stats
    assert max(stats["conf_zeros"]) > 100, stats
    assert chain[2:].sum() > 100, stats
    assert own > 100, stats
    assert len(set(stats["anchors"]) - {-1}) >= 2, stats

    out = {"wvt": np.stack([c.world_view_transform for c in cams]), "full": np.stack([c.full_proj_transform for c in cams]),
           "fov": np.array([[c.FoVx, c.FoVy] for c in cams], np.float64), "depths": np.stack(depths),
           "clouds": np.stack(clouds), "images": images, "masks": np.stack(masks), "n_input": np.int64(N_INPUT),
           "dict": np.array(json.dumps({str(k): [[v, p] for v, p in pairs] for k, pairs in gdict.items()})),
           "anchors": np.array(ANCHORS, np.int64), "depth_threshold": np.float64(THRESHOLD),
           "point_conf": conf_a, "point_png": png_a, "plane_png": png_b,
           "point_conf_agreed": np.packbits(agreed_conf.reshape(-1)), "point_png_agreed": np.packbits(agreed_a.reshape(-1)),
           "plane_png_agreed": np.packbits(agreed_b.reshape(-1)),
           "excluded": np.array([int((~agreed_conf).sum()), int((~agreed_a).sum()), int((~agreed_b).sum())]),
           "stats": np.array(json.dumps(stats))}
    path = os.path.join(HERE, "consistency.npz")
    np.savez_compressed(path, **out)
    print(f"wrote consistency.npz {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
