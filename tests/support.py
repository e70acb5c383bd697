"""What the test files share: the comparison behind "bit for bit", the transfers to and from the device, the cameras and the
golden loaders that a CPU and a GPU test file both use, and the build of the tests/hip_unit programs.  A plain module, imported
like the *_ref.py files; importing it touches no GPU.  tests/common.py stays the rasterizer's parity gate.

"Bit for bit" means equal dtype, equal shape and equal bytes (same_bits).  The one licensed exception is a NaN's sign and
payload (nan_payload=False): the device and numpy make different NaNs, so there a NaN only has to meet a NaN."""
import json
import math
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
CSRC = os.path.join(ROOT, "g4splat_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
DEV = torch.device("cuda:0")
f32, f64 = np.float32, np.float64


# ---- transfers ---------------------------------------------------------------------------------------------------------------
def dev(a, dtype=None):
    """A host array on the device (made contiguous first); None stays None."""
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def devs(arrays):
    return [dev(a) for a in arrays]


def host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def hosts(ts):
    return [host(t) for t in ts]


# ---- comparison --------------------------------------------------------------------------------------------------------------
def _pairs(got, want, what):
    """The (got, want, what) leaves of two equally nested lists or tuples, as host arrays; None has to meet None."""
    if isinstance(got, (list, tuple)) or isinstance(want, (list, tuple)):
        assert isinstance(got, (list, tuple)) and isinstance(want, (list, tuple)), (what, type(got), type(want))
        assert len(got) == len(want), (what, "lengths", len(got), len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            yield from _pairs(g, w, f"{what}[{i}]")
    elif got is None or want is None:
        assert got is None and want is None, (what, "None against a value")
    else:
        got, want = host(got), host(want)
        assert got.dtype == want.dtype, (what, "dtype", got.dtype, want.dtype)
        assert got.shape == want.shape, (what, "shape", got.shape, want.shape)
        yield got, want, what


def _report(got, want, differ, what):
    g, w = got.reshape(-1), want.reshape(-1)
    first = int(np.flatnonzero(differ)[0])
    where = tuple(int(i) for i in np.unravel_index(first, got.shape))
    msg = (f"{what}: {int(differ.sum())} of {differ.size} elements differ, first at {where}: "
           f"got {g[first]} ({g[first].tobytes().hex()}), want {w[first]} ({w[first].tobytes().hex()})")
    if got.dtype.kind in "fiub":
        with np.errstate(invalid="ignore"):  # widening a signalling NaN
            a, b = g.astype(f64), w.astype(f64)
        finite = np.isfinite(a) & np.isfinite(b)
        msg += f"; largest |difference| over the finite elements {np.abs(a[finite] - b[finite]).max(initial=0.0):.3e}"
    return msg


def same_bits(got, want, what="", nan_payload=True):
    """Equal dtype, shape and bytes.  Arrays, tensors on any device or scalars; lists and tuples element by element.  With
    nan_payload=False a NaN of a float array has to meet a NaN, of whatever sign and payload."""
    for g, w, name in _pairs(got, want, what):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        differ = (g.reshape(-1, 1).view(np.uint8) != w.reshape(-1, 1).view(np.uint8)).any(axis=1)
        if not nan_payload and g.dtype.kind == "f":
            differ &= ~(np.isnan(g) & np.isnan(w)).reshape(-1)
        assert not differ.any(), _report(g, w, differ, name)


def same_values(got, want, what=""):
    """Equal dtype, shape and values: -0.0 meets 0.0 and a NaN meets nothing.  Only for a site recorded as unable to be
    bitwise."""
    for g, w, name in _pairs(got, want, what):
        assert np.array_equal(g, w), _report(g, w, (g != w).reshape(-1), name)


def words(a):
    """A float32 array as its uint32 words."""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.uint32)


def twice(fn):
    """fn() run twice: the first result, after asserting that the second has the same bits."""
    a, b = fn(), fn()
    same_bits(b, a, "second run")
    return a


# ---- cameras -----------------------------------------------------------------------------------------------------------------
def pinhole_camera(W, H, fx, fy, t=(0.0, 0.0, 0.0)):
    """A camera looking down +z from -t: world_view_transform = identity with the translation in its last row."""
    M = np.eye(4, dtype=np.float32)
    M[3, :3] = t
    return SimpleNamespace(world_view_transform=M, full_proj_transform=M, FoVx=2.0 * math.atan(W / (2.0 * fx)),
                           FoVy=2.0 * math.atan(H / (2.0 * fy)))


def device_camera(cam):
    """A synthetic camera with its matrices and centre on the device."""
    return SimpleNamespace(image_width=cam.image_width, image_height=cam.image_height, FoVx=cam.FoVx, FoVy=cam.FoVy,
                           world_view_transform=dev(cam.world_view_transform), full_proj_transform=dev(cam.full_proj_transform),
                           camera_center=dev(cam.camera_center), znear=cam.znear, zfar=cam.zfar)


def golden_cameras(g, **more):
    """The cameras a golden file records as (wvt, full, fov), one per view; `more` is set on each."""
    return [SimpleNamespace(world_view_transform=w, full_proj_transform=f, FoVx=float(a[0]), FoVy=float(a[1]), **more)
            for w, f, a in zip(g["wvt"], g["full"], g["fov"])]


# ---- goldens that a CPU and a GPU test file both load ------------------------------------------------------------------------
def _pairs_dict(text):
    return {int(k): [(int(v), int(p)) for v, p in pairs] for k, pairs in json.loads(str(text)).items()}


def load_planes_golden():
    g = np.load(os.path.join(GOLDEN, "global_planes.npz"))

    def ragged(key):
        flat, offs = g[key].astype(np.int64), g[key + "_offsets"]
        return [flat[a:b] for a, b in zip(offs[:-1], offs[1:])]

    return SimpleNamespace(g=g, cams=golden_cameras(g), masks=list(g["masks"]), points=g["points"],
                           depth_thresh=float(g["depth_thresh"]), ids=_pairs_dict(g["ids"]), ids3=_pairs_dict(g["ids3"]),
                           resume_ids=_pairs_dict(g["resume_ids"]), idx=ragged("idx"), resume_idx=ragged("resume_idx"),
                           hand_cases=json.loads(str(g["hand_cases"])), hand_results=json.loads(str(g["hand_results"])),
                           stats=json.loads(str(g["stats"])))


def load_consistency_golden():
    g = np.load(os.path.join(GOLDEN, "consistency.npz"))
    images = list(g["images"])

    def agreed(key, shape):
        return np.unpackbits(g[key])[: int(np.prod(shape))].astype(bool).reshape(shape)

    return SimpleNamespace(
        g=g, cams=golden_cameras(g), depths=list(g["depths"]), clouds=list(g["clouds"]), points=g["clouds"].reshape(-1, 3),
        images=images, float_images=[im.astype(f32) / f32(255) for im in images],  # the cameras' original_image
        masks=list(g["masks"]), n_input=int(g["n_input"]), gdict=_pairs_dict(g["dict"]), anchors=[int(a) for a in g["anchors"]],
        threshold=float(g["depth_threshold"]), point_conf=g["point_conf"], point_png=g["point_png"], plane_png=g["plane_png"],
        point_conf_agreed=agreed("point_conf_agreed", g["point_conf"].shape),
        point_png_agreed=agreed("point_png_agreed", g["point_png"].shape[:3]),
        plane_png_agreed=agreed("plane_png_agreed", g["plane_png"].shape[:3]), stats=json.loads(str(g["stats"])))


def load_depth_cues_golden():
    g = np.load(os.path.join(GOLDEN, "depth_cues.npz"))
    V = len(g["wvt"])
    H, W = g["depths"].shape[1:]
    planes = {int(k): (row[:3].copy(), row[3:].copy()) for k, row in zip(g["plane_keys"], g["plane_rows"])}
    disps = list(g["disps"])
    out = SimpleNamespace(g=g, V=V, H=H, W=W, cams=golden_cameras(g, image_width=W, image_height=H), gdict=_pairs_dict(g["gdict"]),
                          planes=planes, n_input=int(g["n_input"]), threshold=float(g["threshold"]), depths=list(g["depths"]),
                          masks=list(g["masks"]), disps=disps, alphas=list(g["alphas"]),
                          monos=[(f32(1) / d).astype(f32) for d in disps], confs=list(g["confs"]),
                          yard=json.loads(str(g["yardstick"])), agreed=g["agreed"],
                          visible=[a > f32(g["threshold"]) for a in g["alphas"]])
    # the merged depth of the reference's float64 run: the rendered depth where visible, its aligned depth elsewhere
    out.ref_merged = np.stack([np.where(out.visible[v], g["depths"][v].astype(f64), g["ref64_aligned_depth"][v]) for v in range(V)])
    return out


def load_chart_init_golden():
    g = dict(np.load(os.path.join(GOLDEN, "chart_init.npz")))
    g["yard"] = json.loads(str(g["yardstick"]))
    return g


PLANE_MASK_MAPS = ("small", "large")


def load_plane_masks_golden():
    return dict(np.load(os.path.join(GOLDEN, "plane_masks.npz")))


PLANE_FIT_KEYS = (10, 11, 12)


def load_plane_fit_golden():
    return np.load(os.path.join(GOLDEN, "plane_fit.npz"))


def plane_fit_scene(g):
    """(cams, depths, normals, masks, confs, gdict) of the plane-fit golden's scene as numpy arrays."""
    gdict = {int(k): [tuple(p) for p in pairs] for k, pairs in json.loads(str(g["gdict"])).items()}
    return golden_cameras(g), list(g["depths"]), list(g["normals"]), list(g["masks"].astype(np.int32)), list(g["confs"]), gdict


# ---- the tests/hip_unit programs ---------------------------------------------------------------------------------------------
def makefile_cxxflags():
    """CXXFLAGS of g4splat_amd/csrc/Makefile, with $(ARCH) resolved from the same file."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*=\s*(.+)$", text, re.M).group(1).replace("$(ARCH)", arch).split()
    assert "--offload-arch=gfx950" in flags and "-ffp-contract=off" in flags, flags
    return flags


def build_harness(tmp_path, unit, *library_sources):
    """tests/hip_unit/<unit>.hip compiled and linked with the named files of g4splat_amd/csrc; returns the program's path."""
    exe = str(tmp_path / unit)
    cmd = [HIPCC] + makefile_cxxflags() + [os.path.join(HERE, "hip_unit", unit + ".hip")] \
        + [os.path.join(CSRC, *s.split("/")) for s in library_sources] + ["-o", exe]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    return exe
