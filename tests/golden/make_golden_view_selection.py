"""Golden vectors of view selection, produced by RUNNING THE REFERENCE'S OWN CODE on the CPU of the build container:

    view_selection.npz   guidance/cam_utils.py `get_visible_points_mask`, `covisibility_check_by_gs`,
                         `select_need_inpaint_views`, `farthest_point_sample` and `get_novel_cams_lookat_points`, imported
                         and called for real, in float32 and in float64.  The import stand-ins are
                         make_golden_visibility._stubs(); cam_utils.to_tensor_safe is replaced as there.

Scene.  Seventy look-at cameras on a spiral about the unit sphere (tests/view_selection_ref.py spiral_cameras: 32 x 24, every
third 64 x 48, every seventh 40 x 40) and 4 000 points: a tenth near the sphere's surface, the others uniform in the box
[-4, 4]^3 (covisibility ratios then spread from about 0.45 to 0.9), the camera centres among them.

Masks.  A mask bit is a decision; torch orders its matmul differently from the contract, so everything is run a second time
in float64, and so is the restatement.  The agreed set = the (camera, point) pairs on which ref32 == ref64 and
restatement32 == restatement64; its complement may hold at most 0.1 % of the pairs (asserted here, counts stored).

Selection.  Recorded cases (rates, bounds and seeds chosen below) that between them reject a candidate for covisibility,
enter step 4, enter step 5, have an empty filtered list and reach select_num early (asserted).  For each the npz holds the
reference's ids and the next random.random() after the call.  Every ratio the reference compared differs from the bound by
more than 2 d / min|V|, d the number of mask bits of the two cameras outside the agreed set or on which the restatement
differs from the reference (asserted): a flipped bit cannot flip a decision.

Sampling.  The index sequences of farthest_point_sample (read from the torch.argmax calls it makes) on random clouds, a
4 x 4 x 4 lattice, a cloud of identical points and a cloud whose coordinates reach 2e5; ref32 == ref64 on each (asserted).
Look-at points: the five clouds and camera centres of visibility_grid.npz, thirty novel centres; the reference's
torch.randint draws are recorded, under torch.manual_seed, by wrapping torch.randint.

Nothing of the reference is copied: the npz holds inputs and recorded results only.
Run in the build container only (needs /root/reference):  python tests/golden/make_golden_view_selection.py"""
import contextlib
import io
import json
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_visibility as mgv  # noqa: E402
from _ref_import import reference_modules  # noqa: E402

N_POINTS = 4000
LOOKAT_SEED = 1234
FPS_NUM = 10
N_NOVEL = 30

# name -> (seed, rates as (generator seed, low, high) or a list, select_num, low bound, high bound, covisibility bound)
SELECTION_CASES = {
    "typical": (11, (101, 0.0, 0.7), 10, 0.05, 0.5, 0.8),
    "early": (12, (102, 0.06, 0.45), 3, 0.05, 0.5, 0.8),
    "tight": (13, (103, 0.0, 0.6), 10, 0.05, 0.5, 0.5),
    "step4": (14, (104, 0.0, 0.08), 10, 0.05, 0.5, 0.6),
    "step5": (15, (105, 0.0, 0.12), 12, 0.05, 0.5, 0.05),
    "empty": (16, (106, 0.0, 0.049), 6, 0.05, 0.5, 0.7),
    "none_left": (17, (107, 0.6, 0.9), 5, 0.05, 0.5, 0.8),
    "one": (18, (108, 0.1, 0.4), 1, 0.05, 0.5, 0.8),
}


def make_scene():
    import view_selection_ref as sr
    cams = sr.spiral_cameras(70, True)
    rng = np.random.default_rng(2026)
    pts = rng.uniform(-4.0, 4.0, (N_POINTS, 3))
    s = rng.normal(size=(N_POINTS // 10, 3))
    pts[: N_POINTS // 10] = s / np.linalg.norm(s, axis=1, keepdims=True) * rng.uniform(0.9, 1.1, (N_POINTS // 10, 1))
    centres = np.stack([np.asarray(c.camera_center, np.float64) for c in cams])
    pts[-len(centres):] = centres
    return cams, pts.astype(np.float32)


def case_rates(spec, n):
    if isinstance(spec, tuple):
        seed, lo, hi = spec
        return np.random.default_rng(seed).uniform(lo, hi, n).tolist()
    return list(spec)


def sampling_clouds():
    import view_selection_ref as sr
    rng = np.random.default_rng(77)
    big = rng.uniform(-2e5, 2e5, (40, 3)).astype(np.float32)
    return {
        "random257": (rng.normal(size=(257, 3)).astype(np.float32), 10, 256),
        "random11": (rng.normal(size=(11, 3)).astype(np.float32), 10, 0),
        "three": (rng.normal(size=(3, 3)).astype(np.float32), 2, 2),
        "lattice": (sr.lattice(4), 12, 21),
        "identical": (np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (11, 1)), 5, 7),
        "far": (big, 8, 39),
    }


class _Recorder:
    """Wraps torch.randint (optionally forcing its next results) and torch.argmax, recording what they return."""

    def __init__(self):
        self.randint, self.argmax, self.forced = [], [], []
        self._randint, self._argmax = torch.randint, torch.argmax

    def __enter__(self):
        def randint(*a, **k):
            r = self._randint(*a, **k)
            if self.forced:
                r = torch.full_like(r, self.forced.pop(0))
            self.randint.append(r.reshape(-1).tolist())
            return r

        def argmax(*a, **k):
            r = self._argmax(*a, **k)
            if r.numel() == 1:
                self.argmax.append(int(r))
            return r
        torch.randint, torch.argmax = randint, argmax
        return self

    def __exit__(self, *exc):
        torch.randint, torch.argmax = self._randint, self._argmax
        return False


def run_reference(cams, points, double):
    dt = torch.float64 if double else torch.float32
    npdt = np.float64 if double else np.float32
    out = {}
    saved_float, saved_default = torch.Tensor.float, torch.get_default_dtype()
    try:
        if double:
            torch.set_default_dtype(torch.float64)
            torch.Tensor.float = lambda self, *a, **k: self.to(torch.float64)
        with reference_modules(mgv._stubs()):
            sys.path.insert(0, "/root/reference")
            import guidance.cam_utils as cam_utils
            cam_utils.to_tensor_safe = lambda data, dtype=None, device=None: torch.as_tensor(np.asarray(data)).to(dt)
            ref_cams = []
            for c in cams:
                wvt = np.asarray(c.world_view_transform, npdt)
                ref_cams.append(types.SimpleNamespace(R=wvt[:3, :3].copy(), T=wvt[3, :3].copy(), FoVx=c.FoVx, FoVy=c.FoVy,
                                                      image_width=c.image_width, image_height=c.image_height))
            pts = torch.tensor(points, dtype=dt)
            gaussians = types.SimpleNamespace(get_xyz=pts)
            masks = np.stack([cam_utils.get_visible_points_mask(c, pts).numpy() for c in ref_cams])
            out["masks"] = masks
            pairs = [(0, 1), (0, 35), (3, 4), (10, 27), (69, 68), (5, 5)]
            out["pairs"] = pairs
            out["pair_ratios"] = [float(cam_utils.covisibility_check_by_gs(ref_cams[i], ref_cams[j], gaussians)) for i, j in pairs]
            # selection: the ratios it compares are recorded through a wrapper of the function it calls
            index_of = {id(c): i for i, c in enumerate(ref_cams)}
            compared = []
            inner = cam_utils.covisibility_check_by_gs

            def recording(c1, c2, g):
                r = inner(c1, c2, g)
                compared.append((index_of[id(c1)], index_of[id(c2)], float(r)))
                return r
            cam_utils.covisibility_check_by_gs = recording
            out["selection"] = {}
            for name, (seed, spec, num, lo, hi, bound) in SELECTION_CASES.items():
                rates = case_rates(spec, len(ref_cams))
                del compared[:]
                random.seed(seed)
                text = io.StringIO()
                with contextlib.redirect_stdout(text):
                    ids = cam_utils.select_need_inpaint_views(ref_cams, rates, gaussians, num, lo, hi, bound)
                out["selection"][name] = {
                    "ids": [int(i) for i in ids], "next_random": random.random(), "compared": list(compared),
                    "step4": "Relaxing constraints" in text.getvalue(), "step5": "Adding remaining views" in text.getvalue(),
                    "filtered": sum(lo <= r <= hi for r in rates)}
            cam_utils.covisibility_check_by_gs = inner
            # sampling
            out["sampling"] = {}
            for name, (cloud, k, first) in sampling_clouds().items():
                with _Recorder() as rec:
                    rec.forced.append(first)
                    got = cam_utils.farthest_point_sample(torch.tensor(cloud, dtype=dt), k)
                idx = [first] + rec.argmax
                assert len(idx) == k and np.array_equal(got.numpy(), cloud.astype(npdt)[idx])
                out["sampling"][name] = idx
            g = np.load(os.path.join(HERE, "visibility_grid.npz"))
            clouds = torch.tensor(g["clouds"], dtype=dt)
            train = torch.tensor(np.asarray(mgv.EYES), dtype=dt)
            novel = torch.tensor(lookat_novel_centres(), dtype=dt)
            torch.manual_seed(LOOKAT_SEED)
            with _Recorder() as rec:
                look = cam_utils.get_novel_cams_lookat_points(train, clouds, novel, FPS_NUM)
            out["lookat"] = look.numpy()
            out["lookat_draws"] = rec.randint
            out["lookat_closest"] = torch.argmin(torch.cdist(novel, train), dim=1).numpy()
    finally:
        torch.Tensor.float = saved_float
        torch.set_default_dtype(saved_default)
    return out


def lookat_novel_centres():
    return np.random.default_rng(55).uniform(-3.5, 3.5, (N_NOVEL, 3)).astype(np.float32)


def main():
    import view_selection_ref as sr
    cams, points = make_scene()
    r32 = run_reference(cams, points, False)
    r64 = run_reference(cams, points, True)
    s32, s64 = sr.visible_masks(points, cams, np.float32), sr.visible_masks(points, cams, np.float64)
    ref_differ = r32["masks"] != r64["masks"]
    agreed = ~ref_differ & (s32 == s64)
    excluded = int((~agreed).sum())
    assert excluded <= 0.001 * agreed.size, (excluded, agreed.size)
    unsafe = ~agreed | (s32 != r32["masks"])  # bits that may differ between the restatement and the reference
    visible = r32["masks"].sum(1)
    table = sr.counts(s32)
    assert 0.05 < r32["masks"].mean() < 0.8 and visible.min() > 100
    ratio = sr.ratio_of(table)
    for (i, j), want in zip(r32["pairs"], r32["pair_ratios"]):
        if unsafe[i].sum() + unsafe[j].sum() == 0:
            assert ratio(i, j) == want, (i, j, ratio(i, j), want)
    # selection
    seen = {"rejected": False, "step4": False, "step5": False, "empty": False, "early": False}
    for name, (seed, spec, num, lo, hi, bound) in SELECTION_CASES.items():
        a, b = r32["selection"][name], r64["selection"][name]
        assert a["ids"] == b["ids"] and a["next_random"] == b["next_random"], name
        for i, j, r in a["compared"]:
            d = int(unsafe[i].sum() + unsafe[j].sum())
            margin = 2.0 * d / max(min(int(visible[i]), int(visible[j])), 1)
            assert abs(r - bound) > margin, (name, i, j, r, bound, margin)
            seen["rejected"] |= r > bound
        seen["step4"] |= a["step4"]
        seen["step5"] |= a["step5"]
        seen["empty"] |= a["filtered"] == 0
        seen["early"] |= len(a["ids"]) >= num and not a["step4"] and a["filtered"] > len(a["ids"])
    assert all(seen.values()), seen
    # sampling
    for name, (cloud, k, first) in sampling_clouds().items():
        assert r32["sampling"][name] == r64["sampling"][name], name
        assert sr.fps(cloud, k, first)[0].tolist() == r32["sampling"][name], name
    assert r32["lookat_draws"] == r64["lookat_draws"] and np.array_equal(r32["lookat_closest"], r64["lookat_closest"])
    assert np.array_equal(r32["lookat"], r64["lookat"].astype(np.float32))
    draws = r32["lookat_draws"]
    first, ids = [d[0] for d in draws[:-1]], draws[-1]
    assert len(first) == len(mgv.EYES) and len(ids) == N_NOVEL
    g = np.load(os.path.join(HERE, "visibility_grid.npz"))
    novel = lookat_novel_centres()
    assert np.array_equal(sr.nearest_train_indices(np.asarray(mgv.EYES, np.float32), novel), r32["lookat_closest"])
    assert len(set(r32["lookat_closest"].tolist())) >= 3

    selection = {name: {"seed": seed, "rates": case_rates(spec, len(cams)), "select_num": num, "low": lo, "high": hi,
                        "bound": bound, "ids": r32["selection"][name]["ids"],
                        "next_random": r32["selection"][name]["next_random"], "step4": r32["selection"][name]["step4"],
                        "step5": r32["selection"][name]["step5"]}
                 for name, (seed, spec, num, lo, hi, bound) in SELECTION_CASES.items()}
    sampling = {name: {"k": k, "first": first, "indices": r32["sampling"][name]}
                for name, (cloud, k, first) in sampling_clouds().items()}
    out = {"points": points, "wvt": np.stack([c.world_view_transform for c in cams]).astype(np.float32),
           "fov": np.array([[c.FoVx, c.FoVy] for c in cams], np.float64),
           "sizes": np.array([[c.image_width, c.image_height] for c in cams], np.int32),
           "masks": np.packbits(r32["masks"].reshape(-1)), "masks_ref64": np.packbits(r64["masks"].reshape(-1)),
           "masks_agreed": np.packbits(agreed.reshape(-1)), "masks_shape": np.array(r32["masks"].shape),
           "masks_excluded": np.array([excluded, agreed.size, int(ref_differ.sum()), int((s32 != s64).sum())]),
           "pairs": np.array(r32["pairs"]), "pair_ratios": np.array(r32["pair_ratios"], np.float64),
           "selection": np.array(json.dumps(selection)), "sampling": np.array(json.dumps(sampling)),
           **{"cloud_" + name: cloud for name, (cloud, _k, _f) in sampling_clouds().items()},
           "lookat_train": np.asarray(mgv.EYES, np.float32), "lookat_novel": novel, "lookat_fps_num": np.int64(FPS_NUM),
           "lookat_seed": np.int64(LOOKAT_SEED), "lookat_first": np.array(first, np.int64), "lookat_ids": np.array(ids, np.int64),
           "lookat_closest": r32["lookat_closest"].astype(np.int64), "lookat": r32["lookat"].astype(np.float32)}
    assert g["clouds"].shape[0] == len(mgv.EYES)
    path = os.path.join(HERE, "view_selection.npz")
    np.savez_compressed(path, **out)
    print(f"wrote view_selection.npz {os.path.getsize(path)} bytes")
    print(f"masks: ref32 != ref64 on {int(ref_differ.sum())}, restatement32 != restatement64 on {int((s32 != s64).sum())}, "
          f"excluded {excluded} of {agreed.size}; restatement32 != ref32 on {int((s32 != r32['masks']).sum())}; "
          f"true on {float(r32['masks'].mean()):.3f}")
    for name, c in selection.items():
        print(name, c["ids"], "step4" if c["step4"] else "", "step5" if c["step5"] else "",
              len(r32["selection"][name]["compared"]), "ratios compared")
    print(seen)


if __name__ == "__main__":
    main()
