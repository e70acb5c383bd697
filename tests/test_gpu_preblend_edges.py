"""The short kernels between the preprocess and the blend at their size edges.

Builds tests/hip_unit/preblend_edges.hip against g4splat_amd/csrc/binning.hip with the library's own compiler flags and
runs it: the block-sum scan, the instance expansion, the count scan and the tile order against host restatements, bit
for bit.  And one frame pair through the rasterizer: the tile ranges are cleared by the preprocess kernel's workgroups,
so a tile that a frame leaves empty must read (0, 0) whatever the frame before left in the same image chunk."""
import os
import subprocess

import numpy as np
import pytest

from common import hip_state, run_hip, scene_inputs
from support import HIPCC, build_harness


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_preblend_harness_compiles_and_links(tmp_path):
    """No GPU needed: the harness builds against every launcher it calls."""
    assert os.path.getsize(build_harness(tmp_path, "preblend_edges", "binning.hip")) > 0


@pytest.mark.gpu
def test_preblend_kernels_against_host_restatements(tmp_path):
    exe = build_harness(tmp_path, "preblend_edges", "binning.hip")
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(res.stdout[-6000:])
    assert res.returncode == 0 and "preblend_edges OK" in res.stdout, res.stdout[-20000:]


def ranges_from_entries(entries, tiles):
    """[start, end) of every tile's run in the tile-ordered instance list; (0, 0) for a tile without one."""
    want = np.zeros((tiles, 2), np.uint32)
    tile = (entries >> np.uint64(32)).astype(np.int64)
    assert np.all(np.diff(tile) >= 0)
    for t in np.unique(tile):
        where = np.nonzero(tile == t)[0]
        want[t] = (where[0], where[-1] + 1)
    return want


@pytest.mark.gpu
def test_tiles_a_frame_leaves_empty_read_zero_ranges():
    """A 48 x 32 frame (six tiles) that fills every tile, then one whose Gaussians all sit on one spot, into the same image
    chunk: through _C.rasterize_gaussians (the allocator hands the freed chunk out again) and through a PresizedState
    (the same chunk by construction)."""
    import torch
    from g4splat_amd.diff_surfel_rasterization import _C
    W, H, P, tiles = 48, 32, 400, 6
    full = scene_inputs(P=P, W=W, H=H, seed=5, D=1)
    h = run_hip(full)
    st = hip_state(h, full)
    assert np.array_equal(st["ranges"], ranges_from_entries(st["entries"], tiles))
    assert np.all(st["ranges"][:, 1] > st["ranges"][:, 0]), "the first frame is to fill every tile"
    first_img = h["img"].data_ptr()
    # every Gaussian on the spot of the smallest visible one whose centre lies well inside a tile, a fiftieth of its size
    cx, cy = st["rec"][:, 0], st["rec"][:, 1]
    inside = (h["radii"] > 0) & (np.abs(cx % 16 - 8) < 3) & (np.abs(cy % 16 - 8) < 3) & (cx > 0) & (cx < W) & (cy > 0) & (cy < H)
    assert inside.any()
    j = int(np.argmin(np.where(inside, h["radii"], 1 << 30)))
    sparse = dict(full)
    sparse["means3D"] = np.repeat(full["means3D"][j:j + 1], P, axis=0).astype(np.float32)
    sparse["scales"] = (full["scales"] * 0.02).astype(np.float32)
    del h, st
    h = run_hip(sparse)
    st = hip_state(h, sparse)
    print("image chunk handed out again:", h["img"].data_ptr() == first_img)
    want = ranges_from_entries(st["entries"], tiles)
    assert np.count_nonzero(want[:, 1]) <= 2, want
    assert np.array_equal(st["ranges"], want), (st["ranges"], want)

    state = _C.PresizedState(P, W, H, 4 * P * tiles, "cuda:0")
    for inp in (full, sparse):
        a = dict((k, torch.as_tensor(np.ascontiguousarray(v), device="cuda:0")) for k, v in inp.items() if isinstance(v, np.ndarray))
        fw = _C.rasterize_gaussians_presized(state, a["bg"], a["means3D"], a["colors"], a["opacity"], a["scales"], a["rotations"],
                                             1.0, a["transMat"], a["view"], a["proj"], inp["tanfovx"], inp["tanfovy"], H, W, a["sh"],
                                             inp["D"], a["campos"], False, False)
        torch.cuda.synchronize()
        assert state.status.tolist()[3] == 0
        st = hip_state(dict(R=fw[0], geom=fw[4], binning=fw[5], img=fw[6]), inp)
        assert np.array_equal(st["ranges"], ranges_from_entries(st["entries"], tiles)), st["ranges"]
    assert np.count_nonzero(st["ranges"][:, 1]) <= 2
