"""g4splat_amd/_device.py without a device: the host arrays, the device resolution, the shared map checks and the view stack's
host side (which only compares devices and reads addresses, so CPU tensors stand in for device maps)."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from g4splat_amd import _device, depth_cues, view_selection

CPU = torch.device("cpu")
FOVS = [(1.0, 0.8), (0.3, 3.1), (math.pi - 1e-6, 1e-3), (math.pi / 2, math.pi / 3), (2.5, 0.05)]
SIZES = [(3, 2), (4, 3), (640, 480), (1, 1), (1600, 1199)]


def _camera(fov_x, fov_y, W=4, H=3, seed=0):
    rng = np.random.default_rng(seed)
    return SimpleNamespace(world_view_transform=torch.tensor(rng.normal(size=(4, 4)).astype(np.float32)), FoVx=fov_x, FoVy=fov_y,
                           image_width=W, image_height=H)


@pytest.mark.parametrize("fov", FOVS)
@pytest.mark.parametrize("size", SIZES)
def test_focal_lengths_are_the_three_former_expressions(fov, size):
    (W, H), cam = size, _camera(*fov, *size)
    fx, fy = _device.focal_lengths(cam, W, H)
    # visibility's and view_selection's wording, then depth_cues'
    assert [fx, fy] == [W / (2.0 * math.tan(float(cam.FoVx) / 2.0)), H / (2.0 * math.tan(float(cam.FoVy) / 2.0))]
    width, height = W, H
    assert fx == width / (2.0 * math.tan(float(cam.FoVx) / 2.0)) and fy == height / (2.0 * math.tan(float(cam.FoVy) / 2.0))
    assert isinstance(fx, float) and isinstance(fy, float)
    # ... and reaches the three users as the same float32
    want = np.array([fx, fy], np.float32)
    assert np.array_equal(depth_cues.plane_camera_record(cam, W, H)[12:], want)
    assert np.array_equal(np.array(view_selection._camera_arrays([cam])[2][:], np.float32), want)
    stack = _device.camera_views([cam], [torch.ones((H, W))], CPU)
    assert np.array_equal(np.array(stack.head[2][:], np.float32), want)


def test_host_arrays_are_never_empty():
    for ctype, values in ((ctypes.c_int, [3, -1, 7]), (ctypes.c_float, [0.5, -2.0]), (ctypes.c_void_p, [256, 512])):
        empty, full = _device.host_array(ctype, []), _device.host_array(ctype, values)
        assert len(empty) == 1 and not empty[0] and empty._type_ is ctype
        assert len(full) == len(values) and list(full) == values and full._type_ is ctype
    assert list(_device.host_array(ctypes.c_int, iter([4, 5]))) == [4, 5]  # any iterable
    third = _device.host_array(ctypes.c_float, [1.0 / 3.0])[0]  # rounded to float32 as numpy rounds it
    assert third == float(np.float32(1.0 / 3.0))
    f = _device.host_f32(np.array([[1.5, 2.5], [3.5, 1.0 / 3.0]]))
    assert len(f) == 4 and list(f) == [1.5, 2.5, 3.5, float(np.float32(1.0 / 3.0))] and len(_device.host_f32([])) == 0
    assert _device.to_np(torch.tensor([1, 2])).tolist() == [1, 2] and _device.to_np([1.5]).tolist() == [1.5]


def test_device_resolution():
    with pytest.raises(RuntimeError, match=r"the mesh kernels need tensors on a HIP device \(there is no CPU path\)"):
        _device.hip_device("cpu")
    with pytest.raises(RuntimeError, match="the mesh kernels need tensors on a HIP device"):
        _device.hip_device(torch.zeros(1).device)
    assert _device.hip_device("cuda:1") == torch.device("cuda", 1)  # an index is taken as given; no device is asked
    with pytest.raises(RuntimeError, match="points must be a tensor on a HIP device"):
        _device.device_points([[0.0, 0.0, 0.0]])
    with pytest.raises(RuntimeError, match="cloud must be a tensor on a HIP device"):
        _device.device_points(None, "cloud")
    with pytest.raises(RuntimeError, match="depth must be a tensor on a HIP device"):
        _device.depth_map([[1.0]])
    with pytest.raises(RuntimeError, match="the mesh kernels need tensors on a HIP device"):
        _device.depth_map(torch.ones((2, 3)))
    with pytest.raises(RuntimeError, match="depth must be a tensor on cuda:0"):
        _device.depth_map(torch.ones((2, 3)), "cuda:0")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match=r"mesh operations need a HIP device \(there is no CPU path\)"):
            _device.default_device()
    b, u = torch.ones((2, 3), dtype=torch.bool), torch.ones((2, 3), dtype=torch.uint8)
    assert _device.mask_bytes(b).dtype == torch.uint8 and _device.mask_bytes(b).data_ptr() == b.data_ptr() and _device.mask_bytes(u) is u


def test_shared_map_checks_keep_their_messages():
    m = torch.ones((2, 3))
    assert _device.on_device(m, CPU, "depth").data_ptr() == m.data_ptr()
    for bad in ([[1.0]], None):
        with pytest.raises(RuntimeError, match="rgb must be a tensor on cuda:0"):
            _device.on_device(bad, torch.device("cuda", 0), "rgb")
    with pytest.raises(RuntimeError, match="mask must be a tensor on cuda:0"):
        _device.on_device(m, torch.device("cuda", 0), "mask")
    assert _device.drop_leading_one(m[None]).shape == (2, 3) and _device.drop_leading_one(torch.ones((2, 2, 3))).shape == (2, 2, 3)
    assert _device.drop_leading_one(torch.ones((1, 1, 2, 3))).shape == (1, 1, 2, 3)
    assert [tuple(t.shape) for t in _device.view_list(torch.ones((2, 4, 5)), "maps")] == [(4, 5), (4, 5)]
    as_list = _device.view_list((m, m[None]), "maps")
    assert isinstance(as_list, list) and as_list[0] is m and as_list[1].shape == (1, 2, 3)  # a list is taken as it is
    with pytest.raises(ValueError, match=r"maps: a stacked tensor must be \[V,H,W\] \(got \(4, 5\)\)"):
        _device.view_list(torch.ones((4, 5)), "maps")
    with pytest.raises(ValueError, match=r"points: a stacked tensor must be \[V,H,W,3\] \(got \(4, 5, 3\)\)"):
        _device.view_list(torch.ones((4, 5, 3)), "points", ",3")
    _device.check_view_count([m], "maps", None)
    with pytest.raises(ValueError, match="2 views but 1 maps"):
        _device.check_view_count([m], "maps", 2)
    with pytest.raises(ValueError, match=r"masks\[1\] must be torch.bool or torch.uint8 \(got torch.float32\)"):
        _device.check_dtype(m, (torch.bool, torch.uint8), "masks[1]")
    for bad in (m, [[1.0]]):
        with pytest.raises(ValueError, match=r"maps\[0\] must be a tensor on a HIP device"):
            _device.same_device(bad, None, "maps[0]")


def _restated(views, n_matrices, matrices, focal):
    """The arrays the wrappers used to build for themselves, in a few lines: (sizes, matrix floats per matrix, focal floats)."""
    sizes, mats, foc = [], [[] for _ in range(n_matrices)], []
    for cam, depth, _rgb in views:
        H, W = depth.shape[-2:]
        sizes += [W, H]
        for m, M in zip(mats, matrices(cam)):
            m += np.asarray(M, np.float32).reshape(16).tolist()
        if focal:
            foc += [W / (2.0 * math.tan(float(cam.FoVx) / 2.0)), H / (2.0 * math.tan(float(cam.FoVy) / 2.0))]
    return sizes, [np.array(m, np.float32) for m in mats], np.array(foc, np.float32)


def test_view_stack_host_arrays():
    cams = [_camera(1.0, 0.8, seed=1), _camera(0.3, 3.1, seed=2), _camera(math.pi - 1e-6, 0.5, seed=3)]
    depths = [torch.ones((2, 3)), torch.ones((1, 5, 4)), torch.ones((7, 6), dtype=torch.float64)[:, ::2]]
    rgbs = [torch.zeros((3, 2, 3)), torch.zeros((3, 5, 4)), torch.zeros((3, 7, 3), dtype=torch.float16)]
    views = list(zip(cams, depths, rgbs))
    two = lambda cam: [cam.world_view_transform, cam.world_view_transform.T * 2]
    stack = _device.ViewStack(views, CPU, True, 2, two)
    sizes, mats, _f = _restated(views, 2, two, False)
    assert stack.n == 3 and list(stack.sizes) == sizes == [3, 2, 4, 5, 3, 7]
    assert [stack.size(v) for v in range(3)] == [(2, 3), (5, 4), (7, 3)]
    assert len(stack.head) == 5 and stack.head[0] == 3 and stack.head[3] is stack.sizes and stack.head[4] is stack.depth
    for got, want in zip(stack.head[1:3], mats):
        assert np.array_equal(np.array(got[:], np.float32), want)
    # the maps are float32, contiguous, kept alive, and their addresses are the pointer arrays
    assert [tuple(t.shape) for t in stack.maps] == [(2, 3), (3, 2, 3), (5, 4), (3, 5, 4), (7, 3), (3, 7, 3)]
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in stack.maps)
    assert list(stack.depth) == [t.data_ptr() for t in stack.maps[0::2]] and list(stack.rgb) == [t.data_ptr() for t in stack.maps[1::2]]
    assert stack.maps[0].data_ptr() == depths[0].data_ptr()  # what is float32 and contiguous already is not copied
    assert not hasattr(stack, "ws")  # nothing is allocated: the view table's workspace belongs to the call

    # the visibility family: one matrix, the focal lengths between the matrices and the sizes
    vis = _device.camera_views(cams, depths, CPU)
    sizes, mats, focal = _restated(views, 1, lambda cam: [cam.world_view_transform], True)
    assert vis.rgb is None and len(vis.head) == 5 and vis.head[0] == 3 and list(vis.head[3]) == sizes
    assert np.array_equal(np.array(vis.head[1][:], np.float32), mats[0]) and np.array_equal(np.array(vis.head[2][:], np.float32), focal)
    assert list(vis.head[4]) == [t.data_ptr() for t in vis.maps]

    # maps alone (depth_cues), and no views at all: arrays of one zero element
    bare = _device.ViewStack([(None, d, None) for d in depths], CPU)
    assert bare.head == [3, bare.sizes, bare.depth] and list(bare.sizes) == sizes
    none = _device.camera_views([], [], CPU)
    assert none.n == 0 and [len(a) for a in none.head[1:]] == [1, 1, 1, 1] and not any(none.head[1][:] + none.head[2][:])
    assert list(none.sizes) == [0] and not none.depth[0]
    assert len(_device.ViewStack([], CPU, True, 2, two).rgb) == 1


def test_view_stack_checks():
    cam, d = _camera(1.0, 1.0), torch.ones((2, 3))
    with pytest.raises(ValueError, match="2 cameras but 1 depth maps"):
        _device.camera_views([cam, cam], [d], CPU)
    with pytest.raises(RuntimeError, match="depth must be a tensor on cpu"):
        _device.camera_views([cam], [[[1.0]]], CPU)
    with pytest.raises(RuntimeError, match="depth must be a tensor on cuda:0"):
        _device.camera_views([cam], [d], torch.device("cuda", 0))
    for bad in (torch.ones((2, 2, 3)), torch.ones(3), torch.ones((1, 1, 2, 3))):
        with pytest.raises(RuntimeError, match=r"depth must be \[H,W\] or \[1,H,W\] \(got \(" + ", ".join(map(str, bad.shape))):
            _device.camera_views([cam], [bad], CPU)
    with pytest.raises(RuntimeError, match="colours need the rgb map of every view"):
        _device.ViewStack([(cam, d, None)], CPU, True)
    with pytest.raises(RuntimeError, match="rgb must be a tensor on cpu"):
        _device.ViewStack([(cam, d, [[0.0]])], CPU, True)
    for bad in (torch.zeros((3, 3, 2)), torch.zeros((1, 3, 2, 3)), torch.zeros((2, 3))):
        with pytest.raises(RuntimeError, match=r"rgb must have shape \(3, 2, 3\) \(got \("):
            _device.ViewStack([(cam, d, bad)], CPU, True)
    # the first view that is wrong speaks, a view's depth before its rgb
    with pytest.raises(RuntimeError, match=r"depth must be \[H,W\]"):
        _device.ViewStack([(cam, d, torch.zeros((3, 2, 3))), (cam, torch.ones(3), None)], CPU, True)
