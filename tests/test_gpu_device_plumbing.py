"""The launch helper of g4splat_amd/_device.py on the device: the three kinds of workspace, the synchronisation it is asked
for, and the error it raises for a status the library returns."""
from types import SimpleNamespace

import pytest
import torch

from g4splat_amd import _device, _lib, visibility
from support import DEV

pytestmark = pytest.mark.gpu


def _camera():
    view = torch.tensor([[0.8, 0.0, -0.6, 0.0], [0.0, 1.0, 0.0, 0.0], [0.6, 0.0, 0.8, 0.0], [0.1, -0.2, 2.0, 1.0]])
    proj = torch.tensor([[1.2, 0.0, 0.0, 0.0], [0.0, 1.6, 0.0, 0.0], [0.0, 0.0, 1.0, 1.0], [0.0, 0.0, -0.01, 0.0]])
    return SimpleNamespace(world_view_transform=view, full_proj_transform=view @ proj, FoVx=1.0, FoVy=0.8)


def test_launch_without_a_workspace_synchronises_when_asked(hip_lib):
    cam, (H, W) = _camera(), (2, 3)
    depth = torch.tensor([[1.0, 2.5, 0.0], [3.0, 0.125, 7.0]], device=DEV)
    want = visibility.depths_to_points(depth, cam)
    ray = _device.host_f32(visibility.ray_record(cam, W, H))
    got = torch.full((H * W, 3), float("nan"), device=DEV)
    assert _device.launch(DEV, "g4s_depth_to_points", W, H, _lib.ptr(depth), ray, _lib.ptr(got), workspace=None, sync=True) is None
    assert torch.cuda.current_stream(DEV).query()  # idle on return
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    later = torch.full_like(got, float("nan"))
    _device.launch(DEV, "g4s_depth_to_points", W, H, _lib.ptr(depth), ray, _lib.ptr(later))  # sync=False: the caller waits
    torch.cuda.current_stream(DEV).synchronize()
    assert torch.equal(later.view(torch.int32), want.view(torch.int32))


def test_launch_allocates_or_takes_the_workspace(hip_lib):
    tris = torch.tensor([[0, 1, 2], [2, 1, 3], [4, 5, 6]], dtype=torch.int32, device=DEV)  # the first two share edge (1, 2)
    nbytes = hip_lib.g4s_mesh_cluster_workspace(3)
    assert nbytes > 0
    for sync in (False, True):
        labels, sizes = torch.full((3,), -7, dtype=torch.int32, device=DEV), torch.full((3,), -7, dtype=torch.int32, device=DEV)
        ws = _device.launch(DEV, "g4s_mesh_cluster_triangles", 3, _lib.ptr(tris), _lib.ptr(labels), _lib.ptr(sizes), workspace=nbytes,
                            sync=sync)
        if sync:
            assert torch.cuda.current_stream(DEV).query()
        else:
            torch.cuda.current_stream(DEV).synchronize()
        assert labels.tolist() == [0, 0, 2] and sizes.tolist() == [2, 2, 1]
        assert ws.dtype == torch.uint8 and ws.numel() == nbytes and ws.device == DEV
    # the returned tensor is what a count / emit pair hands to its second call
    labels.fill_(-7)
    sizes.fill_(-7)
    assert _device.launch(DEV, "g4s_mesh_cluster_triangles", 3, _lib.ptr(tris), _lib.ptr(labels), _lib.ptr(sizes), workspace=ws,
                          sync=True) is ws
    assert labels.tolist() == [0, 0, 2] and sizes.tolist() == [2, 2, 1]


def test_a_refused_call_raises_with_the_symbol_and_the_message(hip_lib):
    depth, points = torch.ones((2, 3), device=DEV), torch.zeros((6, 3), device=DEV)
    ray = _device.host_f32(visibility.ray_record(_camera(), 3, 2))
    for W, H in ((0, 2), (3, -1)):  # refused on the host: no kernel runs
        with pytest.raises(RuntimeError) as err:
            _device.launch(DEV, "g4s_depth_to_points", W, H, _lib.ptr(depth), ray, _lib.ptr(points), sync=True)
        message = _lib.last_error()
        assert message and str(err.value).startswith("g4s_depth_to_points failed (") and str(err.value).endswith(": " + message)
    assert not points.any()
