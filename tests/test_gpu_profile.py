"""The per-kernel profiling (g4s_profile_*) across translation units: the recording scope lives in api.hip, the entry
points that open it beside their kernels in loss.hip, optim.hip and maps.hip.  Every group counts exactly the calls made
in it and no other group counts anything; the values computed under profiling are checked against the torch
restatements of test_gpu_losses.py / test_gpu_optim.py at those files' tolerances."""
import ctypes
import math

import pytest
import torch

from g4splat_amd import _lib
from g4splat_amd.losses import geometry_regularizers, photometric_loss
from g4splat_amd.render_maps import render_maps
from oracle import losses_ref
from render_scenes import MAP_NAMES, allmap, maps_camera

pytestmark = pytest.mark.gpu

W, H = 21, 19  # ragged against the 16-pixel tile of the loss kernels and the 64x4 block of the map kernels
BETA1, BETA2, EPS, LR = 0.9, 0.999, 1e-15, 0.01


def _adam_inputs(dev, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(5, generator=g).to(dev) for _ in range(2)] + [torch.zeros(5, device=dev) for _ in range(2)]


def test_groups_count_the_calls_made_in_them(hip_lib):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    gt = torch.rand((3, H, W), generator=g).to(dev)
    img = (gt + 0.1 * torch.randn((3, H, W), generator=g).to(dev)).clamp(0, 1)
    rn, sn, rd = (torch.randn(s, generator=g).to(dev) for s in ((3, H, W), (3, H, W), (1, H, W)))
    geo = [t.clone().requires_grad_(True) for t in (rn, sn, rd.abs())]
    x = img.clone().requires_grad_(True)
    am = torch.tensor(allmap(W, H, 5), device=dev, requires_grad=True)
    cam = maps_camera(W, H, dev="cuda:0")
    host = _adam_inputs(dev, 7)    # g4s_adam_step: p, g, m, v of the 5-element segment
    devi = _adam_inputs(dev, 7)    # g4s_adam_step_device: the same
    lr_dev = torch.full((2,), LR, dtype=torch.float64, device=dev)
    steps = [torch.zeros((), dtype=torch.float32, device=dev) for _ in range(2)]
    coef = torch.zeros(16, dtype=torch.float32, device=dev)
    numel = _lib.array(ctypes.c_longlong, [5, 0])
    seg = lambda t: _lib.ptrs([t, None])  # the second segment is empty: no pointers
    stream = _lib.stream(dev)
    torch.cuda.synchronize()

    hip_lib.g4s_profile_reset()
    hip_lib.g4s_profile_enable(1)
    try:
        loss, l1, ss = photometric_loss(x, gt, 0.2)  # one call: the gradient image is written by the forward
        ne, dm = geometry_regularizers(*geo)
        (0.05 * ne + 100.0 * dm).backward()
        _lib.call("g4s_adam_step", 2, seg(host[0]), seg(host[1]), seg(host[2]), seg(host[3]), numel,
                  _lib.array(ctypes.c_double, [LR, LR]), _lib.array(ctypes.c_int, [1, 1]), BETA1, BETA2, EPS, stream)
        _lib.call("g4s_adam_step_device", 2, seg(devi[0]), seg(devi[1]), seg(devi[2]), seg(devi[3]), numel, _lib.ptr(lr_dev),
                  _lib.ptrs(steps), _lib.ptr(coef), BETA1, BETA2, EPS, stream)
        out = render_maps(am, cam, 0.5)
        sum(out[k].sum() for k in MAP_NAMES).backward()
    finally:
        hip_lib.g4s_profile_enable(0)
    torch.cuda.synchronize()
    want = {"photometric_loss": 1, "geometry_regularizers": 2, "adam": 2, "maps_fwd": 1, "maps_bwd": 1}
    seen = {}
    for k in range(hip_lib.g4s_profile_kernels()):
        ms, cnt = ctypes.c_double(), ctypes.c_int()
        assert hip_lib.g4s_profile_read(k, ctypes.byref(ms), ctypes.byref(cnt)) == 0
        name = hip_lib.g4s_profile_name(k).decode()
        seen[name] = cnt.value
        assert cnt.value == want.get(name, 0), (name, cnt.value)
        assert math.isfinite(ms.value) and ms.value >= 0.0, (name, ms.value)
    hip_lib.g4s_profile_reset()
    assert set(want) <= set(seen)

    # the photometric loss against eager torch (test_gpu_losses.py)
    (3.0 * loss).backward()
    x2 = img.clone().requires_grad_(True)
    rl, r1, rs = losses_ref.photometric_loss(x2, gt, 0.2)
    (3.0 * rl).backward()
    assert abs(float(loss.detach()) - float(rl.detach())) <= 1e-5 and abs(float(l1) - float(r1.detach())) <= 1e-6
    assert abs(float(ss) - float(rs.detach())) <= 1e-5
    assert float((x.grad - x2.grad).abs().max()) <= 1e-3 * float(x2.grad.abs().max())
    # Adam against torch.optim.Adam's first step (test_gpu_optim.py), both entry points
    p0, grad = _adam_inputs("cpu", 7)[:2]
    ref = torch.nn.Parameter(p0.clone())
    ref.grad = grad.clone()
    opt = torch.optim.Adam([ref], lr=LR, betas=(BETA1, BETA2), eps=EPS)
    opt.step()
    moved = (ref.detach() - p0).abs().max()
    for got in (host, devi):
        d = (got[0].cpu() - ref.detach()).abs().max()
        assert d <= 2e-5 * moved + 2.4e-7 * float(ref.detach().abs().max()), (float(d), float(moved))
        for t, key in ((got[2], "exp_avg"), (got[3], "exp_avg_sq")):
            w = opt.state[ref][key]
            assert (t.cpu() - w).abs().max() <= 1e-5 * w.abs().max(), key
    assert torch.equal(host[0], devi[0])
    assert [float(s) for s in steps] == [1.0, 1.0]  # the device path advances every segment's count, empty or not
