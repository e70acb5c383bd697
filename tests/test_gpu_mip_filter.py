"""The mip filter on the fused path (include/g4s_optim.h): g4s_mip_filter against its float32 restatement bit for bit,
the activations with the filter on against float64 autograd of the same formulas, render() through get_activated
against render() through the three torch getters, and a captured training step that follows the filter."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mip_filter_ref import camera_table, filter_scale, mip_filter_ref
from g4splat_amd.gaussian_model import GaussianModel

pytestmark = pytest.mark.gpu

ZNEAR, VARIANCE = 0.2, 0.2


# ---- 1. g4s_mip_filter ------------------------------------------------------------------------------------------
def _look_at(eye):
    eye = np.asarray(eye, np.float64)
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(np.array([0.0, 1.0, 0.1]), fwd)
    right /= np.linalg.norm(right)
    w2c = np.stack([right, np.cross(fwd, right), fwd])
    return w2c.T.astype(np.float32), (-w2c @ eye).astype(np.float32)  # camera space = xyz @ R + T


def _views(V, seed):
    rng = np.random.default_rng(seed)
    cams = []
    for _ in range(V):
        eye = rng.normal(size=3)
        R, T = _look_at(eye / np.linalg.norm(eye) * rng.uniform(2.5, 5.0))
        w, h = int(rng.integers(120, 1300)), int(rng.integers(100, 900))
        cams.append(SimpleNamespace(R=R, T=T, focal_x=float(rng.uniform(0.4, 1.6) * w), focal_y=float(rng.uniform(0.4, 1.6) * w),
                                    image_width=w, image_height=h))
    return cams


def _front_camera():
    """Identity pose: camera space is world space, +z in front."""
    return SimpleNamespace(R=np.eye(3, dtype=np.float32), T=np.zeros(3, np.float32), focal_x=300.0, focal_y=310.0,
                           image_width=320, image_height=240)


def _hip_filter(xyz, cams, out=None):
    from g4splat_amd.optim import mip_filter
    return mip_filter(torch.tensor(xyz, device="cuda:0"), cams, ZNEAR, VARIANCE, out=out)


def _restated(xyz, cams):
    out, seen = mip_filter_ref(xyz, camera_table(cams), ZNEAR, filter_scale(cams, VARIANCE))
    return torch.tensor(out)[:, None], seen


@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 10_007])
def test_mip_filter_equals_the_restatement_bit_for_bit(hip_lib, P):
    """Every size around the wave and the block, 1 / 2 / 7 views (the kernel walks the table, it stages no chunk of
    it): a mixed cloud -- a cluster the cameras see, a wide box, far points -- must come out with the restatement's
    bits, and a second run with the first run's."""
    rng = np.random.default_rng(P)
    xyz = np.concatenate([rng.normal(0, 0.7, (P, 3)), rng.uniform(-6, 6, (P, 3)), rng.normal(0, 40, (P, 3))])
    xyz = xyz[rng.permutation(3 * P)[:P]].astype(np.float32)
    for V in (1, 2, 7):
        cams = _views(V, seed=100 * V + P % 7)
        want, seen = _restated(xyz, cams)
        got = _hip_filter(xyz, cams)
        assert got.shape == (P, 1) and got.dtype == torch.float32
        assert torch.equal(got.cpu(), want), (P, V, int(seen.sum()))
        assert torch.equal(_hip_filter(xyz, cams), got)
    if P == 10_007:
        assert 0 < seen.sum() < P  # both kinds of rows are present where it matters


def test_mip_filter_edge_cases(hip_lib):
    cam = [_front_camera()]
    behind = lambda n, seed: np.random.default_rng(seed).uniform((-1, -1, -3), (1, 1, -1), (n, 3)).astype(np.float32)
    front = lambda n, seed: np.random.default_rng(seed).uniform((-0.3, -0.3, 1), (0.3, 0.3, 4), (n, 3)).astype(np.float32)
    # seen rows only in the last block (two full blocks see nothing)
    xyz = np.concatenate([behind(512, 0), front(88, 1)])
    want, seen = _restated(xyz, cam)
    assert not seen[:512].any() and seen[512:].all()
    got = _hip_filter(xyz, cam).cpu()
    assert torch.equal(got, want)
    assert bool((got[:512] == got[512:].max()).all())
    # exactly one seen row: everybody takes its depth
    xyz = behind(300, 2)
    xyz[137] = (0.1, -0.05, 2.5)
    want, seen = _restated(xyz, cam)
    assert seen.sum() == 1 and seen[137]
    got = _hip_filter(xyz, cam).cpu()
    assert torch.equal(got, want) and bool((got == got[137]).all())
    # no seen row: the documented constant (the reference raises here)
    xyz = behind(300, 3)
    want, seen = _restated(xyz, cam)
    assert not seen.any()
    got = _hip_filter(xyz, cam).cpu()
    assert torch.equal(got, want)
    assert bool((got == float(np.float32(100000.0) * filter_scale(cam, VARIANCE))).all())
    # z_cam == znear exactly is NOT seen (the test is `>`); one ulp further is
    zn = np.float32(ZNEAR)
    xyz = np.array([[0, 0, zn], [0, 0, np.nextafter(zn, np.float32(1))], [0, 0, np.nextafter(zn, np.float32(0))]], np.float32)
    want, seen = _restated(xyz, cam)
    assert list(seen) == [False, True, False]
    got = _hip_filter(xyz, cam).cpu()
    assert torch.equal(got, want) and float(got[0]) == float(got[1]) == float(got[2])


def test_mip_filter_in_place_keeps_the_address(hip_lib):
    """A second computation into the same tensor (what compute_mip_filter does at unchanged P) keeps the address and
    equals a fresh call; a model whose P changed gets a new tensor."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    xyz_a = rng.normal(0, 1.0, (1000, 3)).astype(np.float32)
    xyz_b = (xyz_a + rng.normal(0, 0.5, xyz_a.shape)).astype(np.float32)
    cams = _views(3, seed=8)
    m = GaussianModel(sh_degree=0, use_mip_filter=True)
    m._xyz = torch.nn.Parameter(torch.tensor(xyz_a, device=dev))
    m.compute_mip_filter(cams, znear=ZNEAR, filter_variance=VARIANCE)
    first, addr = m.mip_filter.clone(), m.mip_filter.data_ptr()
    assert torch.equal(first.cpu(), _restated(xyz_a, cams)[0])
    with torch.no_grad():
        m._xyz.copy_(torch.tensor(xyz_b, device=dev))
    m.compute_mip_filter(cams, znear=ZNEAR, filter_variance=VARIANCE)
    assert m.mip_filter.data_ptr() == addr and not torch.equal(m.mip_filter, first)
    assert torch.equal(m.mip_filter, _hip_filter(xyz_b, cams))
    m._xyz = torch.nn.Parameter(torch.tensor(xyz_b[:700], device=dev))
    m.compute_mip_filter(cams, znear=ZNEAR, filter_variance=VARIANCE)
    assert m.mip_filter.shape == (700, 1) and torch.equal(m.mip_filter, _hip_filter(xyz_b[:700], cams))
    from g4splat_amd.optim import mip_filter
    with pytest.raises(RuntimeError):
        mip_filter(torch.tensor(xyz_a), cams)  # host tensors: the torch loop of compute_mip_filter is the CPU path
    with pytest.raises(RuntimeError):
        mip_filter(torch.tensor(xyz_a, device=dev), [])


# ---- 2. activations with the filter on --------------------------------------------------------------------------
ULP4 = 4 * 2.0 ** -23  # 4.8e-7


def _truth(s, q, o, f):
    """The header's formulas on float64 leaves."""
    e2 = torch.exp(s) ** 2
    a = e2 + f * f
    coef = torch.sqrt((e2[:, 0] * e2[:, 1]) / (a[:, 0] * a[:, 1]))[:, None]
    return torch.sqrt(a), torch.nn.functional.normalize(q), torch.sigmoid(o) * coef


@pytest.mark.parametrize("P", [1, 64, 65, 257, 200_003])
def test_fused_mip_activations_match_float64(hip_lib, P, capsys):
    """Forward and backward of fused_activations(..., mip_filter=f) against float64 autograd of the same formulas.  The
    bar is not fixed in advance: torch's own float32 getter chain (the reference's formulas: GaussianModel.get_scaling /
    get_rotation / get_opacity) is measured against the same truth, and the kernel's largest error may be at most 4x
    torch's (another expf, coef formed from the same rounded intermediates), with a floor of 4 ulp; more than that
    would be a wrong formula, not rounding.  Scaling gradient: error over |g_sc dscales/ds| + |g_op dopacity/ds| (the two
    terms can cancel)."""
    from g4splat_amd.optim import fused_activations
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(100 + P)
    raw = [torch.rand((P, 2), generator=g) * 14.0 - 12.0, torch.randn((P, 4), generator=g), torch.randn((P, 1), generator=g) * 3]
    raw[1][::1000] *= 1e-3  # nearly-degenerate quaternions
    raw[1][P // 2] = 0.0    # an exactly-zero quaternion takes the clamped branch
    f = torch.rand((P, 1), generator=g) * (0.1 - 1e-4) + 1e-4
    f[::7] = 0.0            # rows without a filter: coef = 1, scales = exp(s)
    cot = [torch.randn(t.shape, generator=g).to(dev) for t in raw]
    leaves = lambda dt: [t.clone().to(dev, dt).requires_grad_(True) for t in raw]
    fd = f.to(dev)
    # the kernel
    a = leaves(torch.float32)
    fa = fd.clone().requires_grad_(True)
    ya = fused_activations(*a, mip_filter=fa)
    sum((y * c).sum() for y, c in zip(ya, cot)).backward()
    assert fa.grad is None  # the filter receives no gradient
    # torch's float32 chain: the model's three getters
    m = GaussianModel(sh_degree=0, use_mip_filter=True)
    m._scaling, m._rotation, m._opacity = b = leaves(torch.float32)
    m.mip_filter = fd
    yb = (m.get_scaling, m.get_rotation, m.get_opacity)
    sum((y * c).sum() for y, c in zip(yb, cot)).backward()
    # float64 truth
    t = leaves(torch.float64)
    yt = _truth(*t, fd.double())
    sum((y * c.double()).sum() for y, c in zip(yt, cot)).backward()
    torch.cuda.synchronize()
    with torch.no_grad():
        s64, o64, f64 = t[0], t[2], fd.double()
        e2 = torch.exp(s64) ** 2
        a64 = e2 + f64 * f64
        term = (cot[0].double() * e2 / yt[0]).abs() + (cot[2].double() * yt[2] * (f64 * f64) / a64).abs()
        rowmax = lambda r: r.abs().max(dim=1, keepdim=True).values.clamp_min(1e-6)
        scale = {"scales": yt[0].abs(), "rotations": yt[1].abs(), "opacities": yt[2].abs(), "d scaling": term,
                 "d rotation": rowmax(t[1].grad), "d opacity": t[2].grad.abs().clamp_min(1e-6)}
        mine = {"scales": ya[0], "rotations": ya[1], "opacities": ya[2], "d scaling": a[0].grad, "d rotation": a[1].grad,
                "d opacity": a[2].grad}
        theirs = {"scales": yb[0], "rotations": yb[1], "opacities": yb[2], "d scaling": b[0].grad, "d rotation": b[1].grad,
                  "d opacity": b[2].grad}
        truth = {"scales": yt[0], "rotations": yt[1], "opacities": yt[2], "d scaling": t[0].grad, "d rotation": t[1].grad,
                 "d opacity": t[2].grad}
        figures = {}
        for k in mine:
            assert mine[k].shape == truth[k].shape and mine[k].dtype == torch.float32, k
            sc = scale[k].expand_as(truth[k])
            nz = sc > 0  # (the zero quaternion normalises to exact zeros: nothing to divide by)
            assert bool((mine[k][~nz] == 0).all()), k
            err = lambda y: float(((y.double() - truth[k]).abs()[nz] / sc[nz]).max()) if bool(nz.any()) else 0.0
            figures[k] = (err(mine[k]), err(theirs[k]))
        with capsys.disabled():
            print(f"\nmip activations P={P}: largest error, kernel / torch float32: " +
                  ", ".join(f"{k} {u:.2e} / {v:.2e}" for k, (u, v) in figures.items()))
        for k, (u, v) in figures.items():
            assert u <= max(4.0 * v, ULP4), (k, u, v)
        # rows without a filter: coef is 1 and scales are exp(s), within 1 ulp of the filter-free kernel
        plain = fused_activations(*[x.detach() for x in a])
        z = (fd[:, 0] == 0)
        ulp = 2.0 ** -23
        assert bool(((ya[0][z] - plain[0][z]).abs() <= ulp * plain[0][z]).all())
        assert bool(((ya[2][z] - plain[2][z]).abs() <= ulp * plain[2][z]).all())
        assert torch.equal(ya[1], plain[1])


def test_fused_mip_activations_refuse_bad_tensors(hip_lib):
    from g4splat_amd.optim import fused_activations
    dev = torch.device("cuda:0")
    P = 33
    s, q, o, f = (torch.zeros((P, w), device=dev) for w in (2, 4, 1, 1))
    fused_activations(s, q, o, mip_filter=f)
    odd = lambda w: torch.zeros(P * w + 1, device=dev)[1:].view(P, w)  # contiguous, 4 bytes off every wider alignment
    with pytest.raises(RuntimeError, match="aligned"):
        fused_activations(odd(2), q, o, mip_filter=f)
    with pytest.raises(RuntimeError, match="aligned"):
        fused_activations(s, odd(4), o, mip_filter=f)
    with pytest.raises(RuntimeError, match="HIP tensors only"):
        fused_activations(s, q, o, mip_filter=f.cpu())
    with pytest.raises(RuntimeError, match="HIP tensors only"):
        fused_activations(s.cpu(), q.cpu(), o.cpu(), mip_filter=f.cpu())
    with pytest.raises(RuntimeError, match="mip_filter"):
        fused_activations(s, q, o, mip_filter=f[:-1])
    m = GaussianModel(sh_degree=0, use_mip_filter=True)
    m._scaling, m._rotation, m._opacity = s, q, o
    with pytest.raises(RuntimeError, match="mip filter is on but has not been computed"):
        m.get_activated


# ---- 3. / 4. render() and the captured training step -----------------------------------------------------------------
def _mip_cameras(cams):
    """The reference's camera fields compute_mip_filter reads, from the render cameras (world_view_transform = W2C^T)."""
    out = []
    for c in cams:
        wvt = c.world_view_transform.cpu().numpy()
        w, h = int(c.image_width), int(c.image_height)
        out.append(SimpleNamespace(R=wvt[:3, :3].copy(), T=wvt[3, :3].copy(), focal_x=w / (2 * math.tan(c.FoVx / 2)),
                                   focal_y=h / (2 * math.tan(c.FoVy / 2)), image_width=w, image_height=h))
    return out


class _TorchGetters(GaussianModel):
    """The same model read through the three torch getters."""
    get_activated = property(lambda self: (self.get_scaling, self.get_rotation, self.get_opacity))


def test_render_with_the_filter_on_matches_the_torch_getters(hip_lib):
    """200 Gaussians, 64x48: outputs and every parameter gradient through get_activated (fused) against the three
    getters (torch), within the bars tests/test_gpu_render.py holds the HIP path to."""
    from g4splat_amd import synthetic
    from g4splat_amd.gaussian_renderer import render
    from render_scenes import render_loss
    dev = torch.device("cuda:0")
    W, H, P = 64, 48, 200
    cam = synthetic.look_at_camera((0.4, -0.3, -2.6), (0, 0, 0), (0, 1, 0), 1.0, W, H)
    cam = SimpleNamespace(image_width=W, image_height=H, FoVx=cam.FoVx, FoVy=cam.FoVy,
                          world_view_transform=torch.tensor(cam.world_view_transform, device=dev),
                          full_proj_transform=torch.tensor(cam.full_proj_transform, device=dev),
                          camera_center=torch.tensor(cam.camera_center, device=dev), znear=0.01, zfar=100.0)
    t = lambda a: torch.tensor(a.astype(np.float32), device=dev)
    outs, models = [], []
    for cls in (GaussianModel, _TorchGetters):
        r = np.random.default_rng(11)
        m = cls(sh_degree=3, use_mip_filter=True)
        m.create_from_parameters(t(r.uniform(-0.9, 0.9, (P, 3))), t(r.uniform(0.01, 0.15, (P, 2))), t(r.normal(size=(P, 4))),
                                 t(r.uniform(0, 1, (P, 3))))
        with torch.no_grad():
            m._opacity += 2.5
        m.active_sh_degree = 1
        m.compute_mip_filter(_mip_cameras([cam]), znear=ZNEAR, filter_variance=2.0)
        out = render(cam, m, SimpleNamespace(depth_ratio=0.5, compute_cov3D_python=False), torch.tensor([0.1, 0.2, 0.3], device=dev))
        render_loss(out).backward()
        outs.append(out)
        models.append(m)
    torch.cuda.synchronize()
    assert float(models[0].mip_filter.min()) > 0.01  # the filter is of the order of the splats: it matters in this image
    a, b = outs
    for k in a:
        if k == "viewspace_points":
            continue
        if a[k].dtype.is_floating_point:
            assert float((a[k] - b[k]).detach().abs().max()) <= 2e-4, k
        else:
            assert torch.equal(a[k], b[k]), k
    for name, p, q in zip(("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"), models[0].parameters(), models[1].parameters()):
        assert float((p.grad - q.grad).abs().max()) <= 1e-3 * float(q.grad.abs().max()) + 1e-9, name
    g2, r2 = a["viewspace_points"].grad, b["viewspace_points"].grad
    assert float((g2 - r2).abs().max()) <= 1e-3 * float(r2.abs().max()) + 1e-9


def test_graphed_training_step_follows_the_mip_filter(hip_lib):
    """TrainStepGraph with the filter on, the small scene of test_training_iteration_replayed_from_a_hip_graph_equals_the_
    eager_loop: replays equal the eager loop bit for bit; compute_mip_filter at unchanged P writes in place and the next
    replays read the new values (again equal to eager steps); rebinding the filter makes the graph stale."""
    from g4splat_amd.gaussian_renderer import render
    from g4splat_amd.graphed import TrainStepGraph
    from g4splat_amd.losses import geometry_regularizers, photometric_loss
    from render_scenes import TRAIN_H as H, TRAIN_W as W, train_cams, train_model
    dev = torch.device("cuda", 0)
    cams = train_cams(dev)[:3]
    mip_cams = _mip_cameras(cams)
    g = torch.Generator(device=dev).manual_seed(3)
    gts = [torch.rand((3, H, W), device=dev, generator=g) for _ in cams]

    def body(out, gt):
        loss, _l1, _s = photometric_loss(out["render"], gt, 0.2)
        normal_mean, dist_mean = geometry_regularizers(out["rend_normal"], out["surf_normal"], out["rend_dist"])
        return loss + 0.05 * normal_mean + 100.0 * dist_mean

    def fresh():
        m = train_model(0, dev, jitter=True)
        m.set_mip_filter(True)
        m.compute_mip_filter(mip_cams, znear=ZNEAR, filter_variance=VARIANCE)
        m.training_setup(capturable=True)
        return m

    pipe = SimpleNamespace(depth_ratio=0.0, compute_cov3D_python=False)
    bg = torch.zeros(3, device=dev)

    def eager(m, it):
        m.update_learning_rate(it + 1)
        out = render(cams[it % 3], m, pipe, bg)
        loss = body(out, gts[it % 3])
        loss.backward()
        with torch.no_grad():
            m.add_densification_stats(out["viewspace_points"], out["visibility_filter"], out["radii"])
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
        return float(loss.detach())

    def same(a, b):
        for name, p, q in zip(("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"), a.parameters(), b.parameters()):
            assert torch.equal(p, q), name
        for pa, pb in zip(a.parameters(), b.parameters()):
            sa, sb = a.optimizer.state[pa], b.optimizer.state[pb]
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
        assert torch.equal(a.xyz_gradient_accum, b.xyz_gradient_accum) and torch.equal(a.denom, b.denom)

    a, b = fresh(), fresh()
    assert torch.equal(a.mip_filter, b.mip_filter)
    step = TrainStepGraph(b, body, cams[0], (3, H, W), instance_capacity=200_000)
    iters = 6
    losses_a = [eager(a, it) for it in range(iters)]
    losses_b = []
    for it in range(iters):
        b.update_learning_rate(it + 1)
        losses_b.append(float(step(cams[it % 3], gts[it % 3])))
    assert not step.overflowed() and losses_a == losses_b, (losses_a, losses_b)
    same(a, b)
    # the filter is recomputed at unchanged P (after an opacity reset in the trainer): same storage, new values
    addr, old = b.mip_filter.data_ptr(), b.mip_filter.clone()
    for m in (a, b):
        m.compute_mip_filter(mip_cams[:1], znear=ZNEAR, filter_variance=3.0)
    assert b.mip_filter.data_ptr() == addr and not torch.equal(b.mip_filter, old)
    for it in range(iters, iters + 3):
        la = eager(a, it)
        b.update_learning_rate(it + 1)
        assert la == float(step(cams[it % 3], gts[it % 3])), it
    same(a, b)
    # a filter that moved (or was switched off) is not what the graph reads: refuse
    b.mip_filter = b.mip_filter.clone()
    with pytest.raises(RuntimeError, match="stale.*mip filter"):
        step(cams[0], gts[0])
    b.mip_filter = None
    b.set_mip_filter(False)
    with pytest.raises(RuntimeError, match="stale.*mip filter"):
        step(cams[0], gts[0])
