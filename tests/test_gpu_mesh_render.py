"""The mesh rasteriser and the dilated depth on the MI355X against the numpy restatement of the contract
(tests/mesh_render_ref.py) bit for bit, the Python surface of g4splat_amd/mesh_render.py, and the two depth switches of
GaussianExtractor.extract_mesh_tetra."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mesh_render_ref as mr
import tetra_ref as tr
from g4splat_amd import mesh as mesh_mod
from g4splat_amd import mesh_render as mrn
from g4splat_amd import synthetic
from support import DEV, dev, device_camera, host, same_bits, twice

pytestmark = pytest.mark.gpu

f32 = np.float32
BACKGROUND = (0.1, 0.2, 0.3)
ALL = ("pix_to_face", "zbuf", "bary", "attr", "normal", "stats")


def _colours(n, seed=5):
    return np.random.default_rng(seed).uniform(0, 1, (n, 3)).astype(f32)


def _gpu_render(dm, Wv, Pm, W, H, off, seen=None):
    """Every output of one g4s_mesh_raster call, as host arrays; `seen` is accumulated into."""
    if seen is None:
        seen = torch.zeros(max(dm.triangles.size(0), 1), dtype=torch.uint8, device=DEV)
    o = mrn._raster(dm, (Wv, Pm), (H, W), off, 1e-6, ALL, attributes=dm.vertex_colors, background=BACKGROUND,
                    flags=mrn.FLIP_NORMALS | mrn.SURFELS_CONVENTION, seen=seen)
    return [host(o[k]) for k in ALL] + [host(seen)[: dm.triangles.size(0)]]


def _want(vertices, colours, faces, Wv, Pm, W, H, off):
    r = mr.render(vertices, faces, Wv, Pm, W, H, off=off, attributes=colours, background=BACKGROUND, centre=np.zeros(3, f32))
    return [r.pix_to_face, r.zbuf, r.bary, r.attr, r.normal, r.stats, r.seen]


def _compare(vertices, colours, faces, Wv, Pm, W, H, off, dm=None):
    if dm is None:
        dm = mesh_mod.DeviceMesh(dev(vertices), dev(colours), dev(faces))
    got = twice(lambda: _gpu_render(dm, Wv, Pm, W, H, off))  # two runs give identical bytes
    want = _want(vertices, colours, faces, Wv, Pm, W, H, off)
    for g, w, name in zip(got, want, ALL + ("seen",)):
        same_bits(g, w, name)
    return want


# ---- the rasteriser ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diagonal", [0, 1])
@pytest.mark.parametrize("winding", [0, 1])
def test_split_quads_equal_the_restatement(hip_lib, diagonal, winding):
    for corners in ((3, 2, 11, 9), (3, 2, 9, 8)):
        Wq, Hq, fq, z = 16, 12, 8.0, 2.0
        x0, y0, x1, y1 = corners
        pts = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
        vertices = np.array([[((2 * x / Wq - 1) / (2 * fq / Wq)) * z, ((2 * y / Hq - 1) / (2 * fq / Hq)) * z, z] for x, y in pts], f32)
        faces = [[0, 1, 2], [0, 2, 3]] if diagonal == 0 else [[0, 1, 3], [1, 2, 3]]
        faces = np.array([f[::-1] for f in faces] if winding else faces, np.int32)
        Wv, Pm = mr.pinhole(Wq, Hq, fq, fq)
        pix = _compare(vertices, _colours(4), faces, Wv, Pm, Wq, Hq, 0.0)[0]
        want = np.zeros((Hq, Wq), bool)
        want[y0:y1, x0:x1] = True  # top and left borders owned, bottom and right not; the diagonal once
        assert np.array_equal(pix >= 0, want)


def _soup_with_traps(seed=1):
    """The 300-face soup of the CPU file plus one face of every kind the contract skips.  The vertex tensor is a view into
    a larger buffer whose rows before and after it hold a point that would draw a near, screen-filling face if an
    out-of-range index were used as an address."""
    W, H = 67, 45
    vertices, faces = mr.soup(seed, 300, 0.25, W, H, 60.0)
    extra = np.array([[0.0, 0.0, -3.0], [0.5, 0.0, -3.0], [0.0, 0.5, -3.0],   # 900..902: behind the camera
                      [0.0, 0.0, -1.0],                                          # 903: with 0, 1 a face straddling znear
                      [np.nan, 0.0, 3.0],                                        # 904
                      [3000.0, 0.0, 2.0]], f32)                                  # 905: beyond the guard band
    vertices = np.concatenate([vertices, extra])
    V = len(vertices)
    traps = np.array([[0, 0, 1],            # zero area
                      [900, 901, 902],      # behind
                      [903, 0, 1],          # straddles znear
                      [904, 3, 4],          # a NaN vertex
                      [0, 1, V],            # names index V
                      [-1, 1, 2],           # names index -1
                      [905, 6, 7]], np.int32)  # guard band
    faces = np.concatenate([traps[:4], faces[:150], traps[4:], faces[150:]])
    sentinel = np.array([-40.0, -40.0, 1.0], f32)  # with two soup vertices this would cover much of the image at depth ~1
    buffer = dev(np.concatenate([sentinel[None], vertices, sentinel[None]]))
    colours = _colours(V)
    dm = mesh_mod.DeviceMesh(buffer[1:V + 1], dev(colours), dev(faces))
    assert dm.vertices.data_ptr() == buffer.data_ptr() + 12
    return SimpleNamespace(W=W, H=H, vertices=vertices, faces=faces, colours=colours, dm=dm, buffer=buffer)


@pytest.mark.parametrize("off", [0.5, 0.0])
def test_the_soup_with_every_skipped_kind_equals_the_restatement(hip_lib, off):
    s = _soup_with_traps()
    Wv, Pm = mr.pinhole(s.W, s.H, 60.0, 60.0)
    pix, zbuf, _b, _a, _n, stats, seen = _compare(s.vertices, s.colours, s.faces, Wv, Pm, s.W, s.H, off, dm=s.dm)
    assert list(stats) == [3, 1]
    trap_faces = [0, 1, 2, 3, 154, 155, 156]
    assert not seen[trap_faces].any() and not np.isin(pix, trap_faces).any()
    assert (pix >= 0).mean() > 0.25 and zbuf[pix >= 0].min() > 1.5  # nothing near: the sentinel rows were not read
    assert seen.sum() == len(np.unique(pix[pix >= 0]))


def test_a_screen_filling_triangle_among_sub_pixel_faces(hip_lib):
    """The large-face path and the two sides of its threshold: one triangle over all of 256 x 256, 1000 sub-pixel faces in
    front of and behind it, and 60 faces whose boxes straddle 64 samples."""
    W = H = 256
    fq = 200.0
    rng = np.random.default_rng(11)
    big = np.array([[-10.0, -10.0, 4.0], [30.0, -10.0, 4.0], [-10.0, 30.0, 4.0]], f32)
    z = np.where(rng.uniform(size=1000) < 0.5, rng.uniform(2, 3, 1000), rng.uniform(5, 6, 1000))
    c = np.stack([rng.uniform(-0.6, 0.6, 1000) * z, rng.uniform(-0.6, 0.6, 1000) * z, z], 1)
    small = (c[:, None, :] + rng.uniform(-0.004, 0.004, (1000, 3, 3))).astype(f32)
    zm = rng.uniform(2, 3, 60)
    cm = np.stack([rng.uniform(-0.5, 0.5, 60) * zm, rng.uniform(-0.5, 0.5, 60) * zm, zm], 1)
    size = rng.uniform(6, 30, 60)[:, None, None] * (zm[:, None, None] / fq)  # vertices in a square of 6 .. 30 pixels
    medium = (cm[:, None, :] + rng.uniform(-0.5, 0.5, (60, 3, 3)) * size * np.array([1, 1, 0.2])).astype(f32)
    vertices = np.concatenate([small[:500].reshape(-1, 3), big, small[500:].reshape(-1, 3), medium.reshape(-1, 3)])
    faces = np.arange(len(vertices), dtype=np.int32).reshape(-1, 3)
    Wv, Pm = mr.pinhole(W, H, fq, fq)
    for off in (0.5, 0.0):
        pix, *_rest = _compare(vertices, _colours(len(vertices)), faces, Wv, Pm, W, H, off)
        assert (pix >= 0).all()  # the big triangle fills what nothing else does
        assert (pix == 500).mean() > 0.8 and (pix < 500).sum() > 3 and (pix > 1000).sum() > 100
    fc = mr.setup(*mr.face_positions(vertices, faces), Wv, Pm, W, H, 0.5, 1e-6)
    samples = (fc.x1 - fc.x0 + 1).clip(0) * (fc.y1 - fc.y0 + 1).clip(0)
    assert samples[500] == W * H and (samples[:500] <= 4).all()
    assert ((samples > 64) & (samples < 1000)).sum() >= 5 and ((samples > 8) & (samples <= 64)).sum() >= 5  # both sides of the threshold


def test_no_faces_and_one_pixel(hip_lib):
    Wv, Pm = mr.pinhole(67, 45, 60.0, 60.0)
    vertices = np.zeros((3, 3), f32)
    _compare(vertices, _colours(3), np.zeros((0, 3), np.int32), Wv, Pm, 67, 45, 0.5)
    pix, zbuf, bary = mrn.rasterize_mesh(mesh_mod.DeviceMesh(dev(vertices), dev(_colours(3)), dev(np.zeros((0, 3), np.int32))),
                                         (Wv, Pm), image_size=(45, 67))
    assert (host(pix) == -1).all() and (host(zbuf) == 0).all() and (host(bary) == 0).all()
    # one pixel: a face over the optical axis is seen with off = 0.5 (sample at the image centre)
    Wv1, Pm1 = mr.pinhole(1, 1, 0.5, 0.5)
    tri = np.array([[-1.0, -1.0, 2.0], [2.0, -1.0, 2.5], [-1.0, 2.0, 3.0]], f32)
    one = np.array([[0, 1, 2]], np.int32)
    for off in (0.5, 0.0):
        pix1 = _compare(tri, _colours(3), one, Wv1, Pm1, 1, 1, off)[0]
        assert pix1.shape == (1, 1)
    assert _want(tri, _colours(3), one, Wv1, Pm1, 1, 1, 0.5)[0][0, 0] == 0


def _three_cameras():
    cams = []
    for t in ((0.0, 0.0, 0.0), (1.5, 0.2, 0.5), (-1.2, -0.3, 1.0)):
        Wv = np.eye(4, dtype=f32)
        Wv[3, :3] = t
        cams.append((Wv, mr.pinhole(67, 45, 60.0, 60.0)[1]))
    return cams


def test_visible_faces_over_three_cameras_and_the_cull(hip_lib):
    vertices, faces = mr.soup(2, 300, 0.25)
    colours = _colours(len(vertices))
    cams, sizes = _three_cameras(), [(45, 67)] * 3
    dm = mesh_mod.DeviceMesh(dev(vertices), dev(colours), dev(faces))
    mask = mrn.visible_face_mask(dm, cams, sizes)
    assert mask.dtype == torch.bool and mask.shape == (300,)
    want = np.zeros(300, bool)
    for cam in cams:
        pix = host(mrn.rasterize_mesh(dm, cam, image_size=(45, 67))[0])
        same_bits(pix, mr.render(vertices, faces, cam[0], cam[1], 67, 45).pix_to_face)
        want[np.unique(pix[pix >= 0])] = True
    assert np.array_equal(host(mask), want) and 50 < want.sum() < 300
    # the cull returns the kind it was given
    on_device = mrn.cull_unseen_faces(dm, cams, sizes)
    assert isinstance(on_device, mesh_mod.DeviceMesh) and on_device.triangles.size(0) == want.sum()
    on_host = mrn.cull_unseen_faces(mesh_mod.TriangleMesh(vertices, colours, faces), cams, sizes)
    assert isinstance(on_host, mesh_mod.TriangleMesh) and on_host.triangles.shape == (want.sum(), 3)
    assert np.array_equal(on_host.triangles, host(on_device.triangles))
    assert np.array_equal(on_host.vertices[on_host.triangles], vertices[faces[want]])


def test_render_mesh_returns_the_references_dict(hip_lib):
    vertices, faces = mr.soup(1, 300, 0.25)
    colours = _colours(len(vertices))
    cam = synthetic.look_at_camera((0.3, -0.2, -0.5), (0.0, 0.0, 4.0), (0.0, -1.0, 0.0), math.radians(60), 67, 45)
    dc = device_camera(cam)
    maps = mrn.render_mesh(mesh_mod.TriangleMesh(vertices, colours, faces), dc, background_color=BACKGROUND)
    assert set(maps) == {"rgb", "depth", "normal", "pix_to_face", "bary_coords"}
    Wv, Pm = np.asarray(cam.world_view_transform, f32), mesh_mod._projection_matrix(dc)
    r = mr.render(vertices, faces, Wv, Pm, 67, 45, attributes=colours, background=BACKGROUND,
                  centre=np.asarray(cam.camera_center, f32))
    assert (r.pix_to_face >= 0).mean() > 0.05
    for got, want, name in ((maps["rgb"], r.attr, "rgb"), (maps["depth"], r.zbuf, "depth"), (maps["normal"], r.normal, "normal"),
                            (maps["pix_to_face"], r.pix_to_face, "pix_to_face"), (maps["bary_coords"], r.bary, "bary")):
        same_bits(got, want, name)
    plain = mrn.render_mesh(mesh_mod.TriangleMesh(vertices, colours, faces), dc, use_gaussian_surfels_convention=False,
                            flip_normals_toward_camera=False)
    want_plain = mr.render(vertices, faces, Wv, Pm, 67, 45, centre=None, flip=False, surfels=False).normal
    same_bits(plain["normal"], want_plain, "unflipped normal")


# ---- dilated depth -------------------------------------------------------------------------------------------------------
DW, DH, DF = 33, 29, 40.0


def _pm(W=DW, H=DH, f=DF):
    return mr.pinhole(W, H, f, f)[1]


def _camera(W=DW, H=DH, f=DF):
    return (np.eye(4, dtype=f32), _pm(W, H, f))


def _smooth(W=DW, H=DH):
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (2.5 + 0.4 * np.sin(jj / 7.0) + 0.3 * np.cos(ii / 5.0)).astype(f32)


def _cpu_maps():
    """The maps of tests/test_mesh_render_cpu.py: (name, depth, rgb, dilation_pixels, max_dilation)."""
    constant = np.full((DH, DW), 2.0, f32)
    step = np.full((DH, DW), 3.0, f32)
    step[:, :16] = 1.0
    holes = _smooth()
    holes[10:14, 12:17] = 0.0
    holes[20, 5] = np.inf
    rgb3 = np.random.default_rng(3).uniform(-0.2, 1.2, (3, DH, DW)).astype(f32)
    rgb4 = np.random.default_rng(4).uniform(0, 1, (3, DH, DW)).astype(f32)
    return [("constant", constant, None, 1.5, 1e8), ("constant, limited", constant, None, 1.5, 0.05),
            ("identity", _smooth(), rgb3, 0.0, 1e8), ("step", step, None, 1.5, 1e8), ("holes", holes, rgb4, 0.0, 1e8),
            ("holes, dilated", holes, rgb4, 0.5, 1e8)]


@pytest.mark.parametrize("case", range(6))
def test_dilated_maps_equal_the_restatement(hip_lib, case):
    name, depth, rgb, pixels, limit = _cpu_maps()[case]
    want_d, want_c, pix = mr.dilate(depth, _pm(), pixels, limit, rgb=rgb)
    assert (pix >= 0).mean() > 0.5
    (got_d, got_c), = twice(lambda: [tuple(None if t is None else host(t) for t in pair)
                                     for pair in mrn.dilated_depths([(_camera(), dev(depth), dev(rgb))], pixels, limit)])
    same_bits(got_d, want_d, name)
    same_bits(got_c, want_c, name + " rgb")


def test_two_views_in_one_call_equal_two_calls(hip_lib):
    rng = np.random.default_rng(8)
    a = (_camera(), _smooth(), rng.uniform(0, 1, (3, DH, DW)).astype(f32))
    b = (_camera(20, 47, 30.0), _smooth(20, 47) + f32(0.5), rng.uniform(0, 1, (3, 47, 20)).astype(f32))
    views = [(cam, dev(d), dev(c)) for cam, d, c in (a, b)]
    both = mrn.dilated_depths(views, 1.5, 0.04)
    assert both[0][0].shape == (DH, DW) and both[1][0].shape == (47, 20) and both[1][1].shape == (3, 47, 20)
    for view, (d, c), (cam, depth, rgb) in zip(views, both, (a, b)):
        (d1, c1), = mrn.dilated_depths([view], 1.5, 0.04)
        same_bits(d, d1)
        same_bits(c, c1)
        want_d, want_c, _pix = mr.dilate(depth, cam[1], 1.5, 0.04, rgb=rgb)
        same_bits(d, want_d)
        same_bits(c, want_c)
    # rgb absent
    (d, c), = mrn.dilated_depths([(views[1][0], views[1][1], None)], 1.5, 0.04)
    assert c is None
    same_bits(d, both[1][0])
    assert mrn.dilated_depths([]) == []


def test_faces_that_a_depth_step_blows_up_go_through_the_list(hip_lib):
    """A dilation of 12 pixels across a step from depth 1 to 3 pulls faces over boxes of more than 64 samples: the
    dilation's large-face list, in the first and in the last of three views of different sizes, so that the global face
    ids, the search for their view and the views' key offsets all carry work."""
    rng = np.random.default_rng(12)
    stack = [(_camera(), mr.step_map(DW, DH, 16, True)), (_camera(24, 18, 25.0), _smooth(24, 18)),
             (_camera(20, 47, 30.0), mr.step_map(20, 47, 20, False))]
    rgbs = [rng.uniform(0, 1, (3,) + d.shape).astype(f32) for _cam, d in stack]
    large = [(mr.box_samples(mr.dilated_faces(d, cam[1], 12.0, 1e8)) > 64).sum() for cam, d in stack]
    print("faces with more than 64 samples per view:", large)
    assert large[0] >= 5 and large[1] == 0 and large[2] >= 5  # from the restatement alone
    views = [(cam, dev(d), dev(c)) for (cam, d), c in zip(stack, rgbs)]
    got = twice(lambda: [(host(d), host(c)) for d, c in mrn.dilated_depths(views, 12.0, 1e8)])
    for (cam, depth), rgb, (d, c), view in zip(stack, rgbs, got, views):
        want_d, want_c, _pix = mr.dilate(depth, cam[1], 12.0, 1e8, rgb=rgb)
        same_bits(d, want_d)
        same_bits(c, want_c)
        (d1, c1), = mrn.dilated_depths([view], 12.0, 1e8)
        same_bits(d1, want_d)
        same_bits(c1, want_c)


def test_get_dilated_depth_keeps_the_references_shapes(hip_lib):
    depth, rgb = _smooth(), np.random.default_rng(9).uniform(0, 1, (3, DH, DW)).astype(f32)
    want_d, want_c, _pix = mr.dilate(depth, _pm(), 1.5, 0.03, rgb=rgb)
    cam = _camera()
    for shape in ((1, DH, DW), (DH, DW), (DH, DW, 1)):
        d, c = mrn.get_dilated_depth(cam, dev(depth.reshape(shape)), 1.5, rgb=dev(rgb), max_dilation=0.03)
        assert d.shape == shape and c.shape == (3, DH, DW)
        same_bits(host(d).reshape(DH, DW), want_d)
        same_bits(c, want_c)
    d, c = mrn.get_dilated_depth(cam, dev(depth), 1.5, rgb=dev(np.ascontiguousarray(rgb.transpose(1, 2, 0))), max_dilation=0.03)
    assert c.shape == (DH, DW, 3)
    same_bits(host(c).transpose(2, 0, 1), want_c)
    d, c = mrn.get_dilated_depth(cam, dev(depth), 1.5, max_dilation=0.03)
    assert c is None
    same_bits(d, want_d)


# ---- the two depth switches of the tetrahedral extraction ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def room(hip_lib):
    """The small scene of tests/test_gpu_mesh_tetra.py's end-to-end test: 20 000 Gaussians of a room, six views of 160 x 120."""
    from g4splat_amd.gaussian_model import GaussianModel
    from g4splat_amd.gaussian_renderer import render
    n = 20000
    sc = synthetic.scene_room(n, seed=4, size=(6.0, 4.0, 3.0), scale_mean=0.12, scale_sigma=0.2)
    model = GaussianModel(sh_degree=3)
    model.create_from_parameters(dev(sc.means3D), dev(sc.scales), dev(sc.rotations),
                                 dev(np.random.default_rng(1).uniform(0.2, 0.9, (n, 3)).astype(f32)))
    with torch.no_grad():
        model._opacity.fill_(math.log(0.97 / 0.03))
    model.active_sh_degree = 2
    cams = [device_camera(c) for c in synthetic.room_cameras(6, 160, 120)]
    pipe = SimpleNamespace(depth_ratio=1.0, compute_cov3D_python=False, convert_SHs_python=False)
    ex = mesh_mod.GaussianExtractor(model, render, pipe)
    ex.reconstruction(cams)
    n_points = 9 * int(n * 0.1)
    cells = dev(tr.kuhn_lattice(int(round(n_points ** (1 / 3))) - 1)[1])
    kw = dict(downsample_ratio=0.1, cells=cells, to_host=False)
    return SimpleNamespace(ex=ex, cams=cams, kw=kw, gen=lambda: torch.Generator().manual_seed(9),
                           extent=mesh_mod.cameras_spatial_extent(cams))


def test_tetra_with_both_switches_spelled_off_equals_the_call_without_them(hip_lib, room):
    """The call at the parent's signature and the one that names both switches False give the same bytes.  (That the default
    path is the parent's is a property of the code -- the branch is not entered -- which no test of one tree can show.)"""
    plain = room.ex.extract_mesh_tetra(generator=room.gen(), **room.kw)
    spelled = room.ex.extract_mesh_tetra(generator=room.gen(), use_dilated_depth=False, use_sdf_tolerance=False, **room.kw)
    assert plain.triangles.size(0) > 100
    for a, b, name in zip(plain, spelled, ("vertices", "colours", "faces")):
        same_bits(a, b, name)


@pytest.mark.parametrize("switch", ["use_dilated_depth", "use_sdf_tolerance"])
def test_tetra_with_a_depth_switch_samples_the_adjusted_maps(hip_lib, room, switch):
    ex = room.ex
    plain = ex.extract_mesh_tetra(generator=room.gen(), texture_mesh=False, **room.kw)
    plain_sdf = ex.tetra[3].clone()
    mesh = ex.extract_mesh_tetra(generator=room.gen(), **{switch: True}, **room.kw)
    points, sdf = ex.tetra[0], ex.tetra[3]
    limit = 1e-3 * room.extent
    views = [(cam, d, None) for cam, d in zip(room.cams, ex.depthmaps)]
    if switch == "use_dilated_depth":
        views = [(cam, d, None) for cam, (d, _c) in zip(room.cams, mrn.dilated_depths(views, 1.5, limit))]
    else:
        views = [(cam, d - ((1.5 / ((fx + fy) / 2.0)) * d).clamp(max=limit), None)
                 for (cam, d, _c) in views
                 for fx, fy in [(160 / (2.0 * math.tan(cam.FoVx / 2.0)), 120 / (2.0 * math.tan(cam.FoVy / 2.0)))]]
    same_bits(sdf, mesh_mod.adaptive_tsdf(points, views, 5e-3 * room.extent), switch)
    assert not torch.equal(sdf, plain_sdf)  # the switch does something
    assert mesh.triangles.size(0) > 100 and mesh.vertex_colors.max() > 0.2 and plain.triangles.size(0) > 100


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_wrong_devices_dtypes_and_shapes_raise_before_any_launch(hip_lib):
    vertices, faces = mr.soup(0, 40, 0.5)
    colours = _colours(len(vertices))
    cam = (np.eye(4, dtype=f32), mr.pinhole(67, 45, 60.0, 60.0)[1])
    v, c, t = dev(vertices), dev(colours), dev(faces)
    with pytest.raises(RuntimeError, match="HIP device"):
        mrn.rasterize_mesh(mesh_mod.DeviceMesh(v.cpu(), c.cpu(), t.cpu()), cam, image_size=(45, 67))
    with pytest.raises(RuntimeError, match="float32"):
        mrn.rasterize_mesh(mesh_mod.DeviceMesh(v.double(), c, t), cam, image_size=(45, 67))
    with pytest.raises(RuntimeError, match="integer"):
        mrn.rasterize_mesh(mesh_mod.DeviceMesh(v, c, t.float()), cam, image_size=(45, 67))
    with pytest.raises(RuntimeError, match=r"\[n,3\]"):
        mrn.rasterize_mesh(mesh_mod.DeviceMesh(v.reshape(-1), c, t), cam, image_size=(45, 67))
    with pytest.raises(ValueError, match="image_size"):
        mrn.rasterize_mesh(mesh_mod.DeviceMesh(v, c, t), cam)
    with pytest.raises(RuntimeError, match="pixel_offset"):
        mrn.rasterize_mesh(mesh_mod.DeviceMesh(v, c, t), cam, image_size=(45, 67), pixel_offset=0.25)
    with pytest.raises(ValueError, match="2\\^31"):
        mrn.rasterize_mesh(mesh_mod.DeviceMesh(v, c, t), cam, image_size=(65536, 32768))
    with pytest.raises(ValueError, match="cameras"):
        mrn.visible_face_mask(mesh_mod.DeviceMesh(v, c, t), [cam, cam], [(45, 67)])
    depth = dev(_smooth())
    with pytest.raises(RuntimeError, match="HIP device"):
        mrn.dilated_depths([(_camera(), depth.cpu(), None)])
    with pytest.raises(RuntimeError, match="floating"):
        mrn.dilated_depths([(_camera(), depth.int(), None)])
    with pytest.raises(RuntimeError, match="shape"):
        mrn.dilated_depths([(_camera(), depth, dev(np.zeros((3, DH, DW + 1), f32)))])
    with pytest.raises(RuntimeError, match="every view or for none"):
        mrn.dilated_depths([(_camera(), depth, None), (_camera(), depth, dev(np.zeros((3, DH, DW), f32)))])
    lib = hip_lib  # overlapping maps are refused by the library: an output on an input, and two outputs on one another
    rgb = dev(np.zeros((3, DH, DW), f32))
    out_d, out_c = torch.empty_like(depth), torch.empty_like(rgb)
    pm = mrn.host_f32(_pm())
    sizes = mrn.host_array(mrn.ctypes.c_int, [DW, DH])
    ws = torch.empty(lib.g4s_depth_dilate_workspace(1, sizes), dtype=torch.uint8, device=DEV)
    for d_o, c_o in ((depth, out_c), (out_d, rgb), (out_d, rgb[1:]), (out_c[0], out_c)):
        rc = lib.g4s_depth_dilate(1, pm, sizes, mrn._lib.ptrs([depth]), mrn._lib.ptrs([rgb]), 1.5, 1e8, 1e-6, mrn._lib.ptrs([d_o]),
                                  mrn._lib.ptrs([c_o]), mrn._lib.ptr(ws), ws.numel(), None)
        assert rc == -1 and b"overlaps" in lib.g4s_last_error()
    with pytest.raises(RuntimeError, match="dilation_pixels"):
        mrn.dilated_depths([(_camera(), depth, None)], dilation_pixels=-1.0)
    with pytest.raises(RuntimeError, match=r"\(H,W\)"):
        mrn.get_dilated_depth(_camera(), dev(np.zeros((2, DH, DW), f32)), 1.5)
