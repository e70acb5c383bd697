"""The plane-mask stage without a GPU: the numpy restatement (tests/plane_masks_ref.py) against sklearn's recorded k-means and
the reference's recorded cluster merges (tests/golden/plane_masks.npz), against scipy.ndimage for the opening and the
components, hand-worked joins, and the wrappers' refusals, which come before any library call."""

import numpy as np
import pytest
import torch

import plane_masks_ref as R
from g4splat_amd import plane_masks as pm
from support import PLANE_MASK_MAPS as MAPS, load_plane_masks_golden


@pytest.fixture(scope="module")
def golden():
    return load_plane_masks_golden()


@pytest.fixture(scope="module")
def restated(golden):
    """The restatement's k-means from the recorded seeds, computed once."""
    return {name: R.kmeans_normals(golden[f"{name}_normals"], golden[f"{name}_seeds"]) for name in MAPS}


# ---- k-means against sklearn ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MAPS)
def test_restated_kmeans_matches_sklearn(golden, restated, name):
    """The same iteration count, centres within 1e-5, and the same labels except where the two smallest distances are
    within 1e-5 relative (at most 0.1 % of the pixels)."""
    labels, centres, counts, n_iter = restated[name]
    assert n_iter == int(golden[f"{name}_n_iter"])
    assert np.abs(centres.astype(np.float64) - golden[f"{name}_centres"]).max() <= 1e-5
    want = golden[f"{name}_labels"]
    differ = labels != want
    print(name, "differing labels", int(differ.sum()), "of", differ.size)
    d = np.sort(R.distances(golden[f"{name}_normals"].reshape(-1, 3), centres).astype(np.float64), axis=1)
    near_tie = ((d[:, 1] - d[:, 0]) < 1e-5 * d[:, 1]).reshape(differ.shape)
    assert not (differ & ~near_tie).any()
    assert differ.sum() <= 0.001 * differ.size
    assert counts.tolist() == np.bincount(labels.reshape(-1), minlength=8).tolist()


def test_fixed_sum_is_a_sum_and_depends_on_nothing_but_the_order():
    rng = np.random.default_rng(0)
    for n in (1, 255, 4096, 4097, 70 * 4096 + 3):
        v = rng.normal(size=(n, 2))
        s = R.fixed_sum(v)
        assert np.allclose(s, v.sum(axis=0), rtol=0, atol=1e-9 * n)
        assert (R.fixed_sum(v) == s).all()


def test_kmeans_nan_pixels_empty_clusters_and_max_iter():
    rng = np.random.default_rng(1)
    normals = rng.normal(size=(9, 11, 3)).astype(np.float32)
    normals[2, 3, 1] = np.nan
    init = np.concatenate([normals[0, :3], [[50.0, 50.0, 50.0]]]).astype(np.float32)  # the last centre attracts nobody
    labels, centres, counts, n_iter = R.kmeans_normals(normals, init, max_iter=1)
    assert n_iter == 1 and labels[2, 3] == -1 and counts[3] == 0 and (centres[3] == 50.0).all()
    assert counts.sum() == 9 * 11 - 1
    assert (labels == R.assign(normals.reshape(-1, 3), centres, R.valid_pixels(normals.reshape(-1, 3))).reshape(9, 11)).all()


# ---- the pick and merge against the reference's recorded results ------------------------------------------------------------
def test_merge_cases_equal_the_reference(golden):
    names = [str(n) for n in golden["merge_cases"]]
    assert names == ["no_merge", "one_merge", "chain", "admits_seventh"]
    for n in names:
        counts, topk, centres, want = (golden[f"merge_{n}_{k}"] for k in ("counts", "topk", "centres", "lut"))
        assert pm.merge_normal_clusters(counts, topk, centres).tolist() == want.tolist(), n
        assert R.merge_normal_clusters(counts, topk, centres).tolist() == want.tolist(), n
        if n != "admits_seventh":  # there the recorded first pick holds the larger of three tied labels
            assert pm.select_normal_clusters(counts, centres, 6).tolist() == want.tolist(), n
    seventh = golden["merge_admits_seventh_lut"]
    assert seventh[4] >= 0 and 4 not in golden["merge_admits_seventh_topk"]


def test_select_ranks_ties_by_label_and_takes_fewer_than_k():
    centres = np.eye(3)
    assert pm.select_normal_clusters([5, 7, 5], centres, 2).tolist() == [1, 0, -1]
    assert pm.select_normal_clusters([5, 7, 5], centres, 6).tolist() == [1, 0, 2]
    assert pm.select_normal_clusters([3, 0, 9], np.array([[1, 0, 0], [0, 0, 0], [0.99, 0.1, 0]]), 2).tolist() == [0, -1, 0]


# ---- opening and components against scipy -----------------------------------------------------------------------------------
def _scipy_open(mask):
    ndi = pytest.importorskip("scipy.ndimage")
    box = np.ones((9, 9), bool)
    return ndi.binary_dilation(ndi.binary_erosion(mask, box, border_value=1), box)


def _blobs(rng, H, W, n_ranks, fill):
    """A rank image of blocks of random ranks over a background of -1, with salt noise."""
    rank = np.full((H, W), -1, np.int8)
    for _ in range(fill):
        y, x = rng.integers(0, H), rng.integers(0, W)
        h, w = rng.integers(1, 16, 2)
        rank[y:y + h, x:x + w] = rng.integers(0, n_ranks)
    rank[rng.random((H, W)) < 0.02] = -1
    return rank


@pytest.mark.parametrize("shape", [(45, 67), (5, 40), (40, 5), (9, 9), (8, 30), (3, 3), (1, 1)])
def test_opening_and_components_equal_scipy(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    for trial in range(4):
        rank = _blobs(rng, *shape, 3, 12) if trial else np.zeros(shape, np.int8)
        opened = R.open_ranks(rank)
        for r in range(3):
            assert ((opened == r) == _scipy_open(rank == r)).all(), (shape, trial, r)
        for min_size in (1, 30):
            comps, sizes, n = R.components(opened, min_size)
            want, k = np.full(shape, -1, np.int32), 0
            for r in range(3):
                lab, m = ndi.label(opened == r, structure=np.ones((3, 3)))
                for i in range(1, m + 1):
                    if (lab == i).sum() >= min_size:
                        want[lab == i] = k
                        assert sizes[k] == (lab == i).sum()
                        k += 1
            assert n == k and (comps == want).all(), (shape, trial, min_size)


# ---- hand-worked joins -------------------------------------------------------------------------------------------------------
def _host_join(normals, masks, comps, n, bar, max_planes=100):
    """The module's host functions around numpy counts and the paint rule of the contract: the last qualifying mask wins."""
    H, W = comps.shape
    masks = np.asarray(masks).reshape(-1, H, W) != 0
    order = np.argsort(masks.reshape(len(masks), H * W).sum(axis=1), kind="stable")
    C = np.array([[(m & (comps == c)).sum() for c in range(n)] for m in masks]).reshape(len(masks), n)
    ids, count = pm.assign_pair_ids(C, order, bar)
    seg = np.zeros((H, W), np.int32)
    for y in range(H):
        for x in range(W):
            c = comps[y, x]
            for m in order[::-1]:
                if c >= 0 and ids[m, c] and masks[m, y, x]:
                    seg[y, x] = ids[m, c]
                    break
    relabel, areas = pm.renumber_planes(np.bincount(seg.reshape(-1), minlength=count + 1), count, max_planes, bar)
    seg = relabel[seg]
    if not len(areas):
        return seg, None, None
    sums = np.array([R.fixed32(normals[seg == i + 1]).sum(axis=0) for i in range(len(areas))])
    return seg, pm.mean_normals(sums, areas), areas


def _case(masks, comps, n, bar, max_planes=100, seed=0):
    H, W = comps.shape
    normals = np.random.default_rng(seed).normal(size=(H, W, 3))
    normals = (normals / np.linalg.norm(normals, axis=2, keepdims=True)).astype(np.float32)  # inside the clamp of +-2
    seg, normal, areas, _count = R.excavate_planes(normals, masks, comps, n, bar, max_planes)
    seg2, normal2, areas2 = _host_join(normals, masks, comps, n, bar, max_planes)
    assert (seg == seg2).all()
    if areas is None:
        assert areas2 is None and normal2 is None
    else:
        assert areas.tolist() == areas2.tolist() and (normal == normal2).all()
        for i, a in enumerate(areas):
            want = normals[seg == i + 1].astype(np.float64).mean(axis=0)
            assert np.allclose(normal[i], want / np.linalg.norm(want), atol=1e-8)
    return seg, areas


def _rect(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), bool)
    m[y0:y1, x0:x1] = True
    return m


def test_join_nested_masks_and_an_id_that_is_painted_over():
    H, W = 6, 8
    comps = np.zeros((H, W), np.int32)
    big, small = _rect(H, W, 0, 6, 0, 6), _rect(H, W, 1, 3, 1, 3)
    seg, areas = _case([big, small], comps, 1, 3)  # the small mask is painted first (id 1), the big one over all of it
    assert areas.tolist() == [36] and (seg == big).all()


def test_join_equal_areas_keep_their_order():
    H, W = 6, 8
    comps = np.zeros((H, W), np.int32)
    x, y = _rect(H, W, 0, 2, 0, 4), _rect(H, W, 0, 2, 2, 6)
    seg, areas = _case([x, y], comps, 1, 4)
    assert areas.tolist() == [4, 8] and (seg[0, :6] == [1, 1, 2, 2, 2, 2]).all()
    seg, areas = _case([y, x], comps, 1, 4)
    assert areas.tolist() == [4, 8] and (seg[0, :6] == [2, 2, 2, 2, 1, 1]).all()


def test_join_pair_at_and_below_the_bar():
    H, W = 6, 8
    comps = np.repeat(np.array([[0, 0, 0, 0, 1, 1, 1, 1]], np.int32), H, axis=0)
    mask = _rect(H, W, 0, 1, 1, 8)  # 3 pixels of component 0, 4 of component 1
    seg, areas = _case([mask], comps, 2, 4)
    assert areas.tolist() == [4] and (seg[0] == [0, 0, 0, 0, 1, 1, 1, 1]).all()
    seg, areas = _case([mask], comps, 2, 3)
    assert areas.tolist() == [3, 4] and (seg[0] == [0, 1, 1, 1, 2, 2, 2, 2]).all()
    seg, areas = _case([mask], comps, 2, 4.5)
    assert areas is None and not seg.any()
    seg, areas = _case([mask], comps, 2, 3.5)  # the reference's bar is a float
    assert areas.tolist() == [4]


def test_join_more_ids_than_max_planes_and_no_masks():
    H, W = 6, 8
    comps = np.zeros((H, W), np.int32)
    masks = [_rect(H, W, 0, 1, 0, 8), _rect(H, W, 1, 3, 0, 8), _rect(H, W, 3, 6, 0, 8)]
    seg, areas = _case(masks, comps, 1, 2, max_planes=2)
    assert areas.tolist() == [8, 16] and not seg[3:].any() and (seg[0] == 1).all() and (seg[1:3] == 2).all()
    seg, areas = _case(np.zeros((0, H, W), bool), comps, 1, 2)
    assert areas is None
    seg, areas = _case(masks, np.full((H, W), -1, np.int32), 0, 2)
    assert areas is None


def test_fixed_point_of_a_normal_component():
    f = R.fixed32(np.array([0.5, -1.0, np.nan, 3.0, -7.0, 2.0 ** -33, 3 * 2.0 ** -33], np.float32))
    assert f.tolist() == [2 ** 31, -2 ** 32, 0, 2 ** 33, -2 ** 33, 0, 2]  # halves round to even


def test_plane_mask_files(tmp_path):
    seg = torch.arange(12, dtype=torch.int32).reshape(3, 4) * 100
    pm.save_plane_mask(tmp_path / "plane_mask_frame000000.npy", seg)
    back = pm.load_plane_mask(tmp_path / "plane_mask_frame000000.npy")
    assert back.dtype == torch.int32 and (back == seg).all()
    np.save(tmp_path / "u8.npy", np.arange(6, dtype=np.uint8).reshape(2, 3))
    assert pm.load_plane_mask(tmp_path / "u8.npy").dtype == torch.int32


def test_kmeanspp_seeds_are_valid_normals_and_repeat():
    rng = np.random.default_rng(3)
    normals = rng.normal(size=(80, 90, 3)).astype(np.float32)
    normals[::7, ::5] = np.nan
    a = pm.kmeanspp_seeds(torch.from_numpy(normals), 8, torch.Generator().manual_seed(5))
    b = pm.kmeanspp_seeds(torch.from_numpy(normals), 8, torch.Generator().manual_seed(5))
    assert a.shape == (8, 3) and a.dtype == np.float32 and (a == b).all() and np.isfinite(a).all()
    flat = normals.reshape(-1, 3)
    assert all((flat == s).all(axis=1).any() for s in a)
    assert len(np.unique(a, axis=0)) == 8


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_before_any_library_call(monkeypatch):
    from g4splat_amd import _lib

    def no_library(*a, **k):
        raise AssertionError("a refusal must come before the library is loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "call", no_library)
    normals = torch.zeros((4, 5, 3))
    masks = torch.zeros((2, 4, 5), dtype=torch.bool)
    with pytest.raises(ValueError, match="k must be in 1 .. 16"):
        pm.kmeans_normals(normals, np.zeros((17, 3)))
    with pytest.raises(ValueError, match="k must be in 1 .. 16"):
        pm.excavate_planes(normals, masks, n_init_normal_clusters=17)
    with pytest.raises(ValueError, match="torch.float32"):
        pm.kmeans_normals(normals.double(), np.zeros((8, 3)))
    with pytest.raises(ValueError, match="HIP device"):  # a CPU tensor
        pm.kmeans_normals(normals, np.zeros((8, 3)))
    with pytest.raises(ValueError, match="torch.float32"):
        pm.excavate_planes(normals.double(), masks)
    with pytest.raises(ValueError, match="HIP device"):
        pm.excavate_planes(normals, masks)
    with pytest.raises(ValueError, match="2 views but 1 sam_masks"):
        pm.excavate_planes([normals, normals], [masks])
    with pytest.raises(ValueError, match="2 views but 3 init"):
        pm.kmeans_normals([normals, normals], np.zeros((3, 8, 3)))
    with pytest.raises(ValueError, match="torch.int8"):
        pm.normal_components(torch.zeros((4, 5), dtype=torch.int32), [0], 1)
    with pytest.raises(ValueError, match="2 views but 1 lut"):
        pm.normal_components([torch.zeros((4, 5), dtype=torch.int8)] * 2, [[0]], 1)
    with pytest.raises(ValueError, match="max_iter"):
        pm.kmeans_normals(normals, np.zeros((8, 3)), max_iter=0)


def test_library_refuses_bad_arguments_on_the_host(hip_lib):
    """Every entry point of the unit checks its arguments before it touches the device (no GPU is needed to see that)."""
    import ctypes
    lib = hip_lib
    one, big = ctypes.c_void_p(256), 1 << 20  # never dereferenced: validation fails first
    ptrs = (ctypes.c_void_p * 1)(256)
    sizes = (ctypes.c_int * 2)(4, 3)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    init = (ctypes.c_float * 51)()
    n_iter = ints(0)

    def expect(rc, text):
        assert rc == -1, rc
        assert text.encode() in lib.g4s_last_error(), lib.g4s_last_error()

    expect(lib.g4s_kmeans_normals(1, sizes, ptrs, 17, init, 300, 1e-4, ptrs, one, one, n_iter, one, big, None), "k must be in 1 .. 16")
    expect(lib.g4s_kmeans_normals(1, sizes, ptrs, 8, init, 0, 1e-4, ptrs, one, one, n_iter, one, big, None), "max_iter must be")
    expect(lib.g4s_kmeans_normals(1, sizes, ptrs, 8, init, 3, -1.0, ptrs, one, one, n_iter, one, big, None), "tol must not be")
    expect(lib.g4s_kmeans_normals(1, sizes, ptrs, 8, init, 3, 1e-4, ptrs, one, one, n_iter, one, 8, None), "workspace too small")
    expect(lib.g4s_kmeans_normals(1, ints(0, 3), ptrs, 8, init, 3, 1e-4, ptrs, one, one, n_iter, one, big, None), "must be positive")
    assert lib.g4s_kmeans_normals_workspace(-1, sizes) == 0 and lib.g4s_kmeans_normals_workspace(1, sizes) >= 64 * 8
    lut = ints(*([0] * 15 + [16]))
    expect(lib.g4s_normal_components_count(1, sizes, ptrs, lut, 1, ints(1), None, ptrs, n_iter, one, big, None), "a rank must be in")
    expect(lib.g4s_normal_components_count(1, sizes, ptrs, ints(*[0] * 16), 1, ints(0), None, ptrs, n_iter, one, big, None),
           "min_size[0] must be at least 1")
    expect(lib.g4s_normal_components_count(1, sizes, ptrs, ints(*[0] * 16), 1, ints(1), None, ptrs, n_iter, one, 8, None),
           "workspace too small")
    expect(lib.g4s_normal_components_sizes(1, sizes, ints(13), ptrs, one, big, None), "n[0] must be the count")
    assert lib.g4s_normal_components_workspace(1, sizes) >= 12 * 25 and lib.g4s_normal_components_workspace(70000, sizes) == 0
    expect(lib.g4s_plane_pair_counts(1, sizes, ptrs, ptrs, ints(-1), ints(1), one, one, one, big, None), "n_masks[0] must not be negative")
    expect(lib.g4s_plane_paint(1, sizes, ptrs, ptrs, ints(2), ints(1), ints(0, 0), ints(0, 0), ints(0), ptrs, one, one, big, None),
           "not a permutation")
    expect(lib.g4s_plane_paint(1, sizes, ptrs, ptrs, ints(2), ints(1), ints(1, 0), ints(0, 2), ints(1), ptrs, one, one, big, None),
           "an id must be in 0 .. n_ids")
    expect(lib.g4s_plane_relabel(1, sizes, ptrs, ptrs, ints(0), ints(1), ints(1), one, one, big, None), "0 stays 0")
    assert lib.g4s_plane_paint_workspace(1, -1, 0) == 0 and lib.g4s_plane_relabel_workspace(1, -1) == 0
    assert lib.g4s_plane_pair_counts(0, None, None, None, None, None, None, None, None, 0, None) == 0
