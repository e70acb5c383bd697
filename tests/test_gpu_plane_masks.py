"""The plane-mask kernels on the GPU (g4splat_amd/plane_masks.py over csrc/tsdf/plane_masks.hip) against the numpy
restatement tests/plane_masks_ref.py, bit for bit, at the shapes where a kernel takes another trip or another branch; every
call is made twice and must give the same bits.  The restatement itself is held against sklearn, the reference's merge and
scipy.ndimage in tests/test_plane_masks_cpu.py."""
import numpy as np
import pytest
import torch

import plane_masks_ref as R
from g4splat_amd import plane_masks as pm
from plane_masks_ref import unit_normals
from support import PLANE_MASK_MAPS as MAPS, dev, host, load_plane_masks_golden, same_bits, twice

pytestmark = pytest.mark.gpu

SPAN = R.SPAN


@pytest.fixture(scope="module")
def golden():
    return load_plane_masks_golden()


def test_span_constant_is_the_kernels():
    assert pm.KMEANS_SPAN == SPAN and pm.MAX_K == 16


# ---- k-means -----------------------------------------------------------------------------------------------------------------
def check_kmeans(views, inits, **kw):
    got = twice(lambda: pm.kmeans_normals([dev(v) for v in views], [np.asarray(i) for i in inits], **kw))
    for v, (normals, init) in enumerate(zip(views, inits)):
        labels, centres, counts, n_iter = R.kmeans_normals(normals, init, **kw)
        assert got[3][v] == n_iter, (v, got[3][v], n_iter)
        assert host(got[0][v]).dtype == np.int8 and (host(got[0][v]) == labels).all(), v
        same_bits(got[1][v], centres, f"centres of view {v}")
        assert host(got[2][v]).tolist() == counts.tolist(), v
    return got


def test_kmeans_two_golden_views_of_different_sizes_in_one_call(golden):
    got = check_kmeans([golden[f"{n}_normals"] for n in MAPS], [golden[f"{n}_seeds"] for n in MAPS])
    assert got[3] == [int(golden[f"{n}_n_iter"]) for n in MAPS]  # sklearn's iteration counts
    single = pm.kmeans_normals(dev(golden["small_normals"]), golden["small_seeds"])
    assert (single[0] == got[0][0]).all() and (single[1] == got[1][0]).all() and single[3] == got[3][0]


@pytest.mark.parametrize("pixels", [SPAN - 1, SPAN, SPAN + 1, 65 * SPAN + 7], ids=lambda p: f"{p}px")
def test_kmeans_span_edges_and_more_than_64_spans(pixels):
    rng = np.random.default_rng(pixels)
    normals = unit_normals(rng, 1, pixels, 3)
    check_kmeans([normals], [normals[0, :3]], max_iter=3)


def test_kmeans_nan_pixel_empty_cluster_and_k16():
    rng = np.random.default_rng(7)
    a = unit_normals(rng, 45, 67)
    a[3, 5, 0] = a[44, 66, 2] = np.nan
    init_a = np.concatenate([a[0, :4], [[9.0, 9.0, 9.0]]]).astype(np.float32)  # the last cluster stays empty
    b = unit_normals(rng, 31, 140, 16, 0.05)
    got = check_kmeans([a], [init_a], max_iter=20)
    assert host(got[0][0])[3, 5] == -1 and host(got[2][0])[4] == 0 and (host(got[1][0])[4] == 9.0).all()
    check_kmeans([b], [b[0, :16]], max_iter=4)


def test_kmeans_stops_by_tolerance_by_stability_and_at_max_iter():
    rng = np.random.default_rng(11)
    normals = unit_normals(rng, 45, 67, 6, 0.3)
    init = normals[1, :6]
    by_tol = check_kmeans([normals], [init], tol=0.05)
    stable = check_kmeans([normals], [init], tol=0.0)
    assert by_tol[3][0] < stable[3][0]  # tol = 0 is reached only together with label stability, which is tested first
    once = check_kmeans([normals], [init], max_iter=1)
    assert once[3] == [1]
    mixed = check_kmeans([normals, normals[:20], normals], [init, init, init], tol=0.0, max_iter=stable[3][0] - 1)
    assert mixed[3][0] == stable[3][0] - 1  # cut off at max_iter while another view of the call may have stopped


def test_kmeanspp_init_runs_and_repeats(golden):
    normals = dev(golden["small_normals"])
    a = pm.kmeans_normals(normals, "k-means++", k=8, generator=torch.Generator().manual_seed(3))
    b = pm.kmeans_normals(normals, "k-means++", k=8, generator=torch.Generator().manual_seed(3))
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and int(a[2].sum()) == normals.shape[0] * normals.shape[1]
    seeds = pm.kmeanspp_seeds(normals, 8, torch.Generator().manual_seed(3))
    want = R.kmeans_normals(golden["small_normals"], seeds)
    assert (host(a[0]) == want[0]).all() and a[3] == want[3]


# ---- opening and components ------------------------------------------------------------------------------------------------------
def check_components(label_maps, luts, min_sizes, do_open=True):
    got = twice(lambda: pm.normal_components([dev(l, torch.int8) for l in label_maps], luts, min_sizes, open=do_open,
                                             return_opened=True))
    for v, labels in enumerate(label_maps):
        lut = np.asarray(luts[v])
        rank = np.where((labels >= 0) & (labels < len(lut)), lut[np.clip(labels, 0, len(lut) - 1)], -1).astype(np.int8)
        opened = R.open_ranks(rank) if do_open else rank
        comps, sizes, n = R.components(opened, min_sizes[v])
        assert (host(got[3][v]) == opened).all(), v
        assert got[2][v] == n, (v, got[2][v], n)
        assert (host(got[0][v]) == comps).all(), v
        assert host(got[1][v]).tolist() == sizes.tolist(), v
    return got


def blocks_image(H, W, side):
    """Blocks of side x side at every corner, at the middle of every edge and in the middle, rank 0 on -1."""
    img = np.full((H, W), -1, np.int8)
    for y in (0, (H - side) // 2, H - side):
        for x in (0, (W - side) // 2, W - side):
            img[y:y + side, x:x + side] = 0
    return img


def test_open_thin_images_and_tile_edges_in_one_call():
    rng = np.random.default_rng(5)
    shapes = [(5, 40), (40, 5), (9, 9), (67, 45), (45, 67), (8, 33), (1, 1), (16, 64)]
    maps = []
    for H, W in shapes:
        img = (rng.random((H, W)) < 0.97).astype(np.int8) - 1  # mostly label 0, holes of -1
        img[rng.random((H, W)) < 0.3 * (rng.random() < 0.5)] = 1
        maps.append(img)
    maps.append(np.zeros((9, 9), np.int8))
    maps.append(np.zeros((5, 40), np.int8))
    check_components(maps, [[0, 1]] * len(maps), [1] * len(maps))


def test_open_blocks_of_8_and_9_at_every_corner_and_edge():
    eight, nine = blocks_image(45, 67, 8), blocks_image(45, 67, 9)
    got = check_components([eight, nine], [[0], [0]], [1, 1])
    opened8, opened9 = host(got[3][0]), host(got[3][1])
    assert (opened9 == nine).all() and got[2][1] == 9
    # an 8 x 8 block vanishes in the open image and along an edge; in a corner the border completes its window
    assert got[2][0] == 4 and (opened8[18:26, 29:37] == -1).all() and (opened8[:8, :8] == 0).all() and (opened8[:8, 29:37] == -1).all()


def test_open_two_ranks_in_stripes():
    H, W = 45, 67
    wide = (np.arange(W)[None, :] // 9 % 2 + np.zeros((H, 1))).astype(np.int8)     # stripes of 9: every one survives
    narrow = (np.arange(W)[None, :] // 8 % 2 + np.zeros((H, 1))).astype(np.int8)  # stripes of 8: only at the border
    rows = (np.arange(H)[:, None] // 10 % 3 + np.zeros((1, W))).astype(np.int8)
    got = check_components([wide, narrow, rows], [[0, 1], [1, 0], [2, 0, 1]], [1, 1, 1])
    assert (host(got[3][0])[:, :63] == wide[:, :63]).all() and (host(got[3][0])[:, 63:] == -1).all()  # the last stripe is 4 wide


def snake(H, W):
    img = np.full((H, W), -1, np.int8)
    img[0::2] = 0
    img[1::4, W - 1] = 0
    img[3::4, 0] = 0
    return img


def test_components_long_chains_diagonals_and_ranks_that_touch():
    H, W = 45, 67
    diag = np.full((H, W), -1, np.int8)
    diag[np.arange(H), np.arange(H)] = 0           # joined by corners only
    diag[np.arange(H), np.arange(H) + 10] = 0      # a second diagonal, ten pixels away
    touch = np.full((H, W), -1, np.int8)
    touch[:, :30], touch[:, 30:] = 0, 1
    touch[10, 29], touch[11, 30] = 1, 0            # each rank reaches into the other by a corner
    got = check_components([snake(H, W), diag, touch], [[0], [0], [0, 1]], [1, 1, 1], do_open=False)
    assert got[2] == [1, 2, 2] and host(got[1][0]).tolist() == [23 * W + 22]


def test_components_more_than_64_and_the_size_bar():
    H, W = 45, 67
    dots = np.full((H, W), -1, np.int8)
    dots[0::2, 0::2] = np.arange(34)[None, :] % 3  # 23 x 34 single pixels of three ranks
    bars = np.full((H, W), -1, np.int8)
    for i, length in enumerate((6, 7, 8, 7, 6)):
        bars[4 * i, 2:2 + length] = i % 2
    got = check_components([dots, bars, bars, bars], [[2, 0, 1], [0, 1], [0, 1], [1, 0]], [1, 7, 8, 7], do_open=False)
    assert got[2] == [23 * 34, 3, 1, 3]
    assert host(got[1][1]).tolist() == [8, 7, 7]  # of rank 0's bars of 6, 8, 6 only the 8 stays; then rank 1's two of 7


# ---- the join ----------------------------------------------------------------------------------------------------------------------
def check_join(views, max_planes=100):
    """views: (normals, masks [M,H,W] array, components, n, bar)."""
    got = twice(lambda: pm.join_planes([dev(v[0]) for v in views], [dev(v[1]) for v in views],
                                       [dev(v[2], torch.int32) for v in views], [v[3] for v in views], [v[4] for v in views],
                                       max_planes))
    for v, (normals, masks, comps, n, bar) in enumerate(views):
        seg, normal, areas, count = R.excavate_planes(normals, masks, comps, n, bar, max_planes)
        assert host(got[v].seg_mask).dtype == np.int32 and (host(got[v].seg_mask) == seg).all(), v
        if areas is None:
            assert got[v].normal is None and got[v].areas is None, v
        else:
            assert got[v].areas.tolist() == areas.tolist(), v
            same_bits(got[v].normal, normal, f"normals of view {v}")
    return got


def random_masks(rng, M, H, W, dtype=bool):
    masks = np.zeros((M, H, W), dtype)
    for m in range(M):
        y, x = rng.integers(0, H - 4), rng.integers(0, W - 4)
        masks[m, y:y + rng.integers(3, H), x:x + rng.integers(3, W)] = 1
    return masks


def halves(H, W):
    comps = np.zeros((H, W), np.int32)
    comps[:, W // 2:] = 1
    comps[:3] = -1
    return comps


@pytest.mark.parametrize("M", [0, 1, 33, 256])
def test_join_mask_counts(M):
    rng = np.random.default_rng(M)
    H, W = 45, 67
    normals = unit_normals(rng, H, W)
    normals[7, 7, 1] = np.nan
    masks = random_masks(rng, M, H, W)
    if M:
        masks[:, 20, 40] = True  # a pixel covered by all masks
        masks[0] = True
    small = random_masks(rng, M, 9, 300, np.uint8) * 3  # uint8 masks, any non-zero value, another size in the same call
    views = [(normals, masks, halves(H, W), 2, 40), (unit_normals(rng, 9, 300), small, halves(9, 300), 2, 12.5)]
    got = check_join(views, max_planes=1000)  # the mask of everything is painted last: its ids are the highest
    assert (got[0].areas is None) == (M == 0)
    check_join(views)  # with the reference's 100, 256 masks leave only what the first hundred ids still cover


def test_join_component_counts_and_ids_beyond_255():
    rng = np.random.default_rng(9)
    H, W = 45, 67
    normals = unit_normals(rng, H, W)
    cells = (np.arange(H)[:, None] // 3) * 23 + np.arange(W)[None, :] // 3  # 15 x 23 cells of 3 x 3 (the last column 3 x 1)
    cells = cells.astype(np.int32)
    n = int(cells.max()) + 1
    all_on = np.ones((2, H, W), bool)
    all_on[1, :, 60:] = False  # the smaller mask is painted first and then covered
    none = np.full((H, W), -1, np.int32)
    one = np.zeros((H, W), np.int32)
    got = check_join([(normals, all_on, cells, n, 9), (normals, all_on, none, 0, 9), (normals, all_on, one, 1, 9)],
                     max_planes=1000)
    assert n > 64 and len(got[0].areas) == 15 * 22 and int(host(got[0].seg_mask).max()) == 330 > 255
    assert got[1].areas is None and got[2].areas.tolist() == [H * W]
    capped = check_join([(normals, all_on, cells, n, 9)], max_planes=300)
    # ids 1 .. 300 are the smaller mask's pairs, all painted over by the larger mask: nothing is left below the cap
    assert capped[0].areas is None and not host(capped[0].seg_mask).any()


# ---- the whole stage from the recorded seeds -----------------------------------------------------------------------------------------
def test_golden_normals_cluster_and_excavate_planes(golden):
    rng = np.random.default_rng(2)
    views = [golden[f"{n}_normals"] for n in MAPS]
    seeds = [golden[f"{n}_seeds"] for n in MAPS]
    masks = [random_masks(rng, 12, *v.shape[:2]) for v in views]
    ratio = 0.004
    want = []
    for normals, init, m in zip(views, seeds, masks):
        labels, centres, counts, _ = R.kmeans_normals(normals, init)
        lut = R.select_normal_clusters(counts, centres, 6)
        comps, sizes, n = R.normal_components(labels, lut, normals.shape[0] * normals.shape[1] * ratio)
        want.append((comps, n, R.excavate_planes(normals, m, comps, n, normals.shape[0] * normals.shape[1] * ratio)))
    assert all(w[1] > 0 for w in want) and all(w[2][2] is not None for w in want)
    normal_masks = pm.normals_cluster([dev(v) for v in views], None, 8, 6, ratio, init=seeds)
    for v, (comps, n, _j) in enumerate(want):
        assert len(normal_masks[v]) == n
        for i, mask in enumerate(normal_masks[v]):
            assert mask.dtype == torch.bool and (host(mask) == (comps == i)).all()
    flat = pm.normals_cluster(dev(views[0]).reshape(-1, 3), views[0].shape[:2], init=seeds[0])
    assert len(flat) == want[0][1] and all((a == b).all() for a, b in zip(flat, normal_masks[0]))
    got = twice(lambda: pm.excavate_planes([dev(v) for v in views], [dev(m) for m in masks], min_size_ratio=ratio, init=seeds))
    for v, (_c, _n, (seg, normal, areas, _count)) in enumerate(want):
        seg_mask, got_normal, got_areas = got[v]
        assert (host(seg_mask) == seg).all() and got_areas.tolist() == areas.tolist()
        same_bits(got_normal, normal, f"normals of view {v}")
    one = pm.excavate_planes(dev(views[0]), dev(masks[0]), min_size_ratio=ratio, init=seeds[0])
    assert (one.seg_mask == got[0].seg_mask).all()
