"""View selection on the MI355X (g4splat_amd.view_selection, csrc/tsdf/view_select.hip) against the numpy restatement of the
contract (tests/view_selection_ref.py): words, counts, indices and float bits are compared exactly.  The restatement itself
is pinned to the reference's code in tests/test_view_selection_cpu.py.  The last tests run the reference-named entry points
on the golden scene against the reference's recorded results."""
import json
import math
import os
import random

import numpy as np
import pytest
import torch

import view_selection_ref as sr
from g4splat_amd import _lib, synthetic, view_selection as vs
from support import DEV, dev, same_bits

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P_EDGE = 4097
P_MAX = 64 * 129 + 1  # 130 words: a full chunk of the count kernel (OVERLAP_CHUNK = 128 words) and a second of two words


def _world(cam, c):
    """World points of camera-space points c [n,3] (double)."""
    M = np.asarray(cam.world_view_transform, np.float64)
    return (np.asarray(c, np.float64) - M[3, :3]) @ np.linalg.inv(M[:3, :3])


@pytest.fixture(scope="module")
def scene():
    """Seventy cameras of mixed sizes and 8 257 points whose every prefix holds edge cases: the first camera's centre
    (z = 0), a NaN point, points on u = 0, u = W, v = 0 and v = H of the first two cameras, points behind them, further
    camera centres; then a cloud in and about the scene, 4 097 points in all, and after them 4 160 more random points.
    The restatement's masks are computed once; a prefix of the points and of the cameras is a slice of them."""
    cams = sr.spiral_cameras(70, True)
    rng = np.random.default_rng(31)
    special = [np.asarray(cams[0].camera_center, np.float64), [np.nan, 0.1, 0.2]]
    for cam in cams[:2]:
        W, H = cam.image_width, cam.image_height
        fx, fy = W / (2.0 * math.tan(cam.FoVx / 2.0)), H / (2.0 * math.tan(cam.FoVy / 2.0))
        for z in (0.5, 2.0, 3.0):
            edge = [(-W / (2 * fx) * z, 0.1, z), (W / (2 * fx) * z, -0.1, z), (0.05, -H / (2 * fy) * z, z), (0.0, H / (2 * fy) * z, z),
                    (0.1, 0.1, -z), (0.0, 0.0, z)]
            special.extend(_world(cam, edge))
    special.extend(np.asarray(c.camera_center, np.float64) for c in cams[1:12])
    special.append([0.0, np.inf, 0.0])
    pts = rng.uniform(-4.0, 4.0, (P_EDGE, 3))
    s = rng.normal(size=(400, 3))
    pts[-400:] = s / np.linalg.norm(s, axis=1, keepdims=True) * rng.uniform(0.9, 1.1, (400, 1))
    pts[: len(special)] = np.asarray(special)
    assert len(special) < 63
    pts = np.concatenate([pts, rng.uniform(-4.0, 4.0, (P_MAX - P_EDGE, 3))]).astype(np.float32)
    masks = sr.visible_masks(pts, cams)
    assert 0.1 < masks.mean() < 0.6 and not masks[:, 1].any() and masks[:2, 2:38].any() and not masks[:2, 2:38].all()
    return cams, pts, masks


@pytest.mark.parametrize("C", [1, 2, 64, 65, 70])
@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 1023, 1025, 4097])
def test_bits_and_counts_equal_the_restatement(hip_lib, scene, P, C):
    """P covers word tails and workgroup tails (a workgroup owns 1 024 points), C the camera tiles of 16."""
    _check_table(scene, P, C)


def test_bits_and_counts_across_the_chunk_boundary_of_the_count_kernel(hip_lib, scene):
    """All 8 257 points: 130 words per camera, so the bits kernel's rows feed the count kernel a full chunk of 128 words
    and a second of two, over the three tile pairs of 70 cameras."""
    cams, _pts, masks = scene
    assert P_MAX == 8257 and (P_MAX + 63) // 64 == 128 + 2  # OVERLAP_CHUNK = 128
    _check_table(scene, P_MAX, 70)
    assert masks[:, 64 * 128:].any(1).sum() > 35  # the second chunk holds bits of most cameras


def _check_table(scene, P, C):
    cams, pts, masks = scene
    want = masks[:C, :P]
    table = vs.Covisibility(dev(pts[:P]), cams[:C])
    W = (P + 63) // 64
    assert table.words.dtype == torch.int64 and tuple(table.words.shape) == (C, W)
    words = table.words.cpu().numpy().view(np.uint64).reshape(C, W)
    assert np.array_equal(words, sr.words(want))
    if P % 64:
        assert (words[:, -1] >> np.uint64(P % 64) == 0).all()  # tail bits
    counts = table.counts
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (C, C)
    got = counts.cpu().numpy()
    assert np.array_equal(got, sr.counts(want)) and np.array_equal(got, got.T)
    assert np.array_equal(table.visible_counts.cpu().numpy(), want.sum(1))
    if P:
        c = C - 1
        assert np.array_equal(table.mask(c).cpu().numpy(), want[c])
        ratio = sr.ratio_of(got)
        assert table.ratio(0, c) == ratio(0, c)
    else:
        assert not got.any() and table.ratio(0, C - 1) == 0 and table.mask(0).shape == (0,)


# The count kernel on words it did not make.  Its grid is (tile pairs, per_pair) with per_pair = clamp(2048 / pairs, 1, chunks):
# OVERLAP_MAX_BLOCKS = 2048 workgroups for all pairs of tiles of CAM_TILE = 16 cameras, a chunk being OVERLAP_CHUNK = 128
# words; a workgroup walks chunks blockIdx.y, blockIdx.y + per_pair, ...  Whoever changes one of these moves the sizes below.
OVERLAP_CASES = [
    (17, 127),            # 3 pairs, one chunk, one word short
    (17, 128),            # one chunk exactly
    (17, 129),            # a second chunk of one word
    (70, 128 * 137 + 5),  # 15 pairs: per_pair = 136 < 138 chunks, workgroups 0 and 1 of a pair take two; the last has 5 words
    (1040, 257),          # 65 tiles, 2145 pairs > 2048: per_pair clamps to 1, a workgroup walks three chunks, the last of one word
]


@pytest.mark.parametrize("C,n_words", OVERLAP_CASES)
def test_counts_of_given_words_equal_the_matrix_product_of_their_bits(hip_lib, C, n_words):
    tiles = (C + 15) // 16
    pairs, chunks = tiles * (tiles + 1) // 2, (n_words + 127) // 128
    per_pair = min(max(2048 // pairs, 1), chunks)
    assert (pairs, per_pair, chunks, n_words - 128 * (chunks - 1)) == {
        (17, 127): (3, 1, 1, 127), (17, 128): (3, 1, 1, 128), (17, 129): (3, 2, 2, 1), (70, 17541): (15, 136, 138, 5),
        (1040, 257): (2145, 1, 3, 1)}[(C, n_words)]  # what the case is for
    words = sr.random_words(C, n_words, 7 * C + n_words)
    dev_words = dev(words.view(np.int64))
    counts = torch.empty((C, C), dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        _lib.call("g4s_view_overlap", C, n_words, _lib.ptr(dev_words), _lib.ptr(counts), None, 0, _lib.stream(DEV))
    got = counts.cpu().numpy()
    want = sr.bit_counts(words)
    assert np.array_equal(got, want) and np.array_equal(got, got.T)
    assert got[1, 1] == 64 * n_words and not got[2].any() and not got[:, 2].any()  # the row of ones, the empty row
    assert np.array_equal(got[1], np.diag(got)) and 1 <= got[C - 1, C - 1] <= 64 and got[1, C - 1] == got[C - 1, C - 1]
    assert np.array_equal(dev_words.cpu().numpy().view(np.uint64), words)  # the words are only read


def test_a_camera_that_sees_nothing(hip_lib, scene):
    cams, pts, masks = scene
    away = synthetic.look_at_camera((50.0, 0.0, 0.0), (100.0, 0.0, 0.0), (0.0, 0.0, 1.0), math.radians(55.0), 32, 24)
    table = vs.Covisibility(dev(pts), [cams[0], away, cams[1]])
    got = table.counts.cpu().numpy()
    assert not got[1].any() and not got[:, 1].any() and got[0, 2] == (masks[0] & masks[1]).sum() > 0
    assert table.ratio(0, 1) == 0 and table.ratio(1, 1) == 0 and not table.mask(1).any()
    assert table.ratio(0, 2) == sr.ratio_of(sr.counts(masks[:2]))(0, 1)


def test_reference_named_covisibility_helpers(hip_lib, scene):
    cams, pts, masks = scene
    dp = dev(pts)
    m = vs.get_visible_points_mask(cams[3], dp)
    assert m.dtype == torch.bool and np.array_equal(m.cpu().numpy(), masks[3])
    both = vs.get_covisible_points(cams[3], cams[4], dp)
    same_bits(both, pts[masks[3] & masks[4]])
    assert len(both) > 10
    ratio = sr.ratio_of(sr.counts(masks[3:5]))(0, 1)
    assert vs.covisibility_check_by_gs(cams[3], cams[4], dp) == ratio
    from types import SimpleNamespace
    assert vs.covisibility_check_by_gs(cams[3], cams[4], SimpleNamespace(get_xyz=dp)) == ratio


# ---- sampling ---------------------------------------------------------------------------------------------------------------
def _clouds(M, N, seed):
    rng = np.random.default_rng(seed)
    clouds = rng.normal(size=(M, N, 3)).astype(np.float32)
    if M > 1:
        clouds[1] = rng.uniform(-2e5, 2e5, (N, 3)).astype(np.float32)  # squared distances beyond the 1e10 cap
    return clouds


def _check_sampling(clouds, k, first):
    want_idx, want_pts, want_dist = sr.fps_batch(clouds, k, first)
    idx, pts, dist = vs.farthest_point_indices(dev(clouds), k, first, return_dist=True)
    M, N = clouds.shape[:2]
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (M, k) and tuple(pts.shape) == (M, k, 3) and tuple(dist.shape) == (M, N)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    same_bits(pts, want_pts)
    same_bits(dist, want_dist)
    return want_idx, want_dist


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("N,k", [(3, 2), (11, 10), (257, 10), (65537, 16)])
def test_sampling_equals_the_restatement(hip_lib, N, k, M):
    """N = 65 537: 65 workgroups per cloud fold into one slot; the other sizes are one workgroup.  The second cloud's
    coordinates reach 2e5, so the 1e10 cap binds there."""
    clouds = _clouds(M, N, 100 + N)
    first = [N - 1, 0, N // 2][:M]
    _check_sampling(clouds, k, first)
    if M > 1 and N > 3:  # round 1 of the second cloud: some squared distance to the first sample is cut to 1e10
        assert (((clouds[1] - clouds[1][first[1]]) ** 2).sum(1) > np.float32(1e10)).any()


def test_sampling_ties_go_to_the_smallest_index(hip_lib):
    lattice = sr.lattice(4)
    idx, _d = _check_sampling(np.stack([lattice, lattice[::-1].copy()]), 12, [21, 63])
    assert len(set(idx[0].tolist())) == 12
    same = np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (2, 11, 1))
    idx, dist = _check_sampling(same, 5, [7, 0])
    assert idx.tolist() == [[7, 0, 0, 0, 0], [0, 0, 0, 0, 0]] and not dist.any()  # all-zero distances select index 0


def test_sampling_past_the_grid_cap(hip_lib):
    """A round launches at most FPS_MAX_BLOCKS = 1024 workgroups of 256 * FPS_ITEMS = 1024 points per cloud, so a cloud
    of more than 1 048 576 points sends workgroups round their loop again: workgroup 0 for 1 024 more points, workgroup 1
    for one.  Cloud 0's farthest point lies in that second pass; cloud 1 has the same far point twice, once in each pass,
    and the smaller index has to win although the larger is folded later by the same thread."""
    one_pass = 1024 * 1024  # FPS_MAX_BLOCKS * 256 * FPS_ITEMS
    N = one_pass + 1025
    rng = np.random.default_rng(1049)
    clouds = rng.normal(size=(2, N, 3)).astype(np.float32)
    far, low, high = one_pass + 517, 608, one_pass + 608  # `low` and `high` belong to the same thread of workgroup 0
    clouds[0, far] = (50.0, -50.0, 50.0)
    clouds[1, low] = clouds[1, high] = (40.0, 40.0, -40.0)
    idx, dist = _check_sampling(clouds, 4, [N - 1, 0])
    assert idx[0, 1] == far and idx[1, 1] == low and high not in idx[1].tolist()
    assert dist[1, low] == 0 and dist[1, high] == 0 and (dist[:, one_pass:] > 0).sum() > 2000  # the tail's distances are written


def test_farthest_point_sample_keeps_the_reference_quirk_and_draws_on_the_device(hip_lib):
    small = dev(np.random.default_rng(1).normal(size=(10, 3)).astype(np.float32))
    assert vs.farthest_point_sample(small, 10) is small and vs.farthest_point_sample(small, 12) is small
    cloud = np.random.default_rng(2).normal(size=(300, 3)).astype(np.float32)
    got = vs.farthest_point_sample(dev(cloud), 7, first_index=299)
    same_bits(got, cloud[sr.fps(cloud, 7, 299)[0]])
    torch.manual_seed(3)
    first = int(torch.randint(0, 300, (1,), device=DEV))
    torch.manual_seed(3)
    got = vs.farthest_point_sample(dev(cloud), 7)
    same_bits(got, cloud[sr.fps(cloud, 7, first)[0]])


# ---- end to end on the golden scene ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLDEN, "view_selection.npz")))
    g["cams"] = [sr.camera(w, f[0], f[1], s[0], s[1]) for w, f, s in zip(g["wvt"], g["fov"], g["sizes"])]
    g["selection"] = json.loads(str(g["selection"]))
    return g


def test_select_need_inpaint_views_equals_the_reference(hip_lib, gold):
    pts = dev(gold["points"])
    for name, case in gold["selection"].items():
        random.seed(case["seed"])
        ids = vs.select_need_inpaint_views(gold["cams"], case["rates"], pts, case["select_num"], case["low"], case["high"],
                                           case["bound"])
        assert ids == case["ids"], name
        assert random.random() == case["next_random"], name


def test_get_novel_cams_lookat_points_equals_the_reference(hip_lib, gold, monkeypatch):
    clouds = dev(np.load(os.path.join(GOLDEN, "visibility_grid.npz"))["clouds"])
    train, novel = dev(gold["lookat_train"]), dev(gold["lookat_novel"])
    fps_num = int(gold["lookat_fps_num"])
    torch.manual_seed(9)
    a = vs.get_novel_cams_lookat_points(train, clouds, novel, fps_num)
    torch.manual_seed(9)
    b = vs.get_novel_cams_lookat_points(train, clouds, novel, fps_num)
    assert tuple(a.shape) == (len(gold["lookat_novel"]), 3) and torch.equal(a, b)
    # with the reference's recorded draws: the reference's points
    monkeypatch.setattr(vs, "draw_lookat_indices", lambda *args: (dev(gold["lookat_first"]), dev(gold["lookat_ids"])))
    got = vs.get_novel_cams_lookat_points(train, clouds, novel, fps_num)
    same_bits(got, gold["lookat"])


def test_outputs_are_bit_identical_from_run_to_run(hip_lib, scene):
    cams, pts, _masks = scene
    dp = dev(pts)
    clouds = dev(_clouds(3, 65537, 5))
    runs = []
    for _ in range(2):
        table = vs.Covisibility(dp, cams)
        runs.append((table.words.clone(), table.counts.clone()) + vs.farthest_point_indices(clouds, 16, [0, 1, 65536], return_dist=True))
    for x, y in zip(*runs):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
