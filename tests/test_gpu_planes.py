"""Global planes on the MI355X (g4splat_amd.planes, csrc/tsdf/planes.hip) against the numpy restatement of the contract
(tests/planes_ref.py): labels, counts, membership words, dicts and indices are compared exactly.  The restatement itself is
pinned to the reference's code in tests/test_planes_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import planes_ref as pr
from g4splat_amd import planes
from support import DEV, dev, load_planes_golden, pinhole_camera, same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return load_planes_golden()


@pytest.fixture(scope="module")
def golden_labels(hip_lib, golden):
    """The library's labels of the golden scene (one launch over the five views) and the restatement's, computed once."""
    got = planes.front_point_labels(golden.cams, dev(golden.points), [dev(m) for m in golden.masks], golden.depth_thresh)
    want = np.stack([pr.front_labels(golden.points, c, m, golden.depth_thresh) for c, m in zip(golden.cams, golden.masks)])
    return got, want


# ---- labels ------------------------------------------------------------------------------------------------------------------
def test_labels_of_the_golden_scene(golden, golden_labels):
    got, want = golden_labels
    assert got.dtype == torch.int32 and tuple(got.shape) == want.shape
    got = got.cpu().numpy()
    for v in range(len(golden.cams)):
        assert np.array_equal(got[v], want[v]), v
        assert (got[v] != 0).sum() > 500
    # every view in a launch of its own gives the same rows (the chunked path of a long view list)
    for v in (0, 3):
        one = planes.front_point_labels(golden.cams[v:v + 1], dev(golden.points), [dev(golden.masks[v])], golden.depth_thresh)
        assert np.array_equal(one.cpu().numpy()[0], want[v])
    ids = planes.plane_point_indices(golden_labels[0][1], int(want[1].max()))
    assert ids.dtype == torch.int64 and np.array_equal(ids.cpu().numpy(), np.nonzero(want[1] == want[1].max())[0])
    assert planes.plane_point_indices(golden_labels[0][1], 0).numel() == 0


EW, EH, EF, ETHRESH = 16, 8, 8.0, 0.25


def _edge_cloud():
    """(points [4099,3] float32, {name: index}) for an identity camera with W = 16, H = 8, fx = fy = 8: u = 8 x / z + 8 and
    v = 8 y / z + 4 are exact for the dyadic coordinates used."""
    specs, names = [], {}

    def add(name, u, v, z):
        names.setdefault(name, len(specs))
        specs.append(((u - EW / 2) / EF * z, (v - EH / 2) / EF * z, z))

    add("point0", 8, 4, 0.5)  # the nearest point of pixel (8, 4): not labelled, does not set zmin
    add("front", 8, 4, 1.0)
    add("equal_z", 8, 4, 1.0)
    add("inside", 8, 4, 1.125)
    add("at_threshold", 8, 4, 1.25)  # zmin + depth_thresh exactly: rejected
    add("behind", 8, 4, 3.0)
    add("half_even", 2.5, 4, 1.0)  # -> column 2
    add("half_odd", 3.5, 4, 1.0)  # -> column 4
    add("half_v_even", 5, 0.5, 1.0)  # -> row 0
    add("half_v_odd", 5, 1.5, 1.0)  # -> row 2
    add("clamp_u", 15.5, 4, 1.0)  # rint = 16 -> column 15
    add("clamp_u2", 15.75, 2, 1.0)
    add("clamp_v", 6, 7.5, 1.0)  # rint = 8 -> row 7
    names["below_zero"] = len(specs)
    specs.append((float(np.nextafter(f32(-1.0), f32(-2.0))), 0.0, 1.0))  # u just below 0
    names["z_zero"] = len(specs)
    specs.append((0.0, 0.0, 0.0))
    names["z_negative"] = len(specs)
    specs.append((0.0, 0.0, -1.0))
    for k, bad in enumerate([(np.nan, 0, 1), (0, np.nan, 1), (0, 0, np.nan), (np.inf, 0, 1), (0, -np.inf, 1), (0, 0, np.inf),
                             (0, 0, -np.inf), (np.inf, np.inf, np.inf)]):
        names.setdefault("bad", len(specs))
        specs.append(bad)
    for j in range(600):  # one pixel holding 600 points, all within the threshold of the nearest
        add("crowd", 1, 1, 1.0 + j / 4096.0)
    add("crowd_behind", 1, 1, 1.5)
    rng = np.random.default_rng(7)
    n_rest = 4099 - len(specs)
    z = rng.uniform(2.0, 4.0, n_rest)  # behind every named point
    rest = np.stack([rng.uniform(-1.3, 1.3, n_rest) * z, rng.uniform(-0.7, 0.7, n_rest) * z, z], 1)
    pts = np.concatenate([np.asarray(specs, np.float64), rest]).astype(np.float32)
    # the first 65 points hold the named cases but the crowd
    order = [i for i in range(len(specs)) if not names["crowd"] <= i < names["crowd"] + 600]
    order = order + [i for i in range(len(pts)) if i not in set(order)]
    remap = {old: new for new, old in enumerate(order)}
    return pts[order], {k: remap[i] for k, i in names.items()}


def _edge_views():
    y, x = np.meshgrid(np.arange(EH), np.arange(EW), indexing="ij")
    mask = (1 + x % 3 + 3 * (y % 2)).astype(np.int32) * 7 - 50  # -43 .. -8: negative, non-contiguous ids
    mask[3, 11] = 0
    small = np.array([[5, 0, 9], [9, 9, 5], [0, 5, 2 ** 31 - 1]], np.int32)  # a second view of another size
    return [pinhole_camera(EW, EH, EF, EF), pinhole_camera(3, 3, 2.0, 2.0, (0.1, -0.2, 0.3))], [mask, small]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4099])
@pytest.mark.parametrize("depth_thresh", [ETHRESH, -1.0])
def test_labels_of_the_edge_cloud(hip_lib, n, depth_thresh):
    pts, names = _edge_cloud()
    pts = pts[:n]
    cams, masks = _edge_views()
    got = planes.front_point_labels(cams, dev(pts), [dev(m) for m in masks], depth_thresh).cpu().numpy()
    want = np.stack([pr.front_labels(pts, c, m, depth_thresh) for c, m in zip(cams, masks)])
    assert np.array_equal(got, want)
    assert got[0, 0] == 0 and got[1, 0] == 0  # point 0 never carries a label
    if n < 4099:
        return
    lab, mask = got[0], masks[0]
    on = depth_thresh >= 0
    assert lab[names["front"]] == mask[4, 8] == lab[names["equal_z"]] == lab[names["inside"]]
    assert lab[names["at_threshold"]] == (0 if on else mask[4, 8]) and lab[names["behind"]] == (0 if on else mask[4, 8])
    assert lab[names["half_even"]] == mask[4, 2] and lab[names["half_odd"]] == mask[4, 4]
    assert lab[names["half_v_even"]] == mask[0, 5] and lab[names["half_v_odd"]] == mask[2, 5]
    assert lab[names["clamp_u"]] == mask[4, 15] and lab[names["clamp_u2"]] == mask[2, 15] and lab[names["clamp_v"]] == mask[7, 6]
    assert lab[names["below_zero"]] == 0 and lab[names["z_zero"]] == 0 and lab[names["z_negative"]] == 0
    # NaN and infinite coordinates are in no image (inf * 0 in the transform is NaN, as is inf / inf)
    assert not lab[names["bad"]: names["bad"] + 8].any()
    crowd = lab[names["crowd"]: names["crowd"] + 600]
    assert (crowd == mask[1, 1]).all()  # no cap of 500 points per pixel
    assert lab[names["crowd_behind"]] == (0 if on else mask[1, 1])
    assert (want[1] != 0).sum() > 100  # the second, smaller view of the same launch


# ---- membership and counts against numpy sets -------------------------------------------------------------------------------
N_SETS = 1061  # five blocks, not a multiple of 64


def _random_membership(G, rng, N=N_SETS, tail=None):
    """(PlaneMembership, bool [G, N]) built by three assign launches, so that points belong to several rows.  With `tail`
    the last row gets members at and above that index only."""
    member = planes.PlaneMembership(N, DEV)
    want = np.zeros((G, N), bool)
    for _round in range(3):
        labels = rng.integers(0, G + 1, N).astype(np.int32)
        labels[rng.integers(0, N, 40)] = G + 7  # outside 1 .. P: counts as no label
        labels[rng.integers(0, N, 40)] = -3
        target = rng.permutation(G).tolist()
        if G > 2 and target[1] != G - 1:
            target[1] = -1
        if tail is not None:
            head = labels[:tail]
            head[head == target.index(G - 1) + 1] = 0
        member.assign(dev(labels), target)
        for p, t in enumerate(target):
            if t >= 0:
                want[t] |= labels == p + 1
    assert member.G == G and member.n_words >= (G + 63) // 64
    assert tail is None or (want[G - 1, tail:].any() and not want[G - 1, :tail].any())
    return member, want


def _check_words(member, want):
    words = member.words.cpu().numpy().view(np.uint64)
    G, N = want.shape
    for w in range(member.n_words):
        expect = np.zeros(N, np.uint64)
        for b in range(64):
            if 64 * w + b < G:
                expect |= want[64 * w + b].astype(np.uint64) << np.uint64(b)
        assert np.array_equal(words[w, :N], expect), w  # the bits at and above G stay zero


@pytest.mark.parametrize("P", [1, 70])
@pytest.mark.parametrize("G", [1, 63, 64, 65, 130])
def test_counts_and_assign_against_numpy_sets(hip_lib, G, P):
    rng = np.random.default_rng(100 * G + P)
    member, want = _random_membership(G, rng)
    _check_words(member, want)
    labels = rng.integers(0, P + 1, N_SETS).astype(np.int32)
    labels[::97] = P + 1
    labels[5::101] = -1
    # runs of equal labels next to scattered ones: both ends of the wave-level aggregation
    labels[200:400] = 1
    sizes, counts = member.overlap(dev(labels), P)
    assert sizes == [int((labels == p).sum()) for p in range(1, P + 1)]
    assert counts == [[int(((labels == p) & want[g]).sum()) for g in range(G)] for p in range(1, P + 1)]
    # row overlap, row merge, row to indices
    for row in sorted({0, G // 2, G - 1}):
        assert member.row_counts(row) == [int((want[row] & want[h]).sum()) for h in range(G)]
        idx = member.row_indices(row)
        assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), np.nonzero(want[row])[0])
    src, dst = G - 1, 0
    member.merge_rows(dst, src)
    want[dst] |= want[src]
    _check_words(member, want)
    assert member.row_counts(dst) == [int((want[dst] & want[h]).sum()) for h in range(G)]


def test_counts_beyond_the_workgroup_table(hip_lib):
    """8200 global planes: more entries than a workgroup keeps in LDS (8192), so both count kernels add straight into the
    global tables; 129 words per point."""
    G = 8200
    rng = np.random.default_rng(8200)
    member, want = _random_membership(G, rng)
    assert member.n_words >= 129
    _check_words(member, want)
    rows = want.astype(np.int64)
    for row in (0, 4100, G - 1):
        assert member.row_counts(row) == (rows @ rows[row]).tolist()
    labels = rng.integers(0, 3, N_SETS).astype(np.int32)
    sizes, counts = member.overlap(dev(labels), 2)
    assert sizes == [int((labels == p).sum()) for p in (1, 2)]
    assert counts == [(rows @ (labels == p).astype(np.int64)).tolist() for p in (1, 2)]


# Both count kernels launch at most COUNT_MAX_BLOCKS = 2048 workgroups of 256 points and keep their table in LDS while it
# has at most COUNT_LDS_MAX = 8192 entries.  Whoever changes one of the two moves the sizes below.
ONE_PASS = 2048 * 256  # COUNT_MAX_BLOCKS * 256 points
N_PAST = ONE_PASS + 300  # workgroup 0 takes a second block of 256 points, workgroup 1 one of 44
LDS_MAX = 8192  # COUNT_LDS_MAX


@pytest.mark.parametrize("P,G", [(3, 65), (70, 130)])
def test_overlap_past_the_grid_cap(hip_lib, P, G):
    """(3, 65): 198 entries, the LDS table over two words per point; (70, 130): 9 170 entries, the global table.  Label P
    and global row G - 1 occur at and above point 524 288 only: a kernel that stops after its first pass leaves their
    row and column at zero."""
    assert (P * G + P <= LDS_MAX) == (P == 3)
    rng = np.random.default_rng(100 * G + P)
    member, want = _random_membership(G, rng, N_PAST, tail=ONE_PASS)
    labels = rng.integers(0, P, N_PAST).astype(np.int32)
    labels[ONE_PASS:] = rng.integers(0, P + 1, N_PAST - ONE_PASS)
    labels[::97] = P + 1
    labels[5::101] = -1
    labels[ONE_PASS + 250: ONE_PASS + 290] = P  # a run of the tail's label across the last wave boundary
    sizes, counts = member.overlap(dev(labels), P)
    want_sizes, want_counts = pr.overlap_counts(labels, P, want)
    assert sizes == want_sizes and counts == want_counts
    assert sizes[P - 1] == int((labels[ONE_PASS:] == P).sum()) >= 40 and not (labels[:ONE_PASS] == P).any()
    assert sum(want_counts[P - 1]) > 0 and sum(row[G - 1] for row in want_counts) > 0  # the tail's row and column count
    in_tail = pr.overlap_counts(labels[ONE_PASS:], P, want[:, ONE_PASS:])
    assert in_tail[1][P - 1] == want_counts[P - 1] and [row[G - 1] for row in in_tail[1]] == [row[G - 1] for row in want_counts]


def test_row_counts_past_the_grid_cap_with_a_workgroup_table(hip_lib):
    """G = 130: the LDS table of the row kernel, flushed after two passes.  Row 0 holds half of all points, so that every
    wave has lanes at work in both passes; row G - 1 has members in the second pass only."""
    G = 130
    rng = np.random.default_rng(130)
    member, want = _random_membership(G, rng, N_PAST, tail=ONE_PASS)
    half = rng.integers(0, 2, N_PAST).astype(np.int32)
    member.assign(dev(half), [0])
    want[0] |= half == 1
    for row in (0, G - 1):
        got = member.row_counts(row)
        assert got == pr.row_overlap_counts(want, row)
        assert got[row] == int(want[row].sum()) > 0
    assert any(member.row_counts(G - 1)[:G - 1])  # the tail's row shares points with other rows
    head = pr.row_overlap_counts(want[:, :ONE_PASS], 0)
    assert head != pr.row_overlap_counts(want, 0)  # the second pass changes row 0's counts


def test_row_counts_past_the_grid_cap_with_the_global_table(hip_lib):
    """G = 8 200 over 524 588 points (129 words per point): the row kernel adds straight into the global table.  Only five
    rows have members, so the expected counts are five boolean rows and not 8 200; row 8 199 has members in the second
    pass only."""
    G, rows = 8200, [0, 63, 64, 4100, 8199]
    assert G > LDS_MAX
    rng = np.random.default_rng(8201)
    member = planes.PlaneMembership(N_PAST, DEV)
    some = np.zeros((len(rows), N_PAST), bool)
    for _round in range(3):
        labels = rng.integers(0, 2 * len(rows), N_PAST).astype(np.int32)  # half of the labels: no target
        order = rng.permutation(len(rows)).tolist()
        tail_label = order.index(len(rows) - 1) + 1
        head = labels[:ONE_PASS]
        head[head == tail_label] = 0
        target = [-1] * G
        for p, k in enumerate(order):
            target[p] = rows[k]
            some[k] |= labels == p + 1
        member.assign(dev(labels), target)
    assert member.G == G and member.n_words >= 129
    assert some[-1, ONE_PASS:].any() and not some[-1, :ONE_PASS].any() and (some.sum(0) > 1).any()
    for k, row in enumerate(rows):
        want = [0] * G
        for h, c in zip(rows, pr.row_overlap_counts(some, k)):
            want[h] = c
        assert member.row_counts(row) == want, row
        assert want[row] == int(some[k].sum()) > 0
    assert member.row_counts(5) == [0] * G  # a row without members


@pytest.mark.parametrize("P,G", [(64, 127), (64, 128)])
def test_overlap_at_the_switch_between_the_workgroup_and_the_global_table(hip_lib, P, G):
    """64 * 127 + 64 = 8 192 entries: the largest LDS table (32 KiB of dynamic LDS); 64 * 128 + 64 = 8 256: the first
    global one."""
    assert (P * G + P <= LDS_MAX) == (G == 127) and P * 127 + P == LDS_MAX
    rng = np.random.default_rng(100 * G + P)
    member, want = _random_membership(G, rng)
    labels = rng.integers(0, P + 1, N_SETS).astype(np.int32)
    labels[::97] = P + 1
    labels[5::101] = -1
    labels[200:400] = P  # the last table row, in runs
    sizes, counts = member.overlap(dev(labels), P)
    want_sizes, want_counts = pr.overlap_counts(labels, P, want)
    assert sizes == want_sizes and counts == want_counts
    assert sizes[P - 1] >= 200 and min(sizes) > 0
    assert any(want_counts[P - 1]) and any(row[G - 1] for row in want_counts)  # the table's last row and column are in use


@pytest.mark.parametrize("G", [8192, 8193])
def test_row_counts_at_the_switch_between_the_workgroup_and_the_global_table(hip_lib, G):
    """G = 8 192 = COUNT_LDS_MAX: the largest LDS table of the row kernel; 8 193: the first global one."""
    assert (G <= LDS_MAX) == (G == 8192)
    rng = np.random.default_rng(G)
    member, want = _random_membership(G, rng)
    labels = rng.integers(0, 4, N_SETS).astype(np.int32)  # a thousand points spread over G rows leave most rows empty:
    member.assign(dev(labels), [0, 4100, G - 1])        # the rows asked for below get a quarter of the points each
    for p, row in enumerate((0, 4100, G - 1)):
        want[row] |= labels == p + 1
    _check_words(member, want)
    for row in (0, 4100, G - 1):
        got = member.row_counts(row)
        assert got == pr.row_overlap_counts(want, row)
        assert got[row] == int(want[row].sum()) > 200 and sum(1 for c in got if c) > 100
    assert got[G - 1] > 200  # the table's last entry is in use


def test_membership_grows_across_a_word(hip_lib):
    """Rows are added one view at a time until G crosses 64 and 128; earlier bits survive the growth."""
    rng = np.random.default_rng(3)
    member = planes.PlaneMembership(N_SETS, DEV)
    want = np.zeros((0, N_SETS), bool)
    for step in range(5):
        labels = rng.integers(0, 31, N_SETS).astype(np.int32)
        G = want.shape[0]
        member.assign(dev(labels), list(range(G, G + 30)))
        want = np.concatenate([want, np.stack([labels == p for p in range(1, 31)])])
        assert member.G == G + 30
    _check_words(member, want)
    assert member.row_counts(149) == [int((want[149] & want[h]).sum()) for h in range(150)]


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _run(golden, previous=None):
    idx, ids = planes.get_global_3Dplane(golden.cams, dev(golden.points), [dev(m) for m in golden.masks], previous, 0.5,
                                         golden.depth_thresh)
    assert all(i.dtype == torch.int64 and i.device.type == "cuda" for i in idx)
    return [i.cpu().numpy() for i in idx], ids


def test_golden_dict_and_index_sets(hip_lib, golden):
    idx, ids = _run(golden)
    assert ids == golden.ids
    assert len(idx) == len(golden.idx) and all(np.array_equal(a, b) for a, b in zip(idx, golden.idx))


def test_golden_resume_path(hip_lib, golden):
    idx3, ids3 = planes.get_global_3Dplane(golden.cams[:3], dev(golden.points), [dev(m) for m in golden.masks[:3]], None,
                                           0.5, golden.depth_thresh)
    assert ids3 == golden.ids3
    idx, ids = _run(golden, ids3)
    assert ids == golden.resume_ids
    assert len(idx) == len(golden.resume_idx) and all(np.array_equal(a, b) for a, b in zip(idx, golden.resume_idx))


def test_seventy_stripes_push_G_over_a_word_and_an_empty_plane_of_view_zero_stays(hip_lib):
    """A planar grid of points at z = 2 under a mask of 70 two-pixel stripes; the second view is shifted by one pixel, so
    every stripe covers exactly half of two stripes of the first view, 0.5 is not above the threshold and all but the first stay apart:
    140 global planes through the public function.  View 0 also has a mask id on columns no point projects to."""
    W, H, F = 144, 8, 64.0
    x, y = np.meshgrid(np.arange(140), np.arange(H), indexing="xy")
    grid = np.stack([(x.reshape(-1) - W / 2) / F * 2.0, (y.reshape(-1) - H / 2) / F * 2.0, np.full(x.size, 2.0)], 1)
    pts = np.concatenate([[[50.0, 50.0, 1.0]], grid]).astype(np.float32)  # point 0 is nowhere
    cols = np.arange(W)
    row = np.where(cols < 140, 3 * (cols // 2) + 4, 0).astype(np.int32)
    mask0 = np.repeat(row[None], H, 0)
    mask0[:, 142:] = 999  # no point projects there: an empty plane of view 0
    mask1 = np.repeat(row[None], H, 0)
    cams = [pinhole_camera(W, H, F, F), pinhole_camera(W, H, F, F, (2.0 / F, 0.0, 0.0))]
    idx, ids = planes.get_global_3Dplane(cams, dev(pts), [dev(mask0), dev(mask1)])
    ref_idx, ref_ids = pr.get_global_3Dplane(pts, cams, [mask0, mask1])
    assert ids == ref_ids
    assert len(idx) == len(ref_idx) and all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(idx, ref_idx))
    assert len(ids) > 128 and ids[70] == [(0, 999)] and idx[70].numel() == 0
    # view 1's first stripe sees only column 0 and lies inside view 0's first; every other stripe stays alone
    assert len(ids) == 140 and ids[0] == [(0, 4), (1, 4)] and sum(len(pairs) == 1 for pairs in ids.values()) == 139
    # with a lower threshold the halves merge
    idx, ids = planes.get_global_3Dplane(cams, dev(pts), [dev(mask0), dev(mask1)], None, 0.4)
    ref_idx, ref_ids = pr.get_global_3Dplane(pts, cams, [mask0, mask1], None, 0.4)
    assert ids == ref_ids and len(ids) < 72 and [(0, 999)] in ids.values()
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(idx, ref_idx))


def test_two_runs_are_identical_byte_for_byte(hip_lib, golden, golden_labels):
    pts, masks = dev(golden.points), [dev(m) for m in golden.masks]
    again = planes.front_point_labels(golden.cams, pts, masks, golden.depth_thresh)
    assert torch.equal(again, golden_labels[0])
    runs = []
    for _ in range(2):
        views = planes._LabelledViews(golden.cams, pts, masks, golden.depth_thresh)
        provider = planes._DeviceProvider(views)
        read = []
        for v in range(len(golden.cams)):
            ids, sizes, counts = provider.view_counts(v)
            provider.assign(v, [k % 7 for k in range(len(ids))])
            read.append((ids, sizes, counts))
        read.append([provider.row_counts(g) for g in range(provider.member.G)])
        idx, ids = _run(golden)
        runs.append((read, ids, [provider.member.words] + list(idx)))
    assert runs[0][:2] == runs[1][:2]
    same_bits(runs[1][2], runs[0][2], "second run")


# ---- argument validation ------------------------------------------------------------------------------------------------------
def test_argument_validation_is_host_side(hip_lib):
    """Bad sizes and NULL pointers return the library's error code with a message before anything is launched."""
    lib = hip_lib
    nul, one, big = ctypes.c_void_p(0), ctypes.c_void_p(256), 1 << 20  # `one` is never dereferenced
    INVALID = -1

    def expect(rc, text):
        assert rc == INVALID, rc
        assert text.encode() in lib.g4s_last_error(), lib.g4s_last_error()

    wv, focal = (ctypes.c_float * 16)(), (ctypes.c_float * 2)(1.0, 1.0)
    sizes, bad_sizes = (ctypes.c_int * 2)(4, 4), (ctypes.c_int * 2)(0, 4)
    masks, no_mask = (ctypes.c_void_p * 1)(256), (ctypes.c_void_p * 1)(0)
    assert lib.g4s_plane_labels_workspace(1, sizes) >= 88 + 64
    assert lib.g4s_plane_labels_workspace(1, bad_sizes) == 0 and lib.g4s_plane_labels_workspace(-1, sizes) == 0
    expect(lib.g4s_plane_labels(-1, one, 0.01, 1, wv, focal, sizes, masks, one, one, big, nul), "n_points must be in")
    expect(lib.g4s_plane_labels(5, one, float("nan"), 1, wv, focal, sizes, masks, one, one, big, nul), "must not be NaN")
    expect(lib.g4s_plane_labels(5, one, 0.01, -1, wv, focal, sizes, masks, one, one, big, nul), "n_views must not be negative")
    expect(lib.g4s_plane_labels(5, nul, 0.01, 1, wv, focal, sizes, masks, one, one, big, nul), "NULL required pointer")
    expect(lib.g4s_plane_labels(5, one, 0.01, 1, wv, focal, sizes, nul, one, one, big, nul), "NULL required pointer")
    expect(lib.g4s_plane_labels(5, one, 0.01, 1, wv, focal, bad_sizes, masks, one, one, big, nul), "must be positive")
    huge_sizes = (ctypes.c_int * 2)(1 << 15, (1 << 15) + 1)
    expect(lib.g4s_plane_labels(5, one, 0.01, 1, wv, focal, huge_sizes, masks, one, one, big, nul), "width * height at most 2^30")
    expect(lib.g4s_plane_labels(5, one, 0.01, 1, wv, focal, nul, masks, one, one, big, nul), "NULL required pointer")
    assert lib.g4s_plane_labels_workspace(70000, (ctypes.c_int * 140000)(*([2, 2] * 70000))) > 70000 * (88 + 256)  # no view cap
    expect(lib.g4s_plane_labels(5, one, 0.01, 1, wv, focal, sizes, masks, one, one, 8, nul), "workspace too small")
    edge = lib.g4s_plane_labels_workspace(1, sizes) - 1
    expect(lib.g4s_plane_labels(5, one, 0.01, 1, wv, focal, sizes, masks, one, one, edge, nul), "workspace too small")
    expect(lib.g4s_plane_labels(5, one, 0.01, 1, wv, focal, sizes, no_mask, one, one, 8, nul), "workspace too small")  # checked first
    expect(lib.g4s_plane_labels(5, one, 0.01, 1, wv, focal, sizes, no_mask, one, one, big, nul), "NULL map pointer")
    assert lib.g4s_plane_labels(5, one, 0.01, 0, nul, nul, nul, nul, nul, nul, 0, nul) == 0  # no view: nothing to do
    expect(lib.g4s_plane_overlap(5, one, 2, 3, 0, one, one, one, nul, 0, nul), "n_words must be in")
    expect(lib.g4s_plane_overlap(5, one, 2, 65, 1, one, one, one, nul, 0, nul), "n_global in 0 .. 64 * n_words")
    expect(lib.g4s_plane_overlap(5, one, -1, 3, 1, one, one, one, nul, 0, nul), "n_planes must not be negative")
    expect(lib.g4s_plane_overlap(5, one, 1 << 20, 1 << 12, 64, one, one, one, nul, 0, nul), "at most 2^30")
    expect(lib.g4s_plane_overlap(5, one, 2, 3, 1, nul, one, one, nul, 0, nul), "NULL required pointer")
    expect(lib.g4s_plane_overlap(5, one, 2, 3, 1, one, nul, one, nul, 0, nul), "NULL required pointer")
    expect(lib.g4s_plane_overlap(5, nul, 2, 3, 1, one, one, one, nul, 0, nul), "NULL required pointer")
    target, bad_target = (ctypes.c_int * 2)(0, -1), (ctypes.c_int * 2)(0, 3)
    expect(lib.g4s_plane_assign(5, one, 2, bad_target, 3, 1, one, one, big, nul), "target[1] must be -1 or a global plane")
    expect(lib.g4s_plane_assign(5, one, 2, nul, 3, 1, one, one, big, nul), "NULL required pointer")
    expect(lib.g4s_plane_assign(5, one, 2, target, 3, 1, one, one, 4, nul), "workspace too small")
    assert lib.g4s_plane_assign_workspace(2) == 8 + 256 and lib.g4s_plane_assign_workspace(-1) == 256
    expect(lib.g4s_plane_assign(5, one, 2, target, 3, 1, one, one, 8 + 255, nul), "workspace too small")
    expect(lib.g4s_plane_assign(5, one, 2, target, 3, 1, one, nul, big, nul), "workspace too small")
    expect(lib.g4s_plane_assign((1 << 30) + 1, one, 2, target, 3, 1, one, one, big, nul), "n_points must be in")
    expect(lib.g4s_plane_row_overlap(5, 3, 1, one, 3, one, nul, 0, nul), "row must be a global plane below n_global")
    expect(lib.g4s_plane_row_overlap(5, 3, 1, one, 0, nul, nul, 0, nul), "NULL required pointer")
    expect(lib.g4s_plane_row_merge(5, 3, 1, one, -1, 0, nul, 0, nul), "src must be a global plane below n_global")
    expect(lib.g4s_plane_row_merge(5, 3, 1, one, 0, 3, nul, 0, nul), "dst must be a global plane below n_global")
    expect(lib.g4s_plane_row_merge(5, 3, 1, nul, 0, 1, nul, 0, nul), "NULL required pointer")
    expect(lib.g4s_plane_row_mask(5, 3, 1, one, 5, one, nul, 0, nul), "row must be a global plane below n_global")
    expect(lib.g4s_plane_row_mask(5, 3, 1, one, 0, nul, nul, 0, nul), "NULL required pointer")
