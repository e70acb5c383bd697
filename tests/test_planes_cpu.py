"""The numpy restatement of the global-planes contract (tests/planes_ref.py) and the shared decision function of
g4splat_amd/planes.py against vectors recorded from the reference's own code (tests/golden/make_golden_planes.py):
labels on the agreed set, dicts and index sets exactly, the resume path, the hand-made merge cases, the JSON round trip.
No GPU: the GPU tests (tests/test_gpu_planes.py) hold the library to the restatement bit for bit."""
import json

import numpy as np
import pytest

import planes_ref as pr
from g4splat_amd import planes
from support import load_planes_golden


@pytest.fixture(scope="module")
def golden():
    return load_planes_golden()


@pytest.fixture(scope="module")
def ref_planes(golden):
    """Per view [(plane id, set)] from the restatement's float32 labels, computed once."""
    return pr.all_planes(golden.points, golden.cams, golden.masks, golden.depth_thresh)


def _same_sets(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert np.array_equal(np.asarray(a, np.int64), np.asarray(b, np.int64))


def test_golden_scene_has_the_cases_the_merge_needs(golden):
    s = golden.stats
    assert s["update_merges"] >= 1 and s["new_planes"] >= 1 and s["final_merges"] >= 1 and s["empty_planes"] >= 1
    assert max(r / n for r, n in s["rejected"]) >= 0.05
    excluded, total, _differ = golden.g["labels_excluded"]
    assert excluded <= 0.001 * total
    assert len({int(i) for m in golden.masks for i in np.unique(m)}) > 20  # non-contiguous ids, different per view


def test_restatement_labels_equal_the_reference_on_the_agreed_set(golden):
    V, N = golden.g["labels"].shape
    agreed = np.unpackbits(golden.g["labels_agreed"])[: V * N].astype(bool).reshape(V, N)
    for v in range(V):
        got = pr.front_labels(golden.points, golden.cams[v], golden.masks[v], golden.depth_thresh)
        assert got[0] == 0
        assert np.array_equal(got[agreed[v]], golden.g["labels"][v][agreed[v]])
        assert (got != 0).sum() > 500


def test_restatement_merge_equals_the_reference(golden):
    idx, ids = pr.get_global_3Dplane(golden.points, golden.cams, golden.masks, None, 0.5, golden.depth_thresh)
    assert ids == golden.ids
    _same_sets(idx, golden.idx)


def test_restatement_resume_path_equals_the_reference(golden):
    _i3, ids3 = pr.get_global_3Dplane(golden.points, golden.cams[:3], golden.masks[:3], None, 0.5, golden.depth_thresh)
    assert ids3 == golden.ids3
    idx, ids = pr.get_global_3Dplane(golden.points, golden.cams, golden.masks, golden.ids3, 0.5, golden.depth_thresh)
    assert ids == golden.resume_ids
    _same_sets(idx, golden.resume_idx)


def test_shared_decisions_over_restatement_counts_equal_the_reference(golden, ref_planes):
    idx, ids = planes.merge_global_planes(pr.SetProvider(ref_planes), len(golden.cams))
    assert ids == golden.ids
    _same_sets(idx, golden.idx)
    # resume: the dict as loaded from JSON (string keys, lists) is accepted
    previous = {str(k): [list(p) for p in pairs] for k, pairs in golden.ids3.items()}
    idx, ids = planes.merge_global_planes(pr.SetProvider(ref_planes), len(golden.cams), previous)
    assert ids == golden.resume_ids
    _same_sets(idx, golden.resume_idx)
    idx3, ids3 = planes.merge_global_planes(pr.SetProvider(ref_planes[:3]), 3)
    assert ids3 == golden.ids3


def _hand(case):
    """(views of [(id, set)], previous dict, {the reference's (view, plane): ours}) of a hand-made case for the decision
    function.  Global planes may overlap, the local planes of one view may not, so every given global plane enters as the
    single plane of a view of its own, named by a previous dict: rebuilt, then updated and swept."""
    init = case.get("final", case.get("init"))
    views = [[(1, set(s))] for s in init]
    names = {(k, 1) if "final" in case else (0, k + 1): (k, 1) for k in range(len(init))}
    if "update" in case:
        views.append([(k + 1, set(s)) for k, s in enumerate(case["update"])])
        names.update({(1, k + 1): (len(init), k + 1) for k in range(len(case["update"]))})
    return views, {k: [(k, 1)] for k in range(len(init))}, names


@pytest.mark.parametrize("name", ["chain", "chain_reordered", "exactly_half", "first_wins"])
def test_hand_made_cases(golden, name):
    case, want = golden.hand_cases[name], golden.hand_results[name]
    views, previous, names = _hand(case)
    want_ids = {int(k): [names[(v, p)] for v, p in pairs] for k, pairs in want["ids"].items()}
    idx, ids = planes.merge_global_planes(pr.SetProvider(views), len(views), previous)
    assert ids == want_ids
    assert [a.tolist() for a in idx] == want["sets"]
    # and the restatement's own loops
    n = len(previous)
    sets, rids = [set(S) for (_p, S), in views[:n]], {k: [(k, 1)] for k in range(n)}
    if "update" in case:
        pr.update_sets(sets, rids, views[n], n)
    sets, rids, _n = pr.final_merge_sets(sets, rids)
    assert rids == want_ids and [sorted(s) for s in sets] == want["sets"]


def test_hand_made_cases_say_what_they_are_for(golden):
    r = golden.hand_results
    assert len(r["chain"]["sets"]) == 1 and len(r["chain_reordered"]["sets"]) == 2  # C passes only against A ∪ B
    assert len(r["exactly_half"]["sets"]) == 2  # 0.5 is not above 0.5
    assert r["first_wins"]["ids"]["0"][:2] == [[0, 1], [1, 1]]
    assert planes.covisibility_rate(2, 4, 4) == 0.5 and not planes.covisibility_rate(2, 4, 4) > 0.5
    assert planes.covisibility_rate(0, 0, 5) == 0.0 and planes.covisibility_rate(0, 5, 0) == 0.0


def test_empty_plane_in_view_zero_keeps_its_entry_and_never_merges():
    views = [[(3, {1, 2, 3}), (9, set())], [(4, {1, 2, 3, 4}), (5, set())]]
    idx, ids = planes.merge_global_planes(pr.SetProvider(views), 2)
    assert ids == {0: [(0, 3), (1, 4)], 1: [(0, 9)]}
    assert [a.tolist() for a in idx] == [[1, 2, 3, 4], []]


@pytest.mark.parametrize("P,G,N,block", [(1, 1, 64, 1 << 16), (3, 65, 1061, 1 << 16), (7, 13, 1061, 100), (5, 4, 300, 300)])
def test_matrix_product_counts_equal_the_sets(P, G, N, block):
    """pr.overlap_counts and pr.row_overlap_counts serve the GPU tests whose point counts are too large for Python sets;
    here they run against SetProvider's own counts, whole and in blocks of points that do not divide N."""
    rng = np.random.default_rng(1000 * P + G)
    member = rng.random((G, N)) < 0.3
    member[G - 1, : N // 2] = False  # a row with members in the tail only
    labels = rng.integers(-1, P + 3, N)  # -1, 0, P + 1 and P + 2: no label
    labels[N // 2:][labels[N // 2:] == 1] = 0  # a label in the first half only
    view = [(p, set(np.nonzero(labels == p)[0].tolist())) for p in range(1, P + 1)]
    provider = pr.SetProvider([view])
    provider.rows = [set(np.nonzero(m)[0].tolist()) for m in member]
    _ids, want_sizes, want_counts = provider.view_counts(0)
    sizes, counts = pr.overlap_counts(labels, P, member, block)
    assert sizes == want_sizes and counts == want_counts
    assert all(type(c) is int for c in sizes) and all(type(c) is int for row in counts for c in row)
    assert sum(sizes) == int(((labels >= 1) & (labels <= P)).sum()) > 0
    for row in sorted({0, G // 2, G - 1}):
        assert pr.row_overlap_counts(member, row, block) == provider.row_counts(row)
    # the expression the GPU tests of small tables use
    assert counts == [[int(((labels == p) & member[g]).sum()) for g in range(G)] for p in range(1, P + 1)]


def test_previous_dict_is_validated():
    views = [[(1, {1})], [(1, {1})]]
    with pytest.raises(ValueError, match="keys 0 .. K-1"):
        planes.merge_global_planes(pr.SetProvider(views), 2, {1: [(0, 1)]})
    with pytest.raises(ValueError, match="names view 5"):
        planes.merge_global_planes(pr.SetProvider(views), 2, {0: [(5, 1)]})
    with pytest.raises(ValueError, match="twice"):
        planes.merge_global_planes(pr.SetProvider(views), 2, {0: [(0, 1)], 1: [(0, 1)]})


def test_json_round_trip(golden, tmp_path):
    path = tmp_path / "global_3Dplane_ID_dict.json"
    planes.save_global_3Dplane_ID_dict(path, golden.ids)
    raw = json.load(open(path))
    assert list(raw) == [str(k) for k in golden.ids]  # the reference's shape: string keys, lists of pairs
    assert all(isinstance(p, list) and len(p) == 2 for pairs in raw.values() for p in pairs)
    assert raw == json.loads(str(golden.g["ids"]))
    assert planes.load_global_3Dplane_ID_dict(path) == golden.ids


def test_plane_masks_are_checked_before_the_device():
    import torch
    cpu, hip = torch.device("cpu"), torch.device("cuda", 0)
    for bad in (torch.zeros((3, 4), dtype=torch.int32), [[0]]):
        with pytest.raises(RuntimeError, match="plane masks must be tensors on cuda:0"):
            planes.slot_mask(bad, hip)
    for bad in (torch.zeros((3, 4)), torch.zeros((1, 3, 4), dtype=torch.int32)):
        with pytest.raises(RuntimeError, match=r"a plane mask must be an integer tensor \[H,W\]"):
            planes.slot_mask(bad, cpu)
    slots, ids = planes.slot_mask(torch.tensor([[0, 7, 7], [3, 0, -2]]), cpu)
    assert slots.dtype == torch.int32 and slots.tolist() == [[0, 3, 3], [2, 0, 1]] and ids.tolist() == [-2, 3, 7]
    with pytest.raises(RuntimeError, match="points must be a tensor on a HIP device"):
        planes.front_point_labels([None], [[0.0, 0.0, 0.0]], [torch.zeros((3, 4), dtype=torch.int32)])
