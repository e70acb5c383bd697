"""numpy restatement of the global-planes contract (include/g4s_render_maps.h, "Global planes").

Labels are computed exactly per the header: the projection is visibility_ref.project (float32 in the header's order, or
float64 with dtype=np.float64, which only the golden generator's cross-check uses), the per-pixel minimum is a plain
minimum, the depth test one float add and a strict <.  The merge is written with Python sets, once directly
(`update_sets`, `final_merge_sets`, `get_global_3Dplane`: the reference's loops restated) and once as a counts provider
(`SetProvider`) for the shared decision function of g4splat_amd/planes.py.  It asserts the two facts the device path
rests on: the local planes of a view are disjoint, and sizes follow |G ∪ S| = |G| + |S| - |G ∩ S|.  Slow and simple: for tests
only.
"""
import numpy as np

import visibility_ref as vr

f32 = np.float32


def _host(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def candidates(points, cam, W, H, dtype=f32):
    """(candidate [n] bool, pixel [n] int64 row-major, z [n]) of points [n,3] in a view whose mask is W x H."""
    z, u, v, inside = vr.project(points, cam, W, H, dtype)
    with np.errstate(invalid="ignore"):
        cand = inside & (z > 0)
    if len(cand):
        cand[0] = False
    uu, vv = np.where(cand, u, 0), np.where(cand, v, 0)
    px = np.minimum(np.rint(uu).astype(np.int64), W - 1)  # np.rint rounds half to even
    py = np.minimum(np.rint(vv).astype(np.int64), H - 1)
    return cand, py * W + px, z


def front_labels(points, cam, mask, depth_thresh=0.01, dtype=f32):
    """int64 [n]: the mask value of every front point, 0 elsewhere.  depth_thresh < 0: no depth test."""
    mask = _host(mask)
    H, W = mask.shape
    cand, pix, z = candidates(points, cam, W, H, dtype)
    idx = np.nonzero(cand)[0]
    labels = np.zeros(len(cand), np.int64)
    if depth_thresh < 0:
        keep = idx
    else:
        zmin = np.full(H * W, np.inf, dtype)
        np.minimum.at(zmin, pix[idx], z[idx])
        keep = idx[z[idx] < zmin[pix[idx]] + dtype(depth_thresh)]
    labels[keep] = mask.reshape(-1)[pix[keep]]
    return labels


def depth_rejected(points, cam, mask, depth_thresh=0.01, dtype=f32):
    """(rejected, candidates in the mask): how many in-image, in-mask points the depth test drops."""
    on = front_labels(points, cam, mask, depth_thresh, dtype) != 0
    off = front_labels(points, cam, mask, -1.0, dtype) != 0
    return int(off.sum() - on.sum()), int(off.sum())


def local_planes(labels):
    """[(plane id, set of point indices)] in ascending id order, 0 left out; the sets are disjoint by construction
    (fact 1: a point has one label)."""
    ids = [int(i) for i in np.unique(labels) if i != 0]
    sets = [set(np.nonzero(labels == i)[0].tolist()) for i in ids]
    assert sum(len(s) for s in sets) == int((labels != 0).sum()) == len(set().union(*sets)) if sets else True
    assert all(0 not in s for s in sets)
    return list(zip(ids, sets))


def mask_plane_ids(mask):
    return [int(i) for i in np.unique(_host(mask)) if i != 0]


def rate(G, S):
    """The reference's get_covisibility_rate; an empty set has rate 0 (the reference raises)."""
    if not G or not S:
        return 0.0
    c = len(G & S)
    return max(c / len(G), c / len(S))


def update_sets(sets, ids, planes, view_id, thresh=0.5):
    """update_global_3Dplane over sets; planes = [(plane id, set)] ascending.  Returns what happened per plane."""
    events = []
    for pid, S in planes:
        if not S:
            events.append("empty")
            continue
        for g in range(len(sets)):
            if rate(sets[g], S) > thresh:
                sets[g] = sets[g] | S
                ids[g].append((view_id, pid))
                events.append("merge")
                break
        else:
            ids[len(sets)] = [(view_id, pid)]
            sets.append(set(S))
            events.append("new")
    return events


def final_merge_sets(sets, ids, thresh=0.5):
    """final_merge_global_3Dplane over sets -> (new sets, new ids, number of merges)."""
    merged = [False] * len(sets)
    out_sets, out_ids, n_merges = [], {}, 0
    for i in range(len(sets)):
        if merged[i]:
            continue
        cur, cur_ids = set(sets[i]), list(ids[i])
        for j in range(i + 1, len(sets)):
            if merged[j]:
                continue
            if rate(cur, sets[j]) > thresh:
                cur |= sets[j]
                cur_ids.extend(ids[j])
                merged[j] = True
                n_merges += 1
        out_ids[len(out_sets)] = cur_ids
        out_sets.append(cur)
        merged[i] = True
    return out_sets, out_ids, n_merges


def all_planes(points, cams, masks, depth_thresh=0.01, dtype=f32):
    """Per view [(plane id, set)] for EVERY id of the mask, ascending (a mask id without front points gives an empty set)."""
    out = []
    for cam, mask in zip(cams, masks):
        found = dict(local_planes(front_labels(points, cam, mask, depth_thresh, dtype)))
        out.append([(pid, found.get(pid, set())) for pid in mask_plane_ids(mask)])
    return out


def get_global_3Dplane(points, cams, masks, previous=None, thresh=0.5, depth_thresh=0.01, dtype=f32, stats=None):
    """The reference's get_global_3Dplane restated over sets -> (list of sorted index arrays, dict)."""
    planes = all_planes(points, cams, masks, depth_thresh, dtype)
    if previous is None:
        sets = [set(S) for _pid, S in planes[0]]
        ids = {k: [(0, pid)] for k, (pid, _S) in enumerate(planes[0])}
        start = 1
    else:
        ids = {int(k): [(int(v), int(p)) for v, p in pairs] for k, pairs in previous.items()}
        start = max(v for pairs in ids.values() for v, _p in pairs) + 1
        sets = [set().union(*[dict(planes[v]).get(p, set()) for v, p in pairs]) for pairs in ids.values()]
    events = []
    for v in range(start, len(cams)):
        events += update_sets(sets, ids, planes[v], v, thresh)
    sets, ids, n_final = final_merge_sets(sets, ids, thresh)
    if stats is not None:
        stats.update(update_merges=events.count("merge"), new_planes=events.count("new"), empty_planes=events.count("empty"),
                     final_merges=n_final)
    return [np.array(sorted(s), np.int64) for s in sets], ids


def overlap_counts(labels, n_planes, member, block=1 << 16):
    """(sizes [P], counts [P][G]) as Python ints: what SetProvider.view_counts counts, for slot labels [N] (anything outside
    1 .. P is no label) and a membership table bool [G,N], as the matrix product of the one-hot labels and the table.
    float64 sums of 0/1 products are exact far beyond any N; a block of points at a time keeps the one-hot matrix small."""
    labels, member = np.asarray(labels).reshape(-1), np.asarray(member, bool)
    P, (G, N) = int(n_planes), member.shape
    assert labels.shape == (N,)
    sizes, counts = np.zeros(P, np.int64), np.zeros((P, G), np.int64)
    planes = np.arange(1, P + 1)
    for a in range(0, N, block):
        onehot = (labels[None, a:a + block] == planes[:, None]).astype(np.float64)
        sizes += onehot.sum(1).astype(np.int64)
        counts += (onehot @ member[:, a:a + block].T.astype(np.float64)).astype(np.int64)
    return sizes.tolist(), counts.tolist()


def row_overlap_counts(member, row, block=1 << 16):
    """[G] Python ints: |row ∩ h| for every row h of a membership table bool [G,N], as matrix-vector products over blocks
    of points."""
    member = np.asarray(member, bool)
    out = np.zeros(member.shape[0], np.int64)
    for a in range(0, member.shape[1], block):
        part = member[:, a:a + block].astype(np.float64)
        out += (part @ part[row]).astype(np.int64)
    return out.tolist()


class SetProvider:
    """The counts provider of g4splat_amd.planes.merge_global_planes over Python sets: the counts the device would read
    back, from labels of this restatement.  Asserts the two facts."""

    def __init__(self, planes):
        self.planes = planes  # per view [(plane id, set)], every mask id
        self.rows = []

    def view_counts(self, v):
        ids = [pid for pid, _S in self.planes[v]]
        sets = [S for _pid, S in self.planes[v]]
        for a in range(len(sets)):  # fact 1
            for b in range(a + 1, len(sets)):
                assert not (sets[a] & sets[b])
        return ids, [len(S) for S in sets], [[len(S & G) for G in self.rows] for S in sets]

    def assign(self, v, target):
        for (_pid, S), g in zip(self.planes[v], target):
            if g < 0:
                continue
            while len(self.rows) <= g:
                self.rows.append(set())
            before, c = len(self.rows[g]), len(self.rows[g] & S)
            self.rows[g] = self.rows[g] | S
            assert len(self.rows[g]) == before + len(S) - c  # fact 1's size update

    def row_counts(self, g):
        return [len(self.rows[g] & H) for H in self.rows]

    def merge_rows(self, dst, src):
        self.rows[dst] = self.rows[dst] | self.rows[src]

    def row_indices(self, g):
        return np.array(sorted(self.rows[g]), np.int64)


class IndexSetProvider(SetProvider):
    """A provider over hand-made index sets: `init` are the global planes at the start (view 0's planes), `later` the
    local planes of views 1, 2, ... as lists of sets."""

    def __init__(self, init, later):
        super().__init__([[(k + 1, set(S)) for k, S in enumerate(view)] for view in [init] + list(later)])
