"""The marching-cubes cases of tests/mc_cases.py, checked on the numpy restatement alone: each case contains what it is
meant to put in front of the HIP kernels (tests/test_gpu_mc_cases.py) -- every cube configuration, invalid cubes, unused
crossings, every adjacency class, far keys that do not interact, counts on both sides of the scan's chunk boundary."""
import itertools

import numpy as np
import pytest

import mc_cases
import tsdf_ref
import unbounded_ref as ur

_MESH = {}


def _case(name):
    if name not in _MESH:
        case = mc_cases.SPARSE[name]()
        _MESH[name] = (case, tsdf_ref.extract_mesh(*case))
    return _MESH[name]


def _ntris():
    return np.array([len(t) for t in tsdf_ref.mc_table()])


@pytest.mark.parametrize("name", ["noise", "noise_holes", "exact_zeros"])
def test_valid_cubes_cover_all_256_configurations(name):
    (keys, tsdf, weight, _c, _v), _mesh = _case(name)
    valid, cfg, _mixed = tsdf_ref.cube_cases(keys, tsdf, weight)
    hist = np.bincount(cfg[valid], minlength=256)
    assert (hist > 0).all(), np.nonzero(hist == 0)[0]


def test_cube_cases_agree_with_the_extracted_triangles():
    """The exposed per-cube configuration is the one extract_mesh triangulates: the table's triangle counts add up."""
    for name in ("noise", "noise_holes", "single"):
        (keys, tsdf, weight, _c, _v), (_verts, _cols, tris) = _case(name)
        valid, cfg, mixed = tsdf_ref.cube_cases(keys, tsdf, weight)
        assert _ntris()[cfg[valid]].sum() == len(tris)
        assert (mixed[valid] == ((cfg[valid] != 0) & (cfg[valid] != 255))).all()


def test_noise_with_holes_has_invalid_cubes_and_unused_crossings():
    (keys, tsdf, weight, _c, _v), _mesh = _case("noise_holes")
    assert 0.08 < (weight == 0).mean() < 0.12
    assert np.isnan(tsdf[weight == 0]).all() and np.isfinite(tsdf[weight > 0]).all()
    valid, _cfg, mixed = tsdf_ref.cube_cases(keys, tsdf, weight)
    assert (mixed & ~valid).sum() >= 0.20 * mixed.sum(), ((mixed & ~valid).sum(), mixed.sum())
    assert tsdf_ref.unused_crossings(keys, tsdf, weight) >= 50
    # with every weight positive every crossing inside the block set is used by a cube, except on its outer faces
    zk, zt, zw, _zc, _zv = _case("holes_zero_block")[0]
    (b,) = np.nonzero((tsdf_ref.unpack_keys(zk) == 0).all(1))[0]
    assert (zw[b] == 0).all() and np.isfinite(zt[b]).any() and np.array_equal(zk, keys)
    zvalid, _c2, _m2 = tsdf_ref.cube_cases(zk, zt, zw)
    assert not zvalid[b].any() and zvalid.sum() < valid.sum() - valid[b].sum()  # the neighbours' cubes that touch it too


def _neighbour_offsets(coords):
    have = {tuple(c) for c in coords}
    offs = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]
    return {c: {d for d in offs if tuple(np.add(c, d)) in have} for c in have}


def _components(nbrs):
    seen, comps = set(), []
    for c in sorted(nbrs):
        if c in seen:
            continue
        comp, todo = set(), [c]
        while todo:
            b = todo.pop()
            if b in comp:
                continue
            comp.add(b)
            todo += [tuple(np.add(b, d)) for d in nbrs[b]]
        seen |= comp
        comps.append(sorted(comp))
    return comps


def test_gaps_contain_every_adjacency_class():
    keys = _case("gaps")[0][0]
    nbrs = _neighbour_offsets(tsdf_ref.unpack_keys(keys))
    comps = _components(nbrs)
    nonzero = lambda d: sum(x != 0 for x in d)
    pairs = {nonzero(np.subtract(c[1], c[0])) for c in comps if len(c) == 2}
    assert pairs == {1, 2, 3}                       # a pair sharing a face, one sharing an edge only, one a corner only
    assert any(len(c) == 1 for c in comps)          # an isolated block
    # an L: three blocks, two face contacts through one block, the two ends touching along an edge
    assert any(len(c) == 3 and sorted(nonzero(np.subtract(a, b)) for a, b in itertools.combinations(c, 2)) == [1, 1, 2]
               for c in comps)
    minus = {(-1, 0, 0), (0, -1, 0), (0, 0, -1)}
    plus = {(1, 0, 0), (0, 1, 0), (0, 0, 1)}
    assert any(s == minus for s in nbrs.values()) and any(s == plus for s in nbrs.values())
    # the groups do not interact: the components are the groups
    assert sorted(comps) == sorted(sorted(g) for g in mc_cases.GAP_GROUPS.values())


@pytest.mark.parametrize("name", ["noise", "noise_holes", "gaps", "exact_zeros", "subnormals", "single", "far_keys",
                                  "holes_zero_block", "single_holes"])
def test_reference_meshes_are_indexed_without_waste_or_repeats(name):
    case, (verts, cols, tris) = _case(name)
    assert len(tris) > 100
    assert len(np.unique(tris)) == len(verts)  # no unreferenced vertex
    assert max(tsdf_ref.edge_use(tris).values()) == 1  # no directed edge twice
    assert np.isfinite(verts).all() and np.isfinite(cols).all()
    if name != "far_keys":
        assert np.abs(verts).max() < 4.0


def test_exact_zeros_and_subnormals_are_in_the_crossings():
    keys, tsdf, weight, color, v = _case("exact_zeros")[0]
    assert 0.03 < (np.signbit(tsdf) & (tsdf == 0)).mean() < 0.07 and 0.03 < (~np.signbit(tsdf) & (tsdf == 0)).mean() < 0.07
    verts = _case("exact_zeros")[1][0]
    frac = verts / np.float32(v) - np.float32(0.5)
    assert ((frac == np.round(frac)).all(1)).sum() > 100  # vertices at voxel centres: e = 0 or 1
    keys, tsdf, weight, color, v = _case("subnormals")[0]
    tiny = np.finfo(np.float32).tiny
    sub = (np.abs(tsdf) < tiny) & (tsdf != 0)
    assert 0.03 < sub.mean() < 0.07 and (tsdf[sub] < 0).any() and (tsdf[sub] > 0).any()
    # an edge between two subnormals of opposite sign: e = 1e-40 / 2e-40, a division of subnormals
    flat = tsdf.reshape(-1, 8, 8, 8)  # [block, z, y, x]
    both = sub.reshape(flat.shape)[..., :-1] & sub.reshape(flat.shape)[..., 1:] & ((flat[..., :-1] < 0) != (flat[..., 1:] < 0))
    assert both.sum() >= 3


def test_single_block_has_only_interior_cubes():
    (keys, tsdf, weight, _c, _v), (verts, _cols, _tris) = _case("single")
    valid, _cfg, _mixed = tsdf_ref.cube_cases(keys, tsdf, weight)
    lane = np.arange(512)
    interior = ((lane & 7) < 7) & (((lane >> 3) & 7) < 7) & ((lane >> 6) < 7)
    assert np.array_equal(valid[0], interior)
    g = verts / np.float32(0.1) - np.float32(0.5)  # voxel units; the block spans (0, -8, 0) .. (7, -1, 7)
    lo, hi = np.array([0, -8, 0], np.float32), np.array([7, -1, 7], np.float32)
    assert (g >= lo).all() and (g <= hi).all()
    # with every weight positive each crossing inside the block lies in an interior cube: only holes leave one unused
    assert tsdf_ref.unused_crossings(keys, tsdf, weight) == 0
    hk, ht, hw, _hc, _hv = _case("single_holes")[0]
    assert tsdf_ref.unused_crossings(hk, ht, hw) >= 10


def test_many_blocks_have_counts_on_both_sides_of_the_scan_chunk():
    full = mc_cases.many_blocks(1025)
    assert len(full[0]) == 1025 and len(np.unique(full[0])) == 1025 and (np.diff(full[0]) > 0).all()
    for n in (1023, 1024, 1025):
        (keys, tsdf, weight, _c, v), (verts, _cols, tris) = _case(f"many_{n}")
        assert len(keys) == n and np.array_equal(keys, full[0][:n]) and np.array_equal(tsdf, full[1][:n])
        assert len(tris) > 0 and np.abs(verts).max() < 4.0
        valid, cfg, _m = tsdf_ref.cube_cases(keys, tsdf, weight)
        per_block = (_ntris()[cfg] * valid).sum(1)
        assert per_block.sum() == len(tris)
        assert per_block[0] > 0 and per_block[1022] > 0
        if n > 1024:
            assert per_block[1023] > 0 and per_block[1024] > 0  # triangles owned on both sides of position 1024
        assert (per_block > 0).sum() < 80  # the restatement's triangle loop stays short


def test_far_key_clusters_do_not_interact():
    (keys, tsdf, weight, color, v), (verts, cols, tris) = _case("far_keys")
    coords = tsdf_ref.unpack_keys(keys)
    assert coords.min() == -mc_cases.LIM and coords.max() == mc_cases.LIM - 1
    assert np.array_equal(tsdf_ref.pack_keys(coords), keys)
    # the aliasing pairs: the key one step beyond the field's end is the other block's key
    wrap = lambda b: ((b[0] + mc_cases.LIM) << 42) + ((b[1] + mc_cases.LIM) << 21) + (b[2] + mc_cases.LIM)
    assert wrap((0, mc_cases.LIM, 0)) == tsdf_ref.pack_keys([(1, -mc_cases.LIM, 0)])[0]
    assert wrap((0, 0, mc_cases.LIM)) == tsdf_ref.pack_keys([(0, 1, -mc_cases.LIM)])[0]
    want_t, counts, first, v0 = [], [], 0, 0
    for cluster in mc_cases.FAR_CLUSTERS:
        n = len(cluster)
        assert [tuple(c) for c in coords[first:first + n]] == cluster
        base = coords[first:first + n].min(0)
        local = tsdf_ref.pack_keys(coords[first:first + n] - base)  # the cluster alone, translated to the origin
        assert (np.diff(local) > 0).all()
        lv, lc, lt = tsdf_ref.extract_mesh(local, tsdf[first:first + n], weight[first:first + n], color[first:first + n], v)
        assert len(lt) > 100
        want_t.append(lt + v0)
        counts.append(len(lv))
        part = verts[v0:v0 + len(lv)]
        shift = (base * 8).astype(np.float64) * float(np.float32(v))
        bar = 4 * np.spacing(np.abs(part).max().astype(np.float32)) + 1e-6  # two roundings at the far magnitude
        assert np.abs(part.astype(np.float64) - (lv.astype(np.float64) + shift)).max() <= bar
        assert np.array_equal(cols[v0:v0 + len(lv)], lc)
        first, v0 = first + n, v0 + len(lv)
    assert v0 == len(verts) and np.array_equal(tris, np.concatenate(want_t)) and tris.dtype == np.int32
    # no triangle references a vertex of another cluster
    owner = np.searchsorted(np.cumsum(counts), tris, side="right")
    assert (owner == owner[:, :1]).all() and len(np.unique(owner)) == len(mc_cases.FAR_CLUSTERS)


@pytest.mark.parametrize("name", ["noise_17", "noise_33"])
def test_dense_noise_covers_all_256_configurations(name):
    field, N = mc_cases.DENSE[name]()
    neg = (field < 0).reshape(N, N, N)
    cfg = np.zeros((N - 1,) * 3, np.int64)
    for c in range(8):
        ox, oy, oz = c & 1, (c >> 1) & 1, c >> 2
        cfg |= neg[oz:N - 1 + oz, oy:N - 1 + oy, ox:N - 1 + ox].astype(np.int64) << c
    assert (np.bincount(cfg.reshape(-1), minlength=256) > 0).all()


def test_dense_scan_case_has_counts_on_both_sides_of_the_chunk():
    field, N = mc_cases.DENSE["scan_65"]()
    G = mc_cases.DENSE_GROUP
    groups = (N ** 3 + G - 1) // G
    assert groups == 1073 and N ** 3 % G != 0
    neg = np.pad(field < 0, (0, groups * G - N ** 3)).reshape(groups, G)
    idx = np.arange(groups * G).reshape(groups, G)
    i_ok = (idx % N < N - 1) & (idx < N ** 3 - 1)
    nxt = np.pad(field < 0, (0, groups * G - N ** 3 + 1))[1:].reshape(groups, G)
    nv_x = ((neg != nxt) & i_ok).sum(1)  # +x vertices owned per workgroup: a lower bound of its vertex count
    assert nv_x[:4].min() > 0 and nv_x[1022:1026].min() > 0 and nv_x[1040:1056].min() > 0  # plane k = 63
    assert (nv_x[100:1000] == 0).all()  # the restatement's loop stays short
    verts, tris = ur.dense_cubes(field, N, mc_cases.DENSE_R, (0.0, 0.0, 0.0), 1.0)
    assert 1000 < len(tris) < 40000 and np.abs(verts).max() < 4.0


def test_dense_zero_lattice_holds_signed_zeros_and_subnormals():
    field, N = mc_cases.DENSE["zeros_17"]()
    tiny = np.finfo(np.float32).tiny
    assert ((field == 0) & np.signbit(field)).sum() > 100 and ((field == 0) & ~np.signbit(field)).sum() > 100
    sub = (field != 0) & (np.abs(field) < tiny)
    assert (field[sub] < 0).sum() > 50 and (field[sub] > 0).sum() > 50
    verts, tris = ur.dense_cubes(field, N, mc_cases.DENSE_R, (0.0, 0.0, 0.0), 1.0)
    assert np.isfinite(verts).all() and len(tris) > 1000
