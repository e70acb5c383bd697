"""Mesh operations without a GPU: the numpy restatement of the header's semantics (tests/mesh_ops_ref.py) on hand-built
meshes and against scipy's connected components, host-side validation of the g4s_mesh_* entry points, and the parts of
g4splat_amd.mesh that are plain host code (join_meshes of numpy meshes, the DeviceMesh type)."""
import ctypes

import numpy as np
import pytest

import mesh_ops_ref as ref
from g4splat_amd import mesh as mesh_mod

TET = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int32)  # a closed tetrahedron on vertices 0..3


def _mesh(tris, n_verts=None, seed=0):
    tris = np.asarray(tris, np.int32).reshape(-1, 3)
    n = int(tris.max()) + 1 if n_verts is None else n_verts
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 3)).astype(np.float32), rng.uniform(0, 1, (n, 3)).astype(np.float32), tris


def _strip(n_tris, first_vertex):
    """A triangle strip of n_tris triangles on vertices first_vertex .. first_vertex + n_tris + 1: one cluster."""
    i = np.arange(n_tris) + first_vertex
    return np.stack([i, i + 1, i + 2], 1).astype(np.int32)


def test_two_tetrahedra_sharing_one_vertex_are_two_clusters():
    second = TET.copy()
    second[second > 0] += 3  # vertices 0, 4, 5, 6: only vertex 0 is shared
    labels, sizes = ref.cluster_connected_triangles(np.concatenate([TET, second]))
    assert labels.tolist() == [0, 0, 0, 0, 4, 4, 4, 4] and sizes.tolist() == [4] * 8


def test_two_tetrahedra_sharing_one_edge_are_one_cluster():
    second = TET.copy()
    second[second > 1] += 2  # vertices 0, 1, 4, 5: edge {0,1} is shared (by four triangles)
    labels, sizes = ref.cluster_connected_triangles(np.concatenate([TET, second]))
    assert (labels == 0).all() and (sizes == 8).all()


def test_fan_of_three_triangles_on_one_edge_is_one_cluster():
    labels, sizes = ref.cluster_connected_triangles([[0, 1, 2], [5, 6, 7], [1, 0, 3], [0, 1, 4]])
    assert labels.tolist() == [0, 1, 0, 0] and sizes.tolist() == [3, 1, 3, 3]


def test_triangle_with_a_repeated_index_owns_its_other_edge():
    # (4,4,5) has the single edge {4,5}: joined to (4,5,6); (7,7,7) has no edge at all
    labels, sizes = ref.cluster_connected_triangles([[0, 1, 2], [4, 4, 5], [4, 5, 6], [7, 7, 7], [9, 8, 9]])
    assert labels.tolist() == [0, 1, 1, 3, 4] and sizes.tolist() == [1, 2, 2, 1, 1]
    assert ref.triangle_edges([9, 8, 9]) == {(8, 9)} and ref.triangle_edges([7, 7, 7]) == set()


def test_labels_do_not_depend_on_the_order_edges_are_met():
    """A long chain whose links arrive in a scrambled order: the label is still the smallest triangle of the chain."""
    rng = np.random.default_rng(5)
    tris = _strip(300, 0)[rng.permutation(300)]
    labels, sizes = ref.cluster_connected_triangles(tris)
    assert (labels == 0).all() and (sizes == 300).all()


def _clusters_of_sizes(sizes):
    parts, first = [], 0
    for n in sizes:
        parts.append(_strip(n, first))
        first += n + 2
    return np.concatenate(parts)


def test_post_process_keeps_all_ties_at_the_kth_size():
    tris = _clusters_of_sizes([80, 60, 70, 60, 60, 55])
    mesh = _mesh(tris)
    v, c, t = ref.post_process_mesh(mesh, cluster_to_keep=3)  # third largest = 60: the three 60s all stay, 55 goes
    assert len(t) == 80 + 60 + 70 + 60 + 60
    assert len(v) == len(t) + 2 * 5 and np.array_equal(np.unique(t), np.arange(len(v)))
    v1, _c1, t1 = ref.post_process_mesh(mesh, cluster_to_keep=1)
    assert len(t1) == 80 and np.array_equal(v1, mesh[0][:82])


def test_post_process_with_fewer_clusters_than_k_uses_the_smallest_size_and_the_floor_of_50():
    mesh = _mesh(_clusters_of_sizes([80, 10, 60, 49, 50]))
    labels, sizes = ref.cluster_connected_triangles(mesh[2])
    assert ref.cluster_threshold(labels, sizes, 1000) == 50  # smallest cluster (10) stands in; the floor lifts it to 50
    assert ref.cluster_threshold(labels, sizes, 5) == 50 and ref.cluster_threshold(labels, sizes, 2) == 60
    _v, _c, t = ref.post_process_mesh(mesh, cluster_to_keep=1000)
    assert len(t) == 80 + 60 + 50  # 49 and 10 fall below the floor, 50 stays (>=)
    big = _mesh(_clusters_of_sizes([80, 70]))
    assert len(ref.post_process_mesh(big, cluster_to_keep=1000)[2]) == 150  # t = max(70, 50)


def test_post_process_order_is_stable_and_vertices_of_degenerate_triangles_remain():
    strip = _strip(60, 0)  # vertices 0..61
    # (30,31,100) hangs on the strip by edge {30,31}; the degenerate (31,100,100) hangs on it by its one edge {31,100};
    # sixty copies of the degenerate (150,151,151) share the edge {150,151}: a cluster of 60 that has no proper triangle
    tris = np.concatenate([strip[:30], [[30, 31, 100]], [[31, 100, 100]], strip[30:], _strip(5, 200),
                           np.tile([[150, 151, 151]], (60, 1))]).astype(np.int32)
    verts, cols, _ = _mesh(tris, n_verts=210)
    labels, sizes = ref.cluster_connected_triangles(tris)
    assert (labels[:62] == 0).all() and (sizes[:62] == 62).all() and (sizes[62:67] == 5).all()
    assert (labels[67:] == 67).all() and (sizes[67:] == 60).all()
    v, c, t = ref.post_process_mesh((verts, cols, tris), cluster_to_keep=2)
    # the small strip is gone with its vertices; every degenerate triangle is gone, but the vertices they named stay:
    # unreferenced vertices are dropped BEFORE degenerate triangles are
    keep_v = np.r_[np.arange(62), 100, 150, 151]
    assert np.array_equal(v, verts[keep_v]) and np.array_equal(c, cols[keep_v])
    expect = np.concatenate([strip[:30], [[30, 31, 62]], strip[30:]])  # vertex 100 is now number 62
    assert np.array_equal(t, expect)
    v1, _c1, t1 = ref.post_process_mesh((verts, cols, tris), cluster_to_keep=1)
    assert np.array_equal(t1, expect) and np.array_equal(v1, verts[keep_v[:63]])


def test_compaction_is_stable_and_marks_out_of_range_indices():
    verts, cols, _ = _mesh([[0, 1, 2]], n_verts=8)
    tris = np.array([[7, 5, 6], [0, 1, 2], [5, 9, 7], [2, 2, 2]], np.int32)
    v, c, t = ref.compact((verts, cols, tris), np.array([1, 0, 1, 1], bool))
    assert np.array_equal(v, verts[[2, 5, 6, 7]]) and np.array_equal(c, cols[[2, 5, 6, 7]])
    assert t.tolist() == [[3, 1, 2], [1, -1, 3], [0, 0, 0]]
    v2, _c2, t2 = ref.compact((verts, cols, tris), None, compact_vertices=False)
    assert v2 is not None and len(v2) == 8 and t2.tolist() == [[7, 5, 6], [0, 1, 2], [5, -1, 7], [2, 2, 2]]


def test_clusters_agree_with_scipy_connected_components():
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    rng = np.random.default_rng(11)
    F = 4000
    tris = rng.integers(0, 300, (F, 3)).astype(np.int32)  # sparse random mesh: many clusters of mixed size
    tris[:50, 1] = tris[:50, 0]                            # some repeated indices
    labels, sizes = ref.cluster_connected_triangles(tris)
    users = {}
    for i, tri in enumerate(tris):
        for e in ref.triangle_edges(tri):
            users.setdefault(e, []).append(i)
    rows, cols = [], []
    for us in users.values():
        for a in us:
            for b in us:
                if a != b:
                    rows.append(a)
                    cols.append(b)
    g = sparse.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(F, F))
    n, comp = connected_components(g, directed=False)
    assert n == len(np.unique(labels)) and 10 < n < F
    # same partition: a bijection between component numbers and labels
    assert len({(int(a), int(b)) for a, b in zip(comp, labels)}) == n
    for l in np.unique(labels):
        members = np.flatnonzero(labels == l)
        assert members[0] == l and (sizes[members] == len(members)).all()


def test_filter_mesh_keeps_an_edge_of_exactly_the_threshold():
    verts = np.array([[0, 0, 0], [0.3, 0, 0], [0, 0.4, 0], [0, 0, 2.0], [9, 9, 9]], np.float32)
    tris = np.array([[0, 1, 2], [0, 1, 3], [1, 2, 0]], np.int32)
    mesh = (verts, np.zeros_like(verts), tris)
    longest = ref.edge_lengths(mesh)[0].max()  # |(0.3,0,0) - (0,0.4,0)| from the float32 coordinates, in float64
    assert longest == np.sqrt(np.float64(np.float32(0.3)) ** 2 + np.float64(np.float32(0.4)) ** 2)
    v, _c, t = ref.filter_mesh(mesh, longest)  # <= keeps the boundary
    assert t.tolist() == [[0, 1, 2], [1, 2, 0]] and len(v) == 3
    assert len(ref.filter_mesh(mesh, np.nextafter(longest, 0))[2]) == 0
    assert len(ref.filter_mesh(mesh, 5.0)[2]) == 3


def _camera(eye, target):
    from g4splat_amd import synthetic
    return synthetic.look_at_camera(eye, target, (0, 1, 0), np.radians(60), 64, 48)


def test_observed_vertices_need_inside_and_close_and_ignore_points_behind():
    cam = _camera((0, 0, -2), (0, 0, 0))
    pts = np.array([[0, 0, 0],      # centre of the image, depth 2
                    [0, 0, 3],      # centre, depth 5
                    [50, 0, 0],     # far outside the image
                    [0, 0, -4],     # behind the camera: w <= 0 is clamped to 1e-6, the quotient is 0/1e-6 = 0 (inside),
                    [1, 1, -4]],    #   depth negative hence "close" -- observed, as in the reference; off-axis: outside
                   np.float32)
    assert ref.observed_vertices(pts, [cam], 3.0).tolist() == [True, False, False, True, False]
    assert ref.observed_vertices(pts, [cam], 6.0).tolist() == [True, True, False, True, False]
    assert not ref.observed_vertices(pts, [], 6.0).any()
    # a second camera that sees (50,0,0)
    cam2 = _camera((50, 0, -2), (50, 0, 0))
    assert ref.observed_vertices(pts, [cam, cam2], 3.0).tolist() == [True, False, True, True, False]
    tris = np.array([[0, 3, 0], [0, 1, 3], [0, 3, 2], [0, 3, 7]], np.int32)
    assert ref.keep_unobserved(tris, ref.observed_vertices(pts, [cam], 3.0)).tolist() == [False, True, True, True]


def test_join_meshes_offsets_indices_and_device_mesh_has_the_same_fields():
    a, b = _mesh(TET, seed=1), _mesh([[0, 1, 2]], seed=2)
    joined = mesh_mod.join_meshes([mesh_mod.TriangleMesh(*a), mesh_mod.TriangleMesh(*b), mesh_mod.TriangleMesh(*a)])
    rv, rc, rt = ref.join_meshes([a, b, a])
    assert isinstance(joined, mesh_mod.TriangleMesh)
    assert np.array_equal(joined.vertices, rv) and np.array_equal(joined.vertex_colors, rc)
    assert np.array_equal(joined.triangles, rt) and joined.triangles.dtype == np.int32
    assert rt[4].tolist() == [4, 5, 6] and rt[5].tolist() == [7, 8, 9]
    assert mesh_mod.DeviceMesh._fields == mesh_mod.TriangleMesh._fields
    with pytest.raises(ValueError):
        mesh_mod.join_meshes([])
    for name in ("cull_observed_faces", "cluster_connected_triangles", "post_process_mesh", "filter_mesh"):
        assert callable(getattr(mesh_mod, name))
    import inspect
    sig = inspect.signature(mesh_mod.GaussianExtractor.extract_mesh_multires)
    assert sig.parameters["multires_factors"].default == (2, 8, 16) and sig.parameters["mesh_res"].default == 1024
    assert inspect.signature(mesh_mod.post_process_mesh).parameters["cluster_to_keep"].default == 1000
    assert inspect.signature(mesh_mod.filter_mesh).parameters["length_threshold"].default == 0.05
    assert inspect.signature(mesh_mod.TSDFVolume.extract_triangle_mesh).parameters["to_host"].default is True


def test_write_triangle_mesh_accepts_tensors(tmp_path):
    import torch
    from g4splat_amd import ply_io
    v, c, t = _mesh(TET, seed=3)
    dm = mesh_mod.DeviceMesh(torch.from_numpy(v), torch.from_numpy(c), torch.from_numpy(t))
    path = str(tmp_path / "m.ply")
    ply_io.write_triangle_mesh(path, dm)
    v2, c2, t2 = ply_io.read_triangle_mesh(path)
    assert np.array_equal(v2, v) and np.array_equal(t2, t) and np.abs(c2 - c).max() <= 0.5 / 255 + 1e-6


def test_mesh_ops_argument_validation_is_host_side(hip_lib):
    """Every g4s_mesh_* entry point rejects bad arguments before it touches the device: negative status + a message."""
    from g4splat_amd import _lib
    lib = hip_lib
    nul = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)   # never dereferenced: validation fails first
    two = ctypes.c_void_p(512)
    BIG = (2 ** 31 - 1) // 3 + 1  # 3 * BIG >= 2^31
    tot = (ctypes.c_int * 2)()

    def expect(rc, text):
        assert rc < 0, rc
        assert text.encode() in lib.g4s_last_error(), lib.g4s_last_error()

    expect(lib.g4s_mesh_observed_vertices(5, nul, 2, one, one, 1.0, one, nul), "NULL required pointer")
    expect(lib.g4s_mesh_observed_vertices(5, one, 2, one, nul, 1.0, one, nul), "NULL required pointer")
    expect(lib.g4s_mesh_observed_vertices(5, one, 2, one, one, 1.0, nul, nul), "NULL required pointer")
    expect(lib.g4s_mesh_observed_vertices(-1, one, 2, one, one, 1.0, one, nul), "must not be negative")
    expect(lib.g4s_mesh_observed_vertices(5, one, -2, one, one, 1.0, one, nul), "must not be negative")
    expect(lib.g4s_mesh_observed_vertices(BIG, one, 2, one, one, 1.0, one, nul), "exceeds 2^31")
    expect(lib.g4s_mesh_observed_vertices(5, one, 2, one, one, float("nan"), one, nul), "NaN")
    assert lib.g4s_mesh_observed_vertices(0, nul, 0, nul, nul, 1.0, nul, nul) == 0

    expect(lib.g4s_mesh_keep_unobserved(5, nul, 5, one, one, nul), "NULL required pointer")
    expect(lib.g4s_mesh_keep_unobserved(5, one, 5, nul, one, nul), "NULL required pointer")
    expect(lib.g4s_mesh_keep_unobserved(5, one, 5, one, nul, nul), "NULL required pointer")
    expect(lib.g4s_mesh_keep_unobserved(-5, one, 5, one, one, nul), "must not be negative")
    expect(lib.g4s_mesh_keep_unobserved(BIG, one, 5, one, one, nul), "exceeds 2^31")

    expect(lib.g4s_mesh_keep_min_size(5, nul, 50, one, nul), "NULL required pointer")
    expect(lib.g4s_mesh_keep_min_size(5, one, 50, nul, nul), "NULL required pointer")
    expect(lib.g4s_mesh_keep_min_size(-1, one, 50, one, nul), "must not be negative")
    expect(lib.g4s_mesh_keep_min_size(BIG, one, 50, one, nul), "exceeds 2^31")

    expect(lib.g4s_mesh_keep_nondegenerate(5, nul, one, nul), "NULL required pointer")
    expect(lib.g4s_mesh_keep_nondegenerate(5, one, nul, nul), "NULL required pointer")
    expect(lib.g4s_mesh_keep_nondegenerate(-1, one, one, nul), "must not be negative")
    expect(lib.g4s_mesh_keep_nondegenerate(BIG, one, one, nul), "exceeds 2^31")

    expect(lib.g4s_mesh_keep_short_edges(5, nul, 5, one, 0.05, one, nul), "NULL required pointer")
    expect(lib.g4s_mesh_keep_short_edges(5, one, 5, nul, 0.05, one, nul), "NULL required pointer")
    expect(lib.g4s_mesh_keep_short_edges(5, one, 5, one, 0.05, nul, nul), "NULL required pointer")
    expect(lib.g4s_mesh_keep_short_edges(5, one, -5, one, 0.05, one, nul), "must not be negative")
    expect(lib.g4s_mesh_keep_short_edges(BIG, one, 5, one, 0.05, one, nul), "exceeds 2^31")
    expect(lib.g4s_mesh_keep_short_edges(5, one, 5, one, float("nan"), one, nul), "NaN")

    cws = lib.g4s_mesh_cluster_workspace(1000)
    assert cws >= 6 * 1000 * 12 + 2 * 1000 * 4
    expect(lib.g4s_mesh_cluster_triangles(1000, nul, one, one, one, cws, nul), "NULL required pointer")
    expect(lib.g4s_mesh_cluster_triangles(1000, one, nul, one, one, cws, nul), "NULL required pointer")
    expect(lib.g4s_mesh_cluster_triangles(1000, one, one, nul, one, cws, nul), "NULL required pointer")
    expect(lib.g4s_mesh_cluster_triangles(-1, one, one, one, one, cws, nul), "must not be negative")
    expect(lib.g4s_mesh_cluster_triangles(BIG, one, one, one, one, 1 << 40, nul), "exceeds 2^31")
    expect(lib.g4s_mesh_cluster_triangles(1000, one, one, one, one, cws - 1, nul), "workspace too small")
    expect(lib.g4s_mesh_cluster_triangles(1000, one, one, one, nul, cws, nul), "workspace too small")
    assert lib.g4s_mesh_cluster_triangles(0, nul, nul, nul, nul, 0, nul) == 0

    pws = lib.g4s_mesh_compact_workspace(500, 1000)
    assert pws >= 2 * 1000 * 4 + 2 * 500 * 4
    expect(lib.g4s_mesh_compact_count(500, 1000, nul, one, 1, tot, one, pws, nul), "NULL required pointer")
    expect(lib.g4s_mesh_compact_count(500, 1000, one, one, 1, None, one, pws, nul), "NULL required pointer")
    expect(lib.g4s_mesh_compact_count(-1, 1000, one, one, 1, tot, one, pws, nul), "must not be negative")
    expect(lib.g4s_mesh_compact_count(500, -1, one, one, 1, tot, one, pws, nul), "must not be negative")
    expect(lib.g4s_mesh_compact_count(500, BIG, one, one, 1, tot, one, 1 << 40, nul), "exceeds 2^31")
    expect(lib.g4s_mesh_compact_count(500, 1000, one, one, 1, tot, one, pws - 1, nul), "workspace too small")
    expect(lib.g4s_mesh_compact_count(500, 1000, one, one, 1, tot, nul, pws, nul), "workspace too small")

    def emit(V=500, F=1000, v=one, c=one, t=one, cv=1, vo=two, co=two, to=two, Vo=10, Fo=10, w=one, wsb=pws):
        return lib.g4s_mesh_compact_emit(V, F, v, c, t, cv, vo, co, to, Vo, Fo, w, wsb, nul)
    expect(emit(t=nul), "NULL required pointer")
    expect(emit(to=nul), "NULL required pointer")
    expect(emit(v=nul), "NULL required pointer")
    expect(emit(vo=nul), "NULL required pointer")
    expect(emit(co=nul), "go together")
    expect(emit(V=-1), "must not be negative")
    expect(emit(F=BIG, wsb=1 << 40), "exceeds 2^31")
    expect(emit(Vo=501), "output counts")
    expect(emit(Fo=-1), "output counts")
    expect(emit(to=one), "must not alias")
    expect(emit(vo=one), "must not alias")
    expect(emit(wsb=pws - 1), "workspace too small")
    expect(emit(w=nul), "workspace too small")
    assert _lib.last_error() != ""
    assert lib.g4s_mesh_keep_nondegenerate(0, nul, nul, nul) == 0 and _lib.last_error() == ""  # a good call clears it


def test_mesh_arguments_are_checked_before_the_device():
    import torch
    host = mesh_mod.TriangleMesh(np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32))
    on_cpu = mesh_mod.DeviceMesh(torch.zeros((3, 3)), torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32))
    for op in (mesh_mod.cluster_connected_triangles, mesh_mod.post_process_mesh, mesh_mod.filter_mesh,
               lambda m: mesh_mod.cull_observed_faces(m, [], 1.0)):
        with pytest.raises(RuntimeError, match="a DeviceMesh lives on one HIP device"):
            op(on_cpu)
    with pytest.raises(RuntimeError, match=r"vertex_colors \(2, 3\) must match vertices \(3, 3\)"):
        mesh_mod.as_device_mesh(host._replace(vertex_colors=np.zeros((2, 3), np.float32)), "cpu")
    with pytest.raises(ValueError, match="cluster_to_keep must be at least 1"):
        mesh_mod.post_process_mesh(host, 0)
    with pytest.raises(ValueError, match="at least one mesh"):
        mesh_mod.join_meshes([])
    with pytest.raises(TypeError, match="meshes of one kind"):
        mesh_mod.join_meshes([host, on_cpu])
    with pytest.raises(ValueError, match="quantile of an empty tensor"):
        mesh_mod.quantile_linear(torch.zeros(0), 0.5)
