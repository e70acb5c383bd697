"""Numpy restatement of the mesh operations of include/g4s_render_maps.h ("mesh operations" section): the yardstick of
tests/test_mesh_ops_cpu.py and tests/test_gpu_mesh_ops.py.  Written from the header's wording, kept obviously right
rather than fast: a dict of edge -> triangles and a union-find for the clusters, float32 expressions in the header's
order for the observed-vertex test."""
import numpy as np

f32 = np.float32


def _col(p, M, k):
    """col_k(M) of the header: ((x*M[0][k] + y*M[1][k]) + z*M[2][k]) + M[3][k], float32 throughout."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return ((x * M[0, k] + y * M[1, k]) + z * M[2, k]) + M[3, k]


def observed_vertices(vertices, cameras, near_trunc):
    """bool [V]: inside some camera's image and nearer to it than near_trunc.  cameras: objects with
    world_view_transform / full_proj_transform (4x4, row-vector convention)."""
    p = np.ascontiguousarray(vertices, f32).reshape(-1, 3)
    obs = np.zeros(len(p), bool)
    near = f32(near_trunc)
    for cam in cameras:
        W = np.asarray(cam.world_view_transform, f32).reshape(4, 4)
        P = np.asarray(cam.full_proj_transform, f32).reshape(4, 4)
        hx, hy, hw = _col(p, P, 0), _col(p, P, 1), _col(p, P, 3)
        w = np.where(hw > f32(1e-6), hw, f32(1e-6)).astype(f32)
        with np.errstate(all="ignore"):
            inside = (np.abs(hx / w) < f32(1)) & (np.abs(hy / w) < f32(1))
        obs |= inside & (_col(p, W, 2) < near)
    return obs


def keep_unobserved(triangles, observed):
    """bool [F]: False where all three vertices are observed (an index outside [0, V) counts as unobserved)."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    V = len(observed)
    ok = (t >= 0) & (t < V)
    o = np.zeros(t.shape, bool)
    o[ok] = np.asarray(observed, bool)[t[ok]]
    return ~o.all(1)


def compact(mesh, keep=None, compact_vertices=True):
    """(vertices, colours, triangles) after dropping the triangles with keep False and -- compact_vertices -- the
    vertices no surviving triangle names; order preserved; an out-of-range index becomes -1."""
    v, c, t = (np.asarray(mesh[0], f32).reshape(-1, 3), np.asarray(mesh[1], f32).reshape(-1, 3),
               np.asarray(mesh[2], np.int32).reshape(-1, 3))
    if keep is not None:
        t = t[np.asarray(keep, bool)]
    V = len(v)
    ok = (t >= 0) & (t < V)
    if not compact_vertices:
        return v, c, np.where(ok, t, -1).astype(np.int32)
    used = np.zeros(V, bool)
    used[t[ok]] = True
    new = (np.cumsum(used) - 1).astype(np.int32)
    out = np.full(t.shape, -1, np.int32)
    out[ok] = new[t[ok]]
    return v[used], c[used], out


def cull_observed_faces(mesh, cameras, near_trunc):
    keep = keep_unobserved(mesh[2], observed_vertices(mesh[0], cameras, near_trunc))
    return compact(mesh, keep)


def join_meshes(meshes):
    offs = np.cumsum([0] + [len(m[0]) for m in meshes[:-1]])
    return (np.concatenate([np.asarray(m[0], f32).reshape(-1, 3) for m in meshes]),
            np.concatenate([np.asarray(m[1], f32).reshape(-1, 3) for m in meshes]),
            np.concatenate([np.asarray(m[2], np.int32).reshape(-1, 3) + np.int32(o) for m, o in zip(meshes, offs)]))


def triangle_edges(tri):
    """The undirected edges {a,b}, a != b, of one triangle, as sorted tuples (a set: a repeated edge counts once)."""
    a, b, c = (int(x) for x in tri)
    return {(min(u, w), max(u, w)) for u, w in ((a, b), (b, c), (c, a)) if u != w}


def cluster_connected_triangles(triangles):
    """(labels [F], sizes [F]) int32: smallest triangle index of the edge-connected cluster, and its triangle count."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    F = len(t)
    users = {}
    for i in range(F):
        for e in triangle_edges(t[i]):
            users.setdefault(e, []).append(i)
    parent = list(range(F))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for tris in users.values():
        for other in tris[1:]:
            a, b = find(tris[0]), find(other)
            if a != b:
                parent[max(a, b)] = min(a, b)
    labels = np.array([find(i) for i in range(F)], np.int32).reshape(F)
    assert all(labels[l] == l for l in labels)  # a label is the smallest member: its own label
    sizes = np.bincount(labels, minlength=max(F, 1))[labels].astype(np.int32) if F else np.zeros(0, np.int32)
    return labels, sizes


def cluster_threshold(labels, sizes, cluster_to_keep):
    """t = max(k-th largest cluster size, 50); with fewer than k clusters the smallest size stands in."""
    roots = labels == np.arange(len(labels))
    s = np.sort(sizes[roots])[::-1]
    kth = s[min(cluster_to_keep, len(s)) - 1]
    return max(int(kth), 50)


def post_process_mesh(mesh, cluster_to_keep=1000):
    t = np.asarray(mesh[2], np.int32).reshape(-1, 3)
    if len(t) == 0:
        return compact(mesh)
    labels, sizes = cluster_connected_triangles(t)
    kept = compact(mesh, sizes >= cluster_threshold(labels, sizes, cluster_to_keep))
    t = kept[2]
    nondegenerate = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    return compact(kept, nondegenerate, compact_vertices=False)


def edge_lengths(mesh):
    """[F,3] float64: |ab|, |bc|, |ca| as the header evaluates them."""
    v = np.asarray(mesh[0], f32).reshape(-1, 3).astype(np.float64)
    t = np.asarray(mesh[2], np.int64).reshape(-1, 3)
    ok = ((t >= 0) & (t < len(v))).all(1)  # a triangle with an index outside [0, V) fails the test: NaN length
    out = np.full((len(t), 3), np.nan, np.float64)
    for k in range(3):
        d = v[t[ok, k]] - v[t[ok, (k + 1) % 3]]
        out[ok, k] = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return out


def filter_mesh(mesh, length_threshold=0.05):
    return compact(mesh, (edge_lengths(mesh) <= np.float64(length_threshold)).all(1))
