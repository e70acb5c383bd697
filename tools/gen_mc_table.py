"""Generates g4splat_amd/csrc/tsdf/tsdf_mc_table.h, the marching-cubes table of the TSDF mesh extraction (tsdf.hip).

    python tools/gen_mc_table.py            # rewrite the header
    python tools/gen_mc_table.py --check    # exit 1 if the committed header differs

The table is built here from first principles, not copied: for each of the 256 sign configurations the crossing
polygons are found by walking the six cube faces, ambiguous faces are resolved by one fixed rule, the face segments are
chained into closed loops and each loop is fan-triangulated with no diagonal on a cube face.

Conventions (include/g4s_render_maps.h, TSDF section):
  corner c = x | y << 1 | z << 2 at (x, y, z) in {0,1}^3; configuration bit c set <=> tsdf(corner c) < 0 ("inside").
  edge id = 4 * axis + n: the edge along `axis` whose lower corner has the other two coordinates
            (a, b) = (n & 1, n >> 1), in axis order (x: (y, z), y: (x, z), z: (x, y)).
  ambiguous face (two diagonal negative corners): the negative corners are separated (each is cut off by its own
            segment) -- a rule that reads only the face's four signs, so the two cubes sharing a face agree.
  orientation: the triangles' normals (right-hand rule) point towards positive tsdf.
  order: loops by their smallest edge id, walked from it; the fan (v0, v_i, v_i+1) starts at the first vertex of that
         walk whose diagonals v0-v_i all cross the cube's interior (none lies on a face).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "g4splat_amd", "csrc", "tsdf", "tsdf_mc_table.h")


def corner_pos(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_corners(e):
    """(lower corner, upper corner) of edge e."""
    axis, n = divmod(e, 4)
    a, b = n & 1, n >> 1
    others = [ax for ax in range(3) if ax != axis]
    lo = [0, 0, 0]
    lo[others[0]], lo[others[1]] = a, b
    hi = list(lo)
    hi[axis] = 1
    idx = lambda p: p[0] | p[1] << 1 | p[2] << 2
    return idx(lo), idx(hi)


EDGES = [edge_corners(e) for e in range(12)]


def edge_between(c0, c1):
    for e, (a, b) in enumerate(EDGES):
        if {a, b} == {c0, c1}:
            return e
    raise ValueError((c0, c1))


def faces():
    """(outward normal, four corners in cyclic order) of the six faces."""
    out = []
    for axis in range(3):
        for side in (0, 1):
            n = [0, 0, 0]
            n[axis] = 1 if side else -1
            u, v = [ax for ax in range(3) if ax != axis]
            cyc = []
            for (pu, pv) in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0, 0, 0]
                p[axis], p[u], p[v] = side, pu, pv
                cyc.append(p[0] | p[1] << 1 | p[2] << 2)
            out.append((n, cyc))
    return out


def _mid2(e):
    """Twice the midpoint of edge e (integer coordinates)."""
    a, b = (corner_pos(c) for c in EDGES[e])
    return tuple(x + y for x, y in zip(a, b))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def face_segments(neg, normal, cyc):
    """Directed segments (edge p, edge q) of one face for the corner signs `neg` (a set of negative corners)."""
    crossing = [edge_between(cyc[k], cyc[(k + 1) % 4]) for k in range(4)
                if (cyc[k] in neg) != (cyc[(k + 1) % 4] in neg)]
    if not crossing:
        return []
    if len(crossing) == 2:
        pairs = [tuple(crossing)]
    else:  # ambiguous: cut off each negative corner of the face
        pairs = []
        for c in cyc:
            if c in neg:
                pairs.append(tuple(e for e in crossing if c in EDGES[e]))
    segs = []
    for e1, e2 in pairs:
        shared = set(EDGES[e1]) & set(EDGES[e2])
        if shared:
            k = shared.pop()
            ref, ref_neg = k, k in neg
        else:
            ref, ref_neg = next(c for c in cyc if c in neg), True
        p, q = _mid2(e1), _mid2(e2)
        d = tuple(y - x for x, y in zip(p, q))
        side = sum(a * (2 * b - c) for a, b, c in zip(_cross(normal, d), corner_pos(ref), p))
        # n x (q - p) must point to the positive side: a negative reference corner lies on the other side
        if (side < 0) != ref_neg:
            e1, e2 = e2, e1
        segs.append((e1, e2))
    return segs


def config_triangles(cfg):
    neg = {c for c in range(8) if cfg >> c & 1}
    nxt = {}
    for normal, cyc in faces():
        for p, q in face_segments(neg, normal, cyc):
            assert p not in nxt, (cfg, p)
            nxt[p] = q
    assert sorted(nxt) == sorted(nxt.values()), cfg  # every crossing point: one segment in, one out
    tris, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop = [start]
        while nxt[loop[-1]] != start:
            loop.append(nxt[loop[-1]])
        seen.update(loop)
        loop = fan_start(loop)
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


def edge_faces(e):
    """The two cube faces (axis, side) edge e lies on."""
    a, b = (corner_pos(c) for c in EDGES[e])
    return {(ax, a[ax]) for ax in range(3) if a[ax] == b[ax]}


def fan_start(loop):
    """The loop rotated to start at its first vertex whose fan diagonals all cross the cube's interior.  A diagonal
    between two vertices on one face would lie IN that face, and the neighbouring cube, which sees the same face,
    would produce the same flat triangle reversed (two coincident triangles, each edge used twice)."""
    n = len(loop)
    for k in range(n):
        r = loop[k:] + loop[:k]
        if all(not (edge_faces(r[0]) & edge_faces(r[i])) for i in range(2, n - 1)):
            return r
    raise AssertionError(f"no fan start without a diagonal on a face: {loop}")


def table():
    return [config_triangles(cfg) for cfg in range(256)]


def render_header():
    tab = table()
    maxt = max(len(t) for t in tab)
    lines = [
        "// GENERATED by tools/gen_mc_table.py -- do not edit.  Marching-cubes table of the TSDF mesh extraction (tsdf.hip).",
        "// corner c = x | y << 1 | z << 2; configuration bit c set <=> tsdf(corner c) < 0.  edge id = 4 * axis + n, n = a | b << 1",
        "// with (a, b) the lower corner's other two coordinates in axis order.  Ambiguous faces: negative corners separated.",
        "// Triangles point their normals (right-hand rule) towards positive tsdf.",
        "#pragma once",
        "",
        f"#define G4S_MC_MAX_TRIS {maxt}",
        "",
        "static const unsigned char g4s_mc_ntris[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(t)) for t in tab[r:r + 32]) + ",")
    lines += ["};", "", f"static const signed char g4s_mc_tris[256][{3 * maxt}] = {{"]
    for cfg, t in enumerate(tab):
        flat = [e for tri in t for e in tri] + [-1] * (3 * (maxt - len(t)))
        lines.append("    {" + ", ".join(str(e) for e in flat) + "},")
    lines += ["};", ""]
    return "\n".join(lines)


def main(argv):
    text = render_header()
    if "--check" in argv:
        ok = os.path.exists(HEADER) and open(HEADER).read() == text
        print("up to date" if ok else f"{HEADER} differs from the generator")
        return 0 if ok else 1
    with open(HEADER, "w") as f:
        f.write(text)
    print("wrote", HEADER)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
