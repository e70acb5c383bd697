"""Restatements of the mip-filter contract of include/g4s_optim.h for the tests:

  * `mip_filter_ref`: g4s_mip_filter in float32 numpy, every operation rounded on its own and in the header's order
    (numpy's float32 +, *, / and maximum are correctly rounded and never fused), so the kernel can be held to it bit
    for bit;
  * `activations_mip_ref`: the activations with the filter on and their gradients in closed form, float64.

Camera objects and the [V,16] table: `camera_table`."""
import numpy as np

UNSEEN = np.float32(100000.0)


def camera_table(cameras):
    """[V,16] float32: R row-major (9), T (3), focal_x, focal_y, image_width, image_height."""
    t = np.empty((len(cameras), 16), dtype=np.float32)
    for row, c in zip(t, cameras):
        row[0:9] = np.asarray(c.R, dtype=np.float32).reshape(9)
        row[9:12] = np.asarray(c.T, dtype=np.float32).reshape(3)
        row[12:16] = (c.focal_x, c.focal_y, c.image_width, c.image_height)
    return t


def filter_scale(cameras, filter_variance=0.2):
    """sqrt(filter_variance) / max focal_x, in double, rounded once."""
    return np.float32(float(filter_variance) ** 0.5 / max(float(c.focal_x) for c in cameras))


def view_tests(xyz, cam, znear):
    """One view of the table: (z' [P], seen [P]) in float32, the header's order of operations."""
    f32 = np.float32
    xyz = np.asarray(xyz, dtype=f32)
    c = np.asarray(cam, dtype=f32)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    xc = ((x * c[0] + y * c[3]) + z * c[6]) + c[9]
    yc = ((x * c[1] + y * c[4]) + z * c[7]) + c[10]
    zc = ((x * c[2] + y * c[5]) + z * c[8]) + c[11]
    zp = np.maximum(zc, f32(0.001))
    w, h = c[14], c[15]
    u = (xc / zp) * c[12] + f32(0.5) * w
    v = (yc / zp) * c[13] + f32(0.5) * h
    seen = (zc > f32(znear)) & (u >= f32(-0.15) * w) & (u <= f32(1.15) * w) & (v >= f32(-0.15) * h) & (v <= f32(1.15) * h)
    assert zp.dtype == f32 and u.dtype == f32
    return zp, seen


def mip_filter_ref(xyz, table, znear, scale):
    """-> (mip filter [P] float32, seen-by-any-view [P] bool)."""
    xyz = np.asarray(xyz, dtype=np.float32)
    d = np.full(xyz.shape[0], UNSEEN, dtype=np.float32)
    seen = np.zeros(xyz.shape[0], dtype=bool)
    with np.errstate(all="ignore"):
        for cam in np.asarray(table, dtype=np.float32):
            zp, ok = view_tests(xyz, cam, znear)
            d = np.where(ok, np.minimum(d, zp), d)
            seen |= ok
    far = d[seen].max() if seen.any() else UNSEEN  # nobody sees anything: the documented constant
    d = np.where(d == UNSEEN, far, d)
    out = d * np.float32(scale)
    assert out.dtype == np.float32
    return out, seen


def activations_mip_ref(s, q, o, f, g_scales=None, g_rots=None, g_opac=None):
    """float64: scales [P,2], rotations [P,4], opacity [P,1] with the filter f [P,1] on; with the three cotangents also
    the gradients with respect to s, q, o (the filter has none)."""
    s, q, o, f = (np.asarray(a, dtype=np.float64) for a in (s, q, o, f))
    f = f.reshape(-1, 1)
    e2 = np.exp(s) ** 2
    a = e2 + f * f
    scales = np.sqrt(a)
    coef = np.sqrt((e2[:, 0] * e2[:, 1]) / (a[:, 0] * a[:, 1]))[:, None]
    sg = 1.0 / (1.0 + np.exp(-o.reshape(-1, 1)))
    opac = sg * coef
    norm = np.sqrt((q * q).sum(axis=1, keepdims=True))
    den = np.maximum(norm, 1e-12)
    rots = q / den
    if g_scales is None:
        return scales, rots, opac
    gs, gr, go = (np.asarray(a, dtype=np.float64) for a in (g_scales, g_rots, g_opac))
    go = go.reshape(-1, 1)
    d_s = gs * e2 / scales + go * sg * coef * (f * f) / a
    d_o = go * coef * sg * (1.0 - sg)
    d_q = np.where(norm > 1e-12, (gr - rots * (rots * gr).sum(axis=1, keepdims=True)) / den, gr / 1e-12)
    return (scales, rots, opac), (d_s, d_q, d_o)
