// The depth, normal and curvature terms of MAtCha's chart alignment (include/g4s_losses.h, "Chart alignment losses":
// g4s_chart_align_*), kernels and entry points.
//
// Reference semantics: ParallelAligner.loss and the gradient, normal and curvature terms of ParallelAligner.optimize
// (matcha/dm_scene/parallel_aligner.py:422-458, 713-722, 757-788) with depth2normal_parallel and normal2curv_parallel
// (matcha/dm_utils/rendering.py:249-322, 409-436) and img_grad (matcha/dm_utils/image.py:4-9), which back-project all n
// charts, slice, cross, normalise, pad and difference [n,H,W,3] tensors and keep every one of them for autograd.
//
// MI355X design: a short chain of kernels, one thread per pixel, 256 consecutive pixels of ONE view per block (the camera
// record and the view's depth map are kernel parameters of their own, const and __restrict__, so the record is read through
// a uniform address).  A stencil reads its neighbours straight from global memory: a block's rows are shared with the blocks
// before and behind it through L2, and nothing is staged in LDS.  The normals, and in the backward the adjoints A and B of
// the two point differences, pass through [n,H,W,3] buffers of the workspace, because the backward's depth footprint has
// radius 4 and recomputing it per pixel would cost more than the three passes do.  Every step of the backward is a gather
// from a fixed neighbourhood: no atomics, no fixed-point sums, no range limit.
//   forward:  normals -> terms + per-block partials in double -> one block folds the partials     (3 launches; 2 without
//             the normal and curvature terms)
//   backward: normals -> A, B of every interior pixel -> gather into dL/ddepths, dL/dconfidence   (3 launches; 1 without
//             the normal and curvature terms)
#include "g4s_internal.h"
#include "fixed_sums.h"
#include "chart_common.h"
#include "../../include/g4s_losses.h"

namespace g4s {

constexpr int CA_CAM_FLOATS = 12;     // o[3], D[3][3]
constexpr float CA_NORM_EPS = 1e-12f;  // F.normalize's eps

struct AlignArgs {
    int n, H, W, N;     // N = H W
    int bpv, nblocks;   // blocks per view, n * bpv
    int flags;
    float lambda;
    const float *ref, *conf, *mask, *depths0, *gmask, *normals0, *curv0;
    float *nrm, *A, *B;  // [n,H,W,3] each (workspace)
    double* partials;    // [nblocks][4]
    float* out4;
    const float* g4;
    float *d_depths, *d_conf;
};

// The view and the pixel of a thread: block b of the grid owns pixels 256 (b % bpv) .. + 255 of view b / bpv.
struct Pix {
    int v, p, y, x;
    bool valid;
};
__device__ __forceinline__ Pix ca_pixel(const AlignArgs& a) {
    Pix o;
    o.v = (int)blockIdx.x / a.bpv;
    o.p = ((int)blockIdx.x % a.bpv) * 256 + (int)threadIdx.x;
    o.valid = o.p < a.N;
    o.y = o.p / a.W;
    o.x = o.p % a.W;
    return o;
}

// dir = D (x, y, 1) of pixel (x, y) under the record c
__device__ __forceinline__ void ca_dir(const float* __restrict__ c, int y, int x, float dir[3]) {
    const float fx = (float)x, fy = (float)y;
#pragma unroll
    for (int k = 0; k < 3; k++) dir[k] = (c[3 + 3 * k] * fx + c[4 + 3 * k] * fy) + c[5 + 3 * k];
}
// a = q(y+1,x) - q(y-1,x), b = q(y,x+1) - q(y,x-1), cr = a x b, L = |cr| of an INTERIOR pixel; Dv: the view's depth map.
// The two differences are not formed from the points: q = d dir + o is of the scene's size and the difference of two
// neighbours a fraction of a pixel's footprint, so the subtraction would keep the points' rounding and lose four to five
// bits.  With dir(y+1,x) - dir(y-1,x) = 2 D[.][1] and dir(y,x+1) - dir(y,x-1) = 2 D[.][0], both exact,
//   a = (d_below - d_above) dir(y+1,x) + d_above (2 D[.][1]),   b = (d_right - d_left) dir(y,x+1) + d_left (2 D[.][0])
// are the same differences with the rounding of their own size.
__device__ __forceinline__ float ca_cross(const float* __restrict__ c, const float* __restrict__ Dv, int W, int y, int x,
                                          float a[3], float b[3], float cr[3]) {
    const int p = y * W + x;
    const float du = Dv[p - W], dd = Dv[p + W], dl = Dv[p - 1], dr = Dv[p + 1];
    float dirb[3], dirr[3];
    ca_dir(c, y + 1, x, dirb);
    ca_dir(c, y, x + 1, dirr);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a[k] = (dd - du) * dirb[k] + du * (c[4 + 3 * k] + c[4 + 3 * k]);
        b[k] = (dr - dl) * dirr[k] + dl * (c[3 + 3 * k] + c[3 + 3 * k]);
    }
    cr[0] = a[1] * b[2] - a[2] * b[1];
    cr[1] = a[2] * b[0] - a[0] * b[2];
    cr[2] = a[0] * b[1] - a[1] * b[0];
    return sqrtf((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]);
}
__device__ __forceinline__ bool ca_interior(int H, int W, int y, int x) { return y >= 1 && y <= H - 2 && x >= 1 && x <= W - 2; }

__device__ __forceinline__ void ca_normal(const float* __restrict__ c, const float* __restrict__ Dv, int H, int W, int y, int x,
                                          float nu[3]) {
    nu[0] = nu[1] = nu[2] = 0.0f;
    if (!ca_interior(H, W, y, x)) return;
    float a[3], b[3], cr[3];
    const float L = ca_cross(c, Dv, W, y, x, a, b, cr);
    const float den = L < CA_NORM_EPS ? CA_NORM_EPS : L;  // clamp_min: a NaN stays
#pragma unroll
    for (int k = 0; k < 3; k++) nu[k] = cr[k] / den;
}

// The normal of pixel (y, x): read from the view's [H,W,3] map, or (FROM_DEPTH) formed on the spot.
template <bool FROM_DEPTH>
__device__ __forceinline__ void ca_get_normal(const float* __restrict__ c, const float* __restrict__ Dv, const float* __restrict__ Nv,
                                              int H, int W, int y, int x, float nu[3]) {
    if (FROM_DEPTH) {
        ca_normal(c, Dv, H, W, y, x, nu);
    } else {
        const float* s = Nv + 3 * (y * W + x);
        nu[0] = s[0]; nu[1] = s[1]; nu[2] = s[2];
    }
}
// lap_c = (((n_u - n_p) + (n_l - n_p)) + (n_b - n_p)) + (n_r - n_p), replicate padding; returns curv = sum_c |lap_c|
template <bool FROM_DEPTH>
__device__ __forceinline__ float ca_lap(const float* __restrict__ c, const float* __restrict__ Dv, const float* __restrict__ Nv,
                                        int H, int W, int y, int x, float lap[3]) {
    float p[3], u[3], l[3], b[3], r[3];
    ca_get_normal<FROM_DEPTH>(c, Dv, Nv, H, W, y, x, p);
    ca_get_normal<FROM_DEPTH>(c, Dv, Nv, H, W, clampi(y - 1, H - 1), x, u);
    ca_get_normal<FROM_DEPTH>(c, Dv, Nv, H, W, y, clampi(x - 1, W - 1), l);
    ca_get_normal<FROM_DEPTH>(c, Dv, Nv, H, W, clampi(y + 1, H - 1), x, b);
    ca_get_normal<FROM_DEPTH>(c, Dv, Nv, H, W, y, clampi(x + 1, W - 1), r);
#pragma unroll
    for (int k = 0; k < 3; k++) lap[k] = (((u[k] - p[k]) + (l[k] - p[k])) + (b[k] - p[k])) + (r[k] - p[k]);
    return (fabsf(lap[0]) + fabsf(lap[1])) + fabsf(lap[2]);
}

// grid n * bpv; out [n,H,W,3]
__global__ void __launch_bounds__(256) chart_align_normals_kernel(AlignArgs a, const float* __restrict__ cams,
        const float* __restrict__ depths, float* __restrict__ out) {
    const Pix t = ca_pixel(a);
    if (!t.valid) return;
    float nu[3];
    ca_normal(cams + t.v * CA_CAM_FLOATS, depths + (size_t)t.v * a.N, a.H, a.W, t.y, t.x, nu);
    float* o = out + 3 * ((size_t)t.v * a.N + t.p);
    o[0] = nu[0]; o[1] = nu[1]; o[2] = nu[2];
}

// out [n,H,W]; FROM_DEPTH: cams and depths are read and normals is not
template <bool FROM_DEPTH>
__global__ void __launch_bounds__(256) chart_align_curv_kernel(AlignArgs a, const float* __restrict__ cams,
        const float* __restrict__ depths, const float* __restrict__ normals, float* __restrict__ out) {
    const Pix t = ca_pixel(a);
    if (!t.valid) return;
    float lap[3];
    out[(size_t)t.v * a.N + t.p] = ca_lap<FROM_DEPTH>(FROM_DEPTH ? cams + t.v * CA_CAM_FLOATS : nullptr,
                                                       FROM_DEPTH ? depths + (size_t)t.v * a.N : nullptr,
                                                       FROM_DEPTH ? nullptr : normals + 3 * (size_t)t.v * a.N, a.H, a.W, t.y, t.x, lap);
}

// |gm t| of the row (DY = 1) or column (DY = 0) difference based at (y, x); sg: its derivative gm sign(gm t)
template <int DY>
__device__ __forceinline__ float ca_grad_term(const AlignArgs& a, const float* __restrict__ Dv, const float* __restrict__ D0v,
                                              const float* __restrict__ Gv, int y, int x, float& sg) {
    const int p = y * a.W + x, q = DY ? p + a.W : p + 1;
    const float t = (Dv[q] - Dv[p]) - (D0v[q] - D0v[p]);
    const float gm = Gv ? Gv[y * (a.W - 1) + x] : 1.0f;
    const float w = gm * t;
    sg = gm * signf(w);
    return fabsf(w);
}

__global__ void __launch_bounds__(256) chart_align_fwd_kernel(AlignArgs a, const float* __restrict__ depths) {
    __shared__ double s_red[4][4];
    const Pix t = ca_pixel(a);
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (t.valid) {
        const size_t at = (size_t)t.v * a.N + t.p;
        const float* Dv = depths + (size_t)t.v * a.N;
        const float e = fabsf(Dv[t.p] - a.ref[at]);
        float v = e;
        if (a.conf) {
            const float c = a.conf[at];
            v = c * e - a.lambda * logf(c);
        }
        s[0] = a.mask ? a.mask[at] * v : v;
        if ((a.flags & G4S_CHART_ALIGN_GRADIENT) && t.y < a.H - 1 && t.x < a.W - 1) {
            const float* D0v = a.depths0 + (size_t)t.v * a.N;
            const float* Gv = a.gmask ? a.gmask + (size_t)t.v * (a.H - 1) * (a.W - 1) : nullptr;
            float sg;
            s[1] = ca_grad_term<1>(a, Dv, D0v, Gv, t.y, t.x, sg) + ca_grad_term<0>(a, Dv, D0v, Gv, t.y, t.x, sg);
        }
        const float* Nv = a.nrm + 3 * (size_t)t.v * a.N;
        if (a.flags & G4S_CHART_ALIGN_NORMAL) {
            const float* n0 = a.normals0 + 3 * at;
            const float* nu = Nv + 3 * t.p;
            s[2] = 1.0f - ((n0[0] * nu[0] + n0[1] * nu[1]) + n0[2] * nu[2]);
        }
        if (a.flags & G4S_CHART_ALIGN_CURVATURE) {
            float lap[3];
            s[3] = fabsf(a.curv0[at] - ca_lap<false>(nullptr, nullptr, Nv, a.H, a.W, t.y, t.x, lap));
        }
    }
    // The terms are float32, their sums are not: a mean over n N terms is then as good as its terms.
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double b = block_sum_pairs((double)s[k], s_red[k]);
        if (threadIdx.x == 0) a.partials[4 * (size_t)blockIdx.x + k] = b;
    }
}

// one block of 1024 threads folds the block partials; fixed association => bit-reproducible
__global__ void __launch_bounds__(1024) chart_align_reduce_kernel(AlignArgs a) {
    __shared__ double s_v[4][1024];
    fold_partials<4>(a.partials, a.nblocks, s_v);
    if (threadIdx.x < 4) {
        const int k = (int)threadIdx.x;
        const bool on = k == 0 || (a.flags & (1 << (k - 1)));
        const double count = k == 1 ? 2.0 * a.n * (double)(a.H - 1) * (double)(a.W - 1) : (double)a.n * (double)a.N;
        a.out4[k] = on ? (float)(s_v[k][0] / count) : 0.0f;
    }
}

// A = b x dL/dc, B = dL/dc x a of every pixel ([n,H,W,3]; zero off the interior) from the normals in a.nrm
__global__ void __launch_bounds__(256) chart_align_bwd_ab_kernel(AlignArgs a, const float* __restrict__ cams,
        const float* __restrict__ depths) {
    const Pix t = ca_pixel(a);
    if (!t.valid) return;
    const size_t at = (size_t)t.v * a.N + t.p;
    float A[3] = {0.0f, 0.0f, 0.0f}, B[3] = {0.0f, 0.0f, 0.0f};
    if (ca_interior(a.H, a.W, t.y, t.x)) {
        const float nN = (float)((double)a.n * (double)a.N);
        float G[3] = {0.0f, 0.0f, 0.0f};
        if (a.flags & G4S_CHART_ALIGN_CURVATURE) {
            // the sign weights of the pixel and of its four neighbours (all inside: the pixel is interior); small
            // integers, their differences and sums are exact
            const float* Nv = a.nrm + 3 * (size_t)t.v * a.N;
            const float* K0 = a.curv0 + (size_t)t.v * a.N;
            const int ys[5] = {t.y, t.y - 1, t.y, t.y + 1, t.y}, xs[5] = {t.x, t.x, t.x - 1, t.x, t.x + 1};
            float w[5][3];
#pragma unroll
            for (int j = 0; j < 5; j++) {
                float lap[3];
                const float curv = ca_lap<false>(nullptr, nullptr, Nv, a.H, a.W, ys[j], xs[j], lap);
                const float sc = signf(curv - K0[ys[j] * a.W + xs[j]]);
#pragma unroll
                for (int k = 0; k < 3; k++) w[j][k] = sc * signf(lap[k]);
            }
            const float k3 = a.g4[3] / nN;
#pragma unroll
            for (int k = 0; k < 3; k++)
                G[k] = k3 * ((((w[1][k] - w[0][k]) + (w[2][k] - w[0][k])) + (w[3][k] - w[0][k])) + (w[4][k] - w[0][k]));
        }
        if (a.flags & G4S_CHART_ALIGN_NORMAL) {
            const float k2 = a.g4[2] / nN;
            const float* n0 = a.normals0 + 3 * at;
#pragma unroll
            for (int k = 0; k < 3; k++) G[k] = G[k] - k2 * n0[k];
        }
        float av[3], bv[3], cr[3], g[3];
        const float L = ca_cross(cams + t.v * CA_CAM_FLOATS, depths + (size_t)t.v * a.N, a.W, t.y, t.x, av, bv, cr);
        if (L < CA_NORM_EPS) {  // below the clamp: nu = c / 1e-12
#pragma unroll
            for (int k = 0; k < 3; k++) g[k] = G[k] / CA_NORM_EPS;
        } else {  // at or above it (a NaN too): nu = c / L
            const float f = ((cr[0] * G[0] + cr[1] * G[1]) + cr[2] * G[2]) / ((L * L) * L);
#pragma unroll
            for (int k = 0; k < 3; k++) g[k] = G[k] / L - cr[k] * f;
        }
        A[0] = bv[1] * g[2] - bv[2] * g[1];
        A[1] = bv[2] * g[0] - bv[0] * g[2];
        A[2] = bv[0] * g[1] - bv[1] * g[0];
        B[0] = g[1] * av[2] - g[2] * av[1];
        B[1] = g[2] * av[0] - g[0] * av[2];
        B[2] = g[0] * av[1] - g[1] * av[0];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a.A[3 * at + k] = A[k];
        a.B[3 * at + k] = B[k];
    }
}

// dL/ddepths and dL/dconfidence of every pixel: the depth term, the at most four memberships in gradient stencils, and
// dir . dL/dq gathered from A and B of the four neighbours
__global__ void __launch_bounds__(256) chart_align_bwd_gather_kernel(AlignArgs a, const float* __restrict__ cams,
        const float* __restrict__ depths) {
    const Pix t = ca_pixel(a);
    if (!t.valid) return;
    const size_t at = (size_t)t.v * a.N + t.p;
    const float* Dv = depths + (size_t)t.v * a.N;
    const float nN = (float)((double)a.n * (double)a.N);
    const float e = Dv[t.p] - a.ref[at];
    float km = a.g4[0] / nN;
    if (a.mask) km = km * a.mask[at];
    float gd;
    if (a.conf) {
        const float c = a.conf[at];
        gd = (km * c) * signf(e);
        a.d_conf[at] = km * (fabsf(e) - a.lambda / c);
    } else {
        gd = km * signf(e);
    }
    if (a.flags & G4S_CHART_ALIGN_GRADIENT) {
        const float* D0v = a.depths0 + (size_t)t.v * a.N;
        const float* Gv = a.gmask ? a.gmask + (size_t)t.v * (a.H - 1) * (a.W - 1) : nullptr;
        const bool below = t.y < a.H - 1, right = t.x < a.W - 1;
        float s = 0.0f, sg;
        if (below && right) {  // the base of its own two differences
            ca_grad_term<1>(a, Dv, D0v, Gv, t.y, t.x, sg);
            s = s - sg;
            ca_grad_term<0>(a, Dv, D0v, Gv, t.y, t.x, sg);
            s = s - sg;
        }
        if (t.y >= 1 && right) {  // the far end of the row difference based above
            ca_grad_term<1>(a, Dv, D0v, Gv, t.y - 1, t.x, sg);
            s = s + sg;
        }
        if (t.x >= 1 && below) {  // the far end of the column difference based to the left
            ca_grad_term<0>(a, Dv, D0v, Gv, t.y, t.x - 1, sg);
            s = s + sg;
        }
        const float k1 = a.g4[1] / (float)(2.0 * a.n * (double)(a.H - 1) * (double)(a.W - 1));
        gd = gd + k1 * s;
    }
    if (a.flags & (G4S_CHART_ALIGN_NORMAL | G4S_CHART_ALIGN_CURVATURE)) {
        const float* Av = a.A + 3 * (size_t)t.v * a.N;
        const float* Bv = a.B + 3 * (size_t)t.v * a.N;
        float dq[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (t.y >= 1) dq[k] = dq[k] + Av[3 * (t.p - a.W) + k];
            if (t.y < a.H - 1) dq[k] = dq[k] - Av[3 * (t.p + a.W) + k];
            if (t.x >= 1) dq[k] = dq[k] + Bv[3 * (t.p - 1) + k];
            if (t.x < a.W - 1) dq[k] = dq[k] - Bv[3 * (t.p + 1) + k];
        }
        float dir[3];
        ca_dir(cams + t.v * CA_CAM_FLOATS, t.y, t.x, dir);
        gd = gd + ((dir[0] * dq[0] + dir[1] * dq[1]) + dir[2] * dq[2]);
    }
    a.d_depths[at] = gd;
}

}  // namespace g4s

using namespace g4s;

// n H W 3, the element count of the [n,H,W,3] buffers, has to fit a 32-bit index
static inline bool ca_size_ok(int n, int height, int width) {
    return n > 0 && height > 0 && width > 0 && (long long)n * height * width * 3 <= 2147483647ll;
}

struct AlignLayout { size_t partials, nrm, A, B, bytes; };
static AlignLayout ca_layout(int n, int height, int width) {
    WorkspaceCursor c;
    AlignLayout L;
    const size_t map3 = (size_t)n * height * width * 3 * 4;
    L.partials = c.take((size_t)n * chart_view_blocks(height, width) * 4 * 8);
    L.nrm = c.take(map3);
    L.A = c.take(map3);
    L.B = c.take(map3);
    L.bytes = c.off;
    return L;
}

extern "C" size_t g4s_chart_align_workspace(int n, int height, int width) {
    if (!ca_size_ok(n, height, width)) return 0;
    return ca_layout(n, height, width).bytes + WORKSPACE_BASE_SLACK;
}

static int ca_check(int n, int height, int width) {
    if (n <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "chart align: n must be positive (no charts)");
    if (width <= 0 || height <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "chart align: width, height must be positive");
    if (!ca_size_ok(n, height, width))
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart align: the [n,H,W,3] maps must have fewer than 2^31 elements, got %lld",
                    (long long)n * height * width * 3);
    return G4S_OK;
}

static AlignArgs ca_args(int n, int height, int width, char* workspace) {
    AlignArgs a{};
    a.n = n; a.H = height; a.W = width; a.N = height * width;
    a.bpv = (int)chart_view_blocks(height, width);
    a.nblocks = n * a.bpv;
    if (workspace) {
        const AlignLayout L = ca_layout(n, height, width);
        a.partials = workspace_at<double>(workspace, L.partials);
        a.nrm = workspace_at<float>(workspace, L.nrm);
        a.A = workspace_at<float>(workspace, L.A);
        a.B = workspace_at<float>(workspace, L.B);
    }
    return a;
}

extern "C" int g4s_chart_align_normals(int n, int height, int width, const float* cameras, const float* depths,
                                       float* normals, float* curv_out, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (int rc = ca_check(n, height, width)) return rc;
    if (depths && !cameras) return fail(G4S_ERR_INVALID_ARGUMENT, "chart align: depths without cameras");
    if (!depths && !(normals && curv_out))
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart align: without depths, normals (read) and curv_out (written) are required");
    if (!normals && !curv_out) return fail(G4S_ERR_INVALID_ARGUMENT, "chart align: no output asked for");
    AlignArgs a = ca_args(n, height, width, nullptr);
    const dim3 grid((unsigned)a.nblocks), block(256);
    if (depths && normals) hipLaunchKernelGGL(chart_align_normals_kernel, grid, block, 0, s, a, cameras, depths, normals);
    if (curv_out) {
        if (normals) hipLaunchKernelGGL(chart_align_curv_kernel<false>, grid, block, 0, s, a, cameras, depths, (const float*)normals, curv_out);
        else hipLaunchKernelGGL(chart_align_curv_kernel<true>, grid, block, 0, s, a, cameras, depths, (const float*)nullptr, curv_out);
    }
    return stage_done("chart_align_normals", s);
}

// what forward and backward check alike, and the argument block they share
static int ca_loss_args(AlignArgs& a, int n, int height, int width, const float* cameras, const float* depths,
                        const float* reference_depths, const float* confidence, const float* masks,
                        const float* initial_depths, const float* gradient_masks, const float* initial_normals,
                        const float* initial_curvatures, float confidence_weighting, int flags, char* workspace,
                        size_t workspace_bytes) {
    if (int rc = ca_check(n, height, width)) return rc;
    if (flags & ~(G4S_CHART_ALIGN_GRADIENT | G4S_CHART_ALIGN_NORMAL | G4S_CHART_ALIGN_CURVATURE))
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart align: unknown bits in flags (%d)", flags);
    if ((flags & G4S_CHART_ALIGN_GRADIENT) && (height < 2 || width < 2))
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart align: the gradient term needs H >= 2 and W >= 2 (no difference to average), got %d x %d",
                    height, width);
    if (!cameras || !depths || !reference_depths) return null_pointer();
    if ((flags & G4S_CHART_ALIGN_GRADIENT) && !initial_depths)
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart align: the gradient term needs initial_depths");
    if ((flags & G4S_CHART_ALIGN_NORMAL) && !initial_normals)
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart align: the normal term needs initial_normals");
    if ((flags & G4S_CHART_ALIGN_CURVATURE) && !initial_curvatures)
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart align: the curvature term needs initial_curvatures");
    if (int rc = check_workspace(workspace, workspace_bytes, g4s_chart_align_workspace(n, height, width))) return rc;
    a = ca_args(n, height, width, workspace);
    a.flags = flags; a.lambda = confidence_weighting;
    a.ref = reference_depths; a.conf = confidence; a.mask = masks; a.depths0 = initial_depths; a.gmask = gradient_masks;
    a.normals0 = initial_normals; a.curv0 = initial_curvatures;
    return G4S_OK;
}

extern "C" int g4s_chart_align_forward(int n, int height, int width, const float* cameras, const float* depths,
                                       const float* reference_depths, const float* confidence, const float* masks,
                                       const float* initial_depths, const float* gradient_masks,
                                       const float* initial_normals, const float* initial_curvatures,
                                       float confidence_weighting, int flags, float* out4, char* workspace,
                                       size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    AlignArgs a;
    if (int rc = ca_loss_args(a, n, height, width, cameras, depths, reference_depths, confidence, masks, initial_depths,
                              gradient_masks, initial_normals, initial_curvatures, confidence_weighting, flags, workspace,
                              workspace_bytes))
        return rc;
    if (!out4) return null_pointer();
    a.out4 = out4;
    const dim3 grid((unsigned)a.nblocks), block(256);
    if (flags & (G4S_CHART_ALIGN_NORMAL | G4S_CHART_ALIGN_CURVATURE))
        hipLaunchKernelGGL(chart_align_normals_kernel, grid, block, 0, s, a, cameras, depths, a.nrm);
    hipLaunchKernelGGL(chart_align_fwd_kernel, grid, block, 0, s, a, depths);
    hipLaunchKernelGGL(chart_align_reduce_kernel, dim3(1), dim3(1024), 0, s, a);
    return stage_done("chart_align_forward", s);
}

extern "C" int g4s_chart_align_backward(int n, int height, int width, const float* cameras, const float* depths,
                                        const float* reference_depths, const float* confidence, const float* masks,
                                        const float* initial_depths, const float* gradient_masks,
                                        const float* initial_normals, const float* initial_curvatures,
                                        float confidence_weighting, int flags, const float* grad_out4, float* dL_ddepths,
                                        float* dL_dconfidence, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    AlignArgs a;
    if (int rc = ca_loss_args(a, n, height, width, cameras, depths, reference_depths, confidence, masks, initial_depths,
                              gradient_masks, initial_normals, initial_curvatures, confidence_weighting, flags, workspace,
                              workspace_bytes))
        return rc;
    if (!grad_out4 || !dL_ddepths || (confidence && !dL_dconfidence)) return null_pointer();
    a.g4 = grad_out4; a.d_depths = dL_ddepths; a.d_conf = dL_dconfidence;
    const dim3 grid((unsigned)a.nblocks), block(256);
    if (flags & (G4S_CHART_ALIGN_NORMAL | G4S_CHART_ALIGN_CURVATURE)) {
        if (flags & G4S_CHART_ALIGN_CURVATURE)
            hipLaunchKernelGGL(chart_align_normals_kernel, grid, block, 0, s, a, cameras, depths, a.nrm);
        hipLaunchKernelGGL(chart_align_bwd_ab_kernel, grid, block, 0, s, a, cameras, depths);
    }
    hipLaunchKernelGGL(chart_align_bwd_gather_kernel, grid, block, 0, s, a, cameras, depths);
    return stage_done("chart_align_backward", s);
}
