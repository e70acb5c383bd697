// The deformation of MAtCha's chart alignment (include/g4s_losses.h, "Chart deformation": g4s_chart_deform_*), kernels and
// entry points.
//
// Reference semantics: ParallelAligner.verts_deformations, .verts and .deformed_depths
// (matcha/dm_scene/parallel_aligner.py:341-413) with MultiResChartsEncoding, ChartsEncoding and DepthEncoding
// (matcha/dm_deformation/encodings.py:49-179) and DeformationMultiMLP / MultiLinear (matcha/dm_deformation/multi_mlp.py:33-242),
// which run five grid_sample calls, a cat, three bmm and keep every [n, H W, 32] and [n, H W, 64] tensor for autograd.
//
// MI355X design.  A workgroup of four waves serves G4S_CHART_DEFORM_WG_PIXELS consecutive pixels of ONE chart in tiles of
// G4S_CHART_DEFORM_TILE = 64, sixteen pixels per wave.  The chart's weights lie in LDS, transposed ([in][out + 4]: the A
// operand of the forward product is then read without bank conflicts).  Every layer but the last runs on
// v_mfma_f32_16x16x4_f32 with the weights as the A operand and the activations as the B operand:
//   A[i][k] = W[16 ot + i][kk],   B[k][j] = a[kk][pixel j],   D[i][j] = z[16 ot + i][pixel j]
// The accumulator tile D holds, in lane (pixel j, group g = lane / 16), the rows 4 g + r, r = 0..3 -- and the B operand of
// one MFMA wants, in the same lane, ONE row of group g.  So the k-step r of input tile t takes register r of the previous
// layer's tile t as it lies: its four k are the rows 16 t + 4 g + r, g = 0..3.  That permutes the order of the sum over k
// (stated in the header), costs nothing, and no activation ever leaves the registers in the forward.  The last layer has one
// output: sixteen fmaf per lane and two cross-lane adds.
//
// The backward recomputes the activations of its tile, forms the cotangents by the same MFMA with the roles of the weight
// matrix's indices exchanged (A[i][k] = W[16 ot + 4 g' + r][16 kt + i], read from the same LDS image), and passes the layer's
// dz [out][64 pixels] and input a [in][64 pixels] through two LDS tiles (pitch 68: conflict-free as MFMA operands), from which
// wave w forms rows 16 w .. 16 w + 15 of the tile's dW = dz a^T -- sixteen k-steps over the tile's 64 pixels in index order,
// from 0 -- and adds it to accumulators that live across the workgroup's tiles (two levels: a 4096-long float32 chain would
// carry four times the rounding of torch's blocked sums).  One partial per workgroup goes to the workspace; a second kernel
// folds a chart's partials in workgroup order.  dL/dx [n, H W, E] goes to the workspace; the encoding grids GATHER from it
// (per texel the rectangle of pixels whose taps can reach it; per depth bin a walk over the pixels in index order, in
// workgroup-sized pieces that the same fold finishes).  No atomics, no fixed-point sums.
//
// The forward, backward, fold and level kernels carry a compile-time switch REG ("Chart alignment: confidence, weighted
// encodings, encoding regularisers" of the header: g4s_chart_deform_reg_*).  REG = false is the plain pair's code, unchanged;
// REG = true adds the per-pixel encoding weight, the norm of the unweighted chart encoding (formed in the gather, reduced
// per workgroup in double) and, in the backward, the norm's and the total variation's cotangents.  The confidence
// activation (g4s_chart_confidence_*) lives here too.
#include "g4s_internal.h"
#include "g4s_device.h"
#include "chart_common.h"
#include "../../include/g4s_losses.h"

namespace g4s {

constexpr int CD_TILE = G4S_CHART_DEFORM_TILE;            // pixels per workgroup tile (16 per wave)
constexpr int CD_WG_PIXELS = G4S_CHART_DEFORM_WG_PIXELS;  // pixels per workgroup
constexpr int CD_MAX_LEVELS = G4S_CHART_DEFORM_MAX_LEVELS;
constexpr int CD_MAX_LAYERS = 4;
constexpr int CD_PITCH = CD_TILE + 4;  // of the two [row][pixel] LDS tiles
constexpr int CD_CAM_FLOATS = 12;
// the LDS image of the largest network: E = S = 64, four layers
constexpr int CD_MAX_PARAMS = 3 * 64 * 68 + 64 + 3 * 64 + 1;

using f32x4 = __attribute__((ext_vector_type(4))) float;

// LDS image of a chart's parameters: layer l < NL - 1 as Wt[in][out + 4] (transposed), the last as w[S]; then the biases.
struct Image {
    int w[CD_MAX_LAYERS], b[CD_MAX_LAYERS], wlast, blast;
};

struct DeformArgs {
    int n, H, W, N;
    int L, C, E, B, NL, S;
    int lh[CD_MAX_LEVELS], lw[CD_MAX_LEVELS];
    const float* level[CD_MAX_LEVELS];  // [n,C,h_l,w_l]
    const float* denc;                  // [n,E,B] or NULL
    const float* w[CD_MAX_LAYERS];      // [n,out,in]
    const float* b[CD_MAX_LAYERS];      // [n,out]
    const float* coords;                // [n,N]
    const float* cams;                  // [n,12]
    const float* d0;                    // [n,N]
    float R, Rd;
    int wgs;                           // workgroups per chart
    Image im;                          // offsets into the LDS image
    int goff_w[CD_MAX_LAYERS], goff_b[CD_MAX_LAYERS], goff_denc, gcount;  // a partial: the gradients packed in their own layouts
    float *depths, *delta;
    const float* g;   // dL/ddepths
    float* dx;        // [n,N,E]
    float* partials;  // [n wgs][gcount]
    float* dw[CD_MAX_LAYERS];
    float* db[CD_MAX_LAYERS];
    float* dlevel[CD_MAX_LEVELS];
    float* ddenc;
    // REG only
    const float* encw;  // [n,N] or NULL: the weight of the chart encoding
    int flags;          // G4S_CHART_DEFORM_REG_NORM | _TV
    const float* dreg;  // [2]: dL/dreg
    float* coef;        // [n,N]: (dL/dreg[0] / r(p)) / (n N), 0 where r(p) = 0
    double* rpart;      // [n wgs]: a workgroup's sum of r(p)
    float* reg_out;     // [2]
};

constexpr int CD_REG_NORM = G4S_CHART_DEFORM_REG_NORM, CD_REG_TV = G4S_CHART_DEFORM_REG_TV;

__device__ __forceinline__ int cd_in(const DeformArgs& a, int l) { return l == 0 ? a.E : a.S; }
__device__ __forceinline__ int cd_out(const DeformArgs& a, int l) { return l == a.NL - 1 ? 1 : a.S; }

// ---- the sampling positions ---------------------------------------------------------------------------------------------
// lin_K[i] of the contract: (2 i - (K - 1)) / (K - 1), one rounding (the numerator is an exact integer); -1 for K = 1
__device__ __forceinline__ float cd_lin(int i, int K) { return K > 1 ? (float)(2 * i - (K - 1)) / (float)(K - 1) : -1.0f; }

// The two taps along one axis of `size` texels at the normalised coordinate u: i0, i1 (clamped) and their weights.
struct Taps {
    int i0, i1;
    float w0, w1;
};
__device__ __forceinline__ Taps cd_taps(float u, int size) {
    float x = ((u + 1.0f) * (float)size - 1.0f) / 2.0f;
    const float top = (float)(size - 1);
    x = x < 0.0f ? 0.0f : (x > top ? top : x);  // padding_mode='border'
    const float f = floorf(x);
    Taps t;
    t.i0 = clampi((int)f, size - 1);  // a NaN coordinate reads texel 0, never outside
    t.i1 = t.i0 + 1 > size - 1 ? size - 1 : t.i0 + 1;  // weight exactly 0 where clamped
    t.w0 = (f + 1.0f) - x;
    t.w1 = x - f;
    return t;
}

// sign(d0) / |D (x, y, 1)| of pixel (y, x): d(depth)/d(delta)
__device__ __forceinline__ float cd_ray_scale(const float* __restrict__ c, int y, int x, float d0) {
    const float fx = (float)x, fy = (float)y;
    float dir[3];
#pragma unroll
    for (int k = 0; k < 3; k++) dir[k] = (c[3 + 3 * k] * fx + c[4 + 3 * k] * fy) + c[5 + 3 * k];
    const float len = sqrtf((dir[0] * dir[0] + dir[1] * dir[1]) + dir[2] * dir[2]);
    return signf(d0) / len;
}

// The lane's share of its pixel's input: x[t][r] = a0 of channel 16 t + 4 g + r, t < ET.  REG: the chart encoding is
// multiplied by the pixel's weight before the depth encoding is added, and ss takes the fma chain of the lane's unweighted
// enc_e^2 in the order t, r.
template <int ET, bool REG>
__device__ __forceinline__ void cd_gather(const DeformArgs& a, int chart, int p, int g, float (&x)[ET][4], float& ss) {
    const int row = p / a.W, col = p % a.W;
    const float ux = cd_lin(row, a.H), uy = cd_lin(col, a.W);  // the reference's transposed indexing: the ROW drives x
    Taps td{};
    if (a.denc) {
        const float y = -1.0f + 2.0f * a.coords[(size_t)chart * a.N + p];
        td = cd_taps(y, a.B);
    }
    float wgt = 1.0f;
    if constexpr (REG) {
        ss = 0.0f;
        if (a.encw) wgt = a.encw[(size_t)chart * a.N + p];
    }
#pragma unroll
    for (int t = 0; t < ET; t++) {
        const int e0 = 16 * t + 4 * g;
        const int l = e0 / a.C, c0 = e0 % a.C;  // C is a multiple of 4: the four channels share a level
        const int h = a.lh[l], w = a.lw[l];
        const Taps tx = cd_taps(ux, w), ty = cd_taps(uy, h);
        const float w00 = tx.w0 * ty.w0, w01 = tx.w1 * ty.w0, w10 = tx.w0 * ty.w1, w11 = tx.w1 * ty.w1;
        const float* __restrict__ base = a.level[l] + ((size_t)chart * a.C + c0) * h * w;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float* __restrict__ v = base + (size_t)r * h * w;
            float s = ((v[ty.i0 * w + tx.i0] * w00 + v[ty.i0 * w + tx.i1] * w01) + v[ty.i1 * w + tx.i0] * w10) + v[ty.i1 * w + tx.i1] * w11;
            if constexpr (REG) {
                ss = fmaf(s, s, ss);
                if (a.encw) s = s * wgt;
            }
            if (a.denc) {
                const float* __restrict__ q = a.denc + ((size_t)chart * a.E + e0 + r) * a.B;
                s = s + (q[td.i0] * td.w0 + q[td.i1] * td.w1);
            }
            x[t][r] = s / a.R;
        }
    }
}

// r(p) = sqrt((s_0 + s_1) + (s_2 + s_3)) of the four lanes' chains, in every lane of the pixel
__device__ __forceinline__ float cd_norm(float ss) {
    ss = ss + __shfl_xor(ss, 16, 64);
    ss = ss + __shfl_xor(ss, 32, 64);
    return sqrtf(ss);
}

// ---- the network -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void cd_load_image(const DeformArgs& a, const Image& im, int chart, float* s_p) {
    const int P = a.S + 4;
    for (int l = 0; l < a.NL; l++) {
        const int in = cd_in(a, l), out = cd_out(a, l);
        const float* __restrict__ W = a.w[l] + (size_t)chart * out * in;
        for (int j = (int)threadIdx.x; j < out * in; j += (int)blockDim.x) {
            const int o = j / in, k = j % in;
            s_p[im.w[l] + (l == a.NL - 1 ? k : k * P + o)] = W[j];
        }
        for (int j = (int)threadIdx.x; j < out; j += (int)blockDim.x) s_p[im.b[l] + j] = a.b[l][(size_t)chart * out + j];
    }
}

// z = b + W a over IT input tiles, by MFMA; ReLU applied to the accumulators.  x[t][r]: row 16 t + 4 g + r of the input of
// this lane's pixel; z alike for the output.
template <int IT, int ST>
__device__ __forceinline__ void cd_layer(const float* __restrict__ Wt, const float* __restrict__ bias, int P, int pl, int g,
                                         const float (&x)[IT][4], float (&z)[ST][4]) {
#pragma unroll
    for (int ot = 0; ot < ST; ot++) {
        f32x4 acc;
#pragma unroll
        for (int r = 0; r < 4; r++) acc[r] = bias[16 * ot + 4 * g + r];
#pragma unroll
        for (int t = 0; t < IT; t++) {
#pragma unroll
            for (int r = 0; r < 4; r++)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Wt[(16 * t + 4 * g + r) * P + 16 * ot + pl], x[t][r], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) z[ot][r] = acc[r] > 0.0f ? acc[r] : 0.0f;
    }
}

// da = W^T dz: rows 16 kt + 4 g + r of the input's cotangent from dz[ot][r] (row 16 ot + 4 g + r of the output's)
template <int IT, int ST>
__device__ __forceinline__ void cd_layer_T(const float* __restrict__ Wt, int P, int pl, int g, const float (&dz)[ST][4],
                                           float (&da)[IT][4]) {
#pragma unroll
    for (int kt = 0; kt < IT; kt++) {
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ot = 0; ot < ST; ot++) {
#pragma unroll
            for (int r = 0; r < 4; r++)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Wt[(16 * kt + pl) * P + 16 * ot + 4 * g + r], dz[ot][r], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) da[kt][r] = acc[r];
    }
}

// out = ((p_0 + p_1) + (p_2 + p_3)) + b of the last layer, p_g the lane group's fmaf chain over its sixteen rows
template <int ST>
__device__ __forceinline__ float cd_last(const float* __restrict__ wl, float bias, int g, const float (&x)[ST][4]) {
    float p = 0.0f;
#pragma unroll
    for (int t = 0; t < ST; t++) {
#pragma unroll
        for (int r = 0; r < 4; r++) p = fmaf(wl[16 * t + 4 * g + r], x[t][r], p);
    }
    p = p + __shfl_xor(p, 16, 64);
    p = p + __shfl_xor(p, 32, 64);
    return p + bias;
}

// The hidden activations of the lane's pixel: h[0] = layer 0 of x, h[l] = layer l of h[l-1] for l < NL - 1.
template <int ET, int ST>
__device__ __forceinline__ void cd_hidden(const DeformArgs& a, const Image& im, const float* __restrict__ s_p, int pl, int g,
                                          const float (&x)[ET][4], float (&h)[CD_MAX_LAYERS - 1][ST][4]) {
    const int P = a.S + 4;
    cd_layer<ET, ST>(s_p + im.w[0], s_p + im.b[0], P, pl, g, x, h[0]);
#pragma unroll
    for (int l = 1; l < CD_MAX_LAYERS - 1; l++) {
        if (l < a.NL - 1) cd_layer<ST, ST>(s_p + im.w[l], s_p + im.b[l], P, pl, g, h[l - 1], h[l]);
    }
}

// grid n * wgs; block 256
template <int ET, int ST, bool REG>
__global__ void __launch_bounds__(256) chart_deform_fwd_kernel(DeformArgs a) {
    __shared__ float s_p[CD_MAX_PARAMS];
    __shared__ double s_r[REG ? CD_TILE : 1];
    double racc = 0.0;  // REG: the sum of r(p) over this lane's pixels, in tile order
    const int chart = (int)blockIdx.x / a.wgs, first = ((int)blockIdx.x % a.wgs) * CD_WG_PIXELS;
    const int last = first + CD_WG_PIXELS < a.N ? first + CD_WG_PIXELS : a.N;
    const Image& im = a.im;
    cd_load_image(a, im, chart, s_p);
    __syncthreads();
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6, pl = lane & 15, g = lane >> 4;
    const float* __restrict__ cam = a.cams + chart * CD_CAM_FLOATS;
    for (int base = first; base < last; base += CD_TILE) {
        const int p = base + 16 * wv + pl;
        const int pc = p < last ? p : last - 1;  // a lane past the end repeats the last pixel and stores nothing
        float x[ET][4], h[CD_MAX_LAYERS - 1][ST][4], ss;
        cd_gather<ET, REG>(a, chart, pc, g, x, ss);
        if constexpr (REG) {
            if (a.flags & CD_REG_NORM) {
                const float r = cd_norm(ss);
                if (p < last) racc = racc + (double)r;
            }
        }
        cd_hidden<ET, ST>(a, im, s_p, pl, g, x, h);
        float out = 0.0f;
#pragma unroll
        for (int l = 0; l < CD_MAX_LAYERS - 1; l++) {
            if (l == a.NL - 2) out = cd_last<ST>(s_p + im.wlast, s_p[im.blast], g, h[l]);
        }
        if (g == 0 && p < last) {
            const size_t at = (size_t)chart * a.N + p;
            const float delta = out * a.Rd, d0 = a.d0[at];
            a.depths[at] = d0 == 0.0f ? d0 : d0 + delta * cd_ray_scale(cam, p / a.W, p % a.W, d0);
            if (a.delta) a.delta[at] = delta;
        }
    }
    if constexpr (REG) {
        if (a.flags & CD_REG_NORM) {  // the workgroup's sum: the 64 pixel slots of a tile in index order
            if (g == 0) s_r[16 * wv + pl] = racc;
            __syncthreads();
            if (threadIdx.x == 0) {
                double s = s_r[0];
                for (int j = 1; j < CD_TILE; j++) s = s + s_r[j];
                a.rpart[blockIdx.x] = s;
            }
        }
    }
}

// grid n * wgs; block 256.  Leaves dL/dx of its pixels in a.dx and one partial of the weight and bias gradients.
template <int ET, int ST, bool REG>
__global__ void __launch_bounds__(256) chart_deform_bwd_kernel(DeformArgs a) {
    __shared__ float s_p[CD_MAX_PARAMS];
    __shared__ float s_act[64 * CD_PITCH], s_dz[64 * CD_PITCH], s_gz[CD_TILE];
    const int chart = (int)blockIdx.x / a.wgs, first = ((int)blockIdx.x % a.wgs) * CD_WG_PIXELS;
    const int last = first + CD_WG_PIXELS < a.N ? first + CD_WG_PIXELS : a.N;
    const Image& im = a.im;
    cd_load_image(a, im, chart, s_p);
    __syncthreads();
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6, pl = lane & 15, g = lane >> 4;
    const int P = a.S + 4, S = a.S;
    const float* __restrict__ cam = a.cams + chart * CD_CAM_FLOATS;
    // what lives across the tiles: rows 16 wv .. + 15 of every hidden layer's dW, one bias entry per thread and layer, and
    // one entry of the last layer's weight gradient (thread S holds its bias gradient)
    f32x4 gw0[ET], gw[CD_MAX_LAYERS - 2][ST];
    float gb[CD_MAX_LAYERS - 1], glast = 0.0f;
#pragma unroll
    for (int t = 0; t < ET; t++) gw0[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int l = 0; l < CD_MAX_LAYERS - 2; l++) {
#pragma unroll
        for (int t = 0; t < ST; t++) gw[l][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
#pragma unroll
    for (int l = 0; l < CD_MAX_LAYERS - 1; l++) gb[l] = 0.0f;

    for (int base = first; base < last; base += CD_TILE) {
        const int p = base + 16 * wv + pl;
        const bool valid = p < last;
        const int pc = valid ? p : last - 1;
        float x[ET][4], h[CD_MAX_LAYERS - 1][ST][4], ss;
        cd_gather<ET, REG>(a, chart, pc, g, x, ss);
        if constexpr (REG) {
            if (a.flags & CD_REG_NORM) {  // the norm's cotangent per pixel, for the level kernels
                const float r = cd_norm(ss);
                if (g == 0 && valid) a.coef[(size_t)chart * a.N + p] = r > 0.0f ? (a.dreg[0] / r) / (float)((long long)a.n * a.N) : 0.0f;
            }
        }
        cd_hidden<ET, ST>(a, im, s_p, pl, g, x, h);
        const size_t at = (size_t)chart * a.N + pc;
        const float d0 = a.d0[at];
        // cotangent of the network's output; a lane past the end carries exactly 0
        const float gz = valid && d0 != 0.0f ? (a.g[at] * cd_ray_scale(cam, pc / a.W, pc % a.W, d0)) * a.Rd : 0.0f;
        // the last layer: its input and gz through LDS for the sums over the tile's pixels
        float dz[ST][4];
#pragma unroll
        for (int l = 0; l < CD_MAX_LAYERS - 1; l++) {
            if (l == a.NL - 2) {
#pragma unroll
                for (int t = 0; t < ST; t++) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int k = 16 * t + 4 * g + r;
                        s_act[k * CD_PITCH + 16 * wv + pl] = h[l][t][r];
                        dz[t][r] = h[l][t][r] > 0.0f ? s_p[im.wlast + k] * gz : 0.0f;
                    }
                }
            }
        }
        if (g == 0) s_gz[16 * wv + pl] = gz;
        __syncthreads();
        if (tid < S) {  // the tile's sum from 0, then onto the running sum: two levels keep the rounding of a long chain out
            float s = 0.0f;
            for (int j = 0; j < CD_TILE; j++) s = fmaf(s_act[tid * CD_PITCH + j], s_gz[j], s);
            glast = glast + s;
        } else if (tid == S) {
            float s = 0.0f;
            for (int j = 0; j < CD_TILE; j++) s = s + s_gz[j];
            glast = glast + s;
        }
        __syncthreads();
        // the hidden layers, last to first: dz is the cotangent of layer l's output
#pragma unroll
        for (int l = CD_MAX_LAYERS - 2; l >= 0; l--) {
            if (l <= a.NL - 2) {
#pragma unroll
                for (int t = 0; t < ST; t++) {
#pragma unroll
                    for (int r = 0; r < 4; r++) s_dz[(16 * t + 4 * g + r) * CD_PITCH + 16 * wv + pl] = dz[t][r];
                }
                if (l == 0) {
#pragma unroll
                    for (int t = 0; t < ET; t++) {
#pragma unroll
                        for (int r = 0; r < 4; r++) s_act[(16 * t + 4 * g + r) * CD_PITCH + 16 * wv + pl] = x[t][r];
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < ST; t++) {
#pragma unroll
                        for (int r = 0; r < 4; r++) s_act[(16 * t + 4 * g + r) * CD_PITCH + 16 * wv + pl] = h[l > 0 ? l - 1 : 0][t][r];
                    }
                }
                __syncthreads();
                if (wv < ST) {  // dW rows 16 wv .. + 15: A[i][k] = dz[16 wv + i][pixel], B[k][j] = a[16 kt + j][pixel]
#pragma unroll
                    for (int kt = 0; kt < (l == 0 ? ET : ST); kt++) {
                        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};  // the tile's sum from 0
#pragma unroll
                        for (int s = 0; s < CD_TILE / 4; s++)
                            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(s_dz[(16 * wv + pl) * CD_PITCH + 4 * s + g],
                                                                       s_act[(16 * kt + pl) * CD_PITCH + 4 * s + g], acc, 0, 0, 0);
                        if (l == 0) gw0[kt < ET ? kt : 0] += acc;
                        else gw[l > 0 ? l - 1 : 0][kt < ST ? kt : 0] += acc;
                    }
                }
                if (tid < S) {
                    float s = 0.0f;
                    for (int j = 0; j < CD_TILE; j++) s = s + s_dz[tid * CD_PITCH + j];
                    gb[l] = gb[l] + s;
                }
                if (l == 0) {
                    float da[ET][4];
                    cd_layer_T<ET, ST>(s_p + im.w[0], P, pl, g, dz, da);
                    if (valid) {
#pragma unroll
                        for (int t = 0; t < ET; t++) {
                            float4 v;
                            v.x = da[t][0] / a.R; v.y = da[t][1] / a.R; v.z = da[t][2] / a.R; v.w = da[t][3] / a.R;
                            *(float4*)(a.dx + ((size_t)chart * a.N + p) * a.E + 16 * t + 4 * g) = v;
                        }
                    }
                } else {
                    float da[ST][4];
                    cd_layer_T<ST, ST>(s_p + im.w[l], P, pl, g, dz, da);
#pragma unroll
                    for (int t = 0; t < ST; t++) {
#pragma unroll
                        for (int r = 0; r < 4; r++) dz[t][r] = h[l > 0 ? l - 1 : 0][t][r] > 0.0f ? da[t][r] : 0.0f;
                    }
                }
                __syncthreads();
            }
        }
    }
    // the partial, in the parameters' own layouts
    float* __restrict__ part = a.partials + (size_t)blockIdx.x * a.gcount;
    if (wv < ST) {
#pragma unroll
        for (int kt = 0; kt < ET; kt++) {
#pragma unroll
            for (int r = 0; r < 4; r++) part[a.goff_w[0] + (16 * wv + 4 * g + r) * a.E + 16 * kt + pl] = gw0[kt][r];
        }
#pragma unroll
        for (int l = 1; l < CD_MAX_LAYERS - 1; l++) {
            if (l < a.NL - 1) {
#pragma unroll
                for (int kt = 0; kt < ST; kt++) {
#pragma unroll
                    for (int r = 0; r < 4; r++) part[a.goff_w[l] + (16 * wv + 4 * g + r) * S + 16 * kt + pl] = gw[l - 1][kt][r];
                }
            }
        }
    }
    if (tid < S) {
#pragma unroll
        for (int l = 0; l < CD_MAX_LAYERS - 1; l++) {
            if (l < a.NL - 1) part[a.goff_b[l] + tid] = gb[l];
        }
        part[a.goff_w[a.NL - 1] + tid] = glast;
    } else if (tid == S) {
        part[a.goff_b[a.NL - 1]] = glast;
    }
}

// The depth encoding's share of a partial: element (e, b) sums, over the workgroup's pixels in index order, dx_e times the
// weight of the tap(s) that land on bin b.  grid n * wgs; block 256.
__global__ void __launch_bounds__(256) chart_deform_denc_kernel(DeformArgs a) {
    __shared__ int s_i0[256], s_i1[256];
    __shared__ float s_w0[256], s_w1[256];
    const int chart = (int)blockIdx.x / a.wgs, first = ((int)blockIdx.x % a.wgs) * CD_WG_PIXELS;
    const int last = first + CD_WG_PIXELS < a.N ? first + CD_WG_PIXELS : a.N;
    const int tid = (int)threadIdx.x, count = a.E * a.B;
    float* __restrict__ part = a.partials + (size_t)blockIdx.x * a.gcount + a.goff_denc;
    for (int j0 = 0; j0 < count; j0 += 4 * 256) {  // four elements per thread and pass
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int e[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int j = j0 + 256 * q + tid;
            e[q] = j < count ? j / a.B : -1;
            b[q] = j < count ? j % a.B : -1;
        }
        for (int base = first; base < last; base += 256) {
            __syncthreads();
            if (base + tid < last) {
                const Taps t = cd_taps(-1.0f + 2.0f * a.coords[(size_t)chart * a.N + base + tid], a.B);
                s_i0[tid] = t.i0; s_i1[tid] = t.i1; s_w0[tid] = t.w0; s_w1[tid] = t.w1;
            }
            __syncthreads();
            const int m = last - base < 256 ? last - base : 256;
            for (int i = 0; i < m; i++) {
                const int i0 = s_i0[i], i1 = s_i1[i];
                const float* __restrict__ dx = a.dx + ((size_t)chart * a.N + base + i) * a.E;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (b[q] == i0) acc[q] = acc[q] + dx[e[q]] * s_w0[i];
                    if (b[q] == i1) acc[q] = acc[q] + dx[e[q]] * s_w1[i];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (e[q] >= 0) part[j0 + 256 * q + tid] = acc[q];
        }
    }
}

// Element j of a chart's packed gradients: its partials summed in workgroup order, written where the parameter's own
// gradient tensor has it.  grid (ceil(gcount / 256), n)
template <bool REG>
__global__ void __launch_bounds__(256) chart_deform_fold_kernel(DeformArgs a) {
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x, chart = (int)blockIdx.y;
    if (j >= a.gcount) return;
    const float* __restrict__ part = a.partials + (size_t)chart * a.wgs * a.gcount + j;
    float s = part[0];
    for (int k = 1; k < a.wgs; k++) s = s + part[(size_t)k * a.gcount];
    if (a.denc && j >= a.goff_denc) {
        if constexpr (REG) {
            if (a.flags & CD_REG_TV) {  // (sign(q[b] - q[b-1]) - sign(q[b+1] - q[b])) (dL/dreg[1] / (n E (B - 1)))
                const int k = j - a.goff_denc, b = k % a.B;
                const float* __restrict__ q = a.denc + (size_t)chart * a.E * a.B + k;
                const float sl = b > 0 ? signf(q[0] - q[-1]) : 0.0f, sr = b < a.B - 1 ? signf(q[1] - q[0]) : 0.0f;
                s = s + (sl - sr) * (a.dreg[1] / (float)((long long)a.n * a.E * (a.B - 1)));
            }
        }
        a.ddenc[(size_t)chart * a.E * a.B + (j - a.goff_denc)] = s;
        return;
    }
    for (int l = a.NL - 1; l >= 0; l--) {
        const int in = cd_in(a, l), out = cd_out(a, l);
        if (j >= a.goff_b[l]) {
            a.db[l][(size_t)chart * out + (j - a.goff_b[l])] = s;
            return;
        }
        if (j >= a.goff_w[l]) {
            a.dw[l][(size_t)chart * out * in + (j - a.goff_w[l])] = s;
            return;
        }
    }
}

// The gradient of level `l`: one thread per texel and four channels gathers from dx over the rectangle of pixels whose taps
// can reach the texel, rows then columns in index order, the four taps of a pixel in the forward's order.
// grid (ceil(h w (C / 4) / 256), n)
// REG: the pixel's term is (w(p) dL/dx_e(p)) + enc_e(p) coef(p), each part only where it is asked for; enc_e(p) is formed
// from the pixel's four texels by the forward's expression.
template <bool REG>
__global__ void __launch_bounds__(256) chart_deform_level_kernel(DeformArgs a, int l) {
    const int h = a.lh[l], w = a.lw[l], c4 = a.C / 4, chart = (int)blockIdx.y;
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= h * w * c4) return;
    const int cq = j / (h * w), ty = (j / w) % h, tx = j % w;
    // pixel ROWS drive x: ix(row) = row w / (H - 1) - 1/2 before the clamp; one more row each way covers the rounding, the
    // exact test below decides.  The border texels also take every row that the clamp sends to them.
    int r0 = 0, r1 = a.H - 1, q0 = 0, q1 = a.W - 1;
    if (a.H > 1) {
        if (tx > 0) r0 = clampi((int)floorf(((float)tx - 0.5f) * (float)(a.H - 1) / (float)w) - 1, a.H - 1);
        if (tx < w - 1) r1 = clampi((int)ceilf(((float)tx + 1.5f) * (float)(a.H - 1) / (float)w) + 1, a.H - 1);
    }
    if (a.W > 1) {
        if (ty > 0) q0 = clampi((int)floorf(((float)ty - 0.5f) * (float)(a.W - 1) / (float)h) - 1, a.W - 1);
        if (ty < h - 1) q1 = clampi((int)ceilf(((float)ty + 1.5f) * (float)(a.W - 1) / (float)h) + 1, a.W - 1);
    }
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int row = r0; row <= r1; row++) {
        const Taps px = cd_taps(cd_lin(row, a.H), w);
        if (px.i0 != tx && px.i1 != tx) continue;
        for (int col = q0; col <= q1; col++) {
            const Taps py = cd_taps(cd_lin(col, a.W), h);
            if (py.i0 != ty && py.i1 != ty) continue;
            const float4 d = *(const float4*)(a.dx + ((size_t)chart * a.N + (size_t)row * a.W + col) * a.E + l * a.C + 4 * cq);
            float dv[4] = {d.x, d.y, d.z, d.w};
            const float wt[4] = {px.w0 * py.w0, px.w1 * py.w0, px.w0 * py.w1, px.w1 * py.w1};
            if constexpr (REG) {
                const size_t at = (size_t)chart * a.N + (size_t)row * a.W + col;
                if (a.encw) {
                    const float wgt = a.encw[at];
#pragma unroll
                    for (int c = 0; c < 4; c++) dv[c] = dv[c] * wgt;
                }
                if (a.flags & CD_REG_NORM) {
                    const float cf = a.coef[at];
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const float* __restrict__ v = a.level[l] + ((size_t)chart * a.C + 4 * cq + c) * h * w;
                        const float enc = ((v[py.i0 * w + px.i0] * wt[0] + v[py.i0 * w + px.i1] * wt[1]) + v[py.i1 * w + px.i0] * wt[2]) +
                                          v[py.i1 * w + px.i1] * wt[3];
                        dv[c] = dv[c] + enc * cf;
                    }
                }
            }
            const bool hit[4] = {px.i0 == tx && py.i0 == ty, px.i1 == tx && py.i0 == ty, px.i0 == tx && py.i1 == ty,
                                 px.i1 == tx && py.i1 == ty};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (hit[k]) {
#pragma unroll
                    for (int c = 0; c < 4; c++) acc[c] = acc[c] + dv[c] * wt[k];
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; c++) a.dlevel[l][(((size_t)chart * a.C + 4 * cq + c) * h + ty) * w + tx] = acc[c];
}

// The two regularisers' values.  One workgroup: thread t sums, in double and in index order, the entries t, t + 256, ... of
// the workgroups' partial sums of r(p) and of |q[b + 1] - q[b]| (a float32 difference) over (chart, e, b); thread 0 adds the
// 256 sums in thread order.  grid 1; block 256
__global__ void __launch_bounds__(256) chart_deform_reg_kernel(DeformArgs a) {
    __shared__ double s_n[256], s_t[256];
    const int tid = (int)threadIdx.x;
    double sn = 0.0, st = 0.0;
    if (a.flags & CD_REG_NORM) {
        for (int k = tid; k < a.n * a.wgs; k += 256) sn = sn + a.rpart[k];
    }
    const long long tv_count = (long long)a.n * a.E * (a.B - 1);
    if (a.flags & CD_REG_TV) {
        for (long long k = tid; k < tv_count; k += 256) {
            const float* __restrict__ q = a.denc + (k / (a.B - 1)) * a.B + k % (a.B - 1);
            st = st + (double)fabsf(q[1] - q[0]);
        }
    }
    s_n[tid] = sn;
    s_t[tid] = st;
    __syncthreads();
    if (tid == 0) {
        for (int j = 1; j < 256; j++) {
            sn = sn + s_n[j];
            st = st + s_t[j];
        }
        a.reg_out[0] = (a.flags & CD_REG_NORM) ? (float)(sn / (double)((long long)a.n * a.N)) : 0.0f;
        a.reg_out[1] = (a.flags & CD_REG_TV) ? (float)(st / (double)tv_count) : 0.0f;
    }
}

// conf = 1 + exp(raw); weight = 1 - exp(-((conf - 1) (conf - 1)) / 2).  grid ceil(count / 256); block 256
__global__ void __launch_bounds__(256) chart_confidence_fwd_kernel(long long count, const float* __restrict__ raw,
                                                                   float* __restrict__ conf, float* __restrict__ weight) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const float c = 1.0f + expf(raw[i]);
    conf[i] = c;
    if (weight) {
        const float cw = c - 1.0f;
        weight[i] = 1.0f - expf(-(cw * cw) / 2.0f);
    }
}

__global__ void __launch_bounds__(256) chart_confidence_bwd_kernel(long long count, const float* __restrict__ raw,
                                                                   const float* __restrict__ dconf, float* __restrict__ draw) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    draw[i] = dconf[i] * expf(raw[i]);
}

}  // namespace g4s

using namespace g4s;

static inline int cd_wgs(int N) { return (N + CD_WG_PIXELS - 1) / CD_WG_PIXELS; }

// the packed gradients of one chart: W_0, b_0, W_1, b_1, ..., then the depth encoding
static void cd_pack(DeformArgs& a) {
    int at = 0;
    for (int l = 0; l < a.NL; l++) {
        const int in = l == 0 ? a.E : a.S, out = l == a.NL - 1 ? 1 : a.S;
        a.goff_w[l] = at;
        at += out * in;
        a.goff_b[l] = at;
        at += out;
    }
    a.goff_denc = at;
    if (a.B > 0) at += a.E * a.B;
    a.gcount = at;
}

static int cd_shape(DeformArgs& a, const g4s_chart_deform_shape* sh) {
    if (!sh) return null_pointer();
    if (sh->n <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "chart deform: n must be positive (no charts)");
    if (sh->width <= 0 || sh->height <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "chart deform: width, height must be positive");
    if ((long long)sh->n * sh->height * sh->width > 2147483647ll)
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart deform: n H W must stay below 2^31, got %lld", (long long)sh->n * sh->height * sh->width);
    if (sh->levels < 1 || sh->levels > CD_MAX_LEVELS)
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart deform: 1 to %d encoding levels, got %d", CD_MAX_LEVELS, sh->levels);
    if (sh->channels < 4 || sh->channels % 4)
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart deform: the channels per level must be a positive multiple of 4, got %d", sh->channels);
    const int E = sh->levels * sh->channels;
    if (E != 16 && E != 32 && E != 64)
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart deform: the encoding width levels x channels must be 16, 32 or 64, got %d", E);
    if (sh->layer_size != 32 && sh->layer_size != 64)
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart deform: the layer size must be 32 or 64, got %d", sh->layer_size);
    if (sh->layers < 2 || sh->layers > CD_MAX_LAYERS)
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart deform: 2 to %d layers, got %d", CD_MAX_LAYERS, sh->layers);
    if (sh->bins < 0 || sh->bins > 4096)
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart deform: 0 (no depth encoding) to 4096 depth bins, got %d", sh->bins);
    for (int l = 0; l < sh->levels; l++) {
        if (sh->level_height[l] < 1 || sh->level_width[l] < 1 || (long long)sh->level_height[l] * sh->level_width[l] > (1 << 24))
            return fail(G4S_ERR_INVALID_ARGUMENT, "chart deform: level %d must have 1 to 2^24 texels, got %d x %d", l, sh->level_height[l],
                        sh->level_width[l]);
    }
    if (!(sh->scene_radius > 0.0f) || !(sh->deformation_radius == sh->deformation_radius))
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart deform: scene_radius must be positive and deformation_radius a number");
    a = DeformArgs{};
    a.n = sh->n; a.H = sh->height; a.W = sh->width; a.N = sh->height * sh->width;
    a.L = sh->levels; a.C = sh->channels; a.E = E; a.B = sh->bins; a.NL = sh->layers; a.S = sh->layer_size;
    for (int l = 0; l < a.L; l++) { a.lh[l] = sh->level_height[l]; a.lw[l] = sh->level_width[l]; }
    a.R = sh->scene_radius; a.Rd = sh->deformation_radius;
    a.wgs = cd_wgs(a.N);
    cd_pack(a);
    int at = 0;
    for (int l = 0; l < a.NL; l++) {
        a.im.w[l] = at;
        at += l == a.NL - 1 ? a.S : (l == 0 ? a.E : a.S) * (a.S + 4);
    }
    for (int l = 0; l < a.NL; l++) {
        a.im.b[l] = at;
        at += l == a.NL - 1 ? 1 : a.S;
    }
    a.im.wlast = a.im.w[a.NL - 1];
    a.im.blast = a.im.b[a.NL - 1];
    return G4S_OK;
}

// The backward's workspace: dx and the partials; the regulariser pair (REG) has rpart before them -- alone the workspace of
// its forward, `forward_bytes` -- and coef behind.
struct DeformLayout { size_t rpart, dx, partials, coef, forward_bytes, bytes; };
static DeformLayout cd_layout(const DeformArgs& a, bool reg) {
    WorkspaceCursor c;
    DeformLayout L{};
    if (reg) L.rpart = c.take((size_t)a.n * a.wgs * 8);
    L.forward_bytes = c.off;
    L.dx = c.take((size_t)a.n * a.N * a.E * 4);
    L.partials = c.take((size_t)a.n * a.wgs * a.gcount * 4);
    if (reg) L.coef = c.take((size_t)a.n * a.N * 4);
    L.bytes = c.off;
    return L;
}

extern "C" size_t g4s_chart_deform_workspace(const g4s_chart_deform_shape* shape) {
    DeformArgs a;
    if (cd_shape(a, shape)) return 0;
    return cd_layout(a, false).bytes + WORKSPACE_BASE_SLACK;
}

// what forward and backward check alike
static int cd_inputs(DeformArgs& a, const g4s_chart_deform_shape* shape, const float* const* levels, const float* depth_encoding,
                     const float* const* weights, const float* const* biases, const float* depth_coords, const float* cameras,
                     const float* initial_depths) {
    if (int rc = cd_shape(a, shape)) return rc;
    if (!levels || !weights || !biases || !cameras || !initial_depths) return null_pointer();
    if (a.B > 0 && (!depth_encoding || !depth_coords))
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart deform: bins > 0 needs depth_encoding and depth_coords");
    for (int l = 0; l < a.L; l++) {
        if (!levels[l]) return null_pointer();
        a.level[l] = levels[l];
    }
    for (int l = 0; l < a.NL; l++) {
        if (!weights[l] || !biases[l]) return null_pointer();
        a.w[l] = weights[l]; a.b[l] = biases[l];
    }
    a.denc = a.B > 0 ? depth_encoding : nullptr;
    a.coords = depth_coords; a.cams = cameras; a.d0 = initial_depths;
    return G4S_OK;
}

#define CD_LAUNCH(kernel, REG, a, grid, s)                                                                  \
    do {                                                                                                 \
        const int et_ = (a).E / 16, st_ = (a).S / 16;                                                    \
        if (et_ == 1 && st_ == 2) hipLaunchKernelGGL((kernel<1, 2, REG>), grid, dim3(256), 0, s, a);          \
        else if (et_ == 2 && st_ == 2) hipLaunchKernelGGL((kernel<2, 2, REG>), grid, dim3(256), 0, s, a);     \
        else if (et_ == 4 && st_ == 2) hipLaunchKernelGGL((kernel<4, 2, REG>), grid, dim3(256), 0, s, a);     \
        else if (et_ == 1 && st_ == 4) hipLaunchKernelGGL((kernel<1, 4, REG>), grid, dim3(256), 0, s, a);     \
        else if (et_ == 2 && st_ == 4) hipLaunchKernelGGL((kernel<2, 4, REG>), grid, dim3(256), 0, s, a);     \
        else hipLaunchKernelGGL((kernel<4, 4, REG>), grid, dim3(256), 0, s, a);                               \
    } while (0)

// the gradient pointers of a backward, checked and stored
static int cd_gradients(DeformArgs& a, float* const* dL_dlevels, float* dL_ddepth_encoding, float* const* dL_dweights,
                        float* const* dL_dbiases) {
    if (!dL_dlevels || !dL_dweights || !dL_dbiases || (a.B > 0 && !dL_ddepth_encoding)) return null_pointer();
    for (int l = 0; l < a.L; l++) {
        if (!dL_dlevels[l]) return null_pointer();
        a.dlevel[l] = dL_dlevels[l];
    }
    for (int l = 0; l < a.NL; l++) {
        if (!dL_dweights[l] || !dL_dbiases[l]) return null_pointer();
        a.dw[l] = dL_dweights[l]; a.db[l] = dL_dbiases[l];
    }
    a.ddenc = dL_ddepth_encoding;
    return G4S_OK;
}

// the workspace of `need` bytes, checked, and its ranges; the regulariser's forward has rpart only (need = its own query)
static int cd_workspace(DeformArgs& a, bool reg, char* workspace, size_t workspace_bytes, size_t need, bool forward_only = false) {
    if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    const DeformLayout L = cd_layout(a, reg);
    if (reg) a.rpart = workspace_at<double>(workspace, L.rpart);
    if (forward_only) return G4S_OK;
    a.dx = workspace_at<float>(workspace, L.dx);
    a.partials = workspace_at<float>(workspace, L.partials);
    if (reg) a.coef = workspace_at<float>(workspace, L.coef);
    return G4S_OK;
}

// the backward: dL/dx and the workgroups' partials, the depth encoding's share, the fold, one gather per level
template <bool REG>
static void cd_launch_backward(const DeformArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)(a.n * a.wgs));
    CD_LAUNCH(chart_deform_bwd_kernel, REG, a, grid, s);
    if (a.denc) hipLaunchKernelGGL(chart_deform_denc_kernel, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(chart_deform_fold_kernel<REG>, dim3(blocks256(a.gcount), (unsigned)a.n), dim3(256), 0, s, a);
    for (int l = 0; l < a.L; l++)
        hipLaunchKernelGGL(chart_deform_level_kernel<REG>, dim3(blocks256(a.lh[l] * a.lw[l] * (a.C / 4)), (unsigned)a.n), dim3(256), 0, s, a, l);
}

extern "C" int g4s_chart_deform_forward(const g4s_chart_deform_shape* shape, const float* const* levels,
                                        const float* depth_encoding, const float* const* weights, const float* const* biases,
                                        const float* depth_coords, const float* cameras, const float* initial_depths,
                                        float* depths, float* delta, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    DeformArgs a;
    if (int rc = cd_inputs(a, shape, levels, depth_encoding, weights, biases, depth_coords, cameras, initial_depths)) return rc;
    if (!depths) return null_pointer();
    (void)workspace; (void)workspace_bytes;  // the forward needs none
    a.depths = depths; a.delta = delta;
    const dim3 grid((unsigned)(a.n * a.wgs));
    CD_LAUNCH(chart_deform_fwd_kernel, false, a, grid, s);
    return stage_done("chart_deform_forward", s);
}

extern "C" int g4s_chart_deform_backward(const g4s_chart_deform_shape* shape, const float* const* levels,
                                         const float* depth_encoding, const float* const* weights, const float* const* biases,
                                         const float* depth_coords, const float* cameras, const float* initial_depths,
                                         const float* dL_ddepths, float* const* dL_dlevels, float* dL_ddepth_encoding,
                                         float* const* dL_dweights, float* const* dL_dbiases, char* workspace,
                                         size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    DeformArgs a;
    if (int rc = cd_inputs(a, shape, levels, depth_encoding, weights, biases, depth_coords, cameras, initial_depths)) return rc;
    if (!dL_ddepths) return null_pointer();
    if (int rc = cd_gradients(a, dL_dlevels, dL_ddepth_encoding, dL_dweights, dL_dbiases)) return rc;
    if (int rc = cd_workspace(a, false, workspace, workspace_bytes, g4s_chart_deform_workspace(shape))) return rc;
    a.g = dL_ddepths;
    cd_launch_backward<false>(a, s);
    return stage_done("chart_deform_backward", s);
}

// ---- the weighted deformation with the encoding regularisers, and the confidence -------------------------------------
static int cd_reg_flags(const DeformArgs& a, int reg_flags) {
    if (reg_flags & ~(CD_REG_NORM | CD_REG_TV))
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart deform: reg_flags has bits 0 (norm) and 1 (total variation) only, got %d", reg_flags);
    if ((reg_flags & CD_REG_TV) && a.B < 2)
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart deform: the total variation needs at least 2 depth bins, got %d", a.B);
    return G4S_OK;
}

extern "C" size_t g4s_chart_deform_reg_workspace(const g4s_chart_deform_shape* shape, int reg_flags) {
    DeformArgs a;
    if (cd_shape(a, shape) || cd_reg_flags(a, reg_flags)) return 0;
    return cd_layout(a, true).bytes + WORKSPACE_BASE_SLACK;
}

extern "C" size_t g4s_chart_deform_reg_forward_workspace(const g4s_chart_deform_shape* shape, int reg_flags) {
    DeformArgs a;
    if (cd_shape(a, shape) || cd_reg_flags(a, reg_flags)) return 0;
    return cd_layout(a, true).forward_bytes + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_chart_deform_reg_forward(const g4s_chart_deform_shape* shape, const float* const* levels,
                                            const float* depth_encoding, const float* const* weights, const float* const* biases,
                                            const float* depth_coords, const float* cameras, const float* initial_depths,
                                            const float* encoding_weights, int reg_flags, float* depths, float* delta,
                                            float* reg_out, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    DeformArgs a;
    if (int rc = cd_inputs(a, shape, levels, depth_encoding, weights, biases, depth_coords, cameras, initial_depths)) return rc;
    if (int rc = cd_reg_flags(a, reg_flags)) return rc;
    if (!depths || (reg_flags && !reg_out)) return null_pointer();
    if (reg_flags & CD_REG_NORM) {  // the partial sums of r(p): the head of the workspace
        if (int rc = cd_workspace(a, true, workspace, workspace_bytes, g4s_chart_deform_reg_forward_workspace(shape, reg_flags), true))
            return rc;
    }
    a.depths = depths; a.delta = delta; a.encw = encoding_weights; a.flags = reg_flags; a.reg_out = reg_out;
    const dim3 grid((unsigned)(a.n * a.wgs));
    CD_LAUNCH(chart_deform_fwd_kernel, true, a, grid, s);
    if (reg_out) hipLaunchKernelGGL(chart_deform_reg_kernel, dim3(1), dim3(256), 0, s, a);
    return stage_done("chart_deform_reg_forward", s);
}

extern "C" int g4s_chart_deform_reg_backward(const g4s_chart_deform_shape* shape, const float* const* levels,
                                             const float* depth_encoding, const float* const* weights, const float* const* biases,
                                             const float* depth_coords, const float* cameras, const float* initial_depths,
                                             const float* encoding_weights, int reg_flags, const float* dL_ddepths,
                                             const float* dL_dreg, float* const* dL_dlevels, float* dL_ddepth_encoding,
                                             float* const* dL_dweights, float* const* dL_dbiases, char* workspace,
                                             size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    DeformArgs a;
    if (int rc = cd_inputs(a, shape, levels, depth_encoding, weights, biases, depth_coords, cameras, initial_depths)) return rc;
    if (int rc = cd_reg_flags(a, reg_flags)) return rc;
    if (!dL_ddepths || (reg_flags && !dL_dreg)) return null_pointer();
    if (int rc = cd_gradients(a, dL_dlevels, dL_ddepth_encoding, dL_dweights, dL_dbiases)) return rc;
    if (int rc = cd_workspace(a, true, workspace, workspace_bytes, g4s_chart_deform_reg_workspace(shape, reg_flags))) return rc;
    a.g = dL_ddepths; a.encw = encoding_weights; a.flags = reg_flags; a.dreg = dL_dreg;
    cd_launch_backward<true>(a, s);
    return stage_done("chart_deform_reg_backward", s);
}

extern "C" int g4s_chart_confidence_forward(long long count, const float* raw, float* confidence, float* encoding_weights,
                                            void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (count <= 0 || count > 2147483647ll)
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart confidence: the element count must be 1 to 2^31 - 1, got %lld", count);
    if (!raw || !confidence) return null_pointer();
    hipLaunchKernelGGL(chart_confidence_fwd_kernel, dim3(blocks256(count)), dim3(256), 0, s, count, raw, confidence,
                       encoding_weights);
    return stage_done("chart_confidence_forward", s);
}

extern "C" int g4s_chart_confidence_backward(long long count, const float* raw, const float* dL_dconfidence, float* dL_draw,
                                             void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (count <= 0 || count > 2147483647ll)
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart confidence: the element count must be 1 to 2^31 - 1, got %lld", count);
    if (!raw || !dL_dconfidence || !dL_draw) return null_pointer();
    hipLaunchKernelGGL(chart_confidence_bwd_kernel, dim3(blocks256(count)), dim3(256), 0, s, count, raw, dL_dconfidence,
                       dL_draw);
    return stage_done("chart_confidence_backward", s);
}
