// TSDF fusion of rendered depth and marching-cubes extraction (include/g4s_render_maps.h, TSDF section; the
// semantics stated there are the contract, tests/tsdf_ref.py restates them in numpy).
//
// Per view:  emit (one thread per pixel: the blocks its truncation segment crosses, exact 3-D DDA, a fixed number of
// key slots per pixel padded with the sentinel) -> LDS radix sort of the packed keys (binning.hip) -> unique ->
// lookup in the volume's sorted (key, slot) table -> compaction of the new keys -> [host: capacity] -> merge (a
// merge-path scatter: every entry's output position is its own index plus its rank in the other list) -> integrate
// (one workgroup per touched block, one voxel per lane).
// Extraction:  count (one workgroup per allocated block, a 10^3 apron of tsdf values in LDS) -> fixed-order exclusive
// scans of the per-block vertex / triangle counts -> [host: sizes] -> emit.
// Nothing is accumulated with atomics: every output position is a scan result, so every result is bit-reproducible.
#include <math.h>

#include "../g4s_internal.h"
#include "../g4s_device.h"
#include "mesh_common.h"
#include "scan.h"
#include "tsdf_mc_table.h"

namespace g4s {

// ---- TSDF fusion and marching cubes (include/g4s_render_maps.h, TSDF section) ---------------------------
constexpr int TSDF_BLOCK = 8;                  // voxels per block edge
constexpr float TSDF_COORD_LIMIT = 1.0e6f;     // |segment end point| in block units: beyond it a pixel allocates nothing
struct TsdfView {
    int W, H;
    float fx, fy, cx, cy;
    float E[12];        // world -> camera, rows of world_view_transform.T
    float C[12];        // camera -> world: the rigid inverse of E (host, double precision, rounded once)
    float voxel_size, block_size, sdf_trunc, depth_trunc;
};
struct TsdfViewLayout {  // byte offsets into the per-view workspace
    size_t n, keys_a, keys_b, hist, bin_total, flag, pos, lb, new_keys, touched_slot, chunks, words, bytes;
};
struct TsdfMcLayout {    // byte offsets into the extraction workspace
    size_t vpre, nv, nt, vbase, tbase, chunks, words, bytes;
};

constexpr int TSDF_VOX = TSDF_BLOCK * TSDF_BLOCK * TSDF_BLOCK;  // 512: voxels per block = lanes per workgroup
constexpr uint64_t KEY_SENTINEL = ~0ull;                         // above every packed key (bit 63 of a key is 0)
constexpr int KEY_BIAS = 1 << 20;

__host__ __device__ inline uint64_t pack_key(int bx, int by, int bz) {
    return ((uint64_t)(uint32_t)(bx + KEY_BIAS) << 42) | ((uint64_t)(uint32_t)(by + KEY_BIAS) << 21) |
           (uint64_t)(uint32_t)(bz + KEY_BIAS);
}
__device__ inline int key_coord(uint64_t k, int shift) { return (int)((k >> shift) & 0x1FFFFFu) - KEY_BIAS; }
__device__ inline bool coord_ok(int c) { return c >= -KEY_BIAS && c < KEY_BIAS; }

// first index i in [0, n) with a[i] >= key (n if none)
__device__ inline int lower_bound_u64(const uint64_t* __restrict__ a, int n, uint64_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Exclusive scan over a 512-thread workgroup (8 waves); `smem8` = 8 words of LDS.  Two barriers.
__device__ inline uint32_t block512_excl_scan_u32(uint32_t v, uint32_t* smem8, uint32_t* total) {
    const int w = (int)(threadIdx.x >> 6);
    const uint32_t inc = wave_incl_scan_u32(v);
    __syncthreads();
    if (lane_id() == 63) smem8[w] = inc;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t s = smem8[i];
        base += i < w ? s : 0u;
        sum += s;
    }
    *total = sum;
    return base + inc - v;
}

// ---------------------------------------------------------------------------------------------------------------------
// per view

__device__ inline bool pixel_depth(const TsdfView& c, const float* __restrict__ depth, const float* __restrict__ mask,
                                   int pix, float* d) {
    const float v = depth[pix];
    if (!(v > 0.0f && v <= c.depth_trunc)) return false;
    if (mask != nullptr && !(mask[pix] >= 0.5f)) return false;
    *d = v;
    return true;
}

// world point of camera-space (x, y, z): C * (x, y, z, 1), rows left to right
__device__ inline void cam_to_world(const TsdfView& c, float x, float y, float z, float* w) {
#pragma unroll
    for (int r = 0; r < 3; r++) w[r] = ((c.C[4 * r] * x + c.C[4 * r + 1] * y) + c.C[4 * r + 2] * z) + c.C[4 * r + 3];
}

// keys[pix * cap + k]: the blocks crossed by pixel pix's segment between depths d - sdf_trunc and d + sdf_trunc, in DDA
// order, then KEY_SENTINEL.  cap = g4s_tsdf_blocks_per_pixel(): never reached by exact arithmetic (the walk is cut there).
__global__ void __launch_bounds__(256) tsdf_emit_kernel(TsdfView c, const float* __restrict__ depth,
                                                        const float* __restrict__ mask, int cap,
                                                        uint64_t* __restrict__ keys) {
    const int pix = (int)(blockIdx.x * 256 + threadIdx.x);
    if (pix >= c.W * c.H) return;
    uint64_t* out = keys + (size_t)pix * cap;
    int n = 0;
    float d;
    if (pixel_depth(c, depth, mask, pix, &d)) {
        const float rx = ((float)(pix % c.W) - c.cx) / c.fx, ry = ((float)(pix / c.W) - c.cy) / c.fy;
        const float z0 = d - c.sdf_trunc, z1 = d + c.sdf_trunc;
        float p0[3], p1[3], a[3], b[3];
        cam_to_world(c, rx * z0, ry * z0, z0, p0);
        cam_to_world(c, rx * z1, ry * z1, z1, p1);
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            a[i] = p0[i] / c.block_size;
            b[i] = p1[i] / c.block_size;
            ok = ok && fabsf(a[i]) < TSDF_COORD_LIMIT && fabsf(b[i]) < TSDF_COORD_LIMIT;  // also rejects NaN
        }
        if (ok) {
            int cell[3], end[3], step[3];
            float dir[3];
#pragma unroll
            for (int i = 0; i < 3; i++) {
                cell[i] = (int)floorf(a[i]);
                end[i] = (int)floorf(b[i]);
                dir[i] = b[i] - a[i];
                step[i] = end[i] > cell[i] ? 1 : -1;
            }
            out[n++] = pack_key(cell[0], cell[1], cell[2]);
            while (n < cap && (cell[0] != end[0] || cell[1] != end[1] || cell[2] != end[2])) {
                // the axis whose next boundary the segment reaches first; ties go to the lower axis
                int best = -1;
                float tb = 0.0f;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    if (cell[i] == end[i]) continue;
                    const float t = ((float)(cell[i] + (step[i] > 0 ? 1 : 0)) - a[i]) / dir[i];
                    if (best < 0 || t < tb) { best = i; tb = t; }
                }
                cell[best] += step[best];
                out[n++] = pack_key(cell[0], cell[1], cell[2]);
            }
        }
    }
    for (; n < cap; n++) out[n] = KEY_SENTINEL;
}

// flag[i] = 1 for the first key of each run of equal sorted keys (the sentinel excluded)
__global__ void __launch_bounds__(256) tsdf_unique_flags_kernel(const uint64_t* __restrict__ sorted, int n,
                                                                uint32_t* __restrict__ flag) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const uint64_t k = sorted[i];
    flag[i] = (k != KEY_SENTINEL && (i == 0 || sorted[i - 1] != k)) ? 1u : 0u;
}

// out[pos[i]] = in[i] where flag[i]
__global__ void __launch_bounds__(256) compact_u64_kernel(const uint64_t* __restrict__ in, const uint32_t* __restrict__ flag,
                                                          const uint32_t* __restrict__ pos, int n,
                                                          uint64_t* __restrict__ out) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i < n && flag[i]) out[pos[i]] = in[i];
}

// touched key r (< *d_m): lb[r] = its lower bound in the table, newflag[r] = not in the table; 0 beyond *d_m
__global__ void __launch_bounds__(256) tsdf_lookup_kernel(const uint64_t* __restrict__ uniq, const uint32_t* __restrict__ d_m,
                                                          int n, const uint64_t* __restrict__ table, int n_blocks,
                                                          int* __restrict__ lb, uint32_t* __restrict__ newflag) {
    const int r = (int)(blockIdx.x * 256 + threadIdx.x);
    if (r >= n) return;
    if (r >= (int)*d_m) {
        newflag[r] = 0;
        return;
    }
    const uint64_t k = uniq[r];
    const int l = lower_bound_u64(table, n_blocks, k);
    lb[r] = l;
    newflag[r] = (l < n_blocks && table[l] == k) ? 0u : 1u;
}

// merge, old entries: position = own index + number of new keys below it
__global__ void __launch_bounds__(256) tsdf_merge_old_kernel(const uint64_t* __restrict__ keys_in,
                                                             const int* __restrict__ slots_in, int n_blocks,
                                                             const uint64_t* __restrict__ new_keys, int n_new,
                                                             uint64_t* __restrict__ keys_out, int* __restrict__ slots_out) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n_blocks) return;
    const uint64_t k = keys_in[i];
    const int pos = i + lower_bound_u64(new_keys, n_new, k);
    keys_out[pos] = k;
    slots_out[pos] = slots_in[i];
}

// merge, touched keys: the new ones take slot n_blocks + (their rank among the new keys) and position rank + lower bound;
// every touched key learns its slot for the integration
__global__ void __launch_bounds__(256) tsdf_merge_touched_kernel(const uint64_t* __restrict__ uniq, int m,
                                                                 const int* __restrict__ lb, const uint32_t* __restrict__ newflag,
                                                                 const uint32_t* __restrict__ new_rank,
                                                                 const int* __restrict__ slots_in, int n_blocks,
                                                                 uint64_t* __restrict__ keys_out, int* __restrict__ slots_out,
                                                                 int* __restrict__ touched_slot) {
    const int r = (int)(blockIdx.x * 256 + threadIdx.x);
    if (r >= m) return;
    if (newflag[r]) {
        const int rank = (int)new_rank[r];
        const int slot = n_blocks + rank;
        keys_out[rank + lb[r]] = uniq[r];
        slots_out[rank + lb[r]] = slot;
        touched_slot[r] = slot;
    } else {
        touched_slot[r] = slots_in[lb[r]];
    }
}

// the voxels of slots [first, first + count): tsdf = weight = colour = 0
__global__ void __launch_bounds__(TSDF_VOX) tsdf_init_kernel(int first, float* __restrict__ tsdf, float* __restrict__ weight,
                                                              float* __restrict__ color) {
    const size_t v = (size_t)(first + (int)blockIdx.x) * TSDF_VOX + threadIdx.x;
    tsdf[v] = 0.0f;
    weight[v] = 0.0f;
    color[3 * v] = 0.0f;
    color[3 * v + 1] = 0.0f;
    color[3 * v + 2] = 0.0f;
}

__device__ inline float quantise_rgb(float x) {
    // clamp to [0, 1] (NaN -> 0), * 255, truncate: what numpy's uint8 cast does to values in [0, 255]
    const float y = fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f;
    return (float)(uint32_t)y;
}

// one workgroup per touched block, one voxel per lane (x fastest)
__global__ void __launch_bounds__(TSDF_VOX) tsdf_integrate_kernel(TsdfView c, const float* __restrict__ depth,
                                                                   const float* __restrict__ mask, const float* __restrict__ rgb,
                                                                   const uint64_t* __restrict__ uniq,
                                                                   const int* __restrict__ touched_slot,
                                                                   float* __restrict__ tsdf, float* __restrict__ weight,
                                                                   float* __restrict__ color) {
    const uint64_t key = uniq[blockIdx.x];
    const int slot = touched_slot[blockIdx.x];
    const int t = (int)threadIdx.x;
    const int g[3] = {key_coord(key, 42) * TSDF_BLOCK + (t & 7), key_coord(key, 21) * TSDF_BLOCK + ((t >> 3) & 7),
                      key_coord(key, 0) * TSDF_BLOCK + (t >> 6)};
    float p[3], q[3];
#pragma unroll
    for (int i = 0; i < 3; i++) p[i] = ((float)g[i] + 0.5f) * c.voxel_size;
#pragma unroll
    for (int r = 0; r < 3; r++) q[r] = ((c.E[4 * r] * p[0] + c.E[4 * r + 1] * p[1]) + c.E[4 * r + 2] * p[2]) + c.E[4 * r + 3];
    const float z = q[2];
    if (!(z > 0.0f)) return;
    const float fu = floorf((c.fx * q[0]) / z + c.cx + 0.5f), fv = floorf((c.fy * q[1]) / z + c.cy + 0.5f);
    if (!(fu >= 0.0f && fu <= (float)(c.W - 1) && fv >= 0.0f && fv <= (float)(c.H - 1))) return;
    const int u = (int)fu, v = (int)fv, pix = v * c.W + u;
    float d;
    if (!pixel_depth(c, depth, mask, pix, &d)) return;
    const float a = (fu - c.cx) / c.fx, b = (fv - c.cy) / c.fy;
    const float sdf = (d - z) * sqrtf((1.0f + a * a) + b * b);
    if (!(sdf > -c.sdf_trunc)) return;
    const float tt = fminf(1.0f, sdf / c.sdf_trunc);
    const size_t vox = (size_t)slot * TSDF_VOX + t;
    const float w = weight[vox], w1 = w + 1.0f;
    tsdf[vox] = (tsdf[vox] * w + tt) / w1;
    const size_t plane = (size_t)c.W * c.H;
#pragma unroll
    for (int k = 0; k < 3; k++) color[3 * vox + k] = (color[3 * vox + k] * w + quantise_rgb(rgb[k * plane + pix])) / w1;
    weight[vox] = w1;
}

// ---------------------------------------------------------------------------------------------------------------------
// extraction

constexpr int APRON = TSDF_BLOCK + 2;          // local coordinates -1 .. 8
constexpr int APRON_VOX = APRON * APRON * APRON;  // 1000
constexpr int CUBES = TSDF_BLOCK + 1;          // cube lower corners -1 .. 7
constexpr int CUBE_N = CUBES * CUBES * CUBES;  // 729

struct McShared {
    float f[APRON_VOX];        // tsdf where allocated with weight > 0, else NaN
    uint16_t cube[CUBE_N];     // bit 8: all eight corners valid; bits 0..7: configuration
    int nbr[27];               // table position of the neighbour block (dx, dy, dz) in -1..1, or -1
    uint32_t scan[8];
};

__device__ inline int apron_idx(int x, int y, int z) { return (x + 1) + APRON * ((y + 1) + APRON * (z + 1)); }
__device__ inline int cube_idx(int x, int y, int z) { return (x + 1) + CUBES * ((y + 1) + CUBES * (z + 1)); }
__device__ inline int nbr_idx(int dx, int dy, int dz) { return (dx + 1) + 3 * ((dy + 1) + 3 * (dz + 1)); }
__device__ inline int block_of(int l) { return l < 0 ? -1 : (l >= TSDF_BLOCK ? 1 : 0); }

// neighbour table, apron, cube flags of table position p
__device__ void mc_stage(McShared& s, const uint64_t* __restrict__ keys, const int* __restrict__ slots, int n_blocks,
                         const float* __restrict__ tsdf, const float* __restrict__ weight, int p) {
    const int t = (int)threadIdx.x;
    const uint64_t key = keys[p];
    if (t < 27) {
        const int bx = key_coord(key, 42) + t % 3 - 1, by = key_coord(key, 21) + (t / 3) % 3 - 1,
                  bz = key_coord(key, 0) + t / 9 - 1;
        int pos = -1;
        if (coord_ok(bx) && coord_ok(by) && coord_ok(bz)) {
            const uint64_t k = pack_key(bx, by, bz);
            const int l = lower_bound_u64(keys, n_blocks, k);
            if (l < n_blocks && keys[l] == k) pos = l;
        }
        s.nbr[t] = pos;
    }
    __syncthreads();
    for (int i = t; i < APRON_VOX; i += TSDF_VOX) {
        const int x = i % APRON - 1, y = (i / APRON) % APRON - 1, z = i / (APRON * APRON) - 1;
        const int nb = s.nbr[nbr_idx(block_of(x), block_of(y), block_of(z))];
        float f = __builtin_nanf("");
        if (nb >= 0) {
            const size_t v = (size_t)slots[nb] * TSDF_VOX + (size_t)((x & 7) + 8 * (y & 7) + 64 * (z & 7));
            if (weight[v] > 0.0f) f = tsdf[v];
        }
        s.f[i] = f;
    }
    __syncthreads();
    for (int i = t; i < CUBE_N; i += TSDF_VOX) {
        const int x = i % CUBES - 1, y = (i / CUBES) % CUBES - 1, z = i / (CUBES * CUBES) - 1;
        uint32_t cfg = 0, valid = 1;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const float f = s.f[apron_idx(x + (c & 1), y + ((c >> 1) & 1), z + (c >> 2))];
            valid &= f == f ? 1u : 0u;
            cfg |= (f < 0.0f ? 1u : 0u) << c;
        }
        s.cube[i] = (uint16_t)(valid << 8 | cfg);
    }
    __syncthreads();
}

__device__ inline bool cube_valid(const McShared& s, int x, int y, int z) { return (s.cube[cube_idx(x, y, z)] >> 8) != 0; }

// bit a: voxel (x, y, z) (local 0..7) owns a vertex on its +a edge -- a sign change between two valid voxels that a
// valid cube uses
__device__ inline uint32_t owned_edges(const McShared& s, int x, int y, int z) {
    const float f0 = s.f[apron_idx(x, y, z)];
    uint32_t mask = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float f1 = s.f[apron_idx(x + (a == 0), y + (a == 1), z + (a == 2))];
        if (!(f0 == f0 && f1 == f1) || (f0 < 0.0f) == (f1 < 0.0f)) continue;
        // the four cubes around the edge: lower corners offset by 0 / -1 along the two other axes
        bool used = false;
#pragma unroll
        for (int o = 0; o < 4; o++) {
            const int d1 = -(o & 1), d2 = -(o >> 1);
            const int cx = x + (a == 0 ? 0 : d1), cy = y + (a == 1 ? 0 : (a == 0 ? d1 : d2)), cz = z + (a == 2 ? 0 : d2);
            used = used || cube_valid(s, cx, cy, cz);
        }
        if (used) mask |= 1u << a;
    }
    return mask;
}

// per block: vertex and triangle counts, and per voxel (exclusive vertex prefix in the block << 3 | owned-edge mask)
__global__ void __launch_bounds__(TSDF_VOX) tsdf_mc_count_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ slots,
                                                                  int n_blocks, const float* __restrict__ tsdf,
                                                                  const float* __restrict__ weight,
                                                                  uint32_t* __restrict__ vpre, uint32_t* __restrict__ nv,
                                                                  uint32_t* __restrict__ nt) {
    __shared__ McShared s;
    const int p = (int)blockIdx.x, t = (int)threadIdx.x;
    mc_stage(s, keys, slots, n_blocks, tsdf, weight, p);
    const int x = t & 7, y = (t >> 3) & 7, z = t >> 6;
    const uint32_t mask = owned_edges(s, x, y, z);
    const uint32_t cube = s.cube[cube_idx(x, y, z)];
    const uint32_t ntri = (cube >> 8) ? g4s_mc_ntris[cube & 0xFF] : 0u;
    uint32_t tv, tt;
    const uint32_t ex = block512_excl_scan_u32((uint32_t)__builtin_popcount(mask), s.scan, &tv);
    vpre[(size_t)p * TSDF_VOX + t] = ex << 3 | mask;
    (void)block512_excl_scan_u32(ntri, s.scan, &tt);
    if (t == 0) {
        nv[p] = tv;
        nt[p] = tt;
    }
}

// global index of the vertex on the +a edge of local voxel (x, y, z), x, y, z in 0..8 (8: the + neighbour block)
__device__ inline uint32_t vertex_id(const McShared& s, const uint32_t* __restrict__ vpre, const uint32_t* __restrict__ vbase,
                                     int x, int y, int z, int a) {
    const int nb = s.nbr[nbr_idx(block_of(x), block_of(y), block_of(z))];
    const uint32_t w = vpre[(size_t)nb * TSDF_VOX + (size_t)((x & 7) + 8 * (y & 7) + 64 * (z & 7))];
    return vbase[nb] + mc_vertex_rank(w, a);
}

__global__ void __launch_bounds__(TSDF_VOX) tsdf_mc_emit_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ slots,
                                                                 int n_blocks, const float* __restrict__ tsdf,
                                                                 const float* __restrict__ weight, const float* __restrict__ color,
                                                                 float voxel_size, const uint32_t* __restrict__ vpre,
                                                                 const uint32_t* __restrict__ vbase,
                                                                 const uint32_t* __restrict__ tbase, float* __restrict__ verts,
                                                                 float* __restrict__ vcols, int* __restrict__ tris,
                                                                 uint32_t vcap, uint32_t tcap) {
    __shared__ McShared s;
    const int p = (int)blockIdx.x, t = (int)threadIdx.x;
    mc_stage(s, keys, slots, n_blocks, tsdf, weight, p);
    const int x = t & 7, y = (t >> 3) & 7, z = t >> 6;
    const uint64_t key = keys[p];
    const int g[3] = {key_coord(key, 42) * TSDF_BLOCK + x, key_coord(key, 21) * TSDF_BLOCK + y, key_coord(key, 0) * TSDF_BLOCK + z};
    const uint32_t w = vpre[(size_t)p * TSDF_VOX + t];
    uint32_t vi = vbase[p] + (w >> 3);
    const float f0 = s.f[apron_idx(x, y, z)];
    const size_t v0 = (size_t)slots[p] * TSDF_VOX + t;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (!(w >> a & 1u) || vi >= vcap) continue;
        const int x1 = x + (a == 0), y1 = y + (a == 1), z1 = z + (a == 2);
        const float f1 = s.f[apron_idx(x1, y1, z1)];
        const float e = f0 / (f0 - f1);
        const int nb = s.nbr[nbr_idx(block_of(x1), block_of(y1), block_of(z1))];
        const size_t v1 = (size_t)slots[nb] * TSDF_VOX + (size_t)((x1 & 7) + 8 * (y1 & 7) + 64 * (z1 & 7));
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float c = (float)g[i] + 0.5f;
            verts[3 * (size_t)vi + i] = (i == a ? c + e : c) * voxel_size;
            const float c0 = color[3 * v0 + i], c1 = color[3 * v1 + i];
            vcols[3 * (size_t)vi + i] = (c0 + e * (c1 - c0)) / 255.0f;
        }
        vi++;
    }
    const uint32_t cube = s.cube[cube_idx(x, y, z)];
    const uint32_t ntri = (cube >> 8) ? g4s_mc_ntris[cube & 0xFF] : 0u;
    uint32_t tt;
    uint32_t ti = tbase[p] + block512_excl_scan_u32(ntri, s.scan, &tt);
    const signed char* row = g4s_mc_tris[cube & 0xFF];
    for (uint32_t k = 0; k < 3 * ntri && ti + k / 3 < tcap; k++) {
        const McEdge e = mc_edge(row[k], x, y, z);
        tris[3 * (size_t)ti + k] = (int)vertex_id(s, vpre, vbase, e.x, e.y, e.z, e.a);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host sequencing (the entry points below validate every argument before calling these)

TsdfViewLayout tsdf_view_layout(int W, int H, int cap) {
    TsdfViewLayout L{};
    const size_t n = (size_t)W * H * cap;
    WorkspaceCursor c;
    L.n = n;
    L.keys_a = c.take(n * 8);
    L.keys_b = c.take(n * 8);
    L.hist = c.take((size_t)256 * sort_blocks(n, SORT_ITEMS_U64) * 4);
    L.bin_total = c.take(512 * 4);
    L.flag = c.take(n * 4);
    L.pos = c.take(n * 4);
    L.lb = c.take(n * 4);
    L.new_keys = c.take(n * 8);
    L.touched_slot = c.take(n * 4);
    L.chunks = c.take((size_t)scan_chunks((long)n) * 4 + 4);
    L.words = c.take(64);
    L.bytes = c.off;
    return L;
}

TsdfMcLayout tsdf_mc_layout(int n_blocks) {
    TsdfMcLayout L{};
    const size_t nb = (size_t)n_blocks;
    WorkspaceCursor c;
    L.vpre = c.take(nb * TSDF_VOX * 4);
    L.nv = c.take(nb * 4);
    L.nt = c.take(nb * 4);
    L.vbase = c.take(nb * 4);
    L.tbase = c.take(nb * 4);
    L.chunks = c.take((size_t)scan_chunks((long)nb) * 4 + 4);
    L.words = c.take(64);
    L.bytes = c.off;
    return L;
}

// counts[0] = touched blocks, counts[1] = new blocks (one host synchronisation)
hipError_t tsdf_alloc_count(const TsdfView& c, const float* depth, const float* mask, int cap, const uint64_t* table,
                            int n_blocks, char* ws, int* counts, hipStream_t s) {
    const TsdfViewLayout L = tsdf_view_layout(c.W, c.H, cap);
    uint64_t* ka = (uint64_t*)(ws + L.keys_a);
    uint64_t* kb = (uint64_t*)(ws + L.keys_b);
    uint32_t* flag = (uint32_t*)(ws + L.flag);
    uint32_t* pos = (uint32_t*)(ws + L.pos);
    uint32_t* chunks = (uint32_t*)(ws + L.chunks);
    uint32_t* words = (uint32_t*)(ws + L.words);
    const int n = (int)L.n, P = c.W * c.H;
    hipLaunchKernelGGL(tsdf_emit_kernel, dim3((P + 255) / 256), dim3(256), 0, s, c, depth, mask, cap, ka);
    // 64 bits = eight 8-bit passes: the sorted keys end in keys_a, the unique keys are compacted into keys_b
    if (radix_sort_u64_keys(ka, kb, n, 0, 64, (uint32_t*)(ws + L.hist), (uint32_t*)(ws + L.bin_total), s) != 0)
        return hipErrorUnknown;
    const uint64_t* sorted = ka;
    uint64_t* uniq = kb;
    const int g = (n + 255) / 256;
    hipLaunchKernelGGL(tsdf_unique_flags_kernel, dim3(g), dim3(256), 0, s, sorted, n, flag);
    scan_u32(flag, pos, n, chunks, words + 0, s);
    hipLaunchKernelGGL(compact_u64_kernel, dim3(g), dim3(256), 0, s, sorted, flag, pos, n, uniq);
    // flag := new-key flags of the touched keys, pos := their ranks among the new keys
    hipLaunchKernelGGL(tsdf_lookup_kernel, dim3(g), dim3(256), 0, s, uniq, words + 0, n, table, n_blocks, (int*)(ws + L.lb), flag);
    scan_u32(flag, pos, n, chunks, words + 1, s);
    hipLaunchKernelGGL(compact_u64_kernel, dim3(g), dim3(256), 0, s, uniq, flag, pos, n, (uint64_t*)(ws + L.new_keys));
    return read_totals(words, counts, s);
}

hipError_t tsdf_merge(const TsdfViewLayout& L, const uint64_t* keys_in, const int* slots_in, int n_blocks, int m, int n_new,
                      uint64_t* keys_out, int* slots_out, float* tsdf, float* weight, float* color, char* ws, hipStream_t s) {
    if (n_blocks > 0)
        hipLaunchKernelGGL(tsdf_merge_old_kernel, dim3((n_blocks + 255) / 256), dim3(256), 0, s, keys_in, slots_in, n_blocks,
                           (const uint64_t*)(ws + L.new_keys), n_new, keys_out, slots_out);
    if (m > 0)
        hipLaunchKernelGGL(tsdf_merge_touched_kernel, dim3((m + 255) / 256), dim3(256), 0, s, (const uint64_t*)(ws + L.keys_b),
                           m, (const int*)(ws + L.lb), (const uint32_t*)(ws + L.flag), (const uint32_t*)(ws + L.pos),
                           slots_in, n_blocks, keys_out, slots_out, (int*)(ws + L.touched_slot));
    if (n_new > 0)
        hipLaunchKernelGGL(tsdf_init_kernel, dim3(n_new), dim3(TSDF_VOX), 0, s, n_blocks, tsdf, weight, color);
    return hipGetLastError();
}

hipError_t tsdf_integrate(const TsdfView& c, const TsdfViewLayout& L, const float* depth, const float* mask, const float* rgb,
                          int m, float* tsdf, float* weight, float* color, char* ws, hipStream_t s) {
    if (m > 0)
        hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(m), dim3(TSDF_VOX), 0, s, c, depth, mask, rgb,
                           (const uint64_t*)(ws + L.keys_b), (const int*)(ws + L.touched_slot), tsdf, weight, color);
    return hipGetLastError();
}

// totals[0] = vertices, totals[1] = triangles (one host synchronisation)
hipError_t tsdf_extract_count(const uint64_t* keys, const int* slots, int n_blocks, const float* tsdf, const float* weight,
                              char* ws, int* totals, hipStream_t s) {
    const TsdfMcLayout L = tsdf_mc_layout(n_blocks);
    uint32_t* nv = (uint32_t*)(ws + L.nv);
    uint32_t* nt = (uint32_t*)(ws + L.nt);
    uint32_t* chunks = (uint32_t*)(ws + L.chunks);
    uint32_t* words = (uint32_t*)(ws + L.words);
    hipLaunchKernelGGL(tsdf_mc_count_kernel, dim3(n_blocks), dim3(TSDF_VOX), 0, s, keys, slots, n_blocks, tsdf, weight,
                       (uint32_t*)(ws + L.vpre), nv, nt);
    scan_u32(nv, (uint32_t*)(ws + L.vbase), n_blocks, chunks, words + 0, s);  // per-block vertex / triangle bases
    scan_u32(nt, (uint32_t*)(ws + L.tbase), n_blocks, chunks, words + 1, s);
    return read_totals(words, totals, s);
}

hipError_t tsdf_extract_emit(const uint64_t* keys, const int* slots, int n_blocks, const float* tsdf, const float* weight,
                             const float* color, float voxel_size, float* verts, float* vcols, int* tris, int n_vertices,
                             int n_triangles, char* ws, hipStream_t s) {
    const TsdfMcLayout L = tsdf_mc_layout(n_blocks);
    hipLaunchKernelGGL(tsdf_mc_emit_kernel, dim3(n_blocks), dim3(TSDF_VOX), 0, s, keys, slots, n_blocks, tsdf, weight, color,
                       voxel_size, (const uint32_t*)(ws + L.vpre), (const uint32_t*)(ws + L.vbase),
                       (const uint32_t*)(ws + L.tbase), verts, vcols, tris, (uint32_t)n_vertices,
                       (uint32_t)n_triangles);
    return hipGetLastError();
}

}  // namespace g4s

using namespace g4s;

// ---------------------------------------------------------------------------------------------------------------------
// extern "C" entry points (include/g4s_render_maps.h, TSDF section); every argument is checked before any launch
namespace {

int tsdf_check_intrinsic(const float* intrinsic) {
    if (!intrinsic) return null_pointer();
    if (!finite_pos(intrinsic[0]) || !finite_pos(intrinsic[1]) || !finite(intrinsic[2]) || !finite(intrinsic[3]))
        return fail(G4S_ERR_INVALID_ARGUMENT, "intrinsic fx, fy must be positive and cx, cy finite");
    return G4S_OK;
}

int tsdf_view(int W, int H, const float* intrinsic, const float* extrinsic, float voxel_size, float sdf_trunc,
              float depth_trunc, TsdfView* c) {
    if (W <= 0 || H <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "width, height must be positive");
    if (!finite_pos(voxel_size) || !finite_pos(sdf_trunc) || !finite_pos(depth_trunc))
        return fail(G4S_ERR_INVALID_ARGUMENT, "voxel_size, sdf_trunc, depth_trunc must be positive");
    if (tsdf_check_intrinsic(intrinsic) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!extrinsic) return null_pointer();
    *c = TsdfView{};
    c->W = W;
    c->H = H;
    c->fx = intrinsic[0];
    c->fy = intrinsic[1];
    c->cx = intrinsic[2];
    c->cy = intrinsic[3];
    for (int i = 0; i < 12; i++) c->E[i] = extrinsic[i];
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) c->C[4 * r + k] = extrinsic[4 * k + r];
        const double t = ((double)extrinsic[r] * (double)extrinsic[3] + (double)extrinsic[4 + r] * (double)extrinsic[7]) +
                         (double)extrinsic[8 + r] * (double)extrinsic[11];
        c->C[4 * r + 3] = (float)(-t);
    }
    c->voxel_size = voxel_size;
    c->block_size = 8.0f * voxel_size;
    c->sdf_trunc = sdf_trunc;
    c->depth_trunc = depth_trunc;
    return G4S_OK;
}

size_t tsdf_view_bytes(int W, int H, int cap) { return W > 0 && H > 0 && cap > 0 ? tsdf_view_layout(W, H, cap).bytes : 0; }

}  // namespace

extern "C" int g4s_tsdf_blocks_per_pixel(int width, int height, const float* intrinsic, float voxel_size, float sdf_trunc) {
    clear_error();
    if (width <= 0 || height <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "width, height must be positive");
    if (!finite_pos(voxel_size) || !finite_pos(sdf_trunc))
        return fail(G4S_ERR_INVALID_ARGUMENT, "voxel_size, sdf_trunc must be positive");
    if (tsdf_check_intrinsic(intrinsic) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    // the segment's length over its z extent 2 sdf_trunc is at most that of the steepest pixel ray (a frame corner);
    // each axis can then change its block index at most ceil(length / B) + 1 times (the +1 absorbs float rounding)
    const double fx = intrinsic[0], fy = intrinsic[1], cx = intrinsic[2], cy = intrinsic[3];
    const double rx = fmax(fabs(-cx), fabs(width - 1 - cx)) / fx, ry = fmax(fabs(-cy), fabs(height - 1 - cy)) / fy;
    const double len = 2.0 * sdf_trunc * sqrt(1.0 + rx * rx + ry * ry) / (8.0 * voxel_size);
    if (!(len < 1.0e4)) return fail(G4S_ERR_INVALID_ARGUMENT, "sdf_trunc spans more than 10^4 blocks per ray");
    return 1 + 3 * ((int)ceil(len * (1.0 + 1e-6)) + 1);
}

extern "C" size_t g4s_tsdf_workspace(int width, int height, int blocks_per_pixel, int n_blocks) {
    const size_t a = tsdf_view_bytes(width, height, blocks_per_pixel);
    const size_t b = n_blocks > 0 ? tsdf_mc_layout(n_blocks).bytes : 0;
    return (a > b ? a : b) + 256;  // + alignment of the base pointer
}

extern "C" int g4s_tsdf_alloc_count(int width, int height, const float* depth, const float* mask, const float* intrinsic,
                                    const float* extrinsic, float voxel_size, float sdf_trunc, float depth_trunc,
                                    int blocks_per_pixel, const long long* keys, int n_blocks, int* counts, char* workspace,
                                    size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    TsdfView c;
    if (tsdf_view(width, height, intrinsic, extrinsic, voxel_size, sdf_trunc, depth_trunc, &c) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (!depth || !counts || (n_blocks > 0 && !keys)) return null_pointer();
    if (n_blocks < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_blocks must not be negative");
    const int need = g4s_tsdf_blocks_per_pixel(width, height, intrinsic, voxel_size, sdf_trunc);
    if (need < 0) return need;
    if (blocks_per_pixel < need)
        return fail(G4S_ERR_INVALID_ARGUMENT, "blocks_per_pixel %d below the %d this camera needs", blocks_per_pixel, need);
    if ((double)width * height * blocks_per_pixel >= 2147483647.0)
        return fail(G4S_ERR_INVALID_ARGUMENT, "width * height * blocks_per_pixel exceeds 2^31 - 1 keys");
    if (check_workspace(workspace, workspace_bytes, g4s_tsdf_workspace(width, height, blocks_per_pixel, 0)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    return finish(tsdf_alloc_count(c, depth, mask, blocks_per_pixel, (const uint64_t*)keys, n_blocks, align_ptr(workspace),
                                   counts, stream),
                  "tsdf alloc_count");
}

extern "C" int g4s_tsdf_merge(int width, int height, int blocks_per_pixel, const long long* keys_in, const int* slots_in,
                              int n_blocks, int n_touched, int n_new, long long* keys_out, int* slots_out, float* tsdf,
                              float* weight, float* color, int pool_blocks, char* workspace, size_t workspace_bytes,
                              void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (width <= 0 || height <= 0 || blocks_per_pixel <= 0)
        return fail(G4S_ERR_INVALID_ARGUMENT, "width, height, blocks_per_pixel must be positive");
    if (n_blocks < 0 || n_touched < 0 || n_new < 0 || n_new > n_touched)
        return fail(G4S_ERR_INVALID_ARGUMENT, "counts must not be negative (and n_new <= n_touched)");
    if ((n_blocks > 0 && (!keys_in || !slots_in)) || !keys_out || !slots_out || !tsdf || !weight || !color)
        return null_pointer();
    if ((const void*)keys_in == (const void*)keys_out || (const void*)slots_in == (const void*)slots_out)
        return fail(G4S_ERR_INVALID_ARGUMENT, "the new table must not alias the old one");
    if ((long long)n_blocks + n_new > (long long)pool_blocks)
        return fail(G4S_ERR_INVALID_ARGUMENT, "pool of %d blocks cannot hold %d + %d", pool_blocks, n_blocks, n_new);
    if ((double)n_touched > (double)width * height * blocks_per_pixel)
        return fail(G4S_ERR_INVALID_ARGUMENT, "n_touched exceeds the view's key slots");
    if (check_workspace(workspace, workspace_bytes, g4s_tsdf_workspace(width, height, blocks_per_pixel, 0)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    return finish(tsdf_merge(tsdf_view_layout(width, height, blocks_per_pixel), (const uint64_t*)keys_in, slots_in, n_blocks,
                             n_touched, n_new, (uint64_t*)keys_out, slots_out, tsdf, weight, color, align_ptr(workspace),
                             stream),
                  "tsdf merge");
}

extern "C" int g4s_tsdf_integrate(int width, int height, const float* depth, const float* mask, const float* rgb,
                                  const float* intrinsic, const float* extrinsic, float voxel_size, float sdf_trunc,
                                  float depth_trunc, int blocks_per_pixel, int n_touched, float* tsdf, float* weight,
                                  float* color, int pool_blocks, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    TsdfView c;
    if (tsdf_view(width, height, intrinsic, extrinsic, voxel_size, sdf_trunc, depth_trunc, &c) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (!depth || !rgb || !tsdf || !weight || !color) return null_pointer();
    if (blocks_per_pixel <= 0 || n_touched < 0 || pool_blocks < 0)
        return fail(G4S_ERR_INVALID_ARGUMENT, "blocks_per_pixel must be positive, counts not negative");
    if ((double)n_touched > (double)width * height * blocks_per_pixel || n_touched > pool_blocks)
        return fail(G4S_ERR_INVALID_ARGUMENT, "n_touched exceeds the view's key slots or the pool");
    if (check_workspace(workspace, workspace_bytes, g4s_tsdf_workspace(width, height, blocks_per_pixel, 0)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    return finish(tsdf_integrate(c, tsdf_view_layout(width, height, blocks_per_pixel), depth, mask, rgb, n_touched, tsdf,
                                 weight, color, align_ptr(workspace), stream),
                  "tsdf integrate");
}

extern "C" int g4s_tsdf_extract_count(const long long* keys, const int* slots, int n_blocks, const float* tsdf,
                                      const float* weight, int pool_blocks, int* totals, char* workspace,
                                      size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (n_blocks < 0 || pool_blocks < n_blocks)
        return fail(G4S_ERR_INVALID_ARGUMENT, "n_blocks must not be negative nor exceed pool_blocks");
    if (!totals || (n_blocks > 0 && (!keys || !slots || !tsdf || !weight)))
        return null_pointer();
    if (n_blocks == 0) {
        totals[0] = totals[1] = 0;
        return G4S_OK;
    }
    if (check_workspace(workspace, workspace_bytes, g4s_tsdf_workspace(0, 0, 0, n_blocks)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    return finish(tsdf_extract_count((const uint64_t*)keys, slots, n_blocks, tsdf, weight, align_ptr(workspace), totals, stream),
                  "tsdf extract_count");
}

extern "C" int g4s_tsdf_extract_emit(const long long* keys, const int* slots, int n_blocks, const float* tsdf,
                                     const float* weight, const float* color, int pool_blocks, float voxel_size,
                                     float* vertices, float* vertex_colors, int* triangles, int n_vertices,
                                     int n_triangles, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (n_blocks < 0 || pool_blocks < n_blocks || n_vertices < 0 || n_triangles < 0)
        return fail(G4S_ERR_INVALID_ARGUMENT, "counts must not be negative, n_blocks not exceed pool_blocks");
    if (!finite_pos(voxel_size)) return fail(G4S_ERR_INVALID_ARGUMENT, "voxel_size must be positive");
    if ((n_blocks > 0 && (!keys || !slots || !tsdf || !weight || !color)) || (n_vertices > 0 && (!vertices || !vertex_colors)) ||
        (n_triangles > 0 && !triangles))
        return null_pointer();
    if (n_blocks == 0 || n_vertices == 0) return G4S_OK;
    if (check_workspace(workspace, workspace_bytes, g4s_tsdf_workspace(0, 0, 0, n_blocks)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    return finish(tsdf_extract_emit((const uint64_t*)keys, slots, n_blocks, tsdf, weight, color, voxel_size, vertices,
                                    vertex_colors, triangles, n_vertices, n_triangles, align_ptr(workspace), stream),
                  "tsdf extract_emit");
}
