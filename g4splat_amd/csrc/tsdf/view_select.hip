// View selection (include/g4s_render_maps.h, "View selection"; the semantics stated there are the contract,
// tests/view_selection_ref.py restates them in numpy): which points each candidate camera sees, as bits; how many points
// every pair of cameras shares, as integers; and farthest-point sampling of a batch of clouds.
//
// Bits:     a lane owns a point (12 bytes, loaded once, four points per lane), the camera records are read wave-uniformly
//           (vis_view.h: THE projection), and the ballot of "in image && z > 0" IS the 64-point word of that camera.  A
//           workgroup owns 1024 consecutive points = 16 words per camera; the ballots of a tile of 16 cameras are parked in
//           LDS and leave as one 128-byte line per camera row instead of one isolated 8-byte store per (wave, camera).
// Counts:   counts[i][j] = sum over w of popcount(words[i][w] & words[j][w]).  A workgroup stages a chunk of words of two
//           tiles of 16 cameras in LDS and a thread owns one pair of the 16 x 16; tiles with tj >= ti only, the result is
//           mirrored.  A thread keeps its integer sum over every chunk its workgroup walks and ends with ONE integer atomic
//           per (pair, workgroup); integer sums do not depend on the order.  No float atomics anywhere.
// Sampling: one launch per round over (blocks per cloud, clouds).  A launch reads the previous round's winner, lowers the
//           running minimum and folds (float bits of dist << 32) | ~n -- dist >= 0: the bits order like the values, and of
//           equal distances the smallest n has the largest word -- per thread, wave and workgroup into the cloud's slot of
//           the round with a 64-bit unsigned atomic max: any execution order gives the same word.  A last small kernel
//           decodes the words and gathers the points.  No cooperative launch, no grid-wide spinning.
//
// Byte model (P points, C cameras, W = ceil(P / 64) words per row, T = ceil(C / 16) tiles):
//   bits     reads 12 P bytes of points and 80 C bytes of records per workgroup (cache resident); writes C / 8 bytes per
//            point, 8 C W in all, each row in lines of 128 bytes.
//   counts   reads every row once per tile pair it is part of: 8 W bytes * (T + 1) per camera instead of 8 W * C, i.e.
//            about C / 16 times; writes at most 2 * 4 bytes per (pair, workgroup), at most 2048 workgroups.
//   sampling per round and point 12 bytes of coordinates and 4 bytes of running minimum read, 4 bytes written (round 1
//            reads no minimum: it is 1e10 everywhere); one 8-byte atomic per workgroup.
#include <vector>

#include "../g4s_internal.h"
#include "../g4s_device.h"
#include "../../../include/g4s_render_maps.h"
#include "mesh_common.h"
#include "vis_view.h"

namespace g4s {

// A candidate camera is a VisView without maps: maps.W, maps.H carry its size, the pointers are NULL and never read.
constexpr int BITS_POINTS = 1024;              // points per workgroup of the bits kernel
constexpr int BITS_WORDS = BITS_POINTS / 64;   // = words per camera row and workgroup: one 128-byte line
constexpr int CAM_TILE = 16;

__global__ void __launch_bounds__(256) view_bits_kernel(int n, const float* __restrict__ points,
                                                        const VisView* __restrict__ views, int n_views, int n_words,
                                                        unsigned long long* __restrict__ words) {
    __shared__ unsigned long long line[CAM_TILE][BITS_WORDS];
    const long long first = (long long)blockIdx.x * BITS_POINTS;
    const int wave = (int)(threadIdx.x >> 6);
    float px[4], py[4], pz[4];
    bool there[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {  // word 4 k + wave of the workgroup: points first + 256 k + threadIdx.x
        const long long i = first + 256 * k + (long long)threadIdx.x;
        there[k] = i < n;
        const size_t at = 3 * (size_t)(there[k] ? i : 0);
        px[k] = there[k] ? points[at] : 0.0f;
        py[k] = there[k] ? points[at + 1] : 0.0f;
        pz[k] = there[k] ? points[at + 2] : 0.0f;
    }
    const long long word0 = first >> 6;
    const int out_cam = (int)(threadIdx.x >> 4), out_word = (int)(threadIdx.x & 15);
    for (int c0 = 0; c0 < n_views; c0 += CAM_TILE) {  // workgroup-uniform
        const int tile = imin_(CAM_TILE, n_views - c0);
        for (int c = 0; c < tile; c++) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                VisProj q;
                const bool sees = there[k] && vis_project(views[c0 + c], px[k], py[k], pz[k], q) && q.z > 0.0f;
                const unsigned long long m = __ballot(sees);
                if (lane_id() == 0) line[c][4 * k + wave] = m;
            }
        }
        __syncthreads();
        if (out_cam < tile && word0 + out_word < n_words)
            words[(size_t)(c0 + out_cam) * (size_t)n_words + (size_t)(word0 + out_word)] = line[out_cam][out_word];
        __syncthreads();
    }
}

constexpr int OVERLAP_CHUNK = 128;                // words of a row staged per step
constexpr int OVERLAP_STRIDE = OVERLAP_CHUNK + 1; // one access width of padding: a column of 16 rows hits 16 banks
constexpr unsigned OVERLAP_MAX_BLOCKS = 2048;

// blockIdx.x names the tile pair (ti <= tj, row-major over the upper triangle), blockIdx.y strides over the chunks.
__global__ void __launch_bounds__(256) view_overlap_kernel(int n_views, int n_tiles, int n_words,
                                                           const unsigned long long* __restrict__ words,
                                                           int* __restrict__ counts) {
    __shared__ unsigned long long rows[2 * CAM_TILE * OVERLAP_STRIDE];
    int ti = 0, rest = (int)blockIdx.x;
    while (rest >= n_tiles - ti) {  // workgroup-uniform
        rest -= n_tiles - ti;
        ti++;
    }
    const int tj = ti + rest;
    const int a = (int)(threadIdx.x >> 4), b = (int)(threadIdx.x & 15);
    const int i = CAM_TILE * ti + a, j = CAM_TILE * tj + b;
    const bool mine = i < n_views && j < n_views && j >= i;
    const unsigned long long* ra = rows + a * OVERLAP_STRIDE;
    const unsigned long long* rb = rows + (CAM_TILE + b) * OVERLAP_STRIDE;
    unsigned int sum = 0u;
    for (long long w0 = (long long)blockIdx.y * OVERLAP_CHUNK; w0 < n_words; w0 += (long long)gridDim.y * OVERLAP_CHUNK) {
        const int len = (int)(n_words - w0 < OVERLAP_CHUNK ? n_words - w0 : OVERLAP_CHUNK);
        for (int e = (int)threadIdx.x; e < 2 * CAM_TILE * OVERLAP_CHUNK; e += 256) {
            const int r = e / OVERLAP_CHUNK, w = e % OVERLAP_CHUNK;
            const int cam = r < CAM_TILE ? CAM_TILE * ti + r : CAM_TILE * tj + (r - CAM_TILE);
            rows[r * OVERLAP_STRIDE + w] = cam < n_views && w < len ? words[(size_t)cam * (size_t)n_words + (size_t)(w0 + w)] : 0ull;
        }
        __syncthreads();
        if (mine) {
            for (int w = 0; w < len; w++) sum += (unsigned int)__builtin_popcountll(ra[w] & rb[w]);
        }
        __syncthreads();
    }
    if (mine && sum != 0u) {
        atomicAdd(counts + (size_t)i * n_views + j, (int)sum);
        if (i != j) atomicAdd(counts + (size_t)j * n_views + i, (int)sum);
    }
}

// ---- farthest-point sampling -------------------------------------------------------------------------------------------
constexpr int FPS_ITEMS = 4;                    // points per thread and grid stride
constexpr unsigned FPS_MAX_BLOCKS = 1024;       // per cloud: at most this many atomics on a slot per round
constexpr float FPS_FAR = 1e10f;

// the point a key names; the clamp never changes a key that a round wrote and keeps every read inside the cloud
__device__ __forceinline__ uint32_t key_index(unsigned long long key, int n) {
    const uint32_t i = ~(uint32_t)key;
    return i < (uint32_t)n ? i : (uint32_t)(n - 1);
}

// Round `round` (1 .. k - 1) of every cloud: blockIdx.y is the cloud.
__global__ void __launch_bounds__(256) fps_round_kernel(int n, int k, int round, const float* __restrict__ clouds,
                                                        const int* __restrict__ first, float* __restrict__ dist,
                                                        unsigned long long* __restrict__ keys) {
    __shared__ unsigned long long part[4];
    const size_t m = blockIdx.y;
    const float* cloud = clouds + 3 * m * (size_t)n;
    float* dm = dist + m * (size_t)n;
    const uint32_t last = round == 1 ? (uint32_t)first[m] : key_index(keys[m * (size_t)k + (size_t)(round - 1)], n);
    const float qx = cloud[3 * (size_t)last], qy = cloud[3 * (size_t)last + 1], qz = cloud[3 * (size_t)last + 2];
    unsigned long long best = 0ull;  // below every key: ~i >= 2^31 for i < 2^31
    for (long long base = (long long)blockIdx.x * (256 * FPS_ITEMS); base < n; base += (long long)gridDim.x * (256 * FPS_ITEMS)) {
#pragma unroll
        for (int t = 0; t < FPS_ITEMS; t++) {
            const long long i = base + 256 * t + (long long)threadIdx.x;
            if (i < n) {
                const float dx = cloud[3 * (size_t)i] - qx, dy = cloud[3 * (size_t)i + 1] - qy, dz = cloud[3 * (size_t)i + 2] - qz;
                const float d = (dx * dx + dy * dy) + dz * dz;
                const float prev = round == 1 ? FPS_FAR : dm[i];
                const float now = fminf(prev, d);
                dm[i] = now;
                const unsigned long long key = ((unsigned long long)__float_as_uint(now) << 32) | (unsigned long long)(~(uint32_t)i);
                best = key > best ? key : best;
            }
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long other = __shfl_xor(best, s);
        best = other > best ? other : best;
    }
    if (lane_id() == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) best = part[w] > best ? part[w] : best;
        atomicMax(keys + m * (size_t)k + (size_t)round, best);
    }
}

// one thread per (cloud, sample)
__global__ void __launch_bounds__(256) fps_gather_kernel(int n_clouds, int n, int k, const float* __restrict__ clouds,
                                                         const int* __restrict__ first,
                                                         const unsigned long long* __restrict__ keys,
                                                         int* __restrict__ indices, float* __restrict__ samples) {
    const int e = (int)(blockIdx.x * 256 + threadIdx.x);
    if (e >= n_clouds * k) return;
    const int m = e / k, r = e % k;
    const uint32_t idx = r == 0 ? (uint32_t)first[m] : key_index(keys[e], n);
    indices[e] = (int)idx;
    const float* p = clouds + 3 * ((size_t)m * (size_t)n + (size_t)idx);
#pragma unroll
    for (int c = 0; c < 3; c++) samples[3 * (size_t)e + c] = p[c];
}

}  // namespace g4s

using namespace g4s;

// ---------------------------------------------------------------------------------------------------------------------
// extern "C" entry points; every argument is checked before any launch
namespace {

constexpr long long MAX_POINTS = (1ll << 31) - 64;
constexpr int MAX_VIEWS = 65535;

int check_views(int n_views) {
    return n_views >= 1 && n_views <= MAX_VIEWS ? G4S_OK : fail(G4S_ERR_INVALID_ARGUMENT, "n_views must be in 1 .. 65535");
}

int check_fps(int n_clouds, int n_points, int n_samples) {
    if (n_clouds < 1 || n_clouds > MAX_VIEWS) return fail(G4S_ERR_INVALID_ARGUMENT, "n_clouds must be in 1 .. 65535");
    if (n_points < 3 || n_points > (1 << 30)) return fail(G4S_ERR_INVALID_ARGUMENT, "n_points must be in 3 .. 2^30");
    if (n_samples < 2 || n_samples >= n_points) return fail(G4S_ERR_INVALID_ARGUMENT, "n_samples must be in 2 .. n_points - 1");
    if ((long long)n_clouds * n_samples > (1ll << 30))
        return fail(G4S_ERR_INVALID_ARGUMENT, "n_clouds * n_samples must be at most 2^30");
    return G4S_OK;
}

size_t fps_keys_bytes(int n_clouds, int n_samples) { return align_up((size_t)n_clouds * (size_t)n_samples * 8); }

}  // namespace

extern "C" size_t g4s_view_bits_workspace(int n_views) { return view_table_bytes<VisView>(n_views); }

extern "C" int g4s_view_bits(int n_points, const float* points, int n_views, const float* world_view, const float* focal,
                             const int* sizes, unsigned long long* words, char* workspace, size_t workspace_bytes,
                             void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (n_points < 0 || n_points > MAX_POINTS) return fail(G4S_ERR_INVALID_ARGUMENT, "n_points must be in 0 .. 2^31 - 64");
    if (check_views(n_views) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!world_view || !focal || !sizes || (n_points > 0 && (!points || !words))) return null_pointer();
    for (int v = 0; v < n_views; v++) {
        if (sizes[2 * v] <= 0 || sizes[2 * v + 1] <= 0)
            return fail(G4S_ERR_INVALID_ARGUMENT, "view %d: width, height must be positive", v);
    }
    if (check_workspace(workspace, workspace_bytes, g4s_view_bits_workspace(n_views)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_points == 0) return G4S_OK;
    // nothing below can fail a check: the first device call comes after every one of them
    std::vector<VisView> host((size_t)n_views);
    for (int v = 0; v < n_views; v++) {
        vis_pose(host[(size_t)v], world_view, focal, v);
        host[(size_t)v].maps = ViewMaps{sizes[2 * v], sizes[2 * v + 1], nullptr, nullptr};
    }
    VisView* table = (VisView*)align_ptr(workspace);
    const hipError_t e = upload(table, host.data(), host.size() * sizeof(VisView), stream);  // `host` dies with this frame
    if (e != hipSuccess) return fail(G4S_ERR_HIP, "view bits view table: %s", hipGetErrorString(e));
    const int n_words = (int)(((long long)n_points + 63) / 64);
    const unsigned blocks = (unsigned)(((long long)n_points + BITS_POINTS - 1) / BITS_POINTS);
    hipLaunchKernelGGL(view_bits_kernel, dim3(blocks), dim3(256), 0, stream, n_points, points, table, n_views, n_words, words);
    return finish(hipSuccess, "view bits");
}

extern "C" int g4s_view_overlap(int n_views, int n_words, const unsigned long long* words, int* counts, char* workspace,
                                size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    (void)workspace;
    (void)workspace_bytes;
    clear_error();
    if (check_views(n_views) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_words < 0 || n_words > (1 << 25)) return fail(G4S_ERR_INVALID_ARGUMENT, "n_words must be in 0 .. 2^25");
    if (!counts || (n_words > 0 && !words)) return null_pointer();
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_views * (size_t)n_views * 4, stream);
    if (e != hipSuccess) return finish(e, "view overlap");
    if (n_words == 0) return G4S_OK;
    const int n_tiles = (n_views + CAM_TILE - 1) / CAM_TILE;
    const long long pairs = (long long)n_tiles * (n_tiles + 1) / 2;
    const long long chunks = ((long long)n_words + OVERLAP_CHUNK - 1) / OVERLAP_CHUNK;
    long long per_pair = OVERLAP_MAX_BLOCKS / pairs;
    per_pair = per_pair < 1 ? 1 : (per_pair > chunks ? chunks : per_pair);
    hipLaunchKernelGGL(view_overlap_kernel, dim3((unsigned)pairs, (unsigned)per_pair), dim3(256), 0, stream, n_views, n_tiles,
                       n_words, words, counts);
    return finish(hipSuccess, "view overlap");
}

extern "C" size_t g4s_fps_workspace(int n_clouds, int n_samples) {
    if (n_clouds < 1 || n_samples < 2 || (long long)n_clouds * n_samples > (1ll << 30)) return 0;
    return fps_keys_bytes(n_clouds, n_samples) + align_up((size_t)n_clouds * 4) + 256;
}

extern "C" int g4s_fps(int n_clouds, int n_points, const float* clouds, const int* first, int n_samples, int* indices,
                       float* samples, float* dist, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_fps(n_clouds, n_points, n_samples) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!clouds || !first || !indices || !samples || !dist) return null_pointer();
    for (int m = 0; m < n_clouds; m++) {
        if (first[m] < 0 || first[m] >= n_points)
            return fail(G4S_ERR_INVALID_ARGUMENT, "first[%d] must be a point index below n_points", m);
    }
    if (check_workspace(workspace, workspace_bytes, g4s_fps_workspace(n_clouds, n_samples)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    // nothing below can fail a check
    unsigned long long* keys = (unsigned long long*)align_ptr(workspace);
    int* dev_first = (int*)((char*)keys + fps_keys_bytes(n_clouds, n_samples));
    hipError_t e = hipMemsetAsync(keys, 0, (size_t)n_clouds * (size_t)n_samples * 8, stream);
    if (e == hipSuccess) e = upload(dev_first, first, (size_t)n_clouds * 4, stream);
    if (e != hipSuccess) return finish(e, "farthest-point sampling");
    const unsigned per_block = 256u * FPS_ITEMS;
    unsigned blocks = ((unsigned)n_points + per_block - 1u) / per_block;
    blocks = blocks < FPS_MAX_BLOCKS ? blocks : FPS_MAX_BLOCKS;
    for (int round = 1; round < n_samples; round++)
        hipLaunchKernelGGL(fps_round_kernel, dim3(blocks, (unsigned)n_clouds), dim3(256), 0, stream, n_points, n_samples, round,
                           clouds, dev_first, dist, keys);
    const unsigned total = (unsigned)(n_clouds * n_samples);
    hipLaunchKernelGGL(fps_gather_kernel, dim3(blocks256(total)), dim3(256), 0, stream, n_clouds, n_points, n_samples, clouds,
                       dev_first, keys, indices, samples);
    return finish(hipSuccess, "farthest-point sampling");
}
