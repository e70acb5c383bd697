// Packed rows for the visible-rows gradient exchange (g4splat_amd/parallel.py), kernels and entry points: g4s_pack_rows,
// g4s_accumulate_rows and g4s_accumulate_rows_ordered of include/g4s_rasterizer.h.
// mode bit 0: direction (0 = pack: rows -> buffer, 1 = unpack: buffer -> rows)
// mode bit 1: buffer layout (0 = segment after segment, packed[seg_off(s) * n + j * w_s + c]; 1 = row-major [n, sum w],
//             packed[j * sum_w + seg_off(s) + c] -- what an all_to_all with per-destination row ranges needs)
// mode bit 2: unpack ADDS to the rows instead of overwriting them (the owner's accumulation of one source's rows; a
//             source holds a row at most once, so there are no duplicate indices inside one launch)
// mode bit 3: (row-major only) buffer rows are sum w + 1 floats: the last one is the row's index as int32 bits --
//             pack writes it, unpack reads it instead of idx[] (idx may be NULL then)
// A row's floats over all segments (58 + 2 for the gradient bucket) are spread over the lanes of a wave --
// lane -> (segment, column) is fixed for the whole kernel, so there is no per-element division -- and each wave
// walks rows j, j + #waves, ...: both sides move contiguous w_s-float runs.  Rows wider than 64 floats take
// several lane passes.
#include "g4s_internal.h"
#include "g4s_device.h"

namespace g4s {
struct RowSegs {
    float* ptr[8];
    int width[8];
    int nseg;
};
__global__ void __launch_bounds__(256) pack_rows_kernel(RowSegs segs, const long long* __restrict__ idx, int n,
                                                        float* __restrict__ packed, int mode) {
    const int lane = (int)(threadIdx.x & 63);
    const int wave = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)), nwaves = (int)(gridDim.x * 4);
    const bool unpack = (mode & 1) != 0, row_major = (mode & 2) != 0, add = (mode & 4) != 0, carry = (mode & 8) != 0;
    int row_floats = 0;
    for (int s = 0; s < segs.nseg; s++) row_floats += segs.width[s];
    // carry (row-major only): every buffer row ends with its row index as an int32 column -- written by pack, and
    // read by unpack INSTEAD of idx[] (the rows and their indices then travel in one all_to_all)
    const int buf_floats = row_floats + (carry ? 1 : 0);
    for (int f0 = 0; f0 < buf_floats; f0 += 64) {
        // this lane's (segment, column) for float f0 + lane of a row
        const int f = f0 + lane;
        int seg = -1, col = 0, w = 1;
        size_t seg_off = 0;  // floats of a row before this segment
        {
            int base = 0;
            size_t off = 0;
            for (int s = 0; s < segs.nseg; s++) {
                if (f >= base && f < base + segs.width[s]) { seg = s; col = f - base; w = segs.width[s]; seg_off = off; }
                base += segs.width[s];
                off += (size_t)segs.width[s];
            }
        }
        const bool index_lane = carry && f == row_floats;
        if (seg < 0 && !index_lane) continue;
        if (index_lane) {
            if (!unpack)
                for (int j = wave; j < n; j += nwaves) packed[(size_t)j * buf_floats + row_floats] = __int_as_float((int)idx[j]);
            continue;
        }
        float* sp = segs.ptr[seg];
        float* pp = row_major ? packed + f : packed + seg_off * (size_t)n + col;
        const size_t pstride = row_major ? (size_t)buf_floats : (size_t)w;
        for (int j = wave; j < n; j += nwaves) {
            const long long row = (carry && unpack) ? (long long)__float_as_int(packed[(size_t)j * buf_floats + row_floats]) : idx[j];
            float* src = sp + (size_t)row * w + col;
            float* dst = pp + (size_t)j * pstride;
            if (!unpack) *dst = *src;
            else if (add) *src += *dst;
            else *src = *dst;
        }
    }
}

// The owner's accumulation of ALL sources in one launch (g4s_accumulate_rows, include/g4s_rasterizer.h).  The per-source
// form -- one pack_rows_kernel(mode 15) launch per source -- reads and writes a destination row once per source that
// holds it and pays a launch per source; here a workgroup owns ACC_CHUNK consecutive destination rows: it loads them into
// LDS, finds each source's rows of the chunk (the sources' rows ascend by index: a 32-ary search by 32 lanes per source,
// all sources at once), adds them source after source -- the same order of additions per element as the per-source
// launches, so the same bits -- and writes the chunk back: 7 x (launch + read + write) become 1 x.
constexpr int ACC_CHUNK = 64;  // (measured at the metric size, eight ranks: 32 rows 0.088 ms, 48 0.075, 64 0.076, 128 0.096)
struct AccSources {
    int off[8], cnt[8];  // rows [off, off + cnt) of the buffer came from source i (ascending row indices)
    int nsrc;
    // the owner's own contribution (already in the segments' rows) takes position `own_pos` in the order of additions:
    // 0 = first (own + s0 + s1 + ...), k = behind the first k sources (((0 + s0 + ... + s_{k-1}) + own) + s_k + ...): with the
    // sources in rank order and own_pos = the owner's rank, every row is summed in RANK ORDER whoever owns it
    // (g4s_accumulate_rows_ordered)
    int own_pos;
};
__global__ void __launch_bounds__(256) accumulate_rows_kernel(RowSegs segs, AccSources src, const float* __restrict__ packed,
                                                              int row_lo, int row_hi) {
    extern __shared__ float s_tile[];  // [ACC_CHUNK][row_floats]
    __shared__ int s_b0[8], s_b1[8];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    int row_floats = 0;
    for (int s = 0; s < segs.nseg; s++) row_floats += segs.width[s];
    const int buf_floats = row_floats + 1;
    const int chunk_lo = row_lo + (int)blockIdx.x * ACC_CHUNK;
    const int chunk_hi = min(chunk_lo + ACC_CHUNK, row_hi);
    const int rows = chunk_hi - chunk_lo;
    // The chunk's rows into LDS.  This lane's (segment, column) for float f0 + lane of a row is fixed (as in
    // pack_rows_kernel); a wave takes rows wave, wave + 4, ...: every load of the loop is in flight at once.  (Other
    // resident workgroups -- up to ten per CU -- cover the latency of this copy and of the search below.)
    for (int f0 = 0; f0 < row_floats; f0 += 64) {
        const int f = f0 + lane;
        int seg = -1, col = 0, w = 1;
        {
            int base = 0;
            for (int s = 0; s < segs.nseg; s++) {
                if (f >= base && f < base + segs.width[s]) { seg = s; col = f - base; w = segs.width[s]; }
                base += segs.width[s];
            }
        }
        if (seg >= 0) {
            const float* sp = segs.ptr[seg] + (size_t)chunk_lo * w + col;
            if (src.own_pos == 0) {
#pragma unroll 4
                for (int r = wave; r < rows; r += 4) s_tile[r * row_floats + f] = sp[(size_t)r * w];
            } else {  // the owner's rows join the sum behind the first own_pos sources (below): start from zero
#pragma unroll 4
                for (int r = wave; r < rows; r += 4) s_tile[r * row_floats + f] = 0.0f;
            }
        }
    }
    // each source's rows of this chunk: group g = 32 lanes searches source g for both ends at once
    {
        const int g = t >> 5, l32 = t & 31;
        const bool live = g < src.nsrc;
        const int off = live ? src.off[g] : 0, cnt = live ? src.cnt[g] : 0;
        int lo[2] = {0, 0}, hi[2] = {cnt, cnt};
        const int target[2] = {chunk_lo, chunk_hi};
        for (int it = 0; it < 7; it++) {  // 32^7 > 2^31 rows (uniform trip count: the ballots need every lane)
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const int span = hi[e] - lo[e];
                const int step = (span + 31) >> 5;
                const int pos = lo[e] + l32 * step;
                const bool valid = span > 0 && pos < hi[e];
                int v = 0x7fffffff;
                if (valid) v = __float_as_int(packed[(size_t)(off + pos) * buf_floats + row_floats]);
                const uint64_t b = __ballot(valid && v < target[e]);
                const uint64_t bv = __ballot(valid);
                const int c = __popc((uint32_t)(b >> (32 * (lane >> 5))));    // probes below the target: a prefix
                const int nv = __popc((uint32_t)(bv >> (32 * (lane >> 5))));  // valid probes
                if (span > 0) {
                    const int nlo = c == 0 ? lo[e] : lo[e] + (c - 1) * step + 1;
                    const int nhi = c == 0 ? lo[e] : (c < nv ? lo[e] + c * step : hi[e]);
                    lo[e] = nlo; hi[e] = nhi;
                }
            }
            if (__syncthreads_or((hi[0] - lo[0]) | (hi[1] - lo[1])) == 0) break;  // every group has both ends
        }
        if (live && l32 == 0) { s_b0[g] = lo[0]; s_b1[g] = lo[1]; }
    }
    __syncthreads();
    // Sources in order; a wave takes rows b0 + wave, + 4, ... of the source's sub-range, four of them in flight (a source
    // holds a row once: the waves never meet on a tile row).
    for (int s = 0; s <= src.nsrc; s++) {
        if (s == src.own_pos && s != 0) {  // (uniform) the owner's own rows, in their place in the order
            for (int f0 = 0; f0 < row_floats; f0 += 64) {
                const int f = f0 + lane;
                int seg = -1, col = 0, w = 1;
                {
                    int base = 0;
                    for (int g = 0; g < segs.nseg; g++) {
                        if (f >= base && f < base + segs.width[g]) { seg = g; col = f - base; w = segs.width[g]; }
                        base += segs.width[g];
                    }
                }
                if (seg >= 0) {
                    const float* sp = segs.ptr[seg] + (size_t)chunk_lo * w + col;
#pragma unroll 4
                    for (int r = wave; r < rows; r += 4) s_tile[r * row_floats + f] += sp[(size_t)r * w];
                }
            }
            __syncthreads();
        }
        if (s == src.nsrc) break;
        const int b0 = s_b0[s], b1 = s_b1[s];
        const float* base = packed + (size_t)src.off[s] * buf_floats;
        for (int j0 = b0 + wave; j0 < b1; j0 += 16) {
            int r[4];
            float v[4][4];  // up to 4 x 64 floats per row (launch check: rows of at most 240 floats)
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = j0 + 4 * u;
                const bool ok = j < b1;
                const float* rowp = base + (size_t)(ok ? j : b0) * buf_floats;
                r[u] = ok ? __float_as_int(rowp[row_floats]) - chunk_lo : -1;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int f = lane + 64 * q;
                    v[u][q] = f < row_floats ? rowp[f] : 0.0f;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                // (unsigned: a received row whose index column lies outside this chunk -- a source that is not sorted, or
                // that holds a row of another shard -- is dropped instead of being added outside the LDS tile)
                if ((unsigned)r[u] < (unsigned)rows) {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int f = lane + 64 * q;
                        if (f < row_floats) s_tile[r[u] * row_floats + f] += v[u][q];
                    }
                }
            }
        }
        __syncthreads();  // (the next source may hold the same rows)
    }
    for (int f0 = 0; f0 < row_floats; f0 += 64) {
        const int f = f0 + lane;
        int seg = -1, col = 0, w = 1;
        {
            int base = 0;
            for (int s = 0; s < segs.nseg; s++) {
                if (f >= base && f < base + segs.width[s]) { seg = s; col = f - base; w = segs.width[s]; }
                base += segs.width[s];
            }
        }
        if (seg >= 0) {
            float* sp = segs.ptr[seg] + (size_t)chunk_lo * w + col;
#pragma unroll 4
            for (int r = wave; r < rows; r += 4) sp[(size_t)r * w] = s_tile[r * row_floats + f];
        }
    }
}
}  // namespace g4s

using namespace g4s;

extern "C" int g4s_pack_rows(int nseg, float* const* segments, const int* widths, const long long* row_index, int n,
                             float* packed, int unpack, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (nseg < 1 || nseg > 8 || n < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "1..8 segments, n >= 0");
    if (unpack < 0 || unpack > 15 || ((unpack & 4) && !(unpack & 1)) || ((unpack & 8) && !(unpack & 2)))
        return fail(G4S_ERR_INVALID_ARGUMENT, "mode: bit 0 unpack, bit 1 row-major buffer, bit 2 add (unpack only), "
                                              "bit 3 index column (row-major only)");
    const bool idx_from_buffer = (unpack & 9) == 9;
    if (!segments || !widths || (n > 0 && ((!row_index && !idx_from_buffer) || !packed)))
        return fail(G4S_ERR_INVALID_ARGUMENT, "NULL pointer");
    for (int i = 0; i < nseg; i++)
        if (!segments[i] || widths[i] <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "segment %d: NULL pointer or width <= 0", i);
    if (n > 0) {
        RowSegs segs{};
        segs.nseg = nseg;
        for (int i = 0; i < nseg; i++) { segs.ptr[i] = segments[i]; segs.width[i] = widths[i]; }
        const int blocks = (n + 31) / 32 < 8192 ? (n + 31) / 32 : 8192;  // >= 8 rows per wave once n is large
        hipLaunchKernelGGL(pack_rows_kernel, dim3(blocks), dim3(256), 0, s, segs, row_index, n, packed, unpack);
    }
    return stage_done("pack_rows", s);
}

static int accumulate_rows_impl(int nseg, float* const* segments, const int* widths, int nsrc, const int* src_offsets,
                                const int* src_counts, const float* packed, int row_lo, int row_hi, int own_position, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (nseg < 1 || nseg > 8 || nsrc < 0 || row_lo < 0 || row_hi < row_lo)
        return fail(G4S_ERR_INVALID_ARGUMENT, "1..8 segments, nsrc >= 0, 0 <= row_lo <= row_hi");
    if (!segments || !widths || (nsrc > 0 && (!src_offsets || !src_counts || !packed)))
        return fail(G4S_ERR_INVALID_ARGUMENT, "NULL pointer");
    for (int i = 0; i < nseg; i++)
        if (!segments[i] || widths[i] <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "segment %d: NULL pointer or width <= 0", i);
    for (int i = 0; i < nsrc; i++)
        if (src_offsets[i] < 0 || src_counts[i] < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "source %d: negative offset / count", i);
    if (nsrc == 0 || row_hi == row_lo) return G4S_OK;
    RowSegs segs{};
    segs.nseg = nseg;
    int row_floats = 0;
    for (int i = 0; i < nseg; i++) { segs.ptr[i] = segments[i]; segs.width[i] = widths[i]; row_floats += widths[i]; }
    const size_t lds = (size_t)ACC_CHUNK * row_floats * sizeof(float);
    if (lds > 60 * 1024) return fail(G4S_ERR_UNSUPPORTED, "rows wider than 240 floats");
    // (the ordered form needs all sources in one launch; g4s_accumulate_rows_ordered has said so before it comes here)
    if (own_position != 0 && nsrc > 8) return fail(G4S_ERR_UNSUPPORTED, "the ordered accumulation takes at most 8 sources");
    const int blocks = (row_hi - row_lo + ACC_CHUNK - 1) / ACC_CHUNK;
    for (int s0 = 0; s0 < nsrc; s0 += 8) {  // (more than eight sources: eight per launch, in order)
        AccSources src{};
        src.nsrc = nsrc - s0 < 8 ? nsrc - s0 : 8;
        src.own_pos = own_position;
        for (int i = 0; i < src.nsrc; i++) { src.off[i] = src_offsets[s0 + i]; src.cnt[i] = src_counts[s0 + i]; }
        hipLaunchKernelGGL(accumulate_rows_kernel, dim3(blocks), dim3(256), lds, s, segs, src, packed, row_lo, row_hi);
    }
    return stage_done("accumulate_rows", s);
}

extern "C" int g4s_accumulate_rows(int nseg, float* const* segments, const int* widths, int nsrc, const int* src_offsets,
                                   const int* src_counts, const float* packed, int row_lo, int row_hi, void* stream_) {
    return accumulate_rows_impl(nseg, segments, widths, nsrc, src_offsets, src_counts, packed, row_lo, row_hi, 0, stream_);
}

extern "C" int g4s_accumulate_rows_ordered(int nseg, float* const* segments, const int* widths, int nsrc, const int* src_offsets,
                                           const int* src_counts, const float* packed, int row_lo, int row_hi, int own_position,
                                           void* stream_) {
    clear_error();
    if (own_position < 0 || own_position > nsrc) return fail(G4S_ERR_INVALID_ARGUMENT, "0 <= own_position <= nsrc");
    if (own_position != 0 && nsrc > 8) return fail(G4S_ERR_UNSUPPORTED, "the ordered accumulation takes at most 8 sources");
    return accumulate_rows_impl(nseg, segments, widths, nsrc, src_offsets, src_counts, packed, row_lo, row_hi, own_position, stream_);
}
