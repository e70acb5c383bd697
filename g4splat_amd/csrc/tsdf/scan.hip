// Exclusive scan of n u32 values in a fixed order (scan.h): three launches -- chunk sums, one workgroup scanning them,
// apply.  The TSDF fusion, both marching-cubes extractions and the mesh compaction take their output positions from it.
#include "scan.h"

#include "../g4s_device.h"

namespace g4s {

constexpr int SCAN_CHUNK = 1024;  // values per 256-thread workgroup (4 per thread, contiguous)

__global__ void __launch_bounds__(256) scan_chunk_sums_kernel(const uint32_t* __restrict__ in, int n,
                                                              uint32_t* __restrict__ chunk_sums) {
    __shared__ uint32_t sm4[4];
    const long base = (long)blockIdx.x * SCAN_CHUNK + 4 * (long)threadIdx.x;
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) s += base + j < n ? in[base + j] : 0u;
    uint32_t total;
    (void)block256_excl_scan_u32(s, sm4, &total);
    if (threadIdx.x == 0) chunk_sums[blockIdx.x] = total;
}

// single workgroup: chunk_offs = exclusive scan of chunk_sums, in place, *total = their sum
__global__ void __launch_bounds__(256) scan_chunk_offs_kernel(uint32_t* __restrict__ chunks, int nchunks,
                                                              uint32_t* __restrict__ total) {
    __shared__ uint32_t sm4[4];
    uint32_t run = 0;
    for (int b = 0; b < nchunks; b += 256) {
        const int i = b + (int)threadIdx.x;
        const uint32_t v = i < nchunks ? chunks[i] : 0u;
        uint32_t t;
        const uint32_t ex = block256_excl_scan_u32(v, sm4, &t);
        if (i < nchunks) chunks[i] = run + ex;
        run += t;
    }
    if (threadIdx.x == 0) *total = run;
}

__global__ void __launch_bounds__(256) scan_apply_kernel(const uint32_t* __restrict__ in, int n,
                                                         const uint32_t* __restrict__ chunk_offs,
                                                         uint32_t* __restrict__ out) {
    __shared__ uint32_t sm4[4];
    const long base = (long)blockIdx.x * SCAN_CHUNK + 4 * (long)threadIdx.x;
    uint32_t v[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        v[j] = base + j < n ? in[base + j] : 0u;
        s += v[j];
    }
    uint32_t total;
    uint32_t run = chunk_offs[blockIdx.x] + block256_excl_scan_u32(s, sm4, &total);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (base + j < n) out[base + j] = run;
        run += v[j];
    }
}

int scan_chunks(long n) { return (int)((n + SCAN_CHUNK - 1) / SCAN_CHUNK); }

void scan_u32(const uint32_t* in, uint32_t* out, int n, uint32_t* chunks, uint32_t* d_total, hipStream_t s) {
    const int nc = scan_chunks(n);
    if (nc == 0) {
        (void)hipMemsetAsync(d_total, 0, 4, s);
        return;
    }
    hipLaunchKernelGGL(scan_chunk_sums_kernel, dim3(nc), dim3(256), 0, s, in, n, chunks);
    hipLaunchKernelGGL(scan_chunk_offs_kernel, dim3(1), dim3(256), 0, s, chunks, nc, d_total);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nc), dim3(256), 0, s, in, n, chunks, out);
}

}  // namespace g4s
