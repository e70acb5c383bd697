// The generic exclusive scan of scan.hip, shared by tsdf.hip, unbounded.hip, mesh_ops.hip, chart_init.hip, warp_init.hip and plane_masks.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace g4s {

// Exclusive scan of n u32 values in a fixed order (three launches): out must not alias in, *d_total = their sum,
// `chunks` = scan_chunks(n) words of device scratch.
int scan_chunks(long n);
void scan_u32(const uint32_t* in, uint32_t* out, int n, uint32_t* chunks, uint32_t* d_total, hipStream_t s);

}  // namespace g4s
