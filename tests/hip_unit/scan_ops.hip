// Standalone check of scan_u32 (g4splat_amd/csrc/tsdf/scan.hip) against a host loop, bit for bit, at the sizes where its
// three kernels change behaviour: nothing to scan, one value, a partial and a full chunk of 1024, one value into the next
// chunk, 256 chunks (one full trip of scan_chunk_offs_kernel's loop) and 257 (its second trip).  Built and run by
// tests/test_gpu_scan_ops.py:
//   hipcc <CXXFLAGS of g4splat_amd/csrc/Makefile> tests/hip_unit/scan_ops.hip g4splat_amd/csrc/tsdf/scan.hip -o scan_ops
//   ./scan_ops seeded | ones      (the input: seeded values in 0..7, or all ones)
// `out`, `chunks` and the total start out as poison and are followed by a poisoned guard.  A HIP error ends the program
// at once; a mismatch prints size, first bad index, got and want, and the next size runs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../g4splat_amd/csrc/tsdf/scan.h"
using namespace g4s;

#define HIP_OK(expr)                                                                                        \
    do {                                                                                                    \
        const hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) {                                                                             \
            printf("HIP error %d (%s) at line %d: %s\n", (int)e_, hipGetErrorString(e_), __LINE__, #expr); \
            printf("scan_ops ABORTED\n");                                                                   \
            fflush(stdout);                                                                                 \
            exit(2);                                                                                        \
        }                                                                                                   \
    } while (0)

constexpr size_t GUARD = 1024;  // words
constexpr uint32_t POISON = 0xA5A5A5A5u;

static int g_failed = 0;

static void mismatch(const char* what, int n, size_t i, uint32_t got, uint32_t want) {
    printf("MISMATCH n = %d: %s first bad index %zu got 0x%x want 0x%x\n", n, what, i, got, want);
    g_failed++;
}

// `words` device words followed by the guard, all poison
static uint32_t* poisoned(size_t words) {
    uint32_t* p = nullptr;
    HIP_OK(hipMalloc((void**)&p, (words + GUARD) * 4));
    HIP_OK(hipMemset(p, 0xA5, (words + GUARD) * 4));
    return p;
}

// the first `words` words against want (nullptr: not compared), and the guard behind them
static void check(const char* what, int n, const uint32_t* dev, size_t words, const uint32_t* want) {
    std::vector<uint32_t> got(words + GUARD);
    HIP_OK(hipMemcpy(got.data(), dev, got.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; want != nullptr && i < words; i++)
        if (got[i] != want[i]) return mismatch(what, n, i, got[i], want[i]);
    for (size_t i = words; i < got.size(); i++)
        if (got[i] != POISON) return mismatch("guard", n, i, got[i], POISON);
}

static void run(int n, bool ones) {
    std::vector<uint32_t> in((size_t)n), want((size_t)n);
    uint32_t x = 0x9E3779B9u ^ (uint32_t)n, sum = 0;
    for (int i = 0; i < n; i++) {
        x = x * 1664525u + 1013904223u;
        in[i] = ones ? 1u : (x >> 13) & 7u;
        want[i] = sum;
        sum += in[i];
    }
    const size_t nc = (size_t)scan_chunks(n);
    if (nc != ((size_t)n + 1023) / 1024) mismatch("scan_chunks", n, 0, (uint32_t)nc, (uint32_t)(((size_t)n + 1023) / 1024));
    uint32_t* d_in = poisoned((size_t)n);
    uint32_t* d_out = poisoned((size_t)n);
    uint32_t* d_chunks = poisoned(nc);
    uint32_t* d_total = poisoned(1);
    if (n > 0) HIP_OK(hipMemcpy(d_in, in.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    scan_u32(d_in, d_out, n, d_chunks, d_total, nullptr);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    check("in (must be left alone)", n, d_in, (size_t)n, in.data());
    check("out", n, d_out, (size_t)n, want.data());
    check("chunks", n, d_chunks, nc, nullptr);
    check("total", n, d_total, 1, &sum);
    HIP_OK(hipFree(d_in));
    HIP_OK(hipFree(d_out));
    HIP_OK(hipFree(d_chunks));
    HIP_OK(hipFree(d_total));
    printf("n = %d: %zu chunks, total %u\n", n, nc, sum);
}

int main(int argc, char** argv) {
    const bool ones = argc > 1 && strcmp(argv[1], "ones") == 0;
    if (argc != 2 || (!ones && strcmp(argv[1], "seeded") != 0)) {
        printf("usage: scan_ops seeded | ones\n");
        return 3;
    }
    for (int n : {0, 1, 255, 1023, 1024, 1025, 262144, 262145}) run(n, ones);
    if (g_failed) {
        printf("scan_ops FAILED %s: %d mismatches\n", argv[1], g_failed);
        return 1;
    }
    printf("scan_ops OK %s\n", argv[1]);
    return 0;
}
