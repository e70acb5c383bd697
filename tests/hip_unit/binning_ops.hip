// Standalone check of every launcher of g4splat_amd/csrc/binning.hip against plain host restatements, bit for bit:
// the three radix sorts, the two block-sum scans, the index-order compaction, the instance expansion, the tile ranges
// and the tile processing order, at the sizes where their code paths switch.  Built and run by
// tests/test_gpu_binning_ops.py:
//   hipcc <CXXFLAGS of g4splat_amd/csrc/Makefile> tests/hip_unit/binning_ops.hip g4splat_amd/csrc/binning.hip -o binning_ops
//   ./binning_ops [group]      (group: a substring of a group name below; none = all)
// Every device buffer has the size the product gives it (geom_layout / bin_layout, the hist expressions of knn.hip and
// tsdf.hip) and is followed by a poisoned guard that is checked after each case.  A HIP error ends the program at once;
// a mismatch prints case, size, first bad index, got and want, and the next case runs.
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#include "../../g4splat_amd/csrc/g4s_internal.h"
using namespace g4s;

// ---- plumbing --------------------------------------------------------------------------------------------------------
#define HIP_OK(expr)                                                                                         \
    do {                                                                                                     \
        const hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                              \
            printf("HIP error %d (%s) at line %d: %s\n", (int)e_, hipGetErrorString(e_), __LINE__, #expr);  \
            printf("binning_ops ABORTED in case %s\n", g_case.c_str());                                      \
            fflush(stdout);                                                                                  \
            exit(2);                                                                                         \
        }                                                                                                    \
    } while (0)

static hipStream_t g_s;
static std::string g_case = "(start)";
static bool g_case_bad = false;
static int g_failed = 0;
static std::map<std::string, int> g_count;  // cases run per kernel

constexpr int TK32 = 256 * SORT_ITEMS_U32;
constexpr int TK64 = 256 * SORT_ITEMS_U64;
constexpr uint32_t LOW_MASK = (1u << DEPTH_SORT_LOW_BITS) - 1u;
constexpr size_t GUARD = 4096;
constexpr uint8_t POISON8 = 0xA5;
constexpr uint32_t POISON32 = 0xA5A5A5A5u;
constexpr uint64_t POISON64 = 0xA5A5A5A5A5A5A5A5ull;

static void mismatch(const char* what, size_t n, size_t i, unsigned long long got, unsigned long long want) {
    if (!g_case_bad) printf("MISMATCH case %s: %s (size %zu) first bad index %zu got 0x%llx want 0x%llx\n", g_case.c_str(), what, n, i, got, want);
    g_case_bad = true;
}

struct DBuf;
static std::vector<DBuf*> g_live;
// `bytes` device bytes followed by a guard; everything starts out as poison
struct DBuf {
    char* base = nullptr;
    size_t bytes;
    const char* name;
    DBuf(size_t bytes_, const char* name_) : bytes(bytes_), name(name_) {
        HIP_OK(hipMalloc((void**)&base, bytes + GUARD + 16));
        HIP_OK(hipMemsetAsync(base, POISON8, bytes + GUARD + 16, g_s));
        g_live.push_back(this);
    }
    ~DBuf() {
        g_live.erase(std::find(g_live.begin(), g_live.end(), this));
        HIP_OK(hipFree(base));
    }
    DBuf(const DBuf&) = delete;
    template <typename T> T* p() { return reinterpret_cast<T*>(base); }
    template <typename T> void up(const std::vector<T>& v, size_t at = 0) {
        if ((at + v.size()) * sizeof(T) > bytes) { printf("harness bug: upload past %s\n", name); exit(3); }
        if (!v.empty()) HIP_OK(hipMemcpyAsync(base + at * sizeof(T), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, g_s));
        HIP_OK(hipStreamSynchronize(g_s));  // (the vector may be a temporary)
    }
    template <typename T> std::vector<T> down(size_t count) {
        if (count * sizeof(T) > bytes) { printf("harness bug: download past %s\n", name); exit(3); }
        std::vector<T> v(count);
        HIP_OK(hipStreamSynchronize(g_s));
        if (count) HIP_OK(hipMemcpy(v.data(), base, count * sizeof(T), hipMemcpyDeviceToHost));
        return v;
    }
    void zero() { if (bytes) HIP_OK(hipMemsetAsync(base, 0, bytes, g_s)); }
    void check_guard() {
        std::vector<uint8_t> g(GUARD);
        HIP_OK(hipMemcpy(g.data(), base + bytes, GUARD, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < GUARD; i++)
            if (g[i] != POISON8) { mismatch((std::string("guard behind ") + name).c_str(), bytes, i, g[i], POISON8); return; }
    }
};

static void begin_case(const char* kernel, const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_case = std::string(kernel) + " " + buf;
    g_case_bad = false;
    g_count[kernel]++;
}
static void sync_dev() {
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(g_s));
}
// to be called while the case's buffers are alive
static void end_case() {
    sync_dev();
    for (DBuf* b : g_live) b->check_guard();
    if (g_case_bad) g_failed++;
}

template <typename T>
static void expect_eq(const char* what, const std::vector<T>& got, const std::vector<T>& want) {
    if (got.size() != want.size()) { printf("harness bug: %s sizes differ\n", what); exit(3); }
    for (size_t i = 0; i < got.size(); i++)
        if (got[i] != want[i]) { mismatch(what, got.size(), i, (unsigned long long)got[i], (unsigned long long)want[i]); return; }
}
template <typename T>
static void expect_poison(const char* what, const std::vector<T>& got, size_t from) {
    T want;
    memset(&want, POISON8, sizeof(T));
    for (size_t i = from; i < got.size(); i++)
        if (got[i] != want) { mismatch(what, got.size(), i, (unsigned long long)got[i], (unsigned long long)want); return; }
}
static void expect_word(const char* what, unsigned long long got, unsigned long long want) {
    if (got != want) mismatch(what, 1, 0, got, want);
}

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
    uint64_t next() {  // splitmix64
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint32_t u32() { return (uint32_t)(next() >> 32); }
    uint32_t below(uint32_t n) { return (uint32_t)(((next() >> 32) * (uint64_t)n) >> 32); }
};

// scratch capacities, as the product's layouts give them (the distance to the next sub-buffer)
static size_t geom_hist_bytes(size_t n) { const GeomLayout L = geom_layout(n); return L.bin_total - L.hist; }
static size_t geom_bins_bytes(size_t n) { const GeomLayout L = geom_layout(n); return L.key_min_blocks - L.bin_total; }
static size_t geom_blockwords_bytes(size_t n) { const GeomLayout L = geom_layout(n); return L.block_offs - L.block_sums; }
static size_t geom_total_bytes(size_t n) { const GeomLayout L = geom_layout(n); return L.bytes - 256 - L.total; }
static size_t bin_hist_bytes(size_t R) { const BinLayout L = bin_layout(R); return L.bin_total - L.hist; }
static size_t bin_bins_bytes(size_t R) { const BinLayout L = bin_layout(R); return L.qhit - L.bin_total; }
// knn.hip (knn_layout) and tsdf/tsdf.hip (tsdf layout) keep theirs private: the same expressions
static size_t knn_hist_bytes(size_t n) { return (size_t)256 * (sort_blocks(n, SORT_ITEMS_U32) + 1) * 4; }
static size_t knn_bins_bytes() { return 256 * 4; }
static size_t tsdf_hist_bytes(size_t n) { return (size_t)256 * sort_blocks(n, SORT_ITEMS_U64) * 4; }
static size_t tsdf_bins_bytes() { return 512 * 4; }

// ---- key sets --------------------------------------------------------------------------------------------------------
enum KeySet { K_EQUAL, K_TWO, K_RANDOM, K_ONE_DIGIT, K_DESCENDING, K_DEPTHS, K_SETS };
static const char* const KEYSET_NAME[K_SETS] = {"all-equal", "two-values", "random32", "one-digit", "descending", "depth-ties"};
static std::vector<uint32_t> make_keys(int set, size_t n, uint64_t seed) {
    Rng r(seed * 16 + set);
    std::vector<uint32_t> k(n);
    for (size_t i = 0; i < n; i++) {
        switch (set) {
        case K_EQUAL: k[i] = 0x3F800000u; break;
        case K_TWO: k[i] = (r.u32() & 1u) ? 0x80000005u : 5u; break;
        case K_RANDOM: k[i] = r.u32(); break;
        case K_ONE_DIGIT: k[i] = 0x41230017u | ((r.u32() & 0xFFu) << 8); break;
        case K_DESCENDING: k[i] = 0x40000000u + (uint32_t)(n - i); break;
        default: {  // float bits of positive depths, a thousand distinct values
            const float d = 0.2f + 0.37f * (float)r.below(1000);
            memcpy(&k[i], &d, 4);
        }
        }
    }
    if (set == K_RANDOM && n >= 1) k[n / 3] = 0u;
    if (set == K_RANDOM && n >= 2) k[(2 * n) / 3] = 0xFFFFFFFFu;
    return k;
}

static std::vector<int> sort_sizes(int TK) {
    return {1, 2, 63, 64, 65, 255, 256, 257, TK - 1, TK, TK + 1, 2 * TK + 1, 256 * TK - 1, 256 * TK, 256 * TK + 1, 2500003};
}

// ---- 32-bit sorts ------------------------------------------------------------------------------------------------------
// order[] = stable sort of 0..n-1 by f(key)
template <typename F>
static std::vector<uint32_t> stable_order(const std::vector<uint32_t>& keys, F f) {
    std::vector<uint32_t> o(keys.size());
    std::iota(o.begin(), o.end(), 0u);
    std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return f(keys[a]) < f(keys[b]); });
    return o;
}
static void check_pairs(const char* stage, DBuf* kbuf[2], DBuf* vbuf[2], int cur, size_t n_max, const std::vector<uint32_t>& keys,
                        const std::vector<uint32_t>& order, bool other_is_poison_beyond) {
    if (cur != 0 && cur != 1) { mismatch("ping-pong index", 1, 0, (unsigned long long)cur, 0); return; }
    const size_t n = keys.size();
    std::vector<uint32_t> gk = kbuf[cur]->down<uint32_t>(n_max), gv = vbuf[cur]->down<uint32_t>(n_max);
    std::vector<uint32_t> wk(n), wv(n);
    for (size_t i = 0; i < n; i++) { wk[i] = keys[order[i]]; wv[i] = order[i]; }
    std::string a = std::string(stage) + " keys", b = std::string(stage) + " payload";
    expect_eq(a.c_str(), std::vector<uint32_t>(gk.begin(), gk.begin() + n), wk);
    expect_eq(b.c_str(), std::vector<uint32_t>(gv.begin(), gv.begin() + n), wv);
    expect_poison((a + " beyond the count").c_str(), gk, n);
    expect_poison((b + " beyond the count").c_str(), gv, n);
    if (other_is_poison_beyond) {
        expect_poison((a + " (other buffer) beyond the count").c_str(), kbuf[cur ^ 1]->down<uint32_t>(n_max), n);
        expect_poison((b + " (other buffer) beyond the count").c_str(), vbuf[cur ^ 1]->down<uint32_t>(n_max), n);
    }
}

// dn < 0: host form (count = n_max, scratch as knn.hip sizes it); else the count lives on the device (scratch of geom_layout)
static void case_sort_pairs(int n_max, int dn, int set, uint64_t seed) {
    begin_case("radix_sort_u32_pairs", "n=%d d_n=%d keys=%s", n_max, dn, KEYSET_NAME[set]);
    const size_t n = dn < 0 ? (size_t)n_max : (size_t)dn;
    const std::vector<uint32_t> keys = make_keys(set, n, seed);
    std::vector<uint32_t> idx(n);
    std::iota(idx.begin(), idx.end(), 0u);
    DBuf ka((size_t)n_max * 4, "keys_a"), kb((size_t)n_max * 4, "keys_b"), va((size_t)n_max * 4, "vals_a"), vb((size_t)n_max * 4, "vals_b");
    DBuf hist(dn < 0 ? knn_hist_bytes(n_max) : geom_hist_bytes(n_max), "hist"), bins(dn < 0 ? knn_bins_bytes() : geom_bins_bytes(n_max), "bin_total");
    DBuf cnt(4, "d_n");
    ka.up(keys); va.up(idx);
    cnt.up(std::vector<uint32_t>{(uint32_t)n});
    const int cur = radix_sort_u32_pairs(ka.p<uint32_t>(), kb.p<uint32_t>(), va.p<uint32_t>(), vb.p<uint32_t>(), n_max, hist.p<uint32_t>(),
                                         bins.p<uint32_t>(), g_s, dn < 0 ? nullptr : cnt.p<uint32_t>());
    sync_dev();
    DBuf* kbuf[2] = {&ka, &kb};
    DBuf* vbuf[2] = {&va, &vb};
    check_pairs("sorted", kbuf, vbuf, cur, n_max, keys, stable_order(keys, [](uint32_t k) { return k; }), true);
    end_case();
}

// the depth sort as the forward drives it: count and smallest key in device words, _low, then _top if the keys span 2^27
static void case_sort_depth(int n_max, int dn, int set, uint64_t seed) {
    begin_case("radix_sort_depth", "n=%d d_n=%d keys=%s", n_max, dn, KEYSET_NAME[set]);
    const size_t n = (size_t)dn;
    const std::vector<uint32_t> keys = make_keys(set, n, seed);
    std::vector<uint32_t> idx(n);
    std::iota(idx.begin(), idx.end(), 0u);
    uint32_t kmin = 0, kmax = 0;
    if (n) { kmin = *std::min_element(keys.begin(), keys.end()); kmax = *std::max_element(keys.begin(), keys.end()); }
    DBuf ka((size_t)n_max * 4, "keys_a"), kb((size_t)n_max * 4, "keys_b"), va((size_t)n_max * 4, "vals_a"), vb((size_t)n_max * 4, "vals_b");
    DBuf hist(geom_hist_bytes(n_max), "hist"), bins(geom_bins_bytes(n_max), "bin_total");
    DBuf cnt(4, "d_n"), dmin(4, "key_min");
    ka.up(keys); va.up(idx);
    cnt.up(std::vector<uint32_t>{(uint32_t)n});
    dmin.up(std::vector<uint32_t>{kmin});
    DBuf* kbuf[2] = {&ka, &kb};
    DBuf* vbuf[2] = {&va, &vb};
    int cur = radix_sort_depth_low(ka.p<uint32_t>(), kb.p<uint32_t>(), va.p<uint32_t>(), vb.p<uint32_t>(), n_max, hist.p<uint32_t>(),
                                   bins.p<uint32_t>(), g_s, cnt.p<uint32_t>(), dmin.p<uint32_t>());
    sync_dev();
    const std::vector<uint32_t> full = stable_order(keys, [](uint32_t k) { return k; });
    if (((uint64_t)kmax - kmin) >> DEPTH_SORT_LOW_BITS) {
        check_pairs("_low (low bits of key - key_min)", kbuf, vbuf, cur, n_max, keys,
                    stable_order(keys, [=](uint32_t k) { return (k - kmin) & LOW_MASK; }), true);
        if (cur == 0 || cur == 1) {
            cur = radix_sort_depth_top(ka.p<uint32_t>(), kb.p<uint32_t>(), va.p<uint32_t>(), vb.p<uint32_t>(), n_max, cur, hist.p<uint32_t>(),
                                       bins.p<uint32_t>(), g_s, cnt.p<uint32_t>(), dmin.p<uint32_t>());
            sync_dev();
            check_pairs("_low then _top", kbuf, vbuf, cur, n_max, keys, full, true);
        }
    } else {
        check_pairs("_low alone (span < 2^27)", kbuf, vbuf, cur, n_max, keys, full, true);
    }
    end_case();
}

// ---- 64-bit sort -------------------------------------------------------------------------------------------------------
// keys = tile << 32 | index.  tsdf_form: host count, scratch as tsdf.hip sizes it; else scratch of bin_layout, dn as above.
static void case_sort_u64(int n_max, int dn, int set, int b0, int b1, bool tsdf_form, uint64_t seed) {
    begin_case("radix_sort_u64_keys", "n=%d d_n=%d bits=[%d,%d) keys=%s%s", n_max, dn, b0, b1, KEYSET_NAME[set], tsdf_form ? " (tsdf scratch)" : "");
    const size_t n = dn < 0 ? (size_t)n_max : (size_t)dn;
    const std::vector<uint32_t> tiles = make_keys(set, n, seed);
    std::vector<uint64_t> keys(n);
    for (size_t i = 0; i < n; i++) keys[i] = ((uint64_t)tiles[i] << ENTRY_TILE_SHIFT) | (uint64_t)i;
    DBuf a((size_t)n_max * 8, "ent_a"), b((size_t)n_max * 8, "ent_b");
    DBuf hist(tsdf_form ? tsdf_hist_bytes(n_max) : bin_hist_bytes(n_max), "hist"), bins(tsdf_form ? tsdf_bins_bytes() : bin_bins_bytes(n_max), "bin_total");
    DBuf cnt(4, "d_n");
    a.up(keys);
    cnt.up(std::vector<uint32_t>{(uint32_t)n});
    const int cur = radix_sort_u64_keys(a.p<uint64_t>(), b.p<uint64_t>(), n_max, b0, b1, hist.p<uint32_t>(), bins.p<uint32_t>(), g_s,
                                        dn < 0 ? nullptr : cnt.p<uint32_t>());
    sync_dev();
    std::vector<uint64_t> want = keys;
    if (b1 > b0) {
        const int bits = b1 - b0;
        const uint64_t mask = bits >= 64 ? ~0ull : ((1ull << bits) - 1ull);
        std::stable_sort(want.begin(), want.end(), [=](uint64_t x, uint64_t y) { return ((x >> b0) & mask) < ((y >> b0) & mask); });
    }
    if (cur != 0 && cur != 1) {
        mismatch("ping-pong index", 1, 0, (unsigned long long)cur, 0);
    } else {
        if (b1 <= b0) {
            expect_word("ping-pong index of an empty bit range", (unsigned long long)cur, 0);
            expect_poison("ent_b (nothing may be written)", b.down<uint64_t>(n_max), 0);
            expect_poison("hist (nothing may be written)", hist.down<uint32_t>(hist.bytes / 4), 0);
            expect_poison("bin_total (nothing may be written)", bins.down<uint32_t>(bins.bytes / 4), 0);
        }
        DBuf* res = cur ? &b : &a;
        DBuf* other = cur ? &a : &b;
        const std::vector<uint64_t> g = res->down<uint64_t>(n_max);
        expect_eq("sorted keys", std::vector<uint64_t>(g.begin(), g.begin() + n), want);
        expect_poison("sorted keys beyond the count", g, n);
        expect_poison("other buffer beyond the count", other->down<uint64_t>(n_max), n);
    }
    end_case();
}

static void group_sorts_u32() {
    uint64_t seed = 100;
    for (int n : sort_sizes(TK32))
        for (int set = 0; set < K_SETS; set++) {
            case_sort_pairs(n, -1, set, seed++);
            case_sort_depth(n, n, set, seed++);
        }
    for (int n_max : {3 * TK32 + 5, 256 * TK32 + 1})
        for (int dn : {0, 1, TK32, n_max - 1, n_max})
            for (int set : {K_RANDOM, K_DEPTHS, K_TWO}) {
                case_sort_pairs(n_max, dn, set, seed++);
                case_sort_depth(n_max, dn, set, seed++);
            }
}
static void group_sorts_u64() {
    uint64_t seed = 500;
    const int ranges[5][2] = {{32, 33}, {32, 40}, {32, 45}, {32, 49}, {0, 64}};
    for (int n : sort_sizes(TK64))
        for (int set = 0; set < K_SETS; set++)
            for (const auto& r : ranges) case_sort_u64(n, -1, set, r[0], r[1], r[0] == 0, seed++);
    for (int n : {1, TK64 + 1}) {
        case_sort_u64(n, -1, K_RANDOM, 32, 32, false, seed++);
        case_sort_u64(n, -1, K_RANDOM, 40, 32, false, seed++);
    }
    for (int n_max : {3 * TK64 + 5, 256 * TK64 + 1})
        for (int dn : {0, 1, TK64, n_max - 1, n_max})
            for (const auto& r : ranges) case_sort_u64(n_max, dn, K_RANDOM, r[0], r[1], false, seed++);
}

// ---- count scan --------------------------------------------------------------------------------------------------------
static void case_count_scan(int P, int dn, uint64_t seed) {
    begin_case("launch_count_scan", "P=%d d_n=%d", P, dn);
    Rng r(seed);
    const size_t n = dn < 0 ? (size_t)P : (size_t)dn;
    const int nblocks = geom_layout(P).nblocks;
    std::vector<uint32_t> touched(P), gidx(P);
    for (auto& t : touched) t = (r.u32() & 63u) ? r.below(40) : r.below(20000);  // (the sum stays below 2^32)
    std::iota(gidx.begin(), gidx.end(), 0u);
    for (int i = P - 1; i > 0; i--) std::swap(gidx[i], gidx[r.below((uint32_t)i + 1)]);
    DBuf d_gidx((size_t)P * 4, "vals_b"), d_touched((size_t)P * 4, "tiles_touched"), d_sums(geom_blockwords_bytes(P), "block_sums"),
        d_offs(geom_blockwords_bytes(P), "block_offs"), d_local((size_t)P * 4, "keys_a"), d_total(geom_total_bytes(P), "total"), cnt(4, "d_n");
    d_gidx.up(std::vector<uint32_t>(gidx.begin(), gidx.begin() + n));  // ranks at and beyond the count are never read
    d_touched.up(touched);
    cnt.up(std::vector<uint32_t>{(uint32_t)n});
    launch_count_scan(P, d_gidx.p<uint32_t>(), d_touched.p<uint32_t>(), d_sums.p<uint32_t>(), d_offs.p<uint32_t>(), d_local.p<uint32_t>(),
                      d_total.p<uint32_t>() + 8, nblocks, g_s, dn < 0 ? nullptr : cnt.p<uint32_t>());
    sync_dev();
    const size_t nb = (n + 255) / 256;
    const std::vector<uint32_t> offs = d_offs.down<uint32_t>(nblocks), local = d_local.down<uint32_t>(P), total = d_total.down<uint32_t>(64);
    std::vector<uint32_t> got(n), want(n);
    uint32_t run = 0;
    for (size_t i = 0; i < n; i++) {
        want[i] = run;
        run += touched[gidx[i]];
        got[i] = offs[i >> 8] + local[i];
    }
    expect_eq("block_offs[r >> 8] + rank_local[r]", got, want);
    expect_poison("rank_local beyond the count", local, n);
    expect_poison("block_offs beyond the count's blocks", offs, nb);
    std::vector<uint32_t> wt(64, POISON32);
    wt[8] = run;
    wt[9] = 0;  // (the sum of the absent third array)
    expect_eq("total words", total, wt);
    end_case();
}
static void group_count_scan() {
    uint64_t seed = 900;
    for (int nb : {1, 2, 1023, 1024, 1025, 5003})
        for (int P : {256 * (nb - 1) + 1, 256 * nb - 19, 256 * nb}) {
            case_count_scan(P, -1, seed++);
            case_count_scan(P, P, seed++);
        }
    for (int P : {256 * 3 + 7, 256 * 1025 + 1})
        for (int dn : {0, 1, 257, P - 1, P}) case_count_scan(P, dn, seed++);
}

// ---- totals scan -------------------------------------------------------------------------------------------------------
// fill: 0 = all sums zero, 1 = one block holds 1, 2 = two blocks hold 1, 3 = random.  cap_rel: capacity - total (-1, 0, +1),
// 2 = the regular forward (capacity 0xFFFFFFFF, no status words)
static void case_scan_totals(int nblocks, int fill, int cap_rel, int zero_words, uint64_t seed) {
    begin_case("launch_scan_totals", "nblocks=%d fill=%d capacity-total=%d zero_words=%d", nblocks, fill, cap_rel, zero_words);
    Rng r(seed);
    std::vector<uint32_t> idx(nblocks, 0u), ref(nblocks, 0u), vis(nblocks, 0u), kmin(nblocks, 0xFFFFFFFFu), kmax(nblocks, 0u);
    auto plant = [&](int b, uint32_t c) {
        idx[b] = c * (1 + r.below(300)); if (fill != 3) idx[b] = c;
        ref[b] = idx[b] + (fill == 3 ? r.below(500) : 0);
        vis[b] = c;
        if (c) { const uint32_t x = r.u32(), y = r.u32(); kmin[b] = std::min(x, y); kmax[b] = std::max(x, y); }
    };
    if (fill == 1) plant((int)r.below(nblocks), 1);
    if (fill == 2) { plant(0, 1); if (nblocks > 1) plant(nblocks - 1, 1); else plant(0, 2); }
    if (fill == 3) for (int b = 0; b < nblocks; b++) plant(b, (r.u32() & 7u) ? 1 + r.below(256) : 0);
    uint32_t sa = 0, sr = 0, sv = 0, lo = 0xFFFFFFFFu, hi = 0;
    std::vector<uint32_t> wa(nblocks), wv(nblocks);
    for (int b = 0; b < nblocks; b++) {
        wa[b] = sa; wv[b] = sv;
        sa += idx[b]; sr += ref[b]; sv += vis[b];
        lo = std::min(lo, kmin[b]); hi = std::max(hi, kmax[b]);
    }
    if (lo > hi) lo = hi = 0;
    const bool presized = cap_rel != 2;
    const uint32_t capacity = presized ? (uint32_t)std::max<int64_t>(0, (int64_t)sa + cap_rel) : 0xFFFFFFFFu;
    const size_t P = (size_t)nblocks * 256;
    const size_t bw = geom_blockwords_bytes(P);
    DBuf d_idx(bw, "idx_block_sums"), d_idxo(bw, "idx_block_offs"), d_ref(bw, "ref_block_sums"), d_vis(bw, "vis_block_sums"), d_viso(bw, "vis_block_offs"),
        d_kmin(bw, "key_min_blocks"), d_kmax(bw, "key_max_blocks"), d_total(geom_total_bytes(P), "total"), d_zero((size_t)zero_words * 4, "ranges"),
        d_host(8 * 4, "host words"), d_status(4 * 4, "status words");
    d_idx.up(idx); d_ref.up(ref); d_vis.up(vis); d_kmin.up(kmin); d_kmax.up(kmax);
    launch_scan_totals(d_idx.p<uint32_t>(), d_idxo.p<uint32_t>(), d_ref.p<uint32_t>(), d_vis.p<uint32_t>(), d_viso.p<uint32_t>(), d_total.p<uint32_t>(),
                       nblocks, d_zero.p<uint32_t>(), zero_words, g_s, capacity, d_host.p<uint32_t>(), presized ? d_status.p<uint32_t>() : nullptr,
                       d_kmin.p<uint32_t>(), d_kmax.p<uint32_t>());
    sync_dev();
    expect_eq("idx_block_offs", d_idxo.down<uint32_t>(nblocks), wa);
    expect_eq("vis_block_offs", d_viso.down<uint32_t>(nblocks), wv);
    expect_eq("zero_words", d_zero.down<uint32_t>(zero_words), std::vector<uint32_t>(zero_words, 0u));
    std::vector<uint32_t> wt(64, POISON32);
    wt[0] = sa; wt[1] = sr; wt[2] = sv; wt[3] = std::min(sa, capacity); wt[4] = sa > capacity ? 1u : 0u; wt[5] = lo; wt[6] = hi;
    expect_eq("total words", d_total.down<uint32_t>(64), wt);
    expect_eq("host_out", d_host.down<uint32_t>(8), std::vector<uint32_t>{sa, sr, sv, lo, hi, POISON32, POISON32, POISON32});
    expect_eq("status_out", d_status.down<uint32_t>(4),
              presized ? std::vector<uint32_t>{sr, sa, sv, sa > capacity ? 1u : 0u} : std::vector<uint32_t>(4, POISON32));
    end_case();
}
static void group_scan_totals() {
    uint64_t seed = 1300;
    const int zw[] = {0, 1, 1023, 1024, 1025, 2 * 7500};
    int z = 0;
    for (int nb : {1, 2, 1023, 1024, 1025, 5003})
        for (int fill : {0, 1, 2, 3})
            for (int cap_rel : {-1, 0, 1, 2}) case_scan_totals(nb, fill, cap_rel, zw[z++ % 6], seed++);
}

// ---- slots and compaction (behind the totals scan, as the forward queues them) -------------------------------------------
// density: 0 = no Gaussian emits, 1 = about a quarter, 2 = all
static void case_slots_compact(int P, int density, uint64_t seed) {
    begin_case("launch_slots_and_compact", "P=%d density=%d", P, density);
    Rng r(seed);
    const int nblocks = geom_layout(P).nblocks;
    std::vector<uint32_t> touched(P), keys(P), idx_sums(nblocks, 0u), vis_sums(nblocks, 0u);
    for (int i = 0; i < P; i++) {
        touched[i] = density == 0 ? 0u : (density == 2 || (r.u32() & 3u) == 0) ? 1u + r.below(900) : 0u;
        keys[i] = r.u32();
        idx_sums[i >> 8] += touched[i];
        vis_sums[i >> 8] += touched[i] ? 1u : 0u;
    }
    const size_t bw = geom_blockwords_bytes(P);
    DBuf d_touched((size_t)P * 4, "tiles_touched"), d_keys((size_t)P * 4, "keys (unpacked)"), d_kout((size_t)P * 4, "keys (packed)"), d_iout((size_t)P * 4, "vals"),
        d_rec((size_t)P * REC_FLOATS * 4, "rec"), d_idx(bw, "idx_block_sums"), d_idxo(bw, "idx_block_offs"), d_vis(bw, "vis_block_sums"),
        d_viso(bw, "vis_block_offs"), d_total(geom_total_bytes(P), "total");
    d_touched.up(touched); d_keys.up(keys); d_idx.up(idx_sums); d_vis.up(vis_sums);
    launch_scan_totals(d_idx.p<uint32_t>(), d_idxo.p<uint32_t>(), nullptr, d_vis.p<uint32_t>(), d_viso.p<uint32_t>(), d_total.p<uint32_t>(), nblocks,
                       nullptr, 0, g_s);
    launch_slots_and_compact(P, d_touched.p<uint32_t>(), d_idxo.p<uint32_t>(), d_rec.p<float>(), d_keys.p<uint32_t>(), d_viso.p<uint32_t>(),
                             d_kout.p<uint32_t>(), d_iout.p<uint32_t>(), nblocks, g_s);
    sync_dev();
    std::vector<uint32_t> wrec((size_t)P * REC_FLOATS, POISON32), wk, wi;
    uint32_t run = 0;
    for (int i = 0; i < P; i++) {
        if (touched[i]) {
            wrec[(size_t)i * REC_FLOATS + 2] = run;  // (the float's bits)
            wk.push_back(keys[i]);
            wi.push_back((uint32_t)i);
        }
        run += touched[i];
    }
    const size_t V = wk.size();
    wk.resize(P, POISON32);
    wi.resize(P, POISON32);
    expect_eq("rec words (slot = word 2 of an emitting row, nothing else)", d_rec.down<uint32_t>((size_t)P * REC_FLOATS), wrec);
    expect_eq("packed keys", d_kout.down<uint32_t>(P), wk);
    expect_eq("packed indices", d_iout.down<uint32_t>(P), wi);
    const std::vector<uint32_t> total = d_total.down<uint32_t>(3);
    expect_word("total[0]", total[0], run);
    expect_word("total[2]", total[2], V);
    end_case();
}
static void group_slots_compact() {
    uint64_t seed = 1700;
    for (int P : {1, 2, 255, 256, 257, 5000, 256 * 1023, 256 * 1024 + 1, 256 * 1025 + 3})
        for (int density : {0, 1, 2}) case_slots_compact(P, density, seed++);
}

// ---- expansion ---------------------------------------------------------------------------------------------------------
// ranks: (width, height) of the tile rect of every depth rank.  clamp < 0: the regular forward (R_b = all instances);
// else the presized one: counts on the device, R_b = clamp instances, grid sized for `capacity`.
static void case_emit(const char* label, const std::vector<std::pair<uint32_t, uint32_t>>& ranks, long clamp, uint32_t capacity, uint64_t seed) {
    const int V = (int)ranks.size();
    uint64_t all = 0;
    for (const auto& wh : ranks) all += (uint64_t)wh.first * wh.second;
    const uint32_t R_b = clamp < 0 ? (uint32_t)all : (uint32_t)clamp;
    const uint32_t R_cap = clamp < 0 ? R_b : capacity;
    begin_case("launch_emit", "%s: V=%d instances=%llu R_b=%u capacity=%u%s", label, V, (unsigned long long)all, R_b, R_cap, clamp < 0 ? "" : " (d_counts)");
    Rng r(seed);
    const int tiles_x = 2048;
    const int P = V + V / 3 + 5;
    std::vector<uint32_t> gidx(P);
    std::iota(gidx.begin(), gidx.end(), 0u);
    for (int i = P - 1; i > 0; i--) std::swap(gidx[i], gidx[r.below((uint32_t)i + 1)]);
    gidx.resize(V);
    std::vector<uint32_t> rect(2 * (size_t)P, POISON32);
    const int nblocks_v = (V + 255) / 256;
    std::vector<uint32_t> block_offs(nblocks_v), rank_local(V);
    std::vector<uint64_t> want;
    want.reserve(R_b);
    uint64_t off = 0;
    for (int rk = 0; rk < V; rk++) {
        const uint32_t w = ranks[rk].first, h = ranks[rk].second, idx = gidx[rk];
        const uint32_t x0 = r.below((uint32_t)tiles_x - w + 1), y0 = r.below(1000);
        rect[2 * (size_t)idx] = x0 | (y0 << 16);
        rect[2 * (size_t)idx + 1] = w;
        if ((rk & 255) == 0) block_offs[rk >> 8] = (uint32_t)off;
        rank_local[rk] = (uint32_t)off - block_offs[rk >> 8];
        for (uint32_t k = 0; k < w * h && want.size() < R_b; k++)
            want.push_back(((uint64_t)((y0 + k / w) * (uint32_t)tiles_x + x0 + k % w) << ENTRY_TILE_SHIFT) | idx);
        off += (uint64_t)w * h;
    }
    const BinLayout BL = bin_layout(R_cap);
    const GeomLayout GL = geom_layout(P);
    DBuf d_gidx((size_t)P * 4, "vals_b"), d_offs(geom_blockwords_bytes(P), "block_offs"), d_local((size_t)P * 4, "keys_a"), d_rect((size_t)P * 8, "tight_rect"),
        d_ent(BL.ent_b - BL.ent_a, "ent_a"), d_qhit(R_cap ? R_cap : 1, "qhit"), d_flag(R_cap ? R_cap : 1, "rec_flag"), d_counts(8, "counts");
    d_gidx.up(gidx); d_offs.up(block_offs); d_local.up(rank_local); d_rect.up(rect);
    d_counts.up(std::vector<uint32_t>{(uint32_t)V, R_b});
    if (clamp < 0)
        launch_emit(V, R_b, tiles_x, d_gidx.p<uint32_t>(), d_offs.p<uint32_t>(), nblocks_v, d_local.p<uint32_t>(), d_rect.p<uint2>(), d_ent.p<uint64_t>(),
                    d_qhit.p<uint8_t>(), d_flag.p<uint8_t>(), g_s, nullptr);
    else
        launch_emit(P, R_cap, tiles_x, d_gidx.p<uint32_t>(), d_offs.p<uint32_t>(), GL.nblocks, d_local.p<uint32_t>(), d_rect.p<uint2>(), d_ent.p<uint64_t>(),
                    d_qhit.p<uint8_t>(), d_flag.p<uint8_t>(), g_s, d_counts.p<uint32_t>());
    sync_dev();
    const size_t ent_words = d_ent.bytes / 8;
    want.resize(ent_words, POISON64);
    expect_eq("entries", d_ent.down<uint64_t>(ent_words), want);
    std::vector<uint8_t> wq(d_qhit.bytes, POISON8);
    std::fill(wq.begin(), wq.begin() + R_b, (uint8_t)0);
    expect_eq("qhit", d_qhit.down<uint8_t>(d_qhit.bytes), wq);
    expect_eq("rec_flag", d_flag.down<uint8_t>(d_flag.bytes), wq);
    end_case();
}
static void group_emit() {
    uint64_t seed = 2100;
    typedef std::vector<std::pair<uint32_t, uint32_t>> Ranks;
    auto random_ranks = [&](int V, uint64_t sd) {
        Rng r(sd);
        Ranks k(V);
        for (auto& wh : k) {
            const uint32_t c = r.below(16);
            wh = c < 10 ? std::make_pair(1u, 1u) : (c < 15 || V > 100000) ? std::make_pair(1u + r.below(4), 1u + r.below(4)) : std::make_pair(1u + r.below(40), 1u + r.below(30));
        }
        return k;
    };
    auto total_of = [](const Ranks& k) { uint64_t s = 0; for (const auto& wh : k) s += (uint64_t)wh.first * wh.second; return s; };
    // the last rank is widened until the instance count has the wanted remainder
    for (uint32_t rem : {0u, 1u, 2u, 3u, 1023u, 5u, 6u, 7u, 1020u}) {
        Ranks k = random_ranks(700, seed++);
        k.back() = {1u, 1u};
        const uint32_t have = (uint32_t)(total_of(k) % 1024);
        k.back().first += (rem + 1024u - have) % 1024u;
        char label[64];
        snprintf(label, sizeof label, "instances = %u mod 1024", rem);
        case_emit(label, k, -1, 0, seed++);
    }
    case_emit("one instance", Ranks{{1u, 1u}}, -1, 0, seed++);
    case_emit("one rank over five windows", Ranks{{100u, 50u}}, -1, 0, seed++);
    {   // big splats in front, far ones behind: windows of a single rank, windows of a thousand
        Ranks k = {{3u, 2u}, {100u, 50u}, {1u, 1u}, {2047u, 3u}, {1u, 7u}};
        Ranks tail = random_ranks(3000, seed++);
        k.insert(k.end(), tail.begin(), tail.end());
        case_emit("large ranks among small ones", k, -1, 0, seed++);
    }
    case_emit("one-tile ranks only (1024 staged ranks per window)", Ranks(3000, {1u, 1u}), -1, 0, seed++);
    {   // the window begins inside a two-tile rank and every later slot of it begins a rank
        Ranks k(1023, {1u, 1u});
        k.push_back({2u, 1u});
        k.insert(k.end(), 2500, {1u, 1u});
        case_emit("one-tile ranks behind a rank that straddles the window", k, -1, 0, seed++);
    }
    for (int groups : {1, 2, 256, 257, 4097}) {
        char label[64];
        for (int V : {256 * (groups - 1) + 1, 256 * groups}) {
            snprintf(label, sizeof label, "%d groups of 256 ranks", groups);
            const Ranks k = random_ranks(V, seed++);
            case_emit(label, k, -1, 0, seed++);
        }
    }
    for (int V : {1, 700, 256 * 257 + 9}) {  // presized: the count is clamped, the last rank cut
        Ranks k = random_ranks(V, seed++);
        k.back() = {30u, 20u};
        const uint32_t all = (uint32_t)total_of(k);
        case_emit("clamped inside the last rank", k, (long)all - 301, all - 301, seed++);
        case_emit("clamped, grid larger than the count", k, (long)all - 301, all + 5000, seed++);
        case_emit("not clamped, grid larger than the count", k, (long)all, all + 5000, seed++);
        case_emit("clamped to one instance", k, 1, 4096, seed++);
        case_emit("clamped to nothing", k, 0, 4096, seed++);
    }
}

// ---- tile ranges -------------------------------------------------------------------------------------------------------
// pattern: 0 = one tile holds the whole list, 1 = every present tile once (some absent), 2 = random runs (some absent)
static void case_tile_ranges(int R_max, int dn, int pattern, uint64_t seed) {
    begin_case("launch_tile_ranges", "R=%d d_n=%d pattern=%d", R_max, dn, pattern);
    Rng r(seed);
    const size_t R = dn < 0 ? (size_t)R_max : (size_t)dn;
    std::vector<uint64_t> ent(R);
    uint32_t tile = pattern == 0 ? 37u : r.below(3);
    for (size_t i = 0; i < R; i++) {
        ent[i] = ((uint64_t)tile << ENTRY_TILE_SHIFT) | r.u32();
        if (pattern == 1) tile += 1 + (r.below(4) == 0 ? r.below(3) : 0);
        if (pattern == 2 && r.below(6) == 0) tile += 1 + (r.below(3) == 0 ? r.below(5) : 0);
    }
    const size_t tiles = (size_t)tile + 3;
    DBuf d_ent(bin_layout(R_max).ent_b - bin_layout(R_max).ent_a, "entries"), d_ranges(tiles * 8, "ranges"), cnt(4, "d_n");
    d_ent.up(ent);
    d_ranges.zero();
    cnt.up(std::vector<uint32_t>{(uint32_t)R});
    launch_tile_ranges(R_max, d_ent.p<uint64_t>(), d_ranges.p<uint32_t>(), g_s, dn < 0 ? nullptr : cnt.p<uint32_t>());
    sync_dev();
    std::vector<uint32_t> want(2 * tiles, 0u);
    for (size_t i = 0; i < R; i++) {
        const uint32_t t = entry_tile(ent[i]);
        if (i == 0 || entry_tile(ent[i - 1]) != t) want[2 * t] = (uint32_t)i;
        want[2 * t + 1] = (uint32_t)i + 1;
    }
    expect_eq("ranges", d_ranges.down<uint32_t>(2 * tiles), want);
    end_case();
}
static void group_tile_ranges() {
    uint64_t seed = 2600;
    for (int R : {1, 2, 3, 4, 5, 6, 7, 8, 9, 1023, 1024, 1025, 1027, 1000003})
        for (int pattern : {0, 1, 2}) {
            case_tile_ranges(R, -1, pattern, seed++);
            case_tile_ranges(R, R, pattern, seed++);
        }
    for (int R_max : {9, 4099, 1000003})
        for (int dn : {0, 1, 2, 3, 4, 5, R_max - 2, R_max - 1})
            for (int pattern : {0, 2}) case_tile_ranges(R_max, dn, pattern, seed++);
}

// ---- tile order --------------------------------------------------------------------------------------------------------
// lengths: 0 = all lists empty, 1 = all below 4, 2 = mixed, with lists beyond 4 * 2047 and lists of 0..3
static void case_tile_order(int tiles, int lengths, bool with_zero_word, uint64_t seed) {
    begin_case("launch_tile_order", "tiles=%d lengths=%d zero_word=%d", tiles, lengths, (int)with_zero_word);
    Rng r(seed);
    std::vector<uint32_t> ranges(2 * (size_t)tiles), len(tiles);
    for (int i = 0; i < tiles; i++) {
        const uint32_t c = r.below(8);
        len[i] = lengths == 0 ? 0u : lengths == 1 ? r.below(4) : c == 0 ? r.below(4) : c == 1 ? 4u * 2047u - 4u + r.below(12) : c == 2 ? 8188u + r.below(100000) : r.below(9000);
        ranges[2 * (size_t)i] = r.below(1u << 30);
        ranges[2 * (size_t)i + 1] = ranges[2 * (size_t)i] + len[i];
    }
    DBuf d_ranges((size_t)tiles * 8, "ranges"), d_order((size_t)tiles * 4, "tile_order"), d_word(4, "zero_word");
    d_ranges.up(ranges);
    launch_tile_order(tiles, d_ranges.p<uint32_t>(), d_order.p<uint32_t>(), g_s, with_zero_word ? d_word.p<uint32_t>() : nullptr);
    sync_dev();
    const std::vector<uint32_t> order = d_order.down<uint32_t>(tiles);
    std::vector<uint8_t> seen(tiles, 0);
    uint32_t prev = 0xFFFFFFFFu;
    for (int i = 0; i < tiles; i++) {
        if (order[i] >= (uint32_t)tiles || seen[order[i]]) { mismatch("order is not a permutation of the tiles", tiles, i, order[i], 0); break; }
        seen[order[i]] = 1;
        const uint32_t b = std::min(len[order[i]] >> 2, 2047u);
        if (b > prev) { mismatch("min(len >> 2, 2047) increases along the order", tiles, i, b, prev); break; }
        prev = b;
    }
    expect_word("zero_word", d_word.down<uint32_t>(1)[0], with_zero_word ? 0u : POISON32);
    end_case();
}
static void group_tile_order() {
    uint64_t seed = 3000;
    for (int tiles : {1, 2, 1023, 1024, 1025, 7500, 66049})
        for (int lengths : {0, 1, 2})
            for (bool zw : {false, true}) case_tile_order(tiles, lengths, zw, seed++);
}

int main(int argc, char** argv) {
    const char* only = argc > 1 ? argv[1] : "";
    const auto t0 = std::chrono::steady_clock::now();
    HIP_OK(hipSetDevice(0));
    HIP_OK(hipStreamCreate(&g_s));
    struct Group { const char* name; void (*run)(); };
    const Group groups[] = {{"sorts_u32", group_sorts_u32},     {"sorts_u64", group_sorts_u64},       {"count_scan", group_count_scan},
                            {"scan_totals", group_scan_totals}, {"slots_compact", group_slots_compact}, {"emit", group_emit},
                            {"tile_ranges", group_tile_ranges}, {"tile_order", group_tile_order}};
    for (const Group& g : groups) {
        if (!strstr(g.name, only)) continue;
        const auto g0 = std::chrono::steady_clock::now();
        const int failed_before = g_failed;
        g.run();
        printf("group %-14s %6.2f s, %d failed\n", g.name, std::chrono::duration<double>(std::chrono::steady_clock::now() - g0).count(), g_failed - failed_before);
        fflush(stdout);
    }
    HIP_OK(hipStreamDestroy(g_s));
    int cases = 0;
    for (const auto& kv : g_count) { printf("cases %-26s %d\n", kv.first.c_str(), kv.second); cases += kv.second; }
    printf("%d cases, %d failed, %.1f s\n", cases, g_failed, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    if (g_failed || cases == 0) { printf("binning_ops FAILED (%d)\n", g_failed); return 1; }
    printf("binning_ops OK\n");
    return 0;
}
