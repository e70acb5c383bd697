// Standalone check of the short kernels between the preprocess and the blend (g4splat_amd/csrc/binning.hip) at the sizes
// where their single-sweep forms can go wrong: the block-sum scan (registers of a pass, passes, wave and run borders),
// the instance expansion (group probe, speculative staging of up to five rank groups, owner max-scan), the count scan
// and the tile order.  Every result is compared bit for bit with a plain host restatement kept in this file.  Built
// and run by tests/test_gpu_preblend_edges.py:
//   hipcc <CXXFLAGS of g4splat_amd/csrc/Makefile> tests/hip_unit/preblend_edges.hip g4splat_amd/csrc/binning.hip -o preblend_edges
// Every device buffer is followed by a poisoned guard that is checked after each case; outputs start out as poison, so
// a word the kernels must not write shows.  A HIP error ends the program at once.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../g4splat_amd/csrc/g4s_internal.h"
using namespace g4s;

static hipStream_t g_s;
static std::string g_case = "(start)";
static bool g_bad = false;
static int g_cases = 0, g_failed = 0;

#define HIP_OK(expr)                                                                                        \
    do {                                                                                                    \
        const hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) {                                                                             \
            printf("HIP error %d (%s) at line %d: %s\n", (int)e_, hipGetErrorString(e_), __LINE__, #expr); \
            printf("preblend_edges ABORTED in case %s\n", g_case.c_str());                                  \
            fflush(stdout);                                                                                 \
            exit(2);                                                                                        \
        }                                                                                                   \
    } while (0)

constexpr size_t GUARD = 4096;
constexpr uint8_t POISON8 = 0x5C;
constexpr uint32_t POISON32 = 0x5C5C5C5Cu;

static void bad(const char* what, size_t i, unsigned long long got, unsigned long long want) {
    if (!g_bad) printf("MISMATCH case %s: %s at %zu: got 0x%llx want 0x%llx\n", g_case.c_str(), what, i, got, want);
    g_bad = true;
}

struct Buf;
static std::vector<Buf*> g_live;
struct Buf {  // `count` elements of T and a guard, all poison to begin with
    char* base = nullptr;
    size_t bytes;
    const char* name;
    Buf(size_t bytes_, const char* name_) : bytes(bytes_), name(name_) {
        HIP_OK(hipMalloc((void**)&base, bytes + GUARD));
        HIP_OK(hipMemsetAsync(base, POISON8, bytes + GUARD, g_s));
        g_live.push_back(this);
    }
    ~Buf() {
        g_live.erase(std::find(g_live.begin(), g_live.end(), this));
        HIP_OK(hipFree(base));
    }
    Buf(const Buf&) = delete;
    template <typename T> T* p() { return reinterpret_cast<T*>(base); }
    template <typename T> void up(const std::vector<T>& v) {
        if (v.size() * sizeof(T) > bytes) { printf("harness bug: upload past %s\n", name); exit(3); }
        if (!v.empty()) HIP_OK(hipMemcpyAsync(base, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, g_s));
        HIP_OK(hipStreamSynchronize(g_s));
    }
    template <typename T> std::vector<T> down() {
        std::vector<T> v(bytes / sizeof(T));
        HIP_OK(hipStreamSynchronize(g_s));
        if (!v.empty()) HIP_OK(hipMemcpy(v.data(), base, v.size() * sizeof(T), hipMemcpyDeviceToHost));
        return v;
    }
    void check_guard() {
        std::vector<uint8_t> g(GUARD);
        HIP_OK(hipMemcpy(g.data(), base + bytes, GUARD, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < GUARD; i++)
            if (g[i] != POISON8) { bad((std::string("guard behind ") + name).c_str(), i, g[i], POISON8); return; }
    }
};

static void begin_case(const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_case = buf;
    g_bad = false;
    g_cases++;
}
static void end_case() {
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(g_s));
    for (Buf* b : g_live) b->check_guard();
    if (g_bad) g_failed++;
}
// got against want over the whole buffer: `want` is padded with poison to the buffer's size
template <typename T>
static void expect(const char* what, Buf& b, std::vector<T> want) {
    T poison;
    memset(&poison, POISON8, sizeof(T));
    const std::vector<T> got = b.down<T>();
    if (want.size() > got.size()) { printf("harness bug: %s expects more than the buffer holds\n", what); exit(3); }
    want.resize(got.size(), poison);
    for (size_t i = 0; i < got.size(); i++)
        if (got[i] != want[i]) { bad(what, i, (unsigned long long)got[i], (unsigned long long)want[i]); return; }
}

struct Rng {  // xorshift64*
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x2545F4914F6CDD1Dull + 88172645463325252ull) {}
    uint32_t u32() {
        s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
        return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32);
    }
    uint32_t below(uint32_t n) { return (uint32_t)(((uint64_t)u32() * n) >> 32); }
};

// ---- block-sum scan ------------------------------------------------------------------------------------------------------
// Two arrays (launch_scan_totals), with and without the reference sums and the key ranges.  big: sums near 2^31 (the
// 32-bit totals wrap, as the kernel's do).
static void case_scan_two(int nblocks, bool with_ref_keys, bool big, int zero_words, uint64_t seed) {
    begin_case("scan_totals nblocks=%d ref+keys=%d big=%d zero_words=%d", nblocks, (int)with_ref_keys, (int)big, zero_words);
    Rng r(seed);
    std::vector<uint32_t> a(nblocks), v(nblocks), ref(nblocks), kmin(nblocks), kmax(nblocks);
    for (int i = 0; i < nblocks; i++) {
        v[i] = r.below(257);
        a[i] = big ? 0x7FFFFF00u + r.below(512) : v[i] * r.below(300);
        ref[i] = a[i] + r.below(1000);
        const uint32_t x = r.u32(), y = r.u32();
        kmin[i] = v[i] ? std::min(x, y) : 0xFFFFFFFFu;
        kmax[i] = v[i] ? std::max(x, y) : 0u;
    }
    std::vector<uint32_t> wa(nblocks), wv(nblocks);
    uint32_t sa = 0, sv = 0, sr = 0, lo = 0xFFFFFFFFu, hi = 0u;
    for (int i = 0; i < nblocks; i++) {
        wa[i] = sa; wv[i] = sv;
        sa += a[i]; sv += v[i]; sr += ref[i];
        lo = std::min(lo, kmin[i]); hi = std::max(hi, kmax[i]);
    }
    if (lo > hi) lo = hi = 0u;
    const size_t bw = (size_t)nblocks * 4;
    Buf d_a(bw, "a_sums"), d_ao(bw, "a_offs"), d_v(bw, "b_sums"), d_vo(bw, "b_offs"), d_ref(bw, "ref_sums"), d_kmin(bw, "key_min_blocks"),
        d_kmax(bw, "key_max_blocks"), d_total(64 * 4, "total"), d_zero((size_t)zero_words * 4, "zero words"), d_host(8 * 4, "host words");
    d_a.up(a); d_v.up(v); d_ref.up(ref); d_kmin.up(kmin); d_kmax.up(kmax);
    launch_scan_totals(d_a.p<uint32_t>(), d_ao.p<uint32_t>(), with_ref_keys ? d_ref.p<uint32_t>() : nullptr, d_v.p<uint32_t>(), d_vo.p<uint32_t>(),
                       d_total.p<uint32_t>(), nblocks, zero_words ? d_zero.p<uint32_t>() : nullptr, zero_words, g_s, 0xFFFFFFFFu, d_host.p<uint32_t>(), nullptr,
                       with_ref_keys ? d_kmin.p<uint32_t>() : nullptr, with_ref_keys ? d_kmax.p<uint32_t>() : nullptr);
    expect("a_offs", d_ao, wa);
    expect("b_offs", d_vo, wv);
    expect("zero words", d_zero, std::vector<uint32_t>(zero_words, 0u));
    std::vector<uint32_t> wt = {sa, with_ref_keys ? sr : 0u, sv, sa, 0u};
    std::vector<uint32_t> wh = {sa, with_ref_keys ? sr : 0u, sv};
    if (with_ref_keys) { wt.push_back(lo); wt.push_back(hi); wh.push_back(lo); wh.push_back(hi); }
    expect("total words", d_total, wt);
    expect("host words", d_host, wh);
    end_case();
}
// One array (b_sums == NULL) behind its gather, as launch_count_scan runs them: V depth ranks among P Gaussians, the count
// either on the host or in a device word (the launches are then sized for P).  big: block sums near 2^31.
static void case_count_scan(int V, int P, bool device_count, bool big, uint64_t seed) {
    const int nblocks = (V + 255) / 256;
    begin_case("count_scan V=%d P=%d (%d blocks) d_n=%d big=%d", V, P, nblocks, (int)device_count, (int)big);
    Rng r(seed);
    std::vector<uint32_t> touched(P), gidx(P);
    // zeros among the neighbours: only the Gaussians that the ranks name emit
    std::iota(gidx.begin(), gidx.end(), 0u);
    for (int i = P - 1; i > 0; i--) std::swap(gidx[i], gidx[r.below((uint32_t)i + 1)]);
    std::fill(touched.begin(), touched.end(), 0u);
    for (int k = 0; k < V; k++) touched[gidx[k]] = big ? 0x7FFFFFu + r.below(64) : 1u + ((r.u32() & 31u) ? r.below(6) : r.below(5000));
    const int nb_launch = device_count ? (P + 255) / 256 : nblocks;
    Buf d_gidx((size_t)P * 4, "gidx"), d_touched((size_t)P * 4, "tiles_touched"), d_sums((size_t)nb_launch * 4, "block_sums"),
        d_offs((size_t)nb_launch * 4, "block_offs"), d_local((size_t)P * 4, "rank_local"), d_total(64 * 4, "total"), cnt(4, "d_n");
    d_gidx.up(gidx); d_touched.up(touched);
    cnt.up(std::vector<uint32_t>{(uint32_t)V});
    launch_count_scan(device_count ? P : V, d_gidx.p<uint32_t>(), d_touched.p<uint32_t>(), d_sums.p<uint32_t>(), d_offs.p<uint32_t>(), d_local.p<uint32_t>(),
                      d_total.p<uint32_t>() + 8, nb_launch, g_s, device_count ? cnt.p<uint32_t>() : nullptr);
    std::vector<uint32_t> wsums(nblocks, 0u), woffs(nblocks), wlocal(V);
    uint32_t run = 0;
    for (int k = 0; k < V; k++) {
        if ((k & 255) == 0) woffs[k >> 8] = run;
        wlocal[k] = run - woffs[k >> 8];
        run += touched[gidx[k]];
        wsums[k >> 8] += touched[gidx[k]];
    }
    expect("block_sums", d_sums, wsums);
    expect("block_offs", d_offs, woffs);
    expect("rank_local", d_local, wlocal);
    std::vector<uint32_t> wt(10, POISON32);
    wt[8] = run; wt[9] = 0u;
    expect("total words", d_total, wt);
    end_case();
}
static void group_scan() {
    uint64_t seed = 11;
    const int zw[] = {0, 1, 1023, 15000};
    int z = 0;
    for (int nb : {1, 63, 64, 1023, 1024, 1025, 5860, 12001})
        for (int with_ref : {0, 1})
            for (int big : {0, 1}) case_scan_two(nb, with_ref != 0, big != 0, zw[z++ % 4], seed++);
    for (int zero_words : zw) case_scan_two(5860, true, false, zero_words, seed++);
    for (int nb : {1, 63, 64, 1023, 1024, 1025, 5860, 12001})
        for (int dn : {0, 1}) {
            Rng r(seed);
            const int V = 256 * (nb - 1) + 1 + (int)r.below(256);  // the last block is partial
            case_count_scan(V, V + 300, dn != 0, nb == 1025, seed++);
        }
    for (int V : {1, 255, 256, 257, 513})  // one, two and three blocks of the gather
        for (int dn : {0, 1}) case_count_scan(V, 2 * V + 7, dn != 0, false, seed++);
}
// ---- expansion -------------------------------------------------------------------------------------------------------------
typedef std::vector<std::pair<uint32_t, uint32_t>> Ranks;  // (width, height) of the tile rect of every depth rank
// clamp < 0: the regular forward.  Else the presized form: the counts (V, R_b = clamp) in device words, the launch sized for
// all P Gaussians and `capacity` instances.
static void case_emit(const char* label, const Ranks& ranks, long clamp, uint32_t capacity, uint64_t seed) {
    const int V = (int)ranks.size();
    uint64_t all = 0;
    for (const auto& wh : ranks) all += (uint64_t)wh.first * wh.second;
    const uint32_t R_b = clamp < 0 ? (uint32_t)all : (uint32_t)clamp;
    const uint32_t R_cap = clamp < 0 ? R_b : capacity;
    begin_case("emit %s: V=%d instances=%llu R_b=%u capacity=%u", label, V, (unsigned long long)all, R_b, R_cap);
    Rng r(seed);
    const int tiles_x = 4100;
    const int P = V + V / 2 + 3;
    std::vector<uint32_t> gidx(P);
    std::iota(gidx.begin(), gidx.end(), 0u);
    for (int i = P - 1; i > 0; i--) std::swap(gidx[i], gidx[r.below((uint32_t)i + 1)]);
    gidx.resize(V);
    std::vector<uint32_t> rect(2 * (size_t)P, POISON32), block_offs((V + 255) / 256), rank_local(V);
    std::vector<uint64_t> want;
    uint64_t off = 0;
    for (int k = 0; k < V; k++) {
        const uint32_t w = ranks[k].first, h = ranks[k].second, g = gidx[k];
        const uint32_t x0 = r.below((uint32_t)tiles_x - w + 1), y0 = r.below(500);
        rect[2 * (size_t)g] = x0 | (y0 << 16);
        rect[2 * (size_t)g + 1] = w;
        if ((k & 255) == 0) block_offs[k >> 8] = (uint32_t)off;
        rank_local[k] = (uint32_t)off - block_offs[k >> 8];
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++)
                if (want.size() < R_b) want.push_back(((uint64_t)((y0 + y) * (uint32_t)tiles_x + x0 + x) << ENTRY_TILE_SHIFT) | g);
        off += (uint64_t)w * h;
    }
    const size_t cap = R_cap ? R_cap : 1;
    Buf d_gidx((size_t)P * 4, "gidx"), d_offs((size_t)((P + 255) / 256) * 4, "block_offs"), d_local((size_t)P * 4, "rank_local"), d_rect((size_t)P * 8, "tight_rect"),
        d_ent(cap * 8, "entries"), d_qhit(cap, "qhit"), d_flag(cap, "rec_flag"), d_counts(8, "counts");
    d_gidx.up(gidx); d_offs.up(block_offs); d_local.up(rank_local); d_rect.up(rect);
    d_counts.up(std::vector<uint32_t>{(uint32_t)V, R_b});
    if (clamp < 0)
        launch_emit(V, R_b, tiles_x, d_gidx.p<uint32_t>(), d_offs.p<uint32_t>(), (V + 255) / 256, d_local.p<uint32_t>(), d_rect.p<uint2>(), d_ent.p<uint64_t>(),
                    d_qhit.p<uint8_t>(), d_flag.p<uint8_t>(), g_s, nullptr);
    else
        launch_emit(P, R_cap, tiles_x, d_gidx.p<uint32_t>(), d_offs.p<uint32_t>(), (P + 255) / 256, d_local.p<uint32_t>(), d_rect.p<uint2>(), d_ent.p<uint64_t>(),
                    d_qhit.p<uint8_t>(), d_flag.p<uint8_t>(), g_s, d_counts.p<uint32_t>());
    expect("entries", d_ent, want);                                    // (nothing beyond R_b: the rest is still poison)
    expect("qhit", d_qhit, std::vector<uint8_t>(R_b, (uint8_t)0));
    expect("rec_flag", d_flag, std::vector<uint8_t>(R_b, (uint8_t)0));
    end_case();
}
static Ranks mixed_ranks(int V, uint64_t seed) {
    Rng r(seed);
    Ranks k(V);
    for (auto& wh : k) {
        const uint32_t c = r.below(16);
        wh = c < 9 ? std::make_pair(1u, 1u) : c < 15 ? std::make_pair(1u + r.below(5), 1u + r.below(4)) : std::make_pair(1u + r.below(60), 1u + r.below(40));
    }
    return k;
}
static Ranks small_ranks(int V, uint64_t seed) {  // about two instances per rank
    Rng r(seed);
    Ranks k(V);
    for (auto& wh : k) wh = r.below(16) < 12 ? std::make_pair(1u, 1u) : std::make_pair(1u + r.below(4), 1u + r.below(3));
    return k;
}
static void group_emit() {
    uint64_t seed = 701;
    case_emit("one Gaussian over 4 000 tiles (four windows of a single rank)", Ranks{{80u, 50u}}, -1, 0, seed++);
    case_emit("1 025 one-tile ranks", Ranks(1025, {1u, 1u}), -1, 0, seed++);
    {   // a two-tile rank reaches into the second window from the first, 1 023 one-tile ranks begin in it, one more behind
        Ranks k(1023, {1u, 1u});
        k.push_back({2u, 1u});
        k.insert(k.end(), 1025, {1u, 1u});
        case_emit("1 024 ranks reach into one window, the first from before it", k, -1, 0, seed++);
    }
    {   // ranks of four tiles: rank 256 begins at slot 1 024 -- window, rank and 256-rank group begin together
        Ranks k(256 * 5 + 3, {2u, 2u});
        case_emit("window boundary on a rank and a group boundary", k, -1, 0, seed++);
        k[255] = {5u, 1u};  // ... and one slot later: the window begins with the last instance of the group before
        case_emit("window boundary one slot before a group boundary", k, -1, 0, seed++);
        k[255] = {3u, 1u};  // ... and one slot earlier: the group's first rank is the last to begin in the window before
        case_emit("window boundary one slot behind a group boundary", k, -1, 0, seed++);
    }
    // one-tile ranks only: every window spans four whole groups, five with an offset
    case_emit("four groups per window", Ranks(256 * 9, {1u, 1u}), -1, 0, seed++);
    {
        Ranks k(256 * 9 + 77, {1u, 1u});
        k[100] = {2u, 1u};
        case_emit("five groups per window", k, -1, 0, seed++);
    }
    for (uint32_t R_b : {1u, 1023u, 1024u, 1025u}) {  // the last rank is widened to the wanted count
        Ranks k = mixed_ranks(R_b > 600 ? 300 : 0, seed++);
        uint64_t have = 0;
        for (const auto& wh : k) have += (uint64_t)wh.first * wh.second;
        while (have >= R_b && !k.empty()) { have -= (uint64_t)k.back().first * k.back().second; k.pop_back(); }
        k.push_back({R_b - (uint32_t)have, 1u});
        char label[64];
        snprintf(label, sizeof label, "R_b = %u", R_b);
        case_emit(label, k, -1, 0, seed++);
    }
    case_emit("large ranks among small ones", mixed_ranks(5000, seed), -1, 0, seed + 1);
    seed += 2;
    // more than 2 044 groups: a 256-way round before the probe; near and far ranks, and one-tile ranks only
    case_emit("2 300 groups", small_ranks(256 * 2300 - 9, seed), -1, 0, seed + 1);
    seed += 2;
    case_emit("2 045 groups of one-tile ranks", Ranks(256 * 2045, {1u, 1u}), -1, 0, seed++);
    for (int V : {1, 900, 256 * 9 + 5}) {  // presized: the counts on the device, smaller than the grid allows
        Ranks k = mixed_ranks(V, seed++);
        k.back() = {40u, 30u};
        uint32_t all = 0;
        for (const auto& wh : k) all += wh.first * wh.second;
        case_emit("presized, clamped inside the last rank", k, (long)all - 417, all - 417, seed++);
        case_emit("presized, grid larger than the count", k, (long)all - 417, all + 7000, seed++);
        case_emit("presized, not clamped", k, (long)all, all + 7000, seed++);
        case_emit("presized, one instance", k, 1, 5000, seed++);
        case_emit("presized, nothing", k, 0, 5000, seed++);
    }
}

// ---- tile order ------------------------------------------------------------------------------------------------------------
// The kernel's contract: a permutation of the tiles in which min(len >> 2, 2047) never increases.  Inside a bucket the
// kernel's order is that of its LDS atomics; the restatement accepts any.
// lengths: 0 = all lists empty, 1 = all lists equal, 2 = mixed, with lists beyond what the 2 048 buckets resolve
static void case_tile_order(int tiles, int lengths, bool backward_form, uint64_t seed) {
    begin_case("tile_order tiles=%d lengths=%d backward=%d", tiles, lengths, (int)backward_form);
    Rng r(seed);
    std::vector<uint32_t> ranges(2 * (size_t)tiles), len(tiles);
    for (int i = 0; i < tiles; i++) {
        const uint32_t c = r.below(6);
        len[i] = lengths == 0 ? 0u : lengths == 1 ? 777u : c == 0 ? r.below(4) : c == 1 ? 4u * 2047u - 6u + r.below(12) : c == 2 ? 8188u + r.below(1u << 20) : r.below(9000);
        ranges[2 * (size_t)i] = backward_form ? 0u : r.below(1u << 30);  // (the backward's pairs are (0, depth))
        ranges[2 * (size_t)i + 1] = ranges[2 * (size_t)i] + len[i];
    }
    Buf d_ranges((size_t)tiles * 8, "ranges"), d_order((size_t)tiles * 4, "tile_order"), d_word(4, "zero_word");
    d_ranges.up(ranges);
    launch_tile_order(tiles, d_ranges.p<uint32_t>(), d_order.p<uint32_t>(), g_s, backward_form ? d_word.p<uint32_t>() : nullptr);
    const std::vector<uint32_t> order = d_order.down<uint32_t>();
    std::vector<uint8_t> seen(tiles, 0);
    std::vector<uint32_t> want_buckets(tiles), got_buckets(tiles, 0u);
    for (int i = 0; i < tiles; i++) want_buckets[i] = std::min(len[i] >> 2, 2047u);
    std::sort(want_buckets.begin(), want_buckets.end(), [](uint32_t a, uint32_t b) { return a > b; });
    for (int i = 0; i < tiles; i++) {
        if (order[i] >= (uint32_t)tiles || seen[order[i]]) { bad("order is not a permutation of the tiles", i, order[i], 0); break; }
        seen[order[i]] = 1;
        got_buckets[i] = std::min(len[order[i]] >> 2, 2047u);
    }
    if (!g_bad)
        for (int i = 0; i < tiles; i++)
            if (got_buckets[i] != want_buckets[i]) { bad("bucket along the order (descending)", i, got_buckets[i], want_buckets[i]); break; }
    expect("zero_word", d_word, backward_form ? std::vector<uint32_t>{0u} : std::vector<uint32_t>{});
    end_case();
}
static void group_tile_order() {
    uint64_t seed = 1201;
    for (int tiles : {1, 2047, 2048, 2049, 7500, 8191, 8192, 8193, 20000})
        for (int lengths : {0, 1, 2})
            for (bool bwd : {false, true}) case_tile_order(tiles, lengths, bwd, seed++);
}

int main(int argc, char** argv) {
    const char* only = argc > 1 ? argv[1] : "";
    HIP_OK(hipSetDevice(0));
    HIP_OK(hipStreamCreate(&g_s));
    struct Group { const char* name; void (*run)(); };
    const Group groups[] = {{"scan", group_scan}, {"emit", group_emit}, {"tile_order", group_tile_order}};
    for (const Group& g : groups) {
        if (!strstr(g.name, only)) continue;
        const int before = g_failed, cases_before = g_cases;
        g.run();
        printf("group %-10s %3d cases, %d failed\n", g.name, g_cases - cases_before, g_failed - before);
        fflush(stdout);
    }
    HIP_OK(hipStreamDestroy(g_s));
    printf("%d cases, %d failed\n", g_cases, g_failed);
    if (g_failed || g_cases == 0) { printf("preblend_edges FAILED (%d)\n", g_failed); return 1; }
    printf("preblend_edges OK\n");
    return 0;
}
