// The rasterizer's extern "C" entry points (include/g4s_rasterizer.h) with the host-side sequencing of its kernels --
// mirrors Rasterizer::forward / ::backward (dsr/cuda_rasterizer/rasterizer_impl.cu:198-448) -- and what every unit of
// libg4s_hip.so shares (g4s_internal.h): the error path, the options, the per-kernel profiling, g4s_version.  Every
// other entry point sits beside its kernels.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "g4s_internal.h"

using namespace g4s;

namespace {
thread_local char t_err[512] = "";  // behind g4s_last_error(); written here only
}

// the library's error path (declared in g4s_internal.h)
namespace g4s {
void clear_error() { t_err[0] = 0; }
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t_err, sizeof(t_err), fmt, ap);
    va_end(ap);
    return code;
}
int finish(hipError_t e, const char* what) {
    if (e == hipSuccess) e = hipGetLastError();
    return e == hipSuccess ? G4S_OK : fail(G4S_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
}  // namespace g4s

namespace {

// One pinned, device-mapped word block per host thread for the read-back of the instance counts: the totals kernel
// stores them straight into host memory (no copy launch between it and the event the host waits on).
// hipHostMallocPortable: the same host thread may drive several devices (one process, eight GPUs), and only a portable
// allocation is pinned / mapped for all of them.
uint32_t* pinned_word() {
    thread_local uint32_t* p = nullptr;
    if (!p) {
        if (hipHostMalloc((void**)&p, 64, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) p = nullptr;
    }
    return p;
}
// its address as the current device sees it
uint32_t* pinned_word_device(uint32_t* host) {
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, host, 0) != hipSuccess) return nullptr;
    return (uint32_t*)d;
}

// One event per host thread and device, recorded behind the read-back copy: the forward waits on it instead of on
// the whole stream, so work queued after the copy keeps the GPU busy while the host reads the totals.
hipEvent_t readback_event() {
    thread_local hipEvent_t ev[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    if (!ev[dev]) {
        if (hipEventCreateWithFlags(&ev[dev], hipEventDisableTiming) != hipSuccess) ev[dev] = nullptr;
    }
    return ev[dev];
}

// Diagnostic switches (include/g4s_rasterizer.h: g4s_set_option).  Plain process-wide integers: read on every call,
// written only by g4s_set_option -- the call paths never touch the environment.
struct Option { const char* name; std::atomic<int> value; };
Option g_options[] = {{"box_only", {0}}, {"no_fastpath", {0}}, {"bwd_fwd_order", {0}},
                      {"bwd_hot_threshold", {G4S_OPTION_UNSET}}, {"no_side_zero", {0}}};
enum OptionId { OPT_BOX_ONLY, OPT_NO_FASTPATH, OPT_BWD_FWD_ORDER, OPT_BWD_HOT_THRESHOLD, OPT_NO_SIDE_ZERO };
inline int opt(OptionId id) { return g_options[id].value.load(std::memory_order_relaxed); }

inline bool trace_on() {
    static const bool on = getenv("G4S_TRACE") != nullptr;
    return on;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return fail(G4S_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

#define CHECK_LAUNCH(what) do { if (int _rc = stage_done(what, stream, debug)) return _rc; } while (0)

// ---- optional per-kernel timing with HIP events on the launch stream (bench.py roofline) ----
const char* const kProfNames[PF_COUNT] = {"preprocess_fwd", "depth_sort", "count_scan", "emit", "tile_sort",
                                          "tile_ranges",    "blend_fwd",  "blend_bwd",  "preprocess_bwd",
                                          "maps_fwd",       "maps_bwd",   "photometric_loss",
                                          "adam", "geometry_regularizers", "chart_prior"};
struct ProfRec { int id; hipEvent_t a, b; };
std::mutex g_prof_mu;
bool g_prof_on = false;
std::vector<ProfRec> g_prof;          // recorded (kernel group, start, stop)
std::vector<hipEvent_t> g_prof_pool;  // events are created up front, never inside a timed region
size_t g_prof_next = 0;
constexpr size_t PROF_POOL = 16384;

// Bits of the tile field the partition sorts on: the reference's getHigherMsb(tiles) (rasterizer_impl.cu:301), capped
// at the 32 bits the field has.
uint32_t higher_msb(uint32_t n) {  // rasterizer_impl.cu:35-50
    uint32_t msb = sizeof(n) * 4, step = msb;
    while (step > 1) {
        step /= 2;
        if (n >> msb) msb += step; else msb -= step;
    }
    if (n >> msb) msb++;
    return msb;
}
int tile_sort_bits(int tiles) {
    const int b = (int)higher_msb((uint32_t)tiles);
    return b < 32 ? b : 32;
}

// What a frame size fixes, derived in this one place for g4s_rasterizer_layout, the forward and the backward: the tile
// partition ping-pongs between the two halves of the binning chunk, and its (data-independent) pass count says which
// half the backward finds the sorted entries in.
struct FrameGeom { int tiles_x, tiles_y, tiles, tile_bits, passes; bool entries_in_b; };
FrameGeom frame_geom(int width, int height) {
    FrameGeom f{};
    f.tiles_x = (width + TILE - 1) / TILE; f.tiles_y = (height + TILE - 1) / TILE;
    f.tiles = (int)((uint32_t)f.tiles_x * (uint32_t)f.tiles_y);  // (the forward refuses frames where this wraps)
    f.tile_bits = tile_sort_bits(f.tiles); f.passes = (f.tile_bits + 7) / 8;  // rasterizer_impl.cu:301
    f.entries_in_b = (f.passes & 1) != 0;
    return f;
}

// The arguments of the rasterizer's entry points as named fields: each extern "C" function below fills one by name
// (`c.scales = scales`), so that two of its many float pointers cannot change places unseen on the way to the kernels.
struct ForwardCall {
    // capacity >= 0: the presized, host-synchronisation-free form -- the binning chunk holds `capacity` instances, the
    // instance counts stay on the device (status_dev), nothing is read back.
    int capacity = -1; uint32_t* status_dev;
    struct Chunk { g4s_resize_fn resize; void* ctx; } geometry, binning, image;  // the three scratch callbacks
    int P, D, M, width, height, prefiltered, debug; float scale_modifier, tan_fovx, tan_fovy;
    // shs_rest == NULL: shs is the packed [P,M,3] tensor; otherwise shs = [P,1,3] and shs_rest = [P,M-1,3].
    const float *background, *means3D, *shs, *shs_rest, *colors_precomp, *opacities, *scales, *rotations,
        *transMat_precomp, *viewmatrix, *projmatrix, *cam_pos;
    float *out_color, *out_others; int* radii; void* stream;
};
struct BackwardCall {
    int P, D, M, R, width, height, debug; float scale_modifier, tan_fovx, tan_fovy;
    const float *background, *means3D, *shs, *shs_rest, *colors_precomp, *scales, *rotations, *transMat_precomp,
        *viewmatrix, *projmatrix, *campos, *dL_dpix, *dL_depths;
    const int* radii; char *geom_buffer, *binning_buffer, *image_buffer, *workspace; size_t workspace_bytes;
    float *dL_dmean2D, *dL_dnormal, *dL_dopacity, *dL_dcolor, *dL_dmean3D, *dL_dtransMat, *dL_dsh, *dL_dsh_rest,
        *dL_dscale, *dL_drot;
    // gradient accumulation over views (g4s_rasterizer_backward_accumulate_packed); unset in the other two backwards
    bool accumulate; void* after_event; float* view_stats; const g4s_packed_rows* packed; void* stream;
};
// Declare `c` and fill it with the parameters that the forward / the backward entry points have in common, by the names
// they carry in include/g4s_rasterizer.h; what differs (the SH arguments, the scratch, the extensions) is set beside it.
#define DECLARE_FORWARD_CALL(c)                                                                                       \
    ForwardCall c{}; c.P = P; c.D = D; c.M = M; c.background = background; c.width = width; c.height = height; c.means3D = means3D;    \
    c.opacities = opacities; c.scales = scales; c.scale_modifier = scale_modifier; c.rotations = rotations;           \
    c.transMat_precomp = transMat_precomp; c.viewmatrix = viewmatrix; c.projmatrix = projmatrix; c.cam_pos = cam_pos;  \
    c.tan_fovx = tan_fovx; c.tan_fovy = tan_fovy; c.out_color = out_color; c.out_others = out_others;                 \
    c.radii = radii; c.debug = debug; c.stream = stream
#define DECLARE_BACKWARD_CALL(c)                                                                                      \
    BackwardCall c{}; c.P = P; c.D = D; c.M = M; c.R = R; c.background = background; c.width = width; c.height = height;                \
    c.means3D = means3D; c.scales = scales; c.scale_modifier = scale_modifier; c.rotations = rotations;               \
    c.transMat_precomp = transMat_precomp; c.viewmatrix = viewmatrix; c.projmatrix = projmatrix; c.campos = campos;   \
    c.tan_fovx = tan_fovx; c.tan_fovy = tan_fovy; c.radii = radii; c.geom_buffer = geom_buffer;                       \
    c.binning_buffer = binning_buffer; c.image_buffer = image_buffer; c.dL_dpix = dL_dpix; c.dL_depths = dL_depths;   \
    c.dL_dmean2D = dL_dmean2D; c.dL_dnormal = dL_dnormal; c.dL_dopacity = dL_dopacity; c.dL_dcolor = dL_dcolor;       \
    c.dL_dmean3D = dL_dmean3D; c.dL_dtransMat = dL_dtransMat; c.dL_dscale = dL_dscale; c.dL_drot = dL_drot;           \
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.debug = debug; c.stream = stream

}  // namespace

namespace g4s {
// CHECK_CUDA of the reference (auxiliary.h:295-302): launch errors always, sync + check in debug.
// G4S_TRACE=1 in the environment: synchronise after every stage and log it to stderr.
int stage_done(const char* what, hipStream_t s, bool debug) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && (debug || trace_on())) e = hipStreamSynchronize(s);
    if (trace_on()) { fprintf(stderr, "[g4s] %s: %s\n", what, hipGetErrorString(e)); fflush(stderr); }
    return e == hipSuccess ? G4S_OK : fail(G4S_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
ProfScope::ProfScope(int id_, hipStream_t s_) : id(id_), s(s_) {
    if (!g_prof_on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (g_prof_next + 2 > g_prof_pool.size()) return;  // pool exhausted: stop recording
    a = g_prof_pool[g_prof_next++];
    b = g_prof_pool[g_prof_next++];
    on = hipEventRecord(a, s) == hipSuccess;
}
ProfScope::~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(b, s);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof.push_back(ProfRec{id, a, b});
}
}  // namespace g4s

extern "C" const char* g4s_last_error(void) { return t_err; }

extern "C" void g4s_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (on && g_prof_pool.empty()) {
        g_prof_pool.reserve(PROF_POOL);
        for (size_t i = 0; i < PROF_POOL; i++) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) break;
            g_prof_pool.push_back(e);
        }
    }
    g_prof_on = on != 0;
}
extern "C" int g4s_profile_kernels(void) { return PF_COUNT; }
extern "C" const char* g4s_profile_name(int id) { return (id >= 0 && id < PF_COUNT) ? kProfNames[id] : ""; }
// Sum of the recorded durations of kernel group `id` (ms) and the number of recordings.
// Synchronises on the recorded events.  g4s_profile_reset() drops all recordings.
extern "C" int g4s_profile_read(int id, double* total_ms, int* count) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    double tot = 0; int n = 0;
    for (const ProfRec& r : g_prof) {
        if (r.id != id) continue;
        if (hipEventSynchronize(r.b) != hipSuccess) return G4S_ERR_HIP;
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) return G4S_ERR_HIP;
        tot += ms; n++;
    }
    if (total_ms) *total_ms = tot;
    if (count) *count = n;
    return G4S_OK;
}
extern "C" void g4s_profile_reset(void) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof.clear();
    g_prof_next = 0;  // the pooled events are reused
}
extern "C" int g4s_set_option(const char* name, int value) {
    for (Option& o : g_options)
        if (name && !strcmp(name, o.name)) { o.value.store(value, std::memory_order_relaxed); return G4S_OK; }
    return fail(G4S_ERR_INVALID_ARGUMENT, "unknown option '%s'", name ? name : "(null)");
}
extern "C" int g4s_get_option(const char* name, int* value) {
    for (Option& o : g_options)
        if (name && !strcmp(name, o.name)) { if (value) *value = o.value.load(std::memory_order_relaxed); return G4S_OK; }
    return fail(G4S_ERR_INVALID_ARGUMENT, "unknown option '%s'", name ? name : "(null)");
}
#ifndef G4S_BUILD_ID
#define G4S_BUILD_ID "unknown"
#endif
// "... build <id>": the id is the digest of the library's sources (csrc/Makefile)
extern "C" const char* g4s_version(void) { return "g4s-hip 0.1.0 gfx950 build " G4S_BUILD_ID; }

extern "C" int g4s_rasterizer_layout(int P, int R, int width, int height, g4s_layout* out) {
    if (!out || P < 0 || R < 0 || width <= 0 || height <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "bad layout query");
    const FrameGeom f = frame_geom(width, height);
    const GeomLayout g = geom_layout((size_t)P);
    const BinLayout b = bin_layout((size_t)R);
    const ImgLayout im = img_layout((size_t)width * height, (size_t)f.tiles);
    out->rec = g.rec;
    out->clamped = g.clamped;
    out->depth_sorted = g.vals_b;  // wherever the sort starts and however many passes it takes (g4s_rasterizer_forward)
    out->tiles_touched = g.tiles_touched;
    out->geom_bytes = g.bytes;
    out->entries = f.entries_in_b ? b.ent_b : b.ent_a;
    out->qhit = b.qhit;
    out->binning_bytes = b.bytes;
    out->ranges = im.ranges;
    out->final_T = im.final_T;
    out->n_contrib = im.n_contrib;
    out->tile_order = im.tile_order;
    out->image_bytes = im.bytes;
    out->hot_count = im.hot_count;
    return G4S_OK;
}

// Fixed buffers as "resize callbacks" (g4s_rasterizer_forward_presized): the callback hands the caller's chunk out
// if it is large enough.
struct FixedChunk { char* ptr; size_t bytes; };
char* fixed_chunk_cb(void* ctx, size_t n) {
    FixedChunk* c = (FixedChunk*)ctx;
    return n <= c->bytes ? c->ptr : nullptr;
}

static int rasterizer_forward_impl(const ForwardCall& c) {
    hipStream_t stream = (hipStream_t)c.stream;
    const int P = c.P, debug = c.debug;
    t_err[0] = 0;
    if (P < 0 || c.width <= 0 || c.height <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "P, width, height must be positive");
    if (!c.geometry.resize || !c.binning.resize || !c.image.resize)
        return fail(G4S_ERR_INVALID_ARGUMENT, "resize callbacks must not be NULL");
    if (!c.background || !c.viewmatrix || !c.projmatrix || !c.cam_pos || !c.out_color || !c.out_others)
        return fail(G4S_ERR_INVALID_ARGUMENT, "NULL required pointer");
    const FrameGeom FG = frame_geom(c.width, c.height);
    const int tiles_x = FG.tiles_x, tiles_y = FG.tiles_y, tiles = FG.tiles;
    // (tile coordinates travel in 16 bits each -- the binned rect of a Gaussian -- and the tile id in 32)
    if (tiles_x > 65535 || tiles_y > 32767 || (long long)tiles_x * tiles_y > 0x7FFFFFFFll)
        return fail(G4S_ERR_INVALID_ARGUMENT, "image too large: %d x %d tiles (at most 65535 across, 32767 down)", tiles_x, tiles_y);

    // image chunk first: with P == 0 the frame is still background (rasterize_points.cu:85-99
    // returns zero-filled outputs in that case; the binding handles P == 0 itself)
    const ImgLayout IL = img_layout((size_t)c.width * c.height, (size_t)tiles);
    char* img = c.image.resize(c.image.ctx, IL.bytes);
    if (!img) return fail(G4S_ERR_ALLOC, "image buffer callback returned NULL");
    img = align_ptr(img);
    uint32_t* ranges = (uint32_t*)(img + IL.ranges);
    float* final_T = (float*)(img + IL.final_T);
    uint32_t* n_contrib = (uint32_t*)(img + IL.n_contrib);
    if (P <= 0) HIP_TRY(hipMemsetAsync(ranges, 0, (size_t)tiles * 8, stream));  // rasterizer_impl.cu:311 (P > 0: cleared by the preprocess)
    const bool presized = c.capacity >= 0;
    if (presized && c.status_dev && P <= 0) HIP_TRY(hipMemsetAsync(c.status_dev, 0, 16, stream));

    int R = 0;
    const float* rec_ptr = nullptr;
    const uint64_t* entries_ptr = nullptr;
    uint8_t* qhit_ptr = nullptr;
    if (P > 0) {
        if (!c.means3D || !c.opacities) return fail(G4S_ERR_INVALID_ARGUMENT, "means3D / opacities must not be NULL");
        if (!c.shs && !c.colors_precomp)  // NUM_CHANNELS == 3 here; mirrors rasterizer_impl.cu:243-246
            return fail(G4S_ERR_UNSUPPORTED, "provide SHs or precomputed colours");
        if (!c.transMat_precomp && (!c.scales || !c.rotations))
            return fail(G4S_ERR_INVALID_ARGUMENT, "provide scales+rotations or transMat_precomp");
        if (misaligned(c.rotations, 16) || misaligned(c.scales, 8))
            return fail(G4S_ERR_INVALID_ARGUMENT, "rotations must be 16-byte and scales 8-byte aligned");
        if (c.shs && (c.D < 0 || c.D > 3 || (c.D + 1) * (c.D + 1) > c.M))
            return fail(G4S_ERR_INVALID_ARGUMENT, "SH degree %d does not fit M = %d coefficients", c.D, c.M);

        const GeomLayout GL = geom_layout((size_t)P);
        char* geom = c.geometry.resize(c.geometry.ctx, GL.bytes);
        if (!geom) return fail(G4S_ERR_ALLOC, "geometry buffer callback returned NULL");
        geom = align_ptr(geom);
        float* rec = (float*)(geom + GL.rec);
        uint32_t* tiles_touched = (uint32_t*)(geom + GL.tiles_touched);
        uint32_t* keys_a = (uint32_t*)(geom + GL.keys_a);
        uint32_t* keys_b = (uint32_t*)(geom + GL.keys_b);
        uint32_t* vals_a = (uint32_t*)(geom + GL.vals_a);
        uint32_t* vals_b = (uint32_t*)(geom + GL.vals_b);
        uint32_t* block_sums = (uint32_t*)(geom + GL.block_sums);
        uint32_t* block_offs = (uint32_t*)(geom + GL.block_offs);
        uint32_t* d_total = (uint32_t*)(geom + GL.total);
        int* const radii = c.radii ? c.radii : (int*)(geom + GL.internal_radii);  // rasterizer_impl.cu:230-233

        PreprocessArgs pa{};
        pa.P = P; pa.D = c.D; pa.M = c.M; pa.W = c.width; pa.H = c.height; pa.tiles_x = tiles_x; pa.tiles_y = tiles_y;
        pa.means3D = c.means3D; pa.scales = c.scales; pa.rotations = c.rotations; pa.opacities = c.opacities; pa.shs = c.shs;
        pa.transMat_precomp = c.transMat_precomp; pa.colors_precomp = c.colors_precomp;
        pa.viewmatrix = c.viewmatrix; pa.projmatrix = c.projmatrix; pa.cam_pos = c.cam_pos;
        pa.scale_modifier = c.scale_modifier;
        pa.shs_rest = c.shs_rest;
        pa.sh_vec16 = (c.shs != nullptr && c.shs_rest == nullptr && c.M == 16 && !misaligned(c.shs, 16));
        pa.no_fastpath = opt(OPT_NO_FASTPATH) != 0;
        pa.rec = rec; pa.clamped = (uint8_t*)(geom + GL.clamped); pa.tiles_touched = tiles_touched; pa.radii = radii;
        pa.tight_rect = (uint2*)(geom + GL.tight_rect);
        // The depth sort ping-pongs between the a and the b arrays and its result is to land in vals_b whatever the
        // number of passes (g4s_rasterizer_layout().depth_sorted): three passes (the regular forward) start in the a
        // arrays, four (presized) in the b arrays; the preprocess writes the unpacked keys into the other key array.
        uint32_t* const k_first = presized ? keys_b : keys_a;
        uint32_t* const k_other = presized ? keys_a : keys_b;
        uint32_t* const v_first = presized ? vals_b : vals_a;
        uint32_t* const v_other = presized ? vals_a : vals_b;
        pa.depth_keys = k_other;
        pa.ref_block_sums = (uint32_t*)(geom + GL.ref_block_sums);
        pa.idx_block_sums = (uint32_t*)(geom + GL.idx_block_sums);
        pa.vis_block_sums = (uint32_t*)(geom + GL.vis_block_sums);
        pa.key_min_blocks = (uint32_t*)(geom + GL.key_min_blocks);
        pa.key_max_blocks = (uint32_t*)(geom + GL.key_max_blocks);
        pa.zero_ptr = ranges; pa.zero_words = (uint32_t)tiles * 2u;  // rasterizer_impl.cu:311
        { ProfScope ps(PF_PREPROCESS_FWD, stream); launch_preprocess_fwd(pa, stream); }
        CHECK_LAUNCH("preprocess_fwd");

        // Everything the host has to know comes out of the preprocess' per-block partial sums: the one host
        // synchronisation of the forward (rasterizer_impl.cu:281-282) sits right behind it, and every later launch
        // is sized for the Gaussians that actually emit instances.
        uint32_t* idx_block_offs = (uint32_t*)(geom + GL.idx_block_offs);
        uint32_t* vis_block_offs = (uint32_t*)(geom + GL.vis_block_offs);
        uint32_t* h_total = nullptr;
        uint32_t* h_total_dev = nullptr;
        hipEvent_t totals_ready = nullptr;
        if (!presized) {
            h_total = pinned_word();
            h_total_dev = h_total ? pinned_word_device(h_total) : nullptr;
            if (!h_total || !h_total_dev) return fail(G4S_ERR_HIP, "hipHostMalloc / hipHostGetDevicePointer failed");
            totals_ready = readback_event();
            if (!totals_ready) return fail(G4S_ERR_HIP, "hipEventCreate failed");
        }
        { ProfScope ps(PF_COUNT_SCAN, stream);
          launch_scan_totals(pa.idx_block_sums, idx_block_offs, pa.ref_block_sums, pa.vis_block_sums, vis_block_offs,
                             d_total, GL.nblocks, nullptr, 0, stream, presized ? (uint32_t)c.capacity : 0xFFFFFFFFu,
                             h_total_dev, presized ? c.status_dev : nullptr, pa.key_min_blocks, pa.key_max_blocks); }
        CHECK_LAUNCH("scan totals");
        if (!presized) {
            HIP_TRY(hipEventRecord(totals_ready, stream));  // (the kernel above stored the three counts in host memory)
        }
        // (presized: the kernel wrote status_dev[0..3] = num_rendered, instances binned, emitting Gaussians, overflow flag)

        // Queued BEFORE the host waits for the totals: nothing below needs them on the host -- the gradient slots do
        // not depend on them, and the pack / depth sort / count of the emitting Gaussians read V (d_total[2]) on the
        // device, their launches sized for P.  The GPU therefore has ~0.1 ms of work queued while the host reads the
        // totals back, sizes the binning chunk and issues the rest: the read-back no longer drains the queue.
        const uint32_t* d_V = d_total + 2;
        const uint32_t* d_key_min = d_total + 5;  // smallest depth key of the frame (the totals scan)
        uint32_t* sort_hist = (uint32_t*)(geom + GL.hist);
        uint32_t* sort_bins = (uint32_t*)(geom + GL.bin_total);
        int cur;
        {   // depth order of the emitting Gaussians (stable => ties by ascending index): pack, then sort
            ProfScope ps(PF_DEPTH_SORT, stream);
            launch_slots_and_compact(P, tiles_touched, idx_block_offs, rec, k_other, vis_block_offs, k_first, v_first,
                                     GL.nblocks, stream);
            // three passes over the low 27 bits of (key - smallest key): the whole sort unless the frame's depths span a
            // ratio of 2^16 or more, which the host learns with the totals below.  Presized (no read-back): four passes.
            cur = presized ? radix_sort_u32_pairs(k_first, k_other, v_first, v_other, P, sort_hist, sort_bins, stream, d_V)
                           : radix_sort_depth_low(k_first, k_other, v_first, v_other, P, sort_hist, sort_bins, stream, d_V,
                                                  d_key_min);
        }
        CHECK_LAUNCH("depth sort");

        int R_binned, V_emit, nblocks_v;
        const uint32_t* d_counts = nullptr;   // presized: (V, min(binned, capacity)) on the device
        const uint32_t* d_nbinned = nullptr;
        if (!presized) {
            // the one host wait of the forward (rasterizer_impl.cu:281-282), on the read-back only
            HIP_TRY(hipEventSynchronize(totals_ready));
            // h_total[0]: instances actually binned (3-sigma rect intersected with the alpha-cutoff box),
            // h_total[1]: the reference's count (3-sigma rect only) = the num_rendered this call returns,
            // h_total[2]: Gaussians that emit at least one instance.
            // All buffers are laid out for the reference count, which bounds the binned one.
            if (h_total[1] > 0x7FFFFFFFu) return fail(G4S_ERR_INVALID_ARGUMENT, "num_rendered overflows int");
            R = (int)h_total[1];
            R_binned = (int)h_total[0];
            V_emit = (int)h_total[2];
            nblocks_v = (V_emit + 255) / 256;
            if (V_emit > 0 && ((uint64_t)h_total[4] - h_total[3]) >> DEPTH_SORT_LOW_BITS) {  // a frame that deep: the bits above
                ProfScope ps(PF_DEPTH_SORT, stream);
                cur = radix_sort_depth_top(k_first, k_other, v_first, v_other, P, cur, sort_hist, sort_bins, stream, d_V,
                                           d_key_min);
                CHECK_LAUNCH("depth sort, upper bits");
                // (a fourth pass: the order is in vals_a now -- back to where everything else expects it)
                HIP_TRY(hipMemcpyAsync(vals_b, vals_a, (size_t)V_emit * 4, hipMemcpyDeviceToDevice, stream));
            }
        } else {
            // no read-back: every launch below is sized for the capacity and reads the counts on the device
            R = c.capacity;  // what the layouts (here and in the backward) are computed from
            R_binned = c.capacity;
            V_emit = P;
            nblocks_v = GL.nblocks;
            d_counts = d_total + 2;
            d_nbinned = d_total + 3;
        }

        (void)cur;
        const uint32_t* gidx_sorted = vals_b;
        uint32_t* rank_local = keys_a;  // (neither key array is needed after the sort)
        {
            ProfScope ps(PF_COUNT_SCAN, stream);
            launch_count_scan(P, gidx_sorted, tiles_touched, block_sums, block_offs, rank_local, d_total + 8, GL.nblocks,
                              stream, d_V);
        }
        CHECK_LAUNCH("count scan");

        const BinLayout BL = bin_layout((size_t)R);
        char* bin = c.binning.resize(c.binning.ctx, BL.bytes);
        if (!bin) return fail(G4S_ERR_ALLOC, presized ? "binning buffer smaller than g4s_rasterizer_layout(P, capacity).binning_bytes"
                                                      : "binning buffer callback returned NULL");
        bin = align_ptr(bin);
        uint64_t* ent_a = (uint64_t*)(bin + BL.ent_a);
        uint64_t* ent_b = (uint64_t*)(bin + BL.ent_b);
        entries_ptr = ent_a;
        qhit_ptr = (uint8_t*)(bin + BL.qhit);
        if (R_binned > 0) {
            { ProfScope ps(PF_EMIT, stream);  // (also clears the contribution masks qhit[0, R_binned))
              launch_emit(V_emit, (uint32_t)R_binned, tiles_x, gidx_sorted, block_offs, nblocks_v, rank_local,
                          (const uint2*)(geom + GL.tight_rect), ent_a, qhit_ptr, (uint8_t*)(bin + BL.rec_flag), stream,
                          d_counts); }
            CHECK_LAUNCH("emit");
            int half;
            { ProfScope ps(PF_TILE_SORT, stream);
              half = radix_sort_u64_keys(ent_a, ent_b, R_binned, ENTRY_TILE_SHIFT, ENTRY_TILE_SHIFT + FG.tile_bits,
                                         (uint32_t*)(bin + BL.hist), (uint32_t*)(bin + BL.bin_total), stream, d_nbinned); }
            CHECK_LAUNCH("tile partition");
            if ((half != 0) != FG.entries_in_b) return fail(G4S_ERR_HIP, "tile partition ended in the other half than frame_geom says");
            entries_ptr = FG.entries_in_b ? ent_b : ent_a;
            { ProfScope ps(PF_TILE_RANGES, stream); launch_tile_ranges(R_binned, entries_ptr, ranges, stream, d_nbinned); }
            CHECK_LAUNCH("tile ranges");
        }
        rec_ptr = rec;
    } else {
        // keep the callback protocol: zero-sized chunks are still requested
        (void)c.geometry.resize(c.geometry.ctx, 0);
        (void)c.binning.resize(c.binning.ctx, 0);
    }

    uint32_t* tile_order = (uint32_t*)(img + IL.tile_order);
    launch_tile_order(tiles, ranges, tile_order, stream);
    CHECK_LAUNCH("tile order");
    BlendFwdArgs ba{};
    ba.W = c.width; ba.H = c.height; ba.tiles_x = tiles_x; ba.tiles_y = tiles_y;
    ba.tile_depth = (uint32_t*)(img + IL.tile_depth);
    ba.ranges = ranges; ba.tile_order = tile_order; ba.entries = entries_ptr; ba.rec = rec_ptr; ba.bg = c.background;
    ba.final_T = final_T; ba.n_contrib = n_contrib; ba.out_color = c.out_color; ba.out_others = c.out_others;
    ba.qhit = qhit_ptr;
    ba.box_only = opt(OPT_BOX_ONLY) != 0;
    { ProfScope ps(PF_BLEND_FWD, stream); launch_blend_fwd(ba, stream); }
    CHECK_LAUNCH("blend_fwd");
    return R;
}

extern "C" int g4s_rasterizer_forward(
    g4s_resize_fn geometry_buffer, void* geometry_ctx, g4s_resize_fn binning_buffer, void* binning_ctx,
    g4s_resize_fn image_buffer, void* image_ctx, int P, int D, int M, const float* background, int width, int height,
    const float* means3D, const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
    float scale_modifier, const float* rotations, const float* transMat_precomp, const float* viewmatrix,
    const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color,
    float* out_others, int* radii, int debug, void* stream) {
    DECLARE_FORWARD_CALL(c);
    c.geometry = {geometry_buffer, geometry_ctx}; c.binning = {binning_buffer, binning_ctx}; c.image = {image_buffer, image_ctx};
    c.prefiltered = prefiltered;
    c.shs = shs; c.colors_precomp = colors_precomp;
    return rasterizer_forward_impl(c);
}

extern "C" int g4s_rasterizer_forward_split_sh(
    g4s_resize_fn geometry_buffer, void* geometry_ctx, g4s_resize_fn binning_buffer, void* binning_ctx,
    g4s_resize_fn image_buffer, void* image_ctx, int P, int D, int M, const float* background, int width, int height,
    const float* means3D, const float* sh_dc, const float* sh_rest, const float* opacities, const float* scales,
    float scale_modifier, const float* rotations, const float* transMat_precomp, const float* viewmatrix,
    const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color,
    float* out_others, int* radii, int debug, void* stream) {
    t_err[0] = 0;
    if (P > 0 && (!sh_dc || M < 1 || (M > 1 && !sh_rest)))
        return fail(G4S_ERR_INVALID_ARGUMENT, "split SH needs sh_dc [P,1,3] and, for M > 1, sh_rest [P,M-1,3]");
    DECLARE_FORWARD_CALL(c);
    c.geometry = {geometry_buffer, geometry_ctx}; c.binning = {binning_buffer, binning_ctx}; c.image = {image_buffer, image_ctx};
    c.prefiltered = prefiltered;
    // M == 1: there is no rest tensor; the packed layout [P,1,3] is the same memory
    c.shs = sh_dc; c.shs_rest = M > 1 ? sh_rest : nullptr;
    return rasterizer_forward_impl(c);
}

// The forward without its host synchronisation (include/g4s_rasterizer.h).  sh_rest == NULL: packed SH.
extern "C" int g4s_rasterizer_forward_presized(
    char* geom_buffer, size_t geom_bytes, char* binning_buffer, size_t binning_bytes, char* image_buffer, size_t image_bytes,
    int instance_capacity, uint32_t* status_dev, int P, int D, int M, const float* background, int width, int height,
    const float* means3D, const float* shs, const float* sh_rest, const float* colors_precomp, const float* opacities,
    const float* scales, float scale_modifier, const float* rotations, const float* transMat_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
    float* out_color, float* out_others, int* radii, int debug, void* stream) {
    t_err[0] = 0;
    if (instance_capacity < 0 || !status_dev) return fail(G4S_ERR_INVALID_ARGUMENT, "capacity must be >= 0 and status_dev non-NULL");
    if (!geom_buffer || !binning_buffer || !image_buffer) return fail(G4S_ERR_INVALID_ARGUMENT, "state buffers must not be NULL");
    FixedChunk g{geom_buffer, geom_bytes}, b{binning_buffer, binning_bytes}, im{image_buffer, image_bytes};
    DECLARE_FORWARD_CALL(c);
    c.capacity = instance_capacity; c.status_dev = status_dev;
    c.geometry = {fixed_chunk_cb, &g}; c.binning = {fixed_chunk_cb, &b}; c.image = {fixed_chunk_cb, &im};
    c.shs = shs; c.shs_rest = M > 1 ? sh_rest : nullptr; c.colors_precomp = colors_precomp;
    const int rc = rasterizer_forward_impl(c);
    return rc < 0 ? rc : G4S_OK;  // (the impl returns the capacity as "R"; the real count is status_dev[0])
}

extern "C" size_t g4s_rasterizer_backward_workspace(int P, int R) {
    // gradient records   (their validity bytes live in the forward's binning chunk, the deep-tile list in its image chunk)
    (void)P;
    return align_up((size_t)(R > 0 ? R : 1) * GRAD_STRIDE * 4) + 256;
}

static int rasterizer_backward_impl(const BackwardCall& c) {
    hipStream_t stream = (hipStream_t)c.stream;
    const int P = c.P, M = c.M, R = c.R, debug = c.debug;
    t_err[0] = 0;
    if (P < 0 || R < 0 || c.width <= 0 || c.height <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "bad sizes");
    if (P == 0) return G4S_OK;  // rasterize_points.cu:197: nothing to do, outputs are [0,*]
    if (!c.geom_buffer || !c.image_buffer || (R > 0 && !c.binning_buffer))
        return fail(G4S_ERR_INVALID_ARGUMENT, "state buffers must not be NULL");
    if (!c.dL_dpix || !c.dL_depths || !c.dL_dmean2D || !c.dL_dopacity || !c.dL_dcolor || !c.dL_dmean3D ||
        !c.dL_dscale || !c.dL_drot || (M > 0 && !c.dL_dsh) || (c.shs_rest && M > 1 && !c.dL_dsh_rest))
        return fail(G4S_ERR_INVALID_ARGUMENT, "NULL gradient pointer");
    if (c.workspace_bytes < g4s_rasterizer_backward_workspace(P, R) || !c.workspace)
        return fail(G4S_ERR_INVALID_ARGUMENT, "workspace too small");
    if (misaligned(c.rotations, 16) || misaligned(c.scales, 8) || misaligned(c.dL_drot, 16) || misaligned(c.dL_dscale, 8))
        return fail(G4S_ERR_INVALID_ARGUMENT, "rotations/dL_drot must be 16-byte, scales/dL_dscale 8-byte aligned");

    const FrameGeom FG = frame_geom(c.width, c.height);
    const int tiles = FG.tiles;
    const GeomLayout GL = geom_layout((size_t)P);
    const BinLayout BL = bin_layout((size_t)R);
    const ImgLayout IL = img_layout((size_t)c.width * c.height, (size_t)tiles);
    char* geom = align_ptr(c.geom_buffer);
    char* img = align_ptr(c.image_buffer);
    const float* rec = (const float*)(geom + GL.rec);
    const int* const radii = c.radii ? c.radii : (const int*)(geom + GL.internal_radii);
    float* grad_inst = (float*)align_ptr(c.workspace);

    // gradient records: only instances that receive a contribution are written by the blend backward; instead of
    // clearing 80 B per instance, one validity byte per instance is cleared and the fold selects on it
    // the deep-tile counter + list sit in the image chunk; the counter is cleared by the tile-order kernel below
    uint32_t* hot_count = (uint32_t*)(img + IL.hot_count);
    uint32_t* hot_list = (uint32_t*)(img + IL.hot_list);
    // One validity byte per record slot says which records the blend backward wrote; the bytes live in the binning chunk
    // and were cleared by the forward (emit).  A second backward over the same forward state finds them set -- to the
    // values it is going to write again (which records are written depends on the forward's state only).
    uint8_t* rec_flag = nullptr;
    bool sh_prezeroed = false;
    if (R > 0) {
        char* bin = align_ptr(c.binning_buffer);
        rec_flag = (uint8_t*)(bin + BL.rec_flag);
        BlendBwdArgs bb{};
        bb.W = c.width; bb.H = c.height; bb.tiles_x = FG.tiles_x; bb.tiles_y = FG.tiles_y;
        bb.ranges = (const uint32_t*)(img + IL.ranges);
        // backward order: most blended (entry, quadrant) pairs first -- the forward counted them per tile
        uint32_t* tile_order_bwd = (uint32_t*)(img + IL.tile_order_bwd);
        launch_tile_order(tiles, (const uint32_t*)(img + IL.tile_depth), tile_order_bwd, stream, hot_count);
        bb.tile_order = opt(OPT_BWD_FWD_ORDER) ? (const uint32_t*)(img + IL.tile_order) : tile_order_bwd;
        bb.entries = (const uint64_t*)(bin + (FG.entries_in_b ? BL.ent_b : BL.ent_a));
        bb.rec = rec; bb.bg = c.background;
        bb.final_T = (const float*)(img + IL.final_T);
        bb.n_contrib = (const uint32_t*)(img + IL.n_contrib);
        bb.qhit = (const uint8_t*)(bin + BL.qhit);
        bb.dL_dpix = c.dL_dpix; bb.dL_depths = c.dL_depths; bb.grad_inst = grad_inst; bb.rec_flag = rec_flag;
        bb.n_slots = (uint32_t)R;
        // One wave per tile is the efficient form when there are enough tiles to fill the GPU (1 024 SIMDs x 3
        // waves); a small frame (<= 768 tiles, e.g. 256 x 256) runs about twice as fast with four waves per tile,
        // and so does any single tile that is much deeper than the rest (measured: tools/deep_tile_bench.py).
        // In a full-size frame only OUTLIERS are handed over -- tiles at least four times deeper than the average
        // list (and deeper than 2 048): when every tile is deep (3 M surfels at 1200x680) one wave each stays the
        // faster form, the four-wave kernel does ~1.9x the work per tile.
        const long long avg_list = (long long)R / (tiles > 0 ? tiles : 1);
        const long long outlier = 4 * avg_list > BWD_HOT_THRESHOLD ? 4 * avg_list : BWD_HOT_THRESHOLD;
        const int hot_override = opt(OPT_BWD_HOT_THRESHOLD);
        bb.hot_threshold = hot_override != G4S_OPTION_UNSET ? hot_override
                           : (tiles <= BWD_FOUR_WAVE_MAX_TILES ? -1 : (int)(outlier < 0x7fffffff ? outlier : 0x7fffffff));
        bb.hot_count = hot_count; bb.hot_list = hot_list;
        // dL_dsh is mostly zero rows (invisible Gaussians).  When the one-wave kernel runs, its workgroups clear the
        // tensor on the side (blend.hip) and K8 writes the visible rows only; otherwise K8 clears the rows it skips.
        // (accumulating: dL_dsh holds the sum over the previous views -- nothing is cleared anywhere)
        if (bb.hot_threshold >= 0 && M > 0 && !opt(OPT_NO_SIDE_ZERO) && !c.accumulate) {
            float* zb[2] = {c.dL_dsh, c.dL_dsh_rest};
            const size_t zn[2] = {(size_t)P * (c.dL_dsh_rest ? 1 : M) * 3, c.dL_dsh_rest ? (size_t)P * (M - 1) * 3 : 0};
            bool ok = true;
            for (int z = 0; z < 2; z++) ok = ok && (zn[z] == 0 || (!misaligned(zb[z], 16) && (zn[z] >> 2) < 0x80000000ull));  // (the kernel's u32 loop index must not wrap)
            if (ok) {
                for (int z = 0; z < 2; z++) {
                    if (zn[z] == 0) continue;
                    bb.zero_base[z] = zb[z]; bb.zero_quads[z] = (uint32_t)(zn[z] >> 2); bb.zero_tail[z] = (uint32_t)(zn[z] & 3);
                }
                sh_prezeroed = true;
            }
        }
        { ProfScope ps(PF_BLEND_BWD, stream); launch_blend_bwd(bb, stream); }
        CHECK_LAUNCH("blend_bwd");
    }

    // backward.cu:618-619: W,H re-derived through float truncation (may be W-1 / H-1)
    const float focal_y = c.height / (2.0f * c.tan_fovy);
    const float focal_x = c.width / (2.0f * c.tan_fovx);
    PreprocessBwdArgs pb{};
    pb.P = P; pb.D = c.D; pb.M = M;
    pb.W = (int)(focal_x * c.tan_fovx * 2);
    pb.H = (int)(focal_y * c.tan_fovy * 2);
    pb.means3D = c.means3D; pb.scales = c.scales; pb.rotations = c.rotations; pb.shs = c.shs;
    pb.transMat_precomp = c.transMat_precomp; pb.colors_precomp = c.colors_precomp;
    pb.viewmatrix = c.viewmatrix; pb.projmatrix = c.projmatrix; pb.campos = c.campos;
    pb.radii = radii; pb.rec = rec; pb.clamped = (const uint8_t*)(geom + GL.clamped); pb.grad_inst = grad_inst;
    pb.rec_flag = rec_flag; pb.n_slots = (uint32_t)R;
    // the forward's own T (scale_modifier applied, exact W / H) is what the blend kernels' moments refer to
    pb.frame_W = c.width; pb.frame_H = c.height; pb.scale_modifier = c.scale_modifier;
    pb.shs_rest = c.shs_rest; pb.dL_dsh_rest = c.dL_dsh_rest; pb.sh_prezeroed = sh_prezeroed;
    pb.accumulate = c.accumulate;
    pb.view_stats = c.view_stats;
    const g4s_packed_rows* const packed = c.packed;
    if (packed != nullptr && packed->rows != nullptr) {
        if (c.accumulate) return fail(G4S_ERR_INVALID_ARGUMENT, "packed rows: only the first view of a batch (first_view != 0) can write them");
        if (!packed->block_offs || packed->capacity < 0 || c.shs == nullptr)
            return fail(G4S_ERR_INVALID_ARGUMENT, "packed rows: block_offs must not be NULL, capacity >= 0, colours from SH");
        pb.packed_rows = packed->rows; pb.packed_block_offs = packed->block_offs;
        pb.packed_capacity = (uint32_t)(packed->capacity < 0xFFFFFFFFll ? packed->capacity : 0xFFFFFFFFll);
    }
    // The blend backward above touches only this call's own state; the per-Gaussian kernel below adds into tensors that
    // the previous view's backward -- on another stream -- may still be adding into: it waits for the caller's event.
    if (c.after_event) HIP_TRY(hipStreamWaitEvent(stream, (hipEvent_t)c.after_event, 0));
    pb.sh_vec16 = (c.shs != nullptr && c.shs_rest == nullptr && M == 16 && !misaligned(c.shs, 16) && !misaligned(c.dL_dsh, 16));
    pb.dL_dmean2D = c.dL_dmean2D; pb.dL_dnormal = c.dL_dnormal; pb.dL_dopacity = c.dL_dopacity; pb.dL_dcolor = c.dL_dcolor;
    pb.dL_dmean3D = c.dL_dmean3D; pb.dL_dtransMat = c.dL_dtransMat; pb.dL_dsh = c.dL_dsh; pb.dL_dscale = c.dL_dscale;
    pb.dL_drot = c.dL_drot;
    { ProfScope ps(PF_PREPROCESS_BWD, stream); launch_preprocess_bwd(pb, stream); }
    CHECK_LAUNCH("preprocess_bwd");
    return G4S_OK;
}

extern "C" int g4s_rasterizer_backward(
    int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
    const float* shs, const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
    const float* transMat_precomp, const float* viewmatrix, const float* projmatrix, const float* campos,
    float tan_fovx, float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
    const float* dL_dpix, const float* dL_depths, float* dL_dmean2D, float* dL_dnormal, float* dL_dopacity,
    float* dL_dcolor, float* dL_dmean3D, float* dL_dtransMat, float* dL_dsh, float* dL_dscale, float* dL_drot,
    char* workspace, size_t workspace_bytes, int debug, void* stream) {
    DECLARE_BACKWARD_CALL(c);
    c.shs = shs; c.colors_precomp = colors_precomp; c.dL_dsh = dL_dsh;
    return rasterizer_backward_impl(c);
}

extern "C" int g4s_rasterizer_backward_split_sh(
    int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
    const float* sh_dc, const float* sh_rest, const float* scales, float scale_modifier, const float* rotations,
    const float* transMat_precomp, const float* viewmatrix, const float* projmatrix, const float* campos,
    float tan_fovx, float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
    const float* dL_dpix, const float* dL_depths, float* dL_dmean2D, float* dL_dnormal, float* dL_dopacity,
    float* dL_dcolor, float* dL_dmean3D, float* dL_dtransMat, float* dL_dsh_dc, float* dL_dsh_rest, float* dL_dscale,
    float* dL_drot, char* workspace, size_t workspace_bytes, int debug, void* stream) {
    t_err[0] = 0;
    if (P > 0 && (!sh_dc || M < 1 || (M > 1 && (!sh_rest || !dL_dsh_rest))))
        return fail(G4S_ERR_INVALID_ARGUMENT, "split SH needs sh_dc / dL_dsh_dc and, for M > 1, sh_rest / dL_dsh_rest");
    DECLARE_BACKWARD_CALL(c);
    c.shs = sh_dc; c.shs_rest = M > 1 ? sh_rest : nullptr;
    c.dL_dsh = dL_dsh_dc; c.dL_dsh_rest = M > 1 ? dL_dsh_rest : nullptr;
    return rasterizer_backward_impl(c);
}

// Gradient accumulation over views (include/g4s_rasterizer.h).  sh_rest == NULL: sh_dc is the packed [P,M,3] tensor.
extern "C" int g4s_rasterizer_backward_accumulate_packed(
    int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
    const float* sh_dc, const float* sh_rest, const float* scales, float scale_modifier, const float* rotations,
    const float* transMat_precomp, const float* viewmatrix, const float* projmatrix, const float* campos,
    float tan_fovx, float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
    const float* dL_dpix, const float* dL_depths, float* dL_dmean2D, float* dL_dnormal, float* dL_dopacity,
    float* dL_dcolor, float* dL_dmean3D, float* dL_dtransMat, float* dL_dsh_dc, float* dL_dsh_rest, float* dL_dscale,
    float* dL_drot, float* view_stats, int first_view, const g4s_packed_rows* packed, char* workspace, size_t workspace_bytes,
    void* after_event, int debug, void* stream) {
    t_err[0] = 0;
    if (P > 0 && (!sh_dc || M < 1 || (sh_rest && M > 1 && !dL_dsh_rest)))
        return fail(G4S_ERR_INVALID_ARGUMENT, "accumulating backward needs SH coefficients (packed, or sh_dc + sh_rest / dL_dsh_rest)");
    DECLARE_BACKWARD_CALL(c);
    const bool split = sh_rest && M > 1;
    c.shs = sh_dc; c.shs_rest = split ? sh_rest : nullptr;
    c.dL_dsh = dL_dsh_dc; c.dL_dsh_rest = split ? dL_dsh_rest : nullptr;
    c.accumulate = first_view == 0; c.after_event = after_event; c.view_stats = view_stats; c.packed = packed;
    return rasterizer_backward_impl(c);
}

// (the one ABI-sized call left in this file: the same entry point without the packed rows)
extern "C" int g4s_rasterizer_backward_accumulate(
    int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
    const float* sh_dc, const float* sh_rest, const float* scales, float scale_modifier, const float* rotations,
    const float* transMat_precomp, const float* viewmatrix, const float* projmatrix, const float* campos,
    float tan_fovx, float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
    const float* dL_dpix, const float* dL_depths, float* dL_dmean2D, float* dL_dnormal, float* dL_dopacity,
    float* dL_dcolor, float* dL_dmean3D, float* dL_dtransMat, float* dL_dsh_dc, float* dL_dsh_rest, float* dL_dscale,
    float* dL_drot, float* view_stats, int first_view, char* workspace, size_t workspace_bytes, void* after_event, int debug,
    void* stream) {
    return g4s_rasterizer_backward_accumulate_packed(
        P, D, M, R, background, width, height, means3D, sh_dc, sh_rest, scales, scale_modifier, rotations, transMat_precomp,
        viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii, geom_buffer, binning_buffer, image_buffer, dL_dpix,
        dL_depths, dL_dmean2D, dL_dnormal, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dtransMat, dL_dsh_dc, dL_dsh_rest, dL_dscale,
        dL_drot, view_stats, first_view, /*packed=*/nullptr, workspace, workspace_bytes, after_event, debug, stream);
}
