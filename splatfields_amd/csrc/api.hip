// C ABI of libsplatraster.so (see include/splatraster.h for what each entry replaces).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <thread>
#include <mutex>
#include <string>
#include <vector>
#include "host_api.h"
#include "kernels.h"

namespace {

thread_local std::string g_last_error;
thread_local long long g_last_longest = -1;   // longest tile list of this thread's most recent sr_forward (sr_last_longest_list)

// ---- optional per-stage timing (HIP events on the launch stream) ----
struct ProfRec { int stage; hipEvent_t a, b; bool ended; unsigned long long serial; };
unsigned long long g_prof_serial = 0;
bool g_prof_on = false;
std::vector<ProfRec> g_prof;
std::mutex g_prof_mutex;   // host threads rendering on their own streams may record concurrently
const char* kStageNames[SR_PROFILE_STAGES] = {"preprocess", "scan", "emit", "sort_tiles", "render_forward",
                                              "render_backward", "preprocess_backward"};

}  // namespace

namespace sr {   // host_api.h: shared with the entry points in the ops' own files

int fail(const std::string& msg) { g_last_error = msg; return 1; }

int check_hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return 0;
    return fail(std::string(what) + ": " + hipGetErrorString(e));
}

StageTimer::StageTimer(int stage, hipStream_t s) : st(s) {
    if (!g_prof_on) return;
    ProfRec r; r.stage = stage; r.ended = false;
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
    hipEventRecord(r.a, st);
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    serial = ++g_prof_serial;
    r.serial = serial;
    g_prof.push_back(r); idx = 0;
    end = r.b;
}
// the end event is recorded under the same mutex that sr_profile_collect holds while it walks (and destroys) the list:
// a record whose timer is still open is left alone by the collector
StageTimer::~StageTimer() {
    if (idx < 0) return;
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    for (auto& r : g_prof)
        if (r.serial == serial) { hipEventRecord(end, st); r.ended = true; break; }
}

}  // namespace sr

using sr::fail; using sr::check_hip; using sr::StageTimer;

namespace {

// ---- status blocks: how the instance count of a forward reaches the host ------------------------------------------------
// A pinned, COHERENT 64-byte block of host memory: k_scan_small stores the instance count and the longest list into words 0 / 1
// (and the number of tiles that can hold a list of more than 2048 entries into word 4)
// and then -- system-scope release stores -- the block's current sequence number into words 2 / 3 (and 5).  The host polls those two
// words: nothing is enqueued in the stream for the read-back (rounds 1-3: a copy command; round 4: an event record, which still
// cost the stream ~8 us between k_scan_small and the scatter -- rocprofv3 kernel trace, profiles/r05_v1_*).
// sr_forward keeps one block per (host thread, device); sr_forward_async hands one out per forward in flight (a "ticket",
// pooled per device under a mutex).  A few bytes each, created lazily.
struct StatusBlock { uint32_t* pinned = nullptr; uint32_t* pinned_dev = nullptr; uint32_t seq = 0; hipStream_t stream = nullptr; int dev = 0; };
thread_local StatusBlock g_sync[64];
std::mutex g_ticket_mutex;
std::vector<StatusBlock*> g_ticket_free[64];
// diagnostics (sr_debug_counters): [0] host waits inside sr_forward, [1] sr_forward_async calls, [2] ticket redemptions that
// found stage 1 still running (the host had to wait), [3] tickets ever created
std::atomic<long long> g_counters[4];
// diagnostics (sr_debug_sort_counters): launches of the separate per-tile sort classes in front of the forward blend:
// [0] k_sort_tiles_regs (lists up to 2048 entries: the standalone switch only), [1] 2049..4096, [2] 4097..8192, [3] longer
std::atomic<long long> g_sort_counters[4];

int status_block_init(StatusBlock& b, int dev) {
    // coherent (fine-grained) host memory: the kernel's stores become visible to the host while the stream keeps running
    if (hipHostMalloc(reinterpret_cast<void**>(&b.pinned), 64, hipHostMallocCoherent) != hipSuccess &&
        hipHostMalloc(reinterpret_cast<void**>(&b.pinned), 64, hipHostMallocDefault) != hipSuccess) return fail("hipHostMalloc failed");
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, b.pinned, 0) != hipSuccess) { hipHostFree(b.pinned); b.pinned = nullptr; return fail("hipHostGetDevicePointer failed"); }
    b.pinned_dev = static_cast<uint32_t*>(dp);
    for (int i = 0; i < 16; ++i) b.pinned[i] = 0u;
    b.dev = dev; b.seq = 0;
    return 0;
}
// a new use of the block: the sequence number the kernel will publish (never 0)
uint32_t status_block_arm(StatusBlock& b, hipStream_t st) {
    b.seq = b.seq + 1u == 0u ? 1u : b.seq + 1u;
    b.stream = st;
    return b.seq;
}
// Waits until both words of the armed use have arrived.  *waited = the first look found them missing.  Polls (the data arrives
// while the stream runs); after two seconds without it falls back to draining the stream, which also surfaces a failed launch.
int status_block_wait(StatusBlock& b, bool* waited) {
    volatile uint32_t* p = b.pinned;
    auto ready = [&] { return p[2] == b.seq && p[3] == b.seq && p[5] == b.seq; };
    if (waited) *waited = false;
    if (!ready()) {
        if (waited) *waited = true;
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spins = 0; !ready(); ++spins) {
            if (spins > 4096u) std::this_thread::yield();
            if ((spins & 0xfffu) == 0xfffu && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
                SR_TRY(check_hip(hipStreamSynchronize(b.stream), "wait for the instance count"));
                if (!ready()) return fail("the instance count of the forward never reached the host (k_scan_small did not run?)");
            }
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return 0;
}

int current_device(int* dev) {
    if (hipGetDevice(dev) != hipSuccess || *dev < 0 || *dev >= 64) return fail("hipGetDevice failed");
    return 0;
}

// the calling thread's block for the current device (sr_forward, sr_forward_prepare)
int thread_block(StatusBlock** out) {
    int dev = 0;
    SR_TRY(current_device(&dev));
    *out = &g_sync[dev];
    return (*out)->pinned ? 0 : status_block_init(**out, dev);   // created at the thread's first forward on this device
}

int ticket_acquire(StatusBlock** out) {
    int dev = 0;
    SR_TRY(current_device(&dev));
    {
        std::lock_guard<std::mutex> lock(g_ticket_mutex);
        if (!g_ticket_free[dev].empty()) { *out = g_ticket_free[dev].back(); g_ticket_free[dev].pop_back(); return 0; }
    }
    StatusBlock* t = new StatusBlock;
    if (int rc = status_block_init(*t, dev)) { delete t; return rc; }
    g_counters[3].fetch_add(1, std::memory_order_relaxed);
    *out = t;
    return 0;
}
void ticket_recycle(StatusBlock* t) {
    std::lock_guard<std::mutex> lock(g_ticket_mutex);
    g_ticket_free[t->dev].push_back(t);
}

// 0 = the product choice (entry-per-lane at every footprint), 1 = pixel-per-lane, 2 = entry-per-lane (sr_set_backward_kernel)
std::atomic<int> g_bwd_kernel{[] {
    const char* sel = getenv("SPLATRASTER_BWD");
    return !sel ? 0 : (std::string(sel) == "wave" ? 1 : (std::string(sel) == "quads" ? 2 : 0));
}()};

// Who sorts the tile lists of up to 4096 entries.  0 = the product choice: the workgroup of k_render_forward that blends the
// list (lists of 2049..4096 entries only on views with few of them); 1 = sort kernels in launches of their own in front of the
// forward; 2 = the forward sorts the lists of up to 2048 entries only (sr_set_sort_kernel)
std::atomic<int> g_sort_kernel{[] {
    const char* sel = getenv("SPLATRASTER_SORT");
    return !sel ? 0 : (std::string(sel) == "standalone" ? 1 : (std::string(sel) == "short" ? 2 : 0));
}()};
thread_local long long g_last_long_tiles = -1;     // sr_last_long_tiles
thread_local long long g_expect_long_tiles = -1;   // sr_expect_long_tiles: consumed by the thread's next sr_forward_async

// ---- debug = true: input snapshot on a failed launch ------------------------------------------------------------------
// [EXT] with `debug` set synchronises after every kernel and, when one fails, dumps the call's arguments to
// snapshot_fw.dump / snapshot_bw.dump in the working directory before it re-raises (SURVEY.md section 8b "Error
// conventions").  Same here.  File: "SRSNAP1\0", the failing stage (32 bytes), then records {name[16], uint64 bytes, payload}:
// "view" (SrView scalars: height, width, tanfovx, tanfovy, scale_modifier, sh_degree, sh_coeffs, prefiltered as 8 x 4 bytes),
// "count" (int32), the four camera arrays and every per-splat input that was passed (copied back from the device; a record
// whose copy fails -- the device may be gone after a fault -- has bytes = 0), for the backward also the upstream gradients.
struct CallContext { const SrView* view = nullptr; const SrSplats* splats = nullptr; const char* file = nullptr;
                     const float* dL_dcolor = nullptr; const float* dL_ddepth = nullptr; const float* dL_dalpha = nullptr; };
thread_local CallContext g_call;

void dump_record(FILE* f, const char* name, const void* dev, size_t bytes, bool on_device) {
    char tag[16] = {0};
    std::strncpy(tag, name, 15);
    std::vector<char> host;
    uint64_t n = 0;
    if (dev && bytes) {
        host.resize(bytes);
        if (!on_device) { std::memcpy(host.data(), dev, bytes); n = bytes; }
        else if (hipMemcpy(host.data(), dev, bytes, hipMemcpyDeviceToHost) == hipSuccess) n = bytes;
        else (void)hipGetLastError();
    }
    std::fwrite(tag, 1, 16, f); std::fwrite(&n, 8, 1, f);
    if (n) std::fwrite(host.data(), 1, (size_t)n, f);
}

void dump_snapshot(const char* stage) {
    const CallContext& c = g_call;
    if (!c.view || !c.splats || !c.file) return;
    FILE* f = std::fopen(c.file, "wb");
    if (!f) return;
    char head[8] = {'S', 'R', 'S', 'N', 'A', 'P', '1', 0}, st[32] = {0};
    std::strncpy(st, stage, 31);
    std::fwrite(head, 1, 8, f); std::fwrite(st, 1, 32, f);
    const SrView* v = c.view; const SrSplats* s = c.splats;
    const int32_t vi[4] = {v->image_height, v->image_width, v->sh_degree, v->sh_coeffs};
    const float vf[3] = {v->tanfovx, v->tanfovy, v->scale_modifier};
    char vb[32]; std::memcpy(vb, vi, 16); std::memcpy(vb + 16, vf, 12); const int32_t pf = v->prefiltered; std::memcpy(vb + 28, &pf, 4);
    dump_record(f, "view", vb, 32, false);
    const int32_t n = s->count;
    dump_record(f, "count", &n, 4, false);
    dump_record(f, "viewmatrix", v->viewmatrix, 64, true); dump_record(f, "projmatrix", v->projmatrix, 64, true);
    dump_record(f, "campos", v->campos, 12, true); dump_record(f, "bg", v->bg, 12, true);
    const size_t N = (size_t)(n > 0 ? n : 0);
    dump_record(f, "means3D", s->means3D, N * 12, true); dump_record(f, "opacities", s->opacities, N * 4, true);
    dump_record(f, "scales", s->scales, N * 12, true); dump_record(f, "rotations", s->rotations, N * 16, true);
    dump_record(f, "cov3D_precomp", s->cov3D_precomp, N * 24, true);
    dump_record(f, "shs", s->shs, s->shs ? N * 12 * (size_t)(s->shs_rest ? 1 : v->sh_coeffs) : 0, true);
    dump_record(f, "shs_rest", s->shs_rest, N * 12 * 15, true);
    dump_record(f, "colors_precomp", s->colors_precomp, N * 12, true);
    const size_t px = (size_t)v->image_height * v->image_width;
    dump_record(f, "dL_dcolor", c.dL_dcolor, px * 12, true); dump_record(f, "dL_ddepth", c.dL_ddepth, px * 4, true);
    dump_record(f, "dL_dalpha", c.dL_dalpha, px * 4, true);
    std::fclose(f);
}

int after_launch(const SrView* view, hipStream_t st, const char* what) {
    int rc = check_hip(hipGetLastError(), what);
    if (!rc && view && view->debug) rc = check_hip(hipStreamSynchronize(st), what);
    if (rc && view && view->debug) {
        const std::string keep = g_last_error;
        dump_snapshot(what);
        g_last_error = keep + (g_call.file ? std::string(" (inputs written to ") + g_call.file + ")" : std::string());
    }
    return rc;
}

int validate(const SrView* view, const SrSplats* s) {
    if (!view || !s) return fail("null view/splats");
    if (s->count < 0) return fail("negative splat count");
    if (view->image_height <= 0 || view->image_width <= 0) return fail("image size must be positive");
    if (!view->viewmatrix || !view->projmatrix || !view->campos || !view->bg) return fail("viewmatrix/projmatrix/campos/bg must be device pointers");
    if (s->count > 0) {
        if (!s->means3D || !s->opacities) return fail("means3D/opacities missing");
        const bool has_sr = s->scales && s->rotations;
        if (has_sr == (s->cov3D_precomp != nullptr)) return fail("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
        if ((s->shs != nullptr) == (s->colors_precomp != nullptr)) return fail("Please provide excatly one of either SHs or precomputed colors!");
        if (s->shs) {
            if (view->sh_degree < 0 || view->sh_degree > 3) return fail("sh_degree must be 0..3");
            if (view->sh_coeffs < (view->sh_degree + 1) * (view->sh_degree + 1)) return fail("shs holds fewer coefficients than sh_degree needs");
            if (s->shs_rest) {
                if (view->sh_coeffs != 16) return fail("shs_rest (dc + rest SH tensors) needs sh_coeffs == 16");
                if ((reinterpret_cast<uintptr_t>(s->shs) | reinterpret_cast<uintptr_t>(s->shs_rest)) & 15u) return fail("shs / shs_rest must be 16-byte aligned");
            }
        } else if (s->shs_rest) return fail("shs_rest without shs");
        if (s->raw_params & ~(SR_RAW_SCALES | SR_RAW_OPACITY | SR_RAW_ROTATIONS | SR_FORWARD_ONLY)) return fail("unknown bits in raw_params");
        if (s->cov3D_precomp && (s->raw_params & (SR_RAW_SCALES | SR_RAW_ROTATIONS))) return fail("raw scales/rotations with cov3D_precomp");
    }
    // tile coordinates are stored in 12 bits (Geom::rect carries the small rectangles' reach mask in the top nibbles, common.h)
    if ((sr::tiles_x(view->image_width) > sr::kMaxTilesPerSide) || (sr::tiles_y(view->image_height) > sr::kMaxTilesPerSide)) return fail("image too large (more than 65520 pixels a side)");
    return 0;
}

sr::ViewK make_view(const SrView* v) {
    sr::ViewK k;
    k.H = v->image_height; k.W = v->image_width;
    k.gx = sr::tiles_x(k.W); k.gy = sr::tiles_y(k.H);
    k.tanfovx = v->tanfovx; k.tanfovy = v->tanfovy;
    k.focal_x = k.W / (2.0f * v->tanfovx); k.focal_y = k.H / (2.0f * v->tanfovy);
    k.scale_modifier = v->scale_modifier;
    k.sh_degree = v->sh_degree; k.sh_coeffs = v->sh_coeffs;
    k.viewmatrix = v->viewmatrix; k.projmatrix = v->projmatrix; k.campos = v->campos; k.bg = v->bg;
    return k;
}

sr::SplatsK make_splats(const SrSplats* s) {
    sr::SplatsK k;
    k.N = s->count; k.means3D = s->means3D; k.opacities = s->opacities; k.scales = s->scales;
    k.rotations = s->rotations; k.cov3D = s->cov3D_precomp; k.shs = s->shs; k.colors = s->colors_precomp;
    k.raw = s->raw_params; k.shs_rest = s->shs_rest;
    return k;
}

// The sort classes a list-length hint asks for: lists of up to 2048 / 4096 / 8192 entries, or (-1) all of them.  The Python
// facade judges an overflow by the same figure (splatfields_amd/rasterizer.py: _covered_by_hint): change both together.
long long covered_by_hint(long long hint) { return hint <= 2048 ? 2048 : hint <= 4096 ? 4096 : hint <= 8192 ? 8192 : -1; }

// What every forward / backward entry opens with.  open_call: the arguments validated, the call remembered for the debug
// snapshot, the kernel-side view and splats.  The entry then checks its own buffers (validate first, buffers second: a call
// with a bad view AND null buffers reports the view) and carves the opaque ones it uses.
struct Call {
    hipStream_t st = nullptr;
    sr::ViewK v; sr::SplatsK s;
    sr::Geom g; sr::Binning b; sr::Image im;
    void carve(const void* geom, void* binning, long long capacity, const void* image) {
        sr::carve_geom(const_cast<void*>(geom), s.N, v.H, v.W, &g);
        if (binning) sr::carve_binning(binning, capacity, &b);
        if (image) sr::carve_image(const_cast<void*>(image), v.H, v.W, &im);
    }
};

int open_call(Call& c, const CallContext& ctx, void* hip_stream) {
    SR_TRY(validate(ctx.view, ctx.splats));
    g_call = ctx;
    c.st = static_cast<hipStream_t>(hip_stream);
    c.v = make_view(ctx.view);
    c.s = make_splats(ctx.splats);
    return 0;
}

bool capacity_in_range(long long r) { return r >= 0 && r < (1ll << 32); }

}  // namespace

extern "C" {

int sr_version(void) { return SR_VERSION; }
const char* sr_last_error(void) { return g_last_error.c_str(); }

size_t sr_geom_bytes(int n, int h, int w) { return sr::carve_geom(nullptr, n, h, w, nullptr); }
size_t sr_binning_bytes(long long r, int, int) { return sr::carve_binning(nullptr, r, nullptr); }
size_t sr_image_bytes(int h, int w) { return sr::carve_image(nullptr, h, w, nullptr); }
// scratch layout: one 48-byte gradient slot per tile-splat instance (written only for the instances the forward reached)
size_t sr_backward_scratch_bytes(long long r) {
    const size_t n = (size_t)(r > 0 ? r : 1);
    return sr::align_up(n * sr::kSlotFloats * sizeof(float), 256);
}

}  // extern "C"

namespace {

int launch_stage1(const SrView* view, const sr::ViewK& v, const sr::SplatsK& s, const sr::Geom& g, int* radii, uint32_t* host_out,
                  uint32_t host_seq, hipStream_t st) {
    { StageTimer t_(0, st); sr::launch_preprocess(v, s, g, radii, st); }
    SR_TRY(after_launch(view, st, "preprocess"));
    { StageTimer t_(1, st); sr::launch_count_tiles(v, s.N, g, st); sr::launch_scan_small(v, s.N, g, host_out, host_seq, st); }
    SR_TRY(after_launch(view, st, "scan"));
    return 0;
}

// hs != nullptr: k_scan_small stores the instance count / longest list into hs->pinned (status block above); the host waits for
// them after launching the scatter (the GPU keeps working) and then launches only the sort classes that are needed.
// hs == nullptr: nobody waits; `max_len` = the longest list the sort classes must cover (< 0: launch every class).
// Sort: the forward blend sorts every list of up to 2048 entries itself (stage 4), and the lists of 2049..4096 entries of a view
// that has few of them; the other classes that max_len asks for are launched in front of it (stage 3, empty on most views).
// long_tiles (< 0: unknown): how many tiles can hold a list of more than 2048 entries, known or expected -- with few of them the
// launch of that class is left out (launch_sort_tiles).  The standalone switch restores a launch per class.  Either way
// Binning::sorted_up_to means what it always did: lists longer than the classes that ran have no result.
int launch_stage2(const SrView* view, const sr::ViewK& v, const sr::SplatsK& s, const sr::Geom& g, const sr::Binning& b_in,
                  const sr::Image& im, float* out_color, float* out_depth, float* out_alpha, StatusBlock* hs, long long max_len,
                  long long expected_len, long long long_tiles, hipStream_t st) {
    sr::Binning b = b_in;
    const int who = g_sort_kernel.load(std::memory_order_relaxed);   // one read: the launches below must agree
    b.sort_in_blend = who == 1 ? 0u : (who == 2 ? 2048u : 4096u);
    { StageTimer t_(2, st); sr::launch_emit(v, s.N, g, b, st); }
    SR_TRY(after_launch(view, st, "emit"));
    if (hs) {
        g_counters[0].fetch_add(1, std::memory_order_relaxed);
        SR_TRY(status_block_wait(*hs, nullptr));
        max_len = (long long)hs->pinned[1];
        long_tiles = (long long)hs->pinned[4];   // tiles that can hold a list of more than 2048 entries
        // the binning buffer is too small: the scatter just launched exits on its own, and nothing else of stage 2 is worth
        // launching -- the caller re-runs it with a buffer that fits (SR_NEED_CAPACITY)
        if ((long long)hs->pinned[0] > (long long)b.capacity) return 0;
    }
    int classes = 0;
    { StageTimer t_(3, st); classes = sr::launch_sort_tiles(v, g, b, max_len, expected_len, long_tiles, st); }
    b.long_class_launched = (classes & 2) ? 1u : 0u;
    for (int k = 0; k < 4; ++k) if (classes & (1 << k)) g_sort_counters[k].fetch_add(1, std::memory_order_relaxed);
    SR_TRY(after_launch(view, st, "sort_tiles"));
    { StageTimer t_(4, st); sr::launch_render_forward(v, g, b, im, out_color, out_depth, out_alpha, st); }
    SR_TRY(after_launch(view, st, "render_forward"));
    return 0;
}

}  // namespace

extern "C" {

int sr_forward_prepare(const SrView* view, const SrSplats* splats, void* geom, int* radii,
                       long long* instances_out, void* hip_stream) {
    Call c;
    SR_TRY(open_call(c, CallContext{view, splats, "snapshot_fw.dump"}, hip_stream));
    if (!geom || !instances_out || (splats->count > 0 && !radii)) return fail("null geom/radii/instances_out");
    c.carve(geom, nullptr, 0, nullptr);
    StatusBlock* hs = nullptr;
    SR_TRY(thread_block(&hs));
    SR_TRY(launch_stage1(view, c.v, c.s, c.g, radii, hs->pinned_dev, status_block_arm(*hs, c.st), c.st));
    SR_TRY(check_hip(hipStreamSynchronize(c.st), "sync after prepare"));
    *instances_out = (long long)hs->pinned[0];
    return 0;
}

int sr_forward(const SrView* view, const SrSplats* splats, void* geom, int* radii, void* binning,
               long long binning_capacity, void* image, float* out_color, float* out_depth, float* out_alpha,
               long long* instances_out, void* hip_stream) {
    Call c;
    SR_TRY(open_call(c, CallContext{view, splats, "snapshot_fw.dump"}, hip_stream));
    if (!geom || !binning || !image || !out_color || !out_depth || !instances_out || (splats->count > 0 && !radii)) return fail("null buffer");
    if (!capacity_in_range(binning_capacity)) return fail("binning capacity out of range");
    c.carve(geom, binning, binning_capacity, image);
    StatusBlock* hs = nullptr;
    SR_TRY(thread_block(&hs));
    SR_TRY(launch_stage1(view, c.v, c.s, c.g, radii, hs->pinned_dev, status_block_arm(*hs, c.st), c.st));   // k_scan_small stores the counters into hs->pinned
    SR_TRY(launch_stage2(view, c.v, c.s, c.g, c.b, c.im, out_color, out_depth, out_alpha, hs, -1, -1, -1, c.st));  // waits inside, GPU busy
    const long long total = (long long)hs->pinned[0];
    *instances_out = total;
    g_last_longest = (long long)hs->pinned[1];
    g_last_long_tiles = (long long)hs->pinned[4];
    return total > binning_capacity ? SR_NEED_CAPACITY : 0;
}

int sr_forward_render(const SrView* view, const SrSplats* splats, void* geom, void* binning,
                      long long instances, void* image, float* out_color, float* out_depth,
                      float* out_alpha, void* hip_stream) {
    Call c;
    SR_TRY(open_call(c, CallContext{view, splats, "snapshot_fw.dump"}, hip_stream));
    if (!geom || !binning || !image || !out_color || !out_depth) return fail("null buffer");
    if (!capacity_in_range(instances)) return fail("instance count out of range");
    c.carve(geom, binning, instances, image);
    return launch_stage2(view, c.v, c.s, c.g, c.b, c.im, out_color, out_depth, out_alpha, nullptr, -1, -1, -1, c.st);
}

int sr_forward_async(const SrView* view, const SrSplats* splats, void* geom, int* radii, void* binning,
                     long long binning_capacity, long long longest_list_hint, long long longest_list_expected, void* image,
                     float* out_color, float* out_depth, float* out_alpha, void** ticket_out, void* hip_stream) {
    Call c;
    SR_TRY(open_call(c, CallContext{view, splats, "snapshot_fw.dump"}, hip_stream));
    if (!geom || !binning || !image || !out_color || !out_depth || !ticket_out || (splats->count > 0 && !radii)) return fail("null buffer");
    if (!capacity_in_range(binning_capacity)) return fail("binning capacity out of range");
    if (longest_list_hint < 0) return fail("longest_list_hint must be >= 0");
    c.carve(geom, binning, binning_capacity, image);
    const long long covered = covered_by_hint(longest_list_hint);
    c.b.sorted_up_to = covered < 0 ? 0xffffffffu : (uint32_t)covered;
    const long long long_tiles = g_expect_long_tiles;   // this call's, whether it succeeds or not
    g_expect_long_tiles = -1;
    StatusBlock* t = nullptr;
    SR_TRY(ticket_acquire(&t));
    int rc = launch_stage1(view, c.v, c.s, c.g, radii, t->pinned_dev, status_block_arm(*t, c.st), c.st);
    if (!rc) rc = launch_stage2(view, c.v, c.s, c.g, c.b, c.im, out_color, out_depth, out_alpha, nullptr, covered,
                                longest_list_expected >= 0 && longest_list_expected <= longest_list_hint ? longest_list_expected : -1,
                                long_tiles, c.st);
    if (rc) {   // nothing of this call may still write the block when it is handed out again
        (void)hipStreamSynchronize(c.st);
        ticket_recycle(t);
        return rc;
    }
    g_counters[1].fetch_add(1, std::memory_order_relaxed);
    *ticket_out = t;
    return 0;
}

int sr_ticket_wait(void* ticket, long long* instances_out, long long* longest_list_out) {
    if (!ticket) return fail("null ticket");
    StatusBlock* t = static_cast<StatusBlock*>(ticket);
    bool waited = false;
    const int rc = status_block_wait(*t, &waited);
    if (waited) g_counters[2].fetch_add(1, std::memory_order_relaxed);
    if (rc) {
        // The figures never arrived (failed launch, lost device): the block is NOT handed out again -- a k_scan_small that runs
        // late after all would write into a block that belongs to another forward by then -- and the outputs stay untouched.
        // 64 bytes of pinned memory are leaked per failed forward; the process is about to report a device error anyway.
        return rc;
    }
    if (instances_out) *instances_out = (long long)t->pinned[0];
    if (longest_list_out) *longest_list_out = (long long)t->pinned[1];
    g_last_long_tiles = (long long)t->pinned[4];
    ticket_recycle(t);
    return 0;
}

long long sr_last_longest_list(void) { return g_last_longest; }
long long sr_last_long_tiles(void) { return g_last_long_tiles; }
int sr_expect_long_tiles(long long tiles) { g_expect_long_tiles = tiles < 0 ? -1 : tiles; return 0; }

int sr_ticket_release(void* ticket) { return sr_ticket_wait(ticket, nullptr, nullptr); }

int sr_forward_prepare_views(int n_views, const SrView* views, const SrSplats* splats, void* const* geoms, int* const* radii,
                             long long* instances_out, long long* longest_out, long long* long_tiles_out, void* hip_stream) {
    if (n_views < 1) return fail("sr_forward_prepare_views: n_views must be at least 1");
    if (!views || !splats || !geoms || !radii || !instances_out || !longest_out || !long_tiles_out)
        return fail("null table in sr_forward_prepare_views");
    // everything is validated before the first launch: a refused call has launched nothing and holds no block
    std::vector<Call> calls((size_t)n_views);
    for (int v = 0; v < n_views; ++v) {
        SR_TRY(open_call(calls[v], CallContext{&views[v], &splats[v], "snapshot_fw.dump"}, hip_stream));
        if (views[v].image_height != views[0].image_height || views[v].image_width != views[0].image_width || splats[v].count != splats[0].count)
            return fail("sr_forward_prepare_views: the views of one call share the image size and the splat count (view " + std::to_string(v) + ")");
        if (!geoms[v] || (splats[v].count > 0 && !radii[v])) return fail("null geom/radii in sr_forward_prepare_views (view " + std::to_string(v) + ")");
        calls[v].carve(geoms[v], nullptr, 0, nullptr);
    }
    std::vector<StatusBlock*> blocks;
    int rc = 0;
    for (int v = 0; v < n_views && !rc; ++v) {
        StatusBlock* t = nullptr;
        rc = ticket_acquire(&t);
        if (rc) break;
        blocks.push_back(t);
        g_call = CallContext{&views[v], &splats[v], "snapshot_fw.dump"};   // the debug snapshot of a failed stage names this view
        rc = launch_stage1(&views[v], calls[v].v, calls[v].s, calls[v].g, radii[v], t->pinned_dev, status_block_arm(*t, calls[v].st), calls[v].st);
    }
    if (rc) {   // nothing of this call may still write a block when it is handed out again (sr_forward_async's rule)
        (void)hipStreamSynchronize(static_cast<hipStream_t>(hip_stream));
        for (StatusBlock* t : blocks) ticket_recycle(t);
        return rc;
    }
    g_counters[0].fetch_add(1, std::memory_order_relaxed);   // one wait: the stream is in order, the last view's figures arrive last
    for (int v = n_views - 1; v >= 0; --v) {
        StatusBlock* t = blocks[(size_t)v];
        if (rc) continue;   // figures that never arrived: neither this block nor the ones not yet looked at are reused (sr_ticket_wait)
        rc = status_block_wait(*t, nullptr);
        if (rc) continue;
        instances_out[v] = (long long)t->pinned[0];
        longest_out[v] = (long long)t->pinned[1];
        long_tiles_out[v] = (long long)t->pinned[4];
        ticket_recycle(t);
    }
    return rc;
}

int sr_forward_render_views(int n_views, const SrView* views, const SrSplats* splats, void* const* geoms, void* const* binnings,
                            const long long* capacities, const long long* longest, const long long* long_tiles, void* const* images,
                            float* const* out_color, float* const* out_depth, float* const* out_alpha, void* hip_stream) {
    if (n_views < 1) return fail("sr_forward_render_views: n_views must be at least 1");
    if (!views || !splats || !geoms || !binnings || !capacities || !longest || !long_tiles || !images || !out_color || !out_depth)
        return fail("null table in sr_forward_render_views");
    std::vector<Call> calls((size_t)n_views);
    for (int v = 0; v < n_views; ++v) {
        const std::string at = " (view " + std::to_string(v) + ")";
        SR_TRY(open_call(calls[v], CallContext{&views[v], &splats[v], "snapshot_fw.dump"}, hip_stream));
        if (!geoms[v] || !binnings[v] || !images[v] || !out_color[v] || !out_depth[v]) return fail("null buffer in sr_forward_render_views" + at);
        if (!capacity_in_range(capacities[v])) return fail("sr_forward_render_views: binning capacity out of range" + at);
        if (longest[v] < 0 || long_tiles[v] < 0) return fail("sr_forward_render_views: the longest list and the long-tile count must be the figures of sr_forward_prepare_views" + at);
        calls[v].carve(geoms[v], binnings[v], capacities[v], images[v]);
    }
    for (int v = 0; v < n_views; ++v) {
        Call& c = calls[v];
        g_call = CallContext{&views[v], &splats[v], "snapshot_fw.dump"};
        // the figures are known: nobody waits, and launch_sort_tiles takes them as sr_forward's wait would have delivered them
        SR_TRY(launch_stage2(&views[v], c.v, c.s, c.g, c.b, c.im, out_color[v], out_depth[v], out_alpha ? out_alpha[v] : nullptr, nullptr,
                             longest[v], longest[v], long_tiles[v], c.st));
    }
    return 0;
}

int sr_debug_counters(long long* out4, int reset) {
    if (!out4) return fail("null pointer in sr_debug_counters");
    for (int i = 0; i < 4; ++i) out4[i] = reset ? g_counters[i].exchange(0, std::memory_order_relaxed) : g_counters[i].load(std::memory_order_relaxed);
    return 0;
}

int sr_debug_sort_counters(long long* out4, int reset) {
    if (!out4) return fail("null pointer in sr_debug_sort_counters");
    for (int i = 0; i < 4; ++i) out4[i] = reset ? g_sort_counters[i].exchange(0, std::memory_order_relaxed) : g_sort_counters[i].load(std::memory_order_relaxed);
    return 0;
}

namespace {
// what: 1 = backward blend, 2 = per-splat part for splats [first, first + count), 3 = both
int backward_impl(int what, const SrView* view, const SrSplats* splats, const void* geom, void* binning,
                  long long instances, long long instances_rendered, const void* image, const int* radii,
                  const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha, void* scratch,
                  const SrGrads* grads, int first, int count, void* hip_stream) {
    Call c;
    SR_TRY(open_call(c, CallContext{view, splats, "snapshot_bw.dump", dL_dcolor, dL_ddepth, dL_dalpha}, hip_stream));
    if (!geom || !binning || !image || !scratch) return fail("null buffer");
    if ((what & 1) && !dL_dcolor) return fail("null buffer");
    if ((what & 2) && !grads) return fail("null buffer");
    if (what & 2) {
        if (splats->count > 0 && (!radii || !grads->dL_dmeans3D || !grads->dL_dmeans2D || !grads->dL_dopacity)) return fail("null gradient output");
        if (splats->count > 0 && splats->shs && !grads->dL_dshs && !grads->dL_dcolors) return fail("dL_dshs (or dL_dcolors for the colour-gradient mode) missing");
        if (splats->count > 0 && splats->shs_rest && grads->dL_dshs && !grads->dL_dshs_rest) return fail("dL_dshs_rest missing");
        if (splats->count > 0 && splats->colors_precomp && !grads->dL_dcolors) return fail("dL_dcolors missing");
        if (splats->count > 0 && splats->cov3D_precomp && !grads->dL_dcov3D) return fail("dL_dcov3D missing");
        if (splats->count > 0 && !splats->cov3D_precomp && (!grads->dL_dscales || !grads->dL_drotations)) return fail("dL_dscales/dL_drotations missing");
        if (first < 0 || count < 0 || (first % sr::kBlock) != 0) return fail("splat range must start at a multiple of 256");
    }
    if (splats->raw_params & SR_FORWARD_ONLY) return fail("the forward of these buffers was run with SR_FORWARD_ONLY");
    c.carve(geom, binning, instances, image);   // Binning::reached is written by the backward blend (splatraster.h)
    const hipStream_t st = c.st;
    const sr::SplatsK& s = c.s;
    float* slots = static_cast<float*>(scratch);
    if (what & 1) {
        StageTimer t_(5, st);
        // Two kernels, one slot format.  The entry-per-lane kernel over 4x4 quads (blend_bwd.hip) is the product path at EVERY
        // footprint.  (Round 2 measured a crossover -- pixel-per-lane 0.192 vs 0.203 ms at 7.4 instances per splat, 0.182 vs 0.203
        // at 15 -- and rounds 2-5 switched kernels at SR_BWD_SLOT_SPEC_BELOW instances per splat.  Re-measured in round 6, after
        // three rounds of work on the quad kernel only (MI355X, 800x800, ms of the backward blend, quads vs pixel-per-lane): 4.6
        // instances per splat 0.156 vs 0.262, 7.4: 0.136 vs 0.212, 15: 0.129 vs 0.186, 67: 0.157 vs 0.210, 225: 0.182 vs 0.211,
        // 715: 0.163 vs 0.179, 1270: 0.168 vs 0.171.)  The pixel-per-lane kernel (render.hip) stays as an independently written
        // second implementation of the same slots: SPLATRASTER_BWD=wave / sr_set_backward_kernel(1) select it, the tests and
        // tools/fuzz_backward.py compare the two.
        const int pinned = g_bwd_kernel.load(std::memory_order_relaxed);   // sr_set_backward_kernel / SPLATRASTER_BWD at load time
        const bool wave_kernel = pinned == 1;
        if (wave_kernel) sr::launch_render_backward(c.v, c.g, c.b, c.im, dL_dcolor, dL_ddepth, dL_dalpha, slots, st);
        else sr::launch_render_backward_quads(c.v, c.g, c.b, c.im, dL_dcolor, dL_ddepth, dL_dalpha, slots, st);
    }
    if (what & 1) SR_TRY(after_launch(view, st, "render_backward"));
    if (what & 2) {
        sr::GradsK gr;
        gr.means3D = grads->dL_dmeans3D; gr.means2D = grads->dL_dmeans2D; gr.opacity = grads->dL_dopacity;
        gr.scales = s.cov3D ? nullptr : grads->dL_dscales; gr.rotations = s.cov3D ? nullptr : grads->dL_drotations;
        gr.cov3D = s.cov3D ? grads->dL_dcov3D : nullptr;
        gr.shs = s.shs ? grads->dL_dshs : nullptr;
        gr.shs_rest = (s.shs_rest && gr.shs) ? grads->dL_dshs_rest : nullptr;
        gr.colors = (s.colors || (s.shs && !grads->dL_dshs)) ? grads->dL_dcolors : nullptr;  // SH input + colours only: colour-gradient mode
        // small footprints (fewer than SR_BWD_SLOT_SPEC_BELOW instances per splat on average; unknown counts as small): the
        // variant that requests a splat's first gradient slots together with their `reached` bytes
        const bool small_fp = !(instances_rendered >= 0 && instances_rendered > (long long)SR_BWD_SLOT_SPEC_BELOW * (long long)s.N);
        { StageTimer t_(6, st); sr::launch_preprocess_backward(c.v, s, c.g, radii, slots, c.b.reached, gr, first, count, small_fp, st); }
        SR_TRY(after_launch(view, st, "preprocess_backward"));
    }
    return 0;
}
}  // namespace

int sr_backward(const SrView* view, const SrSplats* splats, const void* geom, void* binning,
                long long instances, long long instances_rendered, const void* image, const int* radii,
                const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha, void* scratch,
                const SrGrads* grads, void* hip_stream) {
    return backward_impl(3, view, splats, geom, binning, instances, instances_rendered, image, radii, dL_dcolor, dL_ddepth, dL_dalpha,
                         scratch, grads, 0, splats ? splats->count : 0, hip_stream);
}

int sr_backward_blend(const SrView* view, const SrSplats* splats, const void* geom, void* binning,
                      long long instances, long long instances_rendered, const void* image,
                      const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha, void* scratch, void* hip_stream) {
    return backward_impl(1, view, splats, geom, binning, instances, instances_rendered, image, nullptr, dL_dcolor, dL_ddepth, dL_dalpha,
                         scratch, nullptr, 0, 0, hip_stream);
}

int sr_backward_splats(const SrView* view, const SrSplats* splats, const void* geom, void* binning,
                       long long instances, long long instances_rendered, const void* image, const int* radii, void* scratch,
                       const SrGrads* grads, int first_splat, int n_splats, void* hip_stream) {
    return backward_impl(2, view, splats, geom, binning, instances, instances_rendered, image, radii, nullptr, nullptr, nullptr, scratch,
                         grads, first_splat, n_splats, hip_stream);
}

int sr_set_backward_kernel(int which) {
    if (which < 0 || which > 2) return -1;
    return g_bwd_kernel.exchange(which, std::memory_order_relaxed);
}

int sr_set_sort_kernel(int which) {
    if (which < 0 || which > 2) return -1;
    return g_sort_kernel.exchange(which, std::memory_order_relaxed);
}

int sr_mark_visible(int n, const float* means3D, const float* viewmatrix, const float*, unsigned char* present, void* hip_stream) {
    if (n < 0 || (n > 0 && (!means3D || !viewmatrix || !present))) return fail("bad arguments to sr_mark_visible");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    sr::launch_mark_visible(n, means3D, viewmatrix, present, st);
    return check_hip(hipGetLastError(), "mark_visible");
}

int sr_densification_stats(int n, const float* dL_dmeans2D, const int* radii, float* grad_accum, float* denom, float* max_radii2D,
                           void* hip_stream) {
    if (n < 0) return fail("bad arguments to sr_densification_stats");
    if (n > 0 && (!dL_dmeans2D || !radii)) return fail("null pointer in sr_densification_stats");
    sr::launch_densification_stats(n, dL_dmeans2D, radii, grad_accum, denom, max_radii2D, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "densification_stats");
}

int sr_debug_layout(int n, int h, int w, long long instances, size_t* out4) {
    if (!out4 || n < 0 || h <= 0 || w <= 0 || instances < 0) return fail("bad arguments to sr_debug_layout");
    sr::Geom g; sr::Binning b;
    char* const origin = reinterpret_cast<char*>(4096);   // carve relative to a non-null base: only differences are used
    sr::carve_geom(origin, n, h, w, &g);
    sr::carve_binning(origin, instances, &b);
    out4[0] = (size_t)(reinterpret_cast<char*>(g.tile_start) - origin);
    out4[1] = (size_t)(reinterpret_cast<char*>(b.sorted_id) - origin);
    out4[2] = (size_t)(reinterpret_cast<char*>(g.total) - origin);
    out4[3] = (size_t)(reinterpret_cast<char*>(g.offsets) - origin);
    return 0;
}

int sr_debug_backward_stats(unsigned long long* out8, int reset) {
    if (!out8) return fail("null pointer in sr_debug_backward_stats");
    if (hipDeviceSynchronize() != hipSuccess) return fail("sr_debug_backward_stats: device synchronisation failed");
    return sr::backward_stats(out8, reset) ? fail("sr_debug_backward_stats: counter copy failed") : 0;
}

/* Test hook: runs the debug path of a failed launch for the given call arguments without breaking the device (writes
 * snapshot_fw.dump / snapshot_bw.dump exactly as a failing stage with view->debug set would).  Returns 0. */
int sr_debug_snapshot(const SrView* view, const SrSplats* splats, const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha,
                      int backward) {
    if (!view || !splats) return fail("null view/splats");
    g_call = CallContext{view, splats, backward ? "snapshot_bw.dump" : "snapshot_fw.dump", dL_dcolor, dL_ddepth, dL_dalpha};
    dump_snapshot(backward ? "render_backward (test hook)" : "preprocess (test hook)");
    return 0;
}

int sr_profile_enable(int on) { g_prof_on = on != 0; return 0; }

int sr_profile_collect(double* ms_sum, long long* launches) {
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    std::vector<ProfRec> open;
    for (auto& r : g_prof) {
        if (!r.ended) { open.push_back(r); continue; }   // another host thread is inside this stage right now
        float ms = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            if (ms_sum) ms_sum[r.stage] += ms;
            if (launches) launches[r.stage] += 1;
        }
        hipEventDestroy(r.a); hipEventDestroy(r.b);
    }
    g_prof.swap(open);
    return 0;
}

const char* sr_profile_stage_name(int stage) { return (stage >= 0 && stage < SR_PROFILE_STAGES) ? kStageNames[stage] : ""; }

}  // extern "C"
