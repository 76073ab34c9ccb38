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
#include "kernels.h"

namespace {

thread_local std::string g_last_error;
thread_local long long g_last_longest = -1;   // longest tile list of this thread's most recent sr_forward (sr_last_longest_list)

int fail(const std::string& msg) { g_last_error = msg; return 1; }

int check_hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return 0;
    return fail(std::string(what) + ": " + hipGetErrorString(e));
}

// any of these pointers (NULL counts as aligned) off a 4-byte boundary
template <typename... P>
bool any_unaligned4(const P*... p) { return ((reinterpret_cast<uintptr_t>(p) | ...) & 3u) != 0; }

#define SR_TRY(expr) do { if (int rc_ = (expr)) return rc_; } while (0)

// ---- optional per-stage timing (HIP events on the launch stream) ----
struct ProfRec { int stage; hipEvent_t a, b; bool ended; unsigned long long serial; };
unsigned long long g_prof_serial = 0;
bool g_prof_on = false;
std::vector<ProfRec> g_prof;
std::mutex g_prof_mutex;   // host threads rendering on their own streams may record concurrently
const char* kStageNames[SR_PROFILE_STAGES] = {"preprocess", "scan", "emit", "sort_tiles", "render_forward",
                                              "render_backward", "preprocess_backward"};
struct StageTimer {
    int idx = -1; hipStream_t st;
    StageTimer(int stage, hipStream_t s) : st(s) {
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
    hipEvent_t end = nullptr;
    unsigned long long serial = 0;
    // the end event is recorded under the same mutex that sr_profile_collect holds while it walks (and destroys) the list:
    // a record whose timer is still open is left alone by the collector
    ~StageTimer() {
        if (idx < 0) return;
        std::lock_guard<std::mutex> lock(g_prof_mutex);
        for (auto& r : g_prof)
            if (r.serial == serial) { hipEventRecord(end, st); r.ended = true; break; }
    }
};

// ---- status blocks: how the instance count of a forward reaches the host ------------------------------------------------
// A pinned, COHERENT 64-byte block of host memory: k_scan_small stores the instance count and the longest list into words 0 / 1
// and then -- system-scope release stores -- the block's current sequence number into words 2 / 3.  The host polls those two
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
    auto ready = [&] { return p[2] == b.seq && p[3] == b.seq; };
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
int launch_stage2(const SrView* view, const sr::ViewK& v, const sr::SplatsK& s, const sr::Geom& g, const sr::Binning& b,
                  const sr::Image& im, float* out_color, float* out_depth, float* out_alpha, StatusBlock* hs, long long max_len,
                  long long expected_len, hipStream_t st) {
    { StageTimer t_(2, st); sr::launch_emit(v, s.N, g, b, st); }
    SR_TRY(after_launch(view, st, "emit"));
    if (hs) {
        g_counters[0].fetch_add(1, std::memory_order_relaxed);
        SR_TRY(status_block_wait(*hs, nullptr));
        max_len = (long long)hs->pinned[1];
        // the binning buffer is too small: the scatter just launched exits on its own, and nothing else of stage 2 is worth
        // launching -- the caller re-runs it with a buffer that fits (SR_NEED_CAPACITY)
        if ((long long)hs->pinned[0] > (long long)b.capacity) return 0;
    }
    { StageTimer t_(3, st); sr::launch_sort_tiles(v, g, b, max_len, expected_len, st); }
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
    SR_TRY(launch_stage2(view, c.v, c.s, c.g, c.b, c.im, out_color, out_depth, out_alpha, hs, -1, -1, c.st));  // waits inside, GPU busy
    const long long total = (long long)hs->pinned[0];
    *instances_out = total;
    g_last_longest = (long long)hs->pinned[1];
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
    return launch_stage2(view, c.v, c.s, c.g, c.b, c.im, out_color, out_depth, out_alpha, nullptr, -1, -1, c.st);
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
    StatusBlock* t = nullptr;
    SR_TRY(ticket_acquire(&t));
    int rc = launch_stage1(view, c.v, c.s, c.g, radii, t->pinned_dev, status_block_arm(*t, c.st), c.st);
    if (!rc) rc = launch_stage2(view, c.v, c.s, c.g, c.b, c.im, out_color, out_depth, out_alpha, nullptr, covered,
                                longest_list_expected >= 0 && longest_list_expected <= longest_list_hint ? longest_list_expected : -1, c.st);
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
    ticket_recycle(t);
    return 0;
}

long long sr_last_longest_list(void) { return g_last_longest; }

int sr_ticket_release(void* ticket) { return sr_ticket_wait(ticket, nullptr, nullptr); }

int sr_debug_counters(long long* out4, int reset) {
    if (!out4) return fail("null pointer in sr_debug_counters");
    for (int i = 0; i < 4; ++i) out4[i] = reset ? g_counters[i].exchange(0, std::memory_order_relaxed) : g_counters[i].load(std::memory_order_relaxed);
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

int sr_sh_forward(int n, int sh_coeffs, int sh_degree, const float* means3D, const float* shs, const float* campos,
                  float* colors, unsigned char* clamped, void* hip_stream) {
    if (n < 0 || sh_degree < 0 || sh_degree > 3 || sh_coeffs < (sh_degree + 1) * (sh_degree + 1)) return fail("bad arguments to sr_sh_forward");
    if (n > 0 && (!means3D || !shs || !campos || !colors || !clamped)) return fail("null pointer in sr_sh_forward");
    sr::launch_sh_forward(n, sh_coeffs, sh_degree, means3D, shs, campos, colors, clamped, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "sh_forward");
}

int sr_sh_forward_views(int n, int sh_coeffs, int sh_degree, int n_views, const float* means3D, const float* shs, const float* campos,
                        float* colors, float* keep, void* hip_stream) {
    if (n < 0 || n_views < 0 || sh_degree < 0 || sh_degree > 3 || sh_coeffs < (sh_degree + 1) * (sh_degree + 1)) return fail("bad arguments to sr_sh_forward_views");
    if (n > 0 && n_views > 0 && (!means3D || !shs || !campos || !colors)) return fail("null pointer in sr_sh_forward_views");
    sr::launch_sh_forward_views(n, sh_coeffs, sh_degree, n_views, means3D, shs, campos, colors, keep, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "sh_forward_views");
}

int sr_sh_backward(int n, int sh_coeffs, int sh_degree, int n_views, const float* means3D, const float* shs, const float* campos,
                   const float* dL_dcolors, float scale, float* dL_dshs, float* dL_dmeans3D, int accumulate_means, void* hip_stream) {
    if (n < 0 || n_views < 0 || sh_degree < 0 || sh_degree > 3 || sh_coeffs < (sh_degree + 1) * (sh_degree + 1)) return fail("bad arguments to sr_sh_backward");
    if (n > 0 && n_views > 0 && (!means3D || !shs || !campos || !dL_dcolors)) return fail("null pointer in sr_sh_backward");
    sr::launch_sh_backward(n, sh_coeffs, sh_degree, n_views, means3D, shs, campos, dL_dcolors, scale, dL_dshs, dL_dmeans3D, accumulate_means,
                           static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "sh_backward");
}

size_t sr_knn_workspace_bytes(int n) { return sr::knn_workspace_bytes(n); }

int sr_knn3_mean_dist2(int n, const float* points, float* mean_dist2, void* workspace, void* hip_stream) {
    if (n < 0 || (n > 0 && (!points || !mean_dist2 || !workspace))) return fail("bad arguments to sr_knn3_mean_dist2");
    sr::launch_knn3(n, points, mean_dist2, workspace, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "knn3");
}

size_t sr_knn_graph_workspace_bytes(int n, int k) { return sr::knn_graph_workspace_bytes(n, k); }

int sr_knn_graph(int n, int k, const float* points, int* nn_ix, unsigned* order, unsigned* rev_start, unsigned* rev_edges, void* workspace,
                 void* hip_stream) {
    if (n <= 0) return fail("bad arguments to sr_knn_graph: sizes must be positive");
    if (k < sr::kKnnMinK || k > sr::kKnnMaxK) return fail("bad arguments to sr_knn_graph: k must be 2 .. 8");
    if (n < k) return fail("bad arguments to sr_knn_graph: fewer points than neighbours (n < k)");
    if (n > 0x7fffffff / (3 * sr::kKnnMaxK)) return fail("too many points for sr_knn_graph");
    if (!points || !nn_ix || !order || !rev_start || !rev_edges || !workspace) return fail("null pointer in sr_knn_graph");
    sr::launch_knn_graph(n, k, points, nn_ix, order, rev_start, rev_edges, workspace, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "knn_graph");
}

size_t sr_moran_workspace_bytes(int n, int n_tensors) { return sr::moran_workspace_bytes(n, n_tensors); }

size_t sr_moran_edges_bytes(int n, int k, int channels) { return sr::moran_edges_bytes(n, k, channels); }

}  // extern "C"

namespace {

// the checks that sr_moran_forward and sr_moran_backward share; fills the kernel-side descriptions
int open_moran(const char* who, int n, int k, float eps, const float* points, const float* weight, const int* nn_ix, const unsigned* order,
               int n_tensors, const float* const* features, const int* widths, sr::MoranSource* s, sr::MoranTensors* t) {
    const std::string name(who);
    if (n <= 0) return fail("bad arguments to " + name + ": sizes must be positive");
    if ((points == nullptr) == (weight == nullptr)) return fail(name + ": points or weight (exactly one of them)");
    if (k < (points ? sr::kKnnMinK : 1) || k > sr::kKnnMaxK) return fail("bad arguments to " + name + ": k must be 2 .. 8 (1 .. 8 with weight)");
    if (points && n < k) return fail("bad arguments to " + name + ": fewer points than neighbours (n < k)");
    if (points && !nn_ix) return fail("null pointer in " + name + ": points need nn_ix");
    if (n_tensors < 1) return fail(name + ": at least one feature tensor");
    if (n_tensors > sr::kMoranMaxTensors) return fail(name + ": at most 8 feature tensors in one call");
    if (!features || !widths) return fail("null pointer in " + name);
    *s = sr::MoranSource{n, k, eps, points, weight, nn_ix, order};
    *t = sr::MoranTensors{};
    t->count = n_tensors;
    long long channels = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (widths[i] <= 0) return fail("bad arguments to " + name + ": sizes must be positive");
        if (!features[i]) return fail("null pointer in " + name);
        t->x[i] = features[i]; t->width[i] = widths[i]; t->offset[i] = (int)channels;
        channels += widths[i];
        if (channels > 0x7fffffff / sr::kKnnMaxK) return fail("too many channels for " + name);
    }
    if ((long long)n > 0x7fffffff / (3 * sr::kKnnMaxK)) return fail("too many items for " + name);
    t->channels = (int)channels;
    return 0;
}

}  // namespace

extern "C" {

int sr_moran_forward(int n, int k, float eps, const float* points, const float* weight, const int* nn_ix, const unsigned* order, int n_tensors,
                     const float* const* features, const int* widths, void* workspace, float* out, void* hip_stream) {
    sr::MoranSource s; sr::MoranTensors t;
    SR_TRY(open_moran("sr_moran_forward", n, k, eps, points, weight, nn_ix, order, n_tensors, features, widths, &s, &t));
    if (!workspace || !out) return fail("null pointer in sr_moran_forward");
    sr::launch_moran_forward(s, t, workspace, out, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "moran_forward");
}

int sr_moran_backward(int n, int k, float eps, const float* points, const float* weight, const int* nn_ix, const unsigned* order,
                      const unsigned* rev_start, const unsigned* rev_edges, int n_tensors, const float* const* features, const int* widths,
                      const float* out, const float* upstream, void* edges, float* const* dL_dfeatures, float* dL_dpoints, float* dL_dweight,
                      void* hip_stream) {
    sr::MoranSource s; sr::MoranTensors t;
    SR_TRY(open_moran("sr_moran_backward", n, k, eps, points, weight, nn_ix, order, n_tensors, features, widths, &s, &t));
    if (!upstream || !edges || !dL_dfeatures) return fail("null pointer in sr_moran_backward");
    if (dL_dpoints && !points) return fail("sr_moran_backward: dL_dpoints without points");
    if (dL_dweight && !weight) return fail("sr_moran_backward: dL_dweight without weight");
    if ((rev_start == nullptr) != (rev_edges == nullptr)) return fail("sr_moran_backward: rev_start and rev_edges go together (both or neither)");
    if (nn_ix && !rev_start) return fail("null pointer in sr_moran_backward: nn_ix needs the reverse adjacency");
    if (!nn_ix && rev_start) return fail("sr_moran_backward: a reverse adjacency without nn_ix");
    for (int i = 0; i < n_tensors; ++i) {
        t.dx[i] = dL_dfeatures[i];
        t.edge_offset[i] = t.edge_channels;
        if (t.dx[i]) t.edge_channels += t.width[i];
    }
    sr::launch_moran_backward(s, t, rev_start, rev_edges, out, upstream, edges, dL_dpoints, dL_dweight, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "moran_backward");
}

int sr_moran_weights(int n, int k, float eps, const float* points, const int* nn_ix, float* weights, void* hip_stream) {
    if (n <= 0) return fail("bad arguments to sr_moran_weights: sizes must be positive");
    if (k < sr::kKnnMinK || k > sr::kKnnMaxK) return fail("bad arguments to sr_moran_weights: k must be 2 .. 8");
    if (n < k) return fail("bad arguments to sr_moran_weights: fewer points than neighbours (n < k)");
    if (n > 0x7fffffff / (3 * sr::kKnnMaxK)) return fail("too many points for sr_moran_weights");
    if (!points || !nn_ix || !weights) return fail("null pointer in sr_moran_weights");
    sr::launch_moran_weights(sr::MoranSource{n, k, eps, points, nullptr, nn_ix, nullptr}, weights, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "moran_weights");
}

int sr_moran_weights_backward(int n, int k, float eps, const float* points, const int* nn_ix, const unsigned* rev_start, const unsigned* rev_edges,
                              const float* dL_dweights, void* edges, float* dL_dpoints, void* hip_stream) {
    if (n <= 0) return fail("bad arguments to sr_moran_weights_backward: sizes must be positive");
    if (k < sr::kKnnMinK || k > sr::kKnnMaxK) return fail("bad arguments to sr_moran_weights_backward: k must be 2 .. 8");
    if (n < k) return fail("bad arguments to sr_moran_weights_backward: fewer points than neighbours (n < k)");
    if (n > 0x7fffffff / (3 * sr::kKnnMaxK)) return fail("too many points for sr_moran_weights_backward");
    if (!points || !nn_ix || !rev_start || !rev_edges || !dL_dweights || !edges || !dL_dpoints) return fail("null pointer in sr_moran_weights_backward");
    sr::launch_moran_weights_backward(sr::MoranSource{n, k, eps, points, nullptr, nn_ix, nullptr}, rev_start, rev_edges, dL_dweights, edges,
                                      dL_dpoints, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "moran_weights_backward");
}

size_t sr_loss_workspace_bytes(int planes, int height, int width) { return sr::loss_workspace_bytes(planes, height, width); }

size_t sr_loss_maps_bytes(int planes, int height, int width) { return sr::loss_maps_bytes(planes, height, width); }

int sr_photometric_forward(int batch, int channels, int height, int width, const float* image, const float* gt, const float* alpha,
                           const float* gt_mask, float lambda_dssim, float lambda_mask, void* workspace, float* maps, float* loss,
                           float* l1, float* ssim, float* mask_l1, void* hip_stream) {
    if (batch <= 0 || channels <= 0 || height <= 0 || width <= 0) return fail("bad arguments to sr_photometric_forward: sizes must be positive");
    if (!sr::loss_shape_ok(batch, channels, height, width)) return fail("image too large for sr_photometric_forward");
    if (!image || !gt || !workspace || !loss || !l1) return fail("null pointer in sr_photometric_forward");
    if ((alpha == nullptr) != (gt_mask == nullptr)) return fail("sr_photometric_forward: alpha and gt_mask go together (both or neither)");
    if (alpha && !mask_l1) return fail("null pointer in sr_photometric_forward: mask_l1 is written when alpha is given");
    if (!alpha && lambda_mask != 0.0f) return fail("sr_photometric_forward: lambda_mask without alpha and gt_mask");
    if (!ssim && (lambda_dssim != 0.0f || maps)) return fail("sr_photometric_forward: the ssim output may be omitted only with lambda_dssim = 0 and no maps");
    sr::launch_loss_forward(batch, channels, height, width, image, gt, alpha, gt_mask, lambda_dssim, lambda_mask, workspace, maps, loss, l1,
                            ssim, mask_l1, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "photometric_forward");
}

int sr_photometric_backward(int batch, int channels, int height, int width, const float* image, const float* gt, const float* alpha,
                            const float* gt_mask, const float* maps, float w_l1, float w_ssim, float w_mask, const float* upstream,
                            int upstream_per_item, float* dL_dimage, float* dL_dalpha, void* hip_stream) {
    if (batch <= 0 || channels <= 0 || height <= 0 || width <= 0) return fail("bad arguments to sr_photometric_backward: sizes must be positive");
    if (!sr::loss_shape_ok(batch, channels, height, width)) return fail("image too large for sr_photometric_backward");
    if (!image || !gt || !upstream || !dL_dimage) return fail("null pointer in sr_photometric_backward");
    if ((alpha == nullptr) != (gt_mask == nullptr)) return fail("sr_photometric_backward: alpha and gt_mask go together (both or neither)");
    if (dL_dalpha && !alpha) return fail("sr_photometric_backward: dL_dalpha without alpha and gt_mask");
    if (w_ssim != 0.0f && !maps) return fail("sr_photometric_backward: a structural-similarity weight needs the maps of the forward");
    sr::launch_loss_backward(batch, channels, height, width, image, gt, alpha, gt_mask, w_ssim != 0.0f ? maps : nullptr, w_l1, w_ssim, w_mask,
                             upstream, upstream_per_item != 0, dL_dimage, dL_dalpha, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "photometric_backward");
}

size_t sr_metrics_workspace_bytes(int batch, int height, int width) { return sr::metrics_workspace_bytes(batch, height, width); }

int sr_image_metrics(int batch, int height, int width, const float* pred, const long long* pred_strides4, const float* gt,
                     const long long* gt_strides4, const float* mask, long long mask_item_stride, int quantize, void* workspace,
                     float* psnr, float* ssim, float* psnr_channels, unsigned char* frames, void* hip_stream) {
    if (batch <= 0 || height <= 0 || width <= 0) return fail("bad arguments to sr_image_metrics: sizes must be positive");
    if (height < 11 || width < 11) return fail("bad arguments to sr_image_metrics: the 11-tap valid window needs height and width >= 11");
    if (!sr::metrics_shape_ok(batch, height, width)) return fail("image too large for sr_image_metrics");
    if (!pred || !gt || !pred_strides4 || !gt_strides4 || !workspace || !psnr || !ssim || !psnr_channels) return fail("null pointer in sr_image_metrics");
    if (quantize != SR_QUANT_NONE && quantize != SR_QUANT_PNG && quantize != SR_QUANT_TO8B)
        return fail("bad arguments to sr_image_metrics: unknown quantisation mode (SR_QUANT_NONE, SR_QUANT_PNG, SR_QUANT_TO8B)");
    if (frames && quantize == SR_QUANT_NONE) return fail("sr_image_metrics: frames are the quantised prediction and need a quantisation mode");
    for (int k = 0; k < 4; ++k)
        if (pred_strides4[k] < 0 || gt_strides4[k] < 0) return fail("bad arguments to sr_image_metrics: negative stride");
    if (mask && mask_item_stride != 0 && mask_item_stride < (long long)height * width)
        return fail("bad arguments to sr_image_metrics: mask_item_stride must be 0 or at least height * width");
    sr::launch_image_metrics(batch, height, width, pred, pred_strides4, gt, gt_strides4, mask, mask_item_stride, quantize, workspace, psnr,
                             ssim, psnr_channels, frames, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "image_metrics");
}

int sr_adam_step(int n_jobs, const SrAdamJob* jobs, const unsigned char* visible, long long rows, void* hip_stream) {
    if (n_jobs < 0 || n_jobs > SR_ADAM_MAX_TENSORS) return fail("bad arguments to sr_adam_step: n_jobs must be 0 .. SR_ADAM_MAX_TENSORS (32)");
    if (n_jobs > 0 && !jobs) return fail("null pointer in sr_adam_step: jobs");
    if (visible && rows < 0) return fail("bad arguments to sr_adam_step: negative row count");
    bool work = false;
    for (int i = 0; i < n_jobs; ++i) {
        const SrAdamJob& j = jobs[i];
        const std::string at = " (job " + std::to_string(i) + ")";
        if (j.count < 0) return fail("bad arguments to sr_adam_step: negative element count" + at);
        if (j.count > 0x7fffffffll) return fail("too many elements for sr_adam_step: at most 2^31 - 1 in one job" + at);
        if (visible && (j.row <= 0 || j.count != rows * (long long)j.row))
            return fail("sr_adam_step: with a row mask every job needs count == rows * row" + at);
        if (j.count == 0) continue;
        if (!j.param || !j.grad || !j.exp_avg || !j.exp_avg_sq) return fail("null pointer in sr_adam_step" + at);
        if (any_unaligned4(j.param, j.grad, j.exp_avg, j.exp_avg_sq)) return fail("sr_adam_step: tensors must be 4-byte aligned" + at);
        work = true;
    }
    if (!work) return 0;
    sr::launch_adam(n_jobs, jobs, visible, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "adam_step");
}

size_t sr_splat_reg_workspace_bytes(int n_splats) { return sr::splat_reg_workspace_bytes(n_splats); }

int sr_splat_reg_forward(int n_splats, const float* means3D, const float* opacity, double lambda_norm, double lambda_norm_mean,
                         double lambda_opacity, void* workspace, float* out, void* hip_stream) {
    if (n_splats < 0) return fail("bad arguments to sr_splat_reg_forward: negative splat count");
    if (!(lambda_norm == lambda_norm) || !(lambda_norm_mean == lambda_norm_mean) || !(lambda_opacity == lambda_opacity))
        return fail("bad arguments to sr_splat_reg_forward: a weight is NaN");
    if (n_splats == 0) return 0;
    if (!workspace || !out) return fail("null pointer in sr_splat_reg_forward");
    if ((lambda_norm != 0.0 || lambda_norm_mean != 0.0) && !means3D) return fail("null pointer in sr_splat_reg_forward: means3D is read by the norm terms");
    if (lambda_opacity != 0.0 && !opacity) return fail("null pointer in sr_splat_reg_forward: opacity is read by the opacity term");
    if (any_unaligned4(means3D, opacity)) return fail("sr_splat_reg_forward: tensors must be 4-byte aligned");
    sr::launch_splat_reg_forward(n_splats, means3D, opacity, lambda_norm, lambda_norm_mean, lambda_opacity, workspace, out,
                                 static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "splat_reg_forward");
}

int sr_splat_reg_backward(int n_splats, const float* means3D, const float* opacity, double lambda_norm, double lambda_norm_mean,
                          double lambda_opacity, const float* out, const float* upstream, float* dL_dmeans3D, float* dL_dopacity,
                          void* hip_stream) {
    if (n_splats < 0) return fail("bad arguments to sr_splat_reg_backward: negative splat count");
    if (!(lambda_norm == lambda_norm) || !(lambda_norm_mean == lambda_norm_mean) || !(lambda_opacity == lambda_opacity))
        return fail("bad arguments to sr_splat_reg_backward: a weight is NaN");
    if (n_splats == 0 || (!dL_dmeans3D && !dL_dopacity)) return 0;
    if (!upstream) return fail("null pointer in sr_splat_reg_backward");
    if (dL_dmeans3D && !means3D) return fail("null pointer in sr_splat_reg_backward: dL_dmeans3D without means3D");
    if (dL_dopacity && !opacity) return fail("null pointer in sr_splat_reg_backward: dL_dopacity without opacity");
    if (dL_dmeans3D && lambda_norm_mean != 0.0 && !out) return fail("null pointer in sr_splat_reg_backward: the centred norm needs the mean in `out` of the forward");
    if (any_unaligned4(means3D, opacity, dL_dmeans3D, dL_dopacity)) return fail("sr_splat_reg_backward: tensors must be 4-byte aligned");
    sr::launch_splat_reg_backward(n_splats, means3D, opacity, lambda_norm, lambda_norm_mean, lambda_opacity, out, upstream, dL_dmeans3D,
                                  dL_dopacity, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "splat_reg_backward");
}

size_t sr_depth_l1_workspace_bytes(int batch, int height, int width) { return sr::depth_l1_workspace_bytes(batch, height, width); }

int sr_depth_l1_forward(int batch, int height, int width, const float* depth, const float* gt_depth, void* workspace, float* out,
                        void* hip_stream) {
    if (batch < 0 || height <= 0 || width <= 0) return fail("bad arguments to sr_depth_l1_forward: the image size must be positive and the batch not negative");
    if (!sr::depth_l1_shape_ok(batch, height, width)) return fail("too many items for sr_depth_l1_forward");
    if (batch == 0) return 0;
    if (!depth || !gt_depth || !workspace || !out) return fail("null pointer in sr_depth_l1_forward");
    if (any_unaligned4(depth, gt_depth)) return fail("sr_depth_l1_forward: tensors must be 4-byte aligned");
    sr::launch_depth_l1_forward(batch, height, width, depth, gt_depth, workspace, out, static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "depth_l1_forward");
}

int sr_depth_l1_backward(int batch, int height, int width, const float* depth, const float* gt_depth, const float* upstream,
                         int upstream_per_item, float* dL_ddepth, void* hip_stream) {
    if (batch < 0 || height <= 0 || width <= 0) return fail("bad arguments to sr_depth_l1_backward: the image size must be positive and the batch not negative");
    if (!sr::depth_l1_shape_ok(batch, height, width)) return fail("too many items for sr_depth_l1_backward");
    if (batch == 0) return 0;
    if (!depth || !gt_depth || !upstream || !dL_ddepth) return fail("null pointer in sr_depth_l1_backward");
    if (any_unaligned4(depth, gt_depth, dL_ddepth)) return fail("sr_depth_l1_backward: tensors must be 4-byte aligned");
    sr::launch_depth_l1_backward(batch, height, width, depth, gt_depth, upstream, upstream_per_item != 0, dL_ddepth,
                                 static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "depth_l1_backward");
}

size_t sr_densify_workspace_bytes(int n) { return sr::densify_workspace_bytes(n); }

int sr_densify_plan(int n, const float* log_scales, int scale_cols, const float* opacity_logits, const float* grad_accum,
                    const float* denom, const float* max_radii2D, float grad_threshold, float min_opacity, float extent,
                    float percent_dense, float max_screen_size, void* workspace, int* dest, long long* counts5, void* hip_stream) {
    if (n < 0 || (scale_cols != 1 && scale_cols != 3)) return fail("bad arguments to sr_densify_plan");
    if (!counts5) return fail("null counts in sr_densify_plan");
    for (int k = 0; k < 5; ++k) counts5[k] = 0;
    if (n == 0) return 0;
    if (!log_scales || !opacity_logits || !grad_accum || !denom || !workspace || !dest) return fail("null pointer in sr_densify_plan");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const sr::DensifyArgs a{grad_threshold, min_opacity, extent, percent_dense, max_screen_size};
    uint32_t* totals = nullptr;
    sr::launch_densify_plan(n, log_scales, scale_cols, opacity_logits, grad_accum, denom, max_radii2D, a, workspace, dest, &totals, st);
    SR_TRY(check_hip(hipGetLastError(), "densify_plan"));
    uint32_t host[5];
    SR_TRY(check_hip(hipMemcpyAsync(host, totals, sizeof(host), hipMemcpyDeviceToHost, st), "read densify counts"));
    SR_TRY(check_hip(hipStreamSynchronize(st), "sync after densify_plan"));
    for (int k = 0; k < 5; ++k) counts5[k] = (long long)host[k];
    return 0;
}

int sr_densify_gather(int n, int row_floats, const float* src, float* dst, const int* dest, int mode, const float* log_scales,
                      int scale_cols, const float* rotations, const float* unit_normals, void* hip_stream) {
    if (n < 0 || row_floats <= 0 || mode < 0 || mode > 3) return fail("bad arguments to sr_densify_gather");
    if (n == 0) return 0;
    if (!src || !dst || !dest) return fail("null pointer in sr_densify_gather");
    if (mode == 2 && (row_floats != 3 || !log_scales || !rotations || !unit_normals || (scale_cols != 1 && scale_cols != 3)))
        return fail("sr_densify_gather mode 2 (positions) needs [N,3] rows, log-scales, rotations and unit normals");
    sr::launch_densify_gather(n, row_floats, src, dst, dest, mode, log_scales, scale_cols, rotations, unit_normals,
                              static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "densify_gather");
}

// items of a hull call: G^3 or n_points; -1 with the message set when the pair is not acceptable
static long long hull_items(const char* name, const double* grid, int G, const void* points, long long n_points) {
    if ((grid != nullptr) == (points != nullptr)) {
        fail(std::string(name) + ": exactly one of grid and points must be given");
        return -1;
    }
    if (grid) {
        if (G < 1) { fail(std::string(name) + ": G must be at least 1"); return -1; }
        if (G > 1290) { fail(std::string(name) + ": G^3 must not exceed 2^31 - 1 (G <= 1290)"); return -1; }
        return (long long)G * G * G;
    }
    if (n_points < 0 || n_points > 2147483647LL) { fail(std::string(name) + ": n_points must be in 0 .. 2^31 - 1"); return -1; }
    return n_points;
}

size_t sr_hull_workspace_bytes(long long n_items) { return n_items < 0 || n_items > 2147483647LL ? 0 : sr::hull_workspace_bytes(n_items); }

int sr_hull_carve(int n_views, const SrHullView* views, const unsigned char* masks, long long mask_bytes, const double* grid, int G,
                  const void* points, long long n_points, int point_is_double, void* workspace, int* count_out, void* hip_stream) {
    if (n_views <= 0 || n_views > SR_HULL_MAX_VIEWS) return fail("sr_hull_carve: n_views must be in 1 .. SR_HULL_MAX_VIEWS");
    if (!views || !masks || !workspace || !count_out) return fail("null pointer in sr_hull_carve");
    const long long n = hull_items("sr_hull_carve", grid, G, points, n_points);
    if (n < 0) return 1;
    for (int k = 0; k < n_views; ++k) {
        const SrHullView& w = views[k];
        const std::string at = "sr_hull_carve: view " + std::to_string(k);
        if (w.height < 1 || w.width < 1) return fail(at + ": H and W must be at least 1");
        if (w.convention != SR_HULL_KRT && w.convention != SR_HULL_NDC) return fail(at + ": unknown pixel-mapping convention");
        if (w.outside != SR_HULL_OUTSIDE_CARVE && w.outside != SR_HULL_OUTSIDE_KEEP) return fail(at + ": unknown outside policy");
        if (w.convention == SR_HULL_KRT && (w.height == 1 || w.width == 1))
            return fail(at + ": H or W of 1 divides by zero in the krt normalisation (W - 1)");
        if (w.mask_offset < 0 || w.mask_offset + (long long)w.height * w.width > mask_bytes)
            return fail(at + ": the mask does not fit into mask_bytes");
    }
    SR_TRY(check_hip(sr::launch_hull_carve(n_views, views, masks, grid, G, points, n, point_is_double != 0, workspace, count_out,
                                           static_cast<hipStream_t>(hip_stream)), "upload of the hull view table"));
    return check_hip(hipGetLastError(), "hull_carve");
}

int sr_hull_gather(const double* grid, int G, const void* points, long long n_points, int point_is_double, const void* workspace,
                   long long capacity, int* indices_out, float* points_out, void* hip_stream) {
    const long long n = hull_items("sr_hull_gather", grid, G, points, n_points);
    if (n < 0) return 1;
    if (capacity < 0) return fail("sr_hull_gather: capacity must not be negative");
    if (!workspace) return fail("null pointer in sr_hull_gather");
    if (n == 0 || capacity == 0 || (!indices_out && !points_out)) return 0;
    sr::launch_hull_gather(grid, G, points, n, point_is_double != 0, workspace, capacity, indices_out, points_out,
                           static_cast<hipStream_t>(hip_stream));
    return check_hip(hipGetLastError(), "hull_gather");
}

static int mlp_chain_entry(const char* name, bool bf16, int n_points, int hidden_tiles, int n_ops, const SrMlpOp* ops, float negative_slope, void* hip_stream) {
    if (n_points < 0 || !ops) return fail(std::string("bad arguments to ") + name);
    if (!(negative_slope >= 0.0f && negative_slope < 1.0f)) return fail(std::string(name) + ": negative_slope must be in [0, 1)");
    if (sr::launch_mlp_chain(n_points, hidden_tiles, n_ops, ops, negative_slope, bf16, static_cast<hipStream_t>(hip_stream)))
        return fail(std::string(name) + ": unsupported op list (hidden_tiles 4 or 8, <= SR_MLP_MAX_OPS ops, even input tile counts, "
                    "16-byte aligned rows wide enough for the tiles read)");
    return check_hip(hipGetLastError(), bf16 ? "mlp_chain_bf16" : "mlp_chain");
}

static int mlp_pack_entry(const char* name, bool bf16, int n_jobs, const SrMlpPackJob* jobs, void* hip_stream) {
    if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return fail(std::string("bad arguments to ") + name);
    if (sr::launch_mlp_pack(n_jobs, jobs, bf16, static_cast<hipStream_t>(hip_stream)))
        return fail(std::string(name) + ": unsupported job (<= SR_MLP_MAX_PACK_JOBS jobs; mem_pad multiple of 32, reg_width of 16, even tile "
                    "count; counts within their padded sizes; 16-byte aligned destination)");
    return check_hip(hipGetLastError(), bf16 ? "mlp_pack_bf16" : "mlp_pack");
}

int sr_mlp_chain(int n_points, int hidden_tiles, int n_ops, const SrMlpOp* ops, float negative_slope, void* hip_stream) {
    return mlp_chain_entry("sr_mlp_chain", false, n_points, hidden_tiles, n_ops, ops, negative_slope, hip_stream);
}

int sr_mlp_chain_bf16(int n_points, int hidden_tiles, int n_ops, const SrMlpOp* ops, float negative_slope, void* hip_stream) {
    return mlp_chain_entry("sr_mlp_chain_bf16", true, n_points, hidden_tiles, n_ops, ops, negative_slope, hip_stream);
}

// `empty`: the call was valid and launched nothing (no device is needed for that)
static int mlp_group_entry(const char* name, const char* why, const char* kernel, bool empty) {
    if (why) return fail(std::string(name) + ": " + why);
    if (empty) return 0;
    return check_hip(hipGetLastError(), kernel);
}

int sr_mlp_chain_group(int n_points, int hidden_tiles, int n_nets, const SrMlpNet* nets, float negative_slope, void* hip_stream) {
    if (!(negative_slope >= 0.0f && negative_slope < 1.0f)) return fail("sr_mlp_chain_group: negative_slope must be in [0, 1)");
    return mlp_group_entry("sr_mlp_chain_group", sr::launch_mlp_chain_group(n_points, hidden_tiles, n_nets, nets, negative_slope, false,
                                                                            static_cast<hipStream_t>(hip_stream)), "mlp_chain_group", n_points == 0 || n_nets == 0);
}

int sr_mlp_chain_group_bf16(int n_points, int hidden_tiles, int n_nets, const SrMlpNet* nets, float negative_slope, void* hip_stream) {
    if (!(negative_slope >= 0.0f && negative_slope < 1.0f)) return fail("sr_mlp_chain_group_bf16: negative_slope must be in [0, 1)");
    return mlp_group_entry("sr_mlp_chain_group_bf16", sr::launch_mlp_chain_group(n_points, hidden_tiles, n_nets, nets, negative_slope, true,
                                                                                 static_cast<hipStream_t>(hip_stream)), "mlp_chain_group_bf16", n_points == 0 || n_nets == 0);
}

int sr_mlp_group_input_forward(int n_points, int n_heads, const SrMlpHeadInput* heads, int n_features, int time_multires, const float* xyz,
                               const float* features, const float* time, void* hip_stream) {
    return mlp_group_entry("sr_mlp_group_input_forward", sr::launch_mlp_group_input_forward(n_points, n_heads, heads, n_features, time_multires, xyz,
                           features, time, static_cast<hipStream_t>(hip_stream)), "mlp_group_input_forward", n_points == 0 || n_heads == 0);
}

int sr_mlp_group_input_backward(int n_points, int n_heads, const SrMlpHeadInput* heads, int n_features, const float* xyz, float* dL_dxyz,
                                float* dL_dfeatures, void* hip_stream) {
    return mlp_group_entry("sr_mlp_group_input_backward", sr::launch_mlp_group_input_backward(n_points, n_heads, heads, n_features, xyz, dL_dxyz,
                           dL_dfeatures, static_cast<hipStream_t>(hip_stream)), "mlp_group_input_backward", n_points == 0 || n_heads == 0 || (!dL_dxyz && !dL_dfeatures));
}

int sr_mlp_group_output(int n_points, int n_heads, const SrMlpHeadOutput* heads, void* hip_stream) {
    return mlp_group_entry("sr_mlp_group_output", sr::launch_mlp_group_output(n_points, n_heads, heads, static_cast<hipStream_t>(hip_stream)),
                           "mlp_group_output", n_points == 0 || n_heads == 0);
}

int sr_mlp_group_top_gradient(int n_points, int n_heads, const SrMlpHeadOutput* heads, float negative_slope, void* hip_stream) {
    if (!(negative_slope >= 0.0f && negative_slope < 1.0f)) return fail("sr_mlp_group_top_gradient: negative_slope must be in [0, 1)");
    return mlp_group_entry("sr_mlp_group_top_gradient", sr::launch_mlp_group_top_gradient(n_points, n_heads, heads, negative_slope,
                           static_cast<hipStream_t>(hip_stream)), "mlp_group_top_gradient", n_points == 0 || n_heads == 0);
}

int sr_mlp_pack(int n_jobs, const SrMlpPackJob* jobs, void* hip_stream) {
    return mlp_pack_entry("sr_mlp_pack", false, n_jobs, jobs, hip_stream);
}

int sr_mlp_pack_bf16(int n_jobs, const SrMlpPackJob* jobs, void* hip_stream) {
    return mlp_pack_entry("sr_mlp_pack_bf16", true, n_jobs, jobs, hip_stream);
}

size_t sr_mlp_weight_grad_workspace(int n_points, int n_jobs, const SrMlpGradJob* jobs) {
    if (!jobs) return 0;
    return sr::mlp_weight_grad_workspace(n_points, n_jobs, jobs);
}

int sr_mlp_weight_grad(int n_points, int n_jobs, const SrMlpGradJob* jobs, void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (!jobs || n_points < 1) return fail("bad arguments to sr_mlp_weight_grad");
    if (sr::launch_mlp_weight_grad(n_points, n_jobs, jobs, workspace, workspace_bytes, static_cast<hipStream_t>(hip_stream)))
        return fail("sr_mlp_weight_grad: unsupported job list (<= SR_MLP_MAX_GRAD_JOBS jobs, <= SR_MLP_MAX_GRAD_TASKS 64x64 blocks, "
                    "16-byte aligned rows with strides that are multiples of 4) or workspace too small");
    return check_hip(hipGetLastError(), "mlp_weight_grad");
}

int sr_mlp_input_forward(int n_points, int multires, int n_features, int time_multires, int row, const float* xyz, const float* features,
                         const float* time, float* x0, void* hip_stream) {
    if (sr::launch_mlp_input_forward(n_points, multires, n_features, time_multires, row, xyz, features, time, x0, static_cast<hipStream_t>(hip_stream)))
        return fail("bad arguments to sr_mlp_input_forward (row a multiple of 4 and >= 3 + 6 multires + n_features [+ 1 + 2 time_multires "
                    "with a time], both multires <= 16)");
    return check_hip(hipGetLastError(), "mlp_input_forward");
}

int sr_mlp_top_gradient(int n_points, int out_features, int row, const float* y, const float* dL_dy, float negative_slope, float* g,
                        void* hip_stream) {
    if (!(negative_slope >= 0.0f && negative_slope < 1.0f)) return fail("sr_mlp_top_gradient: negative_slope must be in [0, 1)");
    if (sr::launch_mlp_top_gradient(n_points, out_features, row, y, dL_dy, negative_slope, g, static_cast<hipStream_t>(hip_stream)))
        return fail("bad arguments to sr_mlp_top_gradient (row a multiple of 4 and >= out_features)");
    return check_hip(hipGetLastError(), "mlp_top_gradient");
}

int sr_mlp_input_backward(int n_points, int multires, int n_features, int row, const float* xyz, const float* dL_dx0, float* dL_dxyz,
                          float* dL_dfeatures, void* hip_stream) {
    if (sr::launch_mlp_input_backward(n_points, multires, n_features, row, xyz, dL_dx0, dL_dxyz, dL_dfeatures, static_cast<hipStream_t>(hip_stream)))
        return fail("bad arguments to sr_mlp_input_backward");
    return check_hip(hipGetLastError(), "mlp_input_backward");
}

int sr_resfield_compose(int n_jobs, const SrResFieldJob* jobs, const long long* frame, void* hip_stream) {
    if (sr::launch_resfield_compose(n_jobs, jobs, frame, static_cast<hipStream_t>(hip_stream)))
        return fail("sr_resfield_compose: unsupported job list (<= SR_RESFIELD_MAX_JOBS jobs, count a multiple of 4, 16-byte aligned "
                    "arrays, 1 <= rank <= SR_RESFIELD_MAX_RANK) or null frame pointer");
    return check_hip(hipGetLastError(), "resfield_compose");
}

size_t sr_resfield_backward_workspace(int n_jobs, const SrResFieldJob* jobs) { return sr::resfield_backward_workspace(n_jobs, jobs); }

int sr_resfield_backward(int n_jobs, const SrResFieldJob* jobs, const long long* frame, void* workspace, size_t workspace_bytes,
                         void* hip_stream) {
    if (sr::launch_resfield_backward(n_jobs, jobs, frame, workspace, workspace_bytes, static_cast<hipStream_t>(hip_stream)))
        return fail("sr_resfield_backward: unsupported job list, null frame pointer or workspace too small");
    return check_hip(hipGetLastError(), "resfield_backward");
}

size_t sr_triplane_backward_workspace(int n_points, int channels, int height, int width) {
    return sr::triplane_backward_workspace(n_points, channels, height, width);
}

int sr_triplane_forward(int n_points, int channels, int height, int width, const float* planes, float* planes_texel_major,
                        const float* points, float* out, void* hip_stream) {
    if (n_points < 0 || !planes || !planes_texel_major || (n_points > 0 && (!points || !out))) return fail("bad arguments to sr_triplane_forward");
    if (sr::launch_triplane_forward(n_points, channels, height, width, planes, planes_texel_major, points, out, static_cast<hipStream_t>(hip_stream)))
        return fail("sr_triplane_forward: channels must be a positive multiple of 4, height * width <= 2^30");
    return check_hip(hipGetLastError(), "triplane_forward");
}

int sr_triplane_backward(int n_points, int channels, int height, int width, const float* planes_texel_major, const float* points,
                         const float* dL_dout, float* dL_dplanes, float* dL_dpoints, void* workspace, void* hip_stream) {
    if (n_points < 0 || !planes_texel_major || (n_points > 0 && (!points || !dL_dout)))
        return fail("bad arguments to sr_triplane_backward");
    // the size limits are checked before the workspace: a caller that sized it with sr_triplane_backward_workspace has none
    // (0 bytes) exactly when the sizes are unsupported, and is told which limit it hit
    const int rc = sr::launch_triplane_backward(n_points, channels, height, width, planes_texel_major, points, dL_dout, dL_dplanes, dL_dpoints,
                                                workspace, static_cast<hipStream_t>(hip_stream));
    if (rc == 1) return fail("sr_triplane_backward: channels must be a positive multiple of 4 (with dL_dplanes: in 4..128), height * width <= 2^30, 12 n_points < 2^32");
    if (rc == 3) return fail("sr_triplane_backward: dL_dplanes needs a workspace of sr_triplane_backward_workspace bytes");
    if (rc) return fail("sr_triplane_backward: clearing the tile counters failed");
    return check_hip(hipGetLastError(), "triplane_backward");
}

// ---- plane generator (planegen.hip): every check happens before the first launch ---------------------------------------------
static int plane_jobs_ok(const char* who, int n_planes, const SrPlaneJob* jobs) {
    if (!jobs) return fail(std::string("null pointer in ") + who + ": jobs");
    if (n_planes < 1 || n_planes > SR_PLANE_MAX_JOBS) return fail(std::string("bad arguments to ") + who + ": n_planes must be 1 .. SR_PLANE_MAX_JOBS (8)");
    return 0;
}
#define SR_PLANE_NEED(who, cond) do { if (!(cond)) return fail(std::string("null pointer in ") + who + ", job " + std::to_string(i_) + ": needs " #cond); } while (0)

size_t sr_groupnorm_stats_workspace(int n_planes, int channels, int groups, int height, int width) {
    if (n_planes < 1 || n_planes > SR_PLANE_MAX_JOBS || !sr::plane_gn_shape_ok(channels, groups, height, width)) return 0;
    return sr::gn_stats_workspace(n_planes, channels, groups, height, width);
}

int sr_groupnorm_stats(int n_planes, const SrPlaneJob* jobs, int channels, int groups, int height, int width, float eps, void* workspace,
                       void* hip_stream) {
    SR_TRY(plane_jobs_ok("sr_groupnorm_stats", n_planes, jobs));
    if (!sr::plane_gn_shape_ok(channels, groups, height, width))
        return fail("sr_groupnorm_stats: channels in 1..64, groups must divide channels, height * width < 2^24");
    if (!workspace) return fail("null pointer in sr_groupnorm_stats: workspace");
    for (int i_ = 0; i_ < n_planes; ++i_) { const SrPlaneJob& j = jobs[i_]; SR_PLANE_NEED("sr_groupnorm_stats", j.x && j.stats); }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(0, st); sr::launch_gn_stats_partial(n_planes, jobs, channels, groups, height, width, workspace, st); }
    { StageTimer t_(0, st); sr::launch_gn_stats_final(n_planes, jobs, channels, groups, height, width, eps, workspace, st); }
    return check_hip(hipGetLastError(), "groupnorm_stats");
}

static int conv_shape_check(const char* who, int cin, int cout, int h_in, int w_in, int groups, int flags) {
    if (!sr::plane_conv_shape_ok(cin, cout, h_in, w_in, flags))
        return fail(std::string(who) + ": cin and cout must be multiples of 8 in 8..64, the output below 2^24 pixels, flags SR_CONV_* bits");
    if ((flags & SR_CONV_PROLOGUE) && (groups < 1 || cin % groups != 0)) return fail(std::string(who) + ": groups must divide cin");
    return 0;
}

int sr_conv3x3_forward(int n_planes, const SrPlaneJob* jobs, int cin, int cout, int h_in, int w_in, int groups, int flags, void* hip_stream) {
    SR_TRY(plane_jobs_ok("sr_conv3x3_forward", n_planes, jobs));
    SR_TRY(conv_shape_check("sr_conv3x3_forward", cin, cout, h_in, w_in, groups, flags));
    for (int i_ = 0; i_ < n_planes; ++i_) {
        const SrPlaneJob& j = jobs[i_];
        SR_PLANE_NEED("sr_conv3x3_forward", j.x && j.weight && j.out);
        if (flags & SR_CONV_PROLOGUE) SR_PLANE_NEED("sr_conv3x3_forward", j.gamma && j.beta && j.stats);
        if (flags & SR_CONV_RESIDUAL) SR_PLANE_NEED("sr_conv3x3_forward", j.residual);
        if (flags & SR_CONV_SILU_OUT) SR_PLANE_NEED("sr_conv3x3_forward", j.pre);
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(0, st); sr::launch_conv3x3_forward(n_planes, jobs, cin, cout, h_in, w_in, groups, flags, st); }
    return check_hip(hipGetLastError(), "conv3x3_forward");
}

int sr_conv3x3_backward_data(int n_planes, const SrPlaneJob* jobs, int cin, int cout, int h_in, int w_in, int flags, void* hip_stream) {
    SR_TRY(plane_jobs_ok("sr_conv3x3_backward_data", n_planes, jobs));
    SR_TRY(conv_shape_check("sr_conv3x3_backward_data", cin, cout, h_in, w_in, 1, flags & ~SR_CONV_PROLOGUE));
    for (int i_ = 0; i_ < n_planes; ++i_) {
        const SrPlaneJob& j = jobs[i_];
        SR_PLANE_NEED("sr_conv3x3_backward_data", j.dy && j.weight && j.dx);
        if (flags & SR_CONV_SILU_OUT) SR_PLANE_NEED("sr_conv3x3_backward_data", j.pre);
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(6, st); sr::launch_conv3x3_backward_data(n_planes, jobs, cin, cout, h_in, w_in, flags, st); }
    return check_hip(hipGetLastError(), "conv3x3_backward_data");
}

size_t sr_groupnorm_silu_backward_workspace(int n_planes, int channels, int height, int width) {
    if (n_planes < 1 || n_planes > SR_PLANE_MAX_JOBS || !sr::plane_gn_shape_ok(channels, 1, height, width)) return 0;
    return sr::gn_silu_backward_workspace(n_planes, channels, height, width);
}

int sr_groupnorm_silu_backward(int n_planes, const SrPlaneJob* jobs, int channels, int groups, int height, int width, float eps,
                               void* workspace, void* hip_stream) {
    SR_TRY(plane_jobs_ok("sr_groupnorm_silu_backward", n_planes, jobs));
    if (!sr::plane_gn_shape_ok(channels, groups, height, width))
        return fail("sr_groupnorm_silu_backward: channels in 1..64, groups must divide channels, height * width < 2^24");
    if (!workspace) return fail("null pointer in sr_groupnorm_silu_backward: workspace");
    for (int i_ = 0; i_ < n_planes; ++i_) {
        const SrPlaneJob& j = jobs[i_];
        SR_PLANE_NEED("sr_groupnorm_silu_backward", j.dx && j.x && j.gamma && j.beta && j.stats && j.dx_out && j.dgamma && j.dbeta);
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(6, st); sr::launch_gn_silu_backward_partial(n_planes, jobs, channels, groups, height, width, eps, workspace, st); }
    { StageTimer t_(6, st); sr::launch_gn_silu_backward_apply(n_planes, jobs, channels, groups, height, width, eps, workspace, st); }
    return check_hip(hipGetLastError(), "groupnorm_silu_backward");
}

size_t sr_conv3x3_weight_grad_workspace(int n_planes, int cin, int cout, int h_in, int w_in, int flags) {
    if (n_planes < 1 || n_planes > SR_PLANE_MAX_JOBS || !sr::plane_conv_shape_ok(cin, cout, h_in, w_in, flags)) return 0;
    return sr::conv3x3_weight_grad_workspace(n_planes, cin, cout, h_in, w_in, flags);
}

int sr_conv3x3_weight_grad(int n_planes, const SrPlaneJob* jobs, int cin, int cout, int h_in, int w_in, int groups, int flags, void* workspace,
                           void* hip_stream) {
    SR_TRY(plane_jobs_ok("sr_conv3x3_weight_grad", n_planes, jobs));
    SR_TRY(conv_shape_check("sr_conv3x3_weight_grad", cin, cout, h_in, w_in, groups, flags));
    if (!workspace) return fail("null pointer in sr_conv3x3_weight_grad: workspace");
    for (int i_ = 0; i_ < n_planes; ++i_) {
        const SrPlaneJob& j = jobs[i_];
        SR_PLANE_NEED("sr_conv3x3_weight_grad", j.dy && j.x && j.dweight);
        if (flags & SR_CONV_PROLOGUE) SR_PLANE_NEED("sr_conv3x3_weight_grad", j.gamma && j.beta && j.stats);
        if (flags & SR_CONV_SILU_OUT) SR_PLANE_NEED("sr_conv3x3_weight_grad", j.pre);
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(6, st); sr::launch_conv3x3_wgrad_partial(n_planes, jobs, cin, cout, h_in, w_in, groups, flags, workspace, st); }
    { StageTimer t_(6, st); sr::launch_conv3x3_wgrad_reduce(n_planes, jobs, cin, cout, h_in, w_in, flags, workspace, st); }
    return check_hip(hipGetLastError(), "conv3x3_weight_grad");
}

// ---- the flow head of the deform network (flow_head.hip) -----------------------------------------------------------------------
static int flow_head_check(const char* who, int model, long long n_points, int width, int n_basis, int n_branches, const SrFlowBranch* branches,
                           bool need_bias) {
    if (const char* why = sr::flow_head_shape_error(model, n_points, width, n_basis)) return fail(std::string(who) + ": " + why);
    if (const char* why = sr::flow_head_branch_error(model, n_basis, n_branches, branches)) return fail(std::string(who) + ": " + why);
    for (int b = 0; b < n_branches; ++b) {
        if (!branches[b].weight || (need_bias && !branches[b].bias)) return fail(std::string("null pointer in ") + who + ": a branch's weight or bias");
        if ((reinterpret_cast<uintptr_t>(branches[b].weight) & 15u) || (reinterpret_cast<uintptr_t>(branches[b].bias) & 3u))
            return fail(std::string(who) + ": branch weights must be 16-byte aligned, biases 4-byte");
    }
    return 0;
}

size_t sr_flow_head_saved_bytes(int model, long long n_points, int width, int n_basis) {
    return sr::flow_head_shape_error(model, n_points, width, n_basis) ? 0 : sr::flow_head_saved_bytes(model, n_points, n_basis);
}

size_t sr_flow_head_workspace_bytes(int model, long long n_points, int width, int n_basis) {
    return sr::flow_head_shape_error(model, n_points, width, n_basis) ? 0 : sr::flow_head_workspace_bytes(model, n_points, n_basis);
}

int sr_flow_head_dz_row(int model, int n_basis) { return sr::flow_head_dz_row(model, n_basis); }

int sr_flow_head_forward(int model, long long n_points, int width, int n_basis, int n_branches, const SrFlowBranch* branches,
                         const float* hidden, const float* pts, const float* bases, float* means3D, float* flow, void* saved,
                         void* hip_stream) {
    SR_TRY(flow_head_check("sr_flow_head_forward", model, n_points, width, n_basis, n_branches, branches, true));
    if (n_points == 0) return 0;
    if (!hidden || !pts || !means3D || !flow) return fail("null pointer in sr_flow_head_forward");
    if (model == SR_FLOW_DCT && !bases) return fail("null pointer in sr_flow_head_forward: the DCT model reads bases");
    if ((reinterpret_cast<uintptr_t>(hidden) & 15u) || (model == SR_FLOW_SE3 && (reinterpret_cast<uintptr_t>(flow) & 15u)) ||
        (reinterpret_cast<uintptr_t>(saved) & 7u) || any_unaligned4(pts, bases, means3D, flow))
        return fail("sr_flow_head_forward: hidden (and the 4x4 flow) must be 16-byte aligned, saved 8-byte, the others 4-byte");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(0, st); sr::launch_flow_head_forward(model, n_points, width, n_basis, n_branches, branches, hidden, pts, bases, means3D, flow, saved, st); }
    return check_hip(hipGetLastError(), "flow_head_forward");
}

int sr_flow_head_backward(int model, long long n_points, int width, int n_basis, int n_branches, const SrFlowBranch* branches,
                          const float* pts, const float* bases, const void* saved, const float* dL_dmeans3D, const float* dL_dflow,
                          float* dL_dpts, float* dL_dz, float* dL_dhidden, void* workspace, void* hip_stream) {
    SR_TRY(flow_head_check("sr_flow_head_backward", model, n_points, width, n_basis, n_branches, branches, false));
    if (n_points == 0) return 0;
    if (!pts || !saved || !dL_dmeans3D || !dL_dz || !workspace) return fail("null pointer in sr_flow_head_backward");
    if (model == SR_FLOW_DCT && !bases) return fail("null pointer in sr_flow_head_backward: the DCT model reads bases");
    if ((reinterpret_cast<uintptr_t>(dL_dz) & 15u) || (reinterpret_cast<uintptr_t>(dL_dhidden) & 15u) || (reinterpret_cast<uintptr_t>(saved) & 7u) ||
        (reinterpret_cast<uintptr_t>(workspace) & 7u) || any_unaligned4(pts, bases, dL_dmeans3D, dL_dflow, dL_dpts))
        return fail("sr_flow_head_backward: dL_dz and dL_dhidden must be 16-byte aligned, saved and workspace 8-byte, the others 4-byte");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(6, st); sr::launch_flow_head_backward(model, n_points, width, n_basis, n_branches, branches, pts, bases, saved, dL_dmeans3D, dL_dflow,
                                                          dL_dpts, dL_dz, dL_dhidden, workspace, st); }
    return check_hip(hipGetLastError(), "flow_head_backward");
}

// ---- the view-dependent colour head (view_color.hip) ------------------------------------------------------------------------------
size_t sr_view_color_saved_bytes(long long n_points, int width, int n_views) {
    return sr::view_color_shape_error(SR_VIEW_FROM_CAMERAS, n_points, width, n_views) ? 0 : sr::view_color_saved_bytes(n_points);
}

size_t sr_view_color_workspace_bytes(long long n_points, int width, int n_views) {
    return sr::view_color_shape_error(SR_VIEW_FROM_CAMERAS, n_points, width, n_views) ? 0 : sr::view_color_workspace_bytes(n_points);
}

int sr_view_color_forward(int mode, long long n_points, int width, int n_views, const float* feature, const float* means3D,
                          const float* campos_or_dirs, const float* weight, const float* bias, float* colours, void* saved,
                          void* hip_stream) {
    if (const char* why = sr::view_color_shape_error(mode, n_points, width, n_views)) return fail(std::string("sr_view_color_forward: ") + why);
    if (n_points == 0) return 0;
    if (!feature || !campos_or_dirs || !weight || !bias || !colours) return fail("null pointer in sr_view_color_forward");
    if (mode == SR_VIEW_FROM_CAMERAS && !means3D) return fail("null pointer in sr_view_color_forward: the camera mode reads means3D");
    if (((reinterpret_cast<uintptr_t>(feature) | reinterpret_cast<uintptr_t>(weight)) & 15u) || (reinterpret_cast<uintptr_t>(saved) & 7u) ||
        any_unaligned4(means3D, campos_or_dirs, bias, colours))
        return fail("sr_view_color_forward: feature and weight must be 16-byte aligned, saved 8-byte, the others 4-byte");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(0, st); sr::launch_view_color_forward(mode, n_points, width, n_views, feature, means3D, campos_or_dirs, weight, bias, colours, saved, st); }
    return check_hip(hipGetLastError(), "view_color_forward");
}

int sr_view_color_backward(int mode, long long n_points, int width, int n_views, const float* means3D, const float* campos_or_dirs,
                           const float* weight, const void* saved, const float* dL_dcolours, float* dL_dfeature, float* dL_dpos,
                           float* dL_dzsum, void* workspace, void* hip_stream) {
    if (const char* why = sr::view_color_shape_error(mode, n_points, width, n_views)) return fail(std::string("sr_view_color_backward: ") + why);
    if (n_points == 0) return 0;
    if (!campos_or_dirs || !weight || !saved || !dL_dcolours || !dL_dzsum || !workspace) return fail("null pointer in sr_view_color_backward");
    if (mode == SR_VIEW_FROM_CAMERAS && !means3D) return fail("null pointer in sr_view_color_backward: the camera mode reads means3D");
    if (((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(dL_dfeature) | reinterpret_cast<uintptr_t>(dL_dzsum)) & 15u) ||
        ((reinterpret_cast<uintptr_t>(saved) | reinterpret_cast<uintptr_t>(workspace)) & 7u) || any_unaligned4(means3D, campos_or_dirs, dL_dcolours, dL_dpos))
        return fail("sr_view_color_backward: weight, dL_dfeature and dL_dzsum must be 16-byte aligned, saved and workspace 8-byte, the others 4-byte");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(6, st); sr::launch_view_color_backward(mode, n_points, width, n_views, means3D, campos_or_dirs, weight, saved, dL_dcolours, dL_dfeature,
                                                           dL_dpos, dL_dzsum, workspace, st); }
    return check_hip(hipGetLastError(), "view_color_backward");
}

// ---- the generator's attention layer (attention.hip) ---------------------------------------------------------------------------
static int attention_check(const char* who, int n_planes, const SrAttentionJob* jobs, int channels, int groups, int height, int width) {
    if (!jobs) return fail(std::string("null pointer in ") + who + ": jobs");
    if (n_planes < 1 || n_planes > SR_PLANE_MAX_JOBS) return fail(std::string("bad arguments to ") + who + ": n_planes must be 1 .. SR_PLANE_MAX_JOBS (8)");
    if (const char* why = sr::attention_shape_error(channels, groups, height, width)) return fail(std::string(who) + ": " + why);
    return 0;
}

size_t sr_attention_saved_bytes(int n_planes, int channels, int groups, int height, int width) {
    if (n_planes < 1 || n_planes > SR_PLANE_MAX_JOBS || sr::attention_shape_error(channels, groups, height, width)) return 0;
    return sr::attention_saved_bytes(n_planes, channels, groups, height, width);
}

size_t sr_attention_backward_workspace(int n_planes, int channels, int groups, int height, int width) {
    if (n_planes < 1 || n_planes > SR_PLANE_MAX_JOBS || sr::attention_shape_error(channels, groups, height, width)) return 0;
    return sr::attention_backward_workspace(n_planes, channels, height, width);
}

int sr_attention_forward(int n_planes, const SrAttentionJob* jobs, int channels, int groups, int height, int width, float eps,
                         void* hip_stream) {
    SR_TRY(attention_check("sr_attention_forward", n_planes, jobs, channels, groups, height, width));
    for (int i_ = 0; i_ < n_planes; ++i_) {
        const SrAttentionJob& j = jobs[i_];
        SR_PLANE_NEED("sr_attention_forward", j.x && j.gamma && j.beta && j.stats && j.wq && j.bq && j.wk && j.bk && j.wv && j.bv && j.wo && j.bo &&
                      j.out && j.saved);
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    { StageTimer t_(0, st); sr::launch_attention_stats(n_planes, jobs, channels, groups, height, width, eps, st); }
    { StageTimer t_(0, st); sr::launch_attention_qkv(n_planes, jobs, channels, groups, height, width, eps, st); }
    { StageTimer t_(0, st); sr::launch_attention_softmax(n_planes, jobs, channels, groups, height, width, eps, st); }
    return check_hip(hipGetLastError(), "attention_forward");
}

int sr_attention_backward(int n_planes, const SrAttentionJob* jobs, int channels, int groups, int height, int width, float eps,
                          void* workspace, void* hip_stream) {
    SR_TRY(attention_check("sr_attention_backward", n_planes, jobs, channels, groups, height, width));
    if (!workspace) return fail("null pointer in sr_attention_backward: workspace");
    for (int i_ = 0; i_ < n_planes; ++i_) {
        const SrAttentionJob& j = jobs[i_];
        SR_PLANE_NEED("sr_attention_backward", j.x && j.gamma && j.beta && j.wq && j.wk && j.wv && j.wo && j.saved && j.dy && j.dx);
        SR_PLANE_NEED("sr_attention_backward", j.dgamma && j.dbeta && j.dwq && j.dbq && j.dwk && j.dbk && j.dwv && j.dbv && j.dwo && j.dbo);
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    for (int step = 0; step < sr::kAttentionBackwardSteps; ++step) {
        StageTimer t_(6, st);
        sr::launch_attention_backward(step, n_planes, jobs, channels, groups, height, width, eps, workspace, st);
    }
    return check_hip(hipGetLastError(), "attention_backward");
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
