// api_common.hip -- library state (device, stream, sync mode, last error) of librestir_hip.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "rs_internal.h"

namespace {
std::mutex g_errMutex;
std::string g_lastError;
rs_context g_default;                                   // what rs_init / rs_set_* configure for threads that never create a context
thread_local rs_context* t_current = nullptr;           // rs_context_set_current
thread_local rs_context* t_scoped = nullptr;            // the object's context while an entry point runs
}  // namespace

rs_context* rs_ctx() { return t_scoped ? t_scoped : (t_current ? t_current : &g_default); }

// An entry point runs with the context's device current and leaves the caller's device as it found it: the host (torch, another
// library, a second context of this one on another GPU) may call hipSetDevice between two library calls, so the device is asked
// for, not remembered.
rs_ctx_scope::rs_ctx_scope(rs_context* c) : prev(t_scoped) {
    if (c) t_scoped = c;
    const int dev = rs_ctx()->device;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); cur = -1; }
    if (cur != dev && hipSetDevice(dev) == hipSuccess) prevDevice = cur;
}
rs_ctx_scope::~rs_ctx_scope() {
    if (prevDevice >= 0) (void)hipSetDevice(prevDevice);
    t_scoped = prev;
}

int rs_fail(int code, const char* msg) {
    std::lock_guard<std::mutex> lock(g_errMutex);
    g_lastError = msg ? msg : "";
    return code;
}

int rs_check_hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return 0;
    std::string m = std::string(what ? what : "hip") + ": " + hipGetErrorString(e);
    return rs_fail((int)e, m.c_str());
}

hipStream_t rs_stream() { rs_context* c = rs_ctx(); return c->streamOverride ? c->streamOverride : c->stream; }
bool rs_sync_enabled() { return rs_ctx()->sync; }

// In asynchronous mode GBuffer::render can be deferred and launched by ReSTIRDirect together with its primary rays (the two rays
// of a pixel in one packet walk).  That saves walk work on a full frame, but the slowest tile of the launch takes longer, which
// costs on scenes whose closest-hit kernels are tails of a few long tiles: by default every rs_restir measures the
// frame period both ways once and keeps the faster (restir.hip); rs_set_side_stream(1) / (2) force it off / on.
// 0 never, 1 always (launches of at least three rounds of wave slots), 2 always (any size), 3 decided per rs_restir by measuring
int rs_fuse_mode() {
    rs_context* c = rs_ctx();
    if (c->fuseMode < 0) c->fuseMode = 3;
    return c->fuseMode;
}
bool rs_fuse_enabled() { return rs_fuse_mode() != 0; }
const rs_context* rs_stream_plan() {
    rs_context* c = rs_ctx();
    if (c->chainStreams < 0) c->chainStreams = 2;          // the defaults of rs_set_stream_plan
    if (c->smallChains < 0) c->smallChains = 1;
    if (c->shadowOnMain < 0) c->shadowOnMain = 2;
    return c;
}
int rs_ris_global_below() {
    rs_context* c = rs_ctx();
    if (c->risGlobalBelow < 0) c->risGlobalBelow = 64 * 1024;
    return c->risGlobalBelow;
}

// ---- the denoise stream ---------------------------------------------------------------------------------------------------------------
// With a filter in the loop the library stream is the one chain that links consecutive frames AND carries the most work (config 5 at
// N = 1: shadow rays 794 us + temporal 208 + spatial 481 + five a-trous levels 243 + tone map, 98 % busy while the chain streams idle at
// 51-57 %, profiles/r05_config5_strip_gpu_paced_traces.txt).  rs_set_denoise_stream(1) gives the filter -- and the tone map that reads
// its result -- auxiliary stream 0: the levels of frame f wait for phase B of f by an event and run next to the temporal / spatial passes
// of f + 1.  A fifth stream with work in flight halves the frame rate, so the chains then take turns on two streams.
int rs_chains_in_flight() {
    const rs_context* c = rs_ctx();
    const int n = rs_context::kAux - (c->ownCommStreams > 0 ? 1 : 0) - (c->denoiseMode == 1 ? 1 : 0);
    return n < 1 ? 1 : n;
}
hipStream_t rs_denoise_stream() {
    rs_context* c = rs_ctx();
    if (c->denoiseMode == 0 || c->sync) return nullptr;
    return rs_aux_stream(0);                            // (null: the auxiliary streams are switched off)
}
rs_denoise_scope::rs_denoise_scope(bool fork, bool enable) {
    c = rs_ctx();
    if (!enable || c->streamOverride) return;           // nested: already there
    const hipStream_t d = rs_denoise_stream();
    if (!d) return;
    if (!c->denoiseFork) err = rs_check_hip(hipEventCreateWithFlags(&c->denoiseFork, hipEventDisableTiming), "hipEventCreate");
    if (!err && fork) {
        err = rs_check_hip(hipEventRecord(c->denoiseFork, c->stream), "denoise stream: fork");
        if (!err) err = rs_check_hip(hipStreamWaitEvent(d, c->denoiseFork, 0), "denoise stream: fork");
    }
    if (err) return;
    c->streamOverride = d; active = true;
}
rs_denoise_scope::~rs_denoise_scope() {
    if (!active) return;
    c->denoiseUsed = true;
    c->streamOverride = nullptr;
}

namespace {
inline bool inside(const rs_context::DenoiseBuf& b, const void* p) { return (const char*)p >= b.base && (const char*)p < b.base + b.bytes; }
}
int rs_denoise_mark(const void* base, size_t bytes, bool readOnly) {
    rs_context* c = rs_ctx();
    if (!c->streamOverride || !base || bytes == 0) return 0;
    rs_context::DenoiseBuf* e = nullptr;
    for (auto& b : c->denoiseBufs) if (b.base == (const char*)base) { e = &b; break; }
    if (!e) {
        if (c->denoiseBufs.size() >= 32) {              // a caller that hands over ever new buffers: order the library stream after the oldest and reuse its entry
            e = &c->denoiseBufs[0];
            for (auto& b : c->denoiseBufs) if (!b.pending) { e = &b; break; }
            if (e->pending) RS_HIP(hipStreamWaitEvent(c->stream, e->ev, 0));
        }
        else {
            hipEvent_t ev = nullptr;
            RS_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            c->denoiseBufs.push_back({ nullptr, 0, ev, true, false });
            e = &c->denoiseBufs.back();
        }
        e->base = (const char*)base; e->bytes = 0; e->readOnly = true; e->pending = false;
    }
    e->bytes = bytes > e->bytes ? bytes : e->bytes;
    e->readOnly = e->pending ? (e->readOnly && readOnly) : readOnly;
    e->pending = true;
    RS_HIP(hipEventRecord(e->ev, c->streamOverride));
    return 0;
}
bool rs_denoise_owns(const void* p) {
    const rs_context* c = rs_ctx();
    for (const auto& b : c->denoiseBufs) if (b.pending && !b.readOnly && inside(b, p)) return true;
    return false;
}
int rs_denoise_order(const void* p, bool write) {
    rs_context* c = rs_ctx();
    if (c->denoiseBufs.empty() || c->streamOverride || !p) return 0;      // (inside a scope: in that stream's order anyway)
    for (auto& b : c->denoiseBufs) {
        if (!b.pending || !inside(b, p) || (b.readOnly && !write)) continue;
        RS_HIP(hipStreamWaitEvent(c->stream, b.ev, 0));
        b.pending = false;
    }
    return 0;
}
int rs_denoise_join() {
    rs_context* c = rs_ctx();
    hipStream_t aux[rs_context::kAux];
    rs_aux_streams_made(aux);
    if (c->streamOverride || !c->denoiseUsed || !aux[0]) return 0;    // (the streams are only ever replaced behind an rs_synchronize, which clears denoiseUsed)
    if (!c->denoiseFork) RS_HIP(hipEventCreateWithFlags(&c->denoiseFork, hipEventDisableTiming));
    RS_HIP(hipEventRecord(c->denoiseFork, aux[0]));
    RS_HIP(hipStreamWaitEvent(c->stream, c->denoiseFork, 0));
    for (auto& b : c->denoiseBufs) b.pending = false;
    return 0;
}

int rs_after_launch(const char* what) {
    RS_TRY(rs_check_hip(hipGetLastError(), what));
    if (rs_ctx()->sync) RS_TRY(rs_check_hip(hipStreamSynchronize(rs_ctx()->stream), what));
    return 0;
}

rs::CamParams rs_make_cam_params(const rs_camera* cam) {
    using namespace rs;
    CamParams c;
    c.position = ld3(cam->position);
    c.right = ld3(cam->right);
    c.up = ld3(cam->up);
    c.view = ld3(cam->view);
    c.inv0 = ld3(cam->rotationMatInv);
    c.inv1 = ld3(cam->rotationMatInv + 3);
    c.inv2 = ld3(cam->rotationMatInv + 6);
    c.width = cam->resolution[0];
    c.height = cam->resolution[1];
    c.aspect = (float)cam->resolution[0] / (float)cam->resolution[1];
    c.tanFovY = tanf(radians(cam->fov[1]));            // glm::tan(glm::radians(fov.y)), sceneStructs.h:72
    c.focalDist = cam->focalDist;
    c.lensRadius = cam->lensRadius;
    c.pixelSizeX = 1.f / (float)cam->resolution[0];
    c.pixelSizeY = 1.f / (float)cam->resolution[1];
    return c;
}

// ---- tile-split hints ---------------------------------------------------------------------------------------------------------
int rs_tile_split_threshold() {
    rs_context* c = rs_ctx();
    if (!c->tileSplitSet) { c->tileSplit = 768; c->tileSplitSet = true; }
    return c->tileSplit;
}
void rs_tile_split_free(rs_tile_split* t) {
    rs_dev_free(t->base);
    if (t->report) { (void)hipHostFree(t->report); t->report = nullptr; }
    t->bytes = 0; t->key = -1; t->rot = 0; t->numTiles = t->capacity = 0;
    t->issued = t->wake = 0; t->sleep = 0; t->lastNone = false;
}
constexpr int kTileSplitSleep = 29;
int rs_tile_split_prepare(rs_tile_split* t, long long key, int numTiles, int regularBlocks, int mode, hipStream_t st, rs::TileSplit* ts, int* helperBlocks) {
    *ts = rs::TileSplit{ nullptr, 0, 0 };
    *helperBlocks = 0;
    int threshold = rs_tile_split_threshold();
    if (threshold == 0 || numTiles <= 0 || (threshold > 0 && mode == 0)) return 0;
    const bool adaptive = threshold > 0 && mode == 2;
    bool fresh = false;
    unsigned found = 0;
    if (adaptive) {
        threshold += threshold / 3;
        // The launch with sequence number q reports what launch q - 1 found, and the first launch after a (re)start reads a stale list:
        // the first fresh report is that of launch wake + 2.  Never waited for -- the host may be a hundred frames ahead of the device
        // (bench.py enqueues all its timed frames before it waits) -- so a site whose last fresh report said "none" goes back to the
        // plain kernels after its two probing launches without waiting for their report, and a report that does name heavy tiles ends
        // that sleep when it arrives.
        if (t->report) {
            const unsigned long long rep = *reinterpret_cast<volatile unsigned long long*>(t->report);
            const unsigned seq = (unsigned)(rep >> 32);
            fresh = rep != ~0ull && seq >= t->wake + 2 && seq <= t->issued;
            found = (unsigned)rep;
            if (fresh) t->lastNone = found == 0;
        }
        if (t->sleep > 0) {
            if (fresh && found > 0) { t->sleep = 0; t->wake = t->issued; fresh = false; }
            else {
                if (--t->sleep == 0) t->wake = t->issued;
                return 0;                               // a plain launch
            }
        }
    }
    if (threshold < 0) threshold = -threshold;      // negative: for every launch, also next to other kernels (tests, measurements)
    const int capacity = std::min(rs_tile_split::kCapacity, std::max(64, regularBlocks / 2));
    key = key * 1048573 + threshold;
    const size_t hintInts = 2 + (size_t)capacity, flagOffset = (8 + 3 * hintInts) * sizeof(int), flagStride = ((size_t)numTiles + 15) & ~(size_t)15;
    const size_t bytes = flagOffset + 3 * flagStride;
    if (t->bytes < bytes) {                         // (hipFree waits for the device: nothing in flight reads the old arrays)
        rs_dev_free(t->base);
        t->bytes = 0; t->key = -1;                  // (if the allocation below fails, the next launch tries again instead of clearing a null array)
        unsigned char* p = nullptr;
        RS_TRY(rs_dev_alloc(&p, bytes));
        t->base = reinterpret_cast<int*>(p); t->bytes = bytes; t->key = -1;
    }
    if (!t->report) {
        RS_HIP(hipHostMalloc((void**)&t->report, sizeof(unsigned long long), hipHostMallocDefault));
        *t->report = ~0ull;
    }
    if (t->key != key || t->numTiles != numTiles || t->capacity != capacity) {      // another geometry: no hints
        RS_HIP(hipMemsetAsync(t->base, 0, bytes, st));
        hipLaunchKernelGGL(rs::k_tile_split_init, dim3(1), dim3(1), 0, st, t->base, capacity, threshold, numTiles, (int)flagOffset, (int)flagStride, t->report);
        t->key = key; t->rot = 0; t->numTiles = numTiles; t->capacity = capacity;
        t->wake = t->issued;                        // (the sequence numbers go on: reports of launches before this point stay behind `wake`)
    }
    t->issued = (t->issued + 1) & 0x0fffffffu;
    if (t->issued == 0) t->wake = 0;
    ts->base = t->base; ts->rot = t->rot + 3 * (int)t->issued; ts->helperBlocks = capacity;
    *helperBlocks = capacity;
    t->rot = (t->rot + 1) % 3;
    if (adaptive && ((fresh && found == 0) || (!fresh && t->lastNone && t->issued - t->wake >= 2))) t->sleep = kTileSplitSleep;
    return 0;
}

int rs_walk_counters(unsigned long long** counters) {
    rs_context* c = rs_ctx();
    if (!c->walkCount) RS_TRY(rs_dev_alloc(&c->walkCount, (size_t)kWalkSub * kWalkStride));
    RS_HIP(hipMemsetAsync(c->walkCount, 0, sizeof(unsigned long long) * kWalkSub * kWalkStride, rs_stream()));
    *counters = c->walkCount;
    return 0;
}
int rs_walk_counters_sum(unsigned long long* rays) {
    if (!rays) return 0;
    if (!rs_ctx()->walkCount) return rs_fail(RS_ERR_INVALID_ARGUMENT, "walk counters: read before any launch counted into them");
    unsigned long long h[kWalkSub * kWalkStride];
    RS_HIP(hipStreamSynchronize(rs_stream()));
    RS_HIP(hipMemcpy(h, rs_ctx()->walkCount, sizeof h, hipMemcpyDeviceToHost));
    *rays = 0;
    for (int i = 0; i < kWalkSub; i++) *rays += h[i * kWalkStride];
    return 0;
}

extern "C" {

int rs_set_tile_split(int threshold) {
    rs_ctx()->tileSplit = threshold; rs_ctx()->tileSplitSet = true;
    return 0;
}

// Test hook (include/restir_hip.h): what the report words of the objects' launch sites say (rs_tilesplit.h: written by every split
// launch, the number of listed tiles its helper blocks found in the hint they read)
int rs_debug_split_tiles(const rs_gbuffer* g, const rs_restir* r, unsigned* renderTiles, unsigned* primaryTiles) {
    rs_ctx_scope scope(g ? g->ctx : r ? r->ctx : nullptr);
    RS_TRY(rs_synchronize());
    auto listed = [](const rs_tile_split& t) {
        const unsigned long long rep = t.report ? *reinterpret_cast<volatile unsigned long long*>(t.report) : ~0ull;
        return rep == ~0ull ? 0u : (unsigned)rep;
    };
    unsigned a = 0, b = 0;
    if (g) for (const rs_tile_split& t : g->split) a = std::max(a, listed(t));
    if (r) for (const auto& perStream : r->split) for (const rs_tile_split& t : perStream) b = std::max(b, listed(t));
    if (renderTiles) *renderTiles = a;
    if (primaryTiles) *primaryTiles = b;
    return 0;
}


const char* rs_last_error(void) {
    std::lock_guard<std::mutex> lock(g_errMutex);
    static thread_local std::string copy;
    copy = g_lastError;
    return copy.c_str();
}

int rs_init(int device) {
    int n = 0;
    RS_HIP(hipGetDeviceCount(&n));
    if (n <= 0) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_init: no HIP device visible (the MI355X path has no CPU fallback)");
    if (device < 0 || device >= n) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_init: device index out of range");
    RS_HIP(hipSetDevice(device));
    g_default.device = device;
    return 0;
}

int rs_context_create(int device, rs_context** out) {
    if (!out) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_context_create: null output");
    *out = nullptr;
    int n = 0;
    RS_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_context_create: device index out of range");
    rs_context* c = new rs_context();
    c->device = device;
    *out = c;
    return 0;
}
int rs_context_destroy(rs_context* c) {
    if (!c || c == &g_default) return 0;
    {
        rs_ctx_scope scope(c);
        (void)rs_synchronize();
        rs_internal_streams_destroy(c);
        rs_dev_free(c->walkCount);
        for (auto& b : c->denoiseBufs) if (b.ev) (void)hipEventDestroy(b.ev);
        c->denoiseBufs.clear();
        if (c->denoiseFork) { (void)hipEventDestroy(c->denoiseFork); c->denoiseFork = nullptr; }
    }
    if (t_current == c) t_current = nullptr;
    delete c;
    return 0;
}
int rs_context_set_current(rs_context* c) {
    t_current = c;
    return rs_check_hip(hipSetDevice(rs_ctx()->device), "rs_context_set_current");      // the context's device becomes this thread's device

}

int rs_set_stream(void* hipStream) {
    rs_context* c = rs_ctx();
    const bool changed = (hipStream_t)hipStream != c->stream;
    if (changed) RS_TRY(rs_synchronize());              // events recorded on the old stream order the auxiliary ones
    c->stream = (hipStream_t)hipStream;
    if (changed) rs_internal_streams_invalidate(c, false);      // the library's own streams were chosen next to the old stream: chosen again on next use
    return 0;
}
int rs_set_sync(int sync) { rs_ctx()->sync = sync != 0; return 0; }
int rs_set_side_stream(int enable) {
    rs_context* c = rs_ctx();
    rs_internal_streams_set_mode(c, enable != 0);       // work already enqueued on the auxiliary streams is still joined by its consumers
    c->fuseMode = enable == 2 ? 1 : enable == 3 ? 2 : enable == 4 ? 3 : 0;      // 2 always, 3 always and at any size (tests), 4 measured
    return 0;
}
// How the asynchronous mode spreads a frame's kernels over the auxiliary streams; every value -1 = keep.
//   chainStreams  1: one stream for every frame's primary -> RIS -> shadow chain; 2: frames alternate between two (default)
//   smallChains   0 / 1: a launch below three rounds of wave slots (a strip) fuses the render with the primary rays and rotates
//                 its chains over three streams (default 1)
//   shadowOnMain  0 never / 1 always / 2 for launches that fill the chip three times over (default): the shadow rays on the library stream
int rs_set_stream_plan(int chainStreams, int smallChains, int shadowOnMain) {
    rs_context* c = rs_ctx();
    if (chainStreams > 2 || smallChains > 1 || shadowOnMain > 2 || chainStreams == 0) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_set_stream_plan: value out of range");
    (void)rs_stream_plan();                             // resolve the defaults first
    if (chainStreams >= 1) c->chainStreams = chainStreams;
    if (smallChains >= 0) c->smallChains = smallChains;
    if (shadowOnMain >= 0) c->shadowOnMain = shadowOnMain;
    return 0;
}
int rs_set_ris_table_pixels(int pixels) {
    if (pixels < 0) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_set_ris_table_pixels: negative");
    rs_ctx()->risGlobalBelow = pixels;
    return 0;
}
int rs_synchronize(void) {
    rs_ctx_scope scope(nullptr);
    RS_TRY(rs_aux_synchronize());
    RS_TRY(rs_check_hip(hipStreamSynchronize(rs_ctx()->stream), "rs_synchronize"));
    RS_TRY(rs_aux_synchronize());                       // (an auxiliary launch may have been waiting for the library stream)
    for (auto& b : rs_ctx()->denoiseBufs) b.pending = false;      // everything the denoise stream was handed has finished
    rs_ctx()->denoiseUsed = false;
    return 0;
}
// LeveledEAWFilter (rs_eaw_filter, rs_strips_eaw_filter) and an rs_copy_image_to_pbo that reads its result on a stream of the library
// (asynchronous launches only): 1 on, 0 off (default).  Their results are then ordered for the caller's stream by events -- every library
// call that is handed one of those buffers waits as needed, and rs_join_denoise_stream() / rs_synchronize() do for the caller's own work.
int rs_set_denoise_stream(int enable) {
    rs_ctx_scope scope(nullptr);
    rs_context* c = rs_ctx();
    if (enable != 0 && enable != 1) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_set_denoise_stream: 0 or 1");
    if (c->denoiseMode == enable) return 0;
    RS_TRY(rs_synchronize());
    c->denoiseMode = enable;
    return 0;
}
int rs_join_denoise_stream(void) {
    rs_ctx_scope scope(nullptr);
    return rs_denoise_join();
}

}  // extern "C"
