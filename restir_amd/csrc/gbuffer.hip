// gbuffer.hip -- GBuffer::create/destroy (src/denoiser.cu:373-403), GBuffer::render / update and the
// renderGBuffer kernel (src/gbuffer.cu:3-86).
//
// Kernel: one lane per pixel, each 64-lane wave owns an 8x8 pixel tile so that the rays of a wave
// stay coherent during the closest-hit walk (the walk is the cost; the 36 B/px of plane writes are
// coalesced in 8-pixel row segments).  HBM per pixel: write albedo 12 + normal 12 + id 4 + depth 4
// + motion 4 = 36 B; BVH node/triangle reads are data dependent and mostly served by L2 / MALL.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "rs_row_layouts.h"

using namespace rs;

// TEX: the scene has texture maps or an environment map (getTexturedMaterialAndSurface, gbuffer.cu:38,59-62)
// 8 blocks per CU: without the bound the kernel takes 100+ SGPRs and runs at 7 waves per SIMD (0.392 -> 0.370 ms at 1080p)
// MOTION: the scene tracks motion (gbuffer_store, rs_internal.h); launch_render picks the instantiation, the untracked ones are unchanged
template <bool TEX, bool SPLIT, bool MOTION>
__device__ __forceinline__ void render_gbuffer_body(const DevScene& s, const CamParams& cam, const CamParams& lastCam, const GBufWrite& g,
                                                    int y0, int y1, int tilesX, const TileSplit& ts) {
    // block = 4 waves, each an 8x8 tile; the block covers 32x8 pixels (a tile that was heavy last time: four waves of 4x4, rs_tilesplit.h)
    RS_SETPRIO(RS_PRIO_WALK);
    int x, py, tile;
    bool mine, helper;
    if (!tile_split_map<8, 8>(ts, tilesX, threadIdx.x & 63, x, py, mine, tile, helper)) return;
    const int y = y0 + py;
    const bool inside = mine && x < cam.width && y < y1;
    const int idx = y * cam.width + x;

    Ray ray = camera_center_ray(cam, x, y);
    unsigned unionNodes = 0;
    Hit h = trace_closest_packet<SPLIT>(s, ray, inside, &unionNodes);       // all 64 lanes take part in the wave's walk
    if (inside) gbuffer_store<TEX, MOTION>(s, cam, lastCam, g, idx, ray, h);
    if (SPLIT) tile_split_report(ts.base, ts.rot, tile, helper, !helper && !mine, unionNodes);
}

template <bool TEX, bool MOTION>
__global__ void __launch_bounds__(256, RS_WALK_WAVES) k_render_gbuffer(DevScene s, CamParams cam, CamParams lastCam, GBufWrite g, int y0, int y1, int tilesX) {
    render_gbuffer_body<TEX, false, MOTION>(s, cam, lastCam, g, y0, y1, tilesX, TileSplit{ nullptr, 0, 0 });
}
template <bool TEX, bool MOTION>
__global__ void __launch_bounds__(256, RS_WALK_WAVES) k_render_gbuffer_split(DevScene s, CamParams cam, CamParams lastCam, GBufWrite g, int y0, int y1, int tilesX, TileSplit ts) {
    render_gbuffer_body<TEX, true, MOTION>(s, cam, lastCam, g, y0, y1, tilesX, ts);
}

namespace {

// G-buffers that hold a render which has been requested but not launched yet.  The record keeps a pointer to the scene, so
// rs_scene_destroy launches (or drops) every pending render of the scene it is about to free (rs_gbuffer_release_scene).
std::mutex g_deferredMutex;
std::vector<const rs_gbuffer*> g_deferred;
void deferred_register(const rs_gbuffer* g) {
    std::lock_guard<std::mutex> lock(g_deferredMutex);
    if (std::find(g_deferred.begin(), g_deferred.end(), g) == g_deferred.end()) g_deferred.push_back(g);
}
void deferred_unregister(const rs_gbuffer* g) {
    std::lock_guard<std::mutex> lock(g_deferredMutex);
    g_deferred.erase(std::remove(g_deferred.begin(), g_deferred.end(), g), g_deferred.end());
}

int launch_render(const rs_gbuffer* g, const rs_scene* scene, const rs_camera* cam, const rs_camera* lastCam, int y0, int y1, hipStream_t st) {
    const int c = g->cur();
    GBufWrite w{ g->albedo[c], g->motion[c], g->normal[c], g->primId[c], g->depth[c] };
    const int tilesX = (g->width + 31) / 32, tilesY = (y1 - y0 + 7) / 8;
    TileSplit ts; int helpers = 0;
    const bool alone = st == rs_stream() && (rs_sync_enabled() || !rs_aux_stream(0));
    RS_TRY(rs_tile_split_prepare(&g->split[st == rs_stream() ? 0 : 1], (((long long)y0 << 20 | y1) << 12 | tilesX), tilesX * 4 * tilesY, tilesX * tilesY,
                                 rs_split_mode(alone, rs_launch_waves(tilesX, tilesY)), st, &ts, &helpers));
    const CamParams cp = rs_make_cam_params(cam), lp = rs_make_cam_params(lastCam);
    rs_dispatch([&](auto TEX, auto MOTION) {
        if (ts.base) hipLaunchKernelGGL((k_render_gbuffer_split<TEX(), MOTION()>), dim3(helpers + tilesX * tilesY), dim3(256), 0, st, scene->dev, cp, lp, w, y0, y1, tilesX, ts);
        else hipLaunchKernelGGL((k_render_gbuffer<TEX(), MOTION()>), dim3(tilesX * tilesY), dim3(256), 0, st, scene->dev, cp, lp, w, y0, y1, tilesX);
    }, scene->textured, scene->dev.prevVertices != nullptr);
    return 0;
}

// launches a deferred render on the auxiliary stream
int flush_deferred(const rs_gbuffer* g) {
    if (!g->deferred.valid) return 0;
    g->deferred.valid = false;
    deferred_unregister(g);
    hipStream_t aux = rs_aux_stream(0);
    if (aux) RS_TRY(rs_gbuffer_order_before_render(g, aux));
    else aux = rs_stream();                                 // (the mode was switched in between: plain launch on the library stream)
    RS_TRY(launch_render(g, g->deferred.scene, &g->deferred.cam, &g->deferred.lastCam, g->deferred.y0, g->deferred.y1, aux));
    RS_TRY(rs_check_hip(hipGetLastError(), "renderGBuffer"));
    if (aux != rs_stream()) { RS_HIP(hipEventRecord(g->doneEv, aux)); g->pending = true; }
    return 0;
}

// ---- reuse of retained planes (rs_internal.h, struct rs_gbuffer) ----
bool same_key(const rs_gbuffer::Key& a, const rs_gbuffer::Key& b) {
    return a.valid && b.valid && a.sceneId == b.sceneId && a.edits == b.edits && a.y0 == b.y0 && a.y1 == b.y1 &&
           std::memcmp(&a.cam, &b.cam, sizeof(rs_camera)) == 0 && std::memcmp(&a.lastCam, &b.lastCam, sizeof(rs_camera)) == 0;
}
// a launch that is being captured into a graph does not run now: what it would write is not there to be reused, and a request
// answered without a launch would be missing from the graph.  (The legacy default stream cannot be captured.)  An error: assume it is.
bool library_stream_capturing() {
    const hipStream_t st = rs_stream();
    if (!st) return false;
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &status) != hipSuccess) { (void)hipGetLastError(); return true; }
    return status != hipStreamCaptureStatusNone;
}
void drop_keys(rs_gbuffer* g) {
    for (rs_gbuffer::Key& k : g->key) k.valid = false;
    for (bool& b : g->posKeyed) b = false;
}

}  // namespace

void rs_gbuffer_note_write(rs_gbuffer* g, int set, int y0, int rows) {
    rs_gbuffer::Key& k = g->key[set];
    if (k.valid && rows > 0 && y0 < k.y1 && y0 + rows > k.y0) k.valid = false;
}

// Nothing that runs before the temporal pass of a frame reads the G-buffer, and the set written is not the one the previous
// frame's passes read: the render is ordered after the last readers of its set (or, for a second render without an update in
// between, after everything enqueued so far on the library stream).
int rs_gbuffer_order_before_render(const rs_gbuffer* g, hipStream_t stream) {
    if (g->deferred.rerender) {
        RS_HIP(hipEventRecord(g->forkEv, rs_stream()));
        RS_HIP(hipStreamWaitEvent(stream, g->forkEv, 0));
    }
    else if (g->useOf[g->cur()] >= 0) RS_HIP(hipStreamWaitEvent(stream, g->useEv[g->useOf[g->cur()]], 0));
    if (g->denoiseValid[g->cur()]) {                    // (five frames old by now: a wait that has long been satisfied)
        RS_HIP(hipStreamWaitEvent(stream, g->denoiseEv[g->cur()], 0));
        g->denoiseValid[g->cur()] = false;
    }
    return 0;
}

int rs_gbuffer_denoise_mark(const rs_gbuffer* g) {
    const int c = g->cur();
    if (!g->denoiseEv[c]) RS_HIP(hipEventCreateWithFlags(&g->denoiseEv[c], hipEventDisableTiming));
    RS_HIP(hipEventRecord(g->denoiseEv[c], rs_stream()));
    g->denoiseValid[c] = true;
    return 0;
}

// ReSTIRDirect has launched the deferred render itself (restir.hip k_gbuffer_primary)
void rs_gbuffer_deferred_taken(const rs_gbuffer* g) {
    g->deferred.valid = false;
    deferred_unregister(g);
}

// rs_scene_destroy: every render of `scene` that is still only recorded is launched now, while the scene's arrays exist (the
// caller then waits for all streams before freeing them), so that no G-buffer keeps a pointer to a dead scene.
int rs_gbuffer_release_scene(const rs_scene* scene) {
    std::vector<const rs_gbuffer*> mine;
    {
        std::lock_guard<std::mutex> lock(g_deferredMutex);
        for (const rs_gbuffer* g : g_deferred) if (g->deferred.valid && g->deferred.scene == scene) mine.push_back(g);
    }
    int e = 0;
    for (const rs_gbuffer* g : mine) { const int r = flush_deferred(g); if (r && !e) e = r; }
    return e;
}

// the library stream waits for a render still running on an auxiliary stream; a deferred render is launched first
int rs_gbuffer_join(const rs_gbuffer* g) {
    if (!g) return 0;
    RS_TRY(flush_deferred(g));
    if (!g->pending) return 0;
    g->pending = false;
    return rs_check_hip(hipStreamWaitEvent(rs_stream(), g->doneEv, 0), "G-buffer join");
}

extern "C" {

int rs_gbuffer_destroy(rs_gbuffer* g) {
    RS_SCOPE(g);
    if (!g) return 0;
    g->deferred.valid = false;                          // a render nobody asked the result of
    deferred_unregister(g);
    (void)rs_synchronize();                             // also a render still running on the auxiliary stream
    for (int i = 0; i < rs_gbuffer::kSets; i++) {
        rs_dev_free(g->albedo[i]); rs_dev_free(g->motion[i]); rs_dev_free(g->normal[i]); rs_dev_free(g->primId[i]); rs_dev_free(g->depth[i]);
        if (g->useEv[i]) (void)hipEventDestroy(g->useEv[i]);
        if (g->denoiseEv[i]) (void)hipEventDestroy(g->denoiseEv[i]);
    }
    if (g->forkEv) (void)hipEventDestroy(g->forkEv);
    if (g->doneEv) (void)hipEventDestroy(g->doneEv);
    for (auto& t : g->split) rs_tile_split_free(&t);
    delete g;
    return 0;
}

int rs_gbuffer_create(int width, int height, rs_gbuffer** out) {
    if (!out || width <= 0 || height <= 0) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_gbuffer_create: bad size");
    *out = nullptr;
    rs_gbuffer* g = new rs_gbuffer();
    g->ctx = rs_ctx();
    rs_ctx_scope scope(g->ctx);
    g->width = width; g->height = height;
    if (const char* e = std::getenv("RS_GBUFFER_REUSE")) g->reuse = std::atoi(e) != 0;     // A/B switch for measurements: the default of rs_gbuffer_set_reuse
    const size_t n = (size_t)width * height;
    int e = 0;
    // The reference leaves the planes uninitialised (cudaMalloc only).  They are zeroed here so that
    // first-frame reads of the "last" planes are deterministic; no reference-visible value changes.
    for (int i = 0; i < rs_gbuffer::kSets && !e; i++) {
        if (!e) e = rs_dev_alloc(&g->albedo[i], n * 3);
        if (!e) e = rs_dev_alloc(&g->motion[i], n);
        if (!e) e = rs_dev_alloc(&g->normal[i], n * 3);
        if (!e) e = rs_dev_alloc(&g->primId[i], n);
        if (!e) e = rs_dev_alloc(&g->depth[i], n);
        if (!e) e = rs_check_hip(hipMemset(g->albedo[i], 0, n * 12), "memset");
        if (!e) e = rs_check_hip(hipMemset(g->motion[i], 0, n * 4), "memset");
        if (!e) e = rs_check_hip(hipMemset(g->normal[i], 0, n * 12), "memset");
        if (!e) e = rs_check_hip(hipMemset(g->primId[i], 0, n * 4), "memset");
        if (!e) e = rs_check_hip(hipMemset(g->depth[i], 0, n * 4), "memset");
        if (!e) e = rs_check_hip(hipEventCreateWithFlags(&g->useEv[i], hipEventDisableTiming), "hipEventCreate");
    }
    if (!e) e = rs_check_hip(hipEventCreateWithFlags(&g->forkEv, hipEventDisableTiming), "hipEventCreate");
    if (!e) e = rs_check_hip(hipEventCreateWithFlags(&g->doneEv, hipEventDisableTiming), "hipEventCreate");
    // the clears above are enqueued on the default stream, which the auxiliary streams are not ordered after: finish them
    // before the first render can be launched there
    if (!e) e = rs_check_hip(hipDeviceSynchronize(), "rs_gbuffer_create");
    if (e) { rs_gbuffer_destroy(g); return e; }
    *out = g;
    return 0;
}

int rs_gbuffer_render_rows(rs_gbuffer* g, const rs_scene* scene, const rs_camera* cam, int y0, int y1) {
    RS_SCOPE(g);
    if (!g || !scene || !cam) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_gbuffer_render: null argument");
    if (cam->resolution[0] != g->width || cam->resolution[1] != g->height)
        return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_gbuffer_render: camera resolution differs from the G-buffer size");
    if (y0 < 0) y0 = 0;
    if (y1 > g->height) y1 = g->height;
    if (y1 <= y0) return 0;
    // The planes depend on the scene, the camera, lastCamera and the rows alone.  The first request of a frame whose key equals those
    // of the two previous frames' sets is answered from them: this frame's position shows the set of the frame before the previous one
    // and prev() is the previous frame's, bit for bit what a render would write and what it would leave as "last" planes.  Nothing is
    // launched, recorded or ordered.
    // A set takes a key only from the single render of its frame, and not at all while a filter may still use it on the denoise stream
    // after the library stream has moved on (rs_set_denoise_stream(1): that mode always renders) or while the stream is being captured.
    const bool first = !g->renderedSinceUpdate;
    rs_gbuffer::Key k;
    k.valid = g->reuse && first && rs_ctx()->denoiseMode != 1 && !library_stream_capturing();
    k.sceneId = scene->id; k.edits = scene->edits; k.cam = *cam; k.lastCam = g->lastCamera; k.y0 = y0; k.y1 = y1;
    const int p1 = g->pos(1), p2 = g->pos(2);
    if (k.valid && !g->deferred.valid && !g->pending && g->posKeyed[p1] && g->posKeyed[p2] && same_key(k, g->key[g->phys[p1]]) &&
        same_key(k, g->key[g->phys[p2]]) && g->phys[p1] != g->phys[p2]) {
        g->phys[g->ring] = g->phys[p2];
        g->posKeyed[g->ring] = true;
        g->renderedSinceUpdate = true;
        g->reusedFrame = true;
        g->numReused++;
        return 0;
    }
    // The set this render writes: one that no other position shows (of five sets, four other positions leave at least one).  After
    // requests answered from retained planes this position shows a set it shares with others: the render takes a free one.  (Rows
    // outside [y0, y1) are nobody's: a strip's neighbour rows are written before they are read, in every frame.)  Only a SECOND render
    // of a frame whose first request was answered from the planes builds on them: the free set receives them first.
    {
        bool shown[rs_gbuffer::kSets] = {};
        for (int q = 0; q < rs_gbuffer::kSets; q++) if (q != g->ring) shown[g->phys[q]] = true;
        const int from = g->phys[g->ring];
        if (shown[from]) {
            int to = from;
            for (int s = 0; s < rs_gbuffer::kSets; s++) if (!shown[s]) { to = s; break; }
            if (g->reusedFrame && (y0 > 0 || y1 < g->height)) {
                // on the library stream: every reader of the free set was enqueued there or has been joined to it (a filter on the denoise
                // stream: by its event); the render itself is ordered after everything enqueued so far (Deferred::rerender)
                const hipStream_t st = rs_stream();
                if (g->denoiseValid[to]) RS_HIP(hipStreamWaitEvent(st, g->denoiseEv[to], 0));
                const size_t n = (size_t)g->width * g->height;
                RS_HIP(hipMemcpyAsync(g->albedo[to], g->albedo[from], n * 12, hipMemcpyDeviceToDevice, st));
                RS_HIP(hipMemcpyAsync(g->motion[to], g->motion[from], n * 4, hipMemcpyDeviceToDevice, st));
                RS_HIP(hipMemcpyAsync(g->normal[to], g->normal[from], n * 12, hipMemcpyDeviceToDevice, st));
                RS_HIP(hipMemcpyAsync(g->primId[to], g->primId[from], n * 4, hipMemcpyDeviceToDevice, st));
                RS_HIP(hipMemcpyAsync(g->depth[to], g->depth[from], n * 4, hipMemcpyDeviceToDevice, st));
            }
            g->phys[g->ring] = to;
        }
    }
    g->key[g->cur()] = k;                                       // (a second render of a frame: no key)
    g->posKeyed[g->ring] = k.valid;
    g->reusedFrame = false;
    g->numRendered++;
    // Asynchronous mode: the render is only recorded here.  ReSTIRDirect launches it together with its primary rays (the two rays
    // of a pixel in one packet walk); any other reader of the planes launches it on the auxiliary stream first, where it is
    // ordered after the last readers of the set it writes and overlaps the other frame's passes (rs_gbuffer_join).
    const hipStream_t aux = rs_aux_stream(0);
    if (aux) {
        RS_TRY(flush_deferred(g));                          // an earlier render of this frame goes first
        g->deferred.valid = true; g->deferred.rerender = g->renderedSinceUpdate;
        g->deferred.scene = scene; g->deferred.cam = *cam; g->deferred.lastCam = g->lastCamera; g->deferred.y0 = y0; g->deferred.y1 = y1;
        deferred_register(g);
        g->renderedSinceUpdate = true;
        if (!rs_fuse_enabled()) RS_TRY(flush_deferred(g));
        return 0;
    }
    RS_TRY(rs_gbuffer_join(g));                             // an earlier render of this frame may still be on the auxiliary stream
    RS_TRY(launch_render(g, scene, cam, &g->lastCamera, y0, y1, rs_stream()));
    g->renderedSinceUpdate = true;
    return rs_after_launch("renderGBuffer");
}

int rs_gbuffer_render(rs_gbuffer* g, const rs_scene* scene, const rs_camera* cam) {
    RS_SCOPE(g);
    return rs_gbuffer_render_rows(g, scene, cam, 0, g ? g->height : 0);
}

int rs_gbuffer_update(rs_gbuffer* g, const rs_camera* cam) {
    RS_SCOPE(g);
    if (!g || !cam) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_gbuffer_update: null argument");
    RS_TRY(rs_gbuffer_join(g));                         // a render nobody consumed (possibly still deferred) belongs to the frame that ends here
    g->lastCamera = *cam;
    // the frame that read sets cur (as current) and prev (as last) has been enqueued on the library stream up to here
    const int c = g->cur(), l = g->prev();
    if (!rs_sync_enabled()) {
        const int k = g->updates % rs_gbuffer::kSets;
        RS_HIP(hipEventRecord(g->useEv[k], rs_stream()));
        g->useOf[c] = g->useOf[l] = k;
    }
    else g->useOf[c] = g->useOf[l] = -1;                // synchronous mode: those readers have finished
    if (!g->renderedSinceUpdate) g->posKeyed[g->ring] = false;   // a frame without a render: what its position shows is not "the previous frame's planes"
    g->reusedFrame = false;
    g->updates++;
    g->ring = (g->ring + 1) % rs_gbuffer::kSets;
    g->frameIdx ^= 1;
    g->renderedSinceUpdate = false;
    return 0;
}

// rows of the id / normal / depth planes, packed [id rows][normal rows][depth rows] (20 B / px: rs_row_layouts.h gbuffer_planes);
// sel 0 = the planes of the current frameIdx, 1 = the "last" planes (what findTemporalNeighbor reads).  One hipMemcpyAsync per plane.
size_t rs_gbuffer_rows_bytes(const rs_gbuffer* g, int rows) { RS_SCOPE(g); return g ? rs_rows::gbuffer_planes(nullptr, 0).bytes(g->width, rows) : 0; }

static int copy_gbuffer_rows(rs_gbuffer* g, int sel, int y0, int rows, char* buf, bool pack, const char* name) {
    if (!g || !buf || (sel != 0 && sel != 1) || y0 < 0 || rows < 0 || y0 + rows > g->height) return rs_fail(RS_ERR_INVALID_ARGUMENT, (std::string(name) + ": bad argument").c_str());
    RS_TRY(rs_gbuffer_join(g));
    rs_rows::SegList l(pack);
    rs_rows::add_rows(l, rs_rows::gbuffer_planes(g, sel ? g->prev() : g->cur()), y0, rows, buf);      // (unpacking: the set's content key hears of it there)
    RS_TRY(rs_copy::memcpy_segments(l));
    return rs_after_launch(name);
}
int rs_gbuffer_rows_pack(const rs_gbuffer* g, int sel, int y0, int rows, void* devBuffer) {
    RS_SCOPE(g);
    return copy_gbuffer_rows(const_cast<rs_gbuffer*>(g), sel, y0, rows, (char*)devBuffer, true, "rs_gbuffer_rows_pack");
}
int rs_gbuffer_rows_unpack(rs_gbuffer* g, int sel, int y0, int rows, const void* devBuffer) {
    RS_SCOPE(g);
    return copy_gbuffer_rows(g, sel, y0, rows, (char*)const_cast<void*>(devBuffer), false, "rs_gbuffer_rows_unpack");
}

int rs_gbuffer_get_view(const rs_gbuffer* g, rs_gbuffer_view* v) {
    RS_SCOPE(g);
    if (!g || !v) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_gbuffer_get_view: null argument");
    RS_TRY(rs_gbuffer_join(g));                         // the caller is about to use the planes on the library stream
    const int c = g->cur(), l = g->prev(), f = g->frameIdx;
    v->devAlbedo = g->albedo[g->latest()]; v->devMotion = g->motion[g->latest()];
    v->devNormal[f] = g->normal[c]; v->devNormal[f ^ 1] = g->normal[l];
    v->devPrimId[f] = g->primId[c]; v->devPrimId[f ^ 1] = g->primId[l];
    v->devDepth[f] = g->depth[c]; v->devDepth[f ^ 1] = g->depth[l];
    v->frameIdx = g->frameIdx; v->width = g->width; v->height = g->height;
    return 0;
}

// GBuffer::render (src/gbuffer.cu:80-86) answered from the planes the G-buffer already holds when nothing it reads has changed: on (the
// default) or off.  Switching it off also forgets what the sets hold.
int rs_gbuffer_set_reuse(rs_gbuffer* g, int on) {
    RS_SCOPE(g);
    if (!g) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_gbuffer_set_reuse: null argument");
    g->reuse = on != 0;
    if (!g->reuse) drop_keys(g);
    return 0;
}

// requests of GBuffer::render (src/gbuffer.cu:80-86) that launched the walk / that were answered from retained planes
int rs_gbuffer_reuse_stats(const rs_gbuffer* g, unsigned long long* rendered, unsigned long long* reused) {
    RS_SCOPE(g);
    if (!g) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_gbuffer_reuse_stats: null argument");
    if (rendered) *rendered = g->numRendered;
    if (reused) *reused = g->numReused;
    return 0;
}

// the caller has written planes through the pointers of rs_gbuffer_get_view: the next GBuffer::render (src/gbuffer.cu:80-86) walks again
int rs_gbuffer_invalidate(rs_gbuffer* g) {
    RS_SCOPE(g);
    if (!g) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_gbuffer_invalidate: null argument");
    drop_keys(g);
    return 0;
}

}  // extern "C"
