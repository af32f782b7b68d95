// rs_internal.h -- host-side objects behind the opaque handles of include/restir_hip.h.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#ifndef RS_AUX_STREAMS
#define RS_AUX_STREAMS 3
#endif
#ifndef RS_SPLIT_SMALL_ROUNDS
#define RS_SPLIT_SMALL_ROUNDS 3
#endif
#include "rs_frame_plan.h"
#include "rs_cut_plan.h"
#include "rs_stream_choice.h"
#ifndef RS_GBUF_SETS
#define RS_GBUF_SETS (RS_AUX_STREAMS + 2)
#endif
#ifndef RS_SURF_SETS
#define RS_SURF_SETS (RS_AUX_STREAMS + 1)
#endif
#include <vector>

#include "rs_scene.h"
#include "rs_geometry_plan.h"
#include "rs_revalidate_plan.h"
#include "rs_walk.h"
#include "rs_bsdf.h"
#include "rs_tilesplit.h"

// ---- contexts ----------------------------------------------------------------------------------
// What used to be process-wide settings: the device, the stream the library enqueues on, synchronous / asynchronous
// launches, the auxiliary streams of the asynchronous mode and how GBuffer::render is launched.  Every object
// (scene, G-buffer, reservoirs, filters, strip driver) belongs to the context that was current in its thread when it
// was created, and every entry point that takes an object runs under that object's context (rs_ctx_scope), so two
// contexts -- two host threads, two devices, two streams, a synchronous and an asynchronous caller -- do not see each
// other's settings.  A thread that never asks for one uses the default context (what rs_init / rs_set_* configure).
struct rs_context {
    static constexpr int kAux = RS_AUX_STREAMS;   // 0: GBuffer::render, 1 + k: the primary -> RIS -> shadow chain of every second frame (rs_restir::kChains); small launches: all of them chains in turn
    int device = 0;
    hipStream_t stream = nullptr;
    bool sync = true;
    rs_internal_streams streams;          // the library's own streams, which were chosen and which are kept (internal_streams.hip owns every field)
    int risGlobalBelow = -1;              // launches of fewer pixels read the RIS light table from global memory (rs_set_ris_table_pixels): -1 = the default, 64 Ki
    int fuseMode = -1;                    // deferred G-buffer render walked with the primary rays: -1 = not resolved yet (rs_set_side_stream; default: measured per rs_restir)
    int chainStreams = -1, smallChains = -1, shadowOnMain = -1;   // rs_set_stream_plan; -1: not resolved yet (environment or default)
    int ownCommStreams = 0;               // strip drivers of this context that keep a transfer stream of their own busy (rs_strips_set_comm_stream(s, 1))
    // The denoise stream (rs_set_denoise_stream): LeveledEAWFilter of frame f -- and the tone map that reads its result -- on auxiliary
    // stream 0, ordered after phase B of f by an event, next to the temporal / spatial passes of frame f + 1 on the library stream.  Four
    // streams that hand events to each other is what the device runs side by side, so the chains then take turns on
    // TWO streams (rs_chains_in_flight).  What that stream writes is ordered for the library stream by events, not by stream order:
    // denoiseBufs lists those buffers with the event that covers their last use there, and every entry point that is handed a raw image
    // pointer asks rs_denoise_order() first.
    int denoiseMode = 0;                  // 0: filters run on the library stream; 1: on auxiliary stream 0, the chains on two streams (asynchronous mode only)
    hipStream_t streamOverride = nullptr; // inside an rs_denoise_scope: what rs_stream() returns
    struct DenoiseBuf { const char* base; size_t bytes; hipEvent_t ev; bool readOnly, pending; };
    std::vector<DenoiseBuf> denoiseBufs;  // (an entry keeps its event for the buffer's next use)
    bool denoiseUsed = false;             // the denoise stream has carried work since the last rs_synchronize
    hipEvent_t denoiseFork = nullptr;     // library stream -> denoise stream
    unsigned long long* walkCount = nullptr;    // BVH-walk counters of the path kernels (gi.hip, pathtrace.hip): kWalkSub partial counters, rs_walk_counters
    int tileSplit = 0; bool tileSplitSet = false;   // union nodes from which a tile of a closest-hit kernel is traced by four waves (rs_tilesplit.h): rs_set_tile_split, default 768; 0 off; negative: |value|, also for launches that overlap others
};
rs_context* rs_ctx();                                   // the context this thread's library code runs under right now
struct rs_ctx_scope {                                   // entry points: run under the context of the object they were handed
    rs_context* prev;
    int prevDevice = -1;                                // the caller's device, restored on exit when the scope had to change it
    explicit rs_ctx_scope(rs_context* c);               // null: keep the thread's current context
    ~rs_ctx_scope();
};
#define RS_SCOPE(obj) rs_ctx_scope rs_scope_guard_((obj) ? (obj)->ctx : nullptr)

// ---- error plumbing --------------------------------------------------------------------------
int rs_fail(int code, const char* msg);                 // records msg, returns code
int rs_check_hip(hipError_t e, const char* what);       // 0 on success
hipStream_t rs_stream();
bool rs_sync_enabled();
// after a launch: hipGetLastError (+ stream sync when sync mode is on), like checkCUDAError
int rs_after_launch(const char* what);
// auxiliary streams of the asynchronous mode (internal_streams.hip): 0 = GBuffer::render, 1 + k = primary rays + RIS + shadow rays of every
// kChains-th frame; nullptr = not in use.  The first call after a change chooses them (about 25 ms); a call that finds them chosen only reads.
hipStream_t rs_aux_stream(int i);
int rs_aux_streams_made(hipStream_t out[rs_context::kAux]);   // the streams that exist right now, by index (null: not made); returns how many.  Makes and measures nothing
int rs_aux_synchronize();
void rs_internal_streams_invalidate(rs_context* c, bool forget);   // the streams are chosen again on next use (another caller stream or preference); forget: the kept choices go as well
void rs_internal_streams_set_mode(rs_context* c, bool on);   // rs_set_side_stream
void rs_internal_streams_destroy(rs_context* c);        // rs_context_destroy, after an rs_synchronize: the current and the kept streams
int rs_chains_in_flight();                             // how many auxiliary streams the frames' chains take in turn: 3, less one per other stream of the context with work in flight (a strip driver's transfer stream, the denoise stream)
// ---- the denoise stream (api_common.hip) ----
hipStream_t rs_denoise_stream();                       // auxiliary stream 0 when rs_set_denoise_stream(1) is in force and launches are asynchronous, else null
// Work for the denoise stream: the constructor orders that stream after everything enqueued on the library stream so far (`fork`) and makes
// rs_stream() return it; the destructor restores the library stream.  Inactive (everything stays on the library stream) when there is no
// denoise stream.
struct rs_denoise_scope {
    rs_context* c = nullptr;
    hipStream_t prev = nullptr;
    bool active = false;
    int err = 0;
    explicit rs_denoise_scope(bool fork, bool enable = true);
    ~rs_denoise_scope();
};
int rs_denoise_mark(const void* base, size_t bytes, bool readOnly);   // inside a scope: `base` is in use on the denoise stream up to here (readOnly: only read there)
int rs_denoise_order(const void* p, bool write = true);               // the library stream waits for the denoise stream's last use of the buffer p points into (no-op for buffers it never touched; reads do not wait for reads)
bool rs_denoise_owns(const void* p);                                  // p points into a buffer the denoise stream has written and the library stream has not been ordered after
int rs_denoise_join();                                                // the library stream waits for everything enqueued on the denoise stream

#define RS_TRY(expr)                                       \
    do {                                                   \
        int _rs_e = (expr);                                \
        if (_rs_e != 0) return _rs_e;                      \
    } while (0)
#define RS_HIP(expr) RS_TRY(rs_check_hip((expr), #expr))

template <typename T>
static inline int rs_dev_alloc(T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    return rs_check_hip(hipMalloc((void**)p, sizeof(T) * count), "hipMalloc");
}
template <typename T>
static inline void rs_dev_free(T*& p) {
    if (p) { (void)hipFree((void*)p); p = nullptr; }
}
// a host table as a device array of its own
template <typename T>
int upload(T** dst, const std::vector<T>& src) {
    RS_TRY(rs_dev_alloc(dst, src.size()));
    if (!src.empty()) RS_HIP(hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
    return 0;
}

// Run-time booleans as template arguments: f is called once, with a std::true_type / std::false_type per boolean --
//   rs_dispatch([&](auto TEX, auto SOBOL) { hipLaunchKernelGGL((kernel<TEX(), SOBOL()>), grid, block, 0, stream, args...); }, tex, sobol);
template <typename F>
inline void rs_dispatch(F&& f) { f(); }
template <typename F, typename... Bools>
inline void rs_dispatch(F&& f, bool b, Bools... rest) {
    if (b) rs_dispatch([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
    else rs_dispatch([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}
// The Sobol branch indexes its table by the caller's looper (State::looper, kept below SobolSampleNum by the reference's
// `(looper + 1) % SobolSampleNum`, restir.cu:441-445): a looper outside the table is refused instead of read.
int rs_check_looper(const struct rs_scene* scene, int looper, const char* what);
// The current context's walk counters (api_common.hip).  A path kernel adds its BVH walks to one of kWalkSub partial counters,
// kWalkStride words apart; they belong to the context, so contexts on other streams or devices count for themselves.
constexpr int kWalkSub = 64, kWalkStride = 8;
int rs_walk_counters(unsigned long long** counters);    // allocated on first use, zeroed in the order of the context's stream
int rs_walk_counters_sum(unsigned long long* rays);     // waits for the stream and adds the partial counters up (null: nothing to do)

// ---- tile-split hints (rs_tilesplit.h) -------------------------------------------------------------
// One per launch site and stream: the lists / flags the last launch of that geometry on that stream left for the next one.
struct rs_tile_split {
    static constexpr int kCapacity = 4096;
    int* base = nullptr;                             // header + three hints + three flag arrays (layout: rs_tilesplit.h)
    size_t bytes = 0;
    int rot = 0;                                     // the hint the next launch reads
    long long key = -1;                              // the launch geometry (and threshold) the hints belong to
    int numTiles = 0, capacity = 0;                  // ... and what the device header says (a changed value re-initialises the hints whatever the key)
    // small overlapped launches (mode 2): the device's report word and the host's view of it
    unsigned long long* report = nullptr;            // pinned host memory (rs_tilesplit.h)
    unsigned issued = 0, wake = 0;                   // split launches issued so far; the count when the site last (re)started splitting
    int sleep = 0;                                   // plain launches left before the site looks again
    bool lastNone = false;                           // the last fresh report named no heavy tile
};
// fills *ts for a launch of `regularBlocks` blocks of four tiles each on stream st (all zero when the feature is off) and
// returns through *helperBlocks how many blocks the grid gets in front of them.  mode:
//   1  the kernel runs with nothing next to it (synchronous mode, per-pass timing): the launch lasts as long as its longest chain;
//   0  a launch of several rounds of wave slots next to other frames' kernels: they fill in around a long tile, and splitting
//      measured 2.5 % SLOWER (extra waves, extra blocks) -- no splitting;
//   2  a launch of less than three rounds of wave slots next to other frames' kernels (a strip): a single round of waves ends with
//      its slowest tile whatever runs next to it -- the 72- and 48-row strips of a cost-balanced 8-way split of the Bistro-class
//      frame 0.42 / 0.46 -> 0.29 / 0.26 ms per frame (profiles/r05_ab_tile_split_on_strips.log).  Split at 4/3 of the threshold (768
//      -> 1024: measured better than 768 on strips), and only while it finds heavy tiles: the kernels that count cost a scene
//      without any (the Sponza-class strips) 1.3 %, so a site whose last fresh report says "none" runs the plain kernels for
//      kTileSplitSleep launches before it looks again.
// (which mode a launch takes: rs_split_mode, rs_frame_plan.h)
int rs_tile_split_prepare(rs_tile_split* t, long long key, int numTiles, int regularBlocks, int mode, hipStream_t st, rs::TileSplit* ts, int* helperBlocks);
void rs_tile_split_free(rs_tile_split* t);
int rs_tile_split_threshold();                      // of the current context

// ---- scene -------------------------------------------------------------------------------------
struct rs_scene {
    rs_context* ctx = nullptr;
    rs::DevScene dev{};              // passed to kernels by value (pointers into the arrays below)
    // owned device arrays
    rs::BvhNode* dNodesAll = nullptr;
    rs::TriRec* dTris = nullptr;
    float* dVertices = nullptr;
    float* dNormals = nullptr;
    int* dMaterialIds = nullptr;
    rs_material* dMaterials = nullptr;
    rs::LightRec* dLights = nullptr;
    rs::AliasRec* dAlias = nullptr;
    rs::TexRec* dTextures = nullptr;
    float* dTexcoords = nullptr;
    rs::AliasRec* dEnvAlias = nullptr;
    std::vector<float*> dTexData;                 // one device array per texture
    std::vector<std::vector<float>> hTexData;     // host copies (rs_scene_host_desc)
    std::vector<rs_texture> hTextures;
    std::vector<float> hEnvProb;
    std::vector<int> hEnvFail;
    int envMapTexId = -1;
    bool textured = false;                        // any material map or an environment map: kernels take the textured variant
    bool hasTexcoords = false;                    // created with texcoords (rs_scene_set_materials: a first map needs them)
    uint32_t* dSampleSeq = nullptr;  // the Sobol table (rs_scene_set_sample_sequence); null: the default thrust engine
    std::vector<uint32_t> hSampleSeq;   // its host copy, without the guard (rs_debug_seeded_uniforms); empty: none
    uint4* dOccNodes = nullptr;      // shadow-ray tree (occlusion_bvh.cpp)
    rs::BvhNode* dOccChain = nullptr;   // reference boxes + parent links by original node id
    int* dLeafOfPrim = nullptr;         // reference leaf node of every primitive (hLeafOf), with dOccChain: the leaf lists' builder reads it (rs_cuts.h)
    rs::TriRec* dOccTris = nullptr;
    uint4* dEmiNodes = nullptr;      // tree of the emissive triangles alone (scene.hip build_emissive_side)
    rs::TriRec* dEmiTris = nullptr;
    uint4* dOrdNodes = nullptr;      // closest-hit trees in the reference's visiting orders (occlusion_bvh.cpp rs_build_ordered_bvh)
    rs::TriRec* dOrdTris = nullptr;
    unsigned long long* dWalkStats = nullptr;   // -DRS_WALK_STATS builds only
    // host copies of the source arrays (rs_scene_host_desc)
    std::vector<float> hVertices, hNormals, hTexcoords, hBoxes, hLightRadiance, hLightProb;
    std::vector<int> hMaterialIds, hNodes[6], hLightPrimIds, hLightFailId;
    std::vector<int> hParent, hLeafOf;   // reference tree: parent by original node id, leaf node of each primitive
    bool properBoxes = false;            // the box table is a proper hierarchy (rs_scene_create); DevScene::axisCull also asks for small triangles
    // Geometry edits (rs_scene_set_triangles, rs_scene_set_geometry; rs_refit.h, scene_refit.hip).  Kept from creation, on the host only: the primitive in every
    // slot of occTris, the box the shadow tree's grid was laid over (a moved vertex must stay inside it) and the grid's margin.
    // Everything else -- device tables, scratch, staging -- belongs to `refit`, which the first edit allocates, but for the scratch of
    // the edit's plan (rs_geometry_plan.h), which needs no device.
    rs_edit_stamps editStamps;
    std::vector<int> hOccLeafPrims;
    float gridLo[3] = {}, gridHi[3] = {};
    double gridMargin = 0.0;
    // ... and of the emissive tree: the primitive in every slot of emiTris, and the margin of its own grid (dev.emiBase / emiScale)
    std::vector<int> hEmiLeafPrims;
    double emiMargin = 0.0;
    struct rs_refit* refit = nullptr;
    // rs_scene_set_partial_refit: the switch and its threshold as the caller set them (< 0: the library's default).  The scene's own, because
    // the switch may be set before the first edit has made `refit`; the tables of the partial path belong to `refit` (rs_refit.h)
    bool partialRefit = false;
    int partialMaxTriangles = -1;
    struct rs_parts* parts = nullptr;   // rigid parts and their rest pose (rs_scene_define_parts; rs_deform.h); null: none defined
    // Motion tracking (rs_scene_set_motion_tracking, rs_scene_advance_motion): dev.prevVertices is dPrevVertices while tracking is on, null
    // otherwise; the array stays allocated until rs_scene_destroy.  motionDirty: a geometry edit has been accepted since prevVertices was
    // last made equal to the vertices, i.e. the two may differ.  The fences are the geometry edits' (rs_refit::before / after), the scene's own
    // because a scene can be tracked before its first edit.
    float* dPrevVertices = nullptr;
    bool motionDirty = false;
    hipEvent_t motionBefore[rs_context::kAux] = {};
    hipEvent_t motionAfter = nullptr;
    std::vector<rs_material> hMaterials;
    float sumLightPower = 0.f;
    int numPrims = 0, bvhSize = 0, numLights = 0;
    unsigned long long id = 0;       // unique per rs_scene_create (a freed scene's address can come back; its id cannot)
    unsigned long long geomEdits = 0;   // counts the edits that refit the box tables (rs_set_geometry, scene_edits.hip): part of a primary cut's key (rs_primary_cut_key, rs_cut_plan.h)
    unsigned long long edits = 0;    // counts the edits that change what GBuffer::render writes (rs_scene_set_emission: baseColor, hence the albedo plane); part of a G-buffer set's content key
    // Edits (rs_scene_set_emission, rs_scene_set_materials, rs_scene_set_texture): a ring of versions of { materials, light records,
    // alias table, texture table }.  Kernels capture
    // `dev` by value at launch, so a version is never written while a launch that captured it may still run: an edit fills the
    // next slot (ordered before every later launch by an event) and points `dev` at it, and a slot is filled again only after the events recorded when the
    // scene moved off it -- on the library stream and on every auxiliary stream -- have completed.  Version 0 is the arrays above.
    static constexpr int kVersions = 8;
    static constexpr int kVersionStreams = 1 + rs_context::kAux;
    struct Version {
        rs_material* materials = nullptr;
        rs::LightRec* lights = nullptr;
        rs::AliasRec* alias = nullptr;
        rs::TexRec* textures = nullptr;          // the texture table: its records point at the texel arrays current when the slot was filled
        uint32_t* moved = nullptr;               // hLightMoved (below), one word per sampler entry: every slot has its own array, slot 0 too
        char* staging = nullptr;                 // pinned host copy the slot is filled from
        hipEvent_t retired[kVersionStreams] = {};
        bool retiredValid[kVersionStreams] = {};
    } ver[kVersions];
    int verCur = 0;
    unsigned long long verSeq = 0;               // how many edits the scene has taken: version verSeq lives in slot verSeq % kVersions
    // Texel arrays and the environment sampler's alias table are too large to ring eightfold, and most are never edited: each is one
    // Edited, which holds only the original array until its first edit and at most kEditedCopies arrays after (rs_scene_set_texture
    // takes a copy no version in flight points at, allocates one while it may, else waits for the oldest to retire).
    static constexpr int kEditedCopies = 3;
    struct Edited {
        void* dev[kEditedCopies] = {};           // [0]: the array rs_scene_create uploaded (owned by dTexData / dEnvAlias)
        char* staging[kEditedCopies] = {};       // pinned host copy each later array is filled from
        unsigned long long lastSeq[kEditedCopies] = {};   // the last version whose tables point at the array (the current one: open)
        int count = 1, cur = 0;
    };
    std::vector<Edited> texEdited;               // one per texture
    Edited envEdited;
    bool verReady = false;                       // slots 1.. and the staging buffers allocated
    hipEvent_t verFilled = nullptr;              // the last fill: the library stream and the auxiliary streams wait for it
    hipStream_t verStream = nullptr;             // the fills' own stream (a free slot waits for no frame in flight)
    std::vector<float> hLightArea;               // per light primitive, Math::triangleArea (filled on the first edit)
    float envPower = 0.f;                        // the environment map's sampler entry (its pdf's sum)
    bool envPowerKnown = false;
    // Moved lamps (rs_restir_set_light_retargeting): lightMoves counts the accepted geometry edits that named an emitter, hLightMoved[i]
    // is lightMoves at the last edit that named light i's primitive (0: never).  The device copy travels in the ring of versions next to
    // the light records, so that a launch reads the stamps of the light records it reads.  hLightOfPrim: sampler entry of a primitive, -1 = none.
    unsigned long long lightMoves = 0;
    std::vector<uint32_t> hLightMoved;
    std::vector<int> hLightOfPrim;
    // Dirty boxes (rs_restir_set_shadow_revalidation; rs_revalidate_plan.h): the box of each of the last RS_DIRTY_BOXES_KEPT accepted
    // geometry edits with its number, geomEdits once the edit was counted.  Host only, written where the edit is enqueued.
    rs_dirty_ring dirty;
    // Skinned triangles, their rest pose and the bone palette (rs_scene_define_skin; rs_deform.h); null: none defined.  Last, so that every
    // field a frame reads lies where it lay before there were skins.
    struct rs_skin* skin = nullptr;
    // Morph targets with a rest pose of their own (rs_scene_define_morph; rs_deform.h); null: none defined.  (A skin's morph is the skin's.)
    struct rs_morph* morph = nullptr;
};

// ---- G-buffer (src/gbuffer.h:41-58) ------------------------------------------------------------
// The reference keeps two sets of the id / normal / depth planes and toggles frameIdx.  Here all planes live in a ring of
// five sets: the set of the previous frame ("last" planes), of the frame whose passes the library stream is at, and of up to
// three frames whose renders run ahead on the auxiliary streams (a strip has three chains in flight, each with the frame's render
// in its first launch), so that no render writes what an earlier frame's temporal pass still reads.  frameIdx is still toggled
// and reported by rs_gbuffer_get_view, whose devNormal[frameIdx] / [frameIdx ^ 1] are the current / last sets.
//
// Reuse (GBuffer::render, src/gbuffer.cu:80-86, reads the scene, the camera, lastCamera and the row range and nothing else): the ring
// is one of POSITIONS, and phys[] says which set of planes a position shows.  Every set carries the key of the one render that wrote it
// during its frame.  A frame's first render request whose key equals the keys of the two previous frames' sets launches nothing: its
// position takes the set of the frame before the previous one -- the bits a render would have written -- and prev() stays the previous
// frame's set, the bits it would have left as "last" planes.  A still camera so alternates between two sets, read and never written by
// all frames in flight.  The ring itself advances as always, so every position shows what it would show without reuse (also the stale
// planes a frame without a render looks at).  A request that differs renders into a set that no other position shows.
struct rs_gbuffer {
    rs_context* ctx = nullptr;
    static constexpr int kSets = RS_GBUF_SETS;
    float* albedo[kSets] = {};
    int* motion[kSets] = {};
    float* normal[kSets] = {};
    int* primId[kSets] = {};
    float* depth[kSets] = {};
    int ring = 0;                // position of the current frame; the previous frame's is (ring + kSets - 1) % kSets
    int phys[kSets];             // the set each position shows (the identity until a request is answered from retained planes)
    bool posKeyed[kSets] = {};   // the frame at that position had exactly one render request, and its set took (or matched) that request's key
    int frameIdx = 0;
    rs_camera lastCamera{};      // uninitialised in the reference until the first update (Q14); zero here
    int width = 0, height = 0;
    // ordering of a render on the auxiliary stream (asynchronous mode)
    hipEvent_t forkEv = nullptr;             // "everything enqueued on the library stream so far"
    hipEvent_t doneEv = nullptr;             // the render
    hipEvent_t useEv[kSets] = {};   // recorded by update(): the frame that ended there has been enqueued
    int useOf[kSets];       // per set: which useEv covers its last readers (-1: none outstanding)
    rs_gbuffer() { for (int i = 0; i < kSets; i++) { useOf[i] = -1; phys[i] = i; } }
    // a filter on the denoise stream reads (a strip's: also writes the rows just outside the strip of) the current set after the library
    // stream has moved on: the next render into that set waits for this event as well (rs_gbuffer_order_before_render)
    mutable hipEvent_t denoiseEv[kSets] = {};
    mutable bool denoiseValid[kSets] = {};
    int updates = 0;
    bool renderedSinceUpdate = false;
    mutable bool pending = false;            // a render on the auxiliary stream has not been joined yet
    // asynchronous mode: a render that has been requested but not launched yet.  ReSTIRDirect launches it together with its
    // primary rays (one packet walk for the two rays of a pixel, restir.hip k_gbuffer_primary); any other reader of the planes
    // launches it by itself first (rs_gbuffer_join).
    struct Deferred {
        bool valid = false, rerender = false;
        const rs_scene* scene = nullptr;
        rs_camera cam{}, lastCam{};
        int y0 = 0, y1 = 0;
    };
    mutable Deferred deferred;
    mutable rs_tile_split split[2];          // k_render_gbuffer on the library stream / on the auxiliary stream
    // content keys (see above).  valid: exactly one render wrote the set during its frame and nothing has written its keyed rows since
    struct Key {
        bool valid = false;
        unsigned long long sceneId = 0, edits = 0;
        rs_camera cam{}, lastCam{};
        int y0 = 0, y1 = 0;
    };
    Key key[kSets];
    bool reuse = true;                       // rs_gbuffer_set_reuse (RS_GBUFFER_REUSE=0: off from the start)
    bool reusedFrame = false;                // this frame's render request was answered from the retained planes (cleared by update and by a second render)
    unsigned long long numRendered = 0, numReused = 0;   // rs_gbuffer_reuse_stats
    int pos(int back) const { return (ring + kSets - back) % kSets; }   // the position of the frame `back` frames ago
    int cur() const { return phys[ring]; }
    int prev() const { return phys[pos(1)]; }
    // albedo / motion are single planes in the reference: they show the most recent render, also after update()
    int latest() const { return (renderedSinceUpdate || updates == 0) ? cur() : prev(); }
};
// the library stream waits for a render that is still on the auxiliary stream (and a deferred one is launched first); every
// reader of the planes calls it first
int rs_gbuffer_join(const rs_gbuffer* g);
// a deferred render was launched by someone else (ReSTIRDirect, fused with its primary rays): forget the record
void rs_gbuffer_deferred_taken(const rs_gbuffer* g);
// launches every render of `scene` that is still only recorded (rs_scene_destroy calls it before it frees the arrays)
int rs_gbuffer_release_scene(const rs_scene* scene);
// orders `stream` after the last readers of the set a (deferred) render is about to write
int rs_gbuffer_order_before_render(const rs_gbuffer* g, hipStream_t stream);
// inside an rs_denoise_scope: the current set is in use on the denoise stream up to here
int rs_gbuffer_denoise_mark(const rs_gbuffer* g);
// somebody other than a render writes rows [y0, y0 + rows) of set `set` (rs_gbuffer_rows_unpack, a strip's halo copies): a content key
// whose rows they overlap no longer describes the set
void rs_gbuffer_note_write(rs_gbuffer* g, int set, int y0, int rows);
bool rs_fuse_enabled();
int rs_ris_global_below();
const rs_context* rs_stream_plan();   // the current context with chainStreams / smallChains / shadowOnMain resolved
int rs_fuse_mode();     // 0 never, 1 always (large launches), 2 always, 3 measured per rs_restir

// device view of the planes the kernels read
struct GBufView {
    const float* albedo;
    const int* motion;
    const float* normal; const float* lastNormal;
    const int* primId;   const int* lastPrimId;
    const float* depth;  const float* lastDepth;
    int width, height;
};
static inline GBufView gbuf_view(const rs_gbuffer* g) {
    GBufView v;
    const int c = g->cur(), l = g->prev();
    v.albedo = g->albedo[g->latest()]; v.motion = g->motion[g->latest()];
    v.normal = g->normal[c]; v.lastNormal = g->normal[l];
    v.primId = g->primId[c]; v.lastPrimId = g->primId[l];
    v.depth = g->depth[c]; v.lastDepth = g->depth[l];
    v.width = g->width; v.height = g->height;
    return v;
}

#if defined(__HIPCC__)
// Wave priorities (s_setprio, 0-3: the SIMD's arbiter issues the ready wave of the highest priority first).  In the overlapped mode the
// streaming kernels of the library stream (temporal merge, border-row copies, spatial pass, tone map) share every SIMD with the walks
// and the RIS loop of other frames, and a GPU-paced kernel trace of a 1/8 strip shows them stretched seven-fold (k_temporal 13 -> 95 us:
// the library stream busy 96 % of the frame period, tools/strip_trace_c.py).  Their waves are few and short, so they go first: full
// frame 1.047 -> 1.027 ms, light strips -7 %, heavy strips -2 % (priority 1 and 3 measure the same).  The walks at ANY raised
// priority cost a third of the frame (1.05 -> 1.42 ms: they take the issue slots of the RIS loop, which is what bounds the frame), and
// the RIS loop raised gains nothing (profiles/r05_ab_wave_priorities.log).
#ifndef RS_PRIO_WALK
#define RS_PRIO_WALK 0
#endif
#ifndef RS_PRIO_STREAM
#define RS_PRIO_STREAM 1
#endif
#ifndef RS_PRIO_RIS
#define RS_PRIO_RIS 0
#endif
#ifndef RS_PRIO_EAW
#define RS_PRIO_EAW 0
#endif
#define RS_SETPRIO(p) do { if ((p) > 0) __builtin_amdgcn_s_setprio(p); } while (0)

// ---- what the per-pixel kernels share (restir.hip, gi.hip, pathtrace.hip) -----------------------------
// One lane per pixel: a block of 256 threads takes 32x8 pixels, each of its four waves an 8x8 tile; rows count from y0.  Returns the
// lane within the wave, for count_walks (kernels that count otherwise ignore it).
__device__ __forceinline__ int pixel_of_lane(int tilesX, int y0, int& x, int& y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bx = blockIdx.x % tilesX, by = blockIdx.x / tilesX;
    x = bx * 32 + wave * 8 + (lane & 7);
    y = y0 + by * 8 + (lane >> 3);
    return lane;
}
// Does a shadow segment's visibility matter?  Not for a contribution whose three components are all +0 (x + (+0) = x for every x but
// -0, and the sums start at +0); a NaN or -0 component has a bit set, and the segment is walked.
__device__ __forceinline__ bool any_bit(rs::f3 v) { return (__float_as_uint(v.x) | __float_as_uint(v.y) | __float_as_uint(v.z)) != 0u; }
// the running mean over iterations of the accumulating passes (pathtrace.cu:273-276,325)
__device__ __forceinline__ void accumulate(float* image, int index, rs::f3 v, int iter) {
    float* o = image + (size_t)index * 3;
    rs::st3(o, (rs::ld3(o) * (float)iter + v) / (float)(iter + 1));
}
// BVH walks for the Mrays/s metric: wave-level sum, one atomic per wave (by `lane` 0), to the address the caller chose.
// `lane` is the value pixel_of_lane returned, on purpose: a second `threadIdx.x & 63` here is not merged with the first and moved
// k_path's register allocation (ReSTIR-GI, plain scene: 108 -> 116 B of scratch; EXPERIMENTS.md).
__device__ __forceinline__ void count_walks(unsigned long long* counter, int walks, int lane) {
    for (int off = 32; off > 0; off >>= 1) walks += __shfl_down(walks, off);
    if (lane == 0 && walks) atomicAdd(counter, (unsigned long long)walks);
}
// what renderGBuffer writes for one pixel (src/gbuffer.cu:21-72); shared by k_render_gbuffer and the kernel that walks the
// G-buffer ray together with the shading ray (restir.hip)
struct GBufWrite {
    float* albedo; int* motion; float* normal; int* primId; float* depth;
};

// MOTION (the scene tracks motion, DevScene::prevVertices): the motion plane asks where the hit point of the TRIANGLE was on last frame's
// screen -- the hit's barycentrics on the triangle's previous pose, in hit_of_walk's expression and order, so that a triangle that has not
// moved gives h.pos bit for bit -- instead of where the world point h.pos was.  A compile-time form: the untracked kernels keep their code.
template <bool TEX, bool MOTION = false>
__device__ __forceinline__ void gbuffer_store(const rs::DevScene& s, const rs::CamParams& cam, const rs::CamParams& lastCam, const GBufWrite& g,
                                              int idx, const rs::Ray& ray, const rs::Hit& h) {
    using namespace rs;
    if (h.primId != kNullPrim) {
        int matId = h.matId;
        f3 norm = h.norm;
        const SurfMat m = TEX ? textured_material(s, h, norm) : plain_material(s, h.matId);
        if (m.type == 4) matId = kNullPrim - 1;          // lights -> -2 (gbuffer.cu:30-31; the map lookup cannot change the type)
        st3(g.albedo + (size_t)idx * 3, m.baseColor);
        st3(g.normal + (size_t)idx * 3, norm);
        g.primId[idx] = matId;
        g.depth[idx] = length(ray.o - h.pos);            // glm::distance(pos, origin) = length(origin - pos)
        int lx, ly;
        f3 prevPos = h.pos;
        if (MOTION) {
            const float* pv = s.prevVertices + (size_t)h.primId * 9;
            prevPos = ld3(pv + 3) * h.bx + ld3(pv + 6) * h.by + ld3(pv) * (1.f - h.bx - h.by);
        }
        camera_raster_coord(lastCam, prevPos, lx, ly);
        g.motion[idx] = (lx >= 0 && lx < cam.width && ly >= 0 && ly < cam.height) ? ly * cam.width + lx : -1;
    }
    else {
        st3(g.albedo + (size_t)idx * 3, (TEX && s.envTex >= 0) ? env_radiance(s, ray.d) : splat(0.f));
        st3(g.normal + (size_t)idx * 3, splat(0.f));
        g.primId[idx] = kNullPrim;
        g.depth[idx] = 1.f;
        g.motion[idx] = 0;
    }
}
#endif

// ---- reservoirs ----------------------------------------------------------------------------------
// One Reservoir<DirectLiSample> (36 B AoS in the reference, src/restir.h:114-116) is stored as four
// planes so that streaming passes read 16 B / lane and the spatial pass can stage only what its
// neighbour tests need:
//   li  float4[N]  { Li.x, Li.y, Li.z, dist }
//   wi  float4[N]  { wi.x, wi.y, wi.z, 0    }
//   w   float [N]  weight
//   m   int   [N]  numSamples
struct ResvPlanes {
    float4* li = nullptr;
    float4* wi = nullptr;
    float*  w = nullptr;
    int*    m = nullptr;
};

// devDirectTemp (src/restir.cu:10), the buffer the spatial pass gathers from.  Weight and M travel
// together with the two G-buffer values every tap test needs, so that the spatial pass stages ONE
// 16-byte record (+ the 12-byte normal) per neighbour instead of four 4-byte planes:
//   tap float4[N] { weight, bits(numSamples), bits(G-buffer id), depth }
// The reservoir half of a record is only written for pixels that published this frame (stale
// otherwise, Q1); the G-buffer half is refreshed for every pixel.
struct TempPlanes {
    float4* li = nullptr;
    float4* wi = nullptr;
    float4* tap = nullptr;
};

// one traversal for the G-buffer ray and the shading ray of a pixel, or two?  Measured once per scene (rs_fuse_mode() == 3):
// frames 6..17 with two launches against 22..33 with one (the four frames after each switch are not timed), by events on the library stream at the frame ends
struct rs_fuse_tuner {
    unsigned long long sceneId = 0;
    int frame = 0;                   // frames with a fusable launch since tuning began
    int choice = -1;                 // -1 measuring, 0 separate, 1 fused
    bool counted = false;            // this frame had a launch the choice applies to
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
    // what a frame of `scene` sees of the measurement (another scene's: one that has not begun), rs_tuned_fuse() of which is the form it takes
    int choice_for(unsigned long long scene) const { return sceneId == scene ? choice : -1; }
    int frame_for(unsigned long long scene) const { return sceneId == scene ? frame : 0; }
    void count(unsigned long long scene) { if (sceneId != scene) { sceneId = scene; frame = 0; choice = -1; } counted = true; }
    void restart() { if (choice < 0) frame = 0; }    // a measurement under way starts again
    int end_frame(hipStream_t st);                   // a frame ended: the time stamps, and the decision once the last one has been reached (restir.hip)
    int reported() const { return choice >= 0 ? choice : (frame > 0 || counted) ? -1 : -2; }     // rs_restir_launch_choice
};

// Static cuts of the tree for the primary rays of a still camera (rs_cuts.h), one slot per phase-A call of a frame (as the tile-split
// hints: a strip driver's calls have rows of their own).  primary_cuts.hip owns every field; the host decisions are rs_cut_plan.h's.
// slot.key is what the cut was built from: the scene and its geometry edits (rs_scene::geomEdits -- materials and emission do not
// count), every byte of the camera, the size, the rows and the caps.  Every call compares its key with the one the same call of the
// previous frame left; the first call that finds it unchanged enqueues the build behind its chain, the calls after that walk the cut, a
// call that finds another key forgets the cut.  Nothing here waits on the host: builtEv orders the readers' streams after the build,
// usedEv[] orders a later build into the same arena after its readers.
struct rs_primary_cut {
    rs_primary_cut_slot slot{};
    rs_primary_cut_sizes size{};             // of the arenas below (zeros: none)
    uint2* cells = nullptr;                  // per cell { first record, count | order << 28 }
    rs::BvhNode* records = nullptr;          // the arena: size.capacity records and one more that is only ever read
    unsigned* orig = nullptr;                // original index of every record (the builder's links; the containment test hook)
    unsigned long long* counters = nullptr;  // [0] records handed out, [1] cells without a cut, [2] records in cuts; [4..6] the same of the leaf lists and tiles
    // the tiles' leaf lists (rs_cuts.h "Leaf lists"): same key, built by the same call behind the cuts, read by the same launches
    uint2* tiles = nullptr;                  // per tile { first record, count | order << 28 }
    float4* leafRecords = nullptr;           // the arena: size.listCapacity 64-byte records and one more that is only ever read
    int* leafOf = nullptr;                   // reference node of every record's leaf
    int tilesPerRow = 0;
    hipEvent_t builtEv = nullptr;
    hipEvent_t usedEv[1 + rs_context::kAux] = {};
    bool usedValid[1 + rs_context::kAux] = {};
    unsigned long long builds = 0, listBuilds = 0;
};

// the cuts of one rs_restir: the slots, the switches and what the last phase-A call did
struct rs_primary_cuts {
    rs_primary_cut slot[3];
    bool on = true;                          // rs_restir_set_primary_cuts (RS_PRIMARY_CUTS=0: off from the start)
    unsigned cap = 4096;                     // records a cell's cut may have (rs_debug_set_primary_cut_cap)
    bool listsOn = true;                     // rs_restir_set_primary_leaf_lists (RS_PRIMARY_LEAF_LISTS=0: off from the start); lists need the cuts' switch too
    unsigned listCap = 192;                  // records a tile's leaf list may have (rs_debug_set_primary_leaf_list_cap; 0: no tile takes a list)
    int last = 0;                            // the last phase-A call's slot
    bool lastUsed = false;                   // the last phase-A call's primary rays walked cuts
    bool lastListsUsed = false;              // ... and its whole tiles their leaf lists
};
namespace rs { struct PrimaryCuts; }
// What phase_a_impl (restir.hip) asks of primary_cuts.hip, in the order it asks: the call's rs_phase_a_inputs::cutState (call: phase-A
// calls of this frame before this one); when the plan says 2, the cuts to hand to the launch, `st` ordered after their build, and after
// the launch the reader's event for stream index k (0 the library stream, 1 + the internal stream); when it says 1, the build, enqueued
// on st after every launch that still reads the arena.
void rs_primary_cuts_init(rs_primary_cuts& c);
int  rs_primary_cuts_begin(rs_primary_cuts& c, int call, const rs_scene* scene, const rs_camera* cam, int y0, int y1);
int  rs_primary_cuts_view(rs_primary_cuts& c, hipStream_t st, rs::PrimaryCuts* out);
int  rs_primary_cuts_launched(rs_primary_cuts& c, int k, hipStream_t st);
int  rs_primary_cuts_build(rs_primary_cuts& c, const rs_scene* scene, const rs::CamParams& cp, int y0, int tilesX, int tilesY, hipStream_t st);
void rs_primary_cuts_destroy(rs_primary_cuts& c);

// Light tracking and retargeting of one rs_restir (include/restir_hip.h); light_history.hip owns every field.  ids
// (rs_restir_set_light_tracking): the light-sampler index of every reservoir's sample, -1 = not known, allocated when tracking is first
// switched on.  records (rs_restir_set_light_retargeting, on top of the ids): a 16-byte record { light, u, v, pdf } beside each id, and
// the planes k_retarget leaves the re-evaluated temporal candidates in; allocated when retargeting is first switched on.
enum { RS_LIGHTS_OFF = 0, RS_LIGHTS_IDS = 1, RS_LIGHTS_RECORDS = 2 };
struct rs_light_history {
    int mode = RS_LIGHTS_OFF;
    int* id[3] = {}; float4* rec[3] = {};      // by the public `which`: 0 cur, 1 last (swapped with the reservoirs), 2 the published copy (TempPlanes)
    int* candId[RS_SURF_SETS] = {}; float4* candRec[RS_SURF_SETS] = {};      // of the RIS winners, one plane per surface set
    unsigned long long sceneId = 0;        // the scene whose light indices id[1] holds (rs_scene::id; 0 = none yet)
    float4 *rtLi = nullptr, *rtWi = nullptr, *rtRec = nullptr;      // re-evaluated candidate: { Li xyz, dist }, { wi xyz, W }, its record
    int* rtFlag = nullptr;           // 1: the pixel's temporal candidate is the one in the three planes above
    unsigned long long seenMoves = 0;      // the scene's lightMoves at the previous frame (forgotten with sceneId)
    unsigned long long frameMoves = 0;     // ... at this frame's phase-A calls: seenMoves of the next frame (rs_light_history_end_frame)
    unsigned long long* dRetarget = nullptr;   // { re-evaluated, segments, zeroed } of the last frame that launched k_retarget: cleared, added to and read in the library stream's order
    bool rtLaunched = false, rtLaunchedLast = false;     // this frame / the frame that ended last launched k_retarget
};
// What restir.hip, rs_row_layouts.h and strips.hip ask of light_history.hip (phase_a_impl's call: rs_light_history.h).  forget: the
// planes of the buffers in `which` (bit k: buffer k as above) become unknown -- `planes` bit 0 the ids, bit 1 the records, -1 what the
// mode has -- with hipMemset (blocking: rs_restir_upload, behind its blocking copies) or in the library stream's order.
inline int  rs_light_mode(const rs_light_history& h) { return h.mode; }
inline int* rs_light_id_plane(const rs_light_history& h, int which) { return h.id[which]; }
int  rs_light_history_forget(rs_light_history& h, size_t pixels, unsigned which, bool blocking, int planes = -1);
void rs_light_history_end_frame(rs_light_history& h, int phaseACalls);      // cur and last change places, as the reservoirs'
void rs_light_history_free(rs_light_history& h);

// Shadow revalidation of one rs_restir (include/restir_hip.h); shadow_revalidate.hip owns every field.  sceneId / seen: the scene of the
// previous frame and its count of accepted geometry edits then -- kept whether the switch is on or not; frameScene / frameEdits: of this
// frame's phase-A calls, which rs_revalidate_end_frame makes the previous frame's.  flag: one word per pixel, equal to the epoch of the
// phase-A call whose k_revalidate found the pixel's temporal candidate occluded -- every launch takes a new epoch, so the plane is never
// cleared, and a block without a walker does not touch it.
struct rs_shadow_revalidation {
    bool on = false;
    bool fresh = false;                    // switched on since the previous frame: the edits made so far count as seen
    unsigned* flag = nullptr;              // 4 B/px, allocated at the first switch-on
    unsigned long long* dStats = nullptr;  // { examined, walked, occluded } of the last frame that launched, each in partial counters: cleared, added to and read in the library stream's order
    unsigned epoch = 0;                    // of the last launch (0: none; the plane starts as zeros)
    unsigned long long sceneId = 0, seen = 0, frameScene = 0, frameEdits = 0;
    bool launched = false, launchedLast = false;      // this frame / the frame that ended last launched k_revalidate
};
void rs_revalidate_end_frame(rs_shadow_revalidation& v, int phaseACalls);
void rs_revalidate_free(rs_shadow_revalidation& v);

// Revalidation of ReSTIR-GI's history of one rs_restir (include/restir_hip.h); indirect_revalidate.hip owns every field.  sceneId / seen:
// the scene of the previous accepted rs_restir_indirect call and its count of accepted geometry edits then -- kept whether the switch is
// on or not, and apart from rs_shadow_revalidation's: rs_restir_direct and rs_restir_indirect are separate calls.  No per-pixel plane: the
// pass edits the history slots themselves.
struct rs_indirect_revalidation {
    bool on = false;
    unsigned long long sceneId = 0, seen = 0;      // sceneId 0: no call yet
    unsigned long long* dStats = nullptr;  // { examined, stale, walked, occluded } of the last call that launched, each in partial counters: cleared, added to and read in the library stream's order
    bool launchedLast = false;             // the last rs_restir_indirect call launched k_revalidate_indirect
};
// What rs_restir_indirect (gi.hip) asks, in this order: before launch_path, the pass over the n slots of `history` (the buffer k_path is
// about to read) when the call merges and the plan says so; after an accepted call, the scene and its edits noted; and, once the stream
// has been waited for, the walked segments of this call's pass added to *rays.
int  rs_indirect_revalidate_before_path(rs_restir* r, const rs_scene* scene, bool merges, rs_indirect_reservoir* history, size_t n);
void rs_indirect_revalidate_note(rs_restir* r, const rs_scene* scene);
int  rs_indirect_revalidate_add_rays(rs_restir* r, unsigned long long* rays);
void rs_indirect_revalidate_free(rs_indirect_revalidation& v);

// Spatial reuse of ReSTIR-GI's reservoirs of one rs_restir (include/restir_hip.h); indirect_spatial.hip owns every field.  Everything is
// allocated at the first switch-on and kept; the recording planes only once rs_debug_restir_indirect_primary has asked for them.
struct rs_indirect_spatial {
    bool on = false;
    int taps = 5;                          // RS_GI_SPATIAL_MAX_TAPS at most
    float radius = 5.f;                    // pixels
    rs_indirect_reservoir* resv = nullptr; // devIndSpatialReservoir (restir.cu:15): 68 B/px, written by every call that runs the pass
    float* temporalImage = nullptr;        // 12 B/px: where the path kernel of such a call leaves its temporal-only radiance (iter 0)
    unsigned long long* dStats = nullptr;  // the eight counters of the last call that ran the pass, each in partial counters
    float4* recorded = nullptr;            // 3 planes of float4 (xv, nv, wo) ...
    int* recordedMat = nullptr;            // ... and the material id, -1 where the pixel does not take part (test hook; null until asked for)
    bool launchedLast = false;             // the last rs_restir_indirect call ran k_spatial_indirect
};
// What rs_restir_indirect (gi.hip) asks, in this order: does this call run the pass (then the path kernel writes `temporalImage` with iter
// 0 instead of the caller's image); after launch_path, the pass from `temporal` (the buffer the path kernel has just written) into the
// caller's image; and, once the stream has been waited for, the winners walked added to *rays.
bool rs_indirect_spatial_runs(rs_restir* r, int reuse);
int  rs_indirect_spatial_after_path(rs_restir* r, const rs_scene* scene, const rs_camera* cam, const GBufView& g, const rs_indirect_reservoir* temporal,
                                    float* image, int iter, int looper);
int  rs_indirect_spatial_add_rays(rs_restir* r, unsigned long long* rays);
void rs_indirect_spatial_free(rs_indirect_spatial& v);

struct rs_restir {
    rs_context* ctx = nullptr;
    rs_primary_cuts cuts;
    // The chain primary rays -> RIS -> shadow rays of a frame depends on no other frame.  Frames put theirs on kChains auxiliary
    // streams in turn, so that consecutive frames' chains overlap: on a 1/8 strip a chain lasts 0.4 ms however few rows it has.
    // A chain writes one of kSurfSets sets of surface planes, which the frame's temporal / spatial passes read afterwards; with as
    // many sets as chains a chain would have to wait until those passes of the frame two back have finished, with one more it
    // starts as soon as its stream is free.  A third chain next to the render's stream would be a fifth stream on the runtime's
    // four hardware queues (slower).  A small launch -- a strip, whose kernels last as long as their slowest wave -- therefore
    // takes the fused launch (render + primary rays, k_gbuffer_primary), after which nothing runs on the render's stream, and
    // gives that stream to a third chain (kSmallChains; rs_frame_plan.h): 8 strips of 1080p 5.96x -> 6.5x.
    static constexpr int kChains = kPlanChains, kSmallChains = kPlanSmallChains, kSurfSets = RS_SURF_SETS;
    int width = 0, height = 0;
    ResvPlanes cur;      // devDirectReservoir      (written this frame)
    ResvPlanes last;     // devLastDirectReservoir  (read by the temporal merge)
    TempPlanes temp;     // devDirectTemp           (published for the spatial pass)
    rs_indirect_reservoir* indResv[2] = { nullptr, nullptr };   // devIndTemporalReservoir / devIndLastTemporalReservoir (gi.hip), allocated on first use
    bool firstFrame = true;
    int looper = 0;                  // of the last phase-A call (phase B resumes the per-pixel samplers it left)
    // per-pixel state carried between the passes of one frame (implementation bytes, not in the
    // reference: its single fused kernel keeps these in registers).  kSurfSets sets, used in turn: the primary-ray,
    // RIS and shadow-ray kernels of the next frames (auxiliary streams) fill theirs while the temporal / spatial passes of frame f read this one.
    struct Surf {
        float4* posKind = nullptr;   // hit position xyz, w = bit pattern of (matId | kind<<24)
        float4* norm = nullptr;      // shading normal xyz (flipped to wo side)
        float4* wo = nullptr;        // wo xyz (read only for non-Lambertian materials)
        uint2*  rngMat = nullptr;    // { RNG state, matId | kind<<24 }
        float4* candLi = nullptr;    // RIS winner: Li xyz, w = dist
        float4* candWi = nullptr;    // RIS winner: wi xyz, w = weight (sum of candidate weights)
    } surf[kSurfSets];
    int surfSet = 0, chain = 0, smallChain = 0;      // of the frame in flight
    hipEvent_t surfFree[kSurfSets] = {};             // recorded by end_frame: the frame that used the set has been enqueued
    bool surfFreeValid[kSurfSets] = {};
    hipEvent_t auxFork = nullptr, auxDone = nullptr;
    int phaseACalls = 0;             // since the last end_frame
    bool idleFrame = false;          // this frame's first phase-A call found the previous frames finished (restir.hip phase_a_impl)
    int idleStreak = 0;
    rs_fuse_tuner tune;
    int lastFused = -1, lastChains = 0;   // form of the last phase-A launch: render fused with the primary rays? how many chain streams in turn? (rs_restir_last_launch)
    unsigned long long* dRayCount = nullptr;   // ring of per-frame counters (1024 slots)
    rs_tile_split split[1 + rs_context::kAux][3];   // primary-ray launches: per stream (library, auxiliary 0..2) and per call within a frame (strips: interior rows, border rows)
    int raySlot = 0;
    // timing
    int timing = 0;                  // 0 off, 1 every pass on the library stream, 2 the spatial pass only, launches as in the overlapped mode
    hipEvent_t ev[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    static constexpr int kSpatialRing = 256;
    hipEvent_t spatialEv[kSpatialRing][2] = {};     // timing 2: the spatial pass of the last frames between two events each (rs_restir_spatial_times)
    int spatialNext = 0;
    bool probe = false;              // the spatial pass goes out as k_spatial_shade_probe (rs_restir_set_probe)
    rs_light_history lights;         // light tracking and retargeting (light_history.hip)
    bool shadowRegroup = true;       // rs_restir_set_shadow_regroup (RS_SHADOW_REGROUP=0: off from the start); a scene without occNodes keeps the plain kernel
    rs_shadow_revalidation reval;    // rs_restir_set_shadow_revalidation (shadow_revalidate.hip)
    rs_indirect_revalidation indReval;   // rs_restir_set_indirect_revalidation (indirect_revalidate.hip)
    rs_indirect_spatial indSpatial;      // rs_restir_set_indirect_spatial (indirect_spatial.hip)
};

static_assert(rs_context::kAux >= 1 + rs_restir::kChains, "one auxiliary stream for GBuffer::render and one per chain");
static_assert(kPlanSmallChains == rs_context::kAux, "the plan's three chains are the context's auxiliary streams");

struct rs_eaw {
    rs_context* ctx = nullptr;
    int width = 0, height = 0, level = 0;
    float sigLumin = 64.f, sigNormal = .2f, sigDepth = 1.f;     // src/denoiser.cu:455
    float* devTempImg = nullptr;
    float* devPos = nullptr;        // per-pixel cam.getPosition(x,y,depth), computed once per filter call
    bool tiled = true;              // levels of step 1, 2, 4 from an LDS tile (k_wavelet_tiled); rs_eaw_set_tiled
    bool fused = true;              // taps in fused arithmetic (denoiser.hip kFusedTaps); rs_eaw_set_fused
};

// SpatioTemporalFilter (src/denoiser.h:45-70); EAWaveletFilter(width, height, 4, 128, 1) (src/denoiser.cu:488)
struct rs_svgf {
    rs_context* ctx = nullptr;
    int width = 0, height = 0, level = 0;
    float sigLumin = 4.f, sigNormal = 128.f, sigDepth = 1.f;
    float* devAccumColor[2] = { nullptr, nullptr };
    float* devAccumMoment[2] = { nullptr, nullptr };
    float* devVariance = nullptr;
    float* devTempColor = nullptr;
    float* devTempVariance = nullptr;
    float* devFilteredVariance = nullptr;
    float* devPos = nullptr;                  // per-pixel cam.getPosition(x,y,depth), once per filter call
    bool firstTime = true;
    int frameIdx = 0;
    bool tiled = true;                        // the a-trous levels from the row-phase LDS tile (k_svgf_wavelet_tiled); rs_svgf_set_tiled
    bool fused = true;                        // taps in fused arithmetic (denoiser.hip svgf_tap_weight FUSED); rs_svgf_set_fused
};

// SpatioTemporalFilter on the rows of a strip (denoiser.hip): `exchange` swaps the first / last `rows` rows of the strip's part of
// image a (ca floats per pixel) -- and of image b when it is not null -- with the strips above and below, into the rows just outside
struct rs_svgf_row_hooks {
    void* ctx;
    int (*exchange)(void* ctx, float* a, int ca, float* b, int cb, int rows);
};
int rs_svgf_filter_rows(rs_svgf* f, float** devColorOut, const float* devColorIn, const rs_gbuffer* g, const rs_camera* cam, int y0, int y1,
                        const rs_svgf_row_hooks* hooks);

rs::CamParams rs_make_cam_params(const rs_camera* cam);

// occlusion_bvh.cpp
int rs_build_occlusion_bvh(int numPrims, const float* primBoxes, std::vector<rs::BvhNode>& nodes, std::vector<int>& leafPrims);
int rs_quantize_occlusion_bvh(const std::vector<rs::BvhNode>& nodes, float base[3], float scale[3], std::vector<unsigned>& out, double* margin = nullptr);
// (rs_grid_over_box: rs_geometry_plan.h)
int rs_build_ordered_bvh(int numPrims, const float* primBoxes, const int* seq, std::vector<rs::BvhNode>& forward, std::vector<rs::BvhNode>& mirrored);
int rs_reference_chain_tables(int bvhSize, const int* order0, std::vector<int>& parent, std::vector<int>& leafOfPrim, int numPrims);
// scene_refit.hip
void rs_refit_free(rs_scene* s);                        // rs_scene_destroy: what the first geometry edit allocated (nothing without one)
// scene_deform.hip (rs_deform.h); null: nothing to do
void rs_parts_free(struct rs_parts* parts);             // rs_scene_destroy, rs_scene_define_parts
void rs_skin_free(struct rs_skin* skin);                // rs_scene_destroy, rs_scene_define_skin
void rs_morph_free(struct rs_morph* morph);             // rs_scene_destroy, rs_scene_define_morph
// scene.hip, for scene_edits.hip as well
// map ids of n materials against a table of numTextures; the two refusal texts carry the entry point's name
int check_materials(int n, const rs_material* m, int numTextures, bool* anyMap,
                    const char* beyond = "rs_scene_create: material map id beyond the texture table",
                    const char* invalid = "rs_scene_create: invalid material map id");
// the light records and alias records of the scene's host arrays
void light_records(const rs_scene* s, float sumInv, rs::LightRec* rec, rs::AliasRec* al);
std::vector<rs::AliasRec> alias_records(const std::vector<float>& prob, const std::vector<int>& fail);
bool far_skip_allowed(const float* vertices, size_t count);   // may skip_far_on_axis (rs_intersect.h) run on a scene with these triangles?
// scene_edits.hip, for rs_scene_destroy and scene_deform.hip as well
int refuse_while_capturing(const char* name);           // edits are not recorded into graphs: RS_ERR_UNSUPPORTED while the library stream is captured
void versions_free(rs_scene* s);                        // what the first edit of materials, lights or textures allocated
void motion_free(rs_scene* s);                          // what rs_scene_set_motion_tracking allocated
