/*
 * restir_hip.h -- C ABI of librestir_hip.so: the MI355X (gfx950) implementation of the ReSTIR-DI
 * per-pixel pipeline and MTBVH traversal of HummaWhite/ReSTIR, behind the reference's own render-pass
 * entry points.  Plain pointers and sizes only; every image / G-buffer pointer is DEVICE memory
 * (hipMalloc), row-major y*W+x, tightly packed float[3] exactly as the reference's glm::vec3 arrays.
 *
 * Each entry point names the reference interface it replaces (paths relative to the reference
 * repository).  The C++ header restir_amd/host/restir_compat.h re-declares the reference's names
 * (GBuffer::render, ReSTIRDirect, copyImageToPBO, ...) on top of this ABI; INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * Return convention: 0 = success, otherwise a hipError_t value (or RS_ERR_*); rs_last_error() gives
 * the message.  (The reference prints and exit()s from checkCUDAError, src/cudaUtil.h:13-31; the
 * compat header reproduces that on top of these codes.)
 *
 * Implicit inputs of the reference launchers (State::looper, Settings::reservoirReuse, the
 * file-static ReSTIRFirstFrame; src/restir.cu:418-446) are explicit parameters / object state here.
 */
#ifndef RESTIR_HIP_H
#define RESTIR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RS_ERR_INVALID_ARGUMENT 10001
#define RS_ERR_UNSUPPORTED      10002   /* e.g. an image or mesh format the scene-file reader does not decode */
#define RS_ERR_INTERNAL         10003   /* a self-check of the library failed (rs_ordered_bvh_host_check) */

/* src/material.h:258-267 -- identical 44-byte layout */
typedef struct rs_material {
    int   type;            /* Material::Type: 0 Lambertian 1 MetallicWorkflow 2 Dielectric 3 Disney 4 Light */
    float baseColor[3];
    float metallic;
    float roughness;
    float ior;
    int   baseColorMapId;  /* -1 NullTextureId, -2 ProceduralTexId (src/material.h:11-13), else index into rs_scene_desc::textures */
    int   metallicMapId;
    int   roughnessMapId;
    int   normalMapId;
} rs_material;

/* src/sceneStructs.h:104-117 -- identical 196-byte layout (glm mat3/mat4 are column-major) */
typedef struct rs_camera {
    int   resolution[2];
    float position[3];
    float rotation[3];
    float view[3];
    float up[3];
    float right[3];
    float fov[2];
    float pixelLength[2];
    float rotationMatInv[9];
    float viewProjection[16];   /* not read by any kernel on this path */
    float lensRadius;
    float focalDist;
    float tanFovY;
} rs_camera;

/* src/restir.h:7-11,114-116 -- Reservoir<DirectLiSample>, identical 36-byte layout */
typedef struct rs_reservoir {
    float Li[3];
    float wi[3];
    float dist;
    int   numSamples;
    float weight;
} rs_reservoir;

/* src/image.h:7-38,76-97 -- a decoded image: linear-RGB float texels, row-major (what Image / DevTextureObj hold;
 * decoding files stays with the caller, as it does with stb_image in the reference, src/image.cpp:14-31) */
typedef struct rs_texture {
    int          width, height;
    const float* data;            /* 3 floats / texel */
} rs_texture;

/* src/restir.h:13-27,114-116 -- Reservoir<IndirectLiSample>, identical 68-byte layout */
typedef struct rs_indirect_reservoir {
    float Lo[3];
    float xv[3], nv[3];
    float xs[3], ns[3];
    int   numSamples;
    float weight;
} rs_indirect_reservoir;

/* Host arrays that define a device scene = the inputs of DevScene::create (src/scene.cpp:435-509),
 * in the layouts Scene::buildDevData leaves them (src/scene.cpp:159-215). */
typedef struct rs_scene_desc {
    int                numPrims;
    const float*       vertices;          /* 9 floats / triangle  (meshData.vertices)  */
    const float*       normals;           /* 9 floats / triangle  (meshData.normals)   */
    const float*       texcoords;         /* 6 floats / triangle  (meshData.texcoords), may be NULL */
    const int*         materialIds;       /* 1 / triangle */
    int                numMaterials;
    const rs_material* materials;
    int                bvhSize;           /* 2*numPrims-1 */
    const float*       boundingBoxes;     /* 6 floats / node: AABB pMin,pMax (src/bvh.h:159-160) */
    const int*         bvhNodes[6];       /* 3 ints / node: MTBVHNode (src/bvh.h:163-171), 6 orders */
    int                numLights;
    const int*         lightPrimIds;
    const float*       lightUnitRadiance; /* 3 / light */
    const float*       lightProb;         /* DiscreteSampler1D::binomDistribs[i].prob   */
    const int*         lightFailId;       /* DiscreteSampler1D::binomDistribs[i].failId */
    float              sumLightPower;     /* lightSampler.sumAll */
    /* Textures and environment map (src/scene.h:78-99,358-392; src/scene.cpp:136-152,479-498).  With an environment
     * map the light sampler has one more entry than there are light primitives (src/scene.cpp:151): numLights
     * counts it, lightProb/lightFailId have numLights entries, lightPrimIds/lightUnitRadiance numLights-1. */
    int                numTextures;
    const rs_texture*  textures;
    int                envMapTexId;        /* Scene::envMapTexId, -1 = none */
    const float*       envMapProb;         /* envMapSampler alias table, width*height entries (NULL without a map) */
    const int*         envMapFailId;
} rs_scene_desc;

typedef struct rs_scene   rs_scene;    /* = Scene::devScene / DevScene      (src/scene.h:64-481)  */
typedef struct rs_gbuffer rs_gbuffer;  /* = GBuffer                          (src/gbuffer.h:15-59) */
typedef struct rs_restir  rs_restir;   /* = module statics of restir.cu      (src/restir.cu:8-18)  */
typedef struct rs_eaw     rs_eaw;      /* = LeveledEAWFilter                 (src/denoiser.h:33-43) */
typedef struct rs_svgf    rs_svgf;     /* = SpatioTemporalFilter             (src/denoiser.h:45-70) */

/* Device pointers of a GBuffer's planes (src/gbuffer.h:41-58): [frameIdx] = this frame's, [frameIdx ^ 1] = last frame's.
 * The library keeps the planes in a ring of five sets (so that the renders of the next frames, which run ahead of the library
 * stream, never overwrite what this frame's temporal pass reads): the pointers are those of the current frame and change at every rs_gbuffer_update -- fetch the
 * view again after it. */
typedef struct rs_gbuffer_view {
    float* devAlbedo;        /* float[3] / px */
    int*   devMotion;
    float* devNormal[2];     /* float[3] / px */
    int*   devPrimId[2];     /* holds the MATERIAL id (lights -2, miss -1), src/gbuffer.cu:29-42 */
    float* devDepth[2];
    int    frameIdx;
    int    width, height;
} rs_gbuffer_view;

/* ---- library ------------------------------------------------------------------------- */
const char* rs_last_error(void);
/* Contexts.  The reference keeps its state in globals (State::scene, Settings::*, one device, the default stream); here that
 * state -- device, stream, synchronous / asynchronous launches, the internal streams of the asynchronous mode -- is a context.
 * Every object (scene, G-buffer, reservoirs, filters, strip driver) belongs to the context that was current in its host thread
 * when it was created, and calls on it run under that context whatever thread makes them, so several host threads, devices or
 * launch modes can use the library side by side.  A caller that never creates one uses the default context (the reference's
 * single-threaded viewer does); rs_init and the rs_set_* calls below configure the CURRENT context of the calling thread.
 * Objects handed to one call (scene + G-buffer + reservoirs) must belong to one context. */
typedef struct rs_context rs_context;
int  rs_context_create(int device, rs_context** ctx);
int  rs_context_destroy(rs_context* ctx);           /* after the objects created under it */
int  rs_context_set_current(rs_context* ctx);       /* for the calling thread; NULL = back to the default context */
/* Selects the HIP device of the default context (hipSetDevice). */
int  rs_init(int device);
/* All work is enqueued on this hipStream_t (NULL = default stream). */
int  rs_set_stream(void* hipStream);
/* The streams the library makes for itself in overlapped mode (three: the chains of consecutive frames and the render) are CHOSEN BY
 * MEASUREMENT when first needed, and again after rs_set_stream: whether four streams of a process run side by side depends on every
 * stream the process has made before (torch's pool, an ncclComm's own), so candidates of every priority level are timed next to the
 * caller's stream and the best three kept (about 25 ms, once, with the device idle; internal_streams.hip).  This call names the PREFERRED level
 * among those that measure equal: 2 (default) = automatic, above the caller's stream first; -1 high / 0 normal / 1 low first.  A caller
 * that runs a denoiser on the library stream every frame does 5 % better with 1 (config 5: 1.87 -> 1.78 ms).  Before the first frame. */
int  rs_set_internal_stream_priority(int level);
/* What the measurement chose: level, the chosen streams' calibration time and the fastest candidate's (us; 0 = plain streams in use). */
int  rs_internal_streams_info(int* priority, double* chosenUs, double* fastestUs);
/* Chooses them again at the next overlapped launch (waits for the library's work): call after the process has made streams of its own
 * since the library's first overlapped frame -- in particular after ncclCommInitRank, which makes several. */
int  rs_choose_internal_streams_again(void);
/* Makes the choice now instead of at the first overlapped launch (about 25 ms; waits for the caller's stream and the candidates, not for
 * the device) -- for a caller that wants no pause inside its first frame.  A choice is kept per caller stream and preference: rs_set_stream
 * back to a stream the library has measured next to takes that choice again.  While the caller's stream is being captured into a graph
 * nothing is measured: plain streams. */
int  rs_prepare_streams(void);
/* 1 (default): every entry point synchronises and checks errors before returning, like
 * checkCUDAError after each launch in the reference.  0: launches are only enqueued. */
int  rs_set_sync(int sync);
/* With rs_set_sync(0), frames overlap: GBuffer::render goes to an internal stream, the primary-ray -> RIS -> shadow-ray kernels of
 * ReSTIRDirect to two more, frames taking them in turn (a full-size frame's shadow rays stay on the library stream; a frame that
 * fills the chip less than three times over -- a strip -- renders in the same launch as its primary rays and has three such chains); each is
 * ordered only after the work that last used its buffers (G-buffer planes in a ring of five, per-frame surface planes in
 * four sets) and joined into the library stream where its results are first read (the temporal pass, the denoisers,
 * rs_gbuffer_get_view, rs_synchronize).  They then run next to the previous frames' temporal / spatial
 * passes.  Results are identical; output buffers are valid in library-stream order as before.  GBuffer::render can in addition
 * be deferred until ReSTIRDirect, which then walks the pixel-centre ray and the jittered ray of every pixel in one traversal:
 * faster or slower by a few percent depending on the scene and the launch size, so by default
 * every rs_restir measures the frame period both ways once per scene (frames 6..17 against 22..33) and keeps the faster.
 *   0 = everything on the library stream (RS_SIDE_STREAM=0 in the environment pre-sets this: the profiling scripts use it)
 *   1 = overlapped frames, the render always its own launch
 *   2 = overlapped frames, the render always deferred for launches of at least three rounds of the chip's wave slots
 *   3 = like 2 for launches of any size
 *   4 = overlapped frames, measured choice (the default) */
int  rs_set_side_stream(int enable);
/* The RIS pass keeps the light table (up to 1 024 lights) in LDS, one copy per 1 024-thread block; a launch of fewer than `pixels`
 * pixels reads it from global memory in 256-thread blocks instead, which spread evenly over the CUs (default 64 Ki pixels: a quarter
 * of the CUs with a block; rounds 2-4 had 384 Ki, which cost every rank of an 8-way split of 1080p 1-13 % of its frame period once the
 * library's streams no longer shared hardware queues).  Same results either way; 0 = always LDS. */
int  rs_set_ris_table_pixels(int pixels);
/* How the overlapped mode spreads a frame's kernels over the internal streams (a setting of the current context; every argument
 * -1 = keep).  chainStreams 1 / 2: the primary-ray -> RIS -> shadow-ray chains of all frames on one stream, or of alternating frames on
 * two (default 2).  smallChains 0 / 1: a launch below three rounds of the chip's wave slots (a strip) takes the fused render and rotates
 * its chains over three streams (default 1).  shadowOnMain 0 / 1 / 2: the shadow rays never / always / for launches of at least three
 * rounds of wave slots (default 2) on the library stream.  Results are identical in every setting (tools/soak_async.py); the defaults
 * are what measured fastest.
 * No entry point waits on the host in overlapped mode: the measurement of rs_set_side_stream's mode 4 polls its last time stamp
 * (hipEventQuery at the frame ends) and frames take two launches until it has arrived. */
int  rs_set_stream_plan(int chainStreams, int smallChains, int shadowOnMain);
/* A denoiser in the loop (src/main.cpp:160-170: LeveledEAWFilter::filter between ReSTIRDirect and copyImageToPBO) makes the library
 * stream both the one chain that links consecutive frames and the busiest stream (config 5: 98 % busy, the chain streams 51-57 %).
 * 1: with rs_set_sync(0), rs_eaw_filter / rs_strips_eaw_filter -- and an rs_copy_image_to_pbo / rs_strips_gather_begin that reads their
 * result -- are enqueued on a stream of the library, ordered after everything enqueued on the library stream so far, and run next to the
 * NEXT frame's temporal and spatial passes; the chains of the frames then take turns on two internal streams instead of three (four
 * streams with work in flight is what the device runs side by side).  Results are identical.  What changes is the ORDER CONTRACT of
 * those calls' outputs (the filtered image, the display buffer, the gathered image): they are ordered for the library stream by events,
 * which every library call that is handed one of those buffers waits for by itself, and which rs_join_denoise_stream() (enqueue-only)
 * or rs_synchronize() hand to the caller's own work on that stream -- a caller that reads the display buffer with its own kernels or
 * copies calls rs_join_denoise_stream() first (rs_pbo_unmap does).  0 (default): everything in library-stream order. */
int  rs_set_denoise_stream(int enable);
/* The library stream waits (on the device; the host does not) for everything enqueued on the denoise stream so far. */
int  rs_join_denoise_stream(void);
/* Closest-hit kernels (GBuffer::render, the primary rays of ReSTIRDirect): a tile whose packet walk visited at least `threshold`
 * nodes the last time the same launch ran is traced by four waves of 16 rays instead of one of 64 -- a launch that runs alone lasts
 * as long as its longest chain of node fetches; results do not depend on the grouping.  Applies where launches run one after the
 * other (synchronous mode, per-pass timing); 0 = off; negative = |threshold| for every launch, also with the frames overlapped
 * (measured slower there); default 768. */
int  rs_set_tile_split(int threshold);
/* Test hook: waits as rs_synchronize does, then reports how many tiles the helper blocks of the most recent split launch took over (the
 * tiles the launch before it listed as heavy), the largest figure over the launch sites of the G-buffer (GBuffer::render as its own
 * launch) and of the ReSTIR object (primary rays, alone or in one launch with the render).  0: no split launch has run there, or none that
 * found a tile listed.  Either object and either output may be NULL.  It tells a test that set a low threshold whether the four-wave
 * form really ran. */
int  rs_debug_split_tiles(const rs_gbuffer* gbuffer, const rs_restir* restir, unsigned* renderTiles, unsigned* primaryTiles);
int  rs_synchronize(void);

/* ---- host scene build: replaces Scene::buildDevData (src/scene.cpp:159-215) ----------- */
/* BVHBuilder::build + buildMTBVH (src/bvh.cpp:10-202).  boundingBoxes: 6*(2n-1) floats;
 * bvhNodes[k]: 3*(2n-1) ints each.  Returns BVHSize via *bvhSize. */
int  rs_build_bvh(int numPrims, const float* vertices, float* boundingBoxes, int* const bvhNodes[6], int* bvhSize);
/* light table of buildDevData (src/scene.cpp:161-190); arrays sized numPrims. */
int  rs_build_light_table(int numPrims, const float* vertices, const int* materialIds,
                          int numMaterials, const rs_material* materials, int* numLights,
                          int* lightPrimIds, float* lightUnitRadiance, float* lightPower);
/* DiscreteSampler1D<float> constructor (src/sampler.h:79-121). */
int  rs_build_alias_table(int n, const float* values, float* prob, int* failId, float* sumAll);
/* The whole of buildDevData on a baked triangle soup: light table, alias table, BVH, upload. */
int  rs_scene_build(int numPrims, const float* vertices, const float* normals, const float* texcoords,
                    const int* materialIds, int numMaterials, const rs_material* materials,
                    rs_scene** scene);
/* The same with textures and an environment map: adds Scene::createLightSampler's environment-map sampler
 * (src/scene.cpp:136-152).  envMapTexId: index into textures or -1. */
int  rs_scene_build_textured(int numPrims, const float* vertices, const float* normals, const float* texcoords,
                             const int* materialIds, int numMaterials, const rs_material* materials,
                             int numTextures, const rs_texture* textures, int envMapTexId, rs_scene** scene);
/* pdf of the environment-map sampler: lum(texel) * sin((.5 + row) / height * Pi) (src/scene.cpp:139-146). */
int  rs_build_envmap_pdf(int width, int height, const float* data, float* pdf);
/* DevScene::create (src/scene.cpp:435-509) from prebuilt host arrays. */
int  rs_scene_create(const rs_scene_desc* desc, rs_scene** scene);
/* Host copies of the arrays the scene was created from (valid until rs_scene_destroy). */
int  rs_scene_host_desc(const rs_scene* scene, rs_scene_desc* desc);
/* DevScene::sampleSequence (src/scene.h:480; src/scene.cpp:500-506 reads "sobol_10k_200.bin" into it): the table of the Sobol
 * sampler, numSamples x numDims uint32 in row order (sample index, then dimension), numDims = 200 (SobolSampleDim, src/sampler.h:11;
 * the reference's table has SobolSampleNum = 10 000 rows).  The reference picks its sampler at compile time (SAMPLER_USE_SOBOL,
 * src/common.h:4); here the scene carries the choice: once a table is set, every pass that draws random numbers (ReSTIRDirect,
 * ReSTIRIndirect, pathTrace*) runs the Sobol branch of src/sampler.h:9-36 -- Sampler(looper * 200 + dim, utilhash(index), data),
 * sample() = (data[ptr++] ^ scramble) * 2^-32, scramble = utilhash(scramble) -- and data == NULL selects the default thrust engine
 * (src/sampler.h:38-49) again.  In Sobol mode `looper` must stay in [0, numSamples): the caller wraps it as the reference does,
 * State::looper = (State::looper + 1) % SobolSampleNum (src/restir.cu:441-445; restir_compat.h does).  The table is copied. */
int  rs_scene_set_sample_sequence(rs_scene* scene, const uint32_t* data, int numSamples, int numDims);
/* Emission (baseColor) of Light-type materials.  Host arrays: count material ids, 3 floats each.  Enqueued on the
 * library stream; does not synchronize the device.  The light table and alias table are rebuilt as rs_scene_build does
 * (the environment map's entry keeps its power), so that the scene equals one built afresh from the edited materials:
 * rs_scene_host_desc returns the new materials, lightUnitRadiance, lightProb, lightFailId and sumLightPower.  On the
 * device the tables go to the next of a small ring of versions: launches enqueued before the call (frames in flight,
 * a G-buffer render recorded but not launched yet) read the old emission, launches after it the new one -- G-buffer
 * albedo, RIS, pathTraceDirect, pathTrace*, ReSTIRIndirect.  The host waits only when the ring runs out, i.e. when a
 * launch that read the version eight edits back has not finished.  Refused with RS_ERR_INVALID_ARGUMENT, the scene
 * unchanged: count < 0, an id out of range or of a material that is not a Light, a negative, NaN or infinite
 * radiance, an edit that leaves the light sampler without a positive total power; with RS_ERR_UNSUPPORTED while the
 * library stream is being captured into a graph (captured frames keep the emission they were captured with).
 * Textured emission and the emitters' geometry are not edited; the environment map is edited by
 * rs_scene_set_texture. */
int  rs_scene_set_emission(rs_scene* scene, int count, const int* materialIds, const float* radiance);
/* Material records of materials that are not Lights.  Host arrays: count material ids and count full rs_material structs, copied as
 * they are (no range checks on the values; a repeated id: the last record wins; count == 0 succeeds and changes nothing).  Ordered
 * exactly as rs_scene_set_emission, in the same ring of versions, so that calls of both kinds stay in order: no device
 * synchronisation, a render that has only been recorded is launched first with the old records, launches enqueued before the call read
 * the old records and launches after it the new ones, and the host waits only when the ring runs out.  The type may change among
 * Lambertian, MetallicWorkflow, Dielectric and Disney (0..3); map ids follow the rules of rs_scene_create against the scene's texture
 * table.  A scene that had no map and no environment map takes its first map here (the procedural one, -2, included): the texture
 * coordinates kept on the host are uploaded then.  Afterwards rs_scene_host_desc returns the new records and the scene renders, bit for
 * bit, like one built afresh from the edited materials; any accepted edit invalidates retained G-buffer planes (base colour and its map
 * feed the albedo plane, the normal map the normal plane).  Refused with RS_ERR_INVALID_ARGUMENT, the scene unchanged: count < 0 or
 * null arrays with count > 0, an id out of range, a material that is a Light now or would become one (the light list, the emissive
 * tree and the G-buffer's -2 ids depend on which materials are Lights; emission stays with rs_scene_set_emission), a bad map id, a
 * first map on a scene created with texcoords == NULL; with RS_ERR_UNSUPPORTED while the library stream is being captured.
 * ReSTIR's temporal reservoirs keep weights drawn under the old BSDF for up to the M clamp's 20 frames, as in the reference;
 * rs_restir_reset drops them. */
int  rs_scene_set_materials(rs_scene* scene, int count, const int* materialIds, const rs_material* records);
/* Triangles: the three vertices (9 floats) and, unless normals is NULL, the three vertex normals (9 floats) of count primitives.  Host
 * arrays, copied before the call returns (through a small ring of pinned staging buffers: the host waits only when that ring is full
 * of edits whose copies have not finished).  The topology of every tree is kept -- the six bvhNodes orders do not change -- and every
 * box is refitted on the device: a leaf box is AABB(va, vb, vc) (src/bvh.h:20-21), an inner box the union of its two children, as
 * rs_refit_boxes computes them.  Afterwards rs_scene_host_desc returns the edited vertices and normals and boundingBoxes equal to
 * rs_refit_boxes of the edited vertices, everything else as before, and the scene renders, in every kernel, bit for bit like
 * rs_scene_create of that description.  A scene created from caller-supplied boxes that were not exact unions has ALL of them replaced
 * by exact unions by its first edit (scenes from rs_scene_build / rs_build_bvh already hold exact unions).
 * Ordering as rs_scene_set_materials, except that geometry is edited in place behind device-side fences instead of in the ring of
 * versions: no device synchronisation; a render that has only been recorded is launched first, with the old geometry; the library
 * stream waits, by events, for what the library's internal streams have been handed so far, the refit runs on the library stream, and
 * the next launch of every internal stream waits for it -- launches enqueued before the call read the old geometry, launches after
 * it the new.  The first edit of a scene builds and uploads the refit's tables and waits for the device once.  Every edit refits the
 * whole scene, O(numPrims) on the device, however few triangles it names, unless rs_scene_set_partial_refit (below) has been switched
 * on (DESIGN.md section 3 has the cost of both).  An
 * accepted edit invalidates retained G-buffer planes.  A repeated id takes its last record; count == 0 succeeds and changes nothing.
 * Refused with RS_ERR_INVALID_ARGUMENT, the scene unchanged: count < 0 or null arrays with count > 0; an id out of range; a vertex or
 * normal that is not finite; a triangle whose material is a Light (this is the call that guarantees that the light sampler, the light
 * records and the emissive tree are untouched; rs_scene_set_geometry moves emitters); and, while the scene has its shadow-ray tree, a vertex outside the root box the scene was created with (the trees' 16-bit grid lies over that box).  With
 * RS_ERR_UNSUPPORTED while the library stream is being captured into a graph.  A large deformation makes the refitted trees slower,
 * never wrong; the remedy is a new scene.  The G-buffer's motion plane follows moved triangles on a scene that tracks motion
 * (rs_scene_set_motion_tracking below) and is camera-only otherwise. */
int  rs_scene_set_triangles(rs_scene* scene, int count, const int* primIds, const float* vertices, const float* normals);
/* rs_scene_set_triangles that also takes triangles whose material is a Light, alone or mixed with others in one call: arguments,
 * staging, fences, refit and "a repeated id takes its last record" are the same, and a call that names no emitter does exactly what
 * rs_scene_set_triangles does (no version of the ring is consumed, no byte of the emissive tree is written).  A call that names an
 * emitter in addition
 *   - rebuilds the light sampler as rs_scene_build_textured builds it: rs_build_light_table's powers (the new areas) over the same
 *     light primitives in the same order, the environment map's entry last with its power kept, then rs_build_alias_table;
 *   - fills the next slot of the ring of versions (rs_scene_set_emission) with light records of the new vertices, normal and pdfArea;
 *   - refits the tree of the emissive triangles that answers the last bounce of a path, on a grid laid anew over the new emissive root
 *     box by the function a fresh build uses, so that the grid equals that of rs_scene_create of the edited description.
 * Afterwards rs_scene_host_desc returns the edited vertices and normals, boundingBoxes equal to rs_refit_boxes of them, and lightProb,
 * lightFailId and sumLightPower as just described (lightPrimIds and lightUnitRadiance do not change: the set of emitters is the same),
 * and the scene renders, in every kernel, bit for bit like rs_scene_create of that description.
 * Both transitions are made at one point of the library stream: launches enqueued before the call read the old geometry and the old
 * lights, launches after it the new of both.  The host waits only where rs_scene_set_triangles and rs_scene_set_emission wait (a full
 * staging ring, a version ring that has run out).
 * An emitter may flip, may become degenerate (a point or three collinear vertices: power 0) and may move anywhere inside the root box
 * the scene was created with.  When all emitters collapse into a box without extent the emissive tree is switched off, as a fresh build
 * leaves it off, until an edit brings an extent back.  (A scene CREATED with such emitters has no emissive tree and gets none.)
 * Refused with RS_ERR_INVALID_ARGUMENT, the scene unchanged: everything rs_scene_set_triangles refuses except emitters, and an edit that
 * leaves the light sampler without a finite, positive total power.  RS_ERR_UNSUPPORTED while the library stream is being captured.
 * Temporal reservoirs keep the direction, distance and radiance they were drawn with for up to the M clamp's 20 frames, as in the
 * reference; rs_restir_reset drops them, and rs_restir_set_light_retargeting evaluates the samples of the moved lamps again instead.
 * Adding or removing emitters still takes a new scene. */
int  rs_scene_set_geometry(rs_scene* scene, int count, const int* primIds, const float* vertices, const float* normals);
/* How many accepted geometry edits (rs_scene_set_geometry, rs_scene_set_part_transforms) have named an emitter so far.  Host only: no
 * wait, no launch.  An edit that names no emitter does not count.  (Per light: RS_TABLE_LIGHT_MOVED of rs_debug_scene_table.) */
int  rs_scene_light_moves(const rs_scene* scene, unsigned long long* moves);
/* Rigid parts: sets of triangles that each move by one matrix (a door, a prop, a swinging lamp), with a rest pose the scene keeps on the
 * host and on the device.  (The reference has no moving geometry: there is no reference line to cite.)
 * rs_scene_define_parts: partFirst holds numParts + 1 offsets into primIds (0 first, non-decreasing; an empty part is allowed), primIds
 * the parts' primitives, emitters among them if wanted, no primitive twice; restVertices / restNormals hold 9 floats per listed primitive
 * in the order of primIds, or are both NULL: the rest pose is then the scene's pose as rs_scene_host_desc returns it at the call.  All arrays
 * are copied: ids and rest pose to the host and to the device (72 bytes per listed triangle), the offsets to the host (a transform carries
 * each named part's range to the device itself).  The call renders nothing and changes no geometry.  Calling it again replaces the definition;
 * numParts == 0 drops it and frees the arrays.  Ordering: a definition that replaces or drops an earlier one waits for the device, as the
 * first edit of a scene does, so a transform enqueued earlier keeps the old tables and a later one finds the new.
 * Refused with RS_ERR_INVALID_ARGUMENT, the definition unchanged: a null scene, numParts < 0, null or bad offsets, an id out of range, a
 * primitive listed twice (in one part or in two), exactly one of the two rest arrays NULL, a rest value that is not finite; with
 * RS_ERR_UNSUPPORTED while the library stream is being captured into a graph.
 * rs_scene_set_part_transforms: matrices16 holds one column-major 4x4 per entry of partIds.  The call does what
 * rs_scene_set_geometry(scene, m, ids, v, n) does, where ids are the primitives of the named parts in the order of the call (a part named
 * twice keeps its place and takes its last matrix) and v, n are rs_bake_matrix of each part's matrix over its rest arrays: the same
 * refusals with the scene unchanged (a baked vertex or normal that is not finite, e.g. from a singular matrix; a vertex outside the
 * creation-time root box; a light sampler left without finite positive power; RS_ERR_UNSUPPORTED while captured), the same
 * rs_scene_host_desc and the same device tables afterwards, lights moved the same way, retained G-buffer planes invalidated, the
 * previous pose of a tracked scene left alone, the same fences at the same point of the library stream.  Only the source of the records
 * differs: the host stages one 112-byte record per named part (the matrix, the normal matrix computed once on the host with GLM's inverse,
 * the part's range in the rest arrays, its offset in the output) through the ring of pinned buffers, and a kernel writes the
 * ids | vertices | normals the refit reads from the device's rest pose, with the arithmetic of rs_bake_matrix, bit for bit.  The host
 * still bakes the named triangles once itself: for the checks above, the light areas, and the tables rs_scene_host_desc returns.
 * The rest pose is never written and transforms do not accumulate: a matrix always acts on the rest pose, so rounding does not drift over
 * any number of frames.  rs_scene_set_triangles / rs_scene_set_geometry on a part's triangle is allowed and moves it until the next
 * transform of that part puts it back on the baked rest pose.  count == 0, or only empty parts, succeeds and changes nothing.
 * Additionally refused with RS_ERR_INVALID_ARGUMENT: no parts defined, a part id out of range, null arrays with count > 0.
 * INTEGRATION.md section 3f has the frame loop; DESIGN.md section 3 the cost (the refit is the whole scene's unless
 * rs_scene_set_partial_refit is on). */
int  rs_scene_define_parts(rs_scene* scene, int numParts, const int* partFirst, const int* primIds, const float* restVertices, const float* restNormals);
int  rs_scene_set_part_transforms(rs_scene* scene, int count, const int* partIds, const float* matrices16);
/* Host only: the number of parts and of primitives listed in them (0, 0: none defined).  Either pointer may be NULL. */
int  rs_scene_parts_info(const rs_scene* scene, int* numParts, int* numListedPrims);
/* Test hooks.  rs_scene_download_part_rest waits as rs_synchronize does, then copies the DEVICE copies of the parts' primitive ids and
 * rest pose out (sizes: rs_scene_parts_info; any array may be NULL).  RS_ERR_INVALID_ARGUMENT: a null scene, or no parts defined;
 * RS_ERR_UNSUPPORTED while the library stream is being captured.  rs_debug_scene_staged_bytes: the bytes the most recent accepted
 * geometry edit of either kind copied from the host to the device (0 before the first); host only. */
int  rs_scene_download_part_rest(const rs_scene* scene, int* primIds, float* restVertices, float* restNormals);
int  rs_debug_scene_staged_bytes(const rs_scene* scene, size_t* bytes);
/* Skinned meshes: triangles whose corners follow a blend of bone matrices (a character, a flag, a cable), with a rest pose, four bone ids
 * and four weights per corner that the scene keeps on the host and on the device, and a palette of bone matrices the caller poses.  (The
 * reference has no moving geometry: there is no reference line to cite.)
 * rs_skin_corners is the skinning counterpart of rs_bake_matrix, host only, no GPU call: n corners (3 floats each in and out), 4 bone ids
 * and 4 weights per corner, numBones column-major 4x4 matrices.  With p_k and q_k the position and the not yet normalised normal that
 * rs_bake_matrix computes for the matrix of the corner's k-th bone,
 *     position = (w0 * p0 + w1 * p1) + (w2 * p2 + w3 * p3)  per component,  normal = normalize((w0 * q0 + w1 * q1) + (w2 * q2 + w3 * q3)),
 * one rounding per operation; the normal matrix is computed once per matrix with GLM's inverse.  All four influences are always evaluated
 * (a slot of weight 0 still names a valid bone) and the weights are used as given, not renormalised.  Non-finite results are returned, not
 * refused.  RS_ERR_INVALID_ARGUMENT: numBones < 1, null matrices, a null array with n > 0, a bone id outside [0, numBones). */
#define RS_SKIN_MAX_BONES 256   /* 28 KB of palette */
int  rs_skin_corners(int numBones, const float* matrices16, size_t n, const float* vertsIn, const float* normalsIn,
                     const int* boneIds4, const float* weights4, float* vertsOut, float* normalsOut);
/* rs_scene_define_skin: primIds[numListed] are the skinned primitives, emitters among them if wanted, no primitive twice; restVertices /
 * restNormals hold 9 floats per listed primitive in the order of primIds, or are both NULL: the rest pose is then the scene's pose as
 * rs_scene_host_desc returns it at the call; boneIds / weights hold 12 values per listed primitive, corner-major, 4 per corner.  (The
 * reference has no moving geometry: there is no reference line to cite.)  Everything is copied, to the host and to the device (4 + 72 + 96
 * bytes per listed triangle); the device copy is read by the skinning kernel alone and never written afterwards.  The call renders
 * nothing and changes no geometry.  The host palette starts as numBones identities.  Calling it again replaces the definition and the
 * palette; numBones == 0 with numListed == 0 drops it and frees the arrays.  Ordering is rs_scene_define_parts': a definition that
 * replaces or drops an earlier one waits for the device.  A skin and parts may coexist and may name the same primitive: as with
 * rs_scene_set_geometry on a part's triangle, the last edit wins.
 * Refused with RS_ERR_INVALID_ARGUMENT, the definition unchanged: a null scene, numBones < 0 or above RS_SKIN_MAX_BONES, numListed < 0 or
 * triangles without a bone, null ids, bone ids or weights with numListed > 0, a primitive id out of range or listed twice, exactly one of
 * the two rest arrays NULL, a rest value or a weight that is not finite, a negative weight, a corner whose four weights are all 0, a bone
 * id outside [0, numBones); with RS_ERR_UNSUPPORTED while the library stream is being captured into a graph. */
int  rs_scene_define_skin(rs_scene* scene, int numBones, int numListed, const int* primIds,
                          const float* restVertices, const float* restNormals, const int* boneIds, const float* weights);
/* rs_scene_set_bone_transforms: matrices16 holds one column-major 4x4 per entry of boneIds.  The named bones take their new matrix (a bone
 * named twice takes its last, bones not named keep the matrix they had), and the call then does exactly what
 * rs_scene_set_geometry(scene, numListed, primIds, v, n) does with v, n = rs_skin_corners of the whole palette over the rest arrays: the
 * same refusals with the scene AND THE PALETTE unchanged (a skinned vertex or normal that is not finite, a vertex outside the
 * creation-time root box, a light sampler left without finite positive power, RS_ERR_UNSUPPORTED while captured), the same
 * rs_scene_host_desc and device tables afterwards, lights moved and rs_scene_light_moves counted the same way, the same dirty box, the
 * partial or whole refit rs_scene_set_partial_refit decides, retained G-buffer planes invalidated, the previous pose of a tracked scene
 * left alone, the same fences at the same point of the library stream.  (The reference has no moving geometry: there is no reference line
 * to cite.)  Only the source of the records differs: the host stages the palette, numBones 112-byte records (the matrix and its normal
 * matrix), through the ring of pinned buffers, and a kernel writes the ids | vertices | normals the refit reads from the device's rest
 * arrays, with the arithmetic of rs_skin_corners, bit for bit.  As for parts, the host still skins the listed triangles once itself: for
 * the checks above, the light areas, and the tables rs_scene_host_desc returns.  The rest arrays are never written and poses do not
 * accumulate.  count == 0 succeeds and changes nothing.  Additionally refused with RS_ERR_INVALID_ARGUMENT: no skin defined, a bone id
 * out of range, null arrays with count > 0.  INTEGRATION.md section 3i has the frame loop; DESIGN.md section 3 the cost. */
int  rs_scene_set_bone_transforms(rs_scene* scene, int count, const int* boneIds, const float* matrices16);
/* Host only: the number of bones and of primitives the skin lists (0, 0: none defined).  Either pointer may be NULL.  (The reference has
 * no moving geometry: there is no reference line to cite.) */
int  rs_scene_skin_info(const rs_scene* scene, int* numBones, int* numListedPrims);
/* Test hook.  Waits as rs_synchronize does, then copies the DEVICE copies of the skin's primitive ids, rest pose, bone ids and weights
 * out (sizes: rs_scene_skin_info; any array may be NULL).  RS_ERR_INVALID_ARGUMENT: a null scene, or no skin defined;
 * RS_ERR_UNSUPPORTED while the library stream is being captured.  (The reference has no moving geometry: there is no reference line to
 * cite.) */
int  rs_scene_download_skin(const rs_scene* scene, int* primIds, float* restVertices, float* restNormals, int* boneIds, float* weights);
/* Morph targets (blend shapes): per-corner position and normal deltas on a rest pose, summed by weight -- a face, a muscle, a wrinkle --
 * alone or, on a skinned mesh, in front of the bones.  The deltas stay on the device; an edit carries weights.  (The reference has no
 * moving geometry: there is no reference line to cite.)
 * The caller's table is by target, glTF's sparse form: targetFirst[numTargets + 1] are offsets (0 first, non-decreasing) into
 * entryCorner[] -- the index of a listed corner, listedIndex * 3 + corner --, deltaPositions[3 per entry] and deltaNormals[3 per entry]
 * (or NULL: zeros).  The library keeps it by corner, each corner's entries in ascending target id (32 bytes an entry and 4 per corner on
 * the device), which fixes the order of every corner's sum.
 * rs_morph_corners is the host function, no GPU call: n corners (3 floats each in and out), the table over those n corners, numTargets
 * weights.  Per corner, with its entries in ascending target id:
 *     p = v; q = n;  for each entry whose weight w[target] != 0 (-0 and +0 both skip):  p = p + w * dp,  q = q + w * dn  per component,
 *     position = p;  normal = normalize(q) if any entry was applied, else n
 * one multiply and one add per component and entry.  A corner without an applied entry returns its rest bits: all weights 0 is the rest
 * pose exactly.  Weights and deltas are used as given (negative, above 1, denormal); non-finite results are returned, not refused.
 * RS_ERR_INVALID_ARGUMENT: numTargets < 0 or above RS_MORPH_MAX_TARGETS, a null array that is needed, offsets that do not start at 0 or
 * that decrease, a corner index outside [0, n), a (target, corner) pair listed twice. */
#define RS_MORPH_MAX_TARGETS 256   /* 1 KB of weights */
int  rs_morph_corners(int numTargets, const int* targetFirst, const int* entryCorner, const float* deltaPositions, const float* deltaNormals,
                      const float* weights, size_t n, const float* vertsIn, const float* normalsIn, float* vertsOut, float* normalsOut);
/* rs_scene_define_morph: a morph with a rest pose of its own.  primIds[numListed], restVertices / restNormals are rs_scene_define_skin's
 * (both NULL: the scene's pose at the call); the table is over the numListed * 3 listed corners.  Everything is copied, to the host and
 * to the device; the device copies are read by the morph kernel alone and never written afterwards.  The call renders nothing and changes
 * no geometry.  Weights start at 0.  Calling it again replaces the definition and the weights; numTargets == 0 with numListed == 0 drops
 * it.  A definition that replaces or drops an earlier one waits for the device.  The scene's morph, parts and a skin may name the same
 * primitive: the last edit wins.
 * rs_scene_define_skin_morph: a morph on the corners the skin lists, held by the skin and evaluated BEFORE its bones.  It needs a skin;
 * rs_scene_define_skin called again, or dropping the skin, drops it as well; numTargets == 0 drops it alone.
 * Both refuse with RS_ERR_INVALID_ARGUMENT, the definition unchanged: a null scene, numTargets < 0 or above RS_MORPH_MAX_TARGETS, null or
 * bad offsets, a corner index out of range, a (target, corner) pair listed twice, a delta that is not finite; rs_scene_define_morph also
 * what rs_scene_define_skin refuses of the listed primitives and the rest arrays, and triangles without a target; rs_scene_define_skin_morph
 * a scene without a skin.  RS_ERR_UNSUPPORTED while the library stream is being captured into a graph. */
int  rs_scene_define_morph(rs_scene* scene, int numTargets, int numListed, const int* primIds, const float* restVertices, const float* restNormals,
                           const int* targetFirst, const int* entryCorner, const float* deltaPositions, const float* deltaNormals);
int  rs_scene_define_skin_morph(rs_scene* scene, int numTargets, const int* targetFirst, const int* entryCorner, const float* deltaPositions,
                                const float* deltaNormals);
/* rs_scene_set_morph_weights: the named targets of the scene's own morph take their new weight (a target named twice takes its last, one
 * not named keeps its weight), and the call then does exactly what rs_scene_set_geometry(scene, numListed, primIds, v, n) does with v, n =
 * rs_morph_corners of all weights over the rest arrays: the same refusals with the scene AND THE WEIGHTS unchanged, the same
 * rs_scene_host_desc and device tables afterwards, lights moved the same way, the same dirty box, the partial or whole refit, retained
 * G-buffer planes invalidated, the same fences.  Only the source of the records differs: the host stages the weights as whole 112-byte
 * records, 28 floats each, zero-padded -- ceil(numTargets / 28) of them -- and a kernel writes the ids | vertices | normals the refit
 * reads from the device's rest arrays and table, with the arithmetic of rs_morph_corners, bit for bit.  The host still morphs the listed
 * triangles once itself (checks, light areas, rs_scene_host_desc).  Every call evaluates every listed triangle.  Weights must be finite;
 * count == 0 succeeds and changes nothing.  Additionally refused with RS_ERR_INVALID_ARGUMENT: no morph defined, a target id out of
 * range, null arrays with count > 0.
 * rs_scene_set_skin_pose names bones and targets of the skin and its morph and makes ONE edit of them: v, n = rs_skin_corners of the whole
 * palette over rs_morph_corners of all weights over the rest arrays, evaluated per corner by one kernel.  It stages the numBones bone
 * records, then the weight records.  Palette and weights become the scene's together, or neither does.  On a skin with a morph
 * rs_scene_set_bone_transforms is this call with targetCount = 0 (the weights stay); on a skin without one, rs_scene_set_bone_transforms
 * stages and launches what it always did and this call with targetCount > 0 is refused.  boneCount == 0 with targetCount == 0 changes
 * nothing.  INTEGRATION.md section 3k has the frame loop; DESIGN.md section 3 the cost. */
int  rs_scene_set_morph_weights(rs_scene* scene, int count, const int* targetIds, const float* weights);
int  rs_scene_set_skin_pose(rs_scene* scene, int boneCount, const int* boneIds, const float* matrices16,
                            int targetCount, const int* targetIds, const float* weights);
/* Host only.  which: 0 the scene's own morph, 1 the skin's: targets, listed primitives and entries (0, 0, 0: none defined; any pointer
 * may be NULL).  RS_ERR_INVALID_ARGUMENT: a null scene, which neither 0 nor 1. */
int  rs_scene_morph_info(const rs_scene* scene, int which, int* numTargets, int* numListedPrims, int* numEntries);
/* Test hook.  Waits as rs_synchronize does, then copies the DEVICE copies out: cornerFirst[numListedPrims * 3 + 1], the numEntries 32-byte
 * entry records { int target; float dp[3]; float dn[3]; int pad; } and, for which = 0, the morph's primitive ids and rest pose (for
 * which = 1 those three must be NULL: rs_scene_download_skin has the skin's).  Any array may be NULL.  RS_ERR_INVALID_ARGUMENT: a null
 * scene, no such morph defined; RS_ERR_UNSUPPORTED while the library stream is being captured. */
int  rs_scene_download_morph(const rs_scene* scene, int which, int* primIds, float* restVertices, float* restNormals, int* cornerFirst, void* entries);
/* What a geometry edit of any of the three kinds decides on the host before it touches the device, as functions of plain arrays and
 * integers (restir_amd/csrc/rs_geometry_plan.h).  The view is what they read of a scene; flags are 0 / 1. */
typedef struct rs_geometry_edit_view {
    int numPrims;
    const int* materialIds;         /* [numPrims] */
    const rs_material* materials;   /* a triangle is an emitter when its material's type is Light */
    int bounded;                    /* the scene has grid-box trees: a vertex must stay inside [gridLo, gridHi], the creation-time root box */
    float gridLo[3], gridHi[3];
    /* read only when the edit names an emitter */
    const float* vertices;          /* [numPrims * 9] before the edit */
    int numLights, numLightPrims;   /* sampler entries; light primitives (one less when the environment map has the last entry) */
    const int* lightPrimIds;        /* [numLightPrims] */
    const float* lightRadiance;     /* [numLightPrims * 3] */
    const float* lightArea;         /* [numLightPrims] Math::triangleArea before the edit */
    float envPower;                 /* the environment map's sampler entry */
    int emissiveTree, numEmissive;  /* the scene has a tree of its emissive triangles; how many they are */
    const int* emiLeafPrims;        /* [numEmissive] */
} rs_geometry_edit_view;
typedef struct rs_geometry_edit_plan {
    int m;                          /* distinct primitives named: the records staged (a repeated id keeps its last record and its first place) */
    int lamps;                      /* the edit names an emitter */
    size_t offV, offN, bytes;       /* ids | vertices | normals, each part 16-byte aligned; without normals bytes == offN */
    size_t staged, onDevice;        /* copied from the host / held in the device buffer when the records themselves are staged */
    size_t partStaged, partOnDevice;   /* ... when numPartRecs 112-byte part records are staged and follow the records a kernel expands them to */
} rs_geometry_edit_plan;
typedef struct rs_geometry_edit_lights {
    float sumAll;                   /* the new light sampler's total power */
    int emiGrid;                    /* a grid could be laid over the emissive root box (0: no emissive tree, or no extent) */
    float emiLo[3], emiHi[3];       /* the emissive root box after the edit (emissiveTree only) */
    float emiBase[3], emiScale[3];
    double emiMargin;
} rs_geometry_edit_lights;
/* Test hook: evaluates those functions for an edit of `count` records made through the entry point `name` (emitters: it takes Light
 * triangles); needs no device.  Returns the refusal the entry point would return, with its text.  slots (may be NULL): [count] the place
 * of every input record among the m staged.  When the plan says lamps and lights is not NULL: *lights, and area [numLightPrims], prob and
 * failId [numLights] (each may be NULL). */
int  rs_debug_plan_geometry_edit(const rs_geometry_edit_view* view, const char* name, int emitters, int count, const int* primIds,
                                 const float* vertices, const float* normals, int numPartRecs, rs_geometry_edit_plan* plan, int* slots,
                                 rs_geometry_edit_lights* lights, float* area, float* prob, int* failId);
/* Partial refit: an edit that names few triangles recomputes, in every tree, only the boxes on the paths from those triangles' leaves to
 * the roots, and leaves every device table bit for bit what the whole-scene refit leaves.  (The reference has no moving geometry: there is
 * no reference line to cite.)  on = 0 is the default: every edit refits the whole scene, through exactly the launches it made before this
 * switch existed, and nothing more is allocated.  on = 1: an accepted edit of any of the three kinds (rs_scene_set_triangles,
 * rs_scene_set_geometry, rs_scene_set_part_transforms) is partial when it names at most maxTriangles distinct triangles, when the bound
 * on the nodes it can dirty -- that number times the sum over the scene's trees of (depth + 1) -- is at most what the path's work words
 * can name (2^32 - 2), and when a whole refit of this scene has run before; otherwise it refits the whole scene.  The first edit of a
 * scene is therefore always whole: it builds the tables and replaces caller-supplied inexact boxes.  maxTriangles < 0 selects the
 * library's default, 4096: the largest m of the sweep 1, 16, 256, 4096, 1 % of the triangles at which the partial refit's stream time
 * was at most 0.8 x the whole refit's on both benchmark scenes.  Stream time of one edit, partial / whole refit of the commit before
 * the switch (DESIGN.md section 3 has the full table and the frame periods):
 *       m        262 144 triangles (Sponza-class)     2 830 336 triangles (Bistro-class)
 *       1        0.298 / 6.10 ms   0.05 x             0.340 / 74.5 ms   0.005 x
 *       16       0.524 / 6.04      0.09               0.544 / 74.4      0.007
 *       256      0.778 / 6.09      0.13               0.910 / 74.6      0.012
 *       4 096    1.828 / 6.19      0.30               2.725 / 74.7      0.037
 *       1 %      1.212 / 6.16      0.20  (2 611)      50.90 / 76.1      0.67  (28 200: host-bound, and a different m per scene)
 * Everything else about the three
 * entry points is unchanged: arguments, refusals, staging ring, fences, "a repeated id takes its last record", count == 0,
 * rs_scene_host_desc afterwards, RS_ERR_UNSUPPORTED during capture, invalidation of retained planes, dirty boxes for shadow
 * revalidation, RS_TABLE_LIGHT_MOVED and the previous pose of a tracked scene.  An edit that names an emitter still re-quantises every
 * record of the emissive tree, whose grid moves with the lamps.  The switch itself is host only, waits for nothing and may be flipped
 * between any two edits; the first edit made with it on builds the path's tables (12 bytes per tree node, 24 per reference node, 4 per
 * triangle and grid-box tree: INTEGRATION.md section 3c) and waits for the device once, as the first edit of a scene does.
 * rs_scene_get_partial_refit returns the switch and the threshold in force (the default's value, not -1); either pointer may be NULL.
 * rs_scene_refit_counts: how many accepted edits of this scene refitted the whole scene and how many were partial (host only; either
 * pointer may be NULL).  Refused with RS_ERR_INVALID_ARGUMENT: a null scene, on other than 0 / 1, maxTriangles == 0. */
int  rs_scene_set_partial_refit(rs_scene* scene, int on, int maxTriangles);
int  rs_scene_get_partial_refit(const rs_scene* scene, int* on, int* maxTriangles);
int  rs_scene_refit_counts(const rs_scene* scene, unsigned long long* whole, unsigned long long* partial);
/* Test hooks.  rs_debug_scene_refit_dirty waits as rs_synchronize does and returns how many distinct nodes the most recent accepted edit
 * recomputed on the partial path, 0 when that edit refitted the whole scene or there was none: nodes of the reference tree, records of
 * the shadow tree and of the six ordered trees; the emissive tree's are not counted.  RS_ERR_UNSUPPORTED while the library stream is being
 * captured.  rs_debug_plan_refit is the decision itself (restir_amd/csrc/rs_geometry_plan.h rs_plan_refit), device-free: m distinct
 * triangles, treeDepth[numTrees] the deepest leaf of each tree with the root at 0; *bound = m x sum (treeDepth + 1), *partial = 1 iff on,
 * keysValid, m <= maxTriangles (< 0: the default) and bound <= capacity.  numNodes does not enter the decision. */
int  rs_debug_scene_refit_dirty(const rs_scene* scene, unsigned long long* nodes);
int  rs_debug_plan_refit(int on, int maxTriangles, int keysValid, int m, int numTrees, const int* treeDepth,
                         unsigned long long numNodes, unsigned long long capacity, int* partial, unsigned long long* bound);
/* Motion tracking: the previous pose of the scene, for the G-buffer's motion plane.  (The reference has no moving geometry: there is no
 * reference line to cite.  Its renderGBuffer, src/gbuffer.cu:49-54, asks where the hit's world point was on last frame's screen.)
 * A tracked scene keeps a second vertex array on the device, 36 bytes per triangle: the vertices as they stood at the last
 * rs_scene_advance_motion.  GBuffer::render then writes, for a hit with barycentrics (bx, by) on primitive p,
 *     prevPos = pv1 * bx + pv2 * by + pv0 * (1 - bx - by)          (pv*: p's previous vertices; the expression that gives the hit position)
 *     motion  = lastCamera.getRasterCoord(prevPos), -1 when outside the image
 * instead of lastCamera.getRasterCoord(hit position); a miss writes 0 as before, and every other plane is unchanged.  A triangle that has
 * not moved since the last advance gets the untracked value, bit for bit.  Consumers (ReSTIR's temporal pass, ReSTIR-GI, SVGF) read the
 * plane as before.
 * rs_scene_set_motion_tracking(scene, 1) allocates the array and fills it with the current vertices; (scene, 0) makes later launches
 * camera-only again (the memory stays until rs_scene_destroy).  A scene that never switches it on allocates nothing and launches the
 * kernels it always launched.  A failed allocation leaves the scene untracked and unchanged.
 * rs_scene_advance_motion: the geometry as it stands at this point of the library stream becomes the previous pose for every launch
 * enqueued after the call.  Call it once per frame, next to rs_gbuffer_update.  rs_scene_set_triangles / rs_scene_set_geometry never
 * write the previous pose: after any number of edits it is still the pose at the last advance.  On an untracked scene the call succeeds
 * and does nothing; with no accepted geometry edit since the last advance it enqueues nothing and retained G-buffer planes stay valid;
 * otherwise it copies the vertex array on the device (DESIGN.md section 3 has the cost) and invalidates retained planes.
 * Ordering of both calls as rs_scene_set_triangles: no device synchronisation; a render that has only been recorded is launched first,
 * with the old previous pose; the copy runs on the library stream behind what the internal streams have been handed so far, and their
 * next launches wait for it.  RS_ERR_INVALID_ARGUMENT: a null scene.  RS_ERR_UNSUPPORTED while the library stream is being captured into
 * a graph (a captured frame keeps the pose it was captured with).  INTEGRATION.md section 3e has the frame loop and what stays as it is. */
int  rs_scene_set_motion_tracking(rs_scene* scene, int on);
int  rs_scene_advance_motion(rs_scene* scene);
/* Test hook: waits as rs_synchronize does, then copies the previous pose (9 floats per primitive) to `out`.  RS_ERR_INVALID_ARGUMENT: a
 * null argument, or a scene that does not track motion.  RS_ERR_UNSUPPORTED while the library stream is being captured. */
int  rs_scene_download_prev_vertices(const rs_scene* scene, float* out);
/* The boxes of the reference tree refitted to `vertices` (9 floats per primitive), host only, no GPU call: order0 is bvhNodes[0] (3 ints
 * per node: primitive or -1, boundingBoxId, miss link), from which the children are derived; boundingBoxes receives 6 floats per node
 * by boundingBoxId.  Min and max are taken with -0 below +0, so the bits do not depend on the order of evaluation.  On the vertices a
 * tree was built from this returns the boxes rs_build_bvh returned.  RS_ERR_INVALID_ARGUMENT: a null array, bvhSize other than
 * 2 * numPrims - 1, a vertex that is not finite, a primitive id or link out of range, an order that is not a tree. */
int  rs_refit_boxes(int numPrims, const float* vertices, int bvhSize, const int* order0, float* boundingBoxes);
/* Test hooks of rs_scene_set_triangles (tests/refit_tables.py holds every record of the refit's device tables to a host restatement).
 * rs_debug_scene_table waits for the library stream and the library's internal streams, as rs_synchronize does, then copies one device
 * array of the scene to `host`.  *bytes receives the array's size (0: the scene has no such array); host == NULL asks for the size
 * only.  RS_ERR_INVALID_ARGUMENT, nothing written: a null scene or `bytes`, an unknown `which`, a capacity below the size.
 * RS_ERR_UNSUPPORTED while the library stream is being captured. */
#define RS_TABLE_VERTICES  0   /* float[9 * numPrims] */
#define RS_TABLE_NORMALS   1   /* float[9 * numPrims] */
#define RS_TABLE_TRIS      2   /* 48-byte triangle records { v0, pad0, e1, pad1, e2, pad2 } [numPrims] */
#define RS_TABLE_NODES_ALL 3   /* 32-byte records { min.xyz, max.z, max.x, max.y, primId, next } [6 * bvhSize + 1] */
#define RS_TABLE_OCC_NODES 4   /* 16-byte grid-box records [occCount + 1], the end record last */
#define RS_TABLE_OCC_CHAIN 5   /* 32-byte records [bvhSize] by original node id */
#define RS_TABLE_OCC_TRIS  6   /* triangle records [numPrims] in the shadow tree's leaf order */
#define RS_TABLE_ORD_NODES 7   /* the whole allocation: 6 * ordStride bytes */
#define RS_TABLE_ORD_TRIS  8   /* triangle records [3 * numPrims] */
#define RS_TABLE_EMI_NODES 9   /* 16-byte grid-box records of the emissive tree and its end record */
#define RS_TABLE_EMI_TRIS  10  /* triangle records, one per emissive triangle */
/* (tables of the scene's edit history, which a scene built afresh from the edited arrays does not share, are numbered from 32) */
#define RS_TABLE_LIGHT_MOVED 32 /* uint32 per light-sampler entry: rs_scene_light_moves at the last edit that named the light's primitive, 0 = never; size 0 before the first edit that names an emitter */
int  rs_debug_scene_table(const rs_scene* scene, int which, void* host, size_t capacity, size_t* bytes);
/* The 16-bit grid of the scene's grid-box trees: plane q of axis k lies at base[k] + q * scale[k]; the margin boxes are cleared by; the
 * box the grid was laid over (a moved vertex must stay inside it); the shadow tree's record count and the byte stride of the ordered
 * trees (0: the scene has no such tree; without the shadow tree everything is 0).  Any pointer may be NULL.  Host only. */
int  rs_debug_scene_grid(const rs_scene* scene, float base[3], float scale[3], double* margin, float lo[3], float hi[3], int* occCount, int* ordStride);
/* The grid of the emissive tree (RS_TABLE_EMI_NODES), which rs_scene_set_geometry lays anew when emitters move: base, scale and margin
 * as above; *state = 1 while the tree answers the last bounce, 0 while it is off; *count = its records without the end record (0, with
 * base, scale and margin 0: the scene has no such tree).  Any pointer may be NULL.  Host only. */
int  rs_debug_scene_emissive_grid(const rs_scene* scene, float base[3], float scale[3], double* margin, int* state, int* count);
/* The function that turns one exact box into the three box dwords of a grid-box record (rs_grid.h grid_box), as it is.  Host only.
 * *fits = 0, out untouched: the box does not fit the grid's 16 bits. */
int  rs_debug_grid_box(const float lo[3], const float hi[3], const float base[3], const float scale[3], double margin, unsigned out[3], int* fits);
/* The texels of texture texId of the scene's table: width x height must be the texture's own, data is host memory of 3 floats per
 * texel and is copied.  Ordering and refusals as rs_scene_set_materials (texId out of range, other dimensions and null data are
 * RS_ERR_INVALID_ARGUMENT).  Memory: a texture that is never edited keeps its one device array.  An edited texture holds at most three
 * device arrays of its size (the original among them; the second and third are allocated by the first edits that find every existing
 * one still referenced by a version in flight) and one pinned host array per device array it has filled; with all three referenced by
 * frames in flight the host waits for the oldest.  A 1024 x 1024 map so costs at most 24 MiB of device and 36 MiB of pinned host
 * memory beyond the unedited scene.  The environment sampler's alias table (8 bytes per texel) is kept the same way.
 * If texId is the environment map the host rebuilds what rs_scene_build_textured builds from it -- rs_build_envmap_pdf, the map's
 * alias table, its entry in the light sampler (the pdf's sum), then the light alias table and sumLightPower, which changes every light
 * record -- and all of it reaches the device with the same version switch; rs_scene_host_desc then returns texels, envMapProb,
 * envMapFailId, lightProb, lightFailId and sumLightPower equal, bit for bit, to those of a scene built afresh, and a later
 * rs_scene_set_emission uses the new environment power.  An environment map whose pdf sum, or the resulting total light power, is not
 * finite and positive is refused with RS_ERR_INVALID_ARGUMENT, the scene unchanged.  (Creation is laxer: rs_scene_build_textured and
 * rs_scene_create take a black environment map and one with an infinite or NaN texel as the reference does -- a black map's entry has power 0
 * and yields no live sample; with an infinite or NaN texel the total light power is infinite or NaN, every pdf of every light 0 or NaN
 * and no reservoir live; the map is still shown where a ray misses -- and such a scene
 * renders bit for bit like the oracle's; the same map handed to this call is refused and the scene keeps the map it had:
 * tests/test_gpu_texture_extremes.py.)  The environment entry stays outside light
 * tracking (rs_restir_set_light_tracking), as before. */
int  rs_scene_set_texture(rs_scene* scene, int texId, int width, int height, const float* data);
/* Scene::clear / DevScene::destroy (src/scene.cpp:217-220,511-532). */
int  rs_scene_destroy(rs_scene* scene);

/* Camera::update (src/sceneStructs.h:88-102): view/right/up/rotationMatInv from rotation. */
int  rs_camera_update(rs_camera* cam);

/* ---- scene files (host only; no GPU call) ------------------------------------------------------
 * Scene::Scene(filename) (src/scene.cpp:96-131) with loadMaterial (:371-433), loadModel (:222-283), loadCamera
 * (:285-354), Resource::loadOBJMesh (:27-61) and the instance baking of buildDevData (:161-176): parses the
 * reference's text scene format and returns the flat arrays rs_scene_build_textured takes.  Image files named in
 * the scene must be PNG, JPEG (Huffman-coded, 8 bit), TGA, BMP, binary PPM (P6, 8 bit) or Radiance HDR (.hdr, RGBE) -- the other stb_image
 * formats stay with the caller, who can build the arrays directly; glTF meshes are not read.  Pointers in the view stay valid until
 * rs_scene_file_free. */
typedef struct rs_scene_file rs_scene_file;
typedef struct rs_scene_file_view {
    int                numPrims;
    const float*       vertices;      /* 9 floats / triangle, transformed (scene.cpp:167) */
    const float*       normals;       /* 9 floats / triangle, normalize(normalMat * n) (:168) */
    const float*       texcoords;     /* 6 floats / triangle */
    const int*         materialIds;   /* 1 / triangle */
    int                numMaterials;
    const rs_material* materials;
    int                numTextures;
    const rs_texture*  textures;
    int                envMapTexId;   /* -1: none */
    rs_camera          camera;        /* after Camera::update */
    int                iterations;    /* "Sample" */
    int                traceDepth;    /* "Depth" (Settings::traceDepth) */
    const char*        imageName;     /* "File" */
    int                numSkippedObjects;   /* objects whose mesh file could not be opened ("[Fail to load, skipped]", scene.cpp:234-240) */
} rs_scene_file_view;
int  rs_scene_file_load(const char* path, rs_scene_file** file);
int  rs_scene_file_get(const rs_scene_file* file, rs_scene_file_view* view);
int  rs_scene_file_free(rs_scene_file* file);
/* The "Object" blocks of the loaded file, in file order (skipped objects are not among them): firstPrim has *numObjects + 1 entries and
 * tiles [0, numPrims) of the view; transforms16 holds each object's load-time matrix (16 floats, column-major); meshVertices[i] /
 * meshNormals[i] point to object i's object-space, de-indexed mesh, 9 floats per triangle (objects that name one mesh file share it).
 * This is what turns objects into the parts of rs_scene_define_parts: primIds is a range, the rest pose is the mesh, and
 * rs_build_transformation_matrix of a new translation / rotation / scale re-poses the object with the bits the loader would have
 * produced.  Pointers stay valid until rs_scene_file_free.  RS_ERR_INVALID_ARGUMENT: a null argument. */
int  rs_scene_file_objects(const rs_scene_file* file, int* numObjects, const int** firstPrim, const float** transforms16,
                           const float* const** meshVertices, const float* const** meshNormals);
/* Math::buildTransformationMatrix (src/mathUtil.cpp:13-20): column-major 4x4, rotation in degrees. */
int  rs_build_transformation_matrix(const float* translation, const float* rotation, const float* scale, float* out16);
/* scene.cpp:167-168 for one instance: vec3(transform * vec4(v, 1)) and normalize(transpose(mat3(inverse(transform))) * n). */
int  rs_bake_instance(const float* translation, const float* rotation, const float* scale, int n,
                      const float* vertsIn, const float* normalsIn, float* vertsOut, float* normalsOut);
/* The same for a caller-supplied column-major 4x4 (n corners, 3 floats each): rs_bake_instance(t, r, s, ...) and rs_bake_matrix of
 * rs_build_transformation_matrix(t, r, s) return the same bits, and so does the kernel behind rs_scene_set_part_transforms.  Values
 * are not checked: a singular matrix yields non-finite normals.  RS_ERR_INVALID_ARGUMENT: a null matrix, n < 0, a null array with n > 0. */
int  rs_bake_matrix(const float* matrix16, int n, const float* vertsIn, const float* normalsIn, float* vertsOut, float* normalsOut);

/* ---- scene services, batched (for parity tests of DevScene::intersect / testOcclusion) */
/* DevScene::intersect (src/scene.h:245-284): n rays of 6 floats (origin, direction), device ptrs.
 * Outputs (device): primId[n], matId[n], pos[3n], norm[3n]. */
int  rs_trace_closest(const rs_scene* scene, int n, const float* devRays,
                      int* devPrimId, int* devMatId, float* devPos, float* devNorm);
/* The same query through the wave-level service the multi-bounce kernels use for their bounce rays (general-case rays walk the
 * closest-hit tree of their threaded order, occlusion_bvh.cpp; same outputs, same bits). */
int  rs_trace_closest_wave(const rs_scene* scene, int n, const float* devRays,
                           int* devPrimId, int* devMatId, float* devPos, float* devNorm);
/* on = 0: bounce rays walk the reference's own tree (src/scene.h:245-284 literally); 1: the closest-hit trees again (the default
 * when the scene's tables allow them).  *was (may be NULL) receives the previous setting.  Results are identical either way. */
int  rs_scene_set_ordered_tree(rs_scene* scene, int on, int* was);
/* Host only (no device call): builds the closest-hit trees of the bounce rays from a reference table (rs_build_bvh's outputs) and
 * verifies what their walk relies on: the leaves list the triangles in the order the threaded orders of src/bvh.cpp:156-193 meet
 * them, boxes contain what is below them, miss links nest.  nodeCounts[3] / maxDepth[3] (may be NULL): per axis. */
int  rs_ordered_bvh_host_check(int numPrims, int bvhSize, const float* boundingBoxes, const int* const bvhNodes[6],
                               int* nodeCounts, int* maxDepth);
/* DevScene::testOcclusion (src/scene.h:286-316): n segments of 6 floats (x, y). */
int  rs_trace_occlusion(const rs_scene* scene, int n, const float* devSegments, int* devOccluded);

/* ---- GBuffer (src/gbuffer.h:24-27; create/destroy are defined in src/denoiser.cu:373-403) */
int  rs_gbuffer_create(int width, int height, rs_gbuffer** g);
int  rs_gbuffer_destroy(rs_gbuffer* g);
/* GBuffer::render (src/gbuffer.cu:80-86) */
int  rs_gbuffer_render(rs_gbuffer* g, const rs_scene* scene, const rs_camera* cam);
/* row-strip variant for framebuffer tiling: only rows [y0,y1) are rendered */
int  rs_gbuffer_render_rows(rs_gbuffer* g, const rs_scene* scene, const rs_camera* cam, int y0, int y1);
/* GBuffer::update (src/gbuffer.cu:75-78): lastCamera = cam; frameIdx ^= 1 */
int  rs_gbuffer_update(rs_gbuffer* g, const rs_camera* cam);
int  rs_gbuffer_get_view(const rs_gbuffer* g, rs_gbuffer_view* view);
/* GBuffer::render (src/gbuffer.cu:80-86) reads the scene, the camera, lastCamera and the row range and nothing else.  A frame's
 * first render request that equals those of the two previous frames in all of them (same scene and no rs_scene_set_emission since,
 * every byte of both cameras, same rows) launches nothing: the G-buffer hands out the planes it already holds, which are the bits a
 * render would have written.  That is the reference's default (a camera that stands still).  Anything else renders: a second
 * render within a frame, a frame that had none, rs_gbuffer_rows_unpack into the rendered rows, rs_set_denoise_stream(1), a stream
 * that is being captured.  The planes of rs_gbuffer_get_view are therefore read-only for the caller, unless it calls
 * rs_gbuffer_invalidate afterwards (or renders again).  on = 1 is the default; the environment variable RS_GBUFFER_REUSE=0 makes 0
 * the default (A/B measurements). */
int  rs_gbuffer_set_reuse(rs_gbuffer* g, int on);
/* GBuffer::render (src/gbuffer.cu:80-86) requests so far that launched the walk / that were answered from retained planes */
int  rs_gbuffer_reuse_stats(const rs_gbuffer* g, unsigned long long* rendered, unsigned long long* reused);
/* for a caller that wrote planes through the pointers of the view: the next GBuffer::render requests (src/gbuffer.cu:80-86) walk again */
int  rs_gbuffer_invalidate(rs_gbuffer* g);
/* Rows [y0,y0+rows) of the id / normal / depth planes as one packed device buffer (20 B/px); sel 0 =
 * planes of the current frame index, 1 = the "last" planes.  Used by the multi-GPU tiling to share
 * G-buffer history when the camera moves (findTemporalNeighbor reads lastPrimId/lastNormal/lastDepth
 * at a reprojected pixel that may belong to another strip). */
size_t rs_gbuffer_rows_bytes(const rs_gbuffer* g, int rows);
int  rs_gbuffer_rows_pack(const rs_gbuffer* g, int sel, int y0, int rows, void* devBuffer);
int  rs_gbuffer_rows_unpack(rs_gbuffer* g, int sel, int y0, int rows, const void* devBuffer);

/* ---- ReSTIR (src/restir.h:128-133) ------------------------------------------------------ */
/* ReSTIRInit (src/restir.cu:478-504): reservoir buffers for width*height pixels, zero-filled. */
int  rs_restir_init(int width, int height, rs_restir** r);
/* ReSTIRFree (src/restir.cu:506-514) */
int  rs_restir_free(rs_restir* r);
/* ReSTIRReset (src/restir.cu:516-518): re-arms the first-frame flag */
int  rs_restir_reset(rs_restir* r);
/* ReSTIRDirect (src/restir.cu:418-446).  looper = State::looper (the caller increments it, as the
 * reference launcher does at :441-445); reuse = Settings::reservoirReuse (bit0 temporal, bit1 spatial).
 * Semantics: the two-phase contract (phase A for every pixel, then phase B), DESIGN.md "Q1". */
int  rs_restir_direct(rs_restir* r, const rs_scene* scene, const rs_camera* cam, const rs_gbuffer* g,
                      float* devDirectIllum, int iter, int looper, int reuse);
/* Row-strip variants for framebuffer tiling across GPUs: phase A (primary hit, RIS, shadow ray,
 * temporal merge, publish) and phase B (spatial reuse, shade, accumulate) on rows [y0,y1).
 * Between them the caller exchanges `halo` rows of published reservoirs with its neighbours
 * (rs_restir_halo_pack / _unpack).  rs_restir_end_frame swaps the ping-pong buffers and clears the
 * first-frame flag (src/restir.cu:434-438). */
int  rs_restir_phase_a(rs_restir* r, const rs_scene* scene, const rs_camera* cam, const rs_gbuffer* g,
                       int looper, int reuse, int y0, int y1);
int  rs_restir_phase_b(rs_restir* r, const rs_scene* scene, const rs_camera* cam, const rs_gbuffer* g,
                       float* devDirectIllum, int iter, int reuse, int y0, int y1);
int  rs_restir_end_frame(rs_restir* r);
/* What the measurement of rs_set_side_stream's mode 4 decided for this object and its current scene: 0 GBuffer::render and the
 * primary rays as two launches, 1 as one, -1 still measuring (decided once 14 frames with such a launch have been enqueued; a
 * caller that times frames runs those first), -2 nothing was measured (synchronous launches; a forced mode; launches below three
 * rounds of the chip's wave slots, which are always one launch -- rs_restir_last_launch tells what a frame actually ran). */
int  rs_restir_launch_choice(const rs_restir* r, int* choice);
/* What the last rs_restir_phase_a / rs_restir_direct call launched, measured or not: *fused = 1 GBuffer::render in the primary rays'
 * launch, 0 its own launch (-1 before the first call); *chains = how many internal streams the frames' chains take in turn (0 in
 * synchronous mode).  A launch below three rounds of wave slots (a strip) is fused and on three chains without a measurement. */
int  rs_restir_last_launch(const rs_restir* r, int* fused, int* chains);
/* What a phase-A call decides before it launches anything, as a function of plain integers (restir_amd/csrc/rs_frame_plan.h; the
 * rules and the measurements behind them are written there, DESIGN.md section 4 lists them).  Flags are 0 / 1. */
typedef struct rs_phase_a_inputs {
    int async;              /* launches of this call are asynchronous (overlapped mode, no per-pass timing) */
    int chainStreams, smallChains, shadowOnMain;   /* rs_set_stream_plan, resolved: 1 / 2, 0 / 1, 0 / 1 / 2 */
    int fuseMode;           /* 0 never, 1 always (large launches), 2 always, 3 measured (rs_set_side_stream's 1 .. 4) */
    int denoiseStream;      /* rs_set_denoise_stream(1) */
    int chainsInFlight;     /* 3, less one per other stream of the context with work in flight */
    int reusedThree;        /* a frame answered from retained G-buffer planes takes one of three chains (0: RS_REUSE_CHAINS=2) */
    int phaseACalls;        /* phase-A calls of this frame before this one */
    int width, y0, y1;      /* rows clamped to the image */
    int deferredValid, deferredMatches, deferredY0, deferredY1;   /* the deferred GBuffer::render: there is one; same scene and camera; its rows */
    int reusedFrame;        /* this frame's render request was answered from retained planes */
    int tuneChoice, tuneFrame;   /* the measurement for this scene: -1 measuring / 0 two launches / 1 one; frames counted so far */
    int chain, smallChain;  /* the frame's turn among two / three chains */
    int idle;               /* the previous frames had finished when this frame began (twice in a row) */
    int numLights, envMap, risGlobalBelow;   /* light table entries; the scene has an environment map; rs_set_ris_table_pixels */
    int cutState;           /* primary cuts (rs_restir_set_primary_cuts): 0 off, or this call's key differs from the previous frame's; 1 the key is
                               unchanged and no cut has been built for it; 2 unchanged and built */
} rs_phase_a_inputs;
#define RS_RIS_GLOBAL    0  /* light table read from global memory */
#define RS_RIS_LDS       1  /* whole table in LDS */
#define RS_RIS_ALIAS_LDS 2  /* alias records in LDS */
typedef struct rs_phase_a_plan {
    int fuse;               /* GBuffer::render rides in the primary rays' launch (rs_restir_last_launch's *fused) */
    int tuneCounted;        /* this launch is one the fused / separate measurement applies to */
    int tuneRestart;        /* a measurement under way starts again */
    int stream;             /* -1 the library stream, else the internal stream 0 .. 2 of the chain primary rays -> RIS -> shadow rays */
    int lastChains;         /* rs_restir_last_launch's *chains */
    int splitSlot, splitCall, splitMode;   /* tile-split hints: per stream (0 library, 1 + stream), per call of the frame (at most 2); mode 1 alone / 0 large / 2 small */
    int shadowOnLibrary;    /* the shadow rays go to the library stream, not to the chain's */
    int risForm;            /* RS_RIS_* */
    int tilesX, tilesY, fusedTilesY;   /* blocks of 32 x 8 pixels over the rows; of 32 x 4 over the deferred render's rows when fused */
    int cut;                /* primary cuts: 0 the primary rays walk the tree; 1 they walk the tree and the build is enqueued behind the chain;
                               2 they walk the cuts */
} rs_phase_a_plan;
/* Test hook: evaluates that function; needs no device. */
int  rs_debug_phase_a_plan(const rs_phase_a_inputs* in, rs_phase_a_plan* out);
/* Primary cuts.  While the scene's geometry, the camera, the size and the rows of a phase-A call stay what they were in the previous
 * frame, the primary rays (not those of the launch fused with GBuffer::render) walk a per-32x8-pixel-block cut of the BVH instead of
 * the tree: a re-linked copy of the node records that some ray of the block can pass at all (restir_amd/csrc/rs_cuts.h).  Every ray
 * enters the nodes it would enter in the tree, in the same order: no result changes by a bit.  The second frame with an unchanged key
 * enqueues the build behind its own kernels (no host wait), the frames after it use the cuts; a camera move, rs_scene_set_triangles,
 * rs_scene_set_geometry and rs_scene_set_part_transforms forget them, material, texture and emission edits do not.  Memory: the first
 * build allocates, per phase-A call of a frame, 512 records of 36 bytes per block of its rows (149 MB for 1920x1080, 597 MB for
 * 3840x2160), kept until rs_restir_free; where that allocation fails the frames keep the tree and no call fails.  on = 1 is the default; the environment variable RS_PRIMARY_CUTS=0
 * makes 0 the default (A/B measurements). */
int  rs_restir_set_primary_cuts(rs_restir* r, int on);
/* Test hooks.  The most records one block's cut may have (default 4096; a block past it walks the tree);
 * what the last phase-A call's cuts hold -- blocks of its launch, blocks without a cut, records in all cuts (zeros while none is built),
 * whether that call's primary rays walked them, builds so far (waits for a build in flight);
 * and containment: each of the n rays { pixel x, pixel y, jitter x, jitter y } walks the whole tree on the geometric part of the
 * reference's box test, out = { nodes passed that block `cell`'s cut lacks, nodes passed, rays left out (a special case of
 * AABB::intersect, another traversal order than the cut's, a block without a cut), records in the block's cut }. */
int  rs_debug_set_primary_cut_cap(rs_restir* r, int records);
int  rs_debug_primary_cut_info(rs_restir* r, int* cells, int* cellsWithoutCut, unsigned long long* records, int* usedLastFrame, unsigned long long* builds);
int  rs_debug_primary_cut_missing(rs_restir* r, const rs_scene* scene, int cell, int n, const float* rays, unsigned long long out[4]);
/* Primary leaf lists, on top of the cuts: every 8x8 tile of such a launch also gets the LEAVES of the cut of its own 8x8 pixels, box and
 * triangle side by side in 64-byte records in the traversal order, and a wave whose tile has a list tests those records one after the
 * other instead of walking its block's cut (a tile without a list -- no common traversal order, an empty list or one past the cap, a
 * full arena, a scene without nested reference boxes -- keeps the cut, as do the quarter-tile waves of a split tile).  A triangle that
 * would become the closest hit while its leaf box is only grazed is confirmed by the reference's own box test up its ancestors: no
 * result changes by a bit.  Same key, build and lifetime as the cuts, and off whenever they are off.  Memory: per phase-A call 32
 * records of 68 bytes per tile (71 MB for 1920x1080); where that allocation fails the frames keep the cuts.  on = 1 is the default;
 * RS_PRIMARY_LEAF_LISTS=0 makes 0 the default (A/B measurements). */
int  rs_restir_set_primary_leaf_lists(rs_restir* r, int on);
/* Test hooks, as the cuts': the most records one tile's list may have (default 192; 0: no tile takes a list); tiles of the last phase-A
 * call's launch, tiles without a list, records in all lists, whether that call walked lists, list builds so far; containment of every
 * ray's own tile's list, out = { leaves passed that the list lacks, leaves passed, rays left out, 0 }; and, on the host alone, the list
 * the builder makes for the tile at pixel (x0, y0) over rs_build_bvh's outputs: *order (-1: the tile takes none), *count (cap + 1: more
 * than cap), positions[min(*count, cap)] = the leaves' record indices in that order's table. */
int  rs_debug_set_primary_leaf_list_cap(rs_restir* r, int records);
int  rs_debug_primary_leaf_list_info(rs_restir* r, int* tiles, int* tilesWithoutList, unsigned long long* records, int* usedLastFrame, unsigned long long* builds);
int  rs_debug_primary_leaf_list_missing(rs_restir* r, const rs_scene* scene, int n, const float* rays, unsigned long long out[4]);
int  rs_debug_plan_primary_leaf_list(const rs_camera* cam, int x0, int y0, int bvhSize, const float* boundingBoxes, const int* const bvhNodes[6], int cap,
                                     int* order, int* count, int* positions);
/* The same for the node cut of the w x h pixels at (x0, y0) (a block is 32 x 8): *order, *count (cap + 1: more than cap),
 * positions[min(*count, cap)] = the kept records' indices in that order's table and, when *count <= cap, links[*count] = their miss links
 * within the cut (*count: the cut's end).  The walk and the re-linking are the functions the device builder runs. */
int  rs_debug_plan_primary_cut(const rs_camera* cam, int x0, int y0, int w, int h, int bvhSize, const float* boundingBoxes, const int* const bvhNodes[6], int cap,
                               int* order, int* count, int* positions, int* links);
/* Shadow rays regrouped by length: in a scene with the shadow tree, a block of the shadow-ray kernel (32x8 pixels, four waves) hands its
 * segments out to its waves by length before the walk -- 64 bins over the diagonal of the scene's root box, the longest bin first -- so
 * that a wave's rays end together instead of waiting for the tile's longest (restir_amd/csrc/rs_shadow_regroup.h).  Occlusion does not
 * depend on the lane that carries a ray: no result changes by a bit.  Full frames and strips.  on = 1 is the default;
 * RS_SHADOW_REGROUP=0 makes 0 the default (A/B measurements). */
int  rs_restir_set_shadow_regroup(rs_restir* r, int on);
/* Test hooks.  Host only: bins[i] = shadow_bin(lengths[i], binsOverExtent) for n segments and, where first and count are given
 * (n <= 256, the lanes of one block; active[i] == 0: the lane has no segment, active == NULL: all have), the block's slot plan:
 * first[64] = the first slot of every bin, *count = the active rays, which take slots 0 .. *count - 1, longest bin first.  rootLo /
 * rootHi non-null: binsOverExtent is computed from that root box as the launch does; *binsOverExtentOut (may be null) is the value used.
 * On the device: the shadow-ray pass of a phase-A call alone, in the form the switch chooses (a scene without the shadow tree: the plain
 * form), over the caller's planes of width * height pixels each -- posTag { position, bits(matId | kind << 24) }, candLi { Li, dist },
 * candWi { wi, weight }, in and out: an occluded segment's weight comes back 0 -- on rows [y0, y1); slots (may be null): the slot every
 * pixel's ray took in its 32x8 block, -1 where a pixel has no segment and everywhere under the plain form; *binsOverExtent (may be
 * null): shadow_bin's scale for this scene, 0 without the shadow tree. */
int  rs_debug_plan_shadow_regroup(int n, const float* lengths, const unsigned char* active, float binsOverExtent, const float* rootLo, const float* rootHi,
                                  int* bins, int* first, int* count, float* binsOverExtentOut);
int  rs_debug_shadow_pass(rs_restir* r, const rs_scene* scene, int y0, int y1, const float* posTag, const float* candLi, float* candWi, int* slots,
                          float* binsOverExtent);
/* What one phase-A call of a frame keeps about its cuts between frames, as plain data (restir_amd/csrc/rs_cut_plan.h).  The key is what
 * the cuts and lists were built from; listCap is 0 while the lists' switch is off.  `cuts` and `lists` say what became of each arena
 * under that key. */
typedef struct rs_primary_cut_key {
    unsigned long long sceneId, geomEdits;
    rs_camera cam;
    int y0, y1;
    unsigned cap, listCap;
} rs_primary_cut_key;
#define RS_CUT_ARENA_NOTHING   0   /* nothing built for the key */
#define RS_CUT_ARENA_NO_MEMORY 1   /* the arena could not be allocated: the key goes without */
#define RS_CUT_ARENA_BUILT     2
typedef struct rs_primary_cut_slot { int keyValid, cuts, lists; rs_primary_cut_key key; } rs_primary_cut_slot;
typedef struct rs_primary_cut_sizes { int numCells; unsigned capacity; int numTiles; unsigned listCapacity; } rs_primary_cut_sizes;
/* Test hook, host only: a call with key *key, the cuts' switch `on` and the library stream `capturing` or not meets *slot -- *cutState as
 * rs_phase_a_inputs has it, *slot as the call leaves it -- and the arenas of a launch of tilesX x tilesY blocks under the key's caps:
 * cells, records, tiles (0: no lists), list records. */
int  rs_debug_plan_primary_cut_slot(int on, int capturing, rs_primary_cut_slot* slot, const rs_primary_cut_key* key, int tilesX, int tilesY,
                                    int* cutState, rs_primary_cut_sizes* sizes);
/* The choice of the internal streams as plain data (restir_amd/csrc/rs_stream_choice.h; rs_set_internal_stream_priority above says what
 * is chosen).  Levels: 0 high, 1 normal, 2 low.  Stream handles are opaque here.  A choice is the internal streams made for one caller
 * stream under one level key (the asked level -1 / 0 / 1, or 2 for automatic), the priority they were made at and, when they were chosen by
 * measurement, the chosen streams' time and the fastest candidates' (zeros: plain streams).  The state is the current choice, what it
 * holds, what the next use has to do first, and the choices kept for other callers and keys, oldest first. */
#ifndef RS_AUX_STREAMS
#define RS_AUX_STREAMS 3
#endif
#define RS_STREAM_CHOICES_KEPT 4
#define RS_STREAMS_HELD_NONE     0   /* no stream made yet */
#define RS_STREAMS_HELD_MEASURED 1   /* chosen by measurement */
#define RS_STREAMS_HELD_PLAIN    2   /* nothing could be measured: made one by one at the level the rule names */
#define RS_STREAMS_PENDING_NONE         0
#define RS_STREAMS_PENDING_AGAIN        1   /* another caller stream or preference: choose again on next use, keep what was measured */
#define RS_STREAMS_PENDING_AGAIN_FORGET 2   /* rs_choose_internal_streams_again: the kept choices go as well */
typedef struct rs_stream_choice { void* caller; int levelKey; void* stream[RS_AUX_STREAMS]; int priority; double chosenUs, fastestUs; } rs_stream_choice;
typedef struct rs_stream_choices { rs_stream_choice current; int held, pending, numKept; rs_stream_choice kept[RS_STREAM_CHOICES_KEPT]; } rs_stream_choices;
typedef struct rs_stream_choice_inputs {
    int least, greatest;        /* the device's stream priority range (hipDeviceGetStreamPriorityRange) */
    int asked;                  /* -1 / 0 / 1, 2 = automatic */
    int callerHasStream, callerPriority;   /* the library stream is not the default stream; its priority */
    double timesUs[3][4];       /* per level: the time of the triple "all four candidates but this one"; levels not in the order are not read */
} rs_stream_choice_inputs;
typedef struct rs_stream_choice_plan {
    int order[3], numLevels;    /* the levels that are measured, preferred first */
    int level, skip;            /* the level chosen and the candidate left out; -1, -1: nothing chosen */
    double fastestUs;
    int plainPriority;          /* the priority of plain streams */
} rs_stream_choice_plan;
/* Test hooks, host only.  The first evaluates the level order, the pick among measured times and the priority of plain streams.  The
 * second is what the first use after a change does to the state: the current choice is kept (measured) or released (plain, or forget:
 * then every kept one too), the oldest kept choice is released when a fifth arrives, and a kept choice for (caller, levelKey) becomes
 * current.  released[RS_STREAM_CHOICES_KEPT + 1]: the choices whose streams the caller has to destroy. */
int  rs_debug_plan_stream_choice(const rs_stream_choice_inputs* in, rs_stream_choice_plan* out);
int  rs_debug_plan_stream_switch(rs_stream_choices* state, int forget, void* caller, int levelKey, rs_stream_choice* released, int* numReleased);
/* Test hook: the per-pixel state the primary rays of the last ended frame left for the later passes (host arrays of width * height
 * pixels): 4 floats { hit position, tag bits }, 4 floats { shading normal, metallic }, 2 words { sampler state, tag }.  Waits for the
 * device. */
int  rs_debug_restir_surface(rs_restir* r, float* posTag, float* normal, unsigned* rngTag);
/* ... and the plane next to them: 4 floats { wo, roughness }, written only for pixels of a MetallicWorkflow material (the others hold
 * whatever the set held before). */
int  rs_debug_restir_surface_wo(rs_restir* r, float* wo4);
#define RS_SPATIAL_HALO_ROWS 5           /* taps reach y-4..y+5 (src/restir.cu:49-56) */
/* bytes needed for `rows` rows of published reservoirs */
size_t rs_restir_halo_bytes(const rs_restir* r, int rows);
int  rs_restir_halo_pack(const rs_restir* r, int y0, int rows, void* devBuffer);
int  rs_restir_halo_unpack(rs_restir* r, int y0, int rows, const void* devBuffer);
/* Same packing for any of the three reservoir buffers (which: as rs_restir_download); which = 1 after
 * rs_restir_end_frame is the history the next frame's temporal merge reads. */
size_t rs_restir_rows_bytes(const rs_restir* r, int which, int rows);
int  rs_restir_rows_pack(const rs_restir* r, int which, int y0, int rows, void* devBuffer);
int  rs_restir_rows_unpack(rs_restir* r, int which, int y0, int rows, const void* devBuffer);
/* Debug / parity: copy a reservoir buffer to host as the reference's AoS records.
 * which: 0 = devDirectReservoir (next frame's output slot), 1 = devLastDirectReservoir (last
 * written), 2 = devDirectTemp. */
int  rs_restir_download(const rs_restir* r, int which, rs_reservoir* host);
int  rs_restir_upload(rs_restir* r, int which, const rs_reservoir* host);
/* Temporal re-evaluation under changed emission (rs_scene_set_emission).  Default 0: the reference's merge, which reuses
 * last frame's sample with the Li and weight it was drawn with (src/restir.cu:180-185) -- a light just switched off can
 * keep winning the merge for many frames.  1: the RIS passes record the light-sampler index of their winner, the
 * reservoirs carry it, and the temporal merge rescales the reused sample to the current emission first,
 * W *= luminance(Le_now) / luminance(Li) and Li = Le_now (not for the environment map's entry, an unknown light or
 * W = 0); so is the published copy the spatial pass gathers from where a pixel shaded nothing this frame and keeps an
 * older reservoir.  With no edit the results are bit-identical to 0.  Switching on starts every reservoir's light as
 * unknown.
 * Costs 16 B/px of memory traffic per frame (RIS writes 4, the temporal merge reads 8 and writes 4).  A tracked rs_restir is refused by
 * rs_strips_frame / rs_strips_exchange_history with RS_ERR_UNSUPPORTED unless the driver was told: rs_strips_set_light_tracking. */
int  rs_restir_set_light_tracking(rs_restir* r, int enable);
/* The light-sampler index of every reservoir's sample, width x height ints; which as rs_restir_download.  -1 = none
 * or unknown (all -1 while tracking is off).  Waits for the library stream.  On a rank of the strip driver the rows of which = 2 (the
 * published copy) outside the rank's strip mean nothing: the border rows of a frame travel without their ids (rs_strips_frame). */
int  rs_restir_download_light_ids(const rs_restir* r, int which, int* host);
/* Rows of the id plane that goes with reservoir buffer `which` (as rs_restir_download_light_ids), 4 B/px: what a history message
 * carries next to rs_restir_rows_pack(r, 1, ...) when the lights are tracked.  Enqueue-only, like rs_restir_rows_pack.  Refused with
 * RS_ERR_INVALID_ARGUMENT while tracking is off, for rows outside the frame and for a devBuffer that is not 4-byte aligned. */
size_t rs_restir_light_rows_bytes(const rs_restir* r, int rows);
int  rs_restir_light_rows_pack(const rs_restir* r, int which, int y0, int rows, void* devBuffer);
int  rs_restir_light_rows_unpack(rs_restir* r, int which, int y0, int rows, const void* devBuffer);
/* Light retargeting: temporal reuse follows lamps that rs_scene_set_geometry / rs_scene_set_part_transforms moved.  On top of light
 * tracking (switching it on switches tracking on; rs_restir_set_light_tracking(r, 0) switches both off).  Every reservoir's sample
 * carries a record { light-sampler index, the barycentric pair (u, v) it was drawn at, the solid-angle pdf it last had }; light = -1:
 * none or unknown.  In the temporal merge of a shaded pixel whose history slot passes the reference's neighbour test, a candidate of a
 * light that an edit has named since this rs_restir's previous frame -- not the environment map's entry, not an unknown light, not W = 0
 * -- is evaluated again from the pixel's own surface on the current light records before it is merged:
 *   (Li', wi', dist', pdf') = the light's sample at (u, v) seen from the pixel; W = 0 if it faces away now or pdf' is not finite and positive;
 *   W = (W * (pNew / pOld)) * (pdfOld / pdf'), p = luminance(Li * BSDF(wi) * cos) of the old and the new sample (0 unless pOld, pdfOld
 *   are finite and positive); Li, wi, dist and the record's pdf become the new ones; M stays; a sample left with W != 0 walks its shadow
 *   segment (one ray in rs_restir_ray_count) and is cleared when occluded.
 * Every other candidate takes today's path, the emission rescale of tracking included.  The history buffers are not written.  Slots of
 * pixels that shade nothing this frame, and the published copies they keep, have no surface to evaluate from: they are treated as
 * tracking treats them (emission rescale only).  Moved occluders are rs_restir_set_shadow_revalidation's (below).
 * With no emitter moved since the previous frame nothing extra is launched, and the results equal tracking's bit for bit.
 * Stream-ordered like tracking; a failed allocation leaves it off with nothing changed.  Switching on marks every record AND every tracked light id
 * unknown (ids that tracking carried so far have no record to go with), and edits made before the switch are taken as seen;
 * rs_restir_upload and a change of scene mark records unknown.  Memory: 164 B/px.  While it is on, rs_restir_light_rows_pack / _unpack,
 * rs_strips_frame and rs_strips_exchange_history are refused with RS_ERR_UNSUPPORTED: their 4 B/px do not carry the records. */
int  rs_restir_set_light_retargeting(rs_restir* r, int enable);
int  rs_restir_get_light_retargeting(const rs_restir* r, int* enabled);
typedef struct rs_light_sample { int light; float u, v, pdf; } rs_light_sample;
/* The record of every reservoir's sample, width x height; which as rs_restir_download_light_ids.  All { -1, 0, 0, 0 } while retargeting
 * is off.  Waits for the library stream. */
int  rs_restir_download_light_samples(const rs_restir* r, int which, rs_light_sample* host);
/* Test hook: what the retargeting kernel did in the last ended frame: out[0] samples evaluated again, out[1] shadow segments walked,
 * out[2] samples left with W = 0.  All 0 when the frame launched no such kernel (no lamp moved since the frame before). */
int  rs_debug_restir_retarget(rs_restir* r, unsigned long long out[3]);
/* ... and whether that frame launched the kernel at all: 1 or 0.  Host only. */
int  rs_debug_restir_retarget_launched(rs_restir* r, int* launched);
/* Shadow revalidation: temporal reuse notices occluders that rs_scene_set_triangles / rs_scene_set_geometry / rs_scene_set_part_transforms
 * moved.  The reference tests visibility once, on the RIS winner, so a temporal reservoir keeps the weight it had when its
 * shadow segment was free, and a floor behind a door that has just closed stays lit from history for up to the M clamp's 20 frames.
 * Off by default; independent of light tracking and retargeting (all three light modes).  While it is on, a phase-A call that merges
 * temporally (reuse & 1, not the first frame) launches one extra pass before the merge when the scene's count of accepted geometry edits
 * (rs_scene_geometry_edits) differs from what this rs_restir saw at its previous frame, or the scene is another one.  The pass examines
 * the temporal candidate of every shaded pixel of the call's rows whose history slot j = motion[i] passes the reference's neighbour test
 * and holds W != 0 -- except, with retargeting on, a candidate that pass has just evaluated again.  Its segment runs from the pixel's own
 * position of this frame to pos + wi * dist (wi, dist of slot j).  The segment is walked when its bounding box overlaps the box of one of
 * the edits made since the previous frame (closed intervals: touching counts; a NaN coordinate never does) -- the scene keeps the boxes
 * of its last RS_DIRTY_BOXES_KEPT edits, each the exact bounds of the old and the new corners of the triangles the edit named -- or,
 * when an edit of that interval has left the ring or the scene changed, always.  A walked segment counts as one ray in
 * rs_restir_ray_count / _total.  A candidate found occluded is merged as if its slot held W = 0: its M is added and it is never selected
 * (the reference's own convention for a blocked shadow ray).  The history buffers are not written (with a moving camera two pixels read
 * one slot), published copies of pixels that shade nothing this frame and ReSTIR-GI's reservoirs are not touched (those are rs_restir_set_indirect_revalidation's, below).
 * A frame without an edit since the previous one launches exactly the kernels it launches with the switch off.  Stream-ordered, no host
 * wait; the boxes are chosen on the host when the frame is enqueued.  Switching on takes the edits made so far as seen; a failed
 * allocation leaves it off with nothing changed.  Memory: 4 B/px from the first switch-on.  Row bands and the strip driver's ranks
 * revalidate their own rows; every rank applies the same edits. */
#define RS_DIRTY_BOXES_KEPT 8
int  rs_restir_set_shadow_revalidation(rs_restir* r, int enable);
int  rs_restir_get_shadow_revalidation(const rs_restir* r, int* enabled);
/* Accepted geometry edits of the scene so far (host only), and what a frame whose previous frame saw sinceEdit of them would take now:
 * *count boxes -- the first min(*count, capacity) in boxes6, { lo xyz, hi xyz } each, oldest edit first -- or *everything = 1 (then
 * *count = 0) when one of those edits has left the ring.  Host only. */
int  rs_scene_geometry_edits(const rs_scene* scene, unsigned long long* count);
int  rs_scene_dirty_boxes(const rs_scene* scene, unsigned long long sinceEdit, int capacity, float* boxes6, int* count, int* everything);
/* Test hooks.  What the revalidation pass did in the last ended frame: out[0] candidates examined, out[1] segments walked, out[2]
 * candidates found occluded; all 0 when the frame launched no such pass.  Waits for the library stream. */
int  rs_debug_restir_revalidate(rs_restir* r, unsigned long long out[3]);
/* ... and whether that frame launched the pass at all: 1 or 0.  Host only. */
int  rs_debug_restir_revalidate_launched(rs_restir* r, int* launched);
/* Host only (restir_amd/csrc/rs_revalidate_plan.h).  The dirty box of an edit of `count` records over a table of numPrims triangles: old
 * corners from oldVertices (9 floats per primitive), new ones from newVertices (9 per record); an id named twice takes its last record. */
int  rs_debug_plan_dirty_box(int numPrims, const float* oldVertices, int count, const int* primIds, const float* newVertices, float lo[3], float hi[3]);
/* numEdits edits numbered firstEdit, firstEdit + 1, ... with the boxes boxes6 enter an empty ring one after the other; then a frame whose
 * previous frame saw `seen` edits chooses at `now`: *launch, *everything, *n boxes (outBoxes6, room for RS_DIRTY_BOXES_KEPT, may be null). */
int  rs_debug_plan_revalidation(int numEdits, unsigned long long firstEdit, const float* boxes6, unsigned long long seen, unsigned long long now, int sameScene,
                                int* launch, int* everything, int* n, float* outBoxes6);
/* n segments { a xyz, b xyz } against m <= RS_DIRTY_BOXES_KEPT boxes { lo xyz, hi xyz }, or against "everything": flags[i] = 1 where the
 * segment is walked -- the function the kernel evaluates per lane. */
int  rs_debug_segment_in_boxes(int n, const float* segments6, int m, const float* boxes6, int everything, unsigned char* flags);
/* Indirect revalidation: ReSTIR-GI's temporal reuse drops the history samples that a geometry edit made stale.  A
 * Reservoir<IndirectLiSample> holds a visible point xv, a sample point xs and the radiance Lo that once arrived from xs; after a door
 * closes or a prop is carried away a slot may keep an xs that hangs in the air or lies behind the door, and with M clamped at 20 it keeps
 * winning merges for tens of frames.  Off by default; independent of light tracking, retargeting and shadow revalidation.
 * When the pass runs: an rs_restir_indirect call runs one extra pass before its path kernel when the call merges temporally (reuse & 1,
 * not the first frame, reservoirs not allocated by this very call) and the scene's count of accepted geometry edits differs from what this
 * rs_restir saw at its previous rs_restir_indirect call, or the scene is another one (the choice shadow revalidation makes, from the same
 * ring of RS_DIRTY_BOXES_KEPT boxes).  The previous call's scene and count are noted on every accepted rs_restir_indirect call, with the
 * switch on or off, apart from what rs_restir_direct notes.
 * The pass has one lane per slot j of the width x height history buffer the call is about to merge from; the verdict depends on the slot
 * alone -- both ends of the segment are stored in it -- so two pixels that read one slot cannot disagree, and the history is edited in place.
 * A slot is examined iff its weight is neither NaN nor infinite, weight > 0, and xv == xs does not hold on all three components (IEEE ==).
 * When an edit of the interval has left the ring or the scene is another one ("everything"), every examined slot is stale and nothing
 * walks.  Otherwise, in this order: the slot is stale iff xs lies in one of the frame's dirty boxes (closed: lo <= xs <= hi on every axis;
 * a NaN coordinate never lies in one); else its segment xv -> xs is walked iff its bounding box overlaps a dirty box (the test of
 * rs_debug_segment_in_boxes); a walked segment is the reference's testOcclusion(xv, xs) on the current geometry and counts as one ray
 * in the `rays` the call returns.  A stale slot and an occluded walker are dropped: numSamples = 0 and weight = 0, the sample fields stay.
 * The path kernel then merges an empty candidate, draws its random number and never selects it, exactly as for a neighbour that fails
 * the reference's neighbour test.  Dropped, not kept with W = 0 and its M: an occluded GI sample is not a sample of zero radiance, and
 * its M would darken the pixel for 20 frames.
 * A call without an accepted geometry edit since the previous rs_restir_indirect call launches exactly what it launches with the switch
 * off and leaves every buffer bit for bit the same.  Stream-ordered, no host wait but the one `rays` asks for; a failed allocation leaves
 * it off with nothing changed.  Memory: 16 KB of counters from the first switch-on, no per-pixel plane.
 * Deliberately left as it is: emission, material and texture edits dirty no box, so a stale Lo stays stale.  The spatial pass
 * (rs_restir_set_indirect_spatial, below) reads the temporal buffer after the path kernel and writes a buffer nothing merges from, so
 * it has nothing to revalidate: its winners are tested on the current geometry. */
int  rs_restir_set_indirect_revalidation(rs_restir* r, int enable);
int  rs_restir_get_indirect_revalidation(const rs_restir* r, int* enabled);
/* Test hooks.  What the pass did in the last rs_restir_indirect call: out[0] slots examined, out[1] found stale, out[2] segments walked,
 * out[3] walkers found occluded; all 0 when the call launched no such pass.  Waits for the library stream. */
int  rs_debug_restir_indirect_revalidate(rs_restir* r, unsigned long long out[4]);
/* ... and whether that call launched the pass at all: 1 or 0.  Host only. */
int  rs_debug_restir_indirect_revalidate_launched(rs_restir* r, int* launched);
/* Host only (restir_amd/csrc/rs_indirect_revalidate.h).  n reservoirs against m <= RS_DIRTY_BOXES_KEPT boxes { lo xyz, hi xyz }, or
 * against "everything": classes[i] = 0 not examined, 1 stale, 2 walk, 3 examined and kept -- the function the kernel evaluates per lane. */
int  rs_debug_indirect_candidate_classes(int n, const rs_indirect_reservoir* reservoirs, int m, const float* boxes6, int everything, unsigned char* classes);
/* BVH walks (intersect + testOcclusion calls) performed by the last rs_restir_direct / phase_a,
 * for the Mrays/s metric. Synchronises. */
int  rs_restir_ray_count(rs_restir* r, unsigned long long* rays);
/* Sum of the walk counters of the last `frames` (<= 1024) frames. Synchronises. */
int  rs_restir_ray_total(rs_restir* r, int frames, unsigned long long* rays);
/* Per-pass GPU time (ms) of the last frame, measured with hipEvents on the library's stream:
 * ms[0] primary hit, ms[1] RIS, ms[2] shadow+temporal, ms[3] spatial+shade.  Synchronises. */
int  rs_restir_pass_times(rs_restir* r, float ms[4]);
/* Enables the hipEvent bracketing above (off by default: it adds 5 event records per frame).  enable = 2: only the spatial pass is
 * bracketed (ms[3]) and the launches stay where the overlapped mode puts them: the pass's duration while the kernels of other
 * frames share the CUs with it. */
int  rs_restir_enable_timing(rs_restir* r, int enable);
/* enable_timing(r, 2) keeps the two events of the last 256 frames: their spans (ms, oldest first; *count of them, at most `capacity`).
 * Nothing waits inside the frames -- what the pass costs while other frames' kernels share the CUs.  Waits for the library stream. */
int  rs_restir_spatial_times(rs_restir* r, float* ms, int capacity, int* count);
/* 1: the spatial pass is launched under the name k_spatial_shade_probe (the same code) until 0 -- for the launches a measurement
 * makes for itself, so that a kernel trace of the process tells them from the launches of the frames. */
int  rs_restir_set_probe(rs_restir* r, int enable);
/* Test hook: the spatial pass estimates tap positions with the hardware sqrt/sin/cos and falls back
 * to the exact evaluation inside an error band; this returns the largest estimate error over n
 * pseudo-random samples so a test can assert the band really covers it. */
int  rs_debug_tap_estimate_error(int n, float* maxErr);
/* Test hook: the light sampler takes the square root of a uniform variate without the general expansion's range scaling and
 * class test (rs_surface.h sqrt_of_uniform); this compares it with the exactly rounded sqrtf on every value the generator can
 * return (2^31 - 2 of them) and returns the number of differing results. */
int  rs_debug_sqrt_of_uniform_mismatches(unsigned long long* mismatches);
/* Test hook: the EAW filter divides by a sigma that is not a power of two in three instructions (Markstein's form, denoiser.hip
 * div_sigma); this compares it with the IEEE division on every float in [2^-100, 2^100] and returns the number of differing quotients. */
int  rs_debug_div_sigma_mismatches(float sigma, unsigned long long* mismatches);
/* The same for every value the Sobol sampler can return: 0 and all floats in [2^-32, 1] (2^28 + 2 of them). */
int  rs_debug_sqrt_of_unit_floats_mismatches(unsigned long long* mismatches);
/* Test hook for restir_amd/csrc/rs_exact.h (the short forms of 1 / d, x / d and sqrt(x) the kernels use for operands in [2^-60, 2^60)),
 * each compared with the compiler's correctly rounded operator.  op 0: the reciprocal of EVERY float in the range and of its negative; op 1: the square root
 * of every float in the range; op 2: the quotient x / d for the denominators 1.s * 2^expD, s in [firstSig, firstSig + countSig) (at most
 * 65 536 per call), each against ALL 2^23 numerators 1.t * 2^expX; op 3 / 4 / 5: the same with negative numerators / a negative denominator /
 * both.  out3[0] = results that differ (must be 0), out3[1] = operands
 * (pairs) compared, out3[2] reserved.  tools/verify_exact_division.py walks op 2 over all 2^23 denominators: every pair of significands. */
int  rs_debug_exact_ops_mismatches(int op, unsigned firstSig, unsigned countSig, int expX, int expD, unsigned long long* out3);
/* Test hook: the default sampler's generator keeps its state minus one and steps that (restir_amd/csrc/rs_math.h Rng), and the RIS
 * loop compares two of a candidate's draws before their division by 2^31, against a scaled light count and a scaled alias threshold.
 * For EVERY state x in [1, 2^31 - 2] this compares, with the step x' = 48271 x mod (2^31 - 1) and the draw float(x' - 1) / 2^31
 * written out as they were: the next state and the bits of the draw (also of the form that steps x itself, which k_path takes: Rng and
 * RngOnX), the sampler entry the draw picks of 1, 3, 1 024, 1 500, 10 240 and
 * 2^24 + 1 lights, and `draw < prob` for prob = 0, the smallest subnormal, 2^-31, 0.5, the float below 1, 1, 2 and a NaN.
 * out2[0] = results that differ (must be 0), out2[1] = results compared (19 per state). */
int  rs_debug_rng_step_mismatches(unsigned long long* out2);
/* The same comparison of the same shared code on the host, for the `count` states from `first` on (all in [1, 2^31 - 2]): needs no device. */
int  rs_debug_rng_step_host_mismatches(unsigned first, unsigned count, unsigned long long* out2);
/* Test hook for restir_amd/csrc/rs_surface.h: the functions under the textured and environment-map kernel variants, unchanged, one
 * lane per element of a batch of n, on host arrays.  op 0: linear_sample of (u, v) on the texture texWidth x texHeight of packed RGB
 * `texels` (n x 2 -> n x 3); op 1: procedural_texture of (u, v) (n x 2 -> n x 3); op 2: to_sphere of (u, v) (n x 2 -> n x 3);
 * op 3: to_plane of a direction (n x 3 -> n x 2); op 4: local_to_world of (normal, vector) (n x 6 -> n x 3).  The texture arguments
 * are read by op 0 only.  Refused with RS_ERR_INVALID_ARGUMENT: an op outside 0..4, null in / out, n < 0 or above 2^26, and for op 0
 * null texels, a width or height that is not positive, more than 2^26 texels.  Waits for the library stream.
 * tests/test_gpu_surface_ops.py holds every op to the oracle's function bit for bit. */
int  rs_debug_surface_ops(int op, int n, const float* in, float* out, int texWidth, int texHeight, const float* texels);

/* ---- framebuffer tiling across the GPUs of one node: the row-strip frame of one rank ------------------------------------------
 * One process per GPU, the scene replicated, the framebuffer of runCuda (src/main.cpp:146-185) cut into `world` row strips.  A rank
 * renders the G-buffer and phase A on its rows, sends its 5 border rows of published reservoirs and of the G-buffer id / normal /
 * depth planes to the strip above and below (68 B/px, the only exchange; taps reach y-4..y+5, src/restir.cu:49-56), runs phase B on
 * its interior rows while they travel and on the two border bands after they have arrived.  Results equal the full-frame
 * rs_restir_direct bit for bit.  The EAW filter on the strip (config 5), the history exchange a moving camera needs and the
 * assembly of the image go through the same transport (rs_strips_eaw_filter / _exchange_history / _gather).  One frame of a rank:
 *     rs_strips_frame;  [rs_strips_eaw_filter;]  rs_gbuffer_update;  [rs_strips_exchange_history;]  [tone map;  rs_strips_gather]
 * (restir_amd/tiling.py drives the same calls from Python.) */
typedef struct rs_comm rs_comm;
typedef struct rs_strips rs_strips;
/* The exchange, as two grouped operations on device buffers.  stream_ordered != 0: send / recv enqueue on `hipStream` and the
 * buffers are touched in stream order (RCCL); 0: they are host calls that complete at group_end at the latest (the frame then
 * hands over a finished library stream and waits for group_end before it unpacks). */
typedef struct rs_transport {
    void* ctx;
    int (*group_begin)(void* ctx);                 /* may be null */
    int (*send)(void* ctx, const void* devBuffer, size_t bytes, int peer, void* hipStream);
    int (*recv)(void* ctx, void* devBuffer, size_t bytes, int peer, void* hipStream);
    int (*group_end)(void* ctx);                   /* may be null */
    int stream_ordered;
} rs_transport;
/* ncclComm: an ncclComm_t of `world` ranks created by the caller (ncclCommInitRank); librccl.so is opened at run time, the
 * transfers are ncclSend / ncclRecv (ncclUint8) inside ncclGroupStart / ncclGroupEnd on the library stream (rs_set_stream), between
 * the launch that packs the border rows and the launch that unpacks the neighbours'; rs_strips_set_comm_stream(strips, 1) puts them on
 * a stream of the strip driver instead, with phase B's interior rows next to them (a fifth stream that hands events to the others, and the
 * device runs four of those side by side: the frames then keep two chains in flight instead of three -- 0.17 -> 0.28 ms per frame on a 1/8
 * strip of 1080p with a transport that moves nothing, DESIGN.md sections 4 and 5).  Create the communicator before the first overlapped frame or call rs_choose_internal_streams_again() after it. */
int  rs_comm_create_rccl(void* ncclComm, int rank, int world, rs_comm** comm);
/* The same, naming the copy of RCCL that created ncclComm (a process can hold two: PyTorch wheels bundle their own librccl.so).
 * librcclPath NULL or "" = rs_comm_create_rccl's search: symbols the process has linked or loaded globally, else a copy already
 * loaded under the soname librccl.so.1 (nothing new is mapped), else a fresh local open of librccl.so.1. */
int  rs_comm_create_rccl_lib(void* ncclComm, int rank, int world, const char* librcclPath, rs_comm** comm);
int  rs_comm_create(const rs_transport* transport, int rank, int world, rs_comm** comm);
int  rs_comm_destroy(rs_comm* comm);
/* one-rank check of a transport: `bytes` of devSend travel to this rank itself into devRecv, grouped and ordered as in a frame */
int  rs_comm_self_exchange(rs_comm* comm, const void* devSend, void* devRecv, size_t bytes);
/* bounds: world + 1 row offsets (bounds[0] = 0, bounds[world] = height, strips of at least 5 rows), or null for equal heights */
int  rs_strips_create(rs_comm* comm, int width, int height, const int* bounds, rs_strips** strips);
int  rs_strips_destroy(rs_strips* strips);
int  rs_strips_rows(const rs_strips* strips, int* y0, int* y1);
/* Stream-ordered transports (RCCL): 0 (default) = the transfers are enqueued on the library stream, in order with the packing and
 * unpacking copies; 1 = on a stream of the driver, ordered by events, so that the interior rows of phase B run while the border rows
 * travel.  Same results.  Call between frames with no gather in flight. */
int  rs_strips_set_comm_stream(rs_strips* strips, int ownStream);
/* Rows of the G-buffer id / normal / depth planes that travel with the 5 reservoir rows of an edge: 5 (default) for the spatial taps; 32 when a
 * denoiser follows (src/main.cpp:160-170), whose own exchange of those rows -- a packing launch, a group and an unpacking launch per frame -- is
 * then skipped.  The same value on every rank; strips of at least that many rows; between frames. */
int  rs_strips_set_gbuffer_halo(rs_strips* strips, int rows);
/* Light tracking (rs_restir_set_light_tracking) through the driver.  0 (default): a tracked rs_restir is refused with RS_ERR_UNSUPPORTED.
 * 1: rs_strips_frame and rs_strips_exchange_history take a tracked rs_restir and refuse an untracked one with RS_ERR_INVALID_ARGUMENT.
 * The border rows of a frame stay 68 B/px (no pass reads a neighbour's ids); every message of rs_strips_exchange_history becomes
 * reservoir rows (40 B/px), G-buffer rows (20), then the reservoirs' light ids (4), so that after it the which = 1 reservoirs and ids of
 * ALL rows equal the full frame's on every rank.  A setting of the driver, not read off the rs_restir, because it is the size of the
 * messages: the same value on every rank; between frames, with no gather in flight.  With one rank the frames equal a tracked
 * rs_restir_direct. */
int  rs_strips_set_light_tracking(rs_strips* strips, int enable);
/* GBuffer::render + ReSTIRDirect of this rank's rows; GBuffer::update stays with the caller, as in runCuda.  Afterwards rows
 * [y0, y1) of devDirectIllum hold the frame's radiance. */
int  rs_strips_frame(rs_strips* strips, rs_restir* r, const rs_scene* scene, const rs_camera* cam, rs_gbuffer* g,
                     float* devDirectIllum, int iter, int looper, int reuse);
/* LeveledEAWFilter::filter (src/denoiser.cu:453-477) on the strip's rows of devColor (a full-frame sized image): the 32 G-buffer
 * rows beyond each edge arrive once, the 2 << level border rows of every level's input before that level.  *devResult is a buffer
 * of the driver whose rows [y0, y1) equal the full-frame rs_eaw_filter's.  Strips of at least 32 rows; call before
 * rs_gbuffer_update; the rows of devColor and of the current G-buffer planes just outside the strip are overwritten. */
int  rs_strips_eaw_filter(rs_strips* strips, rs_eaw* f, rs_gbuffer* g, const rs_camera* cam, float* devColor, float** devResult);
/* SpatioTemporalFilter::filter (src/denoiser.cu:532-564) on the strip: the 32 G-buffer rows beyond each edge arrive once, one row of
 * the accumulated moments after the temporal accumulation, the 2 * step + 1 border rows of every level's input colour and of the
 * variance before that level.  Rows [y0, y1) of the result equal the full-frame rs_svgf_filter's; *devColorOut is handed over as by
 * rs_svgf_filter.  Strips of at least 33 rows; call before rs_gbuffer_update, then rs_svgf_next_frame.  With a moving camera the
 * filter's history (accumulated colour and moments, 24 B/px) travels to every rank by rs_strips_exchange_svgf_history, called after
 * the filter and before rs_svgf_next_frame. */
int  rs_strips_svgf_filter(rs_strips* strips, rs_svgf* f, rs_gbuffer* g, const rs_camera* cam, const float* devColorIn, float** devColorOut);
int  rs_strips_exchange_svgf_history(rs_strips* strips, rs_svgf* f);
/* Moving camera (findTemporalNeighbor reads the reprojected pixel of the last frame, src/restir.cu:20-45, which may belong to
 * another strip): every rank's rows of the reservoirs the next temporal merge reads and of the "last" G-buffer planes travel to
 * every other rank (60 B/px; 64 with rs_strips_set_light_tracking).  Call after rs_gbuffer_update.  Not needed for a static camera
 * (the reference's default). */
int  rs_strips_exchange_history(rs_strips* strips, rs_restir* r, rs_gbuffer* g);
/* Image assembly: rows [y0, y1) of every rank's devImage (full-frame sized, bytesPerPixel bytes per pixel: 12 for the radiance
 * image, 4 for the display image) arrive in the same rows on rank `root`, or on every rank for root = -1. */
int  rs_strips_gather(rs_strips* strips, void* devImage, size_t bytesPerPixel, int root);
/* The same, overlapped with the next frame: _begin records the transfers, which then travel in the next transfer group the driver
 * posts (the border rows of the next rs_strips_frame: one RCCL group per frame) or, failing that, in a group of their own posted by
 * _end; _end returns with the transfers ordered before whatever is enqueued on the library stream next (call it before devImage is
 * written again or read on root).  devImage's rows must be final on the library stream when the next group is posted, i.e. enqueue
 * their producer before rs_strips_frame.  slot in [0, 4) names a gather in flight; every rank begins the same gathers in the same
 * order (all transfers of a strip driver share one stream). */
int  rs_strips_gather_begin(rs_strips* strips, void* devImage, size_t bytesPerPixel, int root, int slot);
int  rs_strips_gather_end(rs_strips* strips, int slot);
/* Measurement: with timing enabled rs_strips_frame brackets the library stream's wait for the neighbours' border rows with two
 * events; rs_strips_halo_wait_ms returns that span for the last frame -- the part of the exchange's latency that the interior rows
 * of phase B did not hide (about 0 when the rows had arrived in time).  It waits for that frame. */
int  rs_strips_enable_timing(rs_strips* strips, int enable);
int  rs_strips_halo_wait_ms(rs_strips* strips, float* ms);

/* ---- path-trace baseline (src/pathtrace.h:12-16) ---------------------------------------- */
int  rs_path_trace_init(void);            /* pathTraceInit (src/pathtrace.cu:23-25) */
int  rs_path_trace_free(void);            /* pathTraceFree (:27-28) */
/* pathTraceDirect (src/pathtrace.cu:457-476) -> PTDirectKernel (:279-328) */
int  rs_path_trace_direct(const rs_scene* scene, const rs_camera* cam, float* devDirectIllum,
                          int iter, int looper, unsigned long long* rays);

/* pathTrace(direct, indirect, iter) -> singleKernelPT (src/pathtrace.cu:156-277,434-455) and pathTraceIndirect ->
 * PTIndirectKernel (:330-432,478-497); maxDepth = Settings::traceDepth */
int  rs_path_trace(const rs_scene* scene, const rs_camera* cam, float* devDirectIllum, float* devIndirectIllum,
                   int iter, int looper, int maxDepth, unsigned long long* rays);
int  rs_path_trace_indirect(const rs_scene* scene, const rs_camera* cam, float* devIndirectIllum,
                            int iter, int looper, int maxDepth, unsigned long long* rays);
/* ReSTIRIndirect(devIndirectIllum, iter, gBuffer) (src/restir.cu:233-416,448-476): one path per pixel into a
 * Reservoir<IndirectLiSample>, temporal reuse (reuse bit 0), clamp<20>; shares the first-frame flag with rs_restir_direct.
 * With rs_restir_set_indirect_revalidation on, a call after a geometry edit first drops the history's stale slots; the segments that
 * pass walks are part of *rays. */
int  rs_restir_indirect(rs_restir* r, const rs_scene* scene, const rs_camera* cam, const rs_gbuffer* g, float* devIndirectIllum,
                        int iter, int looper, int reuse, int maxDepth, unsigned long long* rays);
/* which: 0 = the buffer the next call writes, 1 = the one the last call wrote (devIndLastTemporalReservoir) */
int  rs_restir_download_indirect(rs_restir* r, int which, rs_indirect_reservoir* host);

/* ---- ReSTIR-GI: spatial reuse of the indirect reservoirs --------------------------------------------------------------------------
 * The reference allocates devIndSpatialReservoir (src/restir.cu:15) and never writes it: its ReSTIR-GI is the temporal half only.  This
 * is the spatial half, opt-in and off by default; with it off every launch, buffer and image of rs_restir_indirect is bit for bit what it
 * is without this section.  A GI sample is reused across pixels by reconnecting the neighbour's sample point xs to the receiving pixel's
 * visible point; the weight is corrected by the Jacobian of that shift (Ouyang et al., "ReSTIR GI: Path Resampling for Real-Time Path
 * Tracing", 2021, eq. 11).
 *
 * The setter.  taps in 1..RS_GI_SPATIAL_MAX_TAPS, taps <= 0 selects 5; radius in pixels, finite, in (0, 64], radius <= 0 selects 5.f (the
 * reference's DI values); anything else is refused (also with enable == 0) and changes nothing.  The first switch-on allocates 68 B/px
 * (the spatial reservoirs) + 12 B/px (the path kernel's own image of a call that runs the pass) + 32 KB of counters; the receiver's
 * surface is recomputed, not stored.  A failed allocation leaves the switch off with nothing changed.  Refused while the library stream
 * is being captured.  Independent of every other switch.
 *
 * When the pass runs: in an rs_restir_indirect call iff the switch is on and reuse & 2 -- on the first frame as well, as the DI spatial
 * pass does.  reuse & 2 with the switch off stays ignored, as in the reference.  A call that does not run it launches what it launches
 * with the switch off.
 *
 * The rule.  One launch after the path kernel, when every slot of this call's temporal buffer T is complete; one lane per pixel
 * q = (x, y), index i = y * width + x.  Every expression is a tree of single IEEE float operations, no contraction; dot(a, b) is
 * (a.x * b.x + a.y * b.y) + a.z * b.z.
 *  1. Receiver.  The surface the path kernel computed at its primary hit in this very call: the lane seeds the same engine
 *     seeded(sampleSeq, looper, i, 0), draws sample4D, takes cam.sample(x, y, .) and intersects.  xv_q = the hit position; nv_q = the
 *     normal after getTexturedMaterialAndSurface, negated when dot(nv_q, wo) < 0.f with wo = primWo = -ray.direction
 *     (src/restir.cu:286-288); primMaterial = that material.  The pixel takes part iff the hit exists and the material is neither Light nor
 *     Dielectric.  A pixel that does not take part keeps S[i] = T[i] (all 17 words) and its image value is the one the call gives with
 *     the switch off.
 *  2. Start.  R = T[i] as stored (already clamped) after checkValidity (weight NaN, infinite or < 0: weight = 0, numSamples = 0).  The
 *     engine of the pass is seeded(sampleSeq, looper, i, RS_GI_SPATIAL_DIM).
 *  3. Every tap draws three numbers in this order, accepted or not: sample2D r for the position, then sample1D u for the merge.  The tap
 *     is findSpatialNeighborDisk (src/restir.cu:47-85) with `radius` in place of its constant: rr = sqrt(r.x); theta = (r.y * Pi) * 2.f;
 *     px = int((float(x) + .5f) + (cos(theta) * rr) * radius), py likewise with sin -- cos and sin correctly rounded, the conversion
 *     truncating.  It fails the neighbour test when px, py is outside the image or is q itself, when the G-buffer ids differ, when
 *     dot(normal[i], normal[p]) < .9f, or when |depth[i] - depth[p]| > depth[i] * .1f.
 *  4. Candidate.  A tap that passes yields N = T[p], p = py * width + px.  N invalid (weight NaN, infinite or < 0): rejected, adding
 *     nothing.  N.weight == 0: accepted with w = 0, no geometry evaluated.  N.weight > 0: rejected when N.ns == 0 on all three components
 *     (a first bounce that left the scene has no reconnection vertex); otherwise
 *         vn = N.xv - N.xs;  vq = xv_q - N.xs;  dn2 = dot(vn, vn);  dq2 = dot(vq, vq);  an = |dot(N.ns, vn)|;  aq = |dot(N.ns, vq)|;
 *         jac = ((aq / sqrt(dq2)) * dn2) / ((an / sqrt(dn2)) * dq2)
 *     -- the change of solid-angle measure from the neighbour's visible point to the receiver's.  Rejected, in this order of counting,
 *     when jac is NaN or infinite or jac > RS_GI_SPATIAL_JACOBIAN_MAX ("Jacobian"), then when dot(nv_q, vq) >= 0.f ("horizon": xs is not
 *     above the receiver's horizon).  Otherwise w = N.weight * jac.
 *  5. Merge of an accepted tap (the reference's merge): R.weight = R.weight + w; R.numSamples += N.numSamples; if u * R.weight < w then
 *     R.sample = N.sample with xv, nv replaced by xv_q, nv_q, and the lane's sample is "adopted".  The target is Lo (pHatIndirect), which
 *     does not depend on the receiver: that is why weights add once the Jacobian is in.
 *  6. Visibility, once, on the winner (the reference's own convention for RIS, src/restir.cu:172-176): a lane that adopted a sample walks
 *     testOcclusion(xv_q, R.sample.xs) on the current geometry; blocked: R.weight = 0.f (zeroed, not cleared).  A lane whose winner is its
 *     own sample walks nothing.
 *  7. S[i] = R; nothing reads S in a later call and nothing clamps it.  Shade by src/restir.cu:399-412 with the non-delta factor: when R
 *     is valid, wi = normalize(xs - xv) (v * (1.f / sqrt(dot(v, v)))), L = ((Lo / luminance(Lo)) * weight) / float(numSamples), then
 *     L * (primMaterial.BSDF(nv, primWo, wi) * satDot(nv, wi)); NaN or infinity anywhere gives 0.  The caller's image receives
 *     (image * float(iter) + L) / float(iter + 1) -- the spatial result only.
 *  8. T, the history the next call merges from, everything rs_restir_download_indirect returns and the behaviour of indirect
 *     revalidation equal a run with the switch off, bit for bit.  *rays is the path kernel's count plus one per winner walked.
 * With the Sobol sampler the dimensions 150..197 belong to the pass; the path kernel reaches them only beyond depth 20.
 * Stream-ordered, no host wait but the one `rays` asks for.
 * Not done: the unbiased variant that counts Z over the neighbours' domains, feeding S back into the history, a second spatial
 * iteration, a row-band form, re-evaluating Lo after emission or material edits. */
#define RS_GI_SPATIAL_MAX_TAPS     16
#define RS_GI_SPATIAL_DIM          150     /* sampler dimension of the pass's engine */
#define RS_GI_SPATIAL_JACOBIAN_MAX 10.f
int  rs_restir_set_indirect_spatial(rs_restir* r, int enable, int taps, float radius);
int  rs_restir_get_indirect_spatial(const rs_restir* r, int* enabled, int* taps, float* radius);      /* taps, radius: may be null */
/* devIndSpatialReservoir of the last call that ran the pass (zeros before one); refused before the first switch-on */
int  rs_restir_download_indirect_spatial(rs_restir* r, rs_indirect_reservoir* host);
/* Test hooks.  What the pass did in the last rs_restir_indirect call, in this order: pixels taking part, taps accepted, taps failing the
 * neighbour test, taps rejected for ns == 0, for the Jacobian, for the horizon, winners walked, winners blocked; all 0 when the call did
 * not run the pass.  Waits for the library stream. */
int  rs_debug_restir_indirect_spatial(rs_restir* r, unsigned long long out[8]);
/* ... and whether that call ran the pass at all: 1 or 0.  Host only. */
int  rs_debug_restir_indirect_spatial_launched(rs_restir* r, int* launched);
/* The receiver's surface the pass used, per pixel: xv, nv, wo as float4 (w = 0) and the material id, -1 (and zeros) for a pixel that
 * does not take part.  The planes (52 B/px) exist only once somebody has asked: a first call -- with every output null -- allocates them,
 * later passes record into them, and later calls copy out what the last pass recorded (outputs may be null one by one). */
int  rs_debug_restir_indirect_primary(rs_restir* r, float* xv4, float* nv4, float* wo4, int* matId);
/* Host only: n draws of the library's own sampler seeded(table, iter, index, dim) -- the scene's Sobol table, or the default engine
 * when the scene is null or has none. */
int  rs_debug_seeded_uniforms(const rs_scene* sceneOrNull, int iter, int index, int dim, int n, float* out);

/* ---- display conversion (src/pathtrace.h:8) ---------------------------------------------- */
/* copyImageToPBO(uchar4*, glm::vec3*, w, h, toneMapping, scale) (src/pathtrace.cu:108-113) */
int  rs_copy_image_to_pbo(void* devPBO, const float* devImage, int width, int height, int toneMapping, float scale);
/* the debug-view overloads copyImageToPBO(uchar4*, glm::vec2* / float* / int*, w, h) (src/pathtrace.h:9-11,
 * src/pathtrace.cu:58-106,115-134): gamma only; the int form shows a pixel-index plane such as devMotion */
int  rs_copy_image2_to_pbo(void* devPBO, const float* devImage, int width, int height);
int  rs_copy_imagef_to_pbo(void* devPBO, const float* devImage, int width, int height);
int  rs_copy_imagei_to_pbo(void* devPBO, const int* devImage, int width, int height);

/* ---- viewer interop (src/main.cpp:105-144,176-181, src/preview.cpp:88,112-133) ---------------------------------------------
 * The OpenGL pixel-buffer object of the interactive viewer through HIP's graphics interop, one call per reference call:
 *     cudaGLRegisterBufferObject(pbo)            -> rs_pbo_register(pbo, &p)      (an OpenGL context must be current on the thread)
 *     cudaGLMapBufferObject((void**)&devPBO,pbo) -> rs_pbo_map(p, &devPBO, NULL)  (ordered on the library stream)
 *     copyImageToPBO(devPBO, devImage, ...)      -> rs_copy_image_to_pbo(devPBO, devImage, ...)
 *     cudaGLUnmapBufferObject(pbo)               -> rs_pbo_unmap(p)
 *     cudaGLUnregisterBufferObject(pbo)          -> rs_pbo_unregister(p)
 * (cudaGLSetGLDevice(0) is rs_init(0).)  On a node without a GL context rs_pbo_register fails with the runtime's error. */
typedef struct rs_pbo rs_pbo;
int  rs_pbo_register(unsigned glBuffer, rs_pbo** pbo);
int  rs_pbo_map(rs_pbo* pbo, void** devPBO, size_t* bytes /* may be null */);
int  rs_pbo_unmap(rs_pbo* pbo);
int  rs_pbo_unregister(rs_pbo* pbo);
/* saveImage(false) (src/main.cpp:105-144 with Image::setPixel / savePNG, src/image.cpp:36-58): tone map (0 none, 1 filmic, 2 ACES) and
 * gamma per pixel, stored mirrored in x, clamped, scaled by 255 and truncated; an 8-bit RGB PNG at `path` (the complete file name: the
 * viewer composes "<imageName>.<time>.<samples>samp.png").  The JPEG form (saveImage(true)) is not provided.  Synchronises. */
int  rs_save_image(const char* path, const float* devImage, int width, int height, int toneMapping);
/* the PNG writer by itself (host only): rgb = height rows of width * 3 bytes */
int  rs_write_png(const char* path, const unsigned char* rgb, int width, int height);
/* saveImage(true) (src/main.cpp:138-140): the same tone-mapped, mirrored 8-bit picture through Image::saveJPG (src/image.cpp:60-74:
 * stb_image_write's stbi_write_jpg at quality 90) -- a baseline JFIF file, 4:4:4, Annex-K tables scaled to the quality, AAN float DCT;
 * byte-identical to the reference's file (pinned against its compiled writer).  `path` is the complete file name. */
int  rs_save_image_jpg(const char* path, const float* devImage, int width, int height, int toneMapping);
/* Image::saveJPG's file from bytes that are already clamped and scaled: rgb = height rows of width * 3 bytes. */
int  rs_write_jpg(const char* path, const unsigned char* rgb, int width, int height);

/* ---- EAW denoiser (src/denoiser.h:33-43,72-74) -------------------------------------------- */
int  rs_eaw_create(int width, int height, int level, rs_eaw** f);   /* LeveledEAWFilter::create */
int  rs_eaw_destroy(rs_eaw* f);
/* The members the viewer edits between frames (src/preview.cpp:262-265: LeveledEAWFilter::level and
 * waveletFilter.sigLumin / sigNormal / sigDepth, src/denoiser.h:18-27,41).  create() sets 64 / .2 / 1 (src/denoiser.cu:455).
 * `level` is stored and reported like the reference's member; LeveledEAWFilter::filter runs its five levels whatever it
 * holds (src/denoiser.cu:463-477), and so does rs_eaw_filter. */
int  rs_eaw_set_params(rs_eaw* f, float sigLumin, float sigNormal, float sigDepth, int level);
int  rs_eaw_get_params(const rs_eaw* f, float* sigLumin, float* sigNormal, float* sigDepth, int* level);
/* The levels of step 1, 2 and 4 read their 25 taps from an LDS tile of the block's pixels plus halo (default, 15 % faster per
 * filter call at 1080p) or gather them from memory like the levels of step 8 and 16 (0).  Same arithmetic in the same order: the
 * results are identical bit for bit (tests/test_gpu_parity.py test_eaw_tiled_levels_equal_plain_gathers). */
int  rs_eaw_set_tiled(rs_eaw* f, int tiled);
/* The arithmetic of a tap (waveletFilter's loop body, src/denoiser.cu:98-128).  0: every operation rounded separately in the reference's
 * order, as a host build of the reference without contraction computes it.  1: fused multiply-adds for the three squared distances, for
 * the exponent -(dc.dc / sigLumin + dn.dn / sigNormal + dp.dp / sigDepth) * log2(e) as one chain over coefficients -log2(e) / sigma, and
 * for sum += colour * w -- what a contracting compiler (nvcc's default) is free to produce; 36 vector instructions per tap for 50.  The
 * results agree to a few ulp (all sums are of non-negative terms); both stay inside the filter's stated rtol 1e-5 against the oracle.
 * DEFAULT 1 (a deviation from the reference's operation order that the parity contract states: the filters are compared within rtol,
 * never bit for bit); a caller that wants the reference's order sets 0. */
int  rs_eaw_set_fused(rs_eaw* f, int fused);
/* LeveledEAWFilter::filter (src/denoiser.cu:463-477): *devColorOut is in/out exactly like the
 * reference's `glm::vec3*& devColorOut` (it is swapped with the filter's internal buffer). */
int  rs_eaw_filter(rs_eaw* f, float** devColorOut, const float* devColorIn, const rs_gbuffer* g, const rs_camera* cam);
/* Row-strip form for framebuffer tiling: positions of rows [y0, y1) (EAWaveletFilter's cam.getPosition per tap, computed once),
 * then one wavelet level (src/denoiser.cu:64-134) on rows [y0, y1).  Level l reads rows up to 2 << l outside the strip from
 * devColorIn, the G-buffer and the positions; the caller exchanges those colour rows between the levels and owns the buffers.
 * 0 <= level <= 29 (a tap lies 2 << level pixels away, which must stay an int); rows are clamped to the frame. */
int  rs_eaw_positions_rows(rs_eaw* f, const rs_gbuffer* g, const rs_camera* cam, int y0, int y1);
int  rs_eaw_level_rows(rs_eaw* f, float* devColorOut, const float* devColorIn, const rs_gbuffer* g, int level, int y0, int y1);
/* ---- SVGF (src/denoiser.h:45-70) ---------------------------------------------------------- */
/* SpatioTemporalFilter::create / destroy (src/denoiser.cu:479-504); wavelet sigmas 4 / 128 / 1 as in the reference */
int  rs_svgf_create(int width, int height, int level, rs_svgf** f);
int  rs_svgf_destroy(rs_svgf* f);
/* SpatioTemporalFilter::level and waveletFilter.sig* (src/preview.cpp:278-286, src/denoiser.h:59); create() sets 4 / 128 / 1
 * (src/denoiser.cu:488).  As in the reference the filter always runs five levels. */
int  rs_svgf_set_params(rs_svgf* f, float sigLumin, float sigNormal, float sigDepth, int level);
int  rs_svgf_get_params(const rs_svgf* f, float* sigLumin, float* sigNormal, float* sigDepth, int* level);
/* 1 (default): the a-trous levels read their taps from an LDS tile -- with sigNormal 128 (the reference's default), a sigDepth that is a
 * power of two and any sigLumin; other sigmas gather from memory whatever this switch says.  0: plain gathers.  Same bits
 * (tests/test_gpu_denoise_edges.py, tests/test_gpu_parity.py test_svgf_tiled_levels_equal_plain_gathers). */
int  rs_svgf_set_tiled(rs_svgf* f, int tiled);
/* The arithmetic of a tap, as rs_eaw_set_fused: fused dot products and accumulation, one multiplication per exponent (the colour
 * weight's -log2(e) / denominator and the luminance staged once per pixel).  Acts with the reference's defaults sigNormal 128 and a
 * power-of-two sigDepth; other sigmas keep the separately rounded operations.  Stated tolerance against the oracle as before: rtol 3e-5.
 * DEFAULT 1, as rs_eaw_set_fused. */
int  rs_svgf_set_fused(rs_svgf* f, int fused);
/* SpatioTemporalFilter::filter (src/denoiser.cu:532-564): temporal accumulation (alpha .2), variance estimate, five
 * variance-guided a-trous levels.  *devColorOut is the reference's `glm::vec3*& devColorOut`: it is swapped with the
 * filter's buffers (the level-0 result becomes the history), so the caller continues with the pointer it gets back
 * and, as in the reference, buffers on both sides must come from hipMalloc: rs_svgf_destroy frees what the filter
 * holds at that time, the caller frees the pointer it holds. */
int  rs_svgf_filter(rs_svgf* f, float** devColorOut, const float* devColorIn, const rs_gbuffer* g, const rs_camera* cam);
int  rs_svgf_next_frame(rs_svgf* f);                                                  /* ::nextFrame (:566-568) */
/* Device pointers of the filter's state (devAccumColor / devAccumMoment / devVariance, src/denoiser.h:60-63). */
typedef struct rs_svgf_view {
    float* devAccumColor[2];
    float* devAccumMoment[2];
    float* devVariance;
    int    frameIdx;
    int    width, height;
} rs_svgf_view;
int  rs_svgf_get_view(const rs_svgf* f, rs_svgf_view* view);

int  rs_modulate_albedo(float* devImage, const rs_gbuffer* g);                        /* src/denoiser.cu:405-411 */
int  rs_add_image(float* devImage, const float* devIn, int width, int height);       /* :413-418 */
int  rs_add_image3(float* devOut, const float* devIn1, const float* devIn2, int width, int height); /* :420-425 */

#ifdef __cplusplus
}
#endif
#endif
