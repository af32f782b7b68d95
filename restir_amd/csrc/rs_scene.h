// rs_scene.h -- device-resident scene (the DevScene of src/scene.h:64-481, re-laid-out for CDNA4): its records, the camera and the
// light-sample declaration.  The box and triangle tests are in rs_intersect.h, the BVH walks and the trace_* services in rs_walk.h.
//
// HBM layout (all arrays hipMalloc'ed once by rs_scene_create, read-only afterwards):
//   nodesAll   BvhNode[6*bvhSize+1] 32 B: MTBVHNode (src/bvh.h:163-171) fused with the AABB it points to,
//                                 so one traversal step is ONE 32-byte fetch (two dwordx4 from one
//                                 sector) instead of the reference's two dependent loads
//                                 (12-B node -> 24-B box, src/scene.h:254).  6 threaded orders.
//   tris       TriRec[numPrims]   48 B: v0, e01 = v1-v0, e02 = v2-v0 (the first two lines of
//                                 intersectTriangle, src/intersections.h:20-21, hoisted to scene build;
//                                 IEEE subtraction, so bit-identical) -> three dwordx4 per leaf test.
//   vertices / normals            float[9] per triangle, as given (attribute fetch of the final hit only)
//   prevVertices                  float[9] per triangle: the vertices at the last rs_scene_advance_motion (allocated when motion tracking is
//                                 switched on, written by that call alone; null otherwise)
//   materialIds, materials        as given (44-B Material records)
//   lights     LightRec[numLights] 64 B: v0,v1,v2, geometric normal, unit radiance and the
//                                 per-light constant pdfArea = lum(Le)/(area*2*pi) * sumLightPowerInv
//                                 (src/scene.h:411,419-424: per-candidate in the reference, per-light here)
//   alias      AliasRec[numLights] 8 B: BinomialDistrib {prob, failId} (src/sampler.h:63-67)
//   occNodes   uint4[occCount]    16 B: the shadow-ray tree (occlusion_bvh.cpp): box on a 16-bit grid over the
//                                 scene bounds {lo.x|lo.y<<16, lo.z|hi.x<<16, hi.y|hi.z<<16}, w = miss link of an
//                                 inner node (as a byte offset: index * 16) or ~(firstTriangle*8+count) of a leaf.  Null when the fast path is off.
//   occChain   BvhNode[bvhSize]   32 B: the reference's boxes by ORIGINAL node id with primId = next = parent id
//                                 (-1 at the root): the path a candidate occluder is verified against
//   occTris    TriRec[numPrims]   the same pre-differenced triangles in the shadow tree's leaf order,
//                                 pad0 = bit pattern of the triangle's reference leaf node id
#pragma once

#include "rs_math.h"
#include "rs_exact.h"
#include "../../include/restir_hip.h"

namespace rs {

// field order: the packet walk reads a record through the scalar cache and feeds SGPR pairs to packed FP32 instructions, which
// want (min.x, min.y), (min.z, max.z), (max.x, max.y) in aligned pairs; node_unpack() restores the (min | prim), (max | next)
// view the per-lane walks are written with (register renaming, no instructions)
struct __attribute__((aligned(16))) BvhNode {
    float bminx, bminy, bminz, bmaxz;
    float bmaxx, bmaxy; int primId; int next;
};
struct __attribute__((aligned(16))) TriRec {
    float v0x, v0y, v0z, pad0;
    float e1x, e1y, e1z, pad1;
    float e2x, e2y, e2z, pad2;
};
struct __attribute__((aligned(16))) LightRec {
    float v0x, v0y, v0z, nx;
    float v1x, v1y, v1z, ny;
    float v2x, v2y, v2z, nz;
    float Lx, Ly, Lz, pdfArea;
};
// The pre-differenced triangle of nine floats: the one place the subtraction is written, for the host builders and the device refit alike
struct TriEdges { f3 v0, e1, e2; };
RS_HD TriEdges tri_edges(const float* t) {
    const f3 v0 = ld3(t), v1 = ld3(t + 3), v2 = ld3(t + 6);
    return TriEdges{ v0, v1 - v0, v2 - v0 };
}
// ... as a record; the pads are a table's own (bit patterns of ints, see the layout above)
inline TriRec tri_rec(const float* t, int pad0 = 0, int pad1 = 0) {
    const TriEdges d = tri_edges(t);
    float b0, b1;
    __builtin_memcpy(&b0, &pad0, 4); __builtin_memcpy(&b1, &pad1, 4);
    return TriRec{ d.v0.x, d.v0.y, d.v0.z, b0, d.e1.x, d.e1.y, d.e1.z, b1, d.e2.x, d.e2.y, d.e2.z, 0.f };
}
struct AliasRec { float prob; int failId; };
struct TexRec { const float* data; int width, height; };       // DevTextureObj (src/image.h:76-97): packed float[3] texels

struct DevScene {
    const BvhNode* nodesAll;      // 6 * bvhSize records (+1 padding record): order k starts at k * bvhSize
    const TriRec*  tris;
    const float*   vertices;
    const float*   normals;
    const float*   texcoords;     // 6 floats / triangle; null unless the scene has texture maps
    const int*     materialIds;
    const rs_material* materials;
    const LightRec* lights;
    const AliasRec* alias;
    const TexRec*  textures;      // null unless the scene has texture maps or an environment map
    const AliasRec* envAlias;     // envMapSampler (src/scene.h:364-376), envLen = width*height of the map, 0 = none
    int envTex, envLen;           // envMap = textures + envTex (src/scene.cpp:495-498), -1 = none
    float sumLightPowerInv;       // src/scene.cpp:489
    const uint4*   occNodes;
    const BvhNode* occChain;
    const TriRec*  occTris;
    f3 occBase, occScale;         // grid plane q on axis c = occBase.c + q * occScale.c
    f3 occRootLo, occRootHi;      // the reference's root box
    bool occNested;               // every reference box lies inside its parent's (enables the leaf shortcut)
    bool axisCull;                // boxes contain their children and triangles, and no triangle is too large for skip_far_on_axis (scene.hip far_skip_allowed):
                                  // enables that cull and, with linksNested, the packet walk's fast form (which needs the hierarchy alone and shares the flag)
    bool linksNested;             // in every threaded order the miss links nest: c in (a, link(a)) => link(c) <= link(a)
    int occCount;
    // the emissive triangles alone, as a tree of the shadow tree's kind (scene.hip build_emissive_side; may_hit_emissive_wave):
    // emiState 0 = not built, or switched off by an edit (every ray may hit one), 1 = built, emiCount nodes (0: the scene has no emissive
    // triangle); emiBase / emiScale: its own grid, which rs_scene_set_geometry lays anew when emitters move
    const uint4*   emiNodes;
    const TriRec*  emiTris;
    f3 emiBase, emiScale;
    int emiCount, emiState;
    // closest hit of incoherent rays: six trees in the reference's six visiting orders (occlusion_bvh.cpp rs_build_ordered_bvh), 16-byte
    // records on the shadow tree's grid, order k at byte offset k * ordStride, its end record at (k + 1) * ordStride - 16;
    // ordTris: per axis numPrims triangles in the even order's sequence (pad0 = reference leaf node, pad1 = primitive id).  Null = off.
    const uint4*   ordNodes;
    const TriRec*  ordTris;
    unsigned ordStride;
    unsigned long long* walkStats;   // null unless built with -DRS_WALK_STATS (tools/walk_stats.py)
    const unsigned char* occDepth;   // depth of every occNodes record (-DRS_WALK_STATS builds only)
    int bvhSize;
    int numPrims;
    int numLights;
    int numMaterials;
    // DevScene::sampleSequence (src/scene.h:480, src/scene.cpp:500-506): the Sobol table, sampleCount x kSobolSampleDim uint32 followed
    // by a guard of kSobolGuard zeros; null = the default thrust engine (SAMPLER_USE_SOBOL false).  rs_scene_set_sample_sequence.
    const uint32_t* sampleSeq;
    int sampleCount;
    // The scene's pose at the last rs_scene_advance_motion: 9 floats per triangle, laid out like `vertices`; null = motion tracking off
    // (rs_scene_set_motion_tracking).  Read by the MOTION form of gbuffer_store alone.  Last, so that every other field keeps its offset.
    const float* prevVertices;
};
constexpr int kSobolGuard = 4096;

struct Ray { f3 o, d; };

struct Hit {
    int primId;
    int matId;
    f3  pos;
    f3  norm;
    float bx, by;     // barycentrics of the hit (for the texture coordinates of textured scenes)
};

// ---- camera (src/sceneStructs.h:22-86) ---------------------------------------------------------
// The reference evaluates tan(radians(fov.y)) per thread; it is a per-frame constant, so the host
// evaluates the same expression once (same libm as any host evaluation) and passes it in.
struct CamParams {
    f3 position, right, up, view;
    f3 inv0, inv1, inv2;         // columns of rotationMatInv
    float aspect, tanFovY, focalDist, lensRadius;
    float pixelSizeX, pixelSizeY;
    int width, height;
};

// Camera::sample (sceneStructs.h:69-86); r = first two components of the 4-D jitter
RS_HD Ray camera_sample(const CamParams& c, int x, int y, float rx, float ry) {
    float scrx = (float)x * c.pixelSizeX, scry = (float)y * c.pixelSizeY;
    float ruvx = scrx + c.pixelSizeX * rx, ruvy = scry + c.pixelSizeY * ry;
    ruvx = 1.f - ruvx * 2.f;
    ruvy = 1.f - ruvy * 2.f;
    f3 pLens = mk3(0.f * c.lensRadius, 0.f * c.lensRadius, 0.f);
    f3 pFocus = mk3(ruvx * c.aspect * c.tanFovY, ruvy * 1.f * c.tanFovY, 1.f) * c.focalDist;
    f3 dir = pFocus - pLens;
    Ray r;
    r.d = normalize(mul_cols(c.right, c.up, c.view, dir));
    r.o = c.position + c.right * pLens.x + c.up * pLens.y;
    return r;
}

// pixel-centre ray of renderGBuffer (gbuffer.cu:11-24)
RS_HD Ray camera_center_ray(const CamParams& c, int x, int y) {
    float scrx = (float)x * c.pixelSizeX, scry = (float)y * c.pixelSizeY;
    float ruvx = scrx + c.pixelSizeX * .5f, ruvy = scry + c.pixelSizeY * .5f;
    f3 pLens = splat(0.f);
    f3 pFocus = mk3((1.f - ruvx * 2.f) * c.aspect * c.tanFovY, (1.f - ruvy * 2.f) * 1.f * c.tanFovY, 1.f) * c.focalDist;
    f3 dir = pFocus - pLens;
    Ray r;
    r.d = normalize(mul_cols(c.right, c.up, c.view, dir));
    r.o = c.position + c.right * pLens.x + c.up * pLens.y;
    return r;
}

// Camera::getPosition (sceneStructs.h:48-64)
RS_HD f3 camera_get_position(const CamParams& c, int x, int y, float dist) {
    float scrx = (float)x * c.pixelSizeX, scry = (float)y * c.pixelSizeY;
    float ruvx = scrx + c.pixelSizeX * .5f, ruvy = scry + c.pixelSizeY * .5f;
    ruvx = 1.f - ruvx * 2.f;
    ruvy = 1.f - ruvy * 2.f;
    f3 pLens = mk3(0.f * c.lensRadius, 0.f * c.lensRadius, 0.f);
    f3 pFocus = mk3(ruvx * c.aspect * c.tanFovY, ruvy * 1.f * c.tanFovY, 1.f) * c.focalDist;
    f3 dir = normalize(mul_cols(c.right, c.up, c.view, pFocus - pLens));
    f3 ori = c.position + c.right * pLens.x + c.up * pLens.y;
    return ori + dir * dist;
}

// Camera::getRasterCoord (sceneStructs.h:23-46)
RS_HD void camera_raster_coord(const CamParams& c, f3 pos, int& ox, int& oy) {
    f3 dir = normalize(pos - c.position);
    float d = 1.f / dot(dir, c.view);
    f3 p = mul_cols(c.inv0, c.inv1, c.inv2, dir * d);
    p = p / mk3(c.aspect * c.tanFovY, 1.f * c.tanFovY, 1.f);
    float ndcx = -p.x, ndcy = -p.y;
    ndcx = ndcx * .5f + .5f;
    ndcy = ndcy * .5f + .5f;
    ox = f2i((float)c.width * ndcx);
    oy = f2i((float)c.height * ndcy);
}

// ---- light sampling (src/scene.h:394-459, src/sampler.h:203-207, src/mathUtil.h:94-100,182-185) --
struct LightSample { float pdf; f3 Li, wi; float dist; f3 point; int id; float bu, bv; };     // bu, bv: the barycentric pair of sampleTriangleUniform

#if defined(__HIPCC__)
// sampleDirectLightNoVisibility; `lights`/`alias` may point to global memory or to an LDS copy.
// Bit-exact shortcuts: dot(x-y, x-y) == dot(y-x, y-x) and normalize(x-y) == -normalize(y-x), so
// the pdf conversion (mathUtil.h:182-185) reuses wi and dist instead of re-deriving them.
template <bool ENV, typename AliasPtr, typename LightPtr>
__device__ __forceinline__ LightSample sample_light_nv(const DevScene& s, AliasPtr alias, LightPtr lights, int numLights, f3 pos, f4 r);
#endif

}  // namespace rs

#include "rs_surface.h"

