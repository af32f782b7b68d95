// scene_deform.hip -- rigid parts and skinned meshes (include/restir_hip.h; rs_deform.h), all of them: the rest pose,
// the kernels that write an edit's records from it (k_bake_parts, k_skin), the definitions, the edits, the queries.  An edit is
// rs_set_geometry's (scene_edits.hip) with an rs_record_source (rs_refit.h): the entry point stages its 112-byte records, names the kernel that
// expands them in front of the refit (scene_refit.hip) and hands over the host's own evaluation of the same triangles, by rs_bake.h like the kernel's.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rs_deform.h"

using namespace rs;

namespace {

// rs_scene_set_part_transforms: the staged edit of rs_scene_set_geometry -- ids | vertices | normals of m triangles -- written on the device
// from the parts' rest pose instead of copied from the host.  One lane per output corner: consecutive lanes read consecutive 12-byte rest
// vertices and normals of their part and write consecutive 12-byte results; the lane of corner 0 also writes the primitive id.  A lane finds
// its part by binary search for the last record whose outFirst is not beyond its triangle (outFirst is non-decreasing, recs[0].outFirst = 0,
// no record is empty).  A wave that lies inside one part reads the two matrices through the scalar cache.  The arithmetic is rs_bake.h's
// bake_corner and nothing else: the bits are rs_bake_matrix's.  No hand-off between lanes, nothing shared.
__device__ __forceinline__ void bake_store(const PartRec* rec, const float* __restrict__ v, const float* __restrict__ n, float* outV, float* outN) {
    const BakedCorner o = bake_corner(rec->m, rec->nm, ld3(v), ld3(n));
    st3(outV, o.position);
    st3(outN, o.normal);
}
__global__ void __launch_bounds__(256) k_bake_parts(int numRecs, const PartRec* __restrict__ recs, const int* __restrict__ partPrimIds,
                                                    const float* __restrict__ restVertices, const float* __restrict__ restNormals,
                                                    size_t numCorners, int* __restrict__ ids, float* __restrict__ vertices, float* __restrict__ normals) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= numCorners) return;
    const size_t tri = c / 3, corner = c - tri * 3;
    int lo = 0, hi = numRecs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((size_t)recs[mid].outFirst <= tri) lo = mid; else hi = mid - 1;
    }
    const size_t slot = (size_t)recs[lo].restFirst + (tri - (size_t)recs[lo].outFirst);
    const size_t src = (slot * 3 + corner) * 3;
    const int first = __builtin_amdgcn_readfirstlane(lo);
    if (__all(lo == first)) bake_store(recs + first, restVertices + src, restNormals + src, vertices + c * 3, normals + c * 3);
    else bake_store(recs + lo, restVertices + src, restNormals + src, vertices + c * 3, normals + c * 3);
    if (corner == 0) ids[tri] = partPrimIds[slot];
}

// rs_scene_set_bone_transforms: the same staged edit, written from the skin's rest pose and a palette of bone matrices.  One lane per output
// corner.  The block first copies the whole palette -- numBones records of 112 bytes = 7 x 16, staged 16-byte aligned behind the records
// this kernel writes -- into LDS, 16 bytes a lane and step, and meets at one barrier: lanes past numCorners take part in both, nothing
// returns before the barrier.  A lane then reads its four bone ids and four weights as one int4 and one float4 (16 bytes per corner at a
// hipMalloc'ed base), its 12 + 12 bytes of rest corner, evaluates rs_bake.h's skin_corner against the LDS palette -- the bits are
// rs_skin_corners' -- and writes 12 + 12 bytes; the lane of corner 0 also writes the primitive id.  Bone ids differ from lane to lane, so the
// palette reads conflict on LDS banks: accepted.  The ids were checked against numBones by rs_scene_define_skin and
// the device copy is never written again, so no read leaves the staged palette.  28 KB of LDS: five blocks a CU.
__global__ void __launch_bounds__(256) k_skin(int numBones, const BoneRec* __restrict__ bones, const int* __restrict__ skinPrimIds,
                                              const float* __restrict__ restVertices, const float* __restrict__ restNormals,
                                              const int4* __restrict__ boneIds, const float4* __restrict__ weights,
                                              size_t numCorners, int* __restrict__ ids, float* __restrict__ vertices, float* __restrict__ normals) {
    __shared__ BoneRec palette[RS_SKIN_MAX_BONES];
    {
        const uint4* src = reinterpret_cast<const uint4*>(bones);
        uint4* dst = reinterpret_cast<uint4*>(palette);
        const int n16 = numBones * (int)(sizeof(BoneRec) / 16);
        for (int i = (int)threadIdx.x; i < n16; i += 256) dst[i] = src[i];
    }
    __syncthreads();
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= numCorners) return;
    const int4 b4 = boneIds[c];
    const float4 w4 = weights[c];
    const int b[4] = { b4.x, b4.y, b4.z, b4.w };
    const float w[4] = { w4.x, w4.y, w4.z, w4.w };
    const BakedCorner o = skin_corner(palette, b, w, ld3(restVertices + c * 3), ld3(restNormals + c * 3));
    st3(vertices + c * 3, o.position);
    st3(normals + c * 3, o.normal);
    const size_t tri = c / 3;
    if (c == tri * 3) ids[tri] = skinPrimIds[tri];
}

// rs_record_source::enqueue of a transform (owner: the rs_parts) and of a pose (owner: the rs_skin; dRecs: all numBones records); m > 0
int enqueue_bake(const rs_record_source& src, const void* dRecs, size_t m, int* dIds, float* dVertices, float* dNormals, hipStream_t st) {
    const rs_rest_pose& rest = static_cast<const rs_parts*>(src.owner)->rest;
    const size_t corners = m * 3;
    hipLaunchKernelGGL(k_bake_parts, dim3((unsigned)((corners + 255) / 256)), dim3(256), 0, st, src.numRecs, static_cast<const PartRec*>(dRecs), (const int*)rest.dPrimIds,
                       (const float*)rest.dVertices, (const float*)rest.dNormals, corners, dIds, dVertices, dNormals);
    return rs_check_hip(hipGetLastError(), "rs_scene_set_part_transforms: bake kernel");
}
int enqueue_skin(const rs_record_source& src, const void* dRecs, size_t m, int* dIds, float* dVertices, float* dNormals, hipStream_t st) {
    const rs_skin* skin = static_cast<const rs_skin*>(src.owner);
    const size_t corners = m * 3;
    if (skin->numBones < 1 || skin->numBones > RS_SKIN_MAX_BONES) return rs_fail(RS_ERR_INTERNAL, "rs_scene_set_bone_transforms: a palette the kernel has no room for");
    hipLaunchKernelGGL(k_skin, dim3((unsigned)((corners + 255) / 256)), dim3(256), 0, st, skin->numBones, static_cast<const BoneRec*>(dRecs), (const int*)skin->rest.dPrimIds,
                       (const float*)skin->rest.dVertices, (const float*)skin->rest.dNormals, reinterpret_cast<const int4*>(skin->dBoneIds),
                       reinterpret_cast<const float4*>(skin->dWeights), corners, dIds, dVertices, dNormals);
    return rs_check_hip(hipGetLastError(), "rs_scene_set_bone_transforms: skin kernel");
}

// A definition is replaced (fresh), or removed (fresh null), behind a wait for the device -- rs_synchronize, as the first edit of a scene
// waits once: an edit enqueued earlier reads the tables that are about to be freed, a later one finds the new.  e: what building `fresh`
// returned; on any failure the definition stays what it was.  Nothing of the scene's geometry changes.
template <class T> int replace_definition(T*& held, T* fresh, int e) {
    if (!e && held) e = rs_synchronize();
    if (e) { delete fresh; return e; }
    delete held;
    held = fresh;
    return 0;
}

// rs_skin_corners' and rs_scene_set_bone_transforms' palette: one record per matrix, the normal matrix computed once per matrix
void bone_record(const float* matrix16, BoneRec& rec) {
    std::memcpy(rec.m, matrix16, 16 * sizeof(float));
    rs_bake_normal_matrix(rec.m, rec.nm);
    rec.pad[0] = rec.pad[1] = rec.pad[2] = 0;
}

}  // namespace

// ---- the rest pose (rs_deform.h) ----
int rs_rest_pose::check_listed(const rs_scene* s, const char* name, size_t listed, const int* ids, const float* restVertices, const float* restNormals) {
    std::vector<char> seen((size_t)s->numPrims, 0);
    for (size_t i = 0; i < listed; i++) {
        const int p = ids[i];
        if (p < 0 || p >= s->numPrims) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "a primitive id out of range");
        if (seen[(size_t)p]) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "a primitive listed twice");
        seen[(size_t)p] = 1;
    }
    if (restVertices)
        for (size_t i = 0; i < listed * 9; i++)
            if (!std::isfinite(restVertices[i]) || !std::isfinite(restNormals[i])) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "a rest value that is not finite");
    return 0;
}

int rs_rest_pose::build(const rs_scene* s, size_t listed, const int* ids, const float* restVertices, const float* restNormals) {
    primIds.assign(ids, ids + listed);
    vertices.resize(listed * 9); normals.resize(listed * 9);
    for (size_t i = 0; i < listed; i++) {
        std::memcpy(&vertices[i * 9], restVertices ? restVertices + i * 9 : &s->hVertices[(size_t)ids[i] * 9], 9 * sizeof(float));
        std::memcpy(&normals[i * 9], restNormals ? restNormals + i * 9 : &s->hNormals[(size_t)ids[i] * 9], 9 * sizeof(float));
    }
    RS_TRY(upload(&dPrimIds, primIds));
    RS_TRY(upload(&dVertices, vertices));
    return upload(&dNormals, normals);
}

int rs_rest_pose::download(const char* name, int* ids, float* restVertices, float* restNormals) const {
    RS_TRY(refuse_while_capturing(name));
    RS_TRY(rs_synchronize());
    const size_t n = primIds.size();
    if (n && ids) RS_HIP(hipMemcpy(ids, dPrimIds, n * sizeof(int), hipMemcpyDeviceToHost));
    if (n && restVertices) RS_HIP(hipMemcpy(restVertices, dVertices, n * 9 * sizeof(float), hipMemcpyDeviceToHost));
    if (n && restNormals) RS_HIP(hipMemcpy(restNormals, dNormals, n * 9 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// ---- rigid parts ----
void rs_parts_free(rs_parts* p) { delete p; }
size_t rs_parts::build_records(int count, const int* partIds, const float* matrices16) {
    if (++stamp == 0u) { std::fill(recStamp.begin(), recStamp.end(), 0u); stamp = 1u; }
    recs.clear();
    for (int i = 0; i < count; i++) {
        const size_t part = (size_t)partIds[i];
        const int from = first[part], n = first[part + 1] - from;
        if (n == 0) continue;
        if (recStamp[part] != stamp) {
            recStamp[part] = stamp;
            recOf[part] = (int)recs.size();
            PartRec rec{};
            rec.restFirst = from; rec.count = n;
            recs.push_back(rec);
        }
        std::memcpy(recs[(size_t)recOf[part]].m, matrices16 + (size_t)i * 16, 16 * sizeof(float));
    }
    size_t m = 0;
    for (PartRec& rec : recs) { rec.outFirst = (int)m; m += (size_t)rec.count; }
    ids.resize(m); vertices.resize(m * 9); normals.resize(m * 9);
    for (PartRec& rec : recs) {
        rs_bake_normal_matrix(rec.m, rec.nm);
        const size_t in = (size_t)rec.restFirst, out = (size_t)rec.outFirst;
        std::memcpy(&ids[out], &rest.primIds[in], (size_t)rec.count * sizeof(int));
        rs_bake_corners(rec.m, rec.nm, (size_t)rec.count * 3, &rest.vertices[in * 9], &rest.normals[in * 9], &vertices[out * 9], &normals[out * 9]);
    }
    return m;
}

extern "C" int rs_scene_define_parts(rs_scene* s, int numParts, const int* partFirst, const int* primIds, const float* restVertices, const float* restNormals) {
    RS_SCOPE(s);
    const char* name = "rs_scene_define_parts";
    if (!s) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "null scene");
    if (numParts < 0 || (numParts > 0 && !partFirst)) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "numParts < 0 or null offsets");
    RS_TRY(rs_rest_pose::check_pair(name, restVertices, restNormals));
    if (numParts > 0 && partFirst[0] != 0) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "the first offset is not 0");
    for (int i = 0; i < numParts; i++)
        if (partFirst[i + 1] < partFirst[i]) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "offsets that decrease");
    const size_t listed = numParts > 0 ? (size_t)partFirst[numParts] : 0;
    if (listed > 0 && !primIds) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "null primitive ids");
    RS_TRY(rs_rest_pose::check_listed(s, name, listed, primIds, restVertices, restNormals));
    RS_TRY(refuse_while_capturing(name));
    if (numParts == 0) return replace_definition<rs_parts>(s->parts, nullptr, 0);

    rs_parts* p = new rs_parts();
    p->first.assign(partFirst, partFirst + numParts + 1);
    p->recOf.assign((size_t)numParts, 0); p->recStamp.assign((size_t)numParts, 0u);
    return replace_definition(s->parts, p, p->rest.build(s, listed, primIds, restVertices, restNormals));
}

// Check, build the records and the host's own baking, and then rs_scene_set_geometry's implementation with the records written on the device.
extern "C" int rs_scene_set_part_transforms(rs_scene* s, int count, const int* partIds, const float* matrices16) {
    RS_SCOPE(s);
    const char* name = "rs_scene_set_part_transforms";
    if (!s) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "null scene");
    if (count < 0 || (count > 0 && (!partIds || !matrices16))) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "count < 0 or null arrays");
    rs_parts* p = s->parts;
    if (!p) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "the scene has no parts (rs_scene_define_parts)");
    const int numParts = (int)p->first.size() - 1;
    for (int i = 0; i < count; i++)
        if (partIds[i] < 0 || partIds[i] >= numParts) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "a part id out of range");

    const size_t m = p->build_records(count, partIds, matrices16);
    const rs_record_source src{ p->recs.data(), (int)p->recs.size(), p, enqueue_bake };
    return rs_set_geometry(s, (int)m, p->ids.data(), p->vertices.data(), p->normals.data(), true, name, &src);
}

extern "C" int rs_scene_parts_info(const rs_scene* s, int* numParts, int* numListedPrims) {
    if (!s) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_parts_info: null scene");
    if (numParts) *numParts = s->parts ? (int)s->parts->first.size() - 1 : 0;
    if (numListedPrims) *numListedPrims = s->parts ? (int)s->parts->rest.primIds.size() : 0;
    return 0;
}

extern "C" int rs_scene_download_part_rest(const rs_scene* s, int* primIds, float* restVertices, float* restNormals) {
    RS_SCOPE(s);
    if (!s) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_download_part_rest: null scene");
    if (!s->parts) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_download_part_rest: the scene has no parts (rs_scene_define_parts)");
    return s->parts->rest.download("rs_scene_download_part_rest", primIds, restVertices, restNormals);
}

// ---- skinned meshes ----
void rs_skin_free(rs_skin* k) { delete k; }
extern "C" int rs_skin_corners(int numBones, const float* matrices16, size_t n, const float* vertsIn, const float* normalsIn, const int* boneIds4,
                               const float* weights4, float* vertsOut, float* normalsOut) {
    if (numBones < 1 || !matrices16) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_skin_corners: numBones < 1 or null matrices");
    if (n > 0 && (!vertsIn || !normalsIn || !boneIds4 || !weights4 || !vertsOut || !normalsOut)) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_skin_corners: a null array with n > 0");
    for (size_t i = 0; i < n * 4; i++)
        if (boneIds4[i] < 0 || boneIds4[i] >= numBones) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_skin_corners: a bone id out of range");
    std::vector<BoneRec> palette((size_t)numBones);
    for (int b = 0; b < numBones; b++) bone_record(matrices16 + (size_t)b * 16, palette[(size_t)b]);
    rs_skin_corners_host(palette.data(), n, vertsIn, normalsIn, boneIds4, weights4, vertsOut, normalsOut);
    return 0;
}

extern "C" int rs_scene_define_skin(rs_scene* s, int numBones, int numListed, const int* primIds, const float* restVertices, const float* restNormals,
                                    const int* boneIds, const float* weights) {
    RS_SCOPE(s);
    const char* name = "rs_scene_define_skin";
    if (!s) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "null scene");
    if (numBones < 0 || numBones > RS_SKIN_MAX_BONES) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "numBones < 0 or above RS_SKIN_MAX_BONES");
    if (numListed < 0 || (numBones == 0 && numListed > 0)) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "numListed < 0, or triangles without a bone");
    RS_TRY(rs_rest_pose::check_pair(name, restVertices, restNormals));
    if (numListed > 0 && (!primIds || !boneIds || !weights)) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "null primitive ids, bone ids or weights");
    const size_t listed = (size_t)numListed;
    RS_TRY(rs_rest_pose::check_listed(s, name, listed, primIds, restVertices, restNormals));
    for (size_t c = 0; c < listed * 3; c++) {
        bool any = false;
        for (size_t k = c * 4; k < c * 4 + 4; k++) {
            if (boneIds[k] < 0 || boneIds[k] >= numBones) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "a bone id out of range");
            if (!std::isfinite(weights[k])) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "a weight that is not finite");
            if (weights[k] < 0.f) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "a negative weight");
            any = any || weights[k] != 0.f;
        }
        if (!any) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "a corner whose four weights are all 0");
    }
    RS_TRY(refuse_while_capturing(name));
    if (numBones == 0) return replace_definition<rs_skin>(s->skin, nullptr, 0);

    rs_skin* k = new rs_skin();
    k->numBones = numBones;
    k->boneIds.assign(boneIds, boneIds + listed * 12); k->weights.assign(weights, weights + listed * 12);
    const float identity[16] = { 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f };
    k->palette.resize((size_t)numBones);
    for (BoneRec& rec : k->palette) bone_record(identity, rec);
    int e = k->rest.build(s, listed, primIds, restVertices, restNormals);
    if (!e) e = upload(&k->dBoneIds, k->boneIds);
    if (!e) e = upload(&k->dWeights, k->weights);
    return replace_definition(s->skin, k, e);
}

// The palette the call asks for (a bone named twice takes its last matrix, a bone not named keeps its own), the host's own skinning of every
// listed triangle by it, and then rs_scene_set_geometry's implementation with the records written on the device.
extern "C" int rs_scene_set_bone_transforms(rs_scene* s, int count, const int* boneIds, const float* matrices16) {
    RS_SCOPE(s);
    const char* name = "rs_scene_set_bone_transforms";
    if (!s) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "null scene");
    if (count < 0 || (count > 0 && (!boneIds || !matrices16))) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "count < 0 or null arrays");
    rs_skin* k = s->skin;
    if (!k) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "the scene has no skin (rs_scene_define_skin)");
    for (int i = 0; i < count; i++)
        if (boneIds[i] < 0 || boneIds[i] >= k->numBones) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "a bone id out of range");
    if (count == 0) return 0;

    k->recs = k->palette;
    for (int i = 0; i < count; i++) bone_record(matrices16 + (size_t)i * 16, k->recs[(size_t)boneIds[i]]);
    const size_t listed = k->rest.primIds.size();
    k->vertices.resize(listed * 9); k->normals.resize(listed * 9);
    rs_skin_corners_host(k->recs.data(), listed * 3, k->rest.vertices.data(), k->rest.normals.data(), k->boneIds.data(), k->weights.data(),
                         k->vertices.data(), k->normals.data());
    const rs_record_source src{ k->recs.data(), k->numBones, k, enqueue_skin };
    bool taken = false;
    const int e = rs_set_geometry(s, (int)listed, k->rest.primIds.data(), k->vertices.data(), k->normals.data(), true, name, &src, &taken);
    // Geometry and palette stay one pose: the palette becomes the scene's where the scene took the edit, whatever the call returned after
    // that, and where a skin that lists no triangle had no edit to make and nothing was refused.
    if (taken || (listed == 0 && e == 0)) k->palette.swap(k->recs);
    return e;
}

extern "C" int rs_scene_skin_info(const rs_scene* s, int* numBones, int* numListedPrims) {
    if (!s) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_skin_info: null scene");
    if (numBones) *numBones = s->skin ? s->skin->numBones : 0;
    if (numListedPrims) *numListedPrims = s->skin ? (int)s->skin->rest.primIds.size() : 0;
    return 0;
}

extern "C" int rs_scene_download_skin(const rs_scene* s, int* primIds, float* restVertices, float* restNormals, int* boneIds, float* weights) {
    RS_SCOPE(s);
    if (!s) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_download_skin: null scene");
    const rs_skin* k = s->skin;
    if (!k) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_download_skin: the scene has no skin (rs_scene_define_skin)");
    RS_TRY(k->rest.download("rs_scene_download_skin", primIds, restVertices, restNormals));
    const size_t n = k->rest.primIds.size();
    if (n && boneIds) RS_HIP(hipMemcpy(boneIds, k->dBoneIds, n * 12 * sizeof(int), hipMemcpyDeviceToHost));
    if (n && weights) RS_HIP(hipMemcpy(weights, k->dWeights, n * 12 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
