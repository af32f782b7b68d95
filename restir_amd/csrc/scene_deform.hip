// scene_deform.hip -- rigid parts, skinned meshes and morph targets (include/restir_hip.h; rs_deform.h), all of them: the rest pose,
// the kernels that write an edit's records from it (k_bake_parts, k_skin, k_morph, k_morph_skin), the definitions, the edits, the queries.  An edit is
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

// 16-byte pieces of a staged block into LDS, 16 bytes a lane and step; the caller's barrier follows
__device__ __forceinline__ void stage16(const void* from, void* to, int n16) {
    const uint4* src = reinterpret_cast<const uint4*>(from);
    uint4* dst = reinterpret_cast<uint4*>(to);
    for (int i = (int)threadIdx.x; i < n16; i += 256) dst[i] = src[i];
}

// rs_scene_set_morph_weights: the same staged edit, written from the morph's rest pose, its by-corner table and the weights.  One lane per
// output corner.  The block first copies the weights -- staged as whole 112-byte records, zero-padded, so that ceil(numTargets / 4) 16-byte
// pieces are there to read; at most 1 KB -- into LDS and meets at one barrier, which lanes past numCorners reach too: nothing returns
// before it.  A lane then reads its two offsets and its 12 + 12 bytes of rest corner and walks its entries with rs_bake.h's morph_corner
// -- the bits are rs_morph_corners' --: 16 bytes of target id and position delta, the weight from LDS, and the other 16 bytes only where
// the weight is not 0.  It writes 12 + 12 bytes; the lane of corner 0 also writes the primitive id.  Entry counts differ from lane to lane:
// a wave walks as long as its longest corner (accepted: DESIGN.md section 3).  The target ids were checked against numTargets by the
// definition and the device copy is never written again, so no read leaves the staged weights.  No hand-off between lanes.
__global__ void __launch_bounds__(256) k_morph(int numTargets, const float* __restrict__ staged, const int* __restrict__ morphPrimIds,
                                               const float* __restrict__ restVertices, const float* __restrict__ restNormals,
                                               const int* __restrict__ cornerFirst, const MorphEntry* __restrict__ entries,
                                               size_t numCorners, int* __restrict__ ids, float* __restrict__ vertices, float* __restrict__ normals) {
    __shared__ __attribute__((aligned(16))) float w[RS_MORPH_MAX_TARGETS];
    stage16(staged, w, (numTargets + 3) >> 2);
    __syncthreads();
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= numCorners) return;
    const BakedCorner o = morph_corner(entries, cornerFirst[c], cornerFirst[c + 1], w, ld3(restVertices + c * 3), ld3(restNormals + c * 3));
    st3(vertices + c * 3, o.position);
    st3(normals + c * 3, o.normal);
    const size_t tri = c / 3;
    if (c == tri * 3) ids[tri] = morphPrimIds[tri];
}

// rs_scene_set_skin_pose on a skin that has a morph: k_skin with morph_corner in front -- skin_corner(morph_corner(rest)) per corner, and
// nothing else.  The staged block is the numBones bone records, then the weight records; both go to LDS (28 KB + 1 KB) behind the one barrier.
__global__ void __launch_bounds__(256) k_morph_skin(int numBones, int numTargets, const BoneRec* __restrict__ bones, const int* __restrict__ skinPrimIds,
                                                    const float* __restrict__ restVertices, const float* __restrict__ restNormals,
                                                    const int4* __restrict__ boneIds, const float4* __restrict__ weights,
                                                    const int* __restrict__ cornerFirst, const MorphEntry* __restrict__ entries,
                                                    size_t numCorners, int* __restrict__ ids, float* __restrict__ vertices, float* __restrict__ normals) {
    __shared__ BoneRec palette[RS_SKIN_MAX_BONES];
    __shared__ __attribute__((aligned(16))) float mw[RS_MORPH_MAX_TARGETS];
    stage16(bones, palette, numBones * (int)(sizeof(BoneRec) / 16));
    stage16(bones + numBones, mw, (numTargets + 3) >> 2);
    __syncthreads();
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= numCorners) return;
    const BakedCorner r = morph_corner(entries, cornerFirst[c], cornerFirst[c + 1], mw, ld3(restVertices + c * 3), ld3(restNormals + c * 3));
    const int4 b4 = boneIds[c];
    const float4 w4 = weights[c];
    const int b[4] = { b4.x, b4.y, b4.z, b4.w };
    const float w[4] = { w4.x, w4.y, w4.z, w4.w };
    const BakedCorner o = skin_corner(palette, b, w, r.position, r.normal);
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

// ... of morph weights (owner: the rs_morph; dRecs: the weight records) and of a pose of a skin with a morph (owner: the rs_skin; dRecs: all
// numBones bone records, then the weight records)
int enqueue_morph(const rs_record_source& src, const void* dRecs, size_t m, int* dIds, float* dVertices, float* dNormals, hipStream_t st) {
    const rs_morph* mo = static_cast<const rs_morph*>(src.owner);
    const size_t corners = m * 3;
    if (mo->table.numTargets < 1 || mo->table.numTargets > RS_MORPH_MAX_TARGETS || mo->table.cornerFirst.size() != corners + 1)
        return rs_fail(RS_ERR_INTERNAL, "rs_scene_set_morph_weights: a table the kernel has no room for");
    hipLaunchKernelGGL(k_morph, dim3((unsigned)((corners + 255) / 256)), dim3(256), 0, st, mo->table.numTargets, static_cast<const float*>(dRecs), (const int*)mo->rest.dPrimIds,
                       (const float*)mo->rest.dVertices, (const float*)mo->rest.dNormals, (const int*)mo->table.dCornerFirst, (const MorphEntry*)mo->table.dEntries,
                       corners, dIds, dVertices, dNormals);
    return rs_check_hip(hipGetLastError(), "rs_scene_set_morph_weights: morph kernel");
}
int enqueue_morph_skin(const rs_record_source& src, const void* dRecs, size_t m, int* dIds, float* dVertices, float* dNormals, hipStream_t st) {
    const rs_skin* skin = static_cast<const rs_skin*>(src.owner);
    const rs_morph_table* t = skin->morph;
    const size_t corners = m * 3;
    if (skin->numBones < 1 || skin->numBones > RS_SKIN_MAX_BONES || !t || t->numTargets < 1 || t->numTargets > RS_MORPH_MAX_TARGETS || t->cornerFirst.size() != corners + 1)
        return rs_fail(RS_ERR_INTERNAL, "rs_scene_set_skin_pose: a palette or a table the kernel has no room for");
    hipLaunchKernelGGL(k_morph_skin, dim3((unsigned)((corners + 255) / 256)), dim3(256), 0, st, skin->numBones, t->numTargets, static_cast<const BoneRec*>(dRecs),
                       (const int*)skin->rest.dPrimIds, (const float*)skin->rest.dVertices, (const float*)skin->rest.dNormals,
                       reinterpret_cast<const int4*>(skin->dBoneIds), reinterpret_cast<const float4*>(skin->dWeights), (const int*)t->dCornerFirst,
                       (const MorphEntry*)t->dEntries, corners, dIds, dVertices, dNormals);
    return rs_check_hip(hipGetLastError(), "rs_scene_set_skin_pose: morph and skin kernel");
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

// The palette and the weights the call asks for (a bone or target named twice takes its last value, one not named keeps its own), the
// host's own evaluation of every listed triangle by them -- the targets, where the skin has a morph, and then the bones -- and then
// rs_scene_set_geometry's implementation with the records written on the device: by k_skin from the staged palette, or, where the skin has
// a morph, by k_morph_skin from the staged palette and weight records.
static int set_skin_pose(rs_scene* s, const char* name, int boneCount, const int* boneIds, const float* matrices16, int targetCount, const int* targetIds,
                         const float* weights) {
    if (!s) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "null scene");
    if (boneCount < 0 || (boneCount > 0 && (!boneIds || !matrices16))) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "count < 0 or null arrays");
    rs_skin* k = s->skin;
    if (!k) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "the scene has no skin (rs_scene_define_skin)");
    for (int i = 0; i < boneCount; i++)
        if (boneIds[i] < 0 || boneIds[i] >= k->numBones) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "a bone id out of range");
    rs_morph_table* t = k->morph;
    if (targetCount < 0 || (targetCount > 0 && (!targetIds || !weights))) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "targetCount < 0 or null arrays");
    if (targetCount > 0 && !t) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "the skin has no morph (rs_scene_define_skin_morph)");
    if (t) RS_TRY(t->ask(name, targetCount, targetIds, weights));
    if (boneCount == 0 && targetCount == 0) return 0;

    const size_t listed = k->rest.primIds.size(), bones = (size_t)k->numBones;
    k->recs.assign(k->palette.begin(), k->palette.end());
    for (int i = 0; i < boneCount; i++) bone_record(matrices16 + (size_t)i * 16, k->recs[(size_t)boneIds[i]]);
    k->vertices.resize(listed * 9); k->normals.resize(listed * 9);
    const float *restV = k->rest.vertices.data(), *restN = k->rest.normals.data();
    if (t) {
        k->recs.resize(bones + t->records());
        t->fill_records(k->recs.data() + bones);
        k->morphedVertices.resize(listed * 9); k->morphedNormals.resize(listed * 9);
        t->evaluate(t->asked.data(), restV, restN, k->morphedVertices.data(), k->morphedNormals.data());
        restV = k->morphedVertices.data(); restN = k->morphedNormals.data();
    }
    rs_skin_corners_host(k->recs.data(), listed * 3, restV, restN, k->boneIds.data(), k->weights.data(), k->vertices.data(), k->normals.data());
    const rs_record_source src{ k->recs.data(), (int)k->recs.size(), k, t ? enqueue_morph_skin : enqueue_skin };
    bool taken = false;
    const int e = rs_set_geometry(s, (int)listed, k->rest.primIds.data(), k->vertices.data(), k->normals.data(), true, name, &src, &taken);
    // Geometry, palette and weights stay one pose: they become the scene's where the scene took the edit, whatever the call returned
    // after that, and where a skin that lists no triangle had no edit to make and nothing was refused.
    if (taken || (listed == 0 && e == 0)) {
        k->recs.resize(bones);
        k->palette.swap(k->recs);
        if (t) t->weights.swap(t->asked);
    }
    return e;
}

extern "C" int rs_scene_set_bone_transforms(rs_scene* s, int count, const int* boneIds, const float* matrices16) {
    RS_SCOPE(s);
    return set_skin_pose(s, "rs_scene_set_bone_transforms", count, boneIds, matrices16, 0, nullptr, nullptr);
}

extern "C" int rs_scene_set_skin_pose(rs_scene* s, int boneCount, const int* boneIds, const float* matrices16, int targetCount, const int* targetIds,
                                      const float* weights) {
    RS_SCOPE(s);
    return set_skin_pose(s, "rs_scene_set_skin_pose", boneCount, boneIds, matrices16, targetCount, targetIds, weights);
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

// ---- morph targets ----
void rs_morph_free(rs_morph* m) { delete m; }

int rs_morph_table::check(const char* name, int targets, size_t numCorners, const int* targetFirst, const int* entryCorner, const float* deltaPositions,
                          const float* deltaNormals, bool finite) {
    if (targets < 0 || targets > RS_MORPH_MAX_TARGETS) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "numTargets < 0 or above RS_MORPH_MAX_TARGETS");
    if (targets == 0) return 0;
    if (!targetFirst) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "null target offsets");
    if (targetFirst[0] != 0) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "the first offset is not 0");
    for (int t = 0; t < targets; t++)
        if (targetFirst[t + 1] < targetFirst[t]) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "offsets that decrease");
    const size_t n = (size_t)targetFirst[targets];
    if (n > 0 && (!entryCorner || !deltaPositions)) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "null entry corners or position deltas");
    std::vector<int> lastTarget(numCorners, -1);
    for (int t = 0; t < targets; t++)
        for (size_t e = (size_t)targetFirst[t]; e < (size_t)targetFirst[t + 1]; e++) {
            const int c = entryCorner[e];
            if (c < 0 || (size_t)c >= numCorners) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "a corner index out of range");
            if (lastTarget[(size_t)c] == t) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "a (target, corner) pair listed twice");
            lastTarget[(size_t)c] = t;
        }
    if (finite)
        for (size_t i = 0; i < n * 3; i++)
            if (!std::isfinite(deltaPositions[i]) || (deltaNormals && !std::isfinite(deltaNormals[i]))) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "a delta that is not finite");
    return 0;
}

// A counting sort by corner that visits the targets in ascending order: every corner's entries come out sorted by target id
void rs_morph_table::build(int targets, size_t numCorners, const int* targetFirst, const int* entryCorner, const float* deltaPositions, const float* deltaNormals) {
    numTargets = targets;
    const size_t n = targets > 0 ? (size_t)targetFirst[targets] : 0;
    cornerFirst.assign(numCorners + 1, 0);
    for (size_t e = 0; e < n; e++) cornerFirst[(size_t)entryCorner[e] + 1]++;
    for (size_t c = 0; c < numCorners; c++) cornerFirst[c + 1] += cornerFirst[c];
    std::vector<int> next(cornerFirst.begin(), cornerFirst.end() - 1);
    entries.assign(n, MorphEntry{});
    for (int t = 0; t < targets; t++)
        for (size_t e = (size_t)targetFirst[t]; e < (size_t)targetFirst[t + 1]; e++) {
            MorphEntry& o = entries[(size_t)next[(size_t)entryCorner[e]]++];
            o.head.target = t;
            for (int k = 0; k < 3; k++) {
                o.head.dp[k] = deltaPositions[e * 3 + k];
                o.tail.dn[k] = deltaNormals ? deltaNormals[e * 3 + k] : 0.f;
            }
            o.tail.pad = 0;
        }
    weights.assign((size_t)targets, 0.f);
}

int rs_morph_table::upload_tables() {
    RS_TRY(upload(&dCornerFirst, cornerFirst));
    return upload(&dEntries, entries);
}

int rs_morph_table::ask(const char* name, int count, const int* targetIds, const float* w) {
    for (int i = 0; i < count; i++) {
        if (targetIds[i] < 0 || targetIds[i] >= numTargets) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "a target id out of range");
        if (!std::isfinite(w[i])) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "a weight that is not finite");
    }
    asked = weights;
    for (int i = 0; i < count; i++) asked[(size_t)targetIds[i]] = w[i];
    return 0;
}

void rs_morph_table::fill_records(BoneRec* recs) const {
    std::memset(recs, 0, records() * sizeof(BoneRec));
    std::memcpy(recs, asked.data(), asked.size() * sizeof(float));
}

void rs_morph_table::evaluate(const float* w, const float* vertsIn, const float* normalsIn, float* vertsOut, float* normalsOut) const {
    for (size_t c = 0; c + 1 < cornerFirst.size(); c++) {
        const BakedCorner o = morph_corner(entries.data(), cornerFirst[c], cornerFirst[c + 1], w, ld3(vertsIn + c * 3), ld3(normalsIn + c * 3));
        st3(vertsOut + c * 3, o.position);
        st3(normalsOut + c * 3, o.normal);
    }
}

extern "C" int rs_morph_corners(int numTargets, const int* targetFirst, const int* entryCorner, const float* deltaPositions, const float* deltaNormals,
                                const float* weights, size_t n, const float* vertsIn, const float* normalsIn, float* vertsOut, float* normalsOut) {
    const char* name = "rs_morph_corners";
    if (n > 0 && (!vertsIn || !normalsIn || !vertsOut || !normalsOut)) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "a null array with n > 0");
    if (numTargets > 0 && !weights) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "null weights");
    RS_TRY(rs_morph_table::check(name, numTargets, n, targetFirst, entryCorner, deltaPositions, deltaNormals, false));
    rs_morph_table t;
    t.build(numTargets, n, targetFirst, entryCorner, deltaPositions, deltaNormals);
    t.evaluate(weights, vertsIn, normalsIn, vertsOut, normalsOut);
    return 0;
}

extern "C" int rs_scene_define_morph(rs_scene* s, int numTargets, int numListed, const int* primIds, const float* restVertices, const float* restNormals,
                                     const int* targetFirst, const int* entryCorner, const float* deltaPositions, const float* deltaNormals) {
    RS_SCOPE(s);
    const char* name = "rs_scene_define_morph";
    if (!s) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "null scene");
    if (numTargets < 0 || numTargets > RS_MORPH_MAX_TARGETS) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "numTargets < 0 or above RS_MORPH_MAX_TARGETS");
    if (numListed < 0 || (numTargets == 0 && numListed > 0)) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "numListed < 0, or triangles without a target");
    RS_TRY(rs_rest_pose::check_pair(name, restVertices, restNormals));
    if (numListed > 0 && !primIds) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "null primitive ids");
    const size_t listed = (size_t)numListed;
    RS_TRY(rs_rest_pose::check_listed(s, name, listed, primIds, restVertices, restNormals));
    RS_TRY(rs_morph_table::check(name, numTargets, listed * 3, targetFirst, entryCorner, deltaPositions, deltaNormals, true));
    RS_TRY(refuse_while_capturing(name));
    if (numTargets == 0) return replace_definition<rs_morph>(s->morph, nullptr, 0);

    rs_morph* m = new rs_morph();
    m->table.build(numTargets, listed * 3, targetFirst, entryCorner, deltaPositions, deltaNormals);
    int e = m->rest.build(s, listed, primIds, restVertices, restNormals);
    if (!e) e = m->table.upload_tables();
    return replace_definition(s->morph, m, e);
}

extern "C" int rs_scene_define_skin_morph(rs_scene* s, int numTargets, const int* targetFirst, const int* entryCorner, const float* deltaPositions,
                                          const float* deltaNormals) {
    RS_SCOPE(s);
    const char* name = "rs_scene_define_skin_morph";
    if (!s) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "null scene");
    rs_skin* k = s->skin;
    if (!k) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "the scene has no skin (rs_scene_define_skin)");
    const size_t corners = k->rest.primIds.size() * 3;
    RS_TRY(rs_morph_table::check(name, numTargets, corners, targetFirst, entryCorner, deltaPositions, deltaNormals, true));
    RS_TRY(refuse_while_capturing(name));
    if (numTargets == 0) return replace_definition<rs_morph_table>(k->morph, nullptr, 0);

    rs_morph_table* t = new rs_morph_table();
    t->build(numTargets, corners, targetFirst, entryCorner, deltaPositions, deltaNormals);
    return replace_definition(k->morph, t, t->upload_tables());
}

// The weights the call asks for, the host's own morphing of every listed triangle by them, and then rs_scene_set_geometry's implementation
// with the records written on the device by k_morph from the staged weight records.
extern "C" int rs_scene_set_morph_weights(rs_scene* s, int count, const int* targetIds, const float* weights) {
    RS_SCOPE(s);
    const char* name = "rs_scene_set_morph_weights";
    if (!s) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "null scene");
    if (count < 0 || (count > 0 && (!targetIds || !weights))) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "count < 0 or null arrays");
    rs_morph* m = s->morph;
    if (!m) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "the scene has no morph (rs_scene_define_morph)");
    rs_morph_table& t = m->table;
    RS_TRY(t.ask(name, count, targetIds, weights));
    if (count == 0) return 0;

    const size_t listed = m->rest.primIds.size();
    m->recs.resize(t.records());
    t.fill_records(m->recs.data());
    m->vertices.resize(listed * 9); m->normals.resize(listed * 9);
    t.evaluate(t.asked.data(), m->rest.vertices.data(), m->rest.normals.data(), m->vertices.data(), m->normals.data());
    const rs_record_source src{ m->recs.data(), (int)m->recs.size(), m, enqueue_morph };
    bool taken = false;
    const int e = rs_set_geometry(s, (int)listed, m->rest.primIds.data(), m->vertices.data(), m->normals.data(), true, name, &src, &taken);
    // geometry and weights stay one pose, as a skin's palette does
    if (taken || (listed == 0 && e == 0)) t.weights.swap(t.asked);
    return e;
}

static const rs_morph_table* morph_table_of(const rs_scene* s, int which) { return which == 0 ? (s->morph ? &s->morph->table : nullptr) : (s->skin ? s->skin->morph : nullptr); }

extern "C" int rs_scene_morph_info(const rs_scene* s, int which, int* numTargets, int* numListedPrims, int* numEntries) {
    if (!s) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_morph_info: null scene");
    if (which != 0 && which != 1) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_morph_info: which is neither 0 (the scene's morph) nor 1 (the skin's)");
    const rs_morph_table* t = morph_table_of(s, which);
    if (numTargets) *numTargets = t ? t->numTargets : 0;
    if (numListedPrims) *numListedPrims = t ? (int)((t->cornerFirst.size() - 1) / 3) : 0;
    if (numEntries) *numEntries = t ? (int)t->entries.size() : 0;
    return 0;
}

extern "C" int rs_scene_download_morph(const rs_scene* s, int which, int* primIds, float* restVertices, float* restNormals, int* cornerFirst, void* entries) {
    RS_SCOPE(s);
    const char* name = "rs_scene_download_morph";
    if (!s) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "null scene");
    if (which != 0 && which != 1) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "which is neither 0 (the scene's morph) nor 1 (the skin's)");
    const rs_morph_table* t = morph_table_of(s, which);
    if (!t) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "no such morph defined (rs_scene_define_morph, rs_scene_define_skin_morph)");
    if (which == 1 && (primIds || restVertices || restNormals)) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "a skin's morph has no rest pose of its own (rs_scene_download_skin)");
    if (which == 0) RS_TRY(s->morph->rest.download(name, primIds, restVertices, restNormals));
    else { RS_TRY(refuse_while_capturing(name)); RS_TRY(rs_synchronize()); }
    if (cornerFirst) RS_HIP(hipMemcpy(cornerFirst, t->dCornerFirst, t->cornerFirst.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (entries && !t->entries.empty()) RS_HIP(hipMemcpy(entries, t->dEntries, t->entries.size() * sizeof(MorphEntry), hipMemcpyDeviceToHost));
    return 0;
}
