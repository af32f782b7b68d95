// rs_deform.h -- deformers: geometry edits whose records a kernel writes on the device from a rest pose the scene keeps there.  Rigid parts
// (one matrix per part) and skinned meshes (a blend of bone matrices per corner); entry points, kernels and the host's side of both:
// scene_deform.hip.  The edit itself is rs_set_geometry's (rs_refit.h), which knows of a deformer what rs_record_source says.
#pragma once

#include "rs_refit.h"
#include "rs_bake.h"

// Listed primitives and their rest corners, on the host and on the device: what parts and skins alike keep of a definition.  The device
// copies are read by the deformer's one kernel alone and never written after the definition.  (The library's own: no dynamic symbol.)
struct __attribute__((visibility("hidden"))) rs_rest_pose {
    std::vector<int> primIds;                           // the listed primitives; no primitive twice
    std::vector<float> vertices, normals;               // 9 floats per listed primitive
    int* dPrimIds = nullptr;
    float *dVertices = nullptr, *dNormals = nullptr;
    ~rs_rest_pose() { rs_dev_free(dPrimIds); rs_dev_free(dVertices); rs_dev_free(dNormals); }

    // The refusals two definitions share, under the entry point's `name`.  Two calls, since each entry point keeps the order of its checks
    // and has its own between them: vertices and normals both or neither; every id in range and listed once, the caller's rest values finite.
    static int check_pair(const char* name, const float* restVertices, const float* restNormals) {
        return (restVertices == nullptr) == (restNormals == nullptr) ? 0 : fail_named(RS_ERR_INVALID_ARGUMENT, name, "rest vertices without rest normals, or the reverse");
    }
    static int check_listed(const rs_scene* s, const char* name, size_t listed, const int* ids, const float* restVertices, const float* restNormals);
    // the caller's arrays, or (both null) the scene's own pose of the listed primitives; then the three uploads
    int build(const rs_scene* s, size_t listed, const int* ids, const float* restVertices, const float* restNormals);
    // the device copies, behind a wait for the device (refused while the library stream is captured); a null array is skipped
    int download(const char* name, int* ids, float* restVertices, float* restNormals) const;
};

// The rigid parts of a scene (rs_scene_define_parts): which primitives move by one matrix.  The part offsets stay on the host, whose
// records (rs::PartRec) carry each named part's range to the device.
struct rs_parts {
    rs_rest_pose rest;               // the parts' primitives, concatenated
    std::vector<int> first;          // [numParts + 1] offsets into rest.primIds
    // scratch of one rs_scene_set_part_transforms: the records, and the host's own baking of the named parts (checks, light areas, mirror)
    std::vector<rs::PartRec> recs;
    std::vector<int> recOf, ids;     // recOf: [numParts] the record of a part named by the call, by stamp
    std::vector<unsigned> recStamp; unsigned stamp = 0;
    std::vector<float> vertices, normals;
    // The named parts' records into `recs` (a part named twice keeps its place and takes its last matrix; an empty part has none) and the host's
    // own baking of their triangles into ids / vertices / normals, in k_bake_parts' order.  The part ids are in range.  Returns the number of triangles.
    __attribute__((visibility("hidden"))) size_t build_records(int count, const int* partIds, const float* matrices16);
};

// The skin of a scene (rs_scene_define_skin): which primitives deform by a blend of bone matrices and, per corner, four bone ids and four
// weights (72 + 96 bytes per listed triangle on the device, and its id).  The palette stays on the host; a pose stages all of it
// (rs::BoneRec, 112 bytes a bone).
struct rs_skin {
    rs_rest_pose rest;
    int numBones = 0;
    std::vector<int> boneIds;        // 12 per listed primitive: corner-major, 4 per corner
    std::vector<float> weights;      // the same shape
    int* dBoneIds = nullptr;         // (16 bytes per corner at a 16-byte aligned base: k_skin reads an int4 and a float4)
    float* dWeights = nullptr;
    std::vector<rs::BoneRec> palette;                   // [numBones] as the last accepted pose left it; identities after the definition
    // scratch of one rs_scene_set_bone_transforms: the palette it asks for, and the host's own skinning (checks, light areas, mirror)
    std::vector<rs::BoneRec> recs;
    std::vector<float> vertices, normals;
    ~rs_skin() { rs_dev_free(dBoneIds); rs_dev_free(dWeights); }
};
