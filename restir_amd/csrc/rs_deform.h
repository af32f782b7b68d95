// rs_deform.h -- deformers: geometry edits whose records a kernel writes on the device from a rest pose the scene keeps there.  Rigid parts
// (one matrix per part), skinned meshes (a blend of bone matrices per corner) and morph targets (weighted deltas per corner, alone or
// in front of a skin's bones); entry points, kernels and the host's side of all three: scene_deform.hip.  The edit itself is
// rs_set_geometry's (rs_refit.h), which knows of a deformer what rs_record_source says.
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

// Morph targets over a list of corners (rs_scene_define_morph: the corners of a rest pose of the morph's own; rs_scene_define_skin_morph:
// the skin's).  The caller's table is by target; the library keeps it by corner -- cornerFirst[numCorners + 1] into 32-byte entries
// (rs::MorphEntry), a corner's entries in ascending target id -- which fixes the order of every corner's sum.  The device copies are read
// by the morph kernels alone and never written after the definition.  The weights stay on the host, like a skin's palette.
struct __attribute__((visibility("hidden"))) rs_morph_table {
    int numTargets = 0;
    std::vector<int> cornerFirst;
    std::vector<rs::MorphEntry> entries;
    int* dCornerFirst = nullptr;
    rs::MorphEntry* dEntries = nullptr;
    std::vector<float> weights;      // [numTargets] as the last accepted edit left them; 0 after the definition
    std::vector<float> asked;        // scratch of one edit: the weights it asks for
    ~rs_morph_table() { rs_dev_free(dCornerFirst); rs_dev_free(dEntries); }

    // The refusals of the caller's by-target table over numCorners corners, under the entry point's `name`: numTargets out of range, null
    // arrays, offsets that do not start at 0 or decrease, a corner out of range, a (target, corner) pair twice and -- finite -- a delta
    // that is not finite.
    static int check(const char* name, int numTargets, size_t numCorners, const int* targetFirst, const int* entryCorner, const float* deltaPositions,
                     const float* deltaNormals, bool finite);
    // by target -> by corner on the host (the table has passed check); upload(): the two device copies
    void build(int targets, size_t numCorners, const int* targetFirst, const int* entryCorner, const float* deltaPositions, const float* deltaNormals);
    int upload_tables();
    // weights named by an edit into `asked` (a target named twice takes its last); refusals under `name`
    int ask(const char* name, int count, const int* targetIds, const float* w);
    // `asked` as zero-padded 112-byte records at `recs` (records() of them)
    size_t records() const { return ((size_t)numTargets + rs::kMorphWeightsPerRec - 1) / rs::kMorphWeightsPerRec; }
    void fill_records(rs::BoneRec* recs) const;
    // host: morph_corner of every corner against w
    void evaluate(const float* w, const float* vertsIn, const float* normalsIn, float* vertsOut, float* normalsOut) const;
};

// The scene's own morph (rs_scene_define_morph): a rest pose and a table over its corners.
struct rs_morph {
    rs_rest_pose rest;
    rs_morph_table table;
    // scratch of one rs_scene_set_morph_weights: the staged weight records and the host's own morphing (checks, light areas, mirror)
    std::vector<rs::BoneRec> recs;
    std::vector<float> vertices, normals;
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
    // Morph targets on the skin's corners (rs_scene_define_skin_morph), evaluated before the bones; null: none, and a pose is k_skin's.
    // morphed: scratch of one pose, the rest pose after the targets.
    rs_morph_table* morph = nullptr;
    std::vector<float> morphedVertices, morphedNormals;
    ~rs_skin() { rs_dev_free(dBoneIds); rs_dev_free(dWeights); delete morph; }
};
