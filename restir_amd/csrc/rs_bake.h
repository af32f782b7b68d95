// rs_bake.h -- instance baking of one corner (src/scene.cpp:167-168), one text for the host and the device:
//     position = vec3(transform * vec4(v, 1))                       mat4 * vec4 (type_mat4x4.inl:612-628)
//     normal   = normalize(normalMat * n)                           normalMat = transpose(mat3(inverse(transform))), mat3 * vec3
// in GLM's grouping of every sum.  The scene-file loader, rs_bake_instance, rs_bake_matrix (scene_file.cpp) and the kernel behind
// rs_scene_set_part_transforms (scene_deform.hip k_bake_parts) all evaluate this function and nothing else, so with -ffp-contract=off and
// the correctly rounded divide and square root of rs_math.h they return the same bits.  skin_corner blends four such corners by weight
// out of the same pieces: rs_skin_corners and the kernel behind rs_scene_set_bone_transforms (scene_deform.hip k_skin) evaluate it alone.
// morph_corner adds weighted per-corner deltas to a rest corner, before the bones where there is a skin: rs_morph_corners and the kernels
// behind rs_scene_set_morph_weights and rs_scene_set_skin_pose (k_morph, k_morph_skin) evaluate it alone.
// The inverse is a host matter: the normal matrix is computed once per matrix (scene_file.cpp bake_normal_matrix) and travels next to it.
#pragma once

#include "rs_math.h"

namespace rs {

// What the device needs of one part of rs_scene_set_part_transforms (112 bytes, staged per named part): the column-major 4x4, the columns
// of the normal matrix, the part's triangles in the rest arrays [restFirst, restFirst + count) and the first triangle it writes.
struct __attribute__((aligned(16))) PartRec {
    float m[16];
    float nm[9];
    int restFirst, count, outFirst;
};

// What the device needs of one bone of rs_scene_set_bone_transforms: the column-major 4x4 and the columns of its normal matrix.  PartRec's
// 112 bytes on purpose: rs_plan_edit_records lays a pose's records out as it lays out part records, with numPartRecs = the number of bones.
struct __attribute__((aligned(16))) BoneRec {
    float m[16];
    float nm[9];
    int pad[3];
};
static_assert(sizeof(BoneRec) == 112 && sizeof(BoneRec) == sizeof(PartRec), "a bone record is staged where a part record is");

struct BakedCorner { f3 position, normal; };

// m: column-major 4x4, m[col * 4 + row]; nm: the normal matrix's three columns, nm[col * 3 + row]
RS_HD f3 bake_position(const float* m, f3 v) {
    return mk3((m[0] * v.x + m[4] * v.y) + (m[8] * v.z + m[12] * 1.f),
               (m[1] * v.x + m[5] * v.y) + (m[9] * v.z + m[13] * 1.f),
               (m[2] * v.x + m[6] * v.y) + (m[10] * v.z + m[14] * 1.f));
}
// nm * n, not yet normalised
RS_HD f3 bake_direction(const float* nm, f3 n) {
    return mk3(nm[0] * n.x + nm[3] * n.y + nm[6] * n.z,
               nm[1] * n.x + nm[4] * n.y + nm[7] * n.z,
               nm[2] * n.x + nm[5] * n.y + nm[8] * n.z);
}
RS_HD BakedCorner bake_corner(const float* m, const float* nm, f3 v, f3 n) {
    BakedCorner o;
    o.position = bake_position(m, v);
    o.normal = normalize(bake_direction(nm, n));
    return o;
}

// Linear blend skinning of one corner (rs_skin_corners, rs_scene_set_bone_transforms; scene_deform.hip k_skin): four influences, bone b[k]
// with weight w[k].  With p_k = bake_position of bone b[k] and q_k = bake_direction of bone b[k]:
//     position = (w0 * p0 + w1 * p1) + (w2 * p2 + w3 * p3)             per component
//     normal   = normalize((w0 * q0 + w1 * q1) + (w2 * q2 + w3 * q3))
// All four influences are always evaluated (a slot of weight 0 still names a valid bone: no branch on the weights), and the weights are
// used as given.  (The reference has no moving geometry: there is no reference line to cite.)
RS_HD f3 skin_blend(const float* w, f3 a, f3 b, f3 c, f3 d) {
    return mk3((w[0] * a.x + w[1] * b.x) + (w[2] * c.x + w[3] * d.x),
               (w[0] * a.y + w[1] * b.y) + (w[2] * c.y + w[3] * d.y),
               (w[0] * a.z + w[1] * b.z) + (w[2] * c.z + w[3] * d.z));
}
RS_HD BakedCorner skin_corner(const BoneRec* bones, const int* b, const float* w, f3 v, f3 n) {
    const BoneRec* b0 = bones + b[0];
    const BoneRec* b1 = bones + b[1];
    const BoneRec* b2 = bones + b[2];
    const BoneRec* b3 = bones + b[3];
    BakedCorner o;
    o.position = skin_blend(w, bake_position(b0->m, v), bake_position(b1->m, v), bake_position(b2->m, v), bake_position(b3->m, v));
    o.normal = normalize(skin_blend(w, bake_direction(b0->nm, n), bake_direction(b1->nm, n), bake_direction(b2->nm, n), bake_direction(b3->nm, n)));
    return o;
}

// One entry of a morph's by-corner table (rs_scene_define_morph, rs_scene_define_skin_morph; rs_deform.h): 32 bytes in two 16-byte halves,
// the target id with the position delta, then the normal delta.  The halves are types of their own so that a reader takes each with one
// 16-byte load, and the second only where it needs it.
struct __attribute__((aligned(16))) MorphHead { int target; float dp[3]; };
struct __attribute__((aligned(16))) MorphTail { float dn[3]; int pad; };
struct __attribute__((aligned(16))) MorphEntry { MorphHead head; MorphTail tail; };
static_assert(sizeof(MorphEntry) == 32 && sizeof(MorphHead) == 16, "a morph entry is two 16-byte loads");

// Weights cross the bus as whole 112-byte records, zero-padded: rs_plan_edit_records lays them out as it lays out part records
constexpr int kMorphWeightsPerRec = (int)(sizeof(BoneRec) / sizeof(float));
static_assert(kMorphWeightsPerRec == 28, "28 weights a record");

// Morph targets of one corner (rs_morph_corners, rs_scene_set_morph_weights, rs_scene_set_skin_pose; scene_deform.hip k_morph, k_morph_skin):
// the corner's entries [first, last) of `entries`, in ascending target id, against the weights w[target]:
//     p = v; q = n
//     for each entry e whose weight w[e.target] != 0 (-0 and +0 both skip):   p = p + w * e.dp,  q = q + w * e.dn     per component
//     position = p;  normal = normalize(q) if any entry was applied, else n
// one multiply and one add per component and entry, in the entries' order.  A corner without an applied entry returns its rest bits, so
// all weights 0 is the rest pose exactly; an entry of weight 0 is read as far as its first half.  Under a skin the result is what
// skin_corner takes in the rest corner's place.  (The reference has no moving geometry: there is no reference line to cite.)
RS_HD BakedCorner morph_corner(const MorphEntry* entries, int first, int last, const float* w, f3 v, f3 n) {
    f3 p = v, q = n;
    bool applied = false;
    for (int e = first; e < last; e++) {
        const MorphHead h = entries[e].head;
        const float wt = w[h.target];
        if (wt != 0.f) {
            const MorphTail t = entries[e].tail;
            p = mk3(p.x + wt * h.dp[0], p.y + wt * h.dp[1], p.z + wt * h.dp[2]);
            q = mk3(q.x + wt * t.dn[0], q.y + wt * t.dn[1], q.z + wt * t.dn[2]);
            applied = true;
        }
    }
    BakedCorner o;
    o.position = p;
    o.normal = applied ? normalize(q) : n;
    return o;
}

}  // namespace rs

// host: the normal matrix of a column-major 4x4 with GLM's inverse (scene_file.cpp); no check: a singular matrix gives non-finite entries
void rs_bake_normal_matrix(const float* matrix16, float* nm9);
// host: n corners, 3 floats each in and out
inline void rs_bake_corners(const float* m, const float* nm, size_t n, const float* vertsIn, const float* normalsIn, float* vertsOut, float* normalsOut) {
    for (size_t i = 0; i < n; i++) {
        const rs::BakedCorner o = rs::bake_corner(m, nm, rs::ld3(vertsIn + i * 3), rs::ld3(normalsIn + i * 3));
        rs::st3(vertsOut + i * 3, o.position);
        rs::st3(normalsOut + i * 3, o.normal);
    }
}
// host: n corners against a palette of bone records, 4 bone ids and 4 weights per corner (the ids are in range: the callers check)
inline void rs_skin_corners_host(const rs::BoneRec* bones, size_t n, const float* vertsIn, const float* normalsIn, const int* boneIds4, const float* weights4,
                                 float* vertsOut, float* normalsOut) {
    for (size_t i = 0; i < n; i++) {
        const rs::BakedCorner o = rs::skin_corner(bones, boneIds4 + i * 4, weights4 + i * 4, rs::ld3(vertsIn + i * 3), rs::ld3(normalsIn + i * 3));
        rs::st3(vertsOut + i * 3, o.position);
        rs::st3(normalsOut + i * 3, o.normal);
    }
}
