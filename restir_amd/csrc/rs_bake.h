// rs_bake.h -- instance baking of one corner (src/scene.cpp:167-168), one text for the host and the device:
//     position = vec3(transform * vec4(v, 1))                       mat4 * vec4 (type_mat4x4.inl:612-628)
//     normal   = normalize(normalMat * n)                           normalMat = transpose(mat3(inverse(transform))), mat3 * vec3
// in GLM's grouping of every sum.  The scene-file loader, rs_bake_instance, rs_bake_matrix (scene_file.cpp) and the kernel behind
// rs_scene_set_part_transforms (scene_refit.hip k_bake_parts) all evaluate this function and nothing else, so with -ffp-contract=off and
// the correctly rounded divide and square root of rs_math.h they return the same bits.  The inverse is a host matter: the normal matrix
// is computed once per matrix (scene_file.cpp bake_normal_matrix) and travels next to it.
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

struct BakedCorner { f3 position, normal; };

// m: column-major 4x4, m[col * 4 + row]; nm: the normal matrix's three columns, nm[col * 3 + row]
RS_HD BakedCorner bake_corner(const float* m, const float* nm, f3 v, f3 n) {
    BakedCorner o;
    o.position = mk3((m[0] * v.x + m[4] * v.y) + (m[8] * v.z + m[12] * 1.f),
                     (m[1] * v.x + m[5] * v.y) + (m[9] * v.z + m[13] * 1.f),
                     (m[2] * v.x + m[6] * v.y) + (m[10] * v.z + m[14] * 1.f));
    o.normal = normalize(mk3(nm[0] * n.x + nm[3] * n.y + nm[6] * n.z,
                             nm[1] * n.x + nm[4] * n.y + nm[7] * n.z,
                             nm[2] * n.x + nm[5] * n.y + nm[8] * n.z));
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
