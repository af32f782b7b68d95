// rs_geometry_plan.h -- the device-free half of a geometry edit (rs_scene_set_triangles, rs_scene_set_geometry, rs_scene_set_part_transforms):
// every check of the caller's arrays, the compaction of repeated ids, the layout of the staged records, and -- when an emitter moves --
// the new light sampler and the emissive tree's new grid, as functions of plain arrays and integers (rs_geometry_edit_view ->
// rs_geometry_edit_plan, include/restir_hip.h); and whether the edit refits the whole scene or only above its triangles (rs_plan_refit).  Nothing here touches the device, a context or a global: scene_edits.hip rs_set_geometry
// fills the view from the scene, asks for the plans and acts on their fields, and rs_debug_plan_geometry_edit hands the same functions to
// a test that has no device.  A refusal is the error code returned and, in `why`, the text as the entry point reports it.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rs_bake.h"
#include "../../include/restir_hip.h"

// occlusion_bvh.cpp: the 16-bit grid a grid-box tree with root box [lo, hi] is quantised on (rs_quantize_occlusion_bvh lays it; an edit that
// moves emitters lays the emissive tree's anew); false: the box has no finite, positive extent
bool rs_grid_over_box(const float lo[3], const float hi[3], float base[3], float scale[3], double* margin);

// Math::triangleArea of nine floats
inline float triangle_area(const float* t) {
    const rs::f3 v0 = rs::ld3(t), v1 = rs::ld3(t + 3), v2 = rs::ld3(t + 6);
    return rs::length(rs::cross(v1 - v0, v2 - v0)) * .5f;
}

inline int rs_plan_refuse(std::string& why, const char* name, const char* text) {
    why = std::string(name) + ": " + text;
    return RS_ERR_INVALID_ARGUMENT;
}

// Which primitives an edit names, and where each one's last record goes: a stamp per primitive instead of a set per edit.  Sizes itself
// on first use; begin() opens the next edit.
struct rs_edit_stamps {
    std::vector<unsigned> lastStamp; // [numPrims] the edit that named the primitive last (a repeated id takes its last record)
    std::vector<int> lastIndex;      //            ... its place in that edit's compacted list
    std::vector<int> lastRecord;     //            ... and which of the edit's records is its last
    unsigned stamp = 0;
    void begin(size_t numPrims) {
        if (lastStamp.size() != numPrims) { lastStamp.assign(numPrims, 0u); lastIndex.assign(numPrims, 0); lastRecord.assign(numPrims, 0); stamp = 0u; }
        if (++stamp == 0u) { std::fill(lastStamp.begin(), lastStamp.end(), 0u); stamp = 1u; }
    }
    bool named(size_t p) const { return lastStamp[p] == stamp; }
};

// Everything up to and including the staging layout.  The checks name the first offending record.  The records, a repeated id keeping its
// last: ids | vertices | normals, each part 16-byte aligned; record i goes to slot stamps.lastIndex[primIds[i]] (rs_fill_edit_records).
// What crosses the bus is the records themselves (staged, onDevice) or numPartRecs part records, which follow the records they expand to
// in the device buffer (partStaged, partOnDevice).
inline int rs_plan_edit_records(const rs_geometry_edit_view& v, int count, const int* primIds, const float* vertices, const float* normals,
                                bool emitters, int numPartRecs, const char* name, rs_edit_stamps& stamps, rs_geometry_edit_plan& plan, std::string& why) {
    if (count < 0 || (count > 0 && (!primIds || !vertices))) return rs_plan_refuse(why, name, "count < 0 or null arrays");
    bool lamps = false;
    for (int i = 0; i < count; i++) {
        const int p = primIds[i];
        if (p < 0 || p >= v.numPrims) return rs_plan_refuse(why, name, "a primitive id out of range");
        if (v.materials[(size_t)v.materialIds[(size_t)p]].type == 4) {
            if (!emitters)
                return rs_plan_refuse(why, name, "a triangle whose material is a Light (the light table, the sampler's powers and the emissive tree are built over the emitters' geometry; rs_scene_set_geometry moves emitters)");
            lamps = true;
        }
        for (int k = 0; k < 9; k++) {
            const float x = vertices[(size_t)i * 9 + k];
            if (!std::isfinite(x) || (normals && !std::isfinite(normals[(size_t)i * 9 + k])))
                return rs_plan_refuse(why, name, "a vertex or normal that is not finite");
            if (v.bounded && !(x >= v.gridLo[k % 3] && x <= v.gridHi[k % 3]))
                return rs_plan_refuse(why, name, "a vertex outside the root box the scene was created with (the grid of its shadow-ray tree lies over that box); build a new scene");
        }
    }
    stamps.begin((size_t)v.numPrims);
    int m = 0;
    for (int i = 0; i < count; i++) {
        const size_t p = (size_t)primIds[i];
        if (stamps.lastStamp[p] != stamps.stamp) { stamps.lastStamp[p] = stamps.stamp; stamps.lastIndex[p] = m++; }
        stamps.lastRecord[p] = i;
    }
    auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
    plan.m = m;
    plan.lamps = lamps ? 1 : 0;
    plan.offV = up((size_t)m * sizeof(int));
    plan.offN = plan.offV + up((size_t)m * 9 * sizeof(float));
    plan.bytes = plan.offN + (normals ? up((size_t)m * 9 * sizeof(float)) : 0);
    plan.staged = plan.onDevice = plan.bytes;
    plan.partStaged = (size_t)numPartRecs * sizeof(rs::PartRec);
    plan.partOnDevice = plan.bytes + plan.partStaged;
    return 0;
}

// The records in their slots: `stage` holds plan.bytes bytes
inline void rs_fill_edit_records(const rs_geometry_edit_plan& plan, const rs_edit_stamps& stamps, int count, const int* primIds, const float* vertices,
                                 const float* normals, char* stage) {
    int* hi = reinterpret_cast<int*>(stage);
    float* hv = reinterpret_cast<float*>(stage + plan.offV);
    float* hn = reinterpret_cast<float*>(stage + plan.offN);
    for (int i = 0; i < count; i++) {
        const size_t j = (size_t)stamps.lastIndex[(size_t)primIds[i]];
        hi[j] = primIds[i];
        std::memcpy(hv + j * 9, vertices + (size_t)i * 9, 9 * sizeof(float));
        if (normals) std::memcpy(hn + j * 9, normals + (size_t)i * 9, 9 * sizeof(float));
    }
}

// Whole refit or partial (rs_scene_set_partial_refit): a function of these integers alone.  m: the distinct triangles the edit names;
// treeDepth[numTrees]: the deepest leaf of every tree the partial path climbs (the reference tree, and the grid-box trees the scene has),
// the root at depth 0.  An edited triangle dirties one leaf and that leaf's ancestors in every tree, so
//     bound = m * sum over the trees of (depth + 1)
// is the most nodes the edit can dirty and, being at least m * numTrees, also bounds the lanes of a launch of the partial path (one per
// edited triangle and tree).  capacity is what the path's owner words can name (kRefitPartialCapacity below).  maxTriangles < 0: the
// library's default.  Partial iff on, keysValid (a whole refit of this scene has left its key boxes), m <= maxTriangles, bound <= capacity.
// numNodes is carried for the record (the whole refit's launches are sized by it); the decision does not read it.
// DESIGN.md section 3 has the measurement the default threshold is set from.
constexpr int kRefitPartialDefaultMaxTriangles = 4096;
// a leaf's owner word holds 1 + the index of a lane of the mark launch in 32 bits: so many lanes can be told apart
constexpr unsigned long long kRefitPartialCapacity = 0xfffffffeull;
inline void rs_plan_refit(bool on, int maxTriangles, bool keysValid, int m, int numTrees, const int* treeDepth, unsigned long long numNodes,
                          unsigned long long capacity, bool* partial, unsigned long long* bound) {
    (void)numNodes;
    unsigned long long perTriangle = 0;
    for (int t = 0; t < numTrees; t++) perTriangle += (unsigned long long)treeDepth[t] + 1ull;
    *bound = (unsigned long long)m * perTriangle;
    const int limit = maxTriangles < 0 ? kRefitPartialDefaultMaxTriangles : maxTriangles;
    *partial = on && keysValid && m <= limit && *bound <= capacity;
}

// The light sampler of numLightPrims light primitives with radiance `rad` (3 floats each), areas `area` and, when numLights is one more, the
// environment entry's power envPower last, as rs_scene_build_textured builds it (rs_build_light_table's powers, rs_build_alias_table)
inline int light_sampler(size_t numLights, size_t numLightPrims, const float* rad, const float* area, float envPower, std::vector<float>& prob,
                         std::vector<int>& fail, float* sumAll, const char* name, std::string& why) {
    const size_t nl = numLights, nlp = numLightPrims;
    std::vector<float> power(nl);
    prob.assign(nl, 0.f); fail.assign(nl, 0);
    for (size_t i = 0; i < nlp; i++) {
        const float perArea = rs::luminance(rs::ld3(rad + i * 3)) * 2.f * rs::kGlmPi;       // rs_build_light_table (scene.cpp:164)
        power[i] = perArea * area[i];
    }
    if (nlp < nl) power[nlp] = envPower;
    *sumAll = 0.f;
    if (nl) {
        if (int e = rs_build_alias_table((int)nl, power.data(), prob.data(), fail.data(), sumAll)) return e;
        if (!(*sumAll > 0.f) || std::isinf(*sumAll)) return rs_plan_refuse(why, name, "the edit leaves the light sampler without a finite, positive total power");
    }
    return 0;
}

// An emitter moves: the new light sampler and the emissive tree's new grid
struct rs_edit_lights_plan {
    std::vector<float> area, prob;
    std::vector<int> fail;
    float sumAll = 0.f;
    float emiLo[3] = {}, emiHi[3] = {};      // the emissive root box: the union of the emissive triangles' boxes, which is what a fresh build starts from
    float emiBase[3] = {}, emiScale[3] = {};
    double emiMargin = 0.0;
    bool emiGrid = false;                    // false: no emissive tree, or emitters collapsed to a box without extent
};

// vertices: the edit's, as rs_plan_edit_records saw them
inline int rs_plan_edit_lights(const rs_geometry_edit_view& v, const rs_edit_stamps& stamps, const float* vertices, const char* name,
                               rs_edit_lights_plan& l, std::string& why) {
    // where a primitive's vertices are once the edit has been applied
    auto edited = [&](size_t p) { return stamps.named(p) ? vertices + (size_t)stamps.lastRecord[p] * 9 : v.vertices + p * 9; };
    l.area.assign(v.lightArea, v.lightArea + v.numLightPrims);
    for (size_t i = 0; i < l.area.size(); i++) {
        const size_t p = (size_t)v.lightPrimIds[i];
        if (stamps.named(p)) l.area[i] = triangle_area(edited(p));
    }
    if (int e = light_sampler((size_t)v.numLights, (size_t)v.numLightPrims, v.lightRadiance, l.area.data(), v.envPower, l.prob, l.fail, &l.sumAll, name, why)) return e;
    l.emiGrid = false;
    if (v.emissiveTree) {
        for (int k = 0; k < 3; k++) { l.emiLo[k] = INFINITY; l.emiHi[k] = -INFINITY; }
        for (int i = 0; i < v.numEmissive; i++) {
            const float* t = edited((size_t)v.emiLeafPrims[i]);
            for (int k = 0; k < 9; k++) { l.emiLo[k % 3] = std::min(l.emiLo[k % 3], t[k]); l.emiHi[k % 3] = std::max(l.emiHi[k % 3], t[k]); }
        }
        l.emiGrid = rs_grid_over_box(l.emiLo, l.emiHi, l.emiBase, l.emiScale, &l.emiMargin);
    }
    return 0;
}
