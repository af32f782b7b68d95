// rs_refit.h -- what rs_scene_set_triangles / rs_scene_set_geometry keep per scene (scene_edits.hip: the entry points; rs_geometry_plan.h: their host decisions; scene_refit.hip: tables,
// kernels, rs_refit_boxes), and what an edit whose records a kernel writes hands to them (rs_record_source; the deformers: rs_deform.h).
//
// A refit keeps every tree's topology and recomputes every box from the vertices (the partial refit of rs_scene_set_partial_refit: every
// box above an edited triangle, which leaves the same tables): the reference tree (nodesAll's six orders, occChain)
// and the grid-box trees over the reference's leaf boxes (occNodes, the six orders of ordNodes and, when the edit names an emitter,
// emiNodes on the emissive tree's own grid).  A box is a min / max of floats, taken
// on order-preserving integer keys (-0 below +0), so the result does not depend on the order in which threads arrive and the host
// (rs_refit_boxes) and the device give the same bits.
#pragma once

#include "rs_internal.h"

namespace rs {

// float -> unsigned with the same order (negative values reversed, -0 < +0) and back
RS_HD unsigned refit_key(float x) {
    unsigned u;
    __builtin_memcpy(&u, &x, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
RS_HD float refit_unkey(unsigned k) {
    const unsigned u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
}

}  // namespace rs

struct rs_refit {
    // ---- tables, built on the host and uploaded by the first edit ----
    int* dSlotOf = nullptr;          // [5][numPrims] primitive -> its slot in occTris, then in the three sequences of ordTris, then in emiTris (-1: not emissive)
    int* dEmiLeaf = nullptr;         // [emissive triangles] slot of emiTris -> reference leaf node of its primitive
    int* dLeafOf = nullptr;          // [numPrims] reference leaf node of a primitive
    int* dBoxId = nullptr;           // [6][bvhSize] boundingBoxId of every record of nodesAll
    // One index space for every node a box is computed for: the reference's bvhSize nodes by original id, then the records of occNodes,
    // then all 6 * ordStride / 16 records of ordNodes, then the emiCount + 1 records of emiNodes.  dParent: the parent in that space,
    // -1 at a root, -2 for a record that is no node of a tree (the end records and the padding records: never written).
    int* dParent = nullptr;
    size_t numNodes = 0, gridFirst = 0, occRecords = 0, ordRecords = 0;      // ordRecords: per order (ordStride / 16)
    size_t emiRecords = 0;           // last in the index space, so that an edit that names no emitter simply stops short of them
    bool emiSticky = false;          // the emissive tree was switched off for good (caller-supplied boxes that were not exact unions)
    // ---- the boxes as keys: scratch of a whole refit, and what it leaves is the state a partial refit starts from ----
    unsigned* dKeys = nullptr;       // [numNodes][6] after any refit: the exact key box of every node (the emissive range: only after a refit that reached it)
    unsigned* dArrived = nullptr;    // [numNodes] children that have merged their box into the node
    bool keysValid = false;          // a whole refit has run: dKeys holds every box outside the emissive range, and every later refit keeps it so
    // ---- the partial refit (rs_scene_set_partial_refit; scene_refit.hip).  Trees: the reference tree, then occNodes, then the six orders of
    //      ordNodes, as far as the scene has them; the emissive tree is none of them.  Depths from rs_refit_prepare; the device tables from
    //      the first edit made with the switch on (rs_refit_prepare_partial) ----
    int numTrees = 0;
    int treeDepth[8] = {};           // the deepest leaf of each tree, the root at 0: an edited triangle dirties at most treeDepth + 1 nodes of it
    bool partialReady = false;
    int* dOther = nullptr;           // [numNodes - emiRecords] the node's sibling (-1 at a root, and at a record that is no node)
    int* dLeafNode = nullptr;        // [numTrees - 1][numPrims] primitive -> the leaf record, in the index space, that holds it in each grid-box tree
    int* dNodeRecs = nullptr;        // [bvhSize][6] the inverse of dBoxId: the record of each order of nodesAll that carries the node's box
    unsigned* dExpected = nullptr;   // [numNodes - emiRecords] children of the node that are dirty in the edit under way; 0 between edits
    unsigned* dOwner = nullptr;      // [numNodes - emiRecords] at a leaf: 1 + the lane (edited triangle, tree) that owns it in the edit under way; 0 between edits
    unsigned* dDirty = nullptr;      // [1] nodes the most recent partial refit recomputed (rs_debug_scene_refit_dirty)
    bool lastPartial = false;        // the most recent accepted edit took the partial path
    unsigned long long wholeRefits = 0, partialRefits = 0;      // rs_scene_refit_counts
    // ---- the edited triangles on their way to the device ----
    static constexpr int kStaging = 4;
    struct Stage { char* host = nullptr; size_t capacity = 0; hipEvent_t copied = nullptr; bool pending = false; } stage[kStaging];
    int stageNext = 0;
    char* dStage = nullptr;          // read by the scatter kernel, in the order of the library stream: ids | vertices | normals, copied from a
    size_t dStageCapacity = 0;       // staging buffer or written by an rs_record_source's kernel from its staged records, which then follow them in this buffer
    size_t stagedBytes = 0;          // what the last accepted edit copied from the host (rs_debug_scene_staged_bytes)
    // ---- fences ----
    hipEvent_t before[rs_context::kAux] = {};      // what an internal stream has been handed so far
    hipEvent_t after = nullptr;                    // the edit's kernels
    // ---- the host's copy of the boxes ----
    std::vector<int> hChild;         // [bvhSize][2] children by original node id (-1, -1 at a leaf)
    bool boxesExact = false;         // hBoxes hold rs_refit_boxes of the vertices (from the first accepted edit on)
    size_t root = 0;
};

// An edit whose records a kernel writes on the device (rs_deform.h), as rs_set_geometry knows it.  In the edit's records' place numRecs
// records of 112 bytes are staged (rs_geometry_plan.h partStaged / partOnDevice); `enqueue` has a kernel expand them, on stream st before
// the refit: dRecs is the staged block's device address, dIds | dVertices | dNormals the m triangles in the layout a staged edit has.
struct rs_record_source {
    const void* recs;
    int numRecs;
    const void* owner;               // what else `enqueue` reads: its maker's business
    int (*enqueue)(const rs_record_source& src, const void* dRecs, size_t m, int* dIds, float* dVertices, float* dNormals, hipStream_t st);
};

static inline int fail_named(int code, const char* name, const char* text) { return rs_fail(code, (std::string(name) + ": " + text).c_str()); }      // a refusal under an entry point's name

// scene_edits.hip: rs_scene_set_triangles, rs_scene_set_geometry (emitters) and, with a source, the deformers' edits -- the arrays are then the host's
// own evaluation of the triangles the kernel writes, every id once and in its order.  *taken: the scene took the edit, whatever the call returns.
__attribute__((visibility("hidden"))) int rs_set_geometry(rs_scene* s, int count, const int* primIds, const float* vertices, const float* normals, bool emitters,
                                                          const char* name, const rs_record_source* source = nullptr, bool* taken = nullptr);
// scene_refit.hip
// first edit: builds and uploads the tables, allocates the scratch (waits for the device once: it reads the grid-box trees back)
int rs_refit_prepare(rs_scene* s);
// the first edit made with the switch of rs_scene_set_partial_refit on: builds and uploads the tables of the partial path and allocates
// its counters (waits for the device once, as rs_refit_prepare does: it reads the grid-box trees back again)
int rs_refit_prepare_partial(rs_scene* s);
// one edit, on stream st: scatters the m staged triangles (ids, 9 floats of vertices each, 9 of normals or null: all device pointers) and refits.
// emiTris: the edit names emitters, whose records in emiTris are written too; emiNodes: the emissive tree's boxes are refitted as well, on
// the grid dev.emiBase / emiScale / emiMargin hold at the call.  partial (rs_plan_refit said so; rs_refit_prepare_partial has run): only the
// boxes on the paths from the m triangles' leaves to the roots are recomputed; the emissive range, when asked for, as a whole either way
int rs_refit_enqueue(rs_scene* s, int m, const int* dIds, const float* dVertices, const float* dNormals, bool emiTris, bool emiNodes, bool partial, hipStream_t st);
// rs_scene_set_motion_tracking / rs_scene_advance_motion: prevVertices = vertices (9 floats per triangle, both device arrays), on stream st
int rs_motion_copy_enqueue(const float* vertices, float* prevVertices, size_t numPrims, hipStream_t st);
// the host's side of rs_refit_boxes once the arguments have been checked: `parent` from rs_reference_chain_tables
void rs_refit_boxes_host(int bvhSize, const float* vertices, const int* order0, const int* parent, float* boxes);
// the same boxes when only the m primitives `ids` have moved (boxes: the exact unions of the vertices before the edit): the leaves'
// boxes, then every ancestor's from its two children -- O(m * depth) instead of O(numPrims) for an edit of few triangles
void rs_refit_boxes_host_some(int m, const int* ids, const float* vertices, const int* leafOf, const int* parent, const int* child, float* boxes);
// parents of a pre-order array of 16-byte records (w: sign bit = leaf): parent[i] = base + index, -1 at the root; false: not one binary tree
bool rs_refit_preorder_parents(const unsigned* records, size_t count, int base, int* parent);
