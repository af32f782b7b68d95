// scene_refit.hip -- the device side of rs_scene_set_triangles and rs_scene_set_geometry (their entry points, staging and fences:
// scene_edits.hip; their checks and layout: rs_geometry_plan.h) and rs_refit_boxes, the same definition on the host.
//
// The whole refit -- every edit unless rs_scene_set_partial_refit is on and rs_plan_refit (rs_geometry_plan.h) says partial; always the
// first edit of a scene -- refits everything: O(numPrims), no ancestor can be left stale.  In the order of one stream:
//   k_refit_clear   every box of the index space of rs_refit.h to the empty box (keys: min = all ones, max = 0), every counter to 0
//   k_scatter       the edited vertices and normals, and the pre-differenced TriRec of every edited triangle wherever it is kept
//                   (tris, occTris, the three sequences of ordTris, and emiTris for an emitter; pad0 / pad1 / pad2 stay)
//   k_ref_leaves    leaf box = AABB(va, vb, vc) (src/bvh.h:20-21); then bottom-up: a node merges its box into its parent's and adds one
//                   to the parent's counter, and the second arrival reads the finished union and climbs on.  The reference tree is up
//                   to 52 deep and far from balanced (Sponza-class scene): nothing here depends on the depth but the length of a climb
//   k_ref_write     the box half of nodesAll's 6 * bvhSize records (each fused with the box its boundingBoxId names) and of occChain
//   k_grid_leaves   the same climb through occNodes and the six orders of ordNodes: a leaf's box is the union of the reference leaf
//                   boxes of its triangles, so every record's box is the union of the reference LEAF boxes below it (the invariant of
//                   occlusion_bvh.cpp; NOT of the reference's inner boxes, which this tree's spans do not match)
//   k_grid_write    quantises outward on the scene's grid (rs_grid.h grid_box: the host builder's function) into the three box dwords
//                   of each record; w -- leaf code or miss link -- the end records and the padding records are never written
// The emissive tree (emiNodes: the shadow tree's kind over the reference leaf boxes of the emissive triangles alone) takes part in the last
// two launches when, and only when, the edit names an emitter (rs_scene_set_geometry): its records come last in the index space, so an edit
// of other triangles stops short of them and writes no byte of emiNodes / emiTris.  Its grid is its own and moves with the lamps: the host
// lays it over the new emissive root box before the launches (scene_edits.hip), so base, scale and margin are per record range (GridArgs).
//
// In front of the refit, for the deformers alone (rs_scene_set_part_transforms, rs_scene_set_bone_transforms): a kernel of scene_deform.hip
// writes the records k_scatter reads -- the staged edit -- from a rest pose, instead of a copy from the host bringing them.
//
// Next to the refit: k_copy_pose, the copy rs_scene_advance_motion makes of the vertices into the scene's previous pose (scene_edits.hip).
//
// Hand-off inside a launch (the two climbs): a parent's box is only ever written by agent-scope atomic min / max and only ever read by
// agent-scope atomic loads, both of which act on the one copy all eight XCDs agree on, never on a CU's L1; a child's merges are ordered
// before its counter add (release, and the wave's outstanding memory operations drained), the second arrival's loads after its own add
// (acquire).  Nobody waits for anybody: the first arrival simply ends.  min / max commute, so the bits do not depend on who arrives first.
//
// The partial refit.  A whole refit leaves, in keys[], the exact key box of every reference node and of every record of occNodes /
// ordNodes; from then on keys[] is STATE, and a partial refit must leave it, and every table, exactly as a whole refit of the same
// vertices would -- boxes that shrink included, which merging into a kept box could never give.  Between edits expected[] and owner[] are
// all 0.  A lane is one (edited triangle, tree); the trees are the reference tree, occNodes and the six orders of ordNodes.  In the order
// of one stream, and what each launch makes valid:
//   k_scatter       as above.  Valid after it: vertices, normals, every TriRec
//   k_partial_mark  every lane claims its triangle's leaf through owner[] (a grid leaf holds up to 7 triangles: the first claim owns it), and
//                   an owner walks up while it is the first to add to expected[parent].  Valid after it: owner[leaf] names one lane of
//                   every dirty leaf; expected[p] = the number of dirty children, 1 or 2, of exactly the ancestors of dirty leaves; keys[p]
//                   of those ancestors is the empty box and arrived[p] is 0 (a whole refit leaves 2 there); dirty[0] = the size of the set
//   k_partial_ref   the reference tree.  An owner computes AABB(va, vb, vc) into keys[leaf], writes the leaf's records -- its record in each
//                   of the six orders of nodesAll, found through nodeRecs, the inverse of boxId, and its record of occChain: what
//                   k_ref_write writes of one node -- and climbs with the hand-off above, except that the arrival that completes a
//                   parent is the expected[p]-th, not the second.  That arrival also merges the KEPT box of the clean sibling when only
//                   one child is dirty (other[]: no launch of this edit writes a clean node's keys), writes the parent's records and
//                   sets expected[p] back to 0.  Valid after it: keys[] and the records of every reference node
//   k_partial_grid  the same through occNodes and ordNodes: a leaf's box is the union of the reference leaf boxes of ALL its triangles,
//                   edited or not (k_grid_leaves' rule; hence the launch after k_partial_ref), a record's three box dwords are
//                   k_grid_write's.  Valid after it: keys[] and the box dwords of every record of these trees; expected[] and
//                   owner[] all 0 again -- no O(numNodes) clear, before or after
// and, when the edit names an emitter, k_refit_clear / k_grid_leaves / k_grid_write over the emissive range alone: the host has laid that
// tree's grid anew, so each of its few thousand records is quantised again whichever emitters moved; its leaves read the reference leaf
// boxes k_partial_ref has finished.  The emissive range of keys[] is scratch here as in the whole refit; nothing relies on it between edits.
// What is never written is what the whole refit never writes.  arrived[] is scratch of either kind of refit.
// Hand-off of the partial climbs: keys[p], arrived[p] and expected[p] of a dirty ancestor are touched, inside a climbing launch, by
// agent-scope atomics alone.  A lane reads expected[p] BEFORE its own add to arrived[p], because the completing arrival stores 0 there;
// that load has returned when the add is issued (the drain in front of the add).  The completing arrival's acquire orders its loads of
// keys[p] after every child's merges; the sibling's kept box and everything else a lane reads was written by an earlier launch.
#include <cmath>
#include <cstring>

#include "rs_refit.h"
#include "rs_grid.h"

using namespace rs;

namespace {

#define RS_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct KeyBox { unsigned lo[3], hi[3]; };

__device__ __forceinline__ KeyBox box_of_triangle(const float* __restrict__ v) {
    KeyBox b;
    for (int k = 0; k < 3; k++) {
        const unsigned a = refit_key(v[k]), c = refit_key(v[3 + k]), d = refit_key(v[6 + k]);
        b.lo[k] = min(a, min(c, d));
        b.hi[k] = max(a, max(c, d));
    }
    return b;
}

// node `cur` holds the finished box b: merge it upwards until a parent still waits for its other child
__device__ __forceinline__ void climb(unsigned* keys, unsigned* arrived, const int* __restrict__ parent, size_t cur, KeyBox b) {
    for (;;) {
        const int p = parent[cur];
        if (p < 0) return;
        unsigned* pk = keys + (size_t)p * 6;
        for (int k = 0; k < 3; k++) {
            (void)__hip_atomic_fetch_min(pk + k, b.lo[k], RS_RLX_AGENT);
            (void)__hip_atomic_fetch_max(pk + 3 + k, b.hi[k], RS_RLX_AGENT);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned before = __hip_atomic_fetch_add(arrived + p, 1u, RS_RLX_AGENT);
        if (before == 0u) return;                          // the other child will find both merges and go on
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        for (int k = 0; k < 3; k++) {
            b.lo[k] = __hip_atomic_load(pk + k, RS_RLX_AGENT);
            b.hi[k] = __hip_atomic_load(pk + 3 + k, RS_RLX_AGENT);
        }
        cur = (size_t)p;
    }
}

__global__ void __launch_bounds__(256) k_refit_clear(unsigned* __restrict__ keys, unsigned* __restrict__ arrived, size_t numNodes) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= numNodes) return;
    unsigned* k = keys + i * 6;
    k[0] = k[1] = k[2] = 0xffffffffu;
    k[3] = k[4] = k[5] = 0u;
    arrived[i] = 0u;
}

struct ScatterArgs {
    float* vertices; float* normals;
    TriRec* tris; TriRec* occTris; TriRec* ordTris;      // occTris / ordTris: null when the scene has no such tree
    TriRec* emiTris;                                     // null unless the edit names an emitter
    const int* slotOf;
    int numPrims;
};
__device__ __forceinline__ void put_triangle(TriRec* r, f3 v0, f3 e1, f3 e2) {      // (pad0, pad1, pad2 stay)
    r->v0x = v0.x; r->v0y = v0.y; r->v0z = v0.z;
    r->e1x = e1.x; r->e1y = e1.y; r->e1z = e1.z;
    r->e2x = e2.x; r->e2y = e2.y; r->e2z = e2.z;
}
// ids are distinct (the host keeps the last record of a repeated id) and in range (checked on the host)
__global__ void __launch_bounds__(256) k_scatter(ScatterArgs a, int m, const int* __restrict__ ids, const float* __restrict__ vertices,
                                                 const float* __restrict__ normals) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const size_t p = (size_t)ids[i], np = (size_t)a.numPrims;
    const float* v = vertices + (size_t)i * 9;
    for (int k = 0; k < 9; k++) a.vertices[p * 9 + k] = v[k];
    if (normals) for (int k = 0; k < 9; k++) a.normals[p * 9 + k] = normals[(size_t)i * 9 + k];
    const TriEdges d = tri_edges(v);                     // as rs_scene_create differences them
    put_triangle(a.tris + p, d.v0, d.e1, d.e2);
    if (a.occTris) put_triangle(a.occTris + a.slotOf[p], d.v0, d.e1, d.e2);
    if (a.ordTris) for (size_t s = 0; s < 3; s++) put_triangle(a.ordTris + s * np + (size_t)a.slotOf[(1 + s) * np + p], d.v0, d.e1, d.e2);
    if (a.emiTris) { const int slot = a.slotOf[4 * np + p]; if (slot >= 0) put_triangle(a.emiTris + slot, d.v0, d.e1, d.e2); }
}

__global__ void __launch_bounds__(256) k_ref_leaves(int numPrims, const float* __restrict__ vertices, const int* __restrict__ leafOf,
                                                    const int* __restrict__ parent, unsigned* keys, unsigned* arrived) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= numPrims) return;
    const KeyBox b = box_of_triangle(vertices + (size_t)p * 9);
    const size_t node = (size_t)leafOf[p];
    for (int k = 0; k < 3; k++) { keys[node * 6 + k] = b.lo[k]; keys[node * 6 + 3 + k] = b.hi[k]; }
    climb(keys, arrived, parent, node, b);
}

__device__ __forceinline__ void write_box_half(BvhNode* r, const unsigned* __restrict__ k) {
    // BvhNode: { min.x, min.y, min.z, max.z | max.x, max.y, primId, next }
    *reinterpret_cast<float4*>(r) = make_float4(refit_unkey(k[0]), refit_unkey(k[1]), refit_unkey(k[2]), refit_unkey(k[5]));
    *reinterpret_cast<float2*>(&r->bmaxx) = make_float2(refit_unkey(k[3]), refit_unkey(k[4]));
}
// records [0, 6 * bvhSize): nodesAll; [6 * bvhSize, 7 * bvhSize): occChain (launched without them when the scene has no shadow tree)
__global__ void __launch_bounds__(256) k_ref_write(size_t numRecords, size_t bvhSize, const int* __restrict__ boxId, const unsigned* __restrict__ keys,
                                                   BvhNode* nodesAll, BvhNode* occChain) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= numRecords) return;
    const bool chain = i >= 6 * bvhSize;
    const size_t id = chain ? i - 6 * bvhSize : (size_t)boxId[i];
    write_box_half(chain ? occChain + id : nodesAll + i, keys + id * 6);
}

struct GridArgs {
    uint4* occNodes; uint4* ordNodes; uint4* emiNodes;   // ordNodes: null when the scene has no ordered trees
    const TriRec* occTris; const TriRec* ordTris;
    const int* emiLeaf;                                  // emiTris carries no reference leaf in pad0: the slot's leaf is kept here
    size_t gridFirst, occRecords, ordRecords, emiFirst;  // emiFirst: the first record (counted from gridFirst) of the emissive tree
    int numPrims;
    float base[3], scale[3], emiBase[3], emiScale[3];
    double margin, emiMargin;
};
// record g of the grid part of the index space: its address, and the triangles a leaf code counts through (null: the emissive tree's)
__device__ __forceinline__ uint4* grid_record(const GridArgs& a, size_t g, const TriRec** tris, int* step) {
    if (g < a.occRecords) { *tris = a.occTris; *step = 1; return a.occNodes + g; }
    if (g >= a.emiFirst) { *tris = nullptr; *step = 1; return a.emiNodes + (g - a.emiFirst); }
    const size_t r = g - a.occRecords, order = r / a.ordRecords;
    *tris = a.ordTris + (order >> 1) * (size_t)a.numPrims;
    *step = (order & 1) ? -1 : 1;                        // the mirrored order meets a leaf's triangles at start, start - 1, ...
    return a.ordNodes + r;
}
// the box of leaf record g (w < 0 holds its code): the union of the reference leaf boxes of its triangles (the reference climb, an earlier launch)
__device__ __forceinline__ KeyBox grid_leaf_box(const GridArgs& a, int meta, const TriRec* tris, int step, const unsigned* __restrict__ keys) {
    const int code = ~meta;
    int tri = code >> 3;
    KeyBox b;
    for (int k = 0; k < 3; k++) { b.lo[k] = 0xffffffffu; b.hi[k] = 0u; }
    for (int n = code & 7; n > 0; n--, tri += step) {
        const unsigned* leaf = keys + (size_t)(tris ? __float_as_int(tris[tri].pad0) : a.emiLeaf[tri]) * 6;
        for (int k = 0; k < 3; k++) { b.lo[k] = min(b.lo[k], leaf[k]); b.hi[k] = max(b.hi[k], leaf[3 + k]); }
    }
    return b;
}
// the three box dwords of a record from its key box k, on the grid its tree is quantised on
__device__ __forceinline__ void put_grid_box(uint4* rec, const unsigned* k, const float* base, const float* scale, double margin) {
    const float lo[3] = { refit_unkey(k[0]), refit_unkey(k[1]), refit_unkey(k[2]) }, hi[3] = { refit_unkey(k[3]), refit_unkey(k[4]), refit_unkey(k[5]) };
    // (the host has checked every vertex against the grid's box, so every box fits; one that did not would become the whole grid: conservative)
    unsigned q[3] = { 0u, 0xffff0000u, 0xffffffffu };
    (void)grid_box(lo, hi, base, scale, margin, q);
    rec->x = q[0]; rec->y = q[1]; rec->z = q[2];
}
__global__ void __launch_bounds__(256) k_grid_leaves(GridArgs a, size_t numRecords, const int* __restrict__ parent, unsigned* keys, unsigned* arrived) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= numRecords) return;
    const size_t node = a.gridFirst + g;
    if (parent[node] == -2) return;                      // an end record or a padding record
    const TriRec* tris; int step;
    const int meta = (int)grid_record(a, g, &tris, &step)->w;
    if (meta >= 0) return;                               // an inner record: its children bring its box
    const KeyBox b = grid_leaf_box(a, meta, tris, step, keys);
    for (int k = 0; k < 3; k++) { keys[node * 6 + k] = b.lo[k]; keys[node * 6 + 3 + k] = b.hi[k]; }
    climb(keys, arrived, parent, node, b);
}
__global__ void __launch_bounds__(256) k_grid_write(GridArgs a, size_t numRecords, const int* __restrict__ parent, const unsigned* __restrict__ keys) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= numRecords) return;
    const size_t node = a.gridFirst + g;
    if (parent[node] == -2) return;
    const TriRec* tris; int step;
    uint4* rec = grid_record(a, g, &tris, &step);
    if (g >= a.emiFirst) put_grid_box(rec, keys + node * 6, a.emiBase, a.emiScale, a.emiMargin);
    else put_grid_box(rec, keys + node * 6, a.base, a.scale, a.margin);
}

// ---- the partial refit (the header comment has the contract) ----
// A lane is one (edited triangle i, tree t): lane = t * m + i, t = 0 the reference tree, then the grid-box trees in the order of the index
// space.  m * numTrees < 2^32 (rs_plan_refit's capacity), so 1 + lane fits an owner word.
struct PartialArgs {
    const int* ids; int m, numTrees, numPrims;
    const int* leafOf; const int* leafNode;              // the triangle's leaf: leafOf[p] in the reference tree, leafNode[(t - 1) * numPrims + p] in grid-box tree t
    const int* parent; const int* other;
    unsigned* keys; unsigned* arrived; unsigned* expected; unsigned* owner; unsigned* dirty;
};
__device__ __forceinline__ size_t partial_leaf(const PartialArgs& a, size_t lane) {
    const size_t t = lane / (size_t)a.m, p = (size_t)a.ids[lane - t * (size_t)a.m];
    return (size_t)(t == 0 ? a.leafOf[p] : a.leafNode[(t - 1) * (size_t)a.numPrims + p]);
}
// The dirty set and what the climbs need of it.  The first lane to claim a leaf owns it (a grid leaf holds up to 7 triangles); an owner
// walks up, adds one to expected[] of each parent and goes on only where it was the first to, emptying that parent's key box and its
// arrival counter (a whole refit leaves 2 there).  Afterwards expected[p] is the number of p's children that are dirty, 1 or 2, on
// exactly the ancestors of the edited leaves.  Nothing read here is written here but through the atomics; the climbs are later launches.
__global__ void __launch_bounds__(256) k_partial_mark(PartialArgs a) {
    __shared__ unsigned blockDirty;
    if (threadIdx.x == 0) blockDirty = 0u;
    __syncthreads();
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned mine = 0u;
    if (lane < (size_t)a.m * (size_t)a.numTrees) {
        size_t cur = partial_leaf(a, lane);
        unsigned nobody = 0u;
        if (__hip_atomic_compare_exchange_strong(a.owner + cur, &nobody, (unsigned)lane + 1u, __ATOMIC_RELAXED, RS_RLX_AGENT)) {
            mine = 1u;
            for (;;) {
                const int p = a.parent[cur];
                if (p < 0 || __hip_atomic_fetch_add(a.expected + p, 1u, RS_RLX_AGENT) != 0u) break;
                unsigned* k = a.keys + (size_t)p * 6;
                k[0] = k[1] = k[2] = 0xffffffffu;
                k[3] = k[4] = k[5] = 0u;
                a.arrived[p] = 0u;
                mine++;
                cur = (size_t)p;
            }
        }
    }
    if (mine) (void)atomicAdd(&blockDirty, mine);
    __syncthreads();
    if (threadIdx.x == 0 && blockDirty) (void)__hip_atomic_fetch_add(a.dirty, blockDirty, RS_RLX_AGENT);
}
// this lane owns `leaf` (k_partial_mark, an earlier launch); the word goes back to 0 for the next edit.  The other lanes of the leaf compare
// the word with their own number only, which nobody writes
__device__ __forceinline__ bool take_leaf(const PartialArgs& a, size_t leaf, size_t lane) {
    if (__hip_atomic_load(a.owner + leaf, RS_RLX_AGENT) != (unsigned)lane + 1u) return false;
    __hip_atomic_store(a.owner + leaf, 0u, RS_RLX_AGENT);
    return true;
}
// climb() where only some leaves move: node `cur` holds the finished box b and has written its records.  The hand-off is climb()'s; the
// arrival that completes expected[p] -- read before the lane's own add, since that arrival sets it back to 0 -- finds every dirty child's
// merge, adds the kept box of a clean sibling (no launch of this edit writes it), writes the parent's records and goes on.
template <class Write>
__device__ __forceinline__ void climb_partial(const PartialArgs& a, size_t cur, KeyBox b, const Write& write) {
    for (;;) {
        const int p = a.parent[cur];
        if (p < 0) return;
        unsigned* pk = a.keys + (size_t)p * 6;
        for (int k = 0; k < 3; k++) {
            (void)__hip_atomic_fetch_min(pk + k, b.lo[k], RS_RLX_AGENT);
            (void)__hip_atomic_fetch_max(pk + 3 + k, b.hi[k], RS_RLX_AGENT);
        }
        const unsigned expected = __hip_atomic_load(a.expected + p, RS_RLX_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned before = __hip_atomic_fetch_add(a.arrived + p, 1u, RS_RLX_AGENT);
        if (before + 1u < expected) return;               // the other dirty child will find both merges and go on
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (expected == 1u) {
            const unsigned* sk = a.keys + (size_t)a.other[cur] * 6;
            for (int k = 0; k < 3; k++) {
                (void)__hip_atomic_fetch_min(pk + k, __hip_atomic_load(sk + k, RS_RLX_AGENT), RS_RLX_AGENT);
                (void)__hip_atomic_fetch_max(pk + 3 + k, __hip_atomic_load(sk + 3 + k, RS_RLX_AGENT), RS_RLX_AGENT);
            }
        }
        for (int k = 0; k < 3; k++) {
            b.lo[k] = __hip_atomic_load(pk + k, RS_RLX_AGENT);
            b.hi[k] = __hip_atomic_load(pk + 3 + k, RS_RLX_AGENT);
        }
        write((size_t)p, b);
        __hip_atomic_store(a.expected + p, 0u, RS_RLX_AGENT);
        cur = (size_t)p;
    }
}
// what k_ref_write writes of one reference node: its record in each order of nodesAll (nodeRecs: the inverse of boxId) and in occChain
struct RefWrite {
    const int* nodeRecs; BvhNode* nodesAll; BvhNode* occChain; size_t bvhSize;
    __device__ __forceinline__ void operator()(size_t node, const KeyBox& b) const {
        const unsigned k[6] = { b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2] };
        for (size_t o = 0; o < 6; o++) write_box_half(nodesAll + o * bvhSize + (size_t)nodeRecs[node * 6 + o], k);
        if (occChain) write_box_half(occChain + node, k);
    }
};
// what k_grid_write writes of one record of occNodes / ordNodes (the emissive tree is not climbed here)
struct GridWrite {
    GridArgs g;
    __device__ __forceinline__ void operator()(size_t node, const KeyBox& b) const {
        const unsigned k[6] = { b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2] };
        const TriRec* tris; int step;
        put_grid_box(grid_record(g, node - g.gridFirst, &tris, &step), k, g.base, g.scale, g.margin);
    }
};
__device__ __forceinline__ void put_keys(unsigned* keys, size_t node, const KeyBox& b) {
    for (int k = 0; k < 3; k++) { keys[node * 6 + k] = b.lo[k]; keys[node * 6 + 3 + k] = b.hi[k]; }
}
// lanes [0, m): the reference tree, after k_scatter
__global__ void __launch_bounds__(256) k_partial_ref(PartialArgs a, const float* __restrict__ vertices, RefWrite write) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= (size_t)a.m) return;
    const size_t node = partial_leaf(a, lane);
    if (!take_leaf(a, node, lane)) return;
    const KeyBox b = box_of_triangle(vertices + (size_t)a.ids[lane] * 9);
    put_keys(a.keys, node, b);
    write(node, b);
    climb_partial(a, node, b, write);
}
// lanes [m, m * numTrees): the grid-box trees, after k_partial_ref has finished the reference leaf boxes their leaves are unions of
__global__ void __launch_bounds__(256) k_partial_grid(PartialArgs a, GridWrite write) {
    const size_t lane = (size_t)a.m + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= (size_t)a.m * (size_t)a.numTrees) return;
    const size_t node = partial_leaf(a, lane);
    if (!take_leaf(a, node, lane)) return;
    const TriRec* tris; int step;
    const int meta = (int)grid_record(write.g, node - write.g.gridFirst, &tris, &step)->w;
    const KeyBox b = grid_leaf_box(write.g, meta, tris, step, a.keys);
    put_keys(a.keys, node, b);
    write(node, b);
    climb_partial(a, node, b, write);
}

// rs_scene_advance_motion: the pose as it stands becomes the previous pose.  The whole array, one float per lane (DESIGN.md section 3:
// 36 B per triangle read and written once costs less than a dirty list's staging copy and fence)
__global__ void __launch_bounds__(256) k_copy_pose(const float* __restrict__ vertices, float* __restrict__ prevVertices, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) prevVertices[i] = vertices[i];
}

inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

bool rs_refit_preorder_parents(const unsigned* records, size_t count, int base, int* parent) {
    // pre-order, every inner record with exactly two subtrees behind it: the open inner records form a stack
    struct Open { int node, left; };
    std::vector<Open> open;
    for (size_t i = 0; i < count; i++) {
        if (i > 0 && open.empty()) return false;         // a second root
        parent[i] = open.empty() ? -1 : base + open.back().node;
        if (!open.empty() && --open.back().left == 0) open.pop_back();
        if ((int)records[i * 4 + 3] >= 0) open.push_back(Open{ (int)i, 2 });
    }
    return count > 0 && open.empty();
}

void rs_refit_boxes_host(int bvhSize, const float* vertices, const int* order0, const int* parent, float* boxes) {
    const size_t nn = (size_t)bvhSize;
    std::vector<unsigned> keys(nn * 6);
    for (size_t i = 0; i < nn; i++) { unsigned* k = &keys[i * 6]; k[0] = k[1] = k[2] = 0xffffffffu; k[3] = k[4] = k[5] = 0u; }
    // order 0 is a pre-order (a child's index is larger than its parent's, rs_reference_chain_tables): backwards, a node's box is
    // complete before it is merged into its parent's
    for (size_t i = nn; i-- > 0;) {
        const int prim = order0[i * 3], id = order0[i * 3 + 1];
        unsigned* k = &keys[(size_t)id * 6];
        if (prim >= 0) {
            const float* v = vertices + (size_t)prim * 9;
            for (int c = 0; c < 3; c++) {
                const unsigned a = refit_key(v[c]), b = refit_key(v[3 + c]), d = refit_key(v[6 + c]);
                k[c] = std::min(a, std::min(b, d));
                k[3 + c] = std::max(a, std::max(b, d));
            }
        }
        if (parent[id] >= 0) {
            unsigned* q = &keys[(size_t)parent[id] * 6];
            for (int c = 0; c < 3; c++) { q[c] = std::min(q[c], k[c]); q[3 + c] = std::max(q[3 + c], k[3 + c]); }
        }
    }
    for (size_t i = 0; i < nn * 6; i++) boxes[i] = refit_unkey(keys[i]);
}

void rs_refit_boxes_host_some(int m, const int* ids, const float* vertices, const int* leafOf, const int* parent, const int* child, float* boxes) {
    auto lower = [](float a, float b) { return refit_key(a) < refit_key(b) ? a : b; };
    auto upper = [](float a, float b) { return refit_key(a) > refit_key(b) ? a : b; };
    for (int j = 0; j < m; j++) {
        const float* v = vertices + (size_t)ids[j] * 9;
        float* b = boxes + (size_t)leafOf[ids[j]] * 6;
        for (int c = 0; c < 3; c++) { b[c] = lower(v[c], lower(v[3 + c], v[6 + c])); b[3 + c] = upper(v[c], upper(v[3 + c], v[6 + c])); }
    }
    // One climb per moved leaf, every ancestor recomputed from its children as they are then.  An ancestor is final after the last climb
    // through it: that climb comes through one child, just recomputed, and the other child saw its own last climb earlier.
    for (int j = 0; j < m; j++)
        for (int n = parent[leafOf[ids[j]]]; n >= 0; n = parent[n]) {
            const float* a = boxes + (size_t)child[(size_t)n * 2] * 6;
            const float* b = boxes + (size_t)child[(size_t)n * 2 + 1] * 6;
            float* o = boxes + (size_t)n * 6;
            for (int c = 0; c < 3; c++) { o[c] = lower(a[c], b[c]); o[3 + c] = upper(a[3 + c], b[3 + c]); }
        }
}

extern "C" int rs_refit_boxes(int numPrims, const float* vertices, int bvhSize, const int* order0, float* boundingBoxes) {
    if (numPrims <= 0 || bvhSize != 2 * numPrims - 1 || !vertices || !order0 || !boundingBoxes)
        return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_refit_boxes: null array, or bvhSize is not 2 * numPrims - 1");
    for (size_t i = 0; i < (size_t)numPrims * 9; i++)
        if (!std::isfinite(vertices[i])) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_refit_boxes: a vertex that is not finite");
    for (size_t i = 0; i < (size_t)bvhSize; i++) {
        const int* n = order0 + i * 3;
        if (n[0] < -1 || n[0] >= numPrims || n[2] <= (int)i || n[2] > bvhSize)
            return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_refit_boxes: a primitive id out of range or a link that does not point forward");
    }
    std::vector<int> parent, leafOf;
    RS_TRY(rs_reference_chain_tables(bvhSize, order0, parent, leafOf, numPrims));
    rs_refit_boxes_host(bvhSize, vertices, order0, parent.data(), boundingBoxes);
    return 0;
}

int rs_motion_copy_enqueue(const float* vertices, float* prevVertices, size_t numPrims, hipStream_t st) {
    const size_t count = numPrims * 9;
    if (count == 0) return 0;
    hipLaunchKernelGGL(k_copy_pose, dim3(blocks_for(count)), dim3(256), 0, st, vertices, prevVertices, count);
    return rs_check_hip(hipGetLastError(), "rs_scene_advance_motion: copy kernel");
}

void rs_refit_free(rs_scene* s) {
    rs_refit* r = s->refit;
    if (!r) return;
    rs_dev_free(r->dSlotOf); rs_dev_free(r->dEmiLeaf); rs_dev_free(r->dLeafOf); rs_dev_free(r->dBoxId); rs_dev_free(r->dParent);
    rs_dev_free(r->dKeys); rs_dev_free(r->dArrived); rs_dev_free(r->dStage);
    rs_dev_free(r->dOther); rs_dev_free(r->dLeafNode); rs_dev_free(r->dNodeRecs); rs_dev_free(r->dExpected); rs_dev_free(r->dOwner); rs_dev_free(r->dDirty);
    for (rs_refit::Stage& g : r->stage) {
        if (g.host) (void)hipHostFree(g.host);
        if (g.copied) (void)hipEventDestroy(g.copied);
    }
    for (hipEvent_t e : r->before) if (e) (void)hipEventDestroy(e);
    if (r->after) (void)hipEventDestroy(r->after);
    delete r;
    s->refit = nullptr;
}

namespace {

// the deepest node of the tree whose nodes are records [first, first + count) of the index space (records that are no node: parent -2), the root at 0
int tree_depth(const std::vector<int>& parent, size_t first, size_t count) {
    std::vector<int> depth(count, -1);
    std::vector<size_t> path;
    int deepest = 0;
    for (size_t i = 0; i < count; i++) {
        if (parent[first + i] == -2) continue;
        path.clear();
        size_t n = i;
        while (depth[n] < 0 && parent[first + n] >= 0) { path.push_back(n); n = (size_t)parent[first + n] - first; }
        if (depth[n] < 0) depth[n] = 0;                  // the root
        int d = depth[n];
        for (size_t j = path.size(); j-- > 0;) depth[path[j]] = ++d;
        deepest = std::max(deepest, d);
    }
    return deepest;
}

}  // namespace

int rs_refit_prepare(rs_scene* s) {
    if (s->refit) return 0;
    const size_t np = (size_t)s->numPrims, nn = (size_t)s->bvhSize;
    rs_refit* r = new rs_refit();
    s->refit = r;                                        // (whatever a failure below leaves allocated, rs_scene_destroy frees)
    const bool occ = s->dOccNodes != nullptr, ord = s->dOrdNodes != nullptr;
    r->occRecords = occ ? (size_t)s->dev.occCount : 0;
    r->ordRecords = ord ? (size_t)s->dev.ordStride / 16 : 0;
    const bool emi = s->dEmiNodes != nullptr && s->dev.emiCount > 0;
    r->emiRecords = emi ? (size_t)s->dev.emiCount + 1 : 0;
    r->gridFirst = nn;
    r->numNodes = nn + r->occRecords + 6 * r->ordRecords + r->emiRecords;
    if (r->numNodes >= 0x7fffffffull) { rs_refit_free(s); return rs_fail(RS_ERR_UNSUPPORTED, "rs_scene_set_triangles: the scene's trees have more than 2^31 nodes"); }

    // primitive -> slot: occTris in the shadow tree's leaf order, ordTris in the sequences of the even threaded orders
    std::vector<int> slotOf(5 * np, 0), emiLeaf(s->hEmiLeafPrims.size());
    std::fill(slotOf.begin() + 4 * np, slotOf.end(), -1);
    for (size_t i = 0; i < emiLeaf.size(); i++) {
        slotOf[4 * np + (size_t)s->hEmiLeafPrims[i]] = (int)i;
        emiLeaf[i] = s->hLeafOf[(size_t)s->hEmiLeafPrims[i]];
    }
    if (occ) {
        if (s->hOccLeafPrims.size() != np) { rs_refit_free(s); return rs_fail(RS_ERR_INTERNAL, "rs_scene_set_triangles: the shadow tree's leaf order was not kept"); }
        for (size_t i = 0; i < np; i++) slotOf[(size_t)s->hOccLeafPrims[i]] = (int)i;
    }
    if (ord)
        for (size_t a = 0; a < 3; a++) {
            size_t j = 0;
            for (size_t i = 0; i < nn; i++) { const int p = s->hNodes[2 * a][i * 3]; if (p >= 0) slotOf[(1 + a) * np + (size_t)p] = (int)j++; }
        }
    std::vector<int> boxId(6 * nn);
    for (size_t k = 0; k < 6; k++) for (size_t i = 0; i < nn; i++) boxId[k * nn + i] = s->hNodes[k][i * 3 + 1];

    // parents: the reference's by original id (hParent); the grid-box trees' from their records, read back once
    std::vector<int> parent(r->numNodes, -2);
    std::memcpy(parent.data(), s->hParent.data(), nn * sizeof(int));
    bool trees = true;
    if (occ) {
        std::vector<unsigned> rec(r->occRecords * 4);
        RS_HIP(hipMemcpy(rec.data(), s->dOccNodes, rec.size() * 4, hipMemcpyDeviceToHost));
        trees = rs_refit_preorder_parents(rec.data(), r->occRecords, (int)nn, &parent[nn]);
    }
    if (ord && trees) {
        std::vector<unsigned> rec(6 * r->ordRecords * 4);
        RS_HIP(hipMemcpy(rec.data(), s->dOrdNodes, rec.size() * 4, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < 6 && trees; k++) {
            // the tree of order k: the records from the stride's start up to the first one that is linked to the end record without being
            // a leaf and has an empty box (scene.hip build_ordered_side pads with those), i.e. as many as a binary tree over its leaves has
            const unsigned* t = &rec[k * r->ordRecords * 4];
            size_t leaves = 0, count = 0;
            while (count < r->ordRecords - 1) {          // (the last slot is the end record)
                if ((int)t[count * 4 + 3] < 0) leaves++;
                count++;
                if (count == 2 * leaves - 1) break;      // pre-order: the tree is complete exactly here
            }
            const size_t first = nn + r->occRecords + k * r->ordRecords;
            trees = leaves > 0 && count == 2 * leaves - 1 && rs_refit_preorder_parents(t, count, (int)first, &parent[first]);
        }
    }
    if (emi && trees) {
        std::vector<unsigned> rec((size_t)s->dev.emiCount * 4);
        RS_HIP(hipMemcpy(rec.data(), s->dEmiNodes, rec.size() * 4, hipMemcpyDeviceToHost));
        const size_t first = nn + r->occRecords + 6 * r->ordRecords;
        trees = rs_refit_preorder_parents(rec.data(), (size_t)s->dev.emiCount, (int)first, &parent[first]);
        // a leaf code must stay inside emiTris: the refit reads emiLeaf through it
        for (size_t i = 0; i < (size_t)s->dev.emiCount && trees; i++) {
            const int w = (int)rec[i * 4 + 3];
            if (w < 0) trees = (size_t)(~w >> 3) + (size_t)(~w & 7) <= emiLeaf.size();
        }
    }
    if (!trees) { rs_refit_free(s); return rs_fail(RS_ERR_INTERNAL, "rs_scene_set_triangles: a grid-box tree is not a binary tree in pre-order"); }
    // what rs_plan_refit asks of the trees a partial refit climbs: how deep each one is
    r->treeDepth[r->numTrees++] = tree_depth(parent, 0, nn);
    if (occ) r->treeDepth[r->numTrees++] = tree_depth(parent, nn, r->occRecords);
    for (size_t k = 0; ord && k < 6; k++) r->treeDepth[r->numTrees++] = tree_depth(parent, nn + r->occRecords + k * r->ordRecords, r->ordRecords);

    int e = upload(&r->dSlotOf, slotOf);
    if (!e) e = upload(&r->dEmiLeaf, emiLeaf);
    if (!e) e = upload(&r->dLeafOf, s->hLeafOf);
    if (!e) e = upload(&r->dBoxId, boxId);
    if (!e) e = upload(&r->dParent, parent);
    if (!e) e = rs_dev_alloc(&r->dKeys, r->numNodes * 6);
    if (!e) e = rs_dev_alloc(&r->dArrived, r->numNodes);
    for (rs_refit::Stage& g : r->stage) if (!e) e = rs_check_hip(hipEventCreateWithFlags(&g.copied, hipEventDisableTiming), "hipEventCreate");
    for (hipEvent_t& ev : r->before) if (!e) e = rs_check_hip(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate");
    if (!e) e = rs_check_hip(hipEventCreateWithFlags(&r->after, hipEventDisableTiming), "hipEventCreate");
    if (e) { rs_refit_free(s); return e; }
    r->hChild.assign(nn * 2, -1);
    for (size_t i = 0; i < nn; i++) {
        const int p = s->hParent[i];
        if (p < 0) r->root = i;
        else r->hChild[(size_t)p * 2 + (r->hChild[(size_t)p * 2] < 0 ? 0 : 1)] = (int)i;      // (a tree: rs_reference_chain_tables gave every inner node two children)
    }
    return 0;
}

namespace {

GridArgs grid_args(const rs_scene* s, const rs_refit* r) {
    return GridArgs{ s->dOccNodes, s->dOrdNodes, s->dEmiNodes, s->dOccTris, s->dOrdTris, r->dEmiLeaf, r->gridFirst, r->occRecords, r->ordRecords,
                     r->occRecords + 6 * r->ordRecords, s->numPrims,
                     { s->dev.occBase.x, s->dev.occBase.y, s->dev.occBase.z }, { s->dev.occScale.x, s->dev.occScale.y, s->dev.occScale.z },
                     { s->dev.emiBase.x, s->dev.emiBase.y, s->dev.emiBase.z }, { s->dev.emiScale.x, s->dev.emiScale.y, s->dev.emiScale.z },
                     s->gridMargin, s->emiMargin };
}

// rs_refit_enqueue, the partial path: the launches of the header comment, in its order
int partial_enqueue(rs_scene* s, int m, const int* dIds, const float* dVertices, const float* dNormals, bool emiTris, bool emiNodes, hipStream_t st) {
    rs_refit* r = s->refit;
    const bool occ = s->dOccNodes != nullptr, ord = s->dOrdNodes != nullptr;
    r->partialRefits++;
    RS_HIP(hipMemsetAsync(r->dDirty, 0, sizeof(unsigned), st));
    ScatterArgs sa{ s->dVertices, s->dNormals, s->dTris, occ ? s->dOccTris : nullptr, ord ? s->dOrdTris : nullptr,
                    emiTris && r->emiRecords ? s->dEmiTris : nullptr, r->dSlotOf, s->numPrims };
    hipLaunchKernelGGL(k_scatter, dim3(blocks_for((size_t)m)), dim3(256), 0, st, sa, m, dIds, dVertices, dNormals);
    const PartialArgs pa{ dIds, m, r->numTrees, s->numPrims, r->dLeafOf, r->dLeafNode, r->dParent, r->dOther, r->dKeys, r->dArrived, r->dExpected, r->dOwner, r->dDirty };
    const size_t lanes = (size_t)m * (size_t)r->numTrees;
    hipLaunchKernelGGL(k_partial_mark, dim3(blocks_for(lanes)), dim3(256), 0, st, pa);
    const RefWrite rw{ r->dNodeRecs, s->dNodesAll, occ ? s->dOccChain : nullptr, (size_t)s->bvhSize };
    hipLaunchKernelGGL(k_partial_ref, dim3(blocks_for((size_t)m)), dim3(256), 0, st, pa, (const float*)s->dVertices, rw);
    const GridArgs ga = grid_args(s, r);
    if (r->numTrees > 1) hipLaunchKernelGGL(k_partial_grid, dim3(blocks_for(lanes - (size_t)m)), dim3(256), 0, st, pa, GridWrite{ ga });
    if (emiNodes && r->emiRecords) {
        // the emissive tree as the whole refit treats it, over its own records alone: its grid has just moved, so every one of them is quantised again
        GridArgs ea = ga;
        ea.gridFirst = r->gridFirst + ga.emiFirst; ea.occRecords = 0; ea.emiFirst = 0;
        hipLaunchKernelGGL(k_refit_clear, dim3(blocks_for(r->emiRecords)), dim3(256), 0, st, r->dKeys + ea.gridFirst * 6, r->dArrived + ea.gridFirst, r->emiRecords);
        hipLaunchKernelGGL(k_grid_leaves, dim3(blocks_for(r->emiRecords)), dim3(256), 0, st, ea, r->emiRecords, (const int*)r->dParent, r->dKeys, r->dArrived);
        hipLaunchKernelGGL(k_grid_write, dim3(blocks_for(r->emiRecords)), dim3(256), 0, st, ea, r->emiRecords, (const int*)r->dParent, (const unsigned*)r->dKeys);
    }
    return rs_check_hip(hipGetLastError(), "rs_scene_set_triangles: partial refit kernels");
}

}  // namespace

// The tables of the partial path (rs_refit.h), from the parents as the device holds them and the grid-box trees' leaf codes, read back again:
// w is never written by an edit, so it does not matter how many edits lie between rs_refit_prepare and this.
int rs_refit_prepare_partial(rs_scene* s) {
    rs_refit* r = s->refit;
    if (r->partialReady) return 0;
    const size_t np = (size_t)s->numPrims, nn = (size_t)s->bvhSize, space = r->numNodes - r->emiRecords;
    const bool occ = s->dOccNodes != nullptr, ord = s->dOrdNodes != nullptr;
    std::vector<int> parent(space);
    RS_HIP(hipMemcpy(parent.data(), r->dParent, space * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<int> other(space, -1), firstChild(space, -1);
    for (size_t i = 0; i < space; i++) {
        const int p = parent[i];
        if (p < 0) continue;
        if (firstChild[(size_t)p] < 0) firstChild[(size_t)p] = (int)i;
        else { other[i] = firstChild[(size_t)p]; other[(size_t)firstChild[(size_t)p]] = (int)i; }
    }
    std::vector<int> nodeRecs(nn * 6);
    for (size_t k = 0; k < 6; k++) for (size_t i = 0; i < nn; i++) nodeRecs[(size_t)s->hNodes[k][i * 3 + 1] * 6 + k] = (int)i;

    // primitive -> leaf record of every grid-box tree: a leaf code counts through slots of occTris / of a sequence of ordTris
    std::vector<int> leafNode((size_t)(r->numTrees - 1) * np, -1);
    bool inside = true;
    auto leaves = [&](size_t tree, const unsigned* rec, size_t first, size_t count, const std::vector<int>& primOfSlot, int step) {
        for (size_t g = 0; g < count; g++) {
            const int w = (int)rec[g * 4 + 3];
            if (parent[first + g] == -2 || w >= 0) continue;
            long long slot = ~w >> 3;
            for (int n = ~w & 7; n > 0; n--, slot += step) {
                if (slot < 0 || slot >= (long long)np) { inside = false; return; }
                leafNode[tree * np + (size_t)primOfSlot[(size_t)slot]] = (int)(first + g);
            }
        }
    };
    size_t tree = 0;
    if (occ) {
        std::vector<unsigned> rec(r->occRecords * 4);
        RS_HIP(hipMemcpy(rec.data(), s->dOccNodes, rec.size() * 4, hipMemcpyDeviceToHost));
        leaves(tree++, rec.data(), nn, r->occRecords, s->hOccLeafPrims, 1);
    }
    if (ord) {
        std::vector<unsigned> rec(6 * r->ordRecords * 4);
        RS_HIP(hipMemcpy(rec.data(), s->dOrdNodes, rec.size() * 4, hipMemcpyDeviceToHost));
        std::vector<int> primOfSlot;
        for (size_t k = 0; k < 6; k++) {
            if (!(k & 1)) {                              // the sequence of the even order, shared with its mirror (rs_refit_prepare slotOf)
                primOfSlot.clear();
                for (size_t i = 0; i < nn; i++) { const int p = s->hNodes[k][i * 3]; if (p >= 0) primOfSlot.push_back(p); }
                if (primOfSlot.size() != np) inside = false;
            }
            if (inside) leaves(tree++, &rec[k * r->ordRecords * 4], nn + r->occRecords + k * r->ordRecords, r->ordRecords, primOfSlot, (k & 1) ? -1 : 1);
        }
    }
    for (size_t i = 0; i < leafNode.size() && inside; i++) inside = leafNode[i] >= 0;
    if (!inside) return rs_fail(RS_ERR_INTERNAL, "rs_scene_set_partial_refit: a grid-box tree's leaves do not hold every triangle once");

    int e = upload(&r->dOther, other);
    if (!e) e = upload(&r->dLeafNode, leafNode);
    if (!e) e = upload(&r->dNodeRecs, nodeRecs);
    if (!e) e = rs_dev_alloc(&r->dExpected, space);
    if (!e) e = rs_dev_alloc(&r->dOwner, space);
    if (!e) e = rs_dev_alloc(&r->dDirty, 1);
    if (!e) e = rs_check_hip(hipMemset(r->dExpected, 0, space * sizeof(unsigned)), "hipMemset");
    if (!e) e = rs_check_hip(hipMemset(r->dOwner, 0, space * sizeof(unsigned)), "hipMemset");
    if (!e) e = rs_check_hip(hipMemset(r->dDirty, 0, sizeof(unsigned)), "hipMemset");
    if (e) {      // (the scene stays editable: whole refits need none of these)
        rs_dev_free(r->dOther); rs_dev_free(r->dLeafNode); rs_dev_free(r->dNodeRecs); rs_dev_free(r->dExpected); rs_dev_free(r->dOwner); rs_dev_free(r->dDirty);
        return e;
    }
    r->partialReady = true;
    return 0;
}

int rs_refit_enqueue(rs_scene* s, int m, const int* dIds, const float* dVertices, const float* dNormals, bool emiTris, bool emiNodes, bool partial, hipStream_t st) {
    rs_refit* r = s->refit;
    const size_t np = (size_t)s->numPrims, nn = (size_t)s->bvhSize;
    const bool occ = s->dOccNodes != nullptr, ord = s->dOrdNodes != nullptr;
    const size_t emiRecords = emiNodes ? r->emiRecords : 0, numNodes = r->numNodes - r->emiRecords + emiRecords;
    r->lastPartial = partial;
    if (partial) return partial_enqueue(s, m, dIds, dVertices, dNormals, emiTris, emiNodes, st);
    r->wholeRefits++;
    r->keysValid = true;                                 // (in the order of the stream: after the launches below)
    hipLaunchKernelGGL(k_refit_clear, dim3(blocks_for(numNodes)), dim3(256), 0, st, r->dKeys, r->dArrived, numNodes);
    ScatterArgs sa{ s->dVertices, s->dNormals, s->dTris, occ ? s->dOccTris : nullptr, ord ? s->dOrdTris : nullptr,
                    emiTris && r->emiRecords ? s->dEmiTris : nullptr, r->dSlotOf, s->numPrims };
    hipLaunchKernelGGL(k_scatter, dim3(blocks_for((size_t)m)), dim3(256), 0, st, sa, m, dIds, dVertices, dNormals);
    hipLaunchKernelGGL(k_ref_leaves, dim3(blocks_for(np)), dim3(256), 0, st, s->numPrims, (const float*)s->dVertices, (const int*)r->dLeafOf,
                       (const int*)r->dParent, r->dKeys, r->dArrived);
    const size_t refRecords = (occ ? 7 : 6) * nn;
    hipLaunchKernelGGL(k_ref_write, dim3(blocks_for(refRecords)), dim3(256), 0, st, refRecords, nn, (const int*)r->dBoxId, (const unsigned*)r->dKeys,
                       s->dNodesAll, s->dOccChain);
    const size_t emiFirst = r->occRecords + 6 * r->ordRecords, gridRecords = emiFirst + emiRecords;
    if (gridRecords) {
        const GridArgs ga = grid_args(s, r);
        hipLaunchKernelGGL(k_grid_leaves, dim3(blocks_for(gridRecords)), dim3(256), 0, st, ga, gridRecords, (const int*)r->dParent, r->dKeys, r->dArrived);
        hipLaunchKernelGGL(k_grid_write, dim3(blocks_for(gridRecords)), dim3(256), 0, st, ga, gridRecords, (const int*)r->dParent, (const unsigned*)r->dKeys);
    }
    return rs_check_hip(hipGetLastError(), "rs_scene_set_triangles: refit kernels");
}
