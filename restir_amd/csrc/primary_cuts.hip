// primary_cuts.hip -- the cuts and leaf lists of still-camera primary rays (rs_cuts.h says what they are and why no bit changes): the
// slots' lifetime (rs_primary_cut, rs_internal.h), the build and its two kernels, the containment test kernels, and every entry point of
// include/restir_hip.h that names them.  The host decisions -- key, slot state, arena sizes -- are rs_cut_plan.h's; restir.hip
// phase_a_impl reaches this unit through the rs_primary_cuts_* calls below and hands the PrimaryCuts it gets to k_primary / k_primary_split.
#include <cstdlib>

#include "rs_internal.h"
#include "rs_cuts.h"

using namespace rs;

namespace {

// ---- the builders ---------------------------------------------------------------------------------------------------------------------
// One thread per cell (a block's cut) or tile (its leaf list): the walk that counts, a reservation in the arena, then write(off, count) --
// the same walk again, writing -- and the entry { first record, count | order << 28 }.  ok: the cell has an order and the scene the tables
// this kind of cut needs.  counters (64-bit: a large cap times many cells must not wrap): [0] records handed out, [1] cells without a
// cut, [2] records of the cells that have one.
template <bool LEAVES, class Write>
__device__ void build_cell(const DevScene& s, CutCell& cell, bool ok, unsigned cap, unsigned capacity, uint2* entry, unsigned long long* counters, Write write) {
    const unsigned end = (unsigned)s.bvhSize;
    const BvhNode* nodes = s.nodesAll + (size_t)(cell.order < 0 ? 0 : cell.order) * (size_t)s.bvhSize;
    ok = ok && cell.order >= 0 && end > 0u && cut_cell_margin(cell, nodes[0]);
    unsigned count = 0;
    if (ok) {
        count = cut_walk<LEAVES>(cell, [&](unsigned i) { return nodes[i]; }, end, cap, [](unsigned, unsigned, const BvhNode&) {});
        ok = count > 0u && count <= cap;
    }
    // (space is handed out in the order the cells ask: which cells go without when the arena is too small depends on that order --
    // the results never do)
    unsigned off = 0;
    if (ok) {
        const unsigned long long at = atomicAdd(counters, (unsigned long long)count);
        ok = at + count <= (unsigned long long)capacity;
        off = ok ? (unsigned)at : 0u;
    }
    if (!ok) { *entry = make_uint2(0u, 0u); atomicAdd(counters + 1, 1ull); return; }
    write(nodes, end, off, count);
    *entry = make_uint2(off, count | ((unsigned)cell.order << 28));
    atomicAdd(counters + 2, (unsigned long long)count);
}

// a block's cut: the kept records in nodesAll's format, then their links.  orig[]: the original index of every cut record (the links'
// binary search; rs_debug_primary_cut_missing)
__global__ void __launch_bounds__(64) k_build_primary_cuts(DevScene s, CamParams cam, int y0, int cellsX, int numCells, int cellW, int cellH, unsigned cap, unsigned capacity,
                                                           uint2* cells, BvhNode* records, unsigned* orig, unsigned long long* counters) {
    const int ci = blockIdx.x * blockDim.x + threadIdx.x;
    if (ci >= numCells) return;
    CutCell cell = cut_cell(cam, (ci % cellsX) * cellW, y0 + (ci / cellsX) * cellH, cellW, cellH);
    build_cell<false>(s, cell, s.axisCull && s.linksNested, cap, capacity, cells + ci, counters, [&](const BvhNode* nodes, unsigned end, unsigned off, unsigned count) {
        cut_walk<false>(cell, [&](unsigned i) { return nodes[i]; }, end, count, [&](unsigned k, unsigned at, const BvhNode& n) { records[off + k] = n; orig[off + k] = at; }, count);
        cut_relink([&](unsigned j) { return orig[off + j]; }, [&](unsigned i) { return (unsigned)records[off + i].next; }, count,
                   [&](unsigned i, unsigned to) { records[off + i].next = (int)to; });
    });
}

// a tile's leaf list: box and triangle side by side (LeafListRef, rs_walk.h).  leafOfPrim: the reference node of every primitive's leaf
__global__ void __launch_bounds__(64) k_build_primary_leaf_lists(DevScene s, CamParams cam, int y0, int tilesPerRow, int numTiles, unsigned cap, unsigned capacity,
                                                                 const int* leafOfPrim, uint2* tiles, float4* records, int* leafOf, unsigned long long* counters) {
    const int ti = blockIdx.x * blockDim.x + threadIdx.x;
    if (ti >= numTiles) return;
    CutCell cell = cut_cell(cam, (ti % tilesPerRow) * 8, y0 + (ti / tilesPerRow) * 8, 8, 8);
    build_cell<true>(s, cell, s.axisCull && s.linksNested && s.occChain && s.occNested, cap, capacity, tiles + ti, counters, [&](const BvhNode* nodes, unsigned end, unsigned off, unsigned count) {
        cut_walk<true>(cell, [&](unsigned i) { return nodes[i]; }, end, count, [&](unsigned k, unsigned, const BvhNode& n) {
            const float4* tp = reinterpret_cast<const float4*>(s.tris + n.primId);
            const float4 a = tp[0], b = tp[1], e = tp[2];
            float4* r = records + (size_t)(off + k) * 4u;
            r[0] = make_float4(n.bminx, n.bminy, n.bminz, n.bmaxz);
            r[1] = make_float4(n.bmaxx, n.bmaxy, __int_as_float(n.primId), a.x);
            r[2] = make_float4(a.y, a.z, b.x, b.y);
            r[3] = make_float4(b.z, e.x, e.y, e.z);
            leafOf[off + k] = leafOfPrim[n.primId];
        }, count);
    });
}

// ---- containment, ray by ray ----------------------------------------------------------------------------------------------------------
// The ray { pixel x, pixel y, jitter x, jitter y } of r[0..4) walks the WHOLE tree of its order on the geometric part of the reference's
// test alone (no distance cull): passed(record index, primitive) for every node it passes.  false, and no walk: the ray is left out
// (special-case direction, another order than the entry word's, an entry without records).
template <class Passed>
__device__ bool containment_walk(const DevScene& s, const CamParams& cam, const float* r, unsigned word, Passed passed) {
    const Ray ray = camera_sample(cam, (int)r[0], (int)r[1], r[2], r[3]);
    RayBoxCtx ctx = make_box_ctx(ray);
    ctx.cull = s.axisCull;
    const int order = mtbvh_order(-ray.d);
    if (ray_is_special(ctx, ray) || (word & kCutCountMask) == 0u || order != (int)(word >> 28)) return false;
    const BvhNode* nodes = s.nodesAll + (size_t)order * (size_t)s.bvhSize;
    for (unsigned cur = 0; cur != (unsigned)s.bvhSize;) {
        const float4* rec = reinterpret_cast<const float4*>(nodes + cur);
        float4 lo, hi;
        node_unpack(rec[0], rec[1], lo, hi);
        float tb;
        if (box_hit_general(ctx.o, ctx.dinv, lo, hi, tb)) { passed(cur, __float_as_int(lo.w)); cur++; }
        else cur = (unsigned)__float_as_int(hi.w);
    }
    return true;
}

// each node a ray passes is looked up in block cellIndex's cut.  out: [0] passed nodes absent from the cut, [1] passed nodes, [2] rays
// left out (containment_walk, or a cell without a cut), [3] records in the cell's cut
__global__ void k_primary_cut_missing(DevScene s, CamParams cam, PrimaryCuts cuts, const unsigned* orig, int cellIndex, int n, const float* rays, unsigned long long* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint2 entry = cuts.cells[cellIndex];
    const unsigned off = entry.x, count = entry.y & kCutCountMask;
    if (i == 0) out[3] = count;
    unsigned long long passed = 0, missing = 0;
    const bool walked = containment_walk(s, cam, rays + 4 * i, entry.y, [&](unsigned cur, int) {
        unsigned a = 0, b = count;
        while (a < b) { const unsigned mid = (a + b) >> 1; if (orig[off + mid] < cur) a = mid + 1u; else b = mid; }
        passed++;
        if (a == count || orig[off + a] != cur) missing++;
    });
    if (!walked) { atomicAdd(out + 2, 1ull); return; }
    atomicAdd(out, missing); atomicAdd(out + 1, passed);
}

// each LEAF a ray passes is looked up in the list of the ray's own tile.  out: [0] passed leaves absent from the list, [1] passed leaves,
// [2] rays left out (containment_walk, a pixel outside the launch, a tile without a list)
__global__ void k_primary_leaf_list_missing(DevScene s, CamParams cam, PrimaryCuts cuts, int y0, int tilesPerRow, int numTiles, int n, const float* rays, unsigned long long* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int px = (int)rays[4 * i], py = (int)rays[4 * i + 1];
    const int tile = py >= y0 && px >= 0 ? ((py - y0) / 8) * tilesPerRow + px / 8 : -1;
    if (tile < 0 || tile >= numTiles || px / 8 >= tilesPerRow) { atomicAdd(out + 2, 1ull); return; }
    const uint2 entry = cuts.tiles[tile];
    const unsigned count = entry.y & kCutCountMask;
    const float4* list = cuts.leafRecords + (size_t)entry.x * 4u;
    unsigned long long passed = 0, missing = 0;
    unsigned at = 0;                                        // the list is in the walk's order: the search never goes back
    const bool walked = containment_walk(s, cam, rays + 4 * i, entry.y, [&](unsigned, int prim) {
        if (prim == kNullPrim) return;
        passed++;
        unsigned j = at;
        while (j < count && __float_as_int(list[(size_t)j * 4u + 1u].z) != prim) j++;
        if (j == count) missing++; else at = j + 1u;
    });
    if (!walked) { atomicAdd(out + 2, 1ull); return; }
    atomicAdd(out, missing); atomicAdd(out + 1, passed);
}

// ---- a slot's arenas ------------------------------------------------------------------------------------------------------------------
void list_free(rs_primary_cut& pc) {
    rs_dev_free(pc.tiles); rs_dev_free(pc.leafRecords); rs_dev_free(pc.leafOf);
    pc.tiles = nullptr; pc.leafRecords = nullptr; pc.leafOf = nullptr;
    pc.size.numTiles = 0; pc.size.listCapacity = 0;
    if (pc.slot.lists == RS_CUT_ARENA_BUILT) pc.slot.lists = RS_CUT_ARENA_NOTHING;
}

void cut_free(rs_primary_cut& pc) {
    rs_dev_free(pc.cells); rs_dev_free(pc.records); rs_dev_free(pc.orig); rs_dev_free(pc.counters);
    pc.cells = nullptr; pc.records = nullptr; pc.orig = nullptr; pc.counters = nullptr;
    pc.size.numCells = 0; pc.size.capacity = 0;
    if (pc.slot.cuts == RS_CUT_ARENA_BUILT) pc.slot.cuts = RS_CUT_ARENA_NOTHING;
    list_free(pc);
}

bool cuts_built(const rs_primary_cut& pc) { return pc.slot.cuts == RS_CUT_ARENA_BUILT; }
bool lists_built(const rs_primary_cut& pc) { return cuts_built(pc) && pc.slot.lists == RS_CUT_ARENA_BUILT; }
PrimaryCuts view_of(const rs_primary_cut& pc, bool lists) {
    return lists ? PrimaryCuts{ pc.cells, pc.records, pc.tiles, pc.leafRecords, pc.leafOf } : PrimaryCuts{ pc.cells, pc.records, nullptr, nullptr, nullptr };
}

// the _info hooks: entries of the launch, entries that went without, records in all the others -- counters[at ..]; waits for the build
int read_info(const rs_primary_cut& pc, bool built, int entries, int at, int* total, int* without, unsigned long long* records) {
    *total = 0; *without = 0; *records = 0;
    if (!built) return 0;
    RS_HIP(hipEventSynchronize(pc.builtEv));
    unsigned long long h[4];
    RS_HIP(hipMemcpy(h, pc.counters + at, sizeof h, hipMemcpyDeviceToHost));
    *total = entries; *without = (int)h[1]; *records = h[2];
    return 0;
}

// the _missing hooks: the rays go up, launch(device rays, device out[4]) runs on the library stream behind the build, out comes down
template <class Launch>
int run_missing(const rs_primary_cut& pc, const char* name, int n, const float* rays, unsigned long long out[4], Launch launch) {
    RS_HIP(hipEventSynchronize(pc.builtEv));
    float* dRays = nullptr; unsigned long long* dOut = nullptr;
    RS_TRY(rs_dev_alloc(&dRays, (size_t)n * 4));
    int e = rs_dev_alloc(&dOut, 4);
    if (!e) e = rs_check_hip(hipMemcpy(dRays, rays, (size_t)n * 16, hipMemcpyHostToDevice), "hipMemcpy");
    if (!e) e = rs_check_hip(hipMemset(dOut, 0, 32), "hipMemset");
    if (!e) {
        launch(dRays, dOut);
        e = rs_check_hip(hipStreamSynchronize(rs_stream()), name);
    }
    if (!e) e = rs_check_hip(hipMemcpy(out, dOut, 32, hipMemcpyDeviceToHost), "hipMemcpy");
    rs_dev_free(dRays); rs_dev_free(dOut);
    return e;
}

// the host hooks: the cut (LEAVES: the leaf list) of the w x h pixels at (x0, y0) over rs_build_bvh's tables, by the builders' walk
template <bool LEAVES>
int plan_cell(const rs_camera* cam, int x0, int y0, int w, int h, int bvhSize, const float* boundingBoxes, const int* const bvhNodes[6], int cap,
              int* order, int* count, int* positions, int* links) {
    *order = -1; *count = 0;
    CutCell cell = cut_cell(rs_make_cam_params(cam), x0, y0, w, h);
    if (cell.order < 0 || !bvhNodes[cell.order]) return 0;
    const int* table = bvhNodes[cell.order];
    auto rec = [&](unsigned i) { const int* n = table + (size_t)i * 3; const float* b = boundingBoxes + (size_t)n[1] * 6; return BvhNode{ b[0], b[1], b[2], b[5], b[3], b[4], n[0], n[2] }; };
    if (!cut_cell_margin(cell, rec(0))) return 0;
    *order = cell.order;
    *count = (int)cut_walk<LEAVES>(cell, rec, (unsigned)bvhSize, (unsigned)cap, [&](unsigned k, unsigned at, const BvhNode&) { positions[k] = (int)at; });
    if (links && *count <= cap)
        cut_relink([&](unsigned j) { return (unsigned)positions[j]; }, [&](unsigned i) { return (unsigned)table[(size_t)positions[i] * 3 + 2]; }, (unsigned)*count,
                   [&](unsigned i, unsigned to) { links[i] = (int)to; });
    return 0;
}

}  // namespace

// ---- what phase_a_impl asks (rs_internal.h) -------------------------------------------------------------------------------------------
void rs_primary_cuts_init(rs_primary_cuts& c) {
    if (const char* env = std::getenv("RS_PRIMARY_CUTS")) c.on = std::atoi(env) != 0;     // A/B switch for measurements: the default of rs_restir_set_primary_cuts
    if (const char* env = std::getenv("RS_PRIMARY_LEAF_LISTS")) c.listsOn = std::atoi(env) != 0;     // the same for rs_restir_set_primary_leaf_lists
}

int rs_primary_cuts_begin(rs_primary_cuts& c, int call, const rs_scene* scene, const rs_camera* cam, int y0, int y1) {
    c.last = call < 2 ? call : 2;
    c.lastUsed = c.lastListsUsed = false;
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(rs_stream(), &capturing) != hipSuccess) { (void)hipGetLastError(); capturing = hipStreamCaptureStatusNone; }
    rs_primary_cut_key key{ scene->id, scene->geomEdits, *cam, y0, y1, c.cap, c.listsOn ? c.listCap : 0u };          // (lists off: cap 0, no tile takes one)
    return rs_plan_cut_slot(c.on, capturing != hipStreamCaptureStatusNone, c.slot[c.last].slot, key);
}

int rs_primary_cuts_view(rs_primary_cuts& c, hipStream_t st, PrimaryCuts* out) {
    const rs_primary_cut& pc = c.slot[c.last];
    RS_HIP(hipStreamWaitEvent(st, pc.builtEv, 0));          // after the build, wherever it was enqueued
    *out = view_of(pc, lists_built(pc));
    c.lastUsed = true; c.lastListsUsed = out->tiles != nullptr;
    return 0;
}

int rs_primary_cuts_launched(rs_primary_cuts& c, int k, hipStream_t st) {          // a later build into this arena waits for this reader
    rs_primary_cut& pc = c.slot[c.last];
    if (!pc.usedEv[k]) RS_HIP(hipEventCreateWithFlags(&pc.usedEv[k], hipEventDisableTiming));
    RS_HIP(hipEventRecord(pc.usedEv[k], st));
    pc.usedValid[k] = true;
    return 0;
}

// enqueues the build of the slot's cuts on st: after every launch that still reads the arena, before every launch that waits for builtEv
int rs_primary_cuts_build(rs_primary_cuts& c, const rs_scene* scene, const CamParams& cp, int y0, int tilesX, int tilesY, hipStream_t st) {
    rs_primary_cut& pc = c.slot[c.last];
    const rs_primary_cut_key& key = pc.slot.key;
    const rs_primary_cut_sizes z = rs_plan_cut_sizes(tilesX, tilesY, key.cap, key.listCap);
    if (z.numCells != pc.size.numCells || z.capacity != pc.size.capacity) {      // another launch geometry (hipFree waits for the device: nothing reads the old arena)
        cut_free(pc);
        int e = rs_dev_alloc(&pc.cells, (size_t)z.numCells);
        if (!e) e = rs_dev_alloc(&pc.records, (size_t)z.capacity + 1);
        if (!e) e = rs_dev_alloc(&pc.orig, (size_t)z.capacity + 1);
        if (!e) e = rs_dev_alloc(&pc.counters, 8);
        if (e) {                                             // no memory for the arena: this key renders through the tree, as the frames before it did
            (void)hipGetLastError();
            cut_free(pc);
            pc.slot.cuts = RS_CUT_ARENA_NO_MEMORY;
            return 0;
        }
        pc.size.numCells = z.numCells; pc.size.capacity = z.capacity;
        for (bool& v : pc.usedValid) v = false;
    }
    // the tiles' leaf lists: an arena of their own; without memory, or on a scene without the chain records, the launches keep the cuts alone
    bool lists = z.numTiles > 0 && scene->dLeafOfPrim && scene->dev.occChain && scene->dev.occNested && pc.slot.lists != RS_CUT_ARENA_NO_MEMORY;
    if (lists && (z.numTiles != pc.size.numTiles || z.listCapacity != pc.size.listCapacity)) {
        list_free(pc);
        int e = rs_dev_alloc(&pc.tiles, (size_t)z.numTiles);
        if (!e) e = rs_dev_alloc(&pc.leafRecords, ((size_t)z.listCapacity + 1) * 4);
        if (!e) e = rs_dev_alloc(&pc.leafOf, (size_t)z.listCapacity + 1);
        if (e) { (void)hipGetLastError(); list_free(pc); pc.slot.lists = RS_CUT_ARENA_NO_MEMORY; lists = false; }
        else { pc.size.numTiles = z.numTiles; pc.size.listCapacity = z.listCapacity; }
    }
    if (!lists && pc.slot.lists == RS_CUT_ARENA_BUILT) pc.slot.lists = RS_CUT_ARENA_NOTHING;
    pc.tilesPerRow = tilesX * 4;
    if (!pc.builtEv) RS_HIP(hipEventCreateWithFlags(&pc.builtEv, hipEventDisableTiming));
    for (int i = 0; i < 1 + rs_context::kAux; i++) if (pc.usedValid[i]) { RS_HIP(hipStreamWaitEvent(st, pc.usedEv[i], 0)); pc.usedValid[i] = false; }
    RS_HIP(hipMemsetAsync(pc.counters, 0, 8 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_build_primary_cuts, dim3((z.numCells + 63) / 64), dim3(64), 0, st, scene->dev, cp, y0, tilesX, z.numCells, 32, 8, key.cap, z.capacity,
                       pc.cells, pc.records, pc.orig, pc.counters);
    if (lists) {
        hipLaunchKernelGGL(k_build_primary_leaf_lists, dim3((z.numTiles + 63) / 64), dim3(64), 0, st, scene->dev, cp, y0, pc.tilesPerRow, z.numTiles, key.listCap, z.listCapacity,
                           scene->dLeafOfPrim, pc.tiles, pc.leafRecords, pc.leafOf, pc.counters + 4);
        pc.slot.lists = RS_CUT_ARENA_BUILT; pc.listBuilds++;
    }
    RS_HIP(hipEventRecord(pc.builtEv, st));
    pc.slot.cuts = RS_CUT_ARENA_BUILT; pc.builds++;
    return 0;
}

void rs_primary_cuts_destroy(rs_primary_cuts& c) {
    for (rs_primary_cut& pc : c.slot) {
        cut_free(pc);
        if (pc.builtEv) (void)hipEventDestroy(pc.builtEv);
        for (hipEvent_t& e : pc.usedEv) if (e) (void)hipEventDestroy(e);
    }
}

// ---- entry points (include/restir_hip.h) ----------------------------------------------------------------------------------------------
extern "C" {

// Primary cuts (rs_cuts.h): 1 on (the default; RS_PRIMARY_CUTS=0 makes 0 the default), 0 off -- the cuts are forgotten, their memory stays
int rs_restir_set_primary_cuts(rs_restir* r, int on) {
    RS_SCOPE(r);
    if (!r) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_restir_set_primary_cuts: null");
    r->cuts.on = on != 0;
    if (!r->cuts.on) for (rs_primary_cut& pc : r->cuts.slot) rs_cut_slot_forget(pc.slot);
    return 0;
}

// test hook: the most records a cell's cut may have (1 .. 2^24; the default is 4096); cuts built under another cap are forgotten
int rs_debug_set_primary_cut_cap(rs_restir* r, int records) {
    RS_SCOPE(r);
    if (!r || records < 1 || records > (1 << 24)) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_set_primary_cut_cap: bad argument");
    r->cuts.cap = (unsigned)records;
    return 0;
}

// of the last phase-A call's slot: cells of its launch, cells without a cut, records in all cuts (zeros while nothing is built), whether
// that call's primary rays walked the cuts, and how many builds the slot has seen.  Waits for the build.
int rs_debug_primary_cut_info(rs_restir* r, int* cells, int* cellsWithoutCut, unsigned long long* records, int* usedLastFrame, unsigned long long* builds) {
    RS_SCOPE(r);
    if (!r || !cells || !cellsWithoutCut || !records || !usedLastFrame || !builds) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_primary_cut_info: null argument");
    const rs_primary_cut& pc = r->cuts.slot[r->cuts.last];
    *usedLastFrame = r->cuts.lastUsed ? 1 : 0; *builds = pc.builds;
    return read_info(pc, cuts_built(pc), pc.size.numCells, 0, cells, cellsWithoutCut, records);
}

// test hook: containment of the last phase-A call's cuts, ray by ray (k_primary_cut_missing).  rays: n x { pixel x, pixel y, jitter x,
// jitter y } on the host; the camera is the one the cut was built for.  out[4]: nodes a ray passes geometrically that the cell's cut
// lacks, nodes passed, rays left out (special-case direction, another order than the cut's, no cut), records in the cell's cut.
int rs_debug_primary_cut_missing(rs_restir* r, const rs_scene* scene, int cell, int n, const float* rays, unsigned long long out[4]) {
    RS_SCOPE(r);
    if (!r || !scene || !rays || !out || n <= 0) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_primary_cut_missing: bad argument");
    const rs_primary_cut& pc = r->cuts.slot[r->cuts.last];
    if (!cuts_built(pc) || scene->id != pc.slot.key.sceneId || scene->geomEdits != pc.slot.key.geomEdits) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_primary_cut_missing: no cut has been built for this scene");
    if (cell < 0 || cell >= pc.size.numCells) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_primary_cut_missing: no such cell");
    return run_missing(pc, "rs_debug_primary_cut_missing", n, rays, out, [&](const float* dRays, unsigned long long* dOut) {
        hipLaunchKernelGGL(k_primary_cut_missing, dim3((n + 63) / 64), dim3(64), 0, rs_stream(), scene->dev, rs_make_cam_params(&pc.slot.key.cam), view_of(pc, false), pc.orig, cell, n, dRays, dOut);
    });
}

// Primary leaf lists (rs_cuts.h "Leaf lists"): 1 on (the default; RS_PRIMARY_LEAF_LISTS=0 makes 0 the default), 0 off -- whole tiles walk
// their block's cut again.  The lists live and die with the cuts (rs_restir_set_primary_cuts off: no lists either); a change here forgets both.
int rs_restir_set_primary_leaf_lists(rs_restir* r, int on) {
    RS_SCOPE(r);
    if (!r) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_restir_set_primary_leaf_lists: null");
    r->cuts.listsOn = on != 0;
    return 0;
}

// test hook: the most records a tile's leaf list may have (0 .. 2^24; the default is 192; 0: no tile takes a list); lists and cuts built
// under another cap are forgotten
int rs_debug_set_primary_leaf_list_cap(rs_restir* r, int records) {
    RS_SCOPE(r);
    if (!r || records < 0 || records > (1 << 24)) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_set_primary_leaf_list_cap: bad argument");
    r->cuts.listCap = (unsigned)records;
    return 0;
}

// of the last phase-A call's slot: tiles of its launch, tiles without a list, records in all lists (zeros while nothing is built), whether
// that call's primary rays walked lists, and how many list builds the slot has seen.  Waits for the build.
int rs_debug_primary_leaf_list_info(rs_restir* r, int* tiles, int* tilesWithoutList, unsigned long long* records, int* usedLastFrame, unsigned long long* builds) {
    RS_SCOPE(r);
    if (!r || !tiles || !tilesWithoutList || !records || !usedLastFrame || !builds) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_primary_leaf_list_info: null argument");
    const rs_primary_cut& pc = r->cuts.slot[r->cuts.last];
    *usedLastFrame = r->cuts.lastListsUsed ? 1 : 0; *builds = pc.listBuilds;
    return read_info(pc, lists_built(pc), pc.size.numTiles, 4, tiles, tilesWithoutList, records);
}

// test hook: containment of the last phase-A call's leaf lists, ray by ray (k_primary_leaf_list_missing).  rays as for
// rs_debug_primary_cut_missing; every ray is looked up in its own tile's list.  out[4]: leaves a ray passes geometrically that its
// tile's list lacks, leaves passed, rays left out (special-case direction, another order than the list's, a tile without a list), 0.
int rs_debug_primary_leaf_list_missing(rs_restir* r, const rs_scene* scene, int n, const float* rays, unsigned long long out[4]) {
    RS_SCOPE(r);
    if (!r || !scene || !rays || !out || n <= 0) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_primary_leaf_list_missing: bad argument");
    const rs_primary_cut& pc = r->cuts.slot[r->cuts.last];
    if (!lists_built(pc) || scene->id != pc.slot.key.sceneId || scene->geomEdits != pc.slot.key.geomEdits)
        return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_primary_leaf_list_missing: no lists have been built for this scene");
    return run_missing(pc, "rs_debug_primary_leaf_list_missing", n, rays, out, [&](const float* dRays, unsigned long long* dOut) {
        hipLaunchKernelGGL(k_primary_leaf_list_missing, dim3((n + 63) / 64), dim3(64), 0, rs_stream(), scene->dev, rs_make_cam_params(&pc.slot.key.cam), view_of(pc, true),
                           pc.slot.key.y0, pc.tilesPerRow, pc.size.numTiles, n, dRays, dOut);
    });
}

// test hooks, host only (no device call): the leaf list the builder would make for the 8x8 tile at pixel (x0, y0) of `cam`, and the node
// cut it would make for the w x h cell there, over a reference table (rs_build_bvh's outputs).  *order: the threaded order (-1: cut_cell
// gives none, nothing else is written); *count: the records, or cap + 1 if there are more than `cap`; positions[0 .. min(*count, cap)):
// their record indices in that order's table, in cut order; links[0 .. *count) (*count <= cap): the cut's miss links.  cut_walk and
// cut_relink of rs_cuts.h, the functions the device builders run.
int rs_debug_plan_primary_leaf_list(const rs_camera* cam, int x0, int y0, int bvhSize, const float* boundingBoxes, const int* const bvhNodes[6], int cap,
                                    int* order, int* count, int* positions) {
    if (!cam || !boundingBoxes || !bvhNodes || !order || !count || !positions || bvhSize <= 0 || cap < 0) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_plan_primary_leaf_list: bad argument");
    return plan_cell<true>(cam, x0, y0, 8, 8, bvhSize, boundingBoxes, bvhNodes, cap, order, count, positions, nullptr);
}

int rs_debug_plan_primary_cut(const rs_camera* cam, int x0, int y0, int w, int h, int bvhSize, const float* boundingBoxes, const int* const bvhNodes[6], int cap,
                              int* order, int* count, int* positions, int* links) {
    if (!cam || !boundingBoxes || !bvhNodes || !order || !count || !positions || !links || bvhSize <= 0 || cap < 0 || w <= 0 || h <= 0)
        return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_plan_primary_cut: bad argument");
    return plan_cell<false>(cam, x0, y0, w, h, bvhSize, boundingBoxes, bvhNodes, cap, order, count, positions, links);
}

// test hook, host only: rs_cut_plan.h's two functions for inputs the caller fills in: no device, no context, no object
int rs_debug_plan_primary_cut_slot(int on, int capturing, rs_primary_cut_slot* slot, const rs_primary_cut_key* key, int tilesX, int tilesY, int* cutState, rs_primary_cut_sizes* sizes) {
    if (!slot || !key || !cutState || !sizes || tilesX < 0 || tilesY < 0) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_plan_primary_cut_slot: bad argument");
    *cutState = rs_plan_cut_slot(on != 0, capturing != 0, *slot, *key);
    *sizes = rs_plan_cut_sizes(tilesX, tilesY, key->cap, key->listCap);
    return 0;
}

}  // extern "C"
