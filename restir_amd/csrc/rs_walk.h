// rs_walk.h -- the BVH walks and the per-ray services the kernels call (trace_closest*, trace_occluded_wave, may_hit_emissive_wave).
// Device only.  The walks are built from pieces that each hide a record format or a numeric argument which must be the same in every
// walk: the pair fetch, GridRay (slab test of a 16-byte grid node), root_extent, chain_step (the reference's test along occChain),
// LeafQueue, hit_of_walk, shadow_ray.  Every walk returns the reference's bits; profiles/walk_pieces_ab.log compares this form with the
// copies it replaced.
#pragma once

#include "rs_intersect.h"

#if defined(__HIPCC__)
#ifndef RS_WALK_WAVES
#define RS_WALK_WAVES 8        // waves per SIMD the walk kernels are held to (launch bound; holding them to exactly that many was A/B'd in round 3: no gain)
#endif

namespace rs {

typedef float vf2 __attribute__((ext_vector_type(2)));     // operands of the packed FP32 instructions (v_pk_add / mul / fma_f32)

// ---- traversal ---------------------------------------------------------------------------------
// All six threaded orders live in ONE array (order k at records [k*bvhSize, (k+1)*bvhSize), one padding
// record at the very end), so a lane addresses its node with a 32-bit byte offset from a wave-uniform
// base: the loads compile to `global_load_dwordx4 v, v_off, s[base]` (no 64-bit address arithmetic),
// and the two possible successors of a node can be prefetched before its box test has finished:
//   * entered  -> the next record in memory (pre-order layout: first child / next sibling)
//   * rejected -> nextNodeIfMiss, which is part of the record just loaded
// Both are requested at the top of the step, so the ~40-instruction slab test of node n overlaps the
// memory latency of node n+1 whichever way the test goes.  The walk itself is unchanged: same nodes,
// same order, same arithmetic as DevScene::intersect / testOcclusion (src/scene.h:245-316).

__device__ __forceinline__ float4 ld16(const char* base, unsigned off) {
    return *reinterpret_cast<const float4*>(base + off);
}
// the two 16-byte halves of a BvhNode as loaded -> lo = {min.xyz, bits(primId)}, hi = {max.xyz, bits(next)}
__device__ __forceinline__ void node_unpack(const float4& ra, const float4& rb, float4& lo, float4& hi) {
    lo = make_float4(ra.x, ra.y, ra.z, rb.z);
    hi = make_float4(rb.x, rb.y, ra.w, rb.w);
}

__device__ __forceinline__ void load_tri(const TriRec* tris, int prim, f3& v0, f3& e1, f3& e2) {
    const float4* p = reinterpret_cast<const float4*>(tris + prim);
    float4 a = p[0], b = p[1], c = p[2];
    v0 = mk3(a.x, a.y, a.z); e1 = mk3(b.x, b.y, b.z); e2 = mk3(c.x, c.y, c.z);
}

struct WalkResult {
    float closest = 3.402823466e+38f;      // FLT_MAX
    int prim = kNullPrim;
    float bx = 0.f, by = 0.f;
    unsigned nodes = 0;        // packet walks: nodes the WAVE visited (the union of its lanes' walks), wave-uniform
#ifdef RS_WALK_STATS
    unsigned steps, nearSteps, enteredSteps, leafSteps, clearSteps;   // clearSteps: entered without evaluating the overlap part
    unsigned myVisits;                                                // nodes this lane's own walk visited (packet walks)
    unsigned chainSteps, listSteps;                                   // leaf lists: wave steps up occChain, records walked
#endif
};

// One per-lane MTBVH walk that keeps the closest hit (intersect).  GENERAL: every lane of the wave is a general-case ray.
template <bool GENERAL>
__device__ __forceinline__ WalkResult walk(const DevScene& s, const Ray& ray, const RayBoxCtx& ctx) {
    WalkResult r;
    const char* base = reinterpret_cast<const char*>(s.nodesAll);
    const unsigned first = (unsigned)mtbvh_order(-ray.d) * (unsigned)s.bvhSize * 32u;
    const unsigned endOff = first + (unsigned)s.bvhSize * 32u;
    unsigned cur = first;
    while (cur != endOff) {
        float4 lo, hi;
        node_unpack(ld16(base, cur), ld16(base, cur + 16), lo, hi);
        float tb;
        bool bh;
        if (GENERAL) bh = box_hit_general(ctx.o, ctx.dinv, lo, hi, tb);
        else bh = box_hit(ctx, mk3(lo.x, lo.y, lo.z), mk3(hi.x, hi.y, hi.z), tb);
        if (bh && tb < r.closest) {
            const int prim = __float_as_int(lo.w);
            if (prim != kNullPrim) {
                f3 v0, e1, e2;
                load_tri(s.tris, prim, v0, e1, e2);
                float bx, by, dist;
                if (tri_hit(ray.o, ray.d, v0, e1, e2, bx, by, dist) && dist < r.closest) {
                    r.closest = dist; r.bx = bx; r.by = by; r.prim = prim;
                }
            }
            cur += 32u;
        }
        else {
            cur = first + (unsigned)__float_as_int(hi.w) * 32u;
        }
    }
    return r;
}

// ---- pair-cooperative node fetch for incoherent rays ---------------------------------------------
// Measured on the per-lane walk with shadow rays (profiles/): the L1 can look up one cache line per
// clock, and a wave of incoherent rays touches ~64 different lines in EACH of the two 16-byte loads
// of a step (TD/TA busy 92 %).  Here lanes 2k and 2k+1 fetch together: one load instruction reads
// both halves of the even lane's node (one line), the next both halves of the odd lane's node, and a
// DPP quad-permute hands each lane the half it is missing -- the same 32 bytes per lane, half the
// line look-ups.  Every lane still walks exactly its own node sequence with the same arithmetic.
// Must be called by all 64 lanes (`active` false for lanes without a ray): finished lanes keep
// fetching for their partner.
__device__ __forceinline__ int dpp_swap1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true); }
__device__ __forceinline__ float4 dpp_swap1(float4 v) {
    return make_float4(__int_as_float(dpp_swap1(__float_as_int(v.x))), __int_as_float(dpp_swap1(__float_as_int(v.y))),
                       __int_as_float(dpp_swap1(__float_as_int(v.z))), __int_as_float(dpp_swap1(__float_as_int(v.w))));
}
// the node at byte offset `cur` of this lane, fetched with its pair partner
__device__ __forceinline__ void pair_fetch(const char* base, unsigned cur, float4& lo, float4& hi) {
    const bool odd = (__lane_id() & 1u) != 0;
    const unsigned halfOff = odd ? 16u : 0u;
    const unsigned partner = (unsigned)dpp_swap1((int)cur);
    const float4 r1 = ld16(base, (odd ? partner : cur) + halfOff);      // even lane's node, split over the pair
    const float4 r2 = ld16(base, (odd ? cur : partner) + halfOff);      // odd lane's node
    const float4 s1 = dpp_swap1(r1), s2 = dpp_swap1(r2);
    node_unpack(odd ? s2 : r1, odd ? r2 : s1, lo, hi);
}

template <bool GENERAL>
__device__ __forceinline__ WalkResult walk_paired(const DevScene& s, const Ray& ray, const RayBoxCtx& ctx, bool active) {
    WalkResult r;
    const char* base = reinterpret_cast<const char*>(s.nodesAll);
    const unsigned first = (unsigned)mtbvh_order(-ray.d) * (unsigned)s.bvhSize * 32u;
    const unsigned endOff = first + (unsigned)s.bvhSize * 32u;
    unsigned cur = active ? first : endOff;            // endOff is a readable record (next order / padding)
#ifdef RS_WALK_STATS
    unsigned long long pst[4] = { 1, 0, 0, 0 };
#endif
    while (__any(cur != endOff)) {
#ifdef RS_WALK_STATS
        pst[1]++; pst[2] += __popcll(__ballot(cur != endOff));
#endif
        float4 lo, hi;
        pair_fetch(base, cur, lo, hi);
        if (cur != endOff) {
            float tb;
            bool bh;
            if (GENERAL) bh = box_hit_general(ctx.o, ctx.dinv, lo, hi, tb);
            else bh = box_hit(ctx, mk3(lo.x, lo.y, lo.z), mk3(hi.x, hi.y, hi.z), tb);
            if (bh && tb < r.closest) {
                const int prim = __float_as_int(lo.w);
                cur += 32u;
                if (prim != kNullPrim) {
                    f3 v0, e1, e2;
                    load_tri(s.tris, prim, v0, e1, e2);
                    float bx, by, dist;
                    if (tri_hit(ray.o, ray.d, v0, e1, e2, bx, by, dist) && dist < r.closest) {
                        r.closest = dist; r.bx = bx; r.by = by; r.prim = prim;
                    }
                }
            }
            else {
                cur = first + (unsigned)__float_as_int(hi.w) * 32u;
            }
        }
    }
#ifdef RS_WALK_STATS
    if (s.walkStats && __lane_id() == 0) for (int i = 0; i < 3; i++) atomicAdd(&s.walkStats[80 + i], pst[i]);
#endif
    return r;
}

__device__ __forceinline__ WalkResult walk_dispatch(const DevScene& s, const Ray& ray) {
    RayBoxCtx ctx = make_box_ctx(ray);
    ctx.cull = s.axisCull;
    // the special cases are ~1e-6 of the rays: a wave that has none runs the branch-free test
    if (__any(ray_is_special(ctx, ray))) return walk<false>(s, ray, ctx);
    return walk<true>(s, ray, ctx);
}

// ---- the leaf queue of the walks that defer their leaf tests ------------------------------------------
// Up to four leaf codes per lane in registers, moved by selects (no indexed access, so no scratch).  The shadow-ray walks take the
// NEWEST leaf first (push_lifo: q0 is the newest), the ordered closest-hit walk the OLDEST (push_fifo: q0 is the oldest); pop() takes q0.
constexpr int kLeafQueue = 4;

struct LeafQueue {
    int q0 = 0, q1 = 0, q2 = 0, q3 = 0, n = 0;
    __device__ __forceinline__ void push_lifo(bool push, int code) {
        q3 = push ? q2 : q3; q2 = push ? q1 : q2; q1 = push ? q0 : q1; q0 = push ? code : q0; n = push ? n + 1 : n;
    }
    __device__ __forceinline__ void push_fifo(bool push, int code) {
        q0 = (push && n == 0) ? code : q0; q1 = (push && n == 1) ? code : q1; q2 = (push && n == 2) ? code : q2; q3 = (push && n == 3) ? code : q3;
        n = push ? n + 1 : n;
    }
    __device__ __forceinline__ int pop() {          // n > 0
        const int code = q0;
        q0 = q1; q1 = q2; q2 = q3; n--;
        return code;
    }
};

// ---- any-hit walk with deferred, batched leaf tests ------------------------------------------------
// Measured (profiles/): a vector-memory instruction occupies the return path for ~26 cycles however
// few lanes are active, and in the any-hit walk more than half of all load instructions were the
// three 16-byte triangle loads of a leaf visit, each issued for the one or two lanes that happened to
// sit on a leaf in that step.  testOcclusion only asks whether ANY visited triangle is hit closer than
// the limit, and the walk past a leaf does not depend on that leaf's outcome, so a lane may queue the
// leaf and keep walking.  Queued leaves are tested in rounds in which every lane with a pending leaf
// takes part; a lane that finds a hit is occluded and stops.  The set of triangles tested is the
// reference's set (src/scene.h:286-316) up to its first hit plus possibly a few later ones, so the
// boolean is identical.  Rounds run when a queue is full or when no lane can walk on (A/B: triggering
// earlier, once 12/24/40 lanes wait, was 2-5 % slower).  Node fetches are pair-cooperative as in walk_paired.
template <bool GENERAL>
__device__ __forceinline__ bool walk_anyhit_deferred(const DevScene& s, const Ray& ray, const RayBoxCtx& ctx, float limit, bool active) {
    const char* base = reinterpret_cast<const char*>(s.nodesAll);
    const unsigned first = (unsigned)mtbvh_order(-ray.d) * (unsigned)s.bvhSize * 32u;
    const unsigned endOff = first + (unsigned)s.bvhSize * 32u;
    unsigned cur = active ? first : endOff;
    LeafQueue q;                                       // queued leaf primitives
    bool occluded = false;
    for (;;) {
        const bool walking = cur != endOff;
        const unsigned long long wmask = __ballot(walking);
        const unsigned long long pmask = __ballot(q.n > 0);
        if (!(wmask | pmask)) break;
        const bool round = __any(q.n == kLeafQueue) || wmask == 0;
        if (round) {
            if (q.n > 0) {
                const int prim = q.pop();
                f3 v0, e1, e2;
                load_tri(s.tris, prim, v0, e1, e2);
                float bx, by, dist;
                if (tri_hit(ray.o, ray.d, v0, e1, e2, bx, by, dist) && dist < limit) { occluded = true; cur = endOff; q.n = 0; }
            }
            continue;
        }
        float4 lo, hi;
        pair_fetch(base, cur, lo, hi);
        if (walking) {
            float tb;
            bool bh;
            if (GENERAL) bh = box_hit_general(ctx.o, ctx.dinv, lo, hi, tb);
            else bh = box_hit(ctx, mk3(lo.x, lo.y, lo.z), mk3(hi.x, hi.y, hi.z), tb);
            if (bh && tb < limit) {
                const int prim = __float_as_int(lo.w);
                cur += 32u;
                q.push_lifo(prim != kNullPrim, prim);
            }
            else {
                cur = first + (unsigned)__float_as_int(hi.w) * 32u;
            }
        }
    }
    return occluded;
}

// ---- the pieces of the walks through the trees of 16-byte nodes on a 16-bit grid (occNodes, emiNodes, ordNodes) --------------------
// "Does the ray start within the grid's reach": within 4 grid extents of the scene (the error bound of the grid test, occlusion_bvh.cpp)
__device__ __forceinline__ bool grid_reaches(f3 base, f3 scale, f3 o) {
    const float reach = 4.f * 65535.f;
    return gabs(o.x - base.x) <= reach * scale.x && gabs(o.y - base.y) <= reach * scale.y && gabs(o.z - base.z) <= reach * scale.z;
}

// One ray against the nodes of a grid (plane q on axis c = base.c + q * scale.c).
// slab distance of grid plane q: (base + q*scale - o) / d = q * A + B
// A lane that enters without a ray of its own (outside the frame, a special-case or far-origin ray that takes the reference walk)
// is parked on the sentinel record past the end for the whole walk; it evaluates that record like every other lane, so its
// slab distances must fail the test whatever its ray is: q * 0 + (-1) gives tMax = -1 < 0.  (With its own A and B a ray
// 2^24 grid extents away would absorb q * A in B, pass the empty box and step beyond the allocation.)
// Which of the two grid planes of an axis is the near one depends on the sign of A only (fma is monotone in q): a byte
// permute with a per-ray selector puts {near plane, far plane} of an axis into one dword, and the six min / max of the slab
// test are gone.  Node dwords: x = lo.x | lo.y << 16, y = lo.z | hi.x << 16, z = hi.y | hi.z << 16.
struct GridSlab { float tMin, tMax; };
struct GridRay {
    unsigned selX, selY, selZ;
    vf2 Axy, Bxy, Azz, Bzz;
    __device__ __forceinline__ GridRay(f3 base, f3 scale, const RayBoxCtx& ctx, bool walks) {
        const f3 A = walks ? mk3(scale.x * ctx.dinv.x, scale.y * ctx.dinv.y, scale.z * ctx.dinv.z) : splat(0.f);
        const f3 B = walks ? mk3((base.x - ctx.o.x) * ctx.dinv.x, (base.y - ctx.o.y) * ctx.dinv.y, (base.z - ctx.o.z) * ctx.dinv.z) : splat(-1.f);
        selX = A.x < 0.f ? 0x01000706u : 0x07060100u;      // v_perm_b32(n.y, n.x): bytes 0-3 = n.x, 4-7 = n.y
        selY = A.y < 0.f ? 0x03020504u : 0x05040302u;      // v_perm_b32(n.z, n.x)
        selZ = A.z < 0.f ? 0x01000706u : 0x07060100u;      // v_perm_b32(n.z, n.y)
        Axy = vf2{ A.x, A.y }; Bxy = vf2{ B.x, B.y }; Azz = vf2{ A.z, A.z }; Bzz = vf2{ B.z, B.z };
    }
    __device__ __forceinline__ GridSlab slab(const uint4& n) const {
        const unsigned px = __builtin_amdgcn_perm(n.y, n.x, selX), py = __builtin_amdgcn_perm(n.z, n.x, selY), pz = __builtin_amdgcn_perm(n.z, n.y, selZ);
        const vf2 nearXY = __builtin_elementwise_fma(vf2{ (float)(px & 0xffffu), (float)(py & 0xffffu) }, Axy, Bxy);
        const vf2 farXY = __builtin_elementwise_fma(vf2{ (float)(px >> 16), (float)(py >> 16) }, Axy, Bxy);
        const vf2 zNF = __builtin_elementwise_fma(vf2{ (float)(pz & 0xffffu), (float)(pz >> 16) }, Azz, Bzz);
        GridSlab t;
        t.tMin = fmaxf(fmaxf(nearXY.x, nearXY.y), zNF.x);
        t.tMax = fminf(fminf(farXY.x, farXY.y), zNF.y);
        return t;
    }
};

// largest |slab distance| of a root box: bounds the slab distances of every box inside it (monotone rounding), so it scales the
// margins of chain_step and overlap_margin
__device__ __forceinline__ float root_extent(f3 o, f3 dinv, f3 lo, f3 hi) {
    return fmaxf(fmaxf(fmaxf(gabs((lo.x - o.x) * dinv.x), gabs((hi.x - o.x) * dinv.x)),
                       fmaxf(gabs((lo.y - o.y) * dinv.y), gabs((hi.y - o.y) * dinv.y))),
                 fmaxf(gabs((lo.z - o.z) * dinv.z), gabs((hi.z - o.z) * dinv.z)));
}

// One step of a candidate's verification: the reference's own test (the general case of AABB::intersect) on one record of occChain,
// with tBox < range.  open: the reference enters this box; parent: the record to test next (< 0 at the root).
// clear: the shortcut at the leaf (first record of a chain).  Every ancestor box contains the leaf box
// (checked at scene build), so by monotone rounding its near distances are <= and its far
// distances >= the leaf's: tMax >= 0, tMax >= tMin and tMin < range carry over exactly.  The
// three overlap conditions are, in real arithmetic, fy > nz, fz > nx, fx > ny, and those
// differences can only grow towards the root; evaluated in float they are off by less than
// 2^-20 * tRoot (four roundings of values below 4 * tRoot, tRoot = largest |slab distance| of
// the root box, which bounds every ancestor's).  A leaf that clears them by 2^-18 * tRoot
// therefore settles the whole path; otherwise the ancestors are tested one by one -- and the same
// argument holds from ANY node of the path upwards, so the first ancestor that clears them ends
// the walk (thin leaf boxes in a long scene: a Bistro-class chain took 30 steps to the root).
// The argument needs nested boxes: a caller that has not made DevScene::occNested a precondition combines `clear` with it.
struct ChainStep { bool open, clear; int parent; };
__device__ __forceinline__ ChainStep chain_step(const BvhNode* record, const RayBoxCtx& ctx, float range, float tRoot) {
    const float4* rec = reinterpret_cast<const float4*>(record);
    float4 lo, hi;
    node_unpack(rec[0], rec[1], lo, hi);
    const GeneralSlabs g = general_slabs(ctx.o, ctx.dinv, lo, hi);
    ChainStep c;
    c.open = g.overlap & (g.tMax >= 0.f) & (g.tMax >= g.tMin) & (g.tMin < range);
    c.clear = fminf(fminf(g.fy - g.nz, g.fz - g.nx), g.fx - g.ny) > tRoot * 3.814697265625e-6f;
    c.parent = __float_as_int(lo.w);
    return c;
}

// ---- shadow rays through the second tree ------------------------------------------------------------
// testOcclusion (src/scene.h:286-316) is true iff some triangle T has (a) every node on the reference
// tree's path to T passing the reference's box test with tBox < range and (b) intersectTriangle(T) closer
// than range; the visiting order is irrelevant.  The reference's tree costs 86 node visits per shadow
// ray on the Sponza-class scene (its SAH sweep is not cumulative, src/bvh.cpp:92-100) at 32 bytes each,
// so general-case rays look for triangles with (b) in a well-built tree of 16-byte nodes over the SAME
// leaf boxes (occlusion_bvh.cpp shows why its relaxed slab test cannot miss a triangle whose reference
// leaf box the ray passes) and then evaluate (a) for such a candidate literally: the reference's box test
// on T's leaf and on each of its ancestors (parent links by original node id).  The first candidate that
// passes is what the reference's walk would also have reached and hit -> occluded; if none passes the
// reference reports no occlusion either.
// Three phases alternate until no lane has work left:
//   walk   : cur = byte offset in occNodes; relaxed test on the grid box, branch-free step; leaves are
//            queued (as in walk_anyhit_deferred); ends when a queue is full or all walks have ended
//   leaves : every lane tests the triangles of its newest queued leaf
//   verify : lanes with a candidate run the reference's test along occChain; pass -> occluded,
//            fail -> the lane walks on
// Only for rays that take none of AABB::intersect's special cases (all |d.c| in [1e-6, 1-1e-6]) and start
// within 4 grid extents of the scene (the error bound of the grid test, occlusion_bvh.cpp).
__device__ __forceinline__ bool walk_occlusion_tree(const DevScene& s, const Ray& ray, const RayBoxCtx& ctx, float limit, bool active) {
    const char* nodes = reinterpret_cast<const char*>(s.occNodes);
    const unsigned endOff = (unsigned)s.occCount * 16u;
    const GridRay grid(s.occBase, s.occScale, ctx, active);
    const float tRoot = root_extent(ctx.o, ctx.dinv, s.occRootLo, s.occRootHi);
    unsigned cur = active ? 0u : endOff;
    LeafQueue q;                                                // queued leaf codes
    bool occluded = false;
#ifdef RS_WALK_STATS
    unsigned long long wst[10] = { 1, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    int mySteps = 0, myTris = 0;         // of this lane's ray
#define RS_STAT(i, v) wst[i] += (v)
#else
#define RS_STAT(i, v)
#endif
    for (;;) {
        // walk phase: a tight loop until some lane's leaf queue is full or every walk has ended
        for (;;) {
            const unsigned long long walkers = __ballot(cur != endOff);
            if (!walkers) break;
            RS_STAT(1, 1); RS_STAT(5, 1); RS_STAT(6, __popcll(__ballot(cur != endOff)));
#ifdef RS_WALK_STATS
            if (cur != endOff) mySteps++;
#ifdef RS_WALK_STATS_TIME      // instead of the depth histogram: walking lanes and wave iterations by iteration index (buckets of 24)
            { const unsigned long long walkers = __ballot(cur != endOff);
              if (s.walkStats && __lane_id() == 0) { const int b = wst[5] / 24 < 9 ? (int)(wst[5] / 24) : 9; atomicAdd(&s.walkStats[44 + b], (unsigned long long)__popcll(walkers)); atomicAdd(&s.walkStats[54 + b], 1ull); } }
#endif
#endif
            {   // every lane, also one whose walk has ended: it reads the record past the end, an empty box linked to itself (scene.hip put_end_record)
                const uint4 n = *reinterpret_cast<const uint4*>(nodes + cur);
#if defined(RS_WALK_STATS) && !defined(RS_WALK_STATS_TIME)
                if (s.walkStats && s.occDepth && cur != endOff) { const int dep = s.occDepth[cur >> 4]; atomicAdd(&s.walkStats[44 + (dep < 19 ? dep : 19)], 1ull); }
#endif
                const GridSlab t = grid.slab(n);
                const bool pass = (t.tMax >= fmaxf(t.tMin, 0.f)) && (t.tMin < limit);
                const int meta = (int)n.w;
                const bool leaf = meta < 0;
                q.push_lifo(pass && leaf, ~meta);
                cur = (pass || leaf) ? cur + 16u : (unsigned)meta;
            }
            if (__any(q.n == kLeafQueue)) break;
        }
        if (!__any(q.n > 0)) break;
        // leaf round: every lane takes its newest queued leaf (so no queue is full when the walk resumes) and
        // tests its triangles; a hit becomes a candidate, and the rest of the leaf waits for its verdict
        RS_STAT(2, 1);
        int tri = 0, cnt = 0, verify = -1;
        if (q.n > 0) { const int code = q.pop(); tri = code >> 3; cnt = code & 7; }
        for (;;) {
            while (__any((cnt > 0) & (verify < 0))) {
                RS_STAT(3, 1); RS_STAT(9, __popcll(__ballot((cnt > 0) & (verify < 0))));
                if ((cnt > 0) & (verify < 0)) {
                    const float4* p = reinterpret_cast<const float4*>(s.occTris + tri);
                    const float4 a = p[0], b = p[1], c = p[2];
                    float bx, by, dist;
                    tri++; cnt--;
#ifdef RS_WALK_STATS
                    myTris++;
#endif
                    if (tri_hit(ray.o, ray.d, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z), bx, by, dist) && dist < limit)
                        verify = __float_as_int(a.w);          // reference leaf of the candidate
                }
            }
            if (!__any(verify >= 0)) break;
            // candidates: the reference's own test along the path to the triangle's leaf (normally one step: chain_step)
            while (__any(verify >= 0)) {
                RS_STAT(4, 1); RS_STAT(7, __popcll(__ballot(verify >= 0)));
                if (verify >= 0) {
                    const ChainStep c = chain_step(s.occChain + verify, ctx, limit, tRoot);
                    const bool done = c.open & ((c.parent < 0) | (c.clear & s.occNested));
                    if (done) { occluded = true; cur = endOff; q.n = 0; cnt = 0; }
                    verify = (c.open & !done) ? c.parent : -1;          // closed: the reference never reaches the triangle
                }
            }
        }
    }
#ifdef RS_WALK_STATS
    if (s.walkStats && __lane_id() == 0) for (int i = 0; i < 10; i++) atomicAdd(&s.walkStats[i], wst[i]);
    if (s.walkStats && active) {        // per ray: [10] occluded rays, [11] their steps, [12] unoccluded rays, [13] their steps, [14] triangle tests of all
        atomicAdd(&s.walkStats[occluded ? 10 : 12], 1ull); atomicAdd(&s.walkStats[occluded ? 11 : 13], (unsigned long long)mySteps);
        atomicAdd(&s.walkStats[14], (unsigned long long)myTris);
    }
#endif
#undef RS_STAT
    return occluded;
}

// May the reference's closest hit of this ray be an EMISSIVE triangle?  False only if the ray hits (intersectTriangle) no emissive
// triangle whose reference leaf box it passes -- then DevScene::intersect, which accepts a triangle only on those two conditions, cannot
// return one.  The walk is walk_occlusion_tree's on the tree of the emissive triangles (no range, no verification: any hit answers "maybe");
// special-case and far-origin rays answer "maybe" without walking.  Every lane of the wave must call it.
__device__ __forceinline__ bool may_hit_emissive_wave(const DevScene& s, const Ray& ray, bool active) {
    if (!s.emiState) return active;
    if (s.emiCount == 0) return false;
    RayBoxCtx ctx = make_box_ctx(ray);
    const bool maybe = active && (ray_is_special(ctx, ray) || !grid_reaches(s.emiBase, s.emiScale, ray.o));          // answered without a walk
    const bool walks = active && !maybe;
    const char* nodes = reinterpret_cast<const char*>(s.emiNodes);
    const unsigned endOff = (unsigned)s.emiCount * 16u;
    const GridRay grid(s.emiBase, s.emiScale, ctx, walks);
    unsigned cur = walks ? 0u : endOff;
    LeafQueue q;
    bool found = false;
    for (;;) {
        for (;;) {
            if (!__ballot(cur != endOff)) break;
            const uint4 n = *reinterpret_cast<const uint4*>(nodes + cur);
            const GridSlab t = grid.slab(n);
            const bool pass = t.tMax >= fmaxf(t.tMin, 0.f);
            const int meta = (int)n.w;
            const bool leaf = meta < 0;
            q.push_lifo(pass && leaf, ~meta);
            cur = (pass || leaf) ? cur + 16u : (unsigned)meta;
            if (__any(q.n == kLeafQueue)) break;
        }
        if (!__any(q.n > 0)) break;
        int tri = 0, cnt = 0;
        if (q.n > 0) { const int code = q.pop(); tri = code >> 3; cnt = code & 7; }
        while (__any(cnt > 0)) {
            if (cnt > 0) {
                const float4* p = reinterpret_cast<const float4*>(s.emiTris + tri);
                const float4 a = p[0], b = p[1], c = p[2];
                float bx, by, dist;
                tri++; cnt--;
                if (tri_hit(ray.o, ray.d, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z), bx, by, dist)) { found = true; cur = endOff; q.n = 0; cnt = 0; }
            }
        }
    }
    return maybe || found;
}

// ---- closest hit of incoherent rays through the trees that keep the reference's order ---------------------------------------
// DevScene::intersect (src/scene.h:245-284) accepts a triangle iff its leaf is entered -- the reference's box test passes on the
// leaf (and, before it, on every ancestor) with tBox < closest AT THAT MOMENT -- and intersectTriangle hits closer than closest at
// that moment: the result depends on the order in which the walk meets the triangles.  The tree walked here (occlusion_bvh.cpp
// rs_build_ordered_bvh; one per threaded order) meets them in the reference's order through better boxes on the shadow tree's
// grid, and the rule is applied literally:
//   * a node is entered iff the relaxed test passes with tBox' < closest.  tBox' <= tLeaf of every triangle below (conservative
//     boxes, occlusion_bvh.cpp), so a skipped node holds only leaves the reference would not enter at this `closest` or any later one;
//   * a triangle hit closer than `closest` is a candidate; it is accepted iff the reference's own test passes along the path to
//     its leaf with tLeaf < closest (the chain check of the shadow rays, leaf shortcut included) -- exactly when the reference
//     reaches it.  Boxes are nested (occNested is a precondition), so tLeaf bounds the ancestors' entry distances.
// Leaves are queued and tested in wave-wide rounds as in walk_occlusion_tree, but FIRST IN, FIRST OUT and one candidate at a
// time, so that a lane's triangles are judged in the reference's order with the reference's `closest`; a walk that runs ahead of
// its queue only uses a staler (larger) `closest`, i.e. enters more, never less.  Same primitive, same barycentrics, same bits as
// walk<...>; tested against it and against the oracle on the full scenes.
// Only for general-case rays that start within the grid's reach (as the shadow walk); every lane of the wave must call it.
#ifndef RS_ORD_QUEUE
#define RS_ORD_QUEUE 4          // leaves a lane may queue before the wave runs a leaf round (1..4)
#endif
__device__ __forceinline__ WalkResult walk_ordered_tree(const DevScene& s, const Ray& ray, const RayBoxCtx& ctx, bool active) {
    WalkResult r;
    const char* nodes = reinterpret_cast<const char*>(s.ordNodes);
    const unsigned k = active ? (unsigned)mtbvh_order(-ray.d) : 0u;
    const unsigned endOff = (k + 1u) * s.ordStride - 16u;
    const TriRec* tris = s.ordTris + (size_t)(k >> 1) * (size_t)s.numPrims;
    const int triStep = (k & 1u) ? -1 : 1;
    const GridRay grid(s.occBase, s.occScale, ctx, active);      // a lane without a ray rests on the end record
    const float tRoot = root_extent(ctx.o, ctx.dinv, s.occRootLo, s.occRootHi);
    unsigned cur = active ? k * s.ordStride : endOff;
    LeafQueue q;                                                // queued leaf codes, first in, first out
#ifdef RS_WALK_STATS
    unsigned long long st[12] = { 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    int mySteps = 0;
#define RS_OSTAT(i, v) st[i] += (v)
#else
#define RS_OSTAT(i, v)
#endif
    for (;;) {
        for (;;) {          // walk phase: until some lane's queue is full or every walk has ended
            if (!__ballot(cur != endOff)) break;
            RS_OSTAT(1, 1); RS_OSTAT(2, __popcll(__ballot(cur != endOff)));
#ifdef RS_WALK_STATS
            if (cur != endOff) mySteps++;
#endif
            const uint4 n = *reinterpret_cast<const uint4*>(nodes + cur);
            const GridSlab t = grid.slab(n);
            const bool pass = (t.tMax >= fmaxf(t.tMin, 0.f)) && (t.tMin < r.closest);
            const int meta = (int)n.w;
            const bool leaf = meta < 0;
            q.push_fifo(pass && leaf, ~meta);
            cur = (pass || leaf) ? cur + 16u : (unsigned)meta;
            if (__any(q.n == RS_ORD_QUEUE)) break;
        }
        if (!__any(q.n > 0)) break;
        {
        // leaf round: every lane takes its OLDEST queued leaf and judges its triangles one after the other
        RS_OSTAT(3, 1);
        int tri = 0, cnt = 0, verify = -1;
        if (q.n > 0) { const int code = q.pop(); tri = code >> 3; cnt = code & 7; }
        float cd = 0.f, cbx = 0.f, cby = 0.f; int cprim = kNullPrim;
        for (;;) {
            while (__any((cnt > 0) & (verify < 0))) {
                RS_OSTAT(4, 1); RS_OSTAT(5, __popcll(__ballot((cnt > 0) & (verify < 0))));
                if ((cnt > 0) & (verify < 0)) {
                    const float4* p = reinterpret_cast<const float4*>(tris + tri);
                    const float4 a = p[0], b = p[1], c = p[2];
                    float bx, by, dist;
                    tri += triStep; cnt--;
                    if (tri_hit(ray.o, ray.d, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z), bx, by, dist) && dist < r.closest) {
                        cd = dist; cbx = bx; cby = by; cprim = __float_as_int(b.w);
                        verify = __float_as_int(a.w);          // reference leaf of the candidate
                    }
                }
            }
            if (!__any(verify >= 0)) break;
            while (__any(verify >= 0)) {
                RS_OSTAT(6, 1); RS_OSTAT(7, __popcll(__ballot(verify >= 0)));
                if (verify >= 0) {
                    // the chain check of the shadow rays, leaf shortcut included (occNested is a precondition of this walk)
                    const ChainStep c = chain_step(s.occChain + verify, ctx, r.closest, tRoot);
                    const bool done = c.open & ((c.parent < 0) | c.clear);
                    if (done) { r.closest = cd; r.bx = cbx; r.by = cby; r.prim = cprim; }
                    verify = (c.open & !done) ? c.parent : -1;          // closed: the reference never reaches the triangle
                }
            }
        }
        }
    }
#ifdef RS_WALK_STATS
    if (s.walkStats && __lane_id() == 0) for (int i = 0; i < 8; i++) atomicAdd(&s.walkStats[64 + i], st[i]);
    if (s.walkStats && active) { atomicAdd(&s.walkStats[72], 1ull); atomicAdd(&s.walkStats[73], (unsigned long long)mySteps); }
#endif
#undef RS_OSTAT
    return r;
}

// testOcclusion for the segments of a wave: general-case rays within the grid's reach through the shadow tree, the rare other lanes
// (and every lane of a scene without that tree) through the reference's tree with deferred leaf tests.  All 64 lanes must call this.
__device__ __forceinline__ bool walk_segment_wave(const DevScene& s, const Ray& ray, float limit, bool active) {
    RayBoxCtx ctx = make_box_ctx(ray);
    ctx.cull = s.axisCull;
    const bool special = active && ray_is_special(ctx, ray);
    if (s.occNodes) {
        const bool slow = active && (special || !grid_reaches(s.occBase, s.occScale, ray.o));
        bool any = walk_occlusion_tree(s, ray, ctx, limit, active && !slow);
        if (__any(slow)) any = walk_anyhit_deferred<false>(s, ray, ctx, limit, slow) || any;
        return any;
    }
    return __any(special) ? walk_anyhit_deferred<false>(s, ray, ctx, limit, active)
                          : walk_anyhit_deferred<true>(s, ray, ctx, limit, active);
}

// closest hit for the rays of a wave: through the tree of the ray's order; the rare other rays (and every ray of a scene without
// those trees) walk the reference's.  All 64 lanes must call this.
__device__ __forceinline__ WalkResult walk_closest_wave(const DevScene& s, const Ray& ray, bool active) {
    RayBoxCtx ctx = make_box_ctx(ray);
    ctx.cull = s.axisCull;
    const bool special = active && ray_is_special(ctx, ray);
    if (s.ordNodes) {
        const bool slow = active && (special || !grid_reaches(s.occBase, s.occScale, ray.o));
        WalkResult r = walk_ordered_tree(s, ray, ctx, active && !slow);
        if (__any(slow)) {
            const WalkResult r2 = walk_paired<false>(s, ray, ctx, slow);
            if (slow) r = r2;
        }
        return r;
    }
    if (__any(special)) return walk_paired<false>(s, ray, ctx, active);
    return walk_paired<true>(s, ray, ctx, active);
}

// getIntersecGeomInfo (scene.h:135-151): the Hit of a walk's primitive and barycentrics
__device__ __forceinline__ Hit hit_of_walk(const DevScene& s, int prim, float bx, float by) {
    Hit h;
    h.primId = prim;
    h.matId = 0;
    h.pos = splat(0.f);
    h.norm = splat(0.f);
    h.bx = bx; h.by = by;
    if (prim != kNullPrim) {
        const float* v = s.vertices + (size_t)prim * 9;
        const float* n = s.normals + (size_t)prim * 9;
        float wgt = 1.f - bx - by;
        h.pos = ld3(v + 3) * bx + ld3(v + 6) * by + ld3(v) * wgt;
        h.norm = normalize(ld3(n + 3) * bx + ld3(n + 6) * by + ld3(n) * wgt);
        h.matId = s.materialIds[prim];
    }
    return h;
}

// DevScene::intersect (src/scene.h:245-284): closest hit, stackless threaded walk
__device__ inline Hit trace_closest(const DevScene& s, const Ray& ray) {
    const WalkResult w = walk_dispatch(s, ray);
    return hit_of_walk(s, w.prim, w.bx, w.by);
}

// ---- wave-cooperative ("packet") closest-hit walk for coherent rays ------------------------------
// Measured on the per-lane walk above (rocprofv3, profiles/): the G-buffer and primary-ray kernels
// are bound by the vector-memory return path (TD busy 87-89 %): every lane fetches its own 32-byte
// node, 2 KiB per wave-step, although the 64 rays of an 8x8 pixel tile visit almost the same nodes
// (union of visited nodes 158 vs 142 for the slowest single ray, one threaded order per tile).
//
// Here the WAVE walks the union once.  All walks of one order move forward through the same array,
// so the wave visits c = min over lanes of "the node I want next"; the node record is fetched ONCE
// through the scalar cache (s_load_dwordx8: 32 B per wave-step instead of 2 KiB), every lane whose
// own walk is at c runs its slab / triangle test against the SGPR-resident record, the others wait.
// Each lane still visits exactly the nodes of DevScene::intersect (src/scene.h:245-284), in the same
// order with the same arithmetic, so results are bit-identical to the per-lane walk.
//
// Must be called by all 64 lanes of the wave (`active` false for lanes without a ray).

__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
    // butterfly inside rows of 16 (quad_perm xor1, xor2, row_half_mirror, row_mirror), then the two
    // row broadcasts of gfx9; lane 63 ends up with the minimum of all 64 lanes
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false));
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false));
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false));
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xF, 0xF, false));
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x142, 0xA, 0xF, false));
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x143, 0xC, 0xF, false));
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// ---- the fast form of the packet walk ---------------------------------------------------------------------------------------
// For general-case rays (none of AABB::intersect's special cases) whose direction has the same component signs in every lane of
// the wave (all but the ~1 % of 8x8 tiles that straddle a sign change), on a proper box table with nested miss links
// (DevScene::axisCull && linksNested).  Same nodes per lane, same order, same arithmetic on the values that decide -- what
// changes is how little the wave does per node.  Measured on the r01 loop: 54 VALU + ~30 SALU instructions per union node, and
// both units issue one instruction per SIMD every four cycles, so the scalar side counts as much as the vector side:
//   * near / far plane of each axis: with lo <= hi, (lo - o) * dinv <= (hi - o) * dinv for dinv > 0 and the other way round for
//     dinv < 0, because IEEE subtraction and multiplication round monotonically -- the reference's glm::min / glm::max
//     (bvh.h:128-129) pick a known operand (same floats up to the sign of a zero, which no comparison sees).  The sign pattern
//     NEG is a template parameter (eight loop bodies, one runs), so the choice costs no instruction at all;
//   * AABB::intersect's general case is overlap & tMax >= 0 & tMax >= tMin (bvh.h:147-153) and the walk then asks
//     tMin < closest.  A conjunction can be evaluated in any order: the distance part comes first (tMax >= max(tMin, 0)), and
//     the three overlap comparisons, which cost as much as everything else, only run when some lane passed it;
//   * no reduction for the next node.  The walks of a wave all move forward through one pre-order array whose miss links nest
//     (link(c) <= link(a) for c inside (a, link(a)), checked by rs_scene_create).  A lane that is not at c waits at a node
//     p > c which it reached by rejecting some a < c, so p = link(a) with c inside a's span, hence link(c) <= p; the lanes
//     at c go to c + 1 (entered) or link(c).  The minimum of all pending targets is therefore c + 1 if any lane entered and
//     link(c) otherwise: one ballot instead of a 64-lane DPP minimum.  For the same reason a lane's own target after a node
//     nobody entered is max(myNext, link(c)) -- one instruction, no mask.
// Slab distances of one record held in SGPRs {min.x, min.y, min.z, max.z | max.x, max.y, prim, next}: three packed subtractions
// and three packed multiplications, each the reference's (p - ori) * dirInv on two components
struct SlabT { vf2 xy1, xy2, z12; };      // (t1.x, t1.y), (t2.x, t2.y), (t1.z, t2.z)
__device__ __forceinline__ SlabT slabs(vf2 oxy, vf2 ozz, vf2 dxy, vf2 dzz, const float4& ra, const float4& rb) {
    SlabT t;
    t.xy1 = (vf2{ ra.x, ra.y } - oxy) * dxy;
    t.xy2 = (vf2{ rb.x, rb.y } - oxy) * dxy;
    t.z12 = (vf2{ ra.z, ra.w } - ozz) * dzz;
    return t;
}
template <int NEG> __device__ __forceinline__ float near_x(const SlabT& t) { return (NEG & 1) ? t.xy2.x : t.xy1.x; }
template <int NEG> __device__ __forceinline__ float far_x(const SlabT& t) { return (NEG & 1) ? t.xy1.x : t.xy2.x; }
template <int NEG> __device__ __forceinline__ float near_y(const SlabT& t) { return (NEG & 2) ? t.xy2.y : t.xy1.y; }
template <int NEG> __device__ __forceinline__ float far_y(const SlabT& t) { return (NEG & 2) ? t.xy1.y : t.xy2.y; }
template <int NEG> __device__ __forceinline__ float near_z(const SlabT& t) { return (NEG & 4) ? t.z12.y : t.z12.x; }
template <int NEG> __device__ __forceinline__ float far_z(const SlabT& t) { return (NEG & 4) ? t.z12.x : t.z12.y; }
// Both parts end in ONE float comparison whose operand carries the other conditions (a lane that already failed compares against
// an infinity): the result of a comparison is a lane mask in SGPRs that a ballot can use as it is, where a boolean combined
// from several would first be turned into 0 / 1 per lane and compared again.
template <int NEG>
__device__ __forceinline__ bool slab_distance_part(const SlabT& t, bool part, float closest, float& chord) {
    const float tMin = fmaxf(fmaxf(near_x<NEG>(t), near_y<NEG>(t)), near_z<NEG>(t));
    const float tMax = fminf(fminf(far_x<NEG>(t), far_y<NEG>(t)), far_z<NEG>(t));
    const bool ok = part && (tMax >= fmaxf(tMin, 0.f));
    chord = tMax - tMin;
    return tMin < (ok ? closest : -__builtin_inff());
}
// The overlap part without evaluating it.  In real arithmetic its three comparisons are fy > nz, fz > nx, fx > ny, and each of
// those differences is at least tMax - tMin (fy >= tMax = min f, nz <= tMin = max n).  Evaluated in float as the reference
// does -- (fy - ny) + (fz - nz) > fz - ny: three subtractions and a sum of values below 4 T in magnitude -- the two sides keep
// their order whenever the real difference exceeds 10 * 2^-24 * T, T = the largest |slab distance| at the node.  Every box lies
// inside the root box (DevScene::axisCull) and subtraction and multiplication round monotonically, so T <= tRoot, the largest
// |slab distance| of the ROOT box: a per-ray constant.  A lane with tMax - tMin > 2^-19 * tRoot (three times the bound) therefore
// passes the overlap part whatever its bits; any other lane (a box the ray only grazes, a flat box: tMax == tMin) sends the wave
// to the exact evaluation.  On the benchmark view 98 % of the entered nodes take the shortcut (tools/walk_stats.py).
__device__ __forceinline__ float overlap_margin(f3 o, f3 dinv, const float4& rootA, const float4& rootB) {
    return root_extent(o, dinv, mk3(rootA.x, rootA.y, rootA.z), mk3(rootB.x, rootB.y, rootA.w)) * 1.9073486328125e-6f;       // 2^-19 * tRoot
}
template <int NEG>
__device__ __forceinline__ bool slab_overlap_part(const SlabT& t, bool near) {
    const float nx = near_x<NEG>(t), ny = near_y<NEG>(t), nz = near_z<NEG>(t), fx = far_x<NEG>(t), fy = far_y<NEG>(t), fz = far_z<NEG>(t);
    const float dx = fx - nx, dy = fy - ny, dz = fz - nz;
    const bool ok = near & (dy + dz > fz - ny) & (dz + dx > fx - nz);     // plain "and": the short-circuit form compiles to nested exec-mask regions
    return dx + dy > (ok ? fy - nx : __builtin_inff());
}

// base, end: the records the wave walks and how many -- one threaded order of nodesAll (bvhSize records), or a cell's cut of it
// (rs_cuts.h: the same records re-linked, first record the same root box); the record at `end` is readable either way
template <int NEG, bool COUNT>
__device__ __forceinline__ void packet_walk_fast(const DevScene& s, const char* __restrict__ base, unsigned end, bool mine, const Ray& ray, const RayBoxCtx& ctx, WalkResult& r) {
    const vf2 oxy = { ctx.o.x, ctx.o.y }, ozz = { ctx.o.z, ctx.o.z }, dxy = { ctx.dinv.x, ctx.dinv.y }, dzz = { ctx.dinv.z, ctx.dinv.z };
    unsigned myNext = mine ? 0u : end;
    unsigned c = 0;                                           // wave-uniform
    float4 ra = *reinterpret_cast<const float4*>(base), rb = *reinterpret_cast<const float4*>(base + 16);      // uniform addresses -> scalar loads
    const float margin = overlap_margin(ctx.o, ctx.dinv, ra, rb);        // the first record is the root
    while (c != end) {
        if (COUNT) r.nodes++;                                 // (a scalar instruction per node: only for launches that split their heavy tiles)
#ifdef RS_WALK_STATS
        r.steps++; if (myNext == c) r.myVisits++;
#endif
        const int prim = __float_as_int(rb.z);
        const unsigned nxt = (unsigned)__float_as_int(rb.w), cNext = c + 1u;
        const SlabT t = slabs(oxy, ozz, dxy, dzz, ra, rb);
        float chord;
        const bool near = slab_distance_part<NEG>(t, myNext == c, r.closest, chord);
        const unsigned long long nearMask = __builtin_amdgcn_ballot_w64(near);
        unsigned target = nxt;                                // wave-uniform: the record the wave reads next
        float4 pa, pb;
        bool took = false;
        if (nearMask != 0ull) {
            // the record after this one is requested as soon as some lane may enter (it is the successor then), before the
            // overlap part and the triangle test; a node every lane rejects on the distance part does not pay for it
            pa = *reinterpret_cast<const float4*>(base + cNext * 32u); pb = *reinterpret_cast<const float4*>(base + cNext * 32u + 16u);
#ifdef RS_WALK_STATS
            r.nearSteps++;
#endif
            // (ballots of plain comparisons, combined on the scalar unit: a ballot of a combined boolean costs two vector instructions)
            bool entered = near;
            unsigned long long enteredMask = nearMask;
            if ((nearMask & __builtin_amdgcn_ballot_w64(!(chord > margin))) != 0ull) {
                entered = slab_overlap_part<NEG>(t, near);
                enteredMask = __builtin_amdgcn_ballot_w64(entered);
            }
#ifdef RS_WALK_STATS
            else r.clearSteps++;
#endif
            if (enteredMask != 0ull) {
#ifdef RS_WALK_STATS
                r.enteredSteps++; if (prim != kNullPrim) r.leafSteps++;
#endif
                if (prim != kNullPrim) {                      // uniform branch
                    const float4* tp = reinterpret_cast<const float4*>(s.tris + prim);      // uniform -> scalar
                    const float4 a = tp[0], b = tp[1], e = tp[2];
                    float bx, by, dist;
                    const bool hit = tri_hit<true>(ray.o, ray.d, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(e.x, e.y, e.z), bx, by, dist);
                    if (entered && hit && dist < r.closest) { r.closest = dist; r.bx = bx; r.by = by; r.prim = prim; }
                }
                myNext = entered ? cNext : max(myNext, nxt);
                target = cNext; took = true;
            }
        }
        if (!took) {
            myNext = max(myNext, nxt);
            pa = *reinterpret_cast<const float4*>(base + nxt * 32u); pb = *reinterpret_cast<const float4*>(base + nxt * 32u + 16u);     // (requesting it at the top of every step as well: frame 1.20 -> 1.27 ms)
        }
        c = target; ra = pa; rb = pb;       // (one tail for both outcomes: with `continue` in the entered branch the compiler carried an undefined record index through the other, one v_readfirstlane per node)
    }
}

template <bool GENERAL, bool COUNT>
__device__ __forceinline__ void packet_walk_order(const DevScene& s, int order, bool mine, const Ray& ray,
                                                  const RayBoxCtx& ctx, WalkResult& r) {
    const BvhNode* __restrict__ nodes = s.nodesAll + (size_t)order * (size_t)s.bvhSize;
    const unsigned end = (unsigned)s.bvhSize;
    unsigned myNext = mine ? 0u : end;
    unsigned c = 0;                                           // wave-uniform
    // uniform addresses -> scalar loads.  The record after the current one is requested before the current
    // one is tested: c+1 is the successor whenever any lane enters the node (about half of the steps), and
    // then the scalar-load latency is off the wave's critical path.  nodes[end] is readable (next order / padding).
    const float4* np0 = reinterpret_cast<const float4*>(nodes);
    float4 lo, hi;
    node_unpack(np0[0], np0[1], lo, hi);
    while (c != end) {
        if (COUNT) r.nodes++;
#ifdef RS_WALK_STATS
        r.steps++;
#endif
        const float4* nq = reinterpret_cast<const float4*>(nodes + c + 1);
        float4 plo, phi;
        node_unpack(nq[0], nq[1], plo, phi);
        const int prim = __float_as_int(lo.w);
        const unsigned nxt = (unsigned)__float_as_int(hi.w);
        const bool part = myNext == c;
        float tb;
        bool bh;
        if (GENERAL) bh = box_hit_general(ctx.o, ctx.dinv, lo, hi, tb);
        else bh = box_hit(ctx, mk3(lo.x, lo.y, lo.z), mk3(hi.x, hi.y, hi.z), tb);
        const bool entered = part & bh & (tb < r.closest);
        if (prim != kNullPrim) {                              // uniform branch
            if (__any(entered)) {
                const float4* tp = reinterpret_cast<const float4*>(s.tris + prim);      // uniform -> scalar
                const float4 a = tp[0], b = tp[1], e = tp[2];
                float bx, by, dist;
                const bool hit = tri_hit(ray.o, ray.d, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(e.x, e.y, e.z), bx, by, dist);
                if (entered && hit && dist < r.closest) { r.closest = dist; r.bx = bx; r.by = by; r.prim = prim; }
            }
        }
        myNext = part ? (entered ? c + 1u : nxt) : myNext;
        // every pending target is > c; if some lane wants c+1 that is the minimum
        if (__any(myNext == c + 1u)) { c = c + 1u; lo = plo; hi = phi; }
        else {
            c = wave_min_u32(myNext);
            const float4* np = reinterpret_cast<const float4*>(nodes + c);
            node_unpack(np[0], np[1], lo, hi);
        }
    }
}

// the bits of `neg`: a direction component is negative in the lanes that take part (the same in all of them)
template <bool COUNT>
__device__ __forceinline__ void packet_walk_fast_dispatch(int neg, const DevScene& s, const char* base, unsigned end, bool mine, const Ray& ray, const RayBoxCtx& ctx, WalkResult& r) {
    switch (neg) {
        case 0: packet_walk_fast<0, COUNT>(s, base, end, mine, ray, ctx, r); break;
        case 1: packet_walk_fast<1, COUNT>(s, base, end, mine, ray, ctx, r); break;
        case 2: packet_walk_fast<2, COUNT>(s, base, end, mine, ray, ctx, r); break;
        case 3: packet_walk_fast<3, COUNT>(s, base, end, mine, ray, ctx, r); break;
        case 4: packet_walk_fast<4, COUNT>(s, base, end, mine, ray, ctx, r); break;
        case 5: packet_walk_fast<5, COUNT>(s, base, end, mine, ray, ctx, r); break;
        case 6: packet_walk_fast<6, COUNT>(s, base, end, mine, ray, ctx, r); break;
        default: packet_walk_fast<7, COUNT>(s, base, end, mine, ray, ctx, r); break;
    }
}

// A cell's cut of one threaded order (rs_cuts.h): `end` records at `base`, cut from order `order`; end == 0: the cell has none
struct CutRef { const char* base; unsigned end; int order; };

// ---- the walk through a tile's leaf list (rs_cuts.h "Leaf lists") ---------------------------------------------------------------------
// A tile's list: `end` 64-byte records at `base`, one per leaf that some ray of the tile may pass geometrically, in the threaded order
// `order`; leafOf[c] = the reference node of record c (its record in occChain).  end == 0: the tile has none.  Record c, four float4:
//   { min.x, min.y, min.z, max.z } { max.x, max.y, bits(prim), v0.x } { v0.y, v0.z, e1.x, e1.y } { e1.z, e2.x, e2.y, e2.z }
// -- the box half laid out as a BvhNode's, the triangle as s.tris holds it, so that a step is one scalar fetch of the record after.
struct LeafListRef { const char* base; const int* leafOf; unsigned end; int order; };

// Why the bits stay.  A lane's result depends only on the sequence of triangles it tests and the `closest` it tests each against.  The
// reference tests leaf L's triangle iff it enters L and, before it, every ancestor of L (box test passed with tMin < closest at that
// moment).  Here every lane of the order visits every record of the list, in the threaded order:
//   * entered = the reference's own test on L's box with tMin < closest: slabs + slab_distance_part, then the chord > margin shortcut
//     or slab_overlap_part, exactly as packet_walk_fast decides it;
//   * boxes are nested (DevScene::occNested, checked at scene build) and (p - o) * dinv rounds monotonically, so an ancestor's near
//     distances are <= and its far distances >= the leaf's: tMax >= 0, tMax >= tMin and tMin < closest carry from L to every ancestor
//     -- also to the moment the reference stood on that ancestor, because `closest` only falls.  Conversely an ancestor the reference
//     rejected on those three had tMin >= its closest then >= closest now, and so has L;
//   * the overlap part alone is not monotone in float.  A lane whose leaf clears it by chain_step's margin (2^-18 tRoot) has settled it for
//     the whole path; any other lane with a candidate runs the reference's test up occChain, from the leaf's own record (its `open`
//     is `entered` again, its `clear` the exact form of the margin -- a flat leaf box has chord <= 0 and still clears more often than
//     not) to the first clear ancestor, and accepts only if every record on the way is open.  This is the rule walk_ordered_tree lives
//     by; only triangles that would lower `closest` pay for it, a rejected triangle changes nothing whether the reference met it or not;
//   * a leaf absent from the list is one no ray of the tile passes geometrically (containment, as for the cut: rs_cuts.h), so the
//     reference never enters it;
//   * the list keeps the threaded order, so ties under the strict `<` fall as before.
// Needs what packet_walk_fast needs (general-case rays of one sign pattern, a proper box table) and occChain with nested boxes; the
// builder makes no list otherwise.  There are no links: the record after is requested at the top of every step.
template <int NEG, bool COUNT>
__device__ __forceinline__ void packet_walk_leaves(const DevScene& s, const LeafListRef& list, bool mine, const Ray& ray, const RayBoxCtx& ctx, WalkResult& r) {
    const vf2 oxy = { ctx.o.x, ctx.o.y }, ozz = { ctx.o.z, ctx.o.z }, dxy = { ctx.dinv.x, ctx.dinv.y }, dzz = { ctx.dinv.z, ctx.dinv.z };
    const float tRoot = root_extent(ctx.o, ctx.dinv, s.occRootLo, s.occRootHi);
    const float margin = tRoot * 1.9073486328125e-6f, clearMargin = tRoot * 3.814697265625e-6f;      // 2^-19 (overlap_margin), 2^-18 (chain_step)
    const char* __restrict__ base = list.base;
    const unsigned end = list.end;
    const float4* first = reinterpret_cast<const float4*>(base);      // uniform addresses -> scalar loads
    float4 q0 = first[0], q1 = first[1], q2 = first[2], q3 = first[3];
    for (unsigned c = 0; c != end; c++) {
        const float4* np = reinterpret_cast<const float4*>(base + (c + 1u) * 64u);       // (the record at `end` is readable)
        const float4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
        if (COUNT) r.nodes++;
#ifdef RS_WALK_STATS
        r.steps++; if (mine) r.myVisits++;
#endif
        const SlabT t = slabs(oxy, ozz, dxy, dzz, q0, q1);
        float chord;
        const bool near = slab_distance_part<NEG>(t, mine, r.closest, chord);
        const unsigned long long nearMask = __builtin_amdgcn_ballot_w64(near);
        if (nearMask != 0ull) {
#ifdef RS_WALK_STATS
            r.nearSteps++;
#endif
            bool entered = near;
            unsigned long long enteredMask = nearMask;
            if ((nearMask & __builtin_amdgcn_ballot_w64(!(chord > margin))) != 0ull) {
                entered = slab_overlap_part<NEG>(t, near);
                enteredMask = __builtin_amdgcn_ballot_w64(entered);
            }
#ifdef RS_WALK_STATS
            else r.clearSteps++;
#endif
            if (enteredMask != 0ull) {
#ifdef RS_WALK_STATS
                r.enteredSteps++; r.leafSteps++;
#endif
                float bx, by, dist;
                const bool hit = tri_hit<true>(ray.o, ray.d, mk3(q1.w, q2.x, q2.y), mk3(q2.z, q2.w, q3.x), mk3(q3.y, q3.z, q3.w), bx, by, dist);
                const bool candidate = entered && hit && dist < r.closest;
                bool accept = candidate && chord > clearMargin;
                int verify = -1;
                if (__builtin_amdgcn_ballot_w64(candidate && !(chord > clearMargin)) != 0ull) {
                    const int leaf = list.leafOf[c];                  // uniform -> scalar
                    verify = (candidate && !accept) ? leaf : -1;
                    while (__any(verify >= 0)) {
#ifdef RS_WALK_STATS
                        r.chainSteps++;
#endif
                        if (verify >= 0) {
                            const ChainStep cs = chain_step(s.occChain + verify, ctx, r.closest, tRoot);
                            const bool done = cs.open & ((cs.parent < 0) | cs.clear);
                            accept = accept | done;
                            verify = (cs.open & !done) ? cs.parent : -1;          // closed: the reference never reaches the triangle
                        }
                    }
                }
                if (accept) { r.closest = dist; r.bx = bx; r.by = by; r.prim = __float_as_int(q1.z); }
            }
        }
        q0 = n0; q1 = n1; q2 = n2; q3 = n3;
    }
}

template <bool COUNT>
__device__ __forceinline__ void packet_walk_leaves_dispatch(int neg, const DevScene& s, const LeafListRef& list, bool mine, const Ray& ray, const RayBoxCtx& ctx, WalkResult& r) {
    switch (neg) {
        case 0: packet_walk_leaves<0, COUNT>(s, list, mine, ray, ctx, r); break;
        case 1: packet_walk_leaves<1, COUNT>(s, list, mine, ray, ctx, r); break;
        case 2: packet_walk_leaves<2, COUNT>(s, list, mine, ray, ctx, r); break;
        case 3: packet_walk_leaves<3, COUNT>(s, list, mine, ray, ctx, r); break;
        case 4: packet_walk_leaves<4, COUNT>(s, list, mine, ray, ctx, r); break;
        case 5: packet_walk_leaves<5, COUNT>(s, list, mine, ray, ctx, r); break;
        case 6: packet_walk_leaves<6, COUNT>(s, list, mine, ray, ctx, r); break;
        default: packet_walk_leaves<7, COUNT>(s, list, mine, ray, ctx, r); break;
    }
}

// closest hit for a wave of coherent rays; lanes with active == false carry no ray
// unionNodes (may be null): the number of nodes the wave visited, the length of its chain of dependent fetches (tile splitting, rs_tilesplit.h)
// cut (wave-uniform): the walk of order cut.order goes through the cut's records instead of the tree's when it takes the fast form --
// every other walk (special-case rays, mixed signs, another order, a table without nested links) ignores it
template <bool COUNT = false>
// list (wave-uniform): under the same conditions the walk of order list.order goes through the tile's leaf list instead of either
__device__ inline Hit trace_closest_packet(const DevScene& s, const Ray& ray, bool active, unsigned* unionNodes = nullptr, CutRef cut = CutRef{ nullptr, 0u, 0 },
                                           LeafListRef list = LeafListRef{ nullptr, nullptr, 0u, 0 }) {
    WalkResult w;
    RayBoxCtx ctx = make_box_ctx(ray);
    ctx.cull = s.axisCull;
    const bool special = active && ray_is_special(ctx, ray);
    const bool anySpecial = __any(special);
    const int order = mtbvh_order(-ray.d);
    unsigned long long todo = __ballot(active);
#ifdef RS_WALK_STATS
    w.steps = w.nearSteps = w.enteredSteps = w.leafSteps = w.clearSteps = 0; w.myVisits = 0; w.chainSteps = w.listSteps = 0;
    unsigned norders = 0;
#endif
    while (todo) {                                            // one pass per threaded order present in the wave
#ifdef RS_WALK_STATS
        norders++;
#endif
        const int lead = __ffsll((long long)todo) - 1;
        const int k = __builtin_amdgcn_readlane(order, lead);
        const bool mine = active && order == k;
        const unsigned long long mm = __ballot(mine);
        todo &= ~mm;
        const unsigned long long sx = __ballot(mine && ray.d.x < 0.f), sy = __ballot(mine && ray.d.y < 0.f), sz = __ballot(mine && ray.d.z < 0.f);
        const bool uniformSigns = (sx == 0 || sx == mm) && (sy == 0 || sy == mm) && (sz == 0 || sz == mm);
        if (anySpecial) packet_walk_order<false, COUNT>(s, k, mine, ray, ctx, w);
        else if (uniformSigns && s.axisCull && s.linksNested) {
            const int neg = (sx ? 1 : 0) | (sy ? 2 : 0) | (sz ? 4 : 0);
            if (list.end != 0u && k == list.order) {
#ifdef RS_WALK_STATS
                w.listSteps += list.end;
#endif
                packet_walk_leaves_dispatch<COUNT>(neg, s, list, mine, ray, ctx, w);
                continue;
            }
            const bool cutHere = cut.end != 0u && k == cut.order;
            const char* base = cutHere ? cut.base : reinterpret_cast<const char*>(s.nodesAll + (size_t)k * (size_t)s.bvhSize);
            packet_walk_fast_dispatch<COUNT>(neg, s, base, cutHere ? cut.end : (unsigned)s.bvhSize, mine, ray, ctx, w);
        }
        else packet_walk_order<true, COUNT>(s, k, mine, ray, ctx, w);
    }
#ifdef RS_WALK_STATS
    if (s.walkStats && __lane_id() == 0) {
        atomicAdd(&s.walkStats[16], 1ull); atomicAdd(&s.walkStats[17], (unsigned long long)w.steps);
        atomicMax(&s.walkStats[18], (unsigned long long)w.steps); atomicAdd(&s.walkStats[19], (unsigned long long)norders);
        atomicAdd(&s.walkStats[20], anySpecial ? 1ull : 0ull);
        atomicAdd(&s.walkStats[21], (unsigned long long)w.nearSteps); atomicAdd(&s.walkStats[22], (unsigned long long)w.enteredSteps);
        atomicAdd(&s.walkStats[23], (unsigned long long)w.leafSteps); atomicAdd(&s.walkStats[15], (unsigned long long)w.clearSteps);
        atomicAdd(&s.walkStats[24 + (w.steps ? 31 - __clz((int)w.steps) : 0)], 1ull);
        atomicAdd(&s.walkStats[94], (unsigned long long)w.listSteps); atomicAdd(&s.walkStats[95], (unsigned long long)w.chainSteps);       // (88..93: the RIS loop's, restir.hip)
    }
    {   // is a heavy tile heavy because its rays diverge (large union) or because single rays visit that many nodes?
        unsigned mv = w.myVisits;
        for (int off = 32; off > 0; off >>= 1) mv = max(mv, (unsigned)__shfl_xor((int)mv, off));
        if (s.walkStats && __lane_id() == 0) {
            atomicAdd(&s.walkStats[87], (unsigned long long)mv);
            if (w.steps >= 1024u) { atomicAdd(&s.walkStats[84], 1ull); atomicAdd(&s.walkStats[85], (unsigned long long)w.steps); atomicAdd(&s.walkStats[86], (unsigned long long)mv); }
        }
    }
#endif
    if (unionNodes) *unionNodes = w.nodes;
    return hit_of_walk(s, w.prim, w.bx, w.by);
}

// closest hit for a whole wave of INCOHERENT rays (bounce rays): every lane of the wave must call it, `active` false where there is no ray
__device__ inline Hit trace_closest_wave(const DevScene& s, const Ray& ray, bool active) {
    const WalkResult w = walk_closest_wave(s, ray, active);
    return hit_of_walk(s, active ? w.prim : kNullPrim, w.bx, w.by);
}

// the shadow ray of the segment from x to y: makeOffsetedRay (intersections.h:13-15) and the range testOcclusion walks it with
__device__ __forceinline__ Ray shadow_ray(f3 x, f3 y, float& range) {
    f3 dir = y - x;
    float dist = length(dir);
    dir = div3_exact_signed(dir, dist);
    Ray ray; ray.o = x + dir * 1e-5f; ray.d = dir;
    range = dist - 1e-4f * 2.f;
    return ray;
}

// DevScene::testOcclusion (src/scene.h:286-316), any hit between x and y, for a whole wave of (incoherent) segments; every lane of
// the wave must call it, `active` false where there is no segment
__device__ inline bool trace_occluded_wave(const DevScene& s, f3 x, f3 y, bool active) {
    float range;
    const Ray ray = shadow_ray(x, y, range);
    return walk_segment_wave(s, ray, range, active);
}

}  // namespace rs
#endif  // __HIPCC__
