// rs_cuts.h -- static cuts of the MTBVH for the primary rays of a camera that stands still.
//
// Of the union nodes a tile's packet walk visits, about two in five are rejected by EVERY lane on geometry alone (EXPERIMENTS.md "Primary
// cuts") -- the camera and the box decide that, the same way in every frame.  A CELL is the 32x8 pixels of one primary-ray block
// (four 8x8 tiles, one wave each).  Its cut is a copy, in nodesAll's record format, of the records of one threaded order that some ray of
// the cell may pass geometrically, re-linked among themselves; packet_walk_fast (rs_walk.h) walks it with `base` and `end` set to the
// cell's records and nothing else changed.
//
// Which records.  A node is kept iff all its ancestors are kept and the conservative cell test below passes on its box; kept records keep
// their pre-order, and the link of a kept record is next' = the index within the cut of the first kept record whose original index is >=
// the original miss link (the cut's length if there is none).
//
// Why every lane computes the same bits.  Take one lane and its walk through the whole tree: a sequence of visited nodes, each entered
// (box test passed with tMin < closest: go to the next record) or rejected (go to the miss link).  It visits a node only after entering
// all its ancestors.  Entering needs the geometric part of the test, and a node on which that part passes for some ray of the cell passes
// the cell test (containment, below): by induction from the root every entered node is kept, so a visited node that is NOT kept has kept
// ancestors only, fails the cell test itself and is rejected -- the lane goes to its miss link, past a subtree that holds no kept record
// (kept sets are closed under ancestors).  Unkept nodes are therefore only ever stepped over, one subtree at a time, forwards.
//   * entered -> next record: the whole-tree walk goes from kept node n to n + 1 and from there steps over unkept subtrees until it
//     stands on the first kept node of index > n; the cut walk goes to the record after n's, which is that node.
//   * rejected -> next': the whole-tree walk goes to link(n) and steps over unkept subtrees until it stands on the first kept node of
//     index >= link(n), or leaves the tree; the cut walk goes to next', which is that node, or to the cut's end.
// The kept nodes a lane visits, their order, the boxes and triangles it tests and the `closest` it tests them against are the same in
// both walks, and a stepped-over node changes nothing in a lane's state.  For the wave: packet_walk_fast needs nested links, and next'
// is monotone in the original link, so c inside (a, next'(a)) is a kept node inside (a, link(a)) and next'(c) <= next'(a).
//
// The cell test.  All rays of a cell start at cam.position, and the unnormalised direction of camera_sample (rs_scene.h) is affine in
// the screen coordinate, so per world axis it lies between its values at the cell's four extreme (pixel, jitter) corners -- jitter 0 of
// the first pixel, jitter 1 of the last (Rng::uniform reaches 1).  The slab test is invariant under a positive scale of the direction,
// so nothing is normalised: with D.c in [dlo.c, dhi.c], all of one sign, the near and far slab distances (p - o.c) / D.c of a box have
// exact interval bounds, and the test is the interval form of tMax >= max(tMin, 0):
//     min over axes of (largest far distance)  >=  max(max over axes of (smallest near distance), 0) - margin.
// Evaluated in double, so that its own rounding (2^-52) does not count.  What the margin and the widening of D cover is the lane's float
// arithmetic:
//   * its direction.  camera_sample's sum right * X + up * Y + view * Z has absolute error below 2^-20 |D| per component (a dozen float
//     roundings of terms below |D|), and normalisation and the reciprocal scale all three components alike up to 2^-22: the lane's
//     direction is a positive multiple of some D + e, |e.c| < 2^-20 |D|.  The intervals are widened by 2^-16 M, M = the largest
//     |component| of the corner directions (>= |D| / sqrt 3).  (The rounding of the screen coordinate, 2^-23, enters X scaled by aspect *
//     tanFovY * focalDist while |D| >= |focalDist|: the bound holds while |aspect * tanFovY| and |tanFovY| stay below 16, and a camera
//     beyond that takes no cut at all.  The MAGNITUDES: rs_make_cam_params takes the tangent of the whole angle fov.y, which is
//     negative past 90 degrees -- -2.29e7 at the float right angle, -57.3 at 91 -- and the argument is about the size of X, not its
//     sign.  An angle whose tangent is negative and small, such as 120 or -60 degrees, mirrors the image and keeps its cuts; so does a
//     negative focalDist, which scales all of D.)  A cell whose widened interval reaches within 2^-10 M of zero takes no
//     cut: that covers the sign change, AABB::intersect's near-zero and axis-aligned cases (the wave checks ray_is_special itself
//     and ignores the cut), and keeps the widening below 2^-6 of the interval's ends.
//   * its slab distances.  (p - o) * dinv is a rounded difference times a rounded reciprocal, rounded: relative error below 2^-22.  A
//     lane whose float test passes has far.a >= near.b in float for every pair of axes, hence in real arithmetic far.a - near.b >=
//     -2^-21 T, T = the largest |slab distance| of the ROOT box (root_extent, rs_walk.h: it bounds those of every box).  The margin is
//     2^-16 R with R >= T the interval maximum of the root's |slab distances|: 32 times the rounding it has to cover.
// A cell takes no cut -- and walks the tree as before -- if its four corners do not share one mtbvh_order, if a bound is not finite,
// if its cut is empty or longer than the cap, or if the arena is full.  The wave still compares its own order with the cell's.
//
// Leaf lists.  Nine in ten of the steps a wave still takes through its cell's cut are inner nodes (EXPERIMENTS.md "Primary leaf lists"), and
// for a still camera an inner node only lets the wave skip leaves -- which the camera and the boxes decide as well, once.  The reference
// tree has one triangle per leaf, so an 8x8 TILE (one wave) gets the LEAF records of the cut of its own 8x8 cell, in the threaded order,
// box and triangle side by side in 64 bytes (LeafListRef, rs_walk.h), and packet_walk_leaves walks them one after the other: no links, the
// same triangle tests as before, a quarter of the box tests.  Containment is the cut's, for the tile's own cell: the list is made by the cut's walk,
// which descends through kept nodes only, and the cut's induction shows that every node some ray of the cell passes geometrically after
// passing all its ancestors is kept -- the reference enters no other.  Why the lane's bits stay although the inner nodes are gone is packet_walk_leaves' argument (rs_walk.h).
// A tile takes no list -- and keeps its block's cut, or the tree -- if cut_cell gives it no order, if its list is empty or longer than the
// cap, if the arena is full, or if the scene lacks occChain / nested boxes.  Same key and lifetime as the cuts; built by the same call.
//
// This header: what k_primary / k_primary_split read (PrimaryCuts, cut_of_cell, leaf_list_of_tile) and the geometry, the walk and the
// re-linking as host-and-device functions.  The slots, the build, its kernels and the entry points: primary_cuts.hip; the key and the
// slot's state: rs_cut_plan.h.
#pragma once

#include "rs_walk.h"

namespace rs {

// the cuts of one launch geometry: cells[c] = { first record, count | order << 28 } (count 0: no cut), `records` the arena they index
// tiles[t] = { first record, count | order << 28 } of tile t's leaf list (tiles numbered as primary_body numbers them: row-major over the
// launch's 8x8 tiles), leafRecords / leafOf the arena they index (LeafListRef, rs_walk.h); tiles == null: no lists
struct PrimaryCuts { const uint2* cells; const BvhNode* records; const uint2* tiles; const float4* leafRecords; const int* leafOf; };
constexpr unsigned kCutCountMask = (1u << 28) - 1u;

// what the conservative test of a cell needs: per axis the interval of the unnormalised direction mapped to the POSITIVE case (a negative
// axis is mirrored: planes and origin change sign), so that the near plane is always `a` and the far plane always `b`
struct CutCell {
    double o[3], dlo[3], dhi[3];
    bool neg[3];
    int order;              // -1: the cell takes no cut
    double margin;          // 2^-16 R, set from the root box (cut_cell_margin)
};

// Camera::sample's unnormalised direction for screen position (sx, sy) in pixels (jitter included), in double
RS_HD void cut_corner_dir(const CamParams& c, double sx, double sy, double D[3]) {
    const double ruvx = 1.0 - (sx * (double)c.pixelSizeX) * 2.0, ruvy = 1.0 - (sy * (double)c.pixelSizeY) * 2.0;
    const double X = ruvx * (double)c.aspect * (double)c.tanFovY * (double)c.focalDist, Y = ruvy * (double)c.tanFovY * (double)c.focalDist, Z = (double)c.focalDist;
    D[0] = (double)c.right.x * X + (double)c.up.x * Y + (double)c.view.x * Z;
    D[1] = (double)c.right.y * X + (double)c.up.y * Y + (double)c.view.y * Z;
    D[2] = (double)c.right.z * X + (double)c.up.z * Y + (double)c.view.z * Z;
}

// the cell of pixels [x0, x0 + w) x [y0, y0 + h)
RS_HD CutCell cut_cell(const CamParams& c, int x0, int y0, int w, int h) {
    CutCell cell;
    cell.order = -1; cell.margin = 0.0;
    double lo[3], hi[3], M = 0.0;
    int order = -1;
    bool ok = gabs(c.aspect * c.tanFovY) <= 16.f && gabs(c.tanFovY) <= 16.f;       // (the widening's bound, above, on the magnitudes; false for NaN)
    for (int k = 0; k < 4; k++) {
        double D[3];
        cut_corner_dir(c, (double)(x0 + ((k & 1) ? w : 0)), (double)(y0 + ((k & 2) ? h : 0)), D);
        for (int a = 0; a < 3; a++) {
            if (!(D[a] - D[a] == 0.0)) ok = false;                  // not finite
            lo[a] = k == 0 ? D[a] : (D[a] < lo[a] ? D[a] : lo[a]);
            hi[a] = k == 0 ? D[a] : (D[a] > hi[a] ? D[a] : hi[a]);
            const double m = D[a] < 0.0 ? -D[a] : D[a];
            M = m > M ? m : M;
        }
        const int ord = mtbvh_order(mk3((float)-D[0], (float)-D[1], (float)-D[2]));
        if (k == 0) order = ord; else if (ord != order) ok = false;
    }
    const double o[3] = { (double)c.position.x, (double)c.position.y, (double)c.position.z };
    const double widen = M * (1.0 / 65536.0), keepOff = M * (1.0 / 1024.0);
    for (int a = 0; a < 3; a++) {
        if (!(o[a] - o[a] == 0.0)) ok = false;
        const double l = lo[a] - widen, h2 = hi[a] + widen;
        if (l > keepOff) { cell.neg[a] = false; cell.dlo[a] = l; cell.dhi[a] = h2; cell.o[a] = o[a]; }
        else if (h2 < -keepOff) { cell.neg[a] = true; cell.dlo[a] = -h2; cell.dhi[a] = -l; cell.o[a] = -o[a]; }
        else { ok = false; cell.neg[a] = false; cell.dlo[a] = cell.dhi[a] = 1.0; cell.o[a] = 0.0; }
    }
    if (ok && M > 0.0) cell.order = order;
    return cell;
}

// near / far plane of a record's box on axis a, mirrored with the axis
RS_HD void cut_planes(const CutCell& cell, const BvhNode& n, double pa[3], double pb[3]) {
    const double lo[3] = { (double)n.bminx, (double)n.bminy, (double)n.bminz }, hi[3] = { (double)n.bmaxx, (double)n.bmaxy, (double)n.bmaxz };
    for (int a = 0; a < 3; a++) {
        pa[a] = (cell.neg[a] ? -hi[a] : lo[a]) - cell.o[a];
        pb[a] = (cell.neg[a] ? -lo[a] : hi[a]) - cell.o[a];
    }
}

// R = the interval maximum of the root box's |slab distances|; false: not finite (no cut)
RS_HD bool cut_cell_margin(CutCell& cell, const BvhNode& root) {
    double pa[3], pb[3], R = 0.0;
    cut_planes(cell, root, pa, pb);
    for (int a = 0; a < 3; a++) {
        const double fa = pa[a] < 0.0 ? -pa[a] : pa[a], fb = pb[a] < 0.0 ? -pb[a] : pb[a];
        const double t = (fa > fb ? fa : fb) / cell.dlo[a];
        R = t > R ? t : R;
    }
    cell.margin = R * (1.0 / 65536.0);
    return R - R == 0.0;
}

// may some ray of the cell pass the geometric part of the box test on this record?  (anything that is not a number: yes)
RS_HD bool cut_cell_test(const CutCell& cell, const BvhNode& n) {
    double pa[3], pb[3];
    cut_planes(cell, n, pa, pb);
    double tMinLo = 0.0, tMaxHi = 0.0;
    for (int a = 0; a < 3; a++) {
        const double nearLo = pa[a] >= 0.0 ? pa[a] / cell.dhi[a] : pa[a] / cell.dlo[a];
        const double farHi = pb[a] >= 0.0 ? pb[a] / cell.dlo[a] : pb[a] / cell.dhi[a];
        tMinLo = nearLo > tMinLo ? nearLo : tMinLo;               // (starts at 0: max(tMin, 0))
        tMaxHi = (a == 0 || farHi < tMaxHi) ? farHi : tMaxHi;
        if (!(nearLo == nearLo) || !(farHi == farHi)) return true;
    }
    return !(tMaxHi < tMinLo - cell.margin);
}

// The cut's walk over records [0, end) of the cell's order (rec(i): record i): it descends through kept records only, emit(k, i, record)
// for the k-th kept record -- LEAVES: for the k-th kept LEAF, a tile's list -- in threaded order.  Returns how many there are, or cap + 1
// as soon as there are more than `cap` (nothing is emitted past the cap).  stopAt: a caller that knows the count (the builders' writing
// pass: cap = stopAt = the count) ends the walk with the last emitted record instead of stepping over the rest of the tree.  Host and
// device: the device builders (primary_cuts.hip) and the host's planning hooks (rs_debug_plan_primary_cut,
// rs_debug_plan_primary_leaf_list) run this very function.
// (One thread walks one cell, a dependent load and a double-precision test per step: the loop keeps ONE exit, on `limit`.  With a second
// exit from its middle -- "return cap + 1" where the record past the cap is met -- the cuts' builder took 5 % longer on configs 3 and 5.)
template <bool LEAVES, class Rec, class Emit>
RS_HD unsigned cut_walk(const CutCell& cell, Rec rec, unsigned end, unsigned cap, Emit emit, unsigned stopAt = 0xffffffffu) {
    const unsigned limit = stopAt <= cap ? stopAt : cap + 1u;
    unsigned count = 0;
    for (unsigned cur = 0; cur != end && count != limit;) {
        const BvhNode n = rec(cur);
        if (cut_cell_test(cell, n)) {
            if (!LEAVES || n.primId != kNullPrim) { if (count != cap) emit(count, cur, n); count++; }
            cur++;
        }
        else cur = (unsigned)n.next;
    }
    return count;
}

// The links of a cut of `count` records ("Which records", above): orig(j) is the original index of kept record j (rising), link(i) the
// original miss link of kept record i; set(i, next') with next' = the first kept record after i whose original index is >= link(i),
// or count.  Host and device, as the walk.
template <class Orig, class Link, class Set>
RS_HD void cut_relink(Orig orig, Link link, unsigned count, Set set) {
    for (unsigned i = 0; i < count; i++) {
        const unsigned to = link(i);
        unsigned lo = i + 1u, hi = count;
        while (lo < hi) { const unsigned mid = (lo + hi) >> 1; if (orig(mid) < to) lo = mid + 1u; else hi = mid; }
        set(i, lo);
    }
}

#if defined(__HIPCC__)
// the leaf list of tile `tile` of a primary-ray launch (wave-uniform; tile < 0: none)
__device__ __forceinline__ LeafListRef leaf_list_of_tile(const PrimaryCuts& cuts, int tile) {
    if (!cuts.tiles || tile < 0) return LeafListRef{ nullptr, nullptr, 0u, 0 };
    const uint2 t = cuts.tiles[__builtin_amdgcn_readfirstlane(tile)];                    // (uniform, said explicitly: cut_of_cell)
    const unsigned first = (unsigned)__builtin_amdgcn_readfirstlane((int)t.x), word = (unsigned)__builtin_amdgcn_readfirstlane((int)t.y);
    return LeafListRef{ reinterpret_cast<const char*>(cuts.leafRecords + (size_t)first * 4u), cuts.leafOf + first, word & kCutCountMask, (int)(word >> 28) };
}

// the cut of block `cell` of a primary-ray launch (wave-uniform)
__device__ __forceinline__ CutRef cut_of_cell(const PrimaryCuts& cuts, int cell) {
    if (!cuts.cells) return CutRef{ nullptr, 0u, 0 };
    // (the index and the entry are the same in every lane; said explicitly, because a record base the compiler cannot prove uniform
    // turns the walk's scalar fetches into per-lane loads: 64 registers and scratch instead of 44)
    const uint2 c = cuts.cells[__builtin_amdgcn_readfirstlane(cell)];
    const unsigned first = (unsigned)__builtin_amdgcn_readfirstlane((int)c.x), word = (unsigned)__builtin_amdgcn_readfirstlane((int)c.y);
    return CutRef{ reinterpret_cast<const char*>(cuts.records + first), word & kCutCountMask, (int)(word >> 28) };
}
#endif  // __HIPCC__

}  // namespace rs
