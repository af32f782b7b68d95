// rs_revalidate_plan.h -- the device-free half of shadow revalidation (rs_restir_set_shadow_revalidation; shadow_revalidate.hip): the box
// an accepted geometry edit dirties, the scene's ring of such boxes, what a frame takes from the ring, and the test that says whether a
// shadow segment may cross one of the frame's boxes -- as functions of plain floats and integers.  Nothing here touches the device, a
// context or a global: scene_edits.hip calls the first two when an edit is accepted, shadow_revalidate.hip the third at enqueue time, the
// kernel evaluates the fourth per lane, and the rs_debug_plan_* hooks hand all of them to tests that have no device.
#pragma once
#include <unordered_set>

#if defined(__HIPCC__)
#define RS_REVAL_HD __host__ __device__ inline
#else
#define RS_REVAL_HD inline
#endif

#ifndef RS_DIRTY_BOXES_KEPT
#define RS_DIRTY_BOXES_KEPT 8             // edits whose boxes a scene keeps, and boxes a frame takes at most (include/restir_hip.h)
#endif

struct rs_dirty_box { float lo[3], hi[3]; };
// edit: the scene's count of accepted geometry edits (rs_scene::geomEdits) once this one was counted, 1 for the first
struct rs_dirty_entry { unsigned long long edit; rs_dirty_box box; };
struct rs_dirty_ring { rs_dirty_entry e[RS_DIRTY_BOXES_KEPT]; int count = 0; };      // oldest first
// what a frame hands its kernel, by value: n boxes, or "everything" (every examined segment walks)
struct rs_revalidate_boxes { rs_dirty_box box[RS_DIRTY_BOXES_KEPT]; int n, everything; };
struct rs_revalidate_choice { int launch; rs_revalidate_boxes boxes; };

// The box of one edit: the exact AABB of the old and the new corners of the primitives it names -- min and max alone, no arithmetic.
// oldVertices is the scene's whole table (9 floats per primitive) as it was before the edit, newVertices the edit's records (9 floats per
// record).  An id named twice takes its last record's new corners (the edit calls' rule) and its old corners once; `distinct`: the
// caller knows that no id occurs twice (rs_set_geometry's records) and the set below is not built.  count = 0: lo = +inf, hi = -inf.
inline void rs_plan_dirty_box(const float* oldVertices, int count, const int* ids, const float* newVertices, bool distinct, float lo[3], float hi[3]) {
    for (int k = 0; k < 3; k++) { lo[k] = __builtin_inff(); hi[k] = -__builtin_inff(); }
    auto take = [&](const float* v9) {
        for (int c = 0; c < 9; c++) {
            const float x = v9[c];
            const int k = c % 3;
            lo[k] = x < lo[k] ? x : lo[k];
            hi[k] = x > hi[k] ? x : hi[k];
        }
    };
    std::unordered_set<int> seen;
    for (int j = count - 1; j >= 0; j--) {                      // from the last record down: the first one met of an id is the one that counts
        if (!distinct && !seen.insert(ids[j]).second) continue;
        take(oldVertices + (size_t)ids[j] * 9);
        take(newVertices + (size_t)j * 9);
    }
}

// an accepted edit joins the ring; the oldest entry leaves a full one
inline void rs_dirty_ring_push(rs_dirty_ring& ring, unsigned long long edit, const float lo[3], const float hi[3]) {
    if (ring.count == RS_DIRTY_BOXES_KEPT) {
        for (int i = 1; i < RS_DIRTY_BOXES_KEPT; i++) ring.e[i - 1] = ring.e[i];
        ring.count--;
    }
    rs_dirty_entry& e = ring.e[ring.count++];
    e.edit = edit;
    for (int k = 0; k < 3; k++) { e.box.lo[k] = lo[k]; e.box.hi[k] = hi[k]; }
}

// The frame's choice.  entries: the ring, oldest first; seen: the scene's count of edits at this rs_restir's previous frame; now: the
// count at this frame; sameScene: the scene is the previous frame's.  Another scene: launch, everything.  No edit in (seen, now]: no
// launch.  Otherwise the boxes of the edits seen + 1 .. now in the ring's order -- or everything when one of them has left the ring (more
// than RS_DIRTY_BOXES_KEPT edits in the gap, or an rs_restir that lagged while the ring turned over), or when the count went backwards.
inline void rs_plan_revalidation(const rs_dirty_entry* entries, int count, unsigned long long seen, unsigned long long now, bool sameScene, rs_revalidate_choice& out) {
    out.launch = 0; out.boxes.n = 0; out.boxes.everything = 0;
    for (rs_dirty_box& b : out.boxes.box) for (int k = 0; k < 3; k++) { b.lo[k] = 0.f; b.hi[k] = 0.f; }
    if (!sameScene) { out.launch = 1; out.boxes.everything = 1; return; }
    if (now == seen) return;
    out.launch = 1;
    if (now < seen || now - seen > (unsigned long long)RS_DIRTY_BOXES_KEPT) { out.boxes.everything = 1; return; }
    int n = 0;
    for (int i = 0; i < count; i++)
        if (entries[i].edit > seen && entries[i].edit <= now && n < RS_DIRTY_BOXES_KEPT) out.boxes.box[n++] = entries[i].box;
    if ((unsigned long long)n != now - seen) { out.boxes.n = 0; out.boxes.everything = 1; return; }
    out.boxes.n = n;
}

// Does the segment a -> b have to be walked again?  Its bounding box against every dirty box, closed intervals, comparisons only: on every
// axis min(a, b) <= hi and max(a, b) >= lo, written without min / max so that a NaN coordinate fails (as NumPy's minimum / maximum, which
// carry the NaN into a comparison that is then false).  Conservative: a segment that passes a box's corner within its own bounding box walks.
RS_REVAL_HD bool rs_axis_overlaps(float a, float b, float lo, float hi) {
    return (a <= hi || b <= hi) && (a >= lo || b >= lo) && a == a && b == b;
}
RS_REVAL_HD bool rs_segment_in_boxes(float ax, float ay, float az, float bx, float by, float bz, const rs_revalidate_boxes& boxes) {
    if (boxes.everything) return true;
    bool any = false;
    for (int i = 0; i < RS_DIRTY_BOXES_KEPT; i++) {
        if (i >= boxes.n) break;
        const rs_dirty_box& d = boxes.box[i];
        any = any || (rs_axis_overlaps(ax, bx, d.lo[0], d.hi[0]) && rs_axis_overlaps(ay, by, d.lo[1], d.hi[1]) && rs_axis_overlaps(az, bz, d.lo[2], d.hi[2]));
    }
    return any;
}
