// rs_indirect_revalidate.h -- the device-free half of ReSTIR-GI's revalidation (rs_restir_set_indirect_revalidation;
// indirect_revalidate.hip): what one history slot of Reservoir<IndirectLiSample> is to a frame whose scene took geometry edits since the
// previous rs_restir_indirect call -- a function of the slot's own floats and of the frame's dirty boxes (rs_revalidate_plan.h), which the
// kernel evaluates per lane and rs_debug_indirect_candidate_classes hands to tests that have no device.  Both ends of the segment
// xv -> xs are stored in the slot, so the class does not depend on the pixel that reads it.
// Left as it is, on purpose: an edit of emission, materials or textures changes no box, so a stale Lo stays stale; and there is no
// spatial side to revalidate -- ReSTIR-GI has none here.
#pragma once
#include "rs_revalidate_plan.h"

enum { RS_IND_NOT_EXAMINED = 0, RS_IND_STALE = 1, RS_IND_WALK = 2, RS_IND_KEPT = 3 };

// a point in one of the frame's boxes: closed intervals, lo <= p <= hi on every axis; a NaN coordinate fails every comparison
RS_REVAL_HD bool rs_point_in_boxes(float x, float y, float z, const rs_revalidate_boxes& boxes) {
    bool any = false;
    for (int i = 0; i < RS_DIRTY_BOXES_KEPT; i++) {
        if (i >= boxes.n) break;
        const rs_dirty_box& d = boxes.box[i];
        any = any || (d.lo[0] <= x && x <= d.hi[0] && d.lo[1] <= y && y <= d.hi[1] && d.lo[2] <= z && z <= d.hi[2]);
    }
    return any;
}

// The class of a slot with weight W, visible point xv and sample point xs.
//   RS_IND_NOT_EXAMINED  W is NaN, infinite or not above 0 (-0, +0, negative), or xv == xs on all three components (IEEE ==: +0 equals
//                        -0, a NaN equals nothing) -- a slot no path ever recorded two points into
//   RS_IND_STALE         examined and "everything", or xs lies in a dirty box: the surface it was taken on has moved
//   RS_IND_WALK          examined, not stale, and rs_segment_in_boxes(xv, xs): the segment may cross moved geometry and is walked
//   RS_IND_KEPT          examined and out of every box's reach: the slot stays as it is
// Stale before walk, in that order: a slot in "everything" mode never walks.
RS_REVAL_HD int rs_indirect_slot_class(float W, const float xv[3], const float xs[3], const rs_revalidate_boxes& boxes) {
    const bool finite = W == W && W != __builtin_inff() && W != -__builtin_inff();
    if (!finite || !(W > 0.f)) return RS_IND_NOT_EXAMINED;
    if (xv[0] == xs[0] && xv[1] == xs[1] && xv[2] == xs[2]) return RS_IND_NOT_EXAMINED;
    if (boxes.everything) return RS_IND_STALE;
    if (rs_point_in_boxes(xs[0], xs[1], xs[2], boxes)) return RS_IND_STALE;
    if (rs_segment_in_boxes(xv[0], xv[1], xv[2], xs[0], xs[1], xs[2], boxes)) return RS_IND_WALK;
    return RS_IND_KEPT;
}
