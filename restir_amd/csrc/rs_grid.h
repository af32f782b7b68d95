// rs_grid.h -- the 16-bit grid of the grid-box trees (occlusion_bvh.cpp rs_quantize_occlusion_bvh): how one exact box becomes the three
// box dwords of a 16-byte record.  One definition for the host builder and for the device refit (scene_refit.hip).
#pragma once

#include "rs_math.h"

namespace rs {

// Grid planes on axis k lie at base[k] + q * scale[k].  The planes are moved outward until they clear the exact box by `margin`
// (2^-17 of the grid's extent: why, occlusion_bvh.cpp), checked in double.  out: { lo.x | lo.y << 16, lo.z | hi.x << 16, hi.y | hi.z << 16 }.
// False (out untouched) when the box does not fit the grid's 16 bits.
RS_HD bool grid_box(const float lo[3], const float hi[3], const float base[3], const float scale[3], double margin, unsigned out[3]) {
    unsigned ql[3], qh[3];
    for (int k = 0; k < 3; k++) {
        if (!(lo[k] >= -3.4e38f && hi[k] <= 3.4e38f)) return false;          // (NaN or infinite: the loops below would not end)
        const double b = (double)base[k], s = (double)scale[k];
        long lowest = (long)floor(((double)lo[k] - margin - b) / s);
        long highest = (long)ceil(((double)hi[k] + margin - b) / s);
        while (b + (double)lowest * s > (double)lo[k] - margin) lowest--;
        while (b + (double)highest * s < (double)hi[k] + margin) highest++;
        if (lowest < 0 || highest > 65535) return false;
        ql[k] = (unsigned)lowest; qh[k] = (unsigned)highest;
    }
    out[0] = ql[0] | (ql[1] << 16);
    out[1] = ql[2] | (qh[0] << 16);
    out[2] = qh[1] | (qh[2] << 16);
    return true;
}

}  // namespace rs
