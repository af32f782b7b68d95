// rs_shadow_regroup.h -- the device-free half of the regrouped shadow-ray kernel (restir.hip k_shadow_regroup): which of kShadowBins
// length bins a shadow segment lies in, and which slots the rays of a block's bins take when the block hands its 256 segments out to its
// waves longest first -- as functions of plain floats and integers.  Nothing here touches the device, a context or a global: the kernel
// evaluates shadow_bin per lane and the same descending prefix per wave, and rs_debug_plan_shadow_regroup hands both to a test that has
// no device.  Any-hit occlusion does not depend on which lane carries a ray, so WHICH slot of its bin's range a ray takes is free (the
// kernel takes arrival order); which bin it lies in, and so where the bin's range starts, is not.
#pragma once

#if defined(__HIPCC__)
#define RS_REGROUP_HD __host__ __device__ inline
#else
#define RS_REGROUP_HD inline
#endif

constexpr int kShadowBins = 64;            // one per lane of a wave: a wave scans the histogram in one pass
constexpr int kShadowRegroupRays = 256;    // a block's segments (32x8 pixels, rs_internal.h pixel_of_lane)

// binsOverExtent = kShadowBins / |occRootHi - occRootLo| (the diagonal of the reference's root box).  0 .. kShadowBins - 1, monotone in
// the length.  The clamp comes BEFORE the conversion: an environment sample's length is 1e10 (and +inf, or a degenerate scene's
// inf * length, never reaches a float-to-int conversion) -> the top bin; a NaN fails `t < top` and takes the top bin too (such a ray
// takes the walk's special-case path, the longest there is); a negative length, and -0, take bin 0.
RS_REGROUP_HD int shadow_bin(float length, float binsOverExtent) {
    const float t = length * binsOverExtent;
    if (!(t < (float)(kShadowBins - 1))) return kShadowBins - 1;
    return t > 0.f ? (int)t : 0;
}

inline float shadow_bins_over_extent(const float lo[3], const float hi[3]) {
    const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    return (float)kShadowBins / __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
}

// The slot plan of one block: bins[i] < 0 is an inactive lane.  first[b]: the first slot of bin b's rays when the active rays take slots
// 0 .. count - 1 with the longest bin first (first[b] = number of active rays in bins above b; an empty bin's is where its rays would
// start).  Returns count.
inline int rs_plan_shadow_slots(const int* bins, int n, int first[kShadowBins]) {
    int hist[kShadowBins] = {};
    for (int i = 0; i < n; i++) if (bins[i] >= 0) hist[bins[i] < kShadowBins ? bins[i] : kShadowBins - 1]++;
    int at = 0;
    for (int b = kShadowBins - 1; b >= 0; b--) { first[b] = at; at += hist[b]; }
    return at;
}
