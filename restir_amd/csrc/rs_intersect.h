// rs_intersect.h -- the reference's ray / box and ray / triangle tests (AABB::intersect src/bvh.h:85-157, intersectTriangle
// src/intersections.h:17-54, DevScene::getMTBVHId src/scene.h:101-119), host and device: the leaf tests every walk of rs_walk.h ends in,
// which the oracle and the golden files pin.
#pragma once

#include "rs_scene.h"

namespace rs {

// ---- ray / box / triangle ----------------------------------------------------------------------
// Per-ray constants of AABB::intersect (src/bvh.h:85-157): which special case applies depends only
// on the ray direction, so it is classified once per ray instead of once per node.
struct RayBoxCtx {
    f3 o, d, dinv;
    int mode;          // 0 general, 1/2/3 axis-aligned along x/y/z (abs(d) > 1-1e-6, first match)
    bool zx, zy, zz;   // abs(d.c) < 1e-6
    bool cull;         // skip_far_on_axis allowed: the box table is a proper hierarchy (DevScene::axisCull)
};

RS_HD RayBoxCtx make_box_ctx(const Ray& r) {
    const float Eps = 1e-6f;
    RayBoxCtx c;
    c.o = r.o; c.d = r.d;
#if defined(__HIP_DEVICE_COMPILE__)
    c.dinv = rcp3_exact_signed(r.d);
#else
    c.dinv = mk3(1.f / r.d.x, 1.f / r.d.y, 1.f / r.d.z);
#endif
    c.mode = gabs(r.d.x) > 1.f - Eps ? 1 : (gabs(r.d.y) > 1.f - Eps ? 2 : (gabs(r.d.z) > 1.f - Eps ? 3 : 0));
    c.zx = gabs(r.d.x) < Eps; c.zy = gabs(r.d.y) < Eps; c.zz = gabs(r.d.z) < Eps;
    c.cull = true;
    return c;
}

RS_HD bool in_range(float x, float lo, float hi) { return x >= lo && x <= hi; }

RS_HD bool slab_max_min(float n1, float n2, float f1, float f2_, float& tMin) {   // getDistMaxMin bvh.h:75-79
    tMin = fmaxf(n1, n2);
    float tMax = fminf(f1, f2_);
    return tMax >= 0.f && tMax >= tMin;
}
RS_HD bool slab_min_max(float t1, float t2, float& tMin) {                        // getDistMinMax bvh.h:69-73
    tMin = fminf(t1, t2);
    float tMax = fmaxf(t1, t2);
    return tMax >= 0.f && tMax >= tMin;
}

// true only when the ray's coordinate on the ignored axis stays outside [lo-tol, hi+tol] for every
// t in [max(t0,0), t1]; NaN / infinite inputs never skip.
RS_HD bool skip_far_on_axis(float o, float d, float lo, float hi, float t0, float t1) {
    const float a = o + d * fmaxf(t0, 0.f), b = o + d * t1;
    const float tol = 1e-3f * (1.f + fmaxf(gabs(lo), gabs(hi)));
    const float mn = fminf(a, b), mx = fmaxf(a, b);
    return (mx < lo - tol) || (mn > hi + tol);
}

RS_HD bool box_hit(const RayBoxCtx& c, f3 bmin, f3 bmax, float& tMin) {
    if (c.mode != 0) {                         // axis-aligned rays (bvh.h:91-123), rare
        if (c.mode == 1) {
            if (in_range(c.o.y, bmin.y, bmax.y) && in_range(c.o.z, bmin.z, bmax.z))
                return slab_min_max((bmin.x - c.o.x) * c.dinv.x, (bmax.x - c.o.x) * c.dinv.x, tMin);
            return false;
        }
        if (c.mode == 2) {
            if (in_range(c.o.z, bmin.z, bmax.z) && in_range(c.o.x, bmin.x, bmax.x))
                return slab_min_max((bmin.y - c.o.y) * c.dinv.y, (bmax.y - c.o.y) * c.dinv.y, tMin);
            return false;
        }
        if (in_range(c.o.x, bmin.x, bmax.x) && in_range(c.o.y, bmin.y, bmax.y))
            return slab_min_max((bmin.z - c.o.z) * c.dinv.z, (bmax.z - c.o.z) * c.dinv.z, tMin);
        return false;
    }
    f3 t1 = (bmin - c.o) * c.dinv;
    f3 t2 = (bmax - c.o) * c.dinv;
    f3 tn = vmin(t1, t2);
    f3 tf = vmax(t1, t2);
    f3 td = tf - tn;
    float yz = tf.z - tn.y;
    float zx = tf.x - tn.z;
    float xy = tf.y - tn.x;
    bool oyz = td.y + td.z > yz, ozx = td.z + td.x > zx, oxy = td.x + td.y > xy;
    // Near-zero direction component: the reference tests only the other two slabs (bvh.h:136-146), so
    // such a ray "enters" every box its projection crosses and walks thousands of nodes (measured:
    // 2.5k-10k steps against a mean of 130; a handful of such rays per 1080p frame set the kernel's
    // tail).  skip_far_on_axis() adds a conservative cull on the ignored axis: a box is skipped only
    // if the ray stays farther than a generous tolerance from it over the interval it crosses the
    // other two slabs.  A skipped subtree cannot contain a triangle the ray hits (a Moeller-Trumbore
    // hit point lies inside its triangle's box up to rounding << tol), the visiting order of the
    // remaining nodes is unchanged, so closest hit, ties and occlusion results are identical.  That argument
    // needs boxes that contain their triangles and their children, which rs_scene_create checks
    // (DevScene::axisCull); for any other caller-supplied table the cull is off.  It also needs the hit point to be where the
    // ray is, which fails for a ray inside a triangle's plane: every quantity of the test is rounding then, and only the
    // reference's absolute threshold on the determinant rejects it.  In a scene with triangles large enough for such a
    // determinant to pass that threshold the cull is off as well (scene.hip far_skip_allowed clears DevScene::axisCull).
    if (c.zx && oyz) return slab_max_min(tn.y, tn.z, tf.y, tf.z, tMin) && !(c.cull && skip_far_on_axis(c.o.x, c.d.x, bmin.x, bmax.x, tMin, fminf(tf.y, tf.z)));
    if (c.zy && ozx) return slab_max_min(tn.z, tn.x, tf.z, tf.x, tMin) && !(c.cull && skip_far_on_axis(c.o.y, c.d.y, bmin.y, bmax.y, tMin, fminf(tf.z, tf.x)));
    if (c.zz && oxy) return slab_max_min(tn.x, tn.y, tf.x, tf.y, tMin) && !(c.cull && skip_far_on_axis(c.o.z, c.d.z, bmin.z, bmax.z, tMin, fminf(tf.x, tf.y)));
    if (oyz && ozx && oxy)
        return slab_max_min(fmaxf(tn.x, tn.y), tn.z, fminf(tf.x, tf.y), tf.z, tMin);
    return false;
}

// intersectTriangle (src/intersections.h:17-54) on a pre-differenced triangle record
// SIGNBIT: `if (det < 0) { det = -det; t = -t; }` as sign-bit arithmetic (5 vector instructions instead of 9 in the packet walks;
// the per-lane shadow-ray walk is faster with the branch-free selects, so it keeps them): |det| >= FLT_EPSILON at that point, so
// det < 0 is its sign bit, and a NaN determinant fails every comparison below whatever the sign of t.
template <bool SIGNBIT = false>
RS_HD bool tri_hit(f3 o, f3 d, f3 v0, f3 e01, f3 e02, float& bx, float& by, float& dist) {
    f3 p = cross(d, e02);
    float det = dot(p, e01);
    if (gabs(det) < 1.1920928955078125e-7f) return false;       // FLT_EPSILON
    f3 t = o - v0;
    if (SIGNBIT) {
        const unsigned flip = __builtin_bit_cast(unsigned, det) & 0x80000000u;
        det = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, det) ^ flip);
        t = mk3(__builtin_bit_cast(float, __builtin_bit_cast(unsigned, t.x) ^ flip), __builtin_bit_cast(float, __builtin_bit_cast(unsigned, t.y) ^ flip),
                __builtin_bit_cast(float, __builtin_bit_cast(unsigned, t.z) ^ flip));
    }
    else if (det < 0.f) { det = -det; t = -t; }
    bx = dot(t, p);
    if (bx < 0.f || bx > det) return false;
    f3 q = cross(t, e01);
    by = dot(d, q);
    if (by < 0.f || bx + by > det) return false;
    float inv = 1.f / det;
    dist = dot(e02, q) * inv;
    bx *= inv;
    by *= inv;
    return dist > 0.f;
}

// DevScene::getMTBVHId (src/scene.h:101-119)
RS_HD int mtbvh_order(f3 dir) {
    float ax = gabs(dir.x), ay = gabs(dir.y), az = gabs(dir.z);
    if (ax > ay) {
        if (ax > az) return dir.x > 0 ? 0 : 1;
        return dir.z > 0 ? 4 : 5;
    }
    if (ay > az) return dir.y > 0 ? 2 : 3;
    return dir.z > 0 ? 4 : 5;
}

#if defined(__HIPCC__)
// "Is this a special-case ray": one whose direction takes a special case of AABB::intersect (axis-aligned, a near-zero component) or
// is NaN.  The branch-free general test and the trees on the grid are only for the other rays.
__device__ __forceinline__ bool ray_is_special(const RayBoxCtx& ctx, const Ray& ray) {
    return ctx.mode != 0 || ctx.zx || ctx.zy || ctx.zz || !(ray.d.x == ray.d.x);
}

// General-case slabs (bvh.h:124-156 with none of the special cases): near and far distance per axis, valid when every
// |d.c| is in [1e-6, 1-1e-6].  Then all t are finite, so glm::min/max equal fminf/fmaxf up to the
// sign of a zero, which no comparison below can see.  lo = {min.xyz, .}, hi = {max.xyz, .}
struct GeneralSlabs {
    float nx, ny, nz, fx, fy, fz;
    float tMin, tMax;
    bool overlap;
};
__device__ __forceinline__ GeneralSlabs general_slabs(f3 o, f3 dinv, float4 lo, float4 hi) {
    const float t1x = (lo.x - o.x) * dinv.x, t1y = (lo.y - o.y) * dinv.y, t1z = (lo.z - o.z) * dinv.z;
    const float t2x = (hi.x - o.x) * dinv.x, t2y = (hi.y - o.y) * dinv.y, t2z = (hi.z - o.z) * dinv.z;
    GeneralSlabs g;
    g.nx = fminf(t1x, t2x); g.ny = fminf(t1y, t2y); g.nz = fminf(t1z, t2z);
    g.fx = fmaxf(t1x, t2x); g.fy = fmaxf(t1y, t2y); g.fz = fmaxf(t1z, t2z);
    const float dx = g.fx - g.nx, dy = g.fy - g.ny, dz = g.fz - g.nz;
    g.overlap = (dy + dz > g.fz - g.ny) & (dz + dx > g.fx - g.nz) & (dx + dy > g.fy - g.nx);
    g.tMin = fmaxf(fmaxf(g.nx, g.ny), g.nz);
    g.tMax = fminf(fminf(g.fx, g.fy), g.fz);
    return g;
}
__device__ __forceinline__ bool box_hit_general(f3 o, f3 dinv, float4 lo, float4 hi, float& tMin) {
    const GeneralSlabs g = general_slabs(o, dinv, lo, hi);
    tMin = g.tMin;
    return g.overlap & (g.tMax >= 0.f) & (g.tMax >= g.tMin);
}
#endif  // __HIPCC__

}  // namespace rs
