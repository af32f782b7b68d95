// rs_disk_tap.h -- the exact tap of findSpatialNeighborDisk (restir.cu:47-55) for the spatial passes: restir.hip's phase B (radius 5,
// behind its hardware-trig estimate) and indirect_spatial.hip (any radius, this form alone).
#ifndef RS_DISK_TAP_H
#define RS_DISK_TAP_H
#include "rs_math.h"

#if defined(__HIPCC__)
namespace rs {

// sin and cos of theta in [0, 2*pi] in double precision: quadrant reduction with a two-term pi/2 and
// the classic degree-13/14 kernels (fdlibm k_sin / k_cos coefficients), < 1 ulp(double).  Rounded to
// float this is the correctly rounded sinf/cosf for all but ~1e-9 of the arguments.  A hand-rolled
// routine instead of OCML's sincos(double) because the latter costs 26 VGPRs (6 instead of 8 waves per
// SIMD for the whole spatial pass) for a path taken by ~0.03 % of the taps.
__device__ __forceinline__ void sincos_2pi(double t, double& sn, double& cs) {
    const double k = rint(t * 6.36619772367581382433e-01);                 // 2/pi
    double r = fma(-k, 1.57079632673412561417e+00, t);                      // pi/2 high (33 bits)
    r = fma(-k, 6.07710050650619224932e-11, r);                             // pi/2 low
    const double z = r * r;
    const double ps = -1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 +
                      z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10))));
    const double pc = 4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
                      z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))));
    const double s0 = r + r * z * ps;
    const double c0 = 1.0 - 0.5 * z + z * z * pc;
    const int q = (int)k & 3;
    sn = (q == 0) ? s0 : (q == 1) ? c0 : (q == 2) ? -s0 : -c0;
    cs = (q == 0) ? c0 : (q == 1) ? -s0 : (q == 2) ? -c0 : s0;
}

// exact evaluation of the tap: correctly rounded cos/sin, then the reference's float arithmetic
__device__ __forceinline__ void disk_tap_exact(float rx, float ry, float Radius, int x, int y, int& px, int& py) {
    const float rr = sqrtf(rx);
    const float theta = ry * kPi * 2.0f;
    double sd, cd;
    sincos_2pi((double)theta, sd, cd);
    px = f2i((float)x + .5f + ((float)cd * rr) * Radius);
    py = f2i((float)y + .5f + ((float)sd * rr) * Radius);
}

}  // namespace rs
#endif  // __HIPCC__
#endif  // RS_DISK_TAP_H
