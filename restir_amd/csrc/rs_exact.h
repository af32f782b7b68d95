// rs_exact.h -- correctly rounded FP32 division, reciprocal and square root without the compiler's scaled expansions, for operands in
// a guarded range; outside it the plain operator runs, so every function here returns the IEEE result for EVERY input -- the parity
// contract of rs_math.h is untouched, only the instruction count changes.
//
// The compiler's x / d is v_div_scale x 2, v_rcp, five fused steps, v_div_fmas, v_div_fixup (10 instructions, 30 for the three
// quotients of a vector by one scalar: the scaling depends on numerator AND denominator, nothing is shared); its sqrtf is 16.
// With all operands in [2^-60, 2^60) no intermediate of the forms below leaves the normal range, and every operation in them (product,
// fused multiply-add, the hardware's estimates as functions of the significand) commutes with scaling by powers of two, so a statement
// about all significands at one exponent is a statement about the whole range.  The statements are established by EXHAUSTIVE comparison
// with the compiler's operators on gfx950 (rs_debug_exact_ops_mismatches, exact_checks.hip), not by an error analysis of v_rcp_f32 /
// v_sqrt_f32, whose documented accuracy is 1 ulp:
//   * reciprocal: y0 = v_rcp_f32(d), e = fma(-d, y0, 1), y = fma(e, y0, y0) is RN(1 / d) -- Markstein's refinement (1990; Muller et al.,
//     Handbook of Floating-Point Arithmetic, 5.3), whose one theoretical exception (a significand of all ones) does not occur with this
//     hardware's estimate: all 1 006 632 960 floats of the range agree (tests/test_gpu_exact_ops.py);
//   * quotient: with that y: q0 = x * y, rem = fma(-q0, d, x) (exact), q = fma(rem, y, q0) is RN(x / d) -- ALL 2^46 pairs of significands
//     agree (tools/verify_exact_division.py, half a minute of one MI355X; profiles/r03_exact_division_all_pairs.log), the test suite
//     runs a slice of it plus pairs at the edges of the exponent range;
//   * square root: s = v_sqrt_f32(x), then one ulp down or up by the sign of the two exact residuals -- the compiler's own refinement
//     without its range scaling and class test; every float of the range agrees.
// The guards are wave-uniform (__all): one scalar branch, no exec-mask region; a wave with one operand outside the range takes the
// compiler's operator for all its lanes.  Zero, negative numbers, infinity and NaN are outside the range by construction of the test.
// The RIS loop over the light table in LDS (restir.hip ris_pixel in k_ris_lds, the form of the headline frame) no longer pays one such
// branch per operation: it runs the short forms of a whole candidate unguarded, records the range of their operands and asks its wave
// once per candidate (ExactSpeculative, at the end of this file).  The two forms that gather their light records from memory, k_ris and
// k_ris_alias_lds, keep the per-operation guards (why: restir.hip ris_pixel), like every other caller.
// Whole frames whose waves take the fallback, mix lanes inside and outside the range or carry `unused` lanes are compared with the oracle
// bit for bit in tests/test_gpu_parameter_extremes.py (the cases of tests/extreme_cases.py: roughness 0 and 1e-6 on all or a part of the
// scene, radiances from a denormal to 3e38, an emitter above 2^60 beside an ordinary one).
#ifndef RS_MATH_H_BODY
#include "rs_math.h"        // which includes this file once its vector type and operators are defined (normalize / length use the forms below)
#elif !defined(RS_EXACT_H_BODY)
#define RS_EXACT_H_BODY

namespace rs {

// -DRS_EXACT_PLAIN: every function below is the compiler's operator (A/B measurements: tools/build_variant.sh plain "-DRS_EXACT_PLAIN").
// The short forms are correct by exhaustive test of gfx950's v_rcp_f32 / v_sqrt_f32, not by analysis: a device pass for any other target
// takes the compiler's operators until tests/test_gpu_exact_ops.py has passed there (the host pass of a .hip file never runs them).
#if defined(RS_EXACT_PLAIN) || (defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__))
#define RS_EXACT_GUARD(cond) ((void)(cond), false)
#else
#define RS_EXACT_GUARD(cond) __all(cond)
#endif

constexpr unsigned kExactLo = 0x21800000u;       // 2^-60
constexpr unsigned kExactHi = 0x5D800000u;       // 2^60

// positive, normal, inside [2^-60, 2^60): one unsigned comparison on the bit pattern (negative numbers, NaN, infinity and zero fail it)
__device__ __forceinline__ bool exact_range(unsigned bits) { return bits - kExactLo < kExactHi - kExactLo; }

__device__ __forceinline__ float rcp_refined(float d) {
    const float y0 = __builtin_amdgcn_rcpf(d);
    const float e = __builtin_fmaf(-d, y0, 1.f);
    return __builtin_fmaf(e, y0, y0);
}
__device__ __forceinline__ float div_by_rcp(float x, float d, float y) {
    const float q0 = x * y;
    const float rem = __builtin_fmaf(-q0, d, x);
    return __builtin_fmaf(rem, y, q0);
}

// the same range for |x|: the forms are sign-symmetric (round-to-nearest is, and so is the hardware's estimate: the reciprocal check runs
// over the negative floats of the range as well)
__device__ __forceinline__ bool exact_range_abs(unsigned bits) { return (bits & 0x7FFFFFFFu) - kExactLo < kExactHi - kExactLo; }

// 1.f / d
__device__ __forceinline__ float rcp_exact(float d) {
    const unsigned b = __float_as_uint(d);
    if (RS_EXACT_GUARD(exact_range(b))) return rcp_refined(d);          // wave-uniform: one scalar branch, no exec mask
    return 1.f / d;
}

// x / d
__device__ __forceinline__ float div_exact(float x, float d, bool unused = false) {
    const unsigned bx = __float_as_uint(x), bd = __float_as_uint(d);
    if (RS_EXACT_GUARD(unused || (exact_range(bx) && exact_range(bd)))) return div_by_rcp(x, d, rcp_refined(d));
    return x / d;
}

// g / d, three quotients by one denominator (f3 operator/(f3, float)).  unused: the caller discards this lane's quotients whatever they
// are (a candidate whose pdf is <= 0), so the lane does not keep its wave from the short form.
__device__ __forceinline__ f3 div3_exact(f3 g, float d, bool unused = false) {
    const unsigned bx = __float_as_uint(g.x), by = __float_as_uint(g.y), bz = __float_as_uint(g.z), bd = __float_as_uint(d);
    const unsigned lo = min(min(bx, by), min(bz, bd)), hi = max(max(bx, by), max(bz, bd));
    if (RS_EXACT_GUARD(unused || (lo >= kExactLo && hi < kExactHi))) {
        const float y = rcp_refined(d);
        return mk3(div_by_rcp(g.x, d, y), div_by_rcp(g.y, d, y), div_by_rcp(g.z, d, y));
    }
    return g / d;
}

// the same for operands of either sign: 1 / d per component of a direction, g / d of a difference vector
__device__ __forceinline__ f3 rcp3_exact_signed(f3 d) {
    if (RS_EXACT_GUARD(exact_range_abs(__float_as_uint(d.x)) && exact_range_abs(__float_as_uint(d.y)) && exact_range_abs(__float_as_uint(d.z))))
        return mk3(rcp_refined(d.x), rcp_refined(d.y), rcp_refined(d.z));
    return mk3(1.f / d.x, 1.f / d.y, 1.f / d.z);
}
__device__ __forceinline__ f3 div3_exact_signed(f3 g, float d) {
    if (RS_EXACT_GUARD(exact_range_abs(__float_as_uint(g.x)) && exact_range_abs(__float_as_uint(g.y)) && exact_range_abs(__float_as_uint(g.z)) &&
                       exact_range_abs(__float_as_uint(d)))) {
        const float y = rcp_refined(d);
        return mk3(div_by_rcp(g.x, d, y), div_by_rcp(g.y, d, y), div_by_rcp(g.z, d, y));
    }
    return g / d;
}

__device__ __forceinline__ float sqrt_refined(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float down = __uint_as_float(__float_as_uint(s) - 1u), up = __uint_as_float(__float_as_uint(s) + 1u);
    const float rDown = __builtin_fmaf(-down, s, x), rUp = __builtin_fmaf(-up, s, x);
    float root = rDown <= 0.f ? down : s;
    root = rUp > 0.f ? up : root;
    return root;
}
// sqrtf(x)
__device__ __forceinline__ float sqrt_exact(float x) {
    if (RS_EXACT_GUARD(exact_range(__float_as_uint(x)))) return sqrt_refined(x);
    return sqrtf(x);
}

// ---- one guard for a whole sequence of operations (restir.hip ris_pixel) ------------------------------------------------------------
// A function written once over its arithmetic (sample_light_with, eval_bsdf_with) takes one of three sets of operations: ExactGuarded
// (each operation behind its own guard, as above), ExactPlain (the compiler's operators) and ExactSpeculative, which runs the short
// forms unguarded and only records the range of the operands it was given.  The caller asks the wave once, in_range_or_unused(), and
// evaluates the sequence again with ExactPlain if the answer is no: for operands in range both give the same bits, so how many
// operations one question covers does not matter, and out of range the speculative values are discarded unread.
//   * A lane whose results the caller discards whatever they are says so with set_unused(), from a test that involves none of these
//     operations (the facing test of a light sample; a pdf that came from the compiler's operators): its operands do not count.
//   * A numerator may also be +0 (bit pattern 0): with d in range y is finite and positive, q0 = +0 * y = +0, rem = fma(-0, d, +0) = +0,
//     q = fma(+0, y, +0) = +0, the IEEE quotient -- exact steps, nothing to round.  (-0 is refused: the form would return +0.)  A
//     candidate below the surface's horizon has the numerator +0, one lane in nine of a Sponza-class view.
//   * Implied and therefore not recorded: the argument of rcp_of_root is the root of a recorded x in [2^-60, 2^60), i.e. in [2^-30, 2^30].
#if defined(RS_EXACT_PLAIN) || (defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__))
constexpr bool kExactSpeculate = false;                 // callers run ExactGuarded alone, every operation of which is the compiler's
#else
constexpr bool kExactSpeculate = true;
#endif

struct ExactGuarded {
    static constexpr bool kWholeWave = false;           // (kWholeWave: dead lanes run along instead of leaving through an exec-mask region)
    __device__ __forceinline__ float sqrt(float x) { return sqrt_exact(x); }
    __device__ __forceinline__ float rcp_of_root(float r) { return rcp_exact(r); }
    __device__ __forceinline__ float div(float x, float d) { return div_exact(x, d); }
    __device__ __forceinline__ f3 div3(f3 g, float d, bool unused) { return div3_exact(g, d, unused); }
    __device__ __forceinline__ f3 normalize(f3 v) { return v * rcp_exact(sqrt_exact(dot(v, v))); }
    __device__ __forceinline__ void set_unused(bool) {}
};
struct ExactPlain {
    static constexpr bool kWholeWave = true;
    __device__ __forceinline__ float sqrt(float x) { return sqrtf(x); }
    __device__ __forceinline__ float rcp_of_root(float r) { return 1.f / r; }
    __device__ __forceinline__ float div(float x, float d) { return x / d; }
    __device__ __forceinline__ f3 div3(f3 g, float d, bool) { return g / d; }
    __device__ __forceinline__ f3 normalize(f3 v) { return v * (1.f / sqrtf(dot(v, v))); }
    __device__ __forceinline__ void set_unused(bool) {}
};
struct ExactSpeculative {
    static constexpr bool kWholeWave = true;
    unsigned lo = ~0u, loNum = ~0u, hi = 0u;            // min and max of the bit patterns; numerators' min apart, less one, so that 0 wraps past it
    bool unused = false;
    __device__ __forceinline__ void take(float x) { const unsigned b = __float_as_uint(x); lo = min(lo, b); hi = max(hi, b); }
    __device__ __forceinline__ void take_num(float x) { const unsigned b = __float_as_uint(x); loNum = min(loNum, b - 1u); hi = max(hi, b); }
    __device__ __forceinline__ float sqrt(float x) { take(x); return sqrt_refined(x); }
    __device__ __forceinline__ float rcp_of_root(float r) { return rcp_refined(r); }
    __device__ __forceinline__ float div(float x, float d) { take_num(x); take(d); return div_by_rcp(x, d, rcp_refined(d)); }
    __device__ __forceinline__ f3 div3(f3 g, float d, bool) {
        take_num(g.x); take_num(g.y); take_num(g.z); take(d);
        const float y = rcp_refined(d);
        return mk3(div_by_rcp(g.x, d, y), div_by_rcp(g.y, d, y), div_by_rcp(g.z, d, y));
    }
    __device__ __forceinline__ f3 normalize(f3 v) { const float r = sqrt(dot(v, v)); return v * rcp_of_root(r); }
    __device__ __forceinline__ void set_unused(bool u) { unused = u; }
    // wave-uniform: did every lane that uses its results give every operation operands in [2^-60, 2^60) (numerators: or +0)?
    __device__ __forceinline__ bool in_range_or_unused() const {
        return __all(unused | ((lo >= kExactLo) & (loNum >= kExactLo - 1u) & (hi < kExactHi)));      // (no exec-mask region for `unused`)
    }
};

}  // namespace rs

#endif  // RS_MATH_H_BODY / RS_EXACT_H_BODY
