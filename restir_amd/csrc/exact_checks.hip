// exact_checks.hip -- test hooks for rs_exact.h: the short forms of reciprocal, quotient and square root against the compiler's
// correctly rounded operators (-fhip-fp32-correctly-rounded-divide-sqrt), on every operand the guards of rs_exact.h admit; and for
// the generator's step (rs_math.h Rng) against the form it replaced, on every state.
#include "rs_internal.h"
#include "rs_exact.h"

using namespace rs;

namespace {

// out[0] results that differ, out[1] operands (pairs) compared, out[2] reserved (0)
__device__ __forceinline__ void tally(unsigned long long* out, unsigned long long bad, unsigned long long n, unsigned long long badExcluded) {
    for (int off = 32; off > 0; off >>= 1) { bad += __shfl_down(bad, off); n += __shfl_down(n, off); badExcluded += __shfl_down(badExcluded, off); }
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicAdd(out, bad);
        atomicAdd(out + 1, n);
        if (badExcluded) atomicAdd(out + 2, badExcluded);
    }
}

// op 0: 1 / d for every float d with |d| in [2^-60, 2^60)
// op 1: sqrt(x) for every float x in [2^-60, 2^60)
__global__ void __launch_bounds__(256) k_check_unary(int op, unsigned long long* out) {
    unsigned long long bad = 0, n = 0, badExcluded = 0;
    const unsigned long long span = kExactHi - kExactLo;
    for (unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; k < span; k += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned bits = kExactLo + (unsigned)k;
        const float v = __uint_as_float(bits);
        if (op == 0) {
            n += 2;
            bad += __float_as_uint(rcp_refined(v)) == __float_as_uint(1.f / v) ? 0 : 1;
            bad += __float_as_uint(rcp_refined(-v)) == __float_as_uint(1.f / -v) ? 0 : 1;
        }
        else { n++; bad += __float_as_uint(sqrt_refined(v)) == __float_as_uint(sqrtf(v)) ? 0 : 1; }
    }
    tally(out, bad, n, badExcluded);
}

// op 2: x / d for d = 1.sd * 2^expD over the significands sd in [firstSig, firstSig + gridDim.x) -- one per block -- and x = 1.sx * 2^expX
// over ALL 2^23 significands sx
// signs: bit 0 = negative numerators, bit 1 = negative denominator
__global__ void __launch_bounds__(256) k_check_division(unsigned firstSig, int expX, int expD, int signs, unsigned long long* out) {
    const unsigned sd = firstSig + blockIdx.x;
    const unsigned bd = ((unsigned)(127 + expD) << 23) | sd | ((signs & 2) ? 0x80000000u : 0u);
    const float d = __uint_as_float(bd);
    const float y = rcp_refined(d);
    const unsigned ex = ((unsigned)(127 + expX) << 23) | ((signs & 1) ? 0x80000000u : 0u);
    unsigned long long bad = 0, n = 0;
    for (unsigned sx = threadIdx.x; sx < (1u << 23); sx += 256) {
        const float x = __uint_as_float(ex | sx);
        bad += __float_as_uint(div_by_rcp(x, d, y)) == __float_as_uint(x / d) ? 0 : 1;
        n++;
    }
    tally(out, bad, n, 0);
}

// ---- the generator's step on y = x - 1 (rs_math.h Rng) against the fold on x it replaced, and the two comparisons of the RIS loop that
// take a draw before its division (rs_surface.h sample_light_with, restir.hip ris_pixel) against the comparisons of the divided draw.
// The step as it was, written out: x' = 48271 x mod (2^31 - 1) and the draw float(x' - 1) / 2^31.
RS_HD uint32_t reference_step(uint32_t x) {
    const uint64_t p = (uint64_t)x * 48271u;
    uint32_t s = (uint32_t)(p & 0x7fffffffu) + (uint32_t)(p >> 31);
    if (s >= 2147483647u) s -= 2147483647u;
    return s;
}
RS_HD float reference_draw(uint32_t next) { return (float)(next - 1u) / 2147483648.f; }
RS_HD uint32_t float_bits(float f) { union { float f; uint32_t u; } v; v.f = f; return v.u; }
RS_HD float bits_float(uint32_t u) { union { float f; uint32_t u; } v; v.u = u; return v.f; }

constexpr unsigned kRngCheckPerState = 3 + 2 + 6 + 8;

// the results that differ for the state x in [1, 2^31 - 2]: of kRngCheckPerState compared
RS_HD unsigned rng_forms_differ(uint32_t x) {
    const int lights[6] = { 1, 3, 1024, 1500, 10240, (1 << 24) + 1 };
    // 0, the smallest subnormal, 2^-31, 0.5, the float below 1, 1, 2, a NaN
    const uint32_t probBits[8] = { 0u, 1u, 0x30000000u, 0x3f000000u, 0x3f7fffffu, 0x3f800000u, 0x40000000u, 0x7fc00000u };
    const uint32_t next = reference_step(x);
    const float draw = reference_draw(next);
    Rng a = Rng::from_state(x), b = a;
    const float u = a.uniform(), raw = b.raw();
    unsigned bad = 0;
    bad += a.state() != next;
    bad += float_bits(u) != float_bits(draw);
    bad += b.state() != next;
    RngOnX c = RngOnX::from_state(x);                    // the form on x (k_path, procedural_texture)
    const float ux = c.uniform();
    bad += c.state() != next;
    bad += float_bits(ux) != float_bits(draw);
    for (int i = 0; i < 6; i++) {
        const int n = lights[i];
        bad += sampler_entry((float)n * (1.f / kRngRawScale), raw, n) != imin(f2i((float)n * draw), n - 1);
    }
    for (int i = 0; i < 8; i++) {
        const float prob = bits_float(probBits[i]);
        bad += (raw < prob * kRngRawScale) != (draw < prob);
    }
    return bad;
}

// every state of the period; out[0] results that differ, out[1] results compared
__global__ void __launch_bounds__(256) k_check_rng_step(unsigned long long* out) {
    unsigned long long bad = 0, n = 0;
    for (unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x + 1ull; k <= 0x7ffffffeull; k += (unsigned long long)gridDim.x * blockDim.x) {
        bad += rng_forms_differ((uint32_t)k);
        n += kRngCheckPerState;
    }
    tally(out, bad, n, 0);
}

}  // namespace

extern "C" {

int rs_debug_rng_step_mismatches(unsigned long long* out2) {
    rs_ctx_scope scope(nullptr);
    if (!out2) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_rng_step_mismatches: null");
    unsigned long long* d = nullptr;
    RS_TRY(rs_dev_alloc(&d, 3));
    RS_HIP(hipMemsetAsync(d, 0, 24, rs_stream()));
    hipLaunchKernelGGL(k_check_rng_step, dim3(4096), dim3(256), 0, rs_stream(), d);
    int err = rs_after_launch("rs_debug_rng_step_mismatches");
    if (!err) err = rs_check_hip(hipStreamSynchronize(rs_stream()), "rs_debug_rng_step_mismatches: synchronize");
    if (!err) err = rs_check_hip(hipMemcpy(out2, d, 16, hipMemcpyDeviceToHost), "rs_debug_rng_step_mismatches: copy");
    rs_dev_free(d);
    return err;
}

int rs_debug_rng_step_host_mismatches(unsigned first, unsigned count, unsigned long long* out2) {
    if (!out2 || first < 1u || count == 0u || first > 0x7ffffffeu || count - 1u > 0x7ffffffeu - first)
        return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_rng_step_host_mismatches: null, no state, or states outside [1, 2^31 - 2]");
    unsigned long long bad = 0;
    for (unsigned k = 0; k < count; k++) bad += rng_forms_differ(first + k);
    out2[0] = bad;
    out2[1] = (unsigned long long)count * kRngCheckPerState;
    return 0;
}

int rs_debug_exact_ops_mismatches(int op, unsigned firstSig, unsigned countSig, int expX, int expD, unsigned long long* out3) {
    rs_ctx_scope scope(nullptr);
    if (!out3 || op < 0 || op > 5) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_exact_ops_mismatches: bad argument");
    if (op >= 2 && (countSig == 0 || countSig > (1u << 16) || firstSig >= (1u << 23) || firstSig + countSig > (1u << 23) ||
                    expX < -60 || expX > 59 || expD < -60 || expD > 59))
        return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_exact_ops_mismatches: significands beyond 2^23, more than 65536 per call, or an exponent outside [-60, 59]");
    unsigned long long* d = nullptr;
    RS_TRY(rs_dev_alloc(&d, 3));
    RS_HIP(hipMemsetAsync(d, 0, 24, rs_stream()));
    if (op >= 2) hipLaunchKernelGGL(k_check_division, dim3(countSig), dim3(256), 0, rs_stream(), firstSig, expX, expD, op - 2, d);
    else hipLaunchKernelGGL(k_check_unary, dim3(8192), dim3(256), 0, rs_stream(), op, d);
    int err = rs_after_launch("rs_debug_exact_ops_mismatches");
    if (!err) err = rs_check_hip(hipStreamSynchronize(rs_stream()), "rs_debug_exact_ops_mismatches: synchronize");
    if (!err) err = rs_check_hip(hipMemcpy(out3, d, 24, hipMemcpyDeviceToHost), "rs_debug_exact_ops_mismatches: copy");
    rs_dev_free(d);
    return err;
}

}
