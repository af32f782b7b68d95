// surface_checks.hip -- test hook for rs_surface.h: the functions the TEX / ENV kernel variants are built on (linear_sample,
// procedural_texture, to_sphere, to_plane, local_to_world), as they are, one lane per element of a batch, so that a test can hold each
// to the oracle's function on inputs a rendered frame never produces (tests/test_gpu_surface_ops.py).
#include "rs_internal.h"

using namespace rs;

namespace {

constexpr int kSurfaceOps = 5;
constexpr int kInWidth[kSurfaceOps] = { 2, 2, 2, 3, 6 }, kOutWidth[kSurfaceOps] = { 3, 3, 3, 2, 3 };

__global__ void __launch_bounds__(256) k_surface_ops(int op, int n, const float* __restrict__ in, float* __restrict__ out, TexRec tex) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (op == 3) {
        float u, v;
        to_plane(ld3(in + (size_t)i * 3), u, v);
        out[(size_t)i * 2] = u; out[(size_t)i * 2 + 1] = v;
        return;
    }
    f3 r;
    if (op == 0) r = linear_sample(tex, in[(size_t)i * 2], in[(size_t)i * 2 + 1]);
    else if (op == 1) r = procedural_texture(in[(size_t)i * 2], in[(size_t)i * 2 + 1]);
    else if (op == 2) r = to_sphere(in[(size_t)i * 2], in[(size_t)i * 2 + 1]);
    else r = local_to_world(ld3(in + (size_t)i * 6), ld3(in + (size_t)i * 6 + 3));
    out[(size_t)i * 3] = r.x; out[(size_t)i * 3 + 1] = r.y; out[(size_t)i * 3 + 2] = r.z;
}

}  // namespace

extern "C" int rs_debug_surface_ops(int op, int n, const float* in, float* out, int texWidth, int texHeight, const float* texels) {
    rs_ctx_scope scope(nullptr);
    if (op < 0 || op >= kSurfaceOps || n < 0 || n > (1 << 26) || !in || !out)
        return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_surface_ops: an op outside 0..4, n negative or above 2^26, or a null array");
    if (op == 0 && (texWidth <= 0 || texHeight <= 0 || !texels || (long long)texWidth * texHeight > (1ll << 26)))
        return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_surface_ops: linear_sample needs texels and a width and height above 0 (at most 2^26 texels)");
    if (n == 0) return 0;
    const size_t nin = (size_t)n * kInWidth[op], nout = (size_t)n * kOutWidth[op];
    const size_t ntex = op == 0 ? (size_t)texWidth * texHeight * 3 : 0;
    float *dIn = nullptr, *dOut = nullptr, *dTex = nullptr;
    int err = rs_dev_alloc(&dIn, nin);
    if (!err) err = rs_dev_alloc(&dOut, nout);
    if (!err && ntex) err = rs_dev_alloc(&dTex, ntex);
    if (!err) err = rs_check_hip(hipMemcpy(dIn, in, nin * sizeof(float), hipMemcpyHostToDevice), "rs_debug_surface_ops: copy in");
    if (!err && ntex) err = rs_check_hip(hipMemcpy(dTex, texels, ntex * sizeof(float), hipMemcpyHostToDevice), "rs_debug_surface_ops: copy texels");
    if (!err) {
        const TexRec tex{ dTex, op == 0 ? texWidth : 0, op == 0 ? texHeight : 0 };
        hipLaunchKernelGGL(k_surface_ops, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, rs_stream(), op, n, dIn, dOut, tex);
        err = rs_after_launch("rs_debug_surface_ops");
    }
    if (!err) err = rs_check_hip(hipStreamSynchronize(rs_stream()), "rs_debug_surface_ops: synchronize");
    if (!err) err = rs_check_hip(hipMemcpy(out, dOut, nout * sizeof(float), hipMemcpyDeviceToHost), "rs_debug_surface_ops: copy out");
    rs_dev_free(dTex); rs_dev_free(dOut); rs_dev_free(dIn);
    return err;
}
