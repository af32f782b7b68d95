// indirect_spatial.hip -- spatial reuse of ReSTIR-GI's reservoirs (rs_indirect_spatial, rs_internal.h): after the path kernel of an
// rs_restir_indirect call has written the temporal buffer T, every pixel merges up to 16 neighbours' reservoirs into its own by
// reconnecting the neighbour's sample point xs to its own visible point, each weight corrected by the Jacobian of that shift, tests
// the winner's visibility once and shades the result.  The reference allocates devIndSpatialReservoir (restir.cu:15) and never writes
// it; the rule is include/restir_hip.h's, at rs_restir_set_indirect_spatial.  The switch, k_spatial_indirect and the entry points that
// are only about this; gi.hip launches the pass behind launch_path.
#include "rs_light_history.h"
#include "rs_bsdf.h"
#include "rs_disk_tap.h"

using namespace rs;

namespace {

// { taking part, accepted, failed the neighbour test, ns == 0, Jacobian, horizon, walked, blocked }: each counter is kRaySub partial
// ones, 64 B apart, as the revalidation passes' are
constexpr int kGiStats = 8;
constexpr int kStatWords = kGiStats * kRaySub * kRayStride;
__device__ __forceinline__ unsigned long long* stat_of(unsigned long long* stats, int k) { return stats + ((size_t)k * kRaySub + blockIdx.x % kRaySub) * kRayStride; }
__device__ __forceinline__ int wave_sum(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;                                                   // lane 0 holds the sum
}

constexpr int kGiLanes = 256;

// The winners' walks: 1 = a block compacts its walkers through LDS into dense slots, as k_revalidate_indirect does, and hands the
// verdicts back through LDS; 0 = every wave walks its own lanes' segments where they are.  Measured at 1080p on the Sponza-class scene,
// where four lanes in five walk: a tie (7.24 against 7.23 ms at 5 taps, 8.26 against 8.25 at 16; profiles/indirect_spatial.log).
#ifndef RS_GI_SPATIAL_COMPACT
#define RS_GI_SPATIAL_COMPACT 1
#endif

struct RecordPlanes { float4* xv; float4* nv; float4* wo; int* mat; };      // all null: nothing is recorded

struct GiSample { f3 Lo, xv, nv, xs, ns; };
__device__ __forceinline__ bool weight_invalid(float W) { return is_nan_or_inf(W) || W < 0.f; }      // Reservoir::invalid (restir.h:51-53)

// One lane per pixel in k_path's layout (32x8 pixels per block, an 8x8 tile per wave), because the receiver's surface is k_path's own:
// the lane seeds k_path's engine (looper, index, 0), takes the same camera_sample and walks the primary ray again with the packet walk,
// then the material and the flip of restir.cu:286-288.  k_path itself stays the kernel it is.  Then, in this order: the tap loop (the
// gather: per tap three draws, the exact tap, four G-buffer words and up to 68 bytes of the neighbour's record); the winners' walks,
// only for lanes that adopted a sample; store, shade, accumulate.  A lane that does not take part copies T[i] to S[i] and moves the
// path kernel's value from temporalImage into the caller's image.  Nobody writes T while the kernel runs and a lane writes only its
// own slot of S and its own pixel.  LDS (compacting form): 2 x 256 float4 + 256 verdicts + 4 counts = 9 232 B.
template <bool TEX, bool SOBOL>
__global__ void __launch_bounds__(kGiLanes) k_spatial_indirect(DevScene s, CamParams cam, GBufView g, const rs_indirect_reservoir* __restrict__ T,
                                                               rs_indirect_reservoir* __restrict__ S, const float* __restrict__ temporalImage,
                                                               float* __restrict__ image, int looper, int iter, int taps, float radius, int tilesX,
                                                               unsigned long long* stats, RecordPlanes rec) {
#if RS_GI_SPATIAL_COMPACT
    __shared__ float4 sRay[2 * kGiLanes];
    __shared__ int sOcc[kGiLanes];
    __shared__ int sCount[kGiLanes / 64];
#endif
    int x, y;
    const int lane = pixel_of_lane(tilesX, 0, x, y);
    const int W = cam.width, H = cam.height;
    const bool inside = x < W && y < H;
    const int index = y * W + x;

    // 1. the receiver: what k_path computed at its primary hit in this call
    using PathSampler = typename PathSamplerOf<SOBOL>::type;
    PathSampler pathRng = PathSampler::seeded(s.sampleSeq, looper, index, 0);
    const f4 r4 = pathRng.uniform4();
    const Ray ray = camera_sample(cam, x, y, r4.x, r4.y);
    const Hit h = trace_closest_packet(s, ray, inside);         // all 64 lanes take part in the wave's walk
    const f3 wo = -ray.d;
    bool part = false;
    SurfMat mat = empty_surf_mat();
    f3 xvq = splat(0.f), nvq = splat(0.f);
    if (inside && h.primId != kNullPrim) {
        f3 norm = h.norm;
        mat = TEX ? textured_material(s, h, norm) : plain_material(s, h.matId);
        if (mat.type != 4 && mat.type != 2) {                   // neither Light nor Dielectric
            part = true;
            xvq = h.pos;
            nvq = dot(norm, wo) < 0.f ? -norm : norm;
        }
    }
    if (rec.xv && inside) {
        rec.xv[index] = make_float4(xvq.x, xvq.y, xvq.z, 0.f);
        rec.nv[index] = make_float4(nvq.x, nvq.y, nvq.z, 0.f);
        rec.wo[index] = part ? make_float4(wo.x, wo.y, wo.z, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
        rec.mat[index] = part ? h.matId : -1;
    }

    // 2. start: R = T[i] as stored, after checkValidity
    GiSample smp;
    smp.Lo = smp.xv = smp.nv = smp.xs = smp.ns = splat(0.f);
    int M = 0;
    float Wt = 0.f;
    if (inside) {
        const float* f = reinterpret_cast<const float*>(T + index);
        smp.Lo = ld3(f); smp.xv = ld3(f + 3); smp.nv = ld3(f + 6); smp.xs = ld3(f + 9); smp.ns = ld3(f + 12);
        M = __float_as_int(f[15]); Wt = f[16];
        if (!part) {
            float* o = reinterpret_cast<float*>(S + index);
            st3(o, smp.Lo); st3(o + 3, smp.xv); st3(o + 6, smp.nv); st3(o + 9, smp.xs); st3(o + 12, smp.ns);
            o[15] = __int_as_float(M); o[16] = Wt;
            accumulate(image, index, ld3(temporalImage + (size_t)index * 3), iter);
        }
    }
    bool adopted = false;
    int nAccepted = 0, nFailed = 0, nNoPoint = 0, nJacobian = 0, nHorizon = 0;
    if (part) {
        if (weight_invalid(Wt)) { Wt = 0.f; M = 0; }
        SamplerT<SOBOL> rng = SamplerT<SOBOL>::seeded(s.sampleSeq, looper, index, RS_GI_SPATIAL_DIM);
        const int idC = g.primId[index];
        const f3 nC = ld3(g.normal + (size_t)index * 3);
        const float dC = g.depth[index];
#pragma unroll 1
        for (int t = 0; t < taps; t++) {
            // 3. three draws per tap, accepted or not; the tap of findSpatialNeighborDisk in its exact form
            const f2 r2 = rng.uniform2();
            const float u = rng.uniform();
            int px, py;
            disk_tap_exact(r2.x, r2.y, radius, x, y, px, py);
            const bool inb = (px >= 0) & (px < W) & (py >= 0) & (py < H) & !((px == x) & (py == y));
            bool same = false;
            int p = 0;
            if (inb) {                                          // the reference's test (restir.cu:58-83)
                p = py * W + px;
                same = g.primId[p] == idC && !(dot(nC, ld3(g.normal + (size_t)p * 3)) < .9f) && !(gabs(dC - g.depth[p]) > dC * .1f);
            }
            if (!same) { nFailed++; continue; }
            // 4. the candidate N = T[p]
            const float* f = reinterpret_cast<const float*>(T + p);
            const float NW = f[16];
            if (weight_invalid(NW)) continue;
            float w = 0.f;
            f3 xs = splat(0.f), ns = splat(0.f);
            if (NW > 0.f) {
                xs = ld3(f + 9); ns = ld3(f + 12);
                if (ns.x == 0.f && ns.y == 0.f && ns.z == 0.f) { nNoPoint++; continue; }     // the first bounce left the scene
                const f3 vn = ld3(f + 3) - xs, vq = xvq - xs;
                const float dn2 = dot(vn, vn), dq2 = dot(vq, vq);
                const float an = gabs(dot(ns, vn)), aq = gabs(dot(ns, vq));
                const float jac = ((aq / sqrtf(dq2)) * dn2) / ((an / sqrtf(dn2)) * dq2);
                if (is_nan_or_inf(jac) || jac > RS_GI_SPATIAL_JACOBIAN_MAX) { nJacobian++; continue; }
                if (dot(nvq, vq) >= 0.f) { nHorizon++; continue; }                           // xs is not above the receiver's horizon
                w = NW * jac;
            }
            // 5. Reservoir::merge (restir.h:61-68) with the shifted weight
            nAccepted++;
            Wt += w; M += __float_as_int(f[15]);
            if (u * Wt < w) {
                smp.Lo = ld3(f); smp.xs = xs; smp.ns = ns;
                smp.xv = xvq; smp.nv = nvq;
                adopted = true;
            }
        }
    }

    // 6. visibility, once, on the winner: testOcclusion(xv_q, xs) for the lanes whose final sample came from a neighbour
    const bool walk = part && adopted;
    bool blocked = false;
#if RS_GI_SPATIAL_COMPACT
    {
        const int wave = threadIdx.x >> 6;
        const unsigned long long bWalk = __ballot(walk);
        if (lane == 0) sCount[wave] = __popcll(bWalk);
        __syncthreads();
        const int c0 = sCount[0], c1 = sCount[1], c2 = sCount[2], c3 = sCount[3];
        const int count = c0 + c1 + c2 + c3;
        const int before = (wave > 0 ? c0 : 0) + (wave > 1 ? c1 : 0) + (wave > 2 ? c2 : 0);
        const int slot = before + __popcll(bWalk & ((1ull << lane) - 1ull));
        if (walk) {                                             // slot < count <= 256
            sRay[slot] = make_float4(xvq.x, xvq.y, xvq.z, __int_as_float((int)threadIdx.x));
            sRay[kGiLanes + slot] = make_float4(smp.xs.x, smp.xs.y, smp.xs.z, 0.f);
        }
        __syncthreads();
        if ((int)(threadIdx.x & ~63u) < count) {                // wave-uniform: a wave without a ray walks nothing
            const bool mine = (int)threadIdx.x < count;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (mine) { a = sRay[threadIdx.x]; b = sRay[kGiLanes + threadIdx.x]; }
            const bool occluded = trace_occluded_wave(s, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mine);
            if (mine) sOcc[__float_as_int(a.w)] = occluded ? 1 : 0;      // a.w: a thread of this block that set `walk`, < 256
        }
        __syncthreads();
        if (walk) blocked = sOcc[threadIdx.x] != 0;
    }
#else
    blocked = trace_occluded_wave(s, xvq, smp.xs, walk) && walk;
#endif
    if (blocked) Wt = 0.f;                                      // the weight is zeroed, the reservoir is not cleared

    // 7. store and shade (restir.cu:399-412, the non-delta factor: a receiver that takes part is never Dielectric)
    if (part) {
        float* o = reinterpret_cast<float*>(S + index);
        st3(o, smp.Lo); st3(o + 3, smp.xv); st3(o + 6, smp.nv); st3(o + 9, smp.xs); st3(o + 12, smp.ns);
        o[15] = __int_as_float(M); o[16] = Wt;
        f3 indirect = splat(0.f);
        if (!weight_invalid(Wt)) {
            const f3 primWi = normalize(smp.xs - smp.xv);
            indirect = ((smp.Lo / luminance(smp.Lo)) * Wt) / (float)M;
            indirect = indirect * (material_bsdf(mat, smp.nv, wo, primWi) * sat_dot(smp.nv, primWi));
        }
        if (any_nan_or_inf(indirect)) indirect = splat(0.f);
        accumulate(image, index, indirect, iter);
    }

    // 8. the counters: one atomic per wave each
    const unsigned long long bPart = __ballot(part);
    if (!bPart) return;                                         // wave-uniform
    const int sums[5] = { wave_sum(nAccepted), wave_sum(nFailed), wave_sum(nNoPoint), wave_sum(nJacobian), wave_sum(nHorizon) };
    const unsigned long long bWalked = __ballot(walk), bBlocked = __ballot(blocked);
    if (lane == 0) {
        atomicAdd(stat_of(stats, 0), (unsigned long long)__popcll(bPart));
        for (int k = 0; k < 5; k++) if (sums[k]) atomicAdd(stat_of(stats, 1 + k), (unsigned long long)sums[k]);
        if (bWalked) atomicAdd(stat_of(stats, 6), (unsigned long long)__popcll(bWalked));
        if (bBlocked) atomicAdd(stat_of(stats, 7), (unsigned long long)__popcll(bBlocked));
    }
}

int read_stats(const rs_indirect_spatial& v, unsigned long long out[kGiStats]) {
    unsigned long long host[kStatWords];
    RS_HIP(hipMemcpy(host, v.dStats, sizeof(host), hipMemcpyDeviceToHost));
    for (int k = 0; k < kGiStats; k++) {
        out[k] = 0;
        for (int i = 0; i < kRaySub; i++) out[k] += host[((size_t)k * kRaySub + i) * kRayStride];
    }
    return 0;
}

}  // namespace

void rs_indirect_spatial_free(rs_indirect_spatial& v) {
    rs_dev_free(v.resv); rs_dev_free(v.temporalImage); rs_dev_free(v.dStats); rs_dev_free(v.recorded); rs_dev_free(v.recordedMat);
}

// the pass runs iff the switch is on and reuse & 2 -- on the first frame as well, as the DI spatial pass does; with the switch off
// reuse & 2 stays ignored, as in the reference
bool rs_indirect_spatial_runs(rs_restir* r, int reuse) {
    r->indSpatial.launchedLast = false;
    return r->indSpatial.on && (reuse & 2);
}

int rs_indirect_spatial_after_path(rs_restir* r, const rs_scene* scene, const rs_camera* cam, const GBufView& g, const rs_indirect_reservoir* temporal,
                                   float* image, int iter, int looper) {
    rs_indirect_spatial& v = r->indSpatial;
    const int W = r->width, H = r->height;
    const int tilesX = (W + 31) / 32, tilesY = (H + 7) / 8;
    const CamParams cp = rs_make_cam_params(cam);
    const size_t n = (size_t)W * H;
    RS_HIP(hipMemsetAsync(v.dStats, 0, kStatWords * sizeof(unsigned long long), rs_stream()));
    RecordPlanes rec{ nullptr, nullptr, nullptr, nullptr };
    if (v.recorded) rec = RecordPlanes{ v.recorded, v.recorded + n, v.recorded + 2 * n, v.recordedMat };
    const dim3 grid(tilesX * tilesY), block(kGiLanes);
    rs_dispatch([&](auto TEX, auto SOBOL) {
        hipLaunchKernelGGL((k_spatial_indirect<TEX(), SOBOL()>), grid, block, 0, rs_stream(), scene->dev, cp, g, temporal, v.resv, v.temporalImage, image,
                           looper, iter, v.taps, v.radius, tilesX, v.dStats, rec);
    }, scene->textured, scene->dev.sampleSeq != nullptr);
    v.launchedLast = true;
    return 0;
}

// behind rs_walk_counters_sum, which has waited for the stream
int rs_indirect_spatial_add_rays(rs_restir* r, unsigned long long* rays) {
    if (!rays || !r->indSpatial.launchedLast) return 0;
    unsigned long long st[kGiStats];
    RS_TRY(read_stats(r->indSpatial, st));
    *rays += st[6];
    return 0;
}

extern "C" {

// Everything that can fail comes before anything of the object changes.
int rs_restir_set_indirect_spatial(rs_restir* r, int enable, int taps, float radius) {
    RS_SCOPE(r);
    if (taps > RS_GI_SPATIAL_MAX_TAPS) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_restir_set_indirect_spatial: at most 16 taps");
    if (is_nan_or_inf(radius) || radius > 64.f) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_restir_set_indirect_spatial: the radius is finite and at most 64 pixels");
    if (!r) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_restir_set_indirect_spatial: null");
    RS_TRY(refuse_while_capturing("rs_restir_set_indirect_spatial"));
    rs_indirect_spatial& v = r->indSpatial;
    const bool on = enable != 0;
    if (on && !v.resv) {
        const size_t n = (size_t)r->width * r->height;
        rs_indirect_reservoir* resv = nullptr;
        float* img = nullptr;
        unsigned long long* stats = nullptr;
        int e = rs_dev_alloc(&resv, n);
        if (!e) e = rs_dev_alloc(&img, n * 3);
        if (!e) e = rs_dev_alloc(&stats, kStatWords);
        if (!e) e = rs_check_hip(hipMemset(resv, 0, n * sizeof(rs_indirect_reservoir)), "hipMemset");
        if (!e) e = rs_check_hip(hipMemset(img, 0, n * 3 * sizeof(float)), "hipMemset");
        if (!e) e = rs_check_hip(hipMemset(stats, 0, kStatWords * sizeof(unsigned long long)), "hipMemset");
        if (e) { rs_dev_free(resv); rs_dev_free(img); rs_dev_free(stats); return e; }
        v.resv = resv; v.temporalImage = img; v.dStats = stats;
    }
    v.on = on;
    v.taps = taps <= 0 ? 5 : taps;
    v.radius = radius <= 0.f ? 5.f : radius;
    v.launchedLast = false;
    return 0;
}

int rs_restir_get_indirect_spatial(const rs_restir* r, int* enabled, int* taps, float* radius) {
    if (!r || !enabled) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_restir_get_indirect_spatial: null argument");
    *enabled = r->indSpatial.on ? 1 : 0;
    if (taps) *taps = r->indSpatial.taps;
    if (radius) *radius = r->indSpatial.radius;
    return 0;
}

int rs_restir_download_indirect_spatial(rs_restir* r, rs_indirect_reservoir* host) {
    RS_SCOPE(r);
    if (!r || !host || !r->indSpatial.resv) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_restir_download_indirect_spatial: bad argument");
    RS_HIP(hipStreamSynchronize(rs_stream()));
    RS_HIP(hipMemcpy(host, r->indSpatial.resv, (size_t)r->width * r->height * sizeof(rs_indirect_reservoir), hipMemcpyDeviceToHost));
    return 0;
}

// test hook: the eight counters of the last rs_restir_indirect call; zeros when that call did not run the pass
int rs_debug_restir_indirect_spatial(rs_restir* r, unsigned long long out[8]) {
    RS_SCOPE(r);
    if (!r || !out) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_restir_indirect_spatial: null argument");
    for (int k = 0; k < kGiStats; k++) out[k] = 0;
    if (!r->indSpatial.launchedLast) return 0;
    RS_HIP(hipStreamSynchronize(rs_stream()));
    return read_stats(r->indSpatial, out);
}

// ... and whether that call ran it at all
int rs_debug_restir_indirect_spatial_launched(rs_restir* r, int* launched) {
    if (!r || !launched) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_restir_indirect_spatial_launched: null argument");
    *launched = r->indSpatial.launchedLast ? 1 : 0;
    return 0;
}

// test hook: the receiver's surface of the last call that ran the pass.  The planes are recorded only once somebody has asked: the
// first call (with or without outputs) allocates them, and a call with every output null does nothing else.
int rs_debug_restir_indirect_primary(rs_restir* r, float* xv4, float* nv4, float* wo4, int* matId) {
    RS_SCOPE(r);
    if (!r) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_restir_indirect_primary: null");
    rs_indirect_spatial& v = r->indSpatial;
    const size_t n = (size_t)r->width * r->height;
    const bool asks = xv4 || nv4 || wo4 || matId;
    if (!v.recorded) {
        if (asks) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_restir_indirect_primary: nothing recorded yet (call it once with null outputs before the frame)");
        RS_TRY(refuse_while_capturing("rs_debug_restir_indirect_primary"));
        float4* planes = nullptr;
        int* mat = nullptr;
        int e = rs_dev_alloc(&planes, 3 * n);
        if (!e) e = rs_dev_alloc(&mat, n);
        if (!e) e = rs_check_hip(hipMemset(planes, 0, 3 * n * sizeof(float4)), "hipMemset");
        if (!e) e = rs_check_hip(hipMemset(mat, 0xff, n * sizeof(int)), "hipMemset");
        if (e) { rs_dev_free(planes); rs_dev_free(mat); return e; }
        v.recorded = planes; v.recordedMat = mat;
        return 0;
    }
    if (!asks) return 0;
    RS_HIP(hipStreamSynchronize(rs_stream()));
    if (xv4) RS_HIP(hipMemcpy(xv4, v.recorded, n * sizeof(float4), hipMemcpyDeviceToHost));
    if (nv4) RS_HIP(hipMemcpy(nv4, v.recorded + n, n * sizeof(float4), hipMemcpyDeviceToHost));
    if (wo4) RS_HIP(hipMemcpy(wo4, v.recorded + 2 * n, n * sizeof(float4), hipMemcpyDeviceToHost));
    if (matId) RS_HIP(hipMemcpy(matId, v.recordedMat, n * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

// host only: n draws of the library's own SamplerT<>::seeded(table, iter, index, dim) -- the default engine when the scene is null or
// has no table
int rs_debug_seeded_uniforms(const rs_scene* scene, int iter, int index, int dim, int n, float* out) {
    if (n < 0 || (n > 0 && !out) || dim < 0) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_seeded_uniforms: bad argument");
    if (scene && !scene->hSampleSeq.empty()) {
        const size_t rows = scene->hSampleSeq.size() / kSobolSampleDim;
        if (iter < 0 || (size_t)iter >= rows || (size_t)iter * kSobolSampleDim + dim + n > scene->hSampleSeq.size())
            return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_seeded_uniforms: beyond the Sobol table");
        SamplerT<true> s = SamplerT<true>::seeded(scene->hSampleSeq.data(), iter, index, dim);
        for (int k = 0; k < n; k++) out[k] = s.uniform();
        return 0;
    }
    SamplerT<false> s = SamplerT<false>::seeded(nullptr, iter, index, dim);
    for (int k = 0; k < n; k++) out[k] = s.uniform();
    return 0;
}

}  // extern "C"
