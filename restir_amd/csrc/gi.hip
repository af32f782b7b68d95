// gi.hip -- the multi-bounce half of the reference:
//   singleKernelPT / pathTrace             src/pathtrace.cu:156-277,434-455
//   PTIndirectKernel / pathTraceIndirect   src/pathtrace.cu:330-432,478-497
//   ReSTIRIndirectKernel / ReSTIRIndirect  src/restir.cu:233-416,448-476   (Reservoir<IndirectLiSample>, temporal reuse)
//
// One lane per pixel, 8x8 pixel tile per wave.  The primary ray is coherent and uses the wave-cooperative packet
// walk; after the first bounce rays are incoherent, so continuation rays use the pair-cooperative per-lane walk of
// the reference's tree and shadow rays the shadow tree -- both wave-level services, which is why the path loop is
// run by the whole wave with per-lane `alive` flags instead of lanes breaking out of it.
// The three kernels share one path loop (path_loop below); what differs is cited at each switch.
// (A wavefront form -- path state in SoA queues, one launch per stage and bounce, ray queue bucketed by threaded order, a streaming walk
// that replaces finished rays -- was built in round 4: bit-exact, a tie on the Sponza-class scene and 15-20 % slower on the Bistro-class
// one; the walks cost the same either way.  EXPERIMENTS.md, commits d0141a4 and 220fdf1.)
#include "rs_internal.h"
#include "rs_bsdf.h"

using namespace rs;

namespace {

enum { kModePT = 0, kModePTIndirect = 1, kModeReSTIR = 2 };

// scene.h:358-362
__device__ inline float environment_map_pdf(const DevScene& s, f3 w) {
    const TexRec env = s.textures[s.envTex];
    float u, v;
    to_plane(w, u, v);
    return luminance(linear_sample(env, u, v)) * s.sumLightPowerInv * (float)env.width * (float)env.height * .5f;
}
// scene.h:121-126
__device__ inline float primitive_area(const DevScene& s, int prim) {
    const float* t = s.vertices + (size_t)prim * 9;
    const f3 v0 = ld3(t), v1 = ld3(t + 3), v2 = ld3(t + 6);
    return length(cross(v1 - v0, v2 - v0)) * .5f;
}

// The path loop's cold state lives in LDS, one column of 256 floats per value and block (value k of thread t at column k's [t]:
// conflict-free).  In registers the compiler had to spill it around the walks: the radiance sums, touched once or twice per bounce,
// and the surface state a bounce carries across its shadow-ray walk -- the material (7 words), the shading normal and wo -- which is
// dead weight inside the walk and was the bulk of what was parked in scratch around it (72 VGPRs at 7 blocks per CU; 172-268 bytes of
// scratch per lane, 310 scratch instructions per bounce and wave, every one of them a trip to L2: a CU's 28 waves keep 360 KB of
// scratch behind a 32 KB L1).  With the columns below the kernel keeps 88-140 B of scratch per lane; with the sums and ReSTIR-GI's
// recorded points in LDS and the surface state in registers it was 156-260 B.  The kernel uses no other LDS: 19.5 / 22.5 / 22.5 KB
// per block (pathTraceIndirect / pathTrace / ReSTIR-GI), 136 / 158 / 158 of the CU's 160 KB at 7 blocks per CU.
// (The forms this one was measured against -- the state in registers, the recorded points in 12 more columns -- can be read in this
// commit's parent and in profiles/r05_gi_counters_cold_state_in_lds.txt.)
constexpr int kPathLanes = 256;
struct Cold3 {                                                          // a three-vector in three consecutive columns
    float* p;                                                           // the thread's element of the first
    __device__ __forceinline__ f3 get() const { return mk3(p[0], p[kPathLanes], p[2 * kPathLanes]); }
    __device__ __forceinline__ void set(f3 v) const { p[0] = v.x; p[kPathLanes] = v.y; p[2 * kPathLanes] = v.z; }
    __device__ __forceinline__ void add(f3 v) const { set(get() + v); }
};
struct ColdSurf {                                                       // the surface state of a bounce
    static constexpr int kNormal = 7, kWo = kNormal + 3, kCols = kWo + 3;    // columns: the material's 7 words from 0, the shading normal, wo
    float* p;                                                           // the thread's element of the first
    __device__ __forceinline__ float& at(int k) const { return p[k * kPathLanes]; }
    __device__ __forceinline__ SurfMat mat() const { SurfMat m; m.type = __float_as_int(at(0)); m.baseColor = mk3(at(1), at(2), at(3)); m.metallic = at(4); m.roughness = at(5); m.ior = at(6); return m; }
    __device__ __forceinline__ int type() const { return __float_as_int(at(0)); }
    __device__ __forceinline__ void set_mat(const SurfMat& m) const { at(0) = __int_as_float(m.type); at(1) = m.baseColor.x; at(2) = m.baseColor.y; at(3) = m.baseColor.z; at(4) = m.metallic; at(5) = m.roughness; at(6) = m.ior; }
    __device__ __forceinline__ f3 norm() const { return Cold3{ &at(kNormal) }.get(); }
    __device__ __forceinline__ void set_norm(f3 n) const { Cold3{ &at(kNormal) }.set(n); }
    __device__ __forceinline__ f3 wo() const { return Cold3{ &at(kWo) }.get(); }
    __device__ __forceinline__ void set_wo(f3 w) const { Cold3{ &at(kWo) }.set(w); }
};
template <int MODE>
struct ColdCols {                                                       // first column of each value, in the order of the array
    static constexpr int kIndirect = 0;                                  // the indirect sum (ReSTIR-GI: the sample's Lo)
    static constexpr int kDirect = kIndirect + 3;                        // the direct sum: pathTrace only
    static constexpr int kThroughput = kDirect + (MODE == kModePT ? 3 : 0);
    static constexpr int kSurface = kThroughput + 3;                     // the 13 surface columns: material 7, normal 3, wo 3 (ColdSurf)
    static constexpr int kPrimWo = kSurface + ColdSurf::kCols;            // wo at the primary hit: ReSTIR-GI only
    static constexpr int kTotal = kPrimWo + (MODE == kModeReSTIR ? 3 : 0);
};
static_assert(ColdCols<kModePTIndirect>::kTotal == 19 && ColdCols<kModePT>::kTotal == 22 && ColdCols<kModeReSTIR>::kTotal == 22, "LDS columns per mode");

// ReSTIR-GI's four recorded points (xv, nv at the first hit, xs, ns at the second: restir.cu:316-321,345-360) are written once per path and read
// once after it: they wait in the pixel's slot of the OUTPUT reservoir array (which the kernel overwrites at its end anyway, and which is not
// the array the temporal neighbour is read from), so that the 12 LDS columns they would take hold the surface state instead.
struct Glob3 {
    float* p;
    __device__ __forceinline__ f3 get() const { return ld3(p); }
    __device__ __forceinline__ void set(f3 v) const { st3(p, v); }
};
// what a path of every mode carries; the direct sum exists in pathTrace alone (every use is under `if constexpr`)
struct NoSum {};
template <int MODE>
struct PathState {
    std::conditional_t<MODE == kModePT, Cold3, NoSum> direct;
    Cold3 indirect;               // (ReSTIR-GI: the sample's Lo)
    Cold3 throughput;
    ColdSurf surf;
    int walks;
};
// ReSTIR-GI's record of the primary bounce (restir.cu:273-281,316-321)
struct GiRecord {
    float primSamplePdf; bool primSampleDelta;
    SurfMat primMaterial;         // (textured scenes only; a plain material is read again from its id: seven registers across the whole path loop, or one)
    int primMatId;
    Cold3 primWo;                 // (live from the primary hit to the end of the path)
    Glob3 xv, nv, xs, ns;
};
struct NoRecord {};
template <int MODE> using PathRecord = std::conditional_t<MODE == kModeReSTIR, GiRecord, NoRecord>;

// The loop of the three kernels from the first shaded hit on, run by the WHOLE wave: lanes whose path has ended
// (or never started: `alive` false) stay in the loop with their flag down, so that the shadow rays can use the
// wave-level shadow-tree walk (trace_occluded_wave) and the continuation rays the pair-cooperative walk
// (trace_closest_wave) instead of per-lane walks inside a divergent loop.  Per lane the sequence of
// random draws and arithmetic is that of the reference.
template <int MODE, bool TEX, typename Sampler>
__device__ inline void path_loop(const DevScene& s, Hit h, Ray ray, Sampler& rng, int maxDepth, bool alive, PathState<MODE>& st, PathRecord<MODE>& rec) {
    const ColdSurf surf = st.surf;
    st.throughput.set(splat(1.f));
    f3 pos = h.pos;
    surf.set_norm(h.norm); surf.set_wo(-ray.d);
    const bool env = TEX && s.envTex >= 0;
    for (int depth = 1; depth <= maxDepth; depth++) {
        if (!__any(alive)) break;
        const bool deltaBSDF = surf.type() == 2;
        {
            const f3 n0 = surf.norm();
            if (alive && !deltaBSDF && dot(n0, surf.wo()) < 0.f) surf.set_norm(-n0);
        }

        // next-event estimation (pathtrace.cu:203-213 / 365-376, restir.cu:291-302): sampleDirectLight = light sample,
        // occlusion test towards it, then the single-sided / pdf part
        const bool nee = alive && !deltaBSDF && (MODE == kModePT || depth > 1) && s.numLights > 0;    // pathtrace.cu:203 vs :365, restir.cu:291
        LightSample c = invalid_light_sample(pos);
        if (alive && !deltaBSDF && (MODE == kModePT || depth > 1)) {
            const f4 r = rng.uniform4();                                        // drawn even without lights (sample4D is an argument)
            if (nee) c = sample_scene_light<TEX>(s, pos, r);
        }
        // What the segment's visibility decides is whether `add` is added (pathtrace.cu:205-212).  It is not asked -- the segment is counted
        // as the reference's testOcclusion call and not walked -- where the answer cannot matter: a sample without a valid pdf (the light faces
        // away, scene.h:448-452: sampleDirectLight returns InvalidPdf either way; 42 % of the segments on the Sponza-class scene), and a
        // contribution whose three components are all +0 (the light is below the surface's horizon, sat_dot = 0, or the BSDF is zero: any_bit).
        f3 add = splat(0.f);
        const bool valid = nee && c.pdf > 0.f;
        if (valid) {
            const SurfMat material = surf.mat();
            const f3 norm = surf.norm(), wo = surf.wo();
            const float bsdfPdf = material_pdf(material, norm, wo, c.wi);
            add = ((((st.throughput.get() * material_bsdf(material, norm, wo, c.wi)) * c.Li) * sat_dot(norm, c.wi)) / c.pdf) * power_heuristic(c.pdf, bsdfPdf);
        }
        const bool matters = valid && any_bit(add);
        const bool occluded = trace_occluded_wave(s, pos, c.point, matters);
        if (nee) {
            st.walks++;
            if (matters && !occluded) {
                bool toDirect = false;
                if constexpr (MODE == kModePT) { if (depth == 1) { st.direct.add(add); toDirect = true; } }      // pathtrace.cu:205-212
                if (!toDirect) st.indirect.add(add);
            }
        }

        BsdfSample sample;
        sample.dir = splat(0.f); sample.bsdf = splat(0.f); sample.pdf = 0.f; sample.type = kBsInvalid;
        bool deltaSample = false;
        f3 norm = splat(0.f);
        if (alive) {
            const f3 r3 = mk3(rng.uniform(), rng.uniform(), rng.uniform());    // sample3D
            norm = surf.norm();
            sample = material_sample(surf.mat(), norm, surf.wo(), r3);
            if (sample.type == kBsInvalid) alive = false;
            else if (sample.pdf < 1e-8f) alive = false;
        }
        const f3 curPos = pos;
        if (alive) {
            deltaSample = (sample.type & kBsSpecular) != 0;
            if (MODE != kModeReSTIR || depth > 1) {                             // restir.cu:315-325
                st.throughput.set(st.throughput.get() * ((sample.bsdf / sample.pdf) * (deltaSample ? 1.f : abs_dot(norm, sample.dir))));
            }
            else if constexpr (MODE == kModeReSTIR) {
                rec.primSamplePdf = sample.pdf;
                rec.primSampleDelta = deltaSample;
                rec.xv.set(pos); rec.nv.set(norm);
            }
            ray.o = pos + sample.dir * 1e-5f; ray.d = sample.dir;               // makeOffsetedRay
        }
        // The last bounce only asks whether its closest hit is an emissive triangle (a surface would need another bounce to contribute,
        // and without an environment map neither does a miss): rays that cannot hit one the way the reference accepts triangles
        // (may_hit_emissive_wave, a walk of the few emissive triangles' own tree) are counted as the reference's intersect call and not walked.
        // (ReSTIRIndirect at depth 1 records the hit point whatever it is: restir.cu:345-360.)
        bool walk = alive;
        if (depth == maxDepth && !env && !(MODE == kModeReSTIR && depth == 1)) walk = may_hit_emissive_wave(s, ray, alive);
        h = trace_closest_wave(s, ray, walk);
        if (alive) {
            st.walks++;
            surf.set_wo(-ray.d);
            if (h.primId == kNullPrim) {
                if (env) {
                    const f3 radiance = env_radiance(s, ray.d) * st.throughput.get();
                    const float weight = deltaSample ? 1.f : power_heuristic(sample.pdf, environment_map_pdf(s, ray.d));
                    st.indirect.add(radiance * weight);
                }
                alive = false;
            }
            else {
                pos = h.pos; norm = h.norm;
                const SurfMat material = TEX ? textured_material(s, h, norm) : plain_material(s, h.matId);
                surf.set_mat(material); surf.set_norm(norm);
                if (material.type == 4) {
                    if (!(dot(norm, ray.d) < 0.f)) {                            // SCENE_LIGHT_SINGLE_SIDED: the back side ends the path silently
                        const f3 radiance = material.baseColor;
                        const bool unweighted = deltaSample || (MODE == kModeReSTIR && depth == 1);      // restir.cu:353
                        const float weight = unweighted ? 1.f : power_heuristic(sample.pdf,
                            (luminance(radiance) * s.sumLightPowerInv * primitive_area(s, h.primId)) * dot(curPos - pos, curPos - pos) /
                                abs_dot(norm, normalize(curPos - pos)));         // Math::pdfAreaToSolidAngle (mathUtil.h:182-185)
                        st.indirect.add((radiance * st.throughput.get()) * weight);
                        if constexpr (MODE == kModeReSTIR) { if (depth == 1) { rec.xs.set(pos); rec.ns.set(norm); } }
                    }
                    alive = false;
                }
                else if constexpr (MODE == kModeReSTIR) { if (depth == 1) { rec.xs.set(pos); rec.ns.set(norm); } }
            }
        }
    }
}

struct IndSample { f3 Lo, xv, nv, xs, ns; };                          // IndirectLiSample
struct IndResv { IndSample s; int M; float W; };                      // Reservoir<IndirectLiSample>, 68 B at the boundary
__device__ inline IndResv ind_empty() { IndResv r; r.s.Lo = r.s.xv = r.s.nv = r.s.xs = r.s.ns = splat(0.f); r.M = 0; r.W = 0.f; return r; }
__device__ inline IndResv ind_load(const rs_indirect_reservoir* p) {
    const float* f = reinterpret_cast<const float*>(p);
    IndResv r;
    r.s.Lo = ld3(f); r.s.xv = ld3(f + 3); r.s.nv = ld3(f + 6); r.s.xs = ld3(f + 9); r.s.ns = ld3(f + 12);
    r.M = __float_as_int(f[15]); r.W = f[16];
    return r;
}
__device__ inline void ind_store(rs_indirect_reservoir* p, const IndResv& r) {
    float* f = reinterpret_cast<float*>(p);
    st3(f, r.s.Lo); st3(f + 3, r.s.xv); st3(f + 6, r.s.nv); st3(f + 9, r.s.xs); st3(f + 12, r.s.ns);
    f[15] = __int_as_float(r.M); f[16] = r.W;
}
__device__ inline bool ind_invalid(float W) { return is_nan_or_inf(W) || W < 0.f; }

// WriteSample (restir.cu:372-416): the path's sample into a fresh reservoir, the temporal neighbour's reservoir merged into it, the
// result stored in the pixel's slot of resvOut; returns the pixel's indirect radiance
template <bool TEX, typename Sampler>
__device__ inline f3 write_sample(const DevScene& s, const GiRecord& rec, f3 Lo, Sampler& rng, const GBufView& g, int index,
                                  rs_indirect_reservoir* resvOut, const rs_indirect_reservoir* resvIn, int first, int reuse) {
    const IndSample smp = { Lo, rec.xv.get(), rec.nv.get(), rec.xs.get(), rec.ns.get() };
    IndResv rv = ind_empty();
    float sampleWeight = 0.f;
    if (!(luminance(smp.Lo) < 1e-8f)) {                                         // !indirectSample.invalid()
        sampleWeight = luminance(smp.Lo / rec.primSamplePdf);                   // toScalar(pHatIndirect / primSamplePdf), pHat = Lo
        if ((sampleWeight != sampleWeight) || sampleWeight < 0.f) sampleWeight = 0.f;
    }
    {
        const float u = rng.uniform();                                          // Reservoir::update
        rv.W += sampleWeight; rv.M++;
        if (u * rv.W < sampleWeight) rv.s = smp;
    }
    if (!first && (reuse & 1)) {
        // findTemporalNeighbor (restir.cu:20-45), as k_temporal (restir.hip) makes it through its non-temporal loads.  Written out here and
        // there: as a function returning the neighbour's index, in either kernel, the test came out of the compiler differently
        // (EXPERIMENTS.md), and this form keeps the path loop's instructions those of the measured kernel.
        const int primId = g.primId[index];
        const int lastIdx = g.motion[index];
        bool diff = false;
        if (lastIdx < 0) diff = true;
        else if (primId <= kNullPrim) diff = true;
        else if (g.lastPrimId[lastIdx] != primId) diff = true;
        else {
            const f3 n = ld3(g.normal + (size_t)index * 3), ln = ld3(g.lastNormal + (size_t)lastIdx * 3);
            const float depth = g.depth[index], pdepth = g.lastDepth[lastIdx];
            if (abs_dot(n, ln) < .9f || gabs(pdepth - depth) > depth * .1f) diff = true;
        }
        IndResv t = ind_empty();
        if (!diff) t = ind_load(resvIn + lastIdx);
        if (!ind_invalid(t.W)) {
            const float u = rng.uniform();                                      // Reservoir::merge (restir.h:61-68)
            rv.W += t.W; rv.M += t.M;
            if (u * rv.W < t.W) rv.s = t.s;
        }
    }
    f3 indirect = splat(0.f);
    if (rv.M > 20) { rv.W *= (float)20 / (float)rv.M; rv.M = 20; }            // clamp<20>() (restir.h:79-86)
    if (!ind_invalid(rv.W)) {
        const f3 primWi = normalize(rv.s.xs - rv.s.xv);
        indirect = ((rv.s.Lo / luminance(rv.s.Lo)) * rv.W) / (float)rv.M;
        const SurfMat primMaterial = TEX ? rec.primMaterial : (rec.primMatId >= 0 ? plain_material(s, rec.primMatId) : empty_surf_mat());
        indirect = indirect * (material_bsdf(primMaterial, rv.s.nv, rec.primWo.get(), primWi) * (rec.primSampleDelta ? 1.f : sat_dot(rv.s.nv, primWi)));
    }
    if (any_nan_or_inf(indirect)) indirect = splat(0.f);
    ind_store(resvOut + index, rv);
    return indirect;
}

// 7 blocks per CU = 7 waves per SIMD caps the kernel at 72 VGPRs (it wants 110-140; ~200 B of scratch per lane, outside the
// walk): measured on the bench scene at depth 4, pathTrace 12.98 -> 10.6 ms, pathTraceIndirect 12.20 -> 10.0 ms,
// ReSTIRIndirect 15.26 -> 10.3 ms; 5 blocks 11.5 / 10.8 / 11.0 ms, 6 blocks 11.0 / 10.3 / 10.6 ms, 8 blocks (64 VGPRs) 12.3 / 12.5 / 14.1 ms
#ifndef RS_PATH_BLOCKS
#define RS_PATH_BLOCKS 7
#endif
template <int MODE, bool TEX, bool SOBOL>
__global__ void __launch_bounds__(kPathLanes, RS_PATH_BLOCKS) k_path(DevScene s, CamParams cam, float* __restrict__ directIllum, float* __restrict__ indirectIllum,
                                              rs_indirect_reservoir* __restrict__ resvOut, const rs_indirect_reservoir* __restrict__ resvIn,
                                              GBufView g, int looper, int iter, int maxDepth, int first, int reuse, int tilesX,
                                              unsigned long long* rayCount) {
    using Cols = ColdCols<MODE>;
    static_assert(Cols::kTotal * kPathLanes * 4 * RS_PATH_BLOCKS <= 160 * 1024, "the cold-state columns of RS_PATH_BLOCKS blocks fit in a CU's LDS");
    __shared__ float sCold[Cols::kTotal * kPathLanes];
    const auto column = [&](int k) { return sCold + k * kPathLanes + threadIdx.x; };
    int x, y;
    const int lane = pixel_of_lane(tilesX, 0, x, y);
    const bool inside = x < cam.width && y < cam.height;
    const int index = y * cam.width + x;
    using Sampler = typename PathSamplerOf<SOBOL>::type;                // the default engine on x: no register for an addend here (rs_math.h RngOnX)
    Sampler rng = Sampler::seeded(s.sampleSeq, looper, index, 0);     // pathtrace.cu:170,339, restir.cu:256
    const f4 r = rng.uniform4();
    const Ray ray = camera_sample(cam, x, y, r.x, r.y);
    const Hit h = trace_closest_packet(s, ray, inside);                // all 64 lanes take part in the wave's walk
    PathState<MODE> st;
    st.indirect.p = column(Cols::kIndirect); st.indirect.set(splat(0.f));
    if constexpr (MODE == kModePT) { st.direct.p = column(Cols::kDirect); st.direct.set(splat(0.f)); }
    st.throughput.p = column(Cols::kThroughput);
    st.surf.p = column(Cols::kSurface);
    st.walks = 0;
    PathRecord<MODE> rec;
    if constexpr (MODE == kModeReSTIR) {
        rec.primSamplePdf = 0.f; rec.primSampleDelta = false;
        rec.primMaterial = empty_surf_mat(); rec.primMatId = -1;
        rec.primWo.p = column(Cols::kPrimWo); rec.primWo.set(-ray.d);
        float* slot = reinterpret_cast<float*>(resvOut + (inside ? index : 0));      // (lanes outside the frame never touch it)
        rec.xv.p = slot + 3; rec.nv.p = slot + 6; rec.xs.p = slot + 9; rec.ns.p = slot + 12;
        if (inside) { rec.xv.set(splat(0.f)); rec.nv.set(splat(0.f)); rec.xs.set(splat(0.f)); rec.ns.set(splat(0.f)); }
    }
    // primary hit (pathtrace.cu:172-190 / 343-350, restir.cu:259-270); lanes that end here keep alive = false
    bool alive = false;
    Hit hh = h;
    SurfMat material = empty_surf_mat();
    if (inside) {
        st.walks = 1;
        if (h.primId == kNullPrim) {
            if constexpr (MODE == kModePT) st.direct.set(splat(1.f));                  // pathtrace.cu:175-178
        }
        else {
            f3 norm = h.norm;
            material = TEX ? textured_material(s, h, norm) : plain_material(s, h.matId);
            if (MODE == kModePT) material.baseColor = splat(1.f);                      // DENOISER_DEMODULATE (:181-185)
            if (material.type == 4) {
                if constexpr (MODE == kModePT) st.direct.set(splat(1.f));              // :187-190
            }
            else {
                hh.norm = norm;
                if constexpr (MODE == kModeReSTIR) { if (TEX) rec.primMaterial = material; else rec.primMatId = h.matId; }
                alive = true;
            }
        }
    }
    st.surf.set_mat(material);
    path_loop<MODE, TEX, Sampler>(s, hh, ray, rng, maxDepth, alive, st, rec);                 // every lane of the wave takes part
    if (inside) {
        f3 indirect = st.indirect.get();
        if constexpr (MODE == kModePT) {
            f3 direct = st.direct.get();
            if (any_nan_or_inf(direct)) direct = splat(0.f);
            if (any_nan_or_inf(indirect)) indirect = splat(0.f);
            accumulate(directIllum, index, hdr_to_ldr(direct), iter);                   // Math::HDRToLDR (:273-276)
            accumulate(indirectIllum, index, hdr_to_ldr(indirect), iter);
        }
        else if constexpr (MODE == kModePTIndirect) {
            if (any_nan_or_inf(indirect)) indirect = splat(0.f);
            accumulate(indirectIllum, index, indirect, iter);
        }
        else accumulate(indirectIllum, index, write_sample<TEX>(s, rec, indirect, rng, g, index, resvOut, resvIn, first, reuse), iter);
    }
    count_walks(rayCount + (blockIdx.x % kWalkSub) * kWalkStride, st.walks, lane);
}

template <int MODE>
int launch_path(const rs_scene* scene, const rs_camera* cam, float* direct, float* indirect, rs_indirect_reservoir* out,
                const rs_indirect_reservoir* in, const GBufView& g, int looper, int iter, int maxDepth, int first, int reuse) {
    const int W = cam->resolution[0], H = cam->resolution[1];
    const int tilesX = (W + 31) / 32, tilesY = (H + 7) / 8;
    const CamParams cp = rs_make_cam_params(cam);
    // The Sobol branch reads data[ptr++] without a bound (sampler.h:20); a path draws at most 4 + 7 per bounce + 2 numbers, and the
    // device table ends in a guard of kSobolGuard zeros: refuse what could read beyond it.
    const bool sobol = scene->dev.sampleSeq != nullptr;
    if (sobol) {
        RS_TRY(rs_check_looper(scene, looper, "pathTrace / ReSTIRIndirect"));
        if (6 + 7LL * maxDepth > kSobolSampleDim + kSobolGuard) return rs_fail(RS_ERR_INVALID_ARGUMENT, "pathTrace / ReSTIRIndirect: trace depth too large for the Sobol table's guard");
    }
    unsigned long long* walkCount = nullptr;
    RS_TRY(rs_walk_counters(&walkCount));
    const dim3 grid(tilesX * tilesY), block(kPathLanes);
    rs_dispatch([&](auto TEX, auto SOBOL) {
        hipLaunchKernelGGL((k_path<MODE, TEX(), SOBOL()>), grid, block, 0, rs_stream(), scene->dev, cp, direct, indirect, out, in, g, looper, iter, maxDepth, first, reuse, tilesX, walkCount);
    }, scene->textured, sobol);
    return 0;
}

}  // namespace

extern "C" {

int rs_path_trace(const rs_scene* scene, const rs_camera* cam, float* devDirectIllum, float* devIndirectIllum,
                  int iter, int looper, int maxDepth, unsigned long long* rays) {
    RS_SCOPE(scene);
    if (!scene || !cam || !devDirectIllum || !devIndirectIllum) return rs_fail(RS_ERR_INVALID_ARGUMENT, "pathTrace: null argument");
    RS_TRY(rs_denoise_order(devDirectIllum)); RS_TRY(rs_denoise_order(devIndirectIllum));      // images a filter on the denoise stream may still be reading
    GBufView none{};
    RS_TRY(launch_path<kModePT>(scene, cam, devDirectIllum, devIndirectIllum, nullptr, nullptr, none, looper, iter, maxDepth, 0, 0));
    RS_TRY(rs_after_launch("pathTrace"));
    return rs_walk_counters_sum(rays);
}

int rs_path_trace_indirect(const rs_scene* scene, const rs_camera* cam, float* devIndirectIllum, int iter, int looper, int maxDepth,
                           unsigned long long* rays) {
    RS_SCOPE(scene);
    if (!scene || !cam || !devIndirectIllum) return rs_fail(RS_ERR_INVALID_ARGUMENT, "pathTraceIndirect: null argument");
    RS_TRY(rs_denoise_order(devIndirectIllum));
    GBufView none{};
    RS_TRY(launch_path<kModePTIndirect>(scene, cam, nullptr, devIndirectIllum, nullptr, nullptr, none, looper, iter, maxDepth, 0, 0));
    RS_TRY(rs_after_launch("pathTrace"));
    return rs_walk_counters_sum(rays);
}

int rs_restir_indirect(rs_restir* r, const rs_scene* scene, const rs_camera* cam, const rs_gbuffer* g, float* devIndirectIllum,
                       int iter, int looper, int reuse, int maxDepth, unsigned long long* rays) {
    RS_SCOPE(r);
    RS_TRY(rs_gbuffer_join(g));                         // the render may still be on the auxiliary stream
    if (!r || !scene || !cam || !g || !devIndirectIllum) return rs_fail(RS_ERR_INVALID_ARGUMENT, "ReSTIRIndirect: null argument");
    if (cam->resolution[0] != r->width || cam->resolution[1] != r->height || g->width != r->width || g->height != r->height)
        return rs_fail(RS_ERR_INVALID_ARGUMENT, "ReSTIRIndirect: size mismatch");
    const size_t n = (size_t)r->width * r->height;
    bool history = true;                                        // the buffers hold what an earlier call left
    for (int i = 0; i < 2; i++)
        if (!r->indResv[i]) {                                   // devIndTemporalReservoir / devIndLastTemporalReservoir (restir.cu:13-14,491-494)
            RS_TRY(rs_dev_alloc(&r->indResv[i], n));
            RS_HIP(hipMemsetAsync(r->indResv[i], 0, n * sizeof(rs_indirect_reservoir), rs_stream()));
            history = false;
        }
    RS_TRY(rs_denoise_order(devIndirectIllum));
    // rs_restir_set_indirect_revalidation: geometry moved since the previous call -- the stale slots of the history leave before the merge
    RS_TRY(rs_indirect_revalidate_before_path(r, scene, history && !r->firstFrame && (reuse & 1), r->indResv[1], n));
    // rs_restir_set_indirect_spatial: the caller's image receives the spatial result only, so the path kernel of a call that runs the pass
    // leaves its own radiance in a scratch image (iter 0: the value itself) and the pass accumulates with the call's iter
    const bool spatial = rs_indirect_spatial_runs(r, reuse);
    RS_TRY(launch_path<kModeReSTIR>(scene, cam, nullptr, spatial ? r->indSpatial.temporalImage : devIndirectIllum, r->indResv[0], r->indResv[1], gbuf_view(g),
                                    looper, spatial ? 0 : iter, maxDepth, r->firstFrame ? 1 : 0, reuse));
    if (spatial) RS_TRY(rs_indirect_spatial_after_path(r, scene, cam, gbuf_view(g), r->indResv[0], devIndirectIllum, iter, looper));
    { rs_indirect_reservoir* t = r->indResv[0]; r->indResv[0] = r->indResv[1]; r->indResv[1] = t; }      // std::swap (:463)
    r->firstFrame = false;                                                                                    // ReSTIRFirstFrame (:465-467)
    rs_indirect_revalidate_note(r, scene);
    RS_TRY(rs_after_launch("ReSTIR Indirect"));
    RS_TRY(rs_walk_counters_sum(rays));
    RS_TRY(rs_indirect_revalidate_add_rays(r, rays));
    return rs_indirect_spatial_add_rays(r, rays);
}

int rs_restir_download_indirect(rs_restir* r, int which, rs_indirect_reservoir* host) {
    RS_SCOPE(r);
    if (!r || !host || which < 0 || which > 1 || !r->indResv[which]) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_restir_download_indirect: bad argument");
    RS_HIP(hipStreamSynchronize(rs_stream()));
    RS_HIP(hipMemcpy(host, r->indResv[which], (size_t)r->width * r->height * sizeof(rs_indirect_reservoir), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
