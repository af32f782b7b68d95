// light_history.hip -- light tracking and retargeting of a rs_restir (rs_light_history, rs_internal.h): the planes' lifetime, the one place
// that makes ids and records unknown, what a phase-A call and the end of a frame do to the state, k_retarget, and every entry point of
// include/restir_hip.h that is only about this state.  restir.hip hands the kernel arguments it gets here to its RIS kernels and k_temporal.
#include "rs_light_history.h"

using namespace rs;

namespace {

// Retargeting: the temporal candidates whose lamp has moved since the previous frame, evaluated again on this frame's light records
// before the merge.  One lane per pixel, tiles and walk as k_shadow.  For a shaded pixel whose history slot j = motion[i] passes
// findTemporalNeighbor and holds a sample of a light with moved[light] > seenMoves (not the environment's entry, not W = 0):
//   1  (Li', wi', dist', pdf') of the light at the sample's (u, v) seen from the pixel's position; a sample that now faces away, or a pdf'
//      that is not finite and positive: W = 0
//   2  pOld, pNew: luminance(Li * bsdf(wi) * sat_dot(n, wi)) of the old and the new sample on the pixel's surface (ris_candidate's g)
//   3  W = (W * (pNew / pOld)) * (pdfOld / pdf') when pOld and pdfOld are positive and finite, else 0
//   5  a sample left with W != 0 walks its shadow segment, pos -> pos + wi' * dist', and is cleared when occluded
// The candidate goes to planes of this kernel's own; the history buffers are not written (with a moving camera two pixels read one slot).
// Registers: everything but W and the index is stored before the walk, which then carries what k_shadow's carries.
__global__ void __launch_bounds__(256, RS_WALK_WAVES) k_retarget(DevScene s, SurfPlanes sp, GBufView g, ResvPlanes last, const float4* recLast, const uint32_t* moved,
                                                                 uint32_t seenMoves, int envId, RetargetOut out, int width, int y0, int y1, int tilesX,
                                                                 unsigned long long* rayCount, unsigned long long* stats) {
    RS_SETPRIO(RS_PRIO_WALK);
    int x, y;
    const int lane = pixel_of_lane(tilesX, y0, x, y);
    const bool inside = x < width && y < y1;
    const int index = inside ? y * width + x : 0;
    const float4 pm = inside ? sp.posMat[index] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int mk = __float_as_int(pm.w);
    const bool shaded = inside && mk_kind(mk) == kKindShaded;
    const f3 pos = mk3(pm.x, pm.y, pm.z);
    bool take = false;
    int lastIdx = 0;
    if (shaded) {                                               // findTemporalNeighbor, as k_temporal
        const int primId = g.primId[index];
        lastIdx = g.motion[index];
        bool diff = false;
        if (lastIdx < 0) diff = true;
        else if (primId <= kNullPrim) diff = true;
        else if (g.lastPrimId[lastIdx] != primId) diff = true;
        else {
            const f3 n = ld3(g.normal + (size_t)index * 3), ln = ld3(g.lastNormal + (size_t)lastIdx * 3);
            const float depth = g.depth[index], pdepth = g.lastDepth[lastIdx];
            if (abs_dot(n, ln) < .9f || gabs(pdepth - depth) > depth * .1f) diff = true;
        }
        take = !diff;
    }
    float W = 0.f;
    f3 wi = splat(0.f);
    float dist = 0.f;
    if (take) {
        const float4 rc = recLast[lastIdx];
        const int id = __float_as_int(rc.x);
        W = last.w[lastIdx];
        take = id >= 0 && id < s.numLights && id != envId && W != 0.f;
        if (take) take = moved[id] > seenMoves;
        if (take) {
            const float4 a = last.li[lastIdx], b = last.wi[lastIdx], nr = sp.norm[index];
            const f3 oldLi = mk3(a.x, a.y, a.z), oldWi = mk3(b.x, b.y, b.z), norm = mk3(nr.x, nr.y, nr.z);
            const int type = mk_type(mk);
            f3 wo = splat(0.f);
            float roughness = 0.f;
            if (type == 1) { const float4 w4 = sp.wo[index]; wo = mk3(w4.x, w4.y, w4.z); roughness = w4.w; }
            f3 Li;
            float pdf;
            light_sample_at(s.lights, id, rc.y, rc.z, pos, Li, wi, dist, pdf);
            if (!(pdf > 0.f) || is_nan_or_inf(pdf)) W = 0.f;                                  // step 1
            else {
                const f3 one = splat(1.f);
                const float pOld = luminance(oldLi * eval_bsdf(type, one, nr.w, roughness, norm, wo, oldWi) * sat_dot(norm, oldWi));
                const float pNew = luminance(Li * eval_bsdf(type, one, nr.w, roughness, norm, wo, wi) * sat_dot(norm, wi));
                const float pdfOld = rc.w;
                if (pOld > 0.f && pdfOld > 0.f && !is_nan_or_inf(pOld) && !is_nan_or_inf(pdfOld)) W = (W * (pNew / pOld)) * (pdfOld / pdf);
                else W = 0.f;                                                                 // step 3
            }
            out.li[index] = make_float4(Li.x, Li.y, Li.z, dist);
            out.wi[index] = make_float4(wi.x, wi.y, wi.z, W);
            out.rec[index] = make_float4(rc.x, rc.y, rc.z, pdf);
        }
    }
    if (inside) out.flag[index] = take ? 1 : 0;
    const bool walk = take && W != 0.f;
    const bool occluded = trace_occluded_wave(s, pos, pos + wi * dist, walk);                 // every lane of the wave takes part
    if (walk && occluded) { reinterpret_cast<float*>(out.wi + index)[3] = 0.f; W = 0.f; }    // step 5
    const unsigned long long bTake = __ballot(take), bWalk = __ballot(walk), bZero = __ballot(take && W == 0.f);
    if (lane == 0 && bTake) {
        atomicAdd(stats, (unsigned long long)__popcll(bTake));
        atomicAdd(stats + 2, (unsigned long long)__popcll(bZero));
        if (bWalk) {
            atomicAdd(stats + 1, (unsigned long long)__popcll(bWalk));
            atomicAdd(rayCount + (blockIdx.x % kRaySub) * kRayStride, (unsigned long long)__popcll(bWalk));
        }
    }
}

constexpr unsigned kAll = 7u, kLastAndPublished = 6u;         // rs_light_history_forget's `which`
}  // namespace

// "Unknown" is every byte 0xff: id -1, and a record whose light is -1.
int rs_light_history_forget(rs_light_history& h, size_t n, unsigned which, bool blocking, int planes) {
    if (planes < 0) planes = h.mode == RS_LIGHTS_RECORDS ? 3 : h.mode;
    auto clear = [&](void* p, size_t bytes) { return rs_check_hip(blocking ? hipMemset(p, 0xff, bytes) : hipMemsetAsync(p, 0xff, bytes, rs_stream()), "hipMemset"); };
    for (int k = 0; k < 3; k++) if ((planes & 1) && (which >> k & 1)) RS_TRY(clear(h.id[k], n * sizeof(int)));
    for (int k = 0; k < 3; k++) if ((planes & 2) && (which >> k & 1)) RS_TRY(clear(h.rec[k], n * sizeof(float4)));
    return 0;
}

void rs_light_history_free(rs_light_history& h) {
    for (int*& p : h.id) rs_dev_free(p);
    for (int*& p : h.candId) rs_dev_free(p);
    for (float4*& p : h.rec) rs_dev_free(p);
    for (float4*& p : h.candRec) rs_dev_free(p);
    rs_dev_free(h.rtLi); rs_dev_free(h.rtWi); rs_dev_free(h.rtRec); rs_dev_free(h.rtFlag); rs_dev_free(h.dRetarget);
}

int rs_light_history_phase_a(rs_light_history& h, const rs_scene* scene, int set, bool merges, const SurfPlanes& sp, const GBufView& g, const ResvPlanes& last,
                             int y0, int y1, int tilesX, int tilesY, unsigned long long* rayCounter, LightIds* ids, LightRecs* recs) {
    *ids = LightIds{ nullptr, nullptr, nullptr, nullptr, nullptr, 0, -1 };
    *recs = LightRecs{};
    if (h.mode == RS_LIGHTS_OFF) return 0;
    // the light indices of another scene's reservoirs name other lights: unknown from here on
    if (h.sceneId != scene->id) {
        RS_TRY(rs_light_history_forget(h, (size_t)g.width * g.height, kLastAndPublished, false));
        h.sceneId = scene->id;
        h.seenMoves = scene->lightMoves;                        // (no record names a light of this scene yet)
    }
    *ids = LightIds{ h.candId[set], h.id[1], h.id[0], h.id[2], scene->dev.lights, scene->numLights, scene->envMapTexId >= 0 ? scene->numLights - 1 : -1 };
    if (h.mode != RS_LIGHTS_RECORDS) return 0;
    // Lamps moved since the previous frame: their samples are evaluated again before the merge, on the library stream behind the
    // chain's join.  A frame after which none moved launches nothing extra (the merge's record form carries the records).
    h.frameMoves = scene->lightMoves;
    const bool moved = merges && scene->lightMoves != h.seenMoves;
    *recs = LightRecs{ h.candRec[set], h.rec[1], h.rec[0], h.rec[2], h.rtLi, h.rtWi, h.rtRec, moved ? h.rtFlag : nullptr };
    if (!moved) return 0;
    if (!h.rtLaunched) {
        RS_HIP(hipMemsetAsync(h.dRetarget, 0, 3 * sizeof(unsigned long long), rs_stream()));
        h.rtLaunched = true;
    }
    hipLaunchKernelGGL(k_retarget, dim3(tilesX * tilesY), dim3(256), 0, rs_stream(), scene->dev, sp, g, last, h.rec[1],
                       scene->ver[scene->verCur].moved, (uint32_t)h.seenMoves, ids->envId, RetargetOut{ h.rtLi, h.rtWi, h.rtRec, h.rtFlag },
                       g.width, y0, y1, tilesX, rayCounter, h.dRetarget);
    return 0;
}

void rs_light_history_end_frame(rs_light_history& h, int phaseACalls) {
    int* ti = h.id[0]; h.id[0] = h.id[1]; h.id[1] = ti;         // the reservoirs' light indices travel with them
    float4* tr = h.rec[0]; h.rec[0] = h.rec[1]; h.rec[1] = tr;  // ... and so do their records
    if (h.mode == RS_LIGHTS_RECORDS && phaseACalls > 0) h.seenMoves = h.frameMoves;
    h.rtLaunchedLast = h.rtLaunched; h.rtLaunched = false;
}

extern "C" {

// Light tracking (include/restir_hip.h): the id planes are allocated on the first switch-on; the reservoirs published while tracking was
// off carry no light index, so every switch-on starts from "unknown" (-1) -- ordered on the library stream like the frames around it.
// Switching it off switches retargeting off: the records ride on the ids.
int rs_restir_set_light_tracking(rs_restir* r, int enable) {
    RS_SCOPE(r);
    if (!r) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_restir_set_light_tracking: null");
    rs_light_history& h = r->lights;
    const bool on = enable != 0;
    if (on == (h.mode >= RS_LIGHTS_IDS)) return 0;
    if (on) {
        const size_t n = (size_t)r->width * r->height;
        if (!h.id[0]) {
            for (int*& p : h.id) RS_TRY(rs_dev_alloc(&p, n));
            for (int*& p : h.candId) RS_TRY(rs_dev_alloc(&p, n));
        }
        RS_TRY(rs_light_history_forget(h, n, kAll, false, 1));
        h.sceneId = 0;                   // (the RIS winners' planes need no clearing: a frame writes its set before it reads it)
    }
    h.mode = on ? RS_LIGHTS_IDS : RS_LIGHTS_OFF;
    return rs_after_launch("rs_restir_set_light_tracking");
}

// Light retargeting (include/restir_hip.h), on top of tracking.  The planes are allocated before anything of the object changes, and
// the mode is set last: a failed allocation leaves it as it was with nothing changed, and so does a failure of the tracking switch (which
// leaves tracking as that call leaves it).  A clear that fails to enqueue leaves retargeting off as well.  Every record AND every tracked
// id starts unknown, in the order of the library stream -- ids that tracking carried so far have no record to go with -- and the next frame
// takes the scene's count of moves as seen (sceneId = 0): nothing that happened before the switch is evaluated again.
int rs_restir_set_light_retargeting(rs_restir* r, int enable) {
    RS_SCOPE(r);
    if (!r) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_restir_set_light_retargeting: null");
    rs_light_history& h = r->lights;
    const bool on = enable != 0;
    if (on == (h.mode == RS_LIGHTS_RECORDS)) return 0;
    if (!on) { h.mode = RS_LIGHTS_IDS; return 0; }
    const size_t n = (size_t)r->width * r->height;
    constexpr int kPlanes = 3 + RS_SURF_SETS + 3;
    float4* f[kPlanes] = {};
    int* flag = nullptr;
    unsigned long long* counters = nullptr;
    const bool fresh = !h.rec[0];
    auto drop = [&]() { for (float4*& p : f) rs_dev_free(p); rs_dev_free(flag); rs_dev_free(counters); };
    if (fresh) {
        int e = 0;
        for (float4*& p : f) if (!e) e = rs_dev_alloc(&p, n);
        if (!e) e = rs_dev_alloc(&flag, n);
        if (!e) e = rs_dev_alloc(&counters, 3);
        if (!e) e = rs_check_hip(hipMemset(counters, 0, 3 * sizeof(unsigned long long)), "memset");
        if (e) { drop(); return e; }
    }
    const bool tracked = h.mode >= RS_LIGHTS_IDS;
    if (!tracked) if (int e = rs_restir_set_light_tracking(r, 1)) { drop(); return e; }
    if (fresh) {
        for (int k = 0; k < 3; k++) h.rec[k] = f[k];
        for (int k = 0; k < RS_SURF_SETS; k++) h.candRec[k] = f[3 + k];
        h.rtLi = f[3 + RS_SURF_SETS]; h.rtWi = f[4 + RS_SURF_SETS]; h.rtRec = f[5 + RS_SURF_SETS];
        h.rtFlag = flag; h.dRetarget = counters;
    }
    RS_TRY(rs_light_history_forget(h, n, kAll, false, tracked ? 3 : 2));     // (the ids: a switch-on of tracking has just cleared them)
    h.sceneId = 0;
    h.mode = RS_LIGHTS_RECORDS;
    h.rtLaunched = h.rtLaunchedLast = false;
    return rs_after_launch("rs_restir_set_light_retargeting");
}

int rs_restir_get_light_retargeting(const rs_restir* r, int* enabled) {
    if (!r || !enabled) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_restir_get_light_retargeting: null argument");
    *enabled = r->lights.mode == RS_LIGHTS_RECORDS ? 1 : 0;
    return 0;
}

int rs_restir_download_light_ids(const rs_restir* r, int which, int* host) {
    RS_SCOPE(r);
    if (!r || !host || which < 0 || which > 2) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_restir_download_light_ids: bad argument");
    const size_t n = (size_t)r->width * r->height;
    if (r->lights.mode < RS_LIGHTS_IDS || !r->lights.id[0]) { for (size_t i = 0; i < n; i++) host[i] = -1; return 0; }
    RS_HIP(hipStreamSynchronize(rs_stream()));
    RS_HIP(hipMemcpy(host, r->lights.id[which], n * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

int rs_restir_download_light_samples(const rs_restir* r, int which, rs_light_sample* host) {
    RS_SCOPE(r);
    if (!r || !host || which < 0 || which > 2) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_restir_download_light_samples: bad argument");
    const size_t n = (size_t)r->width * r->height;
    static_assert(sizeof(rs_light_sample) == sizeof(float4), "a record is one 16-byte element of the planes");
    if (r->lights.mode != RS_LIGHTS_RECORDS || !r->lights.rec[0]) { for (size_t i = 0; i < n; i++) host[i] = rs_light_sample{ -1, 0.f, 0.f, 0.f }; return 0; }
    RS_HIP(hipStreamSynchronize(rs_stream()));
    RS_HIP(hipMemcpy(host, r->lights.rec[which], n * sizeof(float4), hipMemcpyDeviceToHost));
    return 0;
}

// test hook: what k_retarget did in the frame that rs_restir_end_frame ended last -- { samples re-evaluated, shadow segments walked,
// samples left with W = 0 }; zeros when that frame did not launch it
int rs_debug_restir_retarget(rs_restir* r, unsigned long long out[3]) {
    RS_SCOPE(r);
    if (!r || !out) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_restir_retarget: null argument");
    out[0] = out[1] = out[2] = 0;
    if (r->lights.mode != RS_LIGHTS_RECORDS || !r->lights.rtLaunchedLast) return 0;
    RS_HIP(hipStreamSynchronize(rs_stream()));
    RS_HIP(hipMemcpy(out, r->lights.dRetarget, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}

// ... and whether that frame launched it at all (a launch that found nothing to evaluate reports zeros too)
int rs_debug_restir_retarget_launched(rs_restir* r, int* launched) {
    if (!r || !launched) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_restir_retarget_launched: null argument");
    *launched = r->lights.mode == RS_LIGHTS_RECORDS && r->lights.rtLaunchedLast ? 1 : 0;
    return 0;
}

}  // extern "C"
