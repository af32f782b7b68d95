// shadow_revalidate.hip -- shadow revalidation of a rs_restir (rs_shadow_revalidation, rs_internal.h): after an accepted geometry edit the
// temporal candidates whose shadow segment crosses the edit's box are walked again on the current geometry before the merge, and the
// merge takes an occluded one as if its slot held W = 0.  The switch, what a phase-A call and the end of a frame do to the state,
// k_revalidate and the entry points of include/restir_hip.h that are only about this.  The host decisions are rs_revalidate_plan.h's.
#include "rs_light_history.h"
#include "rs_shadow_regroup.h"
#include "rs_revalidate.h"

using namespace rs;

namespace {

// { examined, walked, occluded }: each counter is kRaySub partial ones, 64 B apart, as the frames' ray counters are -- nearly every wave of
// a frame adds to `examined`, and one hot address serialises them
constexpr int kStatWords = 3 * kRaySub * kRayStride;
__device__ __forceinline__ unsigned long long* stat_of(unsigned long long* stats, int k) { return stats + ((size_t)k * kRaySub + blockIdx.x % kRaySub) * kRayStride; }

// One lane per pixel, tiles as k_shadow.  The candidate of a shaded pixel whose history slot j = motion[i] passes findTemporalNeighbor is
// examined when the slot's W != 0 and k_retarget did not take it in this call (rtFlag; null: not launched); an examined segment
// a = pos, b = pos + wi * dist (wi, dist of slot j; the pixel's own position) is a walker when rs_segment_in_boxes says so.  Walkers are
// few -- the segments through a moved box -- so the block compacts them through LDS into dense slots before any ray walks: REGROUP as
// k_shadow_regroup does, counted in length bins and handed out longest bin first (rs_shadow_regroup.h; arrival order within a bin),
// otherwise in pixel order (a ballot per wave, the waves' counts through LDS).  Lane t then walks the segment of slot t; a wave whose
// slots are all empty leaves before it touches the tree, so a block without a walker reads no node at all.  An occluded walker writes the
// call's epoch to its pixel's word of the flag plane (rs_shadow_revalidation::flag): nothing else writes the plane, and nothing clears it.
// Any-hit occlusion does not depend on the lane that carries a segment, so both forms mark the same pixels.
// LDS: 2 x 256 float4 + the histogram = 8 448 B, eight blocks per CU.  stats: { examined, walked, occluded } (stat_of), one atomic per wave each.
template <bool REGROUP>
__global__ void __launch_bounds__(kShadowRegroupRays, RS_WALK_WAVES) k_revalidate(DevScene s, const float4* posMat, GBufView g, ResvPlanes last, const int* rtFlag, rs_revalidate_boxes boxes,
                                                                                  unsigned* flag, unsigned epoch, int width, int y0, int y1, int tilesX, float binsOverExtent,
                                                                                  unsigned long long* rayCount, unsigned long long* stats) {
    __shared__ float4 sRay[2 * kShadowRegroupRays];
    __shared__ int sHist[kShadowBins];
    RS_SETPRIO(RS_PRIO_WALK);
    int x, y;
    const int lane = pixel_of_lane(tilesX, y0, x, y);
    if (threadIdx.x < kShadowBins) sHist[threadIdx.x] = 0;
    const bool inside = x < width && y < y1;
    const int index = inside ? y * width + x : 0;
    const float4 pm = inside ? posMat[index] : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool shaded = inside && mk_kind(__float_as_int(pm.w)) == kKindShaded;
    bool examine = false;
    int lastIdx = 0;
    if (shaded) {                                               // findTemporalNeighbor, as k_temporal and k_retarget
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
        examine = !diff;
    }
    if (examine) examine = last.w[lastIdx] != 0.f;
    if (examine && rtFlag) examine = rtFlag[index] == 0;       // k_retarget has just walked that one on this geometry
    const f3 pos = mk3(pm.x, pm.y, pm.z);
    f3 end = pos;
    float dist = 0.f;
    bool walk = false;
    if (examine) {
        const float4 a = last.li[lastIdx], b = last.wi[lastIdx];
        dist = a.w;
        end = pos + mk3(b.x, b.y, b.z) * dist;                  // as k_retarget evaluates it
        walk = rs_segment_in_boxes(pos.x, pos.y, pos.z, end.x, end.y, end.z, boxes);
    }
    const unsigned long long bExamine = __ballot(examine), bWalk = __ballot(walk);
    if (lane == 0 && bExamine) {
        atomicAdd(stat_of(stats, 0), (unsigned long long)__popcll(bExamine));
        if (bWalk) {
            atomicAdd(stat_of(stats, 1), (unsigned long long)__popcll(bWalk));
            atomicAdd(rayCount + (blockIdx.x % kRaySub) * kRayStride, (unsigned long long)__popcll(bWalk));
        }
    }
    // the walkers' slots
    int slot, count;
    if (REGROUP) {
        const int bin = shadow_bin(dist, binsOverExtent);
        __syncthreads();
        int rank = 0;
        if (walk) rank = atomicAdd(&sHist[bin], 1);
        __syncthreads();
        int above = sHist[kShadowBins - 1 - lane];              // lane l holds bin 63 - l: the inclusive scan is the walkers in that bin and above
        for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(above, off); above += lane >= off ? v : 0; }
        count = __shfl(above, 63);
        const int first = __shfl(above, bin < kShadowBins - 1 ? kShadowBins - 2 - bin : 0);
        slot = (bin < kShadowBins - 1 ? first : 0) + rank;
    }
    else {
        const int wave = threadIdx.x >> 6;
        __syncthreads();
        if (lane == 0) sHist[wave] = __popcll(bWalk);
        __syncthreads();
        const int c0 = sHist[0], c1 = sHist[1], c2 = sHist[2], c3 = sHist[3];
        count = c0 + c1 + c2 + c3;
        const int before = (wave > 0 ? c0 : 0) + (wave > 1 ? c1 : 0) + (wave > 2 ? c2 : 0);
        slot = before + __popcll(bWalk & ((1ull << lane) - 1ull));
    }
    if (walk) {                                                 // slot < count <= 256
        sRay[slot] = make_float4(pos.x, pos.y, pos.z, __int_as_float(index));
        sRay[kShadowRegroupRays + slot] = make_float4(end.x, end.y, end.z, 0.f);
    }
    __syncthreads();
    if ((int)(threadIdx.x & ~63u) >= count) return;             // a wave without a ray (wave-uniform); count = 0: the whole block
    const bool mine = (int)threadIdx.x < count;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (mine) { a = sRay[threadIdx.x]; b = sRay[kShadowRegroupRays + threadIdx.x]; }
    const bool occluded = trace_occluded_wave(s, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mine);
    const bool mark = mine && occluded;
    if (mark) flag[__float_as_int(a.w)] = epoch;
    const unsigned long long bMark = __ballot(mark);
    if (lane == 0 && bMark) atomicAdd(stat_of(stats, 2), (unsigned long long)__popcll(bMark));
}

}  // namespace

void rs_revalidate_free(rs_shadow_revalidation& v) {
    rs_dev_free(v.flag); rs_dev_free(v.dStats);
}

// The scene and its count of edits are noted whether the switch is on or not (a later switch-on knows what the previous frame saw).
// On, in a call that merges: the frame's choice from the scene's ring at enqueue time, and the launch on the library stream behind
// k_retarget.  *marks: what the call's merge takes (flag null: the unmarked form, the kernel of a frame without this feature).
int rs_revalidate_phase_a(rs_restir* r, const rs_scene* scene, bool merges, const SurfPlanes& sp, const GBufView& g, int y0, int y1, int tilesX, int tilesY,
                          unsigned long long* rayCounter, const int* rtFlag, RevalMarks* marks) {
    rs_shadow_revalidation& v = r->reval;
    *marks = RevalMarks{ nullptr, 0u };
    if (v.fresh && (v.sceneId == 0 || v.sceneId == scene->id)) { v.sceneId = scene->id; v.seen = scene->geomEdits; }
    v.frameScene = scene->id; v.frameEdits = scene->geomEdits;
    if (!v.on || !merges) return 0;
    rs_revalidate_choice c;
    rs_plan_revalidation(scene->dirty.e, scene->dirty.count, v.seen, scene->geomEdits, v.sceneId == scene->id, c);
    if (!c.launch) return 0;
    if (!v.launched) {
        RS_HIP(hipMemsetAsync(v.dStats, 0, kStatWords * sizeof(unsigned long long), rs_stream()));
        v.launched = true;
    }
    if (++v.epoch == 0u) {                                      // 2^32 launches: the plane's words start again
        RS_HIP(hipMemsetAsync(v.flag, 0, (size_t)r->width * r->height * sizeof(unsigned), rs_stream()));
        v.epoch = 1u;
    }
    const bool regroup = r->shadowRegroup && scene->dev.occNodes;
    float scale = 0.f;
    if (regroup) {
        const float lo[3] = { scene->dev.occRootLo.x, scene->dev.occRootLo.y, scene->dev.occRootLo.z }, hi[3] = { scene->dev.occRootHi.x, scene->dev.occRootHi.y, scene->dev.occRootHi.z };
        scale = shadow_bins_over_extent(lo, hi);
    }
    rs_dispatch([&](auto REGROUP) {
        hipLaunchKernelGGL((k_revalidate<REGROUP()>), dim3(tilesX * tilesY), dim3(kShadowRegroupRays), 0, rs_stream(), scene->dev, sp.posMat, g, r->last, rtFlag, c.boxes,
                           v.flag, v.epoch, g.width, y0, y1, tilesX, scale, rayCounter, v.dStats);
    }, regroup);
    *marks = RevalMarks{ v.flag, v.epoch };
    return 0;
}

void rs_revalidate_end_frame(rs_shadow_revalidation& v, int phaseACalls) {
    if (phaseACalls > 0) { v.sceneId = v.frameScene; v.seen = v.frameEdits; v.fresh = false; }
    v.launchedLast = v.launched; v.launched = false;
}

extern "C" {

// Everything that can fail comes before anything of the object changes.  The plane starts as zeros and the epochs from 1; the edits made
// so far count as seen at the next frame (fresh).
int rs_restir_set_shadow_revalidation(rs_restir* r, int enable) {
    RS_SCOPE(r);
    if (!r) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_restir_set_shadow_revalidation: null");
    rs_shadow_revalidation& v = r->reval;
    const bool on = enable != 0;
    if (on == v.on) return 0;
    if (on && !v.flag) {
        const size_t n = (size_t)r->width * r->height;
        unsigned* flag = nullptr;
        unsigned long long* stats = nullptr;
        int e = rs_dev_alloc(&flag, n);
        if (!e) e = rs_dev_alloc(&stats, kStatWords);
        if (!e) e = rs_check_hip(hipMemset(flag, 0, n * sizeof(unsigned)), "hipMemset");
        if (!e) e = rs_check_hip(hipMemset(stats, 0, kStatWords * sizeof(unsigned long long)), "hipMemset");
        if (e) { rs_dev_free(flag); rs_dev_free(stats); return e; }
        v.flag = flag; v.dStats = stats; v.epoch = 0;
    }
    v.on = on;
    v.fresh = on;
    v.launched = v.launchedLast = false;
    return 0;
}

int rs_restir_get_shadow_revalidation(const rs_restir* r, int* enabled) {
    if (!r || !enabled) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_restir_get_shadow_revalidation: null argument");
    *enabled = r->reval.on ? 1 : 0;
    return 0;
}

// test hook: what k_revalidate did in the frame that rs_restir_end_frame ended last -- { candidates examined, segments walked, candidates
// found occluded }; zeros when that frame did not launch it
int rs_debug_restir_revalidate(rs_restir* r, unsigned long long out[3]) {
    RS_SCOPE(r);
    if (!r || !out) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_restir_revalidate: null argument");
    out[0] = out[1] = out[2] = 0;
    if (!r->reval.on || !r->reval.launchedLast) return 0;
    RS_HIP(hipStreamSynchronize(rs_stream()));
    unsigned long long host[kStatWords];
    RS_HIP(hipMemcpy(host, r->reval.dStats, sizeof(host), hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; k++) for (int i = 0; i < kRaySub; i++) out[k] += host[((size_t)k * kRaySub + i) * kRayStride];
    return 0;
}

// ... and whether that frame launched it at all
int rs_debug_restir_revalidate_launched(rs_restir* r, int* launched) {
    if (!r || !launched) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_restir_revalidate_launched: null argument");
    *launched = r->reval.on && r->reval.launchedLast ? 1 : 0;
    return 0;
}

// the plan's functions for callers without a device (rs_revalidate_plan.h)
int rs_debug_plan_dirty_box(int numPrims, const float* oldVertices, int count, const int* primIds, const float* newVertices, float lo[3], float hi[3]) {
    if (numPrims < 0 || count < 0 || !lo || !hi || (count > 0 && (!oldVertices || !primIds || !newVertices))) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_plan_dirty_box: bad argument");
    for (int j = 0; j < count; j++) if (primIds[j] < 0 || primIds[j] >= numPrims) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_plan_dirty_box: a primitive id out of range");
    rs_plan_dirty_box(oldVertices, count, primIds, newVertices, false, lo, hi);
    return 0;
}

// numEdits edits (boxes6: lo, hi each) numbered firstEdit, firstEdit + 1, ... go through the ring one after the other, then a frame that
// saw `seen` edits chooses at `now`
int rs_debug_plan_revalidation(int numEdits, unsigned long long firstEdit, const float* boxes6, unsigned long long seen, unsigned long long now, int sameScene,
                               int* launch, int* everything, int* n, float* outBoxes6) {
    if (numEdits < 0 || (numEdits > 0 && !boxes6) || !launch || !everything || !n) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_plan_revalidation: bad argument");
    rs_dirty_ring ring;
    for (int i = 0; i < numEdits; i++) rs_dirty_ring_push(ring, firstEdit + (unsigned long long)i, boxes6 + (size_t)i * 6, boxes6 + (size_t)i * 6 + 3);
    rs_revalidate_choice c;
    rs_plan_revalidation(ring.e, ring.count, seen, now, sameScene != 0, c);
    *launch = c.launch; *everything = c.boxes.everything; *n = c.boxes.n;
    for (int i = 0; outBoxes6 && i < c.boxes.n; i++)
        for (int k = 0; k < 3; k++) { outBoxes6[i * 6 + k] = c.boxes.box[i].lo[k]; outBoxes6[i * 6 + 3 + k] = c.boxes.box[i].hi[k]; }
    return 0;
}

// n segments (6 floats: a, b) against m boxes (6 floats: lo, hi), or against "everything": flags[i] = the segment walks
int rs_debug_segment_in_boxes(int n, const float* segments6, int m, const float* boxes6, int everything, unsigned char* flags) {
    if (n < 0 || m < 0 || m > RS_DIRTY_BOXES_KEPT || (n > 0 && (!segments6 || !flags)) || (m > 0 && !boxes6)) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_segment_in_boxes: bad argument");
    rs_revalidate_boxes b{};
    b.n = m; b.everything = everything != 0;
    for (int i = 0; i < m; i++) for (int k = 0; k < 3; k++) { b.box[i].lo[k] = boxes6[i * 6 + k]; b.box[i].hi[k] = boxes6[i * 6 + 3 + k]; }
    for (int i = 0; i < n; i++) {
        const float* q = segments6 + (size_t)i * 6;
        flags[i] = rs_segment_in_boxes(q[0], q[1], q[2], q[3], q[4], q[5], b) ? 1 : 0;
    }
    return 0;
}

}  // extern "C"
