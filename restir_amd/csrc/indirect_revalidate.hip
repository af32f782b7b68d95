// indirect_revalidate.hip -- revalidation of ReSTIR-GI's history (rs_indirect_revalidation, rs_internal.h): after an accepted geometry
// edit, the slots of the buffer rs_restir_indirect is about to merge from whose sample point lies in the edit's box, or whose segment
// xv -> xs crosses the box and is blocked on the current geometry, are emptied before k_path reads them.  The switch, what an
// rs_restir_indirect call does to the state, k_revalidate_indirect and the entry points of include/restir_hip.h that are only about this.
// The per-slot rule is rs_indirect_revalidate.h's, the frame's choice of boxes rs_revalidate_plan.h's (shared with shadow revalidation).
#include "rs_light_history.h"
#include "rs_indirect_revalidate.h"

using namespace rs;

namespace {

// { examined, stale, walked, occluded }: each counter is kRaySub partial ones, 64 B apart, as shadow revalidation's are
constexpr int kIndStats = 4;
constexpr int kStatWords = kIndStats * kRaySub * kRayStride;
__device__ __forceinline__ unsigned long long* stat_of(unsigned long long* stats, int k) { return stats + ((size_t)k * kRaySub + blockIdx.x % kRaySub) * kRayStride; }

constexpr int kIndLanes = 256;

// One lane per history slot j < n, 256 slots per block in the buffer's order.  A lane classifies its slot (rs_indirect_slot_class).  A
// stale one is emptied at once: numSamples = 0 and weight = 0, two words, the sample fields stay -- k_path then merges an empty candidate,
// draws its u and never selects it, as for a neighbour that fails findTemporalNeighbor.  Walkers are few -- the segments through a moved
// box -- so the block compacts them through LDS into dense slots before any ray walks, in slot order (a ballot per wave, the waves'
// counts through LDS).  Lane t then walks the segment of dense slot t; a wave whose slots are all empty leaves before it touches the
// tree, so a block without a walker reads no node at all.  An occluded walker empties its slot the same way.  Nobody else reads or writes
// the buffer while the kernel runs (the library stream's order), and a lane writes only the slot it read or was handed.
// LDS: 2 x 256 float4 + 4 counts = 8 208 B.  stats: { examined, stale, walked, occluded } (stat_of), one atomic per wave each.
__global__ void __launch_bounds__(kIndLanes, RS_WALK_WAVES) k_revalidate_indirect(DevScene s, rs_indirect_reservoir* resv, int n, rs_revalidate_boxes boxes,
                                                                                 unsigned long long* stats) {
    __shared__ float4 sRay[2 * kIndLanes];
    __shared__ int sCount[kIndLanes / 64];
    RS_SETPRIO(RS_PRIO_WALK);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * kIndLanes + threadIdx.x;
    const bool inside = j < n;
    float* f = reinterpret_cast<float*>(resv + (inside ? j : 0));
    float xv[3] = { 0.f, 0.f, 0.f }, xs[3] = { 0.f, 0.f, 0.f };
    int cls = RS_IND_NOT_EXAMINED;
    if (inside) {
        xv[0] = f[3]; xv[1] = f[4]; xv[2] = f[5];
        xs[0] = f[9]; xs[1] = f[10]; xs[2] = f[11];
        cls = rs_indirect_slot_class(f[16], xv, xs, boxes);
    }
    const bool stale = cls == RS_IND_STALE, walk = cls == RS_IND_WALK;
    if (stale) { f[15] = __int_as_float(0); f[16] = 0.f; }
    const unsigned long long bExamine = __ballot(cls != RS_IND_NOT_EXAMINED), bStale = __ballot(stale), bWalk = __ballot(walk);
    if (lane == 0 && bExamine) {
        atomicAdd(stat_of(stats, 0), (unsigned long long)__popcll(bExamine));
        if (bStale) atomicAdd(stat_of(stats, 1), (unsigned long long)__popcll(bStale));
        if (bWalk) atomicAdd(stat_of(stats, 2), (unsigned long long)__popcll(bWalk));
    }
    // the walkers' dense slots
    if (lane == 0) sCount[wave] = __popcll(bWalk);
    __syncthreads();
    const int c0 = sCount[0], c1 = sCount[1], c2 = sCount[2], c3 = sCount[3];
    const int count = c0 + c1 + c2 + c3;
    const int before = (wave > 0 ? c0 : 0) + (wave > 1 ? c1 : 0) + (wave > 2 ? c2 : 0);
    const int slot = before + __popcll(bWalk & ((1ull << lane) - 1ull));
    if (walk) {                                                 // slot < count <= 256
        sRay[slot] = make_float4(xv[0], xv[1], xv[2], __int_as_float(j));
        sRay[kIndLanes + slot] = make_float4(xs[0], xs[1], xs[2], 0.f);
    }
    __syncthreads();
    if ((int)(threadIdx.x & ~63u) >= count) return;             // a wave without a ray (wave-uniform); count = 0: the whole block
    const bool mine = (int)threadIdx.x < count;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (mine) { a = sRay[threadIdx.x]; b = sRay[kIndLanes + threadIdx.x]; }
    const bool occluded = trace_occluded_wave(s, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mine);      // testOcclusion(xv, xs)
    const bool drop = mine && occluded;
    if (drop) {                                                 // a.w: a slot index some lane of this block read, < n
        float* g = reinterpret_cast<float*>(resv + __float_as_int(a.w));
        g[15] = __int_as_float(0); g[16] = 0.f;
    }
    const unsigned long long bDrop = __ballot(drop);
    if (lane == 0 && bDrop) atomicAdd(stat_of(stats, 3), (unsigned long long)__popcll(bDrop));
}

int read_stats(const rs_indirect_revalidation& v, unsigned long long out[kIndStats]) {
    unsigned long long host[kStatWords];
    RS_HIP(hipMemcpy(host, v.dStats, sizeof(host), hipMemcpyDeviceToHost));
    for (int k = 0; k < kIndStats; k++) {
        out[k] = 0;
        for (int i = 0; i < kRaySub; i++) out[k] += host[((size_t)k * kRaySub + i) * kRayStride];
    }
    return 0;
}

}  // namespace

void rs_indirect_revalidate_free(rs_indirect_revalidation& v) {
    rs_dev_free(v.dStats);
}

// On, in a call that merges: the frame's choice from the scene's ring at enqueue time, and the launch on the library stream in front of
// k_path.  A call that launches nothing enqueues nothing: it leaves every buffer as the switch off leaves it.
int rs_indirect_revalidate_before_path(rs_restir* r, const rs_scene* scene, bool merges, rs_indirect_reservoir* history, size_t n) {
    rs_indirect_revalidation& v = r->indReval;
    v.launchedLast = false;
    if (!v.on || !merges || n == 0) return 0;
    rs_revalidate_choice c;
    rs_plan_revalidation(scene->dirty.e, scene->dirty.count, v.seen, scene->geomEdits, v.sceneId == scene->id, c);
    if (!c.launch) return 0;
    RS_HIP(hipMemsetAsync(v.dStats, 0, kStatWords * sizeof(unsigned long long), rs_stream()));
    const unsigned blocks = (unsigned)((n + kIndLanes - 1) / kIndLanes);
    hipLaunchKernelGGL(k_revalidate_indirect, dim3(blocks), dim3(kIndLanes), 0, rs_stream(), scene->dev, history, (int)n, c.boxes, v.dStats);
    v.launchedLast = true;
    return 0;
}

// the scene and its count of edits are noted whether the switch is on or not (a later switch-on knows what the previous call saw)
void rs_indirect_revalidate_note(rs_restir* r, const rs_scene* scene) {
    r->indReval.sceneId = scene->id; r->indReval.seen = scene->geomEdits;
}

// behind rs_walk_counters_sum, which has waited for the stream
int rs_indirect_revalidate_add_rays(rs_restir* r, unsigned long long* rays) {
    if (!rays || !r->indReval.launchedLast) return 0;
    unsigned long long st[kIndStats];
    RS_TRY(read_stats(r->indReval, st));
    *rays += st[2];
    return 0;
}

extern "C" {

// Everything that can fail comes before anything of the object changes.  Switching on or off forgets nothing: the previous call's
// scene and count are kept either way, so an edit that a call has seen while the switch was off is never revalidated later.
int rs_restir_set_indirect_revalidation(rs_restir* r, int enable) {
    RS_SCOPE(r);
    if (!r) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_restir_set_indirect_revalidation: null");
    rs_indirect_revalidation& v = r->indReval;
    const bool on = enable != 0;
    if (on == v.on) return 0;
    if (on && !v.dStats) {
        unsigned long long* stats = nullptr;
        int e = rs_dev_alloc(&stats, kStatWords);
        if (!e) e = rs_check_hip(hipMemset(stats, 0, kStatWords * sizeof(unsigned long long)), "hipMemset");
        if (e) { rs_dev_free(stats); return e; }
        v.dStats = stats;
    }
    v.on = on;
    v.launchedLast = false;
    return 0;
}

int rs_restir_get_indirect_revalidation(const rs_restir* r, int* enabled) {
    if (!r || !enabled) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_restir_get_indirect_revalidation: null argument");
    *enabled = r->indReval.on ? 1 : 0;
    return 0;
}

// test hook: what k_revalidate_indirect did in the last rs_restir_indirect call -- { slots examined, found stale, segments walked, walkers
// found occluded }; zeros when that call did not launch it
int rs_debug_restir_indirect_revalidate(rs_restir* r, unsigned long long out[4]) {
    RS_SCOPE(r);
    if (!r || !out) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_restir_indirect_revalidate: null argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!r->indReval.on || !r->indReval.launchedLast) return 0;
    RS_HIP(hipStreamSynchronize(rs_stream()));
    return read_stats(r->indReval, out);
}

// ... and whether that call launched it at all
int rs_debug_restir_indirect_revalidate_launched(rs_restir* r, int* launched) {
    if (!r || !launched) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_restir_indirect_revalidate_launched: null argument");
    *launched = r->indReval.on && r->indReval.launchedLast ? 1 : 0;
    return 0;
}

// the per-slot rule for callers without a device (rs_indirect_revalidate.h): n reservoirs against m boxes (6 floats: lo, hi), or against
// "everything"
int rs_debug_indirect_candidate_classes(int n, const rs_indirect_reservoir* reservoirs, int m, const float* boxes6, int everything, unsigned char* classes) {
    if (n < 0 || m < 0 || m > RS_DIRTY_BOXES_KEPT || (n > 0 && (!reservoirs || !classes)) || (m > 0 && !boxes6))
        return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_indirect_candidate_classes: bad argument");
    rs_revalidate_boxes b{};
    b.n = m; b.everything = everything != 0;
    for (int i = 0; i < m; i++) for (int k = 0; k < 3; k++) { b.box[i].lo[k] = boxes6[i * 6 + k]; b.box[i].hi[k] = boxes6[i * 6 + 3 + k]; }
    for (int i = 0; i < n; i++) classes[i] = (unsigned char)rs_indirect_slot_class(reservoirs[i].weight, reservoirs[i].xv, reservoirs[i].xs, b);
    return 0;
}

}  // extern "C"
