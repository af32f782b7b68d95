// rs_light_history.h -- what the kernels of restir.hip and light_history.hip share: the per-pixel planes between the passes of a frame and
// the kernel arguments of light tracking and retargeting.  LIGHTS: the mode of rs_light_history (rs_internal.h) as a template argument.
#pragma once
#include "rs_internal.h"

#if defined(__HIPCC__)
namespace rs {

// kind of a pixel after the primary hit
constexpr int kKindMiss = 0, kKindLight = 1, kKindShaded = 2;
// per-pixel tag: material id (24 bits) | kind << 24 (2 bits) | Material::Type << 26 (3 bits)
__device__ __forceinline__ int mk_kind(int mk) { return (mk >> 24) & 3; }
__device__ __forceinline__ int mk_type(int mk) { return (mk >> 26) & 7; }
constexpr int kRaySub = 64, kRayStride = 8;   // BVH-walk counters per frame: 64 partial counters, 64 B apart (one hot address cost ~85 us/frame)

struct SurfPlanes {
    float4* posMat;     // pos.xyz (radiance of the environment map for a miss pixel of an env-mapped scene), bits(tag)
    float4* norm;       // shading normal xyz (normal-mapped, flipped to the wo side), w = metallic (after its map)
    float4* wo;         // wo.xyz, w = roughness (after its map); written and read only for the metallic BSDF
    uint2*  rngMat;     // { RNG state carried from pass to pass, matId | kind << 24 }: all the spatial pass needs for a Lambertian pixel
    float4* candLi;     // RIS winner Li.xyz, dist
    float4* candWi;     // RIS winner wi.xyz, reservoir weight
};

// a RIS kernel's winners beside SurfPlanes: the light-sampler index (LIGHTS >= 1; -1: no winner) and the record { light, u, v, pdf }
template <int LIGHTS> struct RisWinners { int* id; };
template <> struct RisWinners<2> { int* id; float4* rec; };

// Light tracking (rs_restir_set_light_tracking): the light-sampler index of the RIS winners (cand), of the reservoirs the merge reads
// (last) and of those it publishes (cur), and the light records of the scene's current emission
struct LightIds {
    const int* cand; const int* last; int* cur;
    int* temp;                       // of the published copy the spatial pass gathers from (TempPlanes)
    const LightRec* lights;
    int numLights, envId;            // envId: the environment map's sampler entry, -1 = none
};
// Retargeting (rs_restir_set_light_retargeting): the records { light, u, v, pdf } of the RIS winners (cand), of the reservoirs the merge
// reads (last) and publishes (cur, temp), and what k_retarget left for this frame: flag[i] != 0 -- pixel i's temporal candidate is
// { rtLi | rtWi (w = W) | rtRec }[i] instead of last[motion[i]]; M stays the slot's.  flag null: k_retarget was not launched.
struct LightRecs {
    const float4* cand; const float4* last; float4* cur; float4* temp;
    const float4* rtLi; const float4* rtWi; const float4* rtRec; const int* flag;
};
// the temporal merge's light argument (ids: all null with LIGHTS = 0)
template <int LIGHTS> struct MergeLights { LightIds ids; };
template <> struct MergeLights<2> { LightIds ids; LightRecs recs; };
template <int LIGHTS> inline MergeLights<LIGHTS> merge_lights(const LightIds& ids, const LightRecs& recs) {
    if constexpr (LIGHTS == 2) return { ids, recs }; else return { ids };
}
// k_retarget's planes
struct RetargetOut { float4* li; float4* wi; float4* rec; int* flag; };

}  // namespace rs

// the mode as a template argument: f is called once with a std::integral_constant<int, mode> (as rs_dispatch does with booleans)
template <typename F> inline void rs_dispatch_lights(int mode, F&& f) {
    if (mode == 2) f(std::integral_constant<int, 2>{}); else if (mode == 1) f(std::integral_constant<int, 1>{}); else f(std::integral_constant<int, 0>{});
}
// the winners' planes of surface set `set` for a RIS launch in mode LIGHTS (the caller dispatched on h.mode)
template <int LIGHTS> inline rs::RisWinners<LIGHTS> rs_light_history_winners(const rs_light_history& h, int set) {
    if constexpr (LIGHTS == 2) return { h.candId[set], h.candRec[set] }; else return { LIGHTS ? h.candId[set] : nullptr };
}
// What phase_a_impl (restir.hip) asks after the chain's join, on the library stream: a scene other than the one the history names makes
// last and the published copy unknown and takes its count of moves as seen; lamps that moved since the previous frame, when this frame
// merges, launch k_retarget for rows [y0, y1); *ids / *recs: what the call's merge takes for surface set `set` (null below their mode).
int rs_light_history_phase_a(rs_light_history& h, const rs_scene* scene, int set, bool merges, const rs::SurfPlanes& sp, const GBufView& g, const ResvPlanes& last,
                             int y0, int y1, int tilesX, int tilesY, unsigned long long* rayCounter, rs::LightIds* ids, rs::LightRecs* recs);
#endif
