// scene_edits.hip -- edits of a live scene (include/restir_hip.h), all stream-ordered: the ring of versions behind rs_scene_set_emission /
// rs_scene_set_materials / rs_scene_set_texture; geometry edits in place behind fences (rs_set_geometry, the one implementation of
// rs_scene_set_triangles and rs_scene_set_geometry here and of the deformers' edits in scene_deform.hip: its host decisions are
// rs_geometry_plan.h's, its kernels scene_refit.hip's); motion tracking; the refit's and the plans' debug hooks.  The scene itself, its
// trees and its debug tables: scene.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rs_internal.h"
#include "rs_refit.h"

using namespace rs;

// Edits are not recorded into graphs: a captured frame keeps the tables it was captured with
int refuse_while_capturing(const char* name) {
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(rs_stream(), &capturing) != hipSuccess) { (void)hipGetLastError(); capturing = hipStreamCaptureStatusNone; }
    if (capturing != hipStreamCaptureStatusNone) return rs_fail(RS_ERR_UNSUPPORTED, (std::string(name) + ": the library stream is being captured into a graph").c_str());
    return 0;
}

namespace {

// a refusal of rs_geometry_plan.h: its text is in `why` (empty: a library call inside the plan failed and has reported it)
int refused(int code, const std::string& why) { return why.empty() ? code : rs_fail(code, why.c_str()); }

// Byte offsets of one version's tables in its staging buffer (each 64-byte aligned)
struct VersionLayout { size_t mat, light, alias, tex, moved, total; };
VersionLayout version_layout(const rs_scene* s) {
    auto up = [](size_t b) { return (b + 63) & ~(size_t)63; };
    VersionLayout l;
    l.mat = 0;
    l.light = up(s->hMaterials.size() * sizeof(rs_material));
    l.alias = l.light + up((size_t)s->numLights * sizeof(LightRec));
    l.tex = l.alias + up((size_t)s->numLights * sizeof(AliasRec));
    l.moved = l.tex + up(s->hTextures.size() * sizeof(TexRec));
    l.total = l.moved + up((size_t)s->numLights * sizeof(uint32_t));
    return l;
}

// The power of an environment map's sampler entry: the sum of its pdf (left in `pdf`), in rs_build_alias_table's order
int env_power(int width, int height, const float* data, std::vector<float>& pdf, float* total) {
    pdf.resize((size_t)width * height);
    RS_TRY(rs_build_envmap_pdf(width, height, data, pdf.data()));
    *total = 0.f;
    for (float p : pdf) *total += p;
    return 0;
}

// First edit: slots 1.. of the version ring, every slot's staging buffer and events, the per-light areas and the environment map's power
int versions_prepare(rs_scene* s) {
    if (s->verReady) return 0;
    const VersionLayout l = version_layout(s);
    const size_t nm = s->hMaterials.size(), nl = (size_t)s->numLights, nt = s->hTextures.size();
    s->ver[0].materials = s->dMaterials; s->ver[0].lights = s->dLights; s->ver[0].alias = s->dAlias; s->ver[0].textures = s->dTextures;
    for (int v = 0; v < rs_scene::kVersions; v++) {
        rs_scene::Version& x = s->ver[v];
        if (v > 0) {
            RS_TRY(rs_dev_alloc(&x.materials, nm));
            RS_TRY(rs_dev_alloc(&x.lights, nl));
            RS_TRY(rs_dev_alloc(&x.alias, nl));
            if (nt) RS_TRY(rs_dev_alloc(&x.textures, nt));
        }
        RS_TRY(rs_dev_alloc(&x.moved, nl));
        RS_HIP(hipMemset(x.moved, 0, (nl ? nl : 1) * sizeof(uint32_t)));
        RS_HIP(hipHostMalloc((void**)&x.staging, l.total, hipHostMallocDefault));
        for (hipEvent_t& e : x.retired) RS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    s->texEdited.assign(nt, rs_scene::Edited{});
    for (size_t i = 0; i < nt; i++) s->texEdited[i].dev[0] = s->dTexData[i];
    s->envEdited = rs_scene::Edited{};
    s->envEdited.dev[0] = s->dEnvAlias;
    RS_HIP(hipEventCreateWithFlags(&s->verFilled, hipEventDisableTiming));
    RS_HIP(hipStreamCreateWithFlags(&s->verStream, hipStreamNonBlocking));
    // Math::triangleArea of every light primitive, as rs_build_light_table computes it (scene_build.cpp)
    s->hLightMoved.assign(nl, 0u);
    s->hLightOfPrim.assign((size_t)s->numPrims, -1);
    for (size_t i = 0; i < s->hLightPrimIds.size(); i++) s->hLightOfPrim[(size_t)s->hLightPrimIds[i]] = (int)i;
    s->hLightArea.resize(s->hLightPrimIds.size());
    for (size_t i = 0; i < s->hLightArea.size(); i++) s->hLightArea[i] = triangle_area(&s->hVertices[(size_t)s->hLightPrimIds[i] * 9]);
    // the environment map's sampler entry keeps its power: the sum of its pdf, as rs_scene_build_textured passes it on (a scene made by
    // rs_scene_create from a description does not carry it)
    if (s->envMapTexId >= 0 && !s->envPowerKnown) {
        const rs_texture& env = s->hTextures[(size_t)s->envMapTexId];
        std::vector<float> pdf;
        RS_TRY(env_power(env.width, env.height, env.data, pdf, &s->envPower));
        s->envPowerKnown = true;
    }
    s->verReady = true;
    return 0;
}

void edited_free(rs_scene::Edited& e) {
    for (int k = 0; k < rs_scene::kEditedCopies; k++) {
        if (k > 0 && e.dev[k]) (void)hipFree(e.dev[k]);           // ([0] is the scene's own array)
        if (e.staging[k]) (void)hipHostFree(e.staging[k]);
        e.dev[k] = nullptr; e.staging[k] = nullptr;
    }
}

}  // namespace

void versions_free(rs_scene* s) {
    for (int v = 0; v < rs_scene::kVersions; v++) {
        rs_scene::Version& x = s->ver[v];
        if (v > 0) { rs_dev_free(x.materials); rs_dev_free(x.lights); rs_dev_free(x.alias); rs_dev_free(x.textures); }
        rs_dev_free(x.moved);
        if (x.staging) { (void)hipHostFree(x.staging); x.staging = nullptr; }
        for (hipEvent_t& e : x.retired) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    }
    for (rs_scene::Edited& e : s->texEdited) edited_free(e);
    edited_free(s->envEdited);
    if (s->verFilled) { (void)hipEventDestroy(s->verFilled); s->verFilled = nullptr; }
    if (s->verStream) { (void)hipStreamDestroy(s->verStream); s->verStream = nullptr; }
}

// what rs_scene_set_motion_tracking allocated
void motion_free(rs_scene* s) {
    rs_dev_free(s->dPrevVertices);
    for (hipEvent_t& e : s->motionBefore) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    if (s->motionAfter) { (void)hipEventDestroy(s->motionAfter); s->motionAfter = nullptr; }
}

namespace {

// the host waits until no launch that captured the slot still runs: for the events recorded when the scene moved off it
int wait_retired(rs_scene::Version& x) {
    for (int k = 0; k < rs_scene::kVersionStreams; k++)
        if (x.retiredValid[k]) { RS_HIP(hipEventSynchronize(x.retired[k])); x.retiredValid[k] = false; }
    return 0;
}

// An edit, first half (the new host tables have been built and checked; nothing of the scene has changed yet): launches what has only
// been recorded, with the old tables, and frees the slot the edit will fill.
int version_begin(rs_scene* s) {
    // frames in flight: a render that has only been recorded captures `dev` when it is launched -- launch it now, with the old tables
    RS_TRY(rs_gbuffer_release_scene(s));
    return wait_retired(s->ver[(s->verCur + 1) % rs_scene::kVersions]);      // (the ring has run out only if a launch that captured the slot still runs)
}

// Between version_begin and version_commit: the edit replaces the contents of `e` (`bytes`).  They go, on the fills' stream, to an array
// that no version in flight points at -- edited_reserve finds it, edited_fill writes it, so that an edit that replaces two (the
// environment map's texels and its alias table) has reserved both before it changes either.  version_begin has waited for version
// verSeq + 1 - kVersions, and versions retire in order, so an array last used kVersions edits back is free; failing that a new one is
// allocated while the Edited may grow; failing that the host waits for the versions that read the array left longest ago.
int edited_reserve(rs_scene* s, rs_scene::Edited& e, size_t bytes, int* which) {
    const unsigned long long newSeq = s->verSeq + 1;
    int k = -1;
    for (int i = 0; i < e.count && k < 0; i++)
        if (i != e.cur && e.lastSeq[i] + rs_scene::kVersions <= newSeq) k = i;
    if (k < 0 && e.count < rs_scene::kEditedCopies) {
        RS_HIP(hipMalloc(&e.dev[e.count], bytes ? bytes : 1));
        e.lastSeq[e.count] = 0;                                  // (never pointed at yet)
        k = e.count++;
    }
    if (k < 0) {
        for (int i = 0; i < e.count; i++)
            if (i != e.cur && (k < 0 || e.lastSeq[i] < e.lastSeq[k])) k = i;
        // the versions up to lastSeq[k] retire in order, and the events of lastSeq[k] are still in its slot (less than kVersions edits back)
        RS_TRY(wait_retired(s->ver[e.lastSeq[k] % rs_scene::kVersions]));
    }
    if (!e.staging[k]) RS_HIP(hipHostMalloc((void**)&e.staging[k], bytes ? bytes : 1, hipHostMallocDefault));
    *which = k;
    return 0;
}
int edited_fill(rs_scene* s, rs_scene::Edited& e, int k, const void* src, size_t bytes) {
    std::memcpy(e.staging[k], src, bytes);
    RS_HIP(hipMemcpyAsync(e.dev[k], e.staging[k], bytes, hipMemcpyHostToDevice, s->verStream));
    e.lastSeq[e.cur] = s->verSeq;
    e.cur = k;
    return 0;
}

// An edit, second half (the scene's host tables are the new ones): fills the next slot from them and moves the scene there.
int version_commit(rs_scene* s, const char* what) {
    const int next = (s->verCur + 1) % rs_scene::kVersions;
    rs_scene::Version& nv = s->ver[next];
    const size_t nl = (size_t)s->numLights, nt = s->hTextures.size();
    const float sumInv = 1.f / s->sumLightPower;                         // scene.cpp:489
    const VersionLayout l = version_layout(s);
    std::memcpy(nv.staging + l.mat, s->hMaterials.data(), s->hMaterials.size() * sizeof(rs_material));
    light_records(s, sumInv, reinterpret_cast<LightRec*>(nv.staging + l.light), reinterpret_cast<AliasRec*>(nv.staging + l.alias));
    TexRec* recs = reinterpret_cast<TexRec*>(nv.staging + l.tex);
    for (size_t i = 0; i < nt; i++) {
        const rs_scene::Edited& e = s->texEdited[i];
        recs[i] = TexRec{ static_cast<float*>(e.dev[e.cur]), s->hTextures[i].width, s->hTextures[i].height };
    }
    if (nl) std::memcpy(nv.staging + l.moved, s->hLightMoved.data(), nl * sizeof(uint32_t));

    // the current slot is retired by what has been enqueued so far on the library stream and on every auxiliary stream
    hipStream_t aux[rs_context::kAux];
    rs_aux_streams_made(aux);
    const hipStream_t st = rs_stream();
    rs_scene::Version& ov = s->ver[s->verCur];
    RS_HIP(hipEventRecord(ov.retired[0], st)); ov.retiredValid[0] = true;
    for (int i = 0; i < rs_context::kAux; i++)
        if (aux[i]) { RS_HIP(hipEventRecord(ov.retired[1 + i], aux[i])); ov.retiredValid[1 + i] = true; }
    // The slot is free (no launch reads it), so its fill waits for nothing: it goes to a stream of the scene's own and the library and
    // auxiliary streams wait for that copy alone.  (Filled on the library stream, the edit would order the auxiliary streams after the
    // frames in flight there and end the overlap of consecutive frames: config 5 with an edit per frame 1.69 -> 3.12 ms.)
    RS_HIP(hipMemcpyAsync(nv.materials, nv.staging + l.mat, s->hMaterials.size() * sizeof(rs_material), hipMemcpyHostToDevice, s->verStream));
    if (nl) {
        RS_HIP(hipMemcpyAsync(nv.lights, nv.staging + l.light, nl * sizeof(LightRec), hipMemcpyHostToDevice, s->verStream));
        RS_HIP(hipMemcpyAsync(nv.alias, nv.staging + l.alias, nl * sizeof(AliasRec), hipMemcpyHostToDevice, s->verStream));
        RS_HIP(hipMemcpyAsync(nv.moved, nv.staging + l.moved, nl * sizeof(uint32_t), hipMemcpyHostToDevice, s->verStream));
    }
    if (nt) RS_HIP(hipMemcpyAsync(nv.textures, nv.staging + l.tex, nt * sizeof(TexRec), hipMemcpyHostToDevice, s->verStream));
    RS_HIP(hipEventRecord(s->verFilled, s->verStream));
    RS_HIP(hipStreamWaitEvent(st, s->verFilled, 0));             // launches from now on see the new tables
    for (int i = 0; i < rs_context::kAux; i++)
        if (aux[i]) RS_HIP(hipStreamWaitEvent(aux[i], s->verFilled, 0));
    s->dev.materials = nv.materials;
    s->dev.lights = nv.lights;
    s->dev.alias = nv.alias;
    if (nt) s->dev.textures = nv.textures;
    if (s->envMapTexId >= 0) s->dev.envAlias = static_cast<AliasRec*>(s->envEdited.dev[s->envEdited.cur]);
    s->dev.sumLightPowerInv = sumInv;
    s->verCur = next;
    s->verSeq++;
    s->edits++;                                                  // retained G-buffer planes are not this scene's any more
    return rs_after_launch(what);
}

}  // namespace

// Emission of Light-type materials, stream-ordered (include/restir_hip.h).  The host tables are rebuilt as rs_scene_build_textured builds
// them (rs_build_light_table's powers over the scene's light primitives, the environment map's entry last, rs_build_alias_table), so
// that the scene equals, bit for bit, one built afresh from the edited materials.  The device tables go to the next slot of the version
// ring (rs_internal.h rs_scene::Version): launches enqueued before the call keep reading the slot they captured.
extern "C" int rs_scene_set_emission(rs_scene* s, int count, const int* materialIds, const float* radiance) {
    RS_SCOPE(s);
    if (!s) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_set_emission: null scene");
    if (count < 0 || (count > 0 && (!materialIds || !radiance))) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_set_emission: count < 0 or null arrays");
    const int nm = (int)s->hMaterials.size();
    for (int i = 0; i < count; i++) {
        const int m = materialIds[i];
        if (m < 0 || m >= nm || s->hMaterials[(size_t)m].type != 4)
            return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_set_emission: a material id out of range or of a material that is not a Light");
        for (int k = 0; k < 3; k++) {
            const float x = radiance[(size_t)i * 3 + k];
            if (!(x >= 0.f) || std::isinf(x)) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_set_emission: radiance must be finite and >= 0");
        }
    }
    RS_TRY(refuse_while_capturing("rs_scene_set_emission"));
    RS_TRY(versions_prepare(s));

    // the new host tables (nothing of the scene changes before all of them have been built and checked)
    std::vector<rs_material> mats = s->hMaterials;
    for (int i = 0; i < count; i++) std::memcpy(mats[(size_t)materialIds[i]].baseColor, radiance + (size_t)i * 3, 3 * sizeof(float));
    const size_t nlp = s->hLightPrimIds.size();
    std::vector<float> rad(nlp * 3), prob;
    std::vector<int> fail;
    for (size_t i = 0; i < nlp; i++) st3(&rad[i * 3], ld3(mats[(size_t)s->hMaterialIds[(size_t)s->hLightPrimIds[i]]].baseColor));
    float sumAll = 0.f;
    std::string why;
    if (int e = light_sampler((size_t)s->numLights, nlp, rad.data(), s->hLightArea.data(), s->envPower, prob, fail, &sumAll, "rs_scene_set_emission", why)) return refused(e, why);

    RS_TRY(version_begin(s));
    s->hMaterials.swap(mats);
    s->hLightRadiance.swap(rad);
    s->hLightProb.swap(prob);
    s->hLightFailId.swap(fail);
    s->sumLightPower = sumAll;
    return version_commit(s, "rs_scene_set_emission");
}

// Material records, stream-ordered like the emission (include/restir_hip.h).  Light materials stay with rs_scene_set_emission: the light
// list, the emissive tree and the G-buffer's -2 ids are built from which materials are Lights.
extern "C" int rs_scene_set_materials(rs_scene* s, int count, const int* materialIds, const rs_material* records) {
    RS_SCOPE(s);
    if (!s) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_set_materials: null scene");
    if (count < 0 || (count > 0 && (!materialIds || !records))) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_set_materials: count < 0 or null arrays");
    const int nm = (int)s->hMaterials.size();
    for (int i = 0; i < count; i++) {
        const int m = materialIds[i];
        if (m < 0 || m >= nm) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_set_materials: a material id out of range");
        if (s->hMaterials[(size_t)m].type == 4 || records[i].type < 0 || records[i].type > 3)
            return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_set_materials: a material that is a Light or would become one (or of an unknown type); emission is edited by rs_scene_set_emission");
    }
    RS_TRY(refuse_while_capturing("rs_scene_set_materials"));
    if (count == 0) return 0;
    std::vector<rs_material> mats = s->hMaterials;
    for (int i = 0; i < count; i++) mats[(size_t)materialIds[i]] = records[i];           // a repeated id: the last record wins
    bool anyMap = false;
    RS_TRY(check_materials(nm, mats.data(), (int)s->hTextures.size(), &anyMap, "rs_scene_set_materials: material map id beyond the texture table",
                           "rs_scene_set_materials: invalid material map id"));
    if (anyMap && !s->hasTexcoords) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_set_materials: texture maps need texcoords, and the scene was created without");
    RS_TRY(versions_prepare(s));

    RS_TRY(version_begin(s));
    if (anyMap && !s->textured) {
        // the scene's first map: so far it ran the kernels that read no texture coordinates, and none are on the device
        if (!s->dTexcoords) RS_TRY(rs_dev_alloc(&s->dTexcoords, s->hTexcoords.size()));
        RS_HIP(hipMemcpyAsync(s->dTexcoords, s->hTexcoords.data(), s->hTexcoords.size() * sizeof(float), hipMemcpyHostToDevice, s->verStream));
        s->dev.texcoords = s->dTexcoords;
        s->textured = true;
    }
    s->hMaterials.swap(mats);
    return version_commit(s, "rs_scene_set_materials");
}

// The texels of one texture, stream-ordered like the emission (include/restir_hip.h).  For the environment map the host rebuilds what
// rs_scene_build_textured builds from it: the pdf, the map's alias table, its entry in the light sampler and with it the light sampler.
extern "C" int rs_scene_set_texture(rs_scene* s, int texId, int width, int height, const float* data) {
    RS_SCOPE(s);
    if (!s) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_set_texture: null scene");
    if (texId < 0 || texId >= (int)s->hTextures.size()) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_set_texture: texture id out of range");
    const rs_texture& t = s->hTextures[(size_t)texId];
    if (width != t.width || height != t.height || !data) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_set_texture: null data, or dimensions other than the texture's");
    RS_TRY(refuse_while_capturing("rs_scene_set_texture"));
    RS_TRY(versions_prepare(s));
    const size_t n = (size_t)width * height;
    const bool env = texId == s->envMapTexId;
    std::vector<float> envProb, prob;
    std::vector<int> envFail, fail;
    float envSum = 0.f, sumAll = 0.f;
    if (env) {
        std::vector<float> pdf;
        RS_TRY(env_power(width, height, data, pdf, &envSum));
        if (!(envSum > 0.f) || std::isinf(envSum)) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_set_texture: the environment map's pdf has no finite, positive sum");
        envProb.resize(n); envFail.resize(n);
        RS_TRY(rs_build_alias_table((int)n, pdf.data(), envProb.data(), envFail.data(), &envSum));
        std::string why;
        if (int e = light_sampler((size_t)s->numLights, s->hLightPrimIds.size(), s->hLightRadiance.data(), s->hLightArea.data(), envSum, prob, fail, &sumAll, "rs_scene_set_texture", why))
            return refused(e, why);
    }

    RS_TRY(version_begin(s));
    int texels = 0, alias = 0;
    RS_TRY(edited_reserve(s, s->texEdited[(size_t)texId], n * 3 * sizeof(float), &texels));
    if (env) RS_TRY(edited_reserve(s, s->envEdited, n * sizeof(AliasRec), &alias));
    RS_TRY(edited_fill(s, s->texEdited[(size_t)texId], texels, data, n * 3 * sizeof(float)));
    std::memcpy(s->hTexData[(size_t)texId].data(), data, n * 3 * sizeof(float));
    if (env) {
        const std::vector<AliasRec> al = alias_records(envProb, envFail);
        RS_TRY(edited_fill(s, s->envEdited, alias, al.data(), n * sizeof(AliasRec)));
        s->hEnvProb.swap(envProb);
        s->hEnvFail.swap(envFail);
        s->hLightProb.swap(prob);
        s->hLightFailId.swap(fail);
        s->sumLightPower = sumAll;
        s->envPower = envSum; s->envPowerKnown = true;
    }
    return version_commit(s, "rs_scene_set_texture");
}

// Triangles, stream-ordered (include/restir_hip.h).  Geometry is too large for the ring of versions (nodesAll alone is 6 x 32 bytes per
// node), so this edit works in place behind device-side fences: the library stream waits for what the internal streams have been handed
// so far, the edit's kernels (scene_refit.hip) run on the library stream, and the next launch of every internal stream waits for them.
// The host's tables follow at once: hVertices, hNormals, and hBoxes = rs_refit_boxes of the edited vertices.
//
// One implementation behind two entry points.  rs_scene_set_triangles refuses emitters and thereby guarantees that the light sampler, the
// light records and the emissive tree are untouched.  rs_scene_set_geometry takes them: an edit that names one also rebuilds the light
// sampler from the new areas (as rs_scene_set_emission does from new radiance), fills the next slot of the version ring -- light_records
// derives LightRec from hVertices -- and refits the emissive tree on a grid laid anew over the new emissive root box.  Both transitions
// are made at the same point of the library stream: the in-place edit behind before[] / after, the version switch behind verFilled, with
// no launch between them.  An edit through rs_scene_set_geometry that names no emitter does exactly what rs_scene_set_triangles does.
namespace {

// An edit in place of arrays that launches on the library's internal streams read (the geometry; the previous pose): the library stream waits,
// by events, for what those streams have been handed so far (fence_before), the edit's kernels run on the library stream, and the next
// launch of every internal stream waits for them (fence_after).  Launches enqueued before the edit read the old arrays, launches after it the new.
int fence_before(hipEvent_t* before) {
    hipStream_t aux[rs_context::kAux];
    rs_aux_streams_made(aux);
    for (int i = 0; i < rs_context::kAux; i++)
        if (aux[i]) { RS_HIP(hipEventRecord(before[i], aux[i])); RS_HIP(hipStreamWaitEvent(rs_stream(), before[i], 0)); }
    return 0;
}
int fence_after(hipEvent_t after) {
    hipStream_t aux[rs_context::kAux];
    rs_aux_streams_made(aux);
    RS_HIP(hipEventRecord(after, rs_stream()));
    for (int i = 0; i < rs_context::kAux; i++)
        if (aux[i]) RS_HIP(hipStreamWaitEvent(aux[i], after, 0));
    return 0;
}

// What rs_geometry_plan.h reads of the scene.  (hLightArea and envPower are versions_prepare's, emiRecords rs_refit_prepare's: the plan
// of the lights asks for the view again after them.)
rs_geometry_edit_view edit_view(const rs_scene* s) {
    rs_geometry_edit_view v{};
    v.numPrims = s->numPrims; v.materialIds = s->hMaterialIds.data(); v.materials = s->hMaterials.data();
    v.bounded = s->dOccNodes != nullptr;                // the 16-bit grid of the grid-box trees lies over the box the scene was created with
    for (int k = 0; k < 3; k++) { v.gridLo[k] = s->gridLo[k]; v.gridHi[k] = s->gridHi[k]; }
    v.vertices = s->hVertices.data();
    v.numLights = s->numLights; v.numLightPrims = (int)s->hLightPrimIds.size();
    v.lightPrimIds = s->hLightPrimIds.data(); v.lightRadiance = s->hLightRadiance.data(); v.lightArea = s->hLightArea.data();
    v.envPower = s->envPower;
    v.emissiveTree = s->refit && s->refit->emiRecords;
    v.numEmissive = (int)s->hEmiLeafPrims.size(); v.emiLeafPrims = s->hEmiLeafPrims.data();
    return v;
}

// The next buffer of the ring of pinned ones with room for `staged` bytes, and room for `onDevice` bytes in the device buffer
int stage_reserve(rs_refit* r, size_t staged, size_t onDevice, rs_refit::Stage** slot) {
    rs_refit::Stage& g = r->stage[r->stageNext];
    if (g.pending) { RS_HIP(hipEventSynchronize(g.copied)); g.pending = false; }      // the ring is full of edits whose copies have not finished
    if (g.capacity < staged) {
        if (g.host) { (void)hipHostFree(g.host); g.host = nullptr; g.capacity = 0; }
        size_t cap = 4096;
        while (cap < staged) cap *= 2;
        RS_HIP(hipHostMalloc((void**)&g.host, cap, hipHostMallocDefault));
        g.capacity = cap;
    }
    if (r->dStageCapacity < onDevice) {                  // (hipFree waits for the device: no earlier edit still reads the old buffer)
        rs_dev_free(r->dStage);
        r->dStageCapacity = 0;
        size_t cap = 4096;
        while (cap < onDevice) cap *= 2;
        RS_TRY(rs_dev_alloc(&r->dStage, cap));
        r->dStageCapacity = cap;
    }
    *slot = &g;
    return 0;
}

// the edit's m records, every id once, on the host: the staged ones, or -- a source's are staged in their place -- the caller's own arrays
struct Records { const int* ids; const float* vertices; const float* normals; };
Records fill_stage(char* host, const rs_geometry_edit_plan& plan, const rs_edit_stamps& stamps, int count, const int* primIds, const float* vertices,
                   const float* normals, const rs_record_source* source) {
    if (source) { std::memcpy(host, source->recs, plan.partStaged); return Records{ primIds, vertices, normals }; }
    rs_fill_edit_records(plan, stamps, count, primIds, vertices, normals, host);
    return Records{ reinterpret_cast<const int*>(host), reinterpret_cast<const float*>(host + plan.offV), reinterpret_cast<const float*>(host + plan.offN) };
}

// First edit.  Boxes that were not the exact unions (a caller-supplied table): from now on they are.  The emissive tree was built over the
// boxes as given, so it no longer answers for the new ones: the last bounce asks the scene's trees again, for good.
void make_boxes_exact(rs_scene* s) {
    rs_refit* r = s->refit;
    const size_t nn = (size_t)s->bvhSize;
    std::vector<float> exact(nn * 6);
    rs_refit_boxes_host(s->bvhSize, s->hVertices.data(), s->hNodes[0].data(), s->hParent.data(), exact.data());
    bool same = true;
    for (size_t i = 0; i < nn * 6 && same; i++) same = exact[i] == s->hBoxes[i];
    if (!same) { s->dev.emiState = 0; r->emiSticky = true; }
    s->hBoxes.swap(exact);                           // (also when equal as values: rs_refit_boxes' signs of zero from here on)
    r->boxesExact = true;
}

// The host's tables once the edit has been enqueued: hVertices, hNormals, hBoxes = rs_refit_boxes of the edited vertices, and what of
// `dev` follows from them
void update_host_tables(rs_scene* s, int m, const Records& rec, bool normals) {
    rs_refit* r = s->refit;
    // the edit's dirty box (rs_revalidate_plan.h), while hVertices still holds the old corners
    float dirtyLo[3], dirtyHi[3];
    rs_plan_dirty_box(s->hVertices.data(), m, rec.ids, rec.vertices, true, dirtyLo, dirtyHi);
    for (int j = 0; j < m; j++) {
        std::memcpy(&s->hVertices[(size_t)rec.ids[j] * 9], rec.vertices + (size_t)j * 9, 9 * sizeof(float));
        if (normals) std::memcpy(&s->hNormals[(size_t)rec.ids[j] * 9], rec.normals + (size_t)j * 9, 9 * sizeof(float));
    }
    // The boxes hold exact unions already (before the first edit: make_boxes_exact), so an edit of few triangles recomputes only the moved
    // leaves' ancestors: the same min / max, hence the same bits
    if ((size_t)m * 16 < (size_t)s->numPrims) rs_refit_boxes_host_some(m, rec.ids, s->hVertices.data(), s->hLeafOf.data(), s->hParent.data(), r->hChild.data(), s->hBoxes.data());
    else rs_refit_boxes_host(s->bvhSize, s->hVertices.data(), s->hNodes[0].data(), s->hParent.data(), s->hBoxes.data());
    if (s->dev.axisCull && !far_skip_allowed(rec.vertices, (size_t)m)) s->dev.axisCull = false;      // (never back on: that would need every triangle again)
    if (s->dOccNodes) {
        s->dev.occRootLo = ld3(&s->hBoxes[r->root * 6]);
        s->dev.occRootHi = ld3(&s->hBoxes[r->root * 6 + 3]);
    }
    s->edits++;                                                  // retained G-buffer planes are not this scene's any more
    s->geomEdits++;                                              // ... and cuts of the tree carry boxes the refit has just changed
    rs_dirty_ring_push(s->dirty, s->geomEdits, dirtyLo, dirtyHi);   // ... and shadow segments through this box may have changed their answer
    if (s->dev.prevVertices) s->motionDirty = true;              // rs_scene_advance_motion has something to copy
}

}  // namespace

int rs_set_geometry(rs_scene* s, int count, const int* primIds, const float* vertices, const float* normals, bool emitters, const char* name,
                    const rs_record_source* source, bool* taken) {
    if (taken) *taken = false;
    if (!s) return fail_named(RS_ERR_INVALID_ARGUMENT, name, "null scene");
    rs_geometry_edit_plan plan;
    std::string why;
    if (int e = rs_plan_edit_records(edit_view(s), count, primIds, vertices, normals, emitters, source ? source->numRecs : 0, name, s->editStamps, plan, why)) return refused(e, why);
    RS_TRY(refuse_while_capturing(name));
    if (count == 0) return 0;
    RS_TRY(rs_refit_prepare(s));
    if (s->partialRefit) RS_TRY(rs_refit_prepare_partial(s));       // (the first edit with the switch on: the path's tables)
    const bool lamps = plan.lamps != 0;
    if (lamps) RS_TRY(versions_prepare(s));             // (the ring's slots, hLightArea, the environment entry's power)
    rs_refit* r = s->refit;
    // An emitter moves: the new light sampler and the emissive tree's new grid, built and checked before anything of the scene changes
    rs_edit_lights_plan lights;
    if (lamps) if (int e = rs_plan_edit_lights(edit_view(s), s->editStamps, vertices, name, lights, why)) return refused(e, why);

    // what crosses the bus: the records themselves, or a source's records, which follow the records they expand to in the device buffer
    size_t staged = plan.staged, onDevice = plan.onDevice, stagedAt = 0;
    if (source) { staged = plan.partStaged; onDevice = plan.partOnDevice; stagedAt = plan.bytes; }
    rs_refit::Stage* g = nullptr;
    RS_TRY(stage_reserve(r, staged, onDevice, &g));
    const Records rec = fill_stage(g->host, plan, s->editStamps, count, primIds, vertices, normals, source);

    // frames in flight: a render that has only been recorded is launched now, with the old geometry (and the old lights)
    if (lamps) RS_TRY(version_begin(s));
    else RS_TRY(rs_gbuffer_release_scene(s));
    if (!r->boxesExact) make_boxes_exact(s);
    // The emissive tree's grid moves with the lamps (DevScene travels by value; the fences keep earlier launches on the old tree).  Emitters
    // collapsed to a box without extent: a fresh build has no emissive tree either (the quantiser refuses), so the last bounce asks the
    // scene's trees until an edit brings an extent back -- that edit refits every emissive record, whichever emitters it names.
    const bool emiNodes = lamps && r->emiRecords && lights.emiGrid && !r->emiSticky;
    if (lamps && r->emiRecords && !r->emiSticky) {
        s->dev.emiState = lights.emiGrid ? 1 : 0;
        if (lights.emiGrid) {
            s->dev.emiBase = ld3(lights.emiBase); s->dev.emiScale = ld3(lights.emiScale);
            s->emiMargin = lights.emiMargin;
        }
    }

    const hipStream_t st = rs_stream();
    char* d = r->dStage;
    RS_TRY(fence_before(r->before));
    RS_HIP(hipMemcpyAsync(d + stagedAt, g->host, staged, hipMemcpyHostToDevice, st));
    RS_HIP(hipEventRecord(g->copied, st));
    g->pending = true;
    r->stageNext = (r->stageNext + 1) % rs_refit::kStaging;
    r->stagedBytes = staged;
    if (source) RS_TRY(source->enqueue(*source, d + stagedAt, (size_t)plan.m, reinterpret_cast<int*>(d), reinterpret_cast<float*>(d + plan.offV),
                                       reinterpret_cast<float*>(d + plan.offN), st));
    // whole or partial (rs_geometry_plan.h): the first edit of a scene is whole, since no whole refit has left its key boxes yet
    bool partial = false;
    unsigned long long bound = 0;
    rs_plan_refit(s->partialRefit, s->partialMaxTriangles, r->keysValid, plan.m, r->numTrees, r->treeDepth, r->numNodes, kRefitPartialCapacity, &partial, &bound);
    RS_TRY(rs_refit_enqueue(s, plan.m, reinterpret_cast<const int*>(d), reinterpret_cast<const float*>(d + plan.offV),
                            normals ? reinterpret_cast<const float*>(d + plan.offN) : nullptr, lamps, emiNodes, partial, st));
    RS_TRY(fence_after(r->after));

    update_host_tables(s, plan.m, rec, normals != nullptr);
    if (taken) *taken = true;                           // past the last refusal: the scene holds the new pose whatever the calls below return
    if (!lamps) return rs_after_launch(name);
    // the lights' version: light_records reads the vertices just written; launches from here on see new geometry and new lights alike
    s->hLightArea.swap(lights.area);
    s->hLightProb.swap(lights.prob);
    s->hLightFailId.swap(lights.fail);
    s->sumLightPower = lights.sumAll;
    // moved lamps: this edit's number on every sampler entry it named (rs_restir_set_light_retargeting re-evaluates their samples)
    s->lightMoves++;
    for (int j = 0; j < plan.m; j++) {
        const int light = s->hLightOfPrim[(size_t)rec.ids[j]];
        if (light >= 0) s->hLightMoved[(size_t)light] = (uint32_t)s->lightMoves;
    }
    return version_commit(s, name);
}

extern "C" int rs_scene_set_triangles(rs_scene* s, int count, const int* primIds, const float* vertices, const float* normals) {
    RS_SCOPE(s);
    return rs_set_geometry(s, count, primIds, vertices, normals, false, "rs_scene_set_triangles");
}

extern "C" int rs_scene_set_geometry(rs_scene* s, int count, const int* primIds, const float* vertices, const float* normals) {
    RS_SCOPE(s);
    return rs_set_geometry(s, count, primIds, vertices, normals, true, "rs_scene_set_geometry");
}

extern "C" int rs_scene_light_moves(const rs_scene* s, unsigned long long* moves) {
    if (!s || !moves) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_light_moves: null argument");
    *moves = s->lightMoves;
    return 0;
}

extern "C" int rs_scene_geometry_edits(const rs_scene* s, unsigned long long* count) {
    if (!s || !count) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_geometry_edits: null argument");
    *count = s->geomEdits;
    return 0;
}

// what a frame whose previous frame saw `sinceEdit` edits would take from the ring now (rs_plan_revalidation)
extern "C" int rs_scene_dirty_boxes(const rs_scene* s, unsigned long long sinceEdit, int capacity, float* boxes6, int* count, int* everything) {
    if (!s || !count || !everything || capacity < 0 || (capacity > 0 && !boxes6)) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_dirty_boxes: bad argument");
    rs_revalidate_choice c;
    rs_plan_revalidation(s->dirty.e, s->dirty.count, sinceEdit, s->geomEdits, true, c);
    *count = c.boxes.n; *everything = c.boxes.everything;
    for (int i = 0; i < c.boxes.n && i < capacity; i++)
        for (int k = 0; k < 3; k++) { boxes6[i * 6 + k] = c.boxes.box[i].lo[k]; boxes6[i * 6 + 3 + k] = c.boxes.box[i].hi[k]; }
    return 0;
}

extern "C" int rs_debug_scene_staged_bytes(const rs_scene* s, size_t* bytes) {
    if (!s || !bytes) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_scene_staged_bytes: null argument");
    *bytes = s->refit ? s->refit->stagedBytes : 0;
    return 0;
}

// ---- the partial refit's switch (include/restir_hip.h; rs_geometry_plan.h rs_plan_refit decides per edit) ----
extern "C" int rs_scene_set_partial_refit(rs_scene* s, int on, int maxTriangles) {
    if (!s) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_set_partial_refit: null scene");
    if ((on != 0 && on != 1) || maxTriangles == 0) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_set_partial_refit: on is neither 0 nor 1, or maxTriangles is 0");
    s->partialRefit = on != 0;
    s->partialMaxTriangles = maxTriangles < 0 ? -1 : maxTriangles;
    return 0;
}

extern "C" int rs_scene_get_partial_refit(const rs_scene* s, int* on, int* maxTriangles) {
    if (!s) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_get_partial_refit: null scene");
    if (on) *on = s->partialRefit ? 1 : 0;
    if (maxTriangles) *maxTriangles = s->partialMaxTriangles < 0 ? kRefitPartialDefaultMaxTriangles : s->partialMaxTriangles;
    return 0;
}

extern "C" int rs_scene_refit_counts(const rs_scene* s, unsigned long long* whole, unsigned long long* partial) {
    if (!s) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_refit_counts: null scene");
    if (whole) *whole = s->refit ? s->refit->wholeRefits : 0;
    if (partial) *partial = s->refit ? s->refit->partialRefits : 0;
    return 0;
}

extern "C" int rs_debug_scene_refit_dirty(const rs_scene* s, unsigned long long* nodes) {
    RS_SCOPE(s);
    if (!s || !nodes) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_scene_refit_dirty: null argument");
    RS_TRY(refuse_while_capturing("rs_debug_scene_refit_dirty"));
    RS_TRY(rs_synchronize());
    *nodes = 0;
    if (!s->refit || !s->refit->lastPartial) return 0;
    unsigned dirty = 0;
    RS_HIP(hipMemcpy(&dirty, s->refit->dDirty, sizeof(unsigned), hipMemcpyDeviceToHost));
    *nodes = dirty;
    return 0;
}

extern "C" int rs_debug_plan_refit(int on, int maxTriangles, int keysValid, int m, int numTrees, const int* treeDepth, unsigned long long numNodes,
                                   unsigned long long capacity, int* partial, unsigned long long* bound) {
    if (m < 0 || numTrees < 0 || (numTrees > 0 && !treeDepth) || !partial || !bound) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_plan_refit: null or negative argument");
    bool p = false;
    rs_plan_refit(on != 0, maxTriangles, keysValid != 0, m, numTrees, treeDepth, numNodes, capacity, &p, bound);
    *partial = p ? 1 : 0;
    return 0;
}

// Test hook of rs_geometry_plan.h (include/restir_hip.h): the two plans rs_set_geometry asks for, of a view the caller made up
static_assert(sizeof(rs_geometry_edit_view) == 120 && sizeof(rs_geometry_edit_plan) == 64 && sizeof(rs_geometry_edit_lights) == 64, "the sizes restir_amd/ctypes_structs.py mirrors");
extern "C" int rs_debug_plan_geometry_edit(const rs_geometry_edit_view* view, const char* name, int emitters, int count, const int* primIds,
                                           const float* vertices, const float* normals, int numPartRecs, rs_geometry_edit_plan* plan, int* slots,
                                           rs_geometry_edit_lights* lights, float* area, float* prob, int* failId) {
    if (!view || !name || !plan || numPartRecs < 0) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_plan_geometry_edit: null argument");
    rs_edit_stamps stamps;
    std::string why;
    if (int e = rs_plan_edit_records(*view, count, primIds, vertices, normals, emitters != 0, numPartRecs, name, stamps, *plan, why)) return refused(e, why);
    for (int i = 0; slots && i < count; i++) slots[i] = stamps.lastIndex[(size_t)primIds[i]];
    if (!plan->lamps || !lights) return 0;
    rs_edit_lights_plan l;
    if (int e = rs_plan_edit_lights(*view, stamps, vertices, name, l, why)) return refused(e, why);
    lights->sumAll = l.sumAll; lights->emiGrid = l.emiGrid ? 1 : 0; lights->emiMargin = l.emiMargin;
    for (int k = 0; k < 3; k++) { lights->emiLo[k] = l.emiLo[k]; lights->emiHi[k] = l.emiHi[k]; lights->emiBase[k] = l.emiBase[k]; lights->emiScale[k] = l.emiScale[k]; }
    if (area) std::copy(l.area.begin(), l.area.end(), area);
    if (prob) std::copy(l.prob.begin(), l.prob.end(), prob);
    if (failId) std::copy(l.fail.begin(), l.fail.end(), failId);
    return 0;
}

// ---- motion tracking: the previous pose of the scene (include/restir_hip.h) ----
namespace {

// prevVertices = vertices, for every launch enqueued after this call.  Launches already handed to an auxiliary stream may read prevVertices
// (a render that was deferred to it), so the copy sits behind the fences of a geometry edit (fence_before / fence_after).  A render that has only been recorded was launched before (rs_gbuffer_release_scene).
int motion_copy(rs_scene* s, const char* name) {
    RS_TRY(fence_before(s->motionBefore));
    RS_TRY(rs_motion_copy_enqueue(s->dVertices, s->dPrevVertices, (size_t)s->numPrims, rs_stream()));
    RS_TRY(fence_after(s->motionAfter));
    s->motionDirty = false;
    return rs_after_launch(name);
}

}  // namespace

extern "C" int rs_scene_set_motion_tracking(rs_scene* s, int on) {
    RS_SCOPE(s);
    if (!s) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_set_motion_tracking: null scene");
    RS_TRY(refuse_while_capturing("rs_scene_set_motion_tracking"));
    const bool tracked = s->dev.prevVertices != nullptr;
    if ((on != 0) == tracked) return 0;
    if (on && !s->dPrevVertices) {
        // everything that can fail comes first: a failure leaves the scene untracked and unchanged
        int e = rs_dev_alloc(&s->dPrevVertices, (size_t)s->numPrims * 9);
        for (hipEvent_t& ev : s->motionBefore) if (!e) e = rs_check_hip(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate");
        if (!e) e = rs_check_hip(hipEventCreateWithFlags(&s->motionAfter, hipEventDisableTiming), "hipEventCreate");
        if (e) { motion_free(s); return e; }
    }
    // a render that has only been recorded captures `dev` when it is launched: launch it now, in the form it was requested in
    RS_TRY(rs_gbuffer_release_scene(s));
    if (on) {
        RS_TRY(motion_copy(s, "rs_scene_set_motion_tracking"));      // previous pose = current pose: the motion plane of an untracked scene
        s->dev.prevVertices = s->dPrevVertices;
        return 0;
    }
    s->dev.prevVertices = nullptr;
    if (s->motionDirty) s->edits++;                     // the previous pose differed: the camera-only plane is not the retained one
    s->motionDirty = false;
    return 0;
}

extern "C" int rs_scene_advance_motion(rs_scene* s) {
    RS_SCOPE(s);
    if (!s) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_advance_motion: null scene");
    RS_TRY(refuse_while_capturing("rs_scene_advance_motion"));
    // untracked: nothing to do.  No accepted geometry edit since the last advance: prevVertices equals the vertices already, nothing is
    // enqueued and retained G-buffer planes stay this scene's
    if (!s->dev.prevVertices || !s->motionDirty) return 0;
    RS_TRY(rs_gbuffer_release_scene(s));                // with the old previous pose
    RS_TRY(motion_copy(s, "rs_scene_advance_motion"));
    s->edits++;                                         // the motion plane of the frame after a move is not the one of the frame of the move
    return 0;
}

extern "C" int rs_scene_download_prev_vertices(const rs_scene* s, float* out) {
    RS_SCOPE(s);
    if (!s || !out) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_download_prev_vertices: null argument");
    if (!s->dev.prevVertices) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_scene_download_prev_vertices: the scene does not track motion (rs_scene_set_motion_tracking)");
    RS_TRY(refuse_while_capturing("rs_scene_download_prev_vertices"));
    RS_TRY(rs_synchronize());
    RS_HIP(hipMemcpy(out, s->dPrevVertices, (size_t)s->numPrims * 9 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
