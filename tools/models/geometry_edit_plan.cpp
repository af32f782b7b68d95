// tools/models/geometry_edit_plan.cpp -- the two plan functions of a geometry edit (restir_amd/csrc/rs_geometry_plan.h) on their edge cases,
// as a stand-alone host program for AddressSanitizer + UBSan: no device is touched, and the plan needs of the library only its alias
// table and its grid (scene_build.cpp, occlusion_bvh.cpp).  From restir_amd/csrc:
//   for f in ../../tools/models/geometry_edit_plan.cpp scene_build.cpp occlusion_bvh.cpp; do
//     hipcc -O1 -g -std=c++17 -ffp-contract=off -x hip --offload-arch=gfx950 --cuda-host-only -Xarch_host -fsanitize=address,undefined \
//           -Xarch_host -fno-omit-frame-pointer -I. -c $f -o /tmp/gep_$(basename $f).o; done
//   hipcc -fsanitize=address,undefined /tmp/gep_*.o -o /tmp/geometry_edit_plan        (host objects only: the sanitizers never see device code)
//   /tmp/geometry_edit_plan        (prints "geometry_edit_plan: ok"; a failed check or a sanitizer report ends it with a non-zero status)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "rs_geometry_plan.h"

// the one library service the two sources use besides each other
static std::string g_err;
int rs_fail(int code, const char* msg) { g_err = msg ? msg : ""; return code; }

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "geometry_edit_plan.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

namespace {

constexpr int kPrims = 12, kLamp0 = 10, kLamp1 = 11;

struct Scene {
    std::vector<float> vertices, lightArea, radiance;
    std::vector<int> materialIds, lightPrims, emiLeaf;
    std::vector<rs_material> materials;
    rs_geometry_edit_view view{};
    Scene(bool bounded, bool env, bool tree) {
        materials.resize(2);
        materials[0].type = 0; materials[1].type = 4;
        for (int p = 0; p < kPrims; p++) {
            materialIds.push_back(p >= kLamp0 ? 1 : 0);
            for (int k = 0; k < 9; k++) vertices.push_back(-0.9f + 0.15f * (float)((p * 9 + k * 7) % 13));
        }
        lightPrims = { kLamp0, kLamp1 };
        emiLeaf = { kLamp1, kLamp0 };
        radiance = { 10.f, 10.f, 10.f, 4.f, 2.f, 1.f };
        for (int p : lightPrims) lightArea.push_back(triangle_area(&vertices[(size_t)p * 9]));
        view.numPrims = kPrims; view.materialIds = materialIds.data(); view.materials = materials.data();
        view.bounded = bounded;
        for (int k = 0; k < 3; k++) { view.gridLo[k] = -1.f; view.gridHi[k] = 1.f; }
        view.vertices = vertices.data();
        view.numLightPrims = 2; view.numLights = env ? 3 : 2;
        view.lightPrimIds = lightPrims.data(); view.lightRadiance = radiance.data(); view.lightArea = lightArea.data();
        view.envPower = env ? 2.5f : 0.f;
        view.emissiveTree = tree; view.numEmissive = 2; view.emiLeafPrims = emiLeaf.data();
    }
};

struct Edit {
    std::vector<int> ids;
    std::vector<float> v, n;
    void add(const Scene& s, int p, float scale = 1.f) {
        ids.push_back(p);
        for (int k = 0; k < 9; k++) { v.push_back(s.vertices[(size_t)p * 9 + k] * scale); n.push_back(k % 3 == 1 ? 1.f : 0.f); }
    }
};

int plan(const Scene& s, const Edit& e, bool normals, bool emitters, int partRecs, rs_edit_stamps& st, rs_geometry_edit_plan& p, std::string& why) {
    why.clear();
    return rs_plan_edit_records(s.view, (int)e.ids.size(), e.ids.data(), e.v.data(), normals ? e.n.data() : nullptr, emitters, partRecs, "model", st, p, why);
}

}  // namespace

int main() {
    rs_edit_stamps st;
    rs_geometry_edit_plan p;
    std::string why;
    const Scene s(true, false, true);

    {   // a repeated id, ids out of order, the staged records in their slots
        Edit e; e.add(s, 7); e.add(s, 3); e.add(s, 7, .5f); e.add(s, 9); e.add(s, 3, .25f);
        CHECK(plan(s, e, true, false, 0, st, p, why) == 0 && p.m == 3 && !p.lamps);
        CHECK(p.offV == 16 && p.offN == 16 + 112 && p.bytes == 16 + 2 * 112 && p.staged == p.bytes && p.onDevice == p.bytes);
        std::vector<char> stage(p.bytes);
        rs_fill_edit_records(p, st, (int)e.ids.size(), e.ids.data(), e.v.data(), e.n.data(), stage.data());
        const int* ids = reinterpret_cast<const int*>(stage.data());
        const float* v = reinterpret_cast<const float*>(stage.data() + p.offV);
        CHECK(ids[0] == 7 && ids[1] == 3 && ids[2] == 9);
        CHECK(v[0] == s.vertices[7 * 9] * .5f && v[9] == s.vertices[3 * 9] * .25f && v[18] == s.vertices[9 * 9]);
    }
    {   // one record, no records, no normals, part records
        Edit e; e.add(s, 5);
        CHECK(plan(s, e, false, false, 0, st, p, why) == 0 && p.m == 1 && p.offV == 16 && p.offN == 16 + 48 && p.bytes == p.offN);
        CHECK(plan(s, e, true, true, 3, st, p, why) == 0 && p.partStaged == 3 * sizeof(rs::PartRec) && p.partOnDevice == p.bytes + p.partStaged);
        std::vector<char> stage(p.bytes);
        rs_fill_edit_records(p, st, 1, e.ids.data(), e.v.data(), e.n.data(), stage.data());
        CHECK(plan(s, Edit(), true, true, 0, st, p, why) == 0 && p.m == 0 && p.bytes == 0);
        CHECK(rs_plan_edit_records(s.view, -1, nullptr, nullptr, nullptr, true, 0, "model", st, p, why) == RS_ERR_INVALID_ARGUMENT && why == "model: count < 0 or null arrays");
        CHECK(rs_plan_edit_records(s.view, 1, e.ids.data(), nullptr, nullptr, true, 0, "model", st, p, why) == RS_ERR_INVALID_ARGUMENT);
    }
    {   // ids out of range, values that are not finite, the grid's box
        Edit e; e.add(s, 0); e.add(s, 1);
        e.ids[1] = -1;     CHECK(plan(s, e, true, false, 0, st, p, why) == RS_ERR_INVALID_ARGUMENT && why == "model: a primitive id out of range");
        e.ids[1] = kPrims; CHECK(plan(s, e, true, false, 0, st, p, why) == RS_ERR_INVALID_ARGUMENT);
        e.ids[1] = std::numeric_limits<int>::max(); CHECK(plan(s, e, true, false, 0, st, p, why) == RS_ERR_INVALID_ARGUMENT);
        e.ids[1] = std::numeric_limits<int>::min(); CHECK(plan(s, e, true, false, 0, st, p, why) == RS_ERR_INVALID_ARGUMENT);
        e.ids[1] = 1;
        Edit bad = e; bad.v[17] = NAN;       CHECK(plan(s, bad, true, false, 0, st, p, why) == RS_ERR_INVALID_ARGUMENT && why == "model: a vertex or normal that is not finite");
        bad = e; bad.n[4] = INFINITY;        CHECK(plan(s, bad, true, false, 0, st, p, why) == RS_ERR_INVALID_ARGUMENT);
                                             CHECK(plan(s, bad, false, false, 0, st, p, why) == 0);       // (the normals are not read)
        bad = e; bad.v[5] = std::nextafter(1.f, 2.f);
        CHECK(plan(s, bad, true, false, 0, st, p, why) == RS_ERR_INVALID_ARGUMENT && why.find("outside the root box") != std::string::npos);
        CHECK(plan(Scene(false, false, true), bad, true, false, 0, st, p, why) == 0);
        bad = e; bad.v[0] = -1.f; bad.v[16] = 1.f;
        CHECK(plan(s, bad, true, false, 0, st, p, why) == 0);
    }
    {   // emitters: refused, taken; moved, collapsed, without power; with an environment map; without the tree
        Edit e; e.add(s, 2); e.add(s, kLamp0, .5f); e.add(s, kLamp0, .75f);
        CHECK(plan(s, e, true, false, 0, st, p, why) == RS_ERR_INVALID_ARGUMENT && why.find("a Light") != std::string::npos);
        CHECK(plan(s, e, true, true, 0, st, p, why) == 0 && p.lamps && p.m == 2);
        rs_edit_lights_plan l;
        CHECK(rs_plan_edit_lights(s.view, st, e.v.data(), "model", l, why) == 0);
        CHECK(l.area.size() == 2 && l.prob.size() == 2 && l.fail.size() == 2 && l.sumAll > 0.f && l.emiGrid);
        CHECK(l.area[0] == triangle_area(&e.v[18]) && l.area[1] == s.lightArea[1]);
        for (int k = 0; k < 3; k++) CHECK(l.emiLo[k] <= l.emiHi[k] && l.emiLo[k] >= -1.f && l.emiHi[k] <= 1.f);

        Edit c;                                                      // every emitter in one point
        c.add(s, kLamp0, 0.f); c.add(s, kLamp1, 0.f);
        CHECK(plan(s, c, true, true, 0, st, p, why) == 0 && p.lamps);
        why.clear();
        CHECK(rs_plan_edit_lights(s.view, st, c.v.data(), "model", l, why) == RS_ERR_INVALID_ARGUMENT);
        CHECK(why == "model: the edit leaves the light sampler without a finite, positive total power");
        const Scene env(true, true, true);
        CHECK(plan(env, c, true, true, 0, st, p, why) == 0);
        CHECK(rs_plan_edit_lights(env.view, st, c.v.data(), "model", l, why) == 0 && !l.emiGrid && l.sumAll == 2.5f && l.prob.size() == 3);
        const Scene bare(true, true, false);
        CHECK(plan(bare, e, true, true, 0, st, p, why) == 0);
        CHECK(rs_plan_edit_lights(bare.view, st, e.v.data(), "model", l, why) == 0 && !l.emiGrid);
    }
    {   // the stamp wraps: the marks of 2^32 - 1 edits ago must not be taken for this edit's
        Edit e; e.add(s, 4);
        st.stamp = 0xfffffffeu;
        CHECK(plan(s, e, true, false, 0, st, p, why) == 0 && st.stamp == 0xffffffffu && st.named(4));
        Edit f; f.add(s, 6);
        CHECK(plan(s, f, true, false, 0, st, p, why) == 0 && st.stamp == 1u && st.named(6) && !st.named(4));
    }
    std::printf("geometry_edit_plan: ok\n");
    return 0;
}
