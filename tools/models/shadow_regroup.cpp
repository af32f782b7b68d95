// CPU model of the shadow rays' walk per block of the shadow-ray kernel, with and without regrouping the block's segments by length
// before the walk (restir_amd/csrc/rs_shadow_regroup.h, restir.hip k_shadow_regroup), on the benchmark camera at 1920x1080.
// Built on the product's host code: rs_build_bvh, rs_reference_chain_tables and rs_build_occlusion_bvh over the reference's leaf boxes,
// the 16-byte grid records of rs_quantize_occlusion_bvh (decoded back to planes base + q * scale: the boxes the device tests),
// camera_sample, rs_build_light_table, rs_build_alias_table, shadow_bin and rs_plan_shadow_slots.  The light sample is the host form of
// rs_surface.h sample_light_with (a device function): the same alias look-up, uniform triangle sample, single-sided test and pdf, with
// the compiler's division and root instead of rs_exact.h's -- statistics, not bits.
// Per pixel of a block: a jittered primary ray through the reference's threaded tree, a 32-candidate RIS (Lambertian target with base
// colour 1, as the DI path evaluates it: luminance(Li) * cos / pi / pdf), the winner's segment through the shadow tree with the relaxed
// grid test and `limit`, ending at the first leaf that holds a hit.  Simplifications: leaves are tested where they are met (the device
// queues up to four and so walks a few nodes past a hit), no chain check, no special-case rays, every surface Lambertian.
// Per block it prints the wave iterations (the sum over waves of the longest walk in the wave) for
//   today      wave w holds the 8x8 tile w
//   binned     slot = first[bin] + arrival rank in lane order (rs_plan_shadow_slots), wave w holds slots 64 w ..
//   bound      the rays sorted by their true step count
// for 256-thread blocks (32x8 pixels) and 512-thread blocks (32x16), drawn as random 32x16 super-blocks.
// Build (from restir_amd/csrc, after `make`):
//   hipcc -O2 -std=c++17 -ffp-contract=off -I. -x hip --offload-arch=gfx950 -c ../../tools/models/shadow_regroup.cpp -o /tmp/sr.o
//   hipcc /tmp/sr.o -L.. -lrestir_hip -Wl,-rpath,$PWD/.. -o /tmp/sr && /tmp/sr v.bin m.bin mat.bin [super-blocks] [bistro]
//   (host functions of the library only; no device is touched)
// v.bin, m.bin, mat.bin: sd = scenes.sponza_class(1, 1.0) (`bistro`: bistro_class(2, 1.0) and its camera);
//   sd.vertices.tofile("v.bin"); sd.material_ids.tofile("m.bin"); sd.materials.tofile("mat.bin")
#include "rs_internal.h"
#include "rs_shadow_regroup.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
using namespace rs;

static std::vector<char> slurp(const char* path) {
    std::vector<char> d;
    FILE* f = fopen(path, "rb"); if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(1); }
    fseek(f, 0, SEEK_END); d.resize((size_t)ftell(f)); fseek(f, 0, SEEK_SET);
    if (fread(d.data(), 1, d.size(), f) != d.size()) exit(1);
    fclose(f);
    return d;
}

int main(int argc, char** argv) {
    if (argc < 4) return 1;
    const std::vector<char> vb = slurp(argv[1]), mb = slurp(argv[2]), matb = slurp(argv[3]);
    const int np = (int)(vb.size() / 36), nmat = (int)(matb.size() / sizeof(rs_material));
    const float* v = reinterpret_cast<const float*>(vb.data());
    const int* matId = reinterpret_cast<const int*>(mb.data());
    const rs_material* mats = reinterpret_cast<const rs_material*>(matb.data());
    if ((int)(mb.size() / 4) != np || nmat <= 0) return 1;
    const int supers = argc > 4 ? atoi(argv[4]) : 300;
    const bool bistro = argc > 5 && !strcmp(argv[5], "bistro");
    // the reference's tree, its leaf boxes, the shadow tree over them and its grid records
    const size_t nn = 2 * (size_t)np - 1;
    std::vector<float> boxes(nn * 6); std::vector<int> nodes[6]; int* ptr[6];
    for (int k = 0; k < 6; k++) { nodes[k].resize(nn * 3); ptr[k] = nodes[k].data(); }
    int bvhSize = 0; if (rs_build_bvh(np, v, boxes.data(), ptr, &bvhSize)) return 1;
    std::vector<int> parent, leafOf;
    if (rs_reference_chain_tables(bvhSize, nodes[0].data(), parent, leafOf, np)) return 1;
    std::vector<float> primBoxes((size_t)np * 6);
    for (int p = 0; p < np; p++) memcpy(&primBoxes[(size_t)p * 6], &boxes[(size_t)leafOf[(size_t)p] * 6], 24);
    std::vector<BvhNode> occ; std::vector<int> leafPrims;
    if (rs_build_occlusion_bvh(np, primBoxes.data(), occ, leafPrims)) return 1;
    float base[3], scale[3]; std::vector<unsigned> packed;
    if (rs_quantize_occlusion_bvh(occ, base, scale, packed)) return 1;
    const unsigned occEnd = (unsigned)occ.size() * 16u;
    int root = 0; for (int i = 0; i < bvhSize; i++) if (parent[(size_t)i] < 0) root = i;
    const float binsOverExtent = shadow_bins_over_extent(&boxes[(size_t)root * 6], &boxes[(size_t)root * 6 + 3]);
    // lights
    std::vector<int> lightPrim((size_t)np); std::vector<float> lightLe((size_t)np * 3), lightPower((size_t)np);
    int nl = 0; if (rs_build_light_table(np, v, matId, nmat, mats, &nl, lightPrim.data(), lightLe.data(), lightPower.data()) || nl == 0) return 1;
    std::vector<float> prob((size_t)nl); std::vector<int> fail((size_t)nl); float sumPower = 0.f;
    if (rs_build_alias_table(nl, lightPower.data(), prob.data(), fail.data(), &sumPower)) return 1;
    std::vector<char> isLight((size_t)np, 0); for (int i = 0; i < nl; i++) isLight[(size_t)lightPrim[(size_t)i]] = 1;
    // the benchmark camera
    rs_camera cam; memset(&cam, 0, sizeof cam); const int W = 1920, H = 1080;
    cam.resolution[0] = W; cam.resolution[1] = H;
    if (bistro) { cam.position[0] = .3f; cam.position[1] = 1.8f; cam.position[2] = 55.f; cam.rotation[0] = -91.f; cam.rotation[1] = 1.f; }
    else { cam.position[0] = .5f; cam.position[1] = 2.2f; cam.position[2] = 17.f; cam.rotation[0] = -92.f; cam.rotation[1] = -2.f; }
    cam.fov[1] = 30.f; cam.fov[0] = 30.f * W / H; cam.focalDist = 1.f;
    rs_camera_update(&cam); cam.tanFovY = tanf(radians(cam.fov[1]));
    const CamParams cp = rs_make_cam_params(&cam);
    std::mt19937 g(1);
    auto uni = [&]() { return (float)(g() >> 8) * (1.f / 16777216.f); };
    auto tri = [&](const Ray& ray, int p, float& d) { float bx, by; const float* t = v + (size_t)p * 9; const f3 v0 = ld3(t);
        return tri_hit(ray.o, ray.d, v0, ld3(t + 3) - v0, ld3(t + 6) - v0, bx, by, d); };
    // the reference's closest-hit walk
    auto closest = [&](const Ray& ray, float& dist) {
        const RayBoxCtx ctx = make_box_ctx(ray); const int* nd = nodes[mtbvh_order(-ray.d)].data();
        int prim = -1; dist = 3.402823466e+38f;
        for (int cur = 0; cur != bvhSize;) { const int* n = nd + (size_t)cur * 3; const float* b = &boxes[(size_t)n[1] * 6]; float tb;
            if (box_hit(ctx, ld3(b), ld3(b + 3), tb) && tb < dist) { float d; if (n[0] >= 0 && tri(ray, n[0], d) && d < dist) { dist = d; prim = n[0]; } cur++; }
            else cur = n[2]; }
        return prim;
    };
    // node steps of a segment's any-hit walk through the grid records; *occluded: it ended on a hit
    auto shadow_steps = [&](f3 pos, f3 wi, float dist, bool* occluded) {
        Ray ray; ray.o = pos + wi * 1e-5f; ray.d = wi;
        const float limit = dist - 1e-4f * 2.f;
        const float o[3] = { ray.o.x, ray.o.y, ray.o.z }, d[3] = { wi.x, wi.y, wi.z };
        int steps = 0; *occluded = false;
        for (unsigned cur = 0; cur != occEnd;) {
            const unsigned* n = &packed[cur / 4]; steps++;
            const unsigned q[6] = { n[0] & 0xffffu, n[0] >> 16, n[1] & 0xffffu, n[1] >> 16, n[2] & 0xffffu, n[2] >> 16 };      // lo.x lo.y lo.z hi.x hi.y hi.z
            float tMin = -3.402823466e+38f, tMax = 3.402823466e+38f;
            for (int a = 0; a < 3; a++) { const float inv = 1.f / d[a], t0 = ((base[a] + (float)q[a] * scale[a]) - o[a]) * inv, t1 = ((base[a] + (float)q[3 + a] * scale[a]) - o[a]) * inv;
                tMin = fmaxf(tMin, fminf(t0, t1)); tMax = fminf(tMax, fmaxf(t0, t1)); }
            const bool pass = tMax >= fmaxf(tMin, 0.f) && tMin < limit;
            const int meta = (int)n[3];
            if (meta < 0) {
                if (pass) { const int code = ~meta; for (int i = 0; i < (code & 7); i++) { float td; if (tri(ray, leafPrims[(size_t)((code >> 3) + i)], td) && td < limit) { *occluded = true; return steps; } } }
                cur += 16u;
            }
            else cur = pass ? cur + 16u : (unsigned)meta;
        }
        return steps;
    };
    struct Seg { int steps, bin; };                     // steps < 0: the lane has no segment
    auto pixel = [&](int x, int y, long& shaded, long& noWinner, long& occludedRays) {
        Seg s{ -1, 0 };
        float dist; const Ray ray = camera_sample(cp, x, y, uni(), uni());
        const int prim = closest(ray, dist);
        if (prim < 0 || isLight[(size_t)prim]) return s;
        shaded++;
        const float* t = v + (size_t)prim * 9;
        f3 nrm = normalize(cross(ld3(t + 3) - ld3(t), ld3(t + 6) - ld3(t)));
        if (dot(nrm, ray.d) > 0.f) nrm = nrm * -1.f;
        const f3 pos = ray.o + ray.d * dist;
        float sum = 0.f, wDist = 0.f; f3 wWi = splat(0.f);
        for (int c = 0; c < 32; c++) {
            const float r0 = uni(), r1 = uni(), r2 = uni(), r3 = uni(), pick = uni();
            const int pass = std::min((int)((float)nl * r0), nl - 1), id = r1 < prob[(size_t)pass] ? pass : fail[(size_t)pass];
            const float* lt = v + (size_t)lightPrim[(size_t)id] * 9;
            const f3 v0 = ld3(lt), v1 = ld3(lt + 3), v2 = ld3(lt + 6), cr = cross(v1 - v0, v2 - v0);
            const float area = length(cr) * .5f; const f3 ln = normalize(cr);
            const float sr = sqrtf(r3), u = 1.f - sr, vv = r2 * sr;
            const f3 toS = v1 * u + v2 * vv + v0 * (1.f - u - vv) - pos;
            if (dot(ln, toS) > -1e-6f) continue;                               // SCENE_LIGHT_SINGLE_SIDED
            const float dd = dot(toS, toS), len = sqrtf(dd); const f3 wi = toS * (1.f / len);
            const float pdf = (lightPower[(size_t)id] / sumPower / area) * dd / fabsf(dot(ln, wi));
            const float cosS = dot(nrm, wi);
            const float w = cosS > 0.f && pdf > 0.f ? luminance(ld3(&lightLe[(size_t)id * 3])) * cosS * (1.f / kPi) / pdf : 0.f;
            if (!(w > 0.f)) continue;
            sum += w;
            if (pick * sum < w) { wWi = wi; wDist = len; }
        }
        if (!(sum > 0.f)) { noWinner++; return s; }
        bool occl; s.steps = shadow_steps(pos, wWi, wDist, &occl); s.bin = shadow_bin(wDist, binsOverExtent);
        occludedRays += occl;
        return s;
    };
    // wave iterations of `n` lanes' rays handed out to waves of 64 by `slotOf` (lanes without a ray have none)
    auto waves_sum = [](const std::vector<int>& stepsBySlot) { long it = 0;
        for (size_t w = 0; w < stepsBySlot.size(); w += 64) { int m = 0; for (size_t i = w; i < std::min(w + 64, stepsBySlot.size()); i++) m = std::max(m, stepsBySlot[i]); it += m; }
        return it; };
    auto three = [&](const Seg* lanes, int n, long out[3]) {            // lanes in thread order (wave-major: tile by tile)
        std::vector<int> today((size_t)n, 0), bins((size_t)n), first(kShadowBins), binned, bound;
        for (int i = 0; i < n; i++) { today[(size_t)i] = std::max(lanes[i].steps, 0); bins[(size_t)i] = lanes[i].steps >= 0 ? lanes[i].bin : -1; }
        out[0] += waves_sum(today);
        int hist[kShadowBins] = {}, at = 0;
        for (int i = 0; i < n; i++) if (bins[(size_t)i] >= 0) hist[bins[(size_t)i]]++;
        for (int b = kShadowBins - 1; b >= 0; b--) { first[(size_t)b] = at; at += hist[b]; }
        if (n == kShadowRegroupRays) { int f2[kShadowBins]; if (rs_plan_shadow_slots(bins.data(), n, f2) != at || memcmp(f2, first.data(), sizeof f2)) { fprintf(stderr, "slot plan differs\n"); exit(1); } }
        binned.assign((size_t)at, 0);
        for (int i = 0; i < n; i++) if (bins[(size_t)i] >= 0) binned[(size_t)first[(size_t)bins[(size_t)i]]++] = lanes[i].steps;
        out[1] += waves_sum(binned);
        bound = binned; std::sort(bound.begin(), bound.end(), [](int a, int b) { return a > b; });
        out[2] += waves_sum(bound);
    };
    long shaded = 0, noWinner = 0, occl = 0, rays = 0, steps = 0, b256[3] = { 0, 0, 0 }, b512[3] = { 0, 0, 0 };
    for (int s = 0; s < supers; s++) {
        const int X = (int)(g() % (W / 32)) * 32, Y = (int)(g() % (H / 16)) * 16;
        Seg lanes[512];                                 // wave-major: wave w = tile (w & 3, w >> 2), lane = 8 * row + column
        for (int w = 0; w < 8; w++) for (int l = 0; l < 64; l++)
            lanes[w * 64 + l] = pixel(X + (w & 3) * 8 + (l & 7), Y + (w >> 2) * 8 + (l >> 3), shaded, noWinner, occl);
        for (const Seg& q : lanes) if (q.steps >= 0) { rays++; steps += q.steps; }
        three(lanes, 256, b256); three(lanes + 256, 256, b256);
        three(lanes, 512, b512);
    }
    printf("%s: %d triangles, %d lights, %d super-blocks of 32x16 pixels: %ld shaded pixels, %ld without a RIS winner (%.1f %%), %ld segments, %.1f %% occluded\n",
           bistro ? "bistro-class" : "sponza-class", np, nl, supers, shaded, noWinner, 100.0 * noWinner / std::max(shaded, 1l), rays, 100.0 * occl / std::max(rays, 1l));
    printf("steps per ray %.1f; lane use today %.1f %% (ray steps / (64 x wave iterations))\n", (double)steps / rays, 100.0 * steps / (64.0 * b256[0]));
    const char* names[3] = { "today (one tile per wave)", "binned by segment length", "by true step count (bound)" };
    for (int k = 0; k < 3; k++)
        printf("%-28s 256 threads: %7.1f wave iterations per block (%+5.1f %%)   512 threads: %7.1f (%+5.1f %%)\n", names[k],
               (double)b256[k] / (2 * supers), 100.0 * (b256[k] - b256[0]) / b256[0], (double)b512[k] / supers, 100.0 * (b512[k] - b512[0]) / b512[0]);
    return 0;
}
