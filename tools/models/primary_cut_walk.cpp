// CPU model of the primary rays' packet walk with and without a static per-cell cut of the tree (restir_amd/csrc/rs_cuts.h), on the
// benchmark camera at 1920x1080.  Per 8x8 tile it takes the UNION of the nodes its 64 jittered rays visit in the reference's walk -- what
// the wave-cooperative walk pays per tile (rs_walk.h trace_closest_packet) -- and splits it into
//   entered       some lane enters the node (box test passed with tMin < closest)
//   distance      some lane passes the geometric part of the box test, none enters: rejected on distance alone
//   geometric     NO lane passes the geometric part: what the camera and the box decide, the same in every frame of a still camera
// then asks what is left of the union when the walk goes through the cut of the tile's cell, for cells of 32x8, 64x8 and 32x16 pixels
// (cut_cell / cut_cell_test of rs_cuts.h, the very functions the device builder runs), and what SEEDING `closest` with the G-buffer ray's
// triangle (the pixel-centre ray's hit, tested first) would save instead.  Containment is checked on every ray: a node a ray passes
// geometrically must be in its cell's cut.  Cells are drawn as random 64x16 super-cells (2 x 2 cells of 32x8, 8 tiles).
// Build (from restir_amd/csrc, after `make`):
//   hipcc -O2 -std=c++17 -ffp-contract=off -I. -x hip --offload-arch=gfx950 -c ../../tools/models/primary_cut_walk.cpp -o /tmp/pc.o
//   hipcc /tmp/pc.o scene_build.o occlusion_bvh.o api_common.o -o /tmp/pc && /tmp/pc vertices.bin [super-cells] [bistro]
// vertices.bin: the scene's float32 vertices (scenes.sponza_class(1, 1.0).vertices.tofile(...); `bistro`: bistro_class(2, 1.0) and its camera)
#include "rs_internal.h"
#include "rs_cuts.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
using namespace rs;

int main(int argc, char** argv) {
    if (argc < 2) return 1;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 1; fseek(f, 0, SEEK_END); const long bytes = ftell(f); const int np = (int)(bytes / 36); fseek(f, 0, SEEK_SET);
    std::vector<float> v((size_t)np * 9); if (fread(v.data(), 36, np, f) != (size_t)np) return 1; fclose(f);
    const int supers = argc > 2 ? atoi(argv[2]) : 40;
    const bool bistro = argc > 3 && !strcmp(argv[3], "bistro");
    const size_t nn = 2 * (size_t)np - 1;
    std::vector<float> boxes(nn * 6); std::vector<int> nodes[6]; int* ptr[6];
    for (int k = 0; k < 6; k++) { nodes[k].resize(nn * 3); ptr[k] = nodes[k].data(); }
    int bvhSize = 0; rs_build_bvh(np, v.data(), boxes.data(), ptr, &bvhSize);
    std::vector<TriRec> tr(np);
    for (int i = 0; i < np; i++) { const float* t = &v[(size_t)i * 9]; f3 v0 = ld3(t), e1 = ld3(t + 3) - v0, e2 = ld3(t + 6) - v0; tr[i] = TriRec{ v0.x, v0.y, v0.z, 0, e1.x, e1.y, e1.z, 0, e2.x, e2.y, e2.z, 0 }; }
    auto record = [&](int k, int i) { const int* n = &nodes[k][(size_t)i * 3]; const float* b = &boxes[(size_t)n[1] * 6]; return BvhNode{ b[0], b[1], b[2], b[5], b[3], b[4], n[0], n[2] }; };
    rs_camera cam; memset(&cam, 0, sizeof cam); const int W = 1920, H = 1080;
    cam.resolution[0] = W; cam.resolution[1] = H;
    if (bistro) { cam.position[0] = .3f; cam.position[1] = 1.8f; cam.position[2] = 55.f; cam.rotation[0] = -91.f; cam.rotation[1] = 1.f; }
    else { cam.position[0] = .5f; cam.position[1] = 2.2f; cam.position[2] = 17.f; cam.rotation[0] = -92.f; cam.rotation[1] = -2.f; }
    cam.fov[1] = 30.f; cam.fov[0] = 30.f * W / H; cam.focalDist = 1.f;
    rs_camera_update(&cam); cam.tanFovY = tanf(radians(cam.fov[1]));
    const CamParams cp = rs_make_cam_params(&cam);
    std::mt19937 g(1);
    auto uni = [&]() { return (float)(g() >> 8) * (1.f / 16777216.f); };
    auto tri = [&](const Ray& ray, int p, float& d) { float bx, by; const TriRec& t = tr[p];
        return tri_hit(ray.o, ray.d, mk3(t.v0x, t.v0y, t.v0z), mk3(t.e1x, t.e1y, t.e1z), mk3(t.e2x, t.e2y, t.e2z), bx, by, d); };
    // the reference's walk; seed >= 0: that triangle is tested first.  what[node] |= 1 visited, 2 passed geometrically, 4 entered
    auto walk = [&](const Ray& ray, int seed, int& prim, float& closest, std::vector<std::pair<int, int>>& what) {
        const RayBoxCtx ctx = make_box_ctx(ray);
        const int k = mtbvh_order(-ray.d);
        prim = -1; closest = 3.402823466e+38f;
        if (seed >= 0) { float d; if (tri(ray, seed, d)) { closest = d; prim = seed; } }
        const int* nd = nodes[k].data(); int cur = 0;
        while (cur != bvhSize) { const int* n = nd + (size_t)cur * 3; const float* b = &boxes[(size_t)n[1] * 6]; float tb;
            const bool geo = box_hit(ctx, ld3(b), ld3(b + 3), tb), enter = geo && tb < closest;
            what.push_back({ cur, 1 | (geo ? 2 : 0) | (enter ? 4 : 0) });
            if (enter) { if (n[0] >= 0) { float d; if (tri(ray, n[0], d) && d < closest) { closest = d; prim = n[0]; } } cur++; }
            else cur = n[2]; }
        return k;
    };
    // the cut of a cell: the kept nodes of its order, or "none"
    struct Cut { int order; std::set<int> kept; };
    auto cut_of = [&](int x0, int y0, int w, int h) {
        Cut c; CutCell cell = cut_cell(cp, x0, y0, w, h);
        c.order = cell.order;
        if (c.order < 0 || !cut_cell_margin(cell, record(c.order, 0))) { c.order = -1; return c; }
        for (int cur = 0; cur != bvhSize;) { const BvhNode n = record(c.order, cur); if (cut_cell_test(cell, n)) { c.kept.insert(cur); cur++; } else cur = n.next; }
        return c;
    };
    const char* shapeName[3] = { "32x8", "64x8", "32x16" };
    long tiles = 0, uAll = 0, uEntered = 0, uDistance = 0, uGeometric = 0, uSeeded = 0, uCut[3] = { 0, 0, 0 }, missing = 0, seedDiffers = 0, rays = 0;
    long cells[3] = { 0, 0, 0 }, noCut[3] = { 0, 0, 0 }, cutLen[3] = { 0, 0, 0 }, cutMax[3] = { 0, 0, 0 };
    for (int s = 0; s < supers; s++) {
        const int X = (int)(g() % (W / 64)) * 64, Y = (int)(g() % (H / 16)) * 16;
        Cut c32x8[2][2], c64x8[2], c32x16[2];
        for (int j = 0; j < 2; j++) for (int i = 0; i < 2; i++) c32x8[j][i] = cut_of(X + 32 * i, Y + 8 * j, 32, 8);
        for (int j = 0; j < 2; j++) c64x8[j] = cut_of(X, Y + 8 * j, 64, 8);
        for (int i = 0; i < 2; i++) c32x16[i] = cut_of(X + 32 * i, Y, 32, 16);
        auto tally = [&](int shape, const Cut& c) { cells[shape]++; if (c.order < 0) noCut[shape]++; else { cutLen[shape] += (long)c.kept.size(); cutMax[shape] = std::max(cutMax[shape], (long)c.kept.size()); } };
        for (int j = 0; j < 2; j++) for (int i = 0; i < 2; i++) tally(0, c32x8[j][i]);
        for (int j = 0; j < 2; j++) tally(1, c64x8[j]);
        for (int i = 0; i < 2; i++) tally(2, c32x16[i]);
        for (int ty = 0; ty < 2; ty++) for (int tx = 0; tx < 8; tx++) {
            const Cut* cut[3] = { &c32x8[ty][tx / 4], &c64x8[ty], &c32x16[tx / 4] };
            std::map<long, int> flags;                  // order * bvhSize + node -> what
            std::set<long> touchedSeeded;
            for (int l = 0; l < 64; l++) {
                const int x = X + tx * 8 + l % 8, y = Y + ty * 8 + l / 8;
                const Ray rg = camera_center_ray(cp, x, y), rp = camera_sample(cp, x, y, uni(), uni());
                std::vector<std::pair<int, int>> wg, wp, ws;
                int pg, pp, ps; float dg, dp, ds;
                walk(rg, -1, pg, dg, wg);
                const int k = walk(rp, -1, pp, dp, wp);
                walk(rp, pg, ps, ds, ws);
                if (ps != pp || memcmp(&ds, &dp, 4) != 0) seedDiffers++;
                rays++;
                for (auto& e : wp) { flags[(long)k * bvhSize + e.first] |= e.second;
                    if ((e.second & 2) && cut[0]->order == k && !cut[0]->kept.count(e.first)) missing++; }
                for (auto& e : ws) touchedSeeded.insert((long)k * bvhSize + e.first);
            }
            tiles++;
            uAll += (long)flags.size(); uSeeded += (long)touchedSeeded.size();
            for (auto& kv : flags) {
                const int fl = kv.second, k = (int)(kv.first / bvhSize), i = (int)(kv.first % bvhSize);
                if (fl & 4) uEntered++; else if (fl & 2) uDistance++; else uGeometric++;
                for (int sh = 0; sh < 3; sh++) if (cut[sh]->order != k || cut[sh]->kept.count(i)) uCut[sh]++;
            }
        }
    }
    printf("%s, %d triangles, %dx%d, %d super-cells of 64x16 pixels: %ld tiles, %ld rays\n", bistro ? "bistro-class" : "sponza-class", np, W, H, supers, tiles, rays);
    printf("union steps of the reference walk: %ld (%.1f per tile): entered by some lane %ld (%.3f), rejected on distance alone %ld (%.3f), geometric misses for every lane %ld (%.3f)\n",
           uAll, (double)uAll / tiles, uEntered, (double)uEntered / uAll, uDistance, (double)uDistance / uAll, uGeometric, (double)uGeometric / uAll);
    printf("seeding closest with the G-buffer ray's triangle: %ld union steps (%.3f of the reference); results that differ from the unseeded walk: %ld\n", uSeeded, (double)uSeeded / uAll, seedDiffers);
    for (int sh = 0; sh < 3; sh++)
        printf("cut per %-5s cell: %ld union steps (%.3f of the reference); %ld cells, %ld without a cut, cut length mean %.0f max %ld records\n", shapeName[sh], uCut[sh], (double)uCut[sh] / uAll,
               cells[sh], noCut[sh], (double)cutLen[sh] / std::max(1L, cells[sh] - noCut[sh]), cutMax[sh]);
    printf("nodes a ray passes geometrically that its 32x8 cell's cut lacks: %ld\n", missing);
    return missing != 0;
}
