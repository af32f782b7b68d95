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
// Leaf lists (rs_cuts.h "Leaf lists"): the reference tree has one triangle per leaf, so what a still camera's tile can ever test is the
// leaf records of the cut of its OWN 8x8 cell, in the threaded order.  The model prints how long those lists are, what a tile's steps
// become when it walks its list (a list over the cap keeps the 32x8 node cut) for the caps 48 / 96 / 192 / 384, how many accepted
// candidates need the ancestor check (the leaf does not clear the overlap part by chain_step's margin) and how many chain steps those
// take, walks every ray through its list exactly as packet_walk_leaves does and compares primitive and distance with the reference's
// walk bit for bit, and checks containment (every leaf a ray passes geometrically, no distance cull, is in its tile's list) for the
// random jitter and the jitter corners 0 and 1.  Returns non-zero if a leaf is missing or a result differs.
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
    // ---- leaf lists ----
    struct List { int order = -1; std::vector<int> pos; std::set<int> has; };          // positions in the order's array
    auto list_of = [&](int x0, int y0) {
        List L; CutCell cell = cut_cell(cp, x0, y0, 8, 8);
        if (cell.order < 0 || !cut_cell_margin(cell, record(cell.order, 0))) return L;
        L.order = cell.order;
        for (int cur = 0; cur != bvhSize;) { const BvhNode n = record(L.order, cur);
            if (cut_cell_test(cell, n)) { if (n.primId >= 0) { L.pos.push_back(cur); L.has.insert(cur); } cur++; } else cur = n.next; }
        return L;
    };
    std::vector<int> par[6];                    // parent of every record of an order, by position (spans nest: a stack of open spans)
    auto parents = [&](int k) -> const std::vector<int>& {
        if (par[k].empty()) { par[k].assign((size_t)bvhSize, -1); std::vector<int> open;
            for (int i = 0; i < bvhSize; i++) { while (!open.empty() && nodes[k][(size_t)open.back() * 3 + 2] <= i) open.pop_back();
                par[k][(size_t)i] = open.empty() ? -1 : open.back(); if (nodes[k][(size_t)i * 3] < 0) open.push_back(i); } }
        return par[k];
    };
    auto special = [&](const RayBoxCtx& c) { return c.mode != 0 || c.zx || c.zy || c.zz || !(c.d.x == c.d.x); };
    auto root_ext = [&](const RayBoxCtx& c) { const float* b = &boxes[(size_t)nodes[0][1] * 6]; float m = 0.f;
        for (int a = 0; a < 3; a++) { const float o = a == 0 ? c.o.x : a == 1 ? c.o.y : c.o.z, di = a == 0 ? c.dinv.x : a == 1 ? c.dinv.y : c.dinv.z;
            m = fmaxf(m, fmaxf(fabsf((b[a] - o) * di), fabsf((b[3 + a] - o) * di))); }
        return m; };
    // chain_step's `clear`: the three overlap differences of the general case exceed 2^-18 tRoot
    auto clears = [&](const RayBoxCtx& c, const float* b, float tRoot) {
        const float t1x = (b[0] - c.o.x) * c.dinv.x, t1y = (b[1] - c.o.y) * c.dinv.y, t1z = (b[2] - c.o.z) * c.dinv.z;
        const float t2x = (b[3] - c.o.x) * c.dinv.x, t2y = (b[4] - c.o.y) * c.dinv.y, t2z = (b[5] - c.o.z) * c.dinv.z;
        const float nx = fminf(t1x, t2x), ny = fminf(t1y, t2y), nz = fminf(t1z, t2z), fx = fmaxf(t1x, t2x), fy = fmaxf(t1y, t2y), fz = fmaxf(t1z, t2z);
        return fminf(fminf(fy - nz, fz - nx), fx - ny) > tRoot * 3.814697265625e-6f; };
    long lCand = 0, lChecked = 0, lChain = 0, lRefused = 0, lDiffers = 0, lMissing = 0, lRays = 0;
    // packet_walk_leaves for one lane: the list in order, the reference's leaf test with tMin < closest, the triangle, the ancestor check
    auto list_walk = [&](const Ray& ray, const List& L, int& prim, float& closest) {
        const RayBoxCtx ctx = make_box_ctx(ray); const float tRoot = root_ext(ctx); const int k = L.order; const std::vector<int>& pr = parents(k);
        prim = -1; closest = 3.402823466e+38f;
        for (int pos : L.pos) { const int* n = &nodes[k][(size_t)pos * 3]; const float* b = &boxes[(size_t)n[1] * 6]; float tb, d;
            if (!(box_hit(ctx, ld3(b), ld3(b + 3), tb) && tb < closest)) continue;
            if (!(tri(ray, n[0], d) && d < closest)) continue;
            lCand++;
            if (!clears(ctx, b, tRoot)) { lChecked++; bool ok = true;
                for (int a = pr[(size_t)pos]; a >= 0; a = pr[(size_t)a]) { lChain++; const float* ab = &boxes[(size_t)nodes[k][(size_t)a * 3 + 1] * 6]; float ta;
                    if (!(box_hit(ctx, ld3(ab), ld3(ab + 3), ta) && ta < closest)) { ok = false; break; }
                    if (clears(ctx, ab, tRoot)) break; }
                if (!ok) { lRefused++; continue; } }
            closest = d; prim = n[0]; }
    };
    // containment: the whole tree on the geometric part alone
    auto list_contains = [&](const Ray& ray, const List& L) {
        const RayBoxCtx ctx = make_box_ctx(ray);
        if (special(ctx) || mtbvh_order(-ray.d) != L.order) return;
        const int k = L.order;
        for (int cur = 0; cur != bvhSize;) { const int* n = &nodes[k][(size_t)cur * 3]; const float* b = &boxes[(size_t)n[1] * 6]; float tb;
            if (box_hit(ctx, ld3(b), ld3(b + 3), tb)) { if (n[0] >= 0 && !L.has.count(cur)) lMissing++; cur++; } else cur = n[2]; }
    };
    const int caps[4] = { 48, 96, 192, 384 };
    long lTiles = 0, lNone = 0, lLen = 0, lMax = 0, lOver[3] = { 0, 0, 0 }, lSteps[4] = { 0, 0, 0, 0 }, lListed[4] = { 0, 0, 0, 0 }, lTaken[4] = { 0, 0, 0, 0 }, lFlat = 0;
    long uCutLeaf = 0, uLeafEntered = 0;
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
            const List L = list_of(X + tx * 8, Y + ty * 8);
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
                if (L.order >= 0) {
                    list_contains(rp, L); list_contains(camera_sample(cp, x, y, 0.f, 0.f), L); list_contains(camera_sample(cp, x, y, 1.f, 1.f), L);
                    if (k == L.order && !special(make_box_ctx(rp))) { int pl; float dl; list_walk(rp, L, pl, dl); lRays++; if (pl != pp || memcmp(&dl, &dp, 4) != 0) lDiffers++; }
                }
            }
            tiles++;
            uAll += (long)flags.size(); uSeeded += (long)touchedSeeded.size();
            long tileCut = 0, tileOther = 0;            // this tile's steps through the 32x8 cut; of those, in another order than its list's
            for (auto& kv : flags) {
                const int fl = kv.second, k = (int)(kv.first / bvhSize), i = (int)(kv.first % bvhSize);
                if (fl & 4) uEntered++; else if (fl & 2) uDistance++; else uGeometric++;
                for (int sh = 0; sh < 3; sh++) if (cut[sh]->order != k || cut[sh]->kept.count(i)) uCut[sh]++;
                if (cut[0]->order != k || cut[0]->kept.count(i)) { tileCut++; if (k != L.order) tileOther++;
                    if (nodes[k][(size_t)i * 3] >= 0) { uCutLeaf++; if (fl & 4) uLeafEntered++; } }
            }
            lTiles++;
            const long len = (long)L.pos.size();
            if (L.order < 0) lNone++;
            else { lLen += len; lMax = std::max(lMax, len); if (len > 64) lOver[0]++; if (len > 128) lOver[1]++; if (len > 256) lOver[2]++; }
            for (int c = 0; c < 4; c++) {
                const bool take = L.order >= 0 && len > 0 && len <= caps[c];
                lSteps[c] += take ? len + tileOther : tileCut;
                if (take) { lListed[c] += len; lTaken[c]++; }
            }
            if (L.order >= 0 && len <= caps[2]) for (int pos : L.pos) { const float* b = &boxes[(size_t)nodes[L.order][(size_t)pos * 3 + 1] * 6];
                if (b[0] == b[3] || b[1] == b[4] || b[2] == b[5]) lFlat++; }
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
    printf("32x8 cut, per tile: %.1f steps, of which leaf records %.1f, leaves some lane enters %.1f\n", (double)uCut[0] / tiles, (double)uCutLeaf / tiles, (double)uLeafEntered / tiles);
    printf("leaves in the cut of a tile's own 8x8 cell: %ld tiles, %ld without an order, mean %.1f max %ld; tiles over 64 / 128 / 256 leaves: %ld / %ld / %ld\n",
           lTiles, lNone, (double)lLen / std::max(1L, lTiles - lNone), lMax, lOver[0], lOver[1], lOver[2]);
    for (int c = 0; c < 4; c++)
        printf("list cap %3d: %.1f steps per tile (longer lists keep the 32x8 node cut); %ld tiles take a list; %.1f listed leaves per tile\n", caps[c], (double)lSteps[c] / lTiles, lTaken[c], (double)lListed[c] / lTiles);
    printf("listed leaf boxes (cap 192) that are flat on some axis: %.3f\n", (double)lFlat / std::max(1L, lListed[2]));
    printf("list walk, %ld rays (every list, no cap): %ld accepted-or-refused candidates (%.2f per ray), %ld need the ancestor check (%.3f per ray), %ld chain steps (%.2f per check), %ld refused by it\n",
           lRays, lCand, (double)lCand / std::max(1L, lRays), lChecked, (double)lChecked / std::max(1L, lRays), lChain, (double)lChain / std::max(1L, lChecked), lRefused);
    printf("list walk results that differ from the reference walk (primitive or distance bits): %ld\n", lDiffers);
    printf("leaves a ray passes geometrically (random jitter, jitter 0, jitter 1) that its tile's list lacks: %ld\n", lMissing);
    return (missing != 0 || lMissing != 0 || lDiffers != 0) ? 1 : 0;
}
