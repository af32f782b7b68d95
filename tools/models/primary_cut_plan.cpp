// tools/models/primary_cut_plan.cpp -- the host-and-device functions of the primary cuts on their edge cases, as a stand-alone host program
// for AddressSanitizer + UBSan: the cut's walk and its re-linking (restir_amd/csrc/rs_cuts.h cut_walk, cut_relink -- the functions the
// device builders of primary_cuts.hip run) over a small threaded tree made here, every output array allocated at exactly the size the
// contract promises, and the slot's plan (rs_cut_plan.h).  No device is touched and nothing of the library is linked.  From restir_amd/csrc:
//   hipcc -O1 -g -std=c++17 -ffp-contract=off -x hip --offload-arch=gfx950 --cuda-host-only -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-omit-frame-pointer -I. -c ../../tools/models/primary_cut_plan.cpp -o /tmp/primary_cut_plan.o
//   hipcc -fsanitize=address,undefined /tmp/primary_cut_plan.o -o /tmp/primary_cut_plan        (a host object only: the sanitizers never see device code)
//   /tmp/primary_cut_plan        (prints "primary_cut_plan: ok"; a failed check or a sanitizer report ends it with a non-zero status)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "rs_cuts.h"
#include "rs_cut_plan.h"

using namespace rs;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "primary_cut_plan.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

namespace {

// A threaded tree in pre-order over a 16 x 16 grid of flat leaf boxes in the plane z = 0 (x, y in [-2, 2]): a node splits its range of
// leaves in halves; `next` is the miss link (the record after the subtree; the table's length at the end)
struct Tree {
    std::vector<BvhNode> rec;
    int build(int lo, int hi) {                      // leaves [lo, hi) in Morton-free row order; returns the node's index
        const int at = (int)rec.size();
        rec.push_back(BvhNode{});
        float mn[3] = { 1e30f, 1e30f, 0.f }, mx[3] = { -1e30f, -1e30f, 0.f };
        for (int i = lo; i < hi; i++) {
            const float x = -2.f + 0.25f * (float)(i % 16), y = -2.f + 0.25f * (float)(i / 16);
            mn[0] = std::fmin(mn[0], x); mx[0] = std::fmax(mx[0], x + 0.2f); mn[1] = std::fmin(mn[1], y); mx[1] = std::fmax(mx[1], y + 0.2f);
        }
        if (hi - lo > 1) { build(lo, (lo + hi) / 2); build((lo + hi) / 2, hi); }
        rec[(size_t)at] = BvhNode{ mn[0], mn[1], mn[2], mx[2], mx[0], mx[1], hi - lo > 1 ? kNullPrim : lo, (int)rec.size() };
        return at;
    }
    Tree() { build(0, 256); }
};

// a camera at `pos` whose view is turned off every axis, 96 x 54 pixels, a narrow lens
CamParams camera(f3 pos, f3 view) {
    CamParams c{};
    c.position = pos;
    c.view = normalize(view);
    c.right = normalize(cross(c.view, mk3(0.f, 1.f, 0.f)));
    c.up = cross(c.right, c.view);
    c.width = 96; c.height = 54;
    c.aspect = 96.f / 54.f; c.tanFovY = 0.2f; c.focalDist = 1.f; c.lensRadius = 0.f;
    c.pixelSizeX = 1.f / 96.f; c.pixelSizeY = 1.f / 54.f;
    return c;
}

struct Cut { int order; unsigned count; std::vector<unsigned> pos; };

// the walk with its outputs in a heap array of exactly min(count, cap) entries (a first walk says how many)
template <bool LEAVES>
Cut walk(const Tree& t, const CamParams& cam, int x0, int y0, int w, int h, unsigned cap) {
    Cut c{ -1, 0u, {} };
    CutCell cell = cut_cell(cam, x0, y0, w, h);
    if (cell.order < 0 || !cut_cell_margin(cell, t.rec[0])) return c;
    c.order = cell.order;
    auto rec = [&](unsigned i) { CHECK(i < t.rec.size()); return t.rec[i]; };
    const unsigned end = (unsigned)t.rec.size();
    c.count = cut_walk<LEAVES>(cell, rec, end, cap, [](unsigned, unsigned, const BvhNode&) {});
    CHECK(c.count <= cap + 1u);
    c.pos.resize(c.count < cap ? c.count : cap);
    unsigned calls = 0;
    const unsigned again = cut_walk<LEAVES>(cell, rec, end, cap, [&](unsigned k, unsigned at, const BvhNode& n) {
        CHECK(k == calls && k < c.pos.size());
        CHECK(!LEAVES || n.primId != kNullPrim);
        c.pos[k] = at; calls++;
    });
    CHECK(again == c.count && calls == c.pos.size());
    return c;
}

std::vector<unsigned> relink(const Tree& t, const std::vector<unsigned>& pos) {
    std::vector<unsigned> links(pos.size(), 0xffffffffu);
    unsigned calls = 0;
    cut_relink([&](unsigned j) { CHECK(j < pos.size()); return pos[j]; }, [&](unsigned i) { CHECK(i < pos.size()); return (unsigned)t.rec[pos[i]].next; },
               (unsigned)pos.size(), [&](unsigned i, unsigned to) { CHECK(i == calls); links[i] = to; calls++; });
    CHECK(calls == pos.size());
    return links;
}

void walks_and_links() {
    const Tree t;
    const unsigned end = (unsigned)t.rec.size();
    CHECK(end == 511u && t.rec[0].next == (int)end);
    const CamParams cam = camera(mk3(1.5f, 1.0f, 6.f), mk3(-0.3f, -0.2f, -1.f));
    int cuts = 0;
    for (int y0 = 0; y0 < 54; y0 += 8) for (int x0 = 0; x0 < 96; x0 += 32) {
        const Cut c = walk<false>(t, cam, x0, y0, 32, 8, 1u << 24);
        if (c.order < 0 || c.count == 0u) continue;
        cuts++;
        CHECK(c.count < end);                       // a selection, not the tree
        std::vector<char> kept(end, 0);
        for (size_t i = 0; i < c.pos.size(); i++) { CHECK(i == 0 || c.pos[i] > c.pos[i - 1]); kept[c.pos[i]] = 1; }
        for (unsigned p : c.pos) for (unsigned a = 0; a < p; a++) if ((unsigned)t.rec[a].next > p) CHECK(kept[a]);      // closed under ancestors
        const std::vector<unsigned> links = relink(t, c.pos);
        for (unsigned i = 0; i < c.count; i++) {
            unsigned want = c.count;
            for (unsigned j = c.count; j-- > i + 1u;) if (c.pos[j] >= (unsigned)t.rec[c.pos[i]].next) want = j;
            CHECK(links[i] == want && links[i] > i);
            for (unsigned j = i + 1u; j < links[i]; j++) CHECK(links[j] <= links[i]);       // nested
        }
        // the caps: one short, exact, one more, none
        const Cut shorter = walk<false>(t, cam, x0, y0, 32, 8, c.count - 1u), exact = walk<false>(t, cam, x0, y0, 32, 8, c.count), more = walk<false>(t, cam, x0, y0, 32, 8, c.count + 1u);
        CHECK(shorter.count == c.count && shorter.pos.size() == c.count - 1u && std::equal(shorter.pos.begin(), shorter.pos.end(), c.pos.begin()));
        CHECK(exact.count == c.count && exact.pos == c.pos && more.count == c.count && more.pos == c.pos);
        const Cut none = walk<false>(t, cam, x0, y0, 32, 8, 0u);
        CHECK(none.count == 1u && none.pos.empty());
        // the four tiles' leaf lists: the leaves of the cut of their own 8 x 8 pixels, each a part of the block's cut
        for (int q = 0; q < 4; q++) {
            const Cut nodes8 = walk<false>(t, cam, x0 + 8 * q, y0, 8, 8, 1u << 24), leaves = walk<true>(t, cam, x0 + 8 * q, y0, 8, 8, 1u << 24);
            CHECK(nodes8.order == c.order && leaves.order == c.order);
            std::vector<unsigned> want;
            for (unsigned p : nodes8.pos) { CHECK(kept[p]); if (t.rec[p].primId != kNullPrim) want.push_back(p); }
            CHECK(leaves.pos == want);
            if (!want.empty()) {
                const Cut capped = walk<true>(t, cam, x0 + 8 * q, y0, 8, 8, (unsigned)want.size() - 1u);
                CHECK(capped.count == want.size() && capped.pos.size() == want.size() - 1u);
            }
        }
    }
    CHECK(cuts >= 6);
    // re-linking at its ends: no record, one record, every record (the tree's own links come back)
    CHECK(relink(t, {}).empty());
    CHECK(relink(t, { 7u }) == std::vector<unsigned>{ 1u });
    std::vector<unsigned> all(end);
    for (unsigned i = 0; i < end; i++) all[i] = i;
    const std::vector<unsigned> same = relink(t, all);
    for (unsigned i = 0; i < end; i++) CHECK(same[i] == (unsigned)t.rec[i].next);
    // a block that looks past the tree has an order and no record; one that holds a sign change, a camera beyond the lens bound, a
    // position or a root box that is not finite: no order
    const Cut past = walk<false>(t, camera(mk3(40.f, 30.f, 6.f), mk3(0.3f, 0.2f, -1.f)), 32, 24, 32, 8, 64u);
    CHECK(past.order >= 0 && past.count == 0u && past.pos.empty());
    CHECK(walk<false>(t, camera(mk3(0.f, 0.f, 6.f), mk3(0.f, 0.f, -1.f)), 32, 24, 32, 8, 64u).order == -1);
    CamParams wide = cam; wide.tanFovY = 17.f;
    CHECK(cut_cell(wide, 0, 0, 32, 8).order == -1);
    CamParams lost = cam; lost.position.x = std::numeric_limits<float>::quiet_NaN();
    CHECK(cut_cell(lost, 0, 0, 32, 8).order == -1);
    Tree broken; broken.rec[0].bmaxx = std::numeric_limits<float>::infinity();
    CHECK(walk<false>(broken, cam, 0, 0, 32, 8, 64u).order == -1);
}

rs_primary_cut_key key() {
    rs_primary_cut_key k;
    std::memset(&k, 0, sizeof k);
    k.sceneId = 7; k.geomEdits = 3; k.cam.position[0] = 1.f; k.cam.resolution[0] = 96; k.cam.resolution[1] = 54; k.y0 = 0; k.y1 = 54; k.cap = 4096; k.listCap = 192;
    return k;
}

void slot_plan() {
    rs_primary_cut_slot s{};
    const rs_primary_cut_key k = key();
    CHECK(rs_plan_cut_slot(true, false, s, k) == 0 && s.keyValid == 1);
    CHECK(rs_plan_cut_slot(true, false, s, k) == 1 && rs_plan_cut_slot(true, false, s, k) == 1);
    s.cuts = s.lists = RS_CUT_ARENA_BUILT;
    CHECK(rs_plan_cut_slot(true, false, s, k) == 2);
    s.lists = RS_CUT_ARENA_NO_MEMORY;
    CHECK(rs_plan_cut_slot(true, false, s, k) == 2 && s.lists == RS_CUT_ARENA_NO_MEMORY);
    s.cuts = RS_CUT_ARENA_NO_MEMORY;
    CHECK(rs_plan_cut_slot(true, false, s, k) == 0 && s.cuts == RS_CUT_ARENA_NO_MEMORY && s.keyValid == 1);
    for (int off = 0; off < 2; off++) {             // the switch off; the stream being captured
        s.cuts = s.lists = RS_CUT_ARENA_BUILT;
        CHECK(rs_plan_cut_slot(off == 0 ? false : true, off == 1, s, k) == 0 && !s.keyValid && s.cuts == RS_CUT_ARENA_NOTHING && s.lists == RS_CUT_ARENA_NOTHING);
        CHECK(rs_plan_cut_slot(true, false, s, k) == 0 && s.keyValid == 1);
    }
    // every member of the key, every byte of the camera
    auto differs = [&](const rs_primary_cut_key& other) {
        rs_primary_cut_slot t{};
        (void)rs_plan_cut_slot(true, false, t, k);
        t.cuts = t.lists = RS_CUT_ARENA_BUILT;
        CHECK(rs_plan_cut_slot(true, false, t, k) == 2);
        CHECK(rs_plan_cut_slot(true, false, t, other) == 0 && t.keyValid == 1 && t.cuts == RS_CUT_ARENA_NOTHING && t.lists == RS_CUT_ARENA_NOTHING);
        CHECK(rs_cut_key_equal(t.key, other) && !rs_cut_key_equal(t.key, k));
        CHECK(rs_plan_cut_slot(true, false, t, other) == 1);
    };
    { rs_primary_cut_key o = k; o.sceneId++; differs(o); }
    { rs_primary_cut_key o = k; o.geomEdits++; differs(o); }
    { rs_primary_cut_key o = k; o.y0 = 8; differs(o); }
    { rs_primary_cut_key o = k; o.y1 = 46; differs(o); }
    { rs_primary_cut_key o = k; o.cap = 4095; differs(o); }
    { rs_primary_cut_key o = k; o.listCap = 0; differs(o); }
    for (size_t b = 0; b < sizeof(rs_camera); b++) { rs_primary_cut_key o = k; reinterpret_cast<unsigned char*>(&o.cam)[b] ^= 1u; differs(o); }

    auto sizes = [](int tx, int ty, unsigned cap, unsigned listCap, int cells, unsigned capacity, int tiles, unsigned listCapacity) {
        const rs_primary_cut_sizes z = rs_plan_cut_sizes(tx, ty, cap, listCap);
        return z.numCells == cells && z.capacity == capacity && z.numTiles == tiles && z.listCapacity == listCapacity;
    };
    CHECK(sizes(1, 1, 1, 192, 1, 1u, 4, 128u) && sizes(1, 1, 512, 192, 1, 512u, 4, 128u) && sizes(1, 1, 513, 192, 1, 512u, 4, 128u));
    CHECK(sizes(1, 1, 1u << 24, 192, 1, 512u, 4, 128u));
    CHECK(sizes(3, 7, 8, 0, 21, 168u, 0, 0u) && sizes(3, 7, 8, 32, 21, 168u, 84, 84u * 32u) && sizes(3, 7, 8, 33, 21, 168u, 84, 84u * 32u));
    CHECK(sizes(2048, 2048, 4096, 0, 1 << 22, 0x7fffffffu, 0, 0u) && sizes(2048, 2047, 4096, 0, 2048 * 2047, 2048u * 2047u * 512u, 0, 0u));
    CHECK(sizes(1024, 512, 1, 192, 1 << 19, 1u << 19, 1 << 21, 0x3ffffffu) && sizes(1024, 511, 1, 192, 1024 * 511, 1024u * 511u, 4096 * 511, 4096u * 511u * 32u));
    CHECK(sizes(0, 0, 4096, 192, 0, 0u, 0, 0u));
}

}  // namespace

int main() {
    walks_and_links();
    slot_plan();
    std::printf("primary_cut_plan: ok\n");
    return 0;
}
