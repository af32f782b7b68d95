// rs_cut_plan.h -- the device-free half of a primary-cut slot (primary_cuts.hip; rs_cuts.h says what a cut is): the KEY a slot's cuts and
// leaf lists were built from, what a phase-A call does with its slot given this call's key (rs_primary_cut_slot -> cutState), and how
// large the two arenas of a launch geometry are -- as functions of plain structs and integers (include/restir_hip.h).  Nothing here
// touches the device, a context or a global: primary_cuts.hip asks these functions and acts on what they return, and
// rs_debug_plan_primary_cut_slot hands them to a test that has no device.
#pragma once

#include <cstring>

#include "../../include/restir_hip.h"

// every byte of the camera counts (the size is the camera's resolution, which check_frame_args holds to the object's)
inline bool rs_cut_key_equal(const rs_primary_cut_key& a, const rs_primary_cut_key& b) {
    return a.sceneId == b.sceneId && a.geomEdits == b.geomEdits && std::memcmp(&a.cam, &b.cam, sizeof(rs_camera)) == 0 &&
           a.y0 == b.y0 && a.y1 == b.y1 && a.cap == b.cap && a.listCap == b.listCap;
}

inline void rs_cut_slot_forget(rs_primary_cut_slot& s) { s.keyValid = 0; s.cuts = s.lists = RS_CUT_ARENA_NOTHING; }

// rs_phase_a_inputs::cutState for a call with key `key`, and the slot as the call leaves it for the same call of the next frame.
// Switch off, or the library stream being captured (a build is not recorded into a graph): nothing is remembered.  The key of the
// previous frame: 1 until the build has run (primary_cuts.hip sets `cuts` to built, or to no memory, after which this key keeps the tree),
// 2 from then on.  Another key: it is stored, whatever was built or refused for the old one is forgotten, and this frame walks the tree.
inline int rs_plan_cut_slot(bool on, bool capturing, rs_primary_cut_slot& s, const rs_primary_cut_key& key) {
    if (!on || capturing) { rs_cut_slot_forget(s); return 0; }
    if (s.keyValid && rs_cut_key_equal(s.key, key)) return s.cuts == RS_CUT_ARENA_NO_MEMORY ? 0 : s.cuts == RS_CUT_ARENA_BUILT ? 2 : 1;
    rs_cut_slot_forget(s);
    s.keyValid = 1; s.key = key;
    return 0;
}

constexpr unsigned kCutArenaPerCell = 512;     // the arena holds this many records per cell (or the cap, if smaller); cells that do not fit take no cut
constexpr unsigned kListArenaPerTile = 32;     // the lists' arena: this many 64-byte records per tile (the model's mean is 20 / 29 at the default cap); tiles that do not fit take no list

// The arenas of a launch of tilesX x tilesY blocks: a cell is a block (32x8 pixels), a tile a quarter of one.  listCap 0: no lists.
inline rs_primary_cut_sizes rs_plan_cut_sizes(int tilesX, int tilesY, unsigned cap, unsigned listCap) {
    rs_primary_cut_sizes z;
    z.numCells = tilesX * tilesY;
    const unsigned long long want = (unsigned long long)z.numCells * (cap < kCutArenaPerCell ? cap : kCutArenaPerCell);
    z.capacity = want < 0x7fffffffull ? (unsigned)want : 0x7fffffffu;
    z.numTiles = listCap ? z.numCells * 4 : 0;
    const unsigned long long wantList = (unsigned long long)z.numTiles * (listCap < kListArenaPerTile ? listCap : kListArenaPerTile);
    z.listCapacity = wantList < 0x3ffffffull ? (unsigned)wantList : 0x3ffffffu;       // (byte offsets of 64-byte records stay below 2^32)
    return z;
}
