// rs_row_layouts.h -- the packed layout of N rows, written down once.  "N rows of X, packed" always means the rows of X's planes, one plane
// after the other (include/restir_hip.h documents each).  A layout is a list of planes with their bytes per pixel; the public row packing
// (restir.hip, gbuffer.hip) and every message of the strip driver (strips.hip) are sized by it and built from it with add_rows, so two
// places cannot disagree about an offset: there are none, only running sums.
#pragma once
#include "rs_copy_segments.h"

namespace rs_rows {
using rs_copy::SegList;

struct Plane { void* base; size_t bytesPerPixel; };
struct Planes {
    int width, n;
    Plane p[4];
    rs_gbuffer* noteTo = nullptr; int set = 0;             // planes of a G-buffer set: an unpack tells the G-buffer (add_rows)
    size_t bytes_per_pixel() const { size_t sum = 0; for (int i = 0; i < n; i++) sum += p[i].bytesPerPixel; return sum; }
    size_t bytes(int frameWidth, int rows) const { return (size_t)frameWidth * (size_t)(rows > 0 ? rows : 0) * bytes_per_pixel(); }
};

// The four layouts.  A null object gives the layout alone -- what a size needs -- with no planes behind it.
// reservoir buffer `which` 0 (written this frame) / 1 (read by the temporal merge): li, wi, w, m -- 40 B/px
inline Planes reservoir_planes(rs_restir* r, int which) {
    const ResvPlanes b = !r ? ResvPlanes{} : which == 0 ? r->cur : r->last;
    return { r ? r->width : 0, 4, { { b.li, 16 }, { b.wi, 16 }, { b.w, 4 }, { b.m, 4 } } };
}
// the published copy the spatial pass gathers from (which = 2): li, wi, tap -- 48 B/px
inline Planes published_planes(rs_restir* r) {
    const TempPlanes b = r ? r->temp : TempPlanes{};
    return { r ? r->width : 0, 3, { { b.li, 16 }, { b.wi, 16 }, { b.tap, 16 } } };
}
// (the two above under the public functions' numbering of the reservoir buffers: which = 0 / 1 / 2)
inline Planes restir_planes(const rs_restir* r, int which) {
    return which == 2 ? published_planes(const_cast<rs_restir*>(r)) : reservoir_planes(const_cast<rs_restir*>(r), which);
}
// set `set` of the G-buffer's id, normal and depth planes -- 20 B/px
inline Planes gbuffer_planes(rs_gbuffer* g, int set) {
    if (!g) return { 0, 3, { { nullptr, 4 }, { nullptr, 12 }, { nullptr, 4 } } };
    return { g->width, 3, { { g->primId[set], 4 }, { g->normal[set], 12 }, { g->depth[set], 4 } }, g, set };
}
// the light-id plane that goes with reservoir buffer `which` 0 / 1 / 2 (light tracking) -- 4 B/px
inline Planes light_id_plane(rs_restir* r, int which) {
    return { r ? r->width : 0, 1, { { r ? rs_light_id_plane(r->lights, which) : nullptr, 4 } } };
}

// Rows [y, y + rows) of every plane of `planes` against a packed buffer: plane after plane from `packed` on; returns the address after the
// last, where the next layout of the same message goes on.  An unpacking list that writes G-buffer planes says so to the G-buffer here
// (rs_gbuffer_note_write: a content key that survived the overwrite would make the reuse path hand out stale planes): no caller can forget it.
inline char* add_rows(SegList& l, const Planes& planes, int y, int rows, char* packed) {
    const size_t n = (size_t)planes.width * rows, off = (size_t)y * planes.width;
    for (const Plane* p = planes.p; p < planes.p + planes.n; packed += n * p->bytesPerPixel, p++)
        l.add((char*)p->base + off * p->bytesPerPixel, packed, n * p->bytesPerPixel);
    if (!l.pack && planes.noteTo) rs_gbuffer_note_write(planes.noteTo, planes.set, y, rows);
    return packed;
}

}  // namespace rs_rows
