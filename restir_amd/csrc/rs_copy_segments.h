// rs_copy_segments.h -- several rows-of-a-plane copies as ONE launch: the strip driver's messages (strips.hip) and the row packing of the
// light-id planes (restir.hip); or, where it always was, one hipMemcpyAsync per plane.  Which planes a packed layout has: rs_row_layouts.h.
#pragma once
#include "rs_internal.h"

namespace rs_copy {

// Packing and unpacking the border rows of a frame: 6 planes (published reservoirs li / wi / tap, G-buffer id / normal / depth) x 2
// edges.  As 24 hipMemcpyAsync calls per frame they cost the HOST 0.12 ms -- more than half of what a 1/8 strip's kernels last
// (tools/host_enqueue_strips.py: 0.210 ms of host time per frame against 0.18 ms of kernels) -- so all segments of a direction go
// through ONE launch of a copy kernel that finds its segment from a table passed by value.  The same launch carries the eight planes of a
// tracked history message (rs_strips_exchange_history: the own rows packed by one launch, every peer's unpacked by one) and, with a
// table of one segment, the rows of a light-id plane (rs_restir_light_rows_pack / _unpack).
constexpr int kMaxSegs = 12;
struct CopyTable { const char* src[kMaxSegs]; char* dst[kMaxSegs]; unsigned start[kMaxSegs + 1]; int n; };      // start: in units of `unit` bytes
template <typename T>
__global__ void __launch_bounds__(256) k_copy_segments(CopyTable t) {
    RS_SETPRIO(RS_PRIO_STREAM);
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= t.start[t.n]) return;
    int k = 0;
    while (i >= t.start[k + 1]) k++;
    reinterpret_cast<T*>(t.dst[k])[i - t.start[k]] = reinterpret_cast<const T*>(t.src[k])[i - t.start[k]];
}
// pack: plane -> packed buffer; unpack: packed buffer -> plane.  Said once, when the list is made: whoever adds segments knows which side is written.
struct SegList {
    const bool pack;
    const char* a[kMaxSegs]; char* b[kMaxSegs]; size_t bytes[kMaxSegs]; int n = 0;
    explicit SegList(bool packing) : pack(packing) {}
    void add(const void* plane, void* packed, size_t nbytes) { a[n] = (const char*)plane; b[n] = (char*)packed; bytes[n] = nbytes; n++; }
    const char* src(int k) const { return pack ? a[k] : b[k]; }
    char* dst(int k) const { return pack ? b[k] : const_cast<char*>(a[k]); }
};
// the two ways to carry a list out, both on the library stream: one launch of the copy kernel ...
inline int copy_segments(const SegList& l) {
    if (l.n == 0) return 0;
    bool wide = true;
    for (int k = 0; k < l.n; k++) wide = wide && l.bytes[k] % 16 == 0 && ((size_t)l.a[k] % 16 == 0) && ((size_t)l.b[k] % 16 == 0);
    const unsigned unit = wide ? 16u : 4u;
    CopyTable t; t.n = l.n; t.start[0] = 0;
    for (int k = 0; k < l.n; k++) {
        t.src[k] = l.src(k);
        t.dst[k] = l.dst(k);
        t.start[k + 1] = t.start[k] + (unsigned)(l.bytes[k] / unit);
    }
    const unsigned total = t.start[t.n];
    if (total == 0) return 0;
    if (wide) hipLaunchKernelGGL(k_copy_segments<uint4>, dim3((total + 255) / 256), dim3(256), 0, rs_stream(), t);
    else hipLaunchKernelGGL(k_copy_segments<unsigned>, dim3((total + 255) / 256), dim3(256), 0, rs_stream(), t);
    return rs_check_hip(hipGetLastError(), "copy of plane rows (k_copy_segments)");
}
// ... or one hipMemcpyAsync per segment (the public reservoir and G-buffer row packing, the untracked history message)
inline int memcpy_segments(const SegList& l) {
    for (int k = 0; k < l.n; k++)
        if (l.bytes[k]) RS_HIP(hipMemcpyAsync(l.dst(k), l.src(k), l.bytes[k], hipMemcpyDeviceToDevice, rs_stream()));
    return 0;
}

}  // namespace rs_copy
