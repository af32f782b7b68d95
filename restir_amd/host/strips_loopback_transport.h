// strips_loopback_transport.h -- the in-process transport of the "N ranks as N host threads on ONE GPU" checks of the strip driver
// (strips_loopback_ranks.cpp, strips_tracking_ranks.cpp).  It has RCCL's contract -- send / recv are only ENQUEUED on the stream they
// are given, grouped, matched in order per pair of ranks, the send buffer is free again in stream order -- implemented as
// device-to-device copies through a mailbox of staging buffers with events.
#pragma once
#include <condition_variable>

#include "strips_ranks_common.h"

namespace loopback {

constexpr int kMaxRanks = 8, kSlots = 8;
constexpr size_t kSlotBytes = 2u << 20;

struct Slot { char* buf = nullptr; size_t bytes = 0; hipEvent_t ready = nullptr, consumed = nullptr; bool posted = false, used = false; };
struct Channel { Slot slots[kSlots]; int head = 0, tail = 0; };           // messages src -> dst, matched first in, first out
struct Mailbox {
    std::mutex m;
    std::condition_variable cv;
    Channel ch[kMaxRanks][kMaxRanks];
};
struct Op { bool send; void* buf; size_t bytes; int peer; hipStream_t stream; };
struct Endpoint { Mailbox* box; int rank; bool inGroup = false; std::vector<Op> ops; };

// enqueue on `st`: wait until the slot's last reader is done, copy the payload into it, mark it ready
inline int do_send(Endpoint* e, const Op& op) {
    if (op.bytes > kSlotBytes) { std::fprintf(stderr, "loopback: message of %zu bytes exceeds the staging slots\n", op.bytes); return 1; }
    Channel& c = e->box->ch[e->rank][op.peer];
    std::unique_lock<std::mutex> lock(e->box->m);
    Slot& s = c.slots[c.tail % kSlots];
    if (!e->box->cv.wait_for(lock, std::chrono::seconds(60), [&] { return !s.posted; })) { std::fprintf(stderr, "loopback: rank %d -> %d: no free slot (receiver stuck)\n", e->rank, op.peer); return 1; }
    if (s.used && hipStreamWaitEvent(op.stream, s.consumed, 0) != hipSuccess) return 1;
    if (hipMemcpyAsync(s.buf, op.buf, op.bytes, hipMemcpyDeviceToDevice, op.stream) != hipSuccess) return 1;
    if (hipEventRecord(s.ready, op.stream) != hipSuccess) return 1;
    s.bytes = op.bytes; s.posted = true; s.used = true;
    c.tail++;
    e->box->cv.notify_all();
    return 0;
}
// enqueue on `st`: wait for the matching message to be ready, copy it out, mark the slot consumed
inline int do_recv(Endpoint* e, const Op& op) {
    Channel& c = e->box->ch[op.peer][e->rank];
    std::unique_lock<std::mutex> lock(e->box->m);
    Slot& s = c.slots[c.head % kSlots];
    if (!e->box->cv.wait_for(lock, std::chrono::seconds(60), [&] { return s.posted; })) { std::fprintf(stderr, "loopback: rank %d <- %d: nothing was sent\n", e->rank, op.peer); return 1; }
    if (s.bytes != op.bytes) { std::fprintf(stderr, "loopback: rank %d <- %d: %zu bytes expected, %zu sent (send / recv pairing broken)\n", e->rank, op.peer, op.bytes, s.bytes); return 1; }
    if (hipStreamWaitEvent(op.stream, s.ready, 0) != hipSuccess) return 1;
    if (hipMemcpyAsync(op.buf, s.buf, op.bytes, hipMemcpyDeviceToDevice, op.stream) != hipSuccess) return 1;
    if (hipEventRecord(s.consumed, op.stream) != hipSuccess) return 1;
    s.posted = false;
    c.head++;
    e->box->cv.notify_all();
    return 0;
}
inline int run_group(Endpoint* e) {           // as ncclGroupEnd: all sends are issued before any receive waits, so no order of calls can deadlock
    int err = 0;
    for (const Op& op : e->ops) if (op.send && !err) err = do_send(e, op);
    for (const Op& op : e->ops) if (!op.send && !err) err = do_recv(e, op);
    e->ops.clear();
    return err;
}
inline int lb_group_begin(void* ctx) { ((Endpoint*)ctx)->inGroup = true; return 0; }
inline int lb_group_end(void* ctx) { Endpoint* e = (Endpoint*)ctx; e->inGroup = false; return run_group(e); }
inline int lb_send(void* ctx, const void* buf, size_t bytes, int peer, void* stream) {
    Endpoint* e = (Endpoint*)ctx;
    e->ops.push_back({ true, const_cast<void*>(buf), bytes, peer, (hipStream_t)stream });
    return e->inGroup ? 0 : run_group(e);
}
inline int lb_recv(void* ctx, void* buf, size_t bytes, int peer, void* stream) {
    Endpoint* e = (Endpoint*)ctx;
    e->ops.push_back({ false, buf, bytes, peer, (hipStream_t)stream });
    return e->inGroup ? 0 : run_group(e);
}

// the transport of one rank over `ep`
inline rs_transport transport_of(Endpoint* ep) {
    rs_transport t{};
    t.ctx = ep; t.group_begin = lb_group_begin; t.group_end = lb_group_end; t.send = lb_send; t.recv = lb_recv; t.stream_ordered = 1;
    return t;
}
// staging slots and events of every pair of ranks, on the current device
inline bool mailbox_init(Mailbox& box, int world) {
    for (int a = 0; a < world; a++) for (int b = 0; b < world; b++) {
        if (a == b) continue;
        for (Slot& s : box.ch[a][b].slots) {
            if (hipMalloc((void**)&s.buf, kSlotBytes) != hipSuccess || hipEventCreateWithFlags(&s.ready, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&s.consumed, hipEventDisableTiming) != hipSuccess) { std::fprintf(stderr, "mailbox allocation failed\n"); return false; }
        }
    }
    return true;
}

}  // namespace loopback
