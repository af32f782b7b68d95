// internal_streams.hip -- the streams the library makes for itself: rs_context::streams and everything that reads or changes it.
// The decisions are rs_stream_choice.h's, which needs no device; here are the measurement, the streams' creation and destruction, and the
// entry points.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rs_internal.h"

// In overlapped mode four streams carry work at any time: the caller's (temporal / spatial passes, tone map, the strip driver's
// transfers) and three of the library's own (the chains of consecutive frames).  Whether four streams of a process really run side by
// side is decided below the API: the runtime maps streams onto four hardware queues PER PRIORITY LEVEL in the order they are made, the
// legacy default stream holds one of the normal level's, and how hardware queues share the command processor's pipes depends on every
// queue the process has made before -- torch's stream pool, an ncclComm's own streams.  Measured on 1/8 strips of 1080p
// (profiles/r05_ab_stream_priority_pools.log, r05_ab_stream_levels_with_rccl.log): three normal-priority streams next to an ordinary caller
// stream 0.29 ms per frame instead of 0.19 (five streams on four queues); the same three at high priority 0.19 -- until a one-rank RCCL
// communicator exists in the process, then 0.39, and only the normal level gives 0.17.  No fixed rule survives all of that, so the
// streams are CHOSEN BY MEASUREMENT when they are first needed (and again after rs_set_stream): four candidates per level, and for
// every triple of a level eight rounds of [a 20-us spin on each of the four streams, an event hand-over to the neighbour] are timed
// (tools/micro/queue_quads.hip is the same test stand-alone: 280-320 us when the four run side by side, 450-860 when two of them take
// turns).  The best triple within 8 % of the fastest is kept, levels in the order of rs_set_internal_stream_priority's preference
// (default: above the caller's stream -- the chains are the frame's critical path, config 3 1.071 -> 1.045 ms; with a denoiser on the
// library stream below it, config 5 1.87 -> 1.78 ms); the other nine streams are destroyed.  About 25 ms, once, with the device idle:
// the one place where the overlapped mode waits on the host.
namespace {
__global__ void k_calibration_spin(long long ticks) {
    const long long t0 = wall_clock64();                                // 100 MHz
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
struct Calibration {
    static constexpr int kMax = 8;
    hipEvent_t begin = nullptr, end[kMax] = {}, hand[8][kMax] = {};
    bool ok = true;
    Calibration() {
        ok = hipEventCreate(&begin) == hipSuccess;
        for (auto& e : end) ok = ok && hipEventCreate(&e) == hipSuccess;
        for (auto& r : hand) for (auto& e : r) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    }
    ~Calibration() {
        if (begin) (void)hipEventDestroy(begin);
        for (auto& e : end) if (e) (void)hipEventDestroy(e);
        for (auto& r : hand) for (auto& e : r) if (e) (void)hipEventDestroy(e);
        (void)hipGetLastError();
    }
    // microseconds until all n streams have finished their eight rounds (best of three), or a negative value on error
    double chained(const hipStream_t* s, int n = 4) {
        double best = 1e30;
        for (int rep = 0; rep < 3; rep++) {
            for (int k = 0; k < n; k++) if (hipStreamSynchronize(s[k]) != hipSuccess) return -1;      // (these streams only: other contexts' work goes on)
            (void)hipEventRecord(begin, s[0]);
            for (int r = 0; r < 8; r++) {
                for (int k = 0; k < n; k++) { hipLaunchKernelGGL(k_calibration_spin, dim3(1), dim3(64), 0, s[k], 2000); (void)hipEventRecord(hand[r][k], s[k]); }
                for (int k = 0; k < n; k++) (void)hipStreamWaitEvent(s[k], hand[r][(k + 1) % n], 0);
            }
            for (int k = 0; k < n; k++) (void)hipEventRecord(end[k], s[k]);
            for (int k = 0; k < n; k++) if (hipEventSynchronize(end[k]) != hipSuccess) return -1;
            float worst = 0.f;
            for (int k = 0; k < n; k++) { float t = 0.f; if (hipEventElapsedTime(&t, begin, end[k]) != hipSuccess) return -1; worst = t > worst ? t : worst; }
            best = worst < best ? worst : best;
        }
        return best * 1e3;
    }
};

// fills `out` with the streams chosen by measurement next to `caller`, their priority and times; false: nothing could be measured (plain streams)
bool measure_streams(hipStream_t caller, int asked, rs_stream_choice& out) {
    static_assert(rs_context::kAux >= 3 && rs_context::kAux < Calibration::kMax, "three auxiliary streams (measurement builds: up to seven)");
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (rs_context::kAux != 3) {
        // measurement builds with more chains in flight (-DRS_AUX_STREAMS=4): twelve candidates, chosen greedily -- the stream that runs
        // best next to the ones already chosen, one at a time
        Calibration cal;
        if (!cal.ok) { (void)hipGetLastError(); return false; }
        std::vector<hipStream_t> cand;
        for (int p : { greatest, 0, least }) for (int i = 0; i < 4; i++) { hipStream_t st = nullptr; if (hipStreamCreateWithPriority(&st, hipStreamNonBlocking, p) == hipSuccess) cand.push_back(st); }
        (void)hipGetLastError();
        hipStream_t chosen[Calibration::kMax] = { caller };
        double last = 0;
        for (int k = 1; k <= rs_context::kAux; k++) {
            int best = -1; double bestT = 1e30;
            for (size_t i = 0; i < cand.size(); i++) {
                if (!cand[i]) continue;
                chosen[k] = cand[i];
                const double t = cal.chained(chosen, k + 1);
                if (t >= 0 && t < bestT) { bestT = t; best = (int)i; }
            }
            if (best < 0) { for (hipStream_t st : cand) if (st) (void)hipStreamDestroy(st); return false; }
            chosen[k] = cand[(size_t)best]; cand[(size_t)best] = nullptr; last = bestT;
        }
        for (hipStream_t st : cand) if (st) (void)hipStreamDestroy(st);
        for (int k = 0; k < rs_context::kAux; k++) out.stream[k] = chosen[k + 1];
        out.priority = 0; out.chosenUs = last; out.fastestUs = last;
        return true;
    }
    int own = 0;
    if (caller && hipStreamGetPriority(caller, &own) != hipSuccess) { (void)hipGetLastError(); own = 0; }
    int order[3];
    const int n = rs_stream_level_order(least, greatest, asked, caller != nullptr, own, order);
    Calibration cal;
    if (!cal.ok) { (void)hipGetLastError(); return false; }
    hipStream_t cand[3][4] = {};
    double t[3][4];
    for (int q = 0; q < n; q++) for (double& x : t[order[q]]) x = -1;   // not measured: as long as one of them stays so, nothing is chosen
    bool made = true;
    for (int q = 0; q < n && made; q++)
        for (int i = 0; i < 4 && made; i++) made = hipStreamCreateWithPriority(&cand[order[q]][i], hipStreamNonBlocking, rs_stream_level_priority(order[q], least, greatest)) == hipSuccess;
    for (int q = 0; q < n && made; q++)
        for (int skip = 0; skip < 4 && made; skip++) {
            hipStream_t s[4] = { caller };
            int k = 1;
            for (int i = 0; i < 4; i++) if (i != skip) s[k++] = cand[order[q]][i];
            t[order[q]][skip] = cal.chained(s);
            made = t[order[q]][skip] >= 0;
        }
    const rs_stream_pick pick = rs_pick_streams(t, order, n);
    int k = 0;
    for (int p = 0; p < 3; p++)
        for (int i = 0; i < 4; i++) {
            if (!cand[p][i]) continue;
            if (p == pick.level && i != pick.skip) out.stream[k++] = cand[p][i];
            else (void)hipStreamDestroy(cand[p][i]);
        }
    (void)hipGetLastError();
    if (pick.level < 0) return false;
    out.priority = rs_stream_level_priority(pick.level, least, greatest);
    out.chosenUs = t[pick.level][pick.skip];
    out.fastestUs = pick.fastest;
    return true;
}

void destroy_streams(const rs_stream_choice& ch, bool wait) {
    for (void* st : ch.stream) if (st) { if (wait) (void)hipStreamSynchronize((hipStream_t)st); (void)hipStreamDestroy((hipStream_t)st); }
}

bool streams_on(rs_internal_streams& s) {
    if (s.mode < 0) {
        // RS_SIDE_STREAM=0 pre-sets rs_set_side_stream(0) for a process that cannot call it: the profiling scripts in tools/ time every
        // kernel alone on one stream under rocprofv3
        const char* e = std::getenv("RS_SIDE_STREAM");
        s.mode = (e && e[0] == '0') ? 0 : 1;
    }
    return s.mode != 0;
}

// The pending switch (rs_stream_choice.h rs_switch_stream_choice says what is kept, released and recalled).
void switch_choice(rs_context* c) {
    rs_stream_choices& s = c->streams.choices;
    rs_stream_choice released[RS_STREAM_CHOICES_KEPT + 1];
    const int n = rs_switch_stream_choice(s, s.pending == RS_STREAMS_PENDING_AGAIN_FORGET, c->stream, c->streams.asked, released);
    for (int k = 0; k < n; k++) destroy_streams(released[k], true);
}

// Nothing is held, or plain stream i has not been asked for yet.  The first: the choice by measurement for the context's stream and
// preference.  Where that is not possible -- and from then on, until the next switch -- plain streams at the level the rule names, each
// made when it is first asked for.
void choose(rs_context* c, int i) {
    rs_internal_streams& s = c->streams;
    rs_stream_choice& cur = s.choices.current;
    if (s.choices.held == RS_STREAMS_HELD_NONE) {
        cur = rs_stream_choice{};
        cur.caller = c->stream; cur.levelKey = s.asked;
        // a stream that is being captured into a graph cannot be timed (the spins and the waits would end the capture): plain streams
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        if (c->stream && hipStreamIsCapturing(c->stream, &capturing) != hipSuccess) { (void)hipGetLastError(); capturing = hipStreamCaptureStatusNone; }
        if (capturing == hipStreamCaptureStatusNone && measure_streams(c->stream, s.asked, cur)) { s.choices.held = RS_STREAMS_HELD_MEASURED; return; }
        s.choices.held = RS_STREAMS_HELD_PLAIN;
    }
    int least = 0, greatest = 0, own = 0;
    cur.priority = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) (void)hipGetLastError();
    else {
        if (c->stream && hipStreamGetPriority(c->stream, &own) != hipSuccess) { (void)hipGetLastError(); own = 0; }
        cur.priority = rs_plain_stream_priority(least, greatest, s.asked, c->stream != nullptr, own);
    }
    int prio = cur.priority;
#ifdef RS_AUX_PRIORITY_ENV                              // measurement builds: RS_AUX_PRIORITIES=-1,-1,0,... per auxiliary stream
    if (const char* e = std::getenv("RS_AUX_PRIORITIES")) { for (int k = 0; k < i && e; k++) { e = std::strchr(e, ','); if (e) e++; } if (e) prio = std::atoi(e); }
#endif
    hipStream_t st = nullptr;
    if (hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio) != hipSuccess) { (void)hipGetLastError(); st = nullptr; s.mode = 0; }
    cur.stream[i] = st;
}
}  // namespace

// Auxiliary streams (asynchronous mode only): 0 carries GBuffer::render, 1 + k the primary-ray + RIS + shadow-ray kernels of every
// kChains-th frame (frames take the chains in turn, so that these chains of consecutive frames overlap each other
// as well as the passes of the frames before); for small launches, whose render is part of the chain's first launch, stream 0 is
// a third chain.
// Neither reads what the temporal / spatial passes of the previous frame write, so with the per-frame surface planes
// in four sets and the G-buffer planes in a ring of five they run next to those passes; the objects own the events
// that order them (rs_gbuffer, rs_restir).
// The auxiliary stream i of the current context, or nullptr when launches are synchronous (rs_set_sync(1): nothing to overlap)
// or the feature is off (rs_set_side_stream(0) / RS_SIDE_STREAM=0).
hipStream_t rs_aux_stream(int i) {
    rs_context* c = rs_ctx();
    rs_internal_streams& s = c->streams;
    if (c->sync || !streams_on(s) || i < 0 || i >= rs_context::kAux) return nullptr;
    if (s.choices.pending != RS_STREAMS_PENDING_NONE) switch_choice(c);
    if (!s.choices.current.stream[i]) choose(c, i);
    return (hipStream_t)s.choices.current.stream[i];
}
int rs_aux_streams_made(hipStream_t out[rs_context::kAux]) {
    const rs_stream_choice& cur = rs_ctx()->streams.choices.current;
    int n = 0;
    for (int i = 0; i < rs_context::kAux; i++) { out[i] = (hipStream_t)cur.stream[i]; n += out[i] != nullptr; }
    return n;
}
int rs_aux_synchronize() {
    for (void* st : rs_ctx()->streams.choices.current.stream) if (st) RS_HIP(hipStreamSynchronize((hipStream_t)st));
    return 0;
}
void rs_internal_streams_invalidate(rs_context* c, bool forget) {
    int& pending = c->streams.choices.pending;
    if (forget) pending = RS_STREAMS_PENDING_AGAIN_FORGET;
    else if (pending == RS_STREAMS_PENDING_NONE) pending = RS_STREAMS_PENDING_AGAIN;
}
void rs_internal_streams_set_mode(rs_context* c, bool on) { c->streams.mode = on ? 1 : 0; }
void rs_internal_streams_destroy(rs_context* c) {
    rs_stream_choices& s = c->streams.choices;
    destroy_streams(s.current, false);
    for (int k = 0; k < s.numKept; k++) destroy_streams(s.kept[k], false);
    s = rs_stream_choices{};
}

extern "C" {

// what the choice by measurement came to (for logs): the level of the three streams (-1 high / 0 normal / 1 low), the chosen triple's
// calibration time and the fastest time any candidate triple reached, in microseconds (0 / 0: not chosen by measurement -- none made yet,
// or the measurement failed and plain streams are in use)
int rs_internal_streams_info(int* priority, double* chosenUs, double* fastestUs) {
    const rs_stream_choice& cur = rs_ctx()->streams.choices.current;
    if (priority) *priority = cur.priority;
    if (chosenUs) *chosenUs = cur.chosenUs;
    if (fastestUs) *fastestUs = cur.fastestUs;
    return 0;
}
// Makes the choice again at the next overlapped launch: for a caller whose process has gained streams since the library chose (an
// ncclComm created after the first frames, a torch stream pool touched for the first time).  Waits for the library's streams.
int rs_choose_internal_streams_again(void) {
    RS_TRY(rs_synchronize());
    rs_internal_streams_invalidate(rs_ctx(), true);
    return 0;
}
// Makes the choice NOW (about 25 ms: spins on the caller's stream and on twelve candidate streams, waits for those streams only) instead of
// at the first overlapped launch -- for a caller that wants no such pause inside its first frame.  No-op when launches are synchronous,
// the side streams are off, or a choice for the current stream and preference is in force.
int rs_prepare_streams(void) {
    rs_ctx_scope scope(nullptr);
    (void)rs_aux_stream(0);
    return 0;
}
int rs_set_internal_stream_priority(int level) {
    rs_context* c = rs_ctx();
    if (level < -1 || level > 2) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_set_internal_stream_priority: -1 high, 0 normal, 1 low, 2 automatic");
    const bool changed = c->streams.asked != level;
    c->streams.asked = level;
    if (changed) { RS_TRY(rs_synchronize()); rs_internal_streams_invalidate(c, false); }
    return 0;
}

// Test hooks of rs_stream_choice.h (include/restir_hip.h), host only: no device, no context
static_assert(RS_AUX_STREAMS != 3 || (sizeof(rs_stream_choice) == 64 && sizeof(rs_stream_choices) == 336), "the sizes restir_amd/ctypes_structs.py mirrors");
static_assert(sizeof(rs_stream_choice_inputs) == 120 && sizeof(rs_stream_choice_plan) == 40, "the sizes restir_amd/ctypes_structs.py mirrors");
int rs_debug_plan_stream_choice(const rs_stream_choice_inputs* in, rs_stream_choice_plan* out) {
    if (!in || !out || in->asked < -1 || in->asked > 2) return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_plan_stream_choice: bad argument");
    out->numLevels = rs_stream_level_order(in->least, in->greatest, in->asked, in->callerHasStream != 0, in->callerPriority, out->order);
    for (int q = out->numLevels; q < 3; q++) out->order[q] = -1;
    const rs_stream_pick pick = rs_pick_streams(in->timesUs, out->order, out->numLevels);
    out->level = pick.level; out->skip = pick.skip; out->fastestUs = pick.fastest;
    out->plainPriority = rs_plain_stream_priority(in->least, in->greatest, in->asked, in->callerHasStream != 0, in->callerPriority);
    return 0;
}
int rs_debug_plan_stream_switch(rs_stream_choices* state, int forget, void* caller, int levelKey, rs_stream_choice* released, int* numReleased) {
    if (!state || !released || !numReleased || state->numKept < 0 || state->numKept > RS_STREAM_CHOICES_KEPT)
        return rs_fail(RS_ERR_INVALID_ARGUMENT, "rs_debug_plan_stream_switch: bad argument");
    *numReleased = rs_switch_stream_choice(*state, forget != 0, caller, levelKey, released);
    return 0;
}

}  // extern "C"
