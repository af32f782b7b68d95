// rs_stream_choice.h -- the device-free half of the library's internal streams (internal_streams.hip; its head says why they are chosen
// by measurement): which priority levels are measured and in what order, which measured triple is taken, the priority of plain streams
// when nothing can be measured, and what becomes of a choice when the caller's stream or the preference changes -- as functions of plain
// integers, doubles and opaque handles (include/restir_hip.h).  Nothing here touches the device, a context or a global:
// internal_streams.hip asks these functions and acts on what they return, and rs_debug_plan_stream_choice / _switch hand them to a test
// that has no device.
#pragma once

#include "../../include/restir_hip.h"

// Levels: 0 high, 1 normal, 2 low.  The priority a level's streams are made at, for the device's range [greatest, least].
inline int rs_stream_level_priority(int level, int least, int greatest) { return level == 0 ? greatest : level == 2 ? least : 0; }

// The levels that are measured, preferred first: high, normal, low -- or the asked level first when low or normal is asked for; a level
// the range does not offer is absent.  Returns their number.
// Not the caller's own level: there the library's streams share the level's four hardware queues with the caller's stream and whatever
// else the process keeps at it, and the eight-round test does not always see it (RCCL in the process, ordinary caller stream, normal
// level: a calibration time as good as any and a config 5 frame of 2.14 ms instead of 1.79) -- unless that would leave no level.  The
// default stream is no such caller: it holds one queue of the normal level, and next to it the normal level measures as well as any.
inline int rs_stream_level_order(int least, int greatest, int asked, bool callerHasStream, int callerPriority, int order[3]) {
    const bool high = greatest < 0, low = least > 0;
    int n = 0;
    if (asked == 1) { if (low) order[n++] = 2; order[n++] = 1; if (high) order[n++] = 0; }
    else if (asked == 0) { order[n++] = 1; if (high) order[n++] = 0; if (low) order[n++] = 2; }
    else { if (high) order[n++] = 0; order[n++] = 1; if (low) order[n++] = 2; }
    if (callerHasStream) {
        int m = 0;
        for (int q = 0; q < n; q++) if (rs_stream_level_priority(order[q], least, greatest) != callerPriority) order[m++] = order[q];
        if (m > 0) n = m;
    }
    return n;
}

// the best triple of a level is taken when it is within 8 % of the fastest triple of any level: levels that measure equal are told
// apart by the preference, not by the noise of one run
constexpr double kStreamChoiceWithin = 1.08;

// t[level][skip]: the time of the level's triple "all four candidates but `skip`" (levels outside the order are not read).  fastest is
// taken over every measured level; per level the lowest time wins, the lowest index among equals; the first level in the order whose best
// is within kStreamChoiceWithin of the fastest is chosen.  A negative time (a measurement that failed or was never made): nothing is chosen.
struct rs_stream_pick { int level, skip; double fastest; };
inline rs_stream_pick rs_pick_streams(const double t[3][4], const int* order, int n) {
    rs_stream_pick p{ -1, -1, 1e30 };
    for (int q = 0; q < n; q++)
        for (int i = 0; i < 4; i++) {
            if (t[order[q]][i] < 0) return p;
            p.fastest = t[order[q]][i] < p.fastest ? t[order[q]][i] : p.fastest;
        }
    for (int q = 0; q < n && p.level < 0; q++) {
        int best = 0;
        for (int i = 1; i < 4; i++) if (t[order[q]][i] < t[order[q]][best]) best = i;
        if (t[order[q]][best] <= p.fastest * kStreamChoiceWithin) { p.level = order[q]; p.skip = best; }
    }
    return p;
}

// The priority of plain streams: the high level unless the caller's stream is in it (or the range has none), else normal -- or the asked
// level, unless it is the caller stream's own.
inline int rs_plain_stream_priority(int least, int greatest, int asked, bool callerHasStream, int callerPriority) {
    const int own = callerHasStream ? callerPriority : 0;
    int want = (greatest < 0 && own > greatest) ? greatest : 0;
    if (asked != 2) {
        const int level = asked < 0 ? greatest : asked > 0 ? least : 0;
        if (level != own || !callerHasStream) want = level;
    }
    return want;
}

// The first use after rs_set_stream handed the library another stream, rs_set_internal_stream_priority another preference or
// rs_choose_internal_streams_again asked for it (`forget`): the streams are chosen for (caller, levelKey).  The old ones are idle (every
// such call waited for them).  Measured ones are KEPT under the stream and key they were chosen for -- a caller that alternates between two
// streams measures each once, not at every switch -- at most RS_STREAM_CHOICES_KEPT of them: a fifth pushes the oldest out, and that
// BEFORE the kept ones are searched, so with a full list a switch back to the oldest kept caller measures again.  Plain ones are released,
// and with `forget` so is every kept choice.  A kept choice for (caller, levelKey) then becomes current and leaves the list; otherwise
// nothing is held.  Returns how many choices were written to released[RS_STREAM_CHOICES_KEPT + 1]: the caller destroys their streams.
inline int rs_switch_stream_choice(rs_stream_choices& s, bool forget, void* caller, int levelKey, rs_stream_choice* released) {
    int n = 0;
    auto drop_kept = [&](int k) { for (int j = k; j + 1 < s.numKept; j++) s.kept[j] = s.kept[j + 1]; s.numKept--; };
    if (s.held == RS_STREAMS_HELD_MEASURED && !forget) {
        if (s.numKept >= RS_STREAM_CHOICES_KEPT) { released[n++] = s.kept[0]; drop_kept(0); }
        s.kept[s.numKept++] = s.current;
    }
    else {
        if (s.held != RS_STREAMS_HELD_NONE) released[n++] = s.current;
        if (forget) { for (int k = 0; k < s.numKept; k++) released[n++] = s.kept[k]; s.numKept = 0; }
    }
    s.current = rs_stream_choice{};
    s.held = RS_STREAMS_HELD_NONE; s.pending = RS_STREAMS_PENDING_NONE;
    for (int k = 0; k < s.numKept; k++)
        if (s.kept[k].caller == caller && s.kept[k].levelKey == levelKey) {
            s.current = s.kept[k]; s.held = RS_STREAMS_HELD_MEASURED;
            drop_kept(k);
            break;
        }
    return n;
}

// Everything rs_context keeps about its internal streams (internal_streams.hip owns it).
struct rs_internal_streams {
    rs_stream_choices choices{};
    int asked = 2;                        // rs_set_internal_stream_priority: -1 high / 0 normal / 1 low first, 2 automatic; the level key of a choice
    int mode = -1;                        // -1: not decided yet (RS_SIDE_STREAM); 0 off; 1 on
};
