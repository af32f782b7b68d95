// tools/models/stream_choice_plan.cpp -- the host decisions of the library's internal streams on their edge cases, as a stand-alone host
// program for AddressSanitizer + UBSan: the level order, the pick among measured times, the priority of plain streams and the switch of
// choices (restir_amd/csrc/rs_stream_choice.h, the functions internal_streams.hip acts on), with the order in an array of exactly its
// length and the released choices in an array of exactly the most the contract allows.  No device is touched and nothing of the library
// is linked.  Built and run as tools/models/primary_cut_plan.cpp, from restir_amd/csrc:
//   hipcc -O1 -g -std=c++17 -ffp-contract=off -x hip --offload-arch=gfx950 --cuda-host-only -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-omit-frame-pointer -I. -c ../../tools/models/stream_choice_plan.cpp -o /tmp/stream_choice_plan.o
//   hipcc -fsanitize=address,undefined /tmp/stream_choice_plan.o -o /tmp/stream_choice_plan
//   /tmp/stream_choice_plan        (prints "stream_choice_plan: ok"; a failed check or a sanitizer report ends it with a non-zero status)
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "rs_stream_choice.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "stream_choice_plan.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

namespace {

constexpr int HIGH = 0, NORMAL = 1, LOW = 2;

// the order in a heap array of exactly three ints
std::vector<int> order(int least, int greatest, int asked, bool hasStream, int prio) {
    std::unique_ptr<int[]> o(new int[3]);
    const int n = rs_stream_level_order(least, greatest, asked, hasStream, prio, o.get());
    CHECK(n >= 1 && n <= 3);
    return std::vector<int>(o.get(), o.get() + n);
}
using V = std::vector<int>;

void orders() {
    CHECK((order(1, -1, 2, false, 0) == V{ HIGH, NORMAL, LOW }) && (order(1, -1, -1, false, 0) == V{ HIGH, NORMAL, LOW }));
    CHECK((order(1, -1, 1, false, 0) == V{ LOW, NORMAL, HIGH }) && (order(1, -1, 0, false, 0) == V{ NORMAL, HIGH, LOW }));
    CHECK((order(0, -1, 2, false, 0) == V{ HIGH, NORMAL }) && (order(0, -1, 1, false, 0) == V{ NORMAL, HIGH }));
    CHECK((order(1, 0, 2, false, 0) == V{ NORMAL, LOW }) && (order(1, 0, 1, false, 0) == V{ LOW, NORMAL }));
    CHECK((order(0, 0, 2, false, 0) == V{ NORMAL }) && (order(0, 0, 1, false, 0) == V{ NORMAL }));
    CHECK((order(1, -1, 2, true, -1) == V{ NORMAL, LOW }) && (order(1, -1, 2, true, 0) == V{ HIGH, LOW }) && (order(1, -1, 2, true, 1) == V{ HIGH, NORMAL }));
    CHECK((order(0, 0, 2, true, 0) == V{ NORMAL }));                     // the caller on the only level: it stays
    CHECK((order(1, -1, 2, false, -1) == V{ HIGH, NORMAL, LOW }));       // the default stream removes nothing, whatever priority is passed
    CHECK((order(0, -1, 2, true, 1) == V{ HIGH, NORMAL }));
}

// the times in a heap array of exactly 3 x 4 doubles; rows that are not measured are NaN
struct Times {
    std::unique_ptr<double[]> t{ new double[12] };
    Times(std::initializer_list<double> high, std::initializer_list<double> normal, std::initializer_list<double> low) {
        int r = 0;
        for (const auto& row : { high, normal, low }) {
            int k = 0;
            for (int i = 0; i < 4; i++) t[r * 4 + i] = std::numeric_limits<double>::quiet_NaN();
            for (double x : row) t[r * 4 + k++] = x;
            CHECK(k == 0 || k == 4);
            r++;
        }
    }
    rs_stream_pick pick(const V& o) const { return rs_pick_streams(reinterpret_cast<const double(*)[4]>(t.get()), o.data(), (int)o.size()); }
};
bool is(const rs_stream_pick& p, int level, int skip, double fastest) { return p.level == level && p.skip == skip && p.fastest == fastest; }

void picks() {
    const V all{ HIGH, NORMAL, LOW };
    CHECK(is(Times({ 120, 100.0 * 1.08, 130, 140 }, { 100, 101, 102, 103 }, { 300, 300, 300, 300 }).pick(all), HIGH, 1, 100));
    CHECK(is(Times({ 120, 100.0 * 1.0801, 130, 140 }, { 103, 101, 100, 102 }, { 300, 300, 300, 300 }).pick(all), NORMAL, 2, 100));
    CHECK(is(Times({ 7, 5, 5, 5 }, { 9, 9, 9, 9 }, { 9, 9, 9, 9 }).pick(all), HIGH, 1, 5));
    CHECK(is(Times({ 200, 200, 200, 200 }, { 110, 107, 109, 120 }, { 130, 100, 130, 130 }).pick(all), NORMAL, 1, 100));
    CHECK(is(Times({ 200, 200, 200, 200 }, { 110, 109, 109, 120 }, { 130, 100, 130, 130 }).pick(all), LOW, 1, 100));
    CHECK(is(Times({ 200, 200, 200, 200 }, { 110, 109, 109, 120 }, { 130, 100, 130, 130 }).pick({ LOW, NORMAL, HIGH }), LOW, 1, 100));
    for (int at = 0; at < 12; at++) {
        Times t({ 100, 100, 100, 100 }, { 100, 100, 100, 100 }, { 100, 100, 100, 100 });
        t.t[at] = -1;
        CHECK(t.pick(all).level == -1 && t.pick(all).skip == -1);
    }
    CHECK(is(Times({}, { 50, 40, 60, 70 }, { 45, 45, 45, 45 }).pick({ NORMAL, LOW }), NORMAL, 1, 40));
    CHECK(is(Times({ 50, 40, 60, 30 }, {}, { 45, 45, 45, 45 }).pick({ HIGH, LOW }), HIGH, 3, 30));
    CHECK(is(Times({}, { 3, 2, 1, 4 }, {}).pick({ NORMAL }), NORMAL, 2, 1));
    CHECK(is(Times({ -1, -1, -1, -1 }, { 3, 2, 1, 4 }, { -1, -1, -1, -1 }).pick({ NORMAL }), NORMAL, 2, 1));
    CHECK(Times({}, {}, {}).pick({}).level == -1);                       // no level at all
}

void plain_priorities() {
    CHECK(rs_plain_stream_priority(1, -1, 2, false, 0) == -1 && rs_plain_stream_priority(1, -1, 2, true, 0) == -1 && rs_plain_stream_priority(1, -1, 2, true, 1) == -1);
    CHECK(rs_plain_stream_priority(1, -1, 2, true, -1) == 0 && rs_plain_stream_priority(1, 0, 2, false, 0) == 0 && rs_plain_stream_priority(0, 0, 2, true, 0) == 0);
    CHECK(rs_plain_stream_priority(1, -1, 1, false, 0) == 1 && rs_plain_stream_priority(1, -1, 0, false, 0) == 0 && rs_plain_stream_priority(1, -1, -1, true, 0) == -1);
    CHECK(rs_plain_stream_priority(0, -1, 1, false, 0) == 0 && rs_plain_stream_priority(1, 0, -1, false, 0) == 0);
    CHECK(rs_plain_stream_priority(1, -1, 0, true, 0) == -1 && rs_plain_stream_priority(1, -1, 1, true, 1) == -1 && rs_plain_stream_priority(1, -1, -1, true, -1) == 0);
    CHECK(rs_plain_stream_priority(1, -1, 0, false, 7) == 0);             // (the default stream's priority is not read)
}

// the switch as internal_streams.hip drives it: invented handles, the released choices in a heap array of exactly the contract's size
struct Streams {
    rs_stream_choices s{};
    char pool[4096];                                 // handles point into it and are never followed
    int made = 0;
    std::vector<void*> released;
    bool visit(void* caller, int key, bool forget = false, bool plain = false) {
        std::unique_ptr<rs_stream_choice[]> out(new rs_stream_choice[RS_STREAM_CHOICES_KEPT + 1]);
        const int n = rs_switch_stream_choice(s, forget, caller, key, out.get());
        CHECK(n >= 0 && n <= (forget ? RS_STREAM_CHOICES_KEPT + 1 : 1));
        CHECK(s.pending == RS_STREAMS_PENDING_NONE && s.numKept >= 0 && s.numKept <= RS_STREAM_CHOICES_KEPT);
        for (int k = 0; k < n; k++) for (void* h : out[k].stream) if (h) released.push_back(h);
        if (s.held == RS_STREAMS_HELD_MEASURED) { CHECK(s.current.caller == caller && s.current.levelKey == key); return true; }
        CHECK(s.held == RS_STREAMS_HELD_NONE);
        s.current.caller = caller; s.current.levelKey = key;
        for (int k = 0; k < (plain ? 1 : RS_AUX_STREAMS); k++) { CHECK(made < (int)sizeof pool); s.current.stream[k] = pool + made++; }
        s.current.chosenUs = s.current.fastestUs = plain ? 0.0 : (double)made;
        s.held = plain ? RS_STREAMS_HELD_PLAIN : RS_STREAMS_HELD_MEASURED;
        return false;
    }
    void every_handle_in_one_place() {
        std::vector<int> count((size_t)made, 0);
        auto note = [&](const rs_stream_choice& c) { for (void* h : c.stream) if (h) count[(size_t)((char*)h - pool)]++; };
        note(s.current);
        for (int k = 0; k < s.numKept; k++) note(s.kept[k]);
        for (void* h : released) count[(size_t)((char*)h - pool)]++;
        for (int c : count) CHECK(c == 1);
    }
};

void switches() {
    char names[8];
    void *A = names, *B = names + 1, *C = names + 2, *D = names + 3, *E = names + 4, *F = names + 5;
    {   // A, B, A, B, A: two measurements, then recalls that release nothing
        Streams m;
        void* callers[5] = { A, B, A, B, A };
        for (int step = 0; step < 5; step++) { CHECK(m.visit(callers[step], 2) == (step >= 2)); CHECK(m.released.empty()); }
        CHECK(m.made == 6 && m.s.numKept == 1 && m.s.kept[0].caller == B);
        m.every_handle_in_one_place();
    }
    {   // five callers: nothing released; the fifth kept choice releases exactly the oldest
        Streams m;
        for (void* c : { A, B, C, D, E }) CHECK(!m.visit(c, 2));
        CHECK(m.released.empty() && m.s.numKept == 4 && m.s.kept[0].caller == A);
        CHECK(!m.visit(F, 2) && m.released.size() == 3 && m.released[0] == m.pool && m.s.kept[0].caller == B && m.s.kept[3].caller == E);
        // the full list: the oldest is released before it is looked up, so a switch back to it measures again
        CHECK(!m.visit(B, 2) && m.released.size() == 6 && m.released[3] == m.pool + 3 && m.s.kept[0].caller == C && m.s.kept[3].caller == F);
        m.every_handle_in_one_place();
        // forget with a full list: the current choice and the four kept ones
        CHECK(!m.visit(C, 2, true) && m.released.size() == 6 + 15 && m.s.numKept == 0);
        m.every_handle_in_one_place();
    }
    {   // plain streams are released, not kept; another level key is another choice
        Streams m;
        CHECK(!m.visit(A, 2) && !m.visit(B, 2, false, true) && m.s.numKept == 1);
        CHECK(m.visit(A, 2) && m.released.size() == 1 && m.s.numKept == 0);
        CHECK(!m.visit(A, 1) && m.s.numKept == 1 && m.visit(A, 2) && m.visit(A, 1) && m.released.size() == 1);
        CHECK(!m.visit(nullptr, 1) && m.visit(A, 1));                    // the default stream is a caller like any other
        m.every_handle_in_one_place();
    }
    {   // nothing held: nothing released, with or without forget
        Streams m;
        rs_stream_choice none[1];
        CHECK(rs_switch_stream_choice(m.s, true, A, 2, none) == 0 && rs_switch_stream_choice(m.s, false, A, 2, none) == 0);
    }
    unsigned x = 12345u;                             // a few hundred sequences
    auto rnd = [&](unsigned n) { x = x * 1664525u + 1013904223u; return (x >> 16) % n; };
    for (int seq = 0; seq < 300; seq++) {
        Streams m;
        const int steps = 1 + (int)rnd(40);
        for (int i = 0; i < steps; i++) { m.visit(names + rnd(7), rnd(4) ? 2 : 1, rnd(10) == 0, rnd(5) == 0); m.every_handle_in_one_place(); }
    }
}

}  // namespace

int main() {
    orders();
    picks();
    plain_priorities();
    switches();
    std::printf("stream_choice_plan: ok\n");
    return 0;
}
