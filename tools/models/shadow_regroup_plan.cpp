// tools/models/shadow_regroup_plan.cpp -- the device-free functions of the regrouped shadow-ray kernel (restir_amd/csrc/rs_shadow_regroup.h:
// shadow_bin and the slot plan) on their edge cases, as a stand-alone host program for AddressSanitizer + UBSan: the cases of
// tests/test_shadow_regroup_plan.py, every array allocated at exactly the size the contract promises.  The header includes nothing of HIP,
// so a host compiler is enough; no device is touched and nothing of the library is linked.  From restir_amd/csrc:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I. \
//       ../../tools/models/shadow_regroup_plan.cpp -o /tmp/shadow_regroup_plan
//   /tmp/shadow_regroup_plan        (prints "shadow_regroup_plan: ok"; a failed check or a sanitizer report ends it with a non-zero status)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "rs_shadow_regroup.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "shadow_regroup_plan.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

namespace {

void bins() {
    const float lo[3] = { -1.f, 0.f, 2.f }, hi[3] = { 2.f, 4.f, 14.f };          // a diagonal of 13
    const float k = shadow_bins_over_extent(lo, hi);
    CHECK(k == 64.f / 13.f);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(shadow_bin(0.f, k) == 0 && shadow_bin(-0.f, k) == 0 && shadow_bin(std::numeric_limits<float>::denorm_min(), k) == 0);
    CHECK(shadow_bin(-1.f, k) == 0 && shadow_bin(-1e30f, k) == 0 && shadow_bin(-inf, k) == 0);
    CHECK(shadow_bin(13.f, k) == 63 && shadow_bin(26.f, k) == 63 && shadow_bin(1e10f, k) == 63 && shadow_bin(3.4e38f, k) == 63);
    CHECK(shadow_bin(inf, k) == 63 && shadow_bin(nan, k) == 63 && shadow_bin(-nan, k) == 63);
    // bin edges with a scale that is exact: 4 bins per unit of length
    for (int e : { 1, 2, 7, 31, 62, 63 }) {
        const float edge = (float)e * 0.25f;
        CHECK(shadow_bin(edge, 4.f) == e && shadow_bin(std::nextafter(edge, 0.f), 4.f) == e - 1);
    }
    CHECK(shadow_bin(15.75f, 4.f) == 63 && shadow_bin(std::nextafter(15.75f, 0.f), 4.f) == 62 && shadow_bin(16.f, 4.f) == 63);
    // a degenerate root box: the scale is infinite, 0 * inf is a NaN
    const float p[3] = { 1.f, 1.f, 1.f };
    const float deg = shadow_bins_over_extent(p, p);
    CHECK(std::isinf(deg) && shadow_bin(0.f, deg) == 63 && shadow_bin(1.f, deg) == 63 && shadow_bin(-1.f, deg) == 0);
    // monotone and in range
    std::mt19937 rng(7);
    std::vector<float> len(100000);
    std::uniform_real_distribution<float> u(-2.f, 20.f);
    for (float& v : len) v = u(rng);
    len[0] = 1e10f; len[1] = inf; len[2] = 0.f;
    std::sort(len.begin(), len.end());
    int last = 0;
    for (float v : len) { const int b = shadow_bin(v, k); CHECK(b >= 0 && b < kShadowBins && b >= last); last = b; }
    CHECK(last == 63);
}

// the plan of `lanes` (exactly lanes.size() ints) against a restatement: rays sorted by descending bin
void plan(const std::vector<int>& lanes) {
    std::vector<int> first(kShadowBins, -7);
    const int count = rs_plan_shadow_slots(lanes.data(), (int)lanes.size(), first.data());
    std::vector<int> act;
    for (int b : lanes) if (b >= 0) act.push_back(b);
    CHECK(count == (int)act.size() && count <= (int)lanes.size());
    std::sort(act.begin(), act.end(), [](int a, int b) { return a > b; });
    for (int b = 0; b < kShadowBins; b++) {
        const int want = (int)(std::lower_bound(act.begin(), act.end(), b, [](int v, int bin) { return v > bin; }) - act.begin());
        CHECK(first[(size_t)b] == want);
    }
    // handing out first[bin]++ in arrival order: a permutation of 0 .. count - 1, descending in bin
    std::vector<int> next = first, binOfSlot((size_t)count, -1);
    for (int b : lanes) if (b >= 0) { const int s = next[(size_t)b]++; CHECK(s >= 0 && s < count && binOfSlot[(size_t)s] < 0); binOfSlot[(size_t)s] = b; }
    for (int s = 1; s < count; s++) CHECK(binOfSlot[(size_t)s] <= binOfSlot[(size_t)s - 1]);
}

void plans() {
    plan({});
    plan(std::vector<int>(256, -1));
    { std::vector<int> v(256, -1); v[200] = 17; plan(v); }
    plan(std::vector<int>(256, 0)); plan(std::vector<int>(256, 63)); plan(std::vector<int>(256, 31));
    { std::vector<int> v(256); for (int i = 0; i < 256; i++) v[(size_t)i] = i % 64; plan(v); }
    { std::vector<int> v(256); for (int i = 0; i < 256; i++) v[(size_t)i] = (i * 37) % 64; plan(v); }
    for (int n : { 63, 64, 65, 255 }) { std::vector<int> v(256, -1); for (int i = 0; i < n; i++) v[(size_t)((i * 101) % 256)] = (i * 13) % 64; plan(v); }
    std::mt19937 rng(11);
    for (int c = 0; c < 300; c++) {
        std::vector<int> v(256);
        const int spread = 1 + (int)(rng() % 64u), p = (int)(rng() % 101u);
        for (int& b : v) b = (int)(rng() % 100u) < p ? (int)(rng() % (unsigned)spread) + (int)(rng() % (unsigned)(65 - spread)) : -1;
        plan(v);
    }
}

}  // namespace

int main() {
    bins();
    plans();
    std::printf("shadow_regroup_plan: ok\n");
    return 0;
}
