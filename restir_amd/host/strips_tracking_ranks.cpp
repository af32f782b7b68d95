// strips_tracking_ranks.cpp -- light tracking (rs_restir_set_light_tracking) through the strip driver, three ranks carrying real data on
// ONE GPU: three host threads, each a rank with its own library context, stream, scene and tracked rs_restir, over the in-process
// stream-ordered transport of strips_loopback_transport.h, every driver with rs_strips_set_light_tracking(strips, 1).
//
// Before every frame from the second on, every rank applies the same edit to its scene's four lamps (rs_scene_set_emission): each has a
// material of its own, is switched off in some frames and back on in others, and is recoloured in between.  A frame of a rank:
// rs_strips_frame, rs_gbuffer_update, rs_strips_exchange_history, rs_strips_gather of the radiance.  Rank 0 renders every frame once more
// as a tracked full frame (rs_restir_direct) and compares, bit for bit,
//   * the gathered radiance after every frame,
//   * after rs_strips_exchange_history EVERY rank's which = 1 reservoirs and light ids -- all rows, not only the rank's own --
// for a still camera and for one that moves vertically (reprojection crosses the strip borders; a horizontal orbit would pass without
// the id rows in the history messages), 96 x 96; and with the moving camera once more at 70 x 99: strips of 33 rows of 70 pixels are no
// multiple of four pixels, so no plane's rows start or end on 16 bytes and the eight-plane launches of the history exchange (and the
// six-plane ones of the border rows) move ints instead of 16 bytes a thread.
//
//     strips_tracking_ranks [SECONDS]     the process ends itself after SECONDS (default 120)
#include <utility>

#include "strips_loopback_transport.h"

namespace {
using namespace loopback;

constexpr int kWorld = 3, kFrames = 6, kLamps = 4, kModes = 3;
#define CHECK(x) RANKS_CHECK(x)

std::atomic<int> mismatches{ 0 };

// all ranks meet here; what they wrote before is visible to all after
struct Barrier {
    std::mutex m; std::condition_variable cv; int waiting = 0, round = 0;
    void wait() {
        std::unique_lock<std::mutex> lock(m);
        const int r = round;
        if (++waiting == kWorld) { waiting = 0; round++; cv.notify_all(); }
        else cv.wait(lock, [&] { return round != r; });
    }
};
Barrier barrier;
// every rank's history after the exchange, for rank 0 to compare
std::vector<rs_reservoir> rankResv[kWorld];
std::vector<int> rankIds[kWorld];

// the test scene of the rank programs with a material per lamp, so that an edit can switch one lamp off and leave its neighbour lit
rs_scene* build_tracking_scene(int rank) {
    std::vector<float> v, n; std::vector<int> matIds; std::vector<rs_material> mats;
    ranks::make_scene(v, n, matIds, mats);
    const rs_material lamp = mats.back();
    for (int k = 1; k < kLamps; k++) mats.push_back(lamp);
    for (int k = 0; k < kLamps; k++) {
        const size_t t = matIds.size() - kLamps + (size_t)k;
        matIds[t] = 3 + k;
        // The lamps are single-sided and the shared scene's face the ceiling: they light nothing, and no reservoir would ever name one.
        // Turned over (second and third vertex swapped, normals down) they light the floor and the wall.
        for (int c = 0; c < 3; c++) std::swap(v[t * 9 + 3 + (size_t)c], v[t * 9 + 6 + (size_t)c]);
        for (int i = 0; i < 3; i++) { n[t * 9 + 3 * (size_t)i] = 0.f; n[t * 9 + 3 * (size_t)i + 1] = -1.f; n[t * 9 + 3 * (size_t)i + 2] = 0.f; }
    }
    const std::vector<float> uv(matIds.size() * 6, 0.f);
    rs_scene* scene = nullptr;
    CHECK(rs_scene_build((int)matIds.size(), v.data(), n.data(), uv.data(), matIds.data(), (int)mats.size(), mats.data(), &scene));
    return scene;
}
// frame f >= 1: lamp k is dark when (f + k) % 3 == 0 (at most two of the four at a time), else recoloured
void edit_lamps(int rank, rs_scene* scene, int frame) {
    int ids[kLamps]; float rad[kLamps * 3];
    for (int k = 0; k < kLamps; k++) {
        ids[k] = 3 + k;
        const bool dark = (frame + k) % 3 == 0;
        const float gain = 1.f + .5f * (float)((frame * 7 + k * 3) % 4);
        rad[3 * k] = dark ? 0.f : 14.f * gain; rad[3 * k + 1] = dark ? 0.f : 12.f; rad[3 * k + 2] = dark ? 0.f : 9.f / gain;
    }
    CHECK(rs_scene_set_emission(scene, kLamps, ids, rad));
}
void make_camera(rs_camera& cam, int TW, int TH, int frame, bool moving) {
    std::memset(&cam, 0, sizeof cam);
    cam.resolution[0] = TW; cam.resolution[1] = TH;
    cam.position[0] = moving ? .05f * frame : 0.f; cam.position[1] = 1.4f + (moving ? .25f * (float)(frame % 3 - 1) : 0.f); cam.position[2] = .8f;
    cam.rotation[0] = -90.f;
    cam.fov[1] = 28.f; cam.focalDist = 1.f;
}

void run_rank(int rank, Mailbox* box) {
    RANKS_HIP(hipSetDevice(0));
    rs_context* ctx = nullptr;
    CHECK(rs_context_create(0, &ctx));
    CHECK(rs_context_set_current(ctx));
    hipStream_t lib = nullptr;
    RANKS_HIP(hipStreamCreateWithFlags(&lib, hipStreamNonBlocking));
    CHECK(rs_set_stream(lib));
    CHECK(rs_set_sync(0));
    Endpoint ep{ box, rank };
    rs_transport t = transport_of(&ep);
    rs_comm* comm = nullptr;
    CHECK(rs_comm_create(&t, rank, kWorld, &comm));

    for (int mode = 0; mode < kModes; mode++) {
        const bool moving = mode >= 1;
        const int TW = mode == 2 ? 70 : 96, TH = mode == 2 ? 99 : 96;      // strips of 32 rows; of 33 rows of 70 pixels: nothing on 16 bytes
        const size_t px = (size_t)TW * TH;
        rs_scene* scene = build_tracking_scene(rank);              // (a fresh scene: the lamps as built)
        rs_strips* strips = nullptr;
        CHECK(rs_strips_create(comm, TW, TH, nullptr, &strips));
        CHECK(rs_strips_set_light_tracking(strips, 1));
        int y0 = 0, y1 = 0;
        CHECK(rs_strips_rows(strips, &y0, &y1));
        const int sets = rank == 0 ? 2 : 1;                        // rank 0: the strip's objects and a full-frame renderer of its own
        rs_gbuffer* g[2] = {}; rs_restir* r[2] = {}; float* img[2] = {};
        for (int k = 0; k < sets; k++) {
            CHECK(rs_gbuffer_create(TW, TH, &g[k])); CHECK(rs_restir_init(TW, TH, &r[k]));
            CHECK(rs_restir_set_light_tracking(r[k], 1));
            RANKS_HIP(hipMalloc((void**)&img[k], px * 12)); RANKS_HIP(hipMemset(img[k], 0, px * 12));
        }
        float* gathered = nullptr;
        RANKS_HIP(hipMalloc((void**)&gathered, px * 12)); RANKS_HIP(hipMemset(gathered, 0, px * 12));
        rankResv[rank].assign(px, rs_reservoir{}); rankIds[rank].assign(px, 0);
        bool same = true, someLight = false;
        for (int frame = 0; frame < kFrames; frame++) {
            rs_camera cam;
            make_camera(cam, TW, TH, frame, moving);
            CHECK(rs_camera_update(&cam));
            if (frame > 0) edit_lamps(rank, scene, frame);
            CHECK(rs_strips_frame(strips, r[0], scene, &cam, g[0], img[0], 0, frame, 3));
            CHECK(rs_gbuffer_update(g[0], &cam));
            CHECK(rs_strips_exchange_history(strips, r[0], g[0]));
            RANKS_HIP(hipMemcpyAsync(gathered + (size_t)y0 * TW * 3, img[0] + (size_t)y0 * TW * 3, (size_t)(y1 - y0) * TW * 12, hipMemcpyDeviceToDevice, lib));
            CHECK(rs_strips_gather(strips, gathered, 12, 0));
            CHECK(rs_restir_download(r[0], 1, rankResv[rank].data()));
            CHECK(rs_restir_download_light_ids(r[0], 1, rankIds[rank].data()));
            barrier.wait();
            if (rank == 0) {
                CHECK(rs_gbuffer_render(g[1], scene, &cam));
                CHECK(rs_restir_direct(r[1], scene, &cam, g[1], img[1], 0, frame, 3));
                CHECK(rs_gbuffer_update(g[1], &cam));
                CHECK(rs_synchronize());
                std::vector<float> x(3 * px), y(3 * px);
                RANKS_HIP(hipMemcpy(x.data(), gathered, px * 12, hipMemcpyDeviceToHost));
                RANKS_HIP(hipMemcpy(y.data(), img[1], px * 12, hipMemcpyDeviceToHost));
                double sum = 0; for (float f : y) sum += f;
                if (std::memcmp(x.data(), y.data(), px * 12) != 0 || !(sum > 0)) {
                    size_t bad = 0; for (size_t i = 0; i < x.size(); i++) bad += std::memcmp(&x[i], &y[i], 4) != 0;
                    std::fprintf(stderr, "mode %d, frame %d: gathered strips differ from the tracked full frame in %zu values (sum %g)\n", mode, frame, bad, sum);
                    same = false;
                }
                std::vector<rs_reservoir> refResv(px); std::vector<int> refIds(px);
                CHECK(rs_restir_download(r[1], 1, refResv.data()));
                CHECK(rs_restir_download_light_ids(r[1], 1, refIds.data()));
                for (int id : refIds) someLight = someLight || id >= 0;
                for (int k = 0; k < kWorld; k++) {
                    size_t badResv = 0, badIds = 0;
                    for (size_t i = 0; i < px; i++) {
                        const rs_reservoir &a = rankResv[k][i], &b = refResv[i];
                        badResv += std::memcmp(a.Li, b.Li, 12) != 0 || std::memcmp(a.wi, b.wi, 12) != 0 || std::memcmp(&a.dist, &b.dist, 4) != 0 ||
                                   std::memcmp(&a.weight, &b.weight, 4) != 0 || a.numSamples != b.numSamples;
                        badIds += rankIds[k][i] != refIds[i];
                    }
                    if (badResv || badIds) {
                        std::fprintf(stderr, "mode %d, frame %d: rank %d's history differs from the tracked full frame's in %zu reservoirs and %zu light ids\n", mode, frame, k, badResv, badIds);
                        same = false;
                    }
                }
            }
            barrier.wait();                                        // (rank 0 has read the other ranks' arrays)
        }
        CHECK(rs_synchronize());
        RANKS_HIP(hipStreamSynchronize(lib));
        if (rank == 0) {
            if (!someLight) { std::fprintf(stderr, "mode %d: no reservoir ever named a light\n", mode); same = false; }
            std::printf("world %d, %d x %d, %s camera, light tracking, lamps edited every frame: gathered strips, history reservoirs and light ids of every rank == full frame over %d frames: %s\n",
                        kWorld, TW, TH, moving ? "vertically moving" : "still", kFrames, same ? "True" : "False");
            std::fflush(stdout);
            if (!same) mismatches++;
        }
        CHECK(rs_strips_destroy(strips));
        for (int k = 0; k < sets; k++) { rs_restir_free(r[k]); rs_gbuffer_destroy(g[k]); (void)hipFree(img[k]); }
        (void)hipFree(gathered);
        rs_scene_destroy(scene);
    }
    rs_comm_destroy(comm);
    (void)rs_set_stream(nullptr);
    (void)hipStreamDestroy(lib);
    (void)rs_context_set_current(nullptr);
    (void)rs_context_destroy(ctx);
}

}  // namespace

int main(int argc, char** argv) {
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices < 1) { std::fprintf(stderr, "no GPU\n"); return 1; }
    ranks::start_watchdog(argc > 1 ? std::atoi(argv[1]) : 120);
    static Mailbox box;
    if (hipSetDevice(0) != hipSuccess) return 1;
    if (!mailbox_init(box, kWorld)) return 1;
    std::vector<std::thread> threads;
    for (int k = 0; k < kWorld; k++) threads.emplace_back(run_rank, k, &box);
    for (auto& t : threads) t.join();
    if (mismatches) { std::fprintf(stderr, "strips_tracking_ranks: %d mode(s) with mismatches\n", mismatches.load()); return 1; }
    std::printf("strips_tracking_ranks ok (%d ranks)\n", kWorld);
    return 0;
}
