// rs_frame_plan.h -- what a phase-A call of ReSTIRDirect launches, and where: every decision between the call's argument checks and its
// first event, as one function of plain integers (rs_phase_a_inputs -> rs_phase_a_plan, include/restir_hip.h).  Nothing here touches
// the device, a context or a global: restir.hip phase_a_impl gathers the inputs, asks for the plan and launches from its fields, and
// rs_debug_phase_a_plan hands the same function to a test that has no device.
#pragma once

#include "../../include/restir_hip.h"

// (RS_AUX_STREAMS, RS_SPLIT_SMALL_ROUNDS: the build's settings, with their defaults in rs_internal.h, which includes this header)
constexpr long long kSmallLaunchWaves = 3 * 8192;   // three rounds of the chip's 8 192 wave slots (256 CUs x 4 SIMDs x 8 waves)
constexpr long long kSplitSmallWaves = (long long)RS_SPLIT_SMALL_ROUNDS * 8192;   // launches below this many waves split their heavy tiles also when other kernels run next to them
constexpr long long kFuseMinWaves = kSmallLaunchWaves;     // three rounds of the chip's 8 192 wave slots (256 CUs x 4 SIMDs x 8 waves)
constexpr int kPlanChains = 2, kPlanSmallChains = RS_AUX_STREAMS;   // rs_restir::kChains / kSmallChains
constexpr int kRisLdsLights = 1024;
constexpr int kRisAliasLdsLights = 16384;        // alias records only: 128 KB of the CU's 160 KB at most

// Frames at which the measured launch choice takes its time stamps: two launches until kTuneB, one fused launch from there to kTuneD; the
// first span is frames kTuneA..kTuneB, the second kTuneC..kTuneD -- twelve frames each, and the four frames after every switch are not
// timed: chains run up to four frames ahead of the library stream, so the frames around a switch carry the other form's kernels next to
// them.  (Rounds 1-5 timed 2..8 against 8..14: on the Bistro-class scene, where the forms differ by 18 %, one run in four took the
// slower one -- 2.10 instead of 1.78 ms per frame, profiles/r06_fuse_tuner_flips.log.)
constexpr int kTuneA = 6, kTuneB = 18, kTuneC = 22, kTuneD = 34;
// the form a frame the measurement applies to takes: the decided one, or the one whose span the measurement is in
inline bool rs_tuned_fuse(int choice, int frame) { return choice >= 0 ? choice == 1 : (frame >= kTuneB && frame < kTuneD); }

// waves of a closest-hit launch over tilesX x tilesY blocks of four tiles
inline long long rs_launch_waves(int tilesX, int tilesY) { return (long long)tilesX * tilesY * 4; }

// The mode rs_tile_split_prepare (rs_internal.h) is given for a closest-hit launch of `waves` waves; alone: nothing runs next to it
// (synchronous mode, per-pass timing, one frame at a time).
inline int rs_split_mode(bool alone, long long waves) { return alone ? 1 : (waves < kSplitSmallWaves ? 2 : 0); }

inline void rs_plan_phase_a(const rs_phase_a_inputs& in, rs_phase_a_plan& p) {
    const bool async = in.async != 0, rows = in.y1 > in.y0, first = in.phaseACalls == 0;
    const bool parityStreams = in.chainStreams == 2;
    p.tilesX = (in.width + 31) / 32;
    p.tilesY = (rows ? in.y1 - in.y0 + 7 : 0) / 8;
    // A render of this frame that rs_gbuffer_render_rows deferred (asynchronous mode) can be launched here, in ONE launch with the
    // primary rays (k_gbuffer_primary): same scene and camera, rows that contain the rows shaded here.
    //  * A launch that fills the chip at least three times over: ~5 % less work than two launches, longer waves; the frame period is
    //    measured both ways once per scene and the faster form kept (full 1080p frame: the fused launch, by 0.5 %).
    //  * A smaller launch -- a strip -- lasts as long as its slowest wave, and what bounds its frame rate is the length of the chain
    //    primary rays -> RIS -> shadow rays over the number of chains in flight.  With two chains the fused launch loses (its slowest
    //    wave: 0.25 ms against 0.18 on a 1/8 strip), but it leaves the render's stream idle, and with that stream as a THIRD chain
    //    it wins: 8 strips of 1080p 5.96x -> 6.5x (rs_set_stream_plan(-1, 0, -1): two chains and a separate render).
    // Whenever the launch is fused the frame's chain is one of three (a full frame gains another 0.9 % from the third).
    const bool fusable = async && in.fuseMode != 0 && rows && in.deferredValid && in.deferredMatches && in.deferredY0 <= in.y0 && in.deferredY1 >= in.y1;
    const bool large = fusable && rs_launch_waves(p.tilesX, (in.deferredY1 - in.deferredY0 + 7) / 8) >= kFuseMinWaves;
    const bool small = fusable && !large && in.smallChains && parityStreams && in.fuseMode == 3 && first;
    bool fuse = fusable && (small || large || in.fuseMode == 2);
    // (with a denoise stream the render's own stream is that stream: a separate render would queue behind the previous frame's filter)
    const bool denoiseStream = async && in.denoiseStream;
    p.tuneCounted = fuse && large && in.fuseMode == 3 && !denoiseStream;        // measured choice (end_frame advances the measurement)
    if (p.tuneCounted) fuse = rs_tuned_fuse(in.tuneChoice, in.tuneFrame);
    p.fuse = fuse;
    p.fusedTilesY = fuse ? (in.deferredY1 - in.deferredY0 + 3) / 4 : 0;        // 8x4-pixel tiles: two rays per pixel fill the wave
    // A frame whose render request was answered from retained planes (rs_gbuffer_render_rows) launched nothing on the render's stream
    // either: it is idle for the same reason, and the frame's chain is one of three as well.  (RS_REUSE_CHAINS=2: A/B switch, two chains.)
    const bool reused = async && in.reusedFrame && !in.deferredValid && !denoiseStream && rows;
    const bool three = (fuse || (reused && in.reusedThree)) && parityStreams && first;
    // The measured choice compares spans of consecutive frames that each had a render to fuse: a reused frame in between is not
    // one of them, so a measurement under way starts again with the next real render.  (A still camera never decides it.)
    p.tuneRestart = reused && first && in.tuneChoice < 0;
    // (a context that keeps another stream busy next to the frames -- the strip driver with its transfers on a stream of their own, the
    // denoise stream -- leaves room for two chains, or one: four streams that hand events to each other is what the device runs side by
    // side, rs_chains_in_flight)
    const int inFlight = in.chainsInFlight;
    const bool two = parityStreams && inFlight >= 2;
    // one of three: the chain streams first, the render's stream (idle after a fused launch) last
    const int turn = inFlight >= kPlanSmallChains ? in.smallChain : inFlight == 2 ? in.chain : 0;
    p.stream = !async ? -1 : three ? (turn < 2 ? 1 + turn : turn == 2 ? 0 : turn) : two ? 1 + in.chain : 1;
    p.lastChains = !async ? 0 : three ? (inFlight < kPlanSmallChains ? inFlight : kPlanSmallChains) : two ? kPlanChains : 1;
    p.splitSlot = 1 + p.stream;                                  // the hints of the stream this launch goes to (rs_tilesplit.h)
    p.splitCall = in.phaseACalls < 2 ? in.phaseACalls : 2;
    // One frame at a time -- a caller that waits for every frame before it enqueues the next (preview.cpp:337-361) -- has nothing running
    // next to this frame's kernels, like the synchronous mode: a launch lasts as long as its longest tile and RIS has the CUs to itself, so
    // it takes that mode's forms (heavy tiles split four ways, the alias table in LDS for large light sets).  Asked of the previous frame's
    // end event, never waited for: config 5 one frame in flight 3.34 -> 2.6 ms (synchronous 2.84).
    const bool alone = !async || in.idle;
    p.splitMode = rs_split_mode(alone, rs_launch_waves(p.tilesX, fuse ? p.fusedTilesY : p.tilesY));
    // The shadow rays of a launch that fills the chip several times over go to the library stream, behind the previous frame's
    // spatial pass: every stream then has slack against the frame period and three or four kernels are in flight at any time,
    // which is what a frame bound by VALU issue needs (1080p: 1.277 -> 1.245 ms).  A small launch -- a strip -- lasts as long as its
    // slowest wave, and there the library stream is the one chain that links consecutive frames: its shadow rays stay on the
    // frame's own chain (8 strips of 1080p: 0.235 ms against 0.270).  rs_set_stream_plan(-1, -1, 0 / 1): never / always.
    p.shadowOnLibrary = async && (in.shadowOnMain == 1 || (in.shadowOnMain == 2 && rs_launch_waves(p.tilesX, p.tilesY) >= kFuseMinWaves));
    // The LDS form runs one 1024-thread block per copy of the table: a launch of a few dozen blocks leaves most CUs idle and lasts as
    // long as one block.  Below 64 Ki pixels the table is read from global memory by 256-thread blocks, which spread evenly.  (Round 2
    // drew the line at 384 Ki pixels -- a 1/8 strip of 1080p 0.241 -> 0.231 ms per frame with the global table; measured again in round 5
    // through rs_strips_frame the LDS form wins on every rank of that split, 0.193 -> 0.191 ms on the heaviest strip and 0.149 -> 0.130 on
    // the lightest, whose chain is mostly RIS: profiles/r05_ab_strip_knobs.log.)
    // Alone the alias-in-LDS form is a third faster (config 5: 645 -> 455 us); inside overlapped frames it is slower (1.88 -> 1.95 ms per
    // frame: one 1024-thread block with 82 KB of LDS per CU keeps the other streams' kernels off that CU), so it is taken when the
    // kernels run one after the other on the library stream only (`alone`; A/B in profiles/r03_ab_config5_ris_alias_lds.log).
    const bool tableFits = !in.envMap && (long long)(rows ? in.y1 - in.y0 : 0) * in.width >= in.risGlobalBelow;   // (64 Ki pixels unless rs_set_ris_table_pixels says otherwise)
    p.risForm = tableFits && in.numLights > 0 && in.numLights <= kRisLdsLights ? RS_RIS_LDS
              : tableFits && in.numLights > kRisLdsLights && in.numLights <= kRisAliasLdsLights && alone ? RS_RIS_ALIAS_LDS : RS_RIS_GLOBAL;
    // Primary cuts (rs_cuts.h) belong to k_primary / k_primary_split: the fused launch walks two rays per pixel from 8x4 tiles and keeps
    // the tree (it only runs when something moved, or after an emission edit, which leaves the cut alone for the frames after it).  A key
    // that has just been seen unchanged for the first time builds -- behind this call's chain, so the frame itself still walks the tree --
    // and every later call with that key walks the cuts, whatever its rows (a strip), its stream or the number of frames in flight.
    // The tiles' leaf lists (rs_cuts.h "Leaf lists") have no field of their own: they are built by the same build and walked by the same
    // launches as the cuts, wherever the slot holds them.
    p.cut = rows && !fuse ? in.cutState : 0;
}
