#!/usr/bin/env python3
"""tools/bench_motion_vectors.py [CONFIG] -- what motion tracking (rs_scene_set_motion_tracking, rs_scene_advance_motion) costs on the
scene of BASELINE config 3 (Sponza-class, 262 144 triangles) or 5 (Bistro-class) at 1080p.

  A  the G-buffer launch alone (rs_gbuffer_render between two events on the library stream, side streams off, retained planes off,
     device otherwise idle; median of REPS), the tracked kernel against the untracked one on the same scene, alternating, geometry still
  B  stream time of ONE rs_scene_advance_motion (two events around the call, device otherwise idle; median of REPS) and the host time of
     the call, after an edit of 1 triangle, of 1 % of the movable triangles and of all of them, and after no edit -- which must enqueue
     nothing: its stream time is that of an empty pair of events, measured next to it, and the scene's retained G-buffer planes stay valid
  C  the frame period (ms per frame over FRAMES overlapped frames, as bench.py takes ms_per_step: enqueue all, synchronise once) with an
     edit of 1 % of the triangles and an advance before every frame on a tracked scene, against the same edits on the untracked scene and
     the unedited period, measured the same way in the same process, alternating

The frame is bench.py's for N = 1: GBuffer::render, ReSTIRDirect, [LeveledEAWFilter, config 5], copyImageToPBO, GBuffer::update, on a
stream of torch's pool.  Prints one line per figure and, last, one JSON line.  Environment: FRAMES (default 300), REPS (default 15).
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from restir_amd import capi, scenes

CONFIG = int(sys.argv[1]) if len(sys.argv) > 1 else 3
assert CONFIG in (3, 5)
W, H = 1920, 1080
DENOISE = CONFIG == 5
REUSE, TONEMAP = 3, 2
FRAMES = int(os.environ.get("FRAMES", "300"))
REPS = int(os.environ.get("REPS", "15"))

capi.init(0)
t0 = time.perf_counter()
sd = scenes.bistro_class(seed=2, scale=1.0) if DENOISE else scenes.sponza_class(seed=1, scale=1.0)
print("scene data: %d triangles, generated in %.1f s" % (len(sd.material_ids), time.perf_counter() - t0), flush=True)
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
capi.set_stream(stream.cuda_stream)
capi.set_sync(False)
capi.set_internal_stream_priority(1 if DENOISE else 2)      # as bench.py
capi.prepare_streams()
cam = capi.camera_update(sd.camera(W, H))
orig = np.ascontiguousarray(sd.vertices, np.float32).reshape(-1, 3, 3)
movable = np.nonzero(sd.materials["type"][sd.material_ids] != 4)[0].astype(np.int32)
lo, hi = orig.reshape(-1, 3).min(0), orig.reshape(-1, 3).max(0)
ext = float((hi - lo).max())
rng = np.random.default_rng(1)


def jitter(vertices, ids, amount):
    return np.clip(vertices[ids] + rng.uniform(-amount, amount, (len(ids), 3, 3)).astype(np.float32) * np.float32(ext), lo, hi).astype(np.float32)


def timed(call):
    """(stream ms, host ms) of call() between two events on the idle library stream."""
    capi.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    t = time.perf_counter()
    call()
    host = (time.perf_counter() - t) * 1e3
    e1.record(stream)
    capi.synchronize()
    return e0.elapsed_time(e1), host


class Frames:
    def __init__(self, scene):
        self.scene = scene
        self.gbuf, self.restir = capi.GBuffer(W, H), capi.ReSTIR(W, H)
        self.image = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
        self.pbo = torch.zeros((W * H, 4), dtype=torch.uint8, device="cuda")
        self.eaw = capi.EAWFilter(W, H, 5) if DENOISE else None
        self.out = torch.zeros_like(self.image) if DENOISE else None
        self.looper = 0

    def frame(self):
        self.gbuf.render(self.scene, cam)
        self.restir.direct(self.scene, cam, self.gbuf, self.image.data_ptr(), 0, self.looper, REUSE)
        shown = self.eaw.filter(self.out.data_ptr(), self.image.data_ptr(), self.gbuf, cam) if DENOISE else self.image.data_ptr()
        capi.copy_image_to_pbo(self.pbo.data_ptr(), shown, W, H, TONEMAP, 1.0)
        self.gbuf.update(cam)
        self.looper += 1

    def period(self, frames, before=None):
        """ms per frame over `frames` overlapped frames; before(): called ahead of every frame."""
        for _ in range(40):                              # the library's launch-form measurement and the warm-up (bench.py: 38 + warm-up)
            if before:
                before()
            self.frame()
        capi.synchronize()
        t = time.perf_counter()
        for _ in range(frames):
            if before:
                before()
            self.frame()
        capi.synchronize()
        return (time.perf_counter() - t) / frames * 1e3


result = {"config": CONFIG, "triangles": int(len(sd.material_ids)), "movable": int(len(movable)), "frames": FRAMES, "reps": REPS}
scene = capi.Scene(orig, sd.normals, sd.texcoords, sd.material_ids, sd.materials)
scene.set_triangles(movable[:1], orig[movable[:1]])      # the first edit builds the refit's tables
capi.synchronize()
some = np.sort(rng.choice(movable, max(1, len(movable) // 100), replace=False)).astype(np.int32)
moved = [jitter(orig, some, 0.001) for _ in range(8)]
k = [0]


def edit():
    scene.set_triangles(some, moved[k[0] % 8]); k[0] += 1


def edit_and_advance():
    edit()
    scene.advance_motion()


# ---- C: an edit and an advance before every frame ---------------------------------------------------------------------------------------------
f = Frames(scene)
periods = {"unedited": [], "edits_untracked": [], "edits_tracked": [], "tracked_still": []}
for _ in range(2):                                       # alternating: other work shares the host
    scene.set_motion_tracking(False)
    periods["unedited"].append(f.period(FRAMES))
    periods["edits_untracked"].append(f.period(FRAMES, edit))
    scene.set_motion_tracking(True)
    periods["edits_tracked"].append(f.period(FRAMES, edit_and_advance))
    scene.set_triangles(movable, orig[movable]); scene.advance_motion()
    periods["tracked_still"].append(f.period(FRAMES, scene.advance_motion))
result["period_ms"] = periods
print("C  frame period, two rounds each: unedited %s ms; an edit of %d triangles before every frame, untracked %s ms; the same edits and an advance, "
      "tracked %s ms; tracked, still geometry, an advance before every frame (retained planes) %s ms"
      % (", ".join("%.4f" % p for p in periods["unedited"]), len(some), ", ".join("%.4f" % p for p in periods["edits_untracked"]),
         ", ".join("%.4f" % p for p in periods["edits_tracked"]), ", ".join("%.4f" % p for p in periods["tracked_still"])), flush=True)

# ---- B: one advance ------------------------------------------------------------------------------------------------------------------------------
scene.set_motion_tracking(True)
for label, count in (("1", 1), ("1pct", max(1, len(movable) // 100)), ("all", len(movable))):
    ids = np.sort(rng.choice(movable, count, replace=False)).astype(np.int32)
    dev, host = [], []
    for _ in range(REPS):
        scene.set_triangles(ids, jitter(orig, ids, 0.001))
        d, h = timed(scene.advance_motion)
        dev.append(d); host.append(h)
    result["advance_after_edit_%s" % label] = {"triangles": count, "stream_ms": float(np.median(dev)), "stream_ms_min": float(min(dev)),
                                               "stream_ms_max": float(max(dev)), "host_call_ms": float(np.median(host))}
    print("B  rs_scene_advance_motion after an edit of %7d triangles: stream %.4f ms (median of %d; min %.4f, max %.4f), host call %.4f ms"
          % (count, np.median(dev), REPS, min(dev), max(dev), np.median(host)), flush=True)
g = capi.GBuffer(W, H)
g.set_reuse(True)
for _ in range(4):                                       # a still camera: the fourth request is answered from retained planes
    g.render(scene, cam); g.update(cam)
before = g.reuse_stats()
dev, host, empty = [], [], []
for _ in range(REPS):
    d, h = timed(scene.advance_motion)
    dev.append(d); host.append(h)
    empty.append(timed(lambda: None)[0])
    g.render(scene, cam); g.update(cam)
after = g.reuse_stats()
if not (after[0] == before[0] and after[1] == before[1] + REPS):      # nothing enqueued, nothing invalidated: every request must have been reused
    print("B  UNEXPECTED: render requests between the advances were not all answered from retained planes:", before, after, flush=True)
result["advance_after_no_edit"] = {"stream_ms": float(np.median(dev)), "empty_event_pair_ms": float(np.median(empty)), "host_call_ms": float(np.median(host)),
                                   "requests_reused": after[1] - before[1], "requests_rendered": after[0] - before[0]}
print("B  rs_scene_advance_motion after no edit: stream %.4f ms against %.4f ms for an empty pair of events, host call %.4f ms; %d of %d render requests "
      "in between answered from retained planes" % (np.median(dev), np.median(empty), np.median(host), after[1] - before[1], REPS), flush=True)

# ---- A: the G-buffer launch alone ------------------------------------------------------------------------------------------------------------------
capi.synchronize()
capi.set_side_stream(0)                                   # the render goes out on the library stream, as its own launch
g = capi.GBuffer(W, H)
g.set_reuse(False)
times = {False: [], True: []}
for rep in range(REPS + 3):
    for tracked in (False, True):
        scene.set_motion_tracking(tracked)
        d, _ = timed(lambda: g.render(scene, cam))
        g.update(cam)
        if rep >= 3:                                     # (the first launches load the code objects and fill the tile-split hints)
            times[tracked].append(d)
capi.set_side_stream(4)
result["gbuffer_launch_ms"] = {"untracked": float(np.median(times[False])), "tracked": float(np.median(times[True])),
                               "untracked_min_max": [float(min(times[False])), float(max(times[False]))],
                               "tracked_min_max": [float(min(times[True])), float(max(times[True]))]}
print("A  rs_gbuffer_render alone, still geometry: untracked %.4f ms (min %.4f, max %.4f), tracked %.4f ms (min %.4f, max %.4f), median of %d, alternating"
      % (np.median(times[False]), min(times[False]), max(times[False]), np.median(times[True]), min(times[True]), max(times[True]), REPS), flush=True)
print(json.dumps(result))
