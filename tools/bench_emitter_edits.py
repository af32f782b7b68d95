#!/usr/bin/env python3
"""tools/bench_emitter_edits.py [CONFIG] -- what rs_scene_set_geometry costs when it moves emitters, on the scene of BASELINE config 3
(Sponza-class) or 5 (Bistro-class), next to what a caller had before it -- rs_scene_create of the edited scene -- and next to the floor,
rs_scene_set_triangles of the same number of triangles that are no emitters.

  A  ONE rs_scene_set_geometry moving 1, 64 and all emitters: the enqueue time (host time of the call) and the device time (two events
     on the library stream around the call, device otherwise idle), median of REPS
  F  the same for rs_scene_set_triangles with 1, 64 and as many non-emitters as the scene has emitters: the floor
  B  wall time of rs_scene_create from the edited scene's host description (median of 3): the alternative, which also drops the frames in
     flight and every reservoir
  C  the frame period (ms per frame over FRAMES overlapped frames, as bench.py takes ms_per_step) with one rs_scene_set_geometry of 64
     emitters before every frame, with one rs_scene_set_triangles of 64 non-emitters before every frame, and unedited

The frame is bench.py's for N = 1 (tools/bench_geometry_edits.py).  Prints one line per figure and, last, one JSON line.  Environment:
FRAMES (default 300), REPS (default 15).  On a build without rs_scene_set_geometry (the parent commit) A and its period are skipped.
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
HAVE = hasattr(capi.Scene, "set_geometry")

capi.init(0)
sd = scenes.bistro_class(seed=2, scale=1.0) if DENOISE else scenes.sponza_class(seed=1, scale=1.0)
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
capi.set_stream(stream.cuda_stream)
capi.set_sync(False)
capi.set_internal_stream_priority(1 if DENOISE else 2)      # as bench.py
capi.prepare_streams()
cam = capi.camera_update(sd.camera(W, H))
orig = np.ascontiguousarray(sd.vertices, np.float32).reshape(-1, 3, 3)
light = sd.materials["type"][sd.material_ids] == 4
emitters, movable = np.nonzero(light)[0].astype(np.int32), np.nonzero(~light)[0].astype(np.int32)
lo, hi = orig.reshape(-1, 3).min(0), orig.reshape(-1, 3).max(0)
ext = float((hi - lo).max())
rng = np.random.default_rng(1)
print("scene: %d triangles, %d of them emitters" % (len(light), len(emitters)), flush=True)


def jitter(ids, amount=0.001):
    return np.clip(orig[ids] + rng.uniform(-amount, amount, (len(ids), 3, 3)).astype(np.float32) * np.float32(ext), lo, hi).astype(np.float32)


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
        for _ in range(40):                              # the library's launch-form measurement and the warm-up
            self.frame()
        capi.synchronize()
        t = time.perf_counter()
        for _ in range(frames):
            if before:
                before()
            self.frame()
        capi.synchronize()
        return (time.perf_counter() - t) / frames * 1e3


result = {"config": CONFIG, "triangles": int(len(light)), "emitters": int(len(emitters)), "frames": FRAMES, "reps": REPS, "set_geometry": HAVE}
scene = capi.Scene(orig, sd.normals, sd.texcoords, sd.material_ids, sd.materials)
scene.set_triangles(movable[:1], orig[movable[:1]])       # the first edits build the refit's tables and the version ring
if HAVE:
    scene.set_geometry(emitters[:1], orig[emitters[:1]])
capi.synchronize()


def one_edit(call, ids):
    dev, host = [], []
    for _ in range(REPS):
        v = jitter(ids)
        capi.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t = time.perf_counter()
        call(ids, v)
        host.append((time.perf_counter() - t) * 1e3)
        e1.record(stream)
        capi.synchronize()
        dev.append(e0.elapsed_time(e1))
    return {"triangles": int(len(ids)), "device_ms": float(np.median(dev)), "device_ms_min": float(min(dev)), "device_ms_max": float(max(dev)),
            "enqueue_ms": float(np.median(host))}


for label, count in (("1", 1), ("64", 64), ("all", len(emitters))):
    count = min(count, len(emitters))
    rows = [("F", "rs_scene_set_triangles", scene.set_triangles, movable)]
    if HAVE:
        rows.insert(0, ("A", "rs_scene_set_geometry ", scene.set_geometry, emitters))
    for tag, what, call, pool in rows:
        r = one_edit(call, np.sort(rng.choice(pool, count, replace=False)).astype(np.int32))
        result["%s_%s" % (tag, label)] = r
        print("%s  %s, %6d %s: enqueue %.3f ms, device %.3f ms (median of %d; min %.3f, max %.3f)"
              % (tag, what, count, "emitters    " if tag == "A" else "non-emitters", r["enqueue_ms"], r["device_ms"], REPS, r["device_ms_min"], r["device_ms_max"]), flush=True)
scene.set_triangles(movable, orig[movable])
if HAVE:
    scene.set_geometry(emitters, orig[emitters])
capi.synchronize()

# ---- B: the alternative ------------------------------------------------------------------------------------------------------------------
walls = []
for _ in range(3):
    v_now, n_now = scene.geometry()
    desc = scene.host_desc()
    capi.synchronize()
    t = time.perf_counter()
    other = capi.Scene.from_tables(v_now, n_now, sd.texcoords, sd.material_ids, sd.materials, desc)
    capi.synchronize()
    walls.append((time.perf_counter() - t) * 1e3)
    other.destroy()
result["create_wall_ms"] = sorted(walls)[1]
print("B  rs_scene_create of the edited scene's description: %.1f ms wall (median of 3: %s)" % (result["create_wall_ms"], ", ".join("%.1f" % w for w in walls)), flush=True)

# ---- C: an edit before every frame -----------------------------------------------------------------------------------------------------------
f = Frames(scene)
result["period_unedited_ms"] = f.period(FRAMES)
k = [0]


def every_frame(call, pool):
    ids = np.sort(rng.choice(pool, min(64, len(pool)), replace=False)).astype(np.int32)
    moved = [jitter(ids) for _ in range(8)]

    def edit():
        call(ids, moved[k[0] % 8]); k[0] += 1
    return edit
if HAVE:
    result["period_set_geometry_every_frame_ms"] = f.period(FRAMES, every_frame(scene.set_geometry, emitters))
result["period_set_triangles_every_frame_ms"] = f.period(FRAMES, every_frame(scene.set_triangles, movable))
result["period_unedited_again_ms"] = f.period(FRAMES)
print("C  frame period: unedited %.4f ms; 64 emitters moved before every frame %s ms; 64 non-emitters (rs_scene_set_triangles) %.4f ms; unedited again %.4f ms"
      % (result["period_unedited_ms"], "%.4f" % result["period_set_geometry_every_frame_ms"] if HAVE else "n/a",
         result["period_set_triangles_every_frame_ms"], result["period_unedited_again_ms"]), flush=True)
print(json.dumps(result))
