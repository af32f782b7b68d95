#!/usr/bin/env python3
"""tools/bench_geometry_edits.py [CONFIG] -- what rs_scene_set_triangles costs on the scene of BASELINE config 3 (Sponza-class, 262 144
triangles) or 5 (Bistro-class), next to the only alternative a caller had before it: destroy the scene and build a new one.

  A  stream time of ONE rs_scene_set_triangles (two events on the library stream around the call, device otherwise idle; median of
     REPS) and the host time of the call, for 1 triangle, 1 % of the movable triangles and all of them
  B  wall time of rs_scene_destroy + rs_scene_build from the same arrays (median of 3)
  C  the frame period (ms per frame over FRAMES overlapped frames, as bench.py takes ms_per_step: enqueue all, synchronise once) with
     an edit of 1 % of the triangles before every frame, against the unedited period measured the same way in the same process
  D  tree-quality drift: the frame period on a scene refitted 100 times with small jitter (each edit moves every movable triangle by up
     to 0.1 % of the scene's extent from where the edit before left it) against a scene built afresh from the same final vertices

The frame is bench.py's for N = 1: GBuffer::render, ReSTIRDirect, [LeveledEAWFilter, config 5], copyImageToPBO, GBuffer::update, on a
stream of torch's pool.  D also compares 3 Mi trace results of the refitted scene, bit for bit, with those of rs_scene_create of its host
description (must be equal) and of the scene built afresh.  Prints one line per figure and, last, one JSON line.  Environment: FRAMES
(default 300), REPS (default 15), ONLY=D (the drift part alone).
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
ONLY_D = os.environ.get("ONLY", "") == "D"             # the drift part alone (A-C skipped)
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


def build(vertices=None):
    return capi.Scene(orig if vertices is None else vertices, sd.normals, sd.texcoords, sd.material_ids, sd.materials)


def jitter(vertices, ids, amount):
    return np.clip(vertices[ids] + rng.uniform(-amount, amount, (len(ids), 3, 3)).astype(np.float32) * np.float32(ext), lo, hi).astype(np.float32)


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

# ---- B: the alternative ------------------------------------------------------------------------------------------------------------------
scene = build()
walls = []
for _ in range(0 if ONLY_D else 3):
    capi.synchronize()
    t = time.perf_counter()
    scene.destroy()
    scene = build()
    capi.synchronize()
    walls.append((time.perf_counter() - t) * 1e3)
result["rebuild_wall_ms"] = sorted(walls)[1] if walls else None
if not ONLY_D:
    print("B  rs_scene_destroy + rs_scene_build: %.1f ms wall (median of 3: %s)" % (result["rebuild_wall_ms"], ", ".join("%.1f" % w for w in walls)), flush=True)

# ---- A: one edit ---------------------------------------------------------------------------------------------------------------------------
cur = orig.copy()
t = time.perf_counter()
scene.set_triangles(movable[:1], cur[movable[:1]])       # the first edit builds the refit's tables
capi.synchronize()
result["first_edit_wall_ms"] = (time.perf_counter() - t) * 1e3
print("A  first edit (builds and uploads the refit's tables): %.1f ms wall" % result["first_edit_wall_ms"], flush=True)
for label, count in () if ONLY_D else (("1", 1), ("1pct", max(1, len(movable) // 100)), ("all", len(movable))):
    ids = np.sort(rng.choice(movable, count, replace=False)).astype(np.int32)
    dev, host = [], []
    for _ in range(REPS):
        v = jitter(orig, ids, 0.001)
        capi.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t = time.perf_counter()
        scene.set_triangles(ids, v)
        host.append((time.perf_counter() - t) * 1e3)
        e1.record(stream)
        capi.synchronize()
        dev.append(e0.elapsed_time(e1))
    result["edit_%s" % label] = {"triangles": count, "stream_ms": float(np.median(dev)), "stream_ms_min": float(min(dev)),
                                 "host_call_ms": float(np.median(host))}
    print("A  rs_scene_set_triangles, %7d triangles: stream %.3f ms (median of %d; min %.3f, max %.3f), host call %.3f ms"
          % (count, np.median(dev), REPS, min(dev), max(dev), np.median(host)), flush=True)
scene.set_triangles(movable, orig[movable])
capi.synchronize()

# ---- C: an edit before every frame -----------------------------------------------------------------------------------------------------------
f = Frames(scene)
result["period_unedited_ms"] = f.period(FRAMES) if not ONLY_D else None
some = np.sort(rng.choice(movable, max(1, len(movable) // 100), replace=False)).astype(np.int32)
moved = [jitter(orig, some, 0.001) for _ in range(8)]
k = [0]


def edit():
    scene.set_triangles(some, moved[k[0] % 8]); k[0] += 1
result["period_edit_every_frame_ms"] = f.period(FRAMES, edit) if not ONLY_D else None
result["period_unedited_again_ms"] = f.period(FRAMES) if not ONLY_D else None
if not ONLY_D:
    print("C  frame period: unedited %.4f ms, an edit of %d triangles before every frame %.4f ms, unedited again %.4f ms"
      % (result["period_unedited_ms"], len(some), result["period_edit_every_frame_ms"], result["period_unedited_again_ms"]), flush=True)

# ---- D: drift ---------------------------------------------------------------------------------------------------------------------------------
scene.set_triangles(movable, orig[movable])
cur = orig.copy()
for _ in range(100):
    cur[movable] = jitter(cur, movable, 0.001)
    scene.set_triangles(movable, cur[movable])
capi.synchronize()
result["period_refitted_100x_ms"] = Frames(scene).period(FRAMES)
fresh = build(cur)
result["period_fresh_same_vertices_ms"] = Frames(fresh).period(FRAMES)
# Ray for ray, bit for bit (1 Mi rays through rs_trace_closest and rs_trace_closest_wave, 1 Mi segments through rs_trace_occlusion): the
# refitted scene against rs_scene_create of its own host description -- the acceptance criterion, must be 0 -- and against the scene built
# afresh, whose rs_build_bvh chooses another topology: the reference's own result depends on it where a box test rounds the other way.
capi.set_sync(True)
n = 1 << 20
o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
d = rng.normal(size=(n, 3)).astype(np.float32)
d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
rays = torch.from_numpy(np.ascontiguousarray(np.concatenate([o, d], 1))).cuda()
segs = torch.from_numpy(np.ascontiguousarray(np.concatenate([o, rng.uniform(lo, hi, (n, 3)).astype(np.float32)], 1))).cuda()


def differing(a, b):
    count = 0
    for fn in (capi.trace_closest, capi.trace_closest_wave):
        x, y = fn(a, rays), fn(b, rays)
        hit = x[0] >= 0
        count += int((x[0] != y[0]).sum())
        for p, q in zip(x[1:], y[1:]):                   # material id, position, normal of the hits
            count += int((p[hit].view(torch.int32).reshape(int(hit.sum()), -1) != q[hit].view(torch.int32).reshape(int(hit.sum()), -1)).any(1).sum())
    return count + int((capi.trace_occlusion(a, segs) != capi.trace_occlusion(b, segs)).sum())
v_now, n_now = scene.geometry()
assert np.array_equal(v_now.view(np.uint32), cur.view(np.uint32))
described = capi.Scene.from_tables(v_now, n_now, sd.texcoords, sd.material_ids, sd.materials, scene.host_desc())
result["rays_checked"] = 3 * n
result["differing_from_created_from_description"] = differing(scene, described)
result["differing_from_built_afresh"] = differing(scene, fresh)
capi.set_sync(False)
print("D  refitted against rs_scene_create of its host description: %d of %d closest-hit and occlusion results differ; against the scene built afresh (another topology): %d"
      % (result["differing_from_created_from_description"], 3 * n, result["differing_from_built_afresh"]), flush=True)
described.destroy()
print("D  frame period after 100 refits with 0.1 %% jitter: %.4f ms; a scene built afresh from the same vertices: %.4f ms"
      % (result["period_refitted_100x_ms"], result["period_fresh_same_vertices_ms"]), flush=True)
print(json.dumps(result))
