#!/usr/bin/env python3
"""tools/bench_partial_refit.py [CONFIG] -- what a geometry edit of few triangles costs with rs_scene_set_partial_refit off and on, on
the scene of BASELINE config 3 (Sponza-class, 262 144 triangles) or 5 (Bistro-class).  Follows tools/bench_geometry_edits.py:

  A  stream time of ONE edit (two events on the library stream around the call, device otherwise idle; median, min and max of REPS)
     and the host time of the call, for m = 1, 16, 256, 4 096 and 1 % of the movable triangles through rs_scene_set_triangles, for 64
     emitters through rs_scene_set_geometry and for one rigid part of 256 triangles through rs_scene_set_part_transforms; with the mode
     on also the nodes the last edit recomputed (rs_debug_scene_refit_dirty)
  C  the frame period (ms per frame over FRAMES overlapped frames, enqueue all, synchronise once) with such an edit before every frame,
     against the unedited period measured the same way in the same process

The mode on is measured with a threshold that admits every m of the sweep, so that the table shows where the partial path stops paying.
With RESTIR_HIP_LIB naming a library from before the switch existed (an A/B build of the parent commit) only the mode off is measured:
that is the comparison base, the whole refit as it was.  The frame is bench.py's for N = 1.  Prints one line per figure and, last, one
JSON line.  Environment: FRAMES (default 100), REPS (default 15).
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
FRAMES = int(os.environ.get("FRAMES", "100"))
REPS = int(os.environ.get("REPS", "15"))

capi.init(0)
HAS_SWITCH = hasattr(capi.lib(), "rs_scene_set_partial_refit")
t0 = time.perf_counter()
sd = scenes.bistro_class(seed=2, scale=1.0) if DENOISE else scenes.sponza_class(seed=1, scale=1.0)
print("scene data: %d triangles, generated in %.1f s; library %s the switch" % (len(sd.material_ids), time.perf_counter() - t0, "has" if HAS_SWITCH else "is from before"), flush=True)
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
capi.set_stream(stream.cuda_stream)
capi.set_sync(False)
capi.set_internal_stream_priority(1 if DENOISE else 2)      # as bench.py
capi.prepare_streams()
cam = capi.camera_update(sd.camera(W, H))
orig = np.ascontiguousarray(sd.vertices, np.float32).reshape(-1, 3, 3)
light = sd.materials["type"][sd.material_ids] == 4
movable = np.nonzero(~light)[0].astype(np.int32)
lamps = np.nonzero(light)[0].astype(np.int32)
lo, hi = orig.reshape(-1, 3).min(0), orig.reshape(-1, 3).max(0)
ext = float((hi - lo).max())
rng = np.random.default_rng(1)
SWEEP = [("1", 1), ("16", 16), ("256", 256), ("4096", 4096), ("1pct", max(1, len(movable) // 100))]


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


scene = capi.Scene(orig, sd.normals, sd.texcoords, sd.material_ids, sd.materials)
scene.set_triangles(movable[:1], orig[movable[:1]])       # the first edit: whole, builds the refit's tables
capi.synchronize()


class Edit:
    """One edit of the sweep: its ids, and 8 poses it cycles through (a pose: vertices, or the matrix of the part)."""

    def __init__(self, call, ids, poses):
        self.call, self.ids, self.poses, self.k = call, ids, poses, 0

    def __call__(self):
        self.call(self.ids, self.poses[self.k % len(self.poses)])
        self.k += 1


edits = {}
for label, count in SWEEP:
    ids = np.sort(rng.choice(movable, count, replace=False)).astype(np.int32)
    edits[label] = Edit(scene.set_triangles, ids, [jitter(ids) for _ in range(8)])
if len(lamps):
    ids = lamps[:64]
    edits["emitters%d" % len(ids)] = Edit(scene.set_geometry, ids, [jitter(ids) for _ in range(8)])
# one rigid part of 256 triangles, all of them well inside the root box, moved by small translations of its rest pose
inner = movable[((orig[movable] > lo + 0.01 * (hi - lo)) & (orig[movable] < hi - 0.01 * (hi - lo))).all((1, 2))]
part = np.sort(rng.choice(inner, 256, replace=False)).astype(np.int32)
scene.define_parts([part.tolist()])
shifts = []
for j in range(8):
    m = np.eye(4, dtype=np.float32)
    m[3, :3] = np.float32(0.001 * ext) * np.sin(0.3 * j + np.arange(3, dtype=np.float32))
    shifts.append(m.reshape(1, 16))
edits["part256"] = Edit(lambda ids, matrix: scene.set_part_transforms([0], matrix), part, shifts)

result = {"config": CONFIG, "triangles": int(len(sd.material_ids)), "movable": int(len(movable)), "frames": FRAMES, "reps": REPS, "has_switch": HAS_SWITCH}
frames = Frames(scene)
for mode in ("off", "on") if HAS_SWITCH else ("off",):
    if HAS_SWITCH:
        scene.set_partial_refit(mode == "on", len(sd.material_ids))
        edits["1"]()                                     # (the first edit with the switch on builds the path's tables)
        capi.synchronize()
    out = result[mode] = {}
    for label, edit in edits.items():
        ids = edit.ids
        dev, host = [], []
        before = scene.refit_counts() if HAS_SWITCH else None
        for _ in range(REPS):
            capi.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t = time.perf_counter()
            edit()
            host.append((time.perf_counter() - t) * 1e3)
            e1.record(stream)
            capi.synchronize()
            dev.append(e0.elapsed_time(e1))
        r = out[label] = {"triangles": int(len(ids)), "stream_ms": float(np.median(dev)), "stream_ms_min": float(min(dev)), "stream_ms_max": float(max(dev)),
                          "host_call_ms": float(np.median(host))}
        extra = ""
        if HAS_SWITCH:
            after = scene.refit_counts()
            r["whole"], r["partial"], r["dirty_nodes"] = after[0] - before[0], after[1] - before[1], scene.refit_dirty()
            extra = "; %d whole, %d partial, %d nodes recomputed by the last" % (r["whole"], r["partial"], r["dirty_nodes"])
        print("A  mode %-3s %-10s %7d triangles: stream %.3f ms (median of %d; min %.3f, max %.3f), host call %.3f ms%s"
              % (mode, label, len(ids), r["stream_ms"], REPS, r["stream_ms_min"], r["stream_ms_max"], r["host_call_ms"], extra), flush=True)
    out["period_unedited_ms"] = frames.period(FRAMES)
    print("C  mode %-3s frame period, unedited: %.4f ms" % (mode, out["period_unedited_ms"]), flush=True)
    for label, edit in edits.items():
        out[label]["period_ms"] = frames.period(FRAMES, edit)
        print("C  mode %-3s frame period, %-10s before every frame: %.4f ms" % (mode, label, out[label]["period_ms"]), flush=True)
print(json.dumps(result))
