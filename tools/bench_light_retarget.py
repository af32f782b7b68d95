#!/usr/bin/env python3
"""tools/bench_light_retarget.py [--frames N] [--warmup W] [--reps R] -- what light retargeting (rs_restir_set_light_retargeting) costs, on
the scene of BASELINE config 3 at 1080p in the overlapped mode (rs_set_sync(0)): GBuffer::render, ReSTIRDirect (reuse 3), copyImageToPBO
and GBuffer::update with a still camera, timed over N frames between two synchronisations, R times each, interleaved.

  moving   one lamp is a rigid part (rs_scene_define_parts) that a matrix moves before every frame (rs_scene_set_part_transforms), with
           tracking off / tracking / retargeting
  still    no edit at all, with tracking / retargeting: expected equal, nothing extra is launched

Prints one JSON line with the median and the spread of every figure.  A library without retargeting (RESTIR_HIP_LIB pointing at another
build, e.g. the parent commit's, for an A/B in the same run) measures the modes it has."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from restir_amd import capi, scenes
from restir_amd.ctypes_structs import LIGHT

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

W, H = 1920, 1080
capi.init(0)
HAVE = hasattr(capi.lib(), "rs_restir_set_light_retargeting")
sd = scenes.sponza_class(seed=1, scale=1.0)
light = sd.materials["type"][sd.material_ids] == LIGHT
lamp = np.nonzero(light)[0].astype(np.int32)[:2]           # one lamp: two emissive triangles


def matrix(f):
    """A small swing about the rest pose (column-major 4x4): a translation along x."""
    m = np.eye(4, dtype=np.float32)
    m[3, 0] = np.float32(0.05 * np.sin(0.3 * f))
    return m.reshape(1, 16)


def run(mode, moving):
    scene = capi.Scene(sd.vertices, sd.normals, sd.texcoords, sd.material_ids, sd.materials)
    if moving:
        scene.define_parts([lamp])
    cam = capi.camera_update(sd.camera(W, H))
    gbuf, restir = capi.GBuffer(W, H), capi.ReSTIR(W, H)
    if mode == "tracking":
        restir.set_light_tracking(True)
    if mode == "retargeting":
        restir.set_light_retargeting(True)
    image = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
    pbo = torch.zeros((W * H, 4), dtype=torch.uint8, device="cuda")

    def frame(f):
        if moving:
            scene.set_part_transforms([0], matrix(f))
        gbuf.render(scene, cam)
        restir.direct(scene, cam, gbuf, image.data_ptr(), 0, f, 3)
        capi.copy_image_to_pbo(pbo.data_ptr(), image.data_ptr(), W, H, 2, 1.0)
        gbuf.update(cam)

    for f in range(args.warmup):
        frame(f)
    capi.synchronize()
    t0 = time.perf_counter()
    for f in range(args.warmup, args.warmup + args.frames):
        frame(f)
    capi.synchronize()
    ms = (time.perf_counter() - t0) / args.frames * 1e3
    stats = restir.retarget_stats() if mode == "retargeting" else None
    del restir, gbuf, scene
    return ms, stats


capi.set_sync(False)
capi.prepare_streams()
cases = [("moving", m) for m in ("off", "tracking") + (("retargeting",) if HAVE else ())]
cases += [("still", m) for m in ("tracking",) + (("retargeting",) if HAVE else ())]
times = {c: [] for c in cases}
last_stats = None
for rep in range(args.reps):
    for c in cases:
        ms, stats = run(c[1], c[0] == "moving")
        times[c].append(ms)
        if c == ("moving", "retargeting"):
            last_stats = stats
capi.synchronize()
capi.set_sync(True)
out = {"%s_%s" % c: dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4)) for c, v in times.items()}
print(json.dumps(dict(lib=os.environ.get("RESTIR_HIP_LIB", "in-tree"), retargeting=HAVE, width=W, height=H, frames=args.frames, reps=args.reps,
                      lamp_triangles=int(len(lamp)), ms_per_frame=out, last_frame_retarget_stats=last_stats)))
