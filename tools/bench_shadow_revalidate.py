#!/usr/bin/env python3
"""tools/bench_shadow_revalidate.py [--frames N] [--warmup W] [--reps R] -- what shadow revalidation (rs_restir_set_shadow_revalidation)
costs, on the scene of BASELINE config 3 at 1080p in the overlapped mode (rs_set_sync(0)): GBuffer::render, ReSTIRDirect (reuse 3),
copyImageToPBO and GBuffer::update with a still camera, timed over N frames between two synchronisations, R times each, the switch off
and on alternating within one run.

  moving   a rigid part of triangles that emit nothing (rs_scene_define_parts) is moved by a matrix before every frame
           (rs_scene_set_part_transforms), with the switch off / on
  still    no edit at all, off / on: the same kernels are launched (launched_frames counts the frames whose phase A launched
           k_revalidate -- asked on the host after every frame, without a wait -- and must be 0)

Prints one JSON line with the median and the range of every figure, and the kernel's counters { examined, walked, occluded } of the last
moving frame.  A library without the feature (RESTIR_HIP_LIB pointing at another build, e.g. the parent commit's, for an A/B in the same
session) measures the `off` columns alone."""
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
ap.add_argument("--part", type=int, default=64, help="triangles of the moved part")
args = ap.parse_args()

W, H = 1920, 1080
capi.init(0)
HAVE = hasattr(capi.lib(), "rs_restir_set_shadow_revalidation")
sd = scenes.sponza_class(seed=1, scale=1.0)
v = sd.vertices.reshape(-1, 3, 3)
lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
movable = np.nonzero(sd.materials["type"][sd.material_ids] != LIGHT)[0]
far = np.abs((v[movable].mean(1) - (lo + hi) / 2) / (hi - lo)).max(1)
part = movable[np.argsort(far, kind="stable")[:args.part]].astype(np.int32)       # the triangles nearest the scene's middle: an occluder
SWING = np.float32(0.02 * float((hi - lo)[0]))


def matrix(f):
    """A small swing about the rest pose (column-major 4x4): a translation along x."""
    m = np.eye(4, dtype=np.float32)
    m[3, 0] = SWING * np.float32(np.sin(0.3 * f))
    return m.reshape(1, 16)


def run(on, moving):
    scene = capi.Scene(sd.vertices, sd.normals, sd.texcoords, sd.material_ids, sd.materials)
    if moving:
        scene.define_parts([part])
    cam = capi.camera_update(sd.camera(W, H))
    gbuf, restir = capi.GBuffer(W, H), capi.ReSTIR(W, H)
    if on:
        restir.set_shadow_revalidation(True)
    image = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
    pbo = torch.zeros((W * H, 4), dtype=torch.uint8, device="cuda")
    launched = [0]

    def frame(f):
        if moving:
            scene.set_part_transforms([0], matrix(f))
        gbuf.render(scene, cam)
        restir.direct(scene, cam, gbuf, image.data_ptr(), 0, f, 3)
        capi.copy_image_to_pbo(pbo.data_ptr(), image.data_ptr(), W, H, 2, 1.0)
        gbuf.update(cam)
        if HAVE:
            launched[0] += int(restir.revalidate_launched())

    for f in range(args.warmup):
        frame(f)
    capi.synchronize()
    launched[0] = 0
    t0 = time.perf_counter()
    for f in range(args.warmup, args.warmup + args.frames):
        frame(f)
    capi.synchronize()
    ms = (time.perf_counter() - t0) / args.frames * 1e3
    stats = restir.revalidate_stats() if on else None
    del restir, gbuf, scene
    return ms, stats, launched[0]


capi.set_sync(False)
capi.prepare_streams()
cases = [(kind, on) for kind in ("moving", "still") for on in ((False, True) if HAVE else (False,))]
times = {c: [] for c in cases}
launched = {c: [] for c in cases}
last_stats = None
for rep in range(args.reps):
    for c in cases:                                          # off, on, off, on, ...: both columns of a pair in every round
        ms, stats, n = run(c[1], c[0] == "moving")
        times[c].append(ms)
        launched[c].append(n)
        if c == ("moving", True):
            last_stats = stats
capi.synchronize()
capi.set_sync(True)
out = {"%s_%s" % (c[0], "on" if c[1] else "off"): dict(median=round(float(np.median(t)), 4), min=round(float(np.min(t)), 4), max=round(float(np.max(t)), 4),
                                                     launched_frames=launched[c]) for c, t in times.items()}
print(json.dumps(dict(lib=os.environ.get("RESTIR_HIP_LIB", "in-tree"), revalidation=HAVE, width=W, height=H, frames=args.frames, reps=args.reps,
                      part_triangles=int(len(part)), ms_per_frame=out, last_frame_revalidate_stats=last_stats)))
