#!/usr/bin/env python3
"""tools/bench_dynamic_lights.py [--config 3|5] [--frames N] [--warmup W] -- the cost of emission edits (rs_scene_set_emission) and of
light tracking (rs_restir_set_light_tracking) in the overlapped mode (rs_set_sync(0)): runCuda's GBuffer::render, ReSTIRDirect (reuse 3),
copyImageToPBO and GBuffer::update at 1080p with the orbiting camera, timed over N frames between two synchronisations.  Three runs:
no edits; 1/8 of the lamps recoloured before every frame; the same edits with tracking on.  Also the host time of one set_emission call
that edits every lamp material (config 5: 5 120 materials, 10 240 lights).  Prints one JSON line."""
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
ap.add_argument("--config", type=int, default=3, choices=(3, 5))
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--warmup", type=int, default=40)
args = ap.parse_args()

W, H = 1920, 1080
capi.init(0)
sd = scenes.sponza_class(seed=1, scale=1.0) if args.config == 3 else scenes.bistro_class(seed=2, scale=1.0)
lamps = np.nonzero(sd.materials["type"] == LIGHT)[0].astype(np.int32)
E = sd.materials["baseColor"][lamps].astype(np.float32)
rng = np.random.default_rng(1)


def run(edit, track):
    scene = capi.Scene(sd.vertices, sd.normals, sd.texcoords, sd.material_ids, sd.materials)
    cam = capi.camera_update(sd.camera(W, H))
    base = sd.camera_args["position"]
    gbuf, restir = capi.GBuffer(W, H), capi.ReSTIR(W, H)
    restir.set_light_tracking(track)
    image = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
    pbo = torch.zeros((W * H, 4), dtype=torch.uint8, device="cuda")
    k = max(1, len(lamps) // 8)
    edits = []
    for f in range(16):                                   # a few edit sets, prepared outside the timed region
        sel = rng.choice(len(lamps), k, replace=False)
        edits.append((lamps[sel].copy(), (E[sel] * rng.uniform(0.0, 2.0, (k, 1))).astype(np.float32)))

    def frame(f):
        if edit:
            scene.set_emission(*edits[f % len(edits)])
        p = scenes.orbit_position(base, f, radius=1.0)
        for i in range(3):
            cam.position[i] = float(p[i])
        capi.camera_update(cam)
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
    return ms, scene


capi.set_sync(False)
capi.prepare_streams()
plain, _ = run(False, False)
edits, _ = run(True, False)
tracked, scene = run(True, True)
capi.synchronize()
# host time of one edit of every lamp material (the ring has a free slot: the frames above have finished)
host = []
for i in range(20):
    capi.synchronize()
    t0 = time.perf_counter()
    scene.set_emission(lamps, E * (1.0 + 0.01 * i))
    host.append((time.perf_counter() - t0) * 1e3)
capi.synchronize()
capi.set_sync(True)
desc = scene.host_desc()
print(json.dumps(dict(config=args.config, width=W, height=H, frames=args.frames, lights=int(desc["num_lights"]),
                      lamp_materials=int(len(lamps)), edited_per_frame=max(1, len(lamps) // 8),
                      ms_per_frame=dict(no_edits=round(plain, 4), edit_every_frame=round(edits, 4), edit_every_frame_tracked=round(tracked, 4)),
                      set_emission_host_ms=dict(median=round(float(np.median(host)), 4), min=round(float(np.min(host)), 4)))))
