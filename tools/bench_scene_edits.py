#!/usr/bin/env python3
"""tools/bench_scene_edits.py [--frames N] [--warmup W] [--repeats R] -- the cost of material, texture and environment-map edits
(rs_scene_set_materials, rs_scene_set_texture) on the config-3 scene (the Sponza-class hall, 262 144 triangles, 1 024 lights) given a
1024 x 1024 base-colour map and a 64 x 32 environment map:
  * host time of one materials edit, of one texture edit of the 1024 x 1024 map and of one environment edit (the ring has a free slot);
  * host time of an environment edit at 64 x 32, 1024 x 512 and 2048 x 1024 on a Cornell box (the work is the map's: the pdf, its alias
    table, the copies; the light sampler behind it has 3 entries there and 1 025 in the hall), split into rs_build_envmap_pdf,
    rs_build_alias_table (timed on their own) and the rest (staging, copies, the light tables);
  * the overlapped frame period (rs_set_sync(0): GBuffer::render, ReSTIRDirect reuse 3, copyImageToPBO, GBuffer::update at 1080p, orbiting
    camera) with one materials edit before every frame against none, R alternating repeats of each;
  * for scale, rs_scene_create from the scene's own host description: the only way to make such an edit before.
Prints one JSON line."""
import argparse
import ctypes as C
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
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--warmup", type=int, default=40)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()

W, H = 1920, 1080
capi.init(0)
rng = np.random.default_rng(1)
sd = scenes.sponza_class(seed=1, scale=1.0)
big = rng.uniform(0.2, 0.9, (1024, 1024, 3)).astype(np.float32)


def sky(h, w):
    e = np.repeat((0.3 + 0.4 * (1.0 - np.arange(h)[:, None, None] / h)) * np.array([0.6, 0.8, 1.0]), w, axis=1)
    e[h // 5: h // 5 + max(1, h // 10), w // 4: w // 4 + max(1, w // 16)] = (60.0, 55.0, 40.0)
    return e.astype(np.float32)


mats = sd.materials.copy()
mats[0]["baseColorMapId"] = 0
plain = np.nonzero(mats["type"] != LIGHT)[0].astype(np.int32)


def timed(call, n=20):
    out = []
    for i in range(n):
        capi.synchronize()
        t0 = time.perf_counter()
        call(i)
        out.append((time.perf_counter() - t0) * 1e3)
    capi.synchronize()
    out = out[2:]                                           # the first edits allocate the ring and the second and third texel arrays
    return dict(median=round(float(np.median(out)), 4), min=round(float(np.min(out)), 4), max=round(float(np.max(out)), 4))


def material_records(i):
    m = mats[plain].copy()
    m["roughness"] = 0.1 + 0.8 * ((i * 7) % 10) / 10.0
    m["baseColor"] *= np.float32(0.9 + 0.01 * (i % 10))
    return m


t0 = time.perf_counter()
scene = capi.Scene(sd.vertices, sd.normals, sd.texcoords, sd.material_ids, mats, textures=[big, sky(32, 64)], env_map_tex=1)
build_ms = (time.perf_counter() - t0) * 1e3
host = dict(
    set_materials=timed(lambda i: scene.set_materials(plain, material_records(i))),
    set_texture_1024x1024=timed(lambda i: scene.set_texture(0, big * np.float32(0.5 + 0.02 * i))),
    set_environment_64x32=timed(lambda i: scene.set_texture(1, sky(32, 64) * np.float32(0.5 + 0.02 * i))),
)

# rs_scene_create from the scene's own description
desc = scene.host_desc()
create = []
for i in range(3):
    capi.synchronize()
    t0 = time.perf_counter()
    again = capi.Scene.from_tables(sd.vertices, sd.normals, sd.texcoords, sd.material_ids, desc["materials"], desc,
                                   textures=desc["textures"], env_map_tex=1, env_sampler=(desc["env_prob"], desc["env_fail"]))
    capi.synchronize()
    create.append((time.perf_counter() - t0) * 1e3)
    again.destroy()

# environment edits by map size
box = scenes.cornell_box()
env_sizes = {}
L = capi.lib()
for h, w in ((32, 64), (512, 1024), (1024, 2048)):
    e = sky(h, w)
    s = capi.Scene(box.vertices, box.normals, box.texcoords, box.material_ids, box.materials, textures=[e], env_map_tex=0)
    total = timed(lambda i: s.set_texture(0, e * np.float32(0.5 + 0.02 * i)), n=8)
    pdf = np.zeros(h * w, np.float32); prob = np.zeros(h * w, np.float32); fail = np.zeros(h * w, np.int32); total_power = C.c_float(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    t_pdf, t_alias = [], []
    for i in range(5):
        t0 = time.perf_counter()
        capi.check(L.rs_build_envmap_pdf(w, h, p(e), p(pdf)))
        t1 = time.perf_counter()
        capi.check(L.rs_build_alias_table(h * w, p(pdf), p(prob), p(fail), C.byref(total_power)))
        t2 = time.perf_counter()
        t_pdf.append((t1 - t0) * 1e3); t_alias.append((t2 - t1) * 1e3)
    pdf_ms, alias_ms = float(np.median(t_pdf)), float(np.median(t_alias))
    env_sizes["%dx%d" % (w, h)] = dict(total=total, pdf=round(pdf_ms, 4), alias_table=round(alias_ms, 4),
                                       staging_copies_light_tables=round(total["median"] - pdf_ms - alias_ms, 4))
    s.destroy()


def period(edit):
    cam = capi.camera_update(sd.camera(W, H))
    base = sd.camera_args["position"]
    gbuf, restir = capi.GBuffer(W, H), capi.ReSTIR(W, H)
    image = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
    pbo = torch.zeros((W * H, 4), dtype=torch.uint8, device="cuda")
    records = [material_records(i) for i in range(16)]       # prepared outside the timed region

    def frame(f):
        if edit:
            scene.set_materials(plain, records[f % len(records)])
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
    return (time.perf_counter() - t0) / args.frames * 1e3


capi.set_sync(False)
capi.prepare_streams()
none, every = [], []
for r in range(args.repeats):
    none.append(round(period(False), 4))
    every.append(round(period(True), 4))
capi.synchronize()
capi.set_sync(True)
print(json.dumps(dict(width=W, height=H, frames=args.frames, triangles=int(len(sd.material_ids)), lights=int(desc["num_lights"]),
                      materials_edited=int(len(plain)), host_ms=host, environment_edit_host_ms=env_sizes,
                      ms_per_frame=dict(no_edits=none, materials_edit_every_frame=every),
                      scene_build_ms=round(build_ms, 1), scene_create_from_host_desc_ms=[round(x, 1) for x in create])))
