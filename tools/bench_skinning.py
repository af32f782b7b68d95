#!/usr/bin/env python3
"""tools/bench_skinning.py -- what rs_scene_set_bone_transforms costs on the scene of BASELINE config 3 (Sponza-class), next to
rs_scene_set_geometry of the same triangles already skinned on the host (how a caller did the same job before), alternating in one process.

A skin of 64 bones over 256, 4 096 and 65 536 listed triangles (random ids; every corner 1 to 4 non-zero weights on random bones), with the
partial refit off and on:
  B  ONE rs_scene_set_bone_transforms of all 64 bones: stream time (two events on the library stream around the call, device otherwise
     idle) and host time of the call, median of REPS with min and max; the bytes it staged
  G  the same for rs_scene_set_geometry with the arrays rs_skin_corners gives for the same palette (skinned before the clock starts)
  K  rs_skin_corners over the same triangles: the skinning a caller of G does per frame.  (A caller of B does not, but the library does it
     once inside the call, for its checks and its host tables: it is part of B's host time.)
  D  the device's share of B and of G: the same two events, but with the stream kept busy (fills of a scratch array) for longer than the
     call's host time, so that everything the call enqueues is waiting when the stream gets to it; median of 5

Every bone matrix shrinks the scene a little about the middle of its root box (a different factor per bone and repetition), so every blend
of them keeps every vertex inside that box.  Prints one line per figure and one JSON line, and writes the same to LOG (default
profiles/skinning.log).  Environment: REPS (default 15), LOG.
"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from restir_amd import capi, scenes

REPS = int(os.environ.get("REPS", "15"))
LOG = os.environ.get("LOG", os.path.join(ROOT, "profiles", "skinning.log"))
BONES = 64
SIZES = (256, 4096, 65536)
log = open(LOG, "w")


def say(text):
    print(text, flush=True)
    log.write(text + "\n"); log.flush()


capi.init(0)
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
capi.set_stream(stream.cuda_stream)
capi.set_sync(False)
capi.prepare_streams()


def shrink(centre, k):
    """Scale by 1 - k * 1e-6 about `centre`: (4, 4) float32, [column][row]."""
    s = 1.0 - 1e-6 * k
    m = np.eye(4)
    m[:3, :3] *= s
    m[:3, 3] = np.asarray(centre, np.float64) * (1.0 - s)
    return np.ascontiguousarray(m.T.astype(np.float32))


def timed(call):
    capi.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    t = time.perf_counter()
    call()
    host = (time.perf_counter() - t) * 1e3
    e1.record(stream)
    capi.synchronize()
    return e0.elapsed_time(e1), host


ballast = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
fill_ms = min(timed(lambda: [ballast.fill_(0.0) for _ in range(50)])[0] for _ in range(3)) / 50


def device_share(call, host_ms):
    out = []
    for _ in range(5):
        capi.synchronize()
        for _ in range(int(1.5 * host_ms / fill_ms) + 16):
            ballast.fill_(0.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        capi.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), float(min(out)), float(max(out))


def stats(rows):
    a = np.asarray(rows)
    return {"stream_ms": float(np.median(a[:, 0])), "stream_ms_min": float(a[:, 0].min()), "stream_ms_max": float(a[:, 0].max()),
            "host_ms": float(np.median(a[:, 1])), "host_ms_min": float(a[:, 1].min()), "host_ms_max": float(a[:, 1].max())}


def line(tag, what, label, r, extra=""):
    say("%s  %s, %-34s stream %.3f ms (min %.3f, max %.3f), host %.3f ms (min %.3f, max %.3f); median of %d%s"
        % (tag, what, label + ":", r["stream_ms"], r["stream_ms_min"], r["stream_ms_max"], r["host_ms"], r["host_ms_min"], r["host_ms_max"], REPS, extra))


sd = scenes.sponza_class(seed=1, scale=1.0)
orig = np.ascontiguousarray(sd.vertices, np.float32).reshape(-1, 3, 3)
normals = np.ascontiguousarray(sd.normals, np.float32).reshape(-1, 3, 3)
n = len(orig)
centre = (orig.reshape(-1, 3).min(0).astype(np.float64) + orig.reshape(-1, 3).max(0)) / 2
say("config 3: %d triangles, %d bones" % (n, BONES))
result = {"config": 3, "triangles": n, "bones": BONES, "reps": REPS, "cases": []}
bone_ids = np.arange(BONES, dtype=np.int32)
for partial in (False, True):
    scene = capi.Scene(orig, normals, sd.texcoords, sd.material_ids, sd.materials)
    scene.set_partial_refit(partial)
    scene.set_geometry(np.array([0], np.int32), orig[:1], normals[:1])      # the first edit builds the refit's tables (a whole refit)
    capi.synchronize()
    for size in SIZES:
        if size > n:
            say("skipped: %d listed triangles, the scene has %d" % (size, n))
            continue
        rng = np.random.default_rng(size)
        ids = np.sort(rng.choice(n, size, replace=False)).astype(np.int32)
        b = rng.integers(0, BONES, (size * 3, 4)).astype(np.int32)
        w = rng.uniform(0.1, 1.0, (size * 3, 4))
        w[np.argsort(rng.random((size * 3, 4)), axis=1) >= rng.integers(1, 5, size * 3)[:, None]] = 0.0
        w = (w / w.sum(1, keepdims=True)).astype(np.float32)
        rest_v, rest_n = orig[ids], normals[ids]
        scene.define_skin(BONES, ids, b, w, rest_v, rest_n)
        label = "%d triangles, partial refit %s" % (size, "on" if partial else "off")
        b_rows, g_rows, k_rows, staged = [], [], [], [0, 0]
        before = scene.refit_counts()
        for rep in range(REPS + 1):                          # (the first pair grows the staging buffers and is not counted)
            ms = np.stack([shrink(centre, 1 + (2 * rep) * BONES + k) for k in range(BONES)])
            t = timed(lambda: scene.set_bone_transforms(bone_ids, ms))
            staged[0] = scene.staged_bytes()
            m2 = np.stack([shrink(centre, 1 + (2 * rep + 1) * BONES + k) for k in range(BONES)])
            t0 = time.perf_counter()
            sv, sn = capi.skin_corners(m2, rest_v, rest_n, b, w)
            k_ms = (time.perf_counter() - t0) * 1e3
            g = timed(lambda: scene.set_geometry(ids, sv, sn))
            staged[1] = scene.staged_bytes()
            if rep:
                b_rows.append(t); g_rows.append(g); k_rows.append(k_ms)
        after = scene.refit_counts()
        rb, rg = stats(b_rows), stats(g_rows)
        rb["staged_bytes"], rg["staged_bytes"] = staged
        line("B", "rs_scene_set_bone_transforms", label, rb, "; %d bytes staged" % staged[0])
        line("G", "rs_scene_set_geometry       ", label, rg, "; %d bytes staged" % staged[1])
        db = device_share(lambda: scene.set_bone_transforms(bone_ids, ms), rb["host_ms_max"])
        dg = device_share(lambda: scene.set_geometry(ids, sv, sn), rg["host_ms_max"])
        rb["device_ms"], rg["device_ms"] = db[0], dg[0]
        say("D  device share, %-34s rs_scene_set_bone_transforms %.3f ms (min %.3f, max %.3f), rs_scene_set_geometry %.3f ms (min %.3f, max %.3f); median of 5"
            % (label + ":", db[0], db[1], db[2], dg[0], dg[1], dg[2]))
        say("K  rs_skin_corners over the same %d triangles: %.3f ms (median of %d; min %.3f, max %.3f); refits of the timed edits: %d whole, %d partial"
            % (size, float(np.median(k_rows)), REPS, min(k_rows), max(k_rows), after[0] - before[0], after[1] - before[1]))
        result["cases"].append({"triangles": size, "partial_refit": partial, "bone_transforms": rb, "set_geometry": rg,
                                "skin_corners_ms": float(np.median(k_rows)), "whole_refits": after[0] - before[0], "partial_refits": after[1] - before[1]})
    scene.define_skin(0, [], np.zeros((0, 3, 4), np.int32), np.zeros((0, 3, 4), np.float32))
    scene.destroy()
    del scene
say(json.dumps(result))
log.close()
