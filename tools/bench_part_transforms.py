#!/usr/bin/env python3
"""tools/bench_part_transforms.py [CONFIG ...] -- what rs_scene_set_part_transforms costs on the scenes of BASELINE config 3 (Sponza-class)
and 5 (Bistro-class), next to rs_scene_set_geometry of the same triangles already baked on the host, alternating in one process.

For 1 part of 1 triangle, parts of 256 triangles covering 1 % of the scene, and one part covering every triangle:
  T  ONE rs_scene_set_part_transforms: stream time (two events on the library stream around the call, device otherwise idle) and host time
     of the call, median of REPS with min and max; the bytes it staged
  G  the same for rs_scene_set_geometry with the arrays rs_bake_matrix gives for the same matrices (baked before the clock starts)
  K  rs_bake_matrix over the same triangles: the baking a caller of G does per frame and a caller of T no longer does
  D  the device's share of T and of G: the same two events, but with the stream kept busy (fills of a scratch array) for longer than the
     call's host time, so that everything the call enqueues is waiting when the stream gets to it; median of 5
and last the ratio G / T of the stream times for the all-triangles case, where the copy T replaces is largest.

Every matrix shrinks the scene a little about the middle of its root box (a different factor each repetition), so every baked vertex stays
inside that box whichever triangles a part holds.  Prints one line per figure and one JSON line per config, and writes the same to LOG
(default profiles/part_transforms.log).  Environment: REPS (default 15), LOG.
"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from restir_amd import capi, scenes

CONFIGS = [int(a) for a in sys.argv[1:]] or [3, 5]
assert all(c in (3, 5) for c in CONFIGS)
REPS = int(os.environ.get("REPS", "15"))
LOG = os.environ.get("LOG", os.path.join(ROOT, "profiles", "part_transforms.log"))
PART = 256
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
    """Scale by 1 - k * 1e-5 about `centre`: (4, 4) float32, [column][row]."""
    s = 1.0 - 1e-5 * k
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
    say("%s  %s, %-22s stream %.3f ms (min %.3f, max %.3f), host %.3f ms (min %.3f, max %.3f); median of %d%s"
        % (tag, what, label + ":", r["stream_ms"], r["stream_ms_min"], r["stream_ms_max"], r["host_ms"], r["host_ms_min"], r["host_ms_max"], REPS, extra))


for config in CONFIGS:
    sd = scenes.bistro_class(seed=2, scale=1.0) if config == 5 else scenes.sponza_class(seed=1, scale=1.0)
    orig = np.ascontiguousarray(sd.vertices, np.float32).reshape(-1, 3, 3)
    normals = np.ascontiguousarray(sd.normals, np.float32).reshape(-1, 3, 3)
    n = len(orig)
    centre = (orig.reshape(-1, 3).min(0).astype(np.float64) + orig.reshape(-1, 3).max(0)) / 2
    say("config %d: %d triangles" % (config, n))
    scene = capi.Scene(orig, normals, sd.texcoords, sd.material_ids, sd.materials)
    rng = np.random.default_rng(config)
    some = np.sort(rng.choice(n, max(PART, n // 100 // PART * PART), replace=False)).astype(np.int32)
    cases = [("1 part of 1 triangle", [np.array([n // 2], np.int32)]),
             ("%d parts, 1 %% of all" % (len(some) // PART), [some[i:i + PART] for i in range(0, len(some), PART)]),
             ("1 part of all triangles", [np.arange(n, dtype=np.int32)])]
    result = {"config": config, "triangles": n, "reps": REPS}
    scene.set_geometry(np.array([0], np.int32), orig[:1], normals[:1])      # the first edit builds the refit's tables and the version ring
    capi.synchronize()
    for label, parts in cases:
        scene.define_parts(parts)
        ids = np.concatenate(parts)
        part_ids = np.arange(len(parts), dtype=np.int32)
        rest_v, rest_n = orig[ids].reshape(-1, 3), normals[ids].reshape(-1, 3)
        t_rows, g_rows, k_rows, staged = [], [], [], [0, 0]
        for rep in range(REPS + 1):                          # (the first pair grows the staging buffers and is not counted)
            ms = np.stack([shrink(centre, 1 + 2 * rep)] * len(parts))
            t = timed(lambda: scene.set_part_transforms(part_ids, ms))
            staged[0] = scene.staged_bytes()
            m2 = shrink(centre, 2 + 2 * rep)
            t0 = time.perf_counter()
            bv, bn = capi.bake_matrix(m2, rest_v, rest_n)
            k = (time.perf_counter() - t0) * 1e3
            g = timed(lambda: scene.set_geometry(ids, bv, bn))
            staged[1] = scene.staged_bytes()
            if rep:
                t_rows.append(t); g_rows.append(g); k_rows.append(k)
        rt, rg = stats(t_rows), stats(g_rows)
        rt["staged_bytes"], rg["staged_bytes"] = staged
        bake_ms = float(np.median(k_rows))
        line("T", "rs_scene_set_part_transforms", label, rt, "; %d bytes staged" % staged[0])
        line("G", "rs_scene_set_geometry       ", label, rg, "; %d bytes staged" % staged[1])
        dt = device_share(lambda: scene.set_part_transforms(part_ids, ms), rt["host_ms_max"])
        dg = device_share(lambda: scene.set_geometry(ids, bv, bn), rg["host_ms_max"])
        rt["device_ms"], rg["device_ms"] = dt[0], dg[0]
        say("D  device share, %-22s rs_scene_set_part_transforms %.3f ms (min %.3f, max %.3f), rs_scene_set_geometry %.3f ms (min %.3f, max %.3f); median of 5"
            % (label + ":", dt[0], dt[1], dt[2], dg[0], dg[1], dg[2]))
        say("K  rs_bake_matrix over the same %d triangles: %.3f ms (median of %d; min %.3f, max %.3f)" % (len(ids), bake_ms, REPS, min(k_rows), max(k_rows)))
        result[label] = {"triangles": int(len(ids)), "parts": len(parts), "part_transforms": rt, "set_geometry": rg, "bake_matrix_ms": bake_ms}
    allr = result[cases[2][0]]
    result["all_stream_ratio_geometry_over_transforms"] = allr["set_geometry"]["stream_ms"] / allr["part_transforms"]["stream_ms"]
    say("all triangles: stream time of rs_scene_set_geometry / rs_scene_set_part_transforms = %.3f" % result["all_stream_ratio_geometry_over_transforms"])
    say(json.dumps(result))
    scene.define_parts([])
    scene.destroy()
    del scene
log.close()
