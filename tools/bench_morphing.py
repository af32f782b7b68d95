#!/usr/bin/env python3
"""tools/bench_morphing.py -- what rs_scene_set_morph_weights and rs_scene_set_skin_pose cost on the scene of BASELINE config 3
(Sponza-class), next to rs_scene_set_geometry of the same triangles already morphed (and skinned) on the host -- how a caller did the
same job before --, alternating in one process.

16 targets that each touch a quarter of the corners (a corner has 0 to 16 entries, 4 on average) over 256, 4 096 and 65 536 listed
triangles (random ids), with the partial refit off and on:
  M  ONE rs_scene_set_morph_weights of all 16 targets: stream time (two events on the library stream around the call, device otherwise
     idle) and host time of the call, median of REPS with min and max; the bytes it staged
  G  the same for rs_scene_set_geometry with the arrays rs_morph_corners gives for the same weights (morphed before the clock starts)
  K  rs_morph_corners over the same triangles, one thread: the morphing a caller of G does per frame (the library does it once inside M)
  D  the device's share of M and of G: the same two events with the stream kept busy for longer than the call's host time; median of 5
  U  D of M on a table of the same size in which EVERY corner has exactly 4 entries: M's D minus this is what the differing entry
     counts of a wave's lanes cost
and on a skin of 64 bones over the same triangles, with the same morph on its corners:
  P  rs_scene_set_skin_pose of all bones and all targets, against G of rs_skin_corners(rs_morph_corners(rest))
  Z  rs_scene_set_bone_transforms on the skin WITH the morph, every weight 0: the fused kernel with nothing to add
  B  rs_scene_set_bone_transforms on the same skin WITHOUT a morph: k_skin.  D of Z minus D of B is the fused kernel's own overhead.

Every delta points at the middle of the root box and every bone matrix shrinks the scene a little about it, so every vertex stays inside
that box.  Prints one line per figure and one JSON line, and writes the same to LOG (default profiles/morphing.log).  Environment: REPS
(default 15), LOG.
"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from restir_amd import capi, scenes

REPS = int(os.environ.get("REPS", "15"))
LOG = os.environ.get("LOG", os.path.join(ROOT, "profiles", "morphing.log"))
TARGETS, BONES = 16, 64
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


def dline(tag, label, pairs):
    say("%s  device share, %-34s %s; median of 5" % (tag, label + ":", ", ".join("%s %.3f ms (min %.3f, max %.3f)" % ((k,) + v) for k, v in pairs)))


def table(rng, corners, rest, centre, uniform):
    """By target: each of the 16 targets on a random quarter of the corners, or (uniform) on the corners of one residue mod 4 of four, so
    that every corner has exactly 4 entries.  Deltas of about 1e-4 of the way to `centre`; small normal deltas."""
    first, ec = [0], []
    for t in range(TARGETS):
        c = np.flatnonzero((np.arange(corners) + t) % 4 == 0) if uniform else np.flatnonzero(rng.random(corners) < 0.25)
        ec.append(c)
        first.append(first[-1] + len(c))
    ec = np.concatenate(ec).astype(np.int32)
    dp = ((centre - rest.reshape(-1, 3)[ec].astype(np.float64)) * rng.uniform(0.5e-4, 1e-4, (len(ec), 1))).astype(np.float32)
    dn = rng.uniform(-1e-3, 1e-3, (len(ec), 3)).astype(np.float32)
    return np.array(first, np.int32), ec, dp, dn


sd = scenes.sponza_class(seed=1, scale=1.0)
orig = np.ascontiguousarray(sd.vertices, np.float32).reshape(-1, 3, 3)
normals = np.ascontiguousarray(sd.normals, np.float32).reshape(-1, 3, 3)
n = len(orig)
centre = (orig.reshape(-1, 3).min(0).astype(np.float64) + orig.reshape(-1, 3).max(0)) / 2
say("config 3: %d triangles, %d targets, %d bones" % (n, TARGETS, BONES))
result = {"config": 3, "triangles": n, "targets": TARGETS, "bones": BONES, "reps": REPS, "cases": []}
target_ids, bone_ids = np.arange(TARGETS, dtype=np.int32), np.arange(BONES, dtype=np.int32)
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
        rest_v, rest_n = orig[ids], normals[ids]
        tab = table(rng, size * 3, rest_v, centre, False)
        flat = table(rng, size * 3, rest_v, centre, True)
        per_corner = np.bincount(tab[1], minlength=size * 3)
        label = "%d triangles, partial refit %s" % (size, "on" if partial else "off")
        say("table, %s: %d entries, per corner min %d, mean %.2f, max %d; uniform table: %d entries"
            % (label, len(tab[1]), per_corner.min(), per_corner.mean(), per_corner.max(), len(flat[1])))
        weights_of = lambda k: np.random.default_rng(k).uniform(0.1, 1.0, TARGETS).astype(np.float32)

        # ---- the scene's own morph ----
        scene.define_morph(ids, *tab, rest_v, rest_n)
        m_rows, g_rows, k_rows, staged = [], [], [], [0, 0]
        before = scene.refit_counts()
        for rep in range(REPS + 1):                          # (the first pair grows the staging buffers and is not counted)
            w = weights_of(2 * rep)
            t = timed(lambda: scene.set_morph_weights(target_ids, w))
            staged[0] = scene.staged_bytes()
            w2 = weights_of(2 * rep + 1)
            t0 = time.perf_counter()
            mv, mn = capi.morph_corners(*tab, w2, rest_v, rest_n)
            k_ms = (time.perf_counter() - t0) * 1e3
            g = timed(lambda: scene.set_geometry(ids, mv, mn))
            staged[1] = scene.staged_bytes()
            if rep:
                m_rows.append(t); g_rows.append(g); k_rows.append(k_ms)
        after = scene.refit_counts()
        rm, rg = stats(m_rows), stats(g_rows)
        rm["staged_bytes"], rg["staged_bytes"] = staged
        line("M", "rs_scene_set_morph_weights", label, rm, "; %d bytes staged" % staged[0])
        line("G", "rs_scene_set_geometry     ", label, rg, "; %d bytes staged" % staged[1])
        dm = device_share(lambda: scene.set_morph_weights(target_ids, w), rm["host_ms_max"])
        dg = device_share(lambda: scene.set_geometry(ids, mv, mn), rg["host_ms_max"])
        scene.define_morph(ids, *flat, rest_v, rest_n)
        scene.set_morph_weights(target_ids, w)
        du = device_share(lambda: scene.set_morph_weights(target_ids, w2), rm["host_ms_max"])
        scene.define_morph([], [0], [], np.zeros((0, 3), np.float32))
        rm["device_ms"], rg["device_ms"], rm["device_ms_uniform_table"] = dm[0], dg[0], du[0]
        dline("D", label, [("rs_scene_set_morph_weights", dm), ("rs_scene_set_geometry", dg)])
        dline("U", label, [("rs_scene_set_morph_weights, 4 entries on every corner", du)])
        say("K  rs_morph_corners over the same %d triangles: %.3f ms (median of %d; min %.3f, max %.3f); refits of the timed edits: %d whole, %d partial"
            % (size, float(np.median(k_rows)), REPS, min(k_rows), max(k_rows), after[0] - before[0], after[1] - before[1]))
        case = {"triangles": size, "partial_refit": partial, "entries": int(len(tab[1])), "morph_weights": rm, "set_geometry": rg,
                "morph_corners_ms": float(np.median(k_rows)), "whole_refits": after[0] - before[0], "partial_refits": after[1] - before[1]}

        # ---- the same morph under a skin of 64 bones ----
        b = rng.integers(0, BONES, (size * 3, 4)).astype(np.int32)
        bw = rng.uniform(0.1, 1.0, (size * 3, 4))
        bw[np.argsort(rng.random((size * 3, 4)), axis=1) >= rng.integers(1, 5, size * 3)[:, None]] = 0.0
        bw = (bw / bw.sum(1, keepdims=True)).astype(np.float32)
        palette = lambda k: np.stack([shrink(centre, 1 + k * BONES + j) for j in range(BONES)])
        scene.define_skin(BONES, ids, b, bw, rest_v, rest_n)
        scene.define_skin_morph(*tab)
        p_rows, g_rows, z_rows, staged = [], [], [], [0, 0]
        zeros = np.zeros(TARGETS, np.float32)
        for rep in range(REPS + 1):
            ms, w = palette(3 * rep), weights_of(2 * rep)
            t = timed(lambda: scene.set_skin_pose(bone_ids, ms, target_ids, w))
            staged[0] = scene.staged_bytes()
            m2, w2 = palette(3 * rep + 1), weights_of(2 * rep + 1)
            sv, sn = capi.skin_corners(m2, *capi.morph_corners(*tab, w2, rest_v, rest_n), b, bw)
            g = timed(lambda: scene.set_geometry(ids, sv, sn))
            staged[1] = scene.staged_bytes()
            if rep:
                p_rows.append(t); g_rows.append(g)
        rp, rg2 = stats(p_rows), stats(g_rows)
        rp["staged_bytes"], rg2["staged_bytes"] = staged
        line("P", "rs_scene_set_skin_pose    ", label, rp, "; %d bytes staged" % staged[0])
        line("G", "rs_scene_set_geometry     ", label, rg2, "; %d bytes staged" % staged[1])
        dp_ = device_share(lambda: scene.set_skin_pose(bone_ids, ms, target_ids, w), rp["host_ms_max"])
        dg2 = device_share(lambda: scene.set_geometry(ids, sv, sn), rg2["host_ms_max"])
        scene.set_skin_pose(bone_ids, ms, target_ids, zeros)
        for rep in range(REPS + 1):
            m3 = palette(3 * rep + 2)
            t = timed(lambda: scene.set_bone_transforms(bone_ids, m3))
            if rep:
                z_rows.append(t)
        rz = stats(z_rows)
        dz = device_share(lambda: scene.set_bone_transforms(bone_ids, ms), rz["host_ms_max"])
        scene.define_skin_morph([0], [], np.zeros((0, 3), np.float32))
        b_rows = []
        for rep in range(REPS + 1):
            m3 = palette(3 * rep + 2)
            t = timed(lambda: scene.set_bone_transforms(bone_ids, m3))
            if rep:
                b_rows.append(t)
        rb = stats(b_rows)
        db = device_share(lambda: scene.set_bone_transforms(bone_ids, ms), rb["host_ms_max"])
        line("Z", "rs_scene_set_bone_transforms, morph defined, weights 0", label, rz)
        line("B", "rs_scene_set_bone_transforms, no morph defined        ", label, rb)
        dline("D", label, [("rs_scene_set_skin_pose", dp_), ("rs_scene_set_geometry", dg2), ("bone transforms with the morph at 0", dz),
                           ("bone transforms without a morph", db)])
        rp["device_ms"], rg2["device_ms"], rz["device_ms"], rb["device_ms"] = dp_[0], dg2[0], dz[0], db[0]
        case.update({"skin_pose": rp, "skin_pose_set_geometry": rg2, "bone_transforms_morph_at_zero": rz, "bone_transforms_no_morph": rb})
        result["cases"].append(case)
        scene.define_skin(0, [], np.zeros((0, 3, 4), np.int32), np.zeros((0, 3, 4), np.float32))
    scene.destroy()
    del scene
say(json.dumps(result))
log.close()
