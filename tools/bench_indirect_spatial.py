#!/usr/bin/env python3
"""tools/bench_indirect_spatial.py [--parent-lib PATH] [--reps R] [--rounds K] [--frames N] -- what ReSTIR-GI's spatial pass
(rs_restir_set_indirect_spatial) costs, on the scene of BASELINE config 3 (Sponza-class) at 1080p, trace depth 4, reuse 3, still camera.

Every measurement runs in a child process of its own with a time limit; the driver opens no device, starts one child at a time and stops
at the first one that fails (no retries).  A child holds one scene and one rs_restir and measures one column: the switch off, on at the
defaults (5 taps, radius 5), or on at 16 taps / radius 30.  With --parent-lib (the parent commit's librestir_hip.so, through
RESTIR_HIP_LIB) the children go parent / in-tree off / in-tree on / in-tree wide, K rounds, and the parent once more: the base of "with the
switch off a frame costs what it cost" is the parent's library in the same session, not this commit's own switch off.  A child measures:

  call     stream time of ONE rs_restir_indirect call: two events on the library stream around the call, the device idle before it
           (GBuffer::render finished); median, min and max of R calls after ten warm frames.  With the switch on: the pass's eight counters
           of the last call (walked winners: counters[6])
  period   ms per frame over N frames of GBuffer::render, rs_restir_indirect, GBuffer::update enqueued without a wait

Prints one JSON line per child and, last, one JSON line with every child's figures and the verdict on the switch-off frame: does the
in-tree median lie within the min-max of the parent's own children?"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--frames", type=int, default=40)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--child-timeout", type=int, default=240)
ap.add_argument("--child", choices=("off", "on", "wide"), default=None, help=argparse.SUPPRESS)
args = ap.parse_args()

W, H, DEPTH, REUSE = 1920, 1080, 4, 3
SETTINGS = {"on": (5, 5.0), "wide": (16, 30.0)}


def child():
    import ctypes as C

    import numpy as np
    import torch

    from restir_amd import capi, scenes

    capi.init(0)
    lib = capi.lib()
    have = hasattr(lib, "rs_restir_set_indirect_spatial")
    assert have or args.child == "off", "this library has no switch"
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    capi.set_stream(stream.cuda_stream)
    capi.set_sync(False)
    sd = scenes.sponza_class(seed=1, scale=1.0)
    cam = capi.camera_update(sd.camera(W, H))
    image = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
    scene = capi.Scene(sd.vertices, sd.normals, sd.texcoords, sd.material_ids, sd.materials)
    gbuf, restir = capi.GBuffer(W, H), capi.ReSTIR(W, H)
    if args.child != "off":
        restir.set_indirect_spatial(True, *SETTINGS[args.child])
    state = dict(f=0)

    def frame(timed=False):
        gbuf.render(scene, cam)
        ms = None
        if timed:
            capi.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
        capi.check(lib.rs_restir_indirect(restir.handle, scene.handle, C.byref(cam), gbuf.handle, image.data_ptr(), 0, state["f"], REUSE, DEPTH, None))
        if timed:
            e1.record(stream)
            capi.synchronize()
            ms = e0.elapsed_time(e1)
        gbuf.update(cam)
        state["f"] += 1
        return ms

    def summary(x):
        return dict(median=round(float(np.median(x)), 4), min=round(float(np.min(x)), 4), max=round(float(np.max(x)), 4))

    for _ in range(10):
        frame()
    capi.synchronize()
    calls = [frame(timed=True) for _ in range(args.reps)]
    counters = list(restir.indirect_spatial_stats()) if args.child != "off" else None
    for _ in range(5):
        frame()
    capi.synchronize()
    t = time.perf_counter()
    for _ in range(args.frames):
        frame()
    capi.synchronize()
    period = (time.perf_counter() - t) / args.frames * 1e3
    capi.set_sync(True)
    print(json.dumps(dict(lib=os.environ.get("RESTIR_HIP_LIB", "in-tree"), has_switch=have, switch=args.child, settings=SETTINGS.get(args.child), width=W, height=H,
                          depth=DEPTH, reuse=REUSE, reps=args.reps, frames=args.frames, call_ms=summary(calls), period_ms=round(period, 4), counters=counters)), flush=True)


def driver():
    mine = [("in-tree", "off"), ("in-tree", "on"), ("in-tree", "wide")]
    order = mine if not args.parent_lib else (([("parent", "off")] + mine) * args.rounds + [("parent", "off")])
    results = []
    for which, mode in order:
        env = dict(os.environ)
        env.pop("RESTIR_HIP_LIB", None)
        if which == "parent":
            env["RESTIR_HIP_LIB"] = os.path.abspath(args.parent_lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--frames", str(args.frames), "--reps", str(args.reps)]
        p = subprocess.run(cmd, env=env, timeout=args.child_timeout, stdout=subprocess.PIPE, text=True)      # a time limit of its own; raises when it runs out
        if p.returncode != 0:
            sys.exit("the %s child ended with status %d: nothing more is started" % (which, p.returncode))
        line = p.stdout.strip().splitlines()[-1]
        print(which, mode, line, flush=True)
        results.append(dict(which=which, **json.loads(line)))
    out = dict(children=results)
    parents = [r["call_ms"] for r in results if r["which"] == "parent"]
    offs = [r["call_ms"]["median"] for r in results if r["which"] == "in-tree" and r["switch"] == "off"]
    if parents:
        lo, hi = min(p["min"] for p in parents), max(p["max"] for p in parents)
        medians = [p["median"] for p in parents]
        out.update(parent_medians_ms=medians, parent_min_max_ms=[lo, hi], off_medians_ms=offs,
                   off_within_parent_repetitions=all(lo <= m <= hi for m in offs),       # the min-max of every timed call of the parent's children
                   off_within_parent_medians=all(min(medians) <= m <= max(medians) for m in offs))
    print(json.dumps(out))


if __name__ == "__main__":
    child() if args.child else driver()
