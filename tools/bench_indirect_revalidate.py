#!/usr/bin/env python3
"""tools/bench_indirect_revalidate.py [--parent-lib PATH] [--frames N] [--reps R] [--rounds K] -- what ReSTIR-GI's revalidation
(rs_restir_set_indirect_revalidation) costs, on the scene of BASELINE config 3 (Sponza-class) at 1080p, trace depth 4, reuse 1, still camera.

Every measurement runs in a child process of its own with a time limit; the driver opens no device, starts one child at a time and stops
at the first one that fails (no retries).  A child holds one scene and one rs_restir and measures one column: the switch off, or on.
With --parent-lib (the parent commit's librestir_hip.so, through RESTIR_HIP_LIB) the children go parent / in-tree off / in-tree on, K
rounds, and the parent once more: the base of "a frame without an edit costs what it cost" is the parent's library in the same
session, not this commit's own switch off.  A child measures:

  still    stream time of ONE rs_restir_indirect call in a frame without an edit: two events on the library stream around the call, the
           device idle before it (GBuffer::render finished); median, min and max of R calls.  launched counts the calls that launched
           k_revalidate_indirect and must be 0.
  edited   the same for the first call after a rigid part of 64 triangles that emit nothing moved by matrix
           (rs_scene_set_part_transforms); with the switch on the pass's counters { examined, stale, walked, occluded } of the last such call
  period   ms per frame over N frames of GBuffer::render, rs_restir_indirect, GBuffer::update enqueued without a wait, with no edit and
           with the part moved before every frame

Prints one JSON line per child and, last, one JSON line with every child's figures."""
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
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--part", type=int, default=64, help="triangles of the moved part")
ap.add_argument("--child-timeout", type=int, default=240)
ap.add_argument("--child", choices=("off", "on"), default=None, help=argparse.SUPPRESS)
args = ap.parse_args()

W, H, DEPTH = 1920, 1080, 4


def child():
    import ctypes as C

    import numpy as np
    import torch

    from restir_amd import capi, scenes
    from restir_amd.ctypes_structs import LIGHT

    capi.init(0)
    lib = capi.lib()
    have = hasattr(lib, "rs_restir_set_indirect_revalidation")
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    capi.set_stream(stream.cuda_stream)
    capi.set_sync(False)
    sd = scenes.sponza_class(seed=1, scale=1.0)
    v = sd.vertices.reshape(-1, 3, 3)
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    movable = np.nonzero(sd.materials["type"][sd.material_ids] != LIGHT)[0]
    far = np.abs((v[movable].mean(1) - (lo + hi) / 2) / (hi - lo)).max(1)
    part = movable[np.argsort(far, kind="stable")[:args.part]].astype(np.int32)       # the triangles nearest the scene's middle: an occluder
    swing = np.float32(0.02 * float((hi - lo)[0]))
    cam = capi.camera_update(sd.camera(W, H))
    image = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")

    class Run:
        def __init__(self, on):
            self.scene = capi.Scene(sd.vertices, sd.normals, sd.texcoords, sd.material_ids, sd.materials)
            self.scene.define_parts([part])
            self.gbuf, self.restir = capi.GBuffer(W, H), capi.ReSTIR(W, H)
            if on:
                self.restir.set_indirect_revalidation(True)
            self.on, self.f, self.moves, self.launched = on, 0, 0, 0

        def move(self):
            m = np.eye(4, dtype=np.float32)
            self.moves += 1
            m[3, 0] = swing * np.float32(np.sin(0.3 * self.moves))
            self.scene.set_part_transforms([0], m.reshape(1, 16))

        def indirect(self):
            capi.check(lib.rs_restir_indirect(self.restir.handle, self.scene.handle, C.byref(cam), self.gbuf.handle, image.data_ptr(), 0, self.f, 1, DEPTH, None))
            if have:
                self.launched += int(self.restir.indirect_revalidate_launched())      # (host only: no wait)

        def frame(self, edit=False, timed=False):
            if edit:
                self.move()
            self.gbuf.render(self.scene, cam)
            ms = None
            if timed:
                capi.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                self.indirect()
                e1.record(stream)
                capi.synchronize()
                ms = e0.elapsed_time(e1)
            else:
                self.indirect()
            self.gbuf.update(cam)
            self.f += 1
            return ms

        def period(self, edit):
            for _ in range(5):
                self.frame(edit)
            capi.synchronize()
            t = time.perf_counter()
            for _ in range(args.frames):
                self.frame(edit)
            capi.synchronize()
            return (time.perf_counter() - t) / args.frames * 1e3

    def summary(x):
        return dict(median=round(float(np.median(x)), 4), min=round(float(np.min(x)), 4), max=round(float(np.max(x)), 4))

    assert have or args.child == "off", "this library has no switch"
    out = dict(lib=os.environ.get("RESTIR_HIP_LIB", "in-tree"), has_switch=have, switch=args.child, width=W, height=H, depth=DEPTH, frames=args.frames, reps=args.reps,
               part_triangles=int(len(part)))
    on = args.child == "on"
    r = Run(on)
    for _ in range(10):
        r.frame()
    capi.synchronize()
    still, edited, stats = [], [], None
    for rep in range(args.reps):
        r.launched = 0
        still.append(r.frame(timed=True))
        assert r.launched == 0, "a frame without an edit launched the pass"
        edited.append(r.frame(edit=True, timed=True))
        if on:
            assert r.launched == 1
            stats = r.restir.indirect_revalidate_stats()
        r.frame()                                            # a still frame between the samples: the next still call follows no edit
    out.update(still_call_ms=summary(still), edited_call_ms=summary(edited),
               period_still_ms=round(r.period(False), 4), period_edit_every_frame_ms=round(r.period(True), 4), edited_call_counters=stats)
    capi.synchronize()
    capi.set_sync(True)
    print(json.dumps(out), flush=True)


def driver():
    mine = [("in-tree", "off"), ("in-tree", "on")]
    order = mine if not args.parent_lib else (([("parent", "off")] + mine) * args.rounds + [("parent", "off")])
    results = []
    for which, mode in order:
        env = dict(os.environ)
        env.pop("RESTIR_HIP_LIB", None)
        if which == "parent":
            env["RESTIR_HIP_LIB"] = os.path.abspath(args.parent_lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--frames", str(args.frames), "--reps", str(args.reps), "--part", str(args.part)]
        p = subprocess.run(cmd, env=env, timeout=args.child_timeout, stdout=subprocess.PIPE, text=True)      # a time limit of its own; raises when it runs out
        if p.returncode != 0:
            sys.exit("the %s child ended with status %d: nothing more is started" % (which, p.returncode))
        line = p.stdout.strip().splitlines()[-1]
        print(which, mode, line, flush=True)
        results.append(dict(which=which, **json.loads(line)))
    print(json.dumps(dict(children=results)))


if __name__ == "__main__":
    child() if args.child else driver()
