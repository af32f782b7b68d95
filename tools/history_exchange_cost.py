#!/usr/bin/env python3
"""tools/history_exchange_cost.py -- what one rs_strips_exchange_history costs a middle rank of an 8-way split of 1080p: the host
time to enqueue it and the time the library stream spends on it, over a stream-ordered transport that moves nothing (every packing
and unpacking copy or launch of a real exchange is made; RCCL's own group is not, and nothing travels: only the TIMES mean something).

    TRACK=0   the untracked message (60 B/px): seven hipMemcpyAsync calls to pack the own rows and seven per peer to unpack
    TRACK=1   rs_strips_set_light_tracking(strips, 1), 64 B/px: one launch of the copy kernel to pack and one per peer to unpack

Prints one line per repetition and the median; REPS (default 7) repetitions of CALLS (default 300) exchanges each.
  host enqueue   wall clock around the calls alone (they only enqueue)
  stream span    device events on the library stream around the same calls: what the stream was occupied for, idle gaps between
                 the copies included when the host is the slower side
  wall           wall clock until the stream has drained
"""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from restir_amd import capi, scenes

W, H, WORLD, RANK = 1920, 1080, 8, 3
TRACK = os.environ.get("TRACK", "0") == "1"
REPS, CALLS = int(os.environ.get("REPS", "7")), int(os.environ.get("CALLS", "300"))

capi.init(0)
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
capi.set_stream(stream.cuda_stream)
sd = scenes.sponza_class(seed=1, scale=0.1)            # the exchange moves planes: what they hold does not matter, one frame fills them
scene = capi.Scene(sd.vertices, sd.normals, sd.texcoords, sd.material_ids, sd.materials)
cam = capi.camera_update(sd.camera(W, H))
capi.set_sync(False)
noop = lambda p, n, peer: None
comm = capi.Comm(RANK, WORLD, noop, noop, None, None, stream_ordered=True)
drv = capi.Strips(comm, W, H)
gbuf, restir = capi.GBuffer(W, H), capi.ReSTIR(W, H)
if TRACK:
    restir.set_light_tracking(True)
    drv.set_light_tracking(True)
image = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
drv.frame(restir, scene, cam, gbuf, image.data_ptr(), 0, 0, 3)
gbuf.update(cam)
for _ in range(50):
    drv.exchange_history(restir, gbuf)
capi.synchronize(); torch.cuda.synchronize()
rows = []
for rep in range(REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    t0 = time.perf_counter()
    for _ in range(CALLS):
        drv.exchange_history(restir, gbuf)
    t1 = time.perf_counter()
    e1.record(stream)
    capi.synchronize(); torch.cuda.synchronize()
    t2 = time.perf_counter()
    rows.append(((t1 - t0) / CALLS * 1e3, e0.elapsed_time(e1) / CALLS, (t2 - t0) / CALLS * 1e3))
    print("track %d rep %d: host enqueue %.4f ms, stream span %.4f ms, wall %.4f ms per exchange" % ((int(TRACK), rep) + rows[-1]), flush=True)
print("track %d median of %d x %d (rank %d of %d, rows %d): host enqueue %.4f ms, stream span %.4f ms, wall %.4f ms per exchange" % (
    int(TRACK), REPS, CALLS, RANK, WORLD, drv.y1 - drv.y0, *[statistics.median(r[i] for r in rows) for i in range(3)]), flush=True)
drv.destroy(); comm.destroy()
