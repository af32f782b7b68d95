#!/usr/bin/env python3
"""tools/primary_cut_info.py [3|5] [list cap] -- footprint and build time of the primary cuts and leaf lists (restir_amd/csrc/rs_cuts.h) on a
bench scene at 1080p.  Synchronous frames of a still camera: frame 1 builds both (its time minus frame 2's is the build), the frames after
it walk them.  RS_PRIMARY_LEAF_LISTS=0 gives the cuts' build alone."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401  (its HIP runtime first)
from restir_amd import capi, scenes

W, H = 1920, 1080
config = int(sys.argv[1]) if len(sys.argv) > 1 else 3
capi.init(0)
sd = scenes.bistro_class(seed=2, scale=1.0) if config == 5 else scenes.sponza_class(seed=1, scale=1.0)
scene = capi.Scene(sd.vertices, sd.normals, sd.texcoords, sd.material_ids, sd.materials)
cam = capi.camera_update(sd.camera(W, H))
gbuf, restir = capi.GBuffer(W, H), capi.ReSTIR(W, H)
image = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
if len(sys.argv) > 2:
    restir.set_primary_leaf_list_cap(int(sys.argv[2]))
capi.set_sync(True)
ms = []
for frame in range(6):
    capi.synchronize()
    t0 = time.perf_counter()
    gbuf.render(scene, cam)
    restir.direct(scene, cam, gbuf, image.data_ptr(), 0, frame, 3)
    gbuf.update(cam)
    capi.synchronize()
    ms.append((time.perf_counter() - t0) * 1e3)
info = restir.primary_cut_info()
with_cut = info["cells"] - info["without_cut"]
print("config %d: %d triangles, %dx%d: %d blocks of 32x8 pixels, %d without a cut; %d records = %.1f MB (36 B each, + 8 B per block), "
      "mean cut %.0f records" % (config, sd.num_prims, W, H, info["cells"], info["without_cut"], info["records"],
                                 (info["records"] * 36 + info["cells"] * 8) / 1e6, info["records"] / max(with_cut, 1)))
lists = restir.primary_leaf_list_info()
with_list = lists["tiles"] - lists["without_list"]
print("config %d: leaf lists: %d tiles of 8x8 pixels, %d without a list; %d records = %.1f MB (68 B each, + 8 B per tile), mean list %.1f records, "
      "%.1f per tile; arena %.1f MB; lists walked: %s" % (config, lists["tiles"], lists["without_list"], lists["records"],
      (lists["records"] * 68 + lists["tiles"] * 8) / 1e6, lists["records"] / max(with_list, 1), lists["records"] / max(lists["tiles"], 1),
      lists["tiles"] * 32 * 68 / 1e6, lists["used"]))
print("config %d: synchronous frame times (ms): %s; the build (frame 1 minus frame 2): %.2f ms; cuts walked: %s" %
      (config, " ".join("%.2f" % t for t in ms), ms[1] - ms[2], info["used"]))
