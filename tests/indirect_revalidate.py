"""Helpers of tests/test_indirect_revalidate_host.py and tests/test_gpu_indirect_revalidate.py: ReSTIR-GI's revalidation
(rs_restir_set_indirect_revalidation) restated in NumPy and composed with the CPU oracle, which knows nothing of it.

The rule: an rs_restir_indirect call that merges temporally (reuse & 1, not the first frame, not the call that allocated the reservoirs)
and whose scene took a geometry edit since the previous rs_restir_indirect call looks at every slot of the history buffer.  A slot is
examined iff its weight is finite and > 0 and xv != xs on some component.  "Everything" (an edit of the gap has left the ring, or another
scene): every examined slot is stale.  Otherwise: stale iff xs lies in a dirty box (closed); else walked iff the bounding box of xv -> xs
overlaps one; a walked segment is the edited oracle scene's test_occlusion(xv, xs) and one ray.  Stale slots and occluded walkers are
dropped: numSamples = 0, weight = 0, the sample fields stay.  Here that is a patch of o.restir.ind_last, after which the unmodified
oracle runs the frame.  The verdict depends on the slot alone, so no reader of a slot needs a group of its own."""
import numpy as np

from oracle import binding as ob
from tests import motion_vectors as mv
from tests.common import hip_scene, next_looper, oracle_scene
from tests.emitter_edits import edited_oracle_scene, scene_data
from tests.shadow_revalidate import DISPLACEMENT, TALL_BOX, DirtyRing, moved_box, segment_in_boxes  # noqa: F401

F = np.float32
DEPTH = 4
NOT_EXAMINED, STALE, WALK, KEPT = 0, 1, 2, 3
SIZES = {"full": (64, 48), "partial": (40, 24)}             # 3 072 slots fill their 256-lane blocks; 960 leave the last one partial
WARM = {"full": 10, "partial": 6}


def point_in_boxes(p, boxes):
    p = np.asarray(p, F).reshape(-1, 3)
    out = np.zeros(len(p), bool)
    with np.errstate(all="ignore"):
        for box in np.asarray(boxes, F).reshape(-1, 6):
            out |= ((box[:3] <= p) & (p <= box[3:])).all(1)
    return out


def classes(resv, boxes, everything=False):
    """The class of every slot of `resv` (INDIRECT_RESERVOIR_DTYPE): 0 not examined, 1 stale, 2 walk, 3 examined and kept."""
    W, xv, xs = resv["weight"], resv["xv"], resv["xs"]
    with np.errstate(all="ignore"):
        examined = np.isfinite(W) & (W > 0) & ~(xv == xs).all(1)
    if everything:
        stale, walk = examined, np.zeros(len(W), bool)
    else:
        stale = examined & point_in_boxes(xs, boxes)
        walk = examined & ~stale & segment_in_boxes(np.concatenate([xv, xs], 1), boxes)
    return np.where(stale, STALE, np.where(walk, WALK, np.where(examined, KEPT, NOT_EXAMINED))).astype(np.uint8)


def revalidate(scene, resv, boxes, everything=False):
    """(classes, occluded mask, dropped mask) of the history `resv` on the current oracle scene."""
    cls = classes(resv, boxes, everything)
    occluded = np.zeros(len(resv), bool)
    walk = cls == WALK
    if walk.any():
        occluded[walk] = scene.test_occlusion(np.concatenate([resv["xv"][walk], resv["xs"][walk]], 1)) != 0
    return cls, occluded, (cls == STALE) | occluded


def counts_of(cls, occluded):
    return int((cls != NOT_EXAMINED).sum()), int((cls == STALE).sum()), int((cls == WALK).sum()), int(occluded.sum())


def drop(resv, dropped):
    resv["numSamples"][dropped] = 0
    resv["weight"][dropped] = 0


class OracleGI:
    """GBuffer::render, ReSTIRIndirect, GBuffer::update on the oracle, looper = frame number (or the Sobol launcher's)."""

    def __init__(self, capi, sd, W, H, sobol=None, tracked=False):
        self.capi, self.sd, self.W, self.H, self.tracked = capi, sd, W, H, tracked
        self.scene = oracle_scene(sd)
        self.scene.set_sample_sequence(sobol)
        self.sobol_num = None if sobol is None else len(sobol)
        self.cam = ob.camera_update(sd.camera(W, H))
        self.gbuf, self.restir = ob.GBuffer(W, H), ob.ReSTIR(W, H)
        self.image = np.zeros((W * H, 3), F)
        self.looper, self.rays = 0, 0
        self.prev = np.array(self.scene.vertices, F).reshape(-1, 3, 3).copy()

    def set_geometry(self, ids, v, n=None):
        self.scene = edited_oracle_scene(self.capi, self.scene, ids, v, n)

    def set_camera_position(self, pos):
        for i in range(3):
            self.cam.position[i] = float(pos[i])
        ob.camera_update(self.cam)

    def render(self):
        self.gbuf.render(self.scene, self.cam)
        if self.tracked:
            self.gbuf.motion[:] = mv.object_motion_plane(self.scene, self.prev, self.cam, self.gbuf.c.lastCamera, self.W, self.H)

    def finish(self, reuse, extra_rays=0):
        self.image[:] = 0
        self.rays = self.restir.indirect(self.scene, self.cam, self.gbuf, self.image, 0, self.looper, reuse, DEPTH) + extra_rays
        self.looper = next_looper(self.looper, self.sobol_num)
        self.gbuf.update(self.cam)
        if self.tracked:
            self.prev = np.array(self.scene.vertices, F).reshape(-1, 3, 3).copy()

    def state(self):
        return dict(image=self.image.copy(), rays=self.rays, written=self.restir.ind_last.copy(), history=self.restir.ind_reservoir.copy())


class HipGI:
    """The same loop on the library."""

    def __init__(self, capi, sd, W, H, sobol=None, tracked=False, scene=None):
        import torch
        self.capi, self.sd, self.W, self.H, self.tracked = capi, sd, W, H, tracked
        self.scene = scene or hip_scene(capi, sd)
        if scene is None:
            self.scene.set_sample_sequence(sobol)
            if tracked:
                self.scene.set_motion_tracking(True)
        self.sobol_num = None if sobol is None else len(sobol)
        self.cam = capi.camera_update(sd.camera(W, H))
        self.gbuf, self.restir = capi.GBuffer(W, H), capi.ReSTIR(W, H)
        self.image = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
        self.looper, self.rays = 0, 0

    def set_camera_position(self, pos):
        for i in range(3):
            self.cam.position[i] = float(pos[i])
        self.capi.camera_update(self.cam)

    def frame(self, reuse):
        self.gbuf.render(self.scene, self.cam)
        self.image.zero_()
        self.rays = self.restir.indirect(self.scene, self.cam, self.gbuf, self.image.data_ptr(), 0, self.looper, reuse, DEPTH)
        self.looper = next_looper(self.looper, self.sobol_num)
        self.gbuf.update(self.cam)
        if self.tracked:
            self.scene.advance_motion()

    def state(self):
        """The image, the rays, the buffer the call wrote and the history it merged from (after the pass)."""
        return dict(image=self.image.cpu().numpy(), rays=self.rays, written=self.restir.download_indirect(1), history=self.restir.download_indirect(0))


class Pair:
    """An oracle loop and a library loop with indirect revalidation `on`, frame by frame."""

    def __init__(self, capi, name, size, sobol=None, tracked=False, on=True, scene=None):
        W, H = SIZES[size] if isinstance(size, str) else size
        self.capi, self.sd, self.on = capi, scene_data(name), on
        self.o = OracleGI(capi, self.sd, W, H, sobol=sobol, tracked=tracked)
        self.h = HipGI(capi, self.sd, W, H, sobol=sobol, tracked=tracked, scene=scene)
        if on:
            self.h.restir.set_indirect_revalidation(True)
        self.ring, self.seen_edits, self.same_scene, self.called = DirtyRing(), 0, True, False
        self.cls = self.occluded = self.dropped = None

    def edit(self, ids, v, n=None, how="set_geometry", library=True):
        """how: set_geometry, set_triangles, or (part ids, matrices) for set_part_transforms, whose baked arrays are ids / v / n."""
        self.ring.edit(self.o.scene.vertices, ids, v)
        self.o.set_geometry(ids, v, n)
        if not library:
            return
        if isinstance(how, tuple):
            self.h.scene.set_part_transforms(*how)
        else:
            getattr(self.h.scene, how)(ids, v, n)

    def set_camera_position(self, p):
        self.o.set_camera_position(p); self.h.set_camera_position(p)

    def frame(self, reuse=1):
        """Returns (library's state, oracle's state, library's (launched, counters), restated (launched, counters))."""
        o, h = self.o, self.h
        h.frame(reuse)
        o.render()
        merges = self.called and not o.restir.first and bool(reuse & 1)
        launch, everything, boxes = self.ring.choose(self.seen_edits, self.same_scene)
        launched, counts, walked = False, (0, 0, 0, 0), 0
        self.cls = self.occluded = self.dropped = None
        if self.on and merges and launch:
            self.before = o.restir.ind_last.copy()
            self.cls, self.occluded, self.dropped = revalidate(o.scene, o.restir.ind_last, boxes, everything)
            drop(o.restir.ind_last, self.dropped)
            launched, counts = True, counts_of(self.cls, self.occluded)
            walked = counts[2]
        o.finish(reuse, walked)                             # every walked segment is one ray
        self.seen_edits, self.same_scene, self.called = self.ring.edits, True, True
        return h.state(), o.state(), (h.restir.indirect_revalidate_launched(), h.restir.indirect_revalidate_stats()), (launched, counts)
