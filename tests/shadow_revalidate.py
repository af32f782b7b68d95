"""Helpers of tests/test_shadow_revalidate_host.py and tests/test_gpu_shadow_revalidate.py: shadow revalidation
(rs_restir_set_shadow_revalidation) restated in NumPy and composed with the CPU oracle, which knows nothing of it.

The rule: in a frame that merges temporally and whose scene took a geometry edit since the previous frame, the temporal candidate of a
shaded pixel i whose slot j = motion[i] passes findTemporalNeighbor and holds W != 0 is examined (in records mode: unless retargeting has
just evaluated it again); its segment pos[i] -> pos[i] + wi[j] * dist[j] is walked when its bounding box overlaps one of the frame's
dirty boxes (or always: "everything"); a walked segment that the edited oracle scene's test_occlusion finds blocked makes the merge take
the candidate as W = 0.  Here that is a patch of the oracle's history slot -- W = 0, Li, wi and dist as they were -- after which the
unmodified oracle runs the frame (oracle_frame of tests/light_retarget.py).  Occlusion depends on the pixel's own position, so of two
pixels that read one slot (a moving camera) one may be patched and the other not: every other merging reader of a patched slot joins the
candidates with the slot's values as they were, and groups_of gives each reader of a slot a group of its own.

The oracle always runs tracked: with no emission edit its rescale is luminance(Le) / luminance(Li) = x / x = 1 and Li = Le, the same
bits, so the untracked library is held to it as well (light ids are compared only where the library tracks them).  The surface is the
library's (rs_debug_restir_surface / _wo), as in tests/light_retarget.py."""
import numpy as np

from tests import light_retarget as lr
from tests.emitter_edits import HipSide, OracleSide, scene_data
from tests.geometry_edits import root_box
from tests.light_retarget import Pair, groups_of, oracle_frame, reevaluate, surface_of, temporal_neighbours  # noqa: F401

F = np.float32
KEPT = 8                                                    # RS_DIRTY_BOXES_KEPT
TALL_BOX = np.arange(10, 22, dtype=np.int32)                # cornell's tall box (restir_amd.scenes.cornell_box; part 1 of tests/part_transforms.py)
LAMP = np.array([34, 35], np.int32)                         # ... and its lamp
# The move of the tall box that the tests make: towards the middle of the room, under the lamp.  Chosen so that on cornell at 64x48
# after ten warm frames at least 16 segments are free before it and blocked after it, and at least 16 segments with W != 0 miss its
# dirty box (tests/test_shadow_revalidate_host.py asserts both); the box stays inside the root box.
DISPLACEMENT = np.array([0.45, 0.0, 0.4], F)


def moved_box(sd, vertices, d=DISPLACEMENT, ids=TALL_BOX):
    """(ids, vertices) of the triangles `ids` translated by d from where `vertices` has them; nothing leaves the creation-time root box."""
    cur = np.asarray(vertices, F).reshape(-1, 3, 3)
    v = (cur[ids] + np.asarray(d, F)).astype(F)
    lo, hi = root_box(sd.vertices)
    assert (v >= lo).all() and (v <= hi).all(), "the move leaves the root box"
    return np.asarray(ids, np.int32), v


def dirty_box(old_vertices, ids, new_vertices):
    """np.min / np.max over the old corners of the named primitives and the new corners of each id's LAST record."""
    old = np.asarray(old_vertices, F).reshape(-1, 3, 3)
    new = np.asarray(new_vertices, F).reshape(-1, 3, 3)
    ids = np.asarray(ids).reshape(-1)
    last = {int(p): j for j, p in enumerate(ids)}
    pts = np.concatenate([old[sorted(last)].reshape(-1, 3), new[sorted(last.values())].reshape(-1, 3)])
    return pts.min(0), pts.max(0)


def segment_in_boxes(seg, boxes, everything=False):
    """The NumPy expression of the issue: on every axis min(a, b) <= hi and max(a, b) >= lo, for at least one box."""
    seg = np.asarray(seg, F).reshape(-1, 6)
    if everything:
        return np.ones(len(seg), bool)
    a, b = seg[:, :3], seg[:, 3:]
    out = np.zeros(len(seg), bool)
    with np.errstate(all="ignore"):
        for box in np.asarray(boxes, F).reshape(-1, 6):
            out |= ((np.minimum(a, b) <= box[3:]) & (np.maximum(a, b) >= box[:3])).all(1)
    return out


class DirtyRing:
    """rs_scene's ring of dirty boxes and the frame's choice, restated from the edits a test makes."""

    def __init__(self):
        self.edits = 0
        self.kept = []                                      # (edit number, box), oldest first

    def edit(self, old_vertices, ids, new_vertices):
        self.edits += 1
        lo, hi = dirty_box(old_vertices, ids, new_vertices)
        self.kept = (self.kept + [(self.edits, np.concatenate([lo, hi]).astype(F))])[-KEPT:]

    def choose(self, seen, same_scene=True):
        """(launch, everything, boxes) of a frame whose previous frame saw `seen` edits."""
        none = np.zeros((0, 6), F)
        if not same_scene:
            return True, True, none
        if self.edits == seen:
            return False, False, none
        boxes = [b for e, b in self.kept if seen < e <= self.edits]
        if len(boxes) != self.edits - seen:
            return True, True, none
        return True, False, np.stack(boxes)


def segments_of(pos, last, slots):
    """a = pos, b = pos + wi * dist in float32, one rounding per operation."""
    with np.errstate(all="ignore"):
        return np.concatenate([pos, pos + last["wi"][slots] * last["dist"][slots][:, None]], 1).astype(F)


def revalidate(scene, boxes, everything, slots, ok, shaded, pos, last, excluded=None):
    """The rule for every pixel.  Returns (examined, walked, occluded) masks."""
    examined = ok & shaded & (last["weight"][slots] != 0)
    if excluded is not None:
        examined &= ~excluded
    seg = segments_of(pos, last, slots)
    walked = examined & segment_in_boxes(seg, boxes, everything)
    occluded = np.zeros(len(slots), bool)
    if walked.any():
        occluded[walked] = scene.test_occlusion(seg[walked]) != 0
    return examined, walked, occluded


def patches(occluded, slots, ok, shaded, last, records=None):
    """oracle_frame's candidates: the occluded pixels with W = 0, and every other merging reader of their slots with the slot as it is."""
    shared = ok & shaded & np.isin(slots, slots[occluded]) & ~occluded
    px = np.nonzero(occluded | shared)[0]
    j = slots[px]
    W = np.where(occluded[px], F(0), last["weight"][j]).astype(F)
    pdf = np.zeros(len(px), F) if records is None else records["pdf"][j]
    return dict(pixel=px, slot=j, Li=last["Li"][j].copy(), wi=last["wi"][j].copy(), dist=last["dist"][j].copy(), W=W, pdf=pdf)


def join(a, b):
    return {k: np.concatenate([a[k], b[k]]) for k in a}


NONE = dict(pixel=np.zeros(0, np.int64), slot=np.zeros(0, np.int64), Li=np.zeros((0, 3), F), wi=np.zeros((0, 3), F), dist=np.zeros(0, F),
            W=np.zeros(0, F), pdf=np.zeros(0, F))


class RevalPair(Pair):
    """An oracle renderer and a library renderer with shadow revalidation on, frame by frame.  lights: 0 off, 1 ids (tracking),
    2 records (retargeting: the restatement of tests/light_retarget.py runs first, and its candidates are excluded here)."""

    def __init__(self, capi, name, W, H, lights=0, sobol=None, regroup=True, on=True):
        self.capi, self.sd, self.lights = capi, scene_data(name), lights
        self.o = OracleSide(capi, self.sd, W, H, sobol=sobol, track=True)
        self.h = HipSide(capi, self.sd, W, H, sobol=sobol)
        restir = self.h.r.restir
        if lights == 1:
            restir.set_light_tracking(True)
        if lights == 2:
            restir.set_light_retargeting(True)
        restir.set_shadow_regroup(regroup)
        restir.set_shadow_revalidation(on)
        self.moved = lr.MovedAt(self.o.r.scene)
        self.seen = 0
        self.ring, self.seen_edits, self.same_scene = DirtyRing(), 0, True
        self.groups = 1
        n = W * H
        self.rec_cur, self.rec_last, self.rec_temp = lr.no_records(n), lr.no_records(n), lr.no_records(n)
        self.occluded = np.zeros(n, bool)
        self.slots = np.zeros(n, np.int64)

    def edit(self, ids, v, n=None, how="set_geometry"):
        """how: set_geometry, set_triangles, or (part ids, matrices) for set_part_transforms, whose baked arrays are ids / v / n."""
        self.ring.edit(self.o.r.scene.vertices, ids, v)
        self.o.set_geometry(ids, v, n)
        if isinstance(how, tuple):
            self.h.r.scene.set_part_transforms(*how)
        else:
            getattr(self.h, how)(ids, v, n)
        self.moved.edit(ids)

    def frame(self, reuse):
        """Returns (library's state, oracle's state, library's counters, restated counters) of the frame."""
        o, h = self.o.r, self.h.r
        first = o.restir.first
        h.frame(reuse)
        pos_tag, normal, _ = h.restir.surface()
        shaded, pos, nrm, mats, wo = surface_of(pos_tag, normal, h.restir.surface_wo())
        o.gbuf.render(o.scene, o.cam)                       # (repeated inside oracle_frame, with the same result)
        slots, ok = temporal_neighbours(o.gbuf)
        scene = o.scene
        env_id = len(scene.light_prob) - 1 if scene.env_map_tex >= 0 else -1
        n = o.W * o.H
        merges = not first and bool(reuse & 1)
        last = o.restir.last.copy()
        ids_before = o.restir.ids_last.copy() if o.restir.track_scene == scene.uid else np.full(n, -1, np.int32)
        retargeted, taken, rt_counts = NONE, np.zeros(n, bool), (0, 0, 0)
        if self.lights == 2 and merges and self.moved.moves != self.seen:
            taken, retargeted, rt_counts = reevaluate(scene, lr.light_records(scene), self.moved.stamp, self.seen, env_id, slots, ok, shaded, pos, nrm, mats, wo,
                                              last, ids_before, self.rec_last)
        launch, everything, boxes = self.ring.choose(self.seen_edits, self.same_scene)
        cand, counts = NONE, (0, 0, 0)
        self.occluded = np.zeros(n, bool)
        if merges and launch:
            examined, walked, self.occluded = revalidate(scene, boxes, everything, slots, ok, shaded, pos, last, taken)
            cand = patches(self.occluded, slots, ok, shaded, last, self.rec_last)
            counts = (int(examined.sum()), int(walked.sum()), int(self.occluded.sum()))
        self.slots, self.last_before = slots, last
        has = ok & merges
        c_wi, c_dist, c_id, c_rec = last["wi"][slots].copy(), last["dist"][slots].copy(), ids_before[slots], self.rec_last[slots].copy()
        px = retargeted["pixel"]
        c_wi[px] = retargeted["wi"]; c_dist[px] = retargeted["dist"]; c_rec["pdf"][px] = retargeted["pdf"]
        self.groups = oracle_frame(o, reuse, join(retargeted, cand))
        o.rays += counts[1] + rt_counts[1]                  # every walked segment is one ray, retargeting's too
        self.seen, self.seen_edits, self.same_scene = self.moved.moves, self.ring.edits, True
        ref = dict(image=o.image.copy(), rays=o.rays, last=o.restir.last.copy(), temp=o.restir.temp.copy())
        got = dict(image=h.image.cpu().numpy(), rays=h.rays, last=h.restir.download(1), temp=h.restir.download(2))
        if self.lights == 2:
            lr.carry_records(self, scene, env_id, reuse, shaded, pos, has, c_wi, c_dist, c_id, c_rec)
            ref["ids"], got["ids"] = o.restir.light_ids(1), h.restir.download_light_samples(1)["light"].copy()
        elif self.lights == 1:
            ref["ids"], got["ids"] = o.restir.light_ids(1), h.restir.download_light_ids(1)
        return got, ref, h.restir.revalidate_stats(), counts
