"""ReSTIR-GI's revalidation (rs_restir_set_indirect_revalidation) on the GPU.  Against the CPU oracle composed with the NumPy restatement of
tests/indirect_revalidate.py, bit for bit after every frame: the image, the ray count, the reservoirs the call wrote, the history it merged
from (where the pass writes) and the kernel's four counters -- after an occluder moved through each of the three edit calls.  GPU against
GPU: frames that launch nothing, frames in flight.  tests/test_indirect_revalidate_host.py shows without a GPU that the move leaves slots
of every class and that dropping them changes the next frame.  cornell at 64x48 (3 072 slots: twelve full blocks) and 40x24 (960: the
last block partial)."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding as ob
from restir_amd import sobol
from tests import indirect_revalidate as iv
from tests import shadow_revalidate as sv
from tests.common import hip_scene, oracle_scene
from tests.emitter_edits import edited_oracle_scene, scene_data
from tests.part_transforms import bake, identity, parts_of, translation
from tests.scene_edits import assert_same

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def exact_libm(hip):
    ob.set_libm_mode(1)              # cos / sin correctly rounded on both sides: every bit must agree
    hip.set_sync(True)
    yield
    ob.set_libm_mode(0)
    hip.set_sync(True)


class Orbit:
    """A camera that moves a little every frame, along the view too, so that pixels share history slots."""

    def __init__(self, pair, on):
        self.pair, self.on, self.frame = pair, on, 0
        self.base = np.array([pair.o.cam.position[i] for i in range(3)], np.float32)

    def step(self):
        if self.on:
            t = np.float32(0.9 * self.frame)
            self.pair.set_camera_position(self.base + np.float32(0.15) * np.array([np.cos(t), 0.5 * np.sin(t), np.sin(t)], np.float32))
        self.frame += 1


def check_frame(pair, tag, launched, moved=False, reuse=1):
    got, ref, lib, restated = pair.frame(reuse)
    print(tag, "library", lib, "restated", restated)
    assert_same(ref, got, tag)
    assert lib == restated, (tag, lib, restated)
    assert lib[0] == launched, (tag, "launched after a geometry edit and only then")
    examined, stale, walked, occluded = lib[1]
    if not launched:
        assert lib[1] == (0, 0, 0, 0), (tag, lib)
    if moved:                                                # on the library's own counters: every class occurs
        assert stale >= 1 and occluded >= 1 and walked > occluded and examined > stale + walked, (tag, lib)
    return lib[1]


def box_edit(hip, pair, how, back, **kw):
    """The tall box by DISPLACEMENT (or back to its rest pose) through the edit call `how`."""
    if how == "set_part_transforms":
        m = identity() if back else translation(sv.DISPLACEMENT)
        ids, v, n = bake(hip, "cornell", 1, m)
        pair.edit(ids, v, n, how=([1], [m]), **kw)
    else:
        ids, v = sv.moved_box(pair.sd, pair.o.scene.vertices, -sv.DISPLACEMENT if back else sv.DISPLACEMENT)
        pair.edit(ids, v, None, how=how, **kw)


def warm(pair, size, cam=None):
    for f in range(iv.WARM[size]):
        if cam:
            cam.step()
        check_frame(pair, ("warm", f), False)


# ---- (a) parity with the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how,sampler,orbit,size", [
    ("set_geometry", "engine", False, "full"), ("set_triangles", "sobol", False, "partial"), ("set_part_transforms", "engine", True, "partial"),
    ("set_geometry", "sobol", True, "full"), ("set_triangles", "engine", True, "full"), ("set_part_transforms", "sobol", False, "full"),
    ("set_geometry", "engine", True, "partial"), ("set_triangles", "engine", False, "partial")])
def test_parity_after_the_move(hip, how, sampler, orbit, size):
    pair = iv.Pair(hip, "cornell", size, sobol=sobol.sobol_table() if sampler == "sobol" else None)
    if how == "set_part_transforms":
        pair.h.scene.define_parts(parts_of("cornell")[0])
    cam = Orbit(pair, orbit)
    tag = (how, sampler, orbit, size)
    warm(pair, size, cam)
    for back in (False, True):
        box_edit(hip, pair, how, back)
        cam.step()
        check_frame(pair, tag + ("back" if back else "moved",), True, moved=True)
        cam.step()
        check_frame(pair, tag + ("after",), False)
    assert pair.h.scene.geometry_edits() == pair.ring.edits == 2


def test_parity_with_motion_tracking(hip):
    """The G-buffer's motion plane follows the moved box to where it was, so other pixels read the dropped slots."""
    pair = iv.Pair(hip, "cornell", "full", tracked=True)
    warm(pair, "full")
    for back in (False, True):
        box_edit(hip, pair, "set_geometry", back)
        check_frame(pair, ("tracked", back), True, moved=True)
        check_frame(pair, ("tracked", back, "after"), False)


# ---- (b) ring overflow and scene change: "everything" ----------------------------------------------------------------------------------
def test_nine_edits_in_one_gap_drop_everything(hip):
    pair = iv.Pair(hip, "cornell", "full")
    warm(pair, "full")
    for k in range(9):                                       # nine one-triangle edits: the first has left the ring
        pair.edit(*sv.moved_box(pair.sd, pair.o.scene.vertices, ids=sv.TALL_BOX[k:k + 1]), how="set_triangles")
    assert pair.ring.choose(pair.seen_edits)[1]
    examined, stale, walked, occluded = check_frame(pair, "nine edits", True)
    assert stale == examined > 0 and walked == 0 and occluded == 0
    check_frame(pair, "after", False)


def test_a_change_of_scene_drops_everything(hip):
    pair = iv.Pair(hip, "cornell", "partial")
    warm(pair, "partial")
    # another scene object on both sides: cornell with the box where DISPLACEMENT puts it
    fresh = oracle_scene(pair.sd)
    fresh.set_sample_sequence(None)
    ids, v = sv.moved_box(pair.sd, fresh.vertices)
    pair.o.scene = edited_oracle_scene(hip, fresh, ids, v)
    pair.h.scene = hip_scene(hip, pair.sd)
    pair.h.scene.set_sample_sequence(None)
    pair.h.scene.set_geometry(ids, v)
    pair.ring = sv.DirtyRing()
    pair.ring.edits = 1                                      # (the new scene's own count; its ring is not asked)
    pair.same_scene = False
    examined, stale, walked, occluded = check_frame(pair, "another scene", True)
    assert stale == examined > 0 and walked == 0 and occluded == 0
    check_frame(pair, "after", False)


# ---- (c) an edit elsewhere ---------------------------------------------------------------------------------------------------------------
def test_an_edit_in_a_far_corner_leaves_most_slots(hip):
    """One triangle of the tall box becomes a small triangle across the room's minimum corner (parity, as above); the next gap moves it
    within the corner: the pass launches with a box of a fifth of the room's extent, drops what the rule says, and keeps nearly
    everything.  The oracle's figures: 2 305 examined, 3 stale, 37 walked, 2 of them occluded."""
    pair = iv.Pair(hip, "cornell", "full")
    warm(pair, "full")
    lo, hi = sv.root_box(pair.sd.vertices)
    ext = (hi - lo).astype(np.float32)
    small = (lo + np.float32(0.15) * ext * np.eye(3, dtype=np.float32)).astype(np.float32)[None]
    pair.edit(sv.TALL_BOX[:1], small)
    check_frame(pair, "to the corner", True)
    pair.edit(sv.TALL_BOX[:1], (small + np.float32(0.05) * ext).astype(np.float32))
    examined, stale, walked, occluded = check_frame(pair, "within the corner", True)
    assert examined >= 1024 and stale >= 1 and walked > occluded >= 1
    assert (pair.cls == iv.KEPT).sum() >= 0.9 * examined      # most are out of the box's reach and not even walked
    check_frame(pair, "after", False)


# ---- (d) identities, GPU against GPU ---------------------------------------------------------------------------------------------------
def test_frames_that_launch_nothing_equal_the_switch_off(hip):
    sd = scene_data("cornell")
    W, H = iv.SIZES["partial"]
    a, b = iv.HipGI(hip, sd, W, H), iv.HipGI(hip, sd, W, H)
    assert not b.restir.get_indirect_revalidation()          # off by default
    b.restir.set_indirect_revalidation(True)
    assert b.restir.get_indirect_revalidation() and not a.restir.get_indirect_revalidation()
    for f in range(8):
        a.frame(1); b.frame(1)
        assert_same(a.state(), b.state(), f)
        assert not b.restir.indirect_revalidate_launched() and b.restir.indirect_revalidate_stats() == (0, 0, 0, 0)
    ids, v = sv.moved_box(sd, sd.vertices)
    for r in (a, b):
        r.scene.set_triangles(ids, v)
        r.frame(1)
    assert b.restir.indirect_revalidate_launched() and not a.restir.indirect_revalidate_launched()
    sa, sb = a.state(), b.state()
    assert (sa["image"].view(np.uint32) != sb["image"].view(np.uint32)).any(1).sum() >= 16     # (what it buys: the host test's 115 pixels)
    for r in (a, b):
        r.frame(1)
    assert not b.restir.indirect_revalidate_launched() and b.restir.indirect_revalidate_stats() == (0, 0, 0, 0)


def edited_run(hip, frames, in_flight=0):
    """`frames` frames at 40x24 with the switch on and the box moved (there and back) before every frame from the fourth on.  in_flight:
    that many frames are enqueued without a wait (rs_set_sync(0), no ray count asked), each image copied in the library stream's order."""
    import torch
    sd = scene_data("cornell")
    W, H = iv.SIZES["partial"]
    r = iv.HipGI(hip, sd, W, H)
    r.restir.set_indirect_revalidation(True)
    v = sd.vertices.reshape(-1, 3, 3).copy()
    images = [torch.zeros((W * H, 3), dtype=torch.float32, device="cuda") for _ in range(frames)]
    launched = []
    hip.set_sync(not in_flight)
    for f in range(frames):
        if f >= 3:
            ids, ev = sv.moved_box(sd, v, sv.DISPLACEMENT if f % 2 else -sv.DISPLACEMENT)
            r.scene.set_geometry(ids, ev)
            v[ids] = ev
        r.gbuf.render(r.scene, r.cam)
        r.image.zero_()
        if in_flight:
            hip.check(hip.lib().rs_restir_indirect(r.restir.handle, r.scene.handle, C.byref(r.cam), r.gbuf.handle, r.image.data_ptr(), 0, r.looper, 1,
                                                   iv.DEPTH, None))
        else:
            r.restir.indirect(r.scene, r.cam, r.gbuf, r.image.data_ptr(), 0, r.looper, 1, iv.DEPTH)
        r.looper += 1
        r.gbuf.update(r.cam)
        launched.append(r.restir.indirect_revalidate_launched())        # (host only: no wait)
        hip.hip_memcpy_d2d_async(images[f].data_ptr(), r.image.data_ptr(), W * H * 12)
        if in_flight and (f + 1) % in_flight == 0:
            hip.synchronize()
    hip.synchronize()
    hip.set_sync(True)
    return [i.cpu().numpy() for i in images], launched, dict(written=r.restir.download_indirect(1), history=r.restir.download_indirect(0),
                                                              stats=np.array(r.restir.indirect_revalidate_stats()))


def test_three_frames_in_flight_equal_synchronous(hip):
    ref, launched, last = edited_run(hip, 9)
    images, launched3, last3 = edited_run(hip, 9, in_flight=3)
    assert launched == launched3 == [False] * 3 + [True] * 6
    for f, (a, b) in enumerate(zip(ref, images)):
        assert_same(dict(image=a), dict(image=b), f)
    assert_same(last, last3, "final")
    assert last["stats"][1] >= 1 and last["stats"][3] >= 1


# ---- (e) beside shadow revalidation, and two objects on one scene ------------------------------------------------------------------------
def test_beside_shadow_revalidation(hip):
    """One rs_restir, one scene: every frame is rs_restir_direct (reuse 3) with shadow revalidation on, then rs_restir_indirect with
    indirect revalidation on, each from a G-buffer of its own.  Each feature equals its own restatement -- the two note their previous
    scene and edit count apart."""
    size = "full"
    W, H = iv.SIZES[size]
    dp = sv.RevalPair(hip, "cornell", W, H)
    gp = iv.Pair(hip, "cornell", size, scene=dp.h.r.scene, on=False)
    gp.h.restir, gp.o.restir, gp.on = dp.h.r.restir, dp.o.r.restir, True
    gp.h.restir.set_indirect_revalidation(True)
    assert gp.h.restir.get_shadow_revalidation() and gp.h.restir.get_indirect_revalidation()

    def frame(tag, launched):
        got, ref, stats, counts = dp.frame(3)
        assert_same(ref, got, ("direct",) + tag)
        assert stats == counts and dp.h.r.restir.revalidate_launched() == launched, (tag, stats, counts)
        return stats, check_frame(gp, ("indirect",) + tag, launched and tag[0] != "warm")
    for f in range(6):
        frame(("warm", f), False)
    for back in (False, True):
        ids, v = sv.moved_box(dp.sd, dp.o.r.scene.vertices, -sv.DISPLACEMENT if back else sv.DISPLACEMENT)
        gp.ring.edit(dp.o.r.scene.vertices, ids, v)
        dp.edit(ids, v)
        gp.o.scene = dp.o.r.scene
        di, gi = frame(("moved", back), True)
        assert di[1] >= 1 and gi[1] >= 1 and gi[2] >= 1
        frame(("after", back), False)


def test_two_objects_on_one_scene(hip):
    """Two rs_restir on one scene, the second run every second frame: each remembers for itself which edits it has seen (the second
    takes two boxes per frame), and each equals its own restatement."""
    a = iv.Pair(hip, "cornell", "partial")
    b = iv.Pair(hip, "cornell", "partial", scene=a.h.scene)
    b.ring = a.ring
    for f in range(iv.WARM["partial"]):
        check_frame(a, ("a warm", f), False)
        if f % 2:
            check_frame(b, ("b warm", f), False)
    for f in range(4):
        ids, v = sv.moved_box(a.sd, a.o.scene.vertices, sv.DISPLACEMENT if f % 2 == 0 else -sv.DISPLACEMENT)
        a.edit(ids, v)
        b.o.set_geometry(ids, v)                             # (the library's scene and the ring are shared: edited once)
        check_frame(a, ("a", f), True, moved=True)
        if f % 2:
            assert len(b.ring.choose(b.seen_edits)[2]) == 2
            check_frame(b, ("b", f), True)


# ---- (f) switches ----------------------------------------------------------------------------------------------------------------------
def test_switches(hip):
    sd = scene_data("cornell")
    W, H = iv.SIZES["partial"]
    r = iv.HipGI(hip, sd, W, H)
    v = sd.vertices.reshape(-1, 3, 3).copy()

    def move():
        ids, ev = sv.moved_box(sd, v, sv.DISPLACEMENT if move.n % 2 == 0 else -sv.DISPLACEMENT)
        r.scene.set_triangles(ids, ev)
        v[ids] = ev
        move.n += 1
    move.n = 0

    def frame(launched):
        r.frame(1)
        assert r.restir.indirect_revalidate_launched() == launched
        stats = r.restir.indirect_revalidate_stats()
        assert (stats[0] > 0) == launched and (launched or stats == (0, 0, 0, 0))
    assert not r.restir.get_indirect_revalidation()
    for _ in range(4):
        frame(False)
    move()
    frame(False)                                             # off: the edit is seen, nothing is launched
    r.restir.set_indirect_revalidation(True)
    assert r.restir.get_indirect_revalidation()
    frame(False)                                             # the edit made while off and before the previous frame is not revalidated later
    move()
    frame(True)
    r.restir.set_indirect_revalidation(False)
    assert not r.restir.get_indirect_revalidation()
    move()
    frame(False)
    move()                                                   # made while off, but after the previous frame: the next frame sees it, on or off
    r.restir.set_indirect_revalidation(True)
    frame(True)
    move()
    r.restir.set_indirect_revalidation(False); r.restir.set_indirect_revalidation(True)      # on / off / on between edits forgets nothing
    frame(True)
    move()
    r.restir.reset()                                         # the first frame merges nothing: nothing to revalidate, and the edit is seen
    frame(False)
    frame(False)
    move()
    r.restir.set_shadow_revalidation(True)                   # independent of the DI switch
    assert r.restir.get_indirect_revalidation()
    frame(True)
    lib = hip.lib()
    out = (C.c_ulonglong * 4)()
    on = C.c_int(0)
    assert lib.rs_restir_set_indirect_revalidation(None, 1) == hip.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_restir_get_indirect_revalidation(None, C.byref(on)) == hip.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_restir_get_indirect_revalidation(r.restir.handle, None) == hip.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_debug_restir_indirect_revalidate(None, C.byref(out)) == hip.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_debug_restir_indirect_revalidate(r.restir.handle, None) == hip.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_debug_restir_indirect_revalidate_launched(None, C.byref(on)) == hip.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_debug_restir_indirect_revalidate_launched(r.restir.handle, None) == hip.RS_ERR_INVALID_ARGUMENT
