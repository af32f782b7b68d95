"""Shadow revalidation (rs_restir_set_shadow_revalidation) on the GPU.  Against the CPU oracle composed with the NumPy restatement of
tests/shadow_revalidate.py, bit for bit: radiance, ray count, the reservoirs last written and published, the light ids or records where
they are tracked, and the kernel's three counters, after an occluder moved through each of the three edit calls.  GPU against GPU: the
identities of frames that launch nothing, frames in flight, row bands.  tests/test_shadow_revalidate_host.py shows without a GPU that
the move blocks segments that were free and that its dirty box filters."""
import numpy as np
import pytest

from oracle import binding as ob
from restir_amd import sobol
from tests import shadow_revalidate as sv
from tests.common import HipRenderer, bits_equal, hip_scene, oracle_scene
from tests.emitter_edits import edited_oracle_scene, scene_data
from tests.part_transforms import bake, identity, parts_of, translation
from tests.scene_edits import assert_same

pytestmark = pytest.mark.gpu

SIZES = {"grid": (64, 48), "off": (70, 45)}                  # on the 32x8 grid of the kernel's blocks, and off it
WARM = 6


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
        self.base = np.array([pair.o.r.cam.position[i] for i in range(3)], np.float32)

    def step(self):
        if self.on:
            t = np.float32(0.9 * self.frame)
            p = self.base + np.float32(0.15) * np.array([np.cos(t), 0.5 * np.sin(t), np.sin(t)], np.float32)
            self.pair.o.r.set_camera_position(p); self.pair.h.r.set_camera_position(p)
        self.frame += 1


def check_frame(pair, reuse, tag, launched, moved=False):
    got, ref, stats, counts = pair.frame(reuse)
    assert_same(ref, got, tag)
    assert stats == counts, (tag, stats, counts)
    assert pair.h.r.restir.revalidate_launched() == launched, (tag, "launched after a geometry edit and only then")
    if not launched:
        assert stats == (0, 0, 0), (tag, stats)
    if moved:                                                # on the library's own counters
        assert stats[1] >= 1 and stats[2] >= 1 and stats[0] > stats[1], (tag, stats)
    return stats


def box_edit(hip, pair, how, back):
    """The tall box by DISPLACEMENT (or back to its rest pose) through the edit call `how`."""
    sd, cur = pair.sd, pair.o.r.scene.vertices
    if how == "set_part_transforms":
        m = identity() if back else translation(sv.DISPLACEMENT)
        ids, v, n = bake(hip, "cornell", 1, m)
        pair.edit(ids, v, n, how=([1], [m]))
    else:
        ids, v = sv.moved_box(sd, cur, -sv.DISPLACEMENT if back else sv.DISPLACEMENT)
        pair.edit(ids, v, None, how=how)


# ---- (a) parity with the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how,lights,sampler,orbit,regroup,size", [
    ("set_triangles", 0, "engine", False, True, "grid"), ("set_geometry", 1, "engine", False, False, "off"),
    ("set_part_transforms", 2, "engine", False, True, "off"), ("set_triangles", 2, "sobol", True, False, "grid"),
    ("set_geometry", 0, "sobol", True, True, "off"), ("set_part_transforms", 1, "sobol", False, False, "grid"),
    ("set_geometry", 1, "engine", True, True, "grid"), ("set_part_transforms", 0, "engine", True, False, "off"),
    ("set_triangles", 1, "sobol", False, True, "off"), ("set_geometry", 2, "engine", True, True, "off")])
def test_parity_after_an_occluder_move(hip, how, lights, sampler, orbit, regroup, size):
    """lights 0 / 1 / 2: light tracking off, ids, records; regroup: the compaction by length bins, or the plain dense one."""
    W, H = SIZES[size]
    pair = sv.RevalPair(hip, "cornell", W, H, lights=lights, sobol=sobol.sobol_table() if sampler == "sobol" else None, regroup=regroup)
    if how == "set_part_transforms":
        pair.h.r.scene.define_parts(parts_of("cornell")[0])
    cam = Orbit(pair, orbit)
    tag = (how, lights, sampler, orbit, regroup, size)
    for f in range(WARM):
        cam.step()
        check_frame(pair, 3, tag + ("warm", f), False)
    groups = 1
    for back in (False, True):
        box_edit(hip, pair, how, back)
        cam.step()
        check_frame(pair, 3, tag + ("back" if back else "moved",), True, moved=True)
        groups = max(groups, pair.groups)
        cam.step()
        check_frame(pair, 3, tag + ("after",), False)
    assert groups <= sv.lr.MAX_GROUPS and (orbit or groups == 1)
    assert pair.h.r.scene.geometry_edits() == pair.ring.edits == 2


def test_parity_when_one_edit_moves_a_lamp_and_the_box(hip):
    """Records mode: one set_geometry names the box and one of the lamp's two triangles.  Retargeting evaluates that triangle's samples
    again and has walked them; revalidation examines the rest."""
    W, H = SIZES["off"]
    pair = sv.RevalPair(hip, "cornell", W, H, lights=2)
    for f in range(WARM):
        check_frame(pair, 3, ("warm", f), False)
    cur = pair.o.r.scene.vertices.reshape(-1, 3, 3)
    ids, v = sv.moved_box(pair.sd, cur)
    lamp = sv.LAMP[:1]
    pair.edit(np.concatenate([ids, lamp]), np.concatenate([v, cur[lamp] + np.array([0.2, -0.04, 0.15], np.float32)]).astype(np.float32))
    check_frame(pair, 3, "lamp and box", True, moved=True)
    assert pair.h.r.restir.retarget_launched() and pair.h.r.restir.retarget_stats()[0] > 0
    check_frame(pair, 3, "after", False)


# ---- (b) ring overflow and scene change: "everything" ----------------------------------------------------------------------------------
def test_nine_edits_in_one_gap_walk_everything(hip):
    W, H = SIZES["grid"]
    pair = sv.RevalPair(hip, "cornell", W, H)
    for f in range(WARM):
        check_frame(pair, 3, ("warm", f), False)
    for k in range(9):                                       # nine one-triangle edits: the first has left the ring
        cur = pair.o.r.scene.vertices
        pair.edit(*sv.moved_box(pair.sd, cur, ids=sv.TALL_BOX[k:k + 1]), how="set_triangles")
    boxes, everything = pair.h.r.scene.dirty_boxes(0)
    assert everything and len(boxes) == 0
    boxes, everything = pair.h.r.scene.dirty_boxes(1)
    assert not everything and np.array_equal(boxes, pair.ring.choose(1)[2])
    assert pair.ring.choose(0)[1]
    stats = check_frame(pair, 3, "nine edits", True, moved=False)
    assert stats[0] == stats[1] > 0 and stats[2] >= 1          # every examined candidate walked


def test_a_change_of_scene_walks_everything(hip):
    W, H = SIZES["off"]
    pair = sv.RevalPair(hip, "cornell", W, H)
    for f in range(WARM):
        check_frame(pair, 3, ("warm", f), False)
    # another scene object on both sides: cornell with the box where DISPLACEMENT puts it
    fresh = oracle_scene(pair.sd)
    ids, v = sv.moved_box(pair.sd, fresh.vertices)
    pair.o.r.scene = edited_oracle_scene(hip, fresh, ids, v)
    pair.h.r.scene = hip_scene(hip, pair.sd)
    pair.h.r.scene.set_geometry(ids, v)
    pair.ring = sv.DirtyRing()
    pair.ring.edits = 1                                      # (the new scene's own count; its ring is not asked)
    pair.same_scene = False
    stats = check_frame(pair, 3, "another scene", True)
    assert stats[0] == stats[1] > 0 and stats[2] >= 1
    check_frame(pair, 3, "after", False)


# ---- (c) identities, GPU against GPU ---------------------------------------------------------------------------------------------------
def state(r):
    return dict(image=r.image.cpu().numpy(), rays=r.rays, last=r.restir.download(1), temp=r.restir.download(2))


def test_frames_that_launch_nothing_equal_the_switch_off(hip):
    sd = scene_data("cornell")
    W, H = SIZES["off"]
    a, b = HipRenderer(hip, sd, W, H), HipRenderer(hip, sd, W, H)
    assert not b.restir.get_shadow_revalidation()            # off by default
    b.restir.set_shadow_revalidation(True)
    assert b.restir.get_shadow_revalidation() and not a.restir.get_shadow_revalidation()
    for f in range(12):
        a.frame(3); b.frame(3)
        assert_same(state(a), state(b), f)
        assert not b.restir.revalidate_launched() and b.restir.revalidate_stats() == (0, 0, 0)
    ids, v = sv.moved_box(sd, sd.vertices)
    b.scene.set_triangles(ids, v)
    b.frame(3)
    assert b.restir.revalidate_launched() and b.restir.revalidate_stats()[2] >= 1
    b.frame(3)
    assert not b.restir.revalidate_launched() and b.restir.revalidate_stats() == (0, 0, 0)


def edited_run(hip, frames, sync=True, bands=None):
    """`frames` frames with revalidation on and the box moved (there and back) before every frame from the third on."""
    import torch
    sd = scene_data("cornell")
    W, H = SIZES["off"]
    r = HipRenderer(hip, sd, W, H)
    r.restir.set_shadow_revalidation(True)
    v = sd.vertices.reshape(-1, 3, 3).copy()
    images, out = [torch.zeros((W * H, 3), dtype=torch.float32, device="cuda") for _ in range(0 if sync else frames)], []
    hip.set_sync(sync)
    for f in range(frames):
        if f >= 2:
            ids, ev = sv.moved_box(sd, v, sv.DISPLACEMENT if f % 2 == 0 else -sv.DISPLACEMENT)
            r.scene.set_geometry(ids, ev)
            v[ids] = ev
        if not sync:                                         # no wait between the frames: each image is copied in the library stream's order
            r.gbuf.render(r.scene, r.cam)
            r.restir.direct(r.scene, r.cam, r.gbuf, r.image.data_ptr(), 0, r.looper, 3)
            r.looper += 1
            r.gbuf.update(r.cam)
            hip.hip_memcpy_d2d_async(images[f].data_ptr(), r.image.data_ptr(), W * H * 12)
        elif bands is None:
            r.frame(3)
        else:
            r.gbuf.render(r.scene, r.cam)
            for y0, y1 in bands:
                r.restir.phase_a(r.scene, r.cam, r.gbuf, r.looper, 3, y0, y1)
            for y0, y1 in bands:
                r.restir.phase_b(r.scene, r.cam, r.gbuf, r.image.data_ptr(), 0, 3, y0, y1)
            r.restir.end_frame()
            r.rays = r.restir.ray_count()                    # (of the last phase-A call: not compared)
            r.looper += 1
            r.gbuf.update(r.cam)
        if sync:
            d = state(r)
            d.pop("rays")
            d["stats"] = np.array(r.restir.revalidate_stats())      # (of the whole frame: the bands' counters summed)
            out.append(d)
    if not sync:
        hip.synchronize()
        hip.set_sync(True)
        r.rays = r.restir.ray_count()
        return [i.cpu().numpy() for i in images], state(r)
    return out


def test_row_bands_equal_the_full_frame(hip):
    full = edited_run(hip, 6)
    banded = edited_run(hip, 6, bands=((0, 17), (17, SIZES["off"][1])))
    for f, (a, b) in enumerate(zip(full, banded)):
        assert_same(a, b, f)
    assert full[-1]["stats"][2] >= 1 and full[1]["stats"].sum() == 0


def test_frames_in_flight_equal_synchronous(hip):
    """rs_set_sync(0): twelve frames, a move in every gap, no wait in between; every image and the final state."""
    ref = edited_run(hip, 12)
    images, last = edited_run(hip, 12, sync=False)
    for f, (a, b) in enumerate(zip(ref, images)):
        assert bits_equal(a["image"], b), f
    last.pop("rays")
    ref[-1].pop("stats")
    assert_same(ref[-1], last, "final")


def test_two_objects_on_one_scene(hip):
    """Two rs_restir on one scene, the second run every second frame: each remembers for itself which edits it has seen (the second
    takes two boxes per frame), and each equals its own restatement."""
    W, H = SIZES["grid"]
    a, b = sv.RevalPair(hip, "cornell", W, H), sv.RevalPair(hip, "cornell", W, H)
    b.h.r.scene = a.h.r.scene
    b.ring = a.ring
    for f in range(WARM):
        check_frame(a, 3, ("a warm", f), False)
        if f % 2:
            check_frame(b, 3, ("b warm", f), False)
    for f in range(4):
        cur = a.o.r.scene.vertices
        ids, v = sv.moved_box(a.sd, cur, sv.DISPLACEMENT if f % 2 == 0 else -sv.DISPLACEMENT)
        a.edit(ids, v)
        b.o.set_geometry(ids, v); b.moved.edit(ids)          # (the library's scene and the ring are shared: edited once)
        check_frame(a, 3, ("a", f), True, moved=True)
        if f % 2:
            assert len(b.ring.choose(b.seen_edits)[2]) == 2
            check_frame(b, 3, ("b", f), True)


# ---- (d) switches ----------------------------------------------------------------------------------------------------------------------
def test_switches(hip):
    sd = scene_data("cornell")
    W, H = SIZES["grid"]
    r = HipRenderer(hip, sd, W, H, track=True)
    for _ in range(3):
        r.frame(3)
    v = sd.vertices.reshape(-1, 3, 3).copy()
    ids, ev = sv.moved_box(sd, v)
    r.scene.set_triangles(ids, ev)
    v[ids] = ev
    assert r.scene.geometry_edits() == 1
    r.restir.set_shadow_revalidation(True)                   # the edit made before the switch is taken as seen
    r.frame(3)
    assert not r.restir.revalidate_launched()
    ids, ev = sv.moved_box(sd, v, -sv.DISPLACEMENT)
    r.scene.set_triangles(ids, ev)
    v[ids] = ev
    r.restir.set_light_tracking(False)                       # leaves revalidation as it was
    assert r.restir.get_shadow_revalidation()
    r.frame(3)
    assert r.restir.revalidate_launched() and r.restir.revalidate_stats()[1] >= 1
    r.restir.set_shadow_revalidation(False)                  # off: nothing is launched from then on
    ids, ev = sv.moved_box(sd, v)
    r.scene.set_triangles(ids, ev)
    r.frame(3)
    assert not r.restir.revalidate_launched() and r.restir.revalidate_stats() == (0, 0, 0) and not r.restir.get_shadow_revalidation()
    lib = hip.lib()
    assert lib.rs_restir_set_shadow_revalidation(None, 1) == hip.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_restir_get_shadow_revalidation(r.restir.handle, None) == hip.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_debug_restir_revalidate(r.restir.handle, None) == hip.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_debug_restir_revalidate_launched(None, None) == hip.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_scene_geometry_edits(r.scene.handle, None) == hip.RS_ERR_INVALID_ARGUMENT


# ---- (e) what it buys ------------------------------------------------------------------------------------------------------------------
def test_an_occluded_candidate_is_not_reused(hip):
    """The frame after the move, at the pixels whose candidate the restatement found occluded.  Switch on: none of them publishes the
    marked sample (its reservoir's wi differs from the slot's).  Switch off: at least one keeps the stale sample, bit for bit."""
    W, H = SIZES["grid"]
    wi = {}
    for on in (True, False):
        pair = sv.RevalPair(hip, "cornell", W, H, on=on)
        for f in range(10):
            if on:
                check_frame(pair, 3, ("warm", f), False)
            else:
                pair.h.r.frame(3)
        if on:
            box_edit(hip, pair, "set_triangles", False)
            check_frame(pair, 3, "moved", True, moved=True)
            px, slot_wi = np.nonzero(pair.occluded)[0], pair.last_before["wi"][pair.slots[pair.occluded]]
        else:
            ids, v = sv.moved_box(pair.sd, pair.sd.vertices)
            pair.h.r.scene.set_triangles(ids, v)
            pair.h.r.frame(3)
        wi[on] = pair.h.r.restir.download(1)["wi"][px]
    assert len(px) >= 16
    stale_on = (wi[True].view(np.uint32) == slot_wi.view(np.uint32)).all(1)
    stale_off = (wi[False].view(np.uint32) == slot_wi.view(np.uint32)).all(1)
    print("occluded candidates: %d; published stale with the switch on: %d, off: %d" % (len(px), stale_on.sum(), stale_off.sum()))
    assert not stale_on.any()
    assert stale_off.any()
