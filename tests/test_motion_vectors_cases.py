"""tests/motion_vectors.py pinned on the CPU: the helper that states the motion plane of a scene that tracks motion, and the inputs of
tests/test_gpu_motion_vectors.py.

  1. With the previous pose equal to the current one the helper's plane equals orc_gbuffer_render's, bit for bit, on both scenes, at the
     scene's camera and after the camera moved between frames.
  2. The helper's expression on the CURRENT vertices equals Scene.intersect's position bit for bit: the ray, the barycentrics and the
     operation order are the oracle's.
  3. The inputs matter: in the frame of the edit every case's plane differs from the camera-only plane in at least 50 of the 2 867
     pixels, and the ReSTIR-DI image of that frame (the second of the run, reuse 3) differs between the oracle fed the helper's plane
     and the oracle fed the camera-only plane.
     The kinds of tests/geometry_edits.py and tests/emitter_edits.py ALONE do not reach that: they move one triangle, or one lamp, of a
     61 x 47 view.  Pixels of the plane that differ in the frame of the edit, the kind's own edit alone, cornell / sponza:
       triangles: carry 210 / 0, carry_back 0 / 0, one 5 / 0, all 975 / 1900, repeated 44 / 0
       emitters:  one 20 / 0, all 8 / 1, mixed 31 / 2, repeated 7 / 0, carry_min 2 / 0, carry_max 31 / 0, carry_back 29 / 0,
                  scale_up 349 / 0, scale_down 0 / 0, flip 0 / 0, collapse 0 / 0, restore 9 / 0
     and only `all` (both scenes), `repeated` and `mixed` (cornell) change a pixel of the image.  So every case's gap holds two edits, the
     slide of the triangles nearest the image centre by a tenth of the scene's extent and then the kind's own edit
     (motion_vectors.case_edits): every kind is still applied, through its own call, and every case would fail without the feature.
     test_kinds_alone_fall_short keeps that statement honest.
  4. A triangle whose previous pose lies behind the last camera, and one whose previous pose is exactly the last camera's position: the
     helper runs, and what orc_camera_raster_coord yields is the expectation."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding as ob
from tests import motion_vectors as mv
from tests.common import bits_equal, oracle_scene
from tests.scene_edits import differing

W, H = mv.W, mv.H


@pytest.fixture(autouse=True)
def exact_libm():
    ob.set_libm_mode(1)
    yield
    ob.set_libm_mode(0)


@pytest.mark.parametrize("name", list(mv.SCENES) + [mv.TEXTURED])
def test_plane_of_a_scene_at_rest_is_the_oracles(name):
    """1 and 2."""
    sd = mv.scene_data(name)
    scene = oracle_scene(sd)
    cam = ob.camera_update(sd.camera(W, H))
    g = ob.GBuffer(W, H)
    base = np.array(list(cam.position), np.float32)
    hits = 0
    for frame, offset in enumerate([(0, 0, 0), (0, 0, 0), (0.3, -0.1, 0.2), (0.3, -0.1, 0.2), (-0.2, 0.15, -0.4)]):
        for i in range(3):
            cam.position[i] = float(base[i] + np.float32(offset[i]))
        ob.camera_update(cam)
        g.render(scene, cam)
        plane, prim, pos, cur = mv.object_motion_plane(scene, scene.vertices, cam, g.c.lastCamera, W, H, details=True)
        assert np.array_equal(plane, g.motion), (frame, int((plane != g.motion).sum()))
        assert np.array_equal(prim >= 0, g.prim_id[g.frame_idx] != -1)
        assert bits_equal(cur[prim >= 0], pos[prim >= 0]), frame
        hits += int((prim >= 0).sum())
        if frame in (2, 4):
            assert (plane != np.arange(W * H)).any()            # the camera moved since the last frame: the plane is not the identity
        g.update(cam)
    assert hits > W * H


CASES = [(name, kind) for name in mv.SCENES for kind in mv.kinds_for(name)] + [(mv.TEXTURED, kind) for kind in mv.TEXTURED_KINDS]


@pytest.mark.parametrize("name,kind", CASES)
def test_inputs_matter(name, kind):
    """3, for every case the GPU tests run."""
    tracked, camera_only = mv.oracle_case(name, kind, "direct_svgf")
    untracked, _ = mv.oracle_case(name, kind, "direct_svgf", tracked=False)
    moved = int((tracked[1]["motion"] != camera_only[1]).sum())
    print(name, kind, "pixels of the motion plane that differ from the camera-only plane:", moved)
    assert moved >= 50, moved
    assert differing(tracked[1]["image"], untracked[1]["image"]) >= 1
    for f in (0, 2, 3):                                      # at rest before the edit and after the advance: the camera-only plane
        assert np.array_equal(tracked[f]["motion"], camera_only[f]), f
    for f in range(4):                                       # the feature touches the motion plane alone
        for k in ("prim_id", "albedo", "normal", "depth"):
            assert bits_equal(tracked[f][k], untracked[f][k]), (f, k)
        assert np.array_equal(untracked[f]["motion"], camera_only[f])


def test_kinds_alone_fall_short():
    """Why every gap carries the slide: but for `all`, no kind of the two edit helpers moves 50 pixels of the plane on both scenes."""
    for kind in mv.kinds_for("cornell"):
        if ":" not in kind or kind == "triangles:all":
            continue
        moved = []
        for name in mv.SCENES:
            tracked, camera_only = mv.oracle_case(name, kind, "direct_svgf", with_slide=False)
            moved.append(int((tracked[1]["motion"] != camera_only[1]).sum()))
        assert min(moved) < 50, (kind, moved)


@pytest.mark.parametrize("kind", mv.CAMERA_KINDS)
@pytest.mark.parametrize("name", list(mv.SCENES))
def test_previous_pose_behind_and_at_the_last_camera(name, kind):
    """4: the case is what its name says -- in the frame of the edit the camera sees the triangle, and the previous pose of every such hit
    lies behind the last camera (negative along its view direction), or is its position exactly."""
    from restir_amd import capi
    sd = mv.scene_data(name)
    o = mv.OracleMotion(capi, sd)
    position, setup, edit = mv.camera_case(sd, kind)
    o.set_camera_position(position)
    mv.apply(o, setup)
    o.advance()
    o.frame()
    for e in mv.case_edits(name, kind)[1]:
        mv.apply(o, e)
    o.render()
    rays = mv.center_rays(o.cam, W, H)
    prim = o.scene.intersect(rays)[0]
    seen = prim == int(edit[1][0])
    assert seen.sum() >= 20, int(seen.sum())
    prev = mv.hit_points(o.scene, o.scene.vertices, rays, prim, o.prev)[seen]
    last = o.gbuf.c.lastCamera
    eye, view = np.array(list(last.position), np.float32), np.array(list(last.view), np.float32)
    assert bits_equal(eye, position)
    if kind == "at_last_camera":
        assert bits_equal(prev, np.broadcast_to(eye, prev.shape))
    else:
        assert ((prev - eye) @ view < 0).all()
    xy = np.zeros(2 * len(prev), np.int32)
    ob.lib().orc_camera_raster_coord(C.byref(last), len(prev), np.ascontiguousarray(prev).reshape(-1), xy)
    lx, ly = xy[0::2], xy[1::2]
    want = np.where((lx >= 0) & (lx < W) & (ly >= 0) & (ly < H), ly * W + lx, -1)
    assert np.array_equal(o.gbuf.motion[seen], want)
    print(name, kind, "pixels:", int(seen.sum()), "values of the plane there:", np.unique(want)[:8])
