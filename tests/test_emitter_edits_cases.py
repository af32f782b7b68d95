"""No GPU: the inputs of tests/test_gpu_emitter_edits.py mean something.  Every kind of edit changes the oracle's frame, the kinds that
change an area change the light powers, the helper's light tables are those the oracle builds by itself, the carried lamp really leaves
the old emissive root box, and the multi-bounce frames really hold last-bounce rays that end on the moved lamp."""
import numpy as np
import pytest

from oracle import binding as ob
from restir_amd import capi
from tests.common import OracleRenderer, bits_equal, oracle_scene
from tests.emitter_edits import (CHANGES_AREA, EDIT_KINDS, NEEDS_ENV, OracleSide, edited_oracle_scene, edits_up_to, emissive_root_box, emitters,
                                 kinds_for, light_tables, scene_data)
from tests.scene_edits import differing

W, H = 61, 47
SMALL = ("cornell", "single", "env")


def frame(sd, scene):
    r = OracleRenderer(sd, W, H, scene=scene)
    r.frame(3)
    return r.image.copy()


def test_kinds_and_scenes():
    assert kinds_for("cornell") == [k for k in EDIT_KINDS if k not in NEEDS_ENV] and kinds_for("env") == list(EDIT_KINDS)
    assert len(emitters(scene_data("cornell"))) == 2 and len(emitters(scene_data("single"))) == 1
    assert len(emitters(scene_data("bistro"))) == 1228 > 1024 and len(emitters(scene_data("many"))) > 2
    assert scene_data("env").env_map_tex >= 0
    for name in ("cornell", "single", "many", "bistro"):
        assert scene_data(name).env_map_tex < 0


@pytest.mark.parametrize("name", SMALL)
def test_every_kind_changes_the_frame_and_the_tables(name):
    """Kind by kind on the oracle: the frame after the edit differs from the frame before it, the light powers change where the edit
    changes an area, and every vertex stays inside the box the scene was created with."""
    sd = scene_data(name)
    scene = oracle_scene(sd)
    lo, hi = sd.vertices.reshape(-1, 3).min(0), sd.vertices.reshape(-1, 3).max(0)
    before = frame(sd, scene)
    for kind, (ids, v, n) in zip(kinds_for(name), edits_up_to(name, kinds_for(name)[-1])[0]):
        assert (np.asarray(v).reshape(-1, 3) >= lo).all() and (np.asarray(v).reshape(-1, 3) <= hi).all(), kind
        new = edited_oracle_scene(capi, scene, ids, v, n)
        after = frame(sd, new)
        assert differing(before, after) > 0, kind
        changed = not bits_equal(new.light_power, scene.light_power)
        if kind in CHANGES_AREA:
            assert changed and (not bits_equal(new.light_prob, scene.light_prob) or new.sum_power != scene.sum_power), kind
        if kind == "collapse":
            assert (new.light_power == 0).any()
        if kind == "collapse_all":
            assert (new.light_power[:-1] == 0).all() and new.light_power[-1] == scene.light_power[-1] > 0
        scene, before = new, after
    if sd.env_map_tex >= 0:                              # the last kind restores every lamp
        assert bits_equal(scene.vertices[emitters(sd)], sd.vertices.reshape(-1, 3, 3)[emitters(sd)])


@pytest.mark.parametrize("name", ["cornell", "env", "many"])
def test_helper_tables_are_the_oracles_own(name):
    """light_tables (new powers, the old environment entry, alias_build) equals what ob.Scene builds by itself, without `prebuilt`, from
    the same arrays."""
    sd = scene_data(name)
    old = oracle_scene(sd)
    v = edits_up_to(name, "scale_up")[2]
    power, prob, fail, total = light_tables(old, v)
    own = ob.Scene(v, old.normals, sd.texcoords, sd.material_ids, sd.materials, textures=sd.textures, env_map_tex=sd.env_map_tex)
    assert bits_equal(power, own.light_power) and bits_equal(prob, own.light_prob) and np.array_equal(fail, own.light_fail)
    assert np.float32(total) == np.float32(own.sum_power)
    assert np.array_equal(own.light_prim_ids, old.light_prim_ids)
    assert not bits_equal(power, old.light_power)


@pytest.mark.parametrize("name", ["cornell", "many", "bistro"])
def test_carry_leaves_the_old_emissive_root_box(name):
    sd = scene_data(name)
    lo0, hi0 = emissive_root_box(sd, edits_up_to(name, "repeated")[2])
    for kind in ("carry_min", "carry_max"):
        ids, v, _ = edits_up_to(name, kind)[0][-1]
        p = np.asarray(v).reshape(-1, 3)
        assert ((p < lo0) | (p > hi0)).any(), kind
        lo1, hi1 = emissive_root_box(sd, edits_up_to(name, kind)[2])
        assert not (np.array_equal(lo0, lo1) and np.array_equal(hi0, hi1)), kind


@pytest.mark.parametrize("name", ["cornell", "single"])
def test_last_bounce_rays_end_on_the_moved_lamp(name):
    """The scene's only lamp is the moved one.  pathTraceIndirect with max depth 1: a path's only bounce is its last, next-event estimation
    at depth 1 goes to the direct plane, so a pixel of the indirect plane is non-zero exactly where the last-bounce ray's closest hit is
    the lamp -- the question the emissive tree answers.  There are such pixels, and they are not the pixels of the lamp's old place.  At
    depth 4 the frame of the moved lamp differs from the frame at depth 3 (paths that reach their fourth bounce exist)."""
    sd = scene_data(name)
    assert len(np.unique(sd.material_ids[emitters(sd)])) == 1
    old = oracle_scene(sd)
    ids, v, n = edits_up_to(name, "one")[0][-1]
    new = edited_oracle_scene(capi, old, ids, v, n)
    cam = ob.camera_update(sd.camera(W, H))

    def last_hits(scene, depth):
        i = np.zeros((W * H, 3), np.float32)
        ob.pt_indirect(scene, cam, i, 0, 0, depth)
        return i
    a, b = last_hits(old, 1), last_hits(new, 1)
    assert np.count_nonzero(b.any(1)) > 0
    assert differing(a, b) > 0
    assert differing(last_hits(new, 3), last_hits(new, 4)) > 0


def test_oracle_side_keeps_the_scene_identity():
    sd = scene_data("env")
    o = OracleSide(capi, sd, W, H)
    uid, env = o.r.scene.uid, o.r.scene.env_prob.copy()
    o.set_geometry(*edits_up_to("env", "one")[0][-1])
    assert o.r.scene.uid == uid and bits_equal(o.r.scene.env_prob, env) and o.r.scene.c.envMapSamplerLength == len(env)
