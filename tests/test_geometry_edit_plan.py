"""CPU: what a geometry edit decides on the host before it touches the device (restir_amd/csrc/rs_geometry_plan.h), asked through
rs_debug_plan_geometry_edit of a view of the Cornell box: its 36 triangles, its lamp (the last two), the root box of rs_build_bvh as the
box the grid lies over.  The refusals carry the code and the text the three entry points report; no call here needs a device."""
import functools

import numpy as np
import pytest

from restir_amd import capi, scenes
from restir_amd.ctypes_structs import LIGHT
from tests import emitter_tables

SET_TRIANGLES, SET_GEOMETRY = "rs_scene_set_triangles", "rs_scene_set_geometry"
PART_REC_BYTES = 112
OUT_OF_RANGE = "a primitive id out of range"
NOT_FINITE = "a vertex or normal that is not finite"
OUTSIDE = ("a vertex outside the root box the scene was created with (the grid of its shadow-ray tree lies over that box); "
           "build a new scene")
A_LIGHT = ("a triangle whose material is a Light (the light table, the sampler's powers and the emissive tree are built over the "
           "emitters' geometry; rs_scene_set_geometry moves emitters)")
NO_POWER = "the edit leaves the light sampler without a finite, positive total power"


@functools.lru_cache(maxsize=None)
def cornell():
    sd = scenes.cornell_box()
    v = sd.vertices.reshape(-1, 3, 3)
    boxes, nodes = capi.build_bvh(v)
    root = boxes[nodes[0][0][1]]
    lamp = np.flatnonzero(sd.materials["type"][sd.material_ids] == LIGHT)
    assert list(lamp) == [34, 35]
    radiance = sd.materials["baseColor"][sd.material_ids[lamp]]
    return sd, v, (root[:3].copy(), root[3:].copy()), lamp, radiance


def view(bounded=True, env_power=None, tree=True, radiance=None):
    sd, v, grid, lamp, rad = cornell()
    return capi.geometry_edit_view(sd.material_ids, sd.materials, v, grid if bounded else None, lamp, rad if radiance is None else radiance,
                                   emitter_tables.triangle_area(v[lamp]), env_power, lamp[::-1] if tree else None)


def up16(b):
    return (b + 15) & ~15


def refusal(text, name=SET_GEOMETRY):
    return f"librestir_hip error {capi.RS_ERR_INVALID_ARGUMENT}: {name}: {text}"


def refused(text, name, emitters, ids, v, n=None, **kw):
    with pytest.raises(capi.RestirHipError) as e:
        capi.plan_geometry_edit(kw.pop("view", None) or view(), name, emitters, ids, v, n, **kw)
    assert str(e.value) == refusal(text, name)


def test_a_repeated_id_keeps_its_last_record_and_its_first_place():
    _, v, _, _, _ = cornell()
    ids = [7, 3, 7, 9, 3]
    plan, slots, lights = capi.plan_geometry_edit(view(), SET_TRIANGLES, 0, ids, v[ids], v[ids])
    assert (plan.m, plan.lamps, lights) == (3, 0, None)
    assert list(slots) == [0, 1, 0, 2, 1]              # 7 first, then 3, then 9: later records of an id go to its slot, the last one stays
    assert (plan.offV, plan.offN, plan.bytes) == (16, 16 + up16(3 * 36), 16 + 2 * up16(3 * 36))
    assert (plan.staged, plan.onDevice) == (plan.bytes, plan.bytes)


def test_ids_out_of_order_and_a_single_record():
    _, v, _, _, _ = cornell()
    plan, slots, _ = capi.plan_geometry_edit(view(), SET_TRIANGLES, 0, [30, 2, 17, 0], v[[30, 2, 17, 0]])
    assert plan.m == 4 and list(slots) == [0, 1, 2, 3]
    plan, slots, _ = capi.plan_geometry_edit(view(), SET_TRIANGLES, 0, [5], v[[5]], v[[5]])
    assert plan.m == 1 and list(slots) == [0]
    assert (plan.offV, plan.offN, plan.bytes) == (16, 16 + 48, 16 + 96)


def test_an_empty_edit():
    plan, slots, lights = capi.plan_geometry_edit(view(), SET_GEOMETRY, 1, [], np.zeros((0, 3, 3), np.float32))
    assert (plan.m, plan.lamps, plan.offV, plan.offN, plan.bytes, plan.staged, plan.onDevice) == (0, 0, 0, 0, 0, 0, 0)
    assert len(slots) == 0 and lights is None
    refused("count < 0 or null arrays", SET_GEOMETRY, 1, [], np.zeros((0, 3, 3), np.float32), count=-1)


def test_without_normals_the_layout_has_no_normals_part():
    _, v, _, _, _ = cornell()
    plan, _, _ = capi.plan_geometry_edit(view(), SET_TRIANGLES, 0, [1, 2, 3, 4, 5], v[1:6])
    assert plan.offN == 32 + up16(5 * 36) and plan.bytes == plan.offN


def test_the_part_record_source():
    _, v, _, _, _ = cornell()
    plan, _, _ = capi.plan_geometry_edit(view(), "rs_scene_set_part_transforms", 1, [1, 2, 3], v[1:4], v[1:4], num_part_recs=2)
    assert plan.partStaged == 2 * PART_REC_BYTES and plan.partOnDevice == plan.bytes + plan.partStaged
    assert (plan.staged, plan.onDevice) == (plan.bytes, plan.bytes)


@pytest.mark.parametrize("name,emitters", [(SET_TRIANGLES, 0), (SET_GEOMETRY, 1), ("rs_scene_set_part_transforms", 1)])
def test_ids_out_of_range(name, emitters):
    _, v, _, _, _ = cornell()
    refused(OUT_OF_RANGE, name, emitters, [0, -1], v[:2])
    refused(OUT_OF_RANGE, name, emitters, [0, 36], v[:2])
    capi.plan_geometry_edit(view(), name, emitters, [0, 33], v[:2])


def test_values_that_are_not_finite_or_outside_the_grid():
    _, v, (lo, hi), _, _ = cornell()
    bad = v[:2].copy(); bad[1, 2, 0] = np.nan
    refused(NOT_FINITE, SET_TRIANGLES, 0, [0, 1], bad)
    bad = v[:2].copy(); bad[1, 0, 1] = np.inf
    refused(NOT_FINITE, SET_TRIANGLES, 0, [0, 1], v[:2], bad)
    outside = v[:2].copy(); outside[0, 1, 2] = np.nextafter(hi[2], np.float32(np.inf))
    refused(OUTSIDE, SET_TRIANGLES, 0, [0, 1], outside)
    # the first offending record names the refusal: an id out of range in record 0 comes before the NaN of record 1
    refused(OUT_OF_RANGE, SET_TRIANGLES, 0, [40, 1], bad)
    on = v[:2].copy(); on[0, 0], on[1, 2] = lo, hi                  # exactly on the box: inside
    plan, _, _ = capi.plan_geometry_edit(view(), SET_TRIANGLES, 0, [0, 1], on)
    assert plan.m == 2
    # a scene without grid-box trees has no box to stay in
    plan, _, _ = capi.plan_geometry_edit(view(bounded=False), SET_TRIANGLES, 0, [0, 1], outside)
    assert plan.m == 2
    refused(NOT_FINITE, SET_TRIANGLES, 0, [0, 1], v[:2], bad, view=view(bounded=False))


def test_a_light_triangle_needs_the_entry_point_that_takes_emitters():
    _, v, _, lamp, _ = cornell()
    refused(A_LIGHT, SET_TRIANGLES, 0, [3, lamp[0]], v[[3, lamp[0]]])
    plan, _, lights = capi.plan_geometry_edit(view(), SET_GEOMETRY, 1, [3, lamp[0]], v[[3, lamp[0]]])
    assert plan.lamps == 1 and lights is not None
    plan, _, lights = capi.plan_geometry_edit(view(), SET_GEOMETRY, 1, [3], v[[3]])
    assert plan.lamps == 0 and lights is None


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("env_power", [None, 3.25])
def test_a_moved_emitter(env_power):
    """One lamp triangle moved and stretched, named twice (the last record counts) among other triangles: the sampler is the one of a
    scene built afresh from the edited vertices, the emissive root box numpy's, the grid emitter_tables.grid_over_box's."""
    _, v, _, lamp, rad = cornell()
    moved = v[lamp[0]] * np.float32([1.5, 1.0, 1.25]) + np.float32([0.1, -0.5, 0.05])
    ids = [lamp[0], 4, lamp[0]]
    ev = np.stack([v[lamp[0]] * np.float32(0.5), v[4], moved])
    plan, slots, lights = capi.plan_geometry_edit(view(env_power=env_power), SET_GEOMETRY, 1, ids, ev)
    assert (plan.m, plan.lamps, list(slots)) == (2, 1, [0, 1, 0])
    after = v.copy(); after[lamp[0]] = moved
    area, prob, fail, total = emitter_tables.light_sampler_tables(capi, after, lamp, rad, env_power)
    assert same_bits(lights["area"], area) and same_bits(lights["prob"], prob) and same_bits(lights["fail"], fail)
    assert same_bits(lights["sumAll"], total)
    e = after[lamp].reshape(-1, 3)
    assert same_bits(lights["emiLo"], e.min(0)) and same_bits(lights["emiHi"], e.max(0))
    grid = emitter_tables.grid_over_box(e.min(0), e.max(0))
    assert lights["emiGrid"] == 1 and same_bits(lights["emiBase"], grid["base"]) and same_bits(lights["emiScale"], grid["scale"])
    assert lights["emiMargin"] == grid["margin"]
    # a scene without the emissive tree lays no grid
    _, _, lights = capi.plan_geometry_edit(view(env_power=env_power, tree=False), SET_GEOMETRY, 1, ids, ev)
    assert lights["emiGrid"] == 0 and same_bits(lights["area"], area)


def test_emitters_collapsed_to_one_point_leave_no_grid():
    """... and no power of their own: with an environment map the edit is accepted, without one it is refused."""
    _, v, _, lamp, _ = cornell()
    point = np.broadcast_to(np.float32([0.0, 1.5, 0.0]), (2, 3, 3)).copy()
    _, _, lights = capi.plan_geometry_edit(view(env_power=2.0), SET_GEOMETRY, 1, lamp, point)
    assert lights["emiGrid"] == 0 and same_bits(lights["area"], np.zeros(2, np.float32)) and lights["sumAll"] == np.float32(2.0)
    assert same_bits(lights["emiLo"], point[0, 0]) and same_bits(lights["emiHi"], point[0, 0])
    refused(NO_POWER, SET_GEOMETRY, 1, lamp, point)
    refused(NO_POWER, "rs_scene_set_part_transforms", 1, lamp, point)


def test_the_only_emitter_given_zero_area():
    """The scene's power lies in one lamp triangle (the other's radiance is zero): that triangle collapsed, without an environment map."""
    _, v, _, lamp, rad = cornell()
    one = rad.copy(); one[1] = 0
    flat = v[lamp[:1]].copy(); flat[0, 2] = flat[0, 1]
    refused(NO_POWER, SET_GEOMETRY, 1, lamp[:1], flat, view=view(radiance=one))
    plan, _, lights = capi.plan_geometry_edit(view(radiance=one), SET_GEOMETRY, 1, lamp[1:], v[lamp[1:]] * np.float32(0.5))
    assert plan.lamps == 1 and lights["sumAll"] > 0
