"""Primary leaf lists (restir_amd/csrc/rs_cuts.h "Leaf lists", rs_walk.h packet_walk_leaves; rs_restir_set_primary_leaf_lists): a whole 8x8
tile of a still camera's primary-ray launch walks the flat list of the leaves its own pixels can pass instead of its block's cut.

Every comparison is bit for bit, after EVERY frame: the lists on against the CPU oracle, the lists off (cuts on) against the oracle --
image, both reservoir buffers, the published copy, the ray count -- and between the two library runs the surface planes the primary rays
write (rs_debug_restir_surface).  rs_debug_primary_leaf_list_info says which frame built, which frames walked lists and how many tiles
have one; rs_debug_primary_leaf_list_missing is the containment check, ray by ray.

Scenes, sizes and helpers are those of tests/primary_cuts.py, shared with tests/test_gpu_primary_cuts.py (the Cornell box and the Sponza-class scene scaled down so that the
packet walk takes its fast form, the only one that walks cuts or lists), plus the Bistro-class scene scaled the same way: half of its
leaf boxes are flat, as every one of the Cornell box's is, so accepted hits go up the ancestor chain there."""
import numpy as np
import pytest

from tests import extreme_cases as xc
from tests import geometric_cases as gc
from tests.common import EmissionEdits, get_scene
from tests.primary_cuts import (TURNED, Side, fast_form as _fast_form, frames_of, move_camera as _move_camera,
                                move_one_triangle as _move_one_triangle, refit as _refit, sides as _sides, small as _small, three_way,
                                turn_a_part as _turn_a_part, used_after_build as _lists_after_build, view as _view)

pytestmark = pytest.mark.gpu

DEFAULT_CAP = 192


def _three_way(hip, sd, size, rows=None, frames=4, **kw):
    return three_way(hip, sd, size, rows, frames, toggle="lists", **kw)


def _list_frames(h, o, n, tag):
    return frames_of(h, o, n, tag, lists=True)


@pytest.fixture(scope="module", autouse=True)
def _libm():
    with xc.correctly_rounded_libm():
        yield


def _bistro():
    """The Bistro-class scene, small and scaled until its triangles pass scene.hip far_skip_allowed."""
    sd = get_scene("bistro:0.01")
    v = sd.vertices.reshape(-1, 3, 3)
    worst = float((np.abs(v[:, 1] - v[:, 0]).max(1) * np.abs(v[:, 2] - v[:, 0]).max(1)).max())
    s = min(1.0, 0.95 / np.sqrt(worst))
    gc._affine(sd, scale=(s,) * 3)
    assert _fast_form(sd)
    sd.camera_args = dict(sd.camera_args, rotation=(-65.0, -12.0, 0.0), fov_y=14.0)
    return sd


def _tiles(size, rows=None):
    rows = rows or (0, size[1])
    return ((size[0] + 31) // 32) * 4 * ((rows[1] - rows[0] + 7) // 8)


# ---- sizes and cameras ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["sponza", "bistro"])
@pytest.mark.parametrize("size,rows", [((64, 16), None), ((70, 21), None), ((96, 54), (11, 54))], ids=["64x16", "70x21", "rows-from-11"])
def test_still_camera_equals_lists_off_and_oracle(hip, scene, size, rows):
    sd = _view("sponza:0.03", **TURNED) if scene == "sponza" else _bistro()
    on = _three_way(hip, sd, size, rows)
    _lists_after_build(on.lists, 4)
    last = on.lists[-1]
    print(scene, size, rows, last, on.info[-1])
    assert last["tiles"] == _tiles(size, rows)
    assert last["without_list"] < last["tiles"] and 0 < last["records"] <= DEFAULT_CAP * (last["tiles"] - last["without_list"])


def test_a_sign_change_inside_the_frame_leaves_tiles_without_a_list(hip):
    """A view down a diagonal of the y-z plane (tests/test_gpu_primary_cuts.py): d.x changes sign in one column of tiles and the traversal
    order changes across others -- those tiles keep the cut or the tree, the others take lists, in one launch."""
    on = _three_way(hip, _view("sponza:0.03", rotation=(-80.0, -42.0, 0.0), fov_y=10.0), (192, 48))
    last = on.lists[-1]
    print(last)
    assert last["used"] and 0 < last["without_list"] < last["tiles"] == _tiles((192, 48))


def test_a_row_of_special_case_rays_ignores_the_lists(hip):
    """View (0, 0, 1) exactly, 64 x 32 pixels (the view of tests/test_gpu_primary_cuts.py, two tile rows more): the image centre's row and
    column hold AABB::intersect's near-zero and axis-aligned directions.  The two tile rows and two tile columns that touch them (20 of
    32 tiles) are refused a list by cut_cell's keep-off from zero -- a wave with a special-case lane never has one to ignore, and checks
    for itself all the same; the twelve tiles away from the centre lines may take lists next to them in the same launch."""
    sd = _view("cornell", position=(0.0, 0.45, -0.4))
    on = _three_way(hip, sd, (64, 32), axes=((0.0, 0.0, 1.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0)))
    last = on.lists[-1]
    print(last)
    assert last["builds"] == 1 and last["tiles"] == 32
    assert last["without_list"] >= 20, last


# ---- temporal sequence ----------------------------------------------------------------------------------------------------------------
def test_eight_still_frames_a_move_and_still_again(hip):
    sd, h, o = _sides(hip)
    frames = lambda n, tag: _list_frames(h, o, n, tag)
    still = frames(8, "still")
    assert [i["used"] for i in still] == [False, False] + [True] * 6, still          # lists from the third frame on
    assert [i["builds"] for i in still] == [0] + [1] * 7
    assert still[-1]["records"] > 0
    _move_camera(hip, sd, h, o)
    moved = frames(1, "moved")
    assert not moved[0]["used"] and moved[0]["records"] == 0, moved                  # forgotten
    again = frames(2, "still again")
    assert [i["used"] for i in again] == [False, True] and [i["builds"] for i in again] == [2, 2], again
    assert again[-1]["records"] > 0


# ---- caps -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, 1, 4, None], ids=["cap0", "cap1", "cap4", "default"])
def test_caps_mix_tiles_with_and_without_lists(hip, cap):
    on = _three_way(hip, _view("sponza:0.03", **TURNED), (96, 54), frames=4, list_cap=cap)
    last = on.lists[-1]
    print(cap, last)
    if cap == 0:
        assert all(i["builds"] == 0 and not i["used"] for i in on.lists) and on.info[-1]["used"]       # the cuts alone
        return
    assert last["used"] and last["tiles"] == _tiles((96, 54))
    assert last["records"] <= (cap or DEFAULT_CAP) * (last["tiles"] - last["without_list"])
    if cap:
        assert 0 < last["without_list"], last         # some tile is past a cap of 1 or 4: its wave walks the node cut next to waves on lists
    assert last["without_list"] < last["tiles"] or cap == 1


# ---- flat boxes and grazing views -----------------------------------------------------------------------------------------------------
GRAZING = {
    "cornell_own_view": lambda: (_small("cornell"), (96, 54)),          # every leaf box is flat: every accepted hit goes up the chain
    "in_the_plane_of_a_wall": lambda: (_view("cornell", position=(-0.45, 0.45, 0.135), rotation=(-30.0, -14.0, 0.0), fov_y=14.0), (96, 54)),
    "inside_a_box": lambda: (_view("cornell", position=(0.135, 0.5, 0.18), rotation=(-62.0, -20.0, 0.0), fov_y=15.0), (96, 54)),
}


@pytest.mark.parametrize("name", list(GRAZING))
def test_flat_boxes_and_grazing_views(hip, name):
    sd, size = GRAZING[name]()
    on = _three_way(hip, sd, size)
    last = on.lists[-1]
    print(name, last)
    assert last["builds"] == 1 and last["used"] and last["records"] > 0


# ---- edits ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change", [_move_one_triangle, _refit, _turn_a_part], ids=["set_triangles", "set_geometry", "part_transform"])
def test_a_geometry_change_forgets_the_lists(hip, change):
    sd, h, o = _sides(hip)
    info = _list_frames(h, o, 3, "before")
    assert [i["used"] for i in info] == [False, False, True] and info[-1]["builds"] == 1 and info[-1]["records"] > 0
    change(hip, sd, h, o)
    info = _list_frames(h, o, 3, "after")
    assert [i["used"] for i in info] == [False, False, True], info
    assert [i["builds"] for i in info] == [1, 2, 2], info
    assert info[-1]["records"] > 0


def test_material_and_emission_edits_keep_the_lists(hip):
    sd, h, o = _sides(hip)
    _list_frames(h, o, 3, "before")
    ids, rad = EmissionEdits(sd, 11).next()
    for s in (h, o):
        s.set_emission(ids, rad)
    info = _list_frames(h, o, 2, "after the emission edit")
    assert all(i["used"] and i["builds"] == 1 and i["records"] > 0 for i in info), info
    rec = np.array(sd.materials[:1]).copy()
    rec["baseColor"][0] = rec["baseColor"][0] * np.float32(0.5)
    for s in (h, o):
        s.set_materials(np.array([0], np.int32), rec)
    info = _list_frames(h, o, 2, "after the material edit")
    assert all(i["used"] and i["builds"] == 1 and i["records"] > 0 for i in info), info


# ---- containment ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["sponza", "bistro", "cornell"])
def test_no_passed_leaf_is_absent_from_its_tile_s_list(hip, scene):
    """10^4 rays: every pixel corner of the frame's tiles with jitters of exactly 0 and 1, the rest random (pixel, jitter)."""
    sd = {"sponza": lambda: _view("sponza:0.03", **TURNED), "bistro": _bistro, "cornell": lambda: _small("cornell")}[scene]()
    size = (96, 54)
    side = Side(hip, sd, size, lists=True)
    for _ in range(3):
        side.frame()
    info = side.lists[-1]
    assert info["builds"] == 1 and info["used"], info
    rng = np.random.default_rng(7)
    corners = [(x, y, jx, jy) for ty in range(0, size[1], 8) for tx in range(0, size[0], 8)
               for x, jx in ((tx, 0.0), (min(tx + 7, size[0] - 1), 1.0)) for y, jy in ((ty, 0.0), (min(ty + 7, size[1] - 1), 1.0))]
    n = 10000 - len(corners)
    rays = np.array(corners + list(zip(rng.integers(0, size[0], n), rng.integers(0, size[1], n), rng.uniform(0, 1, n), rng.uniform(0, 1, n))), np.float32)
    assert len(rays) == 10000
    out = side.r.restir.primary_leaf_list_missing(side.r.scene, rays)
    print(scene, info, out)
    assert out["missing"] == 0, out
    assert out["passed"] > 0 and out["left_out"] < len(rays)
