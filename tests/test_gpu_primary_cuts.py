"""Primary cuts (restir_amd/csrc/rs_cuts.h; rs_restir_set_primary_cuts, include/restir_hip.h): the primary rays of a camera that stands
still walk a per-block cut of the BVH instead of the tree.

* equality: the frames of a still camera with the cuts on, with the cuts off and on the oracle, bit for bit after EVERY frame -- image,
  both reservoir buffers, the published copy and the ray count against the oracle; between the two library runs also the per-pixel
  state the primary rays leave (rs_debug_restir_surface).  rs_debug_primary_cut_info says which frame built and which frames walked cuts.
* containment: the conservative block test itself.  rs_debug_primary_cut_missing walks single rays of a block -- corner pixels with
  jitters of exactly 0 and 1, and random ones -- through the whole tree on the geometric part of the reference's box test and counts
  the nodes they pass that the block's cut lacks: none, in every scene and view.
* fallbacks: blocks without a cut (a view along +z exactly, a diagonal view with a sign change and an order change inside the frame, a cap of 8
  records) walk the tree; the frames equal the oracle's.
* invalidation: a camera move, rs_scene_set_triangles, a part transform and another size drop the cut -- the frame after equals the
  oracle without it, the next still frame builds again; an emission edit keeps it.
Small scenes and frames: the Cornell box (36 triangles) and the Sponza-class scene at 0.03 (7 864), both SCALED DOWN (by 0.45 and 0.25):
the packet walk takes its fast form -- the only one that walks cuts -- in scenes whose triangles pass scene.hip far_skip_allowed
(DevScene::axisCull: edge product at most 1), which the full-size benchmark scenes do and these two, as generated, do not.  The far,
huge, flat and sub-cell scenes of tests/geometric_cases.py are run as they are: where their triangles are too large no block takes a
cut, which is asserted, and "far", "squashed" and the sub-cell cluster are run a second time on the scaled box, where the blocks do
("huge" and "slab" are their scale: no scaled form of them has triangles small enough)."""
import types
import numpy as np
import pytest

from restir_amd import scenes
from restir_amd.ctypes_structs import LAMBERTIAN, LIGHT, make_materials
from tests import extreme_cases as xc
from tests import geometric_cases as gc
from tests.common import EmissionEdits, hip_scene, oracle_scene
from tests.primary_cuts import (TURNED, Side, fast_form as _fast_form, frames_of as _frames, move_camera as _move_camera,
                                move_one_triangle as _move_one_triangle, sides as _sides, small as _small, three_way as _three_way,
                                turn_a_part as _turn_a_part, used_after_build as _used_after_build, view as _view)
from tests.scene_edits import assert_same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _libm():
    with xc.correctly_rounded_libm():                # the oracle's cos / sin as the device evaluates them: every bit must agree
        yield


# ---- equality -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,rows,overlapped", [((96, 54), None, False), ((96, 54), None, True), ((70, 37), None, False), ((96, 54), (11, 54), False),
                                                  ((70, 37), (11, 30), True)],
                         ids=["96x54", "96x54-overlapped", "70x37", "strip-from-11", "70x37-strip-overlapped"])
def test_still_camera_equals_cuts_off_and_oracle(hip, size, rows, overlapped):
    frames = 8 if overlapped else 6                  # overlapped: three renders before the G-buffer answers from its planes, then the build
    on = _three_way(hip, _view("sponza:0.03", **TURNED), size, rows, frames, overlapped)
    _used_after_build(on.info, frames)
    last = on.info[-1]
    tiles_y = (on.rows[1] - on.rows[0] + 7) // 8
    assert last["cells"] == ((size[0] + 31) // 32) * tiles_y
    assert last["without_cut"] < last["cells"] and last["records"] > 0
    print(size, rows, "overlapped" if overlapped else "synchronous", last)


def test_cornell_equals_cuts_off_and_oracle(hip):
    """The reference's own view: along -z, so the middle column and row of blocks straddle a sign change and keep the tree."""
    on = _three_way(hip, _small("cornell"), (96, 54))
    _used_after_build(on.info, 6)
    assert 0 < on.info[-1]["without_cut"] < on.info[-1]["cells"]


# ---- containment ----------------------------------------------------------------------------------------------------------------------
def _flat_quad():
    """One axis-aligned quad (leaf boxes without thickness) under a small lamp."""
    mats = make_materials([dict(type=LAMBERTIAN, baseColor=(0.7, 0.7, 0.7)), dict(type=LIGHT, baseColor=(8.0, 8.0, 8.0))])
    s = scenes.TriangleSoup()
    s.add_quad((-0.45, 0, 0.45), (0.45, 0, 0.45), (0.45, 0, -0.45), (-0.45, 0, -0.45), 0)
    s.add_quad((-0.1, 0.7, -0.1), (0.1, 0.7, -0.1), (0.1, 0.7, 0.1), (-0.1, 0.7, 0.1), 1)
    return scenes.SceneData("flat_quad", s, mats, dict(position=(0.2, 0.5, 1.0), rotation=(-115.0, -30.0, 0.0), fov_y=12.0, focal_dist=1.0))


def _containment_views():
    v = {
        "inside_a_box": lambda: (_view("cornell", position=(0.135, 0.5, 0.18), rotation=(-62.0, -20.0, 0.0), fov_y=15.0), (96, 54)),
        "1e-3_from_a_wall": lambda: (_view("cornell", position=(-0.449, 0.45, 0.135), rotation=(-30.0, -14.0, 0.0), fov_y=14.0), (96, 54)),
        "flat_quad": lambda: (_flat_quad(), (96, 54)),
        "sponza": lambda: (_view("sponza:0.03", **TURNED), (70, 37)),
        "sponza_own_view": lambda: (_view("sponza:0.03"), (96, 54)),
    }
    for name in ("far", "huge", "slab", "squashed", "sub_cell"):
        v[name] = (lambda n: lambda: (gc.case(n, "cornell").after, gc.SIZE))(name)
    def cluster(c):
        """gc._sub_cell's cluster without its 2^16 scale: 64 triangles within a quarter of a grid step of one point of the scaled box."""
        lo, hi = gc.root_box64(c.sd)
        gc._append(c.sd, gc.cluster_vertices(np.random.default_rng(41), lo, hi, 64), int(np.nonzero(c.sd.materials["type"][c.sd.material_ids] != LIGHT)[0][0]))

    for name, edit in (("far_scaled", gc._far), ("squashed_scaled", gc._squashed), ("sub_cell_scaled", cluster)):
        def build(edit=edit):
            c = types.SimpleNamespace(sd=_small("cornell"))
            edit(c)
            if edit is gc._squashed:                 # the sheet seen from above (from its own height only the rows that straddle y = 0 see it)
                c.sd.camera_args = dict(c.sd.camera_args, position=(0.0, 0.5, 1.2), rotation=(-90.0, -25.0, 0.0))
            return c.sd, gc.SIZE
        v[name] = build
    return v


CONTAINMENT = _containment_views()


def _block_rays(rng, size, cell, cells_x, rows):
    """Rays of block `cell`: its corner pixels (those inside the frame) with jitters of exactly 0 and 1 in both coordinates, 96 random ones."""
    x0, y0 = (cell % cells_x) * 32, rows[0] + (cell // cells_x) * 8
    x1, y1 = min(x0 + 31, size[0] - 1), min(y0 + 7, rows[1] - 1)
    rays = [(x, y, jx, jy) for x in (x0, x1) for y in (y0, y1) for jx in (0.0, 1.0) for jy in (0.0, 1.0)]
    rays += [(x, y, jx, jy) for x in (x0, x1) for y in (y0, y1) for jx, jy in ((0.0, 0.5), (1.0, 0.25), (0.75, 0.0), (0.5, 1.0))]
    px, py = rng.integers(x0, x1 + 1, 96), rng.integers(y0, y1 + 1, 96)
    rays += list(zip(px, py, rng.uniform(0, 1, 96).astype(np.float32), rng.uniform(0, 1, 96).astype(np.float32)))
    return np.array(rays, np.float32)


@pytest.mark.parametrize("name", list(CONTAINMENT))
def test_no_passed_node_is_absent_from_its_block_s_cut(hip, name):
    sd, size = CONTAINMENT[name]()
    side = Side(hip, sd, size)
    for _ in range(3):
        side.frame()
    info = side.info[-1]
    assert info["builds"] == 1 and info["used"], info
    rng = np.random.default_rng(5)
    cells_x = (size[0] + 31) // 32
    with_cut = passed = 0
    for cell in range(info["cells"]):
        out = side.r.restir.primary_cut_missing(side.r.scene, cell, _block_rays(rng, size, cell, cells_x, side.rows))
        assert out["missing"] == 0, (name, cell, out)
        if out["records"]:
            with_cut += 1
            passed += out["passed"]
            assert out["left_out"] == 0, (name, cell, out)        # a block with a cut: one order, no special-case ray
    print(name, info, "blocks with a cut:", with_cut, "nodes passed:", passed)
    assert with_cut == info["cells"] - info["without_cut"]
    if _fast_form(sd):
        assert with_cut > 0 and passed > 0, (name, info)
    else:                                            # triangles too large for the fast form of the packet walk: nothing is cut, nothing to contain
        assert with_cut == 0, (name, info)


# ---- fallbacks ------------------------------------------------------------------------------------------------------------------------
def test_view_along_plus_z_has_no_cut(hip):
    """View (0, 0, 1) exactly, 64 x 16 pixels: the image centre is a corner of all four blocks, so every block's direction interval
    touches zero in x and y (and the centre rays are AABB::intersect's axis-aligned case): no block has a cut, every wave walks the tree."""
    sd = _view("cornell", position=(0.0, 0.45, -0.4))         # inside the room, its back to the back wall: the boxes and the side walls
    on = _three_way(hip, sd, (64, 16), axes=((0.0, 0.0, 1.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0)))
    info = on.info[-1]
    assert info["builds"] == 1 and info["used"]
    assert info["cells"] == 4 and info["without_cut"] == 4 and info["records"] == 0, info


def test_diagonal_view_has_both_kinds_of_block(hip):
    """A view down a diagonal of the y-z plane, 192 x 48 pixels: d.x changes sign in one column of blocks and the traversal order goes from
    z to y across two more (the block rule restated in NumPy gives 6 blocks with a sign change, 12 with two orders, 18 with a cut)."""
    sd = _view("sponza:0.03", rotation=(-80.0, -42.0, 0.0), fov_y=10.0)
    on = _three_way(hip, sd, (192, 48))
    info = on.info[-1]
    print(info)
    assert info["cells"] == 36 and 0 < info["without_cut"] < info["cells"] and info["records"] > 0, info


def test_cap_of_eight_records_overflows(hip):
    sd = _view("sponza:0.03", **TURNED)
    plain = _three_way(hip, sd, (96, 54), frames=3).info[-1]
    capped = _three_way(hip, sd, (96, 54), frames=4, cap=8).info[-1]
    print("default cap:", plain, "cap 8:", capped)
    assert capped["builds"] == 1 and capped["used"]
    assert capped["without_cut"] > plain["without_cut"]
    assert capped["records"] <= 8 * (capped["cells"] - capped["without_cut"])


# ---- invalidation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change", [_move_camera, _move_one_triangle, _turn_a_part], ids=["camera", "set_triangles", "part_transform"])
def test_a_change_drops_the_cut_and_the_next_still_frame_rebuilds(hip, change):
    sd, h, o = _sides(hip)
    info = _frames(h, o, 3, "before")
    assert [i["used"] for i in info] == [False, False, True] and info[-1]["builds"] == 1
    assert info[-1]["without_cut"] < info[-1]["cells"]
    change(hip, sd, h, o)
    info = _frames(h, o, 3, "after")
    assert [i["used"] for i in info] == [False, False, True], info       # the tree, the tree and the build, the new cut
    assert [i["builds"] for i in info] == [1, 2, 2], info
    assert info[-1]["records"] > 0


def test_another_size_builds_its_own_cut(hip):
    """A size is fixed per rs_restir (rs_restir_init), and check_frame_args holds the camera's resolution -- part of the key's camera bytes
    -- to it: one object never sees two sizes, so "a size change drops the cut" cannot happen to a cut and is not a case.  What a caller
    does instead is make an object of the other size: on the same scene it starts without a cut and builds its own on its second still
    frame, next to the first object's."""
    sd = _small("cornell")
    scene_h, scene_o = hip_scene(hip, sd), oracle_scene(sd)
    scene_h.set_sample_sequence(None); scene_o.set_sample_sequence(None)
    for size in ((96, 54), (70, 37)):
        h, o = Side(hip, sd, size, scene=scene_h), Side(None, sd, size, scene=scene_o)
        for f in range(3):
            assert_same(o.frame(), h.frame(), "%dx%d, frame %d" % (size + (f,)))
        assert [i["used"] for i in h.info] == [False, False, True] and h.info[-1]["builds"] == 1
        assert h.info[-1]["cells"] == ((size[0] + 31) // 32) * ((size[1] + 7) // 8)
        assert h.info[-1]["records"] > 0


def test_an_emission_edit_keeps_the_cut(hip):
    sd, h, o = _sides(hip)
    _frames(h, o, 3, "before")
    ids, rad = EmissionEdits(sd, 11).next()
    for s in (h, o):
        s.set_emission(ids, rad)
    info = _frames(h, o, 2, "after the emission edit")
    assert all(i["used"] and i["builds"] == 1 and i["records"] > 0 for i in info), info
