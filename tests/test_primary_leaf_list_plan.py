"""CPU: the leaf list of one 8x8 tile (restir_amd/csrc/rs_cuts.h leaf_list_walk, the function the device builder runs), asked through the
host hook rs_debug_plan_primary_leaf_list over rs_build_bvh's tables of a tiny scene -- the Cornell box scaled as the GPU tests scale it.

* completeness and order: rays of the tile -- every pixel at jitters 0, 1 and in between, in double precision -- walk the WHOLE threaded
  tree of the tile's order on the geometric slab test (tMax >= max(tMin, 0), no distance cull).  Every leaf such a ray passes is in the
  list, the list's positions rise strictly (the threaded order), every entry is a leaf, and the list is not simply every leaf.
* the cap: one leaf fewer than the list has -> count says cap + 1 and only cap positions are written; exactly the length -> the same list.
* the empty list: a tile that looks past the scene has an order and no leaf.
* no order: a tile that holds a sign change of a direction component takes no list."""
import numpy as np
import pytest

from restir_amd import capi
from tests import geometric_cases as gc
from tests.common import get_scene

SIZE = (96, 54)


@pytest.fixture(scope="module")
def box():
    sd = get_scene("cornell")
    gc._affine(sd, scale=(0.45,) * 3)
    boxes, nodes = capi.build_bvh(sd.vertices)
    return sd, boxes, nodes


def _camera(sd, **args):
    from restir_amd.ctypes_structs import make_camera
    return capi.camera_update(make_camera(SIZE[0], SIZE[1], **dict(sd.camera_args, **args)))


def _directions(cam, x0, y0):
    """Camera::sample's unnormalised directions (rs_cuts.h cut_corner_dir) for every pixel of the tile at jitters 0, 0.5, 1 and a few odd ones."""
    W, H = SIZE
    right, up, view = (np.array([getattr(cam, n)[i] for i in range(3)], np.float64) for n in ("right", "up", "view"))
    tan_y = float(np.tan(np.float32(np.radians(cam.fov[1])))); aspect = float(np.float32(W) / np.float32(H)); focal = float(cam.focalDist)
    out = []
    for y in range(y0, y0 + 8):
        for x in range(x0, x0 + 8):
            for jx, jy in ((0, 0), (1, 1), (0, 1), (1, 0), (0.5, 0.5), (0.25, 0.875), (0.9375, 0.125)):
                X = (1.0 - (x + jx) / W * 2.0) * aspect * tan_y * focal
                Y = (1.0 - (y + jy) / H * 2.0) * tan_y * focal
                out.append(right * X + up * Y + view * focal)
    return np.array(out)


def _order(d):
    """DevScene::getMTBVHId of -d."""
    v = -d
    a = np.abs(v)
    if a[0] > a[1]:
        if a[0] > a[2]:
            return 0 if v[0] > 0 else 1
        return 4 if v[2] > 0 else 5
    if a[1] > a[2]:
        return 2 if v[1] > 0 else 3
    return 4 if v[2] > 0 else 5


def _passed_leaves(o, d, boxes, table):
    """Positions of the leaves a ray passes on the geometric slab test alone, walking the whole threaded table { prim, box, miss link }."""
    out, cur, end = [], 0, len(table)
    with np.errstate(divide="ignore"):
        inv = 1.0 / d
    while cur != end:
        prim, box, nxt = (int(t) for t in table[cur])
        t1, t2 = (boxes[box, :3].astype(np.float64) - o) * inv, (boxes[box, 3:].astype(np.float64) - o) * inv
        t_min, t_max = np.minimum(t1, t2).max(), np.maximum(t1, t2).min()
        if t_max >= max(t_min, 0.0):
            if prim >= 0:
                out.append(cur)
            cur += 1
        else:
            cur = nxt
    return out


TILES = [(40, 24), (80, 40), (40, 40)]


@pytest.mark.parametrize("tile", TILES, ids=["%d_%d" % t for t in TILES])
def test_the_list_is_complete_and_in_threaded_order(box, tile):
    sd, boxes, nodes = box
    cam = _camera(sd, rotation=(-80.0, -5.0, 0.0), fov_y=12.0)
    order, count, pos = capi.plan_primary_leaf_list(cam, tile[0], tile[1], boxes, nodes, 1 << 20)
    assert order >= 0 and count == len(pos) > 0
    table = nodes[order]
    assert np.all(np.diff(pos) > 0)                              # the threaded order, no leaf twice
    assert np.all(table[pos, 0] >= 0)                            # leaves only
    assert count < (table[:, 0] >= 0).sum()                      # a selection, not the tree
    o = np.array([cam.position[i] for i in range(3)], np.float64)
    listed, seen = set(int(p) for p in pos), set()
    for d in _directions(cam, *tile):
        assert _order(d) == order
        passed = _passed_leaves(o, d, boxes, table)
        assert set(passed) <= listed, (tile, sorted(set(passed) - listed))
        seen |= set(passed)
    assert seen                                                   # the rays do pass leaves: the inclusion above says something


def test_the_cap(box):
    sd, boxes, nodes = box
    cam = _camera(sd, rotation=(-80.0, -5.0, 0.0), fov_y=12.0)
    order, count, pos = capi.plan_primary_leaf_list(cam, 40, 24, boxes, nodes, 1 << 20)
    assert count >= 2
    o2, c2, p2 = capi.plan_primary_leaf_list(cam, 40, 24, boxes, nodes, count)
    assert (o2, c2) == (order, count) and np.array_equal(p2, pos)
    o3, c3, p3 = capi.plan_primary_leaf_list(cam, 40, 24, boxes, nodes, count - 1)
    assert o3 == order and c3 == count and len(p3) == count - 1 and np.array_equal(p3, pos[:count - 1])     # cap + 1: past the cap, no list
    o4, c4, p4 = capi.plan_primary_leaf_list(cam, 40, 24, boxes, nodes, 0)
    assert o4 == order and c4 == 1 and len(p4) == 0


def test_a_tile_that_looks_past_the_scene_has_an_empty_list(box):
    sd, boxes, nodes = box
    cam = _camera(sd, position=(0.0, 3.0, 1.5), rotation=(-65.0, 40.0, 0.0), fov_y=5.0)        # above the room, looking up and aside
    order, count, pos = capi.plan_primary_leaf_list(cam, 40, 24, boxes, nodes, 64)
    assert order >= 0 and count == 0 and len(pos) == 0


def test_a_sign_change_inside_the_tile_gives_no_order(box):
    sd, boxes, nodes = box
    cam = _camera(sd)                                             # the box's own view, along -z: d.x changes sign in the middle column
    order, count, pos = capi.plan_primary_leaf_list(cam, 44, 8, boxes, nodes, 64)
    assert order == -1 and count == 0
    order, count, pos = capi.plan_primary_leaf_list(cam, 24, 8, boxes, nodes, 1 << 20)         # a tile to the side and above the centre has one
    assert order >= 0
