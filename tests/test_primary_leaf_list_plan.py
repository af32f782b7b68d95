"""CPU: the leaf list of one 8x8 tile (restir_amd/csrc/rs_cuts.h cut_walk, the function the device builder runs), asked through the
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
from tests.cut_plan_cases import box, camera as _camera, directions as _directions, order_of as _order  # noqa: F401  (box: a fixture)


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
