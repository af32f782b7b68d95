"""CPU: the node cut of one block (restir_amd/csrc/rs_cuts.h cut_walk and cut_relink, the functions the device builder runs), asked through
the host hook rs_debug_plan_primary_cut over rs_build_bvh's tables of the scaled Cornell box of tests/test_primary_leaf_list_plan.py
(36 triangles, 71 records, 96 x 54 pixels, blocks of 32 x 8).

* which records: positions rise strictly, and the kept set is closed under ancestors.
* the links: links[i] is the first j > i with positions[j] >= the original miss link of record i, else the count; links are nested.
* the walk: rays of the block -- every pixel at jitters 0, 1 and in between, in double precision -- walk the whole tree and the cut on the
  geometric slab test and visit the same kept records in the same order.
* the leaf records of an 8 x 8 block's node cut are exactly rs_debug_plan_primary_leaf_list's positions.
* the cap: count - 1 -> cap + 1 and cap positions, no links; count and count + 1 -> the same cut.
* no order: a block that holds a sign change of a direction component takes no cut."""
import numpy as np
import pytest

from restir_amd import capi
from tests.cut_plan_cases import box, camera as _camera, directions as _directions, order_of as _order  # noqa: F401  (box: a fixture)

BLOCKS = [(32, 24), (32, 40), (0, 40)]             # three of the blocks that take a cut in this view
VIEW = dict(rotation=(-80.0, -5.0, 0.0), fov_y=12.0)


def _slabs(o, d, boxes, table):
    """Per record of a threaded table: does the ray pass the geometric slab test (tMax >= max(tMin, 0)) on its box?"""
    with np.errstate(divide="ignore"):
        inv = 1.0 / d
    b = boxes[table[:, 1]].astype(np.float64)
    t1, t2 = (b[:, :3] - o) * inv, (b[:, 3:] - o) * inv
    t_min, t_max = np.minimum(t1, t2).max(1), np.maximum(t1, t2).min(1)
    return t_max >= np.maximum(t_min, 0.0)


def _walk(passes, links, end):
    """The records a ray visits: the next record after one it passes, the miss link after one it does not."""
    out, cur = [], 0
    while cur != end:
        out.append(cur)
        cur = cur + 1 if passes[cur] else int(links[cur])
    return out


def _plan(box, block, cap=1 << 20, size=(32, 8)):
    sd, boxes, nodes = box
    cam = _camera(sd, **VIEW)
    return cam, capi.plan_primary_cut(cam, block[0], block[1], size[0], size[1], boxes, nodes, cap)


@pytest.mark.parametrize("block", BLOCKS, ids=["%d_%d" % b for b in BLOCKS])
def test_records_and_links(box, block):
    sd, boxes, nodes = box
    cam, (order, count, pos, links) = _plan(box, block)
    assert order >= 0 and 0 < count == len(pos) == len(links) < nodes.shape[1]        # a selection, not the tree
    table = nodes[order]
    assert np.all(np.diff(pos) > 0)
    # closed under ancestors: in a threaded pre-order the ancestors of record p are the records a < p whose miss link lies beyond p
    kept = set(int(p) for p in pos)
    for p in pos:
        assert all(a in kept for a in range(p) if table[a, 2] > p), p
    for i in range(count):
        orig_link = table[pos[i], 2]
        later = [j for j in range(i + 1, count) if pos[j] >= orig_link]
        assert links[i] == (later[0] if later else count), i
        assert i < links[i] <= count
    for i in range(count):                           # nested: a record inside (i, links[i]) links no further than links[i]
        assert all(links[j] <= links[i] for j in range(i + 1, links[i]))


@pytest.mark.parametrize("block", BLOCKS, ids=["%d_%d" % b for b in BLOCKS])
def test_the_cut_walk_visits_what_the_tree_walk_visits(box, block):
    sd, boxes, nodes = box
    cam, (order, count, pos, links) = _plan(box, block)
    table = nodes[order]
    o = np.array([cam.position[i] for i in range(3)], np.float64)
    kept = set(int(p) for p in pos)
    entered = 0
    for d in _directions(cam, block[0], block[1], 32, 8):
        assert _order(d) == order
        passes = _slabs(o, d, boxes, table)
        whole = _walk(passes, table[:, 2], len(table))
        assert all(p in kept for p in np.array(whole)[passes[whole]])              # containment: every record the ray passes is kept
        through_cut = [int(pos[i]) for i in _walk(passes[pos], links, count)]
        assert through_cut == [p for p in whole if p in kept]
        entered += int(passes[whole].sum())
    assert entered > 0


def test_the_leaves_of_an_8x8_cut_are_the_tile_s_leaf_list(box):
    sd, boxes, nodes = box
    for tile in ((40, 24), (80, 40), (40, 40)):
        cam, (order, count, pos, links) = _plan(box, tile, size=(8, 8))
        o2, c2, leaves = capi.plan_primary_leaf_list(cam, tile[0], tile[1], boxes, nodes, 1 << 20)
        assert order == o2 >= 0 and c2 > 0
        assert np.array_equal(pos[nodes[order][pos, 0] >= 0], leaves)


def test_the_cap(box):
    block = BLOCKS[0]
    _, (order, count, pos, links) = _plan(box, block)
    assert count >= 2
    for cap in (count, count + 1):
        _, (o2, c2, p2, l2) = _plan(box, block, cap)
        assert (o2, c2) == (order, count) and np.array_equal(p2, pos) and np.array_equal(l2, links)
    _, (o3, c3, p3, l3) = _plan(box, block, count - 1)
    assert o3 == order and c3 == count and np.array_equal(p3, pos[:count - 1]) and len(l3) == 0      # cap + 1: past the cap, no cut
    _, (o4, c4, p4, l4) = _plan(box, block, 0)
    assert o4 == order and c4 == 1 and len(p4) == 0 and len(l4) == 0


def test_a_sign_change_inside_the_block_gives_no_order(box):
    sd, boxes, nodes = box
    cam = _camera(sd)                                # the box's own view, along -z: d.x changes sign in the middle column of blocks
    order, count, pos, links = capi.plan_primary_cut(cam, 32, 8, 32, 8, boxes, nodes, 1 << 20)
    assert order == -1 and count == 0 and len(pos) == 0
    order, count, pos, links = capi.plan_primary_cut(cam, 0, 8, 32, 8, boxes, nodes, 1 << 20)      # the block to its side has one
    assert order >= 0 and count > 0
