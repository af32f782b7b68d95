"""rs_refit_boxes on the host (no GPU): a refit of the untouched vertices gives the boxes rs_build_bvh built -- the proof that a refitted
scene and one built by the reference's builder hold the same boxes -- and after edits every box is the exact union the definition
names.  The refusals that need no device."""
import ctypes as C
import functools

import numpy as np
import pytest

from restir_amd import capi, scenes
from tests.geometry_edits import apply_triangles, geometry_edit, numpy_refit, root_box, tree_children, tree_depth

# sponza_class(1, s): the reference tree is 22 deep at s = 0.01 (2 621 triangles, 61 mod 64) and 18 deep at s = 0.005 (1 311 triangles)
SPONZA_SCALE = 0.01


@functools.lru_cache(maxsize=None)
def built(name):
    sd = scenes.cornell_box() if name == "cornell" else scenes.sponza_class(1, SPONZA_SCALE)
    boxes, nodes = capi.build_bvh(sd.vertices)
    return sd, boxes, nodes


@pytest.mark.parametrize("name", ["cornell", "sponza"])
def test_refit_of_untouched_vertices_equals_the_built_boxes(name):
    sd, boxes, nodes = built(name)
    if name == "sponza":
        assert tree_depth(nodes[0]) > 20 and len(sd.vertices) % 64 != 0
    refit = capi.refit_boxes(sd.vertices, nodes[0])
    assert np.array_equal(refit, boxes)                      # as float values: -0 == +0
    assert np.array_equal(numpy_refit(sd.vertices, nodes[0]), boxes)


def test_sponza_scale_is_the_smallest_deeper_than_20():
    sd = scenes.sponza_class(1, SPONZA_SCALE / 2)
    assert tree_depth(capi.build_bvh(sd.vertices)[1][0]) <= 20


def check_boxes(vertices, nodes, boxes):
    v = np.asarray(vertices, np.float32).reshape(-1, 3, 3)
    inner, leaves = tree_children(nodes[0])
    for node, a, b in inner:                                 # every box is the union of its children: contains them, and no larger
        assert np.array_equal(boxes[node, :3], np.minimum(boxes[a, :3], boxes[b, :3]))
        assert np.array_equal(boxes[node, 3:], np.maximum(boxes[a, 3:], boxes[b, 3:]))
    for prim, leaf in leaves.items():
        assert np.array_equal(boxes[leaf, :3], v[prim].min(0)) and np.array_equal(boxes[leaf, 3:], v[prim].max(0))
    lo, hi = root_box(v)
    root = nodes[0][0, 1]
    assert np.array_equal(boxes[root, :3], lo) and np.array_equal(boxes[root, 3:], hi)


@pytest.mark.parametrize("name", ["cornell", "sponza"])
def test_boxes_after_moving_triangles(name):
    sd, boxes0, nodes = built(name)
    v, n = sd.vertices.reshape(-1, 3, 3).copy(), sd.normals.reshape(-1, 3, 3).copy()
    volume = lambda b: np.prod((b[:, 3:] - b[:, :3]).astype(np.float64), axis=1)
    for kind in ("carry", "one", "all", "repeated"):
        ids, ev, en = geometry_edit(sd, v, kind, seed=3)
        v, n = apply_triangles(v, n, ids, ev, en)
        boxes = capi.refit_boxes(v, nodes[0])
        check_boxes(v, nodes, boxes)
        assert np.array_equal(numpy_refit(v, nodes[0]), boxes), kind
        if kind == "carry":
            # a triangle carried across the scene grows its ancestors' boxes; carried back, they shrink to what they were
            carried = boxes
            assert (volume(carried) > volume(boxes0)).any()
            back_ids, back_v, _ = geometry_edit(sd, v, "carry_back")
            v, n = apply_triangles(v, n, back_ids, back_v)
            back = capi.refit_boxes(v, nodes[0])
            assert np.array_equal(back, boxes0)
            assert (volume(back) <= volume(carried)).all() and (volume(back) < volume(carried)).any()


def test_signed_zeros_do_not_depend_on_the_order():
    """-0 is taken as less than +0: a box over { -0, +0 } is [-0, +0] whichever vertex comes first."""
    sd, _, nodes = built("cornell")
    v = sd.vertices.reshape(-1, 3, 3).copy()
    v[0, :, 0] = (-0.0, 0.0, 0.0)
    a = capi.refit_boxes(v, nodes[0])
    v[0, :, 0] = (0.0, 0.0, -0.0)
    b = capi.refit_boxes(v, nodes[0])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    _, leaves = tree_children(nodes[0])
    assert np.signbit(a[leaves[0], 0]) and not np.signbit(a[leaves[0], 3])


def test_refusals_without_a_device():
    sd, _, nodes = built("cornell")
    L = capi.lib()
    v = np.ascontiguousarray(sd.vertices, np.float32).reshape(-1)
    o = np.ascontiguousarray(nodes[0], np.int32)
    n, size = v.size // 9, len(o)
    out = np.zeros((size, 6), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(code):
        assert code == 10001, code                           # RS_ERR_INVALID_ARGUMENT
        assert not out.any()                                 # nothing was written
    refused(L.rs_refit_boxes(n, None, size, p(o), p(out)))
    refused(L.rs_refit_boxes(n, p(v), size, None, p(out)))
    refused(L.rs_refit_boxes(n, p(v), size, p(o), None))
    refused(L.rs_refit_boxes(n, p(v), size - 1, p(o), p(out)))
    refused(L.rs_refit_boxes(0, p(v), -1, p(o), p(out)))
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy(); w[13] = bad
        refused(L.rs_refit_boxes(n, p(w), size, p(o), p(out)))
    for prim in (n, -2):
        q = o.copy(); q[np.nonzero(q[:, 0] >= 0)[0][0], 0] = prim
        refused(L.rs_refit_boxes(n, p(v), size, p(q), p(out)))
    q = o.copy(); q[1, 2] = 0                               # a link that points backwards
    refused(L.rs_refit_boxes(n, p(v), size, p(q), p(out)))
    q = o.copy(); q[3, 1] = size                            # a boundingBoxId out of range
    refused(L.rs_refit_boxes(n, p(v), size, p(q), p(out)))
    # rs_scene_set_triangles: a null scene, whatever else it is handed
    ids = np.zeros(1, np.int32)
    assert L.rs_scene_set_triangles(None, 1, p(ids), p(v), None) == 10001
