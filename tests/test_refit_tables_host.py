"""The restatement of the refit's device tables (tests/refit_tables.py) pinned on the host, no GPU: its grid_box against the library's own
(rs_debug_grid_box is rs::grid_box as is) on boxes at and one ulp around every plane and edge of a grid, its keyed min / max against
rs_refit_boxes, its stack walk on hand-made trees; and the refusals of the debug calls that need no device."""
import ctypes as C

import numpy as np
import pytest

from restir_amd import capi, scenes
from tests.geometry_edits import apply_triangles, extreme_edit, geometry_edit, root_box, soup_scene
from tests.refit_tables import grid_box, leaf_slots, refit_boxes_bits, tree_length, walk_preorder

INVALID = 10001                                             # RS_ERR_INVALID_ARGUMENT


def grid_over(lo, hi):
    """A grid as rs_quantize_occlusion_bvh lays one: 65 535 cells over the box and a margin of 2^-17 of its largest extent.  (What is
    pinned here is grid_box on a given grid, so how the library chooses base, scale and margin does not matter.)"""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    ext = (hi.astype(np.float64) - lo)
    margin = float(ext.max()) * 2.0 ** -17
    base = (lo.astype(np.float64) - 2 * margin).astype(np.float32)
    scale = ((ext + 4 * margin) / 65535.0 * (1 + 2.0 ** -20)).astype(np.float32)
    return base, scale, margin


GRIDS = [((-1, 0, -1), (1, 2, 1)), ((0, 0, 0), (1, 1, 1)), ((-1234.5, -0.001, 3.0), (877.25, 0.002, 3.5)),
         ((-3e-3, -2e3, 1e4), (5e-3, 9e3, 1.00001e4)), ((-1e-30, -1, -1e10), (1e-30, 1, 1e10))]


def boxes_for(lo, hi, base, scale, margin, rng):
    """(n, 3) lo and hi of the boxes of the issue for one grid."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    up, down = (lambda x: np.nextafter(x, np.float32(np.inf))), (lambda x: np.nextafter(x, np.float32(-np.inf)))
    out = []
    a = rng.uniform(lo, hi, (1500, 3)).astype(np.float32); b = rng.uniform(lo, hi, (1500, 3)).astype(np.float32)
    out.append((np.minimum(a, b), np.maximum(a, b)))                       # random boxes inside
    out.append((a[:300], a[:300]))                                         # zero extent
    for j in range(6):                                                     # flat on each face
        l, h = np.minimum(a[:50], b[:50]).copy(), np.maximum(a[:50], b[:50]).copy()
        l[:, j >> 1] = h[:, j >> 1] = (lo, hi)[j & 1][j >> 1]
        out.append((l, h))
    corners = np.array([[(lo, hi)[(j >> k) & 1][k] for k in range(3)] for j in range(8)], np.float32)
    out.append((corners, corners))                                         # points on the corners
    out.append((np.repeat(lo[None], 8, 0), corners)); out.append((corners, np.repeat(hi[None], 8, 0)))
    # lo - margin or hi + margin exactly on a plane of the grid, and one float32 ulp to either side
    q = rng.integers(1, 65535, (800, 3))
    plane = base.astype(np.float64) + q * scale.astype(np.float64)
    for sign in (1.0, -1.0):
        x = (plane + sign * margin).astype(np.float32)                     # (the float nearest the value that lands on the plane)
        x = np.clip(x, lo, hi)
        for y in (x, up(x), down(x), up(up(x)), down(down(x))):
            y = np.clip(y, lo, hi).astype(np.float32)
            out.append((y, y))
            out.append((np.minimum(y, a[:800]), np.maximum(y, a[:800])))
    # one ulp outside the grid's 16 bits: planes 0 and 65535 are the last ones
    first = base.astype(np.float64); last = base.astype(np.float64) + 65535.0 * scale.astype(np.float64)
    inner = rng.uniform(lo, hi, (60, 3)).astype(np.float32)
    for k in range(3):
        x = inner.copy(); x[:, k] = (first[k] + margin).astype(np.float32)
        for y in (x[:, k].copy(), down(x[:, k]), down(down(x[:, k]))):
            z = x.copy(); z[:, k] = y
            out.append((z, np.maximum(z, inner)))
        x = inner.copy(); x[:, k] = (last[k] - margin).astype(np.float32)
        for y in (x[:, k].copy(), up(x[:, k]), up(up(x[:, k]))):
            z = x.copy(); z[:, k] = y
            out.append((np.minimum(z, inner), z))
    return np.concatenate([o[0] for o in out]).astype(np.float32), np.concatenate([o[1] for o in out]).astype(np.float32)


def test_python_grid_box_equals_the_library():
    """At least 20 000 boxes over grids of several extents; a box that does not fit leaves `out` untouched and says fits == 0."""
    rng = np.random.default_rng(1)
    L = capi.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    total = refused = 0
    for lo, hi in GRIDS:
        base, scale, margin = grid_over(lo, hi)
        blo, bhi = boxes_for(lo, hi, base, scale, margin, rng)
        want, fits = grid_box(blo, bhi, base, scale, margin)
        out, flag = np.zeros(3, np.uint32), C.c_int(0)
        for i in range(len(blo)):
            out[:] = 0xdeadbeef
            assert L.rs_debug_grid_box(p(blo[i]), p(bhi[i]), p(base), p(scale), margin, p(out), C.byref(flag)) == 0
            assert flag.value == int(fits[i]), (lo, hi, i, blo[i], bhi[i])
            if flag.value:
                assert np.array_equal(out, want[i]), (lo, hi, i, blo[i], bhi[i], out, want[i])
            else:
                assert (out == 0xdeadbeef).all()
        total += len(blo); refused += int((~fits).sum())
    assert total >= 20000 and refused >= 100, (total, refused)
    for bad in (np.nan, np.inf, -np.inf):                                  # not finite: refused, not looped on
        l = np.array([0.5, bad, 0.5], np.float32)
        assert not grid_box(l, l, *grid_over((0, 0, 0), (1, 1, 1)))[1][0]
        assert capi.grid_box(l, l, *grid_over((0, 0, 0), (1, 1, 1)))[0] is None


@pytest.mark.parametrize("name", ["cornell", "sponza", "soup2", "soup257"])
def test_keyed_min_max_equals_rs_refit_boxes(name):
    """refit_boxes_bits (NumPy, on keys) and rs_refit_boxes give the same bits, signed zeros and subnormal extents included."""
    sd = {"cornell": scenes.cornell_box, "sponza": lambda: scenes.sponza_class(1, 0.01)}.get(name, lambda: soup_scene(int(name[4:])))()
    _, nodes = capi.build_bvh(sd.vertices)
    v, n = sd.vertices.reshape(-1, 3, 3).copy(), sd.normals.reshape(-1, 3, 3).copy()
    lo, hi = root_box(v)
    edits = [geometry_edit(sd, v, "all", seed=4)]
    if name != "soup2":
        edits += [extreme_edit(sd, v, k, lo, hi) for k in ("corners", "tiny_edges", "signed_zeros")]
    for ids, ev, en in edits:
        v, n = apply_triangles(v, n, ids, ev, en)
        a, b = refit_boxes_bits(v, nodes[0]), capi.refit_boxes(v, nodes[0])
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    if name == "cornell":
        assert np.signbit(a[a == 0]).any() and not np.signbit(a[a == 0]).all()


def leaf(first, count):
    return ~(first * 8 + count)


def test_stack_walk_on_hand_made_trees():
    # 1 leaf
    parent, depth, end, slots = walk_preorder([leaf(0, 3)])
    assert list(parent) == [-1] and list(end) == [1] and slots == [[0, 1, 2]]
    # 2 leaves
    parent, depth, end, slots = walk_preorder([32, leaf(0, 1), leaf(1, 2)])
    assert list(parent) == [-1, 0, 0] and list(depth) == [0, 1, 1] and list(end) == [3, 2, 3] and slots == [None, [0], [1, 2]]
    # 3 leaves, the inner child second, and first: ((a) (b c)) and ((a b) c)
    parent, depth, end, slots = walk_preorder([0, leaf(0, 1), 0, leaf(1, 1), leaf(2, 1)])
    assert list(parent) == [-1, 0, 0, 2, 2] and list(depth) == [0, 1, 1, 2, 2] and list(end) == [5, 2, 5, 4, 5]
    parent, depth, end, slots = walk_preorder([0, 0, leaf(0, 1), leaf(1, 1), leaf(2, 1)])
    assert list(parent) == [-1, 0, 1, 1, 0] and list(end) == [5, 4, 3, 4, 5]
    # 7 leaves, lopsided: a chain to the left with a balanced pair of pairs at the bottom
    w = [0, 0, 0, 0, leaf(0, 1), leaf(1, 1), 0, leaf(2, 2), leaf(4, 1), leaf(5, 1), 0, leaf(6, 7), leaf(13, 1)]
    parent, depth, end, slots = walk_preorder(w)
    assert list(parent) == [-1, 0, 1, 2, 3, 3, 2, 6, 6, 1, 0, 10, 10]
    assert list(depth) == [0, 1, 2, 3, 4, 4, 3, 4, 4, 2, 1, 2, 2]
    assert list(end) == [13, 10, 9, 6, 5, 6, 9, 8, 9, 10, 13, 12, 13]
    assert [s for x in slots if x for s in x] == list(range(14))
    assert tree_length(w + [0, 0]) == 13 and tree_length([leaf(0, 1), 0]) == 1
    # a mirrored order counts down
    assert leaf_slots(leaf(9, 3), -1) == [9, 8, 7]
    assert walk_preorder([0, leaf(2, 2), leaf(0, 1)], step=-1)[3] == [None, [2, 1], [0]]
    # a second root, and an array that ends inside a tree
    with pytest.raises(ValueError, match="second root"):
        walk_preorder([0, leaf(0, 1), leaf(1, 1), leaf(2, 1)])
    with pytest.raises(ValueError, match="second root"):
        walk_preorder([leaf(0, 1), leaf(1, 1)])
    with pytest.raises(ValueError, match="ends inside"):
        walk_preorder([0, leaf(0, 1)])
    with pytest.raises(ValueError):
        walk_preorder([])


def test_debug_calls_refuse_null_arguments_without_a_device():
    L = capi.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    size = C.c_size_t(77)
    buf = np.full(64, 0xab, np.uint8)
    assert L.rs_debug_scene_table(None, 0, None, 0, C.byref(size)) == INVALID and size.value == 77
    assert L.rs_debug_scene_table(None, 0, p(buf), buf.size, C.byref(size)) == INVALID and (buf == 0xab).all()
    assert b"rs_debug_scene_table" in L.rs_last_error()
    f = np.full(3, 7.0, np.float32)
    margin, count = C.c_double(7.0), C.c_int(7)
    assert L.rs_debug_scene_grid(None, p(f), p(f), C.byref(margin), p(f), p(f), C.byref(count), C.byref(count)) == INVALID
    assert (f == 7.0).all() and margin.value == 7.0 and count.value == 7
    lo, one = np.zeros(3, np.float32), np.ones(3, np.float32)
    out, fits = np.full(3, 5, np.uint32), C.c_int(5)
    for args in ((None, p(one), p(lo), p(one), 0.0, p(out), C.byref(fits)), (p(lo), None, p(lo), p(one), 0.0, p(out), C.byref(fits)),
                 (p(lo), p(one), None, p(one), 0.0, p(out), C.byref(fits)), (p(lo), p(one), p(lo), None, 0.0, p(out), C.byref(fits)),
                 (p(lo), p(one), p(lo), p(one), 0.0, None, C.byref(fits)), (p(lo), p(one), p(lo), p(one), 0.0, p(out), None)):
        assert L.rs_debug_grid_box(*args) == INVALID
        assert (out == 5).all() and fits.value == 5
