"""No GPU: the host's part of tests/emitter_tables.py.  The NumPy grid and box functions agree with the library's own (rs_debug_grid_box),
the slot matching finds the primitive of every emiTris record, a hand-made emissive tree gets the boxes a brute-force union gives, and
the new entry points refuse a null scene."""
import ctypes as C

import numpy as np

from restir_amd import capi
from restir_amd.capi import GRID_DTYPE, TRI_DTYPE
from tests.emitter_edits import emissive_root_box, emitters, edits_up_to, scene_data
from tests.emitter_tables import grid_over_box, slot_prims
from tests.refit_tables import GridTree, grid_box


def test_grid_over_box_holds_every_emissive_box():
    """On the grid laid over the emissive root box, every emitter's AABB and the root box itself fit, and the NumPy grid_box gives the
    dwords rs_debug_grid_box gives.  A root box without extent has no grid (scale 0)."""
    for name in ("cornell", "single", "many", "bistro"):
        sd = scene_data(name)
        for kind in ("one", "carry_min", "carry_max", "scale_up"):
            v = edits_up_to(name, kind)[2]
            lo, hi = emissive_root_box(sd, v)
            g = grid_over_box(lo, hi)
            assert (g["scale"] > 0).all() and g["margin"] > 0
            tri = v[emitters(sd)]
            blo, bhi = np.concatenate([tri.min(1), lo[None]]), np.concatenate([tri.max(1), hi[None]])
            q, fits = grid_box(blo, bhi, g["base"], g["scale"], g["margin"])
            assert fits.all(), (name, kind)
            for j in (0, len(blo) // 2, len(blo) - 1):
                want, _ = capi.grid_box(blo[j], bhi[j], g["base"], g["scale"], g["margin"])
                assert want is not None and np.array_equal(np.asarray(want, np.uint32), q[j]), (name, kind, j)
    point = np.float32([0.25, 1.0, -0.5])
    assert (grid_over_box(point, point)["scale"] == 0).all()


def test_slot_prims_and_a_hand_made_tree():
    """Five emitters in three leaves under two inner records, in pre-order: slot_prims recovers the primitive of every slot from the
    nine floats, and GridTree's boxes are the unions a brute-force walk of the spans gives."""
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, (9, 3, 3)).astype(np.float32)
    emi = np.array([1, 3, 4, 6, 8])
    order = np.array([6, 1, 8, 3, 4])                     # the primitive in every slot
    tris = np.zeros(9, TRI_DTYPE)
    tris["v0"], tris["e1"], tris["e2"] = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    emi_tris = tris[order].copy()
    assert np.array_equal(slot_prims(emi_tris, tris, emi), order)
    # root(inner) -> leaf{0,1}, inner -> leaf{2}, leaf{3,4}
    leaf = lambda first, count: ~(first * 8 + count)
    rec = np.zeros(6, GRID_DTYPE)
    rec["w"] = [5 * 16, leaf(0, 2), 5 * 16, leaf(2, 1), leaf(3, 2), 5 * 16]
    tree = GridTree(rec.view(rec.dtype), 0, 5, 0, 5 * 16, order, 1)
    lo, hi = tree.boxes(v.min(1), v.max(1))
    spans = [order, order[:2], order[2:], order[2:3], order[3:]]
    for i, span in enumerate(spans):
        assert np.array_equal(lo[i], v[span].reshape(-1, 3).min(0)) and np.array_equal(hi[i], v[span].reshape(-1, 3).max(0)), i


def test_null_scene_is_refused():
    L = capi.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ids, v = np.zeros(1, np.int32), np.zeros(9, np.float32)
    assert L.rs_scene_set_geometry(None, 1, p(ids), p(v), None) == 10001
    f, margin, n = np.zeros(3, np.float32), C.c_double(0), C.c_int(0)
    assert L.rs_debug_scene_emissive_grid(None, p(f), p(f), C.byref(margin), C.byref(n), C.byref(n)) == 10001
