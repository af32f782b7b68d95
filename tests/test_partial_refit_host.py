"""CPU: the partial refit's device-free half (include/restir_hip.h rs_scene_set_partial_refit).  rs_debug_plan_refit is the decision
scene_edits.hip makes per edit (restir_amd/csrc/rs_geometry_plan.h rs_plan_refit): partial iff the switch is on, a whole refit has left
the key boxes, the edit names at most maxTriangles triangles, and the bound m x sum (depth + 1) fits the capacity.  Every case is a
made-up list of tree depths; the bound is restated here.  Then the refusals of the new entry points that need no scene, and the ABI."""
import ctypes as C

import numpy as np
import pytest

from restir_amd import capi

DEPTHS = ([0], [1], [21], [51, 17, 19, 19, 20, 20, 18, 18], [3, 2, 2, 2, 2, 2, 2, 2], [21, 9])     # one tree: a scene without grid-box trees
DEFAULT = 4096


def bound_of(m, depths):
    return m * sum(d + 1 for d in depths)


@pytest.mark.parametrize("depths", DEPTHS)
@pytest.mark.parametrize("m", [0, 1, 7, 4096, 1 << 20])
def test_bound_is_the_formula(depths, m):
    partial, bound = capi.plan_refit(1, 1 << 30, 1, m, depths, capacity=2 ** 63)
    assert bound == bound_of(m, depths) and partial


@pytest.mark.parametrize("depths", DEPTHS)
def test_off_and_keys_not_valid_are_whole(depths):
    assert capi.plan_refit(1, 16, 1, 3, depths) == (True, bound_of(3, depths))
    assert capi.plan_refit(0, 16, 1, 3, depths) == (False, bound_of(3, depths))
    assert capi.plan_refit(1, 16, 0, 3, depths) == (False, bound_of(3, depths))
    assert capi.plan_refit(0, 16, 0, 3, depths) == (False, bound_of(3, depths))


@pytest.mark.parametrize("depths", DEPTHS)
@pytest.mark.parametrize("limit", [1, 2, 255, 4096])
def test_threshold_on_triangles(depths, limit):
    assert capi.plan_refit(1, limit, 1, limit, depths)[0]
    assert not capi.plan_refit(1, limit, 1, limit + 1, depths)[0]
    assert capi.plan_refit(1, limit, 1, limit - 1, depths)[0]


@pytest.mark.parametrize("depths", DEPTHS)
def test_default_threshold(depths):
    assert capi.plan_refit(1, -1, 1, DEFAULT, depths)[0] and not capi.plan_refit(1, -1, 1, DEFAULT + 1, depths)[0]
    assert capi.plan_refit(1, -7, 1, DEFAULT, depths)[0] and not capi.plan_refit(1, -7, 1, DEFAULT + 1, depths)[0]


@pytest.mark.parametrize("depths", DEPTHS)
@pytest.mark.parametrize("m", [1, 5, 300])
def test_threshold_on_capacity(depths, m):
    b = bound_of(m, depths)
    assert capi.plan_refit(1, 1000, 1, m, depths, capacity=b) == (True, b)
    assert capi.plan_refit(1, 1000, 1, m, depths, capacity=b - 1) == (False, b)
    assert capi.plan_refit(1, 1000, 1, m, depths, capacity=b + 1) == (True, b)
    # one more triangle than the capacity takes
    assert capi.plan_refit(1, 1000, 1, m + 1, depths, capacity=b)[0] is False


def test_the_number_of_nodes_does_not_enter():
    for nodes in (0, 1, 10 ** 12):
        assert capi.plan_refit(1, 8, 1, 8, [4, 4], num_nodes=nodes) == (True, 80)


def test_the_bound_does_not_wrap_at_32_bits():
    partial, bound = capi.plan_refit(1, 2 ** 31 - 1, 1, 2 ** 31 - 1, [51] * 8)
    assert bound == (2 ** 31 - 1) * 8 * 52 and not partial           # the library's capacity: what a 32-bit owner word can name
    assert capi.plan_refit(1, 2 ** 31 - 1, 1, 2 ** 20, [51] * 8)[0]


def test_refusals():
    L = capi.lib()
    ull, ci = C.c_ulonglong, C.c_int
    bad = capi.RS_ERR_INVALID_ARGUMENT
    assert L.rs_scene_set_partial_refit(None, 1, 16) == bad
    assert b"null scene" in L.rs_last_error()
    assert L.rs_scene_get_partial_refit(None, C.byref(ci()), C.byref(ci())) == bad
    assert L.rs_scene_refit_counts(None, C.byref(ull()), C.byref(ull())) == bad
    assert L.rs_debug_scene_refit_dirty(None, C.byref(ull())) == bad
    d = np.array([3, 2], np.int32)
    p, b = ci(-1), ull(77)
    assert L.rs_debug_plan_refit(1, 4, 1, 1, 2, d.ctypes.data, 0, 100, None, C.byref(b)) == bad
    assert L.rs_debug_plan_refit(1, 4, 1, 1, 2, d.ctypes.data, 0, 100, C.byref(p), None) == bad
    assert L.rs_debug_plan_refit(1, 4, 1, 1, 2, None, 0, 100, C.byref(p), C.byref(b)) == bad
    assert L.rs_debug_plan_refit(1, 4, 1, -1, 2, d.ctypes.data, 0, 100, C.byref(p), C.byref(b)) == bad
    assert (p.value, b.value) == (-1, 77)
    assert L.rs_debug_plan_refit(1, 4, 1, 1, 0, None, 0, 100, C.byref(p), C.byref(b)) == 0 and (p.value, b.value) == (1, 0)


def test_abi_exports_the_new_symbols():
    L = capi.lib()
    for name in ("rs_scene_set_partial_refit", "rs_scene_get_partial_refit", "rs_scene_refit_counts", "rs_debug_scene_refit_dirty", "rs_debug_plan_refit"):
        assert name in capi.EXPORTS and hasattr(L, name), name
