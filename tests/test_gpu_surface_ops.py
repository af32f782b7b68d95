"""GPU: the functions of restir_amd/csrc/rs_surface.h that the textured and environment-map kernel variants are built on, each called
as it is through rs_debug_surface_ops (surface_checks.hip), one lane per row, and held to the oracle's function bit for bit.

The rendered parity scenes reach these functions with coordinates within a few units of [0, 1], maps of 8 - 64 texels a side and
directions away from the poles.  The rows of tests/surface_cases.py are what they never see: linear_sample at exact texel borders and
centres (the branch `fract(fx) > .5f`), at fract = 0 and fract = 1 (a tiny negative coordinate), on maps of one texel a side (every
neighbour wraps onto the same texel) and 8192 across, at 2^23 and 1e30, at infinities and NaN (f2i(NaN) = 0: the device's conversion
against the oracle's emulation of it); procedural_texture where its seed arithmetic leaves `int` (|u| >= 2048), where f2i saturates
(|u| >= 2 097 152), at the two seeds that are 0 mod 2^31 - 1 and at 1e30 (a large-argument reduction in sin); to_sphere at the texel
centres of small environment maps and the exact quarters; to_plane at the poles, on the seam (atan2(+-0, -x)), at the zero vector,
with subnormal components and with 1e30, whose square overflows; local_to_world with |n.y| at 0.9999f and the float on each side.

The device's sin / cos / atan2 are ocml's double routines rounded to float, the oracle's (libm mode 1) glibc's double routines rounded
to float: "the correctly rounded float on both sides" is what this module asserts per argument.  Rule:
extreme_cases.same_bits_or_nan -- a NaN where the oracle holds one, every other bit equal.  NAN_ROWS states how many rows of each list
the ORACLE answers with a NaN, so that no comparison passes because everything was NaN.
"""
import numpy as np
import pytest

from oracle import binding as ob
from tests import extreme_cases as xc
from tests import surface_cases as sc

pytestmark = pytest.mark.gpu

# rows whose oracle output holds a NaN / rows of the list
NAN_ROWS = {
    ("linear_sample", (1, 1)): (12, 200087), ("linear_sample", (1, 7)): (15, 200159), ("linear_sample", (7, 1)): (15, 200159),
    ("linear_sample", (2, 2)): (12, 200105), ("linear_sample", (37, 53)): (15, 200927), ("linear_sample", (3, 8192)): (3606, 298391),
    "procedural_texture": (10, 200091), "to_sphere": (0, 202091), "to_plane": (91, 201009), "local_to_world": (155, 20288),
}


@pytest.fixture
def correctly_rounded_libm():
    with xc.correctly_rounded_libm():
        yield


def _held(key, want, got, rows):
    nan_rows = int(np.isnan(want).any(axis=1).sum())
    print(key, "rows", len(rows), "oracle NaN rows", nan_rows)
    assert (nan_rows, len(rows)) == NAN_ROWS[key], (key, nan_rows, len(rows))
    differ = (want.view(np.uint32) != got.view(np.uint32)).any(axis=1) & ~(np.isnan(want) & np.isnan(got)).any(axis=1)
    print(key, "rows that differ", int(differ.sum()), rows[differ][:8], want[differ][:8], got[differ][:8])
    xc.same_bits_or_nan(want, got, key)


@pytest.mark.parametrize("shape", sc.TEXTURE_SHAPES, ids=["%dx%d" % s for s in sc.TEXTURE_SHAPES])
def test_linear_sample(hip, correctly_rounded_libm, shape):
    rows, tex = sc.linear_sample_rows(shape), sc.texture(shape)
    _held(("linear_sample", shape), ob.linear_sample(tex, rows), hip.surface_op("linear_sample", rows, tex), rows)


def test_procedural_texture(hip, correctly_rounded_libm):
    rows = sc.procedural_texture_rows()
    want = ob.procedural_texture(rows)
    _held("procedural_texture", want, hip.surface_op("procedural_texture", rows), rows)
    zero = want[-len(sc.SEED_ZERO) - 8:-8]
    assert np.isfinite(zero).all() and zero.shape == (2, 3)          # (the two seeds that are 0 mod 2^31 - 1 were in the list)


def test_to_sphere(hip, correctly_rounded_libm):
    rows = sc.to_sphere_rows()
    _held("to_sphere", ob.to_sphere(rows), hip.surface_op("to_sphere", rows), rows)


def test_to_plane(hip, correctly_rounded_libm):
    rows = sc.to_plane_rows()
    _held("to_plane", ob.to_plane(rows), hip.surface_op("to_plane", rows), rows)


def test_local_to_world(hip, correctly_rounded_libm):
    rows = sc.local_to_world_rows()
    want = ob.local_to_world(np.ascontiguousarray(rows[:, :3]), np.ascontiguousarray(rows[:, 3:]))
    _held("local_to_world", want, hip.surface_op("local_to_world", rows), rows)


def test_refusals(hip):
    one = np.zeros((1, 6), np.float32)
    L, p = hip.lib(), lambda a: a.ctypes.data
    assert L.rs_debug_surface_ops(1, 1, None, p(one), 0, 0, None) == hip.RS_ERR_INVALID_ARGUMENT
    assert L.rs_debug_surface_ops(1, 1, p(one), None, 0, 0, None) == hip.RS_ERR_INVALID_ARGUMENT
    assert L.rs_debug_surface_ops(1, -1, p(one), p(one), 0, 0, None) == hip.RS_ERR_INVALID_ARGUMENT
    assert L.rs_debug_surface_ops(5, 1, p(one), p(one), 0, 0, None) == hip.RS_ERR_INVALID_ARGUMENT
    assert L.rs_debug_surface_ops(-1, 1, p(one), p(one), 0, 0, None) == hip.RS_ERR_INVALID_ARGUMENT
    assert L.rs_debug_surface_ops(0, 1, p(one), p(one), 0, 1, p(one)) == hip.RS_ERR_INVALID_ARGUMENT
    assert L.rs_debug_surface_ops(0, 1, p(one), p(one), 1, -1, p(one)) == hip.RS_ERR_INVALID_ARGUMENT
    assert L.rs_debug_surface_ops(0, 1, p(one), p(one), 1, 1, None) == hip.RS_ERR_INVALID_ARGUMENT
    assert L.rs_debug_surface_ops(1, 0, p(one), p(one), 0, 0, None) == 0
