"""GPU: the TEX / ENV variants of every render kernel on the rows of tests/texture_cases.py, held to the CPU oracle bit for bit.

Every other parity module that reaches restir_amd/csrc/rs_surface.h renders the textured Cornell box as generated.  Here its texture
coordinates are scaled by 4000 and by 1e30, moved to -5000, rounded to integers and to texel centres, NaN on one box and infinite on the
other, and the same at all three corners; its maps are 1 x 1, 1 x 7, 7 x 1 and of odd sizes, hold metallic values of -1 .. 2,
roughness 0 and 1e-6, base colours of 0, -1, 1e30, inf and NaN, normals of length 0 and normals that point inward, a normal map on
faces with |n.y| = 1; the procedural texture covers every surface; the environment map is 1 x 1, 2 x 1, 5 x 3 with one lit texel,
3 x 7, 64 x 1 and 1 x 64, holds 1e30 beside 1e-30, an infinite, a NaN and a negative texel, is black, or is the only light; the camera
looks into both poles of to_plane and along the axes; and one row puts maps and an environment map on the many-lights scene.

  * per row, at 48 x 32, extreme_cases.run against texture_cases.oracle_outputs (libm mode 1): ReSTIRDirect (3 spatiotemporal frames:
    image, ray count and reservoirs after every frame, the five G-buffer planes after the last), 2 RIS-only frames, PT-direct, pathTrace
    at depths 1 and 4, pathTraceIndirect at depth 3, 3 frames of ReSTIR-GI; the NaN counts must be the ones EXPECT states (the many-lights
    row: the two ReSTIRDirect sequences only);
  * the coordinate and texel-value rows again at 97 x 61, ReSTIRDirect with reuse 3 and 0: partial tiles, mixed waves;
  * look_up and look_down with a still camera for five frames through tests/primary_cuts.Side with cuts and leaf lists on, with both
    off and on the oracle (the rule of tests/test_gpu_camera_extremes.py);
  * the environment rows whose map has the base scene's size a second time: where rs_scene_set_texture accepts the map, the base
    scene edited equals the oracle too; where it does not (a pdf sum that is not finite and positive) it refuses, the scene unchanged,
    while creation took the same map in the first test.

One rule compares everything (extreme_cases.same_bits_or_nan): bit for bit, a NaN where the oracle holds one.  No row can index outside
a map: fract puts u into [0, 1] so that fx <= W + 1/2 and the chosen texel is at most W - 1, the `ix + 1` neighbour is brought back
by `ux >= width`, a NaN converts to 0, and sample_env_nv reads a failId that rs_build_alias_table assigns for every entry
(tests/test_texture_cases.py asserts its range on every row's map).
"""
import numpy as np
import pytest

from tests import extreme_cases as xc
from tests import texture_cases as tc
from tests.common import hip_scene, oracle_scene
from tests.primary_cuts import Side
from tests.scene_edits import assert_same
from tests.test_gpu_camera_extremes import _planes
from tests.test_gpu_parameter_extremes import HipBackend

pytestmark = pytest.mark.gpu


@pytest.fixture
def correctly_rounded_libm():
    with xc.correctly_rounded_libm():
        yield


@pytest.fixture(scope="module")
def scenes():
    """The library's scene of a row, built once (the camera rows share the base scene's)."""
    made = {}
    yield made
    for s in made.values():
        s.destroy()


def _key(name):
    return "base" if name in tc.CAMERA else name


def _held_to_the_oracle(hip, scenes, name, size, stages, all_stages=None, key=None):
    oracle = tc.oracle_outputs(name, size, all_stages)
    want = {k: v for k, v in oracle.items() if k.split("/")[0] in stages}
    assert want
    got = xc.run(HipBackend(hip, scenes, key or _key(name), size, sd=tc.scene(name)), stages)
    nans = xc.compare(want, got, (name, size))
    if size == tc.SIZE:
        stated = tc.expected(name)["nan"] if name in tc.EXPECT else {}                  # (the base scene holds none)
        assert nans == {k: v for k, v in stated.items() if k.split("/")[0] in stages}, (name, nans)
    return got


@pytest.mark.parametrize("name", tc.NAMES)
def test_restir_direct_on_textured_rows(hip, scenes, correctly_rounded_libm, name):
    got = _held_to_the_oracle(hip, scenes, name, tc.SIZE, ("direct3", "direct0"))
    res = got["direct3/f2/res"]
    assert int(np.count_nonzero((res["weight"] > 0) & (res["dist"] == tc.ENV_DIST))) == tc.expected(name)["env_live"]


@pytest.mark.parametrize("name", tc.CORNELL)
def test_baseline_passes_on_textured_rows(hip, scenes, correctly_rounded_libm, name):
    _held_to_the_oracle(hip, scenes, name, tc.SIZE, ("ptd", "pt1", "pt4", "pti3"))


@pytest.mark.parametrize("name", tc.CORNELL)
def test_restir_indirect_on_textured_rows(hip, scenes, correctly_rounded_libm, name):
    _held_to_the_oracle(hip, scenes, name, tc.SIZE, ("gi",))


@pytest.mark.parametrize("name", tc.PARTIAL)
def test_coordinate_and_texel_rows_on_partial_tiles(hip, scenes, correctly_rounded_libm, name):
    _held_to_the_oracle(hip, scenes, name, tc.RAGGED, ("direct3", "direct0"), ("direct3", "direct0"))


STILL_FRAMES = 5


@pytest.mark.parametrize("name", tc.POLES)
def test_poles_under_a_still_camera(hip, correctly_rounded_libm, name):
    """Three frames and two further ones without moving the camera: from the second frame on the library may take primary cuts and leaf
    lists; with them on and with them off every frame equals the oracle's."""
    sd = tc.scene(name)
    scene_h, scene_o = hip_scene(hip, sd), oracle_scene(sd)
    scene_h.set_sample_sequence(None); scene_o.set_sample_sequence(None)
    try:
        on = Side(hip, sd, tc.SIZE, scene=scene_h, cuts=True, lists=True)
        off = Side(hip, sd, tc.SIZE, scene=scene_h, cuts=False, lists=False)
        ref = Side(None, sd, tc.SIZE, scene=scene_o)
        for f in range(STILL_FRAMES):
            a, b, c = on.frame(), off.frame(), ref.frame()
            assert_same(c, a, "%s: cuts and lists on against the oracle, frame %d" % (name, f))
            assert_same(c, b, "%s: both off against the oracle, frame %d" % (name, f))
            pc = _planes(ref)
            assert_same(pc, _planes(on), "%s: G-buffer, cuts and lists on, frame %d" % (name, f))
            assert_same(pc, _planes(off), "%s: G-buffer, both off, frame %d" % (name, f))
        assert int(np.count_nonzero(pc["prim_id"] == -1)) == tc.expected(name)["miss"]
    finally:
        hip.synchronize()
        scene_h.destroy()


@pytest.mark.parametrize("name", list(tc.ENV_SAME_SIZE))
def test_environment_rows_by_edit_of_the_base_scene(hip, correctly_rounded_libm, name):
    """The state test_restir_direct_on_textured_rows reaches by creation, reached by rs_scene_set_texture from the base scene -- or
    refused by it, with the base scene left as it was."""
    base, row = tc.scene("base"), tc.scene(name)
    edited = {"edited": hip_scene(hip, base)}
    edited["edited"].set_sample_sequence(None)
    try:
        if tc.ENV_SAME_SIZE[name]:
            edited["edited"].set_texture(base.env_map_tex, row.textures[row.env_map_tex])
            want = name
        else:
            with pytest.raises(hip.RestirHipError, match=str(hip.RS_ERR_INVALID_ARGUMENT)):
                edited["edited"].set_texture(base.env_map_tex, row.textures[row.env_map_tex])
            want = "base"
        _held_to_the_oracle(hip, edited, want, tc.SIZE, ("direct3",), ("direct3",) if want == "base" else None, key="edited")
    finally:
        hip.synchronize()
        edited["edited"].destroy()
