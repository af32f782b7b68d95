"""CPU: the table of tests/texture_cases.py on the oracle alone.

  * every row does what it is there for: the oracle's outputs at 48 x 32 give the figures of EXPECT -- miss pixels, pixels whose hit
    carries a mapped material, live reservoirs and those that hold an environment sample, albedo pixels and reservoirs that differ from
    the base scene's, and which outputs hold NaN or infinity, with their counts;
  * no row equals the base scene: each changes at least one albedo or reservoir bit;
  * every environment row leaves a live reservoir on the environment entry, or is listed in NO_LIVE_ENV with the reason it cannot;
  * the rows whose extreme sits on one box put both kinds of pixel into one 32 x 8 tile, at 48 x 32 and at 97 x 61;
  * the host side of the library at the same extremes: rs_build_envmap_pdf and rs_build_alias_table against the oracle on every row's
    environment map, and rs_scene_create's refusal of a normal-map id of -2 (check_materials; it is refused before any device work).
    That rs_scene_set_texture refuses the black, infinite and NaN environment maps which creation takes needs an rs_scene, hence a
    device: tests/test_gpu_texture_extremes.py asserts it.
"""
import numpy as np
import pytest

from oracle import binding as ob
from restir_amd import capi
from tests import extreme_cases as xc
from tests import texture_cases as tc


@pytest.fixture(autouse=True)
def correctly_rounded_libm():
    with xc.correctly_rounded_libm():
        yield


def test_the_table_holds_the_rows_it_was_asked_for():
    assert len(tc.NAMES) == len(set(tc.NAMES)) == len(tc.EXPECT) == 39
    assert [n for n in tc.NAMES if n not in tc.CORNELL] == ["bistro_textured"]
    assert len(tc.COORDINATES) == 8 and len(tc.TEXELS) == 7 and set(tc.MIXED) <= set(tc.PARTIAL) and set(tc.POLES) <= set(tc.CAMERA)
    assert set(tc.ENV_SAME_SIZE) <= set(tc.ENVIRONMENT) and set(tc.NO_LIVE_ENV) <= set(tc.ENVIRONMENT)
    base = tc.scene("base")
    for name, same in tc.ENV_SAME_SIZE.items():
        assert tc.scene(name).textures[tc.ENV_MAP].shape == base.textures[tc.ENV_MAP].shape
    sd = tc.scene("bistro_textured")
    assert sd.env_map_tex == 1 and sd.textures[1].shape == (4, 8, 3) and len(tc.mapped_materials(sd)) == 1
    from restir_amd.ctypes_structs import LIGHT
    assert int((sd.materials["type"][sd.material_ids] == LIGHT).sum()) > 1024          # k_ris reads the light table from global memory
    for name in tc.CAMERA:                                                              # camera rows share the base scene's arrays
        assert all(np.array_equal(a, b) for a, b in zip(tc.scene(name).textures, base.textures))


@pytest.mark.parametrize("name", tc.NAMES)
def test_row_is_not_vacuous(name):
    o, base = tc.oracle_outputs(name), tc.base_outputs(name)
    got, want = tc.figures(name, o, base), tc.expected(name)
    assert got == want, (name, got, want)
    n = tc.SIZE[0] * tc.SIZE[1]
    assert got["albedo_differs"] + got["res_differs"] > 0                               # no row equals the base scene
    assert got["miss"] + got["mapped"] > n // 2                                         # most pixels go through rs_surface.h
    if name in tc.ENVIRONMENT:
        assert (got["env_live"] == 0) if name in tc.NO_LIVE_ENV else (got["env_live"] > 0), (name, got["env_live"])
    if name in tc.CAMERA and name != "look_nz":
        assert got["miss"] == n                                                         # the whole frame is the environment map
        assert len(np.unique(o["direct3/gbuffer/albedo"].view(np.uint32), axis=0)) > 8  # ... and not one texel of it
    if name in tc.POLES:
        d = tc.scene(name).camera(*tc.SIZE)
        ob.camera_update(d)
        assert abs(d.view[1]) > 0.999999 and max(abs(d.view[0]), abs(d.view[2])) < 1e-6
    if name in ("uv_nan_tall_box", "base_map_nan_texel"):
        assert want["nan"]["direct3/gbuffer/albedo"] > 0 and want["nan"]["direct3/f2/image"] > 0
    if name in ("normal_map_half", "uv_inf_short_box"):
        assert want["nan"]["direct3/gbuffer/normal"] > 100                              # NaN normals reach the G-buffer, and no image
        assert not any(k.endswith("image") and k.startswith("direct") for k in want["nan"])
    if name == "env_dynamic_range":
        img = o["direct3/f2/image"]
        assert np.isfinite(img).all() and img.max() > 2.0 ** 60
    if name == "env_only_light":
        assert got["live"] == got["env_live"] > 0
    if name in ("env_inf_texel", "env_nan_texel"):
        assert got["live"] == 0
    for key, a in o.items():
        if not isinstance(a, int) and not a.dtype.names and a.dtype == np.float32 and key not in want["inf"] and key not in want["nan"]:
            assert np.isfinite(a).all(), key


@pytest.mark.parametrize("size", [tc.SIZE, tc.RAGGED], ids=["48x32", "97x61"])
@pytest.mark.parametrize("name", list(tc.MIXED))
def test_mixed_rows_put_both_kinds_of_pixel_into_one_tile(name, size):
    tiles, both = tc.mixed_tiles(name, size)
    assert tiles >= 2 and both >= 2, (tiles, both)


@pytest.mark.parametrize("name", tc.PARTIAL)
def test_partial_rows_render_at_the_ragged_size(name):
    o = tc.oracle_outputs(name, tc.RAGGED, ("direct3", "direct0"))                     # (what the GPU module compares at this size)
    assert xc.live(o["direct3/f2/res"]) >= tc.RAGGED[0] * tc.RAGGED[1] // 8


@pytest.mark.parametrize("name", tc.ENVIRONMENT)
def test_environment_sampler_of_every_row_on_the_host(name):
    """rs_build_envmap_pdf and rs_build_alias_table (what rs_scene_build_textured builds of the map) against the oracle's, bit for bit;
    every failId is an index into the table, whatever the texels."""
    sd = tc.scene(name)
    env = np.ascontiguousarray(sd.textures[sd.env_map_tex], np.float32)
    pa, pb = capi.build_envmap_pdf(env), ob.envmap_pdf(env)
    xc.same_bits_or_nan(pb, pa, (name, "pdf"))
    (prob_a, fail_a, sum_a), (prob_b, fail_b, sum_b) = capi.build_alias_table(pb), ob.alias_build(pb)
    xc.same_bits_or_nan(prob_b, prob_a, (name, "prob"))
    assert np.array_equal(fail_a, fail_b) and ((fail_a >= 0) & (fail_a < env.shape[0] * env.shape[1])).all()
    assert sum_a == sum_b or (np.isnan(sum_a) and np.isnan(sum_b))
    # ... and the light sampler with the map's entry last (its power is the pdf's sum, whatever that is)
    _, _, power = capi.build_light_table(sd.vertices, sd.material_ids, sd.materials)
    power = np.concatenate([power, np.array([sum_b], np.float32)])
    (prob_a, fail_a, total_a), (prob_b, fail_b, total_b) = capi.build_alias_table(power), ob.alias_build(power)
    xc.same_bits_or_nan(prob_b, prob_a, (name, "light prob"))
    assert np.array_equal(fail_a, fail_b) and ((fail_a >= 0) & (fail_a < len(power))).all()
    if name in tc.ENV_SAME_SIZE:                                                        # what rs_scene_set_texture accepts: a finite positive sum
        assert tc.ENV_SAME_SIZE[name] == bool(np.isfinite(sum_b) and sum_b > 0), (name, sum_b)


def test_a_normal_map_id_of_minus_2_is_refused():
    """check_materials: -2 is the procedural BASE-COLOUR texture; as a normal map it is an error (as metallic / roughness it is ignored:
    the row metal_rough_ids_minus2)."""
    sd = tc.scene("base")
    mats = sd.materials.copy()
    mats[5]["normalMapId"] = -2
    with pytest.raises(capi.RestirHipError, match=str(capi.RS_ERR_INVALID_ARGUMENT)):
        capi.Scene(sd.vertices, sd.normals, sd.texcoords, sd.material_ids, mats, textures=sd.textures, env_map_tex=sd.env_map_tex)
