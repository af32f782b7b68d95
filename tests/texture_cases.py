"""Texture maps, texture coordinates and the environment map at their extremes: a table of named edits of get_scene("cornell_textured"),
the oracle's outputs for each and the figures that make a row non-vacuous.  The fourth of a frame's inputs beside materials and lights
(tests/extreme_cases.py), the camera (tests/camera_cases.py) and geometry (tests/geometric_cases.py).

Every other parity module that reaches restir_amd/csrc/rs_surface.h renders the textured Cornell box as generated: maps of 16 x 32,
16 x 16 and 8 x 8 texels with values in (0, 1), coordinates within a few units of [0, 1], a normal map whose z is always 1, a smooth
32 x 64 sky seen away from its poles.  A row here is a name and a function that edits a fresh copy of that scene -- its coordinates, its
maps, the map ids of its materials, its environment map or its camera arguments; no scene generator changes.  One row gives
get_scene("bistro:0.12") coordinates, a base-colour map and a 4 x 8 environment map: the TEX / ENV kernel variants over a light table
read from global memory (ReSTIR direct only, as extreme_cases' bistro_spread).

The rules -- the call sequence `run`, the two back ends' interface, `compare` / `same_bits_or_nan`, `nan_counts`, `inf_counts`, `live`,
the libm mode -- are tests/extreme_cases.py's and are used from there.  `oracle_outputs(name, size)` is computed once per row and size
and shared; `EXPECT[name]` holds the oracle's figures at 48 x 32 (tests/test_texture_cases.py asserts them on the oracle alone,
tests/test_gpu_texture_extremes.py asserts the NaN counts again on what the device returned).  No row is CPU-only, and the oracle
renders every row of the issue's list: none was dropped.

Out of scope: the denoisers on these albedo planes, the Sobol sampler, the row-strip driver, maps wider than 2^24 texels (where
(float)width stops being exact), and lens sampling.
"""
import copy
import functools

import numpy as np

from restir_amd.ctypes_structs import LAMBERTIAN, LIGHT
from tests import extreme_cases as xc
from tests.common import get_scene

SIZE, RAGGED, TILE = xc.SIZE, xc.RAGGED, xc.TILE
F32 = np.float32
TALL_BOX, SHORT_BOX = slice(10, 22), slice(22, 34)     # triangles of cornell_textured(): material 4 (every map), material 5 (normal map)
FLOOR_AND_CEILING = (0, 1, 2, 3)
BASE_MAP, METAL_MAP, ROUGH_MAP, NORMAL_MAP, ENV_MAP = 0, 1, 2, 3, 4
ENV_DIST = F32(1e10)                                    # the distance sample_env_nv's caller gives an environment sample: no triangle light has it


def _fresh(kind="cornell_textured"):
    """A copy whose coordinates, material table, material ids, texture list and camera arguments a row may write to."""
    sd = copy.copy(get_scene(kind))
    sd.texcoords = sd.texcoords.copy()
    sd.materials = sd.materials.copy()
    sd.material_ids = sd.material_ids.copy()
    sd.textures = [t.copy() for t in sd.textures]
    sd.camera_args = dict(sd.camera_args)
    return sd


def _coords(fn):
    def edit(sd):
        with np.errstate(all="ignore"):
            sd.texcoords = np.ascontiguousarray(fn(sd.texcoords.astype(F32)), F32)
    return edit


def _on(prims, u, v):
    def edit(sd):
        sd.texcoords[prims, :, 0] = u
        sd.texcoords[prims, :, 1] = v
    return edit


def _one_corner(t):
    return np.repeat(t[:, :1], 3, axis=1)


def _maps(**shapes):
    """The material maps redrawn at other sizes (H, W), from a seeded generator and in the ranges cornell_textured() draws them."""
    def edit(sd):
        rng = np.random.default_rng(11)
        for key, (h, w) in shapes.items():
            if key == "base":
                sd.textures[BASE_MAP] = rng.uniform(0.1, 0.9, (h, w, 3)).astype(F32)
            elif key == "metal":
                sd.textures[METAL_MAP] = np.repeat(rng.uniform(0.0, 1.0, (h, w, 1)), 3, axis=2).astype(F32)
            elif key == "rough":
                sd.textures[ROUGH_MAP] = np.repeat(rng.uniform(0.15, 0.9, (h, w, 1)), 3, axis=2).astype(F32)
            else:
                sd.textures[NORMAL_MAP] = np.concatenate([0.5 + rng.uniform(-0.2, 0.2, (h, w, 2)), np.full((h, w, 1), 1.0)], axis=2).astype(F32)
    return edit


def _blocks(shape, values, block=2):
    """An (H, W, 3) map of blocks of block x block texels that cycle through `values`."""
    y, x = np.indices(shape)
    v = np.asarray(values, F32)[((y // block) + (x // block) * 2 + (y // block) * 3) % len(values)]
    return np.ascontiguousarray(np.repeat(v[..., None], 3, axis=2), F32)


def _texture(tex_id, make):
    def edit(sd):
        sd.textures[tex_id] = np.ascontiguousarray(make(sd.textures[tex_id].copy()), F32)
    return edit


def _base_zero_negative_huge(t):
    t = _blocks(t.shape[:2], [0.0, -1.0, 4.0, 1e30, 0.5], block=1)
    t[5, 7] = np.inf
    return t


def _base_nan_texels(t):
    t[3, 5] = np.nan; t[9, 20, 1] = np.nan; t[12, 0] = np.nan
    return t


def _normal_half(t):
    t[:] = 0.5
    return t


def _normal_inward(t):
    t[..., 2] = 0.2
    return t


def _normal_map_on_flat_faces(sd):
    """Material 5's normal map on floor and ceiling too, through a material of their own (the back wall keeps material 0): their
    |n.y| = 1 takes local_to_world's other tangent."""
    xc._new_material(sd, FLOOR_AND_CEILING, normalMapId=NORMAL_MAP)


def _procedural_everywhere(sd):
    for m in range(len(sd.materials)):
        if sd.materials[m]["type"] != LIGHT:
            sd.materials[m]["baseColorMapId"] = -2
    sd.texcoords = np.ascontiguousarray(sd.texcoords * F32(4000))


def _metal_rough_ids_minus2(sd):
    sd.materials[4]["metallicMapId"] = -2; sd.materials[4]["roughnessMapId"] = -2
    sd.materials[0]["metallicMapId"] = -2; sd.materials[5]["roughnessMapId"] = -2


def _env(make):
    def edit(sd):
        sd.textures[ENV_MAP] = np.ascontiguousarray(make(sd.textures[ENV_MAP].copy()), F32)
    return edit


def _env_of(shape, seed=12):
    """A sky of (H, W) texels with values in [0.2, 1.2)."""
    return lambda _: np.random.default_rng(seed).uniform(0.2, 1.2, shape + (3,)).astype(F32)


def _env_one_texel(_):
    t = np.zeros((3, 5, 3), F32)
    t[1, 3] = (30.0, 25.0, 20.0)
    return t


def _env_dynamic_range(t):
    t[10:12, 20:24] = 1e30; t[12:14, 20:24] = 1e-30; t[14:16] = 0.0
    return t


def _env_with(value):
    def make(t):
        t[9, 30] = value
        return t
    return make


def _env_negative_channel(t):
    t[:16, :, 0] = -t[:16, :, 0]
    return t


def _env_only_light(sd):
    sd.materials[3]["type"] = LAMBERTIAN


def _camera(**args):
    def edit(sd):
        sd.camera_args.update(args)
    return edit


def _bistro_textured(sd):
    v = sd.vertices
    t = np.zeros((v.shape[0], 3, 2), F32)
    t[:, :, 0] = v[:, :, 0] * 0.7 + v[:, :, 2] * 0.3 + 0.13            # cornell_textured()'s projection
    t[:, :, 1] = v[:, :, 1] * 0.6 - v[:, :, 2] * 0.2 - 0.21
    sd.texcoords = np.ascontiguousarray(t)
    count = np.bincount(sd.material_ids, minlength=len(sd.materials)).astype(np.int64)
    count[sd.materials["type"] == LIGHT] = -1
    rng = np.random.default_rng(13)
    sd.textures = [rng.uniform(0.05, 0.95, (16, 32, 3)).astype(F32), rng.uniform(0.2, 1.2, (4, 8, 3)).astype(F32)]
    sd.materials[int(np.argmax(count))]["baseColorMapId"] = 0
    sd.env_map_tex = 1


# name: (scene, edit, what the row drives)
TABLE = {
    # ---- coordinates (maps unchanged)
    "uv_x4000":         ("cornell_textured", _coords(lambda t: t * F32(4000)), "coordinates up to 1e4: past the point where the procedural texture's seed product leaves int"),
    "uv_negative_far":  ("cornell_textured", _coords(lambda t: t - F32(5000)), "negative coordinates with 2^-11 of resolution"),
    "uv_integer":       ("cornell_textured", _coords(np.rint), "every corner at fract = 0"),
    "uv_texel_centres": ("cornell_textured", _coords(lambda t: (np.floor(t * F32(16)) + F32(.5)) / F32(16)), "corners at (k + 1/2) / 16: `fract(fx) > .5f` at equality"),
    "uv_nan_tall_box":  ("cornell_textured", _on(TALL_BOX, np.nan, np.nan), "NaN coordinates on the box with every map: f2i(NaN) = 0, NaN filter weights"),
    "uv_inf_short_box": ("cornell_textured", _on(SHORT_BOX, np.inf, -np.inf), "infinite coordinates under the normal map: fract(inf) is NaN"),
    "uv_1e30":          ("cornell_textured", _coords(lambda t: t * F32(1e30)), "fract(1e30) = 0 and a large-argument reduction in the procedural texture's sin"),
    "uv_degenerate":    ("cornell_textured", _coords(_one_corner), "all three corners of a triangle share one coordinate"),
    # ---- map sizes
    "maps_1x1":         ("cornell_textured", _maps(base=(1, 1), metal=(1, 1), rough=(1, 1), normal=(1, 1)), "every neighbour wraps onto the one texel"),
    "maps_1xN_Nx1":     ("cornell_textured", _maps(base=(1, 7), metal=(7, 1), rough=(1, 1), normal=(2, 2)), "one texel along one axis"),
    "maps_odd":         ("cornell_textured", _maps(base=(3, 5), metal=(5, 3), rough=(7, 11), normal=(37, 53)), "sizes that are no power of two"),
    # ---- texel values
    "metal_map_out_of_range":     ("cornell_textured", _texture(METAL_MAP, lambda t: _blocks(t.shape[:2], [-1.0, 0.0, 1.0, 2.0])), "metallic -1, 0, 1, 2 per pixel: 1 / (2 - metallic) divides by zero in some lanes"),
    "rough_map_zero_and_tiny":    ("cornell_textured", _texture(ROUGH_MAP, lambda t: _blocks(t.shape[:2], [0.0, 1e-6, 1e-3, 1.0, 2.0], block=1)), "alpha 0 and alpha^2 below 2^-60 per pixel: the guarded forms beside NaN weights"),
    "base_map_zero_negative_huge": ("cornell_textured", _texture(BASE_MAP, _base_zero_negative_huge), "base-colour texels 0, -1, 4, 1e30 and one inf"),
    "base_map_nan_texel":         ("cornell_textured", _texture(BASE_MAP, _base_nan_texels), "three NaN texels: every sample that blends one is NaN"),
    "normal_map_half":            ("cornell_textured", _texture(NORMAL_MAP, _normal_half), "normalize(0): a NaN normal on both boxes"),
    "normal_map_inward":          ("cornell_textured", _texture(NORMAL_MAP, _normal_inward), "z = 0.2 < 0.5: normals that point below the surface"),
    "normal_map_on_flat_faces":   ("cornell_textured", _normal_map_on_flat_faces, "|n.y| = 1: the tangent (0, 0, 1) of local_to_world"),
    # ---- map ids
    "procedural_everywhere":      ("cornell_textured", _procedural_everywhere, "the procedural texture on every surface, at uv_x4000's coordinates"),
    "metal_rough_ids_minus2":     ("cornell_textured", _metal_rough_ids_minus2, "metallic / roughness ids of -2 are ignored (check_materials): the material's own numbers"),
    # ---- the environment map
    "env_1x1":           ("cornell_textured", _env(_env_of((1, 1))), "one texel: an alias table of one entry"),
    "env_1x2":           ("cornell_textured", _env(_env_of((1, 2))), "height 1, width 2: the texels face +z and -z"),
    "env_5x3_one_texel": ("cornell_textured", _env(_env_one_texel), "width 5 (pix / width is no shift), one lit texel among black ones"),
    "env_3x7":           ("cornell_textured", _env(_env_of((7, 3))), "width 3, height 7"),
    "env_dynamic_range": ("cornell_textured", _env(_env_dynamic_range), "1e30 beside 1e-30 beside 0 in one alias table"),
    "env_inf_texel":     ("cornell_textured", _env(_env_with(np.inf)), "an infinite texel, which creation takes: the pdf sum is infinite"),
    "env_nan_texel":     ("cornell_textured", _env(_env_with(np.nan)), "a NaN texel at creation: a NaN pdf sum"),
    "env_black":         ("cornell_textured", _env(lambda t: np.zeros_like(t)), "a black map at creation: pdf sum 0"),
    "env_negative_channel": ("cornell_textured", _env(_env_negative_channel), "a negative red channel in the upper half"),
    "env_only_light":    ("cornell_textured", _env_only_light, "material 3 Lambertian: the light sampler holds the map's entry alone"),
    "env_rows_64x1":     ("cornell_textured", _env(_env_of((1, 64))), "width 64, height 1"),
    "env_cols_1x64":     ("cornell_textured", _env(_env_of((64, 1))), "width 1, height 64"),
    # ---- the camera into the poles and along the axes (scene unchanged)
    "look_up":           ("cornell_textured", _camera(rotation=(-90.0, 90.0, 0.0)), "straight up: to_plane at the pole y = 1"),
    "look_down":         ("cornell_textured", _camera(rotation=(-90.0, -90.0, 0.0)), "straight down: the pole y = -1"),
    "look_px":           ("cornell_textured", _camera(rotation=(0.0, 0.0, 0.0)), "view (1, 0, 0) exactly"),
    "look_nx":           ("cornell_textured", _camera(rotation=(180.0, 0.0, 0.0)), "view (-1, ..): the seam of atan2(z, x)"),
    "look_pz":           ("cornell_textured", _camera(rotation=(90.0, 0.0, 0.0)), "view (0, 0, 1)"),
    "look_nz":           ("cornell_textured", _camera(position=(0.0, 1.0, 0.9)), "the box's own view (0, 0, -1), from inside it: every pixel hits"),
    # ---- a bigger tree and many lights
    "bistro_textured":   ("bistro:0.12", _bistro_textured, "TEX / ENV kernels over 339 488 triangles and a light table in global memory"),
}
NAMES = list(TABLE)
CORNELL = [n for n in NAMES if TABLE[n][0] == "cornell_textured"]
COORDINATES = [n for n in NAMES if n.startswith("uv_")]
TEXELS = ["metal_map_out_of_range", "rough_map_zero_and_tiny", "base_map_zero_negative_huge", "base_map_nan_texel", "normal_map_half", "normal_map_inward", "normal_map_on_flat_faces"]
PARTIAL = COORDINATES + TEXELS                       # the rows that run again at RAGGED
CAMERA = [n for n in NAMES if n.startswith("look_")]  # rows that change the camera only: they share the base rs_scene
POLES = ("look_up", "look_down")
# rows with surface pixels under an environment map (the other look_* rows see no surface: every pixel is a miss, no reservoir is live)
ENVIRONMENT = [n for n in NAMES if n.startswith("env_")] + ["look_nz", "bistro_textured"]
# environment rows that cannot leave a live reservoir on the environment entry: with a black map the entry's power and every pdf are 0;
# with an infinite texel the total light power is infinite, 1 / sum = 0 and every pdf of every light is 0; with a NaN texel they are NaN;
# a map one texel wide has every texel at u = 1/2, to_sphere's direction (-sin(pi v), cos(pi v), 1e-8 ..): the environment shines from
# -x alone, where the box's left wall stands (its candidates are drawn and their shadow rays walked all the same)
NO_LIVE_ENV = ("env_black", "env_inf_texel", "env_nan_texel", "env_1x1", "env_cols_1x64")
# rows whose extreme sits on one box only, so that a 32 x 8 tile holds its pixels beside Lambertian ones: name -> the extreme materials
MIXED = {"uv_nan_tall_box": (4,), "uv_inf_short_box": (5,), "metal_map_out_of_range": (4,), "rough_map_zero_and_tiny": (4,), "normal_map_half": (4, 5), "normal_map_inward": (4, 5)}
# environment rows whose map keeps the base scene's size: name -> does rs_scene_set_texture accept the map? (it refuses a pdf sum that
# is not finite and positive; rs_scene_build_textured takes such a map at creation)
ENV_SAME_SIZE = {"env_dynamic_range": True, "env_negative_channel": True, "env_inf_texel": False, "env_nan_texel": False, "env_black": False}
BASE = {"cornell_textured": "base", "bistro:0.12": "bistro_base"}


@functools.lru_cache(maxsize=None)
def scene(name):
    """The edited scene of a row (built once; nobody writes to it).  "base" / "bistro_base": the scenes as generated."""
    if name in BASE.values():
        return _fresh({v: k for k, v in BASE.items()}[name])
    kind, edit, _ = TABLE[name]
    sd = _fresh(kind)
    edit(sd)
    return sd


def stages_of(name):
    """The many-lights row runs ReSTIR direct only."""
    return xc.STAGES if name in CORNELL else ("direct3", "direct0")


@functools.lru_cache(maxsize=None)
def _oracle_outputs(name, size, stages):
    assert xc._correctly_rounded, "oracle_outputs: inside extreme_cases.correctly_rounded_libm() only"
    return xc.run(xc.OracleBackend(scene(name), size), stages)


def oracle_outputs(name, size=SIZE, stages=None):
    """The oracle's outputs of `stages` (default: all the row runs), computed once and shared: nobody writes to them."""
    return _oracle_outputs(name, tuple(size), tuple(stages or stages_of(name)))


def base_outputs(name):
    """The ReSTIR-direct outputs of the scene the row edits, as generated."""
    kind = TABLE[name][0]
    return oracle_outputs(BASE[kind], SIZE, ("direct3",))


# ---- figures ------------------------------------------------------------------------------------------------------------------------
def mapped_materials(sd):
    m = sd.materials
    return set(np.nonzero((m["baseColorMapId"] != -1) | (m["metallicMapId"] > -1) | (m["roughnessMapId"] > -1) | (m["normalMapId"] != -1))[0].tolist())


def _differing(a, b):
    from tests.scene_edits import differing
    return differing(a, b)


def figures(name, o, base):
    """What EXPECT states of a row's oracle outputs: miss pixels and pixels whose hit carries a mapped material (the G-buffer's id plane
    holds the MATERIAL id: -1 a miss, -2 a light); live reservoirs after the last spatiotemporal frame and those among them whose sample is
    an environment sample (its distance is 1e10, which no triangle light gives); albedo pixels and last-frame reservoirs that differ from
    the base scene's; every output that holds a NaN or an infinity, with its count."""
    mat = o["direct3/gbuffer/prim_id"].reshape(-1)
    res = o["direct3/f2/res"]
    return dict(miss=int(np.count_nonzero(mat == -1)), mapped=int(np.count_nonzero(np.isin(mat, list(mapped_materials(scene(name)))))),
                live=xc.live(res), env_live=int(np.count_nonzero((res["weight"] > 0) & (res["dist"] == ENV_DIST))),
                albedo_differs=_differing(o["direct3/gbuffer/albedo"], base["direct3/gbuffer/albedo"]),
                res_differs=_differing(res, base["direct3/f2/res"]), nan=xc.nan_counts(o), inf=xc.inf_counts(o))


def mixed_tiles(name, size=SIZE):
    """(tiles of 32 x 8 pixels that hold a pixel of the row's extreme materials, those among them that also hold a Lambertian pixel of another
    material), from the oracle's material-id plane: the rule of extreme_cases.mixed_tiles."""
    sd = scene(name)
    w, h = size
    mat = oracle_outputs(name, size, ("direct3", "direct0") if size != SIZE else None)["direct3/gbuffer/prim_id"].reshape(h, w)
    extreme = np.isin(mat, list(MIXED[name]))
    ordinary = (mat >= 0) & ~extreme & (sd.materials["type"][np.maximum(mat, 0)] == LAMBERTIAN)
    tiles = both = 0
    for y in range(0, h, TILE[1]):
        for x in range(0, w, TILE[0]):
            e, o = extreme[y:y + TILE[1], x:x + TILE[0]], ordinary[y:y + TILE[1], x:x + TILE[0]]
            tiles += bool(e.any()); both += bool(e.any() and o.any())
    return tiles, both


EXPECT = {
    "uv_x4000":                    {'miss': 861, 'mapped': 555, 'live': 488, 'env_live': 307, 'albedo_differs': 507, 'res_differs': 117},
    "uv_negative_far":             {'miss': 861, 'mapped': 555, 'live': 488, 'env_live': 299, 'albedo_differs': 507, 'res_differs': 109},
    "uv_integer":                  {'miss': 861, 'mapped': 555, 'live': 489, 'env_live': 308, 'albedo_differs': 507, 'res_differs': 118},
    "uv_texel_centres":            {'miss': 861, 'mapped': 555, 'live': 485, 'env_live': 297, 'albedo_differs': 507, 'res_differs': 113},
    "uv_nan_tall_box":             {'miss': 861, 'mapped': 555, 'live': 435, 'env_live': 255, 'albedo_differs': 66, 'res_differs': 65, 'nan': {'direct3/f0/image': 198, 'direct3/f1/image': 198, 'direct3/f2/image': 198, 'direct3/gbuffer/albedo': 198, 'direct3/gbuffer/normal': 198, 'direct0/f0/image': 198, 'direct0/f1/image': 198, 'ptd/image': 69}},
    "uv_inf_short_box":            {'miss': 861, 'mapped': 555, 'live': 442, 'env_live': 255, 'albedo_differs': 0, 'res_differs': 54, 'nan': {'direct3/gbuffer/normal': 144}},
    "uv_1e30":                     {'miss': 861, 'mapped': 555, 'live': 491, 'env_live': 307, 'albedo_differs': 507, 'res_differs': 118},
    "uv_degenerate":               {'miss': 861, 'mapped': 555, 'live': 489, 'env_live': 300, 'albedo_differs': 507, 'res_differs': 120},
    "maps_1x1":                    {'miss': 861, 'mapped': 555, 'live': 490, 'env_live': 297, 'albedo_differs': 381, 'res_differs': 118},
    "maps_1xN_Nx1":                {'miss': 861, 'mapped': 555, 'live': 484, 'env_live': 301, 'albedo_differs': 381, 'res_differs': 112},
    "maps_odd":                    {'miss': 861, 'mapped': 555, 'live': 489, 'env_live': 302, 'albedo_differs': 381, 'res_differs': 116},
    "metal_map_out_of_range":      {'miss': 861, 'mapped': 555, 'live': 487, 'env_live': 298, 'albedo_differs': 0, 'res_differs': 59},
    "rough_map_zero_and_tiny":     {'miss': 861, 'mapped': 555, 'live': 486, 'env_live': 298, 'albedo_differs': 0, 'res_differs': 57},
    "base_map_zero_negative_huge": {'miss': 861, 'mapped': 555, 'live': 488, 'env_live': 299, 'albedo_differs': 381, 'res_differs': 0, 'nan': {'ptd/image': 3}, 'inf': {'ptd/image': 45, 'gi/f0/res.weight': 4, 'gi/f1/res.weight': 8, 'gi/f2/res.weight': 9}},
    "base_map_nan_texel":          {'miss': 861, 'mapped': 555, 'live': 488, 'env_live': 299, 'albedo_differs': 12, 'res_differs': 0, 'nan': {'direct3/f0/image': 34, 'direct3/f1/image': 34, 'direct3/f2/image': 34, 'direct3/gbuffer/albedo': 34, 'direct0/f0/image': 34, 'direct0/f1/image': 34, 'ptd/image': 13}},
    "normal_map_half":             {'miss': 861, 'mapped': 555, 'live': 389, 'env_live': 211, 'albedo_differs': 0, 'res_differs': 119, 'nan': {'direct3/gbuffer/normal': 342, 'ptd/image': 69}},
    "normal_map_inward":           {'miss': 861, 'mapped': 555, 'live': 484, 'env_live': 298, 'albedo_differs': 0, 'res_differs': 118},
    "normal_map_on_flat_faces":    {'miss': 861, 'mapped': 555, 'live': 496, 'env_live': 308, 'albedo_differs': 0, 'res_differs': 163},
    "procedural_everywhere":       {'miss': 861, 'mapped': 671, 'live': 488, 'env_live': 307, 'albedo_differs': 671, 'res_differs': 117},
    "metal_rough_ids_minus2":      {'miss': 861, 'mapped': 555, 'live': 486, 'env_live': 300, 'albedo_differs': 0, 'res_differs': 59},
    "env_1x1":                     {'miss': 861, 'mapped': 555, 'live': 419, 'env_live': 0, 'albedo_differs': 861, 'res_differs': 654},
    "env_1x2":                     {'miss': 861, 'mapped': 555, 'live': 617, 'env_live': 302, 'albedo_differs': 861, 'res_differs': 654},
    "env_5x3_one_texel":           {'miss': 861, 'mapped': 555, 'live': 404, 'env_live': 13, 'albedo_differs': 861, 'res_differs': 652},
    "env_3x7":                     {'miss': 861, 'mapped': 555, 'live': 481, 'env_live': 179, 'albedo_differs': 861, 'res_differs': 655},
    "env_dynamic_range":           {'miss': 861, 'mapped': 555, 'live': 258, 'env_live': 258, 'albedo_differs': 245, 'res_differs': 655},
    "env_inf_texel":               {'miss': 861, 'mapped': 555, 'live': 0, 'env_live': 0, 'albedo_differs': 0, 'res_differs': 655},
    "env_nan_texel":               {'miss': 861, 'mapped': 555, 'live': 0, 'env_live': 0, 'albedo_differs': 0, 'res_differs': 655},
    "env_black":                   {'miss': 861, 'mapped': 555, 'live': 472, 'env_live': 0, 'albedo_differs': 861, 'res_differs': 654},
    "env_negative_channel":        {'miss': 861, 'mapped': 555, 'live': 504, 'env_live': 260, 'albedo_differs': 431, 'res_differs': 603},
    "env_only_light":              {'miss': 861, 'mapped': 555, 'live': 404, 'env_live': 404, 'albedo_differs': 0, 'res_differs': 510},
    "env_rows_64x1":               {'miss': 861, 'mapped': 555, 'live': 549, 'env_live': 325, 'albedo_differs': 861, 'res_differs': 654},
    "env_cols_1x64":               {'miss': 861, 'mapped': 555, 'live': 384, 'env_live': 0, 'albedo_differs': 861, 'res_differs': 654},
    "look_up":                     {'miss': 1536, 'mapped': 0, 'live': 0, 'env_live': 0, 'albedo_differs': 1536, 'res_differs': 655},
    "look_down":                   {'miss': 1536, 'mapped': 0, 'live': 0, 'env_live': 0, 'albedo_differs': 1536, 'res_differs': 655},
    "look_px":                     {'miss': 1536, 'mapped': 0, 'live': 0, 'env_live': 0, 'albedo_differs': 1536, 'res_differs': 655},
    "look_nx":                     {'miss': 1536, 'mapped': 0, 'live': 0, 'env_live': 0, 'albedo_differs': 1536, 'res_differs': 655},
    "look_pz":                     {'miss': 1536, 'mapped': 0, 'live': 0, 'env_live': 0, 'albedo_differs': 1536, 'res_differs': 655},
    "look_nz":                     {'miss': 0, 'mapped': 1322, 'live': 1086, 'env_live': 445, 'albedo_differs': 1536, 'res_differs': 1502},
    "bistro_textured":             {'miss': 124, 'mapped': 782, 'live': 1368, 'env_live': 108, 'albedo_differs': 906, 'res_differs': 1409},
}


def expected(name):
    return dict(dict(nan={}, inf={}), **EXPECT[name])
