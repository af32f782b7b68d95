"""Material and light parameters at their extremes: a table of named scene edits, the oracle's outputs for each and the rule by which
the library's outputs are held to them.

Every other parity module renders tame numbers (roughness 0.25 - 0.4, metallic 0.5 - 0.9, ior 1.5, radiance around 10, base colours
inside (0, 1)).  Two parts of the library act only outside that range: the guarded short forms of restir_amd/csrc/rs_exact.h, which run the
compiler's operator for a whole wave as soon as one lane holds an operand outside [2^-60, 2^60), and the filters that drop a sample whose
weight is NaN, infinite or not positive (k_ris, resv_invalid, ind_invalid, the GLM-shaped gmin / gmax).  A case is a name and a function
that edits a fresh get_scene("cornell") -- its material table and, where needed, appended triangles -- or, for the many-lights row, the
emissive materials of get_scene("bistro:0.12").  No scene generator changes.

`oracle_outputs(name, size)` runs the CPU oracle (inside correctly_rounded_libm(): cos / sin / atan2 correctly rounded, libm mode 1) through every entry point the GPU
module drives and returns its outputs under flat keys ("direct3/f2/image", "pt4/rays", "gi/f1/res", ...); it is computed once per case
and size and shared.  `compare(oracle, device)` is the comparison rule; `EXPECT[name]` holds the figures that make a case non-vacuous
(tests/test_extreme_cases.py asserts them on the oracle alone, tests/test_gpu_parameter_extremes.py asserts the NaN counts again on
what the device returned).
"""
import contextlib
import functools

import numpy as np

from oracle import binding as ob
from restir_amd.ctypes_structs import DIELECTRIC, LAMBERTIAN, LIGHT, METALLIC_WORKFLOW
from tests.common import OracleRenderer, get_scene

SIZE = (48, 32)                    # 2 x 4 blocks of 32 x 8 pixels, 24 waves
RAGGED = (97, 61)                  # the mixed cases again: partial tiles that hold both kinds of pixel
TILE = (32, 8)
WALLS = (0, 1, 2)                  # cornell_box(): white (floor, ceiling, back wall, both boxes), red, green; 3 is the light
BACK_WALL = (4, 5)                 # triangle ids of cornell_box(), in the order it adds them
LEFT_WALL = (6, 7)
BOXES = tuple(range(10, 34))
F32 = np.float32


def _set(sd, ids, **fields):
    for m in ids:
        for k, v in fields.items():
            sd.materials[m][k] = v


def _walls(**fields):
    def edit(sd):
        _set(sd, WALLS, **fields)
        return set(WALLS)
    return edit


def _metal_walls(roughness, metallic):
    return _walls(type=METALLIC_WORKFLOW, roughness=roughness, metallic=metallic)


def _light(rgb):
    def edit(sd):
        sd.materials[3]["baseColor"] = rgb
        return set()
    return edit


def _new_material(sd, prims, **fields):
    """One more material, a copy of the white Lambertian one with `fields` set, on the triangles `prims`."""
    sd.materials = np.concatenate([sd.materials, sd.materials[:1]])
    m = len(sd.materials) - 1
    _set(sd, [m], **fields)
    sd.material_ids = sd.material_ids.copy()
    sd.material_ids[list(prims)] = m
    return m


def _only(prims, **fields):
    """The mixed form: only `prims` carry the extreme material, everything else stays Lambertian."""
    def edit(sd):
        return {_new_material(sd, prims, **fields)}
    return edit


def _dielectric_back_wall(ior):
    return _only(BACK_WALL, type=DIELECTRIC, ior=ior, baseColor=(0.9, 0.95, 1.0))


def _append(sd, verts, mat):
    verts = np.asarray(verts, F32).reshape(-1, 3, 3)
    k = len(verts)
    sd.vertices = np.ascontiguousarray(np.concatenate([sd.vertices, verts]))
    sd.normals = np.ascontiguousarray(np.concatenate([sd.normals, np.tile(np.array([0, -1, 0], F32), (k, 3, 1))]))
    sd.texcoords = np.ascontiguousarray(np.concatenate([sd.texcoords, np.zeros((k, 3, 2), F32)]))
    sd.material_ids = np.concatenate([sd.material_ids, np.full(k, mat, np.int32)])


def _zero_area_lights(sd):
    """Two more emissive triangles without area: one a point, one three collinear vertices.  Their power is 0."""
    p = (0.3, 1.5, 0.2)
    _append(sd, [[p, p, p], [(-0.5, 1.6, 0.1), (-0.3, 1.6, 0.1), (-0.1, 1.6, 0.1)]], 3)
    return set()


def _quad_down(cx, cz, h=0.1):
    a, b, c, d = (cx - h, 1.98, cz - h), (cx + h, 1.98, cz - h), (cx + h, 1.98, cz + h), (cx - h, 1.98, cz + h)
    return [[a, b, c], [a, c, d]]


def _dark_and_huge_lights(sd):
    """Two more ceiling lights beside the ordinary one: radiance 0 and radiance 1e30."""
    sd.materials = np.concatenate([sd.materials, sd.materials[3:4], sd.materials[3:4]])
    sd.materials[4]["baseColor"] = (0.0, 0.0, 0.0)
    sd.materials[5]["baseColor"] = (1e30, 1e30, 1e30)
    _append(sd, _quad_down(-0.6, 0.5), 4)
    _append(sd, _quad_down(0.6, -0.5), 5)
    return set()


def _tiny_bright_light(sd):
    """One more emissive triangle, right-angled with legs of 1e-9 just below the ceiling light, of radiance 1e19."""
    sd.materials = np.concatenate([sd.materials, sd.materials[3:4]])
    sd.materials[4]["baseColor"] = (1e19, 1e19, 1e19)
    _append(sd, [[(0.0, 1.9, 0.0), (1e-9, 1.9, 0.0), (0.0, 1.9, 1e-9)]], 4)
    return set()


def _bistro_spread(sd):
    """Every emissive material of the many-lights scene scaled by 10^e, e uniform in [-30, 25] from a seeded generator: radiances
    from 1e-30 to 1e25 and a few above, in a light table that k_ris reads from global memory."""
    rng = np.random.default_rng(20)
    lamps = np.nonzero(sd.materials["type"] == LIGHT)[0]
    e = rng.uniform(-30.0, 25.0, len(lamps))
    sd.materials["baseColor"][lamps] = (sd.materials["baseColor"][lamps].astype(np.float64) * (10.0 ** e)[:, None] / 50.0).astype(F32)
    return set()


ABOVE_ONE, BELOW_ONE = np.nextafter(F32(1), F32(2)), np.nextafter(F32(1), F32(0))

# name: (scene, edit, what the case drives)
TABLE = {
    # ---- the walls and boxes rewritten (materials 0, 1, 2)
    "mirror_metal":      ("cornell", _metal_walls(0.0, 1.0), "gtr2 = 0 / 0 at every mirror direction, every other weight 0: all filtered"),
    "rough0_metal_half": ("cornell", _metal_walls(0.0, 0.5), "alpha = 0 beside a live diffuse lobe: NaN weights filtered among finite ones"),
    "rough1e-6":         ("cornell", _metal_walls(1e-6, 0.0), "gtr2's numerator alpha^2 = 1e-24 < 2^-60: bsdf_div on the compiler's operator in every wave"),
    "rough1e-3_metal_half": ("cornell", _metal_walls(1e-3, 0.5), "alpha^2 = 1e-12, inside the guarded range but far from the tame one"),
    "rough1_metal1":     ("cornell", _metal_walls(1.0, 1.0), "the upper ends of both ranges"),
    "rough2_metal2":     ("cornell", _metal_walls(2.0, 2.0), "past the ends: 1 / (2 - metallic) divides by zero, mix() extrapolates"),
    "metallic0":         ("cornell", _metal_walls(0.3, 0.0), "1 / (2 - metallic) = 0.5"),
    "metallic1":         ("cornell", _metal_walls(0.3, 1.0), "1 / (2 - metallic) = 1: r.z > 1 never picks the diffuse lobe"),
    "base_zero":         ("cornell", _walls(baseColor=(0.0, 0.0, 0.0)), "zero albedo and zero throughput after the first bounce (k_ris shades with base colour 1, restir.cu:141)"),
    "base_above_one":    ("cornell", _walls(baseColor=(4.0, 4.0, 4.0)), "throughput that grows with every bounce"),
    "base_zero_channel": ("cornell", _walls(baseColor=(0.8, 0.0, 0.3)), "one channel of albedo and throughput zero"),
    # ---- the one light's radiance (material 3)
    "light_1e25":        ("cornell", _light((1e25, 1e25, 1e25)), "radiance and power above 2^60"),
    "light_3e38":        ("cornell", _light((3e38, 3e38, 3e38)), "the power sum overflows: 1 / sum = 0, every pdf 0"),
    "light_1e-30":       ("cornell", _light((1e-30, 1e-30, 1e-30)), "radiance below 2^-60"),
    "light_denormal":    ("cornell", _light((1e-42, 1e-42, 1e-42)), "a denormal radiance"),
    "light_zero":        ("cornell", _light((0.0, 0.0, 0.0)), "power 0: 1 / sum is infinite, prob NaN"),
    "light_negative":    ("cornell", _light((-1.0, 2.0, 3.0)), "one negative channel: gmax / gmin and the sign tests of the filters"),
    # ---- a wall as a dielectric
    "ior_1":             ("cornell", _dielectric_back_wall(1.0), "no refraction"),
    "ior_half":          ("cornell", _dielectric_back_wall(0.5), "ior below 1"),
    "ior_zero":          ("cornell", _dielectric_back_wall(0.0), "division by ior 0"),
    "ior_1e4":           ("cornell", _dielectric_back_wall(1e4), "total internal reflection from inside at every angle"),
    "ior_negative":      ("cornell", _dielectric_back_wall(-1.5), "negative ior"),
    "ior_above_one":     ("cornell", _dielectric_back_wall(ABOVE_ONE), "nextafter(1, 2): Fresnel terms that cancel to the last bit"),
    "ior_below_one":     ("cornell", _dielectric_back_wall(BELOW_ONE), "nextafter(1, 0)"),
    # ---- more lights
    "zero_area_lights":  ("cornell", _zero_area_lights, "lights of area 0: normalize(0), power 0 in the alias table"),
    "dark_and_huge_lights": ("cornell", _dark_and_huge_lights, "powers 0, ordinary and 1e30 in one table"),
    "tiny_1e19_light":   ("cornell", _tiny_bright_light, "an emitter of radiance 1e19 and area 5e-19 with twice the ordinary light's power: two of three candidates draw "
                          "it, so in every wave of k_ris lanes whose g and pdf lie above 2^60 sit beside lanes inside the guarded range (its weight is "
                          "area-proportional, 1e-17 of the ordinary light's: it never wins, it must only not disturb its wave)"),
    # ---- mixed: one part of the scene extreme, the rest Lambertian, so that tiles and waves hold both kinds of pixel
    "mixed_rough1e-6_boxes": ("cornell", _only(BOXES, type=METALLIC_WORKFLOW, roughness=1e-6, metallic=0.0), "lanes with alpha^2 below 2^-60 beside Lambertian lanes, which never call bsdf_div"),
    "mixed_base_zero_back_wall": ("cornell", _only(BACK_WALL, baseColor=(0.0, 0.0, 0.0)), "zero throughput beside ordinary throughput (reaches no guarded form: the row the other two mixed rows are read against)"),
    "mixed_mirror_left_wall_boxes": ("cornell", _only(LEFT_WALL + BOXES, type=METALLIC_WORKFLOW, roughness=0.0, metallic=1.0), "gtr2 = 0 / 0 and NaN weights in some lanes of a wave, finite ones in the others"),
    # ---- many lights
    "bistro_spread":     ("bistro:0.12", _bistro_spread, "radiances 1e-30 .. 1e25 in the global-memory light table"),
}
NAMES = list(TABLE)
CORNELL = [n for n in NAMES if TABLE[n][0] == "cornell"]
MIXED = [n for n in NAMES if n.startswith("mixed_")]
PARTIAL = MIXED + ["tiny_1e19_light"]          # the cases that run again at RAGGED: lanes of one wave go different ways


@functools.lru_cache(maxsize=None)
def _scene(name):
    kind, edit, _ = TABLE[name]
    sd = get_scene(kind)
    sd.materials = sd.materials.copy()
    extreme = edit(sd)
    return sd, frozenset(extreme)


def scene(name):
    """The edited scene of a case (built once; nobody writes to it)."""
    return _scene(name)[0]


def extreme_materials(name):
    return _scene(name)[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# the call sequence, once for the oracle and once for the library (tests/test_gpu_parameter_extremes.py passes its own back end)
# ---------------------------------------------------------------------------------------------------------------------------------
PT_LOOPER = {1: 2, 4: 0}             # at these the negative light's pathTrace leaves one +inf element in the indirect plane (at 1, 3, 4, 5 none)
GBUFFER_PLANES = ("prim_id", "albedo", "normal", "depth", "motion")
STAGES = ("direct3", "direct0", "ptd", "pt1", "pt4", "pti3", "gi")


class OracleBackend:
    """The oracle behind the interface `run` drives; the GPU module has the same for the library."""

    def __init__(self, sd, size):
        self.sd, self.size, self.n = sd, size, size[0] * size[1]
        self.shared = OracleRenderer(sd, *size).scene

    def renderer(self):
        return OracleRenderer(self.sd, *self.size, scene=self.shared)

    def last(self, r):
        return r.restir.last.copy()

    def gbuffer(self, r):
        g = r.gbuf
        f = g.frame_idx ^ 1                                  # the planes rendered last: update() flipped the index
        return dict(prim_id=g.prim_id[f].copy(), albedo=g.albedo.copy(), normal=g.normal[f].copy(), depth=g.depth[f].copy(), motion=g.motion.copy())

    def path_trace(self, r, looper, depth):
        d, i = np.zeros((self.n, 3), F32), np.zeros((self.n, 3), F32)
        rays = ob.path_trace(r.scene, r.cam, d, i, 0, looper, depth)
        return d, i, rays

    def pt_indirect(self, r, looper, depth):
        i = np.zeros((self.n, 3), F32)
        rays = ob.pt_indirect(r.scene, r.cam, i, 0, looper, depth)
        return i, rays

    def gi_frames(self, r, frames, depth):
        img = np.zeros((self.n, 3), F32)
        for f in range(frames):
            r.gbuf.render(r.scene, r.cam)
            rays = r.restir.indirect(r.scene, r.cam, r.gbuf, img, 0, f, 1, depth)
            r.gbuf.update(r.cam)
            yield img.copy(), rays, r.restir.ind_last.copy()


def run(be, stages=STAGES):
    """Every entry point on one case: flat keys -> arrays / ray counts."""
    out = {}
    for stage, reuse, frames in (("direct3", 3, 3), ("direct0", 0, 2)):
        if stage not in stages:
            continue
        r = be.renderer()
        for f in range(frames):
            out["%s/f%d/image" % (stage, f)] = np.array(r.frame(reuse))
            out["%s/f%d/rays" % (stage, f)] = int(r.rays)
            out["%s/f%d/res" % (stage, f)] = be.last(r)
        if stage == "direct3":
            for k, v in be.gbuffer(r).items():
                out["direct3/gbuffer/" + k] = v
    if "ptd" in stages:                                      # the PT-direct baseline: its own eval_bsdf / pdf quotient
        r = be.renderer()
        out["ptd/image"] = np.array(r.frame(0, use_reservoir=False))
        out["ptd/rays"] = int(r.rays)
    for stage, depth in (("pt1", 1), ("pt4", 4)):
        if stage in stages:
            d, i, rays = be.path_trace(be.renderer(), PT_LOOPER[depth], depth)
            out[stage + "/direct"], out[stage + "/indirect"], out[stage + "/rays"] = d, i, int(rays)
    if "pti3" in stages:
        i, rays = be.pt_indirect(be.renderer(), 5, 3)
        out["pti3/indirect"], out["pti3/rays"] = i, int(rays)
    if "gi" in stages:
        for f, (img, rays, res) in enumerate(be.gi_frames(be.renderer(), 3, 3)):
            out["gi/f%d/image" % f], out["gi/f%d/rays" % f], out["gi/f%d/res" % f] = img, int(rays), res
    return out


def stages_of(name):
    """The many-lights case runs ReSTIR direct only."""
    return ("direct3", "direct0") if TABLE[name][0] != "cornell" else STAGES


_correctly_rounded = False


@contextlib.contextmanager
def correctly_rounded_libm():
    """The oracle's cos / sin / atan2 correctly rounded (libm mode 1), as the device evaluates them, for the time of the block: the
    fixtures of both test modules are this."""
    global _correctly_rounded
    ob.set_libm_mode(1); _correctly_rounded = True
    try:
        yield
    finally:
        ob.set_libm_mode(0); _correctly_rounded = False


@functools.lru_cache(maxsize=None)
def _oracle_outputs(name, size, stages):
    assert _correctly_rounded, "oracle_outputs: inside correctly_rounded_libm() only (the callers' fixture owns the oracle's libm mode)"
    return run(OracleBackend(scene(name), size), stages)


def oracle_outputs(name, size=SIZE, stages=None):
    """The oracle's outputs of `stages` (default: all the case runs), computed once and shared: nobody writes to them."""
    return _oracle_outputs(name, tuple(size), tuple(stages or stages_of(name)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparison rule
# ---------------------------------------------------------------------------------------------------------------------------------
def same_bits_or_nan(a, b, where=""):
    """a: the oracle's array, b: the library's.  Every element bit for bit -- except where the oracle holds a NaN: there the library
    must hold a NaN too, of any sign and payload (those come from the unit that produced it: x86 gives 0xFFC00000 for 0 / 0, the device
    0x7FC00000, and the reference defines neither).  Returns the number of NaN elements."""
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (where, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype != np.float32:
        assert np.array_equal(a, b), (where, np.nonzero(a.reshape(-1) != b.reshape(-1))[0][:8])
        return 0
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), (where, "NaN in other elements", int(na.sum()), int(nb.sum()), np.nonzero((na != nb).reshape(-1))[0][:8])
    ne = (a.view(np.uint32) != b.view(np.uint32)) & ~na
    assert not ne.any(), (where, "bits differ", int(ne.sum()), np.nonzero(ne.reshape(-1))[0][:8], a[ne][:4], b[ne][:4])
    return int(na.sum())


def fields(v):
    """A reservoir array as (suffix, plain array) pairs, anything else as itself."""
    if isinstance(v, np.ndarray) and v.dtype.names:
        return [("." + k, v[k]) for k in v.dtype.names]
    return [("", v)]


def compare(oracle, device, where=""):
    """Every key of `oracle` in `device` by same_bits_or_nan (ray counts by ==); returns {key: NaN count} of the keys that hold any."""
    nans = {}
    assert set(oracle) == set(device), set(oracle) ^ set(device)
    for key, a in oracle.items():
        if isinstance(a, int):
            assert a == device[key], (where, key, a, device[key])
            continue
        for (suffix, x), (_, y) in zip(fields(a), fields(device[key])):
            n = same_bits_or_nan(x, y, (where, key + suffix))
            if n:
                nans[key + suffix] = n
    return nans


def nan_counts(outputs):
    """{key: NaN count} as `compare` returns it, from one side alone."""
    return compare(outputs, outputs)


def inf_counts(outputs):
    out = {}
    for key, a in outputs.items():
        if isinstance(a, int):
            continue
        for suffix, x in fields(a):
            if x.dtype == np.float32 and np.isinf(x).any():
                out[key + suffix] = int(np.isinf(x).sum())
    return out


def live(res):
    """Reservoirs whose weight W is positive."""
    return int(np.count_nonzero(res["weight"] > 0))


def black(image):
    return int(np.count_nonzero(~image.any(axis=1)))


def image_range(image):
    """Where the largest finite value of an image lies: "above" 2^60, "below" 2^-60, "denormal", "zero" or "tame"."""
    v = image[np.isfinite(image)]
    m = float(v.max()) if v.size else 0.0
    if m > 2.0 ** 60:
        return "above"
    if m <= 0.0:
        return "zero"
    if m < 2.0 ** -126:
        return "denormal"
    return "below" if m < 2.0 ** -60 else "tame"


def figures(o):
    """The figures of one case's oracle outputs that EXPECT states: live reservoirs after the last frame of the spatiotemporal,
    the RIS-only and the ReSTIR-GI sequence, black pixels, range and negative elements of the last spatiotemporal frame, RIS-only
    reservoirs that hold a radiance above 2^60, ray count and lit pixels of pathTrace at depth 4, and every key that holds NaN or infinity with its count."""
    f = dict(live=live(o["direct3/f2/res"]), live0=live(o["direct0/f1/res"]), black=black(o["direct3/f2/image"]),
             range=image_range(o["direct3/f2/image"]), negative=int(np.count_nonzero(o["direct3/f2/image"] < 0)),
             huge_li=int(np.count_nonzero(o["direct0/f1/res"]["Li"].max(axis=1) > 2.0 ** 60)), nan=nan_counts(o), inf=inf_counts(o))
    if "gi/f2/res" in o:
        f.update(gi_live=live(o["gi/f2/res"]), pt4_rays=o["pt4/rays"], pt4_lit=int(np.count_nonzero(o["pt4/indirect"].any(axis=1))))
    return f


def mixed_tiles(name, size):
    """(tiles of 32 x 8 pixels that hold a pixel of an extreme material, those among them that also hold a Lambertian one, waves of
    64 consecutive lanes of such a block -- two rows of it -- that hold both, runs of 64 consecutive pixel indices that hold both),
    from the oracle's primitive-id plane.  That plane
    holds the MATERIAL id of the hit (the reference's G-buffer pass writes it there, src/gbuffer.cu:28-42 as restated by
    orc_gbuffer_render; -1 a miss, -2 a light), so the mapping to materials is the identity."""
    sd = scene(name)
    w, h = size
    mat = oracle_outputs(name, size, ("direct3", "direct0"))["direct3/gbuffer/prim_id"].reshape(h, w)
    assert mat.max() < len(sd.materials)
    extreme = np.isin(mat, list(extreme_materials(name)))
    ordinary = (mat >= 0) & ~extreme & (sd.materials["type"][np.maximum(mat, 0)] == LAMBERTIAN)
    tiles = both = waves = 0
    for y in range(0, h, TILE[1]):
        for x in range(0, w, TILE[0]):
            e, o = extreme[y:y + TILE[1], x:x + TILE[0]], ordinary[y:y + TILE[1], x:x + TILE[0]]
            tiles += bool(e.any()); both += bool(e.any() and o.any())
            waves += sum(bool(e[r:r + 2].any() and o[r:r + 2].any()) for r in range(0, TILE[1], 2))
    e, o = extreme.reshape(-1), ordinary.reshape(-1)
    linear = sum(bool(e[i:i + 64].any() and o[i:i + 64].any()) for i in range(0, w * h, 64))
    return tiles, both, waves, linear



# What the oracle gives at SIZE (figures(): live reservoirs after the last spatiotemporal, RIS-only and ReSTIR-GI frame, black pixels,
# range and negative elements of the last spatiotemporal frame, RIS-only reservoirs with a radiance above 2^60, rays and lit pixels of
# pathTrace at depth 4; `inf` / `nan`: every output that holds any, with its count -- an output not listed holds none).  The oracle is
# deterministic and the size is fixed, so the counts are exact.
EXPECT = {
    "mirror_metal":                  dict(live=0, live0=0, black=1527, range='tame', negative=0, huge_li=0, gi_live=0, pt4_rays=5933, pt4_lit=0),
    "rough0_metal_half":             dict(live=860, live0=826, black=676, range='tame', negative=0, huge_li=0, gi_live=531, pt4_rays=7716, pt4_lit=165),
    "rough1e-6":                     dict(live=860, live0=826, black=676, range='tame', negative=0, huge_li=0, gi_live=692, pt4_rays=7816, pt4_lit=262),
    "rough1e-3_metal_half":          dict(live=860, live0=826, black=676, range='tame', negative=0, huge_li=0, gi_live=552, pt4_rays=7716, pt4_lit=176),
    "rough1_metal1":                 dict(live=860, live0=827, black=676, range='tame', negative=0, huge_li=0, gi_live=847, pt4_rays=5184, pt4_lit=436),
    "rough2_metal2":                 dict(live=860, live0=826, black=676, range='tame', negative=0, huge_li=0, gi_live=0, pt4_rays=2916, pt4_lit=0),
    "metallic0":                     dict(live=860, live0=826, black=676, range='tame', negative=0, huge_li=0, gi_live=1019, pt4_rays=7855, pt4_lit=744),
    "metallic1":                     dict(live=859, live0=825, black=677, range='tame', negative=0, huge_li=0, gi_live=901, pt4_rays=7495, pt4_lit=733),
    "base_zero":                     dict(live=860, live0=826, black=1527, range='tame', negative=0, huge_li=0, gi_live=4, pt4_rays=7994, pt4_lit=1),
    "base_above_one":                dict(live=860, live0=826, black=652, range='tame', negative=0, huge_li=0, gi_live=1035, pt4_rays=7994, pt4_lit=744),
    "base_zero_channel":             dict(live=860, live0=826, black=652, range='tame', negative=0, huge_li=0, gi_live=1035, pt4_rays=7994, pt4_lit=744),
    "light_1e25":                    dict(live=860, live0=826, black=652, range='above', negative=0, huge_li=894, gi_live=1035, pt4_rays=7994, pt4_lit=744),
    "light_3e38":                    dict(live=0, live0=0, black=1527, range='above', negative=0, huge_li=0, inf={'gi/f0/res.weight': 4, 'gi/f1/res.weight': 6, 'gi/f2/res.weight': 3}, gi_live=3, pt4_rays=7994, pt4_lit=4),
    "light_1e-30":                   dict(live=860, live0=826, black=652, range='below', negative=0, huge_li=0, gi_live=0, pt4_rays=7994, pt4_lit=744),
    "light_denormal":                dict(live=0, live0=0, black=1527, range='denormal', negative=0, huge_li=0, gi_live=0, pt4_rays=7994, pt4_lit=0),
    "light_zero":                    dict(live=0, live0=0, black=1536, range='zero', negative=0, huge_li=0, gi_live=0, pt4_rays=7994, pt4_lit=0),
    "light_negative":                dict(live=860, live0=826, black=652, range='tame', negative=884, huge_li=0, inf={'pt1/indirect': 1, 'pt4/indirect': 1}, gi_live=899, pt4_rays=7994, pt4_lit=744),
    "ior_1":                         dict(live=624, live0=588, black=904, range='tame', negative=0, huge_li=0, gi_live=755, pt4_rays=6119, pt4_lit=454),
    "ior_half":                      dict(live=624, live0=588, black=904, range='tame', negative=0, huge_li=0, gi_live=805, pt4_rays=6540, pt4_lit=523),
    "ior_zero":                      dict(live=624, live0=588, black=904, range='tame', negative=0, huge_li=0, gi_live=901, pt4_rays=7178, pt4_lit=635),
    "ior_1e4":                       dict(live=624, live0=588, black=904, range='tame', negative=0, huge_li=0, gi_live=901, pt4_rays=7178, pt4_lit=635),
    "ior_negative":                  dict(live=624, live0=588, black=904, range='tame', negative=0, huge_li=0, gi_live=901, pt4_rays=7178, pt4_lit=635),
    "ior_above_one":                 dict(live=624, live0=588, black=904, range='tame', negative=0, huge_li=0, gi_live=755, pt4_rays=6119, pt4_lit=454),
    "ior_below_one":                 dict(live=624, live0=588, black=904, range='tame', negative=0, huge_li=0, gi_live=755, pt4_rays=6119, pt4_lit=454),
    "zero_area_lights":              dict(live=864, live0=829, black=651, range='tame', negative=0, huge_li=0, gi_live=1038, pt4_rays=7994, pt4_lit=742),
    "dark_and_huge_lights":          dict(live=747, live0=700, black=733, range='above', negative=0, huge_li=778, gi_live=1001, pt4_rays=7932, pt4_lit=701),
    "tiny_1e19_light":               dict(live=865, live0=828, black=648, range='tame', negative=0, huge_li=0, gi_live=469, pt4_rays=7994, pt4_lit=175),
    "mixed_rough1e-6_boxes":         dict(live=860, live0=826, black=671, range='tame', negative=0, huge_li=0, gi_live=979, pt4_rays=7920, pt4_lit=644),
    "mixed_base_zero_back_wall":     dict(live=860, live0=826, black=884, range='tame', negative=0, huge_li=0, gi_live=980, pt4_rays=7994, pt4_lit=600),
    "mixed_mirror_left_wall_boxes":  dict(live=542, live0=512, black=1006, range='tame', negative=0, huge_li=0, gi_live=481, pt4_rays=7039, pt4_lit=245),
    "bistro_spread":                 dict(live=1353, live0=1193, black=151, range='above', negative=0, huge_li=1375),
}


def expected(name):
    return dict(dict(nan={}, inf={}), **EXPECT[name])
