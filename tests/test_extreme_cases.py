"""CPU: the case table of tests/extreme_cases.py on the oracle alone, and the host builders of the light sampler at the same extremes.

  * every case does what its row says: the oracle's three spatiotemporal ReSTIR frames, two RIS-only frames, the PT-direct baseline,
    pathTrace at depths 1 and 4, pathTraceIndirect at depth 3 and three frames of ReSTIR-GI at 48 x 32 give the figures of EXPECT --
    live reservoirs (exactly 0 where the case is about everything being filtered), an image above 2^60 or below 2^-60, black pixels,
    and which outputs hold NaN or infinity, with their counts;
  * the mixed cases put both kinds of pixel into one 32 x 8 tile: at least a quarter of the tiles that hold an extreme-material pixel
    also hold a Lambertian one, at 48 x 32 and at 97 x 61 (a condition on the input of tests/test_gpu_parameter_extremes.py); and the
    tiny 1e19 emitter puts candidates inside and outside the guarded range into every wave of the light sampler;
  * rs_build_light_table and rs_build_alias_table against the oracle, bit for bit, on power vectors that are all zero, a single entry,
    one 1e30 among 1e-30s, denormals only, a sum that overflows and one with a negative entry, and on every case's scene;
  * the comparison rule itself (same_bits_or_nan) refuses what it must refuse.
"""
import numpy as np
import pytest

from oracle import binding as ob
from restir_amd import capi
from restir_amd.ctypes_structs import LAMBERTIAN, LIGHT, make_materials
from tests import extreme_cases as xc
from tests.common import bits_equal

F32 = np.float32


@pytest.fixture(autouse=True)
def correctly_rounded_libm():
    """Owns the oracle's libm mode for every test of the module (extreme_cases.oracle_outputs refuses to run outside it)."""
    with xc.correctly_rounded_libm():
        yield


def test_the_table_holds_the_rows_it_was_asked_for():
    assert len(xc.MIXED) >= 3 and len(xc.NAMES) == len(set(xc.NAMES)) == len(xc.EXPECT)
    assert [n for n in xc.NAMES if xc.TABLE[n][0] != "cornell"] == ["bistro_spread"]
    sd = xc.scene("bistro_spread")
    lamps = sd.materials["baseColor"][sd.materials["type"] == LIGHT]
    assert int((sd.materials["type"][sd.material_ids] == LIGHT).sum()) > 1024            # k_ris reads the table from global memory
    assert 0 < lamps.min() < 1e-29 and 1e24 < lamps.max() < 1e26
    decades = np.floor(np.log10(lamps.max(axis=1).astype(np.float64)))
    assert len(np.unique(decades)) >= 50                                                # spread over the range, not two clusters


@pytest.mark.parametrize("name", xc.NAMES)
def test_case_is_not_vacuous(name):
    """The oracle's figures for the case equal the ones EXPECT states, and they say what the row is there for."""
    o = xc.oracle_outputs(name)
    got, want = xc.figures(o), xc.expected(name)
    assert got == want, (name, got, want)
    n = xc.SIZE[0] * xc.SIZE[1]
    img = o["direct3/f2/image"]
    # (what each family of rows must show, stated once here rather than read off EXPECT)
    if name in ("mirror_metal", "light_3e38", "light_denormal", "light_zero"):
        assert got["live"] == got["live0"] == 0                                          # every weight filtered
        assert all(xc.live(o["direct3/f%d/res" % f]) == 0 for f in range(3))
    else:
        assert got["live"] >= n // 3 and got["live0"] >= n // 3
    if name in ("light_1e25", "light_3e38", "dark_and_huge_lights", "bistro_spread"):
        assert got["range"] == "above" and np.isfinite(img).all()
    if name == "light_1e-30":
        assert got["range"] == "below" and F32(2.0 ** -126) < img.max() < F32(2.0 ** -60)
    if name == "light_denormal":
        assert 0 < img.max() < F32(2.0 ** -126)
    if name == "light_zero":
        assert not img.any() and not o["gi/f2/image"].any() and not o["pti3/indirect"].any()
    if name in ("base_zero", "mirror_metal"):
        lit = o["direct3/gbuffer/prim_id"] == -2
        assert got["black"] >= 1500 and lit[img.any(axis=1)].all()                       # only the light itself is seen
    if name in ("light_1e25", "dark_and_huge_lights", "bistro_spread"):
        assert got["huge_li"] >= 700                                                     # reservoirs that carry a radiance above 2^60
    if name == "light_negative":                                                         # negative values reach the images, and an infinity two planes
        assert got["negative"] >= 800 and want["inf"] == {"pt1/indirect": 1, "pt4/indirect": 1}
        assert all((o[k] < 0).any() for k in ("ptd/image", "pt4/direct", "pt4/indirect", "pti3/indirect", "gi/f2/image"))
        assert np.isneginf(o["pt4/indirect"]).sum() == 1                                 # the red channel: HDRToLDR(-1) = -1 / (1 - 1)
    else:
        assert got["negative"] == 0
    if name == "bistro_spread":
        v = img[img > 0]
        assert v.min() < 2.0 ** -60 and v.max() > 2.0 ** 60                              # both ends of the range in one frame
    if name.startswith("mixed_"):
        tame = xc.figures(xc.oracle_outputs("base_above_one"))                           # (any all-Lambertian run of the same geometry)
        assert got["black"] != tame["black"] or got["gi_live"] != tame["gi_live"]
    for key, a in o.items():
        if not isinstance(a, int) and not a.dtype.names and a.dtype == np.float32 and key not in want["inf"]:
            assert np.isfinite(a).all(), key


def test_tiny_light_puts_lanes_inside_and_outside_the_guarded_range_into_one_wave():
    """The light sampler of tiny_1e19_light, 4096 candidates from a point on the floor: about two of three draw the tiny emitter, with
    Li and pdf above 2^60; the others draw the ordinary light with both inside [2^-60, 2^60).  The draws of a wave's 64 lanes are
    independent, so a wave without both kinds has probability (2/3)^64 + (1/3)^64 < 1e-11."""
    from tests.common import oracle_scene
    sc = oracle_scene(xc.scene("tiny_1e19_light"))
    r = np.random.default_rng(5).uniform(0, 1, (4096, 4)).astype(F32)
    pdf, li, wi, dist = sc.sample_direct_light_nv(np.tile(np.array([0.3, 0.0, 0.2], F32), (4096, 1)), r)
    tiny = li.max(axis=1) > 2.0 ** 60
    assert 0.6 < tiny.mean() < 0.73, tiny.mean()
    assert (pdf[tiny] > 2.0 ** 60).all() and np.isfinite(pdf[tiny]).all()
    assert (li[~tiny] == 10).all() and (pdf[~tiny] > 2.0 ** -60).all() and (pdf[~tiny] < 2.0 ** 60).all()
    waves = tiny.reshape(64, 64)
    assert (waves.any(axis=1) & ~waves.all(axis=1)).all()
    assert (li[tiny].astype(np.float64).max(axis=1) / pdf[tiny] < 1e-15 * (10.0 / pdf[~tiny].max())).all()        # it never wins


def test_ior_rows_take_different_paths():
    """Ray counts differ per ior: the rows are not five copies of one run."""
    rays = {n: xc.expected(n)["pt4_rays"] for n in xc.NAMES if n.startswith("ior_")}
    assert len(set(rays.values())) >= 3, rays
    gi = {n: [xc.oracle_outputs(n)["gi/f%d/rays" % f] for f in range(3)] for n in rays}
    assert gi["ior_zero"] != gi["ior_1e4"], gi


@pytest.mark.parametrize("size", [xc.SIZE, xc.RAGGED], ids=["48x32", "97x61"])
@pytest.mark.parametrize("name", xc.MIXED)
def test_mixed_cases_put_both_kinds_of_pixel_into_one_tile(name, size):
    tiles, both, waves, linear = xc.mixed_tiles(name, size)
    assert tiles >= 6 and 4 * both >= tiles, (tiles, both)
    assert waves >= 16, waves                    # and into one wave of the tiled kernels: two rows of a block
    assert linear >= 8, linear                   # and of the kernels over the linear pixel index (k_ris, k_temporal): 64 consecutive pixels
    o = xc.oracle_outputs(name, size, ("direct3", "direct0"))                # (what the GPU module compares at this size)
    assert xc.nan_counts(o) == {} and xc.inf_counts(o) == {} and xc.live(o["direct3/f2/res"]) >= size[0] * size[1] // 4


def test_tiny_light_case_at_the_ragged_size():
    o = xc.oracle_outputs("tiny_1e19_light", xc.RAGGED, ("direct3", "direct0"))
    assert xc.nan_counts(o) == {} and xc.inf_counts(o) == {} and xc.live(o["direct3/f2/res"]) >= xc.RAGGED[0] * xc.RAGGED[1] // 4


# ---------------------------------------------------------------------------------------------------------------------------------
POWERS = {
    "all_zero": [0.0, 0.0, 0.0, 0.0, 0.0],
    "single": [5.0],
    "one_1e30_among_1e-30": [1e-30, 1e-30, 1e30, 1e-30, 1e-30, 1e-30, 1e-30],
    "denormals": [1e-42, 3e-45, 1e-40, 1.4e-45, 5e-39],
    "sum_overflows": [2e38, 1.0, 2e38, 3e37],
    "negative_entry": [1.0, -2.0, 3.0, 0.5],
}


def _same_alias_tables(power, where):
    pa, fa, sa = capi.build_alias_table(power)
    pb, fb, sb = ob.alias_build(power)
    nans = xc.same_bits_or_nan(pb, pa, (where, "prob"))
    assert np.array_equal(fa, fb), (where, "failId", fa, fb)
    assert sa == sb or (np.isnan(sa) and np.isnan(sb)), (where, "sumAll", sa, sb)
    assert ((fa >= 0) & (fa < len(power))).all()                 # whatever the powers, an index the kernels may chase
    return pb, sb, nans


@pytest.mark.parametrize("kind", list(POWERS))
def test_alias_table_of_extreme_powers(kind):
    power = np.array(POWERS[kind], F32)
    prob, total, nans = _same_alias_tables(power, kind)
    with np.errstate(over="ignore"):
        assert total == np.cumsum(power, dtype=F32)[-1]
    if kind == "all_zero":
        assert total == 0 and nans == len(power)                 # 0 * (n / 0): the NaN branch of the comparison rule is not idle
    elif kind == "single":
        assert total == 5 and prob[0] == 1 and nans == 0
    elif kind == "one_1e30_among_1e-30":
        assert total == F32(1e30) and nans == 0 and np.count_nonzero(prob) >= 1
    elif kind == "denormals":
        assert 0 < total < F32(2.0 ** -126)
    elif kind == "sum_overflows":
        assert np.isinf(total) and nans == 0 and not prob.any()   # n / inf = 0
    elif kind == "negative_entry":
        assert total == 2.5 and prob.min() < 0


@pytest.mark.parametrize("kind", list(POWERS))
def test_light_table_of_extreme_radiances(kind):
    """One emissive triangle of area 1 / (2 pi) per entry, its radiance (v, v, v): the light loop of buildDevData (src/scene.cpp:161-190)
    turns the vector into powers of the same size, and the alias table is built over those."""
    values = np.array(POWERS[kind], F32)
    k = len(values)
    side = np.sqrt(2.0 / (2.0 * np.pi))
    tri = np.array([[0, 0, 0], [side, 0, 0], [0, side, 0]], F32)
    verts = np.stack([tri + F32(i) for i in range(k + 1)])
    mats = make_materials([dict(type=LAMBERTIAN)] + [dict(type=LIGHT, baseColor=(v, v, v)) for v in values])
    ids = np.arange(k + 1, dtype=np.int32)
    la = capi.build_light_table(verts, ids, mats)
    lb = ob.light_table(verts, ids, mats)
    assert np.array_equal(la[0], lb[0]) and list(lb[0]) == list(range(1, k + 1))
    assert xc.same_bits_or_nan(lb[1], la[1], (kind, "radiance")) == 0 and bits_equal(lb[1][:, 0], values)
    assert xc.same_bits_or_nan(lb[2], la[2], (kind, "power")) == 0
    mid = (np.abs(values) >= 1e-30) & (np.abs(values) <= 1e30)        # (2e38 * 2 pi overflows before the area brings it back; denormals lose bits)
    assert np.allclose(lb[2][mid].astype(np.float64) / values[mid].astype(np.float64), 1.0, rtol=1e-5), lb[2]
    _same_alias_tables(lb[2], (kind, "from the light table"))


@pytest.mark.parametrize("name", xc.NAMES)
def test_host_builders_on_the_scene_of_every_case(name):
    sd = xc.scene(name)
    la = capi.build_light_table(sd.vertices, sd.material_ids, sd.materials)
    lb = ob.light_table(sd.vertices, sd.material_ids, sd.materials)
    assert np.array_equal(la[0], lb[0])
    assert xc.same_bits_or_nan(lb[1], la[1], (name, "radiance")) == 0 and xc.same_bits_or_nan(lb[2], la[2], (name, "power")) == 0
    prob, total, nans = _same_alias_tables(lb[2], name)
    if name == "light_zero":
        assert total == 0 and nans == 2
    elif name == "light_3e38":
        assert np.isinf(lb[2]).all() and np.isinf(total) and nans == 2      # power * (n / inf) = inf * 0
    elif name == "zero_area_lights":
        assert len(prob) == 4 and (lb[2][2:] == 0).all() and (prob[2:] == 0).all()
    elif name == "tiny_1e19_light":
        assert np.allclose(prob, [0.5, 0.5, 1.0], rtol=1e-6) and np.allclose(lb[2], [7.853982, 7.853982, 31.415926], rtol=1e-5)
    elif name == "dark_and_huge_lights":
        assert len(prob) == 6 and (lb[2][2:4] == 0).all() and lb[2][4] > 1e27
    else:
        assert nans == 0 and np.isfinite(total)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_comparison_rule_refuses_what_it_must():
    host_nan, device_nan = np.array([0xFFC00000], np.uint32).view(F32)[0], np.array([0x7FC00000], np.uint32).view(F32)[0]
    a = np.array([[1.0, host_nan, 0.0], [np.inf, -0.0, 3.0]], F32)
    b = a.copy(); b[0, 1] = device_nan
    assert xc.same_bits_or_nan(a, b) == 1 and xc.same_bits_or_nan(a, a) == 1 and not bits_equal(a, b)
    for i, v in (((0, 1), 2.0), ((0, 0), device_nan), ((1, 1), 0.0), ((1, 2), np.nextafter(F32(3), F32(4))), ((1, 0), F32(3e38))):
        c = b.copy(); c[i] = v
        with pytest.raises(AssertionError):
            xc.same_bits_or_nan(a, c)
    with pytest.raises(AssertionError):
        xc.same_bits_or_nan(a, b[:1])
    assert xc.same_bits_or_nan(np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32)) == 0
    with pytest.raises(AssertionError):
        xc.same_bits_or_nan(np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32)[::-1])
    # compare(): keys, ray counts and the fields of a reservoir array
    o = xc.oracle_outputs("light_zero")
    d = dict(o)
    assert xc.compare(o, d) == {}
    d["pt4/rays"] = o["pt4/rays"] + 1
    with pytest.raises(AssertionError):
        xc.compare(o, d)
    d = dict(o); r = o["direct3/f2/res"].copy(); r["wi"][5, 1] = host_nan; d["direct3/f2/res"] = r
    with pytest.raises(AssertionError):
        xc.compare(o, d)
    assert xc.compare(d, d) == {"direct3/f2/res.wi": 1}
    d = dict(o); del d["gi/f0/res"]
    with pytest.raises(AssertionError):
        xc.compare(o, d)
