"""CPU: the case table of tests/geometric_cases.py on the oracle and a NumPy restatement of the grid alone -- what makes every case of
tests/test_gpu_geometric_extremes.py non-vacuous.

  * every case obeys the table's rules: float32 vertices, all finite, a camera that went through the same map, appended triangles that
    copy an existing one;
  * the oracle's figures equal EXPECT, and they clear the floors: at least 0.3 of the generator's rays hit, between 0.05 and 0.95 of its
    segments are occluded, the special triangles of a case are hit (both the copies and the originals of `coincident`, at least one
    sliver of `needles`, every aimed segment of `sub_cell` occluded), the camera sees geometry in at least 0.3 of the pixels and the
    last frame is not black;
  * the grid exists exactly where EXPECT says, by rs_quantize_occlusion_bvh restated (scale = ext / 65000, base = lo - 200 * scale
    rounded in float, margin = 2^-17 ext, tests/refit_tables.grid_box over every leaf box and the root), and where it exists at least
    half of the rays and of the segments are general-case and within grid_reaches, so that the fast lanes are really walked;
  * what each case is there for holds of its geometry: ulps of many grid steps (`far`), an apron lost to rounding (`beyond_grid`), 64
    steps across (`slab`), one step thick (`squashed`), boxes inside one cell (`sub_cell`), the smallest scale the reference renders
    (`tiny`).
"""
import numpy as np
import pytest

from tests import extreme_cases as xc
from tests import geometric_cases as gc
from tests.common import OracleRenderer, get_scene, oracle_scene
from tests.geometry_edits import movable
from tests.ray_cases import closest_like_rays

F32, F64 = np.float32, np.float64


@pytest.fixture(autouse=True)
def correctly_rounded_libm():
    """Owns the oracle's libm mode for every test of the module (geometric_cases.oracle_frames refuses to run outside it)."""
    with xc.correctly_rounded_libm():
        yield


def test_the_table_holds_the_cases_it_was_asked_for():
    assert list(gc.TABLE) == ["far", "beyond_grid", "apron_of_two_ulps", "huge", "tiny", "slab", "squashed", "sub_cell", "coincident", "needles",
                              "edited_into_extremes"]
    assert all(gc.TABLE[n][0] == gc.BASES for n in gc.TABLE if n not in ("edited_into_extremes", "apron_of_two_ulps"))
    assert gc.TABLE["edited_into_extremes"][0] == gc.TABLE["apron_of_two_ulps"][0] == ("sponza:0.03",)
    assert set(gc.EXPECT) == set(gc.CASES) and len(gc.CASES) == 20
    assert not any(gc.EXPECT["beyond_grid", b]["grid"] for b in gc.BASES)            # the case is the one without grid trees, on both bases
    assert all(v["grid"] for k, v in gc.EXPECT.items() if k[0] != "beyond_grid")
    assert get_scene("cornell").num_prims == 36 and get_scene("sponza:0.03").num_prims == 7864


@pytest.mark.parametrize("name,base", gc.CASES, ids=gc.CASE_IDS)
def test_case_obeys_the_rules(name, base):
    c, fresh = gc.case(name, base), get_scene(base)
    for sd in (c.sd, c.after):
        assert sd.vertices.dtype == F32 and np.isfinite(sd.vertices).all()
        assert len(sd.vertices) == len(sd.normals) == len(sd.texcoords) == len(sd.material_ids) >= c.n0
    assert np.array_equal(c.sd.normals[:c.n0], fresh.normals) and np.array_equal(c.sd.material_ids[:c.n0], fresh.material_ids)
    assert {k: v for k, v in c.sd.camera_args.items() if k != "position"} == {k: v for k, v in fresh.camera_args.items() if k != "position"}
    # the base triangles and the camera went through ONE affine map: recover it from the root boxes and apply it to the camera
    lo0, hi0 = gc.root_box64(fresh)
    v = c.sd.vertices[:c.n0].reshape(-1, 3).astype(F64)
    lo1, hi1 = v.min(0), v.max(0)
    scale = (hi1 - lo1) / (hi0 - lo0)
    shift = lo1 - lo0 * scale
    mapped = c.notes.get("mapped_camera", c.sd.camera_args["position"])
    want = np.asarray(fresh.camera_args["position"], F64) * scale + shift
    assert np.allclose(mapped, want, rtol=1e-6, atol=np.abs(shift).max() * 1e-7), (mapped, want)
    if len(set(np.round(np.log2(scale), 6))) == 1:
        assert scale[0] <= 2.0 ** 20
    for p in range(c.n0, c.sd.num_prims):                    # an appended triangle copies an existing one's shading data
        same = (c.sd.normals[:c.n0] == c.sd.normals[p]).all((1, 2)) & (c.sd.texcoords[:c.n0] == c.sd.texcoords[p]).all((1, 2))
        assert (same & (c.sd.material_ids[:c.n0] == c.sd.material_ids[p])).any(), p
    assert len(c.rays) == len(c.segs) == gc.N_GENERATED + (gc.N_AIMED if c.aimed is not None else 0)
    assert int(c.aimed_rays.sum()) == int(c.aimed_segs.sum()) == len(c.rays) - gc.N_GENERATED
    for k in range(0, len(c.rays) - 64, 64):                 # shuffled: where there are aimed rays, no wave is of one kind alone
        if c.aimed is not None:
            assert 0 < c.aimed_rays[k:k + 64].sum() < 64 and 0 < c.aimed_segs[k:k + 64].sum() < 64


@pytest.mark.parametrize("name,base", gc.CASES, ids=gc.CASE_IDS)
def test_case_is_not_vacuous(name, base):
    """The figures equal the ones EXPECT states, and they clear the floors."""
    want = {k: v for k, v in gc.EXPECT[name, base].items() if k != "camera"}
    got = dict(gc.figures(name, base), **gc.frame_figures(name, base))
    assert got == want, (name, base, got, want)
    assert got["hits"] >= gc.MIN_HITS and 0.05 < got["occluded"] < 0.95
    assert got["coverage"] >= gc.MIN_COVERAGE and got["lit"] > 0
    if got["grid"]:
        assert min(got["walked"]) >= gc.MIN_REACH
    if name == "sub_cell":
        assert got["aimed_hits"] >= 0.8 * gc.N_AIMED and got["aimed_occluded"] == gc.N_AIMED
        assert got["hits_on_cluster_lights"] > 0 and got["hits_on_cluster"] > got["hits_on_cluster_lights"]
    if name == "coincident":
        assert got["hits_on_copies"] > 0 and got["hits_on_originals"] > 0
    if name == "needles":
        assert got["hits_on_slivers"] >= 1
    if name == "edited_into_extremes":
        assert got["hits_on_cluster"] > 0 and got["hits_on_corners"] > 0 and got["aimed_occluded"] == gc.N_AIMED


@pytest.mark.parametrize("name,base", [(n, b) for n, b in gc.CASES if n in gc.RAGGED_TOO], ids=lambda v: v.split(":")[0])
def test_the_ragged_frames_see_geometry_too(name, base):
    o = gc.oracle_frames(name, base, gc.RAGGED)
    assert gc.coverage(o["direct/f0/gbuffer/prim_id"]) >= gc.MIN_COVERAGE and o["direct/f2/image"].any()


def test_a_camera_is_chosen_only_where_the_mapped_one_sees_too_little():
    chosen = [k for k, v in gc.EXPECT.items() if "camera" in v]
    assert chosen == [("squashed", "cornell")]
    c = gc.case(*chosen[0])
    assert tuple(c.sd.camera_args["position"]) == tuple(gc.EXPECT[chosen[0]]["camera"])
    r = OracleRenderer(c.sd, *gc.SIZE, scene=gc.oracle_scene_of(*chosen[0]))
    r.set_camera_position(c.notes["mapped_camera"])          # edge-on to a box 3e-5 high from 2.5 away: it sees nothing
    r.gbuf.render(r.scene, r.cam)
    assert gc.coverage(r.gbuf.prim_id[r.gbuf.frame_idx]) < gc.MIN_COVERAGE


# ---- the grid ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,base", gc.CASES, ids=gc.CASE_IDS)
def test_the_grid_exists_where_expect_says(name, base):
    c = gc.case(name, base)
    g = gc.grid_of(c.sd.vertices)
    assert g["exists"] == gc.EXPECT[name, base]["grid"] and g["refused"] == gc.EXPECT[name, base]["refused"]
    if c.edit is not None:                                   # the edit stays inside the box the grid was laid over, corners included
        v = c.edit[1].reshape(-1, 3)
        assert (v >= g["lo"]).all() and (v <= g["hi"]).all() and gc.grid_of(c.after.vertices)["exists"]
        assert np.array_equal(gc.grid_of(c.after.vertices)["base"], g["base"])


def test_what_each_case_does_to_the_grid():
    for base in gc.BASES:
        g = {n: gc.grid_of(gc.case(n, base).sd.vertices) for n in ("far", "beyond_grid", "slab", "squashed", "sub_cell", "huge")}
        ulp = lambda x: float(np.spacing(F32(abs(x))))
        far = g["far"]
        assert far["exists"] and ulp(far["hi"][1]) / far["scale"][0] > (30 if base == "cornell" else 1)
        slab = g["slab"]
        steps = (slab["hi"] - slab["lo"]) / slab["scale"]
        assert steps[0] > 64000 and steps[1] < 70 and (base != "cornell" or 60 < steps[2] < 70)
        sq = g["squashed"]
        assert 0 < (sq["hi"][1] - sq["lo"][1]) / sq["scale"][1] < 1.5
        c = gc.case("sub_cell", base)
        v = c.sd.vertices[c.special["cluster"]].astype(F64)
        lo, hi = gc.root_box64(c.sd)                          # (the cluster lies inside the scaled base's box: the root box is that box)
        at = lo + np.asarray(gc.CLUSTER_AT) * (hi - lo)
        step = float(g["sub_cell"]["scale"][0])
        assert np.abs(v - at).max() <= step / 8 + ulp(hi.max()) and (v.max(1) - v.min(1)).max() < step / 2
        assert (c.sd.materials["type"][c.sd.material_ids[c.special["cluster_lights"]]] == gc.LIGHT).all() and len(c.special["cluster_lights"]) == 32
        assert (c.sd.materials["type"][c.sd.material_ids[c.special["cluster"][:32]]] != gc.LIGHT).all()
    # beyond the apron: at x = 1e6 the ulp of cornell's base (1 / 16) swallows its 200 steps (0.006), at 1.6e7 the ulp 1 the Sponza-class
    # scene's 0.12: the base is the root's own lower x face, grid_box turns down every box that touches it, and the scene has no grid
    for base in gc.BASES:
        b = gc.grid_of(gc.case("beyond_grid", base).sd.vertices)
        steps = 200 * float(b["scale"][0])
        assert not b["exists"] and b["refused"] > 0 and b["base"][0] == b["lo"][0] and float(np.spacing(b["lo"][0])) > steps
    # the same scene at 1e6, where the 200 steps are two ulps: an apron survives and the grid fits
    s = gc.grid_of(gc.case("apron_of_two_ulps", "sponza:0.03").sd.vertices)
    assert s["exists"] and 0 < (s["lo"][0] - s["base"][0]) / s["scale"][0] < 400
    assert 1.5 < 200 * float(s["scale"][0]) / float(np.spacing(s["lo"][0])) < 2.5


def test_tiny_is_the_smallest_scale_the_reference_renders():
    """Halving from 1: the first power of two at which the oracle hits fewer than 0.3 of closest_like_rays on one of the bases is half
    of TINY_SCALE."""
    scale = 1.0
    while True:
        shares = []
        for base in gc.BASES:
            sd = get_scene(base)
            gc._affine(sd, scale=(scale,) * 3)
            shares.append(float((oracle_scene(sd).intersect(closest_like_rays(sd, gc.N_GENERATED, 34))[0] >= 0).mean()))
        if min(shares) < gc.MIN_HITS:
            break
        scale /= 2
        assert scale > 2.0 ** -30
    assert scale * 2 == gc.TINY_SCALE
    assert [gc.EXPECT["tiny", b]["hits"] for b in gc.BASES] == [0.7718, 0.8103]


# ---- the special triangles ---------------------------------------------------------------------------------------------------------------
def test_the_special_triangles_are_what_the_cases_say():
    for base in gc.BASES:
        c = gc.case("coincident", base)
        copies, originals = c.special["copies"], c.special["originals"]
        assert len(copies) == min(64, c.n0) == len(set(originals)) and (copies >= c.n0).all() and (originals < c.n0).all()
        for a in ("vertices", "normals", "texcoords", "material_ids"):
            assert np.array_equal(getattr(c.sd, a)[copies], getattr(c.sd, a)[originals])
        c = gc.case("needles", base)
        lo, hi = gc.root_box64(get_scene(base))
        ext = (hi - lo).max()
        v = c.sd.vertices[c.special["slivers"]].astype(F64)
        assert len(v) == 32 and np.allclose(np.linalg.norm(v[:, 2] - v[:, 0], axis=1), ext, rtol=1e-6)
        width = np.linalg.norm(v[:, 1] - v[:, 0], axis=1)
        assert (width < 4 * gc.SLIVER_WIDTH * ext).all() and gc.SLIVER_WIDTH == 2.0 ** -22      # (a few ulps wide: rounding moves the width)
        assert (c.sd.vertices.reshape(-1, 3) >= lo.astype(F32)).all() and (c.sd.vertices.reshape(-1, 3) <= hi.astype(F32)).all()
        z = c.sd.vertices[c.special["zero_area"]].astype(F64)
        assert len(z) == 8 and not np.cross(z[:, 1] - z[:, 0], z[:, 2] - z[:, 0]).any()
        assert (z[:4, 0] == z[:4, 1]).all() and (z[:4, 0] == z[:4, 2]).all() and (z[4:, 0] != z[4:, 2]).any(1).all()
        assert (c.sd.materials["type"][c.sd.material_ids[c.special["zero_area"]]] != gc.LIGHT).all()
    c = gc.case("edited_into_extremes", "sponza:0.03")
    ids, v = c.edit
    assert len(ids) == len(set(ids)) == 72 and np.isin(ids, movable(c.sd)).all()
    g = gc.grid_of(c.sd.vertices)
    corners = v[64:].reshape(-1, 3)
    assert ((corners == g["lo"]) | (corners == g["hi"])).all() and len(np.unique(corners, axis=0)) == 8
    assert np.array_equal(c.after.vertices[ids], v) and np.array_equal(np.delete(c.after.vertices, ids, 0), np.delete(c.sd.vertices, ids, 0))


def test_the_reference_hits_triangles_beside_in_plane_rays_in_large_scenes():
    """What the axis cull of the reference walk must not skip: at the generators' own scale the reference's absolute FLT_EPSILON rejects
    the rounding-sized determinant of a ray inside a triangle's plane; in larger scenes it accepts it, and the ray "hits" a triangle it
    runs beside.  The cases and the scaled room hold such hits, the unscaled bases none."""
    for base in gc.BASES:
        sd = get_scene(base)
        rays = closest_like_rays(sd, gc.N_GENERATED, 34)
        assert gc.hits_beside_the_ray(sd, rays, oracle_scene(sd).intersect(rays)[0]) == 0
        for name in ("huge", "sub_cell"):
            c = gc.case(name, base)
            assert gc.hits_beside_the_ray(c.after, c.rays, gc.oracle_hits(name, base)[0]) > 0, (name, base)
    sd, rays, _ = gc.scaled_room()
    assert gc.hits_beside_the_ray(sd, rays, oracle_scene(sd).intersect(rays)[0]) >= 10


def test_the_edit_that_must_switch_the_axis_cull_off():
    """tests/test_gpu_geometric_extremes.py test_an_edit_that_brings_large_triangles: before the edit every triangle is small enough for
    the cull (scene.hip far_skip_allowed: edge-component product at most 1), after it six are not, they stay inside the root box, and the
    oracle hits them beside in-plane rays -- hits a walk that still culled would miss."""
    sd, (ids, v), after, rays, segs = gc.edit_room()
    assert gc.edge_product(sd.vertices) <= 1.0 < 100.0 < gc.edge_product(after.vertices)
    lo, hi = gc.grid_of(sd.vertices)["lo"], gc.grid_of(sd.vertices)["hi"]
    assert gc.grid_of(sd.vertices)["exists"] and (v.reshape(-1, 3) >= lo).all() and (v.reshape(-1, 3) <= hi).all()
    sc = gc.edit_room_oracle()
    prim = sc.intersect(rays)[0]
    assert gc.hits_beside_the_ray(after, rays, prim) >= 100 and 0.3 < (prim >= 0).mean()
    assert 0.05 < sc.test_occlusion(segs).mean() < 0.95
