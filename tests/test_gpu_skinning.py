"""Skinned meshes (rs_scene_define_skin, rs_scene_set_bone_transforms) bit for bit: against the CPU oracle on the arrays rs_skin_corners
gives (host only; tests/test_skinning_host.py holds it to a NumPy restatement and to rs_bake_matrix), and against a second library scene
edited by rs_scene_set_geometry with the same arrays -- every device table, the emissive grid, the host description.  Corner counts on
either side of a wave and of a block, palettes of 1 to 256 bones, the partial refit, emitters, frames in flight, motion vectors, the rest
arrays and what crosses the bus, subsets of bones, refusals, row bands.  No comparison has a tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import binding as ob
from tests import motion_vectors as mv
from tests import part_transforms as pt
from tests import skinning as sk
from tests.common import HipRenderer, bits_equal, hip_scene, next_looper, oracle_scene
from tests.emitter_edits import edited_oracle_scene, emitters, scene_data
from tests.geometry_edits import apply_triangles, probe_rays, probe_segments, root_box
from tests.scene_edits import assert_same, differing
from tests.test_gpu_part_transforms import (H, INVALID, N_RAYS, N_SEGMENTS, SPONZA, UNSUPPORTED, W, all_tables, assert_desc_equal,
                                            assert_tables_equal, hip_outputs, oracle_outputs, refused, with_libm)

pytestmark = pytest.mark.gpu

BONE_BYTES = 112
ALL_SKINS = [(n, k) for n in sk.SKINS for k in sk.SKINS[n]]


@pytest.fixture(autouse=True)
def exact_libm(hip):
    ob.set_libm_mode(1)            # cos / sin correctly rounded on both sides: every bit must agree
    hip.set_sync(True)
    yield
    ob.set_libm_mode(0)
    hip.set_sync(True)
    hip.set_side_stream(4)         # the library's default


def skinned_scene(hip, name, key):
    s = hip_scene(hip, scene_data(name))
    sk.skin_of(name, key).define(s)
    return s


def emitters_in(name, key):
    return int(np.isin(sk.skin_of(name, key).ids, emitters(scene_data(name))).sum())


# ---- 1. outputs after a pose --------------------------------------------------------------------------------------------------------------
OUTPUT_CASES = [("cornell", "box_lamp"), (SPONZA, "t22"), (SPONZA, "t386"), (SPONZA, "lamps")]


@functools.lru_cache(maxsize=None)
def expected_after(name, key):
    """(vertices, normals) after the pose of step 0 of every bone, from rs_skin_corners alone; the places triangles moved from and to."""
    from restir_amd import capi
    sd = scene_data(name)
    v, n = sd.vertices.reshape(-1, 3, 3).copy(), sd.normals.reshape(-1, 3, 3).copy()
    ids, sv, sn = sk.Palette(capi, name, key).set(*sk.pose(name, key, 0))
    places = np.concatenate([v[ids].mean(1), sv.mean(1)])
    v, n = apply_triangles(v, n, ids, sv, sn)
    return v, n, places


def probes(name, key):
    places = expected_after(name, key)[2]
    places = places[np.random.default_rng(5).permutation(len(places))[:64]]
    sd = scene_data(name)
    return probe_rays(sd, places, N_RAYS, 41), probe_segments(sd, places, N_SEGMENTS, 42)


@functools.lru_cache(maxsize=None)
@with_libm
def oracle_after(name, key):
    from restir_amd import capi
    sd = scene_data(name)
    v, n, _ = expected_after(name, key)
    scene = edited_oracle_scene(capi, oracle_scene(sd), np.arange(len(v), dtype=np.int32), v, n)
    return oracle_outputs(sd, scene, *probes(name, key))


@pytest.mark.parametrize("name,key", OUTPUT_CASES)
def test_outputs_after_pose(hip, name, key):
    """One pose of every bone.  The host description then holds rs_skin_corners of the rest pose on the listed triangles and the old bits
    elsewhere; the device's vertices and normals equal it; closest-hit and occlusion probes, the G-buffer planes and three ReSTIRDirect
    frames with reuse 3 (image, reservoirs), and rs_path_trace at depth 3 equal the oracle's on a fresh scene made from those arrays."""
    sd = scene_data(name)
    v_want, n_want, _ = expected_after(name, key)
    s = skinned_scene(hip, name, key)
    s.set_bone_transforms(*sk.pose(name, key, 0))
    v_got, n_got = s.geometry()
    assert bits_equal(v_got, v_want) and bits_equal(n_got, n_want)
    moved = np.sort(sk.skin_of(name, key).ids.astype(np.int64))
    still = np.setdiff1d(np.arange(len(v_want)), moved)
    assert bits_equal(v_got[still], sd.vertices.reshape(-1, 3, 3)[still]) and bits_equal(n_got[still], sd.normals.reshape(-1, 3, 3)[still])
    assert differing(v_got[moved], sd.vertices.reshape(-1, 3, 3)[moved]) == len(moved)
    assert bits_equal(s.debug_table("vertices"), v_got) and bits_equal(s.debug_table("normals"), n_got)
    assert bits_equal(s.host_desc()["boxes"], hip.refit_boxes(v_want, s.host_desc()["nodes"][0]))
    rays, seg = probes(name, key)
    ref, got = oracle_after(name, key), hip_outputs(hip, sd, s, rays, seg)
    for k, want in ref.items():
        for out in ([k] if k != "closest" else ["closest", "closest_wave"]):
            assert_same(want, got[out], (name, key, out))


# ---- 2. the same as rs_scene_set_geometry -------------------------------------------------------------------------------------------------
def assert_twins(a, b, tag):
    assert_tables_equal(all_tables(a), all_tables(b), tag)
    assert repr(a.emissive_grid()) == repr(b.emissive_grid()), tag
    assert_desc_equal(a.host_desc(), b.host_desc(), tag)
    assert a.light_moves() == b.light_moves() and a.geometry_edits() == b.geometry_edits(), tag
    assert a.refit_counts() == b.refit_counts(), tag
    ba, bb = a.dirty_boxes(0), b.dirty_boxes(0)
    assert bits_equal(ba[0], bb[0]) and ba[1] == bb[1], tag


@pytest.mark.parametrize("partial", [False, True], ids=["whole", "partial"])
@pytest.mark.parametrize("name,key", ALL_SKINS)
def test_same_as_set_geometry(hip, name, key, partial):
    """Two scenes from one description, one posed by rs_scene_set_bone_transforms, the other edited by rs_scene_set_geometry with the
    arrays of rs_skin_corners, three times over: every table of rs_debug_scene_table byte for byte, the emissive grid, the host description
    with lightProb, lightFailId and sumLightPower, rs_scene_light_moves, the dirty boxes and the refit counts.  With the partial refit on,
    the first edit of a scene is whole and the later ones partial on both.  A skin with emitters moves the lights the same way; one
    without leaves the sampler, the emissive tree's records and its grid as they were."""
    sd = scene_data(name)
    a, b = skinned_scene(hip, name, key), hip_scene(hip, sd)
    if partial:
        a.set_partial_refit(True)
        b.set_partial_refit(True)
    lamps = emitters_in(name, key)
    assert (lamps > 0) == (key in ("box_lamp", "lamps"))
    start, start_grid = a.host_desc(), repr(a.emissive_grid())
    start_emi = all_tables(a, ("emiNodes", "emiTris"))
    pal = sk.Palette(hip, name, key)
    for step in (0, 1, 2):
        ids, ms = sk.pose(name, key, step)
        a.set_bone_transforms(ids, ms)
        assert a.staged_bytes() == sk.skin_of(name, key).num_bones * BONE_BYTES
        b.set_geometry(*pal.set(ids, ms))
        assert_twins(a, b, (name, key, step))
        assert a.refit_counts() == ((1, step) if partial else (step + 1, 0)), (name, key, step)
        assert a.light_moves() == (step + 1 if lamps else 0)
        d = a.host_desc()
        if lamps:
            assert not bits_equal(a.debug_table("emiTris")["v0"], start_emi["emiTris"]["v0"])
        else:
            assert bits_equal(d["light_prob"], start["light_prob"]) and d["sum_power"] == start["sum_power"]
            assert repr(a.emissive_grid()) == start_grid
            assert_tables_equal(all_tables(a, ("emiNodes", "emiTris")), start_emi, "no emitter listed")


# ---- 3. the rest arrays, what crosses the bus, no drift -------------------------------------------------------------------------------------
def assert_definition(s, skin, tag, rest=None):
    ids, v, n, b, w = s.download_skin()
    rv, rn = (skin.rest_vertices, skin.rest_normals) if rest is None else rest
    assert np.array_equal(ids, skin.ids) and bits_equal(v, rv) and bits_equal(n, rn), tag
    assert np.array_equal(b, skin.bone_ids) and bits_equal(w, skin.weights), tag
    assert s.skin_info() == (skin.num_bones, len(skin.ids)), tag


def test_staged_bytes_rest_pose_and_no_drift(hip):
    """256 bones over 386 triangles: every pose stages the whole palette, 256 x 112 bytes, whichever bones it names; the device's copy of
    the definition is the same after 12 poses; and the 12th pose's tables equal those of a fresh scene given that palette once."""
    name, key = SPONZA, "t386"
    sd, skin = scene_data(name), sk.skin_of(name, key)
    s = hip_scene(hip, sd)
    assert s.skin_info() == (0, 0) and s.staged_bytes() == 0
    skin.define(s)
    assert_definition(s, skin, "defined")
    pal = sk.Palette(hip, name, key)
    for step in range(12):
        bones = None if step % 3 == 0 else np.arange(step, skin.num_bones, 5)
        ids, ms = sk.pose(name, key, step, bones)
        s.set_bone_transforms(ids, ms)
        pal.set(ids, ms)
        assert s.staged_bytes() == 256 * BONE_BYTES == 28672, step
    assert_definition(s, skin, "after 12 poses")
    want = pal.skinned()
    assert bits_equal(s.geometry()[0][want[0]], want[1]) and bits_equal(s.geometry()[1][want[0]], want[2])
    fresh = skinned_scene(hip, name, key)
    fresh.set_bone_transforms(np.arange(skin.num_bones), pal.matrices)
    assert_tables_equal(all_tables(s), all_tables(fresh), "the 12th pose against the same palette given once")
    assert_desc_equal(s.host_desc(), fresh.host_desc(), "host description")
    # rs_scene_set_geometry stages the records themselves; the next pose puts the triangles back on the skinned rest pose
    s.set_geometry(skin.ids, skin.rest_vertices, skin.rest_normals)
    assert s.staged_bytes() >= 386 * 76 > 28672
    assert_definition(s, skin, "after set_geometry on the skin's triangles")
    s.set_bone_transforms(*sk.pose(name, key, 12, [7]))
    want = pal.set(*sk.pose(name, key, 12, [7]))
    assert bits_equal(s.geometry()[0][want[0]], want[1]) and bits_equal(s.debug_table("vertices"), s.geometry()[0])
    # count == 0: nothing happens
    before = s.geometry()[0]
    s.set_bone_transforms([], np.zeros((0, 4, 4), np.float32))
    assert s.staged_bytes() == 28672 and bits_equal(s.geometry()[0], before) and s.geometry_edits() == 14


def test_definitions_replace_each_other(hip):
    """NULL rest arrays take the pose at the call; explicit ones are kept and posed; a new definition starts from identities; none drops
    it.  Parts and a skin on the same triangles: the last edit wins."""
    name = SPONZA
    sd = scene_data(name)
    s = hip_scene(hip, sd)
    a, b = sk.skin_of(name, "t22"), sk.skin_of(name, "t85")
    a.define(s)
    s.set_bone_transforms(*sk.pose(name, "t22", 0))
    posed = s.geometry()
    a.define(s)                                          # again, NULL rest arrays: the rest pose is the posed one now
    assert_definition(s, a, "the pose at the call", (posed[0][a.ids], posed[1][a.ids]))
    # explicit rest arrays: the triangles pulled 1 % towards their common centroid
    c = a.rest_vertices.reshape(-1, 3).mean(0)
    rest = (np.ascontiguousarray(a.rest_vertices * np.float32(0.99) + np.float32(0.01) * c).astype(np.float32), a.rest_normals)
    s.define_skin(a.num_bones, a.ids, a.bone_ids, a.weights, *rest)
    assert_definition(s, a, "explicit rest arrays", rest)
    assert bits_equal(s.geometry()[0], posed[0])         # a definition changes no geometry
    ids, ms = sk.pose(name, "t22", 1, [3])
    s.set_bone_transforms(ids, ms)                       # the other four bones are identities again
    palette = np.stack([pt.identity()] * a.num_bones)
    palette[3] = ms[0]
    v, n = hip.skin_corners(palette, rest[0], rest[1], a.bone_ids, a.weights)
    assert bits_equal(s.geometry()[0][a.ids], v.reshape(-1, 3, 3)) and bits_equal(s.geometry()[1][a.ids], n.reshape(-1, 3, 3))
    # parts over the same triangles
    s.define_parts([a.ids.tolist()], a.rest_vertices, a.rest_normals)
    m = pt.translation((0.0, 0.01, 0.0))
    s.set_part_transforms([0], [m])
    assert bits_equal(s.geometry()[0][a.ids], hip.bake_matrix(m, a.rest_vertices, a.rest_normals)[0].reshape(-1, 3, 3))
    s.set_bone_transforms(ids, ms)
    assert bits_equal(s.geometry()[0][a.ids], v.reshape(-1, 3, 3))
    assert s.parts_info() == (1, 22) and s.skin_info() == (5, 22)
    now = s.geometry()
    b.define(s)                                          # (some of its triangles are a's: NULL rest arrays take them where they stand)
    assert_definition(s, b, "replaced", (now[0][b.ids], now[1][b.ids]))
    s.define_skin(0, [], np.zeros((0, 3, 4), np.int32), np.zeros((0, 3, 4), np.float32))
    assert s.skin_info() == (0, 0) and s.parts_info() == (1, 22)
    refused(hip, INVALID, s.set_bone_transforms, [0], [pt.identity()])
    refused(hip, INVALID, s.download_skin)


# ---- 4. a subset of bones -----------------------------------------------------------------------------------------------------------------------
def test_subset_of_bones_and_a_bone_named_twice(hip):
    name, key = SPONZA, "t22"
    a, b = skinned_scene(hip, name, key), hip_scene(hip, scene_data(name))
    pal = sk.Palette(hip, name, key)
    m = lambda bone, step: sk.bone_matrix(name, key, bone, step)
    calls = [([0, 1, 2, 3, 4], [m(k, 0) for k in range(5)]),
             ([1, 3], [m(1, 1), m(3, 1)]),               # 0, 2 and 4 stay at step 0
             ([2, 4, 2], [m(2, 2), m(4, 2), m(2, 3)]),   # bone 2 takes its last matrix
             ([0], [m(0, 3)])]
    for i, (ids, ms) in enumerate(calls):
        a.set_bone_transforms(ids, ms)
        want = pal.set(ids, ms)
        assert bits_equal(a.geometry()[0][want[0]], want[1]) and bits_equal(a.geometry()[1][want[0]], want[2]), i
        b.set_geometry(*want)
        assert_twins(a, b, i)
    assert bits_equal(pal.matrices, np.stack([m(0, 3), m(1, 1), m(2, 3), m(3, 1), m(4, 2)]))


# ---- 5. frames in flight --------------------------------------------------------------------------------------------------------------------------
N_LEAD, N_EDITED = 4, 12             # twelve poses: more than the staging ring's four buffers and the version ring's eight slots
FLIGHT = [("cornell", "box_lamp"), (SPONZA, "lamps")]


def flight_pose(name, key, f):
    n = sk.skin_of(name, key).num_bones
    return sk.pose(name, key, f, None if f % 2 == 0 else [f % n, (f + 1) % n])


@functools.lru_cache(maxsize=None)
@with_libm
def oracle_flight(name, key):
    from restir_amd import capi
    o = sk.OracleSide(capi, name, key, W, H)
    out = []
    for f in range(N_LEAD + N_EDITED):
        if f >= N_LEAD:
            o.set_bone_transforms(*flight_pose(name, key, f))
        o.r.frame(3)
        out.append(o.image())
    return out, o.direct_state()


@pytest.mark.parametrize("side_stream", [4, 0], ids=["overlapped", "no_side_streams"])
@pytest.mark.parametrize("name,key", FLIGHT)
def test_twelve_frames_with_a_pose_in_every_gap(hip, name, key, side_stream):
    """rs_set_sync(0): four frames, then twelve with a pose before each (both skins list emitters), no rs_synchronize in between; every
    frame's image is copied device to device and read at the end.  Frame f equals the oracle's after the same f poses: a skinning kernel
    that ran before an earlier frame had finished with the staging buffer, or a refit that read records the kernel had not written yet,
    would not."""
    import torch
    ref, final = oracle_flight(name, key)
    assert all(differing(ref[f], ref[f + 1]) > 0 for f in range(N_LEAD - 1, N_LEAD + N_EDITED - 1))
    hip.set_side_stream(side_stream)
    h = sk.HipSide(hip, name, key, W, H)
    outs = [torch.zeros((W * H, 3), dtype=torch.float32, device="cuda") for _ in range(N_LEAD + N_EDITED)]
    hip.set_sync(False)
    try:
        r = h.r
        for f in range(N_LEAD + N_EDITED):
            if f >= N_LEAD:
                h.set_bone_transforms(*flight_pose(name, key, f))
            r.gbuf.render(r.scene, r.cam)
            r.restir.direct(r.scene, r.cam, r.gbuf, r.image.data_ptr(), 0, r.looper, 3)
            r.looper += 1
            r.gbuf.update(r.cam)
            hip.hip_memcpy_d2d_async(outs[f].data_ptr(), r.image.data_ptr(), W * H * 12)
        hip.synchronize()
    finally:
        hip.set_sync(True)
        hip.set_side_stream(4)
    for f in range(N_LEAD + N_EDITED):
        got = outs[f].cpu().numpy()
        assert bits_equal(ref[f], got), (f, differing(ref[f], got))
    h.r.rays = h.r.restir.ray_count()
    assert_same(final, h.direct_state(), "final")


# ---- 6. motion vectors ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,key", [("cornell", "box_lamp"), (SPONZA, "t386")])
def test_motion_vectors_follow_a_pose(hip, name, key):
    """A tracked scene: a frame, then twice advance, pose, frame.  The motion plane (and everything that reads it) equals the oracle's for
    the pose at the advance, and rs_scene_download_prev_vertices returns that pose: the pose writes the current vertices alone."""
    sd = scene_data(name)
    o, h = mv.OracleMotion(hip, sd, pipeline="indirect"), mv.HipMotion(hip, sd, pipeline="indirect")      # (ReSTIR-GI reads the plane; bit for bit)
    sk.skin_of(name, key).define(h.scene)
    pal = sk.Palette(hip, name, key)
    try:
        assert_same(o.frame(), h.frame(), (name, "at rest"))
        for step in (0, 1):
            before = h.scene.geometry()[0]
            o.advance(); h.advance()
            ids, ms = sk.pose(name, key, step)
            o.set_geometry(*pal.set(ids, ms))
            h.scene.set_bone_transforms(ids, ms)
            assert bits_equal(h.scene.prev_vertices(), before), (name, step)
            a, b = o.frame(), h.frame()
            assert_same(a, b, (name, step))
            assert differing(o.camera_only, a["motion"]) > 0, "the skin is in view: the plane is not the camera-only one"
    finally:
        h.destroy()


# ---- 7. row bands -----------------------------------------------------------------------------------------------------------------------------------
def test_row_bands_with_a_pose(hip):
    """rs_restir_phase_a / _phase_b on two bands, a pose between frames: the banded library equals the oracle's full frame."""
    name, key = "cornell", "box_lamp"
    bands = [(0, 19), (19, H)]
    o, h = sk.OracleSide(hip, name, key, W, H), sk.HipSide(hip, name, key, W, H)
    for f in range(5):
        if f in (2, 3):
            call = sk.pose(name, key, f) if f == 2 else sk.pose(name, key, f, [1])
            o.set_bone_transforms(*call); h.set_bone_transforms(*call)
        o.r.frame(3)
        r = h.r
        r.gbuf.render(r.scene, r.cam)
        for y0, y1 in bands:
            r.restir.phase_a(r.scene, r.cam, r.gbuf, r.looper, 3, y0, y1)
        for y0, y1 in bands:
            r.restir.phase_b(r.scene, r.cam, r.gbuf, r.image.data_ptr(), 0, 3, y0, y1)
        r.restir.end_frame()
        r.looper = next_looper(r.looper, None)
        r.gbuf.update(r.cam)
        r.rays = r.restir.ray_count()
        a, b = o.direct_state(), h.direct_state()
        a.pop("rays"); b.pop("rays")                     # (the banded launches count their rays per band)
        assert_same(a, b, f)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_scene_definition_and_palette_unchanged(hip):
    """Both scenes stand at the pose of step 0: `h` through its skin, the twin through rs_scene_set_geometry.  Every refused call leaves
    h's tables, host description, frames, definition -- and palette: the refused poses name bone 1 with a good new matrix next to the
    offending one, and the accepted pose of the lamp's bone alone at the end shows bones 0 and 1 where step 0 left them."""
    import torch
    name, key = "cornell", "box_lamp"
    sd, skin = scene_data(name), sk.skin_of(name, key)
    h, twin = sk.HipSide(hip, name, key, W, H), HipRenderer(hip, sd, W, H)
    s = h.r.scene
    pal = sk.Palette(hip, name, key)
    s.set_bone_transforms(*sk.pose(name, key, 0))
    twin.scene.set_geometry(*pal.set(*sk.pose(name, key, 0)))
    desc, tables, grid = twin.scene.host_desc(), all_tables(twin.scene), repr(twin.scene.emissive_grid())
    L = hip.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lo, hi = root_box(sd.vertices)
    out_of_box = pt.translation((-(hi[0] - lo[0]) * 0.45, 0.0, 0.0))           # the tall box's base through the left wall
    singular = pt.from_rows(np.diag([1.0, 0.0, 1.0, 1.0]))
    nan = pt.identity(); nan[3, 1] = np.nan
    good = sk.bone_matrix(name, key, 1, 5)
    one, ident = np.array([1], np.int32), pt.identity()
    ids, bid, wts, rv, rn = skin.ids, skin.bone_ids, skin.weights, skin.rest_vertices, skin.rest_normals

    def changed(a, where, value):
        a = a.copy()
        a[where] = value
        return a

    def define_raw(bones, listed, prim=ids, v=None, n=None, b=bid, w=wts, scene=None):
        hip.check(L.rs_scene_define_skin(s.handle if scene is None else scene, bones, listed, None if prim is None else ptr(prim),
                                         None if v is None else ptr(v), None if n is None else ptr(n), None if b is None else ptr(b),
                                         None if w is None else ptr(w)))
    nl = len(ids)
    cases = [
        ("a vertex leaves the root box", lambda: s.set_bone_transforms([1, 0], [good, out_of_box])),
        ("a singular matrix", lambda: s.set_bone_transforms([1, 2], [good, singular])),
        ("a NaN entry", lambda: s.set_bone_transforms([0, 1], [nan, good])),
        ("bone id beyond", lambda: s.set_bone_transforms([1, skin.num_bones], [good, ident])),
        ("bone id below", lambda: s.set_bone_transforms([1, -1], [good, ident])),
        ("null bone ids", lambda: hip.check(L.rs_scene_set_bone_transforms(s.handle, 1, None, ptr(good)))),
        ("null matrices", lambda: hip.check(L.rs_scene_set_bone_transforms(s.handle, 1, ptr(one), None))),
        ("negative count", lambda: hip.check(L.rs_scene_set_bone_transforms(s.handle, -1, ptr(one), ptr(good)))),
        ("null scene", lambda: hip.check(L.rs_scene_set_bone_transforms(None, 1, ptr(one), ptr(good)))),
        # (a light sampler left without power: test_a_pose_that_leaves_no_light_power_is_refused below, on a skin whose corners have bones
        # of their own -- on this one the lamp follows one bone, and a matrix that takes its area to 0 is singular)
        ("define: 257 bones", lambda: define_raw(257, nl)),
        ("define: negative bones", lambda: define_raw(-1, nl)),
        ("define: negative count", lambda: define_raw(3, -1)),
        ("define: triangles without a bone", lambda: define_raw(0, nl)),
        ("define: a primitive twice", lambda: define_raw(3, nl, changed(ids, 3, ids[0]))),
        ("define: an id beyond", lambda: define_raw(3, nl, changed(ids, 2, len(sd.material_ids)))),
        ("define: an id below", lambda: define_raw(3, nl, changed(ids, 2, -1))),
        ("define: null ids", lambda: define_raw(3, nl, None)),
        ("define: null bone ids", lambda: define_raw(3, nl, b=None)),
        ("define: null weights", lambda: define_raw(3, nl, w=None)),
        ("define: rest vertices alone", lambda: define_raw(3, nl, v=rv)),
        ("define: rest normals alone", lambda: define_raw(3, nl, n=rn)),
        ("define: a rest vertex that is not finite", lambda: define_raw(3, nl, v=changed(rv, (3, 1, 2), np.inf), n=rn)),
        ("define: a rest normal that is not finite", lambda: define_raw(3, nl, v=rv, n=changed(rn, (0, 0, 0), np.nan))),
        ("define: a weight that is NaN", lambda: define_raw(3, nl, w=changed(wts, (2, 1, 0), np.nan))),
        ("define: a weight that is infinite", lambda: define_raw(3, nl, w=changed(wts, (2, 1, 0), np.inf))),
        ("define: a negative weight", lambda: define_raw(3, nl, w=changed(wts, (2, 1, 0), -0.25))),
        ("define: a corner without weight", lambda: define_raw(3, nl, w=changed(wts, (5, 2), 0.0))),
        ("define: a bone id beyond", lambda: define_raw(3, nl, b=changed(bid, (4, 0, 3), 3))),
        ("define: a bone id below, at weight 0", lambda: define_raw(3, nl, b=changed(bid, (nl - 1, 0, 0), -1))),
        ("define: null scene", lambda: define_raw(3, nl, scene=C.c_void_p())),
    ]

    def unchanged(tag):
        assert_desc_equal(s.host_desc(), desc, tag)
        assert_tables_equal(all_tables(s), tables, tag)
        assert repr(s.emissive_grid()) == grid, tag
        assert_definition(s, skin, tag)
        a, b = twin.frame(3), h.r.frame(3)
        assert bits_equal(a, b), tag
        ga, gb = twin.gbuf.download(), h.r.gbuf.download()
        for k in ("prim_id", "normal", "depth", "albedo", "motion"):
            assert bits_equal(np.asarray(ga[k]), np.asarray(gb[k])), (tag, k)
        assert twin.rays == h.r.rays, tag
    for tag, call in cases:
        refused(hip, INVALID, call)
        unchanged(tag)
    bare = hip_scene(hip, sd)                            # no skin defined
    refused(hip, INVALID, bare.set_bone_transforms, [0], [ident])
    refused(hip, INVALID, bare.download_skin)

    # while the library stream is being captured into a graph: RS_ERR_UNSUPPORTED, as tests/test_gpu_geometry_edits.py has it for rs_scene_set_triangles
    rt = C.CDLL("libamdhip64.so")
    rt.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    rt.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    rt.hipGraphDestroy.argtypes = [C.c_void_p]
    stream = torch.cuda.Stream()
    hip.synchronize()
    hip.set_stream(stream.cuda_stream)
    graph = C.c_void_p()
    try:
        assert rt.hipStreamBeginCapture(stream.cuda_stream, 2) == 0           # hipStreamCaptureModeRelaxed
        try:
            refused(hip, UNSUPPORTED, s.set_bone_transforms, [1], [good])
            refused(hip, UNSUPPORTED, skin.define, s)
            refused(hip, UNSUPPORTED, s.download_skin)
        finally:
            assert rt.hipStreamEndCapture(stream.cuda_stream, C.byref(graph)) == 0
            if graph:
                rt.hipGraphDestroy(graph)
    finally:
        hip.set_stream(None)
    unchanged("during capture")
    # ... and the scene still takes a pose: the lamp's bone alone; bones 0 and 1 are where step 0 left them
    lamp = sk.pose(name, key, 3, [2])
    s.set_bone_transforms(*lamp)
    want = pal.set(*lamp)
    assert bits_equal(pal.matrices[1], sk.bone_matrix(name, key, 1, 0))
    assert bits_equal(s.geometry()[0][want[0]], want[1]) and bits_equal(s.geometry()[1][want[0]], want[2])
    twin.scene.set_geometry(*want)
    assert_tables_equal(all_tables(s), all_tables(twin.scene), "the accepted pose after the refusals")


def test_a_pose_that_leaves_no_light_power_is_refused(hip):
    """The refusal no rigid part reaches, and the one that comes last in the edit: after the refit's tables and the version ring have been
    prepared, from the plan of the lights.  On the skin whose lamp corners have bones of their own, plain translations put the lamp's six
    corners on one line (tests/skinning.py collapse_pose): every value finite, every vertex inside the root box, both emitters -- the
    scene's only ones -- without area.  Both scenes stand at the pose of step 0, the first edit of either; the pose is then refused on a
    scene whose FIRST edit it would be as well.  The refused pose names the box's bone with a good new matrix alongside; tables, host
    description, emissive grid, frames, definition and counters stay, rs_scene_set_geometry refuses the same arrays with the same words,
    and the accepted pose of one lamp corner's bone afterwards shows the box's bone, and the other five, where step 0 left them."""
    name, key = "cornell", sk.LAMP_CORNERS
    sd, skin = scene_data(name), sk.skin_of(name, key)
    bones, ms, ids, v, n = sk.collapse_pose(hip)
    good = sk.bone_matrix(name, key, 6, 5)
    call = (np.concatenate([[6], bones]), np.concatenate([good[None], ms]))
    words = "without a finite, positive total power"

    def refused_for_power(fn, *args):
        with pytest.raises(hip.RestirHipError) as e:
            fn(*args)
        assert str(e.value).startswith("librestir_hip error %d:" % INVALID) and words in str(e.value), str(e.value)

    # a scene that has seen no edit yet: the refusal leaves it a scene without one
    fresh, bare = skinned_scene(hip, name, key), hip_scene(hip, sd)
    refused_for_power(fresh.set_bone_transforms, *call)
    assert_tables_equal(all_tables(fresh), all_tables(bare), "first edit refused")
    assert_desc_equal(fresh.host_desc(), bare.host_desc(), "first edit refused")
    assert (fresh.geometry_edits(), fresh.light_moves(), fresh.refit_counts(), fresh.staged_bytes()) == (0, 0, (0, 0), 0)

    h, twin = sk.HipSide(hip, name, key, W, H), HipRenderer(hip, sd, W, H)
    s = h.r.scene
    pal = sk.Palette(hip, name, key)
    s.set_bone_transforms(*sk.pose(name, key, 0))
    twin.scene.set_geometry(*pal.set(*sk.pose(name, key, 0)))
    desc, tables, grid = twin.scene.host_desc(), all_tables(twin.scene), repr(twin.scene.emissive_grid())
    counters = s.geometry_edits(), s.light_moves(), s.refit_counts(), s.staged_bytes(), s.dirty_boxes(0)[0].tobytes()
    assert counters[:4] == (1, 1, (1, 0), 7 * BONE_BYTES)

    def unchanged(tag):
        assert_desc_equal(s.host_desc(), desc, tag)
        assert_tables_equal(all_tables(s), tables, tag)
        assert repr(s.emissive_grid()) == grid, tag
        assert_definition(s, skin, tag)
        assert (s.geometry_edits(), s.light_moves(), s.refit_counts(), s.staged_bytes(), s.dirty_boxes(0)[0].tobytes()) == counters, tag
        assert bits_equal(twin.frame(3), h.r.frame(3)), tag
        ga, gb = twin.gbuf.download(), h.r.gbuf.download()
        for k in ("prim_id", "normal", "depth", "albedo", "motion"):
            assert bits_equal(np.asarray(ga[k]), np.asarray(gb[k])), (tag, k)
        assert twin.rays == h.r.rays, tag
    for partial in (False, True):                        # (the switch decides nothing before the refusal)
        s.set_partial_refit(partial)
        refused_for_power(s.set_bone_transforms, *call)
        unchanged(("no light power", partial))
    refused_for_power(s.set_bone_transforms, bones, ms)  # ... and without the good matrix alongside
    unchanged("no light power, the corner bones alone")
    refused_for_power(twin.scene.set_geometry, ids, v, n)
    s.set_partial_refit(False)
    # the palette is where step 0 left it: one corner's bone moves (a shear of the lamp, not a collapse), nothing else
    one = (np.array([2], np.int32), pt.translation((0.05, -0.01, 0.0))[None])
    s.set_bone_transforms(*one)
    want = pal.set(*one)
    assert bits_equal(pal.matrices[6], sk.bone_matrix(name, key, 6, 0)) and not bits_equal(pal.matrices[6], good)
    assert bits_equal(s.geometry()[0][want[0]], want[1]) and bits_equal(s.geometry()[1][want[0]], want[2])
    twin.scene.set_geometry(*want)
    assert_tables_equal(all_tables(s), all_tables(twin.scene), "the accepted pose after the refusals")
    assert_desc_equal(s.host_desc(), twin.scene.host_desc(), "the accepted pose after the refusals")
    assert bits_equal(twin.frame(3), h.r.frame(3))
