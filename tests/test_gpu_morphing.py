"""Morph targets (rs_scene_define_morph, rs_scene_define_skin_morph, rs_scene_set_morph_weights, rs_scene_set_skin_pose) bit for bit:
against the CPU oracle on the arrays rs_morph_corners gives (host only; tests/test_morphing_host.py holds it to a NumPy restatement), and
against a second library scene edited by rs_scene_set_geometry with the same arrays -- every device table, the emissive grid, the host
description.  Corner counts on either side of a wave and of a block, target counts on either side of a weight record, a corner with 256
entries next to corners with none, the device's by-corner table, morph under a skin, frames in flight, motion vectors, row bands,
refusals.  No comparison has a tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import binding as ob
from tests import morphing as mo
from tests import motion_vectors as mv
from tests import part_transforms as pt
from tests import skinning as sk
from tests.common import HipRenderer, bits_equal, hip_scene, next_looper, oracle_scene
from tests.emitter_edits import edited_oracle_scene, emitters, scene_data
from tests.geometry_edits import apply_triangles, probe_rays, probe_segments
from tests.scene_edits import assert_same, differing
from tests.test_gpu_part_transforms import (H, INVALID, N_RAYS, N_SEGMENTS, SPONZA, UNSUPPORTED, W, all_tables, assert_desc_equal,
                                            assert_tables_equal, hip_outputs, oracle_outputs, refused, with_libm)
from tests.test_gpu_skinning import assert_twins

pytestmark = pytest.mark.gpu

F = np.float32
ALL_MORPHS = [(n, k) for n in mo.MORPHS for k in mo.MORPHS[n]]


@pytest.fixture(autouse=True)
def exact_libm(hip):
    ob.set_libm_mode(1)            # cos / sin correctly rounded on both sides: every bit must agree
    hip.set_sync(True)
    yield
    ob.set_libm_mode(0)
    hip.set_sync(True)
    hip.set_side_stream(4)         # the library's default


def morphed_scene(hip, name, key):
    s = hip_scene(hip, scene_data(name))
    mo.morph_of(name, key).define(s)
    return s


def emitters_in(name, key):
    return int(np.isin(mo.morph_of(name, key).ids, emitters(scene_data(name))).sum())


# ---- 1. outputs after a weight step ---------------------------------------------------------------------------------------------------------
OUTPUT_CASES = [("cornell", "box_lamp"), (SPONZA, "t22"), (SPONZA, "t386")]


@functools.lru_cache(maxsize=None)
def expected_after(name, key):
    """(vertices, normals) after weight step 0, from rs_morph_corners alone; the places triangles moved from and to."""
    from restir_amd import capi
    sd = scene_data(name)
    m = mo.morph_of(name, key)
    v, n = sd.vertices.reshape(-1, 3, 3).copy(), sd.normals.reshape(-1, 3, 3).copy()
    ids, sv, sn = mo.Weights(capi, m).set(*mo.weight_step(m.num_targets, 0)).morphed()
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
def test_outputs_after_weight_step(hip, name, key):
    """One step of every weight.  The host description then holds rs_morph_corners of the rest pose on the listed triangles and the old
    bits elsewhere; the device's vertices and normals equal it; closest-hit and occlusion probes, the G-buffer planes and three
    ReSTIRDirect frames with reuse 3, and rs_path_trace at depth 3 equal the oracle's on a fresh scene made from those arrays."""
    sd, m = scene_data(name), mo.morph_of(name, key)
    v_want, n_want, _ = expected_after(name, key)
    s = morphed_scene(hip, name, key)
    s.set_morph_weights(*mo.weight_step(m.num_targets, 0))
    v_got, n_got = s.geometry()
    assert bits_equal(v_got, v_want) and bits_equal(n_got, n_want)
    moved = np.sort(m.ids.astype(np.int64))
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


# ---- 2. the same as rs_scene_set_geometry -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("partial", [False, True], ids=["whole", "partial"])
@pytest.mark.parametrize("name,key", ALL_MORPHS)
def test_same_as_set_geometry(hip, name, key, partial):
    """Two scenes from one description, one edited by rs_scene_set_morph_weights, the other by rs_scene_set_geometry with the arrays of
    rs_morph_corners, three steps over (all targets; every third; every weight 0 but one): assert_twins of tests/test_gpu_skinning.py --
    every table of rs_debug_scene_table byte for byte, the emissive grid, the host description, light moves, dirty boxes, refit counts.
    Each step stages ceil(numTargets / 28) records of 112 bytes."""
    sd, m = scene_data(name), mo.morph_of(name, key)
    a, b = morphed_scene(hip, name, key), hip_scene(hip, sd)
    if partial:
        a.set_partial_refit(True)
        b.set_partial_refit(True)
    lamps = emitters_in(name, key)
    assert (lamps > 0) == (key == "box_lamp")
    assert a.morph_info() == (m.num_targets, len(m.ids), len(m.entry_corner)) and a.staged_bytes() == 0
    w = mo.Weights(hip, m)
    for step in (0, 1, 2):
        ids, ws = mo.weight_step(m.num_targets, step)
        a.set_morph_weights(ids, ws)
        assert a.staged_bytes() == mo.staged_bytes(m.num_targets), (name, key, step)
        b.set_geometry(*w.set(ids, ws).morphed())
        assert_twins(a, b, (name, key, step))
        assert a.refit_counts() == ((1, step) if partial else (step + 1, 0)), (name, key, step)
        assert a.light_moves() == (step + 1 if lamps else 0)
    assert np.count_nonzero(w.w) == 1


# ---- 3. the device's by-corner table, the rest arrays, no drift ---------------------------------------------------------------------------------
def assert_definition(s, m, tag, which=0):
    got = s.download_morph(which)
    first, recs = mo.by_corner(m.num_corners, *m.table())
    assert np.array_equal(got[0], first), tag
    assert got[1].dtype == recs.dtype and got[1].tobytes() == recs.tobytes(), tag
    if which == 0:
        assert np.array_equal(got[2], m.ids) and bits_equal(got[3], m.rest_vertices) and bits_equal(got[4], m.rest_normals), tag
    assert s.morph_info(which) == (m.num_targets, m.num_corners // 3, len(m.entry_corner)), tag


@pytest.mark.parametrize("name,key", [("cornell", "box_lamp"), (SPONZA, "t22"), (SPONZA, "t386")])
def test_device_table_and_rest_arrays(hip, name, key):
    """rs_scene_download_morph against the restated conversion, record by record, after the definition and after ten edits; the tenth
    edit's geometry equals rs_morph_corners of the weights as they then stand (no drift); count == 0 changes nothing."""
    m = mo.morph_of(name, key)
    s = hip_scene(hip, scene_data(name))
    assert s.morph_info() == (0, 0, 0)
    m.define(s)
    assert_definition(s, m, "defined")
    if m.num_corners >= mo.FULL_FROM:
        first = s.download_morph()[0]
        assert first[mo.FULL_CORNER + 1] - first[mo.FULL_CORNER] == m.num_targets
        assert first[mo.FULL_CORNER + 1 + mo.EMPTY_CORNERS] == first[mo.FULL_CORNER + 1]
    w = mo.Weights(hip, m)
    for step in range(10):
        call = mo.weight_step(m.num_targets, step)
        s.set_morph_weights(*call)
        w.set(*call)
    assert_definition(s, m, "after ten edits")
    ids, v, n = w.morphed()
    assert bits_equal(s.geometry()[0][ids], v) and bits_equal(s.geometry()[1][ids], n)
    assert bits_equal(s.debug_table("vertices"), s.geometry()[0])
    before = s.geometry()[0]
    s.set_morph_weights([], [])
    assert bits_equal(s.geometry()[0], before) and s.geometry_edits() == 10
    # all weights 0: the rest pose, bit for bit
    s.set_morph_weights(np.arange(m.num_targets), np.zeros(m.num_targets, F))
    assert bits_equal(s.geometry()[0][ids], m.rest_vertices) and bits_equal(s.geometry()[1][ids], m.rest_normals)
    # dropped
    s.define_morph([], [0], [], np.zeros((0, 3), F))
    assert s.morph_info() == (0, 0, 0)
    refused(hip, INVALID, s.set_morph_weights, [0], [0.5])


# ---- 4. morph under a skin ---------------------------------------------------------------------------------------------------------------------
def skin_morphed_scene(hip, key):
    s = hip_scene(hip, scene_data(SPONZA))
    sk.skin_of(SPONZA, key).define(s)
    mo.skin_morph_of(key).define_on_skin(s)
    return s


@pytest.mark.parametrize("key", list(mo.SKIN_MORPHS))
def test_morph_under_a_skin_same_as_set_geometry(hip, key):
    """rs_scene_set_skin_pose naming bones and targets against a twin edited by rs_scene_set_geometry with
    rs_skin_corners(rs_morph_corners(rest)); one edit a step, numBones + ceil(numTargets / 28) records staged.  Then
    rs_scene_set_bone_transforms alone keeps the weights, and a pose of weights alone keeps the palette."""
    skin, m = sk.skin_of(SPONZA, key), mo.skin_morph_of(key)
    a, b = skin_morphed_scene(hip, key), hip_scene(hip, scene_data(SPONZA))
    a.set_partial_refit(True)
    b.set_partial_refit(True)
    assert_definition(a, m, "defined", which=1)
    pose = mo.SkinPose(hip, key)
    for step in (0, 1, 2):
        bones, targets = sk.pose(SPONZA, key, step), mo.weight_step(m.num_targets, step)
        a.set_skin_pose(*bones, *targets)
        assert a.staged_bytes() == mo.staged_bytes(m.num_targets, skin.num_bones)
        b.set_geometry(*pose.set(*bones, *targets))
        assert_twins(a, b, (key, step))
        assert a.geometry_edits() == step + 1
    bones = sk.pose(SPONZA, key, 3, [0])
    a.set_bone_transforms(*bones)
    assert a.staged_bytes() == mo.staged_bytes(m.num_targets, skin.num_bones)
    b.set_geometry(*pose.set(*bones, [], []))
    assert_twins(a, b, (key, "bones alone"))
    assert np.count_nonzero(pose.weights.w) == 1         # (step 2 left one weight; the bones alone kept it: the twins agree)
    targets = mo.weight_step(m.num_targets, 4)
    a.set_skin_pose([], np.zeros((0, 4, 4), F), *targets)
    b.set_geometry(*pose.set([], [], *targets))
    assert_twins(a, b, (key, "weights alone"))
    assert_definition(a, m, "after five poses", which=1)


@pytest.mark.parametrize("key", ["t22", "t386"])
def test_all_weights_zero_equals_the_plain_skin(hip, key):
    """With every weight 0 the fused kernel writes what k_skin writes: table for table a twin that has the plain skin and
    rs_scene_set_bone_transforms -- which on that twin stages numBones records and nothing more."""
    skin = sk.skin_of(SPONZA, key)
    a, b = skin_morphed_scene(hip, key), hip_scene(hip, scene_data(SPONZA))
    skin.define(b)
    for step in (0, 1):
        bones = sk.pose(SPONZA, key, step)
        a.set_bone_transforms(*bones) if step else a.set_skin_pose(*bones, [0], [0.0])
        b.set_bone_transforms(*bones)
        assert b.staged_bytes() == skin.num_bones * 112 and a.staged_bytes() == mo.staged_bytes(mo.SKIN_MORPHS[key], skin.num_bones)
        assert_twins(a, b, (key, step))
    refused(hip, INVALID, b.set_skin_pose, *sk.pose(SPONZA, key, 2), [0], [0.5])      # targets on a skin without a morph
    b.set_skin_pose(*sk.pose(SPONZA, key, 2), [], [])                                  # ... none named: rs_scene_set_bone_transforms
    a.set_skin_pose(*sk.pose(SPONZA, key, 2), [], [])
    assert b.staged_bytes() == skin.num_bones * 112
    assert_twins(a, b, (key, "no target named"))


def test_redefining_or_dropping_the_skin_drops_its_morph(hip):
    key = "t22"
    s = skin_morphed_scene(hip, key)
    m = mo.skin_morph_of(key)
    assert s.morph_info(1) == (m.num_targets, 22, len(m.entry_corner)) and s.morph_info(0) == (0, 0, 0)
    sk.skin_of(SPONZA, key).define(s)
    assert s.morph_info(1) == (0, 0, 0) and s.skin_info() == (5, 22)
    refused(hip, INVALID, s.set_skin_pose, [0], [pt.identity()], [0], [0.5])
    m.define_on_skin(s)
    s.define_skin_morph([0], [], np.zeros((0, 3), F))                              # no target: the morph alone goes
    assert s.morph_info(1) == (0, 0, 0) and s.skin_info() == (5, 22)
    m.define_on_skin(s)
    s.define_skin(0, [], np.zeros((0, 3, 4), np.int32), np.zeros((0, 3, 4), F))
    assert s.morph_info(1) == (0, 0, 0) and s.skin_info() == (0, 0)
    refused(hip, INVALID, m.define_on_skin, s)                                     # a skin morph needs a skin
    # the scene's own morph and a skin's live side by side
    mo.morph_of(SPONZA, "t21").define(s)
    sk.skin_of(SPONZA, key).define(s)
    m.define_on_skin(s)
    assert s.morph_info(0)[0] == 2 and s.morph_info(1)[0] == m.num_targets


def test_a_refused_pose_leaves_palette_and_weights(hip):
    """The light-sampler refusal of tests/skinning.py collapse_pose, the last one an edit can meet, on the skin whose lamp corners have
    bones of their own and a morph of two targets over the tall box: the refused pose names a good new weight and a good new matrix next
    to the collapsing bones; tables, host description, palette and weights stay, and the accepted pose of one target afterwards shows
    bone 6 and target 0 where the first pose left them."""
    name, key = "cornell", sk.LAMP_CORNERS
    sd, skin = scene_data(name), sk.skin_of(name, key)
    bones, ms, _, _, _ = sk.collapse_pose(hip)
    corners = len(skin.ids) * 3
    box = np.arange(6, corners)                           # the lamp's six corners carry no entry: the collapse stays a collapse
    dp = np.concatenate([np.tile(np.array([[0.0, 0.02, 0.0]], F), (len(box), 1)), np.tile(np.array([[0.015, 0.0, 0.0]], F), (len(box), 1))])
    tab = (np.array([0, len(box), 2 * len(box)], np.int32), np.concatenate([box, box]).astype(np.int32), dp)
    m = mo.Morph(name, key, 2, corners, tab[0], tab[1], tab[2], np.zeros_like(tab[2]))
    a, b = hip_scene(hip, sd), hip_scene(hip, sd)
    skin.define(a)
    m.define_on_skin(a)
    pal, w = sk.Palette(hip, name, key), mo.Weights(hip, m)

    def posed():
        v, n = w.corners(skin.rest_vertices, skin.rest_normals)
        v, n = hip.skin_corners(pal.matrices, v, n, skin.bone_ids, skin.weights)
        return skin.ids, *mo.inside(name, v, n, "lamp corners")
    first = sk.pose(name, key, 0)
    a.set_skin_pose(*first, [0, 1], [1.0, 0.5])
    pal.set(*first)
    w.set([0, 1], [1.0, 0.5])
    b.set_geometry(*posed())
    assert_twins(a, b, "first pose")
    good = sk.bone_matrix(name, key, 6, 5)
    with pytest.raises(hip.RestirHipError) as e:
        a.set_skin_pose(np.concatenate([[6], bones]), np.concatenate([good[None], ms]), [0], [0.25])
    assert "without a finite, positive total power" in str(e.value) and "rs_scene_set_skin_pose" in str(e.value)
    assert_twins(a, b, "refused")
    refused(hip, INVALID, a.set_skin_pose, [6], [good], [1], [np.inf])
    refused(hip, INVALID, a.set_skin_pose, [6], [good], [2], [0.5])
    a.set_skin_pose([], np.zeros((0, 4, 4), F), [1], [0.75])
    w.set([1], [0.75])
    b.set_geometry(*posed())
    assert_twins(a, b, "the accepted pose after the refusals")


# ---- 5. frames in flight, motion vectors, row bands -------------------------------------------------------------------------------------------------
N_LEAD, N_EDITED = 4, 12             # twelve steps: more than the staging ring's four buffers and the version ring's eight slots
FLIGHT = ("cornell", "box_lamp")


def flight_step(f):
    return mo.weight_step(mo.morph_of(*FLIGHT).num_targets, f)


@functools.lru_cache(maxsize=None)
@with_libm
def oracle_flight():
    from restir_amd import capi
    o = mo.OracleSide(capi, *FLIGHT, W, H)
    out = []
    for f in range(N_LEAD + N_EDITED):
        if f >= N_LEAD:
            o.set_morph_weights(*flight_step(f))
        o.r.frame(3)
        out.append(o.image())
    return out, o.direct_state()


def test_twelve_frames_with_a_weight_step_in_every_gap(hip):
    """rs_set_sync(0): four frames, then twelve with a weight step before each (the morph lists the lamp), no rs_synchronize in between;
    every frame's image is copied device to device and read at the end.  Frame f equals the oracle's after the same f steps, and the
    reservoirs at the end equal the oracle's."""
    import torch
    ref, final = oracle_flight()
    assert all(differing(ref[f], ref[f + 1]) > 0 for f in range(N_LEAD - 1, N_LEAD + N_EDITED - 1))
    h = mo.HipSide(hip, *FLIGHT, W, H)
    outs = [torch.zeros((W * H, 3), dtype=torch.float32, device="cuda") for _ in range(N_LEAD + N_EDITED)]
    hip.set_sync(False)
    try:
        r = h.r
        for f in range(N_LEAD + N_EDITED):
            if f >= N_LEAD:
                h.set_morph_weights(*flight_step(f))
            r.gbuf.render(r.scene, r.cam)
            r.restir.direct(r.scene, r.cam, r.gbuf, r.image.data_ptr(), 0, r.looper, 3)
            r.looper += 1
            r.gbuf.update(r.cam)
            hip.hip_memcpy_d2d_async(outs[f].data_ptr(), r.image.data_ptr(), W * H * 12)
        hip.synchronize()
    finally:
        hip.set_sync(True)
    for f in range(N_LEAD + N_EDITED):
        got = outs[f].cpu().numpy()
        assert bits_equal(ref[f], got), (f, differing(ref[f], got))
    h.r.rays = h.r.restir.ray_count()
    assert_same(final, h.direct_state(), "final")


def test_motion_vectors_follow_a_weight_step(hip):
    """A tracked scene: a frame, then twice advance, weight step, frame.  The motion plane equals the oracle's for the pose at the
    advance, and rs_scene_download_prev_vertices returns that pose: the step writes the current vertices alone."""
    name, key = FLIGHT
    sd, m = scene_data(name), mo.morph_of(name, key)
    o, h = mv.OracleMotion(hip, sd, pipeline="indirect"), mv.HipMotion(hip, sd, pipeline="indirect")
    m.define(h.scene)
    w = mo.Weights(hip, m)
    try:
        assert_same(o.frame(), h.frame(), (name, "at rest"))
        for step in (0, 1):
            before = h.scene.geometry()[0]
            o.advance(); h.advance()
            ids, ws = mo.weight_step(m.num_targets, step)
            call = ids, ws * F(4.0)                      # weights up to 6: far enough to cross pixels at this resolution
            o.set_geometry(*w.set(*call).morphed())
            h.scene.set_morph_weights(*call)
            assert bits_equal(h.scene.prev_vertices(), before), step
            a, b = o.frame(), h.frame()
            assert_same(a, b, (name, step))
            assert differing(o.camera_only, a["motion"]) > 0, "the morph is in view: the plane is not the camera-only one"
    finally:
        h.destroy()


def test_row_bands_with_a_weight_step(hip):
    """rs_restir_phase_a / _phase_b on two bands, a weight step between frames: the banded library equals the oracle's full frame."""
    bands = [(0, 19), (19, H)]
    o, h = mo.OracleSide(hip, *FLIGHT, W, H), mo.HipSide(hip, *FLIGHT, W, H)
    for f in range(5):
        if f in (2, 3):
            call = flight_step(f - 2)
            o.set_morph_weights(*call); h.set_morph_weights(*call)
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


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_scene_definition_and_weights_unchanged(hip):
    """Both scenes stand at weight step 0: `h` through its morph, the twin through rs_scene_set_geometry.  Every refused call leaves h's
    tables, host description, frames, definition and weights; the accepted step of one target at the end shows the others where step 0
    left them."""
    import torch
    name, key = "cornell", "box_lamp"
    sd, m = scene_data(name), mo.morph_of(name, key)
    h, twin = mo.HipSide(hip, name, key, W, H), HipRenderer(hip, sd, W, H)
    s = h.r.scene
    w = mo.Weights(hip, m)
    step0 = mo.weight_step(m.num_targets, 0)
    s.set_morph_weights(*step0)
    twin.scene.set_geometry(*w.set(*step0).morphed())
    desc, tables, grid = twin.scene.host_desc(), all_tables(twin.scene), repr(twin.scene.emissive_grid())
    L = hip.lib()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    one, half = np.array([1], np.int32), np.array([0.5], F)
    first, ec, dp, dn = m.table()
    ids, rv, rn = m.ids, m.rest_vertices, m.rest_normals
    nl, nt = len(ids), m.num_targets

    def changed(a, where, value):
        a = a.copy()
        a[where] = value
        return a

    def define_raw(targets=nt, listed=nl, prim=ids, v=None, n=None, first=first, ec=ec, dp=dp, dn=dn, scene=None):
        hip.check(L.rs_scene_define_morph(s.handle if scene is None else scene, targets, listed, ptr(prim), ptr(v), ptr(n), ptr(first), ptr(ec),
                                          ptr(dp), ptr(dn)))
    twice = changed(ec, first[1] + 1, ec[first[1]])      # a corner twice in target 1
    cases = [
        ("a vertex leaves the root box", lambda: s.set_morph_weights([1, 0], [0.5, 1e4])),
        ("a weight that is NaN", lambda: s.set_morph_weights([1, 0], [0.5, np.nan])),
        ("a weight that is infinite", lambda: s.set_morph_weights([1, 0], [0.5, -np.inf])),
        ("target id beyond", lambda: s.set_morph_weights([1, nt], [0.5, 0.5])),
        ("target id below", lambda: s.set_morph_weights([1, -1], [0.5, 0.5])),
        ("null target ids", lambda: hip.check(L.rs_scene_set_morph_weights(s.handle, 1, None, ptr(half)))),
        ("null weights", lambda: hip.check(L.rs_scene_set_morph_weights(s.handle, 1, ptr(one), None))),
        ("negative count", lambda: hip.check(L.rs_scene_set_morph_weights(s.handle, -1, ptr(one), ptr(half)))),
        ("skin pose without a skin", lambda: s.set_skin_pose([0], [pt.identity()], [0], [0.5])),
        ("skin morph without a skin", lambda: s.define_skin_morph(first, ec, dp, dn)),
        ("define: 257 targets", lambda: define_raw(257, first=np.zeros(258, np.int32))),
        ("define: negative targets", lambda: define_raw(-1)),
        ("define: negative count", lambda: define_raw(listed=-1)),
        ("define: triangles without a target", lambda: define_raw(0)),
        ("define: a primitive twice", lambda: define_raw(prim=changed(ids, 3, ids[0]))),
        ("define: an id beyond", lambda: define_raw(prim=changed(ids, 2, len(sd.material_ids)))),
        ("define: null ids", lambda: define_raw(prim=None)),
        ("define: rest vertices alone", lambda: define_raw(v=rv)),
        ("define: rest normals alone", lambda: define_raw(n=rn)),
        ("define: a rest vertex that is not finite", lambda: define_raw(v=changed(rv, (3, 1, 2), np.inf), n=rn)),
        ("define: null offsets", lambda: define_raw(first=None)),
        ("define: offsets that start at 1", lambda: define_raw(first=changed(first, 0, 1))),
        ("define: offsets that decrease", lambda: define_raw(first=changed(first, 1, first[2] + 1))),
        ("define: null corners", lambda: define_raw(ec=None)),
        ("define: null position deltas", lambda: define_raw(dp=None)),
        ("define: a corner beyond", lambda: define_raw(ec=changed(ec, 4, nl * 3))),
        ("define: a corner below", lambda: define_raw(ec=changed(ec, 4, -1))),
        ("define: a (target, corner) pair twice", lambda: define_raw(ec=twice)),
        ("define: a position delta that is NaN", lambda: define_raw(dp=changed(dp, (2, 1), np.nan))),
        ("define: a normal delta that is infinite", lambda: define_raw(dn=changed(dn, (5, 0), np.inf))),
        ("info: which = 2", lambda: s.morph_info(2)),
        ("download: the skin's, without one", lambda: s.download_morph(1)),
    ]

    def unchanged(tag):
        assert_desc_equal(s.host_desc(), desc, tag)
        assert_tables_equal(all_tables(s), tables, tag)
        assert repr(s.emissive_grid()) == grid, tag
        assert_definition(s, m, tag)
        assert bits_equal(twin.frame(3), h.r.frame(3)), tag
        assert twin.rays == h.r.rays, tag
    assert first[2] - first[1] >= 2 and ec[first[1]] != ec[first[1] + 1]
    for tag, call in cases:
        refused(hip, INVALID, call)
        unchanged(tag)
    bare = hip_scene(hip, sd)                            # no morph defined
    refused(hip, INVALID, bare.set_morph_weights, [0], [0.5])
    refused(hip, INVALID, bare.download_morph)

    # while the library stream is being captured into a graph: RS_ERR_UNSUPPORTED, as tests/test_gpu_skinning.py has it
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
            refused(hip, UNSUPPORTED, s.set_morph_weights, [1], [0.5])
            refused(hip, UNSUPPORTED, m.define, s)
            refused(hip, UNSUPPORTED, s.download_morph)
        finally:
            assert rt.hipStreamEndCapture(stream.cuda_stream, C.byref(graph)) == 0
            if graph:
                rt.hipGraphDestroy(graph)
    finally:
        hip.set_stream(None)
    unchanged("during capture")
    # ... and the scene still takes a step: target 1 alone; the others are where step 0 left them
    s.set_morph_weights([1], [0.5])
    want = w.set([1], [0.5]).morphed()
    assert bits_equal(w.w[[0, 2]], step0[1][[0, 2]])
    assert bits_equal(s.geometry()[0][want[0]], want[1]) and bits_equal(s.geometry()[1][want[0]], want[2])
    twin.scene.set_geometry(*want)
    assert_tables_equal(all_tables(s), all_tables(twin.scene), "the accepted step after the refusals")
