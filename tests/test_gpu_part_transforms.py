"""Rigid parts (rs_scene_define_parts, rs_scene_set_part_transforms) bit for bit: against the CPU oracle on the arrays rs_bake_matrix
gives (host only; tests/test_part_transforms_host.py holds it to rs_bake_instance and to a NumPy restatement), and against a second
library scene edited by rs_scene_set_geometry with the same arrays -- every device table, the emissive grid, the host description.
Frames in flight, motion vectors, the rest pose and what crosses the bus, refusals, row bands.  No comparison has a tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import binding as ob
from restir_amd.capi import SCENE_TABLES
from tests import motion_vectors as mv
from tests import part_transforms as pt
from tests.common import HipRenderer, OracleRenderer, bits_equal, hip_scene, next_looper, oracle_scene
from tests.emitter_edits import edited_oracle_scene, scene_data
from tests.geometry_edits import apply_triangles, probe_rays, probe_segments, root_box
from tests.scene_edits import assert_same, differing

pytestmark = pytest.mark.gpu

W, H = 61, 47                        # the size tests/test_gpu_geometry_edits.py uses: partial tiles on both axes
DEPTH = 3
N_RAYS, N_SEGMENTS = 3000, 3000
INVALID, UNSUPPORTED = 10001, 10002
SPONZA = "many"                      # tests/emitter_edits.py's name of sponza:SPONZA_SCALE (2 621 triangles, 61 mod 64)


@pytest.fixture(autouse=True)
def exact_libm(hip):
    ob.set_libm_mode(1)            # cos / sin correctly rounded on both sides: every bit must agree
    hip.set_sync(True)
    yield
    ob.set_libm_mode(0)
    hip.set_sync(True)
    hip.set_side_stream(4)         # the library's default


def with_libm(fn):
    @functools.wraps(fn)
    def wrapped(*a, **k):
        ob.set_libm_mode(1)
        return fn(*a, **k)
    return wrapped


def M(name, part, step=0):
    return pt.part_matrix(name, part, step)


def object_space_box():
    """The Cornell scene's tall box as an object: its mesh about its own centroid, and the matrix that places it where it stands, turned
    and lifted a little.  (rest vertices, rest normals), matrix."""
    sd = scene_data("cornell")
    v, n = pt.rest_of(sd, pt.parts_of("cornell")[0][1])
    c = v.reshape(-1, 3).mean(0).astype(np.float32)
    return (np.ascontiguousarray(v - c), np.ascontiguousarray(n)), pt.rotation_about((0, 0, 0), (0, 1, 0), 4.0, c.astype(np.float64) + (0.0, 0.02, 0.0))


# A case: the calls made on one scene, each a list of (part, matrix); "rest": the rest pose handed to define_parts for part 1, else NULL
def calls_of(name, case):
    n = len(pt.parts_of(name)[0])
    big = 1 if name == "cornell" else 4                  # the box; the part of 193 triangles
    lamp = 0 if name == "cornell" else n - 1
    if case == "one":
        return [[(big, M(name, big))]]
    if case == "all":
        return [[(p, M(name, p)) for p in range(n)]]
    if case == "twice":                                  # the last matrix counts, the first place in the call
        return [[(big, M(name, big, 1)), (lamp, M(name, lamp)), (big, M(name, big, 2))]]
    if case == "second":                                 # a second transform acts on the rest pose, not on the first result
        return [[(big, M(name, big, 1))], [(big, M(name, big, 3))]]
    if case == "explicit_rest":
        return [[(1, object_space_box()[1]), (0, M(name, 0))]]
    raise KeyError(case)


def rest_for(case):
    return {1: object_space_box()[0]} if case == "explicit_rest" else None


def define(s, name, case="one"):
    parts = pt.parts_of(name)[0]
    rest = rest_for(case)
    if rest is None:
        s.define_parts(parts)
        return
    sd = scene_data(name)
    v = np.concatenate([rest[i][0] if i in rest else pt.rest_of(sd, p)[0] for i, p in enumerate(parts)])
    n = np.concatenate([rest[i][1] if i in rest else pt.rest_of(sd, p)[1] for i, p in enumerate(parts)])
    s.define_parts(parts, v, n)


OUTPUT_CASES = [("cornell", c) for c in ("one", "all", "twice", "second", "explicit_rest")] + [(SPONZA, c) for c in ("one", "all", "twice")]


@functools.lru_cache(maxsize=None)
def expected_after(name, case):
    """(vertices, normals) after the case's calls, from rs_bake_matrix alone; the places triangles moved from and to."""
    from restir_amd import capi
    sd = scene_data(name)
    v, n = sd.vertices.reshape(-1, 3, 3).copy(), sd.normals.reshape(-1, 3, 3).copy()
    places = []
    for call in calls_of(name, case):
        ids, bv, bn = pt.baked_edit(capi, name, [p for p, _ in call], [m for _, m in call], rest_for(case))
        places += [v[ids].mean(1), bv.mean(1)]
        v, n = apply_triangles(v, n, ids, bv, bn)
    return v, n, np.concatenate(places)


def probes(name, case):
    places = expected_after(name, case)[2]
    places = places[np.random.default_rng(5).permutation(len(places))[:64]]
    sd = scene_data(name)
    return probe_rays(sd, places, N_RAYS, 41), probe_segments(sd, places, N_SEGMENTS, 42)


def oracle_outputs(sd, scene, rays, seg):
    out = {}
    prim, mat, pos, nrm, _ = scene.intersect(rays)
    hit = prim >= 0
    out["closest"] = dict(prim=prim, mat=mat[hit], pos=pos[hit], nrm=nrm[hit])
    out["occluded"] = dict(occ=scene.test_occlusion(seg))
    r = OracleRenderer(sd, W, H, scene=scene)
    for f in range(3):                                   # three ReSTIR-DI frames with reuse 3: image, reservoirs, ray count, the planes
        r.frame(3)
        g = r.gbuf
        i = g.frame_idx ^ 1
        out["direct%d" % f] = dict(image=r.image.copy(), rays=r.rays, last=r.restir.last.copy(), temp=r.restir.temp.copy(),
                                   prim_id=g.prim_id[i].copy(), albedo=g.albedo.copy(), normal=g.normal[i].copy(), depth=g.depth[i].copy(),
                                   motion=g.motion.copy())
    d, i = np.zeros((W * H, 3), np.float32), np.zeros((W * H, 3), np.float32)
    out["path_trace"] = dict(rays=ob.path_trace(scene, r.cam, d, i, 0, 0, DEPTH), direct=d.copy(), indirect=i.copy())
    return out


def hip_outputs(capi, sd, scene, rays, seg):
    import torch
    out = {}
    drays, dseg = torch.from_numpy(rays).cuda(), torch.from_numpy(seg).cuda()

    def closest(fn):
        prim, mat, pos, nrm = (t.cpu().numpy() for t in fn(scene, drays))
        hit = prim >= 0
        return dict(prim=prim, mat=mat[hit], pos=pos[hit], nrm=nrm[hit])
    out["closest"] = closest(capi.trace_closest)
    out["closest_wave"] = closest(capi.trace_closest_wave)
    out["occluded"] = dict(occ=capi.trace_occlusion(scene, dseg).cpu().numpy())
    r = HipRenderer(capi, sd, W, H, scene=scene)
    for f in range(3):
        r.frame(3)
        g = r.gbuf.download()
        i = g["frame_idx"] ^ 1
        out["direct%d" % f] = dict(image=r.image.cpu().numpy(), rays=r.rays, last=r.restir.download(1), temp=r.restir.download(2),
                                   prim_id=g["prim_id"][i], albedo=g["albedo"], normal=g["normal"][i], depth=g["depth"][i], motion=g["motion"])
    d = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda"); i = torch.zeros_like(d)
    rays_ = capi.path_trace(scene, r.cam, d.data_ptr(), i.data_ptr(), 0, 0, DEPTH)
    out["path_trace"] = dict(rays=rays_, direct=d.cpu().numpy(), indirect=i.cpu().numpy())
    return out


@functools.lru_cache(maxsize=None)
@with_libm
def oracle_after(name, case):
    from restir_amd import capi
    sd = scene_data(name)
    v, n, _ = expected_after(name, case)
    old = oracle_scene(sd)
    scene = edited_oracle_scene(capi, old, np.arange(len(v), dtype=np.int32), v, n)
    rays, seg = probes(name, case)
    return oracle_outputs(sd, scene, rays, seg)


def all_tables(s, names=tuple(SCENE_TABLES)):
    return {k: s.debug_table(k) for k in names}


def assert_tables_equal(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (tag, k)


def assert_desc_equal(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        if k == "textures":
            assert len(a[k]) == len(b[k]) and all(bits_equal(x, y) for x, y in zip(a[k], b[k])), (tag, k)
        elif k == "materials":
            assert a[k].tobytes() == b[k].tobytes(), (tag, k)
        else:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (tag, k)


# ---- 1. outputs after a transform -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case", OUTPUT_CASES)
def test_outputs_after_transform(hip, name, case):
    """The case's calls on one library scene.  The host description then holds rs_bake_matrix of the rest pose on the transformed parts and
    the old bits elsewhere; the device's vertices and normals equal it; closest-hit and occlusion probes, the G-buffer planes and three
    ReSTIRDirect frames with reuse 3, and rs_path_trace at depth 3 equal the oracle's on a scene made from those arrays."""
    sd = scene_data(name)
    v_want, n_want, _ = expected_after(name, case)
    s = hip_scene(hip, sd)
    define(s, name, case)
    for call in calls_of(name, case):
        s.set_part_transforms([p for p, _ in call], [m for _, m in call])
    v_got, n_got = s.geometry()
    assert bits_equal(v_got, v_want) and bits_equal(n_got, n_want)
    moved = np.unique(np.concatenate([np.asarray(pt.parts_of(name)[0][p], np.int64) for call in calls_of(name, case) for p, _ in call]))
    still = np.setdiff1d(np.arange(len(v_want)), moved)
    assert bits_equal(v_got[still], sd.vertices.reshape(-1, 3, 3)[still]) and bits_equal(n_got[still], sd.normals.reshape(-1, 3, 3)[still])
    assert differing(v_got[moved], sd.vertices.reshape(-1, 3, 3)[moved]) == len(moved)
    assert bits_equal(s.debug_table("vertices"), v_got) and bits_equal(s.debug_table("normals"), n_got)
    assert bits_equal(s.host_desc()["boxes"], hip.refit_boxes(v_want, s.host_desc()["nodes"][0]))
    rays, seg = probes(name, case)
    ref, got = oracle_after(name, case), hip_outputs(hip, sd, s, rays, seg)
    for k, want in ref.items():
        for key in ([k] if k != "closest" else ["closest", "closest_wave"]):
            assert_same(want, got[key], (name, case, key))


# ---- 2. the same as rs_scene_set_geometry -------------------------------------------------------------------------------------------------------
def twin_calls(name, what):
    n = len(pt.parts_of(name)[0])
    lamp = 0 if name == "cornell" else n - 1
    boxes = [p for p in range(n) if p != lamp]
    return {"lamp": [lamp], "boxes": boxes, "both": boxes[:1] + [lamp] + boxes[1:]}[what]


@pytest.mark.parametrize("what", ["lamp", "boxes", "both"])
@pytest.mark.parametrize("name", ["cornell", SPONZA])
def test_same_as_set_geometry(hip, name, what):
    """Two scenes from one description, one edited by rs_scene_set_part_transforms, the other by rs_scene_set_geometry with the arrays of
    rs_bake_matrix in the same order, twice over (the second call on an edited scene): every table of rs_debug_scene_table byte for byte,
    the emissive grid, the host description with lightProb, lightFailId and sumLightPower.  An edit that names no emitter leaves the
    light sampler, the emissive tree's records and its grid as they were (the position of the version ring is not visible through the
    interface; both entry points run one implementation, which fills a slot only for an edit that names an emitter)."""
    sd = scene_data(name)
    a, b = hip_scene(hip, sd), hip_scene(hip, sd)
    a.define_parts(pt.parts_of(name)[0])
    start, start_grid = a.host_desc(), repr(a.emissive_grid())
    start_emi = all_tables(a, ("emiNodes", "emiTris"))
    parts = twin_calls(name, what)
    for step in (0, 1):
        ms = [M(name, p, step) for p in parts]
        a.set_part_transforms(parts, ms)
        ids, v, n = pt.baked_edit(hip, name, parts, ms)
        b.set_geometry(ids, v, n)
        assert_tables_equal(all_tables(a), all_tables(b), (name, what, step))
        assert repr(a.emissive_grid()) == repr(b.emissive_grid()), (name, what, step)
        assert_desc_equal(a.host_desc(), b.host_desc(), (name, what, step))
        ga, gb = a.geometry(), b.geometry()
        assert bits_equal(ga[0], gb[0]) and bits_equal(ga[1], gb[1])
        d = a.host_desc()
        if what == "boxes":
            assert bits_equal(d["light_prob"], start["light_prob"]) and d["sum_power"] == start["sum_power"]
            assert repr(a.emissive_grid()) == start_grid
            assert_tables_equal(all_tables(a, ("emiNodes", "emiTris")), start_emi, "no emitter named")
        else:
            assert not bits_equal(a.debug_table("emiTris")["v0"], start_emi["emiTris"]["v0"])


def test_sixty_four_lamps_same_as_set_geometry(hip):
    """A part of 64 emitters (a wave of triangles, three of lanes) next to one of 65 other triangles, on the Bistro-class scene of
    tests/emitter_edits.py -- the Sponza-class scene has ten emitters.  One scene: the transform, then rs_scene_set_geometry back to the
    pose it was created in, then rs_scene_set_geometry with the arrays of rs_bake_matrix: the tables the edit writes directly, the host
    description and the emissive grid after the first and the third call are equal.  (Every table depends on the current vertices alone;
    the trees' records of this scene are 150 MB a copy and are compared on the smaller scenes.)"""
    name = "bistro"
    sd = scene_data(name)
    s = hip_scene(hip, sd)
    parts = pt.parts_of(name)[0]
    s.define_parts(parts)
    ms = [M(name, p) for p in range(len(parts))]
    names = ("vertices", "normals", "tris", "occTris", "emiNodes", "emiTris")
    s.set_part_transforms([0, 1], ms)
    first = all_tables(s, names), s.host_desc(), repr(s.emissive_grid())
    every = np.concatenate([np.asarray(p, np.int32) for p in parts])
    s.set_geometry(every, sd.vertices.reshape(-1, 3, 3)[every], sd.normals.reshape(-1, 3, 3)[every])
    assert not bits_equal(s.debug_table("emiTris")["v0"], first[0]["emiTris"]["v0"])
    ids, v, n = pt.baked_edit(hip, name, [0, 1], ms)
    s.set_geometry(ids, v, n)
    assert_tables_equal(first[0], all_tables(s, names), name)
    assert_desc_equal(first[1], s.host_desc(), name)
    assert first[2] == repr(s.emissive_grid())
    assert bits_equal(s.geometry()[0][ids], v) and bits_equal(s.geometry()[1][ids], n)


# ---- 3. frames in flight --------------------------------------------------------------------------------------------------------------------------
N_LEAD, N_EDITED = 4, 12             # twelve edits: more than the staging ring's four buffers and the version ring's eight slots


def flight_call(name, f):
    n = len(pt.parts_of(name)[0])
    lamp, box = (0, 1) if name == "cornell" else (n - 1, 1 + f % 4)
    return [lamp, box], [M(name, lamp, f), M(name, box, f)]


@functools.lru_cache(maxsize=None)
@with_libm
def oracle_flight(name):
    from restir_amd import capi
    o = pt.OracleSide(capi, name, W, H)
    out = []
    for f in range(N_LEAD + N_EDITED):
        if f >= N_LEAD:
            o.set_part_transforms(*flight_call(name, f))
        o.r.frame(3)
        out.append(o.image())
    return out, o.direct_state()


@pytest.mark.parametrize("side_stream", [4, 0], ids=["overlapped", "no_side_streams"])
@pytest.mark.parametrize("name", ["cornell", SPONZA])
def test_twelve_frames_with_a_transform_in_every_gap(hip, name, side_stream):
    """rs_set_sync(0): four frames, then twelve with a transform of the lamp part and of a box part before each, no rs_synchronize in
    between; every frame's image is copied device to device and read at the end.  Frame f equals the oracle's after the same f
    transforms: a bake kernel that ran before an earlier frame had finished with the staging buffer, or a refit that read records the
    kernel had not written yet, would not."""
    import torch
    ref, final = oracle_flight(name)
    assert all(differing(ref[f], ref[f + 1]) > 0 for f in range(N_LEAD - 1, N_LEAD + N_EDITED - 1))
    hip.set_side_stream(side_stream)
    h = pt.HipSide(hip, name, W, H)
    outs = [torch.zeros((W * H, 3), dtype=torch.float32, device="cuda") for _ in range(N_LEAD + N_EDITED)]
    hip.set_sync(False)
    try:
        r = h.r
        for f in range(N_LEAD + N_EDITED):
            if f >= N_LEAD:
                h.set_part_transforms(*flight_call(name, f))
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
        b = outs[f].cpu().numpy()
        assert bits_equal(ref[f], b), (f, differing(ref[f], b))
    h.r.rays = h.r.restir.ray_count()
    assert_same(final, h.direct_state(), "final")


# ---- 4. motion vectors ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", SPONZA])
def test_motion_vectors_follow_a_transform(hip, name):
    """A tracked scene: a frame, then twice advance, transform, frame.  The motion plane (and everything that reads it) equals the
    oracle's for the pose at the advance, and rs_scene_download_prev_vertices returns that pose: the transform writes the current pose
    alone."""
    sd = scene_data(name)
    o, h = mv.OracleMotion(hip, sd, pipeline="indirect"), mv.HipMotion(hip, sd, pipeline="indirect")      # (ReSTIR-GI reads the plane; bit for bit)
    parts = pt.parts_of(name)[0]
    h.scene.define_parts(parts)
    n = len(parts)
    call = [1, 0] if name == "cornell" else [4, n - 1, 2]
    try:
        assert_same(o.frame(), h.frame(), (name, "at rest"))
        for step in (0, 1):
            before = h.scene.geometry()[0]
            o.advance(); h.advance()
            ms = [M(name, p, step) for p in call]
            o.set_geometry(*pt.baked_edit(hip, name, call, ms))
            h.scene.set_part_transforms(call, ms)
            assert bits_equal(h.scene.prev_vertices(), before), (name, step)
            a, b = o.frame(), h.frame()
            assert_same(a, b, (name, step))
            assert differing(o.camera_only, a["motion"]) > 0, "the moved parts are in view: the plane is not the camera-only one"
    finally:
        h.destroy()


# ---- 5. the rest pose and what crosses the bus ----------------------------------------------------------------------------------------------
def test_rest_pose_and_staged_bytes(hip):
    sd = scene_data(SPONZA)
    s = hip_scene(hip, sd)
    parts = pt.parts_of(SPONZA)[0]
    assert s.parts_info() == (0, 0) and s.staged_bytes() == 0
    s.define_parts(parts)
    listed = np.concatenate([np.asarray(p, np.int32) for p in parts])
    rest_v, rest_n = pt.rest_of(sd, listed)

    def assert_rest(tag):
        ids, v, n = s.part_rest()
        assert np.array_equal(ids, listed) and bits_equal(v, rest_v) and bits_equal(n, rest_n), tag
        assert s.parts_info() == (len(parts), len(listed)), tag
    assert_rest("defined")
    s.set_part_transforms([4], [M(SPONZA, 4)])            # 193 triangles
    big = s.staged_bytes()
    assert_rest("after a transform")
    s.set_part_transforms([0], [M(SPONZA, 0)])            # 1 triangle
    assert s.staged_bytes() == big == 112                # one part record each
    s.set_part_transforms([0, 4, 0], [M(SPONZA, 0, 1), M(SPONZA, 4, 1), M(SPONZA, 0, 2)])
    assert s.staged_bytes() == 2 * big                   # a part named twice has one record
    ids, v, n = pt.baked_edit(hip, SPONZA, [4], [M(SPONZA, 4, 2)])
    s.set_geometry(ids, v, n)
    assert s.staged_bytes() >= 193 * 76 > big
    assert_rest("after set_geometry on a part's triangles")
    s.set_part_transforms([4], [M(SPONZA, 4, 3)])         # ... which the next transform puts back on the baked rest pose
    assert bits_equal(s.geometry()[0][ids], pt.bake(hip, SPONZA, 4, M(SPONZA, 4, 3))[1])
    assert bits_equal(s.debug_table("vertices"), s.geometry()[0])
    # a transform that names only empty parts, or none: nothing happens
    before = s.staged_bytes(), s.geometry()[0]
    s.set_part_transforms([], np.zeros((0, 4, 4), np.float32))
    assert (s.staged_bytes(), ) == before[:1] and bits_equal(s.geometry()[0], before[1])
    # a new definition replaces the old one; none drops it, and a transform is refused
    s.define_parts([parts[1]])
    assert s.parts_info() == (1, 63) and np.array_equal(s.part_rest()[0], parts[1])
    assert bits_equal(s.part_rest()[1], s.geometry()[0][parts[1]])       # NULL rest arrays: the pose at the call
    s.define_parts([])
    assert s.parts_info() == (0, 0)
    refused(hip, INVALID, s.set_part_transforms, [0], [pt.identity()])
    refused(hip, INVALID, s.part_rest)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------
def refused(capi, code, call, *args):
    with pytest.raises(capi.RestirHipError) as e:
        call(*args)
    assert str(e.value).startswith("librestir_hip error %d:" % code), str(e.value)


def test_refusals_leave_scene_unchanged(hip):
    import torch
    name = "cornell"
    sd = scene_data(name)
    h, twin = pt.HipSide(hip, name, W, H), HipRenderer(hip, sd, W, H)
    s = h.r.scene
    parts = pt.parts_of(name)[0]
    desc, tables, grid = twin.scene.host_desc(), all_tables(twin.scene), repr(twin.scene.emissive_grid())
    rest = s.part_rest()
    L = hip.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lo, hi = root_box(sd.vertices)
    out_of_box = pt.translation((-(hi[0] - lo[0]) * 0.45, 0.0, 0.0))           # the tall box through the left wall
    singular = pt.from_rows(np.diag([1.0, 0.0, 1.0, 1.0]))
    nan = pt.identity(); nan[3, 1] = np.nan
    one, ident = np.array([1], np.int32), pt.identity()
    v12, n12 = pt.rest_of(sd, parts[1])
    bad_rest = v12.copy(); bad_rest[3, 1, 2] = np.inf
    first2 = np.array([0, 2], np.int32)
    ids2 = np.array([10, 11], np.int32)

    def define_raw(num, first, ids, v=None, n=None):
        hip.check(L.rs_scene_define_parts(s.handle, num, None if first is None else ptr(first), None if ids is None else ptr(ids),
                                          None if v is None else ptr(v), None if n is None else ptr(n)))
    cases = [
        ("a vertex leaves the root box", lambda: s.set_part_transforms([1], [out_of_box])),
        ("a singular matrix", lambda: s.set_part_transforms([0, 1], [ident, singular])),
        ("a NaN entry", lambda: s.set_part_transforms([1], [nan])),
        ("part id beyond", lambda: s.set_part_transforms([len(parts)], [ident])),
        ("part id below", lambda: s.set_part_transforms([-1], [ident])),
        ("null part ids", lambda: hip.check(L.rs_scene_set_part_transforms(s.handle, 1, None, ptr(ident)))),
        ("null matrices", lambda: hip.check(L.rs_scene_set_part_transforms(s.handle, 1, ptr(one), None))),
        ("negative count", lambda: hip.check(L.rs_scene_set_part_transforms(s.handle, -1, ptr(one), ptr(ident)))),
        ("null scene", lambda: hip.check(L.rs_scene_set_part_transforms(None, 1, ptr(one), ptr(ident)))),
        # (a light sampler left without power has no case of its own: a matrix that takes an emitter's area to 0 is singular, in float32
        # at the latest when its determinant underflows, and is refused for its normals; tests/test_gpu_emitter_edits.py has the refusal)
        ("define: a primitive twice in one part", lambda: s.define_parts([[10, 11, 10]])),
        ("define: a primitive in two parts", lambda: s.define_parts([[10, 11], [34], [11]])),
        ("define: an id beyond", lambda: s.define_parts([[len(sd.material_ids)]])),
        ("define: an id below", lambda: s.define_parts([[-1]])),
        ("define: first offset not 0", lambda: define_raw(1, np.array([1, 2], np.int32), ids2)),
        ("define: offsets that decrease", lambda: define_raw(2, np.array([0, 2, 1], np.int32), ids2)),
        ("define: null offsets", lambda: define_raw(1, None, ids2)),
        ("define: null ids", lambda: define_raw(1, first2, None)),
        ("define: negative count", lambda: define_raw(-1, first2, ids2)),
        ("define: rest vertices alone", lambda: define_raw(1, first2, ids2, np.ascontiguousarray(v12[:2]), None)),
        ("define: rest normals alone", lambda: define_raw(1, first2, ids2, None, np.ascontiguousarray(n12[:2]))),
        ("define: a rest value that is not finite", lambda: s.define_parts([parts[1]], bad_rest, n12)),
        ("define: null scene", lambda: hip.check(L.rs_scene_define_parts(None, 1, ptr(first2), ptr(ids2), None, None))),
    ]

    def unchanged(tag):
        assert_desc_equal(s.host_desc(), desc, tag)
        assert_tables_equal(all_tables(s), tables, tag)
        assert repr(s.emissive_grid()) == grid, tag
        assert s.parts_info() == (len(parts), len(rest[0])), tag
        got = s.part_rest()
        assert np.array_equal(got[0], rest[0]) and bits_equal(got[1], rest[1]) and bits_equal(got[2], rest[2]), tag
        a, b = twin.frame(3), h.r.frame(3)
        assert bits_equal(a, b), tag
        ga, gb = twin.gbuf.download(), h.r.gbuf.download()
        for k in ("prim_id", "normal", "depth", "albedo", "motion"):
            assert bits_equal(np.asarray(ga[k]), np.asarray(gb[k])), (tag, k)
        assert twin.rays == h.r.rays, tag
    for tag, call in cases:
        refused(hip, INVALID, call)
        unchanged(tag)
    s.set_part_transforms([2], [out_of_box])              # only the empty part: succeeds and changes nothing, whatever the matrix
    unchanged("only an empty part")

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
            refused(hip, UNSUPPORTED, s.set_part_transforms, [1], [M(name, 1)])
            refused(hip, UNSUPPORTED, s.define_parts, [parts[1]])
        finally:
            assert rt.hipStreamEndCapture(stream.cuda_stream, C.byref(graph)) == 0
            if graph:
                rt.hipGraphDestroy(graph)
    finally:
        hip.set_stream(None)
    unchanged("during capture")
    s.set_part_transforms([1], [M(name, 1)])              # ... and the scene still takes a transform
    assert bits_equal(s.geometry()[0][parts[1]], pt.bake(hip, name, 1, M(name, 1))[1])


# ---- 7. row bands -----------------------------------------------------------------------------------------------------------------------------------
def test_row_bands_with_a_transform(hip):
    """rs_restir_phase_a / _phase_b on two bands, a transform between frames: the banded library equals the oracle's full frame."""
    name = "cornell"
    bands = [(0, 19), (19, H)]
    o, h = pt.OracleSide(hip, name, W, H), pt.HipSide(hip, name, W, H)
    for f in range(5):
        if f in (2, 3):
            call = ([0, 1], [M(name, 0, f), M(name, 1, f)]) if f == 2 else ([1], [M(name, 1, f)])
            o.set_part_transforms(*call); h.set_part_transforms(*call)
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
