"""Edits that move emitters (rs_scene_set_geometry) against the CPU oracle, bit for bit: the host tables, every trace service and every
render path after every kind of edit, against the oracle AND against a second library scene created from the edited scene's host
description; edits with frames in flight; edits interleaved with the other kinds of edit; the environment map edited between two emitter
edits; retained G-buffer planes; row bands; the refusals.  The oracle's side of an edit is a scene made afresh from the edited arrays
with light tables rebuilt by the oracle's own functions (tests/emitter_edits.py); tests/test_emitter_edits_cases.py shows without a GPU
that these inputs mean something."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import binding as ob
from tests.common import EmissionEdits, HipRenderer, OracleRenderer, bits_equal, hip_scene, next_looper, oracle_scene
from tests.emitter_edits import (SCENES, HipSide, OracleSide, edited_oracle_scene, edits_up_to, emitter_edit, emitters, kinds_for, scene_data)
from tests.geometry_edits import geometry_edit, movable, probe_rays, probe_segments, root_box
from tests.scene_edits import assert_same, differing

pytestmark = pytest.mark.gpu

W, H = 61, 47                        # the size tests/test_gpu_geometry_edits.py uses: partial tiles on both axes
N_RAYS, N_SEGMENTS = 2000, 2000
CASES = [(name, kind) for name in SCENES for kind in kinds_for(name)]


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


def probes(name, kind):
    sd = scene_data(name)
    places = edits_up_to(name, kind)[1]
    places = places[np.random.default_rng(5).permutation(len(places))[:64]]
    return probe_rays(sd, places, N_RAYS, 31), probe_segments(sd, places, N_SEGMENTS, 32)


# ---- what is compared: every trace service and every render path on one scene ---------------------------------------------------------
MULTI = [("path_trace", 4), ("path_trace", 1), ("pt_indirect", 4), ("pt_indirect", 1)]      # depth 1: the only bounce is the last (the emissive tree's question)


def oracle_outputs(sd, scene, rays, seg, size=(W, H)):
    w, h = size
    out = {}
    prim, mat, pos, nrm, _ = scene.intersect(rays)
    hit = prim >= 0
    out["closest"] = dict(prim=prim, mat=mat[hit], pos=pos[hit], nrm=nrm[hit])
    out["occluded"] = dict(occ=scene.test_occlusion(seg))
    for track in (False, True):                          # ReSTIRDirect with reuse 3, 2, 1, 0 in consecutive frames: history carries over
        r = OracleRenderer(sd, w, h, scene=scene, track=track)
        for reuse in (3, 2, 1, 0):
            r.frame(reuse)
            g = r.gbuf
            i = g.frame_idx ^ 1
            out["direct_%s_%d" % ("tracked" if track else "plain", reuse)] = dict(
                image=r.image.copy(), rays=r.rays, last=r.restir.last.copy(), temp=r.restir.temp.copy(), prim_id=g.prim_id[i].copy(),
                albedo=g.albedo.copy(), normal=g.normal[i].copy(), depth=g.depth[i].copy(), motion=g.motion.copy())
    n = w * h
    d, i = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    out["pt_direct"] = dict(rays=ob.pt_direct(scene, r.cam, d, 0, 0), direct=d.copy())
    for what, depth in MULTI:
        d[:] = 0; i[:] = 0
        if what == "path_trace":
            out["%s%d" % (what, depth)] = dict(rays=ob.path_trace(scene, r.cam, d, i, 0, 0, depth), direct=d.copy(), indirect=i.copy())
        else:
            out["%s%d" % (what, depth)] = dict(rays=ob.pt_indirect(scene, r.cam, i, 0, 0, depth), indirect=i.copy())
    for depth in (2, 3):
        i[:] = 0
        r.gbuf.render(scene, r.cam)
        rays_ = r.restir.indirect(scene, r.cam, r.gbuf, i, 0, 0, 1, depth)
        out["restir_indirect%d" % depth] = dict(rays=rays_, indirect=i.copy(), reservoirs=r.restir.ind_last.copy())
    return out


def hip_outputs(capi, sd, scene, rays, seg, size=(W, H)):
    import torch
    w, h = size
    out = {}
    drays, dseg = torch.from_numpy(rays).cuda(), torch.from_numpy(seg).cuda()

    def closest(fn):
        prim, mat, pos, nrm = (t.cpu().numpy() for t in fn(scene, drays))
        hit = prim >= 0
        return dict(prim=prim, mat=mat[hit], pos=pos[hit], nrm=nrm[hit])
    out["closest"] = closest(capi.trace_closest)
    was = capi.set_ordered_tree(scene, True)
    out["closest_wave_ordered"] = closest(capi.trace_closest_wave)
    capi.set_ordered_tree(scene, False)
    out["closest_wave_reference"] = closest(capi.trace_closest_wave)
    capi.set_ordered_tree(scene, was)
    out["occluded"] = dict(occ=capi.trace_occlusion(scene, dseg).cpu().numpy())
    for track in (False, True):
        r = HipRenderer(capi, sd, w, h, scene=scene, track=track)
        for reuse in (3, 2, 1, 0):
            r.frame(reuse)
            g = r.gbuf.download()
            i = g["frame_idx"] ^ 1
            out["direct_%s_%d" % ("tracked" if track else "plain", reuse)] = dict(
                image=r.image.cpu().numpy(), rays=r.rays, last=r.restir.download(1), temp=r.restir.download(2), prim_id=g["prim_id"][i],
                albedo=g["albedo"], normal=g["normal"][i], depth=g["depth"][i], motion=g["motion"])
    n = w * h
    d = torch.zeros((n, 3), dtype=torch.float32, device="cuda"); i = torch.zeros_like(d)
    out["pt_direct"] = dict(rays=capi.path_trace_direct(scene, r.cam, d.data_ptr(), 0, 0), direct=d.cpu().numpy())
    for what, depth in MULTI:
        d.zero_(); i.zero_()
        if what == "path_trace":
            rays_ = capi.path_trace(scene, r.cam, d.data_ptr(), i.data_ptr(), 0, 0, depth)
            out["%s%d" % (what, depth)] = dict(rays=rays_, direct=d.cpu().numpy(), indirect=i.cpu().numpy())
        else:
            rays_ = capi.path_trace_indirect(scene, r.cam, i.data_ptr(), 0, 0, depth)
            out["%s%d" % (what, depth)] = dict(rays=rays_, indirect=i.cpu().numpy())
    for depth in (2, 3):
        i.zero_()
        r.gbuf.render(scene, r.cam)
        rays_ = r.restir.indirect(scene, r.cam, r.gbuf, i.data_ptr(), 0, 0, 1, depth)
        out["restir_indirect%d" % depth] = dict(rays=rays_, indirect=i.cpu().numpy(), reservoirs=r.restir.download_indirect(1))
    return out


def assert_outputs(ref, got, tag):
    for k, want in ref.items():
        for name in ([k] if k != "closest" else ["closest", "closest_wave_ordered", "closest_wave_reference"]):
            assert_same(want, got[name], (tag, name))


@functools.lru_cache(maxsize=None)
@with_libm
def oracle_scene_after(name, kind):
    from restir_amd import capi
    scene = oracle_scene(scene_data(name))
    if kind is not None:
        for ids, v, n in edits_up_to(name, kind)[0]:
            scene = edited_oracle_scene(capi, scene, ids, v, n)
    return scene


@functools.lru_cache(maxsize=None)
@with_libm
def oracle_after(name, kind, size=(W, H)):
    rays, seg = probes(name, kind)
    return oracle_outputs(scene_data(name), oracle_scene_after(name, kind), rays, seg, size)


def second_scene(capi, sd, s):
    """rs_scene_create(rs_scene_host_desc(s))."""
    v, n = s.geometry()
    d = s.host_desc()
    env = d["env_map_tex"] >= 0
    return capi.Scene.from_tables(v, n, sd.texcoords, sd.material_ids, d["materials"], d, textures=d["textures"], env_map_tex=d["env_map_tex"],
                                  env_sampler=(d["env_prob"], d["env_fail"]) if env else None)


def assert_host_tables(hip, s, start, want, v_want, n_want, tag):
    """vertices, normals, boxes, lightProb, lightFailId, sumLightPower as the oracle's side holds them; everything else as at the start."""
    v_got, n_got = s.geometry()
    desc = s.host_desc()
    assert bits_equal(v_got, v_want) and bits_equal(n_got, n_want), tag
    assert bits_equal(desc["boxes"], hip.refit_boxes(v_want, start["nodes"][0])), tag
    assert bits_equal(desc["light_prob"], want.light_prob) and np.array_equal(desc["light_fail"], want.light_fail), tag
    assert bits_equal(np.float32(desc["sum_power"]), np.float32(want.sum_power)), tag
    for k in desc:
        if k not in ("boxes", "textures", "materials", "light_prob", "light_fail", "sum_power"):
            assert np.array_equal(desc[k], start[k]), (tag, k)
    assert desc["materials"].tobytes() == start["materials"].tobytes(), tag
    return desc


# ---- 1. every service and render path after every kind of edit --------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", CASES)
def test_outputs_after_edit(hip, name, kind):
    """The edits up to `kind`, in turn, on one library scene; then the host tables, rs_trace_closest, rs_trace_closest_wave (ordered trees
    on and off), rs_trace_occlusion, the G-buffer planes, ReSTIRDirect with reuse 3, 2, 1 and 0 with and without light tracking,
    rs_path_trace_direct, rs_path_trace and rs_path_trace_indirect at depths 4 and 1 and rs_restir_indirect at depths 2 and 3 equal the
    oracle's on the edited scene, and so do those of a second library scene created from the edited scene's host description; the
    emissive tree's grid equals the second scene's."""
    sd = scene_data(name)
    edits, _, v_want, n_want = edits_up_to(name, kind)
    ref = oracle_after(name, kind)
    rays, seg = probes(name, kind)
    s = hip_scene(hip, sd)
    start = s.host_desc()
    for ids, v, n in edits:
        s.set_geometry(ids, v, n)
    assert_host_tables(hip, s, start, oracle_scene_after(name, kind), v_want, n_want, (name, kind))
    fresh = second_scene(hip, sd, s)
    a, b = s.emissive_grid(), fresh.emissive_grid()
    assert a["state"] == b["state"] == (0 if kind == "collapse_all" else 1), (a, b)
    if a["state"]:
        assert bits_equal(a["base"], b["base"]) and bits_equal(a["scale"], b["scale"]) and a["margin"] == b["margin"], (a, b)
    assert_outputs(ref, hip_outputs(hip, sd, s, rays, seg), (name, kind, "edited"))
    assert_outputs(ref, hip_outputs(hip, sd, fresh, rays, seg), (name, kind, "created from the description"))


def test_partial_tiles_at_97_by_61(hip):
    sd = scene_data("cornell")
    ref = oracle_after("cornell", "mixed", (97, 61))
    rays, seg = probes("cornell", "mixed")
    s = hip_scene(hip, sd)
    for ids, v, n in edits_up_to("cornell", "mixed")[0]:
        s.set_geometry(ids, v, n)
    assert_outputs(ref, hip_outputs(hip, sd, s, rays, seg, (97, 61)), "97 x 61")


# ---- 2. twenty overlapped frames with an edit in every gap ---------------------------------------------------------------------------------
N_LEAD, N_FRAMES = 4, 24             # four frames without an edit (three render, the fourth is answered from retained planes), then twenty with one each


def gap_edit(sd, vertices, f):
    kinds = ("one", "all", "mixed", "repeated", "flip", "scale_down", "carry_back")
    return emitter_edit(sd, vertices, kinds[f % len(kinds)], seed=100 + f)


@functools.lru_cache(maxsize=None)
@with_libm
def oracle_flight(name):
    from restir_amd import capi
    sd = scene_data(name)
    o = OracleSide(capi, sd, W, H)
    out = []
    for f in range(N_FRAMES):
        if f >= N_LEAD:
            o.set_geometry(*gap_edit(sd, o.r.scene.vertices, f))
        o.r.frame(3)
        out.append(o.image())
    return out, o.direct_state()


@pytest.mark.parametrize("side_stream", [4, 0], ids=["overlapped", "no_side_streams"])
@pytest.mark.parametrize("name", ["cornell", "many"])
def test_twenty_frames_with_an_edit_in_every_gap(hip, name, side_stream):
    """rs_set_sync(0): four frames, then twenty with an emitter edit before each, no rs_synchronize in between; every frame's image
    is copied device to device and read at the end.  Frame f equals the oracle's after the same f edits: a pass that saw new vertices
    with the old light records, or the reverse, or the emissive tree of another gap, would not.  More edits than the version ring has
    slots.  Still camera, rs_gbuffer_set_reuse(1): every edit makes the next request render (retained planes are invalidated)."""
    import torch
    sd = scene_data(name)
    ref, final = oracle_flight(name)
    assert all(differing(ref[f], ref[f + 1]) > 0 for f in range(N_LEAD - 1, N_FRAMES - 1))
    hip.set_side_stream(side_stream)
    h = HipSide(hip, sd, W, H)
    h.r.gbuf.set_reuse(True)
    outs = [torch.zeros((W * H, 3), dtype=torch.float32, device="cuda") for _ in range(N_FRAMES)]
    stats = []
    cur = sd.vertices.reshape(-1, 3, 3).copy()
    hip.set_sync(False)
    try:
        r = h.r
        for f in range(N_FRAMES):
            if f >= N_LEAD:
                ids, v, n = gap_edit(sd, cur, f)
                h.set_geometry(ids, v, n)
                for j, p in enumerate(ids):
                    cur[p] = np.asarray(v).reshape(-1, 3, 3)[j]
            r.gbuf.render(r.scene, r.cam)
            r.restir.direct(r.scene, r.cam, r.gbuf, r.image.data_ptr(), 0, r.looper, 3)
            r.looper += 1
            r.gbuf.update(r.cam)
            stats.append(r.gbuf.reuse_stats())
            hip.hip_memcpy_d2d_async(outs[f].data_ptr(), r.image.data_ptr(), W * H * 12)
        hip.synchronize()
    finally:
        hip.set_sync(True)
        hip.set_side_stream(4)
    for f in range(N_FRAMES):
        b = outs[f].cpu().numpy()
        assert bits_equal(ref[f], b), (f, differing(ref[f], b))
    h.r.rays = h.r.restir.ray_count()
    assert_same(final, h.direct_state(), "final")
    assert stats[N_LEAD - 1] == (N_LEAD - 1, 1), stats       # the planes were being reused ...
    assert [s[0] for s in stats[N_LEAD:]] == list(range(N_LEAD, N_FRAMES)) and stats[-1][1] == 1, stats      # ... and every request after an edit rendered


# ---- 3. in one frame gap with the other edits ------------------------------------------------------------------------------------------------
def test_one_gap_with_every_other_edit(hip):
    """One frame gap, overlapped mode: set_geometry of a lamp, set_emission, set_triangles, set_materials, set_geometry of the same lamp
    again.  The calls stay in order: the frames after equal the oracle's with the same calls in the same order."""
    sd = scene_data("cornell")
    lamps = EmissionEdits(sd, 4)
    mat = np.nonzero(sd.materials["type"] != 4)[0][:1].astype(np.int32)
    rec = sd.materials[mat].copy()
    rec["baseColor"] = (0.15, 0.7, 0.35)
    first = emitter_edit(sd, sd.vertices, "one", seed=1)
    lo, hi = root_box(sd.vertices)
    again = (first[0], np.clip(first[1] * np.float32(0.93), lo, hi).astype(np.float32), None)
    calls = [("set_geometry", first), ("set_emission", lamps.next()), ("set_triangles", geometry_edit(sd, sd.vertices, "repeated", seed=1)),
             ("set_materials", (mat, rec)), ("set_geometry", again)]
    o, h = OracleSide(hip, sd, W, H), HipSide(hip, sd, W, H)
    ref = []
    for f in range(5):
        if f == 2:
            for what, args in calls:
                getattr(o, what)(*args)
        o.r.frame(3)
        ref.append(o.direct_state())
    hip.set_sync(False)
    try:
        for f in range(5):
            if f == 2:
                for what, args in calls:
                    getattr(h, what)(*args)
            h.r.frame(3)
            assert_same(ref[f], h.direct_state(), f)
    finally:
        hip.set_sync(True)
    assert differing(ref[1]["image"], ref[2]["image"]) > 0


def test_environment_map_edited_between_two_emitter_edits(hip):
    """set_geometry, set_texture of the environment map, set_geometry: the environment entry's power is the map's at either emitter edit
    (the first carries the power the scene was built with, the second the edited map's), so the host tables and the frames equal the
    oracle's."""
    sd = scene_data("env")
    o, h = OracleSide(hip, sd, W, H), HipSide(hip, sd, W, H)
    start = h.r.scene.host_desc()
    env = (sd.textures[sd.env_map_tex] * np.float32(0.3)).astype(np.float32)
    env[10:14, 30:36] = (40.0, 30.0, 5.0)
    e1 = emitter_edit(sd, sd.vertices, "scale_up", seed=3)
    for step in range(3):
        for side in (o, h):
            if step == 1:
                side.set_texture(sd.env_map_tex, env)
            else:
                cur = o.r.scene.vertices if side is o else h.r.scene.geometry()[0]
                side.set_geometry(*(e1 if step == 0 else emitter_edit(sd, cur, "all", seed=4)))
        want, desc = o.r.scene, h.r.scene.host_desc()
        assert bits_equal(desc["light_prob"], want.light_prob) and np.array_equal(desc["light_fail"], want.light_fail), step
        assert bits_equal(np.float32(desc["sum_power"]), np.float32(want.sum_power)), step
        o.r.frame(3); h.r.frame(3)
        assert_same(o.direct_state(), h.direct_state(), step)
    assert not bits_equal(h.r.scene.host_desc()["light_prob"], start["light_prob"])
    fresh = second_scene(hip, sd, h.r.scene)
    assert bits_equal(fresh.host_desc()["light_prob"], o.r.scene.light_prob)


# ---- 4. row bands -----------------------------------------------------------------------------------------------------------------------------
def test_row_bands_with_an_edit(hip):
    """rs_restir_phase_a / _phase_b on two bands, an emitter edit between frames: the banded library equals the oracle's full frame."""
    sd = scene_data("cornell")
    bands = [(0, 19), (19, H)]
    o, h = OracleSide(hip, sd, W, H), HipSide(hip, sd, W, H)
    for f in range(5):
        if f in (2, 3):
            e = emitter_edit(sd, o.r.scene.vertices, ("one", "scale_up")[f - 2], seed=9)
            o.set_geometry(*e); h.set_geometry(*e)
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


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def refused(capi, code, call, *args):
    with pytest.raises(capi.RestirHipError) as e:
        call(*args)
    assert str(e.value).startswith("librestir_hip error %d:" % code), str(e.value)


def test_refusals_leave_scene_unchanged(hip):
    import torch
    sd = scene_data("cornell")
    o, h = OracleSide(hip, sd, W, H), HipSide(hip, sd, W, H)
    s = h.r.scene
    e = emitter_edit(sd, sd.vertices, "one", seed=1)
    s.set_geometry(*e); o.set_geometry(*e)              # (an edited scene: the refit's tables and the version ring exist)
    lo, hi = root_box(sd.vertices)
    lamp = emitters(sd)
    p = int(lamp[0])
    tri = s.geometry()[0][[p]].copy()
    L = hip.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ids1 = np.array([p], np.int32)

    def moved(axis, value):
        t = tri.copy(); t[0, 1, axis] = value
        return t
    point = np.broadcast_to(tri[0, 0], (len(lamp), 3, 3)).copy()
    cases = [
        ("null ids", lambda: hip.check(L.rs_scene_set_geometry(s.handle, 1, None, ptr(tri), None))),
        ("null vertices", lambda: hip.check(L.rs_scene_set_geometry(s.handle, 1, ptr(ids1), None, None))),
        ("negative count", lambda: hip.check(L.rs_scene_set_geometry(s.handle, -1, ptr(ids1), ptr(tri), None))),
        ("id below", lambda: s.set_geometry([-1], tri)),
        ("id beyond", lambda: s.set_geometry([len(sd.material_ids)], tri)),
        ("NaN vertex", lambda: s.set_geometry([p], moved(0, np.nan))),
        ("infinite normal", lambda: s.set_geometry([p], tri, moved(2, np.inf))),
        ("outside the root box, above", lambda: s.set_geometry([p], moved(1, np.nextafter(hi[1], np.float32(np.inf))))),
        ("outside the root box, below", lambda: s.set_geometry([p], moved(2, lo[2] - np.float32(1.0)))),
        ("the only lamp of a scene without a sky collapsed: no power", lambda: s.set_geometry(lamp, point)),
        ("set_triangles still refuses an emitter", lambda: s.set_triangles([p], tri)),
    ]
    desc, geometry, grid = s.host_desc(), s.geometry(), s.emissive_grid()

    def unchanged(tag):
        d, g = s.host_desc(), s.geometry()
        assert bits_equal(d["boxes"], desc["boxes"]) and bits_equal(g[0], geometry[0]) and bits_equal(g[1], geometry[1]), tag
        assert bits_equal(d["light_prob"], desc["light_prob"]) and d["sum_power"] == desc["sum_power"], tag
        assert repr(s.emissive_grid()) == repr(grid), tag
        o.r.frame(3); h.r.frame(3)
        assert_same(o.direct_state(), h.direct_state(), tag)
    for name, call in cases:
        refused(hip, 10001, call)                            # RS_ERR_INVALID_ARGUMENT
        unchanged(name)
    s.set_geometry(np.zeros(0, np.int32), np.zeros((0, 3, 3), np.float32))    # count == 0 succeeds and changes nothing
    unchanged("empty edit")

    # while the library stream is being captured into a graph: RS_ERR_UNSUPPORTED
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
            refused(hip, 10002, s.set_geometry, [p], tri)
        finally:
            assert rt.hipStreamEndCapture(stream.cuda_stream, C.byref(graph)) == 0
            if graph:
                rt.hipGraphDestroy(graph)
    finally:
        hip.set_stream(None)
    unchanged("during capture")
