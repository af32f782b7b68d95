"""Triangle edits between frames (rs_scene_set_triangles) against the CPU oracle, bit for bit: every trace service and every render path
after every kind of edit, against the oracle AND against a second library scene created from the edited scene's host description; the
host tables; edits with frames in flight and retained G-buffer planes; edits interleaved with material and emission edits; the
refusals; row bands.  The oracle's side of an edit is a scene made afresh from the edited arrays with boxes from rs_refit_boxes
(tests/geometry_edits.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import binding as ob
from tests.common import EmissionEdits, HipRenderer, OracleRenderer, bits_equal, get_scene, hip_scene, next_looper, oracle_scene
from tests.geometry_edits import (EDIT_KINDS, HipSide, OracleSide, apply_triangles, corner_triangle, edited_oracle_scene, geometry_edit,
                                  movable, probe_rays, probe_segments, root_box)
from tests.scene_edits import assert_same, differing
from tests.test_geometry_refit_host import SPONZA_SCALE

pytestmark = pytest.mark.gpu

SCENES = {"cornell": "cornell", "sponza": "sponza:%g" % SPONZA_SCALE}      # 36 triangles; 2 621 (61 mod 64), reference tree 22 deep
W, H = 61, 47                        # partial tiles on both axes
DEPTH = 3
N_RAYS, N_SEGMENTS = 3000, 3000


@pytest.fixture(autouse=True)
def exact_libm(hip):
    ob.set_libm_mode(1)            # cos / sin correctly rounded on both sides: every bit must agree
    hip.set_sync(True)
    yield
    ob.set_libm_mode(0)
    hip.set_sync(True)
    hip.set_side_stream(4)         # the library's default


@functools.lru_cache(maxsize=None)
def scene_data(name):
    return get_scene(SCENES[name])


def with_libm(fn):
    @functools.wraps(fn)
    def wrapped(*a, **k):
        ob.set_libm_mode(1)
        return fn(*a, **k)
    return wrapped


@functools.lru_cache(maxsize=None)
def edits_up_to(name, kind):
    """The edits of EDIT_KINDS up to and including `kind`, each made on the vertices the ones before it left, and the places (points)
    the last one moved triangles from and to."""
    sd = scene_data(name)
    v, n = sd.vertices.reshape(-1, 3, 3).copy(), sd.normals.reshape(-1, 3, 3).copy()
    out, places = [], None
    for k in EDIT_KINDS[:EDIT_KINDS.index(kind) + 1]:
        ids, ev, en = geometry_edit(sd, v, k, seed=11)
        places = np.concatenate([v[ids].mean(1), np.asarray(ev).reshape(-1, 3, 3).mean(1)])
        v, n = apply_triangles(v, n, ids, ev, en)
        out.append((ids, ev, en))
    return out, places, v, n


def probes(name, kind):
    sd = scene_data(name)
    places = edits_up_to(name, kind)[1]
    places = places[np.random.default_rng(5).permutation(len(places))[:64]]
    return probe_rays(sd, places, N_RAYS, 21), probe_segments(sd, places, N_SEGMENTS, 22)


# ---- what is compared: every trace service and every render path on one scene ---------------------------------------------------------
def oracle_outputs(sd, scene, rays, seg):
    out = {}
    prim, mat, pos, nrm, _ = scene.intersect(rays)
    hit = prim >= 0
    out["closest"] = dict(prim=prim, mat=mat[hit], pos=pos[hit], nrm=nrm[hit])
    out["occluded"] = dict(occ=scene.test_occlusion(seg))
    r = OracleRenderer(sd, W, H, scene=scene)
    for f in range(2):                                   # two ReSTIR-DI frames: image, both reservoir buffers, the ray count, the planes
        r.frame(3)
        g = r.gbuf
        i = g.frame_idx ^ 1
        out["direct%d" % f] = dict(image=r.image.copy(), rays=r.rays, last=r.restir.last.copy(), temp=r.restir.temp.copy(),
                                   prim_id=g.prim_id[i].copy(), albedo=g.albedo.copy(), normal=g.normal[i].copy(), depth=g.depth[i].copy(),
                                   motion=g.motion.copy())
    n = W * H
    d, i = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    out["pt_direct"] = dict(rays=ob.pt_direct(scene, r.cam, d, 0, 0), direct=d.copy())
    d[:] = 0
    out["path_trace"] = dict(rays=ob.path_trace(scene, r.cam, d, i, 0, 0, DEPTH), direct=d.copy(), indirect=i.copy())
    i[:] = 0
    r.gbuf.render(scene, r.cam)
    rays_ = r.restir.indirect(scene, r.cam, r.gbuf, i, 0, 0, 1, DEPTH)
    out["restir_indirect"] = dict(rays=rays_, indirect=i.copy(), reservoirs=r.restir.ind_last.copy())
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
    was = capi.set_ordered_tree(scene, True)
    assert was, "the scene has its grid-box trees (the shadow tree and the ordered trees): the refit of their boxes is under test"
    out["closest_wave_ordered"] = closest(capi.trace_closest_wave)
    capi.set_ordered_tree(scene, False)
    out["closest_wave_reference"] = closest(capi.trace_closest_wave)
    capi.set_ordered_tree(scene, was)
    out["occluded"] = dict(occ=capi.trace_occlusion(scene, dseg).cpu().numpy())
    r = HipRenderer(capi, sd, W, H, scene=scene)
    for f in range(2):
        r.frame(3)
        g = r.gbuf.download()
        i = g["frame_idx"] ^ 1
        out["direct%d" % f] = dict(image=r.image.cpu().numpy(), rays=r.rays, last=r.restir.download(1), temp=r.restir.download(2),
                                   prim_id=g["prim_id"][i], albedo=g["albedo"], normal=g["normal"][i], depth=g["depth"][i], motion=g["motion"])
    n = W * H
    d = torch.zeros((n, 3), dtype=torch.float32, device="cuda"); i = torch.zeros_like(d)
    out["pt_direct"] = dict(rays=capi.path_trace_direct(scene, r.cam, d.data_ptr(), 0, 0), direct=d.cpu().numpy())
    d.zero_()
    rays_ = capi.path_trace(scene, r.cam, d.data_ptr(), i.data_ptr(), 0, 0, DEPTH)
    out["path_trace"] = dict(rays=rays_, direct=d.cpu().numpy(), indirect=i.cpu().numpy())
    i.zero_()
    r.gbuf.render(scene, r.cam)
    rays_ = r.restir.indirect(scene, r.cam, r.gbuf, i.data_ptr(), 0, 0, 1, DEPTH)
    out["restir_indirect"] = dict(rays=rays_, indirect=i.cpu().numpy(), reservoirs=r.restir.download_indirect(1))
    return out


def assert_outputs(ref, got, tag):
    for k, want in ref.items():
        for name in ([k] if k != "closest" else ["closest", "closest_wave_ordered", "closest_wave_reference"]):
            assert_same(want, got[name], (tag, name))


@functools.lru_cache(maxsize=None)
@with_libm
def oracle_after(name, kind):
    sd = scene_data(name)
    scene = oracle_scene(sd)
    if kind is not None:
        from restir_amd import capi
        for ids, v, n in edits_up_to(name, kind)[0]:
            scene = edited_oracle_scene(capi, scene, ids, v, n)
    rays, seg = probes(name, kind or EDIT_KINDS[0])
    return oracle_outputs(sd, scene, rays, seg)


def second_scene(capi, sd, s):
    """rs_scene_create(rs_scene_host_desc(s))."""
    v, n = s.geometry()
    return capi.Scene.from_tables(v, n, sd.texcoords, sd.material_ids, sd.materials, s.host_desc())


# ---- 1. every service and render path after every kind of edit --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", EDIT_KINDS)
@pytest.mark.parametrize("name", list(SCENES))
def test_outputs_after_edit(hip, name, kind):
    """The edits of EDIT_KINDS up to `kind`, in turn, on one library scene; then rs_trace_closest, rs_trace_closest_wave (ordered trees
    on and off), rs_trace_occlusion, the G-buffer planes, two ReSTIR-DI frames, rs_path_trace_direct, rs_path_trace and
    rs_restir_indirect at depth 3 equal the oracle's on the edited geometry, and so do those of a second library scene created from the
    edited scene's host description.  Not vacuous: the oracle's outputs differ from the unedited scene's (except after `carry_back`,
    which must restore the original scene bit for bit)."""
    sd = scene_data(name)
    edits, _, v_want, n_want = edits_up_to(name, kind)
    ref = oracle_after(name, kind)
    rays, seg = probes(name, kind)
    s = hip_scene(hip, sd)
    start = s.host_desc()
    for ids, v, n in edits:
        s.set_triangles(ids, v, n)
    # the host tables
    v_got, n_got = s.geometry()
    desc = s.host_desc()
    assert bits_equal(v_got, v_want) and bits_equal(n_got, n_want)
    assert bits_equal(desc["boxes"], hip.refit_boxes(v_want, start["nodes"][0]))
    for k in desc:
        if k not in ("boxes", "textures", "materials"):
            assert np.array_equal(desc[k], start[k]), k
    assert desc["materials"].tobytes() == start["materials"].tobytes()
    if kind == "carry_back":
        assert bits_equal(v_got, sd.vertices.reshape(-1, 3, 3))
        assert np.array_equal(desc["boxes"], start["boxes"])                  # (as values: rs_build_bvh's zeros may differ in sign)
        assert_outputs(oracle_after(name, None), hip_outputs(hip, sd, s, *probes(name, EDIT_KINDS[0])), (name, kind, "original"))
    else:
        base = oracle_after(name, None)
        assert (differing(ref["direct1"]["image"], base["direct1"]["image"]) > 0 or not np.array_equal(ref["closest"]["prim"], base["closest"]["prim"])
                or not np.array_equal(ref["occluded"]["occ"], base["occluded"]["occ"]))
    assert_outputs(ref, hip_outputs(hip, sd, s, rays, seg), (name, kind, "edited"))
    assert_outputs(ref, hip_outputs(hip, sd, second_scene(hip, sd, s), rays, seg), (name, kind, "created from the description"))


# ---- 2. frames in flight, retained planes -------------------------------------------------------------------------------------------------
N_BEFORE, N_AFTER = 5, 4


@functools.lru_cache(maxsize=None)
@with_libm
def oracle_flight(name):
    from restir_amd import capi
    sd = scene_data(name)
    o = OracleSide(capi, sd, W, H)
    out = []
    for f in range(N_BEFORE + N_AFTER):
        if f == N_BEFORE:
            o.set_triangles(*geometry_edit(sd, sd.vertices, "all", seed=2))
        o.r.frame(3)
        out.append(o.image())
    return out, o.direct_state()


@pytest.mark.parametrize("side_stream", [4, 0], ids=["overlapped", "no_side_streams"])
@pytest.mark.parametrize("name", list(SCENES))
def test_edit_with_frames_in_flight(hip, name, side_stream):
    """rs_set_sync(0): five frames, an edit of every movable triangle, four frames, no rs_synchronize in between; every frame's image is
    copied device to device and read at the end.  Frames before the edit equal the oracle's on the old geometry, frames after it the
    oracle's on the new.  Still camera, rs_gbuffer_set_reuse(1): the requests before the edit are answered from retained planes, and the
    edit makes the next request render."""
    import torch
    sd = scene_data(name)
    ref, final = oracle_flight(name)
    assert differing(ref[N_BEFORE - 1], ref[N_BEFORE]) > 0.10 * W * H
    hip.set_side_stream(side_stream)
    h = HipSide(hip, sd, W, H)
    h.r.gbuf.set_reuse(True)
    outs = [torch.zeros((W * H, 3), dtype=torch.float32, device="cuda") for _ in range(N_BEFORE + N_AFTER)]
    stats = []
    hip.set_sync(False)
    try:
        r = h.r
        for f in range(N_BEFORE + N_AFTER):
            if f == N_BEFORE:
                h.set_triangles(*geometry_edit(sd, sd.vertices, "all", seed=2))
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
    for f in range(N_BEFORE + N_AFTER):
        b = outs[f].cpu().numpy()
        assert bits_equal(ref[f], b), (f, differing(ref[f], b))
    h.r.rays = h.r.restir.ray_count()
    assert_same(final, h.direct_state(), "final")
    (r0, u0), (r1, u1) = stats[N_BEFORE - 1], stats[N_BEFORE]
    assert u0 >= 1, stats                                    # the planes were being reused
    assert (r1, u1) == (r0 + 1, u0), stats                   # the request after the edit rendered


# ---- 3. in one frame gap with the other edits ------------------------------------------------------------------------------------------------
def test_interleaved_with_material_and_emission_edits(hip):
    """One frame gap, overlapped mode: set_triangles, set_materials, set_triangles of the same triangle again, set_emission, set_triangles
    of another.  The calls stay in order: the frames after equal the oracle's with the same calls in the same order."""
    sd = scene_data("cornell")
    ids = movable(sd)
    lamps = EmissionEdits(sd, 4)
    mat = np.nonzero(sd.materials["type"] != 4)[0][:1].astype(np.int32)
    rec = sd.materials[mat].copy()
    rec["baseColor"] = (0.15, 0.7, 0.35)
    one = geometry_edit(sd, sd.vertices, "one", seed=1)
    lo, hi = root_box(sd.vertices)
    again = (one[0], np.clip(one[1][:, ::-1] * np.float32(0.97), lo, hi).astype(np.float32), None)
    other = geometry_edit(sd, sd.vertices, "repeated", seed=1)
    calls = [("set_triangles", one), ("set_materials", (mat, rec)), ("set_triangles", again), ("set_emission", lamps.next()),
             ("set_triangles", other)]
    ob.set_libm_mode(1)
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
            h.r.frame(3)                                     # (reads the image back: the device has caught up after every frame ...
            assert_same(ref[f], h.direct_state(), f)         #  ... but the five edits of the gap are enqueued back to back)
    finally:
        hip.set_sync(True)
    assert differing(ref[1]["image"], ref[2]["image"]) > 0


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def refused(capi, code, call, *args):
    with pytest.raises(capi.RestirHipError) as e:
        call(*args)
    assert str(e.value).startswith("librestir_hip error %d:" % code), str(e.value)


def test_refusals_leave_scene_unchanged(hip):
    import torch
    sd = scene_data("cornell")
    o, h = OracleSide(hip, sd, W, H), HipSide(hip, sd, W, H)
    s = h.r.scene
    s.set_triangles(*geometry_edit(sd, sd.vertices, "one", seed=1))           # (an edited scene: the refit's tables exist)
    o.set_triangles(*geometry_edit(sd, sd.vertices, "one", seed=1))
    lo, hi = root_box(sd.vertices)
    p = int(movable(sd)[0])
    emissive = int(np.nonzero(sd.materials["type"][sd.material_ids] == 4)[0][0])
    tri = sd.vertices.reshape(-1, 3, 3)[[p]].copy()
    L = hip.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ids1 = np.array([p], np.int32)

    def moved(axis, value):
        t = tri.copy(); t[0, 1, axis] = value
        return t
    cases = [
        ("null ids", lambda: hip.check(L.rs_scene_set_triangles(s.handle, 1, None, ptr(tri), None))),
        ("null vertices", lambda: hip.check(L.rs_scene_set_triangles(s.handle, 1, ptr(ids1), None, None))),
        ("negative count", lambda: hip.check(L.rs_scene_set_triangles(s.handle, -1, ptr(ids1), ptr(tri), None))),
        ("id below", lambda: s.set_triangles([-1], tri)),
        ("id beyond", lambda: s.set_triangles([len(sd.material_ids)], tri)),
        ("NaN vertex", lambda: s.set_triangles([p], moved(0, np.nan))),
        ("infinite normal", lambda: s.set_triangles([p], tri, moved(2, np.inf))),
        ("an emissive triangle", lambda: s.set_triangles([emissive], tri)),
        ("second of two is emissive", lambda: s.set_triangles([p, emissive], np.concatenate([tri, tri]))),
        ("outside the root box, above", lambda: s.set_triangles([p], moved(1, np.nextafter(hi[1], np.float32(np.inf))))),
        ("outside the root box, below", lambda: s.set_triangles([p], moved(2, lo[2] - np.float32(1.0)))),
    ]
    desc, geometry = s.host_desc(), s.geometry()

    def unchanged(tag):
        d, g = s.host_desc(), s.geometry()
        assert bits_equal(d["boxes"], desc["boxes"]) and bits_equal(g[0], geometry[0]) and bits_equal(g[1], geometry[1]), tag
        o.r.frame(3); h.r.frame(3)
        assert_same(o.direct_state(), h.direct_state(), tag)
    for name, call in cases:
        refused(hip, 10001, call)                            # RS_ERR_INVALID_ARGUMENT
        unchanged(name)
    s.set_triangles(np.zeros(0, np.int32), np.zeros((0, 3, 3), np.float32))   # count == 0 succeeds and changes nothing
    unchanged("empty edit")
    s.set_triangles([p], moved(1, hi[1]))                   # on the box's face: inside
    o.set_triangles([p], moved(1, hi[1]))
    o.r.frame(3); h.r.frame(3)
    assert_same(o.direct_state(), h.direct_state(), "on the face")
    desc, geometry = s.host_desc(), s.geometry()

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
            refused(hip, 10002, s.set_triangles, [p], tri)
        finally:
            assert rt.hipStreamEndCapture(stream.cuda_stream, C.byref(graph)) == 0
            if graph:
                rt.hipGraphDestroy(graph)
    finally:
        hip.set_stream(None)
    unchanged("during capture")


# ---- 5. row bands -----------------------------------------------------------------------------------------------------------------------------
def test_row_bands_with_an_edit(hip):
    """rs_restir_phase_a / _phase_b on two bands, an edit between frames: the banded library equals the oracle's full frame."""
    sd = scene_data("cornell")
    bands = [(0, 19), (19, H)]
    o, h = OracleSide(hip, sd, W, H), HipSide(hip, sd, W, H)
    for f in range(5):
        if f in (2, 3):
            e = geometry_edit(sd, sd.vertices, ("all", "carry")[f - 2], seed=9)
            o.set_triangles(*e); h.set_triangles(*e)
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
