"""Object motion vectors (rs_scene_set_motion_tracking, rs_scene_advance_motion) against the CPU oracle: the motion plane of a tracked
scene equals tests/motion_vectors.py's statement of it bit for bit, and every consumer of the plane -- ReSTIRDirect, ReSTIRIndirect at
depth 3, SpatioTemporalFilter -- equals the oracle fed that plane.  Every case runs in four launch modes (MODES): synchronous
(k_render_gbuffer*) and overlapped (rs_set_side_stream(4): the render deferred into k_gbuffer_primary*), each with the library's
tile-split threshold and with rs_set_tile_split(8).  Under a threshold of 8 practically every tile is listed as heavy, and a launch site
hands its list to its own NEXT launch: of the same rows, on the same stream, in the same split mode.  split_ran() asks the library
(rs_debug_split_tiles) whether helper blocks really took tiles in the kernel that wrote the G-buffer, wherever the case makes that
certain.  Synchronous: one site, so from the second whole-frame render on.  Overlapped: the frames' chains take three streams in turn and a
frame that finds the device idle takes another split mode than one that does not, so certain only where the host reads every frame back
(every frame after the first then finds the device idle) and from the fifth frame on -- the edit-kind cases, which start with three frames
at rest so that the frame of the edit is such a frame, and the tracking-off case; not the twenty frames in flight.  Never in the row-band
case: its three bands alternate on one site and no band meets its own list.

What the cases are and why each gap holds the slide of the centre triangles next to the kind's own edit: tests/motion_vectors.py
(case_edits) and tests/test_motion_vectors_cases.py, which establishes on the CPU that every case moves at least 50 pixels of the plane.

SpatioTemporalFilter is the one output compared within a tolerance, the stated one of rs_svgf_filter against the oracle (rtol 3e-5,
atol 2e-6 on the colour: tests/denoise_cases.py SVGF_COLOUR_TOL, as tests/test_gpu_denoise_edges.py applies it at radiance scale 1)."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import binding as ob
from tests import denoise_cases as dc
from tests import motion_vectors as mv
from tests.common import bits_equal, next_looper
from tests.geometry_edits import apply_triangles, geometry_edit
from tests.scene_edits import assert_same, differing

pytestmark = pytest.mark.gpu

W, H = mv.W, mv.H
MODES = [(overlapped, split) for overlapped in (False, True) for split in (768, 8)]      # 768: the library's default threshold
in_every_mode = pytest.mark.parametrize("overlapped,split", MODES, ids=["sync", "sync_split8", "overlapped", "overlapped_split8"])


@pytest.fixture(autouse=True)
def exact_libm(hip):
    ob.set_libm_mode(1)            # cos / sin correctly rounded on both sides: every bit must agree
    hip.set_sync(True)
    yield
    ob.set_libm_mode(0)
    hip.set_sync(True)
    hip.set_side_stream(4)         # the library's default
    hip.set_tile_split(768)


@contextlib.contextmanager
def launch_mode(hip, overlapped, split):
    hip.set_tile_split(split)
    hip.set_side_stream(4)
    hip.set_sync(not overlapped)
    try:
        yield
    finally:
        hip.synchronize()
        hip.set_sync(True)
        hip.set_tile_split(768)


def split_ran(hip, h, overlapped, split):
    """Under rs_set_tile_split(8): helper blocks took tiles in the last split launch of the kernel that writes the G-buffer -- the render's
    own launch, or the primary rays' when the render went out with them (overlapped ReSTIR-DI)."""
    if split != 8:
        return
    render, primary = hip.split_tiles(h.gbuf, h.restir)
    fused = overlapped and h.pipeline == "direct_svgf" and h.restir.last_launch()[0] == 1
    assert (primary if fused else render) > 0, (overlapped, fused, render, primary)


def same_state(ref, got, tag):
    """Bit for bit, except the filtered image: within one unit of the stated SVGF colour tolerance."""
    ref, got = dict(ref), dict(got)
    a, b = ref.pop("filtered", None), got.pop("filtered", None)
    assert_same(ref, got, tag)
    if a is not None:
        u = float(dc.svgf_units("colour", b, a, 1.0).max())
        assert u <= 1.0, (tag, "filtered", u)


# ---- 1. tracking on, nothing moved --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mv.SCENES) + [mv.TEXTURED])
def test_tracked_scene_at_rest_equals_untracked(hip, name):
    """Three ReSTIR-DI frames with a camera move: a tracked scene whose geometry never moved is bit-identical to an untracked one in image,
    both reservoir buffers, ray count and all G-buffer planes (the MOTION kernels on one side, the parent's on the other), and
    Scene.prev_vertices() equals the vertices.  cornell_textured (maps and an environment map) takes the textured instantiations."""
    sd = mv.scene_data(name)
    base = np.array(sd.camera_args["position"], np.float32)
    for overlapped, split in MODES:
        with launch_mode(hip, overlapped, split):
            sides = [mv.HipMotion(hip, sd, tracked=t) for t in (False, True)]
            for f in range(3):
                states = []
                for s in sides:
                    if f:
                        s.set_camera_position(base + np.float32(0.15 * f) * np.array([1, -0.5, 0.25], np.float32))
                    s.advance()
                    states.append(s.frame())
                same_state(states[0], states[1], (name, overlapped, split, f))
            assert bits_equal(sides[1].scene.prev_vertices(), sides[1].scene.geometry()[0])
            assert differing(states[1]["motion"], np.arange(W * H, dtype=np.int32)) > 0      # the camera moved: not the identity
            if not overlapped:
                split_ran(hip, sides[1], overlapped, split)
            for s in sides:
                s.destroy()


# ---- 2. every edit kind, every consumer ---------------------------------------------------------------------------------------------------
CASES = [(name, kind) for name in mv.SCENES for kind in mv.kinds_for(name)] + [(mv.TEXTURED, kind) for kind in mv.TEXTURED_KINDS]


@pytest.mark.parametrize("pipeline", mv.PIPELINES)
@pytest.mark.parametrize("name,kind", CASES)
def test_edit_kind_against_the_oracle(hip, name, kind, pipeline):
    """frame, edit, frame, advance, frame with no edit, advance, frame.  After every frame the motion plane equals the helper's and the
    image, the reservoirs (`last` / `temp`, or ReSTIR-GI's), the ray count and the other planes the oracle's; the SVGF result within its
    tolerance.  The frame of the edit differs from the camera-only plane; the frames after each advance have it again.  The cases on
    cornell_textured run the textured instantiations of the kernels."""
    sd = mv.scene_data(name)
    ref, camera_only = mv.oracle_case(name, kind, pipeline)
    assert int((ref[1]["motion"] != camera_only[1]).sum()) >= 50
    for overlapped, split in MODES:
        with launch_mode(hip, overlapped, split):
            h = mv.HipMotion(hip, sd, pipeline=pipeline)
            got = mv.run_case(h, name, kind, on_frame=lambda f: f >= 1 and split_ran(hip, h, overlapped, split))     # from the frame of the edit on
            for f in range(4):
                assert np.array_equal(got[f]["motion"], ref[f]["motion"]), (name, kind, overlapped, split, f, differing(got[f]["motion"], ref[f]["motion"]))
                same_state(ref[f], got[f], (name, kind, pipeline, overlapped, split, f))
            for f in (0, 2, 3):
                assert np.array_equal(got[f]["motion"], camera_only[f]), f
            if pipeline == "direct_svgf":
                assert h.restir.last_launch()[0] == (1 if overlapped else 0)      # overlapped: the render went out inside k_gbuffer_primary*
            h.destroy()


# ---- 3. several edits in one gap, then one advance --------------------------------------------------------------------------------------
@in_every_mode
@pytest.mark.parametrize("name", list(mv.SCENES))
def test_previous_pose_is_the_pose_at_the_last_advance(hip, name, overlapped, split):
    """Previous means the pose at the last advance, not the pose before the last edit: after each step Scene.prev_vertices() equals the NumPy
    bookkeeping bit for bit, and triangles never named keep their original vertices."""
    sd = mv.scene_data(name)
    orig = sd.vertices.reshape(-1, 3, 3).copy()
    with launch_mode(hip, overlapped, split):
        h = mv.HipMotion(hip, sd)
        cur, nrm, prev = orig.copy(), sd.normals.reshape(-1, 3, 3).copy(), orig.copy()
        named = set()
        steps = [("edit", "one"), ("edit", "repeated"), ("edit", "one"), ("frame",), ("edit", "carry"), ("advance",), ("frame",), ("edit", "all"),
                 ("edit", "carry_back"), ("advance",), ("advance",), ("edit", "repeated"), ("frame",), ("advance",)]
        for i, step in enumerate(steps):
            if step[0] == "edit":
                ids, v, n = geometry_edit(sd, cur, step[1], seed=i)
                if step[1] == "all":                         # half of them: some triangles stay unnamed to the end
                    ids, v = ids[::2], np.asarray(v)[::2]
                h.set_triangles(ids, v, n)
                cur, nrm = apply_triangles(cur, nrm, ids, v, n)
                named.update(int(p) for p in ids)
            elif step[0] == "advance":
                h.advance()
                prev = cur.copy()
            else:
                h.enqueue()
            got = h.scene.prev_vertices()
            assert bits_equal(got, prev), (i, step, differing(got.reshape(-1, 9), prev.reshape(-1, 9)))
        never = np.array(sorted(set(range(len(orig))) - named), np.int32)
        assert len(never) > 0 and bits_equal(got[never], orig[never]) and bits_equal(h.scene.geometry()[0], cur)
        assert differing(prev.reshape(-1, 9), orig.reshape(-1, 9)) > 0
        if not overlapped:
            split_ran(hip, h, overlapped, split)
        h.destroy()


# ---- 4. twenty overlapped frames, an edit and an advance in every gap ----------------------------------------------------------------------
N_FLIGHT = 20


@functools.lru_cache(maxsize=None)
def flight_edits(name):
    sd = mv.scene_data(name)
    cur, nrm = sd.vertices.reshape(-1, 3, 3).copy(), sd.normals.reshape(-1, 3, 3).copy()
    ids = mv.centre_triangles(sd, mv.SLIDE_COUNT[name])
    lo, hi = cur.reshape(-1, 3).min(0), cur.reshape(-1, 3).max(0)
    out = []
    for f in range(N_FLIGHT):
        if f % 3 == 2:
            e = ("set_triangles",) + tuple(geometry_edit(sd, cur, "all", seed=100 + f))
        else:
            step = (hi - lo).astype(np.float32) * np.float32(0.04) * np.array([np.cos(f), 0.5 * np.sin(f), -0.25], np.float32)
            e = ("set_triangles", ids, np.clip(cur[ids] + step, lo, hi).astype(np.float32), None)
        cur, nrm = apply_triangles(cur, nrm, e[1], e[2], e[3])
        out.append(e)
    return out


@functools.lru_cache(maxsize=None)
def oracle_flight(name):
    from restir_amd import capi
    ob.set_libm_mode(1)
    o = mv.OracleMotion(capi, mv.scene_data(name))
    images, moved = [], 0
    for e in flight_edits(name):
        mv.apply(o, e)
        st = o.frame()
        images.append(st["image"])
        moved += int((st["motion"] != o.camera_only).sum())
        o.advance()
    return images, st, moved


@pytest.mark.parametrize("name", list(mv.SCENES))
def test_twenty_frames_in_flight(hip, name):
    """rs_set_sync(0): twenty frames, before each an edit and after each an advance, no rs_synchronize in between; every frame's image is
    copied device to device and read at the end.  Every frame and the final state equal the oracle's and the synchronous run's, with
    either tile-split threshold."""
    import torch
    sd = mv.scene_data(name)
    ref, final, moved = oracle_flight(name)
    assert moved >= 50 * N_FLIGHT // 2
    results = []
    for overlapped, split in MODES:
        with launch_mode(hip, overlapped, split):
            h = mv.HipMotion(hip, sd)
            outs = [torch.zeros((W * H, 3), dtype=torch.float32, device="cuda") for _ in range(N_FLIGHT)]
            for f, e in enumerate(flight_edits(name)):
                mv.apply(h, e)
                h.enqueue()
                hip.hip_memcpy_d2d_async(outs[f].data_ptr(), h.image.data_ptr(), W * H * 12)
                h.advance()
            st = h.state()
            images = [o.cpu().numpy() for o in outs]
            for f in range(N_FLIGHT):
                assert bits_equal(ref[f], images[f]), (overlapped, split, f, differing(ref[f], images[f]))
            same_state(final, st, (name, overlapped, split, "final"))
            if not overlapped:
                split_ran(hip, h, overlapped, split)
            results.append((images, st))
            h.destroy()
    for images, st in results[1:]:
        for f in range(N_FLIGHT):
            assert bits_equal(results[0][0][f], images[f])
        assert_same(results[0][1], st, "synchronous against the other modes")


# ---- 5. retained planes -------------------------------------------------------------------------------------------------------------------
@in_every_mode
def test_retained_planes(hip, overlapped, split):
    """rs_gbuffer_set_reuse(1), still camera, an advance after every frame.  A request is answered from retained planes when its key equals
    the keys of BOTH previous frames (rs_gbuffer_render_rows), so: three renders, then reuse -- an advance with nothing to copy leaves the
    scene's edit count alone; the edit makes its frame render; the advance that copies makes the next frame render (its motion plane is
    the camera-only one again, not the one of the frame of the move); the frame after that still has the frame of the move two back, and
    renders; from then on the requests are answered from the planes again.  Every frame equals the oracle's."""
    from restir_amd import capi
    sd = mv.scene_data("cornell")
    o = mv.OracleMotion(capi, sd)
    edit = mv.case_edits("cornell", mv.SLIDE)[1][0]
    with launch_mode(hip, overlapped, split):
        h = mv.HipMotion(hip, sd)
        h.gbuf.set_reuse(True)
        stats = []
        for f in range(10):
            if f == 5:
                mv.apply(o, edit); mv.apply(h, edit)
            same_state(o.frame(), h.frame(), f)
            stats.append(h.gbuf.reuse_stats())
            o.advance(); h.advance()
        if not overlapped:                                   # (overlapped: the six renders of the ten frames spread over three streams' sites)
            split_ran(hip, h, overlapped, split)
        h.destroy()
    rendered = [stats[0][0]] + [b[0] - a[0] for a, b in zip(stats, stats[1:])]
    assert rendered == [1, 1, 1, 0, 0, 1, 1, 1, 0, 0], stats
    assert stats[-1] == (6, 4), stats


# ---- 6. row bands ---------------------------------------------------------------------------------------------------------------------------
@in_every_mode
def test_row_bands(hip, overlapped, split):
    """rs_gbuffer_render_rows and rs_restir_phase_a / _phase_b over three bands, an edit before and an advance after every frame from the
    third on: the banded library equals the oracle's full frame."""
    from restir_amd import capi
    sd = mv.scene_data("cornell")
    bands = [(0, 13), (13, 30), (30, H)]
    o = mv.OracleMotion(capi, sd)
    edits = flight_edits("cornell")
    with launch_mode(hip, overlapped, split):
        h = mv.HipMotion(hip, sd)
        moved = 0
        for f in range(6):
            if f >= 2:
                mv.apply(o, edits[f]); mv.apply(h, edits[f])
            a = o.frame()
            moved += int((a["motion"] != o.camera_only).sum())
            for y0, y1 in bands:
                h.gbuf.render(h.scene, h.cam, y0, y1)
            for y0, y1 in bands:
                h.restir.phase_a(h.scene, h.cam, h.gbuf, h.looper, 3, y0, y1)
            for y0, y1 in bands:
                h.restir.phase_b(h.scene, h.cam, h.gbuf, h.image.data_ptr(), 0, 3, y0, y1)
            h.restir.end_frame()
            h.looper = next_looper(h.looper, None)
            h.gbuf.update(h.cam)
            b = h.state()
            for k in ("rays", "filtered"):                   # (the banded launches count their rays per band; no filter in this loop)
                a.pop(k); b.pop(k)
            assert_same(a, b, f)
            o.advance(); h.advance()
        assert moved >= 50
        h.destroy()


# ---- 7. tracking switched off mid-sequence ----------------------------------------------------------------------------------------------------
@in_every_mode
@pytest.mark.parametrize("name", list(mv.SCENES))
def test_tracking_switched_off(hip, name, overlapped, split):
    """frame, edit, frame (tracked: the object plane), edit, tracking off, frame: the camera-only plane and the untracked oracle; on again,
    edit, frame: the object plane again, the previous pose being the pose at the switch."""
    from restir_amd import capi
    sd = mv.scene_data(name)
    o = mv.OracleMotion(capi, sd)
    edits = flight_edits(name)
    with launch_mode(hip, overlapped, split):
        h = mv.HipMotion(hip, sd)
        script = [(None, None), (edits[0], None), (edits[1], False), (None, True), (edits[2], None)]
        differs = []
        for f, (edit, switch) in enumerate(script):
            if edit:
                mv.apply(o, edit); mv.apply(h, edit)
            if switch is not None:
                o.set_tracking(switch); h.set_tracking(switch)
            same_state(o.frame(), h.frame(), (name, f))
            differs.append(int((o.gbuf.motion != o.camera_only).sum()))
        assert differs[0] == 0 and differs[1] >= 50 and differs[2] == 0 and differs[3] == 0 and differs[4] >= 50, differs
        split_ran(hip, h, overlapped, split)                 # (overlapped: the fifth frame, on the second frame's stream)
        h.destroy()


# ---- 8. refusals and no-ops -------------------------------------------------------------------------------------------------------------------
def refused(capi, code, call, *args):
    with pytest.raises(capi.RestirHipError) as e:
        call(*args)
    assert str(e.value).startswith("librestir_hip error %d:" % code), str(e.value)


def test_refusals_and_noops(hip):
    import torch
    from restir_amd import capi
    sd = mv.scene_data("cornell")
    L = hip.lib()
    out = np.zeros((len(sd.material_ids), 3, 3), np.float32)
    ptr = out.ctypes.data_as(C.c_void_p)
    refused(hip, 10001, lambda: hip.check(L.rs_scene_set_motion_tracking(None, 1)))       # RS_ERR_INVALID_ARGUMENT
    refused(hip, 10001, lambda: hip.check(L.rs_scene_advance_motion(None)))
    refused(hip, 10001, lambda: hip.check(L.rs_scene_download_prev_vertices(None, ptr)))
    o, h = mv.OracleMotion(capi, sd, tracked=False), mv.HipMotion(hip, sd, tracked=False)
    refused(hip, 10001, h.scene.prev_vertices)                                             # an untracked scene
    edit = mv.case_edits("cornell", mv.SLIDE)[1][0]
    for f in range(3):                                       # an advance on an untracked scene succeeds and changes no frame
        if f == 1:
            mv.apply(o, edit); mv.apply(h, edit)
        same_state(o.frame(), h.frame(), f)
        h.advance()
    refused(hip, 10001, h.scene.prev_vertices)
    h.set_tracking(True)
    refused(hip, 10001, lambda: hip.check(L.rs_scene_download_prev_vertices(h.scene.handle, None)))
    assert bits_equal(h.scene.prev_vertices(), h.scene.geometry()[0])
    h.set_tracking(True)                                     # twice: nothing
    h.set_tracking(False)
    refused(hip, 10001, h.scene.prev_vertices)
    h.set_tracking(True)

    # while the library stream is being captured into a graph: RS_ERR_UNSUPPORTED, the scene unchanged
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
            refused(hip, 10002, h.scene.advance_motion)
            refused(hip, 10002, h.scene.set_motion_tracking, False)
            refused(hip, 10002, h.scene.prev_vertices)
        finally:
            assert rt.hipStreamEndCapture(stream.cuda_stream, C.byref(graph)) == 0
            if graph:
                rt.hipGraphDestroy(graph)
    finally:
        hip.set_stream(None)
    o.set_tracking(True)
    same_state(o.frame(), h.frame(), "after the capture")
    assert bits_equal(h.scene.prev_vertices(), h.scene.geometry()[0])
    h.destroy()
