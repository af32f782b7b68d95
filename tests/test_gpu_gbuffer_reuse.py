"""GBuffer::render answered from retained planes (rs_gbuffer_set_reuse, include/restir_hip.h).

renderGBuffer (src/gbuffer.cu:3-73) reads the scene, the camera, lastCamera and the row range; it draws no random number.  A frame's
first render request that equals the two previous frames' in all of them launches nothing: the ring of plane sets steps back by one
(restir_amd/csrc/rs_internal.h, struct rs_gbuffer).  Every test here runs the runCuda sequence (render, ReSTIRDirect spatiotemporal,
update) twice, with reuse on and off, and compares after EVERY frame, bit for bit: the five planes of the current view, the three of the
"last" view, both reservoir buffers and the image.  The counters of rs_gbuffer_reuse_stats say which requests walked: a request is
answered from the planes exactly when its inputs equal those of the two frames before it, so hits begin with the fourth frame of a still
camera (the first frame has a zero lastCamera) and resume two frames after the inputs have settled again."""
import os
import subprocess

import numpy as np
import pytest

from tests.common import EmissionEdits, get_scene, hip_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 640, 360


_scenes = {}


def shared_scene(hip, name):
    """One library scene per scene name for the tests that do not edit it."""
    if name not in _scenes:
        _scenes[name] = hip_scene(hip, get_scene(name))
    return _scenes[name]


class Run:
    """One renderer and what a test may touch from its per-frame hook."""

    def __init__(self, hip, sd, scene, width, height, reuse):
        import torch
        self.torch, self.hip, self.sd = torch, hip, sd
        self.scene = scene
        self.W, self.H = width, height
        self.cam = hip.camera_update(sd.camera(width, height))
        self.gbuf = hip.GBuffer(width, height)
        self.gbuf.set_reuse(reuse)
        self.restir = hip.ReSTIR(width, height)
        self.image = torch.zeros((width * height, 3), dtype=torch.float32, device="cuda")
        self.rows = (0, height)
        self.looper = 0
        self.hits = []              # per frame: requests answered from retained planes
        self.walks = []             # per frame: requests that launched the walk
        self.snaps = []             # per frame: one uint8 tensor with everything that is compared
        self.extra = {}             # a test's own per-run objects

    def render(self, rows=None):
        y0, y1 = rows or self.rows
        self.gbuf.render(self.scene, self.cam, y0, y1)

    def snapshot(self):
        """Planes of the current and the last view, both reservoir buffers, the image -- copied on the library stream, no host wait."""
        torch, hip, n = self.torch, self.hip, self.W * self.H
        v = self.gbuf.view()
        f = v.frameIdx
        y0, y1 = self.rows          # albedo and motion: the rendered rows (nothing writes or reads the others: they hold what the set held)
        a, m = y0 * self.W, (y1 - y0) * self.W
        parts = [(v.devAlbedo + a * 12, m * 12), (v.devMotion + a * 4, m * 4), (v.devNormal[f], n * 12), (v.devPrimId[f], n * 4), (v.devDepth[f], n * 4),
                 (v.devNormal[f ^ 1], n * 12), (v.devPrimId[f ^ 1], n * 4), (v.devDepth[f ^ 1], n * 4)]
        resv = [self.restir.rows_bytes(k, self.H) for k in (0, 1)]
        out = torch.empty(sum(b for _, b in parts) + sum(resv) + n * 12, dtype=torch.uint8, device="cuda")
        at = out.data_ptr()
        for ptr, nbytes in parts:
            hip.hip_memcpy_d2d_async(at, ptr, nbytes)
            at += nbytes
        for k in (0, 1):
            self.restir.rows_pack(k, 0, self.H, at)
            at += resv[k]
        hip.hip_memcpy_d2d_async(at, self.image.data_ptr(), n * 12)
        return out

    def albedo_and_ids(self, frame):
        """Of a full-frame run."""
        n = self.W * self.H
        s = self.snaps[frame].cpu().numpy()
        return s[:n * 12].view(np.float32).reshape(n, 3), s[n * 28:n * 32].view(np.int32)


def sequence(hip, name, frames, reuse, overlapped, hook=None, scene=None, size=(W, H), rows=None, in_flight=3, after=None):
    """frames x (hook, GBuffer::render, ReSTIRDirect(3), after, snapshot, GBuffer::update) on the scene called `name`.  hook(run, frame)
    runs before the frame's render and may return "rendered" when it has issued the frame's render requests itself; after(run, frame) runs
    between ReSTIRDirect and GBuffer::update.  Overlapped: asynchronous launches, the host waits only after every `in_flight`-th frame."""
    torch = __import__("torch")
    run = Run(hip, get_scene(name), scene or shared_scene(hip, name), size[0], size[1], reuse)
    if rows:
        run.rows = rows
    hip.set_sync(not overlapped)
    try:
        for frame in range(frames):
            walked, reused = run.gbuf.reuse_stats()
            if not (hook and hook(run, frame) == "rendered"):
                run.render()
            w2, r2 = run.gbuf.reuse_stats()
            run.walks.append(w2 - walked); run.hits.append(r2 - reused)
            y0, y1 = run.rows
            run.restir.phase_a(run.scene, run.cam, run.gbuf, run.looper, 3, y0, y1)
            run.restir.phase_b(run.scene, run.cam, run.gbuf, run.image.data_ptr(), 0, 3, y0, y1)
            run.restir.end_frame()
            run.looper += 1
            if after:
                after(run, frame)
            run.snaps.append(run.snapshot())
            run.gbuf.update(run.cam)
            if overlapped and frame % in_flight == in_flight - 1:
                hip.synchronize()
        hip.synchronize(); torch.cuda.synchronize()
    finally:
        hip.set_sync(True)
    return run


def both(hip, name, frames, overlapped, expect_hits, hook=None, scenes=None, **kw):
    """Reuse on against reuse off: every frame's snapshot equal, the hits where expected (and only there), none with reuse off."""
    torch = __import__("torch")
    on = sequence(hip, name, frames, True, overlapped, hook, scene=scenes and scenes[0], **kw)
    off = sequence(hip, name, frames, False, overlapped, hook, scene=scenes and scenes[1], **kw)
    print("hits per frame, reuse on:", on.hits, "walks:", on.walks, "stats:", on.gbuf.reuse_stats(), "reuse off:", off.gbuf.reuse_stats())
    differing = [f for f in range(frames) if not torch.equal(on.snaps[f], off.snaps[f])]
    print("frames that differ from the reuse-off run:", differing)
    assert not differing, differing
    assert on.snaps[-1].any()
    assert off.gbuf.reuse_stats()[1] == 0 and sum(off.hits) == 0
    assert [f for f in range(frames) if on.hits[f]] == list(expect_hits), on.hits
    assert on.gbuf.reuse_stats() == (sum(on.walks), sum(on.hits))
    return on, off


# ---- 1. still camera -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["synchronous", "overlapped", "overlapped_strip_rows"])
def test_still_camera_equals_reuse_off(hip, mode):
    """12 frames of a scaled Sponza-class scene: three renders, nine requests answered from the planes; nothing differs."""
    frames = 12
    rows = (96, 240) if mode == "overlapped_strip_rows" else None
    on, off = both(hip, "sponza:0.2", frames, mode != "synchronous", range(3, frames), rows=rows)
    assert on.gbuf.reuse_stats() == (3, frames - 3)
    assert off.gbuf.reuse_stats() == (frames, 0)


# ---- 2. every condition that must render -----------------------------------------------------------------------------------------------

def _change_camera(field):
    def hook(run, frame):
        if frame != 5:
            return
        cam = run.cam
        if field == "position":
            cam.position[0] += 0.05
            run.hip.camera_update(cam)
        elif field == "fov":
            cam.fov[1] += 1.0
            run.hip.camera_update(cam)
        elif field == "basis":          # one basis vector alone (the bytes of the camera are the key, not what produced them)
            cam.up[0] += 1e-3
        elif field == "focal":
            cam.focalDist += 0.125
    return hook


@pytest.mark.parametrize("field", ["position", "basis", "fov", "focal"])
@pytest.mark.parametrize("overlapped", [False, True])
def test_camera_change_renders(hip, field, overlapped):
    """One camera field changes before frame 5.  Frame 5 differs in the camera, frame 6 in lastCamera, frame 7 has frame 5 two frames
    back: three renders, hits from frame 8 on."""
    both(hip, "sponza:0.2", 11, overlapped, [3, 4, 8, 9, 10], _change_camera(field))


def test_emission_edit_renders(hip):
    """rs_scene_set_emission before frame 5 changes baseColor, hence the albedo plane: frames 5 and 6 render (the edit is in both their
    keys, not in frame 4's), hits from frame 7 on, and the lamps' albedo is the edited one."""
    sd = get_scene("cornell")
    ids, rad = EmissionEdits(sd, 7).next()

    def hook(run, frame):
        if frame == 5:
            run.scene.set_emission(ids, rad)

    on, off = both(hip, "cornell", 10, True, [3, 4, 7, 8, 9], hook, scenes=(hip_scene(hip, sd), hip_scene(hip, sd)))
    a4, id4 = on.albedo_and_ids(4)
    a5, id5 = on.albedo_and_ids(5)
    b5, _ = off.albedo_and_ids(5)
    lamps = id5 == -2
    assert lamps.any() and np.array_equal(id4, id5)
    assert not np.array_equal(a4[lamps], a5[lamps])                  # the edit is visible ...
    assert a5[lamps].tobytes() == b5[lamps].tobytes()                # ... and is the one the walk writes
    assert a4[~lamps].tobytes() == a5[~lamps].tobytes()


def test_alternating_scenes_render(hip):
    """Two scenes of the same geometry (two ids) take turns from frame 4 to frame 9 (B A B A B A); frame 10 still has the other scene two
    frames back; hits from frame 11 on."""
    sd = get_scene("sponza:0.2")

    def hook(run, frame):
        if "a" not in run.extra:
            run.extra["a"], run.extra["b"] = run.scene, hip_scene(hip, sd)
        run.scene = run.extra["b"] if (4 <= frame < 10 and frame % 2 == 0) else run.extra["a"]

    both(hip, "sponza:0.2", 14, True, [3, 11, 12, 13], hook)


def test_another_row_range_renders(hip):
    """The rows change from the whole frame to its upper half before frame 5: frames 5 and 6 render.  Rows outside a render belong to
    the caller (a strip driver puts its neighbours' rows there before anything reads them): from frame 5 on the lower half of the id /
    normal / depth planes of both views is written with rs_gbuffer_rows_unpack after the render -- outside the rendered rows, so the
    planes stay what the requests describe."""
    torch = __import__("torch")

    def hook(run, frame):
        if frame >= 5:
            run.rows = (0, H // 2)
            run.render()
            zeros = torch.zeros(run.gbuf.rows_bytes(H - H // 2), dtype=torch.uint8, device="cuda")
            for sel in (0, 1):
                run.gbuf.rows_unpack(sel, H // 2, H - H // 2, zeros.data_ptr())
            run.extra.setdefault("keep", []).append(zeros)
            return "rendered"

    both(hip, "sponza:0.2", 10, True, [3, 4, 7, 8, 9], hook)


def test_update_without_render_renders(hip):
    """An extra GBuffer::update before frame 5 -- a frame without a render: its set is not the previous frame's planes."""
    def hook(run, frame):
        if frame == 5:
            run.gbuf.update(run.cam)

    both(hip, "sponza:0.2", 10, True, [3, 4, 7, 8, 9], hook)


@pytest.mark.parametrize("overlapped", [False, True])
def test_two_renders_in_one_frame(hip, overlapped):
    """Frame 5 renders the whole frame and then rows 0..H/2 again: the first request is still answered from the planes, the second always
    walks and leaves the set without a key, so frames 6 and 7 render."""
    def hook(run, frame):
        if frame == 5:
            run.render()
            run.render((0, H // 2))
            return "rendered"

    on, _ = both(hip, "sponza:0.2", 11, overlapped, [3, 4, 5, 8, 9, 10], hook)
    assert on.hits[5] == 1 and on.walks[5] == 1


@pytest.mark.parametrize("where", ["inside", "outside"])
def test_rows_unpack(hip, where):
    """rs_gbuffer_rows_unpack into the "last" planes before frame 5 (the rows' own content, packed just before).  The renders cover rows
    96..240: rows 100..110 are part of what the key describes (frames 5 and 6 render), rows 0..10 are not (nothing changes)."""
    torch = __import__("torch")
    y = 100 if where == "inside" else 0

    def hook(run, frame):
        if frame == 5:
            buf = torch.empty(run.gbuf.rows_bytes(10), dtype=torch.uint8, device="cuda")
            run.gbuf.rows_pack(1, y, 10, buf.data_ptr())
            run.gbuf.rows_unpack(1, y, 10, buf.data_ptr())
            run.hip.synchronize()

    both(hip, "sponza:0.2", 10, True, [3, 4, 7, 8, 9] if where == "inside" else range(3, 10), hook, rows=(96, 240))


@pytest.mark.parametrize("how", ["invalidate", "set_reuse"])
def test_invalidate_renders(hip, how):
    """rs_gbuffer_invalidate (or reuse switched off and on again) before frame 5 forgets what the sets hold: frames 5 and 6 render."""
    def hook(run, frame):
        if frame == 5:
            if how == "invalidate":
                run.gbuf.invalidate()
            elif run.gbuf.reuse_stats()[1]:          # (the reuse-off run stays off)
                run.gbuf.set_reuse(False); run.gbuf.set_reuse(True)

    both(hip, "sponza:0.2", 10, True, [3, 4, 7, 8, 9], hook)


def test_denoise_stream_mode_renders(hip):
    """rs_set_denoise_stream(1) during frames 5 and 6, LeveledEAWFilter after every frame's ReSTIRDirect (on the denoise stream in those
    two frames): they render and their sets take no key, so frames 7 and 8 render too; hits from frame 9 on.  The filtered images are
    compared as well."""
    torch = __import__("torch")

    def hook(run, frame):
        if frame in (5, 7):
            run.hip.synchronize()
            run.hip.set_denoise_stream(1 if frame == 5 else 0)

    def after(run, frame):
        if "filter" not in run.extra:
            run.extra.update(filter=run.hip.EAWFilter(W, H, 5), out=torch.zeros_like(run.image), shown=[])
        p = run.extra["filter"].filter(run.extra["out"].data_ptr(), run.image.data_ptr(), run.gbuf, run.cam)
        run.hip.join_denoise_stream()
        t = torch.empty_like(run.image)
        run.hip.hip_memcpy_d2d_async(t.data_ptr(), p, t.numel() * 4)
        run.extra["shown"].append(t)

    try:
        on, off = both(hip, "sponza:0.2", 12, True, [3, 4, 9, 10, 11], hook, after=after)
    finally:
        hip.synchronize()
        hip.set_denoise_stream(0)
    assert all(torch.equal(a, b) for a, b in zip(on.extra["shown"], off.extra["shown"])) and on.extra["shown"][-1].any()
    for run in (on, off):
        run.extra["filter"].destroy()


# ---- 3. orbit --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("overlapped", [False, True])
def test_orbiting_camera_never_reuses(hip, overlapped):
    from restir_amd.scenes import orbit_position
    sd = get_scene("sponza:0.2")

    def hook(run, frame):
        p = orbit_position(sd.camera_args["position"], frame, radius=0.5)
        for i in range(3):
            run.cam.position[i] = float(p[i])
        run.hip.camera_update(run.cam)

    on, _ = both(hip, "sponza:0.2", 12, overlapped, [], hook)
    assert on.gbuf.reuse_stats() == (12, 0)


# ---- 4. strip driver -------------------------------------------------------------------------------------------------------------------

def test_strip_driver_ranks_reuse_their_rows():
    """restir_amd/host/strips_loopback_ranks.cpp, three ranks as threads over the loopback transport: with a static camera every rank's
    strip (and rank 0's full frame) renders three times and then answers from its planes, without the filter, with rs_strips_eaw_filter,
    and (static-halo) with rs_strips_set_gbuffer_halo(32) next to the filter; the gathered frames equal the full frame in every mode."""
    exe = os.path.join(ROOT, "restir_amd", "host", "strips_loopback_ranks")
    assert os.path.exists(exe), "restir_amd/host/strips_loopback_ranks is built by restir_amd/csrc/Makefile"
    r = subprocess.run([exe, "3", "200", "static-halo"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "strips_loopback_ranks ok (3 ranks)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("== full frame over 6 frames: True") == 12, r.stdout[-3000:]
    assert "UNEXPECTED" not in r.stdout
    for rank in range(3):
        for mode in (0, 2, 4, 6):                     # static camera: library stream / own transfer stream, without / with the filter
            assert "rank %d, mode %d, strip G-buffer: rendered 3, reused 3: as expected" % (rank, mode) in r.stdout, (rank, mode)
        for mode in (1, 3, 5, 7, 8, 9, 10, 11):       # orbit, and everything on the denoise stream
            assert "rank %d, mode %d, strip G-buffer: rendered 6, reused 0: as expected" % (rank, mode) in r.stdout, (rank, mode)


# ---- 5. full size ----------------------------------------------------------------------------------------------------------------------

def test_full_size_config3(hip):
    """1920x1080, the full config-3 scene, ten overlapped frames: seven requests answered from the planes, every frame equal."""
    torch = __import__("torch")
    on = sequence(hip, "sponza:1.0", 10, True, True, size=(1920, 1080))
    off = sequence(hip, "sponza:1.0", 10, False, True, size=(1920, 1080))
    print("reuse on:", on.gbuf.reuse_stats(), on.hits, "reuse off:", off.gbuf.reuse_stats())
    assert all(torch.equal(a, b) for a, b in zip(on.snaps, off.snaps))
    assert on.snaps[-1].any()
    assert on.gbuf.reuse_stats() == (3, 7) and off.gbuf.reuse_stats() == (10, 0)
