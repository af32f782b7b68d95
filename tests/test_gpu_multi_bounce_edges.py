"""GPU: the multi-bounce kernel k_path (restir_amd/csrc/gi.hip: rs_path_trace, rs_path_trace_indirect, rs_restir_indirect) off the 32 x 8
tile grid, past the clamp of the indirect reservoir, on degenerate scenes and with the switches that no other module flips, held to
the CPU oracle bit for bit: images, ray counts and the 68-byte indirect reservoirs.  Nothing here has a tolerance.  The oracle runs with
its cos / sin / atan2 correctly rounded (libm mode 1), as the device evaluates them.

  A. Ragged frames (97 x 61, 33 x 9, 41 x 27, one partial block 31 x 7, one wave and one row 8 x 1, one pixel): lanes with
     x >= width or y >= height walk with their wave and never start a path; at width 33 three of the four waves of the second block
     column have no lane inside the frame.  In ReSTIR-GI such a lane parks its four recorded points in pixel 0's slot of the output
     reservoirs, which therefore is asserted on its own.  Default sampler and Sobol table, plain / textured + environment-lit / larger
     scene, the sequence of test_multi_bounce_kernels_bit_exact and the shallow depths 1 and 2.
  B. The same entry points write nothing outside the caller's images: each image lies between two bands of 8 * (W + 32) pixels
     filled with a NaN payload that no arithmetic produces; the bands come back unchanged and the frame equals the oracle's.
     (Every image of this module is held in such a buffer; elsewhere the bands are empty.)
  C. 26 frames of temporal reuse on a still camera: M reaches 20 at frame index 19 and clamp<20>() (restir.h:79-86: W *= 20 / M)
     acts from frame index 20 on, on at least half of the pixels; then four frames of an orbit, which reproject the clamped
     reservoirs through the motion plane.
  D. The scenes of _edge_scene (no lights, BSDFs that evaluate to zero, one triangle, the light alone) and the scene without
     extent through all three entry points.
  E. maxDepth 0, reuse 0, rs_restir_reset between indirect frames, the first-frame flag that rs_restir_direct and
     rs_restir_indirect share, the Sobol guard (depth 613 refused, 612 accepted) and the size checks of rs_restir_indirect.
  F. The BVH-walk counters belong to the context: two host threads, each with its own context, stream and frame size, get the
     counts and images of the same calls made single-threaded on the default context.

The oracle's own figures asserted as non-vacuity (ray counts 3540 / 1164 / 1107 / 297, M = frame + 1 up to 20, at least half of the
pixels at M = 20 from frame index 20 on) were checked on the CPU with the oracle alone.

What the module found: nothing in gi.hip or the wave services; every comparison holds on an MI355X (33 tests, 4.2 s).
"""
import numpy as np
import pytest

from oracle import binding as ob
from restir_amd import sobol
from restir_amd.scenes import orbit_position
from tests.common import HipRenderer, OracleRenderer, bits_equal, get_scene, radiance_stats
from tests.test_gpu_parity import _compare_reservoirs, _edge_scene, _gi_scene

pytestmark = pytest.mark.gpu

_DEV = "cuda"
BAND_BITS = -3824719                   # 0xFFC5A3B1 as int32: a NaN with a payload, which no arithmetic produces
IND_FIELDS = ("Lo", "xv", "nv", "xs", "ns", "weight")


@pytest.fixture(scope="module")
def table():
    return sobol.sobol_table()


@pytest.fixture(autouse=True)
def exact_libm():
    ob.set_libm_mode(1)
    yield
    ob.set_libm_mode(0)


def _band(width):
    return 8 * (width + 32)


class _DevImage:
    """A float32 [n, 3] image on the device between two bands of `band` pixels that hold BAND_BITS; get() returns the frame after
    checking that both bands still do."""

    def __init__(self, n, band=0):
        import torch
        self.n, self.band = n, band
        self.t = torch.full(((n + 2 * band) * 3,), BAND_BITS, dtype=torch.int32, device=_DEV)
        self.zero()

    def zero(self):
        self.t[self.band * 3:(self.band + self.n) * 3] = 0

    @property
    def ptr(self):
        return self.t.data_ptr() + self.band * 12

    def bits(self):
        return self.t.cpu().numpy().copy()

    def get(self):
        a, b = self.bits(), self.band * 3
        assert (a[:b] == BAND_BITS).all(), ("written before the caller's image", np.nonzero(a[:b] != BAND_BITS)[0][:8] - b)
        assert (a[b + self.n * 3:] == BAND_BITS).all(), ("written behind the caller's image", np.nonzero(a[b + self.n * 3:] != BAND_BITS)[0][:8])
        return a[b:b + self.n * 3].view(np.float32).reshape(self.n, 3)


def _same_reservoirs(a, b, where):
    """a: the oracle's indirect reservoirs, b: the library's.  Pixel 0 first: it is the slot that lanes outside the frame alias."""
    assert a[:1].tobytes() == b[:1].tobytes(), ("pixel 0's reservoir, where the lanes outside the frame park their recorded points", where, a[0], b[0])
    assert np.array_equal(a["numSamples"], b["numSamples"]), (where, "numSamples", np.nonzero(a["numSamples"] != b["numSamples"])[0][:8])
    for k in IND_FIELDS:
        assert bits_equal(a[k], b[k]), (where, k)
    assert a.tobytes() == b.tobytes(), where


class _Pair:
    """The oracle and the library on one scene and frame size, driven through the same calls; every call asserts that its ray
    counts, images and reservoirs are equal."""

    def __init__(self, hip, sd, size, table=None, share=None, band=0):
        self.hip, self.sd = hip, sd
        self.W, self.H = size
        n = self.n = self.W * self.H
        self.o = OracleRenderer(sd, self.W, self.H, scene=share.o.scene if share else None, sobol=table)
        self.h = HipRenderer(hip, sd, self.W, self.H, scene=share.h.scene if share else None, sobol=table)
        self.od = np.zeros((n, 3), np.float32); self.oi = np.zeros((n, 3), np.float32)
        self.hd = _DevImage(n, band); self.hi = _DevImage(n, band)

    def clear(self):
        self.od[:] = 0; self.oi[:] = 0
        self.hd.zero(); self.hi.zero()

    def _same_images(self, where, ra, rb, direct):
        assert ra == rb, (where, "rays", ra, rb)
        gi = self.hi.get()
        assert bits_equal(self.oi, gi), (where, "indirect image", radiance_stats(self.oi, gi))
        if direct:
            gd = self.hd.get()
            assert bits_equal(self.od, gd), (where, "direct image", radiance_stats(self.od, gd))

    def path_trace(self, it, looper, depth):
        o, h = self.o, self.h
        ra = ob.path_trace(o.scene, o.cam, self.od, self.oi, it, looper, depth)
        rb = self.hip.path_trace(h.scene, h.cam, self.hd.ptr, self.hi.ptr, it, looper, depth)
        self._same_images(("pathTrace", it, looper, depth), ra, rb, True)
        return ra

    def pt_indirect(self, it, looper, depth):
        o, h = self.o, self.h
        ra = ob.pt_indirect(o.scene, o.cam, self.oi, it, looper, depth)
        rb = self.hip.path_trace_indirect(h.scene, h.cam, self.hi.ptr, it, looper, depth)
        self._same_images(("pathTraceIndirect", it, looper, depth), ra, rb, False)
        return ra

    def render(self, pos=None):
        o, h = self.o, self.h
        if pos is not None:
            o.set_camera_position(pos); h.set_camera_position(pos)
        o.gbuf.render(o.scene, o.cam); h.gbuf.render(h.scene, h.cam)

    def update(self):
        self.o.gbuf.update(self.o.cam); self.h.gbuf.update(self.h.cam)

    def indirect(self, it, looper, reuse, depth):
        """ReSTIRIndirect on the rendered G-buffer; returns the oracle's ray count."""
        o, h = self.o, self.h
        ra = o.restir.indirect(o.scene, o.cam, o.gbuf, self.oi, it, looper, reuse, depth)
        rb = h.restir.indirect(h.scene, h.cam, h.gbuf, self.hi.ptr, it, looper, reuse, depth)
        where = ("ReSTIRIndirect", it, looper, reuse, depth)
        self._same_images(where, ra, rb, False)
        _same_reservoirs(o.restir.ind_last, h.restir.download_indirect(1), where)
        return ra

    def gi_frame(self, it, looper, reuse, depth, pos=None):
        """One frame of ReSTIR-GI as runCuda drives it; returns the oracle's own reservoirs of the frame."""
        self.render(pos)
        self.indirect(it, looper, reuse, depth)
        self.update()
        return self.o.restir.ind_last


SIZES = [(97, 61), (33, 9), (41, 27), (31, 7), (8, 1), (1, 1)]
RAGGED = ([("cornell_glass", s, False) for s in SIZES] + [("cornell_glass", s, True) for s in SIZES[:2]] +
          [("cornell_textured", s, False) for s in SIZES[:2]] + [("sponza:0.03", SIZES[0], False)])


def _case_id(case):
    name, (w, h), sob = case
    return "%s-%dx%d%s" % (name, w, h, "-sobol" if sob else "")


@pytest.mark.parametrize("case", RAGGED, ids=_case_id)
def test_ragged_frames_bit_exact(hip, table, case):
    """A: frames that are no whole number of 32 x 8 blocks through all three kernels, after every call."""
    name, size, sob = case
    sd = _gi_scene(name)
    p = _Pair(hip, sd, size, table if sob else None)
    for frame, depth in enumerate((1, 3, 5)):                           # iter accumulates like Settings::accumulate
        p.path_trace(frame, frame, depth)
    if p.n >= 297:
        assert p.oi.max() > 0 and p.od.max() > 0
    p.clear()
    for frame, depth in enumerate((2, 4)):
        p.pt_indirect(frame, 7 + frame, depth)
    if p.n >= 297:
        assert p.oi.max() > 0
    p.clear()
    for frame in range(4):                                              # an orbiting camera: reprojection feeds findTemporalNeighbor
        r = p.gi_frame(0, frame, 1, 4, pos=orbit_position(sd.camera_args["position"], frame, radius=0.2))
    if p.n >= 297:
        assert r["numSamples"].max() > 2 and p.oi.max() > 0
    for depth in (1, 2):                                                # the shallow-depth exceptions of the last-bounce shortcut
        q = _Pair(hip, sd, size, table if sob else None, share=p)
        for frame in range(2):
            q.gi_frame(0, frame, 1, depth)


@pytest.mark.parametrize("sob", [False, True], ids=["default", "sobol"])
@pytest.mark.parametrize("size", [(33, 9), (97, 61)], ids=["33x9", "97x61"])
def test_nothing_outside_the_images_is_written(hip, table, size, sob):
    """B: bands of 8 * (W + 32) pixels before and behind every image keep their bits through all three entry points (checked by
    _DevImage.get after every call), and the frames between them equal the oracle's."""
    sd = _gi_scene("cornell_glass")
    band = _band(size[0])
    p = _Pair(hip, sd, size, table if sob else None, band=band)
    assert p.hd.band == p.hi.band == band and p.hi.ptr == p.hi.t.data_ptr() + band * 12
    assert (p.hi.bits()[:band * 3] == BAND_BITS).all() and (p.hi.bits()[(band + p.n) * 3:] == BAND_BITS).all() and len(p.hi.bits()) == (2 * band + p.n) * 3
    for frame, depth in enumerate((1, 4)):
        p.path_trace(frame, frame, depth)
    assert p.oi.max() > 0 and p.od.max() > 0
    for frame, depth in enumerate((2, 4)):
        p.pt_indirect(frame, 7 + frame, depth)
    p.clear()
    for frame in range(3):
        p.gi_frame(0, frame, 1, 4, pos=orbit_position(sd.camera_args["position"], frame, radius=0.2))
    assert p.oi.max() > 0


CLAMPED = [("cornell", (97, 61), False), ("sponza:0.03", (97, 61), False), ("cornell", (41, 27), False), ("sponza:0.03", (41, 27), False),
           ("cornell", (97, 61), True), ("sponza:0.03", (97, 61), True)]


@pytest.mark.parametrize("case", CLAMPED, ids=_case_id)
def test_reservoirs_past_the_clamp(hip, table, case):
    """C: M grows by one per frame of temporal reuse; the 21st frame (index 20) is the first whose merged M, 21, exceeds the clamp."""
    name, size, sob = case
    sd = get_scene(name)
    p = _Pair(hip, sd, size, table if sob else None)
    for frame in range(26):
        r = p.gi_frame(0, frame, 1, 2)
        m = r["numSamples"]
        if frame <= 19:
            assert m.max() == frame + 1, (frame, m.max())               # frame 19: 20 without the clamp having acted
        else:
            assert m.max() == 20, (frame, m.max())
            assert np.count_nonzero(m == 20) >= 0.5 * p.n, (frame, np.count_nonzero(m == 20), p.n)
    assert (r["weight"] > 0).any() and p.oi.max() > 0
    # clamped reservoirs reprojected through `motion`: an orbit of radius 0.2 taken ten steps at a time, so that every frame moves
    # most pixels to another index and, at 97 x 61, leaves borders without a temporal neighbour (lastIdx < 0)
    borders = 0
    for k in range(4):
        r = p.gi_frame(0, 26 + k, 1, 2, pos=orbit_position(sd.camera_args["position"], 10 * k, radius=0.2))
        motion = p.o.gbuf.motion
        assert (motion != np.arange(p.n)).any() and (motion >= 0).any(), k
        borders += np.count_nonzero(motion < 0)
        assert r["numSamples"].max() == 20, k
    assert borders > 0 or size != (97, 61), borders


def _one_point_scene():
    """A scene whose vertices all coincide: no extent for the shadow tree's grid, every ray misses."""
    from restir_amd.scenes import LAMBERTIAN, LIGHT, SceneData, TriangleSoup, make_materials
    soup = TriangleSoup()
    p = np.array([0.25, 0.5, -2.0], np.float32)
    for k in range(4):
        soup.add(np.array([[p, p, p]]), np.array([[[0, 0, 1]] * 3], np.float32), 0 if k < 3 else 1)
    return SceneData("one_point", soup, make_materials([dict(type=LAMBERTIAN, baseColor=(0.7, 0.7, 0.7)), dict(type=LIGHT, baseColor=(5.0, 5.0, 5.0))]),
                     dict(position=(0.0, 0.5, 1.0), rotation=(-90.0, 0.0, 0.0), fov_y=30.0, focal_dist=1.0))


@pytest.mark.parametrize("kind", ["no_lights", "dielectric_disney", "one_triangle", "two_triangles_light_only", "one_point"])
def test_degenerate_scenes_through_the_multi_bounce_kernels(hip, kind):
    """D: numLights == 0 still draws the four light variates; a frame that sees only void or light leaves path_loop on its first
    test of __any(alive); a BVH whose root is a leaf; BSDFs that evaluate to zero."""
    sd = _one_point_scene() if kind == "one_point" else _edge_scene(kind)
    p = _Pair(hip, sd, (41, 27))
    assert p.n == 1107
    rays = p.path_trace(0, 0, 4)
    if kind == "no_lights":
        assert rays == 3540 and p.oi.max() == 0 and p.oi.min() == 0
    elif kind == "one_triangle":
        assert rays == 1164
    elif kind in ("two_triangles_light_only", "one_point"):
        assert rays == 1107
    p.clear()
    rays = p.pt_indirect(0, 0, 4)
    if kind == "no_lights":
        assert p.oi.max() == 0 and p.oi.min() == 0
    elif kind == "dielectric_disney":
        assert p.oi.max() > 0
    elif kind in ("two_triangles_light_only", "one_point"):
        assert rays == 1107
    p.clear()
    for frame in range(3):
        p.render()
        rays = p.indirect(0, frame, 1, 4)
        p.update()
        if kind in ("two_triangles_light_only", "one_point"):
            assert rays == 1107, frame
        elif kind == "no_lights":
            assert p.oi.max() == 0 and p.oi.min() == 0


def test_trace_depth_zero(hip):
    """E: maxDepth 0 ends every path at the primary hit: one ray per pixel, pathTrace's direct image holds HDRToLDR(1) where the
    camera sees the light or the void and nothing else."""
    p = _Pair(hip, _gi_scene("cornell_glass"), (33, 9))
    assert p.path_trace(0, 0, 0) == 297
    assert p.od.max() == 0.5 and p.oi.max() == 0 and p.oi.min() == 0
    assert p.pt_indirect(0, 1, 0) == 297
    for frame in range(2):
        p.render()
        assert p.indirect(0, frame, 1, 0) == 297
        p.update()


def test_restir_indirect_without_reuse(hip):
    """E: reuse 0 never merges: M stays 1."""
    p = _Pair(hip, _gi_scene("cornell_glass"), (33, 9))
    for frame in range(3):
        r = p.gi_frame(0, frame, 0, 4)
        assert r["numSamples"].min() == 1 and r["numSamples"].max() == 1, frame
    assert p.oi.max() > 0


def test_reset_between_indirect_frames(hip):
    """E: rs_restir_reset re-arms the first-frame flag: the frame after it does not merge."""
    p = _Pair(hip, _gi_scene("cornell_glass"), (33, 9))
    for frame in range(3):
        r = p.gi_frame(0, frame, 1, 4)
    assert r["numSamples"].max() == 3
    p.o.restir.reset(); p.h.restir.reset()
    r = p.gi_frame(0, 3, 1, 4)
    assert r["numSamples"].max() == 1
    r = p.gi_frame(0, 4, 1, 4)
    assert r["numSamples"].max() == 2


def test_first_frame_flag_shared_by_direct_and_indirect(hip):
    """E: one rs_restir and the oracle's one ReSTIR object, each frame ReSTIRDirect and then ReSTIRIndirect: the direct pass lowers the
    flag, so the indirect pass of frame 0 already looks for its temporal neighbour (restir.cu:441-446,465-467)."""
    p = _Pair(hip, _gi_scene("cornell_glass"), (33, 9))
    o, h = p.o, p.h
    for frame in range(3):
        p.render()
        assert o.restir.first == (frame == 0)
        ra = o.restir.direct(o.scene, o.cam, o.gbuf, p.od, 0, frame, 3)
        h.restir.direct(h.scene, h.cam, h.gbuf, p.hd.ptr, 0, frame, 3)
        assert ra == h.restir.ray_count(), frame
        gd = p.hd.get()
        assert bits_equal(p.od, gd), (frame, radiance_stats(p.od, gd))
        _compare_reservoirs(o.restir.last, h.restir.download(1))
        assert not o.restir.first
        p.indirect(0, frame, 1, 4)
        p.update()
    assert p.od.max() > 0 and p.oi.max() > 0 and o.restir.ind_last["numSamples"].max() == 3


def test_sobol_depth_beyond_the_guard_is_refused(hip, table):
    """E: a path draws at most 6 + 7 * maxDepth numbers and the device table ends in a guard of 4096 zeros behind its 200 columns:
    6 + 7 * 613 = 4297 > 4296 is refused as an invalid argument with no image touched, 6 + 7 * 612 = 4290 runs.  (Depth 612 is not
    compared: a closed box keeps paths alive that long, and the oracle's table has no such guard.)"""
    p = _Pair(hip, _gi_scene("cornell_glass"), (33, 9), table)
    o, h = p.o, p.h
    p.hd.t[:] = BAND_BITS; p.hi.t[:] = BAND_BITS
    p.render()
    calls = [lambda d: hip.path_trace(h.scene, h.cam, p.hd.ptr, p.hi.ptr, 0, 0, d),
             lambda d: hip.path_trace_indirect(h.scene, h.cam, p.hi.ptr, 0, 0, d),
             lambda d: h.restir.indirect(h.scene, h.cam, h.gbuf, p.hi.ptr, 0, 0, 1, d)]
    for call in calls:
        with pytest.raises(hip.RestirHipError, match="error 10001: .*trace depth too large for the Sobol table's guard"):
            call(613)
        assert (p.hd.bits() == BAND_BITS).all() and (p.hi.bits() == BAND_BITS).all()
    p.hd.zero(); p.hi.zero()                   # (iter 0 still reads the image: image * 0 + sample would keep the NaN of BAND_BITS)
    for call in calls:
        assert call(612) >= 297
        assert np.isfinite(p.hi.get()).all()
    assert np.isfinite(p.hd.get()).all() and p.hd.get().max() >= 0.5       # HDRToLDR(1) where the camera sees the light, at any depth


def test_restir_indirect_refuses_other_sizes(hip):
    """E: a camera or a G-buffer whose size is not the rs_restir's: an invalid argument, no image touched."""
    p = _Pair(hip, _gi_scene("cornell_glass"), (33, 9))
    h = p.h
    p.hi.t[:] = BAND_BITS
    p.render()
    other = HipRenderer(hip, p.sd, 32, 9, scene=h.scene)
    other.gbuf.render(other.scene, other.cam)
    for cam, gbuf in ((other.cam, h.gbuf), (h.cam, other.gbuf), (other.cam, other.gbuf)):
        with pytest.raises(hip.RestirHipError, match="error 10001: .*size mismatch"):
            h.restir.indirect(h.scene, cam, gbuf, p.hi.ptr, 0, 0, 1, 4)
        assert (p.hi.bits() == BAND_BITS).all()
    p.hi.zero()
    p.indirect(0, 0, 1, 4)                                              # and the refused calls left the rs_restir as it was


def _sixty_calls(hip, size):
    """pathTrace, pathTraceIndirect and ReSTIRIndirect, 20 accumulating iterations each at depth 4, under the current context: every
    call's ray count and the four final images."""
    sd = _gi_scene("cornell_glass")
    h = HipRenderer(hip, sd, *size)
    n = size[0] * size[1]
    direct, indirect, pti, gi = (_DevImage(n) for _ in range(4))
    rays = []
    for it in range(20):
        rays.append(hip.path_trace(h.scene, h.cam, direct.ptr, indirect.ptr, it, it, 4))
    for it in range(20):
        rays.append(hip.path_trace_indirect(h.scene, h.cam, pti.ptr, it, it, 4))
    for it in range(20):
        h.gbuf.render(h.scene, h.cam)
        rays.append(h.restir.indirect(h.scene, h.cam, h.gbuf, gi.ptr, it, it, 1, 4))
        h.gbuf.update(h.cam)
    hip.synchronize()
    return rays, [img.get().copy() for img in (direct, indirect, pti, gi)]


def test_ray_counts_belong_to_the_context(hip):
    """F: two host threads, each with its own context, its own stream, asynchronous launches and its own frame size (97 x 61 and
    41 x 27), run the three entry points at the same time.  Every call's ray count and every final image equal, count for count and
    bit for bit, those of the same sixty calls made single-threaded on the default context beforehand.  The counters are a buffer
    of the context (rs_context::walkCount), zeroed and read in the order of its stream; one buffer shared by the process would let
    one thread's clearing fall into the other's kernel and both add into the same words.
    (Two contexts on two devices -- each buffer allocated under its context's device by the entry point's scope -- cannot run on a
    single GPU: that case is verified by reading)"""
    import threading
    import torch
    sizes = {"one": (97, 61), "two": (41, 27)}
    ref = {name: _sixty_calls(hip, size) for name, size in sizes.items()}
    # non-vacuity: every call walked, and the two frame sizes do not count the same
    assert all(r > 0 for name in sizes for r in ref[name][0])
    assert all(a != b for a, b in zip(ref["one"][0], ref["two"][0]))
    assert all(img.max() > 0 for name in sizes for img in ref[name][1])
    results, errors = {}, []

    def worker(name):
        try:
            torch.cuda.set_device(0)
            ctx = hip.Context(0)
            ctx.make_current()
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                hip.set_stream(stream.cuda_stream)
                hip.set_sync(False)
                results[name] = _sixty_calls(hip, sizes[name])
                stream.synchronize()
            hip.Context.use_default()
            ctx.destroy()
        except Exception as e:                          # pragma: no cover
            errors.append((name, repr(e)))

    threads = [threading.Thread(target=worker, args=(name,)) for name in sizes]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for name in sizes:
        assert results[name][0] == ref[name][0], (name, "rays", results[name][0], ref[name][0])
        for k, (a, b) in enumerate(zip(ref[name][1], results[name][1])):
            assert bits_equal(a, b), (name, "image", k, radiance_stats(a, b))
