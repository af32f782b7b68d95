"""Emission edits (rs_scene_set_emission) and temporal light tracking (rs_restir_set_light_tracking) against the CPU oracle, bit for bit
and frame by frame: the radiance, the reservoirs of the frame (download 1), the published copy (download 2), the light indices of all
three and the ray count.  Every tracked RIS form (global table, table in LDS, alias table in LDS, environment map) with both samplers
and every reuse mode, tracking on and off, under random non-uniform edits; the state changes that forget light indices; row bands;
frames in flight with edits between and inside frames and bursts that wrap the ring of emission versions."""
import functools

import numpy as np
import pytest

from oracle import binding as ob
from restir_amd import scenes, sobol
from tests.common import RIS_TABLE_PIXELS_DEFAULT, EmissionEdits, HipRenderer, OracleRenderer, bits_equal, get_scene, next_looper

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def exact_libm(hip):
    ob.set_libm_mode(1)            # cos / sin correctly rounded on both sides: every bit must agree
    hip.set_sync(True)
    yield
    ob.set_libm_mode(0)
    hip.set_sync(True)
    hip.set_ris_table_pixels(RIS_TABLE_PIXELS_DEFAULT)


@functools.lru_cache(maxsize=None)
def scene_data(name):
    return get_scene(name)


@functools.lru_cache(maxsize=None)
def sobol_table():
    return sobol.sobol_table()


def compare(o, h, reuse, tag):
    """Everything the frame left: radiance, ray count, the three reservoir buffers' light indices, the frame's reservoirs and,
    with spatial reuse, the published copy."""
    a, b = o.image, h.image.cpu().numpy()
    assert bits_equal(a, b), (tag, "radiance", int((a.view(np.uint32) != b.view(np.uint32)).any(axis=1).sum()))
    for which in (0, 1, 2):
        x, y = o.light_ids(which), h.light_ids(which)
        assert np.array_equal(x, y), (tag, "light ids", which, int((x != y).sum()))
    resv = [(o.restir.last, h.restir.download(1), 1)]
    if reuse & 2:
        resv.append((o.restir.temp, h.restir.download(2), 2))
    for x, y, which in resv:
        assert np.array_equal(x["numSamples"], y["numSamples"]), (tag, which, "numSamples")
        for k in ("Li", "wi", "dist", "weight"):
            assert bits_equal(x[k], y[k]), (tag, which, k, int((x[k].view(np.uint32) != y[k].view(np.uint32)).reshape(len(x), -1).any(axis=1).sum()))


class Pair:
    """The oracle and the library driven through the same calls: runCuda's frame with an orbiting camera."""

    def __init__(self, hip, sd, W, H, sobol=None, track=True):
        self.o = OracleRenderer(sd, W, H, sobol=sobol, track=track)
        self.h = HipRenderer(hip, sd, W, H, sobol=sobol, track=track)
        self.base = sd.camera_args["position"]
        self.f = 0

    def move(self):
        p = scenes.orbit_position(self.base, self.f, radius=1.0)
        self.o.set_camera_position(p)
        self.h.set_camera_position(p)
        self.f += 1

    def edit(self, ids, rad):
        self.o.set_emission(ids, rad)
        self.h.set_emission(ids, rad)

    def frame(self, reuse):
        self.move()
        self.o.frame(reuse)
        self.h.frame(reuse)
        assert self.o.rays == self.h.rays, (self.f, self.o.rays, self.h.rays)
        compare(self.o, self.h, reuse, self.f - 1)

    def set_light_tracking(self, on):
        self.o.restir.set_light_tracking(on)
        self.h.restir.set_light_tracking(on)


EDIT_FRAMES = (2, 3, 6)            # two consecutive frames and a later one


def run_edited(hip, sd, W, H, reuse, sobol=None, track=True, seed=0, frames=8):
    p = Pair(hip, sd, W, H, sobol=sobol, track=track)
    edits = EmissionEdits(sd, seed)
    for f in range(frames):
        if f in EDIT_FRAMES:
            p.edit(*edits.next())
        p.frame(reuse)
    return p


# ---- a. every tracked RIS form x sampler x reuse, tracking on and off ------------------------------------------------------------
# form: scene, size, rs_set_ris_table_pixels (None = the library's default), synchronous mode
FORMS = {
    "global": ("sponza:0.125", 160, 96, None),        # k_ris<false, *, true>: 15 360 pixels read the table from global memory
    "lds": ("sponza:0.125", 160, 96, 0),              # k_ris_lds<*, true>: 128 lights in LDS
    "alias_lds": ("bistro:0.12", 160, 96, 0),         # k_ris_alias_lds<*, true>: 1 228 lights, the alias records in LDS
    "env": ("cornell_textured", 128, 128, None),      # k_ris<true, *, true>: the environment map's entry (envId) is skipped
}


CASES = [(form, sampler, reuse) for form in FORMS for sampler in ("engine", "sobol")
         for reuse in ((0, 1, 2, 3) if form == "global" else (1, 2, 3))]        # reuse 0 (no merge) once


@pytest.mark.parametrize("track", [True, False], ids=["tracked", "untracked"])
@pytest.mark.parametrize("form,sampler,reuse", CASES)
def test_edits_every_ris_form(hip, form, sampler, reuse, track):
    name, W, H, pixels = FORMS[form]
    hip.set_ris_table_pixels(RIS_TABLE_PIXELS_DEFAULT if pixels is None else pixels)
    sd = scene_data(name)
    run_edited(hip, sd, W, H, reuse, sobol=sobol_table() if sampler == "sobol" else None, track=track,
               seed=CASES.index((form, sampler, reuse)))


# ---- b. state changes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["engine", "sobol"])
def test_tracking_switched_off_and_on_mid_run(hip, sampler):
    sd = scene_data("sponza:0.125")
    p = Pair(hip, sd, 160, 96, sobol=sobol_table() if sampler == "sobol" else None, track=True)
    edits = EmissionEdits(sd, 21)
    for f in range(10):
        if f == 3:
            p.set_light_tracking(False)
            assert all((p.h.light_ids(w) == -1).all() for w in range(3))
        if f == 6:
            p.set_light_tracking(True)             # every light unknown again, on both sides
            assert all((p.h.light_ids(w) == -1).all() for w in range(3))
        if f in (2, 4, 6, 7):
            p.edit(*edits.next())
        p.frame(3)
    assert (p.h.light_ids(1) >= 0).any()


def test_one_restir_two_scenes(hip):
    """An rs_restir that renders scene A, then scene B (the same geometry, other lamps): B's first frame must not take A's light indices
    for its own (rs_light_history::sceneId).  Then A again."""
    sd = scene_data("sponza:0.125")
    W, H = 160, 96
    p = Pair(hip, sd, W, H, track=True)
    a_o, a_h = p.o.scene, p.h.scene
    b_o, b_h = OracleRenderer(sd, W, H).scene, HipRenderer(hip, sd, W, H).scene
    ea, eb = EmissionEdits(sd, 31), EmissionEdits(sd, 32)
    for _ in range(3):
        ids, rad = eb.next()
        b_o.set_emission(ids, rad); b_h.set_emission(ids, rad)
    for f in range(9):
        if f in (3, 6):
            p.o.scene, p.h.scene = (b_o, b_h) if f == 3 else (a_o, a_h)
            last1, temp = p.h.light_ids(1), p.h.light_ids(2)
            assert (last1 >= 0).any() and (temp >= 0).any()
        if f == 4:
            ids, rad = eb.next()
            p.edit(ids, rad)
        if f == 7:
            p.edit(*ea.next())
        p.frame(3)


def test_upload_into_tracked_restir(hip):
    sd = scene_data("sponza:0.125")
    p = Pair(hip, sd, 160, 96, track=True)
    edits = EmissionEdits(sd, 41)
    for f in range(3):
        p.frame(3)
    # the reservoirs go out and come back: the uploaded samples' lights are unknown
    for which in (2, 1, 0):
        arr = p.h.restir.download(which)
        p.h.restir.upload(which, arr)
        p.o.restir.upload(which, arr)
        assert (p.h.light_ids(which) == -1).all()
        compare(p.o, p.h, 3, ("upload", which))
    for f in range(5):
        if f in (0, 1, 3):
            p.edit(*edits.next())
        p.frame(3)


# ---- c. row bands ----------------------------------------------------------------------------------------------------------------
def test_row_bands_with_edits(hip):
    """rs_restir_phase_a over three unequal row bands, then phase_b over the same bands, edits between frames and between the bands'
    phases -- against the oracle's banded phases."""
    sd = scene_data("sponza:0.125")
    W, H = 160, 96
    bands = [(0, 17), (17, 60), (60, H)]
    p = Pair(hip, sd, W, H, track=True)
    o, h = p.o, p.h
    edits = EmissionEdits(sd, 51)
    for f in range(7):
        if f in (2, 3, 5):
            p.edit(*edits.next())
        p.move()
        o.gbuf.render(o.scene, o.cam)
        h.gbuf.render(h.scene, h.cam)
        for i, (y0, y1) in enumerate(bands):
            if f == 4 and i == 1:
                p.edit(*edits.next())              # the second band's RIS and merge see the new emission
            o.restir.phase_a(o.scene, o.cam, o.gbuf, o.looper, 3, y0, y1)
            h.restir.phase_a(h.scene, h.cam, h.gbuf, h.looper, 3, y0, y1)
        for y0, y1 in bands:
            o.restir.phase_b(o.scene, o.cam, o.gbuf, o.image, 0, 3, y0, y1)
            h.restir.phase_b(h.scene, h.cam, h.gbuf, h.image.data_ptr(), 0, 3, y0, y1)
        o.restir.end_frame(); h.restir.end_frame()
        o.looper = next_looper(o.looper, None); h.looper = next_looper(h.looper, None)
        o.gbuf.update(o.cam); h.gbuf.update(h.cam)
        compare(o, h, 3, f)


# ---- d. frames in flight ---------------------------------------------------------------------------------------------------------
# per frame: edits before its G-buffer render, edits between its render and its ReSTIRDirect
IN_FLIGHT_EDITS = {2: (1, 0), 3: (0, 1), 5: (1, 1), 8: (11, 0), 9: (0, 1), 12: (0, 10), 13: (1, 0), 17: (12, 0), 18: (0, 0), 20: (0, 1)}


@pytest.mark.parametrize("plan", ["default", "one_chain"])
@pytest.mark.parametrize("track", [True, False], ids=["tracked", "untracked"])
def test_edits_with_frames_in_flight(hip, plan, track):
    """Overlapped mode, one output buffer per frame, no host wait until the end.  An edit applies to every launch enqueued after it: a
    G-buffer render recorded before it keeps the old emission even though it is launched later.  Bursts of 10 to 12 edits wrap the
    ring of eight emission versions (set_emission then waits on the host).  The oracle makes the same calls in the same order."""
    import torch
    sd = scene_data("sponza:0.125")
    W, H, N = 160, 96, 24
    p = Pair(hip, sd, W, H, track=track)
    o, h = p.o, p.h
    edits = EmissionEdits(sd, 61)
    ref = []
    if plan == "one_chain":
        hip.set_stream_plan(1, 0, 0)
    hip.set_sync(False)
    try:
        outs = [torch.zeros((W * H, 3), dtype=torch.float32, device="cuda") for _ in range(N)]
        for f in range(N):
            before, inside = IN_FLIGHT_EDITS.get(f, (0, 0))
            for _ in range(before):
                p.edit(*edits.next())
            p.move()
            o.gbuf.render(o.scene, o.cam)
            h.gbuf.render(h.scene, h.cam)
            for _ in range(inside):
                p.edit(*edits.next())
            o.restir.direct(o.scene, o.cam, o.gbuf, o.image, 0, o.looper, 3)
            h.restir.direct(h.scene, h.cam, h.gbuf, outs[f].data_ptr(), 0, h.looper, 3)
            o.looper += 1; h.looper += 1
            o.gbuf.update(o.cam); h.gbuf.update(h.cam)
            ref.append((o.image.copy(), o.restir.rays))
        hip.synchronize()
    finally:
        hip.set_sync(True)
        hip.set_stream_plan(2, 1, 2)                 # the library's defaults (include/restir_hip.h)
    for f in range(N):
        b = outs[f].cpu().numpy()
        assert bits_equal(ref[f][0], b), (f, int((ref[f][0].view(np.uint32) != b.view(np.uint32)).any(axis=1).sum()))
    h.image.copy_(outs[-1])
    compare(o, h, 3, "final")
