"""The default sampler's generator on its state minus one (restir_amd/csrc/rs_math.h Rng) and the two draws the RIS loop compares before
their division by 2^31 (rs_surface.h sample_light_with, restir.hip ris_pixel).  There is no tolerance anywhere: the forms are exact or wrong.

  * rs_debug_rng_step_host_mismatches (no GPU): the shared Rng on the host against the step as it was, written out -- next state, bits of
    the draw, the sampler entry the draw picks of 1, 3, 1 024, 1 500, 10 240 and 2^24 + 1 lights, `draw < prob` for prob = 0, the smallest
    subnormal, 2^-31, 0.5, the float below 1, 1, 2 and a NaN; next state and draw of RngOnX, the form k_path steps; 19 results per
    state -- over the first 2^24 states, the last 2^24 below m = 2^31 - 1, and 2^20 states around each of 44 488 and 44 489 (Schrage's
    quotient m div 48 271 and the state after it; both windows begin at state 1 and lie inside the first range: cases the issue names).
  * test_the_switch_selects_the_form_each_case_names (no GPU): the launch plan's rule gives each frame case the kernel form it names.
  * rs_debug_rng_step_mismatches (GPU): the same on the device over all 2^31 - 2 states.
  * frames (GPU): 96 x 40, three frames, spatiotemporal reuse, the default sampler, light tracking off and on, through k_ris_lds with 1 024
    lamps, k_ris_alias_lds and k_ris with 1 500 (switched as tests/test_gpu_ris_guard.py switches them, whose scenes, oracle frames and
    comparison these are), and two small tables through the LDS form and k_ris: one lamp, whose alias record has prob == 1, and three lamps
    of which one emits nothing -- its record has prob == 0 (test_the_small_tables_hold_both_ends_of_the_threshold asserts both).  Radiance,
    ray count, both reservoir buffers and the light indices equal the oracle's bit for bit after every frame."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import binding as ob
from restir_amd import capi, scenes
from restir_amd.ctypes_structs import LAMBERTIAN, LIGHT, make_materials
from tests.common import RIS_TABLE_PIXELS_DEFAULT, HipRenderer, OracleRenderer
from tests.test_gpu_ris_guard import FRAMES, H, W, oracle_frames, same, snapshot, view

M = 2 ** 31 - 1
PER_STATE = 19
REUSE = 3


def host_mismatches(first, count):
    out = (C.c_ulonglong * 2)()
    capi.check(capi.lib().rs_debug_rng_step_host_mismatches(first, count, C.byref(out)))
    return int(out[0]), int(out[1])


@pytest.mark.parametrize("first,count", [(1, 1 << 24), (M - (1 << 24), 1 << 24), (max(1, 44488 - (1 << 19)), 1 << 20), (max(1, 44489 - (1 << 19)), 1 << 20)],
                         ids=["first_2^24", "last_2^24", "around_44488", "around_44489"])
def test_host_step_and_folded_comparisons(first, count):
    assert first >= 1 and first + count - 1 <= M - 1
    bad, compared = host_mismatches(first, count)
    assert compared == count * PER_STATE
    assert bad == 0


def test_host_hook_refuses_states_outside_the_period():
    out = (C.c_ulonglong * 2)()
    for first, count in ((0, 1), (1, 0), (M, 1), (M - 1, 2), (2, M - 1)):
        assert capi.lib().rs_debug_rng_step_host_mismatches(first, count, C.byref(out)) == capi.RS_ERR_INVALID_ARGUMENT, (first, count)
    assert host_mismatches(M - 1, 1) == (0, PER_STATE)


@pytest.mark.gpu
def test_device_step_and_folded_comparisons_over_the_whole_period(hip):
    out = (C.c_ulonglong * 2)()
    hip.check(hip.lib().rs_debug_rng_step_mismatches(C.byref(out)))
    print("rng step: differing", int(out[0]), "of", int(out[1]))
    assert int(out[1]) == (M - 1) * PER_STATE
    assert int(out[0]) == 0


@functools.lru_cache(maxsize=None)
def dark_view():
    """The wall, the lintel and three lamps of tests/test_gpu_ris_guard.py's lambert_3 -- the middle lamp with a radiance of zero."""
    specs = [dict(type=LAMBERTIAN, baseColor=(0.7, 0.7, 0.7)), dict(type=LIGHT, baseColor=(10.0, 10.0, 10.0)),
             dict(type=LIGHT, baseColor=(0.0, 0.0, 0.0)), dict(type=LIGHT, baseColor=(4.0, 9.0, 2.0))]
    s = scenes.TriangleSoup()
    s.add_quad((-7.04, -2.0, -1.0), (7.04, -2.0, -1.0), (7.04, 4.08, -1.0), (-7.04, 4.08, -1.0), 0)
    s.add_quad((-7, 1.45, 1), (7, 1.45, 1), (7, 4, 1), (-7, 4, 1), 0)
    for k, lx in enumerate((-2.0, 0.0, 2.0)):
        s.add_flat([[(lx, 0.4, 0.5), (lx, 0.45, 0.5), (lx + 0.05, 0.4, 0.5)]], 1 + k)
    return scenes.SceneData("dark_3", s, make_materials(specs), dict(position=(0.0, 1.0, 3.5), rotation=(-90.0, 0.0, 0.0), fov_y=19.5, focal_dist=1.0))


@functools.lru_cache(maxsize=None)
def dark_oracle_frames(track):
    ob.set_libm_mode(1)                     # cos / sin / atan2 correctly rounded, as the library evaluates them
    try:
        o = OracleRenderer(dark_view(), W, H, track=track)
        buffers = {1: lambda: o.restir.last, 2: lambda: o.restir.temp}
        frames = []
        for _ in range(FRAMES):
            o.frame(REUSE)
            frames.append(snapshot(o, REUSE, lambda w: buffers[w](), o.light_ids))
        return frames
    finally:
        ob.set_libm_mode(0)


def alias_prob(sd):
    _, _, power = capi.build_light_table(sd.vertices, sd.material_ids, sd.materials)
    return capi.build_alias_table(power)[0]


def test_the_small_tables_hold_both_ends_of_the_threshold():
    assert alias_prob(view("lambert_1")).tolist() == [1.0]
    prob = alias_prob(dark_view())
    assert len(prob) == 3 and (prob == 0).sum() == 1, prob
    lit = dark_oracle_frames(False)[-1]["last"]["weight"] > 0
    assert lit.sum() >= W * H // 4, int(lit.sum())          # the two lamps that do emit light the wall


# (scene, launch form): rs_set_ris_table_pixels(0) = the LDS form the table fits, 1 << 30 = k_ris
CASES = [("lambert_1024", "lds"), ("lambert_1500", "alias_lds"), ("lambert_1500", "global"),
         ("lambert_1", "lds"), ("lambert_1", "global"), ("dark_3", "lds"), ("dark_3", "global")]


def test_the_switch_selects_the_form_each_case_names():
    """The launch plan's rule (rs_debug_phase_a_plan, no GPU) for a synchronous 96 x 40 frame: what rs_set_ris_table_pixels(0) and (1 << 30) select."""
    form = {"lds": capi.RIS_LDS, "alias_lds": capi.RIS_ALIAS_LDS, "global": capi.RIS_GLOBAL}
    lamps = {"lambert_1024": 1024, "lambert_1500": 1500, "lambert_1": 1, "dark_3": 3}
    for name, f in CASES:
        plan = capi.phase_a_plan(width=W, y0=0, y1=H, numLights=lamps[name], risGlobalBelow=(1 << 30) if f == "global" else 0)
        assert plan.risForm == form[f], (name, f, plan.risForm)


@pytest.mark.gpu
@pytest.mark.parametrize("track", [False, True], ids=["untracked", "tracked"])
@pytest.mark.parametrize("name,form", CASES, ids=["%s-%s" % c for c in CASES])
def test_frames_bit_for_bit(hip, name, form, track):
    sd = dark_view() if name == "dark_3" else view(name)
    want = dark_oracle_frames(track) if name == "dark_3" else oracle_frames(name, "engine", track, REUSE)[0]
    hip.set_sync(True)
    hip.set_ris_table_pixels(1 << 30 if form == "global" else 0)
    try:
        h = HipRenderer(hip, sd, W, H, track=track)
        for f in range(FRAMES):
            h.frame(REUSE)
            same(want[f], snapshot(h, REUSE, h.restir.download, h.light_ids), (name, form, track, f))
        h.scene.destroy()
    finally:
        hip.set_ris_table_pixels(RIS_TABLE_PIXELS_DEFAULT)
