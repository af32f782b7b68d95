"""ReSTIR-GI's spatial pass (rs_restir_set_indirect_spatial) on the GPU.  Against the CPU oracle composed with the NumPy restatement of
tests/indirect_spatial.py, bit for bit after every frame: the image, the ray count, T (the buffer the call wrote), the history it merged
from, S and the eight counters -- over the cases of gs.CASES (37x23 and 64x48, radii 5 and 30, 1 / 5 / 16 taps, both samplers, still and
orbiting camera, depth 1 to 3, reuse 2 and 3, iter 0 and a running mean; a plain scene, a textured one with an environment map, one with a
Dielectric box and the lamp in view).  The receiver's surface the kernel used is held to the restated one and, on a first frame, to T's own
xv / nv.  GPU against GPU: calls that must not run the pass, radius 0.25, frames in flight.  tests/test_indirect_spatial_host.py shows
without a GPU that the cases are not vacuous."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import binding as ob
from restir_amd import sobol
from restir_amd.ctypes_structs import DIELECTRIC, INDIRECT_RESERVOIR_DTYPE
from tests import indirect_spatial as gs
from tests import shadow_revalidate as sv
from tests.common import bits_equal
from tests.scene_edits import assert_same

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(autouse=True)
def exact_libm(hip):
    ob.set_libm_mode(1)              # cos / sin correctly rounded on both sides: every bit must agree
    hip.set_sync(True)
    yield
    ob.set_libm_mode(0)
    hip.set_sync(True)


def check_frame(pair, tag, reuse, launched, reval_launched=False):
    got, ref, reval_lib, reval_restated = pair.frame(reuse)
    print(tag, "library", got["spatial"], "restated", ref["spatial"], "rays", got["rays"])
    assert_same(ref, got, tag)
    assert got["spatial"][0] == launched, tag
    if not launched:
        assert got["spatial"][1] == (0,) * 8, tag
    assert reval_lib == reval_restated and reval_lib[0] == reval_launched, (tag, reval_lib, reval_restated)
    return got


def check_primary(pair, tag, first):
    """rs_debug_restir_indirect_primary against the restated receiver; on a first frame T's own xv / nv wherever the weight is > 0 (the
    sample there is the path's own: restir.cu:316-321)."""
    xv, nv, wo, mat = pair.h.restir.indirect_primary()
    r = pair.o.recv
    assert np.array_equal(mat, r["mat_id"]), tag
    for k, a in (("xv", xv), ("nv", nv), ("wo", wo)):
        assert bits_equal(a, r[k]), (tag, k)
    if first:
        T = pair.h.restir.download_indirect(1)
        own = T["weight"] > 0
        assert (r["kind"][own & (mat < 0)] == DIELECTRIC).all(), tag      # a weight without taking part: only behind glass, whose plane is empty
        own &= mat >= 0
        assert own.sum() >= 64, tag
        assert bits_equal(T["xv"][own], xv[own]) and bits_equal(T["nv"][own], nv[own]), tag


# ---- (a) parity with the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gs.CASES, ids=gs.case_id)
def test_parity(hip, case):
    name, size, taps, radius, sampler, orbit, depth, reuse, accumulate = case
    pair = gs.Pair(hip, name, size, spatial=(taps, radius), sobol=sobol.sobol_table() if sampler == "sobol" else None, depth=depth, accumulate=accumulate)
    pair.h.restir.record_indirect_primary()
    base = np.array([pair.o.cam.position[i] for i in range(3)], F)
    total = np.zeros(8, np.int64)
    for f in range(gs.FRAMES):
        if orbit:
            pair.set_camera_position(gs.orbit_position(base, f))
        got = check_frame(pair, (gs.case_id(case), f), reuse, True)
        check_primary(pair, (gs.case_id(case), f), f == 0)
        total += np.array(got["spatial"][1])
    assert total[0] > 0 and total[1] > 0 and total[2] > 0        # (everything else: the host test, on these very cases)


# ---- (b) calls that must not run the pass --------------------------------------------------------------------------------------------------
def test_without_the_pass_the_call_is_todays(hip):
    """Switch on and reuse & 2 clear; switch off and reuse 3: every frame equals the frame of an object that never heard of the switch."""
    sd = gs.scene_of("cornell")
    W, H = gs.SMALL
    plain, on, off = (gs.HipGI(hip, sd, W, H, depth=3) for _ in range(3))
    assert on.restir.get_indirect_spatial() == (False, 5, 5.0)
    on.restir.set_indirect_spatial(True, 16, 30.0)
    off.restir.set_indirect_spatial(True); off.restir.set_indirect_spatial(False)
    for f in range(4):
        plain.frame(1); on.frame(1); off.frame(1)
        a = plain.state()
        for tag, r in (("bit 2 clear", on), ("switch off, reuse 1", off)):
            b = r.state()
            assert not b["spatial"][0] and b["spatial"][1] == (0,) * 8
            assert_same(dict(a, S=None, spatial=None), dict(b, S=None, spatial=None), (tag, f))
    for f in range(4):                                                   # (the same two objects go on: their buffers hold the same history)
        plain.frame(3); off.frame(3)
        a, b = plain.state(), off.state()
        assert not b["spatial"][0] and b["spatial"][1] == (0,) * 8
        assert_same(dict(a, S=None, spatial=None), dict(b, S=None, spatial=None), ("switch off", f))


def test_radius_quarter_equals_the_switch_off(hip):
    """Radius 0.25: every tap lands on the pixel itself.  The pass runs, S = T, and image, T, history and rays are the switch-off ones."""
    sd = gs.scene_of("env")
    W, H = gs.SMALL
    table = sobol.sobol_table()
    a, b = (gs.HipGI(hip, sd, W, H, sobol=table, depth=3, accumulate=True) for _ in range(2))
    b.restir.set_indirect_spatial(True, 5, 0.25)
    for f in range(4):
        a.frame(3); b.frame(3)
        sa, sb = a.state(), b.state()
        assert sb["spatial"][0]
        part, accepted, failed = sb["spatial"][1][:3]
        assert part > 0 and accepted == 0 and failed == 5 * part and sb["spatial"][1][3:] == (0,) * 5
        assert_same(dict(sa, S=None, spatial=None), dict(sb, S=None, spatial=None), f)
        assert_same(dict(S=sb["written"]), dict(S=sb["S"]), f)


# ---- (c) frames in flight ------------------------------------------------------------------------------------------------------------------
def in_flight_run(hip, in_flight):
    import torch
    sd = gs.scene_of("glass")
    W, H = gs.SMALL
    r = gs.HipGI(hip, sd, W, H, depth=3)
    r.restir.set_indirect_spatial(True, 5, 5.0)
    images = [torch.zeros((W * H, 3), dtype=torch.float32, device="cuda") for _ in range(6)]
    hip.set_sync(not in_flight)
    for f in range(6):
        r.gbuf.render(r.scene, r.cam)
        r.image.zero_()
        hip.check(hip.lib().rs_restir_indirect(r.restir.handle, r.scene.handle, C.byref(r.cam), r.gbuf.handle, r.image.data_ptr(), 0, r.looper, 3, r.depth, None))
        r.looper += 1
        r.gbuf.update(r.cam)
        assert r.restir.indirect_spatial_launched()                      # (host only: no wait)
        hip.hip_memcpy_d2d_async(images[f].data_ptr(), r.image.data_ptr(), W * H * 12)
        if in_flight and (f + 1) % 3 == 0:
            hip.synchronize()
    hip.synchronize()
    hip.set_sync(True)
    return [i.cpu().numpy() for i in images], dict(written=r.restir.download_indirect(1), history=r.restir.download_indirect(0), S=r.restir.download_indirect_spatial(),
                                                   stats=np.array(r.restir.indirect_spatial_stats()))


def test_three_frames_in_flight_equal_synchronous(hip):
    ref, last = in_flight_run(hip, False)
    images, last3 = in_flight_run(hip, True)
    for f, (a, b) in enumerate(zip(ref, images)):
        assert_same(dict(image=a), dict(image=b), f)
    assert_same(last, last3, "final")
    assert last["stats"][6] > 0


# ---- (d) beside indirect revalidation, a change of scene, the switch between frames ----------------------------------------------------------
def test_after_a_geometry_edit_both_passes_agree_with_their_restatements(hip):
    pair = gs.Pair(hip, "cornell", gs.LARGE, spatial=(5, 5.0), reval=True)
    for f in range(6):
        check_frame(pair, ("warm", f), 3, True)
    for back in (False, True):
        ids, v = sv.moved_box(pair.sd, pair.o.scene.vertices, -sv.DISPLACEMENT if back else sv.DISPLACEMENT)
        pair.edit(ids, v)
        got = check_frame(pair, ("moved", back), 3, True, reval_launched=True)
        assert got["spatial"][1][7] >= 1                                 # winners blocked on the edited geometry
        check_frame(pair, ("after", back), 3, True)


def test_a_change_of_scene(hip):
    pair = gs.Pair(hip, "cornell", gs.SMALL, spatial=(5, 5.0), sobol=sobol.sobol_table(), depth=3)
    for f in range(3):
        check_frame(pair, ("cornell", f), 3, True)
    pair.new_scene("env")                                                # textured kernels, an environment map, another camera
    for f in range(3):
        check_frame(pair, ("env", f), 3, True)


def test_switches(hip):
    pair = gs.Pair(hip, "glass", gs.SMALL, spatial=(5, 5.0), depth=3)
    r = pair.h.restir
    assert r.get_indirect_spatial() == (True, 5, 5.0)
    check_frame(pair, "on", 3, True)
    pair.set_spatial(None)
    assert r.get_indirect_spatial()[0] is False
    check_frame(pair, "off", 3, False)
    pair.set_spatial((16, 30.0))
    assert r.get_indirect_spatial() == (True, 16, 30.0)
    check_frame(pair, "on again, other settings", 3, True)
    check_frame(pair, "reuse 1", 1, False)
    r.set_indirect_revalidation(True); r.set_shadow_revalidation(True)   # independent of the other switches
    assert r.get_indirect_spatial() == (True, 16, 30.0)
    check_frame(pair, "beside the others", 2, True)
    r.set_indirect_spatial(True)                                         # taps, radius <= 0: the defaults
    assert r.get_indirect_spatial() == (True, 5, 5.0)
    r.set_indirect_spatial(True, -1, -2.0)
    assert r.get_indirect_spatial() == (True, 5, 5.0)
    lib = hip.lib()
    for bad in ((17, 5.0), (5, 64.5), (5, float("nan")), (5, float("inf"))):
        assert lib.rs_restir_set_indirect_spatial(r.handle, 1, bad[0], bad[1]) == hip.RS_ERR_INVALID_ARGUMENT
        assert r.get_indirect_spatial() == (True, 5, 5.0)                # a refusal changes nothing
    fresh = hip.ReSTIR(*gs.SMALL)
    assert lib.rs_restir_download_indirect_spatial(fresh.handle, np.zeros(gs.SMALL[0] * gs.SMALL[1], INDIRECT_RESERVOIR_DTYPE).ctypes.data_as(C.c_void_p)) == hip.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_debug_restir_indirect_primary(fresh.handle, np.zeros(4, F).ctypes.data_as(C.c_void_p), None, None, None) == hip.RS_ERR_INVALID_ARGUMENT


def test_seeded_uniforms_with_the_scenes_table(hip):
    """The Sobol form of rs_debug_seeded_uniforms against the recorded streams of tests/golden/sobol_oracle.npz."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "sobol_oracle.npz"))
    h = gs.HipGI(hip, gs.scene_of("cornell"), *gs.SMALL, sobol=sobol.sobol_table())
    n, m = g["stream_out"].shape
    got = np.stack([hip.seeded_uniforms(h.scene, g["stream_looper"][k], g["stream_index"][k], g["stream_dim"][k], m) for k in range(n)])
    assert bits_equal(got, g["stream_out"])
    h.scene.set_sample_sequence(None)                                    # without a table: the default engine
    assert bits_equal(hip.seeded_uniforms(h.scene, 3, 5, 150, 8), hip.seeded_uniforms(None, 3, 5, 150, 8))


def test_the_setter_refuses_while_the_stream_is_captured(hip):
    """As tests/test_gpu_deformer_refusal_texts.py captures the library stream: the setter answers RS_ERR_UNSUPPORTED and changes nothing."""
    import torch
    r = hip.ReSTIR(*gs.SMALL)
    lib = hip.lib()
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
            assert lib.rs_restir_set_indirect_spatial(r.handle, 1, 5, 5.0) == hip.RS_ERR_UNSUPPORTED
            assert "captured" in lib.rs_last_error().decode()
            assert r.get_indirect_spatial() == (False, 5, 5.0)
        finally:
            assert rt.hipStreamEndCapture(stream.cuda_stream, C.byref(graph)) == 0
            if graph:
                rt.hipGraphDestroy(graph)
    finally:
        hip.set_stream(None)
    r.set_indirect_spatial(True)
    assert r.get_indirect_spatial() == (True, 5, 5.0)
