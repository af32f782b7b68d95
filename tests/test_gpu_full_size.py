"""GPU parity tests at BASELINE.json's FULL sizes: librestir_hip against the CPU oracle on the complete Sponza-class
(262 144 triangles) and Bistro-class (2.83 M triangles, 10 240 lights) scenes at 1920x1080 and 3840x2160.

The small-scene tests of test_gpu_parity.py cannot see an error that depends on the scene's extent or on the depth of its
trees (the shadow tree's 16-bit grid and its margin, the near-zero-axis cull, the packet walk's overlap shortcut, the
nested-links check on a 524 287-node tree): here both sides see the full-size inputs and every plane is compared bit for bit,
with the oracle's libm switch on "correctly rounded" (the mode in which the product is exact).

Reference lines under test: src/scene.h:245-316 (intersect / testOcclusion), src/restir.cu:111-231 (ReSTIRDirectKernel),
src/gbuffer.cu:3-73, src/denoiser.cu:64-134,463-477.
"""
import numpy as np
import pytest

from oracle import binding as ob
from tests.common import HipRenderer, OracleRenderer, bits_equal, get_scene, hip_scene, oracle_scene, radiance_stats
from tests.ray_cases import _shadow_like_segments
from tests.test_gpu_parity import _compare_reservoirs, _random_rays

pytestmark = pytest.mark.gpu


@pytest.fixture
def exact_libm():
    ob.set_libm_mode(1)
    yield
    ob.set_libm_mode(0)


def _compare_gbuffer(o, h, what=""):
    g = h.gbuf.download()
    f = g["frame_idx"] ^ 1                                    # the planes rendered last (update() flipped the index)
    assert f == o.gbuf.frame_idx ^ 1
    assert np.array_equal(o.gbuf.prim_id[f], g["prim_id"][f]), what
    assert np.array_equal(o.gbuf.motion, g["motion"]), what
    assert bits_equal(o.gbuf.albedo, g["albedo"]), what
    assert bits_equal(o.gbuf.normal[f], g["normal"][f]), what
    assert bits_equal(o.gbuf.depth[f], g["depth"][f]), what


def _frames_equal_oracle(hip, sd, W, H, static_frames, orbit_frames, radius=1.0, before_last_update=None, sobol=None):
    """runCuda's sequence (render, ReSTIRDirect, [filter], update) on both sides, everything compared after every frame."""
    from restir_amd.scenes import orbit_position
    o = OracleRenderer(sd, W, H, sobol=sobol)
    h = HipRenderer(hip, sd, W, H, sobol=sobol)
    frames = static_frames + orbit_frames
    for frame in range(frames):
        if frame >= static_frames:                            # runCuda's animateCamera: reprojection through devMotion
            p = orbit_position(sd.camera_args["position"], frame - static_frames + 1, radius=radius)
            o.set_camera_position(p); h.set_camera_position(p)
        o.gbuf.render(o.scene, o.cam); h.gbuf.render(h.scene, h.cam)
        o.rays = o.restir.direct(o.scene, o.cam, o.gbuf, o.image, 0, frame, 3)
        h.restir.direct(h.scene, h.cam, h.gbuf, h.image.data_ptr(), 0, frame, 3)
        a, b = o.image, h.image.cpu().numpy()
        assert o.rays == h.restir.ray_count(), (frame, o.rays, h.restir.ray_count())
        assert bits_equal(a, b), (frame, radiance_stats(a, b))
        _compare_reservoirs(o.restir.last, h.restir.download(1))      # post-temporal reservoirs kept for the next frame
        _compare_reservoirs(o.restir.temp, h.restir.download(2))      # what the spatial pass gathered from
        if frame == frames - 1 and before_last_update is not None:
            before_last_update(o, h)
        o.gbuf.update(o.cam); h.gbuf.update(h.cam)
        _compare_gbuffer(o, h, frame)
    assert np.isfinite(a).all() and a.mean() > 1e-3
    return o, h


def test_config3_full_size_frames_equal_oracle(hip, exact_libm):
    """BASELINE config 3 at its size: Sponza-class 262 144 triangles / 1 024 lights, 1920x1080, spatiotemporal reuse, three
    frames of the static camera and two of the orbit -- radiance, both reservoir buffers and all G-buffer planes bit for bit."""
    sd = get_scene("sponza:1.0")
    assert sd.num_prims == 262144
    o, h = _frames_equal_oracle(hip, sd, 1920, 1080, 3, 2)
    assert o.restir.last["numSamples"].max() > 32                      # history in use


def test_config3_full_size_frames_with_the_sobol_sampler(hip, exact_libm):
    """The same workload with `SAMPLER_USE_SOBOL true` (src/sampler.h:9-36; north_star's "same scene and Sobol seed"): the build's
    10 000 x 200 table on both sides, two static frames and one of the orbit."""
    from restir_amd import sobol
    sd = get_scene("sponza:1.0")
    _frames_equal_oracle(hip, sd, 1920, 1080, 2, 1, sobol=sobol.sobol_table())


def test_config5_full_size_frames_equal_oracle(hip, exact_libm):
    """BASELINE config 5 at its size: Bistro-class 2.83 M triangles / 10 240 lights (the RIS kernel that reads the light table
    from global memory, a reference tree of depth > 30), 1920x1080, spatiotemporal reuse, two frames, then the five-level EAW
    filter of the second frame against the oracle's (expf: rtol 1e-5, as test_eaw_filter)."""
    import torch
    sd = get_scene("bistro:1.0")
    assert 2.7e6 < sd.num_prims < 2.9e6
    W, H = 1920, 1080

    def filtered(o, h):                                                # runCuda's order: render, ReSTIRDirect, filter, update
        ref = ob.eaw_filter(o.gbuf, o.cam, o.image)
        f = hip.EAWFilter(W, H, 5)
        out = torch.zeros_like(h.image)
        p = f.filter(out.data_ptr(), h.image.data_ptr(), h.gbuf, h.cam)
        hip.synchronize()
        res = torch.empty_like(h.image)
        hip.hip_memcpy_d2d(res.data_ptr(), p, res.numel() * 4)
        got = res.cpu().numpy()
        f.destroy()
        assert np.abs(ref - o.image).max() > 1e-3                      # the filter did something
        assert np.allclose(ref, got, rtol=1e-5, atol=1e-6), float(np.abs(ref - got).max())

    _frames_equal_oracle(hip, sd, W, H, 2, 0, before_last_update=filtered)


def _frames_within_tolerance_of_the_pinned_mode(hip, sd, W, H, static_frames, orbit_frames, record):
    """The same frames with the oracle in libm mode 0 -- glibc's cosf / sinf in the spatial taps' disk mapping (src/restir.cu:47-56,
    src/mathUtil.h:128-132), the mode the compiled reference and tests/golden/functions_ref.npz pin.  The device evaluates those two
    functions correctly rounded, so a tap can land one pixel beside the oracle's: stated tolerance (north_star) mean
    per-pixel L1 < 1e-4 and at most 1e-3 of the pixels beyond 1e-3, per frame; everything the taps do not feed is exact -- ray count,
    all G-buffer planes, the post-temporal reservoirs kept for the next frame (restir.cu:188,211-212: the spatial pass is not stored),
    the published reservoirs the taps gather from.  The differing-pixel counts are recorded in the test's properties."""
    from restir_amd.scenes import orbit_position
    ob.set_libm_mode(0)
    o = OracleRenderer(sd, W, H)
    h = HipRenderer(hip, sd, W, H)
    differing = []
    for frame in range(static_frames + orbit_frames):
        if frame >= static_frames:
            p = orbit_position(sd.camera_args["position"], frame - static_frames + 1, radius=1.0)
            o.set_camera_position(p); h.set_camera_position(p)
        o.gbuf.render(o.scene, o.cam); h.gbuf.render(h.scene, h.cam)
        o.rays = o.restir.direct(o.scene, o.cam, o.gbuf, o.image, 0, frame, 3)
        h.restir.direct(h.scene, h.cam, h.gbuf, h.image.data_ptr(), 0, frame, 3)
        a, b = o.image, h.image.cpu().numpy()
        st = radiance_stats(a, b)
        assert st["mean_l1"] < 1e-4 and st["flip_frac"] <= 1e-3, (frame, st)
        differing.append(int(np.count_nonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))))
        assert o.rays == h.restir.ray_count(), (frame, o.rays, h.restir.ray_count())
        _compare_reservoirs(o.restir.last, h.restir.download(1))
        _compare_reservoirs(o.restir.temp, h.restir.download(2))
        o.gbuf.update(o.cam); h.gbuf.update(h.cam)
        _compare_gbuffer(o, h, frame)
    record("differing_pixels_per_frame", differing)
    record("pixels_per_frame", W * H)
    print("glibc-mode parity %dx%d: differing pixels per frame %s of %d" % (W, H, differing, W * H))
    assert np.isfinite(a).all() and a.mean() > 1e-3
    return differing


def test_config3_full_size_within_tolerance_of_glibc_mode(hip, record_property):
    """BASELINE config 3 at 1920x1080 against the PINNED libm mode: three static frames and one of the orbit."""
    sd = get_scene("sponza:1.0")
    _frames_within_tolerance_of_the_pinned_mode(hip, sd, 1920, 1080, 3, 1, record_property)


def test_config5_full_size_within_tolerance_of_glibc_mode(hip, record_property):
    """BASELINE config 5's scene at 1920x1080 against the PINNED libm mode: one frame (its spatial pass reads the published
    reservoirs of 10 240 lights' RIS winners)."""
    sd = get_scene("bistro:1.0")
    _frames_within_tolerance_of_the_pinned_mode(hip, sd, 1920, 1080, 1, 0, record_property)


def test_config4_4k_frames_equal_oracle(hip, exact_libm):
    """BASELINE config 4's frame (the Sponza-class scene at 3840x2160) as one full frame on one GPU against the oracle: two
    frames, so the temporal merge runs at this size too.  (The strips of config 4 are compared with this full frame by
    test_config4_4k_eight_strips_equal_full_frame.)"""
    sd = get_scene("sponza:1.0")
    _frames_equal_oracle(hip, sd, 3840, 2160, 2, 0)


@pytest.mark.parametrize("name", ["sponza:1.0", "bistro:1.0"])
def test_full_scene_rays_equal_oracle(hip, monkeypatch, name):
    """DevScene::intersect and testOcclusion on the FULL scenes: 100 000 random / axis-aligned / near-zero-component rays
    (primitive, material, position, normal) and 400 000 shadow-like, grazing, axis-aligned, far-origin and degenerate segments:
    the fast paths (packet-free per-lane walk with the axis cull; shadow tree + ancestor verification) = the library's own
    reference walk (RS_NO_OCCLUSION_TREE) = the oracle, for every ray."""
    import torch
    sd = get_scene(name)
    osc = oracle_scene(sd)
    fast = hip_scene(hip, sd)
    rays = _random_rays(sd, 100000, 21)
    prim, mat, pos, nrm, _ = osc.intersect(rays)
    gp, gm, gpos, gn = hip.trace_closest(fast, torch.from_numpy(rays).cuda())
    assert np.array_equal(prim, gp.cpu().numpy())
    hit = prim >= 0
    assert hit.sum() > 10000
    assert np.array_equal(mat[hit], gm.cpu().numpy()[hit])
    assert bits_equal(pos[hit], gpos.cpu().numpy()[hit]) and bits_equal(nrm[hit], gn.cpu().numpy()[hit])

    seg = _shadow_like_segments(sd, 400000, 22)
    dseg = torch.from_numpy(seg).cuda()
    a = hip.trace_occlusion(fast, dseg).cpu().numpy()
    ref = osc.test_occlusion(seg)
    assert np.array_equal(ref, a), int((ref != a).sum())
    assert 0.05 < a.mean() < 0.95
    del fast
    monkeypatch.setenv("RS_NO_OCCLUSION_TREE", "1")
    slow = hip_scene(hip, sd)
    monkeypatch.delenv("RS_NO_OCCLUSION_TREE")
    b = hip.trace_occlusion(slow, dseg).cpu().numpy()
    assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["sponza:1.0", "bistro:1.0"])
def test_multi_bounce_kernels_full_size(hip, exact_libm, name):
    """The multi-bounce half at BASELINE sizes: pathTrace (direct + indirect images), pathTraceIndirect and two frames of ReSTIRIndirect
    with a moving camera at 1920x1080 on the FULL scenes, trace depth 4 -- every bounce ray through the closest-hit trees that keep the
    reference's visiting order (occlusion_bvh.cpp rs_build_ordered_bvh; 262 144 / 2.83 M triangles), every shadow ray through the shadow
    tree: images, ray counts and the indirect reservoirs bit for bit against the oracle."""
    import torch
    from restir_amd.scenes import orbit_position
    sd = get_scene(name)
    W, H = 1920, 1080
    o = OracleRenderer(sd, W, H)
    h = HipRenderer(hip, sd, W, H)
    assert hip.set_ordered_tree(h.scene, True)
    od = np.zeros((W * H, 3), np.float32); oi = np.zeros((W * H, 3), np.float32)
    hd = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda"); hi = torch.zeros_like(hd)
    ra = ob.path_trace(o.scene, o.cam, od, oi, 0, 3, 4)
    rb = hip.path_trace(h.scene, h.cam, hd.data_ptr(), hi.data_ptr(), 0, 3, 4)
    assert ra == rb, (ra, rb)
    assert bits_equal(od, hd.cpu().numpy()) and bits_equal(oi, hi.cpu().numpy()), radiance_stats(oi, hi.cpu().numpy())
    assert oi.max() > 0
    oi[:] = 0; hi.zero_()
    ra = ob.pt_indirect(o.scene, o.cam, oi, 0, 5, 4)
    rb = hip.path_trace_indirect(h.scene, h.cam, hi.data_ptr(), 0, 5, 4)
    assert ra == rb and bits_equal(oi, hi.cpu().numpy()), radiance_stats(oi, hi.cpu().numpy())
    oi[:] = 0; hi.zero_()
    for frame in range(2):
        p = orbit_position(sd.camera_args["position"], frame, radius=0.2)
        o.set_camera_position(p); h.set_camera_position(p)
        o.gbuf.render(o.scene, o.cam); h.gbuf.render(h.scene, h.cam)
        ra = o.restir.indirect(o.scene, o.cam, o.gbuf, oi, 0, frame, 1, 4)
        rb = h.restir.indirect(h.scene, h.cam, h.gbuf, hi.data_ptr(), 0, frame, 1, 4)
        assert ra == rb, (frame, ra, rb)
        assert bits_equal(oi, hi.cpu().numpy()), (frame, radiance_stats(oi, hi.cpu().numpy()))
        a, b = o.restir.ind_last, h.restir.download_indirect(1)
        assert np.array_equal(a["numSamples"], b["numSamples"])
        for k in ("Lo", "xv", "nv", "xs", "ns", "weight"):
            assert bits_equal(a[k], b[k]), (frame, k)
        o.gbuf.update(o.cam); h.gbuf.update(h.cam)


def test_svgf_full_size(hip, exact_libm):
    """SpatioTemporalFilter (src/denoiser.cu:136-216,250-371,479-568) at BASELINE size: six frames of an orbiting camera at 1920x1080 on the
    full Sponza-class scene (temporal accumulation through devMotion, the temporal-variance branch from the fifth frame on, five
    variance-guided a-trous levels from the row-phase LDS tiles), filtered image and filter state against the oracle within the
    filter's stated tolerance (rtol 3e-5: its exponentials are the hardware's)."""
    import torch
    from restir_amd.scenes import orbit_position
    sd = get_scene("sponza:1.0")
    W, H = 1920, 1080
    o = OracleRenderer(sd, W, H)
    h = HipRenderer(hip, sd, W, H)
    fo = ob.SVGF(W, H)
    fh = hip.SVGFFilter(W, H, 5)

    def grab(ptr, count):
        t = torch.empty(count, dtype=torch.float32, device="cuda")
        hip.hip_memcpy_d2d(t.data_ptr(), ptr, count * 4)
        return t.cpu().numpy()

    for frame in range(6):
        p = orbit_position(sd.camera_args["position"], frame, radius=0.3)
        o.set_camera_position(p); h.set_camera_position(p)
        o.gbuf.render(o.scene, o.cam); h.gbuf.render(h.scene, h.cam)
        o.restir.direct(o.scene, o.cam, o.gbuf, o.image, 0, o.looper, 1)
        h.restir.direct(h.scene, h.cam, h.gbuf, h.image.data_ptr(), 0, h.looper, 1)
        o.looper += 1; h.looper += 1
        assert bits_equal(o.image, h.image.cpu().numpy()), frame
        ref = fo.filter(o.image, o.gbuf, o.cam)
        got = grab(fh.filter(h.image.data_ptr(), h.gbuf, h.cam), W * H * 3).reshape(-1, 3)
        assert np.allclose(ref, got, rtol=3e-5, atol=2e-6), (frame, float(np.abs(ref - got).max()))
        st = fo.state(); v = fh.view()
        assert np.allclose(st["variance"], grab(v.devVariance, W * H), rtol=3e-5, atol=1e-6), frame
        assert np.allclose(st["accum_color"], grab(v.devAccumColor[v.frameIdx], W * H * 3).reshape(-1, 3), rtol=3e-5, atol=2e-6), frame
        fo.next_frame(); fh.next_frame()
        o.gbuf.update(o.cam); h.gbuf.update(h.cam)
    assert np.abs(ref - o.image).max() > 1e-3
    fh.destroy()


@pytest.mark.parametrize("name", ["sponza:1.0", "bistro:1.0"])
def test_path_trace_direct_full_size(hip, exact_libm, name):
    """PTDirectKernel (src/pathtrace.cu:279-328) at 1920x1080 on the full scenes, two accumulated frames: image and ray count bit for bit."""
    sd = get_scene(name)
    W, H = 1920, 1080
    o = OracleRenderer(sd, W, H)
    h = HipRenderer(hip, sd, W, H)
    for frame in range(2):
        a = o.frame(0, use_reservoir=False, iteration=frame)
        b = h.frame(0, use_reservoir=False, iteration=frame)
        assert o.rays == h.rays, (frame, o.rays, h.rays)
        assert bits_equal(a, b), (frame, radiance_stats(a, b))
    assert a.max() > 0
