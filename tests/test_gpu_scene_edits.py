"""Material, texture and environment-map edits between frames (rs_scene_set_materials, rs_scene_set_texture) against the CPU oracle,
bit for bit: every render path after every kind of edit, a scene's first map, the host tables against a fresh build, the refusals,
edits with frames in flight (the ring of eight versions wraps), retained G-buffer planes and row bands.  The oracle's side of an edit
is a scene built afresh from the edited arrays (tests/scene_edits.py)."""
import functools

import numpy as np
import pytest

from oracle import binding as ob
from restir_amd import sobol
from restir_amd.ctypes_structs import MATERIAL_DTYPE
from tests.common import RIS_TABLE_PIXELS_DEFAULT, EmissionEdits, bits_equal, get_scene, hip_scene, next_looper
from tests.scene_edits import (HipSide, OracleSide, apply_edit, assert_same, cornell_edit, differing, differing_mask, edited_materials)

pytestmark = pytest.mark.gpu

KINDS = ("materials", "texture", "environment")
W1, H1 = 97, 61                      # partial tiles on both axes
FRAMES, EDIT_FRAME, DEPTH = 6, 3, 3


@pytest.fixture(autouse=True)
def exact_libm(hip):
    ob.set_libm_mode(1)            # cos / sin correctly rounded on both sides: every bit must agree
    hip.set_sync(True)
    yield
    ob.set_libm_mode(0)
    hip.set_sync(True)
    hip.set_side_stream(4)         # the library's default
    hip.set_ris_table_pixels(RIS_TABLE_PIXELS_DEFAULT)


@functools.lru_cache(maxsize=None)
def scene_data(name):
    return get_scene(name)


@functools.lru_cache(maxsize=None)
def sobol_table():
    return sobol.sobol_table()


def with_libm(fn):
    """The oracle's cached references are computed under libm mode 1 whoever asks first."""
    @functools.wraps(fn)
    def wrapped(*a, **k):
        ob.set_libm_mode(1)
        return fn(*a, **k)
    return wrapped


# ---- 1. every render path after every kind of edit --------------------------------------------------------------------------------------
def direct_frames(side, sd, edit, reuse):
    """Six ReSTIRDirect frames, the edit before frame 3; what every frame left."""
    out = []
    for f in range(FRAMES):
        if f == EDIT_FRAME and edit is not None:
            apply_edit(side, edit)
        side.r.frame(reuse)
        out.append(side.direct_state())
    return out


@functools.lru_cache(maxsize=None)
@with_libm
def oracle_direct(kind, reuse):
    sd = scene_data("cornell_textured")
    return direct_frames(OracleSide(sd, W1, H1), sd, None if kind is None else cornell_edit(sd, kind), reuse)


# pixels of the 5 917 whose radiance differs from the unedited control's in the frame after the edit, reuse 3 (the oracle's own figures)
RADIANCE_CHANGED = {"materials": 1846, "environment": 5502, "texture": 1158}


def changed_pixels(a, b):
    """Pixels in which anything a frame left (radiance, reservoirs, G-buffer planes) differs between two runs."""
    m = None
    for k, x in a.items():
        if not isinstance(x, np.ndarray):
            continue
        d = np.any([differing_mask(x[n], b[k][n]) for n in x.dtype.names], axis=0) if x.dtype.names else differing_mask(x, b[k])
        m = d if m is None else (m | d)
    return int(m.sum())


@pytest.mark.parametrize("reuse", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_restir_direct_after_edit(hip, kind, reuse):
    """rs_restir_direct: radiance, reservoirs 1 and 2, ray counts and all G-buffer planes of six frames, the edit before frame 3.
    Not vacuous: what the oracle's frames after the edit leave differs from an unedited control's in at least 10 % of the pixels (the
    smallest share is the texture edit's, 1 253 of 5 917 = 21 %), and at reuse 3 the radiance alone in exactly RADIANCE_CHANGED pixels.
    The radiance alone does not reach 10 % in every mode: after the texture edit at reuse 0 it differs in 520, 492 and 487 pixels
    (8.8 %), while the albedo plane of the same frames differs in 1 253."""
    sd = scene_data("cornell_textured")
    ref, control = oracle_direct(kind, reuse), oracle_direct(None, reuse)
    n = W1 * H1
    for f in range(EDIT_FRAME):
        assert changed_pixels(ref[f], control[f]) == 0
    for f in range(EDIT_FRAME, FRAMES):
        changed, radiance = changed_pixels(ref[f], control[f]), differing(ref[f]["image"], control[f]["image"])
        print(kind, reuse, f, "changed pixels:", changed, "radiance:", radiance, "of", n)
        assert changed >= 0.10 * n, (kind, reuse, f, changed)
    if reuse == 3:
        assert differing(ref[EDIT_FRAME]["image"], control[EDIT_FRAME]["image"]) == RADIANCE_CHANGED[kind]
        assert RADIANCE_CHANGED[kind] >= 0.10 * n
    got = direct_frames(HipSide(hip, sd, W1, H1), sd, cornell_edit(sd, kind), reuse)
    for f in range(FRAMES):
        assert_same(ref[f], got[f], (kind, reuse, f))


class OracleMulti(OracleSide):
    def frames(self, path, edit):
        r, n = self.r, W1 * H1
        d, i = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        out = []
        for f in range(FRAMES):
            if f == EDIT_FRAME and edit is not None:
                apply_edit(self, edit)
            if path == "path_trace_direct":
                rays = ob.pt_direct(r.scene, r.cam, d, f, f)
                out.append(dict(direct=d.copy(), rays=rays))
            elif path == "path_trace":
                rays = ob.path_trace(r.scene, r.cam, d, i, f, f, DEPTH)
                out.append(dict(direct=d.copy(), indirect=i.copy(), rays=rays))
            elif path == "path_trace_indirect":
                rays = ob.pt_indirect(r.scene, r.cam, i, f, f, DEPTH)
                out.append(dict(indirect=i.copy(), rays=rays))
            else:
                r.gbuf.render(r.scene, r.cam)
                rays = r.restir.indirect(r.scene, r.cam, r.gbuf, i, 0, f, 1, DEPTH)
                r.gbuf.update(r.cam)
                out.append(dict(indirect=i.copy(), rays=rays, reservoirs=r.restir.ind_last.copy()))
        return out


class HipMulti(HipSide):
    def frames(self, capi, path, edit):
        import torch
        r, n = self.r, W1 * H1
        d = torch.zeros((n, 3), dtype=torch.float32, device="cuda"); i = torch.zeros_like(d)
        out = []
        for f in range(FRAMES):
            if f == EDIT_FRAME and edit is not None:
                apply_edit(self, edit)
            if path == "path_trace_direct":
                rays = capi.path_trace_direct(r.scene, r.cam, d.data_ptr(), f, f)
                out.append(dict(direct=d.cpu().numpy(), rays=rays))
            elif path == "path_trace":
                rays = capi.path_trace(r.scene, r.cam, d.data_ptr(), i.data_ptr(), f, f, DEPTH)
                out.append(dict(direct=d.cpu().numpy(), indirect=i.cpu().numpy(), rays=rays))
            elif path == "path_trace_indirect":
                rays = capi.path_trace_indirect(r.scene, r.cam, i.data_ptr(), f, f, DEPTH)
                out.append(dict(indirect=i.cpu().numpy(), rays=rays))
            else:
                r.gbuf.render(r.scene, r.cam)
                rays = r.restir.indirect(r.scene, r.cam, r.gbuf, i.data_ptr(), 0, f, 1, DEPTH)
                r.gbuf.update(r.cam)
                out.append(dict(indirect=i.cpu().numpy(), rays=rays, reservoirs=r.restir.download_indirect(1)))
        return out


PATHS = ("path_trace_direct", "path_trace", "path_trace_indirect", "restir_indirect")


# Pixels of the 5 917 in which what the frame after the edit left differs from the unedited control's, per path in the order of PATHS
# (the oracle's own figures).  These entry points leave images and reservoirs and no G-buffer planes, and a change of base colour or of
# a base-colour map reaches fewer of their pixels than of a ReSTIRDirect frame with its planes (pathTraceDirect after the texture edit:
# 261 = 4.4 %): the 10 % condition is asserted there (test_restir_direct_after_edit), here the figures are pinned.
MULTI_CHANGED = {"materials": (453, 882, 1333, 1925), "texture": (261, 537, 1005, 1383), "environment": (4208, 1584, 1422, 1422)}


@functools.lru_cache(maxsize=None)
@with_libm
def oracle_multi(kind, path):
    sd = scene_data("cornell_textured")
    return OracleMulti(sd, W1, H1).frames(path, None if kind is None else cornell_edit(sd, kind))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind", KINDS)
def test_multi_bounce_after_edit(hip, kind, path):
    """rs_path_trace_direct, rs_path_trace, rs_path_trace_indirect and rs_restir_indirect at depth 3: images, ray counts and the
    indirect reservoirs of six frames, the edit before frame 3 (the images accumulate over the frames, as Settings::accumulate)."""
    sd = scene_data("cornell_textured")
    ref, control = oracle_multi(kind, path), oracle_multi(None, path)
    n = W1 * H1
    for f in range(EDIT_FRAME, FRAMES):
        print(kind, path, f, "changed pixels:", changed_pixels(ref[f], control[f]), "of", n)
    assert changed_pixels(ref[EDIT_FRAME], control[EDIT_FRAME]) == MULTI_CHANGED[kind][PATHS.index(path)]
    got = HipMulti(hip, sd, W1, H1).frames(hip, path, cornell_edit(sd, kind))
    for f in range(FRAMES):
        assert_same(ref[f], got[f], (kind, path, f))


def generic_materials_edit(sd):
    """For any scene: the first non-Light material becomes a smooth metal of another colour, the second a Dielectric."""
    ids = np.nonzero(sd.materials["type"] != 4)[0][:2].astype(np.int32)
    m = sd.materials[ids].copy()
    m[0]["type"] = 1; m[0]["baseColor"] = (0.2, 0.8, 0.3); m[0]["metallic"] = 1.0; m[0]["roughness"] = 0.1
    m[1]["type"] = 2; m[1]["ior"] = 1.5
    return "set_materials", (ids, m)


@pytest.mark.parametrize("case", ["lds_table", "sobol"])
def test_restir_direct_after_edit_other_forms(hip, case):
    """A materials edit under the RIS form that keeps the light table in LDS (sponza:0.125 at 160 x 96 with rs_set_ris_table_pixels(0)),
    and an environment edit under the Sobol sampler."""
    if case == "lds_table":
        sd, W, H, table = scene_data("sponza:0.125"), 160, 96, None
        hip.set_ris_table_pixels(0)
        edit = generic_materials_edit(sd)
    else:
        sd, W, H, table = scene_data("cornell_textured"), W1, H1, sobol_table()
        edit = cornell_edit(sd, "environment")
    o, h = OracleSide(sd, W, H, sobol=table), HipSide(hip, sd, W, H, sobol=table)
    ref, got = direct_frames(o, sd, edit, 3), direct_frames(h, sd, edit, 3)
    for f in range(FRAMES):
        assert_same(ref[f], got[f], (case, f))
    assert differing(ref[EDIT_FRAME - 1]["albedo"], ref[EDIT_FRAME]["albedo"]) >= 0.10 * W * H


# ---- 2. a scene's first map ---------------------------------------------------------------------------------------------------------------
def test_first_map(hip):
    """Plain cornell (no map, no environment map: the untextured kernel variants, no texcoords on the device) at 33 x 9.  Material 1
    takes the procedural map; later material 0 takes it too and material 1 gives it back."""
    sd = scene_data("cornell")
    assert not len(sd.textures) and (sd.materials["baseColorMapId"] == -1).all()
    W, H = 33, 9
    o, h = OracleSide(sd, W, H), HipSide(hip, sd, W, H)
    m = sd.materials[[1, 0]].copy()
    m["baseColorMapId"] = -2
    back = sd.materials[[1]].copy()
    before = None
    for f in range(7):
        if f == 2:
            for s in (o, h):
                s.set_materials([1], m[:1])
        if f == 4:
            for s in (o, h):
                s.set_materials([0, 1], np.concatenate([m[1:], back]))
        o.r.frame(3); h.r.frame(3)
        a = o.direct_state()
        assert_same(a, h.direct_state(), f)
        if f in (2, 4):
            assert differing(a["albedo"], before["albedo"]) > 0
        before = a


# ---- 3. host tables -----------------------------------------------------------------------------------------------------------------------
def assert_desc_equal(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        if k == "textures":
            assert len(a[k]) == len(b[k]) and all(bits_equal(x, y) for x, y in zip(a[k], b[k])), (tag, k)
        elif k == "materials":
            assert a[k].tobytes() == b[k].tobytes(), (tag, k)
        elif isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and bits_equal(a[k], b[k]), (tag, k)
        else:
            assert a[k] == b[k], (tag, k)


def fresh(capi, sd, materials, textures):
    return capi.Scene(sd.vertices, sd.normals, sd.texcoords, sd.material_ids, materials, textures=textures, env_map_tex=sd.env_map_tex)


def test_host_tables_equal_fresh_build(hip):
    """After each kind of edit rs_scene_host_desc equals, array for array, that of a scene built afresh from the edited data; after an
    environment edit a following set_emission still does (it uses the new environment power)."""
    sd = scene_data("cornell_textured")
    s = hip_scene(hip, sd)
    mats, tex = sd.materials.copy(), [t.copy() for t in sd.textures]
    start = s.host_desc()
    for kind in KINDS:
        what, args = cornell_edit(sd, kind)
        if what == "set_materials":
            s.set_materials(*args)
            mats = edited_materials(mats, *args)
        else:
            s.set_texture(*args)
            tex[args[0]] = args[1]
        d = s.host_desc()
        assert_desc_equal(d, fresh(hip, sd, mats, tex).host_desc(), kind)
        assert bits_equal(d["textures"][args[0]], args[1]) if what == "set_texture" else d["materials"].tobytes() == mats.tobytes()
    assert start["sum_power"] != d["sum_power"] and not bits_equal(start["env_prob"], d["env_prob"])
    ids, rad = EmissionEdits(sd, 5).next()
    s.set_emission(ids, rad)
    mats["baseColor"][ids] = rad
    assert_desc_equal(s.host_desc(), fresh(hip, sd, mats, tex).host_desc(), "emission after environment")
    s.set_materials([], np.zeros(0, MATERIAL_DTYPE))              # count == 0 succeeds and changes nothing
    assert_desc_equal(s.host_desc(), fresh(hip, sd, mats, tex).host_desc(), "empty edit")


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------
def refused(capi, call, *args):
    with pytest.raises(capi.RestirHipError) as e:
        call(*args)
    assert str(e.value).startswith("librestir_hip error 10001:"), str(e.value)          # RS_ERR_INVALID_ARGUMENT


def test_refusals_leave_scene_unchanged(hip):
    import ctypes as C
    sd = scene_data("cornell_textured")
    W, H = 33, 9
    o, h = OracleSide(sd, W, H), HipSide(hip, sd, W, H)
    s = h.r.scene
    nm, nt = len(sd.materials), len(sd.textures)
    light = int(np.nonzero(sd.materials["type"] == 4)[0][0])
    rec = sd.materials[[0]].copy()

    def rec_with(**kw):
        r = rec.copy()
        for k, v in kw.items():
            r[k] = v
        return r
    L = hip.lib()
    ids1 = np.array([0], np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    cases = [
        ("null ids", lambda: hip.check(L.rs_scene_set_materials(s.handle, 1, None, p(rec)))),
        ("null records", lambda: hip.check(L.rs_scene_set_materials(s.handle, 1, p(ids1), None))),
        ("negative count", lambda: hip.check(L.rs_scene_set_materials(s.handle, -1, p(ids1), p(rec)))),
        ("id below", lambda: s.set_materials([-1], rec)),
        ("id beyond", lambda: s.set_materials([nm], rec)),
        ("is a Light", lambda: s.set_materials([light], rec)),
        ("becomes a Light", lambda: s.set_materials([0], rec_with(type=4))),
        ("second of two is bad", lambda: s.set_materials([1, light], np.concatenate([rec, rec]))),
        ("map beyond the table", lambda: s.set_materials([0], rec_with(roughnessMapId=nt))),
        ("base colour map -3", lambda: s.set_materials([0], rec_with(baseColorMapId=-3))),
        ("normal map -2", lambda: s.set_materials([0], rec_with(normalMapId=-2))),
        ("texture dimensions", lambda: s.set_texture(0, np.zeros((32, 16, 3), np.float32))),
        ("texture id below", lambda: s.set_texture(-1, sd.textures[0])),
        ("texture id beyond", lambda: s.set_texture(nt, sd.textures[0])),
        ("black environment", lambda: s.set_texture(sd.env_map_tex, np.zeros_like(sd.textures[sd.env_map_tex]))),
        ("infinite environment", lambda: s.set_texture(sd.env_map_tex, np.full_like(sd.textures[sd.env_map_tex], np.inf))),
    ]
    desc = s.host_desc()
    for name, call in cases:
        refused(hip, call)
        assert_desc_equal(s.host_desc(), desc, name)
        o.r.frame(3); h.r.frame(3)
        assert_same(o.direct_state(), h.direct_state(), name)


def test_first_map_refused_without_texcoords(hip):
    """rs_scene_create's rule: texture maps need texcoords.  A scene created with texcoords == NULL refuses its first map."""
    sd = scene_data("cornell")
    W, H = 33, 9
    o, h = OracleSide(sd, W, H), HipSide(hip, sd, W, H)
    t = h.r.scene.host_desc()
    bare = hip.Scene.from_tables(sd.vertices, sd.normals, None, sd.material_ids, sd.materials, t)
    h.r.scene = bare
    desc = bare.host_desc()
    m = sd.materials[[1]].copy()
    m["baseColorMapId"] = -2
    refused(hip, bare.set_materials, [1], m)
    assert_desc_equal(bare.host_desc(), desc, "first map")
    m = sd.materials[[1]].copy()
    m["roughness"] = 0.25
    bare.set_materials([1], m)                        # an edit without a map is taken
    o.set_materials([1], m)
    for f in range(2):
        o.r.frame(3); h.r.frame(3)
        assert_same(o.direct_state(), h.direct_state(), f)


# ---- 5. frames in flight ------------------------------------------------------------------------------------------------------------------
N_FLIGHT, BURST_FRAME = 20, 11


def flight_edits(sd):
    """Frame -> the edits before it: one before every frame, cycling through materials, texture, environment and emission, and a burst
    of ten more before frame 11.  Thirty edits in all: the ring of eight versions wraps three times."""
    rng = np.random.default_rng(7)
    lamps = EmissionEdits(sd, 8)
    env = sd.env_map_tex

    def one(i):
        k = i % 4
        if k == 0:
            ids = np.array([2, 4, 0], np.int32)
            m = sd.materials[ids].copy()
            m[0]["baseColor"] = rng.uniform(0.05, 0.95, 3)
            m[1]["roughness"] = rng.uniform(0.02, 0.9); m[1]["metallic"] = rng.uniform(0, 1)
            m[2]["baseColorMapId"] = (-1, 0, -2)[(i // 4) % 3]
            return "set_materials", (ids, m)
        if k == 1:
            return "set_texture", (0, (sd.textures[0] * rng.uniform(0.3, 1.1, (1, 1, 3))).astype(np.float32))
        if k == 2:
            e = (sd.textures[env] * np.float32(rng.uniform(0.2, 1.5))).astype(np.float32)
            y, x = int(rng.integers(0, 29)), int(rng.integers(0, 60))
            e[y:y + 3, x:x + 4] = rng.uniform(5, 90, 3)
            return "set_texture", (env, e)
        return "set_emission", lamps.next()
    plan, i = {}, 0
    for f in range(N_FLIGHT):
        k = 11 if f == BURST_FRAME else 1
        plan[f] = [one(i + j) for j in range(k)]
        i += k
    return plan


@functools.lru_cache(maxsize=None)
@with_libm
def oracle_flight():
    sd = scene_data("cornell_textured")
    o = OracleSide(sd, 128, 128)
    plan = flight_edits(sd)
    out = []
    for f in range(N_FLIGHT):
        for e in plan[f]:
            apply_edit(o, e)
        o.r.frame(3)
        out.append(o.image())
    return out, o.direct_state()


@pytest.mark.parametrize("side_stream", [4, 0], ids=["overlapped", "no_side_streams"])
def test_edits_with_frames_in_flight(hip, side_stream):
    """Overlapped mode, 128 x 128, 20 frames with no host synchronisation between them; every frame's image is copied device to device
    into its own buffer and read after the last frame."""
    import torch
    sd = scene_data("cornell_textured")
    W = H = 128
    ref, final = oracle_flight()
    plan = flight_edits(sd)
    hip.set_side_stream(side_stream)
    h = HipSide(hip, sd, W, H)
    outs = [torch.zeros((W * H, 3), dtype=torch.float32, device="cuda") for _ in range(N_FLIGHT)]
    hip.set_sync(False)
    try:
        r = h.r
        for f in range(N_FLIGHT):
            for e in plan[f]:
                apply_edit(h, e)
            r.gbuf.render(r.scene, r.cam)
            r.restir.direct(r.scene, r.cam, r.gbuf, r.image.data_ptr(), 0, r.looper, 3)
            r.looper += 1
            r.gbuf.update(r.cam)
            hip.hip_memcpy_d2d_async(outs[f].data_ptr(), r.image.data_ptr(), W * H * 12)
        hip.synchronize()
    finally:
        hip.set_sync(True)
        hip.set_side_stream(4)
    for f in range(N_FLIGHT):
        b = outs[f].cpu().numpy()
        assert bits_equal(ref[f], b), (f, differing(ref[f], b))
    h.r.rays = h.r.restir.ray_count()
    assert_same(final, h.direct_state(), "final")


# ---- 6. retained G-buffer planes ------------------------------------------------------------------------------------------------------------
def test_retained_planes_follow_edits(hip):
    """Still camera, reuse on.  Once requests are answered from retained planes, a materials edit that changes only a roughness makes
    the next request render, and so does a texture edit of a normal map; with no edit the counters go on as before."""
    sd = scene_data("cornell_textured")
    W, H = 97, 61
    o, h = OracleSide(sd, W, H), HipSide(hip, sd, W, H)
    g = h.r.gbuf

    def frame(tag):
        o.r.frame(3); h.r.frame(3)
        assert_same(o.direct_state(), h.direct_state(), tag)
        return g.reuse_stats()
    for f in range(4):
        rendered, reused = frame(f)
    assert reused >= 1                                   # the planes are being reused
    r0, u0 = frame("still")
    assert (r0, u0) == (rendered, reused + 1)            # no edit: answered from the retained planes again
    rough = sd.materials[[4]].copy()
    rough["roughness"] = 0.9
    for s in (o, h):
        s.set_materials([4], rough)
    r1, u1 = frame("roughness")
    assert (r1, u1) == (r0 + 1, u0), "the request after a materials edit must render"
    while g.reuse_stats()[1] == u1:
        assert g.reuse_stats()[0] < r1 + 4
        frame("settling")
    r2, u2 = g.reuse_stats()
    bumps = (sd.textures[3][::-1] * np.float32(1.0)).copy()
    bumps[..., :2] = 1.0 - bumps[..., :2]
    normal_before = o.gbuffer()["normal"]
    for s in (o, h):
        s.set_texture(3, bumps)
    r3, u3 = frame("normal map")
    assert (r3, u3) == (r2 + 1, u2), "the request after a texture edit must render"
    assert differing(o.gbuffer()["normal"], normal_before) > 0


# ---- 7. row bands -------------------------------------------------------------------------------------------------------------------------
def test_row_bands_with_edits(hip):
    """rs_restir_phase_a / _phase_b on two bands of a 70 x 99 frame, an edit of every kind between frames: the banded library equals the
    oracle's full frame."""
    sd = scene_data("cornell_textured")
    W, H = 70, 99
    bands = [(0, 41), (41, H)]
    o, h = OracleSide(sd, W, H), HipSide(hip, sd, W, H)
    for f in range(7):
        if f in (2, 3, 5):
            e = cornell_edit(sd, KINDS[(2, 3, 5).index(f)])
            apply_edit(o, e); apply_edit(h, e)
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


def test_tracked_restir_under_material_and_emission_edits(hip):
    """A tracked rs_restir under a materials edit and an emission edit in the same run equals the tracked oracle, light indices
    included (the edited scene stays the same scene: the indices are kept)."""
    sd = scene_data("cornell_textured")
    W, H = 97, 61
    o, h = OracleSide(sd, W, H, track=True), HipSide(hip, sd, W, H, track=True)
    lamps = EmissionEdits(sd, 3)
    for f in range(7):
        if f in (2, 5):
            e = cornell_edit(sd, "materials") if f == 2 else generic_materials_edit(sd)
            apply_edit(o, e); apply_edit(h, e)
        if f in (3, 5):
            e = ("set_emission", lamps.next())
            apply_edit(o, e); apply_edit(h, e)
        o.r.frame(3); h.r.frame(3)
        assert_same(o.direct_state(), h.direct_state(), f)
        for which in (0, 1, 2):
            assert np.array_equal(o.r.light_ids(which), h.r.light_ids(which)), (f, which)
    assert (h.r.light_ids(1) >= 0).any()
