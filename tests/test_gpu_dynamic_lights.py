"""Dynamic light emission: rs_scene_set_emission (stream-ordered edits of the Light materials' radiance) and the opt-in temporal
re-evaluation of ReSTIR-DI (rs_restir_set_light_tracking)."""
import numpy as np
import pytest

from restir_amd import scenes
from restir_amd.ctypes_structs import LIGHT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from restir_amd import capi
    capi.init(0)
    capi.set_sync(True)
    yield capi
    capi.set_sync(True)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def make_scene(capi, sd, materials=None):
    return capi.Scene(sd.vertices, sd.normals, sd.texcoords, sd.material_ids, sd.materials if materials is None else materials,
                      textures=sd.textures, env_map_tex=sd.env_map_tex)


def light_materials(sd):
    return np.nonzero(sd.materials["type"] == LIGHT)[0].astype(np.int32)


def edited(sd, ids, radiance):
    m = sd.materials.copy()
    m["baseColor"][ids] = radiance
    return m


def random_edit(sd, seed, frac=0.25):
    """A random subset of the lamps: half of it recoloured, half switched off."""
    rng = np.random.default_rng(seed)
    lm = light_materials(sd)
    ids = rng.choice(lm, max(2, int(len(lm) * frac)), replace=False).astype(np.int32)
    rad = rng.uniform(0.5, 40.0, (len(ids), 3)).astype(np.float32)
    rad[: len(ids) // 2] = 0.0
    return ids, rad


DESC_KEYS = ("light_prim_ids", "light_radiance", "light_prob", "light_fail", "sum_power", "env_prob", "env_fail", "boxes", "nodes")


def assert_desc_equal(a, b):
    for k in DESC_KEYS:
        assert same(a[k], b[k]), k
    assert a["num_lights"] == b["num_lights"]


class Frames:
    """runCuda's sequence (gbuffer render, ReSTIRDirect, gbuffer update) on one scene, one output buffer per frame if asked."""

    def __init__(self, capi, sd, scene, W, H, track=False, orbit=False):
        import torch
        self.capi, self.sd, self.scene, self.W, self.H, self.orbit = capi, sd, scene, W, H, orbit
        self.torch = torch
        self.cam = capi.camera_update(sd.camera(W, H))
        self.base = sd.camera_args["position"]
        self.gbuf = capi.GBuffer(W, H)
        self.restir = capi.ReSTIR(W, H)
        if track:
            self.restir.set_light_tracking(True)
        self.looper = 0
        self.image = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")

    def _move(self):
        if self.orbit:
            p = scenes.orbit_position(self.base, self.looper, radius=1.0)
            for i in range(3):
                self.cam.position[i] = float(p[i])
            self.capi.camera_update(self.cam)

    def render_gbuffer(self):
        self._move()
        self.gbuf.render(self.scene, self.cam)

    def shade(self, out=None, reuse=3):
        out = self.image if out is None else out
        self.restir.direct(self.scene, self.cam, self.gbuf, out.data_ptr(), 0, self.looper, reuse)
        self.looper += 1
        self.gbuf.update(self.cam)
        return out

    def frame(self, reuse=3):
        self.render_gbuffer()
        return self.shade(reuse=reuse).cpu().numpy()

    def resv(self):
        return self.restir.download(1)          # after end_frame: what this frame published

    def albedo(self):
        return self.gbuf.download()["albedo"]   # the last render's


def small_sponza():
    return scenes.sponza_class(1, 0.125)


# ---- 1. tables -------------------------------------------------------------------------------------------------------------------
def test_tables_equal_fresh_build(hip):
    sd = scenes.sponza_class(1, 1.0)                  # 1 024 lamps
    assert len(light_materials(sd)) == 512
    ids, rad = random_edit(sd, 11)
    s = make_scene(hip, sd)
    s.set_emission(ids, rad)
    fresh = make_scene(hip, sd, edited(sd, ids, rad))
    assert_desc_equal(s.host_desc(), fresh.host_desc())
    # the materials rs_scene_host_desc hands out are the edited ones
    d = s.host_desc()
    assert not same(d["light_prob"], make_scene(hip, sd).host_desc()["light_prob"])
    # a second edit of the same scene, back to the original radiance
    s.set_emission(ids, sd.materials["baseColor"][ids])
    assert_desc_equal(s.host_desc(), make_scene(hip, sd).host_desc())


def test_tables_equal_fresh_build_env(hip):
    sd = scenes.cornell_textured(env=True)
    lm = light_materials(sd)
    rad = np.array([[3.0, 5.0, 7.5]], np.float32)
    s = make_scene(hip, sd)
    s.set_emission(lm, rad)
    fresh = make_scene(hip, sd, edited(sd, lm, rad))
    assert_desc_equal(s.host_desc(), fresh.host_desc())
    # switching the lamp off leaves the environment map's entry, which keeps its power
    zero = np.zeros((1, 3), np.float32)
    s.set_emission(lm, zero)
    fresh0 = make_scene(hip, sd, edited(sd, lm, zero))
    assert_desc_equal(s.host_desc(), fresh0.host_desc())
    # a scene made from a description (rs_scene_create) does not carry the entry's power: it is recomputed from the texture
    t = make_scene(hip, sd).host_desc()
    c = hip.Scene.from_tables(sd.vertices, sd.normals, sd.texcoords, sd.material_ids, sd.materials, t, textures=sd.textures,
                              env_map_tex=sd.env_map_tex, env_sampler=(t["env_prob"], t["env_fail"]))
    c.set_emission(lm, rad)
    assert_desc_equal(c.host_desc(), fresh.host_desc())


# ---- 2. every pass after an edit equals a fresh scene -------------------------------------------------------------------------------
def test_passes_after_edit_equal_fresh_scene(hip):
    import torch
    sd = small_sponza()
    W, H = 160, 96
    ids, rad = random_edit(sd, 5, frac=0.5)
    s = make_scene(hip, sd)
    s.set_sample_sequence(None)
    fresh = make_scene(hip, sd, edited(sd, ids, rad))
    fresh.set_sample_sequence(None)
    cam = hip.camera_update(sd.camera(W, H))

    def direct(scene):
        img = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
        hip.path_trace_direct(scene, cam, img.data_ptr(), 0, 7)
        return img.cpu().numpy()

    def path(scene):
        a = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
        b = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
        hip.path_trace(scene, cam, a.data_ptr(), b.data_ptr(), 0, 3, 4)
        return a.cpu().numpy(), b.cpu().numpy()

    before = direct(s)                                   # the scene's first version is in use ...
    r_old = Frames(hip, sd, s, W, H)
    r_old.frame(3)
    s.set_emission(ids, rad)                             # ... then edited
    assert not same(before, direct(s))
    assert same(direct(s), direct(fresh))
    pa, pb = path(s), path(fresh)
    assert same(pa[0], pb[0]) and same(pa[1], pb[1])

    a, b = Frames(hip, sd, s, W, H), Frames(hip, sd, fresh, W, H)
    assert same(a.frame(0), b.frame(0))                  # G-buffer + ReSTIRDirect at reuse 0
    ga, gb = a.gbuf.download(), b.gbuf.download()
    assert same(ga["albedo"], gb["albedo"])              # light pixels show the new emission
    a, b = Frames(hip, sd, s, W, H), Frames(hip, sd, fresh, W, H)
    for _ in range(4):                                   # spatiotemporal frames of an rs_restir whose first frame follows the edit
        assert same(a.frame(3), b.frame(3))
        assert same_rows(a.resv(), b.resv()).all()


# ---- 3. exact re-evaluation ------------------------------------------------------------------------------------------------------------
def fresh_slots(now, two_back):
    """Slots published by this frame: a pixel that shades nothing keeps the value its slot had two frames back (Q1)."""
    return ~(same_rows(now, two_back))


def twice(a, b, alb_a, alb_b):
    """Frame b is frame a under doubled emission.  ReSTIRDirect writes direct * albedo (restir.cu:220-230): direct doubles where the
    jittered ray shaded a surface and is 1 where it hit a light (baseColor forced to 1, restir.cu:143-146), and the G-buffer albedo
    (the pixel-centre ray) is the emission where that ray hit a light.  So b = 2 f a with f = 2 on the G-buffer's light pixels,
    else 1 -- or b = albedo where the jittered ray hit a light."""
    f = np.where(same_rows(alb_b, 2 * alb_a) & np.any(alb_a != 0, axis=1), 2.0, 1.0).astype(np.float32)[:, None]
    light = same_rows(a, alb_a) & same_rows(b, alb_b)
    assert light.sum() < len(a) // 4
    return bool((light | same_rows(b, 2 * f * a)).all())


def same_rows(a, b):
    va = np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)
    vb = np.ascontiguousarray(b).view(np.uint8).reshape(len(b), -1)
    return np.all(va == vb, axis=1)


def test_tracking_rescales_exactly(hip):
    sd = small_sponza()
    W, H = 160, 96
    lm = light_materials(sd)
    E = sd.materials["baseColor"][lm].astype(np.float32)
    K, N = 3, 4

    # premise: a fresh 2E scene renders exactly 2x the E scene, reservoir weights included
    e_run = Frames(hip, sd, make_scene(hip, sd), W, H)
    d_run = Frames(hip, sd, make_scene(hip, sd, edited(sd, lm, 2 * E)), W, H)
    for _ in range(K + N):
        x, y = e_run.frame(3), d_run.frame(3)
        assert twice(x, y, e_run.albedo(), d_run.albedo())
        ra, rb = d_run.resv(), e_run.resv()
        assert same(ra["weight"], 2 * rb["weight"]) and same(ra["Li"], 2 * rb["Li"])

    def run(track):
        ref = Frames(hip, sd, make_scene(hip, sd), W, H, track=True)
        sw = Frames(hip, sd, make_scene(hip, sd), W, H, track=track)
        hist = []
        for f in range(K + N):
            if f == K:
                sw.scene.set_emission(lm, 2 * E)
            a, b = sw.frame(3), ref.frame(3)
            hist.append((a, b, sw.resv(), ref.resv(), sw.albedo(), ref.albedo()))
        return hist

    hist = run(True)
    for f in range(K):
        assert same(hist[f][0], hist[f][1])
    for f in range(K, K + N):
        a, b, ra, rb, aa, ab = hist[f]
        assert twice(b, a, ab, aa), f
        m = fresh_slots(rb, hist[f - 2][3])
        assert m.sum() > W * H // 2
        assert same(ra["weight"][m], 2 * rb["weight"][m]), f
        assert same(ra["Li"][m], 2 * rb["Li"][m]), f
        assert same(ra["numSamples"][m], rb["numSamples"][m]), f
    # self-check: without re-evaluation the frame after the switch is not 2x
    off = run(False)
    assert not twice(off[K][1], off[K][0], off[K][5], off[K][4])


# ---- 4. neutral when nothing changes ------------------------------------------------------------------------------------------------
def test_tracking_neutral_config3(hip):
    sd = scenes.sponza_class(1, 1.0)
    W, H = 1920, 1080
    lm = light_materials(sd)
    E = sd.materials["baseColor"][lm].astype(np.float32)

    def run(track, edit):
        r = Frames(hip, sd, make_scene(hip, sd), W, H, track=track, orbit=True)
        out = []
        for f in range(8):
            if edit and f == 3:
                r.scene.set_emission(lm, E)              # an edit to identical values
            out.append((r.frame(3), r.resv()))
        return out

    base = run(False, False)
    for other in (run(True, False), run(True, True)):
        for (a, ra), (b, rb) in zip(base, other):
            assert same(a, b)
            assert same_rows(ra, rb).all()


# ---- 5. lights off ------------------------------------------------------------------------------------------------------------------
def test_lights_off_stop_winning(hip):
    sd = small_sponza()
    W, H = 160, 96
    lm = light_materials(sd)
    off = lm[: len(lm) // 2]
    E = sd.materials["baseColor"]
    K, N = 4, 4

    def run(track):
        s = make_scene(hip, sd)
        d = s.host_desc()
        light_mat = sd.material_ids[d["light_prim_ids"]]
        off_ids = np.nonzero(np.isin(light_mat, off))[0]                  # light-sampler indices of the lamps switched off
        off_le = {tuple(E[m].astype(np.float32).view(np.uint32)) for m in off}
        r = Frames(hip, sd, s, W, H, track=track)
        hist, ghosts = [], []
        for f in range(K + N):
            if f == K:
                s.set_emission(off, np.zeros((len(off), 3), np.float32))
            r.frame(3)
            rv = r.resv()
            ids = r.restir.download_light_ids(1)
            hist.append(rv)
            if f >= K:
                m = fresh_slots(rv, hist[f - 2]) & (rv["weight"] > 0)
                le = {tuple(x) for x in rv["Li"][m].astype(np.float32).view(np.uint32).reshape(-1, 3)}
                by_id = np.isin(ids[m], off_ids).sum() if track else 0
                ghosts.append((len(le & off_le), by_id))
        return ghosts

    on = run(True)
    assert all(g == (0, 0) for g in on), on
    assert any(g[0] > 0 for g in run(False))          # self-check: the reference's merge keeps some of them


# ---- 6. frames in flight ------------------------------------------------------------------------------------------------------------
def test_edit_between_frames_in_flight(hip):
    import torch
    sd = small_sponza()
    W, H = 256, 160
    lm = light_materials(sd)
    E = sd.materials["baseColor"][lm].astype(np.float32)
    K, N = 4, 4

    # the camera does not move: the G-buffer albedo is the same in every frame (the pixel-centre ray)
    alb = {}
    for k, mats in (("E", sd.materials), ("2E", edited(sd, lm, 2 * E))):
        g = Frames(hip, sd, make_scene(hip, sd, mats), W, H)
        g.frame(3)
        alb[k] = g.albedo()

    def run(edit):
        hip.set_sync(False)
        try:
            r = Frames(hip, sd, make_scene(hip, sd), W, H, track=True)
            outs = [torch.zeros((W * H, 3), dtype=torch.float32, device="cuda") for _ in range(K + N)]
            for f in range(K + N):
                r.render_gbuffer()                           # asynchronous mode: recorded, launched with the primary rays
                if edit and f == K:
                    r.scene.set_emission(lm, 2 * E)          # no synchronisation; the render of frame K is still deferred
                r.shade(outs[f])
            hip.synchronize()
            return [o.cpu().numpy() for o in outs]
        finally:
            hip.set_sync(True)

    ref, got = run(False), run(True)
    for f in range(K):
        assert same(got[f], ref[f]), f
    for f in range(K, K + N):      # frame K: its G-buffer render was recorded before the edit and shows the old emission
        assert twice(ref[f], got[f], alb["E"], alb["E"] if f == K else alb["2E"]), f


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_scene_unchanged(hip):
    sd = scenes.cornell_box()
    lm = light_materials(sd)
    s = make_scene(hip, sd)
    before = s.host_desc()
    mats_before = sd.materials.copy()
    one = np.array([[1.0, 2.0, 3.0]], np.float32)
    bad = [
        (np.array([len(sd.materials)], np.int32), one),            # out of range
        (np.array([-1], np.int32), one),
        (np.array([0], np.int32), one),                            # not a Light material
        (lm, np.array([[-1.0, 1.0, 1.0]], np.float32)),
        (lm, np.array([[np.nan, 1.0, 1.0]], np.float32)),
        (lm, np.array([[np.inf, 1.0, 1.0]], np.float32)),
        (lm, np.zeros((1, 3), np.float32)),                        # no power left in the light sampler
    ]
    for ids, rad in bad:
        with pytest.raises(hip.RestirHipError, match="10001"):
            s.set_emission(ids, rad)
        assert_desc_equal(s.host_desc(), before)
    from restir_amd.capi import lib
    assert lib().rs_scene_set_emission(s.handle, -1, None, None) == 10001
    assert lib().rs_scene_set_emission(None, 0, None, None) == 10001
    assert_desc_equal(s.host_desc(), before)
    assert np.array_equal(sd.materials, mats_before)
    s.set_emission(lm[:0], one[:0])                                # an empty edit is accepted and changes nothing
    assert_desc_equal(s.host_desc(), before)


def test_strip_driver_refuses_tracking(hip):
    import torch
    sd = scenes.cornell_box()
    W, H = 64, 48
    s = make_scene(hip, sd)
    cam = hip.camera_update(sd.camera(W, H))
    g = hip.GBuffer(W, H)
    r = hip.ReSTIR(W, H)
    r.set_light_tracking(True)
    comm = hip.Comm(0, 1, lambda *a: None, lambda *a: None)
    drv = hip.Strips(comm, W, H)
    img = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(hip.RestirHipError, match="10002"):
        drv.frame(r, s, cam, g, img.data_ptr(), 0, 0, 3)
    with pytest.raises(hip.RestirHipError, match="10002"):
        drv.exchange_history(r, g)
    r.set_light_tracking(False)
    drv.frame(r, s, cam, g, img.data_ptr(), 0, 0, 3)               # untracked: as before
    hip.synchronize()
    assert (r.download_light_ids(1) == -1).all()
