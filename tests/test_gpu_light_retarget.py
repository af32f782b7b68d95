"""Light retargeting (rs_restir_set_light_retargeting) on the GPU.  Against the CPU oracle composed with the NumPy restatement of
tests/light_retarget.py, bit for bit: radiance, the reservoirs last written and published, the records' lights, the ray count and the
kernel's own counters, after every kind of emitter edit, with a still and an orbiting camera, both samplers, every RIS form.  GPU
against GPU: the identities the issue names.  Behaviour: the first frame after a lamp moved is closer to the converged render of the new
pose with retargeting than without.  tests/test_light_retarget_host.py shows without a GPU that the restatement means something."""
import numpy as np
import pytest

from oracle import binding as ob
from restir_amd import sobol
from tests import light_retarget as lr
from tests.common import EmissionEdits, HipRenderer, bits_equal
from tests.emitter_edits import emitter_edit, emitters, kinds_for, lamp_of, scene_data
from tests.geometry_edits import geometry_edit, root_box
from tests.scene_edits import assert_same

pytestmark = pytest.mark.gpu

W, H = 70, 45                        # off the 8x8 and the 32x8 grids
GLOBAL_TABLE = 64 * 1024           # rs_set_ris_table_pixels: the library's default, launches of fewer pixels read the light table from global memory
KINDS = ("one", "all", "mixed", "scale_up", "flip", "collapse", "restore")


@pytest.fixture(autouse=True)
def exact_libm(hip):
    ob.set_libm_mode(1)              # cos / sin correctly rounded on both sides: every bit must agree
    hip.set_sync(True)
    yield
    ob.set_libm_mode(0)
    hip.set_sync(True)
    hip.set_ris_table_pixels(GLOBAL_TABLE)


def kinds_of(name):
    return [k for k in KINDS if k in kinds_for(name)]


def check_frame(pair, reuse, tag, moved):
    got, ref, stats, counts = pair.frame(reuse)
    assert_same(ref, got, tag)
    assert stats == counts, (tag, stats, counts)
    # An edit of every lamp finds samples to evaluate wherever a reservoir holds one.  An edit of ONE lamp need not: one lamp of bistro's
    # 1228 may be no pixel's sample, and after `flip` the edited lamp shines upwards, so `collapse` and `restore` of one of its triangles
    # find next to none.  There the counters equal the restatement's, zero or not; the callers ask for a non-zero sum over all edits.
    # On cornell and single the one lamp lights the whole room: `one`, the first edit, always finds samples too.
    if moved and (reuse & 1) and (tag[-1] == "all" or (tag[-1] == "one" and tag[0] in ("cornell", "single"))):
        assert stats[0] > 0, (tag, "the kernel evaluated nothing")
    assert pair.h.r.restir.retarget_launched() == bool(moved and (reuse & 1)), (tag, "the kernel is launched after an emitter edit and only then")
    if not moved:
        assert stats == (0, 0, 0), (tag, stats)
    return stats


def run_edits(hip, name, reuse, size=(W, H), sampler="engine", orbit=False, kinds=None, ris_pixels=GLOBAL_TABLE):
    hip.set_ris_table_pixels(ris_pixels)
    pair = lr.Pair(hip, name, size[0], size[1], sobol=sobol.sobol_table() if sampler == "sobol" else None)
    sd = pair.sd
    base = np.array([pair.o.r.cam.position[i] for i in range(3)], np.float32)
    frame = [0]

    def step(tag, moved):
        if orbit:
            t = np.float32(0.9 * frame[0])                 # (far enough per frame, and along the view too, that pixels share history slots)
            p = base + np.float32(0.3) * np.array([np.cos(t), 0.5 * np.sin(t), np.sin(t)], np.float32)
            pair.o.r.set_camera_position(p); pair.h.r.set_camera_position(p)
        frame[0] += 1
        return check_frame(pair, reuse, (name, reuse, sampler, orbit, tag), moved)

    for f in range(3):
        step("warm %d" % f, False)
    walked = zeroed = carried = 0
    groups = 1
    for kind in kinds or kinds_of(name):
        pair.edit(*emitter_edit(sd, pair.o.r.scene.vertices, kind, seed=13))
        s = step(kind, True)
        walked += s[1]; zeroed += s[2]
        groups = max(groups, pair.groups)
        carried += pair.carried[0]
        step("after " + kind, False)
        carried += pair.carried[0]
    assert carried > 0 or not (reuse & 1), "no published reservoir held its temporal candidate: the carried records were never compared"
    return walked, zeroed, groups


# ---- (a) still camera ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,reuse,sampler,ris_pixels", [
    ("cornell", 3, "engine", GLOBAL_TABLE), ("cornell", 1, "engine", 0), ("cornell", 3, "sobol", 0), ("cornell", 3, "sobol", GLOBAL_TABLE),
    ("many", 3, "engine", GLOBAL_TABLE), ("many", 1, "engine", 0), ("bistro", 3, "engine", 0), ("bistro", 1, "engine", GLOBAL_TABLE),
    ("bistro", 3, "sobol", 0), ("env", 3, "engine", GLOBAL_TABLE), ("env", 1, "sobol", GLOBAL_TABLE)])
def test_edits_with_a_still_camera(hip, name, reuse, sampler, ris_pixels):
    """ris_pixels 0: the light table in LDS (k_ris_lds; with bistro's 1228 lights the alias table alone, k_ris_alias_lds); GLOBAL_TABLE: from global
    memory at this size (k_ris, with `env` its environment form)."""
    walked, zeroed, groups = run_edits(hip, name, reuse, sampler=sampler, ris_pixels=ris_pixels)
    assert walked > 0 and groups == 1
    assert zeroed > 0                                        # (flip and collapse leave samples that face away or have no pdf)


# ---- (b) orbiting camera: two pixels read one slot -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,reuse", [("cornell", 3), ("cornell", 1), ("many", 3), ("many", 1)])
def test_edits_with_an_orbiting_camera(hip, name, reuse):
    """The edits of the still camera, every kind: two pixels read one history slot, and the kernel's own planes keep them apart."""
    walked, zeroed, groups = run_edits(hip, name, reuse, orbit=True)
    assert walked > 0 and zeroed > 0 and 1 < groups <= lr.MAX_GROUPS


# ---- (c) identities, GPU against GPU ---------------------------------------------------------------------------------------------------
def state(r):
    return dict(image=r.image.cpu().numpy(), rays=r.rays, last=r.restir.download(1), temp=r.restir.download(2), ids=r.restir.download_light_ids(1))


def test_without_an_emitter_edit_it_is_tracking(hip):
    """Emission edits, and geometry edits that name no emitter: retargeting equals tracking (mode 1) bit for bit and launches no kernel."""
    sd = scene_data("many")
    a = HipRenderer(hip, sd, W, H, track=True)
    b = HipRenderer(hip, sd, W, H)
    b.restir.set_light_retargeting(True)
    assert b.restir.get_light_retargeting() and not a.restir.get_light_retargeting()
    ea, eb = EmissionEdits(sd, 4), EmissionEdits(sd, 4)
    v = sd.vertices.reshape(-1, 3, 3).copy()
    for f in range(8):
        if f in (2, 3, 6):
            a.set_emission(*ea.next()); b.set_emission(*eb.next())
        if f in (4, 6):
            ids, tv, tn = geometry_edit(sd, v, "one", seed=f)
            a.scene.set_geometry(ids, tv, tn); b.scene.set_geometry(ids, tv, tn)
            v[ids] = np.asarray(tv).reshape(-1, 3, 3)
        a.frame(3); b.frame(3)
        assert_same(state(a), state(b), f)
        assert b.restir.retarget_stats() == (0, 0, 0) and not b.restir.retarget_launched()
        assert np.array_equal(b.restir.download_light_samples(1)["light"], a.restir.download_light_ids(1))
    assert b.scene.light_moves() == 0 and len(b.scene.debug_table("lightMoved")) == 0


def edited_run(hip, name, frames, sync=True, bands=None):
    """`frames` frames of retargeting with an emitter edit before every frame from the third on; the state after each frame."""
    sd = scene_data(name)
    kinds = kinds_of(name)
    r = HipRenderer(hip, sd, W, H)
    r.restir.set_light_retargeting(True)
    v = sd.vertices.reshape(-1, 3, 3).copy()
    import torch
    images, out = [torch.zeros((W * H, 3), dtype=torch.float32, device="cuda") for _ in range(0 if sync else frames)], []
    hip.set_sync(sync)
    for f in range(frames):
        if f >= 2:
            ids, ev, en = emitter_edit(sd, v, kinds[(f - 2) % len(kinds)], seed=f)
            r.scene.set_geometry(ids, ev, en)
            v[ids] = np.asarray(ev).reshape(-1, 3, 3)
        if not sync:                                         # no wait between the frames: each image is copied in the library stream's order
            r.gbuf.render(r.scene, r.cam)
            r.restir.direct(r.scene, r.cam, r.gbuf, r.image.data_ptr(), 0, r.looper, 3)
            r.looper += 1
            r.gbuf.update(r.cam)
            hip.hip_memcpy_d2d_async(images[f].data_ptr(), r.image.data_ptr(), W * H * 12)
        elif bands is None:
            r.frame(3)
        else:
            r.gbuf.render(r.scene, r.cam)
            for y0, y1 in bands:
                r.restir.phase_a(r.scene, r.cam, r.gbuf, r.looper, 3, y0, y1)
            for y0, y1 in bands:
                r.restir.phase_b(r.scene, r.cam, r.gbuf, r.image.data_ptr(), 0, 3, y0, y1)
            r.restir.end_frame()
            r.rays = r.restir.ray_count()                # (of the last phase-A call: not compared)
            r.looper += 1
            r.gbuf.update(r.cam)
        if sync:
            d = state(r)
            d.pop("rays")
            d["stats"] = np.array(r.restir.retarget_stats())
            out.append(d)
    if not sync:
        hip.synchronize()
        hip.set_sync(True)
        r.rays = r.restir.ray_count()
        return [i.cpu().numpy() for i in images], state(r)
    return out


def test_row_bands_equal_the_full_frame(hip):
    full = edited_run(hip, "cornell", 6)
    banded = edited_run(hip, "cornell", 6, bands=((0, 17), (17, H)))
    for f, (a, b) in enumerate(zip(full, banded)):
        assert_same(a, b, f)
    assert full[-1]["stats"][0] > 0


def test_frames_in_flight_equal_synchronous(hip):
    """rs_set_sync(0): an edit before every frame, no wait in between (three frames' chains in flight); every image and the final state."""
    ref = edited_run(hip, "many", 9)
    images, last = edited_run(hip, "many", 9, sync=False)
    for f, (a, b) in enumerate(zip(ref, images)):
        assert bits_equal(a["image"], b), f
    last.pop("rays")
    ref[-1].pop("stats")
    assert_same(ref[-1], last, "final")


@pytest.mark.parametrize("name,size", [("cornell", (9, 5)), ("single", (W, H))])
def test_a_tiny_image_and_a_single_light(hip, name, size):
    walked, _, _ = run_edits(hip, name, 3, size=size)
    assert name != "single" or walked > 0


def test_moved_at_on_the_device(hip):
    """RS_TABLE_LIGHT_MOVED and rs_scene_light_moves after every edit of a sequence, against the restatement."""
    sd = scene_data("many")
    pair = lr.Pair(hip, "many", 16, 8)
    assert len(pair.h.r.scene.debug_table("lightMoved")) == 0
    for kind in kinds_of("many"):
        pair.edit(*emitter_edit(sd, pair.o.r.scene.vertices, kind, seed=13))
        assert pair.h.r.scene.light_moves() == pair.moved.moves
        assert np.array_equal(pair.h.r.scene.debug_table("lightMoved"), pair.moved.stamp)
    ids, v, n = geometry_edit(sd, pair.o.r.scene.vertices, "one", seed=2)
    pair.h.r.scene.set_geometry(ids, v, n)
    assert pair.h.r.scene.light_moves() == pair.moved.moves
    assert np.array_equal(pair.h.r.scene.debug_table("lightMoved"), pair.moved.stamp)


def test_the_records_are_the_winners_samples(hip):
    """Without temporal reuse a reservoir holds its RIS winner: its record's (u, v) on the light records gives the reservoir's Li, wi and
    dist from the frame's surface, and the record's pdf -- the restated sampler against what the RIS forms stored."""
    for ris_pixels in (GLOBAL_TABLE, 0):
        hip.set_ris_table_pixels(ris_pixels)
        pair = lr.Pair(hip, "many", W, H)
        pair.h.r.frame(2)
        rec = pair.h.r.restir.download_light_samples(1)
        resv = pair.h.r.restir.download(1)
        pos_tag, normal, _ = pair.h.r.restir.surface()
        px = np.nonzero(rec["light"] >= 0)[0]
        assert len(px) > W * H // 4
        Li, wi, dist, pdf = lr.light_sample_at(lr.light_records(pair.o.r.scene), rec["light"][px], rec["u"][px], rec["v"][px], pos_tag[px, :3])
        assert bits_equal(Li, resv["Li"][px]) and bits_equal(wi, resv["wi"][px]) and bits_equal(dist, resv["dist"][px]) and bits_equal(pdf, rec["pdf"][px])
        assert np.array_equal(rec["light"], pair.h.r.restir.download_light_ids(1))


# ---- (d) behaviour ---------------------------------------------------------------------------------------------------------------------
def test_the_first_frame_after_a_move_is_closer_to_the_new_pose(hip):
    """cornell 64x48, 10 warm frames, the lamp moved by (0.5, -0.05, 0.3) (kept inside the root box); reference: the mean of frames 6..15
    of a fresh history at the new pose; the error is the mean absolute luminance error of the first frame after the move.  (The figures
    measured on an MI355X: DESIGN.md section 3.)"""
    sd = scene_data("cornell")
    w, h = 64, 48
    orig = sd.vertices.reshape(-1, 3, 3)
    lo, hi = root_box(orig)
    lamp = lamp_of(sd, int(emitters(sd)[0]))
    moved = np.clip(orig[lamp] + np.array([0.5, -0.05, 0.3], np.float32), lo, hi).astype(np.float32)
    assert not np.array_equal(moved, orig[lamp])

    def lum(img):
        return lr.luminance(np.asarray(img, np.float32))

    fresh = HipRenderer(hip, sd, w, h)
    fresh.scene.set_geometry(lamp, moved)
    frames = [fresh.frame(3).copy() for _ in range(17)]
    ref = np.mean([lum(f) for f in frames[6:16]], axis=0)
    floor = float(np.abs(lum(frames[16]) - ref).mean())
    err = {}
    for retarget in (False, True):
        r = HipRenderer(hip, sd, w, h)
        if retarget:
            r.restir.set_light_retargeting(True)
        for _ in range(10):
            r.frame(3)
        r.scene.set_geometry(lamp, moved)
        err[retarget] = float(np.abs(lum(r.frame(3)) - ref).mean())
        if retarget:
            assert r.restir.retarget_stats()[0] > 0
    print("first frame after the move: error without retargeting %.4f, with %.4f, noise floor %.4f" % (err[False], err[True], floor))
    assert err[True] < err[False]


# ---- (e) refusals and unknown records --------------------------------------------------------------------------------------------------
def test_refusals_and_unknown_records(hip):
    sd = scene_data("cornell")
    r = HipRenderer(hip, sd, W, H)
    n = W * H
    unknown = lr.no_records(n)

    def all_unknown(rec):                                    # (light -1; the other fields of an unknown record mean nothing)
        return bool((rec["light"] == -1).all())
    for which in range(3):
        assert np.array_equal(r.restir.download_light_samples(which), unknown)        # off: nothing known
    r.restir.set_light_retargeting(True)
    assert r.restir.get_light_retargeting()
    for which in range(3):
        assert all_unknown(r.restir.download_light_samples(which))        # switched on: every record unknown
    for _ in range(2):
        r.frame(3)
    assert (r.restir.download_light_samples(1)["light"] >= 0).any() and (r.restir.download_light_samples(2)["light"] >= 0).any()
    # the 4 B/px messages do not carry the records
    import torch
    buf = torch.zeros(W * 4, dtype=torch.int32, device="cuda")
    for call in (lambda: r.restir.light_rows_pack(1, 0, 4, buf.data_ptr()), lambda: r.restir.light_rows_unpack(1, 0, 4, buf.data_ptr())):
        with pytest.raises(hip.RestirHipError) as e:
            call()
        assert "error %d" % hip.RS_ERR_UNSUPPORTED in str(e.value)
    # an upload: unknown
    for which in (1, 2):
        r.restir.upload(which, r.restir.download(which))
        assert all_unknown(r.restir.download_light_samples(which))
        assert (r.restir.download_light_ids(which) == -1).all()
    # another scene: the history's and the published copy's records name other lights
    r.frame(3)
    assert (r.restir.download_light_samples(1)["light"] >= 0).any()
    other = HipRenderer(hip, scene_data("single"), W, H)
    r.restir.direct(other.scene, r.cam, r.gbuf, r.image.data_ptr(), 0, r.looper, 0)      # (reuse 0: nothing of the history is merged)
    now = r.restir.download_light_samples(0)                                            # the buffer the history was in: cleared, not rewritten
    assert all_unknown(now)
    # tracking off switches both off; on again starts unknown
    r.restir.set_light_tracking(False)
    assert not r.restir.get_light_retargeting()
    assert np.array_equal(r.restir.download_light_samples(1), unknown)
    r.restir.light_rows_bytes(4)
    r.restir.set_light_retargeting(True)
    assert all_unknown(r.restir.download_light_samples(1)) and (r.restir.download_light_ids(1) == -1).all()


def test_the_strip_driver_refuses_a_retargeted_restir(hip):
    """rs_strips_frame and rs_strips_exchange_history with Comm(0, 1): RS_ERR_UNSUPPORTED while retargeting is on, whatever the driver's
    tracking setting, and nothing of the reservoirs, the records or the image changes; after rs_restir_set_light_retargeting(r, 0) the
    tracked object is taken as before."""
    import torch
    sd = scene_data("cornell")
    w, h = 64, 48
    r = HipRenderer(hip, sd, w, h)
    r.restir.set_light_retargeting(True)
    for _ in range(2):
        r.frame(3)
    comm = hip.Comm(0, 1, lambda *a: None, lambda *a: None)
    drv = hip.Strips(comm, w, h)
    img = torch.full((w * h, 3), 7.0, dtype=torch.float32, device="cuda")
    try:
        before = (r.restir.download(0), r.restir.download(1), r.restir.download(2), r.restir.download_light_samples(1), r.restir.download_light_ids(1))
        for tracking in (False, True):
            drv.set_light_tracking(tracking)
            for call in (lambda: drv.frame(r.restir, r.scene, r.cam, r.gbuf, img.data_ptr(), 0, r.looper, 3), lambda: drv.exchange_history(r.restir, r.gbuf)):
                with pytest.raises(hip.RestirHipError) as e:
                    call()
                assert "error %d" % hip.RS_ERR_UNSUPPORTED in str(e.value) and "retargeting" in str(e.value)
        hip.synchronize()
        after = (r.restir.download(0), r.restir.download(1), r.restir.download(2), r.restir.download_light_samples(1), r.restir.download_light_ids(1))
        for a, b in zip(before, after):
            assert a.tobytes() == b.tobytes()
        assert float((img - 7.0).abs().sum()) == 0.0 and r.restir.get_light_retargeting()
        r.restir.set_light_retargeting(False)                # tracking stays on: the driver, told so, takes the object
        drv.frame(r.restir, r.scene, r.cam, r.gbuf, img.data_ptr(), 0, r.looper, 3)
        hip.synchronize()
        assert float((img - 7.0).abs().sum()) > 0.0
    finally:
        drv.destroy(); comm.destroy()


def test_switching_on_over_a_tracked_history(hip):
    """Tracking on with history and an emitter edit already made, then retargeting on: every id and record is unknown at once, and the
    edit made before the switch is taken as seen -- the next frame launches no kernel; an edit after it does."""
    sd = scene_data("cornell")
    r = HipRenderer(hip, sd, W, H, track=True)
    for _ in range(2):
        r.frame(3)
    r.scene.set_geometry(*emitter_edit(sd, sd.vertices, "one", seed=13))
    assert (r.restir.download_light_ids(1) >= 0).any() and r.scene.light_moves() == 1
    r.restir.set_light_retargeting(True)
    for which in range(3):
        assert (r.restir.download_light_ids(which) == -1).all() and (r.restir.download_light_samples(which)["light"] == -1).all()
    r.frame(3)
    assert not r.restir.retarget_launched()
    r.frame(3)
    assert not r.restir.retarget_launched()
    v = sd.vertices.reshape(-1, 3, 3).copy()
    ids, ev, _ = emitter_edit(sd, v, "one", seed=13)
    v[ids] = np.asarray(ev).reshape(-1, 3, 3)
    r.scene.set_geometry(*emitter_edit(sd, v, "all", seed=13))
    r.frame(3)
    assert r.restir.retarget_launched() and r.restir.retarget_stats()[0] > 0
