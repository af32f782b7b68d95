"""Light tracking (rs_restir_set_light_tracking) on row strips: the row packing of the id planes, strips driven by hand, the strip
driver with rs_strips_set_light_tracking over three ranks on one GPU, and the setting's contract on one rank.  The CPU form of the
decomposition, with its control, is tests/test_tiling_light_tracking.py."""
import os
import subprocess

import numpy as np
import pytest

from oracle import binding as ob
from tests import strips_tracking_cases as cases
from tests.common import EmissionEdits, HipRenderer, OracleRenderer, bits_equal, get_scene, hip_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


@pytest.fixture(scope="module")
def packing_pair(hip):
    """70 x 40: a tracked renderer two frames in, so that the three id planes hold three different sets of ids (which 0: the frame
    before last, 1: the last frame, 2: the published copy), and what its planes hold.  Computed once and left unchanged."""
    W, H = 70, 40
    a = HipRenderer(hip, get_scene("cornell"), W, H, track=True)
    for _ in range(2):
        a.frame(3)
    want = [a.light_ids(which) for which in range(3)]
    assert all((w >= 0).any() for w in want) and not np.array_equal(want[0], want[1])
    return W, H, a, want


# y0 = 3 puts the rows at a byte offset of the plane that is no multiple of 16, and with 5 rows the size is none either (70 * 5 ints):
# the copy kernel moves ints.  Rows 4..12 start and end on 16 bytes: it moves 16 bytes a thread.
@pytest.mark.parametrize("y0,rows", [(3, 5), (3, 8), (4, 8)])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_light_rows_pack_unpack(hip, packing_pair, which, y0, rows):
    import torch
    W, H, a, want = packing_pair
    assert a.restir.light_rows_bytes(rows) == W * rows * 4
    b = hip.ReSTIR(W, H)
    b.set_light_tracking(True)                                       # every id unknown
    buf = torch.zeros(W * rows * 4, dtype=torch.uint8, device="cuda")
    a.restir.light_rows_pack(which, y0, rows, buf.data_ptr())
    b.light_rows_unpack(which, y0, rows, buf.data_ptr())
    hip.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.int32), want[which][y0 * W:(y0 + rows) * W])
    for other in range(3):
        got = b.download_light_ids(other)
        expect = np.full(W * H, -1, np.int32)
        if other == which:
            expect[y0 * W:(y0 + rows) * W] = want[which][y0 * W:(y0 + rows) * W]
        assert np.array_equal(got, expect), (which, other)
    assert all(np.array_equal(a.light_ids(k), want[k]) for k in range(3))     # packing reads only
    b.destroy()


def test_light_rows_refusals(hip, packing_pair):
    import torch
    W, H, a, want = packing_pair
    buf = torch.zeros(W * H * 4 + 4, dtype=torch.uint8, device="cuda")
    bad = [(0, -1, 2), (0, 0, -1), (0, H - 1, 2), (0, H, 1), (3, 0, 1), (-1, 0, 1)]
    for which, y0, rows in bad:
        with pytest.raises(hip.RestirHipError, match="10001"):
            a.restir.light_rows_pack(which, y0, rows, buf.data_ptr())
        with pytest.raises(hip.RestirHipError, match="10001"):
            a.restir.light_rows_unpack(which, y0, rows, buf.data_ptr())
    with pytest.raises(hip.RestirHipError, match="10001"):
        a.restir.light_rows_pack(1, 0, 1, buf.data_ptr() + 1)       # the copy kernel moves ints
    with pytest.raises(hip.RestirHipError, match="10001"):
        a.restir.light_rows_pack(1, 0, 1, 0)
    off = hip.ReSTIR(W, H)                                          # tracking off: there are no planes
    for fn in (off.light_rows_pack, off.light_rows_unpack):
        with pytest.raises(hip.RestirHipError, match="10001"):
            fn(1, 0, 4, buf.data_ptr())
    off.set_light_tracking(True)
    off.light_rows_pack(1, 0, 4, buf.data_ptr())
    off.set_light_tracking(False)                                   # switched off again: refused again
    with pytest.raises(hip.RestirHipError, match="10001"):
        off.light_rows_pack(1, 0, 4, buf.data_ptr())
    a.restir.light_rows_pack(1, 0, 0, buf.data_ptr())               # no rows: accepted, nothing moves
    a.restir.light_rows_pack(1, H, 0, buf.data_ptr())
    hip.synchronize()
    assert all(np.array_equal(a.light_ids(k), want[k]) for k in range(3))
    off.destroy()


@pytest.mark.parametrize("name", ["cornell", "sponza:0.02"])
def test_tracked_strips_by_hand_equal_full_frame_and_oracle(hip, name):
    """Three tracked rank objects on one GPU on the CPU test's strips, edits and camera; the history goes through
    HipBackend(track=True).history_pack / _unpack.  Image, history reservoirs and their light ids of every rank equal the tracked full
    frame of the library AND the tracked oracle, bit for bit."""
    from restir_amd.tiling import HipBackend
    sd = get_scene(name)
    W, H = cases.W, cases.H
    ob.set_libm_mode(1)                                             # the oracle's cos / sin correctly rounded, as the device evaluates them
    try:
        oracle = OracleRenderer(sd, W, H, track=True)
        full = HipRenderer(hip, sd, W, H, track=True)
        ranks = []
        for _ in cases.BOUNDS:
            scene = hip_scene(hip, sd)
            scene.set_sample_sequence(None)
            ranks.append(HipBackend(hip, scene, hip.camera_update(sd.camera(W, H)), W, H, track=True))
        assert ranks[0].history_bytes(3) == W * 3 * 64
        for frame, edit in enumerate(cases.edits(sd)):
            pos = cases.camera_position(sd, frame)
            oracle.set_camera_position(pos); full.set_camera_position(pos)
            for b in ranks:
                for i in range(3):
                    b.cam.position[i] = float(pos[i])
                hip.camera_update(b.cam)
            if edit is not None:
                oracle.set_emission(*edit); full.set_emission(*edit)
                for b in ranks:
                    b.scene.set_emission(*edit)
            want = oracle.frame(cases.REUSE)
            ref = full.frame(cases.REUSE)
            cases.strips_frame(ranks, looper=frame)
            cases.exchange_history(ranks, lambda b, y0, rows: b.history_pack(y0, rows), lambda b, y0, rows, msg: b.history_unpack(y0, rows, msg))
            hip.synchronize()
            got = np.concatenate([b.image.cpu().numpy()[y0 * W:y1 * W] for b, (y0, y1) in zip(ranks, cases.BOUNDS)])
            assert bits_equal(ref, got) and bits_equal(want, got), frame
            ref_resv, ref_ids = full.restir.download(1), full.light_ids(1)
            assert cases.same_resv(oracle.restir.last, ref_resv) and np.array_equal(oracle.light_ids(1), ref_ids), frame
            for k, b in enumerate(ranks):                           # every row of the history, on every rank
                assert cases.same_resv(ref_resv, b.restir.download(1)), (frame, k)
                assert np.array_equal(ref_ids, b.restir.download_light_ids(1)), (frame, k)
        assert float(np.abs(ref).sum()) > 0 and (ref_ids >= 0).any()
    finally:
        ob.set_libm_mode(0)


def test_strip_driver_with_light_tracking_three_ranks_on_one_gpu():
    """restir_amd/host/strips_tracking_ranks.cpp: three tracked ranks as threads on this GPU over the stream-ordered loopback transport,
    rs_strips_set_light_tracking(strips, 1), the lamps edited before every frame: gathered radiance, and after rs_strips_exchange_history
    every rank's history reservoirs and light ids, equal rank 0's tracked full frame -- still and vertically moving camera at 96 x 96, and
    the moving camera at 70 x 99, where 33 rows of 70 pixels put no plane on 16 bytes and the eight-plane launches move ints."""
    exe = os.path.join(ROOT, "restir_amd", "host", "strips_tracking_ranks")
    assert os.path.exists(exe), "restir_amd/host/strips_tracking_ranks is built by restir_amd/csrc/Makefile"
    r = subprocess.run([exe, "60"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "strips_tracking_ranks ok (3 ranks)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("== full frame over 6 frames: True") == 3, r.stdout[-3000:]


def test_light_tracking_setting_on_one_rank(hip):
    """The contract of rs_strips_set_light_tracking with Comm(0, 1): on, a tracked frame sequence with an edit between the frames equals
    tracked rs_restir_direct on a second object bit for bit and an untracked object is refused (10001: the message sizes would
    disagree); off, everything is as before -- a tracked object refused with 10002, an untracked one rendered."""
    import torch
    sd = get_scene("cornell")
    W, H = 64, 48
    scene = hip_scene(hip, sd)
    cam = hip.camera_update(sd.camera(W, H))
    comm = hip.Comm(0, 1, lambda *a: None, lambda *a: None)
    drv = hip.Strips(comm, W, H)
    g = [hip.GBuffer(W, H) for _ in range(2)]
    r = [hip.ReSTIR(W, H) for _ in range(2)]
    for x in r:
        x.set_light_tracking(True)
    plain = hip.ReSTIR(W, H)
    img = [torch.zeros((W * H, 3), dtype=torch.float32, device="cuda") for _ in range(2)]
    edits = EmissionEdits(sd, 3)
    try:
        with pytest.raises(hip.RestirHipError, match="10002"):      # the default
            drv.frame(r[0], scene, cam, g[0], img[0].data_ptr(), 0, 0, 3)
        drv.set_light_tracking(True)
        for frame in range(4):
            if frame:
                scene.set_emission(*edits.next())
            drv.frame(r[0], scene, cam, g[0], img[0].data_ptr(), 0, frame, 3)
            g[0].update(cam)
            drv.exchange_history(r[0], g[0])                        # one rank: nothing travels
            g[1].render(scene, cam)
            r[1].direct(scene, cam, g[1], img[1].data_ptr(), 0, frame, 3)
            g[1].update(cam)
            hip.synchronize()
            assert bits_equal(img[0].cpu().numpy(), img[1].cpu().numpy()), frame
            assert cases.same_resv(r[0].download(1), r[1].download(1)), frame
            assert np.array_equal(r[0].download_light_ids(1), r[1].download_light_ids(1)), frame
        assert (r[0].download_light_ids(1) >= 0).any() and float(img[0].abs().sum()) > 0
        with pytest.raises(hip.RestirHipError, match="10001"):
            drv.frame(plain, scene, cam, g[0], img[0].data_ptr(), 0, 0, 3)
        with pytest.raises(hip.RestirHipError, match="10001"):
            drv.exchange_history(plain, g[0])
        drv.set_light_tracking(False)                               # as before the setting existed
        with pytest.raises(hip.RestirHipError, match="10002"):
            drv.frame(r[0], scene, cam, g[0], img[0].data_ptr(), 0, 0, 3)
        with pytest.raises(hip.RestirHipError, match="10002"):
            drv.exchange_history(r[0], g[0])
        drv.frame(plain, scene, cam, g[0], img[0].data_ptr(), 0, 0, 3)
        drv.exchange_history(plain, g[0])
        hip.synchronize()
        assert (plain.download_light_ids(1) == -1).all()
    finally:
        drv.destroy(); comm.destroy()


def test_light_tracking_setting_is_refused_while_a_gather_is_in_flight(hip):
    """Between frames only: the setting is the size of the next history messages."""
    import torch
    noop = lambda p, n, peer: None
    comm = hip.Comm(0, 2, noop, noop, None, None, stream_ordered=True)
    drv = hip.Strips(comm, 64, 48)
    image = torch.zeros((64 * 48, 4), dtype=torch.uint8, device="cuda")
    try:
        drv.gather_begin(image.data_ptr(), 4, 0, 0)
        with pytest.raises(hip.RestirHipError, match="10001"):
            drv.set_light_tracking(True)
        drv.gather_end(0)
        drv.set_light_tracking(True)
        drv.set_light_tracking(False)
    finally:
        drv.destroy(); comm.destroy()
