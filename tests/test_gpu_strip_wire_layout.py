"""What the strip driver puts on the wire, held to the public packing functions (include/restir_hip.h).

A message of the driver is documented as a concatenation of public packs: the border rows of a frame as rs_restir_halo_pack followed by
rs_gbuffer_rows_pack, a history message as rs_restir_rows_pack, rs_gbuffer_rows_pack and (with light tracking) rs_restir_light_rows_pack,
the G-buffer rows of a filter as rs_gbuffer_rows_pack.  Two ranks agree about a message's bytes only if that holds, so every case here
drives rank 0 of a world of 2 over a host-side transport (capi.Comm with Python callbacks, stream_ordered=False: the driver has
synchronised before a callback runs) and compares bit for bit: what the driver hands to send with the public packs of the rows it sent,
and the public packs of the rows it received with what recv was given.

recv is given a DONOR's bytes: a second renderer of the same size one frame further on, packed through the public functions -- ids and
light indices that later kernels may dereference, never random bytes.  Frames of 64 x 80 and 61 x 80 with bounds [0, 40, 80]: 40 rows
is the least the 32 rows an EAW level reaches (and the 33 of the SVGF strip filter) allow.  At width 64 every plane of every message
lies on 16 bytes and the copy kernel moves 16 bytes a thread; at width 61 the 5-row G-buffer planes of a frame's border rows are no
multiple of 16 bytes and it moves ints."""
import numpy as np
import pytest

from tests.common import HipRenderer, get_scene, hip_scene

pytestmark = pytest.mark.gpu

H, BOUNDS = 80, [0, 40, 80]
Y1 = BOUNDS[1]
HALO, EAW_REACH = 5, 32


@pytest.fixture(scope="module")
def capi(hip):
    hip.set_sync(True)
    yield hip
    hip.set_sync(True)


def pack(nbytes, fn, *args):
    """The bytes a public pack function writes, as a uint8 tensor on the device."""
    import torch
    buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    fn(*args, buf.data_ptr())
    return buf


def halo_message(r, y_resv, y_g, g_rows):
    """rs_restir_halo_pack of 5 rows followed by rs_gbuffer_rows_pack of g_rows rows of the current planes."""
    import torch
    return torch.cat([pack(r.restir.halo_bytes(HALO), r.restir.halo_pack, y_resv, HALO),
                      pack(r.gbuf.rows_bytes(g_rows), r.gbuf.rows_pack, 0, y_g, g_rows)])


def history_message(r, y, rows, track):
    """rs_restir_rows_pack(1), rs_gbuffer_rows_pack(1) and, tracked, rs_restir_light_rows_pack(1) of rows [y, y + rows)."""
    import torch
    parts = [pack(r.restir.rows_bytes(1, rows), r.restir.rows_pack, 1, y, rows),
             pack(r.gbuf.rows_bytes(rows), r.gbuf.rows_pack, 1, y, rows)]
    if track:
        parts.append(pack(r.restir.light_rows_bytes(rows), r.restir.light_rows_pack, 1, y, rows))
    return torch.cat(parts)


_donors = {}


def donor(capi, W):
    """Per width, computed once and left unchanged: a tracked renderer's second frame as the strip below would send it.  Before that
    frame's rs_gbuffer_update: its border rows for both G-buffer reaches, the G-buffer rows of a filter and its image; after the update:
    its history message (the untracked one is the tracked one without the trailing id rows)."""
    if W not in _donors:
        d = HipRenderer(capi, get_scene("cornell"), W, H, track=True)
        d.frame(3)
        d.gbuf.render(d.scene, d.cam)
        d.restir.direct(d.scene, d.cam, d.gbuf, d.image.data_ptr(), 0, d.looper, 3)
        out = {"scene": d.scene, "renderer": d}
        out["halo"] = {g: halo_message(d, Y1, Y1, g) for g in (HALO, EAW_REACH)}
        out["gbuffer"] = pack(d.gbuf.rows_bytes(EAW_REACH), d.gbuf.rows_pack, 0, Y1, EAW_REACH)
        out["image"] = d.image.clone()
        d.gbuf.update(d.cam)
        out["history"] = history_message(d, Y1, H - Y1, True)
        capi.synchronize()
        assert all(int(out[k].count_nonzero()) > 0 for k in ("gbuffer", "history")) and float(out["image"].abs().sum()) > 0
        _donors[W] = out
    return _donors[W]


class Wire:
    """The host-side transport of rank 0: keeps what send is handed, answers recv number k of the case with reply(k, nbytes)."""

    def __init__(self, capi, reply):
        self.capi, self.reply = capi, reply
        self.sent, self.received, self.groups = [], [], 0
        self.comm = capi.Comm(0, 2, self.send, self.recv, self.begin, None, stream_ordered=False)

    def begin(self):
        self.groups += 1

    def send(self, ptr, nbytes, peer):
        import torch
        t = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        self.capi.hip_memcpy_d2d(t.data_ptr(), ptr, nbytes)
        self.sent.append((self.groups, peer, t))

    def recv(self, ptr, nbytes, peer):
        t = self.reply(len(self.received), nbytes)
        assert t.numel() == nbytes and t.element_size() == 1, (len(self.received), nbytes, t.numel())
        self.capi.hip_memcpy_d2d(ptr, t.data_ptr(), nbytes)
        self.received.append((self.groups, peer, nbytes))


def same(a, b):
    return a.numel() == b.numel() and bool((a == b).all())


@pytest.mark.parametrize("g_reach", [HALO, EAW_REACH])
@pytest.mark.parametrize("W", [64, 61])
def test_frame_border_rows_are_the_public_packs(capi, W, g_reach):
    """rs_strips_frame, reuse = 3: one group, one message each way of rs_restir_halo_bytes(5) + rs_gbuffer_rows_bytes(g_reach) bytes."""
    don = donor(capi, W)
    a = HipRenderer(capi, get_scene("cornell"), W, H, scene=don["scene"])
    wire = Wire(capi, lambda k, n: don["halo"][g_reach])
    drv = capi.Strips(wire.comm, W, H, BOUNDS)
    try:
        drv.set_gbuffer_halo(g_reach)
        drv.frame(a.restir, a.scene, a.cam, a.gbuf, a.image.data_ptr(), 0, 0, 3)
        capi.synchronize()
        size = a.restir.halo_bytes(HALO) + a.gbuf.rows_bytes(g_reach)
        assert size == W * (HALO * 48 + g_reach * 20)               # the documented 48 and 20 B/px
        assert [(g, p, t.numel()) for g, p, t in wire.sent] == [(1, 1, size)] and wire.received == [(1, 1, size)]
        assert same(wire.sent[0][2], halo_message(a, Y1 - HALO, Y1 - g_reach, g_reach))
        assert same(halo_message(a, Y1, Y1, g_reach), don["halo"][g_reach])
        assert float(a.image[:Y1 * W].abs().sum()) > 0
    finally:
        drv.destroy(); wire.comm.destroy()


@pytest.mark.parametrize("W", [64, 61])
def test_history_messages_are_the_public_packs(capi, W):
    """rs_strips_exchange_history, untracked and tracked: the rows [0, 40) of this rank travel, the donor's rows [40, 80) arrive; the
    untracked message is the tracked one without its trailing id rows."""
    don = donor(capi, W)
    rows = H - Y1
    sent = {}
    for track in (False, True):
        a = HipRenderer(capi, get_scene("cornell"), W, H, scene=don["scene"], track=track)
        untracked = a.restir.rows_bytes(1, rows) + a.gbuf.rows_bytes(rows)
        size = untracked + (a.restir.light_rows_bytes(rows) if track else 0)
        wire = Wire(capi, lambda k, n: don["history"][:n])
        drv = capi.Strips(wire.comm, W, H, BOUNDS)
        try:
            drv.set_light_tracking(track)
            drv.frame(a.restir, a.scene, a.cam, a.gbuf, a.image.data_ptr(), 0, 0, 1)     # temporal reuse only: no border rows travel
            a.gbuf.update(a.cam)
            assert wire.groups == 0
            drv.exchange_history(a.restir, a.gbuf)
            capi.synchronize()
            assert untracked == W * rows * 60 and size == untracked + (W * rows * 4 if track else 0)      # the documented 40 + 20 (+ 4) B/px
            assert [(g, p, t.numel()) for g, p, t in wire.sent] == [(1, 1, size)] and wire.received == [(1, 1, size)]
            sent[track] = wire.sent[0][2]
            assert same(sent[track], history_message(a, 0, Y1, track))
            assert same(history_message(a, Y1, rows, track), don["history"][:size])
            assert int(sent[track].count_nonzero()) > 0
            if track:
                assert (a.restir.download_light_ids(1)[:Y1 * W] >= 0).any()
        finally:
            drv.destroy(); wire.comm.destroy()
    # the same layout up to where the untracked message ends: the tracked message's first bytes are the two untracked packs of its own rows
    assert sent[True].numel() == sent[False].numel() + W * Y1 * 4
    assert same(sent[True][:sent[False].numel()], history_message(a, 0, Y1, False))


@pytest.mark.parametrize("W", [64, 61])
def test_eaw_gbuffer_rows_are_the_public_pack(capi, W):
    """rs_strips_eaw_filter at the default G-buffer halo of 5: the filter exchanges its 32 G-buffer rows itself, in its first group; the
    five groups after it swap the rows of the levels' inputs, from and into place."""
    import torch
    don = donor(capi, W)
    a = HipRenderer(capi, get_scene("cornell"), W, H, scene=don["scene"])
    image = don["image"].view(H, W * 3)

    def reply(k, n):
        if k == 0:
            return don["halo"][HALO]
        if k == 1:
            return don["gbuffer"]
        level_rows = n // (W * 12)                                  # the rows of a level's input below the strip: the donor's image there
        return image[Y1:Y1 + level_rows].contiguous().view(-1).view(dtype=torch.uint8)

    wire = Wire(capi, reply)
    drv = capi.Strips(wire.comm, W, H, BOUNDS)
    eaw = capi.EAWFilter(W, H)
    try:
        drv.frame(a.restir, a.scene, a.cam, a.gbuf, a.image.data_ptr(), 0, 0, 3)
        drv.eaw_filter(eaw, a.gbuf, a.cam, a.image.data_ptr())
        capi.synchronize()
        g_bytes = a.gbuf.rows_bytes(EAW_REACH)
        assert g_bytes == W * EAW_REACH * 20
        assert [(g, p, t.numel()) for g, p, t in wire.sent] == [(1, 1, W * HALO * 68), (2, 1, g_bytes)] + [(3 + l, 1, (2 << l) * W * 12) for l in range(5)]
        assert [(g, n) for g, p, n in wire.received] == [(g, t.numel()) for g, p, t in wire.sent]
        assert same(wire.sent[1][2], pack(g_bytes, a.gbuf.rows_pack, 0, Y1 - EAW_REACH, EAW_REACH))
        assert same(pack(g_bytes, a.gbuf.rows_pack, 0, Y1, EAW_REACH), don["gbuffer"])
    finally:
        eaw.destroy(); drv.destroy(); wire.comm.destroy()
