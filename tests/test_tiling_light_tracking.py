"""CPU: light tracking (rs_restir_set_light_tracking) on row strips, emulated with the oracle in one process.  Three tracked ranks
on uneven strips, lamps edited every frame, a camera that moves vertically: image, history reservoirs and their light ids equal the
tracked full frame bit for bit when the history exchange carries the id rows of the reservoirs it carries -- and differ when it does
not (the control: without it the test could pass with an exchange that forgets the ids).  The per-frame halo carries no ids."""
import numpy as np
import pytest
import torch

from oracle import binding as ob
from tests import strips_tracking_cases as cases
from tests.common import OracleBackend, OracleRenderer, bits_equal, get_scene, oracle_scene


def id_rows(b, y0, rows):
    return torch.from_numpy(b.restir.ids_last[y0 * b.W:(y0 + rows) * b.W].copy().view(np.uint8))


def pack_with_ids(b, y0, rows):
    return torch.cat([b.history_pack(y0, rows), id_rows(b, y0, rows)])           # the id rows last: the untracked message is a prefix


def unpack_with_ids(b, y0, rows, msg):
    n = b.history_bytes(rows)
    b.history_unpack(y0, rows, msg[:n])
    b.restir.ids_last[y0 * b.W:(y0 + rows) * b.W] = msg[n:].numpy().view(np.int32)


def unpack_without_ids(b, y0, rows, msg):
    b.history_unpack(y0, rows, msg[:b.history_bytes(rows)])


def run(name, with_ids):
    """Returns per frame whether (image, `last` reservoirs, light_ids(1)) of every rank equal the tracked full frame's."""
    sd = get_scene(name)
    full = OracleRenderer(sd, cases.W, cases.H, track=True)
    ranks = []
    for _ in cases.BOUNDS:
        b = OracleBackend(oracle_scene(sd), ob.camera_update(sd.camera(cases.W, cases.H)), cases.W, cases.H)
        b.scene.set_sample_sequence(None)
        b.restir.set_light_tracking(True)
        ranks.append(b)
    equal = []
    for frame, edit in enumerate(cases.edits(sd)):
        pos = cases.camera_position(sd, frame)
        full.set_camera_position(pos)
        for b in ranks:
            for i in range(3):
                b.cam.position[i] = float(pos[i])
            ob.camera_update(b.cam)
        if edit is not None:
            full.set_emission(*edit)
            for b in ranks:
                b.scene.set_emission(*edit)
        ref = full.frame(cases.REUSE).copy()
        cases.strips_frame(ranks, looper=frame)
        cases.exchange_history(ranks, pack_with_ids, unpack_with_ids if with_ids else unpack_without_ids)
        got = np.concatenate([b.image[y0 * cases.W:y1 * cases.W] for b, (y0, y1) in zip(ranks, cases.BOUNDS)])
        # after the exchange EVERY row of the history is the full frame's, on every rank
        equal.append((bits_equal(ref, got), all(cases.same_resv(full.restir.last, b.restir.last) for b in ranks),
                      all(np.array_equal(full.light_ids(1), b.restir.light_ids(1)) for b in ranks)))
    assert float(np.abs(ref).sum()) > 0 and (full.light_ids(1) >= 0).any()
    return equal


@pytest.mark.parametrize("name", ["cornell", "sponza:0.02"])
def test_tracked_strips_equal_tracked_full_frame(name):
    assert run(name, True) == [(True, True, True)] * cases.FRAMES


@pytest.mark.parametrize("name", ["cornell", "sponza:0.02"])
def test_history_without_id_rows_differs(name):
    """The control.  Frame 0 has no history and no edit, so its image and reservoirs still agree; the ids a rank did not receive stay
    unknown.  From the first edit on a reprojection across a strip border meets a reservoir whose light the rank does not know and
    leaves it at last frame's emission: image, reservoirs and ids part in every later frame."""
    equal = run(name, False)
    assert equal[0] == (True, True, False), equal
    assert all(e == (False, False, False) for e in equal[1:]), equal
