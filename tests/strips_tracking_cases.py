"""What the CPU and the GPU test of light tracking on row strips share (test_tiling_light_tracking.py, test_gpu_strips_light_tracking.py):
the frame, the strips, the camera path, the lamp edits, and the strip frame itself, driven by hand over backends with the interface
of restir_amd/tiling.py so that every rank runs in this process."""
import numpy as np

from restir_amd.tiling import HALO
from tests.common import EmissionEdits, bits_equal

W, H = 96, 64
BOUNDS = [(0, 8), (8, 45), (45, 64)]          # uneven strips, the first one barely taller than the halo
FRAMES = 5
REUSE = 3
EDIT_SEED = 7


def camera_position(sd, frame):
    """Vertical motion: the reprojected pixel of the temporal merge crosses strip borders, so the history exchange matters.  (An orbit
    in the horizontal plane reprojects along the rows and passes without the id rows.)"""
    base = np.asarray(sd.camera_args["position"], np.float64)
    return base + np.array([0.05 * frame, 0.25 * ((frame % 3) - 1), 0.0])


def same_resv(a, b):
    """Two arrays of reservoir records, every field bit for bit."""
    return all(bits_equal(a[k], b[k]) for k in ("Li", "wi", "dist", "weight")) and np.array_equal(a["numSamples"], b["numSamples"])


def edits(sd):
    """One edit per frame from frame 1 on: lamps recoloured, switched off and back on; the same for every replica of the scene."""
    e = EmissionEdits(sd, EDIT_SEED)
    return [None] + [e.next() for _ in range(FRAMES - 1)]


def strips_frame(backends, iteration=0, looper=0):
    """One frame of every rank up to GBuffer::update, the neighbours' 5 border rows handed over in between (tiling.StripRenderer's
    schedule without a process group).  The halo carries no light ids: the temporal pass reads the published copy's id only at its own
    pixels, and the spatial pass reads none."""
    for b, (y0, y1) in zip(backends, BOUNDS):
        b.gbuffer_render(y0, y1)
        b.phase_a(looper, REUSE, y0, y1)
    for k in range(len(backends) - 1):
        edge = BOUNDS[k][1]
        down = backends[k].halo_pack(edge - HALO, HALO)
        up = backends[k + 1].halo_pack(edge, HALO)
        backends[k + 1].halo_unpack(edge - HALO, HALO, down)
        backends[k].halo_unpack(edge, HALO, up)
    for b, (y0, y1) in zip(backends, BOUNDS):
        b.phase_b(iteration, REUSE, y0, y1)
        b.end_frame()


def exchange_history(backends, pack, unpack):
    """Every rank's rows to every other rank; pack(backend, y0, rows) -> message, unpack(backend, y0, rows, message)."""
    msgs = [pack(b, y0, y1 - y0) for b, (y0, y1) in zip(backends, BOUNDS)]
    for k, b in enumerate(backends):
        for j, (y0, y1) in enumerate(BOUNDS):
            if j != k:
                unpack(b, y0, y1 - y0, msgs[j])
