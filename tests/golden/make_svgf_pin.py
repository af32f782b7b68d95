"""Writes tests/golden/svgf_oracle_default.npz: the oracle's SpatioTemporalFilter with the reference's default sigmas on a short rendered
sequence (Cornell box, 48 x 32, a static camera, 4 frames).  A regression pin of the oracle's own output: it was written before the
filter's sigmas became parameters (orc_svgf_set_params), and tests/test_denoise_reference.py holds the oracle to it bit for bit.

    python -m tests.golden.make_svgf_pin
"""
import os

import numpy as np

from oracle import binding as ob
from tests.common import OracleRenderer, get_scene

W, H, FRAMES = 48, 32, 4


def run():
    o = OracleRenderer(get_scene("cornell"), W, H)
    f = ob.SVGF(W, H)
    out = {}
    for frame in range(FRAMES):
        o.gbuf.render(o.scene, o.cam)
        o.restir.direct(o.scene, o.cam, o.gbuf, o.image, 0, o.looper, 0)
        o.looper += 1
        out[f"filtered{frame}"] = f.filter(o.image, o.gbuf, o.cam).copy()
        st = f.state()
        out[f"variance{frame}"] = st["variance"]
        out[f"moment{frame}"] = st["accum_moment"]
        f.next_frame()
        o.gbuf.update(o.cam)
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "svgf_oracle_default.npz"), **run())
