"""GPU: every render kernel at the material and light extremes of tests/extreme_cases.py, held to the CPU oracle bit for bit.

Every other parity module renders tame parameters; here the numbers in rs_material and the light powers leave that range: roughness 0,
1e-6 and 2, metallic 0, 1 and 2, base colours of 0, above 1 and with one zero channel, ior 0, 1 +- 1 ulp, 1e4 and negative, radiances of
0, a denormal, 1e-30, 1e25, 3e38 and with a negative channel, lights without area, a dark and a 1e30 light beside the ordinary one, a
1e19 emitter of area 5e-19, and 1228 lights spread over 1e-30 .. 1e25.  The roughness and radiance rows are where the guarded short forms
of restir_amd/csrc/rs_exact.h send a whole wave to the compiler's operator (one lane outside [2^-60, 2^60) is enough: alpha^2 = 1e-24 as
the numerator of gtr2, a radiance or pdf above 2^60 or below 2^-60 in the RIS weight quotient, whose `unused` lanes carry garbage that must
be discarded); the others are where the filters that decide whether a sample lives (is_nan_or_inf(weight) || pdf <= 0 in k_ris,
resv_invalid, ind_invalid, the GLM-shaped gmin / gmax) and the path tracer's throughput see NaN, infinity, zero and negative numbers.  The
base-colour rows reach no guarded form (k_ris shades with base colour 1, the path tracers divide with the plain operator): they drive
albedo and throughput.  Two mixed cases give only a part of the scene a material that leaves the guarded range, so that one 32 x 8 tile
and one wave hold both kinds of pixel (asserted on the oracle's G-buffer in tests/test_extreme_cases.py), and the 1e19 emitter does the
same per candidate in every wave of k_ris: a guard that is wrongly wave-uniform can show there and nowhere in a uniform scene.

Per case, at 48 x 32, the oracle with cos / sin / atan2 correctly rounded (libm mode 1) and the library run the same calls:
  * ReSTIRDirect, 3 spatiotemporal frames, with the RIS light table in LDS and read from global memory: image, ray count and the
    reservoirs written after every frame, and after the last one the G-buffer planes prim_id, albedo, normal, depth, motion;
  * 2 RIS-only frames (reuse 0), the PT-direct baseline (its own eval_bsdf / pdf quotient), pathTrace at depths 1 and 4,
    pathTraceIndirect at depth 3: images and ray counts;
  * ReSTIRIndirect, 3 frames at depth 3 with temporal reuse: image, ray count and every field of the 68-byte reservoirs;
  * the mixed cases' and the 1e19 emitter's ReSTIRDirect sequences again at 97 x 61, where partial tiles hold mixed waves.
Not run: the RIS-only frames with each table form (they take the default one), anything but ReSTIRDirect on the many-lights case, and
that case with the LDS table (1228 lights are more than the LDS form holds: it takes the global-memory kernel whatever the threshold).

One rule compares everything (extreme_cases.same_bits_or_nan): bit for bit, no tolerance; where the oracle holds a NaN the library must
hold a NaN at the same element, of any sign and payload (x86 gives 0xFFC00000 for 0 / 0, the device 0x7FC00000, and the reference
defines neither).  The number of NaNs per output must be the one tests/test_extreme_cases.py asserts on the oracle alone -- which is
none in any output of any case: the filters remove every NaN weight before it is stored, on both sides.  Infinities are compared like any
other value: the negative light leaves one -inf element in pathTrace's indirect plane at both depths, 3e38 infinite weights in ReSTIR-GI.
"""
import numpy as np
import pytest

from tests import extreme_cases as xc
from tests.common import RIS_TABLE_PIXELS_DEFAULT, HipRenderer, hip_scene

pytestmark = pytest.mark.gpu


@pytest.fixture
def correctly_rounded_libm():
    """As in tests/test_gpu_parity.py: the library evaluates cos / sin / atan2 correctly rounded, so the oracle does too.  The fixture owns
    the mode for the whole test body: extreme_cases.oracle_outputs asserts that it runs inside it and never sets the mode itself."""
    with xc.correctly_rounded_libm():
        yield


@pytest.fixture(scope="module")
def scenes():
    """The library's scene of a case, built once."""
    made = {}
    yield made
    for s in made.values():
        s.destroy()


class HipBackend:
    """The library behind the interface extreme_cases.run drives (its OracleBackend is the other one).  sd: the SceneData to render instead
    of the table's scene of that name (tests/test_gpu_camera_extremes.py: one rs_scene under `name`, a camera per row)."""

    def __init__(self, hip, scenes, name, size, sd=None):
        self.hip, self.sd, self.size, self.n = hip, sd or xc.scene(name), size, size[0] * size[1]
        if name not in scenes:
            scenes[name] = hip_scene(hip, self.sd)
            scenes[name].set_sample_sequence(None)
        self.shared = scenes[name]

    def renderer(self):
        return HipRenderer(self.hip, self.sd, *self.size, scene=self.shared)

    def _image(self):
        import torch
        return torch.zeros((self.n, 3), dtype=torch.float32, device="cuda")

    def last(self, r):
        return r.restir.download(1)

    def gbuffer(self, r):
        g = r.gbuf.download()
        f = g["frame_idx"] ^ 1
        return dict(prim_id=g["prim_id"][f], albedo=g["albedo"], normal=g["normal"][f], depth=g["depth"][f], motion=g["motion"])

    def path_trace(self, r, looper, depth):
        d, i = self._image(), self._image()
        rays = self.hip.path_trace(r.scene, r.cam, d.data_ptr(), i.data_ptr(), 0, looper, depth)
        return d.cpu().numpy(), i.cpu().numpy(), rays

    def pt_indirect(self, r, looper, depth):
        i = self._image()
        rays = self.hip.path_trace_indirect(r.scene, r.cam, i.data_ptr(), 0, looper, depth)
        return i.cpu().numpy(), rays

    def gi_frames(self, r, frames, depth):
        img = self._image()
        for f in range(frames):
            r.gbuf.render(r.scene, r.cam)
            rays = r.restir.indirect(r.scene, r.cam, r.gbuf, img.data_ptr(), 0, f, 1, depth)
            r.gbuf.update(r.cam)
            yield img.cpu().numpy(), rays, r.restir.download_indirect(1)


def _held_to_the_oracle(hip, scenes, name, size, stages, all_stages=None):
    """Runs `stages` of the case on the library and compares every output with the oracle's; the NaN counts must be the ones stated
    for the case (tests/extreme_cases.py EXPECT, asserted on the oracle alone by tests/test_extreme_cases.py)."""
    oracle = xc.oracle_outputs(name, size, all_stages)
    want = {k: v for k, v in oracle.items() if k.split("/")[0] in stages}
    assert want
    got = xc.run(HipBackend(hip, scenes, name, size), stages)
    nans = xc.compare(want, got, (name, size))
    stated = xc.expected(name)["nan"] if size == xc.SIZE else {}
    assert nans == {k: v for k, v in stated.items() if k.split("/")[0] in stages}, (name, nans)


# (the many-lights case has more lights than the LDS form holds: whatever the threshold says it takes the global-memory kernel, once)
DIRECT = [(n, t) for n in xc.NAMES for t in ("lds", "global") if t == "global" or n in xc.CORNELL]


@pytest.mark.parametrize("name,table", DIRECT, ids=["%s-%s" % c for c in DIRECT])
def test_restir_direct_at_the_extremes(hip, scenes, correctly_rounded_libm, name, table):
    hip.set_ris_table_pixels(0 if table == "lds" else 1 << 30)
    try:
        _held_to_the_oracle(hip, scenes, name, xc.SIZE, ("direct3",))
    finally:
        hip.set_ris_table_pixels(RIS_TABLE_PIXELS_DEFAULT)


@pytest.mark.parametrize("name", xc.NAMES)
def test_ris_only_frames_at_the_extremes(hip, scenes, correctly_rounded_libm, name):
    _held_to_the_oracle(hip, scenes, name, xc.SIZE, ("direct0",))


@pytest.mark.parametrize("name", xc.CORNELL)
def test_baseline_passes_at_the_extremes(hip, scenes, correctly_rounded_libm, name):
    _held_to_the_oracle(hip, scenes, name, xc.SIZE, ("ptd", "pt1", "pt4", "pti3"))


@pytest.mark.parametrize("name", xc.CORNELL)
def test_restir_indirect_at_the_extremes(hip, scenes, correctly_rounded_libm, name):
    _held_to_the_oracle(hip, scenes, name, xc.SIZE, ("gi",))


@pytest.mark.parametrize("table", ["lds", "global"])
@pytest.mark.parametrize("name", xc.PARTIAL)
def test_mixed_cases_on_partial_tiles(hip, scenes, correctly_rounded_libm, name, table):
    hip.set_ris_table_pixels(0 if table == "lds" else 1 << 30)
    try:
        _held_to_the_oracle(hip, scenes, name, xc.RAGGED, ("direct3", "direct0"), ("direct3", "direct0"))
    finally:
        hip.set_ris_table_pixels(RIS_TABLE_PIXELS_DEFAULT)
