"""ReSTIR-GI's spatial pass (rs_restir_set_indirect_spatial) without a GPU: the setter's refusals, the ABI, the host sampler hook, and
-- from the CPU oracle and the NumPy restatement of tests/indirect_spatial.py alone -- that the restatement with radius 0.25 is the
oracle's own frame, that the Jacobian is 1 at the source, that the cases of tests/test_gpu_indirect_spatial.py are not vacuous, and that
the pass lowers the error of a frame."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import binding as ob
from restir_amd import capi, sobol
from restir_amd.ctypes_structs import DIELECTRIC, INDIRECT_RESERVOIR_DTYPE, LIGHT
from tests import indirect_spatial as gs
from tests.common import bits_equal
from tests.scene_edits import assert_same

F = np.float32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "restir_hip.h")


@pytest.fixture(autouse=True)
def exact_libm():
    ob.set_libm_mode(1)
    yield
    ob.set_libm_mode(0)


def message_of(code):
    assert code == capi.RS_ERR_INVALID_ARGUMENT
    return capi.lib().rs_last_error().decode()


def test_setter_refusals():
    """What needs no object: the arguments are judged first -- more than 16 taps, a radius that is NaN, infinite or above 64 -- then the
    object.  (Defaults and allocation: tests/test_gpu_indirect_spatial.py test_switches.)"""
    lib = capi.lib()
    assert "16 taps" in message_of(lib.rs_restir_set_indirect_spatial(None, 1, 17, 5.0))
    for radius in (np.nan, np.inf, -np.inf, 64.5):
        assert "radius" in message_of(lib.rs_restir_set_indirect_spatial(None, 1, 5, radius))
    for taps, radius in ((0, 0.0), (-3, -1.0), (16, 64.0), (1, 0.25)):               # acceptable values: only the object is missing
        assert message_of(lib.rs_restir_set_indirect_spatial(None, 1, taps, radius)).endswith("null")
    on = C.c_int(0)
    assert lib.rs_restir_get_indirect_spatial(None, C.byref(on), None, None) == capi.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_restir_download_indirect_spatial(None, None) == capi.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_debug_restir_indirect_spatial(None, None) == capi.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_debug_restir_indirect_spatial_launched(None, C.byref(on)) == capi.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_debug_restir_indirect_primary(None, None, None, None, None) == capi.RS_ERR_INVALID_ARGUMENT


def test_abi():
    text = open(HEADER).read()
    defines = dict(re.findall(r"#define\s+(RS_GI_SPATIAL_\w+)\s+([0-9.]+)f?", text))
    assert int(defines["RS_GI_SPATIAL_MAX_TAPS"]) == capi.RS_GI_SPATIAL_MAX_TAPS == 16
    assert int(defines["RS_GI_SPATIAL_DIM"]) == capi.RS_GI_SPATIAL_DIM == gs.DIM == 150
    assert float(defines["RS_GI_SPATIAL_JACOBIAN_MAX"]) == capi.RS_GI_SPATIAL_JACOBIAN_MAX == float(gs.JACOBIAN_MAX) == 10.0
    assert gs.DIM + 3 * capi.RS_GI_SPATIAL_MAX_TAPS <= sobol.SOBOL_SAMPLE_DIM       # dimensions 150..197 of 200
    assert INDIRECT_RESERVOIR_DTYPE.itemsize == 68 and INDIRECT_RESERVOIR_DTYPE.names == ("Lo", "xv", "nv", "xs", "ns", "numSamples", "weight")
    lib = capi.lib()
    for name in ("rs_restir_set_indirect_spatial", "rs_restir_get_indirect_spatial", "rs_restir_download_indirect_spatial", "rs_debug_restir_indirect_spatial",
                 "rs_debug_restir_indirect_spatial_launched", "rs_debug_restir_indirect_primary", "rs_debug_seeded_uniforms"):
        assert name in capi.EXPORTS and hasattr(lib, name) and re.search(r"\b%s\(" % name, text), name
    assert lib.rs_restir_set_indirect_spatial.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_float]


def test_seeded_uniforms_are_the_generators():
    """The default engine of the hook against the oracle's makeSeededRandomEngine + sample1D, which tests/test_oracle_golden.py holds to
    thrust's recorded streams; the Sobol form needs a scene and is held to tests/golden/sobol_oracle.npz on the GPU."""
    rng = np.random.default_rng(7)
    n, m = 64, 48
    looper = rng.integers(0, 5000, n).astype(np.int32)
    index = rng.integers(0, 1920 * 1080, n).astype(np.int32)
    dim = rng.choice(np.array([0, 1, 150, 199], np.int32), n)
    want = np.zeros((n, m), F)
    ob.lib().orc_rng_stream(n, looper, index, dim, m, want.reshape(-1))
    got = np.stack([capi.seeded_uniforms(None, looper[k], index[k], dim[k], m) for k in range(n)])
    assert bits_equal(got, want)
    assert len(capi.seeded_uniforms(None, 0, 0, 0, 0)) == 0
    lib = capi.lib()
    assert lib.rs_debug_seeded_uniforms(None, 0, 0, 0, 4, None) == capi.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_debug_seeded_uniforms(None, 0, 0, -1, 0, None) == capi.RS_ERR_INVALID_ARGUMENT


def test_jacobian_is_one_at_the_source():
    """The receiver at the neighbour's own visible point: vq == vn, and (a / s * d) / (a / s * d) == 1 exactly whenever it is finite."""
    rng = np.random.default_rng(11)
    n = 4096
    xv, xs = rng.uniform(-2, 2, (n, 3)).astype(F), rng.uniform(-2, 2, (n, 3)).astype(F)
    ns = rng.normal(size=(n, 3)).astype(F)
    jac, _ = gs.jacobian(xv, xs, ns, xv)
    assert np.isfinite(jac).all() and (jac == F(1)).all()
    # ... twice as far along the same line, facing xs squarely both times: the solid angle shrinks fourfold, jac = (1/2 * 1) / (1 * 4) ... inverted
    far, _ = gs.jacobian(np.array([[0, 0, 1]], F), np.zeros((1, 3), F), np.array([[0, 0, 1]], F), np.array([[0, 0, 2]], F))
    assert far[0] == F(0.25)
    near, _ = gs.jacobian(np.array([[0, 0, 2]], F), np.zeros((1, 3), F), np.array([[0, 0, 1]], F), np.array([[0, 0, 1]], F))
    assert near[0] == F(4)
    degenerate, _ = gs.jacobian(np.zeros((1, 3), F), np.zeros((1, 3), F), np.array([[0, 0, 1]], F), np.array([[0, 0, 1]], F))
    assert not np.isfinite(degenerate[0])                    # xv == xs: rejected by the rule


def oracle_for(case, spatial=True):
    name, size, taps, radius, sampler, orbit, depth, reuse, accumulate = case
    table = sobol.sobol_table() if sampler == "sobol" else None
    o = gs.OracleGI(capi, gs.scene_of(name), *size, sobol=table, depth=depth, accumulate=accumulate,
                    draw=gs.oracle_sobol_draw(table) if table is not None else None)
    o.spatial = (taps, radius) if spatial else None
    return o


def run(o, case, frames=gs.FRAMES):
    base = np.array([o.cam.position[i] for i in range(3)], F)
    total, states = dict.fromkeys(gs.COUNTERS + ("outside",), 0), []
    for f in range(frames):
        if case[5]:
            o.set_camera_position(gs.orbit_position(base, f))
        o.render(); o.finish(case[7])
        for k in total:
            total[k] += o.counters.get(k, 0)
        states.append(o.state())
    return total, states


@pytest.mark.parametrize("case", [gs.CASES[1], gs.CASES[2], gs.CASES[4]], ids=gs.case_id)
def test_radius_quarter_is_the_oracles_own_frame(case):
    """Radius 0.25: |offset| <= 0.25 < 0.5, so every tap truncates to the pixel itself and fails the reference's test; the restatement
    then stores S = T and shades T exactly as the oracle's kernel does -- image, reservoirs and rays equal the oracle without the pass."""
    quarter = case[:3] + (0.25,) + case[4:]
    a, b = oracle_for(quarter), oracle_for(quarter, spatial=False)
    ta, sa = run(a, quarter)
    _, sb = run(b, quarter)
    assert ta["failed"] == ta["part"] * case[2] > 0 and ta["accepted"] == ta["walked"] == ta["outside"] == 0
    for f, (x, y) in enumerate(zip(sa, sb)):
        assert x["spatial"][0] and not y["spatial"][0]
        assert_same(dict(image=y["image"], rays=y["rays"], written=y["written"], history=y["history"]),
                    dict(image=x["image"], rays=x["rays"], written=x["written"], history=x["history"]), f)
        assert_same(dict(S=x["written"]), dict(S=x["S"]), f)


def test_the_cases_are_not_vacuous():
    """Conditions on the inputs of the GPU parity cases, from the oracle and the restatement alone, counters summed over a case's frames.
    Per scene, over its cases: each of the eight counters is non-zero -- `no_point` (a sample of weight > 0 without a second vertex) only
    where an environment map can give an escaped first bounce radiance, so on `env` alone; elsewhere it is provably 0 and asserted so;
    some case's last frame has at least a quarter of the pixels taking part adopting a neighbour's sample and at least 8 winners
    blocked; taps fall outside the image; and the glass scene shows Dielectric and Light pixels, which do not take part."""
    by_scene = {}
    for case in gs.CASES:
        o = oracle_for(case)
        total, _ = run(o, case)
        last = dict(o.counters, adopted=int(o.adopted.sum()))
        print(gs.case_id(case), total, "last frame:", last)
        assert total["part"] > 0 and total["accepted"] > 0 and total["failed"] > 0
        s = by_scene.setdefault(case[0], dict(total=dict.fromkeys(total, 0), quarter=False, kinds=set()))
        for k in total:
            s["total"][k] += total[k]
        s["quarter"] |= 4 * last["adopted"] >= last["part"] and last["blocked"] >= 8
        s["kinds"] |= set(np.unique(o.recv["kind"]).tolist())
    for name, s in by_scene.items():
        for k in gs.COUNTERS + ("outside",):
            if k == "no_point" and name != "env":
                assert s["total"][k] == 0, (name, k)
            else:
                assert s["total"][k] > 0, (name, k, s["total"])
        assert s["quarter"], name
        assert s["total"]["blocked"] >= 8
    assert {DIELECTRIC, LIGHT, -1} <= by_scene["glass"]["kinds"]


def test_what_it_buys():
    """cornell at 64x48 (a size of the GPU tests), depth 3, reuse 3: mean squared error of one frame against pathTraceIndirect accumulated
    over 1 024 iterations, with the pass (5 taps, radius 5) and without.  The frame is the FIRST one: it has no history, so both runs
    trace the same rays and the difference is the pass alone.  Its error must be lower with the pass; the ratios of the first, second,
    fourth and ninth frame are printed (measured 0.57, 0.48, 0.92, 0.77).  The pass is the biased variant (no count of Z, a blocked
    winner blackens its pixel for the frame): the mean of sixty first frames is 8 % darker than the reference.  At 40x24, where the
    radius of 5 pixels spans a tenth of the room, the ninth frame (M clamped at 20 already) measured 1.19: no gain there."""
    W, H, depth = 64, 48, 3
    sd = gs.scene_of("cornell")
    scene = gs.oracle_scene(sd)
    scene.set_sample_sequence(None)
    cam = ob.camera_update(sd.camera(W, H))
    ref = np.zeros((W * H, 3), F)
    for it in range(1024):
        ob.pt_indirect(scene, cam, ref, it, 100000 + it, depth)
    mse = {}
    for on in (False, True):
        o = gs.OracleGI(capi, sd, W, H, depth=depth)
        o.spatial = (5, 5.0) if on else None
        mse[on] = []
        for f in range(9):
            o.render(); o.finish(3)
            mse[on].append(float(np.mean((o.image.astype(np.float64) - ref) ** 2)))
    for f in (0, 1, 3, 8):
        print("frame %d: mse without %.6g, with %.6g, ratio %.3f" % (f + 1, mse[False][f], mse[True][f], mse[True][f] / mse[False][f]))
    assert mse[True][0] < mse[False][0]
