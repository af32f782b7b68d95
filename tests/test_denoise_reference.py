"""CPU: the C oracle's two denoisers against the float64 reference (tests/denoise_reference.py) on the synthetic cases
(tests/denoise_cases.py), and the oracle's default SpatioTemporalFilter against its pin.

The GPU tests hold the kernels to the stated tolerance against float64 (tests/test_gpu_denoise_edges.py).  That is only meaningful on
inputs for which float32 arithmetic in the reference's own order is well inside the tolerance, so every case and sigma set that takes part
in a tolerance comparison must satisfy here, on every pixel of every plane:

  * the oracle is within 0.5 unit of float64, a unit being |x - ref| / (atol + rtol |ref|) with the stated rtol / atol and atol scaled
    by the case's radiance scale (denoise_cases.py: S for colour, S^2 for variance).  A condition on the case, not a measurement to
    tune: a case that fails it goes to the structural-only list with its reason.
  * oracle and float64 took the same branch on every pixel, with margin (|n . n_last| at least 0.02 from the 0.1 threshold, the sums of
    weights at least a decade from FLT_EPSILON).  The weights' sum of the colour filter cannot vanish for a finite input -- the centre
    tap has dc = dn = dp = 0 exactly, so it alone contributes .1621 -- and SVGF's sumWeight cannot fall below FLT_EPSILON either: its
    centre tap is at least .1621 * 1e-4 * 1 * 1.  sumWeight2 < FLT_EPSILON is reached (case zero_normals).

Measured maxima, oracle against float64, in units:
  LeveledEAWFilter, filtered colour, 25 cases x 2-3 sigma sets                        0.099   (big_one_id, sigmas 64 / .2 / .6)
  SpatioTemporalFilter, 17 cases x 1-3 sigma sets x 7 frames:  filtered colour         0.133   (row_40x1)
                                                               variance                0.314   (block_lights)
                                                               colour history          0.098   (row_40x1)
                                                               moments                 0.264   (block_lights)
Structural-only cases (denoise_cases.TABLE / SVGF_STRUCTURAL carry the reasons):
  nonfinite_130x70, nonfinite_64x8   both filters: +Inf / NaN samples -- which pixels a non-finite value reaches is not a rounding question
  plateaus                           SVGF only: the variance inside a plateau is exactly 0, float32 leaves cancellation noise, and the colour
                                     weight's denominator (1e-4 against ~5e-3) follows it; the oracle is 130 .. 1100 units from float64
  fireflies                          SVGF only: next to a 1e4 S sample E[l^2] - E[l]^2 cancels two decades, the weights' exponents of ~7
                                     carry that 1e-4; the oracle is 0.6 .. 0.9 unit from float64
"""
import os

import numpy as np
import pytest

from tests import denoise_cases as dc
from tests.common import bits_equal

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", dc.TOLERANCE_NAMES)
def test_oracle_eaw_within_half_a_unit_of_float64(name):
    c = dc.get(name)
    worst = 0.0
    for k in dc.eaw_sigma_sets(name):
        sigma = dc.EAW_SIGMAS[k]
        ref, d = dc.eaw_reference(name, sigma)
        got = dc.oracle_eaw(name, sigma)
        assert np.isfinite(ref).all() and np.isfinite(got).all()
        u = float(dc.eaw_units(got, ref, c.scale).max())
        print(f"EAW {name} sigmas {sigma}: oracle vs float64 {u:.3f} units")
        worst = max(worst, u)
        assert not d["sum_w_zero"].any() and d["min_sum_w"] >= 0.16          # the centre tap alone: no pixel near sumWeight == 0
        null = c.frames[0].ids.reshape(-1) <= -1
        assert bits_equal(got[null], c.frames[0].color.reshape(-1, 3)[null])
    assert worst <= 0.5, worst


@pytest.mark.parametrize("name", dc.SVGF_TOLERANCE_NAMES)
def test_oracle_svgf_within_half_a_unit_of_float64(name):
    c = dc.get(name)
    n = c.W * c.H
    worst = {}
    for sigma in sorted({dc.SVGF_FORMS[k][:3] for k in dc.svgf_forms(name)}):
        ref = dc.svgf_reference(name, sigma)
        got = dc.oracle_svgf(name, sigma)
        for frame, (r, g) in enumerate(zip(ref, got)):
            d = r["decisions"]
            # the same branches: history kept or dropped, temporal or spatial variance, the two fall-backs of every level
            assert np.array_equal(g["accum_moment"][:, 2] == 0.0, d["diff"].reshape(-1)), (sigma, frame)
            assert np.array_equal(g["accum_moment"][:, 2] > 3.5, d["temporal_variance"].reshape(-1)), (sigma, frame)
            assert np.array_equal((g["branches"] & 1) != 0, d["sum_w_small"].reshape(5, n)), (sigma, frame)
            assert np.array_equal((g["branches"] & 2) != 0, d["sum_w2_small"].reshape(5, n)), (sigma, frame)
            nd = d["normal_dot"][np.isfinite(d["normal_dot"])]
            assert nd.size == 0 or np.abs(nd - 0.1).min() >= 0.02, (sigma, frame)
            assert d["min_sum_w"] > 10 * np.finfo(np.float32).eps and d["sum_w2_log_margin"] > 1.0, (sigma, frame, d["min_sum_w"], d["sum_w2_log_margin"])
            assert not d["sum_w_small"].any()
            for plane, key in (("colour", "filtered"), ("variance", "variance"), ("colour", "accum_color"), ("moment", "accum_moment")):
                assert np.isfinite(g[key]).all()
                u = float(dc.svgf_units(plane, g[key], r[key], c.scale).max())
                worst[key] = max(worst.get(key, 0.0), u)
                assert u <= 0.5, (sigma, frame, key, u)
    print(f"SVGF {name}: oracle vs float64, units: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_cases_reach_the_branches_they_are_built_for():
    """The time axis crosses the m.z > 3.5 switch, keeps and drops history, and one case takes the variance fall-back."""
    r = dc.svgf_reference("under_tile_63x7", (4.0, 128.0, 1.0))
    assert r[6]["decisions"]["temporal_variance"].any() and not r[3]["decisions"]["temporal_variance"].any()
    d = r[2]["decisions"]
    assert d["diff"].any() and not d["diff"].all()
    seen = np.unique(np.round(d["normal_dot"][np.isfinite(d["normal_dot"])], 2))
    assert set(seen) == {0.0, 0.05, 0.5, 1.0}, seen
    z = dc.svgf_reference("zero_normals", (4.0, 128.0, 1.0))[0]["decisions"]
    assert z["sum_w2_small"].any() and not z["sum_w2_small"].all()
    p = dc.svgf_reference("wide_70x5", (4.0, 128.0, 1.0))[1]["decisions"]["diff"]
    assert p[:2].all() and p[:, :3].all() and not p.all()                       # the pan's source left the frame


def test_every_svgf_dispatch_branch_is_in_the_table():
    """The forms of denoise_cases.SVGF_FORMS between them take every branch of rs_svgf_filter_rows' dispatch, and every form is run by at
    least one case."""
    def branch(form):
        sl, sn, sd, fused, tiled = form
        pow2 = sd in (1.0, 0.25)
        if tiled and sn == 128.0 and pow2:
            return ("tiled", fused)
        if sn == 128.0 and pow2 and fused:
            return ("plain fused",)
        return ({128.0: 7, 64.0: 6, 32.0: 5}.get(sn, -1), pow2)
    seen = {branch(f) for f in dc.SVGF_FORMS}
    assert seen == {("tiled", True), ("tiled", False), ("plain fused",)} | {(n, p) for n in (7, 6, 5, -1) for p in (True, False)}
    used = set()
    for name in dc.SVGF_NAMES:
        used |= set(dc.svgf_forms(name))
    assert used == set(range(len(dc.SVGF_FORMS)))
    sets = set()
    for name in dc.NAMES:
        sets |= set(dc.eaw_sigma_sets(name))
    assert sets == set(range(8))


def test_modulate_and_add_reference_agree_with_the_oracle_on_plain_values():
    from oracle import binding as ob
    from tests import denoise_reference as ref
    rng = np.random.default_rng(3)
    img = rng.uniform(0, 0.95, (64, 3)).astype(np.float32); alb = rng.uniform(-0.2, 1, (64, 3)).astype(np.float32)
    got = img.copy(); ob.lib().orc_modulate(8, 8, got.reshape(-1), alb.reshape(-1))
    assert np.allclose(got, ref.modulate_albedo(img, alb), rtol=1e-6, atol=0)
    assert np.array_equal(ref.add(img, alb).astype(np.float32), img + alb)


def test_default_sigmas_leave_the_oracle_svgf_as_it_was():
    """orc_svgf_set_params is inert until called: the default filter on a rendered sequence equals the pin written before the sigmas
    became parameters (tests/golden/make_svgf_pin.py), bit for bit; setting the defaults explicitly changes nothing either."""
    from tests.golden import make_svgf_pin
    pin = np.load(os.path.join(GOLD, "svgf_oracle_default.npz"))
    out = make_svgf_pin.run()
    assert sorted(pin.files) == sorted(out)
    for k in pin.files:
        assert bits_equal(pin[k], out[k]), k


def test_reference_level_on_a_row_range_is_those_rows_of_the_whole_level():
    from tests import denoise_reference as ref
    c = dc.get("wide_70x5"); fr = c.frames[0]
    pos = ref.positions(c.cam, fr.depth)
    full, _ = ref.eaw_level(fr.ids, fr.normal, pos, fr.color, 64.0, 0.2, 1.0, 2)
    part, _ = ref.eaw_level(fr.ids, fr.normal, pos, fr.color, 64.0, 0.2, 1.0, 2, rows=(-3, 2), out=np.full((c.H, c.W, 3), 7.0))
    assert np.array_equal(part[:2], full[:2]) and (part[2:] == 7.0).all()
    # the oracle's position of a pixel against the float64 one: float32 rounding of a point a few units from the origin
    g = ob_gbuffer(c)
    lvl = np.zeros((c.W * c.H, 3), np.float32)
    from oracle import binding as ob
    import ctypes as C
    ob.lib().orc_eaw_level(C.byref(g.c), C.byref(c.cam), fr.color.reshape(-1), lvl.reshape(-1), 1.0, 0.2, 64.0, 2)
    assert float(dc.eaw_units(lvl, full.reshape(-1, 3), c.scale).max()) <= 0.5


def ob_gbuffer(c):
    from oracle import binding as ob
    g = ob.GBuffer(c.W, c.H)
    dc.load_oracle(g, c.frames[0])
    return g
