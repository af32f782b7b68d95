"""GPU: LeveledEAWFilter and SpatioTemporalFilter (restir_amd/csrc/denoiser.hip) on the synthetic edge cases of tests/denoise_cases.py,
held to the float64 reference of tests/denoise_reference.py.

The denoisers are the part of the product that is compared within a tolerance, and the part whose kernels leave the reference's
arithmetic (hardware 2^t, Markstein division, squarings for powf(c, 128), fused taps, LDS row-phase tiles).  Every kernel form the host
dispatches runs here: k_wavelet<M> / k_wavelet_tiled<S, M, *> for M = 0 .. 8, every k_svgf_wavelet* instantiation of
rs_svgf_filter_rows.  What is asserted, on every pixel (nothing is masked, nothing skipped):

  1. EAW within 1 unit of float64 -- a unit is |x - ref| / (atol + rtol |ref|), rtol 1e-5, atol 1e-6 * S, S the case's radiance scale.
  2. The tile form equals the plain gathers bit for bit: the filter, and every level 0 .. 4 of the row form on ranges that are whole,
     one row, shorter than the step, start inside a block, or clamp; a ranged call writes those rows of the full-frame call only.
  3. Null pixels (id <= -1) keep their colour (and variance) bit for bit; an all-null frame comes back identical.
  4. A constant image stays constant to 64 * 2^-24 relative (two 25-term sums of non-negative terms and one division, first order).
  5. +Inf / NaN samples: the set of non-finite output pixels is the oracle's; the finite ones are within a unit of the oracle.
  6. SVGF over 7 frames within 1 unit of float64 on the filtered colour, the variance, the colour history and the moments (rtol / atol
     3e-5 / 2e-6 S, 3e-5 / 1e-6 S^2, 1e-6 / 1e-7 (S, S^2, 1)); the moments bit-equal to the oracle; tile equals plain where eligible.
  7. rs_modulate_albedo / rs_add_image* bit-exact against the oracle on the values around the zero denominator.
  8. rs_eaw_level_rows: levels 5, 6 and 29 against the float64 level, level 30 refused (x + 2 * (1 << 30) overflows).

Measured on an MI355X, GPU against float64, largest value over all cases, in units:
  rs_eaw_filter        separately rounded taps (k_wavelet<0..7>, k_wavelet_tiled<S, 0..7, *>)          0.095   (oracle: 0.099)
                       fused taps (k_wavelet<8>, k_wavelet_tiled<S, 8, *>)                             0.075
  rs_eaw_level_rows    levels 5 / 6 / 29                                                               0.045 / 0.045 / 0.007
  rs_svgf_filter       per dispatch branch of rs_svgf_filter_rows:               colour  variance  history  moments
    k_svgf_wavelet_tiled<S, 7, true, true>    4 / 128 / 1 and 10.5 / 128 / .25    0.134    0.314    0.096    0.264
    k_svgf_wavelet_tiled<S, 7, true>          the same sigmas                     0.067    0.314    0.051    0.264
    k_svgf_wavelet<7, true, true>             4 / 128 / 1                         0.059    0.314    0.041    0.264
    k_svgf_wavelet<7, true>                   4 / 128 / .25                       0.133    0.195    0.096    0.207
    k_svgf_wavelet<7, false>                  4 / 128 / .3                        0.129    0.195    0.096    0.207
    k_svgf_wavelet<6, true> / <6, false>      4 / 64 / 1, 10.5 / 64 / .3          0.018    0.089    0.019    0.194
    k_svgf_wavelet<5, true> / <5, false>      4 / 32 / .25, 4 / 32 / .3           0.018    0.267    0.019    0.217
    k_svgf_wavelet<-1, true> / <-1, false>    sigNormal 2, 1, 100, .5, 7.3        0.029    0.223    0.052    0.209
  (the variance and moment columns are the oracle's own distance from float64: the moments are bit-equal to the oracle's and the variance
  estimate is the same operations)
  constant image: largest relative departure 6.0e-7 (EAW), 7.5e-7 (SVGF) for the bound 3.8e-6.
Which kernel instantiations ran: profiles/denoise_edges_kernel_forms.csv (a kernel trace of this module alone).

What the module found: div_sigma's residual is Inf - Inf for an infinite numerator or divisor, so the separately rounded forms answered an
Inf sample with NaN in every channel where the oracle keeps the finite ones (item 5; fixed in denoiser.hip), and rs_eaw_level_rows took
level 30, whose tap offset overflows (item 8; now refused).
Checked once against deliberately wrong kernels (values only, never committed): a Gaussian coefficient off in its last digit fails
test_eaw_filter_on_edge_case (16 cases), test_svgf_filter_on_edge_case (9) and the level 5 / 6 test; wNorm without its + 1e-4f fails
test_svgf_filter_on_edge_case (9 cases); halo columns of the EAW tile staged from the neighbouring pixel fail test_eaw_filter_on_edge_case
and test_eaw_row_form_on_edge_case (12 cases each).  Swapping the loop variables in k_svgf_filter_variance is NOT caught, and cannot be by
a value comparison: the 3 x 3 table is symmetric, so the swap is the same filter with another summation order.
"""
import numpy as np
import pytest

from oracle import binding as ob
from tests import denoise_cases as dc
from tests import denoise_reference as ref64
from tests.common import bits_equal

pytestmark = pytest.mark.gpu

SENTINEL = 777.0


def _same_with_nan(a, b):
    """Bit equality where both are numbers, NaN where either is (a NaN's payload is not part of any contract)."""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _where_differs(a, b, va, vb):
    """For an assertion's message: how many elements of two masks differ, and the first few with the values behind them."""
    idx = np.argwhere(a != b)
    return len(idx), [(tuple(int(t) for t in i), va[tuple(i)], vb[tuple(i)]) for i in idx[:6]]


class Device:
    """One case on the device: the library's G-buffer with the case's planes, the colour of each frame."""

    def __init__(self, hip, name):
        import torch
        self.torch, self.hip = torch, hip
        self.c = dc.get(name)
        self.W, self.H, self.n = self.c.W, self.c.H, self.c.W * self.c.H
        self.cam = self.c.cam                    # the camera the float64 reference and the oracle read, field for field
        self.gbuf = hip.GBuffer(self.W, self.H)
        self.frame(0)

    def frame(self, k):
        fr = self.c.frames[k]
        dc.load_device(self.hip, self.gbuf, fr)
        self.color = self.torch.from_numpy(fr.color.reshape(-1, 3)).cuda()
        self.color_host = fr.color.reshape(-1, 3)
        self.null = fr.ids.reshape(-1) <= -1
        return fr

    def grab(self, ptr, count):
        t = self.torch.empty(count, dtype=self.torch.float32, device="cuda")
        self.hip.hip_memcpy_d2d(t.data_ptr(), ptr, count * 4)
        return t.cpu().numpy()

    def eaw(self, f, sigma, fused, tiled):
        f.set_params(*sigma, level=5); f.set_fused(fused); f.set_tiled(tiled)
        out = self.torch.zeros_like(self.color)
        p = f.filter(out.data_ptr(), self.color.data_ptr(), self.gbuf, self.cam)
        self.hip.synchronize()
        return self.grab(p, self.n * 3).reshape(-1, 3)

    def destroy(self):
        self.gbuf.destroy()


def _constant_bound(got, hit, constant):
    rel = np.abs(got[hit].astype(np.float64) - constant) / np.abs(constant)
    return float(rel.max()) if rel.size else 0.0


@pytest.mark.parametrize("name", dc.NAMES)
def test_eaw_filter_on_edge_case(hip, name):
    """Items 1 - 5 for rs_eaw_filter: every sigma set of the case, separately rounded and fused taps, tile and plain gathers."""
    d = Device(hip, name)
    c, fr = d.c, d.c.frames[0]
    f = hip.EAWFilter(d.W, d.H, 5)
    worst = {False: 0.0, True: 0.0}
    worst_const = 0.0
    for k in dc.eaw_sigma_sets(name):
        sigma = dc.EAW_SIGMAS[k]
        for fused in ((False, True) if k in dc.EAW_FUSED else (False,)):
            tiled, plain = d.eaw(f, sigma, fused, True), d.eaw(f, sigma, fused, False)
            assert _same_with_nan(tiled, plain), (sigma, fused, int((tiled.view(np.uint32) != plain.view(np.uint32)).sum()))       # 2
            assert bits_equal(tiled[d.null], d.color_host[d.null]), (sigma, fused)                                                 # 3
            if c.structural is None:
                r, _ = dc.eaw_reference(name, sigma)
                u = float(dc.eaw_units(tiled, r, c.scale).max())
                print(f"EAW {name} sigmas {sigma} fused {fused}: GPU vs float64 {u:.3f} units")
                worst[fused] = max(worst[fused], u)
                assert u <= 1.0, (sigma, fused, u)                                                                                  # 1
            else:
                o = dc.oracle_eaw(name, sigma)
                assert np.array_equal(np.isfinite(tiled), np.isfinite(o)), (sigma, fused, _where_differs(np.isfinite(tiled), np.isfinite(o), tiled, o))   # 5
                fin = np.isfinite(o)
                assert not fin.all()
                u = float(dc.eaw_units(tiled[fin], o[fin], c.scale).max()) if fin.any() else 0.0
                print(f"EAW {name} sigmas {sigma} fused {fused}: GPU vs oracle on the finite pixels {u:.3f} units")
                assert u <= 1.0, (sigma, fused, u)
            if name == "constant_image":
                const = fr.color.reshape(-1, 3)[0].astype(np.float64)
                worst_const = max(worst_const, _constant_bound(tiled, ~d.null, const))
                assert worst_const <= 64 * 2.0 ** -24, (sigma, fused, worst_const)                                                  # 4
    if name == "constant_image":
        print(f"EAW constant image: largest relative departure {worst_const:.3e} (bound {64 * 2.0 ** -24:.3e})")
    if name == "all_null":
        assert d.null.all()
    f.destroy(); d.destroy()


def _row_ranges(H, step):
    short = max(1, min(step, H) // 2)
    return [(0, H), (1, 2), (H - 1, H), (min(2, H - 1), min(2, H - 1) + short), (3, min(H, 14)), (-5, min(4, H)), (max(0, H - 3), H + 7)]


@pytest.mark.parametrize("name", dc.NAMES)
def test_eaw_row_form_on_edge_case(hip, name):
    """Item 2 for rs_eaw_positions_rows + rs_eaw_level_rows: each level 0 .. 4, tile against plain gathers, on row ranges [0, H), [1, 2),
    [H - 1, H), one shorter than the step, one that starts inside a block, two that clamp.  A ranged call equals those rows of the
    full-frame call of the same level and leaves every other row of its output alone."""
    import torch
    d = Device(hip, name)
    W, H = d.W, d.H
    f = hip.EAWFilter(W, H, 5)
    for sigma, fused in ((dc.EAW_SIGMAS[5], True), (dc.EAW_SIGMAS[dc.NAMES.index(name) % 8], False)):
        f.set_params(*sigma, level=5); f.set_fused(fused)
        f.positions_rows(d.gbuf, d.cam, 0, H)
        for level in range(5):
            results = {}
            for tiled in (True, False):
                f.set_tiled(tiled)
                for (y0, y1) in _row_ranges(H, 1 << level):
                    out = torch.full_like(d.color, SENTINEL)
                    f.level_rows(out.data_ptr(), d.color.data_ptr(), d.gbuf, level, y0, y1)
                    hip.synchronize(); torch.cuda.synchronize()
                    results[(tiled, y0, y1)] = out.cpu().numpy().reshape(H, W, 3)
            full = results[(True, 0, H)]
            assert _same_with_nan(full, results[(False, 0, H)]), (sigma, level)
            untouched = np.full((H, W, 3), SENTINEL, np.float32)
            assert not bits_equal(full, untouched)
            for (tiled, y0, y1), got in results.items():
                a, b = max(0, y0), min(H, y1)
                expect = untouched.copy()
                if b > a:
                    expect[a:b] = full[a:b]
                assert _same_with_nan(got, expect), (sigma, level, tiled, y0, y1)
            hit = ~d.null.reshape(H, W)
            assert bits_equal(full[~hit], d.color_host.reshape(H, W, 3)[~hit])                    # 3, level by level
    f.destroy(); d.destroy()


def test_eaw_level_rows_beyond_the_fifth_level(hip):
    """Item 8.  Levels 5 and 6 (taps 32 and 64 pixels apart, plain gathers whatever rs_eaw_set_tiled says) against the float64 level on a
    frame wide enough to hold such taps; level 29, the last whose tap offsets fit an int, keeps the image to rounding; 30 is refused."""
    import torch
    name = "big_one_id"
    d = Device(hip, name)
    c, fr = d.c, d.c.frames[0]
    W, H = d.W, d.H
    pos = ref64.positions(c.cam, fr.depth)
    f = hip.EAWFilter(W, H, 5)
    f.positions_rows(d.gbuf, d.cam, 0, H)
    sigma = (64.0, 8.0, 16.0)                     # wide enough that a tap 32 or 64 pixels away on this geometry still weighs in
    for fused in (False, True):
        f.set_params(*sigma, level=5); f.set_fused(fused)
        for level in (5, 6, 29):
            out = torch.full_like(d.color, SENTINEL)
            f.level_rows(out.data_ptr(), d.color.data_ptr(), d.gbuf, level, 0, H)
            hip.synchronize(); torch.cuda.synchronize()
            r, dec = ref64.eaw_level(fr.ids, fr.normal, pos, fr.color, *sigma, level)
            u = float(dc.eaw_units(out.cpu().numpy().reshape(-1, 3), r.reshape(-1, 3), c.scale).max())
            print(f"EAW level {level} fused {fused}: GPU vs float64 {u:.3f} units")
            assert u <= 1.0, (level, fused, u)
            if level < 29:
                assert np.abs(r - fr.color).max() > 1e-3                    # taps that far away are inside this frame and count
    for level in (30, 31, -1):
        with pytest.raises(hip.RestirHipError):
            f.level_rows(out.data_ptr(), d.color.data_ptr(), d.gbuf, level, 0, H)
    f.destroy(); d.destroy()


def _svgf_run(d, hip, form, tiled=None):
    sl, sn, sd, fused, t = form
    f = hip.SVGFFilter(d.W, d.H, 5)
    f.set_params(sl, sn, sd, level=5); f.set_fused(fused); f.set_tiled(t if tiled is None else tiled)
    out = []
    for k in range(len(d.c.frames)):
        d.frame(k)
        img = d.grab(f.filter(d.color.data_ptr(), d.gbuf, d.cam), d.n * 3).reshape(-1, 3)
        v = f.view()
        assert v.frameIdx == k % 2
        out.append(dict(filtered=img, variance=d.grab(v.devVariance, d.n), accum_color=d.grab(v.devAccumColor[v.frameIdx], d.n * 3).reshape(-1, 3),
                        accum_moment=d.grab(v.devAccumMoment[v.frameIdx], d.n * 3).reshape(-1, 3)))
        f.next_frame()
    f.destroy()
    return out


PLANES = (("colour", "filtered"), ("variance", "variance"), ("colour", "accum_color"), ("moment", "accum_moment"))


@pytest.mark.parametrize("name", dc.SVGF_NAMES)
def test_svgf_filter_on_edge_case(hip, name):
    """Items 3 - 6 for rs_svgf_filter over the case's 7 frames, in every form of the case (sigmas x fused x tiled -> one dispatch branch
    of rs_svgf_filter_rows each)."""
    d = Device(hip, name)
    c = d.c
    tolerance = name in dc.SVGF_TOLERANCE_NAMES
    for k in dc.svgf_forms(name):
        form = dc.SVGF_FORMS[k]
        sigma = form[:3]
        got = _svgf_run(d, hip, form)
        orc = dc.oracle_svgf(name, sigma)
        r64 = dc.svgf_reference(name, sigma) if tolerance else None
        eligible = sigma[1] == 128.0 and sigma[2] in (1.0, 0.25)
        twin = _svgf_run(d, hip, form, tiled=not form[4]) if eligible else None
        worst = {}
        for frame, g in enumerate(got):
            fr = c.frames[frame]
            null = fr.ids.reshape(-1) <= -1
            o = orc[frame]
            assert bits_equal(g["filtered"][null], fr.color.reshape(-1, 3)[null]), (form, frame)                                   # 3
            assert _same_with_nan(g["variance"][null], o["variance"][null]), (form, frame)
            assert _same_with_nan(g["accum_moment"], o["accum_moment"]), (form, frame)                                             # 6: identical operations
            if twin is not None:
                for _, key in PLANES:
                    assert _same_with_nan(g[key], twin[frame][key]), (form, frame, key)                                            # 2
            if tolerance:
                for plane, key in PLANES:
                    u = float(dc.svgf_units(plane, g[key], r64[frame][key], c.scale).max())
                    worst[key] = max(worst.get(key, 0.0), u)
                    assert u <= 1.0, (form, frame, key, u)                                                                          # 6
            else:
                for _, key in PLANES:
                    assert np.array_equal(np.isfinite(g[key]), np.isfinite(o[key])), (form, frame, key, _where_differs(np.isfinite(g[key]), np.isfinite(o[key]), g[key], o[key]))   # 5
            if name == "constant_image":
                const = fr.color.reshape(-1, 3)[0].astype(np.float64)
                rel = _constant_bound(g["filtered"], ~null, const)
                worst["constant"] = max(worst.get("constant", 0.0), rel)
                assert rel <= 64 * 2.0 ** -24, (form, frame, rel)                                                                   # 4
        print(f"SVGF {name} form {k} {form}: GPU vs float64, units: " + ", ".join(f"{a} {b:.3g}" for a, b in worst.items()))
    d.destroy()


def test_modulate_and_add_around_the_zero_denominator(hip):
    """Item 7: rs_modulate_albedo (c / (1 - c + 1e-4f) * max(albedo, 0)) and rs_add_image / rs_add_image3 bit-exact against the oracle on
    colours {0, .5, 1 - 1e-4, 1, 1 + 1e-4 and its float neighbours (the denominator passes through zero), 2, 1e4, +Inf, NaN} x albedo
    {-1, 0, .3, 1}."""
    import torch
    one = np.float32(1.0); e = np.float32(1e-4)
    z = one + e
    colours = np.array([0.0, 0.5, one - e, 1.0, np.nextafter(z, np.float32(0)), z, np.nextafter(z, np.float32(2)), 2.0, 1e4, np.inf, np.nan], np.float32)
    albedos = np.array([-1.0, 0.0, 0.3, 1.0], np.float32)
    W, H = len(colours) * len(albedos), 1
    img = np.repeat(colours, len(albedos))[:, None] * np.ones((1, 3), np.float32)
    img[:, 1] = np.roll(img[:, 1], 4)                                             # the channels of a pixel differ
    alb = np.tile(albedos, len(colours))[:, None] * np.ones((1, 3), np.float32)
    other = np.linspace(-1.0, 3.0, W * 3, dtype=np.float32).reshape(W, 3)
    g = hip.GBuffer(W, H)
    v = g.view()
    t_alb = torch.from_numpy(alb).cuda()
    hip.hip_memcpy_d2d(v.devAlbedo, t_alb.data_ptr(), W * 12)
    expect = img.copy()
    with np.errstate(all="ignore"):
        ob.lib().orc_modulate(W, H, expect.reshape(-1), alb.reshape(-1))
    t = torch.from_numpy(img).cuda()
    hip.check(hip.lib().rs_modulate_albedo(t.data_ptr(), g.handle))
    hip.synchronize()
    got = t.cpu().numpy()
    assert _same_with_nan(got, expect), (got, expect)
    assert np.isfinite(expect).sum() > W and not np.isfinite(expect).all()
    t2 = torch.from_numpy(other).cuda()
    hip.check(hip.lib().rs_add_image(t.data_ptr(), t2.data_ptr(), W, H))
    hip.synchronize()
    with np.errstate(all="ignore"):
        assert _same_with_nan(t.cpu().numpy(), expect + other)
        t3 = torch.empty_like(t)
        hip.check(hip.lib().rs_add_image3(t3.data_ptr(), t.data_ptr(), t2.data_ptr(), W, H))
        hip.synchronize()
        assert _same_with_nan(t3.cpu().numpy(), (expect + other) + other)
    g.destroy()
