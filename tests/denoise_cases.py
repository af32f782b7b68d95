"""Synthetic edge inputs for the two denoisers: a seeded table of named cases, written straight into the G-buffer planes.

A case is a frame size, an id pattern, a geometry (normals, depth), a colour model with a radiance scale and -- for SpatioTemporalFilter
-- a time axis of 7 frames (motion, last ids, last normals).  The axes are combined sparingly: a few dozen named cases, not a cross
product.  `make(name)` returns the float32 planes; `load_oracle` / `load_device` put one frame of them into the oracle's G-buffer
(numpy planes) and into the library's (device planes of rs_gbuffer_get_view, both sets).  Nothing is rendered.

A case whose `structural` is a string takes part in the structural checks only (bit equality of the kernel forms, null pixels, the set
of non-finite pixels), not in a comparison within a tolerance; the string says why.
"""
import zlib

import numpy as np

from oracle import binding as ob
from tests.common import get_scene

FRAMES = 7
LUM32 = np.array([.2126, .7152, .0722], np.float32)

# name: (W, H, ids, geometry, colour, scale, time axis or None, structural-only reason or None)
#   ids       one | vstripes:P | hstripes:P | checker:P | tile_edges | extremes | null
#             + "+miss:F" scattered misses (-1), "+lights:F" scattered lights (-2), "+blockmiss" / "+blocklights" blocks of them
#   geometry  flat | curved (normals turn 1 rad, depth spreads |dp|^2 to ~5, over 32 pixels) | ripple (ramp + ripple of the depth) |
#             depthstep (a step of the depth inside one id) | far (depth 1e4) | zeronormal (a block of zero normals)
#   colour    smooth (structure + noise) | constant | zero | plateaus | fireflies | nonfinite
#   time      identity | pan | idchange | normals | nullflip
TABLE = {
    "one_pixel":          (1, 1, "one", "flat", "smooth", 4.0, "identity", None),
    "column_1x40":        (1, 40, "hstripes:3", "curved", "smooth", 0.4, "identity", None),
    "row_40x1":           (40, 1, "checker:2", "curved", "smooth", 4.0, "pan", None),
    "tiny_5x3":           (5, 3, "one", "curved", "smooth", 40.0, "normals", None),
    "under_tile_63x7":    (63, 7, "vstripes:16", "curved", "smooth", 4.0, "normals", None),
    "tile_64x8_hdr":      (64, 8, "one", "ripple", "smooth", 1000.0, "nullflip", None),
    "tile_edges_65x9":    (65, 9, "tile_edges", "curved", "smooth", 4.0, "idchange", None),
    "tall_3x50":          (3, 50, "hstripes:17", "ripple", "smooth", 40.0, None, None),
    "wide_70x5":          (70, 5, "vstripes:17", "ripple", "smooth", 4.0, "pan", None),
    "checker1_130x70":    (130, 70, "checker:1", "curved", "smooth", 0.4, None, None),
    "checker3_nulls":     (130, 70, "checker:3+miss:0.1", "curved", "smooth", 4.0, "identity", None),
    "block_lights":       (130, 70, "one+blocklights", "depthstep", "smooth", 40.0, "pan", None),
    "block_misses":       (130, 70, "hstripes:16+blockmiss+lights:0.02", "ripple", "smooth", 4.0, None, None),
    "big_one_id":         (300, 200, "one", "curved", "smooth", 4.0, None, None),
    "pan_200x136":        (200, 136, "vstripes:17+miss:0.02", "curved", "smooth", 4.0, "pan", None),
    "big_stripes2_hdr":   (300, 200, "vstripes:2+miss:0.02", "ripple", "smooth", 1000.0, None, None),
    "extreme_ids":        (65, 9, "extremes", "curved", "smooth", 4.0, "identity", None),
    "lights_30pc":        (63, 7, "hstripes:2+lights:0.3", "flat", "smooth", 4.0, None, None),
    "all_null":           (64, 8, "null", "flat", "smooth", 4.0, "identity", None),
    "constant_image":     (130, 70, "vstripes:16+miss:0.02", "curved", "constant", 4.0, "pan", None),
    "zero_image":         (63, 7, "one", "curved", "zero", 1.0, "identity", None),
    "plateaus":           (130, 70, "checker:17", "ripple", "plateaus", 4.0, "identity", None),
    "fireflies":          (130, 70, "one+miss:0.02", "curved", "fireflies", 4.0, "identity", None),
    "far_depth_1e4":      (65, 9, "vstripes:16", "far", "smooth", 4.0, "identity", None),
    "zero_normals":       (65, 9, "one", "zeronormal", "smooth", 4.0, "identity", None),
    "nonfinite_130x70":   (130, 70, "vstripes:16+miss:0.02", "curved", "nonfinite", 4.0, "identity",
                           "+Inf and NaN samples: float64 and float32 need not agree on which pixels they reach"),
    "nonfinite_64x8":     (64, 8, "one", "ripple", "nonfinite", 4.0, "pan",
                           "+Inf and NaN samples: float64 and float32 need not agree on which pixels they reach"),
}
NAMES = list(TABLE)
TOLERANCE_NAMES = [n for n in NAMES if TABLE[n][7] is None]
SVGF_NAMES = [n for n in NAMES if TABLE[n][6] is not None]
# cases that are structural-only for SpatioTemporalFilter alone (LeveledEAWFilter still compares them within its tolerance)
SVGF_STRUCTURAL = {
    "plateaus": "inside a plateau the variance E[l^2] - E[l]^2 is exactly 0 and float32 leaves cancellation noise of ~1e-7 S^2 in its place: "
                "the colour weight's denominator is 1e-4 in float64 and ~5e-3 in float32, and the weight of a tap across a plateau edge "
                "(exp(-|dl| / denominator), dl ~ 0.07) follows it -- the oracle itself is 130 .. 1100 units from float64",
    "fireflies": "a 1e4 S sample in the history: the variance E[l^2] - E[l]^2 next to it cancels two decades (float32 1.6407e6 for 1.6409e6), "
                 "and the colour weights of its neighbours carry that relative 1e-4 in exponents of ~7 -- the oracle is 0.6 .. 0.9 unit from float64",
}
SVGF_TOLERANCE_NAMES = [n for n in SVGF_NAMES if TABLE[n][7] is None and n not in SVGF_STRUCTURAL]

# LeveledEAWFilter sigma sets (sigLumin, sigNormal, sigDepth), one per division / multiplication instantiation of the kernel: bit 0 / 1 / 2
# of the index is set where sigLumin / sigNormal / sigDepth is a power of two.  Index 5 is the reference's default up to sigNormal .2.
EAW_SIGMAS = [(3.7, 0.2, 0.6), (64.0, 0.2, 0.6), (3.7, 0.25, 0.6), (64.0, 0.25, 0.6),
              (3.7, 0.2, 1.0), (64.0, 0.2, 1.0), (3.7, 0.25, 1.0), (64.0, 0.25, 1.0)]
EAW_FUSED = (0, 5, 7)               # the sets that also run with fused taps


def eaw_sigma_sets(name):
    """The sigma sets a case runs with: the default and two more, rotating through the table so that each is used by several cases."""
    k = NAMES.index(name)
    return sorted({5, k % 8, (3 * k + 2) % 8})


# SpatioTemporalFilter: (sigLumin, sigNormal, sigDepth, fused, tiled) -> the kernel rs_svgf_filter_rows dispatches to
SVGF_FORMS = [
    (4.0, 128.0, 1.0, True, True),        # k_svgf_wavelet_tiled<S, 7, true, true>   (the default)
    (4.0, 128.0, 1.0, False, True),       # k_svgf_wavelet_tiled<S, 7, true>
    (10.5, 128.0, 0.25, True, True),      # the tile with another power-of-two sigDepth and another sigLumin, fused
    (10.5, 128.0, 0.25, False, True),     # ... separately rounded
    (4.0, 128.0, 1.0, True, False),       # k_svgf_wavelet<7, true, true>
    (4.0, 128.0, 0.25, False, False),     # k_svgf_wavelet<7, true>
    (4.0, 128.0, 0.3, True, True),        # k_svgf_wavelet<7, false>   (no tile, no fused form without a power-of-two sigDepth)
    (4.0, 64.0, 1.0, False, True),        # k_svgf_wavelet<6, true>
    (10.5, 64.0, 0.3, True, False),       # k_svgf_wavelet<6, false>
    (4.0, 32.0, 0.25, True, True),        # k_svgf_wavelet<5, true>
    (4.0, 32.0, 0.3, False, False),       # k_svgf_wavelet<5, false>
    (4.0, 2.0, 1.0, True, True),          # k_svgf_wavelet<-1, true>   (powf)
    (4.0, 1.0, 0.3, False, True),         # k_svgf_wavelet<-1, false>
    (10.5, 100.0, 1.0, True, False),      # powf, sigNormal not a power of two
    (4.0, 0.5, 0.25, False, False),       # powf, a root
    (4.0, 7.3, 0.3, True, True),          # powf
]


def svgf_forms(name):
    """The forms a case runs with: the default one and two more, rotating so that every form is used by at least two cases."""
    k = SVGF_NAMES.index(name)
    if name == "pan_200x136":                 # the largest frame of the time axis: the default form and the separately rounded tile
        return [0, 1]
    return sorted({0, (2 * k + 1) % 16, (2 * k + 2) % 16})


class Case:
    pass


def camera(W, H):
    return ob.camera_update(get_scene("cornell").camera(W, H))


def _ids(spec, W, H, rng, x, y):
    parts = spec.split("+")
    kind, _, arg = parts[0].partition(":")
    p = int(arg) if arg else 0
    if kind == "one":
        ids = np.full((H, W), 5)
    elif kind == "vstripes":
        ids = 3 + (x // p) % 4
    elif kind == "hstripes":
        ids = 3 + (y // p) % 4
    elif kind == "checker":
        ids = 7 + ((x // p) + (y // p)) % 2
    elif kind == "tile_edges":                               # boundaries on x = 63 | 64 and y = 7 | 8: the edges of the 64 x 8 tile
        ids = 1 + (x >= 64) + 2 * (y >= 8)
    elif kind == "extremes":
        ids = np.where(x < W // 2, 0, 2 ** 31 - 1)
    elif kind == "null":
        ids = np.where((x + y) % 3 == 0, -2, -1)
    else:
        raise ValueError(spec)
    ids = ids.astype(np.int64)
    for extra in parts[1:]:
        k, _, a = extra.partition(":")
        if k in ("miss", "lights"):
            ids[rng.random((H, W)) < float(a)] = -1 if k == "miss" else -2
        elif k in ("blockmiss", "blocklights"):              # a block that covers whole tiles' corners, and one two pixels wide
            v = -1 if k == "blockmiss" else -2
            ids[H // 4:H // 2 + 3, W // 3:W // 3 + 40] = v
            ids[:, W - 9:W - 7] = v
        else:
            raise ValueError(spec)
    return ids.astype(np.int32)


def _tangent(n):
    t = np.cross(n, np.array([0.0, 1.0, 0.0]))
    return t / np.linalg.norm(t, axis=-1, keepdims=True)


def make(name):
    """The case's planes for its frames (one frame for a case without a time axis)."""
    W, H, idspec, geom, colour, scale, time, structural = TABLE[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    c = Case()
    c.name, c.W, c.H, c.structural, c.time = name, W, H, structural, time
    c.cam = camera(W, H)
    x = np.arange(W)[None, :] * np.ones((H, 1), np.int64)
    y = np.arange(H)[:, None] * np.ones((1, W), np.int64)
    ids = _ids(idspec, W, H, rng, x, y)
    # normals: the direction turns by 1 rad over 32 pixels, so that |dn|^2 / sigNormal runs from 0 to 5 within the reach of level 4
    th = (x / 32.0 + y / 45.0) if geom != "flat" else 0.0 * x
    n = np.stack([np.sin(th) * 0.8, 0.3 * np.cos(0.5 * th), -np.cos(th) * 0.8 - 0.3], -1)
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    if geom == "zeronormal":
        n[2:7, 20:50] = 0.0
    # depth: one pixel is 2 tan(fovY) / H wide at distance 1; d0 puts 32 pixels |dp| = sqrt(5) apart
    pitch = 2.0 * np.tan(np.radians(float(c.cam.fov[1]))) / H
    d0 = np.sqrt(5.0) / (32.0 * pitch)
    if geom == "far":
        depth = 1e4 + 0.0 * x
    elif geom == "ripple":
        depth = d0 * (0.6 + 0.004 * x + 0.003 * y) + 0.05 * np.sin(x * 0.7) * np.cos(y * 0.4)
    elif geom == "depthstep":
        depth = d0 * (0.7 + 0.002 * x) + 1.5 * (x >= W // 2)
    else:
        depth = d0 * (0.8 + 0.002 * y) + 0.0 * x
    albedo = np.stack([0.3 + 0.5 * np.sin(x * 0.2) ** 2, 0.5 + 0.0 * x, 0.9 * np.cos(y * 0.1) ** 2], -1)

    def colour_of(frame):
        if colour == "zero":
            return np.zeros((H, W, 3))
        if colour == "constant":
            return np.ones((H, W, 3)) * np.array([0.7, 1.1, 0.4]) * scale
        base = 1.0 + 0.6 * np.stack([np.sin(x * .11 + y * .05), np.cos(x * .07 - y * .13), np.sin(x * .03 + 2.0)], -1)
        if colour == "plateaus":                                   # piecewise constant, the same every frame: zero variance inside
            return np.round(base * 2.0) / 2.0 * scale * 0.5
        col = scale * 0.5 * (base + 0.5 * rng.random((H, W, 3)))   # fresh noise every frame, as a renderer's samples
        if colour == "fireflies":
            for k in range(max(1, W * H // 400)):
                col[rng.integers(H), rng.integers(W)] = 1e4 * scale
        if colour == "nonfinite":
            for k in range(max(2, W * H // 600)):
                col[rng.integers(H), rng.integers(W), rng.integers(3)] = np.inf if k % 2 == 0 else np.nan
        return col

    c.frames = []
    prev_ids, prev_n = ids, n
    for f in range(FRAMES if time else 1):
        fr = Case()
        fr.ids = ids.copy(); fr.normal = n.copy(); fr.depth = depth.copy(); fr.albedo = albedo
        fr.motion = (y * W + x).astype(np.int32)
        fr.last_ids, fr.last_normal = prev_ids.copy(), prev_n.copy()
        if time == "pan":                                          # the image moves by (+3, +2) pixels per frame: -1 where its source left the frame
            sx, sy = x - 3, y - 2                                  # the last frame's planes: every source pixel carries its target's id and normal
            fr.motion = np.where((sx >= 0) & (sy >= 0), sy * W + sx, -1).astype(np.int32)
            src = fr.motion.reshape(-1)
            ok = src >= 0
            fr.last_ids = np.full(H * W, -1, np.int32); fr.last_ids[src[ok]] = fr.ids.reshape(-1)[ok]
            fr.last_ids = fr.last_ids.reshape(H, W)
            ln = np.tile(np.array([0.0, 0.0, -1.0]), (H * W, 1)); ln[src[ok]] = fr.normal.reshape(-1, 3)[ok]
            fr.last_normal = ln.reshape(H, W, 3)
        elif time == "idchange" and f in (2, 5):                   # another id under a band of pixels for one frame
            fr.ids[:, W // 4:W // 2] = np.where(fr.ids[:, W // 4:W // 2] > -1, 42, fr.ids[:, W // 4:W // 2])
        elif time == "normals" and f >= 1:                         # last normals at |n . n_last| = 0, .05, .5, 1 by quarter of the width
            v = np.choose(np.minimum(x * 4 // max(W, 4), 3), [0.0, 0.05, 0.5, 1.0])[..., None]
            fr.last_normal = v * n + np.sqrt(1.0 - v * v) * _tangent(n)
        elif time == "nullflip" and f in (1, 2, 4):                # hits that become null for a frame or two and come back
            fr.ids[2:6, 10:30] = -1 if f != 4 else -2
        for k in ("normal", "depth", "albedo", "last_normal"):
            setattr(fr, k, np.ascontiguousarray(getattr(fr, k), np.float32))
        fr.color = np.ascontiguousarray(colour_of(f), np.float32)
        c.frames.append(fr)
        prev_ids, prev_n = fr.ids, fr.normal.astype(np.float64)
    # the radiance scale of the tolerances: colour is homogeneous of degree 1 in the radiance, variance of degree 2
    lum = np.concatenate([(fr.color.reshape(-1, 3) @ LUM32) for fr in c.frames])
    lum = lum[np.isfinite(lum)]
    c.scale = max(1.0, float(lum.max())) if lum.size else 1.0
    return c


_cache = {}


def get(name):
    if name not in _cache:
        _cache[name] = make(name)
    return _cache[name]


def load_oracle(g, fr):
    """One frame's planes into an ob.GBuffer: the current set, the last set, motion and albedo."""
    cur = g.frame_idx
    g.prim_id[cur][:] = fr.ids.reshape(-1); g.prim_id[cur ^ 1][:] = fr.last_ids.reshape(-1)
    g.normal[cur][:] = fr.normal.reshape(-1, 3); g.normal[cur ^ 1][:] = fr.last_normal.reshape(-1, 3)
    g.depth[cur][:] = fr.depth.reshape(-1); g.depth[cur ^ 1][:] = fr.depth.reshape(-1)
    g.motion[:] = fr.motion.reshape(-1)
    g.albedo[:] = fr.albedo.reshape(-1, 3)


def load_device(hip, gbuf, fr):
    """The same into the library's G-buffer, through the device pointers of rs_gbuffer_get_view (fetched anew: they move with
    rs_gbuffer_update).  Returns the uploaded tensors' owner list only to keep the copies ordered; the planes own their memory."""
    import torch
    v = gbuf.view()
    cur = v.frameIdx

    def put(ptr, a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        hip.hip_memcpy_d2d(ptr, t.data_ptr(), t.numel() * t.element_size())

    put(v.devPrimId[cur], fr.ids.reshape(-1)); put(v.devPrimId[cur ^ 1], fr.last_ids.reshape(-1))
    put(v.devNormal[cur], fr.normal.reshape(-1)); put(v.devNormal[cur ^ 1], fr.last_normal.reshape(-1))
    put(v.devDepth[cur], fr.depth.reshape(-1)); put(v.devDepth[cur ^ 1], fr.depth.reshape(-1))
    put(v.devMotion, fr.motion.reshape(-1)); put(v.devAlbedo, fr.albedo.reshape(-1))


def units(got, ref64, rtol, atol):
    """|got - ref| / (atol + rtol |ref|), the error in units of a stated tolerance; every element, nothing masked."""
    ref64 = np.asarray(ref64, np.float64)
    return np.abs(np.asarray(got, np.float64).reshape(ref64.shape) - ref64) / (atol + rtol * np.abs(ref64))


# ---- the stated tolerances (include/restir_hip.h, tests/test_gpu_parity.py test_eaw_filter / test_svgf_filter) with the one scaling the
# filters' structure implies: colour is homogeneous of degree 1 in the radiance and variance of degree 2, so a case of scale S uses
# atol * S for colour planes and atol * S^2 for the variance plane; the moments plane holds (l, l^2, a count).  S = 1: the stated numbers.
EAW_TOL = (1e-5, 1e-6)
SVGF_COLOUR_TOL = (3e-5, 2e-6)
SVGF_VARIANCE_TOL = (3e-5, 1e-6)
SVGF_MOMENT_TOL = (1e-6, 1e-7)


def eaw_units(got, ref64, S):
    return units(got, ref64, EAW_TOL[0], EAW_TOL[1] * S)


def svgf_units(plane, got, ref64, S):
    """plane: 'colour' (filtered colour, colour history) | 'variance' | 'moment' ((n, 3): first moment, second moment, count)."""
    if plane == "colour":
        return units(got, ref64, SVGF_COLOUR_TOL[0], SVGF_COLOUR_TOL[1] * S)
    if plane == "variance":
        return units(got, ref64, SVGF_VARIANCE_TOL[0], SVGF_VARIANCE_TOL[1] * S * S)
    atol = SVGF_MOMENT_TOL[1] * np.array([S, S * S, 1.0])
    return units(got, np.asarray(ref64).reshape(-1, 3), SVGF_MOMENT_TOL[0], atol)


_ref_cache = {}


def eaw_reference(name, sigma):
    """The float64 five-level filter of the case's first frame: ((n, 3) image, decisions)."""
    from tests import denoise_reference as ref
    key = ("eaw", name, tuple(np.float32(s) for s in sigma))
    if key not in _ref_cache:
        c = get(name); fr = c.frames[0]
        img, d = ref.eaw_filter(fr.ids, fr.normal, ref.positions(c.cam, fr.depth), fr.color, *sigma)
        _ref_cache[key] = (img.reshape(-1, 3), d)
    return _ref_cache[key]


def svgf_reference(name, sigma):
    """The float64 SpatioTemporalFilter over the case's frames: a list of dict(filtered, variance, accum_color, accum_moment, decisions)."""
    from tests import denoise_reference as ref
    key = ("svgf", name, tuple(np.float32(s) for s in sigma))
    if key not in _ref_cache:
        c = get(name)
        f = ref.SVGF(c.W, c.H, *sigma)
        out = []
        for fr in c.frames:
            img = f.filter(fr.color, fr.ids, fr.normal, fr.depth, fr.motion, fr.last_ids, fr.last_normal, c.cam)
            out.append(dict(filtered=img.reshape(-1, 3), variance=f.variance.reshape(-1), accum_color=f.accum_color[f.frame_idx].reshape(-1, 3),
                            accum_moment=f.accum_moment[f.frame_idx].reshape(-1, 3), decisions=f.decisions, frame_idx=f.frame_idx))
            f.next_frame()
        _ref_cache[key] = out
    return _ref_cache[key]


def oracle_svgf(name, sigma):
    """The C oracle's SpatioTemporalFilter over the case's frames, same layout, with the oracle's branch log."""
    c = get(name)
    g = ob.GBuffer(c.W, c.H)
    f = ob.SVGF(c.W, c.H)
    f.set_params(*sigma)
    out = []
    for fr in c.frames:
        load_oracle(g, fr)
        img = f.filter(fr.color.reshape(-1, 3), g, c.cam).copy()
        st = f.state()
        out.append(dict(filtered=img, variance=st["variance"], accum_color=st["accum_color"], accum_moment=st["accum_moment"], branches=f.branches()))
        f.next_frame()
    return out


def oracle_eaw(name, sigma):
    c = get(name)
    g = ob.GBuffer(c.W, c.H)
    load_oracle(g, c.frames[0])
    return ob.eaw_filter_with(g, c.cam, c.frames[0].color.reshape(-1, 3), *sigma).copy()
