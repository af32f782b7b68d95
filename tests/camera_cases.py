"""The camera at its extremes: a table of named cameras on the untouched Cornell box, the oracle's outputs for each and the figures that
make a row non-vacuous.  The third of a frame's inputs beside materials and lights (tests/extreme_cases.py) and geometry
(tests/geometric_cases.py).

Every other parity module renders fov_y 10 - 30 degrees, focal_dist 1, a camera 0.1 - 55 units in front of the geometry and frames at
least 48 pixels wide.  What reads CamParams (restir_amd/csrc/rs_scene.h) -- camera_center_ray in the G-buffer pass, camera_sample in the
primary-ray kernels, the path tracers and ReSTIR-GI, camera_raster_coord behind the motion plane, cut_cell of the primary cuts
(rs_cuts.h) -- has therefore never run where the tangent is huge, zero or negative (rs_make_cam_params takes tanf(radians(fov_y)) of the
WHOLE angle: fov_y = 90 gives -2.29e7, 91 gives -57.3), where all rays of a frame are parallel, where the unnormalised direction
overflows or where the frame is one pixel wide.

A case is a name and a dict merged into get_scene("cornell").camera_args; nothing else of the scene changes.  The rules -- the call
sequence `run`, the two back ends' interface, `compare` / `same_bits_or_nan`, the libm mode -- are tests/extreme_cases.py's and are used
from there.  `oracle_outputs(name, size)` is computed once per row and size and shared; `EXPECT[name]` are the oracle's figures at 48 x 32
(tests/test_camera_cases.py asserts them on the oracle alone).

PAIRS is the second table: two frames at camera A, then two at camera B, with spatiotemporal reuse -- what the motion plane and the
temporal pass do when the camera that reprojects (the LAST one, camera_raster_coord) and the camera that renders differ.
"""
import functools

import numpy as np

from oracle import binding as ob
from tests import extreme_cases as xc
from tests.common import get_scene

SIZE = xc.SIZE                      # 48 x 32
SMALL_SIZES = ((97, 61), (1, 33), (130, 1), (2, 2))      # partial tiles; aspects of 1 / 33, 130 and 1
INSIDE = dict(position=(0.0, 1.0, 0.9))                 # inside the box: every pixel hits, even through a wide lens


def _inside(**args):
    return dict(INSIDE, **args)


# name: (camera arguments over the box's own -- position (0, 1, 3.5), rotation (-90, 0, 0), fov_y 19.5, focal_dist 1 --, what the row drives)
TABLE = {
    "fov_0":        (dict(fov_y=0.0), "tan = 0: every ray of the frame is the view direction; camera_raster_coord divides by aspect * tan = 0"),
    "fov_1e-3":     (dict(fov_y=1e-3), "tan = 1.7e-5: rays that differ in their last bits"),
    "in_fov_60":    (_inside(fov_y=60.0), "tan(60 deg) = 1.73: a half angle of 60"),
    "in_fov_83.6":  (_inside(fov_y=83.6), "tan = 8.92: aspect * tan just under the cuts' bound of 16 at aspects 1.5 and 16 / 9"),
    "in_fov_86.5":  (_inside(fov_y=86.5), "tan = 16.35: past the cuts' bound"),
    "in_fov_89.99": (_inside(fov_y=89.99), "tan = 5727"),
    "in_fov_90":    (_inside(fov_y=90.0), "tan of the float right angle = -2.29e7: the image plane nearly edge-on, and mirrored"),
    "in_fov_91":    (_inside(fov_y=91.0), "tan = -57.3: negative and far above the cuts' bound in magnitude"),
    "in_fov_120":   (_inside(fov_y=120.0), "tan = -1.73: in_fov_60 mirrored in both screen axes"),
    "in_fov_-60":   (_inside(fov_y=-60.0), "a negative angle: tan = -1.73 again, by another route"),
    "fov_neg":      (dict(fov_y=-19.5), "the box's own view mirrored"),
    "pitch_90":     (dict(rotation=(-90.0, 90.0, 0.0), position=(0.0, 0.2, 0.0)), "straight up: cosf of the float right angle is -4.4e-8, a basis made of roundings"),
    "pitch_-90":    (dict(rotation=(-90.0, -90.0, 0.0), position=(0.0, 1.8, 0.0)), "straight down"),
    "yaw_0":        (dict(rotation=(0.0, 0.0, 0.0), position=(-0.9, 1.0, 0.0)), "view (1, 0, 0) exactly"),
    "yaw_180":      (dict(rotation=(180.0, 0.0, 0.0), position=(0.9, 1.0, 0.0)), "view (-1, 8.7e-8 ..): sinf of the float straight angle"),
    "far_1e4":      (dict(position=(0.0, 1.0, 1e4), fov_y=0.006), "1e4 units away through a lens of 0.006 degrees: origins with 1e-3 of resolution"),
    "far_1e7":      (dict(position=(0.0, 1.0, 1e7), fov_y=6e-6), "1e7 units away: origins with a resolution of 1, slab distances of 1e7"),
    "focal_1e-20":  (dict(focal_dist=1e-20), "pFocus of 1e-20: the squared length 1e-40 is a denormal"),
    "focal_1e18":   (_inside(focal_dist=1e18), "pFocus of 1e18: the squared length 1e36 still a float"),
    "focal_neg":    (dict(focal_dist=-1.0, position=(0.0, 1.0, -3.5)), "a negative focal distance: the camera looks backwards, from behind the back wall"),
    "on_wall":      (dict(position=(-1.0, 1.0, 0.5), rotation=(-40.0, 0.0, 0.0)), "the origin in the left wall's plane"),
    "at_vertex":    (dict(position=(1.0, 0.0, 1.0), rotation=(-135.0, 20.0, 0.0), fov_y=30.0), "the origin at a corner of the box"),
    "looking_away": (dict(rotation=(90.0, 0.0, 0.0)), "no ray meets the root box: every wave leaves at the root"),
    "focal_1e20":   (_inside(focal_dist=1e20), "the squared length 1e40 overflows: normalize gives 0 and NaN direction components"),
}
NAMES = list(TABLE)
WIDE = [n for n in NAMES if n.startswith("in_fov_")]
RESIZED = ("in_fov_60", "in_fov_91")              # the rows that run again at SMALL_SIZES
STILL = ("in_fov_60", "in_fov_83.6", "in_fov_120", "fov_1e-3", "far_1e4", "far_1e7", "focal_1e18", "focal_neg")
# Rows that the GPU module leaves to the oracle: none.  (focal_1e20's directions are not finite; why the device walks may see them is in
# tests/test_gpu_camera_extremes.py.)
CPU_ONLY = ()


def camera_args(name):
    return dict(get_scene("cornell").camera_args, **TABLE[name][0])


@functools.lru_cache(maxsize=None)
def _box():
    return get_scene("cornell")


def with_camera(args, sd=None):
    """The Cornell box (or `sd`) under camera `args` (merged into its own): a shallow copy, the arrays shared -- nobody writes to them."""
    import copy
    sd = copy.copy(sd or _box())
    sd.camera_args = dict(sd.camera_args, **args)
    return sd


def scene(name):
    return with_camera(TABLE[name][0])


@functools.lru_cache(maxsize=None)
def _oracle_outputs(name, size, stages):
    assert xc._correctly_rounded, "oracle_outputs: inside extreme_cases.correctly_rounded_libm() only"
    return xc.run(xc.OracleBackend(scene(name), size), stages)


def oracle_outputs(name, size=SIZE, stages=xc.STAGES):
    """The oracle's outputs of `stages`, computed once and shared: nobody writes to them."""
    return _oracle_outputs(name, tuple(size), tuple(stages))


# ---- figures ------------------------------------------------------------------------------------------------------------------------
def motion_mix(motion):
    """(entries that are the pixel's own index, entries of -1, the rest) of a motion plane.  (A miss writes 0.)"""
    m = np.asarray(motion).reshape(-1)
    own = int(np.count_nonzero(m == np.arange(len(m))))
    gone = int(np.count_nonzero(m == -1))
    return own, gone, len(m) - own - gone


def hit_mix(prim_id):
    """(surface hits, lights, misses) of a G-buffer id plane: a material id, -2 for a light, -1 for a miss."""
    p = np.asarray(prim_id).reshape(-1)
    return int(np.count_nonzero(p >= 0)), int(np.count_nonzero(p == -2)), int(np.count_nonzero(p == -1))


def figures(o):
    return dict(hits=hit_mix(o["direct3/gbuffer/prim_id"]), live=xc.live(o["direct3/f2/res"]), motion=motion_mix(o["direct3/gbuffer/motion"]),
                live0=xc.live(o["direct0/f1/res"]), gi_live=xc.live(o["gi/f2/res"]), pt4_rays=o["pt4/rays"], nan=xc.nan_counts(o), inf=xc.inf_counts(o))


# What the oracle gives at 48 x 32 in libm mode 1: (surface hits, lights, misses) of the G-buffer; live reservoirs after the third
# spatiotemporal frame; the motion plane of that frame -- a STILL camera's -- as (identity, -1, elsewhere); live reservoirs after the
# second RIS-only and the third ReSTIR-GI frame; rays of pathTrace at depth 4; every output that holds a NaN or an infinity, with its
# count: none in any row.  The oracle is deterministic, so the counts are exact.
EXPECT = {
    "fov_0":         dict(hits=(1536, 0, 0), live=1536, motion=(0, 1536, 0), live0=1536, gi_live=1154, pt4_rays=11790),
    "fov_1e-3":      dict(hits=(1536, 0, 0), live=1536, motion=(1536, 0, 0), live0=1536, gi_live=1510, pt4_rays=11790),
    "in_fov_60":     dict(hits=(1503, 32, 1), live=1223, motion=(1535, 0, 1), live0=1184, gi_live=1411, pt4_rays=9802),
    "in_fov_83.6":   dict(hits=(1533, 2, 1), live=1209, motion=(1535, 0, 1), live0=1173, gi_live=1345, pt4_rays=9078),
    "in_fov_86.5":   dict(hits=(1533, 0, 3), live=1241, motion=(1533, 0, 3), live0=1204, gi_live=1324, pt4_rays=8858),
    "in_fov_89.99":  dict(hits=(1530, 0, 6), live=1282, motion=(1530, 0, 6), live0=1242, gi_live=1283, pt4_rays=8452),
    "in_fov_90":     dict(hits=(1533, 0, 3), live=1307, motion=(109, 177, 1250), live0=1244, gi_live=1144, pt4_rays=8614),
    "in_fov_91":     dict(hits=(1532, 0, 4), live=1278, motion=(1532, 0, 4), live0=1231, gi_live=1297, pt4_rays=8712),
    "in_fov_120":    dict(hits=(1503, 32, 1), live=1221, motion=(1535, 0, 1), live0=1172, gi_live=1387, pt4_rays=10064),
    "in_fov_-60":    dict(hits=(1503, 32, 1), live=1221, motion=(1535, 0, 1), live0=1172, gi_live=1387, pt4_rays=10064),
    "fov_neg":       dict(hits=(1138, 12, 386), live=866, motion=(1151, 0, 385), live0=819, gi_live=1031, pt4_rays=8100),
    "pitch_90":      dict(hits=(1392, 144, 0), live=422, motion=(1536, 0, 0), live0=409, gi_live=1341, pt4_rays=9466),
    "pitch_-90":     dict(hits=(1536, 0, 0), live=1534, motion=(1536, 0, 0), live0=1491, gi_live=1471, pt4_rays=10856),
    "yaw_0":         dict(hits=(1536, 0, 0), live=639, motion=(1536, 0, 0), live0=627, gi_live=1466, pt4_rays=10608),
    "yaw_180":       dict(hits=(1536, 0, 0), live=1535, motion=(1536, 0, 0), live0=1516, gi_live=1423, pt4_rays=10320),
    "far_1e4":       dict(hits=(900, 0, 636), live=834, motion=(901, 0, 635), live0=790, gi_live=869, pt4_rays=7800),
    "far_1e7":       dict(hits=(930, 0, 606), live=825, motion=(931, 0, 605), live0=781, gi_live=887, pt4_rays=7892),
    "focal_1e-20":   dict(hits=(1138, 12, 386), live=860, motion=(1151, 0, 385), live0=826, gi_live=1033, pt4_rays=7994),
    "focal_1e18":    dict(hits=(1536, 0, 0), live=1536, motion=(1536, 0, 0), live0=1535, gi_live=1446, pt4_rays=10284),
    "focal_neg":     dict(hits=(1152, 0, 384), live=0, motion=(1153, 0, 383), live0=0, gi_live=0, pt4_rays=3854),
    "on_wall":       dict(hits=(1536, 0, 0), live=1059, motion=(1536, 0, 0), live0=1045, gi_live=1479, pt4_rays=10730),
    "at_vertex":     dict(hits=(1210, 2, 324), live=649, motion=(1213, 0, 323), live0=618, gi_live=1104, pt4_rays=8764),
    "looking_away":  dict(hits=(0, 0, 1536), live=0, motion=(1, 0, 1535), live0=0, gi_live=0, pt4_rays=1536),
    "focal_1e20":    dict(hits=(0, 0, 1536), live=0, motion=(1, 0, 1535), live0=0, gi_live=0, pt4_rays=1536),
}


def expected(name):
    return dict(dict(nan={}, inf={}), **EXPECT[name])


# ---- moving pairs -------------------------------------------------------------------------------------------------------------------
MOVED = dict(position=(0.1, 1.05, 0.9))
# name: (camera A, camera B -- both over INSIDE --, what the pair drives)
PAIRS = {
    "pan_small":     (dict(), MOVED, "a small move: nearly every pixel reprojects to another one"),
    "fov_91_pan":    (dict(fov_y=91.0), dict(MOVED, fov_y=91.0), "the same move under a tangent of -57.3"),
    "zoom_in_to_60": (dict(), dict(fov_y=60.0), "19.5 -> 60 degrees: most of the new frame lies outside the last one"),
    "zoom_from_0":   (dict(fov_y=0.0), dict(), "0 -> 19.5: every reprojection divides by zero in the LAST camera"),
    "zoom_to_0":     (dict(), dict(fov_y=0.0), "19.5 -> 0: every pixel sees the same point"),
    "turn_90":       (dict(), dict(rotation=(0.0, 0.0, 0.0)), "a quarter turn: the last frame saw another wall"),
    "turn_10":       (dict(), dict(rotation=(-80.0, 0.0, 0.0)), "ten degrees: the turn whose reprojections land on what the last frame saw"),
}
PAIR_NAMES = list(PAIRS)
GI_PAIRS = ("pan_small", "fov_91_pan", "turn_90", "turn_10")
PAIR_FRAMES = 4
CANDIDATES = {"direct": 32, "gi": 1}                 # what one frame alone puts into a reservoir (RESERVOIR_SIZE of restir.cu:3; one path)


def set_camera(cam, update, position=None, rotation=None, fov_y=None, focal_dist=None):
    """Writes a renderer's camera as OracleRenderer.set_camera_position does, and derives its basis with `update` (the side's camera_update)."""
    for field, v in (("position", position), ("rotation", rotation)):
        if v is not None:
            for i in range(3):
                getattr(cam, field)[i] = float(v[i])
    if fov_y is not None:
        cam.fov[1] = float(fov_y)
    if focal_dist is not None:
        cam.focalDist = float(focal_dist)
    update(cam)


def run_pair(be, name, kind="direct"):
    """Two frames at camera A, two at camera B on back end `be` (extreme_cases.OracleBackend or the GPU module's), whose scene carries
    camera A.  kind "direct": ReSTIRDirect with reuse 3; "gi": ReSTIRIndirect at depth 3 with temporal reuse.  After every frame: image,
    ray count, the `last` reservoirs and the motion plane, under flat keys."""
    b = _inside(**PAIRS[name][1])
    update = getattr(be, "hip", ob).camera_update
    r = be.renderer()
    out = {}

    def record(f, image, rays, res):
        out["f%d/image" % f], out["f%d/rays" % f], out["f%d/res" % f] = np.array(image), int(rays), res
        out["f%d/motion" % f] = be.gbuffer(r)["motion"]

    if kind == "gi":
        for f, (img, rays, res) in enumerate(be.gi_frames(r, PAIR_FRAMES, 3)):
            record(f, img, rays, res)
            if f == 1:                                # (the generator renders frame 2 only when asked for it: with camera B)
                set_camera(r.cam, update, **b)
        return out
    for f in range(PAIR_FRAMES):
        if f == 2:
            set_camera(r.cam, update, **b)
        image = r.frame(3)
        record(f, image, r.rays, be.last(r))
    return out


def pair_scene(name):
    return with_camera(_inside(**PAIRS[name][0]))


@functools.lru_cache(maxsize=None)
def oracle_pair(name, kind="direct", size=SIZE):
    assert xc._correctly_rounded, "oracle_pair: inside extreme_cases.correctly_rounded_libm() only"
    return run_pair(xc.OracleBackend(pair_scene(name), size), name, kind)


def merged_reprojected(o, kind="direct", f=2):
    """Pixels of frame f whose reservoir holds more samples than the frame's own candidates and whose motion entry points elsewhere:
    a reservoir of the last frame, fetched through the reprojection, was merged."""
    m = o["f%d/motion" % f].reshape(-1)
    moved = (m != -1) & (m != np.arange(len(m)))
    return int(np.count_nonzero(moved & (o["f%d/res" % f]["numSamples"] > CANDIDATES[kind])))


def pair_figures(o):
    return dict(motion=motion_mix(o["f2/motion"]), merged=merged_reprojected(o), live=xc.live(o["f3/res"]),
                nan=xc.nan_counts(o), inf=xc.inf_counts(o))


# The oracle's figures per pair at 48 x 32: the motion plane after the first frame at camera B as (identity, -1, elsewhere), pixels of
# that frame that merged a reprojected reservoir, live reservoirs after the last frame, NaN / infinity counts (none).
PAIR_EXPECT = {
    "pan_small":     dict(motion=(0, 50, 1486), merged=1366, live=1536),
    "fov_91_pan":    dict(motion=(97, 110, 1329), merged=1026, live=1260),
    "zoom_in_to_60": dict(motion=(0, 1475, 61), merged=60, live=1239),
    "zoom_from_0":   dict(motion=(0, 1536, 0), merged=0, live=1536),
    "zoom_to_0":     dict(motion=(1, 0, 1535), merged=1535, live=1536),
    "turn_90":       dict(motion=(1, 928, 607), merged=0, live=1536),
    "turn_10":       dict(motion=(0, 268, 1268), merged=1205, live=1536),
}
# ... and of the pairs that run again as ReSTIRIndirect: pixels of the first B frame that merged a reprojected reservoir
GI_PAIR_MERGED = {"pan_small": 1366, "fov_91_pan": 1026, "turn_90": 0, "turn_10": 1205}


# ---- the camera functions restated (NumPy, float32), for the mutation check of tests/test_camera_cases.py -----------------------------
F32 = np.float32


def _normalize(v):
    with np.errstate(all="ignore"):
        return (v * (F32(1) / np.sqrt((v * v).sum(-1, dtype=F32, keepdims=True), dtype=F32))).astype(F32)


def raster_coord(cam, pos, size, drop_half=False):
    """camera_raster_coord (rs_scene.h) of points `pos` (n, 3) for ctypes camera `cam`: the motion entry, or -1 outside the frame.
    drop_half: the mutant without the `ndc * .5 + .5` step.  A restatement for telling mutants apart, not a bit-exact one (NumPy sums
    in another order): the test compares it with itself."""
    W, H = size
    v = lambda n: np.array([getattr(cam, n)[i] for i in range(3)], F32)
    inv = np.array([cam.rotationMatInv[i] for i in range(9)], F32).reshape(3, 3)      # [column][row]
    tan = F32(np.tan(F32(np.radians(F32(cam.fov[1])))))
    aspect = F32(W) / F32(H)
    with np.errstate(all="ignore"):
        d = _normalize(pos.astype(F32) - v("position"))
        d = d * (F32(1) / (d * v("view")).sum(-1, dtype=F32, keepdims=True))
        p = d[:, 0:1] * inv[0] + d[:, 1:2] * inv[1] + d[:, 2:3] * inv[2]
        nx, ny = -(p[:, 0] / (aspect * tan)), -(p[:, 1] / tan)
        if not drop_half:
            nx, ny = nx * F32(.5) + F32(.5), ny * F32(.5) + F32(.5)
        fx, fy = F32(W) * nx, F32(H) * ny
        ok = np.isfinite(fx) & np.isfinite(fy) & (np.abs(fx) < 2e9) & (np.abs(fy) < 2e9)
        x, y = np.where(ok, fx, -1).astype(np.int64), np.where(ok, fy, -1).astype(np.int64)      # f2i truncates; what it makes of the rest lies outside the frame
    inside = ok & (x >= 0) & (x < W) & (y >= 0) & (y < H)
    return np.where(inside, y * W + x, -1)


def center_dirs(cam, size, swap_focus=False):
    """camera_center_ray's directions for every pixel.  swap_focus: the mutant whose pFocus multiplies (ruv * tan) * aspect -- the
    operands of the first product in another order, another rounding."""
    W, H = size
    v = lambda n: np.array([getattr(cam, n)[i] for i in range(3)], F32)
    tan = F32(np.tan(F32(np.radians(F32(cam.fov[1])))))
    aspect, focal = F32(W) / F32(H), F32(cam.focalDist)
    psx, psy = F32(1) / F32(W), F32(1) / F32(H)
    y, x = np.divmod(np.arange(W * H), W)
    ruvx = F32(1) - (x.astype(F32) * psx + psx * F32(.5)) * F32(2)
    ruvy = F32(1) - (y.astype(F32) * psy + psy * F32(.5)) * F32(2)
    with np.errstate(all="ignore"):
        X = ((ruvx * tan) * aspect if swap_focus else (ruvx * aspect) * tan) * focal
        Y = (ruvy * F32(1)) * tan * focal
        Z = np.full_like(X, focal)
        d = X[:, None] * v("right") + Y[:, None] * v("up") + Z[:, None] * v("view")
        return _normalize(d.astype(F32))
