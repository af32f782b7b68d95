"""Scenes at their geometric extremes: a table of named edits of a scene's GEOMETRY, the rays, segments and frames that go with each, the
oracle's answers and the figures that make a case non-vacuous.

Three walks carry most of every frame -- the shadow tree, the ordered closest-hit trees and the emissive tree -- and all three store
their boxes on one 16-bit grid over the scene's root box (restir_amd/csrc/rs_grid.h grid_box, occlusion_bvh.cpp
rs_quantize_occlusion_bvh, rs_walk.h GridRay / grid_reaches, scene.hip build_occlusion_side): planes pushed out by 2^-17 of the extent,
a 200-step apron below the root box whose base is rounded in float, a slow lane for rays that start more than 4 grid extents away and a
silent fall-back to the reference's tree when a box does not fit the 16 bits.  Every other module walks scenes centred near the origin,
a few units across, roughly cubic and far coarser than a grid step.  A case here is a name and a function that edits a fresh
get_scene(base), base = "cornell" (36 triangles) or "sponza:0.03" (7 864): moved far from the origin, onto the edge of the grid's apron and beyond it, scaled up
and down, stretched into a slab, squashed to one grid step, with triangles smaller than a grid cell, with exact duplicates, with slivers
and zero-area triangles, and edited into such places by rs_scene_set_triangles.  No scene generator changes.

Rules of every transform: applied in float64 and rounded once to float32; the camera position goes through the same map (rotation and
field of view stay; vertex normals and texture coordinates stay as well: they shade, the walks never read them); appended triangles copy
normals, texture coordinates and material of an existing triangle; every vertex is finite; no uniform scale exceeds 2^20.

`case(name, base)` builds a case once (nobody writes to it): the scene, the rays and segments (the generators of tests/ray_cases.py at
4 133, seeds 34 and 36, plus the case's aimed ones, all shuffled so that each wave mixes kinds) and the ids of its special triangles.
`oracle_hits`, `oracle_occlusion` and `oracle_frames` are the oracle's answers, computed once and shared.  `grid_of` restates the grid of
rs_quantize_occlusion_bvh in NumPy and asks tests/refit_tables.grid_box whether every leaf box and the root fit.  `EXPECT[name, base]`
holds the figures (tests/test_geometric_cases.py asserts them on the oracle alone; tests/test_gpu_geometric_extremes.py holds the
library to the oracle on the same inputs, bit for bit)."""
import copy
import functools

import numpy as np

from oracle import binding as ob
from tests import extreme_cases as xc
from tests import refit_tables as rt
from tests.common import OracleRenderer, get_scene, oracle_scene
from tests.geometry_edits import apply_triangles, movable, rebuilt_oracle_scene
from tests.ray_cases import _shadow_like_segments, closest_like_rays

F32, F64 = np.float32, np.float64
LIGHT = 4
BASES = ("cornell", "sponza:0.03")
N_GENERATED, N_AIMED = 4133, 2048          # 64 full waves and a partial one; the aimed rays of a case
SIZE, RAGGED = (48, 32), (97, 61)          # frames: whole tiles of 32 x 8, and partial tiles
CLUSTER_AT = (0.61, 0.37, 0.43)            # where in the root box the sub-cell cluster sits
GRID_STEPS = 65000.0                       # rs_quantize_occlusion_bvh: scale = extent / 65000
MIN_COVERAGE, MIN_HITS, MIN_REACH = 0.3, 0.3, 0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------------------------------
def root_box64(sd):
    v = sd.vertices.reshape(-1, 3).astype(F64)
    return v.min(0), v.max(0)


def _affine(sd, scale=(1.0, 1.0, 1.0), shift=(0.0, 0.0, 0.0)):
    """x -> x * scale + shift on every vertex and on the camera position, in float64, rounded once."""
    s, t = np.asarray(scale, F64), np.asarray(shift, F64)
    assert len(set(s)) > 1 or s[0] <= 2.0 ** 20
    sd.vertices = np.ascontiguousarray((sd.vertices.astype(F64) * s + t).astype(F32))
    p = (np.asarray(sd.camera_args["position"], F64) * s + t).astype(F32)
    sd.camera_args = dict(sd.camera_args, position=tuple(float(x) for x in p))


def _append(sd, verts, like):
    """More triangles: `verts` (k, 3, 3) float64, rounded once; triangle j takes normals, texcoords and material of triangle like[j]."""
    verts = np.asarray(verts, F64).reshape(-1, 3, 3).astype(F32)
    like = np.broadcast_to(np.asarray(like, np.int64), (len(verts),))
    first = sd.num_prims
    sd.vertices = np.ascontiguousarray(np.concatenate([sd.vertices, verts]))
    sd.normals = np.ascontiguousarray(np.concatenate([sd.normals, sd.normals[like]]))
    sd.texcoords = np.ascontiguousarray(np.concatenate([sd.texcoords, sd.texcoords[like]]))
    sd.material_ids = np.ascontiguousarray(np.concatenate([sd.material_ids, sd.material_ids[like]]))
    return np.arange(first, first + len(verts))


def _emissive(sd):
    return np.nonzero(sd.materials["type"][sd.material_ids] == LIGHT)[0]


def _unit(d):
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _aimed(rng, sd, tris, k, lo=0.2, hi=0.4, min_cos=0.2):
    """k rays and k segments aimed at points well inside triangles drawn from `tris` ((m, 3, 3) float64; both free barycentrics in
    [lo, hi]): from an origin in the middle 40 % of the root box (rounded to float32 first, so that the direction is the one from the
    origin the walk sees), the segment ending half its length beyond the point.  Pairs of origin and triangle that meet at a grazing
    angle (|cos| below min_cos against the triangle's float64 normal) are drawn again: an aimed ray is meant to hit."""
    blo, bhi = root_box64(sd)
    rays, segs = np.zeros((0, 6), F32), np.zeros((0, 6), F32)
    while len(rays) < k:
        t = tris[rng.integers(0, len(tris), k)]
        u = rng.uniform(lo, hi, (k, 2))
        p = t[:, 0] * (1 - u.sum(1))[:, None] + t[:, 1] * u[:, :1] + t[:, 2] * u[:, 1:]
        o = rng.uniform(blo + 0.3 * (bhi - blo), blo + 0.7 * (bhi - blo), (k, 3)).astype(F32).astype(F64)
        d = _unit(p - o)
        with np.errstate(invalid="ignore", divide="ignore"):
            n = _unit(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]))
            keep = np.abs(np.einsum("ij,ij->i", n, d)) >= min_cos          # (False where the normal is NaN)
        rays = np.concatenate([rays, np.concatenate([o, d], 1)[keep].astype(F32)])
        segs = np.concatenate([segs, np.concatenate([o, o + 1.5 * (p - o)], 1)[keep].astype(F32)])
    return np.ascontiguousarray(rays[:k]), np.ascontiguousarray(segs[:k])


def cluster_vertices(rng, lo, hi, count):
    """`count` triangles whose vertices lie within +-(grid step) / 8 of the point CLUSTER_AT of the box lo .. hi (float64)."""
    step = (hi - lo).max() / GRID_STEPS
    return lo + np.asarray(CLUSTER_AT) * (hi - lo) + rng.uniform(-step / 8, step / 8, (count, 3, 3))


def corner_triangles(lo, hi):
    """8 triangles whose vertices are corners of the box exactly: corner j and the two corners across a face diagonal from it."""
    c = np.array([[(lo, hi)[(j >> k) & 1][k] for k in range(3)] for j in range(8)], F32)
    return np.stack([c[[j, j ^ 3, j ^ 5]] for j in range(8)])


class Case:
    """What the builders fill in: sd (the scene as created), special ({kind: triangle ids}), aimed rays and segments, and for the edited
    case the edit (ids, vertices) that follows creation."""

    def __init__(self, name, base):
        self.name, self.base, self.sd = name, base, get_scene(base)
        self.sd.materials = self.sd.materials.copy()
        self.n0 = self.sd.num_prims
        self.special, self.aimed, self.edit, self.notes = {}, None, None, {}


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------
TINY_SCALE = 2.0 ** -11            # see _tiny: the oracle hits 0.7718 (cornell) and 0.8103 (sponza) of the rays there, 0.661 and 0.2458 at 2^-12, none at 2^-13
SLIVER_WIDTH = 2.0 ** -22          # of the extent; see _needles


def _far(c):
    _affine(c.sd, shift=(1e4, -3e4, 2e4))


BEYOND_GRID_SHIFT = {"cornell": 1e6, "sponza:0.03": 1.6e7}


def _beyond_grid(c):
    """A translation along x that loses the apron: `base = lo - 200 * scale` rounds back to lo as soon as one ulp of the coordinate
    exceeds the 200 steps.  Those are 0.006 for cornell, whose ulp at 1e6 is 1 / 16.  The Sponza-class scene's are 0.12, two ulps at
    1e6 (it keeps its grid there: `apron_of_two_ulps`), so it goes to 1.6e7, where one ulp is 1."""
    _affine(c.sd, shift=(BEYOND_GRID_SHIFT[c.base], 0.0, 0.0))


def _apron_of_two_ulps(c):
    _affine(c.sd, shift=(1e6, 0.0, 0.0))


def _huge(c):
    _affine(c.sd, scale=(2.0 ** 20,) * 3)


def _tiny(c):
    """The reference stops finding triangles when the scene is small (its triangle test has absolute epsilons): TINY_SCALE is the
    smallest power of two at which the oracle still hits at least 30 % of closest_like_rays on both bases, found by halving from 1
    (tests/test_geometric_cases.py test_tiny_is_the_smallest_scale_the_reference_renders repeats the search)."""
    _affine(c.sd, scale=(TINY_SCALE,) * 3)


def _slab(c):
    _affine(c.sd, scale=(1024.0, 1.0, 1.0))


def _squashed(c):
    _affine(c.sd, scale=(1.0, 2.0 ** -16, 1.0))


def _sub_cell(c):
    sd = c.sd
    _affine(sd, scale=(2.0 ** 16,) * 3)
    rng = np.random.default_rng(41)
    lo, hi = root_box64(sd)
    v = cluster_vertices(rng, lo, hi, 64)
    plain, lamps = movable(sd), _emissive(sd)
    ids = _append(sd, v, np.concatenate([np.full(32, plain[0]), np.full(32, lamps[0])]))
    c.special = dict(cluster=ids, cluster_lights=ids[32:])
    c.aimed = _aimed(rng, sd, sd.vertices[ids].astype(F64), N_AIMED)


def _coincident(c):
    sd = c.sd
    rng = np.random.default_rng(42)
    pick = np.sort(rng.choice(c.n0, min(64, c.n0), replace=False))
    ids = _append(sd, sd.vertices[pick].astype(F64), pick)
    assert np.array_equal(sd.vertices[ids], sd.vertices[pick])
    c.special = dict(copies=ids, originals=pick)
    c.aimed = _aimed(rng, sd, sd.vertices[pick].astype(F64), N_AIMED)


def _needles(c):
    """32 slivers as long as the extent and SLIVER_WIDTH * extent wide at one end (a point at the other), running through the interior
    along the longest axis with a tilt, so that their boxes are fat; 8 triangles without area (4 single points, 4 with collinear
    vertices); rays aimed at points of the slivers' wide halves."""
    sd = c.sd
    rng = np.random.default_rng(43)
    lo, hi = root_box64(sd)
    size = hi - lo
    ext, main = size.max(), int(np.argmax(size))
    others = [k for k in range(3) if k != main]
    u = np.zeros((32, 3)); u[:, main] = 1.0
    u[:, others] = rng.uniform(-0.2, 0.2, (32, 2)) * size[others] / ext
    u = _unit(u)
    mid = (lo + hi) / 2 + rng.uniform(-0.3, 0.3, (32, 3)) * size
    mid[:, main] = (lo[main] + hi[main]) / 2
    a, b = mid - 0.5 * ext * u, mid + 0.5 * ext * u
    side = _unit(np.cross(u, rng.normal(size=(32, 3))))
    slivers = np.stack([a, a + SLIVER_WIDTH * ext * side, b], 1)
    plain = movable(sd)
    s_ids = _append(sd, slivers, plain[0])
    p = np.round((lo + rng.uniform(0.3, 0.7, (8, 3)) * size) * 1024) / 1024        # multiples of 2^-10: p, p + e, p + 2 e are exact in
    e = np.round(rng.uniform(0.02, 0.1, (8, 3)) * size * 1024) / 1024              # float32, so the collinear ones are collinear exactly
    flat = np.stack([p, p, p], 1)
    flat[4:] = np.stack([p[4:], p[4:] + e[4:], p[4:] + 2 * e[4:]], 1)
    z_ids = _append(sd, flat, plain[0])
    c.special = dict(slivers=s_ids, zero_area=z_ids)
    c.aimed = _aimed(rng, sd, sd.vertices[s_ids].astype(F64), N_AIMED, 0.05, 0.3)


def _edited_into_extremes(c):
    """The scene is created as the 2^16-scaled base; rs_scene_set_triangles then moves 64 non-emissive triangles into the sub-cell
    cluster and 8 more onto the corners of the creation-time root box."""
    sd = c.sd
    _affine(sd, scale=(2.0 ** 16,) * 3)
    rng = np.random.default_rng(44)
    lo, hi = root_box64(sd)
    ids = np.sort(rng.choice(movable(sd), 72, replace=False)).astype(np.int32)
    v = np.concatenate([cluster_vertices(rng, lo, hi, 64).astype(F32), corner_triangles(lo.astype(F32), hi.astype(F32))])
    c.edit = (ids, np.ascontiguousarray(v, F32))
    c.special = dict(cluster=ids[:64], corners=ids[64:])
    after = edited_scene_data(c)
    r1, s1 = _aimed(rng, after, after.vertices[ids[:64]].astype(F64), N_AIMED - 256)
    r2, s2 = _aimed(rng, after, after.vertices[ids[64:]].astype(F64), 256)
    c.aimed = np.concatenate([r1, r2]), np.concatenate([s1, s2])


# name: (bases, edit, what the case drives)
TABLE = {
    "far":          (BASES, _far, "translated by (1e4, -3e4, 2e4): coordinates whose ulp is 30 to 60 grid steps of cornell; the grid still fits"),
    "beyond_grid":  (BASES, _beyond_grid, "translated by (1e6, 0, 0), the Sponza-class scene by (1.6e7, 0, 0): the rounding of `base` exceeds the "
                                          "200-step apron, grid_box refuses boxes, the scene comes up without grid trees and renders through "
                                          "the reference's tree"),
    "apron_of_two_ulps": (("sponza:0.03",), _apron_of_two_ulps, "translated by (1e6, 0, 0): the 200 steps below the root box are two ulps of "
                                                                "the coordinate; the grid just fits and is walked"),
    "huge":         (BASES, _huge, "uniform scale 2^20"),
    "tiny":         (BASES, _tiny, "the smallest power-of-two scale at which the reference itself still finds its triangles"),
    "slab":         (BASES, _slab, "x scaled by 1024: the y and z extents span about 64 grid steps"),
    "squashed":     (BASES, _squashed, "y scaled by 2^-16: the whole scene is about one grid step thick in y"),
    "sub_cell":     (BASES, _sub_cell, "scaled by 2^16, plus 64 triangles (32 of them lights) within a quarter of a grid step of one point: "
                                       "boxes, an emissive tree and light-table entries smaller than a cell"),
    "coincident":   (BASES, _coincident, "exact copies of up to 64 triangles: equal hit distances, the reference's visiting order decides"),
    "needles":      (BASES, _needles, "32 slivers a few ulps wide and as long as the scene, 8 triangles without area"),
    "edited_into_extremes": (("sponza:0.03",), _edited_into_extremes, "rs_scene_set_triangles moves triangles into the sub-cell cluster "
                                                                      "and onto the corners of the creation-time root box"),
}
CASES = [(n, b) for n in TABLE for b in TABLE[n][0]]
CASE_IDS = ["%s-%s" % (n, b.split(":")[0]) for n, b in CASES]
RAGGED_TOO = ("far", "sub_cell")


def edited_scene_data(c):
    """The scene data after the case's edit (the generators and the oracle read it); the case's own where there is none."""
    if c.edit is None:
        return c.sd
    after = copy.copy(c.sd)
    after.vertices, after.normals = apply_triangles(c.sd.vertices, c.sd.normals, *c.edit)
    return after


@functools.lru_cache(maxsize=None)
def case(name, base):
    bases, edit, _ = TABLE[name]
    assert base in bases
    c = Case(name, base)
    edit(c)
    camera = EXPECT.get((name, base), {}).get("camera")
    if camera is not None:                                   # a position chosen on the CPU: the mapped one sees too little
        c.notes["mapped_camera"] = c.sd.camera_args["position"]
        c.sd.camera_args = dict(c.sd.camera_args, position=tuple(camera))
    c.after = edited_scene_data(c)
    assert np.isfinite(c.after.vertices).all() and np.isfinite(c.sd.vertices).all()
    rays, segs = closest_like_rays(c.after, N_GENERATED, 34), _shadow_like_segments(c.after, N_GENERATED, 36)
    if c.aimed is not None:
        rays, segs = np.concatenate([rays, c.aimed[0]]), np.concatenate([segs, c.aimed[1]])
    c.aimed_rays = np.random.default_rng(35).permutation(len(rays)) >= N_GENERATED          # after the shuffle: which rays are aimed ones
    c.rays = np.ascontiguousarray(rays[np.random.default_rng(35).permutation(len(rays))])
    c.aimed_segs = np.random.default_rng(37).permutation(len(segs)) >= N_GENERATED
    c.segs = np.ascontiguousarray(segs[np.random.default_rng(37).permutation(len(segs))])
    return c


@functools.lru_cache(maxsize=None)
def oracle_scene_of(name, base):
    """The oracle's scene of a case.  Of the edited case: the edited vertices under the threaded orders of the scene as created and
    boxes refitted by the NumPy restatement (tests/refit_tables.refit_boxes_bits) -- what an edit leaves, with no library call in it."""
    c = case(name, base)
    sc = oracle_scene(c.sd)
    sc.set_sample_sequence(None)
    if c.edit is not None:
        sc = rebuilt_oracle_scene(sc, c.after.vertices, c.after.normals, rt.refit_boxes_bits(c.after.vertices, sc.nodes[0]))
    return sc


@functools.lru_cache(maxsize=None)
def oracle_hits(name, base):
    """(primitive, material, position, normal) of every ray of the case."""
    return oracle_scene_of(name, base).intersect(case(name, base).rays)[:4]


@functools.lru_cache(maxsize=None)
def oracle_occlusion(name, base):
    return oracle_scene_of(name, base).test_occlusion(case(name, base).segs)


# ---------------------------------------------------------------------------------------------------------------------------------
# frames: the call sequence, once for the oracle and once for the library (tests/test_gpu_geometric_extremes.py passes its own back end)
# ---------------------------------------------------------------------------------------------------------------------------------
class OracleFrames(xc.OracleBackend):
    def __init__(self, sd, scene, size):
        self.sd, self.size, self.n, self.shared = sd, size, size[0] * size[1], scene

    def temp(self, r):
        return r.restir.temp.copy()


def run_frames(be, frames=3, multi_bounce=True):
    """`frames` frames of ReSTIRDirect with reuse 3 -- image, ray count, both reservoir buffers and every G-buffer plane after each --
    then the PT-direct baseline and pathTrace at depth 4 (the emissive tree and the bounce-ray service): flat keys -> arrays / counts."""
    out = {}
    r = be.renderer()
    for f in range(frames):
        k = "direct/f%d/" % f
        out[k + "image"], out[k + "rays"], out[k + "last"], out[k + "temp"] = np.array(r.frame(3)), int(r.rays), be.last(r), be.temp(r)
        for plane, a in be.gbuffer(r).items():
            out[k + "gbuffer/" + plane] = a
    if multi_bounce:
        r = be.renderer()
        out["ptd/image"], out["ptd/rays"] = np.array(r.frame(0, use_reservoir=False)), int(r.rays)
        out["pt4/direct"], out["pt4/indirect"], rays = be.path_trace(be.renderer(), 0, 4)
        out["pt4/rays"] = int(rays)
    return out


def frames_of(name):
    """(frames, multi-bounce passes too): the edited case runs one frame after its edit."""
    return (1, False) if name == "edited_into_extremes" else (3, True)


@functools.lru_cache(maxsize=None)
def oracle_frames(name, base, size):
    assert xc._correctly_rounded, "oracle_frames: inside extreme_cases.correctly_rounded_libm() only"
    c = case(name, base)
    return run_frames(OracleFrames(c.after, oracle_scene_of(name, base), size), *frames_of(name))


def coverage(prim_plane):
    """The share of pixels that see geometry (the G-buffer's id plane holds -1 at a miss)."""
    return float(np.mean(prim_plane != -1))


# ---------------------------------------------------------------------------------------------------------------------------------
# the grid, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def grid_of(vertices):
    """rs_quantize_occlusion_bvh in NumPy: dict(exists, base, scale, margin, lo, hi, refused) for a scene of these triangles.  The leaf
    boxes are the min / max of each triangle's vertices, the root box their union; `refused` counts the leaf boxes and the root that
    grid_box turns down (every inner box lies between a leaf's and the root's: if those fit, it fits)."""
    v = np.asarray(vertices, F32).reshape(-1, 3, 3)
    tlo, thi = v.min(1), v.max(1)
    lo, hi = tlo.min(0), thi.max(0)
    ext = F32((hi - lo).max())                               # float32 differences, as the library takes them
    if not (ext > 0 and np.isfinite(ext)):
        return dict(exists=False, refused=None, lo=lo, hi=hi)
    scale = np.full(3, ext / F32(GRID_STEPS), F32)
    base = (lo - F32(200.0) * scale).astype(F32)
    margin = float(np.ldexp(F64(ext), -17))
    _, fits = rt.grid_box(np.concatenate([tlo, lo[None]]), np.concatenate([thi, hi[None]]), base, scale, margin)
    return dict(exists=bool(fits.all()), base=base, scale=scale, margin=margin, lo=lo, hi=hi, refused=int((~fits).sum()))


def general_and_in_reach(grid, origins, directions):
    """Which rays walk the grid-box trees (rs_walk.h): none of AABB::intersect's special cases -- every |d.c| in [1e-6, 1 - 1e-6], no
    NaN -- and an origin within 4 grid extents of the grid's base (grid_reaches), in float32 as the device evaluates it."""
    o, d = np.asarray(origins, F32), np.asarray(directions, F32)
    eps = F32(1e-6)
    with np.errstate(invalid="ignore"):
        general = ((np.abs(d) >= eps) & (np.abs(d) <= F32(1) - eps)).all(1)
        reach = (np.abs(o - grid["base"]) <= F32(4.0) * F32(65535.0) * grid["scale"]).all(1)
    return general & reach


def walked_share(c, grid):
    """(share of the case's rays, share of its segments) that are general-case and within reach."""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = c.segs[:, 3:] - c.segs[:, :3]
        d = d / np.sqrt((d * d).sum(1, dtype=F32))[:, None]
    return (float(general_and_in_reach(grid, c.rays[:, :3], c.rays[:, 3:]).mean()),
            float(general_and_in_reach(grid, c.segs[:, :3], d).mean()))


def hits_beside_the_ray(sd, rays, prim):
    """Closest hits on a triangle that the ray, by its geometry, never comes near: rays with a near-zero direction component on an axis
    (the reference tests only the other two slabs of a box then, src/bvh.h:136-146) whose origin lies outside the hit triangle's box on
    that axis by more than 1e-3 * (1 + |coordinate|) -- the distance at which skip_far_on_axis (rs_intersect.h) skips a box.  The
    reference reports them for rays inside the triangle's plane, where its test is pure rounding."""
    v, o, d = sd.vertices, rays[:, :3], rays[:, 3:]
    count = 0
    with np.errstate(invalid="ignore"):
        for c in range(3):
            idx = np.nonzero((np.abs(d[:, c]) < F32(1e-6)) & (prim >= 0) & (np.abs(d) <= F32(1) - F32(1e-6)).all(1))[0]
            lo, hi = v[prim[idx]][:, :, c].min(1), v[prim[idx]][:, :, c].max(1)
            tol = F32(1e-3) * (F32(1) + np.maximum(np.abs(lo), np.abs(hi)))
            count += int(((o[idx, c] < lo - tol) | (o[idx, c] > hi + tol)).sum())
    return count


def scaled_room():
    """The Cornell box scaled by 2 -- a room 4 units wide -- and 20 000 rays and 20 000 segments of every kind for it."""
    sd = get_scene("cornell")
    _affine(sd, scale=(2.0, 2.0, 2.0))
    return sd, closest_like_rays(sd, 20000, 38), _shadow_like_segments(sd, 20000, 39)


def edit_room_oracle():
    """The oracle's scene of edit_room() after its edit: the threaded orders of the scene as created, boxes refitted in NumPy."""
    sd, _, after, _, _ = edit_room()
    sc = oracle_scene(sd)
    return rebuilt_oracle_scene(sc, after.vertices, after.normals, rt.refit_boxes_bits(after.vertices, sc.nodes[0]))


def edit_room():
    """A scene the axis cull runs in, and an edit that must switch it off: 256 triangles no larger than 0.8 across in a box 16 units
    wide (edge-component products at most 0.64), six of which rs_scene_set_triangles then stretches over face diagonals of the root box
    (products of 256: a ray inside such a triangle's plane "hits" it by rounding wherever it runs, hits_beside_the_ray).  Returns (scene
    data, (ids, vertices) of the edit, scene data after it, rays, segments): the generators' rays and segments for the edited scene,
    plus 4 096 rays and segments inside the planes of the six, along an edge of theirs and so with one direction component exactly
    zero, starting outside the triangle."""
    from restir_amd import scenes
    from restir_amd.ctypes_structs import LAMBERTIAN, make_materials
    rng = np.random.default_rng(45)
    soup = scenes.TriangleSoup()
    soup.add_flat((rng.uniform(-7.5, 7.5, (256, 1, 3)) + rng.uniform(-0.4, 0.4, (256, 3, 3))).astype(F32), 0)
    sd = scenes.SceneData("edit_room", soup, make_materials([dict(type=LAMBERTIAN, baseColor=(0.6, 0.6, 0.6))]),
                          dict(position=(0.0, 0.0, 30.0), rotation=(-90.0, 0.0, 0.0), fov_y=30.0, focal_dist=1.0))
    lo, hi = root_box64(sd)
    ids = np.array([3, 50, 97, 144, 191, 238], np.int32)
    edit = (ids, np.ascontiguousarray(corner_triangles(lo.astype(F32), hi.astype(F32))[:6]))
    after = copy.copy(sd)
    after.vertices, after.normals = apply_triangles(sd.vertices, sd.normals, *edit)
    t = after.vertices[ids].astype(F64)[rng.integers(0, 6, 4096)]
    u = rng.uniform(0.1, 0.4, (4096, 2))
    g = t[:, 0] * (1 - u.sum(1))[:, None] + t[:, 1] * u[:, :1] + t[:, 2] * u[:, 1:]
    o, b = g + (t[:, 0] - g) * 1.5, g + (t[:, 1] - g) * 1.5          # corners 0 and 1 of a triangle differ on two axes: zero on the third
    rays = np.concatenate([closest_like_rays(after, 4096, 46), np.concatenate([o, _unit(b - o)], 1).astype(F32)])
    segs = np.concatenate([_shadow_like_segments(after, 4096, 47), np.concatenate([o, b], 1).astype(F32)])
    return sd, edit, after, np.ascontiguousarray(rays), np.ascontiguousarray(segs)


def edge_product(vertices):
    """The largest product of the largest components of a triangle's two edge vectors (scene.hip far_skip_allowed bounds it by 1)."""
    v = np.asarray(vertices, F32)
    return float((np.abs(v[:, 1] - v[:, 0]).max(1) * np.abs(v[:, 2] - v[:, 0]).max(1)).max())


def figures(name, base):
    """The figures of one case that EXPECT states, from the oracle and NumPy alone."""
    c = case(name, base)
    prim = oracle_hits(name, base)[0]
    occ = oracle_occlusion(name, base)
    grid = grid_of(c.sd.vertices)                            # the grid is laid at creation; an edit keeps it
    f = dict(grid=grid["exists"], refused=grid["refused"],
             hits=round(float((prim[~c.aimed_rays] >= 0).mean()), 4), occluded=round(float(occ[~c.aimed_segs].mean()), 4))
    if grid["exists"]:
        f["walked"] = tuple(round(x, 4) for x in walked_share(c, grid))
    for kind, ids in c.special.items():
        f["hits_on_" + kind] = int(np.isin(prim, ids).sum())
    if c.aimed is not None:
        f["aimed_hits"] = int(np.isin(prim[c.aimed_rays], np.concatenate(list(c.special.values()))).sum())
        f["aimed_occluded"] = int(occ[c.aimed_segs].sum())
    return f


def frame_figures(name, base):
    """From the oracle's frames at SIZE: the share of pixels that see geometry, and the lit pixels of the last ReSTIR frame."""
    o = oracle_frames(name, base, SIZE)
    last = "direct/f%d/" % (frames_of(name)[0] - 1)
    return dict(coverage=round(coverage(o["direct/f0/gbuffer/prim_id"]), 4), lit=int(o[last + "image"].any(1).sum()))


# What the oracle and the NumPy restatement of the grid give (figures(); the oracle is deterministic, so the counts are exact).
#   grid / refused: whether the grid-box trees exist, and how many of the leaf boxes and the root grid_box turns down;
#   hits, occluded: the oracle's fractions on the generators' 4 133 rays and segments;
#   walked: the share of all the case's rays and of its segments that are general-case and within grid_reaches;
#   hits_on_<kind>: closest hits (of all rays) that land on the case's special triangles; aimed_hits: aimed rays whose closest hit is a
#   special triangle; aimed_occluded: occluded aimed segments (of 2 048);
#   (beyond_grid: the restatement refuses 9 of cornell's 37 boxes -- the root and the 8 triangles that touch its lower x face, where the
#   rounded base leaves no apron -- and 575 of the Sponza-class scene's 7 865)
#   camera: a camera position chosen on the CPU where the mapped one sees geometry in less than 30 % of the oracle's pixels, and
#   coverage, lit: the share of pixels that see geometry at 48 x 32, and the pixels of the last ReSTIR frame that are not black.
EXPECT = {
    ("far", "cornell"): {'grid': True, 'refused': 0, 'hits': 0.8091, 'occluded': 0.5754, 'walked': (0.7663, 0.7256), 'coverage': 0.7493, 'lit': 877},
    ("far", "sponza:0.03"): {'grid': True, 'refused': 0, 'hits': 0.9594, 'occluded': 0.7377, 'walked': (0.828, 0.8149), 'coverage': 1.0, 'lit': 928},
    ("beyond_grid", "cornell"): {'grid': False, 'refused': 9, 'hits': 0.8069, 'occluded': 0.6056, 'coverage': 0.7493, 'lit': 868},
    ("apron_of_two_ulps", "sponza:0.03"): {'grid': True, 'refused': 0, 'hits': 0.954, 'occluded': 0.7068, 'walked': (0.7975, 0.7283), 'coverage': 1.0, 'lit': 976},
    ("beyond_grid", "sponza:0.03"): {'grid': False, 'refused': 575, 'hits': 0.9489, 'occluded': 0.3053, 'coverage': 1.0, 'lit': 1235},
    ("huge", "cornell"): {'grid': True, 'refused': 0, 'hits': 0.8009, 'occluded': 0.4999, 'walked': (0.7663, 0.6475), 'coverage': 0.7493, 'lit': 882},
    ("huge", "sponza:0.03"): {'grid': True, 'refused': 0, 'hits': 0.9521, 'occluded': 0.6506, 'walked': (0.8287, 0.6971), 'coverage': 1.0, 'lit': 1006},
    ("tiny", "cornell"): {'grid': True, 'refused': 0, 'hits': 0.7718, 'occluded': 0.2988, 'walked': (0.7663, 0.7423), 'coverage': 0.7493, 'lit': 997},
    ("tiny", "sponza:0.03"): {'grid': True, 'refused': 0, 'hits': 0.8103, 'occluded': 0.2487, 'walked': (0.8287, 0.8219), 'coverage': 0.6185, 'lit': 867},
    ("slab", "cornell"): {'grid': True, 'refused': 0, 'hits': 0.6932, 'occluded': 0.4815, 'walked': (0.7203, 0.61), 'coverage': 1.0, 'lit': 1334},
    ("slab", "sponza:0.03"): {'grid': True, 'refused': 0, 'hits': 0.9141, 'occluded': 0.4972, 'walked': (0.7868, 0.6436), 'coverage': 1.0, 'lit': 1284},
    ("squashed", "cornell"): {'grid': True, 'refused': 0, 'hits': 0.8427, 'occluded': 0.6547, 'walked': (0.7641, 0.728), 'coverage': 1.0, 'lit': 768, 'camera': (0.0, 1.52587890625e-05, 0.875)},
    ("squashed", "sponza:0.03"): {'grid': True, 'refused': 0, 'hits': 0.9383, 'occluded': 0.5376, 'walked': (0.805, 0.7564), 'coverage': 1.0, 'lit': 835},
    ("sub_cell", "cornell"): {'grid': True, 'refused': 0, 'hits': 0.8684, 'occluded': 0.8217, 'walked': (0.8848, 0.8707), 'hits_on_cluster': 2690, 'hits_on_cluster_lights': 1638, 'aimed_hits': 1704, 'aimed_occluded': 2048, 'coverage': 0.7493, 'lit': 882},
    ("sub_cell", "sponza:0.03"): {'grid': True, 'refused': 0, 'hits': 0.9528, 'occluded': 0.7377, 'walked': (0.8855, 0.8267), 'hits_on_cluster': 2061, 'hits_on_cluster_lights': 1284, 'aimed_hits': 2048, 'aimed_occluded': 2048, 'coverage': 1.0, 'lit': 1021},
    ("coincident", "cornell"): {'grid': True, 'refused': 0, 'hits': 0.7955, 'occluded': 0.5708, 'walked': (0.8478, 0.8266), 'hits_on_copies': 2782, 'hits_on_originals': 2554, 'aimed_hits': 2048, 'aimed_occluded': 2048, 'coverage': 0.7493, 'lit': 885},
    ("coincident", "sponza:0.03"): {'grid': True, 'refused': 0, 'hits': 0.9444, 'occluded': 0.5611, 'walked': (0.8855, 0.8798), 'hits_on_copies': 666, 'hits_on_originals': 766, 'aimed_hits': 1407, 'aimed_occluded': 2048, 'coverage': 1.0, 'lit': 1321},
    ("needles", "cornell"): {'grid': True, 'refused': 0, 'hits': 0.7602, 'occluded': 0.3893, 'walked': (0.845, 0.8478), 'hits_on_slivers': 1296, 'hits_on_zero_area': 0, 'aimed_hits': 1247, 'aimed_occluded': 2023, 'coverage': 0.7493, 'lit': 884},
    ("needles", "sponza:0.03"): {'grid': True, 'refused': 0, 'hits': 0.946, 'occluded': 0.5466, 'walked': (0.8863, 0.8798), 'hits_on_slivers': 2030, 'hits_on_zero_area': 0, 'aimed_hits': 2030, 'aimed_occluded': 2042, 'coverage': 1.0, 'lit': 1321},
    ("edited_into_extremes", "sponza:0.03"): {'grid': True, 'refused': 0, 'hits': 0.9739, 'occluded': 0.8253, 'walked': (0.8853, 0.8266), 'hits_on_cluster': 1765, 'hits_on_corners': 2885, 'aimed_hits': 2041, 'aimed_occluded': 2048, 'coverage': 0.9954, 'lit': 149},
}
