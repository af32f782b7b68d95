"""Helpers of tests/test_part_transforms_host.py and tests/test_gpu_part_transforms.py: rigid parts (rs_scene_define_parts,
rs_scene_set_part_transforms).  Matrices, a NumPy restatement of rs_bake_matrix in float32 with GLM's grouping of every sum (used only
to cross-check rs_bake_matrix without a GPU), the parts the GPU tests define on their scenes, and the oracle's side of a transform: a
fresh oracle scene of the vertices and normals rs_bake_matrix (host only) gives, made as tests/emitter_edits.py makes it -- never
anything read back from the scene under test."""
import functools

import numpy as np

from tests.emitter_edits import HipSide as _HipSide, OracleSide as _OracleSide, emitters, scene_data
from tests.geometry_edits import movable, root_box

F = np.float32


# ---- matrices: (4, 4) float32, [column][row], as rs_build_transformation_matrix returns them --------------------------------------------
def identity():
    return np.eye(4, dtype=F)


def from_rows(rows):
    """A matrix written the way it is read on paper (rows) in the library's [column][row] layout."""
    return np.ascontiguousarray(np.asarray(rows, np.float64).T.astype(F))


def translation(t):
    m = np.eye(4)
    m[:3, 3] = t
    return from_rows(m)


def rotation_about(centre, axis, degrees, shift=(0.0, 0.0, 0.0)):
    """Rotation by `degrees` about the line through `centre` along `axis`, then a translation by `shift`."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.radians(degrees)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * (k @ k)
    c = np.asarray(centre, np.float64)
    m = np.eye(4)
    m[:3, :3] = r
    m[:3, 3] = c - r @ c + np.asarray(shift, np.float64)
    return from_rows(m)


# ---- rs_bake_matrix restated ---------------------------------------------------------------------------------------------------------------
def numpy_inverse(m):
    """glm::inverse of a 4x4 (type_mat4x4.inl:37-92) in float32, one operation per rounding, with GLM's grouping; m[column][row]."""
    m = np.asarray(m, F).reshape(4, 4)
    row_pair = [(2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1)]
    col_pair = [(2, 3), (1, 3), (1, 2)]
    minor = np.zeros((6, 3), F)
    for g, (ra, rb) in enumerate(row_pair):
        for k, (ca, cb) in enumerate(col_pair):
            minor[g, k] = F(m[ca, ra] * m[cb, rb]) - F(m[cb, ra] * m[ca, rb])

    def fac(g, k):
        return minor[g, 0 if k < 2 else k - 1]

    def vec(r, k):
        return m[1 if k == 0 else 0, r]
    inv = np.zeros((4, 4), F)
    for k in range(4):
        plus = F(-1.0) if k & 1 else F(1.0)
        minus = F(-plus)
        inv[0, k] = F(F(F(vec(1, k) * fac(0, k)) - F(vec(2, k) * fac(1, k))) + F(vec(3, k) * fac(2, k))) * plus
        inv[1, k] = F(F(F(vec(0, k) * fac(0, k)) - F(vec(2, k) * fac(3, k))) + F(vec(3, k) * fac(4, k))) * minus
        inv[2, k] = F(F(F(vec(0, k) * fac(1, k)) - F(vec(1, k) * fac(3, k))) + F(vec(3, k) * fac(5, k))) * plus
        inv[3, k] = F(F(F(vec(0, k) * fac(2, k)) - F(vec(1, k) * fac(4, k))) + F(vec(2, k) * fac(5, k))) * minus
    det = F(F(m[0, 0] * inv[0, 0]) + F(m[0, 1] * inv[1, 0])) + F(F(m[0, 2] * inv[2, 0]) + F(m[0, 3] * inv[3, 0]))
    with np.errstate(all="ignore"):
        return (inv * F(F(1.0) / F(det))).astype(F)


def numpy_bake(matrix, vertices, normals):
    """vec3(m * vec4(v, 1)) and normalize(transpose(mat3(inverse(m))) * n) for (k, 3) float32 corners, in rs_bake.h's grouping."""
    m = np.asarray(matrix, F).reshape(4, 4)
    v = np.asarray(vertices, F).reshape(-1, 3)
    n = np.asarray(normals, F).reshape(-1, 3)
    inv = numpy_inverse(m)
    nm = np.ascontiguousarray(inv[:3, :3].T)              # columns of transpose(mat3(inverse)): nm[j][k] = inv[k][j]
    with np.errstate(all="ignore"):
        pos = np.stack([(m[0, r] * v[:, 0] + m[1, r] * v[:, 1]) + (m[2, r] * v[:, 2] + m[3, r] * F(1.0)) for r in range(3)], 1)
        q = np.stack([(nm[0, r] * n[:, 0] + nm[1, r] * n[:, 1]) + nm[2, r] * n[:, 2] for r in range(3)], 1)
        dot = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        nrm = q * (F(1.0) / np.sqrt(dot))[:, None]
    assert pos.dtype == F and nrm.dtype == F
    return pos, nrm


# ---- the parts of the GPU tests -----------------------------------------------------------------------------------------------------------
SPONZA_PART_SIZES = (1, 63, 64, 65, 193)                 # wave (64 lanes = 21 1/3 triangles) and block boundaries inside, between and on part edges
BISTRO_LAMPS = 64


@functools.lru_cache(maxsize=None)
def parts_of(name):
    """The parts (lists of primitive ids) the tests define on scene `name` of tests/emitter_edits.py, and what each is: "lamp", "box" or "empty".
      cornell: the lamp's two triangles; the tall box; an empty part.
      many (the Sponza-class scene, 2 621 triangles): parts of 1, 63, 64, 65 and 193 triangles dealt from the shuffled movable triangles
        nearest the scene's middle (ids far from contiguous), then a part of its emitters -- all ten: the scene at this scale has no 64.
      bistro: 64 of the emitters, those nearest the scene's middle, and 65 other triangles.
    Every other triangle is in no part."""
    sd = scene_data(name)
    if name == "cornell":
        return [emitters(sd).tolist(), list(range(10, 22)), []], ["lamp", "box", "empty"]
    v = sd.vertices.reshape(-1, 3, 3)
    lo, hi = root_box(v)
    far = np.abs((v.mean(1) - (lo + hi) / 2) / (hi - lo)).max(1)
    rng = np.random.default_rng(17)
    if name == "many":
        ids = movable(sd)
        near = ids[np.argsort(far[ids], kind="stable")[:sum(SPONZA_PART_SIZES)]]
        near = near[rng.permutation(len(near))]
        cuts = np.cumsum((0,) + SPONZA_PART_SIZES)
        return [near[a:b].tolist() for a, b in zip(cuts[:-1], cuts[1:])] + [emitters(sd).tolist()], ["box"] * len(SPONZA_PART_SIZES) + ["lamp"]
    if name == "bistro":
        e, ids = emitters(sd), movable(sd)
        lamps = e[np.argsort(far[e], kind="stable")[:BISTRO_LAMPS]]
        other = ids[np.argsort(far[ids], kind="stable")[:65]]
        return [lamps[rng.permutation(len(lamps))].tolist(), other[rng.permutation(len(other))].tolist()], ["lamp", "box"]
    raise KeyError(name)


def rest_of(sd, part):
    ids = np.asarray(part, np.int64)
    return sd.vertices.reshape(-1, 3, 3)[ids], sd.normals.reshape(-1, 3, 3)[ids]


def part_matrix(name, part, step=0):
    """The matrix test step `step` gives part `part` of scene `name`: a rotation of a few degrees about an axis through the part's own
    centroid and a translation of at most 2 % of the scene's extent (the Cornell lamp, 2 cm under the ceiling: about the vertical axis,
    and downwards).  bake() asserts that every baked vertex stays inside the box the scene was created with."""
    sd = scene_data(name)
    ids, kinds = parts_of(name)
    lo, hi = root_box(sd.vertices)
    ext = (hi - lo).astype(np.float64)
    v, _ = rest_of(sd, ids[part])
    if len(v) == 0:
        return identity()
    centre = v.reshape(-1, 3).astype(np.float64).mean(0)
    rng = np.random.default_rng(1000 * part + step)
    if kinds[part] == "lamp" and name == "cornell":
        return rotation_about(centre, (0, 1, 0), 3.0 + 2.0 * (step % 4), ext * (0.01, -0.008 - 0.001 * step, 0.012))
    axis = (0, 1, 0) if name == "cornell" else rng.normal(size=3)        # (the Cornell box stands on the floor: it turns, and rises)
    shift = rng.uniform(-0.02, 0.02, 3) * ext
    shift = np.where(centre + shift > (lo + hi) / 2, -np.abs(shift), np.abs(shift))       # towards the middle
    return rotation_about(centre, axis, 2.0 + 1.5 * (step % 4), shift)


def bake(capi, name, part, matrix, rest=None):
    """(ids, vertices, normals) of part `part` of scene `name` under `matrix`: rs_bake_matrix (host only) over its rest pose -- the pose
    the scene was created in, or rest = (vertices, normals) as handed to define_parts."""
    sd = scene_data(name)
    ids = np.asarray(parts_of(name)[0][part], np.int32)
    v, n = rest_of(sd, ids) if rest is None else rest
    bv, bn = capi.bake_matrix(matrix, v, n)
    bv, bn = bv.reshape(-1, 3, 3), bn.reshape(-1, 3, 3)
    lo, hi = root_box(sd.vertices)
    assert np.isfinite(bv).all() and np.isfinite(bn).all()
    assert (bv >= lo).all() and (bv <= hi).all(), (name, part, "a baked vertex leaves the creation-time root box")
    return ids, bv, bn


def baked_edit(capi, name, part_ids, matrices, rest=None):
    """The rs_scene_set_geometry arguments that equal set_part_transforms(part_ids, matrices): the named parts' primitives in the order of
    the call, rs_bake_matrix of each part's matrix over its rest pose (rest: {part: (vertices, normals)} where define_parts was given one)."""
    out = [bake(capi, name, p, m, (rest or {}).get(p)) for p, m in zip(part_ids, matrices)]
    if not out:
        return np.zeros(0, np.int32), np.zeros((0, 3, 3), F), np.zeros((0, 3, 3), F)
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


class OracleSide(_OracleSide):
    """The oracle's side of a transform: set_geometry of tests/emitter_edits.py with the arrays of rs_bake_matrix."""

    def __init__(self, capi, name, W, H, **kw):
        super().__init__(capi, scene_data(name), W, H, **kw)
        self.name = name

    def set_part_transforms(self, part_ids, matrices, rest=None):
        ids, v, n = baked_edit(self.capi, self.name, part_ids, matrices, rest)
        if len(ids):
            self.set_geometry(ids, v, n)


class HipSide(_HipSide):
    def __init__(self, capi, name, W, H, **kw):
        super().__init__(capi, scene_data(name), W, H, **kw)
        self.r.scene.define_parts(parts_of(name)[0])

    def set_part_transforms(self, part_ids, matrices):
        self.r.scene.set_part_transforms(part_ids, matrices)
