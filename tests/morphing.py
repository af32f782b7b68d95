"""Helpers of tests/test_morphing_host.py and tests/test_gpu_morphing.py: morph targets (rs_scene_define_morph, rs_scene_define_skin_morph,
rs_scene_set_morph_weights, rs_scene_set_skin_pose).  A NumPy restatement of rs_bake.h's morph_corner in float32 -- one rounding per
operation, ascending target order, the skip of a zero weight and the `applied` rule -- and of the by-target -> by-corner conversion; the
morphs the GPU tests define on the scenes of tests/emitter_edits.py and on the skins of tests/skinning.py, and their weight steps; and the
oracle's side of a weight step: a fresh oracle scene of the arrays rs_morph_corners (host only) gives, as tests/skinning.py makes it --
never anything read back from the scene under test."""
import functools

import numpy as np

from tests import part_transforms as pt
from tests import skinning as sk
from tests.emitter_edits import HipSide as _HipSide, OracleSide as _OracleSide, emitters, scene_data
from tests.geometry_edits import movable, root_box

F = np.float32
MAX_TARGETS = 256
WEIGHTS_PER_RECORD, RECORD_BYTES = 28, 112
ENTRY = np.dtype([("target", np.int32), ("dp", np.float32, 3), ("dn", np.float32, 3), ("pad", np.int32)])


def staged_bytes(num_targets, num_bones=0):
    """What an edit stages: the bone records of a skin pose, then the weights as whole zero-padded records of 28 floats."""
    return RECORD_BYTES * (num_bones + -(-num_targets // WEIGHTS_PER_RECORD))


# ---- rs_morph_corners restated ------------------------------------------------------------------------------------------------------------
def numpy_morph(target_first, entry_corner, delta_positions, delta_normals, weights, vertices, normals):
    """morph_corner for (k, 3) float32 corners.  The targets in ascending order; a target of weight 0 (either sign) is skipped whole;
    otherwise p = p + w * dp and q = q + w * dn per component on the target's corners (no corner twice in one target, so one vector
    operation per target keeps every corner's own order); normal = q * (1 / sqrt((qx * qx + qy * qy) + qz * qz)) where a target was
    applied, else the rest normal's bits."""
    first = np.asarray(target_first, np.int64)
    ec = np.asarray(entry_corner, np.int64)
    dp = np.asarray(delta_positions, F).reshape(-1, 3)
    dn = np.zeros_like(dp) if delta_normals is None else np.asarray(delta_normals, F).reshape(-1, 3)
    w = np.asarray(weights, F)
    p, q = np.array(vertices, F).reshape(-1, 3), np.array(normals, F).reshape(-1, 3)
    rest_n = q.copy()
    applied = np.zeros(len(p), bool)
    with np.errstate(all="ignore"):
        for t in range(len(first) - 1):
            if w[t] == 0:
                continue
            e = slice(first[t], first[t + 1])
            c = ec[e]
            assert len(np.unique(c)) == len(c)
            p[c] = p[c] + w[t] * dp[e]
            q[c] = q[c] + w[t] * dn[e]
            applied[c] = True
        dot = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        nrm = q * (F(1.0) / np.sqrt(dot))[:, None]
    assert p.dtype == F and nrm.dtype == F
    return p, np.where(applied[:, None], nrm, rest_n)


def by_corner(num_corners, target_first, entry_corner, delta_positions, delta_normals):
    """The by-corner form the device keeps: (cornerFirst [num_corners + 1], ENTRY records), a corner's entries in ascending target id."""
    first = np.asarray(target_first, np.int64)
    ec = np.asarray(entry_corner, np.int64)
    dp = np.asarray(delta_positions, F).reshape(-1, 3)
    dn = np.zeros_like(dp) if delta_normals is None else np.asarray(delta_normals, F).reshape(-1, 3)
    target = np.repeat(np.arange(len(first) - 1), np.diff(first))
    order = np.lexsort((target, ec))                     # by corner, then by target
    recs = np.zeros(len(ec), ENTRY)
    recs["target"], recs["dp"], recs["dn"] = target[order], dp[order], dn[order]
    corner_first = np.zeros(num_corners + 1, np.int32)
    corner_first[1:] = np.cumsum(np.bincount(ec, minlength=num_corners))
    return corner_first, recs


# ---- the morphs of the GPU tests ------------------------------------------------------------------------------------------------------------
# "many" (2 621 triangles): listed triangles -> targets.  3 corners; 63 and 66 corners, either side of a wave; 255 and 258, either side of a
# block; 1 158 corners over five blocks.  1, 2, 28, 29 (either side of a weight record) and 256 targets.
MANY_MORPHS = {"t1": (1, 1), "t21": (21, 2), "t22": (22, 28), "t85": (85, 29), "t86": (86, 2), "t386": (386, 256)}
MORPHS = {"cornell": ("box_lamp",), "many": tuple(MANY_MORPHS)}
# the skins of tests/skinning.py that get a morph over a subset of their corners -> targets
SKIN_MORPHS = {"t22": 3, "t85": 29, "t386": 256, "lamps": 5}
FULL_CORNER, EMPTY_CORNERS, FULL_FROM = 5, 2, 60         # from 60 corners on, corner 5 carries an entry of every target and the two after it none


class Morph:
    """A by-target table over `num_corners` corners; for a scene's own morph also ids and the rest pose (the pose at creation)."""

    def __init__(self, name, key, num_targets, num_corners, target_first, entry_corner, dp, dn, ids=None):
        self.name, self.key, self.num_targets, self.num_corners = name, key, num_targets, num_corners
        self.target_first = np.ascontiguousarray(target_first, np.int32)
        self.entry_corner = np.ascontiguousarray(entry_corner, np.int32)
        self.dp, self.dn = np.ascontiguousarray(dp, F), np.ascontiguousarray(dn, F)
        assert len(self.target_first) == num_targets + 1 and self.target_first[-1] == len(self.entry_corner) == len(self.dp) == len(self.dn)
        if ids is not None:
            self.ids = np.ascontiguousarray(ids, np.int32)
            self.rest_vertices, self.rest_normals = pt.rest_of(scene_data(name), self.ids)
            assert len(self.ids) * 3 == num_corners and len(np.unique(self.ids)) == len(self.ids)

    def table(self):
        return self.target_first, self.entry_corner, self.dp, self.dn

    def define(self, scene):
        scene.define_morph(self.ids, *self.table())

    def define_on_skin(self, scene):
        scene.define_skin_morph(*self.table())


def random_table(rng, corners, num_targets, rest, towards, size, share=0.25):
    """A by-target table: every target touches about `share` of the corners (at least one), FULL_CORNER carries every target and the
    EMPTY_CORNERS corners after it none (from FULL_FROM corners on).  A corner's deltas are at most `size` / (its number of entries) long per
    component and point from its rest position `rest` towards `towards`, so that weights in [0, 1.5] move it at most 1.5 * size that
    way; normal deltas are small and random."""
    first, ec = [0], []
    for _ in range(num_targets):
        c = np.flatnonzero(rng.random(corners) < share)
        if corners >= FULL_FROM:
            c = np.union1d(c[(c < FULL_CORNER) | (c > FULL_CORNER + EMPTY_CORNERS)], [FULL_CORNER])
        if len(c) == 0:
            c = np.array([rng.integers(corners)])
        ec.append(rng.permutation(c))
        first.append(first[-1] + len(c))
    ec = np.concatenate(ec)
    per_corner = np.bincount(ec, minlength=corners)[ec][:, None]
    inward = np.sign(np.asarray(towards, np.float64) - rest.reshape(-1, 3)[ec])
    dp = rng.uniform(0.2, 1.0, (len(ec), 3)) * inward * size / per_corner
    dn = rng.uniform(-0.3, 0.3, (len(ec), 3)) / per_corner
    return first, ec, dp.astype(F), dn.astype(F)


@functools.lru_cache(maxsize=None)
def morph_of(name, key):
    sd = scene_data(name)
    v = sd.vertices.reshape(-1, 3, 3)
    lo, hi = root_box(v)
    if name == "cornell":
        ids, targets, share = np.concatenate([np.arange(10, 22), emitters(sd)]), 3, 0.6      # the tall box and the lamp
    else:
        (count, targets), share = MANY_MORPHS[key], 0.25
        far = np.abs((v.mean(1) - (lo + hi) / 2) / (hi - lo)).max(1)
        rng = np.random.default_rng(31 + count)
        ids = movable(sd)
        near = ids[np.argsort(far[ids], kind="stable")[:2 * count]]
        ids = near[rng.permutation(len(near))[:count]]
    rng = np.random.default_rng(77 + len(ids))
    table = random_table(rng, len(ids) * 3, targets, v[ids], (lo + hi) / 2, 0.02 * (hi - lo).astype(np.float64), share)
    return Morph(name, key, targets, len(ids) * 3, *table, ids=ids)


@functools.lru_cache(maxsize=None)
def skin_morph_of(key):
    """A morph over every second corner of a skin of tests/skinning.py on "many"."""
    skin = sk.skin_of("many", key)
    targets = SKIN_MORPHS[key]
    lo, hi = root_box(scene_data("many").vertices)
    corners = len(skin.ids) * 3
    rng = np.random.default_rng(131 + corners)
    first, ec, dp, dn = random_table(rng, corners, targets, skin.rest_vertices, (lo + hi) / 2, 0.01 * (hi - lo).astype(np.float64), share=0.5)
    keep = (ec % 2 == 1) | (ec == FULL_CORNER)
    first = np.concatenate([[0], np.cumsum([keep[a:b].sum() for a, b in zip(first[:-1], first[1:])])])
    return Morph("many", key, targets, corners, first, ec[keep], dp[keep], dn[keep])


def weight_step(num_targets, step, seed=0):
    """(target ids, weights) of test step `step`: 0 -- every target, in [0, 1.5] (above 1 among them); 1 -- every third target, the rest
    keep theirs; 2 -- every weight 0 but the last target's; later steps -- every second target from `step` on."""
    rng = np.random.default_rng(7001 * step + num_targets + 13 * seed)
    if step == 0:
        ids = np.arange(num_targets)
    elif step == 1:
        ids = np.arange(0, num_targets, 3)
    elif step == 2:
        w = np.zeros(num_targets, F)
        w[-1] = 0.75
        return np.arange(num_targets, dtype=np.int32), w
    else:
        ids = np.arange(step % num_targets, num_targets, 2)
    return ids.astype(np.int32), rng.uniform(0.0, 1.5, len(ids)).astype(F)


class Weights:
    """The host's restatement of a morph's weights: zeros, then what set() names."""

    def __init__(self, capi, morph):
        self.capi, self.morph = capi, morph
        self.w = np.zeros(morph.num_targets, F)

    def set(self, target_ids, weights):
        for t, x in zip(target_ids, np.asarray(weights, F)):
            self.w[int(t)] = x
        return self

    def corners(self, vertices, normals):
        """rs_morph_corners (host only) of the weights over (k, 3) corners"""
        return self.capi.morph_corners(*self.morph.table(), self.w, vertices, normals)

    def morphed(self):
        """(ids, vertices, normals): the rs_scene_set_geometry arguments that equal the scene's morph at these weights.  Every vertex
        stays inside the box the scene was created with."""
        mo = self.morph
        v, n = self.corners(mo.rest_vertices, mo.rest_normals)
        return mo.ids, *inside(mo.name, v, n, (mo.name, mo.key))


def inside(name, v, n, tag):
    v, n = v.reshape(-1, 3, 3), n.reshape(-1, 3, 3)
    lo, hi = root_box(scene_data(name).vertices)
    assert np.isfinite(v).all() and np.isfinite(n).all(), tag
    assert (v >= lo).all() and (v <= hi).all(), (tag, "a vertex leaves the creation-time root box")
    return v, n


class SkinPose:
    """The host's restatement of a skin with a morph: palette and weights, composed by the two host functions."""

    def __init__(self, capi, key):
        self.capi, self.key = capi, key
        self.palette = sk.Palette(capi, "many", key)
        self.weights = Weights(capi, skin_morph_of(key))

    def set(self, bone_ids, matrices, target_ids, weights):
        for b, m in zip(bone_ids, np.asarray(matrices, F).reshape(-1, 4, 4)):
            self.palette.matrices[int(b)] = m
        self.weights.set(target_ids, weights)
        return self.posed()

    def posed(self):
        """(ids, vertices, normals) = rs_skin_corners(rs_morph_corners(rest))"""
        skin = self.palette.skin
        v, n = self.weights.corners(skin.rest_vertices, skin.rest_normals)
        v, n = self.capi.skin_corners(self.palette.matrices, v, n, skin.bone_ids, skin.weights)
        return skin.ids, *inside("many", v, n, ("many", self.key, "skin pose"))


class OracleSide(_OracleSide):
    """The oracle's side of a weight step: set_geometry of tests/emitter_edits.py with the arrays of rs_morph_corners."""

    def __init__(self, capi, name, key, W, H, **kw):
        super().__init__(capi, scene_data(name), W, H, **kw)
        self.weights = Weights(capi, morph_of(name, key))

    def set_morph_weights(self, target_ids, weights):
        if len(target_ids):
            self.set_geometry(*self.weights.set(target_ids, weights).morphed())


class HipSide(_HipSide):
    def __init__(self, capi, name, key, W, H, **kw):
        super().__init__(capi, scene_data(name), W, H, **kw)
        morph_of(name, key).define(self.r.scene)

    def set_morph_weights(self, target_ids, weights):
        self.r.scene.set_morph_weights(target_ids, weights)
