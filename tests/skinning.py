"""Helpers of tests/test_skinning_host.py and tests/test_gpu_skinning.py: skinned meshes (rs_scene_define_skin,
rs_scene_set_bone_transforms).  A NumPy restatement of rs_bake.h's skin_corner in float32, one rounding per operation and the header's
grouping of every sum, built on the pieces of tests/part_transforms.py (used only to cross-check rs_skin_corners without a GPU); the skins
the GPU tests define on the scenes of tests/emitter_edits.py and their poses; and the oracle's side of a pose: a fresh oracle scene of the
vertices and normals rs_skin_corners (host only) gives, made as tests/emitter_edits.py makes it -- never anything read back from the scene
under test."""
import functools

import numpy as np

from tests import part_transforms as pt
from tests.emitter_edits import HipSide as _HipSide, OracleSide as _OracleSide, emitters, scene_data
from tests.geometry_edits import movable, root_box

F = np.float32


# ---- rs_skin_corners restated -------------------------------------------------------------------------------------------------------------
def numpy_skin(matrices, vertices, normals, bone_ids, weights):
    """skin_corner for (k, 3) float32 corners, (k, 4) bone ids and (k, 4) weights over (bones, 4, 4) matrices, [column][row]:
        p_b = (m0 * x + m1 * y) + (m2 * z + m3 * 1)        q_b = (nm0 * nx + nm1 * ny) + nm2 * nz       for EVERY slot's bone,
        position = (w0 * p0 + w1 * p1) + (w2 * p2 + w3 * p3)
        normal   = q * (1 / sqrt((qx * qx + qy * qy) + qz * qz)),  q = (w0 * q0 + w1 * q1) + (w2 * q2 + w3 * q3)."""
    ms = np.asarray(matrices, F).reshape(-1, 4, 4)
    v = np.asarray(vertices, F).reshape(-1, 3)
    n = np.asarray(normals, F).reshape(-1, 3)
    b = np.asarray(bone_ids, np.int64).reshape(-1, 4)
    w = np.asarray(weights, F).reshape(-1, 4)
    k = np.arange(len(v))
    with np.errstate(all="ignore"):
        p_of, q_of = [], []
        for m in ms:
            nm = np.ascontiguousarray(pt.numpy_inverse(m)[:3, :3].T)      # columns of transpose(mat3(inverse)), as numpy_bake takes them
            p_of.append(np.stack([(m[0, r] * v[:, 0] + m[1, r] * v[:, 1]) + (m[2, r] * v[:, 2] + m[3, r] * F(1.0)) for r in range(3)], 1))
            q_of.append(np.stack([(nm[0, r] * n[:, 0] + nm[1, r] * n[:, 1]) + nm[2, r] * n[:, 2] for r in range(3)], 1))
        p_of, q_of = np.stack(p_of), np.stack(q_of)          # (bones, k, 3)

        def blend(of):
            a = [of[b[:, s], k] for s in range(4)]
            return (w[:, 0:1] * a[0] + w[:, 1:2] * a[1]) + (w[:, 2:3] * a[2] + w[:, 3:4] * a[3])
        pos, q = blend(p_of), blend(q_of)
        dot = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        nrm = q * (F(1.0) / np.sqrt(dot))[:, None]
    assert pos.dtype == F and nrm.dtype == F
    return pos, nrm


# ---- the skins of the GPU tests -----------------------------------------------------------------------------------------------------------
# "many" (the Sponza-class scene, 2 621 triangles): listed triangles -> bones.  3 corners; 63 and 66 corners, either side of a wave; 255 and
# 258, either side of a block; 1 158 corners over five blocks.  1, 2, 5 and 256 bones: every block stages the whole palette, and 256 bones
# are a block's 256 lanes.  "lamps": the scene's ten emitters and 40 other triangles on 5 bones.
MANY_SKINS = {"t1": (1, 1), "t21": (21, 2), "t22": (22, 5), "t85": (85, 256), "t86": (86, 2), "t386": (386, 256), "lamps": (40, 5)}
SKINS = {"cornell": ("box_lamp",), "many": tuple(MANY_SKINS)}
# "cornell" again, for the one refusal a rigid part cannot reach (collapse_pose below): no skin of the lists above
LAMP_CORNERS = "lamp_corners"


class Skin:
    """num_bones, ids [listed], bone_ids and weights (listed, 3, 4), the rest pose (the pose the scene was created in)."""

    def __init__(self, name, key, num_bones, ids, bone_ids, weights):
        sd = scene_data(name)
        self.name, self.key, self.num_bones = name, key, num_bones
        self.ids = np.ascontiguousarray(ids, np.int32)
        self.bone_ids = np.ascontiguousarray(bone_ids, np.int32)
        self.weights = np.ascontiguousarray(weights, F)
        self.rest_vertices, self.rest_normals = pt.rest_of(sd, self.ids)
        assert self.bone_ids.shape == self.weights.shape == (len(self.ids), 3, 4)
        assert len(np.unique(self.ids)) == len(self.ids)
        assert (self.bone_ids >= 0).all() and (self.bone_ids < num_bones).all()
        assert (self.weights >= 0).all() and ((self.weights > 0).sum(2) >= 1).all()

    def define(self, scene):
        scene.define_skin(self.num_bones, self.ids, self.bone_ids, self.weights)


def random_influences(rng, corners, num_bones):
    """(corners, 4) bone ids and weights: 1 to 4 non-zero weights per corner in random slots, summing to 1 up to rounding; a slot of weight
    0 names a bone all the same."""
    b = rng.integers(0, num_bones, (corners, 4))
    w = rng.uniform(0.1, 1.0, (corners, 4))
    live = rng.integers(1, 5, corners)
    order = np.argsort(rng.random((corners, 4)), axis=1)
    w[order >= live[:, None]] = 0.0
    w /= w.sum(1, keepdims=True)
    return b.astype(np.int32), w.astype(F)


@functools.lru_cache(maxsize=None)
def skin_of(name, key):
    sd = scene_data(name)
    v = sd.vertices.reshape(-1, 3, 3)
    if name == "cornell" and key == LAMP_CORNERS:
        # every corner of the lamp's two triangles on a bone of its own (0 .. 5: the one influence in slot 1), the tall box on bone 6
        box, lamp = np.arange(10, 22), emitters(sd)
        ids = np.concatenate([lamp, box])
        b = np.full((len(ids), 3, 4), 6, np.int32)
        w = np.zeros((len(ids), 3, 4), F)
        b[:len(lamp), :, 1] = np.arange(len(lamp) * 3).reshape(-1, 3)
        w[:len(lamp), :, 1] = 1.0
        w[len(lamp):, :, 0] = 1.0
        return Skin(name, key, 7, ids, b, w)
    if name == "cornell":
        # the tall box between bones 0 and 1 by height (its base follows bone 0, its top bone 1), the lamp's two triangles on bone 2
        box, lamp = np.arange(10, 22), emitters(sd)
        y = v[box][:, :, 1]
        t = ((y - y.min()) / (y.max() - y.min())).astype(F)
        ids = np.concatenate([box, lamp])
        b = np.zeros((len(ids), 3, 4), np.int32)
        w = np.zeros((len(ids), 3, 4), F)
        b[:len(box)] = (0, 1, 1, 0)
        w[:len(box), :, 0], w[:len(box), :, 1] = F(1.0) - t, t
        b[len(box):] = (2, 0, 1, 2)
        w[len(box):, :, 3] = 1.0                         # the one influence in the last slot
        return Skin(name, key, 3, ids, b, w)
    count, bones = MANY_SKINS[key]
    lo, hi = root_box(v)
    far = np.abs((v.mean(1) - (lo + hi) / 2) / (hi - lo)).max(1)
    rng = np.random.default_rng(23 + count)
    ids = movable(sd)
    near = ids[np.argsort(far[ids], kind="stable")[:2 * count]]
    ids = near[rng.permutation(len(near))[:count]]        # shuffled, and every second one left out: far from contiguous
    if key == "lamps":
        ids = rng.permutation(np.concatenate([ids, emitters(sd)]))
    b, w = random_influences(rng, len(ids) * 3, bones)
    return Skin(name, key, bones, ids, b.reshape(-1, 3, 4), w.reshape(-1, 3, 4))


def bone_matrix(name, key, bone, step=0):
    """The matrix test step `step` gives bone `bone`: part_matrix's kind -- a rotation of a few degrees about an axis through the skin's
    centroid and a shift of at most 2 % of the scene's extent towards its middle (Cornell: the box's and the lamp's part matrices)."""
    if name == "cornell" and key == LAMP_CORNERS:        # the six corner bones move the lamp as one, bone 6 the box
        return pt.part_matrix(name, 1, step) if bone == 6 else pt.part_matrix(name, 0, step)
    if name == "cornell":
        return pt.part_matrix(name, 0, step) if bone == 2 else pt.part_matrix(name, 1, step + bone)
    sd = scene_data(name)
    sk = skin_of(name, key)
    lo, hi = root_box(sd.vertices)
    ext = (hi - lo).astype(np.float64)
    centre = sk.rest_vertices.reshape(-1, 3).astype(np.float64).mean(0)
    rng = np.random.default_rng(100003 * bone + step)
    shift = rng.uniform(-0.02, 0.02, 3) * ext
    shift = np.where(centre + shift > (lo + hi) / 2, -np.abs(shift), np.abs(shift))
    return pt.rotation_about(centre, rng.normal(size=3), 2.0 + 1.5 * (step % 4), shift)


def pose(name, key, step=0, bones=None):
    """(bone ids, matrices) of test step `step` for the bones `bones` (default: all of them)."""
    ids = np.arange(skin_of(name, key).num_bones) if bones is None else np.asarray(bones)
    return ids.astype(np.int32), np.stack([bone_matrix(name, key, int(b), step) for b in ids])


def collapse_pose(capi):
    """(bone ids, matrices, ids, vertices, normals) on the LAMP_CORNERS skin of "cornell": plain translations along z of the lamp's corner
    bones that put all six corners on one line.  A part cannot do this -- a matrix that takes a triangle's area to 0 is singular and is
    refused for its normals -- but corners on bones of their own can: every normal matrix is the identity, every value is finite, every
    vertex is inside the root box, and both emitters -- the scene's only ones -- have area exactly 0 (their corners differ in x alone), so
    the light sampler is left without power.  The arrays are rs_skin_corners of the pose with every other bone at the identity."""
    skin = skin_of("cornell", LAMP_CORNERS)
    lamp = skin.rest_vertices[:2].reshape(6, 3)
    z0 = lamp[:, 2].min()
    bones = np.arange(6, dtype=np.int32)
    ms = np.stack([pt.translation((0.0, 0.0, float(z0) - float(z))) for z in lamp[:, 2]])
    palette = np.stack([pt.identity()] * skin.num_bones)
    palette[:6] = ms
    v, n = capi.skin_corners(palette, skin.rest_vertices, skin.rest_normals, skin.bone_ids, skin.weights)
    v, n = v.reshape(-1, 3, 3), n.reshape(-1, 3, 3)
    lo, hi = root_box(scene_data("cornell").vertices)
    assert np.isfinite(v).all() and np.isfinite(n).all() and (v >= lo).all() and (v <= hi).all()
    assert np.ptp(v[:2, :, 1]) == 0 and np.ptp(v[:2, :, 2]) == 0 and np.ptp(v[:2, :, 0]) > 0          # one line along x
    assert np.array_equal(skin.ids[:2], emitters(scene_data("cornell")))
    return bones, ms, skin.ids, v, n


class Palette:
    """The host's restatement of the scene's palette: identities, then what set() names."""

    def __init__(self, capi, name, key):
        self.capi, self.skin = capi, skin_of(name, key)
        self.matrices = np.stack([pt.identity()] * self.skin.num_bones)

    def set(self, bone_ids, matrices):
        for b, m in zip(bone_ids, np.asarray(matrices, F).reshape(-1, 4, 4)):
            self.matrices[int(b)] = m
        return self.skinned()

    def skinned(self):
        """(ids, vertices, normals): rs_skin_corners (host only) of the palette over the rest pose -- the rs_scene_set_geometry arguments
        that equal the pose.  Every skinned vertex stays inside the box the scene was created with."""
        sk = self.skin
        v, n = self.capi.skin_corners(self.matrices, sk.rest_vertices, sk.rest_normals, sk.bone_ids, sk.weights)
        v, n = v.reshape(-1, 3, 3), n.reshape(-1, 3, 3)
        lo, hi = root_box(scene_data(sk.name).vertices)
        assert np.isfinite(v).all() and np.isfinite(n).all()
        assert (v >= lo).all() and (v <= hi).all(), (sk.name, sk.key, "a skinned vertex leaves the creation-time root box")
        return sk.ids, v, n


class OracleSide(_OracleSide):
    """The oracle's side of a pose: set_geometry of tests/emitter_edits.py with the arrays of rs_skin_corners."""

    def __init__(self, capi, name, key, W, H, **kw):
        super().__init__(capi, scene_data(name), W, H, **kw)
        self.palette = Palette(capi, name, key)

    def set_bone_transforms(self, bone_ids, matrices):
        if len(bone_ids):
            self.set_geometry(*self.palette.set(bone_ids, matrices))


class HipSide(_HipSide):
    def __init__(self, capi, name, key, W, H, **kw):
        super().__init__(capi, scene_data(name), W, H, **kw)
        skin_of(name, key).define(self.r.scene)

    def set_bone_transforms(self, bone_ids, matrices):
        self.r.scene.set_bone_transforms(bone_ids, matrices)
