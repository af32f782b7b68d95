"""CPU: the host pieces of skinned meshes.  rs_skin_corners against a NumPy restatement of rs_bake.h's skin_corner, bit for bit, and
against rs_bake_matrix in the rigid case; non-finite results; the argument refusals; and that the poses the GPU tests make keep every
skinned vertex inside the box their scene was created with.  The device side is tests/test_gpu_skinning.py."""
import ctypes as C

import numpy as np
import pytest

from restir_amd import capi
from tests import part_transforms as pt
from tests import skinning as sk
from tests.common import bits_equal
from tests.test_part_transforms_host import corners, random_trs

F = np.float32
INVALID = 10001                                          # RS_ERR_INVALID_ARGUMENT
BONES = 5


def palette(seed, count=BONES):
    return np.stack([capi.build_transformation_matrix(*random_trs(1000 * seed + b)) for b in range(count)])


def assert_restated(m, v, n, b, w, tag):
    got, want = capi.skin_corners(m, v, n, b, w), sk.numpy_skin(m, v, n, b, w)
    assert bits_equal(got[0], want[0]), (tag, "vertices")
    assert bits_equal(got[1], want[1]), (tag, "normals")
    return got


@pytest.mark.parametrize("seed", range(8))
def test_skin_corners_equals_the_restatement_random(seed):
    v, n = corners(seed)
    b, w = sk.random_influences(np.random.default_rng(50 + seed), len(v), BONES)
    got = assert_restated(palette(seed), v, n, b, w, seed)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()


def edge_weights(case, count):
    rng = np.random.default_rng(9)
    b = rng.integers(0, BONES, (count, 4)).astype(np.int32)
    w = rng.uniform(0.1, 1.0, (count, 4)).astype(F)
    w /= w.sum(1, keepdims=True)
    if case == "slot_3_only":
        w[:, :3] = 0.0
        w[:, 3] = 1.0
    elif case == "four_equal":
        w[:] = 0.25
    elif case == "denormal":                             # 2^-140 next to ordinary weights, and alone (the sum then is a denormal's product)
        w[:, 1] = F(2.0 ** -140)
        w[::4, [0, 2, 3]] = 0.0
    elif case == "sum_half":
        w *= F(0.5)
    elif case == "sum_two":
        w *= F(2.0)
    elif case == "same_bone":
        b[:] = b[:, :1]
    else:
        raise KeyError(case)
    return b, w


@pytest.mark.parametrize("case", ["slot_3_only", "four_equal", "denormal", "sum_half", "sum_two", "same_bone"])
def test_skin_corners_equals_the_restatement_edge(case):
    v, n = corners(7)
    b, w = edge_weights(case, len(v))
    assert w.dtype == F
    if case == "denormal":
        assert 0 < w[0, 1] < np.finfo(F).tiny
    if case in ("sum_half", "sum_two"):
        assert np.allclose(w.sum(1), 0.5 if case == "sum_half" else 2.0, rtol=1e-6)
    got = assert_restated(palette(3), v, n, b, w, case)
    assert np.isfinite(got[0]).all()
    if case in ("sum_half", "sum_two"):                  # used as given, not renormalised: the position scales with the sum
        full = capi.skin_corners(palette(3), v, n, b, w / w.sum(1, keepdims=True))
        assert np.allclose(got[0], full[0] * w.sum(1)[:, None], rtol=1e-5, atol=1e-5)
        assert not np.allclose(got[0], full[0], rtol=1e-3)


@pytest.mark.parametrize("slot", range(4))
def test_one_influence_equals_bake_matrix(slot):
    """One influence of weight 1, the other three slots at weight 0 on finite bones: the values of rs_bake_matrix.  np.array_equal, i.e.
    value equality, not bits: the blend adds the other slots' products, which are zeros of either sign, so a component that rs_bake_matrix
    returns as -0 comes back as +0 (-0 + +0 = +0).  Nothing else can differ: 1 * p is p, and p + 0 is p."""
    v, n = corners(11)
    v[3] = 0.0                                           # a corner at the origin under a pure rotation: zeros of both signs in the position
    ms = palette(4)
    ms[2] = capi.build_transformation_matrix((0, 0, 0), (0, 180, 0), (1, 1, 1))
    rng = np.random.default_rng(slot)
    b = rng.integers(0, BONES, (len(v), 4)).astype(np.int32)
    b[3, slot] = 2
    w = np.zeros((len(v), 4), F)
    w[:, slot] = 1.0
    got = capi.skin_corners(ms, v, n, b, w)
    for i in range(len(v)):
        want = capi.bake_matrix(ms[b[i, slot]], v[i:i + 1], n[i:i + 1])
        assert np.array_equal(got[0][i], want[0][0]) and np.array_equal(got[1][i], want[1][0]), (slot, i)
    assert bits_equal(got[0], sk.numpy_skin(ms, v, n, b, w)[0])


def test_skin_corners_of_no_corners():
    m = palette(1)
    v, n = capi.skin_corners(m, np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros((0, 4), np.int32), np.zeros((0, 4), F))
    assert v.shape == (0, 3) and n.shape == (0, 3)
    # n == 0 asks for no array but the matrices
    capi.check(capi.lib().rs_skin_corners(BONES, m.ctypes.data_as(C.c_void_p), 0, None, None, None, None, None, None))


def test_non_finite_results_are_returned_not_refused():
    v, n = corners(3, 6)
    b = np.zeros((6, 4), np.int32)
    b[:, 1] = 1
    w = np.tile(np.array([0.5, 0.5, 0, 0], F), (6, 1))
    ms = np.stack([pt.identity(), capi.build_transformation_matrix((0, 0, 0), (0, 0, 0), (1, 0, 1))])      # bone 1 is singular
    sv, sn = capi.skin_corners(ms, v, n, b, w)
    assert np.isfinite(sv).all() and not np.isfinite(sn).any()
    w0 = np.tile(np.array([1, 0, 0, 0], F), (6, 1))        # weight 0 on the singular bone still evaluates it: 0 * inf
    sv, sn = capi.skin_corners(ms, v, n, b, w0)
    assert np.isfinite(sv).all() and not np.isfinite(sn).any()
    assert bits_equal(sn, sk.numpy_skin(ms, v, n, b, w0)[1])
    bad = pt.identity()
    bad[3, 0] = np.nan                                   # the translation's x
    sv, sn = capi.skin_corners(np.stack([pt.identity(), bad]), v, n, b, w)
    assert np.isnan(sv[:, 0]).all() and np.isfinite(sv[:, 1:]).all()
    winf = w.copy()
    winf[2, 0] = np.inf                                  # weights are not checked here either
    sv, _ = capi.skin_corners(np.stack([pt.identity()] * 2), v, n, b, winf)
    assert not np.isfinite(sv[2]).all() and np.isfinite(np.delete(sv, 2, 0)).all()


def test_skin_corners_refusals():
    L = capi.lib()
    m = palette(2)
    v, n = corners(1, 3)
    b, w = sk.random_influences(np.random.default_rng(1), 3, BONES)
    vo, no = np.zeros_like(v), np.zeros_like(n)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    good = [BONES, p(m), 3, p(v), p(n), p(b), p(w), p(vo), p(no)]
    assert L.rs_skin_corners(*good) == 0
    for k in (1, 3, 4, 5, 6, 7, 8):                      # null matrices; each null array with n > 0
        args = list(good)
        args[k] = None
        assert L.rs_skin_corners(*args) == INVALID, k
        assert b"rs_skin_corners" in L.rs_last_error()
    for bones in (0, -1):
        args = list(good)
        args[0] = bones
        assert L.rs_skin_corners(*args) == INVALID, bones
    for bad in (BONES, -1):                              # a bone id out of range, in a slot of weight 0 too
        b2, w2 = b.copy(), w.copy()
        b2[1, 2], w2[1, 2] = bad, 0.0
        before = vo.copy()
        assert L.rs_skin_corners(BONES, p(m), 3, p(v), p(n), p(b2), p(w2), p(vo), p(no)) == INVALID, bad
        assert b"bone id" in L.rs_last_error() and bits_equal(vo, before)


def test_the_collapse_pose_is_finite_inside_the_box_and_without_light_power():
    """The pose tests/test_gpu_skinning.py has refused for the light sampler: collapse_pose asserts finite values inside the root box on
    one line; the device-free plan of the edit (rs_geometry_plan.h) refuses exactly these arrays for the sampler's power and for nothing
    earlier, under the name and with the record count rs_scene_set_bone_transforms hands it."""
    from tests.test_geometry_edit_plan import NO_POWER, refused as plan_refused, view as plan_view
    bones, ms, ids, v, n = sk.collapse_pose(capi)
    assert len(bones) == 6 and all(bits_equal(m[:3], pt.identity()[:3]) for m in ms)      # plain translations: identity normal matrices
    plan_refused(NO_POWER, "rs_scene_set_bone_transforms", 1, ids, v, n, num_part_recs=7)
    # the lamp moved as one by the same six bones is accepted
    skin = sk.skin_of("cornell", sk.LAMP_CORNERS)
    ids, v, n = sk.Palette(capi, "cornell", sk.LAMP_CORNERS).set(*sk.pose("cornell", sk.LAMP_CORNERS, 1))
    plan, _, lights = capi.plan_geometry_edit(plan_view(), "rs_scene_set_bone_transforms", 1, ids, v, n, num_part_recs=skin.num_bones)
    assert plan.lamps == 1 and plan.partStaged == 7 * 112 and lights["sumAll"] > 0


@pytest.mark.parametrize("name,key", [(n, k) for n in sk.SKINS for k in sk.SKINS[n]])
def test_the_gpu_tests_poses_stay_inside_the_root_box(name, key):
    """Every skin of tests/test_gpu_skinning.py, every step it poses: Palette.skinned() asserts finiteness and containment.  Each corner
    has 1 to 4 non-zero weights, and all four counts occur on the larger skins."""
    s = sk.skin_of(name, key)
    live = (s.weights > 0).sum(2)
    assert live.min() >= 1 and live.max() <= 4
    if name == "many" and len(s.ids) >= 21:
        assert set(np.unique(live)) == {1, 2, 3, 4}
    pal = sk.Palette(capi, name, key)
    for step in range(16):
        ids, v, n = pal.set(*sk.pose(name, key, step))
        assert len(ids) == len(v) == len(n) == len(s.ids)
        assert not bits_equal(v, s.rest_vertices)
