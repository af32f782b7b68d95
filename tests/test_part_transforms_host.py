"""CPU: the host pieces of rigid parts.  rs_bake_matrix against rs_bake_instance and against a NumPy restatement, bit for bit;
non-finite results; rs_scene_file_objects on the committed scene file (tests/golden/scene_files.npz); the argument refusals.
The device side is tests/test_gpu_part_transforms.py."""
import ctypes as C
import os

import numpy as np
import pytest

from restir_amd import capi
from tests import part_transforms as pt
from tests import scene_file_cases as cases
from tests.common import bits_equal

F = np.float32
GOLD = os.path.join(os.path.dirname(__file__), "golden", "scene_files.npz")
INVALID = 10001                                          # RS_ERR_INVALID_ARGUMENT


def corners(seed, n=40):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-3, 3, (n, 3)).astype(F)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    nrm[::5] *= F(2.5)                                   # some are not unit
    return v, nrm


EDGE_TRS = {
    "identity": ((0, 0, 0), (0, 0, 0), (1, 1, 1)),
    "negative_scale": ((0.5, -1, 2), (10, 20, 30), (-1.5, -0.5, -2)),
    "mirrored": ((0, 0, 0), (0, 0, 0), (-1, 1, 1)),
    "rotate_0": ((1, 2, 3), (0, 0, 0), (1, 1, 1)),
    "rotate_90": ((1, 2, 3), (90, 0, 0), (1, 1, 1)),
    "rotate_180": ((1, 2, 3), (0, 180, 0), (1, 1, 1)),
    "rotate_90_each": ((0, 0, 0), (90, 90, 90), (1, 2, 3)),
    "scale_2^-20": ((0, 0, 0), (15, 0, 0), (2.0 ** -20,) * 3),
    "scale_2^20": ((0, 0, 0), (0, 25, 0), (2.0 ** 20,) * 3),
    "translate_1e6": ((1e6, -1e6, 1e6), (5, 6, 7), (1, 1, 1)),
}


def random_trs(seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-5, 5, 3), rng.uniform(-180, 180, 3), rng.uniform(0.2, 3, 3) * rng.choice([-1, 1], 3)


def assert_bake_agrees(t, r, s, v, n, tag):
    m = capi.build_transformation_matrix(t, r, s)
    a = capi.bake_instance(t, r, s, v, n)
    b = capi.bake_matrix(m, v, n)
    c = pt.numpy_bake(m, v, n)
    for k, what in enumerate(("vertices", "normals")):
        assert bits_equal(a[k], b[k]), (tag, what, "rs_bake_instance")
        assert bits_equal(c[k], b[k]), (tag, what, "the NumPy restatement")
    assert np.isfinite(b[0]).all() and np.isfinite(b[1]).all(), tag


@pytest.mark.parametrize("seed", range(8))
def test_bake_matrix_equals_bake_instance_random(seed):
    v, n = corners(seed)
    assert_bake_agrees(*random_trs(100 + seed), v, n, seed)


@pytest.mark.parametrize("case", sorted(EDGE_TRS))
def test_bake_matrix_equals_bake_instance_edge(case):
    v, n = corners(7)
    assert_bake_agrees(*EDGE_TRS[case], v, n, case)


def test_bake_matrix_of_no_corners():
    m = capi.build_transformation_matrix(*EDGE_TRS["negative_scale"])
    v, n = capi.bake_matrix(m, np.zeros((0, 3), F), np.zeros((0, 3), F))
    assert v.shape == (0, 3) and n.shape == (0, 3)
    # n == 0 asks for no array at all
    capi.check(capi.lib().rs_bake_matrix(m.ctypes.data_as(C.c_void_p), 0, None, None, None, None))


def test_identity_is_not_a_copy():
    """The contract of the identity: m * vec4(v, 1) adds +0 terms, so a -0 coordinate comes back as +0 (and nothing else changes), and the
    normal is normalised whatever its length was."""
    v = np.array([[-0.0, 1.5, -2.0], [3.0, -0.0, -0.0], [-1.0, -2.0, -3.0]], F)
    n = np.array([[0.0, 3.0, 4.0], [2.0, 0.0, 0.0], [0.0, 0.0, 1.0]], F)
    bv, bn = capi.bake_matrix(pt.identity(), v, n)
    want = v.copy()
    want[v == 0] = 0.0                                   # +0
    assert bits_equal(bv, want)
    assert not bits_equal(bv, v)
    assert bits_equal(bn[2], n[2])
    assert np.array_equal(bn[1], [1.0, 0.0, 0.0])
    assert not np.array_equal(bn[0], n[0]) and abs(float(np.linalg.norm(bn[0].astype(np.float64))) - 1.0) < 1e-6
    assert bits_equal(bn, pt.numpy_bake(pt.identity(), v, n)[1])


def test_non_finite_results_are_returned_not_refused():
    v, n = corners(3, 6)
    singular = capi.build_transformation_matrix((0, 0, 0), (0, 0, 0), (1, 0, 1))
    bv, bn = capi.bake_matrix(singular, v, n)
    assert np.isfinite(bv).all() and not np.isfinite(bn).any()
    bad = pt.identity()
    bad[3, 0] = np.nan                                   # the translation's x
    bv, bn = capi.bake_matrix(bad, v, n)
    assert np.isnan(bv[:, 0]).all() and np.isfinite(bv[:, 1:]).all()
    assert not np.isfinite(bn).all()                     # the inverse of a matrix with a NaN entry


def test_bake_matrix_refusals():
    L = capi.lib()
    m = pt.identity()
    v, n = corners(1, 3)
    vo, no = np.zeros_like(v), np.zeros_like(n)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    good = [p(m), 3, p(v), p(n), p(vo), p(no)]
    assert L.rs_bake_matrix(*good) == 0
    for k in (0, 2, 3, 4, 5):
        args = list(good)
        args[k] = None
        assert L.rs_bake_matrix(*args) == INVALID, k
        assert b"rs_bake_matrix" in L.rs_last_error()
    args = list(good)
    args[1] = -1
    assert L.rs_bake_matrix(*args) == INVALID


# ---- rs_scene_file_objects ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_path(tmp_path_factory):
    g = np.load(GOLD)
    d = tmp_path_factory.mktemp("part_scene_case")
    for name in cases.CASE_FILES:
        (d / name).write_bytes(g["file_" + name].tobytes())
    return str(d / "scene.txt")


def test_scene_file_objects(scene_path):
    a = capi.SceneFile(scene_path)
    n = len(a.vertices)
    assert a.num_skipped_objects == 1                    # the skipped object is not among them
    assert len(a.objects) == 8                           # floor, walls, five instances of cube.obj, the lamp
    first = a.object_first
    assert first[0] == 0 and first[-1] == n and (np.diff(first) > 0).all()
    for i, o in enumerate(a.objects):
        assert (o["first"], o["count"]) == (first[i], first[i + 1] - first[i])
        bv, bn = capi.bake_matrix(o["transform"], o["vertices"], o["normals"])
        sl = slice(o["first"], o["first"] + o["count"])
        assert bits_equal(bv.reshape(-1, 3, 3), a.vertices[sl]), i
        assert bits_equal(bn.reshape(-1, 3, 3), a.normals[sl]), i
    cubes = a.objects[2:7]
    assert len({o["mesh"] for o in cubes}) == 1          # one mesh file, one mesh
    assert all(bits_equal(o["vertices"], cubes[0]["vertices"]) and bits_equal(o["normals"], cubes[0]["normals"]) for o in cubes)
    assert len({o["mesh"] for o in a.objects}) == 4
    # the load-time matrix is Math::buildTransformationMatrix of the block's Translate / Rotate / Scale (b1 of tests/scene_file_cases.py)
    assert bits_equal(cubes[0]["transform"], capi.build_transformation_matrix((-0.3, 0.6, -0.3), (0, 17.5, 0), (0.55, 1.2, 0.55)))
    # ... and a new pose of the object has the bits the loader would have produced for it
    t, r, s = (0.1, 0.7, -0.2), (5, 40, -3), (0.5, 1.0, 0.6)
    re = capi.bake_matrix(capi.build_transformation_matrix(t, r, s), cubes[0]["vertices"], cubes[0]["normals"])
    loader = capi.bake_instance(t, r, s, cubes[0]["vertices"].reshape(-1, 3), cubes[0]["normals"].reshape(-1, 3))
    assert bits_equal(re[0], loader[0]) and bits_equal(re[1], loader[1])


def test_scene_file_objects_refusals(scene_path):
    L = capi.lib()
    h = C.c_void_p()
    capi.check(L.rs_scene_file_load(os.fsencode(scene_path), C.byref(h)))
    try:
        count, ptrs = C.c_int(0), [C.c_void_p() for _ in range(4)]
        good = [h, C.byref(count)] + [C.byref(q) for q in ptrs]
        assert L.rs_scene_file_objects(*good) == 0 and count.value == 8
        for k in range(6):
            args = list(good)
            args[k] = None
            assert L.rs_scene_file_objects(*args) == INVALID, k
            assert b"rs_scene_file_objects" in L.rs_last_error()
    finally:
        L.rs_scene_file_free(h)
