"""rs_morph_corners (host only, no GPU) against the NumPy restatement of rs_bake.h's morph_corner in tests/morphing.py, bit for bit: random
morphs, corners without entries and with entries of all 256 targets, targets without entries, zero, signed-zero, negative, large and
denormal weights, no normal deltas, a normal sum of exactly 0; the composition with rs_skin_corners; the refusals that need no device;
and the weight steps of tests/test_gpu_morphing.py, which keep every vertex inside its scene's creation-time root box."""
import ctypes as C

import numpy as np
import pytest

from restir_amd import capi
from tests import morphing as mo
from tests import skinning as sk
from tests.common import bits_equal

F = np.float32
INVALID = 10001                                          # RS_ERR_INVALID_ARGUMENT


def corners(seed, k):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-5, 5, (k, 3)).astype(F)
    n = rng.normal(size=(k, 3))
    return v, (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)


def table(seed, k, targets, share=0.3):
    """A random by-target table over k corners, entries of a target in random order; some targets may be empty."""
    rng = np.random.default_rng(seed)
    first, ec = [0], []
    for _ in range(targets):
        c = rng.permutation(np.flatnonzero(rng.random(k) < share))
        ec.append(c)
        first.append(first[-1] + len(c))
    ec = np.concatenate(ec).astype(np.int32)
    return (np.array(first, np.int32), ec, rng.uniform(-1, 1, (len(ec), 3)).astype(F), rng.uniform(-0.5, 0.5, (len(ec), 3)).astype(F))


def assert_restated(tab, w, v, n, tag):
    got = capi.morph_corners(*tab, w, v, n)
    want = mo.numpy_morph(*tab, w, v, n)
    assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1]), tag
    return got


@pytest.mark.parametrize("seed", range(8))
def test_morph_corners_equals_the_restatement_random(seed):
    rng = np.random.default_rng(900 + seed)
    k, targets = int(rng.integers(1, 400)), int(rng.integers(1, 40))
    v, n = corners(seed, k)
    w = rng.uniform(-1, 2, targets).astype(F)
    w[rng.random(targets) < 0.3] = 0
    assert_restated(table(seed, k, targets), w, v, n, seed)


EMPTY_TARGETS = (100, 255)


def full_table():
    """40 corners, 256 targets: corner 7 carries an entry of every target -- 256 entries --, corner 8 none, and targets 100 and 255 have
    no entry but corner 7's."""
    first, ec, dp, dn = table(3, 40, 256, share=0.2)
    out_first, out_ec = [0], []
    for t in range(256):
        c = ec[first[t]:first[t + 1]]
        c = np.array([7], np.int32) if t in EMPTY_TARGETS else np.union1d(c[(c != 7) & (c != 8)], [7]).astype(np.int32)
        out_ec.append(c)
        out_first.append(out_first[-1] + len(c))
    out_ec = np.concatenate(out_ec)
    rng = np.random.default_rng(4)
    return (np.array(out_first, np.int32), out_ec, (rng.uniform(-1, 1, (len(out_ec), 3)) / 64).astype(F),
            (rng.uniform(-1, 1, (len(out_ec), 3)) / 64).astype(F))


EDGE = ("all_targets", "zeros", "minus_zero", "negative", "two", "denormal", "no_normal_deltas", "one_nonzero")


@pytest.mark.parametrize("case", EDGE)
def test_morph_corners_equals_the_restatement_edge(case):
    tab = full_table()
    first, ec = tab[0], tab[1]
    counts = np.bincount(ec, minlength=40)
    assert counts[7] == 256 == mo.MAX_TARGETS and counts[8] == 0 and all(first[t + 1] - first[t] == 1 for t in EMPTY_TARGETS)
    v, n = corners(11, 40)
    v[3, 1], n[3, 2], v[8, 0] = -0.0, -0.0, -0.0
    rng = np.random.default_rng(12)
    w = rng.uniform(0.1, 1, 256).astype(F)
    if case == "zeros":
        w[:] = 0
    elif case == "minus_zero":
        w[::2] = -0.0
    elif case == "negative":
        w = -w
    elif case == "two":
        w[:] = 2
    elif case == "denormal":
        w[:] = F(2.0) ** -140
        assert 0 < w[0] < np.finfo(F).tiny
    elif case == "no_normal_deltas":
        tab = tab[:3] + (None,)
    elif case == "one_nonzero":
        w[:] = 0
        w[37] = 1.25
    pv, pn = assert_restated(tab, w, v, n, case)
    assert bits_equal(pv[8], v[8]) and bits_equal(pn[8], n[8])              # the corner without entries: its rest bits, the -0.0 too
    if case == "zeros":
        assert bits_equal(pv, v) and bits_equal(pn, n)
    elif case == "minus_zero":                           # skipped: the same as plain zeros in their place
        w0 = w.copy()
        w0[::2] = 0.0
        want = capi.morph_corners(*tab, w0, v, n)
        assert bits_equal(pv, want[0]) and bits_equal(pn, want[1])
        touched = np.unique(np.concatenate([ec[first[t]:first[t + 1]] for t in range(0, 256, 2)]))
        only_even = np.setdiff1d(touched, np.concatenate([ec[first[t]:first[t + 1]] for t in range(1, 256, 2)]))
        assert bits_equal(pv[only_even], v[only_even]) and bits_equal(pn[only_even], n[only_even])
    elif case == "no_normal_deltas":                     # applied corners are renormalised, not copied
        assert bits_equal(pn, mo.numpy_morph(tab[0], tab[1], tab[2], np.zeros_like(tab[2]), w, v, n)[1])
    elif case == "denormal":                             # applied, but 256 * 2^-140 / 64 is far below half an ulp of corner 7's position
        assert np.array_equal(pv[7], v[7]) and np.abs(v[7]).min() > 1e-3
    else:
        assert not bits_equal(pv[7], v[7])


@pytest.mark.parametrize("empty", [(0,), (3,), (8,), (0, 1, 8)], ids=str)
def test_targets_with_no_entry(empty):
    """Targets whose range of the table is empty -- the first, one in the middle, the last, several: whatever their weight, the result
    equals the restatement and the result without them."""
    first, ec, dp, dn = table(21, 50, 9)
    keep = np.ones(len(ec), bool)
    for t in empty:
        keep[first[t]:first[t + 1]] = False
    counts = np.array([keep[a:b].sum() for a, b in zip(first[:-1], first[1:])])
    tab = (np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), ec[keep], dp[keep], dn[keep])
    assert all(tab[0][t + 1] == tab[0][t] for t in empty)
    v, n = corners(22, 50)
    w = np.random.default_rng(23).uniform(0.2, 1.5, 9).astype(F)
    pv, pn = assert_restated(tab, w, v, n, empty)
    w0 = w.copy()
    w0[list(empty)] = 0
    qv, qn = capi.morph_corners(*tab, w0, v, n)
    assert bits_equal(pv, qv) and bits_equal(pn, qn)


def test_a_normal_sum_of_exactly_zero_is_returned_not_refused():
    v, n = np.array([[1, 2, 3], [4, 5, 6]], F), np.array([[0, 0, 1], [0, 1, 0]], F)
    tab = (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([[0.5, 0, 0]], F), np.array([[0, 0, -1]], F))
    pv, pn = assert_restated(tab, np.array([1], F), v, n, "zero sum")
    assert bits_equal(pv[0], np.array([1.5, 2, 3], F)) and not np.isfinite(pn[0]).any()
    assert bits_equal(pv[1], v[1]) and bits_equal(pn[1], n[1])
    # weights and deltas are not checked here either
    pv, _ = capi.morph_corners(*tab, np.array([np.inf], F), v, n)
    assert not np.isfinite(pv[0]).all() and bits_equal(pv[1], v[1])


def test_morph_corners_of_no_corners_and_no_targets():
    v, n = corners(1, 4)
    none = (np.array([0], np.int32), np.zeros(0, np.int32), np.zeros((0, 3), F), None)
    pv, pn = capi.morph_corners(*none, np.zeros(0, F), v, n)
    assert bits_equal(pv, v) and bits_equal(pn, n)
    tab = (np.array([0, 0], np.int32), np.zeros(0, np.int32), np.zeros((0, 3), F), np.zeros((0, 3), F))
    pv, pn = capi.morph_corners(*tab, np.ones(1, F), np.zeros((0, 3), F), np.zeros((0, 3), F))
    assert pv.shape == (0, 3) and pn.shape == (0, 3)


@pytest.mark.parametrize("seed", range(3))
def test_skin_of_morph_equals_the_restated_composition(seed):
    rng = np.random.default_rng(40 + seed)
    k, targets, bones = 120, 9, 5
    v, n = corners(seed, k)
    tab = table(50 + seed, k, targets)
    w = rng.uniform(-0.5, 1.5, targets).astype(F)
    w[2] = 0
    from tests.test_skinning_host import palette
    ms = palette(seed, bones)
    b, bw = sk.random_influences(rng, k, bones)
    got = capi.skin_corners(ms, *capi.morph_corners(*tab, w, v, n), b, bw)
    want = sk.numpy_skin(ms, *mo.numpy_morph(*tab, w, v, n), b, bw)
    assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1])


def test_by_corner_restated_on_a_small_table():
    """The conversion the device tables are held to (tests/test_gpu_morphing.py), checked by hand on four corners."""
    first, ec = [0, 2, 2, 5], [3, 0, 0, 1, 3]
    dp = np.arange(15, dtype=F).reshape(5, 3)
    cf, recs = mo.by_corner(4, first, ec, dp, None)
    assert cf.tolist() == [0, 2, 3, 3, 5]
    assert recs["target"].tolist() == [0, 2, 2, 0, 2]
    assert recs["dp"][:, 0].tolist() == [3, 6, 9, 0, 12] and not recs["dn"].any() and not recs["pad"].any()
    assert recs.dtype.itemsize == 32 and capi.MORPH_ENTRY == mo.ENTRY


def test_refusals_that_need_no_device():
    L = capi.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    v, n = corners(1, 6)
    first, ec = np.array([0, 2, 3], np.int32), np.array([0, 4, 4], np.int32)
    dp, dn, w = np.ones((3, 3), F), np.ones((3, 3), F), np.ones(2, F)
    vo, no = np.zeros_like(v), np.zeros_like(n)
    good = [2, p(first), p(ec), p(dp), p(dn), p(w), 6, p(v), p(n), p(vo), p(no)]
    assert L.rs_morph_corners(*good) == 0
    before = vo.copy()

    def refused(args, words):
        assert L.rs_morph_corners(*args) == INVALID, words
        err = L.rs_last_error()
        assert b"rs_morph_corners" in err and words in err, err
        assert bits_equal(vo, before)

    def with_(k, value):
        args = list(good)
        args[k] = value
        return args
    for k in (1, 2, 3, 5, 7, 8, 9, 10):                  # each null array but the normal deltas
        refused(with_(k, None), b"null")
    assert L.rs_morph_corners(*with_(4, None)) == 0
    refused(with_(0, -1), b"numTargets")
    big = np.zeros(258, np.int32)
    refused(with_(0, 257)[:1] + [p(big)] + good[2:], b"numTargets")
    refused(with_(1, p(np.array([1, 2, 3], np.int32))), b"first offset")
    refused(with_(1, p(np.array([0, 3, 2], np.int32))), b"decrease")
    refused(with_(2, p(np.array([0, 4, 6], np.int32))), b"corner index")
    refused(with_(2, p(np.array([0, -1, 4], np.int32))), b"corner index")
    refused(with_(2, p(np.array([4, 4, 0], np.int32))), b"listed twice")
    assert L.rs_morph_corners(*with_(2, p(np.array([4, 0, 4], np.int32)))) == 0      # the same corner in two targets is what a morph is

    # every entry point refuses a null scene before it touches a device
    one, wt = np.array([0], np.int32), np.array([0.5], F)
    ident = np.eye(4, dtype=F)
    null = [(L.rs_scene_define_morph, (None, 2, 2, p(one), None, None, p(first), p(ec), p(dp), p(dn))),
            (L.rs_scene_define_skin_morph, (None, 2, p(first), p(ec), p(dp), p(dn))),
            (L.rs_scene_set_morph_weights, (None, 1, p(one), p(wt))),
            (L.rs_scene_set_skin_pose, (None, 1, p(one), p(ident), 1, p(one), p(wt))),
            (L.rs_scene_morph_info, (None, 0, None, None, None)),
            (L.rs_scene_download_morph, (None, 0, None, None, None, None, None))]
    for fn, args in null:
        assert fn(*args) == INVALID, fn
        assert b"null" in L.rs_last_error()


ALL_MORPHS = [(n, k) for n in mo.MORPHS for k in mo.MORPHS[n]]


@pytest.mark.parametrize("name,key", ALL_MORPHS)
def test_the_gpu_tests_weight_steps_stay_inside_the_root_box(name, key):
    """Every morph of tests/test_gpu_morphing.py, every step it takes: Weights.morphed() asserts finiteness and containment, so the
    reference alone stays inside every limit the GPU tests assume.  The larger morphs have a corner with every target next to corners
    with none."""
    m = mo.morph_of(name, key)
    counts = np.bincount(m.entry_corner, minlength=m.num_corners)
    assert (np.diff(m.target_first) >= 1).all()
    if m.num_corners >= mo.FULL_FROM:
        assert counts[mo.FULL_CORNER] == m.num_targets and not counts[mo.FULL_CORNER + 1:mo.FULL_CORNER + 1 + mo.EMPTY_CORNERS].any()
    w = mo.Weights(capi, m)
    for step in range(16):
        ids, v, n = w.set(*mo.weight_step(m.num_targets, step)).morphed()
        assert len(ids) == len(v) == len(n) == len(m.ids)
        if step == 2:
            assert np.count_nonzero(w.w) == 1
    assert (w.w > 1).any() or m.num_targets < 3


@pytest.mark.parametrize("key", list(mo.SKIN_MORPHS))
def test_the_gpu_tests_skin_poses_stay_inside_the_root_box(key):
    m = mo.skin_morph_of(key)
    assert (m.entry_corner % 2 == 1).all() and (np.diff(m.target_first) >= 1).all()
    pose = mo.SkinPose(capi, key)
    for step in range(4):
        ids, v, n = pose.set(*sk.pose("many", key, step), *mo.weight_step(m.num_targets, step))
        assert len(ids) == len(v) == len(pose.palette.skin.ids)
    rest = pose.palette.skin.rest_vertices
    assert not bits_equal(pose.weights.corners(rest, pose.palette.skin.rest_normals)[0].reshape(rest.shape), rest)
