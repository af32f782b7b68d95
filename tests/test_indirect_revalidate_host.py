"""ReSTIR-GI's revalidation without a GPU: the per-slot class function of restir_amd/csrc/rs_indirect_revalidate.h
(rs_debug_indirect_candidate_classes) against the NumPy restatement of tests/indirect_revalidate.py, bit for bit; and, from the CPU oracle
alone, that the move the GPU tests make is not vacuous: slots of every class exist, and dropping them changes the next frame."""
import numpy as np
import pytest

from oracle import binding as ob
from restir_amd import capi
from restir_amd.ctypes_structs import INDIRECT_RESERVOIR_DTYPE
from tests import indirect_revalidate as iv
from tests.shadow_revalidate import dirty_box

F = np.float32
BOX = np.array([[-1, -2, -3, 1, 2, 3]], F)


def slots(W, xv, xs):
    W, xv, xs = np.asarray(W, F).reshape(-1), np.asarray(xv, F).reshape(-1, 3), np.asarray(xs, F).reshape(-1, 3)
    r = np.zeros(len(W), INDIRECT_RESERVOIR_DTYPE)
    r["weight"], r["xv"], r["xs"], r["numSamples"] = W, xv, xs, 3
    r["Lo"] = 1
    return r


def both(resv, boxes, everything=False):
    got, want = capi.indirect_candidate_classes(resv, boxes, everything), iv.classes(resv, boxes, everything)
    assert got.dtype == want.dtype == np.uint8 and np.array_equal(got, want), (got, want)
    return got


def test_weights():
    """0, -0, a denormal, negative, NaN, both infinities, an ordinary one: only the denormal and the ordinary one are examined."""
    W = np.array([0.0, -0.0, 1e-42, -1.0, np.nan, np.inf, -np.inf, 0.5], F)
    n = len(W)
    inside = both(slots(W, np.full((n, 3), 9, F), np.zeros((n, 3), F)), BOX)
    assert inside.tolist() == [0, 0, 1, 0, 0, 0, 0, 1]
    through = both(slots(W, np.full((n, 3), 9, F), np.full((n, 3), -9, F)), BOX)
    assert through.tolist() == [0, 0, 2, 0, 0, 0, 0, 2]
    away = both(slots(W, np.full((n, 3), 9, F), np.full((n, 3), 8, F)), BOX)
    assert away.tolist() == [0, 0, 3, 0, 0, 0, 0, 3]
    assert both(slots(W, np.full((n, 3), 9, F), np.full((n, 3), 8, F)), BOX, True).tolist() == [0, 0, 1, 0, 0, 0, 0, 1]


def test_equal_points_are_not_examined():
    """xv == xs on all three components, IEEE ==: +0 equals -0; one differing component is enough; a NaN equals nothing."""
    xv = np.array([[0, 0, 0], [0.0, 0, 0], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [np.nan, 0, 0]], F)
    xs = np.array([[0, 0, 0], [-0.0, -0.0, 0], [0.5, 0.5, 0.5], [0.5, 0.5, np.nextafter(F(0.5), F(1))], [np.nan, 0, 0]], F)
    assert both(slots(np.ones(5, F), xv, xs), BOX).tolist() == [0, 0, 0, 1, 3]
    assert both(slots(np.ones(5, F), xv, xs), BOX, True).tolist() == [0, 0, 0, 1, 1]


def test_closed_boxes_and_nan_coordinates():
    """xs on a face and on a corner is inside; one ulp outside is not -- the segment from inside the box's reach then walks; a NaN
    coordinate lies in no box and overlaps none."""
    out = np.nextafter(F(1), F(2))
    xs = np.array([[1, 0, 0], [1, 2, 3], [-1, -2, -3], [out, 0, 0], [np.nan, 0, 0], [0, np.nan, 0]], F)
    xv = np.array([[5, 5, 5], [5, 5, 5], [5, 5, 5], [5, 0, 0], [5, 5, 5], [0, 0, 0]], F)
    assert both(slots(np.ones(6, F), xv, xs), BOX).tolist() == [1, 1, 1, 3, 3, 3]
    xv[3] = [0.5, 0, 0]                                      # the same end point, reached from inside the box
    assert both(slots(np.ones(6, F), xv, xs), BOX).tolist() == [1, 1, 1, 2, 3, 3]
    nan_xv = slots([1.0], [[np.nan, 0, 0]], [[0, 0, 0]])     # xs inside: stale whatever xv is
    assert both(nan_xv, BOX).tolist() == [1]
    nan_xv["xs"] = [[4, 0, 0]]
    assert both(nan_xv, BOX).tolist() == [3]


def test_a_segment_that_touches_a_box_at_one_point_walks():
    xv = np.array([[1, 2, 3], [2, 3, 4], [1, 5, 5], [np.nextafter(F(1), F(2)), 2, 3]], F)
    xs = np.array([[2, 3, 4], [1, 2, 3], [4, 2, 3], [2, 3, 4]], F)
    assert both(slots(np.ones(4, F), xv, xs), BOX).tolist() == [2, 1, 2, 3]


def test_eight_boxes_and_none():
    boxes = np.array([[k, k, k, k + 0.5, k + 0.5, k + 0.5] for k in range(8)], F)
    xs = np.array([[k + 0.25] * 3 for k in range(9)], F)     # one point in every box, and one beyond the last
    xv = np.full((9, 3), -5, F)
    assert both(slots(np.ones(9, F), xv, xs), boxes).tolist() == [1] * 8 + [2]
    assert both(slots(np.ones(9, F), xv, xs), boxes[:3]).tolist() == [1] * 3 + [2] * 6
    assert both(slots(np.ones(9, F), xv, xs), np.zeros((0, 6), F)).tolist() == [3] * 9
    assert both(slots(np.ones(9, F), xv, xs), np.zeros((0, 6), F), True).tolist() == [1] * 9
    assert len(capi.indirect_candidate_classes(np.zeros(0, INDIRECT_RESERVOIR_DTYPE), boxes)) == 0
    lib = capi.lib()
    assert lib.rs_debug_indirect_candidate_classes(1, None, 0, None, 0, None) == capi.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_debug_indirect_candidate_classes(0, None, 9, None, 0, None) == capi.RS_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("m", [1, 3, 8])
def test_random_slots(m):
    """4 096 slots around m random boxes, with special weights and coordinates sprinkled in."""
    rng = np.random.default_rng(40 + m)
    n = 4096
    lo = rng.uniform(-1, 0.5, (m, 3)).astype(F)
    boxes = np.concatenate([lo, lo + rng.uniform(0.05, 0.6, (m, 3)).astype(F)], 1)
    W = rng.uniform(-0.2, 2, n).astype(F)
    W[rng.integers(0, n, 200)] = rng.choice(np.array([0, -0.0, np.nan, np.inf, -np.inf, 1e-40], F), 200)
    xv, xs = rng.uniform(-1.5, 1.5, (n, 3)).astype(F), rng.uniform(-1.5, 1.5, (n, 3)).astype(F)
    k = rng.integers(0, n, 300)
    xs[k] = xv[k]
    k = rng.integers(0, n, 300)                              # end points on faces and corners
    xs[k] = boxes[rng.integers(0, m, 300)].reshape(-1, 2, 3)[np.arange(300)[:, None], rng.integers(0, 2, (300, 3)), np.arange(3)]
    xs[rng.integers(0, n, 50), rng.integers(0, 3, 50)] = np.nan
    xv[rng.integers(0, n, 50), rng.integers(0, 3, 50)] = np.nan
    got = both(slots(W, xv, xs), boxes)
    assert all((got == c).sum() >= 64 for c in range(4)), np.bincount(got, minlength=4)
    everything = both(slots(W, xv, xs), boxes, True)
    assert np.array_equal(everything != 0, got != 0) and not (everything == iv.WALK).any() and not (everything == iv.KEPT).any()


# ---- from the oracle alone: the GPU tests' move is not vacuous -------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["full", "partial"])
def test_the_move_leaves_slots_of_every_class(size):
    """cornell, depth 4, reuse 1, looper = frame number: after the warm frames and the move of the tall box the history holds at least 16
    slots that are stale, walked and occluded, walked and free, and examined but out of the box's reach; and the next frame with them
    dropped differs from the frame without the patch in at least 16 pixels.
    Measured: 64x48 after 10 frames 582 / 151 / 439 / 1 386, 465 pixels; 40x24 after 6 frames 128 / 60 / 110 / 348, 115 pixels."""
    ob.set_libm_mode(1)
    try:
        images = {}
        for patched in (True, False):
            o = iv.OracleGI(capi, iv.scene_data("cornell"), *iv.SIZES[size])
            for _ in range(iv.WARM[size]):
                o.render(); o.finish(1)
            ids, v = iv.moved_box(o.sd, o.scene.vertices)
            box = np.concatenate(dirty_box(o.scene.vertices, ids, v))[None].astype(F)
            o.set_geometry(ids, v)
            if patched:
                cls, occluded, dropped = iv.revalidate(o.scene, o.restir.ind_last, box)
                iv.drop(o.restir.ind_last, dropped)
            o.render(); o.finish(1)
            images[patched] = o.image.copy()
        stale, occ, free, kept = (cls == iv.STALE).sum(), occluded.sum(), ((cls == iv.WALK) & ~occluded).sum(), (cls == iv.KEPT).sum()
        changed = (images[True].view(np.uint32) != images[False].view(np.uint32)).any(1).sum()
        print("%s: stale %d, occluded %d, walked and free %d, kept %d; pixels changed %d" % (size, stale, occ, free, kept, changed))
        assert min(stale, occ, free, kept) >= 16
        assert changed >= 16
    finally:
        ob.set_libm_mode(0)
