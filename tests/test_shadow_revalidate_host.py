"""No GPU: the device-free half of shadow revalidation (restir_amd/csrc/rs_revalidate_plan.h through its rs_debug_plan_* hooks) against
the NumPy restatement of tests/shadow_revalidate.py -- the dirty box of an edit, the ring and the frame's choice, the segment test -- and,
from the oracle alone, that the move the GPU tests make is not vacuous: segments that were free are blocked after it, and segments miss
its dirty box."""
import functools

import numpy as np
import pytest

from restir_amd import capi
from tests import shadow_revalidate as sv
from tests.common import OracleRenderer
from tests.emitter_edits import edited_oracle_scene, scene_data
from tests.geometry_edits import root_box
from tests.motion_vectors import center_rays
from tests.part_transforms import parts_of

F = np.float32


def same_box(got, want):
    """min and max are comparisons: -0 and +0 are the same bound, so values are compared (np.array_equal: -0 == +0)."""
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].dtype == F


# ---- the dirty box of an edit -------------------------------------------------------------------------------------------------------------
def test_dirty_box_of_one_triangle_and_of_a_part():
    sd = scene_data("cornell")
    old = sd.vertices.reshape(-1, 3, 3)
    ids, v = sv.moved_box(sd, old, ids=sv.TALL_BOX[:1])
    lo, hi = capi.plan_dirty_box(old, ids, v)
    assert same_box((lo, hi), sv.dirty_box(old, ids, v))
    pts = np.concatenate([old[ids[0]], v[0]])
    assert np.array_equal(lo, pts.min(0)) and np.array_equal(hi, pts.max(0))
    box = np.asarray(parts_of("cornell")[0][1], np.int32)      # the tall box as the part the GPU test transforms
    assert np.array_equal(box, sv.TALL_BOX)
    ids, v = sv.moved_box(sd, old)
    assert same_box(capi.plan_dirty_box(old, ids, v), sv.dirty_box(old, ids, v))
    rl, rh = root_box(old)
    lo, hi = capi.plan_dirty_box(old, ids, v)
    assert (lo >= rl).all() and (hi <= rh).all() and (hi - lo > sv.DISPLACEMENT).all()


def test_dirty_box_of_repeated_ids_takes_the_last_record():
    rng = np.random.default_rng(4)
    old = rng.uniform(-1, 1, (9, 3, 3)).astype(F)
    ids = np.array([3, 5, 3, 7, 5, 3], np.int32)
    v = rng.uniform(-1, 1, (len(ids), 3, 3)).astype(F)
    v[0] = 50; v[1] = -50; v[2] = 70                          # records that later ones replace: they must not widen the box
    lo, hi = capi.plan_dirty_box(old, ids, v)
    pts = np.concatenate([old[[3, 5, 7]].reshape(-1, 3), v[[5, 4, 3]].reshape(-1, 3)])
    assert np.array_equal(lo, pts.min(0)) and np.array_equal(hi, pts.max(0))
    assert same_box((lo, hi), sv.dirty_box(old, ids, v))
    assert hi.max() < 2 and lo.min() > -2
    with pytest.raises(capi.RestirHipError):
        capi.plan_dirty_box(old, np.array([9], np.int32), v[:1])


def test_dirty_box_with_signed_zeros():
    old = np.zeros((2, 3, 3), F)
    old[0, :, 0] = (-0.0, 0.0, -0.0); old[0, :, 1] = (-1, -0.0, 0.0); old[0, :, 2] = (0.0, 1, -0.0)
    v = np.zeros((1, 3, 3), F)
    v[0, :, 0] = (0.0, -0.0, 0.0); v[0, :, 1] = (-0.0, -0.0, -0.0); v[0, :, 2] = (-0.0, 0.0, 0.5)
    lo, hi = capi.plan_dirty_box(old, [0], v)
    assert same_box((lo, hi), sv.dirty_box(old, [0], v))
    assert np.array_equal(lo, [0, -1, 0]) and np.array_equal(hi, [0, 0, 1])
    # whichever zero the bound carries, the segment test sees the same box
    seg = np.array([[0.0, -0.5, 0.5, -0.0, -0.5, 0.5], [-0.0, 0.0, 0.0, -0.0, -0.0, -0.0]], F)
    for z in (0.0, -0.0):
        b = np.array([[z, -1, z, z, z, 1]], F)
        assert capi.segment_in_boxes(seg, b).all() and sv.segment_in_boxes(seg, b).all()


# ---- the ring and the frame's choice --------------------------------------------------------------------------------------------------------
def boxes_of(count, seed=2):
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-1, 0, (count, 3))
    return np.concatenate([lo, lo + rng.uniform(0.1, 1, (count, 3))], 1).astype(F)


def restated(boxes, seen, now, same=True):
    ring = sv.DirtyRing()
    for b in boxes[:now]:
        ring.edits += 1
        ring.kept = (ring.kept + [(ring.edits, b)])[-sv.KEPT:]
    return ring.choose(seen, same)


@pytest.mark.parametrize("edits,seen,want", [
    (0, 0, (False, False, 0)), (5, 5, (False, False, 0)),     # no edit: no launch
    (1, 0, (True, False, 1)), (8, 0, (True, False, 8)), (9, 0, (True, True, 0)),     # 1, 8 and 9 edits in the gap
    (12, 4, (True, False, 8)), (12, 3, (True, True, 0)),     # an rs_restir that lags while the ring turns over: 12 edits keep 5 .. 12
    (12, 11, (True, False, 1)), (20, 2, (True, True, 0))])
def test_ring_and_choice(edits, seen, want):
    boxes = boxes_of(edits)
    launch, everything, out = capi.plan_revalidation(boxes, seen, edits)
    assert (launch, everything, len(out)) == want
    r = restated(boxes, seen, edits)
    assert (launch, everything) == r[:2] and np.array_equal(out, r[2])
    if not everything:
        assert np.array_equal(out, boxes[seen:edits])            # the boxes of the edits seen + 1 .. now, oldest first


def test_choice_for_another_scene_and_after_switch_on():
    boxes = boxes_of(3)
    for seen in (0, 3):                                      # another scene: everything, whatever its count of edits
        assert capi.plan_revalidation(boxes, seen, 3, same_scene=False)[:2] == (True, True)
        assert restated(boxes, seen, 3, same=False)[:2] == (True, True)
    # switch-on takes the edits made so far as seen: the frame after it chooses with seen = now, and the first edit after it is one box
    assert capi.plan_revalidation(boxes, 3, 3)[:2] == (False, False)
    more = boxes_of(4)
    launch, everything, out = capi.plan_revalidation(more, 3, 4)
    assert (launch, everything) == (True, False) and np.array_equal(out, more[3:])
    # edit numbers need not start at 1 for the ring (a lagging reader of a ring that starts later sees "everything")
    assert capi.plan_revalidation(boxes, 5, 8, first_edit=6)[:2] == (True, False)
    assert capi.plan_revalidation(boxes, 4, 8, first_edit=6)[:2] == (True, True)
    lib = capi.lib()
    assert lib.rs_scene_geometry_edits(None, None) == capi.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_scene_dirty_boxes(None, 0, 0, None, None, None) == capi.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_restir_set_shadow_revalidation(None, 1) == capi.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_restir_get_shadow_revalidation(None, None) == capi.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_debug_restir_revalidate(None, None) == capi.RS_ERR_INVALID_ARGUMENT
    assert lib.rs_debug_restir_revalidate_launched(None, None) == capi.RS_ERR_INVALID_ARGUMENT
    assert capi.DIRTY_BOXES_KEPT == sv.KEPT


# ---- the segment test -------------------------------------------------------------------------------------------------------------------------
def test_segment_test_cases():
    box = np.array([[0, 0, 0, 1, 1, 1]], F)
    cases = [
        ((.2, .2, .2, .8, .8, .8), True),                      # inside
        ((.2, .2, .2, 3, 3, 3), True),                         # leaves the box
        ((1, .5, .5, 2, .5, .5), True),                        # touches a face from outside: closed intervals
        ((-1, .5, .5, 0, .5, .5), True),
        ((1, 1, 1, 2, 2, 2), True),                            # touches a corner
        # Passes a corner's bounding box without touching the box: the segment (1.5, 0.9) -> (0.9, 1.5) stays outside x, y <= 1, but its
        # own bounding box overlaps.  It walks: the test is conservative on purpose (a slab test is out of scope).
        ((1.5, .9, .5, .9, 1.5, .5), True),
        ((1.5, .5, .5, 2.5, .5, .5), False),                   # beside the box
        ((.5, .5, 1.0001, .5, .5, 2), False),
        ((-3, -3, -3, -.0001, 5, 5), False),
        ((.5, .5, .5, .5, .5, .5), True),                      # a point inside
    ]
    seg = np.array([c[0] for c in cases], F)
    want = np.array([c[1] for c in cases])
    for s in (seg, seg[:, [3, 4, 5, 0, 1, 2]]):                # ... and with the endpoints reversed
        assert np.array_equal(capi.segment_in_boxes(s, box), want)
        assert np.array_equal(sv.segment_in_boxes(s, box), want)
    # a NaN coordinate never walks, wherever it stands
    for k in range(6):
        s = seg[:6].copy()
        s[:, k] = np.nan
        assert not capi.segment_in_boxes(s, box).any() and not sv.segment_in_boxes(s, box).any()
    assert not capi.segment_in_boxes(seg, np.zeros((0, 6), F)).any()     # no box: nothing walks
    s = seg.copy()
    s[0, 0] = np.nan
    assert capi.segment_in_boxes(s, box, everything=True).all() and sv.segment_in_boxes(s, box, everything=True).all()      # everything
    with pytest.raises(capi.RestirHipError):
        capi.segment_in_boxes(seg, np.zeros((9, 6), F))


def test_segment_test_against_numpy_on_random_segments():
    rng = np.random.default_rng(8)
    boxes = boxes_of(8, seed=5)
    seg = rng.uniform(-1.5, 1.5, (20000, 6)).astype(F)
    seg[:4000, 3:] = seg[:4000, :3] + rng.normal(size=(4000, 3)).astype(F) * F(0.05)       # short ones
    faces = rng.integers(0, 8, 2000)
    seg[4000:6000, 0] = boxes[faces, 3]                          # an endpoint exactly on a box's face
    seg[6000:7000, 4] = boxes[faces[:1000], 1]
    seg[7000:7100, rng.integers(0, 6, 100)] = np.nan
    seg[7100:7200, 0] = np.inf
    for m in (1, 3, 8):
        got, want = capi.segment_in_boxes(seg, boxes[:m]), sv.segment_in_boxes(seg, boxes[:m])
        assert np.array_equal(got, want)
        assert 0.05 < want.mean() < 0.95


# ---- the GPU tests' move is not vacuous: from the oracle alone ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def warm_cornell():
    sd = scene_data("cornell")
    W, H = 64, 48
    o = OracleRenderer(sd, W, H)
    for _ in range(10):
        o.frame(3)
    prim, _, pos, _, _ = o.scene.intersect(center_rays(o.cam, W, H))
    last = o.restir.last
    return sd, o, prim >= 0, sv.segments_of(pos, last, np.arange(W * H)), last["weight"] != 0


def test_the_move_blocks_segments_that_were_free():
    sd, o, hit, seg, weighted = warm_cornell()
    ids, v = sv.moved_box(sd, o.scene.vertices)
    assert np.array_equal(ids, sv.TALL_BOX) and np.array_equal(v - o.scene.vertices.reshape(-1, 3, 3)[ids], np.broadcast_to(sv.DISPLACEMENT, v.shape))
    before = o.scene.test_occlusion(seg) != 0
    after = edited_oracle_scene(capi, o.scene, ids, v).test_occlusion(seg) != 0
    newly = hit & weighted & ~before & after
    print("segments free before the move and occluded after it:", int(newly.sum()))
    assert newly.sum() >= 16


def test_the_dirty_box_of_the_move_filters():
    sd, o, hit, seg, weighted = warm_cornell()
    ids, v = sv.moved_box(sd, o.scene.vertices)
    lo, hi = capi.plan_dirty_box(o.scene.vertices, ids, v)
    inside = capi.segment_in_boxes(seg, np.concatenate([lo, hi])[None])
    assert np.array_equal(inside, sv.segment_in_boxes(seg, np.concatenate([lo, hi])[None]))
    missing = hit & weighted & ~inside
    print("segments with W != 0 that miss the dirty box:", int(missing.sum()), "that cross it:", int((hit & weighted & inside).sum()))
    assert missing.sum() >= 16 and (hit & weighted & inside).sum() >= 16
    # a segment that misses the box keeps its answer
    before = o.scene.test_occlusion(seg[missing]) != 0
    after = edited_oracle_scene(capi, o.scene, ids, v).test_occlusion(seg[missing]) != 0
    assert np.array_equal(before, after)
