"""CPU: the camera table of tests/camera_cases.py on the oracle alone, the primary cuts' planner at the same cameras, and a mutation check
of the camera functions.

  * every row does what it is there for: the oracle's outputs at 48 x 32 (every stage of extreme_cases.STAGES) give the figures of
    camera_cases.EXPECT -- hits, lights and misses of the G-buffer, live reservoirs, the motion plane's mix, ray counts -- and hold no
    NaN and no infinity.  Once per family: the wide rows hit in at least 95 % of the pixels, fov_0's motion plane is all -1, the still
    camera of in_fov_90 does NOT reproject onto itself, the far rows hit in at least half of the pixels, looking_away and focal_1e20
    hit nothing;
  * in_fov_60 and in_fov_91 again at 97 x 61, 1 x 33, 130 x 1 and 2 x 2: every pixel of the three tiny frames hits;
  * the moving pairs: the motion plane after the first frame at camera B shows the mix of PAIR_EXPECT, and the temporal pass merges a
    reprojected reservoir (more samples than one frame draws, at a pixel whose motion entry points elsewhere) in at least 40 pixels.
    Two pairs cannot, and say why: zoom_from_0 (every reprojection divides by zero: all -1, the point of the pair) and turn_90, whose
    607 reprojected pixels all land on ANOTHER material of the last frame (camera B sees the green wall only, camera A never saw it),
    so findTemporalNeighbor refuses every one of them in the first B frame; it merges in the second, where the camera stands still
    and 607 entries still point to a neighbour (a basis from yaw 0 rounds that way) -- asserted there.  turn_10 is the turn that does
    merge across the move;
  * the cut planner (rs_debug_plan_primary_cut, the function the device builder runs) at twelve views from inside the scaled box: on
    every block that takes a cut, containment as tests/test_primary_cut_node_plan.py checks it (double-precision rays, geometric slab
    test, the cut walk visits what the tree walk visits); and WHICH views take a cut is pinned: none where |tan| or |aspect * tan|
    exceeds 16 -- 83.7, 89.99, and 90 and 91 degrees, whose tangents are negative (cut_cell compares magnitudes) --, some at 60, 83.6,
    120, -60 and 179 degrees and at focal distances of 1e-30, 1e18 and -1;
  * the blocks that take a cut for the still-camera rows of tests/test_gpu_camera_extremes.py, as that module writes them down.

Mutation check (test_a_wrong_camera_function_would_show).  camera_center_ray and camera_raster_coord restated in NumPy
(camera_cases.center_dirs, raster_coord), traced through the oracle's own intersect, reproduce the oracle's depth and motion planes; two
mutants are run against that:
  * camera_raster_coord without its `ndc * .5 + .5` step changes the motion plane -- a compared output -- of 21 rows: every row but
    fov_0 (all -1 either way), looking_away and focal_1e20 (no hit);
  * pFocus with the operands of its first product swapped, (ruv * tan) * aspect, changes the depth plane of 18 rows: in_fov_60,
    in_fov_83.6, in_fov_86.5, in_fov_89.99, in_fov_90, in_fov_91, in_fov_120, in_fov_-60, fov_neg, pitch_90, pitch_-90, yaw_0, yaw_180,
    focal_1e-20, focal_1e18, focal_neg, on_wall and at_vertex (the narrow lenses -- fov_0, fov_1e-3, far_* -- are where the product's
    rounding drowns in the view direction's 1; the test asserts at least five rows and prints the set).
"""
import numpy as np
import pytest

from oracle import binding as ob
from restir_amd import capi
from restir_amd.ctypes_structs import make_camera
from tests import camera_cases as cc
from tests import extreme_cases as xc
from tests.common import oracle_scene
from tests.cut_plan_cases import SIZE as PLAN_SIZE, box, camera as _camera, directions as _directions, order_of as _order  # noqa: F401  (box: a fixture)
from tests.test_primary_cut_node_plan import _slabs, _walk

F32 = np.float32


@pytest.fixture(autouse=True)
def correctly_rounded_libm():
    with xc.correctly_rounded_libm():
        yield


# ---- the rows -----------------------------------------------------------------------------------------------------------------------
def test_the_table_holds_the_rows_it_was_asked_for():
    assert len(cc.NAMES) == len(cc.EXPECT) == 24 and set(cc.NAMES) == set(cc.EXPECT)
    assert set(cc.STILL) <= set(cc.NAMES) and set(cc.RESIZED) <= set(cc.NAMES) and set(cc.CPU_ONLY) <= set(cc.NAMES)
    assert set(cc.PAIR_NAMES) == set(cc.PAIR_EXPECT) and set(cc.GI_PAIRS) <= set(cc.PAIR_NAMES)
    box_ = cc._box()
    for name in cc.NAMES:                                # only the camera differs
        sd = cc.scene(name)
        assert sd.vertices is box_.vertices and sd.materials is box_.materials and sd.camera_args != box_.camera_args


@pytest.mark.parametrize("name", cc.NAMES)
def test_row_is_not_vacuous(name):
    o = cc.oracle_outputs(name)
    got, want = cc.figures(o), cc.expected(name)
    print(name, got)
    assert got == want, (name, got, want)
    assert got["nan"] == {} and got["inf"] == {}
    n = cc.SIZE[0] * cc.SIZE[1]
    hits, lights, misses = got["hits"]
    motion = o["direct3/gbuffer/motion"]
    if name in cc.WIDE:
        assert hits + lights >= 0.95 * n
    if name == "fov_0":
        assert (motion == -1).all()
    if name == "in_fov_90":
        assert got["motion"][0] < n // 4 and got["motion"][1] > 0 and got["motion"][2] > n // 2        # a still camera, and not the identity
    elif name not in ("fov_0",):
        own = motion == np.arange(n)                     # every other still camera reprojects a hit onto its own pixel
        assert own[o["direct3/gbuffer/prim_id"] != -1].all()
    if name.startswith("far_"):
        assert hits >= n // 2
    if name in ("looking_away", "focal_1e20"):
        assert hits == lights == 0 and got["live"] == got["live0"] == got["gi_live"] == 0 and got["pt4_rays"] == n
        assert not o["direct3/f2/image"].any() and not o["gi/f2/image"].any()
    for key, a in o.items():
        if not isinstance(a, int):
            for suffix, x in xc.fields(a):
                if x.dtype == np.float32:
                    assert np.isfinite(x).all(), key + suffix


def test_the_rows_differ():
    """Rows whose figures coincide are not copies of one run: 120 and -60 degrees have the same tangent up to rounding, 60 its negative."""
    a, b, c = (cc.oracle_outputs(n)["direct3/f2/image"] for n in ("in_fov_60", "in_fov_120", "in_fov_-60"))
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    assert cc.expected("fov_neg") != cc.expected("focal_1e-20")
    assert not np.array_equal(cc.oracle_outputs("fov_neg")["direct3/gbuffer/prim_id"], cc.oracle_outputs("focal_1e-20")["direct3/gbuffer/prim_id"])


@pytest.mark.parametrize("size", cc.SMALL_SIZES, ids=["%dx%d" % s for s in cc.SMALL_SIZES])
@pytest.mark.parametrize("name", cc.RESIZED)
def test_small_and_ragged_sizes(name, size):
    o = cc.oracle_outputs(name, size)
    hits, lights, misses = cc.hit_mix(o["direct3/gbuffer/prim_id"])
    n = size[0] * size[1]
    assert xc.nan_counts(o) == {} and xc.inf_counts(o) == {}
    if n <= 130:
        assert hits + lights == n and misses == 0        # 33, 130 and 4 hits
    else:
        assert hits + lights >= 0.95 * n
    assert xc.live(o["direct3/f2/res"]) > n // 2 and o["pt4/rays"] > n


# ---- the pairs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.PAIR_NAMES)
def test_pair_shows_its_mix(name):
    o = cc.oracle_pair(name)
    got = cc.pair_figures(o)
    print(name, got, [cc.motion_mix(o["f%d/motion" % f]) for f in range(cc.PAIR_FRAMES)])
    assert got == dict(dict(nan={}, inf={}), **cc.PAIR_EXPECT[name]), (name, got)
    own, gone, elsewhere = got["motion"]
    if name == "zoom_from_0":
        assert gone == 1536 and got["merged"] == 0       # no reprojection survives the division by zero, nothing is merged through one
        assert (o["f2/res"]["numSamples"] <= cc.CANDIDATES["direct"]).all()
    elif name == "turn_90":
        m = o["f2/motion"]
        there = (m != -1) & (m != np.arange(len(m)))
        assert there.sum() == elsewhere == 607 and got["merged"] == 0
        assert (o["f2/res"]["numSamples"][there] <= cc.CANDIDATES["direct"]).all()
        assert cc.merged_reprojected(o, f=3) >= 40       # ... and in the next frame they merge
    else:
        assert got["merged"] >= 40, (name, got)
    if name in ("pan_small", "fov_91_pan", "turn_10"):
        assert elsewhere >= 1000
    if name == "zoom_in_to_60":
        assert gone >= 1400 and elsewhere >= 40
    if name == "zoom_to_0":
        assert elsewhere >= 1500 and len(np.unique(o["f2/motion"])) <= 4      # every pixel sees one point


@pytest.mark.parametrize("name", cc.GI_PAIRS)
def test_gi_pair_merges_through_the_reprojection(name):
    o = cc.oracle_pair(name, "gi")
    merged = cc.merged_reprojected(o, "gi")
    print(name, merged)
    assert xc.nan_counts(o) == {} and xc.inf_counts(o) == {}
    assert merged == cc.GI_PAIR_MERGED[name]
    if name == "turn_90":
        assert merged == 0                               # as the direct pair: every reprojection lands on another material (the module's docstring)
    else:
        assert merged >= 40
    assert np.array_equal(o["f2/motion"], cc.oracle_pair(name)["f2/motion"])


# ---- the cut planner ----------------------------------------------------------------------------------------------------------------
PLAN_BASE = dict(position=(0.02, 0.47, 0.4), rotation=(-80.0, -5.0, 0.0))         # inside the scaled box
# view: blocks of 32 x 8 that take a cut, of the 21 of a 96 x 54 frame
PLAN_VIEWS = {
    "fov_60": (dict(fov_y=60.0), 3), "fov_83.6": (dict(fov_y=83.6), 3), "fov_83.7": (dict(fov_y=83.7), 0), "fov_89.99": (dict(fov_y=89.99), 0),
    "fov_90": (dict(fov_y=90.0), 0), "fov_91": (dict(fov_y=91.0), 0), "fov_120": (dict(fov_y=120.0), 2), "fov_-60": (dict(fov_y=-60.0), 2),
    "fov_179": (dict(fov_y=179.0), 21),
    "focal_1e-30": (dict(fov_y=30.0, focal_dist=1e-30), 6), "focal_1e18": (dict(fov_y=30.0, focal_dist=1e18), 6), "focal_-1": (dict(fov_y=30.0, focal_dist=-1.0), 6),
}


def _blocks(size):
    return [(x, y) for y in range(0, size[1], 8) for x in range(0, size[0], 32)]


@pytest.mark.parametrize("view", list(PLAN_VIEWS))
def test_cut_planner_at_the_camera_extremes(box, view):
    sd, boxes, nodes = box
    args, want = PLAN_VIEWS[view]
    cam = _camera(sd, **dict(PLAN_BASE, **args))
    tan = np.tan(F32(np.radians(F32(args["fov_y"]))))
    aspect = F32(PLAN_SIZE[0]) / F32(PLAN_SIZE[1])
    o = np.array([cam.position[i] for i in range(3)], np.float64)
    with_cut = entered = 0
    for x0, y0 in _blocks(PLAN_SIZE):
        order, count, pos, links = capi.plan_primary_cut(cam, x0, y0, 32, 8, boxes, nodes, 1 << 20)
        if order < 0 or count == 0:
            assert count == 0 and len(pos) == 0
            continue
        with_cut += 1
        assert 0 < count == len(pos) == len(links) <= nodes.shape[1]
        table = nodes[order]
        kept = set(int(p) for p in pos)
        for d in _directions(cam, x0, y0, 32, 8)[:: (1 if want <= 6 else 5)]:       # (all 21 blocks of the 179-degree view: every fifth ray)
            assert _order(d) == order
            passes = _slabs(o, d, boxes, table)
            whole = _walk(passes, table[:, 2], len(table))
            assert all(p in kept for p in np.array(whole)[passes[whole]]), (view, x0, y0)         # containment
            assert [int(pos[i]) for i in _walk(passes[pos], links, count)] == [p for p in whole if p in kept]
            entered += int(passes[whole].sum())
    print(view, "tan", tan, "aspect * tan", aspect * tan, "blocks with a cut:", with_cut)
    assert with_cut == want, (view, with_cut)
    if abs(tan) > 16 or abs(aspect * tan) > 16:          # the widening's bound (rs_cuts.h), on the magnitudes
        assert want == 0
    else:
        assert want > 0 and entered > 0


# view of the still-camera test of tests/test_gpu_camera_extremes.py: the row's camera in the box scaled by 0.45, its position scaled
# with it, 97 x 61 pixels -> blocks that take a cut, of 32
STILL_SIZE = (97, 61)
STILL_SCALE = 0.45
STILL_BLOCKS_WITH_A_CUT = {"in_fov_60": 7, "in_fov_83.6": 11, "in_fov_120": 7, "fov_1e-3": 0, "far_1e4": 0, "far_1e7": 0, "focal_1e18": 21, "focal_neg": 14,
                           "in_fov_90": 0, "in_fov_91": 0}


def still_camera_args(name):
    a = cc.camera_args(name)
    return dict(a, position=tuple(STILL_SCALE * p for p in a["position"]))


def planned_blocks_with_a_cut(name, boxes, nodes, size=STILL_SIZE):
    cam = capi.camera_update(make_camera(size[0], size[1], **still_camera_args(name)))
    plans = [capi.plan_primary_cut(cam, x0, y0, 32, 8, boxes, nodes, 1 << 20) for x0, y0 in _blocks(size)]
    return sum(1 for order, count, pos, links in plans if order >= 0 and count > 0)          # (an order and no record: no ray of the block meets the root box)


@pytest.mark.parametrize("name", list(STILL_BLOCKS_WITH_A_CUT))
def test_blocks_with_a_cut_of_the_still_camera_rows(box, name):
    sd, boxes, nodes = box
    assert planned_blocks_with_a_cut(name, boxes, nodes) == STILL_BLOCKS_WITH_A_CUT[name]
    assert set(cc.STILL) | {"in_fov_90", "in_fov_91"} == set(STILL_BLOCKS_WITH_A_CUT)
    assert sum(1 for n in cc.STILL if STILL_BLOCKS_WITH_A_CUT[n] > 0) >= 3


# ---- mutation check -----------------------------------------------------------------------------------------------------------------
def test_a_wrong_camera_function_would_show():
    sc = oracle_scene(cc._box())
    n = cc.SIZE[0] * cc.SIZE[1]
    moved_motion, moved_depth = [], []
    for name in cc.NAMES:
        o = cc.oracle_outputs(name)
        cam = ob.camera_update(cc.scene(name).camera(*cc.SIZE))
        origin = np.array([cam.position[i] for i in range(3)], F32)

        def traced(**kw):
            d = cc.center_dirs(cam, cc.SIZE, **kw)
            if not np.isfinite(d).all():
                return None, None, None
            prim, mat, pos, nrm, uv = sc.intersect(np.concatenate([np.tile(origin, (n, 1)), d], axis=1))
            diff = origin - pos
            return prim, pos, np.sqrt((diff * diff).sum(1, dtype=F32), dtype=F32)

        prim, pos, depth = traced()
        if prim is None:
            assert name == "focal_1e20"
            continue
        hit = o["direct3/gbuffer/prim_id"] != -1
        assert np.mean((prim >= 0) == hit) >= 0.99, name                     # the restatement IS the oracle's G-buffer ray, up to NumPy's order of summation
        hit &= prim >= 0
        if hit.any():                                                         # (to a few ulps: NumPy sums and normalises in its own order)
            assert np.mean(np.isclose(depth[hit], o["direct3/gbuffer/depth"][hit], rtol=1e-5, atol=0)) >= 0.99, name
        motion = cc.raster_coord(cam, pos, cc.SIZE)
        if name != "in_fov_90" and hit.any():                                 # (tan = -2.29e7: its entries hang on the last bits of the quotient)
            assert np.mean(motion[hit] == o["direct3/gbuffer/motion"][hit]) >= 0.99, name
        if hit.any() and not np.array_equal(cc.raster_coord(cam, pos, cc.SIZE, drop_half=True)[hit], motion[hit]):
            moved_motion.append(name)
        prim2, pos2, depth2 = traced(swap_focus=True)
        if not np.array_equal(prim2, prim) or not np.array_equal(depth2[hit].view(np.uint32), depth[hit].view(np.uint32)):
            moved_depth.append(name)
    print("motion plane changed by the raster mutant:", moved_motion)
    print("depth plane changed by the pFocus mutant:", moved_depth)
    assert len(moved_motion) >= 5 and len(moved_depth) >= 5
    assert set(cc.NAMES) - set(moved_motion) == {"fov_0", "looking_away", "focal_1e20"}
