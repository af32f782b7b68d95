"""Shadow rays regrouped by length (restir_amd/csrc/restir.hip k_shadow_regroup, rs_shadow_regroup.h; rs_restir_set_shadow_regroup): a
block of the shadow-ray kernel hands its 256 segments out to its four waves by length bin before the walk.  Any-hit occlusion does not
depend on the lane that carries a ray, so nothing may change by a bit.

Every frame comparison is three-way and bit for bit, after EVERY one of 4 frames of spatiotemporal reuse: regroup on against the CPU
oracle and regroup off against the oracle -- image, both reservoir buffers, the published copy, the ray count.  The shadow pass alone
(rs_debug_shadow_pass) runs both forms over hand-made candidate planes and is held to rs_trace_occlusion of the same segments; it also
returns the slot every ray took, which is held to the host's plan (rs_debug_plan_shadow_regroup).

A segment whose weight has exactly the bits of +0 does not walk in either form; -0 and NaN weights do."""
import os

import numpy as np
import pytest

from restir_amd import scenes
from restir_amd.ctypes_structs import LAMBERTIAN, LIGHT, make_materials
from tests import extreme_cases as xc
from tests.common import HipRenderer, get_scene, hip_scene, oracle_scene
from tests.primary_cuts import Side
from tests.scene_edits import assert_same

pytestmark = pytest.mark.gpu

F = np.float32
SHADED = 2                                            # kind of a pixel the RIS shades (tag bits 24, 25)


@pytest.fixture(scope="module", autouse=True)
def _libm():
    with xc.correctly_rounded_libm():
        yield


class _Side(Side):
    def __init__(self, hip, sd, size, rows=None, scene=None, regroup=True):
        super().__init__(hip, sd, size, rows, scene=scene)
        if hip:
            self.r.restir.set_shadow_regroup(regroup)


def _three_way(hip, sd, size, rows=None, frames=4, overlapped=False):
    scene_h, scene_o = hip_scene(hip, sd), oracle_scene(sd)
    scene_h.set_sample_sequence(None); scene_o.set_sample_sequence(None)
    on = _Side(hip, sd, size, rows, scene=scene_h, regroup=True)
    off = _Side(hip, sd, size, rows, scene=scene_h, regroup=False)
    ref = _Side(None, sd, size, rows, scene=scene_o)
    hip.set_sync(not overlapped)
    try:
        for f in range(frames):
            a, b, c = on.frame(), off.frame(), ref.frame()
            assert_same(c, a, "regroup on against the oracle, frame %d" % f)
            assert_same(c, b, "regroup off against the oracle, frame %d" % f)
    finally:
        hip.synchronize()
        hip.set_sync(True)
    return on, ref, c


def _shaded(side):
    tag = side.r.restir.surface()[2][:, 1]
    return ((tag >> 24) & 3) == SHADED


# ---- scenes made here ------------------------------------------------------------------------------------------------------------------
def _floor(s, half, mat=0):
    s.add_quad((-half, 0, half), (half, 0, half), (half, 0, -half), (-half, 0, -half), mat)


def one_lamp():
    """A floor, a box on it and ONE emissive triangle above: every segment ends on the same small lamp."""
    mats = make_materials([dict(type=LAMBERTIAN, baseColor=(0.7, 0.7, 0.7)), dict(type=LIGHT, baseColor=(12.0, 11.0, 9.0))])
    s = scenes.TriangleSoup()
    _floor(s, 2.0)
    scenes._box(s, (-0.4, 0.0, -0.4), (0.3, 0.7, 0.2), 0, yaw_deg=20.0)
    s.add_flat(np.array([[(-0.2, 1.9, -0.2), (0.2, 1.9, -0.2), (0.0, 1.9, 0.25)]], F), 1)       # normal -y
    return scenes.SceneData("one_lamp", s, mats, dict(position=(0.0, 1.2, 3.5), rotation=(-90.0, -12.0, 0.0), fov_y=19.5, focal_dist=1.0))


def lit_from_below():
    """A lamp that faces down hangs BELOW a slab; the camera looks down on the slab's top, which no candidate can light (every light
    sample lies behind the surface: no RIS winner, weight +0), and on the floor around it, which the lamp does light."""
    mats = make_materials([dict(type=LAMBERTIAN, baseColor=(0.7, 0.7, 0.7)), dict(type=LIGHT, baseColor=(10.0, 10.0, 10.0))])
    s = scenes.TriangleSoup()
    _floor(s, 4.0)
    s.add_quad((-1.7, 1.0, 1.7), (1.7, 1.0, 1.7), (1.7, 1.0, -1.7), (-1.7, 1.0, -1.7), 0)         # the slab, normal +y
    s.add_quad((-0.3, 0.6, -0.3), (0.3, 0.6, -0.3), (0.3, 0.6, 0.3), (-0.3, 0.6, 0.3), 1)         # the lamp, normal -y
    return scenes.SceneData("lit_from_below", s, mats, dict(position=(0.0, 3.0, 2.6), rotation=(-90.0, -45.0, 0.0), fov_y=30.0, focal_dist=1.0))


def _high_above(sd):
    """The scene's own view from far above it: nothing but sky (or nothing at all)."""
    p = sd.camera_args["position"]
    sd.camera_args = dict(sd.camera_args, position=(p[0], p[1] + 50.0, p[2]))
    return sd


SCENES = {
    "cornell-37x21": lambda: (get_scene("cornell"), (37, 21), None),                 # partial tiles, partial blocks, a width that is no multiple of 32
    "cornell-64x48": lambda: (get_scene("cornell"), (64, 48), None),
    "sponza-96x54": lambda: (get_scene("sponza:0.05"), (96, 54), None),
    "bistro-96x54": lambda: (get_scene("bistro:0.03"), (96, 54), None),               # the global-table RIS
    "cornell_textured-64x48": lambda: (get_scene("cornell_textured"), (64, 48), None),        # environment samples: lengths of 1e10, the top bin
    "cornell-rows-8-29": lambda: (get_scene("cornell"), (64, 48), (8, 29)),           # the strip form, y0 != 0
    "one_lamp-64x48": lambda: (one_lamp(), (64, 48), None),
    "lit_from_below-64x48": lambda: (lit_from_below(), (64, 48), None),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_frames_equal_regroup_off_and_the_oracle(hip, name):
    sd, size, rows = SCENES[name]()
    on, ref, last = _three_way(hip, sd, size, rows)
    assert last["image"].any() and last["rays"] > 0 and _shaded(on).any()


@pytest.mark.parametrize("name", ["cornell-64x48", "sponza-96x54", "cornell-rows-8-29"])
def test_overlapped_frames(hip, name):
    sd, size, rows = SCENES[name]()
    _three_way(hip, sd, size, rows, overlapped=True)


@pytest.mark.parametrize("name,sky", [("cornell", False), ("cornell_textured", True)])
def test_a_view_without_a_shaded_pixel(hip, name, sky):
    """Every wave of every block leaves before the walk."""
    on, ref, last = _three_way(hip, _high_above(get_scene(name)), (64, 48))
    assert not _shaded(on).any()
    assert bool(last["image"].any()) == sky


def test_whole_tiles_without_a_winner(hip):
    """lit_from_below: in the oracle's first frame without reuse the slab's top holds no weight, over whole 8x8 tiles, next to lit floor."""
    sd = lit_from_below()
    ref = _Side(None, sd, (64, 48), scene=oracle_scene(sd))
    ref.r.scene.set_sample_sequence(None)
    r = ref.r
    r.gbuf.render(r.scene, r.cam); r.restir.phase_a(r.scene, r.cam, r.gbuf, 0, 0, 0, 48)
    w = np.asarray(r.restir.reservoir["weight"]).reshape(48, 64)
    hit = np.asarray(r.gbuf.prim_id[r.gbuf.frame_idx]).reshape(48, 64) >= 0
    tiles = lambda a: a.reshape(6, 8, 8, 8).transpose(0, 2, 1, 3).reshape(6, 8, 64)
    dark = (tiles(w) == 0).all(2) & tiles(hit).all(2)                  # tiles of surface pixels only, none with a weight
    print("tiles of surface pixels without any weight:", int(dark.sum()), "of 48; lit pixels:", int((w > 0).sum()))
    assert dark.sum() >= 2 and (w > 0).sum() >= 256


# ---- the shadow pass alone: hand-made candidate planes --------------------------------------------------------------------------------------
def _planes(hip, sd, size, seed):
    """A real frame's positions and tags; candidates made here: each shaded pixel aims at a random point of the scene's bounding box
    (so lengths spread over the bins and a good part is occluded), with a random positive weight."""
    r = HipRenderer(hip, sd, *size)
    r.frame(3)
    pos_tag = r.restir.surface()[0]
    n = len(pos_tag)
    shaded = ((pos_tag[:, 3].view(np.int32) >> 24) & 3) == SHADED
    rng = np.random.default_rng(seed)
    v = sd.vertices.reshape(-1, 3)
    target = rng.uniform(v.min(0), v.max(0), (n, 3)).astype(F)
    d = target - pos_tag[:, :3]
    dist = np.sqrt((d * d).sum(1, dtype=F)).astype(F)
    dist = np.where(dist > 0, dist, F(1))
    wi = (d / dist[:, None]).astype(F)
    cand_li = np.concatenate([np.ones((n, 3), F), dist[:, None]], 1).astype(F)
    cand_wi = np.concatenate([wi, rng.uniform(0.5, 2.0, (n, 1)).astype(F)], 1).astype(F)
    return r, pos_tag, cand_li, cand_wi, shaded


def _expected(hip, r, pos_tag, cand_li, cand_wi, walks):
    """rs_trace_occlusion of the segments the kernels build: from pos to pos + wi * dist (float32, no contraction)."""
    import torch
    end = (pos_tag[:, :3] + (cand_wi[:, :3] * cand_li[:, 3:4]).astype(F)).astype(F)
    seg = np.concatenate([pos_tag[:, :3], end], 1).astype(F)[walks]
    occ = hip.trace_occlusion(r.scene, torch.from_numpy(np.ascontiguousarray(seg)).cuda()).cpu().numpy() != 0
    want = cand_wi.copy()
    idx = np.flatnonzero(walks)[occ]
    want[idx, 3] = 0
    return want, int(occ.sum())


def _both_forms(r, pos_tag, cand_li, cand_wi, rows=None):
    r.restir.set_shadow_regroup(True)
    on = r.restir.shadow_pass(r.scene, pos_tag, cand_li, cand_wi, rows)
    r.restir.set_shadow_regroup(False)
    off = r.restir.shadow_pass(r.scene, pos_tag, cand_li, cand_wi, rows)
    assert (off[1] == -1).all()                        # the plain form has no slots
    return on, off


@pytest.mark.parametrize("name,size", [("cornell", (64, 48)), ("sponza:0.05", (96, 54))])
def test_the_pass_alone_equals_the_plain_form_and_single_segments(hip, name, size):
    sd = get_scene(name)
    r, pos_tag, cand_li, cand_wi, shaded = _planes(hip, sd, size, 3)
    (w_on, slots, k), (w_off, _, _) = _both_forms(r, pos_tag, cand_li, cand_wi)
    want, occluded = _expected(hip, r, pos_tag, cand_li, cand_wi, shaded)
    print(name, "segments", int(shaded.sum()), "occluded", occluded)
    assert 0 < occluded < shaded.sum()
    assert np.array_equal(w_on.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(w_off.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(slots >= 0, shaded)


def test_zero_negative_zero_and_nan_weights(hip):
    """+0: no segment in either form (nothing written, no slot).  -0 and NaN: a segment like any other -- an occluded one comes back as
    +0, whose bits differ -- and the pixels come out as from the plain kernel."""
    sd = get_scene("cornell")
    r, pos_tag, cand_li, cand_wi, shaded = _planes(hip, sd, (64, 48), 5)
    rng = np.random.default_rng(6)
    what = rng.integers(0, 4, len(cand_wi))              # 0 keeps the weight
    cand_wi[what == 1, 3] = F(0.0)
    cand_wi[what == 2, 3] = F(-0.0)
    cand_wi[what == 3, 3] = F(np.nan)
    cand_wi[:64 * 8, 3].reshape(8, 64)[:, 8:16] = F(0.0)                 # one whole tile without a winner
    cand_wi[64 * 8:64 * 16, 3] = F(-0.0)                                 # two whole blocks of -0
    walks = shaded & (cand_wi[:, 3].view(np.uint32) != 0)
    (w_on, slots, k), (w_off, _, _) = _both_forms(r, pos_tag, cand_li, cand_wi)
    want, occluded = _expected(hip, r, pos_tag, cand_li, cand_wi, walks)
    neg = shaded & (cand_wi[:, 3].view(np.uint32) == 0x80000000)
    nan = shaded & np.isnan(cand_wi[:, 3])
    cleared = lambda m: int((want[m, 3].view(np.uint32) == 0).sum())
    print("walks", int(walks.sum()), "occluded", occluded, "-0 cleared", cleared(neg), "of", int(neg.sum()), "NaN cleared", cleared(nan), "of", int(nan.sum()))
    assert 0 < cleared(neg) < neg.sum() and 0 < cleared(nan) < nan.sum()
    assert np.array_equal(w_on.view(np.uint32), w_off.view(np.uint32))
    assert np.array_equal(w_on.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(slots >= 0, walks)


# ---- the slots against the host's plan ---------------------------------------------------------------------------------------------------
def _check_blocks(hip, size, rows, cand_li, walks, slots, k):
    W, H = size
    y0, y1 = rows or (0, H)
    lengths, walks, slots = cand_li[:, 3].reshape(H, W), walks.reshape(H, W), slots.reshape(H, W)
    assert (slots[:y0] == -1).all() and (slots[y1:] == -1).all()
    checked = 0
    for by in range(y0, y1, 8):
        for bx in range(0, W, 32):
            blk = (slice(by, min(by + 8, y1)), slice(bx, min(bx + 32, W)))
            ln, act, sl = lengths[blk].reshape(-1), walks[blk].reshape(-1), slots[blk].reshape(-1)
            bins, _, first, count = hip.plan_shadow_regroup(ln, bins_over_extent=k, active=act, plan=True)
            assert count == act.sum()
            assert sorted(sl[act].tolist()) == list(range(count))                  # a permutation of 0 .. count - 1
            assert (sl[~act] == -1).all()
            hist = np.bincount(bins[act], minlength=64)
            assert ((sl[act] >= first[bins[act]]) & (sl[act] < first[bins[act]] + hist[bins[act]])).all()      # inside its bin's range
            order = np.argsort(sl[act])
            assert (np.diff(bins[act][order]) <= 0).all()                           # longest first
            checked += 1
    return checked


@pytest.mark.parametrize("rows", [None, (8, 29)], ids=["full", "rows-8-29"])
def test_slots_lie_in_the_ranges_of_the_host_plan(hip, rows):
    sd = get_scene("cornell")
    size = (64, 48)
    r, pos_tag, cand_li, cand_wi, shaded = _planes(hip, sd, size, 9)
    cand_li[::7, 3] = F(1e10)                                                       # some environment-length segments: the top bin
    cand_wi[::5, 3] = F(0.0)
    walks = shaded & (cand_wi[:, 3].view(np.uint32) != 0)
    r.restir.set_shadow_regroup(True)
    w, slots, k = r.restir.shadow_pass(r.scene, pos_tag, cand_li, cand_wi, rows)
    v = sd.vertices.reshape(-1, 3)
    assert np.isfinite(k) and abs(k - 64.0 / float(np.linalg.norm(v.max(0) - v.min(0)))) < 1e-3 * k         # the diagonal of the scene's box
    if rows:
        inside = np.zeros((48, 64), bool); inside[rows[0]:rows[1]] = True
        walks = walks & inside.reshape(-1)
    blocks = _check_blocks(hip, size, rows, cand_li, walks, slots, k)
    assert blocks == 2 * ((rows[1] - rows[0] + 7) // 8 if rows else 6)
    bins = hip.plan_shadow_regroup(cand_li[walks, 3], bins_over_extent=k)[0]
    assert bins.max() == 63 and len(np.unique(bins)) > 8


def test_a_scene_without_the_shadow_tree_keeps_the_plain_kernel(hip):
    sd = get_scene("cornell")
    os.environ["RS_NO_OCCLUSION_TREE"] = "1"
    try:
        r, pos_tag, cand_li, cand_wi, shaded = _planes(hip, sd, (64, 48), 3)
    finally:
        del os.environ["RS_NO_OCCLUSION_TREE"]
    r.restir.set_shadow_regroup(True)
    w, slots, k = r.restir.shadow_pass(r.scene, pos_tag, cand_li, cand_wi)
    assert (slots == -1).all()
    want, occluded = _expected(hip, r, pos_tag, cand_li, cand_wi, shaded)
    assert occluded > 0 and np.array_equal(w.view(np.uint32), want.view(np.uint32))
