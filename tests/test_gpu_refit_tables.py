"""The device tables rs_scene_set_triangles rewrites, record by record and bit for bit, against the host restatement of
tests/refit_tables.py.  tests/test_gpu_geometry_edits.py sees those tables through rays and images only, which cannot tell a box that
is too large from a right one, nor a write where none belongs.  Here every array is read back (rs_debug_scene_table) and compared with
what a snapshot taken before the first edit and the edited vertices say it must hold: after an identity edit, after every kind of
edit, in the three scene configurations (both grid-box trees, the shadow tree alone, neither), after the first edit of a scene created
from inexact boxes, at the geometry where box code goes wrong, and with the staging ring full.  No comparison has a tolerance."""
import functools

import numpy as np
import pytest

from oracle import binding as ob
from tests.common import HipRenderer, OracleRenderer, bits_equal, get_scene, hip_scene, oracle_scene
from tests.geometry_edits import (EDIT_KINDS, EXTREME_KINDS, HipSide, OracleSide, apply_triangles, corner_triangle, edited_oracle_scene,
                                  extreme_edit, geometry_edit, movable, numpy_refit, probe_rays, probe_segments, root_box, soup_scene,
                                  zero_axis)
from tests.refit_tables import Snapshot, assert_tables, box_floats, first_difference
from tests.scene_edits import assert_same, differing
from tests.test_geometry_refit_host import SPONZA_SCALE

pytestmark = pytest.mark.gpu

SOUPS = (2, 3, 255, 256, 257)        # the root's children are leaves; the last thread of a block of 256 and the first of the next
RENDERED = ("cornell", "sponza")     # 36 triangles; 2 621, reference tree 22 deep.  (The soups have no light: their tables only.)
SCENES = RENDERED + tuple("soup%d" % n for n in SOUPS)
W, H = 61, 47
N_RAYS = 1500
BOX_TABLES = ("nodesAll", "occChain")


@pytest.fixture(autouse=True)
def exact_libm(hip):
    ob.set_libm_mode(1)            # cos / sin correctly rounded on both sides: every bit must agree
    hip.set_sync(True)
    yield
    ob.set_libm_mode(0)
    hip.set_sync(True)
    hip.set_side_stream(4)         # the library's default


@functools.lru_cache(maxsize=None)
def scene_data(name):
    if name.startswith("soup"):
        return soup_scene(int(name[4:]))
    return get_scene("sponza:%g" % SPONZA_SCALE if name == "sponza" else name)


@functools.lru_cache(maxsize=None)
def edits_up_to(name, kind):
    """The edits of EDIT_KINDS up to and including `kind`, each made on the vertices the ones before it left; the vertices and normals
    after them; the places the last one moved triangles from and to."""
    sd = scene_data(name)
    v, n = sd.vertices.reshape(-1, 3, 3).copy(), sd.normals.reshape(-1, 3, 3).copy()
    out, places = [], None
    for k in EDIT_KINDS[:EDIT_KINDS.index(kind) + 1]:
        ids, ev, en = geometry_edit(sd, v, k, seed=11)
        places = np.concatenate([v[ids].mean(1), np.asarray(ev).reshape(-1, 3, 3).mean(1)])
        v, n = apply_triangles(v, n, ids, ev, en)
        out.append((ids, ev, en))
    return out, v, n, places


def fresh(hip, name):
    """A new scene and the snapshot of its tables; both grid-box trees are there."""
    s = hip_scene(hip, scene_data(name))
    snap = Snapshot(s)
    assert snap.has_occ and snap.has_ord, "the scene has its shadow tree and its ordered trees: the refit of their boxes is under test"
    return s, snap


def assert_as_before(snap, s, tag):
    """Every table equals the snapshot bitwise, except the box floats of nodesAll / occChain, which equal it as values (a zero from
    rs_build_bvh may differ in sign from the refit's)."""
    for name, want in snap.tables.items():
        got = s.debug_table(name)
        if name in BOX_TABLES and len(want):
            assert np.array_equal(box_floats(got), box_floats(want)), (tag, name)
            got = got.copy()
            for f in ("min", "maxx", "maxy", "maxz"):
                got[f] = want[f]
        d = first_difference(name, want, got)
        assert d is None, (tag, d)


def assert_reference_boxes(hip, snap, s, v, tag):
    """nodesAll and occChain hold rs_refit_boxes(v) bitwise and numpy_refit(v) as values."""
    nn = snap.bvh_size
    exact, values = hip.refit_boxes(v, snap.nodes[0]), numpy_refit(v, snap.nodes[0])
    got = box_floats(s.debug_table("nodesAll"))
    for k in range(6):
        ids = snap.nodes[k][:, 1]
        assert bits_equal(got[k * nn:(k + 1) * nn], exact[ids]), (tag, "nodesAll", k)
        assert np.array_equal(got[k * nn:(k + 1) * nn], values[ids]), (tag, "nodesAll", k)
    if snap.has_occ:
        chain = box_floats(s.debug_table("occChain"))
        assert bits_equal(chain, exact) and np.array_equal(chain, values), (tag, "occChain")


# ---- what rays and one frame see ----------------------------------------------------------------------------------------------------------
def oracle_views(sd, scene, rays, seg, frames=1):
    out = {}
    prim, mat, pos, nrm, _ = scene.intersect(rays)
    hit = prim >= 0
    out["closest"] = dict(prim=prim, mat=mat[hit], pos=pos[hit], nrm=nrm[hit])
    out["occluded"] = dict(occ=scene.test_occlusion(seg))
    r = OracleRenderer(sd, W, H, scene=scene)
    for f in range(frames):
        r.frame(3)
        out["direct%d" % f] = dict(image=r.image.copy(), rays=r.rays, last=r.restir.last.copy(), temp=r.restir.temp.copy())
    return out, r


def hip_views(hip, sd, scene, rays, seg, frames=1):
    import torch
    out = {}
    prim, mat, pos, nrm = (t.cpu().numpy() for t in hip.trace_closest(scene, torch.from_numpy(rays).cuda()))
    hit = prim >= 0
    out["closest"] = dict(prim=prim, mat=mat[hit], pos=pos[hit], nrm=nrm[hit])
    out["occluded"] = dict(occ=hip.trace_occlusion(scene, torch.from_numpy(seg).cuda()).cpu().numpy())
    r = HipRenderer(hip, sd, W, H, scene=scene)
    for f in range(frames):
        r.frame(3)
        out["direct%d" % f] = dict(image=r.image.cpu().numpy(), rays=r.rays, last=r.restir.download(1), temp=r.restir.download(2))
    return out, r


def assert_views(hip, sd, s, oracle, places, tag, frames=1):
    rays, seg = probe_rays(sd, places, N_RAYS, 21), probe_segments(sd, places, N_RAYS, 22)
    want, o = oracle_views(sd, oracle, rays, seg, frames)
    got, h = hip_views(hip, sd, s, rays, seg, frames)
    for k in want:
        assert_same(want[k], got[k], (tag, k))
    return o, h


# ---- 0. the read-back itself --------------------------------------------------------------------------------------------------------------
def test_debug_table_sizes_and_refusals(hip):
    """Sizes first (host == NULL); a capacity that is too small, an unknown table and a captured stream are refused and write nothing."""
    import ctypes as C
    import torch
    sd = scene_data("cornell")
    s, snap = fresh(hip, "cornell")
    L = hip.lib()
    n, nn, g = sd.num_prims, 2 * sd.num_prims - 1, snap.grid
    lights = int((sd.materials["type"][sd.material_ids] == 4).sum())
    sizes = dict(vertices=36 * n, normals=36 * n, tris=48 * n, nodesAll=32 * (6 * nn + 1), occNodes=16 * (g["occ_count"] + 1), occChain=32 * nn,
                 occTris=48 * n, ordNodes=6 * g["ord_stride"], ordTris=3 * 48 * n, emiTris=48 * lights)
    size = C.c_size_t(0)
    for name, (which, _) in hip.SCENE_TABLES.items():
        hip.check(L.rs_debug_scene_table(s.handle, which, None, 0, C.byref(size)))
        assert size.value == snap.tables[name].nbytes and size.value == sizes.get(name, size.value), name
    assert lights == 2 and snap.tables["emiNodes"].nbytes >= 32
    buf = np.full(sizes["tris"], 0xab, np.uint8)
    ptr = buf.ctypes.data_as(C.c_void_p)

    def refused(code, *args):
        size.value = 77
        assert L.rs_debug_scene_table(*args, C.byref(size)) == code
        assert size.value == 77 and (buf == 0xab).all()
    refused(10001, s.handle, 2, ptr, buf.size - 1)           # RS_ERR_INVALID_ARGUMENT
    refused(10001, s.handle, 11, ptr, buf.size)
    refused(10001, s.handle, -1, ptr, buf.size)
    rt = C.CDLL("libamdhip64.so")
    rt.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    rt.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    rt.hipGraphDestroy.argtypes = [C.c_void_p]
    stream = torch.cuda.Stream()
    hip.synchronize()
    hip.set_stream(stream.cuda_stream)
    graph = C.c_void_p()
    try:
        assert rt.hipStreamBeginCapture(stream.cuda_stream, 2) == 0           # hipStreamCaptureModeRelaxed
        try:
            refused(10002, s.handle, 2, ptr, buf.size)       # RS_ERR_UNSUPPORTED
        finally:
            assert rt.hipStreamEndCapture(stream.cuda_stream, C.byref(graph)) == 0
            if graph:
                rt.hipGraphDestroy(graph)
    finally:
        hip.set_stream(None)
    hip.check(L.rs_debug_scene_table(s.handle, 2, ptr, buf.size, C.byref(size)))
    assert size.value == buf.size and buf.tobytes() == snap.tables["tris"].tobytes()


# ---- 1. the identity edit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_identity_edit(hip, name):
    """Every movable triangle set to its own vertices and normals: every table is what it was, and follows the restatement."""
    sd = scene_data(name)
    s, snap = fresh(hip, name)
    v, n = sd.vertices.reshape(-1, 3, 3), sd.normals.reshape(-1, 3, 3)
    ids = movable(sd)
    s.set_triangles(ids, v[ids], n[ids])
    assert_as_before(snap, s, name)
    assert_reference_boxes(hip, snap, s, v, name)
    assert_tables(snap.expected(v, n), s, name)


# ---- 2. every table after every kind of edit ----------------------------------------------------------------------------------------------
# Every scene takes every kind: the kinds name one, two or all movable triangles, and the smallest soup has two.
@pytest.mark.parametrize("kind", EDIT_KINDS)
@pytest.mark.parametrize("name", SCENES)
def test_tables_after_edit(hip, name, kind):
    """The device-side counterpart of the host tables of test_outputs_after_edit: after the edits of EDIT_KINDS up to `kind`, all
    eleven arrays hold what the snapshot and the edited vertices say; after `carry_back` they hold the snapshot again."""
    s, snap = fresh(hip, name)
    edits, v, n, _ = edits_up_to(name, kind)
    for ids, ev, en in edits:
        s.set_triangles(ids, ev, en)
    want = snap.expected(v, n)
    assert_tables(want, s, (name, kind))
    assert_reference_boxes(hip, snap, s, v, (name, kind))
    if kind == "carry_back":
        assert bits_equal(v, scene_data(name).vertices.reshape(-1, 3, 3))
        assert_as_before(snap, s, (name, kind))
    else:                                                    # not vacuous: the edit changed boxes of every tree
        for t in ("nodesAll", "occNodes", "ordNodes"):
            assert first_difference(t, snap.tables[t], want[t]) is not None, t


# ---- 3. the three configurations ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["shadow_tree_only", "no_trees"])
@pytest.mark.parametrize("name", RENDERED)
def test_other_configurations(hip, monkeypatch, name, config):
    """A scene without the ordered trees (k_ref_write covers 7 x bvhSize records, the grid kernels occNodes alone) and one with neither
    tree (6 x bvhSize, no grid kernels, and a vertex may leave the root box the scene was created with): the tables after every kind
    of edit, and what rays and a ReSTIR-DI frame see at the end.  (Both trees: every other test of this file.)"""
    sd = scene_data(name)
    monkeypatch.setenv("RS_NO_ORDERED_TREE" if config == "shadow_tree_only" else "RS_NO_OCCLUSION_TREE", "1")
    s = hip_scene(hip, sd)
    monkeypatch.undo()
    snap = Snapshot(s)
    g = s.debug_grid()
    assert g["ord_stride"] == 0 and len(snap.tables["ordNodes"]) == 0 and len(snap.tables["ordTris"]) == 0
    if config == "shadow_tree_only":
        assert g["occ_count"] > 0 and len(snap.trees) == 1
    else:
        assert g["occ_count"] == 0 and not snap.trees and g["margin"] == 0.0
        assert all(len(snap.tables[t]) == 0 for t in ("occNodes", "occChain", "occTris", "emiNodes", "emiTris"))
    oracle = oracle_scene(sd)
    v, n = sd.vertices.reshape(-1, 3, 3).copy(), sd.normals.reshape(-1, 3, 3).copy()
    edits = list(edits_up_to(name, EDIT_KINDS[-1])[0])
    if config == "no_trees":                                 # ten root-box extents away: allowed without the grid
        lo, hi = root_box(sd.vertices)
        p = corner_triangle(sd)
        far = (edits_up_to(name, EDIT_KINDS[-1])[1][p] + np.float32(10.0) * (hi - lo)).astype(np.float32)
        edits.append((np.array([p], np.int32), far[None], None))
    for j, (ids, ev, en) in enumerate(edits):
        s.set_triangles(ids, ev, en)
        oracle = edited_oracle_scene(hip, oracle, ids, ev, en)
        v, n = apply_triangles(v, n, ids, ev, en)
        assert_tables(snap.expected(v, n), s, (name, config, j))
        assert_reference_boxes(hip, snap, s, v, (name, config, j))
    if config == "no_trees":
        assert (v.reshape(-1, 3).max(0) > root_box(sd.vertices)[1] * 5).all()
    places = np.concatenate([v[edits[-1][0]].mean(1), v[edits[-2][0]].mean(1)])
    assert_views(hip, sd, s, oracle, places, (name, config))


# ---- 4. the first edit of a scene created from inexact boxes ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RENDERED)
def test_first_edit_of_caller_supplied_inexact_boxes(hip, name):
    """rs_scene_create with every box of rs_build_bvh grown outward by three ulps: still a proper hierarchy, so both trees are built.
    The device holds the supplied boxes until the first edit; that edit replaces all of them by the exact unions, on the device as on
    the host, and the emissive tree (built over the grown boxes) is no longer asked: rs_path_trace at depth 3 and two direct frames
    equal the oracle's with rs_refit_boxes' boxes."""
    import torch
    sd = scene_data(name)
    tables = hip_scene(hip, sd).host_desc()
    grown = tables["boxes"].copy()
    for _ in range(3):
        grown[:, :3] = np.nextafter(grown[:, :3], np.float32(-np.inf))
        grown[:, 3:] = np.nextafter(grown[:, 3:], np.float32(np.inf))
    tables["boxes"] = grown
    s = hip.Scene.from_tables(sd.vertices, sd.normals, sd.texcoords, sd.material_ids, sd.materials, tables)
    snap = Snapshot(s)
    assert snap.has_occ and snap.has_ord, "grown boxes still nest: the trees are built"
    nn = snap.bvh_size
    for k in range(6):
        assert bits_equal(box_floats(snap.tables["nodesAll"][k * nn:(k + 1) * nn]), grown[snap.nodes[k][:, 1]])
    assert bits_equal(box_floats(snap.tables["occChain"]), grown)
    assert len(snap.tables["emiNodes"]) > 1
    ids, ev, en = geometry_edit(sd, sd.vertices, "one", seed=11)
    s.set_triangles(ids, ev, en)
    v, n = apply_triangles(sd.vertices, sd.normals, ids, ev, en)
    want = snap.expected(v, n)
    assert_tables(want, s, name)
    assert_reference_boxes(hip, snap, s, v, name)
    assert bits_equal(s.host_desc()["boxes"], hip.refit_boxes(v, snap.nodes[0]))
    untouched = np.setdiff1d(np.arange(nn), [snap.leaf_of[ids[0]]])
    assert not bits_equal(box_floats(want["occChain"])[untouched], grown[untouched])         # (boxes the edit did not move changed too)
    oracle = edited_oracle_scene(hip, oracle_scene(sd), ids, ev, en)
    places = np.concatenate([sd.vertices.reshape(-1, 3, 3)[ids].mean(1), v[ids].mean(1)])
    o, h = assert_views(hip, sd, s, oracle, places, name, frames=2)
    px = W * H
    d, i = np.zeros((px, 3), np.float32), np.zeros((px, 3), np.float32)
    rays = ob.path_trace(oracle, o.cam, d, i, 0, 0, 3)
    dd = torch.zeros((px, 3), dtype=torch.float32, device="cuda"); di = torch.zeros_like(dd)
    assert hip.path_trace(s, h.cam, dd.data_ptr(), di.data_ptr(), 0, 0, 3) == rays
    assert bits_equal(dd.cpu().numpy(), d) and bits_equal(di.cpu().numpy(), i)
    assert differing(i, np.zeros_like(i)) > 0


# ---- 5. geometric extremes ------------------------------------------------------------------------------------------------------------------
# "signed_zeros" needs an axis with 0 inside the grid's box: both scenes have one (x).
def test_a_scene_has_an_axis_through_zero():
    assert all(zero_axis(*root_box(scene_data(name).vertices)) is not None for name in RENDERED)


@pytest.mark.parametrize("kind", EXTREME_KINDS)
@pytest.mark.parametrize("name", RENDERED)
def test_geometric_extremes(hip, name, kind):
    """Triangles flat on the six faces of the grid's box, points on its eight corners, a point and a line inside, -0 and +0 mixed, an
    edge of one ulp and a subnormal one, every id three times in one call: every table, closest hits, occlusion and one direct frame."""
    sd = scene_data(name)
    s, snap = fresh(hip, name)
    g = s.debug_grid()
    lo, hi = root_box(sd.vertices)
    assert np.array_equal(g["lo"], lo) and np.array_equal(g["hi"], hi)
    ids, ev, en = extreme_edit(sd, sd.vertices, kind, g["lo"], g["hi"], seed=5)
    if kind == "signed_zeros":
        k = zero_axis(g["lo"], g["hi"])
        assert np.signbit(ev[..., k]).any() and (ev[..., k] == 0).all() and not np.signbit(ev[..., k]).all()
    if kind == "tiny_edges":
        e1 = ev[:, 1] - ev[:, 0]
        assert len(ev) == 2 and (e1[1] != 0).any() and (np.abs(e1[1][e1[1] != 0]) < np.finfo(np.float32).tiny).all()
    if kind == "thrice":
        assert len(ids) == 3 * len(movable(sd))
    s.set_triangles(ids, ev, en)
    v, n = apply_triangles(sd.vertices, sd.normals, ids, ev, en)
    want = snap.expected(v, n)
    assert_tables(want, s, (name, kind))
    assert_reference_boxes(hip, snap, s, v, (name, kind))
    assert first_difference("occNodes", snap.tables["occNodes"], want["occNodes"]) is not None
    oracle = edited_oracle_scene(hip, oracle_scene(sd), ids, ev, en)
    places = np.concatenate([sd.vertices.reshape(-1, 3, 3)[ids].mean(1), v[ids].mean(1)])
    if len(places) > 64:
        places = places[np.random.default_rng(5).permutation(len(places))[:64]]
    assert_views(hip, sd, s, oracle, places, (name, kind))


# ---- 6. a full staging ring -------------------------------------------------------------------------------------------------------------------
RING_SIZES = (1, 3, 40, None, 1, None, 2, None, 1)           # None: every movable triangle
FRAME_AFTER = (2, 5, 9)


@functools.lru_cache(maxsize=None)
def ring_edits():
    sd = scene_data("sponza")
    rng = np.random.default_rng(17)
    ids_all = movable(sd)
    lo, hi = root_box(sd.vertices)
    v, n = sd.vertices.reshape(-1, 3, 3).copy(), sd.normals.reshape(-1, 3, 3).copy()
    edits = []
    for size in RING_SIZES:
        ids = ids_all if size is None else np.sort(rng.choice(ids_all, size, replace=False)).astype(np.int32)
        ev = np.clip(v[ids] + rng.uniform(-0.04, 0.04, (len(ids), 3, 3)) * (hi - lo), lo, hi).astype(np.float32)
        v, n = apply_triangles(v, n, ids, ev)
        edits.append((ids, ev, None))
    return edits, v, n


@functools.lru_cache(maxsize=None)
def ring_oracle():
    from restir_amd import capi
    ob.set_libm_mode(1)
    o = OracleSide(capi, scene_data("sponza"), W, H)
    images = []
    for j, e in enumerate(ring_edits()[0]):
        o.set_triangles(*e)
        if j + 1 in FRAME_AFTER:
            o.r.frame(3)
            images.append(o.image())
    return images


@pytest.mark.parametrize("side_stream", [4, 0], ids=["overlapped", "no_side_streams"])
def test_full_staging_ring(hip, side_stream):
    """rs_set_sync(0): nine edits of 1, 3, 40, all, 1, all, 2, all, 1 triangles with a frame after the 2nd, 5th and 9th and no wait
    anywhere -- more edits than the ring has pinned buffers (4), and small edits followed by ones that outgrow the device staging
    buffer while the earlier ones are still queued.  Each frame equals the oracle's; the final tables follow the restatement."""
    import torch
    sd = scene_data("sponza")
    edits, v, n = ring_edits()
    up = lambda b: (b + 15) & ~15
    staged = [up(len(ids) * 4) + up(len(ids) * 36) for ids, _, _ in edits]
    assert staged[2] <= 4096 < min(staged[3], staged[5], staged[7]), "the edits of every triangle regrow the 4 096-byte staging buffers"
    ref = ring_oracle()
    assert differing(ref[0], ref[1]) > 0 and differing(ref[1], ref[2]) > 0
    hip.set_side_stream(side_stream)
    h = HipSide(hip, sd, W, H)
    snap = Snapshot(h.r.scene)
    assert snap.has_occ and snap.has_ord
    outs = [torch.zeros((W * H, 3), dtype=torch.float32, device="cuda") for _ in FRAME_AFTER]
    hip.set_sync(False)
    try:
        r = h.r
        for j, e in enumerate(edits):
            h.set_triangles(*e)
            if j + 1 in FRAME_AFTER:
                r.gbuf.render(r.scene, r.cam)
                r.restir.direct(r.scene, r.cam, r.gbuf, r.image.data_ptr(), 0, r.looper, 3)
                r.looper += 1
                r.gbuf.update(r.cam)
                hip.hip_memcpy_d2d_async(outs[FRAME_AFTER.index(j + 1)].data_ptr(), r.image.data_ptr(), W * H * 12)
        hip.synchronize()
    finally:
        hip.set_sync(True)
        hip.set_side_stream(4)
    for f, want in enumerate(ref):
        got = outs[f].cpu().numpy()
        assert bits_equal(want, got), (f, differing(want, got))
    assert_tables(snap.expected(v, n), h.r.scene, "after nine edits")
    assert_reference_boxes(hip, snap, h.r.scene, v, "after nine edits")
