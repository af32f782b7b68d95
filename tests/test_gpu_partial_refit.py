"""The partial refit (rs_scene_set_partial_refit): an edit that names few triangles recomputes only the boxes above their leaves and
must leave every device table bit for bit what the whole-scene refit leaves.  The arbiter is the host restatement of
tests/refit_tables.py: after every edit all tables of capi.SCENE_TABLES equal Snapshot.expected of the edited vertices, the scene's
counters say the edit took the partial path, and the number of nodes the device recomputed equals the size of the dirty set counted
from the snapshot's own parent arrays (the distinct ancestors of the edited leaves in every tree, leaves included).  Every case makes an
identity edit first -- the first edit of a scene is whole -- and then switches the mode on.  No comparison has a tolerance."""
import functools

import numpy as np
import pytest

from tests.common import HipRenderer, bits_equal, hip_scene, oracle_scene
from tests.emitter_edits import edits_up_to as emitter_edits_up_to, emissive_root_box, emitters, scene_data as emitter_scene_data
from tests.emitter_tables import EmissiveSnapshot, grid_over_box
from tests.geometry_edits import EDIT_KINDS, apply_triangles, edited_oracle_scene, extreme_edit, geometry_edit, movable, root_box, tree_children, zero_axis
from tests.part_transforms import parts_of, translation
from tests.refit_tables import Snapshot, assert_tables, first_difference
from tests.test_gpu_refit_tables import RENDERED, SCENES, H, W, assert_reference_boxes, assert_views, exact_libm, scene_data  # noqa: F401 (exact_libm: autouse here too)

pytestmark = pytest.mark.gpu

ADMITS = 16                          # the threshold of most cases: admits every small edit here, refuses the edits of every triangle


# ---- the dirty set, from the snapshot alone -----------------------------------------------------------------------------------------------
def tree_tables(snap):
    """[(parent, leaf of a primitive)] of the reference tree and of every grid-box tree of the snapshot, each in its own numbering."""
    if not hasattr(snap, "_partial_trees"):
        inner, _ = tree_children(snap.nodes[0])
        parent = np.full(snap.bvh_size, -1, np.int64)
        for node, a, b in inner:
            parent[a] = parent[b] = node
        out = [(parent, {p: int(snap.leaf_of[p]) for p in range(snap.num_prims)})]
        for _, tree in snap.trees:
            leaf = {int(p): int(i) for j, i in enumerate(tree.leaves) for p in tree.leaf_prims[j] if p >= 0}
            assert len(leaf) == snap.num_prims
            out.append((tree.parent, leaf))
        snap._partial_trees = out
    return snap._partial_trees


def dirty_nodes(snap, ids):
    total = 0
    for parent, leaf in tree_tables(snap):
        seen = set()
        for p in np.unique(ids):
            n = leaf[int(p)]
            while n >= 0 and n not in seen:              # (every ancestor of a node already seen has been seen)
                seen.add(n)
                n = int(parent[n])
        total += len(seen)
    return total


def tree_depths(snap):
    """The deepest leaf of every tree, the root at 0."""
    out = []
    for parent, leaf in tree_tables(snap):
        deepest = 0
        for n in set(leaf.values()):
            d = 0
            while parent[n] >= 0:
                n, d = int(parent[n]), d + 1
            deepest = max(deepest, d)
        out.append(deepest)
    return out


# ---- a scene whose first edit has been made, the mode on ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def snapshot_of(name, config="both"):
    """The snapshot of a scene as created (a scene's tables are a function of its description: every test makes its own scene)."""
    from restir_amd import capi
    return Snapshot(make_scene(capi, name, config))


def make_scene(hip, name, config="both"):
    import os
    var = {"both": None, "shadow_tree_only": "RS_NO_ORDERED_TREE", "no_trees": "RS_NO_OCCLUSION_TREE"}[config]
    if var:
        os.environ[var] = "1"
    try:
        return hip_scene(hip, scene_data(name))
    finally:
        if var:
            del os.environ[var]


class Edited:
    """A scene after its identity edit, with the vertices and normals it holds; edit() makes one edit and checks everything."""

    def __init__(self, hip, name, admits=ADMITS, config="both", scene=None):
        self.hip, self.name, self.sd = hip, name, scene_data(name)
        self.snap = snapshot_of(name, config)
        self.s = scene or make_scene(hip, name, config)
        self.v, self.n = self.sd.vertices.reshape(-1, 3, 3).copy(), self.sd.normals.reshape(-1, 3, 3).copy()
        ids = movable(self.sd)
        assert self.s.refit_counts() == (0, 0)
        self.s.set_triangles(ids, self.v[ids], self.n[ids])
        assert self.s.refit_counts() == (1, 0) and self.s.refit_dirty() == 0
        self.s.set_partial_refit(True, admits)
        assert self.s.partial_refit() == (True, admits)

    def expected(self):
        return self.snap.expected(self.v, self.n)

    def edit(self, ids, ev, en=None, partial=True, tag=None, call=None):
        whole, part = self.s.refit_counts()
        (call or self.s.set_triangles)(ids, ev, en)
        self.v, self.n = apply_triangles(self.v, self.n, ids, ev, en)
        assert_tables(self.expected(), self.s, (self.name, tag))
        assert_reference_boxes(self.hip, self.snap, self.s, self.v, (self.name, tag))
        assert self.s.refit_counts() == ((whole, part + 1) if partial else (whole + 1, part)), (self.name, tag)
        assert self.s.refit_dirty() == (dirty_nodes(self.snap, ids) if partial else 0), (self.name, tag)

    def moved(self, ids, scale=0.07, seed=3):
        """The triangles `ids` jittered inside the root box."""
        rng = np.random.default_rng(seed)
        lo, hi = root_box(self.sd.vertices)
        return np.clip(self.v[ids] + rng.uniform(-scale, scale, (len(ids), 3, 3)) * (hi - lo), lo, hi).astype(np.float32)


def some_triangle(sd):
    ids = movable(sd)
    return int(ids[len(ids) // 2])


# ---- 0. the switch ------------------------------------------------------------------------------------------------------------------------
def test_switch_refusals_and_default(hip):
    s = make_scene(hip, "cornell")
    L = hip.lib()
    assert s.partial_refit() == (False, 4096) and s.refit_counts() == (0, 0) and s.refit_dirty() == 0
    for on, limit in ((2, 4), (-1, 4), (1, 0), (0, 0)):
        assert L.rs_scene_set_partial_refit(s.handle, on, limit) == hip.RS_ERR_INVALID_ARGUMENT
        assert s.partial_refit() == (False, 4096)
    s.set_partial_refit(True, 7)
    assert s.partial_refit() == (True, 7)
    s.set_partial_refit(True, -5)
    assert s.partial_refit() == (True, 4096)
    s.set_partial_refit(False, 9)
    assert s.partial_refit() == (False, 9)
    assert L.rs_debug_scene_refit_dirty(s.handle, None) == hip.RS_ERR_INVALID_ARGUMENT


def test_first_edit_is_whole_with_the_mode_on(hip):
    """Switched on before any edit: the first edit still refits the whole scene (no key boxes yet), the second is partial."""
    sd = scene_data("cornell")
    s = make_scene(hip, "cornell")
    s.set_partial_refit(True, ADMITS)
    snap = snapshot_of("cornell")
    ids, ev, en = geometry_edit(sd, sd.vertices, "one", seed=11)
    s.set_triangles(ids, ev, en)
    v, n = apply_triangles(sd.vertices, sd.normals, ids, ev, en)
    assert s.refit_counts() == (1, 0) and s.refit_dirty() == 0
    assert_tables(snap.expected(v, n), s, "first")
    ids, ev, en = geometry_edit(sd, v, "carry", seed=11)
    s.set_triangles(ids, ev, en)
    v, n = apply_triangles(v, n, ids, ev, en)
    assert s.refit_counts() == (1, 1) and s.refit_dirty() == dirty_nodes(snap, ids)
    assert_tables(snap.expected(v, n), s, "second")


def test_plan_inputs_are_the_snapshot_s(hip):
    """The bound of the library's decision, from the depths the snapshot has: an edit of m triangles is partial exactly while m is at
    most the threshold (the capacity test cannot fail at these sizes), and the dirty nodes never exceed m x sum (depth + 1)."""
    e = Edited(hip, "sponza", admits=3)
    depths = tree_depths(e.snap)
    assert len(depths) == 8
    ids = movable(e.sd)[10:14]
    for m, partial in ((3, True), (4, False)):
        assert hip.plan_refit(1, 3, 1, m, depths) == (partial, m * sum(d + 1 for d in depths))
        e.edit(ids[:m], e.moved(ids[:m]), partial=partial, tag=m)
        assert dirty_nodes(e.snap, ids[:m]) <= m * sum(d + 1 for d in depths)


# ---- 1. which triangles -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_one_triangle(hip, name):
    e = Edited(hip, name)
    p = np.array([some_triangle(e.sd)], np.int32)
    e.edit(p, e.moved(p), tag="one")
    want = e.expected()
    for t in ("nodesAll", "occNodes", "ordNodes"):           # not vacuous
        assert first_difference(t, e.snap.tables[t], want[t]) is not None, t


@pytest.mark.parametrize("name", SCENES)
def test_sibling_leaves(hip, name):
    """Two triangles whose reference leaves are the two children of one node: that node expects two arrivals, its ancestors one."""
    e = Edited(hip, name)
    inner, leaves = tree_children(e.snap.nodes[0])
    prim_of = {leaf: p for p, leaf in leaves.items()}
    ok = set(movable(e.sd).tolist())
    pairs = [(prim_of[a], prim_of[b]) for _, a, b in inner if a in prim_of and b in prim_of and prim_of[a] in ok and prim_of[b] in ok]
    assert pairs
    ids = np.array(pairs[len(pairs) // 2], np.int32)
    e.edit(ids, e.moved(ids), tag="siblings")


@pytest.mark.parametrize("tree", [0, 1, 6], ids=["occNodes", "ordNodes0", "ordNodes5"])
@pytest.mark.parametrize("name", ["cornell", "sponza", "soup257"])
def test_triangles_of_one_grid_leaf(hip, name, tree):
    """Two triangles that share a leaf of a grid-box tree (one lane owns it), then every triangle of that leaf."""
    e = Edited(hip, name)
    ok = set(movable(e.sd).tolist())
    rows = [[int(p) for p in row if p >= 0] for row in e.snap.trees[tree][1].leaf_prims]
    rows = [r for r in rows if len(r) >= 2 and all(p in ok for p in r)]
    assert rows, "the tree has a leaf of several movable triangles"
    row = max(rows, key=len)
    two = np.array(row[:2], np.int32)
    e.edit(two, e.moved(two), tag="two of a leaf")
    every = np.array(row, np.int32)
    e.edit(every, e.moved(every, seed=4), tag="a whole leaf")


@pytest.mark.parametrize("name", SCENES)
def test_boxes_shrink(hip, name):
    """A triangle carried to the far corner and back to where it was: its ancestors' boxes must shrink to the exact union again, which a
    climb that only ever grows a box cannot do.  The tables end as the snapshot's boxes of the original vertices."""
    e = Edited(hip, name)
    for kind in ("carry", "carry_back"):
        ids, ev, en = geometry_edit(e.sd, e.v, kind, seed=11)
        e.edit(ids, ev, en, tag=kind)
    assert bits_equal(e.v, e.sd.vertices.reshape(-1, 3, 3))
    # inside its old box: a triangle shrunk about its centroid
    p = np.array([some_triangle(e.sd)], np.int32)
    c = e.v[p].mean(1, keepdims=True)
    e.edit(p, (c + (e.v[p] - c) * np.float32(0.25)).astype(np.float32), tag="shrunk in place")


@pytest.mark.parametrize("name", RENDERED)
def test_signed_zeros(hip, name):
    """-0 and +0 mixed on an axis: the key order puts -0 below +0, in a partial climb as in a whole one."""
    e = Edited(hip, name)
    g = e.s.debug_grid()
    ids, ev, en = extreme_edit(e.sd, e.v, "signed_zeros", g["lo"], g["hi"], seed=5)
    k = zero_axis(g["lo"], g["hi"])
    assert np.signbit(ev[..., k]).any() and (ev[..., k] == 0).all() and not np.signbit(ev[..., k]).all()
    e.edit(ids, ev, en, tag="signed zeros")
    # ... and the other way round on the same triangles: every zero changes its sign, no value changes
    flipped = ev.copy()
    flipped[..., k] = -flipped[..., k]
    e.edit(ids, flipped, en, tag="signed zeros flipped")


@pytest.mark.parametrize("name", SCENES)
def test_same_triangle_again(hip, name):
    """Consecutive partial edits of one triangle: the counters and owner words of the first are back at 0 for the second and third."""
    e = Edited(hip, name)
    p = np.array([some_triangle(e.sd)], np.int32)
    for j in range(3):
        e.edit(p, e.moved(p, seed=20 + j), tag=("again", j))


@pytest.mark.parametrize("name", ["cornell", "sponza", "soup256"])
def test_partial_whole_partial(hip, name):
    e = Edited(hip, name, admits=2)
    ids = movable(e.sd)
    a, many = ids[:2], ids[:3]
    e.edit(a, e.moved(a, seed=1), tag="partial")
    e.edit(many, e.moved(many, seed=2), partial=False, tag="whole")
    e.edit(a, e.moved(a, seed=3), tag="partial again")
    e.s.set_partial_refit(False, 2)
    e.edit(a, e.moved(a, seed=4), partial=False, tag="switched off")
    e.s.set_partial_refit(True, 3)
    e.edit(many, e.moved(many, seed=5), tag="switched on, a higher threshold")


@pytest.mark.parametrize("name", ["soup2", "soup3"])
def test_every_triangle_of_the_smallest_trees(hip, name):
    """Both children of the root are dirty, and the root's children are leaves."""
    e = Edited(hip, name)
    ids = movable(e.sd)
    assert len(ids) == int(name[4:])
    e.edit(ids, e.moved(ids), tag="every triangle")
    assert e.s.refit_dirty() == sum(len(parent) for parent, _ in tree_tables(e.snap))


@pytest.mark.parametrize("name", RENDERED)
def test_edit_kinds(hip, name):
    """The edits of EDIT_KINDS in their order: those of at most ADMITS triangles are partial, "all" is whole."""
    e = Edited(hip, name)
    seen = set()
    for kind in EDIT_KINDS:
        ids, ev, en = geometry_edit(e.sd, e.v, kind, seed=11)
        partial = len(np.unique(ids)) <= ADMITS
        e.edit(ids, ev, en, partial=partial, tag=kind)
        seen.add(partial)
    assert seen == {True, False}


# ---- 2. the other two entry points ------------------------------------------------------------------------------------------------------------
def test_geometry_edit_that_names_an_emitter(hip):
    """rs_scene_set_geometry of the Cornell box's lamp, partial: the other tables follow the partial climb, the emissive tree is
    re-quantised as a whole on its new grid, as tests/test_gpu_emitter_tables.py expects it."""
    sd = emitter_scene_data("cornell")
    s = hip_scene(hip, sd)
    snap = EmissiveSnapshot(s, emitters(sd))
    v, n = sd.vertices.reshape(-1, 3, 3).copy(), sd.normals.reshape(-1, 3, 3).copy()
    ids = movable(sd)
    s.set_triangles(ids, v[ids], n[ids])
    s.set_partial_refit(True, ADMITS)
    edits = emitter_edits_up_to("cornell", "mixed")[0]
    for j, (ids, ev, en) in enumerate(edits[:1] + edits[2:]):          # "one" (the lamp) and "mixed" (the lamp and another triangle); "all" is every lamp
        s.set_geometry(ids, ev, en)
        v, n = apply_triangles(v, n, ids, ev, en)
        grid = s.emissive_grid()
        g = grid_over_box(*emissive_root_box(sd, v))
        assert grid["state"] == 1 and bits_equal(grid["base"], g["base"]) and bits_equal(grid["scale"], g["scale"]) and grid["margin"] == g["margin"]
        assert_tables(snap.expected_all(v, n, grid), s, ("lamp", j))
        assert s.refit_counts() == (1, 1 + j) and s.refit_dirty() == dirty_nodes(snap, ids)
    assert not bits_equal(s.emissive_grid()["base"], snap.emi_grid["base"])
    # a partial edit that names no emitter writes no emissive byte
    nodes, tris = s.debug_table("emiNodes"), s.debug_table("emiTris")
    ids, ev, en = geometry_edit(sd, v, "one", seed=6)
    s.set_geometry(ids, ev, en)
    assert s.refit_counts() == (1, 3)
    assert first_difference("emiNodes", nodes, s.debug_table("emiNodes")) is None and first_difference("emiTris", tris, s.debug_table("emiTris")) is None


def test_part_transform(hip):
    """rs_scene_set_part_transforms of one part of 63 triangles on the Sponza-class scene: baked on the device, refitted partially."""
    e = Edited(hip, "sponza", admits=64)
    part = np.array(parts_of("many")[0][1], np.int32)
    assert len(part) == 63
    rest_v, rest_n = e.v[part].copy(), e.n[part].copy()
    e.s.define_parts([part.tolist()])
    lo, hi = root_box(e.sd.vertices)
    for j, shift in enumerate(((0.01, -0.02, 0.015), (0.0, 0.0, 0.0))):           # away, and back onto the rest pose
        m = translation(np.asarray(shift) * (hi - lo))
        bv, bn = hip.bake_matrix(m, rest_v, rest_n)
        e.edit(part, bv.reshape(-1, 3, 3), bn.reshape(-1, 3, 3), tag=("part", j), call=lambda ids, v, n: e.s.set_part_transforms([0], m[None]))


# ---- 3. the other configurations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["shadow_tree_only", "no_trees"])
@pytest.mark.parametrize("name", RENDERED)
def test_other_configurations(hip, name, config):
    """Two trees (the reference tree and occNodes) and one (the reference tree alone: no grid-box launch at all)."""
    e = Edited(hip, name, config=config)
    assert len(e.snap.trees) == (1 if config == "shadow_tree_only" else 0)
    for kind in ("carry", "carry_back", "one", "repeated"):
        ids, ev, en = geometry_edit(e.sd, e.v, kind, seed=11)
        e.edit(ids, ev, en, tag=(config, kind))


# ---- 4. what rays and a frame see -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RENDERED)
def test_rendered_after_a_partial_edit(hip, name):
    """Closest hits, occlusion and one ReSTIR frame after partial edits equal the oracle's on the edited description."""
    e = Edited(hip, name)
    oracle = oracle_scene(e.sd)
    places = []
    for kind in ("carry", "one"):
        ids, ev, en = geometry_edit(e.sd, e.v, kind, seed=11)
        places += [e.v[ids].mean(1), np.asarray(ev).reshape(-1, 3, 3).mean(1)]
        e.edit(ids, ev, en, tag=kind)
        oracle = edited_oracle_scene(hip, oracle, ids, ev, en)
    assert e.s.refit_counts() == (1, 2)
    assert_views(hip, e.sd, e.s, oracle, np.concatenate(places), name)


def frames_with_edits(hip, sync):
    """Frame, partial edit, frame, partial edit, frame on the Sponza-class scene; the last image and the scene."""
    import torch
    sd = scene_data("sponza")
    r = HipRenderer(hip, sd, W, H)
    e = Edited(hip, "sponza", scene=r.scene)
    out = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
    hip.set_sync(sync)
    try:
        for j in range(3):
            if j:
                ids, ev, en = geometry_edit(sd, e.v, ("carry", "one")[j - 1], seed=11)
                r.scene.set_triangles(ids, ev, en)
                e.v, e.n = apply_triangles(e.v, e.n, ids, ev, en)
            r.gbuf.render(r.scene, r.cam)
            r.restir.direct(r.scene, r.cam, r.gbuf, r.image.data_ptr(), 0, r.looper, 3)
            r.looper += 1
            r.gbuf.update(r.cam)
        hip.hip_memcpy_d2d_async(out.data_ptr(), r.image.data_ptr(), W * H * 12)
        hip.synchronize()
    finally:
        hip.set_sync(True)
    return out.cpu().numpy(), e


def test_frames_in_flight(hip):
    """rs_set_sync(0), side stream 4: partial edits between frames that are still in flight give the image of the synchronous run."""
    hip.set_side_stream(4)
    want, _ = frames_with_edits(hip, True)
    got, e = frames_with_edits(hip, False)
    assert bits_equal(want, got)
    assert e.s.refit_counts() == (1, 2)
    assert_tables(e.expected(), e.s, "in flight")


# ---- 5. the mode off ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "soup3"])
def test_mode_off_counts_whole_refits_only(hip, name):
    sd = scene_data(name)
    s = make_scene(hip, name)
    snap = snapshot_of(name)
    v, n = sd.vertices.reshape(-1, 3, 3).copy(), sd.normals.reshape(-1, 3, 3).copy()
    for j, kind in enumerate(("one", "carry", "carry_back")):
        ids, ev, en = geometry_edit(sd, v, kind, seed=11)
        s.set_triangles(ids, ev, en)
        v, n = apply_triangles(v, n, ids, ev, en)
        assert s.refit_counts() == (j + 1, 0) and s.refit_dirty() == 0
        assert_tables(snap.expected(v, n), s, (name, kind))
