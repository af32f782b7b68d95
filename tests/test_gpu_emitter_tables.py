"""The device tables rs_scene_set_geometry rewrites, record by record and bit for bit, against the host restatement of
tests/emitter_tables.py (the emissive tree) and tests/refit_tables.py (the other ten tables).  Rays and images cannot tell a box that is
too large from a right one, nor a write where none belongs, and a box of the emissive tree that is too small shows only when a last
bounce happens to pass it.  After every kind of edit: every emiTris record with its pads, every emiNodes record -- the box dwords equal
grid_box of the union of the triangles' AABBs below the record on the grid the hook reports, w and the end record are the snapshot's --,
the reported grid equals that of a scene created afresh from the host description and the NumPy restatement of the grid function, and
the other tables equal refit_tables' expectations.  An edit that names no emitter leaves emiNodes / emiTris byte-identical."""
import numpy as np
import pytest

from oracle import binding as ob
from tests.common import bits_equal, hip_scene
from tests.emitter_edits import SCENES, edits_up_to, emissive_root_box, emitters, kinds_for, scene_data
from tests.emitter_tables import EmissiveSnapshot, grid_over_box
from tests.geometry_edits import geometry_edit
from tests.refit_tables import assert_tables, first_difference

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def synchronous(hip):
    hip.set_sync(True)
    yield
    hip.set_sync(True)


def second_scene(capi, sd, s):
    v, n = s.geometry()
    d = s.host_desc()
    env = d["env_map_tex"] >= 0
    return capi.Scene.from_tables(v, n, sd.texcoords, sd.material_ids, d["materials"], d, textures=d["textures"], env_map_tex=d["env_map_tex"],
                                  env_sampler=(d["env_prob"], d["env_fail"]) if env else None)


@pytest.mark.parametrize("name", list(SCENES))
def test_tables_after_every_kind(hip, name):
    sd = scene_data(name)
    s = hip_scene(hip, sd)
    others = sd.num_prims <= 5000                        # the other ten tables: on the four scenes where their Python restatement takes no seconds
    snap = EmissiveSnapshot(s, emitters(sd), others)
    assert s.debug_grid()["occ_count"] > 0 and snap.emi_grid["state"] == 1 and snap.emi_grid["count"] >= 1
    lo, hi = emissive_root_box(sd, sd.vertices)
    g = grid_over_box(lo, hi)
    assert bits_equal(snap.emi_grid["base"], g["base"]) and bits_equal(snap.emi_grid["scale"], g["scale"]) and snap.emi_grid["margin"] == g["margin"]
    stale = None
    for kind in kinds_for(name):
        edits, _, v, n = edits_up_to(name, kind)
        s.set_geometry(*edits[-1])
        grid = s.emissive_grid()
        # (the scene created afresh: after every kind on the small scenes, after two on the large one, where creating it takes a second;
        #  the NumPy restatement of the grid function stands in between)
        fresh = second_scene(hip, sd, s).emissive_grid() if others or kind in ("carry_max", "flip", "collapse_all") else None
        assert grid["count"] == snap.emi_grid["count"], kind
        if kind == "collapse_all":                       # no extent: off, as a fresh build leaves it; the records keep what they held
            assert grid["state"] == 0 and fresh["state"] == 0 and fresh["count"] == 0, (kind, grid, fresh)
            want = snap.expected_all(v, n, None, others)
            want["emiNodes"] = stale
        else:
            lo, hi = emissive_root_box(sd, v)
            g = grid_over_box(lo, hi)
            for other in (g,) if fresh is None else (g, fresh):
                assert grid["state"] == 1 and other.get("state", 1) == 1, (kind, grid, other)
                assert bits_equal(grid["base"], other["base"]) and bits_equal(grid["scale"], other["scale"]) and grid["margin"] == other["margin"], (kind, grid, other)
            want = snap.expected_all(v, n, grid, others)
            stale = want["emiNodes"]
        assert_tables(want, s, (name, kind), only=list(want))
        got = s.debug_table("emiNodes")
        assert np.array_equal(got["w"], snap.tables["emiNodes"]["w"]) and got[-1].tobytes() == snap.tables["emiNodes"][-1].tobytes(), kind


@pytest.mark.parametrize("name", ["cornell", "many"])
def test_an_edit_that_names_no_emitter_writes_no_emissive_byte(hip, name):
    """rs_scene_set_geometry with triangles that are no emitters, on a fresh scene and after an emitter edit: emiNodes and emiTris stay
    byte for byte, the grid stays, no light table changes, and the other tables are those of rs_scene_set_triangles."""
    sd = scene_data(name)
    s = hip_scene(hip, sd)
    snap = EmissiveSnapshot(s, emitters(sd))
    desc = s.host_desc()
    ids, v, n = geometry_edit(sd, sd.vertices, "all", seed=5)
    s.set_geometry(ids, v, n)
    cur = sd.vertices.reshape(-1, 3, 3).copy(); cur[ids] = v
    assert_tables(snap.expected(cur, sd.normals), s, (name, "plain"))          # (expected(): emiNodes / emiTris are the snapshot's)
    assert repr(s.emissive_grid()) == repr(snap.emi_grid)
    after = s.host_desc()
    assert bits_equal(after["light_prob"], desc["light_prob"]) and after["sum_power"] == desc["sum_power"]
    edit = edits_up_to(name, "one")[0][-1]
    s.set_geometry(*edit)
    cur[edit[0]] = edit[1]
    nodes, tris, grid = s.debug_table("emiNodes"), s.debug_table("emiTris"), s.emissive_grid()
    assert first_difference("emiTris", snap.tables["emiTris"], tris) is not None and not bits_equal(grid["base"], snap.emi_grid["base"])
    ids, v, n = geometry_edit(sd, cur, "one", seed=6)
    s.set_geometry(ids, v, n)
    assert first_difference("emiNodes", nodes, s.debug_table("emiNodes")) is None
    assert first_difference("emiTris", tris, s.debug_table("emiTris")) is None
    assert repr(s.emissive_grid()) == repr(grid)
