"""What the GPU tests of the primary cuts and leaf lists share (tests/test_gpu_primary_cuts.py, tests/test_gpu_primary_leaf_lists.py): the
scaled scenes and their views, one side of a comparison (Side), the three-way loop -- a switch on, the switch off, the CPU oracle, bit
for bit after every frame --, "used after the build", and the two sides, frame loop and changes of the invalidation tests."""
import numpy as np

from tests import geometric_cases as gc
from tests import part_transforms as pt
from tests.common import HipRenderer, OracleRenderer, bits_equal, get_scene, hip_scene, oracle_scene
from tests.geometry_edits import geometry_edit
from tests.scene_edits import assert_same

SCALE = {"cornell": 0.45, "sponza:0.03": 0.25}


def fast_form(sd):
    """scene.hip far_skip_allowed: the largest product of a triangle's two edge extents is at most 1."""
    v = sd.vertices.reshape(-1, 3, 3)
    return float((np.abs(v[:, 1] - v[:, 0]).max(1) * np.abs(v[:, 2] - v[:, 0]).max(1)).max()) <= 1.0


def small(name):
    sd = get_scene(name)
    gc._affine(sd, scale=(SCALE[name],) * 3)
    assert fast_form(sd)
    return sd


# The Sponza-class scene seen at an angle through a narrow lens: no direction component changes sign inside the frame and one traversal
# order covers nearly all of it, so most blocks take a cut (its own camera looks along -z: two thirds of the blocks straddle a sign
# change or an order change and keep the tree)
TURNED = dict(rotation=(-65.0, -15.0, 0.0), fov_y=12.0)


def view(sd, **camera):
    sd = small(sd) if isinstance(sd, str) else sd
    if camera:
        sd.camera_args = dict(sd.camera_args, **camera)
    return sd


def _set_axes(cam, view, right, up):
    """The camera's basis written exactly (rs_camera_update derives it from angles, whose cosines are never exactly 0)."""
    for i in range(3):
        cam.view[i], cam.right[i], cam.up[i] = view[i], right[i], up[i]
    for col in range(3):                             # the inverse of an orthonormal basis is its transpose; [col * 3 + row]
        for row, axis in enumerate((right, up, view)):
            cam.rotationMatInv[col * 3 + row] = axis[col]


# ---- one side of a comparison: frames over rows [y0, y1) ------------------------------------------------------------------------------
class Side:
    """hip: the library (cuts / lists: its two switches, None leaves one alone; cap / list_cap: the test hooks' caps) or, None, the
    oracle.  Per frame of a library side: info (rs_debug_primary_cut_info) and lists (rs_debug_primary_leaf_list_info)."""

    def __init__(self, hip, sd, size, rows=None, scene=None, cuts=True, cap=None, lists=None, list_cap=None, axes=None):
        self.hip, self.W, self.H = hip, size[0], size[1]
        self.rows = rows or (0, size[1])
        self.r = HipRenderer(hip, sd, *size, scene=scene) if hip else OracleRenderer(sd, *size, scene=scene)
        if axes:
            _set_axes(self.r.cam, *axes)
        if hip:
            self.r.restir.set_primary_cuts(cuts)
            if cap:
                self.r.restir.set_primary_cut_cap(cap)
            if lists is not None:
                self.r.restir.set_primary_leaf_lists(lists)
            if list_cap is not None:
                self.r.restir.set_primary_leaf_list_cap(list_cap)
        self.info, self.lists = [], []

    def frame(self):
        r, (y0, y1) = self.r, self.rows
        r.gbuf.render(r.scene, r.cam, y0, y1)
        r.restir.phase_a(r.scene, r.cam, r.gbuf, r.looper, 3, y0, y1)
        r.restir.phase_b(r.scene, r.cam, r.gbuf, r.image.data_ptr() if self.hip else r.image, 0, 3, y0, y1)
        r.restir.end_frame()
        if self.hip:
            r.rays = r.restir.ray_count()
            self.info.append(r.restir.primary_cut_info())
            self.lists.append(r.restir.primary_leaf_list_info())
        else:
            r.rays = r.restir.rays
        r.looper += 1
        r.gbuf.update(r.cam)
        return self.state()

    def _rows(self, a):
        return np.ascontiguousarray(a[self.rows[0] * self.W:self.rows[1] * self.W])

    def state(self):
        r = self.r
        if self.hip:
            planes = dict(image=r.image.cpu().numpy(), cur=r.restir.download(0), last=r.restir.download(1), temp=r.restir.download(2))
        else:
            planes = dict(image=r.image.copy(), cur=r.restir.reservoir.copy(), last=r.restir.last.copy(), temp=r.restir.temp.copy())
        return dict(rays=int(r.rays), **{k: self._rows(v) for k, v in planes.items()})

    def surface(self):
        return [self._rows(a) for a in self.r.restir.surface()]


def used_after_build(records, frames):
    """The one build of a still camera, and the cuts (lists) walked by exactly the frames after it."""
    builds = [i["builds"] for i in records]
    assert builds[-1] == 1 and builds[0] == 0, builds
    built_in = builds.index(1)
    assert [i["used"] for i in records] == [f > built_in for f in range(frames)], (builds, [i["used"] for i in records])
    assert built_in + 1 < frames
    return built_in


def three_way(hip, sd, size, rows=None, frames=6, overlapped=False, toggle="cuts", **kw):
    """toggle: "cuts" or "lists", the switch that is on on the first side and off on the second (whose records of it, Side.info or
    Side.lists, stay empty); kw: Side's, the toggled kind's cap for the first side alone.  Returns the first side."""
    record, cap = {"cuts": ("info", "cap"), "lists": ("lists", "list_cap")}[toggle]
    plain = {k: v for k, v in kw.items() if k != cap}
    scene_h, scene_o = hip_scene(hip, sd), oracle_scene(sd)
    scene_h.set_sample_sequence(None); scene_o.set_sample_sequence(None)
    on = Side(hip, sd, size, rows, scene=scene_h, **{toggle: True}, **kw)
    off = Side(hip, sd, size, rows, scene=scene_h, **{toggle: False}, **plain)
    ref = Side(None, sd, size, rows, scene=scene_o, **plain)
    hip.set_sync(not overlapped)
    try:
        for f in range(frames):
            a, b, c = on.frame(), off.frame(), ref.frame()
            assert_same(c, a, "%s on against the oracle, frame %d" % (toggle, f))
            assert_same(c, b, "%s off against the oracle, frame %d" % (toggle, f))
            for k, (x, y) in enumerate(zip(on.surface(), off.surface())):
                assert bits_equal(x, y), ("surface plane %d, frame %d" % (k, f))
    finally:
        hip.synchronize()
        hip.set_sync(True)
    assert a["image"].any() and a["rays"] > 0
    assert all(i["builds"] == 0 and not i["used"] and i["records"] == 0 for i in getattr(off, record)), getattr(off, record)
    if toggle == "lists":
        assert all(i["used"] == j["used"] for i, j in zip(on.info, off.info))             # the cuts themselves are built and walked on both sides
    return on


# ---- invalidation: the library and the oracle side by side, a change between their frames -------------------------------------------------
SIZE = (96, 54)
BOX = list(range(10, 22))                            # the tall box of the Cornell scene


def sides(hip):
    from tests import emitter_edits as ee
    sd = small("cornell")
    h, o = ee.HipSide(hip, sd, *SIZE), ee.OracleSide(hip, sd, *SIZE)
    h.r.scene.define_parts([BOX])
    return sd, h, o


def frames_of(h, o, n, tag, lists=False):
    """n frames on both sides, equal after each; per frame the cuts' info, or the lists'."""
    out = []
    for f in range(n):
        h.r.frame(3); o.r.frame(3)
        assert_same(o.direct_state(), h.direct_state(), "%s, frame %d" % (tag, f))
        out.append(h.r.restir.primary_leaf_list_info() if lists else h.r.restir.primary_cut_info())
    return out


def move_camera(hip, sd, h, o):
    p = sd.camera_args["position"]
    for s in (h, o):
        s.r.set_camera_position((p[0] + 0.02, p[1], p[2]))


def move_one_triangle(hip, sd, h, o):
    ids, v, n = geometry_edit(sd, sd.vertices, "one")
    for s in (h, o):
        s.set_triangles(ids, v, n)


def refit(hip, sd, h, o):
    """rs_scene_set_geometry of the tall box's triangles, moved a little: the device refit."""
    ids = np.arange(10, 22, dtype=np.int32)
    v = sd.vertices.reshape(-1, 3, 3)[ids] + np.float32(0.004)
    for s in (h, o):
        s.set_geometry(ids, v)


def turn_a_part(hip, sd, h, o):
    """rs_scene_set_part_transforms on the library; on the oracle the geometry edit that equals it (rs_bake_matrix of the rest pose)."""
    v, n = pt.rest_of(sd, BOX)
    m = pt.rotation_about(v.reshape(-1, 3).astype(np.float64).mean(0), (0, 1, 0), 3.0, (0.01, 0.005, 0.01))
    bv, bn = hip.bake_matrix(m, v, n)
    h.r.scene.set_part_transforms([0], [m])
    o.set_geometry(np.asarray(BOX, np.int32), bv.reshape(-1, 3, 3), bn.reshape(-1, 3, 3))
