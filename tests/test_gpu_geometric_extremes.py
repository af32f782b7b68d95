"""GPU: the grid-box tree walks on the scenes of tests/geometric_cases.py, held to the CPU oracle bit for bit.

The shadow tree, the ordered closest-hit trees and the emissive tree store their boxes on a 16-bit grid over the scene's root box
(rs_grid.h grid_box, occlusion_bvh.cpp rs_quantize_occlusion_bvh, rs_walk.h GridRay / grid_reaches, scene.hip build_occlusion_side).
That a walk through them returns what the reference's walk returns rests on an error argument -- planes pushed out by 2^-17 of the
extent, an apron of 200 steps below the root box, a slow lane for rays that start more than 4 grid extents away, a fall-back to the
reference's tree when a box does not fit -- and every other module walks scenes near the origin, a few units across, roughly cubic
and far coarser than a grid step.  Here the scenes are far from the origin, on the last two ulps of the apron and beyond it, huge, as small as the reference renders,
a slab 64 steps across, one step thick, with triangles inside one cell, exact duplicates, slivers and triangles without area, and
edited into such places (case x base, 20 in all; tests/test_geometric_cases.py asserts on the CPU that each is what it claims).

Per case, nothing masked or sampled -- every ray, every segment and every pixel:
  * the path taken: rs_debug_scene_grid reports a shadow tree and closest-hit trees exactly where the NumPy restatement says the grid
    fits, on the restated base, scale and margin; where it does not fit there are no trees and every query is still answered;
  * closest hit: the generator's 4 133 rays and the case's aimed ones, shuffled so that every wave mixes kinds, through trace_closest,
    trace_closest_wave with the ordered trees and trace_closest_wave without them: primitive and material of every ray, position and
    normal bits of every hit, equal to the oracle's;
  * occlusion: the same for the segments through trace_occlusion, equal to the oracle's testOcclusion and to the library's own walk of
    the reference's tree (a scene created under RS_NO_OCCLUSION_TREE);
  * frames at 48 x 32 (and at 97 x 61 for `far` and `sub_cell`): three frames of ReSTIRDirect with reuse 3 -- every G-buffer plane,
    radiance, both reservoir buffers and the ray count after each -- then the PT-direct baseline and pathTrace at depth 4 with cos / sin
    / atan2 correctly rounded on both sides, which puts the emissive tree and the bounce-ray service on the same geometry;
  * `edited_into_extremes`: all of the above after rs_scene_set_triangles, with one frame; the oracle's side is the edited vertices
    under the threaded orders of the scene as created and boxes refitted in NumPy.

Beside the grid, the axis cull of the reference walk (rs_intersect.h skip_far_on_axis, switched per scene by scene.hip far_skip_allowed):
a ray inside a triangle's plane with a zero direction component "hits" that triangle through rounding wherever it runs in the plane,
unless the reference's absolute FLT_EPSILON rejects the determinant, which it does only in scenes of small triangles.  `huge`,
`sub_cell` and `edited_into_extremes` hold such hits; test_in_plane_rays_in_a_room_four_units_wide has them at an everyday scale, and
test_an_edit_that_brings_large_triangles in a scene whose cull is on until rs_scene_set_triangles brings the triangles that forbid it."""
import numpy as np
import pytest

from tests import extreme_cases as xc
from tests import geometric_cases as gc
from tests.common import HipRenderer, bits_equal, hip_scene

pytestmark = pytest.mark.gpu


@pytest.fixture
def correctly_rounded_libm():
    """The library evaluates cos / sin / atan2 correctly rounded, so the oracle does too; the fixture owns the mode for the whole test
    body (geometric_cases.oracle_frames asserts that it runs inside it)."""
    with xc.correctly_rounded_libm():
        yield


def _create(hip, c):
    """The library's scene of a case: created from the scene data, then edited where the case has an edit.  Returns it with the grid
    it reported at creation."""
    s = hip_scene(hip, c.sd)
    s.set_sample_sequence(None)
    grid = s.debug_grid()
    if c.edit is not None:
        if grid["occ_count"] > 0:                             # the corner triangles: corners of the creation-time root box exactly
            corners = c.edit[1][64:].reshape(-1, 3)
            assert ((corners == grid["lo"]) | (corners == grid["hi"])).all(), "the case's corner triangles are not on the grid's box"
        s.set_triangles(*c.edit)
    return s, grid


@pytest.fixture(scope="module")
def scenes(hip):
    """{(name, base): (scene, grid at creation)}, each built once."""
    made = {}

    def get(name, base):
        if (name, base) not in made:
            made[name, base] = _create(hip, gc.case(name, base))
        return made[name, base]
    yield get
    for s, _ in made.values():
        s.destroy()


CASES = pytest.mark.parametrize("name,base", gc.CASES, ids=gc.CASE_IDS)


@CASES
def test_the_path_taken(hip, scenes, name, base):
    c = gc.case(name, base)
    s, grid = scenes(name, base)
    want = gc.grid_of(c.sd.vertices)
    assert want["exists"] == gc.EXPECT[name, base]["grid"]
    assert (grid["occ_count"] > 0) == want["exists"] and (grid["ord_stride"] > 0) == want["exists"], (grid, want)
    if want["exists"]:
        for k in ("base", "scale", "lo", "hi"):
            assert bits_equal(grid[k], want[k]), (k, grid[k], want[k])
        assert grid["margin"] == want["margin"]
        assert s.debug_grid()["occ_count"] == grid["occ_count"]          # an edit keeps the trees
        assert hip.set_ordered_tree(s, True)
    else:
        assert grid["occ_count"] == 0 and grid["ord_stride"] == 0
        assert not hip.set_ordered_tree(s, True) and not hip.set_ordered_tree(s, True)      # no trees, and asking for them makes none


def _same_as_the_oracle(want, got, where):
    prim, mat, pos, nrm = want
    gp, gm, gpos, gn = [t.cpu().numpy() for t in got]
    bad = np.nonzero(prim != gp)[0]
    assert not len(bad), (where, "primitive", len(bad), bad[:8], prim[bad[:8]], gp[bad[:8]])
    h = prim >= 0
    assert np.array_equal(mat[h], gm[h]), (where, "material")
    assert bits_equal(pos[h], gpos[h]) and bits_equal(nrm[h], gn[h]), (where, "position / normal bits")


@CASES
def test_closest_hit_equals_the_oracle_on_every_ray(hip, scenes, name, base):
    import torch
    c = gc.case(name, base)
    s, grid = scenes(name, base)
    want = gc.oracle_hits(name, base)
    assert (want[0][~c.aimed_rays] >= 0).mean() >= gc.MIN_HITS
    dr = torch.from_numpy(c.rays).cuda()
    _same_as_the_oracle(want, hip.trace_closest(s, dr), (name, base, "trace_closest"))
    had = hip.set_ordered_tree(s, True)
    assert had == (grid["ord_stride"] > 0)
    try:
        _same_as_the_oracle(want, hip.trace_closest_wave(s, dr), (name, base, "trace_closest_wave, ordered trees on"))
        assert hip.set_ordered_tree(s, False) == had
        _same_as_the_oracle(want, hip.trace_closest_wave(s, dr), (name, base, "trace_closest_wave, ordered trees off"))
    finally:
        hip.set_ordered_tree(s, True)


@CASES
def test_occlusion_equals_the_oracle_on_every_segment(hip, scenes, monkeypatch, name, base):
    import torch
    c = gc.case(name, base)
    s, _ = scenes(name, base)
    want = gc.oracle_occlusion(name, base)
    assert 0.05 < want[~c.aimed_segs].mean() < 0.95
    dseg = torch.from_numpy(c.segs).cuda()
    got = hip.trace_occlusion(s, dseg).cpu().numpy()
    bad = np.nonzero(want != got)[0]
    assert not len(bad), (name, base, "against the oracle", len(bad), bad[:8], want[bad[:8]], got[bad[:8]])
    monkeypatch.setenv("RS_NO_OCCLUSION_TREE", "1")
    slow, slow_grid = _create(hip, c)
    monkeypatch.delenv("RS_NO_OCCLUSION_TREE")
    try:
        assert slow_grid["occ_count"] == 0 and slow_grid["ord_stride"] == 0
        ref = hip.trace_occlusion(slow, dseg).cpu().numpy()
    finally:
        slow.destroy()
    assert np.array_equal(ref, got), (name, base, "against the reference's tree", int((ref != got).sum()))


class HipFrames:
    """The library behind the interface geometric_cases.run_frames drives (its OracleFrames is the other one)."""

    def __init__(self, hip, sd, scene, size):
        self.hip, self.sd, self.shared, self.size, self.n = hip, sd, scene, size, size[0] * size[1]

    def renderer(self):
        return HipRenderer(self.hip, self.sd, *self.size, scene=self.shared)

    def last(self, r):
        return r.restir.download(1)

    def temp(self, r):
        return r.restir.download(2)

    def gbuffer(self, r):
        g = r.gbuf.download()
        f = g["frame_idx"] ^ 1
        return dict(prim_id=g["prim_id"][f], albedo=g["albedo"], normal=g["normal"][f], depth=g["depth"][f], motion=g["motion"])

    def path_trace(self, r, looper, depth):
        import torch
        d = torch.zeros((self.n, 3), dtype=torch.float32, device="cuda"); i = torch.zeros_like(d)
        rays = self.hip.path_trace(r.scene, r.cam, d.data_ptr(), i.data_ptr(), 0, looper, depth)
        return d.cpu().numpy(), i.cpu().numpy(), rays


FRAMES = [(n, b, gc.SIZE) for n, b in gc.CASES] + [(n, b, gc.RAGGED) for n, b in gc.CASES if n in gc.RAGGED_TOO]


@pytest.mark.parametrize("name,base,size", FRAMES, ids=["%s-%s-%dx%d" % (n, b.split(":")[0], *s) for n, b, s in FRAMES])
def test_frames_equal_the_oracle_on_every_pixel(hip, scenes, correctly_rounded_libm, name, base, size):
    c = gc.case(name, base)
    s, _ = scenes(name, base)
    want = gc.oracle_frames(name, base, size)
    assert gc.coverage(want["direct/f0/gbuffer/prim_id"]) >= gc.MIN_COVERAGE
    got = gc.run_frames(HipFrames(hip, c.after, s, size), *gc.frames_of(name))
    assert xc.compare(want, got, (name, base, size)) == {}          # bit for bit, and no NaN on either side


def _every_service_equals_the_oracle(hip, s, sc, rays, segs):
    import torch
    want = sc.intersect(rays)[:4]
    dr = torch.from_numpy(rays).cuda()
    _same_as_the_oracle(want, hip.trace_closest(s, dr), "trace_closest")
    assert hip.set_ordered_tree(s, True)
    _same_as_the_oracle(want, hip.trace_closest_wave(s, dr), "trace_closest_wave, ordered trees on")
    hip.set_ordered_tree(s, False)
    _same_as_the_oracle(want, hip.trace_closest_wave(s, dr), "trace_closest_wave, ordered trees off")
    hip.set_ordered_tree(s, True)
    occ = sc.test_occlusion(segs)
    got = hip.trace_occlusion(s, torch.from_numpy(segs).cuda()).cpu().numpy()
    assert np.array_equal(occ, got), ("trace_occlusion", int((occ != got).sum()), np.nonzero(occ != got)[0][:8])
    return want[0]


def test_in_plane_rays_in_a_room_four_units_wide(hip):
    """The Cornell box scaled by 2: rays inside a wall's plane with a zero direction component "hit" the wall through rounding although
    they run beside it, because a determinant of 2^-27 * 16 passes the reference's FLT_EPSILON.  The oracle reports such hits
    (tests/test_geometric_cases.py asserts that there are some); every closest-hit service must report them too, and trace_occlusion,
    whose slow lanes walk with the same cull, must agree on the generator's segments."""
    sd, rays, segs = gc.scaled_room()
    s = hip_scene(hip, sd)
    try:
        prim = _every_service_equals_the_oracle(hip, s, gc.oracle_scene(sd), rays, segs)
        assert gc.hits_beside_the_ray(sd, rays, prim) > 0
    finally:
        s.destroy()


def test_an_edit_that_brings_large_triangles(hip):
    """gc.edit_room(): a scene of small triangles, in which the axis cull runs, until rs_scene_set_triangles stretches six of them over
    the root box.  From then on rays inside their planes hit them beside the ray (410 of the 8 192 on the oracle); the edit must have
    switched the cull off.  Before the edit and after it every service equals the oracle."""
    sd, edit, after, rays, segs = gc.edit_room()
    s = hip_scene(hip, sd)
    try:
        _every_service_equals_the_oracle(hip, s, gc.oracle_scene(sd), rays, segs)
        s.set_triangles(*edit)
        prim = _every_service_equals_the_oracle(hip, s, gc.edit_room_oracle(), rays, segs)
        assert gc.hits_beside_the_ray(after, rays, prim) >= 100
    finally:
        s.destroy()
