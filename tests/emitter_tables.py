"""What emiNodes and emiTris must hold after rs_scene_set_geometry, restated in NumPy in the manner of tests/refit_tables.py (which this
imports and does not change): helpers of tests/test_emitter_tables_host.py and tests/test_gpu_emitter_tables.py.  The topology is read
from the `w` words of a snapshot taken BEFORE the first edit; the expected records are then a function of the snapshot, the edited
vertices and the grid the debug hook reports (which the tests hold to the grid of a scene created afresh)."""
import numpy as np

from tests.refit_tables import GridTree, Snapshot, grid_box


def slot_prims(emi_tris, tris, emitters):
    """The primitive in every slot of emiTris.  The records carry no id, so a slot is matched to the emitter with the same nine floats
    (emitters with identical vertices are interchangeable; each is used once)."""
    key = lambda a: np.concatenate([a["v0"], a["e1"], a["e2"]], 1).view(np.uint32)
    left = {}
    for p, k in zip(emitters, key(tris[emitters])):
        left.setdefault(k.tobytes(), []).append(int(p))
    return np.array([left[k.tobytes()].pop(0) for k in key(emi_tris)], np.int64)


class EmissiveSnapshot(Snapshot):
    """refit_tables.Snapshot plus the emissive tree: its records [0, count) of emiNodes, the end record after them."""

    def __init__(self, scene, emitters, others=True):
        """others = False: the emissive tables alone (refit_tables.Snapshot parses the reference tree and seven grid-box trees record by
        record in Python, which takes seconds on a scene of 10^5 triangles)."""
        if others:
            super().__init__(scene)
        else:
            self.tables = {name: scene.debug_table(name).copy() for name in ("tris", "emiNodes", "emiTris")}
            self.num_prims = len(self.tables["tris"])
        t = self.tables
        self.emitters = np.asarray(emitters, np.int64)
        self.emi_grid = scene.emissive_grid()
        count = self.emi_grid["count"]
        assert len(t["emiNodes"]) == count + 1 and len(t["emiTris"]) == len(self.emitters)
        assert tuple(t["emiNodes"][count]["box"]) == (0xffffffff, 0x0000ffff, 0) and t["emiNodes"][count]["w"] == count * 16      # the end record
        self.emi_prims = slot_prims(t["emiTris"], t["tris"], self.emitters)
        self.emi_tree = GridTree(t["emiNodes"], 0, count, 0, count * 16, self.emi_prims, 1)

    def expected_emissive(self, vertices, grid):
        """(emiNodes, emiTris) for a scene whose triangles are now `vertices`, on the emissive grid `grid` (dict of base, scale, margin):
        every record's box is grid_box of the union of the triangles' AABBs below it; w, the end record and the pads stay.  grid None
        (the tree is off: no extent): emiNodes is None, the triangle records are written all the same."""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3, 3)
        nodes, tris = self.tables["emiNodes"].copy(), self.tables["emiTris"].copy()
        p = self.emi_prims
        tris["v0"], tris["e1"], tris["e2"] = v[p, 0], v[p, 1] - v[p, 0], v[p, 2] - v[p, 0]
        if grid is None:
            return None, tris
        lo, hi = self.emi_tree.boxes(v.min(1), v.max(1))
        q, fits = grid_box(lo, hi, grid["base"], grid["scale"], grid["margin"])
        assert fits.all(), "an emissive box does not fit the emissive grid"
        nodes["box"][:self.emi_tree.count] = q
        return nodes, tris

    def expected_all(self, vertices, normals, grid, others=True):
        """Every table: refit_tables' expectations for the other ten (they do not depend on which call made the edit; others = False
        leaves them out: their restatement walks the reference tree node by node in Python), ours for the two."""
        out = self.expected(vertices, normals) if others else {}
        out["emiNodes"], out["emiTris"] = self.expected_emissive(vertices, grid)
        return out


def triangle_area(vertices):
    """Math::triangleArea of (n, 3, 3) float32 triangles: length(cross(v1 - v0, v2 - v0)) / 2, one float32 rounding per operation, sums
    from the left."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3, 3)
    a, b = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    c = np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2], a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0], a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], 1)
    return np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]) * np.float32(0.5)


def light_sampler_tables(capi, vertices, light_prims, radiance, env_power=None):
    """(area, prob, fail, sumAll) of the light sampler over the light primitives of `vertices`: rs_build_light_table's power per light,
    luminance(radiance) * 2 * pi * area in float32, the environment map's entry (env_power, if any) last, then the library's alias table."""
    area = triangle_area(np.asarray(vertices, np.float32).reshape(-1, 3, 3)[np.asarray(light_prims, np.int64)])
    r = np.asarray(radiance, np.float32).reshape(-1, 3)
    lum = r[:, 0] * np.float32(0.2126) + r[:, 1] * np.float32(0.7152) + r[:, 2] * np.float32(0.0722)
    power = lum * np.float32(2.0) * np.float32(np.pi) * area
    if env_power is not None:
        power = np.concatenate([power, np.float32([env_power])])
    prob, fail, total = capi.build_alias_table(power)
    return area, prob, fail, total


def grid_over_box(lo, hi):
    """The grid a grid-box tree with root box [lo, hi] lies on, as the library's one function lays it: the largest extent over 65 000
    steps on every axis, 200 steps of apron below lo, a margin of 2^-17 of the extent.  float32 arithmetic, one rounding per operation."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    ext = np.float32((hi - lo).max())
    scale = np.full(3, ext / np.float32(65000.0), np.float32)
    base = (lo - np.float32(200.0) * scale).astype(np.float32)
    return dict(base=base, scale=scale, margin=float(np.ldexp(np.float64(ext), -17)))
