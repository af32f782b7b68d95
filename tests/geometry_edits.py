"""Helpers of tests/test_gpu_geometry_edits.py, tests/test_gpu_refit_tables.py and tests/test_geometry_refit_host.py: triangle edits (rs_scene_set_triangles) driven
through the oracle and the library alike.  The oracle has no edit of its own: its side of an edit is a fresh oracle.binding.Scene made
from the edited vertices and normals, with the old threaded orders and the boxes refitted by capi.refit_boxes (rs_refit_boxes, host
only) handed over as `prebuilt` -- never boxes read back from the scene under test."""
import numpy as np

from oracle import binding as ob
from tests.scene_edits import HipSide as _HipSide, OracleSide as _OracleSide

LIGHT = 4
EDIT_KINDS = ("carry", "carry_back", "one", "all", "repeated")


def movable(sd):
    """The primitives an edit may name: every triangle whose material is not a Light."""
    return np.nonzero(sd.materials["type"][sd.material_ids] != LIGHT)[0].astype(np.int32)


def root_box(vertices):
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    return v.min(0), v.max(0)


def numpy_refit(vertices, order0):
    """rs_refit_boxes restated: leaf = min / max of the three vertices, inner = min / max of its two children (children of the record
    at i of order 0: i + 1 and the miss link of i + 1).  Boxes by boundingBoxId.  np.minimum / np.maximum: -0 == +0, compare as values."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3, 3)
    o = np.asarray(order0, np.int32).reshape(-1, 3)
    boxes = np.zeros((len(o), 6), np.float32)
    for i in range(len(o) - 1, -1, -1):                      # pre-order: children come after their parent
        prim, box_id, _ = o[i]
        if prim >= 0:
            boxes[box_id, :3], boxes[box_id, 3:] = v[prim].min(0), v[prim].max(0)
        else:
            a, b = o[i + 1, 1], o[o[i + 1, 2], 1]
            boxes[box_id, :3] = np.minimum(boxes[a, :3], boxes[b, :3])
            boxes[box_id, 3:] = np.maximum(boxes[a, 3:], boxes[b, 3:])
    return boxes


def tree_children(order0):
    """[(boundingBoxId of a node, of its first child, of its second child)] for the inner nodes, and {primitive: boundingBoxId of its leaf}."""
    o = np.asarray(order0, np.int32).reshape(-1, 3)
    inner = [(o[i, 1], o[i + 1, 1], o[o[i + 1, 2], 1]) for i in range(len(o)) if o[i, 0] < 0]
    leaves = {int(o[i, 0]): int(o[i, 1]) for i in range(len(o)) if o[i, 0] >= 0}
    return inner, leaves


def tree_depth(order0):
    o = np.asarray(order0, np.int32).reshape(-1, 3)
    ends, deepest = [], 0
    for i in range(len(o)):
        while ends and ends[-1] <= i:
            ends.pop()
        ends.append(o[i, 2])
        deepest = max(deepest, len(ends))
    return deepest


def apply_triangles(vertices, normals, ids, v, n=None):
    """The arrays after the edit; a repeated id takes its last record."""
    vertices = np.array(vertices, np.float32).reshape(-1, 3, 3)
    normals = np.array(normals, np.float32).reshape(-1, 3, 3)
    v = np.asarray(v, np.float32).reshape(-1, 3, 3)
    for j, p in enumerate(np.asarray(ids).reshape(-1)):
        vertices[p] = v[j]
        if n is not None:
            normals[p] = np.asarray(n, np.float32).reshape(-1, 3, 3)[j]
    return vertices, normals


def corner_triangle(sd):
    """The movable triangle whose centroid is nearest the minimum corner of the scene."""
    lo, _ = root_box(sd.vertices)
    ids = movable(sd)
    c = sd.vertices.reshape(-1, 3, 3)[ids].mean(1)
    return int(ids[np.argmin(np.linalg.norm(c - lo, axis=1))])


def geometry_edit(sd, vertices, kind, seed=0):
    """(ids, vertices, normals or None) of the edit `kind`, given the scene's current `vertices`; every vertex stays inside the root box
    of sd.vertices (the box the scene was created with) and no emissive triangle is named."""
    rng = np.random.default_rng(seed)
    cur = np.asarray(vertices, np.float32).reshape(-1, 3, 3)
    orig = sd.vertices.reshape(-1, 3, 3)
    lo, hi = root_box(orig)
    ids = movable(sd)
    ext = (hi - lo).astype(np.float32)

    def inside(v):
        return np.clip(v, lo, hi).astype(np.float32)
    if kind == "one":
        p = int(ids[len(ids) // 2])
        v = inside(cur[p] + ext * np.float32(0.11) * np.array([1, -1, 0.5], np.float32))
        n = rng.normal(size=(3, 3)); n /= np.linalg.norm(n, axis=1, keepdims=True)
        return np.array([p], np.int32), v[None], n.astype(np.float32)[None]
    if kind == "all":
        v = inside(cur[ids] + rng.uniform(-0.03, 0.03, (len(ids), 3, 3)) * ext)
        return ids, v, None
    if kind == "repeated":
        a, b = int(ids[1]), int(ids[-2])
        first = inside(cur[a] + ext * np.float32(0.2))
        last = inside(cur[a] - ext * np.float32(0.07))
        other = inside(cur[b] * np.float32(0.9) + np.float32(0.1) * (lo + hi) / 2)
        return np.array([a, b, a], np.int32), np.stack([first, other, last]), None
    if kind == "carry":                                   # from the minimum corner to the maximum corner: every ancestor's box changes
        p = corner_triangle(sd)
        t = cur[p]
        v = inside(t - t.min(0) + hi - (t.max(0) - t.min(0)))
        return np.array([p], np.int32), v[None], None
    if kind == "carry_back":
        p = corner_triangle(sd)
        return np.array([p], np.int32), orig[p][None].copy(), None
    raise KeyError(kind)


# ---- the geometry at which box code goes wrong (tests/test_gpu_refit_tables.py) ----------------------------------------------------------
EXTREME_KINDS = ("faces", "corners", "point_and_line", "signed_zeros", "tiny_edges", "thrice")


def zero_axis(lo, hi):
    """The first axis whose range holds 0 in its interior, or None."""
    for k in range(3):
        if lo[k] < 0 < hi[k]:
            return k
    return None


def extreme_edit(sd, vertices, kind, lo, hi, seed=0):
    """(ids, vertices, None) of an edit that puts triangles where box code goes wrong; lo, hi: the box of the scene's grid (every vertex
    stays inside it).  Needs 8 movable triangles (6 for "faces", 2 for "point_and_line", 1 otherwise); "signed_zeros" and the subnormal
    edge of "tiny_edges" need an axis with 0 inside (zero_axis)."""
    rng = np.random.default_rng(seed)
    cur = np.asarray(vertices, np.float32).reshape(-1, 3, 3)
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    ids = movable(sd)
    mid = ((lo.astype(np.float64) + hi) / 2).astype(np.float32)
    if kind == "faces":                                      # one triangle flat on each of the six faces of the grid's box
        pick = ids[np.linspace(0, len(ids) - 1, 6).astype(int)]
        v = np.clip(cur[pick], lo, hi).astype(np.float32)
        for j in range(6):
            v[j, :, j >> 1] = (lo, hi)[j & 1][j >> 1]
        return pick, v, None
    if kind == "corners":                                    # a point triangle on each of the eight corners
        pick = ids[np.linspace(0, len(ids) - 1, 8).astype(int)]
        v = np.zeros((8, 3, 3), np.float32)
        for j in range(8):
            v[j, :] = [(lo, hi)[(j >> k) & 1][k] for k in range(3)]
        return pick, v, None
    if kind == "point_and_line":                             # zero-extent boxes in the interior: only the margin keeps them open
        pick = ids[[0, len(ids) - 1]]
        a = (lo + (hi - lo) * np.float32(0.3)).astype(np.float32)
        b = (lo + (hi - lo) * np.float32(0.6)).astype(np.float32)
        b[1:] = a[1:]                                        # the line runs along x
        return pick, np.array([[a, a, a], [a, a, b]], np.float32), None
    if kind == "signed_zeros":                               # -0 and +0 mixed on an axis whose range holds 0
        k = zero_axis(lo, hi)
        pick = ids[[0, len(ids) - 1]]
        v = np.clip(cur[pick], lo, hi).astype(np.float32)
        v[0, :, k] = (-0.0, 0.0, 0.0)
        v[1, :, k] = (0.0, -0.0, -0.0)
        return pick, v, None
    if kind == "tiny_edges":
        pick = ids[[len(ids) // 3]]
        t = mid.copy()
        v = [np.stack([t, np.nextafter(t, hi), t + (hi - lo) * np.float32(0.1)])]      # v1 = nextafter(v0)
        k = zero_axis(lo, hi)
        if k is not None and len(ids) > 1:                   # v1 - v0 is subnormal
            pick = np.append(pick, ids[(len(ids) // 3 + 1) % len(ids)]).astype(np.int32)
            a, b, c = mid.copy(), mid.copy(), (mid + (hi - lo) * np.float32(0.05)).astype(np.float32)
            a[k], b[k] = 0.0, 1e-40
            v.append(np.stack([a, b, c]))
        return pick.astype(np.int32), np.stack(v).astype(np.float32), None
    if kind == "thrice":                                     # every movable id three times in one call: the last record wins
        ext = (hi - lo).astype(np.float32)
        v = [np.clip(cur[ids] + rng.uniform(-0.05, 0.05, (len(ids), 3, 3)) * ext, lo, hi).astype(np.float32) for _ in range(3)]
        return np.concatenate([ids, ids[::-1], ids]).astype(np.int32), np.concatenate([v[0], v[1][::-1], v[2]]), None
    raise KeyError(kind)


def soup_scene(count, seed=7):
    """`count` random triangles in [-1, 1]^3 with one diffuse material and no light: the refit's tables at the smallest trees (2 and 3
    triangles: the root's children are leaves) and around one block of 256 threads."""
    from restir_amd import scenes
    from restir_amd.ctypes_structs import LAMBERTIAN, make_materials
    rng = np.random.default_rng(seed + count)
    centre = rng.uniform(-0.8, 0.8, (count, 1, 3))
    soup = scenes.TriangleSoup()
    soup.add_flat((centre + rng.uniform(-0.2, 0.2, (count, 3, 3))).astype(np.float32), 0)
    mats = make_materials([dict(type=LAMBERTIAN, baseColor=(0.6, 0.6, 0.6))])
    return scenes.SceneData("soup%d" % count, soup, mats, dict(position=(0.0, 0.0, 3.5), rotation=(-90.0, 0.0, 0.0), fov_y=19.5, focal_dist=1.0))


def rebuilt_oracle_scene(old, vertices, normals, boxes):
    """The oracle scene of the edited geometry: the old tables and threaded orders, the refitted boxes."""
    new = ob.Scene(vertices, normals, old.texcoords, old.material_ids, old.materials,
                   prebuilt=(old.light_prim_ids, old.light_radiance, old.light_power, old.light_prob, old.light_fail, old.sum_power,
                             np.ascontiguousarray(boxes, np.float32), old.nodes),
                   textures=old.textures, env_map_tex=old.env_map_tex)
    new.uid = old.uid                                       # an edited rs_scene stays the same scene
    if old.sample_sequence is not None:
        new.sample_sequence, new.sample_count = old.sample_sequence, old.sample_count
        new.c.sampleSequence = new.sample_sequence.ctypes.data
    return new


def edited_oracle_scene(capi, old, ids, v, n=None):
    vertices, normals = apply_triangles(old.vertices, old.normals, ids, v, n)
    return rebuilt_oracle_scene(old, vertices, normals, capi.refit_boxes(vertices, old.nodes[0]))


class OracleSide(_OracleSide):
    def __init__(self, capi, sd, W, H, **kw):
        super().__init__(sd, W, H, **kw)
        self.capi = capi

    def set_triangles(self, ids, v, n=None):
        self.r.scene = edited_oracle_scene(self.capi, self.r.scene, ids, v, n)


class HipSide(_HipSide):
    def set_triangles(self, ids, v, n=None):
        self.r.scene.set_triangles(ids, v, n)


def probe_rays(sd, places, count, seed):
    """(count, 6) rays (origin, unit direction): random ones inside the scene, axis-aligned and near-zero-component ones (the reference's
    special cases), and rays aimed at `places` ((k, 3) points: where edited triangles were and are)."""
    rng = np.random.default_rng(seed)
    lo, hi = root_box(sd.vertices)
    o = rng.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo), (count, 3)).astype(np.float32)
    d = rng.normal(size=(count, 3)).astype(np.float32)
    k = count // 16
    d[:k] = 0; d[np.arange(k), rng.integers(0, 3, k)] = rng.choice([-1.0, 1.0], k)
    d[k:2 * k, 0] = rng.uniform(-1e-6, 1e-6, k)
    d[2 * k:3 * k, 1] = 0.0
    places = np.asarray(places, np.float32).reshape(-1, 3)
    if len(places):
        aim = places[rng.integers(0, len(places), count // 4)] + rng.normal(size=(count // 4, 3)).astype(np.float32) * 0.01 * (hi - lo)
        d[3 * k:3 * k + count // 4] = aim - o[3 * k:3 * k + count // 4]
        o[:k // 2] = places[rng.integers(0, len(places), k // 2)]          # axis-aligned rays that start at the places
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([o, d], 1), np.float32)


def probe_segments(sd, places, count, seed):
    """(count, 6) segments: random pairs of points inside the scene, axis-aligned ones, and ones that end at or pass `places`."""
    rng = np.random.default_rng(seed)
    lo, hi = root_box(sd.vertices)
    a = rng.uniform(lo, hi, (count, 3)).astype(np.float32)
    b = rng.uniform(lo, hi, (count, 3)).astype(np.float32)
    k = count // 8
    b[:k] = a[:k]; b[np.arange(k), rng.integers(0, 3, k)] += rng.choice([-1.0, 1.0], k).astype(np.float32) * (hi - lo).max()
    places = np.asarray(places, np.float32).reshape(-1, 3)
    if len(places):
        t = places[rng.integers(0, len(places), 2 * k)]
        b[k:2 * k] = t[:k]
        b[2 * k:3 * k] = a[2 * k:3 * k] + (t[k:] - a[2 * k:3 * k]) * np.float32(1.5)
    return np.ascontiguousarray(np.concatenate([a, b], 1), np.float32)
