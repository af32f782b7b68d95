"""Helpers of tests/test_emitter_edits_cases.py, tests/test_gpu_emitter_edits.py and tests/test_gpu_emitter_tables.py: edits that move
emitters (rs_scene_set_geometry) driven through the oracle and the library alike.  The oracle has no edit of its own, and the arbiter is
never the scene under test: its side of an edit is a fresh oracle.binding.Scene made from the edited vertices and normals, the old
threaded orders, the boxes of capi.refit_boxes (rs_refit_boxes, host only) and light tables rebuilt by the oracle's own functions --
ob.light_table's powers of the new vertices, the old environment entry appended, then ob.alias_build."""
import functools

import numpy as np

from oracle import binding as ob
from restir_amd.ctypes_structs import LIGHT
from tests.common import get_scene
from tests.geometry_edits import HipSide as _HipSide, OracleSide as _OracleSide, apply_triangles, geometry_edit, movable, root_box
from tests.test_geometry_refit_host import SPONZA_SCALE

# one lamp of two emissive triangles (the emissive tree at its smallest); one emissive triangle (root = leaf); many lamps; 1228 emitters
# (more than 1024: the RIS loop reads the light table from global memory); an environment map behind the lamps
SCENES = {"cornell": "cornell", "single": "cornell", "many": "sponza:%g" % SPONZA_SCALE, "bistro": "bistro:0.12", "env": "cornell_textured"}
# every kind is made on the vertices the kinds before it left, in this order
EDIT_KINDS = ("one", "all", "mixed", "repeated", "carry_min", "carry_max", "carry_back", "scale_up", "scale_down", "flip", "collapse",
              "restore", "collapse_all", "restore_all")
CHANGES_AREA = ("all", "scale_up", "scale_down", "collapse", "restore", "collapse_all", "restore_all")
NEEDS_ENV = ("collapse_all", "restore_all")              # without an environment map the sampler would be left without power: refused


@functools.lru_cache(maxsize=None)
def scene_data(name):
    sd = get_scene(SCENES[name])
    if name == "single":                                 # the lamp's second triangle becomes part of the ceiling
        e = emitters(sd)
        ceiling = sd.material_ids[movable(sd)[0]]
        sd.material_ids = sd.material_ids.copy()
        sd.material_ids[e[1:]] = ceiling
    return sd


def emitters(sd):
    return np.nonzero(sd.materials["type"][sd.material_ids] == LIGHT)[0].astype(np.int32)


def kinds_for(name):
    """The kinds the scene takes: without an environment map the sampler must keep some power, so not every emitter may collapse (with
    a single emitter none may); the refusal itself is a case of tests/test_gpu_emitter_edits.py."""
    sd = scene_data(name)
    env = sd.env_map_tex >= 0
    refused = () if env else NEEDS_ENV + (("collapse", "restore") if len(emitters(sd)) == 1 else ())
    return [k for k in EDIT_KINDS if k not in refused]


def lamp_of(sd, p):
    """The emissive triangles of the lamp `p` belongs to: p and the emissive neighbours in the primitive order that share an edge with it."""
    v = sd.vertices.reshape(-1, 3, 3)
    e = set(emitters(sd).tolist())
    out = [p]
    for q in (p - 1, p + 1):
        if q in e and sum(any(np.array_equal(a, b) for b in v[q]) for a in v[p]) >= 2:
            out.append(q)
    return np.array(sorted(out), np.int32)


def emitter_edit(sd, vertices, kind, seed=0):
    """(ids, vertices, normals or None) of the edit `kind`, given the scene's current `vertices`; every vertex stays inside the root box
    of sd.vertices (the box the scene was created with)."""
    rng = np.random.default_rng(seed)
    cur = np.asarray(vertices, np.float32).reshape(-1, 3, 3)
    orig = sd.vertices.reshape(-1, 3, 3)
    lo, hi = root_box(orig)
    ext = (hi - lo).astype(np.float32)
    e = emitters(sd)
    lamp = lamp_of(sd, int(e[len(e) // 2]))
    other = lamp_of(sd, int(e[0]))

    def inside(v):
        return np.clip(v, lo, hi).astype(np.float32)

    def about_centre(v, factor):
        c = v.reshape(-1, 3).mean(0).astype(np.float32)
        return inside(c + (v - c) * np.float32(factor))
    if kind == "one":                                    # one lamp translated
        return lamp, inside(cur[lamp] + ext * np.float32(0.09) * np.array([1, -1, 0.5], np.float32)), None
    if kind == "all":                                    # all lamps jittered
        return e, inside(cur[e] + rng.uniform(-0.02, 0.02, (len(e), 3, 3)) * ext), None
    if kind == "mixed":                                  # a lamp and triangles that are no emitters in one call
        ids, v, n = geometry_edit(sd, cur, "one", seed)
        lv = inside(cur[lamp] - ext * np.float32(0.05) * np.array([0.5, 1, -1], np.float32))
        n2 = rng.normal(size=(len(lamp) + 1, 3, 3)); n2 /= np.linalg.norm(n2, axis=2, keepdims=True)
        return np.concatenate([lamp[:1], ids, lamp[1:]]).astype(np.int32), np.concatenate([lv[:1], v, lv[1:]]), n2.astype(np.float32)
    if kind == "repeated":                               # an emitter twice, another triangle in between: the last record wins
        a, b = int(other[0]), int(movable(sd)[-2])
        first = inside(cur[a] + ext * np.float32(0.2))
        last = inside(cur[a] - ext * np.float32(0.04) * np.array([1, 1, 0], np.float32))
        return np.array([a, b, a], np.int32), np.stack([first, inside(cur[b] * np.float32(0.95) + np.float32(0.05) * (lo + hi) / 2), last]), None
    if kind in ("carry_min", "carry_max"):               # a lamp into a corner of the root box: far outside the old emissive root box
        t = cur[lamp]
        size = t.reshape(-1, 3).max(0) - t.reshape(-1, 3).min(0)
        to = lo if kind == "carry_min" else hi - size
        return lamp, inside(t - t.reshape(-1, 3).min(0) + to), None
    if kind == "carry_back":
        return lamp, orig[lamp].copy(), None
    if kind == "scale_up":
        return lamp, about_centre(cur[lamp], 4.0), None
    if kind == "scale_down":                             # (a quarter of the original: the lamp was scaled by 4 before)
        return lamp, about_centre(orig[lamp], 0.25), None
    if kind == "flip":                                   # the winding reversed: the normal of the light record points the other way
        return lamp, np.ascontiguousarray(cur[lamp][:, [0, 2, 1]]), None
    if kind == "collapse":                               # a point: area and power 0, normalize(0) in the light record
        c = cur[lamp[:1]].reshape(-1, 3).mean(0).astype(np.float32)
        return lamp[:1], np.broadcast_to(c, (1, 3, 3)).copy(), None
    if kind == "restore":
        return lamp[:1], orig[lamp[:1]].copy(), None
    if kind == "collapse_all":                           # every emitter in one point: no power but the environment map's, no emissive extent
        c = ((lo + hi) / 2).astype(np.float32)
        return e, np.broadcast_to(c, (len(e), 3, 3)).copy(), None
    if kind == "restore_all":
        return e, orig[e].copy(), None
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def edits_up_to(name, kind):
    """The edits of kinds_for(name) up to and including `kind`, each made on the vertices the ones before it left; the places (points) the
    last one moved triangles from and to; the vertices and normals after all of them."""
    sd = scene_data(name)
    v, n = sd.vertices.reshape(-1, 3, 3).copy(), sd.normals.reshape(-1, 3, 3).copy()
    out, places = [], None
    kinds = kinds_for(name)
    for k in kinds[:kinds.index(kind) + 1]:
        ids, ev, en = emitter_edit(sd, v, k, seed=13)
        places = np.concatenate([v[ids].mean(1), np.asarray(ev).reshape(-1, 3, 3).mean(1)])
        v, n = apply_triangles(v, n, ids, ev, en)
        out.append((ids, ev, en))
    return out, places, v, n


def emissive_root_box(sd, vertices):
    return root_box(np.asarray(vertices, np.float32).reshape(-1, 3, 3)[emitters(sd)])


def light_tables(old, vertices):
    """(power, prob, fail, sum) of the oracle's own functions on the new vertices; the environment entry keeps its power."""
    prim_ids, radiance, power = ob.light_table(vertices, old.material_ids, old.materials)
    assert np.array_equal(prim_ids, old.light_prim_ids) and np.array_equal(radiance, old.light_radiance)      # the set of emitters is the same
    if old.env_map_tex >= 0:
        power = np.concatenate([power, old.light_power[-1:]])
    prob, fail, total = ob.alias_build(power)
    return power, prob, fail, total


def rebuilt_oracle_scene(old, vertices, normals, boxes):
    """The oracle scene of the edited geometry: the old threaded orders, the refitted boxes, the light tables built anew."""
    power, prob, fail, total = light_tables(old, vertices)
    new = ob.Scene(vertices, normals, old.texcoords, old.material_ids, old.materials,
                   prebuilt=(old.light_prim_ids, old.light_radiance, power, prob, fail, total, np.ascontiguousarray(boxes, np.float32), old.nodes),
                   textures=old.textures, env_map_tex=old.env_map_tex)
    new.env_prob, new.env_fail = old.env_prob, old.env_fail          # (the constructor builds them only without `prebuilt`)
    new.c.envMapSamplerLength = len(new.env_prob)
    new.c.envMapProb = new.env_prob.ctypes.data
    new.c.envMapFailId = new.env_fail.ctypes.data
    new.uid = old.uid                                       # an edited rs_scene stays the same scene
    if old.sample_sequence is not None:
        new.sample_sequence, new.sample_count = old.sample_sequence, old.sample_count
        new.c.sampleSequence = new.sample_sequence.ctypes.data
    return new


def edited_oracle_scene(capi, old, ids, v, n=None):
    vertices, normals = apply_triangles(old.vertices, old.normals, ids, v, n)
    return rebuilt_oracle_scene(old, vertices, normals, capi.refit_boxes(vertices, old.nodes[0]))


class OracleSide(_OracleSide):
    def set_geometry(self, ids, v, n=None):
        self.r.scene = edited_oracle_scene(self.capi, self.r.scene, ids, v, n)

    set_triangles = set_geometry                            # (the same scene when no emitter is named; this one keeps an environment sampler)


class HipSide(_HipSide):
    def set_geometry(self, ids, v, n=None):
        self.r.scene.set_geometry(ids, v, n)
