"""The refusals of the deformers' six entry points -- rs_scene_define_parts, rs_scene_set_part_transforms, rs_scene_download_part_rest,
rs_scene_define_skin, rs_scene_set_bone_transforms, rs_scene_download_skin -- by return code AND by the exact text rs_last_error gives:
every refusal tests/test_gpu_part_transforms.py test_refusals_leave_scene_unchanged and tests/test_gpu_skinning.py
test_refusals_leave_scene_definition_and_palette_unchanged provoke (those tests hold the scene unchanged; this one holds the words), the
two downloads on a scene without a definition, and per definition one input with two faults at once, to pin which check comes first.
The expected texts are written out here, as the library had them when parts and skins were added.  Cornell box, no frame rendered."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import part_transforms as pt
from tests import skinning as sk
from tests.common import hip_scene
from tests.emitter_edits import scene_data
from tests.geometry_edits import root_box

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 10001, 10002
NAME, KEY = "cornell", "box_lamp"

OUTSIDE = ("a vertex outside the root box the scene was created with (the grid of its shadow-ray tree lies over that box); "
           "build a new scene")
NOT_FINITE = "a vertex or normal that is not finite"
NULL_ARRAYS = "count < 0 or null arrays"
PAIR = "rest vertices without rest normals, or the reverse"
ID_RANGE = "a primitive id out of range"
TWICE = "a primitive listed twice"
REST_VALUE = "a rest value that is not finite"
NO_PARTS = "the scene has no parts (rs_scene_define_parts)"
NO_SKIN = "the scene has no skin (rs_scene_define_skin)"
CAPTURED = "the library stream is being captured into a graph"


def outcome(hip, call):
    """(return code, rs_last_error's text) of a call made through capi.check; (0, "") when it was accepted."""
    try:
        call()
    except hip.RestirHipError as e:
        m = re.fullmatch(r"librestir_hip error (-?\d+): (.*)", str(e), re.S)
        assert m, str(e)
        return int(m.group(1)), m.group(2)
    return 0, ""


def changed(a, where, value):
    a = a.copy()
    a[where] = value
    return a


def part_cases(hip, s, bare, sd):
    """(tag, entry point, code, text after the entry point's name, call): tests/test_gpu_part_transforms.py's refusals, on its scene."""
    L, ptr = hip.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
    parts = pt.parts_of(NAME)[0]
    lo, hi = root_box(sd.vertices)
    out_of_box = pt.translation((-(hi[0] - lo[0]) * 0.45, 0.0, 0.0))
    singular = pt.from_rows(np.diag([1.0, 0.0, 1.0, 1.0]))
    nan = pt.identity(); nan[3, 1] = np.nan
    one, ident = np.array([1], np.int32), pt.identity()
    v12, n12 = pt.rest_of(sd, parts[1])
    bad_rest = v12.copy(); bad_rest[3, 1, 2] = np.inf
    first2, ids2 = np.array([0, 2], np.int32), np.array([10, 11], np.int32)
    beyond = len(sd.material_ids)
    v3, n3 = pt.rest_of(sd, [10, 11, 12])

    def define_raw(num, first, ids, v=None, n=None):
        hip.check(L.rs_scene_define_parts(s.handle, num, None if first is None else ptr(first), None if ids is None else ptr(ids),
                                          None if v is None else ptr(v), None if n is None else ptr(n)))
    T, D, R = "rs_scene_set_part_transforms", "rs_scene_define_parts", "rs_scene_download_part_rest"
    return [
        ("a vertex leaves the root box", T, INVALID, OUTSIDE, lambda: s.set_part_transforms([1], [out_of_box])),
        ("a singular matrix", T, INVALID, NOT_FINITE, lambda: s.set_part_transforms([0, 1], [ident, singular])),
        ("a NaN entry", T, INVALID, NOT_FINITE, lambda: s.set_part_transforms([1], [nan])),
        ("part id beyond", T, INVALID, "a part id out of range", lambda: s.set_part_transforms([len(parts)], [ident])),
        ("part id below", T, INVALID, "a part id out of range", lambda: s.set_part_transforms([-1], [ident])),
        ("null part ids", T, INVALID, NULL_ARRAYS, lambda: hip.check(L.rs_scene_set_part_transforms(s.handle, 1, None, ptr(ident)))),
        ("null matrices", T, INVALID, NULL_ARRAYS, lambda: hip.check(L.rs_scene_set_part_transforms(s.handle, 1, ptr(one), None))),
        ("negative count", T, INVALID, NULL_ARRAYS, lambda: hip.check(L.rs_scene_set_part_transforms(s.handle, -1, ptr(one), ptr(ident)))),
        ("null scene", T, INVALID, "null scene", lambda: hip.check(L.rs_scene_set_part_transforms(None, 1, ptr(one), ptr(ident)))),
        ("no parts", T, INVALID, NO_PARTS, lambda: bare.set_part_transforms([0], [ident])),
        ("define: a primitive twice in one part", D, INVALID, TWICE, lambda: s.define_parts([[10, 11, 10]])),
        ("define: a primitive in two parts", D, INVALID, TWICE, lambda: s.define_parts([[10, 11], [34], [11]])),
        ("define: an id beyond", D, INVALID, ID_RANGE, lambda: s.define_parts([[beyond]])),
        ("define: an id below", D, INVALID, ID_RANGE, lambda: s.define_parts([[-1]])),
        ("define: first offset not 0", D, INVALID, "the first offset is not 0", lambda: define_raw(1, np.array([1, 2], np.int32), ids2)),
        ("define: offsets that decrease", D, INVALID, "offsets that decrease", lambda: define_raw(2, np.array([0, 2, 1], np.int32), ids2)),
        ("define: null offsets", D, INVALID, "numParts < 0 or null offsets", lambda: define_raw(1, None, ids2)),
        ("define: null ids", D, INVALID, "null primitive ids", lambda: define_raw(1, first2, None)),
        ("define: negative count", D, INVALID, "numParts < 0 or null offsets", lambda: define_raw(-1, first2, ids2)),
        ("define: rest vertices alone", D, INVALID, PAIR, lambda: define_raw(1, first2, ids2, np.ascontiguousarray(v12[:2]), None)),
        ("define: rest normals alone", D, INVALID, PAIR, lambda: define_raw(1, first2, ids2, None, np.ascontiguousarray(n12[:2]))),
        ("define: a rest value that is not finite", D, INVALID, REST_VALUE, lambda: s.define_parts([parts[1]], bad_rest, n12)),
        ("define: null scene", D, INVALID, "null scene", lambda: hip.check(L.rs_scene_define_parts(None, 1, ptr(first2), ptr(ids2), None, None))),
        # two faults at once: the ids are scanned before the rest values
        ("define: an id beyond, then a rest value that is not finite", D, INVALID, ID_RANGE,
         lambda: s.define_parts([[10, beyond, 12]], changed(v3, (2, 1, 0), np.inf), n3)),
        ("download: no parts", R, INVALID, NO_PARTS, bare.part_rest),
        ("download: null scene", R, INVALID, "null scene", lambda: hip.check(L.rs_scene_download_part_rest(None, None, None, None))),
    ], [
        ("captured", T, UNSUPPORTED, CAPTURED, lambda: s.set_part_transforms([1], [pt.part_matrix(NAME, 1)])),
        ("define: captured", D, UNSUPPORTED, CAPTURED, lambda: s.define_parts([parts[1]])),
        ("download: captured", R, UNSUPPORTED, CAPTURED, s.part_rest),
    ]


def skin_cases(hip, s, bare, sd):
    """The same of tests/test_gpu_skinning.py's refusals, on its scene."""
    L, ptr = hip.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
    skin = sk.skin_of(NAME, KEY)
    lo, hi = root_box(sd.vertices)
    out_of_box = pt.translation((-(hi[0] - lo[0]) * 0.45, 0.0, 0.0))
    singular = pt.from_rows(np.diag([1.0, 0.0, 1.0, 1.0]))
    nan = pt.identity(); nan[3, 1] = np.nan
    good = sk.bone_matrix(NAME, KEY, 1, 5)
    one, ident = np.array([1], np.int32), pt.identity()
    ids, bid, wts, rv, rn = skin.ids, skin.bone_ids, skin.weights, skin.rest_vertices, skin.rest_normals
    nl, beyond = len(ids), len(sd.material_ids)

    def define_raw(bones, listed, prim=ids, v=None, n=None, b=bid, w=wts, scene=None):
        hip.check(L.rs_scene_define_skin(s.handle if scene is None else scene, bones, listed, None if prim is None else ptr(prim),
                                         None if v is None else ptr(v), None if n is None else ptr(n), None if b is None else ptr(b),
                                         None if w is None else ptr(w)))
    T, D, R = "rs_scene_set_bone_transforms", "rs_scene_define_skin", "rs_scene_download_skin"
    BONES, LISTED = "numBones < 0 or above RS_SKIN_MAX_BONES", "numListed < 0, or triangles without a bone"
    NULLS, WEIGHT = "null primitive ids, bone ids or weights", "a weight that is not finite"
    return [
        ("a vertex leaves the root box", T, INVALID, OUTSIDE, lambda: s.set_bone_transforms([1, 0], [good, out_of_box])),
        ("a singular matrix", T, INVALID, NOT_FINITE, lambda: s.set_bone_transforms([1, 2], [good, singular])),
        ("a NaN entry", T, INVALID, NOT_FINITE, lambda: s.set_bone_transforms([0, 1], [nan, good])),
        ("bone id beyond", T, INVALID, "a bone id out of range", lambda: s.set_bone_transforms([1, skin.num_bones], [good, ident])),
        ("bone id below", T, INVALID, "a bone id out of range", lambda: s.set_bone_transforms([1, -1], [good, ident])),
        ("null bone ids", T, INVALID, NULL_ARRAYS, lambda: hip.check(L.rs_scene_set_bone_transforms(s.handle, 1, None, ptr(good)))),
        ("null matrices", T, INVALID, NULL_ARRAYS, lambda: hip.check(L.rs_scene_set_bone_transforms(s.handle, 1, ptr(one), None))),
        ("negative count", T, INVALID, NULL_ARRAYS, lambda: hip.check(L.rs_scene_set_bone_transforms(s.handle, -1, ptr(one), ptr(good)))),
        ("null scene", T, INVALID, "null scene", lambda: hip.check(L.rs_scene_set_bone_transforms(None, 1, ptr(one), ptr(good)))),
        ("no skin", T, INVALID, NO_SKIN, lambda: bare.set_bone_transforms([0], [ident])),
        ("define: 257 bones", D, INVALID, BONES, lambda: define_raw(257, nl)),
        ("define: negative bones", D, INVALID, BONES, lambda: define_raw(-1, nl)),
        ("define: negative count", D, INVALID, LISTED, lambda: define_raw(3, -1)),
        ("define: triangles without a bone", D, INVALID, LISTED, lambda: define_raw(0, nl)),
        ("define: a primitive twice", D, INVALID, TWICE, lambda: define_raw(3, nl, changed(ids, 3, ids[0]))),
        ("define: an id beyond", D, INVALID, ID_RANGE, lambda: define_raw(3, nl, changed(ids, 2, beyond))),
        ("define: an id below", D, INVALID, ID_RANGE, lambda: define_raw(3, nl, changed(ids, 2, -1))),
        ("define: null ids", D, INVALID, NULLS, lambda: define_raw(3, nl, None)),
        ("define: null bone ids", D, INVALID, NULLS, lambda: define_raw(3, nl, b=None)),
        ("define: null weights", D, INVALID, NULLS, lambda: define_raw(3, nl, w=None)),
        ("define: rest vertices alone", D, INVALID, PAIR, lambda: define_raw(3, nl, v=rv)),
        ("define: rest normals alone", D, INVALID, PAIR, lambda: define_raw(3, nl, n=rn)),
        ("define: a rest vertex that is not finite", D, INVALID, REST_VALUE, lambda: define_raw(3, nl, v=changed(rv, (3, 1, 2), np.inf), n=rn)),
        ("define: a rest normal that is not finite", D, INVALID, REST_VALUE, lambda: define_raw(3, nl, v=rv, n=changed(rn, (0, 0, 0), np.nan))),
        ("define: a weight that is NaN", D, INVALID, WEIGHT, lambda: define_raw(3, nl, w=changed(wts, (2, 1, 0), np.nan))),
        ("define: a weight that is infinite", D, INVALID, WEIGHT, lambda: define_raw(3, nl, w=changed(wts, (2, 1, 0), np.inf))),
        ("define: a negative weight", D, INVALID, "a negative weight", lambda: define_raw(3, nl, w=changed(wts, (2, 1, 0), -0.25))),
        ("define: a corner without weight", D, INVALID, "a corner whose four weights are all 0", lambda: define_raw(3, nl, w=changed(wts, (5, 2), 0.0))),
        ("define: a bone id beyond", D, INVALID, "a bone id out of range", lambda: define_raw(3, nl, b=changed(bid, (4, 0, 3), 3))),
        ("define: a bone id below, at weight 0", D, INVALID, "a bone id out of range", lambda: define_raw(3, nl, b=changed(bid, (nl - 1, 0, 0), -1))),
        ("define: null scene", D, INVALID, "null scene", lambda: define_raw(3, nl, scene=C.c_void_p())),
        # two faults at once: the ids are scanned before the rest values
        ("define: an id beyond, then a rest value that is not finite", D, INVALID, ID_RANGE,
         lambda: define_raw(3, nl, changed(ids, 2, beyond), v=changed(rv, (3, 1, 2), np.inf), n=rn)),
        ("download: no skin", R, INVALID, NO_SKIN, bare.download_skin),
        ("download: null scene", R, INVALID, "null scene", lambda: hip.check(L.rs_scene_download_skin(None, None, None, None, None, None))),
    ], [
        ("captured", T, UNSUPPORTED, CAPTURED, lambda: s.set_bone_transforms([1], [good])),
        ("define: captured", D, UNSUPPORTED, CAPTURED, lambda: skin.define(s)),
        ("download: captured", R, UNSUPPORTED, CAPTURED, s.download_skin),
    ]


@pytest.mark.parametrize("kind", ["parts", "skin"])
def test_refusal_codes_and_texts(hip, kind):
    import torch
    hip.set_sync(True)
    sd = scene_data(NAME)
    s, bare = hip_scene(hip, sd), hip_scene(hip, sd)
    if kind == "parts":
        s.define_parts(pt.parts_of(NAME)[0])
        plain, captured = part_cases(hip, s, bare, sd)
    else:
        sk.skin_of(NAME, KEY).define(s)
        s.set_bone_transforms(*sk.pose(NAME, KEY, 0))    # the pose the refusals of tests/test_gpu_skinning.py are made at
        plain, captured = skin_cases(hip, s, bare, sd)

    def expect(cases):
        for tag, entry, code, text, call in cases:
            got = outcome(hip, call)
            print(kind, tag, got)
            assert got == (code, entry + ": " + text), (kind, tag)
    expect(plain)

    # while the library stream is being captured into a graph, as the two refusal tests do it
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
            expect(captured)
        finally:
            assert rt.hipStreamEndCapture(stream.cuda_stream, C.byref(graph)) == 0
            if graph:
                rt.hipGraphDestroy(graph)
    finally:
        hip.set_stream(None)
