"""Helpers of tests/test_motion_vectors_cases.py and tests/test_gpu_motion_vectors.py: the G-buffer's motion plane of a scene that tracks
motion (rs_scene_set_motion_tracking, rs_scene_advance_motion), stated without the library, and frame loops that drive the oracle and
the library through the same edits and advances.

The oracle has no previous pose: its renderGBuffer asks where the hit's world point was on last frame's screen.  Its G-buffer is a host
image, so "the oracle" of these tests renders, overwrites the motion plane with object_motion_plane() and then runs the consumers of
the plane (ReSTIRDirect, ReSTIRIndirect, SpatioTemporalFilter) on it."""
import ctypes as C
import functools

import numpy as np

from oracle import binding as ob
from tests import emitter_edits as ee
from tests import geometry_edits as ge
from tests.common import get_scene, hip_scene, next_looper, oracle_scene
from tests.test_geometry_refit_host import SPONZA_SCALE

SCENES = {"cornell": "cornell", "sponza": "sponza:%g" % SPONZA_SCALE}      # 36 triangles; 2 621 (61 mod 64)
TEXTURED = "cornell_textured"        # the Cornell box with texture maps and an environment map: the textured instantiations of the kernels
W, H = 61, 47                        # partial tiles on both axes: 2 867 pixels
DEPTH = 3
F = np.float32


@functools.lru_cache(maxsize=None)
def scene_data(name):
    return get_scene(SCENES.get(name, name))


# ---- the plane ------------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def center_rays(cam, width, height):
    """The pixel-centre rays of renderGBuffer (the reference's gbuffer.cu:11-23) restated in float32 NumPy, one operation per rounding, in
    the reference's order: (n, 6) origin | direction, row-major pixels."""
    w, h = F(width), F(height)
    aspect = w / h
    tan_fov_y = ob.tanf(F(cam.fov[1]) * F(0.01745329251994329576923690768489))
    px, py = F(1.0) / w, F(1.0) / h
    y, x = np.mgrid[0:height, 0:width]
    x, y = x.reshape(-1).astype(F), y.reshape(-1).astype(F)
    ruvx, ruvy = x * px + px * F(0.5), y * py + py * F(0.5)
    focal = F(cam.focalDist)
    d = np.stack([(F(1.0) - ruvx * F(2.0)) * aspect * tan_fov_y, (F(1.0) - ruvy * F(2.0)) * F(1.0) * tan_fov_y, np.ones_like(x)], 1) * focal
    lens = np.zeros(3, F)
    d = d - lens
    right, up, view, pos = (np.array(list(v), F) for v in (cam.right, cam.up, cam.view, cam.position))
    d = (right[None, :] * d[:, :1] + up[None, :] * d[:, 1:2]) + view[None, :] * d[:, 2:3]
    d = d * (F(1.0) / np.sqrt(_dot(d, d)))[:, None]
    o = (pos + right * lens[0]) + up * lens[1]
    rays = np.empty((len(x), 6), F)
    rays[:, :3], rays[:, 3:] = o, d
    assert rays.dtype == F and d.dtype == F
    return rays


def hit_points(scene, vertices, rays, prim, of_vertices):
    """pv1 * bx + pv2 * by + pv0 * (1 - bx - by) for every ray that hit: the barycentrics of orc_intersect_triangle on the hit primitive's
    current `vertices`, the expression on `of_vertices`.  (n, 3) float32, rows of misses 0."""
    hit = prim >= 0
    n = int(hit.sum())
    out = np.zeros((len(prim), 3), F)
    if n == 0:
        return out
    cur = np.ascontiguousarray(np.asarray(vertices, F).reshape(-1, 9)[prim[hit]])
    flag, bary, dist = np.zeros(n, np.int32), np.zeros(2 * n, F), np.zeros(n, F)
    ob.lib().orc_intersect_triangle(n, np.ascontiguousarray(rays[hit]).reshape(-1), cur.reshape(-1), flag, bary, dist)
    assert flag.all(), "Scene.intersect named a primitive that orc_intersect_triangle misses"
    bx, by = bary[0::2, None], bary[1::2, None]
    pv = np.asarray(of_vertices, F).reshape(-1, 3, 3)[prim[hit]]
    out[hit] = (pv[:, 1] * bx + pv[:, 2] * by) + pv[:, 0] * (F(1.0) - bx - by)
    return out


def object_motion_plane(scene, prev_vertices, cam, last_cam, width, height, details=False):
    """The motion plane GBuffer::render writes for `scene` (an oracle.binding.Scene) seen from `cam` when the previous pose of its triangles
    is `prev_vertices` and the previous camera `last_cam`: for a hit, the raster coordinate of the hit's barycentric point on the previous
    pose under last_cam (y * width + x inside the image, -1 outside); 0 for a miss.  details: also the hit primitives, Scene.intersect's
    positions and the same expression on the current vertices."""
    rays = center_rays(cam, width, height)
    prim, _, pos, _, _ = scene.intersect(rays)
    prev = hit_points(scene, scene.vertices, rays, prim, prev_vertices)
    xy = np.zeros(2 * len(prim), np.int32)
    ob.lib().orc_camera_raster_coord(C.byref(last_cam), len(prim), np.ascontiguousarray(prev).reshape(-1), xy)
    lx, ly = xy[0::2], xy[1::2]
    inside = (lx >= 0) & (lx < width) & (ly >= 0) & (ly < height)
    plane = np.where(prim >= 0, np.where(inside, ly * width + lx, -1), 0).astype(np.int32)
    if details:
        return plane, prim, pos, hit_points(scene, scene.vertices, rays, prim, scene.vertices)
    return plane


# ---- edits -------------------------------------------------------------------------------------------------------------------------------------
CAMERA_KINDS = ("behind_last_camera", "at_last_camera")
SLIDE = "slide_centre"
SLIDE_COUNT = {"cornell": 4, "sponza": 48, TEXTURED: 4}               # triangles of the slide: enough for 50 pixels of the 2 867 (test_motion_vectors_cases.py)


def centre_triangles(sd, count, cam_position=None):
    """The `count` movable triangles nearest the image centre of the scene as created: those the pixel-centre rays hit, in rings around
    the centre pixel."""
    cam = sd.camera(W, H)
    if cam_position is not None:
        for i in range(3):
            cam.position[i] = float(cam_position[i])
    cam = ob.camera_update(cam)
    scene = oracle_scene(sd)
    prim = scene.intersect(center_rays(cam, W, H))[0].reshape(H, W)
    movable = set(ge.movable(sd).tolist())
    y, x = np.mgrid[0:H, 0:W]
    ring = np.maximum(abs(y - H // 2), abs(x - W // 2)).reshape(-1)
    out = []
    for i in np.argsort(ring, kind="stable"):
        p = int(prim.reshape(-1)[i])
        if p in movable and p not in out:
            out.append(p)
            if len(out) == count:
                break
    return np.array(sorted(out), np.int32)


def slide_edit(sd, vertices, ids):
    """The triangles `ids` slid by a tenth of the scene's extent."""
    cur = np.asarray(vertices, F).reshape(-1, 3, 3)
    lo, hi = ge.root_box(sd.vertices)
    v = np.clip(cur[ids] + (hi - lo).astype(F) * F(0.1) * np.array([1, 0.5, -0.25], F), lo, hi).astype(F)
    return "set_triangles", ids, v, None


def motion_edit(sd, vertices, kind, seed=0):
    """(setter, ids, vertices, normals or None) of the edit `kind` of geometry_edits.EDIT_KINDS ("triangles:<kind>") or of
    emitter_edits.EDIT_KINDS ("emitters:<kind>") on the scene's current `vertices`."""
    if kind.startswith("triangles:"):
        return ("set_triangles",) + tuple(ge.geometry_edit(sd, vertices, kind.split(":")[1], seed))
    if kind.startswith("emitters:"):
        return ("set_geometry",) + tuple(ee.emitter_edit(sd, vertices, kind.split(":")[1], seed))
    raise KeyError(kind)


def camera_case(sd, kind):
    """A triangle whose previous pose lies behind the last camera, or exactly at its position: (camera position, the edit before the first
    frame that puts the triangle there, the edit under test that brings it in front of the camera).  A vertex must stay inside the root box
    the scene was created with, so the camera goes inside it: to the box's centre, or ("at_last_camera") to the origin, which both boxes
    contain and where pv * bx + pv * by + pv * w is exactly the camera's position for every hit."""
    lo, hi = ge.root_box(sd.vertices)
    cam = ob.camera_update(sd.camera(W, H))
    view, up, right = (np.array(list(v), F) for v in (cam.view, cam.up, cam.right))
    ext = (hi - lo).astype(F)
    at = kind == "at_last_camera"
    pos = np.zeros(3, F) if at else ((lo + hi) / F(2)).astype(F)
    assert ((pos >= lo) & (pos <= hi)).all()
    p = ge.movable(sd)[:1]
    size = F(0.08) * ext.max()
    shape = np.stack([-right * size, right * size, up * size]).astype(F)
    was = np.broadcast_to(pos, (3, 3)).astype(F).copy() if at else (pos - view * F(0.2) * ext.min() + shape).astype(F)
    now = np.clip(pos + view * F(0.3) * abs(float(np.dot(view, ext))) + shape, lo, hi).astype(F)
    return pos, ("set_triangles", p, np.clip(was, lo, hi).astype(F)[None], None), ("set_triangles", p, now[None], None)


TEXTURED_KINDS = (SLIDE, "emitters:one")                 # on TEXTURED: a plain edit and one through the ring of versions


def kinds_for(name):
    """Every edit kind the GPU tests run on the scene."""
    emit = [k for k in ee.EDIT_KINDS if k not in ee.NEEDS_ENV]         # (neither scene has an environment map)
    return ["triangles:" + k for k in ge.EDIT_KINDS] + ["emitters:" + k for k in emit] + [SLIDE] + list(CAMERA_KINDS)


@functools.lru_cache(maxsize=None)
def case_edits(name, kind, with_slide=True):
    """(edits before the first frame, the edits of the gap under test): each a tuple (setter, ids, vertices, normals).  The kinds of
    geometry_edits and emitter_edits are made on the vertices the kinds before them left, as in their own tests.  Most of them move a
    triangle or a lamp that covers few pixels of a 61 x 47 image or none (one triangle of 2 621; figures in test_motion_vectors_cases.py),
    so the gap under test holds two edits: first the slide of the SLIDE_COUNT triangles nearest the image centre, then the kind's own edit,
    made on the vertices the slide left.  SLIDE is the slide alone.  with_slide=False: the kind's own edit alone (for those figures)."""
    sd = scene_data(name)
    v, n = sd.vertices.reshape(-1, 3, 3).copy(), sd.normals.reshape(-1, 3, 3).copy()
    before, gap = [], []
    family = kind.split(":")[0]
    cam_position = camera_case(sd, kind)[0] if kind in CAMERA_KINDS else None
    if kind in CAMERA_KINDS:
        before.append(camera_case(sd, kind)[1])
    elif family in ("triangles", "emitters"):
        kinds = list(ge.EDIT_KINDS) if family == "triangles" else [k for k in ee.EDIT_KINDS if k not in ee.NEEDS_ENV]
        for k in kinds[:kinds.index(kind.split(":")[1])]:
            before.append(motion_edit(sd, v, family + ":" + k, seed=11))
            v, n = ge.apply_triangles(v, n, *before[-1][1:])
    if kind in CAMERA_KINDS:
        v, n = ge.apply_triangles(v, n, *before[-1][1:])
    if with_slide or kind == SLIDE:
        gap.append(slide_edit(sd, v, centre_triangles(sd, SLIDE_COUNT[name], cam_position)))
        v, n = ge.apply_triangles(v, n, gap[0][1], gap[0][2], gap[0][3])
    if kind in CAMERA_KINDS:
        gap.append(camera_case(sd, kind)[2])
    elif kind != SLIDE:
        gap.append(motion_edit(sd, v, kind, seed=11))
    return before, gap


# ---- frame loops ---------------------------------------------------------------------------------------------------------------------------------
PIPELINES = ("direct_svgf", "indirect")


class OracleMotion:
    """runCuda on the oracle with a tracked scene: set_triangles / set_geometry as tests/emitter_edits.py makes them, advance() and the
    NumPy bookkeeping of the previous pose."""

    def __init__(self, capi, sd, tracked=True, pipeline="direct_svgf"):
        self.capi, self.sd, self.pipeline = capi, sd, pipeline
        self.scene = oracle_scene(sd)
        self.scene.set_sample_sequence(None)
        self.cam = ob.camera_update(sd.camera(W, H))
        self.gbuf, self.restir, self.svgf = ob.GBuffer(W, H), ob.ReSTIR(W, H), ob.SVGF(W, H)
        self.image = np.zeros((W * H, 3), np.float32)
        self.filtered = None
        self.looper, self.rays = 0, 0
        self.tracked = tracked
        self.prev = np.array(self.scene.vertices, F).reshape(-1, 3, 3).copy()

    def set_tracking(self, on):
        if on and not self.tracked:
            self.prev = np.array(self.scene.vertices, F).reshape(-1, 3, 3).copy()
        self.tracked = on

    def set_geometry(self, ids, v, n=None):
        self.scene = ee.edited_oracle_scene(self.capi, self.scene, ids, v, n)

    set_triangles = set_geometry

    def advance(self):
        if self.tracked:
            self.prev = np.array(self.scene.vertices, F).reshape(-1, 3, 3).copy()

    def set_camera_position(self, pos):
        for i in range(3):
            self.cam.position[i] = float(pos[i])
        ob.camera_update(self.cam)

    def render(self):
        self.gbuf.render(self.scene, self.cam)
        self.camera_only = self.gbuf.motion.copy()
        if self.tracked:
            self.gbuf.motion[:] = object_motion_plane(self.scene, self.prev, self.cam, self.gbuf.c.lastCamera, W, H)

    def frame(self):
        self.render()
        if self.pipeline == "indirect":
            self.image[:] = 0
            self.rays = self.restir.indirect(self.scene, self.cam, self.gbuf, self.image, 0, self.looper, 1, DEPTH)
        else:
            self.rays = self.restir.direct(self.scene, self.cam, self.gbuf, self.image, 0, self.looper, 3)
            self.filtered = self.svgf.filter(self.image, self.gbuf, self.cam)
            self.svgf.next_frame()
        self.looper = next_looper(self.looper, None)
        self.gbuf.update(self.cam)
        return self.state()

    def state(self):
        g = self.gbuf
        f = g.frame_idx ^ 1                                 # the planes rendered last: update() flipped the index
        out = dict(image=self.image.copy(), rays=self.rays, prim_id=g.prim_id[f].copy(), albedo=g.albedo.copy(), normal=g.normal[f].copy(),
                   depth=g.depth[f].copy(), motion=g.motion.copy())
        if self.pipeline == "indirect":
            out["reservoirs"] = self.restir.ind_last.copy()
        else:
            out.update(last=self.restir.last.copy(), temp=self.restir.temp.copy(), filtered=self.filtered.copy())
        return out


class HipMotion:
    """The same loop on the library."""

    def __init__(self, capi, sd, tracked=True, pipeline="direct_svgf", scene=None):
        import torch
        self.torch, self.capi, self.sd, self.pipeline = torch, capi, sd, pipeline
        self.scene = scene or hip_scene(capi, sd)
        self.scene.set_sample_sequence(None)
        if tracked:
            self.scene.set_motion_tracking(True)
        self.cam = capi.camera_update(sd.camera(W, H))
        self.gbuf, self.restir = capi.GBuffer(W, H), capi.ReSTIR(W, H)
        self.svgf = capi.SVGFFilter(W, H, 5) if pipeline == "direct_svgf" else None
        self.image = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
        self.filtered = torch.zeros_like(self.image)
        self.looper, self.rays = 0, 0

    def set_tracking(self, on):
        self.scene.set_motion_tracking(on)

    def set_geometry(self, ids, v, n=None):
        self.scene.set_geometry(ids, v, n)

    def set_triangles(self, ids, v, n=None):
        self.scene.set_triangles(ids, v, n)

    def advance(self):
        self.scene.advance_motion()

    def set_camera_position(self, pos):
        for i in range(3):
            self.cam.position[i] = float(pos[i])
        self.capi.camera_update(self.cam)

    def enqueue(self):
        """One frame without reading anything back."""
        self.gbuf.render(self.scene, self.cam)
        if self.pipeline == "indirect":
            self.image.zero_()
            self.rays = self.restir.indirect(self.scene, self.cam, self.gbuf, self.image.data_ptr(), 0, self.looper, 1, DEPTH)
        else:
            self.restir.direct(self.scene, self.cam, self.gbuf, self.image.data_ptr(), 0, self.looper, 3)
            p = self.svgf.filter(self.image.data_ptr(), self.gbuf, self.cam)
            self.capi.hip_memcpy_d2d_async(self.filtered.data_ptr(), p, W * H * 12)
            self.svgf.next_frame()
        self.looper = next_looper(self.looper, None)
        self.gbuf.update(self.cam)

    def frame(self):
        self.enqueue()
        return self.state()

    def state(self):
        self.capi.synchronize()
        g = self.gbuf.download()
        f = g["frame_idx"] ^ 1
        out = dict(image=self.image.cpu().numpy(), prim_id=g["prim_id"][f], albedo=g["albedo"], normal=g["normal"][f], depth=g["depth"][f],
                   motion=g["motion"])
        if self.pipeline == "indirect":
            out.update(rays=self.rays, reservoirs=self.restir.download_indirect(1))
        else:
            out.update(rays=self.restir.ray_count(), last=self.restir.download(1), temp=self.restir.download(2), filtered=self.filtered.cpu().numpy())
        return out

    def destroy(self):
        if self.svgf is not None:
            self.svgf.destroy()


def apply(side, edit):
    getattr(side, edit[0])(*edit[1:])


WARM_FRAMES = 3


def run_case(side, name, kind, with_slide=True, on_frame=None):
    """WARM_FRAMES frames at rest, then frame, edit, frame, advance, frame with no edit, advance, frame: the states of those four;
    on_frame(i) is called after the i-th of them.  The frames at rest are there for the library's launch sites: overlapped frames take the
    three chain streams in turn and a tile-split site hands its list of heavy tiles to its own next launch, so only from the fourth frame
    on does every launch -- the frame of the edit among them -- meet a list (tests/test_gpu_motion_vectors.py, split_ran)."""
    sd = scene_data(name)
    before, gap = case_edits(name, kind, with_slide)
    if kind in CAMERA_KINDS:
        side.set_camera_position(camera_case(sd, kind)[0])
    for e in before:
        apply(side, e)
    side.advance()                                          # the case starts from a scene at rest
    for _ in range(WARM_FRAMES):
        side.frame()
    out = []

    def frame():
        out.append(side.frame())
        if on_frame:
            on_frame(len(out) - 1)
    frame()
    for e in gap:
        apply(side, e)
    frame()
    side.advance()
    frame()
    side.advance()
    frame()
    return out


@functools.lru_cache(maxsize=None)
def oracle_case(name, kind, pipeline, tracked=True, with_slide=True):
    """run_case on the oracle (cos / sin correctly rounded, as the device evaluates them): the four states, and the camera-only motion
    plane of each frame."""
    from restir_amd import capi
    ob.set_libm_mode(1)
    o = OracleMotion(capi, scene_data(name), tracked=tracked, pipeline=pipeline)
    camera_only = []
    frame = o.frame

    def noting():
        st = frame()
        camera_only.append(o.camera_only)
        return st
    o.frame = noting
    return run_case(o, name, kind, with_slide), camera_only[-4:]
