"""CPU: the oracle against the reference's own functions compiled from the reference's sources (oracle/_ref/libref_subset.so)
and against rocThrust (libthrust_probe.so), on seeded random inputs -- larger than the committed golden vectors.  Where oracle/_ref
is absent (the reference's sources are not at hand), against the digests of the reference's outputs for the same inputs
(tests/golden/ref_digests.json, tests.common.RefOutputs)."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding as ob
from restir_amd.ctypes_structs import MATERIAL_DTYPE, copy_camera, make_camera
from tests.common import RefOutputs, bits_equal

R = ob.ref_subset()
T = ob.thrust_probe()
needs_ref = pytest.mark.skipif(R is None or T is None, reason="oracle/_ref not built (the reference's sources are not at hand)")


@pytest.fixture
def ref(request):
    r = RefOutputs(request.node.nodeid, R is not None and T is not None)
    yield r
    r.finish()


def unit(rng, n):
    v = rng.normal(size=(n, 3)).astype(np.float32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("seed", [1, 2])
def test_triangle_and_box(seed, ref):
    rng = np.random.default_rng(seed)
    n = 100000
    from tests.golden.make_golden import special_rays
    rays = special_rays(rng, n)
    tris = rng.uniform(-1, 1, (n, 9)).astype(np.float32)

    def triangles(fn):
        hit = np.zeros(n, np.int32); b = np.zeros((n, 2), np.float32); d = np.zeros(n, np.float32)
        fn(n, rays.reshape(-1), tris.reshape(-1), hit, b.reshape(-1), d)
        m = hit == 1
        return hit, b[m], d[m]                      # (barycentrics and distances of the hits)
    ref.same(triangles(ob.lib().orc_intersect_triangle), lambda: triangles(R.ref_intersect_triangle))
    boxes = np.sort(rng.uniform(-1.5, 1.5, (n, 2, 3)).astype(np.float32), axis=1).reshape(n, 6).copy()

    def aabbs(fn):
        hit = np.zeros(n, np.int32); t = np.zeros(n, np.float32)
        fn(n, rays.reshape(-1), boxes.reshape(-1), hit, t)
        return hit, t[hit == 1]
    ours = aabbs(ob.lib().orc_aabb_intersect)
    assert (ours[0] == 1).sum() > 1000
    ref.same(ours, lambda: aabbs(R.ref_aabb_intersect))


def test_rng_against_thrust(ref):
    rng = np.random.default_rng(5)
    seeds = rng.integers(-2 ** 31, 2 ** 31, 20000).astype(np.int32)
    a = np.zeros((len(seeds), 181), np.float32); b = np.zeros_like(a)
    ob.lib().orc_rng_stream_raw(len(seeds), seeds, 181, a.reshape(-1))
    ref.same((a,), lambda: (T.thr_rng_stream_raw(len(seeds), seeds, 181, b.reshape(-1)), b)[1:])


def test_bsdf_and_math(ref):
    rng = np.random.default_rng(6)
    n = 200000
    mats = np.zeros(n, MATERIAL_DTYPE)
    mats["type"] = rng.integers(0, 5, n); mats["baseColor"] = rng.uniform(0, 1, (n, 3))
    mats["metallic"] = rng.uniform(0, 1, n); mats["roughness"] = rng.uniform(0.02, 1, n); mats["ior"] = 1.5
    nr, wo, wi = unit(rng, n), unit(rng, n), unit(rng, n)
    a = np.zeros((n, 3), np.float32); b = np.zeros_like(a)
    ob.lib().orc_bsdf(n, mats.ctypes.data, nr.reshape(-1), wo.reshape(-1), wi.reshape(-1), a.reshape(-1))
    ref.same((a,), lambda: (R.ref_bsdf(n, mats.ctypes.data, nr.reshape(-1), wo.reshape(-1), wi.reshape(-1), b.reshape(-1)), b)[1:])
    col = rng.uniform(0, 16, (n, 3)).astype(np.float32)
    for mode in (0, 1, 2):
        ob.lib().orc_tonemap(n, col.reshape(-1), mode, a.reshape(-1))
        ref.same((a,), lambda: (R.ref_tonemap(n, col.reshape(-1), mode, b.reshape(-1)), b)[1:])


@pytest.mark.parametrize("nt", [1, 2, 3, 50, 3000, 40000])
def test_bvh_builder(nt, ref):
    rng = np.random.default_rng(nt)
    v = (rng.uniform(-5, 5, (nt, 1, 3)) + rng.uniform(-.3, .3, (nt, 3, 3))).astype(np.float32)
    if nt == 50:
        v[:, :, 2] = 1.0
    ref.same(ob.bvh_build(v), lambda: ob.bvh_build(v, R.ref_bvh_build))


def test_camera(ref):
    rng = np.random.default_rng(8)
    for args in [(256, 256, (0, 1, 3.5), (-90, 0, 0), 19.5), (1280, 720, (-3, 4, 9), (200, 25, 0), 35.0)]:
        a = make_camera(*args); b = copy_camera(a)
        ob.camera_update(a)

        def fields(c):
            return tuple(np.array(getattr(c, f), np.float32) for f in ("view", "up", "right", "rotationMatInv"))

        def ref_fields():
            R.ref_camera_update(C.byref(b))
            return fields(b)
        ref.same(fields(a), ref_fields)
        b = a                                          # (its fields bit-equal to the reference's: the camera both samplers below use)
        k = 50000
        xy = np.stack([rng.integers(0, args[0], k), rng.integers(0, args[1], k)], 1).astype(np.int32)
        r4 = rng.uniform(0, 1, (k, 4)).astype(np.float32)
        ra = np.zeros((k, 6), np.float32); rb = np.zeros_like(ra)
        ob.lib().orc_camera_sample(C.byref(b), k, xy.reshape(-1), r4.reshape(-1), ra.reshape(-1))
        ref.same((ra,), lambda: (R.ref_camera_sample(C.byref(b), k, xy.reshape(-1), r4.reshape(-1), rb.reshape(-1)), rb)[1:])


def test_texture_and_environment_helpers(ref):
    """image.h linearSample (through DevTextureObj) and mathUtil.h toSphere / toPlane / localToWorld, 2e5 inputs each."""
    rng = np.random.default_rng(5)
    tex = rng.uniform(0, 2, (37, 53, 3)).astype(np.float32)
    uv = rng.uniform(-3, 3, (200000, 2)).astype(np.float32)
    uv[:1000] = rng.integers(-2, 3, (1000, 2)).astype(np.float32)
    uv[1000:2000] = (rng.integers(0, 53, (1000, 2)) / np.float32(53)).astype(np.float32)
    b = np.zeros((len(uv), 3), np.float32)
    ref.same((ob.linear_sample(tex, uv),), lambda: (R.ref_linear_sample(53, 37, tex.reshape(-1), len(uv), uv.reshape(-1), b.reshape(-1)), b)[1:])
    u2 = rng.uniform(0, 1, (200000, 2)).astype(np.float32)
    b = np.zeros((len(u2), 3), np.float32)
    ref.same((ob.to_sphere(u2),), lambda: (R.ref_to_sphere(len(u2), u2.reshape(-1), b.reshape(-1)), b)[1:])
    d = rng.normal(size=(200000, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:100, 0] = 0; d[100:200, 2] = 0; d[200:300] = [0, 1, 0]
    b = np.zeros((len(d), 2), np.float32)
    ref.same((ob.to_plane(d),), lambda: (R.ref_to_plane(len(d), d.reshape(-1), b.reshape(-1)), b)[1:])
    n = rng.normal(size=(200000, 3)).astype(np.float32); n /= np.linalg.norm(n, axis=1, keepdims=True); n[:100] = [0, 1, 0]
    v = rng.uniform(-1, 1, (200000, 3)).astype(np.float32)
    b = np.zeros((len(n), 3), np.float32)
    ref.same((ob.local_to_world(n, v),), lambda: (R.ref_local_to_world(len(n), n.reshape(-1), v.reshape(-1), b.reshape(-1)), b)[1:])


def test_texture_and_environment_helpers_at_their_edges(ref):
    """The same four helpers on the edge lists of tests/surface_cases.py, which tests/test_gpu_surface_ops.py holds the device to: maps of
    1 x 1, 1 x 7, 7 x 1, 2 x 2 and 3 x 8192 texels, coordinates at exact texel borders and centres with the float on either side, at
    fract = 0 and fract = 1, at 2^23 and 1e30; texel centres of small environment maps; poles, seam, zero vector, subnormal components and
    1e30 in toPlane; |n.y| around 0.9999f in localToWorld.  Only the FINITE rows: compiled for x86 the reference converts a NaN coordinate
    to INT_MIN and indexes the map with it, while f2i's NaN -> 0 is the device's conversion, which the oracle and the library both
    restate and tests/test_gpu_surface_ops.py compares.  (proceduralTexture stays unpinned: DESIGN.md section 2.)"""
    from tests import surface_cases as sc
    for shape in sc.TEXTURE_SHAPES:
        if shape == (37, 53):
            continue                                     # (the map of the test above)
        tex = sc.texture(shape)
        uv = sc.finite_rows(sc.linear_sample_rows(shape, random_rows=20000))
        assert len(uv) > 20000 + 4 * sum(shape)
        b = np.zeros((len(uv), 3), np.float32)
        ref.same((ob.linear_sample(tex, uv),), lambda: (R.ref_linear_sample(shape[1], shape[0], tex.reshape(-1), len(uv), uv.reshape(-1), b.reshape(-1)), b)[1:])
    u2 = sc.finite_rows(sc.to_sphere_rows(random_rows=0))
    b = np.zeros((len(u2), 3), np.float32)
    ref.same((ob.to_sphere(u2),), lambda: (R.ref_to_sphere(len(u2), u2.reshape(-1), b.reshape(-1)), b)[1:])
    d = sc.finite_rows(sc.to_plane_rows(random_rows=0))
    assert len(d) == 4 ** 3 + 9 ** 3 + 3 ** 3
    b = np.zeros((len(d), 2), np.float32)
    ref.same((ob.to_plane(d),), lambda: (R.ref_to_plane(len(d), d.reshape(-1), b.reshape(-1)), b)[1:])
    nv = sc.finite_rows(sc.local_to_world_rows(random_rows=0))
    n, v = np.ascontiguousarray(nv[:, :3]), np.ascontiguousarray(nv[:, 3:])
    b = np.zeros((len(n), 3), np.float32)
    ours = ob.local_to_world(n, v)
    theirs = lambda: (R.ref_local_to_world(len(n), n.reshape(-1), v.reshape(-1), b.reshape(-1)), b)[1:]
    # normalize(0) is NaN on both sides (a zero vector, a zero normal): of the unit's own sign and payload, so those rows are compared as NaN rows
    gone = np.isnan(ours).any(axis=1)
    assert 0 < gone.sum() < len(n) // 2               # (3 of the 9 vectors have length 0 in float, and so have 5 of the 32 normals or their tangents)
    if ref.live:
        assert np.array_equal(np.isnan(theirs()[0]).any(axis=1), gone)
    ref.same((ours[~gone],), lambda: (theirs()[0][~gone],))


def test_material_sample_and_pdf(ref):
    """Material::sample / pdf against the reference's material.h on 3e5 random inputs of every type."""
    rng = np.random.default_rng(3)
    n = 300000
    mats = np.zeros(n, MATERIAL_DTYPE)
    mats["type"] = rng.integers(0, 5, n); mats["baseColor"] = rng.uniform(0, 1, (n, 3))
    mats["metallic"] = rng.uniform(0, 1, n); mats["roughness"] = rng.uniform(0.02, 1, n); mats["ior"] = rng.uniform(1.0, 2.5, n)
    mats["metallic"][:1000] = 0; mats["metallic"][1000:2000] = 1; mats["roughness"][2000:3000] = 0
    nrm, wo, wi = unit(rng, n), unit(rng, n), unit(rng, n)
    nrm[:500] = [0, 1, 0]; wo[500:1000] = nrm[500:1000]
    r3 = rng.uniform(0, 1, (n, 3)).astype(np.float32); r3[:50] = 0; r3[50:100] = 1
    ref.same(ob.material_sample(mats, nrm, wo, r3), lambda: ob.material_sample(mats, nrm, wo, r3, R.ref_material_sample))
    ref.same((ob.material_pdf(mats, nrm, wo, wi),), lambda: (ob.material_pdf(mats, nrm, wo, wi, R.ref_material_pdf),))


@needs_ref
def test_closest_hit_loop_over_reference_intersections():
    """bench.py's "reference loop" CPU baseline -- DevScene::intersect's traversal around the reference's compiled
    AABB::intersect / intersectTriangle on the reference builder's tree -- returns the oracle's hits (primitive ids; the oracle
    reports position, not distance, so distances are compared through it)."""
    from tests.common import get_scene, oracle_scene
    sd = get_scene("sponza:0.05")
    W, H = 160, 90
    cam = ob.camera_update(sd.camera(W, H))
    rng = np.random.default_rng(2)
    ys, xs = np.mgrid[0:H, 0:W]
    xy = np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.int32)
    r4 = rng.uniform(0, 1, (len(xy), 4)).astype(np.float32)
    rays = np.zeros((len(xy), 6), np.float32)
    ob.lib().orc_camera_sample(C.byref(cam), len(xy), xy.reshape(-1), r4.reshape(-1), rays.reshape(-1))
    prim, dist, seconds = ob.ref_closest_hit_loop(R, sd.vertices, rays)
    oprim, _, opos, _, _ = oracle_scene(sd).intersect(rays)
    assert np.array_equal(prim, oprim)
    hit = prim >= 0
    assert hit.mean() > 0.5 and seconds > 0
    d = np.linalg.norm(opos[hit] - rays[hit, :3], axis=1)
    assert np.allclose(d, dist[hit], rtol=1e-4, atol=1e-4)
