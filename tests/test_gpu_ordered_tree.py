"""GPU parity tests of the closest-hit trees that keep the reference's visiting order (occlusion_bvh.cpp rs_build_ordered_bvh,
rs_walk.h walk_ordered_tree): the wave-level service the multi-bounce kernels use for their bounce rays must return what
DevScene::intersect (src/scene.h:245-284) returns -- primitive, material, position and normal bit for bit -- for every ray:
against the library's literal per-lane walk of the reference's tree, against the same service with the trees switched off, and
against the oracle."""
import numpy as np
import pytest

from tests.common import bits_equal, get_scene, hip_scene, oracle_scene
from tests.ray_cases import closest_like_rays

pytestmark = pytest.mark.gpu


def _same(a, b):
    pa, ma, xa, na = [t.cpu().numpy() for t in a]
    pb, mb, xb, nb = [t.cpu().numpy() for t in b]
    assert np.array_equal(pa, pb), int((pa != pb).sum())
    hit = pa >= 0
    assert np.array_equal(ma[hit], mb[hit])
    assert bits_equal(xa[hit], xb[hit]) and bits_equal(na[hit], nb[hit])
    return hit


@pytest.mark.parametrize("name,n", [("cornell", 200000), ("sponza:0.1", 400000), ("bistro:0.05", 400000)])
def test_ordered_tree_equals_reference_walk(hip, name, n):
    import torch
    sd = get_scene(name)
    hsc = hip_scene(hip, sd)
    rays = closest_like_rays(sd, n, 31)
    dr = torch.from_numpy(rays).cuda()
    ref = hip.trace_closest(hsc, dr)                       # DevScene::intersect literally, lane by lane
    assert hip.set_ordered_tree(hsc, True), "the closest-hit trees were not built for a scene from rs_build_bvh"
    fast = hip.trace_closest_wave(hsc, dr)
    hit = _same(ref, fast)
    assert 0.3 < hit.mean() <= 1.0
    assert hip.set_ordered_tree(hsc, False)
    _same(ref, hip.trace_closest_wave(hsc, dr))            # the same service on the reference's tree
    hip.set_ordered_tree(hsc, True)
    sub = rays[::20]
    prim, mat, pos, nrm, _ = oracle_scene(sd).intersect(sub)
    gp, gm, gpos, gn = [t.cpu().numpy()[::20] for t in fast]
    assert np.array_equal(prim, gp)
    h = prim >= 0
    assert np.array_equal(mat[h], gm[h]) and bits_equal(pos[h], gpos[h]) and bits_equal(nrm[h], gn[h])


@pytest.mark.parametrize("name", ["sponza:1.0", "bistro:1.0"])
def test_ordered_tree_on_the_full_scenes(hip, name):
    """200 000 rays of every kind on the FULL scenes (262 144 / 2.83 M triangles): the closest-hit trees = the library's
    reference walk for every ray, = the oracle on every 10th."""
    import torch
    sd = get_scene(name)
    hsc = hip_scene(hip, sd)
    assert hip.set_ordered_tree(hsc, True)
    rays = closest_like_rays(sd, 200000, 32)
    dr = torch.from_numpy(rays).cuda()
    fast = hip.trace_closest_wave(hsc, dr)
    hit = _same(hip.trace_closest(hsc, dr), fast)
    assert hit.mean() > 0.3
    sub = rays[::10]
    prim, mat, pos, nrm, _ = oracle_scene(sd).intersect(sub)
    gp, gm, gpos, gn = [t.cpu().numpy()[::10] for t in fast]
    assert np.array_equal(prim, gp)
    h = prim >= 0
    assert np.array_equal(mat[h], gm[h]) and bits_equal(pos[h], gpos[h]) and bits_equal(nrm[h], gn[h])


def test_ordered_tree_in_waves_that_mix_every_kind_of_ray(hip):
    """closest_like_rays lays its kinds out in contiguous blocks, so almost every wave holds one kind.  Shuffled, every wave holds
    general-case rays (the ordered trees) beside special-case and far-origin rays (the reference walk of the slow lanes), whose
    results the service merges lane by lane.  4 133 rays: 64 full waves and one partial.  The oracle is asked about every ray."""
    import torch
    sd = get_scene("sponza:0.03")
    hsc = hip_scene(hip, sd)
    rays = closest_like_rays(sd, 4133, 34)
    rays = np.ascontiguousarray(rays[np.random.default_rng(35).permutation(len(rays))])
    dr = torch.from_numpy(rays).cuda()
    ref = hip.trace_closest(hsc, dr)
    assert hip.set_ordered_tree(hsc, True)
    fast = hip.trace_closest_wave(hsc, dr)
    hit = _same(ref, fast)
    assert 0.3 < hit.mean() <= 1.0
    assert hip.set_ordered_tree(hsc, False)
    _same(ref, hip.trace_closest_wave(hsc, dr))
    hip.set_ordered_tree(hsc, True)
    prim, mat, pos, nrm, _ = oracle_scene(sd).intersect(rays)
    gp, gm, gpos, gn = [t.cpu().numpy() for t in fast]
    assert np.array_equal(prim, gp)
    h = prim >= 0
    assert np.array_equal(mat[h], gm[h]) and bits_equal(pos[h], gpos[h]) and bits_equal(nrm[h], gn[h])


def test_ordered_tree_is_off_for_tables_without_mirrored_orders(hip):
    """rs_scene_create accepts any table of threaded orders.  The closest-hit trees need the odd orders to be the mirror images of
    the even ones (src/bvh.cpp:186-190); a table where they are not keeps the reference walk, and the results are the reference's."""
    import torch
    sd = get_scene("sponza:0.03")
    base = hip_scene(hip, sd)
    t = base.host_desc()
    t["nodes"] = t["nodes"].copy()
    t["nodes"][1] = t["nodes"][0]                            # order 1 := order 0: still a valid threaded order, no longer a mirror
    hsc = hip.Scene.from_tables(sd.vertices, sd.normals, sd.texcoords, sd.material_ids, sd.materials, t)
    assert not hip.set_ordered_tree(hsc, True)
    rays = closest_like_rays(sd, 50000, 33)
    dr = torch.from_numpy(rays).cuda()
    _same(hip.trace_closest(hsc, dr), hip.trace_closest_wave(hsc, dr))
    assert hip.set_ordered_tree(base, True)                  # and the scene those tables came from has them
