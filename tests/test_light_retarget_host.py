"""No GPU: the NumPy restatement of light retargeting (tests/light_retarget.py) means something.  Its light sample equals the oracle's
sampleDirectLightNoVisibility bit for bit, a sample whose light did not move comes back unchanged, the grouping gives distinct slots,
and the moved-at stamps follow the edits of tests/emitter_edits.py."""
import functools

import numpy as np
import pytest

from restir_amd import capi
from tests import light_retarget as lr
from tests.common import bits_equal, oracle_scene
from tests.emitter_edits import edits_up_to, emitters, kinds_for, scene_data

F = np.float32


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return oracle_scene(scene_data(name))


def positions(scene, count, seed):
    rng = np.random.default_rng(seed)
    v = scene.vertices.reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    return (lo + (hi - lo) * rng.uniform(0, 1, (count, 3))).astype(F), rng.uniform(0, 1, (count, 4)).astype(F)


@pytest.mark.parametrize("name", ["cornell", "many", "bistro"])
def test_the_light_sample_is_the_oracles(name):
    """10^4 random positions and draws: pdf, Li, wi and dist of the restated sampler against Scene::sampleDirectLightNoVisibility.  Where
    the oracle reports an invalid sample (pdf <= 0) only that is compared: it leaves the rest undefined."""
    scene = scene_of(name)
    pos, r = positions(scene, 10000, 5)
    pdf, Li, wi, dist = scene.sample_direct_light_nv(pos, r)
    mine = lr.sample_light(scene, lr.light_records(scene), pos, r)
    valid = pdf > 0
    assert 0.2 < valid.mean() < 1.0                          # both branches of the facing test are taken
    assert np.array_equal(valid, mine[0] > 0)
    for a, b in zip((pdf, Li, wi, dist), mine[:4]):
        assert bits_equal(a[valid], b[valid])


def test_an_unmoved_sample_comes_back_unchanged():
    """A sample drawn at (u, v), evaluated again on the same light records from the same position: the same Li, wi, dist and pdf, the
    target ratio 1 and the pdf ratio 1, so W is W."""
    scene = scene_of("cornell")
    rec = lr.light_records(scene)
    pos, r = positions(scene, 4000, 9)
    pdf, Li, wi, dist, ids, u, v = lr.sample_light(scene, rec, pos, r)
    keep = pdf > 0
    Li2, wi2, dist2, pdf2 = lr.light_sample_at(rec, ids[keep], u[keep], v[keep], pos[keep])
    for a, b in ((Li[keep], Li2), (wi[keep], wi2), (dist[keep], dist2), (pdf[keep], pdf2)):
        assert bits_equal(a, b)
    W = np.random.default_rng(1).uniform(0.1, 9, keep.sum()).astype(F)
    assert bits_equal((W * (F(3) / F(3))) * (pdf[keep] / pdf2), W)


def test_reevaluate_leaves_other_lights_alone():
    """reevaluate() takes only samples of lights stamped after seen_moves, with W != 0, known and inside the table."""
    scene = scene_of("cornell")
    n = 6
    last = np.zeros(n, capi.RESERVOIR_DTYPE)
    last["weight"] = [1, 1, 0, 1, 1, 1]
    last["Li"] = 1; last["wi"] = (0, 1, 0)
    ids_last = np.array([0, 1, 0, -1, 2, 0], np.int32)       # light 1 did not move; W = 0; unknown; outside the table; not shaded
    records = np.zeros(n, lr.LIGHT_SAMPLE_DTYPE)
    records["light"] = ids_last; records["u"] = .25; records["v"] = .25; records["pdf"] = 1
    stamp = np.array([1, 0], np.uint32)
    shaded = np.array([1, 1, 1, 1, 1, 0], bool)
    pos = np.tile(np.array([[0, 0.5, 0]], F), (n, 1)); nrm = np.tile(np.array([[0, 1, 0]], F), (n, 1))
    mats = np.zeros(n, lr.MATERIAL_DTYPE); mats["baseColor"] = 1
    take, cand, counts = lr.reevaluate(scene, lr.light_records(scene), stamp, 0, -1, np.arange(n), np.ones(n, bool), shaded, pos, nrm, mats,
                                       np.zeros((n, 3), F), last, ids_last, records)
    assert list(take) == [True, False, False, False, False, False] and list(cand["pixel"]) == [0] and counts[0] == 1
    assert not lr.reevaluate(scene, lr.light_records(scene), stamp, 1, -1, np.arange(n), np.ones(n, bool), shaded, pos, nrm, mats,
                             np.zeros((n, 3), F), last, ids_last, records)[0].any()       # seen already


def test_groups_have_distinct_slots():
    rng = np.random.default_rng(3)
    slots = rng.integers(0, 40, 300)
    pixels = np.arange(300)
    group = lr.groups_of(pixels, slots)
    for g in range(group.max() + 1):
        assert len(np.unique(slots[group == g])) == (group == g).sum()
    assert group.max() + 1 == np.bincount(slots).max()       # no more groups than the busiest slot has readers
    assert lr.groups_of(np.arange(5), np.arange(5)).max() == 0
    assert len(lr.groups_of(np.zeros(0, np.int64), np.zeros(0, np.int64))) == 0


@pytest.mark.parametrize("name", ["cornell", "many", "env"])
def test_moved_at_follows_the_edits(name):
    """lightMoves counts the edits that name an emitter, and every named emitter's stamp is the count at its last edit; the library exports
    the count (host only: a null scene is refused without a device)."""
    sd = scene_data(name)
    scene = scene_of(name)
    e = emitters(sd)
    assert np.array_equal(scene.light_prim_ids, e)           # sampler entry i is the i-th emitter in primitive order
    moved = lr.MovedAt(scene)
    want = np.zeros(len(scene.light_prob), np.uint32)
    count = 0
    edits = edits_up_to(name, kinds_for(name)[-1])[0]
    for ids, _, _ in edits:
        moved.edit(ids)
        hit = np.nonzero(np.isin(e, ids))[0]
        if len(hit):
            count += 1
            want[hit] = count
        assert moved.moves == count and np.array_equal(moved.stamp, want)
    assert count == len(edits)                               # every kind names an emitter
    moved.edit(np.setdiff1d(np.arange(len(sd.material_ids)), e)[:3])
    assert moved.moves == count and np.array_equal(moved.stamp, want)       # an edit that names none changes nothing
    if scene.env_map_tex >= 0:
        assert want[-1] == 0                                 # the environment's entry never moves
    lib = capi.lib()
    assert lib.rs_scene_light_moves(None, None) == capi.RS_ERR_INVALID_ARGUMENT
    assert "lightMoved" in capi.HISTORY_TABLES and "lightMoved" not in capi.SCENE_TABLES
