"""Helpers of tests/test_light_retarget_host.py and tests/test_gpu_light_retarget.py: light retargeting (rs_restir_set_light_retargeting)
restated in NumPy float32, one operation per rounding, in the order of sample_light_with -- and composed with the CPU oracle, which knows
nothing of retargeting: the temporal candidate of pixel i sits in the oracle's `last` slot motion[i], so the helper writes pixel i's
re-evaluated sample there and lets the unmodified oracle run the frame.  (The oracle's tracked merge then rescales the patched sample by
luminance(Le) / luminance(Li') = x / x = 1: nothing.)  When two shaded pixels read one slot (a moving camera) the pixels are coloured into
groups with distinct slots and phase A runs per group on copies.  The oracle keeps a pixel's post-temporal reservoir in its per-frame
state as well, which phase B shades from, so every group has a state of its own: phase B runs per group on the reservoirs and the
published copy that the groups assembled, and every pixel's radiance is taken from its own group's run.

Light records and the moved-at stamps are restated from the oracle's tables and from the edits the test makes; the BSDF is the oracle's
(orc_bsdf), occlusion the edited oracle scene's test_occlusion.  The frame's surface (position, shading normal, material) is the one the
library wrote (rs_debug_restir_surface / _wo): the oracle's own RIS of the same frame runs from the oracle's own surface, so a wrong
position breaks the same comparison.

The records { light, u, v, pdf } are carried on this side too (Pair.rec_cur / rec_last / rec_temp, ping-ponged like the library's) and
compared whole after every frame.  A reservoir the ORACLE published holds either its temporal candidate -- then the record is the one
this side carried for that slot, with the restated pdf' where the candidate was evaluated again -- or this frame's RIS winner.  The
oracle does not tell which (u, v) its RIS drew, so for a RIS winner the library's pair is taken, but only after it has been held to the
oracle's reservoir: the restated light sample at (u, v) from the pixel's position must give the oracle's Li, wi and dist and the
library's pdf bit for bit.  From then on the re-evaluation is fed from this side's records, never from the library's."""
import numpy as np

from oracle import binding as ob
from restir_amd.ctypes_structs import LIGHT_SAMPLE_DTYPE, MATERIAL_DTYPE
from tests.common import next_looper

F = np.float32
PI_GLM = F(3.14159265358979323846264338327950288)
LUMA = (F(.2126), F(.7152), F(.0722))
MAX_GROUPS = 8


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def luminance(c):
    return (c[..., 0] * LUMA[0] + c[..., 1] * LUMA[1]) + c[..., 2] * LUMA[2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1)


def light_records(scene):
    """The device's light records (scene.hip light_records) of an oracle scene: dict of v0, v1, v2, nrm, Le (k, 3) and pdf_area (k,), one per
    light primitive (the environment map's sampler entry has none)."""
    with np.errstate(all="ignore"):
        v = scene.vertices[scene.light_prim_ids].astype(F)
        v0, v1, v2 = v[:, 0], v[:, 1], v[:, 2]
        c = cross(v1 - v0, v2 - v0)
        root = np.sqrt(dot(c, c))
        nrm = c * (F(1) / root)[:, None]
        area = root * F(.5)
        Le = scene.light_radiance.reshape(-1, 3).astype(F)
        power = luminance(Le) / ((area * F(2)) * PI_GLM)
        sum_inv = F(1) / F(scene.sum_power)
        return dict(v0=v0, v1=v1, v2=v2, nrm=nrm, Le=Le, pdf_area=power * sum_inv)


def light_sample_at(rec, ids, u, v, pos):
    """rs_surface.h light_sample_at: (Li, wi, dist, pdf) of light ids[k] at (u[k], v[k]) seen from pos[k]; a sample that faces away has
    pdf -1 and zeros."""
    with np.errstate(all="ignore"):
        u = u.astype(F); v = v.astype(F); pos = pos.astype(F)
        v0, v1, v2, nrm = rec["v0"][ids], rec["v1"][ids], rec["v2"][ids], rec["nrm"][ids]
        sampled = (v1 * u[:, None] + v2 * v[:, None]) + v0 * ((F(1) - u) - v)[:, None]
        to_s = sampled - pos
        away = dot(nrm, to_s) > F(-1e-6)
        dd = dot(to_s, to_s)
        length = np.sqrt(dd)
        wi = to_s * (F(1) / length)[:, None]
        pdf = (rec["pdf_area"][ids] * dd) / np.abs(-dot(nrm, wi))
        Li = rec["Le"][ids].copy()
        Li[away] = 0; wi[away] = 0
        return Li, wi, np.where(away, F(0), length), np.where(away, F(-1), pdf)


def sample_light(scene, rec, pos, r):
    """Scene::sampleDirectLightNoVisibility for scenes without an environment map: the entry from (r.x, r.y), the point from (r.z, r.w).
    Returns (pdf, Li, wi, dist, id, u, v)."""
    n = len(scene.light_prob)
    r = r.astype(F)
    entry = np.minimum((F(n) * r[:, 0]).astype(np.int32), n - 1)
    ids = np.where(r[:, 1] < scene.light_prob[entry], entry, scene.light_fail[entry]).astype(np.int32)
    sr = np.sqrt(r[:, 3])
    u = F(1) - sr
    v = r[:, 2] * sr
    Li, wi, dist, pdf = light_sample_at(rec, ids, u, v, pos)
    return pdf, Li, wi, dist, ids, u, v


class MovedAt:
    """rs_scene's lightMoves and movedAt[numLights], restated from the edits a test makes."""

    def __init__(self, scene):
        self.light_of = {int(p): i for i, p in enumerate(scene.light_prim_ids)}
        self.moves = 0
        self.stamp = np.zeros(len(scene.light_prob), np.uint32)

    def edit(self, prim_ids):
        named = [self.light_of[int(p)] for p in np.asarray(prim_ids).reshape(-1) if int(p) in self.light_of]
        if named:
            self.moves += 1
            self.stamp[named] = self.moves


def surface_of(pos_tag, normal, wo4):
    """The shading surface as ris_pixel reconstructs it: (shaded mask, pos, nrm, materials with baseColor 1, wo)."""
    tag = pos_tag[:, 3].view(np.int32)
    shaded = ((tag >> 24) & 3) == 2
    kind = (tag >> 26) & 7
    mats = np.zeros(len(tag), MATERIAL_DTYPE)
    mats["type"] = kind
    mats["baseColor"] = 1
    mats["metallic"] = normal[:, 3]
    metal = kind == 1
    mats["roughness"] = np.where(metal, wo4[:, 3], F(0))
    wo = np.where(metal[:, None], wo4[:, :3], F(0)).astype(F)
    return shaded, np.ascontiguousarray(pos_tag[:, :3]), np.ascontiguousarray(normal[:, :3]), mats, wo


def temporal_neighbours(gbuf):
    """findTemporalNeighbor (restir.cu:20-45) on the oracle's planes after render and before update: (slot, ok) per pixel."""
    c = gbuf.frame_idx
    motion = gbuf.motion
    j = np.clip(motion, 0, len(motion) - 1)
    prim = gbuf.prim_id[c]
    ok = (motion >= 0) & (prim > -1) & (gbuf.prim_id[c ^ 1][j] == prim)
    with np.errstate(all="ignore"):
        ok &= ~(np.abs(dot(gbuf.normal[c], gbuf.normal[c ^ 1][j])) < F(.9))
        ok &= ~(np.abs(gbuf.depth[c ^ 1][j] - gbuf.depth[c]) > gbuf.depth[c] * F(.1))
    return j, ok


def target(mats, nrm, wo, Li, wi):
    """ris_candidate's g as a scalar: luminance(Li * bsdf(wi) * sat_dot(n, wi))."""
    bsdf = np.zeros((len(mats), 3), F)
    if len(mats):
        ob.lib().orc_bsdf(len(mats), mats.ctypes.data, np.ascontiguousarray(nrm, F).reshape(-1), np.ascontiguousarray(wo, F).reshape(-1),
                          np.ascontiguousarray(wi, F).reshape(-1), bsdf.reshape(-1))
    with np.errstate(all="ignore"):
        return luminance((Li * bsdf) * np.maximum(dot(nrm, wi), F(0))[:, None])


def reevaluate(scene, rec, stamp, seen_moves, env_id, slots, ok, shaded, pos, nrm, mats, wo, last, ids_last, records):
    """Steps 1-5 for every pixel.  Returns (take mask, dict of the re-evaluated candidates of the taken pixels in pixel order:
    pixel, slot, Li, wi, dist, W, pdf), and the counts (re-evaluated, segments walked, left with W = 0)."""
    n_lights = len(stamp)
    id_ = ids_last[slots]
    W = last["weight"][slots]
    take = ok & shaded & (id_ >= 0) & (id_ < n_lights) & (id_ != env_id) & (W != 0)
    take[take] &= stamp[id_[take]] > seen_moves
    px = np.nonzero(take)[0]
    j = slots[px]
    r = records[j]
    assert np.array_equal(r["light"], id_[px]), "a record's light differs from the tracked id"
    with np.errstate(all="ignore"):
        Li, wi, dist, pdf = light_sample_at(rec, id_[px], r["u"], r["v"], pos[px])
        Wn = last["weight"][j].astype(F)
        bad1 = ~(pdf > 0) | ~np.isfinite(pdf)
        p_old = target(mats[px], nrm[px], wo[px], last["Li"][j], last["wi"][j])
        p_new = target(mats[px], nrm[px], wo[px], Li, wi)
        pdf_old = r["pdf"]
        fine = (p_old > 0) & (pdf_old > 0) & np.isfinite(p_old) & np.isfinite(pdf_old)
        Wn = np.where(bad1 | ~fine, F(0), (Wn * (p_new / p_old)) * (pdf_old / pdf)).astype(F)
        walk = Wn != 0
        seg = np.concatenate([pos[px], pos[px] + wi * dist[:, None]], 1).astype(F)
        occ = np.zeros(len(px), bool)
        if walk.any():
            occ[walk] = scene.test_occlusion(seg[walk]) != 0
        Wn[occ] = 0
    out = dict(pixel=px, slot=j, Li=Li, wi=wi, dist=dist, W=Wn, pdf=pdf)
    return take, out, (len(px), int(walk.sum()), int((Wn == 0).sum()))


def groups_of(pixels, slots):
    """Colours the pixels into groups in which every slot occurs once: the k-th pixel (in pixel order) that reads a slot goes to group k."""
    order = np.argsort(slots, kind="stable")
    s = slots[order]
    start = np.concatenate([[0], np.nonzero(s[1:] != s[:-1])[0] + 1]) if len(s) else np.zeros(0, np.int64)
    rank = np.arange(len(s)) - np.repeat(start, np.diff(np.concatenate([start, [len(s)]])))
    group = np.zeros(len(pixels), np.int64)
    group[order] = rank
    return group


def oracle_frame(o, reuse, cand, iteration=0):
    """One frame of the OracleRenderer `o` with the candidates `cand` (reevaluate's dict) in place of their history slots.  Returns the
    number of groups it took."""
    r = o.restir
    o.gbuf.render(o.scene, o.cam)
    group = groups_of(cand["pixel"], cand["slot"])
    count = int(group.max()) + 1 if len(group) else 1
    assert count <= MAX_GROUPS, count
    n = o.W * o.H
    owner = np.zeros(n, np.int64)                          # the group whose phase A a pixel's results are taken from
    owner[cand["pixel"]] = group
    if r.track and r.track_scene != o.scene.uid:          # another scene's light indices: unknown, once, before the copies are made
        r.ids_last[:] = -1; r.ids_temp[:] = -1
        r.track_scene = o.scene.uid
    base = dict(reservoir=r.reservoir, last=r.last, temp=r.temp, ids=r.ids, ids_last=r.ids_last, ids_temp=r.ids_temp)
    got = {k: base[k].copy() for k in ("reservoir", "temp", "ids", "ids_temp")}
    if getattr(r, "_state", None) is None:
        r._state = ob.lib().orc_restir_state_create(o.W, o.H)
    states = getattr(r, "_group_states", None) or [r._state]
    while len(states) < count:
        states.append(ob.lib().orc_restir_state_create(o.W, o.H))
    r._group_states = states
    for g in range(count):
        r._state = states[g]
        r.reservoir, r.temp, r.ids, r.ids_temp = base["reservoir"].copy(), base["temp"].copy(), base["ids"].copy(), base["ids_temp"].copy()
        r.last, r.ids_last = base["last"].copy(), base["ids_last"].copy()
        m = group == g
        j = cand["slot"][m]
        r.last["Li"][j] = cand["Li"][m]; r.last["wi"][j] = cand["wi"][m]; r.last["dist"][j] = cand["dist"][m]; r.last["weight"][j] = cand["W"][m]
        r.phase_a(o.scene, o.cam, o.gbuf, o.looper, reuse, 0, o.H)
        mine = owner == g
        for k, a in (("reservoir", r.reservoir), ("temp", r.temp), ("ids", r.ids), ("ids_temp", r.ids_temp)):
            got[k][mine] = a[mine]
    r.reservoir, r.temp, r.ids, r.ids_temp = got["reservoir"], got["temp"], got["ids"], got["ids_temp"]
    r.last, r.ids_last = base["last"], base["ids_last"]
    before = o.image.copy()
    for g in range(count):                                 # (iteration > 0 accumulates: every group starts from the image as it was)
        r._state = states[g]
        image = before.copy()
        r.phase_b(o.scene, o.cam, o.gbuf, image, iteration, reuse, 0, o.H)
        o.image[owner == g] = image[owner == g]
    r._state = states[0]
    r.end_frame()
    o.rays = r.rays
    o.looper = next_looper(o.looper, o.sobol_num)
    o.gbuf.update(o.cam)
    return count


class Pair:
    """An oracle renderer and a library renderer with retargeting on, frame by frame: frame() runs the library's frame, restates the
    re-evaluation from what the library carried before it and runs the oracle's frame on the patched history."""

    def __init__(self, capi, name, W, H, sobol=None):
        from tests.emitter_edits import HipSide, OracleSide, scene_data
        self.capi, self.sd = capi, scene_data(name)
        self.o = OracleSide(capi, self.sd, W, H, sobol=sobol, track=True)
        self.h = HipSide(capi, self.sd, W, H, sobol=sobol)
        self.h.r.restir.set_light_retargeting(True)
        self.moved = MovedAt(self.o.r.scene)
        self.seen = 0
        self.groups = 1
        n = W * H
        self.rec_cur, self.rec_last, self.rec_temp = no_records(n), no_records(n), no_records(n)

    def edit(self, ids, v, n=None):
        self.o.set_geometry(ids, v, n)
        self.h.set_geometry(ids, v, n)
        self.moved.edit(ids)

    def frame(self, reuse):
        """Returns (library's state, oracle's state, library's counters, restated counters) of the frame."""
        o, h = self.o.r, self.h.r
        records = self.rec_last
        first = o.restir.first
        h.frame(reuse)
        pos_tag, normal, _ = h.restir.surface()
        shaded, pos, nrm, mats, wo = surface_of(pos_tag, normal, h.restir.surface_wo())
        # (the oracle's planes of this frame: its render is repeated inside oracle_frame, with the same result)
        o.gbuf.render(o.scene, o.cam)
        slots, ok = temporal_neighbours(o.gbuf)
        scene = o.scene
        env_id = len(scene.light_prob) - 1 if scene.env_map_tex >= 0 else -1
        n = o.W * o.H
        none = dict(pixel=np.zeros(0, np.int64), slot=np.zeros(0, np.int64), Li=np.zeros((0, 3), F), wi=np.zeros((0, 3), F), dist=np.zeros(0, F),
                    W=np.zeros(0, F), pdf=np.zeros(0, F))
        cand, counts = none, (0, 0, 0)
        if not first and (reuse & 1) and self.moved.moves != self.seen and o.restir.ids_last is not None:
            ids_last = o.restir.ids_last if o.restir.track_scene == scene.uid else np.full(n, -1, np.int32)
            _, cand, counts = reevaluate(scene, light_records(scene), self.moved.stamp, self.seen, env_id, slots, ok, shaded, pos, nrm, mats, wo,
                                         o.restir.last, ids_last, records)
        # every pixel's temporal candidate as the merge will see it: sample, light and record
        has = ok & (not first) & bool(reuse & 1)
        last_before = o.restir.last.copy()
        ids_before = o.restir.ids_last.copy() if o.restir.track_scene == scene.uid else np.full(n, -1, np.int32)
        c_wi, c_dist, c_id, c_rec = last_before["wi"][slots].copy(), last_before["dist"][slots].copy(), ids_before[slots], self.rec_last[slots].copy()
        px = cand["pixel"]
        c_wi[px] = cand["wi"]; c_dist[px] = cand["dist"]; c_rec["pdf"][px] = cand["pdf"]
        self.groups = oracle_frame(o, reuse, cand)
        o.rays += counts[1]
        self.seen = self.moved.moves
        carry_records(self, scene, env_id, reuse, shaded, pos, has, c_wi, c_dist, c_id, c_rec)
        ref = dict(image=o.image.copy(), rays=o.rays, last=o.restir.last.copy(), temp=o.restir.temp.copy(), ids=o.restir.light_ids(1))
        got = dict(image=h.image.cpu().numpy(), rays=h.rays, last=h.restir.download(1), temp=h.restir.download(2),
                   ids=h.restir.download_light_samples(1)["light"].copy())
        return got, ref, h.restir.retarget_stats(), counts


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_records(want, got, tag):
    """Records bit for bit: the light everywhere, the rest where a light is known."""
    assert np.array_equal(want["light"], got["light"]), (tag, "light", int((want["light"] != got["light"]).sum()))
    known = want["light"] >= 0
    for k in ("u", "v", "pdf"):
        ne = bits(want[k][known]) != bits(got[k][known])
        assert not ne.any(), (tag, k, int(ne.sum()), np.nonzero(known)[0][ne][:8])


def carry_records(self, scene, env_id, reuse, shaded, pos, has, c_wi, c_dist, c_id, c_rec):
    """This side's records after the frame the oracle has just run (see the module's text), then the comparison with the library's."""
    o, h = self.o.r, self.h.r
    new, ids = o.restir.last, o.restir.light_ids(1)         # (end_frame has swapped: what the frame published)
    lib = h.restir.download_light_samples(1)
    rec = self.rec_cur
    px = np.nonzero(shaded)[0]
    out = no_records(len(px))
    id_ = ids[px]
    out["light"] = id_
    from_cand = has[px] & (id_ >= 0) & (id_ == c_id[px]) & (bits(new["wi"][px]) == bits(c_wi[px])).all(1) & (bits(new["dist"][px]) == bits(c_dist[px]))
    same = np.ones(len(px), bool)
    for k in ("u", "v", "pdf"):
        same &= bits(c_rec[k][px]) == bits(lib[k][px])
    from_cand &= same                                       # (a RIS winner that is the candidate's very sample passes the check below instead)
    for k in ("u", "v", "pdf"):
        out[k][from_cand] = c_rec[k][px][from_cand]
    ris = (id_ >= 0) & ~from_cand
    q = px[ris]
    assert np.array_equal(lib["light"][q], id_[ris]), "a RIS winner's record names another light"
    tri = id_[ris] != env_id
    Li, wi, dist, pdf = light_sample_at(light_records(scene), id_[ris][tri], lib["u"][q][tri], lib["v"][q][tri], pos[q][tri])
    for name, a, b in (("Li", Li, new["Li"][q][tri]), ("wi", wi, new["wi"][q][tri]), ("dist", dist, new["dist"][q][tri]), ("pdf", pdf, lib["pdf"][q][tri])):
        ne = (bits(a) != bits(b)).reshape(len(a), -1).any(1)
        assert not ne.any(), ("the record of a RIS winner does not give the oracle's sample", name, int(ne.sum()), q[tri][ne][:8])
    env = lib[q][~tri]
    assert (env["u"] == 0).all() and (env["v"] == 0).all() and (env["pdf"] > 0).all()
    for k in ("u", "v", "pdf"):
        out[k][ris] = lib[k][q]
    rec[px] = out
    self.rec_cur, self.rec_last = self.rec_last, rec        # the records travel with their reservoirs
    if reuse & 2:
        self.rec_temp[px] = out
    self.carried = (int(from_cand.sum()), int(ris.sum()))
    same_records(self.rec_last, lib, "history")
    assert np.array_equal(o.restir.light_ids(2), self.rec_temp["light"]) or not (reuse & 2)
    if reuse & 2:
        same_records(self.rec_temp, h.restir.download_light_samples(2), "published copy")


def no_records(n):
    out = np.zeros(n, LIGHT_SAMPLE_DTYPE)
    out["light"] = -1
    return out

