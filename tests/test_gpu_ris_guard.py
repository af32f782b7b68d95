"""The RIS loop's single range guard per candidate (restir_amd/csrc/rs_exact.h ExactSpeculative, restir.hip ris_pixel) against the CPU
oracle, bit for bit: three frames from fresh reservoirs at 96 x 40 (the last wave of a row segment is partial, 3 840 pixels are no
multiple of the 1 024-thread block), spatiotemporal and RIS-only, through all three launch forms (k_ris, k_ris_lds, k_ris_alias_lds;
rs_set_ris_table_pixels(0) sends the 3 840 pixels to the LDS forms), both samplers, light tracking on and off.  Only k_ris_lds
carries the single guard and its re-evaluation; the other two forms run the same scenes through the Lambertian-only loop and their
per-operation guards.  Compared after every
frame: the radiance, the ray count, the frame's reservoirs (after a RIS-only frame these are the RIS winners that passed their shadow
ray), with spatial reuse the published copy, and the light indices of all three buffers.

The scenes (`view`): one wall that fills the frame, a lintel in front of the lamps that fills the top rows -- every lamp faces away
from it, so the waves of those rows hold dead candidates only, next to live rows below -- and a grid of lamps between them that face
the wall.
  lambert_N       every pixel Lambertian, N = 1, 3, 1 024 lamps (the LDS table at its smallest and its largest) and 1 500 (alias form);
  checker_3       metallic (roughness 0.3) and Lambertian cells of about two pixels alternate on the wall: both kinds inside every wave;
  metal_3         the wall all metallic;
  range_3, range_1500   the metallic cells have roughness 0 and 1e-6 in turn (alpha^2 = 1e-24 < 2^-60 as gtr2's numerator), and one more
                  lamp of area 5e-19 and a radiance that gives it two percent of the table's power: its pdf lies above 2^60, in a few lanes of
                  a wave's candidate and in none of the next one's.
Not reachable, hence not a case: a used dd below 2^-60.  A sample passes the facing test only with dot(n, toS) <= -1e-6 for the lamp's
unit normal, so |toS| >= 1e-6 and dd >= 1e-12; nearer samples are dead lanes, which the lintel rows and every back-facing lamp provide.
test_the_scenes_reach_what_they_are_for (no GPU) asserts on the oracle's outputs that the scenes are not vacuous."""
import functools

import numpy as np
import pytest

from oracle import binding as ob
from restir_amd import scenes, sobol
from restir_amd.ctypes_structs import LAMBERTIAN, LIGHT, METALLIC_WORKFLOW, make_materials
from tests.common import RIS_TABLE_PIXELS_DEFAULT, HipRenderer, OracleRenderer, bits_equal, oracle_scene

W, H = 96, 40
FRAMES = 3
WAVE = 64
F32 = np.float32

# name: (wall, lamps, with the tiny emitter)
SCENES = {
    "lambert_1": ("lambert", 1, False), "lambert_3": ("lambert", 3, False), "lambert_1024": ("lambert", 1024, False),
    "lambert_1500": ("lambert", 1500, False), "checker_3": ("checker", 3, False), "metal_3": ("metal", 3, False),
    "range_3": ("range", 3, True), "range_1500": ("range", 1500, True),
}
TINY_LEG = 1e-9


@functools.lru_cache(maxsize=None)
def view(name):
    wall, lamps, tiny = SCENES[name]
    specs = [dict(type=LAMBERTIAN, baseColor=(0.7, 0.7, 0.7)),                                               # 0
             dict(type=METALLIC_WORKFLOW, baseColor=(0.9, 0.6, 0.3), metallic=0.6, roughness=0.3),            # 1
             dict(type=METALLIC_WORKFLOW, baseColor=(0.9, 0.6, 0.3), metallic=0.5, roughness=0.0),            # 2
             dict(type=METALLIC_WORKFLOW, baseColor=(0.9, 0.6, 0.3), metallic=0.0, roughness=1e-6),           # 3
             dict(type=LIGHT, baseColor=(10.0, 10.0, 10.0)), dict(type=LIGHT, baseColor=(4.0, 9.0, 2.0)),     # 4, 5
             dict(type=LIGHT, baseColor=(1.0, 1.0, 1.0))]                                                     # 6: the tiny emitter
    s = scenes.TriangleSoup()
    # the wall z = -1, facing the camera, in cells of 0.16 (about two pixels at 96 x 40)
    nx, ny, cell = 88, 38, 0.16
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    x0, y0 = (-7.04 + ix * cell).reshape(-1), (-2.0 + iy * cell).reshape(-1)
    z = np.full_like(x0, -1.0)
    a, b, c, d = (np.stack(p, axis=1) for p in ((x0, y0, z), (x0 + cell, y0, z), (x0 + cell, y0 + cell, z), (x0, y0 + cell, z)))
    odd = ((ix + iy) & 1).reshape(-1)
    mat = {"lambert": np.zeros_like(odd), "metal": np.ones_like(odd), "checker": odd,
           "range": np.where(odd == 1, 2 + ((ix >> 1) & 1).reshape(-1), 0)}[wall]
    s.add_flat(np.stack([a, b, c], axis=1), mat)
    s.add_flat(np.stack([a, c, d], axis=1), mat)
    s.add_quad((-7, 1.45, 1), (7, 1.45, 1), (7, 4, 1), (-7, 4, 1), 0)                  # the lintel: the lamps are behind it and face away
    # the lamps: right-angled triangles with legs of 0.05 at z = 0.5, facing the wall
    cols = int(np.ceil(np.sqrt(lamps * 3.0)))
    k = np.arange(lamps)
    lx, ly = -3.0 + 6.0 * ((k % cols) + 0.5) / cols, -0.5 + 1.8 * ((k // cols) + 0.5) / (lamps // cols + 1)
    lz = np.full_like(lx, 0.5)
    s.add_flat(np.stack([np.stack(p, axis=1) for p in ((lx, ly, lz), (lx, ly + 0.05, lz), (lx + 0.05, ly, lz))], axis=1), 4 + (k & 1))
    if tiny:
        # a few percent of the table's power: power = luminance * area (the area cancels in the weight, the radiance does not)
        total = sum(np.dot(specs[4 + (i & 1)]["baseColor"], (.2126, .7152, .0722)) for i in range(lamps)) * 0.00125
        specs[6]["baseColor"] = (F32(0.02 * total / (0.5 * TINY_LEG * TINY_LEG)),) * 3
        s.add_flat([[(0.0, 0.0, 0.5), (0.0, TINY_LEG, 0.5), (TINY_LEG, 0.0, 0.5)]], 6)             # (at 0, where a float holds a leg of 1e-9)
    return scenes.SceneData(name, s, make_materials(specs), dict(position=(0.0, 1.0, 3.5), rotation=(-90.0, 0.0, 0.0), fov_y=19.5, focal_dist=1.0))


@functools.lru_cache(maxsize=None)
def sobol_table():
    return sobol.sobol_table()


def snapshot(r, reuse, download, ids):
    out = dict(image=np.array(r.image if isinstance(r.image, np.ndarray) else r.image.cpu().numpy()), rays=int(r.rays), last=download(1).copy(),
               ids=[ids(w).copy() for w in (0, 1, 2)])
    if reuse & 2:
        out["temp"] = download(2).copy()
    return out


@functools.lru_cache(maxsize=None)
def oracle_frames(name, sampler, track, reuse):
    """What the oracle leaves after each of the FRAMES frames, computed once and shared among the launch forms (nobody writes to it).
    libm mode 1 (cos / sin / atan2 correctly rounded, as the library evaluates them) for the time of the run."""
    ob.set_libm_mode(1)
    try:
        o = OracleRenderer(view(name), W, H, sobol=sobol_table() if sampler == "sobol" else None, track=track)
        buffers = {1: lambda: o.restir.last, 2: lambda: o.restir.temp}
        frames = []
        for _ in range(FRAMES):
            o.frame(reuse)
            frames.append(snapshot(o, reuse, lambda w: buffers[w](), o.light_ids))
        prim = o.gbuf.prim_id[o.gbuf.frame_idx ^ 1].copy()          # the material id of the hit; -1 a miss, -2 a lamp
        return frames, prim
    finally:
        ob.set_libm_mode(0)


def same(a, b, tag):
    assert a["rays"] == b["rays"], (tag, "rays", a["rays"], b["rays"])
    assert bits_equal(a["image"], b["image"]), (tag, "radiance", int((a["image"].view(np.uint32) != b["image"].view(np.uint32)).any(axis=1).sum()))
    for w in (0, 1, 2):
        assert np.array_equal(a["ids"][w], b["ids"][w]), (tag, "light ids", w, int((a["ids"][w] != b["ids"][w]).sum()))
    for which in ("last", "temp"):
        if which in a:
            x, y = a[which], b[which]
            assert np.array_equal(x["numSamples"], y["numSamples"]), (tag, which, "numSamples")
            for k in ("Li", "wi", "dist", "weight"):
                assert bits_equal(x[k], y[k]), (tag, which, k, int((x[k].view(np.uint32) != y[k].view(np.uint32)).reshape(len(x), -1).any(axis=1).sum()))


# the launch forms a table of that many lamps can take: rs_set_ris_table_pixels(0) = the LDS form the table fits, 1 << 30 = k_ris
CASES = [(n, form) for n in SCENES for form in (("lds" if SCENES[n][1] + SCENES[n][2] <= 1024 else "alias_lds"), "global")]


@pytest.mark.gpu
@pytest.mark.parametrize("track", [True, False], ids=["tracked", "untracked"])
@pytest.mark.parametrize("sampler", ["engine", "sobol"])
@pytest.mark.parametrize("name,form", CASES, ids=["%s-%s" % c for c in CASES])
def test_ris_forms_bit_for_bit(hip, name, form, sampler, track):
    hip.set_sync(True)
    hip.set_ris_table_pixels(1 << 30 if form == "global" else 0)
    try:
        for reuse in (3, 0):
            want, _ = oracle_frames(name, sampler, track, reuse)
            h = HipRenderer(hip, view(name), W, H, sobol=sobol_table() if sampler == "sobol" else None, track=track)
            for f in range(FRAMES):
                h.frame(reuse)
                same(want[f], snapshot(h, reuse, h.restir.download, h.light_ids), (name, form, sampler, track, reuse, f))
            h.scene.destroy()
    finally:
        hip.set_ris_table_pixels(RIS_TABLE_PIXELS_DEFAULT)


def runs(flags):
    """flags per pixel -> per run of 64 consecutive pixel indices (a wave of the RIS kernels; the last one of the frame is whole: 3 840 = 60 x 64)"""
    return flags.reshape(-1, WAVE)


def test_the_scenes_reach_what_they_are_for():
    """On the oracle alone (RIS-only frames, whose reservoirs are the RIS winners that passed the shadow ray)."""
    frames, prim = oracle_frames("lambert_3", "engine", True, 0)
    shaded, lit = runs(prim >= 0), runs(frames[0]["last"]["weight"] > 0)
    dead = shaded.any(axis=1) & ~lit.any(axis=1)
    assert dead.sum() >= 8 and (~dead & lit.any(axis=1)).sum() >= 8, (int(dead.sum()), int(lit.any(axis=1).sum()))   # waves of dead candidates beside live ones
    assert (shaded.any(axis=1) & ~shaded.all(axis=1)).any()              # waves with lanes that shade nothing (a lamp in view)
    for name in ("checker_3", "range_3", "range_1500"):
        frames, prim = oracle_frames(name, "engine", True, 0)
        metal, lambert = runs(prim >= 1), runs(prim == 0)
        assert (metal.any(axis=1) & lambert.any(axis=1)).sum() >= 30, name       # both materials inside a wave
    for name in ("range_3", "range_1500"):
        frames, prim = oracle_frames(name, "engine", True, 0)
        sd = view(name)
        # gtr2's numerator alpha^2 (alpha = roughness^2) per pixel of the rendered frame: +0 for roughness 0 (a numerator the short form
        # takes), 1e-24 < 2^-60 for roughness 1e-6 (outside), none for a Lambertian pixel -- and runs of 64 pixels that hold both sides
        rough = sd.materials["roughness"][np.maximum(prim, 0)].astype(F32)
        alpha = rough * rough
        aa = alpha * alpha
        metal = sd.materials["type"][np.maximum(prim, 0)] == METALLIC_WORKFLOW
        outside, inside_or_none = runs((prim >= 0) & metal & (aa > 0) & (aa < F32(2.0 ** -60))), runs((prim >= 0) & (~metal | (aa == 0)))
        assert (outside.any(axis=1) & inside_or_none.any(axis=1)).sum() >= 30 and (runs(metal & (prim >= 0) & (aa == 0))).any(), name
        # The operands of the weight quotient (pdf, itself the quotient of d.w * dd by |cos|, and the numerator g) candidate by candidate,
        # from the oracle's light sampler, for 64 points of the wall one pixel apart along a row.  The draws are a seeded generator's: the
        # renderer's own are not visible from outside; they have the same distribution, and what is asserted is a count with a wide margin.
        scene = oracle_scene(sd)
        pos = np.stack([-3.2 + 0.1 * np.arange(WAVE), np.full(WAVE, 0.5), np.full(WAVE, -1.0)], axis=1).astype(F32)
        rng = np.random.default_rng(7)
        inside = lambda x: (x >= 2.0 ** -60) & (x < 2.0 ** 60)
        clean = mixed = 0
        for _ in range(128):
            pdf, Li, wi, _ = scene.sample_direct_light_nv(pos, rng.random((WAVE, 4), dtype=F32))
            live = pdf > 0
            g = Li * F32(1.0 / np.pi) * np.maximum(wi[:, 2:3], 0)                # the Lambertian weight's numerator; the wall's normal is +z
            ok = inside(pdf) & (inside(g) | (g == 0)).all(axis=1)
            clean += bool(live.any() and ok[live].all())
            mixed += bool((live & ok).any() and (live & ~ok).any())
        assert clean >= 8 and mixed >= 8, (name, clean, mixed)        # candidates that stay in range and candidates with lanes on both sides
