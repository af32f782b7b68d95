"""Inputs for the function-level checks of the surface functions (restir_amd/csrc/rs_surface.h and their restatement in
oracle/restir_oracle.c): linear_sample, procedural_texture, to_sphere, to_plane and local_to_world at the edges a rendered frame does not
reach.  tests/test_gpu_surface_ops.py feeds every row to the device's functions (rs_debug_surface_ops) and to the oracle's;
tests/test_oracle_vs_reference.py feeds the finite rows to the oracle's and to the reference's own.  Everything is seeded: the lists
are the same wherever they are built.
"""
import functools

import numpy as np

F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)
TAME = F32(0.3)
RANDOM_ROWS = 200000
TEXTURE_SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (37, 53), (3, 8192))        # (H, W)


def _f32(values):
    return np.asarray(values, dtype=np.float64).astype(F32)


def around(x):
    """x (float32 array) with the float on either side of each element."""
    x = np.asarray(x, F32)
    return np.concatenate([np.nextafter(x, F32(-np.inf)), x, np.nextafter(x, F32(np.inf))])


@functools.lru_cache(maxsize=None)
def texture(shape):
    h, w = shape
    return np.random.default_rng(h * 10007 + w).uniform(0, 2, (h, w, 3)).astype(F32)


def edge_coordinates(n):
    """One texture coordinate at the edges of linear_sample for a map of n texels along that axis: integers (fract = 0), texel borders
    k / n and texel centres (k + 1/2) / n -- where `fract(fx) > .5f` decides -- with the float on either side of each, zeros of both signs,
    tiny numbers of both signs (fract of a tiny negative number is exactly 1), the floats next to +-1, numbers whose fraction float
    cannot hold, and infinities and NaN."""
    k = np.arange(n, dtype=np.float64)
    cells = around(np.concatenate([(k / n).astype(F32), ((k + 0.5) / n).astype(F32)]))
    fixed = _f32([-2, -1, 0, 1, 2, -0.0, 1e-45, -1e-45, 1e-10, -1e-10, 2.0 ** 23 + 0.5, -(2.0 ** 23 + 0.5), 2.0 ** 22 + 0.5, -(2.0 ** 22 + 0.5),
                  2048.5, -2048.5, 1e30, -1e30, np.inf, -np.inf, np.nan])
    near_one = np.array([np.nextafter(F32(1), F32(0)), np.nextafter(F32(-1), F32(0))], F32)
    return np.concatenate([fixed, near_one, cells])


def linear_sample_rows(shape, random_rows=RANDOM_ROWS):
    """(n, 2) coordinates for the map of `shape` = (H, W): uniform ones in [-3, 3)^2, every edge of u beside a tame v, every edge of v beside
    a tame u, and edges in both components at once."""
    h, w = shape
    rng = np.random.default_rng(1000 + h * 10007 + w)
    uv = rng.uniform(-3, 3, (random_rows, 2)).astype(F32)
    eu, ev = edge_coordinates(w), edge_coordinates(h)
    m = max(len(eu), len(ev))
    both = np.stack([np.resize(eu, m), np.resize(np.roll(ev, 3), m)], 1)
    return np.ascontiguousarray(np.concatenate([uv, np.stack([eu, np.full(len(eu), TAME)], 1), np.stack([np.full(len(ev), TAME), ev], 1), both]).astype(F32))


# the two coordinates whose seed is 0 mod 2^31 - 1 (linear_congruential_engine::seed then takes 1)
SEED_ZERO = ((0.0, 0.0), (2097151.0 / 1024.0, 1023.0 / 1024.0))


def procedural_texture_rows(random_rows=RANDOM_ROWS):
    """(n, 2): uniform in [-3, 3)^2; one component on both sides of +-2048 (from there f2i(u * 1024) * 1024 leaves int), +-2 097 152
    (from there f2i saturates) and +-2^24, beside a tame one and beside itself; the two seeds that are 0 mod 2^31 - 1; +-1e30 (a
    large-argument reduction in sin), infinities, NaN; components of opposite sign."""
    rng = np.random.default_rng(77)
    uv = rng.uniform(-3, 3, (random_rows, 2)).astype(F32)
    big = around(_f32([2048, -2048, 2097152, -2097152, 2.0 ** 24, -(2.0 ** 24)]))
    wild = np.concatenate([big, _f32([1e30, -1e30, np.inf, -np.inf, np.nan, 3000.25, -3000.25, 1e6, -1e6])])
    tame = np.full(len(wild), TAME)
    signs = _f32([(-1.7, 2.3), (1.7, -2.3), (-3000.25, 5.5), (3000.25, -5.5), (-0.0, 0.0), (0.0, -0.0), (-2048.0, 2048.0), (2048.0, -2048.0)])
    return np.ascontiguousarray(np.concatenate([uv, np.stack([wild, tame], 1), np.stack([tame, wild], 1), np.stack([wild, np.roll(wild, 1)], 1),
                                                _f32(SEED_ZERO), signs]).astype(F32))


ENV_SIZES = ((1, 1), (2, 1), (3, 5), (64, 32))          # (w, h)


def to_sphere_rows(random_rows=RANDOM_ROWS):
    """(n, 2): uniform in [0, 1)^2, the texel centres sample_env_nv computes for maps of ENV_SIZES -- (.5f + x) / w in float -- and the
    exact quarters 0 .. 1 of both components."""
    rng = np.random.default_rng(78)
    rows = [rng.uniform(0, 1, (random_rows, 2)).astype(F32)]
    for w, h in ENV_SIZES:
        y, x = np.divmod(np.arange(w * h), w)
        rows.append(np.stack([(F32(.5) + x.astype(F32)) / F32(w), (F32(.5) + y.astype(F32)) / F32(h)], 1))
    q = _f32([0, .25, .5, .75, 1])
    rows.append(np.stack(np.meshgrid(q, q), -1).reshape(-1, 2))
    return np.ascontiguousarray(np.concatenate(rows).astype(F32))


def _triples(values):
    v = _f32(values)
    return np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)


def to_plane_rows(random_rows=RANDOM_ROWS):
    """(n, 3): unit vectors; every triple over {+-0, +-1} (the six axes with every sign of zero beside them, the poles and the seam of
    atan2, and the zero vector of every sign); every triple over {0, +-1e-45, +-1e-30, +-1e30, +-1} (subnormal squares, and 1e30 whose
    square overflows); triples with an infinity or a NaN."""
    rng = np.random.default_rng(79)
    d = rng.normal(size=(random_rows, 3)).astype(F32)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    return np.ascontiguousarray(np.concatenate([d, _triples([0.0, -0.0, 1.0, -1.0]), _triples([0, 1e-45, -1e-45, 1e-30, -1e-30, 1e30, -1e30, 1, -1]),
                                                _triples([np.inf, -np.inf, np.nan, 0.0, 1.0, -1.0])]).astype(F32))


def local_to_world_rows(random_rows=20000):
    """(n, 6) = normal, vector: normals whose |y| is 0.9999f (where the tangent switches) and the float on each side of it, in both signs and
    with the rest of the unit length on x, on z and on both; (0, +-1, 0); the axes; a NaN normal -- each beside a few vectors, the zero
    vector and a NaN vector among them; and random unit normals beside random vectors."""
    rng = np.random.default_rng(80)
    ys = around(_f32([0.9999]))
    normals = []
    for y in np.concatenate([ys, -ys]):
        r = F32(np.sqrt(1.0 - float(y) ** 2))
        normals += [(r, y, 0), (0, y, r), (r * F32(0.6), y, -r * F32(0.8)), (0, y, 0)]
    normals += [(0, 1, 0), (0, -1, 0), (1, 0, 0), (0, 0, -1), (-0.0, 1, -0.0), (0, 0, 0), (np.nan, 1, 0), (0, np.nan, 0)]
    vectors = [(0, 0, 1), (0, 0, 0), (0.3, -0.2, 0.93), (1, 0, 0), (0, -1, 0), (-0.5, 0.5, 0.70710678), (1e-30, 0, 1e-30), (np.nan, 0, 1), (0, 0, -0.0)]
    n, v = _f32(normals), _f32(vectors)
    listed = np.concatenate([np.repeat(n, len(v), 0), np.tile(v, (len(n), 1))], 1)
    rn = rng.normal(size=(random_rows, 3)).astype(F32)
    rn = (rn / np.linalg.norm(rn, axis=1, keepdims=True)).astype(F32)
    rv = rng.uniform(-1, 1, (random_rows, 3)).astype(F32)
    return np.ascontiguousarray(np.concatenate([np.concatenate([rn, rv], 1), listed]).astype(F32))


def finite_rows(rows):
    return np.ascontiguousarray(rows[np.isfinite(rows).all(axis=1)])
