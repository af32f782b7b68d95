"""The two generators of rays and segments that the walk tests share (tests/test_gpu_ordered_tree.py, tests/test_gpu_parity.py,
tests/test_gpu_full_size.py, tests/geometric_cases.py): every kind of ray the render passes produce and the corner cases of the box
tests, from a seeded generator.  Plain NumPy, no GPU."""
import numpy as np


def closest_like_rays(sd, n, seed):
    """Rays of the kinds the bounce passes produce and the corner cases of an order-dependent closest hit: random rays inside
    the scene, bounce rays (origin on a surface, offset 1e-5 along a direction of the hemisphere), rays aimed at triangle
    vertices and at points of shared edges (equal hit distances on several triangles: the first in the reference's order wins),
    rays inside a triangle's plane (hit distances that are pure rounding), axis-aligned / near-zero components (reference walk),
    origins far outside the scene (beyond the grid's reach), NaN directions."""
    rng = np.random.default_rng(seed)
    v = sd.vertices.reshape(-1, 3, 3).astype(np.float64)
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)

    def points_on(k):
        t = v[rng.integers(0, len(v), k)]
        u = rng.uniform(size=(k, 2)); flip = u.sum(1) > 1; u[flip] = 1 - u[flip]
        p = t[:, 0] * (1 - u.sum(1))[:, None] + t[:, 1] * u[:, :1] + t[:, 2] * u[:, 1:]
        nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]); nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-20)
        return p, nrm, t

    def unit(d):
        return d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-30)

    o = rng.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo), (n, 3))
    d = unit(rng.normal(size=(n, 3)))
    k = n // 8
    # bounce rays
    p, nrm, _ = points_on(2 * k)
    dd = unit(rng.normal(size=(2 * k, 3))); dd *= np.sign(np.einsum("ij,ij->i", dd, nrm))[:, None]
    o[k:3 * k] = p + dd * 1e-5; d[k:3 * k] = dd
    # at vertices and at points of edges
    _, _, t = points_on(k)
    w = rng.uniform(size=(k, 1)); w[: k // 2] = 0.0
    target = t[:, 0] * (1 - w) + t[:, 1] * w
    d[3 * k:4 * k] = unit(target - o[3 * k:4 * k])
    # inside a triangle's plane, starting outside the triangle
    g, _, tg = points_on(k)
    o[4 * k:5 * k] = g + (tg[:, 0] - g) * 3.0; d[4 * k:5 * k] = unit((g + (tg[:, 1] - g) * 3.0) - o[4 * k:5 * k])
    # special directions
    s = k // 3
    ax = rng.integers(0, 3, s)
    d[5 * k:5 * k + s] = 0; d[np.arange(5 * k, 5 * k + s), ax] = rng.choice([-1.0, 1.0], s)
    d[5 * k + s:5 * k + 2 * s, 0] = rng.uniform(-1e-6, 1e-6, s)
    d[5 * k + 2 * s:5 * k + 3 * s, 1] = 0.0
    d[5 * k:6 * k] = unit(d[5 * k:6 * k])
    # far origins, aimed at the scene
    o[6 * k:6 * k + 64] = hi + (hi - lo) * rng.uniform(6, 40, (64, 1))
    d[6 * k:6 * k + 64] = unit(rng.uniform(lo, hi, (64, 3)) - o[6 * k:6 * k + 64])
    rays = np.ascontiguousarray(np.concatenate([o, d], 1), np.float32)
    rays[-8:, 3:] = np.nan
    return rays


def _shadow_like_segments(sd, n, seed):
    """Segments of the kinds the shadow pass produces and the corner cases of the occlusion tree: surface point ->
    light point, random pairs, short, grazing along a triangle's plane, axis-aligned / near-zero directions
    (reference walk), and origins far outside the scene (beyond the grid test's reach)."""
    rng = np.random.default_rng(seed)
    v = sd.vertices.reshape(-1, 3, 3).astype(np.float64)
    lights = np.nonzero(sd.materials["type"][sd.material_ids] == 4)[0]

    def points_on(tris, k):
        t = v[rng.choice(tris, k)]
        u = rng.uniform(size=(k, 2)); flip = u.sum(1) > 1; u[flip] = 1 - u[flip]
        p = t[:, 0] * (1 - u.sum(1))[:, None] + t[:, 1] * u[:, :1] + t[:, 2] * u[:, 1:]
        nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]); nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-20)
        return p, nrm, t

    a, na, _ = points_on(np.arange(len(v)), n)
    b, _, _ = points_on(lights if len(lights) else np.arange(len(v)), n)
    na *= np.sign(np.einsum("ij,ij->i", na, b - a))[:, None]
    a = a + 1e-4 * na
    k = n // 8
    b[k:2 * k] = points_on(np.arange(len(v)), k)[0]                                   # random surface pairs
    b[2 * k:3 * k] = a[2 * k:3 * k] + rng.normal(size=(k, 3)) * 0.05                      # short
    g, ng, tg = points_on(np.arange(len(v)), k)                                           # grazing: inside a triangle's plane
    a[3 * k:4 * k] = g + (tg[:, 0] - g) * 3.0; b[3 * k:4 * k] = g + (tg[:, 1] - g) * 3.0
    ax = rng.integers(0, 3, k)                                                            # axis-aligned / near-zero components
    b[4 * k:5 * k] = a[4 * k:5 * k]; b[np.arange(4 * k, 5 * k), ax] += rng.choice([-3.0, 3.0], k)
    b[4 * k:4 * k + k // 2, (ax[:k // 2] + 1) % 3] += rng.uniform(-2e-6, 2e-6, k // 2)
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    a[5 * k:5 * k + 64] = hi + (hi - lo) * rng.uniform(6, 40, (64, 1))                    # far origins
    seg = np.ascontiguousarray(np.concatenate([a, b], 1), np.float32)
    seg[-16:, 3:] = seg[-16:, :3]                                                         # x == y: NaN direction
    return seg
