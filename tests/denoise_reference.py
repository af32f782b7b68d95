"""The two denoisers in float64: an independent statement of src/denoiser.cu, the arbiter between the HIP kernels and the C oracle.

Plain numpy.  The float32 input planes (ids, normals, depth, motion, colour, the camera's fields) are taken as exact and widened; every
operation after that is a float64 one (np.exp, **, np.sqrt).  The reference's float32 constants -- both Gaussian tables, 1e-4f,
FLT_EPSILON, the luminance weights, Alpha = .2f -- enter as the float32 value widened, because that value is what the filter is
defined with.  Images are (H, W, 3) / (H, W) arrays here; the callers reshape.

  positions            Camera::getPosition                       sceneStructs.h:48-64
  eaw_level            waveletFilter, colour form                src/denoiser.cu:64-134
  eaw_filter           LeveledEAWFilter::filter                  src/denoiser.cu:463-477
  SVGF                 SpatioTemporalFilter                      src/denoiser.cu:136-216,250-371,479-568
  modulate_albedo/add  modulateAlbedo, addImage                  src/denoiser.cu:218-248

Next to its planes every filter returns the branch decisions it took per pixel, so that a test can show that a case does not sit on a
discontinuity of the filter (a pixel that flips a branch between float32 and float64 is not a rounding difference).
"""
import numpy as np


def f32(x):
    """A float32 constant of the reference, widened."""
    return np.float64(np.float32(x))


GAUSSIAN_5X5 = np.array([[.0030, .0133, .0219, .0133, .0030],            # src/denoiser.cu:18-24
                         [.0133, .0596, .0983, .0596, .0133],
                         [.0219, .0983, .1621, .0983, .0219],
                         [.0133, .0596, .0983, .0596, .0133],
                         [.0030, .0133, .0219, .0133, .0030]], np.float32).astype(np.float64)
GAUSSIAN_3X3 = np.array([[.075, .124, .075],                              # src/denoiser.cu:11-15
                         [.124, .204, .124],
                         [.075, .124, .075]], np.float32).astype(np.float64)
LUMINANCE = np.array([.2126, .7152, .0722], np.float32).astype(np.float64)   # mathUtil.h:119-123
EPS_W = f32(1e-4)                  # the floor added to every SVGF weight factor and to the colour denominator
FLT_EPSILON = np.float64(np.finfo(np.float32).eps)
ALPHA = f32(.2)                    # SpatioTemporalFilter's blend factor (:252)
NULL_PRIM = -1


def _vec(a):
    return np.array(list(a), np.float32).astype(np.float64)


def positions(cam, depth):
    """Camera::getPosition(x, y, depth[y, x]) for every pixel (sceneStructs.h:48-64): the pixel centre's ray through a pinhole
    (lens radius times 0), normalised, times the depth, from the camera position.  depth: (H, W)."""
    H, W = depth.shape
    assert (W, H) == (cam.resolution[0], cam.resolution[1])
    aspect = np.float64(W) / np.float64(H)
    tan_fov_y = np.tan(np.radians(np.float64(np.float32(cam.fov[1]))))
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    ru = 1.0 - ((x + 0.5) / W) * 2.0
    rv = 1.0 - ((y + 0.5) / H) * 2.0
    fd = np.float64(np.float32(cam.focalDist))
    d = np.stack([np.broadcast_to(ru * aspect * tan_fov_y * fd, (H, W)), np.broadcast_to(rv * tan_fov_y * fd, (H, W)),
                  np.full((H, W), fd)], -1)
    right, up, view = _vec(cam.right), _vec(cam.up), _vec(cam.view)
    w = d[..., 0:1] * right + d[..., 1:2] * up + d[..., 2:3] * view          # mat3(right, up, view) * dir
    w = w / np.sqrt((w * w).sum(-1, keepdims=True))
    return _vec(cam.position) + w * np.asarray(depth, np.float64)[..., None]


def tap(a, dy, dx):
    """a[y + dy, x + dx] where that pixel exists (0 elsewhere) and the mask of where it does."""
    H, W = a.shape[:2]
    out = np.zeros_like(a)
    ok = np.zeros((H, W), bool)
    if abs(dy) < H and abs(dx) < W:
        ys, yd = slice(max(0, dy), min(H, H + dy)), slice(max(0, -dy), min(H, H - dy))
        xs, xd = slice(max(0, dx), min(W, W + dx)), slice(max(0, -dx), min(W, W - dx))
        out[yd, xd] = a[ys, xs]
        ok[yd, xd] = True
    return out, ok


def _rows(H, rows):
    y0, y1 = (0, H) if rows is None else rows
    return max(0, y0), min(H, y1)


def eaw_level(ids, normal, pos, color, sig_lumin, sig_normal, sig_depth, level, rows=None, out=None):
    """One a-trous level of the colour filter (src/denoiser.cu:64-134) on rows [y0, y1) (default all): 5 x 5 taps `1 << level` apart,
    taps outside the image or on another id dropped, weight exp(-|dc|^2 / sigLumin) exp(-|dn|^2 / sigNormal) exp(-|dp|^2 / sigDepth)
    times the Gaussian (each factor min(1, .), which never acts on a non-positive exponent), the weighted mean of the taps' colours;
    a null pixel (id <= -1) and a pixel whose weights sum to zero keep their colour.  Rows outside the range keep `out` (zeros).
    Returns (image, dict(sum_w_zero=mask, min_sum_w=smallest weight sum over the hit pixels))."""
    H, W = ids.shape
    step = 1 << level
    color = np.asarray(color, np.float64)
    normal = np.asarray(normal, np.float64)
    sum_c = np.zeros((H, W, 3))
    sum_w = np.zeros((H, W))
    sl, sn, sd = (np.float64(np.float32(s)) for s in (sig_lumin, sig_normal, sig_depth))
    for i in range(-2, 3):
        for j in range(-2, 3):
            idq, inside = tap(ids, i * step, j * step)
            live = inside & (idq == ids)
            if not live.any():
                continue
            nq, _ = tap(normal, i * step, j * step)
            cq, _ = tap(color, i * step, j * step)
            pq, _ = tap(pos, i * step, j * step)
            with np.errstate(over="ignore", invalid="ignore"):
                e = ((color - cq) ** 2).sum(-1) / sl + ((normal - nq) ** 2).sum(-1) / sn + ((pos - pq) ** 2).sum(-1) / sd
                w = np.where(live, np.exp(-e) * GAUSSIAN_5X5[i + 2, j + 2], 0.0)
                sum_c += np.where(live[..., None], cq * w[..., None], 0.0)
            sum_w += w
    hit = ids > NULL_PRIM
    zero = hit & (sum_w == 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        res = np.where((zero | ~hit)[..., None], color, sum_c / np.where(sum_w == 0.0, 1.0, sum_w)[..., None])
    y0, y1 = _rows(H, rows)
    full = np.zeros((H, W, 3)) if out is None else np.array(out, np.float64).reshape(H, W, 3)
    full[y0:y1] = res[y0:y1]
    return full, dict(sum_w_zero=zero, min_sum_w=float(sum_w[hit].min()) if hit.any() else np.inf)


def eaw_filter(ids, normal, pos, color, sig_lumin=64.0, sig_normal=np.float32(.2), sig_depth=1.0, levels=5):
    """LeveledEAWFilter::filter (src/denoiser.cu:463-477): levels 0 .. 4, each on the previous one's output."""
    c = np.asarray(color, np.float64)
    zero = np.zeros(ids.shape, bool)
    low = np.inf
    for level in range(levels):
        c, d = eaw_level(ids, normal, pos, c, sig_lumin, sig_normal, sig_depth, level)
        zero |= d["sum_w_zero"]
        low = min(low, d["min_sum_w"])
    return c, dict(sum_w_zero=zero, min_sum_w=low)


def modulate_albedo(image, albedo):
    """modulateAlbedo (src/denoiser.cu:218-228): Math::LDRToHDR (c / 1, then c / (1 - c + 1e-4f)) times max(albedo, 0)."""
    c = np.asarray(image, np.float64) / 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        c = c / ((1.0 - c) + EPS_W)
    return c * np.maximum(np.asarray(albedo, np.float64), 0.0)


def add(a, b):
    """addImage (src/denoiser.cu:230-248)."""
    return np.asarray(a, np.float64) + np.asarray(b, np.float64)


class SVGF:
    """SpatioTemporalFilter with its state over frames.  The buffers are handed over as filter() and nextFrame do (:532-568): the
    colour of level 0 becomes the history (the caller's buffer is swapped with devAccumColor[frameIdx]), variance and its temporary
    alternate, nextFrame flips frameIdx.

    After filter(): .accum_color[frame_idx], .accum_moment[frame_idx], .variance (the last level's) and .decisions, a dict of
      diff              (H, W) the pixel restarted its history (temporalAccumulate :250-305)
      normal_dot        (H, W) |n . n_last| where the history was kept or dropped by that test alone, NaN elsewhere
      temporal_variance (H, W) variance from the accumulated moments (m.z > 3.5) instead of the 3 x 3 estimate (:307-343)
      sum_w_small       (5, H, W) level l returned the input colour   (sumWeight  < FLT_EPSILON, :208)
      sum_w2_small      (5, H, W) level l returned the input variance (sumWeight2 < FLT_EPSILON, :209)
      min_sum_w, sum_w2_log_margin   how far the sums stayed from FLT_EPSILON (smallest sum; smallest |log10(sumW2 / eps)|)."""

    def __init__(self, width, height, sig_lumin=4.0, sig_normal=128.0, sig_depth=1.0):          # :488
        self.W, self.H = width, height
        self.set_params(sig_lumin, sig_normal, sig_depth)
        z3 = lambda: np.zeros((height, width, 3))
        self.accum_color = [z3(), z3()]
        self.accum_moment = [z3(), z3()]
        self.variance = np.zeros((height, width))
        self.first_time = True
        self.frame_idx = 0
        self.decisions = None

    def set_params(self, sig_lumin, sig_normal, sig_depth):
        self.sig_lumin, self.sig_normal, self.sig_depth = (np.float64(np.float32(s)) for s in (sig_lumin, sig_normal, sig_depth))

    def next_frame(self):
        self.frame_idx ^= 1

    # temporalAccumulate (:250-305): the history of the pixel `motion` names is kept when that pixel exists, this pixel is a hit, the ids
    # agree and the normals are not nearly perpendicular; colour and first two moments then move a fifth of the way to the new sample
    def _temporal(self, color, ids, normal, motion, last_ids, last_normal):
        H, W = self.H, self.W
        fi = self.frame_idx
        m = np.asarray(motion).reshape(-1)
        li = np.where(m < 0, 0, m)
        idf = ids.reshape(-1)
        same = last_ids.reshape(-1)[li] == idf
        ndot = np.abs((normal.reshape(-1, 3) * last_normal.reshape(-1, 3)[li]).sum(-1))
        reached = (m >= 0) & (idf > NULL_PRIM) & same & (not self.first_time)
        diff = ~reached | (ndot < f32(.1))
        lum = color @ LUMINANCE
        lumf = lum.reshape(-1)
        lc = self.accum_color[fi ^ 1].reshape(-1, 3)[li]
        lm = self.accum_moment[fi ^ 1].reshape(-1, 3)[li]
        cf = color.reshape(-1, 3)
        with np.errstate(invalid="ignore", over="ignore"):
            acc_c = np.where(diff[:, None], cf, lc + (cf - lc) * ALPHA)
            acc_m = np.stack([np.where(diff, lumf, lm[:, 0] + ALPHA * (lumf - lm[:, 0])),
                              np.where(diff, lumf * lumf, lm[:, 1] + ALPHA * (lumf * lumf - lm[:, 1])),
                              np.where(diff, 0.0, lm[:, 2] + 1.0)], -1)
        self.accum_color[fi] = acc_c.reshape(H, W, 3)
        self.accum_moment[fi] = acc_m.reshape(H, W, 3)
        self.first_time = False
        return diff.reshape(H, W), np.where(reached, ndot, np.nan).reshape(H, W)

    # estimateVariance (:307-343): E[l^2] - E[l]^2 from the accumulated moments once more than 3.5 frames went in, before that from the
    # means of the two moments over the 3 x 3 pixels around (those inside the image)
    def _estimate_variance(self, moment):
        sx = np.zeros((self.H, self.W)); sy = np.zeros((self.H, self.W)); n = np.zeros((self.H, self.W))
        for i in range(-1, 2):
            for j in range(-1, 2):
                q, ok = tap(moment, i, j)
                sx += q[..., 0]; sy += q[..., 1]; n += ok
        temporal = moment[..., 2] > 3.5
        with np.errstate(invalid="ignore", over="ignore"):
            var = np.where(temporal, moment[..., 1] - moment[..., 0] ** 2, sy / n - (sx / n) ** 2)
        return var, temporal

    # filterVariance (:345-371): the 3 x 3 Gaussian mean of the variance.  The reference moves qx with the OUTER loop variable and qy with
    # the inner one (:358-359) while it indexes the table [outer][inner]; the table is symmetric, so only the summation order differs
    @staticmethod
    def _filter_variance(var):
        s = np.zeros_like(var); w = np.zeros_like(var)
        for i in range(-1, 2):
            for j in range(-1, 2):
                q, ok = tap(var, j, i)                      # qx = x + i, qy = y + j
                with np.errstate(invalid="ignore"):
                    s += np.where(ok, q * GAUSSIAN_3X3[i + 1, j + 1], 0.0)
                w += ok * GAUSSIAN_3X3[i + 1, j + 1]
        return s / w

    # waveletFilter, joint form (:139-216)
    def _level(self, color, var, ids, normal, pos, level):
        H, W = self.H, self.W
        step = 1 << level
        vf = self._filter_variance(var)
        with np.errstate(invalid="ignore"):
            denom = self.sig_lumin * np.sqrt(np.maximum(vf, 0.0)) + EPS_W
        lum = color @ LUMINANCE
        sc = np.zeros((H, W, 3)); sv = np.zeros((H, W)); sw = np.zeros((H, W)); sw2 = np.zeros((H, W))
        for i in range(-2, 3):
            for j in range(-2, 3):
                idq, inside = tap(ids, i * step, j * step)
                live = inside & (idq == ids)
                if not live.any():
                    continue
                nq, _ = tap(normal, i * step, j * step); cq, _ = tap(color, i * step, j * step); pq, _ = tap(pos, i * step, j * step)
                vq, _ = tap(var, i * step, j * step); dq, _ = tap(denom, i * step, j * step); lq, _ = tap(lum, i * step, j * step)
                with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                    w_pos = np.exp(-((pos - pq) ** 2).sum(-1) / self.sig_depth) + EPS_W
                    w_norm = np.maximum((normal * nq).sum(-1), 0.0) ** self.sig_normal + EPS_W
                    w_col = np.exp(-np.abs(lum - lq) / np.where(live, dq, 1.0)) + EPS_W
                    w = np.where(live, w_col * w_norm * w_pos * GAUSSIAN_5X5[i + 2, j + 2], 0.0)
                    sc += np.where(live[..., None], cq * w[..., None], 0.0)
                    sv += np.where(live, vq * w * w, 0.0)
                sw += w; sw2 += w * w
        hit = ids > NULL_PRIM
        small = hit & (sw < FLT_EPSILON)
        small2 = hit & (sw2 < FLT_EPSILON)
        with np.errstate(invalid="ignore", divide="ignore"):
            c_out = np.where((small | ~hit)[..., None], color, sc / np.where(sw == 0.0, 1.0, sw)[..., None])
            v_out = np.where(small2 | ~hit, var, sv / np.where(sw2 == 0.0, 1.0, sw2))
        return c_out, v_out, small, small2, sw[hit], sw2[hit]

    def filter(self, color, ids, normal, depth, motion, last_ids, last_normal, cam):
        """One frame (:532-564).  color (H, W, 3); ids, depth (H, W); normal (H, W, 3); motion (H, W) the index of the pixel's place in
        the last frame or -1; last_ids / last_normal the last frame's planes.  Returns the filtered colour."""
        color = np.asarray(color, np.float64); normal = np.asarray(normal, np.float64); last_normal = np.asarray(last_normal, np.float64)
        pos = positions(cam, depth)
        fi = self.frame_idx
        diff, ndot = self._temporal(color, ids, normal, motion, last_ids, last_normal)
        var, temporal = self._estimate_variance(self.accum_moment[fi])
        smalls, smalls2, lows, margins = [], [], [np.inf], [np.inf]
        c = self.accum_color[fi]
        for level in range(5):
            c, var, s1, s2, sw, sw2 = self._level(c, var, ids, normal, pos, level)
            if level == 0:
                self.accum_color[fi] = c                        # the filtered colour of level 0 is the new history (:546)
            smalls.append(s1); smalls2.append(s2)
            if sw.size:
                lows.append(float(sw.min()))
                with np.errstate(divide="ignore"):
                    margins.append(float(np.abs(np.log10(sw2 / FLT_EPSILON)).min()))
        self.variance = var
        self.decisions = dict(diff=diff, normal_dot=ndot, temporal_variance=temporal, sum_w_small=np.stack(smalls),
                              sum_w2_small=np.stack(smalls2), min_sum_w=min(lows), sum_w2_log_margin=min(margins))
        return c
