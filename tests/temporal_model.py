"""The temporal stage of the denoiser (mi_denoise_image_temporal, include/mi355pt.h) as a NumPy model: float32, one rounding per operation, in the order of the
definition, so that the device result can be compared bit for bit.  Rules 1, 2 and 5 (demodulation, the automatic position width, the a-trous levels) are those of
tests/denoise_model.py.  The four bilinear taps are applied to all candidate pixels at once, j outer and i inner, which keeps each pixel's own operation order; a
tap that does not count is selected away, never multiplied in.  A history is a dict (a, n, N, P, M, demod, frames); None stands for "no frame yet"."""
import numpy as np
from tests import denoise_model as dm

f32 = np.float32
DEFAULTS = dict(max_history=32.0, temporal_sigma_position=-0.01, min_normal_dot=0.9)


def project(M, q):
    """X, Y, Wc of the points q [..., 3] under the projection M (12 floats), each as a three-step float32 sum"""
    M = np.asarray(M, f32).reshape(12); x, y, z = q[..., 0], q[..., 1], q[..., 2]
    return tuple(((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3] for r in range(3))


def accumulate(hist, c0, N, P, Q, tp, max_history=32.0, min_normal_dot=0.9, stats=None):
    """rule 3: -> (a, n).  stats (a dict, optional) receives boolean maps: `alone`, `outside` (no history by rule 3.1 / 3.2), `rejected` (projected inside the
    image, no tap counted) and `accepted`."""
    H, W = c0.shape[:2]
    with np.errstate(all="ignore"):
        finite = np.isfinite(c0).all(-1) & np.isfinite(N).all(-1) & np.isfinite(P).all(-1) & np.isfinite(Q).all(-1)
        a = c0.copy(); n = np.where(finite, f32(1.0), f32(0.0)).astype(f32)
        maps = dict(alone=~finite if hist is not None else np.ones((H, W), bool), outside=np.zeros((H, W), bool), rejected=np.zeros((H, W), bool), accepted=np.zeros((H, W), bool))
        if hist is not None:
            X, Y, Wc = project(hist["M"], Q)
            front = finite & (Wc > 0)
            fx = X / Wc - f32(0.5); fy = Y / Wc - f32(0.5)
            cand = front & (fx > f32(-1.0)) & (fx < f32(W)) & (fy > f32(-1.0)) & (fy < f32(H))
            maps["outside"] = finite & ~cand
            ys, xs = np.nonzero(cand)
            fx, fy = fx[ys, xs], fy[ys, xs]; q = Q[ys, xs]; Np = N[ys, xs]; c = c0[ys, xs]
            xf, yf = np.floor(fx), np.floor(fy); tx, ty = fx - xf, fy - yf; x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
            tp2 = f32(tp) * f32(tp)
            sw = np.zeros(len(ys), f32); sn = np.zeros(len(ys), f32); s = np.zeros((len(ys), 3), f32)
            for j in (0, 1):
                for i in (0, 1):
                    x, y = x0 + i, y0 + j
                    inside = (x >= 0) & (x < W) & (y >= 0) & (y < H); xc, yc = np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)      # clipped taps are selected away
                    b = (tx if i else f32(1.0) - tx) * (ty if j else f32(1.0) - ty)
                    nt = hist["n"][yc, xc]; e = q - hist["P"][yc, xc]; Nh = hist["N"][yc, xc]
                    d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
                    dot = (Np[:, 0] * Nh[:, 0] + Np[:, 1] * Nh[:, 1]) + Np[:, 2] * Nh[:, 2]
                    use = inside & (b > 0) & (nt > 0) & (d2 <= tp2) & (dot >= f32(min_normal_dot))
                    bz = np.where(use, b, f32(0.0)); at = hist["a"][yc, xc]
                    sw = np.where(use, sw + bz, sw); sn = np.where(use, sn + bz * np.where(use, nt, f32(0.0)), sn)
                    for k in range(3):
                        s[:, k] = np.where(use, s[:, k] + bz * np.where(use, at[:, k], f32(0.0)), s[:, k])
            has = sw > 0; swd = np.where(has, sw, f32(1.0))
            hc = s / swd[:, None]; nh = sn / swd
            nn = np.minimum(nh + f32(1.0), f32(max_history)); alpha = f32(1.0) / nn
            blended = hc + (c - hc) * alpha[:, None]
            a[ys[has], xs[has]] = blended[has]; n[ys[has], xs[has]] = nn[has]
            maps["accepted"][ys[has], xs[has]] = True; maps["rejected"][ys[~has], xs[~has]] = True
    if stats is not None: stats.update(maps)
    return a.astype(f32), n.astype(f32)


def temporal_frame(hist, color, normal, position, albedo=None, prev_position=None, world_to_pixel=None, iterations=5, sigma_color=4.0, sigma_normal=0.3,
                   sigma_position=-0.05, max_history=32.0, temporal_sigma_position=-0.01, min_normal_dot=0.9, stats=None):
    """One frame -> (out, resolved spatial width, resolved temporal tolerance, the new history).  `hist` is not modified."""
    C = np.asarray(color, f32); N = np.asarray(normal, f32); P = np.asarray(position, f32); Q = P if prev_position is None else np.asarray(prev_position, f32)
    demod = albedo is not None
    if hist is not None and hist["demod"] != demod: raise ValueError("demodulate differs from the history's last frame")
    with np.errstate(all="ignore"):
        D = None; c0 = C
        if demod:
            A = np.asarray(albedo, f32); D = np.where(A > f32(1e-3), A, f32(1e-3)); c0 = C / D
        tp, _ = dm.resolve_sigma_position(P, temporal_sigma_position)
        a, n = accumulate(hist, c0, N, P, Q, tp, max_history, min_normal_dot, stats)
        if iterations == 0:
            c, resolved = a, (f32(sigma_position) if sigma_position > 0 else f32(0.0))
        else:
            c, resolved = dm.atrous(a, N, P, None, iterations=iterations, sigma_color=sigma_color, sigma_normal=sigma_normal, sigma_position=sigma_position)
        out = c * D if demod else c
    new = dict(a=a, n=n, N=N.copy(), P=P.copy(), M=np.asarray(world_to_pixel, f32).reshape(12).copy(), demod=demod, frames=(hist["frames"] if hist else 0) + 1)
    return out.astype(f32), f32(resolved), f32(tp), new


# ---------------------------------------------------------------------------------------------- the test sequence
PAN_CX = (0.0, 0.4, 0.8, 0.8, 1.2)      # pinhole x per frame
PAN_GX = (0.0, 0.0, 0.0, 0.5, 0.5)      # foreground rectangle's centre x per frame: it moves in frame 3
PANNING = (1, 2, 4)                     # the frames whose camera moved
SIZES = ((70, 37), (33, 19), (45, 13))  # census sizes; the device comparison adds (1, 1) and (3, 2)


def pan_sequence(w, h):
    """Five frames of a pinhole at (cx, 0, 0) looking along +z, focal length w / (2 tan 30 deg) pixels, in front of a back plane z = 10 (normal (0, 0, -1)) and a
    foreground rectangle |x - gx| < 1.2, |y| < 0.8 at z = 5 (normal (0.3, 0, -0.954)).  P is the exact hit of each pixel centre's ray (float64, rounded once);
    prev_position carries the foreground's move.  The albedo is a checkerboard of 0.5 world units fixed to the surfaces, the colour albedo x irradiance (1.0 back,
    0.3 foreground) x gamma(2, 0.5) noise with a new seed per frame, as denoise_model.synthetic.  70 x 37: frame 2 carries a NaN colour, an Inf colour and a NaN
    normal pixel (denoise_model.plant_non_finite; `places`).  -> list of dicts color, normal, position, albedo, prev_position, world_to_pixel, clean."""
    f = w / (2.0 * np.tan(np.radians(30.0))); frames = []
    i, j = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5); dx, dy = (i - w / 2.0) / f, (j - h / 2.0) / f
    for k, (cx, gx) in enumerate(zip(PAN_CX, PAN_GX)):
        xf, yf = cx + 5.0 * dx, 5.0 * dy; fg = (np.abs(xf - gx) < 1.2) & (np.abs(yf) < 0.8)
        z = np.where(fg, 5.0, 10.0); P64 = np.stack([cx + z * dx, z * dy, z], -1)
        move = gx - PAN_GX[k - 1] if k else 0.0
        Q64 = P64 - np.where(fg[..., None], [move, 0.0, 0.0], [0.0, 0.0, 0.0])
        normal = np.where(fg[..., None], f32([0.3, 0.0, -0.954]), f32([0.0, 0.0, -1.0])).astype(f32)
        sx = P64[..., 0] - np.where(fg, gx, 0.0)      # the checkerboard rides on its surface
        check = (np.floor(sx / 0.5) + np.floor(P64[..., 1] / 0.5)) % 2 == 0
        albedo = np.where(check[..., None], f32([0.8, 0.7, 0.6]), f32([0.2, 0.25, 0.3])).astype(f32)
        clean = (albedo * np.where(fg, 0.3, 1.0)[..., None]).astype(f32)
        rng = np.random.default_rng(1000 * w + 10 * h + k)
        color = (clean * rng.gamma(2.0, 0.5, (h, w, 3))).astype(f32)
        M = f32([f, 0.0, w / 2.0, -f * cx, 0.0, f, h / 2.0, 0.0, 0.0, 0.0, 1.0, 0.0])
        fr = dict(color=color, normal=normal, position=P64.astype(f32), albedo=albedo, prev_position=Q64.astype(f32), world_to_pixel=M, clean=clean, foreground=fg)
        if (w, h) == (70, 37) and k == 2: fr, fr["places"] = dm.plant_non_finite(fr)
        frames.append(fr)
    return frames


def run_sequence(frames, with_albedo=True, census=None, **kw):
    """the model over a list of frames from an empty history -> list of (out, resolved, tp, history after the frame); census (a list, optional) receives one dict of
    boolean maps per frame"""
    hist = None; res = []
    for fr in frames:
        st = {} if census is not None else None
        out, r, tp, hist = temporal_frame(hist, fr["color"], fr["normal"], fr["position"], fr["albedo"] if with_albedo else None, fr["prev_position"], fr["world_to_pixel"], stats=st, **kw)
        res.append((out, r, tp, hist))
        if census is not None: census.append(st)
    return res

