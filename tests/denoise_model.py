"""The edge-avoiding a-trous filter with albedo demodulation (mi_denoise_image, include/mi355pt.h) as a NumPy model: float32, one rounding per operation, in the
order of the definition, so that the device result can be compared bit for bit.  Every tap is applied to the whole image before the next one (dy outer, dx inner),
which keeps each pixel's own operation order.  expf is the host libm's routine through ctypes (the kernels restate glibc's expf, libm_glibc.h), not np.exp.  A zero
weight is never multiplied by a colour: the product is selected away.  dtype=np.float64 runs the same definition in binary64 (np.exp there) for tolerance checks."""
import ctypes as C
import ctypes.util
import numpy as np

f32 = np.float32
TAP = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
_libm = C.CDLL(ctypes.util.find_library("m")); _libm.expf.restype = C.c_float; _libm.expf.argtypes = [C.c_float]


def expf(x):
    """libm's expf on a float32 array (one call per distinct argument)"""
    x = np.ascontiguousarray(x, f32); u, inv = np.unique(x.view(np.uint32).reshape(-1), return_inverse=True)
    vals = np.array([_libm.expf(float(v)) for v in u.view(f32)], f32)
    return vals[inv].reshape(x.shape)


def resolve_sigma_position(position, sigma_position, dtype=f32):
    """(resolved width or 0 when the term is off, kp) of rule 2 / rule 4"""
    t = dtype; sp = t(sigma_position)
    with np.errstate(all="ignore"):
        if sp > 0:
            return sp, t(1.0) / (sp * sp)
        P = np.asarray(position, t).reshape(-1, 3); ok = np.isfinite(P).all(1)
        if not ok.any():
            return t(0.0), t(0.0)
        d = P[ok].max(0) - P[ok].min(0)
        diag = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        if diag == 0:
            return t(0.0), t(0.0)
        s = abs(sp) * diag
        return s, t(1.0) / (s * s)


def synthetic(seed=1, width=70, height=37):
    """Two planes that meet at a vertical edge: the left half has normal (0, 0, 1) and irradiance 1.0, the right half normal (1, 0, 0), irradiance 0.3, and recedes
    in z; positions advance 0.1 per pixel; the albedo is a 4-pixel checkerboard; colour = albedo x irradiance x gamma(2, 0.5) noise (mean 1, one draw per pixel and
    channel).  -> dict of color, normal, position, albedo, clean (float32) and edge (the first column of the right half)."""
    rng = np.random.default_rng(seed); W, H, e = width, height, width // 2
    x, y = np.meshgrid(np.arange(W), np.arange(H)); left = x < e
    normal = np.where(left[..., None], f32([0, 0, 1]), f32([1, 0, 0])).astype(f32)
    position = np.stack([np.where(left, 0.1 * x, 0.1 * e), 0.1 * y, np.where(left, 0.0, -0.1 * (x - e))], -1).astype(f32)
    check = ((x // 4 + y // 4) % 2 == 0)
    albedo = np.where(check[..., None], f32([0.8, 0.7, 0.6]), f32([0.2, 0.25, 0.3])).astype(f32)
    irr = np.where(left, 1.0, 0.3)[..., None]
    clean = (albedo * irr).astype(f32)
    color = (clean * rng.gamma(2.0, 0.5, (H, W, 3))).astype(f32)
    return dict(color=color, normal=normal, position=position, albedo=albedo, clean=clean, edge=e)


def random_case(width, height, seed):
    """Random colour, guides and albedo with planted edges: a vertical edge at a third of the width where the normal turns and the position jumps by 40 -- with a
    position width of 0.5, or of a twentieth of the box diagonal (about 2), the exponent across it is -6400 or -400, far under the -80 cut -- and a horizontal edge
    at half the height where the colour level changes tenfold (levels 0.1 and 1.0 over an albedo of 0.3 .. 0.9: a colour width of 4 lets them through, so the pixels next to the edge do change)."""
    rng = np.random.default_rng(seed); W, H = width, height
    x, y = np.meshgrid(np.arange(W), np.arange(H)); right = (x > W // 3)[..., None]; low = (y >= (H + 1) // 2)[..., None]
    color = (rng.gamma(2.0, 0.5, (H, W, 3)) * np.where(low, 1.0, 0.1)).astype(f32)
    n = rng.normal(0, 0.05, (H, W, 3)) + np.where(right, [1.0, 0, 0], [0, 0, 1.0]); normal = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(f32)
    position = (np.stack([0.1 * x, 0.1 * y, np.zeros_like(x, float)], -1) + rng.normal(0, 0.01, (H, W, 3)) + np.where(right, [0, 0, 40.0], [0, 0, 0])).astype(f32)
    albedo = rng.uniform(0.3, 0.9, (H, W, 3)).astype(f32)
    return dict(color=color, normal=normal, position=position, albedo=albedo)


# image sizes (width, height) of the device comparison: a single pixel; smaller than the 5 x 5 stencil; narrower than the step of level 3 in one dimension, either way
# round; several tiles with ragged edges; one and a fraction of the level kernel's 32 x 8 tile in each dimension
GPU_SIZES = ((1, 1), (3, 2), (17, 5), (5, 17), (33, 19), (70, 37), (45, 13))
GPU_ITERATIONS = (1, 2, 3, 5, 8)


def plant_non_finite(case):
    """a NaN colour pixel, an Inf colour pixel and a NaN normal pixel (copies; -> case, the three (y, x) places)"""
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    places = ((5, 7), (20, 50), (30, 12))
    c["color"][places[0]] = np.nan; c["color"][places[1]][1] = np.inf; c["normal"][places[2]][0] = np.nan
    return c, places


def _d2(a, ps, qs):
    e = a[ps] - a[qs]
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def atrous(color, normal, position, albedo=None, iterations=5, sigma_color=4.0, sigma_normal=0.3, sigma_position=-0.05, dtype=f32, stats=None):
    """-> (out H x W x 3, resolved sigma_position).  albedo given = demodulate.  stats (a dict, optional) receives `cut`: the taps inside the image whose exponent
    was a number below -80, `taps`: the taps inside the image, and `levels`: the output the filter would give after 1, 2, ..., K iterations (the levels do not
    depend on K, so one run serves every smaller K)."""
    t = dtype; c = np.array(color, t); N = np.asarray(normal, t); P = np.asarray(position, t); H, W = c.shape[:2]
    if stats is not None: stats["cut"] = 0; stats["taps"] = 0; stats["levels"] = []
    if iterations == 0:
        return np.array(color, t), (t(sigma_position) if sigma_position > 0 else t(0.0))
    with np.errstate(all="ignore"):
        resolved, kp = resolve_sigma_position(P, sigma_position, t)
        D = None
        if albedo is not None:
            A = np.asarray(albedo, t); D = np.where(A > t(f32(1e-3)), A, t(f32(1e-3))); c = c / D
        kn = t(1.0) / (t(sigma_normal) * t(sigma_normal))
        for i in range(iterations):
            s = 1 << i; sc = t(sigma_color) * t(2.0 ** -i); kc = t(1.0) / (sc * sc)
            sw = np.zeros((H, W), t); acc = np.zeros((H, W, 3), t)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ox, oy = s * dx, s * dy
                    x0, x1, y0, y1 = max(0, -ox), min(W, W - ox), max(0, -oy), min(H, H - oy)
                    if x0 >= x1 or y0 >= y1: continue
                    ps = (slice(y0, y1), slice(x0, x1)); qs = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    x = -((_d2(c, ps, qs) * kc + _d2(N, ps, qs) * kn) + _d2(P, ps, qs) * kp)
                    sel = x >= t(-80.0)                     # False for NaN
                    if stats is not None: stats["cut"] += int((x < t(-80.0)).sum()); stats["taps"] += int(x.size)
                    e = np.zeros_like(x)
                    if sel.any(): e[sel] = expf(x[sel]) if t is f32 else np.exp(x[sel])
                    w = np.where(sel, t(TAP[dy + 2] * TAP[dx + 2]) * e, t(0.0))
                    use = sel & (w != 0)
                    sw[ps] = np.where(use, sw[ps] + w, sw[ps])
                    cq = c[qs]
                    for k in range(3):
                        acc[ps + (k,)] = np.where(use, acc[ps + (k,)] + np.where(use, w, t(0.0)) * np.where(use, cq[..., k], t(0.0)), acc[ps + (k,)])
            has = sw > 0
            c = np.where(has[..., None], acc / np.where(has, sw, t(1.0))[..., None], c)
            if stats is not None: stats["levels"].append((c * D if D is not None else c).astype(t))
        out = c * D if D is not None else c
    return out.astype(t), t(resolved)
