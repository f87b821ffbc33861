"""Inputs of the film-unit tests (tests/test_gpu_film_units.py; checked on the CPU by tests/test_film_inputs.py): samples placed by hand on a 22 x 15 film, the positions a
camera almost never produces -- pixel corners and centres, px + 1 exactly, 1e-5 from an edge, across the film's edges, far outside -- and values the scenes never
produce: NaN, infinite and negative radiance or alpha.  Pure numpy, fixed seeds.

A layout is (pos [K, 330, 2], val [K, 330, 4]): plane-major, the tile pixel pl = y * 22 + x minor, as the kernels index q.pos / q.acc.

  isolated  12 active pixels, x in {0, 7, 14, 21}, y in {0, 7, 14}, 16 planes inside (or on the edge of) the own pixel; every other pixel carries rejected values.
            hb = floor(radius + 0.5) <= 3 cells, so 7 pixels apart no two footprints meet even at px + 0 and px + 1: every film cell belongs to ONE thread
  single    one active pixel (10, 7) whose 48 samples lie anywhere: in other pixels, across the four edges and corners, outside by more than the radius, at +-2^20
  dense     every pixel, 8 planes: 80 % inside the own pixel (random and the edge fractions), 15 % up to 3 pixels away, 5 % rejected values
"""
import numpy as np

f32 = np.float32
W, H = 22, 15
N_PIX = W * H
FILTER_NAMES = ["box", "gaussian", "tent", "mitchell", "catmullrom", "lanczos"]      # = scenes.FILTER_* 0..5: box 0.5, gaussian sigma 0.5, tent, mitchell 1/3 1/3, catmullrom, lanczos 3
ACTIVE_X, ACTIVE_Y = (0, 7, 14, 21), (0, 7, 14)
EDGE_FRACTIONS = np.array([0.0, 0.5, 1.0, 5e-6, 1 - 5e-6, 1e-5, 1.5e-5, 0.25, 0.999999], f32)
REJECT_CAUSES = ("nan", "inf", "negative", "nan_alpha", "negative_alpha")
SINGLE_PIXEL = (10, 7)
AVERAGE_LUMINANCE = 1.0


def scene(S, kind):
    """the 22 x 15 film behind filter `kind` (the Cornell box: the film units never trace it), independent sampler, 8 spp -- what mi_render_set_adaptive asks for"""
    return S.cornell_box(W, H, 8, sampler=S.SAMPLER_INDEPENDENT, filter_kind=kind)


def rejected_value(cause, rng):
    """Li rgb + alpha that ImageBlock::put refuses for `cause`, the other values ordinary"""
    v = np.concatenate([np.exp2(rng.uniform(-3, 3, 3)), [1.0]]).astype(f32); c = REJECT_CAUSES[cause % 5]; ch = int(rng.integers(0, 3))
    if c == "nan": v[ch] = np.nan
    elif c == "inf": v[ch] = np.inf
    elif c == "negative": v[ch] = -1.0
    elif c == "nan_alpha": v[3] = np.nan
    else: v[3] = -0.5
    return v


def reject_cause(val):
    """index into REJECT_CAUSES per sample, -1 = accepted (the first cause in the order of the list)"""
    v = np.asarray(val, f32); out = np.full(v.shape[:-1], -1, np.int64); rgb, a = v[..., :3], v[..., 3]
    with np.errstate(invalid="ignore"):
        for i, m in reversed(list(enumerate([np.isnan(rgb).any(-1), np.isinf(rgb).any(-1), (rgb < 0).any(-1), np.isnan(a), a < 0]))): out[m] = i
    return out


def ordinary_values(rng, n, spread=10.0, base=1.0):
    """n x 4: rgb = base x 2^U(-spread, spread) clipped to [2^-10, 2^10] (no denormal product with a filter weight), alpha out of {0, 0.5, 1}"""
    rgb = np.clip(base * np.exp2(rng.uniform(-spread, spread, (n, 3))), 2.0 ** -10, 2.0 ** 10)
    return np.concatenate([rgb, rng.choice([0.0, 0.5, 1.0], (n, 1))], 1).astype(f32)


def active_pixels():
    return [(x, y) for y in ACTIVE_Y for x in ACTIVE_X]


def isolated(seed=1, inactive="inside"):
    """-> pos [16, 330, 2], val [16, 330, 4], active [330] bool.  Active pixel j, plane s: position (px + f, py + g) in float32, f and g walking EDGE_FRACTIONS with
    different strides (planes 0..11) and random (12..15); its values are near-constant (j % 3 == 0), moderately spread (1) or spread over the whole range (2), so that an
    adaptive run with max_error 0.2 ends at spp, in between and at the cap; two of its planes carry rejected values (late ones where j % 3 == 0).  Every other pixel:
    rejected values, the causes in rotation, at a random position inside the own pixel -- or, inactive="outside", 64 pixels off the film, for the field kernel, which has no
    check: there only the active pixels' threads put."""
    rng = np.random.default_rng(seed); K = 16
    pos = np.zeros((K, N_PIX, 2), f32); val = np.zeros((K, N_PIX, 4), f32); active = np.zeros(N_PIX, bool)
    yy, xx = np.divmod(np.arange(N_PIX), W); cause = 0
    for pl in range(N_PIX):
        for s in range(K):
            pos[s, pl] = (xx[pl] + rng.uniform(0.05, 0.95), yy[pl] + rng.uniform(0.05, 0.95))
            if inactive != "inside": pos[s, pl] = (-64.0 - xx[pl], -64.0 - yy[pl])
            val[s, pl] = rejected_value(cause, rng); cause += 1
    E = EDGE_FRACTIONS; n = len(E)
    for j, (px, py) in enumerate(active_pixels()):
        pl = py * W + px; active[pl] = True
        cls = j % 3
        v = ordinary_values(rng, K, spread=(0.05, 1.3, 10.0)[cls], base=float(np.exp2(rng.uniform(-4, 4))) if cls < 2 else 1.0)
        bad = (9 + j % 2, 13 + j % 3) if cls == 0 else (12 + j % 2, 14 + j % 2) if cls == 1 else (2 + j % 5, 8 + j % 7)
        for s in range(K):
            f = E[(s + j) % n] if s < 12 else f32(rng.uniform(0, 1)); g = E[(2 * s + 3 * j + 1) % n] if s < 12 else f32(rng.uniform(0, 1))
            if s == 12: g = E[j % n]           # a random f against an edge g, and the other way round
            if s == 13: f = E[(j + 4) % n]
            pos[s, pl] = (f32(px) + f32(f), f32(py) + f32(g))
            val[s, pl] = rejected_value(j + s, rng) if s in bad else v[s]
    return pos, val, active


def single(seed=2, planes=48):
    """-> pos [48, 330, 2], val [48, 330, 4], active [330].  The one active pixel's samples: 12 inside other pixels anywhere on the film, 16 off the four edges and corners by
    0.75 .. 2.5 cells (the footprint is cut at 0 and at W - 1 / H - 1), 8 outside the film by 4 .. 40 cells (empty footprint under every filter), 4 at +-2^20, 8 at the edge fractions of the film's
    own corners.  Accepted values; every other pixel carries rejected values at its own centre."""
    rng = np.random.default_rng(seed)
    pos = np.zeros((planes, N_PIX, 2), f32); val = np.zeros((planes, N_PIX, 4), f32); active = np.zeros(N_PIX, bool)
    yy, xx = np.divmod(np.arange(N_PIX), W)
    pos[:, :, 0] = xx[None] + 0.5; pos[:, :, 1] = yy[None] + 0.5
    for pl in range(N_PIX):
        for s in range(planes): val[s, pl] = rejected_value(pl + s, rng)
    pl = SINGLE_PIXEL[1] * W + SINGLE_PIXEL[0]; active[pl] = True
    cx, cy = SINGLE_PIXEL[0] + 0.5, SINGLE_PIXEL[1] + 0.5      # four in the pixels next to the own one (the narrow filters' own +- 1 cells), eight anywhere
    pts = [(cx + dx + rng.uniform(-0.4, 0.4), cy + dy + rng.uniform(-0.4, 0.4)) for dx, dy in ((-1, -1), (1, 1), (-1, 0), (0, 1))]
    pts += [(rng.uniform(0, W), rng.uniform(0, H)) for _ in range(8)]
    # d cells outside an edge.  d = 1 exactly is the one position at which the box filter's footprint is cut by the film's edge and not empty (its border is one cell, its
    # radius 0.5 + 1e-5); the wider filters are cut from d = 0.5 to their radius + 0.5
    lo = lambda d: -d
    for d in (1.0, 0.75):
        pts += [(lo(d), rng.uniform(0, H)), (W + d, rng.uniform(0, H)), (rng.uniform(0, W), lo(d)), (rng.uniform(0, W), H + d)]
    for dx, dy in ((1.0, 1.0), (1.5, 2.5)):
        pts += [(lo(dx), lo(dy)), (W + dx, lo(dy)), (lo(dx), H + dy), (W + dx, H + dy)]
    far = lambda n: (lambda t: -t if rng.integers(0, 2) else n + t)(rng.uniform(4.0, 40.0))
    for k in range(8):
        pts.append([(far(W), rng.uniform(0, H)), (rng.uniform(0, W), far(H)), (far(W), far(H)), (far(W), far(H))][k % 4])
    big = 2.0 ** 20
    pts += [(big, 7.5), (-big, 7.5), (10.5, big), (-big, -big)]
    E = EDGE_FRACTIONS
    pts += [(E[k] if k % 2 else W - 1 + E[k], E[8 - k] if k % 4 < 2 else H - 1 + E[8 - k]) for k in range(8)]
    assert len(pts) == planes
    pos[:, pl] = np.asarray(pts, np.float64).astype(f32); val[:, pl] = ordinary_values(rng, planes)
    return pos, val, active


def dense(seed=3, planes=8):
    """-> pos [8, 330, 2], val [8, 330, 4].  Per sample: 80 % inside the own pixel (half of them random, half an edge fraction per axis), 15 % displaced by up to +-3
    pixels (on the film's edge pixels every other one of these exactly one cell outside the edge), 5 % rejected values."""
    rng = np.random.default_rng(seed)
    yy, xx = np.divmod(np.arange(N_PIX), W); n = planes * N_PIX
    f = np.where(rng.random((n, 2)) < 0.5, rng.random((n, 2)), EDGE_FRACTIONS[rng.integers(0, len(EDGE_FRACTIONS), (n, 2))].astype(np.float64))
    u = rng.random(n); away = (u >= 0.80) & (u < 0.95); f[away] += rng.uniform(-3, 3, (int(away.sum()), 2))
    own = np.stack([np.tile(xx, planes), np.tile(yy, planes)], 1).astype(f32)
    pos = (own + f.astype(f32)).astype(f32)
    # every other displaced sample of a pixel on the film's edge goes exactly one cell outside that edge: where every filter's footprint, the box filter's included, is
    # cut by the film and not empty (single(), above)
    snap = away & (rng.random(n) < 0.5)
    for axis, size in ((0, W), (1, H)):
        pos[snap & (own[:, axis] == 0), axis] = -1.0; pos[snap & (own[:, axis] == size - 1), axis] = size + 1.0
    pos = pos.reshape(planes, N_PIX, 2)
    val = ordinary_values(rng, n).reshape(planes, N_PIX, 4)
    for i in np.flatnonzero(u >= 0.95): val.reshape(-1, 4)[i] = rejected_value(int(i), rng)
    return pos, val


def by_pixel(a):
    """[K, n_pix, c] plane-major -> [n_pix, K, c]"""
    return np.ascontiguousarray(np.swapaxes(a, 0, 1))


def flat(pos, val):
    """sample order of a sequential put that equals every thread's own order: pixel by pixel, each pixel's planes in order"""
    return by_pixel(pos).reshape(-1, 2), by_pixel(val).reshape(-1, val.shape[-1])
