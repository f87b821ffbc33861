"""The film stage restated in numpy, one sample at a time (ImageBlock::put, include/mitsuba/render/imageblock.h:161-221; the reference's adaptive.cpp:307-317 for the
adaptive film; src/libcore/bitmap.cpp:1621-1625 for the develop).  No device code is used here: the weights come from the oracle's discretized filter table
(adaptive_model.filter_table), the float32 sequential film itself from oracle.Oracle.film_put_units.

  put64       float64 sums of float32 weights, with the magnitude and the number of contributions per cell: what a sum in ANY order is bounded against
  adaptive32  k_adapt_accumulate's arithmetic: per pixel the footprint rows as float32 chains in sample order, cut to own +- hb, scaled by f32(1 / n) at the stop
  develop32   f32(sum * f32(1 / w)), the reciprocal zero where w == 0
"""
import numpy as np

f32 = np.float32
REJECT_CAUSES = ("nan", "inf", "negative", "nan_alpha", "negative_alpha")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def film_coord(p, border):
    """sample position -> the block's continuous cell coordinate: (p - 0.5f) - (float) (0 - border), two float32 roundings"""
    return f32(f32(f32(p) - f32(0.5)) + f32(border))


def span(pos, rad, n):
    """the cells ceil(pos - r) .. floor(pos + r) cut to 0 .. n - 1 (empty: lo > hi)"""
    return max(int(np.ceil(f32(pos - rad))), 0), min(int(np.floor(f32(pos + rad))), n - 1)


def accepted(val4):
    """ImageBlock::put's check on Li rgb and alpha (the weight 1 always passes): every value finite and >= 0"""
    v = np.asarray(val4, f32)
    with np.errstate(invalid="ignore"):
        return (np.isfinite(v) & (v >= 0)).all(-1)


def footprint(ev, rad, border, width, height, sx, sy, own=None, hb=0):
    """(x0, x1, y0, y1, wx [x1 - x0 + 1], wy [...]) of one sample: the cell range cut to the film (and, with `own` = the (x, y) of a cell incl. border, to own +- hb as
    k_adapt_accumulate cuts it) and the float32 table weights per column and row"""
    W, H = width + 2 * border, height + 2 * border
    posx, posy = film_coord(sx, border), film_coord(sy, border)
    x0, x1 = span(posx, rad, W); y0, y1 = span(posy, rad, H)
    if own is not None:
        x0 = max(x0, own[0] - hb); x1 = min(x1, own[0] + hb); y0 = max(y0, own[1] - hb); y1 = min(y1, own[1] + hb)
    wx = np.array([ev(f32(x) - posx) for x in range(x0, x1 + 1)], f32); wy = np.array([ev(f32(y) - posy) for y in range(y0, y1 + 1)], f32)
    return x0, x1, y0, y1, wx, wy


def put64(ev, rad, border, width, height, pos2, vals, reject=False):
    """Every sample i (pos2 [n, 2], vals [n, nch]) put as ImageBlock::put does, weight w = f32(f32(wx) * f32(wy)), sums in float64.  reject: the put's check on the
    values.  Returns (H + 2b) x (W + 2b) x (nch + 1) sums (the weight plane last: v = 1), the same shape of sum |w v|, and the contributions per cell (H + 2b) x (W + 2b)."""
    pos2 = np.asarray(pos2, f32).reshape(-1, 2); vals = np.asarray(vals).reshape(len(pos2), -1); nch = vals.shape[1] + 1
    W, H = width + 2 * border, height + 2 * border
    exp = np.zeros((H, W, nch)); mag = np.zeros((H, W, nch)); cnt = np.zeros((H, W), np.int64)
    ok = accepted(vals) if reject else np.ones(len(pos2), bool)
    for i in np.flatnonzero(ok):
        x0, x1, y0, y1, wx, wy = footprint(ev, rad, border, width, height, pos2[i, 0], pos2[i, 1])
        if x0 > x1 or y0 > y1: continue
        w = (wy[:, None] * wx[None, :]).astype(f32).astype(np.float64)[..., None]      # f32(wx * wy): the product the kernels and the reference form
        v = np.concatenate([vals[i].astype(np.float64), [1.0]])
        exp[y0:y1 + 1, x0:x1 + 1] += w * v; mag[y0:y1 + 1, x0:x1 + 1] += np.abs(w * v); cnt[y0:y1 + 1, x0:x1 + 1] += 1
    return exp, mag, cnt


def thread_cells(ev, rad, border, width, height, pos2, vals, owner, reject=True):
    """per film cell (H + 2b) x (W + 2b): the set of `owner` values (one per sample: the thread that puts it) whose samples touch the cell, as a list of sets"""
    pos2 = np.asarray(pos2, f32).reshape(-1, 2); vals = np.asarray(vals).reshape(len(pos2), -1)
    W, H = width + 2 * border, height + 2 * border
    cells = [[set() for _ in range(W)] for _ in range(H)]
    ok = accepted(vals) if reject else np.ones(len(pos2), bool)
    for i in np.flatnonzero(ok):
        x0, x1, y0, y1, _, _ = footprint(ev, rad, border, width, height, pos2[i, 0], pos2[i, 1])
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1): cells[y][x].add(int(owner[i]))
    return cells


def adaptive32(ev, rad, border, width, height, pixels, pos, val4, n):
    """k_adapt_accumulate.  pixels [P, 2] film pixels (px, py), pos [P, K, 2], val4 [P, K, 4] their samples in order, n [P] the samples each takes
    (adaptive_model.counts).  Per pixel: footprint rows of (2 hb + 1)^2 cells x 5 values {R, G, B, alpha, weight}, hb = floor(radius + 0.5); an accepted sample k < n adds
    f = f32(f + f32(w * v)) to the cells of its footprint cut to the film AND to own +- hb; a rejected one adds nothing.  At the stop every footprint cell inside the film
    contributes c = f32(f * f32(1 / n)).  Returns the float32 film of ONE contribution per cell ((H + 2b) x (W + 2b) x 5, exact where no two pixels share a cell) and, per
    film cell (y, x), the list of the contributions [5] it receives, zeros included, in pixel order."""
    hb = int(np.floor(f32(rad) + f32(0.5))); side = 2 * hb + 1
    W, H = width + 2 * border, height + 2 * border
    film = np.zeros((H, W, 5), f32); contrib = {}
    ok = accepted(val4)
    for i in range(len(pixels)):
        ox, oy = int(pixels[i][0]) + border, int(pixels[i][1]) + border
        fp = np.zeros((side, side, 5), f32)
        for k in range(int(n[i])):
            if not ok[i, k]: continue
            x0, x1, y0, y1, wx, wy = footprint(ev, rad, border, width, height, pos[i, k, 0], pos[i, k, 1], own=(ox, oy), hb=hb)
            if x0 > x1 or y0 > y1: continue
            w = (wy[:, None] * wx[None, :]).astype(f32)[..., None]
            v = np.array([val4[i, k, 0], val4[i, k, 1], val4[i, k, 2], val4[i, k, 3], 1.0], f32)
            cy, cx = y0 - oy + hb, x0 - ox + hb
            fp[cy:cy + (y1 - y0 + 1), cx:cx + (x1 - x0 + 1)] += (w * v).astype(f32)
        inv = f32(f32(1) / f32(int(n[i])))
        for dy in range(-hb, hb + 1):
            for dx in range(-hb, hb + 1):
                x, y = ox + dx, oy + dy
                if x < 0 or y < 0 or x >= W or y >= H: continue
                c = (fp[dy + hb, dx + hb] * inv).astype(f32)
                contrib.setdefault((y, x), []).append(c); film[y, x] = film[y, x] + c
    return film, contrib


def contribution_sums(contrib, shape):
    """float64 sum, sum of magnitudes and number of the NONZERO contributions per cell and value (a zero is not added by the kernel's spill, and adds nothing)"""
    tot = np.zeros(shape); mag = np.zeros(shape); num = np.zeros(shape, np.int64)
    for (y, x), cs in contrib.items():
        a = np.asarray(cs, np.float64); tot[y, x] = a.sum(0); mag[y, x] = np.abs(a).sum(0); num[y, x] = (a != 0).sum(0)
    return tot, mag, num


def inner(raw, border):
    return raw[border:raw.shape[0] - border, border:raw.shape[1] - border] if border else raw


def develop32(raw_inner):
    """The reference's develop of a multichannel (and of the 5-channel) film, src/libcore/bitmap.cpp:1621-1625: invWeight = weight == 0 ? 0 : 1 / weight, value * invWeight --
    f32(sum * f32(1 / w)) per value plane, the weight plane (last) dropped.  Where w == 0 the factor is 0: a finite sum develops to 0 (a non-finite one to NaN, as the
    reference's product does)."""
    raw_inner = np.asarray(raw_inner, f32); w = raw_inner[..., -1:]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(w != 0, f32(1) / w, f32(0)).astype(f32)
        return (raw_inner[..., :-1] * inv).astype(f32)
