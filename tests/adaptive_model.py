"""The adaptive stopping rule (include/mi355pt.h; the reference's src/integrators/misc/adaptive.cpp:202-319) restated in numpy float32, one operation per rounding,
and a film model with float64 sums.  The inputs are per-sample radiance values (and film positions): from oracle.Oracle.render_samples, or on the GPU from
Render.samples, which the parity tests pin to the oracle bit for bit.  No device code is used here."""
import ctypes as C
import math

import numpy as np

f32 = np.float32
LAST_INDEX = (1 << 24) - 1            # last sample index of the independent stream: the luminance estimate's, never a render's
SQRT_TWO = f32(1.41421356237309504880)


def approx_erfinv(x):
    """adaptive.cpp:26-60 in float32.  The logarithm is the correctly rounded one (test_adaptive_model pins it to the C library's logf at the arguments used)."""
    x = f32(x); one = f32(1)
    w = f32(-f32(math.log(float(f32(f32(one - x) * f32(one + x))))))
    if w < f32(5):
        w = f32(w - f32(2.5))
        coef = [2.81022636e-08, 3.43273939e-07, -3.5233877e-06, -4.39150654e-06, 0.00021858087, -0.00125372503, -0.00417768164, 0.246640727, 1.50140941]
    else:
        w = f32(f32(np.sqrt(w)) - f32(3))
        coef = [-0.000200214257, 0.000100950558, 0.00134934322, -0.00367342844, 0.00573950773, -0.0076224613, 0.00943887047, 1.00167406, 2.83297682]
    p = f32(coef[0])
    for c in coef[1:]:
        p = f32(f32(c) + f32(p * w))
    return f32(p * x)


def raw_quantile(p_value):
    """what the reference computes: approx_erfinv(-1 + pValue) * SQRT_TWO -- negative for every pValue in (0, 1)"""
    return f32(approx_erfinv(f32(f32(-1) + f32(p_value))) * SQRT_TWO)


def quantile(p_value):
    """what is built: the absolute value of the polynomial, times SQRT_TWO (the quantile of 1 - p / 2 the reference's comment at :192-195 means)"""
    return f32(f32(abs(approx_erfinv(f32(f32(-1) + f32(p_value))))) * SQRT_TWO)


def luminance(li):
    li = np.asarray(li, f32)
    return (li[..., 0] * f32(0.212671) + li[..., 1] * f32(0.715160)) + li[..., 2] * f32(0.072169)


def accepted(li):
    """ImageBlock::put's / k_film's rejection on the radiance (alpha and weight are 1 or 0: never rejected)"""
    li = np.asarray(li, f32)
    return (np.isfinite(li) & (li >= 0)).all(-1)


def sample_pairs(pixels, k0, k1):
    """(px, py, k) for every pixel of `pixels` [n, 2] and k in [k0, k1): pixel-major"""
    pixels = np.asarray(pixels, np.uint32).reshape(-1, 2); ks = np.arange(k0, k1, dtype=np.uint32)
    return np.concatenate([np.repeat(pixels, len(ks), 0), np.tile(ks, len(pixels))[:, None]], 1)


def tile_pixels(x0, y0, x1, y1):
    yy, xx = np.meshgrid(np.arange(y0, y1), np.arange(x0, x1), indexing="ij")
    return np.stack([xx.ravel(), yy.ravel()], 1).astype(np.uint32)


def counts(li, spp, max_error, average_luminance, max_sample_factor=32, p_value=0.05):
    """li [n_pixels, K, 3]: sample k of every pixel, K >= the samples any pixel needs (K = max_sample_factor x spp when there is a cap).  Returns the samples each pixel
    takes (uint32 [n_pixels]); a pixel that has not stopped after K samples raises."""
    li = np.asarray(li, f32); P, K = li.shape[:2]
    cap = max_sample_factor * spp if max_sample_factor > 0 else LAST_INDEX - 1
    ok = accepted(li); lum_all = np.where(ok, luminance(li), f32(0)).astype(f32)
    q = quantile(p_value); floor = f32(f32(average_luminance) * f32(0.01)); me = f32(max_error)
    mean = np.zeros(P, f32); msq = np.zeros(P, f32); out = np.zeros(P, np.uint32); live = np.ones(P, bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(K):
            n = k + 1; nf = f32(n); lum = lum_all[:, k]
            delta = lum - mean
            mean = np.where(live, mean + delta / nf, mean).astype(f32)
            msq = np.where(live, msq + delta * (lum - mean), msq).astype(f32)
            stop = np.full(P, n >= cap)
            if n >= spp and n < cap:
                variance = msq / f32(n - 1)
                std_error = np.sqrt(variance / nf)
                ci_width = std_error * q
                base = np.maximum(mean, floor)
                stop = ci_width <= me * base
            stop &= live
            out[stop] = n; live &= ~stop
            if not live.any():
                break
    if live.any():
        raise ValueError(f"{int(live.sum())} pixels have not stopped after {K} samples")
    return out


def filter_table(oracle, orc):
    """(eval(x) -> float32 weight, radius float32, border) of the oracle's discretized reconstruction filter"""
    olib = oracle.lib(); table = np.zeros(32, f32); radius = C.c_float(); border = C.c_int()
    olib.orc_filter_table(orc.h, table.ctypes.data, C.byref(radius), C.byref(border))
    return (lambda x: f32(olib.orc_filter_eval_discretized(orc.h, float(f32(x))))), f32(radius.value), border.value


def film(oracle, orc, width, height, pixels, li, pos, n):
    """The adaptive film in float64: for pixel i of `pixels` its first n[i] samples (li [n_pixels, K, 3], pos [n_pixels, K, 2]) put as ImageBlock::put does (footprint
    ceil / floor on pos - 0.5 + border, weight filter(x) * filter(y) in float32), the pixel's whole footprint scaled by 1 / n[i].  Returns (H + 2b) x (W + 2b) x 5
    sums {R, G, B, alpha, weight}; alpha is put as 1 (a closed scene) and not meant to be compared elsewhere."""
    ev, rad, b = filter_table(oracle, orc); W, H = width + 2 * b, height + 2 * b
    out = np.zeros((H, W, 5)); ok = accepted(li)
    for i in range(len(pixels)):
        inv = 1.0 / float(n[i])
        for k in range(int(n[i])):
            if not ok[i, k]: continue
            posx = f32(f32(pos[i, k, 0] - f32(0.5)) + f32(b)); posy = f32(f32(pos[i, k, 1] - f32(0.5)) + f32(b))
            x0 = max(int(np.ceil(f32(posx - rad))), 0); x1 = min(int(np.floor(f32(posx + rad))), W - 1)
            y0 = max(int(np.ceil(f32(posy - rad))), 0); y1 = min(int(np.floor(f32(posy + rad))), H - 1)
            v = np.array([li[i, k, 0], li[i, k, 1], li[i, k, 2], 1.0, 1.0], np.float64)
            for y in range(y0, y1 + 1):
                wy = ev(f32(y) - posy)
                for x in range(x0, x1 + 1):
                    out[y, x] += float(f32(ev(f32(x) - posx) * wy)) * inv * v
    return out


def develop(film5, border):
    """sum / weight of the inner pixels (hdrfilm.cpp:352,396)"""
    b = border; inner = film5[b:film5.shape[0] - b, b:film5.shape[1] - b] if b else film5
    w = inner[..., 4:5]
    return np.where(w != 0, inner[..., :3] / np.where(w != 0, w, 1), 0.0)


def luminance_estimate_pairs(width, height):
    """the (px, py, 2^24 - 1) triples of the average-luminance estimate: N = min(10000, W H) pixels p_i = (i W H) // N"""
    wh = width * height; n = min(10000, wh); p = (np.arange(n, dtype=np.int64) * wh) // n
    return np.stack([p % width, p // width, np.full(n, LAST_INDEX)], 1).astype(np.uint32)


def luminance_estimate(li):
    """float64 sum of the float32 luminances in index order, over N, cast to float32"""
    lum = luminance(li); s = 0.0
    for v in lum.tolist():
        s += v
    return f32(s / len(lum))


def oracle_samples(oracle, sc, pixels, k1):
    """(li [n_pixels, k1, 3], pos [n_pixels, k1, 2]) of samples 0 .. k1 - 1 of every pixel, from the CPU oracle"""
    got = oracle.Oracle(sc).render_samples(sample_pairs(pixels, 0, k1))
    return got["li"].reshape(len(pixels), k1, 3), got["pos"].reshape(len(pixels), k1, 2)


def device_samples(render, pixels, k1):
    """li [n_pixels, k1, 3] of samples 0 .. k1 - 1 of every pixel, from Render.samples"""
    return render.samples(sample_pairs(pixels, 0, k1)).reshape(len(pixels), k1, 3)
