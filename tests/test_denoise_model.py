"""CPU: the NumPy model of the edge-avoiding a-trous filter (tests/denoise_model.py; the definition is mi_denoise_image's comment in include/mi355pt.h) on a synthetic
input -- two planes that meet at an edge, a checkerboard albedo, gamma noise -- with K = 5 and the widths (4, 0.3, 0.5).  The GPU tests (tests/test_gpu_denoise.py)
compare the device against this model bit for bit; here the model itself is shown to be a denoiser and to follow the definition's edge rules."""
import numpy as np
import pytest
from tests import denoise_model as dm

f32 = np.float32
WIDTHS = dict(iterations=5, sigma_color=4.0, sigma_normal=0.3, sigma_position=0.5)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


@pytest.fixture(scope="module")
def syn():
    s = dm.synthetic()
    s["out"], _ = dm.atrous(s["color"], s["normal"], s["position"], s["albedo"], **WIDTHS)
    return s


def test_float32_against_float64(syn):
    """The float32 model against the same definition in float64: the largest relative difference is 6.8e-07 here (seed 1, glibc 2.35); the bound is 8 x that,
    5.5e-06.  The margin covers another libm or seed, not another algorithm."""
    o64, _ = dm.atrous(syn["color"], syn["normal"], syn["position"], syn["albedo"], dtype=np.float64, **WIDTHS)
    rel = float(np.max(np.abs(syn["out"] - o64) / np.abs(o64)))
    print(f"[denoise model] float32 vs float64: largest relative difference {rel:.3e}")
    assert rel <= 8 * 6.8e-07


def test_rmse_halves_and_demodulation_helps(syn):
    """RMSE to the noise-free image: at most half the input's (0.0255 against 0.2818 here, 0.09 of it); without demodulation it is larger (0.172): the filter then
    blurs the checkerboard."""
    raw = rmse(syn["color"], syn["clean"]); den = rmse(syn["out"], syn["clean"])
    plain, _ = dm.atrous(syn["color"], syn["normal"], syn["position"], None, **WIDTHS); nod = rmse(plain, syn["clean"])
    print(f"[denoise model] rmse raw {raw:.4f}, filtered {den:.4f} ({den / raw:.3f}), without demodulation {nod:.4f}")
    assert den <= 0.5 * raw
    assert nod > den


def test_edge_is_preserved(syn):
    """out / albedo = the filtered irradiance: 1.0 left of the edge, 0.3 right of it; the columns next to the edge stay within 10 % (1.004 and 0.286 here)."""
    q = syn["out"] / syn["albedo"]; e = syn["edge"]; left = float(q[:, e - 1].mean()); right = float(q[:, e].mean())
    print(f"[denoise model] irradiance at the edge: {left:.4f} | {right:.4f}")
    assert abs(left - 1.0) <= 0.10 * 1.0 and abs(right - 0.3) <= 0.10 * 0.3


def test_non_finite_pixels_stay_isolated(syn):
    """A NaN colour pixel and an Inf colour pixel stay non-finite, a pixel with a NaN normal keeps its input value, every other pixel is finite."""
    c, (p_nan, p_inf, p_nrm) = dm.plant_non_finite(syn)
    out, _ = dm.atrous(c["color"], c["normal"], c["position"], c["albedo"], **WIDTHS)
    bad = ~np.isfinite(out).all(-1); exp = np.zeros_like(bad); exp[p_nan] = exp[p_inf] = True
    assert (bad == exp).all(), np.argwhere(bad != exp)
    # (C / D) x D is the input up to the two roundings
    assert np.allclose(out[p_nrm], c["color"][p_nrm], rtol=4 * 2.0 ** -24, atol=0)
    plain, _ = dm.atrous(c["color"], c["normal"], c["position"], None, **WIDTHS)
    assert (bits(plain[p_nrm]) == bits(c["color"][p_nrm])).all()


def test_zero_iterations_return_the_input(syn):
    out, res = dm.atrous(syn["color"], syn["normal"], syn["position"], syn["albedo"], iterations=0, sigma_color=4.0, sigma_normal=0.3, sigma_position=0.5)
    assert (bits(out) == bits(syn["color"])).all() and res == f32(0.5)


@pytest.mark.parametrize("w,h", [(1, 1), (2, 3), (3, 2), (5, 17), (17, 5)])
def test_tiny_images(w, h):
    """K = 8 on images smaller than the steps: finite, and every channel a weighted mean of its inputs -- within [min, max] up to the roundings of the sums and the
    division.  Slack: 4 ulp; observed 1 ulp (the 1 x 1 image: (9/64 c) / (9/64) is one ulp under c in one channel)."""
    c = dm.random_case(w, h, 5)
    out, _ = dm.atrous(c["color"], c["normal"], c["position"], None, iterations=8, sigma_color=4.0, sigma_normal=0.3, sigma_position=0.5)
    assert out.shape == (h, w, 3) and np.isfinite(out).all()
    for k in range(3):
        lo, hi = c["color"][..., k].min(), c["color"][..., k].max(); slack = 4 * 2.0 ** -23
        under = max(0.0, float((lo - out[..., k].min()) / lo)); over = max(0.0, float((out[..., k].max() - hi) / hi))
        print(f"[denoise model] {w} x {h} channel {k}: {under / 2.0 ** -23:.2f} ulp under the minimum, {over / 2.0 ** -23:.2f} ulp over the maximum")
        assert under <= slack and over <= slack


def test_automatic_position_width(syn):
    """sigma_position < 0: |sigma_position| x the diagonal of the finite positions' box, against a float64 computation; 0 (term off) when no position is finite or
    the box is a point."""
    P = syn["position"].copy(); P[3, 4] = np.nan; P[9, 9, 2] = np.inf       # not part of the box
    ok = np.isfinite(P).all(-1); d = P[ok].astype(np.float64).max(0) - P[ok].astype(np.float64).min(0); exp = 0.05 * float(np.sqrt((d * d).sum()))
    _, res = dm.atrous(syn["color"], syn["normal"], P, syn["albedo"], iterations=1, sigma_color=4.0, sigma_normal=0.3, sigma_position=-0.05)
    assert res.dtype == f32 and abs(float(res) - exp) <= 4 * 2.0 ** -24 * exp, (res, exp)
    out, res = dm.atrous(syn["color"], syn["normal"], np.full_like(P, np.nan), syn["albedo"], iterations=2, sigma_color=4.0, sigma_normal=0.3, sigma_position=-0.05)
    assert res == 0
    # kp = 0 times a NaN distance is NaN: every tap is dropped and the image keeps its values
    assert (bits(out) == bits((syn["color"] / syn["albedo"]) * syn["albedo"])).all()
    _, res = dm.atrous(syn["color"], syn["normal"], np.ones_like(P), syn["albedo"], iterations=1, sigma_color=4.0, sigma_normal=0.3, sigma_position=-0.05)
    assert res == 0


@pytest.mark.parametrize("w,h", dm.GPU_SIZES)
def test_device_comparison_cases_are_not_vacuous(w, h):
    """The random cases tests/test_gpu_denoise.py feeds the device: after every iteration count it uses the model's output differs from the input in more than 90 %
    of the finite pixels (a single pixel has nothing to mix with), and taps across the planted position edge fall under the -80 cut wherever the image is wide
    enough to hold the edge."""
    c = dm.random_case(w, h, seed=100 + w)
    if (w, h) == (70, 37): c, _ = dm.plant_non_finite(c)
    for A in (c["albedo"], None):
        for sp in (0.5, -0.05):
            st = {}; dm.atrous(c["color"], c["normal"], c["position"], A, iterations=8, sigma_color=4.0, sigma_normal=0.3, sigma_position=sp, stats=st)
            fin = np.isfinite(c["color"]).all(-1)
            for k in dm.GPU_ITERATIONS:
                moved = float((bits(st["levels"][k - 1]) != bits(c["color"])).any(-1)[fin].mean())
                if (w, h) != (1, 1): assert moved > 0.90, (k, moved)
            if w >= 3: assert st["cut"] > 0
