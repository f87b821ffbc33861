"""CPU: the NumPy model of the denoiser's temporal stage (tests/temporal_model.py; the definition is mi_denoise_image_temporal's comment in include/mi355pt.h) on its
own test sequence -- a pinhole panning past a back plane and a foreground rectangle that moves once.  The GPU tests (tests/test_gpu_temporal.py) compare the device
against this model bit for bit; here the sequence is shown to exercise every branch of the rule (accepted, rejected inside the frame, projected outside, non-finite)
and the model to follow the definition's consequences."""
import numpy as np
import pytest
from tests import denoise_model as dm
from tests import temporal_model as tm

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module", params=tm.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def seq(request):
    w, h = request.param; frames = tm.pan_sequence(w, h); census = []
    return dict(w=w, h=h, frames=frames, runs=tm.run_sequence(frames, census=census, iterations=2), census=census)


def test_census_of_the_pan_sequence(seq):
    """Conditions on the inputs, asserted on the model alone: on every frame >= 1 at least 0.85 of the pixels accept history, at least 0.01 are rejected inside the
    frame (disocclusion next to the foreground, and behind it once it moves), and on the panning frames 1, 2 and 4 at least 0.02 project outside the previous
    frame.  A float64 prototype of the rule gave 0.91 - 0.96, 0.014 - 0.089 and 0.022 - 0.030."""
    for k, st in enumerate(seq["census"]):
        acc, rej, out = (float(st[key].mean()) for key in ("accepted", "rejected", "outside"))
        print(f"[temporal model] {seq['w']} x {seq['h']} frame {k}: accepted {acc:.3f}, rejected inside {rej:.3f}, outside {out:.3f}, alone {float(st['alone'].mean()):.3f}")
        if k == 0:
            assert st["alone"].all() and acc == rej == out == 0
            continue
        assert acc >= 0.85 and rej >= 0.01, (k, acc, rej)
        if k in tm.PANNING: assert out >= 0.02, (k, out)
        assert (st["accepted"].astype(int) + st["rejected"] + st["outside"] + st["alone"] == 1).all()      # the four cases partition the image


def test_frame_0_equals_the_spatial_filter(seq):
    """the first frame of a history is mi_denoise_image: same bits, with and without demodulation, and the history holds c0 with a count of 1"""
    fr = seq["frames"][0]
    for A in (fr["albedo"], None):
        out, res, tp, hist = tm.temporal_frame(None, fr["color"], fr["normal"], fr["position"], A, fr["prev_position"], fr["world_to_pixel"], iterations=3)
        exp, eres = dm.atrous(fr["color"], fr["normal"], fr["position"], A, iterations=3)
        assert (bits(out) == bits(exp)).all() and bits(res) == bits(eres)
        assert (hist["n"] == 1).all() and hist["frames"] == 1
        assert (bits(hist["a"]) == bits(fr["color"] / A if A is not None else fr["color"])).all()
        d = fr["position"].reshape(-1, 3).max(0) - fr["position"].reshape(-1, 3).min(0)
        assert abs(float(tp) - 0.01 * float(np.sqrt((d.astype(np.float64) ** 2).sum()))) <= 1e-6 * float(tp)


def test_planted_non_finite_pixels_stay_alone():
    """70 x 37, frame 2: the NaN colour, Inf colour and NaN normal pixels get n = 0 and keep their colour; in frame 3 no pixel inherits from them -- every count
    stays a number, every accumulated colour outside the planted places is finite, and the planted places themselves start again at n = 1."""
    frames = tm.pan_sequence(70, 37); runs = tm.run_sequence(frames, iterations=0); places = frames[2]["places"]
    h2, h3 = runs[2][3], runs[3][3]
    for p in places: assert h2["n"][p] == 0
    assert np.isnan(h2["a"][places[0]]).all() and np.isinf(h2["a"][places[1]]).any() and np.isfinite(h2["a"][places[2]]).all()
    bad = ~np.isfinite(h2["a"]).all(-1); exp = np.zeros_like(bad); exp[places[0]] = exp[places[1]] = True
    assert (bad == exp).all() and (h2["n"] > 0).sum() == 70 * 37 - 3
    assert np.isfinite(h3["a"]).all() and np.isfinite(h3["n"]).all() and (h3["n"] >= 1).all()
    # the pixels of frame 3 that look at a planted place with the whole bilinear weight lose their history; nobody's count came from n = 0
    assert (h3["n"] <= 4).all() and (h3["n"][h3["n"] > 1] >= 1.0).all()


def test_max_history_caps_the_count():
    """a static camera, eight frames: the count reaches max_history = 3 and stays; without the cap it is the frame number"""
    fr = tm.pan_sequence(33, 19)[0]; hist = None; free = None
    for k in range(8):
        _, _, _, hist = tm.temporal_frame(hist, fr["color"], fr["normal"], fr["position"], fr["albedo"], None, fr["world_to_pixel"], iterations=0, max_history=3.0)
        _, _, _, free = tm.temporal_frame(free, fr["color"], fr["normal"], fr["position"], fr["albedo"], None, fr["world_to_pixel"], iterations=0)
        assert (hist["n"] == min(k + 1, 3)).all() and (free["n"] == k + 1).all(), k


def test_constant_colour_is_returned_exactly():
    """hist + (c0 - hist) x alpha with c0 = hist is hist: a constant image accumulates to itself over the whole pan, bit for bit, whatever the taps' weights --
    wherever the bilinear mean of equal values is that value (s / sw with s = sum of b x v: exact when one tap counts; checked against 2 ulp otherwise)."""
    frames = tm.pan_sequence(45, 13); hist = None; v = f32([0.25, 0.5, 1.0])
    for fr in frames:
        C = np.broadcast_to(v, fr["color"].shape).astype(f32)
        out, _, _, hist = tm.temporal_frame(hist, C, fr["normal"], fr["position"], None, fr["prev_position"], fr["world_to_pixel"], iterations=0)
        assert (bits(out) == bits(hist["a"])).all()
        assert np.abs(hist["a"] - C).max() <= 2 * 2.0 ** -23
    # a static camera reprojects every pixel onto itself with weight 1: exact
    fr = frames[0]; hist = None
    for _ in range(4):
        out, _, _, hist = tm.temporal_frame(hist, C, fr["normal"], fr["position"], None, None, fr["world_to_pixel"], iterations=0)
        assert (bits(out) == bits(C)).all()
    assert (hist["n"] == 4).all()


def test_a_moved_surface_drops_its_history():
    """frame 3 without prev_position: the foreground moved 0.5 along x, more than tp (about 0.14 at 70 x 37).  The rectangle slides in its own plane, so where the new
    rectangle overlaps the old one a pixel still finds a record at its own world position (another point of the surface: the price of Pprev = P); the strip the
    old rectangle did not cover (x > 1.2 + tp) finds the back plane's records 5 units away and starts again at n = 1 with its own colour instead of ghosting.
    With prev_position the whole rectangle keeps its history."""
    frames = tm.pan_sequence(70, 37); runs = tm.run_sequence(frames[:3], iterations=0); hist = runs[2][3]; fr = frames[3]; fg = fr["foreground"]
    tp = float(runs[2][2]); assert tp < 0.5
    _, _, _, kept = tm.temporal_frame(hist, fr["color"], fr["normal"], fr["position"], fr["albedo"], fr["prev_position"], fr["world_to_pixel"], iterations=0)
    _, _, _, lost = tm.temporal_frame(hist, fr["color"], fr["normal"], fr["position"], fr["albedo"], None, fr["world_to_pixel"], iterations=0)
    strip = fg & (fr["position"][..., 0] > 1.2 + tp); assert strip.sum() >= 50
    assert (kept["n"][fg] > 1).mean() > 0.9 and (kept["n"][strip] > 1).mean() > 0.9 and (lost["n"][strip] == 1).all()
    assert (bits(lost["a"][strip]) == bits((fr["color"] / fr["albedo"])[strip])).all()
