"""GPU (MI355X): the temporal stage of the denoiser (mi_denoise_image_temporal / mi_render_denoise_temporal, include/mi355pt.h; csrc/kernels_temporal.hip) against the
NumPy model of its definition (tests/temporal_model.py): bit for bit at the image level over the model's own pan sequence, reset, the render level against the image
level on the render's own developed films, the scene's projection, what the history buys on a static scene and drops on a turned one, the refusals, the device
output, and the command line."""
import importlib
import os
import subprocess
import sys
import numpy as np
import pytest
from tests import denoise_model as dm
from tests import temporal_model as tm
from tests.conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
f32 = np.float32
WG = 256            # k_tp_accumulate's block (one thread per pixel): 45 x 13 = 585 pixels is two blocks and a fraction
GUIDES = [("shNormal", 0.0), ("position", 0.0), "albedo"]
GPU_SIZES = ((1, 1), (3, 2), (33, 19), (45, 13), (70, 37))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(got, exp):
    """equal bits wherever the expectation is a number, NaN exactly where it is NaN"""
    got = np.asarray(got, f32); exp = np.asarray(exp, f32); nan = np.isnan(exp)
    return (np.isnan(got) == nan).all() and (bits(got)[~nan] == bits(exp)[~nan]).all()


_SEQ = {}


def sequence(w, h):
    if (w, h) not in _SEQ: _SEQ[(w, h)] = tm.pan_sequence(w, h)
    return _SEQ[(w, h)]


# ---------------------------------------------------------------------------------------------- 1: image level
@pytest.mark.parametrize("iterations", [0, 2])
@pytest.mark.parametrize("with_albedo", [True, False])
@pytest.mark.parametrize("w,h", GPU_SIZES)
def test_image_level_equals_the_model(mi, w, h, with_albedo, iterations):
    """Every frame of the pan sequence: the output, the history's accumulated colour and count and both resolved widths equal the model bit for bit (NaN where the
    model has NaN), with an automatic (-0.01) and an absolute (0.05) temporal tolerance and max_history 2 and 32.  45 x 13 is one and a fraction of a 256-thread
    block; 70 x 37 carries a NaN colour, an Inf colour and a NaN normal pixel in frame 2."""
    assert WG < 45 * 13 and 45 * 13 % WG
    frames = sequence(w, h)
    for tol in (-0.01, 0.05):
        for cap in (2.0, 32.0):
            kw = dict(iterations=iterations, sigma_color=4.0, sigma_normal=0.3, sigma_position=-0.05, max_history=cap, temporal_sigma_position=tol, min_normal_dot=0.9)
            exp = tm.run_sequence(frames, with_albedo, **kw); H = mi.History(w, h)
            for k, (fr, (eout, eres, etp, ehist)) in enumerate(zip(frames, exp)):
                out, res, tp = mi.denoise_image_temporal(H, fr["color"], fr["normal"], fr["position"], fr["albedo"] if with_albedo else None, fr["prev_position"],
                                                         fr["world_to_pixel"], **kw)
                col, cnt = H.read(); tag = (tol, cap, k)
                assert same_bits(col, ehist["a"]), (tag, int((bits(col) != bits(ehist["a"])).sum()))
                assert (bits(cnt) == bits(ehist["n"])).all(), (tag, int((bits(cnt) != bits(ehist["n"])).sum()))
                assert same_bits(out, eout), (tag, int((bits(out) != bits(eout)).sum()))
                assert bits(f32(res)) == bits(f32(eres)) and bits(f32(tp)) == bits(f32(etp)), (tag, res, eres, tp, etp)
                assert H.frames == k + 1
            if (w, h) == (70, 37):      # not vacuous (a condition on the model): the last frame blended history in -- nearly everywhere under the automatic tolerance
                share = (ehist["n"] > 1).mean()      # (about 0.14), and only where a tap lies within 0.05 of the point under the absolute one (pixels are 0.165 apart on the back plane)
                assert share > 0.85 if tol < 0 else 0.1 < share < 0.5, (tol, share)
            H.close()


def test_reset_gives_back_the_first_frame(mi):
    """after mi_history_reset the next frame equals denoise_image bit for bit and frames == 1"""
    frames = sequence(33, 19); H = mi.History(33, 19); kw = dict(iterations=3, sigma_color=4.0, sigma_normal=0.3, sigma_position=-0.05)
    for fr in frames[:3]: mi.denoise_image_temporal(H, fr["color"], fr["normal"], fr["position"], fr["albedo"], fr["prev_position"], fr["world_to_pixel"], **kw)
    assert H.frames == 3 and (H.read()[1] > 1).mean() > 0.85
    H.reset(); assert H.frames == 0
    with pytest.raises(mi.api.MiError, match="no frame"): H.read()
    fr = frames[3]
    out, res, _ = mi.denoise_image_temporal(H, fr["color"], fr["normal"], fr["position"], fr["albedo"], fr["prev_position"], fr["world_to_pixel"], **kw)
    exp, eres = mi.denoise_image(fr["color"], fr["normal"], fr["position"], fr["albedo"], **kw)
    assert same_bits(out, exp) and bits(f32(res)) == bits(f32(eres)) and H.frames == 1 and (H.read()[1] == 1).all()


# ---------------------------------------------------------------------------------------------- 3: render level
def scene_of(mi, name):
    S = mi.scenes
    return S.cornell_box(64, 36, 8, sampler=S.SAMPLER_SOBOL) if name == "cornell_small" else S.sky_view(60, 44, 8, sampler=S.SAMPLER_SOBOL)


@pytest.mark.parametrize("name", ["cornell_small", "sky_view"])
def test_render_level_equals_image_level(mi, name):
    """Three frames along a 24-frame orbit, each cleared and rendered with its own four sample indices: Render.denoise_temporal equals denoise_image_temporal on
    read_film(2), read_fields(2) and Scene.world_to_pixel(), and both equal the model -- output, history and widths.  The films are read, not written.  sky_view has
    camera rays that miss: the fields' `undefined` guides take part as they stand."""
    render = importlib.import_module("mitsuba-im_amd.render")
    sc = scene_of(mi, name); gs = mi.Scene(sc); r = mi.Render(gs, spp=12, fields=GUIDES); cams = render.orbit_cameras(sc, 24)      # 12: a run stays within [0, spp]
    Hr = mi.History(sc.width, sc.height); Hi = mi.History(sc.width, sc.height); hist = None
    kw = dict(iterations=3, sigma_color=4.0, sigma_normal=0.3, sigma_position=-0.05, max_history=32.0, temporal_sigma_position=-0.01, min_normal_dot=0.9)
    for f in range(3):
        gs.update_camera(sc.sample_to_camera, cams[f], sc.near, sc.far); r.clear(); r.run(s0=4 * f, s1=4 * f + 4)
        film = r.read_film(2); fl = r.read_fields(2); N, P, A = fl[..., 0:3], fl[..., 3:6], fl[..., 6:9]; M = gs.world_to_pixel()
        before = (bits(r.read_film(0)).copy(), bits(r.read_fields(0)).copy())
        got = r.denoise_temporal(Hr, **kw); gres, gtp = r.last_denoise_sigma_position, r.last_temporal_sigma_position
        img, ires, itp = mi.denoise_image_temporal(Hi, film, N, P, A, None, M, **kw)
        exp, eres, etp, hist = tm.temporal_frame(hist, film, N, P, A, None, M, **kw)
        assert same_bits(got, img) and same_bits(img, exp), f
        assert bits(f32(gres)) == bits(f32(ires)) == bits(f32(eres)) and bits(f32(gtp)) == bits(f32(itp)) == bits(f32(etp))
        for H in (Hr, Hi):
            col, cnt = H.read(); assert same_bits(col, hist["a"]) and (bits(cnt) == bits(hist["n"])).all(), f
        assert (bits(r.read_film(0)) == before[0]).all() and (bits(r.read_fields(0)) == before[1]).all()
        if name == "sky_view": assert ((N == 0).all(-1) & (P == 0).all(-1)).mean() > 0.05
    # not vacuous (a condition on the model's history): history was blended in -- on sky_view only where the camera sees the ground -- and somewhere dropped
    assert (hist["n"] > 1).mean() > (0.25 if name == "cornell_small" else 0.05) and (hist["n"] == 1).any()


# ---------------------------------------------------------------------------------------------- 4: the projection
def projection_scene(mi, name):
    S = mi.scenes
    if name == "sky_view_crop": return S.set_crop_window(S.sky_view(60, 44, 8, sampler=S.SAMPLER_SOBOL), 150, 100, 70, 31)      # the window (70, 31) .. (130, 75) of a 150 x 100 frame
    if name == "sky_view_lens": return S.with_lens(S.sky_view(60, 44, 8, sampler=S.SAMPLER_SOBOL), 0.05, 4.0)
    return scene_of(mi, name)


@pytest.mark.parametrize("name", ["sky_view", "sky_view_crop", "sky_view_lens", "cornell_small"])
def test_world_to_pixel(mi, name):
    """Scene.world_to_pixel(): the points o + t d of 64 pixel centres' camera rays at t = 1 and t = 7 project to their centre within 1e-3 pixel, and every entry of
    the matrix is within 1e-5 relative of diag(w, h, 1, 1) x inverse(sample_to_camera) x inverse(to_world) in float64 (plus 1e-12 of its row's largest entry, for
    the entries that are zero but for the inversion's own rounding); again after update_camera.  sky_view_crop renders a crop window: pixel (0, 0) is the window's
    first pixel.  sky_view_lens has a thin lens: its rays are those through the lens centre (the aperture sample (0.5, 0.5)), which the projection follows.
    sky_view's camera sits 4.7 units from the origin: the largest entry of M is 196 and the residual 1e-5 pixel.  The Cornell box's camera sits at (278, 273, -800):
    M's translation column reaches 50514, where a float is 0.004 apart, and one unit in front of that camera (Wc = 0.97) the rounding of M to float alone moves the
    projection by 0.0019 pixel (0.00027 at t = 7; both computed in float64 from the float matrix, and measured on the device's rays).  There t = 1 is held to what the
    format allows instead: every entry of M is within 2^-24 relative of its double value, so |X / Wc - x| <= 2^-24 (|M_X| . |q| + |X / Wc| |M_W| . |q|) / Wc, plus
    1e-4 for the ray's own float arithmetic."""
    render = importlib.import_module("mitsuba-im_amd.render")
    sc = projection_scene(mi, name); gs = mi.Scene(sc); rng = np.random.default_rng(3)
    px = np.stack([rng.integers(0, sc.width, 64), rng.integers(0, sc.height, 64)], 1) + 0.5
    for c2w in (None, render.orbit_cameras(sc, 24)[5]):
        if c2w is not None: gs.update_camera(sc.sample_to_camera, c2w, sc.near, sc.far)
        M = gs.world_to_pixel(); assert M.shape == (3, 4) and M.dtype == f32
        full = np.diag([sc.width, sc.height, 1.0, 1.0]) @ np.linalg.inv(np.asarray(sc.sample_to_camera, np.float64)) @ np.linalg.inv(np.asarray(sc.cam_to_world, np.float64))
        ref = full[[0, 1, 3]]
        assert (np.abs(M - ref) <= 1e-5 * np.abs(ref) + 1e-12 * np.abs(ref).max(1, keepdims=True)).all(), np.abs(M - ref).max()
        rays = gs.camera_rays(px.astype(f32)).astype(np.float64)
        for t in (1.0, 7.0):
            Md = M.astype(np.float64); q = np.concatenate([rays[:, 0:3] + t * rays[:, 4:7], np.ones((64, 1))], 1); X, Y, W = (q @ Md[i] for i in range(3))
            ex, ey = np.abs(X / W - px[:, 0]), np.abs(Y / W - px[:, 1])
            print(f"[temporal] world_to_pixel {name} t = {t:g}: residual {ex.max():.2e}, {ey.max():.2e} pixel (largest entry of M {np.abs(M).max():.0f})")
            assert (W > 0).all()
            if name != "cornell_small" or t == 7.0: assert ex.max() <= 1e-3 and ey.max() <= 1e-3, (t, ex.max(), ey.max())
            else:
                aq = np.abs(q); bound = lambda row, v: 2.0 ** -24 * (aq @ np.abs(Md[row]) + np.abs(v / W) * (aq @ np.abs(Md[2]))) / W + 1e-4
                assert (ex <= bound(0, X)).all() and (ey <= bound(1, Y)).all(), (t, ex.max(), ey.max())


# ---------------------------------------------------------------------------------------------- 5, 6: what the history buys and what it drops
def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def test_eight_static_frames_beat_one(mi):
    """Static Cornell box 64 x 36, eight frames of 1 spp with distinct sample indices.  RMSE against a 1024-spp render: denoise_temporal on frame 7 is lower than plain
    denoise() on frame 7 -- no preset ratio: a mean over eight independent frames cannot be worse by construction.  The count is >= 7.5 on at least half the pixels.
    The temporal tolerance is -0.075 here, not the default -0.01.  At 1 spp the position guide of a pixel is the hit of its one sample, anywhere in the pixel's
    footprint; at 64 x 36 a footprint in this room is 21 units across its diagonal in the median, 54 at the 90th percentile and 71 at the most (the corner rays of
    every pixel against the room's walls), while 0.01 of the scene's diagonal (961) is 9.6: under the default a pixel's own record of the frame before is usually
    further away than the tolerance, whatever the history holds.  0.075 x 961 = 72 covers the largest footprint and stays under the width of the small box (165).
    With the default the device gives rmse 0.01478 against 0.01566 (still lower) and a count >= 7.5 on 0.125 of the pixels; at 1920 x 1080 a footprint is 0.5
    units.  Measured with -0.075: see DESIGN.md section 3 (temporal stage)."""
    sc = scene_of(mi, "cornell_small"); gs = mi.Scene(sc)
    rr = mi.Render(gs, spp=1024); rr.run(); ref = rr.read_film(2); rr.close()
    r = mi.Render(gs, fields=GUIDES); H = mi.History(sc.width, sc.height); Hd = mi.History(sc.width, sc.height)
    for f in range(8):
        r.clear(); r.run(s0=f, s1=f + 1); default = r.denoise_temporal(Hd); temporal = r.denoise_temporal(H, temporal_sigma_position=-0.075)
    plain = r.denoise(); _, cnt = H.read()
    e_plain, e_temporal, share = rmse(plain, ref), rmse(temporal, ref), float((cnt >= 7.5).mean()); e_default = rmse(default, ref)
    print(f"[temporal] the same with the default tolerance: rmse denoise_temporal {e_default:.5f}; count >= 7.5 on {float((Hd.read()[1] >= 7.5).mean()):.3f} of the pixels")
    assert e_default < e_plain      # the default tolerance keeps less history here and is still no worse than the last frame alone
    print(f"[temporal] static cornell 64 x 36, frame 7 of 8 x 1 spp: rmse denoise {e_plain:.5f}, denoise_temporal {e_temporal:.5f}; count >= 7.5 on {share:.3f} of the pixels, tp {r.last_temporal_sigma_position:.3f}")
    assert H.frames == 8 and e_temporal < e_plain
    assert share >= 0.5


def test_disocclusion_on_a_real_scene(mi):
    """After an orbit step of 90 degrees more pixels start again at n == 1 than after a step of 15 degrees, and the output is finite wherever the input is."""
    render = importlib.import_module("mitsuba-im_amd.render")
    sc = scene_of(mi, "cornell_small"); gs = mi.Scene(sc); r = mi.Render(gs, fields=GUIDES); cams = render.orbit_cameras(sc, 24); H = mi.History(sc.width, sc.height); share = {}
    for step in (1, 6):      # 15 and 90 degrees
        H.reset()
        for f, cam in enumerate((cams[0], cams[step])):
            gs.update_camera(sc.sample_to_camera, cam, sc.near, sc.far); r.clear(); r.run(s0=4 * f, s1=4 * f + 4); out = r.denoise_temporal(H)
            assert np.isfinite(out[np.isfinite(r.read_film(2)).all(-1)]).all()
        share[step] = float((H.read()[1] == 1).mean())
    print(f"[temporal] share of pixels at n == 1 after an orbit step of 15 degrees {share[1]:.3f}, of 90 degrees {share[6]:.3f}")
    assert share[6] > share[1]


# ---------------------------------------------------------------------------------------------- 7: refusals
def test_refusals_name_their_reason(mi):
    E = mi.api.MiError; fr = sequence(33, 19)[0]; H = mi.History(33, 19)
    args = (fr["color"], fr["normal"], fr["position"]); M = fr["world_to_pixel"]
    with pytest.raises(E, match="iterations"): mi.denoise_image_temporal(H, *args, world_to_pixel=M, iterations=9)
    with pytest.raises(E, match="sigma_color"): mi.denoise_image_temporal(H, *args, world_to_pixel=M, sigma_color=0.0)
    with pytest.raises(E, match="max_history"): mi.denoise_image_temporal(H, *args, world_to_pixel=M, max_history=0.5)
    with pytest.raises(E, match="max_history"): mi.denoise_image_temporal(H, *args, world_to_pixel=M, max_history=float("inf"))
    with pytest.raises(E, match="temporal sigma_position"): mi.denoise_image_temporal(H, *args, world_to_pixel=M, temporal_sigma_position=0.0)
    with pytest.raises(E, match="temporal sigma_position"): mi.denoise_image_temporal(H, *args, world_to_pixel=M, temporal_sigma_position=float("nan"))
    with pytest.raises(E, match="min_normal_dot"): mi.denoise_image_temporal(H, *args, world_to_pixel=M, min_normal_dot=1.5)
    with pytest.raises(E, match="world_to_pixel"): mi.denoise_image_temporal(H, *args)
    assert H.frames == 0      # a refused frame leaves the history as it was
    c = sequence(3, 2)[0]
    with pytest.raises(E, match="image size"): mi.denoise_image_temporal(H, c["color"], c["normal"], c["position"], world_to_pixel=M)
    with pytest.raises(E, match="width or height"): mi.History(0, 4)
    # a demodulate switch without reset
    mi.denoise_image_temporal(H, *args, albedo=fr["albedo"], world_to_pixel=M)
    with pytest.raises(E, match="demodulate differs"): mi.denoise_image_temporal(H, *args, world_to_pixel=M)
    H.reset(); mi.denoise_image_temporal(H, *args, world_to_pixel=M); assert H.frames == 1
    # render level: the field rules of denoise(), and a history of another size
    sc = scene_of(mi, "cornell_small"); gs = mi.Scene(sc); Hs = mi.History(sc.width, sc.height)
    r = mi.Render(gs, fields=["shNormal", "albedo"]); r.run()
    with pytest.raises(E, match="position"): r.denoise_temporal(Hs)
    r = mi.Render(gs, fields=["shNormal", "position"]); r.run()
    with pytest.raises(E, match="demodulate without albedo"): r.denoise_temporal(Hs, demodulate=True)
    with pytest.raises(E, match="image size"): r.denoise_temporal(H)
    assert np.isfinite(r.denoise_temporal(Hs)).all() and Hs.frames == 1
    with pytest.raises(E, match="demodulate differs"): mi.Render(gs, fields=GUIDES).denoise_temporal(Hs)


# ---------------------------------------------------------------------------------------------- 8: device output
def _device_output_main():
    """child process of test_device_output: torch opens the device first, as bench.py does, then the library writes into its tensor"""
    import torch
    t = torch.zeros((36, 64, 3), dtype=torch.float32, device="cuda:0")
    mi = importlib.import_module("mitsuba-im_amd")
    sc = scene_of(mi, "cornell_small"); r = mi.Render(mi.Scene(sc), fields=GUIDES); Hh = mi.History(64, 36); Hd = mi.History(64, 36)
    for f in range(2):
        r.clear(); r.run(s0=4 * f, s1=4 * f + 4)
        host = r.denoise_temporal(Hh, iterations=3)
        assert r.denoise_temporal(Hd, iterations=3, device_ptr=t.data_ptr()) is None
        torch.cuda.synchronize()
        assert same_bits(t.cpu().numpy(), host) and np.abs(host).sum() > 0 and (bits(host) != bits(r.read_film(2))).any()
    assert (bits(Hh.read()[0]) == bits(Hd.read()[0])).all() and (Hd.read()[1] == 2).mean() > 0.5
    print("device output ok")


def test_device_output():
    """denoise_temporal(device_ptr=...) leaves the same bits in a torch device tensor as the host form returns.  In a process of its own: torch has to open the device
    before the library does (the order bench.py keeps)."""
    p = subprocess.run([sys.executable, "-c", "import tests.test_gpu_temporal as t; t._device_output_main()"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "device output ok" in p.stdout, p.stdout + p.stderr


# ---------------------------------------------------------------------------------------------- 9: command line
def test_command_line(mi, tmp_path, capsys, monkeypatch):
    """render.py --orbit 3 --denoise 2 --denoise-temporal writes three frames; frame 0 equals the run without --denoise-temporal but with --sample-offset-per-frame
    (the first frame of a history is the spatial filter), frame 2 differs.  Without a sequence, and with --adaptive: an error that says so."""
    render = importlib.import_module("mitsuba-im_amd.render"); ranges = []; original = mi.api.Render.run

    def spy(self, tile=None, s0=0, s1=None, row_stride=1):
        ranges.append((s0, s1, self.params.spp)); return original(self, tile, s0, s1, row_stride)
    monkeypatch.setattr(mi.api.Render, "run", spy)
    base = [os.path.join(GOLDEN, "meshes", "bunny_box.xml"), "-D", "res=48", "-D", "spp=4", "--denoise", "2"]
    assert render.main(base + ["--orbit", "3", "--denoise-temporal", "-o", str(tmp_path / "t.npy")]) == 0
    assert render.main(base + ["--orbit", "3", "--sample-offset-per-frame", "-o", str(tmp_path / "s.npy")]) == 0
    assert render.main(base + ["--orbit", "3", "-o", str(tmp_path / "p.npy")]) == 0
    t, s, p = ([np.load(tmp_path / f"{k}_{f:03d}.npy") for f in range(3)] for k in "tsp")
    assert t[0].shape == (96, 48, 3) and all(np.isfinite(x).all() for x in t)
    assert (bits(t[0]) == bits(s[0])).all() and (bits(t[2]) != bits(s[2])).any()
    # with the flag (or --denoise-temporal) frame f takes the indices [4 f, 4 f + 4) of a render created for 12; without it every frame takes [0, 4) as before
    assert ranges == [(0, 4, 12), (4, 8, 12), (8, 12, 12)] * 2 + [(0, None, 4)] * 3, ranges
    capsys.readouterr()
    assert render.main(base + ["--denoise-temporal", "-o", str(tmp_path / "x.npy")]) == 1
    assert "--denoise-temporal needs a frame sequence" in capsys.readouterr().err
    assert render.main(base[:5] + ["--orbit", "3", "--denoise-temporal", "-o", str(tmp_path / "x.npy")]) == 1      # without --denoise
    assert "belongs to --denoise" in capsys.readouterr().err
    assert render.main(base + ["--orbit", "3", "--denoise-temporal", "--sampler", "independent", "--spp", "8", "--adaptive", "-o", str(tmp_path / "x.npy")]) == 1
    capsys.readouterr()      # without --denoise the older refusal does not come first: the flag's own one, by its message
    assert render.main(base[:5] + ["--orbit", "3", "--sample-offset-per-frame", "--sampler", "independent", "--spp", "8", "--adaptive", "-o", str(tmp_path / "x.npy")]) == 1
    assert "--sample-offset-per-frame cannot be combined with adaptive sampling" in capsys.readouterr().err
