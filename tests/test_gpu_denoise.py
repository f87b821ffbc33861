"""GPU (MI355X): the edge-avoiding a-trous denoiser (mi_denoise_image / mi_render_denoise, include/mi355pt.h; csrc/kernels_denoise.hip) against the NumPy model of its
definition (tests/denoise_model.py): bit for bit at the image level, the render level against the image level on the render's own developed films, the device
output, the refusals, and the command line."""
import importlib
import os
import subprocess
import sys
import numpy as np
import pytest
from tests import denoise_model as dm
from tests.conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
f32 = np.float32
TILE = (32, 8)      # the level kernel's workgroup tile (MI_DN_TILE_W x MI_DN_TILE_H, csrc/denoise.h); steps 1 and 2 go through LDS, steps >= 4 read directly
GUIDES = [("shNormal", 0.0), ("position", 0.0), "albedo"]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(got, exp):
    """equal bits wherever the expectation is a number, NaN exactly where it is NaN"""
    got = np.asarray(got, f32); exp = np.asarray(exp, f32); nan = np.isnan(exp)
    return (np.isnan(got) == nan).all() and (bits(got)[~nan] == bits(exp)[~nan]).all()


def case_of(w, h):
    c = dm.random_case(w, h, seed=100 + w)
    if (w, h) == (70, 37): c, _ = dm.plant_non_finite(c)
    return c


# ---------------------------------------------------------------------------------------------- 1: image level
@pytest.mark.parametrize("sigma_position", [0.5, -0.05])
@pytest.mark.parametrize("with_albedo", [True, False])
@pytest.mark.parametrize("w,h", dm.GPU_SIZES)
def test_image_level_equals_the_model(mi, w, h, with_albedo, sigma_position):
    """mi_denoise_image equals the model bit for bit (NaN where the model has NaN) after 1, 2, 3, 5 and 8 iterations -- LDS levels, direct levels and steps beyond
    the image -- with and without demodulation, with a given and an automatic position width (the resolved width's bits too).  45 x 13 is one and a fraction of the
    32 x 8 tile in each dimension; 70 x 37 carries a NaN colour, an Inf colour and a NaN normal pixel."""
    assert TILE[0] < 45 < 2 * TILE[0] and TILE[1] < 13 < 2 * TILE[1]
    c = case_of(w, h); A = c["albedo"] if with_albedo else None; st = {}
    _, res = dm.atrous(c["color"], c["normal"], c["position"], A, iterations=8, sigma_color=4.0, sigma_normal=0.3, sigma_position=sigma_position, stats=st)
    for k in dm.GPU_ITERATIONS:
        got, gres = mi.denoise_image(c["color"], c["normal"], c["position"], A, iterations=k, sigma_color=4.0, sigma_normal=0.3, sigma_position=sigma_position)
        exp = st["levels"][k - 1]
        assert same_bits(got, exp), (k, int((bits(got) != bits(exp)).sum()))
        assert bits(f32(gres)) == bits(f32(res)), (k, gres, res)
        if (w, h) != (1, 1):      # not vacuous: the filter moved the image (a single pixel has nothing to mix with)
            fin = np.isfinite(c["color"]).all(-1)
            assert (bits(got) != bits(c["color"])).any(-1)[fin].mean() > 0.90, k
    if w >= 3: assert st["cut"] > 0      # taps across the planted position edge fell under the -80 cut
    if (w, h) == (70, 37): assert np.isnan(got).any() and np.isinf(got).any()


def test_zero_iterations_and_the_resolved_width(mi):
    c = case_of(33, 19)
    got, res = mi.denoise_image(c["color"], c["normal"], c["position"], c["albedo"], iterations=0, sigma_position=0.5)
    assert (bits(got) == bits(c["color"])).all() and res == 0.5
    # no finite position: the term is off
    got, res = mi.denoise_image(c["color"], c["normal"], np.full_like(c["position"], np.inf), None, iterations=2, sigma_position=-0.05)
    assert res == 0.0 and (bits(got) == bits(c["color"])).all()      # kp = 0 times an Inf - Inf distance: every tap is dropped


# ---------------------------------------------------------------------------------------------- 2, 3: render level
def scene_of(mi, name):
    S = mi.scenes
    # 8 spp: the tests render samples 0..3, filter, render samples 4..7 and filter again
    return S.cornell_box(64, 36, 8, sampler=S.SAMPLER_SOBOL) if name == "cornell_small" else S.sky_view(60, 44, 8, sampler=S.SAMPLER_SOBOL)


@pytest.mark.parametrize("name,streams", [("cornell_small", None), ("sky_view", None), ("cornell_small", "1")])
def test_render_level_equals_image_level(mi, name, streams, monkeypatch):
    """Render.denoise -- radiance and guides developed from the film planes in place -- equals denoise_image on read_film(2) and read_fields(2), and both equal the model;
    again after four more samples (the scratch is reused, the films were only read).  sky_view has camera rays that miss: the fields' `undefined` enters the guides.
    MI355PT_STREAMS=1: one pool instead of two feeds the films."""
    if streams: monkeypatch.setenv("MI355PT_STREAMS", streams)
    sc = scene_of(mi, name); gs = mi.Scene(sc); r = mi.Render(gs, fields=GUIDES)
    for round_no, (s0, s1) in enumerate(((0, 4), (4, 8))):
        r.run(s0=s0, s1=s1)
        film = r.read_film(2); fl = r.read_fields(2); N, P, A = fl[..., 0:3], fl[..., 3:6], fl[..., 6:9]
        before = (bits(r.read_film(0)).copy(), bits(r.read_fields(0)).copy())
        if name == "sky_view":
            miss = (N == 0).all(-1) & (P == 0).all(-1)
            assert miss.mean() > 0.05
        for kw in (dict(iterations=5, sigma_color=4.0, sigma_normal=0.3, sigma_position=-0.05), dict(iterations=2, sigma_color=2.0, sigma_normal=0.2, sigma_position=30.0)):
            for demod in (True, False):
                got = r.denoise(demodulate=demod, **kw); gres = r.last_denoise_sigma_position
                img, ires = mi.denoise_image(film, N, P, A if demod else None, **kw)
                exp, eres = dm.atrous(film, N, P, A if demod else None, **kw)
                assert same_bits(got, img) and same_bits(img, exp), (round_no, kw, demod)
                assert bits(f32(gres)) == bits(f32(ires)) == bits(f32(eres))
                if kw["iterations"] == 5: assert (bits(got) != bits(film)).any(-1).mean() > 0.5
        assert (bits(r.read_film(0)) == before[0]).all() and (bits(r.read_fields(0)) == before[1]).all()      # the films were read, not written
    assert same_bits(r.denoise(iterations=0), film)


def _device_output_main():
    """child process of test_device_output: torch opens the device first, as bench.py does, then the library writes into its tensor"""
    import torch
    t = torch.zeros((36, 64, 3), dtype=torch.float32, device="cuda:0")
    mi = importlib.import_module("mitsuba-im_amd")
    sc = scene_of(mi, "cornell_small"); r = mi.Render(mi.Scene(sc), fields=GUIDES); r.run(s0=0, s1=4)
    host = r.denoise(iterations=3)
    assert r.denoise(iterations=3, device_ptr=t.data_ptr()) is None
    torch.cuda.synchronize()
    assert same_bits(t.cpu().numpy(), host) and np.abs(host).sum() > 0 and (bits(host) != bits(r.read_film(2))).any()
    print("device output ok")


def test_device_output():
    """denoise(device_ptr=...) leaves the same bits in a torch device tensor as the host form returns.  In a process of its own: torch has to open the device before
    the library does (the order bench.py keeps), which no test that runs after the others can arrange in this process."""
    p = subprocess.run([sys.executable, "-c", "import tests.test_gpu_denoise as t; t._device_output_main()"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "device output ok" in p.stdout, p.stdout + p.stderr


# ---------------------------------------------------------------------------------------------- 4: refusals
def test_refusals_name_their_reason(mi):
    E = mi.api.MiError; S = mi.scenes
    sc = scene_of(mi, "cornell_small"); gs = mi.Scene(sc)
    r = mi.Render(gs, fields=["shNormal", "albedo"]); r.run()
    with pytest.raises(E, match="position"): r.denoise()
    r = mi.Render(gs, fields=["shNormal", "position"]); r.run()
    with pytest.raises(E, match="demodulate without albedo"): r.denoise(demodulate=True)
    assert np.isfinite(r.denoise()).all()      # demodulate=None: no albedo field, no demodulation
    with pytest.raises(E, match="iterations"): r.denoise(iterations=9)
    with pytest.raises(E, match="sigma_color"): r.denoise(sigma_color=0.0)
    with pytest.raises(E, match="sigma_normal"): r.denoise(sigma_normal=float("nan"))
    with pytest.raises(E, match="sigma_position"): r.denoise(sigma_position=0.0)
    c = case_of(3, 2)
    with pytest.raises(E, match="iterations"): mi.denoise_image(c["color"], c["normal"], c["position"], iterations=9)
    with pytest.raises(E, match="sigma_color"): mi.denoise_image(c["color"], c["normal"], c["position"], sigma_color=float("inf"))
    with pytest.raises(E, match="width or height"): mi.denoise_image(np.zeros((0, 4, 3), f32), np.zeros((0, 4, 3), f32), np.zeros((0, 4, 3), f32))
    # plastic: set_fields refuses the albedo field as before; filtering without it works
    cm = S.cbox_materials(48, 48, 4); gm = mi.Scene(cm)
    with pytest.raises(E, match="albedo") as ei: mi.Render(gm, fields=GUIDES)
    assert ei.value.code == 3
    rm = mi.Render(gm, fields=["shNormal", "position"]); rm.run()
    out = rm.denoise(iterations=3); assert np.isfinite(out).all() and (bits(out) != bits(rm.read_film(2))).any()
    # a film that holds an adaptive run has no field film
    sa = S.cornell_box(32, 24, 8, sampler=S.SAMPLER_INDEPENDENT, max_depth=3); ra = mi.Render(mi.Scene(sa)); ra.set_adaptive(max_error=0.5, max_sample_factor=2); ra.run_adaptive()
    with pytest.raises(E, match="adaptive run"): ra.denoise()


# ---------------------------------------------------------------------------------------------- 5: command line
def test_command_line(mi, tmp_path, monkeypatch):
    """render.py --denoise 3 --denoise-raw: both files are written, the fields the option added are not; the filtered file equals the model applied to the raw file
    and to the fields read through the API in the same process (read when the script calls Render.denoise: no second render)."""
    render = importlib.import_module("mitsuba-im_amd.render"); imageio = importlib.import_module("mitsuba-im_amd.imageio")
    seen = {}; original = mi.api.Render.denoise

    def spy(self, **kw):
        seen["names"] = list(self.field_names); seen["fields"] = self.read_fields(2); seen["kw"] = kw
        return original(self, **kw)
    monkeypatch.setattr(mi.api.Render, "denoise", spy)
    out = str(tmp_path / "f.exr"); raw = str(tmp_path / "raw.exr")
    args = [os.path.join(GOLDEN, "meshes", "bunny_box.xml"), "--denoise", "3", "--denoise-raw", raw, "--denoise-sigma", "2.0", "0.3", "-0.05", "-D", "res=48", "-D", "spp=4", "-o", out]
    assert render.main(args) == 0
    def rgb_of(path):
        px, names = imageio.read_exr(path); assert sorted(names) == ["B", "G", "R"], names      # the three fields the option added are not written
        return np.ascontiguousarray(px[..., [names.index(ch) for ch in "RGB"]], f32)
    filtered, unfiltered = rgb_of(out), rgb_of(raw)
    assert filtered.shape == unfiltered.shape == (96, 48, 3)
    assert seen["names"] == ["shNormal", "position", "albedo"] and seen["kw"]["iterations"] == 3
    fl = seen["fields"]
    exp, _ = dm.atrous(unfiltered, fl[..., 0:3], fl[..., 3:6], fl[..., 6:9], iterations=3, sigma_color=2.0, sigma_normal=0.3, sigma_position=-0.05)
    assert same_bits(filtered, exp) and (bits(filtered) != bits(unfiltered)).any(-1).mean() > 0.5
    # refused by name with adaptive sampling
    assert render.main(args + ["--sampler", "independent", "--spp", "8", "--adaptive"]) == 1


def test_command_line_keeps_the_scene_files_own_fields_and_works_per_frame(mi, tmp_path, capsys):
    """A multichannel scene file that asks for distance and position: --denoise reuses its position, adds shNormal and albedo, and the file holds the radiance and
    the scene's two fields only.  A scene with a plastic has no albedo field: filtered without demodulation, with a message.  --orbit: one filter call per frame."""
    render = importlib.import_module("mitsuba-im_amd.render"); imageio = importlib.import_module("mitsuba-im_amd.imageio"); X = importlib.import_module("mitsuba-im_amd.xml_scene")
    S = mi.scenes; sc = S.cornell_box(32, 24, 4, sampler=S.SAMPLER_SOBOL); sc.fields = [("distance", 0.0), ("position", 0.0)]
    d = tmp_path / "m"; d.mkdir(); p = X.export_scene(sc, str(d))
    assert render.main([p, "-o", str(tmp_path / "plain.exr")]) == 0 and render.main([p, "--denoise", "-o", str(tmp_path / "m.exr"), "--denoise-raw", str(tmp_path / "mraw.npy")]) == 0
    plain, names0 = imageio.read_exr(str(tmp_path / "plain.exr")); px, names = imageio.read_exr(str(tmp_path / "m.exr"))
    assert names == names0 and len(names) == 9 and not any("shNormal" in n or "albedo" in n for n in names)
    colour = [i for i, n in enumerate(names) if n.startswith("color")]; rest = [i for i in range(9) if i not in colour]
    assert (bits(px[..., rest]) == bits(plain[..., rest])).all() and (bits(px[..., colour]) != bits(plain[..., colour])).any(-1).mean() > 0.5
    raw = np.load(tmp_path / "mraw.npy"); order = [names.index("color." + ch) for ch in "RGB"]
    assert (bits(raw) == bits(plain[..., order])).all()
    # plastic: no albedo field
    cm = S.cbox_materials(32, 32, 4); d2 = tmp_path / "p"; d2.mkdir(); p2 = X.export_scene(cm, str(d2)); capsys.readouterr()
    assert render.main([p2, "--denoise", "3", "-o", str(tmp_path / "p.npy")]) == 0
    assert "without albedo demodulation" in capsys.readouterr().err and np.isfinite(np.load(tmp_path / "p.npy")).all()
    # frames
    assert render.main([p2, "--denoise", "2", "--orbit", "8", "-o", str(tmp_path / "o.npy"), "--denoise-raw", str(tmp_path / "oraw.npy")]) == 0
    for f in ("o_000.npy", "o_001.npy", "oraw_000.npy", "oraw_001.npy"): assert np.load(tmp_path / f).shape == (32, 32, 3)
    for f in ("000", "001"):      # frame 1: the camera turned by 45 degrees still sees the room
        fr, rw = np.load(tmp_path / f"o_{f}.npy"), np.load(tmp_path / f"oraw_{f}.npy")
        assert rw.max() > 0 and (bits(fr) != bits(rw)).any(-1).mean() > 0.25
