"""GPU: adaptive sampling (mi_render_set_adaptive / mi_render_run_adaptive; csrc/adaptive.h, kernels_adaptive.hip) against the sequential float32 model of
tests/adaptive_model.py.  The model is fed with per-sample radiance from the CPU oracle or from Render.samples (pinned to the oracle by the parity tests); the sample-count
map must equal it EXACTLY, pixel for pixel: both sides evaluate the same correctly rounded binary32 +, -, x, / and sqrt in the same order, and a pixel's state is owned by
one thread in sample order whatever the round, batch and pool shapes are.

MI355PT_STREAMS / MI355PT_SEGMENTS are set in-process with monkeypatch, as tests/test_gpu_pool_geometry.py sets them (the library reads them when a render is created /
a pool is allocated)."""
import numpy as np
import pytest
from tests import adaptive_model as M

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H, SPP, FACTOR, AVG = 16, 12, 8, 8, 0.177
KNOBS = ("MI355PT_SEGMENTS", "MI355PT_STREAMS", "MI355PT_POOL_LIMIT", "MI355PT_BATCH_PATHS")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def box_film_close(a, b):
    """the allowance of the box-filter film test (tests/test_gpu_parity.py): >= 99.5 % of the pixels bit-equal (own cells: plain sums in sample order), the rest -- pixels
    that received a spill through float atomics -- within 2e-6 relative"""
    same = (bits(a) == bits(b)).all(-1)
    return same.mean() > 0.995 and np.allclose(a, b, rtol=2e-6, atol=1e-7)


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS: monkeypatch.delenv(k, raising=False)


_cache = {}


def cbox(mi, **kw):
    S = mi.scenes
    return S.cornell_box(W, H, SPP, sampler=S.SAMPLER_INDEPENDENT, max_depth=3, **kw)


def cornell(mi, oracle):
    """the shared case: scene, its Scene handle, oracle radiance and film positions of samples 0 .. 63 of every pixel (computed once, never modified)"""
    if "cornell" not in _cache:
        sc = cbox(mi); px = M.tile_pixels(0, 0, W, H); li, pos = M.oracle_samples(oracle, sc, px, SPP * FACTOR)
        li.setflags(write=False); pos.setflags(write=False)
        _cache["cornell"] = (sc, mi.Scene(sc), px, li, pos)
    return _cache["cornell"]


def adaptive_render(mi, gs, max_error, factor=FACTOR, avg=AVG, round_samples=0, tile=None, **kw):
    r = mi.Render(gs, **kw); r.set_adaptive(max_error=max_error, max_sample_factor=factor, round_samples=round_samples, average_luminance=avg)
    r.run_adaptive(tile); return r


def check_stats(st, n, cap):
    assert st["samples_used"] == int(n.sum()) and st["min_count"] == int(n.min()) and st["max_count"] == int(n.max()) and st["pixels_at_cap"] == int((n == cap).sum())
    assert st["samples_traced"] >= st["samples_used"] and st["rounds"] >= 1
    assert bits(st["quantile"]) == bits(M.quantile(0.05))


# ---------------------------------------------------------------------------------------------- 1: counts against the oracle-fed model
@pytest.mark.parametrize("max_error", [0.2, 0.5])
def test_counts_equal_the_oracle_model(mi, oracle, max_error):
    sc, gs, px, li, pos = cornell(mi, oracle)
    want = M.counts(li, SPP, max_error, AVG, FACTOR).reshape(H, W)
    r = adaptive_render(mi, gs, max_error); got = r.sample_counts(); st = r.adaptive_stats()
    print(f"[adaptive] maxError {max_error}: {int((got != want).sum())} of {W * H} counts differ; used {st['samples_used']}, traced {st['samples_traced']}, rounds {st['rounds']}")
    assert got.dtype == np.uint32 and got.shape == (H, W) and (got == want).all()
    check_stats(st, want, SPP * FACTOR)
    assert bits(st["average_luminance"]) == bits(f32(AVG)) and st["rounds"] == FACTOR and r.stats()["samples"] == st["samples_traced"]
    if max_error == 0.2:      # the scene exercises all three endings (tests/test_adaptive_model.py shows it for the inputs)
        assert (got == SPP).sum() >= 20 and ((got > SPP) & (got < SPP * FACTOR)).sum() >= 20 and (got == SPP * FACTOR).sum() >= 20


# ---------------------------------------------------------------------------------------------- 2: batching must not move a bit
def test_rounds_batches_streams_and_segments_do_not_move_a_bit(mi, oracle, monkeypatch):
    """round_samples 1 / 3 / 8 / 64 x planes_per_batch 1 / 0 x MI355PT_STREAMS 1 / 2, and a pool cut into several segments: a pixel that stops in the middle of a batch
    (round 64, automatic planes), rounds that span batches (planes 1), a short last batch (round 3 against the cap of 64), active counts that are no multiple of 64"""
    sc, gs, px, li, pos = cornell(mi, oracle)
    want = M.counts(li, SPP, 0.2, AVG, FACTOR).reshape(H, W); base = None; seen = 0
    for streams in ("1", "2"):
        for segments in (None, "5"):
            for rs in (1, 3, 8, 64):
                for planes in (1, 0):
                    if segments is not None and (rs, planes) not in ((3, 0), (64, 0), (8, 1)): continue
                    monkeypatch.setenv("MI355PT_STREAMS", streams)
                    if segments is None: monkeypatch.delenv("MI355PT_SEGMENTS", raising=False)
                    else: monkeypatch.setenv("MI355PT_SEGMENTS", segments)
                    r = adaptive_render(mi, gs, 0.2, round_samples=rs, planes_per_batch=planes)
                    info = r.pool_info(); assert info["n_pools"] == int(streams) and (segments is None or 2 <= info["n_seg"] <= 5)      # (a pool of 192 paths holds three segments of 64 at the most)
                    got = r.sample_counts(); film = r.read_film(0); st = r.adaptive_stats(); tag = (streams, segments, rs, planes)
                    assert (got == want).all(), tag
                    assert st["rounds"] == -(-int(want.max()) // rs) and st["samples_used"] == int(want.sum()), tag
                    if rs == 1: assert st["samples_traced"] == st["samples_used"], tag      # rounds of one sample trace nothing after a stop
                    if base is None: base = film
                    assert box_film_close(film, base), tag
                    seen += 1; r.close()
    assert seen == 2 * (8 + 3)


# ---------------------------------------------------------------------------------------------- 3: compaction across workgroups
def test_compaction_across_workgroups(mi):
    """40 x 30: 1200 active pixels = 19 wave-owned ranges in 5 workgroups; the model is fed from Render.samples"""
    S = mi.scenes; sc = S.cornell_box(40, 30, SPP, sampler=S.SAMPLER_INDEPENDENT, max_depth=3); gs = mi.Scene(sc)
    li = M.device_samples(mi.Render(gs), M.tile_pixels(0, 0, 40, 30), SPP * 4)
    want = M.counts(li, SPP, 0.2, AVG, 4).reshape(30, 40)
    assert len(np.unique(want)) >= 3
    r = adaptive_render(mi, gs, 0.2, factor=4); got = r.sample_counts()
    assert (got == want).all(), int((got != want).sum())
    check_stats(r.adaptive_stats(), want, SPP * 4)
    r3 = adaptive_render(mi, gs, 0.2, factor=4, round_samples=3, planes_per_batch=2); assert (r3.sample_counts() == want).all()


def test_compaction_ranges_longer_than_a_wave(mi):
    """320 x 240: 76800 active pixels are more than 1024 x 64, so every wave of the compaction owns a range of 128 entries and walks it in two steps (the last ranges are
    short or empty); the second round starts from a list that is no multiple of anything"""
    S = mi.scenes; sc = S.cornell_box(320, 240, SPP, sampler=S.SAMPLER_INDEPENDENT, max_depth=3); gs = mi.Scene(sc)
    li = M.device_samples(mi.Render(gs), M.tile_pixels(0, 0, 320, 240), SPP * 2)
    want = M.counts(li, SPP, 0.5, AVG, 2).reshape(240, 320)
    assert len(np.unique(want)) >= 3 and 1000 < (want > SPP).sum() < 76000
    r = adaptive_render(mi, gs, 0.5, factor=2, round_samples=4); got = r.sample_counts()
    assert (got == want).all(), int((got != want).sum())
    check_stats(r.adaptive_stats(), want, SPP * 2); assert r.adaptive_stats()["rounds"] == 4


# ---------------------------------------------------------------------------------------------- 4: anchor against the uniform render
@pytest.mark.parametrize("factor", [1, 4])
def test_max_error_zero_is_the_uniform_render(mi, oracle, factor):
    """box filter, max_error 0: a pixel stops before the cap only where its variance is exactly 0.  Factor 1: every count is 8 and the film is run()'s at 8 spp.  Factor 4:
    run()'s at 32 spp (1 / 8 and 1 / 32 are powers of two: scaling a footprint by them commutes with every rounding, and developing divides them out) -- except in the
    pixels whose first 8 samples are all black: their variance is 0, `ciWidth <= 0` holds, and they stop at 8 by the rule itself (6 of the 192 here; some of their later
    samples are not black).  Those are compared with run() at 8 spp: every pixel against the uniform render of its own count."""
    sc, gs, px, li, pos = cornell(mi, oracle)
    want = M.counts(li[:, :SPP * factor], SPP, 0.0, AVG, factor).reshape(H, W)
    r = adaptive_render(mi, gs, 0.0, factor=factor); got = r.sample_counts()
    assert (got == want).all() and set(np.unique(want).tolist()) <= {SPP, SPP * factor}
    if factor == 1: assert (got == SPP).all()
    early = want < SPP * factor; assert (M.luminance(li[:, :SPP])[early.ravel()] == 0).all() and early.sum() <= 8      # the pixels that stop early are black so far
    u = mi.Render(gs, spp=SPP * factor); u.run(); u8 = mi.Render(gs, spp=SPP); u8.run()
    a, b = r.read_film(2), np.where(early[..., None], u8.read_film(2), u.read_film(2))
    print(f"[adaptive] factor {factor}: {int(early.sum())} pixels stop early; developed film bit-equal on {(bits(a) == bits(b)).all(-1).mean():.4f} of the pixels, max |diff| {np.abs(a - b).max():.3g}")
    assert box_film_close(a, b)
    b_ = r.film_shape(0)[3]; inner = lambda f: f[b_:f.shape[0] - b_, b_:f.shape[1] - b_, 4]
    assert np.allclose(inner(r.read_film(0))[~early], inner(u.read_film(0))[~early] / (SPP * factor), rtol=1e-6)      # weights of ONE sample per pixel


# ---------------------------------------------------------------------------------------------- 5: wide filter
def test_gaussian_film_against_the_float64_model(mi, oracle):
    S = mi.scenes; sc = cbox(mi, filter_kind=S.FILTER_GAUSSIAN); gs = mi.Scene(sc); px = M.tile_pixels(0, 0, W, H)
    li, pos = M.oracle_samples(oracle, sc, px, SPP * 4); orc = oracle.Oracle(sc)
    want = M.counts(li, SPP, 0.2, AVG, 4); model = M.film(oracle, orc, W, H, px, li, pos, want); b = orc.border
    r = adaptive_render(mi, gs, 0.2, factor=4); assert (r.sample_counts().ravel() == want).all() and len(np.unique(want)) >= 3
    dev = r.read_film(2); ref = M.develop(model, b)
    print(f"[adaptive] gaussian: max relative error of the developed film {np.abs(dev - ref).max() / np.abs(ref).max():.3g}")
    assert np.allclose(dev, ref, rtol=2e-5, atol=2e-6)      # the wide-filter tolerance against the oracle (tests/test_gpu_parity.py)
    raw = r.read_film(0); assert raw.shape == model.shape and np.allclose(raw[..., 4], model[..., 4], rtol=2e-5, atol=2e-6)
    # interior pixels hold the filter weights of ONE sample per contributing pixel: what a uniform render holds, over spp
    u = mi.Render(gs); u.run(); uw = u.read_film(0)[..., 4]; inner = (slice(2 * b, -2 * b),) * 2
    ratio = raw[..., 4][inner] / (uw[inner] / SPP); assert 0.5 < ratio.min() and ratio.max() < 2.0      # (the uniform render's weights are spp times as large)


# ---------------------------------------------------------------------------------------------- 6: degenerate shapes
def test_degenerate_shapes(mi, oracle):
    sc, gs, px, li, pos = cornell(mi, oracle)
    r = adaptive_render(mi, gs, 1e9); st = r.adaptive_stats()      # everything stops at spp: one round, no launch on an empty list
    assert (r.sample_counts() == SPP).all() and st["rounds"] == 1 and st["samples_used"] == st["samples_traced"] == W * H * SPP and st["pixels_at_cap"] == 0
    full = M.counts(li, SPP, 0.2, AVG, FACTOR).reshape(H, W)
    r = adaptive_render(mi, gs, 0.2, tile=(5, 7, 6, 8)); got = r.sample_counts()      # a 1 x 1 tile
    assert got[7, 5] == full[7, 5] and got.sum() == full[7, 5] and r.adaptive_stats()["samples_used"] == int(full[7, 5])
    r = adaptive_render(mi, gs, 0.2, tile=(3, 2, 11, 9)); got = r.sample_counts(); inside = np.zeros((H, W), bool); inside[2:9, 3:11] = True
    assert (got[inside] == full[inside]).all() and (got[~inside] == 0).all()
    check_stats(r.adaptive_stats(), full[inside], SPP * FACTOR)
    # no cap but the stream's: maxError 1.0 ends within 8 rounds of 8 (the model raises if a pixel needs more than the 64 samples it is given)
    want = M.counts(li, SPP, 1.0, AVG, -1).reshape(H, W); assert want.max() > 4 * SPP
    r = adaptive_render(mi, gs, 1.0, factor=-1); st = r.adaptive_stats()
    assert (r.sample_counts() == want).all() and st["rounds"] == -(-int(want.max()) // SPP) <= 8 and st["pixels_at_cap"] == 0


# ---------------------------------------------------------------------------------------------- 7: other scenes
@pytest.mark.parametrize("name", ["volpath_fog_box", "thinlens", "envmap"])
def test_other_scenes(mi, name):
    S = mi.scenes
    if name == "volpath_fog_box": sc = S.fog_box(W, H, SPP, sampler=S.SAMPLER_INDEPENDENT, max_depth=4, integrator=S.INTEGRATOR_VOLPATH)
    elif name == "thinlens": sc = S.with_lens(cbox(mi), 20.0, 800.0)
    else: sc = S.sky_view(W, H, SPP, sampler=S.SAMPLER_INDEPENDENT, max_depth=3, hide_emitters=True)      # camera rays that miss: radiance 0, variance 0
    gs = mi.Scene(sc); li = M.device_samples(mi.Render(gs), M.tile_pixels(0, 0, W, H), SPP * 4)
    want = M.counts(li, SPP, 0.2, AVG, 4).reshape(H, W); assert len(np.unique(want)) >= 3
    if name == "envmap": assert ((M.luminance(li).max(1) == 0) & (want.ravel() == SPP)).sum() >= 20
    r = adaptive_render(mi, gs, 0.2, factor=4); got = r.sample_counts()
    assert (got == want).all(), (name, int((got != want).sum()))
    check_stats(r.adaptive_stats(), want, SPP * 4)


# ---------------------------------------------------------------------------------------------- 8: average luminance
def test_average_luminance_estimate(mi, oracle):
    sc, gs, px, li, pos = cornell(mi, oracle)
    want = M.luminance_estimate(mi.Render(gs).samples(M.luminance_estimate_pairs(W, H)))
    r = adaptive_render(mi, gs, 0.2, avg=0.0); st = r.adaptive_stats()
    assert bits(st["average_luminance"]) == bits(want) and 0.01 < want < 10
    # the render used it: its counts are the model's at that value, and never reached the estimate's sample index
    assert (r.sample_counts() == M.counts(li, SPP, 0.2, float(want), FACTOR).reshape(H, W)).all()
    S = mi.scenes; big = S.cornell_box(128, 96, SPP, sampler=S.SAMPLER_INDEPENDENT, max_depth=3); gb = mi.Scene(big)      # more pixels than the 10000 of the estimate
    pairs = M.luminance_estimate_pairs(128, 96); assert len(pairs) == 10000
    rb = adaptive_render(mi, gb, 1e9, factor=1, avg=-1.0)
    assert bits(rb.adaptive_stats()["average_luminance"]) == bits(M.luminance_estimate(mi.Render(gb).samples(pairs)))


# ---------------------------------------------------------------------------------------------- 9: edits and clear
def test_edit_needs_clear_and_then_matches_a_fresh_scene(mi):
    sc = cbox(mi); gs = mi.Scene(sc); r = adaptive_render(mi, gs, 0.2)
    c2w = np.array(sc.cam_to_world, f32).reshape(4, 4).copy(); c2w[0, 3] += f32(25.0); c2w[1, 3] -= f32(10.0)
    gs.update_camera(sc.sample_to_camera, c2w, sc.near, sc.far)
    with pytest.raises(mi.api.MiError, match="mi_render_clear"):
        r.run_adaptive()
    r.clear(); assert (r.sample_counts() == 0).all() and r.adaptive_stats()["samples_used"] == 0
    r.run_adaptive()
    fresh_sc = cbox(mi); fresh_sc.cam_to_world = c2w; f = adaptive_render(mi, mi.Scene(fresh_sc), 0.2)
    assert (r.sample_counts() == f.sample_counts()).all() and box_film_close(r.read_film(0), f.read_film(0))
    before = cbox(mi); assert (adaptive_render(mi, mi.Scene(before), 0.2).sample_counts() != f.sample_counts()).any()      # the edit moved the image


def test_average_luminance_is_estimated_again_after_an_edit(mi):
    sc = cbox(mi); gs = mi.Scene(sc); r = adaptive_render(mi, gs, 0.2, avg=0.0); a0 = r.adaptive_stats()["average_luminance"]
    ems = [dict(e, radiance=[3.0 * x for x in e["radiance"]]) for e in sc.emitters]; gs.update_emitters(ems)
    r.clear(); r.run_adaptive(); a1 = r.adaptive_stats()["average_luminance"]
    assert bits(a1) == bits(M.luminance_estimate(mi.Render(gs).samples(M.luminance_estimate_pairs(W, H)))) and a1 > 2.5 * a0


# ---------------------------------------------------------------------------------------------- 10: refusals, by message
def test_refusals(mi, monkeypatch):
    S = mi.scenes; E = mi.api.MiError; sc = cbox(mi); gs = mi.Scene(sc)
    with pytest.raises(E, match="independent sampler"):
        mi.Render(gs, sampler=S.SAMPLER_SOBOL).set_adaptive()
    with pytest.raises(E, match="less than 8 samples per pixel"):
        mi.Render(gs, spp=4).set_adaptive()
    for integ in (S.INTEGRATOR_DIRECT, S.INTEGRATOR_AO):
        with pytest.raises(E, match="direct and ao integrators is not implemented"):
            mi.Render(gs, integrator=integ).set_adaptive()
    with pytest.raises(E, match="field channels"):
        mi.Render(gs, fields=["distance"]).set_adaptive()
    r = mi.Render(gs)
    with pytest.raises(E, match="max_sample_factor must not be 0"):
        r.set_adaptive(max_sample_factor=0)
    with pytest.raises(E, match="max_error must be >= 0"):
        r.set_adaptive(max_error=-0.5)
    for p in (0.0, 1.0, -0.1):
        with pytest.raises(E, match=r"p_value must lie in \(0, 1\)"):
            r.set_adaptive(p_value=p)
    with pytest.raises(E, match="end of the independent stream"):
        r.set_adaptive(max_sample_factor=1 << 21)      # 2^21 x 8 = 2^24
    r.set_adaptive(max_sample_factor=(1 << 21) - 1)     # 2^24 - 8 samples: allowed
    with pytest.raises(E, match="no adaptive parameters are set"):
        mi.Render(gs).run_adaptive()
    r = mi.Render(gs); r.set_adaptive(max_error=0.5, max_sample_factor=2, average_luminance=AVG); r.set_adaptive(None)
    with pytest.raises(E, match="no adaptive parameters are set"):
        r.run_adaptive()
    r = adaptive_render(mi, gs, 0.5, factor=2)
    with pytest.raises(E, match="one adaptive run per mi_render_clear"):
        r.run_adaptive()
    with pytest.raises(E, match="holds an adaptive run"):
        r.run()
    with pytest.raises(E, match="holds an adaptive run"):
        mi.Render(gs).merge_film(r)
    with pytest.raises(E, match="the film holds samples"):
        r.set_adaptive()
    u = mi.Render(gs); u.run()
    with pytest.raises(E, match="the film holds samples"):
        u.set_adaptive()
    u.clear(); u.set_adaptive(max_error=0.5, max_sample_factor=2, average_luminance=AVG); u.run(); u.clear(); u.run_adaptive()      # uniform runs stay possible on a clear film
    assert u.sample_counts().min() >= SPP
    monkeypatch.setenv("MI355PT_POOL_LIMIT", "4096")
    r = mi.Render(gs); r.set_adaptive(average_luminance=AVG)
    with pytest.raises(E, match="footprint, state and count buffers .* larger than MI355PT_POOL_LIMIT"):
        r.run_adaptive()


def test_scene_description_carries_the_parameters(mi, oracle):
    """api.Render picks up sc.adaptive, the way it picks up sc.fields (scene files with an `adaptive` integrator)"""
    sc, gs, px, li, pos = cornell(mi, oracle)
    sc2 = type(sc)(sc); sc2.adaptive = dict(max_error=0.2, p_value=0.05, max_sample_factor=FACTOR); gs2 = mi.Scene(sc2)
    r = mi.Render(gs2); r.set_adaptive(**dict(sc2.adaptive, average_luminance=AVG)); r.run_adaptive()
    assert (r.sample_counts() == M.counts(li, SPP, 0.2, AVG, FACTOR).reshape(H, W)).all()
    r = mi.Render(gs2); r.run_adaptive(); assert r.adaptive_stats()["average_luminance"] > 0 and r.sample_counts().min() >= SPP
    with pytest.raises(mi.api.MiError, match="host mirror does not offer adaptive sampling"):
        mi.api.HostIntegrator(gs2)


def test_cancel_is_observed_before_the_first_batch(mi):
    gs = mi.Scene(cbox(mi)); r = mi.Render(gs); r.set_adaptive(max_error=0.5, max_sample_factor=2, average_luminance=AVG); r.cancel()
    with pytest.raises(mi.api.MiError, match="cancelled") as e:
        r.run_adaptive()
    assert e.value.code == 4
    with pytest.raises(mi.api.MiError, match="mi_render_clear"):      # whatever the cancelled run left is an adaptive film
        r.run_adaptive()
    r.clear(); r.run_adaptive(); assert r.sample_counts().min() >= SPP


def test_command_line_renders_adaptive_scene_files(mi, oracle, tmp_path):
    """render.py: a scene file with the `adaptive` integrator renders through run_adaptive and --sample-counts writes the map; --adaptive wraps a plain `path` file, also
    with --orbit (clear, camera edit, adaptive run per frame; frame 0 is the scene's own camera)"""
    import importlib
    render = importlib.import_module("mitsuba-im_amd.render"); X = importlib.import_module("mitsuba-im_amd.xml_scene")
    sc, gs, px, li, pos = cornell(mi, oracle)
    wrapped = type(sc)(sc); wrapped.adaptive = dict(max_error=0.5, p_value=0.05, max_sample_factor=2)
    d1 = tmp_path / "a"; d1.mkdir(); p1 = X.export_scene(wrapped, str(d1)); d2 = tmp_path / "b"; d2.mkdir(); p2 = X.export_scene(sc, str(d2))
    assert render.main([p1, "-o", str(tmp_path / "a.npy"), "--sample-counts", str(tmp_path / "ca.npy")]) == 0
    ca = np.load(tmp_path / "ca.npy"); img = np.load(tmp_path / "a.npy")
    assert ca.shape == (H, W) and ca.min() >= SPP and ca.max() <= 2 * SPP and len(np.unique(ca)) >= 3 and img.shape == (H, W, 3) and np.isfinite(img).all() and img.max() > 0
    assert render.main([p2, "-o", str(tmp_path / "b.npy"), "--adaptive", "0.5", "--max-sample-factor", "2", "--sample-counts", str(tmp_path / "cb.npy")]) == 0
    assert (np.load(tmp_path / "cb.npy") == ca).all() and (bits(np.load(tmp_path / "b.npy")) == bits(img)).all(-1).mean() > 0.995
    assert render.main([p2, "-o", str(tmp_path / "o.npy"), "--adaptive", "0.5", "--max-sample-factor", "2", "--orbit", "2", "--sample-counts", str(tmp_path / "co.npy")]) == 0
    c0, c1 = np.load(tmp_path / "co_000.npy"), np.load(tmp_path / "co_001.npy")
    assert (c0 == ca).all() and (c1 != ca).any() and c1.min() >= SPP and np.load(tmp_path / "o_001.npy").shape == (H, W, 3)
    assert render.main([p2, "-o", str(tmp_path / "x.npy"), "--sample-counts", str(tmp_path / "cx.npy")]) == 1      # no adaptive sampling asked for
