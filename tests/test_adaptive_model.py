"""CPU: the numpy model of the adaptive stopping rule (tests/adaptive_model.py; adaptive.cpp:202-319) is checked on its own before anything runs on a GPU, the test
scene is shown to exercise all three ways a pixel can end, and the new entry points are declared, exported and bound."""
import ctypes as C
import ctypes.util
import inspect
import os
import re

import numpy as np
import pytest
from tests import adaptive_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_quantile_is_positive_and_the_raw_polynomial_is_not():
    """pValue = 0.05: |approx_erfinv(-0.95)| * sqrt(2) = 1.9599638, the two-sided 95 % quantile the reference's comment (adaptive.cpp:192-195) means.  The reference's own
    expression gives -1.9599638: the confidence interval's width is then negative, `ciWidth <= maxError * base` holds at the first test and every pixel stops at spp.
    That is the reason for the absolute value."""
    assert bits(M.quantile(0.05)) == bits(f32(1.9599638)) and bits(M.approx_erfinv(f32(-0.95))) == bits(f32(-1.3859037))
    assert bits(M.raw_quantile(0.05)) == bits(f32(-1.9599638))
    for p in (0.001, 0.01, 0.05, 0.3, 0.9):
        assert M.raw_quantile(p) < 0 < M.quantile(p) and bits(M.quantile(p)) == bits(-M.raw_quantile(p))
    assert M.quantile(0.01) > M.quantile(0.05) > M.quantile(0.3)
    assert abs(float(M.quantile(1e-4)) - 3.8906) < 5e-3      # the tail branch of the polynomial (w >= 5)


def test_model_logarithm_is_the_c_librarys_logf():
    """the model rounds the double logarithm to float32; the library calls the C library's float logarithm: the same value at the arguments the tests use"""
    libm = C.CDLL(ctypes.util.find_library("m")); libm.logf.restype = C.c_float; libm.logf.argtypes = [C.c_float]
    import math
    for p in (0.001, 0.01, 0.05, 0.1, 0.3, 0.9, 1e-4):
        x = f32(f32(-1) + f32(p)); a = f32(f32(f32(1) - x) * f32(f32(1) + x))
        assert bits(f32(libm.logf(float(a)))) == bits(f32(math.log(float(a)))), p


def test_welford_and_stop_rule_by_hand():
    """three pixels, spp 8, cap 16: constant samples stop at 8 (variance 0); alternating 0 / 1 never meets 5 % and stops at the cap; a rejected sample counts as 0"""
    k = 16; li = np.zeros((3, k, 3), f32)
    li[0] = 0.5; li[1, ::2] = 1.0; li[2] = 0.5; li[2, 3, 1] = np.nan
    n = M.counts(li, 8, 0.05, 0.5, max_sample_factor=2)
    assert n.tolist() == [8, 16, 16]
    # the same rule with a loose threshold: pixel 1 has mean 0.5, variance 8 / 15 * 0.5 ... evaluate in float32 by hand at n = 8
    lum = M.luminance(li[1, :8]); mean = f32(0); msq = f32(0)
    for i, v in enumerate(lum.tolist()):
        d = f32(f32(v) - mean); mean = f32(mean + f32(d / f32(i + 1))); msq = f32(msq + f32(d * f32(f32(v) - mean)))
    ci = f32(f32(np.sqrt(f32(f32(msq / f32(7)) / f32(8)))) * M.quantile(0.05)); base = max(mean, f32(f32(0.5) * f32(0.01)))
    loose = float(ci / base) * 1.001; tight = float(ci / base) * 0.999
    assert M.counts(li[1:2], 8, loose, 0.5, 2)[0] == 8 and M.counts(li[1:2], 8, tight, 0.5, 2)[0] > 8
    with pytest.raises(ValueError, match="have not stopped"):
        M.counts(li[1:2, :12], 8, 0.0, 0.5, max_sample_factor=-1)


@pytest.fixture(scope="module")
def cbox(mi):
    S = mi.scenes
    return S.cornell_box(16, 12, 8, sampler=S.SAMPLER_INDEPENDENT, max_depth=3)


def test_cornell_case_ends_in_all_three_ways(oracle, cbox):
    """The GPU tests' scene: 16 x 12, independent sampler, maxDepth 3, spp 8, factor 8, average luminance 0.177, maxError 0.2.  A condition on the INPUTS, not on the code
    under test: at least 20 pixels stop at spp, 20 strictly between, 20 at the cap (measured with the oracle: 35 / 83 / 74, 37 distinct counts in between)."""
    li, _ = M.oracle_samples(oracle, cbox, M.tile_pixels(0, 0, 16, 12), 64)
    n = M.counts(li, 8, 0.2, 0.177, 8)
    lo, mid, hi = int((n == 8).sum()), int(((n > 8) & (n < 64)).sum()), int((n == 64).sum())
    print(f"[adaptive] cornell 16x12: {lo} at spp, {mid} between ({len(np.unique(n[(n > 8) & (n < 64)]))} distinct), {hi} at the cap")
    assert lo >= 20 and mid >= 20 and hi >= 20 and lo + mid + hi == 192
    n5 = M.counts(li, 8, 0.5, 0.177, 8); assert (n5 <= n).all() and (n5 < n).sum() > 50      # a looser threshold never asks for more


def test_film_model_is_the_uniform_film_when_nobody_stops_early(oracle, cbox):
    """maxError 0 and factor 1: every pixel takes spp samples and the model film times spp is the oracle's film of the uniform render"""
    px = M.tile_pixels(0, 0, 16, 12); li, pos = M.oracle_samples(oracle, cbox, px, 8); orc = oracle.Oracle(cbox)
    n = M.counts(li, 8, 0.0, 0.177, 1); assert (n == 8).all()
    mine = M.film(oracle, orc, 16, 12, px, li, pos, n) * 8.0; ref, _ = orc.render_image()
    assert np.allclose(mine[..., :3], ref[..., :3], rtol=2e-6, atol=1e-6) and np.allclose(mine[..., 4], ref[..., 4], rtol=2e-6)


def test_luminance_estimate_pairs():
    p = M.luminance_estimate_pairs(16, 12); assert len(p) == 192 and (p[:, 2] == (1 << 24) - 1).all() and (p[:, 1] * 16 + p[:, 0] == np.arange(192)).all()
    p = M.luminance_estimate_pairs(160, 120); idx = p[:, 1].astype(np.int64) * 160 + p[:, 0]
    assert len(p) == 10000 and idx[0] == 0 and idx[1] == 1 and idx[-1] == (9999 * 19200) // 10000 and (np.diff(idx) >= 1).all()


def test_entry_points_are_declared_exported_and_bound(mi):
    mi.build()
    hdr = open(os.path.join(ROOT, "include", "mi355pt.h")).read(); L = C.CDLL(mi.api.LIB_PATH)
    for name in ("mi_render_set_adaptive", "mi_render_run_adaptive", "mi_render_read_sample_counts", "mi_render_adaptive_stats"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and hasattr(L, name) and name in mi.api.EXPORTS, name
    assert re.search(r"float\s+max_error,\s*p_value;\s*int32_t\s+max_sample_factor;\s*uint32_t\s+round_samples;\s*float\s+average_luminance;\s*uint32_t\s+pad\[3\];\s*}\s*mi_adaptive_params;", hdr)
    assert C.sizeof(mi.api.MiAdaptiveParams) == 32 and C.sizeof(mi.api.MiAdaptiveStats) == 40
    for m in ("set_adaptive", "run_adaptive", "sample_counts", "adaptive_stats"):
        assert callable(getattr(mi.api.Render, m))
    sig = inspect.signature(mi.api.Render.set_adaptive).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("max_error", 0.05), ("p_value", 0.05), ("max_sample_factor", 32), ("round_samples", 0), ("average_luminance", 0.0)]
    mk = open(os.path.join(ROOT, "mitsuba-im_amd", "csrc", "Makefile")).read(); assert "kernels_adaptive" in mk
    src = open(os.path.join(ROOT, "mitsuba-im_amd", "csrc", "kernels_adaptive.hip")).read()
    for k in ("k_adapt_list", "k_adapt_accumulate", "k_adapt_compact"):
        assert k + "(" in src
    # the render parameter block and the statistics block are untouched
    assert C.sizeof(mi.api.MiRenderParams) == 64 and C.sizeof(mi.api.MiStats) == 96


def test_refusals_that_need_no_device(mi):
    """null handles are refused by name before any device call"""
    L = mi.lib(); p = mi.api.MiAdaptiveParams(0.05, 0.05, 32, 0, 0.0); st = mi.api.MiAdaptiveStats(); out = np.zeros(4, np.uint32)
    for rc, name in ((L.L.mi_render_set_adaptive(None, C.byref(p)), "mi_render_set_adaptive"), (L.L.mi_render_run_adaptive(None, mi.api.MiTile(0, 0, 1, 1)), "mi_render_run_adaptive"),
                     (L.L.mi_render_read_sample_counts(None, out.ctypes.data), "mi_render_read_sample_counts"), (L.L.mi_render_adaptive_stats(None, C.byref(st)), "mi_render_adaptive_stats")):
        assert rc == 1
    assert L.L.mi_render_adaptive_stats(None, C.byref(st)) == 1 and b"mi_render_adaptive_stats" in L.L.mi_last_error()
    assert L.L.mi_render_set_adaptive(None, None) == 1 and b"mi_render_set_adaptive" in L.L.mi_last_error()


def test_command_line_options(mi, cbox):
    render = __import__("importlib").import_module("mitsuba-im_amd.render"); S = mi.scenes
    sc = render.use_adaptive(type(cbox)(cbox), 0.2, 8)
    assert sc.adaptive == dict(max_error=0.2, p_value=0.05, max_sample_factor=8) and cbox.get("adaptive") is None
    sc = render.use_adaptive(type(cbox)(cbox)); assert sc.adaptive == dict(max_error=0.05, p_value=0.05, max_sample_factor=32)
    own = type(cbox)(cbox); own.adaptive = dict(max_error=0.1, p_value=0.01, max_sample_factor=4)      # a scene file's own wrapper keeps what the command line does not give
    assert render.use_adaptive(own, None, 16).adaptive == dict(max_error=0.1, p_value=0.01, max_sample_factor=16)
    for integ in (S.INTEGRATOR_DIRECT, S.INTEGRATOR_AO):
        bad = type(cbox)(cbox); bad.integrator = integ
        with pytest.raises(ValueError, match="direct and ao are not supported"):
            render.use_adaptive(bad, 0.05)
    withf = type(cbox)(cbox); withf.fields = [("distance", (0.0, 0.0, 0.0))]
    with pytest.raises(ValueError, match="field channels"):
        render.use_adaptive(withf, 0.05)
    with pytest.raises(ValueError, match="must not be 0"):
        render.use_adaptive(type(cbox)(cbox), 0.05, 0)
    with pytest.raises(ValueError, match=">= 0"):
        render.use_adaptive(type(cbox)(cbox), -1.0)
    with pytest.raises(SystemExit, match="--sample-counts expects a .npy"):
        render.main(["none.xml", "--adaptive", "--sample-counts", "counts.txt"])
    with pytest.raises(SystemExit, match="--adaptive cannot be combined with --ao"):
        render.main(["none.xml", "--adaptive", "0.1", "--ao", "4"])
