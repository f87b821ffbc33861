"""CPU: the Python model of the ambient-occlusion integrator (tests/ao_model.py; ao.cpp:84-125) is pinned to the oracle's units before anything runs on a GPU, and the
new entry points and fields are declared, exported and bound.

No vectors compiled from the reference pin `ao`: the reference build used as a checker holds no such plugin.  What is pinned here: the 2-D request of ao(1) IS the first
request `path` makes after the pixel offset (the oracle logs the values its `path` draws), the array of ao(N) IS the emitter-side array of direct(N, 0), and the value
has the form count * (1.0f / N)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from tests.ao_model import AoModel, auto_ray_length
from tests.direct_model import DirectModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 24; SPP = 4
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def all_pairs(sc):
    return np.array([(x, y, s) for y in range(sc.height) for x in range(sc.width) for s in range(sc.spp)], np.uint32)


@pytest.fixture(scope="module")
def cbox(mi):
    return mi.scenes.cornell_box(W, H, SPP, max_depth=2)


def test_own_request_is_paths_first_request_after_the_pixel_offset(oracle, cbox):
    """N = 1: nextSample2D on the sample's own index = the third and fourth sampler values of `path` on the same (pixel, sample), wherever the camera ray hits a smooth
    diffuse surface (there `path` requests its emitter sample next: six values at maxDepth = 2)"""
    pairs = all_pairs(cbox); log = oracle.Oracle(cbox).render_samples(pairs, log=True)
    m = AoModel(oracle, cbox, 1); smooth = log["nvals"] == 6
    assert smooth.sum() > 1000
    own = np.array([m.samples2d(px, py, s)[0] for px, py, s in pairs.tolist()], f32)
    assert (bits(own[smooth]) == bits(log["vals"][smooth, 2:4])).all()


def test_array_is_the_emitter_array_of_direct(oracle, cbox):
    """N = 4: the one 2-D array at Sobol' dimensions 5 / 6, the points look_up(m * N + j)"""
    m = AoModel(oracle, cbox, 4); d = DirectModel(oracle, cbox, 4, 0); assert d.em_array_dim == 5 and d.array_end == 7
    for px, py, s in all_pairs(cbox)[::37].tolist():
        a = np.array(m.samples2d(px, py, s), f32); b = np.array(d._array(px, py, s, 4, d.em_array_dim), f32)
        assert a.shape == (4, 2) and (bits(a) == bits(b)).all()
    a = np.array(m.samples2d(3, 5, 2), f32); assert len({tuple(x) for x in a.tolist()}) == 4      # four different points


def b1(x):
    return int(np.float32(x).view(np.uint32))


@pytest.mark.parametrize("n", [1, 3, 4, 7])
def test_values_are_counts_times_the_reciprocal(mi, oracle, n):
    """k * (1.0f / N) with integer k in [0, N], and a camera miss is exactly 1 whatever the environment (sky_view: an environment map).  In float32 the product equals
    the quotient k / N for every k at N = 3 (and at 1 and 4); N = 7 is the smallest count at which the two differ (k = 3 and k = 6, in the last bit), so it is here too."""
    sc = mi.scenes.sky_view(W, H, SPP, max_depth=2); got = AoModel(oracle, sc, n).render_samples(all_pairs(sc))
    recip = f32(1) / f32(n); allowed = {b1(f32(k) * recip) for k in range(n + 1)}
    li = got["li"]; assert (bits(li[:, 0]) == bits(li[:, 1])).all() and (bits(li[:, 0]) == bits(li[:, 2])).all()
    seen = set(bits(li[got["hit"], 0]).tolist())
    assert seen <= allowed and len(seen) >= min(n, 2)
    assert (~got["hit"]).sum() > 100 and (bits(li[~got["hit"]]) == b1(1)).all()
    assert got["rays"] == len(li) and got["shadow_rays"] == n * int(got["hit"].sum())
    if n == 7:
        odd = {b1(f32(k) * recip) for k in (3, 6)}; assert odd.isdisjoint({b1(f32(k) / f32(7)) for k in range(8)}) and seen & odd
    if n == 3: assert all(b1(f32(k) * recip) == b1(f32(k) / f32(3)) for k in range(4))


def test_rays_shorter_than_epsilon_see_nothing(oracle, cbox):
    got = AoModel(oracle, cbox, 4, ray_length=5e-5).render_samples(all_pairs(cbox)[::3])
    assert (bits(got["li"]) == b1(1)).all() and got["hit"].sum() > 500


def test_occlusion_never_falls_when_the_rays_grow(oracle, cbox):
    pairs = all_pairs(cbox)[::2]
    short = AoModel(oracle, cbox, 4, ray_length=60.0).render_samples(pairs); long_ = AoModel(oracle, cbox, 4, ray_length=400.0).render_samples(pairs)
    assert not (long_["visible"] & ~short["visible"]).any()       # the same directions: a ray free at 400 is free at 60
    assert (long_["li"][:, 0] <= short["li"][:, 0]).all() and (long_["li"][:, 0] < short["li"][:, 0]).sum() > 100 and short["li"][:, 0].min() < 1


def test_automatic_length_is_half_the_bounding_sphere_radius(oracle, cbox):
    """scene.cpp:394-421 -> getBSphere().radius * 0.5f, restated here scalar by scalar in float32 from the scene arrays: the box of the vertices, enlarged as the
    kd-tree enlarges its root (gkdtree.h:1213-1220: min first, then max from the new extent), expanded by the camera position (the Cornell box has area lights only)"""
    pos = np.asarray(cbox.pos, f32).reshape(-1, 3); cam = np.asarray(cbox.cam_to_world, f32).reshape(4, 4)[:3, 3]; eps = f32(1e-3); d2 = f32(0)
    for i in range(3):
        lo, hi = f32(pos[:, i].min()), f32(pos[:, i].max())
        lo = f32(lo - f32(f32(f32(hi - lo) * eps) + eps)); hi = f32(hi + f32(f32(f32(hi - lo) * eps) + eps))
        lo, hi = min(lo, cam[i]), max(hi, cam[i])
        d = f32(f32(f32(hi + lo) * f32(0.5)) - hi); d2 = f32(d2 + f32(d * d))
    want = f32(f32(np.sqrt(d2)) * f32(0.5))
    assert bits(auto_ray_length(cbox)) == bits(want) and bits(AoModel(oracle, cbox, 1).ray_length) == bits(want) and 300 < want < 1500
    far = mi_scene_with_far_camera(cbox); assert auto_ray_length(far) > want      # the sphere depends on the camera


def mi_scene_with_far_camera(sc):
    out = type(sc)(sc); c = np.array(sc.cam_to_world, f32).reshape(4, 4).copy(); c[:3, 3] = c[:3, 3] + f32(5000); out.cam_to_world = c
    return out


def test_new_entry_points_and_fields_are_declared_exported_and_bound(mi):
    mi.build()
    hdr = open(os.path.join(ROOT, "include", "mi355pt.h")).read(); host = open(os.path.join(ROOT, "include", "mi355pt_host.h")).read()
    L = C.CDLL(mi.api.LIB_PATH)
    assert re.search(r"#define\s+MI_INTEGRATOR_AO\s+4\b", hdr) and mi.scenes.INTEGRATOR_AO == 4
    assert re.search(r"uint32_t\s+bsdf_samples;[^}]*uint32_t\s+shading_samples;[^}]*float\s+ray_length;[^}]*}\s*mi_render_params;", hdr)      # trailing, in this order
    names = [n for n, _ in mi.api.MiRenderParams._fields_]; assert names[-4:] == ["emitter_samples", "bsdf_samples", "shading_samples", "ray_length"]
    P = mi.api.MiRenderParams; assert (P.emitter_samples.offset, P.shading_samples.offset, P.ray_length.offset, C.sizeof(P)) == (48, 56, 60, 64)
    assert re.search(r"\bmi_host_create_ao\s*\(", host) and hasattr(L, "mi_host_create_ao") and "mi_host_create_ao" in mi.api.HOST_EXPORTS
    import inspect
    for cls in (mi.api.Render, mi.api.HostIntegrator):
        assert {"shading_samples", "ray_length"} <= set(inspect.signature(cls.__init__).parameters)
    mk = open(os.path.join(ROOT, "mitsuba-im_amd", "csrc", "Makefile")).read(); assert "kernels_ao" in mk
    src = open(os.path.join(ROOT, "mitsuba-im_amd", "csrc", "ao.h")).read(); assert "k_ao_resolve" in src and "k_ao(" in src
    # the host mirror refuses shadingSamples = 0 before any device work
    L.mi_host_create_ao.restype = C.c_void_p; L.mi_host_last_error.restype = C.c_char_p
    L.mi_host_create_ao.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_double]
    assert not L.mi_host_create_ao(1, 4, 0, None, 0, 0, 0, -1.0, -1.0) and b"shadingSamples" in L.mi_host_last_error()
    h = L.mi_host_create_ao(1, 4, 0, None, 0, 0, 3, -1.0, -1.0); assert h
    L.mi_host_destroy.argtypes = [C.c_void_p]; L.mi_host_destroy(h)


def test_command_line_option_puts_ao_in_place_of_the_scenes_integrator(mi, cbox):
    render = __import__("importlib").import_module("mitsuba-im_amd.render")
    sc = render.use_ao(type(cbox)(cbox), 8, 120.0)
    assert (sc.integrator, sc.shading_samples, sc.ray_length) == (mi.scenes.INTEGRATOR_AO, 8, 120.0) and cbox.integrator == mi.scenes.INTEGRATOR_PATH
    with pytest.raises(ValueError, match="shading samples"):
        render.use_ao(type(cbox)(cbox), 0)
    with pytest.raises(SystemExit):
        render.main(["none.xml", "--ao-length", "3"])
