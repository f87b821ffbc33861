"""GPU (MI355X): the thin-lens sensor (src/sensors/thinlens.cpp:324-361 behind the sample order of src/librender/integrator.cpp:166-181) through mi_scene_set_lens /
mi_scene_update_lens / mi_debug_camera_rays_lens, k_generate and the differentials of the sensor ray.

No reference-compiled vectors exist for this sensor; the checks rest on a float64 restatement of the ray written here, on pieces the suite pins elsewhere (Sobol values,
intersection records, the perspective camera) and on invariants of a lens: what lies in the focal plane does not move, what lies elsewhere moves by the aperture point."""
import copy
import os
import subprocess
import sys
import numpy as np
import pytest
from tests.conftest import GOLDEN, ROOT
from tests.test_gpu_fields import UNDEF, albedo_scene, bits, expected_from_records, np_checkerboard, np_nearest, sample_triples

pytestmark = pytest.mark.gpu
f32 = np.float32
DOF_ROW = os.path.join(GOLDEN, "scenes", "dof_row.xml")
HIT_FIELDS = ["position", "distance", "primIndex"]


def clone(sc):
    """a deep copy of a scene description (scenes.Scene answers every attribute lookup from its dict, which copy.deepcopy cannot probe)"""
    return type(sc)({k: copy.deepcopy(v) for k, v in sc.items()})


# ---------------------------------------------------------------------------------------------- restatements
def disk_concentric(a):
    """warp::squareToUniformDiskConcentric (src/libcore/warp.cpp:81-101) in float64"""
    a = np.asarray(a, np.float64); r1 = 2 * a[:, 0] - 1; r2 = 2 * a[:, 1] - 1
    first = r1 * r1 > r2 * r2; zero = (r1 == 0) & (r2 == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(first, r1, r2); phi = np.where(first, (np.pi / 4) * (r2 / r1), (np.pi / 2) - (r1 / r2) * (np.pi / 4))
    r = np.where(zero, 0.0, r); phi = np.where(zero, 0.0, phi)
    return np.stack([r * np.cos(phi), r * np.sin(phi)], 1)


def near_points(sc, pos):
    """m_sampleToCamera(pos * invResolution, 0) in float64 (homogeneous divide), and the near-plane differentials m_dx / m_dy"""
    m = np.asarray(sc.sample_to_camera, np.float64)

    def pt(x, y):
        v = np.stack([x, y, np.zeros_like(x), np.ones_like(x)], 1) @ m.T; return v[:, :3] / v[:, 3:4]
    pos = np.asarray(pos, np.float64); irx, iry = 1.0 / sc.width, 1.0 / sc.height
    z = np.zeros(1); p0 = pt(z, z)
    return pt(pos[:, 0] * irx, pos[:, 1] * iry), pt(z + irx, z)[0] - p0[0], pt(z, z + iry)[0] - p0[0]


def lens_rays64(sc, pos, aperture):
    """ThinLens::sampleRayDifferential in float64 -> origin, direction, mint, maxt, rx direction, ry direction"""
    c2w = np.asarray(sc.cam_to_world, np.float64); R, t = c2w[:3, :3], c2w[:3, 3]
    tmp = disk_concentric(aperture) * sc.aperture_radius
    near_p, dx, dy = near_points(sc, pos)
    ap = np.concatenate([tmp, np.zeros((len(tmp), 1))], 1)
    fdist = sc.focus_distance / near_p[:, 2:3]
    nrm = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    d = nrm(near_p * fdist - ap); inv_z = 1.0 / d[:, 2]
    return (ap @ R.T + t, d @ R.T, sc.near * inv_z, sc.far * inv_z, nrm((near_p + dx) * fdist - ap) @ R.T, nrm((near_p + dy) * fdist - ap) @ R.T)


def tea(v0, v1):
    """sampleTEA, 4 rounds (include/mitsuba/core/qmc.h:146-156) on uint32 arrays -> (low word, high word)"""
    v0 = v0.astype(np.uint64); v1 = v1.astype(np.uint64); M = np.uint64(0xFFFFFFFF); s = np.uint64(0)
    for _ in range(4):
        s = (s + np.uint64(0x9e3779b9)) & M
        v0 = (v0 + ((((v1 << np.uint64(4)) & M) + np.uint64(0xA341316C) & M) ^ ((v1 + s) & M) ^ (((v1 >> np.uint64(5)) + np.uint64(0xC8013EA4)) & M))) & M
        v1 = (v1 + ((((v0 << np.uint64(4)) & M) + np.uint64(0xAD90777D) & M) ^ ((v0 + s) & M) ^ (((v0 >> np.uint64(5)) + np.uint64(0x7E95761E)) & M))) & M
    return v0.astype(np.uint32), v1.astype(np.uint32)


def bits_to_float(b):
    return (((b >> np.uint32(9)) | np.uint32(0x3f800000)).view(f32) - f32(1.0)).astype(f32)


def film_and_aperture(sc, gs, pairs):
    """Film position and aperture sample of every (px, py, sample index) as k_generate draws them.  Sobol: dimensions 0 / 1 of Scene.sobol rescaled to the pixel
    (src/samplers/sobol.cpp:239-245), dimensions 2 / 3 raw.  Independent: draws 0 and 1 of the path's counter-based stream."""
    pairs = np.asarray(pairs, np.uint32); px = pairs[:, 0].astype(np.int64); py = pairs[:, 1].astype(np.int64)
    if sc.sampler == 1:
        idx, v = gs.sobol(pairs, 4); res = f32(1 << int(np.ceil(np.log2(max(sc.width, sc.height)))))
        rescale = idx != pairs[:, 2].astype(np.uint64)
        jx = np.where(rescale, (v[:, 0] * res).astype(f32) - px.astype(f32), v[:, 0]).astype(f32); jy = np.where(rescale, (v[:, 1] * res).astype(f32) - py.astype(f32), v[:, 1]).astype(f32)
        ap = np.ascontiguousarray(v[:, 2:4])
    else:
        v0 = (pairs[:, 1] * np.uint32(sc.width) + pairs[:, 0]) ^ np.uint32((sc.seed * 0x9E3779B9) & 0xFFFFFFFF); k = pairs[:, 2] << np.uint32(8)
        lo, hi = tea(v0, k); jx, jy = bits_to_float(lo), bits_to_float(hi)
        lo, hi = tea(v0, k | np.uint32(1)); ap = np.stack([bits_to_float(lo), bits_to_float(hi)], 1)
    pos = np.stack([(px.astype(f32) + jx).astype(f32), (py.astype(f32) + jy).astype(f32)], 1)
    return pos, ap


def lens_on_box_centre(mi, sc, radius_share=0.05):
    """a copy of the scene with a lens: radius = share x the diagonal of the vertex box, focal plane through the box centre"""
    sc = clone(sc); lo = sc.pos.min(0).astype(np.float64); hi = sc.pos.max(0).astype(np.float64)
    centre = np.linalg.inv(np.asarray(sc.cam_to_world, np.float64)) @ np.append((lo + hi) * 0.5, 1.0)
    assert centre[2] > 0
    return mi.scenes.with_lens(sc, radius_share * np.linalg.norm(hi - lo), centre[2])


# ---------------------------------------------------------------------------------------------- 1: the ray
def test_lens_rays_against_float64(mi, golden_scenes):
    plain = golden_scenes["cornell_small"]; sc = lens_on_box_centre(mi, plain); gs = mi.Scene(sc)
    rng = np.random.default_rng(11); n = 4096
    pos = (rng.random((n, 2)) * [sc.width, sc.height]).astype(f32); ap = rng.random((n, 2)).astype(f32)
    ap[:9] = [(0, 0), (1, 0), (0, 1), (1, 1), (0.5, 0.5), (0.5, 0.25), (0.25, 0.5), (0.75, 0.25), (0.25, 0.75)]      # corners, the r = 0 branch, both wedges and their diagonal
    got = gs.camera_rays(pos, ap, differentials=True); assert got.shape == (n, 14)
    o, d, mint, maxt, rx, ry = lens_rays64(sc, pos, ap)
    scale_o = np.abs(np.asarray(sc.cam_to_world, np.float64)[:3, 3]).max() + sc.aperture_radius
    err = {"origin": np.abs(got[:, 0:3] - o).max() / scale_o, "direction": np.abs(got[:, 4:7] - d).max(), "mint": (np.abs(got[:, 3] - mint) / mint).max(),
           "maxt": (np.abs(got[:, 7] - maxt) / maxt).max(), "rx": np.abs(got[:, 8:11] - rx).max(), "ry": np.abs(got[:, 11:14] - ry).max()}
    print("[thinlens] ray error relative to the largest magnitude:", {k: f"{v:.2e}" for k, v in err.items()})
    for k, v in err.items():
        assert v <= 1e-5, (k, v)
    # the rays really leave a disk of the lens's radius, and the differentials are not the ray
    w2c = np.linalg.inv(np.asarray(sc.cam_to_world, np.float64)); oc = got[:, 0:3].astype(np.float64) @ w2c[:3, :3].T + w2c[:3, 3]
    rad = np.hypot(oc[:, 0], oc[:, 1]); assert rad.max() > 0.95 * sc.aperture_radius and rad.max() <= sc.aperture_radius * (1 + 1e-5) and np.abs(oc[:, 2]).max() < 1e-4 * scale_o
    assert rad[4] < 1e-6 * scale_o and np.abs(got[:, 8:11] - got[:, 4:7]).max() > 1e-4
    # the 8-float entry point evaluates the aperture sample (0.5, 0.5)
    assert (bits(gs.camera_rays(pos)) == bits(gs.camera_rays(pos, np.full((n, 2), 0.5, f32)))).all()
    # without a lens: the aperture is ignored, the ray is mi_debug_camera_rays' bit for bit
    gp = mi.Scene(plain); ref = gp.camera_rays(pos); got_p = gp.camera_rays(pos, ap, differentials=True)
    assert (bits(got_p[:, :8]) == bits(ref)).all() and (bits(gp.camera_rays(pos, ap)) == bits(ref)).all()
    assert not (bits(got[:, :8]) == bits(ref)).all(1).any()


# ---------------------------------------------------------------------------------------------- 2: the render kernel draws the aperture where the reference does
def check_first_hits(mi, sc, gs, integrator, n=2000):
    pairs = sample_triples(sc, n - 4); pos, ap = film_and_aperture(sc, gs, pairs)
    recs = gs.ray_intersect(gs.camera_rays(pos, ap))
    r = mi.Render(gs, integrator=integrator, fields=[(f, UNDEF) for f in HIT_FIELDS]); got = r.field_samples(pairs)
    hit = recs["valid"] != 0; exp = expected_from_records(sc, recs)
    for i, f in enumerate(HIT_FIELDS):
        same = (bits(got[hit, i]) == bits(exp[f][hit])).all(1)
        assert same.all(), (f, int((~same).sum()), int(hit.sum()), got[hit, i][~same][:3], exp[f][hit][~same][:3])
        assert (bits(got[~hit, i]) == bits(np.asarray(UNDEF, f32))).all(), f
    assert hit.mean() > 0.2
    # not vacuous: the centre of the lens would have hit somewhere else
    mid = gs.ray_intersect(gs.camera_rays(pos)); both = hit & (mid["valid"] != 0)
    assert (bits(mid["p"][both]) != bits(recs["p"][both])).any(1).mean() > 0.9
    return hit.mean()


@pytest.mark.parametrize("sampler", ["sobol", "independent"])
@pytest.mark.parametrize("name", ["cornell_small", "atrium_small", "instanced_garden", "textured_shapes"])
def test_render_draws_the_aperture_sample(mi, golden_scenes, name, sampler):
    """position, distance, primIndex of mi_render_field_samples on a lens scene equal Scene::rayIntersect of the lens ray built from the sampler's first four values, bit
    for bit: a wrong dimension, a swapped component or a Sobol fast path that forgets dimensions 2 / 3 cannot pass.  cornell_small is traced as a packet, the others walk trees."""
    sc = lens_on_box_centre(mi, golden_scenes[name]); sc.sampler = 1 if sampler == "sobol" else 0; sc.seed = 0 if sampler == "sobol" else 5
    gs = mi.Scene(sc); share = check_first_hits(mi, sc, gs, 0)
    print(f"[thinlens] {name} {sampler}: hit share {share:.3f}")


@pytest.mark.parametrize("integrator", [1, 2])
def test_volumetric_integrators_draw_the_aperture_sample(mi, golden_scenes, integrator):
    sc = lens_on_box_centre(mi, golden_scenes["cornell_small"]); check_first_hits(mi, sc, mi.Scene(sc), integrator)


@pytest.mark.parametrize("sampler", ["sobol", "independent"])
def test_path_state_reproduces_the_aperture_sample(mi, golden_scenes, sampler):
    """mi_render_debug_sensor_differentials: after k_generate, the state words a path carries (st0.y / st0.z) give back, through lensSampleOfPath, the aperture sample the
    path was started with, bit for bit, and sensorDifferentials -- the one function behind the five users of the differentials -- returns the rx / ry directions of
    mi_debug_camera_rays_lens for that sample (spp = 1: no scaling).  Sample indices beyond spp take k_generate's slow Sobol path, the first its table path."""
    sc = lens_on_box_centre(mi, golden_scenes["cornell_small"]); sc.sampler = 1 if sampler == "sobol" else 0; sc.seed = 0 if sampler == "sobol" else 5
    gs = mi.Scene(sc); pairs = sample_triples(sc, 3000); pos, ap = film_and_aperture(sc, gs, pairs)
    got = mi.Render(gs, spp=1).sensor_differentials(pairs); rays = gs.camera_rays(pos, ap, differentials=True)
    assert (bits(got[:, :2]) == bits(ap)).all() and (bits(got[:, 2:]) == bits(rays[:, 8:])).all()
    assert len(np.unique(bits(ap), axis=0)) > 2900 and (pairs[:, 2] == 0).any() and (pairs[:, 2] > 0).any()
    plain = golden_scenes["cornell_small"]; gp = mi.Scene(plain); gotp = mi.Render(gp, spp=1).sensor_differentials(pairs)      # no lens: the centre, the perspective differentials
    assert (gotp[:, :2] == 0.5).all() and (bits(gotp[:, 2:]) == bits(gp.camera_rays(film_and_aperture(plain, gp, pairs)[0], None, differentials=True)[:, 8:])).all()


def test_dimension_budget_moves_by_two(mi, golden_scenes):
    """mi_render_create counts a path's sampler draws: 3 + 5 per bounce against the 128 loaded Sobol dimensions, 2 + 5 per bounce against the 256 draws the independent
    stream numbers.  A lens adds two to either count: the deepest Sobol render is maxDepth 24 instead of 25, and the refusals keep their names."""
    plain = golden_scenes["cornell_small"]; gp = mi.Scene(plain); gl = mi.Scene(lens_on_box_centre(mi, plain))
    mi.Render(gp, max_depth=25).close(); mi.Render(gl, max_depth=24).close()
    for scene, depth in ((gp, 26), (gl, 25)):
        with pytest.raises(mi.MiError) as e:
            mi.Render(scene, max_depth=depth)
        assert e.value.code == 1 and "Lookup dimension exceeds the direction number table size" in str(e.value)
    mi.Render(gl, max_depth=50, sampler=0).close()                                   # 4 + 250 draws
    with pytest.raises(mi.MiError) as e:
        mi.Render(gl, max_depth=51, sampler=0)
    assert e.value.code == 3 and "independent sampler stream numbers 256 draws" in str(e.value)
    # a deep lens path really reads its last dimensions: the render at the boundary runs
    r = mi.Render(gl, max_depth=24, rr_depth=24, spp=1); r.run(); assert np.isfinite(r.read_film(2)).all()


# ---------------------------------------------------------------------------------------------- 3: focus invariant
def wall_scene(S, dist, f=3.0, lens=True, textured=False, width=37, height=23, spp=5, max_depth=2, emitter="point"):
    """one rectangle facing the camera at `dist`, large enough for the view plus the aperture on every side; lens radius 0.2 f, focal plane at f"""
    b = S._Builder(); m = b.bsdf(reflectance=(0.5, 0.5, 0.5)); h = 6.0 * f
    tex = [S.make_texture(S.TEXTURE_CHECKERBOARD, (0.9, 0.8, 0.7), (0.1, 0.15, 0.2), uscale=150.0, vscale=110.0)] if textured else None
    if textured: b.bsdfs[m]["texture"] = 0
    b.begin(); b.quad([(0.3 + h, 0.2 - h, dist), (0.3 - h, 0.2 - h, dist), (0.3 - h, 0.2 + h, dist), (0.3 + h, 0.2 + h, dist)]); b.end(m)
    if emitter == "area":      # a small light above the view, facing down: outside every sensor ray, so the wall's radiance is all the film sees
        b.begin(); b.quad([(-0.2, 2.0, 1.0), (0.8, 2.0, 1.0), (0.8, 2.0, 2.0), (-0.2, 2.0, 2.0)]); b.end(b.bsdf(reflectance=(0.5, 0.5, 0.5)), radiance=(40.0, 36.0, 30.0))
    cam = S.look_at((0.3, 0.2, 0.0), (0.3, 0.2, 1.0), (0, 1, 0))
    sc = S.finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 40.0, 0.05, 100.0, width, height, spp, S.SAMPLER_SOBOL, max_depth, uvs=[(0, 0), (1, 0), (1, 1), (0, 1)] * (2 if emitter == "area" else 1), name="wall", textures=tex)
    if emitter != "area": S.add_scene_emitters(sc, [S.point_emitter((0.5, 1.0, -1.0), (20.0, 20.0, 20.0)) if emitter == "point" else S.constant_emitter((0.8, 0.9, 1.0))])
    return S.with_lens(sc, 0.2 * f, f) if lens else sc


def test_focal_plane_is_sharp_and_the_rest_moves_by_the_aperture(mi):
    S = mi.scenes; f = 3.0
    sc = wall_scene(S, f); gs = mi.Scene(sc); plain = wall_scene(S, f, lens=False); gp = mi.Scene(plain)
    yy, xx, kk = np.meshgrid(np.arange(sc.height), np.arange(sc.width), np.arange(sc.spp), indexing="ij"); pairs = np.stack([xx.ravel(), yy.ravel(), kk.ravel()], 1).astype(np.uint32)
    a = mi.Render(gs, fields=["position"]).field_samples(pairs)[:, 0]; p = mi.Render(gp, fields=["position"]).field_samples(pairs)[:, 0]
    err = np.abs(a.astype(np.float64) - p).max(); print(f"[thinlens] in focus: max |lens hit - pinhole hit| = {err / f:.2e} f")
    assert err <= 1e-5 * f
    # the wall at 2 f: in camera space 2 focusP - hit is the aperture point, radius x diskConcentric(dimensions 2 / 3)
    far = wall_scene(S, 2 * f); gf = mi.Scene(far); hit = mi.Render(gf, fields=["position"]).field_samples(pairs)[:, 0].astype(np.float64)
    pos, ap = film_and_aperture(far, gf, pairs)
    w2c = np.linalg.inv(np.asarray(far.cam_to_world, np.float64)); hc = hit @ w2c[:3, :3].T + w2c[:3, 3]
    near_p, _, _ = near_points(far, pos); focus_p = near_p * (far.focus_distance / near_p[:, 2:3])
    got = 2 * focus_p - hc; exp = np.concatenate([disk_concentric(ap) * far.aperture_radius, np.zeros((len(ap), 1))], 1)
    err = np.abs(got - exp).max(); print(f"[thinlens] at 2 f: max |2 focusP - hit - apertureP| = {err / f:.2e} f")
    assert err <= 1e-5 * f
    assert np.hypot(exp[:, 0], exp[:, 1]).max() > 0.9 * far.aperture_radius


# ---------------------------------------------------------------------------------------------- 4: the rest of the path is unbiased
@pytest.mark.parametrize("emitter", ["constant", "area"])
def test_lens_image_of_a_diffuse_wall_has_the_pinhole_expectation(mi, emitter):
    """A diffuse checkerboard wall in the focal plane: its radiance does not depend on the aperture point, so lens and pinhole image share their expectation.  Means of
    4 x 4 pixel blocks at 256 spp; sigma of a block from the per-sample values of the PINHOLE render; every block and channel within 6 sigma.  Under the `constant` emitter
    the wall is a furnace (every NEE and BSDF sample sees the same sky): the only variance is which check a film position lands on, and a block inside one check has none.
    Such a block (per-sample standard deviation within 2 ulp of its mean: nothing but float32 rounding of the one value) is compared with a rounding allowance of 2e-5
    of the value instead -- 256 float32 additions per pixel sum (256 x 2^-24 = 1.5e-5) plus the roundings of one sample; every other block gets the plain 6 sigma.  The
    `area` case (a small light outside the view) is the one where the path's later dimensions carry variance: a lens path that reused dimensions 2 / 3 for its first
    emitter sample would shift whole blocks."""
    S = mi.scenes; kw = dict(textured=True, width=32, height=24, spp=256, max_depth=3, emitter=emitter)
    lens = wall_scene(S, 3.0, **kw); plain = wall_scene(S, 3.0, lens=False, **kw)
    rl = mi.Render(mi.Scene(lens)); rl.run(); rp = mi.Render(mi.Scene(plain)); rp.run()
    il = rl.read_film(2).astype(np.float64); ip = rp.read_film(2).astype(np.float64)
    yy, xx, kk = np.meshgrid(np.arange(24), np.arange(32), np.arange(256), indexing="ij"); pairs = np.stack([xx.ravel(), yy.ravel(), kk.ravel()], 1).astype(np.uint32)
    smp = rp.samples(pairs).astype(np.float64).reshape(24, 32, 256, 3)
    blocks = lambda img: img.reshape(6, 4, 8, 4, 3).mean((1, 3))
    per_block = smp.reshape(6, 4, 8, 4, 256, 3).transpose(0, 2, 1, 3, 4, 5).reshape(6, 8, -1, 3)
    mean = per_block.mean(2); sigma = per_block.std(2, ddof=1) / np.sqrt(per_block.shape[2])
    assert np.allclose(blocks(ip), mean, rtol=2e-3) and (mean > 0.01).all()      # the film is these samples (a sample within 1e-5 of a pixel edge also lands in the neighbour: not exactly the mean)
    diff = np.abs(blocks(il) - blocks(ip)); flat = per_block.std(2, ddof=1) <= 2.0 ** -22 * mean      # no variance beyond float32 rounding
    dev = diff[~flat] / sigma[~flat]
    print(f"[thinlens] lens vs pinhole ({emitter}), 4 x 4 blocks: largest deviation {dev.max():.2f} sigma, mean {dev.mean():.2f} sigma over {int((~flat).sum())} of {flat.size} block channels; "
          f"{int(flat.sum())} without variance, largest relative difference there {(diff[flat] / mean[flat]).max() if flat.any() else 0.0:.2e}")
    assert (dev <= 6.0).all(), float(dev.max())
    assert (diff[flat] <= 2e-5 * mean[flat]).all()
    assert (~flat).mean() > 0.5 and not (bits(il) == bits(ip)).all()


# ---------------------------------------------------------------------------------------------- 5: edits
def dof_row(mi):
    xs = __import__("importlib").import_module("mitsuba-im_amd.xml_scene"); sc = xs.load_scene(DOF_ROW)
    sc.width, sc.height, sc.spp = 37, 23, 5; sc.sample_to_camera = mi.scenes.sample_to_camera(sc.xfov, sc.near, sc.far, 37 / 23)
    return sc


def film_and_counters(r):
    r.clear(); r.run(); st = r.stats(); return r.read_film(0), (st["rays"], st["shadow_rays"], st["path_length_sum"], st["samples"])


def test_update_lens_equals_a_fresh_commit(mi):
    sc = dof_row(mi); r2, f2 = 0.31, 8.5
    gs = mi.Scene(clone(sc)); r = mi.Render(gs); before, cnt_before = film_and_counters(r); rev0, builds0 = gs.revision()
    gs.update_lens(r2, f2)
    assert gs.revision() == (rev0 + 1, builds0) and (gs.sc.aperture_radius, gs.sc.focus_distance) == (r2, f2)
    with pytest.raises(mi.MiError) as e:
        r.run()                                                                      # the film still holds samples of the earlier lens
    assert e.value.code == 1
    edited, cnt_edited = film_and_counters(r)                                        # the handle created before the edit follows it after clear()
    fresh_sc = mi.scenes.with_lens(clone(sc), r2, f2); gf = mi.Scene(fresh_sc); fresh, cnt_fresh = film_and_counters(mi.Render(gf))
    assert (bits(edited) == bits(fresh)).all() and cnt_edited == cnt_fresh
    assert not (bits(edited) == bits(before)).all()
    late, cnt_late = film_and_counters(mi.Render(gs)); assert (bits(late) == bits(fresh)).all() and cnt_late == cnt_fresh
    # turning the lens off, or on, changes the sample layout: refused, nothing changes
    with pytest.raises(mi.MiError) as e:
        gs.update_lens(0.0, f2)
    assert e.value.code == 3 and str(e.value).count("mi_scene_update_lens: ") == 1 and gs.revision() == (rev0 + 1, builds0) and gs.sc.aperture_radius == r2
    again, cnt_again = film_and_counters(r); assert (bits(again) == bits(fresh)).all() and cnt_again == cnt_fresh
    pin_sc = mi.scenes.with_lens(clone(sc), 0.0, 0.0); gp = mi.Scene(pin_sc); rp = mi.Render(gp); pin, cnt_pin = film_and_counters(rp)
    with pytest.raises(mi.MiError) as e:
        gp.update_lens(0.1, 4.0)
    assert e.value.code == 3 and "mi_scene_update_lens: " in str(e.value) and gp.revision()[0] == 0 and gp.sc.aperture_radius == 0.0
    pin2, cnt_pin2 = film_and_counters(rp); assert (bits(pin2) == bits(pin)).all() and cnt_pin2 == cnt_pin
    with pytest.raises(mi.MiError) as e:
        gs.update_lens(-1.0, f2)
    assert e.value.code == 1
    # a camera edit keeps the lens
    S = mi.scenes; c2w = S.look_at((0.8, 1.5, -5.5), (0, 0.6, 0), (0, 1, 0))
    gs.update_camera(sc.sample_to_camera, c2w, sc.near, sc.far); moved, cnt_moved = film_and_counters(r)
    fresh_sc.cam_to_world = c2w; moved_fresh, cnt_moved_fresh = film_and_counters(mi.Render(mi.Scene(fresh_sc)))
    assert (bits(moved) == bits(moved_fresh)).all() and cnt_moved == cnt_moved_fresh
    # the host mirror
    gh = mi.Scene(clone(sc)); hi = mi.api.HostIntegrator(gh, devices=(0,)); hi.set_lens(r2, f2)
    assert gh.revision()[0] == 1 and gh.sc.aperture_radius == r2
    via_host, cnt_host = film_and_counters(mi.Render(gh)); assert (bits(via_host) == bits(fresh)).all() and cnt_host == cnt_fresh
    with pytest.raises(RuntimeError, match="mi_scene_update_lens"):
        hi.set_lens(0.0, 1.0)
    hi.close()


# ---------------------------------------------------------------------------------------------- 6: textured first hit
def test_albedo_of_the_lens_hit(mi):
    """The albedo field of a lens scene = the texture at the uv of the lens ray's hit, with test_gpu_fields.py::test_albedo's comparisons on its scene and a lens.  The
    field looks textures up UNFILTERED (field.cpp hands getDiffuseReflectance an intersection without uv partials) and refuses scenes that hold a plastic, as
    textured_shapes does -- so this says nothing about differentials; test_filtered_texture_of_a_real_lens below is the check of the partials."""
    S = mi.scenes; sc, m = albedo_scene(S); sc = lens_on_box_centre(mi, sc, 0.03); gs = mi.Scene(sc); pairs = sample_triples(sc, 4000)
    pos, ap = film_and_aperture(sc, gs, pairs); recs = gs.ray_intersect(gs.camera_rays(pos, ap))
    got = mi.Render(gs, fields=[("albedo", UNDEF)]).field_samples(pairs)[:, 0]
    hit = recs["valid"] != 0; mat = recs["material"]; u = recs["uv"][:, 0].astype(f32); v = recs["uv"][:, 1].astype(f32)
    assert (bits(got[~hit]) == bits(np.asarray(UNDEF, f32))).all()
    sel = {k: hit & (mat == m[k]) for k in ["const", "checker", "bitmap", "conductor"]}
    for k, s in sel.items():
        assert s.mean() > 0.02, k
    assert (bits(got[sel["const"]]) == bits(np.asarray(sc.bsdfs[m["const"]]["reflectance"], f32))).all()
    assert (bits(got[sel["checker"]]) == bits(np_checkerboard(sc.textures[0], u[sel["checker"]], v[sel["checker"]]))).all()
    exp = np_nearest(sc, sc.textures[1], u[sel["bitmap"]], v[sel["bitmap"]])
    assert (bits(got[sel["bitmap"]]) == bits(exp)).all() and len(np.unique(bits(exp), axis=0)) > 20
    assert (bits(got[sel["conductor"]]) == 0).all()
    inv_pi = np.float64(f32(0.31830988618379067154)); pi = np.float64(f32(3.14159265358979323846)); refl = lambda k: np.asarray(sc.bsdfs[m[k]]["reflectance"], f32).astype(np.float64)
    within_4ulp = lambda g, e: (np.abs(g.astype(np.float64) - e) <= 4 * np.spacing(np.abs(np.broadcast_to(e, g.shape)).astype(f32)).astype(np.float64)).all()
    for k in ("mask", "mixture"):
        assert (hit & (mat == m[k])).mean() > 0.02, k
    assert within_4ulp(got[hit & (mat == m["mask"])], (refl("under_mask") * inv_pi) * refl("mask") * pi)
    w = [np.float64(f32(x)) for x in (0.3, 0.5)]
    assert within_4ulp(got[hit & (mat == m["mixture"])], ((refl("child0") * inv_pi) * w[0] + (refl("child1") * inv_pi) * w[1]) * pi)


# ---------------------------------------------------------------------------------------------- 6a: the filtered lookup of a lens that moves rays
def np_texel(sc, t, level, x, y):
    """TMIPMap::evalTexel with repeat wrapping -> float64 [n, 3]"""
    w, h, off = (int(v) for v in sc.texture_levels[t["first_level"] + level]); assert t["wrap_u"] == 1 and t["wrap_v"] == 1
    return np.asarray(sc.texture_texels[off:off + w * h * 3], np.float64).reshape(h, w, 3)[np.mod(y, h), np.mod(x, w)]


def np_bilinear(sc, t, level, uvx, uvy):
    """TMIPMap::evalBilinear (mipmap.h:572-596; beyond the last level: evalBox of the last) in float64, per-sample integer `level`"""
    out = np.zeros((len(uvx), 3))
    for lv in np.unique(level):
        s = level == lv; u, v = uvx[s], uvy[s]
        if lv >= t["n_levels"]:
            w, h, _ = (int(q) for q in sc.texture_levels[t["first_level"] + t["n_levels"] - 1])
            out[s] = np_texel(sc, t, t["n_levels"] - 1, np.floor(u * w).astype(np.int64), np.floor(v * h).astype(np.int64)); continue
        w, h, _ = (int(q) for q in sc.texture_levels[t["first_level"] + int(lv)]); u = u * w - 0.5; v = v * h - 0.5
        x = np.floor(u).astype(np.int64); y = np.floor(v).astype(np.int64); dx1 = (u - x)[:, None]; dy1 = (v - y)[:, None]; tx = lambda a, b: np_texel(sc, t, int(lv), a, b)
        out[s] = tx(x, y) * (1 - dx1) * (1 - dy1) + tx(x, y + 1) * (1 - dx1) * dy1 + tx(x + 1, y) * dx1 * (1 - dy1) + tx(x + 1, y + 1) * dx1 * dy1
    return out


def np_trilinear(sc, t, uvx, uvy, pa):
    """TMIPMap::eval with the trilinear filter (mipmap.h:625-705; csrc/pt_device.h mipEval) in float64; pa = (dudx, dvdx, dudy, dvdy) of the uv BEFORE the texture's scale"""
    w0, h0, _ = (float(q) for q in sc.texture_levels[t["first_level"]])
    du0 = pa[:, 0] * t["uscale"] * w0; dv0 = pa[:, 1] * t["vscale"] * h0; du1 = pa[:, 2] * t["uscale"] * w0; dv1 = pa[:, 3] * t["vscale"] * h0
    A = dv0 * dv0 + dv1 * dv1; B = -2.0 * (du0 * dv0 + du1 * dv1); Cc = du0 * du0 + du1 * du1; F = A * Cc - B * B * 0.25
    ap = 0.5 * (A + Cc - np.hypot(A - Cc, B))
    with np.errstate(divide="ignore", invalid="ignore"):
        major = np.where(ap != 0, np.sqrt(F / ap), 0.0)
    level = np.log2(np.maximum(major, 1e-4)); il = np.floor(level).astype(np.int64); a = (level - il)[:, None]
    lo = np_bilinear(sc, t, np.maximum(il, 0), uvx, uvy); hi = np_bilinear(sc, t, np.maximum(il, 0) + 1, uvx, uvy)
    return np.where((il < 0)[:, None], np_bilinear(sc, t, np.zeros_like(il), uvx, uvy), lo * (1 - a) + hi * a), level


def np_partials(p, ng, dpdu, dpdv, o, rxd, ryd):
    """Intersection::computePartials (src/librender/intersection.cpp:5-76) in float64 -> (dudx, dvdx, dudy, dvdy)"""
    dot = lambda a, b: (a * b).sum(1); pp = dot(ng, p); po = dot(ng, o)
    tx = ((pp - po) / dot(ng, rxd))[:, None]; ty = ((pp - po) / dot(ng, ryd))[:, None]
    ax = np.abs(ng); n = len(p); r = np.arange(n)
    a0 = np.where((ax[:, 0] > ax[:, 1]) & (ax[:, 0] > ax[:, 2]), 1, 0); a1 = np.where((ax[:, 0] > ax[:, 1]) & (ax[:, 0] > ax[:, 2]), 2, np.where(ax[:, 1] > ax[:, 2], 2, 1))
    px = o + rxd * tx; py = o + ryd * ty
    A00, A01, A10, A11 = dpdu[r, a0], dpdv[r, a0], dpdu[r, a1], dpdv[r, a1]
    Bx0, Bx1, By0, By1 = px[r, a0] - p[r, a0], px[r, a1] - p[r, a1], py[r, a0] - p[r, a0], py[r, a1] - p[r, a1]
    inv = 1.0 / (A00 * A11 - A01 * A10)
    return np.stack([(A11 * Bx0 - A01 * Bx1) * inv, (A00 * Bx1 - A10 * Bx0) * inv, (A11 * By0 - A01 * By1) * inv, (A00 * By1 - A10 * By0) * inv], 1)


@pytest.mark.parametrize("integrator", [0, 1, 2])
def test_filtered_texture_of_a_real_lens(mi, integrator):
    """The tilted bitmap wall of ewa_wall under its point light, trilinear filter, through a lens of radius 0.15 focused in front of it: Li = filtered texture x a
    lighting term that depends on the ray alone.  The same scene with the `nearest` filter has the same rays and the same lighting term, so per sample and channel
    Li_trilinear x c_nearest = Li_nearest x c_trilinear, with c_nearest the texel at the hit's uv (np_nearest, bit-exact in test_albedo) and c_trilinear a float64
    restatement of computePartials + TMIPMap::eval fed with the differentials of Scene.camera_rays(pos, aperture, differentials=True) scaled by 1 / sqrt(spp) -- the
    aperture being the one the test derives from the sampler (film_and_aperture), which the shading kernels have to recompute from the path's state.
    Tolerance 2e-3 of the largest texel: the partials are float32 differences of hit points ~1e-2 apart at coordinates ~5 (relative error ~5e-5), the MIP level inherits
    that, the lookup moves by at most that times the contrast between levels; a factor of 40 of room.  The lookup with the aperture held at (0.5, 0.5) instead must
    miss that tolerance on a fair share of the samples: the check can tell a wrong aperture from the right one."""
    S = mi.scenes; pairs = sample_triples(ewa_wall(S), 1500); lens = lambda f: S.with_lens(ewa_wall(S, f), 0.15, 3.0)
    sc = lens(S.MIP_TRILINEAR); gs = mi.Scene(sc); near = lens(S.MIP_NEAREST); gn = mi.Scene(near); t = sc.textures[0]
    li = mi.Render(gs, integrator=integrator).samples(pairs).astype(np.float64); li_n = mi.Render(gn, integrator=integrator).samples(pairs).astype(np.float64)
    pos, ap = film_and_aperture(sc, gs, pairs); uvt = gs.read_geometry("tri_uv").view(f32).astype(np.float64); scale = 1.0 / np.sqrt(np.float64(sc.spp))

    def lookup(aperture):
        rays = gs.camera_rays(pos, aperture, differentials=True).astype(np.float64); recs = gs.ray_intersect(rays[:, :8].astype(f32))
        d = rays[:, 4:7]; rxd = d + (rays[:, 8:11] - d) * scale; ryd = d + (rays[:, 11:14] - d) * scale; prim = recs["prim"].astype(np.int64) * (recs["valid"] != 0)
        pa = np_partials(recs["p"].astype(np.float64), recs["ng"].astype(np.float64), uvt[prim, 6:9], uvt[prim, 9:12], rays[:, 0:3], rxd, ryd)
        uvx = recs["uv"][:, 0].astype(np.float64) * t["uscale"] + t["uoffset"]; uvy = recs["uv"][:, 1].astype(np.float64) * t["vscale"] + t["voffset"]
        c, level = np_trilinear(sc, t, uvx, uvy, pa); return recs, c, level
    recs, c_tri, level = lookup(ap); hit = (recs["valid"] != 0) & (li_n > 0).all(1)
    c_near = np_nearest(near, near.textures[0], recs["uv"][:, 0].astype(f32), recs["uv"][:, 1].astype(f32)).astype(np.float64)
    tol = 2e-3 * float(np.asarray(sc.texture_texels).max())
    err = lambda c: (np.abs(li * c_near - li_n * c) / np.where(li_n > 0, li_n, 1.0)).max(1)      # |c_device - c| with c_device = Li / (Li_nearest / c_nearest): largest channel, texel units
    e = err(c_tri)[hit]; _, c_mid, _ = lookup(None); e_mid = err(c_mid)[hit]
    print(f"[thinlens] filtered lookup, integrator {integrator}: {int(hit.sum())} lit hits, MIP level {level[hit].min():.2f} .. {level[hit].max():.2f}, max |device - restatement| {e.max():.2e} "
          f"(tolerance {tol:.2e}); with the aperture held at the lens centre: {(e_mid > tol).mean():.2f} of the samples beyond it")
    assert hit.mean() > 0.5 and level[hit].max() > 0.5 and level[hit].min() < level[hit].max() - 0.5
    assert (e <= tol).all(), float(e.max())
    assert (e_mid > tol).mean() > 0.2


# ---------------------------------------------------------------------------------------------- 6b: the differentials inside the shading kernels
def degenerate_lens(mi, sc):
    """A lens that cannot move a ray: radius 1e-30 is absorbed by every sum it enters, and focus distance = near clip x 2^k scales the near-plane point exactly, so ray and
    differentials keep the perspective camera's bits -- while every kernel takes its lens branch."""
    return mi.scenes.with_lens(clone(sc), 1e-30, float(f32(sc.near)) * 64.0)


def ewa_wall(S, filter_type=None):
    """a tilted quad with an EWA-filtered bitmap under one point light, maxDepth 2: Li = filtered texture x the point light's term -- a function of the sensor ray and
    its differentials alone (a single point light is sampled the same whatever the sample values), so shifting the sampler's dimensions by two cannot change it"""
    b = S._Builder(); m = b.bsdf(reflectance=(0.5, 0.5, 0.5)); b.bsdfs[m]["texture"] = 0
    tex = [S.make_texture(S.TEXTURE_BITMAP, pyramid=S.load_texture_pyramid(), uscale=6.0, vscale=5.0, filter_type=S.MIP_EWA if filter_type is None else filter_type)]
    b.begin(); b.quad([(4, -3, 2.0), (-4, -3, 5.0), (-4, 3, 6.0), (4, 3, 3.0)]); b.end(m)
    cam = S.look_at((0.3, 0.2, -1.0), (0.1, 0.0, 1.0), (0, 1, 0))
    sc = S.finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 50.0, 0.05, 100.0, 37, 23, 5, S.SAMPLER_SOBOL, 2, uvs=[(0, 0), (1, 0), (1, 1), (0, 1)], name="ewa_wall", textures=tex)
    return S.add_scene_emitters(sc, [S.point_emitter((0.5, 1.0, -2.0), (30.0, 30.0, 30.0))])


@pytest.mark.parametrize("integrator", [0, 1, 2])
def test_degenerate_lens_keeps_the_filtered_texture_lookup(mi, integrator):
    S = mi.scenes; plain = ewa_wall(S); lens = degenerate_lens(mi, plain); pairs = sample_triples(plain, 3000)
    gp = mi.Scene(plain); gl = mi.Scene(lens)
    pos, ap = film_and_aperture(lens, gl, pairs)
    assert (bits(gl.camera_rays(pos, ap, differentials=True)) == bits(gp.camera_rays(pos, None, differentials=True))).all()      # the premise
    a = mi.Render(gl, integrator=integrator).samples(pairs); p = mi.Render(gp, integrator=integrator).samples(pairs)
    assert (bits(a) == bits(p)).all(), int((bits(a) != bits(p)).any(1).sum())
    assert len(np.unique(bits(p), axis=0)) > 500 and (p > 0).any(1).mean() > 0.5


@pytest.mark.parametrize("integrator", [0, 1])
def test_degenerate_lens_keeps_the_filtered_sky_lookup(mi, golden_scenes, integrator):
    """maxDepth 1: a sensor ray that leaves the scene gets the EWA-filtered environment lookup from its differentials and nothing else (k_env_primary / the volumetric stages)"""
    plain = clone(golden_scenes["sky_view"]); plain.max_depth = 1; lens = degenerate_lens(mi, plain); pairs = sample_triples(plain, 3000)
    a = mi.Render(mi.Scene(lens), integrator=integrator).samples(pairs); p = mi.Render(mi.Scene(plain), integrator=integrator).samples(pairs)
    assert (bits(a) == bits(p)).all() and (p > 0).any(1).mean() > 0.05


# ---------------------------------------------------------------------------------------------- 7: command line
def test_render_cli_focus_pull(mi, tmp_path):
    out = str(tmp_path / "pull.exr"); env = dict(os.environ); env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    subprocess.run([sys.executable, "-m", "mitsuba-im_amd.render", DOF_ROW, "-o", out, "--spp", "2", "--focus-pull", "3", "--focus-from", "3.5", "--focus-to", "9"], check=True, cwd=ROOT, env=env, timeout=300)
    names = sorted(p.name for p in tmp_path.glob("pull_*.exr")); assert names == ["pull_000.exr", "pull_001.exr", "pull_002.exr"]
    imageio = __import__("importlib").import_module("mitsuba-im_amd.imageio"); xs = __import__("importlib").import_module("mitsuba-im_amd.xml_scene")
    def rgb_of(path):
        pix, chan = imageio.read_exr(path); return np.stack([pix[..., list(chan).index(c)] for c in "RGB"], 2)
    frames = [rgb_of(str(tmp_path / n)) for n in names]
    sc = xs.load_scene(DOF_ROW); sc.spp = 2; mi.scenes.with_lens(sc, sc.aperture_radius, 3.5)
    r = mi.Render(mi.Scene(sc)); r.run(); rgb = r.read_film(2)
    assert (bits(frames[0]) == bits(rgb)).all()
    assert not (bits(frames[1]) == bits(frames[0])).all() and not (bits(frames[2]) == bits(frames[1])).all()
