"""GPU (MI355X): field channels -- the reference's `multichannel` integrator with nested `field` integrators (src/integrators/misc/multichannel.cpp:164-221,
src/integrators/misc/field.cpp:124-177) through mi_render_set_fields / mi_render_field_samples / mi_render_read_fields (include/mi355pt.h, csrc/kernels_field.hip).

Every expected value is derived from pieces the suite already pins bit for bit against the oracle: the film positions of the samples (Oracle.render_samples "pos"),
the camera rays (Scene.camera_rays) and the full intersection records (Scene.ray_intersect, test_scene_ray_intersect_full_records)."""
import os
import subprocess
import sys
import numpy as np
import pytest
from tests import adaptive_model as AM
from tests import film_model as FM
from tests.conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
f32 = np.float32
UNDEF = (-1.0, 2.5, 7.0)
RECORD_FIELDS = ["position", "distance", "geoNormal", "shNormal", "uv", "primIndex", "shapeIndex"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def sample_triples(sc, n, seed=7):
    """n random (px, py, sampleIndex) triples plus the four film corners"""
    rng = np.random.default_rng(seed)
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    corners = np.array([(0, 0, 0), (sc.width - 1, 0, sc.spp - 1), (0, sc.height - 1, 0), (sc.width - 1, sc.height - 1, sc.spp - 1)], np.uint32)
    return np.concatenate([pairs, corners])


def records_of(mi, oracle, sc, gs, pairs):
    """the pinned pieces: oracle film positions -> device camera rays -> device intersection records"""
    pos = oracle.Oracle(sc).render_samples(pairs)["pos"]
    return pos, gs.ray_intersect(gs.camera_rays(pos))


def expected_from_records(sc, recs):
    """name -> [n, 3] values of the record-derived fields on the hits"""
    n = len(recs); n_tris = len(sc.idx); prim = recs["prim"].astype(np.int64); tri = prim < n_tris
    first = np.array([s["first_tri"] for s in sc.shapes], np.int64); ts = sc.tri_shape.astype(np.int64)
    safe = np.where(tri, prim, 0)
    prim_index = np.where(tri, safe - first[ts[safe]], 0).astype(f32)
    shape_index = np.where(recs["instance"] >= 0, -1, np.where(tri, ts[safe], len(sc.shapes) + (prim - n_tris))).astype(f32)
    rep = lambda a: np.repeat(np.asarray(a, f32).reshape(n, 1), 3, 1)
    return {"position": recs["p"], "distance": rep(recs["t"]), "geoNormal": recs["ng"], "shNormal": recs["ns"],
            "uv": np.concatenate([recs["uv"], np.zeros((n, 1), f32)], 1), "primIndex": rep(prim_index), "shapeIndex": rep(shape_index)}


# ---------------------------------------------------------------------------------------------- 1: per-sample values against the pinned pieces
@pytest.mark.parametrize("name,fused", [("cornell_small", False), ("cbox_shapes", False), ("instanced_garden", False), ("textured_shapes", False), ("atrium_small", False),
                                        ("atrium_small", True), ("sky_view", False), ("fog_box", False), ("fog_sky", False)])
def test_field_samples_equal_the_intersection_records(mi, oracle, golden_scenes, name, fused, monkeypatch):
    """Hits: position, distance, geoNormal, shNormal, uv, primIndex, shapeIndex of mi_render_field_samples equal the fields of Scene::rayIntersect's record of the same
    camera ray bit for bit (primIndex = triangle index within its mesh, 0 on analytic shapes; shapeIndex = mesh / analytic shape index, -1 through an instance); misses
    equal `undefined` bit for bit.  `fused`: no packet, 4-wide nodes -- the fused tree walk (trace_fused.h) feeds the field stage."""
    if fused:
        monkeypatch.setenv("MI355PT_NO_PACKET", "1"); monkeypatch.setenv("MI355PT_BVH2", "0")
    sc = golden_scenes[name]; gs = mi.Scene(sc); pairs = sample_triples(sc, 4000)
    pos, recs = records_of(mi, oracle, sc, gs, pairs)
    r = mi.Render(gs, fields=[(f, UNDEF) for f in RECORD_FIELDS]); got = r.field_samples(pairs)
    assert got.shape == (len(pairs), len(RECORD_FIELDS), 3) and r.field_names == RECORD_FIELDS
    hit = recs["valid"] != 0; exp = expected_from_records(sc, recs)
    print(f"[fields] {name} fused={fused}: hit share {hit.mean():.3f}, instance share {(recs['instance'][hit] >= 0).mean() if hit.any() else 0:.3f}")
    for i, f in enumerate(RECORD_FIELDS):
        same = (bits(got[hit, i]) == bits(exp[f][hit])).all(1)
        assert same.all(), (f, int((~same).sum()), got[hit, i][~same][:3], exp[f][hit][~same][:3])
        assert (bits(got[~hit, i]) == bits(np.asarray(UNDEF, f32))).all(), f
    # conditions that keep the test from passing vacuously
    assert hit.mean() > 0.20
    if name in ("cbox_shapes", "instanced_garden", "textured_shapes", "sky_view", "fog_sky"): assert (~hit).mean() > 0.05
    if name == "instanced_garden": assert (recs["instance"] >= 0).mean() > 0.10
    if name in ("cbox_shapes", "textured_shapes"): assert (recs["prim"][hit] >= len(sc.idx)).any()          # analytic shapes are hit


# ---------------------------------------------------------------------------------------------- 2: relPosition
@pytest.mark.parametrize("name", ["cornell_small", "instanced_garden"])
def test_rel_position(mi, golden_scenes, name):
    """relPosition = M p with M = the float64 inverse of the camera's world transform rounded to float32; per component |err| <= 4 * 2^-23 * (sum_j |m_ij p_j| + |m_i3|),
    the rounding bound of a four-term float32 sum (no contraction)."""
    sc = golden_scenes[name]; gs = mi.Scene(sc); pairs = sample_triples(sc, 4000)
    r = mi.Render(gs, fields=[("relPosition", UNDEF), ("position", UNDEF)]); got = r.field_samples(pairs)
    hit = ~(bits(got[:, 1]) == bits(np.asarray(UNDEF, f32))).all(1); assert hit.mean() > 0.2
    M = np.linalg.inv(np.asarray(sc.cam_to_world, np.float64)).astype(f32).astype(np.float64)[:3]
    p = got[hit, 1].astype(np.float64); rel = got[hit, 0].astype(np.float64)
    exp = p @ M[:, :3].T + M[:, 3]
    bound = 4 * 2.0 ** -23 * (np.abs(p)[:, None, :] * np.abs(M[:, :3])[None]).sum(2) + 4 * 2.0 ** -23 * np.abs(M[:, 3])
    err = np.abs(rel - exp)
    print(f"[fields] relPosition {name}: max err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), float((err / bound).max())
    assert (bits(got[~hit, 0]) == bits(np.asarray(UNDEF, f32))).all()


# ---------------------------------------------------------------------------------------------- 3: albedo
def albedo_scene(S):
    """six unit quads in a wall facing the camera: constant diffuse, checkerboard diffuse, nearest-filtered bitmap diffuse (mirror / clamp wrapping, uv beyond [0, 1]),
    twosided conductor, mask (constant opacity) over a diffuse, mixture of two diffuse records; a small area light above"""
    b = S._Builder(); uvs = []
    pyr = S.load_texture_pyramid()
    tex = [S.make_texture(S.TEXTURE_CHECKERBOARD, (0.8, 0.75, 0.6), (0.15, 0.2, 0.3), uscale=5.0, vscale=3.0, uoffset=0.13, voffset=-0.2),
           S.make_texture(S.TEXTURE_BITMAP, pyramid=pyr, uscale=1.7, vscale=1.3, uoffset=-0.4, voffset=0.2, wrap_u=S.WRAP_MIRROR, wrap_v=S.WRAP_CLAMP, filter_type=S.MIP_NEAREST)]
    m = {}
    m["const"] = b.bsdf(reflectance=(0.2, 0.5, 0.7))
    m["checker"] = b.bsdf(reflectance=(0.5, 0.5, 0.5)); b.bsdfs[m["checker"]]["texture"] = 0
    m["bitmap"] = b.bsdf(reflectance=(0.5, 0.5, 0.5)); b.bsdfs[m["bitmap"]]["texture"] = 1
    m["conductor"] = b.bsdf(kind=S.BSDF_CONDUCTOR, twosided=True, eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.2))
    m["under_mask"] = b.bsdf(reflectance=(0.5, 0.4, 0.3))
    m["mask"] = b.bsdf(kind=S.BSDF_MASK, reflectance=(0.6, 0.7, 0.8), nested=m["under_mask"])
    m["child0"] = b.bsdf(reflectance=(0.9, 0.1, 0.3)); m["child1"] = b.bsdf(reflectance=(0.05, 0.6, 0.45))
    m["mixture"] = b.bsdf(kind=S.BSDF_MIXTURE, nested=[m["child0"], m["child1"]], weights=[0.3, 0.5])
    m["light"] = b.bsdf(reflectance=(0.5, 0.5, 0.5))
    uv_quad = [(-0.3, -0.2), (1.6, -0.2), (1.6, 1.4), (-0.3, 1.4)]
    for i, key in enumerate(["const", "checker", "bitmap", "conductor", "mask", "mixture"]):
        x0 = -1.5 + (i % 3); y0 = float(i // 3)
        b.begin(); b.quad([(x0 + 1, y0, 0), (x0, y0, 0), (x0, y0 + 1, 0), (x0 + 1, y0 + 1, 0)]); uvs.extend(uv_quad); b.end(m[key])
    b.begin(); b.quad([(0.5, 2.5, -1), (0.5, 2.5, -2), (-0.5, 2.5, -2), (-0.5, 2.5, -1)]); uvs.extend([(0, 0)] * 4); b.end(m["light"], radiance=(10.0, 10.0, 10.0))
    cam = S.look_at((0.0, 1.0, -3.2), (0.0, 1.0, 0.0), (0, 1, 0))
    sc = S.finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 60.0, 0.05, 100.0, 48, 32, 8, S.SAMPLER_SOBOL, 4, uvs=uvs, name="albedo_wall", textures=tex)
    return sc, m


def np_checkerboard(t, u, v):
    """Checkerboard::eval under Texture2D::eval (csrc/pt_device.h textureEval) in float32"""
    uvx = (u * f32(t["uscale"]) + f32(t["uoffset"])).astype(f32); uvy = (v * f32(t["vscale"]) + f32(t["voffset"])).astype(f32)
    a = np.fmod(np.trunc(uvx * f32(2)).astype(np.int64), 2); b = np.fmod(np.trunc(uvy * f32(2)).astype(np.int64), 2); a[a < 0] += 2; b[b < 0] += 2
    first = (2 * a - 1) * (2 * b - 1) == 1
    return np.where(first[:, None], np.asarray(t["color0"], f32)[None], np.asarray(t["color1"], f32)[None])


def np_nearest(sc, t, u, v):
    """TMIPMap::evalBox at level 0 (mipmap.h:562-566) with the texture's wrap modes, in float32"""
    w, h, off = (int(x) for x in sc.texture_levels[t["first_level"]])
    uvx = (u * f32(t["uscale"]) + f32(t["uoffset"])).astype(f32); uvy = (v * f32(t["vscale"]) + f32(t["voffset"])).astype(f32)
    x = np.floor(uvx * f32(w)).astype(np.int64); y = np.floor(uvy * f32(h)).astype(np.int64)

    def wrap(i, n, mode):
        if mode == 1: return np.mod(i, n)
        if mode == 0: return np.clip(i, 0, n - 1)
        assert mode == 2
        j = np.mod(i, 2 * n); return np.where(j >= n, 2 * n - j - 1, j)
    x = wrap(x, w, t["wrap_u"]); y = wrap(y, h, t["wrap_v"])
    tex = np.asarray(sc.texture_texels[off:off + w * h * 3], f32).reshape(h, w, 3)
    return tex[y, x]


def test_albedo(mi, oracle, golden_scenes):
    """albedo = its.shape->getBSDF()->getDiffuseReflectance(its) restated in numpy from the material table and the record's uv: texture lookups bit-equal (constant,
    checkerboard, nearest texel with its wrap modes), the conductor exactly 0, mask and mixture within 4 ulp of the float64 value of the generic rule
    (src/librender/bsdf.cpp:82-86: eval at wi = wo = (0, 0, 1) times pi; at most four roundings).  plastic: refused by name, the other fields still work."""
    S = mi.scenes; sc, m = albedo_scene(S); gs = mi.Scene(sc); pairs = sample_triples(sc, 4000)
    pos, recs = records_of(mi, oracle, sc, gs, pairs)
    r = mi.Render(gs, fields=[("albedo", UNDEF)]); got = r.field_samples(pairs)[:, 0]
    hit = recs["valid"] != 0; mat = recs["material"]; u = recs["uv"][:, 0].astype(f32); v = recs["uv"][:, 1].astype(f32)
    assert (bits(got[~hit]) == bits(np.asarray(UNDEF, f32))).all()
    sel = {k: hit & (mat == m[k]) for k in ["const", "checker", "bitmap", "conductor", "mask", "mixture"]}
    for k, s in sel.items():
        print(f"[fields] albedo {k}: share {s.mean():.3f}"); assert s.mean() > 0.02, k
    refl = lambda k: np.asarray(sc.bsdfs[m[k]]["reflectance"], f32)
    assert (bits(got[sel["const"]]) == bits(refl("const"))).all()
    assert (bits(got[sel["checker"]]) == bits(np_checkerboard(sc.textures[0], u[sel["checker"]], v[sel["checker"]]))).all()
    exp = np_nearest(sc, sc.textures[1], u[sel["bitmap"]], v[sel["bitmap"]])
    assert (bits(got[sel["bitmap"]]) == bits(exp)).all()
    assert len(np.unique(bits(exp), axis=0)) > 20                                     # many different texels were looked up
    assert (bits(got[sel["conductor"]]) == 0).all()
    inv_pi = np.float64(f32(0.31830988618379067154)); pi = np.float64(f32(3.14159265358979323846))

    def within_4ulp(g, e64):
        e = np.broadcast_to(e64, g.shape); return (np.abs(g.astype(np.float64) - e) <= 4 * np.spacing(np.abs(e).astype(f32)).astype(np.float64)).all()
    e_mask = (refl("under_mask").astype(np.float64) * inv_pi) * refl("mask").astype(np.float64) * pi
    assert within_4ulp(got[sel["mask"]], e_mask), (got[sel["mask"]][:2], e_mask)
    w = [np.float64(f32(x)) for x in (0.3, 0.5)]
    e_mix = ((refl("child0").astype(np.float64) * inv_pi) * w[0] + (refl("child1").astype(np.float64) * inv_pi) * w[1]) * pi
    assert within_4ulp(got[sel["mixture"]], e_mix), (got[sel["mixture"]][:2], e_mix)
    # refused BSDFs: by name, and only the albedo field
    rp = mi.Render(mi.Scene(golden_scenes["cbox_materials"]))
    assert any(b["type"] == S.BSDF_PLASTIC for b in golden_scenes["cbox_materials"].bsdfs)
    with pytest.raises(mi.MiError) as e:
        rp.set_fields(["albedo"])
    assert e.value.code == 3 and "plastic" in str(e.value)
    rp.set_fields(["shNormal"]); assert rp.field_samples(pairs[:8] % 8).shape == (8, 1, 3)


# ---------------------------------------------------------------------------------------------- 4 / 5: the field film
FILM_FIELDS = ["shNormal", "distance", "position"]
_film_cache = {}


def film_case(mi, oracle, name, filt):
    """scene (film 37 x 23, 5 spp), its Scene handle, and the field film restated with float64 sums (tests/film_model.py put64): every sample's values from field_samples,
    put at the oracle's film position as ImageBlock::put does; also sum |w v| and the number of contributions per pixel and plane"""
    key = (name, filt)
    if key in _film_cache: return _film_cache[key]
    S = mi.scenes; sc = getattr(S, name)(width=37, height=23, spp=5)
    sc.filter = filt; sc.filter_radius = {S.FILTER_BOX: 0.5}.get(filt, 2.0); sc.filter_stddev = 0.5
    gs = mi.Scene(sc); orc = oracle.Oracle(sc)
    yy, xx, kk = np.meshgrid(np.arange(sc.height), np.arange(sc.width), np.arange(sc.spp), indexing="ij")
    pairs = np.stack([xx.ravel(), yy.ravel(), kk.ravel()], 1).astype(np.uint32)
    pos = orc.render_samples(pairs)["pos"]
    r = mi.Render(gs, fields=[(f, UNDEF) for f in FILM_FIELDS]); vals = r.field_samples(pairs).reshape(len(pairs), -1).astype(np.float64)
    ev, rad, b = AM.filter_table(oracle, orc)
    exp, mag, cnt = FM.put64(ev, rad, b, sc.width, sc.height, pos, vals)
    _film_cache[key] = (sc, gs, exp, mag, cnt, b)
    return _film_cache[key]


def check_film(got, exp, mag, cnt, tag):
    """per pixel and plane |got - expected| <= (n + 2) * 2^-24 * sum |w v| over that pixel's n contributions (the weight plane: v = 1)"""
    bound = (cnt[..., None] + 2) * 2.0 ** -24 * mag
    err = np.abs(got.astype(np.float64) - exp); ratio = float((err / np.maximum(bound, 1e-300))[bound > 0].max()) if (bound > 0).any() else 0.0
    print(f"[fields] film {tag}: max err / bound {ratio:.3f}")
    assert (err <= bound).all(), (tag, ratio)


@pytest.mark.parametrize("name", ["cbox_shapes", "instanced_garden"])
@pytest.mark.parametrize("filt", [0, 1])
def test_field_film(mi, oracle, name, filt):
    """37 x 23 film, 5 spp, two planes per batch: three batches over both path pools with a short last one.  The raw field film (layout 0) equals the numpy restatement
    of ImageBlock::put within the rounding bound of its float32 sums; layout 2 = the reference's develop of layout 0 exactly (film_model.develop32: sum x f32(1 / weight), src/libcore/bitmap.cpp:1621-1625)."""
    sc, gs, exp, mag, cnt, b = film_case(mi, oracle, name, filt)
    r = mi.Render(gs, planes_per_batch=2, fields=[(f, UNDEF) for f in FILM_FIELDS]); r.run()
    raw = r.read_fields(0); assert raw.shape == exp.shape and r.field_film_shape(0)[3] == b
    assert (cnt[b:-b, b:-b] >= sc.spp).all()
    check_film(raw, exp, mag, cnt, f"{name} filter {filt}")
    dev = r.read_fields(2); inner = raw[b:raw.shape[0] - b, b:raw.shape[1] - b]
    print(f"[fields] develop {name} filter {filt}: share of values a division would give differently {float((bits(FM.develop32(inner)) != bits(inner[..., :-1] / inner[..., -1:])).mean()):.4f}")
    assert dev.shape == (sc.height, sc.width, 3 * len(FILM_FIELDS)) and (bits(dev) == bits(FM.develop32(inner))).all()


def test_field_film_composition(mi, oracle):
    """The same job as two tiles, as two sample ranges, and as interleaved rows on two handles merged with mi_render_merge_film reproduces the field film; the radiance
    (samples and film) is what it is without fields; call-order errors."""
    sc, gs, exp, mag, cnt, b = film_case(mi, oracle, "cbox_shapes", 0); fields = [(f, UNDEF) for f in FILM_FIELDS]; Wd, Ht = sc.width, sc.height
    r = mi.Render(gs, planes_per_batch=2, fields=fields)
    r.run(tile=(0, 0, 20, Ht)); r.run(tile=(20, 0, Wd, Ht)); check_film(r.read_fields(0), exp, mag, cnt, "two tiles")
    r.clear(); assert not r.read_fields(0).any()
    r.run(s0=0, s1=2); r.run(s0=2, s1=5); check_film(r.read_fields(0), exp, mag, cnt, "two sample ranges")
    ra = mi.Render(gs, planes_per_batch=2, fields=fields); rb = mi.Render(gs, planes_per_batch=2, fields=fields)
    ra.run(tile=(0, 0, Wd, Ht), row_stride=2); rb.run(tile=(0, 1, Wd, Ht), row_stride=2); ra.merge_film(rb)
    check_film(ra.read_fields(0), exp, mag, cnt, "interleaved rows, merged")
    plain = mi.Render(gs, planes_per_batch=2)
    with pytest.raises(mi.MiError) as e:
        ra.merge_film(plain)                                                           # different field lists
    assert e.value.code == 1
    # radiance: untouched by the fields
    pairs = sample_triples(sc, 2000)
    assert (bits(r.samples(pairs)) == bits(plain.samples(pairs))).all()
    r.clear(); r.run(); plain.run(); fa, fb = r.read_film(0), plain.read_film(0)
    assert (bits(fa[b:-b, b:-b]) == bits(fb[b:-b, b:-b])).mean() > 0.995 and np.allclose(fa, fb, rtol=1e-5, atol=1e-6)
    assert r.stats()["rays"] == plain.stats()["rays"]
    # call order
    with pytest.raises(mi.MiError) as e:
        plain.read_fields(0)
    assert e.value.code == 1
    with pytest.raises(mi.MiError) as e:
        plain.set_fields(["distance"])                                                 # the film holds samples
    assert e.value.code == 1
    plain.clear(); plain.set_fields(["distance"]); assert plain.read_fields(0).shape[2] == 4 and not plain.read_fields(0).any()
    plain.set_fields([])
    with pytest.raises(mi.MiError):
        plain.read_fields(0)


# ---------------------------------------------------------------------------------------------- 6: end to end
def test_render_cli_writes_field_channels(mi, tmp_path):
    """python -m mitsuba-im_amd.render on a multichannel scene file (path + shNormal + distance, 32 x 24, box filter, pixelFormat "rgb, rgb, luminance"): the EXR holds
    exactly color.R/G/B, normal.R/G/B, distance.Y, equal to read_film(2) / read_fields(2) of the same job through api.py."""
    xml = os.path.join(GOLDEN, "scenes", "multichannel_fields.xml"); out = str(tmp_path / "fields.exr")
    env = dict(os.environ); env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    subprocess.run([sys.executable, "-m", "mitsuba-im_amd.render", xml, "-o", out], check=True, cwd=ROOT, env=env, timeout=300)
    imageio = __import__("importlib").import_module("mitsuba-im_amd.imageio"); xs = __import__("importlib").import_module("mitsuba-im_amd.xml_scene")
    pix, names = imageio.read_exr(out); planes = [pix[..., i] for i in range(pix.shape[2])]
    assert sorted(names) == sorted(["color.R", "color.G", "color.B", "normal.R", "normal.G", "normal.B", "distance.Y"])
    sc = xs.load_scene(xml); r = mi.Render(mi.Scene(sc)); r.run(); rgb = r.read_film(2); fl = r.read_fields(2)
    assert r.field_names == ["shNormal", "distance"]
    ch = dict(zip(names, planes))
    for i, c in enumerate("RGB"):
        assert (bits(ch["color." + c]) == bits(rgb[..., i])).all() and (bits(ch["normal." + c]) == bits(fl[..., i])).all()
    assert (bits(ch["distance.Y"]) == bits(fl[..., 3])).all()
