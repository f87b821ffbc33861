"""GPU (MI355X): the ambient-occlusion integrator (MI_INTEGRATOR_AO; csrc/ao.h, kernels_ao.hip) through the C-ABI.

No vectors compiled from the reference pin this integrator (the reference build used as a checker holds no `ao` plugin): the yardstick is the Python model of ao.cpp
(tests/ao_model.py), composed of oracle units and pinned on the CPU by tests/test_ao_model.py.

1. samples(pairs) against the model for N = 1 (the own request), 4 (the array) and 3 (a reciprocal that is no power of two) on eight scenes, with the ray counters.
2. Ray length: shorter than Epsilon, automatic, monotone.   3. The independent sampler.   4. Pool shapes, batch sizes and pool counts do not move a bit.
5. Fields.   6. In-place edits.   7. The host mirror.   8. Refusals.   9. The scenes `direct` refuses."""
import os

import numpy as np
import pytest
from tests.ao_model import AoModel, auto_ray_length
from tests.test_gpu_direct import CRITERIA      # the GPU-vs-oracle criterion each scene has between GPU and oracle, quoted there from tests/test_gpu_parity.py
from tests.test_gpu_fused_walk import ATRIUM_40K      # the scene and size at which the fused walk is engaged

pytestmark = pytest.mark.gpu
W = H = 24; SPP = 4
f32 = np.float32
DOF_ROW = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenes", "dof_row.xml")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def all_pairs(sc):
    return np.array([(x, y, s) for y in range(sc.height) for x in range(sc.width) for s in range(sc.spp)], np.uint32)


SCENES = {
    "cornell_box": lambda S: S.cornell_box(W, H, SPP, max_depth=2),                                    # packet mode
    "cbox_shapes": lambda S: S.cbox_shapes(W, H, SPP, max_depth=2),                                    # analytic shapes
    "instanced_garden": lambda S: S.instanced_garden(W, H, SPP, max_depth=2),                          # instances
    "wavy_sheet": lambda S: S.wavy_sheet(4, amp=0.5, width=W, height=H, spp=SPP, max_depth=2),         # smooth normals far from the geometric ones: shading frame != geometric frame
    "atrium_40k": lambda S: S.atrium(**ATRIUM_40K),                                                    # the fused walk
    "sky_view": lambda S: S.sky_view(W, H, SPP, max_depth=2),                                          # misses are 1 under an environment map
    "layered_room": lambda S: S.layered_room(W, H, SPP, max_depth=2),                                  # mixturebsdf / bumpmap / normalmap: refused by `direct`
    "fog_box": lambda S: S.fog_box(W, H, SPP, max_depth=2),                                            # media, `null` boundaries: refused by `direct`
}


def criterion_of(sc):
    """bit for bit; where analytic shapes or instances enter, the criterion the scene has between GPU and oracle (CRITERIA["libm"] of tests/test_gpu_direct.py, i.e.
    test_analytic_shapes / test_instances of tests/test_gpu_parity.py:  (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-6 and bit_share > 0.9999)"""
    return "libm" if (sc.get("analytic") or sc.get("instances")) else "bits"


def length_of(sc):
    """the automatic length (-1) where the model restates the scene's bounding sphere (mesh scenes); with analytic shapes or instances an explicit one of the same order:
    a quarter of the diagonal of the vertex box"""
    if not (sc.get("analytic") or sc.get("instances")): return -1.0
    pos = np.asarray(sc.pos, f32).reshape(-1, 3); return float(f32(0.25) * f32(np.linalg.norm(pos.max(0) - pos.min(0))))


def ao(mi, gs, n=1, length=-1.0, **kw):
    return mi.Render(gs, integrator=mi.scenes.INTEGRATOR_AO, shading_samples=n, ray_length=length, **kw)


@pytest.fixture(scope="module")
def model_cache(mi, oracle):
    cache = {}
    def get(name, n):
        if (name, n) not in cache:
            sc = SCENES[name](mi.scenes); cache[(name, n)] = (sc, AoModel(oracle, sc, n, length_of(sc)).render_samples(all_pairs(sc)))
        return cache[(name, n)]
    return get


# ---------------------------------------------------------------------------------------------- 1: against the model
@pytest.mark.parametrize("n", [1, 4, 3])
@pytest.mark.parametrize("name", list(SCENES))
def test_ao_vs_model(mi, model_cache, name, n):
    sc, model = model_cache(name, n); pairs = all_pairs(sc); gs = mi.Scene(sc)
    r = ao(mi, gs, n, length_of(sc)); got = r.samples(pairs); ref = model["li"]
    share = float((bits(got) == bits(ref)).all(1).mean())
    print(f"[ao] {name} N={n}: {model['hit'].mean():.3f} of the camera rays hit, mean {ref.mean():.4f}, bit share {share:.5f}, max abs difference {np.abs(got - ref).max():.3e}")
    assert model["hit"].mean() > 0.2 and 0.05 < ref[model["hit"]].mean() < 0.999      # the scene is in the picture, and so is the occlusion
    assert CRITERIA[criterion_of(sc)](got, ref)
    r.clear(); r.run(); st = r.stats()
    assert (st["rays"], st["shadow_rays"], st["path_length_sum"], st["samples"]) == (len(pairs), model["shadow_rays"], 0, len(pairs))
    assert model["shadow_rays"] == n * int(model["hit"].sum()) and r.pool_info()["integrator"] == mi.scenes.INTEGRATOR_AO


def test_product_with_the_reciprocal_where_it_is_not_the_quotient(mi, model_cache, oracle):
    """N = 7: the smallest count at which k * (1.0f / N) and k / N differ in float32 (k = 3, 6; at N = 3 they agree for every k, tests/test_ao_model.py)"""
    sc, _ = model_cache("cornell_box", 1); pairs = all_pairs(sc); model = AoModel(oracle, sc, 7).render_samples(pairs)
    got = ao(mi, mi.Scene(sc), 7).samples(pairs); odd = {int(f32(f32(k) * (f32(1) / f32(7))).view(np.uint32)) for k in (3, 6)}
    assert (bits(got) == bits(model["li"])).all() and odd & set(bits(got[:, 0]).tolist())


def test_misses_are_one_under_an_environment_map(mi, model_cache):
    sc, model = model_cache("sky_view", 3); got = ao(mi, mi.Scene(sc), 3).samples(all_pairs(sc))
    assert (~model["hit"]).sum() > 100 and (bits(got[~model["hit"]]) == bits(f32(1))).all()
    # alpha: 1 on a hit, 0 on a miss (records.inl:117-144) -- the rule of `path`, whose film holds the same camera rays: alpha and weight planes bit for bit
    gs = mi.Scene(sc); r = ao(mi, gs, 3, opacity=True); r.run(); film = r.read_film(0); p = mi.Render(gs, opacity=True); p.run(); ref = p.read_film(0)
    assert (bits(film[..., 3:]) == bits(ref[..., 3:])).all() and (film[..., 3] < film[..., 4]).any() and (film[..., 3] > 0).any()
    plain = ao(mi, gs, 3); plain.run(); assert (bits(plain.read_film(0)[..., 3]) == bits(ref[..., 4])).all()      # without EOpacity: alpha = 1 everywhere


# ---------------------------------------------------------------------------------------------- 2: ray length
def test_ray_length(mi, model_cache):
    sc, _ = model_cache("cornell_box", 4); gs = mi.Scene(sc); pairs = all_pairs(sc)
    assert (bits(ao(mi, gs, 4, 5e-5).samples(pairs)) == bits(f32(1))).all()         # shorter than Epsilon: nothing is seen, hits and misses alike
    auto = float(auto_ray_length(sc)); assert auto > 0
    a = ao(mi, gs, 4, -1.0); a.run(); b = ao(mi, gs, 4, auto); b.run()
    assert (bits(a.read_film(0)) == bits(b.read_film(0))).all() and 0 < a.read_film(2).mean() < 1
    c = ao(mi, gs, 4, auto * 1.25); c.run(); assert not (bits(c.read_film(0)) == bits(a.read_film(0))).all()      # the length is in the picture
    short, long_ = ao(mi, gs, 4, 60.0).samples(pairs), ao(mi, gs, 4, 400.0).samples(pairs)
    assert (long_ <= short).all() and (long_ < short).any(1).sum() > 100


# ---------------------------------------------------------------------------------------------- 3: the independent sampler
def test_independent_sampler(mi, model_cache):
    """The build-defined stream: the four array elements of ao(4) are four different calls.  Were they one and the same draw, every value would be 0 or 1.  Under the
    model (Sobol') 0.71 of the camera hits of this scene have a value strictly between 0 and 1 (0.93 of the camera rays hit); the bound asserted is half of that share,
    from the model alone.  Observed on the device under the independent sampler: 0.688 of all samples.  And ao(4) has the
    expectation of ao(1): the image means agree within 4 standard errors, each estimated from its own samples (shared camera rays only bring them closer)."""
    sc_s, model = model_cache("cornell_box", 4); li = model["li"][model["hit"], 0]; model_share = float(((li > 0) & (li < 1)).mean())
    sc = mi.scenes.cornell_box(W, H, SPP, sampler=0, max_depth=2); gs = mi.Scene(sc); pairs = all_pairs(sc)
    a = ao(mi, gs, 4).samples(pairs)[:, 0].astype(np.float64); b = ao(mi, gs, 1).samples(pairs)[:, 0].astype(np.float64)
    share = float(((a > 0) & (a < 1)).mean()); se = lambda x: x.std() / np.sqrt(len(x))
    print(f"[ao-indep] share strictly between 0 and 1: {share:.3f} (Sobol' model, camera hits: {model_share:.3f}); mean ao(4) {a.mean():.5f} +- {se(a):.5f}, ao(1) {b.mean():.5f} +- {se(b):.5f}")
    assert model_share > 0.1 and share > 0.5 * model_share * model["hit"].mean()
    assert set(np.unique(b).tolist()) <= {0.0, 1.0} and set(np.unique(a).tolist()) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    assert 0 < a.mean() < 1 and abs(a.mean() - b.mean()) < 4 * np.hypot(se(a), se(b))


# ---------------------------------------------------------------------------------------------- 4: pool geometry
def test_pool_shapes_do_not_move_a_bit(mi, monkeypatch):
    """6000 samples of N = 3: the default shape (94 x 64 slots: one-wave segments), 6 x 1024 (several chunks per segment) and 47 x 128 (a part-filled last chunk)"""
    sc = mi.scenes.cornell_box(64, 48, 4, max_depth=2); gs = mi.Scene(sc); rng = np.random.default_rng(3)
    pairs = np.stack([rng.integers(0, sc.width, 6000), rng.integers(0, sc.height, 6000), rng.integers(0, sc.spp, 6000)], 1).astype(np.uint32)
    out = {}
    for seg, shape in ((None, (94, 64)), (6, (6, 1024)), (47, (47, 128))):
        if seg is None: monkeypatch.delenv("MI355PT_SEGMENTS", raising=False)
        else: monkeypatch.setenv("MI355PT_SEGMENTS", str(seg))
        r = ao(mi, gs, 3); out[seg] = r.samples(pairs); info = r.pool_info()
        assert (info["n_seg"], info["cap"]) == shape and info["integrator"] == mi.scenes.INTEGRATOR_AO
    assert (bits(out[None]) == bits(out[6])).all() and (bits(out[None]) == bits(out[47])).all() and 0 < out[None].mean() < 1


def test_batch_sizes_and_pool_counts_give_identical_films(mi, monkeypatch):
    sc = mi.scenes.cornell_box(32, 24, 6, max_depth=2); gs = mi.Scene(sc); films = []
    for streams, planes in ((1, 1), (1, 3), (2, 1), (2, 3)):
        monkeypatch.setenv("MI355PT_STREAMS", str(streams))
        r = ao(mi, gs, 3, planes_per_batch=planes); r.run(); films.append(r.read_film(0)); assert r.pool_info()["n_pools"] == streams
    assert all((bits(f) == bits(films[0])).all() for f in films[1:]) and 0 < films[0][..., :3].max()


# ---------------------------------------------------------------------------------------------- 5: fields
def test_field_channels_next_to_ao_equal_those_next_to_path(mi):
    sc = mi.scenes.cornell_box(32, 24, 4, max_depth=2); gs = mi.Scene(sc); names = ["position", "distance", "shNormal", "albedo", "primIndex"]
    a = mi.Render(gs, fields=names); a.run(); b = ao(mi, gs, 4, fields=names); b.run()
    assert (bits(a.read_fields(0)) == bits(b.read_fields(0))).all() and np.abs(b.read_fields(0)).max() > 0 and 0 < b.read_film(2).mean() < 1


def test_field_channels_on_the_lens_scene(mi):
    """the thinlens fixture scene: the lens only shifts the own request by two dimensions; the field stage sees the same camera hits"""
    xs = __import__("importlib").import_module("mitsuba-im_amd.xml_scene")
    sc = xs.load_scene(DOF_ROW); sc.spp = 2; assert sc.aperture_radius > 0
    gs = mi.Scene(sc); names = ["position", "distance", "primIndex"]
    a = mi.Render(gs, fields=names); a.run(); b = ao(mi, gs, 1, fields=names); b.run(); c = ao(mi, gs, 4, fields=names); c.run()
    assert (bits(a.read_fields(0)) == bits(b.read_fields(0))).all() and (bits(a.read_fields(0)) == bits(c.read_fields(0))).all()
    assert np.abs(b.read_fields(0)).max() > 0 and 0 < b.read_film(2).mean() < 1 and 0 < c.read_film(2).mean() < 1


# ---------------------------------------------------------------------------------------------- 6: in-place edits
def test_camera_edit_in_place_equals_a_fresh_commit(mi):
    S = mi.scenes; A = S.cornell_box(32, 24, 4, max_depth=2); B = S.cornell_box(32, 24, 4, max_depth=2)
    B.cam_to_world = S.look_at((200.0, 300.0, -2500.0), (278.0, 273.0, 280.0), (0.0, 1.0, 0.0)).astype(np.float32)      # far out: the bounding sphere, and with it the automatic length, grows
    assert auto_ray_length(B) > 1.5 * auto_ray_length(A)
    gs = mi.Scene(A); r = ao(mi, gs, 3); r.run(); before = r.read_film(0)
    gs.update_camera(B.sample_to_camera, B.cam_to_world, B.near, B.far)
    with pytest.raises(mi.MiError, match="mi_render_clear"):
        r.run()
    r.clear(); r.run(); edited = r.read_film(0)
    f = ao(mi, mi.Scene(B), 3); f.run(); fresh = f.read_film(0)
    assert (bits(edited) == bits(fresh)).all() and not (bits(edited) == bits(before)).all() and r.stats()["shadow_rays"] == f.stats()["shadow_rays"]
    e = ao(mi, mi.Scene(B), 3, float(auto_ray_length(B))); e.run(); assert (bits(e.read_film(0)) == bits(fresh)).all()      # ... and it is the length of the edited scene


def test_vertex_edit_in_place_moves_the_automatic_length(mi):
    """the scene doubled about the camera: every distance doubles, and so does the automatic length -- the picture stays the picture of the doubled scene, which a length
    left at the committed value would not give"""
    S = mi.scenes; A = S.cornell_box(32, 24, 4, max_depth=2); cam = np.asarray(A.cam_to_world, f32).reshape(4, 4)[:3, 3]
    pos2 = (cam + (np.asarray(A.pos, f32).reshape(-1, 3) - cam) * f32(2)).astype(f32)
    B = type(A)(A); B.pos = pos2; committed = float(auto_ray_length(A))      # (taken now: the edit below moves the description's vertices too)
    assert auto_ray_length(B) > 1.9 * committed
    gs = mi.Scene(A); r = ao(mi, gs, 3); r.run(); before = r.read_film(0)
    gs.update_vertices(pos2); r.clear(); r.run(); edited = r.read_film(0)
    f = ao(mi, mi.Scene(B), 3); f.run(); fresh = f.read_film(0)
    assert (bits(edited) == bits(fresh)).all()
    stale = ao(mi, mi.Scene(B), 3, committed); stale.run()
    assert not (bits(stale.read_film(0)) == bits(fresh)).all() and 0 < before[..., :3].max()


# ---------------------------------------------------------------------------------------------- 7: the host mirror
def test_host_integrator_ao_equals_render(mi):
    sc = mi.scenes.cornell_box(32, 24, 4, max_depth=2); gs = mi.Scene(sc)
    for n, length in ((3, -1.0), (1, 150.0)):
        h = mi.api.HostIntegrator(gs, integrator=mi.scenes.INTEGRATOR_AO, shading_samples=n, ray_length=length)
        target = np.zeros((sc.height + 2, sc.width + 2, 4), np.float32); assert h.render("responsive", target) == 0
        r = ao(mi, gs, n, length, opacity=True); r.run()
        assert (bits(target) == bits(r.read_film(1))).all() and 0 < target[..., :3].max()
    with pytest.raises(RuntimeError, match="shadingSamples must be at least 1"):
        mi.api.HostIntegrator(gs, integrator=mi.scenes.INTEGRATOR_AO, shading_samples=0)
    sc.integrator = mi.scenes.INTEGRATOR_AO; sc.shading_samples = 3      # the scene description's keys are the defaults
    h = mi.api.HostIntegrator(mi.Scene(sc)); t2 = np.zeros_like(target); assert h.render("responsive", t2) == 0
    r = mi.Render(gs, integrator=mi.scenes.INTEGRATOR_AO, shading_samples=3, opacity=True); r.run(); assert (bits(t2) == bits(r.read_film(1))).all()


# ---------------------------------------------------------------------------------------------- 8: refusals
def test_refusals_by_name(mi):
    S = mi.scenes; gs = mi.Scene(S.cornell_box(W, H, SPP, max_depth=2))
    with pytest.raises(mi.MiError, match="shadingSamples must be at least 1"):
        ao(mi, gs, 0)
    with pytest.raises(mi.MiError, match="spp x shadingSamples beyond 2\\^22"):
        ao(mi, gs, (1 << 20) + 1)
    ao(mi, gs, 1 << 12).close()
    with pytest.raises(mi.MiError, match="film of at least 2 x 2 pixels"):
        ao(mi, mi.Scene(S.cornell_box(1, 1, SPP, max_depth=2)), 2)
    ao(mi, mi.Scene(S.cornell_box(1, 1, SPP, max_depth=2)), 1).close()             # the own request needs no array
    gi = mi.Scene(S.cornell_box(W, H, SPP, sampler=0, max_depth=2))
    with pytest.raises(mi.MiError, match="independent sampler stream numbers 256 draws"):
        ao(mi, gi, 256)
    assert ao(mi, gi, 255).samples(all_pairs(gi.sc)[:64]).shape == (64, 3)           # calls 1 .. 255 after the camera's call 0
    with pytest.raises(mi.MiError, match="`opacity` on a scene with participating media"):
        ao(mi, mi.Scene(S.fog_box(W, H, SPP)), 2, opacity=True)
    with pytest.raises(RuntimeError, match="integrators path"):
        mi.Render(gs, integrator=5)


def test_refusal_of_a_short_sobol_table(mi):
    """six Sobol' dimensions loaded: the own request (dimensions 2 / 3) fits, the array (dimensions 5 / 6) does not"""
    import struct
    L = mi.lib()
    with open(mi.api.SOBOL_PATH, "rb") as f:
        assert f.read(8) == b"MISOBOL1"; dims, rows = struct.unpack("<2I", f.read(8))
        m32 = np.frombuffer(f.read(dims * 52 * 4), dtype="<u4").copy(); vdc = np.frombuffer(f.read(rows * 52 * 8), dtype="<u8").copy(); vdci = np.frombuffer(f.read(rows * 52 * 8), dtype="<u8").copy()
    try:
        short = np.ascontiguousarray(m32[:6 * 52]); L.check(L.L.mi_set_sobol_tables(short.ctypes.data, 6, vdc.ctypes.data, vdci.ctypes.data))
        gs = mi.Scene(mi.scenes.cornell_box(W, H, SPP, max_depth=2))
        with pytest.raises(mi.MiError, match="Lookup dimension exceeds the direction number table size.*ao integrator"):
            ao(mi, gs, 2)
        ao(mi, gs, 1).close()
    finally:
        mi.api.load_sobol_tables(L)


# ---------------------------------------------------------------------------------------------- 9: the scenes `direct` refuses
@pytest.mark.parametrize("name", ["layered_room", "fog_box"])
def test_scenes_direct_refuses_render(mi, name):
    sc = SCENES[name](mi.scenes); gs = mi.Scene(sc)
    with pytest.raises(mi.MiError, match="direct integrator does not"):
        mi.Render(gs, integrator=mi.scenes.INTEGRATOR_DIRECT)
    r = ao(mi, gs, 4); r.run(); rgb = r.read_film(2); st = r.stats()
    assert np.isfinite(rgb).all() and 0 < rgb.mean() < 1 and rgb.max() <= 1 and st["samples"] == sc.width * sc.height * sc.spp and 0 < st["shadow_rays"] <= 4 * st["samples"]


# ---------------------------------------------------------------------------------------------- 10: the command line
def test_command_line(mi, tmp_path):
    """an `ao` scene file renders as any other; `--ao N [--ao-length L]` puts the integrator in place of a scene file's own"""
    il = __import__("importlib"); xs = il.import_module("mitsuba-im_amd.xml_scene"); render = il.import_module("mitsuba-im_amd.render")
    sc = mi.scenes.cornell_box(32, 24, 2, max_depth=2); sc.integrator = mi.scenes.INTEGRATOR_AO; sc.shading_samples = 3; sc.ray_length = 200.0
    path = xs.export_scene(sc, str(tmp_path)); out = str(tmp_path / "a.npy")
    assert render.main([path, "-o", out]) == 0
    loaded = xs.load_scene(path); r = mi.Render(mi.Scene(loaded)); r.run(); want = r.read_film(2)
    got = np.load(out); assert (bits(got) == bits(want)).all() and 0 < got.mean() < 1 and r.pool_info()["integrator"] == mi.scenes.INTEGRATOR_AO
    out2 = str(tmp_path / "b.npy"); assert render.main([DOF_ROW, "--ao", "4", "--ao-length", "1.5", "--spp", "2", "-o", out2]) == 0      # a `path` scene file with a thinlens sensor
    lens = xs.load_scene(DOF_ROW); lens.spp = 2; r2 = ao(mi, mi.Scene(lens), 4, 1.5); r2.run()
    assert (bits(np.load(out2)) == bits(r2.read_film(2))).all() and 0 < np.load(out2).mean() < 1
