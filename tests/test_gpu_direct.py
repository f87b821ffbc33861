"""GPU (MI355X): the direct-illumination integrator (MI_INTEGRATOR_DIRECT; csrc/direct.h, kernels_direct_*.hip) through the C-ABI.

1. direct(1,1) IS `path` at maxDepth = 2 (see tests/test_direct_model.py for the one difference: specular camera hits) -> against the oracle's `path`, per scene by the
   criterion the scene's own test in tests/test_gpu_parity.py applies between GPU and oracle (quoted below), both samplers, incl. `mask` (masked_room), strictNormals (a coarse wavy_sheet) and the specular camera hits of cbox_materials at the size
   at which they change the radiance; films against the device's own `path`.
2. direct(N, M) against the Python model of direct.cpp (tests/direct_model.py, pinned to the oracle on the CPU): sample arrays, skip rules, fractions, counters.
3. Pool shapes, batch sizes and pool counts do not move a bit.   4. Fields, in-place edits, the host mirror, refusals."""
import numpy as np
import pytest
from tests.direct_model import DirectModel

pytestmark = pytest.mark.gpu
W = H = 24; SPP = 4
NM_CASES = [(4, 0), (0, 4), (3, 2), (4, 4), (1, 4), (4, 1)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def all_pairs(sc):
    return np.array([(x, y, s) for y in range(sc.height) for x in range(sc.width) for s in range(sc.spp)], np.uint32)


def rel_err(got, ref):
    return np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)


def bit_share(got, ref):
    return float((bits(got) == bits(ref)).all(1).mean())


# GPU-vs-oracle criterion of each scene, as tests/test_gpu_parity.py states it:
CRITERIA = {
    # test_li_samples_bit_exact_vs_oracle / test_texture_coordinates_and_procedural_textures:  assert (bits(got) == bits(ref)).all()
    "bits": lambda got, ref: (bits(got) == bits(ref)).all(),
    # test_roughconductor_veach_mis:  assert (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-6 ... assert bit_share(got, ref, "veach_small") > 0.9999
    # test_instances:  assert bit_share(got, ref, "instances") > 0.9999 and (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-6
    # test_analytic_shapes:  assert (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-6 and bit_share(got, ref, "analytic_shapes " + name) > 0.9999
    "libm": lambda got, ref: (rel_err(got, ref) < 1e-4).mean() > 0.995 and np.median(rel_err(got, ref)) < 1e-6 and bit_share(got, ref) > 0.9999,
    # test_roughplastic:  assert (err < 1e-4).mean() > 0.99 and np.median(err) < 1e-6
    "roughplastic": lambda got, ref: (rel_err(got, ref) < 1e-4).mean() > 0.99 and np.median(rel_err(got, ref)) < 1e-6,
    # test_bitmap_textures:  assert (err < 1e-4).mean() > 0.998 and np.median(err) < 1e-6 and bit_share(got, ref, "bitmap_textures") >= 0.9999
    "bitmap": lambda got, ref: (rel_err(got, ref) < 1e-4).mean() > 0.998 and np.median(rel_err(got, ref)) < 1e-6 and bit_share(got, ref) >= 0.9999,
    # test_scene_level_emitters, open_constant (rough-conductor sphere):  assert (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-6
    "constant": lambda got, ref: (rel_err(got, ref) < 1e-4).mean() > 0.995 and np.median(rel_err(got, ref)) < 1e-6,
    # test_scene_level_emitters, cbox_lights:  assert bit_share(got, ref, name) > 0.9999 and (err < 1e-5).mean() > 0.999
    "lights": lambda got, ref: bit_share(got, ref) > 0.9999 and (rel_err(got, ref) < 1e-5).mean() > 0.999,
    # test_filtered_environment_lookups:  assert (err < 1e-5).mean() > 0.95 and (err < 1e-3).mean() > 0.995 and err.max() < 5e-3
    "sky": lambda got, ref: (rel_err(got, ref) < 1e-5).mean() > 0.95 and (rel_err(got, ref) < 1e-3).mean() > 0.995 and rel_err(got, ref).max() < 5e-3,
    # test_rough_dielectric_and_difftrans:  assert (err < 1e-4).mean() > 0.99 and np.median(err) < 1e-6 and (bits(got) == bits(ref)).all(1).mean() > 0.5
    "translucent": lambda got, ref: (rel_err(got, ref) < 1e-4).mean() > 0.99 and np.median(rel_err(got, ref)) < 1e-6 and bit_share(got, ref) > 0.5,
}
SCENES_11 = [("cornell_box", {}, "bits"), ("veach_mis", {}, "libm"), ("cbox_roughplastic", {}, "roughplastic"), ("textured_room", {}, "bits"), ("bitmap_room", {}, "bitmap"),
             ("cbox_shapes", {}, "libm"), ("instanced_garden", {}, "libm"), ("open_constant", {}, "constant"), ("open_constant", dict(hide_emitters=True), "constant"),
             ("sky_view", {}, "sky"), ("sky_view", dict(hide_emitters=True), "sky"), ("cbox_lights", {}, "lights")]


def make(mi, name, sampler=1, **kw):
    return getattr(mi.scenes, name)(W, H, SPP, sampler=sampler, max_depth=2, **kw)


def direct(mi, gs, n=1, m=1, **kw):
    return mi.Render(gs, integrator=mi.scenes.INTEGRATOR_DIRECT, emitter_samples=n, bsdf_samples=m, **kw)


# ---------------------------------------------------------------------------------------------- 1: direct(1,1) = path at maxDepth 2
@pytest.mark.parametrize("sampler", [1, 0], ids=["sobol", "independent"])
@pytest.mark.parametrize("name,kw,criterion", SCENES_11, ids=[n + ("_hide" if k else "") for n, k, _ in SCENES_11])
def test_direct_11_vs_oracle_path(mi, oracle, name, kw, criterion, sampler):
    sc = make(mi, name, sampler, **kw); pairs = all_pairs(sc)
    ref = oracle.Oracle(sc).render_samples(pairs)["li"]
    got = direct(mi, mi.Scene(sc)).samples(pairs)
    assert (np.abs(ref).max(1) > 0).mean() > 0.2
    print(f"[direct11] {name} {kw} sampler {sampler}: bit share {bit_share(got, ref):.5f}, err < 1e-4 {(rel_err(got, ref) < 1e-4).mean():.5f}, max {rel_err(got, ref).max():.3e}")
    assert CRITERIA[criterion](got, ref)


@pytest.mark.parametrize("sampler", [1, 0], ids=["sobol", "independent"])
def test_direct_11_with_lens_equals_device_path(mi, sampler):
    """thin lens: the aperture sample holds Sobol' dimensions 2 / 3, the running dimension starts at 4, the first next2D jumps to the end of the array range.  The oracle
    has no lens, so the yardstick is the device's own `path` at maxDepth = 2 -- the same arithmetic: bit for bit."""
    sc = mi.scenes.with_lens(make(mi, "cornell_box", sampler), 12.0, 600.0); pairs = all_pairs(sc); gs = mi.Scene(sc)
    ref = mi.Render(gs).samples(pairs); got = direct(mi, gs).samples(pairs)
    assert (bits(got) == bits(ref)).all() and (np.abs(ref).max(1) > 0).mean() > 0.2
    plain = direct(mi, mi.Scene(make(mi, "cornell_box", sampler))).samples(pairs)
    assert not (bits(got) == bits(plain)).all()                  # the lens is in the picture


@pytest.mark.parametrize("sampler,hide", [(1, False), (0, True)], ids=["sobol", "independent_hide"])
def test_direct_11_mask_vs_oracle_path(mi, oracle, sampler, hide):
    """masked_room: `mask` in front of twosided diffuse (checkerboard opacity 1 / 0), plastic (coloured constant opacity) and a rough conductor (grid), under a constant
    sky and a directional sun: eval / pdf scaled by the opacity, the ENull pass-through with the rescaled sample, and with hideEmitters the sky that stays hidden
    behind a pass-through (the BSDF ray that leaves the scene after a null event adds nothing).
    test_mask:  assert bit_share(got, ref, "mask " + name) > 0.9999 and (err < 1e-4).mean() > 0.995 and np.median(err) == 0"""
    sc = make(mi, "masked_room", sampler, hide_emitters=hide); pairs = all_pairs(sc)
    ref = oracle.Oracle(sc).render_samples(pairs)["li"]; got = direct(mi, mi.Scene(sc)).samples(pairs); err = rel_err(got, ref)
    print(f"[direct11] masked_room sampler {sampler} hide {hide}: bit share {bit_share(got, ref):.5f}, err < 1e-4 {(err < 1e-4).mean():.5f}, max {err.max():.3e}")
    assert (np.abs(ref).max(1) > 0).mean() > 0.2
    assert bit_share(got, ref) > 0.9999 and (err < 1e-4).mean() > 0.995 and np.median(err) == 0
    if hide:                                                      # the switch is in the picture: the sky behind the holes of the screen is gone
        shown = oracle.Oracle(make(mi, "masked_room", sampler)).render_samples(pairs)["li"]
        assert not (bits(shown) == bits(ref)).all()


def test_direct_11_strict_normals_vs_oracle_path(mi, oracle):
    """wavy_sheet with 4 x 4 quads and a large amplitude: smooth vertex normals far from the geometric ones, so strictNormals ends camera hits early and rejects
    emitter and BSDF sub-samples whose direction lies on different sides of the two normals (direct.cpp:175-187, :229-232, :262-265).  Diffuse BSDFs, a checkerboard,
    an area light: free of libm like textured_room -> test_texture_coordinates_and_procedural_textures:  assert (bits(got) == bits(ref)).all()"""
    mk = lambda: mi.scenes.wavy_sheet(4, amp=0.5, width=32, height=24, spp=SPP, max_depth=2)
    sc = mk(); sc.strict_normals = 1; pairs = all_pairs(sc)
    ref = oracle.Oracle(sc).render_samples(pairs)["li"]; got = direct(mi, mi.Scene(sc)).samples(pairs)
    print(f"[direct11] wavy_sheet strict: bit share {bit_share(got, ref):.5f}, max err {rel_err(got, ref).max():.3e}")
    assert (bits(got) == bits(ref)).all() and (np.abs(ref).max(1) > 0).mean() > 0.2
    lax = oracle.Oracle(mk()).render_samples(pairs)["li"]
    assert (~(bits(lax) == bits(ref)).all(1)).sum() >= 5          # the switch is in the picture


def test_direct_11_specular_camera_hits_consume_the_emitter_sample(mi, oracle):
    """cbox_materials at the size at which it shows in the radiance (tests/test_direct_model.py, SPECULAR_SIZE): on a camera hit without smooth component `direct` has
    consumed the emitter side's sample, so the glass sphere chooses between reflection and refraction by another value than under `path`.  The device equals the
    model bit for bit (test_smooth_bsdfs: assert (bits(got) == bits(ref)).all()), and with it differs from `path` on some specular camera hit and nowhere else."""
    from tests.test_direct_model import specular_case
    sc, pairs = specular_case(mi)
    model = DirectModel(oracle, sc, 1, 1).render_samples(pairs); path = oracle.Oracle(sc).render_samples(pairs)["li"]
    got = direct(mi, mi.Scene(sc)).samples(pairs)
    assert (bits(got) == bits(model["li"])).all()
    differs = ~(bits(got) == bits(path)).all(1)
    assert (differs & model["specular"]).any() and not (differs & ~model["specular"]).any()


def test_direct_11_film_equals_device_path_film(mi):
    """films through mi_render_run: radiance, alpha and weights of direct(1,1) equal the device's own path film at maxDepth = 2, bit for bit; so do the ray counters"""
    sc = make(mi, "cornell_box"); gs = mi.Scene(sc)
    a = mi.Render(gs, opacity=True); a.run(); b = direct(mi, gs, opacity=True); b.run()
    fa, fb = a.read_film(0), b.read_film(0)
    assert (bits(fa) == bits(fb)).all() and fa[..., :3].max() > 0 and fa[..., 3].max() > 0 and fa[..., 4].max() > 0
    sa, sb = a.stats(), b.stats()
    assert (sa["rays"], sa["shadow_rays"], sa["samples"]) == (sb["rays"], sb["shadow_rays"], sb["samples"]) and sb["path_length_sum"] == 0 and sa["path_length_sum"] > 0


# ---------------------------------------------------------------------------------------------- 2: direct(N, M) against the model
@pytest.fixture(scope="module")
def model_cache(mi, oracle):
    cache = {}
    def get(name, n, m):
        if (name, n, m) not in cache:
            sc = make(mi, name); cache[(name, n, m)] = (sc, DirectModel(oracle, sc, n, m).render_samples(all_pairs(sc)))
        return cache[(name, n, m)]
    return get


@pytest.mark.parametrize("nm", NM_CASES, ids=[f"{n}_{m}" for n, m in NM_CASES])
@pytest.mark.parametrize("name,criterion", [("cornell_box", "bits"), ("veach_mis", "libm")])
def test_direct_nm_vs_model(mi, model_cache, name, criterion, nm):
    """(4,0) / (0,4): MIS weight exactly 1, the array indexing alone; (3,2): fractions other than 1/2, a weight 1/3 that is no power of two; (1,4) / (4,1): the skip rule
    of next2D around the one array; (4,4): two arrays.  Counters: rays = camera rays + BSDF rays cast, shadow rays = emitter samples with pdf != 0, no path lengths."""
    sc, model = model_cache(name, *nm); pairs = all_pairs(sc); gs = mi.Scene(sc)
    r = direct(mi, gs, *nm); got = r.samples(pairs)
    print(f"[directNM] {name} {nm}: bit share {bit_share(got, model['li']):.5f}, max err {rel_err(got, model['li']).max():.3e}")
    assert CRITERIA[criterion](got, model["li"])
    r.clear(); r.run(); st = r.stats()
    assert (st["rays"], st["shadow_rays"], st["path_length_sum"], st["samples"]) == (model["rays"], model["shadow_rays"], 0, len(pairs))


@pytest.mark.parametrize("nm", [(1, 1), (4, 4)], ids=["1_1", "4_4"])
@pytest.mark.parametrize("name,criterion", [("cbox_translucent", "translucent"), ("cbox_materials", "bits")])
def test_direct_sampler_drawing_and_specular_bsdfs_vs_model(mi, model_cache, name, criterion, nm):
    """cbox_translucent: `roughdielectric` draws its extra 1-D value from the sample's RUNNING dimension, one after another over the BSDF sub-samples (stored back into
    the camera-hit queue between the passes).  cbox_materials: smooth conductor / dielectric camera hits still consume the emitter side's sample (test_smooth_bsdfs:
    assert (bits(got) == bits(ref)).all())."""
    sc, model = model_cache(name, *nm); got = direct(mi, mi.Scene(sc), *nm).samples(all_pairs(sc))
    print(f"[directNM] {name} {nm}: bit share {bit_share(got, model['li']):.5f}, max err {rel_err(got, model['li']).max():.3e}")
    assert CRITERIA[criterion](got, model["li"])
    if name == "cbox_materials" and nm == (1, 1): assert model["specular"].sum() > 20


def test_distinct_sub_samples_draw_distinct_values_independent(mi):
    """the build-defined stream: the sub-samples of a side take different calls of the stream.  hideEmitters, so that the estimate is the direct
    lighting alone.
    (a) (4,4) has the expectation of (1,1): the image means agree within 4 standard errors (each estimated from its own samples; the two share the camera rays,
        which only brings them closer).
    (b) Same camera rays, emitter side only: L1, L4, L64 = the (1,0), (4,0), (64,0) estimates of one camera sample, s2 = the variance of one emitter draw given the
        camera ray.  The array elements count down from call 255, so L64 holds the four draws of L4 and 60 more: L4 - L64 = 60/64 (L4 - mean of the other 60) has
        variance (60/64)^2 (1/4 + 1/60) s2 = 0.234 s2, and L1 (call 1, no part of L64) gives var(L1 - L64) = (1 + 1/64) s2.  Ratio 4.3.  Were the sub-samples of a
        side one and the same draw, L4 = L64 and the ratio has no bound; were they the draw of (1,0), it is 1.  Asserted: between 2 and 9."""
    sc = make(mi, "cornell_box", sampler=0, hide_emitters=True); gs = mi.Scene(sc); pairs = all_pairs(sc)
    lum = lambda n, m: direct(mi, gs, n, m).samples(pairs).mean(1).astype(np.float64)
    a, b = lum(4, 4), lum(1, 1); se = lambda x: x.std() / np.sqrt(len(x))
    print(f"[direct-indep] mean (4,4) {a.mean():.5f} +- {se(a):.5f}, (1,1) {b.mean():.5f} +- {se(b):.5f}")
    assert a.mean() > 0 and abs(a.mean() - b.mean()) < 4 * np.hypot(se(a), se(b))
    l1, l4, l64 = lum(1, 0), lum(4, 0), lum(64, 0)
    ratio = np.mean((l1 - l64) ** 2) / np.mean((l4 - l64) ** 2)
    print(f"[direct-indep] var(L1 - L64) / var(L4 - L64) = {ratio:.2f}")
    assert 2 < ratio < 9


# ---------------------------------------------------------------------------------------------- 3: pool geometry
def test_pool_shapes_do_not_move_a_bit(mi, monkeypatch):
    """6000 samples of (3,2): the default shape (94 x 64 slots), 6 x 1024 and 47 x 128 (ragged last chunk) -- every pass re-reads the same camera-hit queue and adds in
    launch order, whichever slot a path sits in"""
    sc = mi.scenes.cornell_box(64, 48, 4, max_depth=2); gs = mi.Scene(sc); rng = np.random.default_rng(3)
    pairs = np.stack([rng.integers(0, sc.width, 6000), rng.integers(0, sc.height, 6000), rng.integers(0, sc.spp, 6000)], 1).astype(np.uint32)
    out = {}
    for seg, shape in ((None, (94, 64)), (6, (6, 1024)), (47, (47, 128))):
        if seg is None: monkeypatch.delenv("MI355PT_SEGMENTS", raising=False)
        else: monkeypatch.setenv("MI355PT_SEGMENTS", str(seg))
        r = direct(mi, gs, 3, 2); out[seg] = r.samples(pairs); info = r.pool_info()
        assert (info["n_seg"], info["cap"]) == shape and info["integrator"] == mi.scenes.INTEGRATOR_DIRECT
    assert (bits(out[None]) == bits(out[6])).all() and (bits(out[None]) == bits(out[47])).all() and (np.abs(out[None]).max(1) > 0).mean() > 0.3


def test_batch_sizes_and_pool_counts_give_identical_films(mi, monkeypatch):
    sc = mi.scenes.cornell_box(32, 24, 6, max_depth=2); gs = mi.Scene(sc); films = []
    for streams, planes in ((1, 1), (1, 3), (2, 1), (2, 3)):
        monkeypatch.setenv("MI355PT_STREAMS", str(streams))
        r = direct(mi, gs, 3, 2, planes_per_batch=planes); r.run(); films.append(r.read_film(0)); assert r.pool_info()["n_pools"] == streams
    assert all((bits(f) == bits(films[0])).all() for f in films[1:]) and films[0][..., :3].max() > 0


# ---------------------------------------------------------------------------------------------- 4: around it
def test_field_channels_next_to_direct_equal_those_next_to_path(mi):
    sc = mi.scenes.cornell_box(32, 24, 4, max_depth=2); gs = mi.Scene(sc); names = ["position", "distance", "shNormal", "albedo", "primIndex"]
    a = mi.Render(gs, fields=names); a.run(); b = direct(mi, gs, 4, 4, fields=names); b.run()
    assert (bits(a.read_fields(0)) == bits(b.read_fields(0))).all() and np.abs(b.read_fields(0)).max() > 0 and b.read_film(0)[..., :3].max() > 0


def test_edits_in_place_equal_a_fresh_commit(mi):
    S = mi.scenes; A = S.cornell_box(32, 24, 4, max_depth=2); B = S.cornell_box(32, 24, 4, max_depth=2)
    B.cam_to_world = S.look_at((200.0, 300.0, -700.0), (278.0, 273.0, 280.0), (0.0, 1.0, 0.0)).astype(np.float32)
    B.emitters = [dict(e, radiance=tuple(0.5 * x for x in e["radiance"][::-1])) for e in A.emitters]
    gs = mi.Scene(A); r = direct(mi, gs, 3, 2); r.run(); before = r.read_film(0)
    gs.update_camera(B.sample_to_camera, B.cam_to_world, B.near, B.far); gs.update_emitters(B.emitters)
    with pytest.raises(mi.MiError, match="mi_render_clear"):
        r.run()
    r.clear(); r.run(); edited = r.read_film(0)
    f = direct(mi, mi.Scene(B), 3, 2); f.run(); fresh = f.read_film(0)
    assert (bits(edited) == bits(fresh)).all() and not (bits(edited) == bits(before)).all() and r.stats()["rays"] == f.stats()["rays"]


def test_host_integrator_direct_equals_render(mi):
    sc = mi.scenes.cornell_box(32, 24, 4, max_depth=2); gs = mi.Scene(sc)
    h = mi.api.HostIntegrator(gs, integrator=mi.scenes.INTEGRATOR_DIRECT, emitter_samples=3, bsdf_samples=2)
    target = np.zeros((sc.height + 2, sc.width + 2, 4), np.float32); assert h.render("responsive", target) == 0
    r = direct(mi, gs, 3, 2, opacity=True); r.run()
    assert (bits(target) == bits(r.read_film(1))).all() and target[..., :3].max() > 0
    with pytest.raises(RuntimeError, match="m_emitterSamples \\+ m_bsdfSamples > 0"):
        mi.api.HostIntegrator(gs, integrator=mi.scenes.INTEGRATOR_DIRECT, emitter_samples=0, bsdf_samples=0)


def test_refusals_by_name(mi):
    S = mi.scenes
    with pytest.raises(mi.MiError, match="direct integrator does not implement `mixturebsdf`"):
        direct(mi, mi.Scene(S.layered_room(W, H, SPP)))
    with pytest.raises(mi.MiError, match="direct integrator does not support participating media"):
        direct(mi, mi.Scene(S.fog_box(W, H, SPP)))
    gs = mi.Scene(make(mi, "cornell_box"))
    with pytest.raises(mi.MiError, match="emitterSamples and bsdfSamples must not both be 0"):
        direct(mi, gs, 0, 0)
    with pytest.raises(mi.MiError, match="independent sampler stream numbers 256 draws"):
        direct(mi, mi.Scene(make(mi, "cornell_box", sampler=0)), 128, 64)
    with pytest.raises(mi.MiError, match="beyond 2\\^22"):
        direct(mi, gs, 1 << 21, 1)
    assert direct(mi, gs, 64, 64).samples(all_pairs(gs.sc)[:64]).shape == (64, 3)      # 128 light-transport samples per camera sample: fine
