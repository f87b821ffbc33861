"""GPU (MI355X): in-place edits of a committed scene (mi_scene_update_camera / _materials / _emitters / _envmap_transform; Scene.update_* of mitsuba-im_amd/api.py).

The rule under test: after an update every result equals what a fresh commit with the new parameters gives.  Every case commits the GPU scene from the factory's
description A, creates a Render, updates scene and render to the edited description B and compares 20 000 random (px, py, sample) triples (the four film corners
forced) with
  * the oracle on B, under the criterion the existing parity test of that scene family applies against the oracle (tests/test_gpu_parity.py): "bits" = bit equality
    (all-diffuse scenes and the smooth BSDFs, which never call the math library), "share" = bit_share > 0.9999 (libm enters: rough conductors, the spot's transition
    zone), "vol" = test_volpath_simple's (share > 0.999 and rtol 1e-5), "env" = test_filtered_environment_lookups' (the EWA footprint moves with last-bit changes);
  * a fresh mi.Scene(B): bit for bit, always -- per-sample results are deterministic, so this is an identity;
and Scene.revision() reports one tree build throughout."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32
N = 20000


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def triples(sc, n=N, seed=11):
    rng = np.random.default_rng(seed)
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    pairs[:4] = [[0, 0, 0], [sc.width - 1, sc.height - 1, sc.spp - 1], [sc.width - 1, 0, 0], [0, sc.height - 1, sc.spp - 1]]
    return pairs


def clone(sc):
    """a copy of the description whose records can be edited without touching the original (the geometry arrays are shared: no edit touches them)"""
    out = type(sc)(sc)
    out["bsdfs"] = [dict(b) for b in sc.bsdfs]; out["emitters"] = [dict(e) for e in sc.emitters]
    if sc.envmap is not None: out["envmap"] = dict(sc.envmap)
    return out


def with_camera(S, sc, origin, target, fov, up=(0, 1, 0)):
    out = clone(sc)
    out["cam_to_world"] = S.look_at(origin, target, up); out["xfov"] = float(fov)
    out["sample_to_camera"] = S.sample_to_camera(fov, sc.near, sc.far, sc.width / sc.height)
    return out


def check(got, ref, how, tag):
    same = (bits(got) == bits(ref)).all(1); share = float(same.mean())
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    print(f"[live-edit] {tag}: bit share vs oracle {share:.5f}, max rel err {float(err.max()):.3g}")
    if how == "bits": assert same.all(), (tag, int((~same).sum()))
    elif how == "share": assert share > 0.9999, (tag, share)
    elif how == "vol": assert share > 0.999 and np.allclose(got, ref, rtol=1e-5, atol=1e-7), (tag, share)
    elif how == "env": assert (err < 1e-5).mean() > 0.95 and (err < 1e-3).mean() > 0.995 and err.max() < 5e-3, (tag, float((err < 1e-5).mean()), float(err.max()))
    else: raise ValueError(how)


def apply_edit(gs, B, kind):
    if kind == "camera": gs.update_camera(B.sample_to_camera, B.cam_to_world, B.near, B.far)
    elif kind == "materials": gs.update_materials(B.bsdfs)
    elif kind == "emitters": gs.update_emitters(B.emitters)
    elif kind == "envmap": gs.update_envmap(B.envmap["to_world"], B.envmap["scale"])
    else: raise ValueError(kind)


def edit_and_compare(mi, oracle, A, B, kind, how, tag, gs=None, r=None):
    """commit A, create the render, update to B, compare with the oracle on B and with a fresh scene of B; returns (scene, render, oracle of B)"""
    if gs is None:
        gs = mi.Scene(clone(A)); r = mi.Render(gs)
    pairs = triples(B); orc = oracle.Oracle(B)
    before = r.samples(pairs)                     # the render has traced the scene as it was: its copy of the scene record must follow the edit
    rev0, builds = gs.revision(); assert builds == 1
    apply_edit(gs, B, kind)
    assert gs.revision() == (rev0 + 1, 1)
    got = r.samples(pairs); check(got, orc.render_samples(pairs)["li"], how, tag)
    fresh_scene = mi.Scene(clone(B)); fresh = mi.Render(fresh_scene).samples(pairs)
    assert (bits(got) == bits(fresh)).all(), (tag, int((bits(got) != bits(fresh)).any(1).sum()))
    assert (bits(got) != bits(before)).any(1).mean() > 0.05, tag          # the edit is visible: the comparison above is not one of A with A
    assert gs.revision()[1] == 1 and fresh_scene.revision() == (0, 1)
    return gs, r, orc


# ---------------------------------------------------------------------------------------------- camera
def test_camera_packet_scene(mi, oracle):
    """cornell_box (32 triangles: the packet path): a view from inside the box with another field of view; the camera rays themselves equal the oracle's bit for bit."""
    S = mi.scenes; A = S.cornell_box(96, 64, 4); B = with_camera(S, A, (278, 273, 100), (180, 200, 500), 62.0)
    gs, r, orc = edit_and_compare(mi, oracle, A, B, "camera", "bits", "camera cornell")
    pos = orc.render_samples(triples(B, 2000))["pos"]; rays = gs.camera_rays(pos)
    for i in range(0, len(pos), 7):
        assert (bits(rays[i]) == bits(orc.camera_ray(float(pos[i, 0]), float(pos[i, 1])))).all(), i
    # ... and Scene::rayIntersect sees the same scene from the new camera as a fresh one does
    recs = gs.ray_intersect(rays); fresh = mi.Scene(clone(B)).ray_intersect(rays)
    assert recs.tobytes() == fresh.tobytes()


def test_camera_leaves_the_scene_box(mi, oracle):
    """sky_view: the new camera sits far outside the scene's box, so the bounding sphere of the environment emitter (which includes the sensor position) changes --
    and with it the emitter-sampling rays towards the map."""
    S = mi.scenes; A = S.sky_view(); B = with_camera(S, A, (3.0, 6.0, -30.0), (0.0, 1.0, 0.0), 30.0)
    edit_and_compare(mi, oracle, A, B, "camera", "env", "camera sky_view")


def test_camera_with_point_and_spot_emitters(mi, oracle):
    S = mi.scenes; A = S.cbox_lights(); B = with_camera(S, A, (400, 300, -1500), (250, 250, 200), 25.0)
    edit_and_compare(mi, oracle, A, B, "camera", "share", "camera cbox_lights")


def test_camera_tree_scene_with_instances_and_fields(mi, oracle):
    """instanced_garden (the tree path, two-level): radiance as above; the field channels of the same render follow the camera too -- position against the
    intersection records of the new camera rays, relPosition against the float64 inverse of the NEW world transform (the bound of tests/test_gpu_fields.py)."""
    S = mi.scenes; A = S.instanced_garden(); B = with_camera(S, A, (6.0, 3.0, -7.0), (0.0, 0.6, 0.5), 48.0)
    UNDEF = (-1.0, 2.5, 7.0)
    gs = mi.Scene(clone(A)); r = mi.Render(gs, fields=[("relPosition", UNDEF), ("position", UNDEF)])
    r.field_samples(triples(A, 64))
    gs, r, orc = edit_and_compare(mi, oracle, A, B, "camera", "share", "camera instanced_garden", gs=gs, r=r)
    pairs = triples(B, 4000, seed=7); got = r.field_samples(pairs)
    pos = orc.render_samples(pairs)["pos"]; recs = gs.ray_intersect(gs.camera_rays(pos)); hit = recs["valid"] != 0
    assert hit.mean() > 0.2 and (recs["instance"][hit] >= 0).mean() > 0.1
    assert (bits(got[hit, 1]) == bits(recs["p"][hit])).all() and (bits(got[~hit]) == bits(np.asarray(UNDEF, f32))).all()
    M = np.linalg.inv(np.asarray(B.cam_to_world, np.float64)).astype(f32).astype(np.float64)[:3]
    p = got[hit, 1].astype(np.float64); rel = got[hit, 0].astype(np.float64)
    bound = 4 * 2.0 ** -23 * (np.abs(p)[:, None, :] * np.abs(M[:, :3])[None]).sum(2) + 4 * 2.0 ** -23 * np.abs(M[:, 3])
    err = np.abs(rel - (p @ M[:, :3].T + M[:, 3]))
    assert (err <= bound).all(), float((err / bound).max())
    fresh = mi.Render(mi.Scene(clone(B)), fields=[("relPosition", UNDEF), ("position", UNDEF)]).field_samples(pairs)
    assert (bits(got) == bits(fresh)).all()


def test_camera_volumetric_render(mi, oracle):
    """fog_box (volpath_simple): a render handle of a volumetric integrator follows the camera (its environment-hit distance is recomputed with the scene record)."""
    S = mi.scenes; A = S.fog_box(); B = with_camera(S, A, (450, 400, -600), (200, 200, 300), 50.0)
    edit_and_compare(mi, oracle, A, B, "camera", "vol", "camera fog_box")


# ---------------------------------------------------------------------------------------------- materials
def test_materials_flag_bits_flip_and_flip_back(mi, oracle):
    """cornell_box: a new colour on the red wall, and the white material's reflectance set to zero -- a `diffuse` without any component is not smooth, so the
    no-emitter-sampling bit flips on the 26 (of 32) triangles that use it: less than one wave of the patch kernel.  Then back to A."""
    S = mi.scenes; A = S.cornell_box(96, 64, 4); B = clone(A)
    assert sum(s["tri_count"] for s in A.shapes if s["bsdf"] == 0) == 26 and len(A.idx) == 32
    B.bsdfs[1]["reflectance"] = (0.1, 0.2, 0.7); B.bsdfs[0]["reflectance"] = (0.0, 0.0, 0.0)
    gs, r, _ = edit_and_compare(mi, oracle, A, B, "materials", "bits", "materials cornell")
    gs, r, _ = edit_and_compare(mi, oracle, B, A, "materials", "bits", "materials cornell, back", gs=gs, r=r)
    assert gs.revision() == (2, 1)


def test_materials_group_members_and_twosided(mi, oracle):
    """instanced_garden (its triangle count is no multiple of 64): the wood of the crates -- members of a shape group -- turns black (flag flip inside a group), the
    ground becomes twosided (back-side bit of a scene-level mesh), the leaves' colour changes."""
    S = mi.scenes; A = S.instanced_garden(); B = clone(A)
    assert len(A.idx) % 64 != 0 and any(s.get("group", 0) and s["bsdf"] == 2 for s in A.shapes) and not any(s.get("group", 0) for s in A.shapes if s["bsdf"] == 0)
    B.bsdfs[2]["reflectance"] = (0.0, 0.0, 0.0); B.bsdfs[0]["twosided"] = 1; B.bsdfs[1]["reflectance"] = (0.6, 0.3, 0.1)
    edit_and_compare(mi, oracle, A, B, "materials", "share", "materials instanced_garden")


def test_materials_values_and_derived_weights(mi, oracle):
    """cbox_materials: conductor eta / k / specular, and a plastic's diffuse colour, which changes the specular sampling weight the library derives for it."""
    S = mi.scenes; A = S.cbox_materials(); B = clone(A)
    eta, k = S.CONDUCTOR_IOR["Cu"]; gold = next(i for i, b in enumerate(A.bsdfs) if b["type"] == S.BSDF_CONDUCTOR)
    B.bsdfs[gold]["eta"] = tuple(map(float, eta)); B.bsdfs[gold]["k"] = tuple(map(float, k)); B.bsdfs[gold]["specular"] = (0.8, 0.9, 1.0)
    for i, b in enumerate(A.bsdfs):
        if b["type"] == S.BSDF_PLASTIC and not b.get("nonlinear"): B.bsdfs[i]["reflectance"] = (0.7, 0.1, 0.05)
    edit_and_compare(mi, oracle, A, B, "materials", "bits", "materials cbox_materials")


def test_materials_rough_conductor_parameters(mi, oracle):
    """open_constant's rough-conductor sphere: alpha, eta, k."""
    S = mi.scenes; A = S.open_constant(); B = clone(A)
    rc = next(i for i, b in enumerate(A.bsdfs) if b["type"] == S.BSDF_ROUGHCONDUCTOR); eta, k = S.CONDUCTOR_IOR["Al"]
    B.bsdfs[rc]["alpha"] = 0.35; B.bsdfs[rc]["eta"] = tuple(map(float, eta)); B.bsdfs[rc]["k"] = tuple(map(float, k))
    gs = mi.Scene(clone(A)); r = mi.Render(gs); pairs = triples(A)
    apply_edit(gs, B, "materials")
    got = r.samples(pairs); ref = oracle.Oracle(B).render_samples(pairs)["li"]
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    assert (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-6          # test_scene_level_emitters' criterion for this scene (rough-conductor sphere: tolerance-pinned)
    assert (bits(got) == bits(mi.Render(mi.Scene(clone(B))).samples(pairs))).all() and gs.revision() == (1, 1)


def test_materials_on_analytic_shapes(mi, oracle):
    """shape_lights: the material of the four analytic lights loses its reflectance (the flag bits of AnalyticD), the grey of floor mesh and room sphere changes."""
    S = mi.scenes; A = S.shape_lights(96, 64); B = clone(A)
    B.bsdfs[2]["reflectance"] = (0.0, 0.0, 0.0); B.bsdfs[0]["reflectance"] = (0.3, 0.5, 0.6); B.bsdfs[1]["twosided"] = 0
    edit_and_compare(mi, oracle, A, B, "materials", "bits", "materials shape_lights")


# ---------------------------------------------------------------------------------------------- emitters
def test_emitters_area_radiance(mi, oracle):
    S = mi.scenes; A = S.cornell_box(96, 64, 4); B = clone(A); B.emitters[0]["radiance"] = (3.0, 9.0, 20.0)
    edit_and_compare(mi, oracle, A, B, "emitters", "bits", "emitters cornell")


def test_emitters_point_spot_and_weights(mi, oracle):
    S = mi.scenes; A = S.cbox_lights(); B = clone(A)
    kinds = [e["type"] for e in A.emitters]; pt, sp = kinds.index(S.EMITTER_POINT), kinds.index(S.EMITTER_SPOT)
    B.emitters[pt].update(S.point_emitter((400, 300, 250), (6e5, 3e5, 2e5), weight=0.5))
    B.emitters[sp].update(S.spot_emitter((150, 520, 120), (330, 0, 300), (1e6, 2.5e6, 2e6), cutoff=40.0, beam=12.0, weight=2.0))
    for e in B.emitters:
        if e["type"] == S.EMITTER_AREA: e["weight"] = 3.0
    edit_and_compare(mi, oracle, A, B, "emitters", "share", "emitters cbox_lights")


def test_emitters_constant_radiance(mi, oracle):
    S = mi.scenes; A = S.open_constant(); B = clone(A)
    c = next(i for i, e in enumerate(A.emitters) if e["type"] == S.EMITTER_CONSTANT); B.emitters[c]["radiance"] = (1.2, 0.6, 0.3)
    gs = mi.Scene(clone(A)); r = mi.Render(gs); pairs = triples(A)
    apply_edit(gs, B, "emitters")
    got = r.samples(pairs); ref = oracle.Oracle(B).render_samples(pairs)["li"]
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    assert (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-6          # test_scene_level_emitters' criterion for open_constant
    assert (bits(got) == bits(mi.Render(mi.Scene(clone(B))).samples(pairs))).all() and gs.revision() == (1, 1)


def test_envmap_transform(mi, oracle):
    """sky_view: the map rotated by another 90 degrees about y, scale 0.5; the image and its CDFs stay where they are."""
    S = mi.scenes; A = S.sky_view(); B = clone(A)
    B.envmap["to_world"] = (S.rotate((0, 1, 0), 90.0) @ np.asarray(A.envmap["to_world"])).astype(f32); B.envmap["scale"] = 0.5
    edit_and_compare(mi, oracle, A, B, "envmap", "env", "envmap sky_view")


# ---------------------------------------------------------------------------------------------- film and revision rule
def test_film_of_an_older_revision_is_never_mixed(mi, oracle):
    """After an update run() refuses to add to a film that holds samples of the scene before it; after clear() the film and the ray counters are those of the
    oracle on B (box filter: the criterion of test_film_vs_oracle_and_reference)."""
    S = mi.scenes; A = S.cornell_box(96, 54, 8); B = with_camera(S, A, (278, 273, 100), (180, 200, 500), 62.0); B.emitters[0]["radiance"] = (3.0, 9.0, 20.0)
    gs = mi.Scene(clone(A)); r = mi.Render(gs); r.run(s1=4)
    gs.update_camera(B.sample_to_camera, B.cam_to_world, B.near, B.far); gs.update_emitters(B.emitters)
    with pytest.raises(mi.MiError) as e:
        r.run()
    assert e.value.code == 1 and "mi_render_clear" in str(e.value)
    r.clear(); r.run(); film = r.read_film(0); st = r.stats()
    ofilm, cnt = oracle.Oracle(B).render_image(threads=4)
    same = (bits(film) == bits(ofilm)).all(2)
    print(f"[live-edit] film: same-bits share {float(same.mean()):.5f}")
    assert same.mean() > 0.995 and np.allclose(film, ofilm, rtol=2e-6, atol=1e-7)
    assert (st["rays"], st["shadow_rays"], st["path_length_sum"]) == tuple(int(c) for c in cnt)
    assert gs.revision() == (2, 1)
    r.run(s0=0, s1=2)                                   # the same revision: accumulating goes on as before


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_scene_usable(mi):
    """One refusal per rule of "values only" (MI_ERR_UNSUPPORTED = 3, the message names the record); the value checks of mi_scene_set_* still apply; after every
    refused call the scene renders what it rendered before."""
    S = mi.scenes; cases = []

    def bad(sc, kind, fn, code, word):
        b = clone(sc); fn(b); cases.append((sc, b, kind, code, word))
    cb = S.cornell_box(48, 32, 4); cm = S.cbox_materials(48, 32, 4); rp = S.cbox_roughplastic(48, 32, 4); cl = S.cbox_lights(48, 32, 4)
    bad(cb, "materials", lambda b: b.bsdfs.append(dict(b.bsdfs[0])), 3, "record count")
    bad(cb, "materials", lambda b: b.bsdfs[1].update(S.make_bsdf(kind=S.BSDF_CONDUCTOR)), 3, "material 1 changes its type")
    bad(cb, "materials", lambda b: b.bsdfs[2].update(texture=0), 3, "material 2 changes its texture binding")
    bad(cm, "materials", lambda b: b.bsdfs[4].update(nonlinear=0), 3, "material 4 changes its anisotropic / nonlinear / sampleVisible bit")
    bad(rp, "materials", lambda b: [x.update(k=(x["k"][0], x["k"][1], x["k"][2] - 1.0)) for x in b.bsdfs if x["type"] == S.BSDF_ROUGHPLASTIC][:0], 3, "rough-transmittance slice")
    bad(cm, "materials", lambda b: b.bsdfs[5].update(eta=(-1.0, 0.0, 0.0)), 1, "indices of refraction must be positive")          # a value check of mi_scene_set_materials
    bad(cb, "emitters", lambda b: b.emitters.append(dict(b.emitters[0])), 3, "record count")
    bad(cl, "emitters", lambda b: b.emitters[0].update(type=S.EMITTER_CONSTANT), 3, "emitter 0 changes its type")
    bad(cb, "emitters", lambda b: b.emitters[0].update(shape=0), 3, "emitter 0 changes its shape")
    bad(cl, "emitters", lambda b: [e.update(cutoff=5.0, beam=10.0) for e in b.emitters if e["type"] == S.EMITTER_SPOT][:0], 1, "cutoffAngle >= beamWidth")
    lr = S.layered_room(48, 32, 4); br = S.blend_room(48, 32, 4)
    mask = next(i for i, x in enumerate(lr.bsdfs) if x["type"] == S.BSDF_MASK); mix = next(i for i, x in enumerate(lr.bsdfs) if x["type"] == S.BSDF_MIXTURE)
    blend = next(i for i, x in enumerate(br.bsdfs) if x["type"] == S.BSDF_BLEND)
    bad(lr, "materials", lambda b: b.bsdfs[mask].update(distr=0), 3, f"material {mask} changes `distr` of a wrapper")
    bad(lr, "materials", lambda b: b.bsdfs[mix].update(reflectance=(b.bsdfs[mix]["reflectance"][1], b.bsdfs[mix]["reflectance"][0], b.bsdfs[mix]["reflectance"][2])), 3, f"material {mix} changes the child indices of a mixturebsdf")
    bad(br, "materials", lambda b: b.bsdfs[blend].update(eta=(b.bsdfs[blend]["eta"][1], b.bsdfs[blend]["eta"][0], 0.0)), 3, f"material {blend} changes the child indices of a blendbsdf")
    scenes = {}
    for sc, b, kind, code, word in cases:
        if id(sc) not in scenes:
            gs = mi.Scene(clone(sc)); r = mi.Render(gs); pairs = triples(sc, 2000); scenes[id(sc)] = (gs, r, pairs, r.samples(pairs))
        gs, r, pairs, before = scenes[id(sc)]; rev = gs.revision(); described = (list(gs.sc.bsdfs), list(gs.sc.emitters))
        with pytest.raises(mi.MiError) as e:
            apply_edit(gs, b, kind)
        assert e.value.code == code and word in str(e.value), (word, str(e.value))
        assert gs.revision() == rev and (list(gs.sc.bsdfs), list(gs.sc.emitters)) == described
        assert (bits(r.samples(pairs)) == bits(before)).all(), word
    # an envmap transform on a scene without an envmap
    gs = scenes[id(cb)][0]
    with pytest.raises(mi.MiError) as e:
        gs.update_envmap(np.eye(4, dtype=f32), 1.0)
    assert e.value.code == 1 and "no envmap" in str(e.value)
    assert len(cases) == 13


# ---------------------------------------------------------------------------------------------- host mirror
def _host_render(mi, gs, sc, devices):
    h = mi.api.HostIntegrator(gs, devices=devices, planes_per_batch=4)
    target = np.zeros((sc.height + 2, sc.width + 2, 4), np.float32)
    assert h.render("responsive", target) == 0
    return h, target


@pytest.mark.parametrize("devices", [(0,), (0, 0)])
def test_host_mirror_set_camera(mi, golden_scenes, devices):
    """MIPathTracerHIP::setCamera between two render() calls, no preprocess in between: the second target is that of a fresh scene with the new camera -- one device:
    bit for bit (test_host_mirror_controls' criterion); devices = (0, 0): both replicas must have moved, the merged film equals the single-device film as in
    test_host_mirror_devices_replicas (box filter: own-pixel sums only, edge splats aside)."""
    S = mi.scenes; A = golden_scenes["cornell_small"]; B = with_camera(S, A, (278, 273, 100), (180, 200, 500), 62.0)
    gs = mi.Scene(clone(A)); h, first = _host_render(mi, gs, A, devices)
    h.set_camera(B.sample_to_camera, B.cam_to_world, B.near, B.far)
    target = np.zeros_like(first); assert h.render("responsive", target) == 0
    r = mi.Render(mi.Scene(clone(B)), opacity=True); r.run(); ref = r.read_film(1)
    same = (bits(target) == bits(ref)).all(2)
    assert not (bits(target) == bits(first)).all()
    if len(devices) == 1:
        assert same.all()
    else:
        assert same[1:-1, 1:-1].mean() > 0.999 and np.allclose(target, ref, rtol=1e-6, atol=1e-7)
    assert gs.revision() == (1, 1)
    h.close()


# ---------------------------------------------------------------------------------------------- command line
def test_render_cli_orbit(mi, tmp_path, capsys):
    """python -m mitsuba-im_amd.render --orbit 3: one commit, three in-place camera edits, three images; frame 0 is the scene's own view, frame 1 equals the render of a
    fresh scene with that frame's camera; the summary line reports the build once."""
    import importlib
    import os
    from tests.conftest import GOLDEN
    X = importlib.import_module("mitsuba-im_amd.xml_scene"); cli = importlib.import_module("mitsuba-im_amd.render")
    path = os.path.join(GOLDEN, "scenes", "sky_ball.xml"); out = str(tmp_path / "turn.npy")
    assert cli.main([path, "-o", out, "--orbit", "3", "--orbit-axis", "y", "--spp", "4"]) == 0
    line = capsys.readouterr().out
    assert "upload+BVH" in line and "once (1 tree build, 3 camera edits)" in line and "per frame" in line
    frames = [np.load(str(tmp_path / f"turn_{f:03d}.npy")) for f in range(3)]
    sc = X.load_scene(path); sc.spp = 4; cams = cli.orbit_cameras(sc, 3, "y")
    for f in (0, 1):
        b = clone(sc); b["cam_to_world"] = cams[f]
        r = mi.Render(mi.Scene(b)); r.run()
        assert (bits(r.read_film(2)) == bits(frames[f])).all(), f
    assert not (bits(frames[0]) == bits(frames[1])).all() and not (bits(frames[1]) == bits(frames[2])).all()
