"""GPU (MI355X): instance edits of a committed scene (mi_scene_update_instances; Scene.update_instances of mitsuba-im_amd/api.py): the instance records and the padded
boxes of their leaves by k_instance_records, the scene-level tree refitted by k_refit (csrc/kernels_geometry.hip over csrc/geometry_records.h), the scene box and the
bounding spheres by the commit's own pieces on the host.

The rule under test is that of tests/test_gpu_live_edit.py, whose helpers and criteria are used as they are: after an update every result equals what a fresh commit
with the new instances gives.  Every case commits A, creates the Render, traces 20 000 random (px, py, sample) triples (the four corners forced), updates to B's
placements and requires
  * the samples to equal a fresh mi.Scene(B)'s bit for bit;
  * the mi_intersection records of B's camera rays to equal the fresh scene's byte for byte (the `instance` field is part of the record);
  * revision() to go from (r, 1) to (r + 1, 1) -- no tree build;
  * the device tables nodes, leaf_records, instances, scene_box to equal those of a clone() of the edited scene (which uploads the host-refreshed mirrors: device
    arithmetic = host arithmetic), `instances` to equal the fresh scene's in every word but `root`, and scene_box to equal the fresh scene's.
Every scene is 48 x 32 at 4 spp.  B is clone(A) with the instances of a second generator call: the generator's seed also seeds the sampler, so only the placements may
differ.  The bounds on the share of triples an edit must change are half or less of what the oracle alone gives for A against B (quoted with each case)."""
import ctypes as C
import importlib
import os
import numpy as np
import pytest
from tests.conftest import GOLDEN
from tests.test_gpu_live_edit import bits, triples, clone, check, with_camera, N

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT_WORD = 27      # InstanceD: to_world 12 words, to_object 12, glo 3, root


def placed(sc, instances):
    """the description with other instance records; everything else shared"""
    out = clone(sc); out["instances"] = list(instances); return out


def garden(S, n_side=4, seed=0):
    return S.instanced_garden(48, 32, 4, n_side=n_side, seed=seed)


def garden_pair(S, n_side=4):
    A = garden(S, n_side); other = garden(S, n_side, seed=1)
    assert (A.pos == other.pos).all() and (A.idx == other.idx).all() and A.shapes == other.shapes and [i["group"] for i in A.instances] == [i["group"] for i in other.instances]
    return A, placed(A, other.instances)


def compare_tables(gs, fresh):
    twin = gs.clone()
    for what in ("nodes", "leaf_records", "instances", "scene_box"):
        a = gs.read_geometry(what); b = twin.read_geometry(what)
        assert a.shape == b.shape and (a == b).all(), (what, int((a != b).any(1).sum()) if a.shape == b.shape else (a.shape, b.shape))
    twin.close()
    a = gs.read_geometry("instances").copy(); b = fresh.read_geometry("instances").copy(); a[:, ROOT_WORD] = 0; b[:, ROOT_WORD] = 0
    assert a.shape == b.shape and (a == b).all(), int((a != b).any(1).sum())
    assert (gs.read_geometry("scene_box") == fresh.read_geometry("scene_box")).all()


def same_intersections(gs, fresh_scene, sc, tag, n=4000, instances=True):
    """Scene::rayIntersect records of the scene's camera rays through n random film positions: byte for byte those of the fresh scene"""
    rays = gs.camera_rays(np.random.default_rng(5).random((n, 2)).astype(f32) * np.asarray((sc.width, sc.height), f32))
    recs = gs.ray_intersect(rays); hit = recs["valid"] != 0; assert hit.mean() > 0.05, tag
    if instances: assert (recs["instance"][hit] >= 0).any(), tag
    assert recs.tobytes() == fresh_scene.ray_intersect(rays).tobytes(), tag


def edit_and_compare(mi, oracle, A, B, tag, min_changed, how="share", gs=None, r=None, n_oracle=N, builds=1, instances_visible=True):
    """commit A, create the render, move the instances to B's, compare with a fresh scene of B and (how) with the oracle on B; returns (scene, render, samples before, samples after)"""
    if gs is None:
        gs = mi.Scene(clone(A)); r = mi.Render(gs)
    pairs = triples(B); before = r.samples(pairs)
    rev0, nb = gs.revision(); assert nb == builds
    gs.update_instances(B.instances)
    assert gs.revision() == (rev0 + 1, builds)
    got = r.samples(pairs)
    fresh_scene = mi.Scene(clone(B)); fresh = mi.Render(fresh_scene).samples(pairs)
    assert (bits(got) == bits(fresh)).all(), (tag, int((bits(got) != bits(fresh)).any(1).sum()))
    changed = float((bits(got) != bits(before)).any(1).mean()); print(f"[instance-edit] {tag}: {changed:.3f} of the triples changed")
    if min_changed is not None: assert changed > min_changed, (tag, changed)
    if how: check(got[:n_oracle], oracle.Oracle(B).render_samples(pairs[:n_oracle])["li"], how, tag)
    same_intersections(gs, fresh_scene, B, tag, instances=instances_visible)
    assert gs.revision() == (rev0 + 1, builds) and fresh_scene.revision() == (0, 1)
    compare_tables(gs, fresh_scene)
    fresh_scene.close()
    return gs, r, before, got


# ---------------------------------------------------------------------------------------------- 1. the garden, both node kinds
@pytest.mark.parametrize("bvh2", ["1", "0"])
def test_garden(mi, oracle, monkeypatch, bvh2):
    """all 16 placements change in rotation, non-uniform scale and translation; binary and 4-wide scene-level nodes.  The oracle alone: 0.40 of the triples change."""
    monkeypatch.setenv("MI355PT_BVH2", bvh2)
    S = mi.scenes; A, B = garden_pair(S)
    assert len(A.instances) == 16 and all(not np.array_equal(a["to_world"], b["to_world"]) for a, b in zip(A.instances, B.instances))
    gs, r, _, _ = edit_and_compare(mi, oracle, A, B, f"garden bvh2={bvh2}", 0.05)
    nodes = gs.read_geometry("nodes"); assert len(nodes) > 16


# ---------------------------------------------------------------------------------------------- 2. out of the scene box and back
def test_instance_leaves_the_scene_box_and_comes_back(mi, oracle):
    """one crate goes far outside: the scene box grows and with it the constant sky's bounding sphere (the oracle alone: 0.056 of the triples change); the edit back
    restores the first samples and the first scene box bit for bit -- a refit that only grew boxes would fail here"""
    S = mi.scenes; A = garden(S); crate = next(i for i, x in enumerate(A.instances) if x["group"] == 1)
    far = list(A.instances); far[crate] = S.make_instance(1, S.translate(30, 25, 40) @ S.rotate((0, 1, 0), 30.0) @ S.scale(3, 2, 3)); B = placed(A, far)
    gs = mi.Scene(clone(A)); r = mi.Render(gs); box0 = gs.read_geometry("scene_box"); nodes0 = gs.read_geometry("nodes")
    gs, r, first, _ = edit_and_compare(mi, oracle, A, B, "crate far away", 0.01, gs=gs, r=r, n_oracle=4000, instances_visible=True)
    box1 = gs.read_geometry("scene_box").view(f32)[0]; assert box1[3] > 30 and box1[4] > 25 and box1[5] > 40 and (box0.view(f32)[0][3:] < 20).all()
    gs, r, _, last = edit_and_compare(mi, oracle, B, A, "crate back", 0.01, how=None, gs=gs, r=r)
    assert (bits(last) == bits(first)).all() and (gs.read_geometry("scene_box") == box0).all() and (gs.read_geometry("nodes") == nodes0).all()
    assert gs.revision() == (2, 1)


# ---------------------------------------------------------------------------------------------- 3. counts around the wave and workgroup sizes
def outwards(S, sc, which):
    """the instances at the indices `which` moved far outwards, one per face of the scene box in the order -x, +x, -z, +z, +y, -y"""
    faces = [(0, -40.0), (0, 40.0), (2, -40.0), (2, 40.0), (1, 40.0), (1, -40.0)]; out = list(sc.instances)
    for i, (axis, where) in zip(which, faces):
        tw = np.asarray(out[i]["to_world"], np.float64).copy(); tw[axis, 3] = where      # its placed origin goes to +-40 on that axis
        out[i] = S.make_instance(out[i]["group"], tw)
    return placed(sc, out)


@pytest.mark.parametrize("n_side,min_changed", [(1, 0.01), (9, 0.05), (17, 0.05)])
def test_instance_counts_around_wave_and_workgroup(mi, oracle, n_side, min_changed):
    """1, 81 and 289 instances (the oracle alone: 0.04, 0.49, 0.60 of the triples change).  Then, for 81 and 289, the instances at 0, 63, 64 and n - 1 (and 255, 256)
    go far outwards, each along an axis of its own: the first and last lanes of a wave and of a workgroup each define a face of the scene box."""
    S = mi.scenes; A, B = garden_pair(S, n_side); n = n_side * n_side; assert len(A.instances) == n
    gs, r, _, _ = edit_and_compare(mi, oracle, A, B, f"n_side={n_side}", min_changed, n_oracle=4000, instances_visible=n_side > 1)
    if n_side == 1: return
    which = [0, 63, 64, n - 1] + ([255, 256] if n > 256 else [])
    C2 = outwards(S, B, which)
    gs, r, _, _ = edit_and_compare(mi, oracle, B, C2, f"n_side={n_side}, lanes {which}", None, how=None, gs=gs, r=r)      # the moved instances may all be off screen: the box below shows the edit
    box = gs.read_geometry("scene_box").view(f32)[0]
    assert box[0] < -35 and box[3] > 35 and box[2] < -35 and box[5] > 35 and ((box[4] > 35 and box[1] < -35) if n > 256 else (box[4] < 20 and box[1] > -5))
    assert gs.revision() == (2, 1)


# ---------------------------------------------------------------------------------------------- 4. interpenetrating instances
def test_interpenetrating_instances(mi, oracle):
    """two bushes moved into each other (different transforms, no exact ties in t): compared with the fresh scene only"""
    S = mi.scenes; A = garden(S); bushes = [i for i, x in enumerate(A.instances) if x["group"] == 0][:2]; inst = list(A.instances)
    inst[bushes[0]] = S.make_instance(0, S.translate(0.0, 0.0, -1.0) @ S.rotate((0, 1, 0), 17.0) @ S.scale(1.3, 1.2, 1.1))
    inst[bushes[1]] = S.make_instance(0, S.translate(0.45, 0.1, -0.8) @ S.rotate((0, 1, 0), 64.0) @ S.rotate((1, 0, 0), 5.0) @ S.scale(1.1, 1.4, 1.2))
    gs, r, _, _ = edit_and_compare(mi, oracle, A, placed(A, inst), "interpenetrating bushes", None, how=None)
    rays = gs.camera_rays(np.random.default_rng(5).random((4000, 2)).astype(f32) * np.asarray((A.width, A.height), f32)); recs = gs.ray_intersect(rays)
    assert (recs["instance"] == bushes[0]).any() and (recs["instance"] == bushes[1]).any()      # both are seen: neither hides the other


# ---------------------------------------------------------------------------------------------- 5. a sequence on one handle
def recommit_instances(gs, instances):
    """mi_scene_set_instances + mi_scene_commit on the SAME handle (a render handle does not survive this)"""
    L = gs.L; M = importlib.import_module(type(gs).__module__); instances = list(instances)
    L.check(L.L.mi_scene_set_instances(gs.h, C.cast(M.pack_instances(instances), C.c_void_p), len(instances)))
    L.check(L.L.mi_scene_commit(gs.h, 0)); gs.sc.instances = instances


def test_sequence_on_one_handle(mi, oracle):
    """instances -> camera -> materials (the wood turns black: a flag flip inside a group) -> instances back -> materials and camera back: each step equals a fresh
    scene, the last the very first render; one tree build throughout.  Then a recommit on the same handle and another edit: the edit state of the old tree is gone."""
    S = mi.scenes; A, B = garden_pair(S); pairs = triples(A)
    gs = mi.Scene(clone(A)); r = mi.Render(gs); first = r.samples(pairs)
    state = {"rev": 0}

    def same_as_fresh(desc, tag):
        state["rev"] += 1; assert gs.revision() == (state["rev"], 1), tag
        fresh_scene = mi.Scene(clone(desc)); got = r.samples(pairs); fresh = mi.Render(fresh_scene).samples(pairs)
        assert (bits(got) == bits(fresh)).all(), tag
        same_intersections(gs, fresh_scene, desc, tag); fresh_scene.close()
    gs.update_instances(B.instances); same_as_fresh(B, "instances")
    D = with_camera(S, B, (6.0, 3.0, -7.0), (0.0, 0.6, 0.5), 48.0); gs.update_camera(D.sample_to_camera, D.cam_to_world, D.near, D.far); same_as_fresh(D, "camera")
    E = clone(D); E.bsdfs[2]["reflectance"] = (0.0, 0.0, 0.0); gs.update_materials(E.bsdfs); same_as_fresh(E, "materials")
    gs.update_instances(A.instances); same_as_fresh(placed(E, A.instances), "instances back")
    gs.update_materials(A.bsdfs); gs.update_camera(A.sample_to_camera, A.cam_to_world, A.near, A.far)
    assert (bits(r.samples(pairs)) == bits(first)).all() and gs.revision() == (6, 1)
    r.close()
    gs.update_instances(B.instances)                      # leaves edit state (stale host mirrors included) behind for the commit to drop
    recommit_instances(gs, B.instances); assert gs.revision() == (7, 2)
    fresh = mi.Scene(clone(B))
    for what in ("nodes", "leaf_records", "instances", "scene_box"):
        assert (gs.read_geometry(what) == fresh.read_geometry(what)).all(), what
    fresh.close()
    edit_and_compare(mi, oracle, B, A, "after the recommit", 0.05, how=None, gs=gs, r=mi.Render(gs), builds=2)


# ---------------------------------------------------------------------------------------------- 6. fields, film rule
def test_fields_follow_the_edit_and_the_film_is_never_mixed(mi, oracle):
    """position and shapeIndex fields: after the edit a run without clear() is refused (the film holds samples of the earlier placement); after clear() and a run the
    field film and the radiance film equal a fresh scene's bit for bit"""
    S = mi.scenes; A, B = garden_pair(S); F = [("position", (-1.0, 2.5, 7.0)), ("shapeIndex", -7.0)]
    gs = mi.Scene(clone(A)); r = mi.Render(gs, fields=F); r.run(s1=2); old = r.read_fields(2)
    gs.update_instances(B.instances); assert gs.revision() == (1, 1)
    with pytest.raises(mi.MiError) as e:
        r.run()
    assert e.value.code == 1 and "mi_render_clear" in str(e.value)
    r.clear(); r.run(s1=2)
    fresh_scene = mi.Scene(clone(B)); fr = mi.Render(fresh_scene, fields=F); fr.run(s1=2)
    got = r.read_fields(2); ref = fr.read_fields(2)
    assert (bits(got) == bits(ref)).all() and (bits(r.read_film(0)) == bits(fr.read_film(0))).all()
    assert (bits(got) != bits(old)).any(2).mean() > 0.05
    p = triples(B, 4000); assert (bits(r.field_samples(p)) == bits(fr.field_samples(p))).all()


# ---------------------------------------------------------------------------------------------- 7. host mirror
def _host_render(mi, gs, sc, devices):
    h = mi.api.HostIntegrator(gs, devices=devices, planes_per_batch=4)
    target = np.zeros((sc.height + 2, sc.width + 2, 4), f32)
    assert h.render("responsive", target) == 0
    return h, target


def test_host_mirror_set_instances_on_replicas(mi):
    """MIPathTracerHIP::setInstances between two render() calls: with devices = (0, 0) both replicas move -- the second target equals that of one device and that of a
    host integrator on a fresh scene of B, bit for bit"""
    S = mi.scenes; A, B = garden_pair(S); targets = {}
    for devices in ((0,), (0, 0)):
        gs = mi.Scene(clone(A)); h, first = _host_render(mi, gs, A, devices)
        h.set_instances(B.instances)
        t = np.zeros_like(first); assert h.render("responsive", t) == 0
        assert gs.revision() == (1, 1) and (bits(t) != bits(first)).any(2).mean() > 0.05
        fresh_scene = mi.Scene(clone(B)); same_intersections(gs, fresh_scene, B, f"replicas {devices}")
        fh, fresh = _host_render(mi, fresh_scene, B, devices)
        assert (bits(t) == bits(fresh)).all(), devices
        targets[devices] = t; h.close(); fh.close()
    assert (bits(targets[(0, 0)]) == bits(targets[(0,)])).all()


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_on_a_committed_scene(mi):
    """wrong count, a changed group (code 3, the message names the instance), a NaN in to_object, a scene without instances: revision() and the samples stay"""
    S = mi.scenes; A = garden(S); gs = mi.Scene(clone(A)); r = mi.Render(gs); pairs = triples(A, 4000); before = r.samples(pairs)

    def refused(instances, code, *words):
        with pytest.raises(mi.MiError) as e:
            gs.update_instances(instances)
        assert e.value.code == code and "mi_scene_update_instances: " in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
        assert gs.revision() == (0, 1) and gs.sc.instances is not instances
    refused(A.instances[:-1], 1, "16 -> 15")
    other = [dict(x) for x in A.instances]; other[5]["group"] = 1 - other[5]["group"]; refused(other, 3, "instance 5", "group")
    nan = [dict(x) for x in A.instances]; nan[9]["to_object"] = nan[9]["to_object"].copy(); nan[9]["to_object"][1, 2] = np.nan; refused(nan, 1, "instance 9", "to_object")
    assert (bits(r.samples(pairs)) == bits(before)).all()
    cb = S.cornell_box(48, 32, 4); cs = mi.Scene(clone(cb)); cr = mi.Render(cs); cp = triples(cb, 2000); cbefore = cr.samples(cp)
    with pytest.raises(mi.MiError) as e:
        cs.update_instances(A.instances)
    assert e.value.code == 1 and "mi_scene_update_instances: " in str(e.value) and "the scene has no instances" in str(e.value)
    assert cs.revision() == (0, 1) and (bits(cr.samples(cp)) == bits(cbefore)).all()
    assert cs.read_geometry("instances").shape == (0, 32) and cs.read_geometry("scene_box").shape == (1, 6)


# ---------------------------------------------------------------------------------------------- 9. command line
def test_render_cli_spin(mi, tmp_path, capsys):
    """python -m mitsuba-im_amd.render --spin 3: one commit, three in-place instance edits, three images; every frame equals the render of a scene committed with that
    frame's transforms; a scene without instances ends with a message"""
    X = importlib.import_module("mitsuba-im_amd.xml_scene"); cli = importlib.import_module("mitsuba-im_amd.render")
    path = os.path.join(GOLDEN, "scenes", "crate_garden.xml"); out = str(tmp_path / "spin.npy")
    assert cli.main([path, "-o", out, "--spin", "3", "--spin-axis", "y"]) == 0
    line = capsys.readouterr().out
    assert "once (1 tree build, 3 instance edits)" in line and "per frame" in line
    frames = [np.load(str(tmp_path / f"spin_{f:03d}.npy")) for f in range(3)]
    sc = X.load_scene(path); assert len(sc.instances) == 4
    for f, insts in enumerate(cli.spin_instances(sc, 3, "y")):
        r = mi.Render(mi.Scene(placed(sc, insts))); r.run()
        assert (bits(r.read_film(2)) == bits(frames[f])).all(), f
    assert not (bits(frames[0]) == bits(frames[1])).all() and not (bits(frames[1]) == bits(frames[2])).all()
    assert cli.main([os.path.join(GOLDEN, "scenes", "sky_ball.xml"), "-o", out, "--spin", "3"]) == 1 and "has none" in capsys.readouterr().err
