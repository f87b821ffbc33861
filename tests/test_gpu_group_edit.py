"""GPU (MI355X): geometry edits of a committed scene (mi_scene_update_geometry; Scene.update_geometry of mitsuba-im_amd/api.py): new vertices for the whole vertex
array, the members of shape groups included, and / or new instance transforms in ONE call -- the per-triangle records by k_tri_records, the group boxes taken into
InstanceD::glo / ghi and the instance leaf boxes by k_instance_records, every tree (scene level and groups) refitted by k_refit (csrc/kernels_geometry.hip over
csrc/geometry_records.h), the group boxes, the scene box and the bounding spheres by the commit's own pieces on the host.

The rule under test is that of tests/test_gpu_live_edit.py, whose helpers are used as they are, with the comparison scheme of tests/test_gpu_instance_edit.py: every
case commits A, creates the Render, traces 20 000 random (px, py, sample) triples (the four corners forced), calls update_geometry and requires
  * the samples to equal a fresh mi.Scene(B)'s bit for bit;
  * the mi_intersection records of 4000 camera rays to equal the fresh scene's byte for byte;
  * revision() to go from (r, 1) to (r + 1, 1) -- one step, no tree build;
  * the device tables nodes, leaf_records, tri_shade, instances, scene_box to equal those of a clone() of the edited scene (which uploads the host-refreshed mirrors:
    device arithmetic = host arithmetic);
  * instances (every word but 27, `root`), tri_shade, leaf_records and scene_box to equal the fresh scene's.  leaf_records are compared per primitive, as
    tests/test_gpu_geometry_edit.py compares them: a fresh commit builds its trees for the NEW vertices and may order the leaf records differently -- that order and
    `root` are what a commit legitimately numbers differently;
  * the oracle on B to agree under check(..., "share") on the first 4000 triples.
Every scene is the garden at 48 x 32, 4 spp.  The bounds on the share of triples an edit must change are half or less of what the oracle alone gives for A against B
(4000 triples, seed 11; quoted with each case), so a no-op cannot pass."""
import ctypes as C
import importlib
import numpy as np
import pytest
from tests.test_gpu_live_edit import bits, triples, clone, check, with_camera, N

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT_WORD = 27      # InstanceD: to_world 12 words, to_object 12, glo 3, root, ghi 3, group
GLO_GHI = [24, 25, 26, 28, 29, 30]
TABLES = ("nodes", "leaf_records", "tri_shade", "instances", "scene_box")


def garden(S, n_side=4, seed=0, bush_levels=2):
    return S.instanced_garden(48, 32, 4, n_side=n_side, seed=seed, bush_levels=bush_levels)


def described(sc, pos=None, nrm=None, instances=None):
    """the description with other vertices / normals / instance records; everything else shared"""
    out = clone(sc)
    if pos is not None: out["pos"] = np.ascontiguousarray(pos, f32)
    if nrm is not None: out["nrm"] = np.ascontiguousarray(nrm, f32)
    if instances is not None: out["instances"] = list(instances)
    return out


def group_verts(sc, group):
    """vertex indices of the member shapes of shape group `group` (1-based, as mi_shape::group)"""
    return np.concatenate([np.arange(s["first_vert"], s["first_vert"] + s["vert_count"]) for s in sc.shapes if s.get("group", 0) == group])


def deformed(sc):
    """the standard deformation: bush (group 1) vertices scaled by (1.3, 1.5, 1.2), its normals divided by the same factors and renormalised, crate (group 2) vertices
    scaled by (1, 1.8, 1)"""
    pos = np.array(sc.pos, f32, copy=True); nrm = np.array(sc.nrm, f32, copy=True); k = np.asarray((1.3, 1.5, 1.2), f32)
    bush = group_verts(sc, 1); crate = group_verts(sc, 2)
    pos[bush] = pos[bush] * k; n = nrm[bush] / k; nrm[bush] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(f32)
    pos[crate] = pos[crate] * np.asarray((1.0, 1.8, 1.0), f32)
    return described(sc, pos, nrm)


def leaf_by_prim(tab):
    """leaf records sorted by (instance record or not, primitive): word 0 = k (5 = the record of an instance, whose primitive index counts instances), word 10 =
    primitive index; the never-hit record of unused 4-wide slots carries primitive 0xFFFFFFFF and is left out"""
    real = tab[tab[:, 10] != 0xFFFFFFFF]
    return real[np.lexsort((real[:, 10], real[:, 0] == 5))]


def same(a, b, what):
    assert a.shape == b.shape and (a == b).all(), (what, int((a != b).any(1).sum()) if a.shape == b.shape else (a.shape, b.shape))


def compare_tables(gs, fresh):
    twin = gs.clone()
    for what in TABLES: same(gs.read_geometry(what), twin.read_geometry(what), what + " (clone)")
    twin.close()
    a = gs.read_geometry("instances").copy(); b = fresh.read_geometry("instances").copy(); a[:, ROOT_WORD] = 0; b[:, ROOT_WORD] = 0; same(a, b, "instances")
    same(gs.read_geometry("tri_shade"), fresh.read_geometry("tri_shade"), "tri_shade")
    same(leaf_by_prim(gs.read_geometry("leaf_records")), leaf_by_prim(fresh.read_geometry("leaf_records")), "leaf_records")
    same(gs.read_geometry("scene_box"), fresh.read_geometry("scene_box"), "scene_box")


def same_intersections(gs, fresh_scene, sc, tag, n=4000, instances=True):
    rays = gs.camera_rays(np.random.default_rng(5).random((n, 2)).astype(f32) * np.asarray((sc.width, sc.height), f32))
    recs = gs.ray_intersect(rays); hit = recs["valid"] != 0; assert hit.mean() > 0.05, tag
    if instances: assert (recs["instance"][hit] >= 0).any(), tag
    assert recs.tobytes() == fresh_scene.ray_intersect(rays).tobytes(), tag


def edit_and_compare(mi, oracle, A, B, tag, min_changed, verts=True, inst=False, how="share", gs=None, r=None, n_oracle=4000, builds=1, instances_visible=True):
    """commit A, create the render, one update_geometry to B (the parts named by verts / inst), compare with a fresh scene of B and (how) with the oracle on B;
    returns (scene, render, samples before, samples after)"""
    if gs is None:
        gs = mi.Scene(clone(A)); r = mi.Render(gs)
    pairs = triples(B); before = r.samples(pairs)
    rev0, nb = gs.revision(); assert nb == builds
    gs.update_geometry(B.pos if verts else None, B.nrm if verts else None, B.instances if inst else None)
    assert gs.revision() == (rev0 + 1, builds)
    got = r.samples(pairs)
    fresh_scene = mi.Scene(clone(B)); fresh = mi.Render(fresh_scene).samples(pairs)
    assert (bits(got) == bits(fresh)).all(), (tag, int((bits(got) != bits(fresh)).any(1).sum()))
    changed = float((bits(got) != bits(before)).any(1).mean()); print(f"[group-edit] {tag}: {changed:.3f} of the triples changed")
    if min_changed is not None: assert changed > min_changed, (tag, changed)
    if how: check(got[:n_oracle], oracle.Oracle(B).render_samples(pairs[:n_oracle])["li"], how, tag)
    same_intersections(gs, fresh_scene, B, tag, instances=instances_visible)
    assert gs.revision() == (rev0 + 1, builds) and fresh_scene.revision() == (0, 1)
    compare_tables(gs, fresh_scene)
    fresh_scene.close()
    return gs, r, before, got


# ---------------------------------------------------------------------------------------------- 1. / 2. the standard deformation, both node kinds, both bush sizes
@pytest.mark.parametrize("bvh2", ["1", "0"])
@pytest.mark.parametrize("bush_levels", [2, 4])
def test_group_members_deform(mi, oracle, monkeypatch, bvh2, bush_levels):
    """bush and crate deform inside their groups: group boxes, instance boxes, both trees follow (the oracle alone: 0.44 of the triples change with the 128-triangle
    bush, 0.46 with the 2048-triangle one, where a level of the group tree spans several 256-thread workgroups); then, from A again, the deformation and the seed-1
    placements in the same call (0.52).  Binary and 4-wide nodes, scene level and groups alike."""
    monkeypatch.setenv("MI355PT_BVH2", bvh2)
    S = mi.scenes; A = garden(S, bush_levels=bush_levels); B = deformed(A)
    assert len(A.idx) == (142 if bush_levels == 2 else 2062) and not (A.pos == B.pos).all() and not (A.nrm == B.nrm).all()
    gs, r, _, _ = edit_and_compare(mi, oracle, A, B, f"deformation bvh2={bvh2} levels={bush_levels}", 0.2)
    nodes = gs.read_geometry("nodes"); assert len(nodes) > (16 if bush_levels == 2 else 1000 if bvh2 == "1" else 500)      # 4 levels: 1152 binary / 564 wide nodes, the lowest refit level holds 515 / 378 of them
    glo = gs.read_geometry("instances")[:, GLO_GHI]; r.close(); gs.close()      # the render before its scene
    if bush_levels == 2:
        D = described(B, instances=garden(S, seed=1).instances)
        gs, r, _, _ = edit_and_compare(mi, oracle, A, D, f"deformation + placements bvh2={bvh2}", 0.25, inst=True)
        assert (gs.read_geometry("instances")[:, GLO_GHI] == glo).all()      # the same group boxes under other transforms


# ---------------------------------------------------------------------------------------------- 3. 81 instances, lanes at the wave's edges
def outwards(S, sc, which):
    """the instances at the indices `which` moved far outwards, one per face of the scene box in the order -x, +x, -z, +z (as in the instance-edit test)"""
    faces = [(0, -40.0), (0, 40.0), (2, -40.0), (2, 40.0)]; out = list(sc.instances)
    for i, (axis, where) in zip(which, faces):
        tw = np.asarray(out[i]["to_world"], np.float64).copy(); tw[axis, 3] = where
        out[i] = S.make_instance(out[i]["group"], tw)
    return described(sc, instances=out)


def test_81_instances_and_the_lanes_at_the_edges_of_a_wave(mi, oracle):
    """n_side = 9 (the oracle alone: 0.58 of the triples change): the deformation, and in the same call the instances 0, 63, 64 and 80 pushed outwards, each along an
    axis of its own: every side face of the scene box is defined by a first or last lane of a wave"""
    S = mi.scenes; A = garden(S, 9); assert len(A.instances) == 81
    B = outwards(S, deformed(A), [0, 63, 64, 80])
    gs, r, _, _ = edit_and_compare(mi, oracle, A, B, "n_side=9, lanes 0 63 64 80", 0.25, inst=True)
    box = gs.read_geometry("scene_box").view(f32)[0]
    assert box[0] < -35 and box[3] > 35 and box[2] < -35 and box[5] > 35 and gs.revision() == (1, 1)


# ---------------------------------------------------------------------------------------------- 4. the group box grows and comes back
def test_group_box_grows_and_comes_back(mi, oracle):
    """the highest bush vertex (index 10) goes to (0, 6, 0) (the oracle alone: 0.14 of the triples change): glo / ghi of every bush instance and the scene box change;
    the edit back restores the first samples, scene_box, instances and nodes bit for bit -- a refit that only grew boxes would fail here"""
    S = mi.scenes; A = garden(S); assert 10 in group_verts(A, 1) and A.pos[10, 1] == A.pos[group_verts(A, 1), 1].max()
    pos = np.array(A.pos, f32, copy=True); pos[10] = (0.0, 6.0, 0.0); B = described(A, pos, A.nrm)
    gs = mi.Scene(clone(A)); r = mi.Render(gs); box0 = gs.read_geometry("scene_box"); nodes0 = gs.read_geometry("nodes"); inst0 = gs.read_geometry("instances")
    gs, r, first, _ = edit_and_compare(mi, oracle, A, B, "bush tip up", 0.05, gs=gs, r=r)
    inst1 = gs.read_geometry("instances"); bush = np.asarray([i["group"] == 0 for i in A.instances])
    assert (inst1[bush][:, GLO_GHI] != inst0[bush][:, GLO_GHI]).any(1).all() and (inst1[~bush] == inst0[~bush]).all()
    assert (gs.read_geometry("scene_box") != box0).any() and gs.read_geometry("scene_box").view(f32)[0][4] > box0.view(f32)[0][4]
    gs, r, _, last = edit_and_compare(mi, oracle, B, A, "bush tip back", 0.05, how=None, gs=gs, r=r)
    assert (bits(last) == bits(first)).all() and (gs.read_geometry("scene_box") == box0).all() and (gs.read_geometry("instances") == inst0).all() and (gs.read_geometry("nodes") == nodes0).all()
    assert gs.revision() == (2, 1)


# ---------------------------------------------------------------------------------------------- 5. a scene-level vertex of an instanced scene
def test_scene_level_vertex_of_an_instanced_scene(mi, oracle):
    """only vertex 0 (a floor corner) moves, to y = 2 (the oracle alone: 0.61 of the triples change): the instance records stay, the two floor triangles' records change"""
    S = mi.scenes; A = garden(S); assert A.shapes[0].get("group", 0) == 0 and (A.idx[:2] == 0).any(1).all() and not (A.idx[2:] == 0).any()
    pos = np.array(A.pos, f32, copy=True); pos[0, 1] = 2.0; B = described(A, pos, A.nrm)
    gs = mi.Scene(clone(A)); r = mi.Render(gs); inst0 = gs.read_geometry("instances"); shade0 = gs.read_geometry("tri_shade")
    gs, r, _, _ = edit_and_compare(mi, oracle, A, B, "floor corner up", 0.25, gs=gs, r=r)
    shade1 = gs.read_geometry("tri_shade")
    assert (gs.read_geometry("instances") == inst0).all() and (shade1[:2] != shade0[:2]).any(1).all() and (shade1[2:] == shade0[2:]).all()


# ---------------------------------------------------------------------------------------------- 6. sequences on one handle
def recommit(gs, sc):
    """mi_scene_set_triangles + mi_scene_set_instances + mi_scene_commit on the SAME handle with the vertices and placements of `sc` (a render handle does not survive this)"""
    L = gs.L; M = importlib.import_module(type(gs).__module__); shapes = (M.MiShape * len(sc.shapes))()
    for i, s in enumerate(sc.shapes):
        shapes[i] = M.MiShape(s["first_tri"], s["tri_count"], s["first_vert"], s["vert_count"], s["bsdf"], s["emitter"], (s["face_normals"] & 1) | ((s.get("has_uv", 0) & 1) << 1), s.get("group", 0))
    p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data
    pos = np.ascontiguousarray(sc.pos, f32); nrm = np.ascontiguousarray(sc.nrm, f32); insts = list(sc.instances)
    L.check(L.L.mi_scene_set_triangles(gs.h, p(pos), p(nrm), p(sc.uv), p(sc.idx), len(pos), len(sc.idx), C.cast(shapes, C.c_void_p), len(sc.shapes)))
    L.check(L.L.mi_scene_set_instances(gs.h, C.cast(M.pack_instances(insts), C.c_void_p), len(insts)))
    L.check(L.L.mi_scene_commit(gs.h, 0)); gs.sc.pos = pos; gs.sc.nrm = nrm; gs.sc.instances = insts


def test_sequence_on_one_handle(mi, oracle):
    """update_instances -> update_geometry(pos, nrm) -> camera -> materials (the wood turns black: a flag flip inside a group) -> update_geometry(instances) ->
    update_geometry back to A: each step equals a fresh scene, the last -- materials and camera restored -- the very first render; one tree build throughout; a
    clone() taken mid-sequence, while every host mirror is stale, renders the same bits.  Then a recommit on the same handle and another edit: the edit state of the
    old trees is gone."""
    S = mi.scenes; A = garden(S); other = garden(S, seed=1).instances; V = deformed(A); pairs = triples(A)
    gs = mi.Scene(clone(A)); r = mi.Render(gs); first = r.samples(pairs)
    state = {"rev": 0}

    def same_as_fresh(desc, tag):
        state["rev"] += 1; assert gs.revision() == (state["rev"], 1), tag
        fresh_scene = mi.Scene(clone(desc)); got = r.samples(pairs); fresh = mi.Render(fresh_scene).samples(pairs)
        assert (bits(got) == bits(fresh)).all(), tag
        same_intersections(gs, fresh_scene, desc, tag); compare_tables(gs, fresh_scene); fresh_scene.close()
        return got
    gs.update_instances(other); D1 = described(A, instances=other); same_as_fresh(D1, "instances (older call)")
    gs.update_geometry(V.pos, V.nrm); D2 = described(D1, V.pos, V.nrm); got = same_as_fresh(D2, "vertices")
    twin = gs.clone(); assert (bits(mi.Render(twin).samples(pairs)) == bits(got)).all(); twin.close()
    gs.update_instances(A.instances); gs.update_geometry(instances=other); state["rev"] += 2      # there and back through both calls, no refresh between
    twin = gs.clone(); assert (bits(mi.Render(twin).samples(pairs)) == bits(got)).all(); twin.close()
    D3 = with_camera(S, D2, (6.0, 3.0, -7.0), (0.0, 0.6, 0.5), 48.0); gs.update_camera(D3.sample_to_camera, D3.cam_to_world, D3.near, D3.far); same_as_fresh(D3, "camera")
    D4 = clone(D3); D4.bsdfs[2]["reflectance"] = (0.0, 0.0, 0.0); gs.update_materials(D4.bsdfs); same_as_fresh(D4, "materials")
    gs.update_geometry(instances=A.instances); D5 = described(D4, instances=A.instances); same_as_fresh(D5, "instances (geometry call)")
    gs.update_geometry(A.pos, A.nrm); same_as_fresh(described(D5, A.pos, A.nrm), "vertices back")
    gs.update_materials(A.bsdfs); gs.update_camera(A.sample_to_camera, A.cam_to_world, A.near, A.far)
    assert (bits(r.samples(pairs)) == bits(first)).all() and gs.revision() == (10, 1)
    r.close()
    gs.update_geometry(V.pos, V.nrm, other)                      # leaves edit state (stale host mirrors included) behind for the commit to drop
    B = described(V, instances=other); recommit(gs, B); assert gs.revision() == (11, 2)
    fresh = mi.Scene(clone(B))
    for what in TABLES: same(gs.read_geometry(what), fresh.read_geometry(what), what + " (recommit)")
    fresh.close()
    edit_and_compare(mi, oracle, B, A, "after the recommit", 0.25, inst=True, how=None, gs=gs, r=mi.Render(gs), builds=2)


def test_geometry_call_first_then_the_older_call(mi, oracle):
    """a fresh handle's first edit is update_geometry(pos, nrm), its second update_instances, with no read of the scene in between: the older call finds the tables of
    the first edit (the device's leaf boxes, newer than their host mirror, among them) and adds its own; tables, intersections and samples equal a fresh scene's"""
    S = mi.scenes; A = garden(S); other = garden(S, seed=1).instances; V = deformed(A); pairs = triples(A)
    gs = mi.Scene(clone(A)); r = mi.Render(gs)
    gs.update_geometry(V.pos, V.nrm); gs.update_instances(other)
    assert gs.revision() == (2, 1)
    D = described(V, instances=other); fresh_scene = mi.Scene(clone(D)); got = r.samples(pairs); fresh = mi.Render(fresh_scene).samples(pairs)
    assert (bits(got) == bits(fresh)).all(), int((bits(got) != bits(fresh)).any(1).sum())
    same_intersections(gs, fresh_scene, D, "geometry call, then the older call"); compare_tables(gs, fresh_scene)
    assert gs.revision() == (2, 1)


def test_edit_a_clone_taken_mid_sequence(mi, oracle):
    """two edits on gs (vertices, then instances), a clone() of it, and update_geometry back to A on the clone: the clone's first edit finds the edit state prepared and
    no device edit table; its tables and samples equal a fresh scene of A, its revision advances by one, and gs renders what it rendered before"""
    S = mi.scenes; A = garden(S); other = garden(S, seed=1).instances; V = deformed(A); pairs = triples(A)
    gs = mi.Scene(clone(A)); r = mi.Render(gs)
    gs.update_geometry(V.pos, V.nrm); gs.update_instances(other); kept = r.samples(pairs)
    twin = gs.clone(); twin.sc = clone(gs.sc); rev0 = twin.revision()      # a description of its own: Scene.clone() shares the source's
    twin.update_geometry(A.pos, A.nrm, A.instances)
    assert twin.revision() == (rev0[0] + 1, rev0[1]) and gs.revision() == (2, 1)
    fresh_scene = mi.Scene(clone(A)); got = mi.Render(twin).samples(pairs); fresh = mi.Render(fresh_scene).samples(pairs)
    assert (bits(got) == bits(fresh)).all(), int((bits(got) != bits(fresh)).any(1).sum())
    same_intersections(twin, fresh_scene, A, "edited clone"); compare_tables(twin, fresh_scene)
    assert (bits(got) != bits(kept)).any(1).mean() > 0.25      # as "after the recommit" above: the same two descriptions
    D = described(V, instances=other); fresh_d = mi.Scene(clone(D))
    assert (bits(r.samples(pairs)) == bits(kept)).all() and (bits(kept) == bits(mi.Render(fresh_d).samples(pairs))).all()
    compare_tables(gs, fresh_d)


# ---------------------------------------------------------------------------------------------- 7. a scene without instances
def test_scene_without_instances(mi, oracle):
    """cornell_box (32 triangles, the packet path): update_geometry(pos) leaves the device tables and the samples update_vertices(pos) leaves on a second handle;
    update_geometry(instances=...) is refused there with code 1"""
    S = mi.scenes; A = S.cornell_box(48, 32, 4); pos = np.array(A.pos, f32, copy=True)
    s = A.shapes[-1]; v = slice(s["first_vert"], s["first_vert"] + s["vert_count"]); c = pos[v].mean(0); pos[v] = ((pos[v] - c) * np.asarray((1.2, 0.7, 1.1), f32) + c + np.asarray((15.0, 0.0, -20.0), f32)).astype(f32)
    B = described(A, pos, A.nrm); pairs = triples(A)
    g1 = mi.Scene(clone(A)); r1 = mi.Render(g1); g2 = mi.Scene(clone(A)); r2 = mi.Render(g2); before = r1.samples(pairs)
    g1.update_geometry(B.pos, B.nrm); g2.update_vertices(B.pos, B.nrm)
    assert g1.revision() == (1, 1) and g2.revision() == (1, 1)
    for what in ("nodes", "leaf_records", "tri_shade", "tri_uv", "packet_exact", "packet_groups", "scene_box"): same(g1.read_geometry(what), g2.read_geometry(what), what)
    got = r1.samples(pairs); assert (bits(got) == bits(r2.samples(pairs))).all() and (bits(got) != bits(before)).any(1).mean() > 0.05
    fresh = mi.Scene(clone(B)); assert (bits(got) == bits(mi.Render(fresh).samples(pairs))).all()
    for what in ("tri_shade", "packet_exact", "packet_groups", "scene_box"): same(g1.read_geometry(what), fresh.read_geometry(what), what + " (fresh)")
    g1.update_vertices(A.pos, A.nrm); g2.update_geometry(A.pos, A.nrm)      # back through the other call each
    for what in ("nodes", "leaf_records", "tri_shade", "packet_exact", "packet_groups", "scene_box"): same(g1.read_geometry(what), g2.read_geometry(what), what + " (back)")
    assert (bits(r1.samples(pairs)) == bits(before)).all() and (bits(r2.samples(pairs)) == bits(before)).all()
    with pytest.raises(mi.MiError) as e:
        g1.update_geometry(instances=garden(S).instances)
    assert e.value.code == 1 and "mi_scene_update_geometry: " in str(e.value) and "the scene has no instances" in str(e.value) and g1.revision() == (2, 1)


# ---------------------------------------------------------------------------------------------- 8. fields, film rule
def test_fields_follow_the_edit_and_the_film_is_never_mixed(mi, oracle):
    """position and shapeIndex fields: after the edit a run without clear() is refused (the film holds samples of the earlier geometry); after clear() and a run the
    field film and the radiance film equal a fresh scene's bit for bit"""
    S = mi.scenes; A = garden(S); B = deformed(A); F = [("position", (-1.0, 2.5, 7.0)), ("shapeIndex", -7.0)]
    gs = mi.Scene(clone(A)); r = mi.Render(gs, fields=F); r.run(s1=2); old = r.read_fields(2)
    gs.update_geometry(B.pos, B.nrm); assert gs.revision() == (1, 1)
    with pytest.raises(mi.MiError) as e:
        r.run()
    assert e.value.code == 1 and "mi_render_clear" in str(e.value)
    r.clear(); r.run(s1=2)
    fresh_scene = mi.Scene(clone(B)); fr = mi.Render(fresh_scene, fields=F); fr.run(s1=2)
    got = r.read_fields(2); ref = fr.read_fields(2)
    assert (bits(got) == bits(ref)).all() and (bits(r.read_film(0)) == bits(fr.read_film(0))).all()
    assert (bits(got) != bits(old)).any(2).mean() > 0.05
    p = triples(B, 4000); assert (bits(r.field_samples(p)) == bits(fr.field_samples(p))).all()


# ---------------------------------------------------------------------------------------------- 9. host mirror
def _host_render(mi, gs, sc, devices):
    h = mi.api.HostIntegrator(gs, devices=devices, planes_per_batch=4)
    target = np.zeros((sc.height + 2, sc.width + 2, 4), f32)
    assert h.render("responsive", target) == 0
    return h, target


def test_host_mirror_set_geometry_on_replicas(mi):
    """MIPathTracerHIP::setGeometry between two render() calls: with devices = (0, 0) both replicas are edited -- the second target equals that of one device and that
    of a host integrator on a fresh scene of B, bit for bit"""
    S = mi.scenes; A = garden(S); B = described(deformed(A), instances=garden(S, seed=1).instances); targets = {}
    for devices in ((0,), (0, 0)):
        gs = mi.Scene(clone(A)); h, first = _host_render(mi, gs, A, devices)
        h.set_geometry(B.pos, B.nrm, B.instances)
        t = np.zeros_like(first); assert h.render("responsive", t) == 0
        assert gs.revision() == (1, 1) and (bits(t) != bits(first)).any(2).mean() > 0.05
        fresh_scene = mi.Scene(clone(B)); same_intersections(gs, fresh_scene, B, f"replicas {devices}")
        fh, fresh = _host_render(mi, fresh_scene, B, devices)
        assert (bits(t) == bits(fresh)).all(), devices
        targets[devices] = t; h.close(); fh.close()
    assert (bits(targets[(0, 0)]) == bits(targets[(0,)])).all()


# ---------------------------------------------------------------------------------------------- 10. refusals
def test_refusals_on_a_committed_scene(mi):
    """a wrong vertex count, normals missing, a NaN position, a wrong instance count, a changed group (code 3), a NaN in to_object, both parts None: each with its code
    and a message that names the function (and the vertex / instance); revision(), the description and the samples stay"""
    S = mi.scenes; A = garden(S); gs = mi.Scene(clone(A)); r = mi.Render(gs); pairs = triples(A, 4000); before = r.samples(pairs); tables = {w: gs.read_geometry(w) for w in TABLES}
    pos0, inst0 = gs.sc.pos, gs.sc.instances

    def refused(code, *words, **kw):
        with pytest.raises(mi.MiError) as e:
            gs.update_geometry(**kw)
        assert e.value.code == code and "mi_scene_update_geometry: " in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
        assert gs.revision() == (0, 1) and gs.sc.pos is pos0 and gs.sc.instances is inst0
    nv = len(A.pos)
    refused(1, f"{nv} -> {nv - 1}", pos=A.pos[:-1], nrm=A.nrm[:-1])
    refused(1, "normals are required", pos=A.pos)
    nan = np.array(A.pos, f32, copy=True); nan[37, 1] = np.nan; refused(1, "vertex 37", pos=nan, nrm=A.nrm, instances=A.instances)
    refused(1, "16 -> 15", instances=A.instances[:-1])
    other = [dict(x) for x in A.instances]; other[5]["group"] = 1 - other[5]["group"]; refused(3, "instance 5", "group", pos=A.pos, nrm=A.nrm, instances=other)
    bad = [dict(x) for x in A.instances]; bad[9]["to_object"] = bad[9]["to_object"].copy(); bad[9]["to_object"][1, 2] = np.nan; refused(1, "instance 9", "to_object", instances=bad)
    refused(1, "null argument")
    assert (bits(r.samples(pairs)) == bits(before)).all()
    for w in TABLES: same(gs.read_geometry(w), tables[w], w)
    with pytest.raises(mi.MiError) as e:      # the older call keeps its refusal of instanced scenes
        gs.update_vertices(A.pos, A.nrm)
    assert e.value.code == 3 and "mi_scene_update_vertices: " in str(e.value) and gs.revision() == (0, 1)
