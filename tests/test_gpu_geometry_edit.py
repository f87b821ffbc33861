"""GPU (MI355X): vertex edits of a committed scene (mi_scene_update_vertices; Scene.update_vertices of mitsuba-im_amd/api.py): per-triangle records by k_tri_records,
the existing tree refitted by k_refit (csrc/kernels_geometry.hip over csrc/geometry_records.h), the small tables by the commit's own pieces on the host.

The rule under test is that of tests/test_gpu_live_edit.py, whose helpers and criteria are used as they are: after an update every result equals what a fresh commit of
the new vertices gives.  Every case commits A, creates the Render, traces 20 000 random (px, py, sample) triples (the four corners forced), updates to B and compares
  * with a fresh mi.Scene(B): bit for bit, always;
  * with the oracle on B under the criterion of that scene family's parity test ("bits", "vol", "env" of test_gpu_live_edit.check);
and asserts that more than 5 % of the triples changed, that revision() went from (r, 1) to (r + 1, 1) -- no tree build -- and that the mi_intersection records of the new
camera rays equal the fresh scene's byte for byte.  The device tables themselves (Scene.read_geometry) are compared too: with a clone of the edited scene, which uploads
the host-refreshed tables (device arithmetic = host arithmetic, every record and every quantised node), and with the fresh scene per primitive."""
import os
import subprocess
import sys
import numpy as np
import pytest
from tests.conftest import ROOT
from tests.test_gpu_live_edit import bits, triples, clone, check, N

pytestmark = pytest.mark.gpu
f32 = np.float32


def moved(sc, pos, nrm=None):
    """the description with other vertex positions (and normals); everything else shared"""
    out = clone(sc); out["pos"] = np.ascontiguousarray(pos, f32)
    if nrm is not None: out["nrm"] = np.ascontiguousarray(nrm, f32)
    return out


def shape_verts(sc, shape):
    s = sc.shapes[shape]; return slice(s["first_vert"], s["first_vert"] + s["vert_count"])


def rotate_y(p, centre, degrees):
    a = np.deg2rad(degrees); c, s = np.cos(a), np.sin(a); q = np.asarray(p, np.float64) - centre
    return np.stack([c * q[:, 0] + s * q[:, 2], q[:, 1], -s * q[:, 0] + c * q[:, 2]], 1) + centre


def leaf_by_prim(tab):
    """leaf records (word 10 = primitive index; the never-hit record of unused 4-wide slots carries 0xFFFFFFFF) sorted by primitive"""
    real = tab[tab[:, 10] != 0xFFFFFFFF]; return real[np.argsort(real[:, 10], kind="stable")]


def compare_tables(gs, fresh, packet=False):
    """device tables after the edit: equal to the clone's (which come from the host mirror) byte for byte, nodes included; equal to the fresh scene's per primitive (the two trees differ by design: the fresh one is built for the new vertices)"""
    twin = gs.clone()
    for what in ("nodes", "leaf_records", "tri_shade", "tri_uv", "packet_exact", "packet_groups"):
        a = gs.read_geometry(what); b = twin.read_geometry(what)
        assert a.shape == b.shape and (a == b).all(), (what, int((a != b).any(1).sum()) if a.shape == b.shape else (a.shape, b.shape))
    for what in ("tri_shade", "tri_uv", "packet_exact") + (("packet_groups",) if packet else ()):
        a = gs.read_geometry(what); b = fresh.read_geometry(what)
        assert a.shape == b.shape and (a == b).all(), (what, int((a != b).any(1).sum()) if a.shape == b.shape else (a.shape, b.shape))
    a = leaf_by_prim(gs.read_geometry("leaf_records")); b = leaf_by_prim(fresh.read_geometry("leaf_records"))
    assert a.shape == b.shape and (a == b).all()
    twin.close()


def same_intersections(gs, fresh_scene, sc, tag, n=4000):
    """Scene::rayIntersect records of the scene's camera rays through n random film positions: byte for byte those of the fresh scene"""
    rays = gs.camera_rays(np.random.default_rng(5).random((n, 2)).astype(f32) * np.asarray((sc.width, sc.height), f32))
    recs = gs.ray_intersect(rays); assert (recs["valid"] != 0).mean() > 0.05, tag
    assert recs.tobytes() == fresh_scene.ray_intersect(rays).tobytes(), tag


def recommit(gs, sc):
    """mi_scene_set_triangles + mi_scene_commit on the SAME handle with the vertices of `sc` (a render handle does not survive this)"""
    import ctypes as C
    L = gs.L; M = sys.modules[type(gs).__module__]; shapes = (M.MiShape * len(sc.shapes))()
    for i, s in enumerate(sc.shapes):
        shapes[i] = M.MiShape(s["first_tri"], s["tri_count"], s["first_vert"], s["vert_count"], s["bsdf"], s["emitter"], (s["face_normals"] & 1) | ((s.get("has_uv", 0) & 1) << 1), s.get("group", 0))
    p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data
    pos = np.ascontiguousarray(sc.pos, f32); nrm = None if sc.nrm is None else np.ascontiguousarray(sc.nrm, f32)
    L.check(L.L.mi_scene_set_triangles(gs.h, p(pos), p(nrm), p(sc.uv), p(sc.idx), len(pos), len(sc.idx), C.cast(shapes, C.c_void_p), len(sc.shapes)))
    L.check(L.L.mi_scene_commit(gs.h, 0)); gs.sc.pos = pos
    if nrm is not None: gs.sc.nrm = nrm


def edit_and_compare(mi, oracle, A, B, how, tag, gs=None, r=None, n_oracle=N, tables=True, packet=False, builds=1):
    """commit A, create the render, move the vertices to B's, compare with the oracle on B and with a fresh scene of B; returns (scene, render, fresh scene, samples)"""
    if gs is None:
        gs = mi.Scene(clone(A)); r = mi.Render(gs)
    pairs = triples(B); orc = oracle.Oracle(B)
    before = r.samples(pairs)
    rev0, nb = gs.revision(); assert nb == builds
    gs.update_vertices(B.pos, B.nrm)
    assert gs.revision() == (rev0 + 1, builds)
    got = r.samples(pairs); check(got[:n_oracle], orc.render_samples(pairs[:n_oracle])["li"], how, tag)
    fresh_scene = mi.Scene(clone(B)); fresh = mi.Render(fresh_scene).samples(pairs)
    assert (bits(got) == bits(fresh)).all(), (tag, int((bits(got) != bits(fresh)).any(1).sum()))
    changed = float((bits(got) != bits(before)).any(1).mean()); print(f"[geometry-edit] {tag}: {changed:.3f} of the triples changed")
    assert changed > 0.05, tag
    rays = gs.camera_rays(orc.render_samples(pairs[:4000])["pos"])
    assert gs.ray_intersect(rays).tobytes() == fresh_scene.ray_intersect(rays).tobytes(), tag
    assert gs.revision() == (rev0 + 1, builds) and fresh_scene.revision() == (0, 1)
    if tables: compare_tables(gs, fresh_scene, packet)
    return gs, r, fresh_scene, got


# ---------------------------------------------------------------------------------------------- 1. packet scene
def cornell_edit(A):
    """the short box turned by 35 degrees about its axis and moved, the upper corner of one of its rectangular sides lifted (that side's two triangles stop being a
    parallelogram pair: the pass-1 table grows by one record), the light shrunk to 60 % about its centre"""
    pos = A.pos.astype(np.float64).copy()
    box = shape_verts(A, 6); c = pos[box].mean(0); pos[box] = rotate_y(pos[box], c, 35.0) + (70.0, 0.0, -25.0); pos[box.start + 5, 1] += 40.0
    lamp = shape_verts(A, 5); c = pos[lamp].mean(0); pos[lamp] = c + 0.6 * (pos[lamp] - c)
    return moved(A, pos)


def test_packet_scene(mi, oracle):
    S = mi.scenes; A = S.cornell_box(96, 64, 4); B = cornell_edit(A)
    assert len(A.idx) == 32 and A.shapes[5]["emitter"] == 0 and A.shapes[6]["tri_count"] == 10
    gs, r, fresh, _ = edit_and_compare(mi, oracle, A, B, "bits", "cornell", packet=True)
    committed = mi.Scene(clone(A)); groups_before = len(committed.read_geometry("packet_groups")); committed.close()
    assert len(gs.read_geometry("packet_groups")) == groups_before + 1      # one pair dissolved into two single triangles


# ---------------------------------------------------------------------------------------------- 2. tree, both node kinds, both walks
SHEET_B = dict(phase=1.3, amp=0.3, lift=2.5, light_size=0.2, light_x=0.5)


def sheet_case(mi, oracle, tag):
    S = mi.scenes; A = S.wavy_sheet(32); B = S.wavy_sheet(32, **SHEET_B)
    assert len(A.idx) == 2048 + 4 and (A.idx == B.idx).all() and (A.uv == B.uv).all() and A.bsdfs[0].get("texture") == 0
    assert B.pos[:1089, 1].min() > A.pos[:1089, 1].max() + 1.0                                                              # lifted clear of the old sheet: a stale box would show
    gs, r, fresh, _ = edit_and_compare(mi, oracle, A, B, "bits", tag)
    nodes = gs.read_geometry("nodes"); assert len(nodes) > 64                                                           # several levels of either node kind
    return gs


@pytest.mark.parametrize("bvh2", ["1", "0"])
def test_tree_sheet(mi, oracle, monkeypatch, bvh2):
    """the wavy sheet (n = 32) walked as a tree: binary nodes with the while-while kernels, 4-wide nodes with the fused walk"""
    monkeypatch.setenv("MI355PT_NO_PACKET", "1"); monkeypatch.setenv("MI355PT_BVH2", bvh2)
    sheet_case(mi, oracle, f"sheet bvh2={bvh2}")


def _sheet_case_main():
    """body of test_tree_sheet_wide_without_fused_walk, run in a process of its own"""
    import importlib
    import oracle
    mi = importlib.import_module("mitsuba-im_amd")
    sheet_case(mi, oracle, "sheet bvh2=0 fused=0")
    print("sheet case ok")


def test_tree_sheet_wide_without_fused_walk(monkeypatch):
    """4-wide nodes with MI355PT_FUSED=0 (the while-while kernels on quantised nodes).  The library reads that switch once, when it is loaded, so this one variant runs
    in a process of its own; the environment is set with monkeypatch like the other switches."""
    monkeypatch.setenv("MI355PT_NO_PACKET", "1"); monkeypatch.setenv("MI355PT_BVH2", "0"); monkeypatch.setenv("MI355PT_FUSED", "0")
    p = subprocess.run([sys.executable, "-c", "import tests.test_gpu_geometry_edit as t; t._sheet_case_main()"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and "sheet case ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


# ---------------------------------------------------------------------------------------------- 3. default wide tree
def test_default_wide_tree(mi, oracle):
    """n = 96: 18 432 sheet triangles (>= 16 384), so a commit without switches gives 4-wide nodes in area-sorted order and the fused walk"""
    S = mi.scenes; A = S.wavy_sheet(96); B = S.wavy_sheet(96, **SHEET_B)
    assert 2 * 96 * 96 >= 16384
    gs, r, fresh, _ = edit_and_compare(mi, oracle, A, B, "bits", "sheet n=96", n_oracle=4000)
    rays = gs.camera_rays(np.random.default_rng(3).random((256, 2)).astype(f32) * (A.width, A.height))
    _, info = gs.intersect_fused(rays); assert info["wide"] == 1                                                        # this scene has the fused walk


# ---------------------------------------------------------------------------------------------- 4. a sequence on one handle
def test_sequence_on_one_handle(mi, oracle):
    """vertex edit -> material colour -> camera -> vertex edit back to A: each step equals a fresh scene, the last one (with the first material and camera restored) the
    very first samples; one tree build throughout; a run without clear() after the edit is refused"""
    from tests.test_gpu_live_edit import with_camera
    S = mi.scenes; A = S.cornell_box(96, 64, 4); B = cornell_edit(A); pairs = triples(A)
    gs = mi.Scene(clone(A)); r = mi.Render(gs); first = r.samples(pairs); r.run(s1=2)
    gs.update_vertices(B.pos)
    with pytest.raises(mi.MiError) as e:
        r.run()
    assert e.value.code == 1 and "mi_render_clear" in str(e.value)
    r.clear(); r.run(s1=2)

    state = {"rev": 1, "prev": first}

    def same_as_fresh(desc, tag, visible=True):
        fresh_scene = mi.Scene(clone(desc)); got = r.samples(pairs); fresh = mi.Render(fresh_scene).samples(pairs)
        assert (bits(got) == bits(fresh)).all(), tag
        assert gs.revision() == (state["rev"], 1), tag; state["rev"] += 1                                      # (r, 1) -> (r + 1, 1) with every step
        if visible: assert (bits(got) != bits(state["prev"])).any(1).mean() > 0.05, tag
        same_intersections(gs, fresh_scene, desc, tag); state["prev"] = got
        return got
    assert gs.revision() == (1, 1); same_as_fresh(B, "vertices")
    C2 = clone(B); C2.bsdfs[1]["reflectance"] = (0.1, 0.2, 0.7); gs.update_materials(C2.bsdfs); same_as_fresh(C2, "colour", visible=False)
    D = with_camera(S, C2, (278, 273, 100), (180, 200, 500), 62.0); gs.update_camera(D.sample_to_camera, D.cam_to_world, D.near, D.far); same_as_fresh(D, "camera")
    gs.update_vertices(A.pos); same_as_fresh(moved(D, A.pos), "vertices back")
    gs.update_materials(A.bsdfs); gs.update_camera(A.sample_to_camera, A.cam_to_world, A.near, A.far)
    last = r.samples(pairs)
    assert (bits(last) == bits(first)).all() and gs.revision() == (6, 1)
    assert (bits(last) == bits(oracle.Oracle(A).render_samples(pairs)["li"])).all()


@pytest.mark.parametrize("bvh2", ["1", "0"])
def test_edit_recommit_edit_on_one_handle(mi, oracle, monkeypatch, bvh2):
    """A commit on the same handle after an edit builds another tree (for the edited vertices): the state of the first tree's edits must not survive it.  Edit to B,
    recommit B without reading anything in between, clone (tables = a fresh scene's, nodes included), then edit back to A on the second tree: a fresh scene of A"""
    monkeypatch.setenv("MI355PT_NO_PACKET", "1"); monkeypatch.setenv("MI355PT_BVH2", bvh2)
    S = mi.scenes; A = S.wavy_sheet(32); B = S.wavy_sheet(32, **SHEET_B)
    gs = mi.Scene(clone(A)); r = mi.Render(gs); gs.update_vertices(B.pos, B.nrm); r.close()
    recommit(gs, B); assert gs.revision() == (1, 2)
    twin = gs.clone(); fresh = mi.Scene(clone(B))
    for what in ("nodes", "leaf_records", "tri_shade", "tri_uv", "packet_exact"):
        a, b, c = gs.read_geometry(what), twin.read_geometry(what), fresh.read_geometry(what)
        assert a.shape == b.shape == c.shape and (a == b).all() and (a == c).all(), what
    twin.close(); fresh.close()
    edit_and_compare(mi, oracle, B, A, "bits", f"recommit bvh2={bvh2}", gs=gs, r=mi.Render(gs), builds=2)


# ---------------------------------------------------------------------------------------------- 5. media and environment
def test_fog_box_smoke_cube_moves(mi, oracle):
    """fog_box (volpath_simple; a tree with an analytic sphere in it): the smoke cube's mesh moved and turned; ray counters of a short run equal the fresh scene's"""
    S = mi.scenes; A = S.fog_box(); pos = A.pos.astype(np.float64).copy(); cube = shape_verts(A, 6)
    assert A.shapes[6]["interior"] == 0 and len(A.analytic) == 1
    pos[cube] = rotate_y(pos[cube], pos[cube].mean(0), -25.0) + (60.0, 120.0, 40.0); B = moved(A, pos)
    gs, r, fresh, _ = edit_and_compare(mi, oracle, A, B, "vol", "fog_box")
    r.clear(); r.run(s1=2); fr = mi.Render(fresh); fr.run(s1=2); a, b = r.stats(), fr.stats()
    assert (a["rays"], a["shadow_rays"], a["path_length_sum"], a["samples"]) == (b["rays"], b["shadow_rays"], b["path_length_sum"], b["samples"])
    assert (bits(r.read_film(0)) == bits(fr.read_film(0))).all()


def test_sky_view_geometry_leaves_the_old_box(mi, oracle):
    """sky_view: the block grows to eight times its height and moves, far beyond the old scene box, so the environment emitter's bounding sphere changes"""
    S = mi.scenes; A = S.sky_view(); pos = A.pos.astype(np.float64).copy(); block = shape_verts(A, 1)
    pos[block] = pos[block] * (1.0, 8.0, 1.0) + (-0.5, 0.0, 0.7); B = moved(A, pos)
    assert pos[:, 1].max() > 2 * A.pos[:, 1].max() + 8
    edit_and_compare(mi, oracle, A, B, "env", "sky_view")


# ---------------------------------------------------------------------------------------------- 6. fields
def test_fields_follow_the_edit(mi, oracle):
    """the position and shNormal fields of the same render follow the edit: the field film after clear + run equals a fresh scene's"""
    S = mi.scenes; A = S.wavy_sheet(32); B = S.wavy_sheet(32, **SHEET_B); F = [("position", (-1.0, 2.5, 7.0)), ("shNormal", 0.0)]
    gs = mi.Scene(clone(A)); r = mi.Render(gs, fields=F); r.run(s1=2); old = r.read_fields(2)
    assert gs.revision() == (0, 1); gs.update_vertices(B.pos, B.nrm); assert gs.revision() == (1, 1)
    r.clear(); r.run(s1=2)
    fresh_scene = mi.Scene(clone(B)); fr = mi.Render(fresh_scene, fields=F); fr.run(s1=2)
    same_intersections(gs, fresh_scene, B, "fields")
    got = r.read_fields(2); ref = fr.read_fields(2)
    assert (bits(got) == bits(ref)).all() and (bits(r.read_film(0)) == bits(fr.read_film(0))).all()
    assert (bits(got) != bits(old)).any(2).mean() > 0.05
    pairs = triples(B, 4000); assert (bits(r.field_samples(pairs)) == bits(fr.field_samples(pairs))).all()


# ---------------------------------------------------------------------------------------------- 7. replicas and the refusal
def _host_render(mi, gs, sc, devices):
    h = mi.api.HostIntegrator(gs, devices=devices, planes_per_batch=4)
    target = np.zeros((sc.height + 2, sc.width + 2, 4), f32)
    assert h.render("responsive", target) == 0
    return h, target


def test_host_mirror_set_vertices_on_replicas(mi):
    """MIPathTracerHIP::setVertices between two render() calls: with devices = (0, 0) both replicas move -- the second target equals that of one device, bit for bit,
    and that of a host integrator on a fresh scene of B"""
    S = mi.scenes; A = S.cornell_box(48, 32, 4); B = cornell_edit(A); targets = {}
    for devices in ((0,), (0, 0)):
        gs = mi.Scene(clone(A)); h, first = _host_render(mi, gs, A, devices)
        h.set_vertices(B.pos)
        t = np.zeros_like(first); assert h.render("responsive", t) == 0
        assert gs.revision() == (1, 1) and (bits(t) != bits(first)).any(2).mean() > 0.05
        fresh_scene = mi.Scene(clone(B)); same_intersections(gs, fresh_scene, B, f"replicas {devices}")
        fh, fresh = _host_render(mi, fresh_scene, B, devices)
        assert (bits(t) == bits(fresh)).all(), devices
        targets[devices] = t; h.close(); fh.close()
    assert (bits(targets[(0, 0)]) == bits(targets[(0,)])).all()


def test_instances_are_refused(mi):
    """instanced_garden: MI_ERR_UNSUPPORTED (3), the message names instances, the scene renders what it rendered before"""
    S = mi.scenes; A = S.instanced_garden(48, 32, 4); gs = mi.Scene(clone(A)); r = mi.Render(gs); pairs = triples(A, 4000); before = r.samples(pairs)
    with pytest.raises(mi.MiError) as e:
        gs.update_vertices(A.pos + f32(0.25), A.nrm)
    assert e.value.code == 3 and "mi_scene_update_vertices" in str(e.value) and "instance" in str(e.value)
    assert gs.revision() == (0, 1) and (gs.sc.pos == A.pos).all()
    assert (bits(r.samples(pairs)) == bits(before)).all()
