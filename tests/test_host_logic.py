"""CPU: host-side logic -- the C-ABI library loads and exports every symbol include/mi355pt.h declares, argument validation and
error strings (no compute calls without a GPU), scene generators, tile sharding."""
import ctypes as C
import os
import re
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(mi):
    mi.build()
    hdr = open(os.path.join(ROOT, "include", "mi355pt.h")).read() + open(os.path.join(ROOT, "include", "mi355pt_host.h")).read()
    declared = set(re.findall(r"\b(mi_[a-z_0-9]+)\s*\(", hdr))
    assert len(declared) >= 25
    L = C.CDLL(mi.api.LIB_PATH)
    missing = [n for n in sorted(declared) if not hasattr(L, n)]
    assert not missing, missing
    assert declared == set(mi.api.EXPORTS) | set(mi.api.HOST_EXPORTS)


def test_argument_validation_without_gpu(mi):
    L = mi.lib(); h = C.c_void_p()
    L.check(L.L.mi_scene_create(C.byref(h)))
    sc = mi.scenes.cornell_box(16, 9, 1)
    shapes = (mi.api.MiShape * 1)(mi.api.MiShape(0, 999, 0, 4, 0, -1, 1, 0))
    rc = L.L.mi_scene_set_triangles(h, sc.pos.ctypes.data, None, None, sc.idx.ctypes.data, len(sc.pos), len(sc.idx), C.cast(shapes, C.c_void_p), 1)
    assert rc == 1 and b"shape range" in L.L.mi_last_error()
    bad_idx = sc.idx.copy(); bad_idx[0, 0] = 10 ** 6
    shapes[0].tri_count = 2
    rc = L.L.mi_scene_set_triangles(h, sc.pos.ctypes.data, None, None, bad_idx.ctypes.data, len(sc.pos), len(sc.idx), C.cast(shapes, C.c_void_p), 1)
    assert rc == 1 and b"index out of range" in L.L.mi_last_error()
    assert L.L.mi_scene_set_film(h, 0, 10, 0, 0.5, 0.5) == 1
    assert L.L.mi_scene_set_materials(h, None, 0) == 1
    mats = (mi.api.MiMaterial * 1)(mi.api.MiMaterial(99, 0, 0, 0.1))
    assert L.L.mi_scene_set_materials(h, C.cast(mats, C.c_void_p), 1) == 3          # MI_ERR_UNSUPPORTED
    assert L.L.mi_scene_commit(h, 0) == 1 and b"must be set first" in L.L.mi_last_error()
    assert L.L.mi_scene_set_envmap(h, None, 0, 0, None, 1.0) == 1 and b"mi_scene_set_envmap" in L.L.mi_last_error()
    ems = (mi.api.MiEmitter * 2)(mi.api.MiEmitter(1, -1), mi.api.MiEmitter(1, -1))
    assert L.L.mi_scene_set_emitters(h, C.cast(ems, C.c_void_p), 2) == 1 and b"only contain one environment emitter" in L.L.mi_last_error()
    L.L.mi_scene_destroy(h)
    with pytest.raises(mi.MiError):
        mi.api.Lib("/nonexistent/libmi355pt.so")


def test_round3_material_validation_without_gpu(mi):
    """mi_scene_set_materials on the adapter records added in round 3: a coating nests ONE plain reflective record and needs two different indices of refraction
    (coating.cpp:119-121); a blendbsdf blends two plain, untextured records; neither may be the child of a mixturebsdf; anisotropic `ward` passes the material
    check (the texture-coordinate requirement is a commit-time check)."""
    L = mi.lib(); h = C.c_void_p(); L.check(L.L.mi_scene_create(C.byref(h))); M = mi.api.MiMaterial
    def mat(t, flags=0, distr=0, alpha=0.1, refl=(0.5, 0.5, 0.5), eta=(0, 0, 0), k=(0, 0, 0), spec=(1, 1, 1)):
        return M(t, flags, distr, alpha, (C.c_float * 3)(*refl), (C.c_float * 3)(*eta), (C.c_float * 3)(*k), (C.c_float * 3)(*spec))
    def rc(*ms):
        arr = (M * len(ms))(*ms); return L.L.mi_scene_set_materials(h, C.cast(arr, C.c_void_p), len(ms)), L.L.mi_last_error()
    COAT, BLEND, MIX, DIEL, WARD = 17, 18, 10, 3, 16
    assert rc(mat(0), mat(COAT, distr=0, eta=(1.5, 0, 0)))[0] == 0
    r, msg = rc(mat(0), mat(COAT, distr=0, eta=(1.0, 0, 0))); assert r == 1 and b"must be positive and differ" in msg
    r, msg = rc(mat(0), mat(COAT, distr=5, eta=(1.5, 0, 0))); assert r == 3 and b"coating nests a plain BSDF" in msg
    r, msg = rc(mat(DIEL, eta=(1.5, 0, 0)), mat(COAT, distr=0, eta=(1.5, 0, 0))); assert r == 3 and b"reflective" in msg
    r, msg = rc(mat(0, flags=1), mat(COAT, distr=0, eta=(1.5, 0, 0))); assert r == 3 and b"twosided" in msg
    r, msg = rc(mat(0), mat(COAT, distr=0, eta=(1.5, 0, 0)), mat(COAT, distr=1, eta=(1.3, 0, 0))); assert r == 3          # a coating over a coating
    assert rc(mat(0), mat(0), mat(BLEND, eta=(0, 1, 0)))[0] == 0
    r, msg = rc(mat(0), mat(0, flags=1 << 8), mat(BLEND, eta=(0, 1, 0))); assert r == 3 and b"textures on the BSDFs inside a blendbsdf" in msg
    r, msg = rc(mat(0), mat(0), mat(BLEND, eta=(0, 1, 0)), mat(BLEND, eta=(0, 2, 0))); assert r == 3 and b"plain BSDF records" in msg
    r, msg = rc(mat(0), mat(COAT, distr=0, eta=(1.5, 0, 0)), mat(MIX, distr=2, refl=(0, 1, 0), k=(0.5, 0.5, 0))); assert r == 3 and b"children of a mixturebsdf" in msg
    assert rc(mat(WARD, flags=8, distr=2, alpha=0.1, k=(0.3, 0.4, 0), spec=(0.2, 0.2, 0.2)))[0] == 0
    RCOAT, COND = 19, 2
    r, msg = rc(mat(COND), mat(RCOAT, distr=0, eta=(1.5, 1.0, 0.0), k=(0, 0, 100))); assert r == 3 and b"without a Dirac delta lobe" in msg
    assert rc(mat(0), mat(RCOAT, distr=0, eta=(1.5, 1.0, 1.0), k=(0, 0, 100)))[0] == 0          # (its transmittance slice is checked at commit)
    r, msg = rc(mat(0), mat(RCOAT, distr=0, eta=(1.5, 1.0, 3.0), k=(0, 0, 100))); assert r == 1 and b"invalid distribution" in msg
    assert rc(mat(20))[0] == 3
    L.L.mi_scene_destroy(h)


def test_scene_generators(mi):
    S = mi.scenes
    sc = S.cornell_box()
    assert len(sc.idx) == 32 and sc.width == 1920 and sc.height == 1080 and len(sc.emitters) == 1
    # consistent winding: wall normals face the room centre, block normals face away from the block centres
    c = np.array([278, 273, 280], np.float32)
    for t in range(12):
        p0, p1, p2 = sc.pos[sc.idx[t]]; n = np.cross(p1 - p0, p2 - p0)
        assert np.dot(n, c - (p0 + p1 + p2) / 3) > 0
    for si in (6, 7):
        s = sc.shapes[si]; verts = sc.pos[s["first_vert"]:s["first_vert"] + s["vert_count"]]; centre = verts.mean(0)
        for t in range(s["first_tri"], s["first_tri"] + s["tri_count"]):
            p0, p1, p2 = sc.pos[sc.idx[t]]; n = np.cross(p1 - p0, p2 - p0)
            assert np.dot(n, (p0 + p1 + p2) / 3 - centre) > 0
    # camera matrix: sample (0.5, 0.5) maps to the optical axis
    m = sc.sample_to_camera.astype(np.float64); p = m @ np.array([0.5, 0.5, 0, 1.0]); p = p[:3] / p[3]
    assert abs(p[0]) < 1e-6 and abs(p[1]) < 1e-6 and abs(p[2] - sc.near) < 1e-4
    import tempfile
    with tempfile.NamedTemporaryFile(suffix=".miscene") as f:
        S.save_scene(sc, f.name); assert os.path.getsize(f.name) > 1000


def test_tile_sharding(mi):
    d = importlib_dist(mi)
    for h, world in [(1080, 1), (1080, 2), (1080, 8), (7, 8), (2160, 5)]:
        bands = [d.shard_rows(h, r, world) for r in range(world)]
        assert bands[0][0] == 0 and bands[-1][1] == h
        assert all(bands[i][1] == bands[i + 1][0] for i in range(world - 1))
        sizes = [b - a for a, b in bands]; assert max(sizes) - min(sizes) <= 1


def importlib_dist(mi):
    import importlib
    return importlib.import_module("mitsuba-im_amd.dist")


def test_bench_dump_outputs_size_limit(tmp_path, monkeypatch):
    """bench.py's --dump-outputs writer: float32 as a whole within the size limit, above it a fixed seeded sample of pixels with their flat indices"""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    small = np.arange(6 * 5 * 3, dtype=np.float64).reshape(6, 5, 3)
    bench.dump_outputs(str(tmp_path / "a"), {"film": small})
    got = np.load(tmp_path / "a" / "film.npy")
    assert got.dtype == np.float32 and (got == small).all()
    big = np.random.default_rng(1).random((200, 300, 5)).astype(np.float32)
    monkeypatch.setattr(bench, "DUMP_LIMIT", 40_000)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"film": big})
    assert sorted(os.listdir(tmp_path / "b")) == ["film_sample.npy", "film_sample_index.npy"]
    s, i = np.load(tmp_path / "b" / "film_sample.npy"), np.load(tmp_path / "b" / "film_sample_index.npy")
    assert s.dtype == np.float32 and i.dtype == np.float64 and s.nbytes + i.nbytes <= 40_000 and len(s) > 1000
    assert (np.diff(i) > 0).all() and (s == big.reshape(-1, 5)[i.astype(np.int64)]).all()
    assert (np.load(tmp_path / "c" / "film_sample_index.npy") == i).all()


def _uncommitted_scene(mi, sc):
    """an mi_scene holding sc's geometry (triangles, analytic shapes, instances), not committed: nothing here touches a device"""
    L = mi.lib(); A = mi.api; h = C.c_void_p(); L.check(L.L.mi_scene_create(C.byref(h)))
    shapes = (A.MiShape * len(sc.shapes))()
    for i, s in enumerate(sc.shapes):
        shapes[i] = A.MiShape(s["first_tri"], s["tri_count"], s["first_vert"], s["vert_count"], s["bsdf"], s["emitter"], s["face_normals"] & 1, s.get("group", 0))
    L.check(L.L.mi_scene_set_triangles(h, sc.pos.ctypes.data, None, None, sc.idx.ctypes.data, len(sc.pos), len(sc.idx), C.cast(shapes, C.c_void_p), len(sc.shapes)))
    recs = sc.get("analytic") or []
    if recs:
        an = (A.MiAnalytic * len(recs))()
        for i, a in enumerate(recs):
            r = A.MiAnalytic(a["type"], a["bsdf"], a["emitter"], a["flags"]); r.to_world[:] = a["to_world"].reshape(-1).tolist(); r.to_object[:] = a["to_object"].reshape(-1).tolist()
            r.radius, r.length = a["radius"], a["length"]; an[i] = r
        L.check(L.L.mi_scene_set_analytic(h, C.cast(an, C.c_void_p), len(recs)))
    insts = sc.get("instances") or []
    if insts:
        arr = (A.MiInstance * len(insts))()
        for i, a in enumerate(insts):
            r = A.MiInstance(a["group"]); r.to_world[:] = a["to_world"].reshape(-1).tolist(); r.to_object[:] = a["to_object"].reshape(-1).tolist(); arr[i] = r
        L.check(L.L.mi_scene_set_instances(h, C.cast(arr, C.c_void_p), len(insts)))
    return h


def test_fused_walk_entry_refuses_without_gpu(mi, monkeypatch):
    """mi_debug_intersect_fused serves triangle-only trees: analytic shapes, instances and packet scenes are refused with MI_ERR_UNSUPPORTED and a message naming the
    reason -- decided on host data, before the commit check and before any device call, so no kernel runs."""
    monkeypatch.delenv("MI355PT_NO_PACKET", raising=False)
    L = mi.lib(); S = mi.scenes
    rays = np.zeros((1, 8), np.float32); rays[0, 3] = 1e-4; rays[0, 6] = 1; rays[0, 7] = np.inf
    seg = np.array([1], np.uint32); out = np.zeros((1, 4), np.float32); info = mi.api.MiFusedDebugInfo()
    def call(h, any_hit=0, n_seg=1, thr=48, grid=1, lds=10):
        rc = L.L.mi_debug_intersect_fused(h, rays.ctypes.data, 1, any_hit, seg.ctypes.data, n_seg, thr, grid, lds, out.ctypes.data, C.byref(info)); return rc, L.L.mi_last_error()
    for sc, word in ((S.cbox_shapes(32, 32, 1), b"analytic shapes"), (S.instanced_garden(32, 32, 1), b"instances"), (S.cornell_box(16, 9, 1), b"triangle packet")):
        h = _uncommitted_scene(mi, sc)
        for any_hit in (0, 1):
            rc, msg = call(h, any_hit); assert rc == 3 and word in msg and b"mi_debug_intersect_fused" in msg, (rc, msg)
        L.L.mi_scene_destroy(h)
    h = _uncommitted_scene(mi, S.closed_box()); monkeypatch.setenv("MI355PT_NO_PACKET", "1")      # 26 triangles, but the packet is switched off: only the commit is missing
    rc, msg = call(h); assert rc == 1 and b"must be committed" in msg
    rc, msg = call(None); assert rc == 1 and b"null argument" in msg
    L.L.mi_scene_destroy(h)


def test_fused_walk_ray_sets_without_gpu(mi):
    """The numpy side of tests/test_gpu_fused_walk.py (b): the speck scene and its rays meet the precondition of the empty-slot case -- the room has >= 64 triangles, the
    speck 12 .. 24 of extent ~1e-5 (in its plane y = 0) around the origin, and for >= 1000 rays max_a(2 extent_a / |d_a|) <= 1e-6 t, among them rays along the body diagonals."""
    from tests import test_gpu_fused_walk as F
    sc = mi.scenes.speck_room(); s = sc.shapes[-1]; T = s["tri_count"]
    V = sc.pos[s["first_vert"]:s["first_vert"] + s["vert_count"]]
    assert len(sc.idx) - T >= 64 and 12 <= T <= 24 and 2 <= F.speck_leaf_bounds(sc)[1] <= 3
    e = V.max(0) - V.min(0); assert (np.abs(V.max(0) + V.min(0)) < 1e-9).all() and 2e-6 < e[0] < 3e-5 and 2e-6 < e[2] < 3e-5 and e[1] == 0      # flat: see test_speck_rays_short_of_the_slack
    rays, counts = F.speck_rays(sc)
    t = np.linalg.norm(rays[:, :3].astype(np.float64), axis=1); d = np.abs(rays[:, 4:7].astype(np.float64))
    assert counts.sum() >= 1000 and 0.9 < t.min() < 1.1 and 99 < t.max() < 101.1
    ext = F.speck_extent(sc); assert (ext < 1e-5).all()
    assert ((2 * ext[None, :] / d[counts]).max(1) <= 1e-6 * t[counts]).all() and t[counts].min() > 10
    assert (np.abs(d[counts] - 3 ** -0.5) < 1e-6).all(1).sum() >= 100      # body diagonals among them
    assert (~counts[(d == 0).any(1)]).all()                              # an axis-parallel ray never qualifies: its zero components keep the inverted box shut
    sl = mi.scenes.sliver_stack(); r = F.sliver_rays(sl)
    assert 4000 <= len(sl.idx) <= 4200 and len(r) == 2400 and np.allclose(np.linalg.norm(r[:, 4:7], axis=1), 1, atol=1e-6)


def test_surface_units_entry_refuses_without_gpu(mi):
    """mi_debug_surface is exported, and its bad-argument paths are decided on the arguments alone, before the commit check and before any device call: a NULL scene,
    ray, hit or output pointer, n == 0, a mode outside 0..2, modes 1 / 2 without their query values; with good arguments an uncommitted scene is what is refused."""
    L = mi.lib(); assert "mi_debug_surface" in mi.api.EXPORTS and hasattr(L.L, "mi_debug_surface")
    h = _uncommitted_scene(mi, mi.scenes.cornell_box(16, 9, 1))
    rays = np.zeros((1, 8), np.float32); hits = np.full((1, 4), -1.0, np.float32); inst = np.full(1, -1, np.int32); q = np.zeros((1, 3), np.float32); out = np.zeros((1, 51), np.float32)
    r, t, i, qq, o = (a.ctypes.data for a in (rays, hits, inst, q, out))
    def call(*a): rc = L.L.mi_debug_surface(*a); return rc, L.L.mi_last_error()
    for args in ((None, 0, r, t, i, None, None, 1, o), (h, 0, None, t, i, None, None, 1, o), (h, 0, r, None, i, None, None, 1, o), (h, 0, r, t, i, None, None, 1, None), (h, 0, r, t, i, None, None, 0, o),
                 (h, -1, r, t, i, None, None, 1, o), (h, 3, r, t, i, None, qq, 1, o), (h, 1, r, t, i, None, None, 1, o), (h, 2, r, t, i, None, None, 1, o)):
        rc, msg = call(*args); assert rc == 1 and b"mi_debug_surface: bad argument" in msg, (args[1], rc, msg)
    for args in ((h, 0, r, t, i, None, None, 1, o), (h, 0, r, t, None, None, None, 1, o), (h, 1, r, t, i, None, qq, 1, o), (h, 2, r, t, i, None, qq, 1, o)):
        rc, msg = call(*args); assert rc == 1 and b"mi_debug_surface: the scene must be committed" in msg, (args[1], rc, msg)
    L.L.mi_scene_destroy(h)


def test_film_units_entry_refuses_without_gpu(mi):
    """mi_render_debug_film_put is exported and bound; its null-argument refusal is decided before any device call (a render handle cannot exist without a device: the
    other refusals -- tile, planes, positions, the preconditions of `which` -- are in tests/test_gpu_film_units.py test_refusals)"""
    L = mi.lib(); assert "mi_render_debug_film_put" in mi.api.EXPORTS and hasattr(L.L, "mi_render_debug_film_put")
    pos = np.zeros((1, 1, 2), np.float32); val = np.zeros((1, 1, 4), np.float32); t = mi.api.MiTile(0, 0, 1, 1)
    for which in (0, 1, 2, 7):
        rc = L.L.mi_render_debug_film_put(None, which, t, 1, 1, 0, pos.ctypes.data, val.ctypes.data)
        assert rc == 1 and b"mi_render_debug_film_put: null argument" in L.L.mi_last_error()
    assert hasattr(mi.Render, "film_put_units")
