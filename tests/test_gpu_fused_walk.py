"""GPU (MI355X): the fused tree walk of csrc/trace_fused.h -- the ray cast of every large triangle scene (k_extend_f / k_shadow_f) -- handed rays one by one through
mi_debug_intersect_fused (Scene.intersect_fused), which lays them into queue segments and launches the stage production launches.  Every comparison is bit for bit
against the oracle's closest hit (hit flag, t, u, v, global triangle index) and any-hit flag; no tolerance anywhere.  The ray generators and the conditions they
must meet (share of hits, share of ties, the empty-slot precondition) are plain numpy over the oracle, so they are also checked without a GPU
(tests/test_host_logic.py)."""
import math
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the oracle's side
def oracle_results(orc, sc, rays):
    """closest hit and any hit of every ray: dict(hit, tuv (float32), prim (global triangle index, -1: miss), occ)"""
    n = len(rays); hit = np.zeros(n, bool); tuv = np.zeros((n, 3), np.float32); prim = np.full(n, -1, np.int64); occ = np.zeros(n, bool)
    first = np.array([s["first_tri"] for s in sc.shapes], np.int64)
    for i in range(n):
        ok, h = orc.intersect(rays[i]); hit[i] = ok
        if ok: tuv[i] = (h[0], h[13], h[14]); prim[i] = first[int(h[19])] + int(h[18])
        occ[i] = orc.occluded(rays[i])
    return dict(hit=hit, tuv=tuv, prim=prim, occ=occ)


def _wald(acc, o, d):
    """TriAccel::rayIntersect without the interval test, in numpy float32 with the oracle's operation order: acc (..., 10) = orc_triaccel records, o / d (..., 3).
    Returns (t, inside)."""
    f = np.float32; k = acc[..., 0].astype(np.int64); kk = np.where(k < 3, k, 0)
    def comp(v, j): return np.take_along_axis(v, ((kk + j) % 3)[..., None], -1)[..., 0]
    o_k, o_u, o_v, d_k, d_u, d_v = comp(o, 0), comp(o, 1), comp(o, 2), comp(d, 0), comp(d, 1), comp(d, 2)
    n_u, n_v, n_d, a_u, a_v, b_nu, b_nv, c_nu, c_nv = (acc[..., j].astype(f) for j in range(1, 10))
    with np.errstate(all="ignore"):
        t = (n_d - o_u * n_u - o_v * n_v - o_k) / (d_u * n_u + d_v * n_v + d_k)
        hu = o_u + t * d_u - a_u; hv = o_v + t * d_v - a_v
        uu = hv * b_nu + hu * b_nv; vv = hu * c_nu + hv * c_nv
        return t, (k < 3) & (uu >= 0) & (vv >= 0) & (uu + vv <= f(1.0))


def tie_flags(oracle, orc, sc, rays, res):
    """Which hitting rays meet two triangles at an equal t: the oracle's Wald records (orc_triaccel) of the triangles that share a vertex position with the hit
    triangle, evaluated in the oracle's arithmetic.  The evaluation is checked against the oracle first: it reproduces t of every hit bit for bit."""
    L = oracle.lib(); nt = len(sc.idx)
    acc = np.zeros((nt, 10), np.float32)
    for t in range(nt): L.orc_triaccel(orc.h, t, acc[t].ctypes.data)
    _, vid = np.unique(sc.pos, axis=0, return_inverse=True); tv = vid.reshape(-1)[sc.idx.astype(np.int64)]      # (nt, 3) position ids
    order = np.argsort(tv.reshape(-1), kind="stable"); owners = order // 3; sorted_v = tv.reshape(-1)[order]
    start = np.searchsorted(sorted_v, np.arange(sorted_v.max() + 2))
    h = np.flatnonzero(res["hit"]); ties = np.zeros(len(rays), bool)
    o = rays[h, 0:3]; d = rays[h, 4:7]; p = res["prim"][h]
    t_self, in_self = _wald(acc[p], o, d)
    assert (bits(t_self) == bits(res["tuv"][h, 0])).all() and in_self.all(), "the numpy restatement of the Wald test disagrees with the oracle"
    for j, i in enumerate(h):
        cand = np.unique(np.concatenate([owners[start[v]:start[v + 1]] for v in tv[p[j]]])); cand = cand[cand != p[j]]
        if len(cand) == 0: continue
        tc, inside = _wald(acc[cand], np.broadcast_to(o[j], (len(cand), 3)), np.broadcast_to(d[j], (len(cand), 3)))
        ties[i] = bool((inside & (bits(tc) == bits(t_self[j:j + 1]))).any())
    return ties


# ------------------------------------------------------------------------------------------------ ray generators
def targeted_rays(sc, rng, tris_per_round=160, rounds=12):
    """The six target kinds and three origin kinds of test_packet_candidate_search_is_conservative (tests/test_gpu_parity.py), on `tris_per_round` random triangles
    per round: rays exactly at vertices and at points on edges, at interior points, next to the centroid, within 1e-6 of an edge, in the plane but mostly outside;
    from origins inside the scene box, ON other surfaces, and (almost) in the target triangle's plane; every fourth round ends the interval (almost) at the target."""
    P = sc.pos[sc.idx.reshape(-1, 3).astype(np.int64)].astype(np.float64); nt = len(P); lo, hi = sc.pos.min(0), sc.pos.max(0); ext = (hi - lo).max()
    m = min(nt, tris_per_round); rays = []
    for rep in range(rounds):
        t = rng.integers(0, nt, m); w = rng.dirichlet([1, 1, 1], m)
        for kind in range(6):
            if kind == 0: target = P[t, rng.integers(0, 3, m)]
            elif kind == 1: a = rng.random((m, 1)); e = rng.integers(0, 3, m); target = P[t, e] * a + P[t, (e + 1) % 3] * (1 - a)
            elif kind == 2: target = (P[t] * w[:, :, None]).sum(1)
            elif kind == 3: target = (P[t, 0] + P[t, 1] + P[t, 2]) / 3 + (P[t, 1] - P[t, 0]) * 1e-4
            elif kind == 4: a = rng.random((m, 1)); target = P[t, 1] * a + P[t, 2] * (1 - a) + (P[t, 0] - P[t, 1]) * 1e-6 * rng.normal(size=(m, 1))
            else: target = P[t, 0] + (P[t, 1] - P[t, 0]) * rng.random((m, 1)) * 3 - (P[t, 2] - P[t, 0]) * rng.random((m, 1))
            if rep % 3 == 0: o = lo + rng.random((m, 3)) * (hi - lo)
            elif rep % 3 == 1:
                t2 = rng.integers(0, nt, m); o = (P[t2] * rng.dirichlet([1, 1, 1], m)[:, :, None]).sum(1)
            else:
                nrm = np.cross(P[t, 1] - P[t, 0], P[t, 2] - P[t, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True) + 1e-30
                side = P[t, 0] + (P[t, 1] - P[t, 0]) * (rng.random((m, 1)) * 4 - 2) + (P[t, 2] - P[t, 0]) * (rng.random((m, 1)) * 4 - 2)
                o = side + nrm * ext * 10.0 ** rng.uniform(-7, -2, (m, 1)) * rng.choice([-1, 1], (m, 1))
            d = target - o; ln = np.linalg.norm(d, axis=1, keepdims=True); ok = ln[:, 0] > 1e-9
            d = d / np.maximum(ln, 1e-30)
            mint = np.full(m, 1e-4); maxt = np.full(m, np.inf)
            if rep % 4 == 3: maxt = ln[:, 0] * (1 + rng.choice([-1e-6, 0, 1e-6], m))
            rays.append(np.concatenate([o, mint[:, None], d, maxt[:, None]], 1)[ok])
    return np.concatenate(rays).astype(np.float32)


def near_rays(sc, rng, n=2400):
    """The supply of ties (two triangles answering at one t).  Half: rays exactly at vertices from 0.1 .. 1 of the scene's extent away -- the triangles of the fan
    around the vertex each decide on their own rounding whether they hold the hit point, and their planes often round to one t.  Half: short rays (3e-4 .. 1e-2 of
    the extent) at points on edges, where the rounding of the direction moves the hit point by less than the edge tests resolve."""
    P = sc.pos[sc.idx.reshape(-1, 3).astype(np.int64)].astype(np.float64); nt = len(P); ext = float((sc.pos.max(0) - sc.pos.min(0)).max())
    t = rng.integers(0, nt, n); e = rng.integers(0, 3, n); a = rng.random((n, 1)); a[::2] = 1.0
    target = P[t, e] * a + P[t, (e + 1) % 3] * (1 - a)
    v = rng.normal(size=(n, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    dist = ext * 10.0 ** rng.uniform(-3.5, -2, (n, 1)); dist[::2] = ext * 10.0 ** rng.uniform(-1, 0, (n // 2, 1))
    o = target + v * dist; d = target - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, np.full((n, 1), 1e-4), d, np.full((n, 1), np.inf)], 1).astype(np.float32)


def box_rays(sc, rng, n=1500):
    """The ray set of test_intersection_bit_exact scaled to the scene: random origins in and around the scene box, random directions, zero direction components on
    one axis, on two axes, finite maxt."""
    lo, hi = sc.pos.min(0), sc.pos.max(0); ext = float((hi - lo).max()); lo, hi = lo - 0.1 * ext, hi + 0.1 * ext
    o = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    d = rng.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d[:50, 0] = 0; d[50:100, 1] = 0; d[100:110] = [0, 0, 1]; d[110:120] = [0, -1, 0]; d[120:130] = [1, 0, 0]
    rays = np.concatenate([o, np.full((n, 1), 1e-4, np.float32), d, np.full((n, 1), np.inf, np.float32)], 1).astype(np.float32)
    rays[200:400, 7] = rng.random(200) * ext
    return rays


def plane_rays(sc, rng, n=600):
    """Axis-parallel rays whose origins lie exactly on the bounding planes of the scene (the planes the root's child boxes are cut from), pointing inwards; half of
    them share their other two coordinates with a vertex, so they run along triangle edges and through vertices."""
    lo, hi = sc.pos.min(0).astype(np.float32), sc.pos.max(0).astype(np.float32); rays = np.zeros((n, 8), np.float32)
    for i in range(n):
        a = i % 3; far = (i // 3) % 2
        o = (lo + rng.random(3).astype(np.float32) * (hi - lo)) if i % 4 < 2 else sc.pos[rng.integers(0, len(sc.pos))].copy()
        o[a] = hi[a] if far else lo[a]; d = np.zeros(3, np.float32); d[a] = -1.0 if far else 1.0
        rays[i] = (*o, 1e-4, *d, np.inf)
    return rays


def adversarial_rays(sc, orc, seed=23):
    """The ray set of tests (a) and (c): targeted_rays + near_rays + box_rays + plane_rays, and -- for 400 of them that hit -- the same ray three more times with maxt equal to
    the oracle's hit distance times (1 - 1e-6, 1, 1 + 1e-6)."""
    rng = np.random.default_rng(seed)
    base = np.concatenate([targeted_rays(sc, rng), near_rays(sc, rng), box_rays(sc, rng), plane_rays(sc, rng)])
    ends = []
    for i in rng.permutation(len(base)):
        if len(ends) >= 1200: break
        if not np.isinf(base[i, 7]): continue
        ok, h = orc.intersect(base[i])
        if ok:
            for f in (1 - 1e-6, 1.0, 1 + 1e-6):
                r = base[i].copy(); r[7] = np.float32(np.float64(h[0]) * f); ends.append(r)
    return np.concatenate([base, np.asarray(ends, np.float32).reshape(-1, 8)]).astype(np.float32)


def speck_extent(sc):
    """box of the speck (the last shape of scenes.speck_room) as the tree builder pads it (scene_build.cpp: 1e-4 of the largest extent + 2e-5 of the magnitude + 1e-7 per side)"""
    s = sc.shapes[-1]; P = sc.pos[s["first_vert"]:s["first_vert"] + s["vert_count"]].astype(np.float64); lo, hi = P.min(0), P.max(0)
    pad = 1e-4 * (hi - lo).max() + 2e-5 * (np.abs(lo) + np.abs(hi)).max() + 1e-7
    return (hi - lo) + 2 * pad


def speck_rays(sc, seed=31):
    """Rays from distance 1 .. 100 at the speck: at its vertices and triangle centroids, just past its edge, and through its centre; along each axis, each face
    diagonal, each body diagonal, and along random directions without a small component.  Returns (rays, counts): counts marks the rays that meet the precondition
    of the empty-slot case -- max_a(2 extent_a / |d_a|) <= 1e-6 t, the slack of the box test (2e-6 t) exceeds what an inverted box of a speck-sized node adds."""
    rng = np.random.default_rng(seed); s = sc.shapes[-1]
    V = sc.pos[s["first_vert"]:s["first_vert"] + s["vert_count"]].astype(np.float64)
    T = sc.pos[sc.idx[s["first_tri"]:s["first_tri"] + s["tri_count"]].astype(np.int64)].astype(np.float64).mean(1)
    h = np.abs(V).max()
    targets = np.concatenate([V[::3], T[::3], [[0, 0, 0]], [[1.2 * h, 0.6 * h, 0], [0, 0.6 * h, -1.2 * h], [-1.3 * h, -1.3 * h, -1.3 * h], [3 * h, 0, 0]]])
    dirs = [np.array(v, np.float64) for v in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]
    dirs += [np.array(v, np.float64) for v in ((1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1))]
    dirs += [np.array(v, np.float64) for v in ((1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1))]
    dirs = dirs + [-v for v in dirs]
    while len(dirs) < 26 + 150:
        v = rng.normal(size=3); v /= np.linalg.norm(v)
        if np.abs(v).min() >= 0.3: dirs.append(v)
    dirs = np.array([v / np.linalg.norm(v) for v in dirs])
    dists = np.array([1.0, 3.0, 10.0, 30.0, 45.0, 60.0, 80.0, 100.0])
    rays = []
    for tg in targets:
        for dist in dists:
            d = dirs.astype(np.float32); o = (tg[None, :] - dirs * dist).astype(np.float32)
            rays.append(np.concatenate([o, np.full((len(d), 1), 1e-4, np.float32), d, np.full((len(d), 1), np.inf, np.float32)], 1))
    rays = np.concatenate(rays).astype(np.float32)
    ext = speck_extent(sc); t = np.linalg.norm(rays[:, 0:3].astype(np.float64), axis=1)
    with np.errstate(divide="ignore"):
        counts = (2 * ext[None, :] / np.abs(rays[:, 4:7].astype(np.float64))).max(1) <= 1e-6 * t
    return rays, counts


def sliver_rays(sc, seed=37, n=2400):
    """rays through the unit cube of scenes.sliver_stack: between random points of two different faces of a slightly larger cube, from the camera side, along and
    across the diagonal the slivers span"""
    rng = np.random.default_rng(seed); rays = np.zeros((n, 8), np.float32)
    for i in range(n):
        if i % 4 == 3:          # along the bundle: parallel to the diagonal, through the grid of slivers
            o = rng.normal(size=3) * 0.04 - np.array([0.3, 0.3, 0.3]); d = np.array([1.0, 1.0, 1.0]) + (rng.normal(size=3) * 0.02 if i % 8 == 7 else 0.0)
        else:
            p = rng.random(3) * 1.2 - 0.1; q = rng.random(3) * 1.2 - 0.1; a, b = rng.integers(0, 3), rng.integers(0, 3)
            p[a] = -0.1; q[b] = 1.1; o = p; d = q - p
            if i % 4 == 2: o = 0.5 + (p - 0.5) * 3; d = (0.5 + rng.normal(size=3) * 0.05) - o      # from outside, across the middle of the bundle
        d = d / np.linalg.norm(d); rays[i] = (*o, 1e-4, *d, np.inf)
    return rays


# ------------------------------------------------------------------------------------------------ comparison
def assert_equal_to_oracle(res, got, occ, tag=""):
    """hit flag, (t, u, v) bits, global triangle index, any-hit flag -- the checks of the traverse<> tests"""
    ghit = got[:, 3] >= 0
    bad = np.flatnonzero(ghit != res["hit"]); assert len(bad) == 0, (tag, "hit flag", bad[:8])
    h = res["hit"]
    bad = np.flatnonzero(h & (bits(got[:, :3]) != bits(res["tuv"])).any(1)); assert len(bad) == 0, (tag, "t, u, v", bad[:8], got[bad[:2]], res["tuv"][bad[:2]])
    bad = np.flatnonzero(h & (got[:, 3].astype(np.int64) != res["prim"])); assert len(bad) == 0, (tag, "triangle", bad[:8], got[bad[:4], 3], res["prim"][bad[:4]])
    bad = np.flatnonzero((occ[:, 3] >= 0) != res["occ"]); assert len(bad) == 0, (tag, "any hit", bad[:8])


def assert_bookkeeping(info_c, info_a, n, tag=""):
    """every ray retired exactly once: no sentinel left in Queues::hit, the closest-hit counter grew by n, every shadow accumulator holds 0 or 1"""
    assert info_c["unretired"] == 0, (tag, info_c["unretired"])
    assert info_c["rays_counted"] == n, (tag, info_c["rays_counted"], n)
    assert np.isin(info_a["acc_x"], (0.0, 1.0)).all(), (tag, np.unique(info_a["acc_x"]))


def fused_both(gs, rays, **kw):
    got, ic = gs.intersect_fused(rays, **kw); occ, ia = gs.intersect_fused(rays, any_hit=True, **kw)
    assert_bookkeeping(ic, ia, len(rays), str(kw))
    return got, occ, ic, ia


ATRIUM_40K = dict(width=64, height=36, spp=1, detail=0.4, env_size=(64, 32))      # the scene of test_large_scene_bvh_vs_oracle


def scene_by_name(mi, golden_scenes, name):
    """bunny_box keeps its walls and its light as analytic rectangles, which the fused walk does not serve (mi_debug_intersect_fused refuses them, as production falls
    back to traverse<>): its mesh -- all 69 k triangles -- is taken without them, under a point light so that the scene still commits."""
    if name == "atrium_40k": return mi.scenes.atrium(**ATRIUM_40K)
    sc = golden_scenes[name]
    if sc.get("analytic"):
        sc = mi.scenes.Scene(sc); sc.analytic = []; sc.emitters = [mi.scenes.point_emitter((0.0, 1.5, 0.0), (10.0, 10.0, 10.0))]
    return sc


@pytest.fixture(scope="module")
def cases(mi, oracle, golden_scenes):
    """per scene: (scene, rays, the oracle's results), built once"""
    cache = {}
    def get(name):
        if name not in cache:
            sc = scene_by_name(mi, golden_scenes, name); orc = oracle.Oracle(sc); rays = adversarial_rays(sc, orc)
            cache[name] = (sc, rays, oracle_results(orc, sc, rays), orc)
        return cache[name]
    return get


# ------------------------------------------------------------------------------------------------ (a) adversarial rays, both node kinds
@pytest.mark.parametrize("bvh2", ["0", "1"])
@pytest.mark.parametrize("name", ["atrium_40k", "bunny_box", "veach_small"])
def test_adversarial_rays(mi, oracle, cases, name, bvh2, monkeypatch):
    """Rays where walks go wrong -- exactly at vertices and edges, grazing, zero direction components, intervals that end at the hit, origins on the bounding planes --
    through the 4-wide (MI355PT_BVH2=0) and the binary (=1) instantiation of the fused walk.  The oracle alone says the set is what it claims: at least a quarter of
    the rays hit, at least 1 % of those meet two triangles at an equal t (the tie-break of the closest hit)."""
    monkeypatch.setenv("MI355PT_NO_PACKET", "1"); monkeypatch.setenv("MI355PT_BVH2", bvh2)
    sc, rays, res, orc = cases(name)
    ties = tie_flags(oracle, orc, sc, rays, res)
    print(f"[fused-walk] {name}: {len(rays)} rays, {res['hit'].mean():.3f} hit, {ties.sum() / max(1, res['hit'].sum()):.4f} of the hits are ties")
    assert res["hit"].mean() >= 0.25 and ties.sum() >= 0.01 * res["hit"].sum()
    gs = mi.Scene(sc); got, occ, ic, ia = fused_both(gs, rays)
    print(f"[fused-walk] {name} bvh2={bvh2}: wide {ic['wide']} depth {ic['bvh_depth']} bound {ic['bvh_stack_direct']} deepest stack {ic['max_stack_seen']} / {ia['max_stack_seen']}")
    assert ic["wide"] == (bvh2 == "0")
    assert_equal_to_oracle(res, got, occ, name)
    assert max(ic["max_stack_seen"], ia["max_stack_seen"]) <= ic["bvh_stack_direct"] <= 3 * ic["bvh_depth"] + 4


# ------------------------------------------------------------------------------------------------ (b) unused slots of 4-wide nodes, small geometry seen from far away
MAX_LEAF = 8      # scene_build.cpp Builder::build: a leaf holds at most 8 primitives (every makeLeaf() is behind count <= 8 or count <= 2)


def speck_leaf_bounds(sc):
    """(T, least number of leaves): the speck's T triangles need at least ceil(T / MAX_LEAF) leaves; with T in 12 .. 24 that is two or three, so the speck cannot sit in
    one leaf -- it is a subtree of its own, far smaller than anything around it.  A subtree of L leaves fills every slot of its W four-wide nodes only if L = 3 W + 1;
    the builder as it stands gives the 18-triangle speck three nodes of three children each, of extent 2.2e-6 x 2e-7 x 6.2e-6: three unused slots."""
    T = sc.shapes[-1]["tri_count"]
    return T, math.ceil(T / MAX_LEAF)


@pytest.fixture(scope="module")
def speck_case(mi, oracle):
    sc = mi.scenes.speck_room(); rays, counts = speck_rays(sc); orc = oracle.Oracle(sc)
    return sc, rays, counts, oracle_results(orc, sc, rays)


def _compare_speck(mi, speck_case, sel, tag):
    """closest and any hit of the selected speck rays through the fused walk AND through traverse<> (Scene.intersect): both walks read the same unused slots"""
    sc, rays, counts, res = speck_case; T = sc.shapes[-1]["tri_count"]; sub = {k: v[sel] for k, v in res.items()}; r = rays[sel]
    on = (sub["prim"] >= len(sc.idx) - T).sum()
    print(f"[fused-walk] speck, {tag}: {len(r)} rays, {sub['hit'].mean():.3f} hit, {on} on the speck")
    gs = mi.Scene(sc); got, occ, ic, ia = fused_both(gs, r); tr, tro = gs.intersect(r), gs.intersect(r, any_hit=True)
    for name, g in (("fused walk", got), ("traverse", tr)):
        differ = (sub["hit"] != (g[:, 3] >= 0)) | (sub["hit"] & ((bits(g[:, :3]) != bits(sub["tuv"])).any(1) | (g[:, 3].astype(np.int64) != sub["prim"])))
        print(f"[fused-walk] speck, {tag}, {name}: {differ.sum()} of {len(r)} closest hits differ from the oracle's")
    assert ic["wide"] == 1 and on >= 100
    assert_equal_to_oracle(sub, got, occ, f"speck, {tag}, fused walk")
    assert_equal_to_oracle(sub, tr, tro, f"speck, {tag}, traverse")
    assert max(ic["max_stack_seen"], ia["max_stack_seen"]) <= ic["bvh_stack_direct"]


def test_empty_slots_far_away(mi, speck_case, monkeypatch):
    """A subtree that ends in fewer than four leaves leaves slots of its 4-wide nodes unused.  Their inverted boxes (qlo 255, qhi 0) fail the box test only while
    255 step / |d| exceeds its slack 2e-6 t: for a speck of 6e-6 seen from t > ~30 the unused slot passes and the walk follows its code.  That code now names a
    record no triangle test accepts (scene_build.cpp MI_K_NONE), in the fused walk and in traverse<> alike.  These are the rays that meet the precondition."""
    monkeypatch.setenv("MI355PT_BVH2", "0")
    sc, rays, counts, res = speck_case
    assert len(sc.idx) - sc.shapes[-1]["tri_count"] >= 64
    T, leaves = speck_leaf_bounds(sc); assert 12 <= T <= 24 and 2 <= leaves <= 3
    assert counts.sum() >= 1000, counts.sum()      # the precondition, in numpy: these rays would have followed an unused slot
    _compare_speck(mi, speck_case, counts, "past the slack")


def test_speck_rays_short_of_the_slack(mi, speck_case, monkeypatch):
    """The rest of the speck rays: nearer than the precondition asks, or with a zero direction component (each axis, each face diagonal), which keeps an unused slot shut:
    on such an axis the box test compares the origin's coordinate with the box exactly (the reciprocal is 1e30, no slack survives).
    Why the speck is flat (scenes.speck_room): from t = 100 the Wald test rounds t to ulp(100) = 7.6e-6, more than a speck triangle, and never looks at the axis it
    projects along.  On a TILTED speck a ray with d = 0 on that axis is then given a triangle it passes 1e-6 beside -- by the test over all triangles, and by a
    tree only if its leaf padding happens to be that large (the oracle's is 1e-6, the product's 1e-7: 23 such rays differed, in both walks).  There the answer
    is a property of the padding constant, not of the ray cast, so it is no reference.  On a patch perpendicular to its projection axis the coordinates on every
    zero-direction axis are exact in the Wald test and in the box test alike, and every ray of the set has one answer (the oracle's tree and its loop over all
    triangles agree on all 32384, checked on the CPU)."""
    monkeypatch.setenv("MI355PT_BVH2", "0")
    sc, rays, counts, res = speck_case
    _compare_speck(mi, speck_case, ~counts, "short of the slack")


# ------------------------------------------------------------------------------------------------ (c) the stack beyond its LDS entries
@pytest.mark.parametrize("bvh2", ["0", "1"])
@pytest.mark.parametrize("name", ["atrium_40k", "bunny_box", "veach_small"])
def test_stack_spill_small_lds(mi, cases, name, bvh2, monkeypatch):
    """four LDS entries per lane: the ray set of (a) drives every tree through the spill pushes and pops"""
    monkeypatch.setenv("MI355PT_NO_PACKET", "1"); monkeypatch.setenv("MI355PT_BVH2", bvh2)
    sc, rays, res, _ = cases(name)
    got, occ, ic, ia = fused_both(mi.Scene(sc), rays, lds_stack=4)
    print(f"[fused-walk] {name} bvh2={bvh2} lds_stack=4: deepest stack {ic['max_stack_seen']} / {ia['max_stack_seen']}, bound {ic['bvh_stack_direct']}")
    assert ic["max_stack_seen"] > 4
    assert_equal_to_oracle(res, got, occ, name)
    assert max(ic["max_stack_seen"], ia["max_stack_seen"]) <= ic["bvh_stack_direct"]


def test_stack_spill_sliver_stack(mi, oracle, monkeypatch):
    """4096 slivers along the diagonal of the unit cube: every box is nearly the whole cube, so a ray through it descends every level with all siblings waiting --
    more than the 10 LDS entries of production, within the builder's bound (which sizes the production spill area), which is within the worst case the debug entry
    allocates for.  Then the same scene through Render.samples: the production allocation of Queues::stkSpill and k_extend_f / k_shadow_f themselves."""
    monkeypatch.setenv("MI355PT_BVH2", "0")
    sc = mi.scenes.sliver_stack(); rays = sliver_rays(sc); orc = oracle.Oracle(sc); res = oracle_results(orc, sc, rays)
    gs = mi.Scene(sc); got, occ, ic, ia = fused_both(gs, rays)
    print(f"[fused-walk] sliver_stack: {res['hit'].mean():.3f} hit, depth {ic['bvh_depth']} bound {ic['bvh_stack_direct']} deepest stack {ic['max_stack_seen']} / {ia['max_stack_seen']}")
    assert ic["wide"] == 1
    assert ic["max_stack_seen"] > 10
    assert max(ic["max_stack_seen"], ia["max_stack_seen"]) <= ic["bvh_stack_direct"]
    assert ic["bvh_stack_direct"] <= 3 * ic["bvh_depth"] + 4
    assert_equal_to_oracle(res, got, occ, "sliver_stack")
    rng = np.random.default_rng(41); n = 2000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    li = mi.Render(gs).samples(pairs); ref = orc.render_samples(pairs)["li"]
    assert (bits(li) == bits(ref)).all()
    assert ref.max() > 0


# ------------------------------------------------------------------------------------------------ (d) refill and segments
def test_refill_and_segments(mi, oracle):
    """take / rank / nxt and the ticket over ragged segments: empty segments, a single ray, full segments, a ragged last one; one workgroup, seven, the production grid;
    refill when no lane is busy, at the production threshold, at every idle lane.  A ray lost or traced twice shows as a sentinel, a counter, an accumulator of 2 --
    and every combination returns the same bits, the oracle's."""
    sc = mi.scenes.atrium(**ATRIUM_40K); gs = mi.Scene(sc); orc = oracle.Oracle(sc)
    rng = np.random.default_rng(9); n = 4000      # the rays of test_large_scene_bvh_vs_oracle
    lo, hi = sc.pos.min(0), sc.pos.max(0)
    o = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32); o[:, 1] = np.abs(o[:, 1]) * 0.9 + 0.05
    d = rng.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays = np.concatenate([o, np.full((n, 1), 1e-4, np.float32), d, np.full((n, 1), np.inf, np.float32)], 1).astype(np.float32)
    res = oracle_results(orc, sc, rays)
    layouts = [[0, 1, 1024, 0, 1024, 63, 0, 1024, 500, 364], [64] * 62 + [0, 0, 31, 1], [4000], [0, 0, 0, 4000, 0]]
    first = None
    for seg in layouts:
        assert sum(seg) == n
        for thr in (1, 48, 64):
            for grid in (1, 7, 1792):
                got, occ, ic, ia = fused_both(gs, rays, seg_counts=seg, thr=thr, grid=grid)
                if first is None:
                    first = (got, occ); assert_equal_to_oracle(res, got, occ, "refill")
                assert (bits(got) == bits(first[0])).all() and (bits(occ) == bits(first[1])).all(), (len(seg), thr, grid)
