"""Scenes and rays of tests/test_gpu_packet_units.py (the small-scene packet ray cast, csrc/trace.h), and the oracle's answers to them.  tests/test_packet_inputs.py
takes a census of these inputs against the oracle alone; the GPU test compares the device with the same answers.  Everything is a function of fixed seeds."""
import numpy as np

f32 = np.float32
CATS = ("vertex", "edge", "near_edge", "interior", "in_plane", "surface_origin", "grazing", "one_zero", "two_zero", "parallel_in_plane", "centroid",
        "maxt_at_hit", "mint_at_hit")
STACKS = ("stack_k0", "stack_k1", "stack_k2")
NAMES = ("one", "pgram", "trapezoid") + STACKS + ("n32", "n33", "n64", "tie", "far")
_cache = {}


def _unit(v):
    v = np.asarray(v, np.float64); return v / np.linalg.norm(v)


def _quad(c, n, h, K):
    """two triangles of a square (a parallelogram: one pass-1 record) of half size h around c with normal n, whose largest component is along axis K"""
    ax = np.eye(3); n = _unit(n); e1 = _unit(np.cross(n, ax[(K + 2) % 3])); e2 = np.cross(n, e1); c = np.asarray(c, np.float64)
    p = [c - h * e1 - h * e2, c + h * e1 - h * e2, c + h * e1 + h * e2, c - h * e1 + h * e2]
    return [np.array([p[0], p[1], p[2]]), np.array([p[0], p[2], p[3]])]


def _stack(K):
    """four staggered parallel quads per direction: two axis-aligned directions' worth (normal = axis K) and four tilted (n_u, n_v != 0), each quad's centre outside
    the footprint of its neighbours, so a ray along the normal through a centre hits that quad and no other of its direction"""
    ax = np.eye(3); tris = []
    for tilt, base in (((0.0, 0.0), 0.0), ((0.3, -0.2), 6.0)):
        n = ax[K] + tilt[0] * ax[(K + 1) % 3] + tilt[1] * ax[(K + 2) % 3]
        for j in range(4):
            c = ax[K] * (0.5 * j - 0.75) + ax[(K + 1) % 3] * (0.8 * j - 1.2 + base) + ax[(K + 2) % 3] * 0.1 * j
            tris += _quad(c, n, 0.5, K)
    return tris


def _many(n, seed):
    """exactly n triangles: quads of all three axis classes with random tilts, and one lone triangle when n is odd"""
    rng = np.random.default_rng(seed); ax = np.eye(3); tris = []
    for j in range(n // 2):
        K = j % 3; nrm = ax[K] * rng.choice([-1, 1]) + ax[(K + 1) % 3] * rng.uniform(-0.6, 0.6) + ax[(K + 2) % 3] * rng.uniform(-0.6, 0.6)
        tris += _quad(rng.uniform(-2, 2, 3), nrm, rng.uniform(0.3, 0.8), K)
    if n % 2: tris.append(np.array([[0.1, 0.2, 2.5], [1.3, 0.1, 2.6], [0.4, 1.2, 2.4]]))
    assert len(tris) == n
    return tris


def triangles(name):
    if name == "one": return [np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.2], [0.2, 1.0, -0.1]])]
    if name == "pgram": return _quad((0.1, 0.2, 0.3), (0.2, 1.0, 0.3), 0.7, 1)
    if name == "trapezoid":      # coplanar, sharing an edge, not a parallelogram: two single-triangle records of one plane
        p = np.array([[0, 0, 0], [2, 0, 0.4], [1.5, 1, 0.5], [0.5, 1, 0.3]], np.float64); return [p[[0, 1, 2]], p[[0, 2, 3]]]
    if name in STACKS: return _stack(STACKS.index(name))
    if name in ("n32", "n33", "n64"): return _many(int(name[1:]), 5)
    if name == "tie":            # triangles 0 and 1 are the same triangle (equal t, u, v: the lower index wins), 2 overlaps them in the same plane, 3 is a bystander
        a = np.array([[0.0, 0.0, 0.5], [1.0, 0.0, 0.5], [0.0, 1.0, 0.5]]); return [a, a.copy(), np.array([[-0.5, -0.5, 0.5], [1.5, -0.25, 0.5], [-0.25, 1.5, 0.5]]), a + [0.2, 0.1, 1.0]]
    if name == "far": return [t + np.array([1000.0, -2000.0, 500.0]) for t in _stack(1) + _quad((0.3, 2.0, 0.1), (0.4, 0.2, 1.0), 0.6, 2)]      # |o| >> extent
    raise KeyError(name)


def scene(S, name):
    tris = triangles(name); b = S._Builder(); m = b.bsdf(reflectance=(0.5, 0.5, 0.5)); b.begin()
    for T in tris:
        base = len(b.verts); b.verts.extend(tuple(map(float, p)) for p in T); b.tris.append((base, base + 1, base + 2))
    b.end(m, radiance=(1.0, 1.0, 1.0))
    P = np.concatenate(tris); c = (P.min(0) + P.max(0)) / 2; ext = float((P.max(0) - P.min(0)).max())
    cam = S.look_at(tuple(c + np.array([0.0, 0.0, -3.0 * ext])), tuple(c), (0, 1, 0))
    return S.finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 40.0, 0.01 * ext, 100.0 * ext, 16, 16, 1, S.SAMPLER_SOBOL, 2, name="packet_" + name)


def base_rays(sc, seed):
    """(rays [n, 8] float32 as ox oy oz mint dx dy dz maxt, category [n]); maxt = inf throughout"""
    rng = np.random.default_rng(seed); P = sc.pos[sc.idx.reshape(-1, 3)].astype(np.float64); nt = len(P)
    lo, hi = sc.pos.min(0).astype(np.float64), sc.pos.max(0).astype(np.float64); ext = (hi - lo).max(); m = max(9, 96 // nt * 3)
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rays, cats = [], []

    def emit(o, d, cat, normalise=True):
        o = np.asarray(o, np.float64).reshape(-1, 3); d = np.asarray(d, np.float64).reshape(-1, 3)
        ln = np.linalg.norm(d, axis=1, keepdims=True); ok = ln[:, 0] > 1e-9 * ext
        if normalise: d = d / np.maximum(ln, 1e-30)
        r = np.concatenate([o, np.full((len(o), 1), 1e-4 * ext), d, np.full((len(o), 1), np.inf)], 1)[ok]
        rays.append(r); cats.append(np.full(len(r), CATS.index(cat)))

    def origins(kind, t, n):
        if kind == 0: return lo - 0.2 * ext + rng.random((n, 3)) * (hi - lo + 0.4 * ext)
        if kind == 1: t2 = rng.integers(0, nt, n); return (P[t2] * rng.dirichlet([1, 1, 1], n)[:, :, None]).sum(1)            # ON another surface
        side = P[t, 0] + (P[t, 1] - P[t, 0]) * (rng.random((n, 1)) * 4 - 2) + (P[t, 2] - P[t, 0]) * (rng.random((n, 1)) * 4 - 2)      # (almost) in the target's plane
        return side + nrm[t] * ext * 10.0 ** rng.uniform(-7, -2, (n, 1)) * rng.choice([-1, 1], (n, 1))

    for rep in range(m):
        t = rng.integers(0, nt, nt); w = rng.dirichlet([1, 1, 1], nt); a = rng.random((nt, 1)); e = rng.integers(0, 3, nt); T = P[t]; idx = np.arange(nt)
        targets = dict(vertex=T[idx, rng.integers(0, 3, nt)], edge=T[idx, e] * a + T[idx, (e + 1) % 3] * (1 - a), interior=(T * w[:, :, None]).sum(1),
                       near_edge=T[:, 1] * a + T[:, 2] * (1 - a) + (T[:, 0] - T[:, 1]) * 1e-6 * rng.normal(size=(nt, 1)),
                       in_plane=T[:, 0] + (T[:, 1] - T[:, 0]) * rng.random((nt, 1)) * 3 - (T[:, 2] - T[:, 0]) * rng.random((nt, 1)))
        for cat, target in targets.items():
            o = origins(rep % 3, t, nt); emit(o, target - o, ("surface_origin" if cat == "interior" else cat) if rep % 3 == 1 else ("grazing" if rep % 3 == 2 and cat == "interior" else cat))
        # directions with one / two components exactly zero, through an interior point (float32 origins, so the zero survives the cast)
        target = targets["interior"]
        for zeros, cat in ((1, "one_zero"), (2, "two_zero")):
            d = rng.normal(size=(nt, 3)); z = rng.integers(0, 3, nt); d[idx, z] = 0
            if zeros == 2: d[idx, (z + 1) % 3] = 0
            d /= np.linalg.norm(d, axis=1, keepdims=True); emit((target - d * ext * rng.uniform(0.2, 2, (nt, 1))).astype(f32), d.astype(f32), cat, normalise=False)
    # from both sides onto every centroid along the normal: every triangle index is some ray's closest hit
    cen = P.mean(1)
    for s in (-1.0, 1.0): emit(cen + s * nrm * 0.05 * ext, -s * nrm, "centroid")
    # exactly parallel to an axis-aligned triangle's plane from an origin in it: D = 0 and N = 0 (the NaN path)
    p32 = sc.pos[sc.idx.reshape(-1, 3)]
    for t in range(nt):
        for K in range(3):
            if not (p32[t, :, K] == p32[t, 0, K]).all(): continue
            for rep in range(6):
                o = (lo + rng.random(3) * (hi - lo)).astype(f32); o[K] = p32[t, 0, K]; tgt = (P[t] * rng.dirichlet([1, 1, 1])[:, None]).sum(0)
                d = _unit(np.where(np.arange(3) == K, 0.0, tgt - o + 1e-3)).astype(f32); d[K] = 0
                emit(o, d, "parallel_in_plane", normalise=False)
    return np.concatenate(rays).astype(f32), np.concatenate(cats)


def oracle_results(orc, sc, rays):
    """closest hit and any hit of every ray: hit, tuv (float32), prim (triangle index, -1: miss), occ"""
    n = len(rays); hit = np.zeros(n, bool); tuv = np.zeros((n, 3), f32); prim = np.full(n, -1, np.int64); occ = np.zeros(n, bool)
    first = np.array([s["first_tri"] for s in sc.shapes], np.int64)
    for i in range(n):
        ok, h = orc.intersect(rays[i]); hit[i] = ok
        if ok: tuv[i] = (h[0], h[13], h[14]); prim[i] = first[int(h[19])] + int(h[18])
        occ[i] = orc.occluded(rays[i])
    return dict(hit=hit, tuv=tuv, prim=prim, occ=occ)


def case(mi, oracle, name):
    """dict(sc, rays, cat, ref): the base rays plus, for every fourth base ray that hits, six copies whose maxt / mint is the hit distance or one of its two float
    neighbours; ref holds the oracle's answers for all of them.  Computed once per session and never modified."""
    if name not in _cache:
        sc = scene(mi.scenes, name); orc = oracle.Oracle(sc); rays, cat = base_rays(sc, 1000 + NAMES.index(name))
        ref = oracle_results(orc, sc, rays); sel = np.flatnonzero(ref["hit"])[::4]; extra, ecat = [], []
        for col, cname in ((7, "maxt_at_hit"), (3, "mint_at_hit")):
            for step in (-np.inf, None, np.inf):
                r = rays[sel].copy(); t = ref["tuv"][sel, 0]; r[:, col] = t if step is None else np.nextafter(t, f32(step)); extra.append(r); ecat.append(np.full(len(r), CATS.index(cname)))
        rays2 = np.concatenate([rays] + extra); ref2 = oracle_results(orc, sc, rays2[len(rays):])
        for v in (rays2, cat): v.setflags(write=False)
        _cache[name] = dict(sc=sc, rays=rays2, cat=np.concatenate([cat] + ecat), ref={k: np.concatenate([ref[k], ref2[k]]) for k in ref})
    return _cache[name]
