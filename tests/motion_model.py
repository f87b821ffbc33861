"""The prevPosition / motion field channels (include/mi355pt.h, csrc/kernels_field.hip) as a NumPy model: float32, one rounding per operation, in the order of the
definition, so that the device result can be compared bit for bit.  A scene state is a dict `pos` [n_verts, 3], `to_world` [n_instances, 3, 4] (rows 0..2 of every
instance's transform), `w2p` (the 12 floats of mi_scene_world_to_pixel) and `origin` (the camera origin); `idx` [n_tris, 3] does not change.  Records are what the
intersection of every sample's camera ray with the CURRENT scene gave: hit, instance (-1: none), prim, u, v, P.

Also the census scene of the tests: a sheet of which half the vertices move, a crate (shape group) placed twice with one placement moved and one member vertex
deformed, a sphere and the sky -- and the edit that makes the "after" state."""
import numpy as np

f32 = np.float32
CLASSES = ("moved_mesh", "unmoved_mesh", "moved_instance", "deformed_member", "static_instance", "analytic", "miss")


def bary(c0, c1, c2, u, v):
    """(c0 b.x + c1 b.y) + c2 b.z per component with b = ((1 - u) - v, u, v)"""
    u = np.asarray(u, f32)[:, None]; v = np.asarray(v, f32)[:, None]; bx = (f32(1.0) - u) - v
    return (np.asarray(c0, f32) * bx + np.asarray(c1, f32) * u) + np.asarray(c2, f32) * v


def xf_point(m, p):
    """rows 0..2 of an affine matrix (m [n, 3, 4]) on points p [n, 3]: ((m0 x + m1 y) + m2 z) + m3 per row"""
    m = np.asarray(m, f32); x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    return ((m[:, :, 0] * x + m[:, :, 1] * y) + m[:, :, 2] * z) + m[:, :, 3]


def project(M, q):
    """X, Y, Wc of the points q [n, 3] under the 12 floats M, each ((M0 x + M1 y) + M2 z) + M3"""
    M = np.asarray(M, f32).reshape(12); x, y, z = q[:, 0], q[:, 1], q[:, 2]
    return tuple(((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3] for r in range(3))


def distance(q, origin):
    e = q - np.asarray(origin, f32).reshape(1, 3)
    return np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])


def prev_position(idx, prev, cur, rec):
    """prevPosition of every record (misses: P as given; the caller puts `undefined` there)"""
    n_tris = len(idx); hit = np.asarray(rec["hit"], bool); inst = np.asarray(rec["inst"], np.int64); prim = np.asarray(rec["prim"], np.int64)
    P = np.asarray(rec["p"], f32); out = P.copy()
    tri = hit & ((inst >= 0) | (prim < n_tris))      # through an instance `prim` is the member triangle; outside, prim >= n_tris is an analytic shape: P
    t = np.nonzero(tri)[0]
    if len(t) == 0: return out
    c = np.asarray(idx, np.int64)[prim[t]]; u = rec["u"][t]; v = rec["v"][t]
    bcur = bary(cur["pos"][c[:, 0]], cur["pos"][c[:, 1]], cur["pos"][c[:, 2]], u, v)
    bprev = bary(prev["pos"][c[:, 0]], prev["pos"][c[:, 1]], prev["pos"][c[:, 2]], u, v)
    through = inst[t] >= 0
    if through.any():
        k = inst[t][through]
        bcur[through] = xf_point(cur["to_world"][k], bcur[through]); bprev[through] = xf_point(prev["to_world"][k], bprev[through])
    out[t] = P[t] + (bprev - bcur)
    return out.astype(f32)


def motion(prev, cur, P, Q):
    """(values [n, 3], defined [n]): (Xprev - Xcur, Yprev - Ycur, dprev - dcur); not defined where a projection's Wc is not positive"""
    with np.errstate(all="ignore"):
        Xp, Yp, Wp = project(prev["w2p"], Q); Xc, Yc, Wc = project(cur["w2p"], P)
        val = np.stack([Xp / Wp - Xc / Wc, Yp / Wp - Yc / Wc, distance(Q, prev["origin"]) - distance(P, cur["origin"])], 1).astype(f32)
    return val, (Wp > 0) & (Wc > 0)


def fields(idx, prev, cur, rec, undefined=(0.0, 0.0, 0.0)):
    """name -> [n, 3] of position, prevPosition, motion; a miss gets `undefined`, and so does a motion that is not defined"""
    hit = np.asarray(rec["hit"], bool); P = np.asarray(rec["p"], f32); und = np.asarray(undefined, f32).reshape(1, 3)
    Q = prev_position(idx, prev, cur, rec); mv, ok = motion(prev, cur, P, Q)
    return {"position": np.where(hit[:, None], P, und).astype(f32), "prevPosition": np.where(hit[:, None], Q, und).astype(f32),
            "motion": np.where((hit & ok)[:, None], mv, und).astype(f32)}


def classify(sc, prev, cur, rec):
    """name -> boolean [n] over CLASSES, from the tables alone: which vertices and transforms the edit changed"""
    idx = np.asarray(sc.idx, np.int64); n_tris = len(idx); hit = np.asarray(rec["hit"], bool); inst = np.asarray(rec["inst"], np.int64); prim = np.asarray(rec["prim"], np.int64)
    vmoved = (prev["pos"].view(np.uint32) != cur["pos"].view(np.uint32)).any(1); tmoved = vmoved[idx].any(1)
    imoved = (prev["to_world"].view(np.uint32) != cur["to_world"].view(np.uint32)).reshape(len(cur["to_world"]), -1).any(1) if len(cur["to_world"]) else np.zeros(0, bool)
    shape_moved = np.zeros(len(sc.shapes), bool)
    for si, s in enumerate(sc.shapes): shape_moved[si] = tmoved[s["first_tri"]:s["first_tri"] + s["tri_count"]].any()
    through = hit & (inst >= 0); plain = hit & (inst < 0) & (prim < n_tris); safe = np.where(through | plain, prim, 0); ki = np.where(through, inst, 0)
    return {"moved_mesh": plain & tmoved[safe], "unmoved_mesh": plain & ~tmoved[safe] & shape_moved[np.asarray(sc.tri_shape, np.int64)[safe]],
            "moved_instance": through & ~tmoved[safe] & (imoved[ki] if len(imoved) else False), "deformed_member": through & tmoved[safe],
            "static_instance": through & ~tmoved[safe] & ~(imoved[ki] if len(imoved) else False), "analytic": hit & (inst < 0) & (prim >= n_tris), "miss": ~hit}


# ---------------------------------------------------------------------------------------------- camera states
def world_to_pixel64(sc):
    """mi_scene_world_to_pixel's definition in float64, rounded once (the library's own elimination may differ in the last bit: device tests take Scene.world_to_pixel)"""
    full = np.diag([sc.width, sc.height, 1.0, 1.0]) @ np.linalg.inv(np.asarray(sc.sample_to_camera, np.float64)) @ np.linalg.inv(np.asarray(sc.cam_to_world, np.float64))
    return full[[0, 1, 3]].astype(f32).reshape(12)


def state(sc, w2p=None):
    """the scene state a mark snapshots, from a scene description"""
    tw = np.stack([np.asarray(i["to_world"], f32)[:3] for i in sc.instances]) if sc.instances else np.zeros((0, 3, 4), f32)
    return dict(pos=np.asarray(sc.pos, f32).copy(), to_world=np.ascontiguousarray(tw, f32), w2p=world_to_pixel64(sc) if w2p is None else np.asarray(w2p, f32).reshape(12).copy(),
                origin=np.asarray(sc.cam_to_world, f32)[:3, 3].copy())


# ---------------------------------------------------------------------------------------------- the census scene
W, H = 32, 24


def census_scene(S, width=W, height=H, spp=1, filter_kind=None):
    """A 9 x 7-vertex sheet y = 0 over x in [-4, 4], z in [-2, 4] (plain mesh, shared vertices); a crate 2 x 1.2 x 2 (shape group 0, six quads) placed at x = -2.1 and at
    x = +2.1; a sphere of radius 0.7 between them; a light out of view; sky above the horizon.  Independent sampler, so that sample 0 of a pixel is one camera ray."""
    b = S._Builder(); grey = b.bsdf(reflectance=(0.5, 0.5, 0.45)); wood = b.bsdf(reflectance=(0.5, 0.33, 0.18)); ball = b.bsdf(reflectance=(0.3, 0.4, 0.7)); lightm = b.bsdf(reflectance=(0.5, 0.5, 0.5))
    b.begin(); base = len(b.verts); nx, nz = 9, 7
    for j in range(nz):
        for i in range(nx): b.verts.append((-4.0 + i, 0.0, -2.0 + j))
    for j in range(nz - 1):
        for i in range(nx - 1):
            a = base + j * nx + i; b.tris.append((a, a + nx, a + 1)); b.tris.append((a + 1, a + nx, a + nx + 1))
    b.end(grey)
    b.begin(); b.quad([(1, 9, -1), (1, 9, 1), (-1, 9, 1), (-1, 9, -1)]); b.end(lightm, radiance=(20.0, 20.0, 20.0))
    x0, x1, y0, y1, z0, z1 = -1.0, 1.0, 0.0, 1.2, -1.0, 1.0
    b.begin()
    for q in ([(x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)], [(x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)], [(x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)],
              [(x1, y0, z1), (x1, y1, z1), (x0, y1, z1), (x0, y0, z1)], [(x0, y0, z1), (x0, y1, z1), (x0, y1, z0), (x0, y0, z0)]): b.quad(q)
    b.end(wood, group=1)
    b.add_analytic(S.SHAPE_SPHERE, S.translate(0.0, 0.7, 0.6), ball, radius=0.7)
    inst = [S.make_instance(0, S.translate(-2.1, 0.0, 0.8) @ S.rotate((0, 1, 0), 20.0)), S.make_instance(0, S.translate(2.1, 0.0, 0.8) @ S.rotate((0, 1, 0), -15.0))]
    cam = S.look_at((0.0, 3.4, -6.0), (0.0, 0.9, 0.8), (0, 1, 0))
    sc = S.finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 64.0, 0.05, 100.0, width, height, spp, S.SAMPLER_INDEPENDENT, 4,
                        filter_kind=S.FILTER_BOX if filter_kind is None else filter_kind, name="motion_census", analytic=b.resolve_analytic(), instances=inst)
    return S.add_scene_emitters(sc, [S.constant_emitter((0.3, 0.35, 0.45))])


def census_edit(S, sc, step=1.0):
    """(pos, instances, cam_to_world) of the edited scene: the sheet's vertices with x > 0 rise in a wave; the first vertex of the crate's lid rises by 0.5 (a member
    vertex: both placements show it); the placement at +x turns by 25 degrees and shifts; the camera moves sideways and turns with its target.  step scales all of it."""
    pos = np.asarray(sc.pos, f32).copy(); s0 = sc.shapes[0]; v = slice(s0["first_vert"], s0["first_vert"] + s0["vert_count"]); sheet = pos[v]
    lift = (0.25 * step * (1.0 + np.sin(2.0 * sheet[:, 0] + sheet[:, 2]))).astype(f32); sheet[:, 1] = np.where(sheet[:, 0] > 0, sheet[:, 1] + lift + f32(0.05 * step), sheet[:, 1]); pos[v] = sheet
    crate = sc.shapes[2]; pos[crate["first_vert"], 1] += f32(0.5 * step)
    insts = [sc.instances[0], S.make_instance(0, S.translate(2.1 + 0.3 * step, 0.0, 0.8 + 0.2 * step) @ S.rotate((0, 1, 0), -15.0 + 25.0 * step))]
    cam = S.look_at((0.4 * step, 3.4, -6.0), (0.1 * step, 0.9, 0.8), (0, 1, 0))
    return pos, insts, np.ascontiguousarray(cam, f32)


def edited(S, sc, step=1.0):
    """a copy of the description with census_edit applied"""
    pos, insts, cam = census_edit(S, sc, step); out = S.Scene(sc); out.pos = pos; out.instances = insts; out.cam_to_world = cam
    return out


def pixel_samples(sc, k=0):
    """one explicit sample per pixel: (px, py, k), row-major"""
    yy, xx = np.meshgrid(np.arange(sc.height), np.arange(sc.width), indexing="ij")
    return np.stack([xx.ravel(), yy.ravel(), np.full(xx.size, k)], 1).astype(np.uint32)


def oracle_records(orc, pairs):
    """the oracle's intersection record of every sample's camera ray: film position -> camera ray -> Scene::rayIntersect; also the rays and the film positions.
    The oracle names a triangle by (shape, index within the shape) and an analytic shape by a shape index past the meshes: `prim` is the library's global index."""
    sc = orc.sc; first = [s["first_tri"] for s in sc.shapes]; n_tris = len(sc.idx)
    pos = orc.render_samples(pairs)["pos"]; n = len(pairs)
    rec = dict(hit=np.zeros(n, bool), inst=np.full(n, -1, np.int64), prim=np.zeros(n, np.int64), u=np.zeros(n, f32), v=np.zeros(n, f32), p=np.zeros((n, 3), f32), ng=np.zeros((n, 3), f32))
    rays = np.zeros((n, 8), f32)
    for i in range(n):
        rays[i] = orc.camera_ray(float(pos[i, 0]), float(pos[i, 1])); ok, o = orc.intersect(rays[i])
        if not ok: continue
        shape = int(o[19]); rec["hit"][i] = True; rec["inst"][i] = int(o[20]); rec["u"][i] = o[13]; rec["v"][i] = o[14]; rec["p"][i] = o[1:4]; rec["ng"][i] = o[4:7]
        rec["prim"][i] = first[shape] + int(o[18]) if shape < len(first) else n_tris + (shape - len(first))
    return rec, rays, pos
