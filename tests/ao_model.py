"""Reference model of the ambient-occlusion integrator: AmbientOcclusionIntegrator::Li (src/integrators/direct/ao.cpp:84-125) restated in Python, float32 arithmetic
in the reference's operation order, composed ONLY from units the oracle exports and has pinned against the reference:

    orc_sobol_look_up / orc_sobol_sample   the sampler (src/samplers/sobol.cpp:171-250: the one 2-D array at dimensions 5 / 6, or next2D on the sample's own index)
    orc_camera_ray, orc_ray_intersect      camera ray and hit record (p, shading normal, s; t = n x s as Frame builds it)
    orc_warp                               warp::squareToCosineHemisphere
    orc_ray_occluded                       Scene::rayIntersect(shadowRay) with mint = Epsilon, maxt = rayLength

The array rule is DirectModel._array of tests/direct_model.py, taken by import.  No vectors compiled from the reference pin this integrator (the reference build used as
a checker holds no `ao` plugin): the model is the yardstick, like the ones of `thinlens` and `direct`.  It serves the Sobol' sampler and the perspective camera."""
import ctypes as C
import numpy as np
import oracle.binding as _binding
from tests.direct_model import DirectModel

f32 = np.float32
EPSILON = f32(1e-4)


def _cross(a, b):
    return np.array([f32(a[1] * b[2]) - f32(a[2] * b[1]), f32(a[2] * b[0]) - f32(a[0] * b[2]), f32(a[0] * b[1]) - f32(a[1] * b[0])], f32)


def auto_ray_length(sc):
    """ao.cpp:77-80: scene->getAABB().getBSphere().radius * 0.5f in float32, from the scene arrays.  Scene::initializeBidirectional (scene.cpp:394-421): the kd-tree box --
    the union of the shapes' boxes, enlarged by gkdtree.h:1213-1220 -- expanded by the sensor's position and by the emitters with a position; AABB::getBSphere
    (aabb.cpp:44-47): centre (max + min) * 0.5, radius |centre - max|.  Mesh scenes without instances or analytic shapes (the scenes the tests hand it)."""
    assert not (sc.get("instances") or sc.get("analytic"))
    pos = np.asarray(sc.pos, f32).reshape(-1, 3); lo = pos.min(0).astype(f32); hi = pos.max(0).astype(f32); eps = f32(1e-3)
    lo = (lo - ((hi - lo) * eps + eps)).astype(f32); hi = (hi + ((hi - lo) * eps + eps)).astype(f32)
    pts = [np.asarray(sc.cam_to_world, f32).reshape(4, 4)[:3, 3]]
    pts += [np.asarray(e["to_world"], f32).reshape(4, 4)[:3, 3] for e in sc.emitters if e["type"] in (3, 4, 7)]      # point, spot, collimated
    for p in pts: lo = np.minimum(lo, p); hi = np.maximum(hi, p)
    d = ((hi + lo) * f32(0.5) - hi).astype(f32); d2 = f32(0)
    for i in range(3): d2 = f32(d2 + f32(d[i] * d[i]))
    return f32(np.sqrt(d2) * f32(0.5))


class AoModel:
    def __init__(self, oracle_module, sc, shading_samples=1, ray_length=-1.0):
        assert sc.sampler == 1 and shading_samples >= 1 and not float(sc.get("aperture_radius", 0.0) or 0.0)
        self.sc = sc; self.orc = oracle_module.Oracle(sc); self.L = _binding.lib(); self.N = int(shading_samples)
        self.ray_length = f32(ray_length) if ray_length >= 0 else auto_ray_length(sc)
        self.recip = f32(1) / f32(self.N)                 # Spectrum::operator/= (spectrum.h:447-456): recip = 1.0f / f, then one multiplication
        r = max(sc.width, sc.height); p = 1; l = 0
        while p < r: p <<= 1; l += 1
        self.log_res = l
        self.array_dim = 5                                # sobol.cpp:171-178: the first (and only) 2-D array

    _sobol = DirectModel._sobol
    _look_up = DirectModel._look_up
    _array = DirectModel._array                           # sobol.cpp:189-197 + sampler.cpp:83-90

    def samples2d(self, px, py, m):
        """the 2-D samples of pixel-sample m: the array, or nextSample2D on the sample's own index (dimensions 2 / 3 after the pixel offset)"""
        if self.N > 1: return self._array(px, py, m, self.N, self.array_dim)
        idx = self._look_up(m, px, py)
        return [(self._sobol(idx, 2), self._sobol(idx, 3))]

    def li(self, px, py, m, pos):
        """-> (Li float32, closest-hit rays cast, shadow rays cast, the per-ray visibility list or None on a camera miss)"""
        orc, L = self.orc, self.L
        ray = orc.camera_ray(float(pos[0]), float(pos[1]))
        ok, h = orc.intersect(ray)
        if not ok: return f32(1), 1, 0, None              # ao.cpp:91-95
        p = h[1:4].copy(); ns = h[7:10].copy(); s = h[10:13].copy(); tt = _cross(ns, s)
        count = f32(0); vis = []
        for sx, sy in self.samples2d(px, py, m):
            w = np.zeros(7, f32); L.orc_warp(C.c_float(sx), C.c_float(sy), w.ctypes.data)
            d = ((s * w[0] + tt * w[1]) + ns * w[2]).astype(f32)      # its.toWorld: the shading frame (frame.h: s * v.x + t * v.y + n * v.z)
            free = not orc.occluded(np.concatenate([p, [EPSILON], d, [self.ray_length]]).astype(f32))
            if free: count = f32(count + f32(1))
            vis.append(free)
        return f32(count * self.recip), 1, len(vis), vis

    def render_samples(self, pairs):
        """pairs: uint32 [n, 3] = (px, py, sample index) -> dict(li [n, 3], rays, shadow_rays, hit [n] bool, visible [n, N] bool (False on misses))"""
        pairs = np.ascontiguousarray(pairs, np.uint32); pos = self.orc.render_samples(pairs)["pos"]
        li = np.zeros((len(pairs), 3), f32); hit = np.zeros(len(pairs), bool); visible = np.zeros((len(pairs), self.N), bool); rays = shadow = 0
        for i, (px, py, m) in enumerate(pairs.tolist()):
            v, r, s, vis = self.li(px, py, m, pos[i]); li[i] = v; rays += r; shadow += s
            if vis is not None: hit[i] = True; visible[i] = vis
        return dict(li=li, rays=rays, shadow_rays=shadow, hit=hit, visible=visible)
