"""Synthetic scene generators + the flattened-scene container ("mi_scene" boundary content).

The reference ships no cbox.xml / Veach-MIS / Sponza assets, so every BASELINE
scene is generated here, deterministically, as the flattened arrays the C-ABI consumes
(include/mi355pt.h) -- the same content an adapter would pull out of a live mitsuba::Scene
(TriMesh::getTriangles/getVertexPositions/..., reference include/mitsuba/render/trimesh.h:122-160).

`save_scene` writes the arrays in a small binary container ("MISCENE2") that the oracle-side
harness (oracle/ref_build/harness.cpp) reads to build the very same scene inside the reference.
"""
import math
import struct
import numpy as np

BSDF_DIFFUSE = 0
BSDF_ROUGHCONDUCTOR = 1
BSDF_CONDUCTOR = 2        # src/bsdfs/conductor.cpp: eta, k, specular
BSDF_DIELECTRIC = 3       # src/bsdfs/dielectric.cpp: eta[0] = intIOR / extIOR, specular = specularReflectance, reflectance = specularTransmittance
BSDF_ROUGHDIELECTRIC = 5  # src/bsdfs/roughdielectric.cpp: alpha, distr, eta[0], specular = specularReflectance, reflectance = specularTransmittance
BSDF_DIFFTRANS = 6        # src/bsdfs/difftrans.cpp: reflectance = transmittance
BSDF_ROUGHPLASTIC = 7     # src/bsdfs/roughplastic.cpp: alpha, distr, eta[0], specular, reflectance = diffuseReflectance, k = (Tdiff_int, table offset, table length)
BSDF_THINDIELECTRIC = 8   # src/bsdfs/thindielectric.cpp: eta[0] = intIOR / extIOR, specular = specularReflectance, reflectance = specularTransmittance
BSDF_MASK = 9             # src/bsdfs/mask.cpp: reflectance = opacity (constant or textured), distr = index of the nested material record (an earlier one)
BSDF_MIXTURE = 10         # src/bsdfs/mixturebsdf.cpp: distr = number of children (2..4); their material indices in reflectance[0..2], eta[0] (as numbers), weights in k[0..2], specular[0]
BSDF_BUMPMAP = 11         # src/bsdfs/bumpmap.cpp: distr = index of the nested material record, bound texture = the displacement, alpha = factor of an enclosing `scale` texture
BSDF_NULL = 13            # src/bsdfs/null.cpp: index-matched boundary of a participating medium (passes straight through, ENull)
BSDF_ROUGHDIFFUSE = 14     # src/bsdfs/roughdiffuse.cpp (Oren-Nayar): reflectance, alpha (roughness, averaged over the channels there), distr = useFastApprox
BSDF_PHONG = 15            # src/bsdfs/phong.cpp: reflectance = diffuseReflectance, specular = specularReflectance, alpha = exponent, k[0] = specular sampling weight
BSDF_WARD = 16             # src/bsdfs/ward.cpp: as phong, alpha = alphaU, k[1] = alphaV, distr = variant (WARD_*)
WARD_WARD, WARD_DUER, WARD_BALANCED = 0, 1, 2
BSDF_COATING = 17          # src/bsdfs/coating.cpp: distr = nested record, eta[0] = intIOR / extIOR, alpha = thickness, reflectance = sigmaA, specular = specularReflectance
BSDF_BLEND = 18            # src/bsdfs/blendbsdf.cpp: eta[0..1] = the two child records, reflectance = (w, w, w) or the value of the bound `weight` texture
BSDF_ROUGHCOATING = 19     # src/bsdfs/roughcoating.cpp: distr = nested record, eta = (intIOR / extIOR, thickness, microfacet distribution), alpha, reflectance = sigmaA, specular, k[1..2] = transmittance slice
BSDF_NORMALMAP = 12       # src/bsdfs/normalmap.cpp: distr = nested record, bound texture = the tangent-space normals
BSDF_PLASTIC = 4          # src/bsdfs/plastic.cpp: eta[0], specular, reflectance = diffuseReflectance, k[0] = fdrInt, nonlinear
EMITTER_AREA = 0
EMITTER_ENVMAP = 1
EMITTER_CONSTANT = 2      # src/emitters/constant.cpp
EMITTER_POINT = 3         # src/emitters/point.cpp
EMITTER_SPOT = 4          # src/emitters/spot.cpp
EMITTER_DIRECTIONAL = 5   # src/emitters/directional.cpp
EMITTER_COLLIMATED = 7    # src/emitters/collimated.cpp (6: the compound sunsky of scene files)
FILTER_BOX = 0
FILTER_GAUSSIAN = 1
FILTER_TENT = 2
FILTER_MITCHELL = 3        # B in filter_radius, C in filter_stddev
FILTER_CATMULLROM = 4
FILTER_LANCZOS = 5         # lobes in filter_radius
SAMPLER_INDEPENDENT = 0
SAMPLER_SOBOL = 1
DISTR_BECKMANN = 0
DISTR_GGX = 1
DISTR_PHONG = 2            # isotropic: Phong; anisotropic: Ashikhmin-Shirley (src/bsdfs/microfacet.h:214-221); roughconductor only
SHAPE_RECTANGLE = 0
SHAPE_DISK = 1
SHAPE_SPHERE = 2
SHAPE_CYLINDER = 3

f32 = np.float32


class Scene(dict):
    """Plain dict of numpy arrays / scalars; attribute access for convenience."""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def _quad(verts, tris, shape_ranges, quad_pts):
    base = len(verts)
    verts.extend(quad_pts)
    tris.append((base, base + 1, base + 2))
    tris.append((base, base + 2, base + 3))


def fresnel_dielectric_ext(cos_i, eta):
    """reference src/libcore/util.cpp:653-683 (float64, vectorised over cos_i >= 0)."""
    cos_i = np.asarray(cos_i, np.float64); scale = 1.0 / eta
    ct2 = 1.0 - (1.0 - cos_i * cos_i) * scale * scale
    ct = np.sqrt(np.maximum(ct2, 0.0))
    rs = (cos_i - eta * ct) / (cos_i + eta * ct); rp = (eta * cos_i - ct) / (eta * cos_i + ct)
    return np.where(ct2 <= 0.0, 1.0, 0.5 * (rs * rs + rp * rp))


def fresnel_diffuse_reflectance(eta):
    """fresnelDiffuseReflectance(eta, fast=false) = integral_0^1 F(sqrt(xi), eta) dxi (src/libcore/util.cpp:809-861; the reference runs an
    adaptive Gauss-Lobatto rule to 1e-5).  Substituting xi = c^2: integral_0^1 2 c F(c) dc, composite Gauss-Legendre; pinned against the
    reference's own values in tests/golden/fresnel_diffuse_reflectance.npy."""
    x, w = np.polynomial.legendre.leggauss(64); total = 0.0; n = 256
    for i in range(n):
        a, b = i / n, (i + 1) / n; c = 0.5 * (b - a) * x + 0.5 * (b + a)
        total += 0.5 * (b - a) * np.sum(w * 2.0 * c * fresnel_dielectric_ext(c, eta))
    return float(total)


_RT_SLICES = None


def rough_transmittance_slice(distr, ior, alpha):
    """RoughPlastic::configure's rough-transmittance data for (distribution, eta, alpha): the reference's own slices of data/microfacet/*.dat
    (setEta + setAlpha -> 100 values over the warped incidence angle; internal diffuse transmittance), dumped by oracle/_ref/harness `tables`
    into mitsuba-im_amd/data/rough_transmittance_slices.npy for a grid of parameters.  Returns (Tdiff_int, table[100])."""
    global _RT_SLICES
    if _RT_SLICES is None:
        import os
        _RT_SLICES = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "rough_transmittance_slices.npy"))
    for row in _RT_SLICES:
        if int(row[0]) == int(distr) and row[1] == f32(ior) and row[2] == f32(alpha):
            return float(row[3]), np.ascontiguousarray(row[4:], f32)
    raise ValueError("no rough-transmittance slice for distr=%s ior=%s alpha=%s (extend the grid in oracle/ref_build/harness.cpp modeTables)" % (distr, ior, alpha))


INTEGRATOR_PATH = 0            # src/integrators/path/path.cpp
INTEGRATOR_VOLPATH_SIMPLE = 1  # src/integrators/path/volpath_simple.cpp
INTEGRATOR_VOLPATH = 2         # src/integrators/path/volpath.cpp (multiple importance sampling, emitters found through index-matched boundaries)
INTEGRATOR_DIRECT = 3          # src/integrators/direct/direct.cpp (scene keys emitter_samples / bsdf_samples, default 1 each)
INTEGRATOR_AO = 4              # src/integrators/direct/ao.cpp (scene keys shading_samples, default 1, and ray_length, default -1 = automatic)
MEDIUM_BALANCE, MEDIUM_SINGLE, MEDIUM_MANUAL = 0, 1, 2      # HomogeneousMedium sampling strategies (homogeneous.cpp:192-226; `maximum` is not built)
PHASE_ISOTROPIC, PHASE_HG = 0, 1


def make_medium(sigma_a, sigma_s, strategy=MEDIUM_BALANCE, phase=PHASE_ISOTROPIC, g=0.0, medium_sampling_weight=None, sampling_density=None, channel=None):
    """`homogeneous` medium (src/medium/homogeneous.cpp) with an `isotropic` / `hg` phase function.  sigma_a / sigma_s are the final coefficients (the reference's
    `scale` and material presets are folded in by the caller).  The derived sampling parameters follow the constructor (homogeneous.cpp:168-222) in float arithmetic."""
    sa = np.asarray(sigma_a, f32); ss = np.asarray(sigma_s, f32); st = (sa + ss).astype(f32)
    w = -1.0 if medium_sampling_weight is None else float(medium_sampling_weight)
    if w == -1.0:
        w = f32(-1.0)
        for i in range(3):
            albedo = f32(ss[i] / st[i]) if st[i] != 0 else f32(np.inf)
            if albedo > w and st[i] != 0: w = albedo
        if w > 0: w = max(w, f32(0.5))
        w = float(w)
    density = 0.0
    if strategy == MEDIUM_SINGLE:
        ch = int(np.argmin(st)) if channel is None else int(channel)         # the first smallest sigma_t (strict < in the reference's loop)
        density = float(st[ch])
    elif strategy == MEDIUM_MANUAL:
        density = float(f32(sampling_density))
    return dict(sigma_a=tuple(map(float, sa)), sigma_s=tuple(map(float, ss)), strategy=int(strategy), sampling_density=density, medium_sampling_weight=float(f32(w)),
                phase=int(phase), g=float(f32(g)))


def make_bsdf(kind=BSDF_DIFFUSE, reflectance=(0.5, 0.5, 0.5), twosided=False, alpha=0.1,
              distr=DISTR_BECKMANN, eta=(0.0, 0.0, 0.0), k=(1.0, 1.0, 1.0),
              specular=(1.0, 1.0, 1.0), sample_visible=True, ior=1.5046, nonlinear=False, alpha_v=None, nested=None, weights=None, texture=-1, scale=1.0):
    if kind == BSDF_NULL:
        reflectance = (0.0, 0.0, 0.0)
    if kind == BSDF_MASK:
        distr = int(nested)                           # reflectance = opacity
    if kind in (BSDF_BUMPMAP, BSDF_NORMALMAP):        # wrapper around record `nested`; `texture` = displacement / normal map, `scale` = ScaleTexture factor (bumpmap)
        d = dict(type=kind, twosided=0, distr=int(nested), sample_visible=0, nonlinear=0, table=None, texture=int(texture), aniso=0,
                 reflectance=(0.0, 0.0, 0.0), alpha=float(scale), eta=(0.0, 0.0, 0.0), k=(0.0, 0.0, 0.0), specular=(0.0, 0.0, 0.0))
        return d
    if kind == BSDF_ROUGHCOATING:                     # rough dielectric layer over record `nested`; `distr` = its microfacet distribution, alpha = its roughness, scale = thickness
        if distr == DISTR_PHONG: sample_visible = False
        _, table = rough_transmittance_slice(distr, ior, alpha)
        return dict(type=kind, twosided=int(twosided), distr=int(nested), sample_visible=int(bool(sample_visible)), nonlinear=0, table=table, texture=-1, aniso=0,
                    reflectance=tuple(map(float, reflectance)), alpha=float(alpha), eta=(float(f32(ior)), float(scale), float(distr)), k=(0.0, 0.0, float(len(table))), specular=tuple(map(float, specular)))
    if kind == BSDF_COATING:                          # smooth dielectric layer over record `nested`; reflectance = sigmaA (absorption per unit thickness), scale = thickness
        return dict(type=kind, twosided=int(twosided), distr=int(nested), sample_visible=0, nonlinear=0, table=None, texture=-1, aniso=0,
                    reflectance=tuple(map(float, reflectance)), alpha=float(scale), eta=(float(f32(ior)), 0.0, 0.0), k=(0.0, 0.0, 0.0), specular=tuple(map(float, specular)))
    if kind == BSDF_BLEND:                            # children = `nested` (two earlier records), weight = `alpha` (constant) or the bound texture
        if len(nested) != 2: raise ValueError("blendbsdf: BSDF count mismatch: expected two nested BSDF instances!")
        w = float(f32(alpha))
        return dict(type=kind, twosided=int(twosided), distr=0, sample_visible=0, nonlinear=0, table=None, texture=int(texture), aniso=0,
                    reflectance=(w, w, w), alpha=0.0, eta=(float(int(nested[0])), float(int(nested[1])), 0.0), k=(0.0, 0.0, 0.0), specular=(0.0, 0.0, 0.0))
    if kind == BSDF_MIXTURE:                          # children = `nested` (list of 2..4 earlier records), `weights` as given (rescaled by the BSDF itself when they sum to > 1)
        ch = [float(int(c)) for c in nested] + [0.0] * (4 - len(nested)); w = [float(f32(x)) for x in weights] + [0.0] * (4 - len(weights))
        if not (2 <= len(nested) <= 4) or len(nested) != len(weights): raise ValueError("mixturebsdf: 2..4 children with one weight each")
        return dict(type=kind, twosided=int(twosided), distr=len(nested), sample_visible=0, nonlinear=0, table=None, texture=-1, aniso=0,
                    reflectance=tuple(ch[:3]), alpha=0.0, eta=(ch[3], 0.0, 0.0), k=tuple(w[:3]), specular=(w[3], 0.0, 0.0))
    if kind == BSDF_ROUGHDIELECTRIC:
        eta = (float(f32(ior)), 0.0, 0.0)
    if kind == BSDF_ROUGHDIFFUSE:
        distr = 1 if distr else 0; sample_visible = False     # distr = useFastApprox
    if kind == BSDF_WARD:                             # distr = variant; alpha / alpha_v = alphaU / alphaV; k[0] as for phong (ward.cpp:160-164)
        lum = lambda c: f32(f32(f32(f32(c[0]) * f32(0.212671)) + f32(f32(c[1]) * f32(0.715160))) + f32(f32(c[2]) * f32(0.072169)))
        if max(float(f32(a) + f32(b)) for a, b in zip(reflectance, specular)) > 1.0: raise ValueError("ward: diffuseReflectance + specularReflectance > 1 (the reference rescales both, BSDF::ensureEnergyConservation): not implemented")
        d_avg, s_avg = lum(reflectance), lum(specular); k = (float(f32(s_avg / f32(d_avg + s_avg))), float(f32(alpha if alpha_v is None else alpha_v)), 0.0); sample_visible = False
        if distr not in (0, 1, 2): raise ValueError("ward: variant 0 (ward), 1 (ward-duer) or 2 (balanced)")
    if kind == BSDF_PHONG:                            # alpha = exponent; k[0] = m_specularSamplingWeight (phong.cpp:104-108), float arithmetic as in Spectrum::getLuminance (spectrum.h:725-727)
        lum = lambda c: f32(f32(f32(f32(c[0]) * f32(0.212671)) + f32(f32(c[1]) * f32(0.715160))) + f32(f32(c[2]) * f32(0.072169)))
        if max(float(f32(a) + f32(b)) for a, b in zip(reflectance, specular)) > 1.0: raise ValueError("phong: diffuseReflectance + specularReflectance > 1 (the reference rescales both, BSDF::ensureEnergyConservation): not implemented")
        d_avg, s_avg = lum(reflectance), lum(specular); k = (float(f32(s_avg / f32(d_avg + s_avg))), 0.0, 0.0); distr = 0; sample_visible = False
    table = None
    if kind == BSDF_ROUGHPLASTIC:
        eta = (float(f32(ior)), 0.0, 0.0); tdiff, table = rough_transmittance_slice(distr, ior, alpha); k = (tdiff, 0.0, float(len(table)))
    if kind == BSDF_THINDIELECTRIC:
        eta = (float(f32(ior)), 0.0, 0.0)
    if kind in (BSDF_DIELECTRIC, BSDF_PLASTIC):      # scalar relative index; plastic: k[0] = m_fdrInt = fresnelDiffuseReflectance(1 / eta) (plastic.cpp:200)
        eta = (float(f32(ior)), 0.0, 0.0); distr = int(nonlinear)
        k = (float(f32(fresnel_diffuse_reflectance(1.0 / float(f32(ior))))), 0.0, 0.0) if kind == BSDF_PLASTIC else (0.0, 0.0, 0.0)
    if kind == BSDF_ROUGHPLASTIC:
        if distr == DISTR_PHONG: sample_visible = False      # microfacet.h:141-145
        sample_visible = (1 if sample_visible else 0) | (2 if nonlinear else 0)      # container field: bit 0 sampleVisible, bit 1 the nonlinear flag of roughplastic (read by the harness)
    aniso = 0
    if kind == BSDF_WARD and k[1] != float(f32(alpha)):
        aniso = 1                                      # EAnisotropic (ward.cpp:143-145): the shape then needs texture coordinates (tangents)
    if kind in (BSDF_ROUGHCONDUCTOR, BSDF_ROUGHDIELECTRIC):
        if distr == DISTR_PHONG:
            sample_visible = False                     # microfacet.h:141-145: the Phong / Ashikhmin-Shirley distribution samples all normals
        if alpha_v is not None and float(f32(alpha_v)) != float(f32(alpha)):
            aniso = 1                                  # anisotropic roughness (flags bit3): alphaV travels in reflectance[0] (roughconductor) / k[0] (roughdielectric)
            if kind == BSDF_ROUGHCONDUCTOR: reflectance = (float(f32(alpha_v)), 0.0, 0.0)
            else: k = (float(f32(alpha_v)), 0.0, 0.0)
    return dict(type=kind, twosided=int(twosided), distr=distr, sample_visible=int(sample_visible), nonlinear=int(nonlinear), table=table, texture=-1, aniso=aniso,
                reflectance=tuple(map(float, reflectance)), alpha=float(alpha),
                eta=tuple(map(float, eta)), k=tuple(map(float, k)),
                specular=tuple(map(float, specular)))


# ---------------------------------------------------------------------------------------------
# camera: reference src/sensors/perspective.cpp:126-178 (configure), src/libcore/transform.cpp:99-122
# (perspective), :191-201 (lookAt), src/librender/sensor.cpp:237-280 (fov handling, fovAxis "x")
# ---------------------------------------------------------------------------------------------
def look_at(origin, target, up):
    o = np.asarray(origin, f32); t = np.asarray(target, f32); u = np.asarray(up, f32)
    d = (t - o).astype(f32); d = (d / f32(np.sqrt(np.dot(d, d)))).astype(f32)
    left = np.cross(u, d).astype(f32); left = (left / f32(np.sqrt(np.dot(left, left)))).astype(f32)
    new_up = np.cross(d, left).astype(f32)
    m = np.eye(4, dtype=f32)
    m[:3, 0] = left; m[:3, 1] = new_up; m[:3, 2] = d; m[:3, 3] = o
    return m


_LIBM = None


def _tanf(x):
    """glibc tanf: std::tan(float) of the reference's Transform::perspective (numpy's float32 tan is its own SIMD routine)."""
    global _LIBM
    if _LIBM is None:
        import ctypes
        _LIBM = ctypes.CDLL("libm.so.6"); _LIBM.tanf.restype = ctypes.c_float; _LIBM.tanf.argtypes = [ctypes.c_float]
    return f32(_LIBM.tanf(float(x)))


def _mat_mul_f32(a, b):
    """Matrix<4,4,float> operator* (include/mitsuba/core/matrix.h:743-756): float accumulation, k ascending, sum starts at 0."""
    r = np.zeros((4, 4), f32)
    for i in range(4):
        for j in range(4):
            acc = f32(0)
            for k in range(4):
                acc = f32(acc + f32(a[i, k] * b[k, j]))
            r[i, j] = acc
    return r


def _mat_invert_f32(m):
    """Matrix::invert (include/mitsuba/core/matrix.inl:138-191): Gauss-Jordan with full pivoting in float, the reference's operation order."""
    t = np.array(m, f32).copy(); n = 4
    ipiv = [0] * n; indxr = [0] * n; indxc = [0] * n
    for i in range(n):
        irow = icol = -1; big = f32(0)
        for j in range(n):
            if ipiv[j] != 1:
                for k in range(n):
                    if ipiv[k] == 0:
                        if abs(t[j, k]) >= big:
                            big = abs(t[j, k]); irow, icol = j, k
                    elif ipiv[k] > 1:
                        raise ValueError("singular matrix")
        ipiv[icol] += 1
        if irow != icol:
            t[[irow, icol]] = t[[icol, irow]]
        indxr[i], indxc[i] = irow, icol
        if t[icol, icol] == 0:
            raise ValueError("singular matrix")
        pivinv = f32(f32(1) / t[icol, icol]); t[icol, icol] = f32(1)
        for j in range(n):
            t[icol, j] = f32(t[icol, j] * pivinv)
        for j in range(n):
            if j != icol:
                save = f32(t[j, icol]); t[j, icol] = f32(0)
                for k in range(n):
                    t[j, k] = f32(t[j, k] - f32(t[icol, k] * save))
    for j in range(n - 1, -1, -1):
        if indxr[j] != indxc[j]:
            t[:, [indxr[j], indxc[j]]] = t[:, [indxc[j], indxr[j]]]
    return t


def sample_to_camera(xfov_deg, near, far, aspect, rel_size=(1.0, 1.0), rel_offset=(0.0, 0.0)):
    """PerspectiveCameraImpl::configure (src/sensors/perspective.cpp:126-157), in the reference's own single-precision arithmetic so that camera
    rays come out bit-identical: cameraToSample = scale(1/relSize) * translate(-relOffset) * scale(-0.5,-0.5*aspect,1) * translate(-1,-1/aspect,0)
    * perspective(xfov,near,far); every Transform carries its inverse (scale / translate: closed form, perspective: Matrix::invert), products multiply
    the inverses in reverse (transform.cpp:28-31); sampleToCamera = the accumulated inverse.  `aspect` is the FULL film's; rel_size / rel_offset =
    crop size / offset over the full film size."""
    one = f32(1)
    aspect = f32(aspect); near = f32(near); far = f32(far); fov = f32(xfov_deg)
    rsx, rsy = f32(rel_size[0]), f32(rel_size[1]); rox, roy = f32(rel_offset[0]), f32(rel_offset[1])

    def scale_t(x, y, z):
        m = np.diag(np.array([x, y, z, one], f32)).astype(f32); i = np.diag(np.array([one / x, one / y, one / z, one], f32)).astype(f32); return m, i

    def translate_t(x, y, z):
        m = np.eye(4, dtype=f32); i = np.eye(4, dtype=f32); m[:3, 3] = [x, y, z]; i[:3, 3] = [-x, -y, -z]; return m, i

    recip = f32(one / f32(far - near))
    cot = f32(one / _tanf(f32(f32(fov / f32(2)) * f32(f32(3.14159265358979323846) / f32(180)))))      # degToRad(fov / 2.0f), util.h:309
    persp = np.array([[cot, 0, 0, 0], [0, cot, 0, 0], [0, 0, f32(far * recip), f32(f32(-near * far) * recip)], [0, 0, 1, 0]], dtype=f32)
    chain = [scale_t(f32(one / rsx), f32(one / rsy), one), translate_t(f32(-rox), f32(-roy), f32(0)),
             scale_t(f32(-0.5), f32(f32(-0.5) * aspect), one), translate_t(f32(-1), f32(f32(-1) / aspect), f32(0)), (persp, _mat_invert_f32(persp))]
    m, inv = chain[0]
    for (m2, i2) in chain[1:]:
        m, inv = _mat_mul_f32(m, m2), _mat_mul_f32(i2, inv)
    return inv


def set_crop_window(sc, full_width, full_height, offset_x, offset_y):
    """Turn `sc` (whose width x height stay the rendered film) into the crop window at (offset_x, offset_y) of a full_width x full_height frame
    (Film cropOffsetX/Y, cropWidth/Height, src/librender/film.cpp:35-47): only the camera's sample-to-camera mapping changes."""
    if offset_x < 0 or offset_y < 0 or offset_x + sc.width > full_width or offset_y + sc.height > full_height:
        raise ValueError("Invalid crop window specification!")
    sc.crop = (int(full_width), int(full_height), int(offset_x), int(offset_y))
    sc.sample_to_camera = sample_to_camera(sc.xfov, sc.near, sc.far, full_width / full_height,
                                           (f32(sc.width) / f32(full_width), f32(sc.height) / f32(full_height)), (f32(offset_x) / f32(full_width), f32(offset_y) / f32(full_height)))
    return sc


def with_lens(sc, aperture_radius, focus_distance):
    """The scene description with a thin lens: world-space aperture radius, distance of the focal plane along the camera axis.  Returns sc."""
    if not (aperture_radius >= 0) or (aperture_radius > 0 and not (focus_distance > 0)): raise ValueError("with_lens: aperture radius >= 0 and, with a lens, focus distance > 0")
    sc.aperture_radius = float(f32(aperture_radius)); sc.focus_distance = float(f32(focus_distance)) if aperture_radius > 0 else 0.0
    return sc


def finish_scene(verts, tris, shapes, bsdfs, emitters, cam_to_world, xfov, near, far, width, height,
                 spp, sampler, max_depth, rr_depth=5, filter_kind=FILTER_BOX, seed=0,
                 normals=None, uvs=None, strict_normals=False, hide_emitters=False, envmap=None,
                 name="scene", analytic=None, instances=None, textures=None, media=None, sensor_medium=-1, integrator=INTEGRATOR_PATH):
    sc = Scene()
    sc.name = name
    sc.pos = np.ascontiguousarray(np.asarray(verts, dtype=f32).reshape(-1, 3))
    sc.idx = np.ascontiguousarray(np.asarray(tris, dtype=np.uint32).reshape(-1, 3))
    sc.nrm = None if normals is None else np.ascontiguousarray(np.asarray(normals, dtype=f32).reshape(-1, 3))
    sc.uv = None if uvs is None else np.ascontiguousarray(np.asarray(uvs, dtype=f32).reshape(-1, 2))
    sc.shapes = shapes          # list of dict(first_tri, tri_count, first_vert, vert_count, bsdf, emitter, face_normals)
    sc.bsdfs = bsdfs
    sc.emitters = emitters      # list of dict(type, shape, radiance, weight)
    sc.cam_to_world = np.ascontiguousarray(cam_to_world, dtype=f32)
    sc.xfov = float(xfov); sc.near = float(near); sc.far = float(far)
    sc.width = int(width); sc.height = int(height)
    sc.sample_to_camera = sample_to_camera(xfov, near, far, width / height)
    sc.filter = filter_kind
    sc.filter_radius = {FILTER_BOX: 0.5, FILTER_MITCHELL: 1.0 / 3.0, FILTER_LANCZOS: 3.0}.get(filter_kind, 2.0)
    sc.filter_stddev = 1.0 / 3.0 if filter_kind == FILTER_MITCHELL else 0.5
    sc.max_depth = int(max_depth); sc.rr_depth = int(rr_depth)
    sc.strict_normals = int(strict_normals); sc.hide_emitters = int(hide_emitters)
    sc.sampler = sampler; sc.spp = int(spp); sc.seed = int(seed)
    sc.envmap = envmap          # None or dict(rgb[h,w,3] f32, to_world[4,4], scale)
    sc.aperture_radius = 0.0; sc.focus_distance = 0.0   # thin lens (src/sensors/thinlens.cpp) on top of the perspective camera; radius 0 = none (with_lens)
    sc.fields = []              # field channels next to the radiance (the reference's multichannel + field integrators): names out of api.FIELD_NAMES or (name, undefined) pairs
    textures = list(textures or [])
    sc.env_texture = 0                              # index + 1 of the texture record holding the environment map's MIP pyramid (camera-ray lookups, envmap.cpp:398-411)
    if envmap is not None and envmap.get("filtered", True):
        levels = envmap.get("levels") or build_mip_pyramid(envmap["rgb"], WRAP_REPEAT, WRAP_CLAMP, float("inf"))
        textures.append(make_texture(TEXTURE_BITMAP, pyramid=dict(levels=levels), wrap_u=WRAP_REPEAT, wrap_v=WRAP_CLAMP, filter_type=MIP_EWA, max_anisotropy=10.0))
        sc.env_texture = len(textures)
    lv = []; tx = []                                # MIP pyramids of the bitmap textures, concatenated: texture_levels[n][3] = (w, h, offset), texture_texels
    for t in (textures or []):
        if t.get("pyramid") is not None:
            levels = t["pyramid"]["levels"] if t["filter"] >= MIP_TRILINEAR else t["pyramid"]["levels"][:1]      # mipmap.h:183-191: one level without trilinear / EWA
            t["first_level"] = len(lv); t["n_levels"] = len(levels)
            for (w, h, data) in levels:
                lv.append((w, h, sum(len(a) for a in tx))); tx.append(data)
    sc.texture_levels = np.asarray(lv, np.uint32).reshape(-1, 3) if lv else None
    sc.texture_texels = np.concatenate(tx).astype(f32) if tx else None
    sc.textures = list(textures or [])             # 2-D procedural textures (make_texture); a bsdf dict binds one to its reflectance through "texture" = index
    for sh in shapes: sh.setdefault("has_uv", int(uvs is not None))
    tabs = []                                       # float tables referenced by materials (roughplastic): k[1] = offset into sc.material_tables
    for bd in bsdfs:
        if bd.get("table") is not None:
            off = sum(len(t) for t in tabs); tabs.append(bd["table"]); bd["k"] = (bd["k"][0], float(off), float(len(bd["table"])))
    sc.material_tables = np.concatenate(tabs).astype(f32) if tabs else None
    sc.instances = list(instances or [])  # placements of shape groups (make_instance); shapes carry "group" = g + 1 when they belong to group g
    sc.analytic = list(analytic or [])   # analytic shapes (make_analytic); shape index of the i-th = len(shapes) + i; primitive index = len(idx) + i
    tri_shape = np.zeros(len(sc.idx), dtype=np.uint32)
    for si, s in enumerate(shapes):
        tri_shape[s["first_tri"]:s["first_tri"] + s["tri_count"]] = si
    sc.tri_shape = tri_shape
    # participating media (make_medium); a shape / analytic record names its "interior" / "exterior" medium by index (-1: none), the sensor its own
    sc.media = list(media or []); sc.sensor_medium = int(sensor_medium) if sc.media else -1; sc.integrator = int(integrator)
    sc.shape_media = np.asarray([[r.get("interior", -1), r.get("exterior", -1)] for r in list(shapes) + list(sc.analytic)], np.int32).reshape(-1, 2) if sc.media else None
    return sc


# ---------------------------------------------------------------------------------------------
# analytic shapes: reference src/shapes/{rectangle,disk,sphere,cylinder}.cpp.  A record carries the shape's objectToWorld as the
# reference holds it AFTER the constructor (sphere / cylinder: scale split off into radius / length) and its inverse.
# ---------------------------------------------------------------------------------------------
def translate(x, y, z):
    m = np.eye(4); m[:3, 3] = (x, y, z); return m


def scale(x, y=None, z=None):
    y = x if y is None else y; z = x if z is None else z
    return np.diag([x, y, z, 1.0])


def rotate(axis, degrees):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a); t = math.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4); m[:3, :3] = np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)
    return m


def make_analytic(kind, to_world, bsdf, emitter=-1, flip=False, radius=1.0, length=1.0):
    tw = np.ascontiguousarray(to_world, dtype=f32)
    to = np.ascontiguousarray(np.linalg.inv(tw.astype(np.float64)), dtype=f32)
    return dict(type=int(kind), bsdf=int(bsdf), emitter=int(emitter), flags=int(bool(flip)), to_world=tw, to_object=to,
                radius=float(f32(radius)), length=float(f32(length)))


TEXTURE_CHECKERBOARD = 0   # src/textures/checkerboard.cpp
TEXTURE_GRID = 1           # src/textures/gridtexture.cpp
TEXTURE_BITMAP = 2         # src/textures/bitmap.cpp over TMIPMap (include/mitsuba/render/mipmap.h); the MIP pyramid is input data
WRAP_CLAMP, WRAP_REPEAT, WRAP_MIRROR, WRAP_ZERO, WRAP_ONE = 0, 1, 2, 3, 4          # ReconstructionFilter::EBoundaryCondition
MIP_NEAREST, MIP_BILINEAR, MIP_TRILINEAR, MIP_EWA = 0, 1, 2, 3                       # EMIPFilterType


def load_texture_pyramid(name="texture_pyramid_48x40.npz"):
    """A MIP pyramid as the reference builds it (TMIPMap<Color3, Color3h>, 2-lobed Lanczos, repeat): dumped by `oracle/_ref/harness mipmap` from
    the procedural base image stored alongside.  Returns dict(base[h,w,3], levels=[(w, h, texels[h*w*3])...])."""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", name))
    levels = []; off = 0
    for w, h in d["sizes"]:
        n = int(w) * int(h) * 3; levels.append((int(w), int(h), np.ascontiguousarray(d["texels"][off:off + n], f32))); off += n
    return dict(base=np.ascontiguousarray(d["base"], f32), levels=levels)


def make_texture(kind, color0=(0, 0, 0), color1=(0, 0, 0), line_width=0.01, uoffset=0.0, voffset=0.0, uscale=1.0, vscale=1.0,
                 pyramid=None, wrap_u=WRAP_REPEAT, wrap_v=WRAP_REPEAT, filter_type=MIP_EWA, max_anisotropy=20.0):
    if kind == TEXTURE_BITMAP and pyramid is not None:
        # a bitmap's average (TMIPMap::getAverage: the float sum of the base image in row-major order / pixel count, barray.h:309-332) travels in color0:
        # plastic / roughplastic derive their lobe-selection weight from it (plastic.cpp:204-207)
        base = pyramid.get("base")
        if base is None:
            w0, h0, t0 = pyramid["levels"][0]; base = np.asarray(t0, f32).reshape(h0, w0, 3)
        elif (wrap_u, wrap_v) != (WRAP_REPEAT, WRAP_REPEAT) and not pyramid.get("wrapped"):
            # the reference resamples with the texture's own boundary conditions (bitmap.cpp:363-401): rebuild the levels for this wrap mode
            pyramid = dict(base=base, levels=build_mip_pyramid(base, wrap_u, wrap_v, 1.0), wrapped=True)
        flat = np.maximum(np.asarray(base, f32), f32(0)).reshape(-1, 3)
        color0 = tuple(float(np.cumsum(flat[:, c], dtype=f32)[-1] / f32(len(flat))) for c in range(3))
    return dict(type=int(kind), color0=tuple(map(float, color0)), color1=tuple(map(float, color1)), line_width=float(line_width),
                uoffset=float(uoffset), voffset=float(voffset), uscale=float(uscale), vscale=float(vscale), pyramid=pyramid,
                wrap_u=int(wrap_u), wrap_v=int(wrap_v), filter=int(filter_type), max_anisotropy=float(max_anisotropy if filter_type == MIP_EWA else 1.0),
                first_level=0, n_levels=0)


def make_instance(group, to_world):
    """src/shapes/instance.cpp: placement of shape group `group` (0-based); to_object as the reference's Transform::inverse would hold it."""
    tw = np.ascontiguousarray(to_world, dtype=f32)
    return dict(group=int(group), to_world=tw, to_object=np.ascontiguousarray(np.linalg.inv(tw.astype(np.float64)), dtype=f32))


def _coordinate_system(a):
    """reference src/libcore/util.cpp:594-603 in float32: returns (b, c) with b = cross(c, a)."""
    a = np.asarray(a, f32)
    if abs(a[0]) > abs(a[1]):
        inv = f32(1.0) / np.sqrt(a[0] * a[0] + a[2] * a[2], dtype=f32); c = np.array([a[2] * inv, 0.0, -a[0] * inv], f32)
    else:
        inv = f32(1.0) / np.sqrt(a[1] * a[1] + a[2] * a[2], dtype=f32); c = np.array([0.0, a[2] * inv, -a[1] * inv], f32)
    b = np.array([c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]], f32)
    return b, c


def cylinder_to_world(p0, p1):
    """translate(p0) * fromFrame(Frame(d / |d|)) (cylinder.cpp:88-92, scale split off); returns (matrix, length)."""
    p0 = np.asarray(p0, f32); d = (np.asarray(p1, f32) - p0).astype(f32)
    length = np.sqrt(np.dot(d, d), dtype=f32); n = (d / length).astype(f32)
    s_, t_ = _coordinate_system(n)
    m = np.eye(4, dtype=f32); m[:3, 0] = s_; m[:3, 1] = t_; m[:3, 2] = n; m[:3, 3] = p0
    return m, float(length)


class _Builder:
    def __init__(self):
        self.verts, self.tris, self.shapes, self.bsdfs, self.emitters = [], [], [], [], []
        self.normals = None
        self.analytic = []

    def add_analytic(self, kind, to_world, bsdf, radiance=None, flip=False, radius=1.0, length=1.0, interior=-1, exterior=-1):
        """call after all meshes: the shape index of an analytic shape is len(shapes) + its position."""
        rec = make_analytic(kind, to_world, bsdf, -1, flip, radius, length)
        rec["_radiance"] = None if radiance is None else tuple(map(float, radiance)); rec["interior"] = int(interior); rec["exterior"] = int(exterior)
        self.analytic.append(rec)

    def resolve_analytic(self):
        for i, rec in enumerate(self.analytic):
            rad = rec.pop("_radiance", None)
            if rad is not None:
                self.emitters.append(dict(type=EMITTER_AREA, shape=len(self.shapes) + i, radiance=rad, weight=1.0))
                rec["emitter"] = len(self.emitters) - 1
        return self.analytic

    def bsdf(self, **kw):
        self.bsdfs.append(make_bsdf(**kw))
        return len(self.bsdfs) - 1

    def begin(self):
        self._ft, self._fv = len(self.tris), len(self.verts)

    def quad(self, pts):
        _quad(self.verts, self.tris, None, [tuple(map(float, p)) for p in pts])

    def end(self, bsdf, radiance=None, face_normals=True, group=0, interior=-1, exterior=-1):
        em = -1
        si = len(self.shapes)
        if radiance is not None:
            self.emitters.append(dict(type=EMITTER_AREA, shape=si, radiance=tuple(map(float, radiance)), weight=1.0))
            em = len(self.emitters) - 1
        self.shapes.append(dict(first_tri=self._ft, tri_count=len(self.tris) - self._ft,
                                first_vert=self._fv, vert_count=len(self.verts) - self._fv,
                                bsdf=bsdf, emitter=em, face_normals=int(face_normals), group=int(group), interior=int(interior), exterior=int(exterior)))


def cornell_box(width=1920, height=1080, spp=8, sampler=SAMPLER_SOBOL, max_depth=8, rr_depth=5,
                filter_kind=FILTER_BOX, seed=0, strict_normals=False, hide_emitters=False):
    """S1: the classic Cornell box data (units 0..560), one-sided `diffuse` everywhere with
    consistent winding (face normals point into the room / out of the blocks), ceiling quad light lowered to
    y=548.3 so that no two surfaces coincide; block bottoms (coplanar with the floor) are left out => 32 triangles."""
    b = _Builder()
    white = b.bsdf(reflectance=(0.725, 0.71, 0.68))
    red = b.bsdf(reflectance=(0.63, 0.065, 0.05))
    green = b.bsdf(reflectance=(0.14, 0.45, 0.091))
    lightm = b.bsdf(reflectance=(0.78, 0.78, 0.78))
    b.begin(); b.quad([(552.8, 0, 0), (0, 0, 0), (0, 0, 559.2), (549.6, 0, 559.2)]); b.end(white)          # floor
    b.begin(); b.quad([(556, 548.8, 0), (556, 548.8, 559.2), (0, 548.8, 559.2), (0, 548.8, 0)]); b.end(white)  # ceiling
    b.begin(); b.quad([(549.6, 0, 559.2), (0, 0, 559.2), (0, 548.8, 559.2), (556, 548.8, 559.2)]); b.end(white)  # back
    b.begin(); b.quad([(0, 0, 559.2), (0, 0, 0), (0, 548.8, 0), (0, 548.8, 559.2)]); b.end(green)          # right (x=0)
    b.begin(); b.quad([(552.8, 0, 0), (549.6, 0, 559.2), (556, 548.8, 559.2), (556, 548.8, 0)]); b.end(red)  # left
    b.begin(); b.quad([(343, 548.3, 227), (343, 548.3, 332), (213, 548.3, 332), (213, 548.3, 227)])
    b.end(lightm, radiance=(17.0, 12.0, 4.0))
    b.begin()                                                                                             # short block
    b.quad([(130, 165, 65), (82, 165, 225), (240, 165, 272), (290, 165, 114)])
    b.quad([(290, 0, 114), (290, 165, 114), (240, 165, 272), (240, 0, 272)])
    b.quad([(130, 0, 65), (130, 165, 65), (290, 165, 114), (290, 0, 114)])
    b.quad([(82, 0, 225), (82, 165, 225), (130, 165, 65), (130, 0, 65)])
    b.quad([(240, 0, 272), (240, 165, 272), (82, 165, 225), (82, 0, 225)])
    b.end(white)
    b.begin()                                                                                             # tall block
    b.quad([(423, 330, 247), (265, 330, 296), (314, 330, 456), (472, 330, 406)])
    b.quad([(423, 0, 247), (423, 330, 247), (472, 330, 406), (472, 0, 406)])
    b.quad([(472, 0, 406), (472, 330, 406), (314, 330, 456), (314, 0, 456)])
    b.quad([(314, 0, 456), (314, 330, 456), (265, 330, 296), (265, 0, 296)])
    b.quad([(265, 0, 296), (265, 330, 296), (423, 330, 247), (423, 0, 247)])
    b.end(white)
    cam = look_at((278, 273, -800), (278, 273, -799), (0, 1, 0))
    return finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 39.3, 10.0, 2800.0,
                        width, height, spp, sampler, max_depth, rr_depth, filter_kind, seed, strict_normals=strict_normals,
                        hide_emitters=hide_emitters, name="cornell")


def fog_sky(width=96, height=64, spp=16, sampler=SAMPLER_SOBOL, max_depth=6, rr_depth=4, seed=0, global_fog=False, hide_emitters=False, integrator=INTEGRATOR_VOLPATH, env_size=(64, 32), constant_env=False):
    """Volumetric loops under an environment map: ground, a diffuse block, a `null` sphere of haze, a glass block with a scattering interior, an area light; with
    global_fog the sensor sits in a thin medium (the reference then sees the sky through emitter sampling only: a ray that leaves the scene inside an unbounded
    medium has zero transmittance, volpath.cpp:383-384 with its->t = infinity)."""
    b = _Builder()
    grey = b.bsdf(reflectance=(0.5, 0.5, 0.5)); red = b.bsdf(reflectance=(0.65, 0.2, 0.15)); null = b.bsdf(kind=BSDF_NULL); glass = b.bsdf(kind=BSDF_DIELECTRIC, ior=1.5, reflectance=(1.0, 1.0, 1.0))
    lightm = b.bsdf(reflectance=(0.5, 0.5, 0.5))
    media = [make_medium((0.05, 0.1, 0.2), (0.9, 0.8, 0.7), phase=PHASE_HG, g=0.4), make_medium((0.2, 0.05, 0.2), (0.5, 1.0, 0.5), strategy=MEDIUM_SINGLE)]
    ext = -1
    if global_fog:
        media.append(make_medium((0.005, 0.005, 0.008), (0.03, 0.03, 0.025))); ext = 2
    b.begin(); b.quad([(8, 0, -8), (-8, 0, -8), (-8, 0, 8), (8, 0, 8)]); b.end(grey)
    b.begin(); _closed_box(b, [(-1.2, 0.8), (-1.2, 2.0), (0.2, 2.0), (0.2, 0.8)], 0.001, 1.4); b.end(red)
    b.begin(); _closed_box(b, [(0.9, 0.2), (0.9, 1.3), (2.0, 1.3), (2.0, 0.2)], 0.001, 1.1); b.end(glass, interior=1, exterior=ext)
    b.begin(); b.quad([(-0.5, 3.2, 0.5), (0.5, 3.2, 0.5), (0.5, 3.2, 1.5), (-0.5, 3.2, 1.5)]); b.end(lightm, radiance=(6.0, 5.0, 4.0))
    b.add_analytic(SHAPE_SPHERE, translate(-0.3, 0.9, -0.6), null, radius=0.7, interior=0, exterior=ext)
    cam = look_at((0.8, 1.3, -4.5), (0.1, 1.0, 1.0), (0, 1, 0))
    env = None if constant_env else dict(rgb=detailed_sky(*env_size), to_world=(rotate((0, 1, 0), 25.0) @ rotate((1, 0, 0), 8.0)).astype(f32), scale=0.8)
    sc = finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 55.0, 0.05, 100.0, width, height, spp, sampler, max_depth, rr_depth,
                      seed=seed, hide_emitters=hide_emitters, envmap=env, name="fog_sky", analytic=b.resolve_analytic(), media=media, sensor_medium=ext, integrator=integrator)
    return add_scene_emitters(sc, [constant_emitter((0.55, 0.7, 0.95)) if constant_env else dict(type=EMITTER_ENVMAP, shape=-1, radiance=(0.0, 0.0, 0.0), weight=1.0)])


def _closed_box(b, top, y0, y1):
    """closed box over the quadrilateral `top` = four (x, z) corners in the Cornell blocks' order (normal up); all faces point outwards"""
    P = [tuple(map(float, p)) for p in top]
    b.quad([(p[0], y1, p[1]) for p in P])
    for i in range(4):
        j = (i + 1) % 4
        b.quad([(P[j][0], y0, P[j][1]), (P[j][0], y1, P[j][1]), (P[i][0], y1, P[i][1]), (P[i][0], y0, P[i][1])])
    b.quad([(p[0], y0, p[1]) for p in reversed(P)])


def fog_box(width=96, height=96, spp=16, sampler=SAMPLER_SOBOL, max_depth=8, rr_depth=5, seed=0, global_fog=False, strict_normals=False, hide_emitters=False, integrator=INTEGRATOR_VOLPATH_SIMPLE, pane=False, dusty=False):
    """Cornell room for the volumetric path tracer (volpath_simple): a smoke cube behind an index-matched (`null`) boundary (isotropic, `balance`
    sampling), a glass block filled with a forward-scattering medium (hg, `single`), a `null` sphere of thin haze (hg backwards, `manual`); with global_fog the
    sensor sits in a thin isotropic medium that fills the room (the shapes name it as their exterior medium)."""
    b = _Builder()
    white = b.bsdf(reflectance=(0.725, 0.71, 0.68)); red = b.bsdf(reflectance=(0.63, 0.065, 0.05)); green = b.bsdf(reflectance=(0.14, 0.45, 0.091))
    lightm = b.bsdf(reflectance=(0.78, 0.78, 0.78)); null = b.bsdf(kind=BSDF_NULL); glass = b.bsdf(kind=BSDF_DIELECTRIC, ior=1.5, reflectance=(1.0, 1.0, 1.0))
    media = [make_medium((0.001, 0.002, 0.004), (0.012, 0.010, 0.008)),
             make_medium((0.002, 0.0005, 0.002), (0.004, 0.008, 0.004), strategy=MEDIUM_SINGLE, phase=PHASE_HG, g=0.6),
             make_medium((0.0005, 0.0005, 0.0005), (0.006, 0.006, 0.007), strategy=MEDIUM_MANUAL, sampling_density=0.008, phase=PHASE_HG, g=-0.3)]
    ext = -1
    if global_fog:
        media.append(make_medium((0.0001, 0.0001, 0.00015), (0.0006, 0.0006, 0.0005))); ext = 3
    b.begin(); b.quad([(552.8, 0, 0), (0, 0, 0), (0, 0, 559.2), (549.6, 0, 559.2)]); b.end(white)
    b.begin(); b.quad([(556, 548.8, 0), (556, 548.8, 559.2), (0, 548.8, 559.2), (0, 548.8, 0)]); b.end(white)
    b.begin(); b.quad([(549.6, 0, 559.2), (0, 0, 559.2), (0, 548.8, 559.2), (556, 548.8, 559.2)]); b.end(white)
    b.begin(); b.quad([(0, 0, 559.2), (0, 0, 0), (0, 548.8, 0), (0, 548.8, 559.2)]); b.end(green)
    b.begin(); b.quad([(552.8, 0, 0), (549.6, 0, 559.2), (556, 548.8, 559.2), (556, 548.8, 0)]); b.end(red)
    b.begin(); b.quad([(343, 548.3, 227), (343, 548.3, 332), (213, 548.3, 332), (213, 548.3, 227)]); b.end(lightm, radiance=(17.0, 12.0, 4.0))
    b.begin(); _closed_box(b, [(130, 65), (82, 225), (240, 272), (290, 114)], 0.5, 165.0); b.end(null, interior=0, exterior=ext)
    b.begin(); _closed_box(b, [(423, 247), (265, 296), (314, 456), (472, 406)], 0.5, 330.0); b.end(glass, interior=1, exterior=ext)
    if pane:        # a thin glass pane in front of the smoke cube: its transmission is an ENull lobe -- emitter sampling and the emitter search look THROUGH it (attenuated)
        thin = b.bsdf(kind=BSDF_THINDIELECTRIC, ior=1.5, reflectance=(0.9, 0.95, 1.0))
        p0, e1, e2 = np.array([40.3, 1.2, 40.7]), np.array([290.4, 0.37, -20.3]), np.array([0.53, 318.9, 0.21])      # (odd numbers: no Sobol sample lands exactly on the quad's diagonal, cf. closed_box)
        if dusty:   # a dusty pane: mixturebsdf of the thin glass and a diffuse film -- the walks see weight x the glass' pass-through value (mixturebsdf.cpp:176-183)
            dust = b.bsdf(reflectance=(0.5, 0.45, 0.4)); thin = b.bsdf(kind=BSDF_MIXTURE, nested=[thin, dust], weights=[0.7, 0.3])
        b.begin(); b.quad([p0, p0 + e1, p0 + e1 + e2, p0 + e2]); b.end(thin)
    b.add_analytic(SHAPE_SPHERE, translate(150.0, 390.0, 300.0), null, radius=70.0, interior=2, exterior=ext)
    cam = look_at((278, 273, -800), (278, 273, -799), (0, 1, 0))
    return finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 39.3, 10.0, 2800.0, width, height, spp, sampler, max_depth, rr_depth, FILTER_BOX, seed,
                        strict_normals=strict_normals, hide_emitters=hide_emitters, name="fog_box", analytic=b.resolve_analytic(), media=media,
                        sensor_medium=ext, integrator=integrator)


def cbox_shapes(width=256, height=256, spp=16, sampler=SAMPLER_SOBOL, max_depth=8, rr_depth=5, filter_kind=FILTER_BOX, seed=0,
                strict_normals=False, hide_emitters=False, disk_cap=True):
    """Cornell room (mesh walls) furnished with analytic shapes: `rectangle` ceiling light, a diffuse `sphere`,
    a rough-conductor `sphere`, an open `cylinder` (twosided diffuse) capped by a `disk` (disk_cap=False leaves it out: the reference's
    Disk::fillIntersectionRecord never sets the geometric frame, so `strictNormals` reads a stale normal there -- DESIGN.md)."""
    b = _Builder()
    white = b.bsdf(reflectance=(0.725, 0.71, 0.68))
    red = b.bsdf(reflectance=(0.63, 0.065, 0.05))
    green = b.bsdf(reflectance=(0.14, 0.45, 0.091))
    lightm = b.bsdf(reflectance=(0.78, 0.78, 0.78))
    white2 = b.bsdf(reflectance=(0.725, 0.71, 0.68), twosided=True)
    eta, k = CONDUCTOR_IOR["Cu"]
    copper = b.bsdf(kind=BSDF_ROUGHCONDUCTOR, alpha=0.15, distr=DISTR_GGX, eta=eta, k=k)
    b.begin(); b.quad([(552.8, 0, 0), (0, 0, 0), (0, 0, 559.2), (549.6, 0, 559.2)]); b.end(white)
    b.begin(); b.quad([(556, 548.8, 0), (556, 548.8, 559.2), (0, 548.8, 559.2), (0, 548.8, 0)]); b.end(white)
    b.begin(); b.quad([(549.6, 0, 559.2), (0, 0, 559.2), (0, 548.8, 559.2), (556, 548.8, 559.2)]); b.end(white)
    b.begin(); b.quad([(0, 0, 559.2), (0, 0, 0), (0, 548.8, 0), (0, 548.8, 559.2)]); b.end(green)
    b.begin(); b.quad([(552.8, 0, 0), (549.6, 0, 559.2), (556, 548.8, 559.2), (556, 548.8, 0)]); b.end(red)
    # rectangle light: [-1,1]^2, normal +z -> scaled to 130 x 105, turned to face down (-y), hung at y = 548.3
    b.add_analytic(SHAPE_RECTANGLE, translate(278, 548.3, 279.5) @ rotate((1, 0, 0), 90) @ scale(65, 52.5, 1), lightm, radiance=(17.0, 12.0, 4.0))
    b.add_analytic(SHAPE_SPHERE, translate(150, 90, 170) @ rotate((0.3, 1, 0.2), 35), white, radius=90.0)
    b.add_analytic(SHAPE_SPHERE, translate(420, 70, 130), copper, radius=70.0)
    m, length = cylinder_to_world((370, 0, 380), (370, 260, 380))
    b.add_analytic(SHAPE_CYLINDER, m, white2, radius=80.0, length=length)
    if disk_cap:
        b.add_analytic(SHAPE_DISK, translate(370, 260, 380) @ rotate((1, 0, 0), -90) @ scale(80), white)
    cam = look_at((278, 273, -800), (278, 273, -799), (0, 1, 0))
    return finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 39.3, 10.0, 2800.0, width, height, spp, sampler, max_depth, rr_depth,
                        filter_kind, seed, strict_normals=strict_normals, hide_emitters=hide_emitters, name="cbox_shapes", analytic=b.resolve_analytic())


def textured_shapes(width=96, height=96, spp=16, sampler=SAMPLER_SOBOL, max_depth=8, rr_depth=5, seed=0):
    """Textures on ANALYTIC shapes through their own parameterisations (rectangle.cpp:163, disk.cpp:193, sphere.cpp:225-226, cylinder.cpp:209-210): a
    checkerboard `rectangle` floor, a grid-textured `plastic` sphere, a bitmap-textured (EWA) cylinder with a checkerboard `disk` lid, a `mask`ed
    rectangle screen; mesh walls and the rectangle light of `cbox_shapes`."""
    b = _Builder()
    white = b.bsdf(reflectance=(0.725, 0.71, 0.68)); red = b.bsdf(reflectance=(0.63, 0.065, 0.05)); green = b.bsdf(reflectance=(0.14, 0.45, 0.091))
    lightm = b.bsdf(reflectance=(0.78, 0.78, 0.78))
    pyr = load_texture_pyramid()
    tex = [make_texture(TEXTURE_CHECKERBOARD, (0.8, 0.75, 0.6), (0.15, 0.2, 0.3), uscale=8.0, vscale=8.0),
           make_texture(TEXTURE_GRID, (0.2, 0.55, 0.7), (0.95, 0.9, 0.2), line_width=0.07, uscale=10.0, vscale=5.0),
           make_texture(TEXTURE_BITMAP, pyramid=pyr, uscale=4.0, vscale=2.0, filter_type=MIP_EWA),
           make_texture(TEXTURE_CHECKERBOARD, (0.9, 0.3, 0.2), (0.1, 0.1, 0.1), uscale=3.0, vscale=6.0, uoffset=0.2),
           make_texture(TEXTURE_CHECKERBOARD, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), uscale=6.0, vscale=6.0)]
    floor = b.bsdf(reflectance=(0.5, 0.5, 0.5)); b.bsdfs[floor]["texture"] = 0
    ball = b.bsdf(kind=BSDF_PLASTIC, ior=1.49, specular=(0.9, 0.9, 0.9)); b.bsdfs[ball]["texture"] = 1
    tube = b.bsdf(reflectance=(0.5, 0.5, 0.5), twosided=True); b.bsdfs[tube]["texture"] = 2
    lid = b.bsdf(reflectance=(0.5, 0.5, 0.5), twosided=True); b.bsdfs[lid]["texture"] = 3
    blue2 = b.bsdf(reflectance=(0.15, 0.25, 0.7), twosided=True)
    screen = b.bsdf(kind=BSDF_MASK, nested=blue2); b.bsdfs[screen]["texture"] = 4
    b.begin(); b.quad([(556, 548.8, 0), (556, 548.8, 559.2), (0, 548.8, 559.2), (0, 548.8, 0)]); b.end(white)
    b.begin(); b.quad([(549.6, 0, 559.2), (0, 0, 559.2), (0, 548.8, 559.2), (556, 548.8, 559.2)]); b.end(white)
    b.begin(); b.quad([(0, 0, 559.2), (0, 0, 0), (0, 548.8, 0), (0, 548.8, 559.2)]); b.end(green)
    b.begin(); b.quad([(552.8, 0, 0), (549.6, 0, 559.2), (556, 548.8, 559.2), (556, 548.8, 0)]); b.end(red)
    b.add_analytic(SHAPE_RECTANGLE, translate(278, 548.3, 279.5) @ rotate((1, 0, 0), 90) @ scale(65, 52.5, 1), lightm, radiance=(17.0, 12.0, 4.0))
    b.add_analytic(SHAPE_RECTANGLE, translate(278, 0, 279.6) @ rotate((1, 0, 0), -90) @ scale(278, 279.6, 1), floor)                 # the floor: +y
    b.add_analytic(SHAPE_SPHERE, translate(150, 90, 170) @ rotate((0.3, 1, 0.2), 35), ball, radius=90.0)
    m, length = cylinder_to_world((370, 0, 380), (370, 260, 380))
    b.add_analytic(SHAPE_CYLINDER, m, tube, radius=80.0, length=length)
    b.add_analytic(SHAPE_DISK, translate(370, 260, 380) @ rotate((1, 0, 0), -90) @ scale(80), lid)
    b.add_analytic(SHAPE_RECTANGLE, translate(300, 150, 60) @ rotate((0, 1, 0), 20) @ scale(120, 110, 1), screen)
    cam = look_at((278, 273, -800), (278, 273, -799), (0, 1, 0))
    return finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 39.3, 10.0, 2800.0, width, height, spp, sampler, max_depth, rr_depth,
                        seed=seed, name="textured_shapes", analytic=b.resolve_analytic(), textures=tex)


def cbox_materials(width=96, height=96, spp=16, sampler=SAMPLER_SOBOL, max_depth=10, rr_depth=5, seed=0, strict_normals=False, hide_emitters=False):
    """Cornell room with the smooth BSDF family: glass `dielectric` sphere, gold smooth `conductor` sphere, `plastic` tall
    block, nonlinear `plastic` floor, a `twosided(conductor)` mirror sheet; the usual ceiling quad light."""
    b = _Builder()
    white = b.bsdf(reflectance=(0.725, 0.71, 0.68)); red = b.bsdf(reflectance=(0.63, 0.065, 0.05)); green = b.bsdf(reflectance=(0.14, 0.45, 0.091))
    lightm = b.bsdf(reflectance=(0.78, 0.78, 0.78))
    floor = b.bsdf(kind=BSDF_PLASTIC, reflectance=(0.6, 0.5, 0.35), specular=(1.0, 1.0, 1.0), ior=1.49, nonlinear=True)
    blockm = b.bsdf(kind=BSDF_PLASTIC, reflectance=(0.15, 0.25, 0.6), specular=(0.9, 0.9, 0.9), ior=1.5046)
    glass = b.bsdf(kind=BSDF_DIELECTRIC, reflectance=(0.95, 1.0, 0.97), specular=(1.0, 1.0, 1.0), ior=1.5046)
    eta, k = CONDUCTOR_IOR["Au"]; gold = b.bsdf(kind=BSDF_CONDUCTOR, eta=eta, k=k)
    eta, k = CONDUCTOR_IOR["Al"]; mirror = b.bsdf(kind=BSDF_CONDUCTOR, eta=eta, k=k, specular=(0.9, 0.9, 0.9), twosided=True)
    b.begin(); b.quad([(552.8, 0, 0), (0, 0, 0), (0, 0, 559.2), (549.6, 0, 559.2)]); b.end(floor)
    b.begin(); b.quad([(556, 548.8, 0), (556, 548.8, 559.2), (0, 548.8, 559.2), (0, 548.8, 0)]); b.end(white)
    b.begin(); b.quad([(549.6, 0, 559.2), (0, 0, 559.2), (0, 548.8, 559.2), (556, 548.8, 559.2)]); b.end(white)
    b.begin(); b.quad([(0, 0, 559.2), (0, 0, 0), (0, 548.8, 0), (0, 548.8, 559.2)]); b.end(green)
    b.begin(); b.quad([(552.8, 0, 0), (549.6, 0, 559.2), (556, 548.8, 559.2), (556, 548.8, 0)]); b.end(red)
    b.begin(); b.quad([(343, 548.3, 227), (343, 548.3, 332), (213, 548.3, 332), (213, 548.3, 227)]); b.end(lightm, radiance=(17.0, 12.0, 4.0))
    b.begin()
    b.quad([(423, 330, 247), (265, 330, 296), (314, 330, 456), (472, 330, 406)])
    b.quad([(423, 0, 247), (423, 330, 247), (472, 330, 406), (472, 0, 406)])
    b.quad([(472, 0, 406), (472, 330, 406), (314, 330, 456), (314, 0, 456)])
    b.quad([(314, 0, 456), (314, 330, 456), (265, 330, 296), (265, 0, 296)])
    b.quad([(265, 0, 296), (265, 330, 296), (423, 330, 247), (423, 0, 247)])
    b.end(blockm)
    b.begin(); b.quad([(20, 40, 420), (150, 40, 540), (150, 300, 540), (20, 300, 420)]); b.end(mirror)
    b.add_analytic(SHAPE_SPHERE, translate(170, 100, 190), glass, radius=100.0)
    b.add_analytic(SHAPE_SPHERE, translate(400, 60, 120), gold, radius=60.0)
    cam = look_at((278, 273, -800), (278, 273, -799), (0, 1, 0))
    return finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 39.3, 10.0, 2800.0, width, height, spp, sampler, max_depth, rr_depth,
                        seed=seed, strict_normals=strict_normals, hide_emitters=hide_emitters, name="cbox_materials", analytic=b.resolve_analytic())


def instanced_garden(width=96, height=64, spp=16, sampler=SAMPLER_SOBOL, max_depth=6, rr_depth=4, seed=0, n_side=4, smooth=True, bush_levels=2):
    """`shapegroup` + `instance`: two shape groups -- a smooth-shaded "bush" (octahedral blob with vertex normals) and a
    face-normal "crate" with a rough-conductor lid -- placed n_side x n_side times with rotation, non-uniform scale and shear-free tilts,
    over a mesh floor, lit by an area light and a constant sky.  bush_levels: subdivisions of the bush's octahedron (8 * 4^levels triangles; 4 gives a 2048-triangle
    group, the smallest whose tree has a level wider than one 256-thread workgroup)."""
    b = _Builder()
    ground = b.bsdf(reflectance=(0.45, 0.5, 0.4)); leaf = b.bsdf(reflectance=(0.2, 0.55, 0.15), twosided=True); wood = b.bsdf(reflectance=(0.5, 0.33, 0.18))
    eta, k = CONDUCTOR_IOR["Cu"]; lid = b.bsdf(kind=BSDF_ROUGHCONDUCTOR, alpha=0.12, distr=DISTR_GGX, eta=eta, k=k)
    lightm = b.bsdf(reflectance=(0.5, 0.5, 0.5))
    b.begin(); b.quad([(8, 0, -8), (-8, 0, -8), (-8, 0, 8), (8, 0, 8)]); b.end(ground)
    b.begin(); b.quad([(1.5, 6, -1.5), (1.5, 6, 1.5), (-1.5, 6, 1.5), (-1.5, 6, -1.5)]); b.end(lightm, radiance=(30.0, 28.0, 24.0))
    normals = [(0.0, 1.0, 0.0)] * len(b.verts)
    # group 0: bush = subdivided octahedron pushed to a bumpy sphere, vertex normals
    b.begin(); base = len(b.verts)
    P = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    F = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    pts = [np.asarray(p, np.float64) for p in P]; faces = list(F)
    for _ in range(bush_levels):
        nf = []; cache = {}
        def mid(i, j):
            key = (min(i, j), max(i, j))
            if key not in cache:
                m = pts[i] + pts[j]; pts.append(m / np.linalg.norm(m)); cache[key] = len(pts) - 1
            return cache[key]
        for (a, c, e) in faces:
            ab, ce, ea = mid(a, c), mid(c, e), mid(e, a); nf += [(a, ab, ea), (ab, c, ce), (ea, ce, e), (ab, ce, ea)]
        faces = nf
    for p in pts:
        r = 0.5 * (1.0 + 0.18 * math.sin(5 * p[0]) * math.cos(4 * p[1] + 1.0) + 0.1 * math.sin(7 * p[2]))
        q = p * r + np.array([0.0, 0.5, 0.0]); b.verts.append(tuple(map(float, q))); normals.append(tuple(map(float, p)))
    for (a, c, e) in faces: b.tris.append((base + a, base + c, base + e))
    b.end(leaf, face_normals=False, group=1)
    # group 1: crate (5 wooden faces) + metal lid
    def box(x0, y0, z0, x1, y1, z1, top):
        q = []
        if top: q.append([(x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)])
        else:
            q += [[(x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)], [(x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)],
                  [(x1, y0, z1), (x1, y1, z1), (x0, y1, z1), (x0, y0, z1)], [(x0, y0, z1), (x0, y1, z1), (x0, y1, z0), (x0, y0, z0)]]
        return q
    b.begin()
    for qd in box(-0.4, 0.0, -0.3, 0.4, 0.5, 0.3, False): b.quad(qd)
    n0 = len(b.verts); b.end(wood, group=2)
    b.begin()
    for qd in box(-0.4, 0.0, -0.3, 0.4, 0.5, 0.3, True): b.quad(qd)
    b.end(lid, group=2)
    normals += [(0.0, 1.0, 0.0)] * (len(b.verts) - len(normals))
    rng = np.random.default_rng(12345 + seed); inst = []
    for iz in range(n_side):
        for ix in range(n_side):
            x = (ix - (n_side - 1) / 2) * 2.6 + rng.uniform(-0.4, 0.4); z = (iz - (n_side - 1) / 2) * 2.6 + rng.uniform(-0.4, 0.4)
            g = int((ix + iz) % 2)
            m = translate(x, 0.0, z) @ rotate((0, 1, 0), rng.uniform(0, 360)) @ rotate((1, 0, 0), rng.uniform(-8, 8) if g == 0 else 0.0) @ \
                scale(rng.uniform(0.8, 1.5), rng.uniform(0.8, 1.6), rng.uniform(0.8, 1.5))
            inst.append(make_instance(g, m))
    cam = look_at((0.5, 4.5, -9.5), (0.0, 0.4, 0.0), (0, 1, 0))
    sc = finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 45.0, 0.05, 200.0, width, height, spp, sampler, max_depth, rr_depth,
                      seed=seed, normals=normals, name="instanced_garden", instances=inst)
    return add_scene_emitters(sc, [constant_emitter((0.25, 0.3, 0.4))])


def cbox_translucent(width=96, height=96, spp=16, sampler=SAMPLER_SOBOL, max_depth=10, rr_depth=5, seed=0, strict_normals=False, hide_emitters=False, frost_kw=None, slab_kw=None):
    """Cornell room with `roughdielectric` (frosted Beckmann sphere, GGX slab -- microfacet refraction, draws one extra sampler dimension per
    bounce) and a `difftrans` sheet in front of the back wall."""
    b = _Builder()
    white = b.bsdf(reflectance=(0.725, 0.71, 0.68)); red = b.bsdf(reflectance=(0.63, 0.065, 0.05)); green = b.bsdf(reflectance=(0.14, 0.45, 0.091))
    lightm = b.bsdf(reflectance=(0.78, 0.78, 0.78))
    frost = b.bsdf(kind=BSDF_ROUGHDIELECTRIC, ior=1.5046, reflectance=(0.97, 1.0, 0.95), specular=(1.0, 1.0, 1.0), **(frost_kw or dict(alpha=0.15, distr=DISTR_BECKMANN)))
    slab = b.bsdf(kind=BSDF_ROUGHDIELECTRIC, ior=1.33, reflectance=(0.8, 0.9, 1.0), specular=(0.9, 0.9, 0.9), **(slab_kw or dict(alpha=0.3, distr=DISTR_GGX)))   # the slab mesh has no uv: isotropic only
    shade = b.bsdf(kind=BSDF_DIFFTRANS, reflectance=(0.7, 0.55, 0.3))
    b.begin(); b.quad([(552.8, 0, 0), (0, 0, 0), (0, 0, 559.2), (549.6, 0, 559.2)]); b.end(white)
    b.begin(); b.quad([(556, 548.8, 0), (556, 548.8, 559.2), (0, 548.8, 559.2), (0, 548.8, 0)]); b.end(white)
    b.begin(); b.quad([(549.6, 0, 559.2), (0, 0, 559.2), (0, 548.8, 559.2), (556, 548.8, 559.2)]); b.end(white)
    b.begin(); b.quad([(0, 0, 559.2), (0, 0, 0), (0, 548.8, 0), (0, 548.8, 559.2)]); b.end(green)
    b.begin(); b.quad([(552.8, 0, 0), (549.6, 0, 559.2), (556, 548.8, 559.2), (556, 548.8, 0)]); b.end(red)
    b.begin(); b.quad([(343, 548.3, 227), (343, 548.3, 332), (213, 548.3, 332), (213, 548.3, 227)]); b.end(lightm, radiance=(17.0, 12.0, 4.0))
    b.begin()                                                              # closed slab (6 faces) so that rays enter and leave the medium
    x0, y0, z0, x1, y1, z1 = 330.0, 0.5, 200.0, 500.0, 240.0, 260.0
    b.quad([(x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)]); b.quad([(x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)])
    b.quad([(x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)]); b.quad([(x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)])
    b.quad([(x1, y0, z1), (x1, y1, z1), (x0, y1, z1), (x0, y0, z1)]); b.quad([(x0, y0, z1), (x0, y1, z1), (x0, y1, z0), (x0, y0, z0)])
    b.end(slab)
    b.begin(); b.quad([(60, 60, 500), (300, 60, 520), (300, 420, 520), (60, 420, 500)]); b.end(shade)
    b.add_analytic(SHAPE_SPHERE, translate(170, 100, 190), frost, radius=100.0)
    cam = look_at((278, 273, -800), (278, 273, -799), (0, 1, 0))
    return finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 39.3, 10.0, 2800.0, width, height, spp, sampler, max_depth, rr_depth,
                        seed=seed, strict_normals=strict_normals, hide_emitters=hide_emitters, name="cbox_translucent", analytic=b.resolve_analytic())


def cbox_roughplastic(width=96, height=96, spp=16, sampler=SAMPLER_SOBOL, max_depth=8, rr_depth=5, seed=0, strict_normals=False, sample_visible=True, phong=False):
    """Cornell box with `roughplastic` blocks and floor (Beckmann / GGX, linear and nonlinear; phong: all three with the Phong distribution), one of them `twosided`."""
    sc = cornell_box(width, height, spp, sampler, max_depth, rr_depth, seed=seed, strict_normals=strict_normals)
    sc.name = "cbox_roughplastic"
    mats = [make_bsdf(kind=BSDF_ROUGHPLASTIC, reflectance=(0.55, 0.5, 0.4), alpha=0.3, distr=DISTR_PHONG if phong else DISTR_BECKMANN, ior=1.49, nonlinear=True, sample_visible=sample_visible),      # floor
            make_bsdf(kind=BSDF_ROUGHPLASTIC, reflectance=(0.1, 0.3, 0.65), specular=(0.9, 0.9, 0.9), alpha=0.1, distr=DISTR_PHONG if phong else DISTR_GGX, ior=1.5046, sample_visible=sample_visible),     # short block
            make_bsdf(kind=BSDF_ROUGHPLASTIC, reflectance=(0.7, 0.25, 0.1), alpha=0.05, distr=DISTR_PHONG if phong else DISTR_BECKMANN, ior=1.9, twosided=True, sample_visible=sample_visible)]             # tall block
    base = len(sc.bsdfs); sc.bsdfs.extend(mats)
    sc.shapes[0]["bsdf"] = base; sc.shapes[6]["bsdf"] = base + 1; sc.shapes[7]["bsdf"] = base + 2
    tabs = []
    for bd in sc.bsdfs:
        if bd.get("table") is not None:
            off = sum(len(t) for t in tabs); tabs.append(bd["table"]); bd["k"] = (bd["k"][0], float(off), float(len(bd["table"])))
    sc.material_tables = np.concatenate(tabs).astype(f32)
    return sc


def textured_room(width=96, height=64, spp=16, sampler=SAMPLER_SOBOL, max_depth=6, rr_depth=4, seed=0):
    """Meshes WITH texture coordinates (shading frames from the UV tangents, TriMesh::computeUVTangents) and procedural 2-D textures on diffuse
    BSDFs: `checkerboard` floor (scaled / offset uv), `gridtexture` wall, a smooth-shaded textured mound, one mesh without texture; area light."""
    b = _Builder(); uvs = []; normals = []
    def quad_uv(pts, uv, n=(0.0, 1.0, 0.0)):
        b.quad(pts); uvs.extend(uv); normals.extend([n] * 4)
    tex = [make_texture(TEXTURE_CHECKERBOARD, (0.8, 0.75, 0.6), (0.15, 0.2, 0.3), uscale=6.0, vscale=4.0, uoffset=0.13, voffset=-0.2),
           make_texture(TEXTURE_GRID, (0.7, 0.3, 0.25), (0.05, 0.05, 0.05), line_width=0.06, uscale=5.0, vscale=5.0),
           make_texture(TEXTURE_CHECKERBOARD, (0.2, 0.6, 0.25), (0.9, 0.9, 0.2), uscale=3.0, vscale=3.0)]
    floor = b.bsdf(reflectance=(0.5, 0.5, 0.5)); b.bsdfs[floor]["texture"] = 0
    wall = b.bsdf(reflectance=(0.5, 0.5, 0.5), twosided=True); b.bsdfs[wall]["texture"] = 1
    mound = b.bsdf(reflectance=(0.5, 0.5, 0.5)); b.bsdfs[mound]["texture"] = 2
    plain = b.bsdf(reflectance=(0.6, 0.6, 0.65)); lightm = b.bsdf(reflectance=(0.5, 0.5, 0.5))
    b.begin(); quad_uv([(4, 0, -4), (-4, 0, -4), (-4, 0, 4), (4, 0, 4)], [(1, 0), (0, 0), (0, 1), (1, 1)]); b.end(floor)
    b.begin(); quad_uv([(-4, 0, 4), (-4, 3, 4), (4, 3, 4), (4, 0, 4)], [(0, 0), (0, 0.7), (1.3, 0.9), (1.1, 0.1)], (0, 0, -1)); b.end(wall)   # sheared uv: non-orthogonal tangents
    b.begin(); base = len(b.verts); nu, nv = 10, 6                                                                                        # mound: smooth normals + uv
    for j in range(nv + 1):
        for i in range(nu + 1):
            u, v = i / nu, j / nv; x = -1.5 + 3.0 * u; z = -0.5 + 2.0 * v; y = 0.9 * math.sin(math.pi * u) * math.sin(math.pi * v) + 0.01
            dydx = 0.9 * math.pi / 3.0 * math.cos(math.pi * u) * math.sin(math.pi * v); dydz = 0.9 * math.pi / 2.0 * math.sin(math.pi * u) * math.cos(math.pi * v)
            nn = np.array([-dydx, 1.0, -dydz]); nn /= np.linalg.norm(nn)
            b.verts.append((x, y, z)); uvs.append((u, v)); normals.append(tuple(map(float, nn)))
    for j in range(nv):
        for i in range(nu):
            a = base + j * (nu + 1) + i; c = a + 1; d_ = a + nu + 1; e = d_ + 1
            b.tris.append((a, d_, c)); b.tris.append((c, d_, e))
    b.end(mound, face_normals=False)
    b.begin(); quad_uv([(2.0, 0.0, -1.0), (2.0, 1.2, -1.0), (3.2, 1.2, -0.2), (3.2, 0.0, -0.2)], [(0, 0)] * 4, (0, 0, -1)); b.end(plain)
    b.shapes[-1]["has_uv"] = 0
    b.begin(); quad_uv([(1, 2.9, -1), (1, 2.9, 1), (-1, 2.9, 1), (-1, 2.9, -1)], [(0, 0), (1, 0), (1, 1), (0, 1)], (0, -1, 0)); b.end(lightm, radiance=(12.0, 11.0, 9.0))
    cam = look_at((0.3, 1.8, -5.5), (0.0, 0.7, 0.5), (0, 1, 0))
    return finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 50.0, 0.05, 100.0, width, height, spp, sampler, max_depth, rr_depth,
                        seed=seed, normals=normals, uvs=uvs, name="textured_room", textures=tex)


def wavy_sheet(n=32, phase=0.0, amp=0.15, lift=0.0, light_size=0.4, light_x=0.0, width=96, height=64, spp=4, sampler=SAMPLER_SOBOL, max_depth=5, rr_depth=4, seed=0):
    """A deformable mesh for the vertex-edit tests (Scene.update_vertices): the sheet y = lift + amp sin(3 x + phase) cos(2 z) over [-1, 1]^2 as n x n quads on a shared
    grid -- smooth normals, texture coordinates, a checkerboard on its diffuse BSDF, so the UV tangents matter -- under a two-triangle area light of half-width
    light_size at (light_x, lift + 1.5), over a plain floor.  Every call with the same n has the same indices, texture coordinates and shapes: only positions and
    normals depend on the other parameters."""
    b = _Builder(); uvs = []; normals = []
    tex = [make_texture(TEXTURE_CHECKERBOARD, (0.8, 0.75, 0.6), (0.15, 0.2, 0.3), uscale=5.0, vscale=3.0, uoffset=0.13, voffset=-0.2)]
    sheet = b.bsdf(reflectance=(0.5, 0.5, 0.5), twosided=True); b.bsdfs[sheet]["texture"] = 0
    plain = b.bsdf(reflectance=(0.6, 0.6, 0.65)); lightm = b.bsdf(reflectance=(0.5, 0.5, 0.5))
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1)); u = (i / n).reshape(-1); v = (j / n).reshape(-1); x = 2 * u - 1; z = 2 * v - 1
    y = lift + amp * np.sin(3 * x + phase) * np.cos(2 * z)
    dydx = amp * 3 * np.cos(3 * x + phase) * np.cos(2 * z); dydz = -amp * 2 * np.sin(3 * x + phase) * np.sin(2 * z); l = np.sqrt(dydx * dydx + 1 + dydz * dydz)
    b.begin(); b.verts.extend(zip(x.tolist(), y.tolist(), z.tolist())); uvs.extend(zip(u.tolist(), v.tolist())); normals.extend(zip((-dydx / l).tolist(), (1 / l).tolist(), (-dydz / l).tolist()))
    for jj in range(n):
        for ii in range(n):
            a = jj * (n + 1) + ii; c = a + 1; d_ = a + n + 1; e = d_ + 1
            b.tris.append((a, d_, c)); b.tris.append((c, d_, e))
    b.end(sheet, face_normals=False)
    h = lift + 1.5; s_ = light_size
    b.begin(); b.quad([(light_x + s_, h, -s_), (light_x + s_, h, s_), (light_x - s_, h, s_), (light_x - s_, h, -s_)]); uvs.extend([(0, 0)] * 4); normals.extend([(0, -1, 0)] * 4)
    b.end(lightm, radiance=(30.0, 27.0, 22.0)); b.shapes[-1]["has_uv"] = 0
    b.begin(); b.quad([(4, -0.6, -4), (-4, -0.6, -4), (-4, -0.6, 4), (4, -0.6, 4)]); uvs.extend([(0, 0)] * 4); normals.extend([(0, 1, 0)] * 4)
    b.end(plain); b.shapes[-1]["has_uv"] = 0
    cam = look_at((0.6, 3.0, -7.0), (0.0, 1.3, 0.0), (0, 1, 0))
    return finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 40.0, 0.05, 100.0, width, height, spp, sampler, max_depth, rr_depth,
                        seed=seed, normals=normals, uvs=uvs, name="wavy_sheet", textures=tex)


def bitmap_room(width=96, height=64, spp=16, sampler=SAMPLER_SOBOL, max_depth=6, rr_depth=4, seed=0):
    """The textured room with `bitmap` textures: EWA-filtered floor seen at grazing angles (anisotropic footprints, clamped anisotropy), trilinear
    wall with mirror / clamp wrapping, bilinear mound, nearest-neighbour panel.  Camera hits filter with the ray differentials
    (Intersection::computePartials); every later bounce reads level 0."""
    sc = textured_room(width, height, spp, sampler, max_depth, rr_depth, seed)
    pyr = load_texture_pyramid()
    tex = [make_texture(TEXTURE_BITMAP, pyramid=pyr, uscale=3.0, vscale=2.0, uoffset=0.1, filter_type=MIP_EWA),
           make_texture(TEXTURE_BITMAP, pyramid=pyr, uscale=1.7, vscale=1.3, wrap_u=WRAP_MIRROR, wrap_v=WRAP_CLAMP, filter_type=MIP_TRILINEAR),
           make_texture(TEXTURE_BITMAP, pyramid=pyr, uscale=1.0, vscale=1.0, filter_type=MIP_BILINEAR),
           make_texture(TEXTURE_BITMAP, pyramid=pyr, uscale=0.5, vscale=0.5, filter_type=MIP_NEAREST, wrap_u=WRAP_ZERO, wrap_v=WRAP_ONE)]
    sc.shapes[3]["has_uv"] = 1                     # the plain panel gets texcoords + the nearest-neighbour texture
    sc.uv[sc.shapes[3]["first_vert"]:sc.shapes[3]["first_vert"] + 4] = np.array([(-0.3, -0.2), (-0.3, 1.4), (1.6, 1.4), (1.6, -0.2)], f32)
    sc.bsdfs[3]["texture"] = 3
    out = finish_scene(sc.pos, sc.idx, sc.shapes, sc.bsdfs, sc.emitters, sc.cam_to_world, sc.xfov, sc.near, sc.far, width, height, spp, sampler, max_depth, rr_depth,
                       seed=seed, normals=sc.nrm, uvs=sc.uv, name="bitmap_room", textures=tex)
    return out


def normal_map_image(w=64, h=48):
    """A tangent-space normal map (RGB = 0.5 + 0.5 n) of a rippled height field, closed form."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64); u = (x + 0.5) / w; v = (y + 0.5) / h
    hx = 0.35 * np.cos(2 * np.pi * 3 * u) * np.sin(2 * np.pi * 2 * v); hy = 0.35 * np.sin(2 * np.pi * 3 * u) * np.cos(2 * np.pi * 2 * v)
    n = np.stack([-hx, -hy, np.ones_like(hx)], -1); n /= np.linalg.norm(n, axis=-1, keepdims=True)
    return np.ascontiguousarray((0.5 + 0.5 * n).astype(f32))


def layered_room(width=96, height=64, spp=16, sampler=SAMPLER_SOBOL, max_depth=6, rr_depth=4, seed=0, strict_normals=False, procedural_maps=False, fog=None):
    """The textured room with the three BSDF adapters of SURVEY §8 f2: `bumpmap` floor (bitmap displacement under a `scale` texture, bilinear gradient),
    `normalmap` wall over a twosided rough conductor, a `mixturebsdf` mound (plastic + diffuse), a twosided three-way mixture whose weights sum to
    1.4 (rescaled by the BSDF), a bump-mapped mixture (grid displacement: finite-difference gradient) and a mask over a bump-mapped diffuse.
    fog = INTEGRATOR_VOLPATH_SIMPLE / INTEGRATOR_VOLPATH: the room for the volumetric integrators -- the sensor sits in a thin medium that fills the room, a `null`
    sphere of denser forward-scattering haze hangs over the mound, and the masked sheet (refused in volumetric renders) is a plain bump-mapped one."""
    sc = textured_room(width, height, spp, sampler, max_depth, rr_depth, seed)
    pyr = load_texture_pyramid(); nimg = normal_map_image()
    tex = [make_texture(TEXTURE_BITMAP, pyramid=pyr, uscale=2.0, vscale=1.5, uoffset=0.05, filter_type=MIP_BILINEAR),
           make_texture(TEXTURE_BITMAP, pyramid=dict(base=nimg, levels=build_mip_pyramid(nimg, WRAP_REPEAT, WRAP_REPEAT)), uscale=1.5, vscale=1.0, filter_type=MIP_BILINEAR),
           make_texture(TEXTURE_CHECKERBOARD, (0.75, 0.7, 0.2), (0.15, 0.25, 0.6), uscale=4.0, vscale=4.0),
           make_texture(TEXTURE_GRID, (0.9, 0.9, 0.9), (0.1, 0.1, 0.1), line_width=0.08, uscale=3.0, vscale=3.0)]
    if procedural_maps:      # the same adapters over procedural maps only (a reference build without image codecs cannot serialise bitmap textures for the plugin adapter)
        tex[0] = make_texture(TEXTURE_GRID, (0.8, 0.8, 0.8), (0.2, 0.2, 0.2), line_width=0.11, uscale=5.0, vscale=4.0, uoffset=0.05)
        tex[1] = make_texture(TEXTURE_CHECKERBOARD, (0.5, 0.5, 1.0), (0.64, 0.42, 0.9), uscale=5.0, vscale=3.0)
    B = []
    def add(**kw): B.append(make_bsdf(**kw)); return len(B) - 1
    m0 = add(reflectance=(0.6, 0.6, 0.6))
    floor = add(kind=BSDF_BUMPMAP, nested=m0, texture=0, scale=0.25)
    m2 = add(kind=BSDF_ROUGHCONDUCTOR, alpha=0.2, distr=DISTR_GGX, eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14), twosided=True)
    wall = add(kind=BSDF_NORMALMAP, nested=m2, texture=1)
    m4 = add(kind=BSDF_PLASTIC, reflectance=(0.25, 0.5, 0.3), ior=1.49)
    m5 = add(reflectance=(0.45, 0.2, 0.6))
    mound = add(kind=BSDF_MIXTURE, nested=[m4, m5], weights=[0.7, 0.3])
    m7 = add(kind=BSDF_ROUGHCONDUCTOR, alpha=0.15, distr=DISTR_BECKMANN, eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14))
    m8 = add(reflectance=(0.7, 0.15, 0.1))
    panel = add(kind=BSDF_MIXTURE, nested=[m7, m8, m0], weights=[0.6, 0.5, 0.3], twosided=True)
    light = add(reflectance=(0.5, 0.5, 0.5))
    bumpmix = add(kind=BSDF_BUMPMAP, nested=mound, texture=3, scale=0.03)
    masked = add(kind=BSDF_MASK, reflectance=(0.55, 0.6, 0.7), nested=floor)
    shapes = [dict(s) for s in sc.shapes]
    for sh, m in zip(shapes, (floor, wall, mound, panel, light)): sh["bsdf"] = m
    shapes[3]["has_uv"] = 1
    uv = sc.uv.copy(); uv[shapes[3]["first_vert"]:shapes[3]["first_vert"] + 4] = np.array([(0, 0), (0, 1), (1, 1), (1, 0)], f32)
    # two more quads: a bump-mapped mixture leaning against the left side, a masked bump-mapped sheet in front of the mound
    verts = [tuple(v) for v in sc.pos]; tris = [tuple(t) for t in sc.idx]; nrm = [tuple(n) for n in sc.nrm]; uvl = [tuple(t) for t in uv]
    def quad(pts, n, mat):
        b0 = len(verts); verts.extend(pts); nrm.extend([n] * 4); uvl.extend([(0, 0), (0, 1), (1, 1), (1, 0)]); tris.extend([(b0, b0 + 1, b0 + 2), (b0, b0 + 2, b0 + 3)])
        shapes.append(dict(first_tri=len(tris) - 2, tri_count=2, first_vert=b0, vert_count=4, bsdf=mat, emitter=-1, face_normals=1, has_uv=1))
    quad([(-3.2, 0.0, 0.5), (-3.2, 1.6, 1.3), (-1.9, 1.6, 1.3), (-1.9, 0.0, 0.5)], (0.0, 0.0, -1.0), bumpmix)
    quad([(0.6, 0.0, -2.2), (0.6, 1.1, -2.2), (1.9, 1.1, -1.9), (1.9, 0.0, -1.9)], (0.0, 0.0, -1.0), floor if fog else masked)
    extra = {}
    if fog:
        B.pop()                                   # (the mask record: last one added, unused here)
        null = add(kind=BSDF_NULL)
        haze = make_analytic(SHAPE_SPHERE, translate(0.4, 1.5, -0.6), null, radius=0.8); haze["interior"] = 1; haze["exterior"] = 0
        extra = dict(media=[make_medium((0.004, 0.004, 0.006), (0.05, 0.05, 0.04)), make_medium((0.02, 0.01, 0.02), (0.5, 0.6, 0.5), phase=PHASE_HG, g=0.5)],
                     sensor_medium=0, integrator=fog, analytic=[haze])
    return finish_scene(verts, tris, shapes, B, sc.emitters, sc.cam_to_world, sc.xfov, sc.near, sc.far, width, height, spp, sampler, max_depth, rr_depth,
                        seed=seed, normals=nrm, uvs=uvl, name="layered_room", textures=tex, strict_normals=strict_normals, **extra)


def textured_plastics(width=96, height=64, spp=16, sampler=SAMPLER_SOBOL, max_depth=6, rr_depth=4, seed=0, rough=True):
    """The textured room with textures on the OTHER diffuse-like parameters: `plastic` floor (checkerboard diffuseReflectance, nonlinear), `roughplastic` wall
    (bitmap diffuseReflectance, trilinear), `difftrans` mound (grid transmittance), `roughplastic` panel (grid texture).  plastic / roughplastic pick their lobe
    with a weight derived from the texture's AVERAGE (plastic.cpp:204-207), evaluate with its local value."""
    sc = textured_room(width, height, spp, sampler, max_depth, rr_depth, seed)
    pyr = load_texture_pyramid()
    tex = [make_texture(TEXTURE_CHECKERBOARD, (0.8, 0.75, 0.6), (0.15, 0.2, 0.3), uscale=6.0, vscale=4.0, uoffset=0.13, voffset=-0.2),
           make_texture(TEXTURE_BITMAP, pyramid=pyr, uscale=1.7, vscale=1.3, wrap_u=WRAP_MIRROR, wrap_v=WRAP_CLAMP, filter_type=MIP_TRILINEAR),
           make_texture(TEXTURE_GRID, (0.2, 0.6, 0.25), (0.9, 0.9, 0.2), line_width=0.08, uscale=3.0, vscale=3.0),
           make_texture(TEXTURE_GRID, (0.7, 0.3, 0.25), (0.05, 0.05, 0.05), line_width=0.06, uscale=2.0, vscale=2.0)]
    bs = [make_bsdf(kind=BSDF_PLASTIC, ior=1.49, specular=(0.9, 0.9, 0.9), nonlinear=True),
          make_bsdf(kind=BSDF_ROUGHPLASTIC, alpha=0.1, distr=DISTR_GGX, ior=1.5046, specular=(0.9, 0.9, 0.9), twosided=True),
          make_bsdf(kind=BSDF_DIFFTRANS),
          make_bsdf(kind=BSDF_ROUGHPLASTIC, alpha=0.3, distr=DISTR_BECKMANN, ior=1.49, nonlinear=True)]
    if not rough:      # smooth plastics and procedural textures only: the reference's roughplastic needs its data/microfacet tables at run time, and its
        # BitmapTexture can only be serialised (= read by the adapter) in a build with OpenEXR
        tex[1] = make_texture(TEXTURE_CHECKERBOARD, (0.3, 0.5, 0.8), (0.85, 0.8, 0.7), uscale=5.0, vscale=3.0, uoffset=0.2)
        bs[1] = make_bsdf(kind=BSDF_PLASTIC, ior=1.5046, specular=(0.9, 0.9, 0.9), twosided=True); bs[3] = make_bsdf(kind=BSDF_PLASTIC, ior=1.9)
    for i, b in enumerate(bs):
        b["texture"] = i; sc.bsdfs[i] = b
    sc.shapes[3]["has_uv"] = 1
    sc.uv[sc.shapes[3]["first_vert"]:sc.shapes[3]["first_vert"] + 4] = np.array([(-0.3, -0.2), (-0.3, 1.4), (1.6, 1.4), (1.6, -0.2)], f32)
    return finish_scene(sc.pos, sc.idx, sc.shapes, sc.bsdfs, sc.emitters, sc.cam_to_world, sc.xfov, sc.near, sc.far, width, height, spp, sampler, max_depth, rr_depth,
                        seed=seed, normals=sc.nrm, uvs=sc.uv, name="textured_plastics", textures=tex)


def shape_lights(width=192, height=128, spp=16, sampler=SAMPLER_SOBOL, max_depth=6, rr_depth=4, seed=0):
    """Area lights on every analytic shape kind inside an inward-facing (`flipNormals`) sphere: a `sphere` light (cone sampling from
    outside, sphere.cpp:275-346), a `cylinder` light, a `disk` light and a `rectangle` light over a mesh floor and a mesh blocker."""
    b = _Builder()
    grey = b.bsdf(reflectance=(0.6, 0.6, 0.6))
    blue = b.bsdf(reflectance=(0.2, 0.3, 0.7), twosided=True)
    lm = b.bsdf(reflectance=(0.5, 0.5, 0.5))
    b.begin(); b.quad([(4, -1, -4), (-4, -1, -4), (-4, -1, 4), (4, -1, 4)]); b.end(grey)                        # floor (+y)
    b.begin(); b.quad([(-0.2, -1, 0.9), (0.9, -1, 0.4), (0.9, 0.3, 0.4), (-0.2, 0.3, 0.9)]); b.end(blue)         # standing blocker
    b.add_analytic(SHAPE_SPHERE, translate(0, 0.5, 0), grey, flip=True, radius=5.0)                              # the room
    b.add_analytic(SHAPE_SPHERE, translate(-1.4, 0.2, 1.0), lm, radiance=(9.0, 7.0, 5.0), radius=0.35)
    m, length = cylinder_to_world((1.2, -0.6, 1.6), (2.0, 0.9, 1.2))
    b.add_analytic(SHAPE_CYLINDER, m, lm, radiance=(2.0, 6.0, 3.0), radius=0.12, length=length)
    b.add_analytic(SHAPE_DISK, translate(0.3, 2.2, 0.5) @ rotate((1, 0, 0), 90) @ rotate((0, 0, 1), 20) @ scale(0.5), lm, radiance=(3.0, 3.0, 8.0))
    b.add_analytic(SHAPE_RECTANGLE, translate(-2.5, 0.4, 2.8) @ rotate((0, 1, 0), 140) @ scale(0.6, 0.4, 1), lm, radiance=(6.0, 2.0, 2.0))
    cam = look_at((0.2, 0.6, -3.6), (0.0, 0.1, 0.5), (0, 1, 0))
    return finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 60.0, 0.05, 100.0, width, height, spp, sampler, max_depth, rr_depth,
                        seed=seed, name="shape_lights", analytic=b.resolve_analytic())


def closed_box(width=128, height=128, spp=16, sampler=SAMPLER_SOBOL, max_depth=8):
    """The survey probe scene: closed 24-triangle diffuse cube room + small ceiling light,
    camera inside. Every path stays inside, so avg path length is the reference's 6.10 figure."""
    b = _Builder()
    grey = b.bsdf(reflectance=(0.5, 0.5, 0.5))
    lightm = b.bsdf(reflectance=(0.5, 0.5, 0.5))
    L = 2.0
    b.begin()
    b.quad([(L, -L, -L), (-L, -L, -L), (-L, -L, L), (L, -L, L)])      # floor  (+y)
    b.quad([(L, L, -L), (L, L, L), (-L, L, L), (-L, L, -L)])          # ceiling (-y)
    b.quad([(L, -L, L), (-L, -L, L), (-L, L, L), (L, L, L)])          # back z=+L (-z)
    b.quad([(-L, -L, -L), (L, -L, -L), (L, L, -L), (-L, L, -L)])      # front z=-L (+z)
    b.quad([(-L, -L, L), (-L, -L, -L), (-L, L, -L), (-L, L, L)])      # x=-L (+x)
    b.quad([(L, -L, -L), (L, -L, L), (L, L, L), (L, L, -L)])          # x=+L (-x)
    b.end(grey)
    b.begin(); b.quad([(0.5, 1.9, -0.5), (0.5, 1.9, 0.5), (-0.5, 1.9, 0.5), (-0.5, 1.9, -0.5)])
    b.end(lightm, radiance=(20.0, 20.0, 20.0))
    cam = look_at((0, 0, -1.9), (0, 0, 0), (0, 1, 0))
    return finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 70.0, 0.01, 100.0,
                        width, height, spp, sampler, max_depth, name="closed_box")


def _grid_room(b, L, n):
    """closed cube room [-L, L]^3, every wall an n x n grid of quads (normals face the room)"""
    def wall(origin, eu, ev):
        o, u, v = (np.asarray(a, np.float64) for a in (origin, eu, ev))
        for j in range(n):
            for i in range(n):
                b.quad([o + u * (i / n) + v * (j / n), o + u * ((i + 1) / n) + v * (j / n), o + u * ((i + 1) / n) + v * ((j + 1) / n), o + u * (i / n) + v * ((j + 1) / n)])
    D = 2 * L
    wall((L, -L, -L), (-D, 0, 0), (0, 0, D)); wall((L, L, -L), (0, 0, D), (-D, 0, 0))      # floor (+y), ceiling (-y)
    wall((L, -L, L), (-D, 0, 0), (0, D, 0)); wall((-L, -L, -L), (D, 0, 0), (0, D, 0))      # z = +L (-z), z = -L (+z)
    wall((-L, -L, L), (0, 0, -D), (0, D, 0)); wall((L, -L, -L), (0, 0, D), (0, D, 0))      # x = -L (+x), x = +L (-x)


SPECK_EXTENT = 6e-6


def speck_room(width=64, height=64, spp=4, sampler=SAMPLER_SOBOL, max_depth=4, room=120.0, patch=3):
    """Small geometry seen from far away (tests of the tree walks): a closed room of 6 * 3 * 3 * 2 = 108 triangles with a ceiling light, and at the world origin --
    where fp32 resolves it -- a "speck": a patch of patch x patch quads (18 triangles) of extent SPECK_EXTENT in the plane y = 0.  The speck's tree nodes are
    so small that, from a distance t beyond ~SPECK_EXTENT / 1e-6, the 2e-6 * t slack of the conservative box tests is larger than the nodes themselves.
    The patch is perpendicular to the axis its Wald records project along: from that far the Wald test rounds t by more than a triangle, and only then does a ray with
    a zero direction component keep one answer whatever the tree's leaf padding (tests/test_gpu_fused_walk.py test_speck_rays_short_of_the_slack)."""
    b = _Builder(); grey = b.bsdf(reflectance=(0.5, 0.5, 0.5)); lightm = b.bsdf(reflectance=(0.5, 0.5, 0.5)); L = float(room)
    b.begin(); _grid_room(b, L, 3); b.end(grey)
    b.begin(); b.quad([(0.2 * L, 0.95 * L, -0.2 * L), (0.2 * L, 0.95 * L, 0.2 * L), (-0.2 * L, 0.95 * L, 0.2 * L), (-0.2 * L, 0.95 * L, -0.2 * L)]); b.end(lightm, radiance=(20.0, 20.0, 20.0))
    h = SPECK_EXTENT / 2
    def pt(i, j):
        return (-h + 2 * h * i / patch, 0.0, -h + 2 * h * j / patch)
    b.begin()
    for j in range(patch):
        for i in range(patch): b.quad([pt(i, j), pt(i, j + 1), pt(i + 1, j + 1), pt(i + 1, j)])
    b.end(grey)
    cam = look_at((0, 0, -0.9 * L), (0, 0, 0), (0, 1, 0))
    return finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 60.0, 0.01, 10 * L, width, height, spp, sampler, max_depth, name="speck_room")


def sliver_stack(width=64, height=64, spp=4, sampler=SAMPLER_SOBOL, max_depth=4, side=64, spacing=2e-3):
    """A tree whose boxes all overlap (tests of the traversal stacks): side x side long thin triangles, each spanning the diagonal of the unit cube, shifted sideways on
    a grid of `spacing`, so every triangle's box -- and every tree node's -- is nearly the whole cube: a ray through the cube meets nearly every box and almost no
    triangle, and the walk descends the full depth of the tree with every sibling waiting on its stack.  A floor and a light around it make it renderable."""
    b = _Builder(); grey = b.bsdf(reflectance=(0.5, 0.5, 0.5)); lightm = b.bsdf(reflectance=(0.5, 0.5, 0.5))
    diag = np.array([1.0, 1.0, 1.0]); e1 = np.array([1.0, -1.0, 0.0]) / math.sqrt(2.0); e2 = np.array([1.0, 1.0, -2.0]) / math.sqrt(6.0)
    b.begin()
    for j in range(side):
        for i in range(side):
            off = e1 * ((i - (side - 1) / 2) * spacing) + e2 * ((j - (side - 1) / 2) * spacing)
            base = len(b.verts); b.verts.extend([tuple(off), tuple(off + diag), tuple(off + diag + e1 * (0.75 * spacing))]); b.tris.append((base, base + 1, base + 2))
    b.end(grey)
    b.begin(); b.quad([(3, -0.5, -2), (-2, -0.5, -2), (-2, -0.5, 3), (3, -0.5, 3)]); b.end(grey)                                                  # floor (+y)
    b.begin(); b.quad([(1.5, 3.0, -0.5), (1.5, 3.0, 1.5), (-0.5, 3.0, 1.5), (-0.5, 3.0, -0.5)]); b.end(lightm, radiance=(20.0, 20.0, 20.0))      # light (-y)
    cam = look_at((2.5, 1.2, -1.5), (0.5, 0.5, 0.5), (0, 1, 0))
    return finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 50.0, 0.01, 100.0, width, height, spp, sampler, max_depth, name="sliver_stack")


# conductor eta / k as linear RGB, produced by the reference itself from data/ior/<name>.{eta,k}.spd (RoughConductor constructor,
# src/bsdfs/roughconductor.cpp:177-189; dumped by oracle/_ref/harness `tables` -> tests/golden/conductor_ior_rgb.npy)
CONDUCTOR_IOR = {
    "Cu": ((0.20043588, 0.9240331, 1.1022109), (3.9129362, 2.452853, 2.1421824)),
    "Al": ((1.6574619, 0.88036764, 0.5212283), (9.223862, 6.2695246, 4.8370023)),
    "Au": ((0.14312422, 0.3749563, 1.4424754), (3.9831533, 2.3857234, 1.6032081)),
}


def _disc(b, center, normal, radius, n=32):
    """Triangle fan of n triangles, wound so that cross(p1-p0, p2-p0) points along `normal`."""
    c = np.asarray(center, np.float64); nrm = np.asarray(normal, np.float64); nrm = nrm / np.linalg.norm(nrm)
    t = np.cross(nrm, [1.0, 0.0, 0.0]); t = t / np.linalg.norm(t); bt = np.cross(nrm, t)
    base = len(b.verts)
    b.verts.append(tuple(map(float, c)))
    for i in range(n):
        a = 2.0 * math.pi * i / n
        b.verts.append(tuple(map(float, c + radius * (math.cos(a) * t + math.sin(a) * bt))))
    for i in range(n):
        b.tris.append((base, base + 1 + i, base + 1 + (i + 1) % n))


def veach_mis(width=1920, height=1080, spp=512, sampler=SAMPLER_SOBOL, max_depth=12, rr_depth=5, filter_kind=FILTER_BOX, microfacets=None, seed=0):
    """S2: Veach's multiple-importance-sampling test -- four tilted plates of increasing roughness
    (`twosided(roughconductor)`, Beckmann alpha 0.005 / 0.02 / 0.05 and GGX 0.1) reflecting four disc lights of radii
    0.03 / 0.1 / 0.3 / 0.9 with power-equalised radiance, over a diffuse floor and back wall; 140 triangles."""
    b = _Builder()
    grey = b.bsdf(reflectance=(0.4, 0.4, 0.4))
    al, cu = CONDUCTOR_IOR["Al"], CONDUCTOR_IOR["Cu"]
    plates = [
        ([(4, -2.70651, 0.25609), (4, -2.08375, -0.526323), (-4, -2.08375, -0.526323), (-4, -2.70651, 0.25609)], 0.005, DISTR_BECKMANN, al),
        ([(4, -3.28825, 1.36972), (4, -2.83856, 0.476536), (-4, -2.83856, 0.476536), (-4, -3.28825, 1.36972)], 0.02, DISTR_BECKMANN, al),
        ([(4, -3.73096, 2.70046), (4, -3.43378, 1.74564), (-4, -3.43378, 1.74564), (-4, -3.73096, 2.70046)], 0.05, DISTR_BECKMANN, cu),
        ([(4, -3.99615, 4.0667), (4, -3.82069, 3.08221), (-4, -3.82069, 3.08221), (-4, -3.99615, 4.0667)], 0.1, DISTR_GGX, cu),
    ]
    b.begin(); b.quad([(-10, -4.14615, -10), (-10, -4.14615, 10), (10, -4.14615, 10), (10, -4.14615, -10)]); b.end(grey)     # floor (+y)
    b.begin(); b.quad([(-10, -10, -2), (10, -10, -2), (10, 10, -2), (-10, 10, -2)]); b.end(grey)                           # back wall (+z)
    plate_shapes = []
    for pi, (pts, alpha, distr, (eta, k)) in enumerate(plates):
        kw = dict(alpha=alpha, distr=distr)
        if microfacets is not None:                  # per-plate overrides: alpha, alpha_v, distr, sample_visible (the full MicrofacetDistribution of src/bsdfs/microfacet.h)
            kw.update(microfacets[pi])
        m = b.bsdf(kind=BSDF_ROUGHCONDUCTOR, twosided=True, eta=eta, k=k, **kw)
        b.begin(); b.quad(pts); b.end(m)
        plate_shapes.append(len(b.shapes) - 1)
    lightm = b.bsdf(reflectance=(0.0, 0.0, 0.0))
    for x, r, tint in [(-3.75, 0.03, (1.0, 0.6, 0.6)), (-1.25, 0.1, (1.0, 1.0, 0.6)), (1.25, 0.3, (0.6, 1.0, 0.6)), (3.75, 0.9, (0.6, 0.6, 1.0))]:
        rad = 8.0 / (math.pi * r * r)
        b.begin(); _disc(b, (x, 0.0, 0.0), (0.0, -0.8, 0.6), r); b.end(lightm, radiance=tuple(rad * t for t in tint))
    b.begin(); b.quad([(-3, 8, 0), (3, 8, 0), (3, 8, 6), (-3, 8, 6)]); b.end(lightm, radiance=(1.5, 1.5, 1.5))             # dim fill light (-y)
    cam = look_at((0, 2, 15), (0, -2, 2.5), (0, 1, 0))
    uvs = None
    if microfacets is not None:                      # anisotropic BSDFs need texture coordinates: the tangent is dp/du (TriMesh::configure, trimesh.cpp:380-382)
        uvs = np.zeros((len(b.verts), 2), f32)
        for sh in b.shapes: sh["has_uv"] = 0
        for k_, si in enumerate(plate_shapes):
            sh = b.shapes[si]; sh["has_uv"] = 1
            quad = [(0, 0), (0, 1), (1, 1), (1, 0)] if k_ % 2 == 0 else [(0.2, 0), (0, 0.8), (0.9, 1), (1, 0.1)]       # every other plate: sheared uv, tangent off the plate's edge
            uvs[sh["first_vert"]:sh["first_vert"] + 4] = quad
    return finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 28.0, 0.1, 100.0,
                        width, height, spp, sampler, max_depth, rr_depth, filter_kind, seed=seed, uvs=uvs, name="veach_mis")


def procedural_sky(w=1024, h=512):
    """Closed-form lat-long sky: blue-to-white gradient above the horizon, dim ground below, one sun lobe.  Texels are rounded to
    half precision because the reference stores its environment MIP map in half floats (src/emitters/envmap.cpp:103-104)."""
    v = (np.arange(h, dtype=np.float64) + 0.5) / h; u = (np.arange(w, dtype=np.float64) + 0.5) / w
    theta = v[:, None] * math.pi; phi = u[None, :] * 2 * math.pi
    d = np.stack([np.sin(phi) * np.sin(theta), np.cos(theta) * np.ones_like(phi), -np.cos(phi) * np.sin(theta)], -1)   # envmap.cpp:604
    up = np.clip(d[..., 1], 0, 1)
    sky = (1 - up[..., None]) * np.array([0.9, 0.95, 1.0]) + up[..., None] * np.array([0.25, 0.45, 0.9])
    ground = np.array([0.08, 0.07, 0.06])
    rgb = np.where(d[..., 1:2] > 0, sky, ground)
    sun = np.array([0.35, 0.8, -0.45]); sun = sun / np.linalg.norm(sun)
    c = np.clip((d * sun).sum(-1), 0, 1)
    rgb = rgb + (60.0 * c ** 400 + 1.5 * c ** 30)[..., None] * np.array([1.0, 0.9, 0.75])
    return rgb.astype(np.float16).astype(f32)


def _lcg(seed):
    state = [seed & 0xFFFFFFFF]
    def nxt():
        state[0] = (1664525 * state[0] + 1013904223) & 0xFFFFFFFF
        return state[0] / 4294967296.0
    return nxt


def atrium(width=3840, height=2160, spp=64, sampler=SAMPLER_SOBOL, max_depth=8, detail=1.0, env_size=(1024, 512), sky_visible=True,
           filter_kind=FILTER_BOX, strict_normals=False, hide_emitters=False, rr_depth=5, seed=0):
    """S3: procedurally generated Sponza-class colonnade / atrium.  A 36 x 24 m tiled floor (per-tile diffuse colours from
    an LCG seeded 1234, 16-colour palette), two rows of tessellated columns with SMOOTH vertex normals, four walls, a gallery slab with an
    open roof, two emissive lanterns and a procedural sky environment map.  detail = 1 gives ~250 k triangles."""
    rnd = _lcg(1234)
    b = _Builder(); normals = []
    def pad_normals():
        while len(normals) < len(b.verts): normals.append((0.0, 0.0, 0.0))
    palette = [b.bsdf(reflectance=(0.25 + 0.5 * rnd(), 0.25 + 0.5 * rnd(), 0.25 + 0.5 * rnd())) for _ in range(16)]
    stone = b.bsdf(reflectance=(0.62, 0.58, 0.5)); wall = b.bsdf(reflectance=(0.7, 0.66, 0.6), twosided=True); lightm = b.bsdf(reflectance=(0.0, 0.0, 0.0))
    X, Z, Hh = 18.0, 12.0, 9.0
    # floor tiles grouped by palette entry (one mesh per colour)
    nx, nz = max(2, int(round(144 * detail))), max(2, int(round(72 * detail)))
    tiles = [[] for _ in palette]
    for iz in range(nz):
        for ix in range(nx):
            tiles[int(rnd() * 16) % 16].append((ix, iz))
    for pi, lst in enumerate(tiles):
        if not lst: continue
        b.begin()
        for ix, iz in lst:
            x0, x1 = -X + 2 * X * ix / nx, -X + 2 * X * (ix + 1) / nx; z0, z1 = -Z + 2 * Z * iz / nz, -Z + 2 * Z * (iz + 1) / nz
            b.quad([(x1, 0, z0), (x0, 0, z0), (x0, 0, z1), (x1, 0, z1)])                       # +y
        b.end(palette[pi]); pad_normals()
    # walls (two-sided), gallery slab with a rectangular opening
    b.begin()
    b.quad([(-X, 0, -Z), (X, 0, -Z), (X, Hh, -Z), (-X, Hh, -Z)]); b.quad([(X, 0, Z), (-X, 0, Z), (-X, Hh, Z), (X, Hh, Z)])
    b.quad([(-X, 0, Z), (-X, 0, -Z), (-X, Hh, -Z), (-X, Hh, Z)]); b.quad([(X, 0, -Z), (X, 0, Z), (X, Hh, Z), (X, Hh, -Z)])
    ox, oz = (X * 0.55, Z * 0.45) if sky_visible else (0.0, 0.0)
    if sky_visible:
        for (x0, x1, z0, z1) in [(-X, X, -Z, -oz), (-X, X, oz, Z), (-X, -ox, -oz, oz), (ox, X, -oz, oz)]:
            b.quad([(x0, Hh, z0), (x1, Hh, z0), (x1, Hh, z1), (x0, Hh, z1)])                   # ceiling ring (-y side visible from below, two-sided)
    else:
        b.quad([(-X, Hh, -Z), (X, Hh, -Z), (X, Hh, Z), (-X, Hh, Z)])
    b.end(wall); pad_normals()
    # columns: smooth cylinders
    ncol = 10; seg = max(6, int(round(48 * detail))); rings = max(2, int(round(120 * detail)))
    for row_z in (-Z * 0.55, Z * 0.55):
        for c in range(ncol):
            cx = -X * 0.85 + 2 * X * 0.85 * c / (ncol - 1); r = 0.55; h = Hh
            b.begin(); base = len(b.verts)
            for j in range(rings + 1):
                y = h * j / rings; rr = r * (1.0 - 0.12 * (j / rings))                        # slight taper
                for i in range(seg):
                    a = 2 * math.pi * i / seg
                    b.verts.append((cx + rr * math.cos(a), y, row_z + rr * math.sin(a)))
                    n = np.array([math.cos(a), 0.12 * r / h, math.sin(a)]); n = n / np.linalg.norm(n); normals.append(tuple(map(float, n)))
            for j in range(rings):
                for i in range(seg):
                    v00 = base + j * seg + i; v01 = base + j * seg + (i + 1) % seg; v10 = v00 + seg; v11 = v01 + seg
                    b.tris.append((v00, v10, v11)); b.tris.append((v00, v11, v01))                # outward
            b.end(stone, face_normals=False)
    # lanterns
    for lx in (-X * 0.5, X * 0.5):
        b.begin(); b.quad([(lx - 0.6, Hh - 0.4, -0.6), (lx + 0.6, Hh - 0.4, -0.6), (lx + 0.6, Hh - 0.4, 0.6), (lx - 0.6, Hh - 0.4, 0.6)])   # -y
        b.end(lightm, radiance=(18.0, 14.0, 9.0)); pad_normals()
    cam = look_at((-X * 0.8, 3.2, 0.5), (X * 0.2, 1.2, -1.0), (0, 1, 0))
    env = dict(rgb=procedural_sky(*env_size), to_world=np.eye(4, dtype=f32), scale=1.0)
    sc = finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 60.0, 0.05, 500.0, width, height, spp, sampler, max_depth,
                      rr_depth, filter_kind, seed, normals=normals, envmap=env, strict_normals=strict_normals, hide_emitters=hide_emitters, name="atrium")
    # the environment emitter is a scene-level emitter: it comes first in Scene::getEmitters() (added before the shapes are expanded)
    sc.emitters.insert(0, dict(type=EMITTER_ENVMAP, shape=-1, radiance=(0.0, 0.0, 0.0), weight=1.0))
    for sh in sc.shapes:
        if sh["emitter"] >= 0: sh["emitter"] += 1
    return sc


def add_scene_emitters(sc, emitters):
    """Prepend scene-level emitters (envmap / constant / point / spot / directional): Scene::m_emitters lists them before the area lights of
    the shapes when they are declared first (harness order), so the indices of the area lights shift."""
    k = len(emitters)
    for sh in sc.shapes:
        if sh["emitter"] >= 0: sh["emitter"] += k
    for a in sc.get("analytic") or []:
        if a["emitter"] >= 0: a["emitter"] += k
    sc.emitters[0:0] = emitters
    return sc


def constant_emitter(radiance, weight=1.0):
    return dict(type=EMITTER_CONSTANT, shape=-1, radiance=tuple(map(float, radiance)), weight=float(weight))


def point_emitter(position, intensity, weight=1.0):
    return dict(type=EMITTER_POINT, shape=-1, radiance=tuple(map(float, intensity)), weight=float(weight), to_world=translate(*position).astype(f32))


def spot_emitter(origin, target, intensity, cutoff=20.0, beam=None, up=(0, 1, 0), weight=1.0):
    return dict(type=EMITTER_SPOT, shape=-1, radiance=tuple(map(float, intensity)), weight=float(weight), to_world=look_at(origin, target, up),
                cutoff=float(cutoff), beam=float(cutoff * 0.75 if beam is None else beam))


def collimated_emitter(origin, target, power, up=(0, 1, 0), weight=1.0):
    """src/emitters/collimated.cpp: a beam from `origin` towards `target`.  Direct sampling of a 0-D emitter always fails, so a unidirectional path tracer never
    receives its light -- it only takes its share of the emitter-selection probability."""
    return dict(type=EMITTER_COLLIMATED, shape=-1, radiance=tuple(map(float, power)), weight=float(weight), to_world=look_at(origin, target, up))


def directional_emitter(direction, irradiance, weight=1.0):
    """direction = where the light travels; toWorld = lookAt(0, d, u) with u from coordinateSystem(d) (directional.cpp:64-67)."""
    d = np.asarray(direction, f32); d = (d / np.sqrt(np.dot(d, d), dtype=f32)).astype(f32)
    u, _ = _coordinate_system(d)
    return dict(type=EMITTER_DIRECTIONAL, shape=-1, radiance=tuple(map(float, irradiance)), weight=float(weight), to_world=look_at((0, 0, 0), d, u))


EMITTER_SUNSKY = 6     # src/emitters/sunsky.cpp -- a compound emitter of the reference: it rasterises the Hosek-Wilkie sky (+ sun disc) into an `envmap` (and a `directional`
                       # sun for sunRadiusScale = 0).  Not restated here: a scene naming it can only be handed to a reference build (oracle/ref_build/harness), where the
                       # drop-in plugin sees the expanded elements; mi.Scene / the oracle refuse it


def sunsky_emitter(sun_direction, turbidity=3.0, scale=1.0, sun_radius_scale=1.0, resolution=256, weight=1.0):
    d = np.asarray(sun_direction, f32); d = d / f32(np.linalg.norm(d)); m = np.eye(4, dtype=f32); m[:3, 2] = d
    return dict(type=EMITTER_SUNSKY, shape=-1, radiance=(float(turbidity), float(scale), float(sun_radius_scale)), weight=float(weight), cutoff=float(resolution), beam=0.0, to_world=m)


def sunsky_terrace(width=96, height=64, spp=16, sampler=SAMPLER_SOBOL, max_depth=6, rr_depth=4, seed=0, sun_radius_scale=1.0):
    """the open_constant geometry under the reference's `sunsky` emitter (drop-in tests only: EMITTER_SUNSKY)"""
    sc = open_constant(width, height, spp, sampler, max_depth, rr_depth, seed); sc.name = "sunsky_terrace"
    sc.emitters = [e for e in sc.emitters if e["type"] == EMITTER_AREA]
    return add_scene_emitters(sc, [sunsky_emitter((0.35, 0.6, -0.4), turbidity=3.0, scale=1.0, sun_radius_scale=sun_radius_scale, resolution=128)])


def cbox_lights(width=96, height=96, spp=16, sampler=SAMPLER_SOBOL, max_depth=8, rr_depth=5, seed=0, hide_emitters=False):
    """Cornell box lit by its area light plus a `point` and a `spot` emitter (emitter selection over three kinds; delta lights: MIS weight 1)."""
    sc = cornell_box(width, height, spp, sampler, max_depth, rr_depth, seed=seed, hide_emitters=hide_emitters)
    sc.name = "cbox_lights"
    return add_scene_emitters(sc, [point_emitter((120, 420, 150), (4e5, 5e5, 9e5)),
                                   spot_emitter((430, 500, 100), (300, 0, 330), (3e6, 2.2e6, 1.2e6), cutoff=28.0, beam=17.0)])


def cbox_collimated(width=96, height=96, spp=16, sampler=SAMPLER_SOBOL, max_depth=8, rr_depth=5, seed=0):
    """cbox_lights plus a `collimated` beam: four emitters in the selection CDF, one of which never returns a sample (collimated.cpp:129-133)."""
    sc = cornell_box(width, height, spp, sampler, max_depth, rr_depth, seed=seed)
    sc.name = "cbox_collimated"
    return add_scene_emitters(sc, [point_emitter((120, 420, 150), (4e5, 5e5, 9e5)), collimated_emitter((278, 540, 280), (278, 0, 280), (50.0, 50.0, 50.0), up=(0, 0, 1), weight=1.5),
                                   spot_emitter((430, 500, 100), (300, 0, 330), (3e6, 2.2e6, 1.2e6), cutoff=28.0, beam=17.0)])


def cbox_roughdiffuse(width=96, height=96, spp=16, sampler=SAMPLER_SOBOL, max_depth=8, rr_depth=5, seed=0, strict_normals=False):
    """Cornell box with `roughdiffuse` (Oren-Nayar) walls, floor and blocks: the full model and the qualitative approximation (useFastApprox), one of them `twosided`."""
    sc = cornell_box(width, height, spp, sampler, max_depth, rr_depth, seed=seed, strict_normals=strict_normals)
    sc.name = "cbox_roughdiffuse"
    mats = [make_bsdf(kind=BSDF_ROUGHDIFFUSE, reflectance=(0.725, 0.71, 0.68), alpha=0.2),                      # floor (full model)
            make_bsdf(kind=BSDF_ROUGHDIFFUSE, reflectance=(0.725, 0.71, 0.68), alpha=0.7, distr=1),             # back wall (fast approximation)
            make_bsdf(kind=BSDF_ROUGHDIFFUSE, reflectance=(0.14, 0.45, 0.091), alpha=0.45),                     # right wall
            make_bsdf(kind=BSDF_ROUGHDIFFUSE, reflectance=(0.2, 0.35, 0.7), alpha=1.0, distr=1, twosided=True), # short block
            make_bsdf(kind=BSDF_ROUGHDIFFUSE, reflectance=(0.8, 0.6, 0.2), alpha=0.05)]                         # tall block
    base = len(sc.bsdfs); sc.bsdfs.extend(mats)
    sc.shapes[0]["bsdf"] = base; sc.shapes[2]["bsdf"] = base + 1; sc.shapes[3]["bsdf"] = base + 2; sc.shapes[6]["bsdf"] = base + 3; sc.shapes[7]["bsdf"] = base + 4
    return sc


def cbox_phong(width=96, height=96, spp=16, sampler=SAMPLER_SOBOL, max_depth=8, rr_depth=5, seed=0, strict_normals=False):
    """Cornell box with modified-`phong` floor, back wall and blocks (exponents 5 .. 300, one `twosided`, one purely specular-dominated)."""
    sc = cornell_box(width, height, spp, sampler, max_depth, rr_depth, seed=seed, strict_normals=strict_normals)
    sc.name = "cbox_phong"
    mats = [make_bsdf(kind=BSDF_PHONG, reflectance=(0.5, 0.5, 0.5), specular=(0.2, 0.2, 0.2), alpha=30.0),                      # floor (the plugin's defaults)
            make_bsdf(kind=BSDF_PHONG, reflectance=(0.3, 0.28, 0.25), specular=(0.6, 0.6, 0.65), alpha=300.0),                  # back wall
            make_bsdf(kind=BSDF_PHONG, reflectance=(0.1, 0.3, 0.6), specular=(0.3, 0.2, 0.1), alpha=5.0, twosided=True),        # short block
            make_bsdf(kind=BSDF_PHONG, reflectance=(0.02, 0.02, 0.02), specular=(0.9, 0.7, 0.3), alpha=80.0)]                   # tall block
    base = len(sc.bsdfs); sc.bsdfs.extend(mats)
    sc.shapes[0]["bsdf"] = base; sc.shapes[2]["bsdf"] = base + 1; sc.shapes[6]["bsdf"] = base + 2; sc.shapes[7]["bsdf"] = base + 3
    return sc


def cbox_ward(width=96, height=96, spp=16, sampler=SAMPLER_SOBOL, max_depth=8, rr_depth=5, seed=0, strict_normals=False):
    """Cornell box with `ward` floor, back wall and blocks: the three variants, one `twosided` (isotropic: the box has no texture coordinates; ward_room has the anisotropic ones)."""
    sc = cornell_box(width, height, spp, sampler, max_depth, rr_depth, seed=seed, strict_normals=strict_normals)
    sc.name = "cbox_ward"
    mats = [make_bsdf(kind=BSDF_WARD, reflectance=(0.5, 0.5, 0.5), specular=(0.2, 0.2, 0.2), alpha=0.1, distr=WARD_BALANCED),                          # floor (the plugin's defaults)
            make_bsdf(kind=BSDF_WARD, reflectance=(0.3, 0.28, 0.25), specular=(0.6, 0.6, 0.65), alpha=0.05, distr=WARD_BALANCED),                        # back wall
            make_bsdf(kind=BSDF_WARD, reflectance=(0.1, 0.3, 0.6), specular=(0.3, 0.2, 0.1), alpha=0.4, distr=WARD_WARD, twosided=True),                 # short block
            make_bsdf(kind=BSDF_WARD, reflectance=(0.05, 0.05, 0.05), specular=(0.9, 0.7, 0.3), alpha=0.2, distr=WARD_DUER)]                             # tall block
    base = len(sc.bsdfs); sc.bsdfs.extend(mats)
    sc.shapes[0]["bsdf"] = base; sc.shapes[2]["bsdf"] = base + 1; sc.shapes[6]["bsdf"] = base + 2; sc.shapes[7]["bsdf"] = base + 3
    return sc


def ward_room(width=96, height=64, spp=16, sampler=SAMPLER_SOBOL, max_depth=6, rr_depth=4, seed=0):
    """The textured room (meshes with texture coordinates: shading frames from the UV tangents) with ANISOTROPIC `ward` on the wall and the mound."""
    sc = textured_room(width, height, spp, sampler, max_depth, rr_depth, seed=seed)
    sc.name = "ward_room"
    sc.bsdfs[2] = make_bsdf(kind=BSDF_WARD, reflectance=(0.2, 0.45, 0.25), specular=(0.5, 0.5, 0.3), alpha=0.08, alpha_v=0.35, distr=WARD_BALANCED)       # mound (smooth normals)
    sc.textures = sc.textures[:1]                           # (the wall's and the mound's textures go with their BSDFs)
    sc.bsdfs[1] = make_bsdf(kind=BSDF_WARD, reflectance=(0.3, 0.3, 0.35), specular=(0.6, 0.55, 0.5), alpha=0.4, alpha_v=0.1, distr=WARD_DUER, twosided=True)   # wall (sheared uv: non-orthogonal tangents)
    return sc


def cbox_coating(width=96, height=96, spp=16, sampler=SAMPLER_SOBOL, max_depth=8, rr_depth=5, seed=0, strict_normals=False):
    """Cornell box with `coating` layers: clear varnish over diffuse, an absorbing layer over diffuse (twosided), a layer over a rough conductor, one over a smooth
    conductor (a delta component under the layer) and one over a rough plastic."""
    sc = cornell_box(width, height, spp, sampler, max_depth, rr_depth, seed=seed, strict_normals=strict_normals)
    sc.name = "cbox_coating"
    eta, k = CONDUCTOR_IOR["Cu"]
    base = len(sc.bsdfs)
    sc.bsdfs.extend([make_bsdf(reflectance=(0.6, 0.55, 0.45)),                                                                  # base + 0: nested diffuse
                     make_bsdf(kind=BSDF_COATING, nested=base, ior=1.5046, reflectance=(0.0, 0.0, 0.0)),                       # base + 1: floor
                     make_bsdf(reflectance=(0.7, 0.7, 0.7)),                                                                    # base + 2
                     make_bsdf(kind=BSDF_COATING, nested=base + 2, ior=1.33, reflectance=(0.2, 0.8, 1.6), scale=0.7, specular=(0.9, 0.9, 0.9), twosided=True),   # base + 3: back wall
                     make_bsdf(kind=BSDF_ROUGHCONDUCTOR, alpha=0.15, distr=DISTR_GGX, eta=eta, k=k),                            # base + 4
                     make_bsdf(kind=BSDF_COATING, nested=base + 4, ior=1.7, reflectance=(0.1, 0.3, 0.05), scale=1.0),           # base + 5: short block
                     make_bsdf(kind=BSDF_CONDUCTOR, eta=eta, k=k),                                                              # base + 6
                     make_bsdf(kind=BSDF_COATING, nested=base + 6, ior=1.5, reflectance=(0.0, 0.0, 0.0)),                       # base + 7: tall block
                     ])
    sc.shapes[0]["bsdf"] = base + 1; sc.shapes[2]["bsdf"] = base + 3; sc.shapes[6]["bsdf"] = base + 5; sc.shapes[7]["bsdf"] = base + 7
    return sc


def blend_room(width=96, height=64, spp=16, sampler=SAMPLER_SOBOL, max_depth=6, rr_depth=4, seed=0):
    """The textured room with `blendbsdf`: the floor blends a rough conductor into a diffuse record through its checkerboard (a TEXTURED weight), the mound blends
    plastic and diffuse with a constant weight, the wall (twosided) blends two diffuse records through a grid texture."""
    sc = textured_room(width, height, spp, sampler, max_depth, rr_depth, seed=seed)
    sc.name = "blend_room"
    eta, k = CONDUCTOR_IOR["Au"]
    base = len(sc.bsdfs)
    sc.bsdfs.extend([make_bsdf(reflectance=(0.7, 0.65, 0.5)), make_bsdf(kind=BSDF_ROUGHCONDUCTOR, alpha=0.2, distr=DISTR_BECKMANN, eta=eta, k=k),       # base, base + 1
                     make_bsdf(kind=BSDF_PLASTIC, reflectance=(0.2, 0.5, 0.25), ior=1.49), make_bsdf(reflectance=(0.8, 0.2, 0.2)),                      # base + 2, base + 3
                     make_bsdf(reflectance=(0.1, 0.15, 0.6)), make_bsdf(reflectance=(0.9, 0.85, 0.3))])                                                # base + 4, base + 5
    sc.bsdfs.extend([make_bsdf(kind=BSDF_BLEND, nested=(base, base + 1), texture=0),                               # base + 6, floor: weight = the checkerboard
                     make_bsdf(kind=BSDF_BLEND, nested=(base + 4, base + 5), texture=1, twosided=True),             # base + 7, wall: weight = the grid texture
                     make_bsdf(kind=BSDF_BLEND, nested=(base + 2, base + 3), alpha=0.35)])                          # base + 8, mound: constant weight
    for i in range(3):                                     # (the children precede the blends; the room's own records 0..2 stay in the table as plain, unused ones)
        for sh in sc.shapes:
            if sh["bsdf"] == i: sh["bsdf"] = base + 6 + i
        sc.bsdfs[i] = make_bsdf(reflectance=(0.5, 0.5, 0.5))
    sc.textures = sc.textures[:2]
    return sc


def cbox_roughcoating(width=96, height=96, spp=16, sampler=SAMPLER_SOBOL, max_depth=8, rr_depth=5, seed=0, strict_normals=False):
    """Cornell box with `roughcoating` layers (Beckmann / GGX / Phong interfaces, with and without absorption, one `twosided`) over diffuse and rough-conductor records."""
    sc = cornell_box(width, height, spp, sampler, max_depth, rr_depth, seed=seed, strict_normals=strict_normals)
    sc.name = "cbox_roughcoating"
    eta, k = CONDUCTOR_IOR["Cu"]
    base = len(sc.bsdfs)
    sc.bsdfs.extend([make_bsdf(reflectance=(0.6, 0.55, 0.45)),                                                                                                  # base + 0
                     make_bsdf(kind=BSDF_ROUGHCOATING, nested=base, ior=1.5046, alpha=0.1, distr=DISTR_BECKMANN, reflectance=(0.0, 0.0, 0.0)),                 # base + 1: floor
                     make_bsdf(reflectance=(0.7, 0.7, 0.7)),                                                                                                    # base + 2
                     make_bsdf(kind=BSDF_ROUGHCOATING, nested=base + 2, ior=1.49, alpha=0.3, distr=DISTR_GGX, reflectance=(0.2, 0.8, 1.6), scale=0.7, specular=(0.9, 0.9, 0.9), twosided=True),   # base + 3: back wall
                     make_bsdf(kind=BSDF_ROUGHCONDUCTOR, alpha=0.15, distr=DISTR_GGX, eta=eta, k=k),                                                            # base + 4
                     make_bsdf(kind=BSDF_ROUGHCOATING, nested=base + 4, ior=1.9, alpha=0.05, distr=DISTR_BECKMANN, reflectance=(0.1, 0.3, 0.05), scale=1.0, sample_visible=False),   # base + 5: short block
                     make_bsdf(reflectance=(0.2, 0.3, 0.65)),                                                                                                   # base + 6
                     make_bsdf(kind=BSDF_ROUGHCOATING, nested=base + 6, ior=1.49, alpha=0.1, distr=DISTR_PHONG)])                                               # base + 7: tall block
    sc.shapes[0]["bsdf"] = base + 1; sc.shapes[2]["bsdf"] = base + 3; sc.shapes[6]["bsdf"] = base + 5; sc.shapes[7]["bsdf"] = base + 7
    tabs = []
    for bd in sc.bsdfs:
        if bd.get("table") is not None:
            off = sum(len(t) for t in tabs); tabs.append(bd["table"]); bd["k"] = (bd["k"][0], float(off), float(len(bd["table"])))
    sc.material_tables = np.concatenate(tabs).astype(f32)
    return sc


def open_constant(width=96, height=64, spp=16, sampler=SAMPLER_SOBOL, max_depth=6, rr_depth=4, seed=0, hide_emitters=False):
    """Open scene under a `constant` environment emitter and a `directional` light: floor + blocks (mesh), a rough-conductor sphere and a
    twosided sheet (reference normal 0 -> uniform-sphere sampling of the constant emitter)."""
    b = _Builder()
    grey = b.bsdf(reflectance=(0.55, 0.5, 0.45)); red = b.bsdf(reflectance=(0.6, 0.15, 0.1))
    sheet = b.bsdf(reflectance=(0.2, 0.5, 0.3), twosided=True)
    eta, k = CONDUCTOR_IOR["Au"]; gold = b.bsdf(kind=BSDF_ROUGHCONDUCTOR, alpha=0.2, distr=DISTR_BECKMANN, eta=eta, k=k)
    b.begin(); b.quad([(6, 0, -6), (-6, 0, -6), (-6, 0, 6), (6, 0, 6)]); b.end(grey)
    b.begin()
    for (x0, z0, x1, z1, h) in [(-2.0, 0.5, -0.8, 1.7, 1.2)]:
        b.quad([(x0, h, z0), (x0, h, z1), (x1, h, z1), (x1, h, z0)])
        b.quad([(x0, 0, z0), (x0, h, z0), (x1, h, z0), (x1, 0, z0)]); b.quad([(x1, 0, z0), (x1, h, z0), (x1, h, z1), (x1, 0, z1)])
        b.quad([(x1, 0, z1), (x1, h, z1), (x0, h, z1), (x0, 0, z1)]); b.quad([(x0, 0, z1), (x0, h, z1), (x0, h, z0), (x0, 0, z0)])
    b.end(red)
    b.begin(); b.quad([(0.3, 0.0, 2.4), (2.2, 0.0, 1.6), (2.2, 1.6, 1.6), (0.3, 1.6, 2.4)]); b.end(sheet)
    b.add_analytic(SHAPE_SPHERE, translate(0.9, 0.6, 0.2), gold, radius=0.6)
    cam = look_at((0.5, 2.2, -5.0), (0.0, 0.6, 0.8), (0, 1, 0))
    sc = finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 50.0, 0.05, 100.0, width, height, spp, sampler, max_depth, rr_depth,
                      seed=seed, hide_emitters=hide_emitters, name="open_constant", analytic=b.resolve_analytic())
    return add_scene_emitters(sc, [constant_emitter((0.55, 0.7, 0.95)), directional_emitter((-0.4, -1.0, 0.35), (3.0, 2.6, 2.0))])


def glass_pane(width=96, height=64, spp=16, sampler=SAMPLER_SOBOL, max_depth=6, rr_depth=4, seed=0, hide_emitters=False):
    """The open scene of `open_constant` seen partly through a `thindielectric` pane (delta reflection + straight-through ENull transmission with the
    internal bounces summed), a second tinted pane deeper in the scene, and a small area light behind the first pane.  A path that has only crossed panes
    counts as unscattered: with hideEmitters the sky stays hidden through the glass (path.cpp:213, 238-239) while the area light does not (:226-231)."""
    b = _Builder()
    grey = b.bsdf(reflectance=(0.55, 0.5, 0.45)); red = b.bsdf(reflectance=(0.6, 0.15, 0.1)); lightm = b.bsdf(reflectance=(0.3, 0.3, 0.3))
    pane = b.bsdf(kind=BSDF_THINDIELECTRIC, ior=1.5046, specular=(1.0, 1.0, 1.0), reflectance=(0.92, 0.97, 1.0))
    tinted = b.bsdf(kind=BSDF_THINDIELECTRIC, ior=1.33, specular=(0.9, 0.8, 0.7), reflectance=(0.5, 0.8, 0.6))
    eta, k = CONDUCTOR_IOR["Au"]; gold = b.bsdf(kind=BSDF_ROUGHCONDUCTOR, alpha=0.2, distr=DISTR_BECKMANN, eta=eta, k=k)
    b.begin(); b.quad([(6, 0, -6), (-6, 0, -6), (-6, 0, 6), (6, 0, 6)]); b.end(grey)
    b.begin()
    x0, z0, x1, z1, h = -2.0, 0.5, -0.8, 1.7, 1.2
    b.quad([(x0, h, z0), (x0, h, z1), (x1, h, z1), (x1, h, z0)])
    b.quad([(x0, 0, z0), (x0, h, z0), (x1, h, z0), (x1, 0, z0)]); b.quad([(x1, 0, z0), (x1, h, z0), (x1, h, z1), (x1, 0, z1)])
    b.quad([(x1, 0, z1), (x1, h, z1), (x0, h, z1), (x0, 0, z1)]); b.quad([(x0, 0, z1), (x0, h, z1), (x0, h, z0), (x0, 0, z0)])
    b.end(red)
    b.begin(); b.quad([(-3.0, 0.0, -2.5), (0.6, 0.0, -2.9), (0.6, 3.2, -2.9), (-3.0, 3.2, -2.5)]); b.end(pane)            # in front of the camera, left part of the view
    b.begin(); b.quad([(0.2, 0.0, 2.6), (2.4, 0.0, 1.8), (2.4, 1.8, 1.8), (0.2, 1.8, 2.6)]); b.end(tinted)
    b.begin(); b.quad([(-1.6, 2.2, 0.4), (-1.6, 2.2, 1.0), (-1.0, 2.2, 1.0), (-1.0, 2.2, 0.4)]); b.end(lightm, radiance=(9.0, 8.0, 6.0))   # faces down, seen through the pane
    b.add_analytic(SHAPE_SPHERE, translate(0.9, 0.6, 0.2), gold, radius=0.6)
    cam = look_at((0.5, 2.2, -5.0), (0.0, 0.9, 0.8), (0, 1, 0))
    sc = finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 50.0, 0.05, 100.0, width, height, spp, sampler, max_depth, rr_depth,
                      seed=seed, hide_emitters=hide_emitters, name="glass_pane", analytic=b.resolve_analytic())
    return add_scene_emitters(sc, [constant_emitter((0.55, 0.7, 0.95)), directional_emitter((-0.4, -1.0, 0.35), (3.0, 2.6, 2.0))])


def masked_room(width=96, height=64, spp=16, sampler=SAMPLER_SOBOL, max_depth=6, rr_depth=4, seed=0, hide_emitters=False, fog=None):
    """`mask` BSDFs (src/bsdfs/mask.cpp) in the open scene: a cut-out screen in front of the camera (checkerboard opacity 1 / 0 over a twosided diffuse), a
    tinted half-transparent sheet over `plastic` (coloured opacity: the pass-through lobe carries 1 - opacity), and a grid-masked rough conductor panel.
    Passing through is an ENull event: with hideEmitters the sky stays hidden through the holes.
    fog = INTEGRATOR_VOLPATH_SIMPLE / INTEGRATOR_VOLPATH: the sensor sits in a thin medium that fills the scene; the masks' ENull lobes then attenuate the transmittance
    walks of emitter sampling and the emitter search (1 - opacity at the hit's uv); the sheet -- a mesh WITHOUT texture coordinates -- gets the grid texture too: the
    walks look it up at uv = (0, 0) (skdtree.cpp:182-184) while shading uses the barycentrics."""
    b = _Builder(); uvs = []
    def quad_uv(pts, uv=((0, 0), (1, 0), (1, 1), (0, 1))):
        b.quad(pts); uvs.extend(uv)
    grey = b.bsdf(reflectance=(0.55, 0.5, 0.45)); red = b.bsdf(reflectance=(0.6, 0.15, 0.1)); lightm = b.bsdf(reflectance=(0.3, 0.3, 0.3))
    green2 = b.bsdf(reflectance=(0.2, 0.6, 0.25), twosided=True)
    plast = b.bsdf(kind=BSDF_PLASTIC, reflectance=(0.7, 0.4, 0.2), ior=1.49, twosided=True)
    eta, k = CONDUCTOR_IOR["Au"]; gold = b.bsdf(kind=BSDF_ROUGHCONDUCTOR, alpha=0.15, distr=DISTR_GGX, eta=eta, k=k, twosided=True)
    screen = b.bsdf(kind=BSDF_MASK, nested=green2); b.bsdfs[screen]["texture"] = 0
    sheet = b.bsdf(kind=BSDF_MASK, nested=plast, reflectance=(0.3, 0.5, 0.7))
    grille = b.bsdf(kind=BSDF_MASK, nested=gold); b.bsdfs[grille]["texture"] = 1
    tex = [make_texture(TEXTURE_CHECKERBOARD, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), uscale=7.0, vscale=5.0, uoffset=0.1),
           make_texture(TEXTURE_GRID, (0.0, 0.0, 0.0), (1.0, 0.9, 0.8), line_width=0.12, uscale=6.0, vscale=6.0)]
    b.begin(); quad_uv([(6, 0, -6), (-6, 0, -6), (-6, 0, 6), (6, 0, 6)]); b.end(grey)
    b.begin()
    x0, z0, x1, z1, h = -2.0, 0.5, -0.8, 1.7, 1.2
    quad_uv([(x0, h, z0), (x0, h, z1), (x1, h, z1), (x1, h, z0)])
    quad_uv([(x0, 0, z0), (x0, h, z0), (x1, h, z0), (x1, 0, z0)]); quad_uv([(x1, 0, z0), (x1, h, z0), (x1, h, z1), (x1, 0, z1)])
    quad_uv([(x1, 0, z1), (x1, h, z1), (x0, h, z1), (x0, 0, z1)]); quad_uv([(x0, 0, z1), (x0, h, z1), (x0, h, z0), (x0, 0, z0)])
    b.end(red)
    b.begin(); quad_uv([(-3.0, 0.0, -2.5), (0.4, 0.0, -2.9), (0.4, 3.0, -2.9), (-3.0, 3.0, -2.5)]); b.end(screen)         # in front of the camera, left part of the view
    b.begin(); quad_uv([(0.2, 0.0, 2.6), (2.4, 0.0, 1.8), (2.4, 1.8, 1.8), (0.2, 1.8, 2.6)]); b.end(sheet)
    b.begin(); quad_uv([(0.8, 0.0, -1.6), (2.6, 0.0, -1.2), (2.6, 1.5, -1.2), (0.8, 1.5, -1.6)]); b.end(grille)
    b.begin(); quad_uv([(-1.6, 2.2, 0.4), (-1.6, 2.2, 1.0), (-1.0, 2.2, 1.0), (-1.0, 2.2, 0.4)]); b.end(lightm, radiance=(9.0, 8.0, 6.0))
    for sh in b.shapes: sh["has_uv"] = 0
    for si in (2, 4): b.shapes[si]["has_uv"] = 1
    cam = look_at((0.5, 2.2, -5.0), (0.0, 0.9, 0.8), (0, 1, 0))
    extra = {}
    if fog:
        b.bsdfs[sheet]["texture"] = 1
        extra = dict(media=[make_medium((0.004, 0.004, 0.006), (0.04, 0.04, 0.035))], sensor_medium=0, integrator=fog)
    sc = finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 50.0, 0.05, 100.0, width, height, spp, sampler, max_depth, rr_depth,
                      seed=seed, hide_emitters=hide_emitters, uvs=uvs, name="masked_room", textures=tex, **extra)
    return add_scene_emitters(sc, [constant_emitter((0.55, 0.7, 0.95)), directional_emitter((-0.4, -1.0, 0.35), (3.0, 2.6, 2.0))])


def detailed_sky(w=256, h=128):
    """Lat-long environment with texel-scale detail (tiles, thin bands, a small sun): seen by the camera on a small film it is minified, so the
    filtered lookup of EnvironmentMap::evalEnvironment (EWA over the MIP pyramid) differs visibly from a level-0 lookup."""
    y, x = np.mgrid[0:h, 0:w]
    tiles = ((x // 3 + y // 2) % 2).astype(np.float64)
    bands = ((y % 7) < 2).astype(np.float64)
    rgb = np.stack([0.15 + 0.8 * tiles, 0.25 + 0.5 * bands, 0.9 - 0.6 * tiles * bands], -1)
    rgb[y > h * 0.55] *= 0.25                                # darker below the horizon
    sun = np.exp(-(((x - w * 0.62) / 2.5) ** 2 + ((y - h * 0.3) / 2.0) ** 2))
    rgb = rgb + (40.0 * sun)[..., None] * np.array([1.0, 0.9, 0.7])
    return rgb.astype(np.float16).astype(f32)


def sky_view(width=64, height=48, spp=16, sampler=SAMPLER_SOBOL, max_depth=5, rr_depth=4, seed=0, env_size=(256, 128), hide_emitters=False):
    """Camera looking at the horizon under a detailed environment map: most camera rays leave the scene directly, each pixel covers several texels
    (EWA-filtered environment lookups with the sensor ray's differentials, envmap.cpp:398-411); a floor and a block keep the bounce loop busy."""
    b = _Builder()
    grey = b.bsdf(reflectance=(0.5, 0.5, 0.5)); red = b.bsdf(reflectance=(0.65, 0.2, 0.15))
    b.begin(); b.quad([(8, 0, -8), (-8, 0, -8), (-8, 0, 8), (8, 0, 8)]); b.end(grey)
    b.begin()
    x0, z0, x1, z1, hh = -1.2, 0.8, 0.2, 2.0, 1.4
    b.quad([(x0, hh, z0), (x0, hh, z1), (x1, hh, z1), (x1, hh, z0)])
    b.quad([(x0, 0, z0), (x0, hh, z0), (x1, hh, z0), (x1, 0, z0)]); b.quad([(x1, 0, z0), (x1, hh, z0), (x1, hh, z1), (x1, 0, z1)])
    b.quad([(x1, 0, z1), (x1, hh, z1), (x0, hh, z1), (x0, 0, z1)]); b.quad([(x0, 0, z1), (x0, hh, z1), (x0, hh, z0), (x0, 0, z0)])
    b.end(red)
    cam = look_at((0.8, 1.1, -4.5), (-0.2, 1.9, 1.0), (0.05, 1, 0))
    env = dict(rgb=detailed_sky(*env_size), to_world=(rotate((0, 1, 0), 25.0) @ rotate((1, 0, 0), 8.0)).astype(f32), scale=0.8)
    sc = finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 55.0, 0.05, 100.0, width, height, spp, sampler, max_depth, rr_depth,
                      seed=seed, hide_emitters=hide_emitters, envmap=env, name="sky_view")
    sc.emitters.insert(0, dict(type=EMITTER_ENVMAP, shape=-1, radiance=(0.0, 0.0, 0.0), weight=1.0))
    return sc


VEACH_MICROFACETS = [   # the plates of veach_mis with the rest of MicrofacetDistribution: anisotropy, all-normal sampling, Phong / Ashikhmin-Shirley
    dict(alpha=0.02, alpha_v=0.1, distr=DISTR_BECKMANN, sample_visible=True),
    dict(alpha=0.15, alpha_v=0.03, distr=DISTR_GGX, sample_visible=False),
    dict(alpha=0.05, distr=DISTR_PHONG),
    dict(alpha=0.04, alpha_v=0.2, distr=DISTR_PHONG),
]
VEACH_MICROFACETS_2 = [
    dict(alpha=0.03, distr=DISTR_BECKMANN, sample_visible=False),
    dict(alpha=0.05, alpha_v=0.25, distr=DISTR_BECKMANN, sample_visible=False),
    dict(alpha=0.2, alpha_v=0.04, distr=DISTR_GGX, sample_visible=True),
    dict(alpha=0.1, distr=DISTR_GGX, sample_visible=False),
]


# ---------------------------------------------------------------------------------------------
# binary container for the oracle-side harness
# ---------------------------------------------------------------------------------------------
def save_scene(sc, path):
    if float(sc.get("aperture_radius", 0.0) or 0.0) != 0.0:
        raise ValueError("save_scene: the MISCENE2 container has no field for a thin lens (aperture_radius / focus_distance); only perspective-camera scenes can be written")
    with open(path, "wb") as f:
        f.write(b"MISCENE2")
        has_n = int(sc.nrm is not None); has_uv = int(sc.uv is not None)
        has_env = int(sc.envmap is not None)
        f.write(struct.pack("<8I", len(sc.pos), len(sc.idx), len(sc.shapes), len(sc.bsdfs),
                            len(sc.emitters), has_n, has_uv, has_env))
        f.write(sc.pos.tobytes())
        if has_n: f.write(sc.nrm.tobytes())
        if has_uv: f.write(sc.uv.tobytes())
        f.write(sc.idx.tobytes())
        for s in sc.shapes:
            f.write(struct.pack("<4I2i2I", s["first_tri"], s["tri_count"], s["first_vert"], s["vert_count"],
                                s["bsdf"], s["emitter"], (s["face_normals"] & 1) | ((s.get("has_uv", 0) & 1) << 1), s.get("group", 0)))
        for b in sc.bsdfs:
            f.write(struct.pack("<4I", b["type"], b["twosided"], b["distr"], b["sample_visible"] | (b.get("aniso", 0) << 2)))
            f.write(struct.pack("<13f", *b["reflectance"], b["alpha"], *b["eta"], *b["k"], *b["specular"]))
        for e in sc.emitters:
            f.write(struct.pack("<Ii4f", e["type"], e["shape"], *e["radiance"], e["weight"]))
            f.write(struct.pack("<2f", e.get("cutoff", 20.0), e.get("beam", 15.0)))
            f.write(np.ascontiguousarray(e.get("to_world", np.eye(4)), dtype=f32).tobytes())
        f.write(sc.cam_to_world.tobytes())
        f.write(struct.pack("<3f2I", sc.xfov, sc.near, sc.far, sc.width, sc.height))
        f.write(struct.pack("<I2f", sc.filter, sc.filter_radius, sc.filter_stddev))
        f.write(struct.pack("<2i2I", sc.max_depth, sc.rr_depth, sc.strict_normals, sc.hide_emitters))
        f.write(struct.pack("<2IQ", sc.sampler, sc.spp, sc.seed))
        if has_env:
            rgb = np.ascontiguousarray(sc.envmap["rgb"], dtype=f32)
            f.write(struct.pack("<2I", rgb.shape[1], rgb.shape[0]))
            f.write(np.ascontiguousarray(sc.envmap["to_world"], dtype=f32).tobytes())
            f.write(struct.pack("<f", sc.envmap["scale"]))
            f.write(rgb.tobytes())
        if sc.get("analytic"):
            f.write(b"ANLY"); f.write(struct.pack("<I", len(sc.analytic)))
            for a in sc.analytic:
                f.write(struct.pack("<I2iI", a["type"], a["bsdf"], a["emitter"], a["flags"]))
                f.write(a["to_world"].tobytes()); f.write(a["to_object"].tobytes())
                f.write(struct.pack("<2f", a["radius"], a["length"]))
        mat_textures = [t for i, t in enumerate(sc.get("textures") or []) if i + 1 != sc.get("env_texture", 0)]     # the environment map's pyramid record is ours; the reference builds its own
        if mat_textures:
            f.write(b"TEXR"); f.write(struct.pack("<I", len(mat_textures)))
            for t in mat_textures:
                f.write(struct.pack("<I11f", t["type"], *t["color0"], *t["color1"], t["line_width"], t["uoffset"], t["voffset"], t["uscale"], t["vscale"]))
                f.write(struct.pack("<3If2I", t["wrap_u"], t["wrap_v"], t["filter"], t["max_anisotropy"], 0, 0))
                if t["type"] == TEXTURE_BITMAP:              # the harness builds the reference's own BitmapTexture (and MIP pyramid) from the base image
                    base = t["pyramid"]["base"]; f.write(struct.pack("<2I", base.shape[1], base.shape[0])); f.write(base.tobytes())
            f.write(struct.pack("<%di" % len(sc.bsdfs), *[b.get("texture", -1) for b in sc.bsdfs]))
        if sc.get("crop"):
            f.write(b"CROP"); f.write(struct.pack("<I", 1)); f.write(struct.pack("<4i", *sc.crop))
        if sc.get("media"):
            f.write(b"MEDI"); f.write(struct.pack("<I", len(sc.media)))
            for m in sc.media:
                f.write(struct.pack("<6fI2fIfI", *m["sigma_a"], *m["sigma_s"], m["strategy"], m["sampling_density"], m["medium_sampling_weight"], m["phase"], m["g"], 0))
            f.write(struct.pack("<2iI", sc.integrator, sc.sensor_medium, len(sc.shape_media))); f.write(np.ascontiguousarray(sc.shape_media, np.int32).tobytes())
        if sc.get("instances"):
            f.write(b"INST"); f.write(struct.pack("<I", len(sc.instances)))
            for a in sc.instances:
                f.write(struct.pack("<4I", a["group"], 0, 0, 0)); f.write(a["to_world"].tobytes()); f.write(a["to_object"].tobytes())


# ---------------------------------------------------------------------------------------------
# MIP pyramid construction: TMIPMap's constructor (include/mitsuba/render/mipmap.h:176-271) over Bitmap::resample
# (src/libcore/bitmap.cpp:2231-2330) and Resampler (include/mitsuba/core/rfilter.h:123-198, :232-330, :437-457) with the 2-lobed
# Lanczos filter (src/rfilters/lanczos.cpp).  Host-side data preparation: the pyramid is INPUT of the path.
# ---------------------------------------------------------------------------------------------
def _lanczos2(x):
    x = np.abs(x.astype(f32))
    x1 = (f32(math.pi) * x).astype(f32); x2 = (x1 / f32(2.0)).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = ((np.sin(x1) * np.sin(x2)) / (x1 * x2)).astype(f32)
    return np.where(x < f32(1e-4), f32(1.0), np.where(x > f32(2.0), f32(0.0), v)).astype(f32)


def _resample_axis(src, target, bc, lo, hi):
    """Resampler::resampleAndClamp along axis 0 of src[n, ...]: every output sample is sum_j source[start + j] * weight[j] accumulated in tap order."""
    n = src.shape[0]
    scale = f32(n) / f32(target); inv = f32(1.0) / scale; radius = f32(2.0) * scale
    taps = int(math.ceil(float(radius) * 2.0))
    i = np.arange(target)
    center = ((i.astype(f32) + f32(0.5)) / f32(target) * f32(n)).astype(f32)
    start = np.floor(center - radius + f32(0.5)).astype(np.int64)
    pos = (start[:, None] + np.arange(taps)[None, :]).astype(f32) + f32(0.5) - center[:, None]
    w = _lanczos2((pos * inv).astype(f32))
    total = np.zeros(target, f32)
    for j in range(taps):
        total = (total + w[:, j]).astype(f32)
    w = (w * (f32(1.0) / total)[:, None]).astype(f32)
    out = np.zeros((target,) + src.shape[1:], f32)
    for j in range(taps):
        p = start + j
        outside = (p < 0) | (p >= n)
        if bc == WRAP_CLAMP:
            q = np.clip(p, 0, n - 1)
        elif bc == WRAP_REPEAT:
            q = np.mod(p, n)
        elif bc == WRAP_MIRROR:
            q = np.mod(p, 2 * n); q = np.where(q >= n, 2 * n - q - 1, q)
        else:
            q = np.clip(p, 0, n - 1)
        v = src[q]
        if bc in (WRAP_ZERO, WRAP_ONE):
            v = np.where(outside.reshape((-1,) + (1,) * (src.ndim - 1)), f32(0.0 if bc == WRAP_ZERO else 1.0), v)
        out = (out + v * w[:, j].reshape((-1,) + (1,) * (src.ndim - 1))).astype(f32)
    return np.minimum(f32(hi), np.maximum(f32(lo), out)).astype(f32)


def build_mip_pyramid(rgb, wrap_u=WRAP_REPEAT, wrap_v=WRAP_REPEAT, max_value=1.0):
    """levels [(w, h, texels[h*w*3])] of `rgb[h, w, 3]` as TMIPMap<Color3, Color3h> holds them: each level is resampled from the previous one in
    float (x first, then y; results clamped to [0, max_value]) and stored rounded to half.  Bitmap textures use max_value = 1, the environment
    map infinity (src/emitters/envmap.cpp:182-185)."""
    cur = np.maximum(np.asarray(rgb, f32), f32(0.0))          # negative texels are clamped (mipmap.h:236-243)
    levels = [(cur.shape[1], cur.shape[0], np.ascontiguousarray(cur.astype(np.float16).astype(f32).reshape(-1)))]
    h, w = cur.shape[:2]
    while w > 1 or h > 1:
        nw, nh = max(1, (w + 1) // 2), max(1, (h + 1) // 2)
        if nw != w:
            cur = np.ascontiguousarray(np.swapaxes(_resample_axis(np.ascontiguousarray(np.swapaxes(cur, 0, 1)), nw, wrap_u, 0.0, max_value), 0, 1))
        if nh != h:
            cur = _resample_axis(cur, nh, wrap_v, 0.0, max_value)
        w, h = nw, nh
        levels.append((w, h, np.ascontiguousarray(cur.astype(np.float16).astype(f32).reshape(-1))))
    return levels
