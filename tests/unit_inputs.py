"""Inputs of the unit-level comparisons of the BSDF and texture routines (tests/test_unit_inputs.py on the CPU, tests/test_gpu_units.py on the device): one generator,
fixed seeds, so that both sides and both tests see the same numbers.  Directions and sample values are aimed at what camera-driven paths almost never produce:
grazing and exactly normal incidence, sample values 0 and 1 - 2^-24, directions below a one-sided surface, texture coordinates on texel edges and wrap seams,
degenerate and non-finite footprints."""
import zlib
import numpy as np

f32 = np.float32
BSDF_SCENES = ["cbox_materials", "veach_small", "veach_microfacets", "veach_microfacets_2", "cbox_translucent", "cbox_translucent_mf", "cbox_translucent_mf2", "cbox_roughplastic",
               "cbox_roughplastic_allnormals", "cbox_roughplastic_phong", "cbox_phong", "cbox_ward", "ward_room", "cbox_roughdiffuse", "cbox_coating", "cbox_roughcoating", "blend_room",
               "glass_pane", "layered_room", "masked_room"]
N_BSDF = 4096
ONE_MINUS = float(f32(1.0) - f32(2.0 ** -24))
EDGE_Z = [1e-7, 1e-4, 1e-2, 1.0, 0.0]
EDGE_AZIMUTH = [(1.0, 0.0), (np.sqrt(0.5), np.sqrt(0.5)), (0.0, 1.0), (-1.0, 0.0)]      # 0, pi / 4, pi / 2, pi
TYPE_NAMES = {0: "diffuse", 1: "roughconductor", 2: "conductor", 3: "dielectric", 4: "plastic", 5: "roughdielectric", 6: "difftrans", 7: "roughplastic", 8: "thindielectric", 9: "mask",
              10: "mixturebsdf", 11: "bumpmap", 12: "normalmap", 13: "null", 14: "roughdiffuse", 15: "phong", 16: "ward", 17: "coating", 18: "blendbsdf", 19: "roughcoating"}
# the device code of these calls no math-library routine (pt_device.h: arithmetic, sqrtf and the restated sincosf of the warps only)
NO_LIBM_TYPES = {0, 2, 3, 4, 6, 8, 13}
ZERO_EVAL_TYPES = {2, 3, 8, 13}            # eval() is identically zero: nothing but Dirac deltas


def children(sc, m):
    """records a wrapper record refers to"""
    b = sc.bsdfs[m]
    if b["type"] in (9, 11, 12, 17, 19): return [int(b["distr"])]
    if b["type"] == 10: return [int(c) for c in (list(b["reflectance"]) + [b["eta"][0]])[:b["distr"]]]
    if b["type"] == 18: return [int(b["eta"][0]), int(b["eta"][1])]
    return []


def refused(sc, m):
    """what mi_debug_bsdf refuses: mask, bumpmap, normalmap, a bound texture -- the record itself or one below it"""
    b = sc.bsdfs[m]
    return b["type"] in (9, 11, 12) or b.get("texture", -1) >= 0 or any(refused(sc, c) for c in children(sc, m))


def leaf_types(sc, m):
    b = sc.bsdfs[m]; ch = children(sc, m)
    return {b["type"]} | set().union(*[leaf_types(sc, c) for c in ch]) if ch else {b["type"]}


def records(sc):
    return [m for m in range(len(sc.bsdfs)) if not refused(sc, m)]


def no_libm(sc, m):
    """plain records of NO_LIBM_TYPES and mixtures / blends of them (a coating's absorption calls exp)"""
    return leaf_types(sc, m) <= (NO_LIBM_TYPES | {10, 18})


def zero_eval(sc, m):
    b = sc.bsdfs[m]
    return b["type"] in ZERO_EVAL_TYPES or (b["type"] == 17 and zero_eval(sc, int(b["distr"])))


def black(sc, m):
    """a diffuse record without reflectance (the BSDF of a light source's mesh): weight and value are zero for every input"""
    b = sc.bsdfs[m]
    return b["type"] == 0 and not any(b["reflectance"])


def _directions(rng, n, upper_share):
    """unit vectors: `upper_share` of them with z > 0; a quarter of all cases with |z| out of EDGE_Z, a third of those at an azimuth out of EDGE_AZIMUTH"""
    z = rng.uniform(0.0, 1.0, n); phi = rng.uniform(0.0, 2 * np.pi, n); c, s = np.cos(phi), np.sin(phi)
    edge = rng.uniform(size=n) < 0.25; z = np.where(edge, np.asarray(EDGE_Z)[rng.integers(0, len(EDGE_Z), n)], z)
    az = edge & (rng.uniform(size=n) < 1.0 / 3); k = rng.integers(0, len(EDGE_AZIMUTH), n); ea = np.asarray(EDGE_AZIMUTH)
    c = np.where(az, ea[k, 0], c); s = np.where(az, ea[k, 1], s)
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z)); sign = np.where(rng.uniform(size=n) < upper_share, 1.0, -1.0)
    return np.ascontiguousarray(np.stack([r * c, r * s, z * sign], 1), f32)


def bsdf_inputs(scene_name, material):
    """wi [n, 3], uv [n, 2], extra [n], wo [n, 3] (the eval directions before the oracle's own samples are mixed in: eval_wo)"""
    rng = np.random.default_rng([zlib.crc32(scene_name.encode()), material, 2718]); n = N_BSDF
    wi = _directions(rng, n, 0.75)
    uv = rng.uniform(size=(n, 2)).astype(f32); uv = np.minimum(uv, f32(ONE_MINUS))
    special = [(0.0, 0.0), (ONE_MINUS, ONE_MINUS), (0.5, 0.5), (2.0 ** -32, 0.25)]
    for i in range(20): uv[i] = special[i // 5]
    extra = np.minimum(rng.uniform(size=n).astype(f32), f32(ONE_MINUS)); extra[20::16] = 0.0; extra[28::16] = ONE_MINUS
    wo = _directions(rng, n, 0.6)
    return dict(wi=wi, uv=uv, extra=extra, wo=wo)


def eval_wo(inp, sampled):
    """every fourth case takes the oracle's own sample for that (wi, u, v) if it is non-zero, so that narrow lobes are not all zeros; sampled = orc.bsdf_sample_units(...)"""
    wo = inp["wo"].copy(); take = np.zeros(len(wo), bool); take[::4] = True
    take &= (sampled[:, 0:3] != 0).any(1) & np.isfinite(sampled[:, 4:7]).all(1)
    wo[take] = sampled[take, 4:7]
    return wo


# ------------------------------------------------------------------------------------------------ textures
N_TEX = 3000
MAX_EWA_TEXELS = 16384
FILTER_NAMES = ["nearest", "bilinear", "trilinear", "ewa"]
WRAP_PAIRS = [(1, 2), (2, 0), (0, 3), (3, 4), (4, 1)]      # (wrap_u, wrap_v): every mode on each axis, never the same on both
ANISOTROPY = [20.0, 10.0, 4.0, 20.0, 1.0]
SCALES = [(3.0, 2.0, 0.1), (1.7, 1.3, 0.0), (1.0, 1.0, 0.0), (0.5, 0.75, -0.3), (2.5, 0.6, 0.5)]      # uscale, vscale, uoffset; the third is the identity (texel_centres)
CONSTANT_COLOR = (0.25, 0.5, 0.75)
N_BITMAPS = 20
TEX_CONSTANT = [20, 21, 22, 23]          # one constant-colour bitmap per filter
CONSTANT_WRAPS = [(2, 0), (1, 2), (0, 1), (2, 1)]      # no zero / one: those return their own colour outside [0, 1]
TEX_CHECKER, TEX_GRID = 24, 25
GRID_LINE_WIDTH = 0.05


def texture_scene(S):
    """bitmap_room's geometry at 32 x 32 under a texture table of its own: 20 bitmaps over the committed 48 x 40 pyramid (4 filters x 5 wrap pairs), a constant-colour
    bitmap under each filter, a checkerboard and a grid.  S = the package's `scenes` module."""
    sc = S.bitmap_room(32, 32, 1); pyr = dict(S.load_texture_pyramid(), wrapped=True)      # the committed levels under every wrap mode
    tex = []
    for f in range(4):
        for j, (wu, wv) in enumerate(WRAP_PAIRS):
            us, vs, uo = SCALES[j]
            tex.append(S.make_texture(S.TEXTURE_BITMAP, pyramid=pyr, uscale=us, vscale=vs, uoffset=uo, wrap_u=wu, wrap_v=wv, filter_type=f, max_anisotropy=ANISOTROPY[j]))
    const_levels = [(w, h, np.tile(np.asarray(CONSTANT_COLOR, f32), w * h)) for (w, h, _) in pyr["levels"]]
    w0, h0, t0 = const_levels[0]
    for f, (wu, wv) in enumerate(CONSTANT_WRAPS):
        tex.append(S.make_texture(S.TEXTURE_BITMAP, pyramid=dict(base=t0.reshape(h0, w0, 3), levels=const_levels, wrapped=True), uscale=1.3, vscale=0.9, uoffset=0.2, wrap_u=wu, wrap_v=wv, filter_type=f))
    tex.append(S.make_texture(S.TEXTURE_CHECKERBOARD, color0=(0.8, 0.7, 0.1), color1=(0.1, 0.2, 0.6), uscale=1.5, vscale=2.0, uoffset=0.25))
    tex.append(S.make_texture(S.TEXTURE_GRID, color0=(0.9, 0.9, 0.8), color1=(0.1, 0.1, 0.1), line_width=GRID_LINE_WIDTH))
    return S.finish_scene(sc.pos, sc.idx, sc.shapes, sc.bsdfs, sc.emitters, sc.cam_to_world, sc.xfov, sc.near, sc.far, 32, 32, 1, sc.sampler, sc.max_depth, sc.rr_depth,
                          normals=sc.nrm, uvs=sc.uv, name="texture_units", textures=tex)


def texture_inputs(sc, t):
    """uv [n, 2] and partials [n, 4] = (dudx, dvdx, dudy, dvdy) for texture record t of texture_scene"""
    rng = np.random.default_rng([t, 314159]); n = N_TEX; tx = sc.textures[t]
    if tx["type"] != 2:                                     # procedural: [-3, 3], multiples of 0.5 (checker flips, grid lines), points within an ulp of the grid's line width
        uv = rng.uniform(-3.0, 3.0, (n, 2)).astype(f32)
        uv[:200] = (rng.integers(-6, 7, (200, 2)) * 0.5).astype(f32)
        lw = f32(GRID_LINE_WIDTH); near = np.array([np.nextafter(lw, f32(0)), lw, np.nextafter(lw, f32(1))], f32)
        k = rng.integers(-3, 3, (200, 2)).astype(f32); sgn = np.where(rng.uniform(size=(200, 2)) < 0.5, f32(-1), f32(1))
        uv[200:400] = k + sgn * near[rng.integers(0, 3, (200, 2))]                   # (the grid record has scale 1, offset 0: these are its texture-space coordinates)
        return np.ascontiguousarray(uv), np.zeros((n, 4), f32)
    w0, h0 = 48, 40
    uv = rng.uniform(-1.5, 2.5, (n, 2))
    uv[60:160] = rng.integers(-1, 3, (100, 2))                                        # integer uv: the wrap seams
    ke = rng.integers(-w0, 2 * w0 + 1, 200); le = rng.integers(-h0, 2 * h0 + 1, 200)      # texture-space coordinates exactly on level-0 texel edges, mapped back through scale / offset
    uv[160:360, 0] = (ke / w0 - tx["uoffset"]) / tx["uscale"]; uv[160:360, 1] = (le / h0 - tx["voffset"]) / tx["vscale"]
    uv = uv.astype(f32)
    # footprints: an orthogonal pair, magnitude 10^U(-5, 1), axis ratio 10^U(0, 2.5), random angle
    mag = 10.0 ** rng.uniform(-5.0, 1.0, n); ratio = 10.0 ** rng.uniform(0.0, 2.5, n); ang = rng.uniform(0.0, 2 * np.pi, n)
    c, s = np.cos(ang), np.sin(ang)
    pa = np.stack([mag * c, mag * s, -(mag / ratio) * s, (mag / ratio) * c], 1)
    # the routes of k_env_primary at the poles: every sixth of the first 60
    unit = np.stack([c, s, -s / ratio, c / ratio], 1)[:60] * 2.0                   # magnitude 2: times 1e20 its squares overflow on every axis
    for i in range(60):
        k = i % 6
        if k == 0: pa[i] = 0.0
        elif k == 1: pa[i, 2:] = 0.0
        elif k == 2: pa[i, 2:] = pa[i, :2]
        elif k == 3: pa[i] = np.nan
        elif k == 4: pa[i, i // 6 % 4] = np.inf
        else: pa[i] = unit[i] * 1e20
    return np.ascontiguousarray(uv), np.ascontiguousarray(pa, f32)


def nearest_rule(x, y, wrap_u, wrap_v, texels):
    """the index rule of TMIPMap::evalTexel (mipmap.h:504-560) restated over arrays; texels [h, w, 3]"""
    h, w, _ = texels.shape
    def wrap(i, n, mode):
        out = (i < 0) | (i >= n)
        j = np.where(mode == 1, i % n, np.where(mode == 0, np.clip(i, 0, n - 1), np.where((i % (2 * n)) >= n, 2 * n - (i % (2 * n)) - 1, i % (2 * n))))
        return np.where(out, j, i), out & (mode >= 3)
    xi, cx = wrap(x, w, wrap_u); yi, cy = wrap(y, h, wrap_v)
    r = texels[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)].copy()
    r[cy] = 0.0 if wrap_v == 3 else 1.0; r[cx] = 0.0 if wrap_u == 3 else 1.0       # the u axis is tested first
    return r


def texel_centres(sc, t):
    """uv whose texture-space position is EXACTLY the centre of a level-0 texel of record t (identity scale / offset): float32 u with u * w == x + 0.5 without rounding
    error, searched among the neighbours of (x + 0.5) / w.  Returns uv [n, 2], the texel indices [n, 2]"""
    tx = sc.textures[t]; assert (tx["uscale"], tx["vscale"], tx["uoffset"], tx["voffset"]) == (1.0, 1.0, 0.0, 0.0)
    w, h = (int(v) for v in sc.texture_levels[tx["first_level"]][:2])
    def exact(n):
        out = {}
        for x in range(n):
            u = f32((x + 0.5) / n)
            for _ in range(4): u = np.nextafter(u, f32(0))
            for _ in range(9):
                if f32(u * f32(n)) == f32(x + 0.5): out[x] = u; break
                u = np.nextafter(u, f32(1))
        return out
    ex, ey = exact(w), exact(h)
    xy = np.array([(x, y) for y in ey for x in ex], np.int64)
    return np.array([(ex[x], ey[y]) for x, y in xy], f32), xy


# ------------------------------------------------------------------------------------------------ the oracle's side, computed once per session
_BSDF_REF, _TEX_REF = {}, {}


def bsdf_reference(oracle, golden_scenes, name):
    """per unrefused record of golden scene `name`: the inputs and the oracle's answers -- dict(inp, sampled [n, 10], wo [n, 3], evald [n, 4])"""
    if name not in _BSDF_REF:
        sc = golden_scenes[name]; orc = oracle.Oracle(sc); out = {}
        for m in records(sc):
            inp = bsdf_inputs(name, m); sampled = orc.bsdf_sample_units(m, inp["wi"], inp["uv"], inp["extra"])
            wo = eval_wo(inp, sampled)
            out[m] = dict(inp=inp, sampled=sampled, wo=wo, evald=orc.bsdf_eval_units(m, inp["wi"], wo))
        _BSDF_REF[name] = out
    return _BSDF_REF[name]


def texture_reference(oracle, S):
    """the texture scene and, per record: uv, partials, the oracle's filtered lookups with what each did (info), its lookups without partials, and `keep` = the
    lookups whose EWA loops stay under MAX_EWA_TEXELS (the only ones a device run may be given)"""
    if "ref" not in _TEX_REF:
        sc = texture_scene(S); orc = oracle.Oracle(sc); per = {}
        for t in range(len(sc.textures)):
            uv, pa = texture_inputs(sc, t)
            ref, info = orc.texture_units(t, uv, pa, info=True)
            per[t] = dict(uv=uv, pa=pa, ref=ref, info=info, plain=orc.texture_units(t, uv), keep=info[:, 2] <= MAX_EWA_TEXELS)
        _TEX_REF["ref"] = (sc, orc, per)
    return _TEX_REF["ref"]
