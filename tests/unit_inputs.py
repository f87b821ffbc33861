"""Inputs of the unit-level comparisons of the BSDF, texture and emitter routines (tests/test_unit_inputs.py on the CPU, tests/test_gpu_units.py and
tests/test_gpu_light_units.py on the device): one generator,
fixed seeds, so that both sides and both tests see the same numbers.  Directions and sample values are aimed at what camera-driven paths almost never produce:
grazing and exactly normal incidence, sample values 0 and 1 - 2^-24, directions below a one-sided surface, texture coordinates on texel edges and wrap seams,
degenerate and non-finite footprints.  The surface step between a hit and the BSDF query (tests/test_surface_inputs.py, tests/test_gpu_surface_units.py) gets rays aimed at
chosen primitives instead: see surface_inputs."""
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


# ------------------------------------------------------------------------------------------------ emitters
# Inputs of the comparisons of Scene::sampleEmitterDirect and of what a BSDF-sampled ray that finds an emitter evaluates (mi_debug_emitter_sample / _eval against
# orc_emitter_sample_units / orc_emitter_eval_units): reference points on the lights' planes, at their vertices, inside and far from a sphere light, on a spot light's
# cones, behind a directional light's disk and outside the environment's bounding sphere; sample values on the entries of the tables the searches walk.
LIGHT_SCENES = ["cornell_small", "cbox_lights", "cbox_collimated", "open_constant", "shape_lights", "atrium_small", "fog_sky", "sky_view", "veach_small"]
N_LIGHT = 4096
ENV_SIZES = [(5, 3), (8, 4), (64, 32)]            # width, height of the unit scene's environment maps: the odd ones give guide tables with more buckets than bins
UNIT_LIGHT_SCENES = [f"light_units_{w}x{h}" for w, h in ENV_SIZES]
MI_EPSILON = 1e-4
TWO_M32 = 2.0 ** -32
EMITTER_KIND_NAMES = {0: "area", 1: "envmap", 2: "constant", 3: "point", 4: "spot", 5: "directional", 7: "collimated"}
SINGLE_TEXEL_ROW = 1                              # the row of the unit scene's maps that holds one non-black texel


def light_envmap(w, h):
    """dim rows (0.01 .. 0.05) with one lit texel each at the seam columns 0 and w - 1 and in the pole rows 0 and h - 1; row SINGLE_TEXEL_ROW holds a single
    non-black texel (column w // 2): its column table is all empty bins but one.  No row is entirely black: its table would be 0 x infinity on every side, which the
    reference does not define."""
    rng = np.random.default_rng([w, h, 577]); rgb = rng.uniform(0.01, 0.05, (h, w, 3))
    rgb[0, 0] = (40.0, 30.0, 20.0); rgb[h - 1, w - 1] = (10.0, 30.0, 50.0)
    if h > 3: rgb[2, w - 1] = (25.0, 25.0, 5.0); rgb[h - 2, 0] = (5.0, 20.0, 20.0)
    rgb[SINGLE_TEXEL_ROW] = 0.0; rgb[SINGLE_TEXEL_ROW, w // 2] = (3.0, 2.0, 1.0)
    return np.ascontiguousarray(rgb, f32)


def light_scene(S, w, h):
    """The unit scene: a floor, a light mesh of three triangles and one of five, each with a zero-area triangle (empty bins on both routes of the triangle search),
    under a w x h environment map.  The zero-area triangle sits in the middle of each mesh, under the 8 x 4 map at its head: a search arrives at an empty bin only
    where the table starts with one (v = 0), and DiscreteDistribution::sample then steps on to the first bin that is not empty -- unlike the environment map's
    sampleReuse, which has no such step (emitter_sample_inputs).  Emitter weights 2, 1, 1: the selection table is 0, 0.5, 0.75, 1, so that the reused sample of the environment
    map is 2 u without a rounding error.  The 5 x 3 map sits in the world frame (world directions are its local ones), the others are rotated."""
    verts, tris, shapes = [], [], []
    def mesh(points, faces, bsdf, emitter):
        fv, ft = len(verts), len(tris); verts.extend(points); tris.extend([tuple(fv + i for i in f) for f in faces])
        shapes.append(dict(first_tri=ft, tri_count=len(faces), first_vert=fv, vert_count=len(points), bsdf=bsdf, emitter=emitter, face_normals=1, group=0, interior=-1, exterior=-1))
    mesh([(4, 0, -4), (-4, 0, -4), (-4, 0, 4), (4, 0, 4)], [(0, 1, 2), (0, 2, 3)], 0, -1)
    # (1, 2, 0), (0, 2, 1), (0.5, 2, 0.5) lie on one line: the cross product of the sides is exactly zero
    head = (w, h) == ENV_SIZES[1]; order = (lambda f, k: [f[k]] + f[:k] + f[k + 1:]) if head else (lambda f, k: f)
    mesh([(0, 2, 0), (1, 2, 0), (0, 2, 1), (0.5, 2, 0.5), (1, 2, 1)], order([(0, 1, 2), (1, 2, 3), (1, 4, 2)], 1), 1, 1)
    mesh([(2, 2.5, 0), (3, 2.5, 0), (2, 2.5, 1), (2.5, 2.5, 0.5), (3, 2.5, 1), (4, 2.5, 0), (4, 2.5, 1)], order([(0, 1, 2), (1, 4, 2), (1, 2, 3), (1, 5, 4), (5, 6, 4)], 2), 1, 2)
    bsdfs = [S.make_bsdf(reflectance=(0.5, 0.5, 0.5)), S.make_bsdf(reflectance=(0.0, 0.0, 0.0))]
    emitters = [dict(type=S.EMITTER_ENVMAP, shape=-1, radiance=(0.0, 0.0, 0.0), weight=2.0), dict(type=S.EMITTER_AREA, shape=1, radiance=(9.0, 7.0, 5.0), weight=1.0),
                dict(type=S.EMITTER_AREA, shape=2, radiance=(2.0, 6.0, 3.0), weight=1.0)]
    to_world = np.eye(4, dtype=f32) if (w, h) == ENV_SIZES[0] else (S.rotate((0, 1, 0), 25.0) @ S.rotate((1, 0, 0), 8.0)).astype(f32)
    env = dict(rgb=light_envmap(w, h), to_world=to_world, scale=0.8, filtered=False)
    cam = S.look_at((0.5, 1.0, -5.0), (0.5, 1.0, 0.0), (0, 1, 0))
    return S.finish_scene(verts, tris, shapes, bsdfs, emitters, cam, 50.0, 0.05, 100.0, 32, 32, 1, S.SAMPLER_SOBOL, 4, 3, envmap=env, name=f"light_units_{w}x{h}")


def emitter_cdf(sc):
    """the emitter-selection table as both sides build it (float32 running sum, times the reciprocal of the total, last entry 1)"""
    c = [f32(0)]
    for e in sc.emitters: c.append(f32(c[-1] + f32(e["weight"])))
    norm = f32(1) / c[-1]; c = [f32(x * norm) for x in c]; c[0] = f32(0); c[-1] = f32(1)
    return np.asarray(c, f32)


def guide_buckets(w, h):
    """bucket counts of the guide tables of a w x h environment map (rows, columns): csrc/scene_build.cpp"""
    p2 = lambda v: 1 << max(0, int(v - 1).bit_length())
    return min(p2(h), 4096), min(max(p2(w) // 4, 1), 1024)


def _mesh_lights(sc):
    """(emitter index, triangles [t, 3, 3]) of every area light on a mesh"""
    return [(e, sc.pos[sc.idx[sc.shapes[em["shape"]]["first_tri"]:sc.shapes[em["shape"]]["first_tri"] + sc.shapes[em["shape"]]["tri_count"]]].astype(np.float64))
            for e, em in enumerate(sc.emitters) if em["type"] == 0 and em["shape"] < len(sc.shapes)]


def _analytic_lights(sc):
    return [(e, sc.analytic[em["shape"] - len(sc.shapes)]) for e, em in enumerate(sc.emitters) if em["type"] == 0 and em["shape"] >= len(sc.shapes)]


def scene_box(sc):
    """the box both sides derive the directional light's disk and the environment's bounding sphere from: the vertices and the boxes of the analytic shapes (a
    sphere's exactly, the others' by their corner points -- no scene here has one of those next to a directional or environment emitter)"""
    lo, hi = sc.pos.min(0).astype(np.float64), sc.pos.max(0).astype(np.float64)
    for a in sc.get("analytic") or []:
        m = np.asarray(a["to_world"], np.float64).reshape(4, 4)
        if a["type"] == 2: pts = [m[:3, 3] - a["radius"], m[:3, 3] + a["radius"]]
        else:
            r = a["radius"] if a["type"] == 3 else 1.0; z = [0.0, a["length"]] if a["type"] == 3 else [0.0]
            pts = [(m @ np.array([x, y, zz, 1.0]))[:3] for x in (-r, r) for y in (-r, r) for zz in z]
        lo = np.minimum(lo, np.min(pts, 0)); hi = np.maximum(hi, np.max(pts, 0))
    return lo, hi


def _unit(rng, n):
    v = rng.normal(size=(n, 3)); return v / np.linalg.norm(v, axis=1, keepdims=True)


def spot_tables(em):
    """cos(cutoff), cos(beam) and the rotation part of the inverse transform of a spot light as both sides store them (float32; cosf through the double routine)"""
    import math
    rad = f32(np.pi) / f32(180.0); cutoff = f32(em["cutoff"]) * rad; beam = f32(em["beam"]) * rad
    m = np.asarray(em["to_world"], f32).reshape(4, 4); a = [m[0, 0], m[0, 1], m[0, 2], m[1, 0], m[1, 1], m[1, 2], m[2, 0], m[2, 1], m[2, 2]]
    det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]); i = f32(1) / det
    row2 = [(a[3] * a[7] - a[4] * a[6]) * i, (a[1] * a[6] - a[0] * a[7]) * i, (a[0] * a[4] - a[1] * a[3]) * i]
    return f32(math.cos(float(cutoff))), f32(math.cos(float(beam))), np.asarray(row2, f32)


def spot_cos_theta(em, ref):
    """Frame::cosTheta of the direction from a spot light to `ref` [n, 3] in the light's frame, in the operation order of SpotEmitter::sampleDirect (float32)"""
    _, _, r2 = spot_tables(em); m = np.asarray(em["to_world"], f32).reshape(4, 4); ref = np.asarray(ref, f32)
    dx, dy, dz = (m[0, 3] - ref[:, 0]), (m[1, 3] - ref[:, 1]), (m[2, 3] - ref[:, 2])
    inv = f32(1) / np.sqrt(dx * dx + dy * dy + dz * dz); dx, dy, dz = dx * inv, dy * inv, dz * inv
    return r2[0] * -dx + r2[1] * -dy + r2[2] * -dz


def _spot_points(em, rng, scale):
    """reference points whose cosTheta is EXACTLY the stored cut-off cosine, the stored beam cosine, or one ulp either side of one of them: candidates around each
    cone, kept where spot_cos_theta hits the target; in the order (below, on, above) x (cut-off, beam), repeated.  test_unit_inputs checks through the oracle's zones
    that the targets were hit."""
    cc, cb, _ = spot_tables(em); m = np.asarray(em["to_world"], np.float64).reshape(4, 4); per = []
    targets = [t for c in (cc, cb) for t in (np.nextafter(c, f32(-1)), c, np.nextafter(c, f32(2)))]
    k = 20000; theta0 = np.arccos(np.asarray([float(c) for c in (cc, cb)]))
    for j, t in enumerate(targets):
        th = theta0[j // 3] + rng.uniform(-4e-7, 4e-7, k); ph = rng.uniform(0, 2 * np.pi, k); dist = rng.uniform(0.2, 1.0, k) * scale
        local = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], 1)
        ref = (m[:3, 3] + (local @ m[:3, :3].T) * dist[:, None]).astype(f32)
        hit = ref[spot_cos_theta(em, ref) == t]
        assert len(hit) >= 8, (j, len(hit))
        per.append(hit[:64])
    n = min(len(p) for p in per)
    return np.stack([p[:n] for p in per], 1).reshape(-1, 3)            # rows 6 i .. 6 i + 5: the six targets


def light_points(sc, rng):
    """the special reference points of a scene, one array [k, 3] per kind"""
    lo, hi = scene_box(sc); size = float(np.linalg.norm(hi - lo)); out = {}
    tris = [t for _, ts in _mesh_lights(sc) for t in ts if np.linalg.norm(np.cross(t[1] - t[0], t[2] - t[0])) > 0]
    if tris:
        T = np.asarray(tris); k = 256; t = T[rng.integers(0, len(T), k)]; ab = rng.uniform(-1.0, 2.0, (k, 2))
        out["light_plane"] = t[:, 0] + (t[:, 1] - t[:, 0]) * ab[:, :1] + (t[:, 2] - t[:, 0]) * ab[:, 1:]
        out["light_vertex"] = np.asarray([t for _, ts in _mesh_lights(sc) for t in ts]).reshape(-1, 3)
    for e, a in _analytic_lights(sc):
        m = np.asarray(a["to_world"], np.float64).reshape(4, 4)
        if a["type"] in (0, 1):
            xy = rng.uniform(-2.0, 2.0, (128, 2)); out[f"light_plane_{e}"] = (np.concatenate([xy, np.zeros((128, 1)), np.ones((128, 1))], 1) @ m.T)[:, :3]
        if a["type"] == 2:
            c, r = m[:3, 3], a["radius"]; u = _unit(rng, 96)
            band = r / (1.0 - MI_EPSILON * np.repeat([0.5, 0.9, 1.0, 1.1, 2.0, 10.0], 16))      # sinAlpha = radius / distance around 1 - epsilon, from both sides
            out[f"sphere_{e}"] = np.concatenate([np.tile(c, (8, 1)), c + u[:16] * r, c + u * band[:, None], c + u[:16] * r * 0.5, c + u[:32] * r * 1e4])
    for em in sc.emitters:
        m = np.asarray(em.get("to_world", np.eye(4)), np.float64).reshape(4, 4)
        if em["type"] in (3, 4): out.setdefault("light_position", []).append(m[:3, 3])
        if em["type"] == 4: out["spot_cones"] = _spot_points(em, rng, 0.5 * size)
        if em["type"] == 5:
            d = m[:3, 2]; c = 0.5 * (lo + hi); r = 0.5 * size * 1.1; centre = c - d * r; t = np.cross(d, _unit(rng, 96)); s = rng.uniform(0.0, 2.0, (96, 1)) * r
            out["directional_disk"] = np.concatenate([centre + t[:48] * s[:48], centre + t[48:] * s[48:] - d * rng.uniform(0.0, 1.0, (48, 1)) * r])
        if em["type"] in (1, 2):
            cam = np.asarray(sc.cam_to_world, np.float64).reshape(4, 4)[:3, 3]; l2, h2 = np.minimum(lo, cam), np.maximum(hi, cam)
            c = 0.5 * (l2 + h2); r = max(MI_EPSILON, 0.5 * float(np.linalg.norm(h2 - l2)) * 1.5); u = _unit(rng, 192)
            # on the sphere, and outside it by a share of 1e-4 .. 0.2 of the radius: close enough for a sampled direction to meet the sphere ahead or behind about as often as it misses
            out["environment_sphere"] = np.concatenate([c + u[:32] * r, c + u[32:] * r * (1.0 + 10.0 ** rng.uniform(-4.0, -0.7, (160, 1)))])
    if "light_position" in out: out["light_position"] = np.tile(np.asarray(out["light_position"]), (16, 1))
    return {k: np.asarray(v, np.float64) for k, v in out.items()}


def _env_row_cdf(rgb):
    lum = rgb.astype(np.float64) @ np.array([0.212671, 0.715160, 0.072169]); h = len(lum)
    c = np.concatenate([[0.0], np.cumsum(lum.sum(1) * np.sin((np.arange(h) + 0.5) * np.pi / h))]); return c / c[-1]


def sample_edges(sc):
    """sample values on the entries of the tables the searches walk, each with its float32 neighbours: for u the emitter table's entries and k / n, and -- mapped back
    through the sample reuse of the environment emitter's bin -- the bucket borders b / K of the column guide tables; for v the borders of the row guide table and the
    entries of every light mesh's triangle table"""
    def around(x):
        x = np.asarray(x, f32).reshape(-1); a = np.concatenate([np.nextafter(x, f32(-1)), x, np.nextafter(x, f32(2))]); return a[(a > 0) & (a < 1)]      # 0 has its own share; 1 is no sample value
    c = emitter_cdf(sc); n = len(sc.emitters); u = [c, np.arange(n + 1, dtype=f32) / f32(n)]; v = []
    if sc.envmap is not None:
        h, w = sc.envmap["rgb"].shape[:2]; kr, kc = guide_buckets(w, h); e = [i for i, em in enumerate(sc.emitters) if em["type"] == 1][0]
        u.append(c[e] + (c[e + 1] - c[e]) * (np.arange(kc + 1, dtype=f32) / f32(kc))); v.append(np.arange(kr + 1, dtype=f32) / f32(kr)); v.append(_env_row_cdf(sc.envmap["rgb"]))
    for _, ts in _mesh_lights(sc):
        area = 0.5 * np.linalg.norm(np.cross(ts[:, 1] - ts[:, 0], ts[:, 2] - ts[:, 0]), axis=1); v.append(np.cumsum(area) / area.sum()); v.append(np.arange(len(ts) + 1) / len(ts))
    return around(np.concatenate(u)), (around(np.concatenate(v)) if v else np.zeros(0, f32))


def emitter_sample_inputs(name, sc):
    """ref [n, 3], ref_n [n, 3], uv [n, 2], `kinds`: which special kind of reference point a case holds ("" = uniform in the box), and `spot_target`: for a point of
    _spot_points which of its six targets it hits (else -1)"""
    rng = np.random.default_rng([zlib.crc32(name.encode()), 1618]); n = N_LIGHT
    lo, hi = scene_box(sc); ref = rng.uniform(lo, hi, (n, 3)); kinds = np.array([""] * n, dtype=object); target = np.full(n, -1)
    special = light_points(sc, rng); m = n // 2; names = sorted(special)
    if "environment_sphere" in names: names += ["environment_sphere"] * 2             # (three turns: of its points only those the emitter search gives to the environment count, and of those a sampled direction must still meet the sphere)
    # the second half: the special kinds in turn
    for j in range(m):
        k = names[j % len(names)]; p = special[k]
        if k == "spot_cones": i = (j // len(names)) % len(p); row = p[i]; target[n - m + j] = i % 6      # in order: all six targets come up equally often
        else: row = p[rng.integers(0, len(p))]
        ref[n - m + j] = row; kinds[n - m + j] = k
    nrm = _unit(rng, n); nrm[::5] = 0.0                                             # every fifth one a two-sided surface
    ue, ve = sample_edges(sc); uv = np.minimum(rng.uniform(size=(n, 2)).astype(f32), f32(ONE_MINUS))
    for col, edges in ((0, ue), (1, ve)):
        r = rng.integers(0, 16, n); uv[r == 0, col] = 0.0; uv[r == 1, col] = ONE_MINUS; uv[r == 2, col] = TWO_M32
        if len(edges): pick = r == 3; uv[pick, col] = edges[rng.integers(0, len(edges), int(pick.sum()))]
    # u = 0 is given only to tables whose first bin is not empty.  An empty first bin turns the reused sample into 0 / 0 and then -- through the tent warp and
    # floorf -- into a float-to-int conversion of NaN, which C leaves undefined.  That is the environment map's sampleReuse; of its tables only the column table of
    # the unit maps' SINGLE_TEXEL_ROW starts with empty bins: a case whose v selects that row (or lies within 1e-6 of its interval) takes u = 2^-32 in place of 0.
    # Both searches then still cross the empty bins.  (The emitter and triangle tables are DiscreteDistribution::sample's, which steps over empty bins before the
    # sample is reused: v = 0 on the 8 x 4 scene's triangle tables, which start with an empty bin, is defined and stays.)
    if name in UNIT_LIGHT_SCENES:
        rc = _env_row_cdf(sc.envmap["rgb"]); r = SINGLE_TEXEL_ROW
        hit = (uv[:, 0] == 0) & (uv[:, 1] >= rc[r] - 1e-6) & (uv[:, 1] <= rc[r + 1] + 1e-6); uv[hit, 0] = TWO_M32
    return dict(ref=np.ascontiguousarray(ref, f32), ref_n=np.ascontiguousarray(nrm, f32), uv=np.ascontiguousarray(uv), kinds=kinds, spot_target=target)


EVAL_DIRECTIONS = [(0, 1, 0), (0, -1, 0), (0.0, 0.3, 0.9539392), (-0.0, 0.3, 0.9539392), (0.0, -0.6, 0.8), (1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1),
                   (0, 0.6, 0.8), (0.6, 0, 0.8), (0.6, 0.8, 0), (0, 0.6, -0.8), (-0.6, 0.8, 0)]      # the poles, the seam (x = +-0, z > 0), the axes, a zero component


def evaluable(sc):
    return [e for e, em in enumerate(sc.emitters) if em["type"] in (0, 1, 2)]


def emitter_eval_inputs(name, sc, e, sample_inp, sampled):
    """the inputs of what a BSDF-sampled ray that finds emitter e evaluates: ref [n, 3], d [n, 3], n [n, 3], dist [n], facing [n].  Directions: uniform, with a quarter
    out of EVAL_DIRECTIONS (for an environment map in its own frame and in the world's) and on the borders and centres of its texels; emitter normals: uniform, with a
    quarter at |d . n| of 0, 1e-7, 1e-4; every fourth case is the oracle's own sample for emitter_sample_inputs' case where that chose emitter e (`sampled`)."""
    ev = evaluable(sc); n = N_LIGHT // len(ev); rng = np.random.default_rng([zlib.crc32(name.encode()), e, 3141]); em = sc.emitters[e]
    lo, hi = scene_box(sc); size = float(np.linalg.norm(hi - lo)); ref = rng.uniform(lo, hi, (n, 3)); d = _unit(rng, n)
    pts = light_points(sc, rng).get(f"sphere_{e}")                                    # a sphere light: half of the reference points at its centre, on it, in its band, far away
    if pts is not None: j = np.arange(n // 2, n); ref[j] = pts[rng.integers(0, len(pts), len(j))]
    edge = rng.uniform(size=n) < 0.25; ed = np.asarray(EVAL_DIRECTIONS, np.float64)[rng.integers(0, len(EVAL_DIRECTIONS), n)]
    if em["type"] == 1:
        h, w = sc.envmap["rgb"].shape[:2]; m = np.asarray(sc.envmap["to_world"], np.float64).reshape(4, 4)[:3, :3]
        # directions through the borders and the centres of texels: (col + 0 or 0.5) / w, (row + 0 or 0.5) / h
        tex = rng.uniform(size=n) < 0.25; ph = 2 * np.pi * rng.integers(0, 2 * w + 1, n) / (2 * w); th = np.pi * rng.integers(0, 2 * h + 1, n) / (2 * h)
        tdir = np.stack([np.sin(ph) * np.sin(th), np.cos(th), -np.cos(ph) * np.sin(th)], 1)
        ed = np.where(tex[:, None] & ~edge[:, None], tdir, ed); edge |= tex
        local = rng.uniform(size=n) < 0.5; ed = np.where(local[:, None], ed @ m.T, ed)
    d = np.where(edge[:, None], ed, d).astype(f32)
    t = np.cross(d.astype(np.float64), _unit(rng, n)); t /= np.maximum(np.linalg.norm(t, axis=1, keepdims=True), 1e-30)
    c = np.where(rng.uniform(size=n) < 0.25, np.asarray([0.0, 1e-7, 1e-4])[rng.integers(0, 3, n)], rng.uniform(0.0, 1.0, n)) * np.where(rng.uniform(size=n) < 0.75, -1.0, 1.0)
    nrm = (t * np.sqrt(1 - c * c)[:, None] + d * c[:, None]).astype(f32)
    dist = (rng.uniform(0.01, 1.0, n) * size).astype(f32); facing = (rng.uniform(size=n) < 0.75).astype(f32)
    ref = ref.astype(f32)
    mine = np.flatnonzero((sampled[:, 14] == e) & (sampled[:, 10] != 0) & np.isfinite(sampled[:, 3:14]).all(1))
    take = np.arange(0, n, 4)[:len(mine)]
    if len(take):
        src = mine[:len(take)]; ref[take] = sample_inp["ref"][src]; d[take] = sampled[src, 6:9]; nrm[take] = sampled[src, 11:14]; dist[take] = sampled[src, 9]; facing[take] = 1.0
    return dict(ref=ref, d=np.ascontiguousarray(d, f32), n=nrm, dist=dist, facing=facing)


_LIGHT_REF = {}


def light_scenes(golden_scenes, S):
    """name -> scene: the golden scenes of LIGHT_SCENES and the three unit scenes"""
    if "scenes" not in _LIGHT_REF:
        _LIGHT_REF["scenes"] = {**{k: golden_scenes[k] for k in LIGHT_SCENES}, **{f"light_units_{w}x{h}": light_scene(S, w, h) for w, h in ENV_SIZES}}
    return _LIGHT_REF["scenes"]


def light_reference(oracle, golden_scenes, S, name):
    """the inputs of scene `name` and the oracle's answers, computed once: dict(sc, sample = dict(inp, out [n, 17], branches, raw [n, 17]), eval = {emitter:
    dict(inp, out [n, 8], branches)})"""
    if name not in _LIGHT_REF:
        sc = light_scenes(golden_scenes, S)[name]; orc = oracle.Oracle(sc); inp = emitter_sample_inputs(name, sc)
        out, br = orc.emitter_sample_units(inp["ref"], inp["ref_n"], inp["uv"]); raw, _ = orc.emitter_sample_units(inp["ref"], inp["ref_n"], inp["uv"], raw=True)
        ev = {}
        for e in evaluable(sc):
            ei = emitter_eval_inputs(name, sc, e, inp, out); eo, eb = orc.emitter_eval_units(e, ei["ref"], ei["d"], ei["n"], ei["dist"], ei["facing"])
            ev[e] = dict(inp=ei, out=eo, branches=eb)
        _LIGHT_REF[name] = dict(sc=sc, sample=dict(inp=inp, out=out, branches=br, raw=raw), eval=ev)
    return _LIGHT_REF[name]


# ------------------------------------------------------------------------------------------------ participating media
# Inputs of the comparisons of the medium routines (mi_debug_medium against orc_medium_units): the records of the fog scenes and those of a table of its own.
MEDIUM_SCENES = ["fog_box", "fog_mis", "fog_sky"]
N_MEDIUM = 2048
FLT_MIN = float(np.finfo(f32).tiny)
HG_G = [0.0, 5e-5, 1.5e-4, 0.4, -0.4, 0.9, -0.9, 0.999, -0.999]      # 5e-5 and 1.5e-4: either side of the |g| < epsilon switch of the Henyey-Greenstein map
AXES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float64)


def medium_scene(S):
    """the unit light scene under a medium table of its own (no shape refers to it: the routines are called on the records): the manual strategy, a channel with
    sigma_t = 0 under each strategy, medium_sampling_weight of 1, 0.5, 2^-10 and the smallest normal float (neither make_medium nor the commit refuses a weight), and a
    Henyey-Greenstein record per entry of HG_G"""
    sc = light_scene(S, *ENV_SIZES[1]); sa, ss = (0.05, 0.1, 0.2), (0.9, 0.8, 0.7)
    media = [S.make_medium(sa, ss, strategy=S.MEDIUM_MANUAL, sampling_density=0.7),
             S.make_medium((0.0, 0.1, 0.2), (0.0, 0.5, 0.3)), S.make_medium((0.0, 0.1, 0.2), (0.0, 0.5, 0.3), strategy=S.MEDIUM_SINGLE), S.make_medium((0.2, 0.0, 0.1), (0.3, 0.0, 0.5), strategy=S.MEDIUM_SINGLE, channel=0),
             S.make_medium((0.0, 0.1, 0.2), (0.0, 0.5, 0.3), strategy=S.MEDIUM_MANUAL, sampling_density=0.4)]
    media += [S.make_medium(sa, ss, medium_sampling_weight=w) for w in (1.0, 0.5, 2.0 ** -10, FLT_MIN)]
    media += [S.make_medium((0.2, 0.05, 0.2), (0.5, 1.0, 0.5), strategy=S.MEDIUM_SINGLE, medium_sampling_weight=w) for w in (1.0, 2.0 ** -10)]
    media += [S.make_medium(sa, ss, phase=S.PHASE_HG, g=g) for g in HG_G]
    sc.media = media; sc.sensor_medium = -1; sc.integrator = S.INTEGRATOR_VOLPATH_SIMPLE; sc.name = "medium_units"
    sc.shape_media = np.full((len(sc.shapes) + len(sc.analytic), 2), -1, np.int32)
    return sc


def _directions_with_axes(rng, n):
    d = _unit(rng, n); ax = rng.uniform(size=n) < 0.25; d[ax] = AXES[rng.integers(0, 6, int(ax.sum()))]; return d


def _with_edges(rng, x, edges):
    """one in sixteen of x replaced by each entry of `edges`"""
    r = rng.integers(0, 16, len(x)); x = x.copy()
    for j, e in enumerate(edges[:15]): x[r == j] = e
    return x


def medium_inputs(name, record, med):
    """per mode the inputs [n, 10] of mi_debug_medium / orc_medium_units for one medium record"""
    rng = np.random.default_rng([zlib.crc32(name.encode()), record, 1414]); n = N_MEDIUM; w = f32(med["medium_sampling_weight"]); out = {}
    # transmittance over [mint, maxt]: lengths 1e-6 .. 300 (the longest leave nothing of any channel), mint = maxt, maxt = infinity
    t = np.zeros((n, 10)); t[:, 6] = rng.uniform(0.0, 2.0, n); t[:, 7] = t[:, 6] + 10.0 ** rng.uniform(-6.0, 2.5, n)
    r = rng.integers(0, 16, n); t[r == 0, 7] = t[r == 0, 6]; t[r == 1, 7] = np.inf
    out["transmittance"] = t.astype(f32)
    # distance sampling
    a = np.zeros((n, 10)); a[:, 0:3] = rng.uniform(-2.0, 2.0, (n, 3)); a[:, 3:6] = _directions_with_axes(rng, n)
    a[:, 6] = np.where(rng.uniform(size=n) < 0.5, 0.0, rng.uniform(0.0, 1.0, n)); a[:, 7] = a[:, 6] + 10.0 ** rng.uniform(-3.0, 2.0, n)
    r = rng.integers(0, 16, n); a[r == 0, 7] = a[r == 0, 6]; a[r == 1, 7] = np.inf
    # a quarter: segments that leave less than 1e-20 of every channel (50 .. 500 mean free paths of the thinnest one; with a channel of sigma_t = 0 nothing does)
    st = np.asarray(med["sigma_a"], np.float64) + np.asarray(med["sigma_s"], np.float64); thin = st.min() if st.min() > 0 else 1.0
    far = (r >= 2) & (r <= 5); a[far, 7] = a[far, 6] + rng.uniform(50.0, 500.0, int(far.sum())) / thin
    # the first value: uniform, half of them scaled into [0, weight) so that a small weight still chooses the medium; 0, the weight itself and one ulp below it,
    # 1 - 2^-24, 2^-32, and -- with an origin of magnitude 1e4 and mint = 0 -- weight * 2^-32 and weight * 2^-20: distances so short that o + t d == o
    u = rng.uniform(size=n); u = np.where(rng.uniform(size=n) < 0.5, u * float(w), u)
    u = _with_edges(rng, np.minimum(u.astype(f32), f32(ONE_MINUS)), [0.0, w, np.nextafter(w, f32(0)), ONE_MINUS, TWO_M32, f32(w * f32(TWO_M32)), f32(w * f32(2.0 ** -20))])
    short = (u == f32(w * f32(TWO_M32))) | (u == f32(w * f32(2.0 ** -20))); a[short, 0:3] = _unit(rng, int(short.sum())) * 1e4; a[short, 6] = 0.0; a[short, 7] = 1e3
    third, two = f32(1.0 / 3.0), f32(2.0 / 3.0)
    v = _with_edges(rng, np.minimum(rng.uniform(size=n).astype(f32), f32(ONE_MINUS)), [0.0, ONE_MINUS, np.nextafter(third, f32(0)), third, np.nextafter(third, f32(1)), np.nextafter(two, f32(0)), two, np.nextafter(two, f32(1))])
    a[:, 8] = np.minimum(u, f32(ONE_MINUS)); a[:, 9] = v
    out["distance"] = a.astype(f32)
    # phase function: wi uniform, a quarter along the axes; the 2-D sample with its edge values
    p = np.zeros((n, 10)); p[:, 0:3] = _directions_with_axes(rng, n)
    for col in (3, 4): p[:, col] = _with_edges(rng, np.minimum(rng.uniform(size=n).astype(f32), f32(ONE_MINUS)), [0.0, ONE_MINUS, TWO_M32, 0.5])
    out["phase_sample"] = p.astype(f32)
    e = np.zeros((n, 10)); e[:, 0:3] = _directions_with_axes(rng, n); e[:, 3:6] = _directions_with_axes(rng, n)
    r = rng.integers(0, 16, n); e[r == 0, 3:6] = e[r == 0, 0:3]; e[r == 1, 3:6] = -e[r == 1, 0:3]      # the two peaks of the lobe
    out["phase_eval"] = e.astype(f32)
    return out


def medium_scenes(golden_scenes, S):
    if "media" not in _LIGHT_REF: _LIGHT_REF["media"] = {**{k: golden_scenes[k] for k in MEDIUM_SCENES}, "medium_units": medium_scene(S)}
    return _LIGHT_REF["media"]


def medium_reference(oracle, golden_scenes, S, name):
    """per medium record of scene `name`: {mode: dict(inp, out [n, 12], branches)}; every fourth phase_eval case takes the oracle's own sample of the phase_sample
    case of the same row"""
    key = "media:" + name
    if key not in _LIGHT_REF:
        sc = medium_scenes(golden_scenes, S)[name]; orc = oracle.Oracle(sc); per = {}
        for m, med in enumerate(sc.media):
            inp = medium_inputs(name, m, med); sampled, _ = orc.medium_units(m, "phase_sample", inp["phase_sample"])
            inp["phase_eval"][::4, 0:3] = inp["phase_sample"][::4, 0:3]; inp["phase_eval"][::4, 3:6] = sampled[::4, 0:3]
            per[m] = {mode: dict(zip(("out", "branches"), orc.medium_units(m, mode, a)), inp=a) for mode, a in inp.items()}
        _LIGHT_REF[key] = dict(sc=sc, records=per)
    return _LIGHT_REF[key]


# ------------------------------------------------------------------------------------------------ the surface step
# Inputs of the comparison of the surface step between a hit and the BSDF query (mi_debug_surface against orc_surface_units): rays AIMED at a chosen primitive and
# target point -- grazing incidence, triangle edges and vertices, seams, poles and centres of the analytic shapes, target uv on texel edges and wrap seams of the bound
# bitmap -- with differentials scaled by 1, 1e-3 and 1e3, perpendicular to the surface or non-finite; on the committed textured scenes and two unit scenes.
SURFACE_SCENES = ["layered_room", "layered_room_procedural", "masked_room", "bitmap_room", "textured_plastics", "textured_plastics_smooth", "textured_shapes"]
SURFACE_UNIT_SCENES = ["surface_units_instanced", "surface_units_edges"]
N_SURFACE, N_SURFACE_UNIT = 2048, 4096
DIFF_SCALES = [1.0, 1e-3, 1e3]
BUMP_SCALES = [0.0, -1.0, 1e4]
CONSTANT_NORMALS = [(0.5, 0.5, 1.0), (0.5, 0.5, 0.5), (0.5, 0.5, 0.0)]


class _Meshes:
    def __init__(self): self.verts, self.tris, self.nrm, self.uv, self.shapes = [], [], [], [], []

    def add(self, pts, faces, bsdf, uv=None, normals=None, group=0, emitter=-1):
        fv, ft = len(self.verts), len(self.tris); self.verts += [tuple(map(float, p)) for p in pts]; self.tris += [tuple(fv + i for i in f) for f in faces]
        self.uv += [tuple(t) for t in uv] if uv is not None else [(0.0, 0.0)] * len(pts); self.nrm += [tuple(t) for t in normals] if normals is not None else [(0.0, 1.0, 0.0)] * len(pts)
        self.shapes.append(dict(first_tri=ft, tri_count=len(faces), first_vert=fv, vert_count=len(pts), bsdf=bsdf, emitter=emitter, face_normals=int(normals is None), group=group,
                                has_uv=int(uv is not None), interior=-1, exterior=-1))
        return len(self.shapes) - 1

    def quad(self, x0, x1, z0, z1, bsdf, group=0, uv=((0, 0), (0, 1), (1, 1), (1, 0))):
        """in the plane y = 0, facing +y"""
        return self.add([(x0, 0, z0), (x0, 0, z1), (x1, 0, z1), (x1, 0, z0)], [(0, 1, 2), (0, 2, 3)], bsdf, uv=uv, group=group)

    def mound(self, x0, x1, z0, z1, height, bsdf, group=0, nu=4, nv=3):
        pts, uv, nrm, faces = [], [], [], []
        for j in range(nv + 1):
            for i in range(nu + 1):
                u, v = i / nu, j / nv; y = height * np.sin(np.pi * u) * np.sin(np.pi * v)
                dydx = height * np.pi / (x1 - x0) * np.cos(np.pi * u) * np.sin(np.pi * v); dydz = height * np.pi / (z1 - z0) * np.sin(np.pi * u) * np.cos(np.pi * v)
                nn = np.array([-dydx, 1.0, -dydz]); nn /= np.linalg.norm(nn)
                pts.append((x0 + (x1 - x0) * u, y, z0 + (z1 - z0) * v)); uv.append((u, v)); nrm.append(tuple(map(float, nn)))
        for j in range(nv):
            for i in range(nu):
                a = j * (nu + 1) + i; faces += [(a, a + nu + 1, a + 1), (a + 1, a + nu + 1, a + nu + 2)]
        return self.add(pts, faces, bsdf, uv=uv, normals=nrm, group=group)

    def room(self, lo, hi, bsdf, light_bsdf, emitters, S):
        """a closed box of plain quads WITHOUT texture coordinates, facing inward, and a small light under its ceiling"""
        (x0, y0, z0), (x1, y1, z1) = lo, hi
        for q in ([(x0, y0, z0), (x0, y0, z1), (x1, y0, z1), (x1, y0, z0)], [(x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1)], [(x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1)],
                  [(x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0)], [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)], [(x0, y0, z1), (x0, y1, z1), (x1, y1, z1), (x1, y0, z1)]):
            self.add(q, [(0, 1, 2), (0, 2, 3)], bsdf)
        y = y1 - 0.05; si = self.add([(-0.5, y, -0.5), (0.5, y, -0.5), (0.5, y, 0.5), (-0.5, y, 0.5)], [(0, 1, 2), (0, 2, 3)], light_bsdf, emitter=len(emitters))
        emitters.append(dict(type=S.EMITTER_AREA, shape=si, radiance=(10.0, 10.0, 10.0), weight=1.0))


def _constant_bitmap(S, rgb, filter_type):
    base = np.ascontiguousarray(np.tile(np.asarray(rgb, f32), (4, 4, 1)))
    return S.make_texture(S.TEXTURE_BITMAP, pyramid=dict(base=base, levels=[(4, 4, base.reshape(-1).copy())], wrapped=True), filter_type=filter_type)


def _finish(S, M, bsdfs, emitters, tex, name, **kw):
    cam = S.look_at((0.0, 3.0, -5.5), (0.0, 0.5, 0.0), (0, 1, 0))
    return S.finish_scene(M.verts, M.tris, M.shapes, bsdfs, emitters, cam, 50.0, 0.05, 100.0, 32, 32, 1, S.SAMPLER_SOBOL, 4, 3, normals=M.nrm, uvs=M.uv, name=name, textures=tex, **kw)


def surface_scene_instanced(S):
    """A shape group -- three UV-mapped quads and a smooth-shaded UV-mapped mound -- instanced three times (identity, rotation, rotation with non-uniform scale) inside
    a plain room without texture coordinates.  The members carry a bitmap-textured diffuse (EWA), a bump map over a bitmap-textured diffuse (bilinear), a normal map
    and a mask over the bump map: the `inst >= 0` branch of the tangent selection with every kind of record that needs tangents."""
    pyr = S.load_texture_pyramid(); nimg = S.normal_map_image()
    tex = [S.make_texture(S.TEXTURE_BITMAP, pyramid=pyr, uscale=2.0, vscale=1.5, uoffset=0.1, filter_type=S.MIP_EWA),
           S.make_texture(S.TEXTURE_BITMAP, pyramid=pyr, uscale=1.5, vscale=2.0, voffset=0.05, filter_type=S.MIP_BILINEAR),
           S.make_texture(S.TEXTURE_BITMAP, pyramid=dict(base=nimg, levels=S.build_mip_pyramid(nimg, S.WRAP_REPEAT, S.WRAP_REPEAT)), uscale=1.5, vscale=1.0, filter_type=S.MIP_BILINEAR)]
    B = []
    def add(**kw): B.append(S.make_bsdf(**kw)); return len(B) - 1
    d_ewa = add(reflectance=(0.5, 0.5, 0.5)); B[d_ewa]["texture"] = 0
    d_bil = add(reflectance=(0.5, 0.5, 0.5)); B[d_bil]["texture"] = 1
    bump = add(kind=S.BSDF_BUMPMAP, nested=d_bil, texture=1, scale=0.25)
    plain = add(reflectance=(0.6, 0.55, 0.5)); nmap = add(kind=S.BSDF_NORMALMAP, nested=plain, texture=2)
    mask = add(kind=S.BSDF_MASK, reflectance=(0.55, 0.6, 0.7), nested=bump)
    wall = add(reflectance=(0.7, 0.7, 0.7)); light = add(reflectance=(0.5, 0.5, 0.5))
    M = _Meshes(); emitters = []
    M.room((-6, -2, -6), (6, 6, 6), wall, light, emitters, S)
    M.quad(-1.6, -0.9, -0.5, 0.5, d_ewa, group=1); M.quad(-0.8, -0.1, -0.5, 0.5, bump, group=1, uv=((0, 0), (0, 0.7), (1.3, 0.9), (1.1, 0.1))); M.quad(0.9, 1.6, -0.5, 0.5, mask, group=1)
    M.mound(0.0, 0.8, -0.5, 0.5, 0.3, nmap, group=1)
    inst = [S.make_instance(0, S.translate(0.0, 0.0, 0.0)), S.make_instance(0, S.translate(0.5, 2.0, 2.5) @ S.rotate((1, 0, 0), -55.0)),
            S.make_instance(0, S.translate(2.5, 2.5, -2.0) @ S.rotate((0, 1, 1), 40.0) @ S.scale(1.3, 0.7, 1.1))]
    return _finish(S, M, B, emitters, tex, "surface_units_instanced", instances=inst)


def surface_scene_edges(S):
    """Quads in a row, one record each: bump maps of scale 0, -1 and 1e4 over a bitmap-textured diffuse, a bump map whose displacement uses the nearest filter (zero
    gradient), normal maps that are constant (0.5, 0.5, 1) (the unperturbed normal), (0.5, 0.5, 0.5) (a zero normal) and (0.5, 0.5, 0) (a normal in the tangent plane), a
    bump-mapped triangle whose three texture coordinates coincide, a coating over a textured diffuse, an axis-aligned textured sphere (its poles: dpdu = 0), inside a
    plain room without texture coordinates."""
    pyr = S.load_texture_pyramid()
    tex = [S.make_texture(S.TEXTURE_BITMAP, pyramid=pyr, uscale=2.0, vscale=1.5, uoffset=0.1, filter_type=S.MIP_EWA),
           S.make_texture(S.TEXTURE_BITMAP, pyramid=pyr, uscale=1.5, vscale=2.0, voffset=0.05, filter_type=S.MIP_BILINEAR),
           S.make_texture(S.TEXTURE_BITMAP, pyramid=pyr, uscale=1.5, vscale=2.0, filter_type=S.MIP_NEAREST)] + [_constant_bitmap(S, c, S.MIP_NEAREST) for c in CONSTANT_NORMALS]      # nearest: the texel itself (the bilinear weights of a constant do not always add up to 1)
    B = []
    def add(**kw): B.append(S.make_bsdf(**kw)); return len(B) - 1
    d_ewa = add(reflectance=(0.5, 0.5, 0.5)); B[d_ewa]["texture"] = 0
    d_bil = add(reflectance=(0.5, 0.5, 0.5)); B[d_bil]["texture"] = 1
    plain = add(reflectance=(0.6, 0.55, 0.5))
    recs = [add(kind=S.BSDF_BUMPMAP, nested=d_bil, texture=1, scale=s) for s in BUMP_SCALES] + [add(kind=S.BSDF_BUMPMAP, nested=d_bil, texture=2, scale=0.25)]
    recs += [add(kind=S.BSDF_NORMALMAP, nested=plain, texture=3 + i) for i in range(3)]
    degenerate = add(kind=S.BSDF_BUMPMAP, nested=d_bil, texture=1, scale=0.25)
    coat = add(kind=S.BSDF_COATING, nested=d_ewa, reflectance=(0.1, 0.2, 0.3), scale=0.5, ior=1.5)
    wall = add(reflectance=(0.7, 0.7, 0.7)); light = add(reflectance=(0.5, 0.5, 0.5))
    M = _Meshes(); emitters = []
    M.room((-6, -2, -6), (6, 6, 6), wall, light, emitters, S)
    for i, r in enumerate(recs + [coat]): M.quad(-4.0 + i, -3.1 + i, -0.5, 0.5, r)
    M.shapes[-3]["aim_weight"] = 0.5                                                 # the zero normal: every output of its cases is NaN; surface_inputs aims at it half as often
    M.add([(-4.0, 0, 1.0), (-4.0, 0, 2.0), (-3.0, 0, 2.0)], [(0, 1, 2)], degenerate, uv=[(0.3, 0.3)] * 3)
    ball = S.make_analytic(S.SHAPE_SPHERE, S.translate(0.0, 1.0, 2.5), d_ewa, radius=0.5)
    return _finish(S, M, B, emitters, tex, "surface_units_edges", analytic=[ball])


def surface_scenes(golden_scenes, S):
    if "surface" not in _LIGHT_REF:
        _LIGHT_REF["surface"] = {**{k: golden_scenes[k] for k in SURFACE_SCENES}, "surface_units_instanced": surface_scene_instanced(S), "surface_units_edges": surface_scene_edges(S)}
    return _LIGHT_REF["surface"]


def chain(sc, m):
    """the records the surface step walks from record m: mask -> bumpmap / normalmap -> coating -> leaf"""
    out = [m]
    for kinds in ((9,), (11, 12), (17, 19)):
        if sc.bsdfs[out[-1]]["type"] in kinds: out.append(int(sc.bsdfs[out[-1]]["distr"]))
    return out


def chain_textures(sc, m):
    return [sc.textures[sc.bsdfs[r]["texture"]] for r in chain(sc, m) if sc.bsdfs[r].get("texture", -1) >= 0]


def surface_no_libm(sc, m, differentials):
    """no_libm extended over the chain: the leaf calls no math-library routine (a coating's absorption calls exp), and no texture on the chain is looked up through the
    trilinear or EWA filter (logarithm, atan / sin / cos), which only a hit with differentials does"""
    c = chain(sc, m)
    return no_libm(sc, c[-1]) and not any(sc.bsdfs[r]["type"] in (17, 19) for r in c) and not (differentials and any(t["type"] == 2 and t["filter"] >= 2 for t in chain_textures(sc, m)))


def _frame(n):
    a = np.where(np.abs(n[:, :1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]])); s = np.cross(n, a); s /= np.linalg.norm(s, axis=1, keepdims=True)
    return s, np.cross(n, s)


EDGE_BARYCENTRICS = [(0, 0), (1, 0), (0, 1), (0.5, 0.5), (0.5, 0), (0, 0.5), (0.25, 0), (0, 0.75), (0.125, 0.875)]      # (b1, b2): the vertices and points on the three edges


def surface_inputs(name, sc):
    """rays8 [n, 8], diff6 [n, 6], and what each case was aimed at: `target` (-1 - a: analytic shape a, else the mesh shape), `instance`, `kind` ("" plain, "edge",
    "texel", "graze"), `diff_kind` ("", "perpendicular", "nonfinite") and the differential scale"""
    n = N_SURFACE_UNIT if name in SURFACE_UNIT_SCENES else N_SURFACE; rng = np.random.default_rng([zlib.crc32(name.encode()), 4242])
    pos = sc.pos.astype(np.float64); lo, hi = scene_box(sc); size = float(np.linalg.norm(hi - lo))
    entries = [(si, -1) for si, sh in enumerate(sc.shapes) if not sh.get("group", 0)]
    entries += [(si, ii) for ii, ins in enumerate(sc.instances) for si, sh in enumerate(sc.shapes) if sh.get("group", 0) == ins["group"] + 1]
    entries += [(-1 - a, -1) for a in range(len(sc.analytic))]
    weight = np.asarray([sc.shapes[e].get("aim_weight", 1.0) if e >= 0 else 1.0 for e, _ in entries]); weight = np.cumsum(weight) / weight.sum()
    P = np.zeros((n, 3)); N = np.zeros((n, 3)); target = np.zeros(n, np.int64); instance = np.full(n, -1); kind = np.array([""] * n, dtype=object)
    special = rng.integers(0, 8, n)                                                 # 0: edges, vertices, seams, poles, centres; 1: texel edges of the bound bitmap
    for i in range(n):
        e, ii = entries[min(int(np.searchsorted(weight, rng.uniform(), side="right")), len(entries) - 1)]; target[i] = e; instance[i] = ii
        if e >= 0:
            sh = sc.shapes[e]; t = sh["first_tri"] + int(rng.integers(0, sh["tri_count"])); i0, i1, i2 = (int(v) for v in sc.idx[t])
            r1, r2 = rng.uniform(size=2); b1, b2 = np.sqrt(r1) * (1 - r2), np.sqrt(r1) * r2
            if special[i] == 0: b1, b2 = EDGE_BARYCENTRICS[rng.integers(0, len(EDGE_BARYCENTRICS))]; kind[i] = "edge"
            bitmaps = [tx for tx in chain_textures(sc, sh["bsdf"]) if tx["type"] == 2]
            if special[i] == 1 and sh.get("has_uv", 0) and sc.uv is not None and bitmaps:
                # a target uv whose texture-space u (or v) lies on a level-0 texel edge (an integer multiple of 1 / w: the wrap seam when it is a multiple of w), one float32 ulp either side included
                tx = bitmaps[0]; w0, h0 = (int(v) for v in sc.texture_levels[tx["first_level"]][:2]); t0, t1, t2 = (sc.uv[j].astype(np.float64) for j in (i0, i1, i2))
                uv = t0 * (1 - b1 - b2) + t1 * b1 + t2 * b2; ax = int(rng.integers(0, 2)); sz, sca, off = ((w0, tx["uscale"], tx["uoffset"]), (h0, tx["vscale"], tx["voffset"]))[ax]
                k = np.round((uv[ax] * sca + off) * sz); k = np.round(k / sz) * sz if rng.uniform() < 0.25 else k
                u32 = f32((k / sz - off) / sca); u32 = [np.nextafter(u32, f32(-1e9)), u32, np.nextafter(u32, f32(1e9))][rng.integers(0, 3)]; uv[ax] = float(u32)
                A = np.stack([t1 - t0, t2 - t0], 1)
                if abs(np.linalg.det(A)) > 1e-12:
                    c1, c2 = np.linalg.solve(A, uv - t0)
                    if c1 >= 0 and c2 >= 0 and c1 + c2 <= 1: b1, b2 = c1, c2; kind[i] = "texel"
            p = pos[i0] * (1 - b1 - b2) + pos[i1] * b1 + pos[i2] * b2; fn = np.cross(pos[i1] - pos[i0], pos[i2] - pos[i0])
            if ii >= 0:
                m = np.asarray(sc.instances[ii]["to_world"], np.float64).reshape(4, 4); p = m[:3, :3] @ p + m[:3, 3]; fn = np.linalg.inv(m[:3, :3]).T @ fn
        else:
            a = sc.analytic[-1 - e]; m = np.asarray(a["to_world"], np.float64).reshape(4, 4); sp = special[i] == 0
            if sp: kind[i] = "edge"
            if a["type"] in (0, 1):                                                 # rectangle: its edges and corners; disk: its centre and rim
                # (next to a rim, not on it: where it is another shape's rim as well, which of the two a ray meets is a tie no side defines)
                if a["type"] == 0: x, y = rng.uniform(-1, 1, 2) if not sp else np.asarray([(-1, 0.3), (1, -1), (0, 1), (0, 0)][rng.integers(0, 4)], np.float64)
                else:
                    r = np.sqrt(rng.uniform()) if not sp else [0.0, 0.999, 0.5][rng.integers(0, 3)]; ph = rng.uniform(0, 2 * np.pi) if not sp else [0.0, np.pi, 0.5 * np.pi][rng.integers(0, 3)]
                    x, y = r * np.cos(ph), r * np.sin(ph)
                pl = np.array([x, y, 0.0]); nl = np.array([0.0, 0.0, 1.0])
            else:                                                                   # sphere: seam and poles; cylinder: seam, next to its rims
                ph = rng.uniform(0, 2 * np.pi) if not sp or rng.uniform() < 0.3 else 0.0
                if a["type"] == 2:
                    th = np.arccos(rng.uniform(-1, 1)) if not sp else [0.0, np.pi, 0.5 * np.pi, 1e-4][rng.integers(0, 4)]
                    nl = np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)]); pl = nl * a["radius"]
                else:
                    z = rng.uniform(0, 1) if not sp else [0.001, 0.999, 0.5][rng.integers(0, 3)]
                    nl = np.array([np.cos(ph), np.sin(ph), 0.0]); pl = nl * a["radius"] + np.array([0.0, 0.0, z * a["length"]])
            p = m[:3, :3] @ pl + m[:3, 3]; fn = np.linalg.inv(m[:3, :3]).T @ nl
        P[i] = p; N[i] = fn / max(np.linalg.norm(fn), 1e-300)
    # origins on a hemisphere around the target: a quarter with incidence cosines out of EDGE_Z, a quarter of all cases from the back side
    cz = rng.uniform(0.05, 1.0, n); graze = rng.uniform(size=n) < 0.25; cz = np.where(graze, np.asarray(EDGE_Z)[rng.integers(0, len(EDGE_Z), n)], cz); kind[graze & (kind == "")] = "graze"
    ph = rng.uniform(0, 2 * np.pi, n); sn = np.sqrt(np.maximum(0.0, 1 - cz * cz)); s, t = _frame(N); side = np.where(rng.uniform(size=n) < 0.75, 1.0, -1.0)
    w = s * (sn * np.cos(ph))[:, None] + t * (sn * np.sin(ph))[:, None] + N * (cz * side)[:, None]
    # the poles of an axis-aligned sphere are met exactly only along its axis
    for i in range(n):
        if target[i] < 0 and kind[i] == "edge" and sc.analytic[-1 - target[i]]["type"] == 2 and abs(abs(N[i, 2]) - 1.0) < 1e-12:
            a = sc.analytic[-1 - target[i]]; w[i] = np.round(N[i]); P[i] = np.asarray(a["to_world"], np.float64).reshape(4, 4)[:3, 3] + w[i] * a["radius"]
    o = (P + w * (rng.uniform(0.03, 0.12, n) * size)[:, None]).astype(f32); d = P - o.astype(np.float64); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    rays = np.zeros((n, 8), f32); rays[:, 0:3] = o; rays[:, 3] = MI_EPSILON; rays[:, 4:7] = d; rays[:, 7] = np.inf
    # differentials: the spacing of the scene's own camera pixels around d, scaled as RayDifferential::scaleDifferential does
    delta = 2.0 * np.tan(np.radians(sc.xfov) / 2) / sc.width; d64 = d.astype(np.float64); ds, dt = _frame(d64)
    rx = d64 + ds * delta; rx /= np.linalg.norm(rx, axis=1, keepdims=True); ry = d64 + dt * delta; ry /= np.linalg.norm(ry, axis=1, keepdims=True)
    scale = np.asarray(DIFF_SCALES)[rng.integers(0, len(DIFF_SCALES), n)]
    rxd = d64 + (rx - d64) * scale[:, None]; ryd = d64 + (ry - d64) * scale[:, None]
    r = rng.integers(0, 16, n); diff_kind = np.array([""] * n, dtype=object)
    perp = r == 0; which = rng.uniform(size=n) < 0.5; tang = np.cross(N, d64); diff_kind[perp] = "perpendicular"      # prx == 0: no differential at all, or one in the tangent plane
    rxd[perp & which] = 0.0; ryd[perp & ~which] = np.where(np.abs(N[perp & ~which]) == 1.0, 0.0, tang[perp & ~which])
    bad = r == 1; diff_kind[bad] = "nonfinite"; col = rng.integers(0, 3, n); val = np.asarray([np.nan, np.inf, -np.inf])[rng.integers(0, 3, n)]
    rxd[bad, col[bad]] = val[bad]
    diff = np.ascontiguousarray(np.concatenate([rxd, ryd], 1), f32)
    return dict(rays=rays, diff=diff, target=target, instance=instance, kind=kind, diff_kind=diff_kind, scale=scale)


_SURF_REF = {}


def surface_reference(oracle, golden_scenes, S, name):
    """the inputs of scene `name` and the oracle's answers, computed once: dict(sc, inp, query (the 2-D samples + extra values), wo_world, and per run -- "record" and
    "sample" with differentials, "record_plain" and "eval" without -- (out, branches))"""
    if name not in _SURF_REF:
        sc = surface_scenes(golden_scenes, S)[name]; orc = oracle.Oracle(sc); inp = surface_inputs(name, sc); n = len(inp["rays"]); b = bsdf_inputs(name, 0)
        query = np.ascontiguousarray(np.concatenate([b["uv"][:n], b["extra"][:n, None]], 1), f32)
        runs = {"record": orc.surface_units("record", inp["rays"], inp["diff"]), "record_plain": orc.surface_units("record", inp["rays"]),
                "sample": orc.surface_units("sample", inp["rays"], inp["diff"], query)}
        # eval directions: bsdf_inputs' wo in the hit's frame, every fourth case the oracle's own sample (of the run without differentials) where it is non-zero -- in world space
        rec = runs["record_plain"][0]; sampled = orc.surface_units("sample", inp["rays"], None, query)[0]; wo = eval_wo(dict(wo=b["wo"][:n]), sampled)
        took = (wo != b["wo"][:n]).any(1) & (rec[:, 19] != 0)                           # a sample of a bumped record lives in the perturbed frame
        fs = np.where(took[:, None], rec[:, 25:28], rec[:, 45:48]); ft = np.where(took[:, None], rec[:, 28:31], rec[:, 48:51]); fn = np.where(took[:, None], rec[:, 31:34], rec[:, 42:45])
        with np.errstate(invalid="ignore"): wo_world = np.ascontiguousarray(fs * wo[:, 0:1] + ft * wo[:, 1:2] + fn * wo[:, 2:3], f32)
        wo_world[~np.isfinite(wo_world).all(1)] = (0.0, 1.0, 0.0)
        runs["eval"] = orc.surface_units("eval", inp["rays"], None, wo_world)
        _SURF_REF[name] = dict(sc=sc, inp=inp, query=query, wo_world=wo_world, runs=runs)
    return _SURF_REF[name]


def hit_records(sc, record):
    """per case of a mode-0 record [n, 51]: the material record at the head of the hit's chain (-1: a miss) -- from the primitive the oracle or the device reports"""
    prim = record[:, 40].astype(np.int64); nt = len(sc.idx); miss = (record[:, 18:22] == 0).all(1) & (record[:, 37] == 0)
    shape_bsdf = np.asarray([s["bsdf"] for s in sc.shapes] + [a["bsdf"] for a in sc.analytic], np.int64)
    shape = np.where(prim < nt, sc.tri_shape[np.minimum(prim, nt - 1)].astype(np.int64), len(sc.shapes) + prim - nt)
    return np.where(miss, -1, shape_bsdf[shape])


def zero_normal_records(sc):
    """records whose chain holds a normal map that is (0.5, 0.5, 0.5) everywhere: the perturbed normal is normalize(0)"""
    out = set()
    for m in range(len(sc.bsdfs)):
        for r in chain(sc, m):
            b = sc.bsdfs[r]
            if b["type"] == 12:
                t = sc.textures[b["texture"]]
                if t["type"] == 2:
                    w, h, off = (int(v) for v in sc.texture_levels[t["first_level"]])
                    if (sc.texture_texels[off:off + w * h * 3] == f32(0.5)).all(): out.add(m)
    return out
