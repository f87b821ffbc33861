"""CPU: the inputs of the device's unit-level comparisons (tests/unit_inputs.py, tests/test_gpu_units.py) and the oracle exports they go through.  These checks keep
the device test from passing vacuously: the new exports agree with the pinned ones, the inputs reach every lobe and every branch of the texture lookup, no lookup's
EWA loops are long, and three properties of the lookups hold without going through the oracle's arithmetic."""
import glob
import os
import numpy as np
import pytest
from tests.conftest import GOLDEN
from tests import unit_inputs as U


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


UNIT_FILES = sorted(os.path.basename(p)[:-len("_units.npz")] for p in glob.glob(os.path.join(GOLDEN, "*_units.npz")))


@pytest.mark.parametrize("name", UNIT_FILES)
def test_sample_ex_equals_sample(oracle, golden_scenes, name):
    """orc_bsdf_sample_ex(..., 0.5) is orc_bsdf_sample -- the export test_units_vs_reference pins to the compiled reference -- bit for bit, on that test's own rows"""
    sc = golden_scenes[name]; rows = np.load(os.path.join(GOLDEN, name + "_units.npz"))["bsdf"]; orc = oracle.Oracle(sc); L = oracle.lib()
    o8 = np.zeros(8, np.float32); n = 0
    for row in rows:
        si = int(row[0]); mat = sc.shapes[si]["bsdf"] if si < len(sc.shapes) else sc.analytic[si - len(sc.shapes)]["bsdf"]
        wi = np.ascontiguousarray(row[1:4], np.float32)
        L.orc_bsdf_sample(orc.h, mat, wi.ctypes.data, float(row[4]), float(row[5]), o8.ctypes.data)
        ex = orc.bsdf_sample_units(mat, wi, row[4:6], [0.5])[0]
        assert (bits(ex[:8]) == bits(o8)).all(), (mat, row[1:6], ex, o8)
        assert ex[8] in (0.0, 1.0, 2.0) and ex[9] in (0.0, 1.0)
        if not U.children(sc, mat): assert ex[9] == float(sc.bsdfs[mat]["type"] == 5)      # a plain record: roughdielectric alone asks its sampler for one more value
        n += 1
    assert n > 0


@pytest.mark.parametrize("name", U.BSDF_SCENES)
def test_bsdf_census(oracle, golden_scenes, name):
    """conditions on the INPUTS, measured on the oracle alone: per record at least 0.35 of the sample cases carry a weight and at least 0.20 of the eval cases a value
    (types that are nothing but Dirac deltas evaluate to zero everywhere and are exempt).  A record that misses a floor asks for other inputs, not another floor."""
    sc = golden_scenes[name]; ref = U.bsdf_reference(oracle, golden_scenes, name)
    assert ref, "no record of this scene reaches the unit entry point"
    for m, r in ref.items():
        s_share = float((r["sampled"][:, :3] != 0).any(1).mean()); e_share = float((r["evald"][:, :3] != 0).any(1).mean())
        print(f"[census] {name} record {m} ({U.TYPE_NAMES[sc.bsdfs[m]['type']]}): sample {s_share:.3f} eval {e_share:.3f}")
        if U.black(sc, m): continue                                     # zero whatever the inputs: compared on the device all the same
        assert s_share >= 0.35, (name, m, s_share)
        if not U.zero_eval(sc, m): assert e_share >= 0.20, (name, m, e_share)


def test_texture_table(mi):
    """the table is what the device test needs it to be: every filter with every wrap mode on each axis, never the same mode on both"""
    sc = U.texture_scene(mi.scenes); tex = sc.textures[:U.N_BITMAPS]
    assert len(sc.textures) == 26 and all(t["type"] == 2 for t in tex) and tuple(sc.texture_levels[0][:2]) == (48, 40)
    for f in range(4):
        mine = [t for t in tex if t["filter"] == f]
        assert len(mine) == 5 and {t["wrap_u"] for t in mine} == {0, 1, 2, 3, 4} == {t["wrap_v"] for t in mine} and all(t["wrap_u"] != t["wrap_v"] for t in mine)
    assert all(np.isfinite([t["uscale"], t["vscale"], t["uoffset"], t["max_anisotropy"]]).all() for t in sc.textures)


def test_texture_census(mi, oracle):
    """orc_texture_last_info: every branch of the lookup is taken by at least 1 % of the lookups of a filter that can reach it, the pole cases go where defined
    comparisons send them, and no lookup's EWA loops visit more than 16384 texels -- asserted here, before anything is launched on a device"""
    sc, orc, per = U.texture_reference(oracle, mi.scenes); B = orc.TEXTURE_BRANCHES
    info = {f: np.concatenate([per[t]["info"] for t in range(U.N_BITMAPS) if sc.textures[t]["filter"] == f]) for f in range(4)}
    share = lambda f, name: float(((info[f][:, 0] & B[name]) != 0).mean())
    reach = {"nearest": [0], "bilinear": [1], "trilinear": [2], "degenerate": [3], "level_negative": [2], "ewa_clamped": [3], "ewa_unclamped": [3], "ewa_to_bilinear": [3],
             "level_past_pyramid": [2, 3]}
    for name, filters in reach.items():
        for f in filters:
            print(f"[texture-census] {name} under {U.FILTER_NAMES[f]}: {share(f, name):.4f}")
            assert share(f, name) >= 0.01, (name, f, share(f, name))
    print(f"[texture-census] ewa_zero_denominator under ewa: {share(3, 'ewa_zero_denominator'):.4f}; level_negative under ewa: {share(3, 'level_negative'):.4f}")
    assert share(0, "nearest") == 1.0 and share(1, "bilinear") == 1.0 and share(2, "trilinear") == 1.0
    # the routes of k_env_primary at the poles (zero, equal, NaN, inf and overflowing partials): the trilinear branch, level < 0, a level-0 bilinear lookup
    for t in range(U.N_BITMAPS):
        if sc.textures[t]["filter"] >= 2:
            b = per[t]["info"][:60, 0]; pole = ~np.isin(np.arange(60) % 6, (1, 2))
            assert ((b[pole] & (B["trilinear"] | B["degenerate"])) != 0).all() and ((b[pole] & B["level_negative"]) != 0).all(), (t, b)
            # (a footprint of rank one -- second pair zero, or two equal pairs -- leaves F = A C - B^2 / 4 at a rounding error of either sign: any branch, but like every lookup a level that is a number)
    levels = np.concatenate([p["info"][:, 1] for p in per.values()])
    assert levels.min() >= -160 and levels.max() <= 64, (levels.min(), levels.max())      # log2 of a finite positive float: no float-to-int conversion out of range on either side
    texels = np.concatenate([p["info"][:, 2] for p in per.values()]); dropped = float(np.mean([(~p["keep"]).mean() for p in per.values()]))
    print(f"[texture-census] most texels visited by one lookup: {texels.max()}; dropped from the device run: {dropped:.5f}")
    assert texels.max() <= U.MAX_EWA_TEXELS and dropped <= 0.001


def texture_properties(lookup, sc, keep=None):
    """three checks that do not go through the oracle's arithmetic, on `lookup(t, uv, partials_or_None) -> [n, 3]` (the oracle here, the device in test_gpu_units;
    keep: per record the lookups whose EWA loops the census found short -- a device is given no others)"""
    rng = np.random.default_rng(99)
    # 1. nearest and bilinear lookups at level-0 texel centres return the stored texel exactly
    for f in (0, 1):
        t = f * 5 + 2; tx = sc.textures[t]; uv, xy = U.texel_centres(sc, t); w, h, off = (int(v) for v in sc.texture_levels[tx["first_level"]])
        assert len(uv) >= 0.9 * w * h
        stored = sc.texture_texels[off:off + w * h * 3].reshape(h, w, 3)[xy[:, 1], xy[:, 0]]
        for pa in (None, np.zeros((len(uv), 4), np.float32), rng.uniform(-1, 1, (len(uv), 4)).astype(np.float32)):
            assert (bits(lookup(t, uv, pa)) == bits(stored)).all(), (t, pa is None)
    # 2. nearest lookups over all five wrap modes against the index rule of TMIPMap::evalTexel restated in numpy
    for t in range(5):
        tx = sc.textures[t]; uv, pa = U.texture_inputs(sc, t); w, h, off = (int(v) for v in sc.texture_levels[tx["first_level"]])
        uvx = uv[:, 0] * np.float32(tx["uscale"]) + np.float32(tx["uoffset"]); uvy = uv[:, 1] * np.float32(tx["vscale"]) + np.float32(tx["voffset"])
        x = np.floor(uvx * np.float32(w)).astype(np.int64); y = np.floor(uvy * np.float32(h)).astype(np.int64)
        want = U.nearest_rule(x, y, tx["wrap_u"], tx["wrap_v"], sc.texture_texels[off:off + w * h * 3].reshape(h, w, 3))
        for p in (pa, None):
            assert (bits(lookup(t, uv, p)) == bits(want)).all(), (t, p is None)
    # 3. the constant-colour bitmap returns its colour under every filter and every footprint
    for t in U.TEX_CONSTANT:
        uv, pa = U.texture_inputs(sc, t)
        if keep is not None: uv, pa = uv[keep[t]], pa[keep[t]]
        for p in (pa, None):
            assert np.abs(lookup(t, uv, p) - np.asarray(U.CONSTANT_COLOR, np.float32)).max() <= 1e-6, (t, p is None)


def test_texture_properties_oracle(mi, oracle):
    sc, orc, per = U.texture_reference(oracle, mi.scenes)
    texture_properties(lambda t, uv, pa: orc.texture_units(t, uv, pa), sc)


# ------------------------------------------------------------------------------------------------ emitters
LIGHT_ALL = U.LIGHT_SCENES + U.UNIT_LIGHT_SCENES
SPOT_ZONES = ["spot_outside", "spot_outside", "spot_transition", "spot_transition", "spot_beam", "spot_beam"]      # one ulp below, on, one ulp above: the cut-off cosine (<=), then the beam cosine (>=)


def scene_branches(sc, name):
    """the branches of orc_emitter_sample_units a scene has, from its emitter list"""
    kinds = {e["type"] for e in sc.emitters}; want = set()
    if any(e["type"] == 0 and e["shape"] < len(sc.shapes) for e in sc.emitters): want.add("area_mesh")
    analytic = [sc.analytic[e["shape"] - len(sc.shapes)] for e in sc.emitters if e["type"] == 0 and e["shape"] >= len(sc.shapes)]
    if analytic: want.add("area_analytic")
    if any(a["type"] == 2 for a in analytic): want |= {"sphere_cone", "sphere_whole"}
    if 1 in kinds: want |= {"envmap", "env_missed_sphere", "env_near", "env_far"}
    # a sample of zero value: the tent warp reaches one texel beyond the chosen one, which is black only in the unit maps (the row with a single texel)
    if name in U.UNIT_LIGHT_SCENES: want.add("env_zero_value")
    if 2 in kinds: want |= {"constant", "constant_normal", "constant_no_normal", "constant_zero_value", "env_missed_sphere", "env_near", "env_far"}
    if 3 in kinds: want.add("point")
    if 4 in kinds: want |= {"spot", "spot_outside", "spot_beam", "spot_transition"}
    if 5 in kinds: want |= {"directional", "directional_behind"}
    if 7 in kinds: want.add("collimated")
    return want


@pytest.mark.parametrize("name", LIGHT_ALL)
def test_emitter_census(mi, oracle, golden_scenes, name):
    """conditions on the INPUTS of the emitter comparisons, measured on the oracle alone: every branch the scene has is taken by at least 1 % of the sampling cases, at
    least 0.2 of them carry a value, no case makes env_pdf_direction form a non-finite texel coordinate, and the points aimed at a spot light's cones hit the stored
    cosines exactly (the zones flip between the neighbours the comparisons `<=` and `>=` say).  env_zero_pdf is exempt: a sample has zero density only where its value
    is zero, and that term comes first."""
    r = U.light_reference(oracle, golden_scenes, mi.scenes, name); sc = r["sc"]; s = r["sample"]; B = oracle.Oracle.EMITTER_BRANCHES; br = s["branches"]
    share = {k: float(((br & v) != 0).mean()) for k, v in B.items()}; want = scene_branches(sc, name)
    value = float((s["out"][:, :3] != 0).any(1).mean())
    print(f"[emitter-census] {name}: value {value:.3f}; " + ", ".join(f"{k} {share[k]:.4f}" for k in B if share[k] > 0))
    assert {k for k in B if share[k] > 0} - {"env_zero_value", "env_zero_pdf"} <= want, (name, share)
    for k in sorted(want): assert share[k] >= 0.01, (name, k, share[k])
    assert value >= 0.2, (name, value)
    assert share["envpdf_non_finite"] == 0 and np.isfinite(s["inp"]["ref"]).all() and np.isfinite(s["inp"]["uv"]).all()
    assert (s["inp"]["uv"] >= 0).all() and (s["inp"]["uv"] <= np.float32(U.ONE_MINUS)).all() and (s["inp"]["ref_n"][::5] == 0).all()
    for special in (0.0, U.ONE_MINUS, U.TWO_M32):
        for col in (0, 1): assert (s["inp"]["uv"][:, col] == np.float32(special)).mean() >= 0.03, (name, special, col)      # one in sixteen each (u = 0 gives some up in the unit scenes)
    if "spot" in want:
        t = s["inp"]["spot_target"]; spot = (br & B["spot"]) != 0
        for j, zone in enumerate(SPOT_ZONES):
            mine = spot & (t == j); assert mine.sum() >= 8 and ((br[mine] & B[zone]) != 0).all(), (name, j, zone, int(mine.sum()))
    # the raw form: the same record, the value not yet divided by the selection probability
    lit = s["out"][:, 10] != 0; raw = s["raw"]
    assert (bits(raw[:, 3:16]) == bits(s["out"][:, 3:16]))[lit].all() and (raw[lit, 16] > 0).all() and (bits(raw[lit, :3] * (np.float32(1) / raw[lit, 16:17])) == bits(s["out"][lit, :3])).all()
    for e, ev in r["eval"].items():
        vs = float((ev["out"][:, :3] != 0).any(1).mean()); ps = float((ev["out"][:, 3] != 0).mean())
        print(f"[emitter-census] {name} eval emitter {e} ({U.EMITTER_KIND_NAMES[sc.emitters[e]['type']]}): value {vs:.3f} density {ps:.3f}")
        assert ((ev["branches"] & B["envpdf_non_finite"]) == 0).all() and all(np.isfinite(ev["inp"][k]).all() for k in ("ref", "d", "n", "dist"))
        assert vs >= 0.2 and (ps >= 0.2 or sc.emitters[e]["type"] == 2), (name, e, vs, ps)
        if sc.emitters[e]["type"] == 0 and e in [i for i, em in enumerate(sc.emitters) if em["shape"] >= len(sc.shapes) and sc.analytic[em["shape"] - len(sc.shapes)]["type"] == 2]:
            for k in ("sphere_cone", "sphere_whole"): assert ((ev["branches"] & B[k]) != 0).mean() >= 0.01, (name, e, k)


def test_emitter_units_equal_pinned_export(mi, oracle, golden_scenes):
    """orc_emitter_sample_units is orc_sample_emitter_direct -- the export test_oracle_golden pins to the compiled reference -- bit for bit wherever that one's
    visibility test lets the sample through"""
    L = oracle.lib(); o12 = np.zeros(12, np.float32); seen = 0
    for name in U.LIGHT_SCENES:
        r = U.light_reference(oracle, golden_scenes, mi.scenes, name); inp = r["sample"]["inp"]; out = r["sample"]["out"]; orc = oracle.Oracle(r["sc"])
        for i in range(0, U.N_LIGHT, 16):
            L.orc_sample_emitter_direct(orc.h, inp["ref"][i].ctypes.data, inp["ref_n"][i].ctypes.data, float(inp["uv"][i, 0]), float(inp["uv"][i, 1]), o12.ctypes.data)
            if not o12[:3].any(): continue
            assert (bits(o12[:11]) == bits(out[i, :11])).all(), (name, i, o12, out[i]); seen += 1
    assert seen > 200


def test_light_unit_scenes(mi):
    """the unit scenes are what the comparisons need: a zero-area triangle in the middle (8 x 4: at the head) of a light mesh of three and of one of five triangles, the selection table
    0, 0.5, 0.75, 1, maps without a black row, one row with a single texel, row guide tables with more buckets than bins for the odd sizes"""
    for (w, h), name in zip(U.ENV_SIZES, U.UNIT_LIGHT_SCENES):
        sc = U.light_scene(mi.scenes, w, h); assert sc.name == name and U.emitter_cdf(sc).tolist() == [0.0, 0.5, 0.75, 1.0]
        for (e, ts), count, middle in zip(U._mesh_lights(sc), (3, 5), (0, 0) if (w, h) == U.ENV_SIZES[1] else (1, 2)):
            area = np.linalg.norm(np.cross(ts[:, 1] - ts[:, 0], ts[:, 2] - ts[:, 0]), axis=1); assert len(ts) == count and area[middle] == 0 and (np.delete(area, middle) > 0).all()
        rgb = sc.envmap["rgb"]; assert rgb.shape == (h, w, 3) and (rgb.sum((1, 2)) > 0).all() and ((rgb[U.SINGLE_TEXEL_ROW] != 0).any(1).sum() == 1)
        kr, kc = U.guide_buckets(w, h); assert kr >= h and (kr > h or h & (h - 1) == 0)
    assert U.guide_buckets(5, 3) == (4, 2) and U.guide_buckets(64, 32) == (32, 16) and U.guide_buckets(1024, 512) == (512, 256)


# ------------------------------------------------------------------------------------------------ participating media
MEDIUM_ALL = U.MEDIUM_SCENES + ["medium_units"]


def medium_branches(med):
    """the branches of medium_sample_distance a record can take.  A weight of 1 always chooses the medium, and then no distance it can draw leaves less than 1e-20 of
    the thinnest channel (-log(2^-24) = 16.6 mean free paths at most); a channel with sigma_t = 0 keeps its transmittance at 1; the single strategy on such a channel
    draws an infinite distance every time"""
    st = np.asarray(med["sigma_a"], np.float32) + np.asarray(med["sigma_s"], np.float32); w = med["medium_sampling_weight"]; want = {"chosen", "beyond"}
    if w < 1: want.add("not_chosen")
    if med["strategy"] == 0: want |= {"channel_0", "channel_1", "channel_2"}
    if not (med["strategy"] == 1 and med["sampling_density"] == 0): want |= {"success", "p_equals_o"}
    if w < 1 and st.min() > 0: want.add("cut")
    return want


@pytest.mark.parametrize("name", MEDIUM_ALL)
def test_medium_census(mi, oracle, golden_scenes, name):
    """conditions on the INPUTS of the medium comparisons, measured on the oracle alone: every branch of medium_sample_distance a record can take is taken by at least
    1 % of its cases; the values drawn are what the strategy says; the transmittance cases reach 0, 1 and what lies between"""
    r = U.medium_reference(oracle, golden_scenes, mi.scenes, name); B = oracle.Oracle.MEDIUM_BRANCHES; assert r["records"]
    for m, per in r["records"].items():
        med = r["sc"].media[m]; br = per["distance"]["branches"]; share = {k: float(((br & v) != 0).mean()) for k, v in B.items()}; want = medium_branches(med)
        print(f"[medium-census] {name} record {m} (strategy {med['strategy']}, weight {med['medium_sampling_weight']:.3g}, g {med['g']:.3g}): " + ", ".join(f"{k} {v:.3f}" for k, v in share.items()))
        assert {k for k in B if share[k] > 0} <= want | {"cut"}, (name, m, share)
        for k in sorted(want): assert share[k] >= 0.01, (name, m, k, share[k])
        out = per["distance"]["out"]; chosen = (br & B["chosen"]) != 0
        assert (out[:, 10] == np.where(chosen & (med["strategy"] == 0), 2.0, 1.0)).all() and (out[:, 0] == ((br & B["success"]) != 0)).all()
        t = per["transmittance"]["out"][:, :3]; assert (t == 0).any() and (t == 1).any() and ((t > 0.01) & (t < 0.99)).any() and not np.isnan(t).any()
        assert np.isfinite(per["phase_sample"]["out"][:, :4]).all() and np.isfinite(per["phase_eval"]["out"][:, 0]).all()
        assert (np.abs(np.linalg.norm(per["phase_sample"]["out"][:, :3].astype(np.float64), axis=1) - 1) < 1e-2).all()      # (a sanity check only: at |g| = 0.999 the map's cosTheta cancels and may pass 1 by some 1e-4, in the reference too)
    if name == "medium_units":
        media = r["sc"].media; assert sorted({round(md["g"], 7) for md in media if md["phase"] == 1}) == sorted(round(float(np.float32(g)), 7) for g in U.HG_G)
        assert {md["strategy"] for md in media} == {0, 1, 2} and {md["medium_sampling_weight"] for md in media} >= {1.0, 0.5, 2.0 ** -10, U.FLT_MIN}
        assert any(min(a + b for a, b in zip(md["sigma_a"], md["sigma_s"])) == 0 for md in media)
